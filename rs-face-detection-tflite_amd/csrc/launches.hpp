// launches.hpp — a chunk of frames lowered to the ordered list of kernel launches that runs it: which kernel every plan node takes (or which
// launch in front of it swallows it), the filled argument struct, the stream it runs on and the events around it.  Pure host code: nothing
// here calls the HIP runtime — pointers are values that are offset and compared, never dereferenced — so the selection can be run, hashed
// and sanitised without a GPU (tests/launches_dump.cpp, tests/asan_lowering.cpp).  The engine walks the list and issues it.
#pragma once

#include <string>
#include <variant>
#include <vector>

#include "bandplan.hpp"
#include "consts.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace mi {

constexpr int kHeadStreams = 4;  // most side streams for output heads that run beside the trunk (option "heads")

// Which nodes of a plan run beside the trunk (per node): the side stream of a forked node (-1: the trunk), the node whose completion it waits
// for (-1: the start of the plan), and whether a forked node waits for this one
struct SideSchedule {
    std::vector<int> slot, wait;
    std::vector<char> event_after;
};
SideSchedule schedule_side_streams(const Plan& plan, int head_streams);

// Everything the lowering reads that is not the plan: device addresses as plain values, the chunk, the options the selection depends on
struct LaunchCtx {
    const float* weights = nullptr;      // the constants blob (PlanConsts offsets)
    float* arena = nullptr;              // the arena region of the lane this chunk runs on
    const float* in = nullptr;           // frame 0 of the run's input
    float* const* out = nullptr;         // per graph output: frame 0 of the run's output buffer
    float* small = nullptr;              // small-batch scratch of the row-pipelined chains, and its size
    size_t small_floats = 0;
    const ResStage* progs = nullptr;     // stage programs (PlanConsts::node_prog)
    const TailStage* tail_progs = nullptr;
    const BandPacked* band_prog = nullptr;   // the single-launch plan: program, constants, workspace, sync words, fail word
    const float* band_consts = nullptr;
    float* band_ws = nullptr;
    unsigned* band_sync = nullptr;
    int* band_fail = nullptr;
    int chunk_cap = 0, chunk_start = 0, F = 0;   // frames the arena is laid out for; first frame and frames of this chunk
    const uint8_t* u8_frames = nullptr;  // u8 input form (null: f32)
    const float* u8_lut = nullptr;
    long u8_frame_bytes = 0;
    int u8_row_bytes = 0;
    // options (engine.cpp, find_option)
    int strip = 1, pair_fuse = 1, stem_fuse = 1, stem_mfma = 1, stem_run = 0, mchain = 1, small_chain = 16, lanes = 1;
    int conv_mfma = 1;
    int conv_bf16 = 0;                   // 1 / 2: the convolutions conv_mfma_kernel has a form for take conv_bf16_kernel (the constants were packed with the same value)
    int pipe_rows = 0, pipe_band = 0, mdb_band = 0, tail_pre = 0, tail_g = 0;
    bool fork = true;                    // nodes of the side schedule leave the trunk (false: everything in line, no events)
    int cu_count = 256;
    bool band = false;                   // this chunk takes the single-launch plan
    int band_test_absent = 0;
};

enum class Launcher {  // one per launch_* entry point (kernels.hpp); SmallChain: launch_strip / launch_block once per block of `blocks`; Act with EltArgs::shift: launch_affine
    Conv, HeadGemm, Dw, Xc, Mdblock, Dblock, Mbneck, Bneck, Tail, Resident, Chain, StripPipe, SmallChain, Ms2, Mwalk, MstripChain, Strip, Mstrip, Block,
    Add, Act, Maxpool, Padc, Resize2x, DepthToSpace, Bandnet, Avgpool, L2norm, Transpose
};

struct Launch {
    Launcher to = Launcher::Conv;
    std::variant<ConvArgs, HeadGemmArgs, DwArgs, XcArgs, DblockArgs, BneckArgs, TailLaunch, ResLaunch, ChainArgs, BlockArgs, EltArgs, BandLaunch> args;
    std::vector<BlockArgs> blocks;  // StripPipe, SmallChain, MstripChain: one per block (args is unused)
    int node = -1, last = -1;       // first and last plan node the launch stands for
    int slot = -1;                  // side stream (-1: the trunk)
    int wait = -1;                  // on a side stream: node whose launch it waits for (-1: whatever the trunk held before this plan)
    bool record = false;            // a launch on a side stream waits for this one
    std::string label;              // kernel name as profile() reports it (only when asked for)
};

struct Lowered {
    std::vector<Launch> launches;
    std::vector<int> launch_of_node;  // per plan node: the launch that stands for it (-1: a view)
};
Lowered lower_chunk(const Plan& plan, const PlanConsts& consts, const BandPlan& band_plan, const SideSchedule& sched, const LaunchCtx& ctx, bool want_labels);

// where tensor t of the chunk lives (its first frame; the floats between frames in *frame_stride): an output buffer or the arena
float* tensor_ptr_mut(const Plan& plan, const LaunchCtx& ctx, int t, long* frame_stride);

// a run on the single-launch plan: node i of the batched plan is inside the band launch (at band_plan.first: it is that launch)
bool band_cut(const BandPlan& band_plan, size_t i);
// ... and the launches such a run makes in all (the band launch and every node that keeps its own)
int band_run_launches(const Plan& plan, const BandPlan& band_plan);

// u8 frames can stand for the graph input: it is read by one node only, and that node is the specialised stem convolution (conv_takes_u8)
bool takes_u8_input(const Plan& plan, const PlanConsts& consts);

}  // namespace mi
