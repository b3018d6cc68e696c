// bandplan.hpp — the planner of the single-launch plan (bandnet_kernels.hip): which nodes of a graph become stages of ONE launch behind the
// first convolution, in which order, on which workgroups, where their tensors live in LDS and in the launch's workspace, and the packed
// constants and 20-dword descriptors the kernel reads.  Pure host code: nothing here calls the HIP runtime, so the planner can be run, hashed
// and sanitised without a GPU (tests/bandplan_dump.cpp, tests/asan_lowering.cpp).  The engine uploads `prog` and `consts` as they are.
#pragma once

#include <string>
#include <vector>

#include "plan.hpp"

namespace mi {

struct BandOptions {
    int nw = 128;        // most workgroups per frame
    bool wide = true;    // stages of more than 128 channels (false: the program ends in front of the first one)
    bool fork = true;    // the second branch behind a fork, and the output heads, on the idle workgroups
    int cu_count = 0;    // compute units of the device the program will run on (the planner never asks the runtime)
};
struct BandExt { int out_k = -1, tensor = -1; };   // BandLaunch::base[2 + j]: graph output out_k, or the arena storage of `tensor` (read by a launch behind the band program)
struct BandPlan {
    bool ready = false;             // the graph has a single-launch form
    std::string why;                // where the planner gave up ("bandplan.cpp:123"), empty when ready
    int first = 0;                  // node of the batched plan the band launch stands for (with every node behind it that node_runs does not name)
    int stem_out = -1;              // tensor the first convolution writes = the band program's input
    int nw = 0, max_frames = 0;     // workgroups per frame of the program that was built; frames one launch takes
    int nstages = 0, lds_bytes = 0;
    int tiles_floats = 0, dw_floats = 0;   // LDS floats of the program's tiles / of the largest depthwise result
    long ws_frame_floats = 0;       // workspace floats per frame (packet buffers and far copies)
    bool cv2 = false, xb = false, wide = false;   // the kernel instantiation (BandLaunch)
    std::vector<BandExt> ext;
    std::vector<char> node_runs;    // per node of the batched plan from `first` on: 1 = it runs as its own launch behind the band launch
    std::vector<BandPacked> prog;   // as uploaded
    std::vector<float> consts;      // as uploaded (with its 64 floats of slack)
};

// plan: the batched plan of the handle (its arena layout final); level2: the level-2 lowering of the same graph (one node per BlazeBlock /
// convolution), from which the stages are made.  A graph without a single-launch form gives ready = false; a constant tensor shorter than
// the layer that reads it throws std::runtime_error.  MI_BAND_DEBUG=1 prints the nodes, the stages and the give-up location.
BandPlan build_band_plan(const Plan& plan, const Plan& level2, const BandOptions& o);

}  // namespace mi
