// consts.hpp — every constant the launches of a plan read, packed into one blob on the host, and the stage programs resolved
// against it.  Pure host code: nothing here calls the HIP runtime, so the layouts can be run, hashed and sanitised without a GPU
// (tests/consts_dump.cpp, tests/asan_lowering.cpp).  The engine uploads `blob` and the two programs as they are.
#pragma once

#include <cstdint>
#include <vector>

#include "plan.hpp"

namespace mi {

// float offsets into the blob of one member's constants (-1: none)
struct MemberOff {
    long w = -1, b = -1, w2 = -1, b2 = -1, alpha = -1;
    long strip = -1;    // Chain member: strip_pack_consts / strip_pack_consts_s2 (row pipelines)
    long cblob = -1;    // xc stage, first block of a dblock / bneck pair: the small constants as the kernel copies them to LDS
    long mconsts = -1;  // second block of a dblock / bneck pair: the pair's operand-layout constants (mdblock_pack_consts / mbneck_pack_consts)
};

struct PlanConsts {
    std::vector<float> blob;  // host image of the device blob; the engine frees it after the upload
    // per node: float offsets into the blob (-1 none)
    std::vector<long> node_w, node_b, node_w2, node_b2, node_alpha;
    std::vector<long> node_pair;        // pair launch this Block node and the next one share (mdblock_pack_consts, pair form)
    std::vector<long> node_wrows;       // Conv node with a conv_mfma_kernel form (conv_mfma_shape_ok): the filter [Co][KH*KW*C] as stored; Affine node: node_w = scale, node_b = shift
    // Conv node with node_wrows, packed with conv_bf16 != 0 (-1 otherwise): that filter rounded to bf16, two values a float slot (element 2 j in the
    // low half of slot j), Co * K / 2 floats a plane: `hi` = rne_bf16(w), and with conv_bf16 == 2 `lo` = rne_bf16(w - hi) (conv_bf16_kernel's B operand)
    std::vector<long> node_wbf16_hi, node_wbf16_lo;
    std::vector<long> node_stem;        // the first convolution inside the launch of the block pair behind it (mdblock_pack_stem)
    std::vector<long> node_mwalk;       // Block node: mwalk_pack_consts, or ms2_pack_consts for a stride-2 block (a node is one or the other)
    std::vector<long> node_chain_pair;  // Chain node of two plain blocks on a wide layer: mdblock_pack_consts, pair form
    std::vector<long> node_strip;       // Block node: strip_pack_consts / mstrip_pack_consts
    std::vector<std::vector<MemberOff>> chain_off;       // per node, per member
    std::vector<std::vector<MemberOff>> chain_head_off;  // per node, per head pair: stacked weights (w2) and bias (b2)
    std::vector<std::vector<long>> res_wblk;   // per Resident node, per stage: K-blocked weight packing (-1: classic order)
    std::vector<std::vector<long>> res_cblob;  // per Resident node, per stage: its small constants (-1: LOAD)
    std::vector<std::vector<long>> tail_wa, tail_wc;  // per tail node, per stage: A operands / small constants (-1: LOAD)
    // stage programs of the Resident nodes: pointer-free descriptors, resolved against ResBases at launch
    std::vector<ResStage> progs;
    std::vector<TailStage> tail_progs;  // ... of the nodes that run on tail_kernels.hip (Node::tail)
    std::vector<long> node_prog;        // per node: its first stage in progs / tail_progs (-1 none)
};

// plan.root_offset is final when this is called (the stage programs carry arena offsets).  conv_bf16: engine option "conv_bf16"; 0 packs no
// bf16 plane, and 1 / 2 append theirs behind everything else: every other offset, and the blob up to there, is the same at all three values
PlanConsts pack_plan_consts(const Plan& plan, int conv_bf16 = 0);

// f32 -> bf16, round to nearest even, as the device's v_cvt_pk_bf16_f32 rounds a finite value: (u + 0x7fff + ((u >> 16) & 1)) >> 16 on the bit pattern u
uint16_t bf16_rne(float v);
float bf16_to_float(uint16_t h);

// constant tensor t, of which the caller reads the first `need` floats: the only way the packers (consts.cpp, bandplan.cpp) read a constant.
// A tensor that does not exist or is shorter than that (the model is untrusted) throws std::runtime_error
const std::vector<float>& const_data(const Graph& g, int t, long need = 0);

// negative-side slope of channel c behind m's activation: PReLU alpha, 1 without an activation, 0 for ReLU / ReLU6
float act_slope(const Graph& g, const Node& m, int c);

}  // namespace mi
