// bandplan.cpp — see bandplan.hpp.
//
// The single-launch plan (bandnet_kernels.hip) is made from the level-2 lowering of the graph — one node per BlazeBlock / convolution — when
// that is: a first convolution (which keeps its launch of the batched plan), then nothing but 3x3 BlazeBlocks whose skip is their own input
// (or, without a stride, another tensor of the program: the iris network's bottlenecks), pointwise blocks, 1x1 convolutions and 2x2 stride-2
// convolutions, each reading the tensor of an earlier one.  The program stops in front of the first node that is none of these (the face
// mesh's and the iris network's two whole-frame convolutions): the plan nodes from there on keep their launches of the batched plan, behind
// the band launch, and the tensors they read are written to their arena storage by the band program — provided no launch of the batched plan
// straddles the cut.  Graphs whose FIRST block is already something else leave the plan not ready and the handle on the batched plan.
// The passes are the member functions of Planner, in the order Planner::run calls them.
#include "bandplan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <stdexcept>

#include "consts.hpp"

namespace mi {
namespace {

struct GiveUp { int line; };   // the graph has no single-launch form (a decision, not an error): BandPlan::why names the line
#define BAND_GIVE_UP throw GiveUp{__LINE__}

bool debug() { return std::getenv("MI_BAND_DEBUG") != nullptr; }
long align_up(long v, long a) { return (v + a - 1) / a * a; }
bool is_view(const Node& n) { return n.kind == Node::Reshape || n.kind == Node::Concat; }

// rows [Co][C] -> the A operands of v_mfma_f32_16x16x4_f32, per 16-channel output tile (BandStage::w_a)
std::vector<float> pack_a_operands(const std::vector<float>& wsrc, int Co, int C, int per_ct) {
    const int nct = (Co + 15) / 16, n16 = C / 16, has8 = (C / 8) & 1, has4 = (C / 4) & 1;
    std::vector<float> A(static_cast<size_t>(nct) * per_ct, 0.f);
    for (int ct = 0; ct < nct; ct++)
        for (int l = 0; l < 64; l++) {
            const int o = 16 * ct + (l & 15), kq = l >> 4;
            if (o >= Co) continue;
            for (int j = 0; j < n16; j++)
                for (int e = 0; e < 4; e++) A[static_cast<size_t>(ct) * per_ct + (j * 64 + l) * 4 + e] = wsrc[static_cast<size_t>(o) * C + 16 * j + 4 * kq + e];
            if (has8)
                for (int e = 0; e < 2; e++) A[static_cast<size_t>(ct) * per_ct + n16 * 256 + l * 2 + e] = wsrc[static_cast<size_t>(o) * C + 16 * n16 + 2 * kq + e];
            if (has4) A[static_cast<size_t>(ct) * per_ct + n16 * 256 + has8 * 128 + l] = wsrc[static_cast<size_t>(o) * C + 16 * n16 + 8 * has8 + kq];
        }
    return A;
}

// [bias 16 nct][slope 16 nct], then for a BLOCK [taps 9 C][depthwise bias C] (BandStage::w_c)
std::vector<float> pack_small_consts(const Graph& g, const Node& n, bool dw_block, int C, int Co) {
    const int nct = (Co + 15) / 16, bt = n.kind == Node::Conv ? n.b : n.b2;
    std::vector<float> cb(static_cast<size_t>(32 * nct + (dw_block ? 10 * C : 0)), 0.f);
    if (bt >= 0) std::copy_n(const_data(g, bt, Co).begin(), Co, cb.begin());
    if (n.act == ACT_PRELU) const_data(g, n.alpha, Co);
    for (int c = 0; c < Co; c++) cb[static_cast<size_t>(16 * nct + c)] = act_slope(g, n, c);
    if (dw_block) {
        std::copy_n(const_data(g, n.w, 9L * C).begin(), 9 * C, cb.begin() + 32 * nct);   // [1][3][3][C]
        if (n.b >= 0) std::copy_n(const_data(g, n.b, C).begin(), C, cb.begin() + 32 * nct + 9 * C);
    }
    return cb;
}

struct Planner {
    const Plan& plan;     // the batched plan
    const Plan& p2;       // the level-2 lowering
    const BandOptions& o;
    const bool conv2_ok;  // 2x2 stride-2 convolutions are stages (false: the program ends in front of the first one)
    const Graph& g = p2.graph;
    BandPlan bp;
    bool saw_conv2 = false;
    int NW = 0;
    size_t i2 = 0;                      // the first convolution in p2
    std::vector<BandStage> prog;
    std::vector<float> consts;
    std::vector<int> producer, out_root;   // per tensor: the stage that writes it (-1: none); per graph output: the root of its storage in p2
    std::vector<char> band_op;          // .tflite operators the band program computes
    size_t cut = 0;                     // first p2 node the program does not take
    std::vector<int> last_reader;       // per stage: the last stage that reads its LDS tile (-1: nobody does)
    int input_last_reader = -1;         // ... the program's input
    long ws = 0;                        // workspace floats per frame

    int ext_slot(int out_k, int tensor) {   // BandLaunch::base index of a graph output / an arena tensor (-1: no slot left)
        for (size_t j = 0; j < bp.ext.size(); j++)
            if (bp.ext[j].out_k == out_k && bp.ext[j].tensor == tensor) return 2 + static_cast<int>(j);
        if (2 + bp.ext.size() >= static_cast<size_t>(kBandBases)) return -1;
        BandExt e; e.out_k = out_k; e.tensor = tensor;
        bp.ext.push_back(e);
        return 1 + static_cast<int>(bp.ext.size());
    }
    long put(const std::vector<float>& v) {
        const long off = align_up(static_cast<long>(consts.size()), 64);
        consts.resize(static_cast<size_t>(off) + v.size(), 0.f);
        std::copy(v.begin(), v.end(), consts.begin() + off);
        return off;
    }
    bool is_graph_output(int t) const {   // (its storage in the batched plan is a graph-output buffer)
        for (int go : g.outputs)
            if (plan.storage[static_cast<size_t>(go)].root == plan.storage[static_cast<size_t>(t)].root) return true;
        return false;
    }
    // prog becomes its stages in `order`; pos[k] = the new index of stage k
    void reorder(const std::vector<int>& order, const std::vector<int>& pos) {
        std::vector<BandStage> re;
        for (size_t k = 0; k < order.size(); k++) {
            BandStage st = prog[static_cast<size_t>(order[k])];
            if (st.dep >= 0) st.dep = pos[static_cast<size_t>(st.dep)];
            if (st.res_dep >= 0) st.res_dep = pos[static_cast<size_t>(st.res_dep)];
            if (st.dep >= static_cast<int>(k) || st.res_dep >= static_cast<int>(k)) BAND_GIVE_UP;   // (cannot happen: a stage only moves to behind what it reads)
            re.push_back(st);
        }
        prog.swap(re);
    }
    std::vector<char> stages_read() const {   // per stage: some stage reads its output
        std::vector<char> read(prog.size(), 0);
        for (const BandStage& st : prog) {
            if (st.dep >= 0) read[static_cast<size_t>(st.dep)] = 1;
            if (st.res_dep >= 0) read[static_cast<size_t>(st.res_dep)] = 1;
        }
        return read;
    }
    // ---- the first launch of both plans must be the same convolution; workgroups per frame
    void stem() {
        size_t i5 = 0;
        while (i5 < plan.nodes.size() && is_view(plan.nodes[i5])) i5++;
        while (i2 < p2.nodes.size() && is_view(p2.nodes[i2])) i2++;
        if (i5 >= plan.nodes.size() || i2 >= p2.nodes.size()) BAND_GIVE_UP;
        const Node &stem5 = plan.nodes[i5], &stem2 = p2.nodes[i2];
        if (stem5.kind != Node::Conv || stem2.kind != Node::Conv || stem5.out != stem2.out || stem5.gemm_head) BAND_GIVE_UP;
        bp.stem_out = stem2.out;
        if (plan.storage[bp.stem_out].root != bp.stem_out || plan.storage[bp.stem_out].offset != 0) BAND_GIVE_UP;
        bp.first = static_cast<int>(i5) + 1;
        while (bp.first < static_cast<int>(plan.nodes.size()) && is_view(plan.nodes[static_cast<size_t>(bp.first)])) bp.first++;
        if (bp.first >= static_cast<int>(plan.nodes.size())) BAND_GIVE_UP;
        // workgroups per frame: one per row of the first tensor, at most o.nw (the bands of the later, smaller tensors are one row of every
        // 2nd, 4th ... workgroup)
        const auto& stem_shape = g.tensors[bp.stem_out].shape;
        if (stem_shape.size() != 4) BAND_GIVE_UP;
        NW = o.nw;
        while (NW > 1 && (stem_shape[1] % NW) && (NW % stem_shape[1])) NW--;
        if (stem_shape[1] < NW) NW = stem_shape[1];
        bp.nw = NW;
        bp.max_frames = NW > 0 ? std::max(0, o.cu_count / NW) : 0;
        if (bp.max_frames < 1) BAND_GIVE_UP;
    }
    // ---- one stage per node: its shape, bands, source and constants
    void stages() {
        producer.assign(g.tensors.size(), -1);
        for (int t : g.outputs) out_root.push_back(p2.storage[t].root);
        band_op.assign(g.ops.size(), 0);
        cut = p2.nodes.size();
        for (size_t i = i2 + 1; i < cut; i++)
            if (!is_view(p2.nodes[i]) && !stage_of(p2.nodes[i], i)) cut = i;   // the program ends in front of node i
        if (prog.empty() || prog.size() > 63) BAND_GIVE_UP;
    }
    // the stage of node n, or false: n is none (the program ends in front of it when it has stages already, else there is none)
    bool stage_of(const Node& n, size_t i) {
        const bool pw_block = n.kind == Node::Block && n.w < 0;
        const bool dw_block = n.kind == Node::Block && n.w >= 0;
        const bool conv1 = n.kind == Node::Conv && n.KH == 1 && n.KW == 1 && n.sh == 1 && n.sw == 1 && !n.gemm_head;
        const bool conv2 = conv2_ok && n.kind == Node::Conv && n.KH == 2 && n.KW == 2 && n.sh == 2 && n.sw == 2 && !n.gemm_head && n.in.size() == 1 &&
                           g.tensors[n.in[0]].shape.size() == 4 && g.tensors[n.in[0]].shape[1] % 2 == 0 && g.tensors[n.in[0]].shape[2] % 2 == 0 &&
                           g.tensors[n.in[0]].shape[3] % 32 == 0 && n.in[0] != bp.stem_out;
        if (debug())
            std::fprintf(stderr, "bandnet: node %zu kind %d K %dx%d s %d in %zu res %d mode %d after %d ept %d act %d gemm %d\n", i, static_cast<int>(n.kind), n.KH, n.KW, n.sh, n.in.size(), n.res, n.res_mode,
                         n.res_after ? 1 : 0, n.ept, n.act, n.gemm_head ? 1 : 0);
        if (!pw_block && !dw_block && !conv1 && !conv2) return false;
        // (2x2 stride-2 convolutions and the blocks behind them, whose skip is the 2x2 max of the convolution's input, are stages too: the whole
        // iris network but its two whole-frame heads is one program.  Should a graph with such nodes have no program with them, it is planned
        // once more with the program ending in front of the first of them: build_band_plan)
        if (conv2) saw_conv2 = true;
        // full_range's lateral convolutions — a 1x1 convolution with a fused activation, then ADD with the bilinearly up-sampled coarser map: the skip
        // joins BEHIND the activation — are stages of the WIDE instantiation when the coarse tensor is the program's; any other such node ends the program
        const bool up2x = (conv1 || pw_block) && n.res_after && n.res >= 0 && n.res_mode == RES_UP2X && o.wide && n.in.size() == 1 && n.ept < 0 &&
                          producer[static_cast<size_t>(n.res)] >= 0 && g.tensors[n.res].shape.size() == 4;
        // (full_range_sparse pads its stride-2 blocks explicitly, one pixel in front: the same stage with its window one row / column earlier)
        const bool pre = dw_block && n.ept == 1 && n.epl == 1 && n.sh == 2 && n.sw == 2 && n.padding == Padding::Valid && n.res < 0 && o.wide;
        if (n.in.size() != 1 || (n.ept >= 0 && !pre) || (n.res_after && !up2x)) return false;
        const auto& si = g.tensors[n.in[0]].shape;
        const auto& so = g.tensors[n.out].shape;
        if (si.size() != 4 || so.size() != 4) BAND_GIVE_UP;
        BandStage st;
        st.kind = dw_block ? BAND_BLOCK : BAND_PW;
        st.H = si[1]; st.W = si[2]; st.C = si[3]; st.Ho = so[1]; st.Wo = so[2]; st.Co = so[3];
        const bool wide_ok = o.wide && !conv2 && st.C <= 384 && st.Co <= 384 && (st.C <= 128 || st.C % 16 == 0) && (st.Co <= 128 || st.Co % 16 == 0);   // (the WIDE instantiation)
        // channel counts the kernel does not take (a wave keeps ONE 16-channel output tile and at most eight 16-value chunks of A operands): full_range
        // without wide stages is the trunk down to 12x12x36
        if (st.C % 4 || st.C < 8 || st.Co < 1 || ((st.C > 128 || st.Co > 128) && !wide_ok)) return false;
        if (dw_block) {
            if (n.KH != 3 || n.KW != 3 || n.sh != n.sw || (n.sh != 1 && n.sh != 2) || (n.padding != Padding::Same && !pre)) BAND_GIVE_UP;
            st.S = n.sh;
            st.pre = pre ? 1 : 0;
            if (st.S == 2 && ((st.H & 1) || (st.W & 1))) BAND_GIVE_UP;
            if (st.Ho != st.H / st.S || st.Wo != st.W / st.S) BAND_GIVE_UP;
        } else if (conv2) {
            st.S = 2;   // (even sizes: SAME and VALID are the same window)
            if (st.Ho != st.H / 2 || st.Wo != st.W / 2 || n.res >= 0) BAND_GIVE_UP;
        } else if (st.Ho != st.H || st.Wo != st.W) {
            BAND_GIVE_UP;
        }
        st.act = n.act;
        if (n.act != ACT_NONE && n.act != ACT_RELU && n.act != ACT_RELU6 && n.act != ACT_PRELU) BAND_GIVE_UP;
        if (up2x) {
            const auto& sr = g.tensors[n.res].shape;
            const BandStage& cd = prog[static_cast<size_t>(producer[static_cast<size_t>(n.res)])];
            if (sr[1] * 2 != st.Ho || sr[2] * 2 != st.Wo || sr[3] != st.Co || (st.Co & 3) || cd.R != 1 || (st.Wo / 2) * (st.Co / 4) > 512) return false;
            st.res_mode = RES_UP2X;
            st.res_dep = producer[static_cast<size_t>(n.res)];   // (its rows come through the packets, not from a tile: readers())
            st.res_c = st.Co;
        } else if (n.res >= 0) {
            if (!dw_block) BAND_GIVE_UP;
            if (n.res != n.in[0] && n.res_mode == RES_MAXPOOL) {
                // the skip is the 2x2 max of the tensor the 2x2 convolution in front of this block read: the rows 2r, 2r + 1 of it that the
                // owner of output row r needs are in the LDS tile that convolution read them from
                const auto& sr = g.tensors[n.res].shape;
                const int d = producer[static_cast<size_t>(n.in[0])];
                // (... or the stride-2 BLOCK in front — full_range's down-sampling pairs: DW s2 + PW reduce, then DW + PW expand + 2x2 max of the
                // pair's input, zero-padded from its res_c channels to Co)
                if (st.S != 1 || sr.size() != 4 || sr[1] != 2 * st.Ho || sr[2] != 2 * st.Wo || sr[3] > st.Co || (sr[3] & 3) || d < 0) BAND_GIVE_UP;
                const BandStage& cv = prog[static_cast<size_t>(d)];
                if (cv.S != 2 || cv.pre || cv.dep < 0 || cv.dep != producer[static_cast<size_t>(n.res)]) BAND_GIVE_UP;
                st.res_dep = cv.dep;
                st.res_mode = RES_MAXPOOL;
                st.res_c = sr[3];
            }
            else if (n.res != n.in[0]) {
                // the skip is another tensor of the program, with the output's shape (its rows then have the output's owners)
                const auto& sr = g.tensors[n.res].shape;
                if (n.res_mode != RES_DIRECT || st.S != 1 || sr.size() != 4 || sr[1] != st.Ho || sr[2] != st.Wo || sr[3] > st.Co || (sr[3] & 3)) BAND_GIVE_UP;   // (fewer channels than Co: zero-padded)
                st.res_c = sr[3];
                if (n.res == bp.stem_out) st.res_dep = -1;
                else if (producer[static_cast<size_t>(n.res)] >= 0) st.res_dep = producer[static_cast<size_t>(n.res)];
                else BAND_GIVE_UP;
                st.res_mode = RES_DIRECT;
            }
            else if (n.res_mode == RES_DIRECT && st.S == 1 && st.Co >= st.C) st.res_mode = RES_DIRECT;   // (Co > C: the skip is zero-padded to Co channels)
            else if (n.res_mode == RES_MAXPOOL && st.S == 2 && st.Co >= st.C) st.res_mode = RES_MAXPOOL;
            else BAND_GIVE_UP;
        }
        // bands: whole rows per workgroup while there are at least NW rows, one row for every (NW / rows)-th workgroup below that
        auto log2_exact = [](int v) { int k = 0; while ((1 << k) < v) k++; return (1 << k) == v ? k : -1; };
        if (st.Ho >= NW) {
            if (st.Ho % NW) BAND_GIVE_UP;
            st.R = st.Ho / NW; st.wshift = 0; st.nbands = NW;
        } else {
            if (st.Ho < 1 || NW % st.Ho || log2_exact(NW / st.Ho) < 0) BAND_GIVE_UP;
            st.R = 1; st.wshift = log2_exact(NW / st.Ho); st.nbands = st.Ho;
        }
        if (n.in[0] == bp.stem_out) {
            st.src_base = 1; st.src_off = 0; st.dep = -1; st.Rin = 0;
            st.src_fs = plan.storage[bp.stem_out].frame_stride;
            if (st.src_fs & 3) BAND_GIVE_UP;
        } else {
            const int d = producer[static_cast<size_t>(n.in[0])];
            if (d < 0) BAND_GIVE_UP;
            const BandStage& pd = prog[static_cast<size_t>(d)];
            st.dep = d;
            st.Rin = pd.R;
            // the owner of output row r must own input row S r, and the rows it lacks must be at most one above and two below its own
            for (int b = 0; b < st.nbands; b++) {
                const int r0 = b * st.R, nro = std::min(st.Ho, r0 + st.R) - r0, p0 = st.S * r0;
                if (((p0 / pd.R) << pd.wshift) != (b << st.wshift) || p0 % pd.R) BAND_GIVE_UP;
                const int rin = std::min(pd.R, st.H - p0);
                const int yb = dw_block ? (st.S == 1 ? p0 + nro + 1 : p0 + 2 * nro + 1 - st.pre) : (conv2 ? p0 + 2 * nro : p0 + nro);
                const int below = yb - (p0 + rin);
                if (below < 0 || below > 2) BAND_GIVE_UP;
                if (((dw_block && (st.S == 1 || st.pre) ? 1 : 0) + below) * st.W * (st.C / 4) > 4 * 512) BAND_GIVE_UP;   // the halo rows: four 16-byte elements per lane
            }
        }
        // a plain copy of the output where it is a graph output (through the reshape / concatenation views behind it)
        const Storage& so_st = p2.storage[n.out];
        for (size_t k = 0; k < out_root.size(); k++)
            if (out_root[k] == so_st.root) {
                st.dst_base = ext_slot(static_cast<int>(k), -1); st.dst_off = so_st.offset; st.dst_fs = so_st.frame_stride;
                if (st.dst_base < 0) BAND_GIVE_UP;
            }
        if (st.dst_base < 0 && so_st.root != n.out) BAND_GIVE_UP;
        if (st.dst_base < 0 && st.Co % 4) BAND_GIVE_UP;
        if ((st.dst_off & 3) || (st.dst_fs & 3)) {
            if (st.Co % 4 == 0) BAND_GIVE_UP;   // 16-byte stores need the alignment; the ragged heads store floats
        }
        // constants
        const int C = conv2 ? 4 * st.C : st.C;   // (the contraction length: [Co][2][2][C] read as [Co][4 C])
        const int nct = (st.Co + 15) / 16;
        st.per_ct = C / 16 * 256 + ((C / 8) & 1) * 128 + ((C / 4) & 1) * 64;
        st.c_floats = bandnet_const_floats(st);   // (what the kernel stages in LDS: without the depthwise taps where they do not fit — a wide stage reads them from L2)
        if (nct > 24 || (nct > 8 && !wide_ok)) BAND_GIVE_UP;
        st.wpc_shift = nct == 1 ? 3 : (nct == 2 ? 2 : (nct <= 4 ? 1 : 0));
        st.w_a = put(pack_a_operands(const_data(g, n.kind == Node::Conv ? n.w : n.w2, static_cast<long>(st.Co) * C), st.Co, C, st.per_ct));
        st.w_c = put(pack_small_consts(g, n, dw_block, C, st.Co));
        auto magic = [](int d) { return d <= 1 ? 0u : static_cast<unsigned>((0x100000000ull + static_cast<unsigned long long>(d) - 1) / static_cast<unsigned long long>(d)); };
        st.mC4 = magic(st.C / 4); st.mWo = magic(st.Wo); st.mrowq = magic(st.W * (st.C / 4));
        if (static_cast<long>(st.R + 3) * st.W * (st.C / 4) >= 65536 || st.R * st.Wo * std::max(st.C, st.Co) / 4 >= 65536) BAND_GIVE_UP;   // the magic divisions' range
        producer[static_cast<size_t>(n.out)] = static_cast<int>(prog.size());
        prog.push_back(st);
        for (int op : n.src_ops) band_op[static_cast<size_t>(op)] = 1;
        return true;
    }
    // ---- the cut: a plan node behind the first convolution either lies wholly inside the band program (the band launch stands for it) or wholly
    // behind it (it keeps its launch); a tensor such a launch reads from the program is written to its arena storage by the producing stage.
    // Then: every graph output is written, whole
    void cut_against_batched_plan() {
        bp.node_runs.assign(plan.nodes.size(), 0);
        if (g.ops.size() != plan.graph.ops.size() || g.tensors.size() > plan.storage.size()) BAND_GIVE_UP;
        std::vector<int> op_producer(g.tensors.size(), -1);
        for (size_t op = 0; op < g.ops.size(); op++)
            for (int t : g.ops[op].outputs)
                if (t >= 0) op_producer[static_cast<size_t>(t)] = static_cast<int>(op);
        std::function<void(const Node&, std::vector<int>&)> reads = [&](const Node& n, std::vector<int>& v) {
            for (int t : n.in) v.push_back(t);
            if (n.res >= 0) v.push_back(n.res);
            for (const Node& m : n.members) reads(m, v);
            for (const Node& m : n.head_nodes) reads(m, v);
            for (const Node::Stage& sg : n.stages) { if (sg.src_t >= 0) v.push_back(sg.src_t); if (sg.res_t >= 0) v.push_back(sg.res_t); }
        };
        const size_t first = static_cast<size_t>(bp.first);
        bool any_band = false;
        for (size_t i = first; i < plan.nodes.size(); i++) {
            const Node& n = plan.nodes[i];
            if (is_view(n)) continue;
            size_t inside = 0;
            for (int op : n.src_ops) inside += band_op[static_cast<size_t>(op)] ? 1 : 0;
            if (n.src_ops.empty() || (inside != 0 && inside != n.src_ops.size())) BAND_GIVE_UP;   // a launch of the batched plan straddles the cut
            if (inside) { any_band = true; continue; }
            bp.node_runs[i] = 1;
            std::vector<int> rd;
            reads(n, rd);
            for (int t : rd) {
                const int op = op_producer[static_cast<size_t>(t)];
                if (op < 0 || !band_op[static_cast<size_t>(op)]) continue;   // a constant, the graph input, or a tensor of another launch behind the cut
                const int d = producer[static_cast<size_t>(t)];
                if (d < 0) BAND_GIVE_UP;   // a tensor inside one of the program's blocks
                const Storage& sp = plan.storage[static_cast<size_t>(t)];
                if (sp.root < 0 || (sp.offset & 3) || (sp.frame_stride & 3)) BAND_GIVE_UP;
                if (is_graph_output(t)) { if (prog[static_cast<size_t>(d)].dst_base < 0) BAND_GIVE_UP; continue; }   // (already written where the launch reads it)
                if (plan.root_offset[static_cast<size_t>(sp.root)] < 0 || (plan.root_offset[static_cast<size_t>(sp.root)] & 3)) BAND_GIVE_UP;
                BandStage& pd = prog[static_cast<size_t>(d)];
                if (pd.dst_base >= 2 && bp.ext[static_cast<size_t>(pd.dst_base - 2)].tensor == t) continue;   // (a second reader of the same tensor)
                if (pd.dst_base >= 0 || (pd.Co & 3)) BAND_GIVE_UP;
                pd.dst_base = ext_slot(-1, t); pd.dst_off = 0; pd.dst_fs = sp.frame_stride;
                if (pd.dst_base < 0) BAND_GIVE_UP;
            }
        }
        if (!any_band || bp.node_runs[first]) BAND_GIVE_UP;
        // the band launch writes its tensors EARLIER than the batched plan's launches would have: a launch that keeps its place in front of the
        // last node the program stands for may only write graph outputs (an arena slot it writes might be one the program's tensors live in)
        size_t last_inside = 0;
        for (size_t i = first; i < plan.nodes.size(); i++)
            if (!is_view(plan.nodes[i]) && !bp.node_runs[i]) last_inside = i;
        for (size_t i = first; i < last_inside; i++) {
            if (!bp.node_runs[i]) continue;
            std::vector<int> outs = plan.nodes[i].extra_out;
            outs.push_back(plan.nodes[i].out);
            for (int t : outs)
                if (!is_graph_output(t)) BAND_GIVE_UP;
        }
        // the nodes in front of the cut in the level-2 lowering must be exactly the program (nothing the batched plan computes is skipped)
        for (size_t i = cut; i < p2.nodes.size(); i++)
            for (int op : p2.nodes[i].src_ops)
                if (band_op[static_cast<size_t>(op)]) BAND_GIVE_UP;
        // every graph output must be written, whole, by the band program or by a launch behind it (the first convolution writes none of them)
        for (size_t k = 0; k < out_root.size(); k++) {
            size_t written = 0;
            for (const BandStage& st : prog)
                if (st.dst_base >= 2 && bp.ext[static_cast<size_t>(st.dst_base - 2)].out_k == static_cast<int>(k)) written += static_cast<size_t>(st.Ho) * st.Wo * st.Co;
            bool later = false;
            for (size_t i = first; i < plan.nodes.size(); i++)
                if (bp.node_runs[i] && plan.storage[static_cast<size_t>(plan.nodes[i].out)].root == out_root[k]) later = true;
            if (!later && written != g.tensors[g.outputs[k]].elems()) BAND_GIVE_UP;
        }
    }
    // ---- a program with 2x2 convolutions (the iris network: two branches of 21 stages behind its 8x8 fork) runs branch by branch, not in the
    // graph's interleaved order: a stage goes behind the newest tensor it can read, so that one branch's skip / middle / output tensors and the
    // fork tensor the other branch still waits for are all that is alive — four LDS tiles
    void branch_order() {
        const int N0 = static_cast<int>(prog.size());
        bool any_cv2 = false;
        for (const BandStage& st : prog) any_cv2 = any_cv2 || (st.kind == BAND_PW && st.S == 2);
        if (!any_cv2) return;
        std::vector<int> pos(static_cast<size_t>(N0), -1), order;
        for (int step = 0; step < N0; step++) {
            int best = -1, best_pos = -2;
            for (int k = 0; k < N0; k++) {
                const BandStage& st = prog[static_cast<size_t>(k)];
                if (pos[static_cast<size_t>(k)] >= 0) continue;
                if (st.dep >= 0 && pos[static_cast<size_t>(st.dep)] < 0) continue;
                if (st.res_dep >= 0 && pos[static_cast<size_t>(st.res_dep)] < 0) continue;
                const int dp = st.dep >= 0 ? pos[static_cast<size_t>(st.dep)] : -1;
                if (dp > best_pos) { best = k; best_pos = dp; }
            }
            if (best < 0) BAND_GIVE_UP;
            pos[static_cast<size_t>(best)] = step;
            order.push_back(best);
        }
        reorder(order, pos);
    }
    // ---- (any program: the face mesh's two branches behind its 6x6 tensor as well) the second branch behind a fork goes to the workgroups
    // the first one leaves idle (BandStage::woff): where a tensor of one-row bands on every 2nd / 4th ... workgroup is the input of two stages, the
    // later one and everything behind it are run by the workgroups half a group further on, at the same time as the first branch; its first
    // stage takes its whole input from the packet buffer
    void fork_branches() {
        const int N0 = static_cast<int>(prog.size());
        const std::vector<char> read = stages_read();
        for (int k = 0; k < N0; k++) {
            const BandStage& fk = prog[static_cast<size_t>(k)];
            std::vector<int> readers;
            for (int j = 0; j < N0; j++)
                if (prog[static_cast<size_t>(j)].dep == k) readers.push_back(j);
            if (readers.size() != 2 || fk.R != 1 || fk.wshift < 1 || fk.woff != 0) continue;
            if (!read[static_cast<size_t>(readers[0])] || !read[static_cast<size_t>(readers[1])]) continue;   // (a reader nobody reads is an output head: fork_heads)
            const int woff = 1 << (fk.wshift - 1);
            std::vector<char> inB(static_cast<size_t>(N0), 0);
            inB[static_cast<size_t>(readers[1])] = 1;
            for (int j = readers[1] + 1; j < N0; j++)
                if (prog[static_cast<size_t>(j)].dep >= 0 && inB[static_cast<size_t>(prog[static_cast<size_t>(j)].dep)]) inB[static_cast<size_t>(j)] = 1;
            bool ok = true;
            for (int j = 0; j < N0 && ok; j++) {
                const BandStage& st = prog[static_cast<size_t>(j)];
                if (inB[static_cast<size_t>(j)]) {
                    ok = st.wshift >= fk.wshift && st.woff == 0 && (st.res_dep < 0 || st.res_dep == k || inB[static_cast<size_t>(st.res_dep)]);
                } else if (st.res_dep >= 0 && inB[static_cast<size_t>(st.res_dep)]) {
                    ok = false;
                }
            }
            const BandStage& root = prog[static_cast<size_t>(readers[1])];
            const int rows = root.kind == BAND_BLOCK ? (root.S == 1 ? root.R + 2 : 2 * root.R + 1) : (root.S == 2 ? 2 * root.R : root.R);
            if (!ok || rows * root.W * (root.C / 4) > 4 * 512) continue;
            for (int j = 0; j < N0; j++)
                if (inB[static_cast<size_t>(j)]) prog[static_cast<size_t>(j)].woff = woff;
            prog[static_cast<size_t>(readers[1])].Rin = 0;
            prog[static_cast<size_t>(readers[1])].cross = 1;
        }
    }
    // ---- the output heads (1x1 stages nobody reads: the SSD heads of the detectors) of a tensor of one-row bands go to workgroups the trunk
    // leaves idle there (BandStage::woff, as the iris network's second branch): they take their input rows from the packet buffer and run beside
    // the trunk's next stages instead of in front of them; the two heads of one tensor on two different sets of idle workgroups where there are two
    void fork_heads() {
        const std::vector<char> read = stages_read();
        std::vector<int> moved(prog.size(), 0);   // heads of a tensor already moved
        for (size_t k = 0; k < prog.size(); k++) {
            BandStage& st = prog[k];
            if (read[k] || st.kind != BAND_PW || st.S != 1 || st.dep < 0 || st.woff != 0 || st.cross || st.res_mode != RES_NONE) continue;
            const BandStage& pd = prog[static_cast<size_t>(st.dep)];
            if (pd.R != 1 || pd.wshift < 1 || pd.woff != 0 || st.R != 1 || st.wshift != pd.wshift || st.nbands != pd.nbands) continue;
            if (st.W * (st.C / 4) > 4 * 512) continue;   // its one input row: four 16-byte elements per lane
            const int j = moved[static_cast<size_t>(st.dep)]++;
            int woff = 1 << (pd.wshift - 1);
            if ((j & 1) && pd.wshift >= 2) woff += 1 << (pd.wshift - 2);
            st.woff = woff; st.Rin = 0; st.cross = 1;
        }
    }
    // ---- the output heads (stages nobody reads) move up behind the first other reader of their input: the LDS tiles hold a tensor
    // only until the trunk has moved on twice, and a head costs its workgroups two microseconds wherever it stands
    void heads_up() {
        const int N0 = static_cast<int>(prog.size());
        const std::vector<char> read = stages_read();
        std::vector<char> placed(static_cast<size_t>(N0), 0);
        auto head = [&](int k) { return !read[static_cast<size_t>(k)] && prog[static_cast<size_t>(k)].kind == BAND_PW; };
        std::vector<int> order;
        for (int k = 0; k < N0; k++) {
            if (placed[static_cast<size_t>(k)] || head(k)) continue;   // (a head is placed behind a sibling, or at the end)
            auto take = [&](int j) { order.push_back(j); placed[static_cast<size_t>(j)] = 1; };
            take(k);
            for (int j = 0; j < N0; j++)
                if (!placed[static_cast<size_t>(j)] && head(j) && prog[static_cast<size_t>(j)].dep == prog[static_cast<size_t>(k)].dep && prog[static_cast<size_t>(j)].dep >= 0) take(j);
        }
        for (int k = 0; k < N0; k++)
            if (!placed[static_cast<size_t>(k)]) order.push_back(k);
        std::vector<int> pos(static_cast<size_t>(N0), -1);
        for (int k = 0; k < N0; k++) pos[static_cast<size_t>(order[static_cast<size_t>(k)])] = k;
        reorder(order, pos);
    }
    // ---- who reads what: the last reader of every LDS tile, the packet buffers for the rows other workgroups read, the far copies
    void readers() {
        const int NS = static_cast<int>(prog.size());
        last_reader.assign(static_cast<size_t>(NS), -1);
        for (int k = 0; k < NS; k++) {
            BandStage& st = prog[static_cast<size_t>(k)];
            if (st.dep >= 0) {
                BandStage& pd = prog[static_cast<size_t>(st.dep)];
                // a lateral convolution reads a trunk tensor that is 10 - 30 stages old: its rows are this workgroup's own, so the producer also writes them to
                // the launch's workspace and this stage reads them back from there (like the program's input) — the tile does not have to stay alive
                if (st.res_mode == RES_UP2X && st.kind == BAND_PW && st.S == 1 && !st.cross && k - st.dep > 2 && pd.R == st.R && pd.wshift == st.wshift && pd.woff == st.woff &&
                    pd.nbands == st.nbands && (pd.dst_base < 0 || pd.far_copy) && (pd.Co & 3) == 0) {
                    st.far_src = 1; pd.far_copy = 1; pd.dst_base = 0;
                } else {
                    last_reader[static_cast<size_t>(st.dep)] = k;
                    const bool cv2_halo = st.kind == BAND_PW && st.S == 2 && pd.R < 2 * st.R;   // its row 2r + 1 is the next workgroup's
                    if (st.cross) pd.pub_lo = 1;   // (one-row bands: all of the tensor)
                    if ((st.kind == BAND_BLOCK || cv2_halo) && pd.nbands > 1) {
                        pd.pub_lo = 1;
                        if (st.kind == BAND_BLOCK && (st.S == 1 || st.pre) && pd.R > 1) pd.pub_hi = 1;
                    }
                }
            } else {
                input_last_reader = k;
            }
            if (st.res_dep >= 0) last_reader[static_cast<size_t>(st.res_dep)] = k;
            if (st.res_dep == -1) input_last_reader = k;
            if (st.res_mode == RES_UP2X) {
                if (st.res_dep < 0) BAND_GIVE_UP;
                prog[static_cast<size_t>(st.res_dep)].pub_lo = 1;   // (one-row bands: all of the coarse tensor travels)
            }
        }
    }

    // LDS tiles, placed by liveness (an interval allocator: full_range's tensors go from 56 KB for a band of 96x96x32 to 14 KB for one of 96x96x8, and
    // its decoder keeps three 31 KB tensors of 48x48x48 alive): a tensor gets a gap that holds it when it is produced and keeps it until its last reader
    // has run.  Rows of a tile: the band's own + one above + one below, + one more below where a stride-2 BLOCK reads the tensor.
    struct Tiles {
        std::vector<int> src, res, dst;   // per stage: LDS floats in front of its input / skip / output tile (-1: none)
        std::vector<char> h3;             // per stage: a stride-2 BLOCK reads the output tile
        int floats = 0;
    };
    // The ONE liveness walk: the tiles of every stage in an arena of S floats, or false when one does not fit.  A tensor goes to the lowest or to the
    // highest gap that holds it — policy 0: whichever end leaves the larger free block (first fit from the bottom alone puts full_range's second
    // 96x96x32 tensor in the middle of the arena, and the third, 56 KB, behind it: 155 KB for 113 KB of live tensors); 1 / 2: wide tensors (>= 32 KB) at
    // the bottom and narrow ones at the top, or the other way round (then the first / last gap that fits)
    bool walk(int S, int policy, Tiles& t) const {
        const size_t NS = prog.size();
        struct Alloc { int off, size, stage; };   // stage: producer (-1: the program's input, -3: a far input held for one stage)
        std::vector<Alloc> lv;
        auto dead_at = [&](const Alloc& al, int k) { return al.stage == -3 || (al.stage == -1 ? input_last_reader <= k : last_reader[static_cast<size_t>(al.stage)] <= k); };
        auto where = [&](int stage) {
            for (const Alloc& al : lv)
                if (al.stage == stage) return al.off;
            return -1;
        };
        auto put = [&](int need, int stage) {
            need = static_cast<int>(align_up(std::max(need, 16), 16));
            std::sort(lv.begin(), lv.end(), [](const Alloc& x, const Alloc& y) { return x.off < y.off; });
            std::vector<std::pair<int, int>> gaps;   // [begin, end)
            int at = 0;
            for (const Alloc& al : lv) { if (al.off > at) gaps.push_back({at, al.off}); at = std::max(at, al.off + al.size); }
            if (S > at) gaps.push_back({at, S});
            int best = -1, best_left = -1;
            for (const auto& gp : gaps) {
                if (gp.second - gp.first < need) continue;
                for (int end = 0; end < 2; end++) {
                    const int off = end ? gp.second - need : gp.first;
                    int left = 0;   // the largest free block that remains
                    for (const auto& g2 : gaps) {
                        if (&g2 != &gp) left = std::max(left, g2.second - g2.first);
                        else left = std::max(left, std::max(off - g2.first, g2.second - (off + need)));
                    }
                    const bool wide_t = need >= 8192;
                    const int score = policy == 0 ? left : ((policy == 1) == wide_t ? (end ? -1 : S - off) : (end ? off : -1));
                    if (score > best_left) { best_left = score; best = off; }
                }
            }
            if (best >= 0) { lv.push_back(Alloc{best, need, stage}); t.floats = std::max(t.floats, best + need); }
            return best;
        };
        t = Tiles{std::vector<int>(NS, -1), std::vector<int>(NS, -1), std::vector<int>(NS, -1), std::vector<char>(NS, 0), 0};
        for (const BandStage& st : prog)
            if (st.kind == BAND_BLOCK && st.S == 2 && !st.pre && st.dep >= 0) t.h3[static_cast<size_t>(st.dep)] = 1;
        for (size_t k = 0; k < NS; k++) {
            const BandStage& st = prog[k];
            // what nobody reads any more is free — but for what THIS stage reads (its last reader may be this very stage)
            const int keep_src = st.dep >= 0 && !st.far_src ? st.dep : (st.dep < 0 ? -1 : -4);
            const int keep_res = st.res_mode != RES_UP2X && st.res_dep >= -1 ? st.res_dep : -4;
            std::vector<Alloc> kept;
            for (const Alloc& al : lv)
                if (!dead_at(al, static_cast<int>(k)) || al.stage == keep_src || al.stage == keep_res) kept.push_back(al);
            lv.swap(kept);
            if (st.dep < 0) {
                // the program's input comes from global memory into a tile of its own: only its first reader may be such a stage (a skip may read it there later)
                if (where(-1) >= 0) BAND_GIVE_UP;
                const int rows = st.kind == BAND_BLOCK ? (st.S == 1 ? st.R + 2 : 2 * st.R + 2) : st.R + 1;
                if ((t.src[k] = put(rows * (st.W + 2) * (st.C + 4), -1)) < 0) return false;
            } else if (st.far_src) {
                // its own rows come back from the workspace into a free place (held for this stage only)
                if ((t.src[k] = put((st.R + 1) * (st.W + 2) * (st.C + 4), -3)) < 0) return false;
            } else if ((t.src[k] = where(st.dep)) < 0) {
                BAND_GIVE_UP;   // its input is no longer in LDS
            }
            if (keep_res != -4 && (t.res[k] = where(st.res_dep)) < 0) BAND_GIVE_UP;
            if (last_reader[k] >= 0)
                if ((t.dst[k] = put(bandnet_tile_floats(st.R, st.Wo, st.Co, 2 + t.h3[k]), static_cast<int>(k))) < 0) return false;
        }
        return true;
    }
    // ---- placement: the tiles of the smallest arena that takes them, the packet buffers and far copies in the workspace, and what the kernel
    // requires of a stage and the tiles it reads
    void place() {
        Tiles t;
        bool ok = false;
        for (int S = 4096; S <= 40960 && !ok; S += 64)   // (floats: 16 .. 160 KB in steps of 256 bytes; three placement policies each)
            for (int policy = 0; policy < 3 && !ok; policy++) ok = walk(S, policy, t);
        if (!ok) BAND_GIVE_UP;
        int dw_floats = 0;
        for (size_t k = 0; k < prog.size(); k++) {
            BandStage& st = prog[k];
            st.src_lds = t.src[k];
            if (st.dep >= 0 && !st.far_src) {
                st.src_ll = prog[static_cast<size_t>(st.dep)].dst_ll;
                const BandStage& pd = prog[static_cast<size_t>(st.dep)];
                const bool cv2_halo = st.kind == BAND_PW && st.S == 2 && pd.R < 2 * st.R;
                if (((st.kind == BAND_BLOCK || cv2_halo) && st.nbands > 1 && st.src_ll < 0) || (st.cross && st.src_ll < 0)) BAND_GIVE_UP;
            }
            if (st.res_mode == RES_UP2X) {
                const BandStage& cd = prog[static_cast<size_t>(st.res_dep)];
                if (cd.dst_ll < 0 || cd.R != 1 || cd.Ho * 2 != st.Ho || cd.Wo * 2 != st.Wo || cd.Co != st.Co || st.R != 1) BAND_GIVE_UP;
                st.res_ll = cd.dst_ll; st.res_stage = st.res_dep;
                dw_floats = std::max(dw_floats, 2 * cd.Wo * (st.Co + 4));   // its two rows land in the depthwise area (a 1x1 stage does not use it)
            } else if (st.res_dep >= -1) {
                st.res_lds = t.res[k];
                st.res_tile = 1;   // (a flag now: the skip comes from another tile, at res_lds)
                // the skip is read at the output's pixel positions: its band must have the output's rows (same shape, same owners)
                if (st.res_mode == RES_MAXPOOL) {
                    // ... or, the 2x2 max of the input of the 2x2 convolution / stride-2 block in front: that stage, run by the same workgroups on the same
                    // bands, left rows 2 r0 .. 2 r0 + 2 R - 1 of the tensor in the tile it read them from
                    if (st.dep < 0 || st.res_dep < 0) BAND_GIVE_UP;
                    const BandStage& cv = prog[static_cast<size_t>(st.dep)];
                    const BandStage& rd = prog[static_cast<size_t>(st.res_dep)];
                    if (cv.S != 2 || cv.dep != st.res_dep || cv.src_lds != st.res_lds || cv.far_src || cv.R != st.R || cv.wshift != st.wshift || cv.nbands != st.nbands)
                        BAND_GIVE_UP;
                    if (rd.Ho != 2 * st.Ho || rd.Wo != 2 * st.Wo || rd.Co != st.res_c) BAND_GIVE_UP;
                } else if (st.res_dep >= 0) {
                    const BandStage& rd = prog[static_cast<size_t>(st.res_dep)];
                    if (rd.Ho != st.Ho || rd.Wo != st.Wo || rd.Co != st.res_c || rd.R != st.R || rd.wshift != st.wshift) BAND_GIVE_UP;
                } else {
                    const BandStage& first = prog[0];   // (the stage that loaded the program's input: own rows at tile rows 1 ..)
                    if (first.dep >= 0 || first.H != st.Ho || first.W != st.Wo || first.C != st.res_c || first.R != st.R || first.wshift != st.wshift || first.S != 1) BAND_GIVE_UP;
                }
            }
            if (last_reader[k] >= 0) {
                st.dst_h3 = t.h3[k]; st.dst_lds = t.dst[k]; st.dst_tile = 0;   // (dst_tile is a flag now: the output stays in LDS, at dst_lds)
                if (st.pub_lo || st.pub_hi) {
                    st.dst_ll = ws;
                    ws += align_up(2 * static_cast<long>(st.Ho) * st.Wo * st.Co, 64);
                }
            }
            if (st.far_copy) {   // the plain copy a lateral convolution reads back (frame stride = the workspace's: patched in pack())
                st.dst_off = ws;
                ws += align_up(static_cast<long>(st.Ho) * st.Wo * st.Co, 64);
            }
            if (st.far_src) {
                const BandStage& pd = prog[static_cast<size_t>(st.dep)];
                if (!pd.far_copy || pd.dst_base != 0) BAND_GIVE_UP;
                st.src_base = 0; st.src_off = pd.dst_off;
            }
            dw_floats = std::max(dw_floats, bandnet_dw_floats(st));
        }
        bp.dw_floats = static_cast<int>(align_up(dw_floats, 4));
        bp.tiles_floats = static_cast<int>(align_up(t.floats, 16));
    }
    // ---- the kernel instantiation, the LDS total, the descriptors as the kernel reads them
    void pack() {
        const int NS = static_cast<int>(prog.size());
        for (const BandStage& st : prog) {
            bp.cv2 = bp.cv2 || (st.kind == BAND_PW && st.S == 2);
            bp.xb = bp.xb || (st.kind == BAND_BLOCK && st.cross);
            bp.wide = bp.wide || st.C > 128 || st.Co > 128 || st.res_mode == RES_UP2X || st.pre;
        }
        if (bp.cv2 && bp.xb) BAND_GIVE_UP;   // (no kernel instantiation for both: the iris network's second branch starts with a 1x1 stage)
        if (bp.wide && (bp.cv2 || bp.xb)) BAND_GIVE_UP;   // (likewise)
        bp.lds_bytes = bandnet_lds_bytes(bp.tiles_floats, bp.dw_floats, NS);
        if (debug()) {
            std::fprintf(stderr, "bandnet: %d stages, NW %d, LDS %d B = tiles %d + depthwise %d + constants + program\n", NS, NW, bp.lds_bytes, bp.tiles_floats * 4, bp.dw_floats * 4);
            for (int k = 0; k < NS; k++) {
                const BandStage& st = prog[static_cast<size_t>(k)];
                std::fprintf(stderr, "  stage %2d %s S%d %dx%dx%d -> %dx%dx%d R %d wshift %d src %d dst %d res %d (dep %d, mode %d, c %d) last reader %d\n", k, st.kind == BAND_BLOCK ? "block" : "pw   ", st.S, st.H, st.W, st.C,
                             st.Ho, st.Wo, st.Co, st.R, st.wshift, st.src_lds * 4, st.dst_tile >= 0 ? st.dst_lds * 4 : -1, st.res_tile >= 0 ? st.res_lds * 4 : -1, st.res_dep, st.res_mode, st.res_c, last_reader[static_cast<size_t>(k)]);
            }
        }
        if (bp.lds_bytes > 160 * 1024) BAND_GIVE_UP;
        bp.ws_frame_floats = std::max<long>(ws, 64);
        bp.nstages = NS;
        consts.resize(consts.size() + 64, 0.f);
        bp.consts.swap(consts);
        bp.prog.resize(prog.size());
        for (size_t k = 0; k < prog.size(); k++) {
            BandStage q = prog[k];
            if (q.far_copy) q.dst_fs = bp.ws_frame_floats;
            if (q.far_src) { q.src_fs = bp.ws_frame_floats; q.dep = -1; q.Rin = 0; }   // (the kernel's "input in plain memory" path; the stage order keeps the host's dep)
            if (!bandnet_pack(q, &bp.prog[k])) BAND_GIVE_UP;
        }
        bp.ready = true;
    }

    void run() {
        stem();
        stages();
        cut_against_batched_plan();
        branch_order();
        if (o.fork) { fork_branches(); fork_heads(); }
        heads_up();
        readers();
        place();
        pack();
    }
};

}  // namespace

BandPlan build_band_plan(const Plan& plan, const Plan& level2, const BandOptions& o) {
    BandPlan none;
    for (bool conv2_ok : {true, false}) {   // (without 2x2 convolutions where a graph that has them gave no program with them)
        Planner p{plan, level2, o, conv2_ok};
        try {
            p.run();
            return std::move(p.bp);
        } catch (const GiveUp& e) {
            none.why = "bandplan.cpp:" + std::to_string(e.line);
            if (debug()) std::fprintf(stderr, "bandnet: no single-launch plan (%s)\n", none.why.c_str());
            if (!p.saw_conv2) break;
        }
    }
    return none;
}

}  // namespace mi
