// launches.cpp — see launches.hpp.
#include "launches.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

namespace mi {

namespace {
void same_pad(int in, int k, int stride, int out, int* before) { *before = std::max(0, (out - 1) * stride + k - in) / 2; }
bool is_view(const Node& n) { return n.kind == Node::Reshape || n.kind == Node::Concat; }
int dim(const std::vector<int>& v, size_t d) { return d < v.size() ? v[d] : 1; }
float clamp_of(int act) { return act == ACT_RELU6 ? 6.f : INFINITY; }
}  // namespace

bool band_cut(const BandPlan& bp, size_t i) { return static_cast<int>(i) >= bp.first && !bp.node_runs[i]; }

int band_run_launches(const Plan& plan, const BandPlan& bp) {
    int launches = 1;
    for (size_t i = 0; i < plan.nodes.size(); i++)
        if (!is_view(plan.nodes[i]) && !band_cut(bp, i)) launches++;
    return launches;
}

float* tensor_ptr_mut(const Plan& plan, const LaunchCtx& c, int t, long* fs) {
    const Graph& g = plan.graph;
    const Storage& s = plan.storage[t];
    *fs = s.frame_stride;
    for (size_t k = 0; k < g.outputs.size(); k++)
        if (plan.storage[g.outputs[k]].root == s.root) return c.out[k] + static_cast<long>(c.chunk_start) * s.frame_stride + s.offset;
    if (s.root == plan.storage[g.inputs[0]].root) throw std::runtime_error("plan writes into the graph input");
    const long off = plan.root_offset[s.root];
    if (off < 0) throw std::runtime_error("tensor has no storage");
    return c.arena + off * c.chunk_cap + s.offset;
}

bool takes_u8_input(const Plan& plan, const PlanConsts& consts) {
    const Graph& g = plan.graph;
    const int root = plan.storage[g.inputs[0]].root;
    int readers = 0;
    bool stem = false;
    for (const Node& n : plan.nodes) {
        if (is_view(n)) continue;
        bool reads = false;
        for (int t : n.in) reads |= t >= 0 && plan.storage[t].root == root;
        if (n.res >= 0 && plan.storage[n.res].root == root) reads = true;
        if (!reads) continue;
        readers++;
        if (n.kind == Node::Conv && !n.gemm_head && n.in[0] >= 0 && plan.storage[n.in[0]].root == root) {
            const auto& si = g.tensors[n.in[0]].shape;
            const auto& so = g.tensors[n.out].shape;
            ConvArgs a;
            a.out = reinterpret_cast<float*>(uintptr_t{256}); a.out_fs = 4;  // aligned placeholders: only the shape tests matter here
            a.C = si[3]; a.Co = so[3]; a.KH = n.KH; a.KW = n.KW; a.sh = n.sh; a.sw = n.sw;
            static const float some_bias = 0.f;
            a.ep.bias = &some_bias;
            a.ep.res_mode = n.res >= 0 ? n.res_mode : RES_NONE;
            stem = conv_takes_u8(a) && consts.node_b[&n - plan.nodes.data()] >= 0;
        }
    }
    return readers == 1 && stem;
}

// Output heads that may run beside the trunk: compute nodes whose output lives in a graph-output buffer and is
// read by no other launch, and that come after the last trunk node in plan order (so no later trunk launch can
// re-use arena memory they still read: the arena's liveness analysis follows plan order)
SideSchedule schedule_side_streams(const Plan& plan, int head_streams) {
    const Graph& g = plan.graph;
    const size_t N = plan.nodes.size();
    SideSchedule sc;
    sc.slot.assign(N, -1); sc.wait.assign(N, -1); sc.event_after.assign(N, 0);
    auto root = [&](int t) { return plan.storage[t].root; };
    auto producer = [&](int t, size_t before) {  // the last launch in front of node `before` that writes (the buffer of) tensor t, -1: none
        int prod = -1;
        for (size_t j = 0; j < before; j++) {
            if (is_view(plan.nodes[j])) continue;
            bool makes = root(plan.nodes[j].out) == root(t);
            for (int x : plan.nodes[j].extra_out) makes |= root(x) == root(t);
            if (makes) prod = static_cast<int>(j);
        }
        return prod;
    };
    auto beside = [&](size_t i, int slot, int prod) {  // node i runs on side stream `slot`, behind launch prod
        sc.slot[i] = slot % std::max(1, std::min(head_streams, kHeadStreams));
        sc.wait[i] = prod;
        if (prod >= 0) sc.event_after[static_cast<size_t>(prod)] = 1;
    };
    std::vector<int> out_roots;
    for (int o : g.outputs) out_roots.push_back(root(o));
    std::vector<char> head(N, 0);
    int last_trunk = -1;
    for (size_t i = 0; i < N; i++) {
        const Node& n = plan.nodes[i];
        if (is_view(n)) continue;
        bool feeds_output = std::find(out_roots.begin(), out_roots.end(), root(n.out)) != out_roots.end();
        for (size_t j = 0; j < N && feeds_output; j++) {
            const Node& m = plan.nodes[j];
            if (is_view(m)) continue;
            for (int x : m.in) if (x == n.out) feeds_output = false;
            if (m.res == n.out) feeds_output = false;
        }
        if (n.kind == Node::Resident && (n.in.size() != 1 || !n.extra_out.empty())) feeds_output = false;  // several inputs / outputs: stays on the trunk
        head[i] = feeds_output;
        if (!feeds_output) last_trunk = static_cast<int>(i);
    }
    int slots = 0;
    for (size_t i = 0; i < N; i++) {
        const Node& n = plan.nodes[i];
        if (!head[i] || static_cast<int>(i) < last_trunk || is_view(n)) continue;
        if (n.res >= 0 && n.res != n.in[0]) continue;  // two producers: keep it on the trunk
        // heads are spread round robin over `heads` side streams (option, default 1).  They are independent of each other, but
        // on BackCamera (four small heads behind the last trunk launch) every extra parallel branch of the replay graph cost
        // more than it hid: 1.675 ms per step with 1 stream, 1.69 / 1.68 / 1.72 with 2 / 3 / 4
        beside(i, slots++, producer(n.in[0], i));
    }
    // tail branches (Plan::branch): chain 0 stays on the trunk stream, every other chain runs on a side stream behind the launch
    // that produced its newest input (the trunk runs in plan order, so the older inputs are done by then; launches of the same
    // chain share a stream).  The arena keeps everything the branches touch allocated to the end of the plan.
    static const bool no_branches = getenv("MI_NO_BRANCHES") != nullptr;  // development aid
    for (size_t i = 0; i < N && !no_branches && plan.branch.size() == N; i++) {
        const Node& n = plan.nodes[i];
        if (plan.branch[i] < 1 || is_view(n)) continue;
        int prod = n.res >= 0 ? producer(n.res, i) : -1;
        for (int t : n.in) prod = std::max(prod, producer(t, i));
        beside(i, plan.branch[i] - 1, prod);
    }
    return sc;
}

namespace {

// One chunk being lowered: the argument structs, each filled in one place, and the choice of kernel per node
struct Lowering {
    const Plan& plan;
    const PlanConsts& pc;
    const BandPlan& bp;
    const SideSchedule& sched;
    const LaunchCtx& c;
    const bool want_labels;
    const Graph& g = plan.graph;

    const std::vector<int>& shape(int t) const { return g.tensors[t].shape; }
    const float* weights(long off) const { return off >= 0 ? c.weights + off : nullptr; }

    float* tensor_ptr_mut(int t, long* fs) const { return mi::tensor_ptr_mut(plan, c, t, fs); }
    const float* tensor_ptr(int t, long* fs) const {
        const Storage& s = plan.storage[t];
        *fs = s.frame_stride;
        if (s.root == plan.storage[g.inputs[0]].root) return c.in + static_cast<long>(c.chunk_start) * s.frame_stride + s.offset;
        return tensor_ptr_mut(t, fs);
    }

    Epilogue epilogue(size_t i) const {
        const Node& n = plan.nodes[i];
        Epilogue ep;
        ep.bias = weights(n.kind == Node::Block ? pc.node_b2[i] : pc.node_b[i]);
        ep.alpha = weights(pc.node_alpha[i]);
        ep.act = n.act;
        if (n.res >= 0) {
            const auto& sr = shape(n.res);
            ep.res = tensor_ptr(n.res, &ep.res_fs);
            ep.res_mode = n.res_mode;
            ep.res_after = n.res_after ? 1 : 0;
            ep.res_C = sr.back();
            ep.res_H = dim(sr, 1);
            ep.res_W = dim(sr, 2);
        }
        return ep;
    }

    // Block node i as the block kernels take it (block / strip / mstrip / mwalk / ms2, and as a member of an mstrip run)
    BlockArgs block_args(size_t i) const {
        const Node& n = plan.nodes[i];
        const auto &si = shape(n.in[0]), &so = shape(n.out);
        BlockArgs a;
        a.in = tensor_ptr(n.in[0], &a.in_fs);
        a.out = tensor_ptr_mut(n.out, &a.out_fs);
        a.has_dw = n.w >= 0;
        a.w_dw = a.has_dw ? c.weights + pc.node_w[i] : nullptr;
        a.b_dw = weights(pc.node_b[i]);
        a.w_pw = c.weights + pc.node_w2[i];
        a.B = c.F; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.Ho = so[1]; a.Wo = so[2]; a.Co = so[3];
        a.sh = n.sh; a.sw = n.sw;
        if (a.has_dw && n.padding == Padding::Same) { same_pad(a.H, 3, a.sh, a.Ho, &a.pt); same_pad(a.W, 3, a.sw, a.Wo, &a.pl); }
        if (a.has_dw && n.ept >= 0) { a.pt = n.ept; a.pl = n.epl; }
        a.ep = epilogue(i);
        a.w_strip = weights(pc.node_strip[i]);
        a.w_mwalk = weights(pc.node_mwalk[i]);
        return a;
    }

    // Two blocks a, b as ONE launch of dblock_kernels.hip / mdblock_kernels.hip, from the tensor t_in at `in` to the tensor t_out.
    // pair: two plain BlazeBlocks, each adding its own input (else full_range's double block: the members say which skips exist)
    DblockArgs dblock_args(const float* in, long in_fs, int t_in, int t_out, const Node& a, const Node& b, long mconsts, bool pair) const {
        const auto& si = shape(t_in);
        DblockArgs d;
        d.in = in; d.in_fs = in_fs;
        d.out = tensor_ptr_mut(t_out, &d.out_fs);
        d.B = c.F; d.H = si[1]; d.W = si[2]; d.C = si[3]; d.Cm = shape(a.out)[3]; d.Co = shape(t_out)[3];
        d.hi1 = clamp_of(a.act); d.hi2 = clamp_of(b.act);
        d.skip1 = pair ? 1 : a.res >= 0;
        d.skip2_from_a = pair ? 1 : b.res == a.out;
        d.act1 = a.act; d.act2 = b.act;
        d.mconsts = weights(mconsts);
        if (pair) d.band_rows = c.mdb_band;
        return d;
    }

    ResBases res_bases() const {
        ResBases r;
        for (int k = 0; k < kResBases; k++) { r.p[k] = nullptr; r.scale[k] = 0; r.frame0[k] = 0; }
        r.p[0] = c.arena;
        r.scale[0] = c.chunk_cap;
        r.p[1] = const_cast<float*>(c.in);
        r.frame0[1] = c.chunk_start;
        for (int k = 0; k < static_cast<int>(g.outputs.size()) && 2 + k < kResBases; k++) { r.p[2 + k] = c.out[k]; r.frame0[2 + k] = c.chunk_start; }
        r.weights = c.weights;
        return r;
    }

    template <class A>
    static void set(Launch& l, Launcher to, const A& a, const char* label) {
        l.to = to;
        l.args = a;
        if (label) l.label = label;
    }
    const char* lab(const char* s) const { return want_labels ? s : nullptr; }

    // The single-launch plan: everything behind the first convolution is ONE launch (bandnet_kernels.hip), but for the nodes behind the program's
    // end (bp.node_runs), which keep their launches
    void band_launch(Launch& l) const {
        BandLaunch a;
        a.prog = c.band_prog; a.nstages = bp.nstages; a.NW = bp.nw; a.F = c.F; a.lds_bytes = bp.lds_bytes;
        a.tiles_floats = bp.tiles_floats;
        a.dw_floats = bp.dw_floats; a.ws_frame_floats = bp.ws_frame_floats;
        long fs = 0;
        a.base[0] = c.band_ws;
        a.base[1] = const_cast<float*>(tensor_ptr(bp.stem_out, &fs));
        a.cv2 = bp.cv2 ? 1 : 0;
        a.xb = bp.xb ? 1 : 0;
        a.wide = bp.wide ? 1 : 0;
        for (size_t k = 0; k < bp.ext.size(); k++)
            a.base[2 + k] = bp.ext[k].out_k >= 0 ? c.out[static_cast<size_t>(bp.ext[k].out_k)] : tensor_ptr_mut(bp.ext[k].tensor, &fs);
        a.consts = c.band_consts; a.sync = c.band_sync; a.fail = c.band_fail;
        a.absent_mod = c.band_test_absent;
        set(l, Launcher::Bandnet, a, lab("bandnet_kernel"));
    }

    // The launch of node i; returns the plan nodes it stands for, from i on (more than one: it swallows the nodes behind it)
    size_t lower_node(size_t i, Launch& l) const {
        const Node& n = plan.nodes[i];
        if (n.kind == Node::Block) return block(i, l);
        const auto& si = shape(n.in[0]);
        const auto& so = shape(n.out);
        const Epilogue ep = epilogue(i);
        long in_fs = 0, out_fs = 0;
        const float* ip = tensor_ptr(n.in[0], &in_fs);
        float* op = tensor_ptr_mut(n.out, &out_fs);
        switch (n.kind) {
            case Node::Conv: return conv(i, l, ep, ip, in_fs, op, out_fs);
            case Node::Dw: {
                DwArgs a;
                a.in = ip; a.out = op; a.in_fs = in_fs; a.out_fs = out_fs;
                a.w = c.weights + pc.node_w[i];
                a.B = c.F; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.Ho = so[1]; a.Wo = so[2];
                a.KH = n.KH; a.KW = n.KW; a.sh = n.sh; a.sw = n.sw;
                if (n.padding == Padding::Same) { same_pad(a.H, a.KH, a.sh, a.Ho, &a.pt); same_pad(a.W, a.KW, a.sw, a.Wo, &a.pl); }
                if (n.ept >= 0) { a.pt = n.ept; a.pl = n.epl; }
                a.ep = ep;
                set(l, Launcher::Dw, a, lab("dw_kernel"));
                return 1;
            }
            case Node::Resident: resident(i, l, ip, in_fs, op, out_fs); return 1;
            case Node::Chain: chain(i, l, ip, in_fs, op, out_fs); return 1;
            default: {
                EltArgs a;
                a.a = ip; a.a_fs = in_fs; a.out = op; a.out_fs = out_fs; a.alpha = ep.alpha; a.act = n.act;
                a.B = c.F; a.H = dim(si, 1); a.W = dim(si, 2); a.C = si.back();
                a.Ho = dim(so, 1); a.Wo = dim(so, 2); a.Co = so.back();
                if (si.size() != 4) { a.H = 1; a.W = 1; a.C = static_cast<int>(g.tensors[n.in[0]].elems()); a.Ho = a.Wo = 1; a.Co = a.C; }
                if (n.kind == Node::Add) {
                    a.b = tensor_ptr(n.in[1], &a.b_fs);
                    set(l, Launcher::Add, a, lab("add_kernel"));
                } else if (n.kind == Node::Affine) {
                    if (si.size() != 4) { a.C = a.Co = si.back(); a.W = a.Wo = a.C > 0 ? static_cast<int>(g.tensors[n.in[0]].elems() / static_cast<size_t>(a.C)) : 0; }
                    a.b = weights(pc.node_w[i]);
                    a.shift = weights(pc.node_b[i]);
                    a.div = n.divide ? 1 : 0;
                    set(l, Launcher::Act, a, lab("affine_kernel"));   // (launch_act hands EltArgs with a shift to launch_affine)
                } else if (n.kind == Node::Act) {
                    set(l, Launcher::Act, a, lab("act_kernel"));
                } else if (n.kind == Node::MaxPool) {
                    a.p0 = n.filter_h; a.p1 = n.filter_w; a.p2 = n.sh; a.p3 = n.sw;
                    set(l, Launcher::Maxpool, a, lab("maxpool_kernel"));
                } else if (n.kind == Node::Pool) {
                    if (si.size() != 4 || so.size() != 4) throw std::runtime_error("internal: pool on a tensor that is not rank 4");
                    a.p0 = n.filter_h; a.p1 = n.filter_w; a.p2 = n.sh; a.p3 = n.sw;
                    set(l, Launcher::Avgpool, a, lab("avgpool_kernel"));
                } else if (n.kind == Node::L2Norm) {
                    // rows of D = the last dimension: [1,D] is one row a frame, [1,H,W,D] H * W of them
                    a.C = a.Co = si.back();
                    a.H = a.Ho = 1;
                    a.W = a.Wo = a.C > 0 ? static_cast<int>(g.tensors[n.in[0]].elems() / static_cast<size_t>(a.C)) : 0;
                    set(l, Launcher::L2norm, a, lab(static_cast<long>(c.F) * a.W < kL2NormLaneRows ? "l2norm_rows_kernel<wave per row>" : "l2norm_rows_kernel<thread per row>"));
                } else if (n.kind == Node::Transpose) {
                    if (si.size() != 4 || so.size() != 4 || n.perm.size() != 4) throw std::runtime_error("internal: transpose on a tensor that is not rank 4");
                    a.p1 = n.perm[1]; a.p2 = n.perm[2]; a.p3 = n.perm[3];
                    set(l, Launcher::Transpose, a, lab(transpose_takes_tiled(a) ? "transpose_tiled_kernel" : "transpose_kernel"));
                } else if (n.kind == Node::Pad) {
                    const auto& pv = g.tensors[n.pads].i32;
                    if (pv[0] != 0 || pv[1] != 0) throw std::runtime_error("PAD on the batch axis unsupported");
                    a.p0 = pv[2]; a.p1 = pv[4]; a.p2 = pv[6];
                    set(l, Launcher::Padc, a, lab("pad_kernel"));
                } else if (n.kind == Node::Resize) {
                    a.p0 = n.half_pixel; a.p1 = n.align_corners;
                    set(l, Launcher::Resize2x, a, lab("resize_kernel"));
                } else if (n.kind == Node::DepthToSpace) {
                    a.p0 = n.block_size;
                    set(l, Launcher::DepthToSpace, a, lab("d2s_kernel"));
                } else {
                    throw std::runtime_error("internal: unhandled node kind");
                }
                return 1;
            }
        }
    }

    size_t conv(size_t i, Launch& l, const Epilogue& ep, const float* ip, long in_fs, float* op, long out_fs) const {
        const Node& n = plan.nodes[i];
        const auto& si = shape(n.in[0]);
        const auto& so = shape(n.out);
        if (n.gemm_head) {
            HeadGemmArgs h;
            h.in = ip; h.out = op; h.in_fs = in_fs; h.out_fs = out_fs;
            h.w = c.weights + pc.node_w[i];
            h.bias = ep.bias; h.alpha = ep.alpha; h.act = ep.act;
            h.B = c.F; h.K = si[1] * si[2] * si[3]; h.N = so[3];
            h.one_form = n.fc ? 1 : 0;   // (a FULLY_CONNECTED: an embedding's bits must not depend on how many items ran with it)
            set(l, Launcher::HeadGemm, h, lab(c.F <= 4 && !n.fc ? "head_dot_kernel" : "head_gemm_kernel"));   // (launch_head_gemm: a handful of frames take the dot-product form)
            return 1;
        }
        // the first convolution inside the launch of the pair of BlazeBlocks behind it (f32 pictures, from 32 frames on: mdblock_kernels.hip, MD::STEM)
        if (c.strip && c.stem_fuse && pc.node_stem[i] >= 0 && !c.u8_frames) {   // (pc.node_stem: the graph's side of the conditions, checked when the constants were packed)
            const size_t j = i + 1;
            if (pc.node_chain_pair[j] >= 0 && !sched.event_after[i] && sched.slot[j] < 0) {
                const Node& ch = plan.nodes[j];
                DblockArgs d = dblock_args(nullptr, 0, n.out, ch.out, ch.members[0], ch.members[1], pc.node_chain_pair[j], true);
                d.stem_in = ip; d.stem_in_fs = in_fs; d.stem_consts = c.weights + pc.node_stem[i];
                d.stem_hi = clamp_of(n.act);
                if (mdblock_kernel_supports(d)) {
                    set(l, Launcher::Mdblock, d, lab("mdblock_kernel<stem+pair>"));
                    return 2;
                }
            }
        }
        ConvArgs a;
        a.in = ip; a.out = op; a.in_fs = in_fs; a.out_fs = out_fs;
        a.w = c.weights + pc.node_w[i];
        a.B = c.F; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.Ho = so[1]; a.Wo = so[2]; a.Co = so[3]; a.Cop = (a.Co + 3) & ~3;
        a.KH = n.KH; a.KW = n.KW; a.sh = n.sh; a.sw = n.sw;
        if (n.padding == Padding::Same) { same_pad(a.H, a.KH, a.sh, a.Ho, &a.pt); same_pad(a.W, a.KW, a.sw, a.Wo, &a.pl); }
        if (n.ept >= 0) { a.pt = n.ept; a.pl = n.epl; }
        a.ep = ep;
        a.no_mfma = c.stem_mfma == 0 ? 1 : c.stem_mfma == 2 ? 2 : 0;
        a.w_rows = weights(pc.node_wrows[i]);
        a.mfma = c.conv_mfma ? 1 : 0;
        if (c.conv_bf16) {   // (planes that the constants were not packed with stay null, and the launch keeps its f32 kernel)
            a.bf16 = c.conv_bf16;
            a.w_bf16 = weights(pc.node_wbf16_hi[i]);
            a.w_bf16_lo = weights(pc.node_wbf16_lo[i]);
        }
        a.stem_run = c.stem_run;
        if (c.u8_frames && plan.storage[n.in[0]].root == plan.storage[g.inputs[0]].root) {
            if (!conv_takes_u8(a)) throw std::runtime_error("plan: this graph's first convolution has no u8 input form");
            a.in_u8 = c.u8_frames + static_cast<long>(c.chunk_start) * c.u8_frame_bytes;
            a.u8_lut = c.u8_lut; a.u8_frame_bytes = c.u8_frame_bytes; a.u8_row_bytes = c.u8_row_bytes;
        }
        set(l, Launcher::Conv, a, want_labels ? conv_kernel_label(a) : nullptr);
        return 1;
    }

    void resident(size_t i, Launch& l, const float* ip, long in_fs, float* op, long out_fs) const {
        const Node& n = plan.nodes[i];
        const auto& si = shape(n.in[0]);
        if (n.xc) {
            XcArgs a;
            a.in = ip; a.in_fs = in_fs; a.out = op; a.out_fs = out_fs;
            a.B = c.F; a.H = si[1]; a.W = si[2]; a.nstages = static_cast<int>(n.members.size());
            for (size_t k = 0; k < n.members.size(); k++) {
                const Node& m = n.members[k];
                const MemberOff& mo = pc.chain_off[i][k];
                XcStage& st = a.st[k];
                st.cblob = c.weights + mo.cblob;
                st.has_dw = m.w >= 0;
                st.w_pw = c.weights + mo.w2;
                st.C = shape(m.in[0])[3]; st.Co = shape(m.out)[3]; st.act = m.act;
                st.skip = m.res < 0 ? 0 : (m.res == m.in[0] ? 1 : (k >= 2 && m.res == n.members[k - 2].out ? 3 : 2));
                if (st.skip == 2) {
                    st.res = tensor_ptr(m.res, &st.res_fs);
                    st.res_C = shape(m.res)[3]; st.res_W = shape(m.res)[2];
                }
            }
            return set(l, Launcher::Xc, a, lab("xc_kernel"));
        }
        if (n.dblock) {
            DblockArgs a = dblock_args(ip, in_fs, n.in[0], n.out, n.members[0], n.members[1], pc.chain_off[i][1].mconsts, false);
            a.w1 = c.weights + pc.chain_off[i][0].w2;
            a.w2 = c.weights + pc.chain_off[i][1].w2;
            a.consts = c.weights + pc.chain_off[i][0].cblob;
            if (c.strip && mdblock_kernel_supports(a)) return set(l, Launcher::Mdblock, a, lab("mdblock_kernel"));
            return set(l, Launcher::Dblock, a, lab("dblock_kernel"));
        }
        if (n.bneck) {
            BneckArgs a;
            a.in = ip; a.in_fs = in_fs; a.out = op; a.out_fs = out_fs;
            a.B = c.F; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.Cm = shape(n.members[0].out)[3];
            a.nblocks = static_cast<int>(n.members.size() / 2);
            a.bands = n.res_bands;
            for (int k = 0; k < a.nblocks; k++) {
                const size_t ka = static_cast<size_t>(2 * k), kb = ka + 1;
                const MemberOff &ma = pc.chain_off[i][ka], &mb = pc.chain_off[i][kb];
                a.blocks[k].w1 = c.weights + ma.w2;
                a.blocks[k].w2 = c.weights + mb.w2;
                a.blocks[k].consts = c.weights + ma.cblob;
                a.blocks[k].hi1 = clamp_of(n.members[ka].act);
                a.blocks[k].hi2 = clamp_of(n.members[kb].act);
                a.blocks[k].act1 = n.members[ka].act;
                a.blocks[k].act2 = n.members[kb].act;
                a.blocks[k].mconsts = weights(mb.mconsts);
            }
            if (c.strip && mbneck_kernel_supports(a)) return set(l, Launcher::Mbneck, a, lab("mbneck_kernel"));
            return set(l, Launcher::Bneck, a, lab("bneck_kernel"));
        }
        if (n.tail) {
            TailLaunch a;
            a.prog = c.tail_progs + pc.node_prog[i];
            a.nstages = static_cast<int>(n.stages.size());
            a.B = c.F;
            a.frame_floats = n.tail_frame_floats;
            a.variant = c.tail_pre;
            // frames per workgroup: as many as keep every CU busy (a workgroup's stage costs the same few thousand cycles of
            // latency whether its pixel tiles are full or not), within what the CU's LDS holds
            const int gmax = std::max(1, (160 * 1024 - 1024) / (4 * n.tail_frame_floats));
            a.G = c.tail_g > 0 ? std::min(c.tail_g, gmax) : std::max(1, std::min(gmax, c.F / c.cu_count));
            a.bases = res_bases();
            return set(l, Launcher::Tail, a, lab("tail_kernel"));
        }
        ResLaunch a;
        a.prog = c.progs + pc.node_prog[i];
        a.nstages = static_cast<int>(n.stages.size());
        a.B = c.F;
        a.bands = n.res_bands;
        a.const_off = n.res_const_off;
        a.const_floats = n.res_const_floats;
        a.lds_bytes = n.res_lds_bytes;
        a.bases = res_bases();
        set(l, Launcher::Resident, a, lab("resident_kernel"));
    }

    void chain(size_t i, Launch& l, const float* ip, long in_fs, float* op, long out_fs) const {
        const Node& n = plan.nodes[i];
        const auto& si = shape(n.in[0]);
        const auto& so = shape(n.out);
        char buf[112];
        ChainArgs a;
        auto fill = [&](ChainBlock& cb, size_t k) {
            const MemberOff& mo = pc.chain_off[i][k];
            cb.w_dw = c.weights + mo.w;
            cb.b_dw = weights(mo.b);
            cb.w_pw = c.weights + mo.w2;
            cb.bias = weights(mo.b2);
            cb.alpha = weights(mo.alpha);
            cb.act = n.members[k].act;
            cb.has_res = n.members[k].res >= 0;
        };
        auto chain_label = [&](int channels) {
            snprintf(buf, sizeof buf, "chain_kernel<%d>", (channels + 31) / 32);
            return lab(buf);
        };
        if (n.chain_pre || n.chain_post || !n.head_pairs.empty()) {  // frame-resident chain with stride-2 blocks around it and / or output heads in the same launch
            const size_t k0 = n.chain_pre ? 1 : 0, k1 = n.members.size() - (n.chain_post ? 1 : 0);
            const auto& sm = shape(n.members[k0].in[0]);  // the resident frame
            a.B = c.F; a.H = sm[1]; a.W = sm[2]; a.C = sm[3]; a.nblocks = static_cast<int>(k1 - k0);
            for (size_t k = k0; k < k1; k++) fill(a.blocks[k - k0], k);
            const int t_main = n.members[k1 - 1].out;   // the chain's own output tensor
            a.write_out = n.out == t_main || std::find(n.extra_out.begin(), n.extra_out.end(), t_main) != n.extra_out.end();
            if (a.write_out) { a.out = tensor_ptr_mut(t_main, &a.out_fs); } else { a.out = op; a.out_fs = out_fs; }
            a.in = ip; a.in_fs = in_fs;
            if (n.chain_pre) {
                a.pre.on = 1; fill(a.pre.blk, 0);
                a.pre.in = ip; a.pre.in_fs = in_fs; a.pre.Cin = si[3];
            }
            if (n.chain_post) {
                const int t_post = n.members.back().out;
                a.post.on = 1; fill(a.post.blk, n.members.size() - 1);
                a.post.out = tensor_ptr_mut(t_post, &a.post.out_fs);
                a.post.Co = shape(t_post)[3];
            }
            for (size_t k = 0; k < n.head_pairs.size(); k++) {
                const Node::HeadPair& hp = n.head_pairs[k];
                ChainHead& H = a.heads[hp.src];
                H.on = 1; H.src = hp.src;
                H.w_pw = c.weights + pc.chain_head_off[i][k].w2;
                H.bias = c.weights + pc.chain_head_off[i][k].b2;
                const int ta = n.head_nodes[static_cast<size_t>(hp.a)].out;
                H.Co_a = shape(ta).back();
                H.out_a = tensor_ptr_mut(ta, &H.out_a_fs);
                if (hp.b >= 0) {
                    const int tb = n.head_nodes[static_cast<size_t>(hp.b)].out;
                    H.Co_b = shape(tb).back();
                    H.out_b = tensor_ptr_mut(tb, &H.out_b_fs);
                }
            }
            if (!chain_kernel_supports(a)) throw std::runtime_error("chain node with edge stages without a kernel");
            return set(l, Launcher::Chain, a, chain_label(n.chain_pre || n.chain_post ? sm.back() : so.back()));
        }
        a.in = ip; a.out = op; a.in_fs = in_fs; a.out_fs = out_fs;
        a.B = c.F; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.nblocks = static_cast<int>(n.members.size());
        if (a.nblocks <= kMaxChain && a.H * a.W <= 256 && chain_kernel_supports(a)) {  // frame-resident in LDS
            for (size_t k = 0; k < n.members.size(); k++) fill(a.blocks[k], k);
            return set(l, Launcher::Chain, a, chain_label(so.back()));
        }
        if (c.strip && pc.node_chain_pair[i] >= 0) {   // a pair of plain BlazeBlocks with an operand-layout form
            const DblockArgs d = dblock_args(ip, in_fs, n.in[0], n.out, n.members[0], n.members[1], pc.node_chain_pair[i], true);
            if (mdblock_kernel_supports(d)) return set(l, Launcher::Mdblock, d, lab("mdblock_kernel<pair>"));
        }
        // row-pipelined group of strip blocks: only the first input and the last output exist in memory
        std::vector<BlockArgs> blk(n.members.size());
        for (size_t k = 0; k < n.members.size(); k++) {
            const MemberOff& mo = pc.chain_off[i][k];
            const Node& m = n.members[k];
            BlockArgs& b = blk[k];
            b.in = ip; b.out = op; b.in_fs = in_fs; b.out_fs = out_fs;
            b.has_dw = 1;
            b.pipe_rows = c.pipe_rows;
            b.pipe_band = c.pipe_band;
            b.w_dw = c.weights + mo.w;
            b.b_dw = weights(mo.b);
            b.w_pw = c.weights + mo.w2;
            b.w_strip = weights(mo.strip);
            b.B = c.F; b.H = si[1]; b.W = si[2]; b.C = si[3]; b.Ho = si[1]; b.Wo = si[2]; b.Co = si[3];
            b.sh = b.sw = 1; b.pt = b.pl = 1;
            b.ep.bias = weights(mo.b2);
            b.ep.alpha = weights(mo.alpha);
            b.ep.act = m.act;
            if (m.res >= 0) { b.ep.res = b.in; b.ep.res_fs = b.in_fs; b.ep.res_C = b.C; b.ep.res_mode = RES_DIRECT; }
            if (m.sh == 2) {  // stride-2 tail: halves the resolution, 2x2 max-pool skip from its (never materialised) input
                b.sh = b.sw = 2; b.pt = b.pl = 0;
                b.Ho = so[1]; b.Wo = so[2]; b.Co = so[3];
                if (m.res >= 0) { b.ep.res_mode = RES_MAXPOOL; b.ep.res_H = b.H; b.ep.res_W = b.W; }
            }
        }
        // Small batches: a row pipeline is a chain of 2S + rows/2 dependent steps of ~5 us whatever the batch (88 us per launch for ONE
        // BackCamera frame, four such launches of its 0.6 ms), while one strip-kernel launch per block is hundreds of independent
        // waves (~5 us).  Below `small_chain` frames the members run one launch each, ping-ponging through a per-handle scratch.
        if (c.small_chain > 0 && c.F <= c.small_chain && c.lanes == 1 && c.small) {
            const int nb = static_cast<int>(blk.size());
            const long fsz = static_cast<long>(si[1]) * si[2] * si[3];
            float* T[2] = {c.small, c.small + static_cast<size_t>(c.small_chain) * fsz};
            std::vector<BlockArgs> sb = blk;
            const float* cur = ip;
            long cur_fs = in_fs;
            bool ok = static_cast<size_t>(2 * c.small_chain) * fsz <= c.small_floats;
            for (int k = 0; k < nb && ok; k++) {
                BlockArgs& b = sb[static_cast<size_t>(k)];
                b.in = cur; b.in_fs = cur_fs;
                if (b.ep.res_mode != RES_NONE) { b.ep.res = cur; b.ep.res_fs = cur_fs; }
                if (k == nb - 1) { b.out = op; b.out_fs = out_fs; } else { b.out = T[k & 1]; b.out_fs = fsz; }
                ok = b.sh == 1 ? strip_kernel_supports(b) : block_kernel_supports(b);   // (the stride-2 member too, or the run fails where the row pipeline below would have taken it)
                cur = b.out; cur_fs = b.out_fs;
            }
            if (ok) {
                l.to = Launcher::SmallChain;
                if (want_labels) {
                    char name[48];
                    const bool s2 = sb[static_cast<size_t>(nb - 1)].sh == 2;
                    snprintf(buf, sizeof buf, "%s x%d%s (small batch)", strip_kernel_label(sb[0], name, sizeof name), s2 ? nb - 1 : nb, s2 ? " + block_kernel" : "");
                    l.label = buf;
                }
                l.blocks = std::move(sb);
                return;
            }
        }
        if (!strip_pipe_supports(blk.data(), static_cast<int>(blk.size()))) throw std::runtime_error("chain node without a kernel");
        l.to = Launcher::StripPipe;
        if (want_labels) l.label = strip_pipe_label(blk.data(), static_cast<int>(blk.size()), buf, sizeof buf);
        l.blocks = std::move(blk);
    }

    size_t block(size_t i, Launch& l) const {
        const Node& n = plan.nodes[i];
        const BlockArgs a = block_args(i);
        char buf[96];
        // this block and the next one as ONE launch (mdblock_kernel, pair form): the tensor between them is neither written nor read
        if (c.strip && c.pair_fuse && pc.node_pair[i] >= 0 && i + 1 < plan.nodes.size() && !sched.event_after[i] && sched.slot[i + 1] < 0 && sched.slot[i] < 0) {
            const Node& nb = plan.nodes[i + 1];
            const DblockArgs d = dblock_args(a.in, a.in_fs, n.in[0], nb.out, n, nb, pc.node_pair[i], true);
            // (the launch reads its input while it writes its output: the arena keeps the two apart — plan.cpp, liveness — and this checks it)
            const bool apart = d.out + d.out_fs * c.F <= d.in || d.in + d.in_fs * c.F <= d.out;
            if (apart && mdblock_kernel_supports(d)) {
                set(l, Launcher::Mdblock, d, lab("mdblock_kernel<pair>"));
                return 2;
            }
        }
        if (c.strip && ms2_kernel_supports(a)) {
            set(l, Launcher::Ms2, a, want_labels ? ms2_kernel_label(a, buf, sizeof buf) : nullptr);
            return 1;
        }
        if (c.strip && mwalk_kernel_supports(a)) {
            set(l, Launcher::Mwalk, a, want_labels ? mwalk_kernel_label(a, buf, sizeof buf) : nullptr);
            return 1;
        }
        const bool strip = c.strip && strip_kernel_supports(a);
        const bool mstrip = c.strip && !strip && mstrip_kernel_supports(a);
        if (mstrip && c.mchain && c.lanes == 1) {
            // the blocks behind this one that the same kernel takes, each reading its predecessor's output: ONE launch for the run
            // (every intermediate tensor keeps its arena slot; a workgroup per frame walks through the blocks)
            std::vector<BlockArgs> run{a};
            for (size_t j = i + 1; j < plan.nodes.size() && run.size() < 8; j++) {
                const Node& m = plan.nodes[j];
                if (m.kind != Node::Block || m.w < 0 || m.in.size() != 1 || m.in[0] != plan.nodes[j - 1].out || pc.node_strip[j] < 0 || sched.slot[j] >= 0) break;
                if (shape(m.in[0]).size() != 4 || shape(m.out) != shape(m.in[0]) || m.ept >= 0) break;
                if (m.res >= 0 && (m.res != m.in[0] || m.res_mode != RES_DIRECT || m.res_after)) break;
                run.push_back(block_args(j));
                if (!mstrip_chain_supports(run.data(), static_cast<int>(run.size()))) { run.pop_back(); break; }
            }
            if (run.size() >= 2) {
                l.to = Launcher::MstripChain;
                if (want_labels) { snprintf(buf, sizeof buf, "mstrip_chain_kernel<%d,%d>", a.C / 4, a.ep.act == ACT_RELU ? 1 : 0); l.label = buf; }
                l.blocks = std::move(run);
                return l.blocks.size();
            }
        }
        if (strip) set(l, Launcher::Strip, a, want_labels ? strip_kernel_label(a, buf, sizeof buf) : nullptr);
        else if (mstrip) set(l, Launcher::Mstrip, a, want_labels ? mstrip_kernel_label(a, buf, sizeof buf) : nullptr);
        else set(l, Launcher::Block, a, want_labels ? block_kernel_label(a, buf, sizeof buf) : nullptr);
        return 1;
    }
};

}  // namespace

Lowered lower_chunk(const Plan& plan, const PlanConsts& consts, const BandPlan& bp, const SideSchedule& sched, const LaunchCtx& c, bool want_labels) {
    const Lowering lo{plan, consts, bp, sched, c, want_labels};
    const size_t N = plan.nodes.size();
    Lowered out;
    out.launch_of_node.assign(N, -1);
    int band_launch = -1;
    for (size_t i = 0; i < N;) {
        const Node& n = plan.nodes[i];
        if (is_view(n)) { i++; continue; }
        if (c.band && band_cut(bp, i)) {
            if (band_launch < 0) {
                band_launch = static_cast<int>(out.launches.size());
                out.launches.emplace_back();
                Launch& l = out.launches.back();
                l.node = static_cast<int>(i);
                lo.band_launch(l);
            }
            // launches behind the program that run beside the trunk wait for the node that made their input: every such node inside the
            // program is this launch
            Launch& l = out.launches[static_cast<size_t>(band_launch)];
            l.last = static_cast<int>(i);
            l.record |= c.fork && sched.event_after[i];
            out.launch_of_node[i++] = band_launch;
            continue;
        }
        out.launches.emplace_back();
        Launch& l = out.launches.back();
        l.node = static_cast<int>(i);
        // (a whole-frame convolution right behind the band launch stays on the trunk: the face mesh's two heads are 9 + 11 us, a side stream's
        // events cost more than they hide — FaceLandmark::infer 208 us forked, 190 us in line)
        const bool in_line = c.band && n.gemm_head && sched.wait[i] >= 0 && !bp.node_runs[static_cast<size_t>(sched.wait[i])];
        if (c.fork && sched.slot[i] >= 0 && !in_line) { l.slot = sched.slot[i]; l.wait = sched.wait[i]; }
        const size_t covered = lo.lower_node(i, l);
        for (size_t k = 0; k < covered; k++) {
            out.launch_of_node[i + k] = static_cast<int>(out.launches.size()) - 1;
            l.record |= c.fork && sched.event_after[i + k];
        }
        l.last = static_cast<int>(i + covered - 1);
        i += covered;
    }
    return out;
}

}  // namespace mi
