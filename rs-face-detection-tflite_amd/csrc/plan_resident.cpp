// plan_resident.cpp — level 5 of the lowering: the small-spatial parts become frame-resident launches (see plan.hpp).
#include "plan_internal.hpp"

#include <cstdlib>
#include <map>

namespace mi {
namespace plan_detail {
namespace {

// Does anybody but the nodes [first, last] read t?  (Readers with the group's own range left out: its members hand t on inside the launch.)
bool read_outside(const std::vector<Node>& ns, int t, size_t first, size_t last) { return Readers{ns, nullptr, 0, first, last}.any(t); }

// Level 5, step 2: one candidate group = plan nodes [i, j].  Builds the stage list and places the in-group activations in
// LDS (first fit by liveness; a block whose skip is its own LDS-resident, now dead, same-shape input tensor is updated in
// place).  Returns false when a node has no stage form or the program does not fit in `budget` bytes of LDS.
bool build_resident(const Graph& g, const std::vector<Node>& ns, size_t i, size_t j, int budget, Node* out) {
    std::vector<Node> M;
    for (size_t k = i; k <= j; k++) {
        const Node& n = ns[k];
        if (n.kind == Node::Chain) {
            const auto& si = g.tensors[n.in[0]].shape;
            if (si[1] * si[2] > 256 || n.chain_pre || n.chain_post || !n.head_pairs.empty()) return false;  // row-pipelined chains and chains with stride-2 edge stages / output heads stay what they are
            for (const Node& m : n.members) M.push_back(m);
        } else if (n.kind == Node::Conv && n.gemm_head) {
            return false;  // a whole-frame convolution is a GEMM over the batch: its weights are read once per 32 frames there, once per frame here
        } else if (n.kind == Node::Block || n.kind == Node::Conv) {
            M.push_back(n);
        } else {
            return false;
        }
    }
    auto shp = [&](int t) -> const std::vector<int>& { return g.tensors[t].shape; };
    std::map<int, int> made;  // tensor -> member that produces it
    for (size_t m = 0; m < M.size(); m++) made[M[m].out] = static_cast<int>(m);
    auto external = [&](int t) { return is_graph_output(g, t) || read_outside(ns, t, i, j); };  // (the group's own rule: a graph output is a reader, its own nodes are not)
    struct Lt { int H, W, C, b = 0, def = -1, last = -1, off = -1; bool in_lds = false; };
    std::map<int, Lt> lt;
    auto geom = [&](int t) -> Lt& {
        auto it = lt.find(t);
        if (it == lt.end()) {
            Lt x;
            x.H = shp(t)[1]; x.W = shp(t)[2]; x.C = shp(t)[3];
            it = lt.emplace(t, x).first;
        }
        return it->second;
    };
    // ---- pass 1: stages with tensor ids
    std::vector<Node::Stage> S;
    std::vector<int> ext_in, ext_out;
    auto add_ext_in = [&](int t) { if (std::find(ext_in.begin(), ext_in.end(), t) == ext_in.end()) ext_in.push_back(t); };
    for (size_t m = 0; m < M.size(); m++) {
        const Node& n = M[m];
        if (n.in.size() != 1 || n.res_after) return false;
        const int src = n.in[0];
        if (shp(src).size() != 4 || shp(n.out).size() != 4) return false;
        const int H = shp(src)[1], W = shp(src)[2], C = shp(src)[3];
        const int Ho = shp(n.out)[1], Wo = shp(n.out)[2], Co = shp(n.out)[3];
        if (C % 4 || Ho * Wo > 256 || H * W > 1024) return false;
        Node::Stage sg;
        ResStage& st = sg.st;
        sg.member = static_cast<int>(m);
        st.src_H = H; st.src_W = W; st.src_C = C;
        st.Ho = Ho; st.Wo = Wo; st.Co = Co;
        st.act = n.act;
        const bool src_inside = made.count(src) && made[src] < static_cast<int>(m);
        if (n.kind == Node::Block && n.w >= 0) {
            if (n.KH != 3 || n.KW != 3 || n.sh != n.sw || (n.sh != 1 && n.sh != 2) || n.padding != Padding::Same) return false;
            st.kind = RES_STAGE_DW;
            st.KH = st.KW = 3; st.S = n.sh; st.Kv = C;
            st.pt = std::max(0, (Ho - 1) * n.sh + 3 - H) / 2;
            st.pl = std::max(0, (Wo - 1) * n.sw + 3 - W) / 2;
            if ((Ho - 1) * n.sh + 2 - st.pt > H || (Wo - 1) * n.sw + 2 - st.pl > W) return false;  // one border pixel covers the overhang
            if (!src_inside && !lt.count(src)) {  // bring the frame into LDS first
                Node::Stage ld;
                ld.st.kind = RES_STAGE_LOAD;
                ld.st.src_H = H; ld.st.src_W = W; ld.st.src_C = C;
                ld.src_t = src;
                ld.dst_t = src;
                Lt& x = geom(src);
                x.in_lds = true; x.def = static_cast<int>(S.size());
                S.push_back(ld);
                add_ext_in(src);
            }
            Lt& x = geom(src);
            if (!x.in_lds) return false;
            x.b = 1;
        } else {
            int K = 1;
            if (n.kind == Node::Conv) {
                if (n.KH != n.KW || n.res >= 0) return false;
                if (n.ept >= 0 || n.epl >= 0) return false;  // a folded spatial PAD: the k x k stride-k gather has no border
                K = n.KH;
                const bool whole = H == K && W == K;  // the window is the frame: one output pixel whatever the stride
                if (!whole && (n.sh != K || n.sw != K || H % K || W % K)) return false;
                if (Ho != H / K || Wo != W / K) return false;
            } else if (n.kind != Node::Block) {
                return false;
            }
            st.kind = RES_STAGE_GATHER;
            st.KH = st.KW = K; st.S = K; st.Kv = K * K * C;
            if (src_inside || lt.count(src)) {
                if (!geom(src).in_lds) return false;
            } else {
                sg.src_t = src;  // gathered straight from global memory
                add_ext_in(src);
            }
        }
        if (lt.count(src) && lt[src].in_lds) lt[src].last = static_cast<int>(S.size());
        if (n.res >= 0) {
            const auto& sr = shp(n.res);
            if (sr.size() != 4 || sr[3] % 4 || sr[3] > Co) return false;
            if (n.res_mode == RES_DIRECT) { if (sr[1] != Ho || sr[2] != Wo) return false; }
            else if (n.res_mode == RES_MAXPOOL) { if (sr[1] != 2 * Ho || sr[2] != 2 * Wo) return false; }
            else return false;
            st.res_mode = n.res_mode; st.res_C = sr[3]; st.res_H = sr[1]; st.res_W = sr[2];
            if (lt.count(n.res) && lt[n.res].in_lds) {
                lt[n.res].last = static_cast<int>(S.size());
            } else if (made.count(n.res) && made[n.res] < static_cast<int>(m)) {
                return false;  // produced inside but not kept: cannot happen (marked below), defensive
            } else {
                sg.res_t = n.res;
                add_ext_in(n.res);
            }
        }
        // where the output goes
        const bool used_inside = Readers{M, nullptr, m + 1}.any(n.out);
        const bool ext = external(n.out);
        if (!used_inside && !ext) return false;
        if (used_inside) {
            if (Co % 4) return false;
            Lt& y = geom(n.out);
            y.in_lds = true; y.def = static_cast<int>(S.size());
        }
        if (ext) { sg.dst_t = n.out; ext_out.push_back(n.out); }
        S.push_back(sg);
    }
    if (ext_out.empty() || ext_in.size() + ext_out.size() > 12) return false;
    // ---- pass 2: LDS placement in stage order
    struct Live { int off, size, t; };
    std::vector<Live> live;
    struct Clean { int off, size, H, W, C, b; };
    std::vector<Clean> clean;
    int high = 0, const_max = 0;
    auto size_of = [&](const Lt& x) { return (x.H + 2 * x.b) * (x.W + 2 * x.b) * (x.C + 4); };
    for (size_t k = 0; k < S.size(); k++) {
        Node::Stage& sg = S[k];
        ResStage& st = sg.st;
        const int src = sg.member >= 0 ? M[sg.member].in[0] : sg.src_t;
        const int dst = sg.member >= 0 ? M[sg.member].out : sg.dst_t;
        const int res = sg.member >= 0 ? M[sg.member].res : -1;
        live.erase(std::remove_if(live.begin(), live.end(), [&](const Live& l) { return lt[l.t].last < static_cast<int>(k); }), live.end());
        if (st.kind != RES_STAGE_LOAD && lt.count(src) && lt[src].in_lds) {
            const Lt& x = lt[src];
            st.src_off = x.off; st.src_PS = x.C + 4; st.src_b = x.b;
        }
        if (res >= 0 && lt.count(res) && lt[res].in_lds) {
            const Lt& x = lt[res];
            st.res_off = x.off; st.res_PS = x.C + 4; st.res_b = x.b;
        }
        if (lt.count(dst) && lt[dst].in_lds && lt[dst].def == static_cast<int>(k)) {
            Lt& y = lt[dst];
            if (y.last < static_cast<int>(k)) y.last = static_cast<int>(k);
            const int size = size_of(y);
            bool placed = false;
            if (st.kind != RES_STAGE_LOAD && res >= 0 && res != src && st.res_off >= 0 && st.res_mode == RES_DIRECT) {
                const Lt& r = lt[res];
                if (r.last == static_cast<int>(k) && r.H == y.H && r.W == y.W && r.C == y.C && r.b == y.b) {  // in place on the skip tensor
                    y.off = r.off;
                    for (Live& l : live) if (l.t == res) l.t = dst;
                    placed = true;
                }
            }
            if (!placed) {
                std::sort(live.begin(), live.end(), [](const Live& a, const Live& b) { return a.off < b.off; });
                int off = 0;
                for (const Live& l : live) {
                    if (off + size <= l.off) break;
                    off = std::max(off, l.off + l.size);
                }
                y.off = off;
                live.push_back({off, size, dst});
                high = std::max(high, off + size);
                bool same = false;
                for (const Clean& c : clean) same |= c.off == off && c.size == size && c.H == y.H && c.W == y.W && c.C == y.C && c.b == y.b;
                if (!same) {
                    clean.erase(std::remove_if(clean.begin(), clean.end(), [&](const Clean& c) { return c.off < off + size && off < c.off + c.size; }), clean.end());
                    clean.push_back({off, size, y.H, y.W, y.C, y.b});
                    st.zero_dst = size;
                }
            }
            st.dst_off = y.off; st.dst_PS = y.C + 4; st.dst_b = y.b;
        }
        const_max = std::max(const_max, resident_const_floats(st));
    }
    // LDS layout: [activations | constants, two halves (stage s computes from one while s+1's land in the other) | depthwise scratch]
    if (const_max > kResConstMax) return false;
    // Depthwise batches: enough pixel groups per batch to give each of the 8 waves a unit — unless smaller batches let two
    // workgroups share a CU (half of its 160 KB each), which hides more latency than full batches do.
    const int base_floats = ((high + 3) & ~3) + 2 * const_max;
    auto scratch_for = [&](int cap_pg) {
        int mx = 0;
        for (Node::Stage& sg : S) {
            ResStage& st = sg.st;
            if (st.kind != RES_STAGE_DW) continue;
            const int MT = (st.Co + 31) / 32, PGn = (st.Ho * st.Wo + 31) / 32, Cp = (st.Kv + 7) & ~7;
            st.dw_pg = std::max(1, std::min(std::min(PGn, cap_pg), (8 + MT - 1) / MT));
            mx = std::max(mx, st.dw_pg * 32 * (Cp + 4));
        }
        return mx;
    };
    // pointwise stages that read global memory stage their source through per-wave LDS slabs (K-blocked contraction order)
    bool slabs = false;
    for (Node::Stage& sg : S) {
        ResStage& st = sg.st;
        if (st.kind == RES_STAGE_GATHER && st.src_off < 0 && st.KH == 1 && st.Kv % 16 == 0) { st.kblk = 16; slabs = true; }
    }
    const int half_cu = 80 * 1024 / 4;
    int scratch_max = scratch_for(8);
    for (int cap = 4; cap >= 1 && base_floats + scratch_max > half_cu && base_floats + scratch_for(1) <= half_cu; cap /= 2) scratch_max = scratch_for(cap);
    if (base_floats + scratch_max > half_cu) scratch_max = scratch_for(8);
    if (slabs && base_floats + std::max(scratch_max, kResSlabFloats) > half_cu && base_floats + scratch_max <= half_cu) {
        slabs = false;  // the slabs would cost the second workgroup per CU: keep the direct gather here
        for (Node::Stage& sg : S) sg.st.kblk = 0;
    }
    if (slabs) scratch_max = std::max(scratch_max, kResSlabFloats);
    Node r;
    r.kind = Node::Resident;
    r.res_const_off = (high + 3) & ~3;
    r.res_const_floats = const_max;
    const int dw_off = r.res_const_off + 2 * const_max;
    for (Node::Stage& sg : S)
        if (sg.st.kind == RES_STAGE_DW || sg.st.kblk) sg.st.dw_off = dw_off;
    r.res_lds_bytes = (dw_off + scratch_max) * 4;
    if (r.res_lds_bytes > budget) return false;
    r.members = std::move(M);
    r.stages = std::move(S);
    r.in = ext_in;
    r.out = ext_out.back();
    ext_out.pop_back();
    r.extra_out = ext_out;
    for (size_t k = i; k <= j; k++) r.src_ops.insert(r.src_ops.end(), ns[k].src_ops.begin(), ns[k].src_ops.end());
    *out = std::move(r);
    return true;
}

// Level 5, round 5: the same candidate group [i, j] as a stage program of tail_kernels.hip (several frames per workgroup, every LDS
// tensor a dense borderless [pixels][C + 4] array, 16x16x4 MFMAs).  Also takes the frame-resident chains with their stride-2
// neighbours (the face mesh's 24x24 -> 12x12 x2 -> 6x6 and 6x6 x3 -> 3x3 launches): a BlazeBlock updates its input tensor in place, the
// stride-2 block in front reads its taps from global memory.  Placement by liveness, the depthwise scratch included.
bool build_tail(const Graph& g, const std::vector<Node>& ns, size_t i, size_t j, Node* out) {
    std::vector<Node> M;
    for (size_t k = i; k <= j; k++) {
        const Node& n = ns[k];
        if (n.kind == Node::Chain) {
            if (!n.head_pairs.empty()) return false;  // chains with output heads stay on chain_kernels.hip
            const auto& sr = g.tensors[n.members[n.chain_pre ? 1 : 0].in[0]].shape;  // the resident frame
            if (sr.size() != 4 || sr[1] * sr[2] > 256) return false;                  // row-pipelined chains
            for (const Node& m : n.members) M.push_back(m);
        } else if (n.kind == Node::Conv && n.gemm_head) {
            return false;
        } else if (n.kind == Node::Block || n.kind == Node::Conv) {
            M.push_back(n);
        } else {
            return false;
        }
    }
    auto shp = [&](int t) -> const std::vector<int>& { return g.tensors[t].shape; };
    std::map<int, int> made;
    for (size_t m = 0; m < M.size(); m++) made[M[m].out] = static_cast<int>(m);
    auto external = [&](int t) { return is_graph_output(g, t) || read_outside(ns, t, i, j); };
    struct Lt { int H = 0, W = 0, C = 0, def = -1, last = -1, off = -1; bool in_lds = false; };
    std::map<int, Lt> lt;
    auto geom = [&](int t) -> Lt& {
        auto it = lt.find(t);
        if (it == lt.end()) {
            Lt x;
            x.H = shp(t)[1]; x.W = shp(t)[2]; x.C = shp(t)[3];
            it = lt.emplace(t, x).first;
        }
        return it->second;
    };
    std::vector<Node::Stage> S;
    std::vector<int> ext_in, ext_out;
    auto add_ext_in = [&](int t) { if (std::find(ext_in.begin(), ext_in.end(), t) == ext_in.end()) ext_in.push_back(t); };
    auto in_lds = [&](int t) { return lt.count(t) && lt[t].in_lds; };
    auto load = [&](int t) {   // bring an external frame into LDS
        const auto& s = shp(t);
        if (s[3] % 4 || static_cast<long>(s[1]) * s[2] * (s[3] + 4) * 4 > 150 * 1024) return false;
        Node::Stage ld;
        ld.tst.kind = TAIL_LOAD;
        ld.tst.src_H = s[1]; ld.tst.src_W = s[2]; ld.tst.src_C = s[3];
        ld.tst.mHW = tail_magic(s[1] * s[2] * (s[3] / 4)); ld.tst.mW = tail_magic(s[3] / 4);
        ld.src_t = t; ld.dst_t = t;
        Lt& x = geom(t);
        x.in_lds = true; x.def = static_cast<int>(S.size());
        S.push_back(ld);
        add_ext_in(t);
        return true;
    };
    int min_px = 1 << 30;
    for (size_t m = 0; m < M.size(); m++) {
        const Node& n = M[m];
        if (n.in.size() != 1 || n.res_after || n.ept >= 0 || n.epl >= 0) return false;
        const int src = n.in[0];
        if (shp(src).size() != 4 || shp(n.out).size() != 4) return false;
        const int H = shp(src)[1], W = shp(src)[2], C = shp(src)[3];
        const int Ho = shp(n.out)[1], Wo = shp(n.out)[2], Co = shp(n.out)[3];
        if (C % 4 || Ho * Wo > 256 || H * W > 1024) return false;
        Node::Stage sg;
        TailStage& st = sg.tst;
        sg.member = static_cast<int>(m);
        st.src_H = H; st.src_W = W; st.src_C = C;
        st.Ho = Ho; st.Wo = Wo; st.Co = Co;
        st.mHW = tail_magic(Ho * Wo); st.mW = tail_magic(Wo);
        st.act = n.act;
        const bool src_inside = made.count(src) && made[src] < static_cast<int>(m);
        if (src_inside && !in_lds(src)) return false;
        // where the output goes
        const bool used_inside = Readers{M, nullptr, m + 1}.any(n.out);
        const bool ext = external(n.out);
        if (!used_inside && !ext) return false;
        if (n.kind == Node::Block && n.w >= 0) {
            if (n.KH != 3 || n.KW != 3 || n.sh != n.sw || (n.sh != 1 && n.sh != 2) || n.padding != Padding::Same) return false;
            st.kind = TAIL_DW;
            st.K = 3; st.S = n.sh; st.Kv = C;
            st.mHWp = tail_magic(Ho * ((Wo + 1) / 2)); st.mWp = tail_magic((Wo + 1) / 2);
            st.pt = std::max(0, (Ho - 1) * n.sh + 3 - H) / 2;
            st.pl = std::max(0, (Wo - 1) * n.sw + 3 - W) / 2;
            if (!tail_stage_ok(TAIL_DW, 3, st.S, C, C, Co, used_inside)) return false;
            if (!in_lds(src)) {
                // a stride-1 block brings its frame in (its skip is the frame, and it updates it in place); a stride-2 block reads the
                // nine taps of a pixel straight from global memory (its input is four times the frame and often does not fit)
                if (n.sh == 1) { if (!load(src)) return false; }
                else { sg.src_t = src; add_ext_in(src); }
            }
        } else {
            int K = 1;
            if (n.kind == Node::Conv) {
                if (n.KH != n.KW || n.res >= 0) return false;
                K = n.KH;
                if (K != 1 && (K != 2 || n.sh != 2 || n.sw != 2 || H % 2 || W % 2)) return false;
                if (K == 1 && (n.sh != 1 || n.sw != 1)) return false;
                if (Ho != H / K || Wo != W / K) return false;
            } else if (n.kind != Node::Block) {
                return false;
            }
            st.kind = TAIL_GATHER;
            st.K = K; st.S = K; st.Kv = K * K * C;
            if (!tail_stage_ok(TAIL_GATHER, K, K, C, st.Kv, Co, used_inside)) return false;
            if (!in_lds(src) && !load(src)) return false;
        }
        if (in_lds(src)) lt[src].last = static_cast<int>(S.size());
        if (n.res >= 0) {
            const auto& sr = shp(n.res);
            if (sr.size() != 4 || sr[3] % 4 || sr[3] > Co) return false;
            if (n.res_mode == RES_DIRECT) { if (sr[1] != Ho || sr[2] != Wo) return false; }
            else if (n.res_mode == RES_MAXPOOL) { if (sr[1] != 2 * Ho || sr[2] != 2 * Wo) return false; }
            else return false;
            st.res_mode = n.res_mode; st.res_C = sr[3]; st.res_W = sr[2];
            if (in_lds(n.res)) {
                lt[n.res].last = static_cast<int>(S.size());
            } else if (made.count(n.res) && made[n.res] < static_cast<int>(m)) {
                return false;
            } else {
                sg.res_t = n.res;
                add_ext_in(n.res);
            }
        }
        if (used_inside) {
            Lt& y = geom(n.out);
            y.in_lds = true; y.def = static_cast<int>(S.size());
        }
        if (ext) { sg.dst_t = n.out; ext_out.push_back(n.out); }
        min_px = std::min(min_px, Ho * Wo);
        S.push_back(sg);
    }
    if (ext_out.empty() || ext_in.size() + ext_out.size() > 12) return false;
    // ---- LDS placement in stage order (floats per frame; the kernel multiplies every offset by the frames per workgroup)
    struct Live { int off, size, t; };   // t < 0: a depthwise scratch
    std::vector<Live> live;
    int high = 0;
    auto size_of = [&](const Lt& x) { return x.H * x.W * (x.C + 4); };
    auto place = [&](int size, int t) {
        std::sort(live.begin(), live.end(), [](const Live& a, const Live& b) { return a.off < b.off; });
        int off = 0;
        for (const Live& l : live) {
            if (off + size <= l.off) break;
            off = std::max(off, l.off + l.size);
        }
        live.push_back({off, size, t});
        high = std::max(high, off + size);
        return off;
    };
    for (size_t k = 0; k < S.size(); k++) {
        Node::Stage& sg = S[k];
        TailStage& st = sg.tst;
        const int src = sg.member >= 0 ? M[static_cast<size_t>(sg.member)].in[0] : sg.src_t;
        const int dst = sg.member >= 0 ? M[static_cast<size_t>(sg.member)].out : sg.dst_t;
        const int res = sg.member >= 0 ? M[static_cast<size_t>(sg.member)].res : -1;
        live.erase(std::remove_if(live.begin(), live.end(), [&](const Live& l) { return l.t < 0 || lt[l.t].last < static_cast<int>(k); }), live.end());
        if (st.kind != TAIL_LOAD && in_lds(src)) st.src_off = lt[src].off;
        if (st.kind != TAIL_LOAD && res >= 0 && in_lds(res)) st.res_off = lt[res].off;
        // (the output first: it outlives the stage's scratch, which then fills the space above it)
        if (in_lds(dst) && lt[dst].def == static_cast<int>(k)) {
            Lt& y = lt[dst];
            if (y.last < static_cast<int>(k)) y.last = static_cast<int>(k);
            bool placed = false;
            // in place on the skip tensor when it dies here: the lane that stores an output quad is the one that read the skip quad at
            // that address.  A depthwise stage may do so even when the skip is its own source (the taps went into the scratch before
            // the stage's barrier); a pointwise stage reads its source across lanes while others store.
            if (st.kind != TAIL_LOAD && res >= 0 && st.res_off >= 0 && st.res_mode == RES_DIRECT && (res != src || st.kind == TAIL_DW)) {
                const Lt& r = lt[res];
                if (r.last == static_cast<int>(k) && r.H == y.H && r.W == y.W && r.C == y.C) {
                    y.off = r.off;
                    for (Live& l : live) if (l.t == res) l.t = dst;
                    placed = true;
                }
            }
            if (!placed) y.off = place(size_of(y), dst);
            st.dst_off = y.off;
        }
        if (st.kind == TAIL_DW) {
            st.scr_off = place(st.Ho * st.Wo * (st.Kv + 4), -1);
            if (st.S == 2 && st.res_mode == RES_MAXPOOL && res == src && st.pt == 0 && st.pl == 0 && st.res_C == st.Kv) {
                const int before = high;
                st.pool_off = place(st.Ho * st.Wo * (st.Kv + 4), -1);
                if ((static_cast<long>(high) + 260) * 4 > 160 * 1024) { st.pool_off = -1; live.pop_back(); high = before; }   // no room: the epilogue pools from the source
            }
        }
    }
    const int frame_floats = (high + 3) & ~3;
    if ((static_cast<long>(frame_floats) + 256) * 4 > 160 * 1024) return false;
    Node r;
    r.kind = Node::Resident;
    r.tail = true;
    r.tail_frame_floats = frame_floats;
    r.tail_min_px = min_px;
    r.res_lds_bytes = (frame_floats + 256) * 4;
    r.members = std::move(M);
    r.stages = std::move(S);
    r.in = ext_in;
    r.out = ext_out.back();
    ext_out.pop_back();
    r.extra_out = ext_out;
    for (size_t k = i; k <= j; k++) r.src_ops.insert(r.src_ops.end(), ns[k].src_ops.begin(), ns[k].src_ops.end());
    *out = std::move(r);
    return true;
}

// Level 5, large frames: the bottleneck pair  r = act(PW(x));  y = act(PW(DW3x3(r)) + b + x')  (iris 32x32: 64 -> 32 -> 64
// channels) whose frame does not fit in LDS runs as ONE launch cut into row bands: a workgroup recomputes the one-row halo of
// r for its band, keeps r in LDS and reads x / x' and writes y in global memory — r never reaches HBM.
bool build_banded_bottleneck(const Graph& g, const std::vector<Node>& ns, size_t i, Node* out) {
    if (i + 1 >= ns.size()) return false;
    const Node &a = ns[i], &b = ns[i + 1];
    if (a.kind != Node::Block || a.w >= 0 || a.res >= 0 || a.in.size() != 1) return false;
    if (b.kind != Node::Block || b.w < 0 || b.in.size() != 1 || b.in[0] != a.out) return false;
    if (b.KH != 3 || b.KW != 3 || b.sh != 1 || b.sw != 1 || b.padding != Padding::Same) return false;
    if (b.res < 0 || b.res_mode != RES_DIRECT || b.res == b.in[0] || b.res_after) return false;
    if (is_graph_output(g, a.out) || read_outside(ns, a.out, i + 1, i + 1)) return false;  // r has one reader
    const auto &sx = g.tensors[a.in[0]].shape, &sr = g.tensors[a.out].shape, &sy = g.tensors[b.out].shape, &ss = g.tensors[b.res].shape;
    if (sx.size() != 4 || sr.size() != 4 || sy.size() != 4 || ss.size() != 4) return false;
    const int H = sx[1], W = sx[2], Cx = sx[3], Cr = sr[3], Cy = sy[3];
    if (sr[1] != H || sr[2] != W || sy[1] != H || sy[2] != W || ss[1] != H || ss[2] != W) return false;
    if (Cx % 4 || Cr % 4 || Cy % 4 || ss[3] % 4 || ss[3] > Cy || H * W <= 256 || W > 64) return false;
    Node::Stage p, c;
    ResStage& ps = p.st;
    ps.kind = RES_STAGE_GATHER; ps.src_H = H; ps.src_W = W; ps.src_C = Cx; ps.KH = ps.KW = 1; ps.S = 1; ps.Kv = Cx;
    ps.Wo = W; ps.Co = Cr; ps.act = a.act; ps.band_role = 1; ps.band_H = H;
    p.member = 0; p.src_t = a.in[0];
    ResStage& cs = c.st;
    cs.kind = RES_STAGE_DW; cs.src_W = W; cs.src_C = Cr; cs.src_PS = Cr + 4; cs.src_b = 1; cs.src_off = 0;
    cs.KH = cs.KW = 3; cs.S = 1; cs.pt = cs.pl = 1; cs.Kv = Cr; cs.Wo = W; cs.Co = Cy; cs.act = b.act;
    cs.res_mode = RES_DIRECT; cs.res_C = ss[3]; cs.res_H = H; cs.res_W = W; cs.band_role = 2; cs.band_H = H;
    c.member = 1; c.dst_t = b.out; c.res_t = b.res;
    const int MT = (Cy + 31) / 32, Cp = (Cr + 7) & ~7;
    const int const_max = std::max(resident_const_floats(ps), resident_const_floats(cs));
    if (const_max > kResConstMax) return false;
    // rows per band: as many as keep two workgroups on a CU (half of the 160 KB each)
    const int slab = Cx % 16 == 0 ? kResSlabFloats : 0;  // the pointwise stage stages x through per-wave LDS slabs
    int R = 0, total = 0, dw_pg = 1;
    for (int r = std::min(H, 32); r >= 2; r--) {
        const int buf = (r + 2) * (W + 2) * (Cr + 4);
        const int PGn = (r * W + 31) / 32;
        const int pg = std::max(1, std::min(PGn, (8 + MT - 1) / MT));
        const int t = ((buf + 3) & ~3) + 2 * const_max + std::max(pg * 32 * (Cp + 4), slab);
        if (t * 4 <= 80 * 1024 - 512) { R = r; total = t; dw_pg = pg; break; }
    }
    if (R < 2) return false;
    R = (H + ((H + R - 1) / R) - 1) / ((H + R - 1) / R);  // same band count, even bands
    const int buf = (R + 2) * (W + 2) * (Cr + 4);
    {
        const int PGn = (R * W + 31) / 32;
        dw_pg = std::max(1, std::min(PGn, (8 + MT - 1) / MT));
        total = ((buf + 3) & ~3) + 2 * const_max + std::max(dw_pg * 32 * (Cp + 4), slab);
    }
    if (slab) { ps.kblk = 16; }
    ps.Ho = R + 2; ps.band_rows = R; ps.dst_off = 0; ps.dst_PS = Cr + 4; ps.dst_b = 1; ps.zero_dst = buf;
    cs.src_H = R; cs.Ho = R; cs.band_rows = R; cs.dw_pg = dw_pg;
    Node r;
    r.kind = Node::Resident;
    r.res_const_off = (buf + 3) & ~3;
    r.res_const_floats = const_max;
    cs.dw_off = r.res_const_off + 2 * const_max;
    ps.dw_off = cs.dw_off;
    r.res_lds_bytes = total * 4;
    r.res_bands = (H + R - 1) / R;
    r.members = {a, b};
    r.stages = {p, c};
    r.in = {a.in[0]};
    if (b.res != a.in[0]) r.in.push_back(b.res);
    r.out = b.out;
    r.src_ops = a.src_ops;
    r.src_ops.insert(r.src_ops.end(), b.src_ops.begin(), b.src_ops.end());
    *out = std::move(r);
    return true;
}

// Level 5: runs of bottleneck pairs  r = act(PW(x));  y = act(PW(DW3x3(r)) + b + x)  on 64 / 128 channels (the iris network) for the
// register-resident kernel (bneck_kernels.hip): frames of <= 256 pixels take the whole run in one launch, larger frames one pair per
// launch in row bands of 256 pixels.  Returns the number of plan nodes consumed (0: no match).
size_t build_bneck(const Graph& g, const std::vector<Node>& ns, size_t i, Node* out) {
    auto pair_at = [&](size_t k, int x_t) {
        if (k + 1 >= ns.size()) return false;
        const Node &a = ns[k], &b = ns[k + 1];
        if (a.kind != Node::Block || a.w >= 0 || a.res >= 0 || a.in.size() != 1 || a.in[0] != x_t) return false;
        if (b.kind != Node::Block || b.w < 0 || b.in.size() != 1 || b.in[0] != a.out) return false;
        if (b.KH != 3 || b.KW != 3 || b.sh != 1 || b.sw != 1 || b.padding != Padding::Same || b.ept >= 0 || b.epl >= 0) return false;
        if (b.res != x_t || b.res_mode != RES_DIRECT || b.res_after) return false;
        if (is_graph_output(g, a.out) || read_outside(ns, a.out, k + 1, k + 1)) return false;  // r has one reader
        const auto &sx = g.tensors[x_t].shape, &sr = g.tensors[a.out].shape, &sy = g.tensors[b.out].shape;
        if (sx.size() != 4 || sr.size() != 4 || sy.size() != 4 || sy != sx || sr[1] != sx[1] || sr[2] != sx[2]) return false;
        return true;
    };
    if (i >= ns.size() || ns[i].in.size() != 1) return 0;
    const int x0 = ns[i].in[0];
    if (!pair_at(i, x0)) return 0;
    const auto& sx = g.tensors[x0].shape;
    const int H = sx[1], W = sx[2], C = sx[3], Cm = g.tensors[ns[i].out].shape[3];
    BneckArgs ba;
    ba.in = fake<const float>(kFakeIn); ba.out = fake<float>(kFakeOut);
    ba.in_fs = ba.out_fs = static_cast<long>(g.tensors[x0].elems());
    ba.B = 1; ba.H = H; ba.W = W; ba.C = C; ba.Cm = Cm;
    for (BneckBlock& bk : ba.blocks) { bk.w1 = bk.w2 = bk.consts = fake<const float>(kFakeAux); }
    size_t npairs = 1;
    if (H * W <= 256) {
        if (H * W < 128) return 0;  // a quarter of the waves would have pixels: the stage programs do these
        // the whole run: the next pair reads this pair's output, which nobody else may need before the run ends ... unless it is written
        int x = ns[i + 1].out;
        while (npairs < static_cast<size_t>(kMaxBneck) && pair_at(i + 2 * npairs, x)) {
            if (is_graph_output(g, x) || read_outside(ns, x, i + 2 * npairs, i + 2 * npairs + 1)) break;  // an intermediate frame that somebody else reads ends the run
            x = ns[i + 2 * npairs + 1].out;
            npairs++;
        }
        ba.bands = 1;
    } else {
        if (W > 256 || 256 / W < 2) return 0;
        const int R = 256 / W;
        ba.bands = (H + R - 1) / R;
    }
    ba.nblocks = static_cast<int>(npairs);
    if (!bneck_kernel_supports(ba)) return 0;
    Node r;
    r.kind = Node::Resident;
    r.bneck = true;
    r.res_bands = ba.bands;
    r.in = {x0};
    r.out = ns[i + 2 * npairs - 1].out;
    for (size_t k = i; k < i + 2 * npairs; k++) {
        r.members.push_back(ns[k]);
        r.src_ops.insert(r.src_ops.end(), ns[k].src_ops.begin(), ns[k].src_ops.end());
    }
    *out = std::move(r);
    return 2 * npairs;
}

// Level 5: full_range's double block  a = act(PW(DW3x3(x)));  y = act(PW(DW3x3(a)) + x)  (two stride-1 BlazeBlocks, the skip around
// both) as one launch of dblock_kernels.hip.  Returns the number of plan nodes consumed (0: no match).
size_t build_dblock(const Graph& g, const std::vector<Node>& ns, size_t i, Node* out) {
    if (i + 1 >= ns.size()) return 0;
    const Node &a = ns[i], &b = ns[i + 1];
    auto dw_block = [](const Node& n) {
        return n.kind == Node::Block && n.w >= 0 && n.KH == 3 && n.KW == 3 && n.sh == 1 && n.sw == 1 && n.padding == Padding::Same && n.ept < 0 && n.epl < 0 && n.in.size() == 1;
    };
    if (!dw_block(a) || !dw_block(b) || b.in[0] != a.out) return 0;
    // either the double block (no skip on the first half, the second half's skip is x) or two plain BlazeBlocks in a row (each adds its own input)
    const bool blaze_pair = a.res == a.in[0] && a.res_mode == RES_DIRECT && !a.res_after && b.res == a.out && b.res_mode == RES_DIRECT && !b.res_after;
    const bool dbl = a.res < 0 && b.res == a.in[0] && b.res_mode == RES_DIRECT && !b.res_after;
    // (the pair form is measured slower than two block-kernel launches — BackCamera 32x32x48: 0.107 against 2 x 0.040 ms, both stages are
    // heavy and the recomputed halo rows cost more than the saved round trip — and stays off unless asked for)
    static const bool pairs_on = getenv("MI_BLAZE_PAIRS") != nullptr;  // development aid
    if (!dbl && !(blaze_pair && pairs_on)) return 0;
    if (is_graph_output(g, a.out) || read_outside(ns, a.out, i + 1, i + 1)) return 0;  // a has one reader
    const auto &sx = g.tensors[a.in[0]].shape, &sa = g.tensors[a.out].shape, &sy = g.tensors[b.out].shape;
    if (sx.size() != 4 || sa.size() != 4 || sy.size() != 4 || sy[1] != sx[1] || sy[2] != sx[2] || sy[3] < sx[3] || sa[1] != sx[1] || sa[2] != sx[2]) return 0;
    if (sx[1] * sx[2] <= 256) return 0;  // small frames: the per-block launches with their tiles spread over the chip do better
    DblockArgs da;
    da.in = fake<const float>(kFakeIn); da.out = fake<float>(kFakeOut);
    da.in_fs = da.out_fs = static_cast<long>(g.tensors[a.in[0]].elems());
    da.B = 1; da.H = sx[1]; da.W = sx[2]; da.C = sx[3]; da.Cm = sa[3]; da.Co = sy[3];
    da.skip1 = blaze_pair; da.skip2_from_a = blaze_pair;
    da.out_fs = static_cast<long>(g.tensors[b.out].elems());
    da.consts = da.w1 = da.w2 = fake<const float>(kFakeAux);
    if (!dblock_kernel_supports(da)) return 0;
    Node r;
    r.kind = Node::Resident;
    r.dblock = true;
    r.in = {a.in[0]};
    r.out = b.out;
    r.members = {a, b};
    r.src_ops = a.src_ops;
    r.src_ops.insert(r.src_ops.end(), b.src_ops.begin(), b.src_ops.end());
    *out = std::move(r);
    return 2;
}

// Level 5: runs of stride-1 BlazeBlocks on tiny frames (<= 64 pixels) whose channel count alternates narrow -> wide -> narrow ...
// (full_range's 6x6x96 -> 384 -> 96 pairs) as one frame-resident launch of xc_kernels.hip.  Returns the number of plan nodes consumed (0: no match).
size_t build_xc(const Graph& g, const std::vector<Node>& ns, size_t i, Node* out) {
    static const bool off = getenv("MI_NO_XC") != nullptr;  // development aid
    if (off || i + 1 >= ns.size()) return 0;
    auto plain = [](const Node& n) {
        return n.kind == Node::Block && n.w >= 0 && n.KH == 3 && n.KW == 3 && n.sh == 1 && n.sw == 1 && n.padding == Padding::Same && n.ept < 0 && n.epl < 0 &&
               n.in.size() == 1 && !n.res_after && n.act != ACT_PRELU;
    };
    // (a contract stage may be pointwise only: the last block of full_range's 6x6 run)
    auto pointwise = [](const Node& n) { return n.kind == Node::Block && n.w < 0 && n.sh == 1 && n.sw == 1 && n.in.size() == 1 && !n.res_after && n.act != ACT_PRELU; };
    if (!plain(ns[i])) return 0;
    const auto& s0 = g.tensors[ns[i].in[0]].shape;
    if (s0.size() != 4 || s0[1] * s0[2] > 64) return 0;
    // skip of an expand stage: 0 none, 1 its own input, 2 the max-pooled previous resolution, 3 the wide tensor of the pair before (full_range's
    // double block: wide -> narrow -> wide with the skip around both), -1 something else
    auto skip_of = [&](size_t n) {
        const Node& m = ns[i + n];
        if (m.res < 0) return 0;
        const auto &sr = g.tensors[m.res].shape, &so = g.tensors[m.out].shape;
        if (sr.size() != 4 || sr[3] % 4 || sr[3] > so[3]) return -1;
        if (m.res == m.in[0]) return m.res_mode == RES_DIRECT ? 1 : -1;
        if (n >= 2 && m.res == ns[i + n - 2].out) return (m.res_mode == RES_DIRECT && sr == so) ? 3 : -1;
        return (m.res_mode == RES_MAXPOOL && sr[1] == 2 * s0[1] && sr[2] == 2 * s0[2]) ? 2 : -1;
    };
    size_t n = 0;
    while (n < static_cast<size_t>(kMaxXc) && i + n < ns.size()) {
        const Node& m = ns[i + n];
        if (!plain(m) && !((n & 1) && pointwise(m))) break;
        if (n > 0 && m.in[0] != ns[i + n - 1].out) break;
        const auto &si = g.tensors[m.in[0]].shape, &so = g.tensors[m.out].shape;
        if (si.size() != 4 || so.size() != 4 || so[1] != s0[1] || so[2] != s0[2] || si[1] != s0[1] || si[2] != s0[2]) break;
        if (n & 1) {   // contract: back to the narrow width, no skip
            if (m.res >= 0 || so[3] != s0[3]) break;
        } else {       // expand: from the narrow width
            if (si[3] != s0[3] || so[3] <= si[3]) break;
            if (n >= 2 && so[3] != g.tensors[ns[i].out].shape[3]) break;
            if (skip_of(n) < 0) break;
        }
        n++;
    }
    // whole pairs whose intermediate tensors nobody outside the run reads (and that are no graph outputs)
    auto internal_ok = [&](size_t len) {
        for (size_t k = 0; k + 1 < len; k++) {
            const int t = ns[i + k].out;
            if (is_graph_output(g, t) || read_outside(ns, t, i, i + len - 1)) return false;
        }
        return true;
    };
    n &= ~static_cast<size_t>(1);
    while (n >= 2 && !internal_ok(n)) n -= 2;
    if (n < 2) return 0;
    XcArgs xa;
    xa.in = fake<const float>(kFakeIn); xa.out = fake<float>(kFakeOut);
    xa.in_fs = xa.out_fs = static_cast<long>(g.tensors[ns[i].in[0]].elems());
    xa.B = 1; xa.H = s0[1]; xa.W = s0[2]; xa.nstages = static_cast<int>(n);
    std::vector<int> extra_in;
    for (size_t k = 0; k < n; k++) {
        const Node& m = ns[i + k];
        XcStage& st = xa.st[k];
        st.w_pw = st.cblob = fake<const float>(kFakeAux);
        st.has_dw = m.w >= 0;
        st.C = g.tensors[m.in[0]].shape[3]; st.Co = g.tensors[m.out].shape[3]; st.act = m.act;
        st.skip = (k & 1) ? 0 : skip_of(k);
        if (st.skip == 2) {
            st.res = fake<const float>(kFakeEdgeOut); st.res_fs = static_cast<long>(g.tensors[m.res].elems());
            st.res_C = g.tensors[m.res].shape[3]; st.res_W = g.tensors[m.res].shape[2];
            if (std::find(extra_in.begin(), extra_in.end(), m.res) == extra_in.end()) extra_in.push_back(m.res);
        }
    }
    if (!xc_kernel_supports(xa)) return 0;
    Node r;
    r.kind = Node::Resident;
    r.xc = true;
    r.in = {ns[i].in[0]};
    for (int t : extra_in) r.in.push_back(t);
    r.out = ns[i + n - 1].out;
    for (size_t k = i; k < i + n; k++) {
        r.members.push_back(ns[k]);
        r.src_ops.insert(r.src_ops.end(), ns[k].src_ops.begin(), ns[k].src_ops.end());
    }
    *out = std::move(r);
    return n;
}

}  // namespace

// Level 5, step 1: make independent branches contiguous.  TFLite serialises the two heads of the face-mesh / iris graphs
// op by op in alternation; following each producer by its (ready) consumer keeps a branch together so that it can become one
// stage program.  Only the order among independent nodes changes.
void reorder_branches(std::vector<Node>& ns) {
    const int N = static_cast<int>(ns.size());
    std::map<int, int> producer;
    for (int i = 0; i < N; i++) producer[ns[i].out] = i;
    std::vector<char> emitted(N, 0);
    std::vector<int> order;
    auto ready = [&](int k) {
        auto ok = [&](int t) {
            auto it = producer.find(t);
            return t < 0 || it == producer.end() || emitted[it->second];
        };
        for (int t : ns[k].in)
            if (!ok(t)) return false;
        return ok(ns[k].res);
    };
    auto reads = [&](const Node& n, int t) { return std::find(n.in.begin(), n.in.end(), t) != n.in.end() || n.res == t; };
    for (int i = 0; i < N; i++) {
        if (emitted[i]) continue;
        int cur = i;
        emitted[cur] = 1;
        order.push_back(cur);
        for (;;) {
            int next = -1;
            for (int k = cur + 1; k < N && next < 0; k++)
                if (!emitted[k] && reads(ns[k], ns[cur].out) && ready(k)) next = k;
            if (next < 0) break;
            emitted[next] = 1;
            order.push_back(next);
            cur = next;
        }
    }
    std::vector<Node> out;
    out.reserve(ns.size());
    for (int k : order) out.push_back(std::move(ns[k]));
    ns = std::move(out);
}

// dep[b][a]: node b needs node a's result, directly or through other nodes (plan order = a topological order)
std::vector<std::vector<char>> dependence(const std::vector<Node>& ns) {
    const size_t N = ns.size();
    if (N > 2048) return {};   // (an N x N table: graphs of that size — none of the reference's has 200 operators — do without the fork analysis)
    std::map<int, int> producer;
    for (size_t i = 0; i < N; i++) {
        producer[ns[i].out] = static_cast<int>(i);
        for (int t : ns[i].extra_out) producer[t] = static_cast<int>(i);
    }
    std::vector<std::vector<char>> dep(N, std::vector<char>(N, 0));
    for (size_t b = 0; b < N; b++) {
        std::vector<int> srcs = ns[b].in;
        if (ns[b].res >= 0) srcs.push_back(ns[b].res);
        for (int t : srcs) {
            auto it = producer.find(t);
            if (it == producer.end() || it->second >= static_cast<int>(b)) continue;
            const size_t a = static_cast<size_t>(it->second);
            dep[b][a] = 1;
            for (size_t k = 0; k < N; k++) dep[b][k] |= dep[a][k];
        }
    }
    return dep;
}

// A fork: node j's output is read by two nodes neither of which needs the other — the start of independent branches (the two heads of
// the iris / face mesh networks).  A stage program that ran on past the fork would chain one branch behind the common part and leave
// the other waiting for the whole launch; ending the launch at the fork lets the engine run the branches side by side.
bool is_fork(const std::vector<Node>& ns, const std::vector<std::vector<char>>& dep, size_t j) {
    if (dep.size() != ns.size()) return false;
    std::vector<int> rd = Readers{ns}.readers(ns[j].out);
    for (int t : ns[j].extra_out)   // a launch with several outputs: their readers part just the same
        for (int k : Readers{ns}.readers(t))
            if (std::find(rd.begin(), rd.end(), k) == rd.end()) rd.push_back(k);
    for (size_t x = 0; x < rd.size(); x++)
        for (size_t y = x + 1; y < rd.size(); y++)
            if (!dep[static_cast<size_t>(rd[y])][static_cast<size_t>(rd[x])] && !dep[static_cast<size_t>(rd[x])][static_cast<size_t>(rd[y])]) return true;
    return false;
}

std::vector<Node> group_resident(const Graph& g, const std::vector<Node>& ns, int budget, bool tail) {
    std::vector<Node> outv;
    static const bool no_bneck = getenv("MI_NO_BNECK") != nullptr;  // development aid
    static const bool no_dblock = getenv("MI_NO_DBLOCK") != nullptr;  // development aid
    static const bool no_fork_split = getenv("MI_NO_FORK_SPLIT") != nullptr;  // development aid
    const bool no_tail = !tail || getenv("MI_NO_TAIL") != nullptr;     // option "tail" 0 / development aid: the round-4 plan (resident_kernel / chain_kernel for every small-spatial part)
    static const bool tail_split = getenv("MI_TAIL_SPLIT") != nullptr;  // development aid
    const std::vector<std::vector<char>> dep = dependence(ns);
    for (size_t i = 0; i < ns.size();) {
        {
            Node xn;
            const size_t used = build_xc(g, ns, i, &xn);
            if (used) {
                outv.push_back(std::move(xn));
                i += used;
                continue;
            }
        }
        {
            Node db;
            const size_t used = no_dblock ? 0 : build_dblock(g, ns, i, &db);
            if (used) {
                outv.push_back(std::move(db));
                i += used;
                continue;
            }
        }
        {
            Node bn;
            const size_t used = no_bneck ? 0 : build_bneck(g, ns, i, &bn);
            if (used) {
                outv.push_back(std::move(bn));
                i += used;
                continue;
            }
        }
        Node best;
        size_t best_j = 0;
        bool have = false;
        // the longest run from i in either form; the several-frames-per-workgroup form (tail_kernels.hip) wins when it reaches at
        // least as far (it also takes frame-resident chains with stride-2 neighbours, which the classic form leaves alone)
        for (int form = no_tail ? 1 : 0; form < 2; form++) {
            Node fbest;
            size_t fj = 0;
            bool fhave = false;
            for (size_t j = i; j < ns.size(); j++) {
                Node cand;
                {   // a stage program does not run on into an expand / contract run: that one has its own launch (xc_kernels.hip)
                    Node xn;
                    if (j > i && build_xc(g, ns, j, &xn)) break;
                }
                if (!(form == 0 ? build_tail(g, ns, i, j, &cand) : build_resident(g, ns, i, j, budget, &cand))) break;  // a longer run only needs more
                fbest = std::move(cand);
                fj = j;
                fhave = true;
                if (!no_fork_split && j > i && is_fork(ns, dep, j)) break;  // the launch ends where the branches part (a fork at the very start is the previous launch's business)
                if (form == 0 && tail_split && j + 1 < ns.size() && ns[j].kind == Node::Chain && ns[j].chain_post) break;  // development aid: a launch per resolution
            }
            if (fhave && (!have || fj > best_j)) { best = std::move(fbest); best_j = fj; have = true; }
        }
        // worth a launch of its own: at least two fused nodes, or a k x k convolution (otherwise the generic direct conv)
        bool take = have && (best.members.size() >= 2 || (best.members[0].kind == Node::Conv && best.members[0].KH > 1));
        Node banded;
        if (take) {
            outv.push_back(std::move(best));
            i = best_j + 1;
        } else if (build_banded_bottleneck(g, ns, i, &banded)) {
            outv.push_back(std::move(banded));
            i += 2;
        } else {
            outv.push_back(ns[i]);
            i++;
        }
    }
    return outv;
}

}  // namespace plan_detail
}  // namespace mi
