// consts.cpp — see consts.hpp.  One function per launch form; a constant tensor is only ever read through Packer::data, which
// refuses a tensor shorter than the layer that names it (the bytes of a model are untrusted).
#include "consts.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace mi {

float act_slope(const Graph& g, const Node& m, int c) {
    if (m.act != ACT_PRELU) return m.act == ACT_NONE ? 1.f : 0.f;
    return g.tensors.at(static_cast<size_t>(m.alpha)).f32.at(static_cast<size_t>(c));
}

const std::vector<float>& const_data(const Graph& g, int t, long need) {
    if (t < 0 || static_cast<size_t>(t) >= g.tensors.size()) throw std::runtime_error("consts: a layer names a constant tensor that does not exist");
    const std::vector<float>& v = g.tensors[static_cast<size_t>(t)].f32;
    if (need < 0 || v.size() < static_cast<size_t>(need)) throw std::runtime_error("consts: a constant tensor is shorter than the layer that reads it");
    return v;
}

uint16_t bf16_rne(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return static_cast<uint16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

float bf16_to_float(uint16_t h) {
    const uint32_t u = static_cast<uint32_t>(h) << 16;
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}

namespace {
// rows [O][I] -> MFMA A-fragment order [tile][k-chunk][lane][4] of a zero padded [Cop][Cp] matrix: lane l = (row m = l & 31,
// k-half h = l >> 5) holds W[tile*32 + m][h*Cp/2 + 4*chunk + e].  kblk == 16: the K-blocked order of the LDS-staged pointwise stages
std::vector<float> a_frag32(const float* src, int O, int I, int Cop, int Cp, int kblk = 0) {
    const int Ch = Cp / 2, MT = Cop / 32;
    std::vector<float> r(static_cast<size_t>(Cop) * Cp, 0.f);
    for (size_t k = 0; k < static_cast<size_t>(MT) * (Ch / 4) * 256; k++) {  // element k = (((tile, chunk j), lane l), e)
        const int e = k & 3, l = k >> 2 & 63, j = k / 256 % (Ch / 4), o = static_cast<int>(k / 256 / (Ch / 4)) * 32 + (l & 31);
        const int c = kblk == 16 ? 16 * (j / 2) + 8 * (l >> 5) + 4 * (j % 2) + e : (l >> 5) * Ch + 4 * j + e;
        if (o < O && c < I) r[k] = src[static_cast<size_t>(o) * I + c];
    }
    return r;
}

// rows [O][Kv] -> the A operands of v_mfma_f32_16x16x4_f32 (tail_kernels.hip): lane (k-quarter kq = l / 16, row m = l % 16) holds, for
// float4 step q, W[16 tile + m][kq * Kv / 4 + 4 q .. + 3]
std::vector<float> a_frag16(const float* src, int O, int Kv) {
    const int nct = (O + 15) / 16, n4 = Kv / 16, K4 = Kv / 4;
    std::vector<float> r(static_cast<size_t>(nct) * n4 * 256, 0.f);
    for (size_t k = 0; k < r.size(); k++) {  // element k = (((tile, step q), lane l), e)
        const int e = k & 3, l = k >> 2 & 63, q = k / 256 % n4, o = static_cast<int>(k / 256 / n4) * 16 + (l & 15);
        if (o < O) r[k] = src[static_cast<size_t>(o) * Kv + (l >> 4) * K4 + 4 * q + e];
    }
    return r;
}

int weight_of(const Node& m) { return m.kind == Node::Conv ? m.w : m.w2; }
int bias_of(const Node& m) { return m.kind == Node::Conv ? m.b : m.b2; }
struct BlockPtrs { const float *w, *b, *w2, *b2, *alpha; int act; };  // what the kernels' *_pack_consts functions take of one block

struct Packer {
    const Plan& plan;
    const Graph& g;
    PlanConsts& pc;
    long put(const std::vector<float>& v) {  // every piece starts on a 64-float boundary
        const size_t off = (pc.blob.size() + 63) / 64 * 64;
        pc.blob.resize(off + v.size(), 0.f);
        std::copy(v.begin(), v.end(), pc.blob.begin() + static_cast<long>(off));
        return static_cast<long>(off);
    }
    const std::vector<int>& shape(int t) const { return g.tensors.at(static_cast<size_t>(t)).shape; }
    int dim(int t, size_t d) const { return shape(t).at(d); }
    const std::vector<float>& data(int t, long need = 0) const { return const_data(g, t, need); }
    const float* ptr(int t, long need) const { return t >= 0 ? data(t, need).data() : nullptr; }
    long put_tensor(int t) { return put(data(t)); }
    // `rows` rows of n floats of tensor t (when it exists) to dst + off, `stride` apart
    void copy(std::vector<float>& dst, size_t off, int t, int n, int rows = 1, int stride = 0) const {
        if (t < 0) return;
        const std::vector<float>& v = data(t, static_cast<long>(rows) * n);
        for (int r = 0; r < rows; r++) std::copy_n(v.begin() + static_cast<long>(r) * n, n, dst.begin() + static_cast<long>(off) + static_cast<long>(r) * stride);
    }
    void slopes(std::vector<float>& dst, size_t off, const Node& m, int n) const { for (int c = 0; c < n; c++) dst[off + static_cast<size_t>(c)] = act_slope(g, m, c); }
    // a block C -> Co: 3x3 depthwise taps and bias (when it has them), pointwise matrix and bias, PReLU slopes
    BlockPtrs block_ptrs(const Node& m, int C, int Co) const {
        return {ptr(m.w, 9L * C), ptr(m.b, C), ptr(m.w2, static_cast<long>(Co) * C), ptr(m.b2, Co), m.act == ACT_PRELU ? data(m.alpha, Co).data() : nullptr, m.act};
    }
    // the constants of one block in a kernel's own layout: fn(dims..., block, dst) fills `floats` floats
    template <class F, class... D>
    long pack_block(F fn, int floats, const BlockPtrs& p, D... dims) {
        std::vector<float> sc(static_cast<size_t>(floats));
        fn(dims..., p.w, p.b, p.w2, p.b2, p.alpha, p.act, sc.data());
        return put(sc);
    }
    long pack_mdblock(int W, int C, int Cm, int Co, const Node& pa, const Node& pb, bool pair) {
        std::vector<float> mc(static_cast<size_t>(mdblock_consts_floats(W, C, Cm, Co, pair)));
        const BlockPtrs a = block_ptrs(pa, C, Cm), b = block_ptrs(pb, Cm, Co);
        mdblock_pack_consts(W, C, Cm, Co, a.w, a.b, a.w2, a.b2, a.alpha, a.act, b.w, b.b, b.w2, b.b2, b.alpha, b.act, mc.data(), pair);
        return put(mc);
    }
    // pointwise weights [O][1][1][I] in the block kernel's A-fragment order.  [O][KH][KW][I] is read as [O][KH*KW*I]: the k x k stride-k
    // convolutions of the stage programs contract over the "virtual channels" (tap, channel) in exactly this order
    long pack_pw(int wt, int kblk = 0) {
        const std::vector<int>& ws = shape(wt);
        int O = ws.at(0), I = ws.at(1) * ws.at(2) * ws.at(3), Cp, Cop;
        block_weight_dims(I, O, &Cp, &Cop);
        return put(a_frag32(data(wt, static_cast<long>(O) * I).data(), O, I, Cop, Cp, kblk));
    }
    void chain_members(size_t i, const Node& n) {
        for (const Node& m : n.members) {
            MemberOff mo;
            mo.w = put_tensor(m.w);
            if (m.b >= 0) mo.b = put_tensor(m.b);
            mo.w2 = pack_pw(m.w2);
            if (m.b2 >= 0) mo.b2 = put_tensor(m.b2);
            if (m.alpha >= 0) mo.alpha = put_tensor(m.alpha);
            const int C = dim(m.w2, 3), Co = dim(m.w2, 0);  // [O][1][1][I]
            const bool piped = !n.chain_pre && !n.chain_post;  // (a frame-resident chain with stride-2 edge stages: block-kernel packing only)
            if (piped && m.sh == 2) mo.strip = pack_block(strip_pack_consts_s2, strip_consts_s2_floats(C, Co), block_ptrs(m, C, Co), C, Co);  // stride-2 tail
            else if (piped && strip_shape_ok(C, Co)) mo.strip = pack_block(strip_pack_consts, strip_consts_floats(C), block_ptrs(m, C, Co), C);
            pc.chain_off[i].push_back(mo);
        }
    }
    // a BlazeBlock that keeps the resolution and adds its own input
    static bool plain(const Node& m) {
        return m.w >= 0 && !m.in.empty() && m.sh == 1 && m.sw == 1 && m.res == m.in[0] && m.res_mode == RES_DIRECT && !m.res_after && m.padding == Padding::Same;
    }
    // tensor t is read by node `reader` alone and is no graph output
    bool only_reader(size_t reader, int t) const {
        bool only = true;
        for (size_t j = 0; j < plan.nodes.size(); j++) {
            if (j == reader) continue;
            for (int x : plan.nodes[j].in) only = only && x != t;
            only = only && plan.nodes[j].res != t;
        }
        for (int o : g.outputs) only = only && plan.storage[o].root != plan.storage[t].root;
        return only;
    }
    // a row-pipelined pair of plain BlazeBlocks on a wide layer also gets the constants of the operand-layout kernel
    // (mdblock_kernels.hip, pair form; which of the two runs is decided per launch)
    void chain_pair(size_t i, const Node& n) {
        if (n.members.size() != 2 || n.chain_pre || n.chain_post || !n.head_pairs.empty()) return;
        const Node &pa = n.members[0], &pb = n.members[1];
        if (!plain(pa) || !plain(pb) || pb.in[0] != pa.out) return;
        const std::vector<int>& sx = shape(pa.in[0]);
        if (sx.size() != 4) return;
        const int C = sx[3], Cm = dim(pa.out, 3), Co = dim(pb.out, 3);
        if (mdblock_shape_ok(sx[2], C, Cm, Co, true)) pc.node_chain_pair[i] = pack_mdblock(sx[2], C, Cm, Co, pa, pb, true);
    }
    // output heads of a chain's launch: the weights of a pair stacked [Co_a + Co_b][C] in A-fragment order, the biases stacked
    void head_pairs(size_t i, const Node& n) {
        for (const Node::HeadPair& hp : n.head_pairs) {
            const Node* hn[2] = {&n.head_nodes.at(static_cast<size_t>(hp.a)), hp.b >= 0 ? &n.head_nodes.at(static_cast<size_t>(hp.b)) : nullptr};
            const int I = dim(weight_of(*hn[0]), 3);
            if (I <= 0) throw std::runtime_error("engine: output head without input channels");
            std::vector<float> rows, bias;
            for (const Node* m : hn) {
                if (!m) continue;
                const std::vector<int>& ws = shape(weight_of(*m));
                if (ws.at(3) != I || ws[1] != 1 || ws[2] != 1) throw std::runtime_error("engine: output heads of a pair differ in their input width");
                const std::vector<float>& w = data(weight_of(*m), static_cast<long>(ws[0]) * I);
                rows.insert(rows.end(), w.begin(), w.end());
                if (bias_of(*m) >= 0) bias.insert(bias.end(), data(bias_of(*m)).begin(), data(bias_of(*m)).end());
                else bias.insert(bias.end(), static_cast<size_t>(ws[0]), 0.f);
            }
            const int O = static_cast<int>(rows.size()) / I, MT = (O + 31) / 32;
            bias.resize(static_cast<size_t>(MT) * 32, 0.f);
            MemberOff mo;
            mo.w2 = put(a_frag32(rows.data(), O, I, MT * 32, I));
            mo.b2 = put(bias);
            pc.chain_head_off[i].push_back(mo);
        }
    }
    // expand / contract runs (xc_kernels.hip): per member the pointwise matrix in the block kernel's packing and the stage's small
    // constants as the kernel copies them to LDS: taps [9][Cp], depthwise bias [Cp], pointwise bias [Cop]
    void xc(size_t i, const Node& n) {
        for (const Node& m : n.members) {
            MemberOff mo;
            mo.w2 = pack_pw(m.w2);
            const int C = dim(m.in.at(0), 3), Co = dim(m.out, 3), Cp = (C + 7) & ~7;
            std::vector<float> cb(static_cast<size_t>(xc_const_floats(C, Co)), 0.f);
            copy(cb, 0, m.w, C, 9, Cp);
            copy(cb, static_cast<size_t>(9) * Cp, m.b, C);
            copy(cb, static_cast<size_t>(10) * Cp, m.b2, Co);
            mo.cblob = put(cb);
            pc.chain_off[i].push_back(mo);
        }
    }
    // double block (dblock_kernels.hip): both pointwise matrices in the block kernel's packing and one blob of small constants
    // (DblockArgs::consts); the wide layers also get the constants of the operand-layout kernel (mdblock_kernels.hip; which of the two
    // runs is decided per launch)
    void dblock(size_t i, const Node& n) {
        const Node &pa = n.members.at(0), &pb = n.members.at(1);
        const int C = dim(pa.in.at(0), 3), Cm = dim(pa.out, 3), Co = dim(pb.out, 3), Cmp = (Cm + 7) & ~7, MT = (Co + 31) / 32, MTA = (Cm + 31) / 32;
        MemberOff ma, mb;
        ma.w2 = pack_pw(pa.w2);
        mb.w2 = pack_pw(pb.w2);
        std::vector<float> cb(static_cast<size_t>(dblock_const_floats(C, Cm, Co)), 0.f);
        size_t o = 0;
        auto at = [&](int floats) { o += static_cast<size_t>(floats); return o - static_cast<size_t>(floats); };  // the next piece, `floats` long
        copy(cb, at(9 * C), pa.w, 9 * C);
        copy(cb, at(C), pa.b, C);
        copy(cb, at(32 * MTA), pa.b2, Cm);
        slopes(cb, at(32 * MTA), pa, Cm);
        copy(cb, at(9 * Cmp), pb.w, Cm, 9, Cmp);
        copy(cb, at(Cmp), pb.b, Cm);
        copy(cb, at(32 * MT), pb.b2, Co);
        slopes(cb, at(32 * MT), pb, Co);
        ma.cblob = put(cb);
        const int Wd = dim(pa.in[0], 2);
        if (mdblock_shape_ok(Wd, C, Cm, Co) && pa.res < 0 && pb.res == pa.in[0]) mb.mconsts = pack_mdblock(Wd, C, Cm, Co, pa, pb, false);
        pc.chain_off[i] = {ma, mb};
    }
    // first pointwise matrix [Cm][C] of a bottleneck pair: its contraction index in the MFMA result order
    static std::vector<float> bneck_first_matrix(const float* w1, int Cm, int C) {
        std::vector<float> r(static_cast<size_t>(Cm) * C, 0.f);
        const int NCH1 = C / 8;
        for (size_t k = 0; k < static_cast<size_t>(Cm / 32) * NCH1 * 256; k++) {  // element k = (((tile t, chunk j), lane l), e)
            const int e = k & 3, l = k >> 2 & 63, j = k / 256 % NCH1, t = static_cast<int>(k / 256 / NCH1);
            r[k] = w1[static_cast<size_t>(32 * t + (l & 31)) * C + 32 * (j / 4) + 8 * (j % 4) + 4 * (l >> 5) + e];
        }
        return r;
    }
    // bottleneck pairs (bneck_kernels.hip): per pair the first pointwise matrix in its own order, the second in the block kernel's, and
    // one blob of small constants; 32-pixel-wide pairs also get the constants of the operand-layout kernel (mdblock_kernels.hip, mbneck_kernel)
    void bneck(size_t i, const Node& n) {
        for (size_t k = 0; k + 1 < n.members.size(); k += 2) {
            const Node &pa = n.members[k], &pb = n.members[k + 1];
            const int Cm = dim(pa.w2, 0), C = dim(pa.w2, 3);  // [Cm][1][1][C]
            MemberOff ma, mb;
            ma.w2 = put(bneck_first_matrix(data(pa.w2, static_cast<long>(Cm) * C).data(), Cm, C));
            mb.w2 = pack_pw(pb.w2);
            std::vector<float> cb(static_cast<size_t>(bneck_const_floats(C, Cm)), 0.f);
            copy(cb, 0, pa.b2, Cm);
            slopes(cb, static_cast<size_t>(Cm), pa, Cm);
            copy(cb, static_cast<size_t>(2) * Cm, pb.w, 9 * Cm);
            copy(cb, static_cast<size_t>(11) * Cm, pb.b, Cm);
            copy(cb, static_cast<size_t>(12) * Cm, pb.b2, C);
            slopes(cb, static_cast<size_t>(12) * Cm + C, pb, C);
            ma.cblob = put(cb);
            const int Wd = dim(pa.in.at(0), 2);
            if (mbneck_shape_ok(Wd, C, Cm)) {
                std::vector<float> mc(static_cast<size_t>(mbneck_consts_floats(Wd, C, Cm)));
                const BlockPtrs a = block_ptrs(pa, C, Cm), b = block_ptrs(pb, Cm, C);
                mbneck_pack_consts(Wd, C, Cm, a.w2, a.b2, a.alpha, a.act, b.w, b.b, b.w2, b.b2, b.alpha, b.act, mc.data());
                mb.mconsts = put(mc);
            }
            pc.chain_off[i].insert(pc.chain_off[i].end(), {ma, mb});
        }
    }
    // tail_kernels.hip: per stage the A operands and the small constants: [bias][slope] padded to whole tiles, then for depthwise
    // stages the taps [9][Kv] and the depthwise bias [Kv]
    void tail_stages(size_t i, const Node& n) {
        pc.tail_wa[i].assign(n.stages.size(), -1);
        pc.tail_wc[i].assign(n.stages.size(), -1);
        for (size_t k = 0; k < n.stages.size(); k++) {
            TailStage st = n.stages[k].tst;
            resolve(st, n.stages[k]);
            pc.tail_progs.push_back(st);
            if (st.kind == TAIL_LOAD) continue;
            const Node& m = n.members.at(static_cast<size_t>(n.stages[k].member));
            const int O = st.Co, Kv = st.Kv, nct = (O + 15) / 16;
            const std::vector<float>& wsrc = data(weight_of(m));
            if (wsrc.size() != static_cast<size_t>(O) * Kv) throw std::runtime_error("engine: tail stage weights do not match its shape");
            pc.tail_progs.back().w_a = pc.tail_wa[i][k] = put(a_frag16(wsrc.data(), O, Kv));
            std::vector<float> cb(static_cast<size_t>(32 * nct) + (st.kind == TAIL_DW ? static_cast<size_t>(10) * Kv : 0), 0.f);
            copy(cb, 0, bias_of(m), O);
            slopes(cb, static_cast<size_t>(16 * nct), m, O);
            if (st.kind == TAIL_DW) {
                copy(cb, static_cast<size_t>(32 * nct), m.w, 9 * Kv);  // [3][3][C]
                copy(cb, static_cast<size_t>(32 * nct + 9 * Kv), m.b, Kv);
            }
            pc.tail_progs.back().w_c = pc.tail_wc[i][k] = put(cb);
        }
    }
    // resident_kernels.hip: per member the pointwise / k x k stride-k weights in A-fragment order (the k x k ones over the virtual channels),
    // per stage the K-blocked copy where the stage wants one and the small constants, padded the way the kernel copies them to LDS
    void resident_stages(size_t i, const Node& n) {
        for (const Node& m : n.members) {
            MemberOff mo;
            mo.w2 = pack_pw(weight_of(m));
            pc.chain_off[i].push_back(mo);
        }
        pc.res_wblk[i].assign(n.stages.size(), -1);
        for (size_t k = 0; k < n.stages.size(); k++)
            if (n.stages[k].st.kblk) pc.res_wblk[i][k] = pack_pw(weight_of(n.members.at(static_cast<size_t>(n.stages[k].member))), n.stages[k].st.kblk);
        pc.res_cblob[i].assign(n.stages.size(), -1);
        for (size_t k = 0; k < n.stages.size(); k++) {
            ResStage st = n.stages[k].st;
            resolve(st, n.stages[k]);
            pc.progs.push_back(st);
            if (st.kind == RES_STAGE_LOAD) continue;
            const Node& m = n.members.at(static_cast<size_t>(n.stages[k].member));
            const int Cp = (st.Kv + 7) & ~7, Cop = (st.Co + 31) / 32 * 32;
            std::vector<float> cb(static_cast<size_t>(resident_const_floats(st)), 0.f);
            size_t o = 0;
            if (st.kind == RES_STAGE_DW) {
                copy(cb, 0, m.w, st.Kv, 9, Cp);  // [3][3][C]
                copy(cb, static_cast<size_t>(9) * Cp, m.b, st.Kv);
                o = static_cast<size_t>(10) * Cp;
            }
            copy(cb, o, bias_of(m), st.Co);
            slopes(cb, o + static_cast<size_t>(Cop), m, st.Co);
            pc.progs.back().cblob = pc.res_cblob[i][k] = put(cb);
            pc.progs.back().w_pw = st.kblk ? pc.res_wblk[i][k] : pc.chain_off[i].at(static_cast<size_t>(n.stages[k].member)).w2;
        }
    }
    // the face mesh's first convolution can run inside the launch of the block pair behind it (mdblock_kernels.hip, MD::STEM): the graph's
    // side of the conditions
    bool stem_fuses(size_t i, const Node& n) const {
        const std::vector<int>&sxi = shape(n.in.at(0)), &sxo = shape(n.out);
        if (sxi.size() != 4 || sxo.size() != 4 || n.padding != Padding::Same || n.ept >= 0 || n.res >= 0 || n.in[0] != g.inputs.at(0)) return false;
        if (n.act != ACT_NONE && n.act != ACT_RELU && n.act != ACT_RELU6 && n.act != ACT_PRELU) return false;
        if (!mdblock_stem_shape_ok(sxi[1], sxi[2], sxi[3], n.KH, n.KW, n.sh, n.sw, sxo[1], sxo[2], sxo[3]) || (n.act == ACT_PRELU && n.alpha < 0)) return false;
        // its output is read once, by the pair behind it (which is the next node), and is no graph output
        if (i + 1 >= plan.nodes.size() || !only_reader(i + 1, n.out)) return false;
        const Node& next = plan.nodes[i + 1];
        return next.kind == Node::Chain && next.members.size() == 2 && next.in.size() >= 1 && next.in[0] == n.out &&
               std::count(next.in.begin(), next.in.end(), n.out) + (next.res == n.out) == 1;
    }
    // generic convolution: [O][KH][KW][I] -> [KH][KW][I][Cop], output channels innermost and padded to a multiple of 4
    void conv(size_t i, const Node& n) {
        const std::vector<int>& ws = shape(n.w);
        const int O = ws.at(0), KH = ws.at(1), KW = ws.at(2), I = ws.at(3), Cop = (O + 3) & ~3;
        const std::vector<float>& src = data(n.w, static_cast<long>(O) * KH * KW * I);
        std::vector<float> r(static_cast<size_t>(KH) * KW * I * Cop, 0.f);
        const size_t per_o = static_cast<size_t>(KH) * KW * I;  // (ky, kx, c) keeps its order, o moves inside
        for (size_t k = 0; k < per_o * O; k++) r[k % per_o * Cop + k / per_o] = src[k];
        pc.node_w[i] = put(r);
        // the dense convolutions conv_mfma_kernel takes read the filter as it is stored, [O][KH*KW*I] (which of the two kernels runs is decided per launch)
        // (but the k x k stride-k ones, the iris network's 2x2 stride-2 steps: those are the stage programs' gather form, and generic where they run alone)
        const std::vector<int>&sin = shape(n.in.at(0)), &sout = shape(n.out);
        const bool whole_frame = sin.size() == 4 && sout.size() == 4 && sin[1] == KH && sin[2] == KW && sout[1] == 1 && sout[2] == 1;   // (a head: the batch GEMM's or the generic kernel's)
        if (conv_mfma_shape_ok(I, KH, KW, O) && !whole_frame && !(n.sh == KH && n.sw == KW) && (n.res < 0 || n.res_mode == RES_DIRECT)) pc.node_wrows[i] = put(std::vector<float>(src.begin(), src.begin() + static_cast<long>(per_o) * O));
        if (!stem_fuses(i, n)) return;
        std::vector<float> sc(static_cast<size_t>(mdblock_stem_consts_floats()));
        mdblock_pack_stem(src.data(), ptr(n.b, O), n.act == ACT_PRELU ? data(n.alpha, O).data() : nullptr, n.act, sc.data());
        pc.node_stem[i] = put(sc);
    }
    // conv_bf16_kernel's B operand of a convolution that has node_wrows: the filter rows rounded to bf16 (`hi`), and with `split` what the
    // rounding dropped, rounded again (`lo` = bf16(w - hi)); two values a float slot
    void conv_bf16_planes(size_t i, const Node& n, bool split) {
        const std::vector<int>& ws = shape(n.w);
        const size_t count = static_cast<size_t>(ws.at(0)) * ws.at(1) * ws.at(2) * ws.at(3);   // (even: C % 32 == 0)
        const std::vector<float>& src = data(n.w, static_cast<long>(count));
        std::vector<uint16_t> hi(count), lo(count);
        for (size_t k = 0; k < count; k++) {
            hi[k] = bf16_rne(src[k]);
            lo[k] = bf16_rne(src[k] - bf16_to_float(hi[k]));
        }
        auto plane = [&](const std::vector<uint16_t>& h) {
            std::vector<float> v(count / 2);
            std::memcpy(v.data(), h.data(), v.size() * sizeof(float));
            return put(v);
        };
        pc.node_wbf16_hi[i] = plane(hi);
        if (split) pc.node_wbf16_lo[i] = plane(lo);
    }
    // BlazeBlock with a launch of its own: the block kernel's constants, and those of every specialised form its shape has
    void block(size_t i, const Node& n) {
        if (n.w >= 0) pc.node_w[i] = put_tensor(n.w);
        pc.node_w2[i] = pack_pw(n.w2);
        const int C = dim(n.w2, 3), Co = dim(n.w2, 0);  // [O][1][1][I]
        if (n.w < 0 || n.padding != Padding::Same) return;
        const std::vector<int>&sin = shape(n.in.at(0)), &sout = shape(n.out);
        if (n.sh == 1 && n.sw == 1) {
            auto p = [&] { return block_ptrs(n, C, Co); };  // (length-checked: only for a form that reads them)
            if (strip_shape_ok(C, Co)) pc.node_strip[i] = pack_block(strip_pack_consts, strip_consts_floats(C), p(), C);
            else if (mstrip_shape_ok(C, Co) && sout.at(2) == 32) pc.node_strip[i] = pack_block(mstrip_pack_consts, mstrip_consts_floats(C), p(), C);
            const int Wn = sout.size() == 4 ? sout[2] : 0;
            if (mwalk_shape_ok(Wn, C, Co)) pc.node_mwalk[i] = pack_block(mwalk_pack_consts, mwalk_consts_floats(Wn, C, Co), p(), Wn, C, Co);
        }
        // stride-2 blocks with an operand-layout form (ms2_kernels.hip)
        const bool pool_skip = n.res >= 0 && n.res == n.in[0] && n.res_mode == RES_MAXPOOL && !n.res_after;
        if (n.sh == 2 && n.sw == 2 && n.ept < 0 && sin.size() == 4 && (n.res < 0 || pool_skip) && ms2_shape_ok(sin[2], C, Co, pool_skip))
            pc.node_mwalk[i] = pack_block(ms2_pack_consts, ms2_consts_floats(sin[2], C, Co, pool_skip), block_ptrs(n, C, Co), sin[2], C, Co, pool_skip);
    }
    // two plain BlazeBlocks in a row on a layer mdblock_kernels.hip has a pair form for (the face mesh's 48x48x32 blocks): the constants of
    // the pair launch, kept at the first node; which form runs is decided per launch
    void plain_pairs() {
        auto alone = [&](const Node& m) { return m.kind == Node::Block && plain(m) && m.in.size() == 1 && m.ept < 0 && (m.act != ACT_PRELU || m.alpha >= 0); };
        for (size_t i = 0; i + 1 < plan.nodes.size(); i++) {
            const Node &pa = plan.nodes[i], &pb = plan.nodes[i + 1];
            if (!alone(pa) || !alone(pb) || pb.in[0] != pa.out) continue;
            const std::vector<int>& sx = shape(pa.in[0]);
            if (sx.size() != 4 || shape(pa.out) != sx || shape(pb.out) != sx || !mdblock_shape_ok(sx[2], sx[3], sx[3], sx[3], true)) continue;
            // the tensor between the two is never written by that launch: nobody else may read it
            if (only_reader(i + 1, pa.out)) pc.node_pair[i] = pack_mdblock(sx[2], sx[3], sx[3], sx[3], pa, pb, true);
        }
    }
    // a tensor as a stage program names it: (base index, offsets), resolved against ResBases at launch
    ResRef ref(int t) const {
        ResRef r;
        const Storage& st = plan.storage.at(static_cast<size_t>(t));
        r.inner = st.offset;
        r.fs = st.frame_stride;
        if (st.root == plan.storage[g.inputs[0]].root) { r.base = 1; return r; }
        for (size_t k = 0; k < g.outputs.size(); k++)
            if (plan.storage[g.outputs[k]].root == st.root) {
                if (2 + k >= static_cast<size_t>(kResBases)) throw std::runtime_error("stage program: too many graph outputs");
                r.base = 2 + static_cast<int>(k);
                return r;
            }
        if (plan.root_offset[st.root] < 0) throw std::runtime_error("stage program: tensor has no storage");
        r.base = 0;
        r.root_off = plan.root_offset[st.root];
        return r;
    }
    // the global references of a stage program's stage (kind 0 is the LOAD stage of both forms: it has a source only)
    template <class S>
    void resolve(S& st, const Node::Stage& sg) const {
        if (sg.src_t >= 0) st.src_g = ref(sg.src_t);
        if (st.kind != 0 && sg.dst_t >= 0) st.dst_g = ref(sg.dst_t);
        if (st.kind != 0 && sg.res_t >= 0) st.res_g = ref(sg.res_t);
    }
};

}  // namespace

PlanConsts pack_plan_consts(const Plan& plan, int conv_bf16) {
    PlanConsts pc;
    Packer p{plan, plan.graph, pc};
    const size_t NN = plan.nodes.size();
    for (std::vector<long>* v : {&pc.node_w, &pc.node_b, &pc.node_w2, &pc.node_b2, &pc.node_alpha, &pc.node_pair, &pc.node_wrows, &pc.node_wbf16_hi, &pc.node_wbf16_lo, &pc.node_stem, &pc.node_mwalk, &pc.node_chain_pair, &pc.node_strip, &pc.node_prog})
        v->assign(NN, -1);
    for (std::vector<std::vector<MemberOff>>* v : {&pc.chain_off, &pc.chain_head_off}) v->assign(NN, {});
    for (std::vector<std::vector<long>>* v : {&pc.res_wblk, &pc.res_cblob, &pc.tail_wa, &pc.tail_wc}) v->assign(NN, {});
    for (size_t i = 0; i < NN; i++) {
        const Node& n = plan.nodes[i];
        if (n.kind == Node::Chain) {
            p.chain_members(i, n);
            p.chain_pair(i, n);
            p.head_pairs(i, n);
        } else if (n.kind == Node::Resident) {
            pc.node_prog[i] = static_cast<long>(n.tail ? pc.tail_progs.size() : pc.progs.size());  // its first stage (the pair forms have none)
            if (n.xc) p.xc(i, n);
            else if (n.dblock) p.dblock(i, n);
            else if (n.bneck) p.bneck(i, n);
            else if (n.tail) p.tail_stages(i, n);
            else p.resident_stages(i, n);
        } else {
            if (n.b >= 0) pc.node_b[i] = p.put_tensor(n.b);
            if (n.b2 >= 0) pc.node_b2[i] = p.put_tensor(n.b2);
            if (n.alpha >= 0) pc.node_alpha[i] = p.put_tensor(n.alpha);
            if (n.kind == Node::Conv && n.gemm_head) pc.node_w[i] = p.put_tensor(n.w);  // [O][KH*KW*I] as stored: the GEMM's W[N][K]
            else if (n.kind == Node::Conv) p.conv(i, n);
            else if (n.kind == Node::Dw) pc.node_w[i] = p.put_tensor(n.w);
            else if (n.kind == Node::Block) p.block(i, n);
            else if (n.kind == Node::Affine) { pc.node_w[i] = p.put(n.scale); pc.node_b[i] = p.put(n.shift); }
        }
    }
    p.plain_pairs();
    if (conv_bf16 != 0)   // behind everything else: no other offset moves
        for (size_t i = 0; i < NN; i++)
            if (plan.nodes[i].kind == Node::Conv && pc.node_wrows[i] >= 0) p.conv_bf16_planes(i, plan.nodes[i], conv_bf16 == 2);
    pc.blob.resize(pc.blob.size() + 4096, 0.f);  // slack: the stage programs' A-fragment prefetch walks up to 8 KiB past a tile's last chunk
    return pc;
}

}  // namespace mi
