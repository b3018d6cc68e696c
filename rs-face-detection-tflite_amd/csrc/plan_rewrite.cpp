// plan_rewrite.cpp — levels 1 and 2 of the lowering: node-by-node rewrites of the operator list (see plan.hpp).
#include "plan_internal.hpp"

namespace mi {
namespace plan_detail {
namespace {

struct Rewriter {
    Graph& g;
    std::vector<Node>& nodes;

    std::vector<int> consumers(int t) const { return Readers{nodes}.refs(t); }
    int producer(int t) const {
        for (size_t i = 0; i < nodes.size(); i++)
            if (!nodes[i].dead && nodes[i].out == t) return static_cast<int>(i);
        return -1;
    }
    bool is_graph_output(int t) const { return plan_detail::is_graph_output(g, t); }
    const std::vector<int>& shape(int t) const { return g.tensors[t].shape; }

    // Fold ADD / activation that exclusively consume node i's output into node i; the fused node takes the
    // position of the last folded op so that every operand (e.g. the skip tensor) is already available there.
    void fuse_epilogues() {
        for (size_t start = 0; start < nodes.size(); start++) {
            for (size_t i = start;;) {
                Node& n = nodes[i];
                if (n.dead || !(n.kind == Node::Conv || n.kind == Node::Dw)) break;
                if (is_graph_output(n.out)) break;
                std::vector<int> cons = consumers(n.out);
                if (cons.size() != 1) break;
                int ci = cons[0];
                if (ci <= static_cast<int>(i)) break;
                Node& c = nodes[ci];
                Node fused = n;
                if (c.kind == Node::Add && n.res < 0 && n.act == ACT_NONE && c.in.size() == 2) {
                    int other = c.in[0] == n.out ? c.in[1] : c.in[0];
                    if (other == n.out || g.tensors[other].is_const) break;
                    if (shape(other) != shape(n.out)) break;
                    fused.res = other;
                    fused.res_mode = RES_DIRECT;
                    fused.act = c.act;
                } else if (c.kind == Node::Add && n.kind == Node::Conv && n.res < 0 && n.act != ACT_NONE && c.act == ACT_NONE && c.in.size() == 2) {
                    // a convolution with a FUSED activation, then ADD: the skip joins behind the activation
                    int other = c.in[0] == n.out ? c.in[1] : c.in[0];
                    if (other == n.out || g.tensors[other].is_const) break;
                    if (shape(other) != shape(n.out)) break;
                    fused.res = other;
                    fused.res_mode = RES_DIRECT;
                    fused.res_after = true;
                } else if (c.kind == Node::Act && n.act == ACT_NONE) {
                    fused.act = c.act;
                    fused.alpha = c.alpha;
                } else {
                    break;
                }
                fused.out = c.out;
                fused.src_ops.insert(fused.src_ops.end(), c.src_ops.begin(), c.src_ops.end());
                n.dead = true;
                nodes[ci] = fused;
                i = static_cast<size_t>(ci);  // continue folding from the new position
                if (fused.res_after) break;   // nothing folds behind a post-activation skip
            }
        }
        // Skip-path simplification: res <- PAD(channels) <- MAX_POOL 2x2/2 | RESIZE x2, each with a single consumer.
        for (size_t i = 0; i < nodes.size(); i++) {
            Node& n = nodes[i];
            if (n.dead || n.res < 0 || n.res_mode != RES_DIRECT) continue;
            int p = producer(n.res);
            if (p >= 0 && nodes[p].kind == Node::Pad && consumers(n.res).size() == 1 && !is_graph_output(n.res)) {
                const Node& pd = nodes[p];
                const auto& pv = g.tensors[pd.pads].i32;
                const auto& si = shape(pd.in[0]);
                bool channel_only = pv.size() == 8 && pv[0] == 0 && pv[1] == 0 && pv[2] == 0 && pv[3] == 0 && pv[4] == 0 &&
                                    pv[5] == 0 && pv[6] == 0 && si.size() == 4;
                if (channel_only) {
                    n.res = pd.in[0];
                    n.src_ops.insert(n.src_ops.end(), pd.src_ops.begin(), pd.src_ops.end());
                    nodes[p].dead = true;
                    p = producer(n.res);
                }
            }
            if (p >= 0 && consumers(n.res).size() == 1 && !is_graph_output(n.res)) {
                const Node& q = nodes[p];
                const auto& si = shape(q.in.empty() ? n.res : q.in[0]);
                const auto& so = shape(n.res);
                if (q.kind == Node::MaxPool && q.filter_h == 2 && q.filter_w == 2 && q.sh == 2 && q.sw == 2 && q.act == ACT_NONE &&
                    si.size() == 4 && si[1] == 2 * so[1] && si[2] == 2 * so[2]) {
                    n.res = q.in[0];
                    n.res_mode = RES_MAXPOOL;
                    n.src_ops.insert(n.src_ops.end(), q.src_ops.begin(), q.src_ops.end());
                    nodes[p].dead = true;
                } else if (q.kind == Node::Resize && q.half_pixel && !q.align_corners && si.size() == 4 && so[1] == 2 * si[1] &&
                           so[2] == 2 * si[2]) {
                    n.res = q.in[0];
                    n.res_mode = RES_UP2X;
                    n.src_ops.insert(n.src_ops.end(), q.src_ops.begin(), q.src_ops.end());
                    nodes[p].dead = true;
                }
            }
        }
    }

    int new_const(std::vector<int> shape, std::vector<float> data) {
        TensorInfo t;
        t.shape = std::move(shape); t.dtype = 0; t.is_const = true; t.f32 = std::move(data);
        g.tensors.push_back(std::move(t));
        return static_cast<int>(g.tensors.size()) - 1;
    }
    int new_activation(std::vector<int> shape) {
        TensorInfo t;
        t.shape = std::move(shape);
        g.tensors.push_back(std::move(t));
        return static_cast<int>(g.tensors.size()) - 1;
    }

    // Per-channel affines (MUL / ADD by constants: a batch normalisation as the converter leaves it when nothing folds it).
    //  (a) consecutive affines merge: (x s1 + t1) s2 + t2 = x (s1 s2) + (t1 s2 + t2), the constants computed in double and rounded once;
    //  (b) an affine behind a convolution / depthwise convolution / FULLY_CONNECTED that has no activation and no skip, and whose output
    //      nobody else reads, folds into that node: filter row o scaled by s[o], bias b s + t, each product rounded once.  (An affine in
    //      FRONT of a convolution stays: with SAME padding its shift would have to reach the zero border.)
    //  (c) an activation that alone reads a remaining affine runs in its launch.
    void fuse_affines() {
        for (size_t i = 0; i < nodes.size(); i++) {
            Node& a = nodes[i];
            if (a.dead || a.kind != Node::Affine || a.act != ACT_NONE || is_graph_output(a.out)) continue;
            std::vector<int> cons = consumers(a.out);
            if (cons.size() != 1 || cons[0] <= static_cast<int>(i)) continue;
            Node& b = nodes[cons[0]];
            if (b.kind != Node::Affine || b.in[0] != a.out || b.scale.size() != a.scale.size()) continue;
            if (a.divide || b.divide) continue;   // a true division merges with nothing: x * (1 / c) is a different number
            for (size_t c = 0; c < a.scale.size(); c++) {
                const double s = static_cast<double>(a.scale[c]) * b.scale[c], t = static_cast<double>(a.shift[c]) * b.scale[c] + b.shift[c];
                b.scale[c] = static_cast<float>(s);
                b.shift[c] = static_cast<float>(t);
            }
            b.in = a.in;
            b.src_ops.insert(b.src_ops.begin(), a.src_ops.begin(), a.src_ops.end());
            a.dead = true;
        }
        for (size_t i = 0; i < nodes.size(); i++) {
            const Node& a = nodes[i];
            if (a.dead || a.kind != Node::Affine || a.divide) continue;
            const int pi = producer(a.in[0]);
            if (pi < 0 || pi >= static_cast<int>(i)) continue;
            const Node& p = nodes[pi];
            if (!(p.kind == Node::Conv || p.kind == Node::Dw) || p.act != ACT_NONE || p.res >= 0 || is_graph_output(p.out) || consumers(p.out).size() != 1) continue;
            const size_t C = a.scale.size();
            const std::vector<int> wshape = g.tensors[p.w].shape;
            const std::vector<float>& wsrc = g.tensors[p.w].f32;
            if (C == 0 || wshape.empty() || wsrc.empty() || wsrc.size() != g.tensors[p.w].elems() || wsrc.size() % C) continue;
            if (static_cast<size_t>(p.kind == Node::Conv ? wshape.front() : wshape.back()) != C) continue;
            if (p.b >= 0 && g.tensors[p.b].f32.size() != C) continue;
            const size_t per = wsrc.size() / C;
            std::vector<float> w(wsrc.size()), b(C);
            for (size_t k = 0; k < w.size(); k++) w[k] = static_cast<float>(static_cast<double>(wsrc[k]) * a.scale[p.kind == Node::Conv ? k / per : k % C]);
            for (size_t c = 0; c < C; c++) b[c] = static_cast<float>(static_cast<double>(p.b >= 0 ? g.tensors[p.b].f32[c] : 0.f) * a.scale[c] + a.shift[c]);
            Node fused = p;
            fused.w = new_const(wshape, std::move(w));
            fused.b = new_const({static_cast<int>(C)}, std::move(b));
            fused.out = a.out;
            fused.act = a.act;
            fused.src_ops.insert(fused.src_ops.end(), a.src_ops.begin(), a.src_ops.end());
            nodes[pi].dead = true;
            nodes[i] = std::move(fused);
        }
        for (size_t i = 0; i < nodes.size(); i++) {
            const Node& a = nodes[i];
            if (a.dead || a.kind != Node::Affine || a.act != ACT_NONE || is_graph_output(a.out)) continue;
            std::vector<int> cons = consumers(a.out);
            if (cons.size() != 1 || cons[0] <= static_cast<int>(i) || nodes[cons[0]].kind != Node::Act) continue;
            const Node& c = nodes[cons[0]];
            Node fused = a;
            fused.act = c.act;
            fused.alpha = c.alpha;
            fused.out = c.out;
            fused.src_ops.insert(fused.src_ops.end(), c.src_ops.begin(), c.src_ops.end());
            nodes[i].dead = true;
            nodes[cons[0]] = std::move(fused);
        }
    }

    // FULLY_CONNECTED over a flattened [1,H,W,C] tensor with weights [N][H W C] is, byte for byte, the whole-frame VALID convolution KH = H,
    // KW = W to [1,1,1,N]: the node reads the 4-D tensor behind the RESHAPE (which goes when nobody else reads it) and writes a [1,1,1,N] view
    // of its [1,N] output.  A rank-2 input without such a producer is the [1,1,1,K] view of itself: a 1x1 convolution.
    void lower_fully_connected() {
        std::vector<std::pair<size_t, Node>> before, after;
        for (size_t i = 0; i < nodes.size(); i++) {
            if (nodes[i].dead || !nodes[i].fc) continue;
            const int x = nodes[i].in[0];
            const std::vector<int> xs = shape(x);
            const int N = shape(nodes[i].w).at(0), K = shape(nodes[i].w).at(1);
            int H = 1, W = 1, C = K;
            std::vector<int> moved;
            if (xs.size() == 4) {
                H = xs[1]; W = xs[2]; C = xs[3];
            } else {
                const int pi = producer(x);
                const int src = pi >= 0 && nodes[pi].kind == Node::Reshape ? nodes[pi].in[0] : -1;
                if (src >= 0 && !g.tensors[src].is_const && shape(src).size() == 4 && shape(src)[0] == 1 && g.tensors[src].elems() == static_cast<size_t>(K)) {
                    H = shape(src)[1]; W = shape(src)[2]; C = shape(src)[3];
                    nodes[i].in = {src};
                    if (consumers(x).empty() && !is_graph_output(x)) {
                        moved = nodes[pi].src_ops;
                        nodes[pi].dead = true;
                    }
                } else {
                    Node r;
                    r.kind = Node::Reshape; r.in = {x}; r.out = new_activation({1, 1, 1, K}); r.src_ops.clear();
                    nodes[i].in = {r.out};
                    before.emplace_back(i, std::move(r));
                }
            }
            Node& n = nodes[i];
            n.src_ops.insert(n.src_ops.begin(), moved.begin(), moved.end());
            n.KH = H; n.KW = W; n.sh = n.sw = 1; n.padding = Padding::Valid;
            n.w = new_const({N, H, W, C}, std::vector<float>(g.tensors[n.w].f32));
            Node r;
            r.kind = Node::Reshape; r.out = n.out; r.src_ops.clear();
            n.out = new_activation({1, 1, 1, N});
            r.in = {n.out};
            after.emplace_back(i, std::move(r));
        }
        if (after.empty()) return;
        std::vector<Node> re;
        size_t kb = 0, ka = 0;
        for (size_t i = 0; i < nodes.size(); i++) {
            if (kb < before.size() && before[kb].first == i) re.push_back(std::move(before[kb++].second));
            re.push_back(std::move(nodes[i]));
            if (ka < after.size() && after[ka].first == i) re.push_back(std::move(after[ka++].second));
        }
        nodes = std::move(re);
    }

    // Spatial PAD (zeros) in front of VALID convolutions — how the MLIR-converted full_range_sparse graph writes every
    // convolution — folds into its consumers: as SAME when the amounts are TF's SAME amounts for that consumer (3x3 stride 1 with
    // 1/1/1/1), as explicit pads before the first row / column otherwise (the kernels bound-check the far side).
    void fold_spatial_pads() {
        for (size_t i = 0; i < nodes.size(); i++) {
            Node& pd = nodes[i];
            if (pd.dead || pd.kind != Node::Pad || is_graph_output(pd.out)) continue;
            const auto& pv = g.tensors[pd.pads].i32;
            const auto& si = shape(pd.in[0]);
            if (pv.size() != 8 || si.size() != 4 || pv[0] || pv[1] || pv[6] || pv[7]) continue;   // batch / channel pads: not this rule
            const int pt = pv[2], pb = pv[3], pl = pv[4], pr = pv[5];
            if (pt < 0 || pb < 0 || pl < 0 || pr < 0 || pt > 1 || pl > 1) continue;             // the kernels keep a one-pixel border
            std::vector<int> cons = consumers(pd.out);
            if (cons.empty()) continue;
            bool ok = true;
            for (int ci : cons) {
                const Node& c = nodes[ci];
                ok &= (c.kind == Node::Conv || c.kind == Node::Dw) && c.padding == Padding::Valid && c.in.size() == 1 && c.in[0] == pd.out && c.res != pd.out && c.ept < 0;
            }
            if (!ok) continue;
            for (int ci : cons) {
                Node& c = nodes[ci];
                const auto& so = shape(c.out);
                int bt, bl, oh, ow;
                same_pad_of(si[1], c.KH, c.sh, bt, oh);
                same_pad_of(si[2], c.KW, c.sw, bl, ow);
                const int tot_h = std::max(0, (oh - 1) * c.sh + c.KH - si[1]), tot_w = std::max(0, (ow - 1) * c.sw + c.KW - si[2]);
                c.in[0] = pd.in[0];
                if (oh == so[1] && ow == so[2] && bt == pt && bl == pl && tot_h - bt == pb && tot_w - bl == pr) {
                    c.padding = Padding::Same;
                } else {
                    c.ept = pt; c.epl = pl;
                }
                c.src_ops.insert(c.src_ops.begin(), pd.src_ops.begin(), pd.src_ops.end());
            }
            // the PAD op is executed by its consumers; with several consumers the op index is listed once (the first)
            for (size_t k = 1; k < cons.size(); k++) {
                Node& c = nodes[cons[k]];
                c.src_ops.erase(c.src_ops.begin(), c.src_ops.begin() + static_cast<long>(pd.src_ops.size()));
            }
            pd.dead = true;
        }
    }
    static void same_pad_of(int in, int k, int stride, int& before, int& out) {
        out = (in + stride - 1) / stride;
        const int total = std::max(0, (out - 1) * stride + k - in);
        before = total / 2;
    }

    // Would the fused MFMA kernel take this node? (shape-level check with placeholder pointers)
    bool block_supported(const Node& f) const {
        const auto& si = shape(f.in[0]);
        const auto& so = shape(f.out);
        if (si.size() != 4 || so.size() != 4) return false;
        BlockArgs a;
        a.in = fake<const float>(kFakeIn);
        a.out = fake<float>(kFakeOut);
        a.in_fs = static_cast<long>(g.tensors[f.in[0]].elems());
        a.out_fs = static_cast<long>(g.tensors[f.out].elems());
        a.B = 1; a.H = si[1]; a.W = si[2]; a.C = si[3]; a.Ho = so[1]; a.Wo = so[2]; a.Co = so[3];
        a.sh = f.sh; a.sw = f.sw;
        a.has_dw = f.w >= 0;
        if (a.has_dw && f.padding == Padding::Same) {
            a.pt = std::max(0, (a.Ho - 1) * a.sh + 3 - a.H) / 2;
            a.pl = std::max(0, (a.Wo - 1) * a.sw + 3 - a.W) / 2;
        }
        if (a.has_dw && f.ept >= 0) { a.pt = f.ept; a.pl = f.epl; }
        if (f.res >= 0) {
            a.ep.res = f.res == f.in[0] ? a.in : fake<const float>(kFakeAux);
            a.ep.res_fs = static_cast<long>(g.tensors[f.res].elems());
            a.ep.res_mode = f.res_mode;
            a.ep.res_C = shape(f.res).back();
        }
        return block_kernel_supports(a);
    }

    // DEPTHWISE 3x3 -> CONV 1x1 (stride 1) with the depthwise result consumed only by that conv.
    void fuse_blocks() {
        for (size_t i = 0; i < nodes.size(); i++) {
            Node& d = nodes[i];
            if (d.dead || d.kind != Node::Dw || d.act != ACT_NONE || d.res >= 0 || is_graph_output(d.out)) continue;
            if (d.KH != 3 || d.KW != 3) continue;
            std::vector<int> cons = consumers(d.out);
            if (cons.size() != 1) continue;
            Node& c = nodes[cons[0]];
            if (c.kind != Node::Conv || c.KH != 1 || c.KW != 1 || c.sh != 1 || c.sw != 1 || c.in[0] != d.out) continue;
            if (c.res == d.out) continue;
            Node f = c;
            f.kind = Node::Block;
            f.in = d.in;
            f.w2 = c.w; f.b2 = c.b;
            f.w = d.w; f.b = d.b;
            f.KH = d.KH; f.KW = d.KW; f.sh = d.sh; f.sw = d.sw; f.padding = d.padding; f.ept = d.ept; f.epl = d.epl;
            f.src_ops = d.src_ops;
            f.src_ops.insert(f.src_ops.end(), c.src_ops.begin(), c.src_ops.end());
            if (!block_supported(f)) continue;
            d.dead = true;
            c = f;
        }
        // remaining plain 1x1 stride-1 convolutions also run on the MFMA kernel (no depthwise stage: w = -1)
        for (Node& c : nodes) {
            if (c.dead || c.kind != Node::Conv || c.KH != 1 || c.KW != 1 || c.sh != 1 || c.sw != 1) continue;
            Node f = c;
            f.kind = Node::Block;
            f.w2 = c.w; f.b2 = c.b;
            f.w = -1; f.b = -1;
            if (!block_supported(f)) continue;
            c = f;
        }
    }
};

}  // namespace

std::vector<Node> rewrite_nodes(Graph& g, std::vector<Node> nodes, int fuse_level) {
    Rewriter rw{g, nodes};
    if (fuse_level >= 1) rw.fuse_affines();
    rw.lower_fully_connected();
    if (fuse_level >= 1) rw.fold_spatial_pads();
    if (fuse_level >= 1) rw.fuse_epilogues();
    if (fuse_level >= 2) rw.fuse_blocks();
    std::vector<Node> live;
    for (Node& n : nodes)
        if (!n.dead) live.push_back(std::move(n));
    return live;
}

}  // namespace plan_detail
}  // namespace mi
