// layout.hpp — layout normalisation of ONNX-exported graphs (included by plan.cpp; a Graph -> Graph rewrite at the head of the lowering, every level).
//
// ONNX converters keep the element-wise operators channel-first — batch-norm constants [1,C,1,1], PRELU slopes [C,1,1], PAD on axes 2 and 3, the ADD
// of the skip on NCHW tensors — wrap every convolution in TRANSPOSE (0,2,3,1) ... TRANSPOSE (0,3,1,2), and flatten in C,H,W order in front of the
// FULLY_CONNECTED.  A tensor is CHANNEL-FIRST here when it is the output of TRANSPOSE (0,3,1,2) of an NHWC activation, or of an operator rewritten
// below; for each such tensor the pass keeps the NHWC tensor that holds the same values, and rewrites its readers onto that tensor:
//   RELU                                            on the NHWC tensor
//   PRELU, C slopes shaped [C,1,1] / [1,C,1,1]      the constant cloned to [1,1,C]
//   ADD / SUB / MUL / DIV by a scalar or by C
//     values shaped [1,C,1,1] / [C,1,1]             the constant cloned to [C]
//   ADD of two channel-first tensors of one shape   on both NHWC tensors
//   PAD [[0,0],[0,0],[t,b],[l,r]]                   paddings permuted to [[0,0],[t,b],[l,r],[0,0]]
//   AVERAGE_POOL_2D / MAX_POOL_2D                   refused: TFLite pools are NHWC, such a graph is malformed
//   MEAN over axes {2,3}                            axes {1,2}
//   RESHAPE to [1,C*H*W] read only by
//     FULLY_CONNECTED operators                     their weight columns permuted once, (c,h,w) -> (h,w,c); the RESHAPE reads the NHWC tensor
//   TRANSPOSE (0,2,3,1)                             disappears: its output IS the NHWC tensor
// Any other reader — a graph output is one — gets ONE materialised TRANSPOSE (0,3,1,2) launch of the NHWC tensor, shared by all such readers: that is
// always correct, so a row that does not apply costs a launch, never an answer.  A graph without TRANSPOSE (0,3,1,2) comes out exactly as it went in.
// Untrusted graphs reach this pass unchecked: every shape, index and constant is verified before it is used; what is not the plain form is left to the
// fallback and to the lowering's own messages.
#pragma once

#include <algorithm>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "tflite_graph.hpp"

namespace mi {
namespace layout_detail {

inline void normalise_layout(Graph& g) {
    const int NT0 = static_cast<int>(g.tensors.size());
    auto valid = [&](int t) { return t >= 0 && t < static_cast<int>(g.tensors.size()); };
    auto act4 = [&](int t) {
        if (!valid(t) || g.tensors[t].is_const || g.tensors[t].shape.size() != 4) return false;
        for (int d : g.tensors[t].shape)
            if (d < 1 || d > (1 << 24)) return false;
        return true;
    };
    auto perm_of = [&](const OpInfo& op, std::vector<int>* p) {
        if (op.op != BuiltinOp::Transpose || op.inputs.size() < 2 || op.outputs.empty() || !valid(op.inputs[1])) return false;
        const TensorInfo& pt = g.tensors[op.inputs[1]];
        if (!pt.is_const || pt.dtype != 2 || pt.i32.size() != 4) return false;
        p->assign(pt.i32.begin(), pt.i32.end());
        return true;
    };
    bool any = false;
    for (const OpInfo& op : g.ops) {
        std::vector<int> p;
        any = any || (perm_of(op, &p) && p == std::vector<int>{0, 3, 1, 2});
    }
    if (!any) return;

    std::map<int, int> nhwc;      // channel-first tensor -> the NHWC tensor that holds the same values
    std::map<int, int> alias;     // output of a removed TRANSPOSE (0,2,3,1) -> the NHWC tensor it is
    std::set<int> materialised;   // channel-first tensors that a TRANSPOSE launch really writes
    std::vector<OpInfo> out;
    int perm_const = -1;
    auto cf = [&](int t) { return nhwc.count(t) != 0; };
    auto resolve = [&](int t) { for (auto it = alias.find(t); it != alias.end(); it = alias.find(t)) t = it->second; return t; };
    auto new_act = [&](std::vector<int> shape) {
        TensorInfo t;
        t.shape = std::move(shape);
        g.tensors.push_back(std::move(t));
        return static_cast<int>(g.tensors.size()) - 1;
    };
    auto clone_const = [&](int t) {  // constants may be shared between operators: every change goes to a private copy
        g.tensors.push_back(TensorInfo(g.tensors[t]));
        return static_cast<int>(g.tensors.size()) - 1;
    };
    auto materialise = [&](int t) {  // one TRANSPOSE (0,3,1,2) launch of the NHWC tensor writes the channel-first tensor itself
        if (!cf(t) || materialised.count(t)) return;
        if (perm_const < 0) {
            TensorInfo p;
            p.shape = {4}; p.dtype = 2; p.is_const = true; p.i32 = {0, 3, 1, 2};
            g.tensors.push_back(std::move(p));
            perm_const = static_cast<int>(g.tensors.size()) - 1;
        }
        OpInfo tr;
        tr.op = BuiltinOp::Transpose; tr.raw_code = static_cast<int>(BuiltinOp::Transpose);
        tr.inputs = {nhwc[t], perm_const}; tr.outputs = {t};
        out.push_back(std::move(tr));
        materialised.insert(t);
    };
    // channel-first [1,C,H,W] as NHWC [1,H,W,C]
    auto to_nhwc_shape = [](const std::vector<int>& s) { return std::vector<int>{s[0], s[2], s[3], s[1]}; };
    // a constant of C values along the channel axis of a channel-first tensor: [1,C,1,1] or [C,1,1]
    auto channel_const = [&](int t, int C) {
        if (!valid(t) || !g.tensors[t].is_const) return false;
        const TensorInfo& ct = g.tensors[t];
        return ct.f32.size() == static_cast<size_t>(C) && (ct.shape == std::vector<int>{1, C, 1, 1} || ct.shape == std::vector<int>{C, 1, 1});
    };
    auto scalar_const = [&](int t) { return valid(t) && g.tensors[t].is_const && g.tensors[t].f32.size() == 1 && g.tensors[t].elems() == 1; };

    for (size_t oi = 0; oi < g.ops.size(); oi++) {
        OpInfo op = g.ops[oi];
        for (int& t : op.inputs) t = t >= 0 ? resolve(t) : t;
        const int x = op.inputs.empty() ? -1 : op.inputs[0], y = op.outputs.empty() ? -1 : op.outputs[0];
        bool done = false;
        std::vector<int> p;
        if (perm_of(op, &p) && valid(y)) {
            const std::vector<int>& so = g.tensors[y].shape;
            if (p == std::vector<int>{0, 3, 1, 2} && act4(x) && !cf(x) && !cf(y) && y != x && so == std::vector<int>{g.tensors[x].shape[0], g.tensors[x].shape[3], g.tensors[x].shape[1], g.tensors[x].shape[2]} &&
                !g.tensors[y].is_const) {
                nhwc[y] = x;   // nothing runs: readers are rewritten, or get the one materialised launch
                continue;
            }
            // (a graph output cannot be the graph input or a second name of another output: such a pair of transposes keeps its two launches)
            auto listed = [&](const std::vector<int>& v, int t) { return std::find(v.begin(), v.end(), t) != v.end(); };
            const bool pinned = cf(x) && listed(g.outputs, y) && (listed(g.inputs, nhwc[x]) || listed(g.outputs, nhwc[x]));
            if (p == std::vector<int>{0, 2, 3, 1} && cf(x) && !pinned && so == g.tensors[nhwc[x]].shape && !g.tensors[y].is_const && !cf(y)) {
                alias[y] = nhwc[x];
                continue;
            }
        }
        if (valid(x) && cf(x) && valid(y) && !g.tensors[y].is_const && !cf(y) && y >= 0 && y < NT0) {
            const std::vector<int> xs = g.tensors[x].shape;            // [1,C,H,W]
            const int xn = nhwc[x], C = xs[1];
            const bool same_shape = g.tensors[y].shape == xs;
            auto elementwise = [&] {  // the operator moves to the NHWC tensors: its output becomes channel-first with an NHWC twin of its own
                op.outputs[0] = new_act(g.tensors[xn].shape);
                nhwc[y] = op.outputs[0];
                done = true;
            };
            switch (op.op) {
                case BuiltinOp::Relu:
                    if (same_shape) { op.inputs[0] = xn; elementwise(); }
                    break;
                case BuiltinOp::Prelu:
                    if (same_shape && op.inputs.size() >= 2 && channel_const(op.inputs[1], C)) {
                        op.inputs[1] = clone_const(op.inputs[1]);
                        g.tensors[op.inputs[1]].shape = {1, 1, C};
                        op.inputs[0] = xn; elementwise();
                    }
                    break;
                case BuiltinOp::AveragePool2D: case BuiltinOp::MaxPool2D:
                    throw std::runtime_error(std::string("plan: ") + (op.op == BuiltinOp::MaxPool2D ? "MAX_POOL_2D" : "AVERAGE_POOL_2D") +
                                             " of a channel-first tensor (the output of TRANSPOSE (0,3,1,2)) unsupported: TFLite pools are NHWC, the graph is malformed");
                case BuiltinOp::Pad:
                    if (op.inputs.size() >= 2 && valid(op.inputs[1]) && g.tensors[op.inputs[1]].is_const && g.tensors[op.inputs[1]].dtype == 2 && g.tensors[op.inputs[1]].i32.size() == 8) {
                        const std::vector<int32_t> pv = g.tensors[op.inputs[1]].i32;   // [[n,n],[c,c],[t,b],[l,r]]
                        bool ok = pv[0] == 0 && pv[1] == 0 && pv[2] == 0 && pv[3] == 0;
                        for (int k = 4; k < 8; k++) ok = ok && pv[k] >= 0 && pv[k] <= (1 << 16);
                        if (ok && g.tensors[y].shape == std::vector<int>{xs[0], C, xs[2] + pv[4] + pv[5], xs[3] + pv[6] + pv[7]}) {
                            op.inputs[1] = clone_const(op.inputs[1]);
                            g.tensors[op.inputs[1]].i32 = {0, 0, pv[4], pv[5], pv[6], pv[7], 0, 0};
                            op.inputs[0] = xn;
                            op.outputs[0] = new_act(to_nhwc_shape(g.tensors[y].shape));
                            nhwc[y] = op.outputs[0];
                            done = true;
                        }
                    }
                    break;
                case BuiltinOp::Mean:
                    if (op.inputs.size() >= 2 && valid(op.inputs[1]) && g.tensors[op.inputs[1]].is_const && g.tensors[op.inputs[1]].dtype == 2 && !g.tensors[op.inputs[1]].i32.empty() &&
                        g.tensors[op.inputs[1]].i32.size() <= 8) {
                        std::set<int> axes;
                        bool ok = true;
                        for (int32_t a : g.tensors[op.inputs[1]].i32) {
                            ok = ok && a >= -4 && a < 4;
                            axes.insert(a < 0 ? a + 4 : a);
                        }
                        const std::vector<int> want = op.keep_dims ? std::vector<int>{xs[0], C, 1, 1} : std::vector<int>{xs[0], C};
                        if (ok && axes == std::set<int>{2, 3} && g.tensors[y].shape == want) {
                            op.inputs[1] = clone_const(op.inputs[1]);
                            g.tensors[op.inputs[1]].shape = {2};
                            g.tensors[op.inputs[1]].i32 = {1, 2};
                            op.inputs[0] = xn;
                            if (op.keep_dims) {   // [1,C,1,1] is the channel-first form of [1,1,1,C]
                                op.outputs[0] = new_act({xs[0], 1, 1, C});
                                nhwc[y] = op.outputs[0];
                            }
                            done = true;
                        }
                    }
                    break;
                case BuiltinOp::Reshape: {
                    // the C,H,W flatten in front of FULLY_CONNECTED operators: their weight columns move to H,W,C order, once
                    const long HW = static_cast<long>(xs[2]) * xs[3];
                    if (HW > (1L << 24) || C * HW > (1L << 24)) break;   // (a constant, and so a weight row, has at most 2^24 elements)
                    const long K = C * HW;
                    if (xs[0] != 1 || g.tensors[y].shape != std::vector<int>{1, static_cast<int>(K)}) break;
                    std::vector<size_t> fcs;
                    bool ok = std::find(g.outputs.begin(), g.outputs.end(), y) == g.outputs.end();
                    for (size_t k = 0; k < g.ops.size() && ok; k++) {
                        const OpInfo& r = g.ops[k];
                        if (std::find(r.inputs.begin(), r.inputs.end(), y) == r.inputs.end()) continue;
                        ok = k > oi && r.op == BuiltinOp::FullyConnected && r.inputs.size() >= 2 && r.inputs[0] == y && std::count(r.inputs.begin(), r.inputs.end(), y) == 1 && valid(r.inputs[1]);
                        if (!ok) break;
                        const TensorInfo& wt = g.tensors[r.inputs[1]];
                        ok = wt.is_const && wt.shape.size() == 2 && wt.shape[0] >= 1 && wt.shape[1] == K && wt.f32.size() == wt.elems();
                        fcs.push_back(k);
                    }
                    if (!ok || fcs.empty()) break;
                    const int H = xs[2], W = xs[3];
                    for (size_t k : fcs) {
                        const int w = clone_const(g.ops[k].inputs[1]);
                        const std::vector<float> src = g.tensors[w].f32;
                        std::vector<float>& dst = g.tensors[w].f32;
                        const long N = g.tensors[w].shape[0];
                        for (long n = 0; n < N; n++)
                            for (int c = 0; c < C; c++)
                                for (int h = 0; h < H; h++)
                                    for (int q = 0; q < W; q++) dst[n * K + (static_cast<long>(h) * W + q) * C + c] = src[n * K + (static_cast<long>(c) * H + h) * W + q];
                        g.ops[k].inputs[1] = w;
                    }
                    op.inputs[0] = xn;
                    done = true;
                    break;
                }
                case BuiltinOp::Add: case BuiltinOp::Sub: case BuiltinOp::Mul: case BuiltinOp::Div:
                default:
                    break;
            }
        }
        // ADD / SUB / MUL / DIV: the channel-first operand may be either input
        if (!done && (op.op == BuiltinOp::Add || op.op == BuiltinOp::Sub || op.op == BuiltinOp::Mul || op.op == BuiltinOp::Div) && op.inputs.size() >= 2 && valid(y) && !g.tensors[y].is_const &&
            !cf(y) && y < NT0 && valid(op.inputs[0]) && valid(op.inputs[1])) {
            const int a = op.inputs[0], b = op.inputs[1];
            if (cf(a) && cf(b) && op.op == BuiltinOp::Add && g.tensors[a].shape == g.tensors[b].shape && g.tensors[y].shape == g.tensors[a].shape) {
                op.inputs = {nhwc[a], nhwc[b]};
                op.outputs[0] = new_act(g.tensors[nhwc[a]].shape);
                nhwc[y] = op.outputs[0];
                done = true;
            } else if (cf(a) != cf(b)) {
                const int k = cf(a) ? 0 : 1, t = op.inputs[k], c = op.inputs[1 - k];
                const int C = g.tensors[t].shape[1];
                if (g.tensors[y].shape == g.tensors[t].shape && (scalar_const(c) || channel_const(c, C))) {
                    if (!scalar_const(c)) {
                        op.inputs[1 - k] = clone_const(c);
                        g.tensors[op.inputs[1 - k]].shape = {C};
                    }
                    op.inputs[k] = nhwc[t];
                    op.outputs[0] = new_act(g.tensors[nhwc[t]].shape);
                    nhwc[y] = op.outputs[0];
                    done = true;
                }
            }
        }
        if (!done)
            for (int t : op.inputs)
                if (t >= 0) materialise(t);
        out.push_back(std::move(op));
    }
    for (int& t : g.outputs) {
        t = t >= 0 ? resolve(t) : t;
        if (t >= 0) materialise(t);
    }
    g.ops = std::move(out);
}

}  // namespace layout_detail
}  // namespace mi
