// plan_widen.cpp — pad_odd_channels: a Graph -> Graph rewrite in front of the lowering (level 2 and up; see plan.hpp).
//
// Activation tensors whose channel count is not a multiple of 4 (front / short-range: 36 -> 42 -> 48) keep their layers off every
// fused kernel (float4 pixels everywhere).  Such a tensor — together with everything tied to it by channel-preserving operators
// (depthwise conv, ADD, RELU / PRELU, MAX_POOL) — is widened to the next multiple of 4 with channels that are exactly zero: the
// producing convolution gets zero filter rows and biases, depthwise stages zero taps and biases, PRELU a zero slope, a per-channel MUL / ADD
// constant the scale 1 / the shift 0 (0 * 1 + 0 is exactly zero), consuming
// convolutions zero filter columns, and channel PADs on either side (zeros appended at the high end) append
// or remove correspondingly fewer / more.  Every real channel computes what it computed before, bit for bit.  Classes that touch a
// graph input / output or an operator not listed here are left alone.
#include "plan_internal.hpp"

#include <cstdlib>
#include <map>
#include <set>

namespace mi {
namespace plan_detail {
namespace {

struct UnionFind {
    std::vector<int> parent;
    explicit UnionFind(int n) : parent(static_cast<size_t>(n)) {
        for (int t = 0; t < n; t++) parent[t] = t;
    }
    int find(int t) {
        int root = t;
        while (parent[root] != root) root = parent[root];
        for (int next; parent[t] != root; t = next) { next = parent[t]; parent[t] = root; }
        return root;
    }
    void unite(int a, int b) { if (a >= 0 && b >= 0) parent[find(a)] = find(b); }
};

// MUL / ADD by a constant: the activation operand, and whether the constant can follow a widening (a scalar factor needs none, a [.., C] constant
// grows with the tensor; anything else is left to the lowering's error message and keeps its class as it is)
int affine_x(const Graph& g, const OpInfo& op) {
    const bool c0 = g.tensors[op.inputs[0]].is_const, c1 = g.tensors[op.inputs[1]].is_const;
    return c0 == c1 ? -1 : (c0 ? op.inputs[1] : op.inputs[0]);
}
int affine_c(const Graph& g, const OpInfo& op) { return g.tensors[op.inputs[0]].is_const ? op.inputs[0] : op.inputs[1]; }
bool affine_widens(const Graph& g, const OpInfo& op) {
    const int x = affine_x(g, op);
    if (x < 0 || g.tensors[x].shape.empty()) return false;
    const TensorInfo& ct = g.tensors[affine_c(g, op)];
    const int C = g.tensors[x].shape.back();
    if (ct.f32.size() != ct.elems()) return false;
    if (ct.elems() == 1) return op.op == BuiltinOp::Mul;   // (a scalar shift would fill the appended channels, which must stay zero)
    return C >= 1 && ct.elems() == static_cast<size_t>(C) && !ct.shape.empty() && ct.shape.back() == C;
}

// Untrusted graphs reach this pass before the lowering has checked them: anything that is not the plain, consistent form
// handled below leaves the graph as it is (and to the lowering's own error messages).
bool plain_form(const Graph& g) {
    for (const OpInfo& op : g.ops) {
        if (op.inputs.empty() || op.outputs.empty()) return false;
        auto cst = [&](int t, size_t rank) {
            return t >= 0 && g.tensors[t].is_const && g.tensors[t].shape.size() == rank && g.tensors[t].f32.size() == g.tensors[t].elems() && g.tensors[t].elems() > 0;
        };
        auto r4 = [&](int t) { return t >= 0 && !g.tensors[t].is_const && g.tensors[t].shape.size() == 4 && g.tensors[t].shape.back() > 0; };
        const int in = op.inputs[0], out = op.outputs[0];
        if (op.op == BuiltinOp::Conv2D || op.op == BuiltinOp::DepthwiseConv2D) {
            if (op.inputs.size() < 2 || !r4(in) || !r4(out) || !cst(op.inputs[1], 4)) return false;
            const auto& ws = g.tensors[op.inputs[1]].shape;
            const int Ci = g.tensors[in].shape.back(), Co = g.tensors[out].shape.back();
            if (op.op == BuiltinOp::Conv2D ? (ws[0] != Co || ws[3] != Ci) : (ws[0] != 1 || ws[3] != Ci || Ci != Co)) return false;
            if (op.inputs.size() > 2 && op.inputs[2] >= 0 && !(cst(op.inputs[2], 1) && g.tensors[op.inputs[2]].shape[0] == Co)) return false;
        } else if (op.op == BuiltinOp::Prelu) {
            if (op.inputs.size() < 2 || !r4(in) || !r4(out)) return false;
            const TensorInfo& al = g.tensors[op.inputs[1]];
            if (!al.is_const || al.shape.empty() || al.f32.size() != al.elems() || static_cast<int>(al.elems()) != g.tensors[in].shape.back() ||
                al.shape.back() != g.tensors[in].shape.back()) return false;
        } else if (op.op == BuiltinOp::Pad) {
            if (op.inputs.size() < 2 || op.inputs[1] < 0 || !g.tensors[op.inputs[1]].is_const) return false;
        } else if (op.op == BuiltinOp::Add || op.op == BuiltinOp::Mul) {
            if (op.inputs.size() < 2 || op.inputs[0] < 0 || op.inputs[1] < 0) return false;
        }
    }
    for (const TensorInfo& t : g.tensors)
        if (!t.is_const && t.shape.empty()) return false;
    return true;
}

// The decision: which activation tensor gets which channel count.
struct Widths {
    const Graph& g;
    const int NT;
    UnionFind cls;            // channel classes: tensors tied by channel-preserving operators
    std::vector<char> bad;    // per class root: left alone
    UnionFind grp;            // growth groups, over class roots
    struct GroupInfo { int maxC = 0, H = 0, W = 0, classes = 0; bool ok = true; };
    std::map<int, GroupInfo> groups;  // by group root (a class root)

    explicit Widths(const Graph& graph) : g(graph), NT(static_cast<int>(graph.tensors.size())), cls(NT), bad(static_cast<size_t>(NT), 0), grp(NT) {}
    bool act(int t) const { return t >= 0 && t < NT && !g.tensors[t].is_const; }
    void mark(int t) { if (act(t)) bad[cls.find(t)] = 1; }

    void channel_classes() {
        for (const OpInfo& op : g.ops) {
            switch (op.op) {
                case BuiltinOp::DepthwiseConv2D: case BuiltinOp::Relu: case BuiltinOp::Prelu: case BuiltinOp::MaxPool2D:
                    cls.unite(op.inputs.at(0), op.outputs.at(0));
                    break;
                case BuiltinOp::Add:
                    cls.unite(op.inputs.at(0), op.outputs.at(0));
                    if (act(op.inputs.at(1))) cls.unite(op.inputs.at(1), op.outputs.at(0));
                    break;
                case BuiltinOp::Mul:
                    if (affine_x(g, op) >= 0) cls.unite(affine_x(g, op), op.outputs.at(0));
                    break;
                default: break;
            }
        }
        for (int t : g.inputs) mark(t);
        for (int t : g.outputs) mark(t);
        for (int t = 0; t < NT; t++)
            if (act(t) && g.tensors[t].shape.size() != 4) mark(t);
        for (const OpInfo& op : g.ops) {
            switch (op.op) {
                case BuiltinOp::Conv2D: case BuiltinOp::DepthwiseConv2D: case BuiltinOp::Relu: case BuiltinOp::MaxPool2D:
                    break;
                case BuiltinOp::Prelu:
                    if (!g.tensors[op.inputs.at(1)].is_const) mark(op.inputs[0]);
                    break;
                case BuiltinOp::Add:
                case BuiltinOp::Mul:
                    if (act(op.inputs.at(0)) && act(op.inputs.at(1)) && op.op == BuiltinOp::Add) break;
                    if (!affine_widens(g, op)) { mark(op.inputs[0]); mark(op.inputs[1]); mark(op.outputs.at(0)); }  // (a constant that cannot follow, MUL of two activations)
                    break;
                case BuiltinOp::Pad: {
                    const auto& pd = g.tensors[op.inputs.at(1)].i32;
                    bool channel_only = pd.size() == 8;
                    for (size_t k = 0; k < 7 && channel_only; k++) channel_only = pd[k] == 0;
                    if (!channel_only) { mark(op.inputs[0]); mark(op.outputs[0]); }
                    break;
                }
                default:  // RESHAPE, CONCATENATION, RESIZE_BILINEAR, DEPTH_TO_SPACE ...: the channel count is part of their meaning
                    for (int t : op.inputs) mark(t);
                    for (int t : op.outputs) mark(t);
                    break;
            }
        }
    }

    // Growth groups: classes tied by the channel PAD on the skip of a stride-1 block (the front / short-range graph widens 32 -> 36 -> 42
    // and 48 -> 56 -> ... -> 88 that way, a few channels per block).  Widened to ONE width, such a run becomes a run of same-shape
    // blocks with plain skips — the shape the fast kernels exist for (BackCamera's: 48 channels on 32-pixel-wide frames, 96 on
    // frames of at most 256 pixels) — and its PADs disappear.  The price is arithmetic on zeros; the gain is kernels and launches
    // (front: five 16x16 blocks of 48..88 channels -> one frame-resident chain).  Only PADs that read a block's own input count: the
    // stride-2 blocks' PADs (behind the max-pool) separate the groups.
    void growth_groups() {
        static const bool no_groups = getenv("MI_NO_WIDEN_GROUPS") != nullptr;  // tuning aid
        if (no_groups) return;
        std::vector<char> from_pool(static_cast<size_t>(NT), 0);
        for (const OpInfo& op : g.ops)
            if (op.op == BuiltinOp::MaxPool2D) from_pool[op.outputs[0]] = 1;
        auto joins = [&](const OpInfo& op) {
            if (op.op != BuiltinOp::Pad) return false;
            const int in = op.inputs.at(0), out = op.outputs.at(0);
            return act(in) && !from_pool[in] && !bad[cls.find(in)] && !bad[cls.find(out)];
        };
        for (const OpInfo& op : g.ops)
            if (joins(op)) grp.unite(cls.find(op.inputs[0]), cls.find(op.outputs[0]));
        std::map<int, std::set<int>> members;
        for (const OpInfo& op : g.ops)
            if (joins(op)) {
                const int in = op.inputs[0], out = op.outputs[0];
                const int root = grp.find(cls.find(out));
                GroupInfo& gi = groups[root];
                const auto& sh = g.tensors[out].shape;
                if (gi.H == 0) { gi.H = sh[1]; gi.W = sh[2]; }
                gi.ok &= gi.H == sh[1] && gi.W == sh[2];
                gi.maxC = std::max({gi.maxC, g.tensors[in].shape.back(), sh.back()});
                members[root].insert(cls.find(in));
                members[root].insert(cls.find(out));
            }
        for (auto& kv : groups) kv.second.classes = static_cast<int>(members[kv.first].size());
    }
    int group_width(int t) {  // 0: the tensor's class is in no group that gets one width
        auto it = groups.find(grp.find(cls.find(t)));
        if (it == groups.end() || !it->second.ok || it->second.classes < 2) return 0;
        const GroupInfo& gi = it->second;
        if (gi.H * gi.W <= 256 && ((gi.maxC + 31) & ~31) <= 128) return (gi.maxC + 31) & ~31;  // frame-resident chains: whole 32-channel tiles
        if (gi.W == 32 && gi.H * gi.W <= 1024 && gi.maxC > 32 && gi.maxC <= 48) return 48;     // mstrip_kernel
        return 0;
    }
    int padded(int t) {  // new channel count of activation tensor t (unchanged when its class is left alone)
        const int C = g.tensors[t].shape.back();
        if (!(act(t) && g.tensors[t].shape.size() == 4 && !bad[cls.find(t)])) return C;
        const int gw = group_width(t);
        if (gw >= C) return gw;
        return (C & 3) ? (C + 3) & ~3 : C;
    }

    // a channel PAD that consumes a widened tensor must have room for the extra channels.  Marking a class changes what its
    // neighbours (and its growth group) are padded to, so the check runs to a fixpoint (a single pass could leave an
    // earlier PAD with a negative amount on crafted graphs)
    // (a pass counts as a change only when a class really flips — a PAD whose data input is a constant can never be marked
    // (mark() skips constants), and with a shrinking output it kept the loop spinning on crafted graphs; every flip is permanent and
    // there are at most NT classes, so the loop ends)
    void shrink_to_fit_pads() {
        auto flip = [&](int t) {
            if (!act(t) || bad[cls.find(t)]) return false;
            bad[cls.find(t)] = 1;
            return true;
        };
        for (bool changed = true; changed;) {
            changed = false;
            for (const OpInfo& op : g.ops)
                if (op.op == BuiltinOp::Pad) {
                    const int in = op.inputs.at(0), out = op.outputs.at(0);
                    if (padded(out) - padded(in) >= 0) continue;
                    const bool a = flip(in), b = flip(out);
                    changed |= a || b;
                }
        }
    }

    // last line of defence before anything is rewritten: the new widths must be consistent operator by operator, or the graph stays
    // exactly as it was stored
    bool consistent(const std::vector<int>& newC) const {
        for (const OpInfo& op : g.ops) {
            const int in = op.inputs.at(0), out = op.outputs.at(0);
            switch (op.op) {
                case BuiltinOp::Pad:
                    if (act(in) && newC[out] - newC[in] < 0) return false;
                    break;
                case BuiltinOp::DepthwiseConv2D: case BuiltinOp::Relu: case BuiltinOp::Prelu: case BuiltinOp::MaxPool2D:
                    if (act(in) && newC[in] != newC[out]) return false;
                    break;
                case BuiltinOp::Add:
                case BuiltinOp::Mul:
                    if ((act(in) && newC[in] != newC[out]) || (act(op.inputs.at(1)) && newC[op.inputs[1]] != newC[out])) return false;
                    break;
                default: break;
            }
        }
        return true;
    }
};

// Constants, shapes and PAD amounts follow the new channel counts newC (per tensor of the graph as it came in; 0 for constants).
void rewrite_constants(Graph& g, const std::vector<int>& newC, std::vector<double>* logical_elems, std::vector<int>* logical_C) {
    const int NT = static_cast<int>(newC.size());
    auto act = [&](int t) { return t >= 0 && t < NT && !g.tensors[t].is_const; };
    auto clone_const = [&](int t) {  // constants may be shared between operators: every change goes to a private copy
        g.tensors.push_back(g.tensors[t]);
        logical_elems->push_back((*logical_elems)[t]);
        logical_C->push_back((*logical_C)[t]);
        return static_cast<int>(g.tensors.size()) - 1;
    };
    auto widen_last = [&](int t, int Cn, float fill = 0.f) {  // [..., C] -> [..., Cn], zeros appended (filters [*,kh,kw,I], taps [1,kh,kw,C], bias / alpha [C]; a MUL's scale: ones)
        TensorInfo& ti = g.tensors[t];
        const int C = ti.shape.back();
        const size_t rows = ti.elems() / static_cast<size_t>(C);
        std::vector<float> w(rows * Cn, fill);
        for (size_t r = 0; r < rows; r++)
            for (int c = 0; c < C; c++) w[r * Cn + c] = ti.f32[r * C + c];
        ti.f32 = std::move(w);
        ti.shape.back() = Cn;
    };
    auto widen_first = [&](int t, int On) {  // [O, ...] -> [On, ...], zero filters appended
        TensorInfo& ti = g.tensors[t];
        const size_t per = ti.elems() / static_cast<size_t>(ti.shape[0]);
        ti.f32.resize(per * On, 0.f);
        ti.shape[0] = On;
    };
    for (OpInfo& op : g.ops) {
        const int in = op.inputs.at(0), out = op.outputs.at(0);
        const int Ci = act(in) ? g.tensors[in].shape.back() : 0, Co = g.tensors[out].shape.back();
        const int Cin = act(in) ? newC[in] : 0, Con = newC[out];
        if (op.op == BuiltinOp::Conv2D) {
            if (Cin != Ci || Con != Co) {
                op.inputs[1] = clone_const(op.inputs[1]);
                if (Cin != Ci) widen_last(op.inputs[1], Cin);
                if (Con != Co) widen_first(op.inputs[1], Con);
            }
            if (Con != Co && op.inputs.size() > 2 && op.inputs[2] >= 0) { op.inputs[2] = clone_const(op.inputs[2]); widen_last(op.inputs[2], Con); }
        } else if (op.op == BuiltinOp::DepthwiseConv2D && Con != Co) {
            op.inputs[1] = clone_const(op.inputs[1]);
            widen_last(op.inputs[1], Con);
            if (op.inputs.size() > 2 && op.inputs[2] >= 0) { op.inputs[2] = clone_const(op.inputs[2]); widen_last(op.inputs[2], Con); }
        } else if (op.op == BuiltinOp::Prelu && Con != Co) {
            op.inputs[1] = clone_const(op.inputs[1]);
            widen_last(op.inputs[1], Con);
        } else if ((op.op == BuiltinOp::Add || op.op == BuiltinOp::Mul) && Con != Co && affine_x(g, op) >= 0 && g.tensors[affine_c(g, op)].elems() != 1) {
            const int k = g.tensors[op.inputs[0]].is_const ? 0 : 1;
            op.inputs[k] = clone_const(op.inputs[k]);
            widen_last(op.inputs[k], Con, op.op == BuiltinOp::Mul ? 1.f : 0.f);
        } else if (op.op == BuiltinOp::Pad && (Cin != Ci || Con != Co)) {
            op.inputs[1] = clone_const(op.inputs[1]);
            g.tensors[op.inputs[1]].i32[7] = Con - Cin;
        }
    }
    for (int t = 0; t < NT; t++)
        if (act(t)) g.tensors[t].shape.back() = newC[t];
}

// channel PADs that no longer append anything: their output is their input
void remove_empty_pads(Graph& g, int NT) {
    auto act = [&](int t) { return t >= 0 && t < NT && !g.tensors[t].is_const; };
    std::vector<OpInfo> kept;
    std::map<int, int> alias;
    auto resolve = [&](int t) { for (auto it = alias.find(t); it != alias.end(); it = alias.find(t)) t = it->second; return t; };
    for (OpInfo& op : g.ops) {
        for (int& t : op.inputs) t = t >= 0 ? resolve(t) : t;
        if (op.op == BuiltinOp::Pad && act(op.inputs[0]) && g.tensors[op.inputs[1]].i32.size() == 8 && g.tensors[op.inputs[1]].i32[7] == 0 &&
            g.tensors[op.inputs[0]].shape == g.tensors[op.outputs[0]].shape) {
            alias[op.outputs[0]] = op.inputs[0];
            continue;
        }
        kept.push_back(std::move(op));
    }
    g.ops = std::move(kept);
    for (int& t : g.outputs) t = resolve(t);
}

}  // namespace

void pad_odd_channels(Graph& g, std::vector<double>* logical_elems, std::vector<int>* logical_C) {
    const int NT = static_cast<int>(g.tensors.size());
    logical_elems->resize(NT);
    logical_C->resize(NT);
    for (int t = 0; t < NT; t++) {
        (*logical_elems)[t] = static_cast<double>(g.tensors[t].elems());
        (*logical_C)[t] = g.tensors[t].shape.empty() ? 0 : g.tensors[t].shape.back();
    }
    if (!plain_form(g)) return;
    Widths w(g);
    w.channel_classes();
    w.growth_groups();
    w.shrink_to_fit_pads();
    std::vector<int> newC(NT);
    bool any = false;
    for (int t = 0; t < NT; t++) {
        newC[t] = w.act(t) ? w.padded(t) : 0;
        any |= w.act(t) && newC[t] != g.tensors[t].shape.back();
    }
    if (!any || !w.consistent(newC)) return;
    rewrite_constants(g, newC, logical_elems, logical_C);
    remove_empty_pads(g, NT);
}

}  // namespace plan_detail
}  // namespace mi
