// plan_ops.cpp — the head of the lowering: the checks an untrusted graph gets, and one Node per builtin operator (see plan.hpp).
#include "plan_internal.hpp"

#include <cmath>
#include <set>
#include <stdexcept>
#include <string>

namespace mi {
namespace plan_detail {
namespace {

int act_of(FusedAct a) {
    switch (a) {
        case FusedAct::None: return ACT_NONE;
        case FusedAct::Relu: return ACT_RELU;
        case FusedAct::Relu6: return ACT_RELU6;
    }
    throw std::runtime_error("plan: unsupported fused activation");
}

void need_const(const Graph& g, int t, const char* what) {
    if (t < 0 || !g.tensors[t].is_const) throw std::runtime_error(std::string("plan: ") + what + " must be a constant tensor");
}

// a [1,..] shape whose dimensions are all in 1 .. 2^24 (the first n of them)
bool dims_ok(const std::vector<int>& s, size_t n) {
    for (size_t d = 0; d < n; d++)
        if (s[d] < 1 || s[d] > (1 << 24)) return false;
    return true;
}

// CONV_2D / DEPTHWISE_CONV_2D
Node conv_node(const Graph& g, const OpInfo& op, Node n) {
    n.kind = op.op == BuiltinOp::Conv2D ? Node::Conv : Node::Dw;
    n.in = {op.inputs.at(0)};
    n.w = op.inputs.at(1);
    need_const(g, n.w, "convolution filter");
    n.b = op.inputs.size() > 2 ? op.inputs[2] : -1;
    if (n.b >= 0) need_const(g, n.b, "convolution bias");
    const auto& ws = g.tensors[n.w].shape;
    if (ws.size() != 4) throw std::runtime_error("plan: convolution filter must be rank 4");
    n.KH = ws[1]; n.KW = ws[2];
    n.sh = op.stride_h; n.sw = op.stride_w;
    n.padding = op.padding;
    n.act = act_of(op.act);
    if (n.kind == Node::Dw && (op.depth_multiplier != 1 || ws[0] != 1 || ws[3] != g.tensors[n.in[0]].shape.at(3)))
        throw std::runtime_error("plan: depthwise conv with depth_multiplier != 1 unsupported");
    if (n.kind == Node::Conv && ws[3] != g.tensors[n.in[0]].shape.at(3))
        throw std::runtime_error("plan: convolution channel mismatch");
    return n;
}

// FULLY_CONNECTED: a Node::Conv with `fc` set, which Rewriter::lower_fully_connected turns into the whole-frame convolution
Node fully_connected_node(const Graph& g, const OpInfo& op, Node n) {
    n.kind = Node::Conv;
    n.fc = true;
    if (op.inputs.size() < 2) throw std::runtime_error("plan: FULLY_CONNECTED without weights");
    n.in = {op.inputs[0]};
    n.w = op.inputs[1];
    n.b = op.inputs.size() > 2 ? op.inputs[2] : -1;
    if (n.w < 0 || !g.tensors[n.w].is_const) throw std::runtime_error("plan: FULLY_CONNECTED weights must be a constant tensor");
    if (n.b >= 0 && !g.tensors[n.b].is_const) throw std::runtime_error("plan: FULLY_CONNECTED bias must be a constant tensor");
    if (op.weights_format != 0)
        throw std::runtime_error("plan: FULLY_CONNECTED weights_format " + std::to_string(op.weights_format) + " unsupported (only DEFAULT: row-major [N][K])");
    const TensorInfo& wt = g.tensors[n.w];
    if (wt.shape.size() != 2 || wt.shape[0] < 1 || wt.shape[1] < 1 || wt.f32.size() != wt.elems())
        throw std::runtime_error("plan: FULLY_CONNECTED weights must be an f32 [N][K] constant");
    const int N = wt.shape[0], K = wt.shape[1];
    if (n.in[0] < 0 || g.tensors[n.in[0]].is_const) throw std::runtime_error("plan: FULLY_CONNECTED of a constant input unsupported");
    const TensorInfo& xt = g.tensors[n.in[0]];
    bool x_ok = (xt.shape.size() == 2 || xt.shape.size() == 4) && xt.shape[0] == 1;
    for (int d : xt.shape) x_ok = x_ok && d >= 1 && d <= (1 << 24);
    if (!x_ok) throw std::runtime_error("plan: FULLY_CONNECTED input must be [1,K] or [1,H,W,C]");
    if (xt.elems() != static_cast<size_t>(K))
        throw std::runtime_error("plan: FULLY_CONNECTED K = " + std::to_string(K) + " does not match its input's " + std::to_string(xt.elems()) + " elements");
    const TensorInfo& ot = g.tensors[n.out];
    if (ot.shape.size() == 4 && op.keep_num_dims) throw std::runtime_error("plan: FULLY_CONNECTED keep_num_dims with a rank-4 output unsupported");
    if (ot.shape.size() != 2 || ot.shape[0] != 1 || ot.shape[1] != N) throw std::runtime_error("plan: FULLY_CONNECTED output must be [1,N]");
    if (n.b >= 0 && (g.tensors[n.b].f32.size() != static_cast<size_t>(N) || g.tensors[n.b].elems() != static_cast<size_t>(N)))
        throw std::runtime_error("plan: FULLY_CONNECTED bias must be an f32 [N] constant");
    n.padding = Padding::Valid;
    n.act = act_of(op.act);
    return n;
}

// ADD / MUL / SUB / DIV: the ADD of two activations, or an affine of x's last dimension
Node arithmetic_node(const Graph& g, const OpInfo& op, Node n) {
    const bool mul = op.op == BuiltinOp::Mul, sub = op.op == BuiltinOp::Sub, div = op.op == BuiltinOp::Div;
    const std::string name = mul ? "MUL" : sub ? "SUB" : div ? "DIV" : "ADD";
    if (op.inputs.size() < 2) throw std::runtime_error("plan: " + name + " needs two operands");
    const int a = op.inputs[0], b = op.inputs[1];
    const bool ca = g.tensors[a].is_const, cb = g.tensors[b].is_const;
    n.act = act_of(op.act);
    if (!ca && !cb) {
        if (mul) throw std::runtime_error("plan: MUL of two activations unsupported (only MUL by a per-channel or scalar constant)");
        if (sub || div) throw std::runtime_error("plan: " + name + " of two activations unsupported (only " + name + " by a per-channel or scalar constant)");
        n.kind = Node::Add;
        n.in = {a, b};
        if (g.tensors[n.in[0]].shape != g.tensors[n.in[1]].shape) throw std::runtime_error("plan: broadcasting ADD unsupported");
        return n;
    }
    if (ca && cb) throw std::runtime_error("plan: " + name + " of two constants unsupported");
    // x * c / x + c, either operand order, c per channel (C elements, C its last dimension) or a scalar: an affine of x's last dimension
    const int x = ca ? b : a, c = ca ? a : b;
    const std::vector<int>& xs = g.tensors[x].shape;
    const TensorInfo& ct = g.tensors[c];
    const int C = xs.back();
    const size_t ce = ct.elems();
    const bool per_channel = C >= 1 && ce == static_cast<size_t>(C) && !ct.shape.empty() && ct.shape.back() == C, scalar = ce == 1;
    if (C < 1 || C > (1 << 16) || !(per_channel || scalar) || ct.f32.size() != ce)   // (65536 channels bound what a crafted graph makes a node allocate)
        throw std::runtime_error("plan: " + name + " by a constant that is neither per-channel ([C]) nor a scalar unsupported");
    if (g.tensors[n.out].shape != xs) throw std::runtime_error("plan: broadcasting " + name + " unsupported");
    n.kind = Node::Affine;
    n.in = {x};
    n.scale.assign(static_cast<size_t>(C), 1.f);
    n.shift.assign(static_cast<size_t>(C), 0.f);
    if (div && ca) throw std::runtime_error("plan: DIV of a constant by an activation (c / x) unsupported");
    // DIV: a divisor that is a power of two has an exact reciprocal, and x * (1 / c) is x / c bit for bit; any other divisor keeps a true
    // division (the node's divisor form), because x * (1 / c) is a different number
    bool pow2 = div;
    for (size_t k = 0; div && k < ce; k++) {
        const float v = ct.f32[k];
        if (!std::isfinite(v) || v == 0.f) throw std::runtime_error("plan: DIV by a zero or non-finite constant unsupported");
        int e = 0;
        pow2 = pow2 && std::fabs(std::frexp(v, &e)) == 0.5f && std::isnormal(v) && std::isnormal(1.f / v);
    }
    n.divide = div && !pow2;
    for (int k = 0; k < C; k++) {
        const float v = ct.f32[scalar ? 0 : static_cast<size_t>(k)];
        float& s = n.scale[static_cast<size_t>(k)];
        float& t = n.shift[static_cast<size_t>(k)];
        if (mul) s = v;
        else if (div) s = pow2 ? 1.f / v : v;
        else if (sub && ca) { s = -1.f; t = v; }   // c - x = (-x) + c
        else if (sub) t = -v;                      // x - c = x + (-c)
        else t = v;
    }
    return n;
}

Node average_pool_node(const Graph& g, const OpInfo& op, Node n) {
    n.kind = Node::Pool; n.in = {op.inputs.at(0)};
    n.filter_h = op.filter_h; n.filter_w = op.filter_w; n.sh = op.stride_h; n.sw = op.stride_w;
    n.padding = op.padding; n.act = act_of(op.act);
    const std::vector<int>&si = g.tensors[n.in[0]].shape, &so = g.tensors[n.out].shape;
    const bool ok = si.size() == 4 && so.size() == 4 && si[0] == 1 && n.filter_h >= 1 && n.filter_w >= 1 && n.sh >= 1 && n.sw >= 1 &&
                    (n.padding == Padding::Same || n.padding == Padding::Valid) && dims_ok(si, 4);
    if (!ok) throw std::runtime_error("plan: AVERAGE_POOL_2D needs a [1,H,W,C] input, a window and strides of at least 1");
    // (every output element has at least one in-frame tap: SAME's first tap of the last window is in the frame, VALID's windows are whole)
    const bool same = n.padding == Padding::Same;
    if (!same && (si[1] < n.filter_h || si[2] < n.filter_w)) throw std::runtime_error("plan: AVERAGE_POOL_2D VALID window larger than the frame");
    const int ho = same ? (si[1] + n.sh - 1) / n.sh : (si[1] - n.filter_h) / n.sh + 1, wo = same ? (si[2] + n.sw - 1) / n.sw : (si[2] - n.filter_w) / n.sw + 1;
    if (so != std::vector<int>{1, ho, wo, si[3]}) throw std::runtime_error("plan: AVERAGE_POOL_2D output shape does not match its window");
    return n;
}

// MEAN over H and W of a [1,H,W,C] tensor is the whole-frame average pool; without keep_dims its [1,C] output is a view of the [1,1,1,C] result: the
// pool and a RESHAPE behind it
std::vector<Node> mean_nodes(Graph& g, const OpInfo& op, Node n) {
    if (op.inputs.size() < 2) throw std::runtime_error("plan: MEAN needs its axes");
    n.kind = Node::Pool; n.in = {op.inputs[0]};
    const TensorInfo& at = g.tensors[op.inputs[1]];
    if (!at.is_const || at.dtype != 2 || at.i32.empty() || at.i32.size() > 8) throw std::runtime_error("plan: MEAN axes must be a constant int32 tensor");
    const std::vector<int> si = g.tensors[n.in[0]].shape, so = g.tensors[n.out].shape;
    if (!(si.size() == 4 && si[0] == 1 && dims_ok(si, 4))) throw std::runtime_error("plan: MEAN of a tensor that is not [1,H,W,C] unsupported");
    std::set<int> axes;
    for (int32_t a : at.i32) {
        if (a < -4 || a >= 4) throw std::runtime_error("plan: MEAN axis outside the input's rank");
        axes.insert(a < 0 ? a + 4 : a);
    }
    if (axes != std::set<int>{1, 2}) throw std::runtime_error("plan: MEAN over axes other than H and W (1, 2) unsupported");
    if (so != (op.keep_dims ? std::vector<int>{1, 1, 1, si[3]} : std::vector<int>{1, si[3]})) throw std::runtime_error("plan: MEAN output shape does not match its axes and keep_dims");
    n.filter_h = si[1]; n.filter_w = si[2]; n.sh = n.sw = 1; n.padding = Padding::Valid;
    if (op.keep_dims) return {n};
    Node r;
    r.kind = Node::Reshape; r.out = n.out; r.src_ops.clear();
    TensorInfo t4;
    t4.shape = {1, 1, 1, si[3]};
    g.tensors.push_back(std::move(t4));
    n.out = static_cast<int>(g.tensors.size()) - 1;
    r.in = {n.out};
    return {n, r};
}

Node l2_normalization_node(const Graph& g, const OpInfo& op, Node n) {
    n.kind = Node::L2Norm; n.in = {op.inputs.at(0)};
    if (op.act != FusedAct::None) throw std::runtime_error("plan: L2_NORMALIZATION with a fused activation unsupported");
    const std::vector<int>&si = g.tensors[n.in[0]].shape, &so = g.tensors[n.out].shape;
    if (!(si.size() >= 2 && si.size() <= 4 && si[0] == 1 && so == si && dims_ok(si, si.size())))
        throw std::runtime_error("plan: L2_NORMALIZATION needs a [1,..,D] tensor of rank 2 to 4 and an output of the same shape");
    return n;
}

Node transpose_node(const Graph& g, const OpInfo& op, Node n) {
    if (op.inputs.size() < 2) throw std::runtime_error("plan: TRANSPOSE needs its perm");
    n.kind = Node::Transpose; n.in = {op.inputs[0]};
    const TensorInfo& pt = g.tensors[op.inputs[1]];
    if (!pt.is_const || pt.dtype != 2 || pt.i32.empty()) throw std::runtime_error("plan: TRANSPOSE perm must be a constant int32 tensor");
    const std::vector<int>&si = g.tensors[n.in[0]].shape, &so = g.tensors[n.out].shape;
    if (!(si.size() == 4 && so.size() == 4 && pt.i32.size() == 4 && dims_ok(si, 4))) throw std::runtime_error("plan: TRANSPOSE of a tensor that is not rank 4 unsupported");
    int seen = 0;
    for (int32_t p : pt.i32) {
        if (p < 0 || p > 3 || (seen >> p & 1)) throw std::runtime_error("plan: TRANSPOSE perm is not a permutation of 0..3");
        seen |= 1 << p;
    }
    if (pt.i32[0] != 0 || si[0] != 1) throw std::runtime_error("plan: TRANSPOSE that moves the batch axis unsupported");
    for (size_t d = 0; d < 4; d++)
        if (so[d] != si[static_cast<size_t>(pt.i32[d])]) throw std::runtime_error("plan: TRANSPOSE output shape does not match its perm");
    n.perm.assign(pt.i32.begin(), pt.i32.end());
    if (n.perm == std::vector<int>{0, 1, 2, 3}) { n.kind = Node::Reshape; n.perm.clear(); }   // the identity: an alias of its input
    return n;
}

}  // namespace

// (untrusted bytes, mi_*_create_from_bytes: the reader has checked every tensor index; the lowering reads shape.back() of the tensors an
// operator touches — a crafted tensor of rank 0 made that a read in front of an empty vector, found under AddressSanitizer)
void check_untrusted_graph(const Graph& g) {
    for (const OpInfo& op : g.ops) {
        if (op.outputs.empty()) throw std::runtime_error("plan: operator without an output");
        for (int t : op.outputs)
            if (t < 0 || g.tensors[static_cast<size_t>(t)].shape.empty()) throw std::runtime_error("plan: operator output without a shape");
        // (but the scalar constant of a MUL / ADD, which converters store with rank 0)
        const bool affine_op = op.op == BuiltinOp::Mul || op.op == BuiltinOp::Add || op.op == BuiltinOp::Sub || op.op == BuiltinOp::Div;
        for (int t : op.inputs)
            if (t >= 0 && g.tensors[static_cast<size_t>(t)].shape.empty() && !(affine_op && g.tensors[static_cast<size_t>(t)].is_const))
                throw std::runtime_error("plan: operator input without a shape");
    }
    // (the reader checks the operators' tensor indices; a crafted subgraph's own input / output lists reach this point unchecked — a mutated output index
    // read behind the tensor table, found under AddressSanitizer)
    const size_t n_tensors = g.tensors.size();
    for (int t : g.inputs)
        if (t < 0 || static_cast<size_t>(t) >= n_tensors || g.tensors[static_cast<size_t>(t)].shape.empty()) throw std::runtime_error("plan: graph input without a shape");
    for (int t : g.outputs)
        if (t < 0 || static_cast<size_t>(t) >= n_tensors || g.tensors[static_cast<size_t>(t)].shape.empty()) throw std::runtime_error("plan: graph output without a shape");
}

std::vector<Node> nodes_of_graph(Graph& g) {
    std::vector<Node> nodes;
    for (size_t oi = 0; oi < g.ops.size(); oi++) {
        const OpInfo& op = g.ops[oi];
        Node n;
        n.out = op.outputs[0];
        n.src_ops = {static_cast<int>(oi)};
        auto emit = [&](Node&& m) {
            for (int t : m.in)
                if (t < 0 || g.tensors[t].is_const) throw std::runtime_error("plan: constant activation inputs unsupported");
            nodes.push_back(std::move(m));
        };
        switch (op.op) {
            case BuiltinOp::Conv2D:
            case BuiltinOp::DepthwiseConv2D: n = conv_node(g, op, std::move(n)); break;
            case BuiltinOp::FullyConnected: n = fully_connected_node(g, op, std::move(n)); break;
            case BuiltinOp::Add:
            case BuiltinOp::Mul:
            case BuiltinOp::Sub:
            case BuiltinOp::Div: n = arithmetic_node(g, op, std::move(n)); break;
            case BuiltinOp::AveragePool2D: n = average_pool_node(g, op, std::move(n)); break;
            case BuiltinOp::Mean: {
                std::vector<Node> two = mean_nodes(g, op, std::move(n));   // the pool, and without keep_dims the RESHAPE behind it
                if (two.size() == 2) emit(std::move(two[0]));
                n = std::move(two.back());
                break;
            }
            case BuiltinOp::L2Normalization: n = l2_normalization_node(g, op, std::move(n)); break;
            case BuiltinOp::Transpose: n = transpose_node(g, op, std::move(n)); break;
            case BuiltinOp::Relu:
                n.kind = Node::Act; n.in = {op.inputs.at(0)}; n.act = ACT_RELU;
                break;
            case BuiltinOp::Prelu:
                n.kind = Node::Act; n.in = {op.inputs.at(0)}; n.act = ACT_PRELU; n.alpha = op.inputs.at(1);
                need_const(g, n.alpha, "PRELU alpha");
                if (static_cast<int>(g.tensors[n.alpha].elems()) != g.tensors[n.in[0]].shape.back())
                    throw std::runtime_error("plan: PRELU alpha must be per-channel");
                break;
            case BuiltinOp::MaxPool2D:
                n.kind = Node::MaxPool; n.in = {op.inputs.at(0)};
                n.filter_h = op.filter_h; n.filter_w = op.filter_w; n.sh = op.stride_h; n.sw = op.stride_w;
                n.padding = op.padding; n.act = act_of(op.act);
                break;
            case BuiltinOp::Pad:
                n.kind = Node::Pad; n.in = {op.inputs.at(0)}; n.pads = op.inputs.at(1);
                need_const(g, n.pads, "PAD paddings");
                if (g.tensors[n.pads].i32.size() != 8) throw std::runtime_error("plan: PAD expects rank-4 paddings");
                break;
            case BuiltinOp::Reshape:
                n.kind = Node::Reshape; n.in = {op.inputs.at(0)};
                break;
            case BuiltinOp::Concatenation:
                n.kind = Node::Concat; n.in = op.inputs; n.axis = op.axis;
                if (op.act != FusedAct::None) throw std::runtime_error("plan: CONCATENATION with activation unsupported");
                break;
            case BuiltinOp::ResizeBilinear:
                n.kind = Node::Resize; n.in = {op.inputs.at(0)};
                n.half_pixel = op.half_pixel_centers; n.align_corners = op.align_corners;
                break;
            case BuiltinOp::DepthToSpace:
                n.kind = Node::DepthToSpace; n.in = {op.inputs.at(0)}; n.block_size = op.block_size;
                break;
            default:
                throw std::runtime_error("plan: builtin operator " + std::to_string(op.raw_code) + " unsupported");
        }
        emit(std::move(n));
    }
    return nodes;
}

}  // namespace plan_detail
}  // namespace mi
