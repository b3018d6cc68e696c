// plan_layout.cpp — the tail of the lowering: batch-GEMM heads, tail branches, views, the activation arena, the plan's figures (see plan.hpp).
#include "plan_internal.hpp"

#include <stdexcept>

namespace mi {
namespace plan_detail {

// whole-frame convolutions (VALID, window = frame, one output pixel: the mesh and iris output heads) as batch GEMMs
void mark_gemm_heads(const Graph& g, std::vector<Node>& nodes, bool fuse_heads) {
    for (Node& n : nodes) {
        if (n.kind != Node::Conv || n.res >= 0 || n.in.size() != 1) continue;
        const auto& si = g.tensors[n.in[0]].shape;
        const auto& so = g.tensors[n.out].shape;
        if (si.size() != 4 || so.size() != 4 || si[1] != n.KH || si[2] != n.KW || so[1] != 1 || so[2] != 1) continue;
        if (n.padding != Padding::Valid && !(n.KH == 1 && n.KW == 1)) continue;
        if (si[1] * si[2] < 2) continue;  // 1x1 frames: pointwise, the stage programs / block kernels have them
        n.gemm_head = fuse_heads && head_gemm_supports(n.KH * n.KW * si[3], so[3]);
    }
}

// tail branches: behind the LAST fork of the plan the remaining launches fall into chains that do not need each other (the
// output heads of the iris / face mesh networks: 16 + 16 stage-program nodes).  branch[i] = chain of node i (0 = stays on the trunk
// stream, >= 1 = may run on a side stream), -1 for everything up to the fork.  A node that needs two different chains joins them: no
// branches then.
std::vector<int> number_tail_branches(const std::vector<Node>& nodes) {
    const std::vector<int> none(nodes.size(), -1);
    const std::vector<std::vector<char>> dep = dependence(nodes);
    if (dep.size() != nodes.size()) return none;
    auto is_view = [](const Node& n) { return n.kind == Node::Reshape || n.kind == Node::Concat; };
    int fork_at = -1;
    for (size_t j = 0; j < nodes.size(); j++)
        if (!is_view(nodes[j]) && is_fork(nodes, dep, j)) fork_at = static_cast<int>(j);
    if (fork_at < 0) return none;
    std::vector<int> br(nodes.size(), -1);
    int next = 0;
    for (size_t i = static_cast<size_t>(fork_at) + 1; i < nodes.size(); i++) {
        int mine = -1;
        for (size_t a = static_cast<size_t>(fork_at) + 1; a < i; a++)
            if (dep[i][a] && br[a] >= 0) {
                if (mine >= 0 && mine != br[a]) return none;
                mine = br[a];
            }
        if (is_view(nodes[i]) && mine < 0) continue;  // a view of a tensor from before the fork
        br[i] = mine >= 0 ? mine : next++;
    }
    return next >= 2 ? br : none;
}

// storage: RESHAPE = view of its input; CONCATENATION inputs live inside the joined buffer.
void resolve_views(Plan& plan) {
    const Graph& g = plan.graph;
    const int NT = static_cast<int>(g.tensors.size());
    plan.storage.resize(NT);
    for (int t = 0; t < NT; t++) plan.storage[t] = Storage{t, 0, static_cast<long>(g.tensors[t].elems())};
    for (int i = static_cast<int>(plan.nodes.size()) - 1; i >= 0; i--) {
        const Node& n = plan.nodes[i];
        if (n.kind == Node::Reshape) {
            plan.storage[n.in[0]] = plan.storage[n.out];
        } else if (n.kind == Node::Concat) {
            const auto& so = g.tensors[n.out].shape;
            int axis = n.axis < 0 ? n.axis + static_cast<int>(so.size()) : n.axis;
            // (a crafted graph's axis may lie outside the output's shape: so[d] below must not be read beyond it — found by the mutation test
            // under AddressSanitizer, a read of four bytes behind the shape vector)
            if (axis < 1 || axis >= static_cast<int>(so.size())) throw std::runtime_error("plan: CONCATENATION axis outside the output's shape");
            long outer = 1;
            for (int d = 1; d < axis; d++) outer *= so[d];
            if (outer != 1) throw std::runtime_error("plan: CONCATENATION must join the first non-batch axis");
            long off = 0;
            for (int t : n.in) {
                if (plan.storage[t].root != t) throw std::runtime_error("plan: tensor feeds two concatenations/views");
                plan.storage[t] = Storage{plan.storage[n.out].root, plan.storage[n.out].offset + off, plan.storage[n.out].frame_stride};
                off += static_cast<long>(g.tensors[t].elems());
            }
        }
    }
    // views created above must be propagated forward to tensors whose storage pointed at an intermediate root
    for (int pass = 0; pass < 4; pass++)
        for (int t = 0; t < NT; t++) {
            Storage& s = plan.storage[t];
            const Storage& r = plan.storage[s.root];
            if (r.root != s.root) s = Storage{r.root, r.offset + s.offset, r.frame_stride};
        }
}

// liveness + first-fit arena (offsets in floats per frame; scaled by the chunk size at run time)
void place_arena(Plan& plan) {
    const Graph& g = plan.graph;
    const int NT = static_cast<int>(g.tensors.size()), NN = static_cast<int>(plan.nodes.size());
    std::vector<int> first(NT, -2), last(NT, -2);
    auto touch = [&](int t, int step) {
        if (t < 0 || g.tensors[t].is_const) return;
        int r = plan.storage[t].root;
        if (first[r] == -2 || step < first[r]) first[r] = step;
        if (step > last[r]) last[r] = step;
    };
    auto touch_all = [&](const Node& n, int step) {   // everything the node reads or writes
        for (int t : n.in) touch(t, step);
        touch(n.res, step);
        touch(n.out, step);
        for (int t : n.extra_out) touch(t, step);
    };
    touch(g.inputs[0], -1);
    for (int i = 0; i < NN; i++) touch_all(plan.nodes[i], i);
    for (int t : g.outputs) touch(t, NN);
    // two plain BlazeBlocks of one shape in a row may run as ONE launch (engine.cpp: mdblock_kernel, pair form) that reads the first one's input while it
    // writes the second one's output: that input stays allocated one node longer
    for (int i = 0; i + 1 < NN; i++) {
        const Node &pa = plan.nodes[i], &pb = plan.nodes[i + 1];
        if (pa.kind != Node::Block || pb.kind != Node::Block || pa.w < 0 || pb.w < 0 || pa.in.size() != 1 || pb.in.size() != 1 || pb.in[0] != pa.out) continue;
        if (pa.sh != 1 || pb.sh != 1 || g.tensors[pa.in[0]].shape != g.tensors[pb.out].shape) continue;
        touch(pa.in[0], i + 1);
    }
    // tail branches may run side by side in any interleaving: everything they read or write stays allocated to the end of the plan
    for (int i = 0; i < NN; i++)
        if (plan.branch[static_cast<size_t>(i)] >= 0) touch_all(plan.nodes[i], NN);
    plan.root_offset.assign(NT, -1);
    plan.root_elems.assign(NT, 0);
    struct Live { long off, size; int until; };
    std::vector<Live> live;
    std::vector<int> order;
    for (int t = 0; t < NT; t++)
        if (first[t] != -2 && plan.storage[t].root == t && !g.tensors[t].is_const) order.push_back(t);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return first[a] < first[b]; });
    long high = 0;
    for (int t : order) {
        long size = (plan.storage[t].frame_stride + 63) & ~63L;  // 256-byte granules
        // buffers whose last reader is an earlier step than this tensor's first writer can be recycled
        live.erase(std::remove_if(live.begin(), live.end(), [&](const Live& l) { return l.until < first[t]; }), live.end());
        std::sort(live.begin(), live.end(), [](const Live& a, const Live& b) { return a.off < b.off; });
        long off = 0;
        for (const Live& l : live) {
            if (off + size <= l.off) break;
            off = std::max(off, l.off + l.size);
        }
        plan.root_offset[t] = off;
        plan.root_elems[t] = size;
        live.push_back({off, size, last[t]});
        high = std::max(high, off + size);
    }
    plan.arena_floats_per_frame = high;
}

// algorithmic traffic / MACs of the plan as launched (per frame); sizes are those of the graph as stored, whatever padding the lowering added
void count_traffic(Plan& plan, const std::vector<double>& logical_elems, const std::vector<int>& logical_C) {
    const Graph& g = plan.graph;
    auto elems = [&](int t) { return t < 0 ? 0.0 : (static_cast<size_t>(t) < logical_elems.size() ? logical_elems[t] : static_cast<double>(g.tensors[t].elems())); };
    auto LC = [&](int t) { return static_cast<size_t>(t) < logical_C.size() ? logical_C[t] : g.tensors[t].shape.back(); };
    double bytes = 0, macs = 0;
    for (const Node& n : plan.nodes) {
        if (n.kind == Node::Reshape || n.kind == Node::Concat) continue;
        for (int t : n.in) bytes += 4 * elems(t);
        bytes += 4 * elems(n.out);
        for (int t : n.extra_out) bytes += 4 * elems(t);
        if (n.kind == Node::Resident) {
            for (const Node& m : n.members) {
                for (int c : {m.w, m.b, m.w2, m.b2, m.alpha}) bytes += 4 * elems(c);
                const auto& so2 = g.tensors[m.out].shape;
                const int Cm = LC(m.in[0]);
                if (m.kind == Node::Conv) macs += elems(m.out) * m.KH * m.KW * Cm;
                else macs += static_cast<double>(so2[1]) * so2[2] * Cm * ((m.w >= 0 ? 9 : 0) + LC(m.out));
            }
            continue;
        }
        if (n.kind == Node::Chain) {
            for (const Node& m : n.members) {
                for (int c : {m.w, m.b, m.w2, m.b2, m.alpha}) bytes += 4 * elems(c);
                const auto& so2 = g.tensors[m.out].shape;
                macs += static_cast<double>(so2[1]) * so2[2] * LC(m.in[0]) * (9 + LC(m.out));
            }
            for (const Node& m : n.head_nodes) {
                for (int c : {m.w, m.b, m.w2, m.b2}) bytes += 4 * elems(c);
                macs += elems(m.out) * LC(m.in[0]);
            }
            continue;
        }
        if (n.res >= 0 && !(n.kind == Node::Block && n.res == n.in[0])) bytes += 4 * elems(n.res);
        for (int c : {n.w, n.b, n.w2, n.b2, n.alpha}) bytes += 4 * elems(c);
        const auto& so = g.tensors[n.out].shape;
        if (n.kind == Node::Conv) macs += elems(n.out) * n.KH * n.KW * LC(n.in[0]);
        if (n.kind == Node::Dw) macs += elems(n.out) * n.KH * n.KW;
        if (n.kind == Node::Block) {
            int C = LC(n.in[0]);
            macs += static_cast<double>(so[1]) * so[2] * C * ((n.w >= 0 ? n.KH * n.KW : 0) + LC(n.out));
        }
    }
    plan.bytes_per_frame = bytes;
    plan.macs_per_frame = macs;
}

}  // namespace plan_detail
}  // namespace mi
