// plan_internal.hpp — private declarations of the graph lowering: the passes build_plan (plan.cpp) runs, in its order, and the file each lives in.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "plan.hpp"

namespace mi {
namespace plan_detail {

inline bool is_graph_output(const Graph& g, int t) { return std::find(g.outputs.begin(), g.outputs.end(), t) != g.outputs.end(); }

// Who reads tensor t, as an input or as its skip: the one scan of the lowering.  Dead nodes never count; a caller names what else does not.
struct Readers {
    const std::vector<Node>& nodes;
    const std::vector<char>* absorbed = nullptr;   // nodes marked here do not count (output heads that run inside an earlier chain's launch)
    size_t from = 0;                               // nodes in front of this index do not count
    size_t skip_first = 1, skip_last = 0;          // nodes of this index range do not count (a group asking who reads a tensor from outside)

    template <class F>
    void each(int t, F f) const {   // f(node index, how often the node refers to t: both operands of an ADD, input and skip)
        for (size_t k = from; k < nodes.size(); k++) {
            const Node& n = nodes[k];
            if (n.dead || (absorbed && (*absorbed)[k]) || (k >= skip_first && k <= skip_last)) continue;
            const int refs = static_cast<int>(std::count(n.in.begin(), n.in.end(), t)) + (n.res == t ? 1 : 0);
            if (refs) f(static_cast<int>(k), refs);
        }
    }
    int count(int t) const {   // references
        int c = 0;
        each(t, [&](int, int refs) { c += refs; });
        return c;
    }
    std::vector<int> refs(int t) const {   // one entry per reference
        std::vector<int> r;
        each(t, [&](int k, int refs) { r.insert(r.end(), static_cast<size_t>(refs), k); });
        return r;
    }
    std::vector<int> readers(int t) const {   // one entry per node
        std::vector<int> r;
        each(t, [&](int k, int) { r.push_back(k); });
        return r;
    }
    bool any(int t) const { return count(t) != 0; }
};

// The kernels' *_supports checks are asked before storage exists: they get placeholder pointers, distinct and 16-byte aligned.  Whether the real
// views are aligned is checked on the finished plan (head_views_aligned, plan.cpp), which lowers the graph again without the heads when they are not.
constexpr uintptr_t kFakeIn = 0x1000, kFakeOut = 0x2000, kFakeAux = 0x3000 /* skip, weights, the front edge's input */,
                    kFakeEdgeOut = 0x4000 /* the back edge's output; an expand / contract run's pooled skip */, kFakeHeadW = 0x5000, kFakeHeadOutA = 0x6000,
                    kFakeHeadOutB = 0x7000;
template <class T>
T* fake(uintptr_t address) { return reinterpret_cast<T*>(address); }

// ---- the passes, in build_plan's order
// plan_ops.cpp: an untrusted graph's shapes and index lists; one Node per builtin operator (MEAN without keep_dims: two)
void check_untrusted_graph(const Graph& g);
std::vector<Node> nodes_of_graph(Graph& g);
// plan_widen.cpp: channel counts that are no multiple of 4 are widened with zero channels.  logical_*: the sizes of the graph as stored
void pad_odd_channels(Graph& g, std::vector<double>* logical_elems, std::vector<int>* logical_C);
// plan_rewrite.cpp: levels 1 and 2 (affines, FULLY_CONNECTED, spatial PADs, epilogues, BlazeBlocks); returns the live nodes
std::vector<Node> rewrite_nodes(Graph& g, std::vector<Node> nodes, int fuse_level);
// plan_chain.cpp: levels 3 and 4 (frame-resident and row-pipelined chains; with_edges: the stride-2 neighbours and output heads of level 5)
std::vector<Node> form_chains(const Graph& g, const std::vector<Node>& nodes, bool with_edges, int pipe_max, bool fuse_heads);
// plan_resident.cpp: level 5 (stage programs and the other frame-resident launches)
void reorder_branches(std::vector<Node>& ns);
std::vector<Node> group_resident(const Graph& g, const std::vector<Node>& ns, int budget, bool tail);
std::vector<std::vector<char>> dependence(const std::vector<Node>& ns);
bool is_fork(const std::vector<Node>& ns, const std::vector<std::vector<char>>& dep, size_t j);
// plan_layout.cpp: what the engine needs besides the nodes
void mark_gemm_heads(const Graph& g, std::vector<Node>& nodes, bool fuse_heads);
std::vector<int> number_tail_branches(const std::vector<Node>& nodes);
void resolve_views(Plan& plan);
void place_arena(Plan& plan);
void count_traffic(Plan& plan, const std::vector<double>& logical_elems, const std::vector<int>& logical_C);

}  // namespace plan_detail
}  // namespace mi
