// plan.cpp — build_plan: the lowering as a list of passes (plan_internal.hpp names each with its file), and Plan::describe (see plan.hpp).
#include "plan.hpp"
#include "layout.hpp"
#include "plan_internal.hpp"

#include <sstream>

namespace mi {
namespace {
using namespace plan_detail;

Plan build_plan_impl(Graph graph, int fuse_level, int pipe_max, int res_budget_bytes, bool fuse_heads, bool tail) {
    Plan plan;
    plan.graph = std::move(graph);
    plan.fuse_level = fuse_level;
    Graph& g = plan.graph;
    check_untrusted_graph(g);
    // ONNX-exported graphs: channel-first element-wise operators move onto NHWC tensors and the transposes around the convolutions go (layout.hpp);
    // a graph without TRANSPOSE (0,3,1,2) passes through untouched
    layout_detail::normalise_layout(g);
    // algorithmic sizes (traffic / MAC figures of the plan) are those of the graph as stored, whatever padding the lowering adds
    std::vector<double> logical_elems;
    std::vector<int> logical_C;
    if (fuse_level >= 2) pad_odd_channels(g, &logical_elems, &logical_C);  // (the op-by-op levels take any channel count)
    plan.nodes = rewrite_nodes(g, nodes_of_graph(g), fuse_level);
    if (fuse_level >= 3) plan.nodes = form_chains(g, plan.nodes, fuse_level >= 5, fuse_level >= 4 ? pipe_max : 0, fuse_heads);
    if (fuse_level >= 2) mark_gemm_heads(g, plan.nodes, fuse_heads);
    if (fuse_level >= 5) {
        reorder_branches(plan.nodes);
        plan.nodes = group_resident(g, plan.nodes, res_budget_bytes, tail);
    }
    plan.branch = fuse_level >= 5 ? number_tail_branches(plan.nodes) : std::vector<int>(plan.nodes.size(), -1);
    resolve_views(plan);
    place_arena(plan);
    count_traffic(plan, logical_elems, logical_C);
    return plan;
}

// The chain's output heads and the batch-GEMM heads are chosen before storage exists (placeholder pointers, 16-byte aligned); the
// kernels need the real views 16-byte aligned with frame strides that are multiples of 4 floats.  A head whose slice of a
// concatenated output starts at an odd offset (e.g. 15 x 15 anchors) fails that: such a graph is lowered again without them.
bool head_views_aligned(const Plan& plan) {
    auto aligned = [&](int t) {
        if (t < 0) return true;
        const Storage& s = plan.storage[t];
        return (s.offset & 3) == 0 && (s.frame_stride & 3) == 0;
    };
    for (const Node& n : plan.nodes) {
        // chain heads: the head with Co % 4 == 0 of a pair is stored as float4 (chain_kernel_supports: out_a, out_a_fs); its partner
        // (the classifier, 2 / 6 channels) is stored float by float and may start anywhere
        if (n.kind == Node::Chain)
            for (const Node::HeadPair& hp : n.head_pairs)
                if (!aligned(n.head_nodes[static_cast<size_t>(hp.a)].out)) return false;
        // batch GEMM heads read their input as float4 (launch_head_gemm: in, in_fs); the output is stored float by float (the face
        // flag is one float per frame)
        if (n.kind == Node::Conv && n.gemm_head && !aligned(n.in[0])) return false;
    }
    return true;
}
}  // namespace

Plan build_plan(Graph graph, int fuse_level, int pipe_max_opt, int res_budget_bytes, bool tail) {
    Plan plan = build_plan_impl(graph, fuse_level, pipe_max_opt, res_budget_bytes, true, tail);
    if (head_views_aligned(plan)) return plan;
    return build_plan_impl(std::move(graph), fuse_level, pipe_max_opt, res_budget_bytes, false, tail);
}

std::string Plan::describe() const {
    static const char* kinds[] = {"conv", "dw", "block", "add", "act", "maxpool", "pad", "reshape", "concat", "resize", "d2s", "chain", "resident", "affine", "pool", "l2norm", "transpose"};
    static const char* acts[] = {"", "+relu", "+relu6", "+prelu"};
    static const char* res[] = {"", "+skip", "+skip(maxpool)", "+skip(up2x)"};
    std::ostringstream os;
    os << "# fuse_level=" << fuse_level << " launches=" << nodes.size() << " arena_floats_per_frame=" << arena_floats_per_frame
       << " bytes_per_frame=" << static_cast<long long>(bytes_per_frame) << " macs_per_frame=" << static_cast<long long>(macs_per_frame) << "\n";
    for (const Node& n : nodes) {
        const auto& si = graph.tensors[n.in[0]].shape;
        const auto& so = graph.tensors[n.out].shape;
        os << kinds[n.kind] << acts[n.act] << res[n.res_mode] << " t" << n.in[0] << "[";
        for (size_t d = 1; d < si.size(); d++) os << (d > 1 ? "x" : "") << si[d];
        os << "] -> t" << n.out << "[";
        for (size_t d = 1; d < so.size(); d++) os << (d > 1 ? "x" : "") << so[d];
        os << "]";
        if (n.kind == Node::Conv || n.kind == Node::Dw || (n.kind == Node::Block && n.w >= 0)) os << " k" << n.KH << "x" << n.KW << " s" << n.sh;
        if (n.kind == Node::Pool) os << " k" << n.filter_h << "x" << n.filter_w << " s" << n.sh << (n.padding == Padding::Same ? " same" : " valid");
        if (n.kind == Node::Affine && n.divide) os << " divisor form";
        if (n.kind == Node::Transpose) os << " perm " << n.perm[0] << n.perm[1] << n.perm[2] << n.perm[3];
        if (n.kind == Node::Conv && n.gemm_head) os << " whole-frame window: GEMM over the batch";
        if (n.ept >= 0) os << " pad" << n.ept << "/" << n.epl;
        if (n.kind == Node::Block && n.w < 0) os << " pointwise";
        if (n.kind == Node::Chain)
            if (n.chain_pre || n.chain_post)
                os << " x" << n.members.size() << " blocks, frame resident in LDS" << (n.chain_pre ? ", stride-2 block in front" : "") << (n.chain_post ? ", stride-2 block behind" : "")
                   << (n.head_nodes.empty() ? "" : ", " + std::to_string(n.head_nodes.size()) + " output heads");
            else
                os << " x" << n.members.size() << " blocks, " << (si[1] * si[2] <= 256 ? "frame resident in LDS" : "row-pipelined through LDS")
                   << (n.members.back().sh == 2 ? " (stride-2 tail)" : "") << (n.head_nodes.empty() ? "" : ", " + std::to_string(n.head_nodes.size()) + " output heads");
        if (n.kind == Node::Resident && n.dblock) {
            os << (n.members[0].res >= 0 ? " two BlazeBlocks (" : " double block (") << graph.tensors[n.members[0].in[0]].shape[3] << " -> " << graph.tensors[n.members[0].out].shape[3] << " -> " << graph.tensors[n.members[1].out].shape[3]
               << " channels), walking row bands, narrow tensor in LDS";
        } else if (n.kind == Node::Resident && n.xc) {
            os << " x" << n.members.size() / 2 << " expand / contract pairs (" << graph.tensors[n.members[0].in[0]].shape[3] << " <-> " << graph.tensors[n.members[0].out].shape[3]
               << " channels), frame resident, depthwise stages on the fly";
        } else if (n.kind == Node::Resident && n.bneck) {
            os << " x" << n.members.size() / 2 << " bottleneck blocks, wide tensor in registers, " << (n.res_bands > 1 ? std::to_string(n.res_bands) + " row bands" : std::string("frame resident"));
        } else if (n.kind == Node::Resident && n.tail) {
            os << " x" << n.members.size() << " nodes in " << n.stages.size() << " stages, several frames per workgroup, " << n.tail_frame_floats * 4 << " B LDS per frame";
            for (int t : n.extra_out) os << " +t" << t;
        } else if (n.kind == Node::Resident) {
            os << " x" << n.members.size() << " nodes in " << n.stages.size() << " stages, " << (n.res_bands > 1 ? "row-band resident" : "frame resident") << ", " << n.res_lds_bytes << " B LDS";
            if (n.res_bands > 1) os << ", " << n.res_bands << " bands of " << n.stages[0].st.band_rows << " rows";
            for (int t : n.extra_out) os << " +t" << t;
        }
        if (n.kind == Node::Chain)
            for (int t : n.extra_out) os << " +t" << t;
        os << " ops{";
        for (size_t k = 0; k < n.src_ops.size(); k++) os << (k ? "," : "") << n.src_ops[k];
        os << "}\n";
    }
    return os.str();
}

}  // namespace mi
