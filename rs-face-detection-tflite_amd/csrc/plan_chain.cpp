// plan_chain.cpp — levels 3 and 4 of the lowering: runs of same-shape stride-1 BlazeBlocks become chains (see plan.hpp).
#include "plan_internal.hpp"

namespace mi {
namespace plan_detail {
namespace {

struct ChainPass {
    const Graph& g;
    const std::vector<Node>& nodes;   // the plan in front of this pass
    const bool fuse_heads;
    std::vector<char> absorbed;       // per node: an output head that runs inside an earlier chain's launch

    ChainPass(const Graph& graph, const std::vector<Node>& ns, bool heads) : g(graph), nodes(ns), fuse_heads(heads), absorbed(ns.size(), 0) {}

    int uses(int t) const { return Readers{nodes}.count(t); }
    bool is_output(int t) const { return is_graph_output(g, t); }

    // a block that can sit inside a chain: stride 1, same shape in and out, skip = its own input (or none)
    bool chainable(const Node& n) const {
        if (n.kind != Node::Block || n.w < 0 || n.sh != 1 || n.sw != 1 || n.padding != Padding::Same) return false;
        const auto& si = g.tensors[n.in[0]].shape;
        const auto& so = g.tensors[n.out].shape;
        if (si.size() != 4 || si != so) return false;
        if (n.res >= 0 && !(n.res == n.in[0] && n.res_mode == RES_DIRECT && !n.res_after)) return false;
        return true;
    }
    bool links(size_t j) const {  // node j+1 continues the chain that node j is in
        return j + 1 < nodes.size() && chainable(nodes[j + 1]) && nodes[j + 1].in[0] == nodes[j].out &&
               g.tensors[nodes[j + 1].in[0]].shape == g.tensors[nodes[j].in[0]].shape &&
               (nodes[j + 1].act == ACT_RELU) == (nodes[j].act == ACT_RELU) &&
               uses(nodes[j].out) == (nodes[j + 1].res >= 0 ? 2 : 1) && !is_output(nodes[j].out);
    }
    Node make_chain(size_t i, size_t j) const {
        Node c;
        c.kind = Node::Chain;
        c.in = {nodes[i].in[0]};
        c.out = nodes[j].out;
        for (size_t k = i; k <= j; k++) {
            c.members.push_back(nodes[k]);
            c.src_ops.insert(c.src_ops.end(), nodes[k].src_ops.begin(), nodes[k].src_ops.end());
        }
        return c;
    }
    // The stride-2 BlazeBlocks on either side of a frame-resident chain join its launch (chain_kernels.hip, ChainEdge): the
    // one in front (DW3x3 s2 -> PW -> + 2x2 max-pool skip -> act; the producer of the chain's input, read by nobody else) gathers
    // its taps from global memory and leaves its output in the LDS tile; the one behind reads the tile and writes global memory.
    static bool edge_block(const Node& e) {
        return e.kind == Node::Block && !e.res_after && e.w >= 0 && e.KH == 3 && e.KW == 3 && e.sh == 2 && e.sw == 2 && e.padding == Padding::Same &&
               (e.res < 0 || (e.res == e.in[0] && e.res_mode == RES_MAXPOOL));
    }
    // t only reaches graph outputs through views (RESHAPE / CONCATENATION).  (Not Readers' rule alone: every tensor on the way must have exactly
    // one reader, and that reader must be a view.)
    bool view_only(int t) const {
        for (int depth = 0; depth < 4; depth++) {
            if (is_output(t)) return true;
            const std::vector<int> rd = Readers{nodes}.readers(t);
            if (rd.size() != 1) return false;
            const Node& m = nodes[static_cast<size_t>(rd[0])];
            if (m.kind != Node::Reshape && m.kind != Node::Concat) return false;
            t = m.out;
        }
        return false;
    }
    // 1x1 convolutions without activation or skip whose result only reaches graph outputs through views: the SSD heads.  Those that read
    // tensor t, at plan positions >= from.
    std::vector<size_t> heads_on(int t, size_t from) const {
        std::vector<size_t> hs;
        for (size_t k = from; k < nodes.size(); k++) {
            const Node& m = nodes[k];
            if (absorbed[k] || m.in.size() != 1 || m.in[0] != t || m.res >= 0 || m.act != ACT_NONE) continue;
            const bool pw = (m.kind == Node::Conv && m.KH == 1 && m.KW == 1 && m.sh == 1 && m.sw == 1 && !m.gemm_head) || (m.kind == Node::Block && m.w < 0);
            if (pw && view_only(m.out)) hs.push_back(k);
        }
        return hs;
    }

    // tin / tout: the resident frame's first and last tensor (c.in / c.out change as edges join); ca: the launch as the kernel's check sees it so far;
    // done: the nodes emitted in front of the chain; next: index in `nodes` of the node after the chain (advanced past an absorbed block)
    void attach_pre(Node& c, int tin, std::vector<Node>& done, ChainArgs& ca) const {
        if (done.empty()) return;
        const auto& sc = g.tensors[tin].shape;  // H x W x C of the resident frame
        const Node& e = done.back();
        const auto& se = g.tensors[e.in.empty() ? tin : e.in[0]].shape;
        const int users = c.members.front().res == tin ? 2 : 1;
        if (!(edge_block(e) && e.out == tin && uses(tin) == users && !is_output(tin) && se.size() == 4 && se[1] == 2 * sc[1] && se[2] == 2 * sc[2] &&
              se[3] % 8 == 0 && se[3] <= sc[3]))
            return;
        ca.pre.on = 1; ca.pre.Cin = se[3]; ca.pre.in = fake<const float>(kFakeAux); ca.pre.in_fs = static_cast<long>(g.tensors[e.in[0]].elems());
        if (!chain_kernel_supports(ca)) {
            ca.pre.on = 0;
            return;
        }
        c.members.insert(c.members.begin(), e);
        c.src_ops.insert(c.src_ops.begin(), e.src_ops.begin(), e.src_ops.end());
        c.in = {e.in[0]};
        c.chain_pre = true;
        done.pop_back();
    }
    void attach_post(Node& c, int tin, int tout, size_t& next, ChainArgs& ca) const {
        if (next >= nodes.size()) return;
        const auto& sc = g.tensors[tin].shape;
        const Node& e = nodes[next];
        const auto& so = g.tensors[e.out].shape;
        if (!(edge_block(e) && e.in[0] == tout && so.size() == 4 && sc[1] % 2 == 0 && sc[2] % 2 == 0 && so[1] * 2 == sc[1] && so[2] * 2 == sc[2])) return;
        ca.post.on = 1; ca.post.Co = so[3]; ca.post.out = fake<float>(kFakeEdgeOut); ca.post.out_fs = static_cast<long>(g.tensors[e.out].elems());
        if (!chain_kernel_supports(ca)) return;
        const bool others = uses(tout) > (e.res == tout ? 2 : 1) || is_output(tout);
        c.members.push_back(e);
        c.src_ops.insert(c.src_ops.end(), e.src_ops.begin(), e.src_ops.end());
        c.chain_post = true;
        if (others) c.extra_out = {e.out};   // the chain's own output is still read (output heads): both are written
        else c.out = e.out;
        next++;
    }
    // output heads on the chain's final frame (src 0) and on the block behind it (src 1)
    void attach_heads(Node& c, int tout, size_t next, ChainArgs& ca) {
        const int t_post = c.chain_post ? c.members.back().out : -1;
        for (int src = 0; src < 2; src++) {
            const int t = src == 0 ? tout : t_post;
            if (t < 0) continue;
            std::vector<size_t> hs = heads_on(t, next);
            if (!fuse_heads || hs.empty() || hs.size() > 2) continue;
            // a = the head whose channel count is a multiple of 4 (the regressors), b = the other one
            auto co = [&](size_t k) { return g.tensors[nodes[k].out].shape.back(); };
            size_t ka = hs[0], kb = hs.size() > 1 ? hs[1] : static_cast<size_t>(-1);
            if (hs.size() > 1 && (co(ka) % 4 != 0 || (co(kb) % 4 == 0 && co(kb) > co(ka)))) std::swap(ka, kb);
            if (co(ka) % 4 != 0) continue;
            ChainArgs cb = ca;
            ChainHead& H = cb.heads[src];
            H.on = 1; H.src = src; H.Co_a = co(ka); H.Co_b = kb != static_cast<size_t>(-1) ? co(kb) : 0;
            H.w_pw = fake<const float>(kFakeHeadW); H.out_a = fake<float>(kFakeHeadOutA); H.out_b = H.Co_b ? fake<float>(kFakeHeadOutB) : nullptr;
            H.out_a_fs = H.out_b_fs = 64;
            if (!chain_kernel_supports(cb)) continue;
            ca = cb;
            Node::HeadPair hp;
            hp.src = src;
            hp.a = static_cast<int>(c.head_nodes.size());
            c.head_nodes.push_back(nodes[ka]);
            if (H.Co_b) { hp.b = static_cast<int>(c.head_nodes.size()); c.head_nodes.push_back(nodes[kb]); }
            c.head_pairs.push_back(hp);
            for (size_t k : {ka, kb}) {
                if (k == static_cast<size_t>(-1)) continue;
                absorbed[k] = 1;
                c.extra_out.push_back(nodes[k].out);
                c.src_ops.insert(c.src_ops.end(), nodes[k].src_ops.begin(), nodes[k].src_ops.end());
            }
        }
    }
    // the chain's final frame needs no memory when every reader runs inside this launch
    void drop_unread_frame(Node& c, int tout, size_t next) const {
        if (!(c.chain_post && c.out == tout && !is_output(tout))) return;
        Readers later{nodes, &absorbed, next};   // the absorbed heads and everything in front of `next` run inside the launch
        if (later.any(tout)) return;
        const int t_post = c.members.back().out;
        c.out = t_post;
        c.extra_out.erase(std::find(c.extra_out.begin(), c.extra_out.end(), t_post));
    }

    // (a) the whole frame fits in LDS: frame-resident chain kernel.  Takes up to kMaxChain of the `run` blocks from i on (false: no chain here)
    bool resident_chain(size_t& i, int run, bool with_edges, std::vector<Node>& done) {
        const auto& si = g.tensors[nodes[i].in[0]].shape;
        ChainArgs ca;
        ca.in = fake<const float>(kFakeIn); ca.out = fake<float>(kFakeOut);
        ca.in_fs = ca.out_fs = static_cast<long>(g.tensors[nodes[i].in[0]].elems());
        ca.B = 1; ca.H = si[1]; ca.W = si[2]; ca.C = si[3];
        ca.nblocks = std::min(run, kMaxChain);
        if (!(si[1] * si[2] <= 256 && si[3] % 8 == 0 && chain_kernel_supports(ca))) return false;
        Node c = make_chain(i, i + ca.nblocks - 1);
        i += ca.nblocks;
        if (with_edges) {
            const int tin = c.in[0], tout = c.out;
            attach_pre(c, tin, done, ca);
            attach_post(c, tin, tout, i, ca);
            attach_heads(c, tout, i, ca);
            drop_unread_frame(c, tout, i);
        }
        done.push_back(std::move(c));
        return true;
    }
    // (b) narrow layers: row-pipelined groups of up to 4 blocks, the intermediate rows handed over in LDS; the
    // stride-2 block that follows the run [i, j] (max-pool skip from its own input) can be the last stage of the last group
    bool pipelined_chains(size_t& i, size_t j, int pipe_max, std::vector<Node>& done) const {
        const auto& si = g.tensors[nodes[i].in[0]].shape;
        if (pipe_max < 2 || !strip_pipe_shape_ok(si[3], si[2])) return false;
        bool s2_tail = false;
        if (j + 1 < nodes.size()) {
            const Node& t = nodes[j + 1];
            s2_tail = t.kind == Node::Block && t.w >= 0 && t.sh == 2 && t.sw == 2 && t.padding == Padding::Same && t.in[0] == nodes[j].out &&
                      t.res == t.in[0] && t.res_mode == RES_MAXPOOL && t.act == ACT_RELU && nodes[i].act == ACT_RELU &&
                      uses(nodes[j].out) == 2 && !is_output(nodes[j].out) && strip_tail_shape_ok(si[3], g.tensors[t.out].shape[3], si[1], si[2]);
        }
        int left = static_cast<int>(j - i + 1) + (s2_tail ? 1 : 0);
        if (left < 2) return false;
        while (left >= 2) {
            int take = std::min(left, std::min(pipe_max, 4));
            if (left - take == 1 && take > 2) take--;  // never leave a single block behind a full group
            done.push_back(make_chain(i, i + take - 1));
            i += take;
            left -= take;
        }
        return true;  // a leftover single block is handled by the next iteration as a plain node
    }

    std::vector<Node> run(bool with_edges, int pipe_max) {
        std::vector<Node> done;
        for (size_t i = 0; i < nodes.size();) {
            if (absorbed[i]) { i++; continue; }  // an output head that runs inside an earlier chain's launch
            if (chainable(nodes[i])) {
                size_t j = i;
                while (links(j)) j++;
                const int run_len = static_cast<int>(j - i + 1);
                if (run_len >= 2 && resident_chain(i, run_len, with_edges, done)) continue;
                if (pipelined_chains(i, j, pipe_max, done)) continue;
            }
            done.push_back(nodes[i]);
            i++;
        }
        return done;
    }
};

}  // namespace

std::vector<Node> form_chains(const Graph& g, const std::vector<Node>& nodes, bool with_edges, int pipe_max, bool fuse_heads) {
    return ChainPass(g, nodes, fuse_heads).run(with_edges, pipe_max);
}

}  // namespace plan_detail
}  // namespace mi
