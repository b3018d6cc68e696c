// Driver of tests/test_plan_pins.py: prints everything build_plan (plan.hpp: host code, no GPU) returns, with printing code of its own.
//   plan_dump shipped file.tflite ...   the rows {defaults (level 5, pipe 4, 156 KiB, tail on), fuse=0 .. fuse=4, tail=0, pipe=0, pipe=2, pipe=3, res=64k,
//                                       fuse=4+pipe=2} per file
//   plan_dump synth file.tflite ...     the rows {defaults, fuse=2, fuse=0} per file
//   plan_dump env file.tflite ...       the row `env` (the defaults; the caller sets the environment variable the row is about) per file
//   plan_dump --time file.tflite ...    per file one line: the name, then the microseconds of ten build_plan calls at the defaults (nothing else is printed)
// Per configuration a header line `== file row`, then
//   G              the graph as the lowering left it: counts, graph inputs and outputs
//   T id           a tensor: shape, is_const, dtype, FNV-1a of its f32 and of its i32 contents
//   O index        an operator: code, inputs, outputs, every option field
//   N path         a node, field by field (path: index in Plan::nodes, `.m<k>` a member, `.h<k>` a head node); scale / shift as bit patterns
//   S path.k       a stage of the node at `path`: member, src_t, dst_t, res_t, every ResStage field, every TailStage field
//   P path.k       a head pair
//   B / R / A      Plan::branch; storage (root, offset, frame_stride), root_offset and root_elems per tensor; the arena and the %a traffic / MAC figures
//   D              describe(), line by line
// or `threw: <message>` where the lowering refuses the graph.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>
#include "plan.hpp"

namespace {
using namespace mi;

uint64_t fnv(const void* p, size_t n) {
    uint64_t h = 14695981039346656037ull;
    for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
    return h;
}

std::string list(const std::vector<int>& v) {
    std::string s = "[";
    for (size_t k = 0; k < v.size(); k++) s += (k ? "," : "") + std::to_string(v[k]);
    return s + "]";
}

std::string bits(const std::vector<float>& v) {
    std::string s = "[";
    char buf[16];
    for (size_t k = 0; k < v.size(); k++) {
        uint32_t u;
        std::memcpy(&u, &v[k], 4);
        std::snprintf(buf, sizeof buf, "%s%08x", k ? "," : "", u);
        s += buf;
    }
    return s + "]";
}

std::string ref(const ResRef& r) { return "(" + std::to_string(r.base) + "," + std::to_string(r.pad_) + "," + std::to_string(r.root_off) + "," + std::to_string(r.inner) + "," + std::to_string(r.fs) + ")"; }

void print_graph(const Graph& g) {
    std::printf("G tensors=%zu ops=%zu inputs=%s outputs=%s\n", g.tensors.size(), g.ops.size(), list(g.inputs).c_str(), list(g.outputs).c_str());
    for (size_t t = 0; t < g.tensors.size(); t++) {
        const TensorInfo& ti = g.tensors[t];
        std::printf("T %zu %s const=%d dtype=%d f32=%zu:%016llx i32=%zu:%016llx\n", t, list(ti.shape).c_str(), ti.is_const ? 1 : 0, ti.dtype, ti.f32.size(),
                    static_cast<unsigned long long>(fnv(ti.f32.data(), ti.f32.size() * sizeof(float))), ti.i32.size(),
                    static_cast<unsigned long long>(fnv(ti.i32.data(), ti.i32.size() * sizeof(int32_t))));
    }
    for (size_t k = 0; k < g.ops.size(); k++) {
        const OpInfo& o = g.ops[k];
        std::printf("O %zu op=%d raw=%d in=%s out=%s padding=%d stride=%dx%d filter=%dx%d dm=%d axis=%d block=%d act=%d align=%d half=%d wf=%d knd=%d kd=%d\n", k, static_cast<int>(o.op),
                    o.raw_code, list(o.inputs).c_str(), list(o.outputs).c_str(), static_cast<int>(o.padding), o.stride_h, o.stride_w, o.filter_h, o.filter_w, o.depth_multiplier, o.axis,
                    o.block_size, static_cast<int>(o.act), o.align_corners ? 1 : 0, o.half_pixel_centers ? 1 : 0, o.weights_format, o.keep_num_dims ? 1 : 0, o.keep_dims ? 1 : 0);
    }
}

void print_node(const std::string& path, const Node& n) {
    std::printf("N %s kind=%d in=%s out=%d dead=%d w=%d b=%d k=%dx%d s=%dx%d padding=%d ept=%d epl=%d w2=%d b2=%d act=%d alpha=%d res=%d res_mode=%d res_after=%d pads=%d axis=%d "
                "filter=%dx%d block=%d half=%d align=%d",
                path.c_str(), static_cast<int>(n.kind), list(n.in).c_str(), n.out, n.dead ? 1 : 0, n.w, n.b, n.KH, n.KW, n.sh, n.sw, static_cast<int>(n.padding), n.ept, n.epl, n.w2, n.b2,
                n.act, n.alpha, n.res, n.res_mode, n.res_after ? 1 : 0, n.pads, n.axis, n.filter_h, n.filter_w, n.block_size, n.half_pixel ? 1 : 0, n.align_corners ? 1 : 0);
    std::printf(" res_const=%d+%d lds=%d bands=%d tail=%d/%d/%d dblock=%d xc=%d bneck=%d pre=%d post=%d gemm=%d fc=%d divide=%d perm=%s extra=%s ops=%s scale=%s shift=%s members=%zu heads=%zu\n",
                n.res_const_off, n.res_const_floats, n.res_lds_bytes, n.res_bands, n.tail ? 1 : 0, n.tail_frame_floats, n.tail_min_px, n.dblock ? 1 : 0, n.xc ? 1 : 0, n.bneck ? 1 : 0,
                n.chain_pre ? 1 : 0, n.chain_post ? 1 : 0, n.gemm_head ? 1 : 0, n.fc ? 1 : 0, n.divide ? 1 : 0, list(n.perm).c_str(), list(n.extra_out).c_str(), list(n.src_ops).c_str(),
                bits(n.scale).c_str(), bits(n.shift).c_str(), n.members.size(), n.head_nodes.size());
    for (size_t k = 0; k < n.stages.size(); k++) {
        const Node::Stage& sg = n.stages[k];
        const ResStage& s = sg.st;
        const TailStage& t = sg.tst;
        std::printf("S %s.%zu member=%d src_t=%d dst_t=%d res_t=%d", path.c_str(), k, sg.member, sg.src_t, sg.dst_t, sg.res_t);
        std::printf(" st{%d %d src %d %d %d %d %d %d %s k %d %d %d %d %d kv %d o %d %d %d dst %d %d %d z %d %s res %d %d %d %d %d %d %d %s act %d dw %d band %d %d %d kblk %d w %ld %ld}", s.kind,
                    s.dw_pg, s.src_off, s.src_H, s.src_W, s.src_C, s.src_PS, s.src_b, ref(s.src_g).c_str(), s.KH, s.KW, s.S, s.pt, s.pl, s.Kv, s.Ho, s.Wo, s.Co, s.dst_off, s.dst_PS, s.dst_b,
                    s.zero_dst, ref(s.dst_g).c_str(), s.res_mode, s.res_C, s.res_H, s.res_W, s.res_off, s.res_PS, s.res_b, ref(s.res_g).c_str(), s.act, s.dw_off, s.band_role, s.band_rows,
                    s.band_H, s.kblk, s.w_pw, s.cblob);
        std::printf(" tst{%d k %d %d %d %d src %d %d %d %d %s kv %d o %d %d %d dst %d %s res %d %d %d %d %s act %d scr %d pool %d m %u %u %u %u w %ld %ld}\n", t.kind, t.K, t.S, t.pt, t.pl,
                    t.src_off, t.src_H, t.src_W, t.src_C, ref(t.src_g).c_str(), t.Kv, t.Ho, t.Wo, t.Co, t.dst_off, ref(t.dst_g).c_str(), t.res_mode, t.res_C, t.res_W, t.res_off,
                    ref(t.res_g).c_str(), t.act, t.scr_off, t.pool_off, t.mHW, t.mW, t.mHWp, t.mWp, t.w_a, t.w_c);
    }
    for (size_t k = 0; k < n.head_pairs.size(); k++) std::printf("P %s.%zu src=%d a=%d b=%d\n", path.c_str(), k, n.head_pairs[k].src, n.head_pairs[k].a, n.head_pairs[k].b);
    for (size_t k = 0; k < n.members.size(); k++) print_node(path + ".m" + std::to_string(k), n.members[k]);
    for (size_t k = 0; k < n.head_nodes.size(); k++) print_node(path + ".h" + std::to_string(k), n.head_nodes[k]);
}

void print_plan(const Plan& p) {
    print_graph(p.graph);
    for (size_t i = 0; i < p.nodes.size(); i++) print_node(std::to_string(i), p.nodes[i]);
    std::printf("B fuse_level=%d nodes=%zu branch=%s\n", p.fuse_level, p.nodes.size(), list(p.branch).c_str());
    std::printf("R storage=%zu root_offset=%zu root_elems=%zu\n", p.storage.size(), p.root_offset.size(), p.root_elems.size());
    for (size_t t = 0; t < p.storage.size(); t++)
        std::printf("R %zu root=%d offset=%ld stride=%ld root_offset=%ld root_elems=%ld\n", t, p.storage[t].root, p.storage[t].offset, p.storage[t].frame_stride,
                    t < p.root_offset.size() ? p.root_offset[t] : -2L, t < p.root_elems.size() ? p.root_elems[t] : -2L);
    std::printf("A arena_floats_per_frame=%ld bytes_per_frame=%a macs_per_frame=%a\n", p.arena_floats_per_frame, p.bytes_per_frame, p.macs_per_frame);
    const std::string text = p.describe();
    for (size_t at = 0; at < text.size();) {
        const size_t nl = std::min(text.find('\n', at), text.size());
        std::printf("D %s\n", text.substr(at, nl - at).c_str());
        at = nl + 1;
    }
}

struct Row {
    const char* name;
    int fuse = 5, pipe = 4, budget = 156 * 1024;
    bool tail = true;
};

void run_config(const char* model, const std::vector<unsigned char>& blob, const Row& row) {
    std::printf("== %s %s\n", model, row.name);
    try {
        print_plan(build_plan(parse_tflite(blob.data(), blob.size()), row.fuse, row.pipe, row.budget, row.tail));
    } catch (const std::exception& e) {
        std::printf("threw: %s\n", e.what());
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode != "shipped" && mode != "synth" && mode != "env" && mode != "--time") return 2;
    const std::vector<Row> shipped = {{"defaults"},    {"fuse=0", 0},    {"fuse=1", 1},    {"fuse=2", 2},    {"fuse=3", 3},           {"fuse=4", 4},
                                      {"tail=0", 5, 4, 156 * 1024, false}, {"pipe=0", 5, 0}, {"pipe=2", 5, 2}, {"pipe=3", 5, 3}, {"res=64k", 5, 4, 64 * 1024}, {"fuse=4+pipe=2", 4, 2}};
    const std::vector<Row> synth = {{"defaults"}, {"fuse=2", 2}, {"fuse=0", 0}};
    for (int i = 2; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        const std::vector<unsigned char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const char* base = std::strrchr(argv[i], '/') ? std::strrchr(argv[i], '/') + 1 : argv[i];
        if (mode == "--time") {
            std::printf("%s", base);
            for (int r = 0; r < 10; r++) {
                Graph g = parse_tflite(b.data(), b.size());
                const auto t0 = std::chrono::steady_clock::now();
                const Plan p = build_plan(std::move(g), 5);
                const auto t1 = std::chrono::steady_clock::now();
                std::printf(" %.1f", std::chrono::duration<double, std::micro>(t1 - t0).count() + (p.nodes.empty() ? 1e9 : 0.0));
            }
            std::printf("\n");
        } else if (mode == "env") {
            run_config(base, b, Row{"env"});
        } else {
            for (const Row& r : mode == "shipped" ? shipped : synth) run_config(base, b, r);
        }
    }
    return 0;
}
