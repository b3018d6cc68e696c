// Driver of tests/test_launch_pins.py: `launches_dump shipped|synth file.tflite ...` lowers every model file the way the engine does (pipe 4,
// 156 KiB, tail on; constants packed), and prints the launch list lower_chunk (launches.cpp: host code, no GPU) makes of one chunk, for 256
// compute units and an arena laid out for exactly the chunk's frames (chunk_cap = F), under these configurations:
//   shipped: the option rows {defaults, strip=0, pair_fuse=0, stem_fuse=0, mchain=0, small_chain=0, stem_mfma=0, fork=0, heads=4, lanes=2,
//            fuse=2} at F in {1, 4, 5, 16, 17, 31, 32}; band=2 at F in {1, 4}; the u8 input form (where the graph has one) at F in {1, 32}
//   synth:   defaults and fuse=2 at F in {1, 32}
//   tensors: defaults at F in {1, 3, 32, 33}, in a form of its own (below): per launch `k "label" in=[tensors] out=[tensors]`
// Per configuration a header line `== model row F=n`, then one line per launch: launcher tag, label, the plan nodes it stands for (first-last
// and how many), stream slot, wait node, record flag, and a 64-bit FNV-1a hash of the argument struct taken field by field (pointers as the
// numbers they are).  The device addresses are fake, 256-byte aligned and 2^40 bytes apart (graph outputs 2^36); nothing dereferences them:
//   weights 0x010000000000  arena 0x020000000000  input 0x030000000000  output k 0x040000000000 + k * 0x001000000000
//   small-batch scratch 0x050000000000  stage programs 0x060000000000  tail programs 0x070000000000
//   band program 0x080000000000, constants 0x090000000000, workspace 0x0a0000000000, sync 0x0b0000000000, fail 0x0c0000000000
//   u8 frames 0x0d0000000000, u8 table 0x0e0000000000
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>
#include "launches.hpp"

namespace {
using namespace mi;

struct Fnv {
    uint64_t h = 14695981039346656037ull;
    void bytes(const void* p, size_t n) {
        for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
    }
    void operator()(int v) { bytes(&v, sizeof v); }
    void operator()(unsigned v) { bytes(&v, sizeof v); }
    void operator()(long v) { bytes(&v, sizeof v); }
    void operator()(float v) { bytes(&v, sizeof v); }
    void operator()(const void* p) { const uint64_t v = reinterpret_cast<uintptr_t>(p); bytes(&v, sizeof v); }

    void operator()(const Epilogue& e) {
        Fnv& f = *this;
        f(e.bias); f(e.alpha); f(e.res); f(e.res_fs); f(e.res_mode); f(e.res_C); f(e.res_W); f(e.res_H); f(e.act); f(e.res_after);
    }
    void operator()(const ConvArgs& a) {
        Fnv& f = *this;
        f(a.in); f(a.in_u8); f(a.u8_lut); f(a.u8_frame_bytes); f(a.u8_row_bytes); f(a.w); f(a.out); f(a.in_fs); f(a.out_fs);
        f(a.B); f(a.H); f(a.W); f(a.C); f(a.Ho); f(a.Wo); f(a.Co); f(a.Cop); f(a.KH); f(a.KW); f(a.sh); f(a.sw); f(a.pt); f(a.pl); f(a.ep); f(a.no_mfma);
    }
    void operator()(const HeadGemmArgs& a) {
        Fnv& f = *this;
        f(a.in); f(a.w); f(a.bias); f(a.alpha); f(a.out); f(a.in_fs); f(a.out_fs); f(a.B); f(a.K); f(a.N); f(a.act);
    }
    void operator()(const DwArgs& a) {
        Fnv& f = *this;
        f(a.in); f(a.w); f(a.out); f(a.in_fs); f(a.out_fs); f(a.B); f(a.H); f(a.W); f(a.C); f(a.Ho); f(a.Wo);
        f(a.KH); f(a.KW); f(a.sh); f(a.sw); f(a.pt); f(a.pl); f(a.ep);
    }
    void operator()(const BlockArgs& a) {
        Fnv& f = *this;
        f(a.in); f(a.w_dw); f(a.b_dw); f(a.w_pw); f(a.w_strip); f(a.w_mwalk); f(a.out); f(a.in_fs); f(a.out_fs);
        f(a.B); f(a.H); f(a.W); f(a.C); f(a.Ho); f(a.Wo); f(a.Co); f(a.sh); f(a.sw); f(a.pt); f(a.pl); f(a.has_dw); f(a.pipe_rows); f(a.pipe_band); f(a.ep);
    }
    void operator()(const ChainBlock& b) {
        Fnv& f = *this;
        f(b.w_dw); f(b.b_dw); f(b.w_pw); f(b.bias); f(b.alpha); f(b.act); f(b.has_res);
    }
    void operator()(const ChainEdge& e) {
        Fnv& f = *this;
        f(e.on); f(e.blk); f(e.in); f(e.in_fs); f(e.Cin); f(e.out); f(e.out_fs); f(e.Co);
    }
    void operator()(const ChainArgs& a) {
        Fnv& f = *this;
        f(a.in); f(a.out); f(a.in_fs); f(a.out_fs); f(a.B); f(a.H); f(a.W); f(a.C); f(a.nblocks);
        for (const ChainBlock& b : a.blocks) f(b);
        f(a.pre); f(a.post);
        for (const ChainHead& h : a.heads) { f(h.on); f(h.src); f(h.w_pw); f(h.bias); f(h.Co_a); f(h.Co_b); f(h.out_a); f(h.out_b); f(h.out_a_fs); f(h.out_b_fs); }
        f(a.write_out);
    }
    void operator()(const EltArgs& a) {
        Fnv& f = *this;
        f(a.a); f(a.b); f(a.alpha); f(a.out); f(a.a_fs); f(a.b_fs); f(a.out_fs); f(a.B); f(a.H); f(a.W); f(a.C); f(a.Ho); f(a.Wo); f(a.Co);
        f(a.act); f(a.p0); f(a.p1); f(a.p2); f(a.p3);
    }
    void operator()(const ResBases& r) {
        Fnv& f = *this;
        for (int k = 0; k < kResBases; k++) { f(r.p[k]); f(r.scale[k]); f(r.frame0[k]); }
        f(r.weights);
    }
    void operator()(const ResLaunch& a) {
        Fnv& f = *this;
        f(a.prog); f(a.nstages); f(a.B); f(a.bands); f(a.const_off); f(a.const_floats); f(a.lds_bytes); f(a.bases);
    }
    void operator()(const TailLaunch& a) {
        Fnv& f = *this;
        f(a.prog); f(a.nstages); f(a.B); f(a.G); f(a.frame_floats); f(a.variant); f(a.bases);
    }
    void operator()(const BneckArgs& a) {
        Fnv& f = *this;
        f(a.in); f(a.out); f(a.in_fs); f(a.out_fs); f(a.B); f(a.H); f(a.W); f(a.C); f(a.Cm); f(a.nblocks); f(a.bands);
        for (const BneckBlock& b : a.blocks) { f(b.w1); f(b.w2); f(b.consts); f(b.hi1); f(b.hi2); f(b.mconsts); f(b.act1); f(b.act2); }
    }
    void operator()(const XcArgs& a) {
        Fnv& f = *this;
        f(a.in); f(a.out); f(a.in_fs); f(a.out_fs); f(a.B); f(a.H); f(a.W); f(a.nstages);
        for (const XcStage& s : a.st) { f(s.cblob); f(s.has_dw); f(s.w_pw); f(s.C); f(s.Co); f(s.act); f(s.skip); f(s.res); f(s.res_fs); f(s.res_C); f(s.res_W); }
    }
    void operator()(const DblockArgs& a) {
        Fnv& f = *this;
        f(a.in); f(a.out); f(a.in_fs); f(a.out_fs); f(a.B); f(a.H); f(a.W); f(a.C); f(a.Cm); f(a.Co); f(a.skip1); f(a.skip2_from_a);
        f(a.consts); f(a.w1); f(a.w2); f(a.hi1); f(a.hi2); f(a.mconsts); f(a.act1); f(a.act2);
        f(a.stem_in); f(a.stem_in_fs); f(a.stem_consts); f(a.stem_hi); f(a.band_rows);
    }
    void operator()(const BandLaunch& a) {
        Fnv& f = *this;
        f(a.prog); f(a.nstages); f(a.NW); f(a.F); f(a.lds_bytes); f(a.tiles_floats); f(a.cv2); f(a.wide); f(a.xb); f(a.dw_floats); f(a.ws_frame_floats);
        for (const float* b : a.base) f(b);
        f(a.consts); f(a.sync); f(a.fail); f(a.absent_mod); f(a.stamps);
    }
};

template <class T>
T* fake(uint64_t address) { return reinterpret_cast<T*>(static_cast<uintptr_t>(address)); }

const char* launcher_name(Launcher l) {
    static const char* const names[] = {"conv", "head_gemm", "dw", "xc", "mdblock", "dblock", "mbneck", "bneck", "tail", "resident", "chain", "strip_pipe",
                                        "small_chain", "ms2", "mwalk", "mstrip_chain", "strip", "mstrip", "block", "add", "act", "maxpool", "padc",
                                        "resize2x", "depth_to_space", "bandnet"};
    return names[static_cast<int>(l)];
}

struct Row {
    const char* name;
    int fuse = 5, heads = 1, band = 0;
    bool u8 = false;
    void (*set)(LaunchCtx&) = nullptr;
};

void print_lowered(const Plan& plan, const Lowered& low) {
    for (size_t k = 0; k < low.launches.size(); k++) {
        const Launch& l = low.launches[k];
        int covered = 0;
        for (int of : low.launch_of_node) covered += of == static_cast<int>(k);
        Fnv f;
        const bool many = l.to == Launcher::StripPipe || l.to == Launcher::SmallChain || l.to == Launcher::MstripChain;
        if (many) { f(static_cast<int>(l.blocks.size())); for (const BlockArgs& b : l.blocks) f(b); }
        else std::visit([&](const auto& a) { f(a); }, l.args);
        std::printf("%zu %s \"%s\" nodes=%d-%d(%d) slot=%d wait=%d record=%d args=%016llx\n", k, launcher_name(l.to), l.label.c_str(), l.node, l.last, covered,
                    l.slot, l.wait, l.record ? 1 : 0, static_cast<unsigned long long>(f.h));
    }
    size_t views = 0;
    for (size_t i = 0; i < plan.nodes.size(); i++) views += low.launch_of_node[i] < 0;
    std::printf("nodes=%zu views=%zu\n", plan.nodes.size(), views);
}

// `tensors` mode: per launch its label and the graph tensors it reads from / writes to memory (what a slice of the graph that holds exactly this
// launch is cut at, tests/tfl_slice.py); the views (nodes without a launch) behind them, by their output tensor
void print_tensors(const Plan& plan, const Lowered& low) {
    auto list = [](const std::vector<int>& v) {
        std::string s;
        for (int t : v) s += (s.empty() ? "" : ",") + std::to_string(t);
        return s;
    };
    for (size_t k = 0; k < low.launches.size(); k++) {
        std::vector<int> in, out;
        for (size_t i = 0; i < plan.nodes.size(); i++) {
            if (low.launch_of_node[i] != static_cast<int>(k)) continue;
            const Node& n = plan.nodes[i];
            for (int t : n.in) in.push_back(t);
            out.push_back(n.out);
            for (int t : n.extra_out) out.push_back(t);
            for (const Node& h : n.head_nodes) out.push_back(h.out);
        }
        std::vector<int> ext;
        for (int t : in)
            if (std::find(out.begin(), out.end(), t) == out.end() && std::find(ext.begin(), ext.end(), t) == ext.end()) ext.push_back(t);
        std::printf("%zu \"%s\" in=[%s] out=[%s]\n", k, low.launches[k].label.c_str(), list(ext).c_str(), list(out).c_str());
    }
    for (size_t i = 0; i < plan.nodes.size(); i++)
        if (low.launch_of_node[i] < 0) std::printf("view in=[%s] out=[%d]\n", list(plan.nodes[i].in).c_str(), plan.nodes[i].out);
}

void run_config(const char* model, const std::vector<unsigned char>& blob, const Row& row, int F, bool tensors = false) {
    std::printf("== %s %s F=%d\n", model, row.name, F);
    try {
        const Plan plan = build_plan(parse_tflite(blob.data(), blob.size()), row.fuse, 4, 156 * 1024, true);
        const PlanConsts consts = pack_plan_consts(plan);
        if (row.u8 && !takes_u8_input(plan, consts)) { std::printf("no u8 input form\n"); return; }
        BandPlan bp;
        if (row.band) bp = build_band_plan(plan, build_plan(parse_tflite(blob.data(), blob.size()), 2), BandOptions{128, true, true, 256});
        const SideSchedule sched = schedule_side_streams(plan, row.heads);
        std::vector<float*> outs;
        for (size_t k = 0; k < plan.graph.outputs.size(); k++) outs.push_back(fake<float>(0x040000000000ull + k * 0x001000000000ull));
        LaunchCtx c;
        c.weights = fake<float>(0x010000000000ull); c.arena = fake<float>(0x020000000000ull); c.in = fake<float>(0x030000000000ull);
        c.out = outs.data();
        c.progs = fake<ResStage>(0x060000000000ull); c.tail_progs = fake<TailStage>(0x070000000000ull);
        c.band_prog = fake<BandPacked>(0x080000000000ull); c.band_consts = fake<float>(0x090000000000ull); c.band_ws = fake<float>(0x0a0000000000ull);
        c.band_sync = fake<unsigned>(0x0b0000000000ull); c.band_fail = fake<int>(0x0c0000000000ull);
        c.chunk_cap = F; c.chunk_start = 0; c.F = F;
        c.cu_count = 256;
        if (row.set) row.set(c);
        if (row.u8) {
            const auto& si = plan.graph.tensors[plan.graph.inputs[0]].shape;
            c.u8_frames = fake<uint8_t>(0x0d0000000000ull); c.u8_lut = fake<float>(0x0e0000000000ull);
            c.u8_row_bytes = si.at(2) * 3; c.u8_frame_bytes = static_cast<long>(si.at(1)) * c.u8_row_bytes;
        }
        // the small-batch scratch as the engine sizes it: two frames of the largest row-pipelined chain input per frame of `small_chain`
        size_t fmax = 0;
        for (const Node& n : plan.nodes)
            if (n.kind == Node::Chain) {
                const auto& sh = plan.graph.tensors[n.in[0]].shape;
                if (sh.size() == 4 && sh[1] * sh[2] > 256) fmax = std::max(fmax, static_cast<size_t>(sh[1]) * sh[2] * sh[3]);
            }
        if (fmax && c.small_chain > 0) { c.small = fake<float>(0x050000000000ull); c.small_floats = 2 * static_cast<size_t>(c.small_chain) * fmax; }
        c.band = row.band && bp.ready && c.lanes == 1 && F <= bp.max_frames;
        if (row.band) std::printf("band=%d\n", c.band ? 1 : 0);
        const Lowered low = lower_chunk(plan, consts, bp, sched, c, true);
        if (tensors) print_tensors(plan, low);
        else print_lowered(plan, low);
    } catch (const std::exception& e) {
        std::printf("threw: %s\n", e.what());
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const bool shipped = !std::strcmp(argv[1], "shipped"), tensors = !std::strcmp(argv[1], "tensors");
    if (!shipped && !tensors && std::strcmp(argv[1], "synth")) return 2;
    Row defaults{"defaults"}, fuse2{"fuse=2"}, heads4{"heads=4"}, band2{"band=2"}, u8{"u8"};
    fuse2.fuse = 2; heads4.heads = 4; band2.band = 2; u8.u8 = true;
    const std::vector<Row> rows = {defaults,
                                   {"strip=0", 5, 1, 0, false, [](LaunchCtx& c) { c.strip = 0; }},
                                   {"pair_fuse=0", 5, 1, 0, false, [](LaunchCtx& c) { c.pair_fuse = 0; }},
                                   {"stem_fuse=0", 5, 1, 0, false, [](LaunchCtx& c) { c.stem_fuse = 0; }},
                                   {"mchain=0", 5, 1, 0, false, [](LaunchCtx& c) { c.mchain = 0; }},
                                   {"small_chain=0", 5, 1, 0, false, [](LaunchCtx& c) { c.small_chain = 0; }},
                                   {"stem_mfma=0", 5, 1, 0, false, [](LaunchCtx& c) { c.stem_mfma = 0; }},
                                   {"fork=0", 5, 1, 0, false, [](LaunchCtx& c) { c.fork = false; }},
                                   heads4,
                                   {"lanes=2", 5, 1, 0, false, [](LaunchCtx& c) { c.lanes = 2; c.fork = false; }},   // (several lanes: nothing forks, enqueue_chunk)
                                   fuse2};
    for (int i = 2; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        const std::vector<unsigned char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const char* base = std::strrchr(argv[i], '/') ? std::strrchr(argv[i], '/') + 1 : argv[i];
        if (tensors) {
            for (int F : {1, 3, 32, 33}) run_config(base, b, defaults, F, true);
        } else if (shipped) {
            for (const Row& r : rows)
                for (int F : {1, 4, 5, 16, 17, 31, 32}) run_config(base, b, r, F);
            for (int F : {1, 4}) run_config(base, b, band2, F);
            for (int F : {1, 32}) run_config(base, b, u8, F);
        } else {
            for (const Row& r : {defaults, fuse2})
                for (int F : {1, 32}) run_config(base, b, r, F);
        }
    }
    return 0;
}
