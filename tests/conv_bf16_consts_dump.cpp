// Driver of tests/test_conv_bf16_cpu.py (host code only, no GPU):
//   conv_bf16_consts_dump consts file.tflite fuse value
//     lowers the graph, packs the constants with pack_plan_consts(plan, value) and prints
//       blob <floats> default_equal <0|1>      (1: the blob is the one-argument call's, byte for byte)
//     then for every convolution node of the plan
//       conv <node> <Co> <KH> <KW> <C> wrows <offset|-1> hi <offset|-1> lo <offset|-1>
//     and, where it has them, the filter rows as stored (32-bit patterns) and the bf16 planes (16-bit patterns, in element order):
//       w xxxxxxxx ...    hi xxxx ...    lo xxxx ...
//   conv_bf16_consts_dump launches file.tflite fuse value F
//     the launch list lower_chunk makes of a chunk of F frames with LaunchCtx::conv_bf16 = value (constants packed with the same value;
//     256 compute units, fake device addresses that nothing dereferences), one line per launch:
//       <label> nodes=<first>-<last> slot=<s> wait=<w> bf16=<0|1>     (bf16: a convolution launch that conv_bf16_supports takes)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>
#include "launches.hpp"

using namespace mi;

template <class T>
static T* fake(uint64_t address) { return reinterpret_cast<T*>(static_cast<uintptr_t>(address)); }

static int dump_consts(const Plan& plan, int value) {
    const PlanConsts pc = pack_plan_consts(plan, value), def = pack_plan_consts(plan);
    const bool same = pc.blob.size() == def.blob.size() && !std::memcmp(pc.blob.data(), def.blob.data(), def.blob.size() * sizeof(float));
    std::printf("blob %zu default_equal %d\n", pc.blob.size(), same ? 1 : 0);
    for (size_t i = 0; i < plan.nodes.size(); i++) {
        const Node& n = plan.nodes[i];
        if (n.kind != Node::Conv) continue;
        const std::vector<int>& ws = plan.graph.tensors[static_cast<size_t>(n.w)].shape;
        const size_t count = static_cast<size_t>(ws.at(0)) * ws.at(1) * ws.at(2) * ws.at(3);
        std::printf("conv %zu %d %d %d %d wrows %ld hi %ld lo %ld\n", i, ws[0], ws[1], ws[2], ws[3], pc.node_wrows[i], pc.node_wbf16_hi[i], pc.node_wbf16_lo[i]);
        if (pc.node_wrows[i] >= 0) {
            std::printf("w");
            for (size_t k = 0; k < count; k++) {
                uint32_t u;
                std::memcpy(&u, pc.blob.data() + pc.node_wrows[i] + k, 4);
                std::printf(" %08x", u);
            }
            std::printf("\n");
        }
        for (const auto& plane : {std::make_pair("hi", pc.node_wbf16_hi[i]), std::make_pair("lo", pc.node_wbf16_lo[i])}) {
            if (plane.second < 0) continue;
            if (static_cast<size_t>(plane.second) + count / 2 > pc.blob.size()) return 3;
            std::printf("%s", plane.first);
            const unsigned char* p = reinterpret_cast<const unsigned char*>(pc.blob.data() + plane.second);
            for (size_t k = 0; k < count; k++) {
                uint16_t h;
                std::memcpy(&h, p + 2 * k, 2);
                std::printf(" %04x", h);
            }
            std::printf("\n");
        }
    }
    return 0;
}

static int dump_launches(const Plan& plan, int value, int F) {
    const PlanConsts consts = pack_plan_consts(plan, value);
    const BandPlan bp;
    const SideSchedule sched = schedule_side_streams(plan, 1);
    std::vector<float*> outs;
    for (size_t k = 0; k < plan.graph.outputs.size(); k++) outs.push_back(fake<float>(0x040000000000ull + k * 0x001000000000ull));
    LaunchCtx c;
    c.weights = fake<float>(0x010000000000ull); c.arena = fake<float>(0x020000000000ull); c.in = fake<float>(0x030000000000ull);
    c.out = outs.data();
    c.progs = fake<ResStage>(0x060000000000ull); c.tail_progs = fake<TailStage>(0x070000000000ull);
    c.chunk_cap = F; c.chunk_start = 0; c.F = F;
    c.cu_count = 256;
    c.conv_bf16 = value;
    size_t fmax = 0;   // the small-batch scratch as the engine sizes it
    for (const Node& n : plan.nodes)
        if (n.kind == Node::Chain) {
            const auto& sh = plan.graph.tensors[n.in[0]].shape;
            if (sh.size() == 4 && sh[1] * sh[2] > 256) fmax = std::max(fmax, static_cast<size_t>(sh[1]) * sh[2] * sh[3]);
        }
    if (fmax && c.small_chain > 0) { c.small = fake<float>(0x050000000000ull); c.small_floats = 2 * static_cast<size_t>(c.small_chain) * fmax; }
    const Lowered low = lower_chunk(plan, consts, bp, sched, c, true);
    for (const Launch& l : low.launches) {
        const bool bf16 = l.to == Launcher::Conv && conv_bf16_supports(std::get<ConvArgs>(l.args));
        std::printf("%s nodes=%d-%d slot=%d wait=%d bf16=%d\n", l.label.c_str(), l.node, l.last, l.slot, l.wait, bf16 ? 1 : 0);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    std::ifstream f(argv[2], std::ios::binary);
    const std::vector<unsigned char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const Plan plan = build_plan(parse_tflite(b.data(), b.size()), std::atoi(argv[3]), 4, 156 * 1024, true);
    const int value = std::atoi(argv[4]);
    if (!std::strcmp(argv[1], "consts")) return dump_consts(plan, value);
    if (!std::strcmp(argv[1], "launches") && argc >= 6) return dump_launches(plan, value, std::atoi(argv[5]));
    return 2;
}
