// Driver of tests/test_resnet_cpu.py: `resnet_consts_dump file.tflite fuse` lowers the graph, packs the constants (consts.cpp: host code, no GPU) and
// prints, for every convolution node of the plan that has the [Co][K] copy of its filter (PlanConsts::node_wrows: the conv_mfma_kernel form), one line
// `conv Co K` and then the filter rows and the bias as they lie in the blob that is uploaded, one 32-bit pattern per value:
//   w xxxxxxxx ...   (Co * K values)
//   b xxxxxxxx ...   (Co values)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>
#include "consts.hpp"

static void row(const char* tag, const float* p, size_t n) {
    std::printf("%s", tag);
    for (size_t k = 0; k < n; k++) {
        uint32_t u;
        std::memcpy(&u, p + k, 4);
        std::printf(" %08x", u);
    }
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<unsigned char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const mi::Plan plan = mi::build_plan(mi::parse_tflite(b.data(), b.size()), std::atoi(argv[2]), 4, 156 * 1024, true);
    const mi::PlanConsts pc = mi::pack_plan_consts(plan);
    for (size_t i = 0; i < plan.nodes.size(); i++) {
        const mi::Node& n = plan.nodes[i];
        if (n.kind != mi::Node::Conv || pc.node_wrows[i] < 0 || pc.node_b[i] < 0) continue;
        const std::vector<int>& ws = plan.graph.tensors[static_cast<size_t>(n.w)].shape;
        const size_t Co = static_cast<size_t>(ws.at(0)), K = static_cast<size_t>(ws.at(1)) * ws.at(2) * ws.at(3);
        std::printf("conv %zu %zu\n", Co, K);
        row("w", pc.blob.data() + pc.node_wrows[i], Co * K);
        row("b", pc.blob.data() + pc.node_b[i], Co);
    }
    return 0;
}
