// Driver of tests/test_band_pins.py: `bandplan_dump ROWS file.tflite ...` lowers every model file at the engine's defaults (fuse 5, pipe 4,
// 156 KiB, tail on) and at level 2, plans the single-launch program (bandplan.cpp: host code, no GPU) for 256 compute units under the first
// ROWS option rows {defaults; wide = 0; fork = 0; nw = 64; nw = 32}, and prints one line per configuration: the plan's scalars in plain text
// and 64-bit FNV-1a hashes of the packed stages, the constants, ext and node_runs.  (A plan that is not ready is all defaults.)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>
#include "bandplan.hpp"

namespace {
struct Fnv {
    uint64_t h = 14695981039346656037ull;
    void bytes(const void* p, size_t n) {
        for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
    }
    template <class T>
    void operator()(T v) { bytes(&v, sizeof v); }
};
void hash(const char* name, const Fnv& f) { std::printf(" %s=%016llx", name, static_cast<unsigned long long>(f.h)); }

void print_band_plan(const char* model, const mi::BandOptions& o, const mi::BandPlan& bp) {
    std::printf("%s opt_nw=%d opt_wide=%d opt_fork=%d", model, o.nw, o.wide ? 1 : 0, o.fork ? 1 : 0);
    std::printf(" ready=%d first=%d stem_out=%d nw=%d max_frames=%d nstages=%d lds_bytes=%d tiles_floats=%d dw_floats=%d ws_frame_floats=%ld cv2=%d xb=%d wide=%d",
                bp.ready ? 1 : 0, bp.first, bp.stem_out, bp.nw, bp.max_frames, bp.nstages, bp.lds_bytes, bp.tiles_floats, bp.dw_floats, bp.ws_frame_floats,
                bp.cv2 ? 1 : 0, bp.xb ? 1 : 0, bp.wide ? 1 : 0);
    Fnv prog, consts, ext, runs;
    prog(bp.prog.size());
    for (const mi::BandPacked& q : bp.prog) prog.bytes(q.w, sizeof q.w);
    consts(bp.consts.size());
    consts.bytes(bp.consts.data(), bp.consts.size() * sizeof(float));
    ext(bp.ext.size());
    for (const mi::BandExt& e : bp.ext) { ext(e.out_k); ext(e.tensor); }
    runs(bp.node_runs.size());
    runs.bytes(bp.node_runs.data(), bp.node_runs.size());
    hash("prog", prog); hash("consts", consts); hash("ext", ext); hash("node_runs", runs);
    std::printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
    const mi::BandOptions rows[5] = {{128, true, true, 256}, {128, false, true, 256}, {128, true, false, 256}, {64, true, true, 256}, {32, true, true, 256}};
    const int nrows = argc > 1 ? std::atoi(argv[1]) : 0;
    if (nrows < 1 || nrows > 5) return 2;
    for (int i = 2; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        std::vector<unsigned char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const char* base = std::strrchr(argv[i], '/') ? std::strrchr(argv[i], '/') + 1 : argv[i];
        const mi::Plan plan = mi::build_plan(mi::parse_tflite(b.data(), b.size()), 5, 4, 156 * 1024, true);
        const mi::Plan level2 = mi::build_plan(mi::parse_tflite(b.data(), b.size()), 2);
        for (int r = 0; r < nrows; r++) print_band_plan(base, rows[r], mi::build_band_plan(plan, level2, rows[r]));
    }
    return 0;
}
