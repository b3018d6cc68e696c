// AddressSanitizer driver of tests/test_lowering_asan.py: parse_tflite + build_plan (the host-only lowering, fuse levels 5 and 2) + pack_plan_consts
// (the host-only packing of every accepted plan's constants) of every blob file given on the command line, then build_band_plan (the host-only
// planner of the single-launch program, for 256 compute units, with and without wide stages) where both lowerings succeeded; every blob must
// give a plan, its constants and a band plan (or none), or an exception (mi_*_create_from_bytes takes untrusted bytes).  Every plan that was
// packed is then lowered to its launch list (lower_chunk, launches.cpp: host only) at 1 and at 32 frames, with fake 256-byte-aligned device
// addresses that nothing dereferences: a list, or an exception.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <vector>
#include "bandplan.hpp"
#include "consts.hpp"
#include "launches.hpp"
int main(int argc, char** argv) {
    int ok = 0, bad = 0, packed = 0, unpacked = 0, band_ready = 0, band_none = 0, band_threw = 0, planned = 0, lowered_ok = 0, lowered_threw = 0;
    for (int i = 1; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        std::vector<unsigned char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        mi::Plan plans[2];
        int lowered = 0;
        for (int lvl : {5, 2}) {
            mi::Plan& plan = plans[lvl == 2];
            try { plan = mi::build_plan(mi::parse_tflite(b.data(), b.size()), lvl); std::string s = plan.describe(); ok++; }
            catch (const std::exception&) { bad++; continue; }
            lowered++;
            mi::PlanConsts consts;
            try { consts = mi::pack_plan_consts(plan); packed += consts.blob.size() > 0; }
            catch (const std::exception&) { unpacked++; continue; }
            for (int F : {1, 32}) {
                std::vector<float*> outs;
                for (size_t k = 0; k < plan.graph.outputs.size(); k++) outs.push_back(reinterpret_cast<float*>(0x040000000000ull + k * 0x001000000000ull));
                mi::LaunchCtx c;
                c.weights = reinterpret_cast<float*>(0x010000000000ull); c.arena = reinterpret_cast<float*>(0x020000000000ull);
                c.in = reinterpret_cast<float*>(0x030000000000ull); c.out = outs.data();
                c.small = reinterpret_cast<float*>(0x050000000000ull); c.small_floats = size_t{1} << 30;
                c.progs = reinterpret_cast<mi::ResStage*>(0x060000000000ull); c.tail_progs = reinterpret_cast<mi::TailStage*>(0x070000000000ull);
                c.chunk_cap = c.F = F;
                try { lowered_ok += !mi::lower_chunk(plan, consts, mi::BandPlan(), mi::schedule_side_streams(plan, 1), c, true).launches.empty(); }
                catch (const std::exception&) { lowered_threw++; }
            }
        }
        if (lowered < 2) continue;
        planned++;
        for (bool wide : {true, false}) {
            try { (mi::build_band_plan(plans[0], plans[1], {128, wide, true, 256}).ready ? band_ready : band_none)++; }
            catch (const std::exception&) { band_threw++; }
        }
    }
    std::printf("ok %d refused %d packed %d unpacked %d band_ready %d band_none %d band_threw %d planned %d lowered %d lower_threw %d\n", ok, bad, packed, unpacked, band_ready, band_none, band_threw, planned,
                lowered_ok, lowered_threw);
    return 0;
}
