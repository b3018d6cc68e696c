// AddressSanitizer driver of tests/test_lowering_asan.py: parse_tflite + build_plan (the host-only lowering, fuse levels 5 and 2) + pack_plan_consts
// (the host-only packing of every accepted plan's constants) of every blob file given on the command line, then build_band_plan (the host-only
// planner of the single-launch program, for 256 compute units, with and without wide stages) where both lowerings succeeded; every blob must
// give a plan, its constants and a band plan (or none), or an exception (mi_*_create_from_bytes takes untrusted bytes).
#include <cstdio>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <vector>
#include "bandplan.hpp"
#include "consts.hpp"
int main(int argc, char** argv) {
    int ok = 0, bad = 0, packed = 0, unpacked = 0, band_ready = 0, band_none = 0, band_threw = 0, planned = 0;
    for (int i = 1; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        std::vector<unsigned char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        mi::Plan plans[2];
        int lowered = 0;
        for (int lvl : {5, 2}) {
            mi::Plan& plan = plans[lvl == 2];
            try { plan = mi::build_plan(mi::parse_tflite(b.data(), b.size()), lvl); std::string s = plan.describe(); ok++; }
            catch (const std::exception&) { bad++; continue; }
            try { packed += mi::pack_plan_consts(plan).blob.size() > 0; }
            catch (const std::exception&) { unpacked++; }
            lowered++;
        }
        if (lowered < 2) continue;
        planned++;
        for (bool wide : {true, false}) {
            try { (mi::build_band_plan(plans[0], plans[1], {128, wide, true, 256}).ready ? band_ready : band_none)++; }
            catch (const std::exception&) { band_threw++; }
        }
    }
    std::printf("ok %d refused %d packed %d unpacked %d band_ready %d band_none %d band_threw %d planned %d\n", ok, bad, packed, unpacked, band_ready, band_none, band_threw, planned);
    return 0;
}
