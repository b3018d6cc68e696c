// AddressSanitizer driver of tests/test_lowering_asan.py: parse_tflite + build_plan (the host-only lowering, fuse levels 5 and 2) + pack_plan_consts
// (the host-only packing of every accepted plan's constants) of every blob file given on the command line; every blob must give a plan and
// its constants, or an exception (mi_*_create_from_bytes takes untrusted bytes).
#include <cstdio>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <vector>
#include "consts.hpp"
int main(int argc, char** argv) {
    int ok = 0, bad = 0, packed = 0, unpacked = 0;
    for (int i = 1; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        std::vector<unsigned char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        for (int lvl : {5, 2}) {
            mi::Plan plan;
            try { plan = mi::build_plan(mi::parse_tflite(b.data(), b.size()), lvl); std::string s = plan.describe(); ok++; }
            catch (const std::exception&) { bad++; continue; }
            try { packed += mi::pack_plan_consts(plan).blob.size() > 0; }
            catch (const std::exception&) { unpacked++; }
        }
    }
    std::printf("ok %d refused %d packed %d unpacked %d\n", ok, bad, packed, unpacked);
    return 0;
}
