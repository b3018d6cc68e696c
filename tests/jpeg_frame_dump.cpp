// jpeg_frame_dump.cpp — test harness (built by tests/test_jpeg_edges.py with g++, CPU only): runs the product's host half of the JPEG
// path, mi::jpeg_entropy_decode (csrc/jpeg.cpp), on every file named and writes what it hands to the two kernels, so that a plain
// restatement of the kernels (tests/jpeg_ref.py) can turn it into pixels without a GPU.
//   usage: jpeg_frame_dump OUT_DIR FILE...      -> OUT_DIR/<k>.frame for the k-th file
//   a decoded frame:  "ok <width> <height> <ncomp> <hmax> <vmax> <progressive> <ncoef>\n", per component
//                     "<id> <h> <v> <tq> <bw> <bh> <dw> <dh> <coef_off>\n", then raw little-endian uint16 qt[4][64] and int16 coef[ncoef]
//   a refused stream: "refused <what()>\n"
// jpeg_parse_size runs first on the same bytes: "info <width> <height>\n" or "info refused <what()>\n" is the first line.
#include <cstdint>
#include <cstdio>
#include <exception>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../rs-face-detection-tflite_amd/csrc/jpeg.hpp"

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s OUT_DIR FILE...\n", argv[0]); return 2; }
    for (int a = 2; a < argc; a++) {
        std::ifstream in(argv[a], std::ios::binary);
        if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        const std::vector<uint8_t> b((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const std::string path = std::string(argv[1]) + "/" + std::to_string(a - 2) + ".frame";
        std::FILE* out = std::fopen(path.c_str(), "wb");
        if (!out) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 2; }
        try {
            int w = 0, h = 0;
            mi::jpeg_parse_size(b.data(), b.size(), &w, &h);
            std::fprintf(out, "info %d %d\n", w, h);
        } catch (const std::exception& e) {
            std::fprintf(out, "info refused %s\n", e.what());
        }
        try {
            mi::JpegFrame f;
            mi::jpeg_entropy_decode(b.data(), b.size(), &f);
            std::fprintf(out, "ok %d %d %d %d %d %d %zu\n", f.width, f.height, f.ncomp, f.hmax, f.vmax, f.progressive ? 1 : 0, f.coef.size());
            for (int c = 0; c < f.ncomp; c++) {
                const mi::JpegComponent& cp = f.comp[c];
                std::fprintf(out, "%d %d %d %d %d %d %d %d %zu\n", cp.id, cp.h, cp.v, cp.tq, cp.bw, cp.bh, cp.dw, cp.dh, cp.coef_off);
            }
            std::fwrite(&f.qt[0][0], sizeof(uint16_t), 4 * 64, out);
            std::fwrite(f.coef.data(), sizeof(int16_t), f.coef.size(), out);
        } catch (const std::exception& e) {
            std::fprintf(out, "refused %s\n", e.what());
        }
        std::fclose(out);
    }
    return 0;
}
