// Driver of tests/test_const_pins.py: lowers every model file given on the command line at fuse levels 0, 2, 3, 4, 5 and at level 5 without
// tail programs, packs the constants (consts.cpp: host code, no GPU) and prints one line per configuration: the float count of the blob and
// 64-bit FNV-1a hashes of the blob, of the two stage programs (field by field: the structs have padding) and of every offset table.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>
#include "consts.hpp"

namespace {
struct Fnv {
    uint64_t h = 14695981039346656037ull;
    void bytes(const void* p, size_t n) {
        for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
    }
    template <class... T>
    void operator()(T... v) { (bytes(&v, sizeof v), ...); }
    void operator()(const mi::ResRef& r) { (*this)(r.base, r.root_off, r.inner, r.fs); }
    void operator()(const mi::MemberOff& m) { (*this)(m.w, m.b, m.w2, m.b2, m.alpha, m.strip, m.cblob, m.mconsts); }
    void operator()(const mi::ResStage& s) {
        (*this)(s.kind, s.dw_pg, s.src_off, s.src_H, s.src_W, s.src_C, s.src_PS, s.src_b);
        (*this)(s.src_g);
        (*this)(s.KH, s.KW, s.S, s.pt, s.pl, s.Kv, s.Ho, s.Wo, s.Co, s.dst_off, s.dst_PS, s.dst_b, s.zero_dst);
        (*this)(s.dst_g);
        (*this)(s.res_mode, s.res_C, s.res_H, s.res_W, s.res_off, s.res_PS, s.res_b);
        (*this)(s.res_g);
        (*this)(s.act, s.dw_off, s.band_role, s.band_rows, s.band_H, s.kblk, s.w_pw, s.cblob);
    }
    void operator()(const mi::TailStage& s) {
        (*this)(s.kind, s.K, s.S, s.pt, s.pl, s.src_off, s.src_H, s.src_W, s.src_C);
        (*this)(s.src_g);
        (*this)(s.Kv, s.Ho, s.Wo, s.Co, s.dst_off);
        (*this)(s.dst_g);
        (*this)(s.res_mode, s.res_C, s.res_W, s.res_off);
        (*this)(s.res_g);
        (*this)(s.act, s.scr_off, s.pool_off, s.mHW, s.mW, s.mHWp, s.mWp, s.w_a, s.w_c);
    }
    template <class T>
    void operator()(const std::vector<T>& v) {
        (*this)(v.size());
        for (const T& x : v) (*this)(x);
    }
};
template <class T>
void field(const char* name, const T& v) {
    Fnv f;
    f(v);
    std::printf(" %s=%016llx", name, static_cast<unsigned long long>(f.h));
}
}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        std::vector<unsigned char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const char* base = std::strrchr(argv[i], '/') ? std::strrchr(argv[i], '/') + 1 : argv[i];
        const int cfg[6][2] = {{0, 1}, {2, 1}, {3, 1}, {4, 1}, {5, 1}, {5, 0}};  // (fuse, tail)
        for (const auto& c : cfg) {
            const mi::Plan plan = mi::build_plan(mi::parse_tflite(b.data(), b.size()), c[0], 4, 156 * 1024, c[1] != 0);
            const mi::PlanConsts pc = mi::pack_plan_consts(plan);
            std::printf("%s fuse=%d tail=%d floats=%zu", base, c[0], c[1], pc.blob.size());
            Fnv blob;
            blob.bytes(pc.blob.data(), pc.blob.size() * sizeof(float));
            std::printf(" blob=%016llx", static_cast<unsigned long long>(blob.h));
            field("progs", pc.progs); field("tail_progs", pc.tail_progs); field("node_prog", pc.node_prog);
            field("node_w", pc.node_w); field("node_b", pc.node_b); field("node_w2", pc.node_w2); field("node_b2", pc.node_b2);
            field("node_alpha", pc.node_alpha); field("node_pair", pc.node_pair); field("node_stem", pc.node_stem);
            field("node_mwalk", pc.node_mwalk); field("node_chain_pair", pc.node_chain_pair); field("node_strip", pc.node_strip);
            field("chain_off", pc.chain_off); field("chain_head_off", pc.chain_head_off);
            field("res_wblk", pc.res_wblk); field("res_cblob", pc.res_cblob); field("tail_wa", pc.tail_wa); field("tail_wc", pc.tail_wc);
            std::printf("\n");
        }
    }
    return 0;
}
