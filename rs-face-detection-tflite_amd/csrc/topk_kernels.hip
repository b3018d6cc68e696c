// topk_kernels.hip — mi_gallery_topk: the k best gallery rows of every query under the rule of topk.hpp, without the score matrix ever
// reaching memory.  The scores are sim_tile_scores' (sim_tile.hpp), the body of similarity_kernel: bit-equal by construction.
#include "topk.hpp"

#include <stdexcept>

#include "engine.hpp"
#include "sim_tile.hpp"

namespace mi {
namespace {

// ---- phase 1.  Workgroup (ti, sp) owns query rows 128 ti .. and the column tiles [sp T / splits, (sp + 1) T / splits) of the T = tiles_m
// there are, and walks them in index order.  Per tile: sim_tile_scores leaves the 128 x 128 scores in LDS — over the staging tiles, which
// are dead by then — and thread t scans half t & 1 (64 columns) of row t >> 1 in column order against its list of K slots in registers.  A
// candidate is first compared with the list's last slot, which almost every candidate fails once a few tiles have gone by; the insertion
// (topk_insert_later) addresses every slot by a constant.  Rows beyond n and columns beyond m are 0 / 0 = NaN and fail like any NaN.
// LDS: the score tile has rows of 130 floats with one float of padding between the halves, so that the 32 lanes of a half-wave — 16 rows,
// both halves — read banks 2 (row & 15) + half: distinct; the epilogue's stores have 32 lanes on 32 consecutive floats of one row half.
// 128 * 130 * 4 + 1 KiB of norms = 67 584 bytes a workgroup: two workgroups a CU (160 KiB), which is also what the registers allow
// (similarity_kernel itself runs at two).
// At the end the lanes t and t ^ 1 merge their two lists (topk_before, k rounds of compare-the-heads and topk_pop) and the even lane
// writes part[row][sp][0 .. k).
constexpr int kTopkLd = kSimTile + 2, kTopkHalf = kSimTile / 2;
constexpr int kTopkTileFloats = kSimTile * kTopkLd;
static_assert(kTopkTileFloats >= 2 * kSimStageFloats, "the score tile lies over both staging tiles");

template <int K>
__global__ __launch_bounds__(kSimThreads, 2) void gallery_topk_kernel(const float* __restrict__ q, int n, const float* __restrict__ g, int m, int D,
                                                                   int k, int tiles_m, int splits, TopkPair* __restrict__ part) {
    __shared__ float s_tile[kTopkTileFloats];
    __shared__ float s_norm[2 * kSimTile];
    const int tid = threadIdx.x;
    const int ti = blockIdx.x / splits, sp = blockIdx.x - ti * splits;
    const int t_begin = (int)((long)sp * tiles_m / splits), t_end = (int)((long)(sp + 1) * tiles_m / splits);
    const long i0 = (long)ti * kSimTile;
    const int row = tid >> 1, half = tid & 1;
    const float* mine = s_tile + row * kTopkLd + half * (kTopkHalf + 1);
    float ls[K];
    int lj[K];
    topk_clear(ls, lj);
    for (int tj = t_begin; tj < t_end; tj++) {
        const long j0 = (long)tj * kSimTile;
        sim_tile_scores(q, n, g, m, D, i0, j0, s_tile, s_tile + kSimStageFloats, s_norm,
                        [&](int r, int c, auto&& score) { s_tile[r * kTopkLd + c + (c >> 6)] = score(); });
        __syncthreads();
        const int jbase = (int)j0 + half * kTopkHalf;
#pragma unroll 1
        for (int c0 = 0; c0 < kTopkHalf; c0 += 4) {
            float v[4];
#pragma unroll
            for (int c = 0; c < 4; c++) v[c] = mine[c0 + c];
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (topk_before_later(v[c], ls[K - 1])) topk_insert_later(ls, lj, v[c], jbase + c0 + c);
        }
        // (the next tile's first barrier stands between these reads and its first store to LDS)
    }
    const long gi = i0 + row;
    TopkPair* out = part + ((gi < n ? gi : 0) * splits + sp) * k;
    for (int r = 0; r < k; r++) {   // (k <= K; the lists are only ever addressed at their heads)
        const float os = __shfl_xor(ls[0], 1);
        const int oj = __shfl_xor(lj[0], 1);
        const bool first = topk_before(ls[0], lj[0], os, oj);
        if (half == 0 && gi < n) out[r] = TopkPair{first ? ls[0] : os, first ? lj[0] : oj};
        if (first) topk_pop(ls, lj);
    }
}

// ---- phase 2.  One wave per query row, lane l holding list l of the row's `splits` (<= 64) lists in registers.  k rounds: a butterfly of
// topk_before over the heads leaves the best head in every lane, lane 0 writes it with its label, and the lane it came from pops its list.
// Heads are distinct (the column ranges are disjoint) or empty, so every lane agrees; once all are empty the round writes the empty slot.
constexpr int kMergeRows = kSimThreads / 64;

__global__ __launch_bounds__(kSimThreads) void gallery_merge_kernel(const TopkPair* __restrict__ part, int n, int k, int splits,
                                                                    const int* __restrict__ labels, int* __restrict__ index,
                                                                    float* __restrict__ score, int* __restrict__ label) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * kMergeRows + (threadIdx.x >> 6);
    if (i >= n) return;   // (whole waves leave: no barrier follows)
    float ls[kTopkMaxK];
    int lj[kTopkMaxK];
    topk_clear(ls, lj);
    if (lane < splits) {
        const TopkPair* p = part + (i * splits + lane) * k;
#pragma unroll
        for (int r = 0; r < kTopkMaxK; r++)
            if (r < k) {
                const TopkPair e = p[r];
                ls[r] = e.score;
                lj[r] = e.index;
            }
    }
    for (int r = 0; r < k; r++) {
        float bs = ls[0];
        int bj = lj[0];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float os = __shfl_xor(bs, off);
            const int oj = __shfl_xor(bj, off);
            if (topk_before(os, oj, bs, bj)) {
                bs = os;
                bj = oj;
            }
        }
        if (lane == 0) {
            index[i * k + r] = bj;
            score[i * k + r] = bs;
            if (label) label[i * k + r] = bj < 0 ? -1 : (labels ? labels[bj] : bj);
        }
        if (bj >= 0 && lj[0] == bj) topk_pop(ls, lj);
    }
}

template <int K>
void launch_phase1(const float* d_q, int n, const float* d_rows, int m, int D, int k, int tiles_m, int splits, unsigned grid, TopkPair* d_part,
                   hipStream_t s) {
    hipLaunchKernelGGL(gallery_topk_kernel<K>, dim3(grid), dim3(kSimThreads), 0, s, d_q, n, d_rows, m, D, k, tiles_m, splits, d_part);
}

}  // namespace

int gallery_auto_splits(int n, int m, int cu_count) {
    const long tiles_n = (static_cast<long>(n) + kSimTile - 1) / kSimTile, tiles_m = (static_cast<long>(m) + kSimTile - 1) / kSimTile;
    long splits = (cu_count + tiles_n - 1) / tiles_n;
    if (splits > kGalleryMaxSplits) splits = kGalleryMaxSplits;
    if (splits > tiles_m) splits = tiles_m;
    return splits < 1 ? 1 : static_cast<int>(splits);
}

void launch_gallery_topk(const float* d_queries, int n, const float* d_rows, int m, int D, int k, int splits, const int* d_labels, TopkPair* d_part,
                         int* d_index, float* d_score, int* d_label, hipStream_t s) {
    const long tiles_n = (static_cast<long>(n) + kSimTile - 1) / kSimTile, tiles_m = (static_cast<long>(m) + kSimTile - 1) / kSimTile;
    if (k < 1 || k > kTopkMaxK || splits < 1 || splits > kGalleryMaxSplits || splits > tiles_m || m > kGalleryMaxRows)
        throw std::runtime_error("gallery top-k: k, splits or m out of range");
    if (tiles_n * splits > 0x7fffffffL) throw std::runtime_error("gallery top-k: n x splits is too large for one launch");
    const unsigned grid = static_cast<unsigned>(tiles_n * splits);
    // the list length of phase 1: the smallest of 1, 4, 8, 16 that holds k (an insertion costs K compares and selects)
    if (k == 1) launch_phase1<1>(d_queries, n, d_rows, m, D, k, static_cast<int>(tiles_m), splits, grid, d_part, s);
    else if (k <= 4) launch_phase1<4>(d_queries, n, d_rows, m, D, k, static_cast<int>(tiles_m), splits, grid, d_part, s);
    else if (k <= 8) launch_phase1<8>(d_queries, n, d_rows, m, D, k, static_cast<int>(tiles_m), splits, grid, d_part, s);
    else launch_phase1<16>(d_queries, n, d_rows, m, D, k, static_cast<int>(tiles_m), splits, grid, d_part, s);
    hip_check(hipGetLastError(), "gallery top-k kernel launch");
    hipLaunchKernelGGL(gallery_merge_kernel, dim3(static_cast<unsigned>((n + kMergeRows - 1) / kMergeRows)), dim3(kSimThreads), 0, s, d_part, n, k,
                       splits, d_labels, d_index, d_score, d_label);
    hip_check(hipGetLastError(), "gallery merge kernel launch");
}

}  // namespace mi
