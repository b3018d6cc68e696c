// topk.hpp — which gallery rows a query matches: the selection rule of mi_topk_select and mi_gallery_topk.  The comparator and the list
// operations below are the only statement of the rule; the host entry mi_topk_select (capi_embed.cpp) and the kernels of topk_kernels.hip all go
// through them.
//
//   For query row i, gallery row j is ELIGIBLE iff S[i][j] > -INFINITY is true: NaN (a zero query or a zero gallery row, through the
//   reference's IEEE division) and -inf are never selected.  Eligible rows are ordered by score descending under the plain f32 `>` (so -0.0
//   and +0.0 tie), ties by the lower j.  The result is the first k rows of that order; slots beyond the number of eligible rows hold
//   index -1, score -INFINITY (and label -1).
//
// The order is total on eligible rows, so every correct algorithm returns the same bytes: the kernels may split the columns, keep partial
// lists and merge them in any arrangement.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_TOPK_HD __host__ __device__
#else
#define MI_TOPK_HD
#endif

namespace mi {

constexpr int kTopkMaxK = 16;               // k: 1..16
constexpr int kGalleryMaxRows = 1 << 24;    // m of a gallery: 1..2^24
constexpr int kGalleryMaxSplits = 64;       // column ranges a row of query tiles is spread over: 1..64

struct TopkPair {   // a list entry; the empty slot is {-INFINITY, -1}
    float score;
    int index;
};

MI_TOPK_HD inline float topk_empty_score() { return -__builtin_huge_valf(); }
MI_TOPK_HD inline bool topk_eligible(float score) { return score > topk_empty_score(); }

// Does entry a come before entry b?  a and b are eligible entries or empty slots: an eligible entry comes before an empty slot, and of two
// empty slots neither comes first.
MI_TOPK_HD inline bool topk_before(float sa, int ja, float sb, int jb) { return sa > sb || (sa == sb && ja < jb); }
// The same for a candidate a whose index is above every index b can have (columns visited in index order): it loses every tie.  With an
// empty slot for b this is the eligibility test itself, and a NaN fails it.
MI_TOPK_HD inline bool topk_before_later(float sa, float sb) { return sa > sb; }

// A list is K slots sorted by the order above, empty slots last.
template <int K>
MI_TOPK_HD inline void topk_clear(float (&s)[K], int (&j)[K]) {
#pragma unroll
    for (int r = 0; r < K; r++) {
        s[r] = topk_empty_score();
        j[r] = -1;
    }
}

// Insert a candidate that topk_before_later(cs, s[K - 1]) has admitted (so it is eligible and the last slot falls out).  Every slot is
// addressed by a constant: the list stays in registers.
template <int K>
MI_TOPK_HD inline void topk_insert_later(float (&s)[K], int (&j)[K], float cs, int cj) {
#pragma unroll
    for (int r = K - 1; r >= 1; r--) {
        const bool above = topk_before_later(cs, s[r - 1]), here = topk_before_later(cs, s[r]);
        j[r] = above ? j[r - 1] : (here ? cj : j[r]);
        s[r] = above ? s[r - 1] : (here ? cs : s[r]);
    }
    const bool first = topk_before_later(cs, s[0]);
    j[0] = first ? cj : j[0];
    s[0] = first ? cs : s[0];
}

// Drop the first entry (a merge has taken it).
template <int K>
MI_TOPK_HD inline void topk_pop(float (&s)[K], int (&j)[K]) {
#pragma unroll
    for (int r = 0; r + 1 < K; r++) {
        s[r] = s[r + 1];
        j[r] = j[r + 1];
    }
    s[K - 1] = topk_empty_score();
    j[K - 1] = -1;
}

// One row of mi_topk_select: scores[m] in index order -> index[k], score[k].
inline void topk_select_row(const float* scores, int m, int k, int* index, float* score) {
    float s[kTopkMaxK];
    int j[kTopkMaxK];
    topk_clear(s, j);
    // (the list is kTopkMaxK long whatever k is: its first k slots are the first k rows of the order)
    for (int c = 0; c < m; c++)
        if (topk_before_later(scores[c], s[kTopkMaxK - 1])) topk_insert_later(s, j, scores[c], c);
    for (int r = 0; r < k; r++) {
        index[r] = j[r];
        score[r] = s[r];
    }
}

// ---- device side (topk_kernels.hip).  Phase 1: tiles_n x splits workgroups, each 128 query rows against a contiguous range of 128-column
// tiles, writes its k best per row to part[n][splits][k]; phase 2 merges the `splits` lists of a row, gathers labels (d_labels null: the
// label is the index) and writes every one of the n * k slots.  d_label may be null.
#if defined(__HIPCC__)
// the automatic `splits`: the smallest count for which tiles_n * splits reaches the device's CU count, at most the column tiles and 64
int gallery_auto_splits(int n, int m, int cu_count);
void launch_gallery_topk(const float* d_queries, int n, const float* d_rows, int m, int D, int k, int splits, const int* d_labels, TopkPair* d_part,
                         int* d_index, float* d_score, int* d_label, hipStream_t s);
#endif

}  // namespace mi
