// face_items.hpp — the item list of mi_pipeline_run_faces: which (frame, face) pairs get a mesh / iris slot.  The per-slot arithmetic below is
// the only statement of the rule; the host entry mi_face_items_layout (capi_pipeline.cpp) and face_items_kernel (preproc.hip) both go through it.
//
//   frame b contributes n_b = min(max(face_counts[b], 0), max_faces) faces; item j = (sum of n_b' for b' < b) + k is face k of frame b while
//   j < max_items; n_items = {min(total, max_items), total - min(total, max_items)}; slots behind the last item hold -1 / -1.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_FACE_ITEMS_HD __host__ __device__
#else
#define MI_FACE_ITEMS_HD
#endif

namespace mi {

constexpr int kFaceItemsMaxFaces = 16;        // max_faces: 1..16
constexpr int kFaceItemsMaxItems = 1 << 20;   // max_items of the layout: 1..2^20
// max_items mi_pipeline_run_faces runs: the pre-processing launch has one grid row (of at most 65535) per item, and the iris stage has two
// items (eyes) per face item
constexpr int kFaceItemsMaxRunItems = 65535 / 2;
constexpr int kFaceItemsMaxBatch = 1 << 26;   // (16 faces of each of 2^26 frames still count in an int)

// n_b: the faces frame b contributes (a negative count is the detector's report of a letterbox it cannot undo: no faces)
MI_FACE_ITEMS_HD inline int face_items_of_frame(int face_count, int max_faces) {
    const int n = face_count > 0 ? face_count : 0;
    return n < max_faces ? n : max_faces;
}

// the slot of face k of a frame whose faces start at `first` (the exclusive sum of n_b over the frames before it); -1: the budget is spent
MI_FACE_ITEMS_HD inline int face_items_slot(int first, int k, int max_items) {
    const int j = first + k;
    return j < max_items ? j : -1;
}

// n_items[0] = slots used, n_items[1] = faces (within max_faces) that got no slot
MI_FACE_ITEMS_HD inline void face_items_totals(int total, int max_items, int n_items[2]) {
    const int used = total < max_items ? total : max_items;
    n_items[0] = used;
    n_items[1] = total - used;
}

}  // namespace mi
