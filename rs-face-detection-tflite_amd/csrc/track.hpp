// track.hpp — the two rules of mi_tracker (landmark-to-ROI face tracking for video streams), stated once for host and device.  The host entries
// mi_track_roi_from_landmarks / mi_track_detect_layout (capi_tracker.cpp) and the kernels of track_kernels.hip all go through the functions below.
// NOT the reference's behaviour (it has no video loop): this is MediaPipe's landmarks-to-ROI step, composed from the reference's own
// bbox_from_landmarks (transform.rs:146-165) and bbox_to_roi (transform.rs:44-109) the way iris_roi_from_face_landmarks composes them for the
// eyes (iris_landmark.rs:268-292).
//
// TRACKED ROI of one item's landmarks (f32 [468][3], normalised to the frame, as the pipeline writes them):
//   bbox       = min / max of x and of y over all 468 landmarks, widened to f64 (min and max do not depend on the order of the reduction)
//   key points = landmarks 33 and 263 (the outer eye corners: iris_landmark.rs's LEFT_EYE_START and RIGHT_EYE_END) in PIXELS, (x * w, y * h),
//                each one f64 multiplication — pixels because face_detection_to_roi takes its key points in pixels and frames are not square
//   roi        = bbox_to_roi(bbox, (w, h), key points, scale (1.5, 1.5), SquareLong)           (face_landmark.rs's ROI_SCALE and size mode)
//   valid      iff every one of the 936 x / y values is finite, BBox::normalized holds, width > 0 and height > 0
//
// DETECT PLAN of S streams with `max_detect` detector slots: the streams with tracked == 0 ("lost") get the slots in cyclic stream order
// beginning at stream `start`: slot j is the j-th lost stream met from `start` on; det_stream[max_detect] holds -1 in unused slots;
// n_detect = {slots used, lost streams left without a slot}.  The handle advances start by max_detect modulo S after every step.
// FAIRNESS: a stream that stays lost gets a slot at least once in any ceil(S / max_detect) consecutive steps (of one max_detect), however many
// streams never show a face: a lost stream whose cyclic position (s - start) mod S is below max_detect has fewer than max_detect lost streams
// in front of it, and the windows [start, start + max_detect) of ceil(S / max_detect) consecutive steps cover every stream.
#pragma once

#include "roi_dev.hpp"

namespace mi {

constexpr int kTrackLandmarks = 468;
constexpr int kTrackEyeA = 33, kTrackEyeB = 263;   // rotation key points
constexpr int kTrackMaxStreams = 65535 / 2;        // one grid row per item of a pre-processing launch, 2 S eyes in the iris stage
constexpr int kTrackLayoutMaxStreams = 1 << 20;    // the host layout entry alone

// ---- tracked ROI
struct TrackBox {          // the reduction's state: any tree of track_box_merge over track_box_of gives the same bits
    float xmin, ymin, xmax, ymax;
    int finite;
};
__host__ __device__ inline bool track_finite(float v) { return v - v == 0.0f; }   // false for NaN and +-Inf
__host__ __device__ inline TrackBox track_box_empty() { return TrackBox{INFINITY, INFINITY, -INFINITY, -INFINITY, 1}; }
__host__ __device__ inline TrackBox track_box_of(float x, float y) { return TrackBox{x, y, x, y, track_finite(x) && track_finite(y) ? 1 : 0}; }
__host__ __device__ inline TrackBox track_box_merge(const TrackBox& a, const TrackBox& b) {
    return TrackBox{fminf(a.xmin, b.xmin), fminf(a.ymin, b.ymin), fmaxf(a.xmax, b.xmax), fmaxf(a.ymax, b.ymax), a.finite & b.finite};
}
// the ROI of a finished box and the two eye corners (x, y of landmarks 33 and 263); returns valid, *out is zeros when it is not
__host__ __device__ inline int track_roi_of_box(const TrackBox& box, const float* eye_a, const float* eye_b, int image_w, int image_h, RectD* out) {
    RectD r = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
    int ok = 0;
    if (box.finite) {
        const double iw = image_w, ih = image_h;
        const double kp[4] = {(double)eye_a[0] * iw, (double)eye_a[1] * ih, (double)eye_b[0] * iw, (double)eye_b[1] * ih};
        const double bbox[4] = {(double)box.xmin, (double)box.ymin, (double)box.xmax, (double)box.ymax};
        ok = bbox_to_roi_dev(bbox, image_w, image_h, kp, 1.5, &r) && r.width > 0.0 && r.height > 0.0 ? 1 : 0;
        if (!ok) r = RectD{0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
    }
    *out = r;
    return ok;
}
// one item, serially (the host entry; the device spreads the merge over a wave)
__host__ __device__ inline int track_roi_from_landmarks(const float* lm /*[468][3]*/, int image_w, int image_h, RectD* out) {
    TrackBox box = track_box_empty();
    for (int i = 0; i < kTrackLandmarks; i++) box = track_box_merge(box, track_box_of(lm[3 * i], lm[3 * i + 1]));
    return track_roi_of_box(box, lm + 3 * kTrackEyeA, lm + 3 * kTrackEyeB, image_w, image_h, out);
}

// ---- detect plan
// the stream at cyclic position p (0 .. S-1) from `start` (0 .. S-1)
__host__ __device__ inline int track_stream_at(int p, int start, int streams) {
    const int s = start + p;
    return s < streams ? s : s - streams;
}
// the slot of the lost stream that has `rank` lost streams in front of it; -1: the budget is spent
__host__ __device__ inline int track_detect_slot(int rank, int max_detect) { return rank < max_detect ? rank : -1; }
__host__ __device__ inline void track_detect_totals(int lost, int max_detect, int n_detect[2]) {
    const int used = lost < max_detect ? lost : max_detect;
    n_detect[0] = used;
    n_detect[1] = lost - used;
}
// the next step's start
inline int track_next_start(int start, int max_detect, int streams) { return (start + max_detect) % streams; }

// ---- the launches of a step (track_kernels.hip); every pointer is device memory
struct PreGeom;
// Plan: ONE workgroup, a scan without atomics over the streams in cyclic order.  Writes det_stream / n_detect, every stream's slot (-1: none)
// and the validity of the detector's `max_detect` uploaded whole-picture geometries: an unused slot is an invalid item, so the pre-processing
// launch writes it a zero tensor and never looks at its frame index of -1.
struct TrackPlanArgs {
    const int* tracked;     // [S]
    int S, max_detect, start;
    int* det_stream;        // [max_detect]
    int* n_detect;          // [2]
    int* stream_slot;       // [S]
    PreGeom* geom;          // [max_detect]: only `valid` is written
};
void launch_track_plan(const TrackPlanArgs& a, hipStream_t s);
// Select: per stream the ROI the mesh runs on and where it came from (2 the state, 1 the detector's top-1 face of its slot, 0 none), and the
// step's per-stream detector results gathered from the slots.
struct TrackSelectArgs {
    int S, cap;
    const int* tracked;         // [S]
    const RectD* state_roi;     // [S]
    const int* stream_slot;     // [S]
    const float* dets;          // [max_detect][cap][17]
    const int* det_counts;      // [max_detect]
    const RectD* det_roi;       // [max_detect] face_detection_to_roi of the slot's first detection
    const int* det_valid;       // [max_detect]
    float* faces;               // [S][17]
    int* face_counts;           // [S]
    int* source;                // [S]
    RectD* rois;                // [S]
    int* valid;                 // [S] source != 0
};
void launch_track_select(const TrackSelectArgs& a, hipStream_t s);
// Update: one wave per stream; where present[s] holds and the tracked ROI of its landmarks is valid that ROI becomes the state and tracked = 1,
// everywhere else tracked = 0 and the state's ROI is zeros.
void launch_track_update(const float* landmarks /*[S][468][3]*/, const int* present, int S, int image_w, int image_h, RectD* state_roi, int* tracked,
                         hipStream_t s);

}  // namespace mi
