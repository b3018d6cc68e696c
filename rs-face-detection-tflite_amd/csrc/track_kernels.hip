// track_kernels.hip — the three small launches mi_tracker_step adds around the detector, the mesh and the iris network: the detect plan, the
// per-stream ROI selection and the state update.  The rules are track.hpp's; nothing here is read back by the host.
#include "track.hpp"

#include "engine.hpp"
#include "preproc.hpp"

namespace mi {
namespace {

// The detect plan.  ONE workgroup: cyclic positions in chunks of 256, per chunk an exclusive scan of the lost flags (shuffles within a wave,
// the four wave totals through LDS), the running sum carried from chunk to chunk in a register every lane holds — face_items_kernel's scan.
// No atomics: slot j is the j-th lost stream from `start` on by arithmetic alone.
constexpr int kTrackPlanThreads = 256;
__global__ __launch_bounds__(kTrackPlanThreads) void track_plan_kernel(TrackPlanArgs a) {
    __shared__ int s_wave[kTrackPlanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int total = 0;   // lost streams in front of this chunk (uniform)
    for (int p0 = 0; p0 < a.S; p0 += kTrackPlanThreads) {
        const int p = p0 + tid;
        const int stream = p < a.S ? track_stream_at(p, a.start, a.S) : -1;
        const int lost = stream >= 0 && a.tracked[stream] == 0 ? 1 : 0;
        int incl = lost;   // inclusive scan within the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, chunk = 0;
#pragma unroll
        for (int w = 0; w < kTrackPlanThreads / 64; w++) {
            const int t = s_wave[w];
            before += w < wave ? t : 0;
            chunk += t;
        }
        __syncthreads();   // (s_wave is written again by the next chunk)
        if (stream >= 0) {
            const int slot = lost ? track_detect_slot(total + before + incl - lost, a.max_detect) : -1;
            a.stream_slot[stream] = slot;
            if (slot >= 0) {   // (slot < max_detect: track_detect_slot)
                a.det_stream[slot] = stream;
                a.geom[slot].valid = 1;
            }
        }
        total += chunk;
    }
    int n_detect[2];
    track_detect_totals(total, a.max_detect, n_detect);
    for (int j = n_detect[0] + tid; j < a.max_detect; j += kTrackPlanThreads) {   // the unused slots: invalid items
        a.det_stream[j] = -1;
        a.geom[j].valid = 0;
    }
    if (tid == 0) { a.n_detect[0] = n_detect[0]; a.n_detect[1] = n_detect[1]; }
}

// One thread per stream.  A slot index is one the plan kernel wrote for this step: -1 or 0 .. max_detect - 1.
__global__ __launch_bounds__(64) void track_select_kernel(TrackSelectArgs a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    const int slot = a.stream_slot[s];
    const int count = slot >= 0 ? a.det_counts[slot] : 0;
    RectD r = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
    int source = 0;
    if (a.tracked[s] != 0) {
        r = a.state_roi[s];
        source = 2;
    } else if (slot >= 0 && count > 0 && a.det_valid[slot] != 0) {
        r = a.det_roi[slot];
        source = 1;
    }
    const float* d = a.dets + (long)(slot >= 0 ? slot : 0) * a.cap * 17;
    float* f = a.faces + (long)s * 17;
#pragma unroll
    for (int i = 0; i < 17; i++) f[i] = source == 1 ? d[i] : 0.f;
    a.face_counts[s] = count;
    a.source[s] = source;
    a.rois[s] = r;
    a.valid[s] = source != 0 ? 1 : 0;
}

// One wave per stream, four streams per workgroup: the lanes walk the 468 landmarks 64 at a time, the boxes merge across the lanes by
// butterfly shuffles (every lane ends with the whole box), lane 0 finishes the ROI.
constexpr int kTrackUpdateWaves = 4;
__global__ __launch_bounds__(64 * kTrackUpdateWaves) void track_update_kernel(const float* __restrict__ lm, const int* __restrict__ present, int S,
                                                                             int image_w, int image_h, RectD* state_roi, int* tracked) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * kTrackUpdateWaves + (threadIdx.x >> 6);
    if (s >= S) return;   // (whole waves)
    RectD r = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
    int ok = 0;
    if (present[s] != 0) {   // (uniform in the wave)
        const float* p = lm + (long)s * kTrackLandmarks * 3;
        TrackBox box = track_box_empty();
        for (int i = lane; i < kTrackLandmarks; i += 64) box = track_box_merge(box, track_box_of(p[3 * i], p[3 * i + 1]));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            TrackBox o;
            o.xmin = __shfl_xor(box.xmin, d, 64); o.ymin = __shfl_xor(box.ymin, d, 64);
            o.xmax = __shfl_xor(box.xmax, d, 64); o.ymax = __shfl_xor(box.ymax, d, 64);
            o.finite = __shfl_xor(box.finite, d, 64);
            box = track_box_merge(box, o);
        }
        if (lane == 0) ok = track_roi_of_box(box, p + 3 * kTrackEyeA, p + 3 * kTrackEyeB, image_w, image_h, &r);
    }
    if (lane == 0) {
        state_roi[s] = r;
        tracked[s] = ok;
    }
}

}  // namespace

void launch_track_plan(const TrackPlanArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(track_plan_kernel, dim3(1), dim3(kTrackPlanThreads), 0, s, a);
    hip_check(hipGetLastError(), "track_plan kernel launch");
}

void launch_track_select(const TrackSelectArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(track_select_kernel, dim3((a.S + 63) / 64), dim3(64), 0, s, a);
    hip_check(hipGetLastError(), "track_select kernel launch");
}

void launch_track_update(const float* landmarks, const int* present, int S, int image_w, int image_h, RectD* state_roi, int* tracked, hipStream_t s) {
    hipLaunchKernelGGL(track_update_kernel, dim3((S + kTrackUpdateWaves - 1) / kTrackUpdateWaves), dim3(64 * kTrackUpdateWaves), 0, s, landmarks, present,
                       S, image_w, image_h, state_roi, tracked);
    hip_check(hipGetLastError(), "track_update kernel launch");
}

}  // namespace mi
