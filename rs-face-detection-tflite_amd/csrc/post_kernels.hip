// post_kernels.hip — what the reference crate does in Rust behind its networks, on the device:
//   ssd_postprocess_kernel    face_detection.rs:269-362 + nms.rs:56-144 + transform.rs:115-142, one workgroup/frame
//   project_landmarks_kernel  transform.rs:351-432
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "roi_dev.hpp"

namespace mi {

// ------------------------------------------------------------------------------------------------ SSD post-processing
// One 256-thread workgroup per frame.  Restates, on the device, the tail of FaceDetection::infer
// (face_detection.rs:259-265): decode_boxes (269-296), get_sigmoid_score (300-314), convert_to_detections
// (317-362), non_maximum_suppression(weighted) (nms.rs:56-144) and detection_letterbox_removal (transform.rs:115-142).
// Ordering/dtype rules kept bit-for-bit: true f32 division by `scale`, score clamp to
// +-80, `sigmoid(x) > 0.5` on the f32 sigmoid, stable descending sort == sort by (score desc, anchor index asc),
// IoU in f64 on f32 coordinates with strict `> 0.3`, weighted sums accumulated in sorted order in f32 with separate
// multiply and add (no FMA), output score = head score, stop when nothing was removed.

__device__ __forceinline__ float sigmoid_f32(float x) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x))); }

// feature f (0..15) of the decoded detection of anchor `a` (face_detection.rs:274-293)
__device__ __forceinline__ float decode_feature(const float* __restrict__ rb, const float* __restrict__ anchors, int a, int f,
                                                float scale) {
    const float* r = rb + (long)a * 16;
    float anc = anchors[2 * a + (f & 1)];
    if (f < 4) {
        float c = __fadd_rn(__fdiv_rn(r[f & 1], scale), anc);            // centre + anchor
        float h = __fdiv_rn(__fdiv_rn(r[2 + (f & 1)], scale), 2.0f);     // size / 2 (no anchor term)
        return f < 2 ? __fsub_rn(c, h) : __fadd_rn(c, h);
    }
    return __fadd_rn(__fdiv_rn(r[f], scale), anc);
}

__device__ __forceinline__ double iou_f64(const float* b1, const float* b2) {  // nms.rs:5-17, types.rs:123-159
    double x0 = fmax((double)b1[0], (double)b2[0]), y0 = fmax((double)b1[1], (double)b2[1]);
    double x1 = fmin((double)b1[2], (double)b2[2]), y1 = fmin((double)b1[3], (double)b2[3]);
    if (!(x0 < x1 && y0 < y1)) return 0.0;
    double iw = x1 - x0, ih = y1 - y0;
    double ia = (iw <= 0.0 || ih <= 0.0) ? 0.0 : iw * ih;
    double w1 = (double)b1[2] - (double)b1[0], h1 = (double)b1[3] - (double)b1[1];
    double w2 = (double)b2[2] - (double)b2[0], h2 = (double)b2[3] - (double)b2[1];
    double a1 = (w1 <= 0.0 || h1 <= 0.0) ? 0.0 : w1 * h1;
    double a2 = (w2 <= 0.0 || h2 <= 0.0) ? 0.0 : w2 * h2;
    double den = a1 + a2 - ia;
    return den > 0.0 ? ia / den : 0.0;
}

template <int NP>  // NP = power of two >= number of anchors
__global__ __launch_bounds__(256) void ssd_postprocess_kernel(PostArgs a) {
    __shared__ unsigned long long keys[NP];   // (~score bits) << 32 | anchor index; sorted ascending
    __shared__ float boxes[NP][4];            // decoded (xmin,ymin,xmax,ymax) per sorted position (first M valid)
    __shared__ unsigned char state[NP];       // 1 = still in `remaining`, 2 = candidate of the current head
    __shared__ int s_count, s_removed, s_head;
    __shared__ float s_w[17];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* rb = a.raw_boxes + (long)b * a.N * 16;
    const float* rs = a.raw_scores + (long)b * a.N;
    if (tid == 0) s_count = 0;
    __syncthreads();
    // --- threshold + validity (convert_to_detections); order-insensitive compaction, the sort restores the order
    for (int i = tid; i < a.N; i += 256) {
        float x = rs[i];
        x = x < -80.0f ? -80.0f : (x > 80.0f ? 80.0f : x);
        float s = sigmoid_f32(x);
        if (s > 0.5f) {
            float x0 = decode_feature(rb, a.anchors, i, 0, a.scale), y0 = decode_feature(rb, a.anchors, i, 1, a.scale);
            float x1 = decode_feature(rb, a.anchors, i, 2, a.scale), y1 = decode_feature(rb, a.anchors, i, 3, a.scale);
            if (x1 > x0 && y1 > y0) {
                int slot = atomicAdd(&s_count, 1);
                keys[slot] = ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(s)) << 32) | (unsigned)i;
            }
        }
    }
    __syncthreads();
    const int M = s_count;
    int P = 1;
    while (P < M) P <<= 1;
    for (int i = M + tid; i < P; i += 256) keys[i] = ~0ull;
    __syncthreads();
    // --- bitonic sort of P keys (unique keys => deterministic, equals the reference's stable sort)
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 256) {
                int l = i ^ j;
                if (l > i) {
                    unsigned long long x = keys[i], y = keys[l];
                    bool up = (i & k) == 0;
                    if ((x > y) == up) { keys[i] = y; keys[l] = x; }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < M; i += 256) {
        int an = (int)(keys[i] & 0xFFFFFFFFu);
#pragma unroll
        for (int f = 0; f < 4; f++) boxes[i][f] = decode_feature(rb, a.anchors, an, f, a.scale);
        state[i] = 1;
    }
    if (tid == 0) s_head = 0;
    __syncthreads();
    // letterbox constants (transform.rs:116-141)
    float lb_l = 0.f, lb_t = 0.f, lb_hs = 1.f, lb_vs = 1.f;
    bool lb_bad = false;
    if (a.padding) {
        const double* pd = a.padding + (long)b * 4;
        double hs = 1.0 - (pd[0] + pd[2]), vs = 1.0 - (pd[1] + pd[3]);
        lb_bad = !(hs > 2.220446049250313e-16) || !(vs > 2.220446049250313e-16);
        lb_l = (float)pd[0]; lb_t = (float)pd[1]; lb_hs = (float)hs; lb_vs = (float)vs;
    }
    int nout = 0;
    const double thr = (double)0.3f;  // MIN_SUPPRESSION_THRESHOLD as f64 (face_detection.rs:139, nms.rs:87)
    float* outp = a.out + (long)b * a.cap * 17;
    while (true) {
        // head = first entry of `remaining`
        if (tid == 0) {
            int h = s_head;
            while (h < M && state[h] == 0) h++;
            s_head = h;
            s_removed = 0;
        }
        __syncthreads();
        const int head = s_head;
        if (head >= M) break;
        const float head_score = __uint_as_float(0xFFFFFFFFu - (unsigned)(keys[head] >> 32));
        // (head.score < MIN_SCORE cannot happen: every kept score is > 0.5 — nms.rs:69-73)
        int removed = 0;
        for (int i = head + tid; i < M; i += 256) {
            if (state[i] == 0) continue;
            double sim = iou_f64(boxes[i], boxes[head]);
            if (sim > thr) { state[i] = 2; removed++; }
        }
        if (removed) atomicAdd(&s_removed, removed);
        __syncthreads();
        const int nrem = s_removed;
        // weighted merge (nms.rs:94-112): lanes 0..15 own one feature each, lane 16 owns total_score; sequential
        // f32 accumulation in sorted order, separate multiply and add.
        if (tid < 17) {
            float acc = 0.0f;
            if (nrem > 0) {
                for (int i = head; i < M; i++) {
                    if (state[i] != 2) continue;
                    unsigned long long k = keys[i];
                    float s = __uint_as_float(0xFFFFFFFFu - (unsigned)(k >> 32));
                    if (tid == 16) acc = __fadd_rn(acc, s);
                    else acc = __fadd_rn(acc, __fmul_rn(decode_feature(rb, a.anchors, (int)(k & 0xFFFFFFFFu), tid, a.scale), s));
                }
            } else if (tid < 16) {
                acc = decode_feature(rb, a.anchors, (int)(keys[head] & 0xFFFFFFFFu), tid, a.scale);  // detection.clone()
            }
            s_w[tid] = acc;
        }
        __syncthreads();
        if (tid < 17 && nout < a.cap) {
            float v;
            if (tid == 16) v = head_score;
            else {
                v = nrem > 0 ? __fdiv_rn(s_w[tid], s_w[16]) : s_w[tid];
                if (a.padding)  // detection_letterbox_removal: (v - left) / h_scale, (v - top) / v_scale
                    v = (tid & 1) ? __fdiv_rn(__fsub_rn(v, lb_t), lb_vs) : __fdiv_rn(__fsub_rn(v, lb_l), lb_hs);
            }
            outp[(long)nout * 17 + tid] = v;
        }
        nout++;
        for (int i = head + tid; i < M; i += 256)
            if (state[i] == 2) state[i] = 0;
        __syncthreads();
        if (nrem == 0) break;  // "number of indexed scores didn't change" (nms.rs:117-119)
    }
    if (tid == 0) a.counts[b] = lb_bad ? -1 : nout;  // -1: the reference's letterbox assert! would have fired
    if (a.zero_rest)
        for (int i = min(nout, a.cap) * 17 + tid; i < a.cap * 17; i += 256) outp[i] = 0.f;
    if (a.face_rois && tid == 0) {   // (slot 0 was written by this workgroup, barriers since)
        RectD r;
        a.face_valid[b] = face_roi_dev(outp, lb_bad ? -1 : nout, a.image_w, a.image_h, &r);
        a.face_rois[b] = r;
    }
}

int launch_postprocess(const PostArgs& a, void* stream) {
    if (a.B <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (a.N <= 1024) hipLaunchKernelGGL(ssd_postprocess_kernel<1024>, dim3(a.B), dim3(256), 0, s, a);
    else if (a.N <= 2048) hipLaunchKernelGGL(ssd_postprocess_kernel<2048>, dim3(a.B), dim3(256), 0, s, a);
    else if (a.N <= 4096) hipLaunchKernelGGL(ssd_postprocess_kernel<4096>, dim3(a.B), dim3(256), 0, s, a);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ landmark projection
// project_landmarks (transform.rs:351-432); one thread per landmark; f32/f64 mix kept as in the Rust source.
__global__ void project_landmarks_kernel(ProjArgs a) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int nt = a.n + a.n2;
    if (idx >= (long)a.B * nt) return;
    const int b = (int)(idx / nt), k = (int)(idx % nt);
    // (a second list of landmarks of the same items — the iris network's two outputs, iris_landmark.rs:213-245, in one launch)
    const bool second = k >= a.n;
    const int li = second ? k - a.n : k;            // index within its list
    const int i = second ? -1 : li;                 // i == 0: the item's first landmark (the flag and the gate bookkeeping belong to it)
    float* o = (second ? a.out2 + (long)b * (a.out2_fs ? a.out2_fs : 3L * a.n2) : a.out + (long)b * (a.out_fs ? a.out_fs : 3L * a.n)) + 3 * li;
    if (a.gate && !a.gate[b]) {
        o[0] = o[1] = o[2] = 0.f;
        if (i == 0 && a.present) a.present[b] = 0;
        if (i == 0 && a.raw_flag_out && a.flag) a.raw_flag_out[b] = a.flag[(long)b * a.flag_fs];
        return;
    }
    const float* r = (second ? a.raw2 + (long)b * a.raw2_fs : a.raw + (long)b * a.raw_fs) + 3 * li;
    float wf = (float)a.tensor_w, hf = (float)a.tensor_h;
    float x = __fdiv_rn(r[0], wf), y = __fdiv_rn(r[1], hf), z = __fdiv_rn(r[2], wf);
    if (a.flip && a.flip[b]) x = __fadd_rn(__fmul_rn(x, -1.0f), 1.0f);
    if (a.padding) {
        const double* pd = a.padding + (long)b * 4;
        if (!(pd[0] == 0.0 && pd[1] == 0.0 && pd[2] == 0.0 && pd[3] == 0.0)) {
            double hs = 1.0 - (pd[0] + pd[2]), vs = 1.0 - (pd[1] + pd[3]);
            x = (float)(((double)x - pd[0]) / hs);
            y = (float)(((double)y - pd[1]) / vs);
            z = (float)(((double)z - 0.) / hs);
        }
    }
    if (i == 0 && a.flag) {
        float fl = a.flag[(long)b * a.flag_fs];
        if (a.present) a.present[b] = sigmoid_f32(fl) <= 0.5f ? 0 : 1;
        if (a.raw_flag_out) a.raw_flag_out[b] = fl;
    }
    if (a.roi) {
        const RectD ro = a.roi[b];
        double xc = ro.x_center, yc = ro.y_center, w = ro.width, h = ro.height, rot = ro.rotation;
        if (!ro.normalized) {  // Rect::scaled(size, true): multiply by the reciprocal (types.rs:67)
            double sx = 1.0 / (double)a.image_size[2 * b], sy = 1.0 / (double)a.image_size[2 * b + 1];
            xc *= sx; yc *= sy; w *= sx; h *= sy;
        }
        float m00 = (float)cos(rot), m01 = (float)sin(rot), m10 = (float)(-sin(rot)), m11 = m00;
        x = __fsub_rn(x, 0.5f); y = __fsub_rn(y, 0.5f); z = __fsub_rn(z, 0.0f);
        float rz = __fmul_rn(z, 0.0f);
        float rx = __fadd_rn(__fadd_rn(__fmul_rn(x, m00), __fmul_rn(y, m10)), __fmul_rn(rz, 1.0f));
        float ry = __fadd_rn(__fadd_rn(__fmul_rn(x, m01), __fmul_rn(y, m11)), __fmul_rn(rz, 1.0f));
        float rzz = __fadd_rn(__fadd_rn(__fmul_rn(x, 0.0f), __fmul_rn(y, 0.0f)), __fmul_rn(rz, 1.0f));
        x = __fadd_rn(__fmul_rn(x, 0.f), rx);
        y = __fadd_rn(__fmul_rn(y, 0.f), ry);
        z = __fadd_rn(__fmul_rn(z, 1.f), rzz);
        x = (float)((double)x * w + xc);
        y = (float)((double)y * h + yc);
        z = (float)((double)z * w + 0.);
    }
    o[0] = x; o[1] = y; o[2] = z;
}

int launch_project(const ProjArgs& a, void* stream) {
    long n = (long)a.B * (a.n + a.n2);
    if (n > 0) hipLaunchKernelGGL(project_landmarks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mi
