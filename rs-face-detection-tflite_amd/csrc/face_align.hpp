// face_align.hpp — aligned face chips: the square ROI whose warp to 112 x 112 puts a face's eyes, nose tip and mouth corners onto the usual
// five ArcFace destination points.  NOT the reference's behaviour: FaceEmbeddings::infer crops the detector's box (face_chip.hpp) and that
// path keeps every bit.  The arithmetic below is the only statement of the rule; the host entries (mi_face_align_template, mi_face_align_points,
// mi_face_align_roi, mi_fe_infer_image_aligned in capi_embed.cpp) and align_geom_kernel (preproc.hip) both go through it.
//
//   A similarity transform (rotation, uniform scale, translation) image -> chip is a rotated square ROI warped to 112 x 112 with
//   keep_aspect_ratio = false: image_to_tensor(image, Some(Rect{cx, cy, side, side, rotation, normalized: false}), (112,112), false, (0,1),
//   false), which compute_geom / warp_px (preproc.hip) reproduce.  So the fit ends in a Rect and nothing else is new.
//
//   With p_i the image points, q_i the template points, m / mq their means and complex numbers for the plane, the least-squares optimum of
//   q ~ z p + t over proper similarities is z = (A + iB) / S,
//     A = sum (dx du + dy dv),  B = sum (dx dv - dy du),  S = sum (dx^2 + dy^2),  N = A^2 + B^2,
//   and its inverse, chip -> image, is p - m = (c + i d)(q - mq) with c = A S / N, d = -(B S / N).  The ROI is the image of the chip's
//   square: side = 112 |c + i d| = 112 S / sqrt(N), rotation = atan2(-B, A), centre = m + (c + i d)((56, 56) - mq).
//
//   Everything is f64, every sum sequential in index order from 0, no FMA (the build has -ffp-contract=off).
#pragma once

#include "kernels.hpp"   // RectD

#if defined(__HIPCC__)
#define MI_FACE_ALIGN_HD __host__ __device__
#else
#define MI_FACE_ALIGN_HD
#endif

namespace mi {

constexpr int kAlignPoints = 0, kAlignMesh = 1, kAlignDetection = 2;   // MI_ALIGN_POINTS / MI_ALIGN_MESH / MI_ALIGN_DETECTION
constexpr int kAlignMaxPoints = 5;
constexpr int kAlignMeshLandmarks = 468;

MI_FACE_ALIGN_HD inline bool align_finite(double v) { return v - v == 0.0; }   // false for NaN and for either infinity

// The template in chip pixels: image-left eye, image-right eye, nose tip, image-left mouth corner, image-right mouth corner.  The detector's
// key points have a mouth centre instead of the corners: its template is the first three rows plus the mean of the last two.
// Returns n (5, or 4 for kAlignDetection); 0 for a source that does not exist.
MI_FACE_ALIGN_HD inline int face_align_template(int source, double u[kAlignMaxPoints], double v[kAlignMaxPoints]) {
    const double tu[5] = {38.2946, 73.5318, 56.0252, 41.5493, 70.7299};
    const double tv[5] = {51.6963, 51.5014, 71.7366, 92.3655, 92.2041};
    if (source != kAlignPoints && source != kAlignMesh && source != kAlignDetection) return 0;
    for (int i = 0; i < 5; i++) { u[i] = tu[i]; v[i] = tv[i]; }
    if (source != kAlignDetection) return 5;
    u[3] = (tu[3] + tu[4]) / 2.0;
    v[3] = (tv[3] + tv[4]) / 2.0;
    u[4] = v[4] = 0.0;
    return 4;
}

// the ROI of an item that has no fit: the whole image, normalised (what face_roi_dev writes for a frame without a face)
MI_FACE_ALIGN_HD inline void face_align_default_roi(RectD* out) {
    out->x_center = 0.5; out->y_center = 0.5; out->width = 1.0; out->height = 1.0; out->rotation = 0.0;
    out->normalized = 1;
    out->pad_ = 0;
}

// (x_i, y_i): image pixels, (u_i, v_i): template points.  Returns 1 and the ROI, or 0 and the default ROI.
MI_FACE_ALIGN_HD inline int face_align_roi(const double* x, const double* y, int n, const double* u, const double* v, RectD* out) {
    face_align_default_roi(out);
    if (n < 2 || n > kAlignMaxPoints) return 0;
    for (int i = 0; i < n; i++)
        if (!(align_finite(x[i]) && align_finite(y[i]) && align_finite(u[i]) && align_finite(v[i]))) return 0;
    double mx = 0.0, my = 0.0, mu = 0.0, mv = 0.0;
    for (int i = 0; i < n; i++) { mx += x[i]; my += y[i]; mu += u[i]; mv += v[i]; }
    const double dn = static_cast<double>(n);
    mx = mx / dn; my = my / dn; mu = mu / dn; mv = mv / dn;
    double A = 0.0, B = 0.0, S = 0.0;
    for (int i = 0; i < n; i++) {
        const double dx = x[i] - mx, dy = y[i] - my, du = u[i] - mu, dv = v[i] - mv;
        A += dx * du + dy * dv;
        B += dx * dv - dy * du;
        S += dx * dx + dy * dy;
    }
    const double N = A * A + B * B;
    if (!(S > 0.0 && N > 0.0 && align_finite(S) && align_finite(N))) return 0;
    const double c = A * S / N, d = -(B * S / N);
    const double side = 112.0 * S / sqrt(N);
    const double rotation = atan2(-B, A);
    const double ex = 56.0 - mu, ey = 56.0 - mv;
    const double x_center = mx + (c * ex - d * ey), y_center = my + (d * ex + c * ey);
    if (!(align_finite(side) && side > 0.0 && align_finite(x_center) && align_finite(y_center))) return 0;
    out->x_center = x_center; out->y_center = y_center; out->width = side; out->height = side; out->rotation = rotation;
    out->normalized = 0;
    return 1;
}

// ---- point sources.  Every source ends in n f32 pixel points [n][2] in the template's order — what a kAlignPoints caller passes — so that
// an item fitted from its mesh or its detection and the same item fitted from mi_face_align_points' output are one computation.
//   kAlignPoints:    src = f32 [5][2], taken as they are
//   kAlignMesh:      src = landmarks f32 [468][3], normalised to the image: px = (double)lm.x * (double)width, py = (double)lm.y * (double)height;
//                    eyes = the midpoints (p33 + p133) / 2.0 and (p362 + p263) / 2.0 of the corners iris_landmark.rs:29-35 uses, nose tip =
//                    landmark 1, mouth corners = 61 and 291
//   kAlignDetection: src = a detection's 17 floats; key points 0..3 (left eye, right eye, nose tip, mouth centre) at d[4 + 2i], d[5 + 2i],
//                    px = (double)d[4 + 2i] * width, py = (double)d[5 + 2i] * height
// Returns n; 0 for a source that does not exist.
MI_FACE_ALIGN_HD inline int face_align_gather(int source, const float* src, int width, int height, float pts[kAlignMaxPoints][2]) {
    const double w = static_cast<double>(width), h = static_cast<double>(height);
    for (int i = 0; i < kAlignMaxPoints; i++) pts[i][0] = pts[i][1] = 0.f;
    if (source == kAlignPoints) {
        for (int i = 0; i < 5; i++) { pts[i][0] = src[2 * i]; pts[i][1] = src[2 * i + 1]; }
        return 5;
    }
    if (source == kAlignMesh) {
        const int eye[2][2] = {{33, 133}, {362, 263}};
        for (int e = 0; e < 2; e++) {
            const float* a = src + 3 * eye[e][0];
            const float* b = src + 3 * eye[e][1];
            const double ax = static_cast<double>(a[0]) * w, ay = static_cast<double>(a[1]) * h;
            const double bx = static_cast<double>(b[0]) * w, by = static_cast<double>(b[1]) * h;
            pts[e][0] = static_cast<float>((ax + bx) / 2.0);
            pts[e][1] = static_cast<float>((ay + by) / 2.0);
        }
        const int single[3] = {1, 61, 291};
        for (int i = 0; i < 3; i++) {
            const float* a = src + 3 * single[i];
            pts[2 + i][0] = static_cast<float>(static_cast<double>(a[0]) * w);
            pts[2 + i][1] = static_cast<float>(static_cast<double>(a[1]) * h);
        }
        return 5;
    }
    if (source == kAlignDetection) {
        for (int i = 0; i < 4; i++) {
            pts[i][0] = static_cast<float>(static_cast<double>(src[4 + 2 * i]) * w);
            pts[i][1] = static_cast<float>(static_cast<double>(src[5 + 2 * i]) * h);
        }
        return 4;
    }
    return 0;
}

// the fit of n f32 pixel points (widened to f64) against the template of `source`; 0 and the default ROI when n is not the template's n
MI_FACE_ALIGN_HD inline int face_align_roi_points(const float pts[][2], int n, int source, RectD* out) {
    double u[kAlignMaxPoints], v[kAlignMaxPoints], x[kAlignMaxPoints], y[kAlignMaxPoints];
    const int tn = face_align_template(source, u, v);
    if (tn == 0 || n != tn) { face_align_default_roi(out); return 0; }
    for (int i = 0; i < n; i++) { x[i] = static_cast<double>(pts[i][0]); y[i] = static_cast<double>(pts[i][1]); }
    return face_align_roi(x, y, n, u, v, out);
}

}  // namespace mi
