// face_chip.hpp — the rectangle FaceEmbeddings::infer crops before it resizes to 112 x 112 (reference:
// /root/reference/src/face_detection_lite/face_embeddings.rs:54,101-109 with types.rs:162-165,219-225).  The arithmetic below is the only
// statement of the rule; the host entries (mi_face_chip_rect, mi_fe_infer_image in capi_embed.cpp) and chip_geom_kernel (preproc.hip) both go
// through it.
//
//   bbox = detection.bbox().scale((width, height)): each of xmin, ymin, xmax, ymax is the detection's f32 widened to f64, times the picture
//   size; Mat::roi {x: xmin as i32, y: ymin as i32, width: (xmax - xmin) as i32, height: (ymax - ymin) as i32} — the differences in f64, every
//   cast Rust's `as` (toward zero, saturating, NaN -> 0).  OpenCV refuses 0 <= x, 0 <= w, x + w <= cols (and rows likewise) when violated; the
//   reference then panics.  An empty rectangle (w or h of 0) passes Mat::roi and dies in the resize: invalid here as well.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_FACE_CHIP_HD __host__ __device__
#else
#define MI_FACE_CHIP_HD
#endif

namespace mi {

constexpr int kChipSize = 112;   // IMG_SIZE, face_embeddings.rs:20

// Rust's `f64 as i32`
MI_FACE_CHIP_HD inline int chip_as_i32(double v) {
    if (v != v) return 0;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return -2147483647 - 1;
    return static_cast<int>(v);
}

// bbox = {xmin, ymin, xmax, ymax} in absolute pixels -> rect = {x, y, w, h}; returns 1 when Mat::roi accepts it and it is not empty
MI_FACE_CHIP_HD inline int face_chip_rect_px(const double bbox[4], int width, int height, int rect[4]) {
    rect[0] = chip_as_i32(bbox[0]);
    rect[1] = chip_as_i32(bbox[1]);
    rect[2] = chip_as_i32(bbox[2] - bbox[0]);
    rect[3] = chip_as_i32(bbox[3] - bbox[1]);
    const long long x = rect[0], y = rect[1], w = rect[2], h = rect[3];
    return (x >= 0 && w > 0 && x + w <= width && y >= 0 && h > 0 && y + h <= height) ? 1 : 0;
}

// det = Detection.data: (xmin, ymin), (xmax, ymax) first, normalised
MI_FACE_CHIP_HD inline int face_chip_rect_det(const float* det, int width, int height, int rect[4]) {
    const double bbox[4] = {static_cast<double>(det[0]) * static_cast<double>(width), static_cast<double>(det[1]) * static_cast<double>(height),
                            static_cast<double>(det[2]) * static_cast<double>(width), static_cast<double>(det[3]) * static_cast<double>(height)};
    return face_chip_rect_px(bbox, width, height, rect);
}

}  // namespace mi
