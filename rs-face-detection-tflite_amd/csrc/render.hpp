// render.hpp — device-side render_to_image (render.rs:361-479) over a batch: the canvas phase (RGB -> RGBA / RGB) and the draw
// phase (one workgroup per frame, annotations in list order).  Kernels in render_kernels.hip; the C entries are in capi_render.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/mi_face.h"

namespace mi {

// Coordinates a line may have after the `as i32` cast (render.rs:435-438): inside this bound every f32 value of imageproc's
// Bresenham walk is a half-integer below 2^23, i.e. exact, and the closed-form skip of the off-canvas prefix is exact too.
constexpr int kRenderCoordLimit = 1 << 20;

struct RenderCanvas {       // device pointers
    const uint8_t* frames;  // [batch][height][stride] RGB u8
    uint8_t* out;           // [batch][height][out_stride], `channels` bytes per pixel (may be `frames`: in place, channels 3)
    int batch, width, height, stride, out_stride, channels;
};

// Canvas phase: to_rgba8 (render.rs:365) or a plain RGB copy.  Nothing is launched when out == frames.
hipError_t launch_render_canvas(const RenderCanvas& cv, hipStream_t s);
// Draw phase of mi_render_annotations: d_anns [n_anns], d_coords [batch][coords_per_frame], d_skipped [batch] or null.
hipError_t launch_render_annotations(const RenderCanvas& cv, const mi_annotation* d_anns, int n_anns, const double* d_coords,
                                     long coords_per_frame, int* d_skipped, hipStream_t s);
// Draw phase of mi_render_faces: the items are generated from the result arrays (any group may be null).
hipError_t launch_render_faces(const RenderCanvas& cv, const mi_detection* d_faces, const int* d_face_counts, int faces_per_frame,
                               const float* d_landmarks, const int* d_present, const float* d_eyes, const mi_render_style& style,
                               int* d_skipped, hipStream_t s);
// Draw phase of mi_render_face_items: the frame's detections, then the mesh, eyes and irises of every item of the frame (the run of the frame's
// index in d_item_frame[0, clamp(d_n_items[0], 0, max_items)), found on the device).  d_faces with d_face_counts, d_item_frame with d_n_items,
// d_landmarks, d_present and d_eyes may be null.
hipError_t launch_render_face_items(const RenderCanvas& cv, const mi_detection* d_faces, const int* d_face_counts, int max_faces,
                                    const int* d_item_frame, const int* d_n_items, int max_items, const float* d_landmarks, const int* d_present,
                                    const float* d_eyes, const mi_render_items_style& style, int* d_skipped, hipStream_t s);

}  // namespace mi
