// capi_render.cpp — the device renderer's entries.
#include "capi_internal.hpp"

using namespace mi::capi;

namespace {
constexpr size_t kEyeFloats = 2 * (MI_NUM_EYE_LANDMARKS + MI_NUM_IRIS_LANDMARKS) * 3;   // both eyes of a face: contour + iris landmarks

// everything mi_render_annotations and mi_render_faces check about their pictures, before any device is touched
void render_check_canvas(const uint8_t* frames, int batch, int width, int height, int stride, const uint8_t* out, int out_channels, int out_stride,
                         int mem) {
    require(frames && out, "null argument");
    require_mem(mem);
    require(batch > 0 && width > 0 && height > 0, "bad frame geometry");
    require(stride >= 3 * static_cast<long>(width), "stride is smaller than 3 * width");
    require(out_channels == 3 || out_channels == 4, "out_channels must be 3 (RGB) or 4 (RGBA)");
    require(out_stride >= out_channels * static_cast<long>(width), "out_stride is smaller than out_channels * width");
    if (out == frames) {
        require(out_channels == 3 && out_stride == stride, "out may be frames (in place) only with out_channels 3 and out_stride == stride");
        return;
    }
    const uint8_t* in_end = frames + frames_bytes(batch, height, stride, static_cast<size_t>(3) * width);
    const uint8_t* out_end = out + frames_bytes(batch, height, out_stride, static_cast<size_t>(out_channels) * width);
    require(out_end <= frames || in_end <= out, "out overlaps frames (only out == frames, in place, is an alias this call accepts)");
}

// The part the two render entries share: staging of the pictures for host callers (tight rows on the device), the canvas phase, the
// draw phase (`draw(canvas, d_skipped, stream)` stages its own operands and launches), the way back.  Rows travel back without
// their padding: the bytes of the caller's rows beyond out_channels * width are never written.
template <class Draw>
void render_run(int device, const uint8_t* frames, int batch, int width, int height, int stride, uint8_t* out, int out_channels, int out_stride,
                int* skipped, int mem, void* stream, bool always_wait, Draw draw) {
    select_device(device, "no such HIP device (the renderer runs on the GPU; no CPU fallback exists)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceBuf b_frames, b_out, b_skipped;
    mi::RenderCanvas cv{frames, out, batch, width, height, stride, out_stride, out_channels};
    const size_t rows = static_cast<size_t>(batch) * height, in_row = static_cast<size_t>(3) * width, out_row = static_cast<size_t>(out_channels) * width;
    if (mem == MI_MEM_HOST) {
        auto* d_frames = b_frames.as<uint8_t>(rows * in_row);
        mi::hip_check(hipMemcpy2DAsync(d_frames, in_row, frames, stride, in_row, rows, hipMemcpyHostToDevice, s), "H2D frames");
        cv.frames = d_frames;
        cv.stride = static_cast<int>(in_row);
        cv.out = out == frames ? d_frames : b_out.as<uint8_t>(rows * out_row);
        cv.out_stride = static_cast<int>(out_row);
    }
    int* d_skipped = skipped ? result_target(b_skipped, skipped, batch, mem) : nullptr;
    check_launch(mi::launch_render_canvas(cv, s), "render canvas");
    draw(cv, d_skipped, s);
    if (mem == MI_MEM_HOST) {
        mi::hip_check(hipMemcpy2DAsync(out, out_stride, cv.out, out_row, out_row, rows, hipMemcpyDeviceToHost, s), "D2H picture");
    }
    hand_back(skipped, d_skipped, batch, mem, s, "D2H skipped");
    finish(mem, stream && !always_wait, s);
}
}  // namespace

extern "C" {

int mi_render_annotations(int device, const uint8_t* frames, int batch, int width, int height, int stride, const mi_annotation* anns, int n_anns,
                          const double* coords, long coords_per_frame, uint8_t* out, int out_channels, int out_stride, int* skipped, int mem,
                          void* stream) {
    return guarded([&] {
        render_check_canvas(frames, batch, width, height, stride, out, out_channels, out_stride, mem);
        require(n_anns >= 0 && coords_per_frame >= 0 && (n_anns == 0 || anns), "bad annotation list");
        bool reads = false;
        for (int a = 0; a < n_anns; a++) {
            const mi_annotation& A = anns[a];
            require(A.kind >= MI_ANN_POINTS && A.kind <= MI_ANN_FILLED_RECTS, "annotation kind must be one of MI_ANN_*");
            require(A.first >= 0 && A.count >= 0, "annotation with a negative first / count");
            const long per_item = A.kind == MI_ANN_POINTS ? 2 : 4;
            require(A.first + A.count * per_item <= coords_per_frame, "annotation reads beyond coords_per_frame");
            reads = reads || A.count > 0;
        }
        require(!reads || coords, "null argument");
        DeviceBuf b_anns, b_coords;
        render_run(device, frames, batch, width, height, stride, out, out_channels, out_stride, skipped, mem, stream, true,
                   [&](const mi::RenderCanvas& cv, int* d_skipped, hipStream_t s) {
                       // (the list itself is host memory whatever `mem` says, and never an empty allocation)
                       const size_t ann_bytes = sizeof(mi_annotation) * n_anns;
                       auto* d_anns = static_cast<mi_annotation*>(b_anns.get(ann_bytes + 16));
                       if (n_anns) mi::hip_check(hipMemcpyAsync(d_anns, anns, ann_bytes, hipMemcpyHostToDevice, s), "H2D annotations");
                       const double* d_coords = reads ? stage(b_coords, coords, static_cast<size_t>(coords_per_frame) * batch, mem, s, "H2D coords") : coords;
                       check_launch(mi::launch_render_annotations(cv, d_anns, n_anns, d_coords, coords_per_frame, d_skipped, s), "render");
                   });
    });
}

int mi_render_faces(int device, const uint8_t* frames, int batch, int width, int height, int stride, const mi_detection* faces, const int* face_counts,
                    int faces_per_frame, const float* landmarks, const int* present, const float* eyes, const mi_render_style* style, uint8_t* out,
                    int out_channels, int out_stride, int* skipped, int mem, void* stream) {
    return guarded([&] {
        render_check_canvas(frames, batch, width, height, stride, out, out_channels, out_stride, mem);
        require(style, "null argument");
        require(!faces || (face_counts && faces_per_frame > 0), "faces need face_counts and faces_per_frame > 0");
        DeviceBuf b_faces, b_counts, b_landmarks, b_present, b_eyes;
        render_run(device, frames, batch, width, height, stride, out, out_channels, out_stride, skipped, mem, stream, false,
                   [&](const mi::RenderCanvas& cv, int* d_skipped, hipStream_t s) {
                       const size_t B = static_cast<size_t>(batch);
                       const char* what = "H2D results";
                       auto* d_faces = stage(b_faces, faces, B * (faces ? faces_per_frame : 0), mem, s, what);
                       auto* d_counts = stage(b_counts, faces ? face_counts : nullptr, B, mem, s, what);
                       auto* d_landmarks = stage(b_landmarks, landmarks, B * MI_NUM_FACE_LANDMARKS * 3, mem, s, what);
                       auto* d_present = stage(b_present, present, B, mem, s, what);
                       auto* d_eyes = stage(b_eyes, eyes, B * kEyeFloats, mem, s, what);
                       check_launch(mi::launch_render_faces(cv, d_faces, d_counts, faces_per_frame, d_landmarks, d_present, d_eyes, *style, d_skipped, s), "render");
                   });
    });
}

int mi_render_face_items(int device, const uint8_t* frames, int batch, int width, int height, int stride, const mi_detection* faces,
                         const int* face_counts, int max_faces, const int* item_frame, const int* n_items, int max_items, const float* landmarks,
                         const int* present, const float* eyes, const mi_render_items_style* style, uint8_t* out, int out_channels, int out_stride,
                         int* skipped, int mem, void* stream) {
    return guarded([&] {
        render_check_canvas(frames, batch, width, height, stride, out, out_channels, out_stride, mem);
        require(style, "null argument");
        require(!faces || (face_counts && max_faces >= 1 && max_faces <= 16), "faces need face_counts and max_faces in 1..16");
        require(max_items >= 1 && max_items <= 32767, "max_items must be 1..32767");
        require((item_frame != nullptr) == (n_items != nullptr), "item_frame and n_items come together");
        require(item_frame || !(landmarks || eyes), "landmarks and eyes need item_frame and n_items");
        // iris_landmark.rs:342-344: "oval_color requires a valid image_size arg"
        require(!style->draw_iris_oval || (width >= 2 && height >= 2), "draw_iris_oval needs width >= 2 and height >= 2");
        DeviceBuf b_faces, b_counts, b_item_frame, b_n_items, b_landmarks, b_present, b_eyes;
        render_run(device, frames, batch, width, height, stride, out, out_channels, out_stride, skipped, mem, stream, false,
                   [&](const mi::RenderCanvas& cv, int* d_skipped, hipStream_t s) {
                       const size_t B = static_cast<size_t>(batch), M = static_cast<size_t>(max_items);
                       const char* what = "H2D results";
                       auto* d_faces = stage(b_faces, faces, B * (faces ? max_faces : 0), mem, s, what);
                       auto* d_counts = stage(b_counts, faces ? face_counts : nullptr, B, mem, s, what);
                       auto* d_item_frame = stage(b_item_frame, item_frame, M, mem, s, what);
                       auto* d_n_items = stage(b_n_items, n_items, 1, mem, s, what);
                       auto* d_landmarks = stage(b_landmarks, landmarks, M * MI_NUM_FACE_LANDMARKS * 3, mem, s, what);
                       auto* d_present = stage(b_present, item_frame ? present : nullptr, M, mem, s, what);
                       auto* d_eyes = stage(b_eyes, eyes, M * kEyeFloats, mem, s, what);
                       check_launch(mi::launch_render_face_items(cv, d_faces, d_counts, max_faces, d_item_frame, d_n_items, max_items, d_landmarks, d_present,
                                                                 d_eyes, *style, d_skipped, s),
                                    "render");
                   });
    });
}

}  // extern "C"
