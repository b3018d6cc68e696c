// preproc.hpp — device-side transform::image_to_tensor (/root/reference/src/face_detection_lite/transform.rs:188-309),
// for one image or for a batch of (frame, ROI) items whose ROIs already live in device memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/mi_face.h"
#include "kernels.hpp"

namespace mi {

// Everything image_to_tensor derives from (image size, ROI, output size, keep_aspect): computed once per item, on the
// host for the single-image entry points and by pre_geom_kernel on the device for batches (same code).
struct PreGeom {
    double Minv[9];             // dst -> src homography of the ROI warp (cv::getPerspectiveTransform + invert)
    double pad_x, pad_y;        // ImageTensor.padding = (pad_x, pad_y, pad_x, pad_y)
    int warp_w, warp_h, bw0;    // warpPerspective target size, OpenCV tile width
    int stage1;                 // 0: none, 1: border only (same-size resize = copy), 2: border + resize to (new_w, new_h)
    int pad_h, pad_v, new_w, new_h;
    int stage2;                 // 1: resize to the output size, 0: already there
    int valid;                  // 0: item skipped (no face / degenerate ROI): output tensor is zero-filled
};

struct PreItems {               // batch description (device pointers unless stated)
    const uint8_t* frames;      // [n_frames][height][stride] RGB u8
    long frame_bytes;           // bytes between frames
    int width, height, stride;
    const RectD* rois;          // [N] or null (whole image)
    const int* roi_valid;       // [N] or null
    const int* flip;            // [N] or null
    int items_per_frame;        // item i reads frame i / items_per_frame
    const int* item_frame;      // [N / items_per_frame] or null: item i reads frame item_frame[i / items_per_frame] instead (mi_pipeline_run_faces:
                                // several items per frame, compacted); a -1 entry belongs to an item whose roi_valid is 0 and is never used
    int N, out_w, out_h, keep_aspect;
    double range_min, range_max;
};

// geometry for N items -> d_geom[N], d_padding[N][4] (may be null)
void launch_pre_geom(const PreItems& it, PreGeom* d_geom, double* d_padding, hipStream_t s);
// ... of N whole pictures of one size (no ROI), computed on the host and uploaded (synchronous: the caller caches it per (width, height, N))
void upload_whole_image_geom(int width, int height, int out_w, int out_h, bool keep_aspect, int N, PreGeom* d_geom, double* d_padding, hipStream_t s);
// warp -> (border, resize) -> resize -> flip -> normalise, fused per output pixel; out f32 [N][out_h][out_w][3]
void launch_pre_tensor(const PreItems& it, const PreGeom* d_geom, float* d_out, hipStream_t s);

// Single-image convenience used by the mi_*_infer_image entry points: uploads the host image into d_scratch
// (>= stride*height + 256 bytes + sizeof(PreGeom)), runs the two kernels with N = 1, returns the padding on the host.
void image_to_tensor_device(const uint8_t* rgb_host, int width, int height, int stride, const mi_rect* roi, int out_w, int out_h,
                            bool keep_aspect_ratio, double range_min, double range_max, bool flip_horizontal, float* d_out,
                            double padding[4], void* d_scratch, hipStream_t stream);
// The same without a host synchronisation and without small uploads: geometry and flip flag travel as kernel arguments, the picture
// is copied into d_img (>= stride * height bytes) on `stream`.  `rgb_host` must stay valid until the caller has synchronised `stream`.
void image_to_tensor_enqueue(const uint8_t* rgb_host, int width, int height, int stride, const mi_rect* roi, int out_w, int out_h,
                             bool keep_aspect_ratio, double range_min, double range_max, bool flip_horizontal, float* d_out,
                             double padding[4], uint8_t* d_img, hipStream_t stream);
// ... for a picture that is in device memory already (the streamed JPEG entries: the decoder's RGB output never visits the host)
void image_to_tensor_enqueue_device(const uint8_t* d_img, int width, int height, int stride, const mi_rect* roi, int out_w, int out_h,
                                    bool keep_aspect_ratio, double range_min, double range_max, bool flip_horizontal, float* d_out,
                                    double padding[4], hipStream_t stream);
size_t image_to_tensor_scratch_bytes(int width, int height, int stride, const mi_rect* roi, int out_w, int out_h, bool keep_aspect_ratio);

// Device-side ROI maths between pipeline stages (face_landmark.rs:180-198, iris_landmark.rs:268-292).
void launch_face_rois(const float* d_dets /*[B][cap][17]*/, const int* d_counts, int B, int cap, int image_w, int image_h,
                      RectD* d_rois, int* d_valid, hipStream_t s);
void launch_iris_rois(const float* d_landmarks /*[B][468][3]*/, const int* d_present, int B, int image_w, int image_h,
                      RectD* d_rois /*[B][2] left,right*/, int* d_valid /*[B][2]*/, int* d_flip /*[B][2]*/, hipStream_t s);

// The item list of mi_pipeline_run_faces (face_items.hpp states the rule), from what the detector's post-processing launch left in device memory:
// one launch of one workgroup, no atomics.  Slot j < n_items[0] gets its frame, its face, face_detection_to_roi of that face and valid = 1 (0 for a
// box that is not normalised); the slots behind get -1 / -1 / valid = 0 (their ROI is not written: every reader asks `valid` first).
struct FaceItemsArgs {
    const float* dets;      // [B][max_faces][17]
    const int* counts;      // [B]
    int B, max_faces, max_items, image_w, image_h;
    int* item_frame;        // [max_items]
    int* item_face;         // [max_items]
    int* n_items;           // [2]
    RectD* rois;            // [max_items]
    int* valid;             // [max_items]
};
void launch_face_items(const FaceItemsArgs& a, hipStream_t s);

// The face chips of FaceEmbeddings::infer (face_embeddings.rs:54-55): crop_image_to_bbox, then image_to_tensor(crop, None, (112, 112), false,
// (0, 1), false) — a warpPerspective of the WHOLE crop, so BORDER_CONSTANT 0 applies at the crop's edge and no pixel next to the box is sampled.
// The crop is the picture the warp reads: source pointer at the crop's origin, the crop's own width and height, the frame's stride.
struct ChipGeom {
    PreGeom g;              // compute_geom(crop width, crop height, no ROI, 112 x 112, keep_aspect = false); g.valid = 0: the chip is zeros
    int x, y, w, h;         // the crop (face_chip.hpp)
};
struct ChipItems {              // device pointers
    const uint8_t* frames;      // [batch][height][stride] RGB u8
    long frame_bytes;
    int batch, width, height, stride;
    const float* faces;         // [batch][max_faces][17]
    int max_faces;
    const int* item_frame;      // [N]: -1 = unused slot
    const int* item_face;       // [N]
    int N;
};
// one geometry step per item (eight lanes each): rectangle of faces[item_frame][item_face] and its homography; valid[i] = 0 for an unused
// slot, an index outside the arrays or a rectangle Mat::roi refuses — neither the frame nor the detection of such an item is read
void launch_chip_geom(const ChipItems& it, ChipGeom* d_geom, int* d_valid, hipStream_t s);
// one thread per output pixel; out f32 [N][112][112][3], zeros for an invalid item
void launch_chip_tensor(const ChipItems& it, const ChipGeom* d_geom, float* d_out, hipStream_t s);
// The same for ONE crop whose rectangle the host has checked: the geometry (same code, on the host) travels as a kernel argument.  d_crop is
// the crop's first pixel, rows `stride` bytes apart.
void chip_tensor_enqueue_one(const uint8_t* d_crop, int w, int h, int stride, float* d_out, hipStream_t s);

// Aligned face chips (face_align.hpp; NOT the reference's chips): per item a least-squares similarity fit of its points to the five-point
// template, as a rotated square ROI of the WHOLE frame warped to 112 x 112 — image_to_tensor(frame, Some(roi), (112,112), false, (0,1), false),
// so BORDER_CONSTANT 0 applies at the frame's edge.
struct AlignItems {             // device pointers
    const uint8_t* frames;      // [batch][height][stride] RGB u8
    long frame_bytes;
    int batch, width, height, stride;
    int source;                 // kAlignPoints / kAlignMesh / kAlignDetection
    const float* src;           // points [N][5][2] / landmarks [N][468][3] / faces [batch][max_faces][17]
    const int* gate;            // point_valid [N] or null / present [N] / unused
    int max_faces;              // kAlignDetection only
    const int* item_frame;      // [N]: -1 = unused slot
    const int* item_face;       // [N], kAlignDetection only
    int N;
};
// one geometry step per item (eight lanes each): gather, fit and the ROI's homography; d_rois may be null.  valid[i] = 0 for an unused slot,
// an index outside the arrays, a gate of 0 or a fit that fails — neither the frame nor any operand row of such an item is read
void launch_align_geom(const AlignItems& it, PreGeom* d_geom, RectD* d_rois, int* d_valid, hipStream_t s);
// one thread per output pixel; out f32 [N][112][112][3], zeros for an invalid item
void launch_aligned_chips(const AlignItems& it, const PreGeom* d_geom, float* d_out, hipStream_t s);
// The same for ONE picture in device memory whose ROI the host has fitted: the geometry (same code, on the host) travels as a kernel argument.
void aligned_chip_enqueue_one(const uint8_t* d_img, int width, int height, int stride, const RectD& roi, float* d_out, hipStream_t s);

}  // namespace mi
