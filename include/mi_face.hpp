// mi_face.hpp — C++17 host-side mirror of the reference crate's public API over the C ABI (mi_face.h).
//
// The reference is compiled (Rust) code; no Rust toolchain exists in this image, so the host side above the C ABI is
// written in C++ with the reference's names, argument meaning and error behaviour:
//   FaceDetection::{new, infer}   /root/reference/src/face_detection_lite/face_detection.rs:153,205
//   FaceLandmark::{new, infer}    face_landmark.rs:208,232        face_detection_to_roi  face_landmark.rs:180
//   IrisLandmark::{new, infer}    iris_landmark.rs:142,158        iris_roi_from_face_landmarks iris_landmark.rs:268
//   Detection / Rect / Landmark / BBox / IrisResults             types.rs:24-246, iris_landmark.rs:115-129
// `anyhow::Error` (and the reference's panics) become `mi_face::Error`; `Option<T>` becomes `std::optional<T>`;
// `&Mat` (8UC3 RGB, utils.rs:8-21) becomes the non-owning `Image` view.  Header-only; link with -lmiface.
#pragma once

#include <array>
#include <algorithm>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "mi_face.h"

namespace mi_face {

class Error : public std::runtime_error {
   public:
    Error(int code, const std::string& msg) : std::runtime_error(msg), code_(code) {}
    int code() const { return code_; }

   private:
    int code_;
};

namespace detail {
inline void check(int rc) {
    if (rc != MI_OK) throw Error(rc, mi_last_error());
}
}  // namespace detail

// types.rs:24-36
struct Rect {
    double x_center = 0.5, y_center = 0.5, width = 1.0, height = 1.0, rotation = 0.0;
    bool normalized = true;
    mi_rect c() const { return mi_rect{x_center, y_center, width, height, rotation, normalized ? 1 : 0}; }
    static Rect from(const mi_rect& r) { return Rect{r.x_center, r.y_center, r.width, r.height, r.rotation, r.normalized != 0}; }
};

// types.rs:99-174 (the parts callers use)
struct BBox {
    double xmin, ymin, xmax, ymax;
    double width() const { return xmax - xmin; }
    double height() const { return ymax - ymin; }
    BBox scale(std::pair<double, double> size) const { return BBox{xmin * size.first, ymin * size.second, xmax * size.first, ymax * size.second}; }   // types.rs:162-165
};

// types.rs:176-187
struct Landmark {
    double x, y, z;
};

// types.rs:189-246: data is [8][2] = (xmin,ymin), (xmax,ymax), 6 keypoints
struct Detection {
    std::array<float, 16> data{};
    float score = 0.f;
    std::size_t keypoint_count() const { return 6; }
    std::pair<float, float> keypoint(std::size_t k) const { return {data[2 * (k + 2)], data[2 * (k + 2) + 1]}; }
    BBox bbox() const { return BBox{data[0], data[1], data[2], data[3]}; }
};

// iris_landmark.rs:115-129
struct IrisResults {
    std::vector<Landmark> contour;  // 71
    std::vector<Landmark> iris;     // 5
    std::vector<Landmark> eyeball_contour() const { return std::vector<Landmark>(contour.begin(), contour.begin() + 15); }
};

// face_detection.rs:117-123
enum class FaceDetectionModel { FrontCamera = 0, BackCamera = 1, Short = 2, Full = 3, FullSparse = 4 };

// Stand-in for `&opencv::core::Mat` holding 8UC3 RGB pixels (utils.rs:8-21); does not own the pixels.
struct Image {
    const std::uint8_t* rgb;
    int width, height;
    int stride;  // bytes per row
};

class FaceDetection {
   public:
    // FaceDetection::new(model_type, model_path): model_path is a DIRECTORY, default "./models" (face_detection.rs:157-161)
    explicit FaceDetection(FaceDetectionModel model_type, std::optional<std::string> model_path = std::nullopt, int device = 0) {
        detail::check(mi_fd_create(static_cast<int>(model_type), model_path ? model_path->c_str() : nullptr, device, &h_));
    }
    ~FaceDetection() { mi_fd_free(h_); }
    FaceDetection(const FaceDetection&) = delete;
    FaceDetection& operator=(const FaceDetection&) = delete;

    // FaceDetection::infer(&Mat, Option<Rect>) -> Vec<Detection> (face_detection.rs:205-267)
    std::vector<Detection> infer(const Image& image, std::optional<Rect> roi = std::nullopt) const {
        std::vector<mi_detection> out(256);
        int n = 0;
        mi_rect r{};
        if (roi) r = roi->c();
        for (;;) {  // the reference returns every detection: when more were found than fit, ask again with that capacity
            detail::check(mi_fd_infer_image(h_, image.rgb, image.width, image.height, image.stride, roi ? &r : nullptr, out.data(),
                                            static_cast<int>(out.size()), &n));
            if (n <= static_cast<int>(out.size())) break;
            out.resize(static_cast<std::size_t>(n));
        }
        std::vector<Detection> dets(static_cast<std::size_t>(n));
        for (std::size_t i = 0; i < dets.size(); i++) {
            for (int k = 0; k < 16; k++) dets[i].data[k] = out[i].data[k];
            dets[i].score = out[i].score;
        }
        return dets;
    }
    // infer() over a batch of equally sized frames in one call (mi_fd_infer_images): `frames` = batch x height rows of `stride`
    // bytes, host memory; rois empty (whole frames) or one per frame.  Up to cap_per_frame detections per frame are returned.
    std::vector<std::vector<Detection>> infer_batch(const std::uint8_t* frames, int batch, int width, int height, int stride,
                                                    const std::vector<Rect>& rois = {}, int cap_per_frame = 64) const {
        if (batch < 1 || cap_per_frame < 1) throw std::invalid_argument("infer_batch: batch and cap_per_frame must be positive");
        if (!rois.empty() && rois.size() != static_cast<std::size_t>(batch))   // (the C side reads `batch` entries)
            throw std::invalid_argument("infer_batch: rois must be empty or hold one entry per frame");
        std::vector<mi_detection> out(static_cast<std::size_t>(batch) * cap_per_frame);
        std::vector<int> counts(static_cast<std::size_t>(batch));
        std::vector<mi_rect> r;
        for (const Rect& x : rois) r.push_back(x.c());
        detail::check(mi_fd_infer_images(h_, frames, batch, width, height, stride, r.empty() ? nullptr : r.data(), out.data(), cap_per_frame,
                                         counts.data(), MI_MEM_HOST, nullptr));
        std::vector<std::vector<Detection>> res(static_cast<std::size_t>(batch));
        for (int b = 0; b < batch; b++)
            for (int i = 0; i < std::min(counts[static_cast<std::size_t>(b)], cap_per_frame); i++) {
                Detection d;
                const mi_detection& m = out[static_cast<std::size_t>(b) * cap_per_frame + i];
                for (int k = 0; k < 16; k++) d.data[k] = m.data[k];
                d.score = m.score;
                res[static_cast<std::size_t>(b)].push_back(d);
            }
        return res;
    }
    // convert_image_to_mat + infer for a stream of encoded pictures (utils.rs:8-21, face_detection.rs:205): submit_jpeg decodes the entropy-coded
    // data on this thread while the device still runs the other slot's picture and queues the rest; collect_jpeg returns that slot's detections
    void submit_jpeg(int slot, const std::uint8_t* bytes, std::size_t nbytes, int cap = 64) const { detail::check(mi_fd_submit_jpeg(h_, slot, bytes, nbytes, cap)); }
    std::vector<Detection> collect_jpeg(int slot, int cap = 64, int* width = nullptr, int* height = nullptr) const {
        std::vector<mi_detection> out(static_cast<std::size_t>(cap));
        int n = 0;
        detail::check(mi_fd_collect_jpeg(h_, slot, out.data(), cap, &n, width, height));
        std::vector<Detection> dets(static_cast<std::size_t>(std::min(n, cap)));
        for (std::size_t i = 0; i < dets.size(); i++) {
            for (int k = 0; k < 16; k++) dets[i].data[k] = out[i].data[k];
            dets[i].score = out[i].score;
        }
        return dets;
    }
    mi_fd* handle() const { return h_; }

   private:
    mi_fd* h_ = nullptr;
};

class FaceLandmark {
   public:
    // FaceLandmark::new(model_path): FILE path, default "./models/face_landmark.tflite" (face_landmark.rs:211-215)
    explicit FaceLandmark(std::optional<std::string> model_path = std::nullopt, int device = 0) {
        detail::check(mi_fl_create(model_path ? model_path->c_str() : nullptr, device, &h_));
    }
    ~FaceLandmark() { mi_fl_free(h_); }
    FaceLandmark(const FaceLandmark&) = delete;
    FaceLandmark& operator=(const FaceLandmark&) = delete;

    // FaceLandmark::infer(&Mat, Option<Rect>) -> Vec<Landmark>; empty when the face flag fails (face_landmark.rs:292-296)
    std::vector<Landmark> infer(const Image& image, std::optional<Rect> roi = std::nullopt) const {
        std::vector<mi_landmark> out(MI_NUM_FACE_LANDMARKS);
        int n = 0;
        mi_rect r{};
        if (roi) r = roi->c();
        detail::check(mi_fl_infer_image(h_, image.rgb, image.width, image.height, image.stride, roi ? &r : nullptr, out.data(),
                                        MI_NUM_FACE_LANDMARKS, &n));
        std::vector<Landmark> lm(static_cast<std::size_t>(n));
        for (std::size_t i = 0; i < lm.size(); i++) lm[i] = Landmark{out[i].x, out[i].y, out[i].z};
        return lm;
    }

    // infer() over a batch (mi_fl_infer_images): `frames` = batch x height rows of `stride` bytes, host memory; item i reads frame
    // i / items_per_frame with ROI rois[i] (rois empty: whole frames, items_per_frame 1).  One entry per item; empty where the
    // face flag fails, like infer().
    std::vector<std::vector<Landmark>> infer_batch(const std::uint8_t* frames, int batch, int width, int height, int stride,
                                                   const std::vector<Rect>& rois = {}, int items_per_frame = 1) const {
        if (batch < 1 || items_per_frame < 1) throw std::invalid_argument("infer_batch: batch and items_per_frame must be positive");
        const std::size_t n = static_cast<std::size_t>(batch) * items_per_frame;
        if (rois.empty() ? items_per_frame != 1 : rois.size() != n) throw std::invalid_argument("infer_batch: rois must hold one entry per item");
        std::vector<mi_rect> r;
        for (const Rect& x : rois) r.push_back(x.c());
        std::vector<float> lm(n * 3 * MI_NUM_FACE_LANDMARKS);
        std::vector<int> present(n);
        detail::check(mi_fl_infer_images(h_, frames, batch, width, height, stride, r.empty() ? nullptr : r.data(), items_per_frame, lm.data(),
                                         present.data(), nullptr, MI_MEM_HOST, nullptr));
        std::vector<std::vector<Landmark>> res(n);
        for (std::size_t i = 0; i < n; i++)
            if (present[i])
                for (int k = 0; k < MI_NUM_FACE_LANDMARKS; k++) {
                    const float* v = &lm[(i * MI_NUM_FACE_LANDMARKS + k) * 3];
                    res[i].push_back(Landmark{v[0], v[1], v[2]});
                }
        return res;
    }

   private:
    mi_fl* h_ = nullptr;
};

class IrisLandmark {
   public:
    explicit IrisLandmark(std::optional<std::string> model_path = std::nullopt, int device = 0) {
        detail::check(mi_iris_create(model_path ? model_path->c_str() : nullptr, device, &h_));
    }
    ~IrisLandmark() { mi_iris_free(h_); }
    IrisLandmark(const IrisLandmark&) = delete;
    IrisLandmark& operator=(const IrisLandmark&) = delete;

    // IrisLandmark::infer(&Mat, Option<Rect>, Option<bool>) -> IrisResults (iris_landmark.rs:158-248)
    IrisResults infer(const Image& image, std::optional<Rect> roi = std::nullopt, std::optional<bool> is_right_eye = std::nullopt) const {
        mi_landmark c[MI_NUM_EYE_LANDMARKS], i5[MI_NUM_IRIS_LANDMARKS];
        mi_rect r{};
        if (roi) r = roi->c();
        detail::check(mi_iris_infer_image(h_, image.rgb, image.width, image.height, image.stride, roi ? &r : nullptr,
                                          is_right_eye.value_or(false) ? 1 : 0, c, i5));
        IrisResults res;
        for (const auto& v : c) res.contour.push_back(Landmark{v.x, v.y, v.z});
        for (const auto& v : i5) res.iris.push_back(Landmark{v.x, v.y, v.z});
        return res;
    }

    // infer() over a batch (mi_iris_infer_images): item i reads frame i / items_per_frame with ROI rois[i] and flip is_right_eye[i]
    // (empty: no flips); rois empty: whole frames, items_per_frame 1.
    std::vector<IrisResults> infer_batch(const std::uint8_t* frames, int batch, int width, int height, int stride, const std::vector<Rect>& rois = {},
                                         const std::vector<bool>& is_right_eye = {}, int items_per_frame = 1) const {
        if (batch < 1 || items_per_frame < 1) throw std::invalid_argument("infer_batch: batch and items_per_frame must be positive");
        const std::size_t n = static_cast<std::size_t>(batch) * items_per_frame;
        if (rois.empty() ? items_per_frame != 1 : rois.size() != n) throw std::invalid_argument("infer_batch: rois must hold one entry per item");
        if (!is_right_eye.empty() && is_right_eye.size() != n) throw std::invalid_argument("infer_batch: is_right_eye must hold one entry per item");
        std::vector<mi_rect> r;
        for (const Rect& x : rois) r.push_back(x.c());
        std::vector<int> flip(is_right_eye.begin(), is_right_eye.end());
        std::vector<float> c(n * 3 * MI_NUM_EYE_LANDMARKS), i5(n * 3 * MI_NUM_IRIS_LANDMARKS);
        detail::check(mi_iris_infer_images(h_, frames, batch, width, height, stride, r.empty() ? nullptr : r.data(), flip.empty() ? nullptr : flip.data(),
                                           items_per_frame, c.data(), i5.data(), MI_MEM_HOST, nullptr));
        std::vector<IrisResults> res(n);
        for (std::size_t i = 0; i < n; i++) {
            for (int k = 0; k < MI_NUM_EYE_LANDMARKS; k++) res[i].contour.push_back(Landmark{c[(i * MI_NUM_EYE_LANDMARKS + k) * 3], c[(i * MI_NUM_EYE_LANDMARKS + k) * 3 + 1], c[(i * MI_NUM_EYE_LANDMARKS + k) * 3 + 2]});
            for (int k = 0; k < MI_NUM_IRIS_LANDMARKS; k++) res[i].iris.push_back(Landmark{i5[(i * MI_NUM_IRIS_LANDMARKS + k) * 3], i5[(i * MI_NUM_IRIS_LANDMARKS + k) * 3 + 1], i5[(i * MI_NUM_IRIS_LANDMARKS + k) * 3 + 2]});
        }
        return res;
    }

   private:
    mi_iris* h_ = nullptr;
};

// face_detection_to_roi(face_detection, image_size, None) (face_landmark.rs:180-198); image_size = (width, height)
inline Rect face_detection_to_roi(const Detection& d, std::pair<int, int> image_size) {
    mi_detection c{};
    for (int k = 0; k < 16; k++) c.data[k] = d.data[k];
    c.score = d.score;
    mi_rect r{};
    detail::check(mi_face_detection_to_roi(&c, image_size.first, image_size.second, &r));
    return Rect::from(r);
}

// iris_roi_from_face_landmarks(face_landmarks, image_size) -> (left_eye_roi, right_eye_roi) (iris_landmark.rs:268-292)
inline std::pair<Rect, Rect> iris_roi_from_face_landmarks(const std::vector<Landmark>& lm, std::pair<int, int> image_size) {
    if (lm.size() < MI_NUM_FACE_LANDMARKS) throw Error(MI_EINVAL, "expected 468 face landmarks");  // the reference would panic on lm[362]
    std::vector<mi_landmark> c(MI_NUM_FACE_LANDMARKS);
    for (int i = 0; i < MI_NUM_FACE_LANDMARKS; i++) c[i] = mi_landmark{lm[i].x, lm[i].y, lm[i].z};
    mi_rect l{}, r{};
    detail::check(mi_iris_roi_from_face_landmarks(c.data(), image_size.first, image_size.second, &l, &r));
    return {Rect::from(l), Rect::from(r)};
}

// bbox_to_roi(bbox, image_size, rotation_keypoints, scale, mode) (transform.rs:44-109); SizeMode as in transform.rs:24-34
enum class SizeMode { Default = 0, SquareLong = 1, SquareShort = 2 };
inline Rect bbox_to_roi(const std::array<double, 4>& bbox, std::pair<int, int> image_size,
                        std::optional<std::array<double, 4>> rotation_keypoints = std::nullopt, std::pair<double, double> scale = {1.0, 1.0},
                        SizeMode mode = SizeMode::Default) {
    mi_rect r{};
    detail::check(mi_bbox_to_roi(bbox.data(), image_size.first, image_size.second, rotation_keypoints ? rotation_keypoints->data() : nullptr,
                                 scale.first, scale.second, static_cast<int>(mode), &r));
    return Rect::from(r);
}
// bbox_from_landmarks(landmarks) (transform.rs:146-165) -> {xmin, ymin, xmax, ymax}
inline std::array<double, 4> bbox_from_landmarks(const std::vector<Landmark>& lm) {
    std::vector<mi_landmark> c(lm.size());
    for (size_t i = 0; i < lm.size(); i++) c[i] = mi_landmark{lm[i].x, lm[i].y, lm[i].z};
    std::array<double, 4> out{};
    detail::check(mi_bbox_from_landmarks(c.data(), static_cast<int>(c.size()), out.data()));
    return out;
}

// convert_image_to_mat(im_bytes) (utils.rs:8-21): an owning RGB picture; `.image()` is the borrowed view the infer() calls take
struct OwnedImage {
    std::vector<std::uint8_t> rgb;
    int width = 0, height = 0;
    Image image() const { return Image{rgb.data(), width, height, 3 * width}; }
};
inline OwnedImage convert_image_to_mat(const std::uint8_t* im_bytes, std::size_t n, int device = 0) {
    OwnedImage o;
    detail::check(mi_jpeg_info(im_bytes, n, &o.width, &o.height));
    o.rgb.resize(static_cast<std::size_t>(3) * o.width * o.height);
    detail::check(mi_jpeg_decode_rgb(device, im_bytes, n, o.rgb.data(), o.rgb.size(), &o.width, &o.height, MI_MEM_HOST, nullptr));
    return o;
}

// update_face_landmarks_with_iris_results(face_landmarks, iris_data_left, iris_data_right) (iris_landmark.rs:380-398)
inline std::vector<Landmark> update_face_landmarks_with_iris_results(const std::vector<Landmark>& face_landmarks, const IrisResults& left,
                                                                     const IrisResults& right) {
    if (face_landmarks.size() != MI_NUM_FACE_LANDMARKS) throw Error(MI_EINVAL, "unexpected number of items in face_landmarks");  // the reference's Err
    if (left.contour.size() != MI_NUM_EYE_LANDMARKS || right.contour.size() != MI_NUM_EYE_LANDMARKS) throw Error(MI_EINVAL, "expected 71 contour landmarks per eye");
    auto pack = [](const std::vector<Landmark>& v) {
        std::vector<mi_landmark> c(v.size());
        for (size_t i = 0; i < v.size(); i++) c[i] = mi_landmark{v[i].x, v[i].y, v[i].z};
        return c;
    };
    std::vector<mi_landmark> f = pack(face_landmarks), l = pack(left.contour), r = pack(right.contour);
    detail::check(mi_update_face_landmarks_with_iris_results(f.data(), l.data(), r.data(), f.data()));
    std::vector<Landmark> out(f.size());
    for (size_t i = 0; i < f.size(); i++) out[i] = Landmark{f[i].x, f[i].y, f[i].z};
    return out;
}

// The item layout of mi_pipeline_run_faces for these detection counts (mi_face_items_layout: host only, no GPU).
struct FaceItemsLayout {
    std::vector<int> item_frame, item_face;  // [max_items], -1 in unused slots
    int n_items = 0, dropped = 0;            // slots used; faces (within max_faces) that got no slot
};
inline FaceItemsLayout face_items_layout(const std::vector<int>& face_counts, int max_faces, int max_items) {
    FaceItemsLayout o;
    // (the C side refuses max_items outside 1..2^20 before it writes, so this allocation stops there too)
    o.item_frame.resize(static_cast<std::size_t>(std::min(std::max(max_items, 0), 1 << 20)));
    o.item_face.resize(o.item_frame.size());
    int n[2] = {0, 0};
    detail::check(mi_face_items_layout(face_counts.data(), static_cast<int>(face_counts.size()), max_faces, max_items, o.item_frame.data(),
                                       o.item_face.data(), n));
    o.n_items = n[0];
    o.dropped = n[1];
    return o;
}

// The batched detector -> mesh -> iris flow on the device (mi_pipeline_*), results in host memory.
struct FacesResults {            // mi_pipeline_run_faces: see include/mi_face.h for the layout of the items
    std::vector<mi_detection> faces;         // [batch][max_faces], zeros behind a frame's last detection
    std::vector<int> face_counts;            // [batch]
    std::vector<int> item_frame, item_face;  // [max_items]
    int n_items = 0, dropped = 0;
    std::vector<float> landmarks;            // [max_items][468][3]
    std::vector<int> present;                // [max_items]
    std::vector<float> eyes;                 // [max_items][2][76][3]
};
class Pipeline {
   public:
    explicit Pipeline(FaceDetectionModel model_type, std::optional<std::string> model_dir = std::nullopt, int device = 0) {
        detail::check(mi_pipeline_create(static_cast<int>(model_type), model_dir ? model_dir->c_str() : nullptr, device, &h_));
    }
    ~Pipeline() { mi_pipeline_free(h_); }
    Pipeline(const Pipeline&) = delete;
    Pipeline& operator=(const Pipeline&) = delete;

    // lib.rs:24-40 for the first max_faces faces of every frame; the mesh and iris networks run on max_items (0: batch * max_faces) items
    // whatever the detector finds, so choose max_items for the faces you expect.
    FacesResults run_faces(const std::uint8_t* frames, int batch, int width, int height, int stride, int max_faces = 4, int max_items = 0) const {
        // the C entry's ranges, checked before anything is sized from them (batch * max_faces must not overflow, and the results are 10 kB an item)
        if (batch < 1 || batch > (1 << 26) || max_faces < 1 || max_faces > 16) throw std::invalid_argument("run_faces: batch 1..2^26, max_faces 1..16");
        if (max_items <= 0) max_items = static_cast<int>(std::min<long long>(static_cast<long long>(batch) * max_faces, 1 << 20));
        if (max_items > 32767) throw std::invalid_argument("run_faces: max_items 1..32767 (0: batch * max_faces)");
        const std::size_t M = static_cast<std::size_t>(max_items);
        FacesResults r;
        r.faces.resize(static_cast<std::size_t>(batch) * max_faces);
        r.face_counts.resize(static_cast<std::size_t>(batch));
        r.item_frame.resize(M);
        r.item_face.resize(M);
        r.landmarks.resize(M * 3 * MI_NUM_FACE_LANDMARKS);
        r.present.resize(M);
        r.eyes.resize(M * 2 * 3 * (MI_NUM_EYE_LANDMARKS + MI_NUM_IRIS_LANDMARKS));
        int n[2] = {0, 0};
        detail::check(mi_pipeline_run_faces(h_, frames, batch, width, height, stride, max_faces, max_items, r.faces.data(), r.face_counts.data(),
                                            r.item_frame.data(), r.item_face.data(), n, r.landmarks.data(), r.present.data(), r.eyes.data(),
                                            MI_MEM_HOST, nullptr));
        r.n_items = n[0];
        r.dropped = n[1];
        return r;
    }

   private:
    mi_pipeline* h_ = nullptr;
};

// Landmark-to-ROI face tracking for video streams (mi_tracker_*), results in host memory.  NOT the reference's behaviour (it has no video
// loop): MediaPipe's — the ROI of a stream's next frame comes from the landmarks of its last one, the detector runs only for streams that
// have no face yet or have lost it.  include/mi_face.h states the two rules.
struct TrackRoi {
    mi_rect roi{};
    bool valid = false;
};
// mi_track_roi_from_landmarks (host only, no GPU): landmarks f32 [468][3], normalised to a frame of width x height
inline TrackRoi track_roi_from_landmarks(const float* landmarks, int width, int height) {
    TrackRoi o;
    int valid = 0;
    detail::check(mi_track_roi_from_landmarks(landmarks, width, height, &o.roi, &valid));
    o.valid = valid != 0;
    return o;
}
struct TrackDetectLayout {
    std::vector<int> det_stream;   // [max_detect], -1 in unused slots
    int used = 0, waiting = 0;     // slots used; lost streams left without a slot
};
// mi_track_detect_layout (host only, no GPU)
inline TrackDetectLayout track_detect_layout(const std::vector<int>& tracked, int max_detect, int start = 0) {
    TrackDetectLayout o;
    // (the C side refuses max_detect outside 1..streams before it writes, so this allocation stops there too)
    o.det_stream.resize(static_cast<std::size_t>(std::min<long long>(std::max(max_detect, 0), static_cast<long long>(tracked.size()))));
    int n[2] = {0, 0};
    detail::check(mi_track_detect_layout(tracked.data(), static_cast<int>(tracked.size()), max_detect, start, o.det_stream.data(), n));
    o.used = n[0];
    o.waiting = n[1];
    return o;
}
struct TrackStep {                 // mi_tracker_step: one entry per stream, zeros where a stream has no result
    std::vector<mi_detection> faces;   // [streams] the detection a stream was acquired from (source 1)
    std::vector<int> face_counts;      // [streams]
    std::vector<int> source;           // [streams] 2: the state's ROI, 1: the detector's, 0: none
    std::vector<mi_rect> rois;         // [streams] the ROI the mesh ran on
    std::vector<float> landmarks;      // [streams][468][3]
    std::vector<int> present;          // [streams]
    std::vector<float> eyes;           // [streams][2][76][3]
    std::vector<int> det_stream;       // [max_detect]
    int used = 0, waiting = 0;
};
struct TrackState {
    std::vector<mi_rect> rois;         // [streams], zeros for a lost stream
    std::vector<int> tracked;          // [streams]
};
class Tracker {
   public:
    Tracker(FaceDetectionModel model_type, int streams, std::optional<std::string> model_dir = std::nullopt, int device = 0) : streams_(streams) {
        detail::check(mi_tracker_create(static_cast<int>(model_type), model_dir ? model_dir->c_str() : nullptr, device, streams, &h_));
    }
    ~Tracker() { mi_tracker_free(h_); }
    Tracker(const Tracker&) = delete;
    Tracker& operator=(const Tracker&) = delete;

    int streams() const { return streams_; }
    void set_option(const std::string& key, int value) { detail::check(mi_tracker_set_option(h_, key.c_str(), value)); }
    // frames: one RGB frame per stream, frame s the next picture of stream s; the detector runs on exactly max_detect (0: streams) items.
    // A handle's steps are ordered: each reads the state the previous one wrote.
    TrackStep step(const std::uint8_t* frames, int width, int height, int stride, int max_detect = 0) {
        if (max_detect <= 0) max_detect = streams_;
        if (max_detect > streams_) throw std::invalid_argument("step: max_detect 1..streams (0: streams)");
        const std::size_t S = static_cast<std::size_t>(streams_);
        TrackStep r;
        r.faces.resize(S);
        r.face_counts.resize(S);
        r.source.resize(S);
        r.rois.resize(S);
        r.landmarks.resize(S * 3 * MI_NUM_FACE_LANDMARKS);
        r.present.resize(S);
        r.eyes.resize(S * 2 * 3 * (MI_NUM_EYE_LANDMARKS + MI_NUM_IRIS_LANDMARKS));
        r.det_stream.resize(static_cast<std::size_t>(max_detect));
        int n[2] = {0, 0};
        detail::check(mi_tracker_step(h_, frames, width, height, stride, max_detect, r.faces.data(), r.face_counts.data(), r.source.data(),
                                      r.rois.data(), r.landmarks.data(), r.present.data(), r.eyes.data(), r.det_stream.data(), n, MI_MEM_HOST,
                                      nullptr));
        r.used = n[0];
        r.waiting = n[1];
        return r;
    }
    void reset(int stream_index = -1) { detail::check(mi_tracker_reset(h_, stream_index)); }
    TrackState state() const {
        TrackState s;
        s.rois.resize(static_cast<std::size_t>(streams_));
        s.tracked.resize(static_cast<std::size_t>(streams_));
        detail::check(mi_tracker_get_state(h_, s.rois.data(), s.tracked.data()));
        return s;
    }
    void set_state(int first, const std::vector<mi_rect>& rois, const std::vector<int>& tracked) {
        if (rois.size() != tracked.size()) throw std::invalid_argument("set_state: one ROI and one flag per stream written");
        detail::check(mi_tracker_set_state(h_, first, static_cast<int>(tracked.size()), rois.data(), tracked.data()));
    }

   private:
    mi_tracker* h_ = nullptr;
    int streams_ = 0;
};

// FaceEmbeddings (face_embeddings.rs:22-109).  The model is the CALLER'S: the reference ships no face_embeddings.tflite, none is shipped here,
// and the reference's own model has never been run on this engine; any graph of the operators the engine lowers that maps [1,112,112,3] to
// one output of D values per frame loads.  Those include the family of a ResNet-style (ArcFace) float graph: dense 3x3 CONV_2D (on the matrix
// cores: option "conv_mfma"), MUL / ADD by per-channel constants (unfolded batch normalisation), PRELU, FULLY_CONNECTED (the list: mi_face.h).
struct FaceItemEmbeddings {       // mi_fe_infer_face_items, results in host memory
    int features = 0;
    std::vector<float> embeddings;   // [max_items][D], zeros where valid is 0
    std::vector<int> valid;          // [max_items]
    std::vector<float> raw;          // [max_items][D] when asked for: the network's output before l2_norm
    std::vector<float> chips;        // [max_items][112][112][3] when asked for: the network's input
    std::vector<Rect> rois;          // [max_items], infer_items_aligned only: the fitted ROI (the whole image where the fit is invalid)
};
// where the points of an aligned chip come from (MI_ALIGN_*; mi_face.h states the gather rule and the fit)
enum class AlignSource { Points = MI_ALIGN_POINTS, Mesh = MI_ALIGN_MESH, Detection = MI_ALIGN_DETECTION };
class FaceEmbeddings {
   public:
    // FaceEmbeddings::new(model_path): a FILE path, default "./models/face_embeddings.tflite" (face_embeddings.rs:30-37)
    explicit FaceEmbeddings(std::optional<std::string> model_path = std::nullopt, int device = 0) {
        detail::check(mi_fe_create(model_path ? model_path->c_str() : nullptr, device, &h_));
        detail::check(mi_fe_features(h_, &features_));
    }
    ~FaceEmbeddings() { mi_fe_free(h_); }
    FaceEmbeddings(const FaceEmbeddings&) = delete;
    FaceEmbeddings& operator=(const FaceEmbeddings&) = delete;
    int features() const { return features_; }
    // operand precision of the network's dense k x k convolutions (mi_model option "conv_bf16" on mi_fe_model): "f32" (default), "bf16"
    // (operands rounded to bf16) or "bf16x3" (operands split into two bf16 values: about f32 accuracy); anything else throws std::invalid_argument
    void set_precision(const std::string& precision) {
        const int v = precision == "f32" ? 0 : precision == "bf16" ? 1 : precision == "bf16x3" ? 2 : -1;
        if (v < 0) throw std::invalid_argument("precision must be \"f32\", \"bf16\" or \"bf16x3\"");
        detail::check(mi_model_set_option(mi_fe_model(h_), "conv_bf16", v));
    }
    std::string precision() const {
        int v = 0;
        detail::check(mi_model_get_option(mi_fe_model(h_), "conv_bf16", &v));
        return v == 1 ? "bf16" : v == 2 ? "bf16x3" : "f32";
    }

    // FaceEmbeddings::infer(&Mat, BBox) -> Array2<f32> [1, D], l2-normalised; bbox in absolute pixels (face_embeddings.rs:46-89).  Throws
    // Error (MI_ERANGE) where the reference panics: a box that leaves the image.
    std::vector<float> infer(const Image& image, const BBox& bbox) const {
        std::vector<float> out(static_cast<std::size_t>(features_));
        const double b[4] = {bbox.xmin, bbox.ymin, bbox.xmax, bbox.ymax};
        detail::check(mi_fe_infer_image(h_, image.rgb, image.width, image.height, image.stride, b, out.data(), features_));
        return out;
    }
    // every item of what Pipeline::run_faces returned, frames in host memory
    FaceItemEmbeddings infer_items(const std::uint8_t* frames, int batch, int width, int height, int stride, const FacesResults& r,
                                   bool want_raw = false, bool want_chips = false) const {
        const std::size_t M = r.item_frame.size(), D = static_cast<std::size_t>(features_);
        if (batch < 1 || M < 1 || M > 32767 || r.item_face.size() != M || r.faces.size() % static_cast<std::size_t>(batch) != 0)
            throw std::invalid_argument("infer_items: the result of run_faces on these frames is expected (max_items 1..32767)");
        FaceItemEmbeddings o;
        o.features = features_;
        o.embeddings.resize(M * D);
        o.valid.resize(M);
        if (want_raw) o.raw.resize(M * D);
        if (want_chips) o.chips.resize(M * 3 * MI_FE_CHIP_SIZE * MI_FE_CHIP_SIZE);
        detail::check(mi_fe_infer_face_items(h_, frames, batch, width, height, stride, r.faces.data(), static_cast<int>(r.faces.size() / batch),
                                             r.item_frame.data(), r.item_face.data(), static_cast<int>(M), o.embeddings.data(), o.valid.data(),
                                             want_raw ? o.raw.data() : nullptr, want_chips ? o.chips.data() : nullptr, MI_MEM_HOST, nullptr));
        return o;
    }

    // Aligned chips — NOT the reference's behaviour (it crops the box: infer / infer_items).  points: pixel coordinates in the template's
    // order, five of them (four for AlignSource::Detection); the least-squares similarity fit to the template, the warp of the WHOLE image
    // by it, the network, l2_norm.  Throws Error (MI_ERANGE) for points without a fit.  roi: the fitted ROI, when asked for.
    std::vector<float> infer_aligned(const Image& image, const std::vector<std::array<float, 2>>& points, AlignSource source = AlignSource::Points,
                                     Rect* roi = nullptr) const {
        std::vector<float> out(static_cast<std::size_t>(features_));
        mi_rect r = Rect{}.c();
        const int rc = mi_fe_infer_image_aligned(h_, image.rgb, image.width, image.height, image.stride, points.empty() ? nullptr : points[0].data(),
                                                 static_cast<int>(points.size()), static_cast<int>(source), out.data(), features_, &r);
        if (roi) *roi = Rect::from(r);
        detail::check(rc);
        return out;
    }
    // ... for every item of what Pipeline::run_faces returned, frames in host memory: the points of an item from its mesh (landmarks, present),
    // from its detection's key points, or from `points` ([max_items][5] pixel points, AlignSource::Points)
    FaceItemEmbeddings infer_items_aligned(const std::uint8_t* frames, int batch, int width, int height, int stride, const FacesResults& r,
                                           AlignSource source = AlignSource::Mesh, const std::vector<std::array<float, 2>>* points = nullptr,
                                           bool want_raw = false, bool want_chips = false) const {
        const std::size_t M = r.item_frame.size(), D = static_cast<std::size_t>(features_);
        if (batch < 1 || M < 1 || M > 32767 || r.item_face.size() != M || r.faces.size() % static_cast<std::size_t>(batch) != 0)
            throw std::invalid_argument("infer_items_aligned: the result of run_faces on these frames is expected (max_items 1..32767)");
        const void* src = nullptr;
        const int* gate = nullptr;
        if (source == AlignSource::Mesh) {
            if (r.landmarks.size() != M * MI_NUM_FACE_LANDMARKS * 3 || r.present.size() != M)
                throw std::invalid_argument("infer_items_aligned: landmarks [max_items][468][3] and present [max_items] are expected");
            src = r.landmarks.data();
            gate = r.present.data();
        } else if (source == AlignSource::Detection) {
            src = r.faces.data();
        } else {
            if (!points || points->size() != M * 5) throw std::invalid_argument("infer_items_aligned: [max_items][5] pixel points are expected");
            src = points->data();
        }
        FaceItemEmbeddings o;
        o.features = features_;
        o.embeddings.resize(M * D);
        o.valid.resize(M);
        if (want_raw) o.raw.resize(M * D);
        if (want_chips) o.chips.resize(M * 3 * MI_FE_CHIP_SIZE * MI_FE_CHIP_SIZE);
        std::vector<mi_rect> rois(M, Rect{}.c());
        detail::check(mi_fe_infer_aligned_items(h_, frames, batch, width, height, stride, static_cast<int>(source), src, gate,
                                                static_cast<int>(r.faces.size() / batch), r.item_frame.data(), r.item_face.data(), static_cast<int>(M),
                                                o.embeddings.data(), o.valid.data(), want_raw ? o.raw.data() : nullptr,
                                                want_chips ? o.chips.data() : nullptr, rois.data(), MI_MEM_HOST, nullptr));
        for (const mi_rect& q : rois) o.rois.push_back(Rect::from(q));
        return o;
    }

   private:
    mi_fe* h_ = nullptr;
    int features_ = 0;
};

// Aligned chips, host only (mi_face.h): the template of a source in chip pixels; the pixel points of one face by the gather rule (src:
// [468][3] normalised landmarks, a detection's 17 floats, or [5][2] points); the fit of such points as the ROI of the chip, and its validity
inline std::vector<std::array<double, 2>> face_align_template(AlignSource source) {
    double xy[5][2];
    int n = 0;
    detail::check(mi_face_align_template(static_cast<int>(source), xy, &n));
    std::vector<std::array<double, 2>> out;
    for (int i = 0; i < n; i++) out.push_back({xy[i][0], xy[i][1]});
    return out;
}
inline std::vector<std::array<float, 2>> face_align_points(AlignSource source, const std::vector<float>& src, std::pair<int, int> image_size) {
    const std::size_t need = source == AlignSource::Mesh ? MI_NUM_FACE_LANDMARKS * 3 : source == AlignSource::Detection ? 17 : 10;
    if (src.size() != need) throw std::invalid_argument("face_align_points: the source's operand has another length");
    float pts[5][2];
    int n = 0;
    detail::check(mi_face_align_points(static_cast<int>(source), src.data(), image_size.first, image_size.second, pts, &n));
    std::vector<std::array<float, 2>> out;
    for (int i = 0; i < n; i++) out.push_back({pts[i][0], pts[i][1]});
    return out;
}
inline std::pair<Rect, bool> face_align_roi(const std::vector<std::array<float, 2>>& points, AlignSource source = AlignSource::Points) {
    mi_rect r = Rect{}.c();
    int valid = 0;
    detail::check(mi_face_align_roi(points.empty() ? nullptr : points[0].data(), static_cast<int>(points.size()), static_cast<int>(source), &r, &valid));
    return {Rect::from(r), valid != 0};
}

// crop_image_to_bbox's rectangle for a detection (face_embeddings.rs:101-109 on bbox().scale(size)); host only.  -> {x, y, w, h}, valid
inline std::pair<std::array<int, 4>, bool> face_chip_rect(const Detection& d, std::pair<int, int> image_size) {
    mi_detection c{};
    std::copy(d.data.begin(), d.data.end(), c.data);
    c.score = d.score;
    std::array<int, 4> rect{};
    int valid = 0;
    detail::check(mi_face_chip_rect(&c, image_size.first, image_size.second, rect.data(), &valid));
    return {rect, valid != 0};
}
// utils::l2_norm / utils::similarity_score (utils.rs:30-50), bit-identical to the reference's order of operations; host only
inline std::vector<float> l2_norm(const std::vector<float>& arr) {
    std::vector<float> out(arr.size());
    detail::check(mi_l2_norm(arr.data(), static_cast<int>(arr.size()), out.data()));
    return out;
}
inline float similarity_score(const std::vector<float>& a, const std::vector<float>& b) {
    if (a.size() != b.size()) throw std::invalid_argument("similarity_score: vectors of one length are expected");
    float out = 0.f;
    detail::check(mi_similarity_score(a.data(), b.data(), static_cast<int>(a.size()), &out));
    return out;
}
// similarity_score of every row of a [n][features] against every row of a gallery b [m][features], on the GPU; pointers follow `mem`
inline void similarity_matrix(const float* a, int n, const float* b, int m, int features, float* out, int mem = MI_MEM_HOST, void* stream = nullptr,
                              int device = 0) {
    detail::check(mi_similarity_matrix(device, a, n, b, m, features, out, mem, stream));
}

// The selection rule of Gallery::topk applied to a score matrix scores [n][m] (mi_topk_select: host only, no GPU): index [n][k], score [n][k]
struct TopK {
    int k = 0;
    std::vector<int> index;     // [n][k], -1 beyond the eligible rows
    std::vector<float> score;   // [n][k], -INFINITY there
    std::vector<int> label;     // [n][k], -1 there (Gallery::topk only)
};
inline TopK topk_select(const std::vector<float>& scores, int n, int m, int k) {
    if (n < 1 || m < 1 || scores.size() != static_cast<std::size_t>(n) * m) throw std::invalid_argument("topk_select: scores must be [n][m]");
    TopK o;
    o.k = k;
    o.index.resize(static_cast<std::size_t>(n) * (k > 0 ? k : 0));
    o.score.resize(o.index.size());
    detail::check(mi_topk_select(scores.data(), n, m, k, o.index.data(), o.score.data()));
    return o;
}
// mi_gallery: enrolled embeddings rows [m][features], copied once into device memory the handle owns, and an int label per row (empty: the
// label is the row index).  topk answers "who is this": the k best rows of every query by cosine score — bit for bit similarity_matrix's
// scores, the rule of topk_select — without the [n][m] matrix ever reaching memory.
class Gallery {
   public:
    Gallery(const float* rows, int m, int features, const std::vector<int>& labels = {}, int mem = MI_MEM_HOST, int device = 0) {
        if (!labels.empty() && labels.size() != static_cast<std::size_t>(m > 0 ? m : 0)) throw std::invalid_argument("Gallery: one label per row is expected");
        detail::check(mi_gallery_create(device, rows, m, features, labels.empty() ? nullptr : labels.data(), mem, &h_));
        detail::check(mi_gallery_dims(h_, &m_, &features_));
    }
    ~Gallery() { mi_gallery_free(h_); }
    Gallery(const Gallery&) = delete;
    Gallery& operator=(const Gallery&) = delete;
    int rows() const { return m_; }
    int features() const { return features_; }
    // "splits": column ranges a row of query tiles is spread over (0 = automatic, otherwise 1..64); the results do not depend on it
    void set_option(const char* key, int value) { detail::check(mi_gallery_set_option(h_, key, value)); }
    int get_option(const char* key) const {
        int v = 0;
        detail::check(mi_gallery_get_option(h_, key, &v));
        return v;
    }
    // queries [n][features] in host memory -> index / score / label [n][k]
    TopK topk(const float* queries, int n, int k) const {
        if (n < 1 || k < 1 || k > 16) throw std::invalid_argument("Gallery::topk: n >= 1 and k 1..16 are expected");
        TopK o;
        o.k = k;
        o.index.resize(static_cast<std::size_t>(n) * k);
        o.score.resize(o.index.size());
        o.label.resize(o.index.size());
        detail::check(mi_gallery_topk(h_, queries, n, k, o.index.data(), o.score.data(), o.label.data(), MI_MEM_HOST, nullptr));
        return o;
    }
    // the same wherever the operands live (`mem`); label may be null; asynchronous with MI_MEM_DEVICE and a caller stream.  The embeddings
    // of FaceEmbeddings' item entry are a valid `queries` as they lie in device memory: invalid items come out as all -1.
    void topk(const float* queries, int n, int k, int* index, float* score, int* label, int mem, void* stream = nullptr) const {
        detail::check(mi_gallery_topk(h_, queries, n, k, index, score, label, mem, stream));
    }

   private:
    mi_gallery* h_ = nullptr;
    int m_ = 0, features_ = 0;
};

// render.rs on the device (include/mi_face.h, "render.rs").  Colors::{BLACK, ...} (render.rs:28-68) as the bytes render_to_image writes.
struct Colors {
    static constexpr mi_color BLACK = MI_COLOR_BLACK, RED = MI_COLOR_RED, GREEN = MI_COLOR_GREEN, BLUE = MI_COLOR_BLUE, PINK = MI_COLOR_PINK,
                              WHITE = MI_COLOR_WHITE;
};
// One picture of render_to_image's result: RGBA rows of 4 * width bytes; `skipped` = items the C entry did not draw (empty
// rectangles, lines beyond 2^20 px).
struct RgbaImage {
    std::vector<std::uint8_t> rgba;
    int width = 0, height = 0, skipped = 0;
};
// render_to_image(annotations, image, blend_mode) (render.rs:361-479) for one picture in host memory: `annotations` index into `coords`
inline RgbaImage render_to_image(const std::vector<mi_annotation>& annotations, const std::vector<double>& coords, const Image& image, int device = 0) {
    RgbaImage o;
    o.width = image.width;
    o.height = image.height;
    o.rgba.resize(static_cast<std::size_t>(4) * image.width * image.height);
    detail::check(mi_render_annotations(device, image.rgb, 1, image.width, image.height, image.stride, annotations.data(),
                                        static_cast<int>(annotations.size()), coords.data(), static_cast<long>(coords.size()), o.rgba.data(), 4,
                                        4 * image.width, &o.skipped, MI_MEM_HOST, nullptr));
    return o;
}
// detections_to_render_data / face_landmarks_to_render_data / eye_landmarks_to_render_data + render_to_image (lib.rs:42-83) on the raw
// results of mi_pipeline_run / mi_fd_infer_images, wherever they live (`mem`); any of the three groups may be null.
inline void render_faces(const std::uint8_t* frames, int batch, int width, int height, int stride, const mi_detection* faces, const int* face_counts,
                         int faces_per_frame, const float* landmarks, const int* present, const float* eyes, const mi_render_style& style,
                         std::uint8_t* out, int out_channels, int out_stride, int* skipped = nullptr, int mem = MI_MEM_HOST, void* stream = nullptr,
                         int device = 0) {
    detail::check(mi_render_faces(device, frames, batch, width, height, stride, faces, face_counts, faces_per_frame, landmarks, present, eyes, &style,
                                  out, out_channels, out_stride, skipped, mem, stream));
}
// The same for the item list of mi_pipeline_run_faces: every face of a frame with its mesh, both eyes and both irises
// (iris_landmarks_to_render_data, iris_landmark.rs:330-377).  faces / face_counts, landmarks, present and eyes may be null.
inline void render_face_items(const std::uint8_t* frames, int batch, int width, int height, int stride, const mi_detection* faces,
                              const int* face_counts, int max_faces, const int* item_frame, const int* n_items, int max_items,
                              const float* landmarks, const int* present, const float* eyes, const mi_render_items_style& style, std::uint8_t* out,
                              int out_channels, int out_stride, int* skipped = nullptr, int mem = MI_MEM_HOST, void* stream = nullptr,
                              int device = 0) {
    detail::check(mi_render_face_items(device, frames, batch, width, height, stride, faces, face_counts, max_faces, item_frame, n_items, max_items,
                                       landmarks, present, eyes, &style, out, out_channels, out_stride, skipped, mem, stream));
}

}  // namespace mi_face
