// capi_landmarks.cpp — FaceLandmark and IrisLandmark: the mesh's and the iris network's entries.
#include "capi_internal.hpp"

namespace mi {
namespace capi {
// the mesh's two outputs into `a`, then project_landmarks + the face flag in one launch
void project_mesh(mi::Model& m, mi::ProjArgs& a, hipStream_t s) {
    a.raw = m.output_device(0);
    a.raw_fs = static_cast<long>(m.output_elems(0));
    a.flag = m.output_device(1) + (m.output_elems(1) - 1);  // `flatten[flatten.len() - 1]` — face_landmark.rs:292-293
    a.flag_fs = static_cast<long>(m.output_elems(1));
    check_launch(mi::launch_project(a, s), "projection");
}

void iris_project(mi_iris* h, int batch, const mi::RectD* d_roi, const int* d_size, const double* d_pad, const int* d_flip, float* d_contour,
                  float* d_iris, hipStream_t s, const int* d_gate, long out_fs) {
    mi::Model& m = *h->model.m;
    // both outputs (71 contour + 5 iris landmarks per eye) in one launch
    mi::ProjArgs a;
    a.B = batch;
    a.n = MI_NUM_EYE_LANDMARKS;
    a.n2 = MI_NUM_IRIS_LANDMARKS;
    a.tensor_w = h->in_w;
    a.tensor_h = h->in_h;
    a.roi = d_roi;
    a.image_size = d_size;
    a.padding = d_pad;
    a.flip = d_flip;
    a.gate = d_gate;
    a.raw = m.output_device(0);
    a.raw_fs = static_cast<long>(m.output_elems(0));
    a.out = d_contour;
    a.out_fs = out_fs;
    a.raw2 = m.output_device(1);
    a.raw2_fs = static_cast<long>(m.output_elems(1));
    a.out2 = d_iris;
    a.out2_fs = out_fs;
    check_launch(mi::launch_project(a, s), "projection");
}

}  // namespace capi
}  // namespace mi

using namespace mi::capi;

extern "C" {

// ------------------------------------------------------------------------------------------------ FaceLandmark
static void fl_finish_create(mi_fl* h) {
    auto d = h->model.m->input_dims();
    h->in_h = d[1];
    h->in_w = d[2];
    // face_landmark.rs:241-247: last dim of outputs()[0] must hold NUM_DIMS * NUM_LANDMARKS = 1404 values
    if (h->model.m->num_outputs() < 2 || h->model.m->output_dims(0).back() < 3 * MI_NUM_FACE_LANDMARKS)
        throw ApiError(MI_EMODEL, "incompatible model: mesh output narrower than 1404");
}

int mi_fl_create_from_bytes(const uint8_t* tflite, size_t nbytes, int device, mi_fl** out) {
    return guarded([&] {
        require(tflite && nbytes && out, "null argument");
        create_handle(tflite, nbytes, device, out, fl_finish_create);
    });
}

int mi_fl_create(const char* model_path, int device, mi_fl** out) {
    return guarded([&] {
        require(out, "null argument");
        create_handle(model_path ? model_path : "./models/face_landmark.tflite", device, out, fl_finish_create);  // face_landmark.rs:211-215
    });
}

void mi_fl_free(mi_fl* h) { delete h; }
mi_model* mi_fl_model(mi_fl* h) { return h ? &h->model : nullptr; }

// A single-image entry's ROI and the picture's size for Rect::scaled, into the entry's block: *d_roi and *d_size are the device's view
// of the two; they stay as they are (null) without a ROI.
static void one_shot_roi(const OneShot& o, const mi_rect* roi, int width, int height, const mi::RectD** d_roi, const int** d_size) {
    if (!roi) return;
    std::memcpy(o.h<char>(kOneRoi), roi, sizeof(mi_rect));
    o.h<int>(kOneSize)[0] = width;
    o.h<int>(kOneSize)[1] = height;
    *d_roi = o.d<mi::RectD>(kOneRoi);
    *d_size = o.d<int>(kOneSize);
}

// the projection of N mesh items, before its operands and targets are set
static mi::ProjArgs mesh_args(const mi_fl* h, int N) {
    mi::ProjArgs a;
    a.B = N;
    a.n = MI_NUM_FACE_LANDMARKS;
    a.tensor_w = h->in_w;
    a.tensor_h = h->in_h;
    return a;
}

// What mi_fl_infer_tensor and mi_fl_infer_images share once the network's input stands in d_in: for host callers the scratch targets in
// front of the network and the three device-to-host copies behind it; then the usual ending.
static void mesh_run(mi_fl* h, const Call& c, const float* d_in, int N, const mi::RectD* d_rois, const int* d_sizes, float* landmarks, int* present,
                     float* raw_flags, int mem) {
    const size_t lm_elems = static_cast<size_t>(3) * MI_NUM_FACE_LANDMARKS * N;
    mi::ProjArgs a = mesh_args(h, N);
    a.roi = d_rois;
    a.image_size = d_sizes;
    a.out = result_target(h->d_lm, landmarks, lm_elems, mem);
    a.present = result_target(h->d_present, present, N, mem);
    a.raw_flag_out = result_target(h->d_flag, raw_flags, N, mem);
    c.m.run_device(d_in, N, c.s);
    project_mesh(c.m, a, c.s);
    hand_back(landmarks, a.out, lm_elems, mem, c.s, "D2H landmarks");
    hand_back(present, a.present, N, mem, c.s, "D2H present");
    hand_back(raw_flags, a.raw_flag_out, N, mem, c.s, "D2H flags");
    c.finish(mem);
}

// the mesh's image_to_tensor(frame, roi, (192,192), keep_aspect_ratio = false, (0,1)) for N items of `batch` frames in device memory
static float* mesh_items_to_tensor(mi_fl* h, mi::Model& m, const uint8_t* d_frames, int batch, int width, int height, int stride, const mi::RectD* d_rois,
                                   int items_per_frame, hipStream_t s) {
    mi::PreItems it = frame_items(d_frames, batch, width, height, stride);
    it.rois = d_rois; it.items_per_frame = items_per_frame; it.N = batch * items_per_frame; it.out_w = h->in_w; it.out_h = h->in_h; it.keep_aspect = 0;
    it.range_min = 0.0; it.range_max = 1.0;
    return items_to_tensor(it, m, h->d_geom, h->d_in, nullptr, s);
}

int mi_fl_infer_tensor(mi_fl* h, const float* in, int batch, const mi_rect* rois, const int* image_sizes, float* landmarks,
                       int* present, float* raw_flags, int mem, void* stream) {
    return guarded([&] {
        require(h && in && landmarks && present, "null argument");
        require(batch > 0, "batch must be positive");
        require_mem(mem);
        require(!rois || image_sizes, "image_sizes is required when rois are given");
        static_assert(sizeof(mi_rect) == sizeof(mi::RectD), "mi_rect layout");
        Call c(h->model, stream);
        const float* d_in = stage(h->d_in, in, c.m.input_elems() * batch, mem, c.s, "H2D input");
        const mi::RectD* d_rois = stage(h->d_roi, reinterpret_cast<const mi::RectD*>(rois), batch, mem, c.s, "H2D rois");
        // (from host memory the sizes travel with the ROIs only)
        const int* d_sizes = mem == MI_MEM_HOST && !rois ? nullptr : stage(h->d_size, image_sizes, static_cast<size_t>(2) * batch, mem, c.s, "H2D sizes");
        mesh_run(h, c, d_in, batch, d_rois, d_sizes, landmarks, present, raw_flags, mem);
    });
}

// FaceLandmark::infer(&Mat, Option<Rect>) for a batch of (frame, ROI) items (face_landmark.rs:232-306): image_to_tensor(frame, roi,
// (192,192), keep_aspect_ratio = false, (0,1)) on the device, network, face flag, project_landmarks.  Item i reads frame
// i / items_per_frame.  Only u8 frames and ROIs cross the bus (the f32 crops of mi_fl_infer_tensor are 442 KB per ROI).
int mi_fl_infer_images(mi_fl* h, const uint8_t* frames, int batch, int width, int height, int stride, const mi_rect* rois, int items_per_frame,
                       float* landmarks, int* present, float* raw_flags, int mem, void* stream) {
    return guarded([&] {
        require(h && frames && landmarks && present, "null argument");
        require_frames(batch, width, height, stride);
        require(items_per_frame > 0, "bad frame geometry");
        require(rois || items_per_frame == 1, "several items per frame need their ROIs");
        require_mem(mem);
        require(static_cast<long long>(batch) * items_per_frame <= (1 << 24), "too many items");
        Call c(h->model, stream);
        const int N = batch * items_per_frame;
        const uint8_t* d_frames = stage_frames(h->d_img, frames, batch, width, height, stride, mem, c.s);
        const mi::RectD* d_rois = stage(h->d_roi, reinterpret_cast<const mi::RectD*>(rois), N, mem, c.s, "H2D rois");
        const float* d_in = mesh_items_to_tensor(h, c.m, d_frames, batch, width, height, stride, d_rois, items_per_frame, c.s);
        const int* d_sizes = d_rois ? h->sizes.get(N, width, height, c.s) : nullptr;
        mesh_run(h, c, d_in, N, d_rois, d_sizes, landmarks, present, raw_flags, mem);
    });
}

// The same for a continuous host feed, split in two like the detector's (mi_fd_submit_images / mi_fd_collect): submit queues the H2D copy
// of the frames on the slot's own stream, then warp + network + projection on the handle's stream behind it, and returns; the projection
// kernel writes into the slot's pinned, mapped host block; collect waits for the slot and hands the results out.
int mi_fl_submit_images(mi_fl* h, int slot, const uint8_t* frames, int batch, int width, int height, int stride, const mi_rect* rois, int items_per_frame) {
    return guarded([&] {
        require(h && frames, "null argument");
        require_slot(slot);
        require_frames(batch, width, height, stride);
        require(items_per_frame > 0, "bad frame geometry");
        require(rois || items_per_frame == 1, "several items per frame need their ROIs");
        require(static_cast<long long>(batch) * items_per_frame <= (1 << 24), "too many items");
        Call c(h->model);
        mi::Model& m = c.m;
        const hipStream_t s = c.s;
        FlSlot& sl = h->slot[slot];
        if (sl.pending) throw ApiError(MI_EINVAL, "slot still holds an uncollected batch (call mi_fl_collect first)");
        sl.open();
        const int N = batch * items_per_frame;
        const size_t lm_bytes = sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * N;
        sl.out.reserve(lm_bytes + (sizeof(int) + sizeof(float)) * N);
        const uint8_t* d_frames = stage_frames(sl.d_frames, frames, batch, width, height, stride, MI_MEM_HOST, sl.copy);
        // (the ROIs are small and usually pageable: the runtime stages them before the call returns)
        const mi::RectD* d_rois = stage(sl.d_rois, reinterpret_cast<const mi::RectD*>(rois), N, MI_MEM_HOST, sl.copy, "H2D rois");
        mi::hip_check(hipEventRecord(sl.copied, sl.copy), "hipEventRecord");
        try {
            const int* d_sizes = d_rois ? h->sizes.get(N, width, height, s) : nullptr;
            mi::hip_check(hipStreamWaitEvent(s, sl.copied, 0), "hipStreamWaitEvent");
            const float* d_in = mesh_items_to_tensor(h, m, d_frames, batch, width, height, stride, d_rois, items_per_frame, s);
            mi::ProjArgs a = mesh_args(h, N);
            a.roi = d_rois; a.image_size = d_sizes;
            a.out = sl.out.d<float>(0);
            a.present = sl.out.d<int>(lm_bytes);
            a.raw_flag_out = sl.out.d<float>(lm_bytes + sizeof(int) * N);
            m.run_device(d_in, N, s);
            project_mesh(m, a, s);
        } catch (...) {
            (void)hipStreamSynchronize(sl.copy);   // the queued copy may still be reading the caller's frames
            throw;
        }
        mi::hip_check(hipEventRecord(sl.done, s), "hipEventRecord");
        sl.N = N; sl.pending = true;
    });
}

int mi_fl_collect(mi_fl* h, int slot, float* landmarks, int* present, float* raw_flags) {
    return guarded([&] {
        require(h && landmarks && present, "null argument");
        require_slot(slot);
        FlSlot& sl = h->slot[slot];
        slot_collect(h->model, sl, [&] {
            const size_t lm_bytes = sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * sl.N;
            std::memcpy(landmarks, sl.out.host, lm_bytes);
            std::memcpy(present, sl.out.h<char>(lm_bytes), sizeof(int) * sl.N);
            if (raw_flags) std::memcpy(raw_flags, sl.out.h<char>(lm_bytes + sizeof(int) * sl.N), sizeof(float) * sl.N);
        });
    });
}

int mi_fl_infer_image(mi_fl* h, const uint8_t* rgb, int width, int height, int stride, const mi_rect* roi, mi_landmark* out,
                      int cap, int* count) {
    return guarded([&] {
        require(h && rgb && out && count, "null argument");
        require(width > 0 && height > 0 && stride >= 3 * width, "bad image geometry");
        require(cap >= MI_NUM_FACE_LANDMARKS, "output capacity must be at least 468");
        Call c(h->model);
        mi::Model& m = c.m;
        const hipStream_t s = c.s;
        float* d_t = h->d_in.as<float>(m.input_elems());
        double pad[4];
        OneShot& o = h->one;
        const size_t lm_bytes = sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS;
        o.reserve(kOneResults + lm_bytes);
        // image_to_tensor(image, roi, (192,192), keep_aspect_ratio = false, (0,1), false) — face_landmark.rs:250
        mi::image_to_tensor_enqueue(rgb, width, height, stride, roi, h->in_w, h->in_h, false, 0.0, 1.0, false, d_t, pad,
                                    h->d_img.as<uint8_t>(static_cast<size_t>(stride) * height), s);
        mi::ProjArgs a = mesh_args(h, 1);
        one_shot_roi(o, roi, width, height, &a.roi, &a.image_size);
        a.out = o.d<float>(kOneResults);
        a.present = o.d<int>(kOneCount);
        BandClaim claim(m, 1);
        auto network = [&](bool one_shot) {
            m.run_device(d_t, 1, s, one_shot);
            project_mesh(m, a, s);
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        };
        with_band_retry(claim.ok, [&] { return m.band_failed(); }, network);
        const float* lm = o.h<float>(kOneResults);
        const int present = *o.h<int>(kOneCount);
        *count = 0;
        if (present) {
            for (int i = 0; i < MI_NUM_FACE_LANDMARKS; i++) out[i] = mi_landmark{lm[3 * i], lm[3 * i + 1], lm[3 * i + 2]};
            *count = MI_NUM_FACE_LANDMARKS;
        }
    });
}

// ------------------------------------------------------------------------------------------------ IrisLandmark
static void iris_finish_create(mi_iris* h) {
    auto d = h->model.m->input_dims();
    h->in_h = d[1];
    h->in_w = d[2];
    // iris_landmark.rs:172-184
    if (h->model.m->num_outputs() < 2 || h->model.m->output_dims(0).back() != 3 * MI_NUM_EYE_LANDMARKS ||
        h->model.m->output_dims(1).back() != 3 * MI_NUM_IRIS_LANDMARKS)
        throw ApiError(MI_EMODEL, "unexpected number of eye landmarks");
}

int mi_iris_create_from_bytes(const uint8_t* tflite, size_t nbytes, int device, mi_iris** out) {
    return guarded([&] {
        require(tflite && nbytes && out, "null argument");
        create_handle(tflite, nbytes, device, out, iris_finish_create);
    });
}

int mi_iris_create(const char* model_path, int device, mi_iris** out) {
    return guarded([&] {
        require(out, "null argument");
        create_handle(model_path ? model_path : "./models/iris_landmark.tflite", device, out, iris_finish_create);  // iris_landmark.rs:145-149
    });
}

void mi_iris_free(mi_iris* h) { delete h; }
mi_model* mi_iris_model(mi_iris* h) { return h ? &h->model : nullptr; }

// What mi_iris_infer_tensor and mi_iris_infer_images share once the network's input stands in d_in: for host callers the scratch targets
// in front of the network and the two device-to-host copies behind it; then the usual ending.
static void iris_run(mi_iris* h, const Call& c, const float* d_in, int N, const mi::RectD* d_rois, const int* d_sizes, const double* d_pad,
                     const int* d_flip, float* contour, float* iris, int mem) {
    const size_t nc = static_cast<size_t>(3) * MI_NUM_EYE_LANDMARKS * N, ni = static_cast<size_t>(3) * MI_NUM_IRIS_LANDMARKS * N;
    float* dc = result_target(h->d_contour, contour, nc, mem);
    float* di = result_target(h->d_iris, iris, ni, mem);
    c.m.run_device(d_in, N, c.s);
    iris_project(h, N, d_rois, d_sizes, d_pad, d_flip, dc, di, c.s);
    hand_back(contour, dc, nc, mem, c.s, "D2H contour");
    hand_back(iris, di, ni, mem, c.s, "D2H iris");
    c.finish(mem);
}

int mi_iris_infer_tensor(mi_iris* h, const float* in, int batch, const mi_rect* rois, const int* image_sizes, const double* padding,
                         const int* is_right_eye, float* contour, float* iris, int mem, void* stream) {
    return guarded([&] {
        require(h && in && contour && iris, "null argument");
        require(batch > 0, "batch must be positive");
        require_mem(mem);
        require(!rois || image_sizes, "image_sizes is required when rois are given");
        Call c(h->model, stream);
        const float* d_in = stage(h->d_in, in, c.m.input_elems() * batch, mem, c.s, "H2D input");
        const mi::RectD* d_rois = stage(h->d_roi, reinterpret_cast<const mi::RectD*>(rois), batch, mem, c.s, "H2D rois");
        // (from host memory the sizes travel with the ROIs only)
        const int* d_sizes = mem == MI_MEM_HOST && !rois ? nullptr : stage(h->d_size, image_sizes, static_cast<size_t>(2) * batch, mem, c.s, "H2D sizes");
        const double* d_pad = stage(h->d_pad, padding, static_cast<size_t>(4) * batch, mem, c.s, "H2D padding");
        const int* d_flip = stage(h->d_flip, is_right_eye, batch, mem, c.s, "H2D flip");
        iris_run(h, c, d_in, batch, d_rois, d_sizes, d_pad, d_flip, contour, iris, mem);
    });
}

// IrisLandmark::infer(&Mat, Option<Rect>, Option<bool>) for a batch of (frame, eye ROI) items (iris_landmark.rs:158-248):
// image_to_tensor(frame, roi, (64,64), keep_aspect_ratio = true, (0,1), flip = is_right_eye) on the device, network, both
// project_landmarks calls.  Item i reads frame i / items_per_frame (2 = the two eyes of a face).
int mi_iris_infer_images(mi_iris* h, const uint8_t* frames, int batch, int width, int height, int stride, const mi_rect* rois, const int* is_right_eye,
                         int items_per_frame, float* contour, float* iris, int mem, void* stream) {
    return guarded([&] {
        require(h && frames && contour && iris, "null argument");
        require_frames(batch, width, height, stride);
        require(items_per_frame > 0, "bad frame geometry");
        require(rois || items_per_frame == 1, "several items per frame need their ROIs");
        require_mem(mem);
        require(static_cast<long long>(batch) * items_per_frame <= (1 << 24), "too many items");
        Call c(h->model, stream);
        const int N = batch * items_per_frame;
        const uint8_t* d_frames = stage_frames(h->d_img, frames, batch, width, height, stride, mem, c.s);
        const mi::RectD* d_rois = stage(h->d_roi, reinterpret_cast<const mi::RectD*>(rois), N, mem, c.s, "H2D rois");
        const int* d_flip = stage(h->d_flip, is_right_eye, N, mem, c.s, "H2D flip");
        mi::PreItems it = frame_items(d_frames, batch, width, height, stride);
        it.rois = d_rois; it.flip = d_flip; it.items_per_frame = items_per_frame; it.N = N; it.out_w = h->in_w; it.out_h = h->in_h; it.keep_aspect = 1;
        it.range_min = 0.0; it.range_max = 1.0;
        double* d_pad = h->d_pad.as<double>(static_cast<size_t>(4) * N);
        const float* d_in = items_to_tensor(it, c.m, h->d_geom, h->d_in, d_pad, c.s);
        const int* d_sizes = d_rois ? h->sizes.get(N, width, height, c.s) : nullptr;
        iris_run(h, c, d_in, N, d_rois, d_sizes, d_pad, d_flip, contour, iris, mem);
    });
}

int mi_iris_infer_image(mi_iris* h, const uint8_t* rgb, int width, int height, int stride, const mi_rect* roi, int is_right_eye,
                        mi_landmark* contour71, mi_landmark* iris5) {
    return guarded([&] {
        require(h && rgb && contour71 && iris5, "null argument");
        require(width > 0 && height > 0 && stride >= 3 * width, "bad image geometry");
        Call call(h->model);
        mi::Model& m = call.m;
        const hipStream_t s = call.s;
        float* d_t = h->d_in.as<float>(m.input_elems());
        OneShot& o = h->one;
        constexpr size_t kContour = kOneResults, kIris = kOneResults + sizeof(float) * 3 * MI_NUM_EYE_LANDMARKS;
        o.reserve(kIris + sizeof(float) * 3 * MI_NUM_IRIS_LANDMARKS);
        // image_to_tensor(image, roi, (64,64), keep_aspect_ratio = true, (0,1), is_right_eye) — iris_landmark.rs:188-189
        mi::image_to_tensor_enqueue(rgb, width, height, stride, roi, h->in_w, h->in_h, true, 0.0, 1.0, is_right_eye != 0, d_t,
                                    o.h<double>(kOnePad), h->d_img.as<uint8_t>(static_cast<size_t>(stride) * height), s);
        const mi::RectD* d_roi = nullptr;
        const int* d_size = nullptr;
        one_shot_roi(o, roi, width, height, &d_roi, &d_size);
        *o.h<int>(kOneFlip) = is_right_eye != 0;
        BandClaim claim(m, 1);
        auto network = [&](bool one_shot) {
            m.run_device(d_t, 1, s, one_shot);
            iris_project(h, 1, d_roi, d_size, o.d<double>(kOnePad), o.d<int>(kOneFlip), o.d<float>(kContour), o.d<float>(kIris), s);
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        };
        with_band_retry(claim.ok, [&] { return m.band_failed(); }, network);
        const float *c = o.h<float>(kContour), *ir = o.h<float>(kIris);
        for (int i = 0; i < MI_NUM_EYE_LANDMARKS; i++) contour71[i] = mi_landmark{c[3 * i], c[3 * i + 1], c[3 * i + 2]};
        for (int i = 0; i < MI_NUM_IRIS_LANDMARKS; i++) iris5[i] = mi_landmark{ir[3 * i], ir[3 * i + 1], ir[3 * i + 2]};
    });
}

}  // extern "C"
