// capi_fd.cpp — FaceDetection: the detector's entries and its streamed JPEG form.
#include "capi_internal.hpp"

namespace mi {
namespace capi {
// shared tail: raw device outputs -> detections
void fd_post(mi_fd* h, const float* d_boxes, const float* d_scores, int batch, const double* padding, mi_detection* out, int cap, int* counts,
             int mem, hipStream_t s, const FdPostPipeline* pipe) {
    mi::PostArgs a;
    if (pipe) {   // zeros behind a frame's last detection (no memset in front of the launch) and, when asked for, faces[0]'s ROI
        a.zero_rest = 1;
        a.face_rois = pipe->face_rois; a.face_valid = pipe->face_valid; a.image_w = pipe->image_w; a.image_h = pipe->image_h;
    }
    a.raw_boxes = d_boxes;
    a.raw_scores = d_scores;
    a.anchors = h->d_anchors;
    a.B = batch;
    a.N = h->n_anchors;
    a.cap = cap;
    a.scale = static_cast<float>(h->in_h);  // decode_boxes(raw_boxes, input_shape[1] as f32) — face_detection.rs:259
    const size_t n_out = static_cast<size_t>(cap) * batch;
    a.padding = stage(h->d_pad, padding, static_cast<size_t>(4) * batch, mem, s, "H2D padding");
    mi_detection* d_out = result_target(h->d_out, out, n_out, mem);
    a.out = reinterpret_cast<float*>(d_out);
    a.counts = result_target(h->d_counts, counts, batch, mem);
    // the kernel stores min(count, cap) detections per frame: the rest of the caller's host buffer reads as zeros, not as
    // whatever the staging buffer held before
    if (mem == MI_MEM_HOST) mi::hip_check(hipMemsetAsync(d_out, 0, sizeof(mi_detection) * n_out, s), "hipMemsetAsync");
    check_launch(mi::launch_postprocess(a, s), "postprocess");
    if (mem == MI_MEM_DEVICE) return;
    hand_back(out, d_out, n_out, mem, s, "D2H detections");
    hand_back(counts, a.counts, batch, mem, s, "D2H counts");
    mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    check_letterbox(counts, batch);
}

// dequantise + IDCT, then up-sampling + colour conversion: coefficients -> RGB picture, all in device memory
void jpeg_launch(const mi::JpegFrame& f, const int16_t* d_coef, const uint16_t* d_qt, uint8_t* d_planes, uint8_t* d_rgb, hipStream_t s) {
    int rc = mi::launch_jpeg_idct(f, d_coef, d_qt, d_planes, s);
    if (rc == 0) rc = mi::launch_jpeg_color(f, d_planes, d_rgb, s);
    check_launch(rc, "jpeg");
}

// submit, first half.  (1) the serial part, on this thread, while the device works on the other slot's picture: the coefficients go straight
// into the slot's pinned block, the quantisation tables behind them; (2) their copy is queued on the slot's own stream, `copied` behind it.
void jpeg_stage(JpegSlot& sl, const uint8_t* bytes, size_t nbytes) {
    sl.f.coef.ctx = &sl;
    sl.f.coef.provide = [](size_t count, void* ctx) -> int16_t* {
        JpegSlot& q = *static_cast<JpegSlot*>(ctx);
        const size_t need = count * sizeof(int16_t) + sizeof q.f.qt;
        if (need > q.coef.cap) q.coef.reserve(need + need / 4);
        return q.coef.h<int16_t>(0);
    };
    try {
        mi::jpeg_entropy_decode(bytes, nbytes, &sl.f);
    } catch (const std::runtime_error& e) {
        throw ApiError(MI_EINVAL, e.what());
    }
    const mi::JpegFrame& f = sl.f;
    const size_t coef_bytes = f.coef.size() * sizeof(int16_t);
    std::memcpy(sl.coef.h<char>(coef_bytes), f.qt, sizeof f.qt);
    sl.open();
    void* d_coef = sl.d_coef.get(coef_bytes + sizeof f.qt);
    sl.d_planes.get(mi::jpeg_plane_bytes(f));
    sl.d_rgb.get(static_cast<size_t>(3) * f.width * f.height);
    mi::hip_check(hipMemcpyAsync(d_coef, sl.coef.host, coef_bytes + sizeof f.qt, hipMemcpyHostToDevice, sl.copy), "H2D coefficients");
    mi::hip_check(hipEventRecord(sl.copied, sl.copy), "hipEventRecord");
}

// submit, second half, on the stream the networks run on: behind the copy, the sample arithmetic; the RGB picture (sl.d_rgb) stays in HBM
void jpeg_to_rgb(JpegSlot& sl, hipStream_t s) {
    mi::hip_check(hipStreamWaitEvent(s, sl.copied, 0), "hipStreamWaitEvent");
    const int16_t* d_coef = sl.d_coef.as<int16_t>();   // the quantisation tables stand behind the coefficients
    jpeg_launch(sl.f, d_coef, reinterpret_cast<const uint16_t*>(d_coef + sl.f.coef.size()), sl.d_planes.as<uint8_t>(), sl.d_rgb.as<uint8_t>(), s);
}

}  // namespace capi
}  // namespace mi

using namespace mi::capi;

extern "C" {

// ------------------------------------------------------------------------------------------------ FaceDetection
static void fd_finish_create(mi_fd* h, int kind) {
    mi::SsdOptions opts;
    if (!mi::ssd_options_for(kind, &opts)) throw ApiError(MI_EINVAL, "unsupported model type");
    h->kind = kind;
    auto d = h->model.m->input_dims();
    h->in_h = d[1];
    h->in_w = d[2];
    if (d[3] != 3) throw ApiError(MI_EMODEL, "detector input must have 3 channels");
    h->anchors = mi::ssd_generate_anchors(opts);
    h->n_anchors = static_cast<int>(h->anchors.size() / 2);
    if (h->model.m->num_outputs() < 2) throw ApiError(MI_EMODEL, "detector must have two outputs");
    const auto& rb = h->model.m->output_dims(0);
    if (rb.size() != 3 || rb[1] != h->n_anchors || rb[2] != 16 || static_cast<int>(h->model.m->output_elems(1)) != h->n_anchors)
        throw ApiError(MI_EMODEL, "detector outputs do not match the SSD anchor layout");
    if (h->in_h != opts.input_h || h->in_w != opts.input_w) throw ApiError(MI_EMODEL, "detector input size does not match SSD options");
    mi::hip_check(hipMalloc(reinterpret_cast<void**>(&h->d_anchors), h->anchors.size() * sizeof(float)), "hipMalloc anchors");
    mi::hip_check(hipMemcpy(h->d_anchors, h->anchors.data(), h->anchors.size() * sizeof(float), hipMemcpyHostToDevice), "upload anchors");
}

int mi_fd_create_from_bytes(int kind, const uint8_t* tflite, size_t nbytes, int device, mi_fd** out) {
    return guarded([&] {
        require(tflite && nbytes && out, "null argument");
        create_handle(tflite, nbytes, device, out, [&](mi_fd* h) { fd_finish_create(h, kind); });
    });
}

int mi_fd_create(int kind, const char* model_dir, int device, mi_fd** out) {
    return guarded([&] {
        require(out, "null argument");
        const char* file = mi::model_file_for(kind);
        if (!file) throw ApiError(MI_EINVAL, "unsupported model type");
        std::string dir = model_dir ? model_dir : "./models";  // face_detection.rs:157-161
        create_handle(dir + "/" + file, device, out, [&](mi_fd* h) { fd_finish_create(h, kind); });
    });
}

void mi_fd_free(mi_fd* h) { delete h; }
mi_model* mi_fd_model(mi_fd* h) { return h ? &h->model : nullptr; }

int mi_fd_input_size(const mi_fd* h, int* width, int* height) {
    if (!h) return MI_EINVAL;
    if (width) *width = h->in_w;
    if (height) *height = h->in_h;
    return MI_OK;
}
int mi_fd_num_anchors(const mi_fd* h) { return h ? h->n_anchors : MI_EINVAL; }
int mi_fd_anchors(const mi_fd* h, float* out_xy, int cap) {
    if (!h || !out_xy) return MI_EINVAL;
    int n = std::min(cap, h->n_anchors);
    std::memcpy(out_xy, h->anchors.data(), static_cast<size_t>(n) * 2 * sizeof(float));
    return n;
}

int mi_fd_infer_tensor(mi_fd* h, const float* in, int batch, const double* padding, mi_detection* out, int cap_per_frame,
                       int* counts, int mem, void* stream) {
    return guarded([&] {
        require(h && in && out && counts, "null argument");
        require(batch > 0 && cap_per_frame > 0, "batch and cap_per_frame must be positive");
        require_mem(mem);
        Call c(h->model, stream);
        c.m.run_device(stage(h->d_in, in, c.m.input_elems() * batch, mem, c.s, "H2D input"), batch, c.s);
        fd_post(h, c.m.output_device(0), c.m.output_device(1), batch, padding, out, cap_per_frame, counts, mem, c.s);
        if (mem == MI_MEM_DEVICE) c.finish(mem);   // (host memory: fd_post has synchronised)
    });
}

int mi_fd_postprocess(mi_fd* h, const float* raw_boxes, const float* raw_scores, int batch, const double* padding,
                      mi_detection* out, int cap_per_frame, int* counts, int mem, void* stream) {
    return guarded([&] {
        require(h && raw_boxes && raw_scores && out && counts, "null argument");
        require(batch > 0 && cap_per_frame > 0, "batch and cap_per_frame must be positive");
        require_mem(mem);
        Call c(h->model, stream);
        const float *db = raw_boxes, *ds = raw_scores;
        if (mem == MI_MEM_HOST) {   // (both operands in ONE block, the scores behind the boxes: not two stage() calls)
            const size_t nb = static_cast<size_t>(16) * h->n_anchors * batch, ns = static_cast<size_t>(h->n_anchors) * batch;
            float* p = h->d_in.as<float>(nb + ns);
            mi::hip_check(hipMemcpyAsync(p, raw_boxes, sizeof(float) * nb, hipMemcpyHostToDevice, c.s), "H2D boxes");
            mi::hip_check(hipMemcpyAsync(p + nb, raw_scores, sizeof(float) * ns, hipMemcpyHostToDevice, c.s), "H2D scores");
            db = p;
            ds = p + nb;
        }
        fd_post(h, db, ds, batch, padding, out, cap_per_frame, counts, mem, c.s);
        if (mem == MI_MEM_DEVICE) c.finish(mem);   // (host memory: fd_post has synchronised)
    });
}

int mi_fd_infer_image(mi_fd* h, const uint8_t* rgb, int width, int height, int stride, const mi_rect* roi, mi_detection* out,
                      int cap, int* count) {
    return guarded([&] {
        require(h && rgb && out && count, "null argument");
        require(width > 0 && height > 0 && stride >= 3 * width && cap > 0, "bad image geometry");
        Call c(h->model);
        mi::Model& m = c.m;
        const hipStream_t s = c.s;
        float* d_t = h->d_in.as<float>(m.input_elems());
        const size_t nout = sizeof(mi_detection) * static_cast<size_t>(cap);
        OneShot& o = h->one;
        o.reserve(kOneResults + nout);
        // image_to_tensor(image, roi, (w,h), keep_aspect_ratio = true, (-1,1), flip = false) — face_detection.rs:219
        mi::image_to_tensor_enqueue(rgb, width, height, stride, roi, h->in_w, h->in_h, true, -1.0, 1.0, false, d_t, o.h<double>(kOnePad),
                                    h->d_img.as<uint8_t>(static_cast<size_t>(stride) * height), s);
        BandClaim claim(m, 1);
        auto network = [&](bool one_shot) {
            std::memset(o.h<char>(kOneResults), 0, nout);  // slots beyond the count read as zeros
            m.run_device(d_t, 1, s, one_shot);
            fd_post(h, m.output_device(0), m.output_device(1), 1, o.d<double>(kOnePad), o.d<mi_detection>(kOneResults), cap, o.d<int>(kOneCount),
                    MI_MEM_DEVICE, s);
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        };
        auto failed = [&] {
            if (!m.band_failed()) return false;
            mark_suspect(h->jslot[0], h->jslot[1]);   // (the flag is the handle's: a streamed picture in flight may have raised it)
            return true;
        };
        with_band_retry(claim.ok, failed, network);
        *count = *o.h<int>(kOneCount);
        std::memcpy(out, o.h<char>(kOneResults), nout);
        check_letterbox(count, 1);
    });
}

// ---- convert_image_to_mat + FaceDetection::infer for a stream of encoded pictures (utils.rs:8-21, lib.rs:20-24), two slots.
// submit: Huffman decoding on the calling thread, straight into the slot's pinned block — the GPU is still busy with the previous picture's
// kernels — then, all asynchronous: coefficients to the device (slot's copy stream), dequantise + IDCT, up-sampling + colour conversion
// (the RGB picture stays in HBM), image_to_tensor, the network (single-launch plan when its CUs are free), post-processing into the slot's
// pinned mapped block.  collect: waits for the slot, repeats the network on the batched plan if its single launch gave up, hands the results out.

static void fd_jpeg_network(mi_fd* h, JpegSlot& sl, bool one_shot, hipStream_t s) {
    mi::Model& m = *h->model.m;
    OneShot& o = sl.one;
    float* d_t = h->d_in.as<float>(m.input_elems());
    mi::image_to_tensor_enqueue_device(sl.d_rgb.as<uint8_t>(), sl.f.width, sl.f.height, 3 * sl.f.width, nullptr, h->in_w, h->in_h, true, -1.0, 1.0, false,
                                       d_t, o.h<double>(kOnePad), s);
    std::memset(o.h<char>(kOneResults), 0, sizeof(mi_detection) * static_cast<size_t>(sl.cap));
    m.run_device(d_t, 1, s, one_shot);
    fd_post(h, m.output_device(0), m.output_device(1), 1, o.d<double>(kOnePad), o.d<mi_detection>(kOneResults), sl.cap, o.d<int>(kOneCount), MI_MEM_DEVICE, s);
}

int mi_fd_submit_jpeg(mi_fd* h, int slot, const uint8_t* bytes, size_t nbytes, int cap) {
    return guarded([&] {
        require(h && bytes, "null argument");
        require_slot(slot);
        require(cap > 0, "cap must be positive");
        JpegSlot& sl = h->jslot[slot];
        if (sl.pending) throw ApiError(MI_EINVAL, "slot holds a picture that has not been collected");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");   // (no Call yet: the decoder runs without holding the handle)
        jpeg_stage(sl, bytes, nbytes);
        sl.one.reserve(kOneResults + sizeof(mi_detection) * static_cast<size_t>(cap));
        sl.cap = cap;
        Call c(h->model);
        const hipStream_t s = c.s;
        jpeg_to_rgb(sl, s);
        sl.band = h->jclaim.acquire(m.device(), m.band_workgroups(1));
        sl.claimed = true;
        sl.suspect = false;
        fd_jpeg_network(h, sl, sl.band, s);
        mi::hip_check(hipEventRecord(sl.done, s), "hipEventRecord");
        sl.pending = true;
    });
}

int mi_fd_collect_jpeg(mi_fd* h, int slot, mi_detection* out, int cap, int* count, int* width, int* height) {
    return guarded([&] {
        require(h && out && count, "null argument");
        require_slot(slot);
        JpegSlot& sl = h->jslot[slot];
        if (!sl.pending) throw ApiError(MI_EINVAL, "nothing was submitted to this slot");
        require(cap >= sl.cap, "cap is smaller than the one the picture was submitted with");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        mi::hip_check(hipEventSynchronize(sl.done), "hipEventSynchronize");
        {
            Call c(h->model);
            const hipStream_t s = c.s;
            jpeg_collect(h->jclaim, sl, h->jslot[1 - slot], [&] { return m.band_failed(); }, [&] {
                fd_jpeg_network(h, sl, false, s);
                mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
            });
        }
        const OneShot& o = sl.one;
        *count = *o.h<int>(kOneCount);
        std::memcpy(out, o.h<char>(kOneResults), sizeof(mi_detection) * static_cast<size_t>(sl.cap));
        if (cap > sl.cap) std::memset(out + sl.cap, 0, sizeof(mi_detection) * static_cast<size_t>(cap - sl.cap));
        if (width) *width = sl.f.width;
        if (height) *height = sl.f.height;
        check_letterbox(count, 1);
    });
}

// image_to_tensor(frame, roi, (w,h), keep_aspect_ratio = true, (-1,1)) for a batch of frames already in device memory, then the
// network and the post-processing into device buffers (face_detection.rs:219-265).  d_rois: device [batch] or null.
static void fd_images_device(mi_fd* h, const uint8_t* d_frames, int batch, int width, int height, int stride, const mi::RectD* d_rois,
                             double* d_pad, mi_detection* d_out, int cap, int* d_counts, hipStream_t s) {
    mi::Model& m = *h->model.m;
    static const bool no_u8_stem = getenv("MI_NO_U8_STEM") != nullptr;  // tuning aid: always through the f32 tensor
    if (!d_rois && width == h->in_w && height == h->in_h && !no_u8_stem && m.takes_u8_input()) {
        // Frames of exactly the network's input size: image_to_tensor is the u8 -> f32 loop alone (transform.rs:292-301, no warp, no
        // letterbox, padding 0), and that loop is a 256-entry table inside the first convolution's tile load: no f32 copy of the frames
        if (!h->d_lut) {
            float lut[256];
            const double k = 1.0 - (-1.0);
            for (int v = 0; v < 256; v++) lut[v] = static_cast<float>(static_cast<double>(v) * k / 255.0 + (-1.0));
            mi::hip_check(hipMalloc(reinterpret_cast<void**>(&h->d_lut), sizeof lut), "hipMalloc lut");
            mi::hip_check(hipMemcpy(h->d_lut, lut, sizeof lut, hipMemcpyHostToDevice), "H2D lut");
        }
        m.run_device_u8(d_frames, static_cast<long>(stride) * height, stride, h->d_lut, batch, s);
        fd_post(h, m.output_device(0), m.output_device(1), batch, nullptr, d_out, cap, d_counts, MI_MEM_DEVICE, s);
        return;
    }
    mi::PreItems it = frame_items(d_frames, batch, width, height, stride);
    it.rois = d_rois; it.out_w = h->in_w; it.out_h = h->in_h; it.keep_aspect = 1;
    it.range_min = -1.0; it.range_max = 1.0;
    m.run_device(items_to_tensor(it, m, h->d_geom, h->d_in, d_pad, s), batch, s);
    fd_post(h, m.output_device(0), m.output_device(1), batch, d_pad, d_out, cap, d_counts, MI_MEM_DEVICE, s);
}

int mi_fd_infer_images(mi_fd* h, const uint8_t* frames, int batch, int width, int height, int stride, const mi_rect* rois, mi_detection* out,
                       int cap_per_frame, int* counts, int mem, void* stream) {
    return guarded([&] {
        require(h && frames && out && counts, "null argument");
        require_frames(batch, width, height, stride);
        require(cap_per_frame > 0, "bad frame geometry");
        require_mem(mem);
        static_assert(sizeof(mi::RectD) == sizeof(mi_rect), "mi_rect and RectD must have one layout");
        Call c(h->model, stream);
        const uint8_t* d_frames = stage_frames(h->d_img, frames, batch, width, height, stride, mem, c.s);
        const mi::RectD* d_rois = stage(h->d_roi, reinterpret_cast<const mi::RectD*>(rois), batch, mem, c.s, "H2D rois");
        double* d_pad = h->d_pad.as<double>(static_cast<size_t>(4) * batch);
        const size_t n_out = static_cast<size_t>(cap_per_frame) * batch;
        mi_detection* d_out = result_target(h->d_out, out, n_out, mem);
        int* d_counts = result_target(h->d_counts, counts, batch, mem);
        // unused slots of the caller's host buffer read as zeros
        if (mem == MI_MEM_HOST) mi::hip_check(hipMemsetAsync(d_out, 0, sizeof(mi_detection) * n_out, c.s), "hipMemsetAsync");
        fd_images_device(h, d_frames, batch, width, height, stride, d_rois, d_pad, d_out, cap_per_frame, d_counts, c.s);
        hand_back(out, d_out, n_out, mem, c.s, "D2H detections");
        hand_back(counts, d_counts, batch, mem, c.s, "D2H counts");
        c.finish(mem);
        if (mem == MI_MEM_HOST) check_letterbox(counts, batch);
    });
}

int mi_fd_submit_images(mi_fd* h, int slot, const uint8_t* frames, int batch, int width, int height, int stride, int cap_per_frame) {
    return guarded([&] {
        require(h && frames, "null argument");
        require_slot(slot);
        require_frames(batch, width, height, stride);
        require(cap_per_frame > 0, "bad frame geometry");
        Call c(h->model);
        const hipStream_t s = c.s;
        FdSlot& sl = h->slot[slot];
        if (sl.pending) throw ApiError(MI_EINVAL, "slot still holds an uncollected batch (call mi_fd_collect first)");
        sl.open();
        const size_t nout = sizeof(mi_detection) * static_cast<size_t>(cap_per_frame) * batch, ncnt = sizeof(int) * batch;
        sl.out.reserve(nout + ncnt);
        // frames: host -> device on the slot's copy stream (asynchronous when `frames` is pinned memory: mi_host_alloc);
        // everything else on the handle's stream, behind the copy.  The post-processing kernel writes detections and counts
        // straight into the slot's pinned host block (mapped into the device's address space): a hipMemcpyAsync of the results
        // blocked the host for whole batches on this runtime (measured: every third call, 7 ms).
        const uint8_t* d_frames = stage_frames(sl.d_frames, frames, batch, width, height, stride, MI_MEM_HOST, sl.copy);
        mi::hip_check(hipEventRecord(sl.copied, sl.copy), "hipEventRecord");
        mi::hip_check(hipStreamWaitEvent(s, sl.copied, 0), "hipStreamWaitEvent");
        std::memset(sl.out.host, 0, nout + ncnt);  // slots beyond a frame's count read as zeros (the slot was collected: nothing in flight writes here)
        double* d_pad = sl.d_pad.as<double>(static_cast<size_t>(4) * batch);
        try {
            fd_images_device(h, d_frames, batch, width, height, stride, nullptr, d_pad, sl.out.d<mi_detection>(0), cap_per_frame, sl.out.d<int>(nout), s);
        } catch (...) {
            (void)hipStreamSynchronize(sl.copy);   //  the queued copy may still be reading the caller's frames: not after we return
            throw;
        }
        mi::hip_check(hipEventRecord(sl.done, s), "hipEventRecord");
        sl.batch = batch; sl.cap = cap_per_frame; sl.pending = true;
    });
}

int mi_fd_collect(mi_fd* h, int slot, mi_detection* out, int* counts) {
    return guarded([&] {
        require(h && out && counts, "null argument");
        require_slot(slot);
        FdSlot& sl = h->slot[slot];
        int batch = 0;
        slot_collect(h->model, sl, [&] {
            batch = sl.batch;
            const size_t nout = sizeof(mi_detection) * static_cast<size_t>(sl.cap) * batch;
            std::memcpy(out, sl.out.host, nout);
            std::memcpy(counts, sl.out.h<char>(nout), sizeof(int) * batch);
        });
        check_letterbox(counts, batch);
    });
}

}  // extern "C"
