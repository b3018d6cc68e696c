// capi_core.cpp — mi_last_error, version and device count, the L0 model entries, pinned host memory and the host helpers.
#include "capi_internal.hpp"

#include <cmath>
#include <cstdio>
#include <fstream>

namespace {
thread_local std::string g_error;
}

namespace mi {
namespace capi {

void set_last_error(const std::string& message) { g_error = message; }
const std::string& last_error() { return g_error; }

std::atomic<int> g_band_cus[64];

std::vector<uint8_t> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw ApiError(MI_EIO, "cannot open model file '" + path + "'");
    std::vector<uint8_t> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (data.empty()) throw ApiError(MI_EIO, "model file '" + path + "' is empty");
    return data;
}

}  // namespace capi
}  // namespace mi

using namespace mi::capi;

static void load_model(const uint8_t* tflite, size_t nbytes, int device, mi_model** out) {
    auto h = std::make_unique<mi_model>();
    h->m = std::make_unique<mi::Model>(tflite, nbytes, device);
    *out = h.release();
}

// the describe entries' way out: as much of `s` as fits into buf[cap], terminated; returns the size the whole text needs
static size_t copy_string(const std::string& s, char* buf, size_t cap) {
    if (buf && cap) {
        size_t k = std::min(cap - 1, s.size());
        std::memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return s.size() + 1;
}

extern "C" {

const char* mi_last_error(void) { return g_error.c_str(); }
const char* mi_version(void) { return "mi_face 0.1 (gfx950)"; }

int mi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------------------------ L0
int mi_model_load_bytes(const uint8_t* tflite, size_t nbytes, int device, mi_model** out) {
    return guarded([&] {
        require(tflite && nbytes && out, "null argument");
        load_model(tflite, nbytes, device, out);
    });
}

int mi_model_load_file(const char* path, int device, mi_model** out) {
    return guarded([&] {
        require(path && out, "null argument");
        const auto bytes = read_file(path);
        load_model(bytes.data(), bytes.size(), device, out);
    });
}

void mi_model_free(mi_model* m) { delete m; }

int mi_model_input_dims(const mi_model* m, int dims[4]) {
    return guarded([&] {
        require(m && dims, "null argument");
        auto d = m->m->input_dims();
        for (int i = 0; i < 4; i++) dims[i] = d[i];
    });
}

int mi_model_num_outputs(const mi_model* m) { return m ? m->m->num_outputs() : MI_EINVAL; }

int mi_model_output_dims(const mi_model* m, int index, int dims[4], int* rank) {
    return guarded([&] {
        require(m && dims, "null argument");
        require(index >= 0 && index < m->m->num_outputs(), "output index out of range");
        const auto& d = m->m->output_dims(index);
        for (int i = 0; i < 4; i++) dims[i] = i < static_cast<int>(d.size()) ? d[i] : 1;
        if (rank) *rank = static_cast<int>(d.size());
    });
}

size_t mi_model_output_elems(const mi_model* m, int index) {
    if (!m || index < 0 || index >= m->m->num_outputs()) return 0;
    return m->m->output_elems(index);
}

int mi_model_run(mi_model* m, const float* in, int batch, float* const* outs, int mem, void* stream) {
    return guarded([&] {
        require(m && in && outs, "null argument");
        require(batch > 0, "batch must be positive");
        require_mem(mem);
        Call c(*m, stream);
        c.m.run(in, batch, outs, mem, static_cast<hipStream_t>(stream));
    });
}

int mi_model_debug_tensor(mi_model* m, int tensor_index, int frame, float* dst, size_t cap, size_t* n) {
    return guarded([&] {
        require(m && dst, "null argument");
        std::lock_guard<std::mutex> lock(m->mu);
        size_t got = m->m->debug_tensor(tensor_index, frame, dst, cap);
        if (n) *n = got;
    });
}

size_t mi_model_describe(const mi_model* m, char* buf, size_t cap) {
    if (!m) return 0;
    std::string s = m->m->describe();
    return copy_string(s, buf, cap);
}

size_t mi_plan_describe(const uint8_t* tflite, size_t nbytes, int fuse_level, char* buf, size_t cap) {
    size_t need = 0;
    int rc = guarded([&] {
        require(tflite && nbytes, "null argument");
        std::string s = mi::build_plan(mi::parse_tflite(tflite, nbytes), fuse_level).describe();
        need = copy_string(s, buf, cap);
    });
    return rc == MI_OK ? need : 0;
}

int mi_model_set_option(mi_model* m, const char* key, int value) {
    return guarded([&] {
        require(m && key, "null argument");
        std::lock_guard<std::mutex> lock(m->mu);
        m->m->set_option(key, value);
    });
}

int mi_model_get_option(mi_model* m, const char* key, int* value) {
    return guarded([&] {
        require(m && key && value, "null argument");
        std::lock_guard<std::mutex> lock(m->mu);
        *value = m->m->get_option(key);
    });
}

size_t mi_model_profile(mi_model* m, const float* in_device, int batch, int reps, char* buf, size_t cap) {
    size_t need = 0;
    int rc = guarded([&] {
        require(m && in_device, "null argument");
        require(batch > 0 && reps > 0, "batch and reps must be positive");
        std::lock_guard<std::mutex> lock(m->mu);
        auto stats = m->m->profile(in_device, batch, reps, nullptr);
        std::string s = "[";
        char line[512];
        for (size_t i = 0; i < stats.size(); i++) {
            std::snprintf(line, sizeof line, "%s{\"kernel\": \"%s\", \"shape\": \"%s\", \"ms\": %.6f, \"bytes\": %.0f, \"macs\": %.0f}", i ? ", " : "",
                          stats[i].kernel.c_str(), stats[i].detail.c_str(), stats[i].ms, stats[i].bytes, stats[i].macs);
            s += line;
        }
        s += "]";
        need = copy_string(s, buf, cap);
    });
    return rc == MI_OK ? need : 0;
}

int mi_model_single_launch_workgroups(mi_model* m, int batch) {
    int n = 0;
    int rc = guarded([&] {
        require(m && m->m, "null argument");
        require(batch > 0, "batch must be positive");
        std::lock_guard<std::mutex> g(m->mu);
        mi::hip_check(hipSetDevice(m->m->device()), "hipSetDevice");
        n = m->m->band_workgroups(batch);
    });
    return rc == MI_OK ? n : rc;
}

int mi_model_plan_stats(const mi_model* m, double* bytes_per_frame, double* macs_per_frame, int* launches) {
    return guarded([&] {
        require(m, "null argument");
        if (bytes_per_frame) *bytes_per_frame = m->m->plan().bytes_per_frame;
        if (macs_per_frame) *macs_per_frame = m->m->plan().macs_per_frame;
        if (launches) {
            int n = 0;
            for (const auto& nd : m->m->plan().nodes) n += !(nd.kind == mi::Node::Reshape || nd.kind == mi::Node::Concat);
            *launches = n;
        }
    });
}

int mi_host_alloc(size_t bytes, void** out) {
    return guarded([&] {
        require(out && bytes > 0, "null argument");
        *out = nullptr;
        mi::hip_check(hipHostMalloc(out, bytes, hipHostMallocDefault), "hipHostMalloc");
    });
}
void mi_host_free(void* p) {
    if (p) hipHostFree(p);
}

// ------------------------------------------------------------------------------------------------ host helpers
int mi_bbox_to_roi(const double bbox[4], int image_w, int image_h, const double* rotation_keypoints, double scale_x, double scale_y, int size_mode,
                   mi_rect* out) {
    return guarded([&] {
        require(bbox && out, "null argument");
        require(size_mode >= 0 && size_mode <= 2, "size_mode must be 0 (Default), 1 (SquareLong) or 2 (SquareShort)");
        if (!mi::bbox_to_roi(bbox, image_w, image_h, rotation_keypoints, scale_x, scale_y, size_mode, out)) throw ApiError(MI_EINVAL, "bbox must be normalized");
    });
}

int mi_bbox_from_landmarks(const mi_landmark* lm, int count, double bbox_out[4]) {
    return guarded([&] {
        require(lm && bbox_out, "null argument");
        if (count < 2) throw ApiError(MI_EINVAL, "landmarks must contain at least 2 items");  // transform.rs:147-149
        double xmin = INFINITY, ymin = INFINITY, xmax = -INFINITY, ymax = -INFINITY;
        for (int i = 0; i < count; i++) {  // f64::min / max: a NaN operand is ignored, like fmin / fmax
            xmin = std::fmin(xmin, lm[i].x); ymin = std::fmin(ymin, lm[i].y);
            xmax = std::fmax(xmax, lm[i].x); ymax = std::fmax(ymax, lm[i].y);
        }
        bbox_out[0] = xmin; bbox_out[1] = ymin; bbox_out[2] = xmax; bbox_out[3] = ymax;
    });
}

int mi_face_detection_to_roi(const mi_detection* det, int image_w, int image_h, mi_rect* out) {
    return guarded([&] {
        require(det && out, "null argument");
        // Detection::scaled_by_image_size multiplies in f32 (types.rs:237-245); keypoints 0/1 = eyes (face_detection.rs:91-98)
        const float w = static_cast<float>(image_w), hgt = static_cast<float>(image_h);
        const float lx = det->data[4] * w, ly = det->data[5] * hgt, rx = det->data[6] * w, ry = det->data[7] * hgt;
        const double kp[4] = {lx, ly, rx, ry};
        const double bbox[4] = {det->data[0], det->data[1], det->data[2], det->data[3]};
        if (!mi::bbox_to_roi(bbox, image_w, image_h, kp, 1.5, 1.5, 1, out)) throw ApiError(MI_EINVAL, "bbox must be normalized");
    });
}

int mi_iris_roi_from_face_landmarks(const mi_landmark* lm, int image_w, int image_h, mi_rect* left_eye, mi_rect* right_eye) {
    return guarded([&] {
        require(lm && left_eye && right_eye, "null argument");
        const int idx[2][2] = {{33, 133}, {362, 263}};  // iris_landmark.rs:29-35
        mi_rect* outs[2] = {left_eye, right_eye};
        for (int e = 0; e < 2; e++) {
            const mi_landmark &a = lm[idx[e][0]], &b = lm[idx[e][1]];
            const double bbox[4] = {std::fmin(a.x, b.x), std::fmin(a.y, b.y), std::fmax(a.x, b.x), std::fmax(a.y, b.y)};
            const double kp[4] = {a.x, a.y, b.x, b.y};
            if (!mi::bbox_to_roi(bbox, image_w, image_h, kp, 2.3, 2.3, 1, outs[e])) throw ApiError(MI_EINVAL, "bbox must be normalized");
        }
    });
}

int mi_jpeg_info(const uint8_t* bytes, size_t nbytes, int* width, int* height) {
    return guarded([&] {
        require(bytes && width && height, "null argument");
        try {
            mi::jpeg_parse_size(bytes, nbytes, width, height);
        } catch (const std::runtime_error& e) {
            throw ApiError(MI_EINVAL, e.what());
        }
    });
}

int mi_jpeg_decode_rgb(int device, const uint8_t* bytes, size_t nbytes, uint8_t* rgb, size_t cap_bytes, int* width, int* height, int mem, void* stream) {
    return guarded([&] {
        require(bytes && rgb && width && height, "null argument");
        require_mem(mem);
        mi::JpegFrame f;
        try {
            mi::jpeg_entropy_decode(bytes, nbytes, &f);  // host: the serial part
        } catch (const std::runtime_error& e) {
            throw ApiError(MI_EINVAL, e.what());
        }
        const size_t out_bytes = static_cast<size_t>(3) * f.width * f.height;
        if (cap_bytes < out_bytes) throw ApiError(MI_EINVAL, "rgb buffer too small for the decoded picture");
        select_device(device, "no such HIP device (the JPEG sample arithmetic runs on the GPU; no CPU fallback exists)");
        hipStream_t s = static_cast<hipStream_t>(stream);
        DeviceBuf coef, qt, planes, out;
        uint8_t* d_rgb = result_target(out, rgb, out_bytes, mem);
        const int16_t* d_coef = stage(coef, f.coef.data(), f.coef.size(), MI_MEM_HOST, s, "H2D coefficients");
        const uint16_t* d_qt = stage(qt, &f.qt[0][0], sizeof f.qt / sizeof(uint16_t), MI_MEM_HOST, s, "H2D quantisation tables");
        jpeg_launch(f, d_coef, d_qt, planes.as<uint8_t>(mi::jpeg_plane_bytes(f)), d_rgb, s);
        hand_back(rgb, d_rgb, out_bytes, mem, s, "D2H rgb");
        mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");  // the scratch buffers and the host coefficients die with this call
        *width = f.width;
        *height = f.height;
    });
}

namespace {
// eye-contour landmark n of the iris model refines face-mesh landmark kEyeToFace[eye][n] (iris_landmark.rs:64-95)
const int kEyeToFace[2][MI_NUM_EYE_LANDMARKS] = {
    {
        33, 7, 163, 144, 145, 153, 154, 155, 133, 246, 161, 160, 159, 158, 157, 173, 130, 25, 110, 24, 23,
        22, 26, 112, 243, 247, 30, 29, 27, 28, 56, 190, 226, 31, 228, 229, 230, 231, 232, 233, 244, 113, 225,
        224, 223, 222, 221, 189, 35, 124, 46, 53, 52, 65, 143, 111, 117, 118, 119, 120, 121, 128, 245, 156,
        70, 63, 105, 66, 107, 55, 193,
    },
    {
        263, 249, 390, 373, 374, 380, 381, 382, 362, 466, 388, 387, 386, 385, 384, 398, 359, 255, 339, 254,
        253, 252, 256, 341, 463, 467, 260, 259, 257, 258, 286, 414, 446, 261, 448, 449, 450, 451, 452, 453,
        464, 342, 445, 444, 443, 442, 441, 413, 265, 353, 276, 283, 282, 295, 372, 340, 346, 347, 348, 349,
        350, 357, 465, 383, 300, 293, 334, 296, 336, 285, 417,
    },
};
}  // namespace

int mi_update_face_landmarks_with_iris_results(const mi_landmark* face, const mi_landmark* left, const mi_landmark* right, mi_landmark* out) {
    return guarded([&] {
        require(face && left && right && out, "null argument");
        if (out != face) std::memmove(out, face, sizeof(mi_landmark) * MI_NUM_FACE_LANDMARKS);
        const mi_landmark* eyes[2] = {left, right};  // left first, then right, as the reference's two loops
        for (int e = 0; e < 2; e++)
            for (int n = 0; n < MI_NUM_EYE_LANDMARKS; n++) out[kEyeToFace[e][n]] = eyes[e][n];
    });
}

int mi_image_to_tensor(int device, const uint8_t* rgb, int width, int height, int stride, const mi_rect* roi, int out_w, int out_h,
                       int keep_aspect_ratio, double range_min, double range_max, int flip_horizontal, float* out,
                       double padding_out[4], int mem, void* stream) {
    return guarded([&] {
        require(rgb && out && padding_out, "null argument");
        require(width > 0 && height > 0 && stride >= 3 * width && out_w > 0 && out_h > 0, "bad image geometry");
        require_mem(mem);
        select_device(device, "no such HIP device");
        hipStream_t s = static_cast<hipStream_t>(stream);
        DeviceBuf img, outbuf;
        const size_t out_elems = static_cast<size_t>(3) * out_w * out_h;
        float* d_out = result_target(outbuf, out, out_elems, mem);
        mi::image_to_tensor_device(rgb, width, height, stride, roi, out_w, out_h, keep_aspect_ratio != 0, range_min, range_max,
                                   flip_horizontal != 0, d_out, padding_out, img.get(mi::image_to_tensor_scratch_bytes(width, height, stride, roi, out_w, out_h, keep_aspect_ratio != 0)), s);
        hand_back(out, d_out, out_elems, mem, s, "D2H tensor");
        mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    });
}

}  // extern "C"
