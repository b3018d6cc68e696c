// capi_internal.hpp — what the units of the extern "C" boundary (capi_*.cpp, include/mi_face.h) share.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mi_face.h"
#include "embed.hpp"
#include "engine.hpp"
#include "face_chip.hpp"
#include "face_items.hpp"
#include "launch.hpp"
#include "host_glue.hpp"
#include "kernels.hpp"
#include "jpeg.hpp"
#include "preproc.hpp"
#include "render.hpp"
#include "topk.hpp"

// Layout: capi_core.cpp (last error, L0 model, host helpers), capi_fd.cpp (detector + its JPEG stream), capi_landmarks.cpp (mesh, iris),
// capi_pipeline.cpp, capi_tracker.cpp (mi_tracker around a private pipeline: capi_pipeline.hpp), capi_render.cpp, capi_embed.cpp (embeddings, similarity, top-k, gallery), capi_dist.cpp (RCCL broadcast, stream probing).
// Everything here that is not a handle struct of the C header lives in mi::capi, which is hidden: libmiface.so exports the mi_* entries only.
#define MI_CAPI_BEGIN namespace mi { namespace capi __attribute__((visibility("hidden"))) {
#define MI_CAPI_END } }

// Concurrency (face_detection.rs:205: `infer(&self)` may be called from several threads): a handle's interpreter state —
// activation arena, captured hipGraphs, staging buffers — is shared by its callers, so calls on one handle are SERIALISED
// by `mu`, and because a call on a caller-supplied stream returns before its kernels finish, the next call on a
// DIFFERENT stream first waits (on the device, hipStreamWaitEvent) for the event the previous call recorded.  Results
// are therefore the same as with one caller; for parallel execution use one handle per worker thread / stream.
struct mi_model {
    std::unique_ptr<mi::Model> m;
    std::mutex mu;
    hipEvent_t done = nullptr;     // recorded after the last enqueued call
    hipStream_t last = nullptr;    // stream of that call
    bool busy = false;
    ~mi_model() {
        if (done) (void)hipEventDestroy(done);
    }
};

MI_CAPI_BEGIN

// the calling thread's mi_last_error() text: one definition, in capi_core.cpp
void set_last_error(const std::string& message);
const std::string& last_error();

struct ApiError : std::runtime_error {
    int code;
    ApiError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

template <typename F>
int guarded(F&& f) {
    try {
        f();
        return MI_OK;
    } catch (const ApiError& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("out of memory");
        return MI_ENOMEM;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        std::string m = e.what();
        if (m.rfind("tflite:", 0) == 0 || m.rfind("plan:", 0) == 0) return MI_EMODEL;
        if (m.find("hip") != std::string::npos || m.find("HIP") != std::string::npos || m.find("device") != std::string::npos ||
            m.find("kernel") != std::string::npos)
            return MI_EDEVICE;
        return MI_EINVAL;
    } catch (...) {
        set_last_error("unknown error");
        return MI_EINVAL;
    }
}

inline void require(bool ok, const char* msg) {
    if (!ok) throw ApiError(MI_EINVAL, msg);
}
inline void require_mem(int mem) { require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE"); }
inline void require_slot(int slot) { require(slot == 0 || slot == 1, "slot must be 0 or 1"); }
// `batch` frames of width x height RGB pixels, rows `stride` bytes apart
inline void require_frames(int batch, int width, int height, int stride) {
    require(batch > 0 && width > 0 && height > 0 && stride >= 3 * width, "bad frame geometry");
}
// the bytes those frames own: the last frame's last row owns row_bytes (3 * width of an RGB picture), not a whole stride
inline size_t frames_bytes(int batch, int height, int stride, size_t row_bytes) {
    return static_cast<size_t>(stride) * height * (batch - 1) + static_cast<size_t>(stride) * (height - 1) + row_bytes;
}

// a launch wrapper's return code (int or hipError_t) -> "<what> kernel launch failed: <hip string>", which guarded() reports as MI_EDEVICE
template <class Rc>
void check_launch(Rc rc, const char* what) {
    if (rc) throw std::runtime_error(std::string(what) + " kernel launch failed: " + hipGetErrorString(static_cast<hipError_t>(rc)));
}

// the device of an entry that takes a device number instead of a handle; `missing` is the entry's own wording of "no such HIP device"
inline void select_device(int device, const char* missing) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) throw ApiError(MI_EDEVICE, missing);
    mi::hip_check(hipSetDevice(device), "hipSetDevice");
}

// small device scratch that grows on demand
struct DeviceBuf {
    void* p = nullptr;
    size_t cap = 0;
    void* get(size_t bytes) {
        if (bytes > cap) {
            if (p) (void)hipFree(p);
            p = nullptr;
            mi::hip_check(hipMalloc(&p, bytes), "hipMalloc scratch");
            cap = bytes;
        }
        return p;
    }
    template <class T> T* as(size_t count) { return static_cast<T*>(get(sizeof(T) * count)); }
    template <class T> T* as() const { return static_cast<T*>(p); }   // what the last get() / as(count) returned
    ~DeviceBuf() {
        if (p) (void)hipFree(p);
    }
};

// `count` elements at `src` as the kernels can read them.  Host memory: their image in `buf`, the copy queued on `s` (`what` names it in
// mi_last_error()).  Device memory, or no operand at all: `src` itself.
template <class T>
const T* stage(DeviceBuf& buf, const T* src, size_t count, int mem, hipStream_t s, const char* what) {
    if (!src || mem == MI_MEM_DEVICE) return src;
    T* d = buf.as<T>(count);
    mi::hip_check(hipMemcpyAsync(d, src, sizeof(T) * count, hipMemcpyHostToDevice, s), what);
    return d;
}
// The same for `batch` RGB frames: whole strides are reserved, the bytes the frames own are copied.  The submit entries pass their slot's
// buffer and copy stream.
inline const uint8_t* stage_frames(DeviceBuf& buf, const uint8_t* frames, int batch, int width, int height, int stride, int mem, hipStream_t s) {
    if (mem == MI_MEM_DEVICE) return frames;
    uint8_t* d = buf.as<uint8_t>(static_cast<size_t>(stride) * height * batch);
    mi::hip_check(hipMemcpyAsync(d, frames, frames_bytes(batch, height, stride, static_cast<size_t>(3) * width), hipMemcpyHostToDevice, s), "H2D frames");
    return d;
}
// Where a kernel writes `count` results the caller wants at `dst`: device memory: `dst` itself; host memory: `buf`, and hand_back() queues
// the copy to `dst` behind the kernel (no copy for a null `dst`: an optional result the caller did not ask for).
template <class T>
T* result_target(DeviceBuf& buf, T* dst, size_t count, int mem) {
    return mem == MI_MEM_DEVICE ? dst : buf.as<T>(count);
}
template <class T>
void hand_back(T* dst, const T* d_src, size_t count, int mem, hipStream_t s, const char* what) {
    if (dst && mem == MI_MEM_HOST) mi::hip_check(hipMemcpyAsync(dst, d_src, sizeof(T) * count, hipMemcpyDeviceToHost, s), what);
}

// The single-image entries (one picture per call: the reference's only operating point, face_detection.rs:205) keep every small
// operand and every result of a call in ONE pinned host block that is mapped into the device's address space: the kernels read the
// padding / ROI / flags from it and write their results into it.  A call is then: one copy of the picture, the pre-processing launch,
// the network's graph, the post-processing launch and ONE synchronisation, with no small copies either way.
// The slots of the two-slot entries keep their results in such a block too; `mapped = false` gives plain pinned memory that only copies
// read (the streamed JPEG form's coefficients): no device pointer.
struct OneShot {
    void* host = nullptr;
    void* dev = nullptr;
    size_t cap = 0;
    const bool mapped;
    explicit OneShot(bool mapped_coherent = true) : mapped(mapped_coherent) {}
    void reserve(size_t bytes) {
        if (bytes <= cap) return;
        if (host) (void)hipHostFree(host);
        host = dev = nullptr;
        cap = 0;
        // (coherent: the kernels' stores must be visible to the host once the stream has been synchronised, without a copy)
        mi::hip_check(hipHostMalloc(&host, bytes, mapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault),
                      mapped ? "hipHostMalloc" : "hipHostMalloc coefficients");
        if (mapped) mi::hip_check(hipHostGetDevicePointer(&dev, host, 0), "hipHostGetDevicePointer");
        cap = bytes;
    }
    template <class T> T* h(size_t off) const { return reinterpret_cast<T*>(static_cast<char*>(host) + off); }
    template <class T> T* d(size_t off) const { return reinterpret_cast<T*>(static_cast<char*>(dev) + off); }
    ~OneShot() {
        if (host) (void)hipHostFree(host);
    }
};
// A single-launch run (bandnet_kernels.hip) needs every one of its workgroups resident, one per CU, until it has finished: the handles of
// a process share the device's CUs through this count.  A call that does not get its CUs runs on the batched plan instead — it never waits.
// (ONE definition, in capi_core.cpp: a second table would let two handles claim the same CUs)
extern std::atomic<int> g_band_cus[64];
struct BandClaim {
    int dev = 0, n = 0;
    bool ok = false;
    BandClaim(mi::Model& m, int batch) : BandClaim(m.device(), m.band_workgroups(batch)) {}
    // (launches that follow one another on one stream share a claim of the largest of them)
    BandClaim(int device, int workgroups) {
        dev = device;
        n = workgroups;
        if (n <= 0 || dev < 0 || dev >= 64) return;
        // A CU mask (HSA_CU_MASK / ROC_GLOBAL_CU_MASK) takes CUs away that hipDeviceAttributeMultiprocessorCount still counts: the launch's
        // workgroups would not all be resident, every call would wait out the kernel's bounded spin and then repeat itself.  Under a
        // mask the single-image entries stay on the batched plan (MI_BAND_WITH_CU_MASK=1: the mask leaves enough CUs, use the plan anyway).
        static const bool masked = (getenv("HSA_CU_MASK") || getenv("ROC_GLOBAL_CU_MASK")) && !getenv("MI_BAND_WITH_CU_MASK");
        if (masked) return;
        if (g_band_cus[dev].fetch_add(n) + n <= mi::device_cu_count()) ok = true;
        else g_band_cus[dev].fetch_sub(n);
    }
    ~BandClaim() {
        if (ok) g_band_cus[dev].fetch_sub(n);
    }
    BandClaim(const BandClaim&) = delete;
    BandClaim& operator=(const BandClaim&) = delete;
};
// The claim of a streamed form (mi_fd_submit_jpeg / mi_pipeline_submit_jpeg): both slots run on one stream, so the handle holds ONE claim
// while any of its streamed pictures is in flight.  acquire() at submit tells whether the picture may take the single-launch plan;
// release() when a picture that acquired is collected.
struct StreamClaim {
    std::unique_ptr<BandClaim> claim;
    int users = 0;
    bool acquire(int device, int workgroups) {
        if (users == 0) claim.reset(new BandClaim(device, workgroups));
        users++;
        return claim && claim->ok;
    }
    void release() {
        if (--users == 0) claim.reset();
    }
};
// offsets of the small operands inside the block; results start at kOneResults
constexpr size_t kOnePad = 0, kOneRoi = 64, kOneSize = 128, kOneFlip = 136, kOneCount = 192, kOneResults = 256;

// a negative count is the post-processing kernel's report of a letterbox it cannot undo
inline void check_letterbox(const int* counts, int n) {
    for (int b = 0; b < n; b++)
        if (counts[b] < 0) throw ApiError(MI_ERANGE, "letterbox scale is too small (reference asserts at transform.rs:121-122)");
}

// One picture per call on the single-launch plan: `network(one_shot)` enqueues the call's work and synchronises; `failed()` asks the
// models' flags afterwards.  A launch that did not get its CUs (someone else's kernels hold them) leaves void results: the call is
// repeated on the batched plan.  Without the claim the first run is the batched plan already.
template <class Failed, class Network>
void with_band_retry(bool claim_ok, Failed failed, Network network) {
    network(claim_ok);
    if (claim_ok && failed()) network(false);
}

// What the two-slot entries' slots share: the slot's own copy stream, `copied` (the upload has been queued in full) and `done` (so has
// everything that writes the slot's results), and whether a submission waits to be collected.
struct SlotSync {
    hipStream_t copy = nullptr;
    hipEvent_t copied = nullptr, done = nullptr;
    bool pending = false;
    SlotSync() = default;
    SlotSync(const SlotSync&) = delete;
    void open() {   // on first use
        if (!copy) mi::hip_check(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking), "hipStreamCreate");
        if (!copied) mi::hip_check(hipEventCreateWithFlags(&copied, hipEventDisableTiming), "hipEventCreate");
        if (!done) mi::hip_check(hipEventCreateWithFlags(&done, hipEventDisableTiming), "hipEventCreate");
    }
    // submitted and never collected: its kernels still read and write the slot's and the handle's buffers.  A slot's own buffers die
    // BEFORE this base does, and the handle's may go first too: both destructors call wait() before they free anything.
    void wait() {
        if (pending && done) (void)hipEventSynchronize(done);
    }
    ~SlotSync() {
        wait();
        if (copy) (void)hipStreamDestroy(copy);
        if (copied) (void)hipEventDestroy(copied);
        if (done) (void)hipEventDestroy(done);
    }
};

// One call's claim on a handle: holds the mutex, orders this call's stream after the previous call's work.
// Construct after hipSetDevice; the destructor (also on the error paths) records the new tail of the handle's work.
struct Use {
    mi_model& h;
    hipStream_t s;
    std::unique_lock<std::mutex> lock;
    Use(mi_model& handle, hipStream_t stream) : h(handle), s(stream), lock(handle.mu) {
        if (h.busy && h.last != s) mi::hip_check(hipStreamWaitEvent(s, h.done, 0), "hipStreamWaitEvent");
    }
    ~Use() {
        if (!h.done && hipEventCreateWithFlags(&h.done, hipEventDisableTiming) != hipSuccess) h.done = nullptr;
        if (h.done && hipEventRecord(h.done, s) == hipSuccess) {
            h.last = s;
            h.busy = true;
        }
    }
};

// The usual ending of an entry: results in host memory, or a call that was not given a stream of the caller's, are complete when the
// entry returns; a call on the caller's stream with device memory returns with its work queued.
inline void finish(int mem, bool caller_stream, hipStream_t s) {
    if (mem == MI_MEM_HOST || !caller_stream) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
}

// The prologue of an entry on a handle: the handle's device, the caller's stream or else the handle's own, and the claim on the handle
// (Use) for as long as the call lasts.  The argument checks stand in front of it: a Call is the first thing that touches the device.
struct Call {
    mi::Model& m;
    const bool caller_stream;
    hipStream_t s;
    Use use;
    explicit Call(mi_model& h, void* stream = nullptr) : m(*h.m), caller_stream(stream != nullptr), s(enter(m, stream)), use(h, s) {}
    void sync() const { mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize"); }
    void finish(int mem) const { capi::finish(mem, caller_stream, s); }

private:
    static hipStream_t enter(mi::Model& m, void* stream) {
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        return stream ? static_cast<hipStream_t>(stream) : m.stream();
    }
};

std::vector<uint8_t> read_file(const std::string& path);

// What a *_create / *_create_from_bytes pair does behind its argument checks: the network from the model's bytes, then the handle's own
// checks and set-up (`finish(handle)`); `out` is written only when all of it went well.
template <class H, class Finish>
void create_handle(const uint8_t* tflite, size_t nbytes, int device, H** out, Finish finish) {
    auto h = std::make_unique<H>();
    h->model.m = std::make_unique<mi::Model>(tflite, nbytes, device);
    finish(h.get());
    *out = h.release();
}
template <class H, class Finish>
void create_handle(const std::string& path, int device, H** out, Finish finish) {
    const auto bytes = read_file(path);
    create_handle(bytes.data(), bytes.size(), device, out, finish);
}

// `batch` frames in device memory as pre-processing items, one item per frame: the caller sets what differs (ROIs, flips, items per frame
// and N, the output size, keep_aspect, the range)
inline mi::PreItems frame_items(const uint8_t* d_frames, int batch, int width, int height, int stride) {
    mi::PreItems it{};
    it.frames = d_frames; it.frame_bytes = static_cast<long>(stride) * height; it.width = width; it.height = height; it.stride = stride;
    it.items_per_frame = 1; it.N = batch;
    return it;
}
// image_to_tensor of the items of `it` into `in`, the network's input buffer (a handle's own, so that its address stays the same from call
// to call: the engine keys its captured graphs by it); d_pad: [N][4] letterbox paddings out, or null
inline float* items_to_tensor(const mi::PreItems& it, mi::Model& m, DeviceBuf& geom, DeviceBuf& in, double* d_pad, hipStream_t s) {
    auto* d_geom = geom.as<mi::PreGeom>(it.N);
    float* d_in = in.as<float>(m.input_elems() * it.N);
    mi::launch_pre_geom(it, d_geom, d_pad, s);
    mi::launch_pre_tensor(it, d_geom, d_in, s);
    return d_in;
}

// (w, h) of the source image for every item of a batch of equally sized frames, on the device (Rect::scaled in project_landmarks); a host
// round trip only when the batch geometry changes.  N, w, h say what `buf` holds.
struct SizesCache {
    DeviceBuf buf;
    int N = 0, w = 0, h = 0;
    int* get(int items, int width, int height, hipStream_t s) {
        int* d = buf.as<int>(2 * static_cast<size_t>(items));
        if (N != items || w != width || h != height) {
            std::vector<int> hs(2 * static_cast<size_t>(items));
            for (int i = 0; i < items; i++) { hs[2 * i] = width; hs[2 * i + 1] = height; }
            N = 0;
            mi::hip_check(hipMemcpyAsync(d, hs.data(), hs.size() * sizeof(int), hipMemcpyHostToDevice, s), "H2D sizes");
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");  // hs is a host temporary
            N = items; w = width; h = height;
        }
        return d;
    }
};

// One of the two slots of the host-fed batch form (mi_fd_submit_images / mi_fd_collect): its own copy stream, device frames
// and results, pinned host results.  The network itself runs on the handle's stream (one arena per handle), so the copies
// of one slot overlap the kernels of the other.
struct FdSlot : SlotSync {
    DeviceBuf d_frames, d_pad;
    OneShot out;                // [batch][cap] detections, then [batch] counts (written by the post-processing kernel)
    int batch = 0, cap = 0;
    ~FdSlot() { wait(); }
};

// One of the two slots of the streamed JPEG form (mi_fd_submit_jpeg / mi_fd_collect_jpeg; utils.rs:8-21 + face_detection.rs:205 for a stream of
// encoded pictures): the entropy decoder writes the coefficients into the slot's pinned block, their copy runs on the slot's own stream, the
// sample arithmetic / image_to_tensor / network / post-processing on the handle's stream, the results land in the slot's pinned mapped block.
// The pipeline's streamed form (mi_pipeline_submit_jpeg) uses the same slot for its decoder and adds its own result blocks (PipeJpegSlot).
struct JpegSlot : SlotSync {
    OneShot coef{false};           // plain pinned: coefficients, then the quantisation tables
    DeviceBuf d_coef, d_planes, d_rgb;   // d_coef: the image of `coef`
    OneShot one;                   // padding in; detections + count out (the detector's form)
    mi::JpegFrame f;               // the picture in flight (its coefficients live in `coef`)
    int cap = 0;
    // band: submitted on the single-launch plan; suspect: a raised flag may be this picture's (collect repeats it on the batched plan);
    // claimed: holds a share of the handle's StreamClaim
    bool band = false, suspect = false, claimed = false;
    ~JpegSlot() { wait(); }
};

// A single-launch flag has been consumed by someone who cannot tell whose launch raised it (the flag is the handle's): every streamed
// picture in flight on that plan may have void results.
inline void mark_suspect(JpegSlot& a, JpegSlot& b) {
    if (a.pending && a.band) a.suspect = true;
    if (b.pending && b.band) b.suspect = true;
}

// The streamed collect entries (mi_fd_collect_jpeg / mi_pipeline_collect_jpeg), between the wait for the slot's `done` and the hand-out,
// under the caller's Use.  A single launch that gave up leaves void results, and the flags are the handles': with the other slot's picture
// in flight behind this one a raised flag may be that launch's.  So both are marked, and each is repeated on the batched plan when it is
// collected (`rerun`: from the RGB picture, which is still in HBM; enqueues and synchronises).  Whatever happens, the slot is free
// afterwards and its share of the claim is given back.
template <class Failed, class Rerun>
void jpeg_collect(StreamClaim& claim, JpegSlot& sl, JpegSlot& other, Failed failed, Rerun rerun) {
    auto release = [&] {
        if (sl.claimed) claim.release();
        sl.claimed = false;
        sl.pending = false;
    };
    try {
        if (sl.band) {
            if (failed()) mark_suspect(sl, other);
            if (sl.suspect) rerun();
        }
    } catch (...) {
        release();
        throw;
    }
    release();
}

// The collect entries of the host-fed batch forms (mi_fd_collect / mi_fl_collect): wait for the slot's `done` without holding the handle,
// then `hand_out()` copies the slot's pinned results to the caller under the handle's mutex, and the slot is free again.
template <class HandOut>
void slot_collect(mi_model& model, SlotSync& sl, HandOut hand_out) {
    {
        std::lock_guard<std::mutex> g(model.mu);
        if (!sl.pending) throw ApiError(MI_EINVAL, "nothing was submitted to this slot");
    }
    mi::hip_check(hipSetDevice(model.m->device()), "hipSetDevice");
    mi::hip_check(hipEventSynchronize(sl.done), "hipEventSynchronize");
    std::lock_guard<std::mutex> g(model.mu);
    hand_out();
    sl.pending = false;
}

// One of the two slots of the mesh's host-fed batch form (mi_fl_submit_images / mi_fl_collect), like FdSlot: its own copy stream, device
// frames and ROIs, and a pinned + mapped host block that the projection kernel writes the results into.
struct FlSlot : SlotSync {
    DeviceBuf d_frames, d_rois;
    OneShot out;                // [N][468][3] landmarks, [N] present, [N] raw flags
    int N = 0;
    ~FlSlot() { wait(); }
};

MI_CAPI_END
namespace capi = mi::capi;

struct mi_fd {
    mi_model model;
    int kind = 0, in_w = 0, in_h = 0, n_anchors = 0;
    std::vector<float> anchors;
    float* d_anchors = nullptr;
    float* d_lut = nullptr;  // u8 -> f32 in (-1, 1), 256 entries (frames of the network's own size feed the first convolution as bytes)
    capi::DeviceBuf d_in, d_pad, d_out, d_counts, d_img, d_geom, d_roi;
    capi::OneShot one;
    capi::FdSlot slot[2];
    capi::JpegSlot jslot[2];
    capi::StreamClaim jclaim;   // the CUs of the single-launch plan, held while a streamed picture is in flight
    ~mi_fd() {
        for (capi::JpegSlot& sl : jslot) sl.wait();
        //  a batch that was submitted and never collected still reads the anchors and the table: wait for it before
        // anything is freed (hipFree happens to synchronise the device; this does not rely on it)
        for (capi::FdSlot& sl : slot) sl.wait();
        if (d_anchors) (void)hipFree(d_anchors);
        if (d_lut) (void)hipFree(d_lut);
    }
};

struct mi_fl {
    mi_model model;
    int in_w = 0, in_h = 0;
    capi::DeviceBuf d_in, d_roi, d_size, d_lm, d_present, d_flag, d_img, d_geom;
    capi::SizesCache sizes;   // mi_fl_infer_images / mi_fl_submit_images
    capi::OneShot one;
    capi::FlSlot slot[2];
    ~mi_fl() {
        for (capi::FlSlot& sl : slot) sl.wait();   // its kernels still read the handle's buffers
    }
};

struct mi_iris {
    mi_model model;
    int in_w = 0, in_h = 0;
    capi::DeviceBuf d_in, d_roi, d_size, d_pad, d_flip, d_contour, d_iris, d_img, d_geom;
    capi::SizesCache sizes;   // mi_iris_infer_images
    capi::OneShot one;
};

MI_CAPI_BEGIN

// ---- what one unit defines and another uses as well
// capi_fd.cpp.  fd_post: raw device outputs -> detections; FdPostPipeline: what the batched pipelines ask of that launch on top of the
// detections (device results only)
struct FdPostPipeline {
    mi::RectD* face_rois = nullptr;   // [batch] or null: faces[0]'s ROI (face_detection_to_roi on a picture of image_w x image_h) from the same launch
    int* face_valid = nullptr;        // [batch], with face_rois
    int image_w = 0, image_h = 0;
};
void fd_post(mi_fd* h, const float* d_boxes, const float* d_scores, int batch, const double* padding, mi_detection* out, int cap, int* counts,
             int mem, hipStream_t s, const FdPostPipeline* pipe = nullptr);
void jpeg_launch(const mi::JpegFrame& f, const int16_t* d_coef, const uint16_t* d_qt, uint8_t* d_planes, uint8_t* d_rgb, hipStream_t s);
void jpeg_stage(JpegSlot& sl, const uint8_t* bytes, size_t nbytes);
void jpeg_to_rgb(JpegSlot& sl, hipStream_t s);
// capi_landmarks.cpp.  project_mesh: the mesh's two outputs into `a`, then project_landmarks + the face flag in one launch; iris_project:
// both outputs of the iris network (71 contour + 5 iris landmarks per eye) in one launch, out_fs floats between the items of either list
// (0 = packed), gate: [batch] or null
void project_mesh(mi::Model& m, mi::ProjArgs& a, hipStream_t s);
void iris_project(mi_iris* h, int batch, const mi::RectD* d_roi, const int* d_size, const double* d_pad, const int* d_flip, float* d_contour,
                  float* d_iris, hipStream_t s, const int* d_gate = nullptr, long out_fs = 0);
// capi_pipeline.cpp
void require_face_items(int batch, int max_faces, int max_items, int items_limit, const char* items_msg);

MI_CAPI_END
