// capi.cpp — extern "C" boundary (include/mi_face.h).  Translates exceptions into status codes + mi_last_error().
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <atomic>
#include <cstring>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mi_face.h"
#include <dlfcn.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <thread>

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

namespace {

thread_local std::string g_error;

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
        g_error = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        g_error = "out of memory";
        return MI_ENOMEM;
    } catch (const std::exception& e) {
        g_error = e.what();
        std::string m = e.what();
        if (m.rfind("tflite:", 0) == 0 || m.rfind("plan:", 0) == 0) return MI_EMODEL;
        if (m.find("hip") != std::string::npos || m.find("HIP") != std::string::npos || m.find("device") != std::string::npos ||
            m.find("kernel") != std::string::npos)
            return MI_EDEVICE;
        return MI_EINVAL;
    } catch (...) {
        g_error = "unknown error";
        return MI_EINVAL;
    }
}

std::vector<uint8_t> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw ApiError(MI_EIO, "cannot open model file '" + path + "'");
    std::vector<uint8_t> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (data.empty()) throw ApiError(MI_EIO, "model file '" + path + "' is empty");
    return data;
}

// small device scratch that grows on demand
struct DeviceBuf {
    void* p = nullptr;
    size_t cap = 0;
    void* get(size_t bytes) {
        if (bytes > cap) {
            if (p) hipFree(p);
            p = nullptr;
            mi::hip_check(hipMalloc(&p, bytes), "hipMalloc scratch");
            cap = bytes;
        }
        return p;
    }
    ~DeviceBuf() {
        if (p) hipFree(p);
    }
};

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
        if (host) hipHostFree(host);
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
        if (host) hipHostFree(host);
    }
};
// A single-launch run (bandnet_kernels.hip) needs every one of its workgroups resident, one per CU, until it has finished: the handles of
// a process share the device's CUs through this count.  A call that does not get its CUs runs on the batched plan instead — it never waits.
std::atomic<int> g_band_cus[64];
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

void require(bool ok, const char* msg) {
    if (!ok) throw ApiError(MI_EINVAL, msg);
}

// a negative count is the post-processing kernel's report of a letterbox it cannot undo
void check_letterbox(const int* counts, int n) {
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
        if (pending && done) hipEventSynchronize(done);
    }
    ~SlotSync() {
        wait();
        if (copy) hipStreamDestroy(copy);
        if (copied) hipEventDestroy(copied);
        if (done) hipEventDestroy(done);
    }
};

}  // namespace

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
        if (done) hipEventDestroy(done);
    }
};

namespace {
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
}  // namespace

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

namespace {
// A single-launch flag has been consumed by someone who cannot tell whose launch raised it (the flag is the handle's): every streamed
// picture in flight on that plan may have void results.
void mark_suspect(JpegSlot& a, JpegSlot& b) {
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
}  // namespace

struct mi_fd {
    mi_model model;
    int kind = 0, in_w = 0, in_h = 0, n_anchors = 0;
    std::vector<float> anchors;
    float* d_anchors = nullptr;
    float* d_lut = nullptr;  // u8 -> f32 in (-1, 1), 256 entries (frames of the network's own size feed the first convolution as bytes)
    DeviceBuf d_in, d_pad, d_out, d_counts, d_img, d_geom, d_roi;
    OneShot one;
    FdSlot slot[2];
    JpegSlot jslot[2];
    StreamClaim jclaim;   // the CUs of the single-launch plan, held while a streamed picture is in flight
    ~mi_fd() {
        for (JpegSlot& sl : jslot) sl.wait();
        //  a batch that was submitted and never collected still reads the anchors and the table: wait for it before
        // anything is freed (hipFree happens to synchronise the device; this does not rely on it)
        for (FdSlot& sl : slot) sl.wait();
        if (d_anchors) hipFree(d_anchors);
        if (d_lut) hipFree(d_lut);
    }
};

// One of the two slots of the mesh's host-fed batch form (mi_fl_submit_images / mi_fl_collect), like FdSlot: its own copy stream, device
// frames and ROIs, and a pinned + mapped host block that the projection kernel writes the results into.
struct FlSlot : SlotSync {
    DeviceBuf d_frames, d_rois;
    OneShot out;                // [N][468][3] landmarks, [N] present, [N] raw flags
    int N = 0;
    ~FlSlot() { wait(); }
};

struct mi_fl {
    mi_model model;
    int in_w = 0, in_h = 0;
    DeviceBuf d_in, d_roi, d_size, d_lm, d_present, d_flag, d_img, d_geom, d_sizes_b;
    int sizes_N = 0, sizes_w = 0, sizes_h = 0;  // what d_sizes_b holds (mi_fl_infer_images: uploaded when the batch geometry changes)
    OneShot one;
    FlSlot slot[2];
    ~mi_fl() {
        for (FlSlot& sl : slot) sl.wait();   // its kernels still read the handle's buffers
    }
};

struct mi_pipeline {
    std::unique_ptr<mi_fd> fd;
    std::unique_ptr<mi_fl> fl;
    std::unique_ptr<mi_iris> iris;
    DeviceBuf frames, geom, pad_det, pad_eye, in_det, dets, roi_face, valid_face, in_lm, roi_eye, valid_eye, flip_eye, in_eye, sizes;
    // results of a call from host memory: ONE device block (faces | counts | landmarks | present | eyes) and its pinned host image — one
    // asynchronous copy and one synchronisation per call (five copies into the caller's pageable arrays were five synchronous round trips:
    // 115 us of the 0.66 ms of a one-picture call)
    DeviceBuf results;
    OneShot out;
    DeviceBuf geom_det;                              // the detector's letterbox geometry of `geom_B` pictures of geom_w x geom_h (no ROI: uploaded once)
    int geom_B = 0, geom_w = 0, geom_h = 0;
    int sizes_B = 0, sizes_w = 0, sizes_h = 0;  // what `sizes` holds (uploaded once per batch geometry, not per call)
    // mi_pipeline_run_faces: ROI and valid flag of every item slot, and the image sizes of its max_items items (as `sizes`, kept apart so that
    // alternating calls of the two entries upload nothing)
    DeviceBuf roi_item, valid_item, sizes_item;
    int sizes_item_N = 0, sizes_item_w = 0, sizes_item_h = 0;
    // the streamed form from encoded pictures (mi_pipeline_submit_jpeg / mi_pipeline_collect_jpeg): per slot the decoder's state and picture, the
    // results' device block and its pinned image
    struct PipeJpegSlot {
        DeviceBuf results;
        OneShot out;
        JpegSlot jpeg;   // (last: destroyed first, and its destructor waits for the picture in flight)
    };
    PipeJpegSlot jslot[2];
    StreamClaim jclaim;
    ~mi_pipeline() {
        for (PipeJpegSlot& sl : jslot) sl.jpeg.wait();
    }
};
using PipeJpegSlot = mi_pipeline::PipeJpegSlot;

struct mi_iris {
    mi_model model;
    int in_w = 0, in_h = 0;
    DeviceBuf d_in, d_roi, d_size, d_pad, d_flip, d_contour, d_iris, d_img, d_geom, d_sizes_b;
    int sizes_N = 0, sizes_w = 0, sizes_h = 0;
    OneShot one;
};

// FaceEmbeddings (face_embeddings.rs:22-26): the caller's network and the scratch of its two entries.
struct mi_fe {
    mi_model model;
    int features = 0;   // D
    DeviceBuf d_in, d_geom, d_valid, d_img, d_frames, d_faces, d_item_frame, d_item_face, d_emb, d_raw;
};

// A gallery of enrolled embeddings (mi_gallery_topk): the rows and labels in device memory, uploaded once, and the scratch of a call —
// the partial lists of phase 1 and, for host-memory callers, the staged operands — which has to outlive an asynchronous call.
// `sync` is the other handles' contract (mutex, event of the last call); it carries no network.
struct mi_gallery {
    mi_model sync;
    int device = 0, m = 0, features = 0;
    int splits = 0;   // option "splits": 0 = automatic
    DeviceBuf d_rows, d_labels, d_part, d_queries, d_index, d_score, d_label;
    bool has_labels = false;
};

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
        auto h = std::make_unique<mi_model>();
        h->m = std::make_unique<mi::Model>(tflite, nbytes, device);
        *out = h.release();
    });
}

int mi_model_load_file(const char* path, int device, mi_model** out) {
    return guarded([&] {
        require(path && out, "null argument");
        auto bytes = read_file(path);
        auto h = std::make_unique<mi_model>();
        h->m = std::make_unique<mi::Model>(bytes.data(), bytes.size(), device);
        *out = h.release();
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
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        mi::hip_check(hipSetDevice(m->m->device()), "hipSetDevice");
        Use use(*m, stream ? static_cast<hipStream_t>(stream) : m->m->stream());
        m->m->run(in, batch, outs, mem, static_cast<hipStream_t>(stream));
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
    if (buf && cap) {
        size_t k = std::min(cap - 1, s.size());
        std::memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return s.size() + 1;
}

size_t mi_plan_describe(const uint8_t* tflite, size_t nbytes, int fuse_level, char* buf, size_t cap) {
    size_t need = 0;
    int rc = guarded([&] {
        require(tflite && nbytes, "null argument");
        std::string s = mi::build_plan(mi::parse_tflite(tflite, nbytes), fuse_level).describe();
        if (buf && cap) {
            size_t k = std::min(cap - 1, s.size());
            std::memcpy(buf, s.data(), k);
            buf[k] = 0;
        }
        need = s.size() + 1;
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
        if (buf && cap) {
            size_t k = std::min(cap - 1, s.size());
            std::memcpy(buf, s.data(), k);
            buf[k] = 0;
        }
        need = s.size() + 1;
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
        auto h = std::make_unique<mi_fd>();
        h->model.m = std::make_unique<mi::Model>(tflite, nbytes, device);
        fd_finish_create(h.get(), kind);
        *out = h.release();
    });
}

int mi_fd_create(int kind, const char* model_dir, int device, mi_fd** out) {
    return guarded([&] {
        require(out, "null argument");
        const char* file = mi::model_file_for(kind);
        if (!file) throw ApiError(MI_EINVAL, "unsupported model type");
        std::string dir = model_dir ? model_dir : "./models";  // face_detection.rs:157-161
        auto bytes = read_file(dir + "/" + file);
        auto h = std::make_unique<mi_fd>();
        h->model.m = std::make_unique<mi::Model>(bytes.data(), bytes.size(), device);
        fd_finish_create(h.get(), kind);
        *out = h.release();
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

// shared tail: raw device outputs -> detections
// what the batched pipelines ask of the post-processing launch on top of the detections (device results only)
struct FdPostPipeline {
    mi::RectD* face_rois = nullptr;   // [batch] or null: faces[0]'s ROI (face_detection_to_roi on a picture of image_w x image_h) from the same launch
    int* face_valid = nullptr;        // [batch], with face_rois
    int image_w = 0, image_h = 0;
};
static void fd_post(mi_fd* h, const float* d_boxes, const float* d_scores, int batch, const double* padding, mi_detection* out,
                    int cap, int* counts, int mem, hipStream_t s, const FdPostPipeline* pipe = nullptr) {
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
    if (mem == MI_MEM_DEVICE) {
        a.padding = padding;
        a.out = reinterpret_cast<float*>(out);
        a.counts = counts;
        int rc = mi::launch_postprocess(a, s);
        if (rc) throw std::runtime_error(std::string("postprocess kernel launch failed: ") + hipGetErrorString(static_cast<hipError_t>(rc)));
        return;
    }
    const double* d_pad = nullptr;
    if (padding) {
        d_pad = static_cast<const double*>(h->d_pad.get(sizeof(double) * 4 * batch));
        mi::hip_check(hipMemcpyAsync(const_cast<double*>(d_pad), padding, sizeof(double) * 4 * batch, hipMemcpyHostToDevice, s), "H2D padding");
    }
    a.padding = d_pad;
    a.out = static_cast<float*>(h->d_out.get(sizeof(mi_detection) * static_cast<size_t>(cap) * batch));
    a.counts = static_cast<int*>(h->d_counts.get(sizeof(int) * batch));
    // the kernel stores min(count, cap) detections per frame: the rest of the caller's host buffer reads as zeros, not as
    // whatever the staging buffer held before
    mi::hip_check(hipMemsetAsync(a.out, 0, sizeof(mi_detection) * static_cast<size_t>(cap) * batch, s), "hipMemsetAsync");
    int rc = mi::launch_postprocess(a, s);
    if (rc) throw std::runtime_error(std::string("postprocess kernel launch failed: ") + hipGetErrorString(static_cast<hipError_t>(rc)));
    mi::hip_check(hipMemcpyAsync(out, a.out, sizeof(mi_detection) * static_cast<size_t>(cap) * batch, hipMemcpyDeviceToHost, s), "D2H detections");
    mi::hip_check(hipMemcpyAsync(counts, a.counts, sizeof(int) * batch, hipMemcpyDeviceToHost, s), "D2H counts");
    mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    check_letterbox(counts, batch);
}

int mi_fd_infer_tensor(mi_fd* h, const float* in, int batch, const double* padding, mi_detection* out, int cap_per_frame,
                       int* counts, int mem, void* stream) {
    return guarded([&] {
        require(h && in && out && counts, "null argument");
        require(batch > 0 && cap_per_frame > 0, "batch and cap_per_frame must be positive");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : m.stream();
        Use use(h->model, s);
        const float* din = in;
        if (mem == MI_MEM_HOST) {
            size_t bytes = m.input_elems() * sizeof(float) * batch;
            din = static_cast<const float*>(h->d_in.get(bytes));
            mi::hip_check(hipMemcpyAsync(const_cast<float*>(din), in, bytes, hipMemcpyHostToDevice, s), "H2D input");
        }
        m.run_device(din, batch, s);
        fd_post(h, m.output_device(0), m.output_device(1), batch, padding, out, cap_per_frame, counts, mem, s);
        if (mem == MI_MEM_DEVICE && !stream) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    });
}

int mi_fd_postprocess(mi_fd* h, const float* raw_boxes, const float* raw_scores, int batch, const double* padding,
                      mi_detection* out, int cap_per_frame, int* counts, int mem, void* stream) {
    return guarded([&] {
        require(h && raw_boxes && raw_scores && out && counts, "null argument");
        require(batch > 0 && cap_per_frame > 0, "batch and cap_per_frame must be positive");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : m.stream();
        Use use(h->model, s);
        const float *db = raw_boxes, *ds = raw_scores;
        if (mem == MI_MEM_HOST) {
            size_t nb = sizeof(float) * 16 * h->n_anchors * batch, ns = sizeof(float) * h->n_anchors * batch;
            char* p = static_cast<char*>(h->d_in.get(nb + ns));
            mi::hip_check(hipMemcpyAsync(p, raw_boxes, nb, hipMemcpyHostToDevice, s), "H2D boxes");
            mi::hip_check(hipMemcpyAsync(p + nb, raw_scores, ns, hipMemcpyHostToDevice, s), "H2D scores");
            db = reinterpret_cast<const float*>(p);
            ds = reinterpret_cast<const float*>(p + nb);
        }
        fd_post(h, db, ds, batch, padding, out, cap_per_frame, counts, mem, s);
        if (mem == MI_MEM_DEVICE && !stream) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    });
}

int mi_fd_infer_image(mi_fd* h, const uint8_t* rgb, int width, int height, int stride, const mi_rect* roi, mi_detection* out,
                      int cap, int* count) {
    return guarded([&] {
        require(h && rgb && out && count, "null argument");
        require(width > 0 && height > 0 && stride >= 3 * width && cap > 0, "bad image geometry");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = m.stream();
        Use use(h->model, s);
        float* d_t = static_cast<float*>(h->d_in.get(m.input_elems() * sizeof(float)));
        const size_t nout = sizeof(mi_detection) * static_cast<size_t>(cap);
        OneShot& o = h->one;
        o.reserve(kOneResults + nout);
        // image_to_tensor(image, roi, (w,h), keep_aspect_ratio = true, (-1,1), flip = false) — face_detection.rs:219
        mi::image_to_tensor_enqueue(rgb, width, height, stride, roi, h->in_w, h->in_h, true, -1.0, 1.0, false, d_t, o.h<double>(kOnePad),
                                    static_cast<uint8_t*>(h->d_img.get(static_cast<size_t>(stride) * height)), s);
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

// dequantise + IDCT, then up-sampling + colour conversion: coefficients -> RGB picture, all in device memory
static void jpeg_launch(const mi::JpegFrame& f, const int16_t* d_coef, const uint16_t* d_qt, uint8_t* d_planes, uint8_t* d_rgb, hipStream_t s) {
    int rc = mi::launch_jpeg_idct(f, d_coef, d_qt, d_planes, s);
    if (rc == 0) rc = mi::launch_jpeg_color(f, d_planes, d_rgb, s);
    if (rc) throw std::runtime_error(std::string("jpeg kernel launch failed: ") + hipGetErrorString(static_cast<hipError_t>(rc)));
}

// submit, first half.  (1) the serial part, on this thread, while the device works on the other slot's picture: the coefficients go straight
// into the slot's pinned block, the quantisation tables behind them; (2) their copy is queued on the slot's own stream, `copied` behind it.
static void jpeg_stage(JpegSlot& sl, const uint8_t* bytes, size_t nbytes) {
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
static void jpeg_to_rgb(JpegSlot& sl, hipStream_t s) {
    mi::hip_check(hipStreamWaitEvent(s, sl.copied, 0), "hipStreamWaitEvent");
    char* d_coef = static_cast<char*>(sl.d_coef.p);
    jpeg_launch(sl.f, reinterpret_cast<const int16_t*>(d_coef), reinterpret_cast<const uint16_t*>(d_coef + sl.f.coef.size() * sizeof(int16_t)),
                static_cast<uint8_t*>(sl.d_planes.p), static_cast<uint8_t*>(sl.d_rgb.p), s);
}

static void fd_jpeg_network(mi_fd* h, JpegSlot& sl, bool one_shot, hipStream_t s) {
    mi::Model& m = *h->model.m;
    OneShot& o = sl.one;
    float* d_t = static_cast<float*>(h->d_in.get(m.input_elems() * sizeof(float)));
    mi::image_to_tensor_enqueue_device(static_cast<const uint8_t*>(sl.d_rgb.p), sl.f.width, sl.f.height, 3 * sl.f.width, nullptr, h->in_w, h->in_h, true, -1.0, 1.0, false,
                                       d_t, o.h<double>(kOnePad), s);
    std::memset(o.h<char>(kOneResults), 0, sizeof(mi_detection) * static_cast<size_t>(sl.cap));
    m.run_device(d_t, 1, s, one_shot);
    fd_post(h, m.output_device(0), m.output_device(1), 1, o.d<double>(kOnePad), o.d<mi_detection>(kOneResults), sl.cap, o.d<int>(kOneCount), MI_MEM_DEVICE, s);
}

int mi_fd_submit_jpeg(mi_fd* h, int slot, const uint8_t* bytes, size_t nbytes, int cap) {
    return guarded([&] {
        require(h && bytes, "null argument");
        require(slot == 0 || slot == 1, "slot must be 0 or 1");
        require(cap > 0, "cap must be positive");
        JpegSlot& sl = h->jslot[slot];
        if (sl.pending) throw ApiError(MI_EINVAL, "slot holds a picture that has not been collected");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        jpeg_stage(sl, bytes, nbytes);
        sl.one.reserve(kOneResults + sizeof(mi_detection) * static_cast<size_t>(cap));
        sl.cap = cap;
        hipStream_t s = m.stream();
        Use use(h->model, s);
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
        require(slot == 0 || slot == 1, "slot must be 0 or 1");
        JpegSlot& sl = h->jslot[slot];
        if (!sl.pending) throw ApiError(MI_EINVAL, "nothing was submitted to this slot");
        require(cap >= sl.cap, "cap is smaller than the one the picture was submitted with");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        mi::hip_check(hipEventSynchronize(sl.done), "hipEventSynchronize");
        {
            hipStream_t s = m.stream();
            Use use(h->model, s);
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
    mi::PreItems it{};
    it.frames = d_frames; it.frame_bytes = static_cast<long>(stride) * height; it.width = width; it.height = height; it.stride = stride;
    it.rois = d_rois; it.items_per_frame = 1; it.N = batch; it.out_w = h->in_w; it.out_h = h->in_h; it.keep_aspect = 1;
    it.range_min = -1.0; it.range_max = 1.0;
    auto* d_geom = static_cast<mi::PreGeom*>(h->d_geom.get(sizeof(mi::PreGeom) * batch));
    float* d_in = static_cast<float*>(h->d_in.get(m.input_elems() * sizeof(float) * batch));
    mi::launch_pre_geom(it, d_geom, d_pad, s);
    mi::launch_pre_tensor(it, d_geom, d_in, s);
    m.run_device(d_in, batch, s);
    fd_post(h, m.output_device(0), m.output_device(1), batch, d_pad, d_out, cap, d_counts, MI_MEM_DEVICE, s);
}

static size_t frames_bytes(int batch, int width, int height, int stride) {
    // the last frame's last row owns 3 * width bytes, not a whole stride
    return static_cast<size_t>(stride) * height * (batch - 1) + static_cast<size_t>(stride) * (height - 1) + static_cast<size_t>(3) * width;
}

int mi_fd_infer_images(mi_fd* h, const uint8_t* frames, int batch, int width, int height, int stride, const mi_rect* rois, mi_detection* out,
                       int cap_per_frame, int* counts, int mem, void* stream) {
    return guarded([&] {
        require(h && frames && out && counts, "null argument");
        require(batch > 0 && cap_per_frame > 0 && width > 0 && height > 0 && stride >= 3 * width, "bad frame geometry");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : m.stream();
        Use use(h->model, s);
        const uint8_t* d_frames = frames;
        const mi::RectD* d_rois = nullptr;
        static_assert(sizeof(mi::RectD) == sizeof(mi_rect), "mi_rect and RectD must have one layout");
        if (mem == MI_MEM_HOST) {
            d_frames = static_cast<const uint8_t*>(h->d_img.get(static_cast<size_t>(stride) * height * batch));
            mi::hip_check(hipMemcpyAsync(const_cast<uint8_t*>(d_frames), frames, frames_bytes(batch, width, height, stride), hipMemcpyHostToDevice, s), "H2D frames");
            if (rois) {
                d_rois = static_cast<const mi::RectD*>(h->d_roi.get(sizeof(mi_rect) * batch));
                mi::hip_check(hipMemcpyAsync(const_cast<mi::RectD*>(d_rois), rois, sizeof(mi_rect) * batch, hipMemcpyHostToDevice, s), "H2D rois");
            }
        } else {
            d_rois = reinterpret_cast<const mi::RectD*>(rois);
        }
        double* d_pad = static_cast<double*>(h->d_pad.get(sizeof(double) * 4 * batch));
        if (mem == MI_MEM_DEVICE) {
            fd_images_device(h, d_frames, batch, width, height, stride, d_rois, d_pad, out, cap_per_frame, counts, s);
            if (!stream) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
            return;
        }
        const size_t nout = sizeof(mi_detection) * static_cast<size_t>(cap_per_frame) * batch;
        auto* d_out = static_cast<mi_detection*>(h->d_out.get(nout));
        int* d_counts = static_cast<int*>(h->d_counts.get(sizeof(int) * batch));
        mi::hip_check(hipMemsetAsync(d_out, 0, nout, s), "hipMemsetAsync");  // unused slots of the caller's buffer read as zeros
        fd_images_device(h, d_frames, batch, width, height, stride, d_rois, d_pad, d_out, cap_per_frame, d_counts, s);
        mi::hip_check(hipMemcpyAsync(out, d_out, nout, hipMemcpyDeviceToHost, s), "D2H detections");
        mi::hip_check(hipMemcpyAsync(counts, d_counts, sizeof(int) * batch, hipMemcpyDeviceToHost, s), "D2H counts");
        mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        check_letterbox(counts, batch);
    });
}

int mi_fd_submit_images(mi_fd* h, int slot, const uint8_t* frames, int batch, int width, int height, int stride, int cap_per_frame) {
    return guarded([&] {
        require(h && frames, "null argument");
        require(slot == 0 || slot == 1, "slot must be 0 or 1");
        require(batch > 0 && cap_per_frame > 0 && width > 0 && height > 0 && stride >= 3 * width, "bad frame geometry");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = m.stream();
        Use use(h->model, s);
        FdSlot& sl = h->slot[slot];
        if (sl.pending) throw ApiError(MI_EINVAL, "slot still holds an uncollected batch (call mi_fd_collect first)");
        sl.open();
        const size_t nout = sizeof(mi_detection) * static_cast<size_t>(cap_per_frame) * batch, ncnt = sizeof(int) * batch;
        sl.out.reserve(nout + ncnt);
        // frames: host -> device on the slot's copy stream (asynchronous when `frames` is pinned memory: mi_host_alloc);
        // everything else on the handle's stream, behind the copy.  The post-processing kernel writes detections and counts
        // straight into the slot's pinned host block (mapped into the device's address space): a hipMemcpyAsync of the results
        // blocked the host for whole batches on this runtime (measured: every third call, 7 ms).
        auto* d_frames = static_cast<uint8_t*>(sl.d_frames.get(static_cast<size_t>(stride) * height * batch));
        mi::hip_check(hipMemcpyAsync(d_frames, frames, frames_bytes(batch, width, height, stride), hipMemcpyHostToDevice, sl.copy), "H2D frames");
        mi::hip_check(hipEventRecord(sl.copied, sl.copy), "hipEventRecord");
        mi::hip_check(hipStreamWaitEvent(s, sl.copied, 0), "hipStreamWaitEvent");
        std::memset(sl.out.host, 0, nout + ncnt);  // slots beyond a frame's count read as zeros (the slot was collected: nothing in flight writes here)
        double* d_pad = static_cast<double*>(sl.d_pad.get(sizeof(double) * 4 * batch));
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
        require(slot == 0 || slot == 1, "slot must be 0 or 1");
        FdSlot& sl = h->slot[slot];
        {
            std::lock_guard<std::mutex> g(h->model.mu);
            if (!sl.pending) throw ApiError(MI_EINVAL, "nothing was submitted to this slot");
        }
        mi::hip_check(hipSetDevice(h->model.m->device()), "hipSetDevice");
        mi::hip_check(hipEventSynchronize(sl.done), "hipEventSynchronize");
        std::lock_guard<std::mutex> g(h->model.mu);
        const size_t nout = sizeof(mi_detection) * static_cast<size_t>(sl.cap) * sl.batch;
        std::memcpy(out, sl.out.host, nout);
        std::memcpy(counts, sl.out.h<char>(nout), sizeof(int) * sl.batch);
        sl.pending = false;
        check_letterbox(counts, sl.batch);
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
        auto h = std::make_unique<mi_fl>();
        h->model.m = std::make_unique<mi::Model>(tflite, nbytes, device);
        fl_finish_create(h.get());
        *out = h.release();
    });
}

int mi_fl_create(const char* model_path, int device, mi_fl** out) {
    return guarded([&] {
        require(out, "null argument");
        auto bytes = read_file(model_path ? model_path : "./models/face_landmark.tflite");  // face_landmark.rs:211-215
        auto h = std::make_unique<mi_fl>();
        h->model.m = std::make_unique<mi::Model>(bytes.data(), bytes.size(), device);
        fl_finish_create(h.get());
        *out = h.release();
    });
}

void mi_fl_free(mi_fl* h) { delete h; }
mi_model* mi_fl_model(mi_fl* h) { return h ? &h->model : nullptr; }

// the mesh's two outputs into `a`, then project_landmarks + the face flag in one launch
static void project_mesh(mi::Model& m, mi::ProjArgs& a, hipStream_t s) {
    a.raw = m.output_device(0);
    a.raw_fs = static_cast<long>(m.output_elems(0));
    a.flag = m.output_device(1) + (m.output_elems(1) - 1);  // `flatten[flatten.len() - 1]` — face_landmark.rs:292-293
    a.flag_fs = static_cast<long>(m.output_elems(1));
    int rc = mi::launch_project(a, s);
    if (rc) throw std::runtime_error(std::string("projection kernel launch failed: ") + hipGetErrorString(static_cast<hipError_t>(rc)));
}

int mi_fl_infer_tensor(mi_fl* h, const float* in, int batch, const mi_rect* rois, const int* image_sizes, float* landmarks,
                       int* present, float* raw_flags, int mem, void* stream) {
    return guarded([&] {
        require(h && in && landmarks && present, "null argument");
        require(batch > 0, "batch must be positive");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        require(!rois || image_sizes, "image_sizes is required when rois are given");
        static_assert(sizeof(mi_rect) == sizeof(mi::RectD), "mi_rect layout");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : m.stream();
        Use use(h->model, s);
        const size_t lm_bytes = sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * batch;
        mi::ProjArgs a;
        a.B = batch;
        a.n = MI_NUM_FACE_LANDMARKS;
        a.tensor_w = h->in_w;
        a.tensor_h = h->in_h;
        const float* din = in;
        if (mem == MI_MEM_HOST) {
            size_t bytes = m.input_elems() * sizeof(float) * batch;
            din = static_cast<const float*>(h->d_in.get(bytes));
            mi::hip_check(hipMemcpyAsync(const_cast<float*>(din), in, bytes, hipMemcpyHostToDevice, s), "H2D input");
            if (rois) {
                a.roi = static_cast<const mi::RectD*>(h->d_roi.get(sizeof(mi_rect) * batch));
                mi::hip_check(hipMemcpyAsync(const_cast<mi::RectD*>(a.roi), rois, sizeof(mi_rect) * batch, hipMemcpyHostToDevice, s), "H2D rois");
                a.image_size = static_cast<const int*>(h->d_size.get(sizeof(int) * 2 * batch));
                mi::hip_check(hipMemcpyAsync(const_cast<int*>(a.image_size), image_sizes, sizeof(int) * 2 * batch, hipMemcpyHostToDevice, s), "H2D sizes");
            }
            a.out = static_cast<float*>(h->d_lm.get(lm_bytes));
            a.present = static_cast<int*>(h->d_present.get(sizeof(int) * batch));
            a.raw_flag_out = static_cast<float*>(h->d_flag.get(sizeof(float) * batch));
        } else {
            a.roi = reinterpret_cast<const mi::RectD*>(rois);
            a.image_size = image_sizes;
            a.out = landmarks;
            a.present = present;
            a.raw_flag_out = raw_flags;
        }
        m.run_device(din, batch, s);
        project_mesh(m, a, s);
        if (mem == MI_MEM_HOST) {
            mi::hip_check(hipMemcpyAsync(landmarks, a.out, lm_bytes, hipMemcpyDeviceToHost, s), "D2H landmarks");
            mi::hip_check(hipMemcpyAsync(present, a.present, sizeof(int) * batch, hipMemcpyDeviceToHost, s), "D2H present");
            if (raw_flags) mi::hip_check(hipMemcpyAsync(raw_flags, a.raw_flag_out, sizeof(float) * batch, hipMemcpyDeviceToHost, s), "D2H flags");
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        } else if (!stream) {
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        }
    });
}

// (w, h) of the source image for every item of a batch of equally sized frames, on the device; re-uploaded only when the batch geometry changes
static int* batch_image_sizes(DeviceBuf& buf, int& have_N, int& have_w, int& have_h, int N, int width, int height, hipStream_t s) {
    int* d = static_cast<int*>(buf.get(sizeof(int) * 2 * N));
    if (have_N != N || have_w != width || have_h != height) {
        std::vector<int> hs(2 * static_cast<size_t>(N));
        for (int i = 0; i < N; i++) { hs[2 * i] = width; hs[2 * i + 1] = height; }
        have_N = 0;
        mi::hip_check(hipMemcpyAsync(d, hs.data(), hs.size() * sizeof(int), hipMemcpyHostToDevice, s), "H2D sizes");
        mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");  // hs is a host temporary
        have_N = N; have_w = width; have_h = height;
    }
    return d;
}

// FaceLandmark::infer(&Mat, Option<Rect>) for a batch of (frame, ROI) items (face_landmark.rs:232-306): image_to_tensor(frame, roi,
// (192,192), keep_aspect_ratio = false, (0,1)) on the device, network, face flag, project_landmarks.  Item i reads frame
// i / items_per_frame.  Only u8 frames and ROIs cross the bus (the f32 crops of mi_fl_infer_tensor are 442 KB per ROI).
int mi_fl_infer_images(mi_fl* h, const uint8_t* frames, int batch, int width, int height, int stride, const mi_rect* rois, int items_per_frame,
                       float* landmarks, int* present, float* raw_flags, int mem, void* stream) {
    return guarded([&] {
        require(h && frames && landmarks && present, "null argument");
        require(batch > 0 && items_per_frame > 0 && width > 0 && height > 0 && stride >= 3 * width, "bad frame geometry");
        require(rois || items_per_frame == 1, "several items per frame need their ROIs");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        require(static_cast<long long>(batch) * items_per_frame <= (1 << 24), "too many items");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : m.stream();
        Use use(h->model, s);
        const int N = batch * items_per_frame;
        const uint8_t* d_frames = frames;
        const mi::RectD* d_rois = reinterpret_cast<const mi::RectD*>(rois);
        if (mem == MI_MEM_HOST) {
            d_frames = static_cast<const uint8_t*>(h->d_img.get(static_cast<size_t>(stride) * height * batch));
            mi::hip_check(hipMemcpyAsync(const_cast<uint8_t*>(d_frames), frames, frames_bytes(batch, width, height, stride), hipMemcpyHostToDevice, s), "H2D frames");
            if (rois) {
                d_rois = static_cast<const mi::RectD*>(h->d_roi.get(sizeof(mi_rect) * N));
                mi::hip_check(hipMemcpyAsync(const_cast<mi::RectD*>(d_rois), rois, sizeof(mi_rect) * N, hipMemcpyHostToDevice, s), "H2D rois");
            }
        }
        mi::PreItems it{};
        it.frames = d_frames; it.frame_bytes = static_cast<long>(stride) * height; it.width = width; it.height = height; it.stride = stride;
        it.rois = d_rois; it.items_per_frame = items_per_frame; it.N = N; it.out_w = h->in_w; it.out_h = h->in_h; it.keep_aspect = 0;
        it.range_min = 0.0; it.range_max = 1.0;
        auto* d_geom = static_cast<mi::PreGeom*>(h->d_geom.get(sizeof(mi::PreGeom) * N));
        float* d_in = static_cast<float*>(h->d_in.get(m.input_elems() * sizeof(float) * N));
        mi::launch_pre_geom(it, d_geom, nullptr, s);
        mi::launch_pre_tensor(it, d_geom, d_in, s);
        const size_t lm_bytes = sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * N;
        mi::ProjArgs a;
        a.B = N; a.n = MI_NUM_FACE_LANDMARKS; a.tensor_w = h->in_w; a.tensor_h = h->in_h;
        a.roi = d_rois;
        a.image_size = d_rois ? batch_image_sizes(h->d_sizes_b, h->sizes_N, h->sizes_w, h->sizes_h, N, width, height, s) : nullptr;
        if (mem == MI_MEM_HOST) {
            a.out = static_cast<float*>(h->d_lm.get(lm_bytes));
            a.present = static_cast<int*>(h->d_present.get(sizeof(int) * N));
            a.raw_flag_out = static_cast<float*>(h->d_flag.get(sizeof(float) * N));
        } else {
            a.out = landmarks; a.present = present; a.raw_flag_out = raw_flags;
        }
        m.run_device(d_in, N, s);
        project_mesh(m, a, s);
        if (mem == MI_MEM_HOST) {
            mi::hip_check(hipMemcpyAsync(landmarks, a.out, lm_bytes, hipMemcpyDeviceToHost, s), "D2H landmarks");
            mi::hip_check(hipMemcpyAsync(present, a.present, sizeof(int) * N, hipMemcpyDeviceToHost, s), "D2H present");
            if (raw_flags) mi::hip_check(hipMemcpyAsync(raw_flags, a.raw_flag_out, sizeof(float) * N, hipMemcpyDeviceToHost, s), "D2H flags");
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        } else if (!stream) {
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        }
    });
}

// The same for a continuous host feed, split in two like the detector's (mi_fd_submit_images / mi_fd_collect): submit queues the H2D copy
// of the frames on the slot's own stream, then warp + network + projection on the handle's stream behind it, and returns; the projection
// kernel writes into the slot's pinned, mapped host block; collect waits for the slot and hands the results out.
int mi_fl_submit_images(mi_fl* h, int slot, const uint8_t* frames, int batch, int width, int height, int stride, const mi_rect* rois, int items_per_frame) {
    return guarded([&] {
        require(h && frames, "null argument");
        require(slot == 0 || slot == 1, "slot must be 0 or 1");
        require(batch > 0 && items_per_frame > 0 && width > 0 && height > 0 && stride >= 3 * width, "bad frame geometry");
        require(rois || items_per_frame == 1, "several items per frame need their ROIs");
        require(static_cast<long long>(batch) * items_per_frame <= (1 << 24), "too many items");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = m.stream();
        Use use(h->model, s);
        FlSlot& sl = h->slot[slot];
        if (sl.pending) throw ApiError(MI_EINVAL, "slot still holds an uncollected batch (call mi_fl_collect first)");
        sl.open();
        const int N = batch * items_per_frame;
        const size_t lm_bytes = sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * N;
        sl.out.reserve(lm_bytes + (sizeof(int) + sizeof(float)) * N);
        const size_t frame_bytes = static_cast<size_t>(stride) * height;
        auto* d_frames = static_cast<uint8_t*>(sl.d_frames.get(frame_bytes * batch));
        mi::hip_check(hipMemcpyAsync(d_frames, frames, frames_bytes(batch, width, height, stride), hipMemcpyHostToDevice, sl.copy), "H2D frames");
        const mi::RectD* d_rois = nullptr;
        if (rois) {   // (the ROIs are small and usually pageable: the runtime stages them before the call returns)
            d_rois = static_cast<const mi::RectD*>(sl.d_rois.get(sizeof(mi_rect) * N));
            mi::hip_check(hipMemcpyAsync(const_cast<mi::RectD*>(d_rois), rois, sizeof(mi_rect) * N, hipMemcpyHostToDevice, sl.copy), "H2D rois");
        }
        mi::hip_check(hipEventRecord(sl.copied, sl.copy), "hipEventRecord");
        try {
            const int* d_sizes = d_rois ? batch_image_sizes(h->d_sizes_b, h->sizes_N, h->sizes_w, h->sizes_h, N, width, height, s) : nullptr;
            mi::hip_check(hipStreamWaitEvent(s, sl.copied, 0), "hipStreamWaitEvent");
            mi::PreItems it{};
            it.frames = d_frames; it.frame_bytes = static_cast<long>(frame_bytes); it.width = width; it.height = height; it.stride = stride;
            it.rois = d_rois; it.items_per_frame = items_per_frame; it.N = N; it.out_w = h->in_w; it.out_h = h->in_h; it.keep_aspect = 0;
            it.range_min = 0.0; it.range_max = 1.0;
            auto* d_geom = static_cast<mi::PreGeom*>(h->d_geom.get(sizeof(mi::PreGeom) * N));
            float* d_in = static_cast<float*>(h->d_in.get(m.input_elems() * sizeof(float) * N));
            mi::launch_pre_geom(it, d_geom, nullptr, s);
            mi::launch_pre_tensor(it, d_geom, d_in, s);
            mi::ProjArgs a;
            a.B = N; a.n = MI_NUM_FACE_LANDMARKS; a.tensor_w = h->in_w; a.tensor_h = h->in_h;
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
        require(slot == 0 || slot == 1, "slot must be 0 or 1");
        FlSlot& sl = h->slot[slot];
        {
            std::lock_guard<std::mutex> g(h->model.mu);
            if (!sl.pending) throw ApiError(MI_EINVAL, "nothing was submitted to this slot");
        }
        mi::hip_check(hipSetDevice(h->model.m->device()), "hipSetDevice");
        mi::hip_check(hipEventSynchronize(sl.done), "hipEventSynchronize");
        std::lock_guard<std::mutex> g(h->model.mu);
        const size_t lm_bytes = sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * sl.N;
        std::memcpy(landmarks, sl.out.host, lm_bytes);
        std::memcpy(present, sl.out.h<char>(lm_bytes), sizeof(int) * sl.N);
        if (raw_flags) std::memcpy(raw_flags, sl.out.h<char>(lm_bytes + sizeof(int) * sl.N), sizeof(float) * sl.N);
        sl.pending = false;
    });
}

int mi_fl_infer_image(mi_fl* h, const uint8_t* rgb, int width, int height, int stride, const mi_rect* roi, mi_landmark* out,
                      int cap, int* count) {
    return guarded([&] {
        require(h && rgb && out && count, "null argument");
        require(width > 0 && height > 0 && stride >= 3 * width, "bad image geometry");
        require(cap >= MI_NUM_FACE_LANDMARKS, "output capacity must be at least 468");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = m.stream();
        Use use(h->model, s);
        float* d_t = static_cast<float*>(h->d_in.get(m.input_elems() * sizeof(float)));
        double pad[4];
        OneShot& o = h->one;
        const size_t lm_bytes = sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS;
        o.reserve(kOneResults + lm_bytes);
        // image_to_tensor(image, roi, (192,192), keep_aspect_ratio = false, (0,1), false) — face_landmark.rs:250
        mi::image_to_tensor_enqueue(rgb, width, height, stride, roi, h->in_w, h->in_h, false, 0.0, 1.0, false, d_t, pad,
                                    static_cast<uint8_t*>(h->d_img.get(static_cast<size_t>(stride) * height)), s);
        mi::ProjArgs a;
        a.B = 1; a.n = MI_NUM_FACE_LANDMARKS; a.tensor_w = h->in_w; a.tensor_h = h->in_h;
        if (roi) {
            std::memcpy(o.h<char>(kOneRoi), roi, sizeof(mi_rect));
            o.h<int>(kOneSize)[0] = width;
            o.h<int>(kOneSize)[1] = height;
            a.roi = o.d<mi::RectD>(kOneRoi);
            a.image_size = o.d<int>(kOneSize);
        }
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
        auto h = std::make_unique<mi_iris>();
        h->model.m = std::make_unique<mi::Model>(tflite, nbytes, device);
        iris_finish_create(h.get());
        *out = h.release();
    });
}

int mi_iris_create(const char* model_path, int device, mi_iris** out) {
    return guarded([&] {
        require(out, "null argument");
        auto bytes = read_file(model_path ? model_path : "./models/iris_landmark.tflite");  // iris_landmark.rs:145-149
        auto h = std::make_unique<mi_iris>();
        h->model.m = std::make_unique<mi::Model>(bytes.data(), bytes.size(), device);
        iris_finish_create(h.get());
        *out = h.release();
    });
}

void mi_iris_free(mi_iris* h) { delete h; }
mi_model* mi_iris_model(mi_iris* h) { return h ? &h->model : nullptr; }

static void iris_project(mi_iris* h, int batch, const mi::RectD* d_roi, const int* d_size, const double* d_pad, const int* d_flip,
                         float* d_contour, float* d_iris, hipStream_t s) {
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
    a.raw = m.output_device(0);
    a.raw_fs = static_cast<long>(m.output_elems(0));
    a.out = d_contour;
    a.raw2 = m.output_device(1);
    a.raw2_fs = static_cast<long>(m.output_elems(1));
    a.out2 = d_iris;
    int rc = mi::launch_project(a, s);
    if (rc) throw std::runtime_error(std::string("projection kernel launch failed: ") + hipGetErrorString(static_cast<hipError_t>(rc)));
}

int mi_iris_infer_tensor(mi_iris* h, const float* in, int batch, const mi_rect* rois, const int* image_sizes, const double* padding,
                         const int* is_right_eye, float* contour, float* iris, int mem, void* stream) {
    return guarded([&] {
        require(h && in && contour && iris, "null argument");
        require(batch > 0, "batch must be positive");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        require(!rois || image_sizes, "image_sizes is required when rois are given");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : m.stream();
        Use use(h->model, s);
        const size_t cb = sizeof(float) * 3 * MI_NUM_EYE_LANDMARKS * batch, ib = sizeof(float) * 3 * MI_NUM_IRIS_LANDMARKS * batch;
        if (mem == MI_MEM_DEVICE) {
            m.run_device(in, batch, s);
            iris_project(h, batch, reinterpret_cast<const mi::RectD*>(rois), image_sizes, padding, is_right_eye, contour, iris, s);
            if (!stream) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
            return;
        }
        size_t bytes = m.input_elems() * sizeof(float) * batch;
        float* din = static_cast<float*>(h->d_in.get(bytes));
        mi::hip_check(hipMemcpyAsync(din, in, bytes, hipMemcpyHostToDevice, s), "H2D input");
        const mi::RectD* d_roi = nullptr;
        const int *d_size = nullptr, *d_flip = nullptr;
        const double* d_pad = nullptr;
        if (rois) {
            d_roi = static_cast<const mi::RectD*>(h->d_roi.get(sizeof(mi_rect) * batch));
            mi::hip_check(hipMemcpyAsync(const_cast<mi::RectD*>(d_roi), rois, sizeof(mi_rect) * batch, hipMemcpyHostToDevice, s), "H2D rois");
            d_size = static_cast<const int*>(h->d_size.get(sizeof(int) * 2 * batch));
            mi::hip_check(hipMemcpyAsync(const_cast<int*>(d_size), image_sizes, sizeof(int) * 2 * batch, hipMemcpyHostToDevice, s), "H2D sizes");
        }
        if (padding) {
            d_pad = static_cast<const double*>(h->d_pad.get(sizeof(double) * 4 * batch));
            mi::hip_check(hipMemcpyAsync(const_cast<double*>(d_pad), padding, sizeof(double) * 4 * batch, hipMemcpyHostToDevice, s), "H2D padding");
        }
        if (is_right_eye) {
            d_flip = static_cast<const int*>(h->d_flip.get(sizeof(int) * batch));
            mi::hip_check(hipMemcpyAsync(const_cast<int*>(d_flip), is_right_eye, sizeof(int) * batch, hipMemcpyHostToDevice, s), "H2D flip");
        }
        float* dc = static_cast<float*>(h->d_contour.get(cb));
        float* di = static_cast<float*>(h->d_iris.get(ib));
        m.run_device(din, batch, s);
        iris_project(h, batch, d_roi, d_size, d_pad, d_flip, dc, di, s);
        mi::hip_check(hipMemcpyAsync(contour, dc, cb, hipMemcpyDeviceToHost, s), "D2H contour");
        mi::hip_check(hipMemcpyAsync(iris, di, ib, hipMemcpyDeviceToHost, s), "D2H iris");
        mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    });
}

// IrisLandmark::infer(&Mat, Option<Rect>, Option<bool>) for a batch of (frame, eye ROI) items (iris_landmark.rs:158-248):
// image_to_tensor(frame, roi, (64,64), keep_aspect_ratio = true, (0,1), flip = is_right_eye) on the device, network, both
// project_landmarks calls.  Item i reads frame i / items_per_frame (2 = the two eyes of a face).
int mi_iris_infer_images(mi_iris* h, const uint8_t* frames, int batch, int width, int height, int stride, const mi_rect* rois, const int* is_right_eye,
                         int items_per_frame, float* contour, float* iris, int mem, void* stream) {
    return guarded([&] {
        require(h && frames && contour && iris, "null argument");
        require(batch > 0 && items_per_frame > 0 && width > 0 && height > 0 && stride >= 3 * width, "bad frame geometry");
        require(rois || items_per_frame == 1, "several items per frame need their ROIs");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        require(static_cast<long long>(batch) * items_per_frame <= (1 << 24), "too many items");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : m.stream();
        Use use(h->model, s);
        const int N = batch * items_per_frame;
        const uint8_t* d_frames = frames;
        const mi::RectD* d_rois = reinterpret_cast<const mi::RectD*>(rois);
        const int* d_flip = is_right_eye;
        if (mem == MI_MEM_HOST) {
            d_frames = static_cast<const uint8_t*>(h->d_img.get(static_cast<size_t>(stride) * height * batch));
            mi::hip_check(hipMemcpyAsync(const_cast<uint8_t*>(d_frames), frames, frames_bytes(batch, width, height, stride), hipMemcpyHostToDevice, s), "H2D frames");
            if (rois) {
                d_rois = static_cast<const mi::RectD*>(h->d_roi.get(sizeof(mi_rect) * N));
                mi::hip_check(hipMemcpyAsync(const_cast<mi::RectD*>(d_rois), rois, sizeof(mi_rect) * N, hipMemcpyHostToDevice, s), "H2D rois");
            }
            if (is_right_eye) {
                d_flip = static_cast<const int*>(h->d_flip.get(sizeof(int) * N));
                mi::hip_check(hipMemcpyAsync(const_cast<int*>(d_flip), is_right_eye, sizeof(int) * N, hipMemcpyHostToDevice, s), "H2D flip");
            }
        }
        mi::PreItems it{};
        it.frames = d_frames; it.frame_bytes = static_cast<long>(stride) * height; it.width = width; it.height = height; it.stride = stride;
        it.rois = d_rois; it.flip = d_flip; it.items_per_frame = items_per_frame; it.N = N; it.out_w = h->in_w; it.out_h = h->in_h; it.keep_aspect = 1;
        it.range_min = 0.0; it.range_max = 1.0;
        auto* d_geom = static_cast<mi::PreGeom*>(h->d_geom.get(sizeof(mi::PreGeom) * N));
        double* d_pad = static_cast<double*>(h->d_pad.get(sizeof(double) * 4 * N));
        float* d_in = static_cast<float*>(h->d_in.get(m.input_elems() * sizeof(float) * N));
        mi::launch_pre_geom(it, d_geom, d_pad, s);
        mi::launch_pre_tensor(it, d_geom, d_in, s);
        const int* d_size = d_rois ? batch_image_sizes(h->d_sizes_b, h->sizes_N, h->sizes_w, h->sizes_h, N, width, height, s) : nullptr;
        const size_t cb = sizeof(float) * 3 * MI_NUM_EYE_LANDMARKS * N, ib = sizeof(float) * 3 * MI_NUM_IRIS_LANDMARKS * N;
        float* dc = mem == MI_MEM_DEVICE ? contour : static_cast<float*>(h->d_contour.get(cb));
        float* di = mem == MI_MEM_DEVICE ? iris : static_cast<float*>(h->d_iris.get(ib));
        m.run_device(d_in, N, s);
        iris_project(h, N, d_rois, d_size, d_pad, d_flip, dc, di, s);
        if (mem == MI_MEM_HOST) {
            mi::hip_check(hipMemcpyAsync(contour, dc, cb, hipMemcpyDeviceToHost, s), "D2H contour");
            mi::hip_check(hipMemcpyAsync(iris, di, ib, hipMemcpyDeviceToHost, s), "D2H iris");
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        } else if (!stream) {
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        }
    });
}

int mi_iris_infer_image(mi_iris* h, const uint8_t* rgb, int width, int height, int stride, const mi_rect* roi, int is_right_eye,
                        mi_landmark* contour71, mi_landmark* iris5) {
    return guarded([&] {
        require(h && rgb && contour71 && iris5, "null argument");
        require(width > 0 && height > 0 && stride >= 3 * width, "bad image geometry");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = m.stream();
        Use use(h->model, s);
        float* d_t = static_cast<float*>(h->d_in.get(m.input_elems() * sizeof(float)));
        OneShot& o = h->one;
        constexpr size_t kContour = kOneResults, kIris = kOneResults + sizeof(float) * 3 * MI_NUM_EYE_LANDMARKS;
        o.reserve(kIris + sizeof(float) * 3 * MI_NUM_IRIS_LANDMARKS);
        // image_to_tensor(image, roi, (64,64), keep_aspect_ratio = true, (0,1), is_right_eye) — iris_landmark.rs:188-189
        mi::image_to_tensor_enqueue(rgb, width, height, stride, roi, h->in_w, h->in_h, true, 0.0, 1.0, is_right_eye != 0, d_t,
                                    o.h<double>(kOnePad), static_cast<uint8_t*>(h->d_img.get(static_cast<size_t>(stride) * height)), s);
        const mi::RectD* d_roi = nullptr;
        const int* d_size = nullptr;
        if (roi) {
            std::memcpy(o.h<char>(kOneRoi), roi, sizeof(mi_rect));
            o.h<int>(kOneSize)[0] = width;
            o.h<int>(kOneSize)[1] = height;
            d_roi = o.d<mi::RectD>(kOneRoi);
            d_size = o.d<int>(kOneSize);
        }
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

// ------------------------------------------------------------------------------------------------ batched pipeline
int mi_pipeline_create(int fd_kind, const char* model_dir, int device, mi_pipeline** out) {
    return guarded([&] {
        require(out, "null argument");
        std::string dir = model_dir ? model_dir : "./models";
        auto p = std::make_unique<mi_pipeline>();
        mi_fd* fd = nullptr;
        mi_fl* fl = nullptr;
        mi_iris* ir = nullptr;
        if (int rc = mi_fd_create(fd_kind, dir.c_str(), device, &fd)) throw ApiError(rc, g_error);
        p->fd.reset(fd);
        if (int rc = mi_fl_create((dir + "/face_landmark.tflite").c_str(), device, &fl)) throw ApiError(rc, g_error);
        p->fl.reset(fl);
        if (int rc = mi_iris_create((dir + "/iris_landmark.tflite").c_str(), device, &ir)) throw ApiError(rc, g_error);
        p->iris.reset(ir);
        *out = p.release();
    });
}

int mi_pipeline_create_from_bytes(int fd_kind, const uint8_t* fd_tflite, size_t fd_nbytes, const uint8_t* fl_tflite, size_t fl_nbytes,
                                  const uint8_t* iris_tflite, size_t iris_nbytes, int device, mi_pipeline** out) {
    return guarded([&] {
        require(out && fd_tflite && fl_tflite && iris_tflite && fd_nbytes && fl_nbytes && iris_nbytes, "null argument");
        auto p = std::make_unique<mi_pipeline>();
        mi_fd* fd = nullptr;
        mi_fl* fl = nullptr;
        mi_iris* ir = nullptr;
        if (int rc = mi_fd_create_from_bytes(fd_kind, fd_tflite, fd_nbytes, device, &fd)) throw ApiError(rc, g_error);
        p->fd.reset(fd);
        if (int rc = mi_fl_create_from_bytes(fl_tflite, fl_nbytes, device, &fl)) throw ApiError(rc, g_error);
        p->fl.reset(fl);
        if (int rc = mi_iris_create_from_bytes(iris_tflite, iris_nbytes, device, &ir)) throw ApiError(rc, g_error);
        p->iris.reset(ir);
        *out = p.release();
    });
}

void mi_pipeline_free(mi_pipeline* p) { delete p; }
mi_model* mi_pipeline_model(mi_pipeline* p, int which) {
    if (!p) return nullptr;
    return which == 0 ? &p->fd->model : which == 1 ? &p->fl->model : which == 2 ? &p->iris->model : nullptr;
}

int mi_pipeline_set_option(mi_pipeline* p, const char* key, int value) {
    return guarded([&] {
        require(p && key, "null argument");
        std::lock_guard<std::mutex> l0(p->fd->model.mu), l1(p->fl->model.mu), l2(p->iris->model.mu);
        p->fd->model.m->set_option(key, value);
        p->fl->model.m->set_option(key, value);
        p->iris->model.m->set_option(key, value);
    });
}

namespace {
struct PipeOut {   // DEVICE pointers the stages of one pipeline pass write their results to
    mi_detection* faces;   // [B] top-1 detection
    int* counts;           // [B]
    float* lm;             // [B][468][3]
    int* present;          // [B]
    float* eyes;           // [B][2][76][3]
};
constexpr int kPipeCap = 4;
constexpr long kEyeFs = 3L * (MI_NUM_EYE_LANDMARKS + MI_NUM_IRIS_LANDMARKS);
struct PipeLayout {        // one block: faces | counts | landmarks | present | eyes
    size_t faces, counts, lm, present, eyes, bytes;
    explicit PipeLayout(int B) {
        auto up16 = [](size_t v) { return (v + 15) & ~static_cast<size_t>(15); };
        faces = 0;
        counts = up16(faces + sizeof(mi_detection) * B);
        lm = up16(counts + sizeof(int) * B);
        present = up16(lm + sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * B);
        eyes = up16(present + sizeof(int) * B);
        bytes = up16(eyes + sizeof(float) * kEyeFs * 2 * B);
    }
    PipeOut in(char* base) const {
        return PipeOut{reinterpret_cast<mi_detection*>(base + faces), reinterpret_cast<int*>(base + counts), reinterpret_cast<float*>(base + lm),
                       reinterpret_cast<int*>(base + present), reinterpret_cast<float*>(base + eyes)};
    }
};
}  // namespace

// (w, h) of the source image of every ROI of a pass over N mesh items (2 N eyes), for Rect::scaled in project_landmarks: a host round trip only
// when the batch geometry changes.  `have_*` say what `buf` holds.
static int* pipeline_sizes(DeviceBuf& buf, int& have_N, int& have_w, int& have_h, int N, int width, int height, hipStream_t s) {
    int* d_sizes = static_cast<int*>(buf.get(sizeof(int) * 4 * N));
    if (have_N != N || have_w != width || have_h != height) {
        std::vector<int> hs(4 * static_cast<size_t>(N));
        for (int i = 0; i < 2 * N; i++) { hs[2 * i] = width; hs[2 * i + 1] = height; }
        have_N = 0;
        mi::hip_check(hipMemcpyAsync(d_sizes, hs.data(), hs.size() * sizeof(int), hipMemcpyHostToDevice, s), "H2D sizes");
        mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");  // hs is a host temporary
        have_N = N; have_w = width; have_h = height;
    }
    return d_sizes;
}

struct PipeTrace {   // MI_PIPE_TRACE=1: host-side step times of a pass, to stderr
    const bool on;
    std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    PipeTrace() : on(enabled()) {}
    static bool enabled() { static const bool e = getenv("MI_PIPE_TRACE") != nullptr; return e; }
    void operator()(const char* what) const {
        if (on) std::fprintf(stderr, "  %-22s %8.1f us\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count());
    }
};

// The detector's stage of a pass over B frames in device memory: image_to_tensor(frame, None, (w,h), keep_aspect = true, (-1,1)) -> net.  Sets up
// `it` (the frames; the later stages change the item fields) and returns the letterbox paddings [B][4] the post-processing launch needs.
static double* pipeline_detect(mi_pipeline* p, mi::PreItems& it, const uint8_t* d_frames, int B, int width, int height, int stride, bool one_shot, hipStream_t s,
                               const PipeTrace& tr) {
    mi::Model& fdm = *p->fd->model.m;
    const size_t frame_bytes = static_cast<size_t>(stride) * height;
    it.frames = d_frames; it.frame_bytes = static_cast<long>(frame_bytes); it.width = width; it.height = height; it.stride = stride;
    it.items_per_frame = 1; it.N = B; it.out_w = p->fd->in_w; it.out_h = p->fd->in_h; it.keep_aspect = 1;
    it.range_min = -1.0; it.range_max = 1.0;
    double* d_pad_det = static_cast<double*>(p->pad_det.get(sizeof(double) * 4 * B));
    float* d_in_det = static_cast<float*>(p->in_det.get(fdm.input_elems() * sizeof(float) * B));
    // (no ROI: the geometry is the same for every call on pictures of this size — no pre_geom launch, 9 us of a one-picture call)
    auto* d_geom_det = static_cast<mi::PreGeom*>(p->geom_det.get(sizeof(mi::PreGeom) * B));
    if (p->geom_B != B || p->geom_w != width || p->geom_h != height) {
        p->geom_B = 0;
        mi::upload_whole_image_geom(width, height, it.out_w, it.out_h, true, B, d_geom_det, d_pad_det, s);
        p->geom_B = B; p->geom_w = width; p->geom_h = height;
    }
    mi::launch_pre_tensor(it, d_geom_det, d_in_det, s);
    tr("pre det");
    fdm.run_device(d_in_det, B, s, one_shot);
    tr("det run_device");
    return d_pad_det;
}

// The mesh and iris stages of a pass for N items whose face ROIs (and valid flags) are in device memory: item i reads frame i of `it`, or frame
// it.item_frame[i] when that is set.  d_sizes: pipeline_sizes() of N items.
static void pipeline_mesh_iris(mi_pipeline* p, mi::PreItems& it, int N, const mi::RectD* d_roi_face, const int* d_valid_face, const int* d_sizes, float* lm,
                               int* present, float* eyes, bool one_shot, hipStream_t s, const PipeTrace& tr) {
    mi::Model& flm = *p->fl->model.m;
    mi::Model& irm = *p->iris->model.m;
    const int width = it.width, height = it.height;
    const long eye_fs = kEyeFs;
    auto* d_geom = static_cast<mi::PreGeom*>(p->geom.get(sizeof(mi::PreGeom) * 2 * N));
    // ---- 2. face -> face_detection_to_roi -> image_to_tensor(frame, roi, (192,192), false, (0,1)) -> mesh net
    it.rois = d_roi_face; it.roi_valid = d_valid_face; it.items_per_frame = 1; it.N = N; it.out_w = p->fl->in_w; it.out_h = p->fl->in_h; it.keep_aspect = 0;
    it.range_min = 0.0; it.range_max = 1.0;
    float* d_in_lm = static_cast<float*>(p->in_lm.get(flm.input_elems() * sizeof(float) * N));
    mi::launch_pre_geom(it, d_geom, nullptr, s);
    mi::launch_pre_tensor(it, d_geom, d_in_lm, s);
    tr("pre mesh");
    flm.run_device(d_in_lm, N, s, one_shot);
    tr("mesh run_device");
    {
        mi::ProjArgs a;
        a.B = N; a.n = MI_NUM_FACE_LANDMARKS; a.tensor_w = p->fl->in_w; a.tensor_h = p->fl->in_h;
        a.roi = d_roi_face; a.image_size = d_sizes; a.gate = d_valid_face;
        a.out = lm; a.present = present;
        project_mesh(flm, a, s);
    }
    // ---- 3. iris_roi_from_face_landmarks -> image_to_tensor(frame, eye roi, (64,64), true, (0,1), flip = right eye) -> iris net
    auto* d_roi_eye = static_cast<mi::RectD*>(p->roi_eye.get(sizeof(mi::RectD) * 2 * N));
    int* d_valid_eye = static_cast<int*>(p->valid_eye.get(sizeof(int) * 2 * N));
    int* d_flip_eye = static_cast<int*>(p->flip_eye.get(sizeof(int) * 2 * N));
    mi::launch_iris_rois(lm, present, N, width, height, d_roi_eye, d_valid_eye, d_flip_eye, s);
    it.rois = d_roi_eye; it.roi_valid = d_valid_eye; it.flip = d_flip_eye; it.items_per_frame = 2; it.N = 2 * N;
    it.out_w = p->iris->in_w; it.out_h = p->iris->in_h; it.keep_aspect = 1;
    double* d_pad_eye = static_cast<double*>(p->pad_eye.get(sizeof(double) * 8 * N));
    float* d_in_eye = static_cast<float*>(p->in_eye.get(irm.input_elems() * sizeof(float) * 2 * N));
    mi::launch_pre_geom(it, d_geom, d_pad_eye, s);
    mi::launch_pre_tensor(it, d_geom, d_in_eye, s);
    tr("pre iris");
    irm.run_device(d_in_eye, 2 * N, s, one_shot);
    tr("iris run_device");
    {   // contour and iris landmarks of both eyes in one launch
        mi::ProjArgs a;
        a.B = 2 * N; a.n = MI_NUM_EYE_LANDMARKS; a.n2 = MI_NUM_IRIS_LANDMARKS; a.tensor_w = p->iris->in_w; a.tensor_h = p->iris->in_h;
        a.roi = d_roi_eye; a.image_size = d_sizes; a.padding = d_pad_eye; a.flip = d_flip_eye; a.gate = d_valid_eye;
        a.raw = irm.output_device(0); a.raw_fs = static_cast<long>(irm.output_elems(0));
        a.raw2 = irm.output_device(1); a.raw2_fs = static_cast<long>(irm.output_elems(1));
        a.out = eyes; a.out_fs = eye_fs;
        a.out2 = eyes + 3 * MI_NUM_EYE_LANDMARKS; a.out2_fs = eye_fs;
        int rc = mi::launch_project(a, s);
        if (rc) throw std::runtime_error(std::string("projection kernel launch failed: ") + hipGetErrorString(static_cast<hipError_t>(rc)));
    }
    tr("projections");
}

// One pass of the flow of lib.rs:24-40 over B frames that are in device memory: everything is queued on `s`, nothing is waited for (but the
// upload of the per-item image sizes when the batch geometry changes).  The caller holds the three handles (Use) and, for one_shot, the CUs.
static void pipeline_enqueue(mi_pipeline* p, const uint8_t* d_frames, int B, int width, int height, int stride, const PipeOut& o, bool one_shot, hipStream_t s) {
    mi::Model& fdm = *p->fd->model.m;
    const int cap = kPipeCap;
    const int* d_sizes = pipeline_sizes(p->sizes, p->sizes_B, p->sizes_w, p->sizes_h, B, width, height, s);
    const PipeTrace tr;
    // ---- 1. detector -> decode + NMS
    mi::PreItems it{};
    double* d_pad_det = pipeline_detect(p, it, d_frames, B, width, height, stride, one_shot, s, tr);
    float* d_dets = static_cast<float*>(p->dets.get(sizeof(mi_detection) * cap * B));
    // ---- 2. faces[0] -> face_detection_to_roi -> mesh, 3. both eyes -> iris
    // (the post-processing launch writes zeros behind a frame's last detection — frames without a face report zeros — and faces[0]'s ROI)
    auto* d_roi_face = static_cast<mi::RectD*>(p->roi_face.get(sizeof(mi::RectD) * B));
    int* d_valid_face = static_cast<int*>(p->valid_face.get(sizeof(int) * B));
    const FdPostPipeline top1{d_roi_face, d_valid_face, width, height};
    fd_post(p->fd.get(), fdm.output_device(0), fdm.output_device(1), B, d_pad_det, reinterpret_cast<mi_detection*>(d_dets), cap, o.counts,
            MI_MEM_DEVICE, s, &top1);
    tr("fd_post");
    pipeline_mesh_iris(p, it, B, d_roi_face, d_valid_face, d_sizes, o.lm, o.present, o.eyes, one_shot, s, tr);
    // ---- top-1 faces out (strided gather [B][cap][17] -> [B][17])
    mi::hip_check(hipMemcpy2DAsync(o.faces, sizeof(mi_detection), d_dets, sizeof(mi_detection) * cap, sizeof(mi_detection), B,
                                   hipMemcpyDeviceToDevice, s), "gather faces");
    tr("gather");
}

// Did a single-launch run of the pass give up?  band_failed() also CLEARS its model's flag, so all three are asked whatever the first
// answers: `||` would leave a raised flag behind for the next call to trip over.
static bool pipeline_band_failed(mi_pipeline* p) {
    return (static_cast<int>(p->fd->model.m->band_failed()) | static_cast<int>(p->fl->model.m->band_failed()) |
            static_cast<int>(p->iris->model.m->band_failed())) != 0;
}

// the CUs a single-launch pass over B pictures needs: its launches follow one another on one stream and share a claim of the largest
static int pipeline_band_workgroups(mi_pipeline* p, int B) {
    return std::max(std::max(p->fd->model.m->band_workgroups(B), p->fl->model.m->band_workgroups(B)), p->iris->model.m->band_workgroups(2 * B));
}

// the results of one pass, from the pinned image of its block into the caller's arrays
static void pipeline_hand_out(const OneShot& out, const PipeLayout& L, int B, mi_detection* faces, int* face_counts, float* landmarks, int* present, float* eyes) {
    std::memcpy(faces, out.h<char>(L.faces), sizeof(mi_detection) * B);
    std::memcpy(face_counts, out.h<char>(L.counts), sizeof(int) * B);
    std::memcpy(landmarks, out.h<char>(L.lm), sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * B);
    std::memcpy(present, out.h<char>(L.present), sizeof(int) * B);
    std::memcpy(eyes, out.h<char>(L.eyes), sizeof(float) * kEyeFs * 2 * B);
    for (int b = 0; b < B; b++) {
        check_letterbox(face_counts + b, 1);
        if (face_counts[b] == 0) std::memset(&faces[b], 0, sizeof(mi_detection));
    }
}

int mi_pipeline_run(mi_pipeline* p, const uint8_t* frames, int batch, int width, int height, int stride, mi_detection* faces,
                    int* face_counts, float* landmarks, int* present, float* eyes, int mem, void* stream) {
    return guarded([&] {
        require(p && frames && faces && face_counts && landmarks && present && eyes, "null argument");
        require(batch > 0 && width > 0 && height > 0 && stride >= 3 * width, "bad frame geometry");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        mi::Model& fdm = *p->fd->model.m;
        mi::hip_check(hipSetDevice(fdm.device()), "hipSetDevice");
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : fdm.stream();
        Use use_fd(p->fd->model, s), use_fl(p->fl->model, s), use_ir(p->iris->model, s);  // the pipeline's own three handles, fixed order
        const int B = batch;
        const PipeLayout L(B);
        char* d_results = nullptr;
        if (mem == MI_MEM_HOST) {
            d_results = static_cast<char*>(p->results.get(L.bytes));
            p->out.reserve(L.bytes);
        }
        const size_t frame_bytes = static_cast<size_t>(stride) * height;
        const uint8_t* d_frames = frames;
        if (mem == MI_MEM_HOST) {
            d_frames = static_cast<const uint8_t*>(p->frames.get(frame_bytes * B));
            mi::hip_check(hipMemcpyAsync(const_cast<uint8_t*>(d_frames), frames, frames_bytes(B, width, height, stride), hipMemcpyHostToDevice, s), "H2D frames");
        }
        // A picture or two from host memory (lib.rs:24-40 on one image): the detector and the face mesh may take their single-launch plans —
        // this call holds the CUs until its synchronisation below, and repeats itself on the batched plan should such a launch have given up.
        std::unique_ptr<BandClaim> claim;
        if (mem == MI_MEM_HOST) claim = std::make_unique<BandClaim>(fdm.device(), pipeline_band_workgroups(p, B));
        const PipeOut o = mem == MI_MEM_DEVICE ? PipeOut{faces, face_counts, landmarks, present, eyes} : L.in(d_results);
        auto network = [&](bool one_shot) {
            pipeline_enqueue(p, d_frames, B, width, height, stride, o, one_shot, s);
            if (mem == MI_MEM_HOST) mi::hip_check(hipMemcpyAsync(p->out.host, d_results, L.bytes, hipMemcpyDeviceToHost, s), "D2H results");
            if (mem == MI_MEM_HOST || !stream) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        };
        with_band_retry(claim && claim->ok, [&] { return pipeline_band_failed(p); }, network);
        if (mem == MI_MEM_HOST) pipeline_hand_out(p->out, L, B, faces, face_counts, landmarks, present, eyes);
    });
}

// ---- every face of a frame (mi_pipeline_run_faces): the detector's first max_faces detections per frame, compacted on the device into a list of
// max_items (frame, face) items (face_items.hpp), mesh and iris on exactly max_items / 2 * max_items items.  Batched plan only.
namespace {
struct FacesOut {   // DEVICE pointers of one pass
    mi_detection* faces;   // [B][max_faces]
    int* counts;           // [B]
    int* item_frame;       // [M]
    int* item_face;        // [M]
    int* n_items;          // [2]
    float* lm;             // [M][468][3]
    int* present;          // [M]
    float* eyes;           // [M][2][76][3]
};
struct FacesLayout {       // one block (host memory calls): faces | counts | item_frame | item_face | n_items | landmarks | present | eyes
    size_t faces, counts, item_frame, item_face, n_items, lm, present, eyes, bytes;
    FacesLayout(int B, int max_faces, int M) {
        auto up16 = [](size_t v) { return (v + 15) & ~static_cast<size_t>(15); };
        faces = 0;
        counts = up16(faces + sizeof(mi_detection) * B * max_faces);
        item_frame = up16(counts + sizeof(int) * B);
        item_face = up16(item_frame + sizeof(int) * M);
        n_items = up16(item_face + sizeof(int) * M);
        lm = up16(n_items + sizeof(int) * 2);
        present = up16(lm + sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * M);
        eyes = up16(present + sizeof(int) * M);
        bytes = up16(eyes + sizeof(float) * kEyeFs * 2 * M);
    }
    FacesOut in(char* base) const {
        return FacesOut{reinterpret_cast<mi_detection*>(base + faces), reinterpret_cast<int*>(base + counts), reinterpret_cast<int*>(base + item_frame),
                        reinterpret_cast<int*>(base + item_face), reinterpret_cast<int*>(base + n_items), reinterpret_cast<float*>(base + lm),
                        reinterpret_cast<int*>(base + present), reinterpret_cast<float*>(base + eyes)};
    }
};
void require_face_items(int batch, int max_faces, int max_items, int items_limit, const char* items_msg) {
    require(batch > 0 && batch <= mi::kFaceItemsMaxBatch, "batch must be 1..2^26");
    require(max_faces >= 1 && max_faces <= mi::kFaceItemsMaxFaces, "max_faces must be 1..16");
    require(max_items >= 1 && max_items <= items_limit, items_msg);
}
}  // namespace

int mi_face_items_layout(const int* face_counts, int batch, int max_faces, int max_items, int* item_frame, int* item_face, int* n_items) {
    return guarded([&] {
        require(face_counts && item_frame && item_face && n_items, "null argument");
        require_face_items(batch, max_faces, max_items, mi::kFaceItemsMaxItems, "max_items must be 1..2^20");
        int total = 0;
        for (int b = 0; b < batch; b++) {
            const int n = mi::face_items_of_frame(face_counts[b], max_faces);
            for (int k = 0; k < n; k++) {
                const int j = mi::face_items_slot(total, k, max_items);
                if (j < 0) break;
                item_frame[j] = b;
                item_face[j] = k;
            }
            total += n;
        }
        mi::face_items_totals(total, max_items, n_items);
        for (int j = n_items[0]; j < max_items; j++) item_frame[j] = item_face[j] = -1;
    });
}

int mi_pipeline_run_faces(mi_pipeline* p, const uint8_t* frames, int batch, int width, int height, int stride, int max_faces, int max_items,
                          mi_detection* faces, int* face_counts, int* item_frame, int* item_face, int* n_items, float* landmarks, int* present,
                          float* eyes, int mem, void* stream) {
    return guarded([&] {
        // (a budget the launches cannot take is refused here, before anything is queued)
        require_face_items(batch, max_faces, max_items, mi::kFaceItemsMaxRunItems, "max_items must be 1..32767 (2 * max_items eyes, one per grid row of a launch)");
        require(p && frames && faces && face_counts && item_frame && item_face && n_items && landmarks && present && eyes, "null argument");
        require(width > 0 && height > 0 && stride >= 3 * width, "bad frame geometry");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        mi::Model& fdm = *p->fd->model.m;
        mi::hip_check(hipSetDevice(fdm.device()), "hipSetDevice");
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : fdm.stream();
        Use use_fd(p->fd->model, s), use_fl(p->fl->model, s), use_ir(p->iris->model, s);  // the pipeline's own three handles, fixed order
        const int B = batch, M = max_items;
        const FacesLayout L(B, max_faces, M);
        const uint8_t* d_frames = frames;
        FacesOut o{faces, face_counts, item_frame, item_face, n_items, landmarks, present, eyes};
        if (mem == MI_MEM_HOST) {
            o = L.in(static_cast<char*>(p->results.get(L.bytes)));
            p->out.reserve(L.bytes);
            d_frames = static_cast<const uint8_t*>(p->frames.get(static_cast<size_t>(stride) * height * B));
            mi::hip_check(hipMemcpyAsync(const_cast<uint8_t*>(d_frames), frames, frames_bytes(B, width, height, stride), hipMemcpyHostToDevice, s), "H2D frames");
        }
        const int* d_sizes = pipeline_sizes(p->sizes_item, p->sizes_item_N, p->sizes_item_w, p->sizes_item_h, M, width, height, s);
        const PipeTrace tr;
        // ---- 1. detector -> decode + NMS, max_faces records per frame straight into `faces` (zeros behind a frame's last detection)
        mi::PreItems it{};
        double* d_pad_det = pipeline_detect(p, it, d_frames, B, width, height, stride, false, s, tr);
        const FdPostPipeline no_top1{};   // (the item kernel computes every face's ROI)
        fd_post(p->fd.get(), fdm.output_device(0), fdm.output_device(1), B, d_pad_det, o.faces, max_faces, o.counts, MI_MEM_DEVICE, s, &no_top1);
        tr("fd_post");
        // ---- the item list: frame, face and face_detection_to_roi of every slot
        mi::FaceItemsArgs fa{};
        fa.dets = reinterpret_cast<const float*>(o.faces); fa.counts = o.counts;
        fa.B = B; fa.max_faces = max_faces; fa.max_items = M; fa.image_w = width; fa.image_h = height;
        fa.item_frame = o.item_frame; fa.item_face = o.item_face; fa.n_items = o.n_items;
        fa.rois = static_cast<mi::RectD*>(p->roi_item.get(sizeof(mi::RectD) * M));
        fa.valid = static_cast<int*>(p->valid_item.get(sizeof(int) * M));
        mi::launch_face_items(fa, s);
        tr("face items");
        // ---- 2. every item's face -> mesh, 3. both eyes -> iris: item i reads frame item_frame[i]
        it.item_frame = o.item_frame;
        pipeline_mesh_iris(p, it, M, fa.rois, fa.valid, d_sizes, o.lm, o.present, o.eyes, false, s, tr);
        if (mem == MI_MEM_HOST) mi::hip_check(hipMemcpyAsync(p->out.host, p->results.p, L.bytes, hipMemcpyDeviceToHost, s), "D2H results");
        if (mem == MI_MEM_HOST || !stream) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (mem == MI_MEM_HOST) {
            const OneShot& h = p->out;
            std::memcpy(faces, h.h<char>(L.faces), sizeof(mi_detection) * B * max_faces);
            std::memcpy(face_counts, h.h<char>(L.counts), sizeof(int) * B);
            std::memcpy(item_frame, h.h<char>(L.item_frame), sizeof(int) * M);
            std::memcpy(item_face, h.h<char>(L.item_face), sizeof(int) * M);
            std::memcpy(n_items, h.h<char>(L.n_items), sizeof(int) * 2);
            std::memcpy(landmarks, h.h<char>(L.lm), sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * M);
            std::memcpy(present, h.h<char>(L.present), sizeof(int) * M);
            std::memcpy(eyes, h.h<char>(L.eyes), sizeof(float) * kEyeFs * 2 * M);
            check_letterbox(face_counts, B);
        }
    });
}

// ---- the flow of lib.rs:18-40 for a STREAM of encoded pictures: convert_image_to_mat + FaceDetection::infer + FaceLandmark::infer + 2 x
// IrisLandmark::infer per picture, two slots (see mi_fd_submit_jpeg): the entropy decoder of picture n + 1 runs on the calling thread while the
// device works through picture n's four networks.
static void pipeline_jpeg_network(mi_pipeline* p, PipeJpegSlot& sl, bool one_shot, hipStream_t s) {
    const PipeLayout L(1);
    char* d_results = static_cast<char*>(sl.results.get(L.bytes));
    const JpegSlot& js = sl.jpeg;
    pipeline_enqueue(p, static_cast<const uint8_t*>(js.d_rgb.p), 1, js.f.width, js.f.height, 3 * js.f.width, L.in(d_results), one_shot, s);
    mi::hip_check(hipMemcpyAsync(sl.out.host, d_results, L.bytes, hipMemcpyDeviceToHost, s), "D2H results");
}

int mi_pipeline_submit_jpeg(mi_pipeline* p, int slot, const uint8_t* bytes, size_t nbytes) {
    return guarded([&] {
        require(p && bytes, "null argument");
        require(slot == 0 || slot == 1, "slot must be 0 or 1");
        PipeJpegSlot& sl = p->jslot[slot];
        JpegSlot& js = sl.jpeg;
        if (js.pending) throw ApiError(MI_EINVAL, "slot holds a picture that has not been collected");
        mi::Model& fdm = *p->fd->model.m;
        mi::hip_check(hipSetDevice(fdm.device()), "hipSetDevice");
        jpeg_stage(js, bytes, nbytes);
        sl.out.reserve(PipeLayout(1).bytes);
        hipStream_t s = fdm.stream();
        Use use_fd(p->fd->model, s), use_fl(p->fl->model, s), use_ir(p->iris->model, s);
        jpeg_to_rgb(js, s);
        js.band = p->jclaim.acquire(fdm.device(), pipeline_band_workgroups(p, 1));
        js.claimed = true;
        js.suspect = false;
        pipeline_jpeg_network(p, sl, js.band, s);
        mi::hip_check(hipEventRecord(js.done, s), "hipEventRecord");
        js.pending = true;
    });
}

int mi_pipeline_collect_jpeg(mi_pipeline* p, int slot, mi_detection* face, int* face_count, float* landmarks, int* present, float* eyes, int* width, int* height) {
    return guarded([&] {
        require(p && face && face_count && landmarks && present && eyes, "null argument");
        require(slot == 0 || slot == 1, "slot must be 0 or 1");
        PipeJpegSlot& sl = p->jslot[slot];
        JpegSlot& js = sl.jpeg;
        if (!js.pending) throw ApiError(MI_EINVAL, "nothing was submitted to this slot");
        mi::Model& fdm = *p->fd->model.m;
        mi::hip_check(hipSetDevice(fdm.device()), "hipSetDevice");
        mi::hip_check(hipEventSynchronize(js.done), "hipEventSynchronize");
        {
            hipStream_t s = fdm.stream();
            Use use_fd(p->fd->model, s), use_fl(p->fl->model, s), use_ir(p->iris->model, s);
            jpeg_collect(p->jclaim, js, p->jslot[1 - slot].jpeg, [&] { return pipeline_band_failed(p); }, [&] {
                pipeline_jpeg_network(p, sl, false, s);
                mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
            });
        }
        pipeline_hand_out(sl.out, PipeLayout(1), 1, face, face_count, landmarks, present, eyes);
        if (width) *width = js.f.width;
        if (height) *height = js.f.height;
    });
}

// ------------------------------------------------------------------------------------------------ multi-GPU: weight broadcast
// The one exchange of the sharded path: the frozen .tflite bytes travel once from `root` to every rank over RCCL, then
// each rank builds its handles with mi_*_create_from_bytes.  A Rust host (north_star) has no torch.distributed: this entry speaks to
// librccl directly (loaded at call time, so the library itself does not depend on it).  Rendezvous = the ncclUniqueId in a file every
// rank of the node can read: `root` writes it (temporary name + rename), the others wait for it.
namespace {
struct UniqueId { char internal[128]; };   // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128), passed by value like the original
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(UniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
}  // namespace

// ------------------------------------------------------------------------------------------------ streams on distinct hardware queues
// HIP streams share the device's hardware queues (GPU_MAX_HW_QUEUES, 4 by default) in the order they are first used; work on two streams of
// one queue runs strictly in order.  A host that keeps two batches in flight on two handles needs two streams that do NOT share a queue, and
// HIP has no call that tells: so the streams are created one by one and each candidate is TESTED — an idle wave of 40 us goes to every stream
// accepted so far and to the candidate at once; side by side the set takes 40 us, one after the other a multiple.
int mi_streams_create_distinct(int device, int n, void** streams) {
    return guarded([&] {
        require(streams != nullptr, "null argument");
        require(n >= 1 && n <= 4, "n must be 1 .. 4");
        mi::hip_check(hipSetDevice(device), "hipSetDevice");
        for (int k = 0; k < n; k++) streams[k] = nullptr;
        int* sink = nullptr;
        mi::hip_check(hipMalloc(reinterpret_cast<void**>(&sink), sizeof(int)), "hipMalloc");
        std::vector<hipStream_t> accepted, rejected;
        auto cleanup = [&](bool all) {
            for (hipStream_t s : rejected) hipStreamDestroy(s);
            if (all) for (hipStream_t s : accepted) hipStreamDestroy(s);
            hipFree(sink);
        };
        const long long ticks = 40 * 100;   // 40 us of the 100 MHz wall clock
        auto timed_together = [&](hipStream_t cand) {
            double best = 1e30;
            for (int rep = 0; rep < 3; rep++) {
                for (hipStream_t s : accepted) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
                mi::hip_check(hipStreamSynchronize(cand), "hipStreamSynchronize");
                const auto t0 = std::chrono::steady_clock::now();
                for (hipStream_t s : accepted)
                    if (mi::launch_spin(ticks, 1 << 20, sink, s) != 0) throw std::runtime_error("spin kernel launch failed");
                if (mi::launch_spin(ticks, 1 << 20, sink, cand) != 0) throw std::runtime_error("spin kernel launch failed");
                for (hipStream_t s : accepted) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
                mi::hip_check(hipStreamSynchronize(cand), "hipStreamSynchronize");
                best = std::min(best, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
            }
            return best;
        };
        try {
            for (int tries = 0; tries < 16 && static_cast<int>(accepted.size()) < n; tries++) {
                hipStream_t c = nullptr;
                mi::hip_check(hipStreamCreateWithFlags(&c, hipStreamNonBlocking), "hipStreamCreate");
                if (accepted.empty()) {
                    if (mi::launch_spin(ticks, 1 << 20, sink, c) != 0) throw std::runtime_error("spin kernel launch failed");   // (first use: the stream gets its queue)
                    mi::hip_check(hipStreamSynchronize(c), "hipStreamSynchronize");
                    accepted.push_back(c);
                    continue;
                }
                // side by side: about one idle wave (40 us + launch and synchronisation cost); sharing a queue with any accepted stream: two or more
                if (timed_together(c) < 1.6 * 40.0 + 30.0 * static_cast<double>(accepted.size())) accepted.push_back(c);
                else rejected.push_back(c);
            }
        } catch (...) {
            cleanup(true);
            throw;
        }
        if (static_cast<int>(accepted.size()) < n) {
            cleanup(true);
            throw ApiError(MI_EDEVICE, "could not find that many streams on distinct hardware queues (GPU_MAX_HW_QUEUES?)");
        }
        for (int k = 0; k < n; k++) streams[k] = accepted[static_cast<size_t>(k)];
        cleanup(false);
    });
}

int mi_streams_destroy(int device, int n, void** streams) {
    return guarded([&] {
        require(streams != nullptr && n >= 0, "bad argument");
        mi::hip_check(hipSetDevice(device), "hipSetDevice");
        for (int k = 0; k < n; k++)
            if (streams[k]) {
                mi::hip_check(hipStreamSynchronize(static_cast<hipStream_t>(streams[k])), "hipStreamSynchronize");
                mi::hip_check(hipStreamDestroy(static_cast<hipStream_t>(streams[k])), "hipStreamDestroy");
                streams[k] = nullptr;
            }
    });
}

int mi_dist_broadcast_bytes(const char* id_path, int rank, int world, int root, int device, uint8_t* buf, size_t nbytes, int timeout_ms) {
    return guarded([&] {
        require(id_path && buf, "null argument");
        require(world >= 1 && rank >= 0 && rank < world && root >= 0 && root < world, "rank / root outside [0, world)");
        require(nbytes > 0 && nbytes <= (static_cast<size_t>(1) << 31), "nbytes must be in (0, 2 GiB]");
        mi::hip_check(hipSetDevice(device), "hipSetDevice");
        static std::mutex mu;
        static Rccl R;
        {
            std::lock_guard<std::mutex> g(mu);
            if (!R.lib) {
                void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
                if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
                if (!lib) throw ApiError(MI_EDEVICE, std::string("librccl is not loadable: ") + dlerror());
                auto sym = [&](const char* n) {
                    void* p = dlsym(lib, n);
                    if (!p) throw ApiError(MI_EDEVICE, std::string("librccl lacks ") + n);
                    return p;
                };
                R.GetUniqueId = reinterpret_cast<decltype(R.GetUniqueId)>(sym("ncclGetUniqueId"));
                R.CommInitRank = reinterpret_cast<decltype(R.CommInitRank)>(sym("ncclCommInitRank"));
                R.Broadcast = reinterpret_cast<decltype(R.Broadcast)>(sym("ncclBroadcast"));
                R.CommDestroy = reinterpret_cast<decltype(R.CommDestroy)>(sym("ncclCommDestroy"));
                R.GetErrorString = reinterpret_cast<decltype(R.GetErrorString)>(sym("ncclGetErrorString"));
                R.lib = lib;
            }
        }
        auto nccl = [&](int rc, const char* what) {
            if (rc != 0) throw ApiError(MI_EDEVICE, std::string(what) + ": " + (R.GetErrorString ? R.GetErrorString(rc) : "rccl error"));
        };
        UniqueId id{};
        const std::string path = id_path, tmp = path + ".tmp";
        // rendezvous file: {"MIRV", world, root} + the 128-byte id.  A file of another job shape is never taken for this one's; a stale file of the
        // SAME shape (a crashed earlier run under a reused name) cannot be told from a root that was simply early — for that case ncclCommInitRank
        // runs under the caller's timeout below instead of blocking for ever.
        const uint32_t head[3] = {0x5652494du, static_cast<uint32_t>(world), static_cast<uint32_t>(root)};
        if (rank == root) {
            std::remove(path.c_str());   // whatever an earlier run left under this name
            nccl(R.GetUniqueId(&id), "ncclGetUniqueId");
            {
                std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
                if (!f || !f.write(reinterpret_cast<const char*>(head), sizeof head) || !f.write(id.internal, sizeof id.internal))
                    throw ApiError(MI_EIO, "cannot write the rendezvous file '" + tmp + "'");
            }
            if (std::rename(tmp.c_str(), path.c_str()) != 0) throw ApiError(MI_EIO, "cannot publish the rendezvous file '" + path + "'");
        } else {
            const auto t0 = std::chrono::steady_clock::now();
            for (;;) {
                std::ifstream f(path, std::ios::binary);
                uint32_t got[3] = {0, 0, 0};
                if (f && f.read(reinterpret_cast<char*>(got), sizeof got) && got[0] == head[0] && got[1] == head[1] && got[2] == head[2] &&
                    f.read(id.internal, sizeof id.internal) && f.gcount() == static_cast<std::streamsize>(sizeof id.internal))
                    break;
                if (timeout_ms >= 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms))
                    throw ApiError(MI_EIO, "no rendezvous file '" + path + "' of this job (world " + std::to_string(world) + ", root " + std::to_string(root) + ") from the root rank within the timeout");
                std::this_thread::sleep_for(std::chrono::milliseconds(2));
            }
        }
        void* comm = nullptr;
        uint8_t* d = nullptr;
        hipStream_t s = nullptr;
        try {
            if (timeout_ms >= 0 && world > 1) {
                // bounded: a communicator that does not form (a stale id, a rank that died) must not hang the caller.  The call cannot be cancelled; on
                // a timeout its thread is left behind and the caller gets MI_EIO (and is expected to exit)
                struct Init { std::mutex m; std::condition_variable cv; bool done = false; int rc = 0; void* comm = nullptr; };
                auto st = std::make_shared<Init>();
                auto fn = R.CommInitRank;
                std::thread([st, fn, world, id, rank, device] {
                    hipSetDevice(device);
                    void* c = nullptr;
                    const int rc = fn(&c, world, id, rank);
                    std::lock_guard<std::mutex> g(st->m);
                    st->rc = rc; st->comm = c; st->done = true;
                    st->cv.notify_all();
                }).detach();
                std::unique_lock<std::mutex> lk(st->m);
                // (the id exchange itself is quick; the bound is the caller's timeout, at least 10 s for the bootstrap of a whole node)
                if (!st->cv.wait_for(lk, std::chrono::milliseconds(std::max(timeout_ms, 10000)), [&] { return st->done; }))
                    throw ApiError(MI_EIO, "ncclCommInitRank did not complete within the timeout (a stale rendezvous file '" + path + "', or a rank that never arrived)");
                comm = st->comm;
                nccl(st->rc, "ncclCommInitRank");
            } else {
                nccl(R.CommInitRank(&comm, world, id, rank), "ncclCommInitRank");
            }
            if (rank == root) std::remove(path.c_str());   // every rank has read it: CommInitRank is collective
            mi::hip_check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
            mi::hip_check(hipMalloc(reinterpret_cast<void**>(&d), nbytes), "hipMalloc");
            if (rank == root) mi::hip_check(hipMemcpyAsync(d, buf, nbytes, hipMemcpyHostToDevice, s), "H2D model bytes");
            nccl(R.Broadcast(d, d, nbytes, /* ncclUint8 */ 1, root, comm, s), "ncclBroadcast");
            if (rank != root) mi::hip_check(hipMemcpyAsync(buf, d, nbytes, hipMemcpyDeviceToHost, s), "D2H model bytes");
            mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        } catch (...) {
            if (d) hipFree(d);
            if (s) hipStreamDestroy(s);
            if (comm) R.CommDestroy(comm);
            throw;
        }
        hipFree(d);
        hipStreamDestroy(s);
        nccl(R.CommDestroy(comm), "ncclCommDestroy");
    });
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
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        mi::JpegFrame f;
        try {
            mi::jpeg_entropy_decode(bytes, nbytes, &f);  // host: the serial part
        } catch (const std::runtime_error& e) {
            throw ApiError(MI_EINVAL, e.what());
        }
        const size_t out_bytes = static_cast<size_t>(3) * f.width * f.height;
        if (cap_bytes < out_bytes) throw ApiError(MI_EINVAL, "rgb buffer too small for the decoded picture");
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) throw ApiError(MI_EDEVICE, "no such HIP device (the JPEG sample arithmetic runs on the GPU; no CPU fallback exists)");
        mi::hip_check(hipSetDevice(device), "hipSetDevice");
        hipStream_t s = static_cast<hipStream_t>(stream);
        DeviceBuf coef, qt, planes, out;
        const size_t coef_bytes = f.coef.size() * sizeof(int16_t);
        auto* d_coef = static_cast<int16_t*>(coef.get(coef_bytes));
        auto* d_qt = static_cast<uint16_t*>(qt.get(sizeof f.qt));
        auto* d_planes = static_cast<uint8_t*>(planes.get(mi::jpeg_plane_bytes(f)));
        uint8_t* d_rgb = mem == MI_MEM_DEVICE ? rgb : static_cast<uint8_t*>(out.get(out_bytes));
        mi::hip_check(hipMemcpyAsync(d_coef, f.coef.data(), coef_bytes, hipMemcpyHostToDevice, s), "H2D coefficients");
        mi::hip_check(hipMemcpyAsync(d_qt, f.qt, sizeof f.qt, hipMemcpyHostToDevice, s), "H2D quantisation tables");
        jpeg_launch(f, d_coef, d_qt, d_planes, d_rgb, s);
        if (mem == MI_MEM_HOST) mi::hip_check(hipMemcpyAsync(rgb, d_rgb, out_bytes, hipMemcpyDeviceToHost, s), "D2H rgb");
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
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) throw ApiError(MI_EDEVICE, "no such HIP device");
        mi::hip_check(hipSetDevice(device), "hipSetDevice");
        hipStream_t s = static_cast<hipStream_t>(stream);
        DeviceBuf img, outbuf;
        float* d_out = out;
        size_t ob = sizeof(float) * 3 * out_w * out_h;
        if (mem == MI_MEM_HOST) d_out = static_cast<float*>(outbuf.get(ob));
        mi::image_to_tensor_device(rgb, width, height, stride, roi, out_w, out_h, keep_aspect_ratio != 0, range_min, range_max,
                                   flip_horizontal != 0, d_out, padding_out, img.get(mi::image_to_tensor_scratch_bytes(width, height, stride, roi, out_w, out_h, keep_aspect_ratio != 0)), s);
        if (mem == MI_MEM_HOST) mi::hip_check(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, s), "D2H tensor");
        mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    });
}

extern "C++" {
namespace {
// bytes `batch` frames of `height` rows own: the last row owns row_bytes, not a whole stride
size_t picture_bytes(int batch, int height, int stride, size_t row_bytes) {
    return static_cast<size_t>(stride) * height * (batch - 1) + static_cast<size_t>(stride) * (height - 1) + row_bytes;
}

// everything mi_render_annotations and mi_render_faces check about their pictures, before any device is touched
void render_check_canvas(const uint8_t* frames, int batch, int width, int height, int stride, const uint8_t* out, int out_channels, int out_stride,
                         int mem) {
    require(frames && out, "null argument");
    require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
    require(batch > 0 && width > 0 && height > 0, "bad frame geometry");
    require(stride >= 3 * static_cast<long>(width), "stride is smaller than 3 * width");
    require(out_channels == 3 || out_channels == 4, "out_channels must be 3 (RGB) or 4 (RGBA)");
    require(out_stride >= out_channels * static_cast<long>(width), "out_stride is smaller than out_channels * width");
    if (out == frames) {
        require(out_channels == 3 && out_stride == stride, "out may be frames (in place) only with out_channels 3 and out_stride == stride");
        return;
    }
    const uint8_t* in_end = frames + picture_bytes(batch, height, stride, static_cast<size_t>(3) * width);
    const uint8_t* out_end = out + picture_bytes(batch, height, out_stride, static_cast<size_t>(out_channels) * width);
    require(out_end <= frames || in_end <= out, "out overlaps frames (only out == frames, in place, is an alias this call accepts)");
}

// The part the two render entries share: staging of the pictures for host callers (tight rows on the device), the canvas phase, the
// draw phase (`draw(canvas, d_skipped, stream)` stages its own operands and launches), the way back.  Rows travel back without
// their padding: the bytes of the caller's rows beyond out_channels * width are never written.
template <class Draw>
void render_run(int device, const uint8_t* frames, int batch, int width, int height, int stride, uint8_t* out, int out_channels, int out_stride,
                int* skipped, int mem, void* stream, bool always_wait, Draw draw) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) throw ApiError(MI_EDEVICE, "no such HIP device (the renderer runs on the GPU; no CPU fallback exists)");
    mi::hip_check(hipSetDevice(device), "hipSetDevice");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceBuf b_frames, b_out, b_skipped;
    mi::RenderCanvas cv{frames, out, batch, width, height, stride, out_stride, out_channels};
    int* d_skipped = skipped;
    const size_t rows = static_cast<size_t>(batch) * height, in_row = static_cast<size_t>(3) * width, out_row = static_cast<size_t>(out_channels) * width;
    if (mem == MI_MEM_HOST) {
        auto* d_frames = static_cast<uint8_t*>(b_frames.get(rows * in_row));
        mi::hip_check(hipMemcpy2DAsync(d_frames, in_row, frames, stride, in_row, rows, hipMemcpyHostToDevice, s), "H2D frames");
        cv.frames = d_frames;
        cv.stride = static_cast<int>(in_row);
        cv.out = out == frames ? d_frames : static_cast<uint8_t*>(b_out.get(rows * out_row));
        cv.out_stride = static_cast<int>(out_row);
        if (skipped) d_skipped = static_cast<int*>(b_skipped.get(sizeof(int) * batch));
    }
    hipError_t e = mi::launch_render_canvas(cv, s);
    if (e != hipSuccess) throw std::runtime_error(std::string("render canvas kernel launch failed: ") + hipGetErrorString(e));
    draw(cv, d_skipped, s);
    if (mem == MI_MEM_HOST) {
        mi::hip_check(hipMemcpy2DAsync(out, out_stride, cv.out, out_row, out_row, rows, hipMemcpyDeviceToHost, s), "D2H picture");
        if (skipped) mi::hip_check(hipMemcpyAsync(skipped, d_skipped, sizeof(int) * batch, hipMemcpyDeviceToHost, s), "D2H skipped");
    }
    if (mem == MI_MEM_HOST || !stream || always_wait) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
}
}  // namespace
}  // extern "C++"

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
                       const size_t ann_bytes = sizeof(mi_annotation) * n_anns, coord_bytes = sizeof(double) * coords_per_frame * batch;
                       auto* d_anns = static_cast<mi_annotation*>(b_anns.get(ann_bytes + 16));
                       if (n_anns) mi::hip_check(hipMemcpyAsync(d_anns, anns, ann_bytes, hipMemcpyHostToDevice, s), "H2D annotations");
                       const double* d_coords = coords;
                       if (mem == MI_MEM_HOST && reads) {
                           d_coords = static_cast<const double*>(b_coords.get(coord_bytes));
                           mi::hip_check(hipMemcpyAsync(const_cast<double*>(d_coords), coords, coord_bytes, hipMemcpyHostToDevice, s), "H2D coords");
                       }
                       hipError_t e = mi::launch_render_annotations(cv, d_anns, n_anns, d_coords, coords_per_frame, d_skipped, s);
                       if (e != hipSuccess) throw std::runtime_error(std::string("render kernel launch failed: ") + hipGetErrorString(e));
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
                       auto staged = [&](DeviceBuf& buf, const void* p, size_t bytes) -> const void* {
                           if (!p || mem == MI_MEM_DEVICE) return p;
                           void* d = buf.get(bytes);
                           mi::hip_check(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, s), "H2D results");
                           return d;
                       };
                       const size_t B = static_cast<size_t>(batch);
                       auto* d_faces = static_cast<const mi_detection*>(staged(b_faces, faces, sizeof(mi_detection) * B * (faces ? faces_per_frame : 0)));
                       auto* d_counts = static_cast<const int*>(staged(b_counts, faces ? face_counts : nullptr, sizeof(int) * B));
                       auto* d_landmarks = static_cast<const float*>(staged(b_landmarks, landmarks, sizeof(float) * B * MI_NUM_FACE_LANDMARKS * 3));
                       auto* d_present = static_cast<const int*>(staged(b_present, present, sizeof(int) * B));
                       auto* d_eyes = static_cast<const float*>(staged(b_eyes, eyes, sizeof(float) * B * 2 * (MI_NUM_EYE_LANDMARKS + MI_NUM_IRIS_LANDMARKS) * 3));
                       hipError_t e = mi::launch_render_faces(cv, d_faces, d_counts, faces_per_frame, d_landmarks, d_present, d_eyes, *style, d_skipped, s);
                       if (e != hipSuccess) throw std::runtime_error(std::string("render kernel launch failed: ") + hipGetErrorString(e));
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
                       auto staged = [&](DeviceBuf& buf, const void* p, size_t bytes) -> const void* {
                           if (!p || mem == MI_MEM_DEVICE) return p;
                           void* d = buf.get(bytes);
                           mi::hip_check(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, s), "H2D results");
                           return d;
                       };
                       const size_t B = static_cast<size_t>(batch), M = static_cast<size_t>(max_items);
                       auto* d_faces = static_cast<const mi_detection*>(staged(b_faces, faces, sizeof(mi_detection) * B * (faces ? max_faces : 0)));
                       auto* d_counts = static_cast<const int*>(staged(b_counts, faces ? face_counts : nullptr, sizeof(int) * B));
                       auto* d_item_frame = static_cast<const int*>(staged(b_item_frame, item_frame, sizeof(int) * M));
                       auto* d_n_items = static_cast<const int*>(staged(b_n_items, n_items, sizeof(int)));
                       auto* d_landmarks = static_cast<const float*>(staged(b_landmarks, landmarks, sizeof(float) * M * MI_NUM_FACE_LANDMARKS * 3));
                       auto* d_present = static_cast<const int*>(staged(b_present, item_frame ? present : nullptr, sizeof(int) * M));
                       auto* d_eyes = static_cast<const float*>(staged(b_eyes, eyes, sizeof(float) * M * 2 * (MI_NUM_EYE_LANDMARKS + MI_NUM_IRIS_LANDMARKS) * 3));
                       hipError_t e = mi::launch_render_face_items(cv, d_faces, d_counts, max_faces, d_item_frame, d_n_items, max_items, d_landmarks,
                                                                   d_present, d_eyes, *style, d_skipped, s);
                       if (e != hipSuccess) throw std::runtime_error(std::string("render kernel launch failed: ") + hipGetErrorString(e));
                   });
    });
}

// ------------------------------------------------------------------------------------------------ FaceEmbeddings
static void fe_finish_create(mi_fe* h) {
    mi::Model& m = *h->model.m;
    const auto d = m.input_dims();
    if (!(d.size() == 4 && d[0] == 1 && d[1] == mi::kChipSize && d[2] == mi::kChipSize && d[3] == 3))
        throw ApiError(MI_EINVAL, "incompatible model: the input must be [1,112,112,3] (image_to_tensor(crop, None, (112,112), ..), face_embeddings.rs:55)");
    if (m.num_outputs() != 1) throw ApiError(MI_EINVAL, "incompatible model: exactly one output is expected (face_embeddings.rs:74-75), found " + std::to_string(m.num_outputs()));
    const auto& o = m.output_dims(0);
    const size_t D = m.output_elems(0);
    if (o.empty() || o[0] != 1 || D < 1 || D > (1u << 24))
        throw ApiError(MI_EINVAL, "incompatible model: the output must hold D >= 1 values per frame ([1,D] or [1,1,1,D])");
    h->features = static_cast<int>(D);
}

int mi_fe_create_from_bytes(const uint8_t* tflite, size_t nbytes, int device, mi_fe** out) {
    return guarded([&] {
        require(tflite && nbytes && out, "null argument");
        auto h = std::make_unique<mi_fe>();
        h->model.m = std::make_unique<mi::Model>(tflite, nbytes, device);
        fe_finish_create(h.get());
        *out = h.release();
    });
}

int mi_fe_create(const char* model_path, int device, mi_fe** out) {
    return guarded([&] {
        require(out, "null argument");
        auto bytes = read_file(model_path ? model_path : "./models/face_embeddings.tflite");  // face_embeddings.rs:33-37
        auto h = std::make_unique<mi_fe>();
        h->model.m = std::make_unique<mi::Model>(bytes.data(), bytes.size(), device);
        fe_finish_create(h.get());
        *out = h.release();
    });
}

void mi_fe_free(mi_fe* h) { delete h; }
mi_model* mi_fe_model(mi_fe* h) { return h ? &h->model : nullptr; }

int mi_fe_features(const mi_fe* h, int* features) {
    return guarded([&] {
        require(h && features, "null argument");
        *features = h->features;
    });
}

int mi_face_chip_rect(const mi_detection* det, int width, int height, int rect[4], int* valid) {
    return guarded([&] {
        require(det && rect && valid, "null argument");
        require(width > 0 && height > 0, "bad image geometry");
        *valid = mi::face_chip_rect_det(det->data, width, height, rect);
    });
}

int mi_fe_infer_image(mi_fe* h, const uint8_t* rgb, int width, int height, int stride, const double bbox[4], float* embedding, int cap) {
    return guarded([&] {
        require(h && rgb && bbox && embedding, "null argument");
        require(width > 0 && height > 0 && stride >= 3 * static_cast<long>(width), "bad image geometry");
        require(cap >= h->features, "output capacity is smaller than the model's feature count");
        int r[4];
        if (!mi::face_chip_rect_px(bbox, width, height, r))
            throw ApiError(MI_ERANGE, "bounding box leaves the image or is empty (reference: Mat::roi(..).unwrap() panics, face_embeddings.rs:102-107)");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = m.stream();
        Use use(h->model, s);
        const int D = h->features;
        // only the crop travels: rows y .. y + h - 1 from column x on; the last row owns 3 * w bytes
        const uint8_t* crop = rgb + static_cast<size_t>(stride) * r[1] + static_cast<size_t>(3) * r[0];
        const size_t crop_bytes = static_cast<size_t>(stride) * (r[3] - 1) + static_cast<size_t>(3) * r[2];
        auto* d_crop = static_cast<uint8_t*>(h->d_img.get(crop_bytes));
        float* d_in = static_cast<float*>(h->d_in.get(m.input_elems() * sizeof(float)));
        float* d_emb = static_cast<float*>(h->d_emb.get(sizeof(float) * D));
        mi::hip_check(hipMemcpyAsync(d_crop, crop, crop_bytes, hipMemcpyHostToDevice, s), "H2D crop");
        mi::chip_tensor_enqueue_one(d_crop, r[2], r[3], stride, d_in, s);
        m.run_device(d_in, 1, s);
        mi::launch_l2_norm(m.output_device(0), nullptr, 1, D, d_emb, nullptr, s);
        mi::hip_check(hipMemcpyAsync(embedding, d_emb, sizeof(float) * D, hipMemcpyDeviceToHost, s), "D2H embedding");
        mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    });
}

int mi_fe_infer_face_items(mi_fe* h, const uint8_t* frames, int batch, int width, int height, int stride, const mi_detection* faces, int max_faces,
                           const int* item_frame, const int* item_face, int max_items, float* embeddings, int* valid, float* raw, float* chips,
                           int mem, void* stream) {
    return guarded([&] {
        // (a budget the launches cannot take is refused here, before anything is queued)
        require_face_items(batch, max_faces, max_items, mi::kFaceItemsMaxRunItems, "max_items must be 1..32767 (one grid row of a launch per item)");
        require(h && frames && faces && item_frame && item_face && embeddings && valid, "null argument");
        require(width > 0 && height > 0 && stride >= 3 * static_cast<long>(width), "bad frame geometry");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        static_assert(sizeof(mi_detection) == 17 * sizeof(float), "mi_detection layout");
        mi::Model& m = *h->model.m;
        mi::hip_check(hipSetDevice(m.device()), "hipSetDevice");
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : m.stream();
        Use use(h->model, s);
        const int B = batch, M = max_items, D = h->features;
        const size_t chip_floats = m.input_elems(), emb_bytes = sizeof(float) * D * M;
        mi::ChipItems it{};
        it.frames = frames; it.frame_bytes = static_cast<long>(stride) * height; it.batch = B; it.width = width; it.height = height; it.stride = stride;
        it.faces = reinterpret_cast<const float*>(faces); it.max_faces = max_faces; it.item_frame = item_frame; it.item_face = item_face; it.N = M;
        float *d_emb = embeddings, *d_raw = raw;
        int* d_valid = valid;
        if (mem == MI_MEM_HOST) {
            auto staged = [&](DeviceBuf& buf, const void* p, size_t bytes) -> const void* {
                void* d = buf.get(bytes);
                mi::hip_check(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, s), "H2D operands");
                return d;
            };
            it.frames = static_cast<const uint8_t*>(h->d_frames.get(static_cast<size_t>(stride) * height * B));
            mi::hip_check(hipMemcpyAsync(const_cast<uint8_t*>(it.frames), frames, frames_bytes(B, width, height, stride), hipMemcpyHostToDevice, s), "H2D frames");
            it.faces = static_cast<const float*>(staged(h->d_faces, faces, sizeof(mi_detection) * B * max_faces));
            it.item_frame = static_cast<const int*>(staged(h->d_item_frame, item_frame, sizeof(int) * M));
            it.item_face = static_cast<const int*>(staged(h->d_item_face, item_face, sizeof(int) * M));
            d_emb = static_cast<float*>(h->d_emb.get(emb_bytes));
            d_raw = raw ? static_cast<float*>(h->d_raw.get(emb_bytes)) : nullptr;
            d_valid = static_cast<int*>(h->d_valid.get(sizeof(int) * M));
        }
        // the network's input is the handle's own buffer whatever `chips` is: the engine keys its captured graphs by that address
        auto* d_geom = static_cast<mi::ChipGeom*>(h->d_geom.get(sizeof(mi::ChipGeom) * M));
        float* d_in = static_cast<float*>(h->d_in.get(chip_floats * sizeof(float) * M));
        mi::launch_chip_geom(it, d_geom, d_valid, s);
        mi::launch_chip_tensor(it, d_geom, d_in, s);
        m.run_device(d_in, M, s);
        mi::launch_l2_norm(m.output_device(0), d_valid, M, D, d_emb, d_raw, s);
        if (chips) mi::hip_check(hipMemcpyAsync(chips, d_in, chip_floats * sizeof(float) * M, mem == MI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s), "chips copy");
        if (mem == MI_MEM_HOST) {
            mi::hip_check(hipMemcpyAsync(embeddings, d_emb, emb_bytes, hipMemcpyDeviceToHost, s), "D2H embeddings");
            if (raw) mi::hip_check(hipMemcpyAsync(raw, d_raw, emb_bytes, hipMemcpyDeviceToHost, s), "D2H raw");
            mi::hip_check(hipMemcpyAsync(valid, d_valid, sizeof(int) * M, hipMemcpyDeviceToHost, s), "D2H valid");
        }
        if (mem == MI_MEM_HOST || !stream) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    });
}

int mi_l2_norm(const float* in, int n, float* out) {
    return guarded([&] {
        require(in && out, "null argument");
        require(n >= 1, "n must be positive");
        const float norm = mi::embed_sqrt(mi::embed_dot(in, in, n));
        for (int k = 0; k < n; k++) out[k] = mi::embed_div(in[k], norm);
    });
}

int mi_similarity_score(const float* a, const float* b, int n, float* out) {
    return guarded([&] {
        require(a && b && out, "null argument");
        require(n >= 1, "n must be positive");
        const float dot = mi::embed_dot(a, b, n);
        const float norm_a = mi::embed_sqrt(mi::embed_dot(a, a, n)), norm_b = mi::embed_sqrt(mi::embed_dot(b, b, n));
        *out = mi::embed_div(dot, mi::embed_mul(norm_a, norm_b));
    });
}

int mi_similarity_matrix(int device, const float* a, int n, const float* b, int m, int features, float* out, int mem, void* stream) {
    return guarded([&] {
        require(a && b && out, "null argument");
        require(n >= 1 && m >= 1, "n and m must be positive");
        require(features >= 1 && features <= mi::kSimMaxFeatures, "features must be 1..4096");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
            throw ApiError(MI_EDEVICE, "no such HIP device (the similarity matrix runs on the GPU; no CPU fallback exists)");
        mi::hip_check(hipSetDevice(device), "hipSetDevice");
        hipStream_t s = static_cast<hipStream_t>(stream);
        DeviceBuf b_a, b_b, b_out;
        const float *d_a = a, *d_b = b;
        float* d_out = out;
        const size_t a_bytes = sizeof(float) * n * features, b_bytes = sizeof(float) * m * features, out_bytes = sizeof(float) * n * static_cast<size_t>(m);
        if (mem == MI_MEM_HOST) {
            d_a = static_cast<const float*>(b_a.get(a_bytes));
            d_b = static_cast<const float*>(b_b.get(b_bytes));
            d_out = static_cast<float*>(b_out.get(out_bytes));
            mi::hip_check(hipMemcpyAsync(const_cast<float*>(d_a), a, a_bytes, hipMemcpyHostToDevice, s), "H2D a");
            mi::hip_check(hipMemcpyAsync(const_cast<float*>(d_b), b, b_bytes, hipMemcpyHostToDevice, s), "H2D b");
        }
        mi::launch_similarity(d_a, n, d_b, m, features, d_out, s);
        if (mem == MI_MEM_HOST) mi::hip_check(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s), "D2H similarity");
        if (mem == MI_MEM_HOST || !stream) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    });
}

int mi_topk_select(const float* scores, int n, int m, int k, int* index, float* score) {
    return guarded([&] {
        require(scores && index && score, "null argument");
        require(n >= 1 && m >= 1, "n and m must be positive");
        require(k >= 1 && k <= mi::kTopkMaxK, "k must be 1..16");
        for (long i = 0; i < n; i++) mi::topk_select_row(scores + i * m, m, k, index + i * k, score + i * k);
    });
}

int mi_gallery_create(int device, const float* rows, int m, int features, const int* labels, int mem, mi_gallery** out) {
    return guarded([&] {
        require(rows && out, "null argument");
        require(m >= 1 && m <= mi::kGalleryMaxRows, "m must be 1..2^24");
        require(features >= 1 && features <= mi::kSimMaxFeatures, "features must be 1..4096");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
            throw ApiError(MI_EDEVICE, "no such HIP device (a gallery lives on the GPU; no CPU fallback exists)");
        mi::hip_check(hipSetDevice(device), "hipSetDevice");
        auto g = std::make_unique<mi_gallery>();
        g->device = device;
        g->m = m;
        g->features = features;
        const size_t row_bytes = sizeof(float) * static_cast<size_t>(m) * features;
        mi::hip_check(hipMemcpy(g->d_rows.get(row_bytes), rows, row_bytes, mem == MI_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice), "gallery rows copy");
        if (labels) {
            mi::hip_check(hipMemcpy(g->d_labels.get(sizeof(int) * m), labels, sizeof(int) * m, hipMemcpyHostToDevice), "H2D labels");
            g->has_labels = true;
        }
        *out = g.release();
    });
}

void mi_gallery_free(mi_gallery* g) { delete g; }

int mi_gallery_dims(const mi_gallery* g, int* m, int* features) {
    return guarded([&] {
        require(g && m && features, "null argument");
        *m = g->m;
        *features = g->features;
    });
}

int mi_gallery_set_option(mi_gallery* g, const char* key, int value) {
    return guarded([&] {
        require(g && key, "null argument");
        require(std::strcmp(key, "splits") == 0, "unknown option (a gallery has: splits)");
        require(value >= 0 && value <= mi::kGalleryMaxSplits, "splits must be 0 (automatic) or 1..64");
        std::lock_guard<std::mutex> lock(g->sync.mu);
        g->splits = value;
    });
}

int mi_gallery_get_option(mi_gallery* g, const char* key, int* value) {
    return guarded([&] {
        require(g && key && value, "null argument");
        require(std::strcmp(key, "splits") == 0, "unknown option (a gallery has: splits)");
        std::lock_guard<std::mutex> lock(g->sync.mu);
        *value = g->splits;
    });
}

int mi_gallery_topk(mi_gallery* g, const float* queries, int n, int k, int* index, float* score, int* label, int mem, void* stream) {
    return guarded([&] {
        require(g && queries && index && score, "null argument");
        require(n >= 1, "n must be positive");
        require(k >= 1 && k <= mi::kTopkMaxK, "k must be 1..16");
        require(mem == MI_MEM_HOST || mem == MI_MEM_DEVICE, "mem must be MI_MEM_HOST or MI_MEM_DEVICE");
        mi::hip_check(hipSetDevice(g->device), "hipSetDevice");
        hipStream_t s = static_cast<hipStream_t>(stream);
        Use use(g->sync, s);
        const int tiles_m = (g->m + 127) / 128;
        const int splits = g->splits ? (g->splits < tiles_m ? g->splits : tiles_m) : mi::gallery_auto_splits(n, g->m, mi::device_cu_count());
        const size_t N = static_cast<size_t>(n), out_elems = N * k, q_bytes = sizeof(float) * N * g->features;
        // (growing frees the old block, which waits for the calls that still use it)
        auto* d_part = static_cast<mi::TopkPair*>(g->d_part.get(sizeof(mi::TopkPair) * out_elems * splits));
        const float* d_q = queries;
        int *d_index = index, *d_label = label;
        float* d_score = score;
        if (mem == MI_MEM_HOST) {
            d_q = static_cast<const float*>(g->d_queries.get(q_bytes));
            d_index = static_cast<int*>(g->d_index.get(sizeof(int) * out_elems));
            d_score = static_cast<float*>(g->d_score.get(sizeof(float) * out_elems));
            if (label) d_label = static_cast<int*>(g->d_label.get(sizeof(int) * out_elems));
            mi::hip_check(hipMemcpyAsync(const_cast<float*>(d_q), queries, q_bytes, hipMemcpyHostToDevice, s), "H2D queries");
        }
        mi::launch_gallery_topk(d_q, n, static_cast<const float*>(g->d_rows.p), g->m, g->features, k, splits,
                                g->has_labels ? static_cast<const int*>(g->d_labels.p) : nullptr, d_part, d_index, d_score, d_label, s);
        if (mem == MI_MEM_HOST) {
            mi::hip_check(hipMemcpyAsync(index, d_index, sizeof(int) * out_elems, hipMemcpyDeviceToHost, s), "D2H index");
            mi::hip_check(hipMemcpyAsync(score, d_score, sizeof(float) * out_elems, hipMemcpyDeviceToHost, s), "D2H score");
            if (label) mi::hip_check(hipMemcpyAsync(label, d_label, sizeof(int) * out_elems, hipMemcpyDeviceToHost, s), "D2H label");
        }
        if (mem == MI_MEM_HOST || !stream) mi::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    });
}

}  // extern "C"
