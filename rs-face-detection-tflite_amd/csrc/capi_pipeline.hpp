// capi_pipeline.hpp — what capi_pipeline.cpp shares with capi_tracker.cpp (a tracker wraps a private pipeline): the handle, the prologue of an
// entry and the mesh + iris stages of a pass.
#pragma once
#include "capi_internal.hpp"

#include <chrono>
#include <cstdio>

struct mi_pipeline {
    std::unique_ptr<mi_fd> fd;
    std::unique_ptr<mi_fl> fl;
    std::unique_ptr<mi_iris> iris;
    capi::DeviceBuf frames, geom, pad_det, pad_eye, in_det, dets, roi_face, valid_face, in_lm, roi_eye, valid_eye, flip_eye, in_eye;
    capi::SizesCache sizes;   // of the 2 B eyes of a pass over B frames (the B mesh items read its first half)
    // results of a call from host memory: ONE device block (faces | counts | landmarks | present | eyes) and its pinned host image — one
    // asynchronous copy and one synchronisation per call (five copies into the caller's pageable arrays were five synchronous round trips:
    // 115 us of the 0.66 ms of a one-picture call)
    capi::DeviceBuf results;
    capi::OneShot out;
    capi::DeviceBuf geom_det;                        // the detector's letterbox geometry of `geom_B` pictures of geom_w x geom_h (no ROI: uploaded once)
    int geom_B = 0, geom_w = 0, geom_h = 0;
    // mi_pipeline_run_faces: ROI and valid flag of every item slot, and the image sizes of its max_items items (as `sizes`, kept apart so that
    // alternating calls of the two entries upload nothing)
    capi::DeviceBuf roi_item, valid_item;
    capi::SizesCache sizes_item;
    // the streamed form from encoded pictures (mi_pipeline_submit_jpeg / mi_pipeline_collect_jpeg): per slot the decoder's state and picture, the
    // results' device block and its pinned image
    struct PipeJpegSlot {
        capi::DeviceBuf results;
        capi::OneShot out;
        capi::JpegSlot jpeg;   // (last: destroyed first, and its destructor waits for the picture in flight)
    };
    PipeJpegSlot jslot[2];
    capi::StreamClaim jclaim;
    ~mi_pipeline() {
        for (PipeJpegSlot& sl : jslot) sl.jpeg.wait();
    }
};

MI_CAPI_BEGIN

// The prologue of the pipeline's entries: a Call on the detector (device, stream) and the claims on the mesh and the iris network behind
// it — the pipeline's own three handles, always in this order.
struct PipeCall {
    Call fd;
    Use fl, iris;
    const hipStream_t s;
    explicit PipeCall(mi_pipeline* p, void* stream = nullptr) : fd(p->fd->model, stream), fl(p->fl->model, fd.s), iris(p->iris->model, fd.s), s(fd.s) {}
};

struct PipeTrace {   // MI_PIPE_TRACE=1: host-side step times of a pass, to stderr
    const bool on;
    std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    PipeTrace() : on(enabled()) {}
    static bool enabled() { static const bool e = getenv("MI_PIPE_TRACE") != nullptr; return e; }
    void operator()(const char* what) const {
        if (on) std::fprintf(stderr, "  %-22s %8.1f us\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count());
    }
};

constexpr int kPipeCap = 4;   // detections per frame the top-1 flows keep
constexpr long kEyeFs = 3L * (MI_NUM_EYE_LANDMARKS + MI_NUM_IRIS_LANDMARKS);

// The mesh and iris stages of a pass for N items whose face ROIs (and valid flags) are in device memory: item i reads frame i of `it`, or frame
// it.item_frame[i] when that is set.  d_sizes: the image sizes of the pass's 2 N eyes (SizesCache).
void pipeline_mesh_iris(mi_pipeline* p, mi::PreItems& it, int N, const mi::RectD* d_roi_face, const int* d_valid_face, const int* d_sizes, float* lm,
                        int* present, float* eyes, bool one_shot, hipStream_t s, const PipeTrace& tr);

MI_CAPI_END
