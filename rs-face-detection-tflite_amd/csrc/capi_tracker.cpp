// capi_tracker.cpp — mi_tracker: landmark-to-ROI face tracking for S video streams (track.hpp states the rules).  A tracker wraps a PRIVATE
// pipeline (its own three networks, buffers and geometry caches) and adds the per-stream state and three small launches per step.
#include "capi_pipeline.hpp"
#include "track.hpp"

using namespace mi::capi;

struct mi_tracker {
    mi_pipeline* pipe = nullptr;
    int S = 0;
    int start = 0;                       // the detect plan's first stream of the next step (host arithmetic, a kernel argument)
    DeviceBuf state_roi, state_tracked;  // the state: RectD [S], int [S]
    DeviceBuf stream_slot, det_counts, valid_mesh;
    int geom_D = 0, geom_w = 0, geom_h = 0;   // what the private pipeline's geom_det / pad_det hold (the plan kernel rewrites `valid` alone)
    bool launches_only = false;          // option "track_launches_only": a step queues its three own launches alone (tools/track_probe.py times them)
    int full_D = 0, full_w = 0, full_h = 0;   // the geometry of the last full step: it sized and wrote every buffer those launches read
    ~mi_tracker() { mi_pipeline_free(pipe); }
};

namespace {
struct TrackOut {   // DEVICE pointers of one step
    mi_detection* faces;   // [S]
    int* counts;           // [S]
    int* source;           // [S]
    mi::RectD* rois;       // [S]
    float* lm;             // [S][468][3]
    int* present;          // [S]
    float* eyes;           // [S][2][76][3]
    int* det_stream;       // [D]
    int* n_detect;         // [2]
};
struct TrackLayout {       // one block (host memory calls): faces | counts | source | rois | landmarks | present | eyes | det_stream | n_detect
    size_t faces, counts, source, rois, lm, present, eyes, det_stream, n_detect, bytes;
    TrackLayout(int S, int D) {
        auto up16 = [](size_t v) { return (v + 15) & ~static_cast<size_t>(15); };
        faces = 0;
        counts = up16(faces + sizeof(mi_detection) * S);
        source = up16(counts + sizeof(int) * S);
        rois = up16(source + sizeof(int) * S);
        lm = up16(rois + sizeof(mi::RectD) * S);
        present = up16(lm + sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * S);
        eyes = up16(present + sizeof(int) * S);
        det_stream = up16(eyes + sizeof(float) * kEyeFs * 2 * S);
        n_detect = up16(det_stream + sizeof(int) * D);
        bytes = up16(n_detect + sizeof(int) * 2);
    }
    TrackOut in(char* base) const {
        return TrackOut{reinterpret_cast<mi_detection*>(base + faces), reinterpret_cast<int*>(base + counts), reinterpret_cast<int*>(base + source),
                        reinterpret_cast<mi::RectD*>(base + rois), reinterpret_cast<float*>(base + lm), reinterpret_cast<int*>(base + present),
                        reinterpret_cast<float*>(base + eyes), reinterpret_cast<int*>(base + det_stream), reinterpret_cast<int*>(base + n_detect)};
    }
};
static_assert(sizeof(mi::RectD) == sizeof(mi_rect), "RectD is mi_rect's image");

void require_streams(int streams) { require(streams >= 1 && streams <= mi::kTrackMaxStreams, "streams must be 1..32767 (2 * streams eyes, one per grid row of a launch)"); }

// every stream lost, and the plan starts at stream 0 (the caller holds the handle's lock and synchronises)
void lose_all(mi_tracker* t, hipStream_t s) {
    mi::hip_check(hipMemsetAsync(t->state_roi.as<mi::RectD>(t->S), 0, sizeof(mi::RectD) * t->S, s), "hipMemsetAsync state");
    mi::hip_check(hipMemsetAsync(t->state_tracked.as<int>(t->S), 0, sizeof(int) * t->S, s), "hipMemsetAsync state");
    t->start = 0;
}

// the handle around a pipeline that has just been created: the state of S streams, all lost.  The pipeline stays the CALLER's until this
// has succeeded: where it throws, the half-made handle goes without touching the pipeline, and the caller frees that, once.
void tracker_finish(mi_pipeline* pipe, int streams, mi_tracker** out) {
    auto t = std::make_unique<mi_tracker>();
    t->S = streams;
    {
        PipeCall c(pipe);
        lose_all(t.get(), c.s);
        t->stream_slot.as<int>(streams);
        t->valid_mesh.as<int>(streams);
        c.fd.sync();
    }
    t->pipe = pipe;
    *out = t.release();
}
}  // namespace

extern "C" {

int mi_tracker_create(int fd_kind, const char* model_dir, int device, int streams, mi_tracker** out) {
    return guarded([&] {
        require(out, "null argument");
        require_streams(streams);
        mi_pipeline* pipe = nullptr;
        if (int rc = mi_pipeline_create(fd_kind, model_dir, device, &pipe)) throw ApiError(rc, last_error());
        try {
            tracker_finish(pipe, streams, out);
        } catch (...) {
            mi_pipeline_free(pipe);
            throw;
        }
    });
}

int mi_tracker_create_from_bytes(int fd_kind, const uint8_t* fd_tflite, size_t fd_nbytes, const uint8_t* fl_tflite, size_t fl_nbytes,
                                 const uint8_t* iris_tflite, size_t iris_nbytes, int device, int streams, mi_tracker** out) {
    return guarded([&] {
        require(out, "null argument");
        require_streams(streams);
        mi_pipeline* pipe = nullptr;
        if (int rc = mi_pipeline_create_from_bytes(fd_kind, fd_tflite, fd_nbytes, fl_tflite, fl_nbytes, iris_tflite, iris_nbytes, device, &pipe))
            throw ApiError(rc, last_error());
        try {
            tracker_finish(pipe, streams, out);
        } catch (...) {
            mi_pipeline_free(pipe);
            throw;
        }
    });
}

void mi_tracker_free(mi_tracker* t) { delete t; }

int mi_tracker_set_option(mi_tracker* t, const char* key, int value) {
    return guarded([&] {
        require(t && key, "null argument");
        if (std::strcmp(key, "track_launches_only") == 0) {
            PipeCall c(t->pipe);   // (the handle's lock: a step reads the flag under it)
            const bool was = t->launches_only;
            t->launches_only = value != 0;
            if (was && !t->launches_only) {   // what the launches-only steps made of the state means nothing: every stream is lost again
                lose_all(t, c.s);
                c.fd.sync();
            }
            return;
        }
        if (int rc = mi_pipeline_set_option(t->pipe, key, value)) throw ApiError(rc, last_error());
    });
}

int mi_track_roi_from_landmarks(const float* landmarks, int width, int height, mi_rect* roi, int* valid) {
    return guarded([&] {
        require(landmarks && roi && valid, "null argument");
        require(width > 0 && height > 0, "bad frame geometry");
        mi::RectD r;
        *valid = mi::track_roi_from_landmarks(landmarks, width, height, &r);
        std::memcpy(roi, &r, sizeof(mi_rect));
    });
}

int mi_track_detect_layout(const int* tracked, int streams, int max_detect, int start, int* det_stream, int* n_detect) {
    return guarded([&] {
        require(tracked && det_stream && n_detect, "null argument");
        require(streams >= 1 && streams <= mi::kTrackLayoutMaxStreams, "streams must be 1..2^20");
        require(max_detect >= 1 && max_detect <= streams, "max_detect must be 1..streams");
        require(start >= 0 && start < streams, "start must be 0..streams-1");
        int lost = 0;
        for (int p = 0; p < streams; p++) {
            const int s = mi::track_stream_at(p, start, streams);
            if (tracked[s] != 0) continue;
            const int j = mi::track_detect_slot(lost, max_detect);
            if (j >= 0) det_stream[j] = s;
            lost++;
        }
        mi::track_detect_totals(lost, max_detect, n_detect);
        for (int j = n_detect[0]; j < max_detect; j++) det_stream[j] = -1;
    });
}

int mi_tracker_step(mi_tracker* t, const uint8_t* frames, int width, int height, int stride, int max_detect, mi_detection* faces, int* face_counts,
                    int* source, mi_rect* rois, float* landmarks, int* present, float* eyes, int* det_stream, int* n_detect, int mem, void* stream) {
    return guarded([&] {
        require(t && frames && faces && face_counts && source && rois && landmarks && present && eyes && det_stream && n_detect, "null argument");
        require_frames(t->S, width, height, stride);
        require(max_detect >= 1 && max_detect <= t->S, "max_detect must be 1..streams");
        require_mem(mem);
        mi_pipeline* p = t->pipe;
        PipeCall c(p, stream);
        // (measurement aid: the plan, the selection and the update alone, on what the last full step of this geometry left in the buffers)
        const bool launches_only = t->launches_only;
        require(!launches_only || (t->full_D == max_detect && t->full_w == width && t->full_h == height),
                "track_launches_only: the last full step of this handle must have had this max_detect, width and height");
        mi::Model& fdm = c.fd.m;
        const hipStream_t s = c.s;
        const int S = t->S, D = max_detect;
        const TrackLayout L(S, D);
        TrackOut o{faces, face_counts, source, reinterpret_cast<mi::RectD*>(rois), landmarks, present, eyes, det_stream, n_detect};
        if (mem == MI_MEM_HOST) {
            o = L.in(p->results.as<char>(L.bytes));
            p->out.reserve(L.bytes);
        }
        const uint8_t* d_frames = stage_frames(p->frames, frames, S, width, height, stride, mem, s);
        const int* d_sizes = p->sizes.get(2 * S, width, height, s);
        const PipeTrace tr;
        // ---- 1. the plan: which lost streams get the D detector slots; an unused slot becomes an invalid item of the detector's geometry
        // (whole pictures, no ROI: computed on the host and uploaded once per (D, width, height), as mi_pipeline_run's)
        mi::PreItems it = frame_items(d_frames, S, width, height, stride);
        it.N = D; it.item_frame = o.det_stream;
        it.out_w = p->fd->in_w; it.out_h = p->fd->in_h; it.keep_aspect = 1;
        it.range_min = -1.0; it.range_max = 1.0;
        double* d_pad_det = p->pad_det.as<double>(static_cast<size_t>(4) * D);
        float* d_in_det = p->in_det.as<float>(fdm.input_elems() * D);
        auto* d_geom_det = p->geom_det.as<mi::PreGeom>(D);
        if (t->geom_D != D || t->geom_w != width || t->geom_h != height) {
            t->geom_D = 0;
            mi::upload_whole_image_geom(width, height, it.out_w, it.out_h, true, D, d_geom_det, d_pad_det, s);
            t->geom_D = D; t->geom_w = width; t->geom_h = height;
        }
        mi::TrackPlanArgs pa{};
        pa.tracked = t->state_tracked.as<int>(); pa.S = S; pa.max_detect = D; pa.start = t->start;
        pa.det_stream = o.det_stream; pa.n_detect = o.n_detect; pa.stream_slot = t->stream_slot.as<int>(); pa.geom = d_geom_det;
        mi::launch_track_plan(pa, s);
        tr("track plan");
        // ---- 2. detector on exactly D items (item j reads frame det_stream[j]; a zero tensor for an unused slot) -> decode + NMS + top-1 ROI
        if (!launches_only) {
            mi::launch_pre_tensor(it, d_geom_det, d_in_det, s);
            tr("pre det");
            fdm.run_device(d_in_det, D, s, false);
            tr("det run_device");
        }
        auto* d_dets = p->dets.as<mi_detection>(static_cast<size_t>(kPipeCap) * D);
        int* d_det_counts = t->det_counts.as<int>(D);
        auto* d_det_roi = p->roi_face.as<mi::RectD>(D);
        int* d_det_valid = p->valid_face.as<int>(D);
        const FdPostPipeline top1{d_det_roi, d_det_valid, width, height};
        if (!launches_only) fd_post(p->fd.get(), fdm.output_device(0), fdm.output_device(1), D, d_pad_det, d_dets, kPipeCap, d_det_counts, MI_MEM_DEVICE, s, &top1);
        tr("fd_post");
        // ---- 3. select: the state's ROI, the slot's detection, or nothing
        mi::TrackSelectArgs sa{};
        sa.S = S; sa.cap = kPipeCap; sa.tracked = pa.tracked; sa.state_roi = t->state_roi.as<mi::RectD>(); sa.stream_slot = pa.stream_slot;
        sa.dets = reinterpret_cast<const float*>(d_dets); sa.det_counts = d_det_counts; sa.det_roi = d_det_roi; sa.det_valid = d_det_valid;
        sa.faces = reinterpret_cast<float*>(o.faces); sa.face_counts = o.counts; sa.source = o.source; sa.rois = o.rois;
        sa.valid = t->valid_mesh.as<int>();
        mi::launch_track_select(sa, s);
        tr("track select");
        // ---- 4. mesh and iris on S items: stream i reads frame i
        it.item_frame = nullptr;
        if (!launches_only) pipeline_mesh_iris(p, it, S, o.rois, sa.valid, d_sizes, o.lm, o.present, o.eyes, false, s, tr);
        // ---- 5. the state of the next step
        mi::launch_track_update(o.lm, o.present, S, width, height, t->state_roi.as<mi::RectD>(), t->state_tracked.as<int>(), s);
        tr("track update");
        t->start = mi::track_next_start(t->start, D, S);
        if (!launches_only) { t->full_D = D; t->full_w = width; t->full_h = height; }
        hand_back(p->out.h<char>(0), p->results.as<char>(), L.bytes, mem, s, "D2H results");
        c.fd.finish(mem);
        if (mem == MI_MEM_HOST) {
            const OneShot& h = p->out;
            std::memcpy(faces, h.h<char>(L.faces), sizeof(mi_detection) * S);
            std::memcpy(face_counts, h.h<char>(L.counts), sizeof(int) * S);
            std::memcpy(source, h.h<char>(L.source), sizeof(int) * S);
            std::memcpy(rois, h.h<char>(L.rois), sizeof(mi_rect) * S);
            std::memcpy(landmarks, h.h<char>(L.lm), sizeof(float) * 3 * MI_NUM_FACE_LANDMARKS * S);
            std::memcpy(present, h.h<char>(L.present), sizeof(int) * S);
            std::memcpy(eyes, h.h<char>(L.eyes), sizeof(float) * kEyeFs * 2 * S);
            std::memcpy(det_stream, h.h<char>(L.det_stream), sizeof(int) * D);
            std::memcpy(n_detect, h.h<char>(L.n_detect), sizeof(int) * 2);
            check_letterbox(face_counts, S);
        }
    });
}

int mi_tracker_reset(mi_tracker* t, int stream_index) {
    return guarded([&] {
        require(t, "null argument");
        require(stream_index >= -1 && stream_index < t->S, "stream_index must be -1 (all streams) or 0..streams-1");
        PipeCall c(t->pipe);
        const int first = stream_index < 0 ? 0 : stream_index, n = stream_index < 0 ? t->S : 1;
        mi::hip_check(hipMemsetAsync(t->state_roi.as<mi::RectD>() + first, 0, sizeof(mi::RectD) * n, c.s), "hipMemsetAsync state");
        mi::hip_check(hipMemsetAsync(t->state_tracked.as<int>() + first, 0, sizeof(int) * n, c.s), "hipMemsetAsync state");
        c.fd.sync();
        if (stream_index < 0) t->start = 0;
    });
}

int mi_tracker_get_state(mi_tracker* t, mi_rect* rois, int* tracked) {
    return guarded([&] {
        require(t && rois && tracked, "null argument");
        PipeCall c(t->pipe);
        mi::hip_check(hipMemcpyAsync(rois, t->state_roi.as<mi::RectD>(), sizeof(mi_rect) * t->S, hipMemcpyDeviceToHost, c.s), "D2H state");
        mi::hip_check(hipMemcpyAsync(tracked, t->state_tracked.as<int>(), sizeof(int) * t->S, hipMemcpyDeviceToHost, c.s), "D2H state");
        c.fd.sync();
    });
}

int mi_tracker_set_state(mi_tracker* t, int first, int n, const mi_rect* rois, const int* tracked) {
    return guarded([&] {
        require(t && rois && tracked, "null argument");
        require(first >= 0 && n >= 1 && first < t->S && n <= t->S - first, "first and n must name streams of the handle");
        PipeCall c(t->pipe);
        mi::hip_check(hipMemcpyAsync(t->state_roi.as<mi::RectD>() + first, rois, sizeof(mi_rect) * n, hipMemcpyHostToDevice, c.s), "H2D state");
        mi::hip_check(hipMemcpyAsync(t->state_tracked.as<int>() + first, tracked, sizeof(int) * n, hipMemcpyHostToDevice, c.s), "H2D state");
        c.fd.sync();
    });
}

}  // extern "C"
