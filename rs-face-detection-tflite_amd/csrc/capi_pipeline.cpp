// capi_pipeline.cpp — the batched pipeline: detector, face mesh and iris network of a pass in one call.
#include "capi_pipeline.hpp"

namespace mi {
namespace capi {
void require_face_items(int batch, int max_faces, int max_items, int items_limit, const char* items_msg) {
    require(batch > 0 && batch <= mi::kFaceItemsMaxBatch, "batch must be 1..2^26");
    require(max_faces >= 1 && max_faces <= mi::kFaceItemsMaxFaces, "max_faces must be 1..16");
    require(max_items >= 1 && max_items <= items_limit, items_msg);
}
}  // namespace capi
}  // namespace mi

using namespace mi::capi;

using PipeJpegSlot = mi_pipeline::PipeJpegSlot;

// the three handles of a pipeline through their own create entries (`make_*(&handle)` returns that entry's status), in the fixed fd, fl, iris order
template <class MakeFd, class MakeFl, class MakeIris>
static void pipeline_create(mi_pipeline** out, MakeFd make_fd, MakeFl make_fl, MakeIris make_iris) {
    auto p = std::make_unique<mi_pipeline>();
    mi_fd* fd = nullptr;
    mi_fl* fl = nullptr;
    mi_iris* ir = nullptr;
    if (int rc = make_fd(&fd)) throw ApiError(rc, last_error());
    p->fd.reset(fd);
    if (int rc = make_fl(&fl)) throw ApiError(rc, last_error());
    p->fl.reset(fl);
    if (int rc = make_iris(&ir)) throw ApiError(rc, last_error());
    p->iris.reset(ir);
    *out = p.release();
}

extern "C" {

// ------------------------------------------------------------------------------------------------ batched pipeline
int mi_pipeline_create(int fd_kind, const char* model_dir, int device, mi_pipeline** out) {
    return guarded([&] {
        require(out, "null argument");
        const std::string dir = model_dir ? model_dir : "./models";
        pipeline_create(
            out, [&](mi_fd** h) { return mi_fd_create(fd_kind, dir.c_str(), device, h); },
            [&](mi_fl** h) { return mi_fl_create((dir + "/face_landmark.tflite").c_str(), device, h); },
            [&](mi_iris** h) { return mi_iris_create((dir + "/iris_landmark.tflite").c_str(), device, h); });
    });
}

int mi_pipeline_create_from_bytes(int fd_kind, const uint8_t* fd_tflite, size_t fd_nbytes, const uint8_t* fl_tflite, size_t fl_nbytes,
                                  const uint8_t* iris_tflite, size_t iris_nbytes, int device, mi_pipeline** out) {
    return guarded([&] {
        require(out && fd_tflite && fl_tflite && iris_tflite && fd_nbytes && fl_nbytes && iris_nbytes, "null argument");
        pipeline_create(
            out, [&](mi_fd** h) { return mi_fd_create_from_bytes(fd_kind, fd_tflite, fd_nbytes, device, h); },
            [&](mi_fl** h) { return mi_fl_create_from_bytes(fl_tflite, fl_nbytes, device, h); },
            [&](mi_iris** h) { return mi_iris_create_from_bytes(iris_tflite, iris_nbytes, device, h); });
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

// The detector's stage of a pass over B frames in device memory: image_to_tensor(frame, None, (w,h), keep_aspect = true, (-1,1)) -> net.  Sets up
// `it` (the frames; the later stages change the item fields) and returns the letterbox paddings [B][4] the post-processing launch needs.
static double* pipeline_detect(mi_pipeline* p, mi::PreItems& it, const uint8_t* d_frames, int B, int width, int height, int stride, bool one_shot, hipStream_t s,
                               const PipeTrace& tr) {
    mi::Model& fdm = *p->fd->model.m;
    it = frame_items(d_frames, B, width, height, stride);
    it.out_w = p->fd->in_w; it.out_h = p->fd->in_h; it.keep_aspect = 1;
    it.range_min = -1.0; it.range_max = 1.0;
    double* d_pad_det = p->pad_det.as<double>(static_cast<size_t>(4) * B);
    float* d_in_det = p->in_det.as<float>(fdm.input_elems() * B);
    // (no ROI: the geometry is the same for every call on pictures of this size — no pre_geom launch, 9 us of a one-picture call)
    auto* d_geom_det = p->geom_det.as<mi::PreGeom>(B);
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

// The mesh and iris stages of a pass (capi_pipeline.hpp)
extern "C++" void mi::capi::pipeline_mesh_iris(mi_pipeline* p, mi::PreItems& it, int N, const mi::RectD* d_roi_face, const int* d_valid_face, const int* d_sizes, float* lm,
                                  int* present, float* eyes, bool one_shot, hipStream_t s, const PipeTrace& tr) {
    mi::Model& flm = *p->fl->model.m;
    mi::Model& irm = *p->iris->model.m;
    const int width = it.width, height = it.height;
    p->geom.as<mi::PreGeom>(static_cast<size_t>(2) * N);   // (both stages' geometry: sized for the eyes at once)
    // ---- 2. face -> face_detection_to_roi -> image_to_tensor(frame, roi, (192,192), false, (0,1)) -> mesh net
    it.rois = d_roi_face; it.roi_valid = d_valid_face; it.items_per_frame = 1; it.N = N; it.out_w = p->fl->in_w; it.out_h = p->fl->in_h; it.keep_aspect = 0;
    it.range_min = 0.0; it.range_max = 1.0;
    const float* d_in_lm = items_to_tensor(it, flm, p->geom, p->in_lm, nullptr, s);
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
    auto* d_roi_eye = p->roi_eye.as<mi::RectD>(static_cast<size_t>(2) * N);
    int* d_valid_eye = p->valid_eye.as<int>(static_cast<size_t>(2) * N);
    int* d_flip_eye = p->flip_eye.as<int>(static_cast<size_t>(2) * N);
    mi::launch_iris_rois(lm, present, N, width, height, d_roi_eye, d_valid_eye, d_flip_eye, s);
    it.rois = d_roi_eye; it.roi_valid = d_valid_eye; it.flip = d_flip_eye; it.items_per_frame = 2; it.N = 2 * N;
    it.out_w = p->iris->in_w; it.out_h = p->iris->in_h; it.keep_aspect = 1;
    double* d_pad_eye = p->pad_eye.as<double>(static_cast<size_t>(8) * N);
    const float* d_in_eye = items_to_tensor(it, irm, p->geom, p->in_eye, d_pad_eye, s);
    tr("pre iris");
    irm.run_device(d_in_eye, 2 * N, s, one_shot);
    tr("iris run_device");
    // contour and iris landmarks of both eyes in one launch, the two lists of an eye side by side: kEyeFs floats from eye to eye
    iris_project(p->iris.get(), 2 * N, d_roi_eye, d_sizes, d_pad_eye, d_flip_eye, eyes, eyes + 3 * MI_NUM_EYE_LANDMARKS, s, d_valid_eye, kEyeFs);
    tr("projections");
}

// One pass of the flow of lib.rs:24-40 over B frames that are in device memory: everything is queued on `s`, nothing is waited for (but the
// upload of the per-item image sizes when the batch geometry changes).  The caller holds the three handles (Use) and, for one_shot, the CUs.
static void pipeline_enqueue(mi_pipeline* p, const uint8_t* d_frames, int B, int width, int height, int stride, const PipeOut& o, bool one_shot, hipStream_t s) {
    mi::Model& fdm = *p->fd->model.m;
    const int cap = kPipeCap;
    const int* d_sizes = p->sizes.get(2 * B, width, height, s);
    const PipeTrace tr;
    // ---- 1. detector -> decode + NMS
    mi::PreItems it{};
    double* d_pad_det = pipeline_detect(p, it, d_frames, B, width, height, stride, one_shot, s, tr);
    auto* d_dets = p->dets.as<mi_detection>(static_cast<size_t>(cap) * B);
    // ---- 2. faces[0] -> face_detection_to_roi -> mesh, 3. both eyes -> iris
    // (the post-processing launch writes zeros behind a frame's last detection — frames without a face report zeros — and faces[0]'s ROI)
    auto* d_roi_face = p->roi_face.as<mi::RectD>(B);
    int* d_valid_face = p->valid_face.as<int>(B);
    const FdPostPipeline top1{d_roi_face, d_valid_face, width, height};
    fd_post(p->fd.get(), fdm.output_device(0), fdm.output_device(1), B, d_pad_det, d_dets, cap, o.counts,
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
        require_frames(batch, width, height, stride);
        require_mem(mem);
        PipeCall c(p, stream);
        mi::Model& fdm = c.fd.m;
        const hipStream_t s = c.s;
        const int B = batch;
        const PipeLayout L(B);
        char* d_results = nullptr;
        if (mem == MI_MEM_HOST) {
            d_results = p->results.as<char>(L.bytes);
            p->out.reserve(L.bytes);
        }
        const uint8_t* d_frames = stage_frames(p->frames, frames, B, width, height, stride, mem, s);
        // A picture or two from host memory (lib.rs:24-40 on one image): the detector and the face mesh may take their single-launch plans —
        // this call holds the CUs until its synchronisation below, and repeats itself on the batched plan should such a launch have given up.
        std::unique_ptr<BandClaim> claim;
        if (mem == MI_MEM_HOST) claim = std::make_unique<BandClaim>(fdm.device(), pipeline_band_workgroups(p, B));
        const PipeOut o = mem == MI_MEM_DEVICE ? PipeOut{faces, face_counts, landmarks, present, eyes} : L.in(d_results);
        auto network = [&](bool one_shot) {
            pipeline_enqueue(p, d_frames, B, width, height, stride, o, one_shot, s);
            hand_back(p->out.h<char>(0), d_results, L.bytes, mem, s, "D2H results");
            c.fd.finish(mem);
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
        require_frames(batch, width, height, stride);   // (batch: checked above)
        require_mem(mem);
        PipeCall c(p, stream);
        mi::Model& fdm = c.fd.m;
        const hipStream_t s = c.s;
        const int B = batch, M = max_items;
        const FacesLayout L(B, max_faces, M);
        FacesOut o{faces, face_counts, item_frame, item_face, n_items, landmarks, present, eyes};
        if (mem == MI_MEM_HOST) {
            o = L.in(p->results.as<char>(L.bytes));
            p->out.reserve(L.bytes);
        }
        const uint8_t* d_frames = stage_frames(p->frames, frames, B, width, height, stride, mem, s);
        const int* d_sizes = p->sizes_item.get(2 * M, width, height, s);
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
        fa.rois = p->roi_item.as<mi::RectD>(M);
        fa.valid = p->valid_item.as<int>(M);
        mi::launch_face_items(fa, s);
        tr("face items");
        // ---- 2. every item's face -> mesh, 3. both eyes -> iris: item i reads frame item_frame[i]
        it.item_frame = o.item_frame;
        pipeline_mesh_iris(p, it, M, fa.rois, fa.valid, d_sizes, o.lm, o.present, o.eyes, false, s, tr);
        hand_back(p->out.h<char>(0), p->results.as<char>(), L.bytes, mem, s, "D2H results");
        c.fd.finish(mem);
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
    char* d_results = sl.results.as<char>(L.bytes);
    const JpegSlot& js = sl.jpeg;
    pipeline_enqueue(p, js.d_rgb.as<uint8_t>(), 1, js.f.width, js.f.height, 3 * js.f.width, L.in(d_results), one_shot, s);
    mi::hip_check(hipMemcpyAsync(sl.out.host, d_results, L.bytes, hipMemcpyDeviceToHost, s), "D2H results");
}

int mi_pipeline_submit_jpeg(mi_pipeline* p, int slot, const uint8_t* bytes, size_t nbytes) {
    return guarded([&] {
        require(p && bytes, "null argument");
        require_slot(slot);
        PipeJpegSlot& sl = p->jslot[slot];
        JpegSlot& js = sl.jpeg;
        if (js.pending) throw ApiError(MI_EINVAL, "slot holds a picture that has not been collected");
        mi::Model& fdm = *p->fd->model.m;
        mi::hip_check(hipSetDevice(fdm.device()), "hipSetDevice");   // (no PipeCall yet: the decoder runs without holding the handles)
        jpeg_stage(js, bytes, nbytes);
        sl.out.reserve(PipeLayout(1).bytes);
        PipeCall c(p);
        const hipStream_t s = c.s;
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
        require_slot(slot);
        PipeJpegSlot& sl = p->jslot[slot];
        JpegSlot& js = sl.jpeg;
        if (!js.pending) throw ApiError(MI_EINVAL, "nothing was submitted to this slot");
        mi::Model& fdm = *p->fd->model.m;
        mi::hip_check(hipSetDevice(fdm.device()), "hipSetDevice");
        mi::hip_check(hipEventSynchronize(js.done), "hipEventSynchronize");
        {
            PipeCall c(p);
            const hipStream_t s = c.s;
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

}  // extern "C"
