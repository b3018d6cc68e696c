// capi_embed.cpp — FaceEmbeddings, similarity and top-k, and the gallery.
#include "capi_internal.hpp"
#include "face_align.hpp"

using namespace mi::capi;

// FaceEmbeddings (face_embeddings.rs:22-26): the caller's network and the scratch of its two entries.
struct mi_fe {
    mi_model model;
    int features = 0;   // D
    DeviceBuf d_in, d_geom, d_valid, d_img, d_frames, d_faces, d_item_frame, d_item_face, d_emb, d_raw;
    DeviceBuf d_gate, d_rois;   // the aligned entries: point_valid / present, the fitted ROIs
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
        create_handle(tflite, nbytes, device, out, fe_finish_create);
    });
}

int mi_fe_create(const char* model_path, int device, mi_fe** out) {
    return guarded([&] {
        require(out, "null argument");
        create_handle(model_path ? model_path : "./models/face_embeddings.tflite", device, out, fe_finish_create);  // face_embeddings.rs:33-37
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
        Call c(h->model);
        mi::Model& m = c.m;
        const hipStream_t s = c.s;
        const int D = h->features;
        // only the crop travels: rows y .. y + h - 1 from column x on; the last row owns 3 * w bytes
        const uint8_t* crop = rgb + static_cast<size_t>(stride) * r[1] + static_cast<size_t>(3) * r[0];
        const size_t crop_bytes = static_cast<size_t>(stride) * (r[3] - 1) + static_cast<size_t>(3) * r[2];
        float* d_in = h->d_in.as<float>(m.input_elems());
        float* d_emb = h->d_emb.as<float>(D);
        const uint8_t* d_crop = stage(h->d_img, crop, crop_bytes, MI_MEM_HOST, s, "H2D crop");
        mi::chip_tensor_enqueue_one(d_crop, r[2], r[3], stride, d_in, s);
        m.run_device(d_in, 1, s);
        mi::launch_l2_norm(m.output_device(0), nullptr, 1, D, d_emb, nullptr, s);
        hand_back(embedding, d_emb, D, MI_MEM_HOST, s, "D2H embedding");
        c.sync();
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
        require_mem(mem);
        static_assert(sizeof(mi_detection) == 17 * sizeof(float), "mi_detection layout");
        Call c(h->model, stream);
        mi::Model& m = c.m;
        const hipStream_t s = c.s;
        const int B = batch, M = max_items, D = h->features;
        const size_t chip_floats = m.input_elems(), n_emb = static_cast<size_t>(D) * M;
        const char* what = "H2D operands";
        mi::ChipItems it{};
        it.frames = stage_frames(h->d_frames, frames, B, width, height, stride, mem, s);
        it.frame_bytes = static_cast<long>(stride) * height; it.batch = B; it.width = width; it.height = height; it.stride = stride;
        it.faces = reinterpret_cast<const float*>(stage(h->d_faces, faces, static_cast<size_t>(B) * max_faces, mem, s, what));
        it.max_faces = max_faces; it.N = M;
        it.item_frame = stage(h->d_item_frame, item_frame, M, mem, s, what);
        it.item_face = stage(h->d_item_face, item_face, M, mem, s, what);
        float* d_emb = result_target(h->d_emb, embeddings, n_emb, mem);
        float* d_raw = raw ? result_target(h->d_raw, raw, n_emb, mem) : nullptr;
        int* d_valid = result_target(h->d_valid, valid, M, mem);
        // the network's input is the handle's own buffer whatever `chips` is: the engine keys its captured graphs by that address
        auto* d_geom = h->d_geom.as<mi::ChipGeom>(M);
        float* d_in = h->d_in.as<float>(chip_floats * M);
        mi::launch_chip_geom(it, d_geom, d_valid, s);
        mi::launch_chip_tensor(it, d_geom, d_in, s);
        m.run_device(d_in, M, s);
        mi::launch_l2_norm(m.output_device(0), d_valid, M, D, d_emb, d_raw, s);
        if (chips) mi::hip_check(hipMemcpyAsync(chips, d_in, chip_floats * sizeof(float) * M, mem == MI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s), "chips copy");
        hand_back(embeddings, d_emb, n_emb, mem, s, "D2H embeddings");
        hand_back(raw, d_raw, n_emb, mem, s, "D2H raw");
        hand_back(valid, d_valid, M, mem, s, "D2H valid");
        c.finish(mem);
    });
}

// ---- aligned chips (face_align.hpp): not the reference's chips; the entries above keep every bit and every launch they have
static int align_template_n(int source) {
    double u[mi::kAlignMaxPoints], v[mi::kAlignMaxPoints];
    const int n = mi::face_align_template(source, u, v);
    require(n > 0, "source must be MI_ALIGN_POINTS, MI_ALIGN_MESH or MI_ALIGN_DETECTION");
    return n;
}

int mi_face_align_template(int source, double xy[5][2], int* n) {
    return guarded([&] {
        require(xy && n, "null argument");
        align_template_n(source);
        double u[mi::kAlignMaxPoints], v[mi::kAlignMaxPoints];
        *n = mi::face_align_template(source, u, v);
        for (int i = 0; i < mi::kAlignMaxPoints; i++) { xy[i][0] = i < *n ? u[i] : 0.0; xy[i][1] = i < *n ? v[i] : 0.0; }
    });
}

int mi_face_align_roi(const float* points_xy, int n, int source, mi_rect* roi, int* valid) {
    return guarded([&] {
        require(points_xy && roi && valid, "null argument");
        require(n == align_template_n(source), "n must be the template's point count (5; 4 for MI_ALIGN_DETECTION)");
        static_assert(sizeof(mi_rect) == sizeof(mi::RectD), "mi_rect layout");
        mi::RectD r;
        *valid = mi::face_align_roi_points(reinterpret_cast<const float(*)[2]>(points_xy), n, source, &r);
        std::memcpy(roi, &r, sizeof r);
    });
}

int mi_face_align_points(int source, const float* landmarks_or_detection, int width, int height, float points_xy[5][2], int* n) {
    return guarded([&] {
        require(landmarks_or_detection && points_xy && n, "null argument");
        require(width > 0 && height > 0, "bad image geometry");
        align_template_n(source);
        *n = mi::face_align_gather(source, landmarks_or_detection, width, height, points_xy);
    });
}

int mi_fe_infer_image_aligned(mi_fe* h, const uint8_t* rgb, int width, int height, int stride, const float* points_xy, int n, int source,
                              float* embedding, int cap, mi_rect* roi) {
    return guarded([&] {
        require(h && rgb && points_xy && embedding, "null argument");
        require(width > 0 && height > 0 && stride >= 3 * static_cast<long>(width), "bad image geometry");
        require(n == align_template_n(source), "n must be the template's point count (5; 4 for MI_ALIGN_DETECTION)");
        require(cap >= h->features, "output capacity is smaller than the model's feature count");
        mi::RectD r;
        const int ok = mi::face_align_roi_points(reinterpret_cast<const float(*)[2]>(points_xy), n, source, &r);
        if (roi) std::memcpy(roi, &r, sizeof r);
        if (!ok) throw ApiError(MI_ERANGE, "the points have no similarity fit (a coordinate is not finite, or all points are equal)");
        Call c(h->model);
        mi::Model& m = c.m;
        const hipStream_t s = c.s;
        const int D = h->features;
        // the WHOLE picture travels: a crop with a shifted ROI would round the ROI's corners to other floats; the last row owns 3 * width bytes
        const size_t bytes = static_cast<size_t>(stride) * (height - 1) + static_cast<size_t>(3) * width;
        float* d_in = h->d_in.as<float>(m.input_elems());
        float* d_emb = h->d_emb.as<float>(D);
        const uint8_t* d_img = stage(h->d_img, rgb, bytes, MI_MEM_HOST, s, "H2D image");
        mi::aligned_chip_enqueue_one(d_img, width, height, stride, r, d_in, s);
        m.run_device(d_in, 1, s);
        mi::launch_l2_norm(m.output_device(0), nullptr, 1, D, d_emb, nullptr, s);
        hand_back(embedding, d_emb, D, MI_MEM_HOST, s, "D2H embedding");
        c.sync();
    });
}

int mi_fe_infer_aligned_items(mi_fe* h, const uint8_t* frames, int batch, int width, int height, int stride, int source, const void* src,
                              const int* gate, int max_faces, const int* item_frame, const int* item_face, int max_items, float* embeddings,
                              int* valid, float* raw, float* chips, mi_rect* rois, int mem, void* stream) {
    return guarded([&] {
        // (a budget the launches cannot take is refused here, before anything is queued)
        align_template_n(source);
        const bool det = source == MI_ALIGN_DETECTION;
        require_face_items(batch, det ? max_faces : 1, max_items, mi::kFaceItemsMaxRunItems, "max_items must be 1..32767 (one grid row of a launch per item)");
        require(h && frames && src && item_frame && embeddings && valid, "null argument");
        require(!det || item_face, "MI_ALIGN_DETECTION needs item_face");
        require(source != MI_ALIGN_MESH || gate, "MI_ALIGN_MESH needs `present` as its gate");
        require(width > 0 && height > 0 && stride >= 3 * static_cast<long>(width), "bad frame geometry");
        require_mem(mem);
        static_assert(sizeof(mi_detection) == 17 * sizeof(float), "mi_detection layout");
        static_assert(sizeof(mi_rect) == sizeof(mi::RectD), "mi_rect layout");
        Call c(h->model, stream);
        mi::Model& m = c.m;
        const hipStream_t s = c.s;
        const int B = batch, M = max_items, D = h->features;
        const size_t chip_floats = m.input_elems(), n_emb = static_cast<size_t>(D) * M;
        const char* what = "H2D operands";
        const size_t src_floats = source == MI_ALIGN_POINTS ? static_cast<size_t>(M) * 2 * mi::kAlignMaxPoints
                                  : source == MI_ALIGN_MESH ? static_cast<size_t>(M) * 3 * mi::kAlignMeshLandmarks
                                                            : static_cast<size_t>(B) * max_faces * 17;
        mi::AlignItems it{};
        it.frames = stage_frames(h->d_frames, frames, B, width, height, stride, mem, s);
        it.frame_bytes = static_cast<long>(stride) * height; it.batch = B; it.width = width; it.height = height; it.stride = stride;
        it.source = source;
        it.src = stage(h->d_faces, static_cast<const float*>(src), src_floats, mem, s, what);
        it.gate = det ? nullptr : stage(h->d_gate, gate, M, mem, s, what);
        it.max_faces = det ? max_faces : 0; it.N = M;
        it.item_frame = stage(h->d_item_frame, item_frame, M, mem, s, what);
        it.item_face = det ? stage(h->d_item_face, item_face, M, mem, s, what) : nullptr;
        float* d_emb = result_target(h->d_emb, embeddings, n_emb, mem);
        float* d_raw = raw ? result_target(h->d_raw, raw, n_emb, mem) : nullptr;
        int* d_valid = result_target(h->d_valid, valid, M, mem);
        auto* d_rois = rois ? reinterpret_cast<mi::RectD*>(result_target(h->d_rois, rois, M, mem)) : nullptr;
        // the network's input is the handle's own buffer whatever `chips` is: the engine keys its captured graphs by that address
        auto* d_geom = h->d_geom.as<mi::PreGeom>(M);
        float* d_in = h->d_in.as<float>(chip_floats * M);
        mi::launch_align_geom(it, d_geom, d_rois, d_valid, s);
        mi::launch_aligned_chips(it, d_geom, d_in, s);
        m.run_device(d_in, M, s);
        mi::launch_l2_norm(m.output_device(0), d_valid, M, D, d_emb, d_raw, s);
        if (chips) mi::hip_check(hipMemcpyAsync(chips, d_in, chip_floats * sizeof(float) * M, mem == MI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s), "chips copy");
        hand_back(embeddings, d_emb, n_emb, mem, s, "D2H embeddings");
        hand_back(raw, d_raw, n_emb, mem, s, "D2H raw");
        hand_back(valid, d_valid, M, mem, s, "D2H valid");
        hand_back(rois, reinterpret_cast<const mi_rect*>(d_rois), M, mem, s, "D2H rois");
        c.finish(mem);
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
        require_mem(mem);
        select_device(device, "no such HIP device (the similarity matrix runs on the GPU; no CPU fallback exists)");
        hipStream_t s = static_cast<hipStream_t>(stream);
        DeviceBuf b_a, b_b, b_out;
        const size_t out_elems = static_cast<size_t>(n) * m;
        const float* d_a = stage(b_a, a, static_cast<size_t>(n) * features, mem, s, "H2D a");
        const float* d_b = stage(b_b, b, static_cast<size_t>(m) * features, mem, s, "H2D b");
        float* d_out = result_target(b_out, out, out_elems, mem);
        mi::launch_similarity(d_a, n, d_b, m, features, d_out, s);
        hand_back(out, d_out, out_elems, mem, s, "D2H similarity");
        finish(mem, stream != nullptr, s);
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
        require_mem(mem);
        select_device(device, "no such HIP device (a gallery lives on the GPU; no CPU fallback exists)");
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
        require_mem(mem);
        mi::hip_check(hipSetDevice(g->device), "hipSetDevice");
        hipStream_t s = static_cast<hipStream_t>(stream);
        Use use(g->sync, s);
        const int tiles_m = (g->m + 127) / 128;
        const int splits = g->splits ? (g->splits < tiles_m ? g->splits : tiles_m) : mi::gallery_auto_splits(n, g->m, mi::device_cu_count());
        const size_t N = static_cast<size_t>(n), out_elems = N * k;
        // (growing frees the old block, which waits for the calls that still use it)
        auto* d_part = g->d_part.as<mi::TopkPair>(out_elems * splits);
        int* d_index = result_target(g->d_index, index, out_elems, mem);
        float* d_score = result_target(g->d_score, score, out_elems, mem);
        int* d_label = label ? result_target(g->d_label, label, out_elems, mem) : nullptr;
        const float* d_q = stage(g->d_queries, queries, N * g->features, mem, s, "H2D queries");
        mi::launch_gallery_topk(d_q, n, g->d_rows.as<const float>(), g->m, g->features, k, splits, g->has_labels ? g->d_labels.as<const int>() : nullptr,
                                d_part, d_index, d_score, d_label, s);
        hand_back(index, d_index, out_elems, mem, s, "D2H index");
        hand_back(score, d_score, out_elems, mem, s, "D2H score");
        hand_back(label, d_label, out_elems, mem, s, "D2H label");
        finish(mem, stream != nullptr, s);
    });
}

}  // extern "C"
