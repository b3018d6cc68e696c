//! Raw declarations of `include/mi_face.h` (the drop-in boundary).  One `extern "C"` item per C entry point the three
//! `infer` paths and their helpers use; layouts are `#[repr(C)]` mirrors of `mi_detection`, `mi_rect`, `mi_landmark`.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_double, c_float, c_int, c_long, c_void};

pub const MI_OK: c_int = 0;
pub const MI_MEM_HOST: c_int = 0;
pub const MI_MEM_DEVICE: c_int = 1;
pub const MI_ALIGN_POINTS: c_int = 0;
pub const MI_ALIGN_MESH: c_int = 1;
pub const MI_ALIGN_DETECTION: c_int = 2;
pub const MI_NUM_FACE_LANDMARKS: usize = 468;
pub const MI_NUM_EYE_LANDMARKS: usize = 71;
pub const MI_NUM_IRIS_LANDMARKS: usize = 5;

/// `Detection { data: Array2<f32>[8,2], score: f32 }` — types.rs:189-193
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mi_detection {
    pub data: [c_float; 16],
    pub score: c_float,
}

/// `Rect` — types.rs:24-36
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mi_rect {
    pub x_center: c_double,
    pub y_center: c_double,
    pub width: c_double,
    pub height: c_double,
    pub rotation: c_double,
    pub normalized: c_int,
}

/// `Landmark { x, y, z: f64 }` — types.rs:176-187
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct mi_landmark {
    pub x: c_double,
    pub y: c_double,
    pub z: c_double,
}

/// `Color` as the bytes `render_to_image` writes — render.rs:6-26,431
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct mi_color {
    pub r: u8,
    pub g: u8,
    pub b: u8,
    pub a: u8,
}

pub const MI_ANN_POINTS: c_int = 0;
pub const MI_ANN_LINES: c_int = 1;
pub const MI_ANN_RECTS: c_int = 2;
pub const MI_ANN_FILLED_RECTS: c_int = 3;

/// `Annotation` — render.rs:207-213: `count` items whose doubles start at index `first` of a frame's coordinate block
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mi_annotation {
    pub kind: c_int,
    pub first: c_int,
    pub count: c_int,
    pub thickness: c_double,
    pub color: mi_color,
    pub normalized: c_int,
}

/// arguments of `detections_to_render_data` / `face_landmarks_to_render_data` / `eye_landmarks_to_render_data`
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mi_render_style {
    pub draw_bounds: c_int,
    pub bounds_color: mi_color,
    pub line_width: c_int,
    pub draw_keypoints: c_int,
    pub keypoint_color: mi_color,
    pub point_width: c_int,
    pub draw_mesh: c_int,
    pub mesh_landmark_color: mi_color,
    pub mesh_connection_color: mi_color,
    pub mesh_thickness: c_float,
    pub draw_eyes: c_int,
    pub eye_landmark_color: mi_color,
    pub eye_connection_color: mi_color,
    pub eye_thickness: c_float,
}

/// `mi_render_style` plus the arguments of `iris_landmarks_to_render_data` — iris_landmark.rs:330-335
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mi_render_items_style {
    pub base: mi_render_style,
    pub draw_iris_oval: c_int,
    pub iris_oval_color: mi_color,
    pub draw_iris_points: c_int,
    pub iris_landmark_color: mi_color,
    pub iris_thickness: c_double,
}

#[repr(C)] pub struct mi_fd { _private: [u8; 0] }
#[repr(C)] pub struct mi_fl { _private: [u8; 0] }
#[repr(C)] pub struct mi_iris { _private: [u8; 0] }
#[repr(C)] pub struct mi_pipeline { _private: [u8; 0] }
#[repr(C)] pub struct mi_tracker { _private: [u8; 0] }
#[repr(C)] pub struct mi_fe { _private: [u8; 0] }
#[repr(C)] pub struct mi_gallery { _private: [u8; 0] }
#[repr(C)] pub struct mi_model { _private: [u8; 0] }

extern "C" {
    pub fn mi_last_error() -> *const c_char;
    pub fn mi_device_count() -> c_int;

    // FaceDetection — face_detection.rs:146-267
    pub fn mi_fd_create(kind: c_int, model_dir: *const c_char, device: c_int, out: *mut *mut mi_fd) -> c_int;
    pub fn mi_fd_create_from_bytes(kind: c_int, tflite: *const u8, nbytes: usize, device: c_int, out: *mut *mut mi_fd) -> c_int;
    pub fn mi_fd_free(h: *mut mi_fd);
    pub fn mi_fd_input_size(h: *const mi_fd, width: *mut c_int, height: *mut c_int) -> c_int;
    pub fn mi_fd_infer_image(h: *mut mi_fd, rgb: *const u8, width: c_int, height: c_int, stride: c_int, roi: *const mi_rect,
                             out: *mut mi_detection, cap: c_int, count: *mut c_int) -> c_int;
    pub fn mi_fd_infer_tensor(h: *mut mi_fd, input: *const c_float, batch: c_int, padding: *const c_double, out: *mut mi_detection,
                              cap_per_frame: c_int, counts: *mut c_int, mem: c_int, stream: *mut c_void) -> c_int;
    pub fn mi_fd_infer_images(h: *mut mi_fd, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int,
                              rois: *const mi_rect, out: *mut mi_detection, cap_per_frame: c_int, counts: *mut c_int, mem: c_int,
                              stream: *mut c_void) -> c_int;
    pub fn mi_fd_submit_images(h: *mut mi_fd, slot: c_int, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int,
                               cap_per_frame: c_int) -> c_int;
    pub fn mi_fd_collect(h: *mut mi_fd, slot: c_int, out: *mut mi_detection, counts: *mut c_int) -> c_int;
    pub fn mi_fd_submit_jpeg(h: *mut mi_fd, slot: c_int, bytes: *const u8, nbytes: usize, cap: c_int) -> c_int;
    pub fn mi_fd_collect_jpeg(h: *mut mi_fd, slot: c_int, out: *mut mi_detection, cap: c_int, count: *mut c_int, width: *mut c_int,
                              height: *mut c_int) -> c_int;
    pub fn mi_host_alloc(bytes: usize, out: *mut *mut c_void) -> c_int;
    pub fn mi_host_free(p: *mut c_void);

    // FaceLandmark — face_landmark.rs:200-306
    pub fn mi_fl_create(model_path: *const c_char, device: c_int, out: *mut *mut mi_fl) -> c_int;
    pub fn mi_fl_free(h: *mut mi_fl);
    pub fn mi_fl_infer_image(h: *mut mi_fl, rgb: *const u8, width: c_int, height: c_int, stride: c_int, roi: *const mi_rect,
                             out: *mut mi_landmark, cap: c_int, count: *mut c_int) -> c_int;
    pub fn mi_fl_infer_tensor(h: *mut mi_fl, input: *const c_float, batch: c_int, rois: *const mi_rect, image_sizes: *const c_int,
                              landmarks: *mut c_float, present: *mut c_int, raw_flags: *mut c_float, mem: c_int, stream: *mut c_void) -> c_int;
    pub fn mi_fl_infer_images(h: *mut mi_fl, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int, rois: *const mi_rect,
                              items_per_frame: c_int, landmarks: *mut c_float, present: *mut c_int, raw_flags: *mut c_float, mem: c_int,
                              stream: *mut c_void) -> c_int;

    pub fn mi_fl_submit_images(h: *mut mi_fl, slot: c_int, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int,
                               rois: *const mi_rect, items_per_frame: c_int) -> c_int;
    pub fn mi_fl_collect(h: *mut mi_fl, slot: c_int, landmarks: *mut c_float, present: *mut c_int, raw_flags: *mut c_float) -> c_int;

    // IrisLandmark — iris_landmark.rs:130-248
    pub fn mi_iris_create(model_path: *const c_char, device: c_int, out: *mut *mut mi_iris) -> c_int;
    pub fn mi_iris_free(h: *mut mi_iris);
    pub fn mi_iris_infer_image(h: *mut mi_iris, rgb: *const u8, width: c_int, height: c_int, stride: c_int, roi: *const mi_rect,
                               is_right_eye: c_int, contour71: *mut mi_landmark, iris5: *mut mi_landmark) -> c_int;
    pub fn mi_iris_infer_images(h: *mut mi_iris, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int, rois: *const mi_rect,
                                is_right_eye: *const c_int, items_per_frame: c_int, contour: *mut c_float, iris: *mut c_float, mem: c_int,
                                stream: *mut c_void) -> c_int;

    // helpers the reference exports next to the three structs
    pub fn mi_face_detection_to_roi(det: *const mi_detection, image_w: c_int, image_h: c_int, out: *mut mi_rect) -> c_int;
    pub fn mi_iris_roi_from_face_landmarks(landmarks468: *const mi_landmark, image_w: c_int, image_h: c_int, left_eye: *mut mi_rect,
                                           right_eye: *mut mi_rect) -> c_int;
    pub fn mi_update_face_landmarks_with_iris_results(face468: *const mi_landmark, left71: *const mi_landmark, right71: *const mi_landmark,
                                                      out468: *mut mi_landmark) -> c_int;
    pub fn mi_bbox_to_roi(bbox: *const c_double, image_w: c_int, image_h: c_int, rotation_keypoints: *const c_double, scale_x: c_double,
                          scale_y: c_double, size_mode: c_int, out: *mut mi_rect) -> c_int;
    pub fn mi_bbox_from_landmarks(landmarks: *const mi_landmark, count: c_int, bbox_out: *mut c_double) -> c_int;
    pub fn mi_jpeg_info(bytes: *const u8, nbytes: usize, width: *mut c_int, height: *mut c_int) -> c_int;
    pub fn mi_jpeg_decode_rgb(device: c_int, bytes: *const u8, nbytes: usize, rgb: *mut u8, cap_bytes: usize, width: *mut c_int,
                              height: *mut c_int, mem: c_int, stream: *mut c_void) -> c_int;

    // multi-GPU: the frozen .tflite bytes from `root` to every rank over RCCL (one process per GPU)
    pub fn mi_dist_broadcast_bytes(id_path: *const c_char, rank: c_int, world: c_int, root: c_int, device: c_int, buf: *mut u8, nbytes: usize,
                                   timeout_ms: c_int) -> c_int;

    // two batches in flight: n hipStream_t's tested to sit on distinct hardware queues
    pub fn mi_streams_create_distinct(device: c_int, n: c_int, streams: *mut *mut c_void) -> c_int;
    pub fn mi_streams_destroy(device: c_int, n: c_int, streams: *mut *mut c_void) -> c_int;

    // batched detector -> mesh -> iris flow on the device (no counterpart in the reference: lib.rs:24-40 per frame)
    pub fn mi_pipeline_create(fd_kind: c_int, model_dir: *const c_char, device: c_int, out: *mut *mut mi_pipeline) -> c_int;
    pub fn mi_pipeline_free(p: *mut mi_pipeline);
    pub fn mi_pipeline_run(p: *mut mi_pipeline, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int,
                           faces: *mut mi_detection, face_counts: *mut c_int, landmarks: *mut c_float, present: *mut c_int,
                           eyes: *mut c_float, mem: c_int, stream: *mut c_void) -> c_int;
    // ... for the first max_faces faces of every frame, compacted into max_items items (include/mi_face.h)
    pub fn mi_pipeline_run_faces(p: *mut mi_pipeline, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int,
                                 max_faces: c_int, max_items: c_int, faces: *mut mi_detection, face_counts: *mut c_int,
                                 item_frame: *mut c_int, item_face: *mut c_int, n_items: *mut c_int, landmarks: *mut c_float,
                                 present: *mut c_int, eyes: *mut c_float, mem: c_int, stream: *mut c_void) -> c_int;
    pub fn mi_face_items_layout(face_counts: *const c_int, batch: c_int, max_faces: c_int, max_items: c_int, item_frame: *mut c_int,
                                item_face: *mut c_int, n_items: *mut c_int) -> c_int;

    // landmark-to-ROI face tracking for video streams (NOT the reference's behaviour: MediaPipe's video loop; include/mi_face.h)
    pub fn mi_track_roi_from_landmarks(landmarks: *const c_float, width: c_int, height: c_int, roi: *mut mi_rect, valid: *mut c_int) -> c_int;
    pub fn mi_track_detect_layout(tracked: *const c_int, streams: c_int, max_detect: c_int, start: c_int, det_stream: *mut c_int,
                                  n_detect: *mut c_int) -> c_int;
    pub fn mi_tracker_create(fd_kind: c_int, model_dir: *const c_char, device: c_int, streams: c_int, out: *mut *mut mi_tracker) -> c_int;
    pub fn mi_tracker_free(t: *mut mi_tracker);
    pub fn mi_tracker_set_option(t: *mut mi_tracker, key: *const c_char, value: c_int) -> c_int;
    pub fn mi_tracker_step(t: *mut mi_tracker, frames: *const u8, width: c_int, height: c_int, stride: c_int, max_detect: c_int,
                           faces: *mut mi_detection, face_counts: *mut c_int, source: *mut c_int, rois: *mut mi_rect, landmarks: *mut c_float,
                           present: *mut c_int, eyes: *mut c_float, det_stream: *mut c_int, n_detect: *mut c_int, mem: c_int,
                           stream: *mut c_void) -> c_int;
    pub fn mi_tracker_reset(t: *mut mi_tracker, stream_index: c_int) -> c_int;
    pub fn mi_tracker_get_state(t: *mut mi_tracker, rois: *mut mi_rect, tracked: *mut c_int) -> c_int;
    pub fn mi_tracker_set_state(t: *mut mi_tracker, first: c_int, n: c_int, rois: *const mi_rect, tracked: *const c_int) -> c_int;

    // render.rs:262-479 on the device
    pub fn mi_render_annotations(device: c_int, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int,
                                 anns: *const mi_annotation, n_anns: c_int, coords: *const c_double, coords_per_frame: c_long, out: *mut u8,
                                 out_channels: c_int, out_stride: c_int, skipped: *mut c_int, mem: c_int, stream: *mut c_void) -> c_int;
    pub fn mi_render_faces(device: c_int, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int,
                           faces: *const mi_detection, face_counts: *const c_int, faces_per_frame: c_int, landmarks: *const c_float,
                           present: *const c_int, eyes: *const c_float, style: *const mi_render_style, out: *mut u8, out_channels: c_int,
                           out_stride: c_int, skipped: *mut c_int, mem: c_int, stream: *mut c_void) -> c_int;
    // ... for the item list of mi_pipeline_run_faces: every face of a frame, with both irises (iris_landmark.rs:330-377)
    pub fn mi_render_face_items(device: c_int, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int,
                                faces: *const mi_detection, face_counts: *const c_int, max_faces: c_int, item_frame: *const c_int,
                                n_items: *const c_int, max_items: c_int, landmarks: *const c_float, present: *const c_int,
                                eyes: *const c_float, style: *const mi_render_items_style, out: *mut u8, out_channels: c_int,
                                out_stride: c_int, skipped: *mut c_int, mem: c_int, stream: *mut c_void) -> c_int;

    // FaceEmbeddings — face_embeddings.rs:22-109, with l2_norm / similarity_score (utils.rs:30-50); the model is the caller's
    pub fn mi_fe_create(model_path: *const c_char, device: c_int, out: *mut *mut mi_fe) -> c_int;
    pub fn mi_fe_create_from_bytes(tflite: *const u8, nbytes: usize, device: c_int, out: *mut *mut mi_fe) -> c_int;
    pub fn mi_fe_free(h: *mut mi_fe);
    pub fn mi_fe_features(h: *const mi_fe, features: *mut c_int) -> c_int;
    pub fn mi_fe_model(h: *mut mi_fe) -> *mut mi_model;
    pub fn mi_model_set_option(m: *mut mi_model, key: *const c_char, value: c_int) -> c_int;
    pub fn mi_model_get_option(m: *mut mi_model, key: *const c_char, value: *mut c_int) -> c_int;
    pub fn mi_face_chip_rect(det: *const mi_detection, width: c_int, height: c_int, rect: *mut c_int, valid: *mut c_int) -> c_int;
    pub fn mi_fe_infer_image(h: *mut mi_fe, rgb: *const u8, width: c_int, height: c_int, stride: c_int, bbox: *const c_double,
                             embedding: *mut c_float, cap: c_int) -> c_int;
    pub fn mi_fe_infer_face_items(h: *mut mi_fe, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int,
                                  faces: *const mi_detection, max_faces: c_int, item_frame: *const c_int, item_face: *const c_int,
                                  max_items: c_int, embeddings: *mut c_float, valid: *mut c_int, raw: *mut c_float, chips: *mut c_float,
                                  mem: c_int, stream: *mut c_void) -> c_int;
    // aligned face chips (not the reference's behaviour: it crops the box); `source` is one of MI_ALIGN_*
    pub fn mi_face_align_template(source: c_int, xy: *mut c_double, n: *mut c_int) -> c_int;
    pub fn mi_face_align_roi(points_xy: *const c_float, n: c_int, source: c_int, roi: *mut mi_rect, valid: *mut c_int) -> c_int;
    pub fn mi_face_align_points(source: c_int, landmarks_or_detection: *const c_float, width: c_int, height: c_int, points_xy: *mut c_float,
                                n: *mut c_int) -> c_int;
    pub fn mi_fe_infer_image_aligned(h: *mut mi_fe, rgb: *const u8, width: c_int, height: c_int, stride: c_int, points_xy: *const c_float,
                                     n: c_int, source: c_int, embedding: *mut c_float, cap: c_int, roi: *mut mi_rect) -> c_int;
    pub fn mi_fe_infer_aligned_items(h: *mut mi_fe, frames: *const u8, batch: c_int, width: c_int, height: c_int, stride: c_int, source: c_int,
                                     src: *const c_void, gate: *const c_int, max_faces: c_int, item_frame: *const c_int,
                                     item_face: *const c_int, max_items: c_int, embeddings: *mut c_float, valid: *mut c_int,
                                     raw: *mut c_float, chips: *mut c_float, rois: *mut mi_rect, mem: c_int, stream: *mut c_void) -> c_int;
    pub fn mi_l2_norm(input: *const c_float, n: c_int, out: *mut c_float) -> c_int;
    pub fn mi_similarity_score(a: *const c_float, b: *const c_float, n: c_int, out: *mut c_float) -> c_int;
    pub fn mi_similarity_matrix(device: c_int, a: *const c_float, n: c_int, b: *const c_float, m: c_int, features: c_int, out: *mut c_float,
                                mem: c_int, stream: *mut c_void) -> c_int;
    pub fn mi_topk_select(scores: *const c_float, n: c_int, m: c_int, k: c_int, index: *mut c_int, score: *mut c_float) -> c_int;
    pub fn mi_gallery_create(device: c_int, rows: *const c_float, m: c_int, features: c_int, labels: *const c_int, mem: c_int,
                             out: *mut *mut mi_gallery) -> c_int;
    pub fn mi_gallery_free(g: *mut mi_gallery);
    pub fn mi_gallery_dims(g: *const mi_gallery, m: *mut c_int, features: *mut c_int) -> c_int;
    pub fn mi_gallery_set_option(g: *mut mi_gallery, key: *const c_char, value: c_int) -> c_int;
    pub fn mi_gallery_get_option(g: *mut mi_gallery, key: *const c_char, value: *mut c_int) -> c_int;
    pub fn mi_gallery_topk(g: *mut mi_gallery, queries: *const c_float, n: c_int, k: c_int, index: *mut c_int, score: *mut c_float,
                           label: *mut c_int, mem: c_int, stream: *mut c_void) -> c_int;
}
