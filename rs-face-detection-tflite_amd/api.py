"""Host-side mirror of the reference crate's public API over the C ABI (include/mi_face.h) via ctypes.

The reference is a Rust crate (`FaceDetection::{new,infer}`, `FaceLandmark::{new,infer}`, `IrisLandmark::{new,infer}`,
/root/reference/src/face_detection_lite/{face_detection,face_landmark,iris_landmark}.rs); there is no Rust toolchain in
this image, so the host side above the C ABI is mirrored here with the same names, argument meaning and error behaviour
(errors that the reference returns as `anyhow::Error` — or panics on — become `MiError`).  A Rust `extern "C"` shim with
identical signatures is listed in INTEGRATION.md.

No numerical work happens in this module: every result comes from the HIP kernels behind libmiface.so.  If that library
is missing, importing this module raises (there is no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import enum
import os
from dataclasses import dataclass
from collections.abc import Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIFACE_LIB") or os.path.join(_HERE, "libmiface.so")   # MIFACE_LIB: a development variant built by build.sh (MI_VARIANT)
REPO_ROOT = os.path.dirname(_HERE)
DEFAULT_MODEL_DIR = os.path.join(REPO_ROOT, "models")

MI_MEM_HOST, MI_MEM_DEVICE = 0, 1
NUM_FACE_LANDMARKS, NUM_EYE_LANDMARKS, NUM_IRIS_LANDMARKS = 468, 71, 5

EXPORTS = [
    "mi_last_error", "mi_device_count", "mi_version",
    "mi_model_load_file", "mi_model_load_bytes", "mi_model_free", "mi_model_input_dims", "mi_model_num_outputs",
    "mi_model_output_dims", "mi_model_output_elems", "mi_model_run", "mi_model_debug_tensor", "mi_model_describe",
    "mi_dist_broadcast_bytes", "mi_streams_create_distinct", "mi_streams_destroy", "mi_model_set_option", "mi_model_get_option", "mi_plan_describe", "mi_model_plan_stats", "mi_model_single_launch_workgroups", "mi_model_profile",
    "mi_fd_create", "mi_fd_create_from_bytes", "mi_fd_free", "mi_fd_model", "mi_fd_input_size", "mi_fd_num_anchors",
    "mi_fd_anchors", "mi_fd_infer_tensor", "mi_fd_postprocess", "mi_fd_infer_image", "mi_fd_infer_images", "mi_fd_submit_images",
    "mi_fd_collect", "mi_fd_submit_jpeg", "mi_fd_collect_jpeg", "mi_pipeline_submit_jpeg", "mi_pipeline_collect_jpeg", "mi_host_alloc", "mi_host_free",
    "mi_fl_create", "mi_fl_create_from_bytes", "mi_fl_free", "mi_fl_model", "mi_fl_infer_tensor", "mi_fl_infer_images", "mi_fl_submit_images", "mi_fl_collect", "mi_fl_infer_image",
    "mi_iris_create", "mi_iris_create_from_bytes", "mi_iris_free", "mi_iris_model", "mi_iris_infer_tensor", "mi_iris_infer_images",
    "mi_iris_infer_image",
    "mi_pipeline_create", "mi_pipeline_create_from_bytes", "mi_pipeline_model", "mi_pipeline_free", "mi_pipeline_set_option", "mi_pipeline_run",
    "mi_pipeline_run_faces", "mi_face_items_layout",
    "mi_tracker_create", "mi_tracker_create_from_bytes", "mi_tracker_free", "mi_tracker_set_option", "mi_tracker_step", "mi_tracker_reset",
    "mi_tracker_get_state", "mi_tracker_set_state", "mi_track_roi_from_landmarks", "mi_track_detect_layout",
    "mi_bbox_to_roi", "mi_bbox_from_landmarks", "mi_face_detection_to_roi", "mi_iris_roi_from_face_landmarks", "mi_update_face_landmarks_with_iris_results", "mi_image_to_tensor", "mi_jpeg_info", "mi_jpeg_decode_rgb",
    "mi_render_annotations", "mi_render_faces", "mi_render_face_items",
    "mi_fe_create", "mi_fe_create_from_bytes", "mi_fe_free", "mi_fe_model", "mi_fe_features", "mi_face_chip_rect", "mi_fe_infer_image",
    "mi_fe_infer_face_items", "mi_face_align_template", "mi_face_align_roi", "mi_face_align_points", "mi_fe_infer_image_aligned",
    "mi_fe_infer_aligned_items", "mi_l2_norm", "mi_similarity_score", "mi_similarity_matrix",
    "mi_topk_select", "mi_gallery_create", "mi_gallery_free", "mi_gallery_dims", "mi_gallery_set_option", "mi_gallery_get_option", "mi_gallery_topk",
]


class MiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mi_face error %d: %s" % (code, msg))
        self.code = code


class CDetection(C.Structure):
    _fields_ = [("data", C.c_float * 16), ("score", C.c_float)]


class Rect(C.Structure):
    """types.rs:24-36."""
    _fields_ = [("x_center", C.c_double), ("y_center", C.c_double), ("width", C.c_double), ("height", C.c_double),
                ("rotation", C.c_double), ("normalized", C.c_int)]

    def __repr__(self):
        return "Rect(x_center=%r, y_center=%r, width=%r, height=%r, rotation=%r, normalized=%r)" % (
            self.x_center, self.y_center, self.width, self.height, self.rotation, bool(self.normalized))


class CLandmark(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]


class Color(C.Structure):
    """render.rs:6-26 as the four bytes render_to_image writes (alpha None -> 255, render.rs:431)."""
    _fields_ = [("r", C.c_uint8), ("g", C.c_uint8), ("b", C.c_uint8), ("a", C.c_uint8)]

    def __init__(self, r=0, g=0, b=0, a=255):
        super().__init__(int(r), int(g), int(b), 255 if a is None else int(a))

    def as_tuple(self):
        return self.r, self.g, self.b, self.a

    def __repr__(self):
        return "Color(%d, %d, %d, %d)" % self.as_tuple()


class Colors:
    """render.rs:28-68."""
    BLACK = Color(0, 0, 0)
    RED = Color(255, 0, 0)
    GREEN = Color(0, 255, 0)
    BLUE = Color(0, 0, 255)
    PINK = Color(255, 0, 255)
    WHITE = Color(255, 255, 255)


ANN_POINTS, ANN_LINES, ANN_RECTS, ANN_FILLED_RECTS = 0, 1, 2, 3     # AnnotationData variants, render.rs:186-192
_ANN_DOUBLES = {ANN_POINTS: 2, ANN_LINES: 4, ANN_RECTS: 4, ANN_FILLED_RECTS: 4}


class Annotation(C.Structure):
    """mi_annotation (render.rs:207-213): `count` items of one kind whose doubles start at index `first` of a frame's coordinate block."""
    _fields_ = [("kind", C.c_int), ("first", C.c_int), ("count", C.c_int), ("thickness", C.c_double), ("color", Color), ("normalized", C.c_int)]

    def __init__(self, kind=ANN_POINTS, first=0, count=0, thickness=1.0, color=None, normalized=True):
        super().__init__(int(kind), int(first), int(count), float(thickness), color if color is not None else Colors.RED, int(bool(normalized)))


class RenderStyle(C.Structure):
    """mi_render_style: the arguments of detections_to_render_data (render.rs:262-265), face_landmarks_to_render_data
    (face_landmark.rs:324-339) and eye_landmarks_to_render_data (iris_landmark.rs:312-331).  A colour of None is the reference's None
    (bounds / keypoints not drawn); mesh / eyes say whether those groups are drawn at all."""
    _fields_ = [("draw_bounds", C.c_int), ("bounds_color", Color), ("line_width", C.c_int),
                ("draw_keypoints", C.c_int), ("keypoint_color", Color), ("point_width", C.c_int),
                ("draw_mesh", C.c_int), ("mesh_landmark_color", Color), ("mesh_connection_color", Color), ("mesh_thickness", C.c_float),
                ("draw_eyes", C.c_int), ("eye_landmark_color", Color), ("eye_connection_color", Color), ("eye_thickness", C.c_float)]

    def __init__(self, bounds_color=None, keypoint_color=None, line_width=1, point_width=1, mesh=False, mesh_landmark_color=None,
                 mesh_connection_color=None, mesh_thickness=1.0, eyes=False, eye_landmark_color=None, eye_connection_color=None, eye_thickness=1.0):
        red = lambda c: c if c is not None else Colors.RED      # landmark_color.unwrap_or(Colors::RED), render.rs:320-321
        super().__init__(int(bounds_color is not None), bounds_color or Colors.BLACK, int(line_width),
                         int(keypoint_color is not None), keypoint_color or Colors.BLACK, int(point_width),
                         int(bool(mesh)), red(mesh_landmark_color), red(mesh_connection_color), float(mesh_thickness),
                         int(bool(eyes)), red(eye_landmark_color), red(eye_connection_color), float(eye_thickness))


class RenderItemsStyle(C.Structure):
    """mi_render_items_style: a RenderStyle (`base`, read as render_faces reads it) plus the arguments of iris_landmarks_to_render_data
    (iris_landmark.rs:330-335).  A colour of None is the reference's None: that group is not drawn.  iris_thickness None is its default, 1.0."""
    _fields_ = [("base", RenderStyle), ("draw_iris_oval", C.c_int), ("iris_oval_color", Color),
                ("draw_iris_points", C.c_int), ("iris_landmark_color", Color), ("iris_thickness", C.c_double)]

    def __init__(self, base=None, iris_oval_color=None, iris_landmark_color=None, iris_thickness=None):
        super().__init__(base if base is not None else RenderStyle(), int(iris_oval_color is not None), iris_oval_color or Colors.BLACK,
                         int(iris_landmark_color is not None), iris_landmark_color or Colors.BLACK,
                         1.0 if iris_thickness is None else float(iris_thickness))


class FaceDetectionModel(enum.IntEnum):
    """face_detection.rs:117-123."""
    FrontCamera = 0
    BackCamera = 1
    Short = 2
    Full = 3
    FullSparse = 4


@dataclass
class Detection:
    """types.rs:189-246: data [8,2] f32 (bbox corners then 6 keypoints), score f32."""
    data: np.ndarray
    score: float

    def bbox(self):
        return tuple(float(v) for v in (self.data[0, 0], self.data[0, 1], self.data[1, 0], self.data[1, 1]))

    def keypoint(self, k):
        return float(self.data[k + 2, 0]), float(self.data[k + 2, 1])


@dataclass
class Landmark:
    x: float
    y: float
    z: float


class LandmarkList(Sequence):
    """Vec<Landmark> the way the C ABI filled it: one [n,3] f64 array (`.array`: x, y, z per row, types.rs:176-187).  It reads like the list of Landmark the
    reference returns (len, index, slice, iteration, ==); the Landmark objects are made on access, not per call — building 468 Python
    objects costs about as much as a third of the whole single-image mesh call (tools/latency_probe.py)."""
    __slots__ = ("array",)

    def __init__(self, array):
        self.array = array

    def __len__(self):
        return len(self.array)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return LandmarkList(self.array[i])
        x, y, z = self.array[i].tolist()
        return Landmark(x, y, z)

    def __iter__(self):
        it = iter(self.array.ravel().tolist())
        return map(Landmark, it, it, it)

    def __eq__(self, other):
        try:
            return len(self) == len(other) and all(a == b for a, b in zip(self, other))
        except TypeError:
            return NotImplemented

    def __repr__(self):
        return "LandmarkList(%d landmarks)" % len(self)


def _landmarks_from(carray, n):
    """n CLandmark structs -> LandmarkList over its own copy of their floats"""
    return LandmarkList(np.frombuffer(carray, np.float64, 3 * n).reshape(n, 3).copy())


@dataclass
class IrisResults:
    """iris_landmark.rs:115-129."""
    contour: list
    iris: list

    def eyeball_contour(self):
        return self.contour[:15]


_lib = None


def lib():
    """Load libmiface.so (built in-tree by build.sh / __graft_entry__.build()). Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run rs-face-detection-tflite_amd/build.sh (hipcc, gfx950). "
                          "There is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm ships its own libamdhip64; when both live in one process torch must be loaded first so that the
    # two share one HIP runtime (otherwise torch later reports "No HIP GPUs are available").  torch is only plumbing
    # here (device buffers, streams, torch.distributed) — set MIFACE_NO_TORCH=1 to skip it entirely.
    if not os.environ.get("MIFACE_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    vp, fp, ip, dp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.mi_last_error.restype = C.c_char_p
    L.mi_version.restype = C.c_char_p
    L.mi_model_load_file.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.mi_model_load_bytes.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.mi_model_free.argtypes = [vp]
    L.mi_model_free.restype = None
    L.mi_model_input_dims.argtypes = [vp, ip]
    L.mi_model_num_outputs.argtypes = [vp]
    L.mi_model_output_dims.argtypes = [vp, C.c_int, ip, ip]
    L.mi_model_output_elems.argtypes = [vp, C.c_int]
    L.mi_model_output_elems.restype = C.c_size_t
    L.mi_model_run.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.c_int, vp]
    L.mi_model_debug_tensor.argtypes = [vp, C.c_int, C.c_int, fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi_model_describe.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.mi_model_describe.restype = C.c_size_t
    L.mi_model_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.mi_model_get_option.argtypes = [vp, C.c_char_p, ip]
    L.mi_plan_describe.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
    L.mi_plan_describe.restype = C.c_size_t
    L.mi_model_plan_stats.argtypes = [vp, dp, dp, ip]
    L.mi_model_single_launch_workgroups.argtypes = [vp, C.c_int]
    L.mi_model_profile.argtypes = [vp, vp, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.mi_model_profile.restype = C.c_size_t
    L.mi_fd_create.argtypes = [C.c_int, C.c_char_p, C.c_int, C.POINTER(vp)]
    L.mi_fd_create_from_bytes.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.mi_fd_free.argtypes = [vp]
    L.mi_fd_free.restype = None
    L.mi_fd_model.argtypes = [vp]
    L.mi_fd_model.restype = vp
    L.mi_fd_input_size.argtypes = [vp, ip, ip]
    L.mi_fd_num_anchors.argtypes = [vp]
    L.mi_fd_anchors.argtypes = [vp, fp, C.c_int]
    L.mi_fd_infer_tensor.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp]
    L.mi_fd_postprocess.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp]
    L.mi_fd_infer_images.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp]
    L.mi_fd_submit_images.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.mi_fd_collect.argtypes = [vp, C.c_int, vp, vp]
    L.mi_fd_submit_jpeg.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t, C.c_int]
    L.mi_fd_collect_jpeg.argtypes = [vp, C.c_int, vp, C.c_int, ip, ip, ip]
    L.mi_pipeline_submit_jpeg.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t]
    L.mi_pipeline_collect_jpeg.argtypes = [vp, C.c_int, vp, ip, vp, ip, vp, ip, ip]
    L.mi_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.mi_host_free.argtypes = [vp]
    L.mi_host_free.restype = None
    L.mi_fd_infer_image.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(Rect), C.POINTER(CDetection), C.c_int, ip]
    L.mi_fl_create.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.mi_fl_create_from_bytes.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.mi_fl_free.argtypes = [vp]
    L.mi_fl_free.restype = None
    L.mi_fl_model.argtypes = [vp]
    L.mi_fl_model.restype = vp
    L.mi_fl_infer_tensor.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp]
    L.mi_fl_infer_images.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp]
    L.mi_fl_submit_images.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int]
    L.mi_fl_collect.argtypes = [vp, C.c_int, vp, vp, vp]
    L.mi_fl_infer_image.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(Rect), C.POINTER(CLandmark), C.c_int, ip]
    L.mi_iris_create.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.mi_iris_create_from_bytes.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.mi_iris_free.argtypes = [vp]
    L.mi_iris_free.restype = None
    L.mi_iris_model.argtypes = [vp]
    L.mi_iris_model.restype = vp
    L.mi_iris_infer_tensor.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp]
    L.mi_iris_infer_images.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp]
    L.mi_iris_infer_image.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(Rect), C.c_int, C.POINTER(CLandmark),
                                      C.POINTER(CLandmark)]
    L.mi_pipeline_create.argtypes = [C.c_int, C.c_char_p, C.c_int, C.POINTER(vp)]
    L.mi_pipeline_create_from_bytes.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.mi_pipeline_model.argtypes = [vp, C.c_int]
    L.mi_pipeline_model.restype = vp
    L.mi_pipeline_free.argtypes = [vp]
    L.mi_pipeline_free.restype = None
    L.mi_pipeline_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.mi_pipeline_run.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp]
    L.mi_pipeline_run_faces.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]
    L.mi_face_items_layout.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.mi_tracker_create.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    L.mi_tracker_create_from_bytes.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(vp)]
    L.mi_tracker_free.argtypes = [vp]
    L.mi_tracker_free.restype = None
    L.mi_tracker_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.mi_tracker_step.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]
    L.mi_tracker_reset.argtypes = [vp, C.c_int]
    L.mi_tracker_get_state.argtypes = [vp, vp, vp]
    L.mi_tracker_set_state.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.mi_track_roi_from_landmarks.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Rect), ip]
    L.mi_track_detect_layout.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.mi_face_detection_to_roi.argtypes = [C.POINTER(CDetection), C.c_int, C.c_int, C.POINTER(Rect)]
    L.mi_iris_roi_from_face_landmarks.argtypes = [C.POINTER(CLandmark), C.c_int, C.c_int, C.POINTER(Rect), C.POINTER(Rect)]
    L.mi_update_face_landmarks_with_iris_results.argtypes = [C.POINTER(CLandmark)] * 4
    L.mi_bbox_to_roi.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_int, C.POINTER(Rect)]
    L.mi_bbox_from_landmarks.argtypes = [C.POINTER(CLandmark), C.c_int, C.POINTER(C.c_double)]
    L.mi_jpeg_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mi_jpeg_decode_rgb.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p]
    L.mi_image_to_tensor.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(Rect), C.c_int, C.c_int, C.c_int,
                                     C.c_double, C.c_double, C.c_int, vp, dp, C.c_int, vp]
    L.mi_render_annotations.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Annotation), C.c_int, vp, C.c_long, vp, C.c_int,
                                        C.c_int, vp, C.c_int, vp]
    L.mi_render_faces.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.POINTER(RenderStyle), vp, C.c_int,
                                  C.c_int, vp, C.c_int, vp]
    L.mi_render_face_items.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp,
                                       C.POINTER(RenderItemsStyle), vp, C.c_int, C.c_int, vp, C.c_int, vp]
    L.mi_fe_create.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.mi_fe_create_from_bytes.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.mi_fe_free.argtypes = [vp]
    L.mi_fe_free.restype = None
    L.mi_fe_model.argtypes = [vp]
    L.mi_fe_model.restype = vp
    L.mi_fe_features.argtypes = [vp, ip]
    L.mi_face_chip_rect.argtypes = [C.POINTER(CDetection), C.c_int, C.c_int, ip, ip]
    L.mi_fe_infer_image.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, dp, vp, C.c_int]
    L.mi_fe_infer_face_items.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    L.mi_face_align_template.argtypes = [C.c_int, vp, ip]
    L.mi_face_align_roi.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Rect), ip]
    L.mi_face_align_points.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, ip]
    L.mi_fe_infer_image_aligned.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.POINTER(Rect)]
    L.mi_fe_infer_aligned_items.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp,
                                            C.c_int, vp]
    L.mi_l2_norm.argtypes = [vp, C.c_int, vp]
    L.mi_similarity_score.argtypes = [vp, vp, C.c_int, fp]
    L.mi_similarity_matrix.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp]
    L.mi_topk_select.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.mi_gallery_create.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.POINTER(vp)]
    L.mi_gallery_free.argtypes = [vp]
    L.mi_gallery_free.restype = None
    L.mi_gallery_dims.argtypes = [vp, ip, ip]
    L.mi_gallery_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.mi_gallery_get_option.argtypes = [vp, C.c_char_p, ip]
    L.mi_gallery_topk.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise MiError(rc, lib().mi_last_error().decode("utf-8", "replace"))


def device_count():
    return lib().mi_device_count()


def dist_broadcast_bytes(id_path, rank, world, root, data, nbytes=None, device=0, timeout_ms=60000) -> bytes:
    """mi_dist_broadcast_bytes: `data` (bytes) on the root rank, None elsewhere (then `nbytes` says how much to receive).  Returns the
    bytes every rank now holds.  Collective over `world` ranks, one process per GPU, RCCL directly (no torch.distributed)."""
    n = len(data) if data is not None else int(nbytes)
    buf = (C.c_uint8 * n)()
    if data is not None:
        C.memmove(buf, data, n)
    L = lib()
    L.mi_dist_broadcast_bytes.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int]
    _check(L.mi_dist_broadcast_bytes(os.fsencode(id_path), rank, world, root, device, buf, n, timeout_ms))
    return bytes(buf)


def streams_create_distinct(n=2, device=0):
    """mi_streams_create_distinct: n hipStream_t handles (ints) that were tested to sit on distinct hardware queues — pass them as the
    `stream` argument of the batched entries of n handles to keep n batches in flight.  Free with streams_destroy."""
    L = lib()
    arr = (C.c_void_p * n)()
    L.mi_streams_create_distinct.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    _check(L.mi_streams_create_distinct(int(device), int(n), arr))
    return [int(v) for v in arr]


def streams_destroy(streams, device=0):
    L = lib()
    n = len(streams)
    arr = (C.c_void_p * n)(*[C.c_void_p(s) for s in streams])
    L.mi_streams_destroy.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    _check(L.mi_streams_destroy(int(device), n, arr))


def plan_describe(tflite_bytes: bytes, fuse_level=4) -> str:
    """Host-only lowering of a .tflite blob (no GPU needed)."""
    L = lib()
    n = L.mi_plan_describe(tflite_bytes, len(tflite_bytes), fuse_level, None, 0)
    if n == 0:
        raise MiError(-3, L.mi_last_error().decode())
    buf = C.create_string_buffer(n)
    L.mi_plan_describe(tflite_bytes, len(tflite_bytes), fuse_level, buf, n)
    return buf.value.decode()


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _device_ready(x, device, dims=None, dtype="float32"):
    """Checks made before a torch CUDA tensor's raw pointer is handed to the kernels: dtype, device ordinal and trailing
    shape.  Then orders the call after the work already queued by torch: the library launches on the handle's own
    (non-blocking) stream unless the caller passes one, and that stream has no ordering against torch's current stream, so
    everything torch queued so far (the producer of `x`, the zero fills of the outputs allocated next to it) is waited
    for here.  Callers that pass their own `stream` and pre-allocated outputs skip nothing by this: it is one host sync."""
    import torch
    if str(x.dtype) != "torch." + dtype:
        raise ValueError("expected a %s tensor, got %s" % (dtype, x.dtype))
    if not x.is_cuda or (x.device.index or 0) != device:
        raise ValueError("tensor lives on %s but the handle is bound to cuda:%d" % (x.device, device))
    if dims is not None and list(x.shape[1:]) != list(dims):
        raise ValueError("expected frames of shape %s, got %s" % (list(dims), list(x.shape[1:])))
    torch.cuda.current_stream(x.device).synchronize()


def _ptr(x):
    """(pointer, mem) of a numpy array (host) or torch CUDA tensor (device)."""
    if _is_torch(x):
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return C.c_void_p(x.data_ptr()), (MI_MEM_DEVICE if x.is_cuda else MI_MEM_HOST)
    return C.c_void_p(x.ctypes.data), MI_MEM_HOST


class Model:
    """L0 engine handle (replaces the `tflite` crate's FlatBufferModel + Interpreter)."""

    def __init__(self, path=None, device=0, handle=None, owner=None):
        self.L = lib()
        self._owner = owner
        self.device = device
        if handle is not None:
            self.h = C.c_void_p(handle)
        else:
            self.h = C.c_void_p()
            _check(self.L.mi_model_load_file(os.fsencode(path), device, C.byref(self.h)))
        d = (C.c_int * 4)()
        _check(self.L.mi_model_input_dims(self.h, d))
        self.input_dims = list(d)
        self.num_outputs = self.L.mi_model_num_outputs(self.h)
        self.output_dims, self.output_elems = [], []
        for i in range(self.num_outputs):
            r = C.c_int()
            _check(self.L.mi_model_output_dims(self.h, i, d, C.byref(r)))
            self.output_dims.append(list(d)[:r.value])
            self.output_elems.append(self.L.mi_model_output_elems(self.h, i))

    def close(self):
        if self._owner is None and getattr(self, "h", None):
            self.L.mi_model_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        _check(self.L.mi_model_set_option(self.h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int(0)
        _check(self.L.mi_model_get_option(self.h, key.encode(), C.byref(v)))
        return v.value

    def describe(self):
        n = self.L.mi_model_describe(self.h, None, 0)
        buf = C.create_string_buffer(n)
        self.L.mi_model_describe(self.h, buf, n)
        return buf.value.decode()

    def plan_stats(self):
        b, m, n = C.c_double(), C.c_double(), C.c_int()
        _check(self.L.mi_model_plan_stats(self.h, C.byref(b), C.byref(m), C.byref(n)))
        return b.value, m.value, n.value

    def single_launch_workgroups(self, batch=1):
        """Workgroups a single-image call of `batch` frames occupies on the single-launch plan (0: the graph has none / batch too large)."""
        n = self.L.mi_model_single_launch_workgroups(self.h, int(batch))
        if n < 0:
            _check(n)
        return n

    def profile(self, x_device, reps=5):
        """Per-launch HIP-event timing (x_device: torch CUDA tensor). Returns a list of dicts."""
        import json
        p, mem = _ptr(x_device)
        if mem != MI_MEM_DEVICE:
            raise ValueError("profile() needs a device tensor")
        _device_ready(x_device, self.device, self.input_dims[1:])
        B = int(x_device.shape[0])
        cap = 1 << 20
        buf = C.create_string_buffer(cap)
        if self.L.mi_model_profile(self.h, p, B, reps, buf, cap) == 0:
            raise MiError(-1, self.L.mi_last_error().decode())
        return json.loads(buf.value.decode())

    def run(self, x, outs=None, stream=None):
        """x: numpy [B,H,W,C] f32 (host) or torch CUDA tensor. Returns list of outputs in the same memory space."""
        p, mem = _ptr(x)
        B = int(x.shape[0])
        if outs is None:
            if mem == MI_MEM_DEVICE:
                import torch
                outs = [torch.empty([B] + d[1:], dtype=torch.float32, device=x.device) for d in self.output_dims]
            else:
                x = np.ascontiguousarray(x, np.float32)
                p = C.c_void_p(x.ctypes.data)
                outs = [np.empty([B] + d[1:], np.float32) for d in self.output_dims]
        if mem == MI_MEM_DEVICE:
            _device_ready(x, self.device, self.input_dims[1:])
        ptrs = (C.c_void_p * self.num_outputs)(*[_ptr(o)[0] for o in outs])
        _check(self.L.mi_model_run(self.h, p, B, ptrs, mem, C.c_void_p(stream or 0)))
        return outs

    def debug_tensor(self, index, frame=0, cap=1 << 24):
        dst = np.empty(cap, np.float32)
        n = C.c_size_t()
        _check(self.L.mi_model_debug_tensor(self.h, index, frame, dst.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n)))
        return dst[:n.value].copy()


def _image_args(image):
    image = np.ascontiguousarray(image, np.uint8)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("image must be uint8 [H,W,3] RGB")
    h, w = image.shape[:2]
    return image, w, h, image.strides[0]



def _frames_and_rois(frames, rois, items_per_frame, device):
    """(pointer, mem, B, H, W, stride, rois pointer, keep-alive) for the batched u8 entry points: frames uint8 [B,H,W,3] (numpy, or a
    contiguous torch CUDA tensor); rois None, a sequence of B * items_per_frame Rect (host frames) or a device tensor holding them."""
    p, mem = _ptr(frames)
    B, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    N = B * items_per_frame
    if rois is None and items_per_frame != 1:
        raise ValueError("several items per frame need their ROIs")
    if mem == MI_MEM_DEVICE:
        import torch
        if frames.dtype != torch.uint8 or not frames.is_contiguous() or frames.shape[3] != 3:
            raise ValueError("frames must be a contiguous uint8 [B,H,W,3] tensor")
        _device_ready(frames, device, None, dtype="uint8")
        rp = C.c_void_p(rois.data_ptr()) if rois is not None else None
        return p, mem, B, H, W, 3 * W, rp, frames
    frames = np.ascontiguousarray(frames, np.uint8)
    if frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError("frames must be uint8 [B,H,W,3]")
    rarr = None
    if rois is not None:
        if len(rois) != N:
            raise ValueError("expected %d rois" % N)
        rarr = rois if isinstance(rois, C.Array) else (Rect * N)(*rois)
    return C.c_void_p(frames.ctypes.data), mem, B, H, W, frames.strides[1], (C.cast(rarr, C.c_void_p) if rarr is not None else None), (frames, rarr)


class PinnedBuffer:
    """Page-locked host memory (mi_host_alloc) viewed as a numpy array; freed with the object."""

    def __init__(self, shape, dtype=np.uint8):
        self.L = lib()
        self.ptr = C.c_void_p()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        _check(self.L.mi_host_alloc(n, C.byref(self.ptr)))
        self.array = np.frombuffer((C.c_char * n).from_address(self.ptr.value), dtype=dtype).reshape(shape)

    def close(self):
        if getattr(self, "ptr", None) and self.ptr.value:
            self.array = None
            self.L.mi_host_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FaceDetection:
    """BlazeFace detector — mirrors face_detection.rs:146-267."""

    def __init__(self, model_type=FaceDetectionModel.FrontCamera, model_path=None, device=0, model_bytes=None):
        self.L = lib()
        self.h = C.c_void_p()
        self._slot_shape = {}   # slot -> (B, cap, frames) of the batch submit_images() queued
        self._jpeg_cap = {}     # slot -> cap of the picture submit_jpeg() queued
        # model_path is a DIRECTORY (face_detection.rs:157-161); default "./models" resolved against the repo here
        d = model_path if model_path is not None else DEFAULT_MODEL_DIR
        if model_bytes is not None:      # the frozen .tflite already in memory (e.g. after an RCCL broadcast)
            _check(self.L.mi_fd_create_from_bytes(int(model_type), model_bytes, len(model_bytes), device, C.byref(self.h)))
        else:
            _check(self.L.mi_fd_create(int(model_type), os.fsencode(d), device, C.byref(self.h)))
        w, h = C.c_int(), C.c_int()
        self.L.mi_fd_input_size(self.h, C.byref(w), C.byref(h))
        self.input_size = (w.value, h.value)
        self.num_anchors = self.L.mi_fd_num_anchors(self.h)
        self.device = device
        self.model = Model(handle=self.L.mi_fd_model(self.h), owner=self, device=device)

    def close(self):
        if getattr(self, "h", None):
            self.L.mi_fd_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def anchors(self):
        a = np.zeros((self.num_anchors, 2), np.float32)
        self.L.mi_fd_anchors(self.h, a.ctypes.data_as(C.POINTER(C.c_float)), self.num_anchors)
        return a

    def infer(self, image, roi=None, cap=256):
        """FaceDetection::infer(&Mat, Option<Rect>) -> Vec<Detection> (face_detection.rs:205-267)."""
        image, w, h, stride = _image_args(image)
        while True:
            out = (CDetection * cap)()
            n = C.c_int()
            _check(self.L.mi_fd_infer_image(self.h, C.c_void_p(image.ctypes.data), w, h, stride,
                                            C.byref(roi) if roi is not None else None, out, cap, C.byref(n)))
            if n.value <= cap:      # the reference returns every detection: never truncate silently
                break
            cap = n.value
        return [Detection(np.frombuffer(out[i].data, np.float32, 16).reshape(8, 2).copy(), float(out[i].score))
                for i in range(min(n.value, cap))]

    def infer_tensor(self, x, padding=None, cap=64, out=None, counts=None, stream=None):
        """Batched tensor-stage entry (configs 2/4). x: [B,H,W,3] f32 numpy or torch CUDA tensor in [-1,1].
        Returns (detections [B,cap,17] f32, counts [B] i32) in the same memory space as x."""
        p, mem = _ptr(x)
        B = int(x.shape[0])
        if mem == MI_MEM_DEVICE:
            import torch
            if out is None:
                out = torch.zeros((B, cap, 17), dtype=torch.float32, device=x.device)
            if counts is None:
                counts = torch.zeros((B,), dtype=torch.int32, device=x.device)
            pp = C.c_void_p(padding.data_ptr()) if padding is not None else None
            _device_ready(x, self.device, self.model.input_dims[1:])
        else:
            x = np.ascontiguousarray(x, np.float32)
            p = C.c_void_p(x.ctypes.data)
            out = np.zeros((B, cap, 17), np.float32) if out is None else out
            counts = np.zeros((B,), np.int32) if counts is None else counts
            if padding is not None:
                padding = np.ascontiguousarray(padding, np.float64).reshape(B, 4)
            pp = C.c_void_p(padding.ctypes.data) if padding is not None else None
        _check(self.L.mi_fd_infer_tensor(self.h, p, B, pp, _ptr(out)[0], cap, _ptr(counts)[0], mem, C.c_void_p(stream or 0)))
        return out, counts

    def infer_images(self, frames, rois=None, cap=64, out=None, counts=None, stream=None):
        """Batched FaceDetection::infer on u8 RGB frames [B,H,W,3] (numpy, or a torch CUDA uint8 tensor): device-side
        image_to_tensor + network + post-processing in one call.  rois: None or a sequence of B Rect (host frames only).
        Returns (detections [B,cap,17] f32, counts [B] i32) in the memory space of `frames`."""
        p, mem = _ptr(frames)
        B, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        if mem == MI_MEM_DEVICE:
            import torch
            if frames.dtype != torch.uint8 or not frames.is_contiguous() or frames.shape[3] != 3:
                raise ValueError("frames must be a contiguous uint8 [B,H,W,3] tensor")
            if rois is not None:
                raise ValueError("rois are host-side only here")
            stride = 3 * W
            out = torch.zeros((B, cap, 17), dtype=torch.float32, device=frames.device) if out is None else out
            counts = torch.zeros((B,), dtype=torch.int32, device=frames.device) if counts is None else counts
            rp = None
            _device_ready(frames, self.device, None, dtype="uint8")
        else:
            frames = np.ascontiguousarray(frames, np.uint8)
            if frames.ndim != 4 or frames.shape[3] != 3:
                raise ValueError("frames must be uint8 [B,H,W,3]")
            p, stride = C.c_void_p(frames.ctypes.data), frames.strides[1]
            out = np.zeros((B, cap, 17), np.float32) if out is None else out
            counts = np.zeros((B,), np.int32) if counts is None else counts
            rarr = (Rect * B)(*rois) if rois is not None else None
            rp = C.cast(rarr, C.c_void_p) if rarr is not None else None
        _check(self.L.mi_fd_infer_images(self.h, p, B, W, H, stride, rp, _ptr(out)[0], cap, _ptr(counts)[0], mem, C.c_void_p(stream or 0)))
        return out, counts

    def submit_images(self, slot, frames, cap=64):
        """Queues one batch of host frames (numpy uint8 [B,H,W,3]; pinned — `pinned_frames()` — for the copy to overlap the other
        slot's kernels) and returns at once; `collect(slot)` hands the results out."""
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or not frames.flags["C_CONTIGUOUS"]:
            raise ValueError("frames must be a C-contiguous uint8 [B,H,W,3] array")
        B, H, W = frames.shape[:3]
        _check(self.L.mi_fd_submit_images(self.h, slot, C.c_void_p(frames.ctypes.data), B, W, H, frames.strides[1], cap))
        self._slot_shape[slot] = (B, cap, frames)   # keeps the frames alive until collect()

    def collect(self, slot):
        B, cap, _ = self._slot_shape.pop(slot)
        out = np.zeros((B, cap, 17), np.float32)
        counts = np.zeros((B,), np.int32)
        _check(self.L.mi_fd_collect(self.h, slot, C.c_void_p(out.ctypes.data), C.c_void_p(counts.ctypes.data)))
        return out, counts

    def submit_jpeg(self, slot, im_bytes, cap=64):
        """convert_image_to_mat + infer for a stream of encoded pictures (utils.rs:8-21, face_detection.rs:205): Huffman decoding happens in this
        call, on this thread, while the device still works on the other slot's picture; everything else is queued.  `collect_jpeg(slot)`
        returns the detections."""
        _check(self.L.mi_fd_submit_jpeg(self.h, slot, im_bytes, len(im_bytes), cap))
        self._jpeg_cap[slot] = cap

    def collect_jpeg(self, slot, with_size=False):
        cap = self._jpeg_cap.get(slot, 64)   # (nothing submitted: the library refuses the call)
        buf = (CDetection * cap)()
        n, w, h = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(self.L.mi_fd_collect_jpeg(self.h, slot, buf, cap, C.byref(n), C.byref(w), C.byref(h)))
        self._jpeg_cap.pop(slot, None)
        dets = [Detection(np.frombuffer(buf[i].data, np.float32, 16).reshape(8, 2).copy(), float(buf[i].score)) for i in range(min(n.value, cap))]
        return (dets, (w.value, h.value)) if with_size else dets

    def postprocess(self, raw_boxes, raw_scores, padding=None, cap=64):
        """Post-network stage only (decode + sigmoid + weighted NMS + letterbox removal) on host arrays."""
        rb = np.ascontiguousarray(raw_boxes, np.float32).reshape(-1, self.num_anchors, 16)
        rs = np.ascontiguousarray(raw_scores, np.float32).reshape(-1, self.num_anchors)
        B = rb.shape[0]
        out = np.zeros((B, cap, 17), np.float32)
        counts = np.zeros((B,), np.int32)
        pp = None
        if padding is not None:
            padding = np.ascontiguousarray(padding, np.float64).reshape(B, 4)
            pp = C.c_void_p(padding.ctypes.data)
        _check(self.L.mi_fd_postprocess(self.h, C.c_void_p(rb.ctypes.data), C.c_void_p(rs.ctypes.data), B, pp,
                                        C.c_void_p(out.ctypes.data), cap, C.c_void_p(counts.ctypes.data), MI_MEM_HOST, None))
        return out, counts


class FaceLandmark:
    """468-point face mesh — mirrors face_landmark.rs:200-306."""

    def __init__(self, model_path=None, device=0, model_bytes=None):
        self.L = lib()
        self.h = C.c_void_p()
        self._slot_shape = {}   # slot -> (N, frames, rois) of the batch submit_images() queued
        p = model_path if model_path is not None else os.path.join(DEFAULT_MODEL_DIR, "face_landmark.tflite")
        if model_bytes is not None:
            _check(self.L.mi_fl_create_from_bytes(model_bytes, len(model_bytes), device, C.byref(self.h)))
        else:
            _check(self.L.mi_fl_create(os.fsencode(p), device, C.byref(self.h)))
        self.device = device
        self.model = Model(handle=self.L.mi_fl_model(self.h), owner=self, device=device)

    def close(self):
        if getattr(self, "h", None):
            self.L.mi_fl_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def infer(self, image, roi=None):
        """FaceLandmark::infer(&Mat, Option<Rect>) -> Vec<Landmark> (empty when the face flag fails)."""
        image, w, h, stride = _image_args(image)
        out = (CLandmark * NUM_FACE_LANDMARKS)()
        n = C.c_int()
        _check(self.L.mi_fl_infer_image(self.h, C.c_void_p(image.ctypes.data), w, h, stride,
                                        C.byref(roi) if roi is not None else None, out, NUM_FACE_LANDMARKS, C.byref(n)))
        return _landmarks_from(out, n.value)

    def infer_tensor(self, x, rois=None, image_sizes=None, stream=None):
        """x [B,192,192,3] in [0,1]. rois: list of Rect (host path) . Returns (landmarks [B,468,3], present [B], flags [B])."""
        p, mem = _ptr(x)
        B = int(x.shape[0])
        if mem == MI_MEM_DEVICE:
            import torch
            lm = torch.zeros((B, NUM_FACE_LANDMARKS, 3), dtype=torch.float32, device=x.device)
            present = torch.zeros((B,), dtype=torch.int32, device=x.device)
            flags = torch.zeros((B,), dtype=torch.float32, device=x.device)
            rp = C.c_void_p(rois.data_ptr()) if rois is not None else None
            sp = C.c_void_p(image_sizes.data_ptr()) if image_sizes is not None else None
            _device_ready(x, self.device, self.model.input_dims[1:])
        else:
            x = np.ascontiguousarray(x, np.float32)
            p = C.c_void_p(x.ctypes.data)
            lm = np.zeros((B, NUM_FACE_LANDMARKS, 3), np.float32)
            present = np.zeros((B,), np.int32)
            flags = np.zeros((B,), np.float32)
            rp = sp = None
            if rois is not None:
                arr = (Rect * B)(*rois)
                rp = C.cast(arr, C.c_void_p)
                image_sizes = np.ascontiguousarray(image_sizes, np.int32).reshape(B, 2)
                sp = C.c_void_p(image_sizes.ctypes.data)
        _check(self.L.mi_fl_infer_tensor(self.h, p, B, rp, sp, _ptr(lm)[0], _ptr(present)[0], _ptr(flags)[0], mem,
                                         C.c_void_p(stream or 0)))
        return lm, present, flags


    def infer_images(self, frames, rois=None, items_per_frame=1, stream=None):
        """Batched FaceLandmark::infer on u8 RGB frames [B,H,W,3] with one ROI per item (item i reads frame i // items_per_frame): device
        image_to_tensor + network + face flag + projection in one call.  Returns (landmarks [N,468,3], present [N], flags [N]) in the
        memory space of `frames`, N = B * items_per_frame."""
        p, mem, B, H, W, stride, rp, keep = _frames_and_rois(frames, rois, items_per_frame, self.device)
        N = B * items_per_frame
        if mem == MI_MEM_DEVICE:
            import torch
            lm = torch.zeros((N, NUM_FACE_LANDMARKS, 3), dtype=torch.float32, device=frames.device)
            present = torch.zeros((N,), dtype=torch.int32, device=frames.device)
            flags = torch.zeros((N,), dtype=torch.float32, device=frames.device)
        else:
            lm, present, flags = np.zeros((N, NUM_FACE_LANDMARKS, 3), np.float32), np.zeros((N,), np.int32), np.zeros((N,), np.float32)
        _check(self.L.mi_fl_infer_images(self.h, p, B, W, H, stride, rp, items_per_frame, _ptr(lm)[0], _ptr(present)[0], _ptr(flags)[0], mem,
                                         C.c_void_p(stream or 0)))
        return lm, present, flags


    def submit_images(self, slot, frames, rois=None, items_per_frame=1):
        """Queues one batch of host frames (numpy uint8 [B,H,W,3], pinned for the copy to overlap the other slot's kernels) with their ROIs
        and returns at once; `collect(slot)` hands the results out."""
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or not frames.flags["C_CONTIGUOUS"]:
            raise ValueError("frames must be a C-contiguous uint8 [B,H,W,3] array")
        B, H, W = frames.shape[:3]
        N = B * items_per_frame
        rarr = None
        if rois is not None:
            rarr = rois if isinstance(rois, C.Array) else (Rect * N)(*rois)
            if len(rarr) != N:
                raise ValueError("expected %d rois" % N)
        _check(self.L.mi_fl_submit_images(self.h, slot, C.c_void_p(frames.ctypes.data), B, W, H, frames.strides[1],
                                          C.cast(rarr, C.c_void_p) if rarr is not None else None, items_per_frame))
        self._slot_shape[slot] = (N, frames, rarr)   # keeps frames and ROIs alive until collect()

    def collect(self, slot):
        N, _, _ = self._slot_shape.pop(slot)
        lm, present, flags = np.zeros((N, NUM_FACE_LANDMARKS, 3), np.float32), np.zeros((N,), np.int32), np.zeros((N,), np.float32)
        _check(self.L.mi_fl_collect(self.h, slot, C.c_void_p(lm.ctypes.data), C.c_void_p(present.ctypes.data), C.c_void_p(flags.ctypes.data)))
        return lm, present, flags


class IrisLandmark:
    """Iris / eye-contour model — mirrors iris_landmark.rs:130-248."""

    def __init__(self, model_path=None, device=0, model_bytes=None):
        self.L = lib()
        self.h = C.c_void_p()
        p = model_path if model_path is not None else os.path.join(DEFAULT_MODEL_DIR, "iris_landmark.tflite")
        if model_bytes is not None:
            _check(self.L.mi_iris_create_from_bytes(model_bytes, len(model_bytes), device, C.byref(self.h)))
        else:
            _check(self.L.mi_iris_create(os.fsencode(p), device, C.byref(self.h)))
        self.device = device
        self.model = Model(handle=self.L.mi_iris_model(self.h), owner=self, device=device)

    def close(self):
        if getattr(self, "h", None):
            self.L.mi_iris_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def infer(self, image, roi=None, is_right_eye=None):
        """IrisLandmark::infer(&Mat, Option<Rect>, Option<bool>) -> IrisResults."""
        image, w, h, stride = _image_args(image)
        c = (CLandmark * NUM_EYE_LANDMARKS)()
        i5 = (CLandmark * NUM_IRIS_LANDMARKS)()
        _check(self.L.mi_iris_infer_image(self.h, C.c_void_p(image.ctypes.data), w, h, stride,
                                          C.byref(roi) if roi is not None else None, int(bool(is_right_eye)), c, i5))
        return IrisResults(_landmarks_from(c, NUM_EYE_LANDMARKS), _landmarks_from(i5, NUM_IRIS_LANDMARKS))

    def infer_tensor(self, x, rois=None, image_sizes=None, padding=None, is_right_eye=None, stream=None):
        p, mem = _ptr(x)
        B = int(x.shape[0])
        if mem == MI_MEM_DEVICE:
            import torch
            contour = torch.zeros((B, NUM_EYE_LANDMARKS, 3), dtype=torch.float32, device=x.device)
            iris = torch.zeros((B, NUM_IRIS_LANDMARKS, 3), dtype=torch.float32, device=x.device)
            g = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
            rp, sp, pp, fp_ = g(rois), g(image_sizes), g(padding), g(is_right_eye)
            _device_ready(x, self.device, self.model.input_dims[1:])
        else:
            x = np.ascontiguousarray(x, np.float32)
            p = C.c_void_p(x.ctypes.data)
            contour = np.zeros((B, NUM_EYE_LANDMARKS, 3), np.float32)
            iris = np.zeros((B, NUM_IRIS_LANDMARKS, 3), np.float32)
            rp = sp = pp = fp_ = None
            keep = []
            if rois is not None:
                arr = (Rect * B)(*rois)
                keep.append(arr)
                rp = C.cast(arr, C.c_void_p)
                image_sizes = np.ascontiguousarray(image_sizes, np.int32).reshape(B, 2)
                sp = C.c_void_p(image_sizes.ctypes.data)
            if padding is not None:
                padding = np.ascontiguousarray(padding, np.float64).reshape(B, 4)
                pp = C.c_void_p(padding.ctypes.data)
            if is_right_eye is not None:
                is_right_eye = np.ascontiguousarray(is_right_eye, np.int32).reshape(B)
                fp_ = C.c_void_p(is_right_eye.ctypes.data)
        _check(self.L.mi_iris_infer_tensor(self.h, p, B, rp, sp, pp, fp_, _ptr(contour)[0], _ptr(iris)[0], mem,
                                           C.c_void_p(stream or 0)))
        return contour, iris


    def infer_images(self, frames, rois=None, is_right_eye=None, items_per_frame=1, stream=None):
        """Batched IrisLandmark::infer on u8 RGB frames [B,H,W,3] with one eye ROI (+ is_right_eye) per item (item i reads frame
        i // items_per_frame).  Returns (contour [N,71,3], iris [N,5,3]) in the memory space of `frames`."""
        p, mem, B, H, W, stride, rp, keep = _frames_and_rois(frames, rois, items_per_frame, self.device)
        N = B * items_per_frame
        fp_ = None
        if mem == MI_MEM_DEVICE:
            import torch
            contour = torch.zeros((N, NUM_EYE_LANDMARKS, 3), dtype=torch.float32, device=frames.device)
            iris = torch.zeros((N, NUM_IRIS_LANDMARKS, 3), dtype=torch.float32, device=frames.device)
            if is_right_eye is not None:
                fp_ = C.c_void_p(is_right_eye.data_ptr())
        else:
            contour, iris = np.zeros((N, NUM_EYE_LANDMARKS, 3), np.float32), np.zeros((N, NUM_IRIS_LANDMARKS, 3), np.float32)
            if is_right_eye is not None:
                is_right_eye = np.ascontiguousarray(is_right_eye, np.int32).reshape(N)
                fp_ = C.c_void_p(is_right_eye.ctypes.data)
        _check(self.L.mi_iris_infer_images(self.h, p, B, W, H, stride, rp, fp_, items_per_frame, _ptr(contour)[0], _ptr(iris)[0], mem,
                                           C.c_void_p(stream or 0)))
        return contour, iris


class Pipeline:
    """Batched detector -> mesh -> iris flow of lib.rs:18-40 / README.md:27-46, every stage on the GPU."""

    def __init__(self, model_type=FaceDetectionModel.BackCamera, model_dir=None, device=0, model_bytes=None):
        self.L = lib()
        self.h = C.c_void_p()
        d = model_dir if model_dir is not None else DEFAULT_MODEL_DIR
        self.device = device
        if model_bytes is not None:   # (detector, face_landmark, iris_landmark) .tflite blobs, e.g. received by RCCL broadcast
            fd_b, fl_b, ir_b = model_bytes
            _check(self.L.mi_pipeline_create_from_bytes(int(model_type), fd_b, len(fd_b), fl_b, len(fl_b), ir_b, len(ir_b), device, C.byref(self.h)))
        else:
            _check(self.L.mi_pipeline_create(int(model_type), os.fsencode(d), device, C.byref(self.h)))
        self.models = [Model(handle=self.L.mi_pipeline_model(self.h, k), owner=self, device=device) for k in range(3)]

    def close(self):
        if getattr(self, "h", None):
            self.L.mi_pipeline_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        _check(self.L.mi_pipeline_set_option(self.h, key.encode(), int(value)))

    def run(self, frames, stream=None):
        """frames: uint8 [B,H,W,3] RGB (numpy, or a torch CUDA tensor).
        Returns dict(faces [B,17], face_counts [B], landmarks [B,468,3], present [B], eyes [B,2,76,3])."""
        B, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        if _is_torch(frames) and frames.is_cuda:
            import torch
            mem, dev = MI_MEM_DEVICE, frames.device
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            out = dict(faces=z((B, 17), torch.float32), face_counts=z((B,), torch.int32), landmarks=z((B, 468, 3), torch.float32),
                       present=z((B,), torch.int32), eyes=z((B, 2, 76, 3), torch.float32))
            p = C.c_void_p(frames.data_ptr())
            stride = int(frames.stride(1))
            if frames.dim() != 4 or frames.shape[3] != 3 or frames.stride(2) != 3 or frames.stride(3) != 1 or frames.stride(0) != stride * H:
                raise ValueError("frames must be [B,H,W,3] with dense pixels and frames stride*H bytes apart")
            _device_ready(frames, self.device, None, "uint8")
        else:
            frames = np.ascontiguousarray(frames, np.uint8)
            mem = MI_MEM_HOST
            out = dict(faces=np.zeros((B, 17), np.float32), face_counts=np.zeros((B,), np.int32), landmarks=np.zeros((B, 468, 3), np.float32),
                       present=np.zeros((B,), np.int32), eyes=np.zeros((B, 2, 76, 3), np.float32))
            p = C.c_void_p(frames.ctypes.data)
            stride = int(frames.strides[1])
        _check(self.L.mi_pipeline_run(self.h, p, B, W, H, stride, _ptr(out["faces"])[0], _ptr(out["face_counts"])[0],
                                      _ptr(out["landmarks"])[0], _ptr(out["present"])[0], _ptr(out["eyes"])[0], mem, C.c_void_p(stream or 0)))
        return out

    def run_faces(self, frames, max_faces=4, max_items=None, stream=None):
        """The same flow for the first `max_faces` (1..16) faces of every frame (mi_pipeline_run_faces; max_items 1..32767).  frames as in run().  The faces of the
        batch are compacted into `max_items` items (None: B * max_faces) in frame order, then detector order; the mesh and iris networks run on
        exactly max_items / 2 * max_items items whatever the detector finds, so choose max_items for the faces you expect.
        Returns dict(faces [B,max_faces,17], face_counts [B], item_frame [M], item_face [M] (-1 in unused slots), landmarks [M,468,3],
        present [M], eyes [M,2,76,3], counts [2] = (n_items, dropped), n_items = slots used, dropped = faces within max_faces that got no slot).
        n_items and dropped are ints for host frames; for device frames they are 0-d views of `counts` (nothing is read back)."""
        B, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        F = int(max_faces)
        M = B * F if max_items is None else int(max_items)
        if not (1 <= F <= 16 and 1 <= M <= 32767):   # (before the outputs are sized by them; the C entry checks again)
            raise MiError(-1, "max_faces must be 1..16 and max_items 1..32767")   # MI_EINVAL
        shapes = dict(faces=((B, F, 17), "float32"), face_counts=((B,), "int32"), item_frame=((M,), "int32"), item_face=((M,), "int32"),
                      counts=((2,), "int32"), landmarks=((M, 468, 3), "float32"), present=((M,), "int32"), eyes=((M, 2, 76, 3), "float32"))
        if _is_torch(frames) and frames.is_cuda:
            import torch
            mem = MI_MEM_DEVICE
            out = {k: torch.zeros(sh, dtype=getattr(torch, dt), device=frames.device) for k, (sh, dt) in shapes.items()}
            p = C.c_void_p(frames.data_ptr())
            stride = int(frames.stride(1))
            if frames.dim() != 4 or frames.shape[3] != 3 or frames.stride(2) != 3 or frames.stride(3) != 1 or frames.stride(0) != stride * H:
                raise ValueError("frames must be [B,H,W,3] with dense pixels and frames stride*H bytes apart")
            _device_ready(frames, self.device, None, "uint8")
        else:
            frames = np.ascontiguousarray(frames, np.uint8)
            mem = MI_MEM_HOST
            out = {k: np.zeros(sh, getattr(np, dt)) for k, (sh, dt) in shapes.items()}
            p = C.c_void_p(frames.ctypes.data)
            stride = int(frames.strides[1])
        _check(self.L.mi_pipeline_run_faces(self.h, p, B, W, H, stride, F, M, _ptr(out["faces"])[0], _ptr(out["face_counts"])[0],
                                            _ptr(out["item_frame"])[0], _ptr(out["item_face"])[0], _ptr(out["counts"])[0], _ptr(out["landmarks"])[0],
                                            _ptr(out["present"])[0], _ptr(out["eyes"])[0], mem, C.c_void_p(stream or 0)))
        # host frames: ints; device frames: 0-d views of `counts` on the device (nothing is read back)
        out["n_items"], out["dropped"] = (int(out["counts"][0]), int(out["counts"][1])) if mem == MI_MEM_HOST else (out["counts"][0], out["counts"][1])
        return out


def face_items_layout(face_counts, max_faces, max_items):
    """mi_face_items_layout (host only, no GPU): the item layout Pipeline.run_faces produces for these detection counts.
    -> (item_frame int32 [max_items], item_face int32 [max_items], n_items, dropped)."""
    counts = np.ascontiguousarray(face_counts, np.int32).reshape(-1)
    M = int(max_items)
    # (the C entry writes max_items entries and refuses a max_items it would not write: the arrays need never be larger than its limit)
    item_frame, item_face, n = np.zeros((max(min(M, 1 << 20), 1),), np.int32), np.zeros((max(min(M, 1 << 20), 1),), np.int32), np.zeros((2,), np.int32)
    _check(lib().mi_face_items_layout(C.c_void_p(counts.ctypes.data), int(counts.size), int(max_faces), M, C.c_void_p(item_frame.ctypes.data),
                                      C.c_void_p(item_face.ctypes.data), C.c_void_p(n.ctypes.data)))
    return item_frame, item_face, int(n[0]), int(n[1])


def track_roi_from_landmarks(landmarks, image_size):
    """mi_track_roi_from_landmarks (host only, no GPU): the ROI Tracker derives for the next frame from one face's landmarks [468,3] (float32,
    normalised to the frame) on a frame of image_size = (width, height).  NOT the reference's behaviour: MediaPipe's landmarks-to-ROI step.
    -> (Rect, valid)."""
    lm = np.ascontiguousarray(landmarks, np.float32)
    if lm.shape != (468, 3):
        raise ValueError("landmarks must be [468, 3]")
    r, ok = Rect(), C.c_int(0)
    _check(lib().mi_track_roi_from_landmarks(C.c_void_p(lm.ctypes.data), int(image_size[0]), int(image_size[1]), C.byref(r), C.byref(ok)))
    return r, bool(ok.value)


def track_detect_layout(tracked, max_detect, start=0):
    """mi_track_detect_layout (host only, no GPU): which lost streams get the detector slots of a Tracker step.
    -> (det_stream int32 [max_detect] (-1 in unused slots), slots used, lost streams left without a slot)."""
    tr = np.ascontiguousarray(tracked, np.int32).reshape(-1)
    D = int(max_detect)
    det, n = np.zeros((max(min(D, 1 << 20), 1),), np.int32), np.zeros((2,), np.int32)
    _check(lib().mi_track_detect_layout(C.c_void_p(tr.ctypes.data), int(tr.size), D, int(start), C.c_void_p(det.ctypes.data), C.c_void_p(n.ctypes.data)))
    return det, int(n[0]), int(n[1])


class Tracker:
    """mi_tracker: landmark-to-ROI face tracking for `streams` video streams, one face per stream.  The ROI of a stream's next frame comes
    from the landmarks of its last one; the detector runs only for streams that have no face yet or have lost it, on `max_detect` items per
    step.  NOT the reference's behaviour (it has no video loop): MediaPipe's, composed from the reference's own functions."""

    def __init__(self, model=FaceDetectionModel.BackCamera, streams=1, model_dir=None, device=0, model_bytes=None):
        self.L = lib()
        self.h = C.c_void_p()
        self.device = device
        self.streams = int(streams)
        d = model_dir if model_dir is not None else DEFAULT_MODEL_DIR
        if model_bytes is not None:   # (detector, face_landmark, iris_landmark) .tflite blobs
            fd_b, fl_b, ir_b = model_bytes
            _check(self.L.mi_tracker_create_from_bytes(int(model), fd_b, len(fd_b), fl_b, len(fl_b), ir_b, len(ir_b), device, self.streams, C.byref(self.h)))
        else:
            _check(self.L.mi_tracker_create(int(model), os.fsencode(d), device, self.streams, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.L.mi_tracker_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        _check(self.L.mi_tracker_set_option(self.h, key.encode(), int(value)))

    def step(self, frames, max_detect=None, stream=None):
        """frames: uint8 [streams,H,W,3] RGB (numpy, or a torch CUDA tensor), frame s the next picture of stream s.  max_detect: detector
        items of this step (1..streams; None: streams).  Returns dict(faces [S,17], face_counts [S], source [S] (2 tracked, 1 detected,
        0 none), rois (a numpy array of RECT_DTYPE [S] for host frames; a uint8 tensor [S,48], mi_rect as it lies in memory, for device frames),
        landmarks [S,468,3], present [S], eyes [S,2,76,3], det_stream [max_detect], n_detect [2])."""
        if len(frames.shape) != 4 or frames.shape[3] != 3:
            raise ValueError("frames must be [S,H,W,3]")
        S, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        D = S if max_detect is None else int(max_detect)
        if S != self.streams:
            raise MiError(-1, "frames must hold one frame per stream (%d), got %d" % (self.streams, S))   # MI_EINVAL
        if not 1 <= D <= S:   # (before the outputs are sized by it; the C entry checks again)
            raise MiError(-1, "max_detect must be 1..streams")
        shapes = dict(faces=((S, 17), "float32"), face_counts=((S,), "int32"), source=((S,), "int32"), rois=((S, 48), "uint8"),
                      landmarks=((S, 468, 3), "float32"), present=((S,), "int32"), eyes=((S, 2, 76, 3), "float32"), det_stream=((D,), "int32"),
                      n_detect=((2,), "int32"))
        if _is_torch(frames) and frames.is_cuda:
            import torch
            mem = MI_MEM_DEVICE
            out = {k: torch.zeros(sh, dtype=getattr(torch, dt), device=frames.device) for k, (sh, dt) in shapes.items()}
            p = C.c_void_p(frames.data_ptr())
            stride = int(frames.stride(1))
            if frames.stride(2) != 3 or frames.stride(3) != 1 or frames.stride(0) != stride * H:
                raise ValueError("frames must be [S,H,W,3] with dense pixels and frames stride*H bytes apart")
            _device_ready(frames, self.device, None, "uint8")
        else:
            frames = np.ascontiguousarray(frames, np.uint8)
            mem = MI_MEM_HOST
            out = {k: np.zeros(sh, getattr(np, dt)) for k, (sh, dt) in shapes.items()}
            p = C.c_void_p(frames.ctypes.data)
            stride = int(frames.strides[1])
        _check(self.L.mi_tracker_step(self.h, p, W, H, stride, D, *[_ptr(out[k])[0] for k in ("faces", "face_counts", "source", "rois", "landmarks",
                                                                                               "present", "eyes", "det_stream", "n_detect")],
                                      mem, C.c_void_p(stream or 0)))
        if mem == MI_MEM_HOST:
            out["rois"] = out["rois"].view(RECT_DTYPE).reshape(S)
        return out

    def reset(self, stream_index=-1):
        """Drops the state of one stream, or of all (-1; the detect plan then starts at stream 0 again)."""
        _check(self.L.mi_tracker_reset(self.h, int(stream_index)))

    def state(self):
        """-> dict(rois: numpy records of RECT_DTYPE [streams] (zeros for a lost stream), tracked int32 [streams]).  Synchronises."""
        rois, tracked = np.zeros((self.streams,), RECT_DTYPE), np.zeros((self.streams,), np.int32)
        _check(self.L.mi_tracker_get_state(self.h, C.c_void_p(rois.ctypes.data), C.c_void_p(tracked.ctypes.data)))
        return dict(rois=rois, tracked=tracked)

    def set_state(self, rois, tracked, first=0):
        """Writes the state of streams first .. first + n - 1: rois (records of RECT_DTYPE [n]), tracked [n].  Synchronises."""
        rois = np.ascontiguousarray(rois, RECT_DTYPE).reshape(-1)
        tracked = np.ascontiguousarray(tracked, np.int32).reshape(-1)
        if rois.size != tracked.size:
            raise ValueError("rois and tracked must have one entry per stream written")
        _check(self.L.mi_tracker_set_state(self.h, int(first), int(tracked.size), C.c_void_p(rois.ctypes.data), C.c_void_p(tracked.ctypes.data)))


def _picture(x, channels, what):
    """(pointer, mem, B, H, W, row stride in bytes) of a batch of pictures: uint8 [B,H,W,channels], numpy or a torch CUDA tensor; rows may be
    padded (a view of a wider buffer) as long as the pixels of a row are dense and frames lie stride * H bytes apart."""
    if x.ndim != 4 or x.shape[3] != channels or str(x.dtype).split(".")[-1] != "uint8":
        raise ValueError("%s must be uint8 [B,H,W,%d]" % (what, channels))
    B, H, W = (int(v) for v in x.shape[:3])
    if _is_torch(x):
        st, mem = [int(v) for v in x.stride()], (MI_MEM_DEVICE if x.is_cuda else MI_MEM_HOST)
        p = C.c_void_p(x.data_ptr())
    else:
        st, mem, p = [int(v) for v in x.strides], MI_MEM_HOST, C.c_void_p(x.ctypes.data)
    if st[3] != 1 or st[2] != channels or (B > 1 and st[0] != st[1] * H):
        raise ValueError("%s: pixels must be dense and frames stride * H bytes apart" % what)
    return p, mem, B, H, W, st[1]


def _render_out(frames, mem, B, H, W, out, out_channels):
    if out is None:
        if mem == MI_MEM_DEVICE:
            import torch
            out = torch.empty((B, H, W, out_channels), dtype=torch.uint8, device=frames.device)
        else:
            out = np.empty((B, H, W, out_channels), np.uint8)
    po, memo, Bo, Ho, Wo, ostride = _picture(out, out_channels, "out")
    if memo != mem or (Bo, Ho, Wo) != (B, H, W):
        raise ValueError("out must live where frames live and have their batch and size")
    return out, po, ostride


def _render_operand(x, mem, device, dtype, what):
    """pointer of an operand that follows `mem` (None stays None); host operands are made contiguous arrays of `dtype`"""
    if x is None:
        return None, None
    if mem == MI_MEM_DEVICE:
        if not (_is_torch(x) and x.is_cuda and x.is_contiguous() and str(x.dtype) == "torch." + dtype):
            raise ValueError("%s must be a contiguous %s CUDA tensor when the frames are" % (what, dtype))
        return C.c_void_p(x.data_ptr()), x
    x = np.ascontiguousarray(x, getattr(np, dtype))
    return C.c_void_p(x.ctypes.data), x


def _skipped_buffer(mem, B, frames):
    if mem == MI_MEM_DEVICE:
        import torch
        return torch.zeros((B,), dtype=torch.int32, device=frames.device)
    return np.zeros((B,), np.int32)


def render_annotations(frames, annotations, coords, out=None, out_channels=4, device=0, stream=None):
    """render_to_image (render.rs:361-479) over a batch, on the GPU: frames uint8 [B,H,W,3] (numpy or a torch CUDA tensor), `annotations` a
    sequence of Annotation (the same list for every frame), coords float64 [B, coords_per_frame] in the memory of the frames.  out: None (a new
    [B,H,W,out_channels] picture), a buffer of that shape, or `frames` itself with out_channels 3 (in place).
    -> (out, skipped int32 [B]: rectangles of size zero and lines beyond 2^20 px that were not drawn, see include/mi_face.h)."""
    p, mem, B, H, W, stride = _picture(frames, 3, "frames")
    if mem == MI_MEM_DEVICE:
        _device_ready(frames, device, None, "uint8")
    out, po, ostride = _render_out(frames, mem, B, H, W, out, out_channels)
    pc, coords = _render_operand(coords, mem, device, "float64", "coords")
    per_frame = int(coords.shape[1]) if coords is not None and coords.ndim == 2 and int(coords.shape[0]) == B else -1
    if coords is not None and per_frame < 0:
        raise ValueError("coords must be [B, coords_per_frame]")
    anns = (Annotation * max(len(annotations), 1))(*annotations)
    skipped = _skipped_buffer(mem, B, frames)
    _check(lib().mi_render_annotations(device, p, B, W, H, stride, anns, len(annotations), pc, max(per_frame, 0), po, out_channels, ostride,
                                       _ptr(skipped)[0], mem, C.c_void_p(stream or 0)))
    return out, skipped


def render_faces(frames, faces=None, face_counts=None, landmarks=None, present=None, eyes=None, style=None, out=None, out_channels=4, device=0,
                 stream=None):
    """detections_to_render_data + face_landmarks_to_render_data + eye_landmarks_to_render_data + render_to_image (lib.rs:42-83) on what
    Pipeline.run / FaceDetection.infer_images returned, in the memory they returned it in: faces float32 [B,17] or [B,F,17] with face_counts
    int32 [B], landmarks float32 [B,468,3] and eyes float32 [B,2,76,3] with present int32 [B]; any group may be None.  style: RenderStyle.
    With CUDA tensors nothing visits the host, and with a caller stream the call is asynchronous.  -> (out, skipped int32 [B])."""
    p, mem, B, H, W, stride = _picture(frames, 3, "frames")
    if mem == MI_MEM_DEVICE:
        _device_ready(frames, device, None, "uint8")
    out, po, ostride = _render_out(frames, mem, B, H, W, out, out_channels)
    per_frame = 0
    if faces is not None:
        per_frame = 1 if faces.ndim == 2 else int(faces.shape[1])
        if int(faces.shape[0]) != B or int(faces.shape[-1]) != 17 or face_counts is None:
            raise ValueError("faces must be [B,17] or [B,F,17] and come with face_counts [B]")
    for x, shape, what in ((landmarks, (B, NUM_FACE_LANDMARKS, 3), "landmarks"), (eyes, (B, 2, NUM_EYE_LANDMARKS + NUM_IRIS_LANDMARKS, 3), "eyes"),
                           (face_counts, (B,), "face_counts"), (present, (B,), "present")):
        if x is not None and tuple(int(v) for v in x.shape) != shape:
            raise ValueError("%s must have shape %s" % (what, list(shape)))
    pf, faces = _render_operand(faces, mem, device, "float32", "faces")
    pn, face_counts = _render_operand(face_counts, mem, device, "int32", "face_counts")
    pl, landmarks = _render_operand(landmarks, mem, device, "float32", "landmarks")
    pp, present = _render_operand(present, mem, device, "int32", "present")
    pe, eyes = _render_operand(eyes, mem, device, "float32", "eyes")
    style = style if style is not None else RenderStyle()
    skipped = _skipped_buffer(mem, B, frames)
    _check(lib().mi_render_faces(device, p, B, W, H, stride, pf, pn, per_frame, pl, pp, pe, C.byref(style), po, out_channels, ostride,
                                 _ptr(skipped)[0], mem, C.c_void_p(stream or 0)))
    return out, skipped


def render_face_items(frames, result, style=None, out=None, out_channels=4, device=0, stream=None):
    """mi_render_face_items: draws what Pipeline.run_faces returned — `result` is its dict, numpy arrays or CUDA tensors, in the memory of the
    frames: faces [B,F,17] + face_counts [B] (boxes and key points of every frame), then for every item of a frame its mesh, both eyes and both
    irises (iris_landmarks_to_render_data, iris_landmark.rs:330-377) from item_frame [M], counts [2] (only counts[0], the slots used, is read —
    on the device), landmarks [M,468,3], present [M] and eyes [M,2,76,3].  Keys that are missing or None leave their group out.  style:
    RenderItemsStyle.  With CUDA tensors no coordinate or count visits the host, and with a caller stream the call is asynchronous.
    -> (out, skipped int32 [B])."""
    p, mem, B, H, W, stride = _picture(frames, 3, "frames")
    if mem == MI_MEM_DEVICE:
        _device_ready(frames, device, None, "uint8")
    out, po, ostride = _render_out(frames, mem, B, H, W, out, out_channels)
    get = lambda k: result.get(k) if result is not None else None
    faces, face_counts, item_frame, counts = get("faces"), get("face_counts"), get("item_frame"), get("counts")
    landmarks, present, eyes = get("landmarks"), get("present"), get("eyes")
    shape = lambda x: tuple(int(v) for v in x.shape)
    F = 1
    if faces is not None:
        if faces.ndim != 3 or shape(faces)[0] != B or shape(faces)[2] != 17 or face_counts is None:
            raise ValueError("faces must be [B,F,17] and come with face_counts [B]")
        F = shape(faces)[1]
    M = 1
    if item_frame is not None:
        if item_frame.ndim != 1 or counts is None or counts.ndim != 1 or shape(counts)[0] < 1:
            raise ValueError("item_frame must be [M] and come with counts [2] (the slots used first)")
        M = shape(item_frame)[0]
    elif landmarks is not None or eyes is not None:
        raise ValueError("landmarks and eyes need item_frame and counts")
    for x, want, what in ((landmarks, (M, NUM_FACE_LANDMARKS, 3), "landmarks"), (eyes, (M, 2, NUM_EYE_LANDMARKS + NUM_IRIS_LANDMARKS, 3), "eyes"),
                          (face_counts, (B,), "face_counts"), (present, (M,), "present")):
        if x is not None and shape(x) != want:
            raise ValueError("%s must have shape %s" % (what, list(want)))
    pf, faces = _render_operand(faces, mem, device, "float32", "faces")
    pn, face_counts = _render_operand(face_counts if faces is not None else None, mem, device, "int32", "face_counts")
    pi, item_frame = _render_operand(item_frame, mem, device, "int32", "item_frame")
    pc, counts = _render_operand(counts if item_frame is not None else None, mem, device, "int32", "counts")
    pl, landmarks = _render_operand(landmarks, mem, device, "float32", "landmarks")
    pp, present = _render_operand(present if item_frame is not None else None, mem, device, "int32", "present")
    pe, eyes = _render_operand(eyes, mem, device, "float32", "eyes")
    style = style if style is not None else RenderItemsStyle()
    skipped = _skipped_buffer(mem, B, frames)
    _check(lib().mi_render_face_items(device, p, B, W, H, stride, pf, pn, F, pi, pc, M, pl, pp, pe, C.byref(style), po, out_channels, ostride,
                                      _ptr(skipped)[0], mem, C.c_void_p(stream or 0)))
    return out, skipped


FE_CHIP_SIZE = 112   # IMG_SIZE, face_embeddings.rs:20


class FaceEmbeddings:
    """Face embeddings — mirrors face_embeddings.rs:22-109.  The MODEL IS THE CALLER'S: the reference ships no face_embeddings.tflite (its
    README tells users to download one), none is shipped here, and the reference's own model has never been run on this engine.  Any graph
    of the operators the engine lowers that maps [1,112,112,3] to one output of D values per frame loads; `features` is D.  ResNet-style
    (ArcFace) float graphs are among them: dense 3x3 CONV_2D (conv_mfma_kernel on the matrix cores; `model.set_option("conv_mfma", 0)` sends
    them back to the generic kernel), MUL / ADD by per-channel constants, PRELU and a FULLY_CONNECTED head.  Pooled heads load too
    (AVERAGE_POOL_2D, MEAN over H and W, L2_NORMALIZATION, SUB / DIV by a per-channel or scalar constant), and so do ONNX-exported graphs:
    TRANSPOSE by a constant perm that keeps the batch axis, with the channel-first element-wise operators moved onto NHWC tensors at load so
    that the transposes around the convolutions disappear.  Still refused: MUL / SUB / DIV of two tensors, c / x, MEAN over other axes,
    CONCATENATION on the channel axis, LOGISTIC and the other activations, quantised graphs.

    `precision` is the operand precision of those dense k x k convolutions (engine option "conv_bf16"; tensors stay f32 in memory): "f32"
    (default: every bit as without the argument), "bf16" (activations and filter values rounded to bf16, products accumulated in f32 on
    v_mfma_f32_32x32x16_bf16) or "bf16x3" (every operand split into two bf16 values, three products for one: about f32 accuracy)."""

    PRECISIONS = {"f32": 0, "bf16": 1, "bf16x3": 2}

    def __init__(self, model_path=None, device=0, model_bytes=None, precision="f32"):
        if precision not in self.PRECISIONS:   # (before a handle is made)
            raise ValueError("precision must be one of %s, not %r" % (sorted(self.PRECISIONS), precision))
        self.L = lib()
        self.h = C.c_void_p()
        if model_bytes is not None:
            _check(self.L.mi_fe_create_from_bytes(model_bytes, len(model_bytes), device, C.byref(self.h)))
        else:
            # None: the reference's default, "./models/face_embeddings.tflite" relative to the working directory (face_embeddings.rs:36)
            _check(self.L.mi_fe_create(os.fsencode(model_path) if model_path is not None else None, device, C.byref(self.h)))
        self.device = device
        self.model = Model(handle=self.L.mi_fe_model(self.h), owner=self, device=device)
        n = C.c_int()
        _check(self.L.mi_fe_features(self.h, C.byref(n)))
        self.features = n.value
        if self.PRECISIONS[precision]:
            self.model.set_option("conv_bf16", self.PRECISIONS[precision])

    @property
    def precision(self):
        """the operand precision the handle runs at, read back from the engine"""
        value = self.model.get_option("conv_bf16")
        return next(name for name, v in self.PRECISIONS.items() if v == value)

    def close(self):
        if getattr(self, "h", None):
            self.L.mi_fe_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def infer(self, image, bbox, cap=None):
        """FaceEmbeddings::infer(&Mat, BBox) -> float32 [1, D], l2-normalised: bbox = (xmin, ymin, xmax, ymax) in absolute pixels (what the
        reference's test passes: faces[0].bbox().scale(size)).  MiError (MI_ERANGE) where the reference panics: a box that leaves the image."""
        image, w, h, stride = _image_args(image)
        box = (C.c_double * 4)(*[float(v) for v in bbox])
        cap = self.features if cap is None else int(cap)
        out = np.zeros((1, max(cap, 1)), np.float32)
        _check(self.L.mi_fe_infer_image(self.h, C.c_void_p(image.ctypes.data), w, h, stride, box, C.c_void_p(out.ctypes.data), cap))
        return out[:, :self.features]

    def infer_items(self, frames, result, want_raw=False, want_chips=False, stream=None):
        """mi_fe_infer_face_items on what Pipeline.run_faces returned (`result`: its dict; faces [B,F,17], item_frame [M], item_face [M] are
        read), numpy arrays or CUDA tensors in the memory of the frames.  Returns dict(embeddings [M,D], valid [M]) plus raw [M,D] (the
        network's output before l2_norm) and chips [M,112,112,3] (its input) when asked for; rows of invalid items (unused slots, boxes that
        leave the frame) are zeros.  With CUDA tensors nothing visits the host, and with a caller stream the call is asynchronous."""
        p, mem, B, H, W, stride = _picture(frames, 3, "frames")
        if mem == MI_MEM_DEVICE:
            _device_ready(frames, self.device, None, "uint8")
        faces, item_frame, item_face = result["faces"], result["item_frame"], result["item_face"]
        shape = lambda x: tuple(int(v) for v in x.shape)
        if faces.ndim != 3 or shape(faces)[0] != B or shape(faces)[2] != 17:
            raise ValueError("faces must be [B,F,17]")
        F, M = shape(faces)[1], shape(item_frame)[0]
        if item_frame.ndim != 1 or shape(item_face) != (M,):
            raise ValueError("item_frame and item_face must be [M]")
        if not (1 <= F <= 16 and 1 <= M <= 32767):   # (before the outputs are sized by them; the C entry checks again)
            raise MiError(-1, "max_faces must be 1..16 and max_items 1..32767")   # MI_EINVAL
        pf, faces = _render_operand(faces, mem, self.device, "float32", "faces")
        pi, item_frame = _render_operand(item_frame, mem, self.device, "int32", "item_frame")
        pk, item_face = _render_operand(item_face, mem, self.device, "int32", "item_face")
        D = self.features
        shapes = dict(embeddings=((M, D), "float32"), valid=((M,), "int32"))
        if want_raw:
            shapes["raw"] = ((M, D), "float32")
        if want_chips:
            shapes["chips"] = ((M, FE_CHIP_SIZE, FE_CHIP_SIZE, 3), "float32")
        if mem == MI_MEM_DEVICE:
            import torch
            out = {k: torch.zeros(sh, dtype=getattr(torch, dt), device=frames.device) for k, (sh, dt) in shapes.items()}
            torch.cuda.current_stream(frames.device).synchronize()   # (the zero fills above were queued on torch's stream)
        else:
            out = {k: np.zeros(sh, getattr(np, dt)) for k, (sh, dt) in shapes.items()}
        opt = lambda k: _ptr(out[k])[0] if k in out else None
        _check(self.L.mi_fe_infer_face_items(self.h, p, B, W, H, stride, pf, F, pi, pk, M, _ptr(out["embeddings"])[0], _ptr(out["valid"])[0],
                                             opt("raw"), opt("chips"), mem, C.c_void_p(stream or 0)))
        return out

    def infer_aligned(self, image, points, source="points", cap=None, want_roi=False):
        """mi_fe_infer_image_aligned — NOT the reference's chip (the reference crops the box: infer()).  `points`: pixel coordinates [5,2] in the
        template's order (face_align_template), or [4,2] with source="detection" (eyes, nose tip, mouth centre); face_align_points gathers them
        from a mesh or a detection.  The least-squares similarity fit to the template, the warp of the WHOLE image by it, the network, l2_norm
        -> float32 [1, D] (with want_roi: (embedding, Rect)).  MiError (MI_ERANGE) for points without a fit."""
        image, w, h, stride = _image_args(image)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        cap = self.features if cap is None else int(cap)
        out = np.zeros((1, max(cap, 1)), np.float32)
        roi = Rect()
        _check(self.L.mi_fe_infer_image_aligned(self.h, C.c_void_p(image.ctypes.data), w, h, stride, C.c_void_p(pts.ctypes.data), int(pts.shape[0]),
                                                _align_source(source), C.c_void_p(out.ctypes.data), cap, C.byref(roi)))
        return (out[:, :self.features], roi) if want_roi else out[:, :self.features]

    def infer_items_aligned(self, frames, result, source="mesh", points=None, point_valid=None, want_raw=False, want_chips=False, want_rois=False,
                            stream=None):
        """mi_fe_infer_aligned_items on what Pipeline.run_faces returned, as it lies in memory — NOT the reference's chips (infer_items is the
        box path).  source "mesh": result's landmarks [M,468,3], present [M] and item_frame [M] are read; "detection": faces [B,F,17], item_frame
        and item_face; "points": `points` float32 [M,5,2] pixel coordinates, `point_valid` int32 [M] or None, and result's item_frame.  Returns
        dict(embeddings [M,D], valid [M]) plus raw [M,D], chips [M,112,112,3] and rois when asked for: a numpy array of RECT_DTYPE [M] for host
        frames, a uint8 CUDA tensor [M,48] holding the same bytes for device frames.  Rows of invalid items are zeros."""
        p, mem, B, H, W, stride = _picture(frames, 3, "frames")
        if mem == MI_MEM_DEVICE:
            _device_ready(frames, self.device, None, "uint8")
        src_id = _align_source(source)
        shape = lambda x: tuple(int(v) for v in x.shape)
        item_frame = result["item_frame"]
        if item_frame.ndim != 1:
            raise ValueError("item_frame must be [M]")
        M, F = shape(item_frame)[0], 1
        pk = pg = None
        if source == "mesh":
            src, gate = result["landmarks"], result["present"]
            if shape(src) != (M, NUM_FACE_LANDMARKS, 3) or shape(gate) != (M,):
                raise ValueError("landmarks must be [M,468,3] and present [M]")
        elif source == "detection":
            src, gate = result["faces"], None
            if src.ndim != 3 or shape(src)[0] != B or shape(src)[2] != 17 or shape(result["item_face"]) != (M,):
                raise ValueError("faces must be [B,F,17] and item_face [M]")
            F = shape(src)[1]
        else:
            src, gate = points, point_valid
            if src is None or shape(src) != (M, 5, 2) or (gate is not None and shape(gate) != (M,)):
                raise ValueError("points must be [M,5,2] and point_valid [M] or None")
        if not (1 <= F <= 16 and 1 <= M <= 32767):   # (before the outputs are sized by them; the C entry checks again)
            raise MiError(-1, "max_faces must be 1..16 and max_items 1..32767")   # MI_EINVAL
        ps, src = _render_operand(src, mem, self.device, "float32", "the source's points")
        pg, gate = _render_operand(gate, mem, self.device, "int32", "the source's gate")
        pi, item_frame = _render_operand(item_frame, mem, self.device, "int32", "item_frame")
        if source == "detection":
            pk, item_face = _render_operand(result["item_face"], mem, self.device, "int32", "item_face")
        D = self.features
        shapes = dict(embeddings=((M, D), "float32"), valid=((M,), "int32"))
        if want_raw:
            shapes["raw"] = ((M, D), "float32")
        if want_chips:
            shapes["chips"] = ((M, FE_CHIP_SIZE, FE_CHIP_SIZE, 3), "float32")
        if want_rois:
            shapes["rois"] = ((M, RECT_DTYPE.itemsize), "uint8")
        if mem == MI_MEM_DEVICE:
            import torch
            out = {k: torch.zeros(sh, dtype=getattr(torch, dt), device=frames.device) for k, (sh, dt) in shapes.items()}
            torch.cuda.current_stream(frames.device).synchronize()   # (the zero fills above were queued on torch's stream)
        else:
            out = {k: np.zeros(sh, getattr(np, dt)) for k, (sh, dt) in shapes.items()}
        opt = lambda k: _ptr(out[k])[0] if k in out else None
        _check(self.L.mi_fe_infer_aligned_items(self.h, p, B, W, H, stride, src_id, ps, pg, F, pi, pk, M, _ptr(out["embeddings"])[0],
                                                _ptr(out["valid"])[0], opt("raw"), opt("chips"), opt("rois"), mem, C.c_void_p(stream or 0)))
        if want_rois and mem == MI_MEM_HOST:
            out["rois"] = out["rois"].view(RECT_DTYPE).reshape(M)
        return out


ALIGN_SOURCES = {"points": 0, "mesh": 1, "detection": 2}   # MI_ALIGN_POINTS / MI_ALIGN_MESH / MI_ALIGN_DETECTION
# mi_rect as it lies in memory (the rois of FaceEmbeddings.infer_items_aligned)
RECT_DTYPE = np.dtype([("x_center", "<f8"), ("y_center", "<f8"), ("width", "<f8"), ("height", "<f8"), ("rotation", "<f8"), ("normalized", "<i4"),
                       ("pad", "<i4")])


def _align_source(source):
    if source not in ALIGN_SOURCES:
        raise ValueError("source must be one of %s, not %r" % (sorted(ALIGN_SOURCES), source))
    return ALIGN_SOURCES[source]


def face_align_template(source="points"):
    """mi_face_align_template (host only): the destination points of the aligned chip, float64 [5,2] in chip pixels (image-left eye,
    image-right eye, nose tip, image-left and image-right mouth corner), or [4,2] for source="detection" (the mouth's centre instead)."""
    xy, n = np.zeros((5, 2), np.float64), C.c_int()
    _check(lib().mi_face_align_template(_align_source(source), C.c_void_p(xy.ctypes.data), C.byref(n)))
    return xy[:n.value].copy()


def face_align_points(source, landmarks_or_detection, image_size):
    """mi_face_align_points (host only): the pixel points of one face, float32 [5,2] from its mesh (source="mesh": landmarks [468,3],
    normalised) or [4,2] from its detection (source="detection": a Detection or 17 floats); image_size = (width, height)."""
    x = landmarks_or_detection
    if isinstance(x, Detection):
        x = np.concatenate([np.asarray(x.data, np.float32).reshape(-1), [np.float32(x.score)]])
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    need = (10, 3 * NUM_FACE_LANDMARKS, 17)[_align_source(source)]
    if x.size != need:
        raise ValueError("source %r takes %d floats, not %d" % (source, need, x.size))
    pts, n = np.zeros((5, 2), np.float32), C.c_int()
    _check(lib().mi_face_align_points(_align_source(source), C.c_void_p(x.ctypes.data), int(image_size[0]), int(image_size[1]),
                                      C.c_void_p(pts.ctypes.data), C.byref(n)))
    return pts[:n.value].copy()


def face_align_roi(points, source="points"):
    """mi_face_align_roi (host only, no GPU): the least-squares similarity fit of pixel `points` ([5,2]; [4,2] for source="detection") to the
    template, as the rotated square Rect whose warp to 112 x 112 is the aligned chip -> (Rect, valid).  An invalid fit (a coordinate that is
    not finite, all points equal) gives the whole-image Rect and valid = False; a wrong number of points is MiError (MI_EINVAL)."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
    roi, valid = Rect(), C.c_int()
    _check(lib().mi_face_align_roi(C.c_void_p(pts.ctypes.data), int(pts.shape[0]), _align_source(source), C.byref(roi), C.byref(valid)))
    return roi, bool(valid.value)


def face_chip_rect(detection, image_size):
    """mi_face_chip_rect (host only, no GPU): the rectangle FaceEmbeddings crops for a detection — `detection` a Detection or 17 floats,
    image_size = (width, height).  -> ((x, y, w, h), valid)."""
    d = CDetection()
    data = np.asarray(detection.data if isinstance(detection, Detection) else detection, np.float32).reshape(-1)
    for i in range(16):
        d.data[i] = data[i]
    rect, valid = (C.c_int * 4)(), C.c_int()
    _check(lib().mi_face_chip_rect(C.byref(d), int(image_size[0]), int(image_size[1]), rect, C.byref(valid)))
    return tuple(rect), bool(valid.value)


def l2_norm(arr):
    """utils::l2_norm (utils.rs:30-33), bit-identical to the reference's order of operations: arr / sqrt(sum arr^2) over ALL elements of
    `arr` (an Array2 in the reference), float32, same shape."""
    a = np.ascontiguousarray(arr, np.float32)
    out = np.zeros_like(a)
    _check(lib().mi_l2_norm(C.c_void_p(a.ctypes.data), int(a.size), C.c_void_p(out.ctypes.data)))
    return out


def similarity_score(a, b):
    """utils::similarity_score (utils.rs:44-50): the cosine of two vectors, all three sums float32 and sequential.  -> numpy float32."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    b = np.ascontiguousarray(b, np.float32).reshape(-1)
    if a.size != b.size:
        raise ValueError("a and b must have the same length")   # (the reference's zip would stop at the shorter one for the dot product only)
    out = C.c_float()
    _check(lib().mi_similarity_score(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), int(a.size), C.byref(out)))
    return np.float32(out.value)


def similarity_matrix(a, b, device=0, stream=None):
    """mi_similarity_matrix: out[i, j] = similarity_score(a[i], b[j]) for a [n, D] against a gallery b [m, D] on the GPU's f32 matrix cores;
    numpy arrays (-> numpy) or CUDA tensors (-> a CUDA tensor; asynchronous with a caller stream).  D 1..4096."""
    if _is_torch(a) and a.is_cuda:
        import torch
        if not (_is_torch(b) and b.is_cuda and a.dim() == 2 and b.dim() == 2 and a.is_contiguous() and b.is_contiguous()):
            raise ValueError("a and b must be contiguous 2-d CUDA tensors")
        _device_ready(a, device)
        _device_ready(b, device)
        mem = MI_MEM_DEVICE
        out = torch.empty((int(a.shape[0]), int(b.shape[0])), dtype=torch.float32, device=a.device)
    else:
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        if a.ndim != 2 or b.ndim != 2:
            raise ValueError("a and b must be [n, D] and [m, D]")
        mem = MI_MEM_HOST
        out = np.empty((a.shape[0], b.shape[0]), np.float32)
    if int(a.shape[1]) != int(b.shape[1]):
        raise ValueError("a and b must have the same number of features")
    _check(lib().mi_similarity_matrix(int(device), _ptr(a)[0], int(a.shape[0]), _ptr(b)[0], int(b.shape[0]), int(a.shape[1]), _ptr(out)[0], mem,
                                      C.c_void_p(stream or 0)))
    return out


TOPK_MAX_K = 16


def topk_select(scores, k):
    """mi_topk_select (host only, no GPU): the selection rule of Gallery.topk applied to a score matrix [n, m] -> (index [n, k] int32,
    score [n, k] float32).  Row j is eligible iff scores[i, j] > -inf (NaN and -inf never are); eligible rows by score descending under the
    plain float32 `>`, ties to the lower j; slots beyond the eligible rows hold -1 / -inf.  k 1..16."""
    s = np.ascontiguousarray(scores, np.float32)
    if s.ndim != 2:
        raise ValueError("scores must be [n, m]")
    k = int(k)
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError("k must be 1..16")
    n, m = s.shape
    index, score = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
    _check(lib().mi_topk_select(C.c_void_p(s.ctypes.data), n, m, k, C.c_void_p(index.ctypes.data), C.c_void_p(score.ctypes.data)))
    return index, score


class Gallery:
    """mi_gallery: enrolled embeddings `rows` [m, D] (numpy, or a CUDA tensor), copied once into device memory the handle owns, with an int
    label per row (None: the label is the row index).  topk() answers "who is this": the k best rows of every query by cosine score, on the
    device, without the [n, m] score matrix ever reaching memory.  m 1..2^24, D 1..4096."""

    def __init__(self, rows, labels=None, device=0):
        self.L, self.device, self.h = lib(), int(device), C.c_void_p()
        if _is_torch(rows) and rows.is_cuda:
            if rows.dim() != 2 or not rows.is_contiguous():
                raise ValueError("rows must be a contiguous 2-d tensor")
            _device_ready(rows, self.device)
        else:
            rows = np.ascontiguousarray(rows, np.float32)
            if rows.ndim != 2:
                raise ValueError("rows must be [m, D]")
        m, D = int(rows.shape[0]), int(rows.shape[1])
        lab = None
        if labels is not None:
            lab = np.ascontiguousarray(labels, np.int32)
            if lab.shape != (m,):
                raise ValueError("labels must be [m]")
        p, mem = _ptr(rows)
        _check(self.L.mi_gallery_create(self.device, p, m, D, C.c_void_p(lab.ctypes.data) if lab is not None else None, mem, C.byref(self.h)))
        self.m, self.features = m, D

    def close(self):
        if getattr(self, "h", None):
            self.L.mi_gallery_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        """"splits": the column ranges a row of query tiles is spread over (0 = automatic, the default; otherwise 1..64, clamped to the
        number of 128-column tiles).  The results do not depend on it."""
        _check(self.L.mi_gallery_set_option(self.h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int()
        _check(self.L.mi_gallery_get_option(self.h, key.encode(), C.byref(v)))
        return v.value

    def topk(self, queries, k=1, stream=None):
        """mi_gallery_topk: queries [n, D] -> (index [n, k] int32, score [n, k] float32, label [n, k] int32).  score[i, r] is bit for bit
        what similarity_matrix gives at [i, index[i, r]]; the selection is topk_select's.  numpy in -> numpy out; a CUDA tensor in (for
        instance the embeddings of FaceEmbeddings.infer_face_items as they lie there: invalid items come out all -1) -> CUDA tensors,
        asynchronous with a caller stream."""
        k = int(k)
        if not 1 <= k <= TOPK_MAX_K:
            raise ValueError("k must be 1..16")
        if _is_torch(queries) and queries.is_cuda:
            import torch
            if queries.dim() != 2 or not queries.is_contiguous():
                raise ValueError("queries must be a contiguous 2-d CUDA tensor")
            _device_ready(queries, self.device)
            empty = lambda dtype: torch.empty((int(queries.shape[0]), k), dtype=dtype, device=queries.device)
            kinds = (torch.int32, torch.float32, torch.int32)
        else:
            queries = np.ascontiguousarray(queries, np.float32)
            if queries.ndim != 2:
                raise ValueError("queries must be [n, D]")
            empty = lambda dtype: np.empty((queries.shape[0], k), dtype)
            kinds = (np.int32, np.float32, np.int32)
        if int(queries.shape[1]) != self.features:
            raise ValueError("queries must have the gallery's %d features" % self.features)
        if int(queries.shape[0]) < 1:
            raise ValueError("queries must hold at least one row")
        index, score, label = (empty(t) for t in kinds)
        p, mem = _ptr(queries)
        _check(self.L.mi_gallery_topk(self.h, p, int(queries.shape[0]), k, _ptr(index)[0], _ptr(score)[0], _ptr(label)[0], mem, C.c_void_p(stream or 0)))
        return index, score, label


def _pipeline_submit_jpeg(self, slot, im_bytes):
    """lib.rs:18-40 for a stream of encoded pictures: Huffman decoding of this picture happens in this call (on this thread, beside the device's work
    on the other slot's picture); the decoder's sample arithmetic and the three stages are queued.  `collect_jpeg(slot)` returns the results."""
    _check(self.L.mi_pipeline_submit_jpeg(self.h, slot, im_bytes, len(im_bytes)))


def _pipeline_collect_jpeg(self, slot):
    """-> dict(faces [1,17], face_counts [1], landmarks [1,468,3], present [1], eyes [1,2,76,3], size (w, h)) of the picture submitted to `slot`."""
    out = dict(faces=np.zeros((1, 17), np.float32), face_counts=np.zeros((1,), np.int32), landmarks=np.zeros((1, 468, 3), np.float32),
               present=np.zeros((1,), np.int32), eyes=np.zeros((1, 2, 76, 3), np.float32))
    w, h = C.c_int(0), C.c_int(0)
    _check(self.L.mi_pipeline_collect_jpeg(self.h, slot, _ptr(out["faces"])[0], C.cast(_ptr(out["face_counts"])[0], C.POINTER(C.c_int)), _ptr(out["landmarks"])[0],
                                           C.cast(_ptr(out["present"])[0], C.POINTER(C.c_int)), _ptr(out["eyes"])[0], C.byref(w), C.byref(h)))
    out["size"] = (w.value, h.value)
    return out


Pipeline.submit_jpeg = _pipeline_submit_jpeg
Pipeline.collect_jpeg = _pipeline_collect_jpeg


def face_detection_to_roi(face_detection: Detection, image_size, size_mode=None) -> Rect:
    """face_landmark.rs:180-198 (size_mode None = SquareLong, the only mode the reference's callers use)."""
    if size_mode not in (None, 1):
        raise ValueError("only SizeMode::SquareLong is exposed through the C ABI")
    d = CDetection()
    d.data[:] = [float(v) for v in np.asarray(face_detection.data, np.float32).reshape(16)]
    d.score = float(face_detection.score)
    r = Rect()
    _check(lib().mi_face_detection_to_roi(C.byref(d), int(image_size[0]), int(image_size[1]), C.byref(r)))
    return r


def iris_roi_from_face_landmarks(face_landmarks, image_size):
    """iris_landmark.rs:268-292 -> (left_eye_roi, right_eye_roi)."""
    if len(face_landmarks) < NUM_FACE_LANDMARKS:
        raise ValueError("expected 468 face landmarks")
    arr = (CLandmark * NUM_FACE_LANDMARKS)(*[CLandmark(l.x, l.y, l.z) for l in face_landmarks[:NUM_FACE_LANDMARKS]])
    a, b = Rect(), Rect()
    _check(lib().mi_iris_roi_from_face_landmarks(arr, int(image_size[0]), int(image_size[1]), C.byref(a), C.byref(b)))
    return a, b


def bbox_to_roi(bbox, image_size, rotation_keypoints=None, scale=(1.0, 1.0), size_mode=0) -> Rect:
    """transform.rs:44-109.  bbox (xmin, ymin, xmax, ymax) normalised; rotation_keypoints [(x0, y0), (x1, y1)] in pixels;
    size_mode 0 Default, 1 SquareLong, 2 SquareShort."""
    b = (C.c_double * 4)(*[float(v) for v in bbox])
    kp = None
    if rotation_keypoints is not None and len(rotation_keypoints) >= 2:   # fewer than two keypoints: rotation 0 (transform.rs:64-66)
        kp = (C.c_double * 4)(*[float(v) for p in rotation_keypoints[:2] for v in p])
    r = Rect()
    _check(lib().mi_bbox_to_roi(b, int(image_size[0]), int(image_size[1]), kp, float(scale[0]), float(scale[1]), int(size_mode), C.byref(r)))
    return r


def bbox_from_landmarks(landmarks):
    """transform.rs:146-165 -> (xmin, ymin, xmax, ymax)."""
    arr = (CLandmark * max(len(landmarks), 1))(*[CLandmark(l.x, l.y, l.z) for l in landmarks])
    out = (C.c_double * 4)()
    _check(lib().mi_bbox_from_landmarks(arr, len(landmarks), out))
    return tuple(out)


def jpeg_info(im_bytes: bytes):
    """(width, height) of a JPEG stream (headers only; works without a GPU)."""
    w, h = C.c_int(), C.c_int()
    _check(lib().mi_jpeg_info(im_bytes, len(im_bytes), C.byref(w), C.byref(h)))
    return w.value, h.value


def convert_image_to_mat(im_bytes: bytes, device=0, to_device=False):
    """utils.rs:8-21: encoded JPEG bytes -> 8UC3 RGB image [H, W, 3] u8 (numpy; a torch CUDA tensor with to_device=True,
    in which case the pixels never visit the host: Huffman decoding on the CPU, everything after it on the GPU)."""
    w, h = jpeg_info(im_bytes)
    ow, oh = C.c_int(), C.c_int()
    if to_device:
        import torch
        out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:%d" % device)
        _check(lib().mi_jpeg_decode_rgb(device, im_bytes, len(im_bytes), C.c_void_p(out.data_ptr()), out.numel(), C.byref(ow), C.byref(oh), MI_MEM_DEVICE, None))
        return out
    out = np.empty((h, w, 3), np.uint8)
    _check(lib().mi_jpeg_decode_rgb(device, im_bytes, len(im_bytes), C.c_void_p(out.ctypes.data), out.size, C.byref(ow), C.byref(oh), MI_MEM_HOST, None))
    return out


def update_face_landmarks_with_iris_results(face_landmarks, iris_data_left, iris_data_right):
    """iris_landmark.rs:380-398: the eye-contour landmarks of both eyes replace the face-mesh points they refine."""
    if len(face_landmarks) != NUM_FACE_LANDMARKS:
        raise MiError(-1, "unexpected number of items in face_landmarks")
    pack = lambda v: (CLandmark * len(v))(*[CLandmark(l.x, l.y, l.z) for l in v])
    if len(iris_data_left.contour) != NUM_EYE_LANDMARKS or len(iris_data_right.contour) != NUM_EYE_LANDMARKS:
        raise MiError(-1, "expected 71 contour landmarks per eye")
    f, l, r = pack(face_landmarks), pack(iris_data_left.contour), pack(iris_data_right.contour)
    _check(lib().mi_update_face_landmarks_with_iris_results(f, l, r, f))
    return [Landmark(x.x, x.y, x.z) for x in f]


def image_to_tensor(image, roi=None, output_size=None, keep_aspect_ratio=False, output_range=(0., 1.), flip_horizontal=False,
                    device=0):
    """transform::image_to_tensor (transform.rs:188-309) on the GPU -> (tensor [h,w,3] f32 numpy, padding)."""
    image, w, h, stride = _image_args(image)
    ow, oh = output_size
    out = np.zeros((oh, ow, 3), np.float32)
    pad = (C.c_double * 4)()
    _check(lib().mi_image_to_tensor(device, C.c_void_p(image.ctypes.data), w, h, stride, C.byref(roi) if roi is not None else None,
                                    ow, oh, int(keep_aspect_ratio), output_range[0], output_range[1], int(flip_horizontal),
                                    C.c_void_p(out.ctypes.data), pad, MI_MEM_HOST, None))
    return out, tuple(pad)
