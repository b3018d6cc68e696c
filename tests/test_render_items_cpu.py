"""mi_render_face_items without a GPU (include/mi_face.h, section "render.rs"): every refusal comes before any device is touched, the ctypes
mirror of mi_render_items_style has the header's layout, the Python wrapper checks shapes before it calls the library, and the Rust and
C++ mirrors name the entry."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EINVAL, EDEVICE = -1, -4
W, H, B, F, M = 4, 3, 1, 2, 3


def _args(mi):
    """one well-formed host-memory call: keyword -> value, in the order of the C parameters"""
    style = mi.RenderItemsStyle(mi.RenderStyle(bounds_color=mi.Colors.GREEN, mesh=True, eyes=True), iris_oval_color=mi.Colors.BLUE,
                                iris_landmark_color=mi.Colors.PINK)
    return dict(device=0, frames=(C.c_uint8 * (3 * W * H))(), batch=B, width=W, height=H, stride=3 * W,
                faces=(C.c_float * (17 * B * F))(), face_counts=(C.c_int * B)(), max_faces=F,
                item_frame=(C.c_int * M)(), n_items=(C.c_int * 2)(), max_items=M,
                landmarks=(C.c_float * (M * 468 * 3))(), present=(C.c_int * M)(), eyes=(C.c_float * (M * 2 * 76 * 3))(),
                style=C.byref(style), out=(C.c_uint8 * (4 * W * H))(), out_channels=4, out_stride=4 * W, skipped=None, mem=mi.MI_MEM_HOST,
                stream=None, _keep=style)


def _call(mi, **changes):
    a = _args(mi)
    a.update(changes)
    a.pop("_keep")
    return mi.lib().mi_render_face_items(*a.values())


def test_render_face_items_refuses_bad_arguments_without_gpu(mi):
    frames = (C.c_uint8 * 64)()
    no_oval = mi.RenderItemsStyle(iris_landmark_color=mi.Colors.PINK)
    oval = mi.RenderItemsStyle(iris_oval_color=mi.Colors.BLUE)
    cases = {
        # the checks of mi_render_faces
        "null frames": _call(mi, frames=None),
        "null out": _call(mi, out=None),
        "null style": _call(mi, style=None),
        "batch 0": _call(mi, batch=0),
        "width 0": _call(mi, width=0),
        "stride < 3 * width": _call(mi, stride=3 * W - 1),
        "out_channels 2": _call(mi, out_channels=2),
        "out_channels 5": _call(mi, out_channels=5),
        "out_stride < channels * width": _call(mi, out_stride=4 * W - 1),
        "aliasing with out_channels 4": _call(mi, frames=frames, out=frames),
        "in place with another stride": _call(mi, frames=frames, out=frames, out_channels=3, out_stride=3 * W + 4),
        "overlap that is not in place": _call(mi, frames=frames, out=C.byref(frames, 8), out_channels=3, out_stride=3 * W),
        "mem 2": _call(mi, mem=2),
        "faces without face_counts": _call(mi, face_counts=None),
        # the item list
        "max_faces 0": _call(mi, max_faces=0),
        "max_faces 17": _call(mi, max_faces=17),
        "max_items 0": _call(mi, max_items=0),
        "max_items 32768": _call(mi, max_items=32768),
        "item_frame without n_items": _call(mi, n_items=None),
        "n_items without item_frame": _call(mi, item_frame=None),
        "landmarks without the item list": _call(mi, item_frame=None, n_items=None, eyes=None),
        "eyes without the item list": _call(mi, item_frame=None, n_items=None, landmarks=None),
        # iris_landmark.rs:342-344
        "oval on a picture one pixel wide": _call(mi, width=1, stride=3, out_stride=4, style=C.byref(oval)),
        "oval on a picture one pixel high": _call(mi, height=1, style=C.byref(oval)),
    }
    assert cases == {k: EINVAL for k in cases}, cases
    assert mi.lib().mi_last_error()
    if mi.device_count() == 0:      # what the contract allows gets as far as the device, and there is no CPU fallback
        allowed = {
            "a well-formed call": _call(mi),
            "no detections (max_faces is then not looked at)": _call(mi, faces=None, face_counts=None, max_faces=0),
            "no item list": _call(mi, item_frame=None, n_items=None, landmarks=None, eyes=None),
            "no present": _call(mi, present=None),
            "no landmarks, no eyes": _call(mi, landmarks=None, eyes=None),
            "one pixel wide without the oval": _call(mi, width=1, stride=3, out_stride=4, style=C.byref(no_oval)),
            "max_items 32767": _call(mi, max_items=32767, landmarks=None, eyes=None, present=None, item_frame=(C.c_int * 32767)()),
        }
        assert allowed == {k: EDEVICE for k in allowed}, allowed


def test_render_items_style_has_the_header_layout(mi, tmp_path):
    names = [f[0] for f in mi.RenderItemsStyle._fields_]
    assert names == ["base", "draw_iris_oval", "iris_oval_color", "draw_iris_points", "iris_landmark_color", "iris_thickness"]
    prints = '  printf("%d ", (int)sizeof(mi_render_items_style));\n' + "".join(
        '  printf("%%d ", (int)offsetof(mi_render_items_style, %s));\n' % f for f in names)
    src = tmp_path / "layout.c"
    src.write_text('#include "mi_face.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n%s'
                   '  printf("%%d\\n", (int)sizeof(mi_render_style));\n  return 0;\n}\n' % prints)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    cls = mi.RenderItemsStyle
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f in names] + [C.sizeof(mi.RenderStyle)]
    # the constructor: a colour of None is a group that is not drawn, the thickness defaults to the reference's 1.0 (iris_landmark.rs:335)
    s = cls()
    assert (s.draw_iris_oval, s.draw_iris_points, s.iris_thickness) == (0, 0, 1.0)
    s = cls(mi.RenderStyle(mesh=True, mesh_thickness=3.0), iris_oval_color=mi.Colors.BLUE, iris_landmark_color=mi.Color(1, 2, 3, 4), iris_thickness=2.5)
    assert (s.draw_iris_oval, s.draw_iris_points, s.iris_thickness) == (1, 1, 2.5)
    assert s.iris_oval_color.as_tuple() == (0, 0, 255, 255) and s.iris_landmark_color.as_tuple() == (1, 2, 3, 4)
    assert s.base.draw_mesh == 1 and s.base.mesh_thickness == 3.0


def test_python_wrapper_checks_shapes_before_the_library_is_called(mi):
    frames = np.zeros((2, 3, 4, 3), np.uint8)
    good = dict(faces=np.zeros((2, 2, 17), np.float32), face_counts=np.zeros(2, np.int32), item_frame=np.zeros(5, np.int32),
                counts=np.zeros(2, np.int32), landmarks=np.zeros((5, 468, 3), np.float32), present=np.zeros(5, np.int32),
                eyes=np.zeros((5, 2, 76, 3), np.float32))
    bad = [
        dict(good, faces=np.zeros((2, 17), np.float32)),                # the item entry takes [B,F,17] only
        dict(good, faces=np.zeros((3, 2, 17), np.float32)),
        dict(good, face_counts=None),
        dict(good, face_counts=np.zeros(3, np.int32)),
        dict(good, landmarks=np.zeros((4, 468, 3), np.float32)),
        dict(good, landmarks=np.zeros((5, 400, 3), np.float32)),
        dict(good, eyes=np.zeros((5, 2, 71, 3), np.float32)),
        dict(good, present=np.zeros(4, np.int32)),
        dict(good, counts=None),
        dict(good, item_frame=None),
        dict(good, item_frame=np.zeros((5, 1), np.int32)),
    ]
    for result in bad:
        with pytest.raises(ValueError):
            mi.render_face_items(frames, result)
    with pytest.raises(ValueError):
        mi.render_face_items(frames[..., :2], good)
    with pytest.raises(ValueError):
        mi.render_face_items(frames, good, out=np.zeros((2, 3, 4, 3), np.uint8), out_channels=4)
    if mi.device_count() == 0:      # a well-formed call passes every check and stops at the device
        with pytest.raises(mi.MiError) as e:
            mi.render_face_items(frames, good)
        assert e.value.code == EDEVICE


def test_rust_shim_names_the_entry():
    src = os.path.join(ROOT, "bindings", "rust", "src")
    ffi = open(os.path.join(src, "ffi.rs")).read()
    assert "pub fn mi_render_face_items(" in ffi
    body = ffi[ffi.index("pub struct mi_render_items_style {"):].split("}")[0]
    import rs_face_detection_tflite_amd as mi
    assert re.findall(r"pub (\w+):", body) == [f[0] for f in mi.RenderItemsStyle._fields_]
    render_rs = open(os.path.join(src, "render.rs")).read()
    for name in ("ffi::mi_render_face_items(", "pub fn render_face_items(", "pub fn iris_landmarks_to_render_data("):
        assert name in render_rs, name
    lib_rs = open(os.path.join(src, "lib.rs")).read()
    assert "render_face_items" in lib_rs and "iris_landmarks_to_render_data" in lib_rs


def test_cpp_mirror_of_the_entry_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "mi_face.hpp"\n'
                   'int main() {\n'
                   '    std::vector<std::uint8_t> px(36, 0), out(48);\n'
                   '    std::vector<int> item_frame(2, -1), n_items(2, 0);\n'
                   '    mi_render_items_style st{};\n'
                   '    st.draw_iris_oval = 1;\n'
                   '    st.iris_oval_color = mi_face::Colors::BLUE;\n'
                   '    st.iris_thickness = 1.0;\n'
                   '    try {\n'
                   '        mi_face::render_face_items(px.data(), 1, 4, 3, 12, nullptr, nullptr, 0, item_frame.data(), n_items.data(), 2, nullptr, nullptr,\n'
                   '                                   nullptr, st, out.data(), 4, 16);\n'
                   '    } catch (const mi_face::Error&) {\n'
                   '    }\n'
                   '    return 0;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])
