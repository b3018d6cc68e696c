"""The renderer's C ABI without a GPU (include/mi_face.h, section "render.rs"): arguments are refused before any device is touched, the
ctypes mirrors have the header's layouts, the connection tables restated in the product source are the reference's, and the Rust shim
names the new entries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

EINVAL = -1


def _call(mi, frames, anns, coords, out, width=4, height=3, stride=12, channels=4, out_stride=None, per_frame=None, batch=1):
    L = mi.lib()
    arr = (mi.Annotation * max(len(anns), 1))(*anns)
    return L.mi_render_annotations(0, frames, batch, width, height, stride, arr, len(anns), coords, len(coords) if per_frame is None else per_frame,
                                   out, channels, channels * width if out_stride is None else out_stride, None, mi.MI_MEM_HOST, None)


def test_render_entries_refuse_bad_arguments_without_gpu(mi):
    L = mi.lib()
    frames = (C.c_uint8 * 64)()
    out = (C.c_uint8 * 64)()
    coords = (C.c_double * 8)()
    ok = [mi.Annotation(mi.ANN_LINES, 0, 2, 1.0, mi.Colors.RED, True)]
    cases = {
        "kind": _call(mi, frames, [mi.Annotation(4, 0, 1)], coords, out),
        "negative kind": _call(mi, frames, [mi.Annotation(-1, 0, 1)], coords, out),
        "first + count beyond coords_per_frame": _call(mi, frames, [mi.Annotation(mi.ANN_LINES, 4, 2)], coords, out),
        "points beyond coords_per_frame": _call(mi, frames, [mi.Annotation(mi.ANN_POINTS, 0, 5)], coords, out),
        "negative count": _call(mi, frames, [mi.Annotation(mi.ANN_POINTS, 0, -1)], coords, out),
        "out_channels 2": _call(mi, frames, ok, coords, out, channels=2),
        "out_channels 5": _call(mi, frames, ok, coords, out, channels=5),
        "aliasing with out_channels 4": _call(mi, frames, ok, coords, frames, channels=4),
        "overlap that is not in place": _call(mi, frames, ok, coords, C.byref(frames, 8), channels=3, out_stride=12),
        "in place with another stride": _call(mi, frames, ok, coords, frames, channels=3, out_stride=16),
        "stride < 3 * width": _call(mi, frames, ok, coords, out, stride=11),
        "out_stride < channels * width": _call(mi, frames, ok, coords, out, out_stride=15),
        "null frames": _call(mi, None, ok, coords, out),
        "null coords": _call(mi, frames, ok, None, out, per_frame=8),
        "batch 0": _call(mi, frames, ok, coords, out, batch=0),
    }
    assert cases == {k: EINVAL for k in cases}, cases
    assert L.mi_last_error()
    style = mi.RenderStyle(bounds_color=mi.Colors.GREEN)
    faces = (C.c_float * 17)()
    counts = (C.c_int * 1)()
    rf = lambda **kw: L.mi_render_faces(0, kw.get("frames", frames), 1, 4, 3, kw.get("stride", 12), faces, kw.get("counts", counts), kw.get("per_frame", 1),
                                        None, None, None, kw.get("style", C.byref(style)), kw.get("out", out), kw.get("channels", 4),
                                        kw.get("out_stride", 16), None, mi.MI_MEM_HOST, None)
    assert rf(channels=1) == EINVAL and rf(out=frames) == EINVAL and rf(stride=11) == EINVAL and rf(style=None) == EINVAL
    assert rf(counts=None) == EINVAL and rf(per_frame=0) == EINVAL and rf(out_stride=12) == EINVAL
    if mi.device_count() == 0:      # well-formed calls get as far as the device, and there is no CPU fallback
        assert _call(mi, frames, ok, coords, out) == -4 and rf() == -4


def test_ctypes_mirrors_have_the_header_layouts(mi, tmp_path):
    fields = {"mi_color": ["r", "g", "b", "a"], "mi_annotation": [f[0] for f in mi.Annotation._fields_],
              "mi_render_style": [f[0] for f in mi.RenderStyle._fields_]}
    prints = "".join('  printf("%%d ", (int)sizeof(%s));\n' % s + "".join('  printf("%%d ", (int)offsetof(%s, %s));\n' % (s, f) for f in fs)
                     for s, fs in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include "mi_face.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  mi_color red = MI_COLOR_RED;\n%s'
                   '  printf("%%d %%d %%d %%d\\n", red.r, red.g, red.b, red.a);\n  return 0;\n}\n' % prints)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for cls in (mi.Color, mi.Annotation, mi.RenderStyle):
        want += [C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
    assert got == want + [255, 0, 0, 255]
    assert [c.as_tuple() for c in (mi.Colors.BLACK, mi.Colors.RED, mi.Colors.GREEN, mi.Colors.BLUE, mi.Colors.PINK, mi.Colors.WHITE)] == \
        [(0, 0, 0, 255), (255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255), (255, 0, 255, 255), (255, 255, 255, 255)]     # render.rs:28-68


def test_connection_tables_in_the_kernel_source_are_the_reference_s():
    from oracle import render
    src = open(os.path.join(ROOT, "rs-face-detection-tflite_amd", "csrc", "render_kernels.hip")).read()
    table = lambda name: [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", re.search(name + r"\[\d+\]\[2\] = \{(.*?)\n\};", src, flags=re.S).group(1))]
    assert table("kFaceConnections") == list(render.FACE_LANDMARK_CONNECTIONS)
    assert table("kEyeConnections") == list(render.EYE_LANDMARK_CONNECTIONS)


def test_rust_shim_names_the_render_entries():
    src = os.path.join(ROOT, "bindings", "rust", "src")
    ffi = open(os.path.join(src, "ffi.rs")).read()
    for name in ("mi_render_annotations", "mi_render_faces", "pub struct mi_color", "pub struct mi_annotation", "pub struct mi_render_style"):
        assert name in ffi, name
    body = lambda name: ffi[ffi.index("pub struct %s {" % name):].split("}")[0]
    import rs_face_detection_tflite_amd as mi
    assert re.findall(r"pub (\w+):", body("mi_annotation")) == [f[0] for f in mi.Annotation._fields_]
    assert re.findall(r"pub (\w+):", body("mi_render_style")) == [f[0] for f in mi.RenderStyle._fields_]
    render_rs = open(os.path.join(src, "render.rs")).read()
    assert "never compiled" in render_rs.lower().split("\n\n")[0] or "uncompiled" in render_rs.lower().split("\n\n")[0]
    for name in ("detections_to_render_data", "landmarks_to_render_data", "render_to_image", "struct Annotation", "struct Colors"):
        assert name in render_rs, name
    assert "pub mod render;" in open(os.path.join(src, "lib.rs")).read()


def test_python_wrappers_check_shapes_before_the_library_is_called(mi):
    import pytest
    frames = np.zeros((2, 3, 4, 3), np.uint8)
    with pytest.raises(ValueError):
        mi.render_annotations(frames[..., :2], [], None)
    with pytest.raises(ValueError):
        mi.render_annotations(frames, [], np.zeros((3, 4)))
    with pytest.raises(ValueError):
        mi.render_faces(frames, faces=np.zeros((2, 17), np.float32))
    with pytest.raises(ValueError):
        mi.render_faces(frames, landmarks=np.zeros((2, 400, 3), np.float32))


def test_cpp_mirror_of_the_render_entries_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "mi_face.hpp"\n'
                   'int main() {\n'
                   '    mi_color c = mi_face::Colors::GREEN;\n'
                   '    std::vector<std::uint8_t> px(36, 0), out(48);\n'
                   '    mi_face::Image im{px.data(), 4, 3, 12};\n'
                   '    std::vector<mi_annotation> a{{MI_ANN_LINES, 0, 1, 1.0, c, 1}};\n'
                   '    mi_render_style st{};\n'
                   '    try {\n'
                   '        mi_face::render_to_image(a, {0.0, 0.0, 1.0, 1.0}, im);\n'
                   '        mi_face::render_faces(px.data(), 1, 4, 3, 12, nullptr, nullptr, 0, nullptr, nullptr, nullptr, st, out.data(), 4, 16);\n'
                   '    } catch (const mi_face::Error&) {\n'
                   '    }\n'
                   '    return 0;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])
