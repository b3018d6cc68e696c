"""mi_face_items_layout — the host statement of the item list mi_pipeline_run_faces builds on the device (both go through
csrc/face_items.hpp) — against a restatement of the rule in numpy, its argument checks, and the presence of the two new entries in
the library, the C header, the C++ mirror and the Rust shim.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

MI_EINVAL = -1


def _rule(counts, max_faces, max_items):
    """include/mi_face.h, mi_pipeline_run_faces: frames in order, each with its first n_b = min(max(count, 0), max_faces) faces."""
    n = np.minimum(np.maximum(np.asarray(counts, np.int64), 0), max_faces)
    frame = np.repeat(np.arange(len(n)), n)
    face = np.concatenate([np.arange(k) for k in n]) if len(n) else np.zeros(0, np.int64)
    used = min(len(frame), max_items)
    item_frame, item_face = np.full(max_items, -1, np.int32), np.full(max_items, -1, np.int32)
    item_frame[:used], item_face[:used] = frame[:used], face[:used]
    return item_frame, item_face, used, len(frame) - used


_RS = np.random.RandomState(7)
CASES = {
    "zeros_negatives_and_beyond_max_faces": ([2, 0, -1, 9, 1, 0, 4, 5, -3, 3], 4),
    "batch_of_one": ([3], 4),
    "batch_of_one_without_a_face": ([0], 2),
    "no_face_anywhere": ([0, -1, 0, 0], 3),
    "max_faces_one": ([5, 1, 0, 2], 1),
    "max_faces_sixteen": ([20, 16, 15, 0, 1], 16),
    "700_frames_more_than_one_scan_chunk": (_RS.randint(-2, 7, 700).tolist(), 4),
    "257_frames_all_full": ([3] * 257, 3),
}


@pytest.mark.parametrize("case", list(CASES))
def test_layout_follows_the_rule(mi, case):
    counts, max_faces = CASES[case]
    total = int(np.minimum(np.maximum(np.asarray(counts), 0), max_faces).sum())
    budgets = sorted({1, max(total - 1, 1), max(total, 1), total + 1, total + 37, max(total // 2, 1)})   # smaller than, equal to and larger than the total
    for max_items in budgets:
        want = _rule(counts, max_faces, max_items)
        got = mi.face_items_layout(counts, max_faces, max_items)
        np.testing.assert_array_equal(got[0], want[0], err_msg="item_frame, budget %d" % max_items)
        np.testing.assert_array_equal(got[1], want[1], err_msg="item_face, budget %d" % max_items)
        assert got[2:] == want[2:], (max_items, got[2:], want[2:])
        assert got[2] == min(total, max_items) and got[3] == total - got[2]


def test_layout_refuses_bad_arguments(mi):
    L = mi.lib()
    counts = (ctypes.c_int * 3)(1, 2, 0)
    fr, fa, n = (ctypes.c_int * 8)(), (ctypes.c_int * 8)(), (ctypes.c_int * 2)()
    call = lambda c, batch, max_faces, max_items, a, b, d: L.mi_face_items_layout(c, batch, max_faces, max_items, a, b, d)
    assert call(counts, 3, 4, 8, fr, fa, n) == 0 and list(n) == [3, 0]
    for max_faces in (0, 17, -1):
        assert call(counts, 3, max_faces, 8, fr, fa, n) == MI_EINVAL
        assert "max_faces" in L.mi_last_error().decode()
    for max_items in (0, -5, (1 << 20) + 1):
        assert call(counts, 3, 4, max_items, fr, fa, n) == MI_EINVAL
        assert "max_items" in L.mi_last_error().decode()
    assert call(counts, 0, 4, 8, fr, fa, n) == MI_EINVAL
    for args in ((None, 3, 4, 8, fr, fa, n), (counts, 3, 4, 8, None, fa, n), (counts, 3, 4, 8, fr, None, n), (counts, 3, 4, 8, fr, fa, None)):
        assert call(*args) == MI_EINVAL
        assert "null" in L.mi_last_error().decode()
    with pytest.raises(mi.MiError) as e:
        mi.face_items_layout([1, 2], 17, 4)
    assert e.value.code == MI_EINVAL


def test_run_faces_refuses_bad_arguments_before_touching_the_device(mi):
    """The argument checks of mi_pipeline_run_faces come before any use of the handle or the device: a null handle is MI_EINVAL."""
    L = mi.lib()
    buf = (ctypes.c_int * 64)()
    rc = L.mi_pipeline_run_faces(None, buf, 1, 4, 4, 12, 4, 4, buf, buf, buf, buf, buf, buf, buf, buf, mi.MI_MEM_HOST, None)
    assert rc == MI_EINVAL and "null" in L.mi_last_error().decode()
    # the launches take 2 * max_items eyes, one per grid row (at most 65535): a larger budget is refused up front, not by a failed launch
    for max_items in (32768, 1 << 20, 0):
        rc = L.mi_pipeline_run_faces(None, buf, 1, 4, 4, 12, 4, max_items, buf, buf, buf, buf, buf, buf, buf, buf, mi.MI_MEM_HOST, None)
        assert rc == MI_EINVAL and "max_items" in L.mi_last_error().decode()


def test_new_entries_are_exported_and_declared_everywhere(mi):
    L = mi.lib()
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    header, hpp, ffi = read("include", "mi_face.h"), read("include", "mi_face.hpp"), read("bindings", "rust", "src", "ffi.rs")
    for name in ("mi_pipeline_run_faces", "mi_face_items_layout"):
        assert hasattr(L, name), "libmiface.so does not export %s" % name
        assert name in mi.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), "%s is not declared in mi_face.h" % name
        assert re.search(r"\b%s\s*\(" % name, hpp), "%s is not used by mi_face.hpp" % name
        assert re.search(r"pub fn %s\s*\(" % name, ffi), "%s is not declared in ffi.rs" % name
    assert "batched plan" in header[header.index("mi_pipeline_run_faces") - 3000:header.index("mi_pipeline_run_faces")]   # no single-launch plan: stated
    assert hasattr(mi.Pipeline, "run_faces") and callable(mi.face_items_layout)
    lib_rs = read("bindings", "rust", "src", "lib.rs")
    assert "pub mod pipeline;" in lib_rs and "run_faces" in read("bindings", "rust", "src", "pipeline.rs")
