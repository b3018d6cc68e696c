"""mi_topk_select — the host statement of the selection rule mi_gallery_topk applies on the device (both go through topk.hpp) — against a
numpy restatement of the rule, the argument refusals of the gallery entries (all made before a device is looked at), and the new kernels'
resource use: no scratch, two workgroups per CU.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

NEG_INF = np.float32(-np.inf)


def rule(S, k):
    """key = where(S > -inf, S, -inf); stable argsort of -key; the first k; entries whose key is -inf become (-1, -inf)"""
    S = np.asarray(S, np.float32)
    with np.errstate(invalid="ignore"):
        key = np.where(S > NEG_INF, S, NEG_INF)
    order = np.argsort(-key, axis=1, kind="stable")[:, :k]
    score = np.take_along_axis(key, order, axis=1)
    index = np.where(score > NEG_INF, order, -1).astype(np.int32)
    n, have = S.shape[0], order.shape[1]
    if have < k:   # m < k
        index = np.concatenate([index, np.full((n, k - have), -1, np.int32)], axis=1)
        score = np.concatenate([score, np.full((n, k - have), NEG_INF, np.float32)], axis=1)
    return index, score.astype(np.float32)


def matrices():
    rs = np.random.RandomState(41)
    plain = rs.standard_normal((7, 300)).astype(np.float32)
    ties = plain.copy()
    ties[0, [5, 127, 128, 299]] = 9.0                 # exact ties above everything: index order
    ties[1, :] = 0.25                                 # a whole row of ties
    ties[2, :] = -1.0
    ties[2, [200, 17, 3]] = [np.float32(-0.0), np.float32(0.0), np.float32(-0.0)]   # -0.0 and +0.0 tie: 3, 17, 200
    ties[3, 40:60] = ties[3, 10]                      # a run of ties in the middle of the order
    special = plain.copy()
    special[0, [1, 9]] = np.nan
    special[0, 7] = np.inf
    special[1, :] = np.nan                            # an all-NaN row
    special[2, :] = -np.inf                           # nothing eligible either
    special[3, 5:] = np.nan                           # five eligible rows: fewer than k = 16
    special[3, 2] = -np.inf                           # ... four
    special[4, [0, 299]] = [np.inf, np.inf]
    special[5, ::2] = -np.inf
    few = rs.standard_normal((3, 4)).astype(np.float32)     # m < k
    few[1, 2] = np.nan
    one = np.asarray([[0.5], [np.nan], [-np.inf], [np.inf]], np.float32)   # m = 1
    return {"random_7x300": plain, "ties": ties, "nan_and_infinities": special, "m_below_k": few, "m_is_1": one}


MATRICES = matrices()


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_topk_select_is_the_rule(mi, name, k):
    S = MATRICES[name]
    want_index, want_score = rule(S, k)
    index, score = mi.topk_select(S, k)
    assert index.shape == (S.shape[0], k) and index.dtype == np.int32 and score.dtype == np.float32
    np.testing.assert_array_equal(index, want_index)
    np.testing.assert_array_equal(score.view(np.uint32), want_score.view(np.uint32))


def test_the_cases_are_what_they_claim():
    index, score = rule(MATRICES["ties"], 5)
    assert list(index[0, :4]) == [5, 127, 128, 299] and list(index[1]) == [0, 1, 2, 3, 4] and list(index[2, :3]) == [3, 17, 200]
    assert np.signbit(score[2, 0]) and not np.signbit(score[2, 1])   # the scores are the rows' own: -0.0, +0.0
    index, score = rule(MATRICES["nan_and_infinities"], 16)
    assert index[0, 0] == 7 and (index[1] == -1).all() and (index[2] == -1).all() and np.isneginf(score[1]).all()
    assert list(index[3, :4]) == sorted(index[3, :4], key=lambda j: -MATRICES["nan_and_infinities"][3, j]) and (index[3, 4:] == -1).all()
    assert list(index[4, :2]) == [0, 299]
    assert (rule(MATRICES["m_below_k"], 16)[0][:, 4:] == -1).all() and list(rule(MATRICES["m_is_1"], 1)[0][:, 0]) == [0, -1, -1, 0]


def _refused(mi, rc, *words):
    assert rc == -1, rc   # MI_EINVAL
    msg = mi.lib().mi_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_argument_refusals_without_a_gpu(mi):
    L = mi.lib()
    buf, ibuf = np.zeros(64, np.float32), np.zeros(64, np.int32)
    p, ip = C.c_void_p(buf.ctypes.data), C.c_void_p(ibuf.ctypes.data)
    # mi_topk_select
    _refused(mi, L.mi_topk_select(None, 1, 1, 1, ip, p), "null")
    _refused(mi, L.mi_topk_select(p, 1, 1, 1, None, p), "null")
    _refused(mi, L.mi_topk_select(p, 1, 1, 1, ip, None), "null")
    for k in (0, 17, -1):
        _refused(mi, L.mi_topk_select(p, 1, 4, k, ip, p), "k", "16")
    _refused(mi, L.mi_topk_select(p, 0, 4, 1, ip, p), "positive")
    _refused(mi, L.mi_topk_select(p, 1, 0, 1, ip, p), "positive")
    # mi_gallery_create: every refusal comes before a device is looked at
    h = C.c_void_p()
    _refused(mi, L.mi_gallery_create(0, None, 1, 4, None, 0, C.byref(h)), "null")
    _refused(mi, L.mi_gallery_create(0, p, 1, 4, None, 0, None), "null")
    for m in (0, -1, (1 << 24) + 1):
        _refused(mi, L.mi_gallery_create(0, p, m, 4, None, 0, C.byref(h)), "m", "2^24")
    for features in (0, 4097):
        _refused(mi, L.mi_gallery_create(0, p, 1, features, None, 0, C.byref(h)), "features", "4096")
    for mem in (2, -1):
        _refused(mi, L.mi_gallery_create(0, p, 1, 4, None, mem, C.byref(h)), "mem")
    assert h.value is None
    # the entries that take a handle
    m_, f_, v = C.c_int(), C.c_int(), C.c_int()
    _refused(mi, L.mi_gallery_dims(None, C.byref(m_), C.byref(f_)), "null")
    _refused(mi, L.mi_gallery_set_option(None, b"splits", 1), "null")
    _refused(mi, L.mi_gallery_get_option(None, b"splits", C.byref(v)), "null")
    _refused(mi, L.mi_gallery_topk(None, p, 1, 1, ip, p, ip, 0, None), "null")
    L.mi_gallery_free(None)
    if mi.device_count() < 1:   # without a device a well-formed gallery is MI_EDEVICE, and says why
        assert L.mi_gallery_create(0, p, 1, 4, None, 0, C.byref(h)) == -4
        assert "device" in L.mi_last_error().decode()


def test_python_mirror_checks_before_sizing_outputs(mi):
    class NoHandle(mi.Gallery):
        def __init__(self):   # the checks under test come before the handle is used
            self.device, self.features, self.m, self.h = 0, 8, 4, None
    q = np.zeros((2, 8), np.float32)
    for k in (0, 17):
        with pytest.raises(ValueError):
            NoHandle().topk(q, k)
    with pytest.raises(ValueError):
        NoHandle().topk(np.zeros((2, 9), np.float32), 1)
    with pytest.raises(ValueError):
        NoHandle().topk(np.zeros(8, np.float32), 1)
    with pytest.raises(ValueError):
        mi.topk_select(np.zeros((2, 3), np.float32), 17)
    with pytest.raises(ValueError):
        mi.Gallery(np.zeros((4, 8), np.float32), labels=np.zeros(5, np.int32))
    for name in ("mi_topk_select", "mi_gallery_create", "mi_gallery_free", "mi_gallery_dims", "mi_gallery_set_option", "mi_gallery_get_option",
                 "mi_gallery_topk"):
        assert name in mi.EXPORTS and hasattr(mi.lib(), name), name


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_new_kernels_use_no_scratch_and_fit_two_workgroups_per_cu():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    out = os.path.join("/tmp", "isa_check_%d_topk.s" % os.getpid())
    isa_report.compile_asm(os.path.join(isa_report.CSRC, "topk_kernels.hip"), out)
    ks = isa_report.kernels(out)
    os.unlink(out)
    names = [k["pretty"] for k in ks]
    assert sum("gallery_topk_kernel" in n for n in names) == 4 and sum("gallery_merge_kernel" in n for n in names) == 1, names
    for k in ks:
        assert k["scratch"] == 0 and k["vspill"] == 0, (k["pretty"], k["scratch"], k["vspill"])
        assert k["vgpr"] + k["agpr"] <= 256, (k["pretty"], k["vgpr"], k["agpr"])    # two waves per SIMD
        if "gallery_topk_kernel" in k["pretty"]:
            assert k["lds"] == 128 * 130 * 4 + 1024 and 2 * k["lds"] <= 160 * 1024, (k["pretty"], k["lds"])   # two workgroups per CU
