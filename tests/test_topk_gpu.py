"""mi_gallery_topk on the device.  The check everywhere is exact: index equals, and score is bit-equal to, mi_topk_select (the host statement
of the rule, tests/test_topk_cpu.py) applied to what mi_similarity_matrix writes for the same operands; label is labels[index], or -1.  The
order is total, so no tolerance and no near-tie is involved: any correct kernel gives these bytes.  Operands live in host and in device
memory.  The embedding network of the flow test is synthetic (embed_synth.embed_graph): its scores mean nothing."""
import ctypes as C

import numpy as np
import pytest

import embed_synth as es

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A   # as int32 no index or label of these tests; as float32 1.5e16: no cosine, and not -inf
GUARD = 64


def _torch():
    """torch carries the device-resident operands: on a GPU box a broken install is a failure, not a skip"""
    try:
        import torch
        return torch
    except Exception as e:  # noqa: BLE001
        pytest.fail("torch is needed for device-resident operands: %r" % (e,))


@pytest.fixture(scope="module")
def gpu(mi):
    if mi.device_count() < 1:
        pytest.fail("no HIP device: the GPU suite must run on an MI355X box")
    return mi


def operands(n, m, D, seed):
    rs = np.random.RandomState(seed)
    q, g = rs.standard_normal((n, D)).astype(np.float32), rs.standard_normal((m, D)).astype(np.float32)
    labels = rs.randint(-5, 1 << 20, m).astype(np.int32)
    return q, g, labels


def expected(gpu, q, g, k, labels=None):
    """mi_topk_select on mi_similarity_matrix's output; labels[index] or -1"""
    index, score = gpu.topk_select(gpu.similarity_matrix(q, g), k)
    lab = np.arange(g.shape[0], dtype=np.int32) if labels is None else labels
    return index, score, np.where(index >= 0, lab[np.maximum(index, 0)], -1).astype(np.int32)


def same(got, want, what=""):
    index, score, label = (np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x) for x in got)
    np.testing.assert_array_equal(index, want[0], err_msg="index " + what)
    np.testing.assert_array_equal(score.view(np.uint32), want[1].view(np.uint32), err_msg="score bits " + what)
    np.testing.assert_array_equal(label, want[2], err_msg="label " + what)


# ---------------------------------------------------------------------------------------------------- 1. tile edges
EDGE_SHAPES = [(1, 1, 1, 1), (3, 2, 5, 4), (130, 257, 33, 5), (129, 16, 100, 16), (2, 17, 64, 16)]


@pytest.fixture(scope="module")
def edge_cases(gpu):
    """(n, m, D, k) -> (q, g, labels, expected), once"""
    cache = {}

    def get(shape):
        if shape not in cache:
            n, m, D, k = shape
            q, g, labels = operands(n, m, D, 7 * n + m)
            cache[shape] = (q, g, labels, expected(gpu, q, g, k, labels))
        return cache[shape]
    return get


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tile_edges(gpu, edge_cases, shape, where):
    n, m, D, k = shape
    q, g, labels, want = edge_cases(shape)
    if where == "device":
        torch = _torch()
        gal = gpu.Gallery(torch.from_numpy(g).cuda(), labels)
        got = gal.topk(torch.from_numpy(q).cuda(), k)
        torch.cuda.synchronize()
    else:
        gal = gpu.Gallery(g, labels)
        got = gal.topk(q, k)
    assert (gal.m, gal.features) == (m, D) and tuple(got[0].shape) == (n, k)
    same(got, want, "%s %s" % (shape, where))
    if m < k:
        assert (want[0][:, m:] == -1).all() and np.isneginf(want[1][:, m:]).all()   # fewer rows than slots
    gal.close()


def test_without_labels_the_label_is_the_index(gpu, edge_cases):
    q, g, _, _ = edge_cases((130, 257, 33, 5))
    gal = gpu.Gallery(g)
    got = gal.topk(q, 5)
    same(got, expected(gpu, q, g, 5), "no labels")
    np.testing.assert_array_equal(got[2], got[0])
    dims = (C.c_int(), C.c_int())
    assert gal.L.mi_gallery_dims(gal.h, C.byref(dims[0]), C.byref(dims[1])) == 0 and (dims[0].value, dims[1].value) == (257, 33)
    # a label array that is not asked for
    index, score = np.empty((130, 5), np.int32), np.empty((130, 5), np.float32)
    assert gal.L.mi_gallery_topk(gal.h, C.c_void_p(q.ctypes.data), 130, 5, C.c_void_p(index.ctypes.data), C.c_void_p(score.ctypes.data), None, 0, None) == 0
    np.testing.assert_array_equal(index, got[0])
    gal.close()


# ---------------------------------------------------------------------------------------------------- 2. splits, ties, NaN
@pytest.fixture(scope="module")
def thousand(gpu):
    """n = 5 queries against m = 1000 rows (eight column tiles), D = 100: rows 5, 127, 128, 300 and 999 are copies of query 2, row 77 is zero,
    query 4 is zero"""
    q, g, labels = operands(5, 1000, 100, 99)
    g[[5, 127, 128, 300, 999]] = q[2]
    g[77] = 0.0
    q[4] = 0.0
    return q, g, labels, expected(gpu, q, g, 16, labels)


def test_every_split_count_gives_the_same_bytes(gpu, thousand):
    q, g, labels, want = thousand
    gal = gpu.Gallery(g, labels)
    assert gal.get_option("splits") == 0
    for splits in (1, 2, 3, 8, 64, 0):   # 64: clamped to the eight column tiles
        gal.set_option("splits", splits)
        assert gal.get_option("splits") == splits
        same(gal.topk(q, 16), want, "splits = %d" % splits)
    for bad in (-1, 65):
        with pytest.raises(gpu.MiError) as e:
            gal.set_option("splits", bad)
        assert e.value.code == -1
    with pytest.raises(gpu.MiError) as e:
        gal.set_option("tiles", 1)
    assert e.value.code == -1 and "unknown option" in str(e.value)
    with pytest.raises(gpu.MiError) as e:
        gal.get_option("tiles")
    assert e.value.code == -1
    assert gal.get_option("splits") == 0
    gal.close()


@pytest.mark.parametrize("splits", [1, 3])
def test_ties_come_out_in_index_order(gpu, thousand, splits):
    q, g, labels, want = thousand
    gal = gpu.Gallery(g, labels)
    gal.set_option("splits", splits)
    index, score, label = gal.topk(q, 16)
    assert list(index[2, :5]) == [5, 127, 128, 300, 999]          # across tiles (127 | 128) and across column ranges
    assert len(set(score[2, :5].view(np.uint32).tolist())) == 1   # copies of one row: one score, bit for bit
    assert score[2, 5] < score[2, 4]
    same((index, score, label), want)
    gal.close()


def test_zero_rows_match_nobody(gpu, thousand):
    q, g, labels, want = thousand
    gal = gpu.Gallery(g, labels)
    index, score, label = gal.topk(q, 16)
    assert not (index == 77).any()                                                          # a zero gallery row is never returned
    assert (index[4] == -1).all() and np.isneginf(score[4]).all() and (label[4] == -1).all()  # a zero query returns nothing
    assert (index[:4] >= 0).all()
    gal.close()
    # where every eligible row is returned, the zero row is the one that is missing
    gal = gpu.Gallery(g[70:80], labels[70:80])
    index, score, label = gal.topk(q[:2], 16)
    assert sorted(index[0, :9].tolist()) == [0, 1, 2, 3, 4, 5, 6, 8, 9] and (index[:, 9:] == -1).all() and (label[:, 9:] == -1).all()
    same((index, score, label), expected(gpu, q[:2], g[70:80], 16, labels[70:80]))
    gal.close()


# ---------------------------------------------------------------------------------------------------- 3. bounds
@pytest.mark.parametrize("where", ["host", "device"])
def test_every_slot_is_written_and_nothing_behind_them(gpu, edge_cases, where):
    n, m, D, k = shape = (130, 257, 33, 5)
    q, g, labels, want = edge_cases(shape)
    gal = gpu.Gallery(g, labels)
    bufs = [np.full(n * k + GUARD, SENTINEL, np.int32) for _ in range(3)]   # index, score (as bits), label
    if where == "device":
        torch = _torch()
        dq = torch.from_numpy(q).cuda()
        dbufs = [torch.from_numpy(b).cuda() for b in bufs]
        torch.cuda.synchronize()
        rc = gal.L.mi_gallery_topk(gal.h, C.c_void_p(dq.data_ptr()), n, k, *[C.c_void_p(b.data_ptr()) for b in dbufs], gpu.MI_MEM_DEVICE, None)
        bufs = [b.cpu().numpy() for b in dbufs]
    else:
        rc = gal.L.mi_gallery_topk(gal.h, C.c_void_p(q.ctypes.data), n, k, *[C.c_void_p(b.ctypes.data) for b in bufs], gpu.MI_MEM_HOST, None)
    assert rc == 0, gal.L.mi_last_error()
    for b, what in zip(bufs, ("index", "score", "label")):
        assert (b[:n * k] != SENTINEL).all(), what + ": a slot was not written"
        assert (b[n * k:] == SENTINEL).all(), what + ": the guard was written"
    same((bufs[0][:n * k].reshape(n, k), bufs[1][:n * k].view(np.float32).reshape(n, k), bufs[2][:n * k].reshape(n, k)), want)
    gal.close()


def test_refusals_on_a_live_handle(gpu, edge_cases):
    q, g, labels, _ = edge_cases((3, 2, 5, 4))
    gal = gpu.Gallery(g, labels)
    out = np.zeros(64, np.int32)
    p, pq = C.c_void_p(out.ctypes.data), C.c_void_p(q.ctypes.data)
    call = lambda **kw: gal.L.mi_gallery_topk(gal.h, kw.get("q", pq), kw.get("n", 3), kw.get("k", 4), kw.get("index", p), kw.get("score", p), p, kw.get("mem", 0), None)
    for kw in (dict(q=None), dict(index=None), dict(score=None), dict(n=0), dict(k=0), dict(k=17), dict(mem=2)):
        assert call(**kw) == -1 and gal.L.mi_last_error(), kw
    assert not out.any()   # nothing was queued
    h = C.c_void_p()
    assert gal.L.mi_gallery_create(64, pq, 3, 5, None, 0, C.byref(h)) == -4 and h.value is None   # MI_EDEVICE: no such device
    gal.close()


# ---------------------------------------------------------------------------------------------------- 4. regrowth and asynchrony
@pytest.fixture(scope="module")
def growth_case(gpu):
    q, g, labels = operands(300, 1000, 64, 5)
    return q, g, labels, expected(gpu, q, g, 8, labels)


def test_scratch_regrowth_leaves_results_unchanged(gpu, growth_case):
    q, g, labels, want = growth_case
    gal = gpu.Gallery(g, labels)   # one handle: its scratch grows, is used below its size, grows no further
    for n in (4, 300, 4):
        fresh = gpu.Gallery(g, labels)
        got, one = gal.topk(q[:n], 8), fresh.topk(q[:n], 8)
        same(got, tuple(w[:n] for w in want), "n = %d" % n)
        same(one, tuple(w[:n] for w in want), "fresh handle, n = %d" % n)
        fresh.close()
    gal.close()


def test_two_caller_streams_on_one_handle(gpu, growth_case):
    torch = _torch()
    q, g, labels, want = growth_case
    gal = gpu.Gallery(torch.from_numpy(g).cuda(), labels)
    dq = torch.from_numpy(q).cuda()
    dq_small = dq[:4].contiguous()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    # the second call shares the handle's scratch with the first, which is still in flight: it waits for it on the device
    big = gal.topk(dq, 8, stream=streams[0].cuda_stream)
    small = gal.topk(dq_small, 8, stream=streams[1].cuda_stream)
    again = gal.topk(dq, 8, stream=streams[0].cuda_stream)
    for s in streams:
        s.synchronize()
    same(big, want, "first stream")
    same(small, tuple(w[:4] for w in want), "second stream")
    same(again, want, "first stream again")
    gal.close()


# ---------------------------------------------------------------------------------------------------- 5. the flow
def canvases(img):
    """Canvases of 720 rows x 1080 columns from man.jpg (360 x 540) and its mirror image: four, two and one face(s), and all black"""
    H, W = img.shape[:2]
    mirror = img[:, ::-1]
    four = np.concatenate([np.concatenate([img, mirror], axis=1), np.concatenate([mirror, img], axis=1)], axis=0)
    two, one = four.copy(), np.zeros_like(four)
    two[H:] = 0
    one[:H, :W] = img
    return np.stack([four, two, one, np.zeros_like(four)])


def test_embeddings_of_run_faces_items_against_a_gallery_of_themselves(gpu, man_image, tmp_path):
    torch = _torch()
    frames = canvases(man_image)
    p = gpu.Pipeline(gpu.FaceDetectionModel.BackCamera)
    res = p.run_faces(frames, max_faces=4, max_items=12)
    p.close()
    path = tmp_path / "embed.tflite"
    path.write_bytes(es.embed_graph(71, 128, True))
    fe = gpu.FaceEmbeddings(str(path))
    dres = {k: torch.from_numpy(np.ascontiguousarray(res[k])).cuda() for k in ("faces", "item_frame", "item_face")}
    stream = torch.cuda.Stream()
    out = fe.infer_items(torch.from_numpy(frames).cuda(), dres, stream=stream.cuda_stream)
    stream.synchronize()
    emb, valid = out["embeddings"], out["valid"].cpu().numpy()   # [12, 128] as they lie in device memory: zeros for invalid items
    assert 5 <= valid.sum() < 12, valid
    extra = torch.from_numpy(np.random.RandomState(8).standard_normal((300, 128)).astype(np.float32)).cuda()
    rows = torch.cat([emb, extra]).contiguous()
    labels = np.arange(1000, 1000 + 312, dtype=np.int32)
    gal = gpu.Gallery(rows, labels)
    got = gal.topk(emb, 5, stream=stream.cuda_stream)
    stream.synchronize()
    index, score, label = (x.cpu().numpy() for x in got)
    same((index, score, label), expected(gpu, emb.cpu().numpy(), rows.cpu().numpy(), 5, labels), "flow")
    for j in range(12):
        if valid[j]:
            assert (index[j] >= 0).all() and (label[j] == 1000 + index[j]).all()
            assert not np.isin(index[j], np.flatnonzero(valid == 0)).any()   # (the zero rows of invalid items are in the gallery: never returned)
        else:
            assert (index[j] == -1).all() and np.isneginf(score[j]).all() and (label[j] == -1).all()
    gal.close()
    fe.close()
