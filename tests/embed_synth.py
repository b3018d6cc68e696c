"""Synthetic 112 x 112 embedding networks for the FaceEmbeddings tests and tools/embeddings_probe.py (test infrastructure; the reference
ships no face_embeddings.tflite, so the model is always the caller's) and the restatements of the reference's arithmetic the tests compare
against: crop_image_to_bbox (face_embeddings.rs:101-109), l2_norm and similarity_score (utils.rs:30-50)."""
import numpy as np

from synth_tflite import VALID, GraphBuilder

I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def embed_graph(seed, features, reshape, c0=16, second_output=False):
    """mesh_like's trunk on a 112 x 112 frame — stem 3x3 s2 + PReLU -> 2 blocks(c0) -> s2 to 2c0 -> 2 blocks -> s2 to 4c0 -> 2 blocks -> s2 to 8c0
    -> 3 blocks: 7 x 7 x 8c0 — then ONE whole-frame VALID convolution to [1,1,1,features], with or without a final RESHAPE to [1,features]."""
    g = GraphBuilder(seed, [1, 112, 112, 3])
    x = g.prelu(g.conv(g.input, c0, 3, 2))
    for mult, nb in ((1, 2), (2, 2), (4, 2), (8, 3)):
        if mult > 1:
            x = g.blaze_block(x, mult * c0, 2, act="prelu")
        for _ in range(nb):
            x = g.blaze_block(x, act="prelu")
    _, h, w, _ = g.shape(x)
    assert (h, w) == (7, 7)
    y = g.conv(x, features, h, 1, VALID)
    if reshape:
        y = g.reshape(y, [1, features])
    g.outputs = [y] + ([g.conv(x, 1, h, 1, VALID)] if second_output else [])   # (two outputs: a graph FaceEmbeddings must refuse)
    return g.finish()


def as_i32(v):
    """Rust's `f64 as i32`: toward zero, saturating, NaN -> 0"""
    v = float(v)
    if v != v:
        return 0
    if v >= I32_MAX:
        return I32_MAX
    if v <= I32_MIN:
        return I32_MIN
    return int(v)


def chip_rect(det, width, height):
    """faces[k].bbox().scale((width as f64, height as f64)) -> crop_image_to_bbox's rectangle and whether Mat::roi takes it (and it is not empty).
    det: at least 4 float32 values (xmin, ymin, xmax, ymax), normalised."""
    f = [float(np.float32(v)) for v in np.asarray(det).reshape(-1)[:4]]   # f32 widened to f64
    xmin, ymin, xmax, ymax = f[0] * float(width), f[1] * float(height), f[2] * float(width), f[3] * float(height)
    with np.errstate(invalid="ignore"):
        x, y, w, h = as_i32(xmin), as_i32(ymin), as_i32(np.float64(xmax) - np.float64(xmin)), as_i32(np.float64(ymax) - np.float64(ymin))
    valid = 0 <= x and 0 < w and x + w <= width and 0 <= y and 0 < h and y + h <= height
    return (x, y, w, h), valid


def seq_sum_f32(products):
    """sum::<f32>() of an iterator: from 0, in index order, every add rounded to f32; products float32 [..., n] -> float32 [...]"""
    p = np.asarray(products, np.float32)
    acc = np.zeros(p.shape[:-1], np.float32)
    for k in range(p.shape[-1]):
        acc = (acc + p[..., k]).astype(np.float32)
    return acc


def l2_norm_ref(x):
    x = np.asarray(x, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        norm = np.sqrt(seq_sum_f32(x * x))
        return (x / norm).astype(np.float32)


def similarity_matrix_ref(a, b):
    """similarity_score(a_i, b_j) for every pair: the three sums float32 and sequential (the accumulation runs over k for all pairs at once:
    the same operations on every element as the scalar loop)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(all="ignore"):
        dot = np.zeros((a.shape[0], b.shape[0]), np.float32)
        for k in range(a.shape[1]):
            dot = (dot + (a[:, k, None] * b[None, :, k]).astype(np.float32)).astype(np.float32)
        na, nb = np.sqrt(seq_sum_f32(a * a)), np.sqrt(seq_sum_f32(b * b))
        return (dot / (na[:, None] * nb[None, :]).astype(np.float32)).astype(np.float32)


def similarity_score_ref(a, b):
    return similarity_matrix_ref(np.asarray(a, np.float32).reshape(1, -1), np.asarray(b, np.float32).reshape(1, -1))[0, 0]
