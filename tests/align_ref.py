"""What the aligned-chip tests share: the five-point template, the fit restated in plain Python floats (sequential loops in the order
csrc/face_align.hpp states), the gather rule restated in numpy, the placements of the hand-made cases and the rotated pictures of man.jpg."""
import math

import numpy as np

TEMPLATE5 = [(38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041)]
TEMPLATE4 = TEMPLATE5[:3] + [((TEMPLATE5[3][0] + TEMPLATE5[4][0]) / 2.0, (TEMPLATE5[3][1] + TEMPLATE5[4][1]) / 2.0)]
TEMPLATES = {"points": TEMPLATE5, "mesh": TEMPLATE5, "detection": TEMPLATE4}
DEFAULT_ROI = (0.5, 0.5, 1.0, 1.0, 0.0, 1)   # the whole image, normalised: what an invalid fit leaves


def fit_ref(points, template):
    """points: (x, y) pairs as the entry sees them (f32 values); -> (valid, kind, (x_center, y_center, side, rotation)).  kind names the
    first test that failed: "n", "input", "S", "N", "result" or None."""
    n = len(points)
    if n < 2 or n > 5:
        return False, "n", None
    x = [float(np.float32(p[0])) for p in points]
    y = [float(np.float32(p[1])) for p in points]
    u = [float(q[0]) for q in template[:n]]
    v = [float(q[1]) for q in template[:n]]
    for i in range(n):
        if not (math.isfinite(x[i]) and math.isfinite(y[i])):
            return False, "input", None
    mx = my = mu = mv = 0.0
    for i in range(n):
        mx += x[i]
        my += y[i]
        mu += u[i]
        mv += v[i]
    mx, my, mu, mv = mx / n, my / n, mu / n, mv / n
    A = B = S = 0.0
    for i in range(n):
        dx, dy, du, dv = x[i] - mx, y[i] - my, u[i] - mu, v[i] - mv
        A += dx * du + dy * dv
        B += dx * dv - dy * du
        S += dx * dx + dy * dy
    N = A * A + B * B
    if not (S > 0.0 and math.isfinite(S)):
        return False, "S", None
    if not (N > 0.0 and math.isfinite(N)):
        return False, "N", None
    c, d = A * S / N, -(B * S / N)
    side = 112.0 * S / math.sqrt(N)
    rotation = math.atan2(-B, A)
    ex, ey = 56.0 - mu, 56.0 - mv
    xc, yc = mx + (c * ex - d * ey), my + (d * ex + c * ey)
    if not (math.isfinite(side) and side > 0.0 and math.isfinite(xc) and math.isfinite(yc)):
        return False, "result", None
    return True, None, (xc, yc, side, rotation)


def place(template, centre, scale=1.0, degrees=0.0):
    """the template carried into the image by the chip -> image similarity that sends the chip's centre (56, 56) to `centre`, scales by
    `scale` and rotates by `degrees`: float32 [n,2].  The fitted ROI is then (centre, 112 * scale, rotation = degrees), up to f32 rounding."""
    t = math.radians(degrees)
    c, s = math.cos(t) * scale, math.sin(t) * scale
    q = np.asarray(template, np.float64) - 56.0
    p = np.stack([centre[0] + c * q[:, 0] - s * q[:, 1], centre[1] + s * q[:, 0] + c * q[:, 1]], axis=1)
    return p.astype(np.float32)


# (name, centre, scale, degrees): the similarities of CPU test 1; the last three put the face partly outside a 320 x 240 frame
PLACEMENTS = [
    ("identity", (56.0, 56.0), 1.0, 0.0),
    ("scale 0.37", (160.0, 120.0), 0.37, 0.0),
    ("scale 4.1", (160.0, 120.0), 4.1, 0.0),
    ("+30", (200.0, 100.0), 1.0, 30.0),
    ("-30", (200.0, 100.0), 1.0, -30.0),
    ("+90", (100.0, 150.0), 1.3, 90.0),
    ("-90", (100.0, 150.0), 1.3, -90.0),
    ("180", (160.0, 120.0), 0.8, 180.0),
    ("179.9", (160.0, 120.0), 0.8, 179.9),
    ("off the top left", (-5.0, -5.0), 1.0, 0.0),
    ("off the bottom left", (10.0, 230.0), 1.0, 10.0),
    ("off the right", (330.0, 120.0), 1.7, -75.0),
]


def noise(index, n):
    """deterministic noise of up to 3 px per coordinate"""
    return np.random.RandomState(1000 + index).uniform(-3.0, 3.0, (n, 2))


def fit_cases(source):
    """(name, float32 points [n,2]) for the template of `source`: every placement, then every placement with noise"""
    t = TEMPLATES[source]
    out = [(name, place(t, c, s, d)) for name, c, s, d in PLACEMENTS]
    out += [(name + " noisy", (place(t, c, s, d).astype(np.float64) + noise(i, len(t))).astype(np.float32)) for i, (name, c, s, d) in enumerate(PLACEMENTS)]
    return out


def gather_ref(source, src, width, height):
    """the gather rule restated: f64 products and midpoints, then the f32 store -> float32 [n,2]"""
    w, h = np.float64(width), np.float64(height)
    if source == "mesh":
        lm = np.asarray(src, np.float32).reshape(468, 3).astype(np.float64)
        px, py = lm[:, 0] * w, lm[:, 1] * h
        mid = lambda a, b: ((px[a] + px[b]) / 2.0, (py[a] + py[b]) / 2.0)
        one = lambda a: (px[a], py[a])
        return np.asarray([mid(33, 133), mid(362, 263), one(1), one(61), one(291)], np.float64).astype(np.float32)
    d = np.asarray(src, np.float32).reshape(17).astype(np.float64)
    return np.asarray([(d[4 + 2 * i] * w, d[5 + 2 * i] * h) for i in range(4)], np.float64).astype(np.float32)


ANGLES = (-20, 0, 20)


def rotated_frames(man_image):
    """man.jpg rotated in-plane about its centre onto a canvas of its own size, black outside: uint8 [3,H,W,3] for ANGLES"""
    from PIL import Image
    img = Image.fromarray(man_image)
    return np.stack([np.asarray(img.rotate(a, resample=Image.BILINEAR)) for a in ANGLES])


def padded_frames(seed, n, height, width, pad=5):
    """(buffer uint8 [n,height,3*width+pad], its view [n,height,width,3]): frames whose rows are 3 * width + pad bytes apart"""
    stride = 3 * width + pad
    buf = np.random.RandomState(seed).randint(0, 256, (n, height, stride)).astype(np.uint8)
    frames = buf[:, :, :3 * width].reshape(n, height, width, 3)
    assert np.shares_memory(frames, buf) and frames.strides == (height * stride, stride, 3, 1)
    return buf, frames
