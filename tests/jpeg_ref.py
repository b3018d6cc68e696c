"""A plain restatement, in numpy int64, of what the two kernels of csrc/jpeg_kernels.hip compute — libjpeg's default decoder behind the
entropy decoder: dequantise + jpeg_idct_islow (jidctint.c) with the range limit's 10-bit wrap and clamp, h2v1 / h2v2 "fancy" chroma
upsampling (jdsample.c; planes up to two samples wide are replicated instead, jinit_upsampler) and the 16-bit fixed-point
YCbCr -> RGB of jdcolor.c.  It turns a frame dumped by tests/jpeg_frame_dump.cpp (the product's host half) into pixels, which
tests/test_jpeg_edges.py compares with libjpeg-turbo's own picture — so a mistake shared with a kernel cannot pass.

`mutations` plants one of the faults a kernel of this kind is prone to (MUTATIONS); the tests assert that the fixtures notice each."""
import numpy as np

MUTATIONS = (
    "h2v1_rounding_swapped",   # the +1 / +2 of the two output phases of h2v1 exchanged
    "h2v2_7_to_8",             # the odd phase of h2v2 rounded with +8 like the even one
    "narrow_lt_2",             # replication for planes narrower than 2 samples only (dw < 2 instead of dw <= 2)
    "no_fy_clamp",             # h2v2's further row not clamped to the plane: it reads whatever lies above / below in the plane buffer
    "bare_clamp",              # range limit without the 10-bit wrap: clamp(x + 128)
    "pass2_round_bit",         # second IDCT pass descaled with half the rounding term (1 << 16 instead of 1 << 17)
)

_C = dict(c0_298=2446, c0_390=3196, c0_541=4433, c0_765=6270, c0_899=7373, c1_175=9633, c1_501=12299, c1_847=15137, c1_961=16069, c2_053=16819,
          c2_562=20995, c3_072=25172)   # FIX(x) = round(x * 2^13)


def read_frame(path):
    """One file of jpeg_frame_dump: {"info": (w, h) or refusal text, "refused": text} or the frame's geometry, tables and coefficients."""
    raw = open(path, "rb").read()
    line, _, rest = raw.partition(b"\n")
    f = {"info": line.decode()[len("info "):]}
    f["info"] = f["info"] if f["info"].startswith("refused") else tuple(int(v) for v in f["info"].split())
    line, _, rest = rest.partition(b"\n")
    if line.startswith(b"refused"):
        f["refused"] = line.decode()[len("refused "):]
        return f
    tag, W, H, ncomp, hmax, vmax, prog, ncoef = line.decode().split()
    assert tag == "ok"
    f.update(W=int(W), H=int(H), ncomp=int(ncomp), hmax=int(hmax), vmax=int(vmax), progressive=int(prog), comp=[])
    for _ in range(f["ncomp"]):
        line, _, rest = rest.partition(b"\n")
        f["comp"].append(dict(zip(("id", "h", "v", "tq", "bw", "bh", "dw", "dh", "coef_off"), (int(v) for v in line.decode().split()))))
    assert len(rest) == 2 * (256 + int(ncoef))
    f["qt"] = np.frombuffer(rest, "<u2", 256).reshape(4, 64).astype(np.int64)
    f["coef"] = np.frombuffer(rest, "<i2", int(ncoef), 512).astype(np.int64)
    return f


def _islow_1d(x, shift, rounding):
    """jpeg_idct_islow's one-dimensional pass along the last axis (CONST_BITS 13), descaled by `shift` with the rounding term given."""
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., k] for k in range(8))
    # even part
    z1 = (x2 + x6) * _C["c0_541"]
    e2 = z1 - x6 * _C["c1_847"]
    e3 = z1 + x2 * _C["c0_765"]
    e0 = (x0 + x4) << 13
    e1 = (x0 - x4) << 13
    a0, a3, a1, a2 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    # odd part
    z1, z2, z3, z4 = x7 + x1, x5 + x3, x7 + x3, x5 + x1
    z5 = (z3 + z4) * _C["c1_175"]
    z1, z2 = -z1 * _C["c0_899"], -z2 * _C["c2_562"]
    z3, z4 = z5 - z3 * _C["c1_961"], z5 - z4 * _C["c0_390"]
    o0 = x7 * _C["c0_298"] + z1 + z3
    o1 = x5 * _C["c2_053"] + z2 + z4
    o2 = x3 * _C["c3_072"] + z2 + z3
    o3 = x1 * _C["c1_501"] + z1 + z4
    out = np.stack([a0 + o3, a1 + o2, a2 + o1, a3 + o0, a3 - o0, a2 - o1, a1 - o2, a0 - o3], axis=-1)
    return (out + rounding) >> shift


def planes(f, mutations=()):
    """Per component the [bh * 8][bw * 8] u8 sample plane: what jpeg_idct_kernel writes."""
    out = []
    for cp in f["comp"]:
        n = cp["bw"] * cp["bh"]
        blocks = f["coef"][cp["coef_off"]: cp["coef_off"] + 64 * n].reshape(n, 8, 8) * f["qt"][cp["tq"]].reshape(8, 8)
        ws = _islow_1d(blocks.transpose(0, 2, 1), 13 - 2, 1 << 10).transpose(0, 2, 1)       # columns, 2 extra bits kept
        px = _islow_1d(ws, 13 + 2 + 3, 1 << (16 if "pass2_round_bit" in mutations else 17))   # rows
        if "bare_clamp" not in mutations:
            px = ((px + 512) & 1023) - 512       # range_limit[x & RANGE_MASK]: the table is indexed with the low 10 bits
        px = np.clip(px + 128, 0, 255)
        out.append(px.reshape(cp["bh"], cp["bw"], 8, 8).transpose(0, 2, 1, 3).reshape(cp["bh"] * 8, cp["bw"] * 8))
    return out


def _upsample(f, pl, c, mutations):
    """Chroma plane c at full resolution, [H][W]."""
    W, H, cp = f["W"], f["H"], f["comp"][c]
    dw, dh = cp["dw"], cp["dh"]
    if f["hmax"] == 1:
        return pl[c][:H, :W]
    narrow = dw < 2 if "narrow_lt_2" in mutations else dw <= 2
    if f["vmax"] == 1:
        s = pl[c][:H, :dw]
        if narrow:
            return np.repeat(s, 2, axis=1)[:, :W]
        r_even, r_odd = (2, 1) if "h2v1_rounding_swapped" in mutations else (1, 2)
        even = (3 * s + np.concatenate([s[:, :1], s[:, :-1]], 1) + r_even) >> 2
        odd = (3 * s + np.concatenate([s[:, 1:], s[:, -1:]], 1) + r_odd) >> 2
        even[:, 0], odd[:, -1] = s[:, 0], s[:, -1]
        return np.stack([even, odd], -1).reshape(H, 2 * dw)[:, :W]
    if narrow:
        return np.repeat(np.repeat(pl[c][:dh, :dw], 2, 0), 2, 1)[:H, :W]
    y = np.arange(H)
    near = y >> 1
    far = np.where(y & 1, near + 1, near - 1)
    if "no_fy_clamp" in mutations:   # rows -1 and dh of the plane as the kernel's buffer holds them: components back to back, zeros behind
        stride = cp["bw"] * 8
        flat = np.concatenate([p.reshape(-1) for p in pl] + [np.zeros(stride, np.int64)])
        off = sum(p.size for p in pl[:c])
        farrow = flat[(off + far * stride)[:, None] + np.arange(dw)[None, :]]
    else:
        farrow = pl[c][np.clip(far, 0, dh - 1), :dw]
    t = 3 * pl[c][near, :dw] + farrow                                     # [H][dw] column sums
    even = (3 * t + np.concatenate([t[:, :1], t[:, :-1]], 1) + 8) >> 4
    odd = (3 * t + np.concatenate([t[:, 1:], t[:, -1:]], 1) + (8 if "h2v2_7_to_8" in mutations else 7)) >> 4
    even[:, 0] = (4 * t[:, 0] + 8) >> 4
    odd[:, -1] = (4 * t[:, -1] + (8 if "h2v2_7_to_8" in mutations else 7)) >> 4
    return np.stack([even, odd], -1).reshape(H, 2 * dw)[:, :W]


def pixels(f, mutations=()):
    """[H][W][3] u8 RGB: what jpeg_color_kernel writes."""
    assert set(mutations) <= set(MUTATIONS)
    pl = planes(f, mutations)
    Y = pl[0][: f["H"], : f["W"]]
    if f["ncomp"] == 1:
        return np.stack([Y, Y, Y], -1).astype(np.uint8)
    cb = _upsample(f, pl, 1, mutations) - 128
    cr = _upsample(f, pl, 2, mutations) - 128
    # jdcolor.c build_ycc_rgb_table, SCALEBITS 16: FIX(1.40200), FIX(1.77200), FIX(0.71414), FIX(0.34414); ONE_HALF is added once to G
    r = Y + ((91881 * cr + 32768) >> 16)
    g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
