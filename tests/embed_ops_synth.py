"""Synthetic graphs and executable specifications of the embedding-graph operators AVERAGE_POOL_2D, MEAN, L2_NORMALIZATION, SUB, DIV and TRANSPOSE
(test infrastructure, on top of resnet_synth.ResnetBuilder): single-operator graphs, the pooled-head network (a small NHWC trunk -> whole-frame average
-> RESHAPE -> FULLY_CONNECTED -> L2_NORMALIZATION behind an input normalisation (x - m) / s) with its oracle twin, the f32 restatements of the
operators in the order the kernels promise, and their float64 evaluations with derived bounds.

The restatements walk the taps / channels in explicit loops; every step is ONE numpy float32 operation on arrays whose elements are independent
output elements, so every operation of every chain is rounded once, exactly as a loop over float32 scalars would round it.

Codes and option layouts (BuiltinOperator / BuiltinOptions of the TFLite schema): AVERAGE_POOL_2D 1 (Pool2DOptions, tag 5), L2_NORMALIZATION 11
(L2NormOptions, tag 12: fused activation), TRANSPOSE 39 (TransposeOptions, tag 26: no fields), MEAN 40 (ReducerOptions, tag 27: keep_dims),
SUB 41 (SubOptions, tag 28: fused activation), DIV 42 (DivOptions, tag 29: fused activation)."""
import numpy as np

from resnet_synth import ResnetBuilder
from synth_tflite import ACT_NONE, ACT_RELU, ACT_RELU6, DEPTHWISE_CONV_2D, OPT_DW, OPT_POOL, SAME, VALID

AVERAGE_POOL_2D, L2_NORMALIZATION, TRANSPOSE, MEAN, SUB, DIV = 1, 11, 39, 40, 41, 42
OPT_L2NORM, OPT_TRANSPOSE, OPT_REDUCER, OPT_SUB, OPT_DIV = 12, 26, 27, 28, 29


class EmbedOpsBuilder(ResnetBuilder):
    def avgpool(self, x, kh, kw, stride=1, padding=VALID, act=ACT_NONE, out_shape=None):
        n, h, w, c = self.shape(x)
        ho, wo = ((h + stride - 1) // stride, (w + stride - 1) // stride) if padding == SAME else ((h - kh) // stride + 1, (w - kw) // stride + 1)
        y = self._act([n, ho, wo, c] if out_shape is None else out_shape, "avgpool")
        self.ops.append((AVERAGE_POOL_2D, [x], [y], OPT_POOL, [("i8", padding), ("i32", stride), ("i32", stride), ("i32", kw), ("i32", kh), ("i8", act)]))
        return y

    def mean(self, x, axes=(1, 2), keep_dims=True, axes_const=True):
        shp = self.shape(x)
        red = {a % len(shp) for a in axes if -len(shp) <= a < len(shp)}
        out = [1 if d in red else s for d, s in enumerate(shp)] if keep_dims else [s for d, s in enumerate(shp) if d not in red]
        at = self.const(np.array(axes), "axes", dtype=2) if axes_const else self._act([len(axes)], "axes")
        y = self._act(out, "mean")
        self.ops.append((MEAN, [x, at], [y], OPT_REDUCER, [("u8", 1 if keep_dims else 0)]))
        return y

    def l2norm(self, x, act=ACT_NONE):
        y = self._act(self.shape(x), "l2norm")
        self.ops.append((L2_NORMALIZATION, [x], [y], OPT_L2NORM, [("i8", act)]))
        return y

    def _arith(self, code, tag, a, b, shape, act):
        y = self._act(shape, "arith")
        self.ops.append((code, [a, b], [y], tag, [("i8", act)]))
        return y

    def sub_const(self, x, c, const_first=False, act=ACT_NONE):
        ct = self.const(np.asarray(c, np.float32), "sub")
        return self._arith(SUB, OPT_SUB, *((ct, x) if const_first else (x, ct)), self.shape(x), act)

    def div_const(self, x, c, const_first=False, act=ACT_NONE):
        ct = self.const(np.asarray(c, np.float32), "div")
        return self._arith(DIV, OPT_DIV, *((ct, x) if const_first else (x, ct)), self.shape(x), act)

    def sub(self, a, b):
        return self._arith(SUB, OPT_SUB, a, b, self.shape(a), ACT_NONE)

    def div(self, a, b):
        return self._arith(DIV, OPT_DIV, a, b, self.shape(a), ACT_NONE)

    def transpose(self, x, perm, perm_const=True, out_shape=None):
        shp = self.shape(x)
        out = [shp[p] if 0 <= p < len(shp) else 1 for p in perm] if out_shape is None else out_shape
        pt = self.const(np.array(perm), "perm", dtype=2) if perm_const else self._act([len(perm)], "perm")
        y = self._act(out, "transpose")
        self.ops.append((TRANSPOSE, [x, pt], [y], OPT_TRANSPOSE, []))
        return y


def single(in_shape, build, seed=1):
    """a graph whose output is build(g, g.input) (a tensor or a list of tensors)"""
    g = EmbedOpsBuilder(seed, in_shape)
    y = build(g, g.input)
    g.outputs = list(y) if isinstance(y, (list, tuple)) else [y]
    return g.finish()


def avgpool_graph(h, w, c, kh, kw, stride=1, padding=VALID, act=ACT_NONE):
    return single([1, h, w, c], lambda g, x: g.avgpool(x, kh, kw, stride, padding, act))


def mean_graph(h, w, c, axes=(1, 2), keep_dims=True):
    return single([1, h, w, c], lambda g, x: g.mean(x, axes, keep_dims))


def l2norm_graph(shape):
    """input [1,H,W,C] -> (RESHAPE to `shape` where it differs) -> L2_NORMALIZATION"""
    shape = list(shape)
    n = int(np.prod(shape))
    in_shape = shape if len(shape) == 4 else [1, 1, 1, n]
    return single(in_shape, lambda g, x: g.l2norm(x if in_shape == shape else g.reshape(x, shape)))


def arith_graph(kind, c, h=5, w=7, const=None, act=ACT_NONE):
    """kind: "x-c", "c-x", "x/c" (the constant per channel, or a scalar when `const` is one)"""
    def build(g, x):
        if kind == "x-c":
            return g.sub_const(x, const, act=act)
        if kind == "c-x":
            return g.sub_const(x, const, const_first=True, act=act)
        return g.div_const(x, const, act=act)
    return single([1, h, w, c], build)


def transpose_graph(h, w, c, perm, back=False):
    """TRANSPOSE as the graph's output; back: followed by its inverse (the output is the input again)"""
    inv = [int(i) for i in np.argsort(perm)]
    return single([1, h, w, c], lambda g, x: g.transpose(g.transpose(x, perm), inv) if back else g.transpose(x, perm))


# ---------------------------------------------------------------------------------------------------- the pooled-head network
POOLED_MEAN = np.array([0.485, 0.456, 0.406], np.float32)   # (x - m) / s on [0, 1] pictures: s is no power of two, a true division
POOLED_STD = np.array([0.229, 0.224, 0.225], np.float32)


def pooled_head(seed, features, pool="avgpool", twin=False, l2=True):
    """[1,112,112,3] -> SUB m -> DIV s -> 3x3 s2 + ReLU -> three stride-2 BlazeBlocks (56 -> 28 -> 14 -> 7, 16 / 32 / 64 / 64 channels) -> the 7x7
    average (AVERAGE_POOL_2D, or MEAN over (1, 2) with and without keep_dims: pool = "avgpool" | "mean_keep" | "mean") -> RESHAPE [1,64] ->
    FULLY_CONNECTED(features) -> L2_NORMALIZATION.  twin: the same constants, drawn in the same order, on operators the oracle runs — the
    normalisation as a 1x1 depthwise convolution (filter 1 / s, bias -m / s), the average as a 7x7 VALID depthwise convolution with 1 / 49 taps, the
    FULLY_CONNECTED as a 1x1 convolution; its output is the vector in front of the L2_NORMALIZATION, which the test applies in numpy."""
    g = EmbedOpsBuilder(seed, [1, 112, 112, 3], twin)
    if twin:
        wt = g.const((1.0 / POOLED_STD.astype(np.float64)).astype(np.float32).reshape(1, 1, 1, 3), "wd")
        bt = g.const((-POOLED_MEAN.astype(np.float64) / POOLED_STD.astype(np.float64)).astype(np.float32), "bd")
        x = g._act(g.shape(g.input), "dw")
        g.ops.append((DEPTHWISE_CONV_2D, [g.input, wt, bt], [x], OPT_DW, [("i8", SAME), ("i32", 1), ("i32", 1), ("i32", 1), ("i8", ACT_NONE)]))
    else:
        x = g.div_const(g.sub_const(g.input, POOLED_MEAN), POOLED_STD)
    x = g.relu(g.conv(x, 16, 3, 2))
    for co in (32, 64, 64):
        x = g.blaze_block(x, co, 2)
    _, h, w, c = g.shape(x)
    assert (h, w, c) == (7, 7, 64)
    wfc = g._w((features, c), c)
    bfc = g.rng.standard_normal(features).astype(np.float32) * 0.1
    if twin:
        wt, bt = g.const(np.full((1, 7, 7, c), 1.0 / 49.0, np.float32), "wd"), g.const(np.zeros(c, np.float32), "bd")
        p = g._act([1, 1, 1, c], "dw")
        g.ops.append((DEPTHWISE_CONV_2D, [x, wt, bt], [p], OPT_DW, [("i8", VALID), ("i32", 1), ("i32", 1), ("i32", 1), ("i8", ACT_NONE)]))
        y = g.reshape(g.conv_with(p, wfc.reshape(features, 1, 1, c), bfc, 1, VALID), [1, features])
    else:
        p = g.avgpool(x, 7, 7) if pool == "avgpool" else g.mean(x, (1, 2), pool == "mean_keep")
        y = g.fc(p if pool == "mean" else g.reshape(p, [1, c]), features, weights=wfc, bias=bfc)
        if l2:
            y = g.l2norm(y)
    g.outputs = [y]
    return g.finish()


# ---------------------------------------------------------------------------------------------------- restatements (f32, the kernels' order)
def _f32(x):
    x = np.asarray(x)
    assert x.dtype == np.float32
    return x


def _pool_geometry(h, w, kh, kw, stride, padding):
    if padding == SAME:
        ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
        pt, pl = max(0, (ho - 1) * stride + kh - h) // 2, max(0, (wo - 1) * stride + kw - w) // 2
    else:
        ho, wo, pt, pl = (h - kh) // stride + 1, (w - kw) // stride + 1, 0, 0
    return ho, wo, pt, pl


def _act(v, act):
    if act == ACT_RELU:
        return np.maximum(v, np.float32(0))
    if act == ACT_RELU6:
        return np.minimum(np.maximum(v, np.float32(0)), np.float32(6))
    return v


def avgpool_ref(x, kh, kw, stride=1, padding=VALID, act=ACT_NONE):
    """per output element: s = 0.0f; the window's in-frame taps added in (ky, kx) order (taps outside the frame are skipped); one division by
    float(taps in the frame); the activation.  x: [B,H,W,C] float32."""
    x = _f32(x)
    B, H, W, C = x.shape
    ho, wo, pt, pl = _pool_geometry(H, W, kh, kw, stride, padding)
    out = np.empty((B, ho, wo, C), np.float32)
    for oy in range(ho):
        for ox in range(wo):
            s, taps = np.zeros((B, C), np.float32), 0
            for ky in range(kh):
                iy = oy * stride - pt + ky
                if iy < 0 or iy >= H:
                    continue
                for kx in range(kw):
                    ix = ox * stride - pl + kx
                    if ix < 0 or ix >= W:
                        continue
                    s = s + x[:, iy, ix, :]
                    taps += 1
            assert s.dtype == np.float32 and taps >= 1
            out[:, oy, ox, :] = _act(s / np.float32(taps), act)
    return out


def avgpool_f64(x, kh, kw, stride=1, padding=VALID, act=ACT_NONE):
    """float64 evaluation and the bound (n + 1) 2^-24 sum|x| / n of an f32 sum of n terms and one division"""
    x64 = np.asarray(x, np.float64)
    B, H, W, C = x64.shape
    ho, wo, pt, pl = _pool_geometry(H, W, kh, kw, stride, padding)
    ref, bound = np.empty((B, ho, wo, C)), np.empty((B, ho, wo, C))
    for oy in range(ho):
        for ox in range(wo):
            y0, y1 = max(0, oy * stride - pt), min(H, oy * stride - pt + kh)
            x0, x1 = max(0, ox * stride - pl), min(W, ox * stride - pl + kw)
            win = x64[:, y0:y1, x0:x1, :]
            n = (y1 - y0) * (x1 - x0)
            ref[:, oy, ox, :] = win.sum(axis=(1, 2)) / n
            bound[:, oy, ox, :] = (n + 1) * 2.0 ** -24 * np.abs(win).sum(axis=(1, 2)) / n
    if act == ACT_RELU:
        ref = np.maximum(ref, 0)
    elif act == ACT_RELU6:
        ref = np.clip(ref, 0, 6)
    return ref, bound


def l2norm_ref(x):
    """over the last dimension: s = 0; s = s + x[c] * x[c] in channel order (multiply and add rounded separately); n = max(sqrt(s), 1e-6f); x[c] / n"""
    x = _f32(x)
    s = np.zeros(x.shape[:-1], np.float32)
    for c in range(x.shape[-1]):
        p = x[..., c] * x[..., c]
        s = s + p
    assert s.dtype == np.float32
    n = np.maximum(np.sqrt(s), np.float32(1e-6))
    assert n.dtype == np.float32
    return (x / n[..., None]).astype(np.float32)


def l2norm_f64(x):
    """float64 evaluation and the bound (D + 8) 2^-24 |y|: D + 2 roundings in the sum of squares, halved by the square root, the root's and the
    division's own, with room to spare"""
    x64 = np.asarray(x, np.float64)
    n = np.maximum(np.sqrt((x64 * x64).sum(axis=-1, keepdims=True)), 1e-6)
    y = x64 / n
    return y, (x64.shape[-1] + 8) * 2.0 ** -24 * np.abs(y)


# ---------------------------------------------------------------------------------------------------- the ONNX-exported idiom
class OnnxStyleBuilder(EmbedOpsBuilder):
    """One network in three writings that draw their constants from the generator in one order.  layout "nchw": as an ONNX converter leaves it — the
    tensors between operators are NCHW, batch-norm constants [1,C,1,1], PRELU slopes [C,1,1], PAD on axes 2 and 3, every convolution wrapped in
    TRANSPOSE (0,2,3,1) ... TRANSPOSE (0,3,1,2), the flatten in C,H,W order.  "nhwc": the same operators without transposes, last-axis constants,
    the FULLY_CONNECTED's columns in H,W,C order.  "twin": operators the oracle runs (resnet_synth's twin rules)."""

    def __init__(self, seed, in_shape, layout):
        super().__init__(seed, in_shape, twin=layout == "twin")
        self.cf = layout == "nchw"

    def channels(self, x):
        return self.shape(x)[1 if self.cf else 3]

    def enter(self, x):
        return self.transpose(x, (0, 3, 1, 2)) if self.cf else x

    def bn(self, x):
        if not self.cf or len(self.shape(x)) != 4:
            return super().bn(x)
        c = self.channels(x)
        scale = self.rng.uniform(0.5, 1.5, c).astype(np.float32)
        shift = (0.1 * self.rng.standard_normal(c)).astype(np.float32)
        return self.add_const(self.mul_const(x, scale.reshape(1, c, 1, 1)), shift.reshape(1, c, 1, 1))

    def prelu(self, x):
        if not self.cf:
            return super().prelu(x)
        c = self.channels(x)
        al = self.const((self.rng.random((1, 1, c)) * 0.5).astype(np.float32).reshape(c, 1, 1), "alpha")
        y = self._act(self.shape(x), "prelu")
        self.ops.append((54, [x, al], [y], 0, None))
        return y

    def conv(self, x, co, k=1, stride=1):
        """k = 3: an explicit PAD of one pixel all round and a VALID convolution, as ONNX writes pads = 1"""
        c = self.channels(x)
        w = self._w((co, k, k, c), k * k * c)
        b = self.rng.standard_normal(co).astype(np.float32) * 0.1
        if k == 3 and self.cf:
            n, _, h, wd = self.shape(x)
            p = self.const(np.array([[0, 0], [0, 0], [1, 1], [1, 1]]), "pads", dtype=2)
            padded = self._act([n, c, h + 2, wd + 2], "pad")
            self.ops.append((34, [x, p], [padded], 22, []))
            x = padded
        elif k == 3:
            x = self.pad_spatial(x, 1, 1, 1, 1)
        if self.cf:
            x = self.transpose(x, (0, 2, 3, 1))
        y = self.conv_with(x, w, b, stride, VALID)
        return self.transpose(y, (0, 3, 1, 2)) if self.cf else y

    def res_block(self, x, co, stride):
        c = self.channels(x)
        y = self.bn(self.conv(self.bn(x), co, 3, 1))
        y = self.bn(self.conv(self.prelu(y), co, 3, stride))
        shortcut = x if stride == 1 and c == co else self.bn(self.conv(x, co, 1, stride))
        return self.add(y, shortcut)


def onnx_style(seed, features, c0=32, blocks=(1, 1, 1, 1), layout="nchw", out="embedding"):
    """resnet_synth.iresnet_like's network (stem, four stages, BN -> flatten -> FULLY_CONNECTED -> BN) in the writing `layout` gives it.
    out = "feature_map": the graph's output is the last stage's tensor as the layout has it (channel-first for "nchw")."""
    g = OnnxStyleBuilder(seed, [1, 112, 112, 3], layout)
    x = g.prelu(g.bn(g.conv(g.enter(g.input), c0, 3, 1)))
    for stage, nb in enumerate(blocks):
        for k in range(nb):
            x = g.res_block(x, c0 << stage, 2 if k == 0 else 1)
    x = g.bn(x)
    if out == "feature_map":
        g.outputs = [x]
        return g.finish()
    c, (h, w) = g.channels(x), (g.shape(x)[2:4] if g.cf else g.shape(x)[1:3])
    assert (h, w, c) == (7, 7, 8 * c0)
    K = h * w * c
    wfc = g._w((features, K), K)                                                   # columns in C,H,W order: what the ONNX graph stores
    w_hwc = wfc.reshape(features, c, h, w).transpose(0, 2, 3, 1).reshape(features, K)
    bfc = g.rng.standard_normal(features).astype(np.float32) * 0.1
    if layout == "twin":
        y = g.reshape(g.bn(g.conv_with(x, w_hwc.reshape(features, h, w, c), bfc, 1, VALID)), [1, features])
    else:
        y = g.bn(g.fc(g.reshape(x, [1, K]), features, weights=wfc if g.cf else w_hwc, bias=bfc))
    g.outputs = [y]
    return g.finish()
