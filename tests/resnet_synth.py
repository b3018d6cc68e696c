"""Synthetic ResNet-style embedding networks (test infrastructure; tools/resnet_probe.py measures them): the operator family of an ArcFace
.tflite — dense 3x3 CONV_2D, unfolded batch normalisation (MUL / ADD by per-channel constants), PRELU, a FULLY_CONNECTED head — on top of
synth_tflite.GraphBuilder, single-layer graphs for the convolution kernel tests, and the float64 restatement of one layer those tests compare
against.  Every network also has a `twin`: the same constants, drawn from the generator in the same order, written with operators the oracle
runs (MUL / ADD pairs as 1x1 DEPTHWISE_CONV_2D with filter = scale and bias = shift, the FULLY_CONNECTED as the VALID whole-frame CONV_2D)."""
import numpy as np

from synth_tflite import ACT_NONE, ADD, CONV_2D, DEPTHWISE_CONV_2D, OPT_ADD, OPT_CONV, OPT_DW, SAME, VALID, GraphBuilder

FULLY_CONNECTED, MUL = 9, 18
OPT_FC, OPT_MUL = 8, 21


class ResnetBuilder(GraphBuilder):
    def __init__(self, seed, in_shape, twin=False):
        super().__init__(seed, in_shape)
        self.twin = twin

    # ---- the three new operators
    def fc(self, x, n, act=ACT_NONE, weights_format=0, keep_num_dims=False, k=None, weights=None, bias=None):
        """FULLY_CONNECTED (code 9, options tag 8) to [1, n]; k: the weights' second dimension when it shall differ from the input's size"""
        size = int(np.prod(self.shape(x)))
        k = size if k is None else k
        wt = self.const(self._w((n, k), k) if weights is None else weights, "wfc")
        bt = self.const(self.rng.standard_normal(n).astype(np.float32) * 0.1 if bias is None else bias, "bfc")
        y = self._act([1, n], "fc")
        self.ops.append((FULLY_CONNECTED, [x, wt, bt], [y], OPT_FC, [("i8", act), ("i8", weights_format), ("u8", 1 if keep_num_dims else 0)]))
        return y

    def mul_const(self, x, c=None, const_first=False):
        """MUL (code 18, options tag 21) by a constant: per channel, uniform in [0.5, 1.5], unless c is given"""
        c = self.rng.uniform(0.5, 1.5, self.shape(x)[-1]).astype(np.float32) if c is None else c
        ct = self.const(c, "scale")
        y = self._act(self.shape(x), "mul")
        self.ops.append((MUL, [ct, x] if const_first else [x, ct], [y], OPT_MUL, [("i8", ACT_NONE)]))
        return y

    def add_const(self, x, c=None, const_first=False):
        """ADD with a constant: per channel, 0.1 N(0, 1), unless c is given"""
        c = (0.1 * self.rng.standard_normal(self.shape(x)[-1])).astype(np.float32) if c is None else c
        ct = self.const(c, "shift")
        y = self._act(self.shape(x), "addc")
        self.ops.append((ADD, [ct, x] if const_first else [x, ct], [y], OPT_ADD, [("i8", ACT_NONE)]))
        return y

    def mul(self, a, b):
        y = self._act(self.shape(a), "mul")
        self.ops.append((MUL, [a, b], [y], OPT_MUL, [("i8", ACT_NONE)]))
        return y

    # ---- batch normalisation as the converter leaves it (twin: the same two constants as a 1x1 depthwise convolution)
    def bn(self, x):
        c = self.shape(x)[-1]
        scale = self.rng.uniform(0.5, 1.5, c).astype(np.float32)
        shift = (0.1 * self.rng.standard_normal(c)).astype(np.float32)
        if not self.twin:
            return self.add_const(self.mul_const(x, scale), shift)
        wt, bt = self.const(scale.reshape(1, 1, 1, c), "wd"), self.const(shift, "bd")
        y = self._act(self.shape(x), "dw")
        self.ops.append((DEPTHWISE_CONV_2D, [x, wt, bt], [y], OPT_DW, [("i8", SAME), ("i32", 1), ("i32", 1), ("i32", 1), ("i8", ACT_NONE)]))
        return y

    def conv_with(self, x, w, b, stride=1, padding=SAME, act=ACT_NONE):
        """CONV_2D with the given filter [co, k, k, c] and bias"""
        n, h, wd, c = self.shape(x)
        co, k = w.shape[0], w.shape[1]
        wt, bt = self.const(w, "w"), self.const(b, "b")
        ho, wo = ((h + stride - 1) // stride, (wd + stride - 1) // stride) if padding == SAME else ((h - k) // stride + 1, (wd - k) // stride + 1)
        y = self._act([n, ho, wo, co], "conv")
        self.ops.append((CONV_2D, [x, wt, bt], [y], OPT_CONV, [("i8", padding), ("i32", stride), ("i32", stride), ("i8", act)]))
        return y

    def res_block(self, x, co, stride):
        """BN -> 3x3 -> BN -> PReLU -> 3x3 stride s -> BN, plus the shortcut: the identity, or 1x1 stride s -> BN when the shape changes"""
        c = self.shape(x)[3]
        y = self.bn(self.conv(self.bn(x), co, 3, 1))
        y = self.bn(self.conv(self.prelu(y), co, 3, stride))
        shortcut = x if stride == 1 and c == co else self.bn(self.conv(x, co, 1, stride))
        return self.add(y, shortcut)


def iresnet_like(seed, features, c0=32, blocks=(1, 1, 1, 1), twin=False):
    """stem 3x3 s1 3 -> c0, BN, PReLU; four stages of widths c0 (1, 2, 4, 8), the first block of each with stride 2 (112 -> 56 -> 28 -> 14 -> 7);
    BN -> RESHAPE [1, 49 * 8 c0] -> FC(features) -> BN."""
    g = ResnetBuilder(seed, [1, 112, 112, 3], twin)
    x = g.prelu(g.bn(g.conv(g.input, c0, 3, 1)))
    for stage, nb in enumerate(blocks):
        for k in range(nb):
            x = g.res_block(x, c0 << stage, 2 if k == 0 else 1)
    x = g.bn(x)
    _, h, w, c = g.shape(x)
    assert (h, w, c) == (7, 7, 8 * c0)
    K = h * w * c
    wfc = g._w((features, K), K)
    bfc = g.rng.standard_normal(features).astype(np.float32) * 0.1
    if twin:
        y = g.bn(g.conv_with(x, wfc.reshape(features, h, w, c), bfc, 1, VALID))
        y = g.reshape(y, [1, features])
    else:
        y = g.bn(g.fc(g.reshape(x, [1, K]), features, weights=wfc, bias=bfc))
    g.outputs = [y]
    return g.finish()


def affine_launches(blocks, fuse):
    """Affine launches the lowering leaves of iresnet_like(blocks=blocks): at level 0 every MUL and every ADD by a constant is one launch (the
    stem's pair, three pairs a block, the shortcut's pair where the shape changes, the pair in front of the RESHAPE, the pair behind the FC);
    from level 1 on a pair is one affine, and the affines behind a convolution / the FC fold into it: what remains is the BN at the head of
    every block (its input has two readers and no convolution in front) and the BN in front of the RESHAPE (behind the last block's ADD)."""
    nblocks = sum(blocks)
    shortcuts = len(blocks)   # the first block of every stage has stride 2
    if fuse == 0:
        return 2 * (1 + 3 * nblocks + shortcuts + 2)
    return nblocks + 1


# ---------------------------------------------------------------------------------------------------- single layers
def conv_layer(seed, h, w, c, co, k=3, stride=1, padding=SAME, explicit_pad=None, skip=None):
    """input [1,h,w,c] -> one CONV_2D (explicit_pad = (top, bottom, left, right): a spatial PAD in front of it); skip: None, "act_then_add" (the
    convolution's fused RELU, then ADD of the input: the skip joins behind the activation) or "add_then_prelu".  Returns (blob, constants)."""
    g = ResnetBuilder(seed, [1, h, w, c])
    wt = g._w((co, k, k, c), k * k * c)
    bt = g.rng.standard_normal(co).astype(np.float32) * 0.1
    x = g.input if explicit_pad is None else g.pad_spatial(g.input, *explicit_pad)
    y = g.conv_with(x, wt, bt, stride, padding, act=1 if skip == "act_then_add" else ACT_NONE)
    consts = dict(w=wt, b=bt, k=k, stride=stride, padding=padding, explicit_pad=explicit_pad, skip=skip, alpha=None)
    if skip == "act_then_add":
        y = g.add(y, g.input)
    elif skip == "add_then_prelu":
        y = g.prelu(g.add(y, g.input))
        consts["alpha"] = np.frombuffer(g.buffers[g.tensors[g.ops[-1][1][1]][1]], np.float32).copy()
    g.outputs = [y]
    return g.finish(), consts


def conv_layer_ref(x, cs):
    """float64 evaluation of conv_layer's graph on x [B,h,w,c] from the same constants, and the per-element bound
    (K + 4) 2^-24 (sum |x w| + |bias| + |skip|): the standard bound of an f32 sum of K products in any order, plus the epilogue's adds."""
    x = np.asarray(x, np.float64)
    w, b, k, s = cs["w"].astype(np.float64), cs["b"].astype(np.float64), cs["k"], cs["stride"]
    B, H, W, C = x.shape
    if cs["explicit_pad"] is not None:
        t, bo, l, r = cs["explicit_pad"]
    elif cs["padding"] == SAME:
        ho, wo = (H + s - 1) // s, (W + s - 1) // s
        th, tw = max(0, (ho - 1) * s + k - H), max(0, (wo - 1) * s + k - W)
        t, l = th // 2, tw // 2
        bo, r = th - t, tw - l
    else:
        t = bo = l = r = 0
    xp = np.zeros((B, H + t + bo, W + l + r, C))
    xp[:, t:t + H, l:l + W] = x
    ho, wo = (xp.shape[1] - k) // s + 1, (xp.shape[2] - k) // s + 1
    acc, mag = np.zeros((B, ho, wo, w.shape[0])), np.zeros((B, ho, wo, w.shape[0]))
    for ky in range(k):
        for kx in range(k):
            win = xp[:, ky:ky + (ho - 1) * s + 1:s, kx:kx + (wo - 1) * s + 1:s]
            acc += win @ w[:, ky, kx].T
            mag += np.abs(win) @ np.abs(w[:, ky, kx]).T
    y = acc + b
    skip = x if cs["skip"] else 0.0
    if cs["skip"] == "act_then_add":
        y = np.maximum(y, 0.0) + skip
    elif cs["skip"] == "add_then_prelu":
        y = y + skip
        y = np.where(y >= 0, y, y * cs["alpha"].astype(np.float64))
    bound = (k * k * C + 4) * 2.0 ** -24 * (mag + np.abs(b) + np.abs(skip))
    return y, bound


def affine_graph(seed, c, h=5, w=7):
    """input -> MUL -> ADD -> PRELU as the only operators.  Returns (blob, scale, shift, alpha)."""
    g = ResnetBuilder(seed, [1, h, w, c])
    scale = g.rng.uniform(0.5, 1.5, c).astype(np.float32)
    shift = (0.1 * g.rng.standard_normal(c)).astype(np.float32)
    y = g.prelu(g.add_const(g.mul_const(g.input, scale), shift))
    alpha = np.frombuffer(g.buffers[g.tensors[g.ops[-1][1][1]][1]], np.float32).copy()
    g.outputs = [y]
    return g.finish(), scale, shift, alpha


def fold_graph(seed, h=6, w=5, c=32, co=8):
    """conv 3x3 -> MUL -> ADD -> PRELU (the PRELU keeps the folded convolution's output off the graph outputs' rule).  Returns (blob, w, b, s, t)."""
    g = ResnetBuilder(seed, [1, h, w, c])
    wt = g._w((co, 3, 3, c), 9 * c)
    bt = g.rng.standard_normal(co).astype(np.float32) * 0.1
    s = g.rng.uniform(0.5, 1.5, co).astype(np.float32)
    t = (0.1 * g.rng.standard_normal(co)).astype(np.float32)
    y = g.add_const(g.mul_const(g.conv_with(g.input, wt, bt), s), t)
    g.outputs = [g.prelu(y)]
    return g.finish(), wt, bt, s, t


def odd_width_graph(seed):
    """30-channel tensors around a normalisation that cannot fold (its producer has an activation, its output two readers): pad_odd_channels
    widens them to 32, the MUL's constant with ones and the ADD's with zeros."""
    g = ResnetBuilder(seed, [1, 16, 16, 3])
    x = g.prelu(g.conv(g.input, 30, 3, 2))
    x = g.bn(x)
    x = g.blaze_block(x, act="prelu")
    g.outputs = [g.conv(x, 8)]
    return g.finish()
