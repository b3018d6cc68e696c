"""Reference and bounds of the bf16 convolutions (engine option "conv_bf16"), shared by tests/test_conv_bf16_cpu.py and tests/test_conv_bf16_gpu.py.

rne_bf16 is the numpy form of the rule the packer (consts.cpp, bf16_rne) and the device's v_cvt_pk_bf16_f32 follow on finite values:
    u = bits(x);  bf16 = (u + 0x7fff + ((u >> 16) & 1)) >> 16

Mode 1 ("bf16"): ref = float64 convolution of x^ = rne_bf16(x) with w^ = rne_bf16(w), plus bias, then the epilogue on the UNROUNDED f32 skip.
    S = sum |x^ w^| + |bias| + |skip|;   bound per output element  F (K + 4) 2^-24 S
    (bf16 x bf16 products are exact in f32, and an f32 sum of K products in any order obeys it; + the epilogue's adds)
Mode 2 ("bf16x3"): ref = float64 convolution of the unrounded x with w.
    S0 = sum |x w| + |bias| + |skip|;    bound  F (3 2^-18 + (3 K + 4) 2^-24) S0
    (|x - hi| <= 2^-9 |x| and |x - hi - lo| <= 2^-18 |x| for x and for w: the dropped lo w_lo term and the two residuals are at most
    3 2^-18 |x w| to first order; three exact products per k accumulate in f32)
F = 1 is derived for IEEE adds.  How a bf16 MFMA rounds inside one instruction is not documented; the observed worst ratios on the hardware
are recorded in tests/test_conv_bf16_gpu.py's docstring."""
import numpy as np

import resnet_synth as rs

F = 1.0   # see the module's docstring


def bf16_bits(x):
    """f32 array -> uint16 bf16 patterns, round to nearest even"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    """uint16 bf16 patterns -> f32"""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def rne_bf16(x):
    return bf16_value(bf16_bits(x)).reshape(np.shape(x))


def trunc_bf16(x):
    """the WRONG rounding (the low 16 bits dropped): what test_conv_bf16_cpu.py checks the bound against"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (u & np.uint32(0xffff0000)).view(np.float32).reshape(np.shape(x))


def split_bf16(x):
    """x -> (hi, lo), hi = rne_bf16(x), lo = rne_bf16(x - hi) (the subtraction in f32, as the kernel and the packer do it)"""
    x = np.asarray(x, np.float32)
    hi = rne_bf16(x)
    return hi, rne_bf16((x - hi).astype(np.float32))


def _ref_with_operands(x, cs, xc, wc):
    """rs.conv_layer_ref's float64 evaluation and magnitude sum with the convolution's operands replaced by (xc, wc); the skip stays x"""
    conv_cs = dict(cs, w=np.asarray(wc, np.float32), skip=None)
    y, bound = rs.conv_layer_ref(xc, conv_cs)          # y = conv + bias;  bound = (K + 4) 2^-24 (mag + |b|)
    K = cs["k"] ** 2 * x.shape[3]
    mag_b = bound / ((K + 4) * 2.0 ** -24)             # sum |xc wc| + |bias|
    skip = np.asarray(x, np.float64) if cs["skip"] else 0.0
    if cs["skip"] == "act_then_add":
        y = np.maximum(y, 0.0) + skip
    elif cs["skip"] == "add_then_prelu":
        y = y + skip
        y = np.where(y >= 0, y, y * cs["alpha"].astype(np.float64))
    return y, mag_b + np.abs(skip), K


def layer_ref(x, cs, mode):
    """(float64 reference, per-element bound) of rs.conv_layer's graph on x [B,h,w,c] at conv_bf16 = mode (1 or 2)"""
    if mode == 1:
        y, S, K = _ref_with_operands(x, cs, rne_bf16(x), rne_bf16(cs["w"]))
        return y, F * (K + 4) * 2.0 ** -24 * S
    assert mode == 2
    y, S0, K = _ref_with_operands(x, cs, x, cs["w"])
    return y, F * (3 * 2.0 ** -18 + (3 * K + 4) * 2.0 ** -24) * S0


def check_layer(y, x, cs, mode, what):
    ref, bound = layer_ref(x, cs, mode)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    ratio = float((np.abs(y.astype(np.float64) - ref) / bound).max())
    print("%s, conv_bf16 = %d: worst |error| / bound = %.4f (max |ref| = %.3g, K = %d)" % (what, mode, ratio, float(np.abs(ref).max()), cs["k"] ** 2 * x.shape[3]))
    assert ratio <= 1.0, (what, mode, ratio)
    return ratio
