// kernels.hip — the general-purpose HIP kernels for gfx950 (MI355X, CDNA4; 64-wide wavefronts): what runs a node that no specialised
// kernel takes (replaces the TensorFlow-Lite CPU kernels behind `interpreter.invoke()`,
// face_detection.rs:235, face_landmark.rs:265, iris_landmark.rs:203):
//   conv_generic_kernel   k x k convolution (2x2 s2, tiny-spatial heads, unaligned stems) + fused epilogue
//   pw_few_kernel         1x1 convolution to at most 4 channels (the classifier heads)
//   dw_kernel             depthwise 3x3 + bias (+activation)                       (un-fused plans only)
//   element-wise fallbacks for graphs the fuser does not recognise
// and launch_conv, which picks a convolution's kernel among these, stem_kernels.hip (the first convolution), conv_mfma_kernels.hip and
// conv_bf16_kernels.hip.  Elsewhere: block_kernels.hip ... (fused BlazeBlocks), head_kernels.hip (whole-frame convolutions), post_kernels.hip
// (SSD post-processing, landmark projection).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "launch.hpp"

namespace mi {

// ------------------------------------------------------------------------------------------------ epilogue
__device__ __forceinline__ float apply_act(float v, int act, const float* __restrict__ alpha, int c) {
    switch (act) {
        case ACT_RELU: return v > 0.f ? v : 0.f;
        case ACT_RELU6: return v < 0.f ? 0.f : (v > 6.f ? 6.f : v);
        case ACT_PRELU: return v >= 0.f ? v : alpha[c] * v;
        default: return v;
    }
}

// skip-connection value for output pixel (b, oy, ox), channel c (see ResMode in kernels.hpp)
__device__ __forceinline__ float load_res(const Epilogue& ep, int b, int oy, int ox, int Wo, int c) {
    if (ep.res_mode == RES_NONE || c >= ep.res_C) return 0.f;
    const float* r = ep.res + (long)b * ep.res_fs;
    if (ep.res_mode == RES_DIRECT) return r[((long)oy * Wo + ox) * ep.res_C + c];
    if (ep.res_mode == RES_MAXPOOL) {
        const float* p = r + ((long)(2 * oy) * ep.res_W + 2 * ox) * ep.res_C + c;
        float m0 = fmaxf(p[0], p[ep.res_C]);
        const float* q = p + (long)ep.res_W * ep.res_C;
        float m1 = fmaxf(q[0], q[ep.res_C]);
        return fmaxf(m0, m1);
    }
    // RES_UP2X: TFLite ResizeBilinear, half_pixel_centers, scale 1/2 (see resize2x_kernel)
    float iy = ((float)oy + 0.5f) * 0.5f - 0.5f, ix = ((float)ox + 0.5f) * 0.5f - 0.5f;
    int y0 = max((int)floorf(iy), 0), y1 = min((int)ceilf(iy), ep.res_H - 1);
    int x0 = max((int)floorf(ix), 0), x1 = min((int)ceilf(ix), ep.res_W - 1);
    float dy = iy - (float)y0, dx = ix - (float)x0;
    float p00 = r[((long)y0 * ep.res_W + x0) * ep.res_C + c], p01 = r[((long)y0 * ep.res_W + x1) * ep.res_C + c];
    float p10 = r[((long)y1 * ep.res_W + x0) * ep.res_C + c], p11 = r[((long)y1 * ep.res_W + x1) * ep.res_C + c];
    return p00 * (1 - dy) * (1 - dx) + p10 * dy * (1 - dx) + p01 * (1 - dy) * dx + p11 * dy * dx;
}

// ------------------------------------------------------------------------------------------------ generic conv
// One thread = one output pixel x 4 consecutive output channels.  Threads of a wave that share a pixel read the
// same input scalar (broadcast) and consecutive float4s of the [KH][KW][C][Cop] filter (coalesced, L1/L2 resident).
__global__ __launch_bounds__(256) void conv_generic_kernel(ConvArgs a) {
    const int G = a.Cop >> 2;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)a.B * a.Ho * a.Wo * G;
    if (idx >= total) return;
    int g = (int)(idx % G);
    long p = idx / G;
    int ox = (int)(p % a.Wo);
    long q = p / a.Wo;
    int oy = (int)(q % a.Ho);
    int b = (int)(q / a.Ho);
    const float* in = a.in + (long)b * a.in_fs;
    const bool vec4 = (a.C & 3) == 0 && (a.in_fs & 3) == 0 && (reinterpret_cast<uintptr_t>(a.in) & 15) == 0;  // same accumulation order either way
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int ky = 0; ky < a.KH; ky++) {
        int iy = oy * a.sh - a.pt + ky;
        if (iy < 0 || iy >= a.H) continue;
        for (int kx = 0; kx < a.KW; kx++) {
            int ix = ox * a.sw - a.pl + kx;
            if (ix < 0 || ix >= a.W) continue;
            const float* ip = in + ((long)iy * a.W + ix) * a.C;
            const float4* wp = reinterpret_cast<const float4*>(a.w + ((long)(ky * a.KW + kx) * a.C) * a.Cop) + g;
            int c = 0;
            if (vec4) {  // the pixel's channels as float4s (front / short: 36 -> 42 and 42 -> 48 channels, which no fused kernel takes)
                for (; c + 4 <= a.C; c += 4) {
                    const float4 x = *reinterpret_cast<const float4*>(ip + c);
                    const float4 w0 = wp[(long)c * G], w1 = wp[(long)(c + 1) * G], w2 = wp[(long)(c + 2) * G], w3 = wp[(long)(c + 3) * G];
                    acc.x = fmaf(x.x, w0.x, acc.x); acc.y = fmaf(x.x, w0.y, acc.y); acc.z = fmaf(x.x, w0.z, acc.z); acc.w = fmaf(x.x, w0.w, acc.w);
                    acc.x = fmaf(x.y, w1.x, acc.x); acc.y = fmaf(x.y, w1.y, acc.y); acc.z = fmaf(x.y, w1.z, acc.z); acc.w = fmaf(x.y, w1.w, acc.w);
                    acc.x = fmaf(x.z, w2.x, acc.x); acc.y = fmaf(x.z, w2.y, acc.y); acc.z = fmaf(x.z, w2.z, acc.z); acc.w = fmaf(x.z, w2.w, acc.w);
                    acc.x = fmaf(x.w, w3.x, acc.x); acc.y = fmaf(x.w, w3.y, acc.y); acc.z = fmaf(x.w, w3.z, acc.z); acc.w = fmaf(x.w, w3.w, acc.w);
                }
            }
            for (; c < a.C; c++) {
                float x = ip[c];
                float4 w = wp[(long)c * G];
                acc.x = fmaf(x, w.x, acc.x);
                acc.y = fmaf(x, w.y, acc.y);
                acc.z = fmaf(x, w.z, acc.z);
                acc.w = fmaf(x, w.w, acc.w);
            }
        }
    }
    float v[4] = {acc.x, acc.y, acc.z, acc.w};
    float* op = a.out + (long)b * a.out_fs + ((long)oy * a.Wo + ox) * a.Co;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int c = 4 * g + j;
        if (c < a.Co) {
            float r = v[j] + (a.ep.bias ? a.ep.bias[c] : 0.f);
            const float sk = load_res(a.ep, b, oy, ox, a.Wo, c);
            if (!a.ep.res_after) r += sk;
            r = apply_act(r, a.ep.act, a.ep.alpha, c);
            if (a.ep.res_after) r += sk;
            op[c] = r;
        }
    }
}


// Pointwise convolution to at most 4 output channels (the classifier heads: 48 -> 1 at 48x48 in full_range, 88 -> 2 in front / short):
// one thread = one pixel, its C input channels read as float4s, the [C][4] filter through the scalar cache.  (The generic kernel above
// reads the pixel scalar by scalar: 48 four-byte loads 192 bytes apart per lane.)
__global__ __launch_bounds__(256) void pw_few_kernel(ConvArgs a) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per_frame = (long)a.Ho * a.Wo;
    if (p >= (long)a.B * per_frame) return;
    const int b = (int)(p / per_frame);
    const long q = p - (long)b * per_frame;
    const int oy = (int)(q / a.Wo), ox = (int)(q - (long)oy * a.Wo);
    const float* ip = a.in + (long)b * a.in_fs + q * a.C;
    const float4* __restrict__ w = reinterpret_cast<const float4*>(a.w);  // [C][Cop = 4], uniform
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < a.C; j += 4) {
        const float4 x = *reinterpret_cast<const float4*>(ip + j);
        const float4 w0 = w[j], w1 = w[j + 1], w2 = w[j + 2], w3 = w[j + 3];
        acc.x = fmaf(x.x, w0.x, acc.x); acc.y = fmaf(x.x, w0.y, acc.y); acc.z = fmaf(x.x, w0.z, acc.z); acc.w = fmaf(x.x, w0.w, acc.w);
        acc.x = fmaf(x.y, w1.x, acc.x); acc.y = fmaf(x.y, w1.y, acc.y); acc.z = fmaf(x.y, w1.z, acc.z); acc.w = fmaf(x.y, w1.w, acc.w);
        acc.x = fmaf(x.z, w2.x, acc.x); acc.y = fmaf(x.z, w2.y, acc.y); acc.z = fmaf(x.z, w2.z, acc.z); acc.w = fmaf(x.z, w2.w, acc.w);
        acc.x = fmaf(x.w, w3.x, acc.x); acc.y = fmaf(x.w, w3.y, acc.y); acc.z = fmaf(x.w, w3.z, acc.z); acc.w = fmaf(x.w, w3.w, acc.w);
    }
    const float v[4] = {acc.x, acc.y, acc.z, acc.w};
    float* op = a.out + (long)b * a.out_fs + q * a.Co;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (j < a.Co) {
            float r = v[j] + (a.ep.bias ? a.ep.bias[j] : 0.f);
            const float sk = load_res(a.ep, b, oy, ox, a.Wo, j);
            if (!a.ep.res_after) r += sk;
            r = apply_act(r, a.ep.act, a.ep.alpha, j);
            if (a.ep.res_after) r += sk;
            op[j] = r;
        }
}

static bool pw_few_applicable(const ConvArgs& a) {
    return a.KH == 1 && a.KW == 1 && a.sh == 1 && a.sw == 1 && a.Cop == 4 && a.C % 4 == 0 && a.H == a.Ho && a.W == a.Wo && (a.in_fs & 3) == 0 &&
           (reinterpret_cast<uintptr_t>(a.in) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.w) & 15) == 0;
}
bool conv_takes_u8(const ConvArgs& a) { return stem_applicable(a); }

// which kernel takes this convolution: the one decision behind conv_kernel_label and launch_conv
enum class ConvForm { Bf16, Mfma, StemMfma, Stem, PwFew, Generic };
static ConvForm conv_form(const ConvArgs& a) {
    if (conv_bf16_supports(a)) return ConvForm::Bf16;
    if (conv_mfma_supports(a)) return ConvForm::Mfma;
    if (stem_applicable(a)) return stem_mfma_applicable(a) ? ConvForm::StemMfma : ConvForm::Stem;
    return pw_few_applicable(a) ? ConvForm::PwFew : ConvForm::Generic;
}

const char* conv_kernel_label(const ConvArgs& a) {
    switch (conv_form(a)) {
        case ConvForm::Bf16: return "conv_bf16_kernel";
        case ConvForm::Mfma: return "conv_mfma_kernel";
        case ConvForm::StemMfma: return "stem_mfma_kernel";   // (either MFMA form)
        case ConvForm::Stem: return "stem_conv_kernel";
        case ConvForm::PwFew: return "pw_few_kernel";
        default: return "conv_generic_kernel";
    }
}

int launch_conv(const ConvArgs& a, void* stream) {
    const ConvForm form = conv_form(a);
    switch (form) {
        case ConvForm::Bf16: return launch_conv_bf16(a, stream);
        case ConvForm::Mfma: return launch_conv_mfma(a, stream);
        case ConvForm::StemMfma: case ConvForm::Stem: return launch_stem_conv(a, stream);
        default: break;
    }
    long total = (long)a.B * a.Ho * a.Wo * (a.Cop >> 2);
    if (total <= 0) return 0;
    unsigned blocks = (unsigned)((total + 255) / 256);
    return (int)launch_kernel(form == ConvForm::PwFew ? pw_few_kernel : conv_generic_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
}

// ------------------------------------------------------------------------------------------------ depthwise 3x3
// One thread = one output pixel x V consecutive channels (V = 4/2/1 by alignment).  HBM-bound: 9 MAC per 8 bytes.
template <int V>
__global__ __launch_bounds__(256) void dw_kernel(DwArgs a) {
    const int G = a.C / V;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)a.B * a.Ho * a.Wo * G;
    if (idx >= total) return;
    int g = (int)(idx % G);
    long p = idx / G;
    int ox = (int)(p % a.Wo);
    long q = p / a.Wo;
    int oy = (int)(q % a.Ho);
    int b = (int)(q / a.Ho);
    const float* in = a.in + (long)b * a.in_fs + g * V;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; j++) acc[j] = 0.f;
    for (int ky = 0; ky < a.KH; ky++) {
        int iy = oy * a.sh - a.pt + ky;
        if (iy < 0 || iy >= a.H) continue;
        for (int kx = 0; kx < a.KW; kx++) {
            int ix = ox * a.sw - a.pl + kx;
            if (ix < 0 || ix >= a.W) continue;
            const float* ip = in + ((long)iy * a.W + ix) * a.C;
            const float* wp = a.w + (long)(ky * a.KW + kx) * a.C + g * V;
#pragma unroll
            for (int j = 0; j < V; j++) acc[j] = fmaf(ip[j], wp[j], acc[j]);
        }
    }
    float* op = a.out + (long)b * a.out_fs + ((long)oy * a.Wo + ox) * a.C + g * V;
#pragma unroll
    for (int j = 0; j < V; j++) {
        int c = g * V + j;
        float r = acc[j] + (a.ep.bias ? a.ep.bias[c] : 0.f);
        r += load_res(a.ep, b, oy, ox, a.Wo, c);
        op[j] = apply_act(r, a.ep.act, a.ep.alpha, c);
    }
}

int launch_dw(const DwArgs& a, void* stream) {
    int V = (a.C % 4 == 0) ? 4 : (a.C % 2 == 0 ? 2 : 1);
    long total = (long)a.B * a.Ho * a.Wo * (a.C / V);
    if (total <= 0) return 0;
    unsigned blocks = (unsigned)((total + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    if (V == 4) return (int)launch_kernel(dw_kernel<4>, dim3(blocks), dim3(256), 0, s, a);
    if (V == 2) return (int)launch_kernel(dw_kernel<2>, dim3(blocks), dim3(256), 0, s, a);
    return (int)launch_kernel(dw_kernel<1>, dim3(blocks), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------------------------ element-wise fallbacks
__global__ void add_kernel(EltArgs a) {  // out = act(a + b), same shape
    long per = (long)a.H * a.W * a.C;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * a.B) return;
    int b = (int)(idx / per);
    long e = idx % per;
    float v = a.a[(long)b * a.a_fs + e] + a.b[(long)b * a.b_fs + e];
    a.out[(long)b * a.out_fs + e] = apply_act(v, a.act, a.alpha, (int)(e % a.C));
}
__global__ void act_kernel(EltArgs a) {
    long per = (long)a.H * a.W * a.C;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * a.B) return;
    int b = (int)(idx / per);
    long e = idx % per;
    a.out[(long)b * a.out_fs + e] = apply_act(a.a[(long)b * a.a_fs + e], a.act, a.alpha, (int)(e % a.C));
}
// Per-channel affine, out = act(x * scale[c] + shift[c]) with b = scale, c the last dimension: a MUL and an ADD by constants (a batch normalisation nothing
// could fold) and the activation behind them as ONE launch.  A separate multiply and add, each rounded, not an fma: the bits of TFLite's two operators.
// V = 4: float4 accesses (C, the frame strides and the pointers allow it).
// DIV: the divisor form, out = act(x / d[c] + shift[c]) with b = d — a DIV by constants that are not powers of two is a true, correctly rounded division.
template <int V, bool DIV = false>
__global__ __launch_bounds__(256) void affine_kernel(EltArgs a) {
    const long per = (long)a.H * a.W * a.C / V;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * a.B) return;
    const int b = (int)(idx / per);
    const long e = (idx % per) * V;
    const int c = (int)(e % a.C);
    const float* x = a.a + (long)b * a.a_fs + e;
    float* o = a.out + (long)b * a.out_fs + e;
    if (V == 4) {
        const float4 xv = *reinterpret_cast<const float4*>(x), s = *reinterpret_cast<const float4*>(a.b + c), t = *reinterpret_cast<const float4*>(a.shift + c);
        float4 r;
        r.x = apply_act(__fadd_rn(DIV ? __fdiv_rn(xv.x, s.x) : __fmul_rn(xv.x, s.x), t.x), a.act, a.alpha, c);
        r.y = apply_act(__fadd_rn(DIV ? __fdiv_rn(xv.y, s.y) : __fmul_rn(xv.y, s.y), t.y), a.act, a.alpha, c + 1);
        r.z = apply_act(__fadd_rn(DIV ? __fdiv_rn(xv.z, s.z) : __fmul_rn(xv.z, s.z), t.z), a.act, a.alpha, c + 2);
        r.w = apply_act(__fadd_rn(DIV ? __fdiv_rn(xv.w, s.w) : __fmul_rn(xv.w, s.w), t.w), a.act, a.alpha, c + 3);
        *reinterpret_cast<float4*>(o) = r;
    } else {
        *o = apply_act(__fadd_rn(DIV ? __fdiv_rn(*x, a.b[c]) : __fmul_rn(*x, a.b[c]), a.shift[c]), a.act, a.alpha, c);
    }
}
// MAX_POOL_2D: p0 = filter_h, p1 = filter_w, p2 = stride_h, p3 = stride_w; SAME/VALID pads folded into Ho/Wo + H/W clip
__global__ void maxpool_kernel(EltArgs a, int pt, int pl) {
    long per = (long)a.Ho * a.Wo * a.C;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * a.B) return;
    int b = (int)(idx / per);
    long e = idx % per;
    int c = (int)(e % a.C);
    int ox = (int)((e / a.C) % a.Wo), oy = (int)(e / ((long)a.C * a.Wo));
    float m = -INFINITY;
    for (int ky = 0; ky < a.p0; ky++) {
        int iy = oy * a.p2 - pt + ky;
        if (iy < 0 || iy >= a.H) continue;
        for (int kx = 0; kx < a.p1; kx++) {
            int ix = ox * a.p3 - pl + kx;
            if (ix < 0 || ix >= a.W) continue;
            m = fmaxf(m, a.a[(long)b * a.a_fs + ((long)iy * a.W + ix) * a.C + c]);
        }
    }
    a.out[(long)b * a.out_fs + e] = m;
}
// PAD with zeros: p0 = top, p1 = left, p2 = channel-before; output dims Ho, Wo, Co
__global__ void pad_kernel(EltArgs a) {
    long per = (long)a.Ho * a.Wo * a.Co;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * a.B) return;
    int b = (int)(idx / per);
    long e = idx % per;
    int c = (int)(e % a.Co) - a.p2;
    int x = (int)((e / a.Co) % a.Wo) - a.p1, y = (int)(e / ((long)a.Co * a.Wo)) - a.p0;
    float v = 0.f;
    if (c >= 0 && c < a.C && x >= 0 && x < a.W && y >= 0 && y < a.H) v = a.a[(long)b * a.a_fs + ((long)y * a.W + x) * a.C + c];
    a.out[(long)b * a.out_fs + e] = v;
}
// RESIZE_BILINEAR (half_pixel_centers = p0, align_corners = p1), arbitrary sizes; TFLite reference formula.
__global__ void resize_kernel(EltArgs a) {
    long per = (long)a.Ho * a.Wo * a.C;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * a.B) return;
    int b = (int)(idx / per);
    long e = idx % per;
    int c = (int)(e % a.C);
    int ox = (int)((e / a.C) % a.Wo), oy = (int)(e / ((long)a.C * a.Wo));
    float hs = (a.p1 && a.Ho > 1) ? (float)(a.H - 1) / (float)(a.Ho - 1) : (float)a.H / (float)a.Ho;
    float ws = (a.p1 && a.Wo > 1) ? (float)(a.W - 1) / (float)(a.Wo - 1) : (float)a.W / (float)a.Wo;
    float iy = a.p0 ? ((float)oy + 0.5f) * hs - 0.5f : (float)oy * hs;
    float ix = a.p0 ? ((float)ox + 0.5f) * ws - 0.5f : (float)ox * ws;
    int y0 = max((int)floorf(iy), 0), y1 = min((int)ceilf(iy), a.H - 1);
    int x0 = max((int)floorf(ix), 0), x1 = min((int)ceilf(ix), a.W - 1);
    float dy = iy - (float)y0, dx = ix - (float)x0;
    const float* r = a.a + (long)b * a.a_fs;
    float p00 = r[((long)y0 * a.W + x0) * a.C + c], p01 = r[((long)y0 * a.W + x1) * a.C + c];
    float p10 = r[((long)y1 * a.W + x0) * a.C + c], p11 = r[((long)y1 * a.W + x1) * a.C + c];
    a.out[(long)b * a.out_fs + e] = p00 * (1 - dy) * (1 - dx) + p10 * dy * (1 - dx) + p01 * (1 - dy) * dx + p11 * dy * dx;
}
// DEPTH_TO_SPACE: p0 = block size
__global__ void d2s_kernel(EltArgs a) {
    long per = (long)a.Ho * a.Wo * a.Co;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * a.B) return;
    int b = (int)(idx / per);
    long e = idx % per;
    int c = (int)(e % a.Co);
    int ox = (int)((e / a.Co) % a.Wo), oy = (int)(e / ((long)a.Co * a.Wo));
    int bs = a.p0;
    int iy = oy / bs, ix = ox / bs, ic = ((oy % bs) * bs + (ox % bs)) * a.Co + c;
    a.out[(long)b * a.out_fs + e] = a.a[(long)b * a.a_fs + ((long)iy * a.W + ix) * a.C + ic];
}
// strided frame copy: per-frame `C` floats (H = W = 1)
__global__ void copy_kernel(EltArgs a) {
    long per = (long)a.C;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * a.B) return;
    int b = (int)(idx / per);
    long e = idx % per;
    a.out[(long)b * a.out_fs + e] = a.a[(long)b * a.a_fs + e];
}

static inline unsigned nblocks(long n) { return (unsigned)((n + 255) / 256); }
int launch_add(const EltArgs& a, void* s) {
    long n = (long)a.B * a.H * a.W * a.C;
    return n > 0 ? (int)launch_kernel(add_kernel, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)s, a) : 0;
}
int launch_act(const EltArgs& a, void* s) {
    if (a.shift) return launch_affine(a, s);   // a per-channel affine with its activation (Node::Affine)
    long n = (long)a.B * a.H * a.W * a.C;
    return n > 0 ? (int)launch_kernel(act_kernel, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)s, a) : 0;
}
int launch_affine(const EltArgs& a, void* s) {
    const long n = (long)a.B * a.H * a.W * a.C;
    if (n <= 0) return 0;
    if (!a.b || !a.shift || (a.act == ACT_PRELU && !a.alpha)) return (int)hipErrorInvalidValue;
    const bool v4 = a.C % 4 == 0 && a.a_fs % 4 == 0 && a.out_fs % 4 == 0 && aligned16(a.a) && aligned16(a.out) && aligned16(a.b) && aligned16(a.shift);
    if (a.div) {
        if (v4) return (int)launch_kernel(affine_kernel<4, true>, dim3(nblocks(n / 4)), dim3(256), 0, (hipStream_t)s, a);
        return (int)launch_kernel(affine_kernel<1, true>, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)s, a);
    }
    if (v4) return (int)launch_kernel(affine_kernel<4>, dim3(nblocks(n / 4)), dim3(256), 0, (hipStream_t)s, a);
    return (int)launch_kernel(affine_kernel<1>, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)s, a);
}
int launch_maxpool(const EltArgs& a, void* s) {
    long n = (long)a.B * a.Ho * a.Wo * a.C;
    // TF SAME pads (only non-zero for odd inputs): total = max(0,(out-1)*stride + filter - in), before = total/2
    int tph = (a.Ho - 1) * a.p2 + a.p0 - a.H, tpw = (a.Wo - 1) * a.p3 + a.p1 - a.W;
    int pt = tph > 0 ? tph / 2 : 0, pl = tpw > 0 ? tpw / 2 : 0;
    return n > 0 ? (int)launch_kernel(maxpool_kernel, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)s, a, pt, pl) : 0;
}
int launch_padc(const EltArgs& a, void* s) {
    long n = (long)a.B * a.Ho * a.Wo * a.Co;
    return n > 0 ? (int)launch_kernel(pad_kernel, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)s, a) : 0;
}
int launch_resize2x(const EltArgs& a, void* s) {
    long n = (long)a.B * a.Ho * a.Wo * a.C;
    return n > 0 ? (int)launch_kernel(resize_kernel, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)s, a) : 0;
}
int launch_depth_to_space(const EltArgs& a, void* s) {
    long n = (long)a.B * a.Ho * a.Wo * a.Co;
    return n > 0 ? (int)launch_kernel(d2s_kernel, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)s, a) : 0;
}
int launch_copy_strided(const EltArgs& a, void* s) {
    long n = (long)a.B * a.C;
    return n > 0 ? (int)launch_kernel(copy_kernel, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)s, a) : 0;
}

// One wave that does nothing for `ticks` of the 100 MHz wall clock (bounded: it leaves after `max_iters` looks at the clock whatever the
// clock says).  mi_streams_create_distinct launches it on several streams at once: streams that share a hardware queue run it one after
// the other, streams on different queues side by side.
__global__ void spin_kernel(long long ticks, int max_iters, int* sink) {
    const long long t0 = wall_clock64();
    int it = 0;
    while (wall_clock64() - t0 < ticks && ++it < max_iters) __builtin_amdgcn_s_sleep(8);
    if (ticks < 0) *sink = it;
}

int launch_spin(long long ticks, int max_iters, int* sink, void* stream) {
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ticks, max_iters, sink);
    return (int)hipGetLastError();
}

}  // namespace mi
