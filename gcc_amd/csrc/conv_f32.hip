// Inference convolution in fp32 on the f32-input matrix instruction: five entries, one tile (conv_f32_tile.hpp: the implicit GEMM,
// its LDS layout, its k loop and the single order of K).  A kernel here is its gather and its store, as macros, around the one
// body text (conv_f32_tile_body.inc).
//
// conv_f32_kernel   Conv2d with zero padding; stride and dilation are index arithmetic, taps outside the image are zeros
//   gcc_conv_eval_f32      square 1 / 3 / 7 kernels with "same" padding, residual and ReLU: the evaluator networks at the
//                          reference's own precision (gcc_amd/metric/drn_seg.py, precision 'fp32')
//   gcc_conv_eval_f32_ex   KH, KW and the two paddings independent (gcc_amd/metric/inception_fid.py, precision 'fp32': 5 x 5,
//                          (1, 7) / (7, 1), padding 0)
//   gcc_conv_eval_f32_act  (EXT) sides up to 9, PReLU (a device slope) and tanh in the epilogue, and an optional PixelShuffle(2)
//                          store: SRResNet at the reference's own precision (engine.SRResNetEngine.infer, precision 'fp32').  With
//                          the shuffle a 32-lane store group (32 consecutive channels of one pixel) puts 8 consecutive floats on
//                          each of the 4 sub-pixels.
// conv_f32_unet_kernel   gcc_conv_eval_f32_unet: the U-Net generator's k4 s2 p1 layers at the reference's own precision
//   (engine.UnetEngine.infer, precision 'fp32').  Forward it gathers the 16 taps of Conv2d; transposed, blockIdx.z is one of the
//   four output parity phases, each a 2 x 2-tap gather over the input (K = 4 Ci) whose tile is stored at pixel stride 2.  The store
//   writes up to two activated copies of fmaf(acc, scale, shift): none / ReLU / LeakyReLU (a host slope) / tanh.
// The fifth entry, gcc_conv_eval_f32_resnet, is in resnet_f32.hip.
#include "conv_f32_tile.hpp"

namespace {

struct ConvF32Args {
    const float* x; const float* w; float* y;
    const float* scale; const float* shift; const float* res;
    int M, H, W, Ho, Wo, Ci, Cip, Co, KW, stride, pad_h, pad_w, dil;
    int ldx, xoff, ldy, yoff, ldr, roff, Kreal, Kp, relu;
    FastDiv dWo, dHo, dCip, dKW;
    const float* slope; int act, shuffle;           // EXT only (gcc_conv_eval_f32_act)
};

// row m is output pixel (n, oh, ow); tap = kh KW + kw reads (oh stride - pad_h + kh dil, ow stride - pad_w + kw dil), zeros outside the
// map.  The store is act(z + residual); EXT = false is that of gcc_conv_eval_f32 / _ex, EXT = true that of gcc_conv_eval_f32_act.
// a: the kernel's ConvF32Args in each of them.
#define CF_ROW(m, ih0, iw0, nb)                                                                        \
    const int q = fdiv(m, a.dWo), ow = m - q * a.Wo;                                                   \
    const int n = fdiv(q, a.dHo), oh = q - n * a.Ho;                                                   \
    ih0 = oh * a.stride - a.pad_h; iw0 = ow * a.stride - a.pad_w; nb = n * a.H * a.W
#define CF_TAP(k4)                                                                                     \
    const int tap = fdiv(k4, a.dCip), ci = k4 - tap * a.Cip;                                           \
    const int kh = fdiv(tap, a.dKW), kw = tap - kh * a.KW;                                             \
    const bool kok = k4 < a.Kreal;                                                                     \
    const int dh = kh * a.dil, dw = kw * a.dil
// the fetch of a zero-padded map (the U-Net's too); the stem's pad channel, whatever it holds, is not an input
#define CF_FETCH_PADDED(v, ih0, iw0, nb)                                                               \
    const int ih = ih0 + dh, iw = iw0 + dw;                                                            \
    if (kok && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W) {                         \
        v = *(const f32x4*)(a.x + (size_t)(nb + ih * a.W + iw) * a.ldx + a.xoff + ci);                 \
        if (a.Ci == 3) v[3] = 0.f;                                                                     \
    }
// PReLU's slope: one device load per thread
#define CF_STORE_SETUP                                                                                 \
    float slope = 0.f;                                                                                 \
    if (EXT && a.act == GCC_EVAL_ACT_PRELU) slope = *a.slope
// nn.PixelShuffle(2): channel co of pixel (n, oh, ow) is channel co >> 2 of pixel (2 oh + bit 1, 2 ow + bit 0); q = n Ho + oh
#define CF_STORE(m, co, z)                                                                             \
    float v = z;                                                                                       \
    if (a.res) v += a.res[(size_t)m * a.ldr + a.roff + co];                                            \
    if (!EXT) {                                                                                        \
        if (a.relu) v = v < 0.f ? 0.f : v;                                                             \
        a.y[(size_t)m * a.ldy + a.yoff + co] = v;                                                      \
    } else {                                                                                           \
        if (a.act == GCC_EVAL_ACT_RELU) v = v < 0.f ? 0.f : v;                                         \
        else if (a.act == GCC_EVAL_ACT_PRELU) v = v >= 0.f ? v : __fmul_rn(slope, v);                  \
        else if (a.act == GCC_EVAL_ACT_TANH) v = tanhf(v);                                             \
        if (!a.shuffle) {                                                                              \
            a.y[(size_t)m * a.ldy + a.yoff + co] = v;                                                  \
        } else {                                                                                       \
            const int q = fdiv(m, a.dWo), ow = m - q * a.Wo;                                           \
            const size_t p = ((size_t)q * 2 + ((co >> 1) & 1)) * ((size_t)a.Wo * 2) + 2 * ow + (co & 1); \
            a.y[p * a.ldy + a.yoff + (co >> 2)] = v;                                                   \
        }                                                                                              \
    }
template <int MI, int NI, int WM, int WN, bool EXT>
__global__ __launch_bounds__(CF_THREADS) void conv_f32_kernel(ConvF32Args a) {
#define CF_SETUP const float* wbase = a.w
#define CF_FETCH CF_FETCH_PADDED
#define CF_NK (a.Kp / CF_BK)
#include "conv_f32_tile_body.inc"
}
#undef CF_SETUP
#undef CF_ROW
#undef CF_TAP
#undef CF_STORE_SETUP
#undef CF_STORE

// ---- gcc_conv_eval_f32_unet: Conv2d / ConvTranspose2d (k4, s2, p1) with two activated outputs -------------------------------
struct ConvF32UnetArgs {
    const float* x; const float* w; float* y; float* y2;
    const float* scale; const float* shift;
    int M, H, W, Hm, Wm, Ci, Cip, Co;              // M = N Hm Wm rows: forward Hm x Wm is the output map, transposed the input map
    int ldx, xoff, ldy, yoff, ldy2, y2off, Kreal, Kp, act, act2;
    float slope;
    FastDiv dWm, dHm, dCip;
};

__device__ __forceinline__ float cf_unet_act(float v, int act, float slope) {
    if (act == GCC_EVAL_ACT_RELU) return v < 0.f ? 0.f : v;
    if (act == GCC_EVAL_ACT_LRELU) return v >= 0.f ? v : __fmul_rn(slope, v);
    if (act == GCC_EVAL_ACT_TANH) return tanhf(v);
    return v;
}

// TR = false: row m is output pixel (n, oh, ow), tap = kh 4 + kw read at (2 oh - 1 + kh, 2 ow - 1 + kw).
// TR = true: blockIdx.z = 2 ph + pw is the phase (each has its own packed weights), row m is input-map pixel (n, i, j) and output
// pixel (n, 2 i + ph, 2 j + pw) of [N][2 H][2 W]; tap = 2 th + tw reads (i + ph - th, j + pw - tw), which is kernel element
// (1 - ph + 2 th, 1 - pw + 2 tw) of ConvTranspose2d.  The store is y = act(z) and, with y2, y2 = act2(z); q = n H + i there.
// a: the kernel's ConvF32UnetArgs in each of them.
#define CF_ROW(m, ih0, iw0, nb)                                                                        \
    const int q = fdiv(m, a.dWm), c = m - q * a.Wm;                                                    \
    const int n = fdiv(q, a.dHm), r = q - n * a.Hm;                                                    \
    ih0 = TR ? r + ph : 2 * r - 1; iw0 = TR ? c + pw : 2 * c - 1; nb = n * a.H * a.W
#define CF_TAP(k4)                                                                                     \
    const int tap = fdiv(k4, a.dCip), ci = k4 - tap * a.Cip;                                           \
    const bool kok = k4 < a.Kreal;                                                                     \
    const int dh = TR ? -(tap >> 1) : (tap >> 2), dw = TR ? -(tap & 1) : (tap & 3)
#define CF_STORE_SETUP
#define CF_STORE(m, co, Z)                                                                             \
    size_t p = (size_t)m;                                                                              \
    if (TR) {                                                                                          \
        const int q = fdiv(m, a.dWm), c = m - q * a.Wm;                                                \
        p = ((size_t)q * 2 + ph) * ((size_t)a.Wm * 2) + 2 * c + pw;                                    \
    }                                                                                                  \
    const float z = Z;                                                                                 \
    a.y[p * a.ldy + a.yoff + co] = cf_unet_act(z, a.act, a.slope);                                     \
    if (a.y2) a.y2[p * a.ldy2 + a.y2off + co] = cf_unet_act(z, a.act2, a.slope)
template <int MI, int NI, int WM, int WN, bool TR>
__global__ __launch_bounds__(CF_THREADS) void conv_f32_unet_kernel(ConvF32UnetArgs a) {
#define CF_SETUP                                                                                       \
    const int ph = TR ? (int)(blockIdx.z >> 1) : 0, pw = TR ? (int)(blockIdx.z & 1) : 0;               \
    const float* wbase = a.w + (TR ? (size_t)blockIdx.z * a.Co * a.Kp : 0)
#include "conv_f32_tile_body.inc"
}
#undef CF_SETUP
#undef CF_ROW
#undef CF_TAP
#undef CF_FETCH
#undef CF_FETCH_PADDED
#undef CF_NK
#undef CF_STORE_SETUP
#undef CF_STORE

// one thread per pixel: C strided reads (consecutive threads read consecutive floats of a plane), cfill / 4 16-byte stores
__global__ __launch_bounds__(CF_THREADS) void nchw_to_nhwc_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int C,
                                                                       size_t plane, size_t pixels, int ld, int off, int cfill) {
    for (size_t p = (size_t)blockIdx.x * CF_THREADS + threadIdx.x; p < pixels; p += (size_t)gridDim.x * CF_THREADS) {
        const size_t n = p / plane, q = p - n * plane;
        const float* s = src + n * C * plane + q;
        float* d = dst + p * ld + off;
        for (int c4 = 0; c4 < cfill; c4 += 4) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = (c4 + j < C) ? s[(size_t)(c4 + j) * plane] : 0.f;
            *(f32x4*)(d + c4) = v;
        }
    }
}

// the way back: one thread per pixel reads its C floats, consecutive threads write consecutive floats of each plane
__global__ __launch_bounds__(CF_THREADS) void nhwc_to_nchw_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int C,
                                                                       size_t plane, size_t pixels, int ld, int off) {
    for (size_t p = (size_t)blockIdx.x * CF_THREADS + threadIdx.x; p < pixels; p += (size_t)gridDim.x * CF_THREADS) {
        const size_t n = p / plane, q = p - n * plane;
        const float* s = src + p * ld + off;
        float* d = dst + n * C * plane + q;
        for (int c = 0; c < C; c++) d[(size_t)c * plane] = s[c];
    }
}

// the tile of a geometry whose kernel and paddings have passed, or the error the call returns for it
int cf_finish(const gcc_conv_t* c, int pad_h, int pad_w, int dilation, int shuffle = 0) {
    if ((c->Ci != 3 && (c->Ci & 7)) || (c->Co & 7) || (shuffle && (c->Co & 31))) return GCC_ERR_UNSUPPORTED;
    if (c->ldx < c->xoff + cf_cip(c->Ci) || c->ldy < c->yoff + (shuffle ? c->Co / 4 : c->Co)) return GCC_ERR_BAD_ARG;
    const int span_h = dilation * (c->KH - 1) + 1, span_w = dilation * (c->KW - 1) + 1;
    if (c->H + 2 * pad_h < span_h || c->W + 2 * pad_w < span_w) return GCC_ERR_BAD_ARG;
    const long long Ho = (c->H + 2 * pad_h - span_h) / c->stride + 1, Wo = (c->W + 2 * pad_w - span_w) / c->stride + 1;
    const long long M = (long long)c->N * Ho * Wo, Min = (long long)c->N * c->H * c->W;
    if (M >= (1ll << 31) - 256 || Min >= (1ll << 31) || (long long)c->KH * c->KW * cf_cip(c->Ci) >= (1ll << 30))
        return GCC_ERR_UNSUPPORTED;
    return cf_tile(M, c->Co);
}

// gcc_conv_eval_f32: square 1 / 3 / 7 kernels with "same" padding, c->pad for both directions
int cf_route(const gcc_conv_t* c, int dilation) {
    const int bad = cf_common(c, c ? c->pad : 0, c ? c->pad : 0, dilation);
    if (bad) return bad;
    if (c->KH != c->KW || (c->KH != 1 && c->KH != 3 && c->KH != 7) || (c->stride != 1 && c->stride != 2)) return GCC_ERR_UNSUPPORTED;
    if ((dilation != 1 && dilation != 2 && dilation != 4) || c->pad != dilation * (c->KH / 2)) return GCC_ERR_UNSUPPORTED;
    return cf_finish(c, c->pad, c->pad, dilation);
}

// gcc_conv_eval_f32_ex: KH and KW each of 1 / 3 / 5 / 7, each padding from 0 to "same"; c->pad must be 0
int cf_route_ex(const gcc_conv_t* c, int pad_h, int pad_w, int dilation) {
    const int bad = cf_common(c, pad_h, pad_w, dilation);
    if (bad) return bad;
    if (c->pad != 0) return GCC_ERR_BAD_ARG;               // the paddings are arguments: a descriptor that carries one is a mistake
    auto k_ok = [](int k) { return k == 1 || k == 3 || k == 5 || k == 7; };
    if (!k_ok(c->KH) || !k_ok(c->KW) || (c->stride != 1 && c->stride != 2)) return GCC_ERR_UNSUPPORTED;
    if ((dilation != 1 && dilation != 2 && dilation != 4) || pad_h > dilation * (c->KH / 2) || pad_w > dilation * (c->KW / 2))
        return GCC_ERR_UNSUPPORTED;
    return cf_finish(c, pad_h, pad_w, dilation);
}

// gcc_conv_eval_f32_act: cf_route_ex with sides up to 9 and the PixelShuffle(2) store (shuffle 0 or 2; Co a multiple of 32, the
// window of y Co / 4 channels wide)
int cf_route_act(const gcc_conv_t* c, int pad_h, int pad_w, int dilation, int shuffle) {
    const int bad = cf_common(c, pad_h, pad_w, dilation);
    if (bad) return bad;
    if (c->pad != 0 || (shuffle != 0 && shuffle != 2)) return GCC_ERR_BAD_ARG;
    auto k_ok = [](int k) { return k == 1 || k == 3 || k == 5 || k == 7 || k == 9; };
    if (!k_ok(c->KH) || !k_ok(c->KW) || (c->stride != 1 && c->stride != 2)) return GCC_ERR_UNSUPPORTED;
    if ((dilation != 1 && dilation != 2 && dilation != 4) || pad_h > dilation * (c->KH / 2) || pad_w > dilation * (c->KW / 2))
        return GCC_ERR_UNSUPPORTED;
    return cf_finish(c, pad_h, pad_w, dilation, shuffle);
}

// the one launch of all entries; route: the tile, from cf_route / cf_route_ex / cf_route_act; slope, shuffle: the act entry's (EXT)
template <bool EXT>
int cf_launch(const gcc_conv_t* c, int route, int pad_h, int pad_w, const float* x, const float* w, float* y,
              const gcc_eval_f32_epilogue_t* ep, gcc_stream_t stream, const float* slope = nullptr, int shuffle = 0) {
    if ((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)y) | ((uintptr_t)ep->residual)) & 15) return GCC_ERR_BAD_ARG;
    if (ep->residual && (ep->ld_residual <= 0 || ep->residual_off < 0 || (ep->ld_residual & 3) || (ep->residual_off & 3) ||
                         ep->ld_residual < ep->residual_off + c->Co))
        return GCC_ERR_BAD_ARG;
    ConvF32Args a;
    const int span_h = ep->dilation * (c->KH - 1) + 1, span_w = ep->dilation * (c->KW - 1) + 1;
    a.x = x; a.w = w; a.y = y; a.scale = ep->scale; a.shift = ep->shift; a.res = ep->residual;
    a.H = c->H; a.W = c->W;
    a.Ho = (c->H + 2 * pad_h - span_h) / c->stride + 1;
    a.Wo = (c->W + 2 * pad_w - span_w) / c->stride + 1;
    a.M = c->N * a.Ho * a.Wo;
    a.Ci = c->Ci; a.Cip = cf_cip(c->Ci); a.Co = c->Co; a.KW = c->KW; a.stride = c->stride; a.pad_h = pad_h; a.pad_w = pad_w;
    a.dil = ep->dilation;
    a.ldx = c->ldx; a.xoff = c->xoff; a.ldy = c->ldy; a.yoff = c->yoff;
    a.ldr = ep->residual ? ep->ld_residual : 0; a.roff = ep->residual ? ep->residual_off : 0;
    a.Kreal = c->KH * c->KW * a.Cip; a.Kp = cf_kp(c->Ci, c->KH * c->KW);
    a.relu = ep->act == GCC_EVAL_ACT_RELU;
    a.slope = slope; a.act = ep->act; a.shuffle = shuffle;
    a.dWo = make_fastdiv(a.Wo); a.dHo = make_fastdiv(a.Ho); a.dCip = make_fastdiv(a.Cip); a.dKW = make_fastdiv(a.KW);
    CF_LAUNCH_TILE(conv_f32_kernel, EXT, a, 1, route, (hipStream_t)stream);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

// gcc_conv_eval_f32_unet: 16 taps forward, 4 per phase transposed
inline int cf_unet_kp(int Ci, int transposed) { return cf_kp(Ci, transposed ? 4 : 16); }

// the rows one launch slice walks: output pixels forward, input pixels (one phase's output pixels) transposed
inline long long cf_unet_rows(const gcc_conv_t* c, int transposed) {
    return transposed ? (long long)c->N * c->H * c->W : (long long)c->N * (c->H / 2) * (c->W / 2);
}

// gcc_conv_eval_f32_unet: the tile of a geometry (cf_tile on the rows of one phase), or the error the call returns for it
int cf_route_unet(const gcc_conv_t* c, int transposed) {
    if (!c || (transposed != 0 && transposed != 1)) return GCC_ERR_BAD_ARG;
    const int bad = cf_common(c, c->pad, c->pad, 1);
    if (bad) return bad;
    if (c->pad != 1) return GCC_ERR_BAD_ARG;               // the U-Net's layers have one padding; anything else is a mistake
    if (c->KH != 4 || c->KW != 4 || c->stride != 2) return GCC_ERR_UNSUPPORTED;
    if ((c->Ci & 7) && (c->Ci != 3 || transposed)) return GCC_ERR_UNSUPPORTED;
    if (c->Co & 7) return GCC_ERR_UNSUPPORTED;
    if (c->ldx < c->xoff + cf_cip(c->Ci) || c->ldy < c->yoff + c->Co) return GCC_ERR_BAD_ARG;
    if (!transposed && (c->H < 2 || c->W < 2)) return GCC_ERR_BAD_ARG;         // a map smaller than the kernel's span
    const long long M = cf_unet_rows(c, transposed), Mout = transposed ? 4 * M : M, Min = (long long)c->N * c->H * c->W;
    if (Mout >= (1ll << 31) - 256 || Min >= (1ll << 31) || 16ll * cf_cip(c->Ci) >= (1ll << 30)) return GCC_ERR_UNSUPPORTED;
    return cf_tile(M, c->Co);
}

// do the windows [0, Co) of two NHWC tensors of `pixels` pixels share a float?  a, b: addresses in floats
bool cf_windows_overlap(long long a, int lda, long long b, int ldb, long long pixels, int Co) {
    if (a + (pixels - 1) * lda + Co <= b || b + (pixels - 1) * ldb + Co <= a) return false;
    if (lda != ldb) return true;                           // interleaved at two strides: not worth telling apart
    const long long r = ((b - a) % lda + lda) % lda;
    return r < Co || r > lda - Co;
}

}  // namespace

extern "C" int gcc_conv_eval_f32_unet_kp(int Ci, int transposed) {
    if (Ci <= 0 || (transposed != 0 && transposed != 1) || 16ll * cf_cip(Ci) >= (1ll << 30)) return GCC_ERR_BAD_ARG;
    return cf_unet_kp(Ci, transposed);
}

extern "C" int gcc_conv_eval_f32_unet_route(const gcc_conv_t* c, int transposed) { return cf_route_unet(c, transposed); }

extern "C" int gcc_conv_eval_f32_unet(const gcc_conv_t* c, int transposed, const float* x, const float* w, float* y,
                                      const gcc_eval_f32_unet_epilogue_t* ep, gcc_stream_t stream) {
    GCC_ENTER();
    if (!c || !x || !w || !y || !ep) return GCC_ERR_BAD_ARG;
    auto act_ok = [](int act) {
        return act == GCC_EVAL_ACT_NONE || act == GCC_EVAL_ACT_RELU || act == GCC_EVAL_ACT_LRELU || act == GCC_EVAL_ACT_TANH;
    };
    if (!act_ok(ep->act) || (ep->y2 && !act_ok(ep->act2))) return GCC_ERR_BAD_ARG;
    const int route = cf_route_unet(c, transposed);
    if (route < 0) return route;
    if ((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)y) | ((uintptr_t)ep->y2)) & 15) return GCC_ERR_BAD_ARG;
    const long long M = cf_unet_rows(c, transposed), Mout = transposed ? 4 * M : M;
    if (ep->y2) {
        if (ep->ldy2 <= 0 || ep->y2off < 0 || (ep->ldy2 & 3) || (ep->y2off & 3) || ep->ldy2 < ep->y2off + c->Co) return GCC_ERR_BAD_ARG;
        if (cf_windows_overlap((long long)((uintptr_t)y / 4) + c->yoff, c->ldy, (long long)((uintptr_t)ep->y2 / 4) + ep->y2off, ep->ldy2,
                               Mout, c->Co))
            return GCC_ERR_BAD_ARG;
    }
    ConvF32UnetArgs a;
    a.x = x; a.w = w; a.y = y; a.y2 = ep->y2; a.scale = ep->scale; a.shift = ep->shift;
    a.M = (int)M; a.H = c->H; a.W = c->W;
    a.Hm = transposed ? c->H : c->H / 2; a.Wm = transposed ? c->W : c->W / 2;
    a.Ci = c->Ci; a.Cip = cf_cip(c->Ci); a.Co = c->Co;
    a.ldx = c->ldx; a.xoff = c->xoff; a.ldy = c->ldy; a.yoff = c->yoff;
    a.ldy2 = ep->y2 ? ep->ldy2 : 0; a.y2off = ep->y2 ? ep->y2off : 0;
    a.Kreal = (transposed ? 4 : 16) * a.Cip; a.Kp = cf_unet_kp(c->Ci, transposed);
    a.act = ep->act; a.act2 = ep->act2; a.slope = ep->slope;
    a.dWm = make_fastdiv(a.Wm); a.dHm = make_fastdiv(a.Hm); a.dCip = make_fastdiv(a.Cip);
    if (transposed) CF_LAUNCH_TILE(conv_f32_unet_kernel, true, a, 4, route, (hipStream_t)stream);
    else CF_LAUNCH_TILE(conv_f32_unet_kernel, false, a, 1, route, (hipStream_t)stream);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_conv_eval_f32_kp(int Ci, int KH, int KW) {
    if (Ci <= 0 || KH <= 0 || KW <= 0 || (long long)KH * KW * cf_cip(Ci) >= (1ll << 30)) return GCC_ERR_BAD_ARG;
    return cf_kp(Ci, (long long)KH * KW);
}

extern "C" int gcc_conv_eval_f32_route(const gcc_conv_t* c, int dilation) { return cf_route(c, dilation); }

extern "C" int gcc_conv_eval_f32_ex_route(const gcc_conv_t* c, int pad_h, int pad_w, int dilation) {
    return cf_route_ex(c, pad_h, pad_w, dilation);
}

extern "C" int gcc_conv_eval_f32(const gcc_conv_t* c, const float* x, const float* w, float* y, const gcc_eval_f32_epilogue_t* ep,
                                 gcc_stream_t stream) {
    GCC_ENTER();
    if (!c || !x || !w || !y || !ep) return GCC_ERR_BAD_ARG;
    if (ep->act != GCC_EVAL_ACT_NONE && ep->act != GCC_EVAL_ACT_RELU) return GCC_ERR_BAD_ARG;
    const int route = cf_route(c, ep->dilation);
    if (route < 0) return route;
    return cf_launch<false>(c, route, c->pad, c->pad, x, w, y, ep, stream);
}

extern "C" int gcc_conv_eval_f32_ex(const gcc_conv_t* c, int pad_h, int pad_w, const float* x, const float* w, float* y,
                                    const gcc_eval_f32_epilogue_t* ep, gcc_stream_t stream) {
    GCC_ENTER();
    if (!c || !x || !w || !y || !ep) return GCC_ERR_BAD_ARG;
    if (ep->act != GCC_EVAL_ACT_NONE && ep->act != GCC_EVAL_ACT_RELU) return GCC_ERR_BAD_ARG;
    const int route = cf_route_ex(c, pad_h, pad_w, ep->dilation);
    if (route < 0) return route;
    return cf_launch<false>(c, route, pad_h, pad_w, x, w, y, ep, stream);
}

extern "C" int gcc_conv_eval_f32_act_route(const gcc_conv_t* c, int pad_h, int pad_w, int dilation, int shuffle) {
    return cf_route_act(c, pad_h, pad_w, dilation, shuffle);
}

extern "C" int gcc_conv_eval_f32_act(const gcc_conv_t* c, int pad_h, int pad_w, const float* x, const float* w, float* y,
                                     const gcc_eval_f32_act_epilogue_t* ep, gcc_stream_t stream) {
    GCC_ENTER();
    if (!c || !x || !w || !y || !ep) return GCC_ERR_BAD_ARG;
    if (ep->act != GCC_EVAL_ACT_NONE && ep->act != GCC_EVAL_ACT_RELU && ep->act != GCC_EVAL_ACT_PRELU && ep->act != GCC_EVAL_ACT_TANH)
        return GCC_ERR_BAD_ARG;
    if (ep->act == GCC_EVAL_ACT_PRELU && !ep->slope) return GCC_ERR_BAD_ARG;
    if (ep->shuffle != 0 && ep->shuffle != 2) return GCC_ERR_BAD_ARG;
    if (ep->shuffle && ep->residual) return GCC_ERR_UNSUPPORTED;
    const int route = cf_route_act(c, pad_h, pad_w, ep->dilation, ep->shuffle);
    if (route < 0) return route;
    const gcc_eval_f32_epilogue_t base = {ep->scale, ep->shift, ep->residual, ep->ld_residual, ep->residual_off, ep->act, ep->dilation};
    return cf_launch<true>(c, route, pad_h, pad_w, x, w, y, &base, stream, ep->act == GCC_EVAL_ACT_PRELU ? ep->slope : nullptr,
                           ep->shuffle);
}

extern "C" int gcc_nhwc_f32_to_nchw_f32(const float* src, float* dst, int N, int C, int H, int W, int ld, int off, gcc_stream_t stream) {
    GCC_ENTER();
    if (!src || !dst || N <= 0 || C <= 0 || H <= 0 || W <= 0 || ld <= 0 || off < 0 || ld < off + C) return GCC_ERR_BAD_ARG;
    const size_t plane = (size_t)H * W, pixels = plane * N;
    size_t blocks = (pixels + CF_THREADS - 1) / CF_THREADS;
    if (blocks > (1u << 20)) blocks = 1u << 20;
    hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel, dim3((unsigned)blocks), dim3(CF_THREADS), 0, (hipStream_t)stream, src, dst, C, plane,
                       pixels, ld, off);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_nchw_f32_to_nhwc_f32(const float* src, float* dst, int N, int C, int H, int W, int ld, int off, int cfill,
                                        gcc_stream_t stream) {
    GCC_ENTER();
    if (!src || !dst || N <= 0 || C <= 0 || H <= 0 || W <= 0) return GCC_ERR_BAD_ARG;
    if (ld <= 0 || off < 0 || cfill < C || (ld & 3) || (off & 3) || (cfill & 3) || ld < off + cfill || (((uintptr_t)dst) & 15))
        return GCC_ERR_BAD_ARG;
    const size_t plane = (size_t)H * W, pixels = plane * N;
    size_t blocks = (pixels + CF_THREADS - 1) / CF_THREADS;
    if (blocks > (1u << 20)) blocks = 1u << 20;
    hipLaunchKernelGGL(nchw_to_nhwc_f32_kernel, dim3((unsigned)blocks), dim3(CF_THREADS), 0, (hipStream_t)stream, src, dst, C, plane,
                       pixels, ld, off, cfill);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
