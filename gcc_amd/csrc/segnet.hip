// The streaming kernels around the convolutions of a DRN-D segmentation network (metric/drn.py, metric/mIoU_score.py:124-157;
// gcc_amd/metric/drn_seg.py drives them):
//   gcc_phase_regroup   an NHWC bf16 image moved between "phase layouts": in layout d logical pixel (n, h, w) lives at batch index
//                       n d^2 + (h mod d) d + (w mod d), row h div d, column w div d of an [N d^2, H / d, W / d] image, so that a
//                       3 x 3 convolution of dilation d and padding d is an ordinary 3 x 3, padding-1 convolution of that image
//   gcc_relu_bf16       in-place ReLU of a channel window: relu(bn(conv) + residual) behind gcc_conv_fprop_eval
//   gcc_seg_head        (and gcc_seg_head_f32: fp32 features) the fp32 output end: the 1 x 1 `seg` conv with bias (NCHW fp32 scores), then the depthwise 16 x 16,
//                       stride-8, padding-4 ConvTranspose2d `up` and LogSoftmax over the classes, per output pixel in registers
// Every thread owns its outputs: no atomics, no inter-workgroup communication, no grid-wide state.
#include "common.hpp"

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_MAX_CLASSES = 64;

inline unsigned sg_blocks(size_t items, size_t cap = 1u << 20) {
    const size_t b = (items + SG_THREADS - 1) / SG_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
inline bool sg_phase_ok(int d) { return d == 1 || d == 2 || d == 4; }

// one thread per 16-byte chunk of the DESTINATION (consecutive threads write consecutive chunks of a pixel, then the next pixel):
// destination pixel index -> logical (n, h, w) -> source pixel index.  d, chunks: launch constants.
__global__ __launch_bounds__(SG_THREADS) void phase_regroup_kernel(const bf16_t* __restrict__ src, int lds, int soff, int ds,
                                                                    bf16_t* __restrict__ dst, int ldd, int doff, int dd, int H, int W,
                                                                    int C, int chunks, size_t total) {
    const int Hd = H / dd, Wd = W / dd, Hs = H / ds, Ws = W / ds;
    for (size_t i = (size_t)blockIdx.x * SG_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * SG_THREADS) {
        const size_t dp = i / chunks;
        const int ch = (int)(i - dp * chunks);
        // destination pixel dp = ((n dd^2 + ph dd + pw) Hd + hq) Wd + wq
        size_t t = dp;
        const int wq = (int)(t % Wd); t /= Wd;
        const int hq = (int)(t % Hd); t /= Hd;
        const int pw = (int)(t % dd); t /= dd;
        const int ph = (int)(t % dd); t /= dd;
        const size_t n = t;
        const int h = hq * dd + ph, w = wq * dd + pw;
        const size_t sp = ((n * ds * ds + (size_t)(h % ds) * ds + (w % ds)) * Hs + h / ds) * Ws + w / ds;
        i32x4 v = *(const i32x4*)(src + sp * lds + soff + ch * 8);
        if (ch * 8 + 8 > C) {          // the last chunk of a width that is no multiple of 8: its pad channels are written as zeros
            bf16_t* e = (bf16_t*)&v;
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (ch * 8 + j >= C) e[j] = 0;
        }
        *(i32x4*)(dst + dp * ldd + doff + ch * 8) = v;
    }
}

// x > 0 ? x : +0 per element; NaN stays.  Elements of the last chunk at or beyond C are left as they are.
__global__ __launch_bounds__(SG_THREADS) void relu_bf16_kernel(bf16_t* __restrict__ x, int ld, int off, int C, int chunks,
                                                                size_t total) {
    for (size_t i = (size_t)blockIdx.x * SG_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * SG_THREADS) {
        const size_t p = i / chunks;
        const int ch = (int)(i - p * chunks);
        i32x4* q = (i32x4*)(x + p * ld + off + ch * 8);
        i32x4 v = *q;
        bf16_t* e = (bf16_t*)&v;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const bool neg = (e[j] & 0x8000u) && (e[j] & 0x7fffu) <= 0x7f80u;       // sign set and not a NaN: by bits, so that
                                                                                     // no denormal mode has a say
            if (neg && ch * 8 + j < C) e[j] = 0;
        }
        *q = v;
    }
}

// seg: scores[n][c][p] = bias[c] + sum_k w[c][k] x[n][p][k] in fp32, k ascending.  A workgroup is 64 pixels x 4 waves; wave v
// owns classes v, v + 4, ... (so the weights of a wave's FMAs are wave-uniform) and reads each 16-byte chunk of its pixel once.
// The feature map is bf16 (gcc_seg_head) or fp32 (gcc_seg_head_f32: two 16-byte loads per 8 channels); the sums are the same.
constexpr int SEG_WAVES = 4, SEG_PER_WAVE = SG_MAX_CLASSES / SEG_WAVES;
__device__ __forceinline__ void seg_load8(const bf16_t* p, float* f) { unpack8(*(const i32x4*)p, f); }
__device__ __forceinline__ void seg_load8(const float* p, float* f) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
    for (int j = 0; j < 4; j++) { f[j] = a[j]; f[4 + j] = b[j]; }
}
template <typename T>
__global__ __launch_bounds__(SG_THREADS) void seg_scores_kernel(const T* __restrict__ x, int ld, int off, int Cin,
                                                                 const float* __restrict__ w, const float* __restrict__ bias, int C,
                                                                 size_t plane, size_t pixels, float* __restrict__ scores) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t p = (size_t)blockIdx.x * 64 + lane;
    if (p >= pixels) return;
    float acc[SEG_PER_WAVE];
#pragma unroll
    for (int j = 0; j < SEG_PER_WAVE; j++) {
        const int c = wave + SEG_WAVES * j;
        acc[j] = (c < C && bias) ? bias[c] : 0.f;
    }
    const T* xp = x + p * ld + off;
    for (int k = 0; k < Cin; k += 8) {           // Cin is a multiple of 8 (checked on the host)
        float f[8];
        seg_load8(xp + k, f);
#pragma unroll
        for (int j = 0; j < SEG_PER_WAVE; j++) {
            const int c = wave + SEG_WAVES * j;
            if (c < C) {
                const float* wr = w + (size_t)c * Cin + k;
#pragma unroll
                for (int e = 0; e < 8; e++) acc[j] = fmaf(wr[e], f[e], acc[j]);
            }
        }
    }
    const size_t n = p / plane, q = p - n * plane;
#pragma unroll
    for (int j = 0; j < SEG_PER_WAVE; j++) {
        const int c = wave + SEG_WAVES * j;
        if (c < C) scores[(n * C + c) * plane + q] = acc[j];
    }
}

// up + LogSoftmax: output pixel (Y, X) of the 8x map receives source row iy through kernel row ky = Y + 4 - 8 iy in [0, 16):
// iy = (Y + 4) div 8 with ky = (Y + 4) mod 8, and iy - 1 with ky + 8; the same along x.  Rows / columns outside the source
// contribute nothing.  The thread keeps the C upsampled values in registers (CMAX: the unrolled bound), then writes
// v[c] - max - log(sum exp(v - max)).
template <int CMAX>
__global__ __launch_bounds__(SG_THREADS) void seg_up_logsoftmax_kernel(const float* __restrict__ scores, int C, int h, int w,
                                                                        const float* __restrict__ upw, size_t total,
                                                                        float* __restrict__ out) {
    const int Ho = 8 * h, Wo = 8 * w;
    const size_t plane = (size_t)h * w, oplane = (size_t)Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * SG_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * SG_THREADS) {
        const size_t n = i / oplane, r = i - n * oplane;
        const int Y = (int)(r / Wo), X = (int)(r - (size_t)Y * Wo);
        const int iy1 = (Y + 4) >> 3, ky1 = (Y + 4) & 7, iy0 = iy1 - 1, ky0 = ky1 + 8;
        const int ix1 = (X + 4) >> 3, kx1 = (X + 4) & 7, ix0 = ix1 - 1, kx0 = kx1 + 8;
        const bool y0 = iy0 >= 0, y1 = iy1 < h, x0 = ix0 >= 0, x1 = ix1 < w;
        const float* s = scores + n * C * plane;
        float v[CMAX];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < CMAX; c++) {
            if (c < C) {
                const float* sc = s + (size_t)c * plane;
                const float* k = upw + c * 256;
                float a = 0.f;
                if (y0 && x0) a = fmaf(sc[iy0 * w + ix0], k[ky0 * 16 + kx0], a);
                if (y0 && x1) a = fmaf(sc[iy0 * w + ix1], k[ky0 * 16 + kx1], a);
                if (y1 && x0) a = fmaf(sc[iy1 * w + ix0], k[ky1 * 16 + kx0], a);
                if (y1 && x1) a = fmaf(sc[iy1 * w + ix1], k[ky1 * 16 + kx1], a);
                v[c] = a;
                m = fmaxf(m, a);
            }
        }
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; c++)
            if (c < C) sum += expf(v[c] - m);
        const float lse = m + logf(sum);
        float* o = out + n * C * oplane + r;
#pragma unroll
        for (int c = 0; c < CMAX; c++)
            if (c < C) o[(size_t)c * oplane] = v[c] - lse;
    }
}

// byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool sg_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char* pa = (const char*)a; const char* pb = (const char*)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" int gcc_phase_regroup(const void* src, int lds, int soff, int d_src, void* dst, int ldd, int doff, int d_dst, int N,
                                 int H, int W, int C, gcc_stream_t stream) {
    GCC_ENTER();
    if (!src || !dst || N <= 0 || H <= 0 || W <= 0 || C <= 0) return GCC_ERR_BAD_ARG;
    if (lds <= 0 || ldd <= 0 || soff < 0 || doff < 0 || (lds & 7) || (ldd & 7) || (soff & 7) || (doff & 7)) return GCC_ERR_BAD_ARG;
    if (lds < soff + ceil8(C) || ldd < doff + ceil8(C)) return GCC_ERR_BAD_ARG;
    if ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) return GCC_ERR_BAD_ARG;
    if (!sg_phase_ok(d_src) || !sg_phase_ok(d_dst)) return GCC_ERR_UNSUPPORTED;
    if (H % d_src || W % d_src || H % d_dst || W % d_dst) return GCC_ERR_UNSUPPORTED;
    const size_t pixels = (size_t)N * H * W;
    if (sg_overlap(src, pixels * lds * 2, dst, pixels * ldd * 2)) return GCC_ERR_BAD_ARG;      // a permutation is not done in place
    const int chunks = ceil8(C) / 8;
    const size_t total = pixels * chunks;
    hipLaunchKernelGGL(phase_regroup_kernel, dim3(sg_blocks(total)), dim3(SG_THREADS), 0, (hipStream_t)stream, (const bf16_t*)src,
                       lds, soff, d_src, (bf16_t*)dst, ldd, doff, d_dst, H, W, C, chunks, total);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_relu_bf16(void* x, int ld, int off, int C, size_t pixels, gcc_stream_t stream) {
    GCC_ENTER();
    if (!x || C <= 0 || pixels == 0) return GCC_ERR_BAD_ARG;
    if (ld <= 0 || off < 0 || (ld & 7) || (off & 7) || ld < off + ceil8(C) || (((uintptr_t)x) & 15)) return GCC_ERR_BAD_ARG;
    const int chunks = ceil8(C) / 8;
    const size_t total = pixels * chunks;
    hipLaunchKernelGGL(relu_bf16_kernel, dim3(sg_blocks(total)), dim3(SG_THREADS), 0, (hipStream_t)stream, (bf16_t*)x, ld, off, C,
                       chunks, total);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

// T: the feature map's element type; ALIGN: what its ld / offset must be multiples of (16 bytes)
template <typename T, int ALIGN>
static int seg_head_impl(const T* x, int ld, int off, int N, int h, int w, int Cin, const float* seg_w, const float* seg_b, int C,
                         const float* up_w, float* scores, float* logp, gcc_stream_t stream) {
    GCC_ENTER();
    if (!scores || N <= 0 || h <= 0 || w <= 0 || C <= 0 || (!x && !logp)) return GCC_ERR_BAD_ARG;
    if (x && (!seg_w || Cin <= 0 || ld <= 0 || off < 0 || (ld & (ALIGN - 1)) || (off & (ALIGN - 1)) || ld < off + ceil8(Cin) ||
              (((uintptr_t)x) & 15)))
        return GCC_ERR_BAD_ARG;
    if (logp && !up_w) return GCC_ERR_BAD_ARG;
    if (C > SG_MAX_CLASSES || (x && (Cin & 7))) return GCC_ERR_UNSUPPORTED;
    const size_t plane = (size_t)h * w, pixels = plane * N;
    if (pixels * 64 >= (size_t)1 << 40) return GCC_ERR_UNSUPPORTED;
    const hipStream_t st = (hipStream_t)stream;
    if (x) {
        hipLaunchKernelGGL(seg_scores_kernel<T>, dim3((unsigned)((pixels + 63) / 64)), dim3(SG_THREADS), 0, st, x, ld, off, Cin, seg_w,
                           seg_b, C, plane, pixels, scores);
        GCC_CHECK_LAUNCH();
    }
    if (logp) {
        const size_t total = pixels * 64;
        if (C <= 24)
            hipLaunchKernelGGL(seg_up_logsoftmax_kernel<24>, dim3(sg_blocks(total)), dim3(SG_THREADS), 0, st, (const float*)scores, C, h,
                               w, up_w, total, logp);
        else
            hipLaunchKernelGGL(seg_up_logsoftmax_kernel<SG_MAX_CLASSES>, dim3(sg_blocks(total)), dim3(SG_THREADS), 0, st,
                               (const float*)scores, C, h, w, up_w, total, logp);
        GCC_CHECK_LAUNCH();
    }
    return GCC_OK;
}

extern "C" int gcc_seg_head(const void* x, int ld, int off, int N, int h, int w, int Cin, const float* seg_w, const float* seg_b,
                            int C, const float* up_w, float* scores, float* logp, gcc_stream_t stream) {
    return seg_head_impl<bf16_t, 8>((const bf16_t*)x, ld, off, N, h, w, Cin, seg_w, seg_b, C, up_w, scores, logp, stream);
}

extern "C" int gcc_seg_head_f32(const float* x, int ld, int off, int N, int h, int w, int Cin, const float* seg_w,
                                const float* seg_b, int C, const float* up_w, float* scores, float* logp, gcc_stream_t stream) {
    return seg_head_impl<float, 4>(x, ld, off, N, h, w, Cin, seg_w, seg_b, C, up_w, scores, logp, stream);
}
