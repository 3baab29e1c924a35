// The streaming kernels around the convolutions of the FID Inception-v3 network (metric/inception.py:166-315;
// gcc_amd/metric/inception_fid.py drives them):
//   gcc_fid_resize       NCHW fp32 [N][3][H][W] in [0, 1] -> NHWC bf16 [N][Ho][Wo][8] = 2 bilinear(x) - 1 (align_corners = False,
//                        no antialiasing: F.interpolate as the network's forward calls it), channels 3 .. 7 zero
//   gcc_pool3x3          3 x 3 pooling of an NHWC bf16 channel window: max stride 2 padding 0, max stride 1 padding 1 (padding is
//                        -inf), average stride 1 padding 1 over the taps inside the map (count_include_pad = False)
//   gcc_border_copy      an NHWC bf16 channel window copied into the middle of a map with a zero border of (ph, pw) pixels, border
//                        included: a (1, 7) / (7, 1) / (1, 3) / (3, 1) convolution with its own padding is then a padding-0 call
//   gcc_global_avgpool   the mean over the pixels of an NHWC bf16 channel window in fp32
//   gcc_map_mean         the same mean of a LARGE map (the network's earlier output blocks) in f64, the pixels of an image split
//                        over workgroups: the one kernel here that is not one thread per chunk (see map_mean_kernel)
// gcc_fid_resize_f32 / gcc_pool3x3_f32 / gcc_global_avgpool_f32 are the same kernels on NHWC fp32 maps (the network at the
// reference's own precision, around gcc_conv_eval_f32_ex): the same arithmetic in the same order without the bf16 roundings, a
// 16-byte chunk holding 4 channels.  Rectangular padding is the fp32 convolution's own index arithmetic: no fp32 border copy.
// One thread per 16-byte chunk (8 bf16 or 4 fp32 channels) of the DESTINATION: consecutive threads write consecutive chunks of a pixel, then the
// next pixel.  Every thread owns its outputs: no atomics, no inter-workgroup communication, no grid-wide state.
#include <math.h>
#include "common.hpp"

namespace {

constexpr int IN_THREADS = 256;

inline unsigned in_blocks(size_t items, size_t cap = 1u << 20) {
    const size_t b = (items + IN_THREADS - 1) / IN_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
// an NHWC channel window of C channels at `off` inside pixels of `ld` elements, 16-byte chunks (ch elements) throughout
inline bool in_window_ok(const void* p, int ld, int off, int C, int ch = 8) {
    return p && ld > 0 && off >= 0 && !(ld & (ch - 1)) && !(off & (ch - 1)) && ld >= off + C && !(((uintptr_t)p) & 15);
}

// a map's element type: the channels of a 16-byte chunk, and a chunk as floats and back (bf16: one rounding on the way back)
template <typename T> struct Chunk;
template <> struct Chunk<bf16_t> {
    static constexpr int CH = 8;
    static __device__ __forceinline__ void load(const bf16_t* p, float* f) { unpack8(*(const i32x4*)p, f); }
    static __device__ __forceinline__ void unpack(const i32x4& v, float* f) { unpack8(v, f); }
    static __device__ __forceinline__ void store(bf16_t* p, const float* f) { *(i32x4*)p = pack8(f); }
};
template <> struct Chunk<float> {
    static constexpr int CH = 4;
    static __device__ __forceinline__ void load(const float* p, float* f) {
        const f32x4 v = *(const f32x4*)p;
#pragma unroll
        for (int j = 0; j < 4; j++) f[j] = v[j];
    }
    static __device__ __forceinline__ void store(float* p, const float* f) { *(f32x4*)p = f32x4{f[0], f[1], f[2], f[3]}; }
    static __device__ __forceinline__ void unpack(const i32x4& v, float* f) {
#pragma unroll
        for (int j = 0; j < 4; j++) f[j] = __int_as_float(v[j]);
    }
};

// torch's area_pixel_compute_source_index (align_corners = False, not cubic): index and the weight of the upper neighbour.  The
// product and the subtraction contract into one fused multiply-add (the intrinsics are plain operators to the compiler), which is
// what torch's own fp32 builds compute: tests/test_inception_f32_kernels_gpu.py holds both to the same fp32 taps.
__device__ __forceinline__ void resize_tap(int d, float scale, int in, int& i0, int& i1, float& l1) {
    float s = __fsub_rn(__fmul_rn(scale, (float)d + 0.5f), 0.5f);
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

template <typename T>
__global__ __launch_bounds__(IN_THREADS) void fid_resize_kernel(const float* __restrict__ x, int H, int W, T* __restrict__ y,
                                                                 int ld, int off, int Ho, int Wo, float sh, float sw, size_t total) {
    constexpr int CH = Chunk<T>::CH;
    const size_t plane = (size_t)H * W, oplane = (size_t)Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * IN_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * IN_THREADS) {
        const size_t n = i / oplane, r = i - n * oplane;
        const int oy = (int)(r / Wo), ox = (int)(r - (size_t)oy * Wo);
        int y0, y1, x0, x1;
        float ly, lx;
        resize_tap(oy, sh, H, y0, y1, ly);
        resize_tap(ox, sw, W, x0, x1, lx);
        const float ky = 1.f - ly, kx = 1.f - lx;
        float f[CH];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float* p = x + (n * 3 + c) * plane;
            const float a = p[(size_t)y0 * W + x0], b = p[(size_t)y0 * W + x1];
            const float cc = p[(size_t)y1 * W + x0], d = p[(size_t)y1 * W + x1];
            const float v = ky * (kx * a + lx * b) + ly * (kx * cc + lx * d);
            f[c] = 2.f * v - 1.f;
        }
#pragma unroll
        for (int c = 3; c < CH; c++) f[c] = 0.f;
        Chunk<T>::store(y + i * ld + off, f);
    }
}

// MODE: GCC_POOL3_MAX_S2 / GCC_POOL3_MAX_S1P1 / GCC_POOL3_AVG_S1P1.  Taps are visited row by row, left to right (torch's order:
// of equal maxima the first met stays, a NaN wins); the average sums in fp32 in that order and divides by the taps inside the map.
template <int MODE, typename T>
__global__ __launch_bounds__(IN_THREADS) void pool3x3_kernel(const T* __restrict__ x, int ldx, int xoff, T* __restrict__ y,
                                                              int ldy, int yoff, int H, int W, int Ho, int Wo, int chunks, size_t total) {
    constexpr int CH = Chunk<T>::CH;
    constexpr int S = MODE == GCC_POOL3_MAX_S2 ? 2 : 1, P = MODE == GCC_POOL3_MAX_S2 ? 0 : 1;
    for (size_t i = (size_t)blockIdx.x * IN_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * IN_THREADS) {
        const size_t dp = i / chunks;
        const int ch = (int)(i - dp * chunks);
        size_t t = dp;
        const int ox = (int)(t % Wo); t /= Wo;
        const int oy = (int)(t % Ho); t /= Ho;
        const size_t n = t;
        float acc[CH];
#pragma unroll
        for (int j = 0; j < CH; j++) acc[j] = MODE == GCC_POOL3_AVG_S1P1 ? 0.f : -INFINITY;
        int count = 0;
#pragma unroll
        for (int ky = 0; ky < 3; ky++) {
            const int iy = oy * S - P + ky;
            if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; kx++) {
                const int ix = ox * S - P + kx;
                if ((unsigned)ix >= (unsigned)W) continue;
                float f[CH];
                Chunk<T>::load(x + ((n * H + iy) * W + ix) * ldx + xoff + ch * CH, f);
                count++;
#pragma unroll
                for (int j = 0; j < CH; j++) {
                    if (MODE == GCC_POOL3_AVG_S1P1) acc[j] += f[j];
                    else if (f[j] > acc[j] || f[j] != f[j]) acc[j] = f[j];
                }
            }
        }
        if (MODE == GCC_POOL3_AVG_S1P1) {
            const float cnt = (float)count;       // >= 1: the centre tap is always inside
#pragma unroll
            for (int j = 0; j < CH; j++) acc[j] = acc[j] / cnt;
        }
        Chunk<T>::store(y + dp * ldy + yoff + ch * CH, acc);
    }
}

__global__ __launch_bounds__(IN_THREADS) void border_copy_kernel(const bf16_t* __restrict__ src, int lds, int soff,
                                                                  bf16_t* __restrict__ dst, int ldd, int doff, int H, int W, int ph,
                                                                  int pw, int chunks, size_t total) {
    const int Hd = H + 2 * ph, Wd = W + 2 * pw;
    for (size_t i = (size_t)blockIdx.x * IN_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * IN_THREADS) {
        const size_t dp = i / chunks;
        const int ch = (int)(i - dp * chunks);
        size_t t = dp;
        const int wd = (int)(t % Wd); t /= Wd;
        const int hd = (int)(t % Hd); t /= Hd;
        const size_t n = t;
        const int h = hd - ph, w = wd - pw;
        i32x4 v = {0, 0, 0, 0};
        if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) v = *(const i32x4*)(src + ((n * H + h) * W + w) * lds + soff + ch * 8);
        *(i32x4*)(dst + dp * ldd + doff + ch * 8) = v;
    }
}

// out[n][c] = (sum over the pixels of x[n][.][c]) / pixels: eight fp32 partial sums (pixel p goes to partial p mod 8), added as
// ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)) -- the order is fixed by the shape alone, and a sum of 64 terms takes 10 roundings
template <typename T>
__global__ __launch_bounds__(IN_THREADS) void global_avgpool_kernel(const T* __restrict__ x, int ld, int off, int pixels, int C,
                                                                     int chunks, float* __restrict__ out, size_t total) {
    constexpr int CH = Chunk<T>::CH;
    for (size_t i = (size_t)blockIdx.x * IN_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * IN_THREADS) {
        const size_t n = i / chunks;
        const int ch = (int)(i - n * chunks);
        const T* p = x + n * pixels * ld + off + ch * CH;
        float part[8][CH];
#pragma unroll
        for (int a = 0; a < 8; a++)
#pragma unroll
            for (int j = 0; j < CH; j++) part[a][j] = 0.f;
        int q = 0;
        for (; q + 8 <= pixels; q += 8) {
#pragma unroll
            for (int a = 0; a < 8; a++) {
                float f[CH];
                Chunk<T>::load(p + (size_t)(q + a) * ld, f);
#pragma unroll
                for (int j = 0; j < CH; j++) part[a][j] += f[j];
            }
        }
#pragma unroll
        for (int a = 0; a < 8; a++) {
            if (q + a < pixels) {
                float f[CH];
                Chunk<T>::load(p + (size_t)(q + a) * ld, f);
#pragma unroll
                for (int j = 0; j < CH; j++) part[a][j] += f[j];
            }
        }
        const float cnt = (float)pixels;
        float o[CH];
#pragma unroll
        for (int j = 0; j < CH; j++)
            o[j] = (((part[0][j] + part[1][j]) + (part[2][j] + part[3][j])) + ((part[4][j] + part[5][j]) + (part[6][j] + part[7][j]))) / cnt;
        float* op = out + n * C + ch * CH;
#pragma unroll
        for (int j = 0; j < CH; j += 4) *(f32x4*)(op + j) = f32x4{o[j], o[j + 1], o[j + 2], o[j + 3]};
    }
}

// gcc_map_mean: the mean of a LARGE map (the 73 x 73, 35 x 35 and 17 x 17 taps of the network), the pixels of an image split over
// workgroups.  Workgroup (n, cb, s) owns image n, a block of CW chunks and pixel range [s P / S, (s + 1) P / S); its MM_THREADS
// threads are R = MM_THREADS / CW pixel rows of CW chunk lanes: thread (pr, cl) adds pixels lo + pr, lo + pr + R, ... of its chunk
// in f64, ascending, MM_FLIGHT 16-byte loads in flight.  The R rows are then folded through LDS in ascending pr by one thread per
// channel.  S == 1: that sum is divided and stored; S > 1: it goes to ws [n][s][C] and map_mean_fold_kernel adds the segments in
// ascending s.  CW is a function of C alone, so the order is a function of (P, C, S): no atomics, nothing grid-wide.
constexpr int MM_THREADS = 256, MM_FLIGHT = 8;

template <typename T>
__global__ __launch_bounds__(MM_THREADS) void map_mean_kernel(const T* __restrict__ x, int ld, int off, int P, int C, int CW, int CB,
                                                               int S, float* __restrict__ out, double* __restrict__ ws) {
    constexpr int CH = Chunk<T>::CH;
    __shared__ double part[MM_THREADS * CH];
    const int b = blockIdx.x;
    const int s = b % S, cb = (b / S) % CB;
    const size_t n = (size_t)(b / S / CB);
    const int t = threadIdx.x, R = MM_THREADS / CW;
    const int cl = t % CW, pr = t / CW;
    const int lo = (int)((long long)s * P / S), hi = (int)((long long)(s + 1) * P / S);
    const T* p = x + n * (size_t)P * ld + off + (size_t)(cb * CW + cl) * CH;
    double acc[CH];
#pragma unroll
    for (int j = 0; j < CH; j++) acc[j] = 0.0;
    for (int q = lo + pr; q < hi; q += MM_FLIGHT * R) {
        i32x4 v[MM_FLIGHT];                                              // the chunks as loaded: converted when they are added
#pragma unroll
        for (int u = 0; u < MM_FLIGHT; u++) {
            const int qq = q + u * R;
            v[u] = qq < hi ? *(const i32x4*)(p + (size_t)qq * ld) : i32x4{0, 0, 0, 0};      // + 0.0 leaves an f64 sum as it is
        }
#pragma unroll
        for (int u = 0; u < MM_FLIGHT; u++) {
            float f[CH];
            Chunk<T>::unpack(v[u], f);
#pragma unroll
            for (int j = 0; j < CH; j++) acc[j] += (double)f[j];
        }
    }
#pragma unroll
    for (int j = 0; j < CH; j++) part[t * CH + j] = acc[j];              // [pr][cl][j]
    __syncthreads();
    const int W = CW * CH;                                                // channels of this workgroup, <= MM_THREADS
    if (t < W) {
        double sum = 0.0;
        for (int r = 0; r < R; r++) sum += part[r * W + t];
        const int c = cb * W + t;
        if (S == 1) out[n * C + c] = (float)(sum / (double)P);
        else ws[(n * S + s) * C + c] = sum;
    }
}

__global__ __launch_bounds__(IN_THREADS) void map_mean_fold_kernel(const double* __restrict__ ws, int S, int C, int P,
                                                                    float* __restrict__ out, size_t total) {
    for (size_t i = (size_t)blockIdx.x * IN_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * IN_THREADS) {
        const size_t n = i / C;
        const int c = (int)(i - n * C);
        const double* p = ws + n * S * C + c;
        double sum = 0.0;
        for (int s = 0; s < S; s++) sum += p[(size_t)s * C];
        out[i] = (float)(sum / (double)P);
    }
}

}  // namespace

namespace {

// the chunk lanes of a gcc_map_mean workgroup: the largest power of two that divides the chunks, at most MM_THREADS / CH (one
// thread per channel folds)
template <typename T> int map_mean_cw(int C) {
    constexpr int CH = Chunk<T>::CH;
    const int chunks = C / CH;
    int cw = 1;
    while (cw * 2 * CH <= MM_THREADS && chunks % (cw * 2) == 0) cw *= 2;
    return cw;
}
inline int map_mean_max_segments(size_t P) { return (int)(P < GCC_MAP_MEAN_MAX_SEGMENTS ? P : GCC_MAP_MEAN_MAX_SEGMENTS); }
// the library's split, the same for both element types: a thread of the fp32 kernel adds about GCC_MAP_MEAN_PIXELS_PER_THREAD
// pixels of a segment (one of the bf16 kernel, whose chunks hold twice the channels, half as many)
int map_mean_segments(size_t P, int C) {
    const size_t rows = MM_THREADS / map_mean_cw<float>(C);
    const size_t s = P / (rows * GCC_MAP_MEAN_PIXELS_PER_THREAD);
    const size_t most = map_mean_max_segments(P);
    return (int)(s < 1 ? 1 : (s > most ? most : s));
}

template <typename T>
int map_mean_impl(const T* x, int ld, int off, int N, int h, int w, int C, int segments, float* out, void* ws, size_t ws_bytes,
                  gcc_stream_t stream) {
    constexpr int CH = Chunk<T>::CH;
    GCC_ENTER();
    if (!out || N <= 0 || h <= 0 || w <= 0 || C <= 0 || segments < 0) return GCC_ERR_BAD_ARG;
    if (!in_window_ok(x, ld, off, (C + CH - 1) / CH * CH, CH) || (((uintptr_t)out) & 15)) return GCC_ERR_BAD_ARG;
    if (C & (CH - 1)) return GCC_ERR_UNSUPPORTED;
    const size_t P = (size_t)h * w;
    if (P >= (size_t)1 << 24 || (size_t)N * P * ld >= (size_t)1 << 40) return GCC_ERR_UNSUPPORTED;
    if (segments > map_mean_max_segments(P)) return GCC_ERR_BAD_ARG;
    const int S = segments ? segments : map_mean_segments(P, C);
    const int CW = map_mean_cw<T>(C), CB = C / CH / CW;
    const size_t wgs = (size_t)N * CB * S;
    if (wgs >= (size_t)1 << 31) return GCC_ERR_UNSUPPORTED;
    if (S > 1) {
        if (!ws || (((uintptr_t)ws) & 7)) return GCC_ERR_BAD_ARG;
        if (ws_bytes < (size_t)N * S * C * sizeof(double)) return GCC_ERR_WORKSPACE;
    }
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(map_mean_kernel<T>, dim3((unsigned)wgs), dim3(MM_THREADS), 0, st, x, ld, off, (int)P, C, CW, CB, S, out,
                       (double*)ws);
    GCC_CHECK_LAUNCH();
    if (S > 1) {
        const size_t total = (size_t)N * C;
        hipLaunchKernelGGL(map_mean_fold_kernel, dim3(in_blocks(total)), dim3(IN_THREADS), 0, st, (const double*)ws, S, C, (int)P, out,
                           total);
        GCC_CHECK_LAUNCH();
    }
    return GCC_OK;
}

template <typename T>
int fid_resize_impl(const float* x, int N, int H, int W, T* y, int ld, int off, int Ho, int Wo, gcc_stream_t stream) {
    GCC_ENTER();
    if (!x || N <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return GCC_ERR_BAD_ARG;
    if (!in_window_ok(y, ld, off, Chunk<T>::CH, Chunk<T>::CH) || (((uintptr_t)x) & 3)) return GCC_ERR_BAD_ARG;
    const size_t total = (size_t)N * Ho * Wo;
    if ((size_t)N * 3 * H * W >= (size_t)1 << 40 || total >= (size_t)1 << 40) return GCC_ERR_UNSUPPORTED;
    // torch's area_pixel_compute_scale<float>: the ratio of the sizes in fp32
    const float sh = (float)H / (float)Ho, sw = (float)W / (float)Wo;
    hipLaunchKernelGGL(fid_resize_kernel<T>, dim3(in_blocks(total)), dim3(IN_THREADS), 0, (hipStream_t)stream, x, H, W, y, ld, off,
                       Ho, Wo, sh, sw, total);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

template <typename T>
int pool3x3_impl(int mode, const T* xp, int ldx, int xoff, T* yp, int ldy, int yoff, int N, int H, int W, int C,
                 gcc_stream_t stream) {
    constexpr int CH = Chunk<T>::CH;
    GCC_ENTER();
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return GCC_ERR_BAD_ARG;
    if (mode != GCC_POOL3_MAX_S2 && mode != GCC_POOL3_MAX_S1P1 && mode != GCC_POOL3_AVG_S1P1) return GCC_ERR_BAD_ARG;
    const int Cc = (C + CH - 1) / CH * CH;
    if (!in_window_ok(xp, ldx, xoff, Cc, CH) || !in_window_ok(yp, ldy, yoff, Cc, CH)) return GCC_ERR_BAD_ARG;
    if (C & (CH - 1)) return GCC_ERR_UNSUPPORTED;
    int Ho = H, Wo = W;
    if (mode == GCC_POOL3_MAX_S2) {
        if (H < 3 || W < 3) return GCC_ERR_UNSUPPORTED;            // no output pixel
        Ho = (H - 3) / 2 + 1; Wo = (W - 3) / 2 + 1;
    }
    const int chunks = C / CH;
    const size_t total = (size_t)N * Ho * Wo * chunks;
    if ((size_t)N * H * W * ldx >= (size_t)1 << 40 || (size_t)N * Ho * Wo * ldy >= (size_t)1 << 40) return GCC_ERR_UNSUPPORTED;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(in_blocks(total)), block(IN_THREADS);
    if (mode == GCC_POOL3_MAX_S2)
        hipLaunchKernelGGL((pool3x3_kernel<GCC_POOL3_MAX_S2, T>), grid, block, 0, st, xp, ldx, xoff, yp, ldy, yoff, H, W, Ho, Wo, chunks, total);
    else if (mode == GCC_POOL3_MAX_S1P1)
        hipLaunchKernelGGL((pool3x3_kernel<GCC_POOL3_MAX_S1P1, T>), grid, block, 0, st, xp, ldx, xoff, yp, ldy, yoff, H, W, Ho, Wo, chunks, total);
    else
        hipLaunchKernelGGL((pool3x3_kernel<GCC_POOL3_AVG_S1P1, T>), grid, block, 0, st, xp, ldx, xoff, yp, ldy, yoff, H, W, Ho, Wo, chunks, total);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

template <typename T>
int global_avgpool_impl(const T* x, int ld, int off, int N, int h, int w, int C, float* out, gcc_stream_t stream) {
    constexpr int CH = Chunk<T>::CH;
    GCC_ENTER();
    if (!out || N <= 0 || h <= 0 || w <= 0 || C <= 0) return GCC_ERR_BAD_ARG;
    if (!in_window_ok(x, ld, off, (C + CH - 1) / CH * CH, CH) || (((uintptr_t)out) & 15)) return GCC_ERR_BAD_ARG;
    if (C & (CH - 1)) return GCC_ERR_UNSUPPORTED;
    if ((size_t)h * w >= (size_t)1 << 24 || (size_t)N * h * w * ld >= (size_t)1 << 40) return GCC_ERR_UNSUPPORTED;
    const int chunks = C / CH;
    const size_t total = (size_t)N * chunks;
    hipLaunchKernelGGL(global_avgpool_kernel<T>, dim3(in_blocks(total)), dim3(IN_THREADS), 0, (hipStream_t)stream, x, ld, off, h * w,
                       C, chunks, out, total);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

}  // namespace

extern "C" int gcc_fid_resize(const float* x, int N, int H, int W, void* y, int ld, int off, int Ho, int Wo, gcc_stream_t stream) {
    return fid_resize_impl(x, N, H, W, (bf16_t*)y, ld, off, Ho, Wo, stream);
}

extern "C" int gcc_fid_resize_f32(const float* x, int N, int H, int W, float* y, int ld, int off, int Ho, int Wo,
                                  gcc_stream_t stream) {
    return fid_resize_impl(x, N, H, W, y, ld, off, Ho, Wo, stream);
}

extern "C" int gcc_pool3x3(int mode, const void* x, int ldx, int xoff, void* y, int ldy, int yoff, int N, int H, int W, int C,
                           gcc_stream_t stream) {
    return pool3x3_impl(mode, (const bf16_t*)x, ldx, xoff, (bf16_t*)y, ldy, yoff, N, H, W, C, stream);
}

extern "C" int gcc_pool3x3_f32(int mode, const float* x, int ldx, int xoff, float* y, int ldy, int yoff, int N, int H, int W, int C,
                               gcc_stream_t stream) {
    return pool3x3_impl(mode, x, ldx, xoff, y, ldy, yoff, N, H, W, C, stream);
}

extern "C" int gcc_border_copy(const void* src, int lds, int soff, void* dst, int ldd, int doff, int N, int H, int W, int C, int ph,
                               int pw, gcc_stream_t stream) {
    GCC_ENTER();
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || ph < 0 || pw < 0) return GCC_ERR_BAD_ARG;
    if (!in_window_ok(src, lds, soff, ceil8(C)) || !in_window_ok(dst, ldd, doff, ceil8(C))) return GCC_ERR_BAD_ARG;
    if (C & 7) return GCC_ERR_UNSUPPORTED;
    if (ph > (1 << 15) || pw > (1 << 15)) return GCC_ERR_UNSUPPORTED;
    const size_t spix = (size_t)N * H * W, dpix = (size_t)N * (H + 2 * ph) * (W + 2 * pw);
    if (spix * lds >= (size_t)1 << 40 || dpix * ldd >= (size_t)1 << 40) return GCC_ERR_UNSUPPORTED;
    {   // never in place: a destination pixel is another source pixel's address
        const char* a = (const char*)src; const char* b = (const char*)dst;
        if (a < b + dpix * ldd * 2 && b < a + spix * lds * 2) return GCC_ERR_BAD_ARG;
    }
    const int chunks = C / 8;
    const size_t total = dpix * chunks;
    hipLaunchKernelGGL(border_copy_kernel, dim3(in_blocks(total)), dim3(IN_THREADS), 0, (hipStream_t)stream, (const bf16_t*)src, lds,
                       soff, (bf16_t*)dst, ldd, doff, H, W, ph, pw, chunks, total);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_global_avgpool(const void* x, int ld, int off, int N, int h, int w, int C, float* out, gcc_stream_t stream) {
    return global_avgpool_impl((const bf16_t*)x, ld, off, N, h, w, C, out, stream);
}

extern "C" int gcc_global_avgpool_f32(const float* x, int ld, int off, int N, int h, int w, int C, float* out, gcc_stream_t stream) {
    return global_avgpool_impl(x, ld, off, N, h, w, C, out, stream);
}

extern "C" int gcc_map_mean_segments(int h, int w, int C) {
    if (h <= 0 || w <= 0 || C <= 0 || (C & 3)) return 0;
    return map_mean_segments((size_t)h * w, C);
}

extern "C" size_t gcc_map_mean_workspace(int N, int h, int w, int C) {
    if (N <= 0 || h <= 0 || w <= 0 || C <= 0) return 0;
    return (size_t)N * map_mean_max_segments((size_t)h * w) * C * sizeof(double);
}

extern "C" int gcc_map_mean(const void* x, int ld, int off, int N, int h, int w, int C, int segments, float* out, void* ws,
                            size_t ws_bytes, gcc_stream_t stream) {
    return map_mean_impl((const bf16_t*)x, ld, off, N, h, w, C, segments, out, ws, ws_bytes, stream);
}

extern "C" int gcc_map_mean_f32(const float* x, int ld, int off, int N, int h, int w, int C, int segments, float* out, void* ws,
                                size_t ws_bytes, gcc_stream_t stream) {
    return map_mean_impl(x, ld, off, N, h, w, C, segments, out, ws, ws_bytes, stream);
}
