// The MobileResnet generator at the reference's own precision (engine.MobileResnetEngine.infer, precision 'fp32'): what its fp32
// program needs beyond gcc_conv_eval_f32_act (the k3 s2 p1 and 1 x 1 convolutions).  All tensors are NHWC fp32.
//
// gcc_conv_eval_f32_resnet   the fifth entry on the fp32 tile (conv_f32_tile.hpp: the implicit GEMM, its k loop and the single
//                            order of K, the body text conv_f32_tile_body.inc; conv_f32.hip has the other four), with two gathers:
//     REFLECT      Conv2d(k, s1, p0) behind ReflectionPad2d(k / 2): a tap outside the map reads its mirror pixel (ih < 0 -> -ih,
//                  ih >= H -> 2 (H - 1) - ih); no padded copy of the map exists
//     TRANSPOSED3  ConvTranspose2d(k3, s2, p1, output_padding 1): blockIdx.z is one of the four output parity phases, a gather of
//                  1 / 2 / 2 / 4 taps over the input stored at pixel stride 2; each phase walks only its own K
// gcc_dwconv3x3_reflect_f32  depthwise 3 x 3 behind ReflectionPad2d(1): bias and nine products as one fmaf chain per output; with a
//                            statistics pointer the launch also writes the InstanceNorm partials of its own output.
// gcc_inorm_stats_f32 / gcc_inorm_apply_f32   InstanceNorm2d(affine=False) in two launches.  A plane is cut into chunks whose
//   size depends on H W alone; per (image, chunk, channel) the stats launch writes the chunk's mean and M2 (the sum of squared
//   deviations from that mean) as doubles, from sums about a pivot (the chunk's first pixel).  The apply launch folds the chunks
//   of its channels in chunk order, in double, and normalises.  No workgroup waits for another; no atomics; no zero-fill contract.
#include "conv_f32_tile.hpp"

namespace {

constexpr int RF_THREADS = 256;                    // the depthwise and InstanceNorm kernels' workgroup

struct ConvF32ResnetArgs {
    const float* x; const float* w; float* y;
    const float* scale; const float* shift;
    int M, H, W, Ci, Cip, Co, KW, pad;             // M = N H W rows: REFLECT output pixels, TRANSPOSED3 input pixels (one phase's outputs)
    int ldx, xoff, ldy, yoff, Kreal, Kp, act;      // Kreal, Kp: REFLECT's; a TRANSPOSED3 phase derives its own
    FastDiv dW, dH, dCip, dKW;
};

__device__ __forceinline__ int rf_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// TR = false: row m is output pixel (n, oh, ow); tap = kh KW + kw reads the mirror of (oh - pad + kh, ow - pad + kw).
// TR = true: blockIdx.z = 2 ph + pw is the phase (its own packed weights, its own K), row m is input pixel (n, i, j) and output
// pixel (n, 2 i + ph, 2 j + pw) of [N][2 H][2 W].  The phase has (1 + ph) (1 + pw) taps, tap = th (1 + pw) + tw reading
// (i + th, j + tw) -- zeros beyond the map -- which is kernel element (ph ? 2 - 2 th : 1, pw ? 2 - 2 tw : 1) of ConvTranspose2d.
// A row beyond M (the tile's sentinel) has no mirror either.  The store is y = act(z); q = n H + i there.
// a: the kernel's ConvF32ResnetArgs in each of them.
#define CF_ROW(m, ih0, iw0, nb)                                                                        \
    const int q = fdiv(m, a.dW), c = m - q * a.W;                                                      \
    const int n = fdiv(q, a.dH), r = q - n * a.H;                                                      \
    ih0 = TR ? r : r - a.pad; iw0 = TR ? c : c - a.pad; nb = n * a.H * a.W
#define CF_TAP(k4)                                                                                     \
    const int tap = fdiv(k4, a.dCip), ci = k4 - tap * a.Cip;                                           \
    const bool kok = k4 < kreal;                                                                       \
    int dh, dw;                                                                                        \
    if (TR) { dh = pw ? tap >> 1 : tap; dw = pw ? tap & 1 : 0; }                                       \
    else { dh = fdiv(tap, a.dKW); dw = tap - dh * a.KW; }
#define CF_FETCH(v, ih0, iw0, nb)                                                                      \
    int ih = ih0 + dh, iw = iw0 + dw;                                                                  \
    bool ok = kok && ih0 > -(1 << 27);                                                                 \
    if (TR) ok = ok && ih < a.H && iw < a.W;                                                           \
    else { ih = rf_reflect(ih, a.H); iw = rf_reflect(iw, a.W); }                                       \
    if (ok) {                                                                                          \
        v = *(const f32x4*)(a.x + (size_t)(nb + ih * a.W + iw) * a.ldx + a.xoff + ci);                 \
        if (a.Ci == 3) v[3] = 0.f;                                                                     \
    }
#define CF_NK nk
#define CF_STORE_SETUP
#define CF_STORE(m, co, z)                                                                             \
    size_t p = (size_t)m;                                                                              \
    if (TR) {                                                                                          \
        const int q = fdiv(m, a.dW), c = m - q * a.W;                                                  \
        p = ((size_t)q * 2 + ph) * ((size_t)a.W * 2) + 2 * c + pw;                                     \
    }                                                                                                  \
    float v = z;                                                                                       \
    if (a.act == GCC_EVAL_ACT_RELU) v = v < 0.f ? 0.f : v;                                             \
    else if (a.act == GCC_EVAL_ACT_TANH) v = tanhf(v);                                                 \
    a.y[p * a.ldy + a.yoff + co] = v
template <int MI, int NI, int WM, int WN, bool TR>
__global__ __launch_bounds__(CF_THREADS) void conv_f32_resnet_kernel(ConvF32ResnetArgs a) {
#define CF_SETUP                                                                                       \
    const int ph = TR ? (int)(blockIdx.z >> 1) : 0, pw = TR ? (int)(blockIdx.z & 1) : 0;               \
    const float* wbase = a.w + (TR ? (size_t)blockIdx.z * a.Co * a.Kp : 0);                            \
    const int kreal = TR ? (1 + ph) * (1 + pw) * a.Ci : a.Kreal;                                       \
    const int nk = TR ? (kreal + CF_BK - 1) / CF_BK : a.Kp / CF_BK
#include "conv_f32_tile_body.inc"
}
#undef CF_SETUP
#undef CF_ROW
#undef CF_TAP
#undef CF_FETCH
#undef CF_NK
#undef CF_STORE_SETUP
#undef CF_STORE

// REFLECT: gcc_conv_eval_f32's packing; TRANSPOSED3: the row stride of all four phases, the four-tap phase's K
inline int rf_kp(int Ci, int kind, int k) { return cf_kp(Ci, kind == GCC_F32_RESNET_REFLECT ? (long long)k * k : 4); }

// the tile of a geometry, or the error the call returns for it
int rf_route(const gcc_conv_t* c, int kind) {
    if (!c || (kind != GCC_F32_RESNET_REFLECT && kind != GCC_F32_RESNET_TRANSPOSED3)) return GCC_ERR_BAD_ARG;
    const int bad = cf_common(c, c->pad, c->pad, 1);
    if (bad) return bad;
    const bool tr = kind == GCC_F32_RESNET_TRANSPOSED3;
    if (tr) {
        if (c->KH != 3 || c->KW != 3 || c->stride != 2) return GCC_ERR_UNSUPPORTED;
        if (c->pad != 1) return GCC_ERR_BAD_ARG;           // the generator's up convs have one padding; anything else is a mistake
        if (c->Ci & 7) return GCC_ERR_UNSUPPORTED;
    } else {
        if (c->KH != c->KW || (c->KH != 7 && c->KH != 3) || c->stride != 1) return GCC_ERR_UNSUPPORTED;
        if (c->pad != 0) return GCC_ERR_BAD_ARG;           // the padding is the reflection's, k / 2: the conv itself has none
        if (c->Ci != 3 && (c->Ci & 7)) return GCC_ERR_UNSUPPORTED;
        if (c->H <= c->KH / 2 || c->W <= c->KH / 2) return GCC_ERR_BAD_ARG;   // ReflectionPad2d needs the pad below the size
    }
    if (c->Co & 7) return GCC_ERR_UNSUPPORTED;
    if (c->ldx < c->xoff + cf_cip(c->Ci) || c->ldy < c->yoff + c->Co) return GCC_ERR_BAD_ARG;
    const long long M = (long long)c->N * c->H * c->W, Mout = tr ? 4 * M : M;
    if (Mout >= (1ll << 31) - 256 || (long long)c->KH * c->KW * cf_cip(c->Ci) >= (1ll << 30)) return GCC_ERR_UNSUPPORTED;
    return cf_tile(M, c->Co);
}

// ---- InstanceNorm partials ------------------------------------------------------------------------------------------------
// A plane of HW pixels is cut into chunks of in_chunk(HW) consecutive pixels (at most 64 chunks, at least 64 pixels each but the
// last): a function of HW alone.  Partials: double [N][chunks][2][C] -- the chunk's mean, then its M2.  A workgroup is
// quads x lanes threads: quads = the channel quads it serves (a power of two up to 16, chosen by C and the chunk size alone), lanes
// = 256 / quads pixel lanes; pixel lane l takes pixels l, l + lanes, ... of the chunk, always in that order.
inline int in_chunk(long long HW) {
    const long long c = ((HW + 63) / 64 + 15) / 16 * 16;
    return (int)(c < 64 ? 64 : c);
}
inline int in_chunks(long long HW) { return (int)((HW + in_chunk(HW) - 1) / in_chunk(HW)); }
inline int in_quads(int C, int chunk) {
    int q = 1;
    while (q < 16 && q * 4 < C) q *= 2;
    while (q > 4 && chunk / (RF_THREADS / q) > 8) q /= 2;          // a long chunk: more pixel lanes, at most ~8 pixels a thread
    return q;
}

struct InStatsAcc {
    f32x4 pivot;
    double s1[4], s2[4];
    __device__ __forceinline__ void init(const f32x4& p) {
        pivot = p;
#pragma unroll
        for (int j = 0; j < 4; j++) s1[j] = s2[j] = 0.0;
    }
    __device__ __forceinline__ void add(const f32x4& v) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double d = (double)(v[j] - pivot[j]);
            s1[j] += d;
            s2[j] = fma(d, d, s2[j]);
        }
    }
};

// the pixel lanes' sums about the pivot -> the chunk's mean and M2, lanes summed in ascending order in double by one thread per
// channel.  red: 2 * 256 * 4 doubles of LDS.  part: the (image, chunk) row of the partials, [2][C].
__device__ __forceinline__ void in_chunk_finish(const InStatsAcc& s, double* red, int quads, int q, int c0, int C, int count, double* part) {
    const int t = threadIdx.x, lanes = RF_THREADS / quads, pl = t / quads;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        red[(pl * quads + q) * 4 + j] = s.s1[j];
        red[RF_THREADS * 4 + (pl * quads + q) * 4 + j] = s.s2[j];
    }
    __syncthreads();
    if (t < quads * 4 && c0 + t < C) {
        double S1 = 0.0, S2 = 0.0;
        for (int l = 0; l < lanes; l++) {
            S1 += red[l * quads * 4 + t];
            S2 += red[RF_THREADS * 4 + l * quads * 4 + t];
        }
        const double pivot = (double)red[2 * RF_THREADS * 4 + t];
        double m2 = S2 - S1 * S1 / count;
        part[c0 + t] = pivot + S1 / count;
        part[C + c0 + t] = m2 < 0.0 ? 0.0 : m2;
    }
}

// grid (chunks, channel groups, N)
__global__ __launch_bounds__(RF_THREADS) void inorm_stats_f32_kernel(const float* __restrict__ x, int ldx, int HW, int C, int chunk,
                                                                      int quads, double* __restrict__ part) {
    __shared__ double red[2 * RF_THREADS * 4 + 64];
    const int t = threadIdx.x, q = t % quads, pl = t / quads, lanes = RF_THREADS / quads;
    const int c0 = blockIdx.y * quads * 4, c = c0 + q * 4;
    const int p0 = blockIdx.x * chunk, count = min(chunk, HW - p0);
    const float* xb = x + ((size_t)blockIdx.z * HW + p0) * ldx;
    InStatsAcc s;
    const bool live = c < C;
    f32x4 pv = {0.f, 0.f, 0.f, 0.f};
    if (live) pv = *(const f32x4*)(xb + c);
    s.init(pv);
    if (pl == 0)
#pragma unroll
        for (int j = 0; j < 4; j++) red[2 * RF_THREADS * 4 + q * 4 + j] = (double)pv[j];
    if (live) {
        int p = pl;
        for (; p + 3 * lanes < count; p += 4 * lanes) {                 // four loads in flight; added in pixel order
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = *(const f32x4*)(xb + (size_t)(p + u * lanes) * ldx + c);
#pragma unroll
            for (int u = 0; u < 4; u++) s.add(v[u]);
        }
        for (; p < count; p += lanes) s.add(*(const f32x4*)(xb + (size_t)p * ldx + c));
    }
    in_chunk_finish(s, red, quads, q, c0, C, count, part + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * 2 * C);
}

// grid (pixel spans of IN_APPLY_PIXELS, channel groups, N): fold the chunks of this group's channels, then y = act((x - mean) rstd) + r
constexpr int IN_APPLY_PIXELS = 256;
__global__ __launch_bounds__(RF_THREADS) void inorm_apply_f32_kernel(const float* x, int ldx, float* y, int ldy, const float* r, int ldr, int HW, int C, int chunk,
                                                                      int chunks, int quads, const double* __restrict__ part, double eps,
                                                                      int relu) {
    __shared__ double mean_s[64], rstd_s[64];
    const int t = threadIdx.x, q = t % quads, pl = t / quads, lanes = RF_THREADS / quads;
    const int c0 = blockIdx.y * quads * 4, c = c0 + q * 4;
    if (t < quads * 4 && c0 + t < C) {
        const double* pp = part + (size_t)blockIdx.z * chunks * 2 * C + c0 + t;
        // both folds walk the chunks in ascending order; the loads of 16 chunks are issued together
        double sum = 0.0, m2 = 0.0;
        for (int k0 = 0; k0 < chunks; k0 += 16) {
            double m[16];
#pragma unroll
            for (int u = 0; u < 16; u++) m[u] = k0 + u < chunks ? pp[(size_t)(k0 + u) * 2 * C] : 0.0;
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (k0 + u < chunks) sum += m[u] * (double)min(chunk, HW - (k0 + u) * chunk);
        }
        const double mean = sum / HW;
        for (int k0 = 0; k0 < chunks; k0 += 16) {
            double m[16], q2[16];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                m[u] = k0 + u < chunks ? pp[(size_t)(k0 + u) * 2 * C] : 0.0;
                q2[u] = k0 + u < chunks ? pp[(size_t)(k0 + u) * 2 * C + C] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (k0 + u < chunks) {
                    const double d = m[u] - mean;
                    m2 += q2[u] + d * d * (double)min(chunk, HW - (k0 + u) * chunk);
                }
        }
        mean_s[t] = mean;
        rstd_s[t] = 1.0 / sqrt(m2 / HW + eps);
    }
    __syncthreads();
    if (c >= C) return;
    double mean[4], rstd[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { mean[j] = mean_s[q * 4 + j]; rstd[j] = rstd_s[q * 4 + j]; }
    const int p0 = blockIdx.x * IN_APPLY_PIXELS, p1 = min(p0 + IN_APPLY_PIXELS, HW);
    const size_t base = (size_t)blockIdx.z * HW;
    auto one = [&](int p, const f32x4& v, const f32x4& rv) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            o[j] = (float)(((double)v[j] - mean[j]) * rstd[j]);
            if (relu) o[j] = o[j] < 0.f ? 0.f : o[j];
            o[j] += rv[j];
        }
        *(f32x4*)(y + (base + p) * ldy + c) = o;
    };
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    int p = p0 + pl;
    for (; p + 3 * lanes < p1; p += 4 * lanes) {                        // four pixels' loads in flight
        f32x4 v[4], rv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            v[u] = *(const f32x4*)(x + (base + p + u * lanes) * ldx + c);
            rv[u] = r ? *(const f32x4*)(r + (base + p + u * lanes) * ldr + c) : zero;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) one(p + u * lanes, v[u], rv[u]);
    }
    for (; p < p1; p += lanes)
        one(p, *(const f32x4*)(x + (base + p) * ldx + c), r ? *(const f32x4*)(r + (base + p) * ldr + c) : zero);
}

// ---- depthwise 3 x 3 behind ReflectionPad2d(1) ------------------------------------------------------------------------------
// w: [9][C] tap-major, b: [C].  The chain: acc = b; acc = fmaf(x(kh, kw), w(kh, kw), acc) for kh, kw ascending.
__device__ __forceinline__ f32x4 dw_pixel(const float* __restrict__ xi, int ldx, int H, int W, int oh, int ow, const f32x4* wq, const f32x4& bq) {
    f32x4 acc = bq;
#pragma unroll
    for (int kh = 0; kh < 3; kh++) {
        const int ih = rf_reflect(oh - 1 + kh, H);
#pragma unroll
        for (int kw = 0; kw < 3; kw++) {
            const int iw = rf_reflect(ow - 1 + kw, W);
            const f32x4 v = *(const f32x4*)(xi + ((size_t)ih * W + iw) * ldx);
#pragma unroll
            for (int j = 0; j < 4; j++) acc[j] = fmaf(v[j], wq[kh * 3 + kw][j], acc[j]);
        }
    }
    return acc;
}

// grid (chunks, channel groups, N): the workgroup owns one chunk of one image's pixels (the InstanceNorm chunking) for its channels
template <bool STATS>
__global__ __launch_bounds__(RF_THREADS) void dwconv3x3_reflect_f32_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y,
                                                                            int ldy, const float* __restrict__ w, const float* __restrict__ b,
                                                                            int H, int W, int C, int chunk, int quads,
                                                                            double* __restrict__ part) {
    __shared__ double red[STATS ? 2 * RF_THREADS * 4 + 64 : 1];
    const int t = threadIdx.x, q = t % quads, pl = t / quads, lanes = RF_THREADS / quads;
    const int c0 = blockIdx.y * quads * 4, c = c0 + q * 4;
    const int HW = H * W, p0 = blockIdx.x * chunk, count = min(chunk, HW - p0);
    const bool live = c < C;
    const float* xi = x + (size_t)blockIdx.z * HW * ldx + c;
    float* yo = y + (size_t)blockIdx.z * HW * ldy + c;
    f32x4 wq[9], bq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 9; k++) wq[k] = live ? *(const f32x4*)(w + (size_t)k * C + c) : bq;
    if (live) bq = *(const f32x4*)(b + c);
    InStatsAcc s;
    if (STATS) {
        f32x4 pv = {0.f, 0.f, 0.f, 0.f};
        if (live) pv = dw_pixel(xi, ldx, H, W, p0 / W, p0 % W, wq, bq);       // the pivot: the chunk's first output pixel
        s.init(pv);
        if (pl == 0)
#pragma unroll
            for (int j = 0; j < 4; j++) red[2 * RF_THREADS * 4 + q * 4 + j] = (double)pv[j];
    }
    if (live)
        for (int p = pl; p < count; p += lanes) {
            const int pix = p0 + p, oh = pix / W, ow = pix - oh * W;
            const f32x4 v = dw_pixel(xi, ldx, H, W, oh, ow, wq, bq);
            *(f32x4*)(yo + (size_t)pix * ldy) = v;
            if (STATS) s.add(v);
        }
    if (STATS) in_chunk_finish(s, red, quads, q, c0, C, count, part + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * 2 * C);
}

// what the three plane entries refuse alike: 0 when there is nothing to refuse
int in_common(const void* x, int ldx, const void* y, int ldy, int N, long long HW, int C) {
    if (!x || !y || N <= 0 || HW <= 0 || C <= 0 || ldx <= 0 || ldy <= 0) return GCC_ERR_BAD_ARG;
    if ((ldx & 3) || (ldy & 3) || ldx < C || ldy < C || ((((uintptr_t)x) | ((uintptr_t)y)) & 15)) return GCC_ERR_BAD_ARG;
    if (C & 3) return GCC_ERR_UNSUPPORTED;
    if (HW >= (1ll << 31) || (long long)N * HW >= (1ll << 31) || N > 65535 || C > 65535 * 4) return GCC_ERR_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int gcc_conv_eval_f32_resnet_kp(int Ci, int kind, int k) {
    if (Ci <= 0 || (kind != GCC_F32_RESNET_REFLECT && kind != GCC_F32_RESNET_TRANSPOSED3)) return GCC_ERR_BAD_ARG;
    if (kind == GCC_F32_RESNET_TRANSPOSED3 ? k != 3 : (k != 3 && k != 7)) return GCC_ERR_BAD_ARG;
    if ((long long)k * k * cf_cip(Ci) >= (1ll << 30)) return GCC_ERR_BAD_ARG;
    return rf_kp(Ci, kind, k);
}

extern "C" int gcc_conv_eval_f32_resnet_route(const gcc_conv_t* c, int kind) { return rf_route(c, kind); }

extern "C" int gcc_conv_eval_f32_resnet(const gcc_conv_t* c, int kind, const float* x, const float* w, float* y,
                                        const gcc_eval_f32_resnet_epilogue_t* ep, gcc_stream_t stream) {
    GCC_ENTER();
    if (!c || !x || !w || !y || !ep) return GCC_ERR_BAD_ARG;
    if (ep->act != GCC_EVAL_ACT_NONE && ep->act != GCC_EVAL_ACT_RELU && ep->act != GCC_EVAL_ACT_TANH) return GCC_ERR_BAD_ARG;
    const int route = rf_route(c, kind);
    if (route < 0) return route;
    if ((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)y)) & 15) return GCC_ERR_BAD_ARG;
    const bool tr = kind == GCC_F32_RESNET_TRANSPOSED3;
    ConvF32ResnetArgs a;
    a.x = x; a.w = w; a.y = y; a.scale = ep->scale; a.shift = ep->shift;
    a.M = c->N * c->H * c->W; a.H = c->H; a.W = c->W;
    a.Ci = c->Ci; a.Cip = cf_cip(c->Ci); a.Co = c->Co; a.KW = c->KW; a.pad = c->KH / 2;
    a.ldx = c->ldx; a.xoff = c->xoff; a.ldy = c->ldy; a.yoff = c->yoff;
    a.Kreal = c->KH * c->KW * a.Cip; a.Kp = rf_kp(c->Ci, kind, c->KH);
    a.act = ep->act;
    a.dW = make_fastdiv(a.W); a.dH = make_fastdiv(a.H); a.dCip = make_fastdiv(a.Cip); a.dKW = make_fastdiv(a.KW);
    if (tr) CF_LAUNCH_TILE(conv_f32_resnet_kernel, true, a, 4, route, (hipStream_t)stream);
    else CF_LAUNCH_TILE(conv_f32_resnet_kernel, false, a, 1, route, (hipStream_t)stream);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" size_t gcc_inorm_f32_workspace(int N, int C, long long HW) {
    if (N <= 0 || C <= 0 || HW <= 0) return 0;
    return (size_t)N * in_chunks(HW) * 2 * C * sizeof(double);
}

extern "C" int gcc_inorm_stats_f32(const float* x, int ldx, int N, int H, int W, int C, void* workspace, size_t workspace_bytes,
                                   gcc_stream_t stream) {
    GCC_ENTER();
    if (H <= 0 || W <= 0) return GCC_ERR_BAD_ARG;
    const long long HW = (long long)H * W;
    const int bad = in_common(x, ldx, x, ldx, N, HW, C);
    if (bad) return bad;
    if (!workspace || (((uintptr_t)workspace) & 15)) return GCC_ERR_BAD_ARG;
    if (workspace_bytes < gcc_inorm_f32_workspace(N, C, HW)) return GCC_ERR_WORKSPACE;
    const int quads = in_quads(C, in_chunk(HW));
    hipLaunchKernelGGL(inorm_stats_f32_kernel, dim3(in_chunks(HW), cdiv(C / 4, quads), N), dim3(RF_THREADS), 0, (hipStream_t)stream, x,
                       ldx, (int)HW, C, in_chunk(HW), quads, (double*)workspace);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_inorm_apply_f32(const float* x, int ldx, float* y, int ldy, const float* residual, int ld_residual, int N, int H,
                                   int W, int C, int act, float eps, const void* workspace, size_t workspace_bytes,
                                   gcc_stream_t stream) {
    GCC_ENTER();
    if (H <= 0 || W <= 0) return GCC_ERR_BAD_ARG;
    const long long HW = (long long)H * W;
    const int bad = in_common(x, ldx, y, ldy, N, HW, C);
    if (bad) return bad;
    if (act != GCC_EVAL_ACT_NONE && act != GCC_EVAL_ACT_RELU) return GCC_ERR_BAD_ARG;
    if (residual && (ld_residual <= 0 || (ld_residual & 3) || ld_residual < C || (((uintptr_t)residual) & 15))) return GCC_ERR_BAD_ARG;
    if (!workspace || (((uintptr_t)workspace) & 15) || !(eps >= 0.f)) return GCC_ERR_BAD_ARG;
    if (workspace_bytes < gcc_inorm_f32_workspace(N, C, HW)) return GCC_ERR_WORKSPACE;
    const int quads = in_quads(C, in_chunk(HW));
    hipLaunchKernelGGL(inorm_apply_f32_kernel, dim3(cdiv((int)HW, IN_APPLY_PIXELS), cdiv(C / 4, quads), N), dim3(RF_THREADS), 0,
                       (hipStream_t)stream, x, ldx, y, ldy, residual, residual ? ld_residual : 0, (int)HW, C, in_chunk(HW), in_chunks(HW),
                       quads, (const double*)workspace, (double)eps, act == GCC_EVAL_ACT_RELU ? 1 : 0);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_dwconv3x3_reflect_f32(const float* x, int ldx, float* y, int ldy, const float* w, const float* bias, int N, int H,
                                         int W, int C, void* stats, size_t stats_bytes, gcc_stream_t stream) {
    GCC_ENTER();
    if (H < 2 || W < 2) return GCC_ERR_BAD_ARG;            // ReflectionPad2d(1) needs two pixels a side
    const long long HW = (long long)H * W;
    const int bad = in_common(x, ldx, y, ldy, N, HW, C);
    if (bad) return bad;
    if (!w || !bias || ((((uintptr_t)w) | ((uintptr_t)bias) | ((uintptr_t)stats)) & 15)) return GCC_ERR_BAD_ARG;
    if (stats && stats_bytes < gcc_inorm_f32_workspace(N, C, HW)) return GCC_ERR_WORKSPACE;
    const int quads = in_quads(C, in_chunk(HW));
    const dim3 grid(in_chunks(HW), cdiv(C / 4, quads), N);
    if (stats)
        hipLaunchKernelGGL(dwconv3x3_reflect_f32_kernel<true>, grid, dim3(RF_THREADS), 0, (hipStream_t)stream, x, ldx, y, ldy, w, bias, H, W,
                           C, in_chunk(HW), quads, (double*)stats);
    else
        hipLaunchKernelGGL(dwconv3x3_reflect_f32_kernel<false>, grid, dim3(RF_THREADS), 0, (hipStream_t)stream, x, ldx, y, ldy, w, bias, H,
                           W, C, in_chunk(HW), quads, (double*)nullptr);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
