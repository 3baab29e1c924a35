// Layout packing, weight packing, losses, distillation loss glue and multi-tensor Adam.
#include <atomic>
#include <mutex>
#include <stdlib.h>
#include <string.h>
#include "common.hpp"
#include <algorithm>

int gcc_internal_igemm(const gcc_conv_t* c, int dgrad, const void* src, const void* w, void* dst, const gcc_epilogue_t* ep,
                       int batch, long src_bstride, long wgt_bstride, long dst_bstride, hipStream_t st);
size_t gcc_internal_wgrad_workspace(const gcc_conv_t* c, int batch);
int gcc_internal_wgrad(const gcc_conv_t* c, const void* x, const void* dy, float* dw, int accumulate, void* ws,
                       size_t ws_bytes, int batch, long x_bstride, long dy_bstride, hipStream_t st, int rows_l, int cols_l,
                       int row_split, int col_split);
int gcc_internal_wgrad_plan(const gcc_conv_t* c, int batch, int out[6]);                  // conv_wgrad.hip
int gcc_internal_igemm_plan(const gcc_conv_t* c, int dgrad, int batch, int out[6]);       // conv_igemm.hip

namespace {

static int grid_for(size_t n, int per_block = 256, int cap = 4096) {
    size_t b = (n + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > (size_t)cap) b = cap;
    return (int)b;
}

// ---------------------------------------------------------------------------------------------
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int N, int C, int HW, int ld,
                                    int off, int Cfill) {
    const size_t total = (size_t)N * HW;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t n = i / HW, r = i - n * HW;
        bf16_t* d = dst + i * ld + off;
        for (int c = 0; c < C; c++) d[c] = f2bf(src[(n * C + c) * HW + r]);
        for (int c = C; c < Cfill; c++) d[c] = 0;
    }
}
__global__ void nhwc_to_nchw_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, int N, int C, int HW, int ld,
                                    int off) {
    const size_t total = (size_t)N * HW;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t n = i / HW, r = i - n * HW;
        const bf16_t* s = src + i * ld + off;
        for (int c = 0; c < C; c++) dst[(n * C + c) * HW + r] = bf2f(s[c]);
    }
}
// vector path (everything a multiple of 8) and scalar path
__global__ void nhwc_copy_vec_kernel(const bf16_t* __restrict__ src, int lds, int soff, bf16_t* __restrict__ dst, int ldd,
                                     int doff, int CH, size_t pixels, int add) {
    const size_t total = pixels * CH;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i / CH;
        const int ch = (int)(i - pix * CH);
        const i32x4 v = *(const i32x4*)(src + pix * lds + soff + ch * 8);
        i32x4* d = (i32x4*)(dst + pix * ldd + doff + ch * 8);
        if (add) {
            float a[8], b[8];
            unpack8(v, a); unpack8(*d, b);
#pragma unroll
            for (int j = 0; j < 8; j++) a[j] += b[j];
            *d = pack8(a);
        } else {
            *d = v;
        }
    }
}
// thin slices whose source and destination each sit inside one aligned 8-channel group (the 3-channel images): 16-byte
// accesses; the destination group is read back only when part of it survives
__global__ __launch_bounds__(256) void nhwc_copy_group_kernel(const bf16_t* __restrict__ src, int lds, int soff, bf16_t* __restrict__ dst,
                                                              int ldd, int doff, int C, int Cfill, size_t pixels, int add) {
    const int sg = soff & ~7, s0 = soff & 7, dg = doff & ~7, d0 = doff & 7;
    const bool whole = !add && d0 == 0 && Cfill == 8;
    for (size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x; pix < pixels; pix += (size_t)gridDim.x * 256) {
        bf16_t es[8], ed[8];
        *(i32x4*)es = *(const i32x4*)(src + pix * lds + sg);
        if (whole) *(i32x4*)ed = i32x4{0, 0, 0, 0};
        else *(i32x4*)ed = *(const i32x4*)(dst + pix * ldd + dg);
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int k = c - d0;                       // index into the copied slice
            if (k >= 0 && k < C) {
                const bf16_t v = es[(s0 + k) & 7];
                ed[c] = add ? f2bf(bf2f(ed[c]) + bf2f(v)) : v;
            } else if (!add && k >= C && k < Cfill) {
                ed[c] = 0;
            }
        }
        *(i32x4*)(dst + pix * ldd + dg) = *(const i32x4*)ed;
    }
}
__global__ void nhwc_copy_scalar_kernel(const bf16_t* __restrict__ src, int lds, int soff, bf16_t* __restrict__ dst, int ldd,
                                        int doff, int C, int Cfill, size_t pixels, int add) {
    for (size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pix < pixels; pix += (size_t)gridDim.x * blockDim.x) {
        const bf16_t* s = src + pix * lds + soff;
        bf16_t* d = dst + pix * ldd + doff;
        for (int c = 0; c < C; c++) d[c] = add ? f2bf(bf2f(d[c]) + bf2f(s[c])) : s[c];
        if (!add)
            for (int c = C; c < Cfill; c++) d[c] = 0;
    }
}

// fp32 master [rows][taps][cols] -> W [rows][taps][colsp] , Wt [cols][taps][rowsp]
__global__ void pack_w_kernel(const float* __restrict__ m, int rows, int taps, int cols, int colsp, bf16_t* __restrict__ w) {
    const size_t total = (size_t)rows * taps * colsp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % colsp);
        const size_t rt = i / colsp;
        w[i] = c < cols ? f2bf(m[rt * cols + c]) : (bf16_t)0;
    }
}
__global__ void pack_wt_kernel(const float* __restrict__ m, int rows, int taps, int cols, int rowsp, bf16_t* __restrict__ wt) {
    // tile transpose through LDS: block = (32 rows x 32 cols) of one tap
    __shared__ float t[32][33];
    const int tap = blockIdx.z;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: ty 0..7
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        t[k][tx] = (r < rows && c < cols) ? m[((size_t)r * taps + tap) * cols + c] : 0.f;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, r = r0 + tx;
        if (c < cols && r < rowsp) wt[((size_t)c * taps + tap) * rowsp + r] = f2bf(t[tx][k]);
    }
}

// multi-tensor form: one launch repacks every conv of an optimizer group (device work list)
__global__ __launch_bounds__(256) void pack_multi_kernel(const gcc_pack_desc_t* __restrict__ descs,
                                                         const gcc_pack_item_t* __restrict__ items) {
    __shared__ float t[64][65];
    const gcc_pack_item_t it = items[blockIdx.x];
    const gcc_pack_desc_t d = descs[it.tensor];
    if (it.kind == 2) {
        // W and Wt of one 64 x 64 tile (rows b*64.., columns c*64..) of tap a, unsplit tensors with cols % 4 == 0: the fp32
        // master is read once for both packings (kinds 0 + 1 read it twice and wrote Wt in 64-byte pieces: the launch ran at a
        // third of its HBM time), 128-byte row pieces in and out, zero rows / columns up to the padded sizes.
        const int tap = it.a, r0 = it.b * 64, c0 = it.c * 64;
        const int cq = threadIdx.x & 15, rr = threadIdx.x >> 4;
        bf16_t* w = (bf16_t*)d.w;
        bf16_t* wt = (bf16_t*)d.wt;
#pragma unroll
        for (int pass = 0; pass < 4; pass++) {
            const int lr = rr + 16 * pass, r = r0 + lr, c = c0 + cq * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (r < d.rows && c < d.cols) v = *(const f32x4*)(d.master + ((size_t)r * d.taps + tap) * d.cols + c);
            t[lr][cq * 4 + 0] = v[0]; t[lr][cq * 4 + 1] = v[1]; t[lr][cq * 4 + 2] = v[2]; t[lr][cq * 4 + 3] = v[3];
            if (w && r < d.rowsp && c < d.colsp) {
                i32x2 o;
                o[0] = (int)pack2bf(v[0], v[1]); o[1] = (int)pack2bf(v[2], v[3]);
                *(i32x2*)(w + ((size_t)r * d.taps + tap) * d.colsp + c) = o;
            }
        }
        __syncthreads();
        if (wt) {
#pragma unroll
            for (int pass = 0; pass < 4; pass++) {
                const int lc = rr + 16 * pass, c = c0 + lc, r = r0 + cq * 4;
                if (c < d.colsp && r < d.rowsp) {
                    i32x2 o;
                    o[0] = (int)pack2bf(t[cq * 4 + 0][lc], t[cq * 4 + 1][lc]); o[1] = (int)pack2bf(t[cq * 4 + 2][lc], t[cq * 4 + 3][lc]);
                    *(i32x2*)(wt + ((size_t)c * d.taps + tap) * d.rowsp + r) = o;
                }
            }
        }
        return;
    }
    if (it.kind == 0) {                 // W: [rowsp][taps][colsp], linear chunk of 2048 elements
        const size_t total = (size_t)d.rowsp * d.taps * d.colsp;
        const size_t beg = (size_t)it.a * 2048;
        bf16_t* w = (bf16_t*)d.w;
        if (d.cols == d.colsp && d.row_split == 0 && d.col_split == 0 && !((uintptr_t)d.master & 15)) {
            // unsplit widths that are multiples of 8: the packing is the master cast to bf16 (plus zero rows), 8 per thread
            const size_t i = beg + (size_t)threadIdx.x * 8;
            if (i < total) {
                i32x4 o = {0, 0, 0, 0};
                if ((int)(i / ((size_t)d.taps * d.colsp)) < d.rows) {
                    const f32x4 lo = *(const f32x4*)(d.master + i), hi = *(const f32x4*)(d.master + i + 4);
                    o[0] = (int)pack2bf(lo[0], lo[1]); o[1] = (int)pack2bf(lo[2], lo[3]);
                    o[2] = (int)pack2bf(hi[0], hi[1]); o[3] = (int)pack2bf(hi[2], hi[3]);
                }
                *(i32x4*)(w + i) = o;
            }
            return;
        }
        for (size_t i = beg + threadIdx.x; i < beg + 2048 && i < total; i += 256) {
            const int cp = (int)(i % d.colsp);
            const size_t rt = i / d.colsp;
            const int tap = (int)(rt % d.taps);
            const int lr = seg_to_logical((int)(rt / d.taps), d.rows, d.row_split);
            const int lc = seg_to_logical(cp, d.cols, d.col_split);
            w[i] = (lr >= 0 && lc >= 0) ? f2bf(d.master[((size_t)lr * d.taps + tap) * d.cols + lc]) : (bf16_t)0;
        }
    } else {                            // Wt: [colsp][taps][rowsp], one 32x32 tile (physical indices) of one tap
        const int tap = it.a, r0 = it.b * 32, c0 = it.c * 32;
        const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
        for (int k = ty; k < 32; k += 8) {
            const int lr = seg_to_logical(r0 + k, d.rows, d.row_split);
            const int lc = seg_to_logical(c0 + tx, d.cols, d.col_split);
            t[k][tx] = (lr >= 0 && lc >= 0) ? d.master[((size_t)lr * d.taps + tap) * d.cols + lc] : 0.f;
        }
        __syncthreads();
        bf16_t* wt = (bf16_t*)d.wt;
        for (int k = ty; k < 32; k += 8) {
            const int c = c0 + k, r = r0 + tx;
            if (c < d.colsp && r < d.rowsp) wt[((size_t)c * d.taps + tap) * d.rowsp + r] = f2bf(t[tx][k]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// block-wide sum (256 threads) -> thread 0
__device__ __forceinline__ float block_sum256(float v, float* sh) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    float t = 0.f;
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; i++) t += sh[i];
    return t;
}

// GANLoss over a 1-channel PatchGAN map; single block (the map is a few 10^4 values)
__global__ __launch_bounds__(1024) void gan_loss_kernel(int mode, int real, int ford, const bf16_t* __restrict__ pred, int ld,
                                                        int off, size_t pixels, float weight, float* loss, int accumulate,
                                                        bf16_t* dpred, float gweight, const float* gweight_dev,
                                                        int dpred_accumulate) {
    __shared__ float sh[16];
    const float inv = 1.f / (float)pixels;
    const float gw = gweight * (gweight_dev ? gweight_dev[0] : 1.f);
    float acc = 0.f;
    auto one = [&](size_t i, float x, float prev) {
        float l, d;
        if (mode == 0) {          // hinge
            if (ford) {
                const float z = real ? x - 1.f : -x - 1.f;
                l = -(z < 0.f ? z : 0.f);
                const float dz = z < 0.f ? -1.f : (z == 0.f ? -0.5f : 0.f);
                d = real ? dz : -dz;
            } else { l = -x; d = -1.f; }
        } else if (mode == 1) {   // lsgan
            const float t = real ? 1.f : 0.f;
            l = (x - t) * (x - t); d = 2.f * (x - t);
        } else if (mode == 2) {   // vanilla: BCE with logits
            const float t = real ? 1.f : 0.f;
            l = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
            d = 1.f / (1.f + expf(-x)) - t;
        } else {                  // wgangp
            l = real ? -x : x; d = real ? -1.f : 1.f;
        }
        acc += l;
        if (dpred) {
            float o[8] = {gw * d * inv + prev, 0, 0, 0, 0, 0, 0, 0};
            *(i32x4*)(dpred + i * ld + off) = pack8(o);
        }
    };
    // single workgroup (the map is ~10^4 values): eight elements per thread in flight -- the 16 x 30 x 30 map of the headline
    // configuration in two round trips per thread (four in flight: four dependent trips, 10.8 us per launch; sixteen spill under __launch_bounds__(1024) and take 19 us; fifteen launches
    // per iteration on the chains between a discriminator's forward and its backward pass)
    const size_t bd = blockDim.x;
    const bool rd = dpred && dpred_accumulate;
    constexpr int U = 8;
    for (size_t i0 = threadIdx.x; i0 < pixels; i0 += U * bd) {
        float x[U], pv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t i = i0 + u * bd;
            x[u] = i < pixels ? bf2f(pred[i * ld + off]) : 0.f;
            pv[u] = (rd && i < pixels) ? bf2f(dpred[i * ld + off]) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (i0 + u * bd < pixels) one(i0 + u * bd, x[u], pv[u]);
    }
    const float t = block_sum256(acc, sh);
    if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + weight * t * inv;
}

// stage 1 of L1 / squared-difference reductions over C channels of NHWC tensors
struct DiffArgs {
    const bf16_t* a; int lda, aoff; const bf16_t* b; int ldb, boff; int C, CH; size_t pixels;
    float* partial; bf16_t* da; int ldda, daoff; float gscale; int mode;   // mode 0: |a-b| ; 1, 2: (a-b)^2 (2: with gradient)
};
__global__ __launch_bounds__(256) void diff_reduce_kernel(const DiffArgs g) {
    __shared__ float sh[4];
    const size_t total = g.pixels * g.CH;
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t pix = i / g.CH;
        const int c0 = (int)(i - pix * g.CH) * 8;
        float av[8], bv[8], dv[8];
        unpack8(*(const i32x4*)(g.a + pix * g.lda + g.aoff + c0), av);
        unpack8(*(const i32x4*)(g.b + pix * g.ldb + g.boff + c0), bv);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float d = (c0 + j < g.C) ? av[j] - bv[j] : 0.f;
            if (g.mode == 0) { acc += fabsf(d); dv[j] = d > 0.f ? g.gscale : (d < 0.f ? -g.gscale : 0.f); }
            else { acc += d * d; dv[j] = g.gscale * d; }            // mode 2: gscale = 2 * weight / count
        }
        if (g.da) *(i32x4*)(g.da + pix * g.ldda + g.daoff + c0) = pack8(dv);
    }
    const float t = block_sum256(acc, sh);
    if (threadIdx.x == 0) g.partial[blockIdx.x] = t;
}
// stage 2: out = f(sum partial): mode 0: (+)= weight*sum/count ; mode 1: sqrt(sum/count) ; mode 2: sum/count
__global__ __launch_bounds__(256) void scalar_finalize_kernel(const float* partial, int n, double count, float weight,
                                                              float* out, int accumulate, int mode) {
    __shared__ float sh[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    const float t = block_sum256(acc, sh);
    if (threadIdx.x == 0) {
        if (mode == 0) out[0] = (accumulate ? out[0] : 0.f) + weight * (float)((double)t / count);
        else if (mode == 1) out[0] = sqrtf((float)((double)t / count));
        else out[0] = (float)((double)t / count);
    }
}

// ---------------------------------------------------------------------------------------------
// distillation: D = (Gf - Gt)/(C*HW) -> bf16 weights S, partial sums of D^2
__global__ __launch_bounds__(256) void gram_diff_kernel(const float* __restrict__ gf, const float* __restrict__ gt, size_t n,
                                                        float inv_chw, bf16_t* __restrict__ s, float* partial) {
    __shared__ float sh[4];
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float d = (gf[i] - gt[i]) * inv_chw;
        acc += d * d;
        s[i] = f2bf(d);
    }
    const float t = block_sum256(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}
// df = kg * dfg + kc * (f - t),  kg = wg*2/(N*C*C*Lg*C*HW),  kc = wc/(N*C*HW*Lc)   (RMSE terms, Pix2Pix)
// squared (plain MSE terms, CycleGAN): d(L^2) = 2 L dL  ->  kg = 2*kg0, kc = 2*kc0
__global__ __launch_bounds__(256) void distill_combine_kernel(const bf16_t* __restrict__ f, int ldf, int foff,
                                                              const bf16_t* __restrict__ t, int ldt, int toff,
                                                              const bf16_t* __restrict__ dfg, int CH, size_t pixels,
                                                              const float* scal, float kg0, float kc0, int squared,
                                                              bf16_t* __restrict__ df, int lddf, int dfoff) {
    const float kg = squared ? 2.f * kg0 : kg0 / scal[0], kc = squared ? 2.f * kc0 : kc0 / scal[1];
    const size_t total = pixels * CH;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t pix = i / CH;
        const int c0 = (int)(i - pix * CH) * 8;
        float fv[8], tv[8], gv[8], o[8];
        unpack8(*(const i32x4*)(f + pix * ldf + foff + c0), fv);
        unpack8(*(const i32x4*)(t + pix * ldt + toff + c0), tv);
        unpack8(*(const i32x4*)(dfg + (pix * CH) * 8 + c0), gv);
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = kg * gv[j] + kc * (fv[j] - tv[j]);
        *(i32x4*)(df + pix * lddf + dfoff + c0) = pack8(o);
    }
}

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(const gcc_adam_tensor_t* __restrict__ tensors,
                                                   const gcc_adam_chunk_t* __restrict__ chunks, int chunk_elems, float lr,
                                                   float b1, float b2, float eps, float bc1, float sqrt_bc2) {
    const gcc_adam_chunk_t ck = chunks[blockIdx.x];
    const gcc_adam_tensor_t t = tensors[ck.tensor];
    const int64_t end = ck.offset + chunk_elems < t.numel ? ck.offset + chunk_elems : t.numel;
    const float step_size = lr / bc1;
    // four elements in flight per thread (16 independent loads): the update is a pure stream of 4 reads + 3 writes
    for (int64_t i0 = ck.offset + threadIdx.x; i0 < end; i0 += 1024) {
        float p[4], g[4], m[4], v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t i = i0 + u * 256;
            if (i < end) { p[u] = t.p[i]; g[u] = t.g[i]; m[u] = t.m[i]; v[u] = t.v[i]; }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t i = i0 + u * 256;
            if (i < end) {
                float gg = g[u] * t.grad_scale;
                if (t.l1 != 0.f) gg += t.l1 * (p[u] > 0.f ? 1.f : (p[u] < 0.f ? -1.f : 0.f));
                const float mn = m[u] + (gg - m[u]) * (1.f - b1);         // lerp_, as torch
                const float vn = v[u] * b2 + (1.f - b2) * gg * gg;
                const float denom = sqrtf(vn) / sqrt_bc2 + eps;
                t.p[i] = p[u] - step_size * (mn / denom); t.m[i] = mn; t.v[i] = vn;
            }
        }
    }
}

// gradient buckets in bf16 for the exchange over xGMI (dist.GradReducer, GCC_DP_BF16=1): four values per thread
__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, size_t n4, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const f32x4 v = ((const f32x4*)src)[i];
        i32x2 o = {(int)pack2bf(v[0], v[1]), (int)pack2bf(v[2], v[3])};
        ((i32x2*)dst)[i] = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[n4 * 4 + threadIdx.x] = f2bf(src[n4 * 4 + threadIdx.x]);
}
__global__ __launch_bounds__(256) void cast_bf16_f32_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, size_t n4, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const i32x2 v = ((const i32x2*)src)[i];
        f32x4 o = {__uint_as_float((uint32_t)v[0] << 16), __uint_as_float((uint32_t)v[0] & 0xffff0000u),
                   __uint_as_float((uint32_t)v[1] << 16), __uint_as_float((uint32_t)v[1] & 0xffff0000u)};
        ((f32x4*)dst)[i] = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[n4 * 4 + threadIdx.x] = bf2f(src[n4 * 4 + threadIdx.x]);
}

__global__ void fill_kernel(float* p, float v, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void add_f32_kernel(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] += src[i];
}
__global__ void clamp_kernel(float* p, float lo, float hi, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        p[i] = fminf(fmaxf(p[i], lo), hi);
}
// out[0] = |a - b| (+ extra terms): the arch-step scalar algebra of models/Pix2Pix.py:484-486, 505-511
__global__ void scalar_ops_kernel(int op, const float* a, const float* b, const float* c, float k0, float k1, float* out) {
    if (threadIdx.x || blockIdx.x) return;
    if (op == 0) out[0] = fabsf(a[0] - b[0]);                               // L1 of two scalars
    else if (op == 1) out[0] = k0 * fabsf(a[0] - b[0]) + k1 * c[0];         // EMA: beta*|a-b| + (1-beta)*prev
    else if (op == 2) out[0] = a[0] + k0 * b[0];
}

constexpr int RED_BLOCKS = 1024;

}  // namespace

// =================================================================================================
extern "C" const char* gcc_strerror(int code) {
    switch (code) {
        case GCC_OK: return "ok";
        case GCC_ERR_BAD_ARG: return "bad argument (null pointer, non-positive size or misaligned ld/offset)";
        case GCC_ERR_UNSUPPORTED: return "geometry not supported by the gfx950 kernels";
        case GCC_ERR_WORKSPACE: return "workspace too small";
        case GCC_ERR_LAUNCH: return "kernel launch failed";
        default: return "unknown error";
    }
}
extern "C" int gcc_version(void) {
    GCC_ENTER(); return GCC_HIP_ABI; }

// ---- route switches (the library's only process-wide state) --------------------------------------------------------
namespace {
struct OptDef { const char* env; int def; };
const OptDef kOptDef[GCC_OPT_COUNT_] = {
    {"GCC_IGEMM_THIN", 1}, {"GCC_FUSE_BN", 3}, {"GCC_BN_BWD_SMALL", 1}, {"GCC_IGEMM_HALO", 3}, {"GCC_INORM_GRID", 1},
    {"GCC_WGRAD_TS", 1}, {"GCC_HALO_XCD_COLS", 1},
};
std::atomic<int> g_opt[GCC_OPT_COUNT_];
int g_opt_default[GCC_OPT_COUNT_];
std::once_flag g_opt_once;
void opt_init() {
    for (int i = 0; i < GCC_OPT_COUNT_; i++) {
        const char* e = getenv(kOptDef[i].env);
        int v = e ? atoi(e) : kOptDef[i].def;
        if (v < 0) v = kOptDef[i].def;
        g_opt_default[i] = v;
        g_opt[i].store(v, std::memory_order_relaxed);
    }
}
}  // namespace
int gcc_opt(int id) {
    std::call_once(g_opt_once, opt_init);
    return g_opt[id].load(std::memory_order_relaxed);
}
// ---- device-side error word ---------------------------------------------------------------------------------------
// A kernel cannot return a code.  The few that wait inside a launch (inorm_grid_kernel's tagged exchange) bound every spin and,
// should one expire, store a code into this word: pinned, mapped host memory the GPU writes directly and the host reads without
// synchronising.  Every entry point of such a kernel returns GCC_ERR_LAUNCH while the word is set (sticky until gcc_device_error(1)).
namespace {
std::once_flag g_err_once;
unsigned* g_err_host = nullptr;
unsigned* g_err_dev = nullptr;
void err_init() {
    void* h = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return; }
    memset(h, 0, 64);
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipGetLastError(); d = h; }
    g_err_host = (unsigned*)h; g_err_dev = (unsigned*)d;
}
}  // namespace
unsigned* gcc_device_error_word() {
    std::call_once(g_err_once, err_init);
    return g_err_dev;
}
extern "C" int gcc_device_error(int clear) {
    std::call_once(g_err_once, err_init);
    if (!g_err_host) return 0;
    const unsigned v = __atomic_load_n(g_err_host, __ATOMIC_RELAXED);
    if (clear) __atomic_store_n(g_err_host, 0u, __ATOMIC_RELAXED);
    return (int)v;
}
namespace { std::atomic<long long> g_launches{0}; }
void gcc_count_launch() { g_launches.fetch_add(1, std::memory_order_relaxed); }
extern "C" long long gcc_launch_count(int reset) {
    return reset ? g_launches.exchange(0, std::memory_order_relaxed) : g_launches.load(std::memory_order_relaxed);
}
extern "C" int gcc_get_option(int id) {
    if (id < 0 || id >= GCC_OPT_COUNT_) return GCC_ERR_BAD_ARG;
    return gcc_opt(id);
}
extern "C" int gcc_set_option(int id, int value) {
    if (id < 0 || id >= GCC_OPT_COUNT_) return GCC_ERR_BAD_ARG;
    std::call_once(g_opt_once, opt_init);
    return g_opt[id].exchange(value < 0 ? g_opt_default[id] : value, std::memory_order_relaxed);
}
// 1 while every route switch holds its built-in default (environment overrides count as changes): what bench.py asserts
extern "C" int gcc_options_default(void) {
    for (int i = 0; i < GCC_OPT_COUNT_; i++)
        if (gcc_opt(i) != kOptDef[i].def) return 0;
    return 1;
}
#ifdef GCC_DIAG_BUILD
namespace { std::atomic<int> g_diag{0}; }
int gcc_diag_bits() { return g_diag.load(std::memory_order_relaxed); }
// diagnostic build only: set the ablation bits (common.hpp), returns the previous ones
extern "C" int gcc_diag_set(int bits) { return g_diag.exchange(bits, std::memory_order_relaxed); }
#endif

extern "C" int gcc_nchw_f32_to_nhwc_bf16(const float* src, void* dst, int N, int C, int H, int W, int ld, int off, int Cfill,
                                         gcc_stream_t stream) {
    GCC_ENTER();
    if (!src || !dst || N <= 0 || C <= 0 || H <= 0 || W <= 0 || off + (Cfill > C ? Cfill : C) > ld) return GCC_ERR_BAD_ARG;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(grid_for((size_t)N * H * W)), dim3(256), 0, (hipStream_t)stream, src,
                       (bf16_t*)dst, N, C, H * W, ld, off, Cfill);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
extern "C" int gcc_nhwc_bf16_to_nchw_f32(const void* src, float* dst, int N, int C, int H, int W, int ld, int off,
                                         gcc_stream_t stream) {
    GCC_ENTER();
    if (!src || !dst || N <= 0 || C <= 0 || H <= 0 || W <= 0 || off + C > ld) return GCC_ERR_BAD_ARG;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_for((size_t)N * H * W)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)src, dst, N, C, H * W, ld, off);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
// which kernel a channel-slice copy (or add: Cfill == C) runs on: 0 the 16-byte vector kernel (everything a multiple of 8), 1 the
// one-group read-modify-write kernel, 2 the scalar kernel; GCC_ERR_BAD_ARG for a window that does not fit its row.  The launch
// below takes its decision from here, so the query cannot say anything else.
extern "C" int gcc_nhwc_copy_route(int lds, int soff, int ldd, int doff, int C, int Cfill) {
    const int Cw = Cfill > C ? Cfill : C;
    if (C <= 0 || soff < 0 || doff < 0 || soff + C > lds || doff + Cw > ldd) return GCC_ERR_BAD_ARG;
    if (!((lds | soff | ldd | doff | C) & 7) && Cfill <= C) return 0;
    if (!((lds | ldd) & 7) && (soff & 7) + C <= 8 && (doff & 7) + Cw <= 8) return 1;
    return 2;
}
static int nhwc_copy_impl(const void* src, int lds, int soff, void* dst, int ldd, int doff, int C, int Cfill, size_t pixels,
                          int add, gcc_stream_t stream) {
    if (!src || !dst || pixels == 0) return GCC_ERR_BAD_ARG;
    const int route = gcc_nhwc_copy_route(lds, soff, ldd, doff, C, Cfill);
    if (route < 0) return route;
    if (route == 0)
        hipLaunchKernelGGL(nhwc_copy_vec_kernel, dim3(grid_for(pixels * (C / 8))), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)src, lds, soff, (bf16_t*)dst, ldd, doff, C / 8, pixels, add);
    else if (route == 1)
        hipLaunchKernelGGL(nhwc_copy_group_kernel, dim3(grid_for(pixels)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)src, lds, soff, (bf16_t*)dst, ldd, doff, C, Cfill, pixels, add);
    else
        hipLaunchKernelGGL(nhwc_copy_scalar_kernel, dim3(grid_for(pixels)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)src, lds, soff, (bf16_t*)dst, ldd, doff, C, Cfill, pixels, add);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
extern "C" int gcc_nhwc_copy(const void* src, int lds, int soff, void* dst, int ldd, int doff, int C, int Cfill, size_t pixels,
                             gcc_stream_t stream) {
    GCC_ENTER();
    return nhwc_copy_impl(src, lds, soff, dst, ldd, doff, C, Cfill, pixels, 0, stream);
}
// dst[.., doff + 0..Ca) = a[.., aoff + 0..Ca), dst[.., doff + Ca .. Ca + Cb) = b[.., boff + 0..Cb), zeros up to the 8-wide group:
// the (image, image) discriminator input, 3 + 3 channels, as ONE 16-byte store per pixel instead of two passes of
// 2-byte accesses (17 us each at 16 x 256 x 256).
__global__ __launch_bounds__(256) void nhwc_pack_pair_kernel(const bf16_t* __restrict__ a, int lda, int aoff, const bf16_t* __restrict__ b,
                                                             int ldb, int boff, bf16_t* __restrict__ dst, int ldd, int doff, int Ca,
                                                             int Cb, size_t pixels) {
    for (size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x; pix < pixels; pix += (size_t)gridDim.x * 256) {
        const i32x4 va = *(const i32x4*)(a + pix * lda + aoff);
        const i32x4 vb = *(const i32x4*)(b + pix * ldb + boff);
        bf16_t ea[8], eb[8], o[8];
        *(i32x4*)ea = va; *(i32x4*)eb = vb;
#pragma unroll
        for (int c = 0; c < 8; c++) o[c] = c < Ca ? ea[c] : (c - Ca < Cb ? eb[c - Ca < 0 ? 0 : c - Ca] : (bf16_t)0);
        *(i32x4*)(dst + pix * ldd + doff) = *(const i32x4*)o;
    }
}
extern "C" int gcc_nhwc_pack_pair(const void* a, int lda, int aoff, const void* b, int ldb, int boff, void* dst, int ldd, int doff,
                                  int Ca, int Cb, size_t pixels, gcc_stream_t stream) {
    GCC_ENTER();
    if (!a || !b || !dst || Ca <= 0 || Cb <= 0 || Ca + Cb > 8 || pixels == 0) return GCC_ERR_BAD_ARG;
    if ((lda & 7) || (ldb & 7) || (ldd & 7) || (aoff & 7) || (boff & 7) || (doff & 7)) return GCC_ERR_BAD_ARG;
    hipLaunchKernelGGL(nhwc_pack_pair_kernel, dim3(grid_for(pixels)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)a, lda, aoff,
                       (const bf16_t*)b, ldb, boff, (bf16_t*)dst, ldd, doff, Ca, Cb, pixels);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_nhwc_add(const void* src, int lds, int soff, void* dst, int ldd, int doff, int C, size_t pixels,
                            gcc_stream_t stream) {
    GCC_ENTER();
    return nhwc_copy_impl(src, lds, soff, dst, ldd, doff, C, C, pixels, 1, stream);
}

extern "C" int gcc_pack_weights(const float* master, int rows, int taps, int cols, void* w, void* wt, gcc_stream_t stream) {
    GCC_ENTER();
    if (!master || rows <= 0 || taps <= 0 || cols <= 0 || (!w && !wt)) return GCC_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (w) {
        const int colsp = ceil8(cols);
        hipLaunchKernelGGL(pack_w_kernel, dim3(grid_for((size_t)rows * taps * colsp)), dim3(256), 0, st, master, rows, taps,
                           cols, colsp, (bf16_t*)w);
        GCC_CHECK_LAUNCH();
    }
    if (wt) {
        const int rowsp = ceil8(rows);
        hipLaunchKernelGGL(pack_wt_kernel, dim3(cdiv(cols, 32), cdiv(rowsp, 32), taps), dim3(256), 0, st, master, rows, taps,
                           cols, rowsp, (bf16_t*)wt);
        GCC_CHECK_LAUNCH();
    }
    return GCC_OK;
}

extern "C" int gcc_pack_weights_multi(const gcc_pack_desc_t* descs, const gcc_pack_item_t* items, int nitems,
                                      gcc_stream_t stream) {
    GCC_ENTER();
    if (!descs || !items || nitems <= 0) return GCC_ERR_BAD_ARG;
    hipLaunchKernelGGL(pack_multi_kernel, dim3(nitems), dim3(256), 0, (hipStream_t)stream, descs, items);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" size_t gcc_loss_workspace(size_t pixels, int C) {
    (void)pixels; (void)C;
    return RED_BLOCKS * sizeof(float);
}

extern "C" int gcc_gan_loss(int mode, int target_is_real, int for_discriminator, const void* pred, int ld, int off,
                            size_t pixels, float weight, float* loss, int accumulate, void* dpred, void* ws, size_t ws_bytes,
                            gcc_stream_t stream) {
    GCC_ENTER();
    (void)ws; (void)ws_bytes;
    if (!pred || !loss || pixels == 0 || (ld & 7) || (off & 7) || mode < 0 || mode > 3) return GCC_ERR_BAD_ARG;
    if (mode == 0 && !for_discriminator && !target_is_real) return GCC_ERR_BAD_ARG;   // reference asserts
    hipLaunchKernelGGL(gan_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, mode, target_is_real, for_discriminator,
                       (const bf16_t*)pred, ld, off, pixels, weight, loss, accumulate, (bf16_t*)dpred, weight, (const float*)nullptr, 0);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_gan_loss_ex(int mode, int target_is_real, int for_discriminator, const void* pred, int ld, int off,
                               size_t pixels, float* loss, void* dpred, float grad_weight, const float* grad_weight_dev,
                               int dpred_accumulate, gcc_stream_t stream) {
    GCC_ENTER();
    if (!pred || !loss || pixels == 0 || (ld & 7) || (off & 7) || mode < 0 || mode > 3) return GCC_ERR_BAD_ARG;
    if (mode == 0 && !for_discriminator && !target_is_real) return GCC_ERR_BAD_ARG;
    hipLaunchKernelGGL(gan_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, mode, target_is_real, for_discriminator,
                       (const bf16_t*)pred, ld, off, pixels, 1.f, loss, 0, (bf16_t*)dpred, grad_weight, grad_weight_dev,
                       dpred_accumulate);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

// arch step scalars (models/Pix2Pix.py:479-487): dS = |Lfr - Lf| ;
// loss = |dS - dT| + w (Lr + Lf) ; c_fr = dloss/dLfr ; c_f = dloss/dLf   (dloss/dLr = w)
// w = 1/2 for Pix2Pix / CycleGAN, 1 for SAGAN (models/SAGAN.py:388-389)
__global__ void arch_coeffs_kernel(const float* Lfr, const float* Lf, const float* Lr, const float* dT, float w, float* loss,
                                   float* c_fr, float* c_f) {
    if (threadIdx.x || blockIdx.x) return;
    const float a = Lfr[0] - Lf[0];
    const float dS = fabsf(a);
    const float s1 = a > 0.f ? 1.f : (a < 0.f ? -1.f : 0.f);
    const float b = dS - dT[0];
    const float s2 = b > 0.f ? 1.f : (b < 0.f ? -1.f : 0.f);
    loss[0] = fabsf(b) + w * (Lr[0] + Lf[0]);
    c_fr[0] = s2 * s1;
    c_f[0] = -s2 * s1 + w;
}
extern "C" int gcc_arch_coeffs(const float* Lfr, const float* Lf, const float* Lr, const float* dT, float real_fake_weight,
                               float* loss, float* c_fr, float* c_f, gcc_stream_t stream) {
    GCC_ENTER();
    if (!Lfr || !Lf || !Lr || !dT || !loss || !c_fr || !c_f) return GCC_ERR_BAD_ARG;
    hipLaunchKernelGGL(arch_coeffs_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, Lfr, Lf, Lr, dT, real_fake_weight, loss,
                       c_fr, c_f);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_l1_loss(const void* a, int lda, int aoff, const void* b, int ldb, int boff, int C, size_t pixels,
                           float weight, float* loss, int accumulate, void* da, int ldda, int daoff, void* ws,
                           size_t ws_bytes, gcc_stream_t stream) {
    GCC_ENTER();
    if (!a || !b || !loss || !ws || C <= 0 || pixels == 0) return GCC_ERR_BAD_ARG;
    if ((lda | aoff | ldb | boff) & 7 || (da && ((ldda | daoff) & 7))) return GCC_ERR_BAD_ARG;
    if (ws_bytes < RED_BLOCKS * sizeof(float)) return GCC_ERR_WORKSPACE;
    DiffArgs g;
    g.a = (const bf16_t*)a; g.lda = lda; g.aoff = aoff; g.b = (const bf16_t*)b; g.ldb = ldb; g.boff = boff;
    g.C = C; g.CH = (C + 7) / 8; g.pixels = pixels; g.partial = (float*)ws;
    g.da = (bf16_t*)da; g.ldda = ldda; g.daoff = daoff;
    const double count = (double)pixels * C;
    g.gscale = (float)(weight / count); g.mode = 0;
    const int blocks = grid_for(pixels * g.CH, 256 * 4, RED_BLOCKS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(diff_reduce_kernel, dim3(blocks), dim3(256), 0, st, g);
    GCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(scalar_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, blocks, count, weight, loss,
                       accumulate, 0);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

// nn.MSELoss: weight * mean((a-b)^2) ; da = weight * 2 (a-b) / count
extern "C" int gcc_mse_loss(const void* a, int lda, int aoff, const void* b, int ldb, int boff, int C, size_t pixels,
                           float weight, float* loss, int accumulate, void* da, int ldda, int daoff, void* ws,
                           size_t ws_bytes, gcc_stream_t stream) {
    GCC_ENTER();
    if (!a || !b || !loss || !ws || C <= 0 || pixels == 0) return GCC_ERR_BAD_ARG;
    if ((lda | aoff | ldb | boff) & 7 || (da && ((ldda | daoff) & 7))) return GCC_ERR_BAD_ARG;
    if (ws_bytes < RED_BLOCKS * sizeof(float)) return GCC_ERR_WORKSPACE;
    DiffArgs g;
    g.a = (const bf16_t*)a; g.lda = lda; g.aoff = aoff; g.b = (const bf16_t*)b; g.ldb = ldb; g.boff = boff;
    g.C = C; g.CH = (C + 7) / 8; g.pixels = pixels; g.partial = (float*)ws;
    g.da = (bf16_t*)da; g.ldda = ldda; g.daoff = daoff;
    const double count = (double)pixels * C;
    g.gscale = (float)(2.0 * weight / count); g.mode = 2;
    const int blocks = grid_for(pixels * g.CH, 256 * 4, RED_BLOCKS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(diff_reduce_kernel, dim3(blocks), dim3(256), 0, st, g);
    GCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(scalar_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, blocks, count, weight, loss,
                       accumulate, 0);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

// workspace layout of one feature pair:
//   [0]   scal[4]  (Lg, Lc, -, -)            fp32
//   [64]  partial[2][RED_BLOCKS]             fp32
//   Gf [N][C][C] fp32 | Gt [N][C][C] fp32 | S [N][C][C] bf16 | dfg [N][HW][C] bf16 | wgrad slabs
static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
struct DistillWs { size_t scal, partial, gf, gt, s, dfg, slabs, total; };
// the two products as convolutions of one image [1][HW] pixels, N problems: G = F^T F is the 1x1 weight gradient with x = dy = the
// feature window; dfg = f . S the 1x1 forward with S as its weight and the dense dfg as its output
static gcc_conv_t distill_gram_conv(int C, int HW, int ld, int off) {
    gcc_conv_t c = {1, 1, HW, C, C, 1, 1, 1, 0, ld, off, ld, off};
    return c;
}
static gcc_conv_t distill_bwd_conv(int C, int HW, int ldf, int foff) {
    gcc_conv_t c = {1, 1, HW, C, C, 1, 1, 1, 0, ldf, foff, C, 0};
    return c;
}
static DistillWs distill_layout(int N, int C, int HW) {
    DistillWs w;
    const gcc_conv_t c = distill_gram_conv(C, HW, C, 0);
    size_t o = 0;
    w.scal = o; o = al256(o + 16 * sizeof(float));
    w.partial = o; o = al256(o + 2 * RED_BLOCKS * sizeof(float));
    w.gf = o; o = al256(o + (size_t)N * C * C * 4);
    w.gt = o; o = al256(o + (size_t)N * C * C * 4);
    w.s = o; o = al256(o + (size_t)N * C * C * 2);
    w.dfg = o; o = al256(o + (size_t)N * HW * C * 2);
    w.slabs = o; o = al256(o + gcc_internal_wgrad_workspace(&c, N));
    w.total = o;
    return w;
}

extern "C" size_t gcc_distill_workspace(int N, int C, int HW) {
    if (N <= 0 || C <= 0 || HW <= 0 || (C & 7)) return 0;
    return distill_layout(N, C, HW).total;
}

// kernel launches of gcc_distill_fwd behind the two Gram products: gram_diff + finalize, diff_reduce + finalize (the copy of the
// two scalars is a memcpy node); of gcc_distill_bwd behind the 1x1 product: distill_combine_kernel
constexpr int DISTILL_FWD_TAIL_LAUNCHES = 4, DISTILL_BWD_TAIL_LAUNCHES = 1;

extern "C" int gcc_distill_plan(int N, int C, int HW, long long* plan) {
    if (!plan || N <= 0 || C <= 0 || HW <= 0 || (C & 7)) return GCC_ERR_BAD_ARG;
    const DistillWs L = distill_layout(N, C, HW);
    plan[GCC_DISTILL_PLAN_OFF_SCAL] = (long long)L.scal; plan[GCC_DISTILL_PLAN_OFF_GF] = (long long)L.gf;
    plan[GCC_DISTILL_PLAN_OFF_GT] = (long long)L.gt; plan[GCC_DISTILL_PLAN_OFF_S] = (long long)L.s;
    plan[GCC_DISTILL_PLAN_OFF_DFG] = (long long)L.dfg; plan[GCC_DISTILL_PLAN_WS_BYTES] = (long long)L.total;
    const gcc_conv_t cg = distill_gram_conv(C, HW, C, 0), cb = distill_bwd_conv(C, HW, C, 0);
    int w[6], g[6];
    int rc = gcc_internal_wgrad_plan(&cg, N, w);
    if (rc) return rc;
    rc = gcc_internal_igemm_plan(&cb, 0, N, g);
    if (rc) return rc;
    plan[GCC_DISTILL_PLAN_GRAM_SPLITS] = w[0]; plan[GCC_DISTILL_PLAN_GRAM_KPER] = w[1];
    plan[GCC_DISTILL_PLAN_GRAM_COL_TILES] = w[2]; plan[GCC_DISTILL_PLAN_GRAM_CO_TILES] = w[3];
    plan[GCC_DISTILL_PLAN_GRAM_FOLD] = w[4];
    plan[GCC_DISTILL_PLAN_BWD_ROUTE] = g[0]; plan[GCC_DISTILL_PLAN_BWD_BP] = g[1]; plan[GCC_DISTILL_PLAN_BWD_BC] = g[2];
    plan[GCC_DISTILL_PLAN_BWD_NTILES] = g[3]; plan[GCC_DISTILL_PLAN_BWD_MTILES] = g[4];
    plan[GCC_DISTILL_PLAN_FWD_LAUNCHES] = 2 * w[5] + DISTILL_FWD_TAIL_LAUNCHES;
    plan[GCC_DISTILL_PLAN_BWD_LAUNCHES] = g[5] + DISTILL_BWD_TAIL_LAUNCHES;
    return GCC_OK;
}

extern "C" int gcc_distill_fwd(const void* f, int ldf, int foff, const void* t, int ldt, int toff, int N, int C, int HW,
                               int squared, float* out2, void* ws, size_t ws_bytes, gcc_stream_t stream) {
    GCC_ENTER();
    if (!f || !t || !out2 || !ws || N <= 0 || C <= 0 || HW <= 0 || (C & 7)) return GCC_ERR_BAD_ARG;
    if ((ldf | foff | ldt | toff) & 7) return GCC_ERR_BAD_ARG;
    const DistillWs L = distill_layout(N, C, HW);
    if (ws_bytes < L.total) return GCC_ERR_WORKSPACE;
    char* base = (char*)ws;
    hipStream_t st = (hipStream_t)stream;
    float* scal = (float*)(base + L.scal);
    float* partial = (float*)(base + L.partial);
    // raw gram matrices: per image, G = F^T F over the HW pixels  (a 1x1 weight-gradient product)
    const gcc_conv_t cf = distill_gram_conv(C, HW, ldf, foff), ct = distill_gram_conv(C, HW, ldt, toff);
    const size_t slab_bytes = L.total - L.slabs;
    int rc = gcc_internal_wgrad(&cf, f, f, (float*)(base + L.gf), 0, base + L.slabs, slab_bytes, N, (long)HW * ldf,
                                (long)HW * ldf, st, 0, 0, 0, 0);
    if (rc) return rc;
    rc = gcc_internal_wgrad(&ct, t, t, (float*)(base + L.gt), 0, base + L.slabs, slab_bytes, N, (long)HW * ldt, (long)HW * ldt, st, 0, 0, 0, 0);
    if (rc) return rc;
    const size_t ng = (size_t)N * C * C;
    const int b1 = grid_for(ng, 256 * 4, RED_BLOCKS);
    hipLaunchKernelGGL(gram_diff_kernel, dim3(b1), dim3(256), 0, st, (const float*)(base + L.gf), (const float*)(base + L.gt),
                       ng, 1.f / ((float)C * (float)HW), (bf16_t*)(base + L.s), partial);
    GCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(scalar_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, b1, (double)ng, 1.f,
                       scal + 0, 0, squared ? 2 : 1);
    GCC_CHECK_LAUNCH();
    DiffArgs g;
    g.a = (const bf16_t*)f; g.lda = ldf; g.aoff = foff; g.b = (const bf16_t*)t; g.ldb = ldt; g.boff = toff;
    g.C = C; g.CH = C / 8; g.pixels = (size_t)N * HW; g.partial = partial + RED_BLOCKS;
    g.da = nullptr; g.ldda = 0; g.daoff = 0; g.gscale = 0.f; g.mode = 1;
    const int b2 = grid_for(g.pixels * g.CH, 256 * 4, RED_BLOCKS);
    hipLaunchKernelGGL(diff_reduce_kernel, dim3(b2), dim3(256), 0, st, g);
    GCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(scalar_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)(partial + RED_BLOCKS), b2,
                       (double)N * HW * C, 1.f, scal + 1, 0, squared ? 2 : 1);
    GCC_CHECK_LAUNCH();
    if (gcc_memcpy_d2d_async(out2, scal, 2 * sizeof(float), st) != hipSuccess) return GCC_ERR_LAUNCH;
    return GCC_OK;
}

extern "C" int gcc_distill_bwd(const void* f, int ldf, int foff, const void* t, int ldt, int toff, int N, int C, int HW,
                               int squared, float wg, float wc, void* df, int lddf, int dfoff, void* ws, size_t ws_bytes,
                               gcc_stream_t stream) {
    GCC_ENTER();
    if (!f || !t || !df || !ws || N <= 0 || C <= 0 || HW <= 0 || (C & 7)) return GCC_ERR_BAD_ARG;
    if ((ldf | foff | ldt | toff | lddf | dfoff) & 7) return GCC_ERR_BAD_ARG;
    const DistillWs L = distill_layout(N, C, HW);
    if (ws_bytes < L.total) return GCC_ERR_WORKSPACE;
    char* base = (char*)ws;
    hipStream_t st = (hipStream_t)stream;
    // dfg[pix][c] = sum_c' f[pix][c'] * D[c'][c]   (D symmetric): per-image 1x1 product
    const gcc_conv_t c1 = distill_bwd_conv(C, HW, ldf, foff);
    int rc = gcc_internal_igemm(&c1, 0, f, base + L.s, base + L.dfg, nullptr, N, (long)HW * ldf, (long)C * C, (long)HW * C, st);
    if (rc) return rc;
    const double kg0 = (double)wg * 2.0 / ((double)N * C * C * (double)C * HW);
    const double kc0 = (double)wc / ((double)N * C * HW);
    const size_t pixels = (size_t)N * HW;
    hipLaunchKernelGGL(distill_combine_kernel, dim3(grid_for(pixels * (C / 8), 256 * 2, 4096)), dim3(256), 0, st,
                       (const bf16_t*)f, ldf, foff, (const bf16_t*)t, ldt, toff, (const bf16_t*)(base + L.dfg), C / 8, pixels,
                       (const float*)(base + L.scal), (float)kg0, (float)kc0, squared, (bf16_t*)df, lddf, dfoff);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

// ---- image history of the CycleGAN discriminators (utils/image_pool.py:5-54) on the device ---------------------------------
// The reference draws, per image, whether the discriminator sees the new fake or an older one from a 50-image history that the
// new one then replaces.  The draws stay on the host (Python's `random`, the reference's order); what they decided travels as
// two ints per image -- mode (0 pass through, 1 store and pass through, 2 swap with slot) and slot -- written by a launch that
// takes them BY VALUE (gcc_write_i32: a recording patches that one argument per iteration), and one kernel moves the pixels.
struct I32x16 { int v[16]; };
__global__ void write_i32_kernel(int* dst, I32x16 vals, int n) {
    if (threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x];
}
extern "C" int gcc_write_i32(int* dst, const int* values, int n, gcc_stream_t stream) {
    GCC_ENTER();
    if (!dst || !values || n < 1 || n > 16) return GCC_ERR_BAD_ARG;
    I32x16 v = {};
    for (int i = 0; i < n; i++) v.v[i] = values[i];
    hipLaunchKernelGGL(write_i32_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, dst, v, n);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
// one thread owns a pixel of EVERY image of the batch and walks the images in order: two images of a batch that draw the same
// slot behave as in the reference's sequential loop (the second one receives the first one's pixels)
__global__ __launch_bounds__(256) void image_pool_kernel(const i32x4* __restrict__ src, i32x4* __restrict__ out, i32x4* pool,
                                                         const int* __restrict__ sel, int N, size_t hw) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (size_t)gridDim.x * 256) {
        for (int n = 0; n < N; n++) {
            const int mode = sel[2 * n], slot = sel[2 * n + 1];
            const i32x4 v = src[n * hw + i];
            i32x4* p = pool + (size_t)slot * hw + i;
            if (mode == 0) { out[n * hw + i] = v; }
            else if (mode == 1) { *p = v; out[n * hw + i] = v; }
            else { const i32x4 old = *p; *p = v; out[n * hw + i] = old; }
        }
    }
}
// images / out: [N][HW][8] bf16 (3 channels in one 16-byte group), pool: [slots][HW][8], sel: device [N][2] = (mode, slot)
extern "C" int gcc_image_pool_query(const void* images, void* out, void* pool, const int* sel, int N, size_t HW, int slots,
                                    gcc_stream_t stream) {
    GCC_ENTER();
    if (!images || !out || !pool || !sel || N < 1 || HW == 0 || slots < 1) return GCC_ERR_BAD_ARG;
    const int bx = (int)std::min<size_t>((HW + 255) / 256, 512);
    hipLaunchKernelGGL(image_pool_kernel, dim3(bx), dim3(256), 0, (hipStream_t)stream, (const i32x4*)images, (i32x4*)out,
                       (i32x4*)pool, sel, N, HW);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_adam_factors(float beta1, float beta2, int step, float* out2) {
    if (!out2 || step < 1) return GCC_ERR_BAD_ARG;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    out2[0] = (float)bc1; out2[1] = (float)sqrt(bc2);
    return GCC_OK;
}

extern "C" int gcc_adam_step(const gcc_adam_tensor_t* tensors, const gcc_adam_chunk_t* chunks, int nchunks, int chunk_elems,
                             float lr, float beta1, float beta2, float eps, int step, gcc_stream_t stream) {
    GCC_ENTER();
    if (!tensors || !chunks || nchunks <= 0 || chunk_elems <= 0 || step < 1) return GCC_ERR_BAD_ARG;
    float f[2];
    gcc_adam_factors(beta1, beta2, step, f);
    hipLaunchKernelGGL(adam_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, chunk_elems, lr, beta1,
                       beta2, eps, f[0], f[1]);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_fill_f32(float* p, float v, size_t n, gcc_stream_t stream) {
    GCC_ENTER();
    if (!p || n == 0) return GCC_ERR_BAD_ARG;
    hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, v, n);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
extern "C" int gcc_add_f32(float* dst, const float* src, size_t n, gcc_stream_t stream) {
    GCC_ENTER();
    if (!dst || !src || n == 0) return GCC_ERR_BAD_ARG;
    hipLaunchKernelGGL(add_f32_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dst, src, n);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
extern "C" int gcc_cast_f32_bf16(const float* src, void* dst, size_t n, gcc_stream_t stream) {
    GCC_ENTER();
    if (!src || !dst || n == 0 || (((uintptr_t)src) & 15) || (((uintptr_t)dst) & 7)) return GCC_ERR_BAD_ARG;
    hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid_for(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, n / 4, n);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
extern "C" int gcc_cast_bf16_f32(const void* src, float* dst, size_t n, gcc_stream_t stream) {
    GCC_ENTER();
    if (!src || !dst || n == 0 || (((uintptr_t)dst) & 15) || (((uintptr_t)src) & 7)) return GCC_ERR_BAD_ARG;
    hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3(grid_for(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, dst, n / 4, n);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
extern "C" int gcc_clamp_f32(float* p, float lo, float hi, size_t n, gcc_stream_t stream) {
    GCC_ENTER();
    if (!p || n == 0) return GCC_ERR_BAD_ARG;
    hipLaunchKernelGGL(clamp_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, lo, hi, n);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
extern "C" int gcc_scalar_op(int op, const float* a, const float* b, const float* c, float k0, float k1, float* out,
                             gcc_stream_t stream) {
    GCC_ENTER();
    if (!a || !b || !out || op < 0 || op > 2 || (op == 1 && !c)) return GCC_ERR_BAD_ARG;   // op 1 alone reads c
    hipLaunchKernelGGL(scalar_ops_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, op, a, b, c, k0, k1, out);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
