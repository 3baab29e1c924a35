// Evaluation arithmetic of the reference on device tensors; the networks that produce the
// activations / score maps (Inception, DRN) stay external inputs.
//   mIoU   metric/mIoU_score.py:108-109, 163-167, 213   argmax over classes, fast_hist (bincount of n * label + pred)
//   PSNR   models/SRGAN.py:653-657, data/sr_dataset.py:36-37, 58-62   luminance of [-1, 1] images, 4-pixel border cropped
//   FID    metric/fid_score.py:219-284, 327-328   mu = mean, sigma = np.cov(act, rowvar=False),
//          d^2 = |mu1 - mu2|^2 + tr(s1) + tr(s2) - 2 tr(sqrtm(s1 s2))
// Integer results are exact; the f64 results are reductions in a fixed order (no atomics on floating point).
// sqrtm: scipy's Schur method is replaced by the coupled Newton-Schulz iteration on B = s1 s2 + delta I (real
// non-negative spectrum, shifted off zero):
//     Y0 = B / |B|_F, Z0 = I ;  T = (3 I - Z Y) / 2 ;  Y <- Y T ;  Z <- T Z ;  Y -> sqrtm(B / |B|_F)
// three f64 GEMMs per iteration, all on the GPU; only tr(Y) is needed.  Covariances of fewer samples than dimensions
// (500 validation images against 2048 Inception features) make s1 s2 singular, where Z -> B^(-1/2) would diverge: the
// shift delta = shift_rel |A|_F bounds it, and a second solve at 4 delta cancels the k sqrt(delta) the k zero
// eigenvalues add to the trace (Richardson extrapolation in sqrt(delta)); measured 1e-8 relative against scipy on
// full-rank and rank-deficient inputs alike.  The GEMM is an LDS-tiled FMA kernel
// (64 x 64 x 16, 4 x 4 per thread): bound by the f64 vector rate (78 TFLOP/s peak), a once-per-epoch computation.
#include "common.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ s, int C, size_t HW, size_t total, int* __restrict__ pred) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t n = i / HW, p = i - n * HW;
        const float* b = s + n * C * HW + p;
        float best = b[0];
        int bi = 0;
        for (int c = 1; c < C; c++) {
            const float v = b[(size_t)c * HW];
            // numpy.argmax: first maximum; a NaN counts as the maximum (first NaN wins)
            if (best == best && (v > best || v != v)) { best = v; bi = c; }
        }
        pred[i] = bi;
    }
}

__global__ __launch_bounds__(256) void hist_kernel(const int* __restrict__ pred, const int* __restrict__ label, size_t count, int n,
                                                   unsigned long long* hist) {
    extern __shared__ unsigned int sh[];
    const int nn = n * n;
    for (int i = threadIdx.x; i < nn; i += 256) sh[i] = 0u;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const int l = label[i];
        if (l >= 0 && l < n) {
            const int p = pred[i];
            if (p >= 0 && p < n) atomicAdd(&sh[n * l + p], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nn; i += 256)
        if (sh[i]) atomicAdd(&hist[i], (unsigned long long)sh[i]);
}

// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) s += sh[i];
    return s;
}

__device__ __forceinline__ float luma(const float* img, size_t plane, size_t o) {
    // convert_image('[-1, 1]' -> 'y-channel'), the reference's operation order in fp32.  The dot product is spelled as the fused
    // chain a matmul row makes of it (r, then g, then b): left as `r * 65.481f + g * 128.553f + b * 24.966f` the compiler chose the
    // contraction per call site, and the two images of one launch went through different roundings (fused g into r * c for one,
    // r into g * c for the other: psnr(x, x) had a sum that was not zero)
    const float r = 255.f * ((img[o] + 1.f) / 2.f), g = 255.f * ((img[plane + o] + 1.f) / 2.f),
                b = 255.f * ((img[2 * plane + o] + 1.f) / 2.f);
    return __fmaf_rn(b, 24.966f, __fmaf_rn(g, 128.553f, r * 65.481f)) / 255.f + 16.f;
}

__global__ __launch_bounds__(256) void psnr_sse_kernel(const float* __restrict__ fake, const float* __restrict__ real, int N, int H,
                                                       int W, double* partial) {
    __shared__ double sh[4];
    const int h = H - 8, w = W - 8;
    const size_t per = (size_t)h * w, total = per * N, plane = (size_t)H * W;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t n = i / per, r = i - n * per;
        const size_t y = r / w + 4, x = r % w + 4;
        const size_t o = y * W + x;
        const double d = (double)luma(fake + n * 3 * plane, plane, o) - (double)luma(real + n * 3 * plane, plane, o);
        acc += d * d;
    }
    const double s = block_sum_f64(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// SSIM on the luminance channel (skimage.metrics.structural_similarity defaults: 7 x 7 uniform window, K1 = .01, K2 = .03,
// sample covariance NP / (NP - 1), mean of S over the window centres that keep the whole window inside the image), on the
// 4-pixel-cropped y-channel image of models/SRGAN.py:653-661.  One thread per window centre, 49 taps in f64.
__global__ __launch_bounds__(256) void ssim_y_kernel(const float* __restrict__ fake, const float* __restrict__ real, int N, int H,
                                                     int W, double data_range, double* partial) {
    __shared__ double sh[4];
    const int h = H - 8, w = W - 8, hv = h - 6, wv = w - 6;       // y image, valid window centres
    const size_t per = (size_t)hv * wv, total = per * N, plane = (size_t)H * W;
    const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t n = i / per, r = i - n * per;
        const size_t y0 = r / wv + 4, x0 = r % wv + 4;                // top-left tap in the uncropped image
        const float* f = fake + n * 3 * plane;
        const float* g = real + n * 3 * plane;
        double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
        for (int dy = 0; dy < 7; dy++)
            for (int dx = 0; dx < 7; dx++) {
                const size_t o = (y0 + dy) * W + x0 + dx;
                const double a = (double)luma(g, plane, o), b = (double)luma(f, plane, o);   // X = real, Y = fake (:660)
                sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
            }
        const double ux = sx / 49.0, uy = sy / 49.0, cn = 49.0 / 48.0;
        const double vx = cn * (sxx / 49.0 - ux * ux), vy = cn * (syy / 49.0 - uy * uy), vxy = cn * (sxy / 49.0 - ux * uy);
        acc += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
    }
    const double s = block_sum_f64(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void sum_partials_kernel(const double* partial, int n, double scale, double* out, int accumulate) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    const double s = block_sum_f64(acc, sh) * scale;
    if (threadIdx.x == 0) out[0] = accumulate ? out[0] + s : s;
}

// ---------------------------------------------------------------------------------------------
// column means of act [n][d] (fp32 or f64) in f64: one thread per column chunk, rows split over blockIdx.y, fixed order
__global__ __launch_bounds__(256) void colsum_kernel(const void* act, int is_f64, int n, int d, int rows_per, double* partial) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    const int r0 = blockIdx.y * rows_per, r1 = min(n, r0 + rows_per);
    double acc = 0.0;
    if (is_f64) { const double* a = (const double*)act; for (int i = r0; i < r1; i++) acc += a[(size_t)i * d + j]; }
    else { const float* a = (const float*)act; for (int i = r0; i < r1; i++) acc += (double)a[(size_t)i * d + j]; }
    partial[(size_t)blockIdx.y * d + j] = acc;
}
__global__ __launch_bounds__(256) void mean_finalize_kernel(const double* partial, int slices, int n, int d, double* mu) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    double acc = 0.0;
    for (int s = 0; s < slices; s++) acc += partial[(size_t)s * d + j];
    mu[j] = acc / (double)n;
}
__global__ __launch_bounds__(256) void center_kernel(const void* act, int is_f64, size_t total, int d, const double* mu, double* xc) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const double v = is_f64 ? ((const double*)act)[i] : (double)((const float*)act)[i];
        xc[i] = v - mu[i % d];
    }
}

// Streamed statistics (gcc_activation_stats_update): a batch [b][d] (row stride ld) merged into running centred moments
// (Chan et al.).  One launch per batch for everything but the rank-b product: a workgroup owns 64 columns, its four waves sum
// interleaved rows (combined in wave order: a fixed order), then write the batch centred on its OWN mean (xc: the GEMM's
// operand), delta = batch mean - running mean (the GEMM's rank-1 term) and the merged mean.  first != 0 (nothing merged yet):
// mean is written, never read, and delta is 0.
__global__ __launch_bounds__(256) void stream_center_kernel(const void* act, int is_f64, int ld, int b, int d, int first,
                                                            double w /* b / (n_before + b) */, double* mean, double* delta,
                                                            double* xc) {
    __shared__ double part[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, j = blockIdx.x * 64 + tx;
    const bool live = j < d;
    double acc = 0.0;
    if (live) {
        if (is_f64) { const double* a = (const double*)act; for (int i = ty; i < b; i += 4) acc += a[(size_t)i * ld + j]; }
        else { const float* a = (const float*)act; for (int i = ty; i < b; i += 4) acc += (double)a[(size_t)i * ld + j]; }
    }
    part[ty][tx] = acc;
    __syncthreads();
    if (!live) return;
    const double mb = (((part[0][tx] + part[1][tx]) + part[2][tx]) + part[3][tx]) / (double)b;
    for (int i = ty; i < b; i += 4) {
        const double v = is_f64 ? ((const double*)act)[(size_t)i * ld + j] : (double)((const float*)act)[(size_t)i * ld + j];
        xc[(size_t)i * d + j] = v - mb;
    }
    if (ty == 0) {
        if (first) { delta[j] = 0.0; mean[j] = mb; }
        else {
            const double m = mean[j], dl = mb - m;
            delta[j] = dl;
            mean[j] = m + dl * w;
        }
    }
}
__global__ __launch_bounds__(256) void scale_kernel(const double* x, double s, size_t n, double* y) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] = x[i] * s;
}
// generated / real images as the FID network's input, the fp32 form: util.tensor2imgs' byte of an NCHW fp32 image in [-1, 1]
// ((x + 1) / 2 * 255 in fp32, clipped, truncated) over 255.  The layout does not change: plain elements, four per lane where the
// pointers allow it.  float(b) / 255.f is the fp32 rounding of the reference's double quotient for every byte.
__device__ __forceinline__ float fid_unit(float x) {
#pragma clang fp contract(off)
    float t = __fmul_rn(__fmul_rn(__fadd_rn(x, 1.f), 0.5f), 255.f);
    t = t > 0.f ? (t < 255.f ? t : 255.f) : 0.f;
    return (float)(unsigned char)t / 255.f;
}
__global__ __launch_bounds__(256) void fid_input_f32_kernel(const float* __restrict__ x, size_t nvec, size_t total,
                                                            float* __restrict__ out) {
    const size_t items = nvec + (total - 4 * nvec);             // float4 groups, then the scalar tail
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        if (i < nvec) {
            const float4 v = ((const float4*)x)[i];
            ((float4*)out)[i] = make_float4(fid_unit(v.x), fid_unit(v.y), fid_unit(v.z), fid_unit(v.w));
        } else {
            const size_t e = 4 * nvec + (i - nvec);
            out[e] = fid_unit(x[e]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// C[M][N] = alpha * (*alpha_dev) * sum_k a(i,k) b(k,j) + diag * [i == j];  a(i,k) = A[i*sai + k*sak], b(k,j) = B[k*sbk + j*sbj]
struct GemmArgs {
    const double* A; long sai, sak;
    const double* B; long sbk, sbj;
    double* C; int M, N, K;
    double alpha, diag;
    const double* alpha_dev;     // optional device scalar; inv != 0: multiply by 1 / (*alpha_dev)
    int inv;
    // MERGE only (the streamed statistics' update): C = beta * C + (the above) + r1c * r1[i] * r1[j]; beta == 0 never reads C
    double beta, r1c;
    const double* r1;
};
template <bool MERGE>
__global__ __launch_bounds__(256) void dgemm_kernel(const GemmArgs g) {
    __shared__ double As[16][65], Bs[16][65];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[r][c] = 0.0;
    for (int k0 = 0; k0 < g.K; k0 += 16) {
#pragma unroll
        for (int e0 = 0; e0 < 1024; e0 += 256) {
            const int e = e0 + tid;
            int ii, kk;
            if (g.sak == 1) { kk = e & 15; ii = e >> 4; } else { ii = e & 63; kk = e >> 6; }       // contiguous index fastest
            As[kk][ii] = (i0 + ii < g.M && k0 + kk < g.K) ? g.A[(long)(i0 + ii) * g.sai + (long)(k0 + kk) * g.sak] : 0.0;
            int jj, kb;
            if (g.sbk == 1) { kb = e & 15; jj = e >> 4; } else { jj = e & 63; kb = e >> 6; }
            Bs[kb][jj] = (j0 + jj < g.N && k0 + kb < g.K) ? g.B[(long)(k0 + kb) * g.sbk + (long)(j0 + jj) * g.sbj] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            double a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; r++) { a[r] = As[kk][ty * 4 + r]; b[r] = Bs[kk][tx * 4 + r]; }
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[r][c] += a[r] * b[c];
        }
        __syncthreads();
    }
    double al = g.alpha;
    if (g.alpha_dev) al = g.inv ? al / g.alpha_dev[0] : al * g.alpha_dev[0];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int i = i0 + ty * 4 + r, j = j0 + tx * 4 + c;
            if (i < g.M && j < g.N) {
                double v = al * acc[r][c] + (i == j ? g.diag : 0.0);
                if constexpr (MERGE) {
                    v += g.r1c * g.r1[i] * g.r1[j];
                    if (g.beta != 0.0) v += g.beta * g.C[(size_t)i * g.N + j];
                }
                g.C[(size_t)i * g.N + j] = v;
            }
        }
}
void dgemm(hipStream_t st, const double* A, long sai, long sak, const double* B, long sbk, long sbj, double* C, int M, int N, int K,
           double alpha, double diag, const double* alpha_dev = nullptr, int inv = 0) {
    GemmArgs g = {A, sai, sak, B, sbk, sbj, C, M, N, K, alpha, diag, alpha_dev, inv, 0.0, 0.0, nullptr};
    hipLaunchKernelGGL(dgemm_kernel<false>, dim3((N + 63) / 64, (M + 63) / 64), dim3(256), 0, st, g);
}

// single-workgroup reductions (fixed order): out[slot] = sqrt(sum x^2) | trace | |a - b|^2
__global__ __launch_bounds__(1024) void reduce_kernel(int mode, const double* x, const double* y, size_t n, int d, double* out) {
    __shared__ double sh[16];
    double acc = 0.0;
    if (mode == 0) for (size_t i = threadIdx.x; i < n; i += 1024) acc += x[i] * x[i];                    // |x|_F^2
    else if (mode == 1) for (int i = threadIdx.x; i < d; i += 1024) acc += x[(size_t)i * d + i];         // trace
    else for (size_t i = threadIdx.x; i < n; i += 1024) { const double t = x[i] - y[i]; acc += t * t; }  // |x - y|^2
    const double s = block_sum_f64(acc, sh);
    if (threadIdx.x == 0) out[0] = mode == 0 ? sqrt(s) : s;
}
// B = A + (mult * |A|_F) I
__global__ void shift_kernel(const double* A, const double* norm, double mult, size_t n2, int d, double* B) {
    const double delta = mult * norm[0];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (size_t)gridDim.x * 256)
        B[i] = A[i] + ((i / d == i % d) ? delta : 0.0);
}
__global__ void scale_identity_kernel(const double* B, const double* norm, size_t n2, int d, double* Y, double* Z) {
    const double inv = 1.0 / norm[0];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (size_t)gridDim.x * 256) {
        Y[i] = B[i] * inv;
        Z[i] = (i / d == i % d) ? 1.0 : 0.0;
    }
}
// scal: 0 |A|_F ; 3 |mu1 - mu2|^2, 4 tr(s1), 5 tr(s2) ; run r (0: shift delta, 1: shift 4 delta): 6+3r |B|_F, 7+3r tr(Y) now,
// 8+3r tr(Y) one step earlier
__global__ void frechet_finish_kernel(const double* scal, int shifted, double* out) {
    const double f1 = scal[7] * sqrt(scal[6]);
    double tr = f1, resid = fabs(scal[7] - scal[8]) / fmax(fabs(scal[7]), 1e-300);
    if (shifted) {
        // tr sqrt(A + delta I) = T + k sqrt(delta) + O(delta) with k the number of zero eigenvalues (rank-deficient
        // covariances: fewer samples than dimensions): two shifts, delta and 4 delta, cancel the sqrt(delta) term
        const double f4 = scal[10] * sqrt(scal[9]);
        tr = 2.0 * f1 - f4;
        resid = fmax(resid, fabs(scal[10] - scal[11]) / fmax(fabs(scal[10]), 1e-300));
    }
    out[0] = scal[3] + scal[4] + scal[5] - 2.0 * tr;
    out[1] = resid;          // relative change of tr(Y) over the last Newton-Schulz step
}

int nblk(size_t n, int cap = 2048) {
    size_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > (size_t)cap ? cap : b));
}

}  // namespace

extern "C" int gcc_argmax_channels(const float* scores, int N, int C, size_t HW, int* pred, gcc_stream_t stream) {
    GCC_ENTER();
    if (!scores || !pred || N <= 0 || C <= 0 || HW == 0) return GCC_ERR_BAD_ARG;
    const size_t total = (size_t)N * HW;
    hipLaunchKernelGGL(argmax_kernel, dim3(nblk(total, 8192)), dim3(256), 0, (hipStream_t)stream, scores, C, HW, total, pred);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_confusion_hist(const int* pred, const int* label, size_t count, int n, long long* hist, gcc_stream_t stream) {
    GCC_ENTER();
    if (!pred || !label || !hist || n <= 0) return GCC_ERR_BAD_ARG;
    if ((size_t)n * n * sizeof(unsigned int) > 48 * 1024) return GCC_ERR_UNSUPPORTED;
    if (count == 0) return GCC_OK;
    hipLaunchKernelGGL(hist_kernel, dim3(nblk(count, 1024)), dim3(256), (size_t)n * n * sizeof(unsigned int), (hipStream_t)stream, pred,
                       label, count, n, (unsigned long long*)hist);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" size_t gcc_psnr_workspace(void) { return 1024 * sizeof(double); }

extern "C" int gcc_psnr_y_sse(const float* fake, const float* real, int N, int H, int W, double* sse, int accumulate, void* ws,
                              size_t ws_bytes, gcc_stream_t stream) {
    GCC_ENTER();
    if (!fake || !real || !sse || !ws || N <= 0 || H <= 8 || W <= 8) return GCC_ERR_BAD_ARG;
    if (ws_bytes < gcc_psnr_workspace()) return GCC_ERR_WORKSPACE;
    const int nb = nblk((size_t)N * (H - 8) * (W - 8), 1024);
    hipLaunchKernelGGL(psnr_sse_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, fake, real, N, H, W, (double*)ws);
    GCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, nb, 1.0, sse, accumulate);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_ssim_y_sum(const float* fake, const float* real, int N, int H, int W, double* ssim_sum, int accumulate, void* ws,
                             size_t ws_bytes, gcc_stream_t stream) {
    GCC_ENTER();
    if (!fake || !real || !ssim_sum || !ws || N <= 0 || H < 8 + 7 || W < 8 + 7) return GCC_ERR_BAD_ARG;
    if (ws_bytes < gcc_psnr_workspace()) return GCC_ERR_WORKSPACE;
    const int nb = nblk((size_t)N * (H - 14) * (W - 14), 1024);
    hipLaunchKernelGGL(ssim_y_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, fake, real, N, H, W, 255.0, (double*)ws);
    GCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, nb, 1.0, ssim_sum, accumulate);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" size_t gcc_activation_stats_workspace(int n, int d) {
    if (n <= 0 || d <= 0) return 0;
    return ((size_t)n * d + (size_t)64 * d) * sizeof(double);      // centred copy | column-sum slices
}

extern "C" int gcc_activation_stats(const void* act, int is_f64, int n, int d, double* mu, double* sigma, void* ws, size_t ws_bytes,
                                    gcc_stream_t stream) {
    GCC_ENTER();
    if (!act || !mu || !sigma || !ws || n < 2 || d <= 0) return GCC_ERR_BAD_ARG;
    if (ws_bytes < gcc_activation_stats_workspace(n, d)) return GCC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double* xc = (double*)ws;
    double* part = xc + (size_t)n * d;
    const int slices = n < 64 ? 1 : 64, rows_per = (n + slices - 1) / slices;
    hipLaunchKernelGGL(colsum_kernel, dim3((d + 255) / 256, slices), dim3(256), 0, st, act, is_f64, n, d, rows_per, part);
    GCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(mean_finalize_kernel, dim3((d + 255) / 256), dim3(256), 0, st, (const double*)part, slices, n, d, mu);
    GCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(center_kernel, dim3(nblk((size_t)n * d)), dim3(256), 0, st, act, is_f64, (size_t)n * d, d, (const double*)mu, xc);
    GCC_CHECK_LAUNCH();
    // sigma = Xc^T Xc / (n - 1)
    dgemm(st, xc, 1, d, xc, d, 1, sigma, d, d, n, 1.0 / (double)(n - 1), 0.0);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" size_t gcc_activation_stats_stream_workspace(int max_batch, int d) {
    if (max_batch <= 0 || d <= 0) return 0;
    return ((size_t)d + (size_t)max_batch * d) * sizeof(double);    // delta | the batch centred on its own mean
}

extern "C" int gcc_activation_stats_update(const void* act, int is_f64, int ld, int b, int d, long long n_before, double* mean,
                                           double* m2, void* ws, size_t ws_bytes, gcc_stream_t stream) {
    GCC_ENTER();
    if (!act || !mean || !m2 || !ws || b <= 0 || d <= 0 || ld < d || n_before < 0) return GCC_ERR_BAD_ARG;
    if (ws_bytes < gcc_activation_stats_stream_workspace(b, d)) return GCC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double* delta = (double*)ws;
    double* xc = delta + d;
    const double n = (double)n_before + (double)b;
    hipLaunchKernelGGL(stream_center_kernel, dim3((d + 63) / 64), dim3(256), 0, st, act, is_f64, ld, b, d, n_before == 0 ? 1 : 0,
                       (double)b / n, mean, delta, xc);
    GCC_CHECK_LAUNCH();
    // M2 <- M2 + Xc^T Xc + (n_before b / n) delta delta^T; the first batch writes M2 without reading it
    GemmArgs g = {xc, 1, d, xc, d, 1, m2, d, d, b, 1.0, 0.0, nullptr, 0, n_before == 0 ? 0.0 : 1.0, (double)n_before * (double)b / n,
                  delta};
    hipLaunchKernelGGL(dgemm_kernel<true>, dim3((d + 63) / 64, (d + 63) / 64), dim3(256), 0, st, g);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_activation_stats_finish(const double* m2, long long n, int d, double* sigma, gcc_stream_t stream) {
    GCC_ENTER();
    if (!m2 || !sigma || n < 2 || d <= 0) return GCC_ERR_BAD_ARG;
    const size_t n2 = (size_t)d * d;
    hipLaunchKernelGGL(scale_kernel, dim3(nblk(n2)), dim3(256), 0, (hipStream_t)stream, m2, 1.0 / (double)(n - 1), n2, sigma);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" size_t gcc_frechet_workspace(int d) {
    if (d <= 0) return 0;
    return ((size_t)6 * d * d + 16) * sizeof(double);
}

extern "C" int gcc_frechet_distance(const double* mu1, const double* sigma1, const double* mu2, const double* sigma2, int d,
                                    int iterations, double shift_rel, double* out, void* ws, size_t ws_bytes,
                                    gcc_stream_t stream) {
    GCC_ENTER();
    if (!mu1 || !sigma1 || !mu2 || !sigma2 || !out || !ws || d <= 0 || iterations < 2 || shift_rel < 0.0) return GCC_ERR_BAD_ARG;
    if (ws_bytes < gcc_frechet_workspace(d)) return GCC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t n2 = (size_t)d * d;
    double* scal = (double*)ws;
    double* A = scal + 16;
    double *Y = A + n2, *Z = Y + n2, *T = Z + n2, *Y2 = T + n2, *Z2 = Y2 + n2;
    dgemm(st, sigma1, d, 1, sigma2, d, 1, A, d, d, d, 1.0, 0.0);
    hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(1024), 0, st, 0, (const double*)A, (const double*)nullptr, n2, d, scal + 0);
    hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(1024), 0, st, 2, mu1, mu2, (size_t)d, d, scal + 3);
    hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(1024), 0, st, 1, sigma1, (const double*)nullptr, n2, d, scal + 4);
    hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(1024), 0, st, 1, sigma2, (const double*)nullptr, n2, d, scal + 5);
    GCC_CHECK_LAUNCH();
    const int runs = shift_rel > 0.0 ? 2 : 1;
    for (int r = 0; r < runs; r++) {
        double* sc = scal + 6 + 3 * r;
        // T doubles as the home of B = A + delta I until the first product overwrites it
        hipLaunchKernelGGL(shift_kernel, dim3(nblk(n2)), dim3(256), 0, st, (const double*)A, (const double*)scal,
                           shift_rel * (r == 0 ? 1.0 : 4.0), n2, d, T);
        hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(1024), 0, st, 0, (const double*)T, (const double*)nullptr, n2, d, sc + 0);
        hipLaunchKernelGGL(scale_identity_kernel, dim3(nblk(n2)), dim3(256), 0, st, (const double*)T, (const double*)sc, n2, d, Y, Z);
        GCC_CHECK_LAUNCH();
        for (int it = 0; it < iterations; it++) {
            dgemm(st, Z, d, 1, Y, d, 1, T, d, d, d, -0.5, 1.5);        // T = (3 I - Z Y) / 2
            dgemm(st, Y, d, 1, T, d, 1, Y2, d, d, d, 1.0, 0.0);         // Y <- Y T
            dgemm(st, T, d, 1, Z, d, 1, Z2, d, d, d, 1.0, 0.0);         // Z <- T Z
            double* t = Y; Y = Y2; Y2 = t;
            t = Z; Z = Z2; Z2 = t;
            if (it >= iterations - 2)
                hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(1024), 0, st, 1, (const double*)Y, (const double*)nullptr, n2, d,
                                   sc + (it == iterations - 1 ? 1 : 2));
        }
        GCC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(frechet_finish_kernel, dim3(1), dim3(1), 0, st, (const double*)scal, runs == 2 ? 1 : 0, out);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

// =============================================================================================
// Input pipeline (data/aligned_dataset.py:27-56, data/base_dataset.py:63-112): the paired image
// is split, each half resized with PIL's BICUBIC, cropped, flipped, scaled to [0, 1] and normalised to [-1, 1].
// Pillow (the reference's un-pinned image library; 12.2.0 in this image) resamples 8-bit images in two passes of
// integer arithmetic -- horizontal, then vertical, with 22-bit fixed-point coefficients and a rounded, clipped uint8
// intermediate (Resample.c: ImagingResampleHorizontal_8bpc / Vertical_8bpc).  The kernels below reproduce exactly that;
// the coefficient tables (double precision, a few hundred entries) are built by the caller with Pillow's arithmetic
// (gcc_amd/data/__init__.py::resample_coeffs) and passed in.
namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ unsigned char clip8(int v) {
    v >>= PRECISION_BITS;                       // arithmetic shift, as the C code's lookup index
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// dst[y][xx][c] over the columns of src: bounds[xx] = {xmin, count}, coef[xx][0..count)
__global__ __launch_bounds__(256) void resample_h_kernel(const unsigned char* __restrict__ src, size_t pitch, int H, int outW,
                                                         const int* __restrict__ bounds, const int* __restrict__ coef, int ksize,
                                                         unsigned char* __restrict__ dst) {
    const size_t total = (size_t)H * outW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / outW), xx = (int)(i - (size_t)y * outW);
        const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
        const int* k = coef + (size_t)xx * ksize;
        const unsigned char* row = src + (size_t)y * pitch + (size_t)xmin * 3;
        int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
        for (int x = 0; x < cnt; x++) {
            const int kv = k[x];
            s0 += row[3 * x] * kv; s1 += row[3 * x + 1] * kv; s2 += row[3 * x + 2] * kv;
        }
        unsigned char* o = dst + i * 3;
        o[0] = clip8(s0); o[1] = clip8(s1); o[2] = clip8(s2);
    }
}
// dst[yy][x][c] over the rows of src (tightly packed [H][W][3])
__global__ __launch_bounds__(256) void resample_v_kernel(const unsigned char* __restrict__ src, size_t pitch, int W, int outH,
                                                         const int* __restrict__ bounds, const int* __restrict__ coef, int ksize,
                                                         unsigned char* __restrict__ dst) {
    const size_t total = (size_t)outH * W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int yy = (int)(i / W), x = (int)(i - (size_t)yy * W);
        const int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
        const int* k = coef + (size_t)yy * ksize;
        const unsigned char* p = src + (size_t)ymin * pitch + (size_t)x * 3;
        int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
        for (int y = 0; y < cnt; y++) {
            const int kv = k[y];
            s0 += p[0] * kv; s1 += p[1] * kv; s2 += p[2] * kv;
            p += pitch;
        }
        unsigned char* o = dst + i * 3;
        o[0] = clip8(s0); o[1] = clip8(s1); o[2] = clip8(s2);
    }
}
// crop + horizontal flip + ToTensor (/255) + a range conversion, NCHW fp32 (and optionally the model's NHWC bf16 input):
//   form 0  Normalize(mean, std): (v / 255 - mean[c]) / std[c]      (base_dataset.py:108-111; sr_dataset.py:52-56)
//   form 1  convert_image '[-1, 1]': 2 * (v / 255) - 1              (sr_dataset.py:49-50)
//   form 2  '[0, 1]': v / 255
struct ConvArgs { float mean[3], stdv[3]; int form; };
__global__ __launch_bounds__(256) void crop_flip_norm_kernel(const unsigned char* __restrict__ src, size_t pitch, int x0, int y0,
                                                             int ch, int cw, int flip, const ConvArgs cv, float* __restrict__ nchw,
                                                             bf16_t* __restrict__ nhwc, int ld) {
    const size_t total = (size_t)ch * cw;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / cw), x = (int)(i - (size_t)y * cw);
        const int sx = flip ? (cw - 1 - x) : x;
        const unsigned char* p = src + (size_t)(y0 + y) * pitch + (size_t)(x0 + sx) * 3;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float t = (float)p[c] / 255.f;
            v[c] = cv.form == 0 ? (t - cv.mean[c]) / cv.stdv[c] : (cv.form == 1 ? 2.f * t - 1.f : t);
        }
        if (nchw) {
#pragma unroll
            for (int c = 0; c < 3; c++) nchw[(size_t)c * total + i] = v[c];
        }
        if (nhwc) {
            bf16_t* o = nhwc + i * ld;
#pragma unroll
            for (int c = 0; c < 3; c++) o[c] = f2bf(v[c]);
        }
    }
}

}  // namespace

extern "C" int gcc_resample_u8(const void* src, int in_h, int in_w, size_t pitch, void* dst, int out_h, int out_w,
                               const int* hbounds, const int* hcoef, int hk, const int* vbounds, const int* vcoef, int vk,
                               void* tmp, gcc_stream_t stream) {
    GCC_ENTER();
    if (!src || !dst || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0 || pitch < (size_t)in_w * 3) return GCC_ERR_BAD_ARG;
    const bool need_h = out_w != in_w, need_v = out_h != in_h;
    if ((need_h && (!hbounds || !hcoef || hk <= 0)) || (need_v && (!vbounds || !vcoef || vk <= 0))) return GCC_ERR_BAD_ARG;
    if (need_h && need_v && !tmp) return GCC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* s = (const unsigned char*)src;
    size_t sp = pitch;
    if (!need_h && !need_v) {        // PIL returns a copy
        if (hipMemcpy2DAsync(dst, (size_t)in_w * 3, src, pitch, (size_t)in_w * 3, in_h, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return GCC_ERR_LAUNCH;
        return GCC_OK;
    }
    if (need_h) {
        unsigned char* o = (unsigned char*)(need_v ? tmp : dst);
        hipLaunchKernelGGL(resample_h_kernel, dim3(nblk((size_t)in_h * out_w, 4096)), dim3(256), 0, st, s, sp, in_h, out_w, hbounds,
                           hcoef, hk, o);
        GCC_CHECK_LAUNCH();
        s = o; sp = (size_t)out_w * 3;
    }
    if (need_v) {
        hipLaunchKernelGGL(resample_v_kernel, dim3(nblk((size_t)out_h * out_w, 4096)), dim3(256), 0, st, s, sp, out_w, out_h, vbounds,
                           vcoef, vk, (unsigned char*)dst);
        GCC_CHECK_LAUNCH();
    }
    return GCC_OK;
}

extern "C" int gcc_crop_convert(const void* src, int H, int W, size_t pitch, int x0, int y0, int crop_h, int crop_w, int flip,
                                int form, const float* mean3, const float* std3, float* nchw, void* nhwc_bf16, int ld,
                                gcc_stream_t stream) {
    GCC_ENTER();
    if (!src || (!nchw && !nhwc_bf16) || crop_h <= 0 || crop_w <= 0 || x0 < 0 || y0 < 0 || x0 + crop_w > W || y0 + crop_h > H ||
        pitch < (size_t)W * 3 || (nhwc_bf16 && (ld < 3)) || form < 0 || form > 2 || (form == 0 && (!mean3 || !std3)))
        return GCC_ERR_BAD_ARG;
    ConvArgs cv = {};
    cv.form = form;
    for (int c = 0; c < 3; c++) { cv.mean[c] = form == 0 ? mean3[c] : 0.f; cv.stdv[c] = form == 0 ? std3[c] : 1.f; }
    hipLaunchKernelGGL(crop_flip_norm_kernel, dim3(nblk((size_t)crop_h * crop_w, 4096)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)src, pitch, x0, y0, crop_h, crop_w, flip, cv, nchw, (bf16_t*)nhwc_bf16, ld);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_crop_flip_normalize(const void* src, int H, int W, size_t pitch, int x0, int y0, int crop_h, int crop_w, int flip,
                                       float* nchw, void* nhwc_bf16, int ld, gcc_stream_t stream) {
    const float half[3] = {0.5f, 0.5f, 0.5f};
    return gcc_crop_convert(src, H, W, pitch, x0, y0, crop_h, crop_w, flip, 0, half, half, nchw, nhwc_bf16, ld, stream);
}

// =============================================================================================
// Cityscapes mIoU around the segmenter (metric/test_metric.py:47-87, metric/mIoU_score.py:70-105, 169-218).
//   gcc_seg_input    util.tensor2im's byte of the generated image, then SegList's ToTensor + Normalize in fp32
//   gcc_miou_score   resize_4d_tensor (PIL's 32-bit float BILINEAR resample, horizontal pass then vertical pass, f64 accumulation
//                    in tap order, fp32 after each pass; a pass PIL skips runs with the table {1.0}, which keeps every value
//                    but turns -0.0 into +0.0: equal under the argmax) + argmax over classes + fast_hist in ONE launch: the resized score tensor
//                    ([N][19][1024][2048] fp32 in the reference) never exists.  Pillow multiplies and adds separately in f64:
//                    the kernel is compiled with `fp contract(off)` and spells the products and sums as plain operators (the
//                    __dmul_rn / __dadd_rn header functions carry the translation unit's contraction flag and were fused).
// A workgroup owns MS_TH output rows x 256 output columns, one column per thread.  The rows of a tile share at most MS_TH + 2
// source rows (supported sizes never shrink, so consecutive output rows advance by at most one source row): per class the thread
// resamples those source rows horizontally once into its own LDS column, applies each output row's vertical taps (read from the
// table once, before the class loop) and carries best / best index per row in registers across the class loop.  Labels feed a
// per-workgroup uint32 histogram in LDS that is folded into the int64 table with 64-bit atomics (integers: the result does not
// depend on arrival order).  Measured at 19 x 256 x 256 -> 1024 x 2048 (profiles/r8_miou_ab.txt): MS_TH 8 beats 4 and 16; staging
// the source window of several class planes in LDS first, or issuing a class plane's loads ahead of their use, was slower.
namespace {

constexpr int MS_TW = 256, MS_TH = 8, MS_SRC = MS_TH + 2, MS_TAPS = 3, MS_MAX_CLASSES = 64;

struct SegInArgs { float mean[3], stdv[3]; };

__global__ __launch_bounds__(256) void seg_input_kernel(const bf16_t* __restrict__ xb, const unsigned char* __restrict__ xu, int ld,
                                                        int off, size_t plane, size_t total, const SegInArgs a,
                                                        float* __restrict__ out) {
#pragma clang fp contract(off)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t n = i / plane, p = i - n * plane;
        float* o = out + n * 3 * plane + p;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float b;
            if (xu) {
                b = (float)xu[i * 3 + c];
            } else {
                // util.tensor2im exactly as gcc_image_to_u8 computes it
                float t = __fmul_rn(__fmul_rn(__fadd_rn(bf2f(xb[i * ld + off + c]), 1.f), 0.5f), 255.f);
                t = t > 0.f ? (t < 255.f ? t : 255.f) : 0.f;
                b = (float)(unsigned char)t;
            }
            // ToTensor's img.float() / 255, then Normalize's t.sub_(m).div_(s): two IEEE divisions, no reciprocal
            o[(size_t)c * plane] = __fsub_rn(b / 255.f, a.mean[c]) / a.stdv[c];
        }
    }
}

struct MiouArgs {
    const float* scores; const unsigned char* labels;
    const int* hb; const double* hc; const int* vb; const double* vc;
    unsigned long long* hist; unsigned char* pred;
    int C, h, w, H, W, hk, vk;
};

__global__ __launch_bounds__(256) void miou_score_kernel(const MiouArgs a) {
#pragma clang fp contract(off)
    extern __shared__ unsigned int sh[];                 // [C][C]
    __shared__ float hv[MS_SRC][MS_TW];                  // column tid belongs to thread tid alone: no barrier around it
    const int tid = threadIdx.x, x = blockIdx.x * MS_TW + tid, y0 = blockIdx.y * MS_TH, n = blockIdx.z;
    const int C = a.C, nn = C * C;
    for (int i = tid; i < nn; i += 256) sh[i] = 0u;
    __syncthreads();
    const int rows = min(MS_TH, a.H - y0);
    if (x < a.W) {
        // the tables come from the caller: every index derived from them is clamped into the source plane
        int xcnt = min(min(a.hb[2 * x + 1], a.hk), MS_TAPS);
        xcnt = max(min(xcnt, a.w), 0);
        const int xmin = max(min(a.hb[2 * x], a.w - xcnt), 0);
        double kx[MS_TAPS];
#pragma unroll
        for (int k = 0; k < MS_TAPS; k++) kx[k] = k < xcnt ? a.hc[(size_t)x * a.hk + k] : 0.0;
        const int ybase = max(min(a.vb[2 * y0], a.h - 1), 0);
        const int ylast = y0 + rows - 1;
        const int nsrc = max(min(min(a.vb[2 * ylast] + a.vb[2 * ylast + 1], a.h) - ybase, MS_SRC), 1);
        // the tile's vertical taps, read once (wave-uniform): the class loop below touches no table
        int vj[MS_TH], vcnt[MS_TH];
        double kv[MS_TH][MS_TAPS];
        float best[MS_TH];
        int bi[MS_TH];
#pragma unroll
        for (int r = 0; r < MS_TH; r++) {
            const int y = min(y0 + r, ylast);
            vcnt[r] = min(min(a.vb[2 * y + 1], a.vk), MS_TAPS);
            vj[r] = a.vb[2 * y] - ybase;
#pragma unroll
            for (int k = 0; k < MS_TAPS; k++) kv[r][k] = k < vcnt[r] ? a.vc[(size_t)y * a.vk + k] : 0.0;
            best[r] = 0.f; bi[r] = 0;
        }
        for (int c = 0; c < C; c++) {
            const float* plane = a.scores + ((size_t)n * C + c) * a.h * a.w;
            for (int j = 0; j < nsrc; j++) {
                const float* row = plane + (size_t)(ybase + j) * a.w + xmin;
                double ss = 0.0;
#pragma unroll
                for (int k = 0; k < MS_TAPS; k++)
                    if (k < xcnt) ss += (double)row[k] * kx[k];
                hv[j][tid] = (float)ss;
            }
#pragma unroll
            for (int r = 0; r < MS_TH; r++) {
                if (r < rows) {
                    double ss = 0.0;
#pragma unroll
                    for (int k = 0; k < MS_TAPS; k++)
                        if (k < vcnt[r]) {
                            const int j = max(min(vj[r] + k, nsrc - 1), 0);
                            ss += (double)hv[j][tid] * kv[r][k];
                        }
                    const float v = (float)ss;
                    // numpy.argmax: first maximum; a NaN counts as the maximum (first NaN wins)
                    if (c == 0) { best[r] = v; }
                    else if (best[r] == best[r] && (v > best[r] || v != v)) { best[r] = v; bi[r] = c; }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < MS_TH; r++) {
            if (r < rows) {
                const size_t o = ((size_t)n * a.H + (y0 + r)) * a.W + x;
                if (a.pred) a.pred[o] = (unsigned char)bi[r];
                const int l = a.labels[o];
                if (l < C) atomicAdd(&sh[C * l + bi[r]], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < nn; i += 256)
        if (sh[i]) atomicAdd(&a.hist[i], (unsigned long long)sh[i]);
}

}  // namespace

extern "C" int gcc_seg_input(const void* x, int is_u8, int ld, int off, int N, int H, int W, const float* mean3, const float* std3,
                             float* out, gcc_stream_t stream) {
    GCC_ENTER();
    if (!x || !out || !mean3 || !std3 || N <= 0 || H <= 0 || W <= 0) return GCC_ERR_BAD_ARG;
    if (!is_u8 && (ld <= 0 || off < 0 || (ld & 7) || (off & 7) || ld < off + 8)) return GCC_ERR_BAD_ARG;
    SegInArgs a;
    for (int c = 0; c < 3; c++) { a.mean[c] = mean3[c]; a.stdv[c] = std3[c]; }
    const size_t plane = (size_t)H * W, total = plane * N;
    hipLaunchKernelGGL(seg_input_kernel, dim3(nblk(total, 4096)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)(is_u8 ? nullptr : x), (const unsigned char*)(is_u8 ? x : nullptr), ld, off, plane, total, a, out);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_fid_input(const void* x, int form, int ld, int off, int N, int H, int W, float* out, gcc_stream_t stream) {
    if (form == GCC_FID_IN_BF16 || form == GCC_FID_IN_U8) {
        // the byte of gcc_seg_input over 255; (q - 0) / 1 keeps q's bits
        const float zero[3] = {0.f, 0.f, 0.f}, one[3] = {1.f, 1.f, 1.f};
        return gcc_seg_input(x, form == GCC_FID_IN_U8, ld, off, N, H, W, zero, one, out, stream);
    }
    GCC_ENTER();
    if (form != GCC_FID_IN_F32 || !x || !out || N <= 0 || H <= 0 || W <= 0) return GCC_ERR_BAD_ARG;
    const size_t total = (size_t)N * 3 * H * W;
    const bool aligned = (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    const size_t nvec = aligned ? total / 4 : 0;
    hipLaunchKernelGGL(fid_input_f32_kernel, dim3(nblk(nvec + (total - 4 * nvec), 4096)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)x, nvec, total, out);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_miou_score(const float* scores, int N, int C, int h, int w, const unsigned char* labels, int H, int W,
                              const int* hbounds, const double* hcoef, int hk, const int* vbounds, const double* vcoef, int vk,
                              long long* hist, unsigned char* pred, gcc_stream_t stream) {
    GCC_ENTER();
    if (!scores || !labels || !hbounds || !hcoef || !vbounds || !vcoef || !hist || N <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 ||
        W <= 0 || hk <= 0 || vk <= 0)
        return GCC_ERR_BAD_ARG;
    // an enlarging (or size-keeping) BILINEAR table has at most 3 taps per row; a reducing one widens with the scale
    if (h > H || w > W || C > MS_MAX_CLASSES || hk > MS_TAPS || vk > MS_TAPS || N > 65535 || (H + MS_TH - 1) / MS_TH > 65535)
        return GCC_ERR_UNSUPPORTED;
    MiouArgs a = {scores, labels, hbounds, hcoef, vbounds, vcoef, (unsigned long long*)hist, pred, C, h, w, H, W, hk, vk};
    hipLaunchKernelGGL(miou_score_kernel, dim3((W + MS_TW - 1) / MS_TW, (H + MS_TH - 1) / MS_TH, N), dim3(256),
                       (size_t)C * C * sizeof(unsigned int), (hipStream_t)stream, a);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
