// Inception Score (Salimans et al. 2016) on the pool features FID is computed from: the classifier head of the FID Inception
// network and the per-split scores (gcc_amd/metric/inception_score.py takes their mean and standard deviation on the host).
//   gcc_is_logits         Z[i][c] = b[c] + sum_k X[i][k] W[c][k]
//   gcc_is_split_scores   scores[s] = exp( mean_{i in split s} sum_c p_ic (log p_ic - log mbar_sc) ), p_i = softmax(Z_i),
//                         mbar_s = mean_{i in split s} p_i, split s = rows [s n / S, (s + 1) n / S)
// The n x C logits of a set never exist for the scorer: rows go through in chunks of GCC_IS_CHUNK, and what a chunk leaves
// behind is [S][C] + [S] doubles of state.  Per chunk three launches:
//   logits  kid.hip's LDS-tiled f64 FMA structure at a 64 x 64 tile (rows of X against rows of W over d in steps of 16, a 4 x 4
//           block of logits per thread).  An accumulator starts at b[c] and takes fma(x_k, w_k, acc) for k = 0, 1, ..., d - 1 --
//           columns past d are staged as zeros and add fma(0, 0, acc) --: the bits of Z[i][c] depend on row i, class c and d
//           alone, not on the tile, the chunk or the rows beside it.  The 64-wide tile, not kid.hip's 128: the 120 to 1000
//           images this project scores against the network's 1008 classes are 32 to 256 workgroups where the wide tile would
//           make 8 to 64.  GCC_IS_CHUNK is 4096 rows, 64 x 16 = 1024 workgroups a launch: at 1024 rows (256 workgroups, one
//           per compute unit, one wave per SIMD with nothing to hide its loads behind) the same 5000 rows took twice the time
//           (profiles/r21_inception_score.txt).
//   rows    one wave per row: m = max_c z_c, s = sum_c exp(z_c - m), logp_c = (z_c - m) - log s, p_c = exp(logp_c) written
//           over z_c, h = sum_c p_c logp_c with a class of p_c == 0 adding exactly 0.  Lane l takes the classes l, l + 64, ...
//           ascending and the lanes fold by xor-shuffles: an order fixed by C.
//   accum   one thread per (split, class) -- and one per split for h -- adds the chunk's rows of its split to the state in row
//           order: ONE chain per (split, class) over the rows of the split, which a chunk edge only interrupts.  The state, and
//           with it every score, has the same bits at every `chunk`.
// and at the end one workgroup per split: mbar_c = M[s][c] / n_s, E = sum_c mbar_c log mbar_c without the zeros (thread t takes
// the classes t, t + 256, ... ascending, lanes fold by xor-shuffles, waves in wave order), score = exp(H[s] / n_s - E).
// All arithmetic in f64.  No floating-point atomics, no workgroup waits for another, no spin: same input, same bits.
#include "common.hpp"

namespace {

constexpr int IT = GCC_IS_TILE, IK = GCC_IS_KSTEP, IR = IT / 16, ILD = IT + 2;        // ILD: an even pad keeps 16-byte reads aligned
static_assert(IT == 64 && IK == 16 && IR == 4, "the staging loops below are written for 64 x 64 x 16 and 256 threads");

struct IsLogitArgs {
    const void* X; const float* W; const float* b;
    long ldx;
    int x_f64, rows, d, C, tiles_c;
    double* Z;                               // [rows][C]
};

__device__ __forceinline__ double is_load(const void* p, int is_f64, long idx) {
    return is_f64 ? ((const double*)p)[idx] : (double)((const float*)p)[idx];
}

__global__ __launch_bounds__(256) void is_logits_kernel(const IsLogitArgs g) {
    __shared__ __attribute__((aligned(16))) double Xs[IK][ILD], Ws[IK][ILD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int ti = blockIdx.x / g.tiles_c, tj = blockIdx.x - ti * g.tiles_c;
    const int i0 = ti * IT, c0 = tj * IT;
    double acc[IR][IR];
#pragma unroll
    for (int c = 0; c < IR; c++) {
        const int cc = c0 + tx * IR + c;
        const double bias = cc < g.C ? (double)g.b[cc] : 0.0;
#pragma unroll
        for (int r = 0; r < IR; r++) acc[r][c] = bias;
    }
    for (int k0 = 0; k0 < g.d; k0 += IK) {
        // IT rows x IK columns per panel, 4 elements per thread, the column index fastest (rows are contiguous in memory);
        // rows past the chunk / classes past C and columns past d are zeros: nothing outside the operands is read
#pragma unroll
        for (int e0 = 0; e0 < IT * IK; e0 += 256) {
            const int e = e0 + tid, kk = e & (IK - 1), rr = e >> 4;
            const bool kin = k0 + kk < g.d;
            Xs[kk][rr] = (kin && i0 + rr < g.rows) ? is_load(g.X, g.x_f64, (long)(i0 + rr) * g.ldx + (k0 + kk)) : 0.0;
            Ws[kk][rr] = (kin && c0 + rr < g.C) ? (double)g.W[(long)(c0 + rr) * g.d + (k0 + kk)] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < IK; kk++) {
            double a[IR], w[IR];
#pragma unroll
            for (int r = 0; r < IR; r++) { a[r] = Xs[kk][ty * IR + r]; w[r] = Ws[kk][tx * IR + r]; }
#pragma unroll
            for (int r = 0; r < IR; r++)
#pragma unroll
                for (int c = 0; c < IR; c++) acc[r][c] = fma(a[r], w[c], acc[r][c]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < IR; r++) {
        const int i = i0 + ty * IR + r;
#pragma unroll
        for (int c = 0; c < IR; c++) {
            const int cc = c0 + tx * IR + c;
            if (i < g.rows && cc < g.C) g.Z[(long)i * g.C + cc] = acc[r][c];
        }
    }
}

__device__ __forceinline__ double is_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);          // a + b == b + a: every lane ends with the same bits
    return v;
}

// one wave per row of Z [rows][C]: the logits become the probabilities in place, h[row] = sum_c p_c log p_c
__global__ __launch_bounds__(256) void is_rows_kernel(double* __restrict__ Z, int rows, int C, double* __restrict__ h) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                 // a whole wave, and nothing below waits for another wave
    double* z = Z + (long)row * C;
    double m = -__builtin_huge_val();
    for (int c = lane; c < C; c += 64) m = fmax(m, z[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += exp(z[c] - m);
    const double ls = log(is_wave_sum(s));
    double hh = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double lp = (z[c] - m) - ls, p = exp(lp);
        z[c] = p;
        hh += p == 0.0 ? 0.0 : p * lp;       // 0 log 0 = 0, also where log p is -inf
    }
    hh = is_wave_sum(hh);
    if (lane == 0) h[row] = hh;
}

// thread (s, c), c < C: M[s][c] (+)= sum of P[i][c] over the chunk's rows i of split s, ascending; thread (s, C): H[s] likewise
// of h.  first: the chunk is the set's first and every state starts at +0, whether its split has rows in the chunk or not.
__global__ __launch_bounds__(256) void is_accum_kernel(const double* __restrict__ P, const double* __restrict__ h, int row0, int rows,
                                                       int n, int S, int C, int first, double* __restrict__ M, double* __restrict__ H) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)S * (C + 1)) return;
    const int s = (int)(idx / (C + 1)), c = (int)(idx - (long)s * (C + 1));
    long lo = (long)s * n / S, hi = (long)(s + 1) * n / S;
    lo = lo > row0 ? lo : row0;
    hi = hi < (long)row0 + rows ? hi : (long)row0 + rows;
    double* st = c < C ? M + (long)s * C + c : H + s;
    if (lo >= hi) {
        if (first) *st = 0.0;
        return;
    }
    const double* src = c < C ? P + c : h;
    const long stride = c < C ? C : 1;
    double acc = first ? 0.0 : *st;
#pragma unroll 8
    for (long i = lo; i < hi; i++) acc += src[(i - row0) * stride];
    *st = acc;
}

__global__ __launch_bounds__(256) void is_finish_kernel(const double* __restrict__ M, const double* __restrict__ H, int n, int S, int C,
                                                        double* __restrict__ scores) {
    __shared__ double red[4];
    const int s = blockIdx.x;
    const double ns = (double)((long)(s + 1) * n / S - (long)s * n / S);
    double e = 0.0;
    for (int c = threadIdx.x; c < C; c += 256) {
        const double mb = M[(long)s * C + c] / ns;
        e += mb > 0.0 ? mb * log(mb) : 0.0;
    }
    e = is_wave_sum(e);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) scores[s] = exp(H[s] / ns - (((red[0] + red[1]) + red[2]) + red[3]));
}

long is_tiles(long v) { return (v + IT - 1) / IT; }

bool is_bad_operands(const void* X, int ldx, int n, int d, const float* W, const float* b, int C, int chunk) {
    return !X || !W || !b || n < 1 || d < 1 || C < 2 || ldx < d || chunk < 0;
}

int is_launch_logits(const void* X, int x_f64, int ldx, int row0, int rows, int d, const float* W, const float* b, int C, double* Z,
                     hipStream_t stream) {
    const size_t elem = x_f64 ? sizeof(double) : sizeof(float);
    IsLogitArgs g = {(const char*)X + (size_t)row0 * (size_t)ldx * elem, W, b, (long)ldx, x_f64 != 0, rows, d, C, (int)is_tiles(C), Z};
    hipLaunchKernelGGL(is_logits_kernel, dim3((unsigned)(is_tiles(rows) * is_tiles(C))), dim3(256), 0, stream, g);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

}  // namespace

extern "C" size_t gcc_is_workspace(int C, int splits, int chunk) {
    if (C < 2 || splits < 1 || chunk < 0) return 0;
    const size_t ch = chunk ? chunk : GCC_IS_CHUNK;
    return (ch * (size_t)C + ch + (size_t)splits * (size_t)C + (size_t)splits) * sizeof(double);
}

extern "C" int gcc_is_logits(const void* X, int x_f64, int ldx, int n, int d, const float* W, const float* b, int C, int chunk,
                             double* Z, gcc_stream_t stream) {
    GCC_ENTER();
    if (is_bad_operands(X, ldx, n, d, W, b, C, chunk) || !Z) return GCC_ERR_BAD_ARG;
    const int ch = chunk ? chunk : GCC_IS_CHUNK;
    if (is_tiles(ch < n ? ch : n) * is_tiles(C) > 0x7fffffffL) return GCC_ERR_UNSUPPORTED;
    for (long row0 = 0; row0 < n; row0 += ch) {
        const int rows = (int)(n - row0 < ch ? n - row0 : ch);
        const int rc = is_launch_logits(X, x_f64, ldx, (int)row0, rows, d, W, b, C, Z + row0 * C, (hipStream_t)stream);
        if (rc != GCC_OK) return rc;
    }
    return GCC_OK;
}

extern "C" int gcc_is_split_scores(const void* X, int x_f64, int ldx, int n, int d, const float* W, const float* b, int C, int splits,
                                   int chunk, double* scores, void* ws, size_t ws_bytes, gcc_stream_t stream) {
    GCC_ENTER();
    if (is_bad_operands(X, ldx, n, d, W, b, C, chunk) || !scores || !ws || splits < 1 || n < splits) return GCC_ERR_BAD_ARG;
    const int ch = chunk ? chunk : GCC_IS_CHUNK;
    const long states = (long)splits * (C + 1);
    if (is_tiles(ch < n ? ch : n) * is_tiles(C) > 0x7fffffffL || (states + 255) / 256 > 0x7fffffffL) return GCC_ERR_UNSUPPORTED;
    if (ws_bytes < gcc_is_workspace(C, splits, chunk)) return GCC_ERR_WORKSPACE;
    double* Z = (double*)ws;                 // [ch][C]: a chunk's logits, then its probabilities
    double* h = Z + (size_t)ch * C;          // [ch]
    double* M = h + ch;                      // [splits][C]
    double* H = M + (size_t)splits * C;      // [splits]
    for (long row0 = 0; row0 < n; row0 += ch) {
        const int rows = (int)(n - row0 < ch ? n - row0 : ch);
        const int rc = is_launch_logits(X, x_f64, ldx, (int)row0, rows, d, W, b, C, Z, (hipStream_t)stream);
        if (rc != GCC_OK) return rc;
        hipLaunchKernelGGL(is_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, Z, rows, C, h);
        GCC_CHECK_LAUNCH();
        hipLaunchKernelGGL(is_accum_kernel, dim3((unsigned)((states + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const double*)Z, (const double*)h, (int)row0, rows, n, splits, C, (int)(row0 == 0), M, H);
        GCC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(is_finish_kernel, dim3((unsigned)splits), dim3(256), 0, (hipStream_t)stream, (const double*)M,
                       (const double*)H, n, splits, C, scores);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
