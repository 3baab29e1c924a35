// Kernel Inception Distance (Binkowski et al. 2018): the sums of the polynomial kernel k(x, y) = (x.y / d + 1)^3 over all pairs
// of rows of two activation sets, the three terms of the unbiased MMD^2 estimate (gcc_amd/metric/kid_score.py).
//   gcc_kid_poly_sum   out[0] = sum_{i, j} k(x_i, y_j), or, symmetric, sum_{i != j} k(x_i, x_j)
// The m x n Gram matrix never exists: a workgroup owns one KID_TILE x KID_TILE tile of pairs, walks d in steps of KID_KSTEP with
// both row panels staged in LDS as f64 (fp32 inputs are converted on the way in), keeps an 8 x 8 block of dot products per thread
// in registers, cubes them there, and writes ONE f64 partial per tile.  A second launch of one workgroup folds the partials.  The
// symmetric form visits only the tiles on and above the diagonal: a diagonal tile holds both (i, j) and (j, i) of its pairs and
// counts once without its i == j entries, a tile above the diagonal stands for its mirror image and counts twice (an exact
// doubling).  Every sum is taken in an order fixed by (m, n, d): a thread adds its 64 cubes in register order, a workgroup
// folds its lanes by xor-shuffles and its four waves in wave order, the fold kernel's lane l adds partials l, l + 1024, ... in
// tile-index order and folds the same way.  No floating-point atomics, no workgroup waits for another, no spin: same input, same
// bits.  The inner product is the LDS-tiled f64 FMA structure of metric.hip's dgemm_kernel (twice its tile side and four times its
// register block: 64 FMAs per 8 + 8 doubles read from LDS), not v_mfma_f64_16x16x4_f64: its f64 accumulator layout is the odd
// one out among the matrix instructions, the vector and matrix f64 peaks are the same 78 TFLOP/s, and a
// once-per-evaluation sum does not pay for a second layout to get wrong.
#include "common.hpp"

namespace {

constexpr int KT = GCC_KID_TILE, KK = GCC_KID_KSTEP, KR = KT / 16, KLD = KT + 2;      // KLD: an even pad keeps 16-byte reads aligned
static_assert(KT == 128 && KK == 16 && KR == 8, "the staging loops below are written for 128 x 128 x 16 and 256 threads");

struct KidArgs {
    const void* X; const void* Y;
    long ldx, ldy;
    int x_f64, y_f64, m, n, d, symmetric, tiles_n;
    double inv_d;
    double* partial;
};

__device__ __forceinline__ double kid_load(const void* p, int is_f64, long idx) {
    return is_f64 ? ((const double*)p)[idx] : (double)((const float*)p)[idx];
}

__device__ __forceinline__ double kid_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) s += sh[i];
    return s;
}

__global__ __launch_bounds__(256) void kid_tile_kernel(const KidArgs g) {
    __shared__ __attribute__((aligned(16))) double Xs[KK][KLD], Ys[KK][KLD];
    __shared__ double red[4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int ti, tj;
    if (g.symmetric) {
        // tile b of the upper triangle, rows first: row ti starts at ti T - ti (ti - 1) / 2
        const long T = g.tiles_n, b = blockIdx.x;
        long r = (long)(((double)(2 * T + 1) - sqrt((double)((2 * T + 1) * (2 * T + 1) - 8 * b))) * 0.5);
        r = r < 0 ? 0 : (r > T - 1 ? T - 1 : r);
        while (r > 0 && r * T - r * (r - 1) / 2 > b) r--;
        while (r + 1 < T && (r + 1) * T - (r + 1) * r / 2 <= b) r++;
        ti = (int)r;
        tj = (int)(r + (b - (r * T - r * (r - 1) / 2)));
    } else {
        ti = blockIdx.x / g.tiles_n;
        tj = blockIdx.x - ti * g.tiles_n;
    }
    const int i0 = ti * KT, j0 = tj * KT;
    double acc[KR][KR];
#pragma unroll
    for (int r = 0; r < KR; r++)
#pragma unroll
        for (int c = 0; c < KR; c++) acc[r][c] = 0.0;
    for (int k0 = 0; k0 < g.d; k0 += KK) {
        // KT rows x KK columns per panel, 8 elements per thread, the column index fastest (rows are contiguous in memory);
        // rows past m / n and columns past d are zeros: they add exact zeros to the dot products
#pragma unroll
        for (int e0 = 0; e0 < KT * KK; e0 += 256) {
            const int e = e0 + tid, kk = e & (KK - 1), rr = e >> 4;
            const bool kin = k0 + kk < g.d;
            Xs[kk][rr] = (kin && i0 + rr < g.m) ? kid_load(g.X, g.x_f64, (long)(i0 + rr) * g.ldx + (k0 + kk)) : 0.0;
            Ys[kk][rr] = (kin && j0 + rr < g.n) ? kid_load(g.Y, g.y_f64, (long)(j0 + rr) * g.ldy + (k0 + kk)) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KK; kk++) {
            double a[KR], b[KR];
#pragma unroll
            for (int r = 0; r < KR; r++) { a[r] = Xs[kk][ty * KR + r]; b[r] = Ys[kk][tx * KR + r]; }
#pragma unroll
            for (int r = 0; r < KR; r++)
#pragma unroll
                for (int c = 0; c < KR; c++) acc[r][c] += a[r] * b[c];
        }
        __syncthreads();
    }
    const bool diag = g.symmetric && ti == tj;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < KR; r++)
#pragma unroll
        for (int c = 0; c < KR; c++) {
            const int i = i0 + ty * KR + r, j = j0 + tx * KR + c;
            if (i < g.m && j < g.n && !(diag && i == j)) {
                const double t = acc[r][c] * g.inv_d + 1.0;
                s += t * t * t;
            }
        }
    s = kid_block_sum(s, red);
    if (tid == 0) g.partial[blockIdx.x] = (g.symmetric && !diag) ? 2.0 * s : s;
}

__global__ __launch_bounds__(1024) void kid_fold_kernel(const double* __restrict__ partial, long tiles, double* out) {
    __shared__ double red[16];
    double acc = 0.0;
    for (long i = threadIdx.x; i < tiles; i += 1024) acc += partial[i];
    const double s = kid_block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = s;
}

long kid_tiles(int rows) { return ((long)rows + KT - 1) / KT; }

}  // namespace

extern "C" size_t gcc_kid_workspace(int m, int n, int d) {
    if (m <= 0 || n <= 0 || d <= 0) return 0;
    return (size_t)(kid_tiles(m) * kid_tiles(n)) * sizeof(double);
}

extern "C" int gcc_kid_poly_sum(const void* X, int x_f64, int ldx, int m, const void* Y, int y_f64, int ldy, int n, int d,
                                int symmetric, double* out, void* ws, size_t ws_bytes, gcc_stream_t stream) {
    GCC_ENTER();
    if (symmetric) { Y = X; y_f64 = x_f64; ldy = ldx; n = m; }       // Y is X: its own arguments are not read
    if (!X || !Y || !out || !ws || m <= 0 || n <= 0 || d <= 0 || ldx < d || ldy < d || (symmetric && m < 2)) return GCC_ERR_BAD_ARG;
    const long T = kid_tiles(m), Tn = kid_tiles(n);
    const long tiles = symmetric ? T * (T + 1) / 2 : T * Tn;
    if (tiles > 0x7fffffffL) return GCC_ERR_UNSUPPORTED;
    if (ws_bytes < (size_t)tiles * sizeof(double)) return GCC_ERR_WORKSPACE;
    KidArgs g = {X, Y, (long)ldx, (long)ldy, x_f64 != 0, y_f64 != 0, m, n, d, symmetric != 0, (int)Tn, 1.0 / (double)d, (double*)ws};
    hipLaunchKernelGGL(kid_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, g);
    GCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(kid_fold_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)ws, tiles, out);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
