// Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) on the activations FID is
// computed from: the pairwise half (gcc_amd/metric/prdc_score.py does the rest).  With D(x, y) = sum_c (x_c - y_c)^2,
//   gcc_prdc_kth_dist     out[i] = the k-th smallest over j of D(x_i, y_j); symmetric: Y is X and j != i
//   gcc_prdc_ball_count   out[j] = #{ i : D(q_j, c_i) <= r2[i] }
// The m x n matrix of distances never exists.  A workgroup of 256 threads owns T rows and one of `chunks` ranges of T-column
// tiles; per column tile it walks d in steps of PK with both row panels staged in LDS as f64 (kid.hip's staging), keeps a
// T/16 x T/16 block of distances per thread in registers and consumes it there: a comparison against the column's radius and an
// integer add, or the selection below.  One partial per row and chunk goes to the workspace, a second launch merges the chunks
// per row.  T is 128 (kid.hip's 8 x 8 register block) where that grid can give every compute unit a workgroup, and 64 (4 x 4)
// below: the evaluation sets of this project are 120 to 1000 images, and a 128 x 128 tile of d = 2048 is 0.4 ms of one
// workgroup's time whatever else the chip is doing -- the small tile quarters that and makes four times the workgroups.
//
// D is the DIFFERENCE form, not |x|^2 + |y|^2 - 2 x.y: t = x_c - y_c (one rounding), acc = fma(t, t, acc) (one rounding), c
// ascending from 0, acc starting at +0.  It costs two f64 instructions per element where the dot form costs one, and buys what
// the four numbers are made of: D >= 0 always, D == 0 exactly for duplicate rows (so a radius of 0 still holds its duplicates
// under the inclusive <=), D(x, y) == D(y, x) bit for bit, and an error relative to D itself -- (d + 2) 2^-53 D -- where the dot
// form's is relative to |x|^2 + |y|^2 and decides close pairs by cancellation.  Rows past the end of a set and columns past d
// are staged as zeros: a padded column adds fma(0, 0, acc) = acc, so the bits of D(i, j) depend on the two rows and d alone --
// not on the tile either: both tiles run the same chain.
//
// Selection (kth_dist).  The k smallest of a row live in LDS (T x KC doubles, KC = 1 or GCC_PRDC_MAX_K), not in registers: 64
// accumulators and 8 x KC candidates per thread do not fit 256 VGPRs together.  After a column tile, per owned row: a thread
// sorts its distances into a KC-list (compare-exchange chain, fully unrolled: no indexed registers), the 16 lanes that share
// the row merge their lists by xor-shuffles (1, 2, 4, 8), and the lane with tx == 0 merges the result into the row's LDS list,
// which no other thread touches.  The k smallest of a multiset do not depend on the order they were met in, a sum of integers
// neither: every legal `chunks` and either tile give the same bits.  No floating-point atomics, no workgroup waits for
// another, no spin.
#include "common.hpp"

namespace {

constexpr int PK = GCC_PRDC_KSTEP, MAXK = GCC_PRDC_MAX_K, NT = 256, PG = 16;      // PG: the lanes that share a row
static_assert(GCC_PRDC_TILE == 128 && GCC_PRDC_SMALL_TILE == 64 && PK == 16 && GCC_PRDC_COL_TILE == GCC_PRDC_TILE,
              "the staging loops below are written for T x T x 16 tiles, T a multiple of 16, and 256 threads");

struct PrdcArgs {
    const void* X; const void* Y;          // rows (queries) and columns (centres)
    long ldx, ldy;
    int x_f64, y_f64, m, n, d, symmetric, k, chunks, col_tiles;
    const double* r2;                      // ball_count: [n]
    void* partial;                         // kth_dist: double [m][chunks][k]; ball_count: int [m][chunks]
};

__device__ __forceinline__ double prdc_load(const void* p, int is_f64, long idx) {
    return is_f64 ? ((const double*)p)[idx] : (double)((const float*)p)[idx];
}

// the R x R block (R = T / 16) of D of rows i0 + ty R + r against columns j0 + tx R + c; every thread of the workgroup calls it
template <int T>
__device__ __forceinline__ void prdc_tile(const PrdcArgs& g, int i0, int j0, double (*Xs)[T + 2], double (*Ys)[T + 2],
                                          double (&acc)[T / PG][T / PG]) {
    constexpr int R = T / PG;
    const int tid = threadIdx.x, tx = tid & (PG - 1), ty = tid / PG;
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int c = 0; c < R; c++) acc[r][c] = 0.0;
    for (int k0 = 0; k0 < g.d; k0 += PK) {
        // T rows x PK columns per panel, the column index fastest (rows are contiguous in memory); rows past m / n and columns
        // past d are zeros
#pragma unroll
        for (int e0 = 0; e0 < T * PK; e0 += NT) {
            const int e = e0 + tid, kk = e & (PK - 1), rr = e / PK;
            const bool kin = k0 + kk < g.d;
            Xs[kk][rr] = (kin && i0 + rr < g.m) ? prdc_load(g.X, g.x_f64, (long)(i0 + rr) * g.ldx + (k0 + kk)) : 0.0;
            Ys[kk][rr] = (kin && j0 + rr < g.n) ? prdc_load(g.Y, g.y_f64, (long)(j0 + rr) * g.ldy + (k0 + kk)) : 0.0;
        }
        __syncthreads();
        // unrolled by 8, not 16 as in kid.hip: at T = 128 the subtraction's temporaries on top of the 64 accumulators spill
        // at 16 under the 256 registers of two workgroups per CU (profiles/r19_prdc.txt)
#pragma unroll 8
        for (int kk = 0; kk < PK; kk++) {
            double a[R], b[R];
#pragma unroll
            for (int r = 0; r < R; r++) { a[r] = Xs[kk][ty * R + r]; b[r] = Ys[kk][tx * R + r]; }
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int c = 0; c < R; c++) {
                    const double t = a[r] - b[c];
                    acc[r][c] = fma(t, t, acc[r][c]);
                }
        }
        __syncthreads();
    }
}

// chunk ch of `chunks` over `tiles` column tiles: [lo, hi), never empty for chunks <= tiles
__device__ __forceinline__ void prdc_range(int ch, int chunks, int tiles, int& lo, int& hi) {
    lo = (int)((long)ch * tiles / chunks);
    hi = (int)((long)(ch + 1) * tiles / chunks);
}

// v into the ascending list l[0 .. KC): the KC smallest of the list and v stay
template <int KC>
__device__ __forceinline__ void prdc_insert(double (&l)[KC], double v) {
#pragma unroll
    for (int s = 0; s < KC; s++) {
        const double lo = v < l[s] ? v : l[s], hi = v < l[s] ? l[s] : v;
        l[s] = lo;
        v = hi;
    }
}

template <int T, int KC>
__global__ __launch_bounds__(NT, 2) void prdc_kth_kernel(const PrdcArgs g) {
    constexpr int R = T / PG;
    __shared__ __attribute__((aligned(16))) double Xs[PK][T + 2], Ys[PK][T + 2];
    __shared__ double Ls[T][KC];
    const int tid = threadIdx.x, tx = tid & (PG - 1), ty = tid / PG;
    const int ti = blockIdx.x / g.chunks, ch = blockIdx.x - ti * g.chunks, i0 = ti * T;
    const double inf = __builtin_huge_val();
    if (tx == 0) {
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int s = 0; s < KC; s++) Ls[ty * R + r][s] = inf;
    }
    int lo, hi;
    prdc_range(ch, g.chunks, g.col_tiles, lo, hi);
    for (int tj = lo; tj < hi; tj++) {
        const int j0 = tj * T;
        double acc[R][R];
        prdc_tile<T>(g, i0, j0, Xs, Ys, acc);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = i0 + ty * R + r;
            double l[KC];
#pragma unroll
            for (int s = 0; s < KC; s++) l[s] = inf;
#pragma unroll
            for (int c = 0; c < R; c++) {
                const int j = j0 + tx * R + c;
                prdc_insert<KC>(l, (j < g.n && !(g.symmetric && i == j)) ? acc[r][c] : inf);
            }
#pragma unroll
            for (int o = 1; o < PG; o <<= 1) {
                double other[KC];
#pragma unroll
                for (int s = 0; s < KC; s++) other[s] = __shfl_xor(l[s], o, 64);
#pragma unroll
                for (int s = 0; s < KC; s++) prdc_insert<KC>(l, other[s]);
            }
            if (tx == 0) {                   // the row's list belongs to this thread alone: no barrier
                double p[KC];
#pragma unroll
                for (int s = 0; s < KC; s++) p[s] = Ls[ty * R + r][s];
#pragma unroll
                for (int s = 0; s < KC; s++) prdc_insert<KC>(p, l[s]);
#pragma unroll
                for (int s = 0; s < KC; s++) Ls[ty * R + r][s] = p[s];
            }
        }
    }
    if (tx == 0) {
        double* partial = (double*)g.partial;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = i0 + ty * R + r;
            if (i < g.m)
                for (int s = 0; s < g.k; s++) partial[((long)i * g.chunks + ch) * g.k + s] = Ls[ty * R + r][s];
        }
    }
}

// one thread per row: the k-th smallest of its chunks x k candidates
__global__ __launch_bounds__(256) void prdc_kth_merge_kernel(const double* __restrict__ partial, int m, int chunks, int k, double* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double l[MAXK];
#pragma unroll
    for (int s = 0; s < MAXK; s++) l[s] = __builtin_huge_val();
    const double* p = partial + (long)i * chunks * k;
    for (int e = 0; e < chunks * k; e++) prdc_insert<MAXK>(l, p[e]);
    double v = l[0];
#pragma unroll
    for (int s = 1; s < MAXK; s++) v = (s == k - 1) ? l[s] : v;
    out[i] = v;
}

template <int T>
__global__ __launch_bounds__(NT, 2) void prdc_count_kernel(const PrdcArgs g) {
    constexpr int R = T / PG;
    __shared__ __attribute__((aligned(16))) double Xs[PK][T + 2], Ys[PK][T + 2];
    const int tid = threadIdx.x, tx = tid & (PG - 1), ty = tid / PG;
    const int ti = blockIdx.x / g.chunks, ch = blockIdx.x - ti * g.chunks, i0 = ti * T;
    int cnt[R];
#pragma unroll
    for (int r = 0; r < R; r++) cnt[r] = 0;
    int lo, hi;
    prdc_range(ch, g.chunks, g.col_tiles, lo, hi);
    for (int tj = lo; tj < hi; tj++) {
        const int j0 = tj * T;
        double acc[R][R];
        prdc_tile<T>(g, i0, j0, Xs, Ys, acc);
#pragma unroll
        for (int c = 0; c < R; c++) {
            const int j = j0 + tx * R + c;
            if (j < g.n) {
                const double rad = g.r2[j];
#pragma unroll
                for (int r = 0; r < R; r++) cnt[r] += acc[r][c] <= rad ? 1 : 0;
            }
        }
    }
    int* partial = (int*)g.partial;
#pragma unroll
    for (int r = 0; r < R; r++) {
        int v = cnt[r];
#pragma unroll
        for (int o = 1; o < PG; o <<= 1) v += __shfl_xor(v, o, 64);
        const int i = i0 + ty * R + r;
        if (tx == 0 && i < g.m) partial[(long)i * g.chunks + ch] = v;
    }
}

__global__ __launch_bounds__(256) void prdc_count_merge_kernel(const int* __restrict__ partial, int m, int chunks, int* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    int v = 0;
    for (int c = 0; c < chunks; c++) v += partial[(long)i * chunks + c];
    out[i] = v;
}

long prdc_tiles(int rows, int tile) { return ((long)rows + tile - 1) / tile; }
int prdc_max_chunks(int n, int tile) { const long t = prdc_tiles(n, tile); return (int)(t < GCC_PRDC_MAX_CHUNKS ? t : GCC_PRDC_MAX_CHUNKS); }

int prdc_chunks_at(int m, int n, int tile) {
    const long rows = prdc_tiles(m, tile), want = (GCC_PRDC_FILL_WORKGROUPS + rows - 1) / rows;
    const int most = prdc_max_chunks(n, tile);
    return (int)(want < most ? want : most);
}

// the tile and the chunks of a call (0: the library's choice of either), or false for a value the sizes do not admit
bool prdc_plan(int m, int n, int& tile, int& chunks) {
    if (tile == 0) tile = gcc_prdc_tile(m, n);
    if (tile != GCC_PRDC_TILE && tile != GCC_PRDC_SMALL_TILE) return false;
    if (chunks == 0) chunks = prdc_chunks_at(m, n, tile);
    return chunks >= 1 && chunks <= prdc_max_chunks(n, tile);
}

}  // namespace

extern "C" int gcc_prdc_tile(int m, int n) {
    if (m <= 0 || n <= 0) return 0;
    return prdc_tiles(m, GCC_PRDC_TILE) * prdc_max_chunks(n, GCC_PRDC_TILE) < GCC_PRDC_SMALL_BELOW ? GCC_PRDC_SMALL_TILE : GCC_PRDC_TILE;
}

extern "C" int gcc_prdc_chunks(int m, int n) {
    if (m <= 0 || n <= 0) return 0;
    return prdc_chunks_at(m, n, gcc_prdc_tile(m, n));
}

extern "C" size_t gcc_prdc_workspace(int m, int n, int k) {
    if (m <= 0 || n <= 0 || k < 1 || k > MAXK) return 0;
    return (size_t)m * (size_t)prdc_max_chunks(n, GCC_PRDC_SMALL_TILE) * (size_t)k * sizeof(double);
}

extern "C" int gcc_prdc_kth_dist(const void* X, int x_f64, int ldx, int m, const void* Y, int y_f64, int ldy, int n, int d,
                                 int symmetric, int k, int chunks, int tile, double* out, void* ws, size_t ws_bytes,
                                 gcc_stream_t stream) {
    GCC_ENTER();
    if (symmetric) { Y = X; y_f64 = x_f64; ldy = ldx; n = m; }       // Y is X: its own arguments are not read
    if (!X || !Y || !out || !ws || m <= 0 || n <= 0 || d <= 0 || ldx < d || ldy < d || k < 1 || k > MAXK ||
        k > (symmetric ? n - 1 : n) || !prdc_plan(m, n, tile, chunks))
        return GCC_ERR_BAD_ARG;
    const long grid = prdc_tiles(m, tile) * chunks;
    if (grid > 0x7fffffffL) return GCC_ERR_UNSUPPORTED;
    if (ws_bytes < (size_t)m * chunks * k * sizeof(double)) return GCC_ERR_WORKSPACE;
    PrdcArgs g = {X, Y, (long)ldx, (long)ldy, x_f64 != 0, y_f64 != 0, m, n, d, symmetric != 0, k, chunks, (int)prdc_tiles(n, tile),
                  nullptr, ws};
    const dim3 G((unsigned)grid), B(NT);
    if (tile == GCC_PRDC_TILE) {
        if (k == 1) hipLaunchKernelGGL((prdc_kth_kernel<GCC_PRDC_TILE, 1>), G, B, 0, (hipStream_t)stream, g);
        else hipLaunchKernelGGL((prdc_kth_kernel<GCC_PRDC_TILE, MAXK>), G, B, 0, (hipStream_t)stream, g);
    } else {
        if (k == 1) hipLaunchKernelGGL((prdc_kth_kernel<GCC_PRDC_SMALL_TILE, 1>), G, B, 0, (hipStream_t)stream, g);
        else hipLaunchKernelGGL((prdc_kth_kernel<GCC_PRDC_SMALL_TILE, MAXK>), G, B, 0, (hipStream_t)stream, g);
    }
    GCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(prdc_kth_merge_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const double*)ws, m, chunks, k, out);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_prdc_ball_count(const void* Q, int q_f64, int ldq, int m, const void* C, int c_f64, int ldc, int n, int d,
                                   const double* r2, int chunks, int tile, int* out, void* ws, size_t ws_bytes,
                                   gcc_stream_t stream) {
    GCC_ENTER();
    if (!Q || !C || !r2 || !out || !ws || m <= 0 || n <= 0 || d <= 0 || ldq < d || ldc < d || !prdc_plan(m, n, tile, chunks))
        return GCC_ERR_BAD_ARG;
    const long grid = prdc_tiles(m, tile) * chunks;
    if (grid > 0x7fffffffL) return GCC_ERR_UNSUPPORTED;
    if (ws_bytes < (size_t)m * chunks * sizeof(int)) return GCC_ERR_WORKSPACE;
    PrdcArgs g = {Q, C, (long)ldq, (long)ldc, q_f64 != 0, c_f64 != 0, m, n, d, 0, 0, chunks, (int)prdc_tiles(n, tile), r2, ws};
    const dim3 G((unsigned)grid), B(NT);
    if (tile == GCC_PRDC_TILE) hipLaunchKernelGGL(prdc_count_kernel<GCC_PRDC_TILE>, G, B, 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(prdc_count_kernel<GCC_PRDC_SMALL_TILE>, G, B, 0, (hipStream_t)stream, g);
    GCC_CHECK_LAUNCH();
    hipLaunchKernelGGL(prdc_count_merge_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const int*)ws, m, chunks, out);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
