// The SAGAN generator at the reference's own precision (engine.SaganGeneratorEngine.infer, precision 'fp32'): what its fp32 program
// needs beyond gcc_conv_eval_f32_unet (l2..l4 and `last`) and gcc_conv_eval_f32_act (the q | k | v convolutions).  All tensors are
// NHWC fp32; both kernels run on the f32-input matrix instructions, bit for bit k-ordered fmaf chains.
//
// gcc_attention_infer_f32    y = gamma softmax_j(q_i . k_j) v + x per image over N = H W positions (reference Self_Attn,
//   models/SAGAN.py:72-104), ONE launch, nothing written but y; the N x N matrices never exist.  The arithmetic contract:
//     s_ij   the fmaf chain over the C8 channels d = 0, 1, 2, ... of q_i[d] k_j[d], from 0 (v_mfma_f32_16x16x4_f32; the
//            channels are zero-padded to the kernel's power-of-two multiple of 4, which adds exact zeros)
//     m_i    max_j s_ij                                          (pass 1 over the keys)
//     p_ij   expf(s_ij - m_i), the device library's expf; s_ij is recomputed in pass 2 by the same instructions: the same bits
//     l_i    sum_j p_ij and  O_ic = sum_j p_ij v_jc              (pass 2), both fmaf chains from 0 on the matrix instruction --
//            l is the product of P with a column of ones -- in ONE order of the keys: the tiles of 16 keys ascending, inside
//            a tile key 4 g + r in the order r = 0..3 outer, g = 0..3 inner (0, 4, 8, 12, 1, 5, ...).  Keys beyond N enter as
//            p = 0 times v = 0.  The order depends on N alone: not on B, the grid, the query's tile or wave, C or the channel.
//     y_ic   fmaf(gamma, O_ic / l_i, x_ic), the division correctly rounded; O is never rescaled
//   A workgroup of four waves owns 16 WQ queries x 64 output channels of one image (wave: 16 queries x 16 WQ channels; WQ = 4, 2
//   or 1 is chosen so that small grids get more workgroups -- it moves no bit) and streams the K rows (pass 1) and the K and V rows
//   (pass 2) of 32 keys per step through LDS, double-buffered, one barrier per step.  No key split, no workspace, no atomics; no
//   workgroup waits for another.
//   Score tiles are computed transposed (keys x queries): accumulator register r of lane (g, lr) is s[query lr][key 4 g + r],
//   which is the A operand (row lr, k index g) of the P V instruction r whose B operand is V[key 4 g + r][channel lr] -- no
//   cross-lane movement; the accumulators of O and l come out as row = query 4 g + r, column = channel lr.
//   LDS rows: K [key][DKP (+ 4)] floats, V [key][64 + 4]: a wave's 64 one-float reads fall on 64 distinct banks.
// gcc_conv_eval_f32_z4       the generator's first layer, ConvTranspose2d(Z, C, 4) on a 1 x 1 map: the GEMM [N, Z] x [Z, 16 C] on
//   the shared fp32 tile (conv_f32_tile.hpp, its single order of K) with a gather and a store of its own: rows are the N latents,
//   columns (kh 4 + kw) C + c; the store applies scale[c] / shift[c] and the activation and writes pixel (n, kh, kw), channel c.
#include "conv_f32_tile.hpp"

namespace {

struct AttnF32Args {
    const float* qkv; int ldq, qoff, koff, voff;
    const float* x; int ldx;
    float* y; int ldy;
    const float* gamma;
    int B, N, C, C8;
};

constexpr int AF_KEYS = 32;          // keys per step: two score tiles
constexpr int AF_VST = 68;           // floats per LDS V row: 64 channels + 4 (row 4 g + r, 16 lanes: 4 x 16 distinct banks)

__device__ __forceinline__ f32x4 mma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// grid (ceil(N / (16 WQ)), ceil(C / 64), B).  DK4: channel quads of q and k (a power of two >= ceil(C8 / 4))
template <int DK4, int WQ>
__global__ __launch_bounds__(256) void attn_infer_f32_kernel(const AttnF32Args a) {
    constexpr int DKP = DK4 * 4, KST = DKP == 4 ? 4 : DKP + 4;      // 4 x odd dwords a row: 16 rows x 4 k on 64 distinct banks
    constexpr int NT = WQ;                                            // 16-channel tiles of a wave
    constexpr int KITEMS = AF_KEYS * DK4, KPER = (KITEMS + 255) / 256, VPER = AF_KEYS * 16 / 256;
    __shared__ __attribute__((aligned(16))) float Ks[2][AF_KEYS * KST];
    __shared__ __attribute__((aligned(16))) float Vs[2][AF_KEYS * AF_VST];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, N = a.N, C = a.C, C8 = a.C8;
    const int q0 = (blockIdx.x * WQ + wave % WQ) * 16, cb0 = blockIdx.y * 64, cw0 = cb0 + (wave / WQ) * NT * 16;
    const float* base = a.qkv + (size_t)b * N * a.ldq;

    float qf[DK4];
#pragma unroll
    for (int kk = 0; kk < DK4; kk++) {
        const int d = kk * 4 + g;
        qf[kk] = (q0 + lr < N && d < C8) ? base[(size_t)(q0 + lr) * a.ldq + a.qoff + d] : 0.f;
    }

    f32x4 kr[KPER], vr[VPER];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    auto load_k = [&](int t) {
#pragma unroll
        for (int i = 0; i < KPER; i++) {
            const int idx = tid + i * 256, key = t * AF_KEYS + idx / DK4, d = (idx % DK4) * 4;
            f32x4 v = zero;
            if (idx < KITEMS && key < N) {
                const float* p = base + (size_t)key * a.ldq + a.koff + d;
                if (d + 4 <= C8) v = *(const f32x4*)p;
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (d + j < C8) v[j] = p[j];
                }
            }
            kr[i] = v;
        }
    };
    auto store_k = [&](int buf) {
#pragma unroll
        for (int i = 0; i < KPER; i++) {
            const int idx = tid + i * 256;
            if (idx < KITEMS) *(f32x4*)&Ks[buf][(idx / DK4) * KST + (idx % DK4) * 4] = kr[i];
        }
    };
    auto load_v = [&](int t) {
#pragma unroll
        for (int i = 0; i < VPER; i++) {
            const int idx = tid + i * 256, key = t * AF_KEYS + (idx >> 4), c = cb0 + (idx & 15) * 4;
            vr[i] = (key < N && c < C) ? *(const f32x4*)(base + (size_t)key * a.ldq + a.voff + c) : zero;
        }
    };
    auto store_v = [&](int buf) {
#pragma unroll
        for (int i = 0; i < VPER; i++) {
            const int idx = tid + i * 256;
            *(f32x4*)&Vs[buf][(idx >> 4) * AF_VST + (idx & 15) * 4] = vr[i];
        }
    };
    // the transposed score tile h of the staged step: s[r] = q_(q0 + lr) . k_(16 h + 4 g + r)
    auto scores = [&](int buf, int h) {
        f32x4 s = zero;
        const float* kp = &Ks[buf][(h * 16 + lr) * KST + g];
#pragma unroll
        for (int kk = 0; kk < DK4; kk++) s = mma4(kp[kk * 4], qf[kk], s);
        return s;
    };

    const int nsteps = cdiv(N, AF_KEYS);
    // pass 1: the row maximum
    float m = -INFINITY;
    load_k(0);
    store_k(0);
    __syncthreads();
    for (int t = 0; t < nsteps; t++) {
        const int buf = t & 1;
        if (t + 1 < nsteps) load_k(t + 1);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const f32x4 s = scores(buf, h);
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (t * AF_KEYS + h * 16 + g * 4 + r < N) m = fmaxf(m, s[r]);
        }
        if (t + 1 < nsteps) store_k(buf ^ 1);
        __syncthreads();
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));               // the maximum of row q0 + lr over all keys

    // pass 2: l and O
    f32x4 L = zero, O[NT];
#pragma unroll
    for (int cb = 0; cb < NT; cb++) O[cb] = zero;
    load_k(0);
    load_v(0);
    store_k(0);
    store_v(0);
    __syncthreads();
    for (int t = 0; t < nsteps; t++) {
        const int buf = t & 1;
        if (t + 1 < nsteps) {
            load_k(t + 1);
            load_v(t + 1);
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const f32x4 s = scores(buf, h);
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; r++) p[r] = (t * AF_KEYS + h * 16 + g * 4 + r < N) ? expf(s[r] - m) : 0.f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                L = mma4(p[r], 1.f, L);
                const float* vp = &Vs[buf][(h * 16 + g * 4 + r) * AF_VST + (cw0 - cb0) + lr];
#pragma unroll
                for (int cb = 0; cb < NT; cb++)
                    if (cw0 + cb * 16 < C) O[cb] = mma4(p[r], vp[cb * 16], O[cb]);
            }
        }
        if (t + 1 < nsteps) {
            store_k(buf ^ 1);
            store_v(buf ^ 1);
        }
        __syncthreads();
    }

    // accumulator register r of lane (g, lr): query q0 + 4 g + r, channel (tile) + lr; L holds that query's l in every column
    const float gm = a.gamma[0];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int q = q0 + g * 4 + r;
        if (q >= N) continue;
        const size_t pix = (size_t)b * N + q;
#pragma unroll
        for (int cb = 0; cb < NT; cb++) {
            const int c = cw0 + cb * 16 + lr;
            if (c < C) a.y[pix * a.ldy + c] = fmaf(gm, O[cb][r] / L[r], a.x[pix * a.ldx + c]);
        }
    }
}

// the geometry's error, or 0
int af_geom(int B, int N, int C, int C8) {
    if (B <= 0 || B > 65535 || N <= 0 || N > 1024 || C <= 0 || C > 512 || C8 <= 0 || C8 > 64 || C8 > C || (C & 7)) return GCC_ERR_UNSUPPORTED;
    return 0;
}

// queries per workgroup / 16: 64-query workgroups once they fill the chip, else 32, else 16
int af_wq(int B, int N, int C) {
    const long long cols = (long long)cdiv(C, 64) * B;
    if (cdiv(N, 64) * cols >= 256) return 4;
    if (cdiv(N, 32) * cols >= 256) return 2;
    return 1;
}

template <int DK4>
void af_launch(const AttnF32Args& a, int wq, hipStream_t st) {
    const dim3 grid(cdiv(a.N, 16 * wq), cdiv(a.C, 64), a.B);
    if (wq == 4) hipLaunchKernelGGL((attn_infer_f32_kernel<DK4, 4>), grid, dim3(256), 0, st, a);
    else if (wq == 2) hipLaunchKernelGGL((attn_infer_f32_kernel<DK4, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_infer_f32_kernel<DK4, 1>), grid, dim3(256), 0, st, a);
}

// ---- the first layer ------------------------------------------------------------------------------------------------------
struct ConvF32Z4Args {
    const float* x; const float* w; float* y;
    const float* scale; const float* shift;        // NULL for the body: the store applies bscale / bshift per channel c, not per column
    const float* bscale; const float* bshift;
    int M, Co, Kp;                                 // M = N latents, Co = 16 C columns
    int Z, C, ldx, ldy, act;
    FastDiv dC;
};

// row m is latent m (one pixel of Z channels); k4 are its channels; column co = tap C + c goes to pixel 16 m + tap, channel c
#define CF_SETUP const float* wbase = a.w
#define CF_ROW(m, ih0, iw0, nb) ih0 = 0; iw0 = 0; nb = m
#define CF_TAP(k4) const bool kok = k4 < a.Z
#define CF_FETCH(v, ih0, iw0, nb) \
    if (kok && ih0 == 0) v = *(const f32x4*)(a.x + (size_t)nb * a.ldx + k4)
#define CF_NK (a.Kp / CF_BK)
#define CF_STORE_SETUP
#define CF_STORE(m, co, z)                                                                             \
    const int tap = fdiv(co, a.dC), c = co - tap * a.C;                                                \
    float v = fmaf(z, a.bscale ? a.bscale[c] : 1.f, a.bshift ? a.bshift[c] : 0.f);                     \
    if (a.act == GCC_EVAL_ACT_RELU) v = v < 0.f ? 0.f : v;                                             \
    a.y[((size_t)m * 16 + tap) * a.ldy + c] = v
template <int MI, int NI, int WM, int WN, bool UNUSED>
__global__ __launch_bounds__(CF_THREADS) void conv_f32_z4_kernel(ConvF32Z4Args a) {
#include "conv_f32_tile_body.inc"
}
#undef CF_SETUP
#undef CF_ROW
#undef CF_TAP
#undef CF_FETCH
#undef CF_NK
#undef CF_STORE_SETUP
#undef CF_STORE

inline int z4_kp(int Z) { return cf_kp(Z, 1); }

// the tile of a geometry (0: 128 x 128, 1: 64 x 64; 16 C >= 128 columns never take the 32-column tile), or its error
int z4_route(int N, int Z, int C) {
    if (N <= 0 || Z <= 0 || C <= 0) return GCC_ERR_BAD_ARG;
    if ((Z & 3) || (C & 7) || Z > (1 << 20) || C > 65536 || N > (1 << 24)) return GCC_ERR_UNSUPPORTED;
    return cf_tile(N, 16 * C);
}

}  // namespace

extern "C" int gcc_attention_infer_f32_route(int B, int N, int C, int C8) {
    const int bad = af_geom(B, N, C, C8);
    return bad ? bad : 1;
}

extern "C" int gcc_attention_infer_f32(const float* qkv, int ldq, int qoff, int koff, int voff, const float* x, int ldx,
                                       const float* gamma, int B, int N, int C, int C8, float* y, int ldy, gcc_stream_t stream) {
    GCC_ENTER();
    if (!qkv || !x || !gamma || !y) return GCC_ERR_BAD_ARG;
    const int bad = af_geom(B, N, C, C8);
    if (bad) return bad;
    if (ldq <= 0 || ldx <= 0 || ldy <= 0 || qoff < 0 || koff < 0 || voff < 0 || ((ldq | qoff | koff | voff | ldx | ldy) & 3)) return GCC_ERR_BAD_ARG;
    if (ldq < voff + C || ldq < qoff + C8 || ldq < koff + C8 || ldx < C || ldy < C) return GCC_ERR_BAD_ARG;
    if ((((uintptr_t)qkv) | ((uintptr_t)x) | ((uintptr_t)y)) & 15) return GCC_ERR_BAD_ARG;
    AttnF32Args a;
    a.qkv = qkv; a.ldq = ldq; a.qoff = qoff; a.koff = koff; a.voff = voff;
    a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.gamma = gamma;
    a.B = B; a.N = N; a.C = C; a.C8 = C8;
    const int wq = af_wq(B, N, C);
    hipStream_t st = (hipStream_t)stream;
    if (C8 <= 4) af_launch<1>(a, wq, st);
    else if (C8 <= 8) af_launch<2>(a, wq, st);
    else if (C8 <= 16) af_launch<4>(a, wq, st);
    else if (C8 <= 32) af_launch<8>(a, wq, st);
    else af_launch<16>(a, wq, st);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}

extern "C" int gcc_conv_eval_f32_z4_kp(int Z) {
    if (Z <= 0 || Z > (1 << 20)) return GCC_ERR_BAD_ARG;
    return z4_kp(Z);
}

extern "C" int gcc_conv_eval_f32_z4_route(int N, int Z, int C) { return z4_route(N, Z, C); }

extern "C" int gcc_conv_eval_f32_z4(const float* x, int ldx, const float* w, const float* scale, const float* shift, int act, int N,
                                    int Z, int C, float* y, int ldy, gcc_stream_t stream) {
    GCC_ENTER();
    if (!x || !w || !y) return GCC_ERR_BAD_ARG;
    if (act != GCC_EVAL_ACT_NONE && act != GCC_EVAL_ACT_RELU) return GCC_ERR_BAD_ARG;
    const int route = z4_route(N, Z, C);
    if (route < 0) return route;
    if (ldx <= 0 || ldy <= 0 || (ldx & 3) || (ldy & 3) || ldx < Z || ldy < C) return GCC_ERR_BAD_ARG;
    if ((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)y)) & 15) return GCC_ERR_BAD_ARG;
    ConvF32Z4Args a;
    a.x = x; a.w = w; a.y = y; a.scale = nullptr; a.shift = nullptr; a.bscale = scale; a.bshift = shift;
    a.M = N; a.Co = 16 * C; a.Kp = z4_kp(Z);
    a.Z = Z; a.C = C; a.ldx = ldx; a.ldy = ldy; a.act = act;
    a.dC = make_fastdiv(C);
    CF_LAUNCH_TILE(conv_f32_z4_kernel, false, a, 1, route, (hipStream_t)stream);
    GCC_CHECK_LAUNCH();
    return GCC_OK;
}
