// The body of the fp32 conv kernels (conv_f32_tile.hpp describes the tile), included inside each __global__ definition so that every
// kernel compiles from this one text with its parameter `a` read straight from the kernel arguments (the idiom of
// igemm_kernel_body.inc).  In scope: MI, NI, WM, WN; `a` with x, scale, shift, M, Co, Kp among its fields; and the kernel's own
// pieces as macros, #undef'd by the kernel behind the #include --
//   CF_SETUP                    declare `const float* wbase` (the packed weights of this workgroup) and what the pieces below share
//   CF_ROW(m, ih0, iw0, nb)     Gather: decode row m < M into what CF_FETCH wants back
//   CF_TAP(k4)                  Gather: once per thread per k step, declare the decoded tap dh, dw, ci and kok (k4 is a real k)
//   CF_FETCH(v, ih0, iw0, nb)   Gather: v (zeros on entry) = the 4 floats of that row and tap where there is something to read
//   CF_NK                       the number of k steps
//   CF_STORE_SETUP              Store: what a thread reads once before its stores
//   CF_STORE(m, co, z)          Store: write the activated z = fmaf(acc, scale, shift) of row m < M, channel co < Co
// The body does not know which entry it serves.
    static_assert(WM * WN == 4, "four waves");
    constexpr int BM = WM * MI * 32, BN = WN * NI * 32;
    constexpr int A_PER = BM * 4 / CF_THREADS, B_PER = (BN * 4 + CF_THREADS - 1) / CF_THREADS;
    __shared__ __attribute__((aligned(16))) float As[2][BM * CF_LDK];
    __shared__ __attribute__((aligned(16))) float Bs[2][BN * CF_LDK];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int chunk = t & 3;                        // the thread's 4 floats of a 16-float k step, for its A rows and its B rows
    CF_SETUP;

    // the thread's A rows; a row beyond M never passes a gather's range test
    int ih0[A_PER], iw0[A_PER], nb[A_PER];
#pragma unroll
    for (int i = 0; i < A_PER; i++) {
        const int m = m0 + ((t + i * CF_THREADS) >> 2);
        if (m < a.M) {
            CF_ROW(m, ih0[i], iw0[i], nb[i]);
        } else {
            ih0[i] = -(1 << 28); iw0[i] = 0; nb[i] = 0;
        }
    }
    const float* wrow[B_PER];
#pragma unroll
    for (int i = 0; i < B_PER; i++) {
        const int idx = t + i * CF_THREADS, co = n0 + (idx >> 2);
        wrow[i] = (idx < BN * 4 && co < a.Co) ? wbase + (size_t)co * a.Kp + chunk * 4 : nullptr;
    }

    f32x4 ra[A_PER], rb[B_PER];
    auto load = [&](int kt) {
        const int k4 = kt * CF_BK + chunk * 4;
        CF_TAP(k4);
#pragma unroll
        for (int i = 0; i < A_PER; i++) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            CF_FETCH(v, ih0[i], iw0[i], nb[i]);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < B_PER; i++) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (wrow[i]) v = *(const f32x4*)(wrow[i] + kt * CF_BK);
            rb[i] = v;
        }
    };
    auto stage = [&](int s) {
#pragma unroll
        for (int i = 0; i < A_PER; i++) *(f32x4*)&As[s][((t + i * CF_THREADS) >> 2) * CF_LDK + chunk * 4] = ra[i];
#pragma unroll
        for (int i = 0; i < B_PER; i++) {
            const int idx = t + i * CF_THREADS;
            if (idx < BN * 4) *(f32x4*)&Bs[s][(idx >> 2) * CF_LDK + chunk * 4] = rb[i];
        }
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
        for (int ni = 0; ni < NI; ni++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[mi][ni][r] = 0.f;

    const int nk_ = CF_NK;
    const int arow = (wm * MI * 32 + (lane & 31)) * CF_LDK + (lane >> 5) * 4;
    const int brow = (wn * NI * 32 + (lane & 31)) * CF_LDK + (lane >> 5) * 4;
    load(0);
    stage(0);
    __syncthreads();
    for (int kt = 0; kt < nk_; kt++) {
        const int cur = kt & 1;
        if (kt + 1 < nk_) load(kt + 1);
#pragma unroll
        for (int g = 0; g < 2; g++) {
            f32x4 af[MI], bf[NI];
#pragma unroll
            for (int mi = 0; mi < MI; mi++) af[mi] = *(const f32x4*)&As[cur][arow + mi * 32 * CF_LDK + g * 8];
#pragma unroll
            for (int ni = 0; ni < NI; ni++) bf[ni] = *(const f32x4*)&Bs[cur][brow + ni * 32 * CF_LDK + g * 8];
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int mi = 0; mi < MI; mi++)
#pragma unroll
                    for (int ni = 0; ni < NI; ni++)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mi][e], bf[ni][e], acc[mi][ni], 0, 0, 0);
        }
        if (kt + 1 < nk_) stage(cur ^ 1);
        __syncthreads();
    }

    // epilogue: only rows < M and channels < Co are touched
    CF_STORE_SETUP;
#pragma unroll
    for (int ni = 0; ni < NI; ni++) {
        const int co = n0 + (wn * NI + ni) * 32 + (lane & 31);
        if (co >= a.Co) continue;
        const float sc = a.scale ? a.scale[co] : 1.f, sh = a.shift ? a.shift[co] : 0.f;
#pragma unroll
        for (int mi = 0; mi < MI; mi++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = m0 + (wm * MI + mi) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m >= a.M) continue;
                CF_STORE(m, co, fmaf(acc[mi][ni][r], sc, sh));
            }
        }
    }
