// Body of the implicit-GEMM kernels of conv_igemm.hip (igemm_kernel, igemm_ex_kernel), included inside each definition so that
// every kernel compiles from the same text with its parameter `p` read straight from the kernel arguments.  In scope: the
// template parameters BP, BC, UT, NS and EPI, the epilogue kind (igemm_common.hpp IgemmEpiArgs): 0 bias / activation /
// statistics, 1 gcc_conv_fprop_eval's (IgemmEvParams.ev), 2 gcc_conv_eval_ex's (IgemmExParams.ex).
    using C = Cfg<BP, BC>;
    static_assert(NS == 2 || (UT && BP == 128 && (BC == 32 || BC == 64)), "deeper loops: uniform-tap 128 x {32, 64} tiles");
    constexpr int NT = C::NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sA = smem;                          // pixels  [NS][BP][128 B]
    char* sW = smem + NS * BP * BK * 2;       // weights [NS][BC][128 B]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: LDS-DMA bases stay scalar
    const int wc = wave % C::WC;
    const int wp = wave / C::WC;
#ifdef GCC_CLOCK_PROBE
    const unsigned long long pe0 = __builtin_amdgcn_s_memrealtime();
#endif

    // ---- per-phase geometry -----------------------------------------------------------------
    int py = 0, px = 0, Hg, Wg, sy, TA, TB, dy0, dx0, dstep, kh0, kw0, kstep, ostr;
    if (!p.dgrad) {
        Hg = p.Hd; Wg = p.Wd; sy = p.stride; TA = p.KH; TB = p.KW;
        dy0 = -p.pad; dx0 = -p.pad; dstep = 1; kh0 = 0; kw0 = 0; kstep = 1; ostr = 1;
    } else {
        const int s = p.stride;
        py = blockIdx.z / s; px = blockIdx.z % s;
        kh0 = (py + p.pad) % s; kw0 = (px + p.pad) % s;
        TA = (p.KH - kh0 + s - 1) / s; TB = (p.KW - kw0 + s - 1) / s;
        dy0 = (py + p.pad - kh0) / s; dx0 = (px + p.pad - kw0) / s;
        dstep = -1; kstep = s; sy = 1; ostr = s;
        Hg = (p.Hd - py + s - 1) / s; Wg = (p.Wd - px + s - 1) / s;
    }
    const int M = p.N * Hg * Wg;
    const int Ktot = TA * TB * p.Ct;
    const int nk_all = (Ktot + BK - 1) / BK;
    const int ks_idx = p.ksplit > 1 ? blockIdx.y : 0;
    const int kbeg = ks_idx * p.kper;
    const int nk = p.ksplit > 1 ? min(p.kper, nk_all - kbeg) : nk_all;

    const int nwg = gridDim.x;
    const int tile = xcd_remap(blockIdx.x, nwg);
    const int mt = tile / p.ntiles;
    const int nt = tile % p.ntiles;
    const int m0 = mt * BP;
    const int n0 = nt * BC;
    if (m0 >= M) {         // smaller phase (odd sizes): uniform exit, no barrier reached yet
        // pair split: both K halves of an empty tile land here; only half 0 counts (a full tile reaches the epilogue once,
        // through its second-arriving half, and make_tail's wgs_per_row = ntiles assumes one arrival per tile)
        if (p.stats && (!p.pair || blockIdx.y == 0)) {
            const int trow = blockIdx.z * p.mtiles_max + mt;
            if (tid < BC && n0 + tid < p.Cout) {
                st_stat(p.stats + ((size_t)trow * 2 + 0) * p.Cout + n0 + tid, 0.f, p.fin.tickets != nullptr);
                st_stat(p.stats + ((size_t)trow * 2 + 1) * p.Cout + n0 + tid, 0.f, p.fin.tickets != nullptr);
            }
            if (p.fin.tickets) stats_tail<NT>(p.fin, p.stats, p.Cout, trow, (int*)smem, tid);     // its row counts like any other
        }
        return;
    }

    const int bidx = p.ksplit > 1 ? 0 : blockIdx.y;
    const bf16_t* srcp = p.src + (size_t)bidx * p.src_bstride;
    const bf16_t* wgtp = p.wgt + (size_t)bidx * p.wgt_bstride;
    bf16_t* dstp = p.dst + (size_t)bidx * p.dst_bstride;
    const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc((void*)srcp, 0, p.src_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_wgt = __builtin_amdgcn_make_buffer_rsrc((void*)wgtp, 0, p.wgt_bytes, 0x00020000);

    // ---- per-thread gather rows (fixed 16-B chunk column) -----------------------------------
    // wave-instruction q = wave*4+i covers rows 8q..8q+7; lane -> row 8q + (lane>>3), physical chunk lane&7, which must
    // hold logical chunk (lane&7) ^ (row&7)
    const int chunk = (lane & 7) ^ (lane >> 3);
    constexpr int AI = C::AI;
    static_assert(AI <= 8, "pixel staging instructions per wave");
    int a_off[8], a_iy[8], a_ix[8];      // byte offset of the row's (iy0, ix0) pixel (+ chunk), and iy0 / ix0 (first AI used)
#pragma unroll
    for (int i = 0; i < AI; i++) {
        const int rloc = (wave * AI + i) * 8 + (lane >> 3);
        const int m = m0 + rloc;
        if (m < M) {
            const int n = m / (Hg * Wg);
            const int r = m - n * (Hg * Wg);
            const int oy = r / Wg;
            const int ox = r - oy * Wg;
            a_iy[i] = oy * sy + dy0;
            a_ix[i] = ox * sy + dx0;
            a_off[i] = (((n * p.Hs + a_iy[i]) * p.Ws + a_ix[i]) * p.lds_ + p.soff) * 2 + (UT ? chunk * 16 : 0);
        } else {
            a_off[i] = 0; a_iy[i] = -(1 << 28); a_ix[i] = 0;   // always out of range -> zeros
        }
    }
    // weight rows of this thread
    constexpr int WPW = C::WPW;                        // LDS-DMA weight instructions per wave (0: waves < WI issue one)
    constexpr int W_N = C::WN;
    int w_off[W_N];
    bool w_ok[W_N];
#pragma unroll
    for (int i = 0; i < W_N; i++) {
        const int row = n0 + (wave * (WPW > 0 ? WPW : 1) + i) * 8 + (lane >> 3);
        w_ok[i] = row < p.Cout;
        w_off[i] = row * p.ldw * 2 + (UT ? chunk * 16 : 0);
    }

    // K walk without divisions: (ta, tb) = tap coordinates, cc = channel offset inside the tap.
    // UT (Ct % 64 == 0): one tap per k-step, wave-uniform state (scalar registers);
    // otherwise every thread walks the tap of its own 8-channel chunk.
    const int tap_row_bytes = p.Ws * p.lds_ * 2 * dstep;   // bytes per +1 in `ta`
    const int tap_col_bytes = p.lds_ * 2 * dstep;          // bytes per +1 in `tb`
    int ta, tb, cc;
    {
        const int k0 = kbeg * BK + (UT ? 0 : chunk * 8);
        const int tap0 = k0 / p.Ct;
        cc = k0 - tap0 * p.Ct;
        ta = tap0 / TB;
        tb = tap0 - ta * TB;
    }

    // issue the global loads of the next k-step (in order), straight into LDS stage `stage`
    auto issue_loads = [&](int stage) {
        const bool kval = ta < TA;
        const int dyo = ta * dstep, dxo = tb * dstep;
        const int pix_off = ta * tap_row_bytes + tb * tap_col_bytes + cc * 2;
        const int wt_off = (((kh0 + ta * kstep) * p.KW + (kw0 + tb * kstep)) * p.Ct + cc) * 2;
#pragma unroll
        for (int i = 0; i < AI; i++) {
            const bool ok = kval && (unsigned)(a_iy[i] + dyo) < (unsigned)p.Hs && (unsigned)(a_ix[i] + dxo) < (unsigned)p.Ws;
            const uint32_t off = ok ? (uint32_t)(a_off[i] + pix_off) : OOB;
            char* dst = sA + stage * (BP * BK * 2) + (wave * AI + i) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_src, LDS_PTR(void, dst), 16, off, 0, 0, 0);
        }
        if (WPW > 0 || wave < C::WI) {       // wave-uniform
#pragma unroll
            for (int i = 0; i < W_N; i++) {
                const uint32_t off = (kval && w_ok[i]) ? (uint32_t)(w_off[i] + wt_off) : OOB;
                char* dst = sW + stage * (BC * BK * 2) + (wave * (WPW > 0 ? WPW : 1) + i) * 1024;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_wgt, LDS_PTR(void, dst), 16, off, 0, 0, 0);
            }
        }
        // advance to the next k-step
        cc += BK;
        if constexpr (UT) {
            if (cc == p.Ct) { cc = 0; if (++tb == TB) { tb = 0; ++ta; } }
        } else {
            while (cc >= p.Ct) { cc -= p.Ct; if (++tb == TB) { tb = 0; ++ta; } }
        }
    };

    f32x4 acc[C::CB][C::PB];
#pragma unroll
    for (int i = 0; i < C::CB; i++)
#pragma unroll
        for (int j = 0; j < C::PB; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int lr = lane & 15;
    const int lq = lane >> 4;
    auto compute = [&](int cur) {
        const char* a = sA + cur * (BP * BK * 2);
        const char* w = sW + cur * (BC * BK * 2);
        // Both k-slices (2 x 32) of the stage are held in registers: the fragment reads of slice 1 are issued while
        // the MFMAs of slice 0 run (the compiler's own order reads two fragments, waits, issues four MFMAs -- LDS
        // latency exposed at every group).  sched_group_barrier pins the interleave: all reads of slice 0, then one
        // read of slice 1 per MFMA_PER_READ MFMAs, then the rest.
        bf16x8 fw[2][C::CB], fa[2][C::PB];
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
#pragma unroll
            for (int i = 0; i < C::CB; i++) {
                const int row = wc * C::TC + i * 16 + lr;
                fw[ks][i] = *(const bf16x8*)(w + row * 128 + (((ks * 4 + lq) ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < C::PB; j++) {
                const int row = wp * C::TP + j * 16 + lr;
                fa[ks][j] = *(const bf16x8*)(a + row * 128 + (((ks * 4 + lq) ^ (row & 7)) << 4));
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int i = 0; i < C::CB; i++)
#pragma unroll
                for (int j = 0; j < C::PB; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[ks][i], fa[ks][j], acc[i][j], 0, 0, 0);
        constexpr int READS = C::CB + C::PB;                 // fragment reads per k-slice
        constexpr int MFMAS = C::CB * C::PB;                 // MFMAs per k-slice
        constexpr int MPR = MFMAS / READS > 0 ? MFMAS / READS : 1;
        __builtin_amdgcn_sched_group_barrier(0x100, READS, 0);          // slice 0 fragments
#pragma unroll
        for (int r = 0; r < READS; r++) {
            __builtin_amdgcn_sched_group_barrier(0x008, MPR, 0);        // MFMAs of slice 0 ...
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);          // ... covering one read of slice 1
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 2 * MFMAS - READS * MPR, 0);
    };

    if constexpr (UT) {
        // Uniform-tap fast path: a tap spans Ct/64 consecutive k-steps, so the per-row source offsets
        // (bounds checks included) are computed once per tap and then just advance by 128 bytes per
        // k-step; the loop body is 8 LDS-DMA + 8 adds + 16 ds_read + 32 MFMA per wave.
        static_assert(C::WN <= 8, "weight staging instructions per wave");
        uint32_t cur_a[8], cur_w[8];   // literal bound on purpose: with a template-dependent bound hipcc (ROCm 7.2)
                                       // silently drops the host stub of this instantiation
        int left;                                  // k-steps left in the current tap (scalar)
        auto load_tap = [&]() {
            const bool kval = ta < TA;
            const int dyo = ta * dstep, dxo = tb * dstep;
            const int pix_off = ta * tap_row_bytes + tb * tap_col_bytes + cc * 2;
            const int wt_off = (((kh0 + ta * kstep) * p.KW + (kw0 + tb * kstep)) * p.Ct + cc) * 2;
#pragma unroll
            for (int i = 0; i < AI; i++) {
                const bool ok = kval && (unsigned)(a_iy[i] + dyo) < (unsigned)p.Hs && (unsigned)(a_ix[i] + dxo) < (unsigned)p.Ws;
                cur_a[i] = ok ? (uint32_t)(a_off[i] + pix_off) : OOB;
            }
#pragma unroll
            for (int i = 0; i < W_N; i++) cur_w[i] = (kval && w_ok[i]) ? (uint32_t)(w_off[i] + wt_off) : OOB;
            left = (p.Ct - cc) / BK;
        };
        auto issue = [&](int stage, bool pixels = true) {
#pragma unroll
            for (int i = 0; i < AI; i++) {
                char* dst = sA + stage * (BP * BK * 2) + (wave * AI + i) * 1024;
                if (pixels) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_src, LDS_PTR(void, dst), 16, cur_a[i], 0, 0, 0);
                cur_a[i] += BK * 2;
            }
            if (WPW > 0 || wave < C::WI) {
#pragma unroll
                for (int i = 0; i < W_N; i++) {
                    char* dst = sW + stage * (BC * BK * 2) + (wave * (WPW > 0 ? WPW : 1) + i) * 1024;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_wgt, LDS_PTR(void, dst), 16, cur_w[i], 0, 0, 0);
                    cur_w[i] += BK * 2;
                }
            }
        };
        auto next_step = [&]() {
            if (--left == 0) {                      // wave-uniform, once per tap
                cc = 0;
                if (++tb == TB) { tb = 0; ++ta; }
                load_tap();
            }
        };
#ifdef GCC_CLOCK_PROBE
        const unsigned long long pt0 = __builtin_amdgcn_s_memtime(), pr0 = __builtin_amdgcn_s_memrealtime();
#endif
        if constexpr (NS > 2) {
            // NS - 1 k-steps in flight.  LDS-DMA from inline assembly (lds_dma16): through the builtin hipcc would put
            // s_waitcnt vmcnt(0) in front of the fragment reads of the stage being multiplied (it counts a pending DMA as an LDS
            // write it cannot prove disjoint) and drain the steps behind it; here the counted wait + barrier below order the data.
            constexpr int PER_STEP = AI + W_N;                     // DMA instructions per wave and k-step (uniform for BC 32 / 64)
            static_assert(C::WPW > 0, "every wave stages weights");
            const i32x4 rsv_src = make_rsrc(srcp, p.src_bytes), rsv_wgt = make_rsrc(wgtp, p.wgt_bytes);
            const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(char, smem);
            auto issue_n = [&](int stage) {
#pragma unroll
                for (int i = 0; i < AI; i++) {
                    lds_dma16(rsv_src, lds0 + stage * (BP * BK * 2) + (wave * AI + i) * 1024, cur_a[i]);
                    cur_a[i] += BK * 2;
                }
#pragma unroll
                for (int i = 0; i < W_N; i++) {
                    lds_dma16(rsv_wgt, lds0 + NS * BP * BK * 2 + stage * (BC * BK * 2) + (wave * WPW + i) * 1024, cur_w[i]);
                    cur_w[i] += BK * 2;
                }
            };
            load_tap();
#pragma unroll
            for (int st = 0; st < NS - 1; st++) { issue_n(st); next_step(); }
            int stage = 0, fill = NS - 1;                          // stage of step kt; stage the next issue goes to
            for (int kt = 0; kt < nk; kt++) {
                // step kt has landed once at most the NS - 2 younger steps are outstanding (vmcnt counts in issue order)
                if constexpr (NS == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER_STEP) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER_STEP) : "memory");
                __syncthreads();                                     // ... for every wave, and everyone left the stage of step kt - 1
                issue_n(fill);                                       // past the end of K: out-of-range offsets, zero fill, unused
                next_step();
                compute(stage);
                stage = stage + 1 == NS ? 0 : stage + 1;
                fill = fill + 1 == NS ? 0 : fill + 1;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        } else {
        load_tap();
        issue(0);
        next_step();
#if GCC_IGEMM_ROT
        // The k loop rotated by half a step: the barrier sits between the two 32-deep k-slices of a stage, so that the
        // fragment reads that follow it (slice 0 of the NEXT stage) run under the MFMAs of slice 1 instead of in front of
        // the step's first MFMA -- with the barrier at the top of the step both waves of a SIMD wait for their first twelve
        // ds_read_b128 at the same time and the matrix pipe idles (in-kernel clock stamps, profiles/r03_l_*: 72 % busy).
        //   A: MFMAs of slice 0 | reads of slice 1 (stage s)         -> nobody reads stage s any more
        //   B: my DMA of stage s^1 landed; barrier                     -> everybody's has, stage s is free
        //   C: DMA of step kt+2 into stage s
        //   D: MFMAs of slice 1 | reads of slice 0 of stage s^1
        // A DMA issued at C is waited for at B of the next step: one full step in flight, as before.
        bf16x8 f0w[C::CB], f0a[C::PB], f1w[C::CB], f1a[C::PB];
        auto read_slice = [&](int stage, int ks, bf16x8 (&fw)[C::CB], bf16x8 (&fa)[C::PB]) {
            const char* a = sA + stage * (BP * BK * 2);
            const char* w = sW + stage * (BC * BK * 2);
#pragma unroll
            for (int i = 0; i < C::CB; i++) {
                const int row = wc * C::TC + i * 16 + lr;
                fw[i] = *(const bf16x8*)(w + row * 128 + (((ks * 4 + lq) ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < C::PB; j++) {
                const int row = wp * C::TP + j * 16 + lr;
                fa[j] = *(const bf16x8*)(a + row * 128 + (((ks * 4 + lq) ^ (row & 7)) << 4));
            }
        };
        auto mfma_slice = [&](const bf16x8 (&fw)[C::CB], const bf16x8 (&fa)[C::PB]) {
#pragma unroll
            for (int i = 0; i < C::CB; i++)
#pragma unroll
                for (int j = 0; j < C::PB; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[i], fa[j], acc[i][j], 0, 0, 0);
        };
        constexpr int R_READS = C::CB + C::PB, R_MFMAS = C::CB * C::PB;
        constexpr int R_MPR = R_MFMAS / R_READS > 0 ? R_MFMAS / R_READS : 1;
        auto pin = [&]() {                          // one fragment read per R_MPR MFMAs, then the remaining MFMAs
#pragma unroll
            for (int r = 0; r < R_READS; r++) {
                __builtin_amdgcn_sched_group_barrier(0x008, R_MPR, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, R_MFMAS - R_READS * R_MPR > 0 ? R_MFMAS - R_READS * R_MPR : 0, 0);
        };
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        issue(1);                                   // past the end of K the offsets are out of range: zero fill, unused
        next_step();
        read_slice(0, 0, f0w, f0a);
        for (int kt = 0; kt < nk; kt++) {
            const int cur = kt & 1;
            read_slice(cur, 1, f1w, f1a);
            mfma_slice(f0w, f0a);
            pin();
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __syncthreads();
            issue(cur);
            next_step();                            // (rare) tap change: its VALU work hides under the MFMAs below
            __builtin_amdgcn_sched_barrier(0);
            read_slice(cur ^ 1, 0, f0w, f0a);       // the last step reads a stage nobody uses
            mfma_slice(f1w, f1a);
            pin();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#else
        for (int kt = 0; kt < nk; kt++) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (!(GCC_DIAG(p.debug) & 2)) {
                issue((kt + 1) & 1, !(GCC_DIAG(p.debug) & 8) || (kt & 3) == 0);    // past the end of K the offsets are out of range: zero fill, unused
                if (!(GCC_DIAG(p.debug) & 4)) next_step();    // (rare) tap change: its VALU work hides under the MFMAs below
                else {
#pragma unroll
                    for (int i = 0; i < AI; i++) cur_a[i] -= BK * 2;
#pragma unroll
                    for (int i = 0; i < W_N; i++) cur_w[i] -= BK * 2;
                }
            }
            compute(kt & 1);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#endif
        }
#ifdef GCC_CLOCK_PROBE
        {
            const unsigned long long pt1 = __builtin_amdgcn_s_memtime(), pr1 = __builtin_amdgcn_s_memrealtime();
            const unsigned b = blockIdx.z * gridDim.x + blockIdx.x;
            if (tid == 0 && b < 4096) {
                g_clock_probe[b][0] = pt1 - pt0; g_clock_probe[b][1] = pr1 - pr0; g_clock_probe[b][2] = (unsigned long long)nk;
                g_clock_probe[b][3] = 1;
                g_clock_probe[b][4] = pe0; g_clock_probe[b][5] = pr0; g_clock_probe[b][6] = pr1;
            }
        }
#endif
    } else {
        // one barrier per k-step: [tile kt landed for every wave AND everyone left tile kt-1] ->
        // issue tile kt+1 into the buffer tile kt-1 occupied -> compute tile kt while it flies
#ifdef GCC_CLOCK_PROBE
        const unsigned long long qr0 = __builtin_amdgcn_s_memrealtime();
#endif
        issue_loads(0);
        for (int kt = 0; kt < nk; kt++) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (kt + 1 < nk) issue_loads((kt + 1) & 1);
            compute(kt & 1);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#ifdef GCC_CLOCK_PROBE
        {
            const unsigned long long qr1 = __builtin_amdgcn_s_memrealtime();
            const unsigned b = blockIdx.z * gridDim.x + blockIdx.x;
            if (tid == 0 && b < 4096) {
                g_clock_probe[b][0] = 0; g_clock_probe[b][1] = qr1 - qr0; g_clock_probe[b][2] = (unsigned long long)nk;
                g_clock_probe[b][3] = 1;
                g_clock_probe[b][4] = pe0; g_clock_probe[b][5] = qr0; g_clock_probe[b][6] = qr1;
            }
        }
#endif
    }

    if constexpr (BP == 256 && BC == 256) {
        if (p.pair) {
            // Two workgroups own this tile, one per K half (in-launch split-K hand-off, cdna_hip_programming.md Guideline 16,
            // recipe R1): write-through (sc1) slab stores, every storing wave drains, one lane publishes the flag; the other
            // half polls that one word, one agent-scope acquire, sc1 slab loads.  a + b == b + a: the result does not
            // depend on which half arrives first.
            typedef __attribute__((address_space(1))) unsigned int gu32;
            const int tile_id = (int)(blockIdx.z * gridDim.x + blockIdx.x);
            gu32* fl = (gu32*)(p.pair_flags + 2 * tile_id);
            int* sh = (int*)smem;                           // the loop's LDS is free: every wave passed its last barrier
            if (tid == 0) sh[0] = (int)__hip_atomic_fetch_add(fl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            const int ticket = sh[0];
            __syncthreads();
            const __amdgpu_buffer_rsrc_t rs_slab =
                __builtin_amdgcn_make_buffer_rsrc((void*)(p.pair_slab + (size_t)tile_id * (BP * BC)), 0, BP * BC * 4, 0x00020000);
            if (ticket == 0) {
#pragma unroll
                for (int i = 0; i < C::CB; i++)
#pragma unroll
                    for (int j = 0; j < C::PB; j++)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, acc[i][j]), rs_slab,
                                                               ((i * C::PB + j) * NT + tid) * 16, 0, 16);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) __hip_atomic_store(fl + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            if (tid == 0) {
                while (__hip_atomic_load(fl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) __builtin_amdgcn_s_sleep(4);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < C::CB; i++)
#pragma unroll
                for (int j = 0; j < C::PB; j++) {
                    const f32x4 o = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_slab, ((i * C::PB + j) * NT + tid) * 16, 0, 16));
                    acc[i][j] += o;
                }
        }
    }
    igemm_epilogue<C, BP, BC, EPI>(p, acc, smem, tid, lr, lq, wc, wp, m0, n0, M, Hg, Wg, ostr, py, px, mt, ks_idx, dstp);
#ifdef GCC_CLOCK_PROBE
    {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned b = blockIdx.z * gridDim.x + blockIdx.x;
        if (tid == 0 && b < 4096) g_clock_probe[b][7] = __builtin_amdgcn_s_memrealtime();
    }
#endif
