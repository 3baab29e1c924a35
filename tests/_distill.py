"""Data, float64 references, per-element bounds, the case table and a CPU emulation for the distillation loss (misc.hip
gcc_distill_fwd / gcc_distill_bwd), shared by tests/test_distill_exact_gpu.py and tests/test_distill_bounds_cpu.py (no tests here).

Distillation is the one caller of the BATCHED weight gradient and 1x1 product (gcc_internal_wgrad / gcc_internal_igemm with
batch = N > 1: problems on grid.y, per-problem strides, the [splits][batch][Co][cols] slabs and their fold, plan_splits(c, batch),
select_tile(..., batch)).  Its five kernels' results are kept in the call's workspace, so each stage is compared with a float64
reference computed FROM THE VALUES THAT STAGE READ on the device, and an error is pinned to one kernel:

  stage 1  Gf, Gt   fp32 [N][C][C], G_n = F_n^T F_n over the HW pixels (wgrad_kernel, batch = N; + wgrad_reduce_flat / _vec)
           'int' data: the exact integers, bit for bit.  'normal': |err| <= bound_wgrad(|F|^T |F|, M = HW, S = pixel splits)
  stage 2  S        bf16 [N][C][C] = f2bf(fp32(fp32(gf - gt) * fp32(1 / (C HW)))), bit for bit from the device's Gf, Gt
  stage 3  scal     Lg = [sqrt] mean D^2 over N C C entries, Lc = [sqrt] mean (f - t)^2 over N HW C entries.  Every term is >= 0, so
           |sum_dev - sum| <= (term + depth) 2^-24 sum: `term` roundings inside a term, `depth` additions on the longest path to the
           total (gram_depth / content_depth count them from the code).  One rounding of the quotient; the RMSE form halves the
           relative error under the root and adds the device sqrtf's (1 ulp = 2^-23, HIP math API).  out2 == scal[0:2] bit for bit
  stage 4  dfg      bf16 [N][HW][C] = f_n . S_n (igemm_kernel, batch = N).  C HW a power of two and 'int' data: S is a multiple of
           1 / (C HW), every partial sum exact in fp32 (asserted), dfg == expected_bits(exact).  Otherwise bound_out(K = C, S = 1)
  stage 5  df       bf16 = kg dfg + kc (f - t) from the device's dfg and scal:
           |err| <= BF16 |ref| + K_COMBINE 2^-24 (|kg dfg| + |kc (f - t)|)
  stage 6  end to end against float64 autograd of oracle.gcc_oracle.gram / rmse / F.mse_loss ('normal' data), per element:
           dD  = (bound_wgrad(|F|^T|F|) + bound_wgrad(|T|^T|T|)) / (C HW) + 3 2^-24 |D|     the Gram products' fp32 error through 1 / (C HW)
           dS  = dD + 2^-8 (|D| + dD)                                                     ... and the rounding of S to bf16
           A   = |f| . dS + (C + 5) 2^-24 |f| . (|D| + dS)                                the 1x1 product of the perturbed S in fp32
           dG  = A + 2^-8 (|f . D| + A)                                                   the rounding of dfg
           eg, ec = relative errors of kg, kc: the casts and the division (3 2^-24) and, RMSE form, those of Lg and Lc:
                    eLg = rms(dD) / Lg + stage 3's relative bound (the norm's triangle inequality; Lg's OWN bound, not the tensor's), eLc = stage 3's
           |df - ref| <= BF16 |ref| + (1 + 2^-7) [ kg dG + eg kg (|f . D| + dG) + ec kc |f - t| + 3 2^-24 (kg |f . D| + kc |f - t|) ]
           with kg 2^-8 sum_c' |f_pc'| |D_c'c| -- the rounding of S -- its largest term by two orders of magnitude.

Tensors here are float64 on the CPU, features [N, HW, C]; every value is bf16-representable."""
import math

import torch
import torch.nn.functional as F

from tests._conv_exact import EXACT_LIMIT, bound_out, bound_wgrad, cdiv, expected_bits
from tests._perelem import BF16, RND_BF16, U24, rb64, within

WG, WC = 1e4, 50.0               # the weights of tests/test_kernels_gpu.py::test_distill_loss (both exact in fp32)
SENTINEL = -768.0                # bf16-exact; what every lane outside a window holds
WIN_OFF, WIN_EXTRA = 8, 16       # windows: lane 8 of buffers 16 lanes wider

# ---- constants restated from the sources (a changed one shows as a named difference in tests/test_distill_bounds_cpu.py) ---------
TP = 64                          # conv_wgrad.hip: pixels per k-step
PLAN_WGRAD_WGS = 512             # common.hpp
RED_BLOCKS = 1024                # misc.hip


def al256(v):
    return (v + 255) & ~255


def plan_splits_py(C, HW, batch):
    """conv_wgrad.hip plan_splits for the 1x1 Gram product of one image (never `big`: that needs 8 tiles of 256 x 256 at batch 1)"""
    ksteps = cdiv(HW, TP)
    tiles = cdiv(C, 128) * cdiv(C, 128) * batch
    splits = 1 if tiles >= PLAN_WGRAD_WGS * 3 // 8 else cdiv(PLAN_WGRAD_WGS, tiles)
    splits = max(1, min(splits, max(1, ksteps // 8)))
    per = cdiv(ksteps, splits)
    return cdiv(ksteps, per), per


def select_tile_py(C, HW, batch):
    """conv_igemm.hip select_tile for the 1x1 product [HW, C] x [C, C] (nk = ceil(C / 64) < PLAN_BIG_NK: no 256-pixel tiles)"""
    BC = 128 if C > 64 else 64 if C > 32 else 32 if C > 16 else 16
    ntiles = cdiv(C, 128) if C > 64 else 1
    if batch == 1 and BC > 32 and cdiv(C, 64) <= 64:
        mt, bc = cdiv(HW, 128), BC
        while bc > 32 and mt * cdiv(C, bc) < 256:
            bc >>= 1
        if mt * cdiv(C, bc) >= 256:
            BC, ntiles = bc, cdiv(C, bc)
    return 128, BC, ntiles, cdiv(HW, 128)


def plan_py(N, C, HW):
    """gcc_distill_plan restated: the names of gcc_amd._lib.DISTILL_PLAN"""
    splits, kper = plan_splits_py(C, HW, N)
    fold = 0 if splits == 1 else (1 if splits <= 8 else 2)
    BP, BC, ntiles, mtiles = select_tile_py(C, HW, N)
    o = al256(16 * 4)
    p = dict(off_scal=0)
    o = al256(o + 2 * RED_BLOCKS * 4)
    p['off_gf'] = o
    o = al256(o + N * C * C * 4)
    p['off_gt'] = o
    o = al256(o + N * C * C * 4)
    p['off_s'] = o
    o = al256(o + N * C * C * 2)
    p['off_dfg'] = o
    o = al256(o + N * HW * C * 2)
    p['ws_bytes'] = al256(o + splits * N * C * C * 4)
    p.update(gram_splits=splits, gram_kper=kper, gram_col_tiles=cdiv(C, 128), gram_co_tiles=cdiv(C, 128), gram_fold=fold, bwd_route=0,
             bwd_bp=BP, bwd_bc=BC, bwd_ntiles=ntiles, bwd_mtiles=mtiles, fwd_launches=2 * (1 if fold == 0 else 2) + 4, bwd_launches=2)
    return p


# ---- cases: the smallest shapes that reach each form under the default plan, worked out by hand ---------------------------------
def _case(N, C, HW, splits, kper, fold, tiles, bc, ntiles, mtiles, win=False, tern=False):
    return dict(name='%dx%dx%d' % (N, C, HW), N=N, C=C, HW=HW, win=win, tern=tern,
                expect=dict(gram_splits=splits, gram_kper=kper, gram_fold=fold, gram_col_tiles=tiles, gram_co_tiles=tiles, bwd_route=0,
                            bwd_bp=128, bwd_bc=bc, bwd_ntiles=ntiles, bwd_mtiles=mtiles, fwd_launches=6 if fold == 0 else 8,
                            bwd_launches=2))


CASES = (
    _case(3, 8, 64, 1, 1, 0, 1, 16, 1, 1),                     # direct write, odd batch; BC 16, half a pixel tile; C HW = 2^9
    _case(2, 24, 25, 1, 1, 0, 1, 32, 1, 1, win=True),          # one ragged tile of 25 rows, in windows
    _case(2, 32, 32, 1, 1, 0, 1, 32, 1, 1),                    # C HW = 2^10
    _case(2, 64, 256, 1, 4, 0, 1, 64, 1, 2),                   # BC 64, two full tiles; C HW = 2^14
    _case(2, 128, 128, 1, 2, 0, 1, 128, 1, 1),                 # BC 128; C HW = 2^14
    _case(2, 136, 200, 1, 4, 0, 2, 128, 2, 2),                 # 2 x 2 Gram tiles, the last 8 wide; 3 k-steps of K, the last of 8; last 72 rows
    _case(2, 8, 1024, 2, 8, 1, 1, 16, 1, 8),                   # 2 pixel splits, flat fold; C HW = 2^13
    _case(2, 40, 1100, 2, 9, 1, 1, 64, 1, 9, win=True),        # 2 splits of 9 k-steps, last k-step of 12 pixels; last tile 76 rows
    _case(2, 8, 4700, 9, 9, 2, 1, 16, 1, 37),                  # 9 splits (> 8: vec fold), the last of 2 k-steps
    _case(1, 8, 300, 1, 5, 0, 1, 16, 1, 3),                    # batch 1 (CycleGAN): the ordinary dispatch
    _case(1, 256, 8192, 16, 8, 2, 2, 64, 4, 64, tern=True),    # batch 1: 16 splits, vec fold; the nk <= 64 narrowing; C HW = 2^21
)
CASE_IDS = [c['name'] for c in CASES]
PLAN_KEYS = tuple(CASES[0]['expect'])


def pow2(v):
    return v & (v - 1) == 0


def check_plan(case, plan, who):
    """the case's intended plan against what `who` reports (a mismatch is a failure, never a skip)"""
    assert isinstance(plan, dict), '%s: %s refuses the size (%r)' % (case['name'], who, plan)
    for k, v in case['expect'].items():
        assert plan[k] == v, '%s: %s gives %s = %d, the case is written for %d' % (case['name'], who, k, plan[k], v)


def route_line(case, plan):
    return 'ROUTE distill %s gram: splits=%d kper=%d tiles=%dx%d fold=%d | bwd: route=%d tile=%dx%d ntiles=%d mtiles=%d | launches fwd=%d bwd=%d' % (
        case['name'], plan['gram_splits'], plan['gram_kper'], plan['gram_col_tiles'], plan['gram_co_tiles'], plan['gram_fold'],
        plan['bwd_route'], plan['bwd_bp'], plan['bwd_bc'], plan['bwd_ntiles'], plan['bwd_mtiles'], plan['fwd_launches'], plan['bwd_launches'])


# ---- data -------------------------------------------------------------------------------------------------------------------------
def make_data(kind, case, seed=0):
    """f, t float64 [N, HW, C].  Every image is drawn with its own seed and has one channel doubled (image b: channel b mod C of f,
    (b + 1) mod C of t), so image b's Gram matrix differs from image b + 1's by construction.
    'int': integers in [-3, 3] ({-1, 0, 1} where the case says tern: the stage-4 exactness condition at C = 256) before the doubling.
    'normal': f ~ N(0, 1), t ~ 0.8 N(0, 1) + 0.1 (tests/test_kernels_gpu.py::test_distill_loss), rounded to bf16."""
    N, C, HW = case['N'], case['C'], case['HW']
    fs, ts = [], []
    for b in range(N):
        gen = torch.Generator().manual_seed(seed + 7919 * b + 31 * C + HW)
        if kind == 'int':
            m = 1 if case['tern'] else 3
            f = torch.randint(-m, m + 1, (HW, C), generator=gen).double()
            t = torch.randint(-m, m + 1, (HW, C), generator=gen).double()
        else:
            assert kind == 'normal'
            f = rb64(torch.randn(HW, C, generator=gen))
            t = rb64(torch.randn(HW, C, generator=gen) * 0.8 + 0.1)
        f[:, b % C] *= 2
        t[:, (b + 1) % C] *= 2
        fs.append(f)
        ts.append(t)
    d = dict(f=torch.stack(fs), t=torch.stack(ts))
    assert torch.equal(rb64(d['f']), d['f']) and torch.equal(rb64(d['t']), d['t'])
    return d


def gram64(x):
    """([N, C, C] G_n = X_n^T X_n, the same product of |X|)"""
    return torch.bmm(x.transpose(1, 2), x), torch.bmm(x.abs().transpose(1, 2), x.abs())


def assert_images_differ(d):
    for x in (d['f'], d['t']):
        G = gram64(x)[0]
        for b in range(G.shape[0] - 1):
            assert not torch.equal(G[b], G[b + 1]), 'images %d and %d have the same Gram matrix' % (b, b + 1)


def f32(v):
    """the fp32 number a kernel receives for a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


def inv_chw32(C, HW):
    """the host's 1.f / ((float)C * (float)HW) as an fp32 tensor"""
    return torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(C), dtype=torch.float32) * torch.tensor(float(HW), dtype=torch.float32))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- depth of the two sums (stage 3), counted from misc.hip ---------------------------------------------------------------------------
def red_grid(n):
    """grid_for(n, 256 * 4, RED_BLOCKS)"""
    return max(1, min(RED_BLOCKS, cdiv(n, 1024)))


BLOCK_DEPTH = 6 + 4          # block_sum256: the six steps of wave_sum, then `t = 0; t += sh[0..3]`: four additions


def finalize_depth(blocks):
    """scalar_finalize_kernel: a thread adds partial[i], i = tid, tid + 256, ...; then block_sum256"""
    return cdiv(blocks, 256) + BLOCK_DEPTH


def gram_depth(N, C):
    """gram_diff_kernel + scalar_finalize_kernel: (term, depth).  A term d * d, d = (gf - gt) * inv_chw: the subtraction, inv_chw's own
    rounding on the host and the product are three roundings of d, so six of d * d, and the square's own: 7.  Depth: one addition per
    trip of the grid-stride loop, block_sum256, the finalize kernel's chain."""
    ng = N * C * C
    b = red_grid(ng)
    return 7, cdiv(ng, b * 256) + BLOCK_DEPTH + finalize_depth(b)


def content_depth(N, C, HW):
    """diff_reduce_kernel (mode 1) + scalar_finalize_kernel.  A term d * d, d = a - b of two bf16 values (one rounding where their
    exponents lie far apart): 2 + 1 = 3.  A trip of the loop adds the 8 channels of one 16-byte piece."""
    total = N * HW * (C // 8)
    b = red_grid(total)
    return 3, 8 * cdiv(total, b * 256) + BLOCK_DEPTH + finalize_depth(b)


def scalar_rel_bound(term, depth, squared):
    """relative bound of stage 3 for a sum of non-negative terms: gamma_(term + depth) on the sum, one rounding of the quotient's
    cast to fp32; RMSE form: the root halves it (sqrt(1 + e) <= 1 + e / 2), sqrtf adds 1 ulp = 2^-23"""
    n = (term + depth) * U24
    e = n / (1 - n) + U24
    return e if squared else 0.5 * e + 2 * U24


# ---- the six stage checks (on CPU tensors: the device's, or the emulation's) ----------------------------------------------------------
K_COMBINE = 7    # distill_combine_kernel, fp32 roundings over |kg dfg| + |kc (f - t)|: the host's (float)kg0 and (float)kc0 (2), the division
#                  by scal -- exact doubling in the squared form -- (1), f - t (1), the two products (2), the add (1; none where contracted)


def stage1(case, d, kind, Gf, Gt):
    """returns the largest err / bound (0 where the comparison is bit for bit)"""
    worst = 0.0
    for name, x, G in (('Gf', d['f'], Gf), ('Gt', d['t'], Gt)):
        ref, mag = gram64(x)
        what = '%s %s stage 1 %s' % (case['name'], kind, name)
        assert G.dtype == torch.float32 and G.shape == ref.shape, what
        if kind == 'int':
            assert float(mag.max()) < EXACT_LIMIT, '%s: magnitude sum %.4g is not below 2^24' % (what, float(mag.max()))
            bad = G.double() != ref
            assert not bool(bad.any()), '%s: %d of %d entries are not the exact integer, first at %s' % (
                what, int(bad.sum()), bad.numel(), tuple(int(v) for v in bad.nonzero()[0]))
        else:
            worst = max(worst, within(G, ref, bound_wgrad(mag, case['HW'], case['expect']['gram_splits']), what))
    return worst


def s_definition(case, Gf, Gt):
    """fp32 D and bf16 S as gram_diff_kernel forms them from the fp32 Gf, Gt it read (IEEE fp32 operations, in torch)"""
    dd = (Gf - Gt) * inv_chw32(case['C'], case['HW'])
    return dd, dd.bfloat16()


def stage2(case, Gf, Gt, S):
    want = s_definition(case, Gf, Gt)[1]
    assert S.dtype == torch.bfloat16 and S.shape == want.shape
    bad = bits(S) != bits(want)
    assert not bool(bad.any()), '%s stage 2: %d of %d entries of S are not f2bf((gf - gt) * inv_chw), first at %s' % (
        case['name'], int(bad.sum()), bad.numel(), tuple(int(v) for v in bad.nonzero()[0]))
    return 0.0


def scalar_refs(case, d, Gf, Gt, squared):
    """float64 Lg from the Gf, Gt the kernel read, Lc from f, t"""
    N, C, HW = case['N'], case['C'], case['HW']
    D = (Gf.double() - Gt.double()) / (C * HW)
    lg, lc = float((D * D).sum()) / (N * C * C), float(((d['f'] - d['t']) ** 2).sum()) / (N * HW * C)
    return (lg, lc) if squared else (math.sqrt(lg), math.sqrt(lc))


def stage3(case, d, Gf, Gt, scal, out2, squared):
    N, C, HW = case['N'], case['C'], case['HW']
    refs = scalar_refs(case, d, Gf, Gt, squared)
    rel = (scalar_rel_bound(*gram_depth(N, C), squared), scalar_rel_bound(*content_depth(N, C, HW), squared))
    worst = 0.0
    for i, name in enumerate(('Lg', 'Lc')):
        got, ref = float(scal[i]), refs[i]
        err, bound = abs(got - ref), rel[i] * abs(ref)
        assert err <= bound, '%s stage 3 %s (squared=%d): got %.9g, ref %.9g, err %.3g > bound %.3g' % (case['name'], name, squared, got, ref, err, bound)
        worst = max(worst, err / bound if err else 0.0)
    assert torch.equal(bits(out2[:2]), bits(scal[:2])), '%s stage 3: out2 %s is not scal %s' % (case['name'], out2[:2].tolist(), scal[:2].tolist())
    return worst


def stage4_exact(case, kind):
    return kind == 'int' and pow2(case['C'] * case['HW'])


def stage4(case, d, kind, S, dfg):
    """dfg [N, HW, C] bf16 against f_n . S_n with the S the product read"""
    C, HW = case['C'], case['HW']
    Sd = S.double()
    ref, mag = torch.bmm(d['f'], Sd), torch.bmm(d['f'].abs(), Sd.abs())
    what = '%s %s stage 4' % (case['name'], kind)
    assert dfg.dtype == torch.bfloat16 and dfg.shape == ref.shape, what
    if stage4_exact(case, kind):
        scaled = Sd * (C * HW)
        assert torch.equal(scaled, scaled.round()), what + ': S is not a multiple of 1 / (C HW)'
        assert float(mag.max()) * (C * HW) < EXACT_LIMIT, '%s: C HW sum |f| |S| = %.4g is not below 2^24' % (what, float(mag.max()) * C * HW)
        bad = bits(dfg) != bits(expected_bits(ref))
        assert not bool(bad.any()), '%s: %d of %d entries are not the one rounding of the exact sum, first at %s' % (
            what, int(bad.sum()), bad.numel(), tuple(int(v) for v in bad.nonzero()[0]))
        return 0.0
    return within(dfg, ref, bound_out(ref, mag, C, 1), what)


def coefficients(case, scal, squared, wg=WG, wc=WC):
    """float64 (kg, kc) from the scalars the kernel read; the host forms kg0, kc0 in double from the fp32 wg, wc it was handed"""
    N, C, HW = case['N'], case['C'], case['HW']
    kg0, kc0 = f32(wg) * 2.0 / (float(N) * C * C * C * HW), f32(wc) / (float(N) * C * HW)
    return (2 * kg0, 2 * kc0) if squared else (kg0 / float(scal[0]), kc0 / float(scal[1]))


def stage5(case, d, scal, dfg, df, squared):
    kg, kc = coefficients(case, scal, squared)
    a, b = kg * dfg.double(), kc * (d['f'] - d['t'])
    ref = a + b
    bound = BF16 * ref.abs() + K_COMBINE * U24 * (a.abs() + b.abs())
    assert df.dtype == torch.bfloat16
    return within(df, ref, bound, '%s stage 5 (squared=%d)' % (case['name'], squared))


def oracle_reference(case, d, squared, wg=WG, wc=WC):
    """(Lg, Lc, df [N, HW, C]) by float64 autograd of the oracle's own functions"""
    from oracle import gcc_oracle as O
    N, C, HW = case['N'], case['C'], case['HW']
    x = d['f'].transpose(1, 2).reshape(N, C, HW, 1).clone().requires_grad_(True)
    t = d['t'].transpose(1, 2).reshape(N, C, HW, 1)
    if squared:
        lg, lc = F.mse_loss(O.gram(x), O.gram(t)), F.mse_loss(x, t)
    else:
        lg, lc = O.rmse(O.gram(x), O.gram(t)), O.rmse(x, t)
    (wg * lg + wc * lc).backward()
    return float(lg.detach()), float(lc.detach()), x.grad.reshape(N, C, HW).transpose(1, 2).contiguous()


def stage6(case, d, out2, df, squared, ref=None):
    """(ratio of Lg, of Lc, of df) against the oracle, with the composed bound of the module docstring"""
    N, C, HW = case['N'], case['C'], case['HW']
    S = case['expect']['gram_splits']
    lg, lc, dref = ref if ref is not None else oracle_reference(case, d, squared)
    f, t = d['f'], d['t']
    (Gf, mf), (Gt, mt) = gram64(f), gram64(t)
    D = (Gf - Gt) / (C * HW)
    dD = (bound_wgrad(mf, HW, S) + bound_wgrad(mt, HW, S)) / (C * HW) + 3 * U24 * D.abs()
    mean_d2, rms_dd = float((D * D).mean()), math.sqrt(float((dD * dD).mean()))
    rg, rc = scalar_rel_bound(*gram_depth(N, C), squared), scalar_rel_bound(*content_depth(N, C, HW), squared)
    if squared:      # |mean D'^2 - mean D^2| <= 2 rms(D) rms(dD) + rms(dD)^2 (Cauchy-Schwarz), then stage 3 on the device's own sum
        eLg = (2 * math.sqrt(mean_d2) * rms_dd + rms_dd ** 2) / mean_d2
    else:            # |rms(D') - rms(D)| <= rms(dD)
        eLg = rms_dd / math.sqrt(mean_d2)
    eLg = eLg + rg * (1 + eLg)
    eLc = rc
    worst = []
    for name, got, want, e in (('Lg', float(out2[0]), lg, eLg), ('Lc', float(out2[1]), lc, eLc)):
        err = abs(got - want)
        assert err <= e * want, '%s stage 6 %s (squared=%d): got %.9g, oracle %.9g, err %.3g > bound %.3g' % (case['name'], name, squared, got, want, err, e * want)
        worst.append(err / (e * want) if err else 0.0)
    dS = dD + RND_BF16 * (D.abs() + dD)
    fa = f.abs()
    A = torch.bmm(fa, dS) + (C + 5) * U24 * torch.bmm(fa, D.abs() + dS)
    fD = torch.bmm(f, D)
    dG = A + RND_BF16 * (fD.abs() + A)
    kg0, kc0 = WG * 2.0 / (float(N) * C * C * C * HW), WC / (float(N) * C * HW)
    if squared:
        kg, kc, eg, ec = 2 * kg0, 2 * kc0, 3 * U24, 3 * U24
    else:
        kg, kc = kg0 / lg, kc0 / lc
        eg, ec = eLg / (1 - eLg) + 3 * U24, eLc / (1 - eLc) + 3 * U24
    ft = (f - t).abs()
    bound = BF16 * dref.abs() + (1 + 2 * RND_BF16) * (kg * dG + eg * kg * (fD.abs() + dG) + ec * kc * ft + 3 * U24 * (kg * fD.abs() + kc * ft))
    worst.append(within(df, dref, bound, '%s stage 6 df (squared=%d)' % (case['name'], squared)))
    return tuple(worst)


def run_stages(case, d, kind, r, squared):
    """every stage on one set of intermediates r = dict(Gf, Gt, S, scal, out2, dfg, df): {stage name: largest err / bound}; stage 6
    on 'normal' data"""
    out = dict(s1=stage1(case, d, kind, r['Gf'], r['Gt']), s2=stage2(case, r['Gf'], r['Gt'], r['S']),
               s3=stage3(case, d, r['Gf'], r['Gt'], r['scal'], r['out2'], squared), s4=stage4(case, d, kind, r['S'], r['dfg']),
               s5=stage5(case, d, r['scal'], r['dfg'], r['df'], squared))
    if kind == 'normal':
        out['s6_Lg'], out['s6_Lc'], out['s6_df'] = stage6(case, d, r['out2'], r['df'], squared)
    return out


def failing_stages(case, d, kind, r, squared):
    """names of the stage checks that raise on r (tests/test_distill_bounds_cpu.py: a wrong variant must fail at least one)"""
    calls = dict(s1=lambda: stage1(case, d, kind, r['Gf'], r['Gt']), s2=lambda: stage2(case, r['Gf'], r['Gt'], r['S']),
                 s3=lambda: stage3(case, d, r['Gf'], r['Gt'], r['scal'], r['out2'], squared),
                 s4=lambda: stage4(case, d, kind, r['S'], r['dfg']), s5=lambda: stage5(case, d, r['scal'], r['dfg'], r['df'], squared))
    bad = []
    for name, fn in calls.items():
        try:
            fn()
        except (AssertionError, ZeroDivisionError):      # a sum that came out as 0 divides kg0: as wrong as a missed bound
            bad.append(name)
    return bad


# ---- CPU emulation with named wrong variants (tests/test_distill_bounds_cpu.py only) --------------------------------------------------
WRONG = ('squared_no_factor2', 'lg_count_nchw', 'kc_no_lc', 'next_image_s', 'truncate_s', 'gram_drop_last_kstep', 'dfg_ragged_spill')


def wrong_applies(wrong, case, squared):
    """does the variant change anything at this case?  lg_count_nchw needs C != HW; next_image_s and dfg_ragged_spill a second image;
    the spill a ragged last pixel tile; the squared / RMSE variants their form"""
    N, C, HW = case['N'], case['C'], case['HW']
    return {'squared_no_factor2': squared, 'lg_count_nchw': C != HW, 'kc_no_lc': not squared, 'next_image_s': N > 1,
            'truncate_s': True, 'gram_drop_last_kstep': True, 'dfg_ragged_spill': N > 1 and HW % 128 != 0}[wrong]


def _trunc_bf16(v):
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def _block_sums(per_thread):
    """block_sum256 on [blocks, 256] fp32 per-thread sums: the wave butterfly (a balanced tree of six levels), then the four wave
    partials added in order to 0"""
    v = per_thread.view(-1, 4, 64)
    o = 32
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o >>= 1
    v = v[..., 0]
    t = torch.zeros(v.shape[0], dtype=torch.float32)
    for i in range(4):
        t = t + v[:, i]
    return t


def _grid_stride_sum(terms, blocks, per_trip=1):
    """a grid-stride loop of `blocks` x 256 threads over terms [n, per_trip] (a thread adds a trip's per_trip values in order), then
    block_sum256 per block and scalar_finalize_kernel's chain + block_sum256 over the partials: the fp32 total"""
    n = terms.shape[0]
    T = blocks * 256
    trips = cdiv(n, T)
    pad = torch.zeros((trips * T, per_trip), dtype=torch.float32)
    pad[:n] = terms
    pad = pad.view(trips, T, per_trip)
    acc = torch.zeros(T, dtype=torch.float32)
    for s in range(trips):
        for j in range(per_trip):
            acc = acc + pad[s, :, j]
    partial = _block_sums(acc.view(blocks, 256))
    fin = torch.zeros(cdiv(blocks, 256) * 256, dtype=torch.float32)
    fin[:blocks] = partial
    fin = fin.view(-1, 256)
    acc = torch.zeros(256, dtype=torch.float32)
    for s in range(fin.shape[0]):
        acc = acc + fin[s]
    return _block_sums(acc.view(1, 256))[0]


def _finalize(total, count, squared):
    q = torch.tensor(float(total.double()) / count, dtype=torch.float32)
    return q if squared else torch.sqrt(q)


def _gram_emul(x32, plan, drop_last):
    """wgrad_kernel per image: fp32 accumulation over the 64-pixel k-steps of each pixel split, the slabs folded as the flat kernel
    (in order) or the vec kernel (four split lanes, then lanes 1..3 added to lane 0) does"""
    N, HW, C = x32.shape
    ksteps, kper, splits = cdiv(HW, TP), plan['gram_kper'], plan['gram_splits']
    slabs = []
    for s in range(splits):
        acc = torch.zeros(N, C, C, dtype=torch.float32)
        for k in range(s * kper, min(ksteps, (s + 1) * kper)):
            if drop_last and k == ksteps - 1:
                continue
            blk = x32[:, k * TP:min(HW, (k + 1) * TP)]
            acc = acc + torch.bmm(blk.transpose(1, 2), blk)
        slabs.append(acc)
    if plan['gram_fold'] == 0:
        return slabs[0]
    if plan['gram_fold'] == 1:
        tot = torch.zeros_like(slabs[0])
        for q in slabs:
            tot = tot + q
        return tot
    lanes = []
    for sl in range(4):
        tot = torch.zeros_like(slabs[0])
        for z in range(sl, splits, 4):
            tot = tot + slabs[z]
        lanes.append(tot)
    tot = lanes[0]
    for q in lanes[1:]:
        tot = tot + q
    return tot


def emulate(case, d, squared, plan, wrong=None):
    """the five kernels in torch on the CPU: fp32 sums in the kernels' chain structure, bf16 S and dfg, the documented constants;
    returns the intermediates run_stages takes.  wrong: one of WRONG --
    squared_no_factor2 (kg = kg0, kc = kc0 in the squared form), lg_count_nchw (Lg's mean over N C HW entries), kc_no_lc (RMSE form: kc
    not divided by Lc), next_image_s (image b's product reads image (b + 1) mod N's S), truncate_s (S truncated, not rounded),
    gram_drop_last_kstep (the Gram products lose their last 64-pixel step), dfg_ragged_spill (the rows of image b's last pixel tile
    past HW land in image b + 1's first rows)"""
    assert wrong is None or wrong in WRONG
    N, C, HW = case['N'], case['C'], case['HW']
    f32_, t32 = d['f'].float(), d['t'].float()
    drop = wrong == 'gram_drop_last_kstep'
    Gf, Gt = _gram_emul(f32_, plan, drop), _gram_emul(t32, plan, drop)
    dd, S = s_definition(case, Gf, Gt)
    if wrong == 'truncate_s':
        S = _trunc_bf16(dd)
    ng = N * C * C
    lg = _finalize(_grid_stride_sum((dd * dd).reshape(-1, 1), red_grid(ng)), float(N * C * HW if wrong == 'lg_count_nchw' else ng), squared)
    diff = (f32_ - t32).reshape(-1, 8)
    lc = _finalize(_grid_stride_sum(diff * diff, red_grid(diff.shape[0]), 8), float(N * HW * C), squared)
    scal = torch.stack([lg, lc])
    Sf = S.float()
    if wrong == 'next_image_s':
        Sf = Sf.roll(-1, 0)
    dfg32 = torch.bmm(f32_, Sf)
    if wrong == 'dfg_ragged_spill':
        flat_f, flat_g = f32_.reshape(N * HW, C), dfg32.reshape(N * HW, C).clone()
        spill = cdiv(HW, 128) * 128 - HW
        for b in range(N - 1):
            rows = slice((b + 1) * HW, min(N * HW, (b + 1) * HW + spill))
            flat_g[rows] = flat_f[rows] @ Sf[b]
        dfg32 = flat_g.view(N, HW, C)
    dfg = dfg32.bfloat16()
    kg0 = torch.tensor(f32(WG) * 2.0 / (float(N) * C * C * C * HW), dtype=torch.float32)
    kc0 = torch.tensor(f32(WC) / (float(N) * C * HW), dtype=torch.float32)
    if squared:
        kg, kc = (kg0, kc0) if wrong == 'squared_no_factor2' else (2 * kg0, 2 * kc0)
    else:
        kg, kc = kg0 / scal[0], (kc0 if wrong == 'kc_no_lc' else kc0 / scal[1])
    df = (kg * dfg.float() + kc * (f32_ - t32)).bfloat16()
    return dict(Gf=Gf, Gt=Gt, S=S, scal=scal, out2=scal.clone(), dfg=dfg, df=df)
