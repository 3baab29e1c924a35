"""gcc_conv_bn_act (conv_igemm.hip; norm_act.hip bn_fold_grid_kernel): conv + training BatchNorm + dropout + activation(s) in one
call, shared by tests/test_convbn_bounds_cpu.py and tests/test_convbn_exact_gpu.py (no tests here): a restatement of the route /
split / grid plan, the case table with the regime every case is built for, exact data whose result is known to the bit (but
for the last roundings), a float64 reference with per-element bounds derived from the kernel text, and a CPU emulation of the
three routes' order with named defects.

A geometry is g = (N, H, W, Ci, Co, k, stride, pad) as in tests/_conv_exact.py; dgrad: the ConvTranspose form (the output is
[N, Ci, H, W]).  Outputs are handled as [P, C] float64 (P pixels of the NHWC output, row-major; C logical channels)."""
import numpy as np
import torch

from tests import _conv_exact as X
from tests._perelem import ACT_LRELU, ACT_RELU, BF16, U24, act_fn, rb64, rng_uniform, within

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3           # include/gcc_hip.h GCC_ERR_*
EPS = float(np.float32(1e-5))
MOMENTUM = float(np.float32(0.125))                    # a power of two: 1 - momentum is exact
SLOPE = 0.25
K4 = (4, 2, 1)
FOLD_BN_MAX_ROWS, PARTIAL_CAP = 4096, 4096 * 1024      # conv_igemm.hip FOLD_BN_MAX_ROWS, FUSE_BN_PARTIAL_BYTES
GRID_WS_BYTES = 4096 + (3 << 19)                       # GCC_INORM_WORKSPACE_BYTES: the part of the tail workspace the grid fold uses
WS_HEADER = 4096
PLAN_BIG_MIN, PLAN_BIG_NK = 120, 24                    # common.hpp, the default plan (tile_families 3)
cdiv, ceil8 = X.cdiv, X.ceil8


# ---- the plan: select_tile, plan_ksplit, the slice cap, conv_bn_decide and bn_fold_grid_prepare restated ---------------------------
def family_wgs(cus=256, queues=4):
    cus = min(cus, 256)
    return max(1, min(cus, 4 * cus // max(queues, 4)))


def geometry(g, dgrad):
    """(Cout, phases, rows of one phase (max), nk, output H, W)"""
    N, H, W, Ci, Co, k, s, p = g
    Ho, Wo = X.out_hw(g)
    if not dgrad:
        return Co, 1, N * Ho * Wo, cdiv(k * k * ceil8(Ci), X.BK), Ho, Wo
    return Ci, s * s, N * cdiv(H, s) * cdiv(W, s), cdiv(cdiv(k, s) ** 2 * ceil8(Co), X.BK), H, W


def select_tile(max_rows, Cout, phases, nk):
    """(BP, BC, ntiles, mtiles, max_slices) under the default plan, batch 1"""
    BC = 128 if Cout > 64 else (64 if Cout > 32 else (32 if Cout > 16 else 16))
    ntiles, max_slices, BP = (cdiv(Cout, 128) if Cout > 64 else 1), 1 << 30, 128
    if BC > 32:
        mt = cdiv(max_rows, 128) * phases
        if nk <= 64:
            bc = BC
            while bc > 32 and mt * cdiv(Cout, bc) < 256:
                bc >>= 1
            if mt * cdiv(Cout, bc) >= 256:
                BC, ntiles = bc, cdiv(Cout, bc)
        elif mt >= 8 and mt * cdiv(Cout, BC) < 128:
            BC, ntiles, max_slices = 64, cdiv(Cout, 64), 8
    if Cout >= 128 and nk >= PLAN_BIG_NK:
        m256 = cdiv(max_rows, 256)
        if Cout % 256 == 0 and m256 * (Cout // 256) * phases >= PLAN_BIG_MIN:
            BP, BC, ntiles = 256, 256, Cout // 256
        elif m256 * cdiv(Cout, 128) * phases >= PLAN_BIG_MIN:
            BP, BC, ntiles = 256, 128, cdiv(Cout, 128)
    return BP, BC, ntiles, cdiv(max_rows, BP), max_slices


def plan_ksplit(blocks, nk, max_slices):
    if blocks >= 128 or nk < 16:
        return 1, nk
    s = min(cdiv(1024, blocks), nk // 4, max_slices)
    if s < 2:
        return 1, nk
    kper = cdiv(nk, s)
    ks = cdiv(nk, kper)
    return (ks, kper) if ks >= 2 else (1, nk)


def cap_slices(ks, kper, per_slice, nk):
    k2 = ks
    while k2 > 4 and per_slice * k2 > PARTIAL_CAP:
        k2 = (k2 + 1) // 2
    if k2 != ks:
        kper = cdiv(nk, k2)
        ks = cdiv(nk, kper)
    return ks, kper


def grid_plan(C, HW, ws_bytes, wgs):
    """inorm_grid_plan with N = 1, px = 1, chg_max = 16"""
    CH = (C + 7) // 8
    if CH > 256:
        return None
    CHg = 8 if CH >= 16 else CH
    CG = cdiv(CH, CHg)
    if CG > wgs:
        return None
    CHP = 1
    while CHP < CHg:
        CHP *= 2
    PL, V = 256 // CHP, CHg * 16
    S = max(1, min(cdiv(HW, PL), wgs // CG, 8 * max(1, 4096 // V)))
    rows = cdiv(cdiv(HW, S), PL) * PL
    S = cdiv(HW, rows)
    S1 = min(S, max(1, 4096 // V))
    G = cdiv(S, S1)
    if G > 8 or (S > 1 and ws_bytes < WS_HEADER + CG * S * V * 8 + CG * G * V * 16):
        return None
    return dict(S=S, S1=S1, G=G, rows=rows, CG=CG, CHg=CHg, PL=PL)


def thin_routed(g, dgrad):
    """conv_bn_decide's `routed`: the thin image-side layers and the single-channel head (default options)"""
    N, H, W, Ci, Co, k, s, p = g
    head = Co == 1 and 4 <= k * k <= 16 and ceil8(Ci) >= 256
    if not dgrad:
        return head or (ceil8(Ci) == 8 and k * k <= 16 and Co >= 16)
    return head or (ceil8(Ci) == 8 and (k, s, p) == K4 and not (H & 1) and not (W & 1) and 16 <= Co <= 128 and (Co <= 64 or (W // 2) % 4 == 0))


def plan(g, dgrad, fuse=3, cus=256, queues=4, tail_ws=True, inorm_grid=1):
    """what gcc_conv_bn_act_plan answers: dict(route, ksplit) and on route 2 S, S1, G, rows, CG, CHg, PL, PPT.  On route 0 ksplit is
    the split gcc_internal_igemm makes with the call's workspace (the uncapped plan's bytes: the capped split always fits)."""
    N, H, W, Ci, Co, k, s, p = g
    Cout, phases, max_rows, nk, Hd, Wd = geometry(g, dgrad)
    BP, BC, ntiles, mtiles, max_slices = select_tile(max_rows, Cout, phases, nk)
    ks, kper = plan_ksplit(mtiles * ntiles * phases, nk, max_slices) if BP == 128 else (1, nk)
    per_slice = phases * max_rows * ntiles * BC * 4
    small = max_rows * phases <= FOLD_BN_MAX_ROWS
    if ks > 4 and small:
        ks, kper = cap_slices(ks, kper, per_slice, nk)
    if thin_routed(g, dgrad) or ks <= 1 or not small or fuse not in (1, 3):
        if ks > 4:                       # gcc_internal_igemm caps a statistics launch whatever its rows
            ks, kper = cap_slices(ks, kper, per_slice, nk)
        if not dgrad and Co == 1 and 4 <= k * k <= 16 and ceil8(Ci) >= 256:
            ks = None                    # the head shape's workspace is the head route's (head_fprop_workspace): not restated
        return dict(route=0, ksplit=ks)
    out = dict(route=1, ksplit=ks)
    if fuse != 3 or not tail_ws or not inorm_grid:
        return out
    if dgrad and (Hd % s or Wd % s):
        return out
    Mph = N * (Hd // (s if dgrad else 1)) * (Wd // (s if dgrad else 1))
    gp = grid_plan(Cout, phases * Mph, GRID_WS_BYTES, family_wgs(cus, queues))
    if gp is None or Mph > max_rows or gp['rows'] // gp['PL'] > 4:
        return out
    ppt = gp['rows'] // gp['PL']
    return dict(out, route=2, PPT=1 if ppt <= 1 else (2 if ppt == 2 else 4), **gp)


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def _c(name, g, dgrad=False, regime=None, fuse=3, tail_ws=True, inorm_grid=1, drop=0.0, why=''):
    return dict(name=name, g=g, dgrad=dgrad, regime=regime or {}, fuse=fuse, tail_ws=tail_ws, inorm_grid=inorm_grid, drop=drop, why=why)


# the regime a case is built for on 256 CUs with 4 hardware queues; `lanes`: rows // PL, the rows a lane of the grid fold holds
CASES = (
    _c('r2-s1', (1, 4, 4, 64, 8) + K4, regime=dict(route=2, ksplit=4, S=1, CHg=1, PL=256, PPT=1, launches=2), why='S = 1: no exchange, 4 rows, CHP 1'),
    _c('r2-tail5', (1, 4, 4, 80, 20) + K4, regime=dict(route=2, ksplit=5, S=1, CHg=3, PL=64), why='5 slices: one behind the four-at-a-time loop; CHP 4, a partial last chunk'),
    _c('r2-tail6', (3, 4, 4, 96, 20) + K4, regime=dict(route=2, ksplit=6), drop=0.5, why='6 slices; count 12 is no power of two; dropout'),
    _c('r2-tail7', (1, 4, 4, 112, 24) + K4, regime=dict(route=2, ksplit=7), why='7 slices'),
    _c('r2-g5', (16, 32, 32, 64, 72) + K4, regime=dict(route=2, ksplit=4, S=128, S1=28, G=5, CHg=9, PL=16, PPT=2, CG=1), why='CHg = 9, CHP 16, two-level exchange, PPT 2'),
    _c('r2-cg3', (1, 32, 32, 64, 136) + K4, regime=dict(route=2, CG=3, CHg=8, PPT=1, lanes=1), why='CG = 3, one live chunk in the last group, PPT 1, S > 1'),
    # more than two rows per lane need rows > 64 (256 // CG) on a layer that is still split: fewer than 8 row tiles of a long K loop
    # and many channel groups (tests/test_convbn_bounds_cpu.py test_rows_per_lane_reachable scans the plan)
    _c('r2-ppt4-3', (14, 16, 16, 264, 1216) + K4, regime=dict(route=2, PPT=4, lanes=3, CG=19, S=10), why='the <4> kernel with three rows per lane'),
    _c('r2-ppt4', (14, 16, 16, 264, 2048) + K4, regime=dict(route=2, PPT=4, lanes=4, CG=32, S=7), why='four rows per lane, 256 chunks'),
    _c('r2-cap', (4, 32, 32, 320, 256) + K4, regime=dict(route=2, ksplit=4, capped_from=8), why='8 planned slices cut to 4 by the 4 MB cap'),
    _c('r2-convT', (1, 4, 4, 256, 256) + K4, dgrad=True, regime=dict(route=2, ksplit=4), drop=0.5, why='ConvTranspose form, equal phases, dropout'),
    _c('r2-convT-n3', (3, 6, 4, 24, 256) + K4, dgrad=True, regime=dict(route=2), why='ConvTranspose form, 3 images, H != W, pad lanes'),
    _c('r1-odd55', (1, 5, 5, 64, 256) + K4, dgrad=True, regime=dict(route=1), why='phases of 9, 6, 6 and 4 rows'),
    _c('r1-odd54', (2, 5, 4, 20, 256) + K4, dgrad=True, regime=dict(route=1), drop=0.5, why='phases of 6 and 4 rows; dropout'),
    _c('r1-nows', (1, 4, 4, 80, 20) + K4, tail_ws=False, regime=dict(route=1, ksplit=5, launches=2), why='no tail workspace'),
    _c('r1-nogrid', (3, 4, 4, 96, 20) + K4, inorm_grid=0, regime=dict(route=1, ksplit=6), drop=0.5, why='GCC_OPT_INORM_GRID 0; dropout'),
    _c('r1-fuse1', (16, 32, 32, 64, 72) + K4, fuse=1, regime=dict(route=1, ksplit=4), why='fuse 1 at 4096 rows'),
    _c('r0-unsplit-f2', (2, 32, 32, 16, 40) + K4, fuse=2, regime=dict(route=0, ksplit=1, launches=2), drop=0.5, why='un-split, finalize in the launch; dropout'),
    _c('r0-unsplit-f0', (2, 32, 32, 16, 40) + K4, fuse=0, regime=dict(route=0, ksplit=1, launches=3), why='un-split, gcc_bn_finalize launch'),
    _c('r0-4097', (1, 2, 8194, 64, 24) + K4, regime=dict(route=0, ksplit=4, launches=3), why='4097 rows: past the threshold, split + splitk_fold_stats_kernel'),
    _c('r2-4096', (1, 2, 8192, 64, 24) + K4, regime=dict(route=2, ksplit=4), why='4096 rows: the threshold'),
    _c('r0-split-f2', (1, 4, 4, 80, 20) + K4, fuse=2, regime=dict(route=0, ksplit=5, launches=3), why='a split layer with fuse 2'),
    _c('r0-convT-f0', (1, 5, 5, 64, 256) + K4, dgrad=True, fuse=0, regime=dict(route=0), why='ConvTranspose form on route 0, unequal phases'),
    _c('r0-thin', (2, 16, 16, 3, 40) + K4, regime=dict(route=0, ksplit=1, routed=True), why='thin image-side geometry'),
    _c('r0-head', (2, 8, 8, 256, 1, 4, 1, 1), regime=dict(route=0, routed=True, planned_split=True), why='the head shape: the only geometry whose K the plan splits and `routed` keeps off the fused routes'),
)
BY_NAME = {c['name']: c for c in CASES}


def check_regime(case, pl):
    """`pl` (the library's answer or the restatement) is the plan the case is named for"""
    assert isinstance(pl, dict), '%s: declined with %r' % (case['name'], pl)
    have = dict(pl)
    if pl['route'] == 2:
        have['lanes'] = pl['rows'] // pl['PL']
    g, dg = case['g'], case['dgrad']
    Cout, phases, max_rows, nk, _, _ = geometry(g, dg)
    BP, BC, ntiles, mtiles, max_slices = select_tile(max_rows, Cout, phases, nk)
    have['capped_from'] = plan_ksplit(mtiles * ntiles * phases, nk, max_slices)[0]
    have['planned_split'] = have['capped_from'] > 1
    have['routed'] = thin_routed(g, dg)
    for k, v in case['regime'].items():
        if k == 'launches' and have.get(k) is None:
            continue
        assert have.get(k) == v, '%s: %s = %r, the case is built for %r (plan %r)' % (case['name'], k, have.get(k), v, have)


# ---- layout helpers ------------------------------------------------------------------------------------------------------------
def to_pc(t):
    """NCHW -> [P, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def out_shape(g, dgrad):
    N, H, W, Ci, Co, k, s, p = g
    Ho, Wo = X.out_hw(g)
    return (N, Ci, H, W) if dgrad else (N, Co, Ho, Wo)


def special(C):
    """(big-mean channel, dead channel, negative-gamma channel)"""
    return 0, min(1, C - 1), min(2, C - 1)


def keep_mask(seed, P, C, p, stride=None):
    idx = np.arange(P, dtype=np.uint64)[:, None] * np.uint64(stride or C) + np.arange(C, dtype=np.uint64)[None]
    return torch.from_numpy(rng_uniform(seed, idx) >= np.float32(p))


# ---- data ----------------------------------------------------------------------------------------------------------------------
def _special_weights(d, g, dgrad, wbig):
    """a plane of ones in the source feeding only the big-mean channel, through weights wbig on the inner 2 x 2 taps of the 4 x 4
    kernel alone: with pad 1 those taps never fall on padding (stride 2 forward and stride 1: all four see the image; the stride-2
    transposed form: exactly one of them reaches every output pixel), so the offset is the same at every pixel, border included;
    and a dead channel"""
    assert g[5] == 4 and g[7] == 1
    Cout = geometry(g, dgrad)[0]
    big, dead, _ = special(Cout)
    src = 'dy' if dgrad else 'x'
    d[src][:, 0] = 1.0
    if dgrad:                          # w [Co, Ci, k, k]: the output channel is Ci
        d['w'][0] = 0.0
        d['w'][0, big, 1:3, 1:3] = wbig
        if Cout > 1:
            d['w'][:, dead] = 0.0
    else:
        d['w'][:, 0] = 0.0
        d['w'][big, 0, 1:3, 1:3] = wbig
        if Cout > 1:
            d['w'][dead] = 0.0
    return d


def params(case, kind, ref_mean, seed):
    """gamma, beta, running_mean, running_var [C] (fp32-representable float64).  'exact': small dyadic values; the sign of beta is
    the sign of -mean gamma, so that shift = beta - mean scale does not cancel (|shift| = |beta| + |mean scale|: the window of the
    exact check is relative to |r||scale| + |shift|)."""
    C = ref_mean.numel()
    gen = torch.Generator().manual_seed(seed + 7)
    _, _, negc = special(C)
    if kind == 'exact':
        gamma = torch.tensor([0.5, 0.75, 1.0, 1.25, 1.5])[torch.randint(0, 5, (C,), generator=gen)].double()
        gamma = gamma * torch.where(torch.rand(C, generator=gen) < 0.3, -1.0, 1.0)
        gamma[negc] = -gamma[negc].abs()
        beta = torch.tensor([0.125, 0.25, 0.375, 0.5])[torch.randint(0, 4, (C,), generator=gen)].double()
        beta = beta * torch.where(ref_mean * gamma > 0, -1.0, 1.0)
        rm = torch.randint(-4, 5, (C,), generator=gen).double() / 8
        rv = torch.randint(1, 9, (C,), generator=gen).double() / 4
    else:
        gamma = ((0.5 + torch.rand(C, generator=gen)) * torch.where(torch.rand(C, generator=gen) < 0.3, -1.0, 1.0)).float().double()
        gamma[negc] = -gamma[negc].abs()
        beta = (0.5 * torch.randn(C, generator=gen)).float().double()
        rm = torch.randn(C, generator=gen).float().double()
        rv = (0.5 + torch.rand(C, generator=gen)).float().double()
    return dict(gamma=gamma, beta=beta, rm=rm, rv=rv)


def make(case, kind, seed):
    """inputs of a case.  'exact': the ternary sparse data of tests/_conv_exact.py ('tiny') with the plane of ones and the weights 4
    of the big-mean channel (a mean of 16, or 4 in the stride-2 transposed form); 'normal': seeded bf16 normals (outputs of unit
    spread), the big-mean channel's weights 20 / (inner taps that reach a pixel): |mean| ~ 20 sigma."""
    g, dg = case['g'], case['dgrad']
    d = X.make_data('tiny' if kind == 'exact' else 'normal', g, seed)
    taps = (2 // g[6]) ** 2 if dg else 4
    d = _special_weights(d, g, dg, 4.0 if kind == 'exact' else 20.0 / taps)
    raw64, pre, mag = (X.ref_dgrad if dg else X.ref_fprop)(d, g)
    d.update(kind=kind, raw64=to_pc(pre), mag=to_pc(mag), case=case, seed=seed)
    d.update(params(case, kind, rb64(d['raw64']).mean(0), seed))
    return d


# ---- float64 finalize and affine ----------------------------------------------------------------------------------------------
def finalize64(r, count, p, gamma=True, beta=True):
    """r [P, C] (the bf16 raw output as float64) -> dict of float64 [C]: mean, var (E[r^2] - mean^2, clamped), rstd, scale, shift,
    rm, rv (momentum blend with the unbiased variance) and the magnitudes the roundings are relative to"""
    m = r.sum(0) / count
    var = ((r * r).sum(0) / count - m * m).clamp_min(0.0)
    rs = 1.0 / torch.sqrt(var + EPS)
    g = p['gamma'] if gamma else torch.ones_like(m)
    b = p['beta'] if beta else torch.zeros_like(m)
    sc = g * rs
    sf = b - m * sc
    unb = var * count / (count - 1.0) if count > 1 else var
    return dict(mean=m, var=var, rstd=rs, scale=sc, shift=sf, rm=(1 - MOMENTUM) * p['rm'] + MOMENTUM * m, rv=(1 - MOMENTUM) * p['rv'] + MOMENTUM * unb,
                Msf=b.abs() + (m * sc).abs(), Mrm=(1 - MOMENTUM) * p['rm'].abs() + MOMENTUM * m.abs(),
                Mrv=(1 - MOMENTUM) * p['rv'].abs() + MOMENTUM * unb, E2=(r * r).sum(0) / count, Eabs=r.abs().sum(0) / count)


# fp32 roundings, read from bn_channel_finalize (common.hpp), splitk_bn_act_kernel and bn_fold_grid_kernel (the same text):
#   mean = (float)m: 1.  rstd = (float)(1 / sqrt(var + eps)): 1 (the double operations in front are 2^-53 each).
#   scale = g * r: the cast in r and the product: 2.
#   shift = b - (float)m * g * r: the two casts, two products and the subtraction (one fewer where the last product is fused): 5,
#     relative to |b| + |m scale|.
#   running = (1.f - mom) * old + mom * (float)new: the difference, two products, the cast, the sum: 5, relative to the two terms.
#   v = r * scale + shift: product and sum (one where fused): 2; dropout's v * keep_scale (keep_scale = 1.f / (1.f - p): 2 more, both
#     exact at p = 0.5); the slope's product: 1 (exact at 0.25).
K_MEAN, K_RSTD, K_SCALE, K_SHIFT, K_RUN, K_AFF = 1, 1, 2, 5, 5, 5
# the exact check's window: the error of scale (2) and of the product and sum (2) on |r||scale|, of shift (5) and the sum on |shift|
# -- exact data has |shift| = |beta| + |mean scale| (params) -- the dropout and slope products on the result: 12 in all
K_WIN = 12


def activations(v, act, act2, keep, drop):
    if keep is not None:
        v = torch.where(keep, v * (1.0 / (1.0 - drop)), torch.zeros_like(v))
    return act_fn(v, act, SLOPE), act_fn(v, act2, SLOPE)


# ---- the exact check -----------------------------------------------------------------------------------------------------------
def exact_ref(d, count=None, act=ACT_LRELU, act2=ACT_RELU, gamma=True, beta=True):
    """everything the call must produce on 'exact' data, from float64 alone; asserts the exactness conditions"""
    case = d['case']
    r = d['raw64']
    P, C = r.shape
    count = float(P if count is None else count)
    assert bool((r == rb64(r)).all()), '%s: a raw output is not its own bf16 rounding' % case['name']
    assert float(d['mag'].max()) < X.EXACT_LIMIT
    # every fp32 sum of r and r^2 any route forms is a sum over a subset of a channel's rows: below 2^24 in units of 1
    assert bool((r == r.round()).all()) and float(r.abs().sum(0).max()) < X.EXACT_LIMIT and float((r * r).sum(0).max()) < X.EXACT_LIMIT
    f = finalize64(r, count, d, gamma, beta)
    v = r * f['scale'] + f['shift']
    win = K_WIN * U24 * (r.abs() * f['scale'].abs() + f['Msf'])       # Msf = |shift| on the case's own gamma / beta (data_conditions)
    keep = keep_mask(d['seed'], P, C, case['drop']) if case['drop'] else None
    lo1, lo2 = activations(v - win, act, act2, keep, case['drop'])
    hi1, hi2 = activations(v + win, act, act2, keep, case['drop'])
    out = dict(f, raw=r, v=v, keep=keep, y=(rb64(lo1), rb64(hi1)), y2=(rb64(lo2), rb64(hi2)), count=count)
    out['ambiguous'] = max(float((out[k][0] != out[k][1]).double().mean()) for k in ('y', 'y2'))
    return out


def data_conditions(d, ref):
    """conditions on the exact data (not measurements), on the reference alone"""
    name = d['case']['name']
    v = ref['v']
    C = v.shape[1]
    big, dead, negc = special(C)
    differ = float((rb64(v) != v).double().mean())
    neg = float((v < 0).double().mean())
    assert differ >= 0.10, '%s: only %.1f %% of the pre-activations differ from their bf16 rounding' % (name, 100 * differ)
    assert 0.25 <= neg <= 0.75, '%s: %.1f %% of the pre-activations are negative' % (name, 100 * neg)
    assert ref['ambiguous'] <= 0.01, '%s: ambiguous share %.3g' % (name, ref['ambiguous'])
    if C > 1:
        assert bool((ref['raw'][:, dead] == 0).all()) and float(ref['var'][dead]) == 0.0
    assert float(d['gamma'][negc]) < 0
    assert bool(((ref['shift'].abs() - ref['Msf']).abs() <= 1e-12 * ref['Msf']).all()), name + ': shift cancels'
    return differ, neg


def rel_ok(got, ref, k, mag=None):
    """|got - ref| <= k 2^-24 mag (mag: |ref| by default), elementwise; returns the number of failures"""
    mag = ref.abs() if mag is None else mag
    return int((~((got.double() - ref).abs() <= k * U24 * mag)).sum())


def exact_faults(ref, got, gamma=True, beta=True):
    """dict of counts of elements outside what the exact reference allows.  got: raw, y, y2 [P, C8] (pad lanes included; None: not
    written), mean, rstd, scale, shift, rm, rv [C] or None"""
    C = ref['raw'].shape[1]
    bad = {}
    bad['raw'] = int((got['raw'][:, :C].double() != ref['raw']).sum())
    for k in ('y', 'y2'):
        if got.get(k) is not None:
            yv = got[k][:, :C].double()
            bad[k] = int((~((yv >= ref[k][0]) & (yv <= ref[k][1]))).sum())
    for k in ('raw', 'y', 'y2'):
        if got.get(k) is not None:
            bad[k + '_pad'] = int((got[k][:, C:] != 0).sum())
    for k, n, mag in (('mean', K_MEAN, None), ('rstd', K_RSTD, None), ('scale', K_SCALE, None), ('shift', K_SHIFT, ref['Msf']),
                      ('rm', K_RUN, ref['Mrm']), ('rv', K_RUN, ref['Mrv'])):
        if got.get(k) is not None:
            bad[k] = rel_ok(got[k], ref[k], n, mag)
    return bad


# ---- per element against float64 ------------------------------------------------------------------------------------------------
def chain(pl):
    """longest fp32 accumulation chain of a channel's statistics.  route 1: none (double from the first addition); route 2: a lane's
    rows (rows // PL <= PPT), the shuffle steps (<= 6), the four-wave fold (4), double across workgroups; route 0: the rows of a
    statistic row (a 128-pixel tile of the conv epilogue -- no case here is large enough for the 256-pixel tiles -- or the rows one
    workgroup of splitk_fold_stats_kernel walks: at most 128 by fold_wpp) in any order, then double (bn_finalize_kernel / stats_tail)"""
    if pl['route'] == 1:
        return 0
    if pl['route'] == 2:
        return pl['rows'] // pl['PL'] + 6 + 4
    return 128


def normal_check(d, pl, got, count=None, act=ACT_LRELU, act2=ACT_RELU, gamma=True, beta=True, what=''):
    """raw against float64 within tests/_conv_exact.py bound_out (S = ksplit); the statistics, coefficients and outputs against
    float64 of the kernel's OWN raw, within bounds that follow the route's accumulation:
      ds   = n u E|r|                                        (n = chain(pl): the fp32 part of the sum; the stored mean adds its cast: dm = ds + u |m|)
      dvar = n' u E[r^2] + 2 |m| ds + 2^-50 E[r^2]           (n' = n + 1 with the fp32 product r r, 0 on route 1 where the product and the
                                                              sums are double; E[r^2] = var + m^2: the cancellation term is (1 + m^2 / var)
                                                              relative to var; m itself is a double in every route)
      dr   = dvar / (2 (var + eps - dvar)^1.5) + u r
      dsc  = |g| dr + u |sc|,  dsf = |g| (r ds + |m| dr) + 4 u (|b| + |m sc|)
      y:   |r| dsc + dsf + K_AFF u (|r sc| + |sf|) through a 1-Lipschitz activation (times keep_scale), then one bf16 rounding.
    Returns the worst err / bound ratios."""
    case = d['case']
    g, dg = case['g'], case['dgrad']
    P, C = d['raw64'].shape
    count = float(P if count is None else count)
    K = X.k_products(g, 'D' if dg else 'F')
    ratios = {}
    ratios['raw'] = within(got['raw'][:, :C], d['raw64'], X.bound_out(d['raw64'], d['mag'], K, pl['ksplit']), what + ' raw')
    r = got['raw'][:, :C].double()
    f = finalize64(r, count, d, gamma, beta)
    n = chain(pl)
    u = U24
    ds = n * u * f['Eabs']
    dm = ds + u * f['mean'].abs()
    dvar = ((n + 1) * u if n else 0.0) * f['E2'] + 2 * f['mean'].abs() * ds + 2.0 ** -50 * f['E2']
    dr = 0.5 * (f['var'] + EPS - dvar).clamp_min(EPS / 2) ** -1.5 * dvar + u * f['rstd']
    gm = d['gamma'].abs() if gamma else torch.ones(C, dtype=torch.float64)
    dsc = gm * dr + u * f['scale'].abs()
    dsf = gm * (f['rstd'] * ds + f['mean'].abs() * dr) + 4 * u * f['Msf']
    unb_f = count / (count - 1.0) if count > 1 else 1.0
    for k, b in (('mean', dm), ('rstd', dr), ('scale', dsc), ('shift', dsf), ('rm', MOMENTUM * dm + K_RUN * u * f['Mrm']),
                 ('rv', MOMENTUM * unb_f * dvar + K_RUN * u * f['Mrv'])):
        if got.get(k) is not None:
            ratios[k] = within(got[k], f[k], b, what + ' ' + k)
    v = r * f['scale'] + f['shift']
    dv = r.abs() * dsc + dsf + K_AFF * u * (r.abs() * f['scale'].abs() + f['shift'].abs())
    keep = keep_mask(d['seed'], P, C, case['drop']) if case['drop'] else None
    if keep is not None:
        dv = dv * keep / (1.0 - case['drop'])
    y1, y2 = activations(v, act, act2, keep, case['drop'])
    for k, ref in (('y', y1), ('y2', y2)):
        if got.get(k) is not None:
            ratios[k] = within(got[k][:, :C], ref, dv + BF16 * (ref.abs() + dv), what + ' ' + k)
            assert int((got[k][:, C:] != 0).sum()) == 0, what + ': pad lanes of ' + k
    big, dead, _ = special(C)
    if C > 1:
        assert bool((r[:, dead] == 0).all()), what + ': the dead channel'
    ratios['cancel'] = float((f['mean'] ** 2 / (f['var'] + EPS))[big])
    return ratios


def old_bar(got, d, count=None, act=ACT_LRELU, act2=ACT_RELU):
    """the checks of tests/test_kernels_gpu.py test_conv_bn_act_one_call (close: max |got - ref| <= tol max |ref| + floor over the
    whole tensor) on fp32 torch of the kernel's own raw: True where every one of them accepts"""
    C = d['raw64'].shape[1]
    P = d['raw64'].shape[0]
    count = float(P if count is None else count)
    case = d['case']
    ok = X.old_rule(got['raw'][:, :C].double(), d['raw64'])[0]
    r = got['raw'][:, :C].float()
    mean, var = r.mean(0), r.var(0, unbiased=False)
    rs = 1.0 / torch.sqrt(var + EPS)
    close = lambda a, b: X.old_rule(a.double(), b.double(), 1e-4, 1e-5)[0]
    ok &= close(got['mean'], mean) and close(got['rstd'], rs)
    ok &= close(got['rm'], (1 - MOMENTUM) * d['rm'].float() + MOMENTUM * mean)
    ok &= close(got['rv'], (1 - MOMENTUM) * d['rv'].float() + MOMENTUM * var * count / (count - 1))
    z = (r - mean) * rs * d['gamma'].float() + d['beta'].float()
    keep = keep_mask(d['seed'], P, C, case['drop']) if case['drop'] else None
    y1, y2 = activations(z.double(), act, act2, keep, case['drop'])
    ok &= X.old_rule(got['y'][:, :C].double(), y1)[0] and X.old_rule(got['y2'][:, :C].double(), y2)[0]
    if C % 8:
        ok &= float(got['y'][:, C:].abs().max()) == 0.0
    return bool(ok)


# ---- the three routes' order on the CPU, with named defects -------------------------------------------------------------------------
DEFECTS = ('last_slice_dropped', 'tail_slices_dropped', 'stats_unrounded', 'unbiased_norm', 'biased_running', 'count_one_phase',
           'momentum_reversed', 'fp32_mean_sq', 'phase_swap', 'drop_ceil8', 'act2_from_act', 'pad_shift', 'raw_truncated', 'l2_drops_group')
# the case a defect can show in: a tail behind the four-at-a-time loop, more than one phase with H != W, pad lanes with dropout, G > 1;
# fp32_mean_sq on route 1, whose statistics are double throughout (an fp32 chain of route 2's length has an error of the defect's size);
# act2_from_act with DEFECT_ACTS (relu(lrelu(v)) = relu(v): the U-Net's own pair cannot show it)
DEFECT_ACTS = dict(act2_from_act=(ACT_RELU, ACT_LRELU))
DEFECT_CASE = dict(last_slice_dropped='r2-tail5', tail_slices_dropped='r2-tail6', stats_unrounded='r2-tail6', unbiased_norm='r2-tail6',
                   biased_running='r2-tail6', count_one_phase='r2-convT-n3', momentum_reversed='r2-tail6', fp32_mean_sq='r1-nogrid',
                   phase_swap='r2-convT-n3', drop_ceil8='r2-tail6', act2_from_act='r2-tail6', pad_shift='r2-tail6', raw_truncated='r2-tail6',
                   l2_drops_group='r2-g5')


def _slices(d, S):
    """fp32 partial outputs of S groups of source channels, [S][P, C]"""
    g, dg = d['case']['g'], d['case']['dgrad']
    N, H, W, Ci, Co, k, s, p = g
    w = d['w'].float()
    out = []
    if not dg:
        x = d['x'].float()
        per = cdiv(Ci, S)
        for a in range(0, Ci, per):
            out.append(to_pc(torch.nn.functional.conv2d(x[:, a:a + per], w[:, a:a + per], None, stride=s, padding=p)))
    else:
        dy = d['dy'].float()
        per = cdiv(Co, S)
        for a in range(0, Co, per):
            out.append(to_pc(torch.nn.grad.conv2d_input((N, Ci, H, W), w[a:a + per], dy[:, a:a + per], stride=s, padding=p)))
    return out


def _phase_rows(g, dgrad, swap=False):
    """the pixel (index into the NHWC output) of every row in the kernels' order: phase-major, then image, then the phase's sub-grid"""
    N, H, W, Ci, Co, k, s, p = g
    Hd, Wd = out_shape(g, dgrad)[2:]
    if not dgrad:
        return torch.arange(N * Hd * Wd), [N * Hd * Wd]
    pix, sizes = [], []
    for z in range(s * s):
        py, px = (z % s, z // s) if swap else (z // s, z % s)
        oy, ox = torch.arange(py, Hd, s), torch.arange(px, Wd, s)
        if swap:           # the sub-grid sizes of the right phase, the origin of the wrong one
            oy, ox = torch.arange(cdiv(Hd - z // s, s)) * s + py, torch.arange(cdiv(Wd - z % s, s)) * s + px
        q = (torch.arange(N)[:, None, None] * Hd + oy[None, :, None]) * Wd + ox[None, None, :]
        pix.append(q.reshape(-1))
        sizes.append(q.numel())
    return torch.cat(pix), sizes


def emulate(d, pl, defect=None, act=ACT_LRELU, act2=ACT_RELU):
    """gcc_conv_bn_act on the CPU in the order of route pl['route']: K slices folded in fp32 in slice order, one rounding to bf16 (the
    raw output), statistics of the rounded values along the route's chain (route 1: double; route 2: fp32 per lane and workgroup,
    double across the S workgroups in groups of S1; route 0: fp32 per 128-row tile, double across tiles), the finalize in double
    with fp32 casts, the fp32 affine, dropout by (pixel * C + channel), both activations, one rounding.  Returns the dict
    exact_faults / normal_check take ([P, C8] outputs with their pad lanes)."""
    assert defect is None or defect in DEFECTS
    f32 = torch.float32
    case = d['case']
    g, dg = case['g'], case['dgrad']
    P, C = d['raw64'].shape
    C8 = ceil8(C)
    S = pl['ksplit']
    parts = _slices(d, S)
    if defect == 'last_slice_dropped':
        parts = parts[:-1]
    if defect == 'tail_slices_dropped':
        parts = parts[:4 * (len(parts) // 4)]
    fold = torch.zeros((P, C), dtype=f32)
    for q in parts:
        fold = fold + q
    rawv = X._trunc_bf16(fold) if defect == 'raw_truncated' else fold.bfloat16().float()
    # rows in the kernels' order; the scatter to pixels
    rows_right, sizes = _phase_rows(g, dg)
    rows_used = _phase_rows(g, dg, swap=True)[0] if defect == 'phase_swap' else rows_right
    vals = rawv[rows_right]                            # the partial tiles hold the right phase's rows ...
    raw = torch.zeros((P, C), dtype=f32)
    raw[rows_used] = vals                              # ... written to the pixels the mapping names
    sv = fold[rows_right] if defect == 'stats_unrounded' else vals
    # statistics
    if pl['route'] == 1:
        s1, s2 = sv.double().sum(0), (sv.double() ** 2).sum(0)
    else:
        if pl['route'] == 2:
            wg_rows, PL = pl['rows'], pl['PL']
        else:
            wg_rows, PL = 128, 128
        nwg = cdiv(P, wg_rows)
        pad = torch.zeros((nwg * wg_rows, C), dtype=f32)
        pad[:P] = sv
        pad = pad.view(nwg, wg_rows // PL, PL, C)
        a1, a2 = torch.zeros((nwg, PL, C), dtype=f32), torch.zeros((nwg, PL, C), dtype=f32)
        for k in range(wg_rows // PL):
            a1, a2 = a1 + pad[:, k], a2 + pad[:, k] * pad[:, k]
        w1, w2 = a1.sum(1).double(), a2.sum(1).double()          # [nwg, C]
        if pl['route'] == 2 and pl['G'] > 1:
            S1 = pl['S1']
            grp1 = [w1[a:a + S1].sum(0) for a in range(0, nwg, S1)]
            grp2 = [w2[a:a + S1].sum(0) for a in range(0, nwg, S1)]
            if defect == 'l2_drops_group':
                grp1, grp2 = grp1[:-1], grp2[:-1]
            s1, s2 = sum(grp1), sum(grp2)
        else:
            s1, s2 = w1.sum(0), w2.sum(0)
    count = float(P)
    if defect == 'count_one_phase':
        count = float(sizes[0])
    m = s1 / count
    msq = m.float().double() ** 2 if defect == 'fp32_mean_sq' else m * m
    var = (s2 / count - msq).clamp_min(0.0)
    unb = var * count / (count - 1.0) if count > 1 else var
    vn = unb if defect == 'unbiased_norm' else var
    r = (1.0 / torch.sqrt(vn + EPS)).to(f32)
    gam, bet = d['gamma'].to(f32), d['beta'].to(f32)
    mf = m.to(f32)
    sc = gam * r
    sf = bet - mf * gam * r
    mom = torch.tensor(MOMENTUM, dtype=f32)
    one = torch.tensor(1.0, dtype=f32)
    a, b = (mom, one - mom) if defect == 'momentum_reversed' else (one - mom, mom)
    rm = a * d['rm'].to(f32) + b * mf
    rv = a * d['rv'].to(f32) + b * (var if defect == 'biased_running' else unb).to(f32)
    v = raw * sc + sf
    if case['drop']:
        keep = keep_mask(d['seed'], P, C, case['drop'], stride=C8 if defect == 'drop_ceil8' else None)
        ks = one / (one - torch.tensor(case['drop'], dtype=f32))
        v = torch.where(keep, v * ks, torch.zeros_like(v))
    y1 = act_fn(v, act, SLOPE)
    y2 = act_fn(y1 if defect == 'act2_from_act' else v, act2, SLOPE)

    def padded(t, padval=0.0):
        o = torch.full((P, C8), float(padval), dtype=torch.float64)
        o[:, :C] = t.bfloat16().double()
        return o
    padv = float(act_fn(sf[-1:], act, SLOPE).bfloat16()[0]) if defect == 'pad_shift' else 0.0
    return dict(raw=padded(raw), y=padded(y1, padv), y2=padded(y2, padv), mean=mf.double(), rstd=r.double(), scale=sc.double(),
                shift=sf.double(), rm=rm.double(), rv=rv.double())


def seeds(case):
    """(exact seed, normal seed) of a case.  A case of a few dozen elements has so few that one open rounding is more than the 1 %
    the ambiguous share may reach: EXACT_SEED holds the first offset at which the data conditions hold (found on the CPU, held to
    by tests/test_convbn_bounds_cpu.py)"""
    base = sum(ord(ch) for ch in case['name']) + sum(case['g'])
    return base + EXACT_SEED.get(case['name'], 0), base + 1000 + NORMAL_SEED.get(case['name'], 0)


# r1-nogrid: the first offset at which the big-mean channel's mean (a multiple of 1/12) is no fp32 number, so that a mean cast to
# fp32 in front of its square shows on the exact data
EXACT_SEED = {'r0-split-f2': 1, 'r1-nogrid': 1}
# likewise on the normal data: the mean of twelve bf16 values near 20 is a multiple of 1 / 96, an fp32 number one time in three
NORMAL_SEED = {'r1-nogrid': 1}
