"""gcc_dw_inorm_fwd (norm_act.hip dw_inorm_kernel: depthwise 3x3 behind ReflectionPad2d(1) + InstanceNorm in one launch), shared
by tests/test_dwin_bounds_cpu.py and tests/test_dw_inorm_exact_gpu.py (no tests here): a restatement of the launch plan, the
case table with the regime every case is built for, exact-integer data whose result is known to the bit, a float64 reference
with a per-element bound derived stage by stage from the kernel text, and a CPU emulation of the kernel's tile / halo / sweep /
exchange order with named defects.  Tensors are [N, HW, C] (images, pixels of a plane row-major, logical channels), float64."""
import numpy as np
import torch

from tests._perelem import U24, BF16, rb64, within

PLAIN, NORM_RELU, RESIDUAL = 0, 1, 2          # include/gcc_hip.h GCC_DWIN_*
MODES = (PLAIN, NORM_RELU, RESIDUAL)
MODE_NAME = ('plain', 'norm_relu', 'residual')
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3  # include/gcc_hip.h GCC_ERR_*
# norm_act.hip: DWIN_LDS_DOUBLES, DWIN_CHG, DWIN_TAP_DOUBLES, DWIN_TILE_BYTES, INORM_WS_HEADER; gcc_hip.h GCC_DW_INORM_WORKSPACE_BYTES
LDS_DOUBLES, CHG, WS_HEADER = 4800, 2, 4096
TAP_DOUBLES = 9 * CHG * 8 // 2
TILE_BYTES = (LDS_DOUBLES - TAP_DOUBLES) * 8
WS_BYTES = 4096 + (3 << 20)
PX = 2                                        # dw_inorm_prepare: pixels per lane the plan aims at
EPS = float(np.float32(1e-5))


# ---- the plan: grid_family_wgs, inorm_grid_plan (px = 2, chg_max = DWIN_CHG) and dw_inorm_prepare restated ------------------------
def family_wgs(cus=256, queues=4):
    cus = min(cus, 256)
    return max(1, min(cus, 4 * cus // max(queues, 4)))


def grid_plan(C, HW, N, px, ws_bytes, wgs, chg_max=16):
    CH = (C + 7) // 8
    if CH > 256 or N > 64:
        return None
    CHg = min(8 if CH >= 16 else CH, chg_max)
    CG = -(-CH // CHg)
    if N * CG > wgs:
        return None
    CHP = 1
    while CHP < CHg:
        CHP *= 2
    PL, V = 256 // CHP, CHg * 16
    S = max(1, min(-(-HW // (px * PL)), wgs // (N * CG), 8 * max(1, 4096 // V)))
    rows = -(-(-(-HW // S)) // PL) * PL
    S = -(-HW // rows)
    S1 = min(S, max(1, 4096 // V))
    G = -(-S // S1)
    if G > 8:
        return None
    if S > 1 and ws_bytes < WS_HEADER + N * CG * S * V * 8 + N * CG * G * V * 16:
        return None
    return dict(S=S, S1=S1, G=G, rows=rows, CG=CG, CHg=CHg, PL=PL)


def plan(C, H, W, N, cus=256, queues=4, ws_bytes=WS_BYTES):
    """the plan of a launch (S, S1, G, rows, CG, CHg, PL, tile: what gcc_dw_inorm_plan answers) or the code it is declined with"""
    if min(C, H, W, N) <= 0:
        return BAD_ARG
    if H < 2 or W < 2 or H * W >= 1 << 31:
        return UNSUPPORTED
    HW, wgs = H * W, family_wgs(cus, queues)
    p = grid_plan(C, HW, N, PX, 1 << 60, wgs, CHG)
    if p is None:
        return UNSUPPORTED
    room = TILE_BYTES // (p['CHg'] * 16) - 2 * W - 2
    tile = (room // p['PL']) * p['PL'] if room >= 0 else 0           # C division truncates: anything below PL is declined
    if tile < p['PL'] or p['rows'] > 8 * p['PL']:
        return UNSUPPORTED
    if ws_bytes < WS_HEADER + 16384:
        return WORKSPACE
    half = ((ws_bytes - WS_HEADER) // 2) & ~15
    p = grid_plan(C, HW, N, PX, WS_HEADER + half, wgs, CHG)
    if p is None:
        return WORKSPACE
    p['tile'] = tile
    return p


def shape_of(pl, H, W):
    """what a regime is named by, from a plan: pixels of the last workgroup, tiles of the first and of the last workgroup's sweep,
    pixels [lo, hi) of the largest tile with its halo, and what the LDS tile holds"""
    HW = H * W
    last = HW - (pl['S'] - 1) * pl['rows']
    span = 0
    for s in range(pl['S']):
        p0, p1 = s * pl['rows'], min((s + 1) * pl['rows'], HW)
        for t0 in range(p0, p1, pl['tile']):
            span = max(span, min(min(t0 + pl['tile'], p1) + W + 1, HW) - max(t0 - W - 1, 0))
    return dict(last=last, tiles=-(-min(pl['rows'], HW) // pl['tile']), tiles_last=-(-last // pl['tile']), span=span,
                room=TILE_BYTES // (pl['CHg'] * 16))


# (C, H, W, N) -> the regime the case is built for on 256 CUs with 4 hardware queues: plan values (gcc_dw_inorm_plan's names) and
# shape_of's.  Both test files assert them; the GPU file from the library's own answer.
CASES = (
    ((3, 2, 2, 1), dict(CHg=1, S=1, tiles=1), 'CHg = 1, S = 1, no exchange; every reflected neighbour is the other pixel'),
    ((9, 3, 2, 2), dict(CHg=2, CG=1, S=1), 'the second chunk has one live channel'),
    ((17, 5, 7, 3), dict(CHg=2, CG=2, S=1), 'CG = 2 with a half-empty last group'),
    ((40, 33, 17, 2), dict(CG=3, S=3, G=1, last=49), 'S = 3, one-level exchange, last workgroup 49 pixels'),
    ((136, 31, 77, 2), dict(CG=9, S=10, G=1, last=83), 'CG = 9, S = 10, last workgroup 83 pixels'),
    ((16, 192, 192, 1), dict(S=144, S1=128, G=2), 'two-level exchange: S = 144, S1 = 128, G = 2'),
    ((8, 300, 300, 1), dict(CHg=1, PL=256, S=176, rows=512, last=400, G=1), 'CHg = 1, S = 176, last workgroup 400 of 512 rows'),
    ((256, 8, 300, 4), dict(rows=640, tile=512, PL=128, tiles=2, tiles_last=1, last=480), 'two tiles per sweep, 5 pixels per lane'),
    ((64, 256, 256, 1), dict(rows=1024, tile=640, PL=128, tiles=2), 'rows at the 8-pixels-per-lane cap: tiles of 640 + 384'),
    ((16, 3, 400, 64), dict(rows=384, tile=256, S=4, tiles=2), 'N at its limit'),
    ((24, 4, 526, 1), dict(CHg=2, tile=128, PL=128, span=1182, room=1182), 'the widest served W at CHg = 2: a middle tile fills the LDS tile'),
    ((8, 4, 1053, 1), dict(CHg=1, tile=256, PL=256, span=2364, room=2364), 'the widest served W at CHg = 1'),
    ((256, 64, 64, 1), dict(CG=16, S=16, rows=256, tiles=1), "the trunk's own geometry"),
    ((256, 64, 64, 2), dict(CG=16, S=8, rows=512, tiles=1), "the trunk's own geometry, two images"),
)
DECLINED = (((24, 4, 527, 1), 'tile < PL at CHg = 2'), ((8, 4, 1054, 1), 'tile < PL at CHg = 1'),
            ((192, 96, 128, 3), 'rows > 8 PL'), ((16, 8, 8, 65), 'N = 65'), ((2056, 4, 4, 1), 'C = 2056'))


def check_regime(case, regime, pl):
    """`pl` (the library's answer or the restatement) is the plan the case is named for"""
    C, H, W, N = case
    assert isinstance(pl, dict), '%r: declined with %r' % (case, pl)
    have = dict(pl, **shape_of(pl, H, W))
    for k, v in regime.items():
        assert have[k] == v, '%r: %s = %r, the case is built for %r (plan %r)' % (case, k, have[k], v, have)
    assert have['span'] <= have['room'] and pl['tile'] % pl['PL'] == 0 and pl['rows'] % pl['PL'] == 0 and pl['rows'] <= 8 * pl['PL']


# ---- the operation in float64 ----------------------------------------------------------------------------------------------------
def conv64(u, w, H, W):
    """depthwise 3x3 behind ReflectionPad2d(1): u [N, HW, C], w [C, 9] (tap ky * 3 + kx) -> [N, HW, C], any dtype"""
    N, HW, C = u.shape
    t = u.reshape(N, H, W, C)
    iy = torch.tensor([1] + list(range(H)) + [H - 2])
    ix = torch.tensor([1] + list(range(W)) + [W - 2])
    t = t[:, iy][:, :, ix]
    d = torch.zeros_like(u).reshape(N, H, W, C)
    for ky in range(3):
        for kx in range(3):
            d = d + w[:, ky * 3 + kx] * t[:, ky:ky + H, kx:kx + W]
    return d.reshape(N, HW, C)


def stats64(z):
    """mean, biased variance (as the kernel forms it: E[z^2] - m^2, clamped at 0) over the plane: [N, 1, C]"""
    m = z.mean(1, keepdim=True)
    var = ((z * z).mean(1, keepdim=True) - m * m).clamp_min(0.0)
    return m, var


def chain(pl):
    """longest fp32 accumulation chain of a plane's statistics: a lane's rows / PL adds, the shuffle steps, the four-wave fold;
    everything across workgroups is double"""
    return pl['rows'] // pl['PL'] + 6 + 4


def stat_bounds(z, dz, pl, eps):
    """(m, var, r, dm, dr) of a plane of values z that the kernel knows to within dz (per element): the dm / dvar / dr formulas of
    tests/test_norm_kernels_gpu.py test_inorm_fwd_bwd; the product z * z is one more rounding than the sum's"""
    n = chain(pl)
    m, var = stats64(z)
    r = 1.0 / torch.sqrt(var + eps)
    dm = n * U24 * z.abs().mean(1, keepdim=True) + U24 * m.abs() + dz.mean(1, keepdim=True)
    dvar = (n + 1) * U24 * (z * z).mean(1, keepdim=True) + 2 * m.abs() * dm + (2 * z.abs() * dz + dz * dz).mean(1, keepdim=True)
    dr = 0.5 * (var + eps - dvar).clamp_min(eps / 2) ** -1.5 * dvar + U24 * r
    return m, var, r, dm, dr


# ---- exact data ------------------------------------------------------------------------------------------------------------------
def exact_eps(HW):
    """even planes: the default 1e-5; odd planes: 1 / HW as fp32, so that var(p) + eps = (HW - 1) / HW + 1 / HW rounds to rstd = 1.0f"""
    return float(np.float32(1.0 / HW)) if HW & 1 else EPS


def special_channels(C):
    """(the channel whose taps are scaled by 2^-9, the channel whose taps are all zero)"""
    return 0, min(2, C - 1)


def exact_seed(case):
    """the seed of a case's exact data.  A plane of a few pixels has so few elements that one open rounding is more than the 1 %
    the ambiguous share may reach: (9, 3, 2, 2) takes the first seed at which the condition holds"""
    return 17 + sum(case) + (2 if case == (9, 3, 2, 2) else 0)


def normal_seed(case):
    return 29 + sum(case)


def exact_inputs(case, seed):
    """p: a balanced arrangement of +1 / -1 per (image, channel), a single 0 where HW is odd (mean exactly 0, every fp32 sum exact);
    r: integers in [-3, 3], where r = -p (u = r + p rstd_p would cancel to ~1e-5 instead of an integer) r = p instead;
    x of PLAIN: integers in [-3, 3]; taps: integers in [-2, 2] with an odd sum per channel, one channel all zero, one scaled by 2^-9 (var(d) of the order of eps)"""
    C, H, W, N = case
    HW = H * W
    g = torch.Generator().manual_seed(seed)
    base = torch.cat([torch.ones(HW // 2), -torch.ones(HW // 2), torch.zeros(HW & 1)]).double()
    p = base[torch.rand(N, HW, C, generator=g).argsort(1)]
    r = torch.randint(-3, 4, (N, HW, C), generator=g).double()
    r = torch.where((r == -p) & (p != 0), p, r)
    u = torch.randint(-3, 4, (N, HW, C), generator=g).double()
    w = torch.randint(-2, 3, (C, 9), generator=g).double()
    small, zero = special_channels(C)
    # an odd tap sum per channel: NORM_RELU's u is 0 or 1 with mean 1/2, so d is an integer and its mean lies near a half-integer --
    # with an even sum a whole cluster of equal d sits next to the mean, where y = (d - m) r cancels and its bf16 rounding is open
    even = w.sum(1) % 2 == 0
    w[even, 4] += torch.where(w[even, 4] < 2, 1.0, -1.0).double()
    w[small] *= 2.0 ** -9
    if zero != small:
        w[zero] = 0.0
    return dict(case=case, p=p, r=r, u=u, w=w, eps=exact_eps(HW))


def tie_margin(v):
    """distance of v from the nearest bf16 rounding tie, in bf16 ulps of v (0.5: v is a bf16 number; 0: v is a tie)"""
    b = rb64(v)
    ulp = torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(1e-300))) - 7)
    return 0.5 - (v - b).abs() / ulp


def exact_ref(mode, dat, pl):
    """The result of the launch on exact_inputs, known to the bit but for the last roundings.  u is exact (its bf16 rounding is
    asserted to be far from a tie), d is an exact fp32 value and every fp32 sum the kernel forms stays below 2^24 in units of its
    terms' last bit (asserted here per workgroup).  The roundings left -- rstd_d to fp32, (float)m, m r, d sc, the add -- move y by
    at most 5 * 2^-24 (|d| r + |m| r): y must lie in [bf16(y64 - win), bf16(y64 + win)], win = 8 * 2^-24 (|d| r + |m| r).  Rounding is
    monotonic, so that is bf16(y64) itself wherever the two ends agree; where they differ (y64 within win of a tie: the ambiguous
    set) they are neighbours and either is allowed -- or y64 is 0 but for the roundings (a constant d) and the window is all there is."""
    C, H, W, N = dat['case']
    HW, eps, w = H * W, dat['eps'], dat['w']
    if mode == PLAIN:
        u = dat['u']
    else:
        p = dat['p']
        cnt = float(HW - (HW & 1))
        assert bool((p.sum(1) == 0).all()) and bool(((p * p).sum(1) == cnt).all())
        var = cnt * (1.0 / HW)
        rp = float(np.float32(1.0 / np.sqrt(var + np.float64(eps))))
        assert abs(rp - 1.0) < 2.0 ** -9, 'rstd_p = %r: relu(+-rstd_p) would not round to 1' % rp
        u64 = (p * rp).clamp_min(0.0) if mode == NORM_RELU else dat['r'] + p * rp
        nz = u64 != 0
        assert float(tie_margin(u64[nz]).min()) > 2.0 ** -10, 'u within 2^-10 ulp of a bf16 tie: the fp32 step could flip it'
        u = rb64(u64)
        assert bool((u == u.round()).all()) and float(u.abs().max()) <= 4, 'u is not an integer in [-4, 4]'
    d = conv64(u, w, H, W)
    assert bool((d == d.float().double()).all())
    # exact sums: in units of the channel's last bit (1, or 2^-9 for the scaled channel) the sums of |d| and d^2 of a workgroup's
    # rows -- and of every partial sum of the nine products -- stay below 2^24
    q = torch.ones(C, dtype=torch.float64)
    q[special_channels(C)[0]] = 2.0 ** -9
    di = d / q
    assert bool((di == di.round()).all())
    rows = pl['rows']
    pad = torch.zeros(N, pl['S'] * rows, C, dtype=torch.float64)
    pad[:, :HW] = di
    wg = pad.view(N, pl['S'], rows, C)
    big = max(float((wg * wg).sum(2).max()), float(wg.abs().sum(2).max()), float(conv64(u.abs(), (w / q[:, None]).abs(), H, W).max()))
    assert big < 2.0 ** 24, 'an fp32 sum of the exact data reaches %g' % big
    m, var = stats64(d)
    rd = 1.0 / torch.sqrt(var + eps)
    y64 = d * rd - m * rd
    win = 8 * U24 * (d.abs() * rd + m.abs() * rd)
    lo, hi = rb64(y64 - win), rb64(y64 + win)
    return dict(u=u, d=d, y64=y64, lo=lo, hi=hi, ambiguous=float((lo != hi).double().mean()), big=big)


def exact_faults(ref, y, u_out=None):
    """(elements of y that are neither allowed value, elements of u_out that differ from the exact u)"""
    y = y.double()
    bad_y = int((~((y >= ref['lo']) & (y <= ref['hi']))).sum())
    bad_u = 0 if u_out is None else int((u_out.double() != ref['u']).sum())
    return bad_y, bad_u


# ---- normal data, per element against float64 -----------------------------------------------------------------------------------
def normal_channels(C):
    """(the channel of large mean, the dead channel)"""
    return 0, min(1, C - 1)


def normal_inputs(case, seed):
    """bf16-rounded normals with per-channel mean and spread; channel 0 (C > 1) has |mean| = 20 sigma; one channel of x is all zero
    (RESIDUAL: u_out = r there; PLAIN / NORM_RELU: u = 0 and y = 0 exactly)"""
    C, H, W, N = case
    g = torch.Generator().manual_seed(seed)
    std, mu = 0.5 + 1.5 * torch.rand(C, generator=g), 2 * torch.rand(C, generator=g) - 1
    big, dead = normal_channels(C)
    mu[big] = 20 * std[big]
    x = torch.randn(N, H * W, C, generator=g) * std + mu
    x[:, :, dead] = 0.0
    r = torch.randn(N, H * W, C, generator=g)
    w = (torch.randn(C, 9, generator=g) * 0.4).float().double()
    return dict(case=case, x=rb64(x), r=rb64(r), w=w, eps=EPS)


def normal_ref(mode, dat, pl, u_kernel=None):
    """float64 reference of u_out and y with per-element bounds, stage by stage as the kernel text goes:
    statistics of p (stat_bounds) -> usc = r_p, usf = 0 - (float)m_p r_p (one rounding);  u = p usc + usf (two), relu, + r (one more,
    RESIDUAL): du = |p| dr + dm r + |m| dr + K 2^-24 M_u with K = 3 (NORM_RELU) or 4 (RESIDUAL), M_u = |p| r + |m| r (+ |r|), then one
    bf16 rounding.  RESIDUAL: u_out is checked against that, and the kernel's own u_out (u_kernel) then feeds the reference of y,
    so du drops out of y's bound.  NORM_RELU: the kernel's u is bf16(u64 + e), |e| <= du, which differs from bf16(u64) only where
    the two ends of that interval round differently: eu = |bf16(relu(v + du)) - bf16(relu(v - du))| (zero almost everywhere),
    carried through d as sum |w| eu.  d: nine products and nine adds in one chain, ten roundings on sum |w||u|.  Statistics of d:
    stat_bounds with dd.  y = d sc + sf: r_d (dd + dm_d) + |d - m_d| dr_d + 3 * 2^-24 (|d| r_d + |m_d| r_d), then the bf16 rounding."""
    C, H, W, N = dat['case']
    x, w, eps = dat['x'], dat['w'], dat['eps']
    out = {}
    zero = torch.zeros_like(x)
    if mode == PLAIN:
        u, eu = x, zero
    else:
        m, var, rr, dm, dr = stat_bounds(x, zero, pl, eps)
        v = (x - m) * rr
        Mu = x.abs() * rr + m.abs() * rr
        if mode == RESIDUAL:
            u64 = dat['r'] + v
            du = x.abs() * dr + dm * rr + m.abs() * dr + 4 * U24 * (Mu + dat['r'].abs())
            out['u'] = (u64, du + BF16 * (u64.abs() + du))
            u, eu = (u_kernel.double() if u_kernel is not None else rb64(u64)), zero
        else:
            du = x.abs() * dr + dm * rr + m.abs() * dr + 3 * U24 * Mu
            u = rb64(v.clamp_min(0.0))
            eu = (rb64((v + du).clamp_min(0.0)) - rb64((v - du).clamp_min(0.0))).abs()
    d = conv64(u, w, H, W)
    dd = 10 * U24 * conv64(u.abs(), w.abs(), H, W) + conv64(eu, w.abs(), H, W)
    m, var, rr, dm, dr = stat_bounds(d, dd, pl, eps)
    y64 = (d - m) * rr
    dy = rr * (dd + dm) + (d - m).abs() * dr + 3 * U24 * (d.abs() * rr + m.abs() * rr)
    out.update(y=(y64, dy + BF16 * (y64.abs() + dy)), d=d, u_ref=u, eu_share=float((eu > 0).double().mean()))
    return out


def normal_check(mode, dat, pl, y, u_out=None, what=''):
    """per-element check of a launch's y (and u_out) on normal_inputs: the worst err / bound ratios; raises where one is over"""
    ref = normal_ref(mode, dat, pl, u_kernel=u_out)
    ratios = {}
    if mode == RESIDUAL:
        ratios['u'] = within(u_out, ref['u'][0], ref['u'][1], what + ' u_out')
        dead = normal_channels(dat['case'][0])[1]
        assert bool((u_out[:, :, dead].double() == dat['r'][:, :, dead]).all()), what + ': u_out != r in the dead channel'
    ratios['y'] = within(y, ref['y'][0], ref['y'][1], what + ' y')
    if mode != RESIDUAL:
        dead = normal_channels(dat['case'][0])[1]
        assert bool((y[:, :, dead].double() == 0).all()), what + ': y != 0 in the dead channel'
    return ratios


def old_bar(y, y64):
    """the whole-tensor bar of tests/test_resnet_infer_gpu.py test_dw_inorm_against_fp32: (accepted, max, mean)"""
    e = (y.double() - y64).abs()
    mx, mean = float(e.max()), float(e.mean())
    return bool(mx <= 3e-2 and mean <= 4e-3), mx, mean


# ---- the kernel's order on the CPU, with named defects ----------------------------------------------------------------------------
DEFECTS = ('halo_top', 'halo_bottom', 'reflect_col', 'reflect_row', 'keep_lo', 'p1_unclipped', 'u_unrounded', 'unbiased', 'eps_dropped',
           'own_rows', 'second_reads_first', 'uout_last', 'pad_u', 'bias')
GARBAGE = 0.37          # what LDS outside the words a tile wrote, and memory past the last image, hold in the emulation


def _reflect(i, n, off_by_one):
    return torch.where(i < 0, -i, torch.where(i >= n, 2 * (n - 1) - i + (1 if off_by_one else 0), i))


def emulate(mode, x, r, w, eps, H, W, pl, defect=None, pad_r=1.0):
    """dw_inorm_kernel in fp32 on the CPU for all channels of x at once under the plan pl (the channels of a launch are independent
    but for the plan): workgroup s owns pixels [s rows, (s + 1) rows); lane sums in fp32 (pixel i of a workgroup belongs to lane
    i mod PL and is added in order; the lanes are then folded in fp32, in torch's order, not the kernel's), partials published to a
    half of the workspace and folded in double; sweeps in tiles of pl['tile'] with u of [lo, hi) made once into an LDS tile that
    keeps what earlier tiles left (GARBAGE at first); RESIDUAL stores u_out in the first sweep; d is recomputed in the last.
    Returns y, u_out [N, HW, C] (float64 of the bf16 values) and the value the pad lanes of u_out hold."""
    assert defect is None or defect in DEFECTS
    f = torch.float32
    N, HW, C = x.shape
    S, rows, PL, tile = pl['S'], pl['rows'], pl['PL'], pl['tile']
    cap, guard = TILE_BYTES // (pl['CHg'] * 16), W + 2
    xf, wf = x.to(f), w.to(f)
    rf = r.to(f) if r is not None else None
    inv_hw = 1.0 / HW
    bias = (1e5 * (1 + torch.arange(C, dtype=torch.float64)) + 0.3).to(f)
    tail = torch.full((rows, C), GARBAGE, dtype=f)

    def rows_of(t, a, b):
        """pixels [a, b) of every image of t; past the plane: the next image's, past the last image GARBAGE"""
        if b <= HW:
            return t[:, a:b]
        flat = torch.cat([t.reshape(N * HW, C), tail])
        return torch.stack([flat[n * HW + a:n * HW + b] for n in range(N)])

    def span(s):
        p0 = s * rows
        return p0, (p0 + rows if defect == 'p1_unclipped' else min(p0 + rows, HW))

    def lane_sums(v):
        n = v.shape[1]
        steps = -(-n // PL)
        pad = torch.zeros((N, steps * PL, C), dtype=f)
        pad[:, :n] = v
        pad = pad.view(N, steps, PL, C)
        acc = torch.zeros((N, PL, C), dtype=f)
        for k in range(steps):
            acc = acc + pad[:, k]
        return acc.sum(1)

    ws = {0: torch.zeros((S, 2, N, C), dtype=f), 1: torch.zeros((S, 2, N, C), dtype=f)}

    def exchange(parts, half):
        """parts [S][2, N, C] -> the totals every workgroup folds: [S][2, N, 1, C] double"""
        ws[half] = torch.stack(parts)
        src = ws[0] if (half == 1 and defect == 'second_reads_first') else ws[half]
        tot = src.double().sum(0)
        if half == 0 and defect == 'own_rows':
            return [ws[0][s].double()[:, :, None] for s in range(S)]
        return [tot[:, :, None]] * S

    def coeffs(tot, second):
        m = tot[0] * inv_hw
        var = tot[1] * inv_hw - m * m
        if second and defect == 'unbiased':
            var = var * HW / (HW - 1)
        var = var.clamp_min(0.0)
        rr = (1.0 / torch.sqrt(var + (0.0 if second and defect == 'eps_dropped' else eps))).to(f)
        return rr, torch.zeros((), dtype=f) - m.to(f) * rr

    ucoef = None
    if mode != PLAIN:
        parts = []
        for s in range(S):
            p0, p1 = span(s)
            v = rows_of(xf, p0, p1)
            parts.append(torch.stack([lane_sums(v), lane_sums(v * v)]))
        ucoef = [coeffs(t, False) for t in exchange(parts, 0)]

    def load_u(s, a, b, coef=None):
        """(what the tile holds, what RESIDUAL stores) of pixels [a, b)"""
        o = xf[:, a:b]
        if mode == PLAIN:
            return o, o
        sc, sf = coef if coef is not None else ucoef[s]
        o = o * sc + sf
        o = o.clamp_min(0.0) if mode == NORM_RELU else o + rf[:, a:b]
        ob = o.bfloat16().to(f)
        return (o if defect == 'u_unrounded' else ob), ob

    y = torch.full((N * HW + rows, C), GARBAGE, dtype=f)
    u_out = torch.zeros((N, HW, C), dtype=f)
    img = torch.arange(N)[:, None] * HW

    def sweep(last, dcoef):
        parts = []
        for s in range(S):
            p0, p1 = span(s)
            lds = torch.full((N, cap + 2 * guard, C), GARBAGE, dtype=f)
            ds = []
            for t0 in range(p0, p1, tile):
                t1 = min(t0 + tile, p1)
                base = p0 if defect == 'keep_lo' else t0
                lo = max(base - W - 1 + (1 if defect == 'halo_top' else 0), 0)
                hi = min(t1 + W + 1 - (1 if defect == 'halo_bottom' else 0), HW)
                held, stored = load_u(s, lo, hi)
                keep = min(hi - lo, cap)                # words past the tile land on the taps: lost to the tile
                lds[:, guard:guard + keep] = held[:, :keep]
                a, b = min(t0, HW), min(t1, HW)
                if mode == RESIDUAL and a < b:
                    if not last and defect != 'uout_last':
                        u_out[:, a:b] = stored[:, a - lo:b - lo]
                    if last and defect == 'uout_last':
                        u_out[:, a:b] = load_u(s, a, b, dcoef[s])[1]
                p = torch.arange(t0, t1)
                py = p // W
                px = p - py * W
                d = torch.zeros((N, t1 - t0, C), dtype=f)
                for ky in range(3):
                    sy = _reflect(py + ky - 1, H, defect == 'reflect_row')
                    for kx in range(3):
                        q = sy * W + _reflect(px + kx - 1, W, defect == 'reflect_col')
                        d = d + wf[:, ky * 3 + kx] * lds[:, (q - lo).clamp(-guard, cap + guard - 1) + guard]
                if defect == 'bias':
                    d = d + bias
                if not last:
                    ds.append(d)
                else:
                    sc, sf = dcoef[s]
                    y[(img + p[None]).reshape(-1)] = (d * sc + sf).bfloat16().to(f).reshape(-1, C)
            if not last:
                dall = torch.cat(ds, 1)
                parts.append(torch.stack([lane_sums(dall), lane_sums(dall * dall)]))
        return parts

    dcoef = [coeffs(t, True) for t in exchange(sweep(False, None), 1)]
    sweep(True, dcoef)
    return y[:N * HW].reshape(N, HW, C).double(), u_out.double(), (pad_r if defect == 'pad_u' else 0.0)
