"""Exact-integer data, float64 references, per-element bounds, the case tables and a CPU emulation for the bf16 training
convolutions (conv_igemm.hip, igemm_kernel_body.inc, conv_halo.hip, conv_ring3.hip, conv_thinout.hip, conv_wgrad.hip), shared by
tests/test_conv_bf16_exact_gpu.py and tests/test_conv_bounds_cpu.py (no tests here).

Why integers: the product of two bf16 values is exact in fp32, and a sum of integers whose running magnitude stays below 2^24 is
exact in fp32 in ANY order -- every tile shape, K split, pair combine, slab fold and phase.  f2bf (common.hpp) is one
round-to-nearest-even.  So on 'int' data a forward / data-gradient output has ONE right value, exact.float().bfloat16(), and a
weight gradient (fp32) is the exact integer; every route must produce those bits.

Tensors here are NCHW float64 on the CPU; a geometry is g = (N, H, W, Ci, Co, k, stride, pad).

The second half of the module does the same for the eval-mode (inference) convolutions gcc_conv_fprop_eval and gcc_conv_eval_ex
(tests/test_conv_eval_exact_gpu.py): data that stays exact behind the affine epilogue, references, bound_eval, an emulation of the
two epilogues with named defects, the case table and the host-side route queries."""
import contextlib
import ctypes as C

import torch
import torch.nn.functional as F

from tests._perelem import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, BF16, U24, act_fn, rb64

SLOPE = 0.25                 # a power of two: LeakyReLU of an integer below 2^24 is exact in fp32
EXACT_LIMIT = 2.0 ** 24
# the device library's tanhf is documented (HIP math API, single precision) with a maximum error of 2 ulps; |tanh| <= 1
# (tests/test_conv_f32_unet_gpu.py TANH_ERR)
TANH_ERR = 2 * 2.0 ** -23
BK = 64                      # igemm_common.hpp: K entries per k-step


def ceil8(v):
    return (v + 7) & ~7


def cdiv(a, b):
    return -(-a // b)


def out_hw(g):
    N, H, W, Ci, Co, k, s, p = g
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def k_products(g, op):
    """products per output element: fprop Ci k^2; dgrad Co ceil(k / s)^2 (the taps of the fullest stride phase); wgrad N Ho Wo"""
    N, H, W, Ci, Co, k, s, p = g
    Ho, Wo = out_hw(g)
    return {'F': Ci * k * k, 'D': Co * cdiv(k, s) ** 2, 'W': N * Ho * Wo}[op]


# ---- data ------------------------------------------------------------------------------------------------------------------------
def make_data(kind, g, seed, xmax=3):
    """x [N,Ci,H,W], w [Co,Ci,k,k], dy [N,Co,Ho,Wo], bias_y [Co], bias_x [Ci] (float64, every value bf16-representable except the
    fp32 biases).
    'int': x, dy uniform integers in [-3, 3] (xmax: a narrower range); w an asymmetric function of the flat index, ((idx * 7919) % m) - m // 2 with m = 509
    (|w| <= 254, exact in bf16) narrowed to 127 / 31 / 7 until max(Ci, Co) k^2 * 3 * (m // 2) + 8 < 2^24 (the worst case of any
    output's magnitude sum, so the exactness condition holds by construction); integer biases in [-8, 8].
    'tiny': x, w, dy in {-1, 0, 1} with density min(1, 4 / sqrt(K)): outputs are integers of a few units, equal to their bf16
    rounding, and a channel's sums of |y| and y^2 stay far below 2^24.
    'normal': seeded normal data rounded to bf16, weights scaled by 1 / sqrt(K); fp32 biases of scale 0.1."""
    N, H, W, Ci, Co, k, s, p = g
    Ho, Wo = out_hw(g)
    gen = torch.Generator().manual_seed(seed)
    if kind == 'int':
        kmax = max(Ci, Co) * k * k
        m = next(m for m in (509, 127, 31, 7) if kmax * 3 * (m // 2) + 8 < EXACT_LIMIT)
        idx = torch.arange(Co * Ci * k * k, dtype=torch.int64).view(Co, Ci, k, k)
        w = (((idx * 7919) % m) - m // 2).double()
        ri = lambda *sh: torch.randint(-xmax, xmax + 1, sh, generator=gen).double()
        return dict(x=ri(N, Ci, H, W), w=w, dy=ri(N, Co, Ho, Wo), bias_y=torch.randint(-8, 9, (Co,), generator=gen).double(),
                    bias_x=torch.randint(-8, 9, (Ci,), generator=gen).double())
    if kind == 'tiny':
        def tern(K, *sh):
            dens = min(1.0, 4.0 / K ** 0.5)
            return (torch.randint(0, 2, sh, generator=gen) * 2 - 1).double() * (torch.rand(sh, generator=gen) < dens)
        return dict(x=tern(Ci * k * k, N, Ci, H, W), w=tern(max(Ci, Co) * k * k, Co, Ci, k, k), dy=tern(Co * k * k, N, Co, Ho, Wo),
                    bias_y=torch.zeros(Co, dtype=torch.float64), bias_x=torch.zeros(Ci, dtype=torch.float64))
    assert kind == 'normal'
    rn = lambda *sh: torch.randn(*sh, generator=gen)
    return dict(x=rb64(rn(N, Ci, H, W)), w=rb64(rn(Co, Ci, k, k) / (Ci * k * k) ** 0.5), dy=rb64(rn(N, Co, Ho, Wo)),
                bias_y=(0.1 * rn(Co)).float().double(), bias_x=(0.1 * rn(Ci)).float().double())


# ---- float64 references --------------------------------------------------------------------------------------------------------
def ref_fprop(d, g, bias=False, act=ACT_NONE):
    """(activated output, pre-activation, magnitude): magnitude = the same convolution of |x| and |w|, plus |bias|"""
    s, p = g[6], g[7]
    pre = F.conv2d(d['x'], d['w'], None, stride=s, padding=p)
    mag = F.conv2d(d['x'].abs(), d['w'].abs(), None, stride=s, padding=p)
    if bias:
        pre = pre + d['bias_y'][None, :, None, None]
        mag = mag + d['bias_y'].abs()[None, :, None, None]
    return act_fn(pre, act, SLOPE), pre, mag


def ref_dgrad(d, g, bias=False, act=ACT_NONE):
    N, H, W, Ci, Co, k, s, p = g
    pre = torch.nn.grad.conv2d_input((N, Ci, H, W), d['w'], d['dy'], stride=s, padding=p)
    mag = torch.nn.grad.conv2d_input((N, Ci, H, W), d['w'].abs(), d['dy'].abs(), stride=s, padding=p)
    if bias:
        pre = pre + d['bias_x'][None, :, None, None]
        mag = mag + d['bias_x'].abs()[None, :, None, None]
    return act_fn(pre, act, SLOPE), pre, mag


def ref_wgrad(d, g):
    N, H, W, Ci, Co, k, s, p = g
    dw = torch.nn.grad.conv2d_weight(d['x'], (Co, Ci, k, k), d['dy'], stride=s, padding=p)
    mag = torch.nn.grad.conv2d_weight(d['x'].abs(), (Co, Ci, k, k), d['dy'].abs(), stride=s, padding=p)
    return dw, mag


def reference(op, d, g, bias=False, act=ACT_NONE):
    if op == 'W':
        dw, mag = ref_wgrad(d, g)
        return dw, dw, mag
    return (ref_fprop if op == 'F' else ref_dgrad)(d, g, bias, act)


def assert_exact_condition(mag, what):
    """on the reference alone, before anything from the GPU is looked at"""
    assert float(mag.max()) < EXACT_LIMIT, '%s: magnitude sum %.4g is not below 2^24: the data does not make the result exact' % (what, float(mag.max()))


def expected_bits(ref):
    """the one right bf16 output of an exact case: a single round-to-nearest-even of the exact fp32 value"""
    return ref.float().bfloat16()


def stats_reference(ref):
    """[2, C] float64 sums over a channel of y_r and y_r^2, y_r = bf16(y), with the exactness condition of the sums"""
    yr = rb64(ref)
    s1, s2 = yr.sum((0, 2, 3)), (yr * yr).sum((0, 2, 3))
    assert float(yr.abs().sum((0, 2, 3)).max()) < EXACT_LIMIT and float(s2.max()) < EXACT_LIMIT
    return torch.stack([s1, s2]), torch.equal(yr, ref)


def rounded_sum_reference(ref):
    """[C] float64 sum over a channel of y_r = bf16(y) on 'int' data, where rounding matters (|y| > 256).  The y_r are integers, so
    their fp32 sum is exact in any order while sum |y_r| < 2^24 (asserted); also says whether the sum of the UNROUNDED outputs
    differs in some channel (then the row tells the two conventions apart)"""
    yr = rb64(ref)
    ok = float(yr.abs().sum((0, 2, 3)).max()) < EXACT_LIMIT
    return yr.sum((0, 2, 3)), ok, bool((yr.sum((0, 2, 3)) != ref.sum((0, 2, 3))).any())


# ---- per-element bounds (derived, not tuned) -------------------------------------------------------------------------------------
def bound_out(ref, mag, K, S, act=ACT_NONE):
    """bf16 output of a forward / data gradient.  A = (K + S + 4) 2^-24 mag bounds the fp32 value in front of the rounding: K
    products accumulated (one rounding per addition, any order), S slices folded, 4 for the bias add, the activation's multiply
    and the fold's adds (no route's code shows more roundings than these counts allow).  The activations
    have slope in [0, 1] (1-Lipschitz): the pre-activation error carries through unchanged; tanh adds the device function's
    documented error.  Then one rounding to bf16 of a value within A of ref."""
    A = (K + S + 4) * U24 * mag
    if act == ACT_TANH:
        A = A + TANH_ERR
    return A + BF16 * (ref.abs() + A)


def bound_wgrad(mag, M, S, old=None):
    """fp32 weight gradient: M = N Ho Wo products, S pixel splits folded, 2 for the fold's adds; accumulating adds one rounding
    of the sum with the old contents"""
    b = (M + S + 2) * U24 * mag
    return b + U24 * old.abs() if old is not None else b


# ---- CPU emulation with named defects (tests/test_conv_bounds_cpu.py only) -----------------------------------------------------------
DEFECTS = ('drop_last_kstep', 'drop_border_tap', 'round_partials_bf16', 'truncate', 'bias_after_round', 'double_count_slice')


def _trunc_bf16(v):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def conv_emul(d, g, bias=False, act=ACT_NONE, S=1, defect=None):
    """forward convolution the way the kernels form it: K = k^2 Ci products (tap-major, channels inside, BK per k-step) accumulated
    in fp32, in S slices of whole k-steps that are folded in fp32, bias, activation, ONE rounding to bf16.  Returns float64.
    Defects: drop_last_kstep (a loop tail loses the last k-step), drop_border_tap (a bounds check treats the last input column as
    padding), round_partials_bf16 (slices rounded to bf16 before the fold), truncate (the output truncated, not rounded),
    bias_after_round (bias added to the rounded sum, rounded again), double_count_slice (the last slice folded twice)."""
    assert defect is None or defect in DEFECTS
    N, H, W, Ci, Co, k, s, p = g
    Ho, Wo = out_hw(g)
    x = d['x'].float()
    if defect == 'drop_border_tap':
        x = x.clone()
        x[..., W - 1] = 0
    cols = F.unfold(x, k, padding=p, stride=s).view(N, Ci, k * k, Ho * Wo).permute(0, 2, 1, 3).reshape(N, k * k * Ci, Ho * Wo)
    wm = d['w'].float().permute(0, 2, 3, 1).reshape(Co, k * k * Ci)
    K = k * k * Ci
    nk = cdiv(K, BK)
    if defect == 'drop_last_kstep':
        wm = wm.clone()
        wm[:, (nk - 1) * BK:] = 0
    kper = cdiv(nk, S)
    parts = [torch.matmul(wm[:, a * BK:min(K, (a + kper) * BK)], cols[:, a * BK:min(K, (a + kper) * BK)]) for a in range(0, nk, kper)]
    if defect == 'round_partials_bf16':
        parts = [q.bfloat16().float() for q in parts]
    if defect == 'double_count_slice':
        parts.append(parts[-1])
    acc = parts[0]
    for q in parts[1:]:
        acc = acc + q
    acc = acc.view(N, Co, Ho, Wo)
    b = d['bias_y'].float()[None, :, None, None] if bias else None
    if defect == 'bias_after_round' and bias:
        acc = acc.bfloat16().float()
    if b is not None:
        acc = acc + b
    v = act_fn(acc, act, SLOPE)
    return (_trunc_bf16(v) if defect == 'truncate' else v.bfloat16().float()).double()


def emul_plain(op, d, g, bias=False, act=ACT_NONE):
    """the operation in fp32 torch on the CPU, rounded once where the kernels round: dgrad / wgrad of the no-defect check"""
    N, H, W, Ci, Co, k, s, p = g
    if op == 'W':
        return torch.nn.grad.conv2d_weight(d['x'].float(), (Co, Ci, k, k), d['dy'].float(), stride=s, padding=p).double()
    v = torch.nn.grad.conv2d_input((N, Ci, H, W), d['w'].float(), d['dy'].float(), stride=s, padding=p)
    if bias:
        v = v + d['bias_x'].float()[None, :, None, None]
    return act_fn(v, act, SLOPE).bfloat16().double()


def old_rule(got, ref, tol=1.2e-2, floor=1e-6):
    """tests/test_kernels_gpu.py close(): max |got - ref| <= tol max |ref| + floor over the whole tensor; returns (passes, err / limit)"""
    err, lim = float((got - ref).abs().max()), tol * float(ref.abs().max()) + floor
    return err <= lim, err / lim


# ---- cases -------------------------------------------------------------------------------------------------------------------
BIG = dict(big_min=1, big_nk=1)          # the 256-pixel tiles (and the halo route) on grids far below a chip's worth of workgroups


def _c(name, op, g, plan=None, opts=None, ws=True, act=ACT_LRELU, bias=True, win=False, stats=False, **expect):
    """one launch under test.  op: 'F' forward, 'D' data gradient, 'W' weight gradient; plan: ops.set_plan fields; opts: option
    name -> value (gcc_set_option); ws: hand the call its split-K workspace; win: operands inside wider, sentinel-filled buffers;
    stats: the statistics tests run it too; expect: route / tile / halo (1 + mode) / split (K slices > 1) / launches / fold (which
    kernel forms the statistic rows of a split launch, see STAT_LAUNCHES) -- what the test asserts BEFORE it compares a number."""
    return dict(name=name, op=op, g=g, plan=plan or {}, opts=opts or {}, ws=ws, act=act, bias=bias, win=win, stats=stats,
                expect=expect)


def _fd(name, g, fe, de, **kw):
    """the forward and the data gradient of one geometry (fe / de: their expectations)"""
    out = []
    if fe is not None:
        out.append(_c(name + '-F', 'F', g, **dict(kw, **fe)))
    if de is not None:
        out.append(_c(name + '-D', 'D', g, **dict(kw, **de)))
    return out


HALO_ON = dict(IGEMM_HALO=3)
CONV_CASES = (
    # ---- igemm_kernel: the tile families (route 0, no halo) ------------------------------------------------------------------
    _fd('t128-ch24-40', (1, 10, 10, 24, 40, 3, 1, 1), dict(tile=128064, stats=True), dict(tile=128032), route=0, halo=0, split=False)
    # three-stage loop, ragged pixel tiles, a channel tail; no workspace: the forward's plan is split (256 statistic rows promised),
    # the un-split launch fills 5 of them and zero-fills the rest
    + _fd('t128-ragged', (3, 20, 36, 64, 48, 4, 2, 1), dict(tile=128064, stats=True, win=True, zero_rows_from=5),
          dict(tile=128064, stats=True, win=True), route=0, halo=0, split=False, ws=False)
    + _fd('t128-k3s2', (2, 16, 16, 16, 32, 3, 2, 1), dict(tile=128032), dict(tile=128016), route=0, halo=0, split=False)   # dgrad: output_padding
    + _fd('t128-1kstep', (2, 8, 8, 64, 64, 1, 1, 0), dict(tile=128064), dict(tile=128064), route=0, halo=0, split=False)   # three stages, ONE k-step
    + _fd('t128x128', (2, 16, 16, 64, 128, 4, 2, 1), dict(tile=128128, split=True), dict(tile=128064, split=False), route=0, halo=0,
          opts=dict(IGEMM_HALO=0))
    + _fd('t256x128-tails', (2, 16, 16, 256, 384, 4, 1, 1), dict(tile=256128, stats=True), dict(tile=256128), route=0, halo=0, split=False,
          plan=dict(tile_families=2, **BIG), opts=dict(IGEMM_HALO=0))           # ragged M (450 rows) and N (384 = 3 x 128) tails
    + _fd('t256x256', (3, 20, 20, 128, 512, 4, 2, 1), dict(tile=256256, stats=True), dict(tile=256128), route=0, halo=0, split=False,
          plan=dict(tile_families=3, **BIG), opts=dict(IGEMM_HALO=0))
    + _fd('t256x256-pair', (2, 8, 8, 256, 256, 4, 2, 1), dict(tile=256256, split=True, launches=1, stats=True), None, route=0, halo=0,
          plan=dict(tile_families=3, pair=1, **BIG), opts=dict(IGEMM_HALO=0))  # two workgroups per tile, K halves combined in the launch
    # ---- split K ------------------------------------------------------------------------------------------------------------
    + _fd('splitk', (2, 4, 4, 512, 512, 4, 2, 1), dict(tile=128128, launches=2, stats=True), dict(tile=128128, launches=2, stats=True), route=0,
          halo=0, split=True, fold='fold_stats')                                                  # K = 8192
    + _fd('splitk-nows', (2, 4, 4, 512, 512, 4, 2, 1), dict(tile=128128, launches=1), dict(tile=128128, launches=1), route=0, halo=0,
          split=False, ws=False)                                               # the same call un-split: same bits on 'int' data
    + _fd('splitk-ntail', (16, 2, 2, 256, 384, 4, 2, 1), dict(tile=128128, launches=2, stats=True), dict(tile=128128, launches=2, stats=True),
          route=0, halo=0, split=True, fold='fold_stats')
    + _fd('splitk-1x1', (1, 4, 4, 8192, 64, 1, 1, 0), dict(tile=128064, launches=2), dict(tile=128032, launches=1, split=False), route=0,
          halo=0, split=True)                                                  # K = 8192 with no padded tap: every output sees all of K
    + _fd('splitk-wide', (2, 4, 4, 64, 2056, 4, 2, 1), dict(tile=128128, launches=2, stats=True), None, route=0, halo=0, split=True,
          fold='channel_stats')
    # (more than 2048 channels: splitk_fold_stats_kernel does not take the layer; statistics by the channel_stats_kernel fallback)
    + [_c('convT-tanh-D', 'D', (2, 16, 16, 24, 64, 4, 2, 1), act=ACT_TANH, route=0, halo=0, tile=128032, split=False)]   # a generator's last layer
    + _fd('s2-dead-edge', (1, 9, 9, 16, 32, 4, 2, 1), None, dict(tile=128016), route=0, halo=0, split=False)   # (H + 2p - k) % s != 0
    + _fd('stem7', (2, 22, 22, 3, 16, 7, 1, 0), dict(tile=128016), dict(tile=128016), route=0, halo=0, split=False)
    + _fd('head7', (2, 22, 22, 16, 3, 7, 1, 0), dict(tile=128016), dict(tile=128016), route=0, halo=0, split=False)
    # ---- thin-input and head routes ---------------------------------------------------------------------------------------------
    + _fd('thin-6-72', (3, 37, 29, 6, 72, 4, 2, 1), dict(route=1, launches=1, win=True), None, halo=0)
    + _fd('thin-3-40', (2, 18, 18, 3, 40, 3, 1, 1), dict(route=1, launches=1), None, halo=0)
    + _fd('thin-dgrad', (3, 20, 28, 5, 56, 4, 2, 1), None, dict(route=1, launches=1, win=True), halo=0)
    + _fd('thin-dgrad-wide', (2, 8, 16, 3, 72, 4, 2, 1), None, dict(route=1, launches=1), halo=0)
    + _fd('head', (2, 8, 8, 256, 1, 4, 1, 1), dict(route=2, launches=2, win=True, head_ks=1), None, halo=0)
    + _fd('head-splitk', (1, 6, 6, 1024, 1, 4, 1, 1), dict(route=2, launches=2, head_ks=4), None, halo=0)
    # ---- conv_thinout.hip -----------------------------------------------------------------------------------------------------
    + _fd('thinout-k9', (1, 36, 70, 32, 3, 9, 1, 4), dict(route=3, launches=1, win=True), dict(route=3, launches=1, bias=False, act=ACT_NONE),
          halo=0)                                                              # 70 columns: just over one 64-column strip; 36 rows = 2 x 2 k: room for two bands
    + _fd('thinout-k3', (2, 13, 40, 8, 1, 3, 1, 1), dict(route=3, launches=1), dict(route=3, launches=1, bias=False, act=ACT_NONE), halo=0)
    # ---- conv_ring3.hip (the smallest geometries R3_MIN_PIXELS = 8192 allows) -----------------------------------------------
    + _fd('ring3-24-20', (1, 96, 96, 24, 20, 3, 1, 1), dict(route=4, launches=1, stats=True, win=True), None, halo=0)    # 20 channels out: pad lanes
    + _fd('ring3-20-24', (1, 96, 96, 20, 24, 3, 1, 1), None, dict(route=4, launches=1), halo=0)
    + _fd('ring3-65col', (1, 127, 65, 8, 16, 3, 1, 1), dict(route=4, launches=1, stats=True), None, halo=0)              # last strip one pixel wide
    + _fd('ring3-65col', (1, 127, 65, 24, 16, 3, 1, 1), None, dict(route=4, launches=1), halo=0)
    + [_c('ring3-act-none-F', 'F', (1, 127, 65, 8, 16, 3, 1, 1), act=ACT_NONE, route=4, launches=1, halo=0),
       _c('ring3-act-relu-F', 'F', (1, 127, 65, 8, 16, 3, 1, 1), act=ACT_RELU, route=4, launches=1, halo=0)]
)
CONV_CASES = tuple(CONV_CASES)


def _halo_cases():
    """conv_halo.hip: every mode on the smallest grid it accepts under big_min = 1 (one image; stride 2: 16 x 64 inputs, a position
    grid of 8 x 32 -- a 16-wide tile's staged neighbourhood, 17 x 24 pixels = 51 pieces, is over HALO_MAX_PIECES = 48; stride 1:
    32 x 32), with 256- and 128-column tiles (halo_hc 0 / 128).  The k4 s2 data gradient of 128 channels is mode 2 (both px phases in one tile) unless
    halo_hc = 128 forces the per-phase form (mode 1)."""
    out = []
    for hc in (0, 128):
        plan = dict(tile_families=3, halo_hc=hc, **BIG)
        tag = '-hc%d' % hc
        out += _fd('halo-m0' + tag, (1, 16, 64, 64, 256, 4, 2, 1), dict(halo=1, stats=True, win=hc == 0), None, route=0, launches=1, plan=plan,
                   opts=HALO_ON)
        out += _fd('halo-m1' + tag, (1, 16, 64, 256, 64, 4, 2, 1), None, dict(halo=2, win=hc == 0), route=0, launches=1, plan=plan, opts=HALO_ON)
        out += _fd('halo-c128' + tag, (1, 16, 64, 128, 64, 4, 2, 1), None, dict(halo=3 if hc == 0 else 2), route=0, launches=1, plan=plan,
                   opts=HALO_ON)
        out += _fd('halo-m3' + tag, (1, 32, 32, 64, 256, 4, 1, 1), dict(halo=4, stats=True), None, route=0, launches=1, plan=plan, opts=HALO_ON)
        out += _fd('halo-m4' + tag, (1, 32, 32, 256, 64, 4, 1, 1), None, dict(halo=5), route=0, launches=1, plan=plan, opts=HALO_ON)
        out += _fd('halo-k3' + tag, (1, 32, 32, 64, 256, 3, 1, 1), dict(halo=4, stats=True), None, route=0, launches=1, plan=plan, opts=HALO_ON)
        out += _fd('halo-k3' + tag, (1, 32, 32, 256, 64, 3, 1, 1), None, dict(halo=5), route=0, launches=1, plan=plan, opts=HALO_ON)
    # the other tile order (HALO_XCD_COLS: one column tile per XCD) needs >= 2 column tiles and a grid that is a multiple of 8
    out += _fd('halo-xcd', (4, 16, 64, 64, 256, 4, 2, 1), dict(halo=1), None, route=0, launches=1, plan=dict(tile_families=3, halo_hc=128, **BIG),
               opts=dict(IGEMM_HALO=3, HALO_XCD_COLS=2))
    return tuple(out)


HALO_CASES = _halo_cases()
FD_CASES = CONV_CASES + HALO_CASES

TS = dict(WGRAD_TS=2)
WGRAD_CASES = (
    # wgrad_kernel, 128 x 128 tiles
    _c('wgrad-direct', 'W', (1, 10, 10, 24, 40, 3, 1, 1), launches=1, splits=1),             # un-split, written directly; ragged columns and Co
    _c('wgrad-ci6', 'W', (2, 16, 16, 6, 128, 4, 2, 1), launches=2, splits=1),                 # 6 channels: the slab + the strided fold
    _c('wgrad-split', 'W', (4, 32, 32, 16, 24, 4, 2, 1), win=True, launches=2, splits=2),     # two pixel slabs + the fold; x, dY in windows
    # 256 x 256 tiles: the smallest geometry of plan_splits' `big`: Co >= 256, 16 * 72 = 1152 >= 256 columns, 5 x 2 = 10 >= 8 tiles,
    # 64 x 64 = 4096 pixels = 64 k-steps; ragged columns (1152 = 4.5 x 256) and channels (264); 4 splits (the 128 x 128 plan: 8)
    _c('wgrad-big', 'W', (1, 65, 65, 72, 264, 4, 1, 1), launches=2, splits=4),
    # tap-stationary (WGRAD_TS = 2), the small members of TS_CASES
    _c('wgrad-ts4-direct', 'W', (2, 9, 21, 64, 64, 4, 1, 1), opts=TS, plan=dict(wgrad_wgs_big=1), launches=1, splits=1),
    _c('wgrad-ts4-split', 'W', (2, 9, 21, 64, 64, 4, 1, 1), opts=TS, plan=dict(wgrad_wgs_big=4), win=True, launches=2, splits=4),
    _c('wgrad-ts3-direct', 'W', (2, 9, 21, 64, 64, 3, 1, 1), opts=TS, plan=dict(wgrad_wgs_big=1), launches=1, splits=1),
    _c('wgrad-ts3-split', 'W', (2, 9, 21, 64, 64, 3, 1, 1), opts=TS, plan=dict(wgrad_wgs_big=8), launches=2, splits=8),
    _c('wgrad-ts4-short', 'W', (1, 5, 40, 64, 192, 4, 1, 1), opts=TS, plan=dict(wgrad_wgs_big=9), launches=2, splits=3),   # one block row, three channel tiles
    _c('wgrad-ts3-short', 'W', (1, 5, 40, 64, 192, 3, 1, 1), opts=TS, plan=dict(wgrad_wgs_big=9), launches=2, splits=3),
    _c('wgrad-ts4-6tiles', 'W', (2, 17, 17, 192, 128, 4, 1, 1), opts=TS, plan=dict(wgrad_wgs_big=6), launches=1, splits=1),  # one block wide, two deep
    _c('wgrad-ts3-6tiles', 'W', (2, 16, 16, 192, 128, 3, 1, 1), opts=TS, plan=dict(wgrad_wgs_big=6), launches=1, splits=1),
    # the head's weight gradient: gather + 1 x 1 wgrad + head_rows_fold_kernel
    _c('wgrad-head', 'W', (2, 8, 8, 256, 1, 4, 1, 1), launches=3, splits=None),
    # conv_thinout.hip: kernel + fold, one slab per workgroup
    _c('wgrad-thinout-k9', 'W', (1, 36, 70, 32, 3, 9, 1, 4), launches=2, splits=None),
    _c('wgrad-thinout-k3', 'W', (2, 13, 40, 8, 1, 3, 1, 1), launches=2, splits=None),
)
# grouped launch: k4 s2, k3, 1 x 1.  group_plan gives a workgroup at least 16 k-steps of 64 pixels: the first layer's 4 x 18 x 18 =
# 1296 pixels are 21 k-steps, two slabs and the group's fold launch; the other two (286 and 432 pixels) are written directly
GROUP_LAYERS = ((4, 36, 36, 16, 32, 4, 2, 1), (2, 11, 13, 24, 40, 3, 1, 1), (3, 12, 12, 48, 16, 1, 1, 0))


def case_seed(case):
    return sum(ord(ch) for ch in case['name']) + sum(case['g'])


# ---- host-side routing (no GPU: the library's plan functions only) ---------------------------------------------------------
def desc(lib_mod, g, plan, ldx=None, ldy=None):
    N, H, W, Ci, Co, k, s, p = g
    fields = tuple(int(plan.get(f, 0)) for f in lib_mod.PLAN_FIELDS)
    return lib_mod.conv_t(N, H, W, Ci, Co, k, k, s, p, ldx or ceil8(Ci), 0, ldy or ceil8(Co), 0, fields)


@contextlib.contextmanager
def forced_options(lib_mod, opts):
    """gcc_set_option for the block, the previous values back afterwards"""
    lib = lib_mod.load()
    ids = {n: i for i, n in enumerate(lib_mod.OPT_NAMES)}
    prev = {n: lib.gcc_get_option(ids[n]) for n in opts}
    try:
        for n, v in opts.items():
            lib.gcc_set_option(ids[n], v)
        yield
    finally:
        for n, v in prev.items():
            lib.gcc_set_option(ids[n], v)


def routing(lib_mod, case, ep=None, with_stats=False, ld=None, d=None):
    """what the library says a forward / data-gradient call of this case runs on: dict(route, tile, halo, S, stat_tiles, ws).
    ep: the call's real epilogue; None: a stand-in with the same NULL / non-NULL fields (the plan functions only test them).
    S: the K slices folded -- 2 for a pair launch, the split of plan_ksplit read back from gcc_conv_workspace (bytes =
    phases x slices x rows x padded columns x 4) when the call has a workspace, taps x the head route's K slices (read back the same
    way) on the head route, 1 otherwise.  A statistics launch may cap its slices below the plan's: S stays an upper count."""
    lib = lib_mod.load()
    g, dg = case['g'], int(case['op'] == 'D')
    N, H, W, Ci, Co, k, s, p = g
    d = d if d is not None else desc(lib_mod, g, case['plan'], *(ld or (None, None)))
    ws = int(lib.gcc_conv_workspace(C.byref(d), dg)) if case['ws'] else 0
    if ep is None:
        fake = 1 << 20
        ep = lib_mod.epilogue_t(fake if case['bias'] else None, case['act'], SLOPE, fake if with_stats else None, fake if ws else None, ws,
                                None, None, 0, 0, 0, None)
    route = int(lib.gcc_conv_route(C.byref(d), dg, C.byref(ep)))
    tile = int(lib.gcc_conv_tile(C.byref(d), dg))
    halo = int(lib.gcc_conv_halo_mode(C.byref(d), dg, int(with_stats)))
    Ho, Wo = out_hw(g)
    phases = s * s if dg else 1
    rows = N * cdiv(H, s) * cdiv(W, s) if dg else N * Ho * Wo
    cout = Ci if dg else Co
    S, head_ks = 1, 0
    if route == 2:
        head_ks = ws // (N * H * W * 16 * 4)          # head_fprop_workspace: K slices x input pixels x 16 tap columns of fp32
        S = k * k * head_ks                           # head_tapsum_kernel adds every tap's slices
    elif route == 0 and not halo and ws:
        if tile == 256256 and case['plan'].get('pair') == 1:
            S = 2
        elif tile // 1000 == 128:
            bc = tile % 1000
            S = ws // (phases * rows * cdiv(cout, bc) * bc * 4)
    return dict(route=route, tile=tile, halo=halo, S=int(S), head_ks=int(head_ks), rows=rows, phases=phases, stat_tiles=int(lib.gcc_conv_stat_tiles(C.byref(d), dg)), ws=ws)


def check_expect(case, r):
    """the case's intended route against what the library reports (a mismatch is a failure, never a skip)"""
    e = case['expect']
    assert r['route'] == e['route'], '%s: route %d, intended %d' % (case['name'], r['route'], e['route'])
    assert r['halo'] == e['halo'], '%s: halo mode + 1 = %d, intended %d' % (case['name'], r['halo'], e['halo'])
    if 'tile' in e:
        assert r['tile'] == e['tile'], '%s: tile %d, intended %d' % (case['name'], r['tile'], e['tile'])
    if 'head_ks' in e:
        assert r['head_ks'] == e['head_ks'], '%s: %d K slices on the head route, intended %d' % (case['name'], r['head_ks'], e['head_ks'])
    if 'split' in e:
        assert (r['S'] > 1) == e['split'], '%s: %d K slices, intended %s' % (case['name'], r['S'], 'a split' if e['split'] else 'no split')


# launches of a statistics call (no BatchNorm descriptor, so no finalize launch): the un-split / pair / halo / ring-walk launch
# writes its rows itself; a split launch hands raw partial tiles to splitk_fold_stats_kernel (partials + fold); where that kernel does
# not take the layer (more than 2048 channels) the partials are folded by splitk_epilogue_kernel and channel_stats_kernel reads the
# stored tensor (partials + fold + statistics).  The count tells the three apart.
STAT_LAUNCHES = {'none': 1, 'fold_stats': 2, 'channel_stats': 3}


def fold_rows(g, dgrad):
    """statistic rows of splitk_fold_stats_kernel (conv_igemm.hip fold_wpp x phases): about 256 workgroups over all phases, never
    fewer per phase than the 128-row tiles, never more than the rows"""
    N, H, W, Ci, Co, k, s, p = g
    Ho, Wo = out_hw(g)
    phases = s * s if dgrad else 1
    rows = N * cdiv(H, s) * cdiv(W, s) if dgrad else N * Ho * Wo
    return max(1, min(rows, max(256 // phases, cdiv(rows, 128)))) * phases


def check_stats_expect(case, r, launches=None):
    """the statistics launch of a case: the same route, tile, halo mode and split as the plain one (check_expect on the routing
    queried WITH statistic rows), the rows of the kernel that forms them, and -- given the launch count of the call -- which
    kernel that was"""
    check_expect(case, r)
    fold = case['expect'].get('fold', 'none')
    assert (fold != 'none') == (r['S'] > 1 and r['tile'] // 1000 == 128 and r['route'] == 0), (case['name'], fold, r)
    dg = case['op'] == 'D'
    if fold == 'fold_stats':
        assert r['stat_tiles'] == fold_rows(case['g'], dg), (case['name'], r['stat_tiles'], fold_rows(case['g'], dg))
    elif r['route'] == 0 and not r['halo'] and fold == 'channel_stats':
        assert r['stat_tiles'] == cdiv(r['rows'], 128) * r['phases'], (case['name'], r['stat_tiles'])
    if launches is not None:
        assert launches == STAT_LAUNCHES[fold], '%s: %d launches, intended %d (%s)' % (case['name'], launches, STAT_LAUNCHES[fold], fold)


# tests/test_kernels_gpu.py test_halo_conv_vs_torch_and_gather_kernel: 1 + the halo kernel's mode (gcc_conv_halo_mode) of the two
# launches it makes on its IGEMM_HALO = 2 leg -- (forward with statistic rows, data gradient) under halo_hc 0 and under halo_hc 128,
# by (N, H, W, Ci, Co, stride); 0: that launch is igemm_kernel on both legs (fewer than PLAN_BIG_MIN workgroups; a data gradient whose
# width does not tile by 128; a statistics launch whose plan has 128-pixel rows).  tests/test_conv_bf16_exact_gpu.py runs every mode
# on small grids under big_min = 1; tests/test_conv_bounds_cpu.py holds this table to the library's host code.
HALO_LEGS = {(16, 128, 128, 128, 256, 2): ((1, 3), (1, 2)), (16, 64, 64, 256, 512, 2): ((1, 2), (1, 2)),
             (16, 32, 32, 512, 1024, 1): ((4, 5), (4, 5)), (8, 64, 64, 128, 256, 2): ((0, 0), (0, 2)),
             (4, 64, 64, 64, 512, 1): ((4, 0), (4, 0)), (16, 128, 128, 64, 128, 2): ((0, 0), (0, 0))}


def wgrad_splits(lib_mod, case):
    """pixel splits of a weight-gradient call, read back from its workspace: bytes = splits x Co x k^2 x ceil8(Ci) x 4 on the
    column-tiled and tap-stationary kernels (None on the head / thin-output routes, which size theirs differently)"""
    lib = lib_mod.load()
    N, H, W, Ci, Co, k, s, p = case['g']
    d = desc(lib_mod, case['g'], case['plan'])
    ws = int(lib.gcc_conv_wgrad_workspace(C.byref(d)))
    return ws, ws // (Co * k * k * ceil8(Ci) * 4)


def wgrad_counts(case):
    """(M, S) of bound_wgrad for a weight-gradient case.  Column-tiled / tap-stationary kernels: M = N Ho Wo products, S = the
    case's pixel splits.  Head route: the 1 x 1 weight gradient runs over the INPUT grid (the gathered dY holds zeros where a tap
    has no output), M = N H W, its splits at most one per 8 k-steps of 64 pixels (plan_splits).  Thin-output route: one slab per
    unit of work at most, units = N x strips of 64 columns x bands of at least 2 k rows (thinout_plan)."""
    N, H, W, Ci, Co, k, s, p = case['g']
    Ho, Wo = out_hw(case['g'])
    if case['expect']['splits'] is not None:
        return N * Ho * Wo, case['expect']['splits']
    if Co == 1 and ceil8(Ci) >= 256:
        return N * H * W, max(1, cdiv(N * H * W, 64) // 8)
    return N * Ho * Wo, N * cdiv(W, 64) * max(1, H // (2 * k))


# ==================================================================================================================================
# The eval-mode (inference) convolutions: gcc_conv_fprop_eval and gcc_conv_eval_ex -- igemm_epilogue with EPI == 1,
# igemm_epilogue_ex, the ring-walk's EV branch (conv_ring3.hip), and the two fold kernels splitk_epilogue_kernel<true> and
# splitk_eval_ex_kernel.  Shared by tests/test_conv_eval_exact_gpu.py and tests/test_conv_bounds_cpu.py.
#
# An eval geometry is g = (N, H, W, Ci, Co, kh, kw, stride, pad, transposed): H, W, Ci describe the call's INPUT, Co its output
# (transposed: the ConvTranspose2d forward, weight [Ci, Co, kh, kw]; the output is (H - 1) stride - 2 pad + kh high).
#
# Why the exact method still holds behind an affine epilogue: on 'int' data the accumulator is an integer, scale is +-0.5, +-1
# or +-2, shift and residual are integers, the slope is 0.25 or -0.5 -- every intermediate (scale acc, + shift, * slope,
# + residual) is a multiple of 2^-3.  While max |scale| mag + |shift| + |residual| < 2^20 each of them is below 2^20 and so
# has at most 23 bits in front of its last (2^-3) one: it is an fp32 number.  The value in front of the store is therefore
# exact in any summation order, with the multiply and the add fused or not, and the bf16 output has ONE right value.
EV_NONE, EV_PRELU, EV_TANH, EV_RELU, EV_LRELU = 0, 1, 2, 3, 4       # include/gcc_hip.h GCC_EVAL_ACT_*
EVAL_LIMIT = 2.0 ** 20
INT_SCALES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)
INT_SLOPES = (0.25, -0.5)
NORMAL_SLOPES = (0.2, -0.3)


def f32(v):
    """the fp32 number a kernel reads for a Python float, as a float"""
    return float(torch.tensor(v, dtype=torch.float32))


def eval_out_hw(g):
    N, H, W, Ci, Co, kh, kw, s, p, tr = g
    if tr:
        return (H - 1) * s - 2 * p + kh, (W - 1) * s - 2 * p + kw
    return (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1


def eval_k(g):
    """products per output element: Ci kh kw forward; Ci ceil(kh / s) ceil(kw / s) transposed (the fullest stride phase)"""
    N, H, W, Ci, Co, kh, kw, s, p, tr = g
    return Ci * cdiv(kh, s) * cdiv(kw, s) if tr else Ci * kh * kw


def make_eval_data(kind, g, seed):
    """x [N,Ci,H,W], w ([Co,Ci,kh,kw]; transposed [Ci,Co,kh,kw]), scale [Co], shift [Co], residual [N,Co,Ho,Wo] (float64; x, w
    and residual bf16-representable, scale and shift fp32-representable).
    'int': x integers in [-3, 3]; w = ((idx * 7919) % m) - m // 2 with m the widest of 509 / 127 / 31 / 7 for which
    2 (K 3 (m // 2)) + 8 + 64 < 2^20 with the case's OWN K = eval_k(g) (the worst case of max |scale| mag + |shift| + |residual|,
    so the exactness condition holds by construction); scale drawn from +-0.5, +-1, +-2; shift integers in [-8, 8]; residual
    integers in [-64, 64].
    'normal': as make_data, with scale = +-U[0.25, 1.75], shift = 0.3 N(0, 1), a bf16-rounded residual ~ N(0, 1)."""
    N, H, W, Ci, Co, kh, kw, s, p, tr = g
    Ho, Wo = eval_out_hw(g)
    gen = torch.Generator().manual_seed(seed)
    K = eval_k(g)
    wshape = (Ci, Co, kh, kw) if tr else (Co, Ci, kh, kw)
    if kind == 'int':
        m = next(m for m in (509, 127, 31, 7) if 2 * K * 3 * (m // 2) + 8 + 64 < EVAL_LIMIT)
        idx = torch.arange(Co * Ci * kh * kw, dtype=torch.int64).view(wshape)
        w = (((idx * 7919) % m) - m // 2).double()
        ri = lambda lo, hi, *sh: torch.randint(lo, hi + 1, sh, generator=gen).double()
        scale = torch.tensor(INT_SCALES, dtype=torch.float64)[torch.randint(0, len(INT_SCALES), (Co,), generator=gen)]
        return dict(x=ri(-3, 3, N, Ci, H, W), w=w, scale=scale, shift=ri(-8, 8, Co), residual=ri(-64, 64, N, Co, Ho, Wo))
    assert kind == 'normal'
    rn = lambda *sh: torch.randn(*sh, generator=gen)
    sign = torch.where(torch.rand(Co, generator=gen) < 0.5, -1.0, 1.0)
    scale = (sign * (0.25 + 1.5 * torch.rand(Co, generator=gen))).float().double()
    return dict(x=rb64(rn(N, Ci, H, W)), w=rb64(rn(*wshape) / K ** 0.5), scale=scale, shift=(0.3 * rn(Co)).float().double(),
                residual=rb64(rn(N, Co, Ho, Wo)))


def eval_act_fn(v, act, slope):
    """a GCC_EVAL_ACT_* id on float64 (slope: the PReLU / LeakyReLU negative-side factor)"""
    if act == EV_TANH:
        return torch.tanh(v)
    neg = slope if act in (EV_PRELU, EV_LRELU) else (0.0 if act == EV_RELU else 1.0)
    return torch.where(v > 0, v, v * neg)


def eval_conv(d, g):
    """(acc, mag): the convolution (transposed: ref_dgrad's formulation) of x and w, and of |x| and |w|, float64"""
    N, H, W, Ci, Co, kh, kw, s, p, tr = g
    if not tr:
        return F.conv2d(d['x'], d['w'], None, stride=s, padding=p), F.conv2d(d['x'].abs(), d['w'].abs(), None, stride=s, padding=p)
    Ho, Wo = eval_out_hw(g)
    size = (N, Co, Ho, Wo)
    return (torch.nn.grad.conv2d_input(size, d['w'], d['x'], stride=s, padding=p),
            torch.nn.grad.conv2d_input(size, d['w'].abs(), d['x'].abs(), stride=s, padding=p))


def eval_z(d, conv, scale=True, shift=True):
    """(z, mag_z): z = scale[c] acc + shift[c] (a NULL scale is 1, a NULL shift 0) and |scale| mag + |shift|"""
    acc, mag = conv
    z, mz = acc, mag
    if scale:
        z, mz = z * d['scale'][None, :, None, None], mz * d['scale'].abs()[None, :, None, None]
    if shift:
        z, mz = z + d['shift'][None, :, None, None], mz + d['shift'].abs()[None, :, None, None]
    return z, mz


def ref_eval(d, g, act, residual, slope=0.25, scale=True, shift=True, conv=None):
    """gcc_conv_fprop_eval in float64: (y, z, mag) with y = act(z) + residual -- the residual is added AFTER the activation --
    and mag = |scale| conv(|x|, |w|) + |shift| (the residual's magnitude is the caller's to add).  conv: eval_conv(d, g) when the
    caller already has it."""
    z, mz = eval_z(d, conv if conv is not None else eval_conv(d, g), scale, shift)
    y = eval_act_fn(z, act, slope)
    if residual:
        y = y + d['residual']
    return y, z, mz


def ref_eval_ex(d, g, act, act2, slope=0.25, scale=True, shift=True, conv=None):
    """gcc_conv_eval_ex in float64: (y, y2, z, mag) with y = act(z), y2 = act2(z) (None without a second output) -- both from z"""
    z, mz = eval_z(d, conv if conv is not None else eval_conv(d, g), scale, shift)
    return eval_act_fn(z, act, slope), (eval_act_fn(z, act2, slope) if act2 is not None else None), z, mz


def assert_eval_exact_condition(d, conv, what, residual=True):
    """max |scale| mag + |shift| (+ |residual|) < 2^20 on the reference alone, before anything from the GPU is looked at (it
    covers every variant: a NULL scale is 1 <= max |scale|, a NULL shift or residual only lowers the left side)"""
    top = max(1.0, float(d['scale'].abs().max())) * conv[1] + d['shift'].abs()[None, :, None, None]
    if residual:
        top = top + d['residual'].abs()
    assert float(top.max()) < EVAL_LIMIT, '%s: max |scale| mag + |shift| + |residual| = %.4g is not below 2^20' % (what, float(top.max()))
    return float(top.max())


def assert_eval_data_conditions(z, what):
    """conditions on the 'int' data (not measurements): a double rounding can only show where an output is not its own bf16
    rounding, an activation branch only where pre-activations of both signs exist"""
    differ = float((rb64(z) != z).double().mean())
    neg = float((z < 0).double().mean())
    assert differ >= 0.10, '%s: only %.1f %% of the outputs differ from their bf16 rounding' % (what, 100 * differ)
    assert 0.25 <= neg <= 0.75, '%s: %.1f %% of the pre-activations are negative' % (what, 100 * neg)
    return differ, neg


# fp32 roundings on the way to the value that is stored, as igemm_epilogue (EPI == 1), igemm_epilogue_ex, splitk_epilogue_kernel<true>,
# splitk_eval_ex_kernel and the ring-walk's EV branch show them: K products accumulated (one rounding per addition, any order), S
# slices folded (one addition each), and K_EVAL = 4: the scale multiply and the shift add (`sc * acc + sh`: two roundings, one where
# the compiler fuses them), the activation's multiply by the slope, the residual add.  gcc_conv_eval_ex has no residual: its count
# is one lower, the bound keeps the common one.
K_EVAL = 4


def bound_eval(ref, mag_z, K, S, act, residual=None):
    """bf16 output of an eval-mode convolution, per element.  n = K + S + K_EVAL roundings, each relative to at most
    M = |scale| sum |x w| + |shift| (+ |residual|): the value in front of the bf16 rounding is within A = gamma_n M of ref,
    gamma_n = n u / (1 - n u), u = 2^-24.  Every activation is 1-Lipschitz (|slope| <= 1), so the pre-activation error carries
    through unchanged; tanh adds the device function's documented error.  Then one rounding to bf16 of a value within A of ref.
    mag_z: |scale| sum |x w| + |shift|; residual: the residual tensor (its magnitude is added here) or None."""
    M = mag_z + (residual.abs() if residual is not None else 0.0)
    n = (K + S + K_EVAL) * U24
    A = n / (1.0 - n) * M
    if act == EV_TANH:
        A = A + TANH_ERR
    return A + BF16 * (ref.abs() + A)


def old_rule_eval_ex(got, ref):
    """tests/test_unet_infer_gpu.py test_eval_ex_epilogue_against_fp32: max |got - ref| <= 1e-2 max(max |ref|, 1) + 2^-7 max |ref|
    over the whole tensor; returns (passes, err / limit)"""
    top = float(ref.abs().max())
    err, lim = float((got - ref).abs().max()), 1e-2 * max(top, 1.0) + 2.0 ** -7 * top
    return err <= lim, err / lim


# ---- CPU emulation of the two eval epilogues, with named defects (tests/test_conv_bounds_cpu.py only) ----------------------------
EVAL_DEFECTS = ('residual_before_act', 'shift_after_round', 'round_before_residual', 'act2_from_act', 'prelu_slope_ignored',
                'scale_missing_on_fold', 'drop_last_slice', 'pad_lane_gets_shift')
# the entry a defect can occur in: a residual exists in gcc_conv_fprop_eval alone, a second output in gcc_conv_eval_ex alone
DEFECT_ENTRIES = dict(residual_before_act=('eval',), round_before_residual=('eval',), act2_from_act=('ex',))


def eval_emul_parts(d, g, S):
    """the fp32 partial sums of eval_emul: S groups of input channels"""
    N, H, W, Ci, Co, kh, kw, s, p, tr = g
    x, w = d['x'].float(), d['w'].float()
    per = cdiv(Ci, S)
    if tr:
        return [F.conv_transpose2d(x[:, a:a + per], w[a:a + per], None, stride=s, padding=p) for a in range(0, Ci, per)]
    return [F.conv2d(x[:, a:a + per], w[:, a:a + per], None, stride=s, padding=p) for a in range(0, Ci, per)]


def eval_emul(d, g, entry, act, act2=None, residual=False, slope=0.25, scale=True, shift=True, S=1, defect=None, parts=None):
    """conv_emul for the eval epilogues: the products accumulated in fp32 in S slices (here: S groups of input channels, another
    order than any kernel's -- on 'int' data every order gives the same sum) that are folded in fp32, then z = scale acc + shift,
    the activation(s), the residual after the activation, ONE rounding to bf16.  Returns (y, y2) as float64 of ceil8(Co)
    channels: the pad lanes Co .. ceil8(Co) are part of what a call writes (exact zeros).
    Defects: residual_before_act (act(z + residual)); shift_after_round (scale acc rounded to bf16, then the shift, the activation
    and the store's rounding: two roundings); round_before_residual (act(z) rounded, the residual added, rounded again); act2_from_act (y2 = act2(act(z)));
    prelu_slope_ignored (the negative side passes unscaled); scale_missing_on_fold (the fold kernel of a split launch skips the
    scale); drop_last_slice (the fold stops one slice early); pad_lane_gets_shift (the pad lanes are treated as channels with
    scale 0 but the last channel's shift, or 1 where that is zero)."""
    assert defect is None or defect in EVAL_DEFECTS
    assert entry in DEFECT_ENTRIES.get(defect, ('eval', 'ex'))
    N, H, W, Ci, Co, kh, kw, s, p, tr = g
    Ho, Wo = eval_out_hw(g)
    parts = list(parts) if parts is not None else eval_emul_parts(d, g, S)
    if defect == 'drop_last_slice':
        assert len(parts) > 1
        parts = parts[:-1]
    acc = parts[0]
    for q in parts[1:]:
        acc = acc + q
    col = lambda t: t.float()[None, :, None, None]
    if scale and not (defect == 'scale_missing_on_fold' and S > 1):
        acc = acc * col(d['scale'])
    neg = 1.0 if defect == 'prelu_slope_ignored' else slope
    rb = lambda t: t.bfloat16().float()
    if defect == 'shift_after_round':
        z = rb(acc) + col(d['shift']) if shift else rb(acc)
    else:
        z = acc + col(d['shift']) if shift else acc
    res = d['residual'].float() if residual else None
    if defect == 'residual_before_act':
        y = eval_act_fn(z + res, act, neg)
    else:
        y = eval_act_fn(z, act, neg)
        if defect == 'round_before_residual':
            y = rb(y)
        if res is not None:
            y = y + res
    y2 = None
    if act2 is not None:
        y2 = eval_act_fn(eval_act_fn(z, act, neg) if defect == 'act2_from_act' else z, act2, neg)

    def store(v):
        out = torch.zeros((N, ceil8(Co), Ho, Wo), dtype=torch.float64)
        out[:, :Co] = rb(v).double()
        if defect == 'pad_lane_gets_shift':
            out[:, Co:] = float(d['shift'][Co - 1]) or 1.0
        return out
    return store(y), (store(y2) if y2 is not None else None)


def eval_expected(ref, Co):
    """the one right output of an exact eval case over ceil8(Co) lanes: one rounding of the exact value, zeros in the pad lanes"""
    out = torch.zeros((ref.shape[0], ceil8(Co)) + tuple(ref.shape[2:]), dtype=torch.float64)
    out[:, :Co] = rb64(ref)
    return out


# ---- eval cases --------------------------------------------------------------------------------------------------------------------
def _ev_variants(acts, residuals=(False, True), coeffs=((True, True), (False, True), (True, False), (False, False))):
    return tuple(dict(act=a, slope_i=si, residual=r, scale=sc, shift=sh) for a, si in acts for r in residuals for sc, sh in coeffs)


# gcc_conv_fprop_eval, "all": act in NONE, PReLU(first slope), PReLU(second slope), TANH; with and without a residual; scale /
# shift both, scale NULL, shift NULL, both NULL.  slope_i indexes INT_SLOPES / NORMAL_SLOPES.  TANH runs per element only.
EV_ALL = _ev_variants(((EV_NONE, 0), (EV_PRELU, 0), (EV_PRELU, 1), (EV_TANH, 0)))
EV_SR_FIRST = _ev_variants(((EV_PRELU, 0), (EV_PRELU, 1)), residuals=(False,), coeffs=((True, True), (False, True)))
EV_SR_LAST = _ev_variants(((EV_TANH, 0), (EV_NONE, 0)), residuals=(False,), coeffs=((False, True),))
EV_DRN = _ev_variants(((EV_NONE, 0),), coeffs=((True, True),))


def _xv(act, act2, slope_i, y2='same', scale=True, shift=True):
    return dict(act=act, act2=act2, slope_i=slope_i, y2=y2, scale=scale, shift=shift)


# gcc_conv_eval_ex: (act, act2) in (LRELU, RELU), (RELU, none), (NONE, TANH), (TANH, none), (NONE, LRELU); y2 once in y's buffer
# at a window of its own ('same') and once in a buffer with another ldy2 ('own').  (LRELU, RELU) runs with both slopes: with a
# positive slope relu(lrelu(z)) = relu(z), so only the negative one tells act2(act(z)) from act2(z).  A NULL scale and a NULL
# shift ride on the two single-output variants.
EX_ALL = (_xv(EV_LRELU, EV_RELU, 0, 'same'), _xv(EV_LRELU, EV_RELU, 1, 'own'), _xv(EV_RELU, None, 0, scale=False),
          _xv(EV_NONE, EV_TANH, 0, 'own'), _xv(EV_TANH, None, 0, shift=False), _xv(EV_NONE, EV_LRELU, 1, 'same'))


def variant_slope(v, kind):
    """the slope of a variant on 'int' / 'normal' data, as the fp32 number the kernel reads"""
    return f32((INT_SLOPES if kind == 'int' else NORMAL_SLOPES)[v['slope_i']])


def variant_reference(case, d, v, kind, conv):
    """float64 reference of one variant of a case: dict(y, y2, z, mag, res, slope); res: the residual tensor or None"""
    slope = variant_slope(v, kind)
    if case['entry'] == 'eval':
        y, z, mag = ref_eval(d, case['g'], v['act'], v['residual'], slope, v['scale'], v['shift'], conv)
        return dict(y=y, y2=None, z=z, mag=mag, res=d['residual'] if v['residual'] else None, slope=slope)
    y, y2, z, mag = ref_eval_ex(d, case['g'], v['act'], v['act2'], slope, v['scale'], v['shift'], conv)
    return dict(y=y, y2=y2, z=z, mag=mag, res=None, slope=slope)


def variant_emul(case, d, v, kind, S=1, defect=None, parts=None):
    """eval_emul of one variant of a case"""
    return eval_emul(d, case['g'], case['entry'], v['act'], v.get('act2'), v.get('residual', False), variant_slope(v, kind), v['scale'],
                     v['shift'], S=S, defect=defect, parts=parts)


def variant_id(v):
    names = {EV_NONE: 'none', EV_PRELU: 'prelu', EV_TANH: 'tanh', EV_RELU: 'relu', EV_LRELU: 'lrelu'}
    tag = names[v['act']] + ('' if v.get('act2') is None else '+' + names[v['act2']] + ':' + v['y2'])
    return '%s slope#%d%s scale %d shift %d' % (tag, v['slope_i'], ' +res' if v.get('residual') else '', v['scale'], v['shift'])


def _e(name, entry, g, variants, opts=None, ws=True, **expect):
    """one eval launch under test.  entry: 'eval' (gcc_conv_fprop_eval) or 'ex' (gcc_conv_eval_ex); g: the 10-tuple above;
    variants: the epilogues it runs; opts: option name -> value; ws: hand the call its split-K workspace; expect: route (0 igemm
    un-split, 4 ring-walk, 5 split K + fold), tile, S (K slices) -- asserted BEFORE a number is compared."""
    return dict(name=name, entry=entry, g=g, variants=variants, opts=opts or {}, ws=ws, expect=expect)


def _sq(N, H, W, Ci, Co, k, s, p, tr=False):
    return (N, H, W, Ci, Co, k, k, s, p, tr)


THIN_ON, THIN_OFF = dict(IGEMM_THIN=1), dict(IGEMM_THIN=0)
EVAL_CASES = (
    # ---- gcc_conv_fprop_eval: un-split igemm_kernel, each column tile; 391 pixels = three full 128-pixel tiles and a partial one
    _e('ev-t16-co13', 'eval', _sq(1, 17, 23, 24, 13, 3, 1, 1), EV_ALL, route=0, tile=128016, S=1),
    _e('ev-t32-co24', 'eval', _sq(1, 17, 23, 24, 24, 3, 1, 1), EV_ALL, route=0, tile=128032, S=1),
    _e('ev-t64-co64', 'eval', _sq(1, 17, 23, 24, 64, 3, 1, 1), EV_ALL, route=0, tile=128064, S=1),
    _e('ev-t128-co136', 'eval', _sq(1, 17, 23, 24, 136, 3, 1, 1), EV_ALL, route=0, tile=128128, S=1),     # two column tiles, the second partial
    # ---- split K + splitk_epilogue_kernel<true>; 5 and 6 slices: both loops of the fold's four-at-a-time sum run
    _e('ev-split4-co13', 'eval', _sq(1, 6, 7, 128, 13, 3, 1, 1), EV_ALL, route=5, tile=128016, S=4),
    _e('ev-split4-co64', 'eval', _sq(1, 6, 7, 128, 64, 3, 1, 1), EV_ALL, route=5, tile=128064, S=4),
    _e('ev-split5-co13', 'eval', _sq(1, 6, 7, 144, 13, 3, 1, 1), EV_ALL, route=5, tile=128016, S=5),
    _e('ev-split6-co64', 'eval', _sq(1, 6, 7, 192, 64, 3, 1, 1), EV_ALL, route=5, tile=128064, S=6),
    _e('ev-split5-nows', 'eval', _sq(1, 6, 7, 144, 13, 3, 1, 1), EV_ALL, ws=False, route=0, tile=128016, S=1),
    # ---- the ring-walk's EV branch (R3_MIN_PIXELS = 8192: these are its smallest) and the same calls with the option off
    _e('ev-ring-64-64', 'eval', _sq(1, 128, 65, 64, 64, 3, 1, 1), EV_ALL, opts=THIN_ON, route=4),
    _e('ev-ring-16-24', 'eval', _sq(1, 128, 65, 16, 24, 3, 1, 1), EV_ALL, opts=THIN_ON, route=4),
    _e('ev-ring-16-20', 'eval', _sq(1, 128, 65, 16, 20, 3, 1, 1), EV_ALL, opts=THIN_ON, route=4),           # Co not a multiple of 8
    _e('ev-ring-64-64-thin0', 'eval', _sq(1, 128, 65, 64, 64, 3, 1, 1), EV_ALL, opts=THIN_OFF, route=0, tile=128064, S=1),
    _e('ev-ring-16-24-thin0', 'eval', _sq(1, 128, 65, 16, 24, 3, 1, 1), EV_ALL, opts=THIN_OFF, route=0, tile=128032, S=1),
    _e('ev-ring-16-20-thin0', 'eval', _sq(1, 128, 65, 16, 20, 3, 1, 1), EV_ALL, opts=THIN_OFF, route=0, tile=128032, S=1),
    # ---- SRResNet's 9 x 9 first and last layers
    _e('ev-sr-first', 'eval', _sq(1, 12, 12, 3, 64, 9, 1, 4), EV_SR_FIRST, route=0, tile=128064, S=1),
    _e('ev-sr-last', 'eval', _sq(1, 12, 12, 64, 3, 9, 1, 4), EV_SR_LAST, route=5, tile=128016, S=17),    # K = 5184: split, 17 = 4 x 4 + 1 slices
    # ---- DRN geometries: 1 x 1, 3 x 3 stride 2, 1 x 1 stride 2
    _e('ev-drn-1x1', 'eval', _sq(2, 9, 9, 72, 40, 1, 1, 0), EV_DRN, route=0, tile=128064, S=1),
    _e('ev-drn-k3s2', 'eval', _sq(1, 15, 17, 32, 64, 3, 2, 1), EV_DRN, route=0, tile=128064, S=1),
    _e('ev-drn-1x1s2', 'eval', _sq(1, 16, 16, 64, 64, 1, 2, 0), EV_DRN, route=0, tile=128064, S=1),
    # ---- gcc_conv_eval_ex, forward
    _e('ex-down-thin', 'ex', _sq(1, 16, 16, 3, 64, 4, 2, 1), EX_ALL, route=0, tile=128064, S=1),
    _e('ex-down-co512', 'ex', _sq(3, 8, 8, 13, 512, 4, 2, 1), EX_ALL, route=0, tile=128128, S=1),
    _e('ex-down-split', 'ex', _sq(1, 2, 2, 512, 512, 4, 2, 1), EX_ALL, route=5, tile=128128, S=32),
    _e('ex-stem-k3s2p0', 'ex', _sq(1, 19, 19, 32, 32, 3, 2, 0), EX_ALL, route=0, tile=128032, S=1),
    _e('ex-k5', 'ex', _sq(1, 9, 9, 48, 64, 5, 1, 2), EX_ALL, route=5, tile=128064, S=4),
    _e('ex-1x1', 'ex', _sq(2, 9, 9, 72, 40, 1, 1, 0), EX_ALL, route=0, tile=128064, S=1),
    _e('ex-rect-1x7', 'ex', (1, 17, 23, 128, 192, 1, 7, 1, 0, False), EX_ALL, route=0, tile=128128, S=1),
    _e('ex-rect-7x1', 'ex', (1, 23, 17, 128, 192, 7, 1, 1, 0, False), EX_ALL, route=0, tile=128128, S=1),
    _e('ex-drn-stem7', 'ex', _sq(1, 14, 14, 3, 16, 7, 1, 3), EX_ALL, route=0, tile=128016, S=1),
    _e('ex-drn-k3', 'ex', _sq(1, 15, 17, 32, 64, 3, 1, 1), EX_ALL, route=0, tile=128064, S=1),
    # ---- gcc_conv_eval_ex, transposed
    _e('exT-bottleneck', 'ex', _sq(1, 1, 1, 512, 512, 4, 2, 1, True), EX_ALL, route=5, tile=128128, S=8),
    _e('exT-thin-co13', 'ex', _sq(3, 4, 4, 512, 13, 4, 2, 1, True), EX_ALL, route=5, tile=128016, S=8),
    _e('exT-image', 'ex', _sq(1, 16, 16, 64, 3, 4, 2, 1, True), EX_ALL, route=0, tile=128016, S=1),
    _e('exT-ci13', 'ex', _sq(3, 8, 8, 13, 64, 4, 2, 1, True), EX_ALL, route=0, tile=128064, S=1),
    _e('exT-sagan-first', 'ex', _sq(2, 1, 1, 128, 512, 4, 1, 0, True), EX_ALL, route=5, tile=128128, S=8),
)
EVAL_BY_NAME = {c['name']: c for c in EVAL_CASES}
assert len(EVAL_BY_NAME) == len(EVAL_CASES), 'case names must be unique'


def eval_seed(case):
    return sum(ord(ch) for ch in case['name']) + sum(int(v) for v in case['g'])


def eval_desc(lib_mod, g, ld_in=None, ld_out=None):
    """the gcc_conv_t of an eval call (default plan).  A transposed call is described as the LAYER whose data gradient it is: the
    descriptor's x side is the call's output, its y side the call's input."""
    N, H, W, Ci, Co, kh, kw, s, p, tr = g
    plan = (0,) * len(lib_mod.PLAN_FIELDS)
    ld_in, ld_out = ld_in or ceil8(Ci), ld_out or ceil8(Co)
    if not tr:
        return lib_mod.conv_t(N, H, W, Ci, Co, kh, kw, s, p, ld_in, 0, ld_out, 0, plan)
    Ho, Wo = eval_out_hw(g)
    return lib_mod.conv_t(N, Ho, Wo, Co, Ci, kh, kw, s, p, ld_out, 0, ld_in, 0, plan)


def eval_routing(lib_mod, case, d=None, ws=None):
    """what the library says an eval call of this case runs on: dict(route, need, ws, tile, S, launches, rows, phases).
    need: gcc_conv_eval_workspace / gcc_conv_eval_ex_workspace; ws: the bytes the call is handed (need, or 0: ws False);
    tile: gcc_conv_tile under the one-family plan the eval entries use; S: the K slices, read back from the workspace size
    (bytes = phases x slices x rows x padded columns x 4); launches: the partial tiles and the fold of a split call, else one."""
    lib = lib_mod.load()
    g = case['g']
    N, H, W, Ci, Co, kh, kw, s, p, tr = g
    tr = int(tr)
    d = d if d is not None else eval_desc(lib_mod, g)
    use = case['ws'] if ws is None else ws
    if case['entry'] == 'eval':
        need = int(lib.gcc_conv_eval_workspace(C.byref(d)))
        have = need if use else 0
        route = int(lib.gcc_conv_eval_route(C.byref(d), have))
    else:
        need = int(lib.gcc_conv_eval_ex_workspace(C.byref(d), tr))
        have = need if use else 0
        route = int(lib.gcc_conv_eval_ex_route(C.byref(d), tr, have))
    one = type(d).from_buffer_copy(d)
    one.plan.tile_families = 1
    tile = int(lib.gcc_conv_tile(C.byref(one), tr))
    Ho, Wo = eval_out_hw(g)
    phases = s * s if tr else 1
    rows = N * cdiv(Ho, s) * cdiv(Wo, s) if tr else N * Ho * Wo
    bc = tile % 1000
    S = have // (phases * rows * cdiv(Co, bc) * bc * 4) if route == 5 else 1
    return dict(route=route, need=need, ws=have, tile=tile, S=int(S), launches=2 if route == 5 else 1, rows=rows, phases=phases)


def check_eval_expect(case, r, launches=None):
    """the case's intended route against what the library reports (a mismatch is a failure, never a skip); launches: the
    gcc_launch_count of the call, when it ran"""
    e, name = case['expect'], case['name']
    assert r['route'] == e['route'], '%s: route %d, intended %s' % (name, r['route'], e['route'])
    assert (r['route'] == 5) == (r['ws'] > 0 and r['S'] > 1), '%s: route %d with a workspace of %d bytes, %d slices' % (name, r['route'], r['ws'], r['S'])
    if 'tile' in e:
        assert r['tile'] == e['tile'], '%s: tile %d, intended %d' % (name, r['tile'], e['tile'])
    if 'S' in e:
        assert r['S'] == e['S'], '%s: %d K slices, intended %d' % (name, r['S'], e['S'])
    if launches is not None:
        assert launches == r['launches'], '%s: %d launches, intended %d' % (name, launches, r['launches'])
