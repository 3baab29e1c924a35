"""The streaming kernels of srgan.hip, each against a plain PyTorch-CPU reference of the same operation from the same bf16-rounded,
seeded inputs, at the sizes where their loops change shape: gcc_prelu (plain and fused with PixelShuffle(2), forward and backward,
the ordered and the atomic slope-gradient sum), gcc_maxpool2x2 (forward, backward, backward through a ReLU), gcc_pool_linear_fwd and
gcc_pool_linear_bwd.  tests/test_srgan_gpu.py keeps its one-shape tests of the same entry points.

What is exact and what is bounded:
  y / dx of gcc_prelu, everything of gcc_maxpool2x2, dx of gcc_pool_linear_bwd: a select or one or two fp32 multiplies, rounded to
      bf16 to nearest even -- compared bit for bit with the fp32 restatement in torch.
  sums (dslope, pooled, logit, dw, db): against float64, |err| <= depth * 2^-24 * sum|terms|, where depth is the longest chain of
      fp32 roundings one term passes through in the kernel, counted from the code beside each bound below.  (Standard bound of a
      summation tree: every rounding on a term's way to the result multiplies its error factor by (1 + 2^-24) once.)"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import BAD_ARG, DEV, _ops, rb

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2                  # include/gcc_hip.h GCC_ERR_UNSUPPORTED
U = 2.0 ** -24                    # unit roundoff of fp32
SLOPE = 0.3
DS_START = 1.5                    # dslope accumulates: every call starts from this value
PRELU_BWD_BLOCKS, GRID_CAP = 1024, 4096


def ceil8(v):
    return (v + 7) & ~7


def nhwc_dev(a, ld=None, pad=0.0):
    """CPU fp32 [N, H, W, C] (bf16-representable) -> (NHWC activation view [N, C, H, W] on the device, its base [N, H, W, ld]); the
    lanes [C, ld) of every pixel hold `pad`"""
    N, H, W, Cc = a.shape
    ld = ld or ceil8(Cc)
    base = torch.full((N, H, W, ld), pad, dtype=torch.bfloat16, device=DEV)
    base[..., :Cc] = a.bfloat16().to(DEV)
    return base.permute(0, 3, 1, 2)[:, :Cc], base


def out_dev(N, Cc, H, W, ld=None, fill=1.0):
    """an output activation whose every lane holds `fill`: zeros found in its padding lanes afterwards are the kernel's own"""
    ld = ld or ceil8(Cc)
    base = torch.full((N, H, W, ld), fill, dtype=torch.bfloat16, device=DEV)
    return base.permute(0, 3, 1, 2)[:, :Cc], base


def bits(t):
    return t.view(torch.int16)


def same_bits(got, ref, what):
    """got, ref: bf16 CPU tensors of one shape"""
    assert got.dtype == torch.bfloat16 and ref.dtype == torch.bfloat16 and got.shape == ref.shape
    ne = bits(got) != bits(ref)
    assert not bool(ne.any()), '%s: %d of %d values differ in their bits (first at flat index %d: %r vs %r)' % (
        what, int(ne.sum()), ne.numel(), int(ne.reshape(-1).nonzero()[0]), got[ne][0].item(), ref[ne][0].item())


def pad_lanes_zero(base, Cc, what):
    c8 = ceil8(Cc)
    if c8 > Cc:
        assert float(base[..., Cc:c8].float().abs().max()) == 0.0, what + ': padding lanes [C, ceil8(C)) are not zero'


# ---- gcc_prelu ------------------------------------------------------------------------------------------------------------
def _items(N, Cc, H, W):
    return N * H * W * ((Cc + 7) // 8)


def _grid(items, cap):
    return max(1, min((items + 255) // 256, cap))


def _dslope_depth(items, grid, per_item, ordered):
    """the longest chain of fp32 additions one g * x term passes through on its way into dslope (srgan.hip prelu_kernel); the
    products themselves are exact (two bf16 factors: 16 significant bits):
      per thread   `ds += g * x`, per_item of them (8 lanes; 32 with the shuffle) for each of its ceil(items / (grid * 256)) items
      wave_sum     6 butterfly steps
      block sum    sh[0] + sh[1] + sh[2] + sh[3]: 3
      ordered      the last workgroup: ceil(grid / 256) serial adds per thread over the partials, 6 + 3 for its block sum, and the
                   one `dslope[0] += total`
      atomic       one atomicAdd per workgroup on dslope: up to `grid` of them after a term's own"""
    trips = -(-items // (grid * 256))
    own = per_item * trips + 6 + 3
    return own + ((-(-grid // 256) + 6 + 3 + 1) if ordered else grid)


def _plant_zeros(x):
    flat = x.view(-1)
    flat[::97] = 0.0
    flat[5::101] = -0.0
    return x


def _slope_terms(g, x):
    t = (g.double() * x.double())[x <= 0]
    return t.sum().item(), t.abs().sum().item()


@functools.lru_cache(maxsize=4)
def _plain_data(N, Cc, H, W):
    """x, dy [N, H, W, C] fp32 (bf16-rounded; half of x non-positive, exact 0.0 and -0.0 planted), y and dx as bf16, the float64
    slope gradient and sum |g x| over x <= 0"""
    g = torch.Generator().manual_seed(N * 1000003 + Cc * 1009 + H * 31 + W)
    x = _plant_zeros(rb(torch.randn(N, H, W, Cc, generator=g)))
    dy = rb(torch.randn(N, H, W, Cc, generator=g))
    s = torch.tensor(SLOPE)
    y = torch.where(x > 0, x, s * x).bfloat16()
    dx = torch.where(x > 0, dy, s * dy).bfloat16()
    frac = (x <= 0).float().mean().item()
    assert 0.45 < frac < 0.56 and bool((x.view(-1)[5::101].view(torch.int32) == -2 ** 31).all())
    return (x, dy, y, dx) + _slope_terms(dy, x)


def _check_dslope(got, ref, mag, depth, what):
    """the issue's bound: depth * 2^-24 * sum |g x| (the start value is one more term: DS_START is far below sum |g x| / depth)"""
    err, lim = abs(got - (DS_START + ref)), depth * U * mag
    print('%s: dslope err %.3g, bound %.3g (depth %d, sum|g x| %.4g)' % (what, err, lim, depth, mag))
    assert err <= lim, '%s: dslope %.9g vs %.9g: err %.3g > %.3g' % (what, got, DS_START + ref, err, lim)


# (N, C, H, W, workgroups of the backward launch): items = N H W ceil(C / 8); the backward grid is min(ceil(items / 256), 1024) with
# two items per thread and trip above it, the forward grid min(ceil(items / 256), 4096)
PLAIN_CASES = [
    (1, 8, 70, 110, 31),          # 7700 items: ntop 31, nsub 1
    (1, 16, 50, 80, 32),          # 8000: ntop 32, nsub 1
    (1, 8, 83, 100, 33),          # 8300: nsub 2 for sub-counter 0, 1 for the others
    (1, 24, 53, 100, 63),         # 15900: nsub 2 but for the last sub-counter
    (2, 8, 90, 90, 64),           # 16200: nsub 2 everywhere
    (1, 40, 200, 256, 1000),      # 256000: below the cap, one item per thread
    (1, 72, 171, 171, 1024),      # 263169: 1025 items past 1024 x 256 -- a handful of threads have a second item
    (2, 20, 300, 333, 1024),      # 599400: between one and two full double trips; C % 8 != 0
    (1, 52, 340, 341, 1024),      # 811580: a third trip; C % 8 != 0
    (1, 8, 1024, 1025, 1024),     # 1049600: past 4096 x 256 -- the forward's grid-stride trip
]


def _plain_id(c):
    return '%dx%dx%dx%d-items%d-grid%d' % (c[0], c[1], c[2], c[3], _items(*c[:4]), c[4])


def _plain_backward(ops, N, Cc, H, W, xd, dyd, sd):
    dxd, dxb = out_dev(N, Cc, H, W)
    ds = torch.full((1,), DS_START, device=DEV)
    ops.prelu_bwd(xd, sd, dyd, dxd, dslope=ds)
    return dxb, ds


@pytest.mark.parametrize('case', PLAIN_CASES, ids=_plain_id)
def test_prelu_plain(case):
    ops = _ops()
    N, Cc, H, W, grid = case
    items = _items(N, Cc, H, W)
    assert _grid(items, PRELU_BWD_BLOCKS) == grid
    x, dy, y_ref, dx_ref, ds_ref, ds_mag = _plain_data(N, Cc, H, W)
    # the padding lanes of the operands hold values the `live` mask has to keep out: x <= 0 there would add g * x to dslope
    xd, _ = nhwc_dev(x, pad=-3.0)
    dyd, _ = nhwc_dev(dy, pad=5.0)
    sd = torch.tensor([SLOPE], device=DEV)
    yd, yb = out_dev(N, Cc, H, W)
    ops.prelu_fwd(xd, sd, yd)
    yb = yb.cpu()
    same_bits(yb[..., :Cc], y_ref, 'prelu y')
    pad_lanes_zero(yb, Cc, 'prelu y')
    dxb, ds = _plain_backward(ops, N, Cc, H, W, xd, dyd, sd)
    dxb = dxb.cpu()
    same_bits(dxb[..., :Cc], dx_ref, 'prelu dx')
    pad_lanes_zero(dxb, Cc, 'prelu dx')
    _check_dslope(ds.item(), ds_ref, ds_mag, _dslope_depth(items, grid, 8, True), 'prelu ' + _plain_id(case))
    _, ds2 = _plain_backward(ops, N, Cc, H, W, xd, dyd, sd)
    assert ds2.view(torch.int32).item() == ds.view(torch.int32).item(), 'two identical calls: dslope %r then %r' % (ds.item(), ds2.item())


def test_prelu_plain_channel_slice():
    """x, dy, dx (and y) as ops.cslice views [8, 28) of 40-wide buffers, 300000 items (the capped, two-items-per-trip backward):
    channels 0..7 and 32..39 of the outputs keep their bits, the slice's own padding lanes 28..31 are written as zeros"""
    ops = _ops()
    N, Cc, H, W, off, wide = 1, 20, 250, 400, 8, 40
    items = _items(N, Cc, H, W)
    assert items == 300000 and _grid(items, PRELU_BWD_BLOCKS) == 1024
    x, dy, y_ref, dx_ref, ds_ref, ds_mag = _plain_data(N, Cc, H, W)
    g = torch.Generator().manual_seed(41)
    sd = torch.tensor([SLOPE], device=DEV)

    def wide_of(t):
        full = rb(torch.randn(N, H, W, wide, generator=g) - 0.5)          # neighbours and padding lanes: non-zero, mostly negative
        full[..., off:off + Cc] = t
        return nhwc_dev(full)

    xw, _ = wide_of(x)
    dyw, _ = wide_of(dy)
    keep = rb(torch.randn(N, H, W, wide, generator=g)).bfloat16()
    for which in ('forward', 'backward'):
        ow, ob = nhwc_dev(keep.float())
        ds = torch.full((1,), DS_START, device=DEV)
        if which == 'forward':
            ops.prelu_fwd(ops.cslice(xw, off, Cc), sd, ops.cslice(ow, off, Cc))
        else:
            ops.prelu_bwd(ops.cslice(xw, off, Cc), sd, ops.cslice(dyw, off, Cc), ops.cslice(ow, off, Cc), dslope=ds)
        ob = ob.cpu()
        same_bits(ob[..., off:off + Cc], y_ref if which == 'forward' else dx_ref, 'sliced prelu ' + which)
        assert float(ob[..., off + Cc:off + ceil8(Cc)].float().abs().max()) == 0.0, which + ': padding lanes of the slice'
        same_bits(ob[..., :off], keep[..., :off], which + ': channels below the slice')
        same_bits(ob[..., off + ceil8(Cc):], keep[..., off + ceil8(Cc):], which + ': channels above the slice')
        if which == 'backward':
            _check_dslope(ds.item(), ds_ref, ds_mag, _dslope_depth(items, 1024, 8, True), 'sliced prelu')


def test_prelu_counters_return_to_zero_between_grids():
    """33, 1024, 31 and 1024 workgroups in a row on the one zero-filled workspace of the stream, never zeroed again: every slope
    gradient meets its bound and the 33 counter words (the whole 256-byte head) read back as zero"""
    ops = _ops()
    sd = torch.tensor([SLOPE], device=DEV)
    for case in (PLAIN_CASES[2], PLAIN_CASES[6], PLAIN_CASES[0], PLAIN_CASES[6]):
        N, Cc, H, W, grid = case
        x, dy, _, dx_ref, ds_ref, ds_mag = _plain_data(N, Cc, H, W)
        xd, _ = nhwc_dev(x)
        dyd, _ = nhwc_dev(dy)
        dxb, ds = _plain_backward(ops, N, Cc, H, W, xd, dyd, sd)
        _check_dslope(ds.item(), ds_ref, ds_mag, _dslope_depth(_items(N, Cc, H, W), grid, 8, True), 'in a row, grid %d' % grid)
        same_bits(dxb.cpu()[..., :Cc], dx_ref, 'prelu dx, grid %d' % grid)
    ws = ops.zeroed_workspace(torch.device(DEV), 'prelu', 256 + 4 * 4096)
    assert int(ws[:256].cpu().to(torch.int32).abs().sum()) == 0, 'arrival counters after the last call'


@pytest.mark.parametrize('case', [PLAIN_CASES[2], PLAIN_CASES[6]], ids=_plain_id)
def test_prelu_atomic_slope_gradient_without_workspace(case):
    """workspace NULL through the C entry: one atomic add per workgroup on dslope; same bound with the atomic chain's depth"""
    ops = _ops()
    N, Cc, H, W, grid = case
    x, dy, _, dx_ref, ds_ref, ds_mag = _plain_data(N, Cc, H, W)
    xd, _ = nhwc_dev(x)
    dyd, _ = nhwc_dev(dy)
    dxd, dxb = out_dev(N, Cc, H, W)
    sd = torch.tensor([SLOPE], device=DEV)
    ds = torch.full((1,), DS_START, device=DEV)
    xp, _, _, _, _, ldx = ops.geom(xd)
    rc = ops.lib().gcc_prelu(1, xp, ldx, sd.data_ptr(), Cc, N, H, W, 1, None, 0, ops.geom(dyd)[0], ops.geom(dyd)[5], ops.geom(dxd)[0],
                             ops.geom(dxd)[5], ds.data_ptr(), None, 0, ops.stream())
    assert rc == 0
    _check_dslope(ds.item(), ds_ref, ds_mag, _dslope_depth(_items(N, Cc, H, W), grid, 8, False), 'atomic, grid %d' % grid)
    same_bits(dxb.cpu()[..., :Cc], dx_ref, 'prelu dx (no workspace)')


def test_prelu_refusals_launch_nothing():
    ops = _ops()
    lib = ops.lib()
    N, Cc, H, W = 1, 8, 2, 2
    xd, _ = out_dev(N, 32, H, W)
    yd, yb = out_dev(N, 32, 2 * H, 2 * W)
    sd = torch.tensor([SLOPE], device=DEV)
    ds = torch.full((1,), DS_START, device=DEV)
    ws = ops.zeroed_workspace(torch.device(DEV), 'prelu', 256 + 4 * 4096)
    xp, yp, sp, st = xd.data_ptr(), yd.data_ptr(), sd.data_ptr(), ops.stream()
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)

    def call(backward, ldx, Cx, shuffle, y, ldy, dy, lddy, dx, lddx):
        return lib.gcc_prelu(backward, xp, ldx, sp, Cx, N, H, W, shuffle, y, ldy, dy, lddy, dx, lddx, ds.data_ptr(), ws.data_ptr(),
                             ws.numel(), st)
    assert call(0, 32, Cc, 3, yp, 32, None, 0, None, 0) == BAD_ARG                  # shuffle 3
    assert call(1, 32, Cc, 3, None, 0, yp, 32, yp, 32) == BAD_ARG
    assert call(0, 12, Cc, 1, yp, 32, None, 0, None, 0) == BAD_ARG                  # ld not a multiple of 8: x, y, dy, dx
    assert call(0, 32, Cc, 1, yp, 12, None, 0, None, 0) == BAD_ARG
    assert call(1, 32, Cc, 1, None, 0, yp, 12, yp, 32) == BAD_ARG
    assert call(1, 32, Cc, 1, None, 0, yp, 32, yp, 12) == BAD_ARG
    assert call(0, 32, 4, 2, yp, 32, None, 0, None, 0) == UNSUPPORTED               # the shuffle reads whole 32-channel groups
    assert call(1, 32, 4, 2, None, 0, yp, 32, yp, 32) == UNSUPPORTED
    assert call(1, 32, Cc, 1, None, 0, None, 0, yp, 32) == BAD_ARG                  # backward without dy
    assert call(1, 32, Cc, 1, None, 0, yp, 32, None, 0) == BAD_ARG                  # ... without dx
    assert call(0, 32, Cc, 1, None, 0, None, 0, None, 0) == BAD_ARG                 # forward without y
    assert int(lib.gcc_launch_count(1)) == 0
    torch.cuda.synchronize()
    assert ds.item() == DS_START and float((yb.float() - 1.0).abs().max()) == 0.0


# (N, C, H, W) of the OUTPUT channels and the INPUT map: x [N, 4C, H, W] -> y [N, C, 2H, 2W]; items = N H W C / 8, grid capped at 4096
SHUFFLE_CASES = [
    (1, 8, 5, 7),                 # 35 items: one workgroup
    (2, 64, 1, 1),                # 16
    (2, 64, 39, 41),              # 25584: 100 workgroups -- 32 sub-counters of 3 or 4 arrivals
    (1, 8, 1024, 1025),           # 1049600: 4096 workgroups (nsub 128) and a grid-stride trip for 1024 items
]


def _shuffle_id(c):
    return '%dx%dx%dx%d-items%d-grid%d' % (c + (_items(*c), _grid(_items(*c), GRID_CAP)))


@pytest.mark.parametrize('case', SHUFFLE_CASES, ids=_shuffle_id)
def test_prelu_pixel_shuffle(case):
    ops = _ops()
    N, Cc, H, W = case
    items = _items(N, Cc, H, W)
    grid = _grid(items, GRID_CAP)
    g = torch.Generator().manual_seed(Cc * 7 + H)
    x = _plant_zeros(rb(torch.randn(N, H, W, 4 * Cc, generator=g)))
    dy = rb(torch.randn(N, 2 * H, 2 * W, Cc, generator=g))
    s = torch.tensor(SLOPE)
    xs = F.pixel_shuffle(x.permute(0, 3, 1, 2), 2)                       # NCHW [N, C, 2H, 2W]
    dyc = dy.permute(0, 3, 1, 2)
    y_ref = torch.where(xs > 0, xs, s * xs).bfloat16()
    dx_ref = F.pixel_unshuffle(torch.where(xs > 0, dyc, s * dyc), 2).bfloat16()
    ds_ref, ds_mag = _slope_terms(dyc, xs)
    xd, _ = nhwc_dev(x)
    dyd, _ = nhwc_dev(dy)
    sd = torch.tensor([SLOPE], device=DEV)
    yd, yb = out_dev(N, Cc, 2 * H, 2 * W)
    ops.prelu_fwd(xd, sd, yd, shuffle=2)
    same_bits(yb.cpu().permute(0, 3, 1, 2), y_ref, 'shuffled prelu y')
    res = []
    for _ in range(2):
        dxd, dxb = out_dev(N, 4 * Cc, H, W)
        ds = torch.full((1,), DS_START, device=DEV)
        ops.prelu_bwd(xd, sd, dyd, dxd, dslope=ds, shuffle=2)
        res.append((dxb, ds))
    same_bits(res[0][0].cpu().permute(0, 3, 1, 2), dx_ref, 'shuffled prelu dx')
    _check_dslope(res[0][1].item(), ds_ref, ds_mag, _dslope_depth(items, grid, 32, True), 'shuffled prelu ' + _shuffle_id(case))
    assert res[0][1].view(torch.int32).item() == res[1][1].view(torch.int32).item(), 'two identical calls'
    ws = ops.zeroed_workspace(torch.device(DEV), 'prelu', 256 + 4 * 4096)
    assert int(ws[:256].cpu().to(torch.int32).abs().sum()) == 0, 'arrival counters'
    if grid in (1, 100):                                                 # the atomic route at a small and a middling grid
        dxd, dxb = out_dev(N, 4 * Cc, H, W)
        ds = torch.full((1,), DS_START, device=DEV)
        rc = ops.lib().gcc_prelu(1, ops.geom(xd)[0], ops.geom(xd)[5], sd.data_ptr(), Cc, N, H, W, 2, None, 0, ops.geom(dyd)[0],
                                 ops.geom(dyd)[5], ops.geom(dxd)[0], ops.geom(dxd)[5], ds.data_ptr(), None, 0, ops.stream())
        assert rc == 0
        _check_dslope(ds.item(), ds_ref, ds_mag, _dslope_depth(items, grid, 32, False), 'shuffled prelu, atomic')
        same_bits(dxb.cpu().permute(0, 3, 1, 2), dx_ref, 'shuffled prelu dx (no workspace)')


# ---- gcc_maxpool2x2 -------------------------------------------------------------------------------------------------------
LEVELS = torch.tensor([-1.0, 0.0, 0.5, 1.0])
POOL_CASES = [(2, Cc, Ho, Wo) for Cc in (8, 20, 24, 72) for Ho, Wo in ((1, 1), (1, 5), (3, 4), (7, 1))] + [
    (1, 8, 1024, 1025)]           # 1049600 items: past 4096 x 256


def _pool_input(family, N, Cc, Ho, Wo, g):
    shape = (N, 2 * Ho, 2 * Wo, Cc)
    if family == 'random':
        return rb(torch.randn(shape, generator=g))
    return LEVELS[torch.randint(0, 4, shape, generator=g)]


def _windows(x):
    """[N, 2Ho, 2Wo, C] -> [N, Ho, Wo, C, 4]: the four values of every window in scan order"""
    N, H, W, Cc = x.shape
    return x.view(N, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, Cc, 4)


def _tie_share(x):
    w = _windows(x)
    return ((w == w.amax(-1, keepdim=True)).sum(-1) >= 2).float().mean().item()


def _pool_reference(x, dy, through_relu):
    """fp32 autograd on the CPU, NCHW contiguous: (y, dx); through_relu: max_pool2d(relu(x)) differentiated with respect to x"""
    xc = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.max_pool2d(F.relu(xc) if through_relu else xc, 2, 2)
    (y * dy.permute(0, 3, 1, 2)).sum().backward()
    return y.detach(), xc.grad


def _pool_check(ops, x, dy, N, Cc, Ho, Wo, family):
    xd, _ = nhwc_dev(x)
    dyd, _ = nhwc_dev(dy)
    y_ref, dx_ref = _pool_reference(x, dy, False)
    yd, yb = out_dev(N, Cc, Ho, Wo)
    ops.maxpool_fwd(xd, yd)
    yb = yb.cpu()
    assert torch.equal(yb[..., :Cc].float().permute(0, 3, 1, 2), y_ref), 'maxpool y'
    pad_lanes_zero(yb, Cc, 'maxpool y')
    dxd, dxb = out_dev(N, Cc, 2 * Ho, 2 * Wo)
    ops.maxpool_bwd(xd, dyd, dxd)
    dxb = dxb.cpu()
    assert torch.equal(dxb[..., :Cc].float().permute(0, 3, 1, 2), dx_ref), 'maxpool dx (%s)' % family
    pad_lanes_zero(dxb, Cc, 'maxpool dx')


@pytest.mark.parametrize('family', ['random', 'levels'])
@pytest.mark.parametrize('case', POOL_CASES, ids=lambda c: '%dx%dx%dx%d-items%d' % (c + (_items(*c),)))
def test_maxpool2x2(case, family):
    """random bf16 values, and values from four levels (about 44 % of the windows tie for their maximum: the backward has to
    pick the first in scan order, as ATen does); then the backward through a ReLU: x = relu(z), gradient with respect to z"""
    ops = _ops()
    N, Cc, Ho, Wo = case
    g = torch.Generator().manual_seed(Cc * 100 + Ho * 10 + Wo + (7 if family == 'levels' else 0))
    x = _pool_input(family, N, Cc, Ho, Wo, g)
    dy = rb(torch.randn(N, Ho, Wo, Cc, generator=g))
    if family == 'levels':
        assert _tie_share(x) >= 0.25, 'the input does not tie often enough: %.3f' % _tie_share(x)
    _pool_check(ops, x, dy, N, Cc, Ho, Wo, family)
    z = _pool_input(family, N, Cc, Ho, Wo, g)
    z[0, :2, :2, 0] = torch.tensor([[0.0, -1.0], [-1.0, 0.0]])            # one window whose maximum after the ReLU is exactly 0
    a = F.relu(z)
    if family == 'levels':
        assert _tie_share(a) >= 0.25 and bool((_windows(a).amax(-1) == 0).any())
    _, dz_ref = _pool_reference(z, dy, True)
    ad, _ = nhwc_dev(a)
    dyd, _ = nhwc_dev(dy)
    dzd, dzb = out_dev(N, Cc, 2 * Ho, 2 * Wo)
    ops.maxpool_bwd(ad, dyd, dzd, relu_mask=True)
    dzb = dzb.cpu()
    assert torch.equal(dzb[..., :Cc].float().permute(0, 3, 1, 2), dz_ref), 'maxpool dz through the ReLU (%s)' % family
    pad_lanes_zero(dzb, Cc, 'maxpool dz')


def test_maxpool2x2_channel_slice():
    """x, y, dy, dx as ops.cslice views [8, 32) of 40-wide buffers: the neighbouring channels of y and dx keep their bits"""
    ops = _ops()
    N, Cc, Ho, Wo, off, wide = 2, 24, 9, 7, 8, 40
    g = torch.Generator().manual_seed(43)
    x = _pool_input('levels', N, Cc, Ho, Wo, g)
    dy = rb(torch.randn(N, Ho, Wo, Cc, generator=g))
    assert _tie_share(x) >= 0.25
    y_ref, dx_ref = _pool_reference(x, dy, False)
    _, dz_ref = _pool_reference(x, dy, True)

    def wide_of(t):
        full = rb(torch.randn(t.shape[:3] + (wide,), generator=g) + 2.0)
        full[..., off:off + Cc] = t
        return nhwc_dev(full)[0]

    xw, aw, dyw = wide_of(x), wide_of(F.relu(x)), wide_of(dy)
    keep_y = rb(torch.randn(N, Ho, Wo, wide, generator=g)).bfloat16()
    keep_x = rb(torch.randn(N, 2 * Ho, 2 * Wo, wide, generator=g)).bfloat16()
    for which, keep, ref in (('y', keep_y, y_ref), ('dx', keep_x, dx_ref), ('dz', keep_x, dz_ref)):
        ow, ob = nhwc_dev(keep.float())
        o = ops.cslice(ow, off, Cc)
        if which == 'y':
            ops.maxpool_fwd(ops.cslice(xw, off, Cc), o)
        elif which == 'dx':
            ops.maxpool_bwd(ops.cslice(xw, off, Cc), ops.cslice(dyw, off, Cc), o)
        else:
            ops.maxpool_bwd(ops.cslice(aw, off, Cc), ops.cslice(dyw, off, Cc), o, relu_mask=True)
        ob = ob.cpu()
        assert torch.equal(ob[..., off:off + Cc].float().permute(0, 3, 1, 2), ref), 'sliced maxpool ' + which
        same_bits(ob[..., :off], keep[..., :off], which + ': channels below the slice')
        same_bits(ob[..., off + Cc:], keep[..., off + Cc:], which + ': channels above the slice')


# ---- gcc_pool_linear_fwd / gcc_pool_linear_bwd ----------------------------------------------------------------------------
# (N, C, H, W): C 1 | < 64 and no multiple of 8 | one channel group | two | past 256 (linear_head's second trip, the weight
# gradient's second workgroup) | the production head; HW 1 | 5 | 31, 32, 33 (one trip of the 32 pixel lanes, and one pixel more) | 576
HEAD_CASES = [(1, 1, 1, 1), (3, 20, 3, 11), (1, 64, 4, 8), (3, 72, 1, 31), (1, 300, 1, 5), (3, 300, 3, 11), (3, 64, 1, 1),
              (1, 72, 16, 36), (3, 1, 4, 8), (3, 512, 16, 36)]
PAD_VALUE = 30000.0               # in the lanes [C, ld) of x: a single one of them in a mean of |x| ~ 1 would show


@functools.lru_cache(maxsize=None)
def _head_data(N, Cc, H, W):
    g = torch.Generator().manual_seed(Cc * 1000 + H * W + N)
    x = rb(torch.randn(N, H, W, Cc, generator=g) + 0.25)
    w = torch.randn(Cc, generator=g) * 0.2
    b = torch.randn(1, generator=g)
    dl = rb(torch.randn(N, generator=g))
    return x, w, b, dl


def _head_forward(ops, N, Cc, H, W):
    x, w, b, dl = _head_data(N, Cc, H, W)
    xd, _ = nhwc_dev(x, pad=PAD_VALUE)
    wd, bd = w.to(DEV), b.to(DEV)
    pooled = torch.full((N * Cc + 8,), 7.0, device=DEV)
    logit = ops.new_act(N, 1, 1, 1, DEV)
    ops.pool_linear_fwd(xd, wd, bd, pooled, logit)
    dld, _ = nhwc_dev(dl.view(N, 1, 1, 1))
    return xd, wd, bd, pooled, logit, dld


def _half_ulp_bf16(v):
    """half a unit in the last place of the bf16 grid (8 significant bits) at magnitude |v| (fp64 tensor)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 8)


def _dw_db_reference(dl, pooled_got, w0, b0, N):
    """dw[c] += sum_n dl[n] pooled[n][c]: N products (dl bf16, pooled fp32: each rounded, or fused into the add) and N serial adds
    into a register that starts at 0, then the `+=`: at most 2 N + 1 roundings on a term's way; db += sum_n dl[n]: N + 1"""
    t = dl.double()[:, None] * pooled_got.double()
    dw_ref, dw_lim = w0.double() + t.sum(0), (2 * N + 1) * U * (t.abs().sum(0) + w0.double().abs())
    db_ref, db_lim = b0 + dl.double().sum().item(), (N + 1) * U * (dl.double().abs().sum().item() + abs(b0))
    return dw_ref, dw_lim, db_ref, db_lim


@pytest.mark.parametrize('case', HEAD_CASES, ids=lambda c: '%dx%dx%dx%d' % c)
def test_pool_linear_forward_backward(case):
    ops = _ops()
    N, Cc, H, W = case
    HW = H * W
    x, w, b, dl = _head_data(N, Cc, H, W)
    xd, wd, bd, pooled, logit, dld = _head_forward(ops, N, Cc, H, W)
    pooled = pooled.cpu()
    assert torch.all(pooled[N * Cc:] == 7.0), 'pooled: written past [N][C]'
    got = pooled[:N * Cc].view(N, Cc)
    # pool_mean_kernel: a pixel lane adds its ceil(HW / 32) values serially, thread c then adds the 32 lanes serially, one
    # division: ceil(HW / 32) + 32 roundings at most (the first add of either chain, into 0, is exact: the division takes its place)
    xs = x.double()
    ref = xs.mean((1, 2))
    lim = (-(-HW // 32) + 32) * U * xs.abs().sum((1, 2)) / HW
    err = (got.double() - ref).abs()
    print('pooled %s: max err / bound %.3g' % (case, (err / lim).max().item()))
    assert bool((err <= lim).all()), 'pooled: err %.3g, bound %.3g at its worst' % (err.max().item(), lim[err.argmax() // Cc, err.argmax() % Cc])
    # linear_head_kernel: thread t adds pooled[c] * w[c] for c = t, t + 256, ..: ceil(C / 256) products and adds (2 roundings each,
    # 1 if fused), wave_sum 6, block sum 3, `+ b` 1; then ONE rounding to bf16: half a bf16 ulp of the result
    lref = got.double() @ w.double() + b.double()
    acc = (2 * -(-Cc // 256) + 6 + 3 + 1) * U * ((got.double().abs() * w.double().abs()).sum(1) + b.double().abs())
    llim = acc + _half_ulp_bf16(lref.abs() + acc)
    lerr = (logit[:, 0, 0, 0].float().cpu().double() - lref).abs()
    print('logit %s: max err / bound %.3g' % (case, (lerr / llim).max().item()))
    assert bool((lerr <= llim).all()), 'logit: %r vs %r' % (logit[:, 0, 0, 0].float().cpu().tolist(), lref.tolist())
    # backward, all three outputs: two launches (dx; dw and db together)
    g = torch.Generator().manual_seed(5)
    w0, b0 = torch.randn(Cc, generator=g), 0.75
    dw, db = w0.to(DEV), torch.full((1,), b0, device=DEV)
    dxd, dxb = out_dev(N, Cc, H, W)
    torch.cuda.synchronize()
    ops.lib().gcc_launch_count(1)
    ops.pool_linear_bwd(dld, wd, pooled[:N * Cc].to(DEV), xd, dx=dxd, dw=dw, db=db)
    assert int(ops.lib().gcc_launch_count(1)) == 2
    _check_head_dx(dxb.cpu(), dl, w, N, Cc, HW)
    dw_ref, dw_lim, db_ref, db_lim = _dw_db_reference(dl, got, w0, b0, N)
    dwe = (dw.cpu().double() - dw_ref).abs()
    print('dw %s: max err / bound %.3g; db err %.3g, bound %.3g' % (case, (dwe / dw_lim).max().item(), abs(db.item() - db_ref), db_lim))
    assert bool((dwe <= dw_lim).all()), 'dw: err %.3g' % dwe.max().item()
    assert abs(db.item() - db_ref) <= db_lim, 'db: %.9g vs %.9g' % (db.item(), db_ref)


def _check_head_dx(dxb, dl, w, N, Cc, HW):
    """pool_head_bwd_kernel in its own order, fp32: (dlogit * (1 / HW)) * w[c], rounded to bf16 once; the same for every pixel"""
    inv = torch.ones(1) / torch.tensor([float(HW)])
    ref = ((dl * inv)[:, None] * w[None, :]).bfloat16()
    same_bits(dxb[..., :Cc], ref[:, None, None, :].expand(dxb.shape[:3] + (Cc,)).contiguous(), 'pool + linear dx')
    pad_lanes_zero(dxb, Cc, 'pool + linear dx')


@pytest.mark.parametrize('which', ['dx', 'dw', 'dw+db', 'db'])
@pytest.mark.parametrize('case', [(3, 20, 3, 11), (3, 512, 16, 36)], ids=lambda c: '%dx%dx%dx%d' % c)
def test_pool_linear_backward_each_output_alone(case, which):
    """dx, dw and db are each optional: the ones asked for are computed (dw and db in one launch), the others not touched"""
    ops = _ops()
    N, Cc, H, W = case
    x, w, b, dl = _head_data(N, Cc, H, W)
    xd, wd, bd, pooled, logit, dld = _head_forward(ops, N, Cc, H, W)
    got = pooled[:N * Cc].cpu().view(N, Cc)
    g = torch.Generator().manual_seed(6)
    w0, b0 = torch.randn(Cc, generator=g), -1.25
    dw, db = w0.to(DEV), torch.full((1,), b0, device=DEV)
    dxd, dxb = out_dev(N, Cc, H, W)
    torch.cuda.synchronize()
    ops.lib().gcc_launch_count(1)
    ops.pool_linear_bwd(dld, wd, pooled[:N * Cc], xd, dx=dxd if which == 'dx' else None, dw=dw if 'dw' in which else None,
                        db=db if 'db' in which else None)
    assert int(ops.lib().gcc_launch_count(1)) == 1
    dw_ref, dw_lim, db_ref, db_lim = _dw_db_reference(dl, got, w0, b0, N)
    if which == 'dx':
        _check_head_dx(dxb.cpu(), dl, w, N, Cc, H * W)
    else:
        assert float((dxb.float() - 1.0).abs().max()) == 0.0, 'dx was not asked for'
    if 'dw' in which:
        assert bool(((dw.cpu().double() - dw_ref).abs() <= dw_lim).all()), 'dw'
    else:
        assert torch.equal(dw.cpu(), w0), 'dw was not asked for'
    if 'db' in which:
        assert abs(db.item() - db_ref) <= db_lim, 'db: %.9g, expected %.9g + %.9g = %.9g' % (db.item(), b0, db_ref - b0, db_ref)
    else:
        assert db.item() == b0, 'db was not asked for'
