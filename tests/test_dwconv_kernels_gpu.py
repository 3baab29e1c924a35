"""dwconv.hip at the shapes a pruned MobileResnet runs: gcc_dwconv3x3_reflect (forward, backward-data),
gcc_dwconv3x3_reflect_wgrad and gcc_reflect_pad (forward, adjoint), each against plain PyTorch on the CPU in float64 from the
same bf16-rounded inputs and the fp32 masters as they are.

Every bound is per element, c * u * sum|terms| plus the rounding of the stored output (u: unit roundoff of the format the sum
is kept in; c: four times the longest serial chain of the kernel's loops at that shape):

  forward / backward-data   at most 36 products + the bias, summed in fp32 in one chain (c = 4 * 37 < 2^8, u = 2^-24 -> 2^-16;
                            the products of a bf16 value and an fp32 weight round once more: 2^-17 is kept as the issue states it
                            and is met with room, see docs/lab_notebook.md), stored as bf16 (one rounding, at most 2^-8):
                                |err| <= 2^-7 |ref| + 2^-17 sum|w v|
  weight / bias gradient    a thread adds `chain` = ceil(pixels / (blocks * PPB)) pixels in fp32, PPB threads of a workgroup are
                            added in fp32, the workgroups' partial sums in four fp32 chains of blocks / 32 each and then in fp64;
                            the result is added to the preset in fp32:
                                |err| <= 1e-5 * max(1, chain / 64) * sum|dy x| + 2^-22 |preset|
                            (1e-5 ~ 4 * 64 * 2^-24 * 0.66: the issue's figure for chains of up to 64 pixels)
  reflect_pad forward       a copy: exact
  reflect_pad adjoint       at most 9 bf16 values summed in fp32, stored as bf16:  |err| <= 2^-7 |ref| + 1e-37
                            (the floor: sums that land among the bf16 denormals)

The finalize kernel's sum order is also checked bit for bit: the workgroups' partial sums are read back from the workspace and
added on the CPU in the order the kernel documents (8 slices x 4 fp32 chains, then fp64) -- a change of that order is a change
of the bits a resumed run reproduces."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._perelem import UNSUPPORTED, report as _report, within
from tests.test_kernels_gpu import BAD_ARG, DEV, _ops, full_view, rb, to_cpu, to_dev

pytestmark = pytest.mark.gpu

def _geometry(Cc):
    """dw_setup: 4-channel slices, padded to a power of two; pixels a workgroup walks at a time"""
    CH4 = (Cc + 7) // 8 * 2
    CHP = 1
    while CHP < CH4:
        CHP *= 2
    return CH4, 256 // CHP


def _blocks(N, Cc, H, W):
    CH4, PPB = _geometry(Cc)
    return min(512, max(1, -(-N * H * W // (4 * PPB)))), PPB


@functools.lru_cache(maxsize=None)
def _case(N, Cc, H, W):
    """inputs and the float64 reference of one shape, computed once and shared by the tests of that shape (read only)"""
    g = torch.Generator().manual_seed(1000 * Cc + 10 * H + W)
    x = rb(torch.randn(N, Cc, H, W, generator=g))
    w = torch.randn(Cc, 1, 3, 3, generator=g) * 0.3
    b = torch.randn(Cc, generator=g)
    gy = rb(torch.randn(N, Cc, H, W, generator=g))
    out = {}
    for tag, (xs, ws, bs, gs) in (('', (x.double(), w.double(), b.double(), gy.double())),
                                  ('m', (x.double().abs(), w.double().abs(), b.double().abs(), gy.double().abs()))):
        xr, wr, br = xs.clone().requires_grad_(True), ws.clone().requires_grad_(True), bs.clone().requires_grad_(True)
        y = F.conv2d(F.pad(xr, (1, 1, 1, 1), mode='reflect'), wr, br, groups=Cc)
        y.backward(gs)
        out[tag + 'y'], out[tag + 'dx'], out[tag + 'dw'], out[tag + 'db'] = y.detach(), xr.grad, wr.grad, br.grad
        y0 = F.conv2d(F.pad(xs, (1, 1, 1, 1), mode='reflect'), ws, None, groups=Cc)
        out[tag + 'y0'] = y0
    out.update(x=x, w=w, b=b, gy=gy)
    return out


def fwd_bound(ref, mag):
    return 2.0 ** -7 * ref.abs() + 2.0 ** -17 * mag


def wgrad_bound(mag, chain, preset=None):
    b = 1e-5 * max(1.0, chain / 64.0) * mag
    return b if preset is None else b + 2.0 ** -22 * preset.double().abs()


SMALL_PLANES = [(1, 8, 2, 2), (2, 12, 2, 5), (1, 8, 3, 3), (2, 20, 3, 8), (1, 8, 7, 3), (3, 8, 2, 9)]      # the general branch
SIDES_4_5 = [(1, 8, 4, 4), (2, 16, 4, 9), (1, 8, 5, 4), (2, 24, 9, 4)]        # rows 1 and H - 2 adjacent; the clamped-border branch
CHANNELS = [(3, c, 6, 7) for c in (1, 4, 5, 13, 72, 520, 1024)]               # N = 3: a workgroup's pixel walk crosses images
CASES = SMALL_PLANES + SIDES_4_5 + CHANNELS
_id = lambda s: 'x'.join(map(str, s))


def _pads_zero(t, Cc, what):
    full = full_view(t)
    if full.shape[1] > Cc:
        assert float(full[:, Cc:].abs().max()) == 0.0, what + ': pad channels are not zero'


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_dwconv_forward(case):
    ops = _ops()
    N, Cc, H, W = case
    r = _case(*case)
    y = ops.new_act(N, Cc, H, W, DEV)
    full = torch.as_strided(y, (N, y.stride(3), H, W), y.stride())
    full.fill_(7.0)                                        # the zeros of the pad channels are the kernel's own
    ops.dwconv_fwd(to_dev(r['x']), r['w'].to(DEV), r['b'].to(DEV), y)
    ratio = within(to_cpu(y), r['y'], fwd_bound(r['y'], r['my']), 'dwconv forward %s' % (case,))
    _pads_zero(y, Cc, 'dwconv forward')
    _report('test_dwconv_forward', case, y=ratio)


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_dwconv_backward_data(case):
    """H < 4 or W < 4: the general branch (three candidate rows and columns); a side of 4 or 5: the clamped-border branch with
    rows 1 and H - 2 adjacent; both never reached by a 6 x 9 or larger plane"""
    ops = _ops()
    N, Cc, H, W = case
    r = _case(*case)
    dx = ops.new_act(N, Cc, H, W, DEV)
    torch.as_strided(dx, (N, dx.stride(3), H, W), dx.stride()).fill_(7.0)
    ops.dwconv_bwd_data(to_dev(r['gy']), r['w'].to(DEV), dx)
    ratio = within(to_cpu(dx), r['dx'], fwd_bound(r['dx'], r['mdx']), 'dwconv backward-data %s' % (case,))
    _pads_zero(dx, Cc, 'dwconv backward-data')
    _report('test_dwconv_backward_data', case, dx=ratio)


def _finalize_on_cpu(partial, blocks, preset):
    """dwconv_wgrad_finalize_kernel's sums in its own order: slice sl of 8 adds blocks sl, sl + 8, ... -- four fp32 chains while
    four more are there (b + 24 < blocks), one chain for the rest -- the four go to fp64 as (a0 + a1) + (a2 + a3), the slices are
    added in fp64 in order, the sum is rounded to fp32 and added to the preset in fp32.  partial: [blocks, 10, C4] fp32."""
    P = partial.astype(np.float32)
    total = np.zeros(P.shape[1:], np.float64)
    for sl in range(8):
        a = [np.zeros(P.shape[1:], np.float32) for _ in range(4)]
        b = sl
        while b + 24 < blocks:
            for j in range(4):
                a[j] = a[j] + P[b + 8 * j]
            b += 32
        while b < blocks:
            a[0] = a[0] + P[b]
            b += 8
        total = total + ((a[0].astype(np.float64) + a[1].astype(np.float64)) + (a[2].astype(np.float64) + a[3].astype(np.float64)))
    return (preset.astype(np.float32) + total.astype(np.float32)).astype(np.float32)


def _wgrad_check(case, name, preset=False, want_blocks=None):
    ops = _ops()
    N, Cc, H, W = case
    r = _case(*case)
    blocks, PPB = _blocks(*case)
    CH4, _ = _geometry(Cc)
    ws_bytes = ops.lib().gcc_dwconv3x3_wgrad_workspace(N, H, W, Cc)
    assert ws_bytes == blocks * 10 * CH4 * 4 * 4, (ws_bytes, blocks, CH4)
    if want_blocks is not None:
        assert ws_bytes // (10 * CH4 * 4 * 4) == want_blocks, (case, ws_bytes // (10 * CH4 * 4 * 4), want_blocks)
    chain = -(-N * H * W // (blocks * PPB))
    g = torch.Generator().manual_seed(7 + Cc)
    dw0 = torch.randn(Cc, 1, 3, 3, generator=g) * 5 if preset else torch.zeros(Cc, 1, 3, 3)
    db0 = torch.randn(Cc, generator=g) * 5 if preset else torch.zeros(Cc)
    dw, db = dw0.to(DEV), db0.to(DEV)
    ops.dwconv_wgrad(to_dev(r['x']), to_dev(r['gy']), dw, db)
    torch.cuda.synchronize()
    rw = within(dw.cpu(), dw0.double() + r['dw'], wgrad_bound(r['mdw'], chain, dw0), '%s dw %s' % (name, case))
    rbias = within(db.cpu(), db0.double() + r['db'], wgrad_bound(r['mdb'], chain, db0), '%s dbias %s' % (name, case))
    # the sum order of the finalize kernel, from the partial sums the first kernel left in the workspace
    part = ops.workspace(ws_bytes, torch.device(DEV), 'dwwgrad')[:ws_bytes].cpu().numpy().view(np.float32).reshape(blocks, 10, CH4 * 4)
    want = _finalize_on_cpu(part[:, :, :Cc], blocks, np.concatenate([dw0.reshape(Cc, 9).numpy().T, db0.numpy()[None]], 0))
    got = np.concatenate([dw.cpu().reshape(Cc, 9).numpy().T, db.cpu().numpy()[None]], 0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), '%s %s: finalize sum order: %d of %d values differ' % (
        name, case, int((got.view(np.uint32) != want.view(np.uint32)).sum()), got.size)
    _report(name, case, dw=rw, dbias=rbias, blocks=blocks, chain=chain)


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_dwconv_weight_gradient(case):
    _wgrad_check(case, 'test_dwconv_weight_gradient')


# blocks = min(512, ceil(pixels / (4 PPB))): C = 256 -> PPB = 4, C = 1024 -> PPB = 1.  The finalize kernel's unrolled loop takes
# 32 blocks a trip while b + 24 < blocks and its tail 8: 1 and 3 (tail of some slices only), 14 (tail, slices unequal), 32 (one
# full trip, no tail), 37 / 49 / 61 (trip + tail with blocks mod 32 in (0, 8], (8, 24], (24, 32)), 512 exactly
# (pixels = 2048 PPB) and more pixels than the cap covers (every thread walks a second and third round)
BLOCK_CASES = [((1, 256, 2, 2), 1), ((1, 256, 6, 7), 3), ((1, 256, 13, 17), 14), ((2, 256, 16, 16), 32), ((2, 256, 17, 17), 37),
               ((2, 256, 14, 28), 49), ((3, 256, 18, 18), 61), ((2, 1024, 32, 32), 512), ((3, 1024, 32, 32), 512)]


@pytest.mark.parametrize('case,blocks', BLOCK_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_dwconv_weight_gradient_block_counts(case, blocks):
    """each case asserts the block count it was chosen for from the workspace query: a retune fails here instead of silently
    losing the coverage; dw and dbias accumulate into a random preset"""
    N, Cc, H, W = case
    if blocks == 512 and N == 2:
        assert N * H * W == 2048 * _geometry(Cc)[1]
    if blocks == 512 and N == 3:
        assert N * H * W > 2048 * _geometry(Cc)[1]
    _wgrad_check(case, 'test_dwconv_weight_gradient_block_counts', preset=True, want_blocks=blocks)


def test_dwconv_block_count_set_is_the_intended_one():
    got = [b for _, b in BLOCK_CASES]
    assert 1 in got and any(1 < b < 8 for b in got) and any(9 <= b <= 31 and b % 8 for b in got) and 32 in got
    over = [b % 32 for b in got if 32 < b < 512]
    assert any(0 < m <= 8 for m in over) and any(8 < m <= 24 for m in over) and any(24 < m < 32 for m in over)
    assert got.count(512) == 2
    for case, b in BLOCK_CASES:
        assert _blocks(*case)[0] == b, (case, _blocks(*case)[0], b)


def test_dwconv_strides():
    """x, dy and the outputs each at a different ld > ceil8(C); the channels beyond ceil8(C) of an output row are not the
    kernel's: unchanged bit for bit"""
    ops = _ops()
    case = (2, 20, 5, 6)
    N, Cc, H, W = case
    r = _case(*case)
    xd, gd = to_dev(r['x'], ld=40), to_dev(r['gy'], ld=48)
    wd, bd = r['w'].to(DEV), r['b'].to(DEV)
    ratios = {}
    for what, ld in (('y', 32), ('dx', 56)):
        out = ops.new_act(N, Cc, H, W, DEV, ld=ld)
        torch.as_strided(out, (N, ld, H, W), out.stride()).fill_(7.0)
        if what == 'y':
            ops.dwconv_fwd(xd, wd, bd, out)
        else:
            ops.dwconv_bwd_data(gd, wd, out)
        ratios[what] = within(to_cpu(out), r[what], fwd_bound(r[what], r['m' + what]), 'strided ' + what)
        full = full_view(out)
        assert float(full[:, Cc:24].abs().max()) == 0.0 and bool((full[:, 24:] == 7.0).all()), what
    dw, db = torch.zeros_like(wd), torch.zeros_like(bd)
    ops.dwconv_wgrad(xd, gd, dw, db)
    blocks, PPB = _blocks(*case)
    chain = -(-N * H * W // (blocks * PPB))
    ratios['dw'] = within(dw.cpu(), r['dw'], wgrad_bound(r['mdw'], chain), 'strided dw')
    ratios['dbias'] = within(db.cpu(), r['db'], wgrad_bound(r['mdb'], chain), 'strided dbias')
    _report('test_dwconv_strides', case, **ratios)


def _wide_slice(ops, N, Cc, H, W, src=None):
    """channel slice [8, 8 + Cc) of a buffer of 8 + ceil8(Cc) + 8 channels pre-filled with 7.0; with src: the slice holds it and
    its pad channels are zero (as the kernel that wrote it would have left them)"""
    wide = ops.new_act(N, ops.ceil8(Cc) + 16, H, W, DEV)
    wide.fill_(7.0)
    if src is not None:
        wide[:, 8:8 + ops.ceil8(Cc)] = 0
        wide[:, 8:8 + Cc] = src.bfloat16().to(DEV)
    return wide, ops.cslice(wide, 8, Cc)


def _neighbours_kept(wide, Cc, what, pads_zero=True):
    full = full_view(wide)
    c8 = (Cc + 7) // 8 * 8
    assert bool((full[:, :8] == 7.0).all()) and bool((full[:, 8 + c8:] == 7.0).all()), what + ': neighbouring channels changed'
    if pads_zero and c8 > Cc:
        assert float(full[:, 8 + Cc:8 + c8].abs().max()) == 0.0, what + ': pad channels are not zero'


def test_dwconv_channel_slices():
    ops = _ops()
    case = (2, 20, 5, 6)
    N, Cc, H, W = case
    r = _case(*case)
    xw, xd = _wide_slice(ops, N, Cc, H, W, r['x'])
    gw, gd = _wide_slice(ops, N, Cc, H, W, r['gy'])
    wd, bd = r['w'].to(DEV), r['b'].to(DEV)
    ratios = {}
    for what in ('y', 'dx'):
        ow, out = _wide_slice(ops, N, Cc, H, W)
        if what == 'y':
            ops.dwconv_fwd(xd, wd, bd, out)
        else:
            ops.dwconv_bwd_data(gd, wd, out)
        ratios[what] = within(to_cpu(out), r[what], fwd_bound(r[what], r['m' + what]), 'sliced ' + what)
        _neighbours_kept(ow, Cc, 'sliced ' + what)
    dw, db = torch.zeros_like(wd), torch.zeros_like(bd)
    ops.dwconv_wgrad(xd, gd, dw, db)
    blocks, PPB = _blocks(*case)
    chain = -(-N * H * W // (blocks * PPB))
    ratios['dw'] = within(dw.cpu(), r['dw'], wgrad_bound(r['mdw'], chain), 'sliced dw')
    ratios['dbias'] = within(db.cpu(), r['db'], wgrad_bound(r['mdb'], chain), 'sliced dbias')
    for wide, what in ((xw, 'x'), (gw, 'dy')):
        _neighbours_kept(wide, Cc, 'input ' + what)
    _report('test_dwconv_channel_slices', case, **ratios)


def test_dwconv_accumulation_and_null_arguments():
    """dw / dbias += into random presets; dbias = None leaves dw the same bits; forward without a bias"""
    ops = _ops()
    case = (2, 12, 5, 6)
    N, Cc, H, W = case
    r = _case(*case)
    xd, gd, wd = to_dev(r['x']), to_dev(r['gy']), r['w'].to(DEV)
    g = torch.Generator().manual_seed(3)
    dw0, db0 = torch.randn(Cc, 1, 3, 3, generator=g) * 4, torch.randn(Cc, generator=g) * 4
    blocks, PPB = _blocks(*case)
    chain = -(-N * H * W // (blocks * PPB))
    dw, db = dw0.to(DEV), db0.to(DEV)
    ops.dwconv_wgrad(xd, gd, dw, db)
    rw = within(dw.cpu(), dw0.double() + r['dw'], wgrad_bound(r['mdw'], chain, dw0), 'preset dw')
    rbias = within(db.cpu(), db0.double() + r['db'], wgrad_bound(r['mdb'], chain, db0), 'preset dbias')
    dw2 = dw0.to(DEV)
    ops.dwconv_wgrad(xd, gd, dw2, None)
    assert torch.equal(dw2, dw), 'dbias = None changed dw'
    y = ops.new_act(N, Cc, H, W, DEV)
    ops.dwconv_fwd(xd, wd, None, y)
    ry = within(to_cpu(y), r['y0'], fwd_bound(r['y0'], r['my0']), 'forward without bias')
    _report('test_dwconv_accumulation_and_null_arguments', case, dw=rw, dbias=rbias, y_nobias=ry)


def test_dwconv_refuses_more_than_1024_channels():
    ops = _ops()
    lib = ops.lib()
    Cc = 1032
    x, out = ops.new_act(1, Cc, 2, 2, DEV), ops.new_act(1, Cc, 2, 2, DEV)
    w, b = torch.zeros(Cc, 1, 3, 3, device=DEV), torch.zeros(Cc, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    xp, op = x.data_ptr(), out.data_ptr()
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    assert lib.gcc_dwconv3x3_wgrad_workspace(1, 2, 2, Cc) == 0
    assert lib.gcc_dwconv3x3_wgrad_workspace(1, 2, 2, 1024) > 0
    assert lib.gcc_dwconv3x3_reflect(0, xp, Cc, None, 0, op, Cc, w.data_ptr(), b.data_ptr(), 1, 2, 2, Cc, ops.stream()) == UNSUPPORTED
    assert lib.gcc_dwconv3x3_reflect(1, None, 0, xp, Cc, op, Cc, w.data_ptr(), None, 1, 2, 2, Cc, ops.stream()) == UNSUPPORTED
    assert lib.gcc_dwconv3x3_reflect_wgrad(xp, Cc, op, Cc, w.data_ptr(), b.data_ptr(), 1, 2, 2, Cc, ws.data_ptr(), ws.numel(),
                                           ops.stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert lib.gcc_launch_count(0) == 0
    assert float(out.float().abs().max()) == 0.0 and float(w.abs().max()) == 0.0


def test_dwconv_bad_arguments():
    ops = _ops()
    lib = ops.lib()
    x, out = ops.new_act(1, 16, 4, 4, DEV), ops.new_act(1, 16, 4, 4, DEV)
    w, b = torch.zeros(16, 1, 3, 3, device=DEV), torch.zeros(16, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    xp, op, wp, bp, s = x.data_ptr(), out.data_ptr(), w.data_ptr(), b.data_ptr(), ops.stream()
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    for H, W in ((1, 16), (16, 1), (1, 1)):                          # a side below 2: ReflectionPad2d(1) does not exist
        assert lib.gcc_dwconv3x3_reflect(0, xp, 16, None, 0, op, 16, wp, bp, 1, H, W, 16, s) == BAD_ARG
        assert lib.gcc_dwconv3x3_reflect(1, None, 0, xp, 16, op, 16, wp, None, 1, H, W, 16, s) == BAD_ARG
        assert lib.gcc_dwconv3x3_reflect_wgrad(xp, 16, op, 16, wp, bp, 1, H, W, 16, ws.data_ptr(), ws.numel(), s) == BAD_ARG
    assert lib.gcc_dwconv3x3_reflect(0, xp, 12, None, 0, op, 16, wp, bp, 1, 4, 4, 12, s) == BAD_ARG      # ld not a multiple of 8
    assert lib.gcc_dwconv3x3_reflect(0, xp, 16, None, 0, op, 12, wp, bp, 1, 4, 4, 12, s) == BAD_ARG
    assert lib.gcc_dwconv3x3_reflect(1, None, 0, xp, 12, op, 16, wp, None, 1, 4, 4, 12, s) == BAD_ARG
    assert lib.gcc_dwconv3x3_reflect_wgrad(xp, 12, op, 16, wp, bp, 1, 4, 4, 12, ws.data_ptr(), ws.numel(), s) == BAD_ARG
    assert lib.gcc_dwconv3x3_reflect_wgrad(xp, 16, op, 12, wp, bp, 1, 4, 4, 12, ws.data_ptr(), ws.numel(), s) == BAD_ARG
    torch.cuda.synchronize()
    assert lib.gcc_launch_count(0) == 0


# ---- reflect_pad ----------------------------------------------------------------------------------------------------------------
def _pad_ref(x, gy, pad):
    xr = x.double().requires_grad_(True)
    ref = F.pad(xr, (pad,) * 4, mode='reflect')
    ref.backward(gy.double())
    return ref.detach(), xr.grad


def _pad_shapes(pad):
    # H == pad + 1: for pad 3 one source pixel collects three padded positions per axis; C = 3: the image in front of the
    # first 7 x 7 convolution
    return [(1, 3, pad + 1, pad + 1), (3, 20, pad + 1, 11), (2, 64, 12, pad + 2), (1, 8, 5, 5)]


@pytest.mark.parametrize('pad', [1, 3])
def test_reflect_pad_forward_and_adjoint(pad):
    ops = _ops()
    worst = 0.0
    for shape in _pad_shapes(pad):
        N, Cc, H, W = shape
        g = torch.Generator().manual_seed(pad * 100 + Cc + W)
        x = rb(torch.randn(shape, generator=g))
        gy = rb(torch.randn(N, Cc, H + 2 * pad, W + 2 * pad, generator=g))
        ref, dx_ref = _pad_ref(x, gy, pad)
        out = ops.new_act(N, Cc, H + 2 * pad, W + 2 * pad, DEV)
        ops.reflect_pad(to_dev(x), out, pad)
        assert torch.equal(to_cpu(out).double(), ref), ('reflect pad forward', shape, pad)
        dx = ops.new_act(N, Cc, H, W, DEV)
        ops.reflect_pad(to_dev(gy), dx, pad, backward=True)
        worst = max(worst, within(to_cpu(dx), dx_ref, 2.0 ** -7 * dx_ref.abs() + 1e-37, 'reflect pad adjoint %s pad %d' % (shape, pad)))
    _report('test_reflect_pad_forward_and_adjoint', (pad,), adjoint=worst)


@pytest.mark.parametrize('sliced', [False, True], ids=['strided', 'sliced'])
def test_reflect_pad_strides_and_slices(sliced):
    """source and destination at different ld (strided), or channel slices at offset 8 of wider buffers filled with 7.0
    (sliced): whatever lies beside the ceil8(C) channels of a destination pixel is unchanged bit for bit"""
    ops = _ops()
    pad, shape = 3, (2, 20, 4, 6)
    N, Cc, H, W = shape
    g = torch.Generator().manual_seed(77)
    x = rb(torch.randn(shape, generator=g))
    gy = rb(torch.randn(N, Cc, H + 2 * pad, W + 2 * pad, generator=g))
    ref, dx_ref = _pad_ref(x, gy, pad)
    worst = 0.0
    for backward in (False, True):
        src, want = (gy, dx_ref) if backward else (x, ref)
        Hd, Wd = want.shape[2:]
        if sliced:
            _, sd = _wide_slice(ops, N, Cc, src.shape[2], src.shape[3], src)
            ow, out = _wide_slice(ops, N, Cc, Hd, Wd)
        else:
            sd = to_dev(src, ld=40)
            out = ops.new_act(N, Cc, Hd, Wd, DEV, ld=56)
            torch.as_strided(out, (N, 56, Hd, Wd), out.stride()).fill_(7.0)
        ops.reflect_pad(sd, out, pad, backward=backward)
        if backward:
            worst = within(to_cpu(out), want, 2.0 ** -7 * want.abs() + 1e-37, 'reflect pad adjoint')
        else:
            assert torch.equal(to_cpu(out).double(), want)
        if sliced:
            _neighbours_kept(ow, Cc, 'reflect pad backward=%d' % backward)
        else:
            full = full_view(out)
            assert float(full[:, Cc:24].abs().max()) == 0.0 and bool((full[:, 24:] == 7.0).all())
    _report('test_reflect_pad_strides_and_slices', (int(sliced),), adjoint=worst)


def test_reflect_pad_past_the_block_cap():
    """2 x 363 x 363 padded pixels x 8 channel groups = 2 108 304 work items, past 8192 workgroups x 256: the grid-stride loop
    goes round again for the last of them.  A copy: exact."""
    ops = _ops()
    N, Cc, H, W, pad = 2, 64, 357, 357, 3
    assert N * (H + 2 * pad) * (W + 2 * pad) * (Cc // 8) > 8192 * 256
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, Cc, H, W, generator=g).bfloat16()
    ref = F.pad(x.float(), (pad,) * 4, mode='reflect').bfloat16()
    xd = ops.new_act(N, Cc, H, W, DEV)
    xd.copy_(x.to(DEV))
    out = ops.new_act(N, Cc, H + 2 * pad, W + 2 * pad, DEV)
    ops.reflect_pad(xd, out, pad)
    assert torch.equal(out.cpu(), ref)


def test_reflect_pad_bad_arguments():
    ops = _ops()
    lib = ops.lib()
    x, out = ops.new_act(1, 8, 3, 8, DEV), ops.new_act(1, 8, 16, 16, DEV)
    s = ops.stream()
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    for backward in (0, 1):
        assert lib.gcc_reflect_pad(x.data_ptr(), 8, out.data_ptr(), 8, 1, 3, 8, 8, 3, backward, s) == BAD_ARG     # H == pad
        assert lib.gcc_reflect_pad(x.data_ptr(), 8, out.data_ptr(), 8, 1, 8, 3, 8, 3, backward, s) == BAD_ARG     # W == pad
        assert lib.gcc_reflect_pad(x.data_ptr(), 12, out.data_ptr(), 8, 1, 3, 8, 8, 1, backward, s) == BAD_ARG    # ld
        assert lib.gcc_reflect_pad(x.data_ptr(), 8, out.data_ptr(), 8, 1, 3, 8, 8, 0, backward, s) == BAD_ARG     # no pad
    torch.cuda.synchronize()
    assert lib.gcc_launch_count(0) == 0
