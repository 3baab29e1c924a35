"""Segmented channels: a channel dimension that is the concatenation of two 8-padded parts (the pruned U-Net students' skip | up
inputs, widths like 12|9).  engine.ConvOp(row_split=...) on the transposed up-convs and ConvOp(col_split=...) on the 1x1 transform
convs rest on seg_to_phys / seg_to_logical (common.hpp), the two-kind path of pack_multi_kernel, gcc_conv_wgrad_seg and
wgrad_reduce_kernel<64,4> / <16,16>; each is compared here with the definition: F.conv2d / F.conv_transpose2d in float64 on the
concatenated LOGICAL tensors (autograd for both gradients), from the same bf16-rounded values.

The physical operands are built the way the engine builds them: each part at its 8-aligned offset (0 and ceil8(split)), pad lanes
zero.  The second part is drawn at 3x the scale of the first, so a mapping that is off by the pad gap lands far outside tolerance.
Tolerances are the suite's: bf16 tensors close() default (1.2e-2 max|ref| + 1e-6), fp32 weight gradients tol 5e-3 floor 1e-4,
packings bit-exact.

test_segmented_conv_exact runs the same nine cases on the data of tests/_conv_exact.py: integers (every logical position bit for
bit, exact zeros in the pad and gap lanes) and seeded normals against float64 with the per-element bounds bound_out / bound_wgrad."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import _conv_exact as X
from tests._perelem import within
from tests.test_kernels_gpu import BAD_ARG, DEV, ERR_WORKSPACE, _ops, close, full_view, rb

pytestmark = pytest.mark.gpu


def ceil8(v):
    return (v + 7) & ~7


def seg_index(n, split):
    """physical positions of the n logical channels, and the physical size (the definition the C side is held to)"""
    if 0 < split < n:
        return list(range(split)) + [ceil8(split) + j for j in range(n - split)], ceil8(split) + ceil8(n - split)
    return list(range(n)), ceil8(n)


def draw(g, shape, split, dim, scale=1.0):
    """bf16-rounded values; along `dim` the part behind `split` at 3x the scale of the first"""
    t = torch.randn(shape, generator=g) * scale
    if 0 < split < shape[dim]:
        t.narrow(dim, split, shape[dim] - split).mul_(3.0)
    return rb(t)


def to_phys(x, split, pad_value=0.0):
    """logical fp32 [N, C, H, W] -> physical NHWC bf16 activation, parts at 0 and ceil8(split); pad lanes = pad_value"""
    ops = _ops()
    N, Cc, H, W = x.shape
    _, P = seg_index(Cc, split)
    t = ops.new_act(N, P, H, W, DEV)
    if pad_value:
        t.fill_(pad_value)
    if 0 < split < Cc:
        ops.nchw_to_nhwc(x[:, :split].contiguous().to(DEV), t, 0, None if pad_value else ceil8(split))
        ops.nchw_to_nhwc(x[:, split:].contiguous().to(DEV), t, ceil8(split), None if pad_value else ceil8(Cc - split))
    else:
        ops.nchw_to_nhwc(x.to(DEV), t, 0, None if pad_value else P)
        t = t[:, :Cc]
    return t


def check_act(got, ref, split, what):
    """logical channels against ref (close() default), every other lane of the buffer exactly zero"""
    idx, _ = seg_index(ref.shape[1], split)
    full = full_view(got)
    err = (full[:, idx] - ref.float()).abs().max().item()
    print('%s: max err %.3g (limit %.3g)' % (what, err, 1.2e-2 * ref.abs().max().item() + 1e-6))
    close(full[:, idx], ref.float(), what=what)
    pad = sorted(set(range(full.shape[1])) - set(idx))
    if pad:
        assert float(full[:, pad].abs().max()) == 0.0, '%s: pad lanes %s are not zero' % (what, pad)


def produced(N, Cc, split, H, W):
    """the buffer a forward / data-gradient call writes.  A segmented dimension is handed to the kernel with its physical channel
    count, so the kernel itself writes every lane, the pad lanes and the gap included (zeros, from the zero rows of the packing):
    the buffer starts out as ones and the zeros found later are the kernel's own.  An unsplit width that is no multiple of 8
    keeps the suite's contract for such buffers (test_conv_fprop_dgrad_wgrad): zero-initialised by ops.new_act, lanes >= C stay
    zero."""
    ops = _ops()
    idx, P = seg_index(Cc, split)
    if not 0 < split < Cc:
        return ops.new_act(N, Cc, H, W, DEV)
    t = ops.new_act(N, P, H, W, DEV)
    t.fill_(1.0)
    return t


def packed_definition(w, row_split, col_split):
    """W [rows_p][taps][cols_p] and Wt [cols_p][taps][rows_p] in bf16 from the logical fp32 master [rows, cols, k, k]"""
    rows, cols, k, _ = w.shape
    ri, rp = seg_index(rows, row_split)
    ci, cp = seg_index(cols, col_split)
    W = torch.zeros(rp, k * k, cp, dtype=torch.bfloat16)
    W[torch.tensor(ri)[:, None], :, torch.tensor(ci)[None, :]] = w.reshape(rows, cols, k * k).to(torch.bfloat16)
    return W, W.permute(2, 1, 0).contiguous()


def make_conv(w, k, s, p, transposed, row_split, col_split):
    from gcc_amd import engine
    m = torch.nn.Parameter(w.to(DEV).contiguous(memory_format=torch.channels_last))
    m.grad = torch.zeros_like(m)
    c = engine.ConvOp(m, None, k, s, p, transposed, row_split=row_split, col_split=col_split)
    assert (c.row_split, c.col_split) == (row_split, col_split)
    return c


# rows, row_split, cols, col_split, k, s, p, transposed, N, conv-input H, W, wgrad_wgs (0: the default plan),
# slabs meant (0: not pinned)
UP = (21, 12, 24, 0, 4, 2, 1, True)
CASES = {
    '1_transform_one_slab_gap4': (32, 0, 20, 12, 1, 1, 0, False, 2, 12, 12, 0, 0),
    '2_transform_gap5_ragged': (40, 0, 13, 3, 1, 1, 0, False, 3, 37, 29, 0, 0),
    '3_up_row_split': UP + (2, 16, 16, 0, 0),
    '4_up_gap1_irregular_cols': (19, 7, 10, 0, 4, 2, 1, True, 2, 16, 16, 0, 0),
    '5_both_splits': (13, 5, 20, 12, 3, 1, 1, False, 2, 10, 14, 0, 0),
    '6_up_8_slabs': UP + (4, 64, 64, 0, 8),            # <64,4>: tail loop only
    '7_up_29_slabs': UP + (4, 128, 128, 87, 29),       # <64,4>: split lane 0 takes the unrolled loop once (z + 28 < 29)
    '8_up_32_slabs': UP + (4, 128, 128, 0, 32),        # <16,16>: tail loop only
    '9_up_128_slabs': UP + (4, 256, 256, 0, 128),      # <16,16>: every split lane takes the unrolled loop (z + 112 < 128)
}


@pytest.fixture
def wgrad_plan():
    ops = _ops()
    ops.set_plan()

    def choose(wgs):
        ops.set_plan(**({'wgrad_wgs': wgs} if wgs else {}))
    yield choose
    ops.set_plan()


@pytest.mark.parametrize('fused', [1, 0])
@pytest.mark.parametrize('name', [n for n in CASES if n[0] in '12345'])
def test_segmented_packing(name, fused, monkeypatch):
    """W and Wt of a PackPlan run against the definition, bit for bit over the WHOLE packed tensors: logical positions, zero pad
    rows / columns, the gap between the parts.  The packings are filled with ones first: the zeros are the launch's own.
    A segmented tensor is packed by work items of kinds 0 and 1 whatever FUSED_PACK says (kind 2, one read of the master for both
    packings, takes unsplit tensors only): both settings must build that same two-kind plan and give the same bits.  Nothing
    here covers the fused path; tests/test_kernels_gpu.py::test_pack_plan_matches_single_tensor_packing does."""
    ops = _ops()
    monkeypatch.setattr(ops, 'FUSED_PACK', bool(fused))
    rows, rs, cols, cs, k, s, p, tr = CASES[name][:8]
    g = torch.Generator().manual_seed(rows * 100 + cols)
    w = draw(g, (rows, cols, k, k), rs, 0, 0.1)
    if 0 < cs < cols:
        w = torch.cat([w[:, :cs], rb(w[:, cs:] * 3.0)], 1)
    c = make_conv(w, k, s, p, tr, rs, cs)
    c.w.fill_(1.0)
    c.wt.fill_(1.0)
    plan = ops.PackPlan([c], DEV)
    assert set(int(v) for v in plan.d_items.cpu()[:, 1]) == {0, 1}, 'segmented tensors keep the two-kind path'
    plan.run()
    torch.cuda.synchronize()
    W, Wt = packed_definition(w, rs, cs)
    assert c.w.shape == W.shape and c.wt.shape == Wt.shape
    assert torch.equal(c.w.cpu(), W), 'W'
    assert torch.equal(c.wt.cpu(), Wt), 'Wt'


@pytest.mark.parametrize('name', list(CASES))
def test_segmented_conv(name, wgrad_plan):
    ops = _ops()
    rows, rs, cols, cs, k, s, p, tr, N, H, W, wgs, slabs = CASES[name]
    g = torch.Generator().manual_seed(N * 1000 + H + rows)
    w = draw(g, (rows, cols, k, k), rs, 0, 0.1)
    if 0 < cs < cols:
        w = torch.cat([w[:, :cs], rb(w[:, cs:] * 3.0)], 1)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    # x: the layer's input, dy: the gradient of its output (logical tensors)
    if tr:      # ConvTranspose2d(rows -> cols): small image in, the adjoint conv's input size (H x W) out
        x = draw(g, (N, rows, Ho, Wo), rs, 1)
        xs, ys = rs, cs
        dy = draw(g, (N, cols, H, W), cs, 1)
    else:
        x = draw(g, (N, cols, H, W), cs, 1)
        xs, ys = cs, rs
        dy = draw(g, (N, rows, Ho, Wo), rs, 1)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = F.conv_transpose2d(xr, wr, None, stride=s, padding=p) if tr else F.conv2d(xr, wr, None, stride=s, padding=p)
    assert y_ref.shape == dy.shape
    y_ref.backward(dy.double())
    dw_ref = wr.grad.float()

    wgrad_plan(wgs)
    c = make_conv(w, k, s, p, tr, rs, cs)
    ops.PackPlan([c], DEV).run()
    Wd, Wtd = packed_definition(w, rs, cs)
    assert torch.equal(c.w.cpu(), Wd) and torch.equal(c.wt.cpu(), Wtd), 'packing'

    xd, dyd = to_phys(x, xs), to_phys(dy, ys)
    out = produced(N, dy.shape[1], ys, dy.shape[2], dy.shape[3])
    c.forward(xd, out)
    check_act(out, y_ref.detach(), ys, name + ' forward')
    dx = produced(N, x.shape[1], xs, x.shape[2], x.shape[3])
    c.backward_data(dyd, dx)
    check_act(dx, xr.grad, xs, name + ' data gradient')

    # the split count this case is meant to reach (cases 6-9), from the library's own workspace size
    cx, cdy = (dyd, xd) if tr else (xd, dyd)
    Cip, Cop = ops.seg_phys(cols, cs), ops.seg_phys(rows, rs)
    d = ops.conv_desc(N, H, W, Cip, Cop, k, s, p, cx.stride(3), cdy.stride(3))
    got_slabs = ops.lib().gcc_conv_wgrad_workspace(C.byref(d)) // (Cop * k * k * ceil8(Cip) * 4)
    print('%s: %d slabs' % (name, got_slabs))
    if slabs:
        assert got_slabs == slabs, 'the plan gives %d slabs, this case is written for %d' % (got_slabs, slabs)

    def wclose(got, ref, what):
        err = (got - ref).abs().max().item()
        print('%s %s: max err %.3g (limit %.3g)' % (name, what, err, 5e-3 * ref.abs().max().item() + 1e-4))
        close(got, ref, tol=5e-3, floor=1e-4, what=name + ' ' + what)

    c._backward_weight(xd, dyd)
    wclose(c.weight.grad.cpu(), dw_ref, 'ConvOp weight gradient')
    dw = torch.full_like(c.weight.grad, 7.0)                 # stale contents must not survive a fresh gradient
    ops.conv_wgrad_seg(cx, cdy, dw, rows, cols, rs, cs, k, s, p, accumulate=False)
    fresh = dw.cpu().clone()
    wclose(fresh, dw_ref, 'gcc_conv_wgrad_seg fresh')
    ops.conv_wgrad_seg(cx, cdy, dw, rows, cols, rs, cs, k, s, p, accumulate=True)
    wclose(dw.cpu(), 2 * dw_ref, 'gcc_conv_wgrad_seg accumulate')
    # finite non-zero pad lanes in both operands: the reduce reads logical positions only -> the same bits
    xg, dyg = to_phys(x, xs, pad_value=0.75), to_phys(dy, ys, pad_value=-1.5)
    cxg, cdyg = (dyg, xg) if tr else (xg, dyg)
    dw2 = torch.zeros_like(dw)
    ops.conv_wgrad_seg(cxg, cdyg, dw2, rows, cols, rs, cs, k, s, p, accumulate=False)
    assert torch.equal(dw2.cpu(), fresh), 'pad lanes of x / dy leak into the weight gradient'


def check_act_exact(got, ref, mag, split, kind, K, S, what):
    """every logical lane against ref -- 'int': the one bf16 rounding of the exact value, bit for bit; 'normal': bound_out per
    element -- and every other lane of the buffer exactly zero; returns the largest err / bound"""
    idx, _ = seg_index(ref.shape[1], split)
    full = full_view(got)
    lanes = full[:, idx]
    if kind == 'int':
        want = X.expected_bits(ref)
        bad = lanes.bfloat16().view(torch.int16) != want.view(torch.int16)
        assert not bool(bad.any()), '%s: %d of %d logical elements are not the rounding of the exact value, first at %s' % (
            what, int(bad.sum()), bad.numel(), tuple(int(v) for v in bad.nonzero()[0]))
        worst = 0.0
    else:
        worst = within(lanes, ref, X.bound_out(ref, mag, K, S), what)
    pad = sorted(set(range(full.shape[1])) - set(idx))
    if pad:
        assert float(full[:, pad].abs().max()) == 0.0, '%s: pad / gap lanes %s are not zero' % (what, pad)
    return worst


@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('name', list(CASES))
def test_segmented_conv_exact(name, kind, wgrad_plan):
    """The nine cases of test_segmented_conv on the data of tests/_conv_exact.py, drawn on the LOGICAL tensors.  'int': the weight
    gradient is the exact integer at every logical position -- fresh over a stale fill, exactly twice when accumulating, the same
    bits on a second run and with finite non-zero pad and gap lanes in both operands -- and forward / data gradient are
    expected_bits at every logical lane, exact zeros in every pad and gap lane of a buffer of ones.  'normal': bound_wgrad(mag, M,
    S) with S read from the workspace size, bound_out per element with K the physical products per output and at most one K slice
    per k-step of 64.  The geometry g is the convolution whose weight gradient gcc_conv_wgrad_seg forms: a transposed layer is
    that convolution's adjoint (its forward the data gradient, its data gradient the forward)."""
    ops = _ops()
    rows, rs, cols, cs, k, s, p, tr, N, H, W, wgs, slabs = CASES[name]
    g = (N, H, W, cols, rows, k, s, p)
    d = X.make_data(kind, g, sum(ord(ch) for ch in name))
    Cip, Cop = ops.seg_phys(cols, cs), ops.seg_phys(rows, rs)
    gp = (N, H, W, Cip, Cop, k, s, p)                     # what the kernels multiply: the pad and gap lanes are zero products
    fwd_op, bwd_op = ('D', 'F') if tr else ('F', 'D')
    x, dy = (d['dy'], d['x']) if tr else (d['x'], d['dy'])     # the LAYER's input and the gradient of its output
    xs, ys = (rs, cs) if tr else (cs, rs)
    y_ref, _, y_mag = X.reference(fwd_op, d, g)
    dx_ref, _, dx_mag = X.reference(bwd_op, d, g)
    dw_ref, dw_mag = X.ref_wgrad(d, g)
    if kind == 'int':
        for m, what in ((y_mag, 'forward'), (dx_mag, 'data gradient'), (2 * dw_mag + 7, 'weight gradient, accumulated')):
            X.assert_exact_condition(m, name + ' ' + what)

    wgrad_plan(wgs)
    c = make_conv(d['w'].float(), k, s, p, tr, rs, cs)
    ops.PackPlan([c], DEV).run()
    xd, dyd = to_phys(x.float(), xs), to_phys(dy.float(), ys)
    ratios = {}
    out = produced(N, dy.shape[1], ys, dy.shape[2], dy.shape[3])
    c.forward(xd, out)
    Kf, Kb = X.k_products(gp, fwd_op), X.k_products(gp, bwd_op)
    ratios['fwd'] = check_act_exact(out, y_ref, y_mag, ys, kind, Kf, X.cdiv(Kf, X.BK), '%s %s forward' % (name, kind))
    dx = produced(N, x.shape[1], xs, x.shape[2], x.shape[3])
    c.backward_data(dyd, dx)
    ratios['dgrad'] = check_act_exact(dx, dx_ref, dx_mag, xs, kind, Kb, X.cdiv(Kb, X.BK), '%s %s data gradient' % (name, kind))

    cx, cdy = (dyd, xd) if tr else (xd, dyd)
    dsc = ops.conv_desc(N, H, W, Cip, Cop, k, s, p, cx.stride(3), cdy.stride(3))
    S = ops.lib().gcc_conv_wgrad_workspace(C.byref(dsc)) // (Cop * k * k * ceil8(Cip) * 4)
    if slabs:
        assert S == slabs, 'the plan gives %d slabs, this case is written for %d' % (S, slabs)
    fold = 'wgrad_reduce_kernel<16,16>' if S >= 32 else 'wgrad_reduce_kernel<64,4>'
    print('ROUTE segmented %s %s: %d slabs, %s' % (name, kind, S, fold))
    M = X.k_products(g, 'W')
    dw = torch.full_like(c.weight.grad, 7.0)                  # stale contents must not survive a fresh gradient
    ops.conv_wgrad_seg(cx, cdy, dw, rows, cols, rs, cs, k, s, p, accumulate=False)
    fresh = dw.cpu().clone()
    assert fresh.shape == dw_ref.shape
    if kind == 'int':
        bad = fresh.double() != dw_ref
        assert not bool(bad.any()), '%s: %d of %d weight-gradient entries are not the exact integer, first at %s' % (
            name, int(bad.sum()), bad.numel(), tuple(int(v) for v in bad.nonzero()[0]))
        ops.conv_wgrad_seg(cx, cdy, dw, rows, cols, rs, cs, k, s, p, accumulate=True)
        assert torch.equal(dw.cpu().double(), 2 * dw_ref), name + ': accumulating does not give exactly twice'
        ratios['wgrad'] = 0.0
    else:
        ratios['wgrad'] = within(fresh, dw_ref, X.bound_wgrad(dw_mag, M, S), '%s normal weight gradient' % name)
    again = torch.full_like(dw, -3.0)
    ops.conv_wgrad_seg(cx, cdy, again, rows, cols, rs, cs, k, s, p, accumulate=False)
    assert torch.equal(again.cpu().view(torch.int32), fresh.view(torch.int32)), name + ': a second run gives other bits'
    xg, dyg = to_phys(x.float(), xs, pad_value=0.75), to_phys(dy.float(), ys, pad_value=-1.5)
    cxg, cdyg = (dyg, xg) if tr else (xg, dyg)
    dw2 = torch.zeros_like(dw)
    ops.conv_wgrad_seg(cxg, cdyg, dw2, rows, cols, rs, cs, k, s, p, accumulate=False)
    assert torch.equal(dw2.cpu().view(torch.int32), fresh.view(torch.int32)), name + ': pad / gap lanes of x / dy leak into the weight gradient'
    print('RATIO segmented %s %s %s' % (name, kind, ' '.join('%s=%.3g' % kv for kv in sorted(ratios.items()))))


def _probe(lib, buf, Co, Ci, rows, cols, rs, cs):
    """the seg entry's answer to a descriptor, with a workspace of zero bytes: nothing is launched either way
    (BAD_ARG: refused by the argument checks; ERR_WORKSPACE: accepted, then stopped at the workspace size)"""
    from gcc_amd import _lib
    d = _lib.conv_t(1, 8, 8, Ci, Co, 1, 1, 1, 0, 64, 0, 64, 0)
    p = buf.data_ptr()
    return lib.gcc_conv_wgrad_seg(C.byref(d), p, p, p, rows, cols, rs, cs, 0, p, 0, None)


def test_wgrad_seg_argument_checks():
    ops = _ops()
    lib = ops.lib()
    buf = torch.zeros(8 * 8 * 64, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    assert _probe(lib, buf, 32, 24, 21, 24, 12, 0) == ERR_WORKSPACE       # the up-conv of case 3, as the engine states it
    assert _probe(lib, buf, 24, 24, 21, 24, 12, 0) == BAD_ARG             # Co = ceil8(rows): the gap forgotten
    assert _probe(lib, buf, 21, 24, 21, 24, 12, 0) == BAD_ARG             # logical Co
    assert _probe(lib, buf, 32, 32, 21, 24, 12, 0) == BAD_ARG             # Ci of another width
    assert _probe(lib, buf, 32, 16, 32, 13, 0, 3) == BAD_ARG              # Ci = ceil8(cols) under a column split (case 2: 3 | 10)
    assert _probe(lib, buf, 32, 24, 32, 13, 0, 3) == ERR_WORKSPACE
    for rows, cols in ((0, 24), (-3, 24), (21, 0), (21, -8)):
        assert _probe(lib, buf, 32, 24, rows, cols, 0, 0) == BAD_ARG, (rows, cols)
        assert _probe(lib, buf, ceil8(max(rows, 1)), ceil8(max(cols, 1)), rows, cols, 0, 0) == BAD_ARG, (rows, cols)
    p = buf.data_ptr()
    assert lib.gcc_conv_wgrad_seg(None, p, p, p, 21, 24, 12, 0, 0, p, 0, None) == BAD_ARG
    assert int(lib.gcc_launch_count(1)) == 0, 'every answer above came before any launch'


def test_seg_phys_python_and_c_agree():
    """ops.seg_phys is what the engine sizes buffers and descriptors with; gcc_conv_wgrad_seg accepts exactly that Co for every
    (n, split), n <= 40 -- splits outside (0, n) mean one part -- and no other multiple of 8"""
    ops = _ops()
    lib = ops.lib()
    buf = torch.zeros(8 * 8 * 64, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    for n in range(1, 41):
        for split in range(-1, n + 2):
            want = seg_index(n, split)[1]
            assert ops.seg_phys(n, split) == want, (n, split)
            for Co in range(8, 65, 8):
                rc = _probe(lib, buf, Co, 8, n, 8, split, 0)
                assert rc == (ERR_WORKSPACE if Co == want else BAD_ARG), (n, split, Co, rc)
    assert int(lib.gcc_launch_count(1)) == 0
