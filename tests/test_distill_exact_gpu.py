"""gcc_distill_fwd / gcc_distill_bwd stage by stage from the device's own intermediates (tests/_distill.py states the stages, the
bounds and the composed end-to-end formula): the batched weight gradient and 1x1 product -- grid.y as the problem index, per-problem
strides, the [splits][batch][Co][cols] slabs and their flat / vec fold, plan_splits(c, batch), select_tile(..., batch) -- which no
public convolution entry reaches, gram_diff_kernel, distill_combine_kernel and modes 1 and 2 of scalar_finalize_kernel.

Every case asserts its plan (gcc_distill_plan against the table, the launch counts against gcc_launch_count) BEFORE it compares a
number; the intermediates are read back at the byte offsets the query reports, so the stage-2 bit equality also shows that those
are the offsets the kernels wrote.  Nothing skips; no assertion is relative to max |ref| or to a norm; no element is left out."""
import ctypes as ct

import pytest
import torch

from tests import _distill as D
from tests.test_kernels_gpu import BAD_ARG, DEV, ERR_WORKSPACE, _ops

pytestmark = pytest.mark.gpu

WS_FILL = 0x7f                       # stale workspace bytes: 0x7f7f7f7f is 3.4e38 as fp32, 0x7f7f is 3.4e38 as bf16


def place(x, case):
    """[N, HW, C] float64 -> (buffer [N, HW, 1, ld] bf16 on the device, ld, off): dense, or (windows) at lane 8 of a buffer 16 lanes
    wider whose other lanes hold the sentinel"""
    N, HW, C = x.shape
    off = D.WIN_OFF if case['win'] else 0
    ld = C + (D.WIN_EXTRA if case['win'] else 0)
    buf = torch.full((N, HW, 1, ld), D.SENTINEL, dtype=torch.bfloat16, device=DEV)
    buf[..., off:off + C] = x.bfloat16().view(N, HW, 1, C).to(DEV)
    return buf, ld, off


def view(buf, C, off):
    """the ops.cslice view of a placed buffer: NHWC activation [N, C, HW, 1]"""
    return _ops().cslice(buf.permute(0, 3, 1, 2), off, C)


def outside_is_sentinel(buf, C, off, what):
    lanes = [i for i in range(buf.shape[-1]) if not off <= i < off + C]
    if lanes:
        got = buf[..., lanes].float().cpu()
        assert bool((got == D.SENTINEL).all()), '%s: %d lanes outside the window were written' % (what, int((got != D.SENTINEL).sum()))


def read_ws(ws, plan, case):
    """the five intermediates at the offsets gcc_distill_plan reports, on the CPU"""
    N, C, HW = case['N'], case['C'], case['HW']

    def at(off, n, dt, shape):
        size = 4 if dt == torch.float32 else 2
        return ws[off:off + n * size].view(dt).view(shape).cpu().clone()
    return dict(scal=at(plan['off_scal'], 2, torch.float32, (2,)), Gf=at(plan['off_gf'], N * C * C, torch.float32, (N, C, C)),
                Gt=at(plan['off_gt'], N * C * C, torch.float32, (N, C, C)), S=at(plan['off_s'], N * C * C, torch.bfloat16, (N, C, C)),
                dfg=at(plan['off_dfg'], N * HW * C, torch.bfloat16, (N, HW, C)))


def run_device(case, d, squared, plan, via_ops=False):
    """one forward and one backward call: the intermediates, out2, df [N, HW, C], the whole df buffer, the two launch counts"""
    ops = _ops()
    lib = ops.lib()
    N, C, HW = case['N'], case['C'], case['HW']
    fb, ld, off = place(d['f'], case)
    tb, _, _ = place(d['t'], case)
    dfb = torch.full_like(fb, D.SENTINEL)
    ws = torch.full((plan['ws_bytes'],), WS_FILL, dtype=torch.uint8, device=DEV)
    out2 = torch.full((4,), -7.0, device=DEV)
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    if via_ops:
        ops.distill_fwd(view(fb, C, off), view(tb, C, off), out2, ws, squared=squared)
    else:
        rc = lib.gcc_distill_fwd(fb.data_ptr(), ld, off, tb.data_ptr(), ld, off, N, C, HW, int(squared), out2.data_ptr(), ws.data_ptr(),
                                 ws.numel(), ops.stream())
        assert rc == 0, 'gcc_distill_fwd: %d' % rc
    n_fwd = int(lib.gcc_launch_count(1))
    if via_ops:
        ops.distill_bwd(view(fb, C, off), view(tb, C, off), D.WG, D.WC, view(dfb, C, off), ws, squared=squared)
    else:
        rc = lib.gcc_distill_bwd(fb.data_ptr(), ld, off, tb.data_ptr(), ld, off, N, C, HW, int(squared), D.WG, D.WC, dfb.data_ptr(), ld, off,
                                 ws.data_ptr(), ws.numel(), ops.stream())
        assert rc == 0, 'gcc_distill_bwd: %d' % rc
    n_bwd = int(lib.gcc_launch_count(1))
    torch.cuda.synchronize()
    r = read_ws(ws, plan, case)
    r['out2'] = out2.cpu()
    r['df'] = dfb[..., off:off + C].reshape(N, HW, C).cpu().clone()
    what = '%s squared=%d' % (case['name'], squared)

    def layout():
        """what the calls must leave alone (checked by the caller once the plan and the launch counts stand)"""
        assert float(r['out2'][2]) == -7.0 and float(r['out2'][3]) == -7.0, what + ': out2 written past its two scalars'
        outside_is_sentinel(dfb, C, off, what + ' df')
        outside_is_sentinel(fb, C, off, what + ' f')
        outside_is_sentinel(tb, C, off, what + ' t')
        assert torch.equal(fb[..., off:off + C].cpu().view(N, HW, C).double(), d['f']), what + ': f changed'
        assert torch.equal(tb[..., off:off + C].cpu().view(N, HW, C).double(), d['t']), what + ': t changed'
    r['layout'] = layout
    return r, n_fwd, n_bwd


def same_bits(a, b, what):
    for k in ('Gf', 'Gt', 'S', 'scal', 'out2', 'dfg', 'df'):
        x, y = a[k], b[k]
        if k == 'out2':
            x, y = x[:2], y[:2]
        assert torch.equal(D.bits(x), D.bits(y)), '%s: %s differs' % (what, k)


@pytest.mark.parametrize('case', D.CASES, ids=D.CASE_IDS)
def test_distill_stages(case):
    ops = _ops()
    N, C, HW = case['N'], case['C'], case['HW']
    plan = ops.distill_plan(N, C, HW)
    D.check_plan(case, plan, 'gcc_distill_plan')
    assert plan['ws_bytes'] == ops.distill_workspace_bytes(N, C, HW)
    print(D.route_line(case, plan))
    if N == 1:
        # CycleGAN's batch goes down the ordinary dispatch: the public queries of the same 1x1 convolution name the route and tile
        from gcc_amd import _lib
        dsc = _lib.conv_t(1, 1, HW, C, C, 1, 1, 1, 0, C, 0, C, 0)
        route, tile = ops.lib().gcc_conv_route(ct.byref(dsc), 0, None), ops.lib().gcc_conv_tile(ct.byref(dsc), 0)
        print('ROUTE distill %s batch 1: gcc_conv_route %d, gcc_conv_tile %d' % (case['name'], route, tile))
        assert route == plan['bwd_route'] and tile == plan['bwd_bp'] * 1000 + plan['bwd_bc']
    worst = {}
    for kind in ('int', 'normal'):
        d = D.make_data(kind, case)
        D.assert_images_differ(d)
        for squared in (False, True):
            r, n_fwd, n_bwd = run_device(case, d, squared, plan)
            what = '%s %s squared=%d' % (case['name'], kind, squared)
            assert n_fwd == plan['fwd_launches'], '%s: %d forward launches, the plan says %d' % (what, n_fwd, plan['fwd_launches'])
            assert n_bwd == plan['bwd_launches'], '%s: %d backward launches, the plan says %d' % (what, n_bwd, plan['bwd_launches'])
            r['layout']()
            ratios = D.run_stages(case, d, kind, r, squared)
            print('RATIO distill %s %s squared=%d %s' % (case['name'], kind, squared, ' '.join('%s=%.3g' % kv for kv in sorted(ratios.items()))))
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
            if kind == 'int' and not squared:
                again, _, _ = run_device(case, d, squared, plan)
                same_bits(r, again, what + ' second run')
    print('RATIO distill %s worst %s' % (case['name'], ' '.join('%s=%.3g' % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize('case', [c for c in D.CASES if c['win']], ids=[c['name'] for c in D.CASES if c['win']])
@pytest.mark.parametrize('squared', [False, True])
def test_distill_windows_through_ops(case, squared):
    """ops.distill_fwd / ops.distill_bwd on ops.cslice views (the offset travels in the pointer) against the C entries with
    foff = toff = dfoff = 8: the same bits in every intermediate, the same launches, every lane outside the windows untouched"""
    ops = _ops()
    plan = ops.distill_plan(case['N'], case['C'], case['HW'])
    D.check_plan(case, plan, 'gcc_distill_plan')
    d = D.make_data('normal', case)
    a, af, ab = run_device(case, d, squared, plan)
    b, bf, bb = run_device(case, d, squared, plan, via_ops=True)
    assert (af, ab) == (bf, bb) == (plan['fwd_launches'], plan['bwd_launches'])
    a['layout']()
    b['layout']()
    same_bits(a, b, '%s squared=%d: views against offsets' % (case['name'], squared))
    D.run_stages(case, d, 'normal', b, squared)


def test_distill_refusals():
    """C & 7, a misaligned ld / off and a workspace one byte short are answered before any launch, the outputs untouched"""
    ops = _ops()
    lib = ops.lib()
    case = D.CASES[1]
    N, C, HW = case['N'], case['C'], case['HW']
    plan = ops.distill_plan(N, C, HW)
    d = D.make_data('normal', case)
    fb, ld, off = place(d['f'], case)
    tb, _, _ = place(d['t'], case)
    dfb = torch.full_like(fb, D.SENTINEL)
    ws = torch.full((plan['ws_bytes'],), WS_FILL, dtype=torch.uint8, device=DEV)
    out2 = torch.full((2,), -7.0, device=DEV)
    torch.cuda.synchronize()
    f, t, o, w, df, st = fb.data_ptr(), tb.data_ptr(), out2.data_ptr(), ws.data_ptr(), dfb.data_ptr(), ops.stream()
    lib.gcc_launch_count(1)

    def fwd(ldf=ld, foff=off, ldt=ld, toff=off, Cc=C, n=N, hw=HW, wsb=ws.numel(), fp=f, op=o, wp=w):
        return lib.gcc_distill_fwd(fp, ldf, foff, t, ldt, toff, n, Cc, hw, 0, op, wp, wsb, st)

    def bwd(ldf=ld, foff=off, lddf=ld, dfoff=off, Cc=C, wsb=ws.numel(), dp=df):
        return lib.gcc_distill_bwd(f, ldf, foff, t, ld, off, N, Cc, HW, 0, D.WG, D.WC, dp, lddf, dfoff, w, wsb, st)
    assert fwd(Cc=C + 4) == BAD_ARG and bwd(Cc=C + 4) == BAD_ARG and fwd(Cc=0) == BAD_ARG
    assert fwd(ldf=ld + 4) == BAD_ARG and fwd(foff=off + 4) == BAD_ARG and fwd(ldt=ld + 2) == BAD_ARG and fwd(toff=off + 1) == BAD_ARG
    assert bwd(ldf=ld + 4) == BAD_ARG and bwd(foff=4) == BAD_ARG and bwd(lddf=ld + 4) == BAD_ARG and bwd(dfoff=off + 4) == BAD_ARG
    assert fwd(n=0) == BAD_ARG and fwd(hw=0) == BAD_ARG and fwd(fp=None) == BAD_ARG and fwd(op=None) == BAD_ARG and fwd(wp=None) == BAD_ARG
    assert bwd(dp=None) == BAD_ARG
    assert fwd(wsb=ws.numel() - 1) == ERR_WORKSPACE and bwd(wsb=ws.numel() - 1) == ERR_WORKSPACE
    assert fwd(wsb=0) == ERR_WORKSPACE
    assert int(lib.gcc_launch_count(1)) == 0, 'a refusal came after a launch'
    torch.cuda.synchronize()
    assert bool((out2.cpu() == -7.0).all()), 'out2 written by a refused call'
    assert bool((ws.cpu() == WS_FILL).all()), 'workspace written by a refused call'
    assert bool((dfb.float().cpu() == D.SENTINEL).all()), 'df written by a refused call'
    assert ops.distill_workspace_bytes(N, C + 4, HW) == 0 and ops.distill_plan(N, C + 4, HW) == BAD_ARG
