"""The bf16 training convolutions -- igemm_kernel on every tile family, split K and the pair combine, the thin-input, head,
thin-output (conv_thinout.hip), ring-walk (conv_ring3.hip) and LDS-neighbourhood (conv_halo.hip) routes, and the weight gradients
of conv_wgrad.hip -- checked three ways (tests/_conv_exact.py has the data, the float64 references and the derivations;
tests/test_conv_bounds_cpu.py examines the checks themselves without a GPU):

1. EXACT on integer data: every partial sum is an integer below 2^24, so any summation order gives the same fp32 value and the
   bf16 output is one round-to-nearest-even of it.  A lost or doubled k-step or slice, a swapped index, a truncation, a second
   rounding or a bias added after the rounding changes bits.  Run twice: the same bits.
2. PER ELEMENT on seeded normal data against float64, with the derived bound of _conv_exact.bound_out / bound_wgrad.
3. STATISTICS on ternary data: stats.sum(0) equals the float64 sums exactly.

Every test asserts which route ran (gcc_conv_route, gcc_conv_tile, gcc_conv_halo_mode, gcc_launch_count, gcc_conv_stat_tiles,
the workspace size for the split counts) before it compares a number, and prints it with its RATIO line.  A case that is not
on its intended route fails; nothing here skips."""
import pytest
import torch

from tests import _conv_exact as X
from tests._perelem import ACT_NONE, ACT_TANH, BF16, report, within

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 7.0               # what lies around a channel window and in an output before the launch: nothing outside may change


def _ops():
    from gcc_amd import ops
    return ops


def _lib():
    from gcc_amd import _lib
    return _lib


class _forced:
    """the case's plan (ops.set_plan) and options (gcc_set_option) for the block; both restored afterwards"""

    def __init__(self, case, **opts):
        self.plan, self.opts = case['plan'], dict(case['opts'], **opts)

    def __enter__(self):
        _ops().set_plan(**self.plan)
        self.cm = X.forced_options(_lib(), self.opts)
        self.cm.__enter__()

    def __exit__(self, *exc):
        try:
            self.cm.__exit__(*exc)
        finally:
            _ops().set_plan()
        return False


def _act_buffer(shape, Cc, win, fill):
    """an NHWC bf16 buffer and the [N, Cc, H, W] view of its channel window.  win: the window sits at lane 8 of a buffer 16 lanes
    wider.  Real lanes and everything outside the window hold `fill`; the window's pad lanes (Cc .. ceil8(Cc)) hold zeros, as
    every activation buffer of the package does."""
    N, H, W = shape
    c8 = X.ceil8(Cc)
    off, ld = (8, c8 + 16) if win else (0, c8)
    base = torch.full((N, H, W, ld), fill, dtype=torch.bfloat16, device=DEV)
    base[..., off + Cc:off + c8] = 0
    return base, base.permute(0, 3, 1, 2)[:, off:off + Cc], off


def _put(t64, win):
    N, Cc, H, W = t64.shape
    base, view, _ = _act_buffer((N, H, W), Cc, win, SENTINEL)
    view.copy_(t64.bfloat16().to(DEV))
    return view


def _check_window(base, off, Cc, what):
    """pad lanes exactly zero, every lane outside the window untouched"""
    c8 = X.ceil8(Cc)
    assert float(base[..., off + Cc:off + c8].float().abs().max()) == 0.0 if c8 > Cc else True, what + ': pad lanes'
    outside = torch.cat([base[..., :off], base[..., off + c8:]], -1)
    assert outside.numel() == 0 or bool((outside.float() == SENTINEL).all()), what + ': lanes outside the window changed'


def _weights(d):
    ops = _ops()
    m = d['w'].float().to(DEV).contiguous(memory_format=torch.channels_last)
    return ops.pack_weights(m)


def _launch(case, d, packed, with_stats=False, bias=None, act=None, y2_mode=0, gate=None):
    """one forward / data-gradient call of the case under the CURRENT plan and options.  Returns dict(out [N,C,H,W] bf16 on the
    CPU, raw (the whole device buffer), launches, routing, stats, y2)"""
    ops, lib_mod = _ops(), _lib()
    op, g, win = case['op'], case['g'], case['win']
    N, H, W, Ci, Co, k, s, p = g
    Ho, Wo = X.out_hw(g)
    bias = case['bias'] if bias is None else bias
    act = case['act'] if act is None else act
    dg = op == 'D'
    src = _put(d['dy'] if dg else d['x'], win)
    Cd, shape = (Ci, (N, H, W)) if dg else (Co, (N, Ho, Wo))
    base, out, off = _act_buffer(shape, Cd, win, SENTINEL)
    b = (d['bias_x'] if dg else d['bias_y']).float().to(DEV) if bias else None
    ldx, ldy = (out.stride(3), src.stride(3)) if dg else (src.stride(3), out.stride(3))
    desc = ops.conv_desc(N, H, W, Ci, Co, k, s, p, ldx, ldy)
    ws_slot = 'splitk' if case['ws'] else None
    stats_probe = torch.empty(1, device=DEV) if with_stats else None
    ep = ops._epilogue(b, act, X.SLOPE, stats_probe, desc, int(dg), src.device, None, ws_slot)
    r = X.routing(lib_mod, case, ep=ep, with_stats=with_stats, d=desc)
    y2 = None
    kw = dict(out=out, bias=b, act=act, slope=X.SLOPE, want_stats=with_stats, ws_slot=ws_slot)
    ops.lib().gcc_launch_count(1)
    if dg:
        res = ops.conv_dgrad(src, packed[1], Ci, H, W, k, s, p, **kw)
    else:
        if y2_mode:
            _, y2, _ = _act_buffer(shape, Cd, False, SENTINEL)
            kw.update(y2=y2, y2_mode=y2_mode, y2_gate=gate)
        res = ops.conv_fprop(src, packed[0], Co, k, s, p, **kw)
    launches = int(ops.lib().gcc_launch_count(1))
    torch.cuda.synchronize()
    _check_window(base, off, Cd, case['name'])
    return dict(out=out.cpu(), raw=base.clone(), launches=launches, r=r, stats=res[1] if with_stats else None,
                y2=y2.cpu() if y2 is not None else None)


def _assert_route(case, run, with_stats=False):
    r = run['r']
    if with_stats:
        # route, tile, halo mode and split as intended, the rows and -- by the launch count -- the kernel that forms the rows
        X.check_stats_expect(case, r, run['launches'])
    else:
        X.check_expect(case, r)
        want = case['expect'].get('launches', None if r['route'] else (2 if r['S'] > 1 and r['tile'] // 1000 == 128 else 1))
        assert want is None or run['launches'] == want, '%s: %d launches, intended %d' % (case['name'], run['launches'], want)
    print('ROUTE %s route %d tile %d halo %d K-slices %d launches %d stat rows %d' % (case['name'], r['route'], r['tile'], r['halo'], r['S'],
                                                                                    run['launches'], r['stat_tiles']))


IDS = [c['name'] for c in X.FD_CASES]


@pytest.mark.parametrize('case', X.FD_CASES, ids=IDS)
def test_forward_and_data_gradient_exact_on_integers(case):
    """every route gives exact.float().bfloat16() bit for bit, twice; nothing outside the output's channel window changes and its
    pad lanes STAY zero (they hold zeros before the launch, as every activation buffer of the package does: the check shows that
    no route writes anything else there, not that it writes them).  A halo case equals the igemm_kernel run of the same call (IGEMM_HALO = 0), and the HALO_XCD_COLS tile
    order the plain one -- consequences of exactness, asserted on the raw buffers.  tanh of an integer is no fp32 number: that
    case is held to the device tanhf's documented error and the one rounding."""
    op, g = case['op'], case['g']
    d = X.make_data('int', g, X.case_seed(case))
    ref, _, mag = X.reference(op, d, g, case['bias'], case['act'])
    X.assert_exact_condition(mag, case['name'])
    with _forced(case):
        packed = _weights(d)
        a = _launch(case, d, packed)
        _assert_route(case, a)
        b = _launch(case, d, packed)
    assert torch.equal(a['raw'], b['raw']), 'same bits run after run'
    if case['act'] == ACT_TANH:
        within(a['out'], ref, X.TANH_ERR + BF16 * (ref.abs() + X.TANH_ERR), case['name'])
    else:
        want = X.expected_bits(ref)
        bad = a['out'] != want
        assert not bool(bad.any()), '%s: %d of %d elements differ from the exact result, first at %s' % (
            case['name'], int(bad.sum()), bad.numel(), tuple(int(v) for v in bad.nonzero()[0]))
    if case['expect']['halo']:
        alt = dict(HALO_XCD_COLS=0) if case['opts'].get('HALO_XCD_COLS') else dict(IGEMM_HALO=0)
        with _forced(case, **alt):
            o = _launch(case, d, packed)
        assert (o['r']['halo'] == 0) == ('IGEMM_HALO' in alt), o['r']
        assert torch.equal(o['raw'], a['raw']), 'the halo route against %s' % (alt,)


@pytest.mark.parametrize('case', X.FD_CASES, ids=IDS)
def test_forward_and_data_gradient_within_the_derived_bound(case):
    """seeded normal data against float64, per element: _conv_exact.bound_out with K products and the S slices the route folds"""
    op, g = case['op'], case['g']
    d = X.make_data('normal', g, X.case_seed(case) + 2)
    ref, _, mag = X.reference(op, d, g, case['bias'], case['act'])
    with _forced(case):
        a = _launch(case, d, _weights(d))
        _assert_route(case, a)
    K, S = X.k_products(g, op), a['r']['S']
    worst = within(a['out'], ref, X.bound_out(ref, mag, K, S, case['act']), case['name'])
    report('conv', (case['name'],), K=K, S=S, worst=worst)


STAT_CASES = [c for c in X.FD_CASES if c['stats']]


@pytest.mark.parametrize('case', STAT_CASES, ids=[c['name'] for c in STAT_CASES])
def test_statistic_rows_sum_exactly(case):
    """BatchNorm partial rows on ternary data.  Every route's epilogue sums the ROUNDED outputs: igemm_kernel's tile epilogue
    (igemm_common.hpp) and the halo kernel re-read the bf16 tile they staged for the store, splitk_fold_stats_kernel unpacks the
    packed bf16 it is about to write, channel_stats_kernel (the fallback behind a split launch the fold kernel does not take: more
    than 2048 channels) reads the stored tensor, the ring-walk kernel sums its staged bf16 row.  On this data a rounded output
    equals the output (asserted on the reference), so the float64 sums of y and y^2 are the one right answer and fp32 sums of
    them are exact in any order: stats.sum(0) must equal them.  Rows the call promised (gcc_conv_stat_tiles) but the route does
    not fill are exact zeros: the un-split fallback of a layer whose plan is split names how many it fills.  Which kernel formed the
    rows is asserted from the launch count (_conv_exact.STAT_LAUNCHES) and, for the fold kernel, from its row count."""
    op, g = case['op'], case['g']
    d = X.make_data('tiny', g, X.case_seed(case) + 1)
    ref = X.reference(op, d, g)[0]
    want, same = X.stats_reference(ref)
    assert same
    with _forced(case):
        packed = _weights(d)
        a = _launch(case, d, packed, with_stats=True, bias=False, act=ACT_NONE)
        _assert_route(case, a, with_stats=True)
        b = _launch(case, d, packed, with_stats=True, bias=False, act=ACT_NONE)
    rows = a['stats'].double().cpu()
    assert rows.shape[0] == a['r']['stat_tiles'] and bool(torch.isfinite(rows).all())
    assert torch.equal(a['out'], X.expected_bits(ref)), 'the output of the statistics launch'
    assert torch.equal(rows.sum(0), want), 'statistics: largest difference %g' % float((rows.sum(0) - want).abs().max())
    assert torch.equal(a['stats'], b['stats']) and torch.equal(a['raw'], b['raw']), 'same bits run after run'
    z = case['expect'].get('zero_rows_from')
    if z is not None:
        assert rows.shape[0] > z and float(rows[z:].abs().max()) == 0.0 and float(rows[:z].abs().max()) > 0.0


@pytest.mark.parametrize('case', STAT_CASES, ids=[c['name'] for c in STAT_CASES])
def test_statistic_sum_row_is_of_the_rounded_outputs(case):
    """the convention itself, on 'int' data, where outputs of thousands do not survive the rounding to bf16: the rounded outputs
    are still integers, their sums exact while sum |y_r| < 2^24 (the widest x range of [-3, 3], [-1, 1] that meets it), and differ
    from the sums of the fp32 accumulators -- the first statistics row equals the former on every route.  (The squares do not
    stay below 2^24 here: the second row is checked on the ternary data above.)"""
    op, g = case['op'], case['g']
    for xmax in (3, 1):
        d = X.make_data('int', g, X.case_seed(case), xmax=xmax)
        ref = X.reference(op, d, g)[0]
        want, ok, differs = X.rounded_sum_reference(ref)
        if ok:
            break
    assert ok and differs, 'the data must keep the sums exact and tell the conventions apart'
    with _forced(case):
        a = _launch(case, d, _weights(d), with_stats=True, bias=False, act=ACT_NONE)
        _assert_route(case, a, with_stats=True)
    got = a['stats'].double().cpu().sum(0)[0]
    assert torch.equal(a['out'], X.expected_bits(ref))
    assert torch.equal(got, want), 'sum row: largest difference %g (from the unrounded sums: %g)' % (
        float((got - want).abs().max()), float((got - ref.sum((0, 2, 3))).abs().max()))


@pytest.mark.parametrize('mode', [1, 2])
def test_thin_forward_second_output_exact(mode):
    """gcc_epilogue_t.y2 on the thin-input route, written by the same launch: relu(out) (mode 1) and out * gate[c] (mode 2, gates
    0, 1/2, 1: powers of two, the product of a bf16 value with them is exact) are exact too"""
    ops = _ops()
    case = next(c for c in X.FD_CASES if c['name'] == 'thin-6-72-F')
    g = case['g']
    d = X.make_data('int', g, X.case_seed(case))
    ref, pre, mag = X.reference('F', d, g, True, case['act'])
    X.assert_exact_condition(mag, case['name'])
    gate = (torch.arange(g[4]) % 3).double() * 0.5
    with _forced(case):
        a = _launch(case, d, _weights(d), y2_mode=mode, gate=gate.float().to(DEV) if mode == 2 else None)
        _assert_route(case, a)                   # route 1, ONE launch: the second output came from the conv launch itself
    assert torch.equal(a['out'], X.expected_bits(ref))
    want2 = torch.relu(pre) if mode == 1 else X.expected_bits(ref).double() * gate[None, :, None, None]
    assert torch.equal(a['y2'], X.expected_bits(want2))


# ---- weight gradients --------------------------------------------------------------------------------------------------------
def _wgrad(case, d, fill=5.0):
    """fresh into a stale buffer, then accumulating, then fresh again; the launches of the first call"""
    ops = _ops()
    N, H, W, Ci, Co, k, s, p = case['g']
    x, dy = _put(d['x'], case['win']), _put(d['dy'], case['win'])      # win: both operands inside wider, sentinel-filled buffers
    dw = torch.full((Co, Ci, k, k), fill, device=DEV).contiguous(memory_format=torch.channels_last)
    ops.lib().gcc_launch_count(1)
    ops.conv_wgrad(x, dy, dw, k, s, p, accumulate=False)
    launches = int(ops.lib().gcc_launch_count(1))
    fresh = dw.clone()
    ops.conv_wgrad(x, dy, dw, k, s, p, accumulate=True)
    twice = dw.clone()
    again = torch.full_like(dw, -fill)
    ops.conv_wgrad(x, dy, again, k, s, p, accumulate=False)
    torch.cuda.synchronize()
    return fresh.cpu(), twice.cpu(), again.cpu(), launches


def _assert_wgrad_route(case, launches):
    ws, splits = X.wgrad_splits(_lib(), case)
    e = case['expect']
    assert launches == e['launches'], '%s: %d launches, intended %d' % (case['name'], launches, e['launches'])
    assert e['splits'] is None or splits == e['splits'], '%s: %d pixel splits, intended %d' % (case['name'], splits, e['splits'])
    print('ROUTE %s launches %d pixel splits %s workspace %d' % (case['name'], launches, splits if e['splits'] is not None else '-', ws))


WIDS = [c['name'] for c in X.WGRAD_CASES]


@pytest.mark.parametrize('case', X.WGRAD_CASES, ids=WIDS)
def test_weight_gradient_exact_on_integers(case):
    """fp32 dW equals the exact integers on every form -- direct write, slabs + fold, 256 x 256 tiles, tap-stationary, the head's
    gather + 1 x 1 + row fold, the thin-output kernel + fold; a fresh call overwrites a stale fill, an accumulating one gives
    exactly twice the gradient; run twice, same bits"""
    g = case['g']
    d = X.make_data('int', g, X.case_seed(case))
    ref, mag = X.ref_wgrad(d, g)
    X.assert_exact_condition(2 * mag, case['name'])
    with _forced(case):
        fresh, twice, again, launches = _wgrad(case, d)
        _assert_wgrad_route(case, launches)
    assert torch.equal(fresh.double(), ref), '%d elements differ from the exact gradient' % int((fresh.double() != ref).sum())
    assert torch.equal(twice.double(), 2 * ref), 'accumulate'
    assert torch.equal(again, fresh), 'same bits run after run'


@pytest.mark.parametrize('case', X.WGRAD_CASES, ids=WIDS)
def test_weight_gradient_within_the_derived_bound(case):
    g = case['g']
    d = X.make_data('normal', g, X.case_seed(case) + 2)
    ref, mag = X.ref_wgrad(d, g)
    M, S = X.wgrad_counts(case)
    with _forced(case):
        fresh, twice, again, launches = _wgrad(case, d)
        _assert_wgrad_route(case, launches)
    w1 = within(fresh, ref, X.bound_wgrad(mag, M, S), case['name'])
    # accumulating: the second gradient's own error, the first one's, and one rounding of the sum with the old contents
    w2 = within(twice, 2 * ref, 2 * X.bound_wgrad(mag, M, S, old=fresh.double()), case['name'] + ' accumulated')
    assert torch.equal(again, fresh)
    report('wgrad', (case['name'],), M=M, S=S, fresh=w1, accumulated=w2)


def test_grouped_weight_gradient_exact_on_integers():
    """gcc_conv_wgrad_group_prepare / _run through ops.WgradGroup: three small layers of different kernel sizes in ONE launch + one
    fold (the first layer in two pixel slabs, the others written directly) give the exact integers -- hence the single launches' bits --, fresh over a stale fill and accumulating"""
    ops = _ops()
    entries, refs = [], []
    for i, g in enumerate(X.GROUP_LAYERS):
        N, H, W, Ci, Co, k, s, p = g
        d = X.make_data('int', g, 500 + i)
        ref, mag = X.ref_wgrad(d, g)
        X.assert_exact_condition(2 * mag, 'group layer %d' % i)
        refs.append(ref)
        dw = torch.full((Co, Ci, k, k), 5.0, device=DEV).contiguous(memory_format=torch.channels_last)
        entries.append((_put(d['x'], False), _put(d['dy'], False), dw, k, s, p, False))
    ops.set_plan()
    grp = ops.WgradGroup()
    assert grp.groupable(entries), 'the three layers must be groupable'
    ops.lib().gcc_launch_count(1)
    grp.run()
    launches = int(ops.lib().gcc_launch_count(1))
    assert launches == 2, launches
    print('ROUTE wgrad-group launches %d layers %d' % (launches, len(entries)))
    torch.cuda.synchronize()
    for (x, dy, dw, k, s, p, _), ref in zip(entries, refs):
        assert torch.equal(dw.double().cpu(), ref)
        single = torch.full_like(dw, 3.0)
        ops.conv_wgrad(x, dy, single, k, s, p, accumulate=False)
        assert torch.equal(single, dw), 'group against the single launch'
    acc = [(x, dy, dw, k, s, p, True) for (x, dy, dw, k, s, p, _) in entries]
    grp2 = ops.WgradGroup()
    assert grp2.groupable(acc)
    grp2.run()
    torch.cuda.synchronize()
    for (x, dy, dw, k, s, p, _), ref in zip(acc, refs):
        assert torch.equal(dw.double().cpu(), 2 * ref)
