"""The bf16 inference convolutions gcc_conv_fprop_eval and gcc_conv_eval_ex -- igemm_epilogue with EPI == 1, igemm_epilogue_ex, the
ring-walk's EV branch (conv_ring3.hip) and the two fold kernels splitk_epilogue_kernel<true> and splitk_eval_ex_kernel -- checked
three ways (tests/_conv_exact.py has the data, the float64 references, the derivation of bound_eval and the case table;
tests/test_conv_bounds_cpu.py examines the checks themselves without a GPU):

1. EXACT on integer data: scale in +-0.5 / +-1 / +-2, integer shift and residual, slope 0.25 or -0.5 -- every intermediate is a
   multiple of 2^-3 below 2^20, so the fp32 value in front of the store is exact in any order, fused or not, and the bf16 output
   is one round-to-nearest-even of it.  A residual added before the activation, a shift added after the rounding, a second
   rounding, act2 taken from act(z), an ignored slope, a fold that skips the scale or a slice, a pad lane that gets the shift:
   each changes bits.  Run twice: the same bits.  A split call and the same call without a workspace: the same bits.
2. PER ELEMENT on seeded normal data against float64, with the derived bound of _conv_exact.bound_eval.
3. LAYOUT: every activation at lane 8 of a buffer 16 lanes wider filled with a sentinel -- the pad lanes Co .. ceil8(Co) come
   out exactly zero (they hold the sentinel before the launch), nothing outside the window changes, the residual's pad lanes
   hold non-zeros that must not reach the output -- and the same bits as on buffers of their own.

Every test asserts which route ran (gcc_conv_eval_route / gcc_conv_eval_ex_route, the workspace size and the K slices it implies,
gcc_conv_tile, gcc_launch_count) before it compares a number, and prints it with its RATIO line.  A case that is not on its
intended route fails; nothing here skips."""
import ctypes as C
import functools

import pytest
import torch

from tests import _conv_exact as X
from tests._perelem import BF16, report, within

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 7.0               # what lies around a channel window and in an output before the launch
PAD_JUNK = 5.0               # what the residual's pad lanes hold
IDS = [c['name'] for c in X.EVAL_CASES]


def _ops():
    from gcc_amd import ops
    return ops


def _lib():
    from gcc_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    """data and float64 convolution of a case: computed once, shared by the three tests, read only"""
    case = X.EVAL_BY_NAME[name]
    d = X.make_eval_data(kind, case['g'], X.eval_seed(case) + (2 if kind == 'normal' else 0))
    return d, X.eval_conv(d, case['g'])


def _buffer(shape, windows, fill=SENTINEL, pad_fill=None):
    """an NHWC bf16 buffer filled with `fill` and the [N, Cc, H, W] views of its channel windows [(lane, Cc), ...]; pad_fill: what
    the windows' pad lanes hold (None: `fill`).  The buffer is as wide as the last window's end plus 8 lanes."""
    N, H, W = shape
    ld = max(off + X.ceil8(Cc) for off, Cc in windows) + (8 if windows[0][0] else 0)
    base = torch.full((N, H, W, ld), fill, dtype=torch.bfloat16, device=DEV)
    views = []
    for off, Cc in windows:
        if pad_fill is not None:
            base[..., off + Cc:off + X.ceil8(Cc)] = pad_fill
        views.append(base.permute(0, 3, 1, 2)[:, off:off + Cc])
    return base, views


def _check_layout(base, windows, what):
    """pad lanes exactly zero, every lane outside the windows untouched"""
    keep = torch.ones(base.shape[-1], dtype=torch.bool)
    for off, Cc in windows:
        c8 = X.ceil8(Cc)
        keep[off:off + c8] = False
        if c8 > Cc:
            assert float(base[..., off + Cc:off + c8].float().abs().max()) == 0.0, what + ': the pad lanes are not zero'
    outside = base[..., keep.to(DEV)]
    assert outside.numel() == 0 or bool((outside.float() == SENTINEL).all()), what + ': lanes outside the window changed'


def _pack(w64, transposed):
    """the bf16 packing the call reads: W of a forward call, Wt of a transposed one (its master is the ConvTranspose2d weight)"""
    packed = _ops().pack_weights(w64.float().to(DEV).contiguous(memory_format=torch.channels_last))
    return packed[1] if transposed else packed[0]


class _Device:
    """the operands of one case on the device: x (in a window or not), the packed weights, scale, shift, the residual, the slopes
    and a workspace filled with NaN bit patterns (a fold that reads a tile no launch wrote shows)"""

    def __init__(self, case, d, kind, win=True):
        self.case, self.kind, self.win = case, kind, win
        N, H, W, Ci, Co, kh, kw, s, p, tr = case['g']
        self.lane = 8 if win else 0
        self.xbase, (self.x,) = _buffer((N, H, W), [(self.lane, Ci)], pad_fill=0.0)
        self.x.copy_(d['x'].bfloat16().to(DEV))
        self.w = _pack(d['w'], tr)
        self.scale, self.shift = d['scale'].float().to(DEV), d['shift'].float().to(DEV)
        Ho, Wo = X.eval_out_hw(case['g'])
        self.out_shape = (N, Ho, Wo)
        self.rbase, (self.res,) = _buffer(self.out_shape, [(self.lane, Co)], pad_fill=PAD_JUNK)
        self.res.copy_(d['residual'].bfloat16().to(DEV))
        self.slopes = {i: torch.tensor([X.variant_slope(dict(slope_i=i), kind)], device=DEV) for i in (0, 1)}
        self.ws = None

    def workspace(self, nbytes):
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = torch.full((max(nbytes, 256),), 0xFF, dtype=torch.uint8, device=DEV)
        return self.ws


def _call(dev, d, v, y, y2, wsp, ws_bytes):
    """the library call of one variant; returns the launches it made (gcc_launch_count)"""
    ops, lib_mod = _ops(), _lib()
    lib = ops.lib()
    case = dev.case
    sc = dev.scale.data_ptr() if v['scale'] else None
    sh = dev.shift.data_ptr() if v['shift'] else None
    wp = wsp.data_ptr() if wsp is not None else None
    lib.gcc_launch_count(1)
    if case['entry'] == 'eval':
        res = v['residual']
        ep = lib_mod.eval_epilogue_t(sc, sh, dev.slopes[v['slope_i']].data_ptr() if v['act'] == X.EV_PRELU else None,
                                     dev.res.data_ptr() if res else None, dev.res.stride(3) if res else 0, 0, v['act'], 0, wp, ws_bytes)
        ops.check(lib.gcc_conv_fprop_eval(C.byref(d), dev.x.data_ptr(), dev.w.data_ptr(), y.data_ptr(), C.byref(ep), ops.stream()),
                  'gcc_conv_fprop_eval')
    else:
        ep = lib_mod.eval_ex_epilogue_t(sc, sh, y2.data_ptr() if y2 is not None else None, y2.stride(3) if y2 is not None else 0, 0, v['act'],
                                        v['act2'] if y2 is not None else 0, X.variant_slope(v, dev.kind), 0, wp, ws_bytes)
        ops.check(lib.gcc_conv_eval_ex(C.byref(d), int(case['g'][9]), dev.x.data_ptr(), dev.w.data_ptr(), y.data_ptr(), C.byref(ep),
                                       ops.stream()), 'gcc_conv_eval_ex')
    launches = int(lib.gcc_launch_count(1))
    torch.cuda.synchronize()
    return launches


def _launch(dev, v, ws):
    """one call of the case's entry with variant v.  Returns dict(y, y2 (bf16 [N,Co,Ho,Wo] on the CPU), raw (the device buffers,
    whole), r (eval_routing of the call's own descriptor), launches)"""
    ops, lib_mod = _ops(), _lib()
    case = dev.case
    N, H, W, Ci, Co, kh, kw, s, p, tr = case['g']
    Ho, Wo = X.eval_out_hw(case['g'])
    c8, lane = X.ceil8(Co), dev.lane
    what = '%s [%s]' % (case['name'], X.variant_id(v))
    two = case['entry'] == 'ex' and v['act2'] is not None
    if two and v['y2'] == 'same':
        # y at `lane`, y2 behind it in the same buffer, 8 untouched lanes between and around them
        wins = [(lane, Co), (lane + c8 + 8, Co)]
        base, (y, y2) = _buffer(dev.out_shape, wins)
        bufs = [(base, wins)]
    else:
        base, (y,) = _buffer(dev.out_shape, [(lane, Co)])
        bufs = [(base, [(lane, Co)])]
        y2 = None
        if two:                                   # a buffer of its own with another pixel stride
            b2, (y2,) = _buffer(dev.out_shape, [(lane + 8, Co)])
            bufs.append((b2, [(lane + 8, Co)]))
            assert y2.stride(3) != y.stride(3)
    ops.set_plan()
    if tr:
        d = ops.conv_desc(N, Ho, Wo, Co, Ci, kh, s, p, y.stride(3), dev.x.stride(3))
    else:
        d = ops.conv_desc(N, H, W, Ci, Co, kh, s, p, dev.x.stride(3), y.stride(3))
    d.KW = kw                                     # a rectangular kernel goes through the C struct, as ops.conv_eval_rect sets it
    r = X.eval_routing(lib_mod, case, d=d, ws=ws)
    wsp = dev.workspace(r['ws']) if r['ws'] else None
    launches = _call(dev, d, v, y, y2 if two else None, wsp, r['ws'])
    if ws == case['ws']:
        X.check_eval_expect(case, r, launches)
    else:
        _assert_unsplit(case, r, launches)
    if tr:
        # on integer data a phase left at the sentinel fails the equality anyway; this names it
        for py in range(s):
            for px in range(s):
                assert not bool((y[:, :, py::s, px::s].float() == SENTINEL).all()), '%s: output phase (%d, %d) of %d was not written' % (what, py, px, s * s)
    for b, wins in bufs:
        _check_layout(b, wins, what)
    return dict(y=y.cpu(), y2=y2.cpu() if two else None, raw=[b for b, _ in bufs], r=r, launches=launches, what=what)


def _assert_unsplit(case, r, launches):
    assert r['route'] in (0, 4) and r['S'] == 1 and launches == 1, '%s without a workspace: route %d, %d slices, %d launches' % (
        case['name'], r['route'], r['S'], launches)


def _modes(case, r_need):
    """the workspace modes a case runs in: its own, and -- where the call can split -- also without a workspace"""
    return [case['ws']] + ([False] if case['ws'] and r_need else [])


def _need(case):
    with X.forced_options(_lib(), case['opts']):
        return X.eval_routing(_lib(), case)['need']


def _print_route(case, run):
    r = run['r']
    print('ROUTE %s route %d tile %d K-slices %d launches %d workspace %d' % (case['name'], r['route'], r['tile'], r['S'], run['launches'], r['ws']))


def _tanh_on_integers(got, ref, what):
    """tanh of an integer is no fp32 number: the device tanhf's documented error and the one rounding"""
    return within(got, ref, X.TANH_ERR + BF16 * (ref.abs() + X.TANH_ERR), what)


def _assert_bits(got, ref, what):
    want = X.expected_bits(ref)
    bad = got != want
    assert not bool(bad.any()), '%s: %d of %d elements differ from the exact result, first at %s' % (
        what, int(bad.sum()), bad.numel(), tuple(int(i) for i in bad.nonzero()[0]))


@pytest.mark.parametrize('name', IDS)
def test_eval_exact_on_integers(name):
    """every route and every epilogue variant gives exact.float().bfloat16() bit for bit, twice; a split call and the same call
    with workspace = NULL (route 0) agree bit for bit.  tanh outputs are held to the device tanhf's documented error (the
    gcc_conv_fprop_eval tanh variants run per element only)."""
    case = X.EVAL_BY_NAME[name]
    d, conv = _reference(name, 'int')
    X.assert_eval_exact_condition(d, conv, name, residual=case['entry'] == 'eval')
    X.assert_eval_data_conditions(X.eval_z(d, conv)[0], name)
    variants = [v for v in case['variants'] if not (case['entry'] == 'eval' and v['act'] == X.EV_TANH)]
    assert variants
    with X.forced_options(_lib(), case['opts']):
        dev = _Device(case, d, 'int')
        modes = _modes(case, _need(case))
        tanh, compared = 0.0, 0
        for i, v in enumerate(variants):
            ref = X.variant_reference(case, d, v, 'int', conv)
            runs = []
            for ws in modes:
                a = _launch(dev, v, ws)
                if i == 0:
                    _print_route(case, a)
                b = _launch(dev, v, ws)
                assert all(torch.equal(p, q) for p, q in zip(a['raw'], b['raw'])), a['what'] + ': same bits run after run'
                runs.append(a)
            a = runs[0]
            for got, r64, act in ((a['y'], ref['y'], v['act']), (a['y2'], ref['y2'], v.get('act2'))):
                if got is None:
                    continue
                if act == X.EV_TANH:
                    tanh = max(tanh, _tanh_on_integers(got, r64, a['what']))
                else:
                    _assert_bits(got, r64, a['what'])
                    compared += got.numel()
            if len(runs) > 1:
                assert runs[0]['r']['route'] == 5 and runs[1]['r']['route'] == 0
                assert all(torch.equal(p, q) for p, q in zip(runs[0]['raw'], runs[1]['raw'])), a['what'] + ': split against un-split'
    report('eval-exact', (name,), variants=len(variants), modes=len(modes), elements=compared, mismatched=0, tanh=tanh)


@pytest.mark.parametrize('name', IDS)
def test_eval_within_the_derived_bound(name):
    """seeded normal data against float64, per element: _conv_exact.bound_eval with K products and the S slices the route folds"""
    case = X.EVAL_BY_NAME[name]
    g = case['g']
    d, conv = _reference(name, 'normal')
    K = X.eval_k(g)
    worst = {}
    with X.forced_options(_lib(), case['opts']):
        dev = _Device(case, d, 'normal')
        for ws in _modes(case, _need(case)):
            w = 0.0
            for i, v in enumerate(case['variants']):
                ref = X.variant_reference(case, d, v, 'normal', conv)
                a = _launch(dev, v, ws)
                if i == 0:
                    _print_route(case, a)
                S = a['r']['S']
                w = max(w, within(a['y'], ref['y'], X.bound_eval(ref['y'], ref['mag'], K, S, v['act'], ref['res']), a['what']))
                if a['y2'] is not None:
                    w = max(w, within(a['y2'], ref['y2'], X.bound_eval(ref['y2'], ref['mag'], K, S, v['act2']), a['what'] + ' y2'))
            worst['split' if a['r']['route'] == 5 else 'route%d' % a['r']['route']] = w
            report('eval', (name, 'route%d' % a['r']['route']), K=K, S=S, worst=w)
    assert all(w <= 1.0 for w in worst.values()), worst


@pytest.mark.parametrize('name', IDS)
def test_eval_layout(name):
    """the windowed call (lane 8 of buffers 16 lanes wider; _launch checks the pad lanes, the lanes outside and the transposed
    phases) against the same call on buffers of their own: the same bits, and the expected ones; the residual's pad lanes hold
    non-zeros in both"""
    case = X.EVAL_BY_NAME[name]
    d, conv = _reference(name, 'int')
    X.assert_eval_exact_condition(d, conv, name, residual=case['entry'] == 'eval')
    exact = [v for v in case['variants'] if v['act'] != X.EV_TANH and v.get('act2') != X.EV_TANH]
    # the fullest variant: a residual and both coefficients where the case has them, a second output
    v = max(exact, key=lambda v: (bool(v.get('residual')), v.get('act2') is not None, v['scale'] + v['shift'], v['slope_i']))
    ref = X.variant_reference(case, d, v, 'int', conv)
    with X.forced_options(_lib(), case['opts']):
        devs = [_Device(case, d, 'int', win=win) for win in (True, False)]
        runs = [_launch(dev, v, case['ws']) for dev in devs]
    _print_route(case, runs[0])
    Co = case['g'][4]
    if v.get('residual') and X.ceil8(Co) > Co:
        for dev in devs:           # the residual the call read did hold non-zeros in its pad lanes (and still does)
            assert bool((dev.rbase[..., dev.lane + Co:dev.lane + X.ceil8(Co)].float() == PAD_JUNK).all())
    for a in runs:
        _assert_bits(a['y'], ref['y'], a['what'])
        if a['y2'] is not None:
            _assert_bits(a['y2'], ref['y2'], a['what'] + ' y2')
    assert torch.equal(runs[0]['y'], runs[1]['y'])
    report('eval-layout', (name,), elements=runs[0]['y'].numel(), mismatched=0)
