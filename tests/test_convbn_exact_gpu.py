"""gcc_conv_bn_act on every route (conv_igemm.hip; norm_act.hip bn_fold_grid_kernel): exact data whose result is known to the bit
but for the last roundings, bf16 normals per element against float64 with the bounds derived in tests/_convbn.py, every operand at
lane 8 of a sentinel-filled buffer, dropout's zero pattern across the routes, single and NULL outputs, independence from what
earlier launches left in the stream's workspaces, and the declined calls.  Every test first asserts the plan the library reports
(gcc_conv_bn_act_plan) against the restatement, against the regime its case is named for (tests/_convbn.py CASES) and the
launch count; nothing here skips."""
import ctypes as C
import functools
import os

import pytest
import torch

from tests import _convbn as B
from tests import _conv_exact as X
from tests._perelem import ACT_LRELU, ACT_NONE, ACT_RELU, report
from tests.test_norm_kernels_gpu import SENT, Win

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
IDS = [c['name'] for c in B.CASES]
# the activation pair of a case, in rotation: the U-Net's two, and a pair whose second output cannot be had from the first
ACTS = ((ACT_LRELU, ACT_RELU), (ACT_RELU, ACT_LRELU), (ACT_RELU, ACT_RELU), (ACT_NONE, ACT_LRELU))


def _ops():
    from gcc_amd import ops
    return ops


def acts_of(case):
    return ACTS[IDS.index(case['name']) % len(ACTS)]


@functools.lru_cache(maxsize=2)
def _data(name, kind):
    case = B.BY_NAME[name]
    return B.make(case, kind, B.seeds(case)[0 if kind == 'exact' else 1])


def _device_plan_args():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    q = int(os.environ.get('GPU_MAX_HW_QUEUES', '0') or 0)
    return cus, (q if q > 0 else 4)


class Launch:
    """one gcc_conv_bn_act call: source, raw, y and y2 at lane 8 of sentinel-filled buffers with ld = ceil8(C) + 16 (the pad lanes of
    the source hold non-zeros); omit: names among y, y2, gamma, beta, mean, rstd, rm, rv handed over as NULL; y2_in_y: y2 is a
    second window of y's buffer; private: freshly zeroed workspaces of its own instead of the stream's shared ones"""

    def __init__(self, case, d, acts=None, omit=(), y2_in_y=False, y2_extra=8, private=False, count=None):
        from gcc_amd import _lib
        ops = _ops()
        self.case, self.d, self.omit = case, d, set(omit)
        self.lib = ops.lib()
        g, dg = case['g'], case['dgrad']
        N, H, W, Ci, Co, k, s, p = g
        src = d['dy'] if dg else d['x']
        self.P, self.Cc = d['raw64'].shape
        self.src = Win((1, src.shape[0] * src.shape[2] * src.shape[3], src.shape[1]), 8, 8, B.to_pc(src)[None], pad=1.5)
        self.raw = Win((1, self.P, self.Cc), 8, 8)
        C8 = self.raw.C8
        self.y = Win((1, self.P, self.Cc), 8 + (C8 + 8 if y2_in_y else 0), 8)
        self.y2 = None if y2_in_y else Win((1, self.P, self.Cc), y2_extra, 8)
        self.y2_off = 8 + C8 + 8 if y2_in_y else 8
        wm = d['w'].float().to(DEV).contiguous(memory_format=torch.channels_last)
        wp, wtp = ops.pack_weights(wm)
        self.w = wtp if dg else wp
        f = lambda t: t.float().contiguous().to(DEV)
        self.par = dict(gamma=f(d['gamma']), beta=f(d['beta']), rm=f(d['rm']), rv=f(d['rv']))
        self.out = {k_: torch.full((self.Cc + 8,), SENT, dtype=torch.float32, device=DEV) for k_ in ('mean', 'rstd', 'scale', 'shift')}
        xw, yw = (self.raw, self.src) if dg else (self.src, self.raw)
        self.conv = _lib.conv_t(N, H, W, Ci, Co, k, k, s, p, xw.ld, 8, yw.ld, 8, tuple([0] * len(_lib.PLAN_FIELDS)))
        self.ws_need = int(self.lib.gcc_conv_bn_act_workspace(C.byref(self.conv), int(dg)))
        if private:
            self.ws = torch.zeros(max(self.ws_need, 256), dtype=torch.uint8, device=DEV)
            self.tail = torch.zeros(ops.TAIL_WS_BYTES, dtype=torch.uint8, device=DEV) if case['tail_ws'] else None
        else:
            self.ws = ops.workspace(max(self.ws_need, 256), DEV, 'convbn')
            self.tail = ops.tail_workspace(DEV) if case['tail_ws'] else None
        ptr = lambda n, t: None if n in self.omit else t.data_ptr()
        self.count = float(self.P if count is None else count)
        self.bn = _lib.bn_t(ptr('gamma', self.par['gamma']), ptr('beta', self.par['beta']), B.EPS, B.MOMENTUM, self.count,
                            ptr('rm', self.par['rm']), ptr('rv', self.par['rv']), ptr('mean', self.out['mean']), ptr('rstd', self.out['rstd']),
                            ptr('scale', self.out['scale']), self.out['shift'].data_ptr(),
                            self.tail.data_ptr() if self.tail is not None else None, self.tail.numel() if self.tail is not None else 0, 1, 0)
        act, act2 = acts or acts_of(case)
        self.acts = dict(act=act, act2=act2)
        self.act = _lib.bnact_t(None, None, None, 0, act, B.SLOPE, act2, case['drop'], d['seed'], 1, 0, None)
        self.opts = dict(FUSE_BN=case['fuse'], INORM_GRID=case['inorm_grid'])
        self.inputs = [(t, t.clone()) for t in (self.src.base, self.w, self.par['gamma'], self.par['beta'])]

    def plan(self):
        from gcc_amd import _lib
        with X.forced_options(_lib, self.opts):
            return _ops().conv_bn_act_plan_of(self.conv, self.case['dgrad'], self.bn)

    def assert_plan(self, regime=True):
        """the library's plan is the restatement's for this device and (regime) the one the case is named for"""
        c = self.case
        pl = self.plan()
        cus, queues = _device_plan_args()
        want = B.plan(c['g'], c['dgrad'], c['fuse'], cus, queues, c['tail_ws'], c['inorm_grid'])
        assert isinstance(pl, dict) and all(pl.get(k) == v for k, v in want.items() if v is not None), (c['name'], pl, want, cus, queues)
        if regime:
            B.check_regime(c, pl)
        return pl

    def call(self, ws_bytes=None, ws_shift=0, ldy=None, y2off=None, both_null=False):
        from gcc_amd import _lib
        ops = _ops()
        yw = self.y
        y2b = self.y if self.y2 is None else self.y2
        yp = None if ('y' in self.omit or both_null) else yw.ptr
        y2p = None if ('y2' in self.omit or both_null) else y2b.ptr
        with X.forced_options(_lib, self.opts):
            return self.lib.gcc_conv_bn_act(C.byref(self.conv), int(self.case['dgrad']), self.src.ptr, self.w.data_ptr(), self.raw.ptr,
                                            C.byref(self.bn), C.byref(self.act), yp, yw.ld if ldy is None else ldy, 8, y2p, y2b.ld,
                                            self.y2_off if y2off is None else y2off, self.ws.data_ptr() + ws_shift,
                                            self.ws.numel() if ws_bytes is None else ws_bytes, ops.stream())

    def run(self, launches=None):
        """running statistics are reset first: every run starts from the same state"""
        self.par['rm'].copy_(self.d['rm'].float())
        self.par['rv'].copy_(self.d['rv'].float())
        self.lib.gcc_launch_count(1)
        rc = self.call()
        assert rc == 0, (self.case['name'], rc)
        n = self.lib.gcc_launch_count(0)
        if launches is not None:
            assert n == launches, '%s: %d launches, the plan says %d' % (self.case['name'], n, launches)
        torch.cuda.synchronize()
        return self.bits()

    def bits(self):
        bufs = [self.raw.base, self.y.base] + ([self.y2.base] if self.y2 is not None else [])
        return [b.view(torch.int16).clone() for b in bufs] + [v.view(torch.int32).clone() for v in self.out.values()] + \
               [self.par['rm'].view(torch.int32).clone(), self.par['rv'].view(torch.int32).clone()]

    def got(self):
        """what exact_faults / normal_check take: [P, C8] outputs with their pad lanes, [C] statistics (None where not written)"""
        C8 = self.raw.C8
        win = lambda b, off: b[0, 0, :, off:off + C8].double().cpu()
        o = dict(raw=win(self.raw.base, 8))
        o['y'] = None if 'y' in self.omit else win(self.y.base, 8)
        o['y2'] = None if 'y2' in self.omit else win((self.y if self.y2 is None else self.y2).base, self.y2_off)
        for k_ in ('mean', 'rstd', 'scale', 'shift'):
            o[k_] = None if k_ in self.omit else self.out[k_][:self.Cc].double().cpu()
        o['rm'] = None if 'rm' in self.omit else self.par['rm'].double().cpu()
        o['rv'] = None if 'rv' in self.omit else self.par['rv'].double().cpu()
        return o

    def check_layout(self, what):
        """nothing outside the windows changed, inputs included; omitted outputs untouched"""
        C8 = self.raw.C8
        self.raw.check(what + ' raw')
        yb = self.y.base[0, 0].float().cpu()
        wins = ([] if 'y' in self.omit else [8]) + ([self.y2_off] if self.y2 is None and 'y2' not in self.omit else [])
        mask = torch.zeros(yb.shape[1], dtype=torch.bool)
        for off in wins:
            mask[off:off + C8] = True
        assert bool((yb[:, ~mask] == SENT).all()), what + ': a lane outside the windows of y changed'
        if self.y2 is not None:
            if 'y2' in self.omit:
                assert bool((self.y2.base == SENT).all()), what + ': y2 written'
            else:
                self.y2.check(what + ' y2')
        for k_, t in self.out.items():
            assert bool((t[self.Cc:] == SENT).all()), what + ': ' + k_ + ' written past C'
            if k_ in self.omit:
                assert bool((t == SENT).all()), what + ': ' + k_ + ' written'
        for t, before in self.inputs:
            assert torch.equal(t.view(torch.int16), before.view(torch.int16)), what + ': an input changed'
        for k_ in ('rm', 'rv'):
            if k_ in self.omit:
                assert torch.equal(self.par[k_].cpu().double(), self.d[k_]), what + ': ' + k_ + ' changed'


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('name', IDS)
def test_exact_data(name):
    """the plan and the launch count first; then raw bit for bit, the statistics within their counted ulps, y and y2 the one (near a
    tie: either) value the exact reference allows, pad lanes zero, nothing else changed; twice on the same workspaces: the same bits"""
    lib = _ops().lib()
    assert lib.gcc_device_error(1) == 0
    case = B.BY_NAME[name]
    d = _data(name, 'exact')
    L = Launch(case, d)
    pl = L.assert_plan()
    ref = B.exact_ref(d, **L.acts)
    assert ref['ambiguous'] <= 0.01
    first = L.run(pl['launches'])
    L.check_layout('exact ' + name)
    bad = B.exact_faults(ref, L.got())
    print('EXACT %s plan=%r ambiguous=%.3g faults=%r' % (name, pl, ref['ambiguous'], bad))
    assert not any(bad.values()), '%s: elements outside what the exact reference allows: %r' % (name, bad)
    C_ = L.Cc
    big, dead, _ = B.special(C_)
    if C_ > 1:
        got = L.got()
        beta = d['beta'][dead:dead + 1].expand(L.P)
        keep = ref['keep'][:, dead] if ref['keep'] is not None else None
        for k_, a in (('y', L.acts['act']), ('y2', L.acts['act2'])):
            v = beta if keep is None else torch.where(keep, beta * 2, torch.zeros_like(beta))
            want = B.rb64(B.act_fn(v, a, B.SLOPE))
            assert bool((got[k_][:, dead] == want).all()), '%s: %s of the dead channel is not bf16(act(beta))' % (name, k_)
    assert _same(L.run(pl['launches']), first), name + ': a second call on the same workspaces gave other bits'
    assert lib.gcc_device_error(0) == 0


@pytest.mark.parametrize('name', IDS)
def test_per_element_against_float64(name):
    """bf16 normals (a channel of |mean| ~ 20 sigma, a dead channel): raw, statistics, coefficients and both outputs within the
    derived bounds per element"""
    lib = _ops().lib()
    assert lib.gcc_device_error(1) == 0
    case = B.BY_NAME[name]
    d = _data(name, 'normal')
    L = Launch(case, d)
    pl = L.assert_plan()
    L.run(pl['launches'])
    L.check_layout('normal ' + name)
    ratios = B.normal_check(d, pl, L.got(), what='normal ' + name, **L.acts)
    assert lib.gcc_device_error(0) == 0
    report('convbn_route%d' % pl['route'], (name,), **ratios)


# one geometry on the three routes: (case, the route its options lead to)
ROUTES_F = (('r2-tail6', 2), ('r1-nogrid', 1), (dict(B.BY_NAME['r2-tail6'], name='r0-tail6', fuse=2), 0))
ROUTES_D = (('r2-convT', 2), (dict(B.BY_NAME['r2-convT'], name='r1-convT', fuse=1), 1), (dict(B.BY_NAME['r2-convT'], name='r0-convT', fuse=2), 0))


@pytest.mark.parametrize('routes', [ROUTES_F, ROUTES_D], ids=['fprop', 'convT'])
def test_dropout_pattern_is_the_same_on_every_route(routes):
    """drop_p 0.5: routes 0, 1 and 2 zero the same elements for one seed and geometry -- the set rng_uniform(seed, pixel * C + channel)
    names, which is the set gcc_bnact_bwd regenerates"""
    ops = _ops()
    base = B.BY_NAME[routes[0][0]]
    d = B.make(base, 'exact', B.seeds(base)[0])
    patterns = []
    for c, route in routes:
        case = B.BY_NAME[c] if isinstance(c, str) else c
        assert case['g'] == base['g'] and case['drop'] == 0.5
        dd = dict(d, case=case)
        L = Launch(case, dd, acts=(ACT_NONE, ACT_LRELU))
        pl = L.plan()
        assert pl['route'] == route, (case['name'], pl)
        L.run(pl['launches'])
        ref = B.exact_ref(dd, act=ACT_NONE, act2=ACT_LRELU)
        bad = B.exact_faults(ref, L.got())
        assert not any(bad.values()), (case['name'], bad)
        patterns.append(L.got()['y'][:, :L.Cc] == 0)
        assert torch.equal(L.got()['y2'][:, :L.Cc] == 0, patterns[-1])
    keep = B.keep_mask(d['seed'], *d['raw64'].shape, 0.5)
    sure = ref['v'].abs() > 0                       # an element whose value is 0 is zero either way (the dead channel has beta != 0)
    for pat in patterns:
        assert torch.equal(pat & sure, ~keep & sure)
    assert 0.3 < float(keep.double().mean()) < 0.7
    # the backward's mask: a bare dropout backward of ones over the same [P, C]
    P, Cc = d['raw64'].shape
    gup, dx, x = Win((1, P, Cc), 8, 8, torch.ones(1, P, Cc)), Win((1, P, Cc), 8, 8), Win((1, P, Cc), 8, 8, torch.ones(1, P, Cc))
    ops.bnact_bwd(x.view, None, gup.view, dx.view, bn=None, act=ops.ACT_NONE, drop_p=0.5, seed=d['seed'])
    torch.cuda.synchronize()
    assert torch.equal(dx.get()[0] != 0, keep)


VARIANT_CASES = ('r2-tail6', 'r1-nogrid', 'r0-split-f2', 'r2-convT-n3')
VARIANTS = (dict(omit=('y2',)), dict(omit=('y',)), dict(y2_in_y=True), dict(y2_extra=24), dict(omit=('gamma', 'beta')), dict(omit=('mean', 'rstd')),
            dict(omit=('rm', 'rv')))


@pytest.mark.parametrize('name', VARIANT_CASES)
def test_single_outputs_windows_and_null_pointers(name):
    """y alone, y2 alone, y2 as a second window of y's buffer and in a buffer of another ld; NULL gamma / beta, NULL mean / rstd, NULL
    running statistics: what is written is what the exact reference allows, what is not asked for is not touched"""
    lib = _ops().lib()
    assert lib.gcc_device_error(1) == 0
    case = B.BY_NAME[name]
    d = _data(name, 'exact')
    for v in VARIANTS:
        L = Launch(case, d, **v)
        pl = L.assert_plan()
        omit = v.get('omit', ())
        ref = B.exact_ref(d, gamma='gamma' not in omit, beta='beta' not in omit, **L.acts)
        L.run(pl['launches'])
        L.check_layout('%s %r' % (name, v))
        bad = B.exact_faults(ref, L.got())
        assert not any(bad.values()), (name, v, bad)
    assert lib.gcc_device_error(0) == 0


def test_workspace_independence():
    """every case's geometry and options with the fuse values 3, 2, 1, 0 in rotation (the restated plan asserted, whatever route that
    is) in two orders on the stream's shared workspaces: the bits each gives on private, freshly zeroed ones"""
    lib = _ops().lib()
    assert lib.gcc_device_error(1) == 0
    data, want, need = [], [], 0
    cases = [dict(c, fuse=(3, 2, 1, 0)[i % 4]) for i, c in enumerate(B.CASES)]
    for case in cases:
        d = dict(B.make(case, 'normal', B.seeds(case)[1]), case=case)
        P = Launch(case, d, private=True)
        pl = P.assert_plan(regime=False)
        want.append(P.run(pl['launches']))
        data.append(d)
        need = max(need, P.ws_need)
        del P
    shared = _ops().workspace(need, DEV, 'convbn')         # grown once to the largest: every launch below holds the same buffer
    launches = [Launch(case, d) for case, d in zip(cases, data)]
    assert {L.plan()['route'] for L in launches} == {0, 1, 2}
    assert all(L.ws.data_ptr() == shared.data_ptr() for L in launches)
    n = len(launches)
    for order in (list(range(n)), [k for pair in zip(range(n - 1, n // 2 - 1, -1), range(n // 2)) for k in pair] + ([n // 2] if n & 1 else [])):
        assert sorted(order) == list(range(n))
        for k in order:
            assert _same(launches[k].run(), want[k]), 'case %s in order %r' % (launches[k].case['name'], order)
    assert lib.gcc_device_error(0) == 0


def test_declined_calls_launch_nothing():
    lib = _ops().lib()
    case = B.BY_NAME['r2-tail5']
    d = _data('r2-tail5', 'exact')

    def declined(L, code, **kw):
        before = L.bits()
        lib.gcc_launch_count(1)
        assert L.call(**kw) == code, kw
        assert lib.gcc_launch_count(0) == 0
        torch.cuda.synchronize()
        assert _same(L.bits(), before)
    L = Launch(case, d)
    assert L.ws_need > 0
    declined(L, B.WORKSPACE, ws_bytes=L.ws_need - 1)
    declined(L, B.WORKSPACE, ws_shift=8)
    declined(L, B.BAD_ARG, both_null=True)
    declined(L, B.BAD_ARG, ldy=L.y.ld + 4)
    declined(L, B.BAD_ARG, y2off=12)
    declined(Launch(case, d, omit=('scale',)), B.BAD_ARG)
    for cnt in (0.0, -4.0):
        Lc = Launch(case, d, count=cnt)
        declined(Lc, B.BAD_ARG)
        assert Lc.plan() == B.BAD_ARG
    assert lib.gcc_device_error(0) == 0


def test_ops_wrapper_reports_the_plan():
    """ops.conv_bn_act_plan on the engine's own activations: the restatement's plan"""
    import torch.nn as nn
    ops = _ops()
    cus, queues = _device_plan_args()
    for g, dg in (((16, 8, 8, 256, 256) + B.K4, False), ((16, 4, 4, 512, 256) + B.K4, True), ((16, 32, 32, 128, 256) + B.K4, False)):
        N, H, W, Ci, Co, k, s, p = g
        Ho, Wo = X.out_hw(g)
        x, y = ops.new_act(N, Ci, H, W, DEV), ops.new_act(N, Co, Ho, Wo, DEV)
        src, raw = (y, x) if dg else (x, y)
        bn = nn.BatchNorm2d(raw.shape[1]).to(DEV)
        got = ops.conv_bn_act_plan(dg, src, raw, k, s, p, bn, ops.BNState(raw.shape[1], DEV), raw.shape[0] * raw.shape[2] * raw.shape[3])
        want = B.plan(g, dg, 3, cus, queues)
        assert isinstance(got, dict) and all(got.get(k_) == v for k_, v in want.items() if v is not None), (g, got, want)
