"""gcc_dw_inorm_fwd (norm_act.hip dw_inorm_kernel, all three modes) at every plan: exact-integer data whose result is known to
the bit, bf16 normals per element against float64 with the bound derived in tests/_dwin.py, operands inside sentinel-filled
buffers, dead channels, the unread bias, independence from what earlier launches left in the stream's workspace, and the declined
geometries.  Every test first asserts the plan the library reports (gcc_dw_inorm_plan) against the restatement and against the
regime its case is named for (tests/_dwin.py CASES); nothing here skips."""
import ctypes as C
import functools
import os

import pytest
import torch

from tests import _dwin as D
from tests._perelem import report
from tests.test_norm_kernels_gpu import Win

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CASE_MODE = [(c, g, m) for c, g, _ in D.CASES for m in D.MODES]
IDS = ['%s-%s' % ('x'.join(map(str, c)), D.MODE_NAME[m]) for c, _, m in CASE_MODE]


def _ops():
    from gcc_amd import ops
    return ops


@functools.lru_cache(maxsize=1)
def _exact(case):
    return D.exact_inputs(case, D.exact_seed(case))


@functools.lru_cache(maxsize=1)
def _normal(case):
    return D.normal_inputs(case, D.normal_seed(case))


def _device_plan_args():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    q = int(os.environ.get('GPU_MAX_HW_QUEUES', '0') or 0)
    return cus, (q if q > 0 else 4)


class Launch:
    """one gcc_dw_inorm_t with every operand at chunk offset 1 of a sentinel-filled buffer, ld = ceil8(C) + 16; the pad lanes of the
    inputs hold non-zeros"""

    def __init__(self, mode, case, x, r, w, eps, workspace=None):
        from gcc_amd import _lib
        ops = _ops()
        Cc, H, Wd, N = case
        shape = (N, H * Wd, Cc)
        self.mode, self.case = mode, case
        self.x = Win(shape, 8, 8, x, pad=1.5)
        self.r = Win(shape, 8, 8, r, pad=2.0) if mode == D.RESIDUAL else None
        self.y = Win(shape, 8, 8)
        self.u = Win(shape, 8, 8) if mode == D.RESIDUAL else None
        self.w = w.float().contiguous().to(DEV)
        self.ws = workspace if workspace is not None else ops.zeroed_workspace(DEV, 'dw_inorm', _lib.DW_INORM_WORKSPACE_BYTES)
        at = lambda win: win.ptr + 2 * win.off if win is not None else None
        ld = lambda win: win.ld if win is not None else 0
        self.d = _lib.dw_inorm_t(mode, at(self.x), ld(self.x), at(self.r), ld(self.r), at(self.u), ld(self.u), self.w.data_ptr(), None,
                                 at(self.y), ld(self.y), N, H, Wd, Cc, eps, self.ws.data_ptr(), self.ws.numel())
        self.inputs = [(win, win.base.clone()) for win in (self.x, self.r) if win is not None]
        self.lib = ops.lib()

    def plan(self):
        from gcc_amd import _lib
        got = {k: int(self.lib.gcc_dw_inorm_plan(C.byref(self.d), i)) for k, i in _lib.DWIN_PLAN.items()}
        return got if min(got.values()) >= 0 else got['S']

    def assert_plan(self, regime):
        """the plan the library reports is the restatement's for this device and the one the case is named for; one launch serves it"""
        Cc, H, Wd, N = self.case
        pl = self.plan()
        cus, queues = _device_plan_args()
        assert pl == D.plan(Cc, H, Wd, N, cus, queues, self.ws.numel()), (self.case, pl, cus, queues)
        D.check_regime(self.case, regime, pl)
        assert self.lib.gcc_dw_inorm_route(C.byref(self.d)) == 1
        return pl

    def run(self):
        ops = _ops()
        self.lib.gcc_launch_count(1)
        rc = self.lib.gcc_dw_inorm_fwd(C.byref(self.d), ops.stream())
        assert rc == 0, (self.case, self.mode, rc)
        assert self.lib.gcc_launch_count(0) == 1
        torch.cuda.synchronize()
        return self.bits()

    def bits(self):
        """the whole buffers of y (and u_out), as stored"""
        return [win.base.view(torch.int16).clone() for win in (self.y, self.u) if win is not None]

    def check_layout(self, what):
        self.y.check(what + ' y')
        if self.u is not None:
            self.u.check(what + ' u_out')
        for win, before in self.inputs:
            assert torch.equal(win.base.view(torch.int16), before.view(torch.int16)), what + ': an input changed'

    def u_out(self):
        return self.u.get() if self.u is not None else None


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('case,regime,mode', CASE_MODE, ids=IDS)
def test_exact_integer_data(case, regime, mode):
    """y is the one (near a tie: either) bf16 value the exact reference allows, u_out the exact u bit for bit; twice on the same
    workspace: the same bits"""
    lib = _ops().lib()
    assert lib.gcc_device_error(1) == 0
    dat = _exact(case)
    L = Launch(mode, case, dat['u'] if mode == D.PLAIN else dat['p'], dat['r'], dat['w'], dat['eps'])
    pl = L.assert_plan(regime)
    ref = D.exact_ref(mode, dat, pl)
    assert ref['ambiguous'] <= 0.01
    first = L.run()
    what = 'exact %r %s' % (case, D.MODE_NAME[mode])
    L.check_layout(what)
    bad_y, bad_u = D.exact_faults(ref, L.y.get(), L.u_out())
    assert (bad_y, bad_u) == (0, 0), '%s: %d elements of y outside the allowed values, %d of u_out differ from the exact u' % (what, bad_y, bad_u)
    if mode == D.RESIDUAL:
        got = L.u.base[:, 0, :, L.u.off:L.u.off + case[0]].cpu().view(torch.int16)
        assert torch.equal(got, ref['u'].bfloat16().view(torch.int16)), what + ': u_out bits'
    assert _same(L.run(), first), what + ': a second launch on the same workspace gave other bits'
    assert lib.gcc_device_error(0) == 0
    print('EXACT %s %s plan=%r ambiguous=%.3g' % ('x'.join(map(str, case)), D.MODE_NAME[mode], pl, ref['ambiguous']))


@pytest.mark.parametrize('case,regime,mode', CASE_MODE, ids=IDS)
def test_per_element_against_float64(case, regime, mode):
    """bf16 normals (a channel of |mean| = 20 sigma, a dead channel) within the derived bound per element; dead channels exact;
    a bias pointer to garbage changes no bits"""
    lib = _ops().lib()
    assert lib.gcc_device_error(1) == 0
    dat = _normal(case)
    L = Launch(mode, case, dat['x'], dat['r'], dat['w'], dat['eps'])
    pl = L.assert_plan(regime)
    first = L.run()
    what = 'normal %r %s' % (case, D.MODE_NAME[mode])
    L.check_layout(what)
    ratios = D.normal_check(mode, dat, pl, L.y.get(), L.u_out(), what)
    garbage = torch.full((case[0] + 64,), float('nan'), device=DEV)
    garbage[::2] = 3e38
    L.d.bias = garbage.data_ptr()
    assert _same(L.run(), first), what + ': the bias was read'
    assert lib.gcc_device_error(0) == 0
    report('dw_inorm_' + D.MODE_NAME[mode], case, **ratios)


def test_workspace_independence():
    """every case, modes in rotation, in two orders on the stream's shared workspace: the bits of a private, freshly zeroed one"""
    from gcc_amd import _lib
    lib = _ops().lib()
    assert lib.gcc_device_error(1) == 0
    g = torch.Generator().manual_seed(5)
    launches, want = [], []
    for i, (case, regime, _) in enumerate(D.CASES):
        Cc, H, Wd, N = case
        mode = D.MODES[i % 3]
        x, r = (torch.randn(N, H * Wd, Cc, generator=g) for _ in range(2))
        w = torch.randn(Cc, 9, generator=g)
        private = torch.zeros(_lib.DW_INORM_WORKSPACE_BYTES, dtype=torch.uint8, device=DEV)
        P = Launch(mode, case, x, r, w, D.EPS, workspace=private)
        P.assert_plan(regime)
        want.append(P.run())
        L = Launch(mode, case, x, r, w, D.EPS)
        L.assert_plan(regime)
        launches.append(L)
    n = len(launches)
    # ascending, then an order that puts every large layout right behind a small one and the two-level exchange last
    for order in (list(range(n)), [k for pair in zip(range(n - 1, n // 2 - 1, -1), range(n // 2)) for k in pair] + ([n // 2] if n & 1 else [])):
        assert sorted(order) == list(range(n))
        for k in order:
            assert _same(launches[k].run(), want[k]), 'case %r after %r' % (launches[k].case, order)
    assert lib.gcc_device_error(0) == 0


def test_ops_wrapper_reports_the_plan():
    """ops.dw_inorm_plan on the engine's own activations: the restatement's plan, or the code of a declined geometry"""
    ops = _ops()
    cus, queues = _device_plan_args()
    for (Cc, H, Wd, N), mode in (((256, 64, 64, 1), D.RESIDUAL), ((40, 33, 17, 2), D.PLAIN), ((24, 4, 527, 1), D.NORM_RELU)):
        x, r, y, u = (ops.new_act(N, Cc, H, Wd, DEV) for _ in range(4))
        w = torch.zeros(Cc, 1, 3, 3, device=DEV)
        kw = dict(r=r, u_out=u) if mode == D.RESIDUAL else {}
        assert ops.dw_inorm_plan(mode, x, w, y, **kw) == D.plan(Cc, H, Wd, N, cus, queues), (Cc, H, Wd, N)


@pytest.mark.parametrize('case,why', D.DECLINED, ids=[w for _, w in D.DECLINED])
def test_declined_geometries_launch_nothing(case, why):
    lib = _ops().lib()
    Cc, H, Wd, N = case
    z = torch.zeros(N, H * Wd, Cc)
    for mode in D.MODES:
        L = Launch(mode, case, z, z, torch.zeros(Cc, 9), D.EPS)
        cus, queues = _device_plan_args()
        assert D.plan(Cc, H, Wd, N, cus, queues) == D.UNSUPPORTED
        assert L.plan() == D.UNSUPPORTED and lib.gcc_dw_inorm_route(C.byref(L.d)) == D.UNSUPPORTED
        before = L.bits()
        lib.gcc_launch_count(1)
        assert lib.gcc_dw_inorm_fwd(C.byref(L.d), _ops().stream()) == D.UNSUPPORTED
        assert lib.gcc_launch_count(0) == 0
        torch.cuda.synchronize()
        assert _same(L.bits(), before)
    assert lib.gcc_device_error(0) == 0
