"""The kernels of csrc/norm_act.hip per element against float64: BatchNorm / InstanceNorm statistics, gcc_bnact_fwd, every route of
gcc_bnact_bwd_ex (act_bwd_kernel, bnact_bwd_small_kernel, reduce + finalize + apply with and without the in-launch finalize,
gcc_bn_bwd_one_launch(_ex)), eval mode, gcc_inorm_fwd / gcc_inorm_bwd -- at the loop edges of make_layout / stream_blocks /
bwd_blocks / SMALL_MAX_PIXELS / FIN_GROUP, in channel windows of wider sentinel-filled buffers, through the ops wrappers and
through the C entries with non-zero offsets.

The reference is tests/_perelem.py fwd_math / bwd_ref in float64 on exactly the values the kernel reads (inputs are bf16 by
construction; the saved output y and the dropout mask, rng_uniform(seed, pix * C + c) >= p written in numpy uint64, are inputs
too).  Every backward case carries a per-channel offset and a component along xhat in its incoming gradient, so that both
projection terms of the BatchNorm backward are of the order of rms(dz) whatever the pixel count (asserted on the reference).

Bounds (per element, tests/_perelem.py): bf16 outputs |err| <= 2^-8 (1 + 2^-7) |ref| + k 2^-24 M, M the sum of the magnitudes of
the terms of the element, k counted from the kernel (K_FWD, K_DZ, K_APPLY); the three-launch route stores dz as bf16 between
reduce and apply and gains |A| 2^-8 |dz|, the one-launch kernels do not; fp32 outputs n 2^-24 (sum of the magnitudes of the summed
terms), n the longest fp32 chain (chain_three / CHAIN_SMALL / chain_grid); rstd / scale through d(var^-1/2) = var^-3/2 / 2.  The
bf16 term is the format's unit roundoff 2^-8: 2^-9 cannot be met by any rounding to bf16 (tests/test_norm_bounds_cpu.py, which
also shows that an emulation of the kernels passes these bounds and wrong formulas do not).  Elements whose activation sign is
recomputed from x (y = None) within 8 * 2^-24 of the affine's terms of zero are left out of the dx comparison (at most 0.1 %).
Bit for bit: the zero pattern under dropout, pad lanes, sentinels outside a window, in place against out of place, two calls on
one workspace.  Each case prints its worst err / bound (RATIO lines, docs/lab_notebook.md)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import _perelem as T
from tests._perelem import within, report, UNSUPPORTED

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENT = -3.0          # what every lane outside a window holds before and after a call


def _ops():
    from gcc_amd import ops
    return ops


class Win:
    """a [G, P, C] activation in channels [off, off + C) of a [G, 1, P, ld] buffer filled with the sentinel; pad: what the
    lanes C .. ceil8(C) - 1 of the window hold (an output window: the sentinel, the kernel must write zeros there)"""

    def __init__(self, shape, ld_extra=8, off=8, vals=None, pad=SENT):
        G, P, Cc = shape
        self.G, self.P, self.C, self.C8, self.off = G, P, Cc, (Cc + 7) & ~7, off
        self.ld = off + self.C8 + ld_extra
        base = torch.full((G, 1, P, self.ld), SENT, dtype=torch.bfloat16)
        if vals is not None:
            base[:, 0, :, off:off + Cc] = vals.to(torch.bfloat16)
            base[:, 0, :, off + Cc:off + self.C8] = pad
        self.base = base.to(DEV)
        self.view = self.base.permute(0, 3, 1, 2)[:, off:off + Cc]
        self.ptr = self.base.data_ptr()

    def get(self):
        return self.base[:, 0, :, self.off:self.off + self.C].double().cpu()

    def check(self, what):
        b = self.base[:, 0].float().cpu()
        assert bool((b[..., self.off + self.C:self.off + self.C8] == 0).all()), '%s: pad lanes not zero' % what
        assert bool((b[..., :self.off] == SENT).all()) and bool((b[..., self.off + self.C8:] == SENT).all()), \
            '%s: a lane outside the window changed' % what


def _f32(t):
    return None if t is None else t.float().contiguous().to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


# ---- B: gcc_bnact_fwd ----------------------------------------------------------------------------------------------------
def _run_fwd(P, Cc, opt, seed, G=1, raw=False):
    ops = _ops()
    from gcc_amd import _lib
    d, kw = T.fwd_case(P, Cc, opt, seed, G)
    if G > 1 and kw['scale'] is not None:       # InstanceNorm: [G][C] coefficients
        kw['scale'], kw['shift'] = kw['scale'].reshape(G, 1, Cc), kw['shift'].reshape(G, 1, Cc)
    y_ref, y2_ref, M, M2 = T.fwd_math(torch.float64, d['x'], **kw)
    x = Win((G, P, Cc), 16, 8, d['x'], pad=1.5)
    y = None if opt.get('no_y') else Win((G, P, Cc), 8, 8)
    y2 = Win((G, P, Cc), 24, 16) if opt.get('y2') else None
    res = Win((G, P, Cc), 8, 0, kw['res'], pad=2.0) if kw['res'] is not None else None
    sc, sf, gate = _f32(kw['scale']), _f32(kw['shift']), _f32(kw['gate'])
    if raw:
        p = _lib.bnact_t(_p(sc), _p(sf), _p(gate), int(kw['after']), kw['act'], 0.2, kw['act2'], kw['p'], seed, G,
                         res.ld if res else 0, res.view.data_ptr() if res else None)
        ops.check(ops.lib().gcc_bnact_fwd(C.byref(p), x.ptr, x.ld, x.off, y.ptr if y else None, y.ld if y else 0, y.off if y else 0,
                                          y2.ptr if y2 else None, y2.ld if y2 else 0, y2.off if y2 else 0, Cc, P, ops.stream()), 'gcc_bnact_fwd')
    else:
        ops.bnact_fwd(x.view, y.view if y else None, y2.view if y2 else None, scale=sc, shift=sf, gate=gate, gate_after_act=kw['after'],
                      act=kw['act'], slope=0.2, act2=kw['act2'], drop_p=kw['p'], seed=seed, groups=G, residual=res.view if res else None)
    torch.cuda.synchronize()
    ratios = {}
    for name, w, ref, m, a in (('y', y, y_ref, M, kw['act']), ('y2', y2, y2_ref, M2, kw['act2'])):
        if w is None:
            continue
        got = w.get()
        what = 'fwd %s %dx%dx%d %r' % (name, G, P, Cc, opt)
        w.check(what)
        ratios[name] = within(got, ref, T.fwd_bound(ref, m, a), what)
        if kw['keep'] is not None:
            # the zero pattern is the numpy mask: exactly, where nothing else makes a zero (tanh / leaky outputs, open gates)
            assert torch.equal(got == 0, ref == 0), what + ': zero pattern'
            if a in (T.ACT_TANH, T.ACT_LRELU) and res is None:
                live = (kw['gate'] != 0) if kw['gate'] is not None else torch.ones(Cc, dtype=torch.bool)
                assert torch.equal((got == 0)[..., live], (~kw['keep']).expand(G, P, Cc)[..., live]), what + ': mask'
    return ratios, (y.base.clone() if y else None, y2.base.clone() if y2 else None)


@pytest.mark.parametrize('Cc', T.FWD_C)
def test_bnact_fwd_channel_and_pixel_edges(Cc):
    """every CH of make_layout x {1, PPB, PPB + 1, 2 PPB + 1} pixels, the options of FWD_OPTIONS rotating over them, each case
    through ops.bnact_fwd (windows by pointer) and through the C entry with non-zero xoff / yoff / y2off: the same bits"""
    worst = {}
    for pi, P in enumerate(T.fwd_pixels(Cc)):
        opt = T.FWD_OPTIONS[(T.FWD_C.index(Cc) + pi) % len(T.FWD_OPTIONS)]
        r, a = _run_fwd(P, Cc, opt, 1000 + Cc + P)
        _, b = _run_fwd(P, Cc, opt, 1000 + Cc + P, raw=True)
        for u, v in zip(a, b):
            assert (u is None and v is None) or torch.equal(u, v), 'C entry with offsets against the pointer windows'
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    report('bnact_fwd', (Cc,), **worst)


@pytest.mark.parametrize('oi', range(len(T.FWD_OPTIONS)))
def test_bnact_fwd_options(oi):
    """every option set at C = 20 (a pad tail) and C = 264 (33 chunks in 64 lanes), 2 PPB + 1 pixels"""
    worst = {}
    for Cc in (20, 264):
        r, _ = _run_fwd(T.fwd_pixels(Cc)[3], Cc, T.FWD_OPTIONS[oi], 1100 + Cc + oi)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    report('bnact_fwd_opt', (oi,), **worst)


def test_bnact_fwd_above_the_workgroup_cap():
    r, _ = _run_fwd(8192 + 3, 520, T.FWD_OPTIONS[1], 1200)        # 2 pixels per sweep: 4098 blocks wanted, 2048 run
    assert T.fwd_blocks(8192 + 3, 520) == 2048
    report('bnact_fwd_cap', (8195, 520), **r)


@pytest.mark.parametrize('Cc', [6, 12])
def test_bnact_fwd_groups(Cc):
    """groups = N: per-image coefficients; C = 6, N = 3: the scalar-parameter branch (po & 3 != 0), C = 12: the vector one.  The
    dropout counter is the pixel index within the image"""
    worst = {}
    for opt in (dict(act=T.ACT_RELU), dict(act=T.ACT_LRELU, drop=0.5), dict(act=T.ACT_NONE, res=True)):
        for raw in (False, True):
            r, _ = _run_fwd(37, Cc, opt, 1300 + Cc, G=3, raw=raw)
            worst['y'] = max(worst.get('y', 0.0), r['y'])
    report('bnact_fwd_groups', (3, Cc), **worst)


# ---- C: gcc_bnact_bwd_ex --------------------------------------------------------------------------------------------------
class Routes:
    """pins the routing knobs of ops.bnact_bwd for one call"""

    def __init__(self, monkeypatch):
        self.mp = monkeypatch

    def set(self, route, tail=False):
        ops = _ops()
        from gcc_amd import _lib
        self.mp.setattr(ops, 'BN_BWD_GRID', False)
        self.mp.setattr(ops, 'BN_BWD_GRID_EX', 0)
        self.mp.setattr(ops, 'BN_BWD_TAIL', tail)
        self.prev = ops.lib().gcc_set_option(_lib.OPT_BN_BWD_SMALL, 0 if route == 'three' else 1)

    def restore(self):
        from gcc_amd import _lib
        _ops().lib().gcc_set_option(_lib.OPT_BN_BWD_SMALL, self.prev)


def _state(d, bn):
    ops = _ops()
    st = ops.BNState(d['x'].shape[2], DEV)
    if bn:
        st.mean.copy_(d['mean']); st.rstd.copy_(d['rstd'])
        st.scale.copy_((d['gamma'] * d['rstd']).float()); st.shift.copy_((d['beta'] - d['mean'] * d['gamma'] * d['rstd']).float())
    return st


def _run_bwd(route, P, Cc, opt, seed, routes, tail=False, bn_eval=False, inplace=False, raw=False, prior_val=0.375, st=None):
    """one backward call on `route` ('three' / 'small' / 'act' through ops.bnact_bwd or the C entry with offsets; 'grid' through
    gcc_bn_bwd_one_launch(_ex)); returns the outputs as read back and the launch count"""
    ops = _ops()
    from gcc_amd import _lib
    d, y, kw = T.bwd_case(P, Cc, opt, seed)
    bn = kw['bn']
    x = Win((1, P, Cc), 16, 8, d['x'], pad=1.5)
    yw = Win((1, P, Cc), 8, 8, y, pad=0.0) if y is not None else None
    g1 = Win((1, P, Cc), 8, 16, d['g1'], pad=0.0)
    g2 = Win((1, P, Cc), 24, 0, kw['g2'], pad=0.0) if kw['g2'] is not None else None
    dx = g1 if inplace else Win((1, P, Cc), 16, 16)
    st = st or _state(d, bn)
    gamma, beta, gate = _f32(kw['gamma']), _f32(kw['beta']), _f32(kw['gate'])
    prior = {n: torch.full((Cc,), v, device=DEV) for n, v in (('dgamma', prior_val), ('dbeta', -prior_val), ('dalpha', 2 * prior_val))}
    before = {n: v.cpu() for n, v in prior.items()}          # non-zero contents: the parameter gradients accumulate
    dgamma, dbeta = (prior['dgamma'], prior['dbeta']) if bn else (None, None)
    dalpha = prior['dalpha'] if kw['gated'] else None
    lib = ops.lib()
    lib.gcc_launch_count(1)
    if route == 'grid':
        ws = ops.inorm_workspace(DEV)
        if opt.get('ex'):
            rc = lib.gcc_bn_bwd_one_launch_ex(x.view.data_ptr(), x.ld, yw.view.data_ptr() if yw else None, yw.ld if yw else 0, g1.view.data_ptr(),
                                              g1.ld, g2.view.data_ptr() if g2 else None, g2.ld if g2 else 0, dx.view.data_ptr(), dx.ld, Cc, P,
                                              kw['act'], kw['act2'], 0.2, kw['p'], seed, st.mean.data_ptr(), st.rstd.data_ptr(),
                                              st.scale.data_ptr(), st.shift.data_ptr(), _p(gamma), _p(dgamma), _p(dbeta), ws.data_ptr(),
                                              ws.numel(), ops.stream())
        else:
            rc = lib.gcc_bn_bwd_one_launch(x.view.data_ptr(), x.ld, yw.view.data_ptr() if yw else None, yw.ld if yw else 0, g1.view.data_ptr(),
                                           g1.ld, dx.view.data_ptr(), dx.ld, Cc, P, kw['act'], 0.2, st.mean.data_ptr(), st.rstd.data_ptr(),
                                           _p(gamma), _p(dgamma), _p(dbeta), ws.data_ptr(), ws.numel(), ops.stream())
        ops.check(rc, 'gcc_bn_bwd_one_launch')
    else:
        routes.set(route, tail)
        try:
            if raw:
                p = _lib.bnact_bwd_t(int(bn), int(bn_eval), _p(st.mean) if bn else None, _p(st.rstd) if bn else None, _p(gamma), _p(beta),
                                     _p(gate), int(kw['after']), kw['act'], 0.2, kw['act2'], kw['p'], seed, _p(dgamma), _p(dbeta), _p(dalpha),
                                     1, 1 if tail else 0)
                need = lib.gcc_bnact_bwd_workspace(Cc, P)
                ws = ops.zeroed_workspace(DEV, 'bnbwd', need) if tail else ops.workspace(need, DEV, 'bnbwd')
                ops.check(lib.gcc_bnact_bwd_ex(C.byref(p), kw['in_act'], 0.2, x.ptr, x.ld, x.off, yw.ptr if yw else None, yw.ld if yw else 0,
                                               yw.off if yw else 0, g1.ptr, g1.ld, g1.off, g2.ptr if g2 else None, g2.ld if g2 else 0,
                                               g2.off if g2 else 0, dx.ptr, dx.ld, dx.off, Cc, P, ws.data_ptr(), ws.numel(), ops.stream()),
                          'gcc_bnact_bwd_ex')
            else:
                ops.bnact_bwd(x.view, yw.view if yw else None, g1.view, dx.view, g2=g2.view if g2 else None, bn=st if bn else None,
                              gamma=gamma, beta=beta, bn_eval=bn_eval, gate=gate, gate_after_act=kw['after'], act=kw['act'], slope=0.2,
                              act2=kw['act2'], drop_p=kw['p'], seed=seed, dgamma=dgamma, dbeta=dbeta, dalpha=dalpha, in_act=kw['in_act'])
        finally:
            routes.restore()
    launches = int(lib.gcc_launch_count(1))
    torch.cuda.synchronize()
    dx.check('bwd dx %s %dx%d %r' % (route, P, Cc, opt))
    out = dict(dx=dx.get(), dx_bits=dx.base.clone(), launches=launches)
    for n in ('dgamma', 'dbeta', 'dalpha'):
        out[n] = prior[n].cpu()
    return out, (d, y, kw, before)


def _compare_bwd(route, P, Cc, opt, out, case, bn_eval=False, chain=None, tag=''):
    d, y, kw, prior = case
    chain = chain or {'three': T.chain_three(P, Cc), 'small': T.CHAIN_SMALL, 'act': 1}[route]
    pri = prior
    ref = T.bwd_ref(d['x'], y, d['g1'], bn_eval=bn_eval, n_chain=chain, three=route == 'three', prior=pri, **kw)
    what = 'bwd %s%s %dx%d %r' % (route, tag, P, Cc, opt)
    if kw['bn'] and not bn_eval and P >= 64:
        T.strong_gradient(ref, what)
    assert float(ref['open'].double().mean()) <= 1e-3, what
    keep = ~ref['open']
    ratios = dict(dx=within(torch.where(keep, out['dx'], ref['dx'][0]), ref['dx'][0], ref['dx'][1], what + ' dx'))
    names = (('dgamma', 'dbeta') if kw['bn'] else ()) + (('dalpha',) if kw['gated'] else ())
    for n in names:
        ratios[n] = within((out[n].double() - pri[n].double())[None], ref[n][0], ref[n][1], what + ' ' + n)
    for n in set(('dgamma', 'dbeta', 'dalpha')) - set(names):
        assert torch.equal(out[n], pri[n]), what + ': %s written' % n
    return ratios, ref


@pytest.mark.parametrize('P,Cc,opt', T.BWD_ACT)
def test_act_bwd_kernel(P, Cc, opt, monkeypatch):
    """dx = (g1 act'(y) + g2 act2'(y)) in_act'(x) in one launch: in_act over NONE / RELU / LRELU / TANH, y given or x standing in
    for it, out of place, in place over g1, and through the C entry with offsets"""
    routes = Routes(monkeypatch)
    o = dict(opt, bn=False)
    out, case = _run_bwd('act', P, Cc, o, 3500 + P + Cc, routes)
    assert out['launches'] == 1
    r, _ = _compare_bwd('act', P, Cc, o, out, case)
    inp, _ = _run_bwd('act', P, Cc, o, 3500 + P + Cc, routes, inplace=True)
    rawo, _ = _run_bwd('act', P, Cc, o, 3500 + P + Cc, routes, raw=True)
    assert torch.equal(inp['dx'], out['dx']) and torch.equal(rawo['dx_bits'], out['dx_bits'])
    report('act_bwd', (P, Cc), **r)


@pytest.mark.parametrize('P,Cc,opt', T.BWD_SMALL)
def test_bnact_bwd_small_kernel(P, Cc, opt, monkeypatch):
    """1, 511, 512, 513 and 4096 (SMALL_MAX_PIXELS) pixels, with and without dropout and a second gradient, y given or recomputed;
    dz stays in fp32: the bound has no bf16 round trip in it"""
    routes = Routes(monkeypatch)
    out, case = _run_bwd('small', P, Cc, opt, 3000 + P + Cc, routes)
    assert out['launches'] == 1
    r, _ = _compare_bwd('small', P, Cc, opt, out, case)
    inp, _ = _run_bwd('small', P, Cc, opt, 3000 + P + Cc, routes, inplace=True)
    assert torch.equal(inp['dx'], out['dx'])
    report('bn_bwd_small', (P, Cc), **r)


@pytest.mark.parametrize('tail', [False, True])
@pytest.mark.parametrize('P,Cc,blocks,opt', T.BWD_THREE)
def test_bnact_bwd_three_launches(P, Cc, blocks, opt, tail, monkeypatch):
    """reduce + finalize + apply (tail: the reduce pass's last workgroups finalize) at 1, 15, 16, 17, 33, 97, 129 and 1024 partial
    rows: the four gate x dropout instantiations, gate before and after the activation with d(alpha), a second gradient, y
    recomputed; parameter gradients accumulate into non-zero contents; twice on one workspace, in place, and the C entry with
    offsets give the same bits"""
    ops = _ops()
    routes = Routes(monkeypatch)
    assert ops.lib().gcc_bnact_bwd_workspace(Cc, P) == T.bwd_workspace(Cc, blocks)
    seed = 3000 + P + Cc
    out, case = _run_bwd('three', P, Cc, opt, seed, routes, tail=tail)
    assert out['launches'] == (2 if tail else 3), out['launches']
    r, _ = _compare_bwd('three', P, Cc, opt, out, case, tag=' tail' if tail else '')
    again, _ = _run_bwd('three', P, Cc, opt, seed, routes, tail=tail, inplace=True)
    rawo, _ = _run_bwd('three', P, Cc, opt, seed, routes, tail=tail, raw=True)
    for o in (again, rawo):
        assert torch.equal(o['dx'], out['dx']) and all(torch.equal(o[n], out[n]) for n in ('dgamma', 'dbeta', 'dalpha'))
    assert torch.equal(rawo['dx_bits'], out['dx_bits'])
    report('bn_bwd_three' + ('_tail' if tail else ''), (P, Cc, blocks), **r)


def test_bnact_bwd_three_launches_groups(monkeypatch):
    """groups = N (InstanceNorm through the three-launch route): per-image statistics and sums, no parameter gradients"""
    ops = _ops()
    G, P, Cc = 3, 531, 12
    d = T.norm_inputs(P, Cc, 4100, G, affine=False)
    kw = dict(mean=d['mean'], rstd=d['rstd'], bn=True, act=T.ACT_RELU, slope=0.2)
    sc, sf = d['rstd'], -d['mean'] * d['rstd']
    y = T.rb64(T.fwd_math(torch.float64, d['x'], sc, sf, act=T.ACT_RELU)[0])
    ref = T.bwd_ref(d['x'], y, d['g1'], n_chain=T.chain_three(P, Cc), three=True, **kw)
    x, yw, g1, dx = (Win((G, P, Cc), 8, 8, v, pad=0.0) for v in (d['x'], y, d['g1'], None))
    st = ops.INState(G, Cc, DEV)
    st.mean.copy_(d['mean'][:, 0]); st.rstd.copy_(d['rstd'][:, 0])
    routes = Routes(monkeypatch)
    routes.set('three')
    try:
        ops.bnact_bwd(x.view, yw.view, g1.view, dx.view, bn=st, act=T.ACT_RELU, groups=G)
    finally:
        routes.restore()
    torch.cuda.synchronize()
    dx.check('groups')
    report('bn_bwd_three_groups', (G, P, Cc), dx=within(dx.get(), ref['dx'][0], ref['dx'][1], 'three-launch route, groups = 3'))


@pytest.mark.parametrize('P,Cc,opt', T.BWD_GRID)
def test_bn_bwd_one_launch_grid_kernels(P, Cc, opt):
    """gcc_bn_bwd_one_launch and its _ex form on the current stream, one launch at a time: dz stays in fp32 (no bf16 round trip in
    the bound); a second gradient, dropout, y recomputed through the forward's scale / shift, windows, in place"""
    ops = _ops()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    chain, plan = T.chain_grid(P, Cc, cus=min(cus, 256), px=2 if opt.get('ex') else 4)
    print('PLAN bn_bwd_grid %dx%d on %d CUs: %r' % (P, Cc, cus, plan))
    seed = 3000 + P + Cc
    out, case = _run_bwd('grid', P, Cc, opt, seed, None)
    assert out['launches'] == 1
    r, _ = _compare_bwd('grid', P, Cc, opt, out, case, chain=chain)
    again, _ = _run_bwd('grid', P, Cc, opt, seed, None, inplace=True)
    assert torch.equal(again['dx'], out['dx']) and torch.equal(again['dgamma'], out['dgamma'])
    assert ops.lib().gcc_device_error(0) == 0
    report('bn_bwd_grid', (P, Cc), **r)


def test_bnact_bwd_refusals(monkeypatch):
    """C = 1032 (258 four-channel chunks) on the three-launch route and C = 2056 on every route: GCC_ERR_UNSUPPORTED, nothing launched"""
    ops = _ops()
    from gcc_amd import _lib
    lib = ops.lib()
    routes = Routes(monkeypatch)
    for Cc, route in ((1032, 'three'), (2056, 'three'), (2056, 'small')):
        C8, P = (Cc + 7) & ~7, 4
        x, g, dx = (torch.zeros((P, C8), dtype=torch.bfloat16, device=DEV) for _ in range(3))
        st = ops.BNState(Cc, DEV)
        st.rstd.fill_(1.0)
        p = _lib.bnact_bwd_t(1, 0, _p(st.mean), _p(st.rstd), None, None, None, 0, T.ACT_RELU, 0.2, T.ACT_NONE, 0.0, 0, None, None, None, 1, 0)
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
        routes.set(route)
        try:
            before = int(lib.gcc_launch_count(0))
            rc = lib.gcc_bnact_bwd_ex(C.byref(p), T.ACT_NONE, 0.2, x.data_ptr(), C8, 0, None, 0, 0, g.data_ptr(), C8, 0, None, 0, 0,
                                      dx.data_ptr(), C8, 0, Cc, P, ws.data_ptr(), ws.numel(), ops.stream())
            after = int(lib.gcc_launch_count(0))
        finally:
            routes.restore()
        if Cc == 2056:
            assert lib.gcc_bnact_bwd_workspace(Cc, P) == 0
        assert rc == UNSUPPORTED, (Cc, route, rc)
        assert after == before, (Cc, route)


# ---- the eval-mode backward ------------------------------------------------------------------------------------------------
def _eval_autograd(d, kw, y):
    """float64 autograd through F.batch_norm(training=False) of the same function, the saved y deciding the activation branch"""
    P, Cc = d['x'].shape[1:]
    x = d['x'][0].t().reshape(1, Cc, P, 1).clone().requires_grad_(True)
    gamma, beta = d['gamma'].double().clone().requires_grad_(True), d['beta'].double().clone().requires_grad_(True)
    rm, rv = d['mean'].double(), 1.0 / d['rstd'].double() ** 2 - 1e-5          # rv + eps = rstd^-2 to double precision
    z = F.batch_norm(x, rm, rv, gamma, beta, training=False, eps=1e-5)
    out = F.leaky_relu(z, 0.2) if kw['act'] == T.ACT_LRELU else F.relu(z)
    (out * d['g1'][0].t().reshape(1, Cc, P, 1)).sum().backward()
    return x.grad.reshape(Cc, P).t()[None], gamma.grad, beta.grad


@pytest.mark.parametrize('as_finalize_leaves_it', [False, True])
@pytest.mark.parametrize('P,Cc,opt', [(531, 40, dict(act=T.ACT_LRELU)), (4097, 40, dict(act=T.ACT_RELU, no_y=True)),
                                       (505, 40, dict(act=T.ACT_LRELU, gate=True)), (471, 40, dict(act=T.ACT_RELU, drop=0.5))])
def test_bnact_bwd_eval_mode(P, Cc, opt, as_finalize_leaves_it, monkeypatch):
    """bn_eval=True: dx = gamma rstd dz, d(beta) += sum dz, d(gamma) += sum dz xhat with the running statistics -- once with a
    BNState filled by hand, once with the state exactly as BNOp.finalize(train=False) leaves it (the regression test of the
    eval-mode state: gcc_bn_eval_state writes mean / rstd next to scale / shift).  The reference is the closed form, itself checked
    against float64 autograd through F.batch_norm(training=False) where the case has neither gate nor dropout."""
    ops = _ops()
    from gcc_amd import engine
    seed = 3700 + P + Cc
    d, y, kw = T.bwd_case(P, Cc, opt, seed)
    st = None
    if as_finalize_leaves_it:
        bn = torch.nn.BatchNorm2d(Cc).to(DEV)
        with torch.no_grad():
            # running statistics that give back the case's fp32 mean and (up to the kernel's own 1 / sqrtf) its rstd
            bn.weight.copy_(d['gamma']); bn.bias.copy_(d['beta']); bn.running_mean.copy_(d['mean'])
            bn.running_var.copy_((1.0 / d['rstd'].double() ** 2).float() - bn.eps)
        st = ops.BNState(Cc, DEV)
        st.mean.fill_(123.0); st.rstd.fill_(0.0)          # stale contents of an earlier training step
        engine.BNOp(bn).finalize(None, P, st, train=False)
        torch.cuda.synchronize()
        rstd = st.rstd.cpu()
        assert torch.equal(st.mean.cpu(), d['mean'])
        within(rstd, d['rstd'], 8 * T.U24 * d['rstd'].double().abs() + 1.5 * T.U24 * d['rstd'].double().abs() ** 3, 'eval rstd')
        within(st.scale.cpu(), d['gamma'].double() * rstd.double(), 2 * T.U24 * (d['gamma'] * rstd).double().abs(), 'eval scale')
        d = dict(d, rstd=rstd)       # the statistics the kernel reads
    routes = Routes(monkeypatch)
    out, case = _run_bwd('three', P, Cc, opt, seed, routes, bn_eval=True, st=st)
    case = (d, case[1], dict(case[2], rstd=d['rstd']), case[3])
    assert out['launches'] == 2           # reduce + finalize: no apply pass
    r, ref = _compare_bwd('three', P, Cc, opt, out, case, bn_eval=True)
    if y is not None and not opt.get('gate') and not opt.get('drop'):
        gx, gg, gb = _eval_autograd(d, case[2], y)
        same = (y[0] > 0) == ((d['x'][0] - d['mean'].double()) * d['rstd'].double() * d['gamma'].double() + d['beta'].double() > 0)
        assert torch.allclose(torch.where(same, gx[0], ref['dx'][0][0]), ref['dx'][0][0], rtol=1e-9, atol=1e-12)
        assert float((~same).double().mean()) < 1e-2
        if bool(same.all()):
            assert torch.allclose(gg, ref['dgamma'][0][0], rtol=1e-9, atol=1e-9) and torch.allclose(gb, ref['dbeta'][0][0], rtol=1e-9, atol=1e-9)
    report('bn_bwd_eval' + ('_state' if as_finalize_leaves_it else ''), (P, Cc), **r)


# ---- A: statistics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cc', [1, 31, 32, 33, 264])
def test_bn_and_in_finalize(Cc):
    """gcc_bn_finalize / gcc_in_finalize on partial rows as given (fp32 rows folded in double: the only fp32 roundings are the
    stored values'): 1, 15, 16, 17, 512 and 513 rows (FIN_GROUP = 16 and the 32-group chunk), 3 groups, running statistics with the
    unbiased factor at count 1 and 2 and at the rows' own count"""
    ops = _ops()
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    worst = {}
    for tiles in (1, 15, 16, 17, 512, 513):
        for count in ((1, 2) if tiles == 1 else (tiles * 7,)):
            g = torch.Generator().manual_seed(tiles * 1000 + Cc + count)
            G = 3
            per = count / tiles
            mu = torch.randn(Cc, generator=g)
            mu[0] = 20.0
            s = (torch.rand(G, tiles, Cc, generator=g) + 0.5) * per * mu
            ss = (torch.rand(G, tiles, Cc, generator=g) + 0.5) * per * (mu * mu + 1.0)
            if Cc > 2:
                s[:, :, 2], ss[:, :, 2] = 0.75 * per, 0.5625 * per          # a constant channel: variance 0
            stats = torch.stack([s, ss], 2).contiguous()                     # [G][tiles][2][C]
            gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
            if Cc > 1:
                gamma[1] = 0.0
            S, SS = s.double().sum(1), ss.double().sum(1)
            m = S / count
            var = (SS / count - m * m).clamp_min(0.0)
            r = 1.0 / torch.sqrt(var + eps)
            # the double fold: 2^-53 per addition on sums of positive-magnitude rows, through the cancellation of the variance
            dvar = (tiles + 4) * 2.0 ** -53 * (ss.double().abs().sum(1) / count + 2 * m.abs() * s.double().abs().sum(1) / count)
            dr = 0.5 * (var + eps - dvar).clamp_min(eps * 0.5) ** -1.5 * dvar + T.U24 * r
            dm = T.U24 * m.abs() + (tiles + 2) * 2.0 ** -53 * s.double().abs().sum(1) / count
            # InstanceNorm form: 3 groups, no affine
            st = ops.INState(G, Cc, DEV)
            ops.in_finalize(stats.to(DEV), count, st)
            torch.cuda.synchronize()
            what = 'in_finalize %d rows C %d count %d' % (tiles, Cc, count)
            res = dict(mean=within(st.mean.cpu(), m, dm, what + ' mean'), rstd=within(st.rstd.cpu(), r, dr, what + ' rstd'),
                       scale=within(st.scale.cpu(), r, dr, what + ' scale'),
                       shift=within(st.shift.cpu(), -m * r, 3 * T.U24 * (m * r).abs() + m.abs() * dr + dm * r, what + ' shift'))
            # BatchNorm form: group 0, affine and running statistics
            bst = ops.BNState(Cc, DEV)
            rm0, rv0 = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
            rm, rv = rm0.to(DEV), rv0.to(DEV)
            ops.bn_finalize(stats[0].contiguous().to(DEV), count, gamma.to(DEV), beta.to(DEV), rm, rv, bst)
            torch.cuda.synchronize()
            what = 'bn_finalize %d rows C %d count %d' % (tiles, Cc, count)
            gd, bd = gamma.double(), beta.double()
            assert torch.equal(bst.mean.cpu(), st.mean[0].cpu()) and torch.equal(bst.rstd.cpu(), st.rstd[0].cpu())
            res['bn_scale'] = within(bst.scale.cpu(), gd * r[0], 2 * T.U24 * (gd * r[0]).abs() + gd.abs() * dr[0], what + ' scale')
            res['bn_shift'] = within(bst.shift.cpu(), bd - m[0] * gd * r[0], 4 * T.U24 * (bd.abs() + (m[0] * gd * r[0]).abs()) +
                                     (m[0] * gd).abs() * dr[0] + dm[0] * (gd * r[0]).abs(), what + ' shift')
            unb = var[0] * count / (count - 1.0) if count > 1 else var[0]
            res['rmean'] = within(rm.cpu(), 0.9 * rm0.double() + 0.1 * m[0], 4 * T.U24 * (rm0.double().abs() + m[0].abs()) + 0.1 * dm[0],
                                  what + ' running mean')
            res['rvar'] = within(rv.cpu(), 0.9 * rv0.double() + 0.1 * unb, 4 * T.U24 * (rv0.double().abs() + unb.abs()) +
                                 0.2 * dvar[0] + 0.1 * T.U24 * unb, what + ' running var')
            for k, v in res.items():
                worst[k] = max(worst.get(k, 0.0), v)
    report('finalize', (Cc,), **worst)


@pytest.mark.parametrize('Cc', [1, 31, 32, 33, 264])
def test_bn_eval_coeffs_and_group(Cc):
    """gcc_bn_eval_coeffs and gcc_bn_eval_coeffs_group (one item with a conv bias, one without running statistics): fp32 formulas,
    1 / sqrtf(var + eps) within 3 ulps, one rounding per further operation"""
    ops = _ops()
    from gcc_amd import _lib
    g = torch.Generator().manual_seed(Cc)
    gamma, beta, rm, bias = (torch.randn(Cc, generator=g) for _ in range(4))
    rv = torch.rand(Cc, generator=g) * 2
    rv[0] = 0.0
    eps = 1e-5
    dev = [t.to(DEV) for t in (gamma, beta, rm, rv, bias)]
    st = ops.BNState(Cc, DEV)
    ops.bn_eval_coeffs(dev[0], dev[1], dev[2], dev[3], st, eps=eps)
    e32 = float(torch.tensor(eps, dtype=torch.float32))
    r = 1.0 / torch.sqrt(rv.double() + e32)
    sc = gamma.double() * r
    torch.cuda.synchronize()
    res = dict(scale=within(st.scale.cpu(), sc, 5 * T.U24 * sc.abs(), 'eval scale'),
               shift=within(st.shift.cpu(), beta.double() - rm.double() * sc, 7 * T.U24 * (beta.double().abs() + (rm.double() * sc).abs()), 'eval shift'),
               rstd=within(st.rstd.cpu(), r, 4 * T.U24 * r, 'eval rstd'))
    assert torch.equal(st.mean.cpu(), rm)
    out = torch.full((4, Cc), SENT, device=DEV)
    items = (_lib.bn_eval_item_t * 2)()
    items[0] = _lib.bn_eval_item_t(_p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]), _p(dev[4]), out[0].data_ptr(), out[1].data_ptr(), Cc, eps)
    items[1] = _lib.bn_eval_item_t(None, None, None, None, _p(dev[4]), out[2].data_ptr(), out[3].data_ptr(), Cc, eps)
    tab = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(DEV)
    ops.check(ops.lib().gcc_bn_eval_coeffs_group(tab.data_ptr(), 2, ops.stream()), 'gcc_bn_eval_coeffs_group')
    torch.cuda.synchronize()
    o = out.cpu()
    res['g_scale'] = within(o[0], sc, 5 * T.U24 * sc.abs(), 'group scale')
    sh = beta.double() + (bias.double() - rm.double()) * sc
    res['g_shift'] = within(o[1], sh, 8 * T.U24 * (beta.double().abs() + ((bias.double() - rm.double()) * sc).abs()), 'group shift')
    assert torch.equal(o[2], torch.ones(Cc)) and torch.equal(o[3], bias)
    report('eval_coeffs', (Cc,), **res)


@pytest.mark.parametrize('G,P,Cc', [(2, 48, 12), (3, 561, 3), (2, 4096, 120), (2, 256, 264)])
def test_channel_stats_window_into_in_finalize(G, P, Cc):
    """gcc_channel_stats on a channel window (non-zero off) fed to gcc_in_finalize against float64 statistics of the same bf16
    data: fp32 partial rows, a lane's pixels plus the LDS fold as the chain"""
    ops = _ops()
    d = T.norm_inputs(P, Cc, 5000 + P + Cc, G)
    x = Win((G, P, Cc), 16, 8, d['x'], pad=0.0)
    tiles = ops.lib().gcc_channel_stats_tiles(P, Cc)
    stats = torch.empty((G, tiles, 2, Cc), dtype=torch.float32, device=DEV)
    ops.check(ops.lib().gcc_channel_stats(x.ptr, x.ld, x.off, Cc, P, G, stats.data_ptr(), ops.stream()), 'gcc_channel_stats')
    st = ops.INState(G, Cc, DEV)
    ops.in_finalize(stats, P, st)
    torch.cuda.synchronize()
    x.check('channel_stats input')
    PPB = T.layout(Cc)[2]
    n = -(-P // (tiles * PPB)) + PPB + 1
    xd = d['x']
    m = xd.mean(1)
    var = (xd - m[:, None]).pow(2).mean(1)
    r = 1.0 / torch.sqrt(var + float(torch.tensor(1e-5, dtype=torch.float32)))
    dm = n * T.U24 * xd.abs().mean(1) + T.U24 * m.abs()
    dvar = n * T.U24 * (xd * xd).mean(1) + 2 * m.abs() * dm
    dr = 0.5 * (var + 1e-5 - dvar).clamp_min(5e-6) ** -1.5 * dvar + T.U24 * r
    what = 'channel_stats %dx%dx%d' % (G, P, Cc)
    report('channel_stats', (G, P, Cc), mean=within(st.mean.cpu(), m, dm, what + ' mean'), rstd=within(st.rstd.cpu(), r, dr, what + ' rstd'))


# ---- D: gcc_inorm_fwd / gcc_inorm_bwd ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [1, 0])
@pytest.mark.parametrize('G,Cc,H,W', [(2, 12, 8, 6), (3, 3, 33, 17), (2, 120, 64, 64), (2, 264, 16, 16)])
def test_inorm_fwd_bwd(G, Cc, H, W, grid):
    """InstanceNorm forward (statistics in the launch; with a residual) and backward (y given, in place over the gradient) in
    windows, per element; grid: the plane split over workgroups that exchange their sums in the launch, or the slab kernels"""
    ops = _ops()
    from gcc_amd import _lib
    P = H * W
    d = T.norm_inputs(P, Cc, 6000 + P + Cc, G, affine=False)
    cus = min(torch.cuda.get_device_properties(0).multi_processor_count, 256)
    print('PLAN inorm %dx%dx%d on %d CUs: forward %r' % (G, P, Cc, cus, T.chain_grid(P, Cc, cus=max(1, cus // G), px=8)[1]))

    def win(vals, pad=0.0):
        w = Win((G, P, Cc), 8, 8, vals, pad=pad)
        w.view = w.base.view(G, H, W, w.ld).permute(0, 3, 1, 2)[:, w.off:w.off + Cc]
        return w
    x, res, y, g1, dx = win(d['x']), win(d['g2']), win(None), win(d['g1']), win(None)
    st = ops.INState(G, Cc, DEV)
    ops.lib().gcc_set_option(_lib.OPT_INORM_GRID, grid)
    try:
        for _ in range(2):         # the second call finds the first one's partials in the workspace
            ops.inorm_fwd(x.view, y.view, st, act=T.ACT_RELU, residual=res.view)
        torch.cuda.synchronize()
        # float64 statistics of the same data; the chain: every pixel of the plane in one lane at the worst
        xd = d['x']
        m = xd.mean(1, keepdim=True)
        var = (xd - m).pow(2).mean(1, keepdim=True)
        e32 = float(torch.tensor(1e-5, dtype=torch.float32))
        r = 1.0 / torch.sqrt(var + e32)
        n = max(T.chain_grid(P, Cc, cus=max(1, cus // G), px=8)[0], -(-P // 128) + 10)
        dm = n * T.U24 * xd.abs().mean(1, keepdim=True) + T.U24 * m.abs()
        dvar = n * T.U24 * (xd * xd).mean(1, keepdim=True) + 2 * m.abs() * dm
        dr = 0.5 * (var + e32 - dvar).clamp_min(e32 / 2) ** -1.5 * dvar + T.U24 * r
        what = 'inorm %dx%dx%d grid %d' % (G, P, Cc, grid)
        ratios = dict(mean=within(st.mean.cpu()[:, None], m, dm, what + ' mean'), rstd=within(st.rstd.cpu()[:, None], r, dr, what + ' rstd'))
        # the normalisation against float64 on the statistics the kernel stored (its scale / shift)
        sc, sf = st.scale.cpu().reshape(G, 1, Cc), st.shift.cpu().reshape(G, 1, Cc)
        y_ref, _, M, _ = T.fwd_math(torch.float64, xd, sc, sf, act=T.ACT_RELU, res=d['g2'])
        y.check(what + ' y')
        ratios['y'] = within(y.get(), y_ref, T.fwd_bound(y_ref, M, T.ACT_RELU), what + ' y')
        # backward: y of a residual-free forward as the saved output
        ysave = win(T.rb64(T.fwd_math(torch.float64, xd, sc, sf, act=T.ACT_RELU)[0]))
        ops.inorm_bwd(x.view, ysave.view, g1.view, dx.view, st, act=T.ACT_RELU)
        torch.cuda.synchronize()
        ref = T.bwd_ref(xd, ysave.get(), d['g1'], n_chain=n, mean=st.mean.cpu().reshape(G, 1, Cc), rstd=st.rstd.cpu().reshape(G, 1, Cc),
                        bn=True, act=T.ACT_RELU)
        T.strong_gradient(ref, what)
        dx.check(what + ' dx')
        ratios['dx'] = within(dx.get(), ref['dx'][0], ref['dx'][1], what + ' dx')
        ops.inorm_bwd(x.view, ysave.view, g1.view, g1.view, st, act=T.ACT_RELU)
        torch.cuda.synchronize()
        assert torch.equal(g1.get(), dx.get())
        g1.check(what + ' in place')
        assert ops.lib().gcc_device_error(0) == 0
    finally:
        ops.lib().gcc_set_option(_lib.OPT_INORM_GRID, -1)
    report('inorm_grid%d' % grid, (G, Cc, H, W), **ratios)
