"""The per-element bounds of tests/test_norm_kernels_gpu.py, checked without a GPU in both directions: an emulation of the
norm_act.hip kernels' arithmetic (fp32 chain, bf16 where a kernel rounds, double folds, the dz round trip of the three-launch
route; tests/_perelem.py fwd_math / bwd_emul) passes every bound of the forward and backward cases at every case's shape, and
deliberately wrong formulas are rejected at them.  Nothing here runs a kernel: it shows what the comparison can and cannot see.

Shapes left out of a rejection, because the wrong formula computes the right thing there: a single pixel for the BatchNorm
projection terms (xhat = 0 and dz - mean(dz) = 0: dx is zero whatever is dropped) and for the mask index (pixel 0 has the same
counter under any stride)."""
import pytest
import torch

from tests import _perelem as T
from tests._perelem import within


def test_bf16_unit_roundoff():
    """why the bf16 term of every bound is 2^-8 |ref| and not 2^-9 |ref|: the correctly rounded bf16 of an exact value is up to
    2^-8 / (1 + 2^-8) of it away (no kernel involved: 1 + 2^-8 + 2^-20 rounds to 1 + 2^-7)"""
    v = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -20, 0.274398136], dtype=torch.float64)
    rel = (T.rb64(v) - v).abs() / v
    assert bool((rel > 2.0 ** -9).all()) and bool((rel <= T.RND_BF16).all())
    g = torch.rand(1 << 16, generator=torch.Generator().manual_seed(0), dtype=torch.float64) + 0.5
    assert float(((T.rb64(g) - g).abs() / g).max()) <= T.RND_BF16


def _fwd_cases():
    for ci, C in enumerate(T.FWD_C):
        for pi, P in enumerate(T.fwd_pixels(C)):
            yield P, C, T.FWD_OPTIONS[(ci + pi) % len(T.FWD_OPTIONS)]
    yield 8192 + 3, 520, T.FWD_OPTIONS[1]           # above the 2048-workgroup cap


@pytest.mark.parametrize('C', T.FWD_C)
def test_forward_emulation_passes(C):
    for P, Cc, opt in _fwd_cases():
        if Cc != C:
            continue
        d, kw = T.fwd_case(P, C, opt, seed=1000 + C + P)
        y, y2, M, M2 = T.fwd_math(torch.float64, d['x'], **kw)
        ey, ey2, _, _ = T.fwd_math(torch.float32, d['x'], **kw)
        r1 = within(T.rb64(ey), y, T.fwd_bound(y, M, kw['act']), 'y %dx%d' % (P, C))
        r2 = within(T.rb64(ey2), y2, T.fwd_bound(y2, M2, kw['act2']), 'y2 %dx%d' % (P, C))
        assert max(r1, r2) <= 1.0


def _rejected(got, ref, bound, what):
    with pytest.raises(AssertionError):
        within(got, ref, bound, what)


@pytest.mark.parametrize('C', T.FWD_C)
def test_forward_wrong_formulas_are_rejected(C):
    for P in T.fwd_pixels(C):
        # the gate applied after the activation when it was asked for before: visible through tanh (a rectifier commutes with a
        # non-negative gate)
        opt = dict(gate=True, act=T.ACT_TANH)
        d, kw = T.fwd_case(P, C, opt, seed=2000 + C + P)
        kw['gate'] = torch.where(kw['gate'] == 0, torch.tensor(0.25), kw['gate'])       # (a zero gate gives zero either way)
        y, _, M, _ = T.fwd_math(torch.float64, d['x'], **kw)
        bad = T.fwd_math(torch.float32, d['x'], wrong='gate_order', **kw)[0]
        if C > 1 or float(kw['gate'][0]) != 1.0:
            _rejected(T.rb64(bad), y, T.fwd_bound(y, M, kw['act']), 'gate order %dx%d' % (P, C))
        # the dropout mask indexed by pix * ld + c
        if P > 1:
            opt = dict(act=T.ACT_LRELU, drop=0.5)
            d, kw = T.fwd_case(P, C, opt, seed=2000 + C + P)
            y, _, M, _ = T.fwd_math(torch.float64, d['x'], **kw)
            kw['keep'] = T.keep_mask(2000 + C + P, P, C, 0.5, stride=((C + 7) & ~7) + 8)
            bad = T.fwd_math(torch.float32, d['x'], **kw)[0]
            assert not torch.equal(bad == 0, y == 0)
            _rejected(T.rb64(bad), y, T.fwd_bound(y, M, kw['act']), 'mask stride %dx%d' % (P, C))


def _bwd_cases():
    for P, C, _, opt in T.BWD_THREE:
        yield 'three', P, C, opt
    for P, C, opt in T.BWD_SMALL:
        yield 'small', P, C, opt
    for P, C, opt in T.BWD_GRID:
        yield 'grid', P, C, opt


def _chain(route, P, C):
    return T.chain_three(P, C) if route == 'three' else (T.CHAIN_SMALL if route == 'small' else T.chain_grid(P, C)[0])


def _check(route, P, C, opt, seed, wrong=None, bn_eval=False):
    d, y, kw = T.bwd_case(P, C, opt, seed)
    ref = T.bwd_ref(d['x'], y, d['g1'], bn_eval=bn_eval, n_chain=_chain(route, P, C), three=route == 'three', **kw)
    if kw['bn'] and not bn_eval and P >= 64:
        T.strong_gradient(ref, '%s %dx%d' % (route, P, C))
    # the reference alone stays under the cap on elements whose recomputed sign is open
    assert float(ref['open'].double().mean()) <= 1e-3
    got = T.bwd_emul(route, d['x'], y, d['g1'], bn_eval=bn_eval, wrong=wrong, **kw)
    keep = ~ref['open']
    worst = within(torch.where(keep, got['dx'], ref['dx'][0]), ref['dx'][0], ref['dx'][1], 'dx %s %dx%d' % (route, P, C))
    if route != 'act':
        for name in ('dbeta', 'dgamma') + (('dalpha',) if kw['gated'] else ()):
            worst = max(worst, within(got[name][None], ref[name][0], ref[name][1], '%s %s %dx%d' % (name, route, P, C)))
    return worst


@pytest.mark.parametrize('route,P,C,opt', list(_bwd_cases()))
def test_backward_emulation_passes(route, P, C, opt):
    assert _check(route, P, C, opt, seed=3000 + P + C) <= 1.0


@pytest.mark.parametrize('P,C,opt', T.BWD_ACT)
def test_activation_backward_emulation_passes(P, C, opt):
    assert _check('act', P, C, dict(opt, bn=False), seed=3500 + P + C) <= 1.0


@pytest.mark.parametrize('P,C,blocks,opt', [c for c in T.BWD_THREE if not c[3].get('after')][:3] + [T.BWD_THREE[-1]])
def test_eval_mode_emulation_passes(P, C, blocks, opt):
    assert _check('three', P, C, opt, seed=3700 + P + C, bn_eval=True) <= 1.0


@pytest.mark.parametrize('wrong', ['no_xhat', 'no_mean', 'neither', 'miss_last'])
@pytest.mark.parametrize('route,P,C,opt', [c for c in _bwd_cases() if c[1] > 1])
def test_wrong_batchnorm_backward_is_rejected(route, P, C, opt, wrong):
    with pytest.raises(AssertionError):
        _check(route, P, C, opt, seed=3000 + P + C, wrong=wrong)


@pytest.mark.parametrize('P,C,opt', [c for c in T.BWD_ACT if c[2]['in_act'] != T.ACT_NONE])
def test_in_act_derivative_on_the_wrong_tensor_is_rejected(P, C, opt):
    with pytest.raises(AssertionError):
        _check('act', P, C, dict(opt, bn=False), seed=3500 + P + C, wrong='in_act_tensor')


def test_the_max_norm_check_misses_what_the_bound_sees():
    """the reason for this file: at 9216 pixels the suite's 2e-2 * max|dx| lets a backward without either projection term pass
    on zero-mean gradients, where the per-element bound on the strong gradient of norm_inputs rejects it"""
    P, C = 9216, 40
    d, y, kw = T.bwd_case(P, C, dict(act=T.ACT_LRELU), seed=11)
    g = T.rb64(torch.randn(1, P, C, generator=torch.Generator().manual_seed(5)))
    ref = T.bwd_ref(d['x'], y, g, n_chain=T.chain_three(P, C), three=True, **kw)
    bad = T.bwd_emul('three', d['x'], y, g, wrong='neither', **kw)['dx']
    assert float((bad - ref['dx'][0]).abs().max()) <= 2e-2 * float(ref['dx'][0].abs().max())
    with pytest.raises(AssertionError):
        _check('three', P, C, dict(act=T.ACT_LRELU), seed=11, wrong='neither')
