"""gcc_kid_poly_sum (gcc_amd/csrc/kid.hip): the sums of the polynomial kernel (x.y / d + 1)^3 over all pairs of rows, without the
Gram matrix.

Exact regime: integer-valued rows and d a power of two make every product, square, cube and partial sum an integer over d^3
below 2^53 (asserted per case: tests/_kid.py poly_exact's budget), so ANY evaluation order gives the exact rational and the
kernel must return it bit for bit -- a diagonal that is not excluded, a tile above the diagonal counted once or thrice, or
garbage from a ragged edge changes it.  Real-valued regime: float64 numpy + math.fsum as the reference and the bound derived in
tests/_kid.py from d, the number of pairs and 2^-53 on sum (|x|.|y| / d + 1)^3."""
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

from . import _kid as K

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3            # include/gcc_hip.h GCC_ERR_*


def _tile():
    from gcc_amd import _lib
    return _lib.KID_TILE, _lib.KID_KSTEP


def _dev(a, f64, pad=0, extra_rows=0):
    """the rows of `a` on the device as fp32 / f64 with row stride d + pad; the gap and `extra_rows` rows after the last hold NaN"""
    a = np.asarray(a, dtype=np.float64)
    rows, d = a.shape
    buf = torch.full((rows + extra_rows, d + pad), float('nan'), dtype=torch.float64 if f64 else torch.float32, device=DEV)
    buf[:rows, :d] = torch.from_numpy(a).to(DEV)
    return buf[:rows, :d]


def _sum(X, Y=None):
    from gcc_amd import ops
    return float(ops.kid_poly_sum(X, Y).cpu()[0])


def _ints(rng, rows, d, lo, hi):
    a = rng.randint(lo, hi + 1, (rows, d)).astype(np.float64)
    a[0, :] = hi                                   # the extremes meet: the budget is the case's, not the average's
    a[-1, :] = lo if rows > 1 else hi
    return a


def _exact(value, want, budget, what):
    assert budget < 2 ** 53, '%s: the case leaves the exact regime (%d >= 2^53)' % (what, budget)
    assert Fraction(float(want)) == want
    print('%s: %r, exact %r, budget 2^%.1f' % (what, value, float(want), np.log2(float(budget))))
    assert np.float64(value).tobytes() == np.float64(float(want)).tobytes(), (what, value, float(want))


# (m, n, d, lo, hi): the issue's shapes and ranges
EXACT_FULL = ((1, 1, 16, -8, 8), (2, 1, 16, -8, 8), (65, 63, 16, -8, 8), (64, 64, 2048, -2, 2), (33, 33, 64, -4, 4))


@pytest.mark.parametrize('case', EXACT_FULL, ids=lambda c: 'x'.join(map(str, c[:3])))
@pytest.mark.parametrize('f64', (0, 1), ids=('fp32', 'f64'))
def test_full_sum_is_the_exact_rational(case, f64):
    m, n, d, lo, hi = case
    rng = np.random.RandomState(m * 131 + n * 17 + d)
    X, Y = _ints(rng, m, d, lo, hi), _ints(rng, n, d, lo, hi)
    want, budget = K.poly_exact(X, Y)
    got = _sum(_dev(X, f64, pad=3, extra_rows=2), _dev(Y, 1 - f64 if d == 64 else f64, pad=1, extra_rows=1))
    _exact(got, want, budget, 'full %dx%dx%d %s' % (m, n, d, 'f64' if f64 else 'fp32'))


def _symmetric_rows():
    T, _ = _tile()
    return (2, 33, 65, 2 * T + 1)


@pytest.mark.parametrize('which', range(4), ids=('m2', 'm33', 'm65', 'above-two-tiles'))
@pytest.mark.parametrize('f64', (0, 1), ids=('fp32', 'f64'))
def test_symmetric_sum_is_the_exact_rational_and_full_minus_diagonal(which, f64):
    m, d = _symmetric_rows()[which], 16
    rng = np.random.RandomState(900 + m)
    X = _ints(rng, m, d, -8, 8)
    want, budget = K.poly_exact(X)
    full, full_budget = K.poly_exact(X, X)
    assert full - K.diag_exact(X) == want
    Xd = _dev(X, f64, pad=5, extra_rows=3)
    sym = _sum(Xd)
    _exact(sym, want, budget, 'symmetric %dx%d' % (m, d))
    both = _sum(Xd, Xd)
    _exact(both, full, full_budget, 'full(X, X) %dx%d' % (m, d))
    assert Fraction(both) - K.diag_exact(X) == Fraction(sym)


def test_symmetric_at_the_other_exact_ranges():
    for m, d, lo, hi in ((64, 2048, -2, 2), (33, 64, -4, 4)):
        X = _ints(np.random.RandomState(m + d), m, d, lo, hi)
        want, budget = K.poly_exact(X)
        _exact(_sum(_dev(X, 0)), want, budget, 'symmetric %dx%d' % (m, d))


# ---- ragged and real-valued ---------------------------------------------------------------------------------------------------
def _real(rng, rows, d, signed):
    a = rng.standard_normal((rows, d)) if signed else np.abs(rng.standard_normal((rows, d))) * 0.6       # pool3 features: >= 0
    return a.astype(np.float32).astype(np.float64)          # representable in either input type


def _check(X, Y, xf, yf, what):
    S, T3, pairs = K.poly_ref(X, Y)
    d = X.shape[1]
    bound = K.poly_bound(d, pairs, T3)
    got = _sum(_dev(X, xf, pad=7, extra_rows=2), None if Y is None else _dev(Y, yf, pad=2, extra_rows=5))
    err = abs(got - S)
    print('%s: %.17g, float64 reference %.17g, err / bound %.3g (bound %.3g relative)' % (what, got, S, err / bound, bound / abs(S)))
    assert np.isfinite(got) and err <= bound, (what, got, S, err, bound)
    # the bound tells a wrong sum from a right one: a single pair more or less is far outside it
    assert bound < 1e-3 * abs(S) / max(pairs, 1)


@pytest.mark.parametrize('signed', (False, True), ids=('nonneg', 'signed'))
def test_sizes_around_the_tile_and_the_k_step(signed):
    T, KS = _tile()
    rng = np.random.RandomState(77 + signed)
    for c, (m, n, d) in enumerate(itertools.product((T - 1, T, T + 1), (T - 1, T, T + 1), (KS - 1, KS, KS + 1))):
        X, Y = _real(rng, m, d, signed), _real(rng, n, d, signed)
        _check(X, Y, c & 1, (c >> 1) & 1, 'full %dx%dx%d' % (m, n, d))
        if n == T:
            _check(X, None, c & 1, 0, 'symmetric %dx%d' % (m, d))


@pytest.mark.parametrize('signed', (False, True), ids=('nonneg', 'signed'))
@pytest.mark.parametrize('case', ((120, 140, 65), (130, 70, 2048), (1, 1, 1), (3, 2, 1)), ids=lambda c: 'x'.join(map(str, c)))
def test_network_widths(case, signed):
    m, n, d = case
    rng = np.random.RandomState(5 + d + signed)
    X, Y = _real(rng, m, d, signed), _real(rng, n, d, signed)
    _check(X, Y, 0, 0, 'full %dx%dx%d' % case)
    _check(X, Y, 1, 0, 'full f64 x fp32 %dx%dx%d' % case)
    if m >= 2:
        _check(X, None, 0, 0, 'symmetric %dx%d' % (m, d))


def test_two_runs_give_the_same_bits():
    from gcc_amd import ops
    T, _ = _tile()
    rng = np.random.RandomState(3)
    X, Y = _dev(_real(rng, 3 * T + 5, 65, True), 0, pad=1), _dev(_real(rng, 2 * T + 9, 65, True), 0)
    runs = [(ops.kid_poly_sum(X, Y).cpu(), ops.kid_poly_sum(X).cpu()) for _ in range(2)]
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64))
    assert torch.equal(runs[0][1].view(torch.int64), runs[1][1].view(torch.int64))


def test_bad_arguments_return_their_code_and_launch_nothing():
    from gcc_amd import ops
    L = ops.lib()
    m, n, d = 5, 4, 6
    X = torch.ones((m, d), dtype=torch.float32, device=DEV)
    Y = torch.ones((n, d), dtype=torch.float64, device=DEV)
    out = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    need = L.gcc_kid_workspace(m, n, d)
    ws = torch.empty(max(need, 64), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()

    def call(x=X.data_ptr(), ldx=d, m_=m, y=Y.data_ptr(), ldy=d, n_=n, d_=d, sym=0, o=out.data_ptr(), w=ws.data_ptr(), wb=ws.numel()):
        return L.gcc_kid_poly_sum(x, 0, ldx, m_, y, 1, ldy, n_, d_, sym, o, w, wb, ops.stream())
    before = L.gcc_launch_count(0)
    for what, kw, code in (('X NULL', dict(x=None), BAD_ARG), ('Y NULL', dict(y=None), BAD_ARG), ('out NULL', dict(o=None), BAD_ARG),
                           ('ws NULL', dict(w=None), BAD_ARG), ('ldx < d', dict(ldx=d - 1), BAD_ARG), ('ldy < d', dict(ldy=d - 1), BAD_ARG),
                           ('m = 0', dict(m_=0), BAD_ARG), ('n = 0', dict(n_=0), BAD_ARG), ('d = 0', dict(d_=0), BAD_ARG),
                           ('short workspace', dict(wb=need - 1), WORKSPACE), ('symmetric m = 1', dict(m_=1, sym=1), BAD_ARG),
                           ('symmetric X NULL', dict(x=None, sym=1), BAD_ARG)):
        assert call(**kw) == code, what
    assert L.gcc_launch_count(0) == before
    torch.cuda.synchronize()
    assert float(out.cpu()[0]) == -7.0
    assert call() == 0 and L.gcc_launch_count(0) == before + 2
    assert float(out.cpu()[0]) == m * n * 8.0                 # ones: t = 2
    assert call(sym=1, y=None) == 0                           # Y is X: its own arguments are not read
    assert float(out.cpu()[0]) == m * (m - 1) * 8.0


def test_workspace_is_one_double_per_tile_not_per_pair():
    from gcc_amd import ops
    L = ops.lib()
    T, _ = _tile()
    tiles = lambda r: -(-r // T)
    for m, n in ((1, 1), (T, T), (T + 1, T), (20000, 20000), (20000, 3)):
        for d in (1, 2048):
            assert L.gcc_kid_workspace(m, n, d) == tiles(m) * tiles(n) * 8, (m, n, d)
    big = L.gcc_kid_workspace(20000, 20000, 2048)
    assert big <= 1 << 20 and big * T * T >= 20000 * 20000 * 8 > big * 1000          # 3.2 GB of Gram matrix never exists
    assert L.gcc_kid_workspace(0, 5, 5) == 0 and L.gcc_kid_workspace(5, 5, 0) == 0


def test_wrapper_refuses_what_it_cannot_pass_on():
    from gcc_amd import ops
    from gcc_amd._lib import GccError
    X = torch.ones((4, 6), dtype=torch.float32, device=DEV)
    with pytest.raises(GccError, match='at least 2 rows'):
        ops.kid_poly_sum(X[:1])
    with pytest.raises(GccError, match='against'):
        ops.kid_poly_sum(X, X[:, :5])
    with pytest.raises(GccError, match='fp32 / f64'):
        ops.kid_poly_sum(X.half())
    # columns that are not contiguous are copied, not misread
    Xt = torch.arange(24, dtype=torch.float32, device=DEV).reshape(6, 4).t()       # [4, 6], stride (1, 4)
    want, T3, pairs = K.poly_ref(Xt.cpu().numpy())
    assert abs(float(ops.kid_poly_sum(Xt).cpu()[0]) - want) <= K.poly_bound(6, pairs, T3)
