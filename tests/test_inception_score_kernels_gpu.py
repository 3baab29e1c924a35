"""gcc_is_logits and gcc_is_split_scores (gcc_amd/csrc/inception_score.hip): the classifier head of the Inception network and
the per-split Inception Scores, in f64, in chunks of rows.

Exact regime: integer-valued X, W and b make every product and partial sum of a logit's chain an integer below 2^53 (asserted
per case), so the logits must equal the int64 product bit for bit -- a ragged edge read past its operand, a bias dropped or a
row taken from the wrong chunk changes them.  One-hot and uniform regimes: probabilities that are exactly 0 or 1, or all equal,
give scores known in closed form (K, 1): the 0 log 0 case.  Real-valued regime: the float64 numpy restatement of
tests/_inception_score.py and the bound derived there from d, C, n, the magnitudes of the case and 2^-53.

Chunking: the implemented contract is BIT-IDENTICAL -- a logit's chain does not know its chunk, a row's sums are fixed by C, and a
split's sums over rows are one chain in row order that a chunk edge only interrupts -- and that is what is asserted."""
import math

import numpy as np
import pytest
import torch

from . import _inception_score as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3            # include/gcc_hip.h GCC_ERR_*
SHAPES = ((5, 3, 2), (130, 17, 129), (33, 2048, 1008), (150, 40, 257))          # (n, d, C)
CHUNKS = (0, 64)


def _dev(a, f64, pad=0, extra_rows=0):
    """the rows of `a` on the device as fp32 / f64 with row stride d + pad; the gap and `extra_rows` rows after the last hold NaN"""
    a = np.asarray(a, dtype=np.float64)
    rows, d = a.shape
    buf = torch.full((rows + extra_rows, d + pad), float('nan'), dtype=torch.float64 if f64 else torch.float32, device=DEV)
    buf[:rows, :d] = torch.from_numpy(a).to(DEV)
    return buf[:rows, :d]


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _logits(X, W, b, chunk=0):
    from gcc_amd import ops
    return ops.is_logits(X, _f32(W), _f32(b), chunk=chunk).cpu().numpy()


def _scores(X, W, b, splits, chunk=0):
    from gcc_amd import ops
    return ops.inception_split_scores(X, _f32(W), _f32(b), splits=splits, chunk=chunk).cpu().numpy()


def _check(got, ref, bound, what):
    err = np.abs(got - ref)
    print('%s: scores %.6g .. %.6g, worst err %.3g, bound %.3g, err / bound %.3g'
          % (what, ref.min(), ref.max(), err.max(), bound.max(), float((err / bound).max())))
    assert got.dtype == np.float64 and np.isfinite(got).all() and (err <= bound).all(), what


# ---- exact logits ----------------------------------------------------------------------------------------------------------------
def _int_case(n, d, C):
    rng = np.random.RandomState(n * 131 + d * 17 + C)
    X = rng.randint(-4, 5, (n, d)).astype(np.float64)
    W = rng.randint(-3, 4, (C, d)).astype(np.float64)
    b = rng.randint(-50, 51, C).astype(np.float64)
    X[0, :], X[-1, :] = 4, -4                      # the extremes meet: the budget is the case's, not the average's
    W[0, :], W[-1, :] = 3, -3
    return X, W, b


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('f64', (0, 1), ids=('fp32', 'f64'))
@pytest.mark.parametrize('chunk', CHUNKS)
def test_integer_operands_give_the_int64_product_exactly(shape, f64, chunk):
    n, d, C = shape
    X, W, b = _int_case(n, d, C)
    want, budget = R.logits_int(X, W, b)
    assert d * 12 + np.abs(b).max() == budget < 2 ** 53
    assert int(np.abs(want).max()) >= d * 12 - 50           # the extreme rows do meet
    got = _logits(_dev(X, f64, pad=3, extra_rows=2), W, b, chunk)
    _same_bits(got, want.astype(np.float64), 'strided rows, NaN around them')
    _same_bits(_logits(_dev(X, f64), W, b, chunk), want.astype(np.float64), 'contiguous rows')


@pytest.mark.parametrize('d, C', ((17, 129), (2048, 1008)))
def test_a_row_alone_has_the_bits_it_has_in_its_set(d, C):
    rng = np.random.RandomState(d + C)
    X = rng.standard_normal((130, d)).astype(np.float32)
    W = (rng.standard_normal((C, d)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(C) * 0.1).astype(np.float32)
    Xd = _f32(X)
    whole = _logits(Xd[0:130], W, b)
    alone = _logits(Xd[7:8], W, b)
    assert alone.shape == (1, C) and np.isfinite(whole).all() and np.abs(whole).max() > 0
    _same_bits(alone[0], whole[7], 'row 7 alone')
    _same_bits(_logits(Xd[0:130], W, b, chunk=5), whole, 'chunks of 5 rows')
    ref, A = R.logits_ref(X, W, b)
    err = np.abs(whole - ref).max()
    print('logits %d x %d x %d: worst err %.3g, bound %.3g' % (130, d, C, err, 2 * (d + 1) * R.U53 * A))
    assert err <= 2 * (d + 1) * R.U53 * A * 1.001           # kernel and reference, (d + 1) u A each


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', (2, 8))
@pytest.mark.parametrize('chunk', CHUNKS + (5,))
def test_one_hot_probabilities_give_the_number_of_classes_hit(K, chunk):
    """X rows are unit vectors, W[c][k] = 800 where class c is the k-th class hit: a logit is 805 or 5, exactly, and exp(-800)
    is exactly 0, so every p is 0 or 1 and KL = log K: the 0 log 0 terms must add 0, not NaN"""
    C, S, reps = 129, 3, 2
    n = S * K * reps
    classes = [(k * 37 + 5) % C for k in range(K)]
    assert len(set(classes)) == K and math.exp(-800.0) == 0.0
    X = np.zeros((n, K))
    X[np.arange(n), np.arange(n) % K] = 1.0              # every split of K * reps rows hits each class reps times
    W = np.zeros((C, K))
    W[classes, np.arange(K)] = 800.0
    b = np.full(C, 5.0)
    Z, budget = R.logits_int(X, W, b)
    assert budget < 2 ** 53 and sorted(set(Z.ravel().tolist())) == [5, 805]
    Xd = _dev(X, 0, pad=1, extra_rows=1)
    _same_bits(_logits(Xd, W, b, chunk), Z.astype(np.float64), 'the logits are exact')
    ref = R.scores_ref(Z, S)
    bound = R.score_bound(n, K, C, 805.0, Z, ref)
    assert np.abs(ref - K).max() <= bound.max()             # the restatement knows the closed form too
    got = _scores(Xd, W, b, S, chunk)
    _check(got, np.full(S, float(K)), bound, 'one-hot, K = %d, chunk %d' % (K, chunk))


def test_equal_logits_give_a_score_of_one():
    n, d, C, S = 20, 5, 257, 4
    X = np.random.RandomState(1).standard_normal((n, d)).astype(np.float32)
    W, b = np.zeros((C, d)), np.full(C, 3.0)
    Z, A = R.logits_ref(X, W, b)
    assert (Z == 3.0).all()
    ref = R.scores_ref(Z, S)
    bound = R.score_bound(n, d, C, A, Z, ref)
    assert np.abs(ref - 1.0).max() <= bound.max()
    _check(_scores(_f32(X), W, b, S), np.ones(S), bound, 'uniform')


# ---- real-valued, against the float64 restatement --------------------------------------------------------------------------------
ROWS = ((150, 1), (150, 10), (151, 7), (10, 10))          # (n, splits): uneven splits; the smallest has one row


def _real_case(n, d, C, spread=None):
    rng = np.random.RandomState(7 * n + 3 * d + C)
    X = rng.standard_normal((n, d)).astype(np.float32)
    W = rng.standard_normal((C, d)) * 0.05
    b = (rng.standard_normal(C) * 0.1).astype(np.float32)
    if spread is not None:                                  # the logits reach +-spread
        W = W * (spread / np.abs(X.astype(np.float64) @ W.T).max())
    return X, W.astype(np.float32), b


_REFS = {}


def _reference(n, d, C, splits, spread=None):
    """(X, W, b, reference scores, bound) of a case, computed once per session"""
    key = (n, d, C, splits, spread)
    if key not in _REFS:
        X, W, b = _real_case(n, d, C, spread)
        Z, A = R.logits_ref(X, W, b)
        ref = R.scores_ref(Z, splits)
        _REFS[key] = (X, W, b, ref, R.score_bound(n, d, C, A, Z, ref), float(np.abs(Z).max()))
    return _REFS[key]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s[1:])))
@pytest.mark.parametrize('rows', ROWS, ids=lambda r: '%dr%ds' % r)
def test_seeded_features_against_the_float64_restatement(shape, rows):
    (_, d, C), (n, splits) = shape, rows
    X, W, b, ref, bound, _ = _reference(n, d, C, splits)
    _check(_scores(_f32(X), W, b, splits), ref, bound, '%d x %d x %d over %d splits' % (n, d, C, splits))
    if (n, splits) == (151, 7):                             # f64 rows, strided, and a chunk edge inside the splits
        got = _scores(_dev(X, 1, pad=5, extra_rows=3), W, b, splits, chunk=64)
        _check(got, ref, bound, 'f64 strided rows, chunk 64')


@pytest.mark.parametrize('shape', SHAPES[1:], ids=lambda s: 'x'.join(map(str, s[1:])))
def test_logits_spread_over_sixty_either_way(shape):
    _, d, C = shape
    X, W, b, ref, bound, zmax = _reference(150, d, C, 10, spread=60.0)
    assert 59.0 < zmax < 61.0
    _check(_scores(_f32(X), W, b, 10), ref, bound, 'spread 60, %d x %d' % (d, C))


# ---- chunks, repeats, refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', (SHAPES[1], SHAPES[2]), ids=lambda s: 'x'.join(map(str, s[1:])))
def test_chunking_does_not_move_a_bit(shape):
    """n = 150, 10 splits: split edges at 15, 30, ..., chunk edges at 64 and 128 -- a split edge inside a chunk and a chunk edge
    inside a split.  The contract implemented is the bit-identical one (see the module's text)."""
    _, d, C = shape
    X, W, b, ref, bound, _ = _reference(150, d, C, 10)
    Xd = _f32(X)
    base = _scores(Xd, W, b, 10, chunk=0)
    _check(base, ref, bound, 'chunk 0')
    for chunk in (64, 7, 150, 1000):
        _same_bits(_scores(Xd, W, b, 10, chunk=chunk), base, 'chunk %d' % chunk)
    _same_bits(_scores(Xd, W, b, 10), base, 'a second run')                     # determinism
    _same_bits(_scores(Xd.double(), W, b, 10, chunk=64), base, 'f64 copies of the fp32 rows')


def test_bad_arguments_return_their_code_and_launch_nothing():
    from gcc_amd import _lib, ops
    L = ops.lib()
    n, d, C, S = 12, 6, 5, 3
    X = torch.ones((n, d), dtype=torch.float32, device=DEV)
    W = torch.zeros((C, d), dtype=torch.float32, device=DEV)
    b = torch.zeros(C, dtype=torch.float32, device=DEV)
    out = torch.full((S,), -7.0, dtype=torch.float64, device=DEV)
    Z = torch.full((n, C), -7.0, dtype=torch.float64, device=DEV)
    need = L.gcc_is_workspace(C, S, 0)
    assert need == (_lib.IS_CHUNK * C + _lib.IS_CHUNK + S * C + S) * 8
    assert L.gcc_is_workspace(C, S, 4) == (4 * C + 4 + S * C + S) * 8 == ops.is_workspace_bytes(C, S, 4)
    assert L.gcc_is_workspace(C, S, 0) == L.gcc_is_workspace(C, S, _lib.IS_CHUNK)          # whatever n is: it is no argument
    assert L.gcc_is_workspace(1, S, 0) == L.gcc_is_workspace(C, 0, 0) == L.gcc_is_workspace(C, S, -1) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()

    def score(x=X.data_ptr(), ldx=d, n_=n, d_=d, w=W.data_ptr(), b_=b.data_ptr(), C_=C, S_=S, chunk=0, o=out.data_ptr(),
              ws_=ws.data_ptr(), wb=need):
        return L.gcc_is_split_scores(x, 0, ldx, n_, d_, w, b_, C_, S_, chunk, o, ws_, wb, ops.stream())

    def logits(x=X.data_ptr(), ldx=d, n_=n, d_=d, w=W.data_ptr(), b_=b.data_ptr(), C_=C, chunk=0, z=Z.data_ptr()):
        return L.gcc_is_logits(x, 0, ldx, n_, d_, w, b_, C_, chunk, z, ops.stream())
    before = L.gcc_launch_count(0)
    for what, kw, code in (('n < splits', dict(S_=n + 1), BAD_ARG), ('splits = 0', dict(S_=0), BAD_ARG), ('C = 1', dict(C_=1), BAD_ARG),
                           ('a workspace one byte short', dict(wb=need - 1), WORKSPACE),
                           ('a forced chunk\'s workspace one byte short', dict(chunk=4, wb=L.gcc_is_workspace(C, S, 4) - 1), WORKSPACE),
                           ('X NULL', dict(x=None), BAD_ARG), ('W NULL', dict(w=None), BAD_ARG), ('b NULL', dict(b_=None), BAD_ARG),
                           ('scores NULL', dict(o=None), BAD_ARG), ('ws NULL', dict(ws_=None), BAD_ARG), ('ldx < d', dict(ldx=d - 1), BAD_ARG),
                           ('n = 0', dict(n_=0), BAD_ARG), ('d = 0', dict(d_=0), BAD_ARG), ('chunk < 0', dict(chunk=-1), BAD_ARG)):
        assert score(**kw) == code, what
    for what, kw in (('C = 1', dict(C_=1)), ('Z NULL', dict(z=None)), ('X NULL', dict(x=None)), ('n = 0', dict(n_=0)),
                     ('ldx < d', dict(ldx=d - 1)), ('chunk < 0', dict(chunk=-1))):
        assert logits(**kw) == BAD_ARG, what
    assert L.gcc_launch_count(0) == before
    torch.cuda.synchronize()
    assert float(out.min()) == -7.0 == float(Z.min())
    assert score() == 0 and L.gcc_launch_count(0) == before + 4               # one chunk: three launches, and the last
    assert score(chunk=5, wb=L.gcc_is_workspace(C, S, 5)) == 0 and L.gcc_launch_count(0) == before + 4 + 3 * 3 + 1
    assert (out.cpu() - 1.0).abs().max() < 1e-12                               # equal logits: every score is 1
    assert logits(chunk=5) == 0 and L.gcc_launch_count(0) == before + 14 + 3
    assert (Z == 0.0).all()


def test_wrappers_refuse_what_they_cannot_pass_on():
    from gcc_amd import ops
    from gcc_amd._lib import GccError
    X = torch.ones((7, 6), dtype=torch.float32, device=DEV)
    W = torch.ones((5, 6), dtype=torch.float32, device=DEV)
    b = torch.ones(5, dtype=torch.float32, device=DEV)
    with pytest.raises(GccError, match='splits = 8'):
        ops.inception_split_scores(X, W, b, splits=8)
    with pytest.raises(GccError, match='splits = 0'):
        ops.inception_split_scores(X, W, b, splits=0)
    with pytest.raises(GccError, match='W must be'):
        ops.inception_split_scores(X, W[:, :5], b)
    with pytest.raises(GccError, match='W must be'):
        ops.is_logits(X, W[:1], b[:1])
    with pytest.raises(GccError, match='W must be'):
        ops.is_logits(X, W.double(), b)
    with pytest.raises(GccError, match='b must be'):
        ops.is_logits(X, W, b[:4])
    with pytest.raises(GccError, match='fp32 / f64'):
        ops.is_logits(X.half(), W, b)
    with pytest.raises(GccError, match='chunk = -1'):
        ops.is_logits(X, W, b, chunk=-1)
    with pytest.raises(GccError, match='out must be'):
        ops.is_logits(X, W, b, out=torch.empty((7, 4), dtype=torch.float64, device=DEV))
    out = torch.empty((7, 5), dtype=torch.float64, device=DEV)
    assert ops.is_logits(X, W, b, out=out) is out and (out == 7.0).all()
