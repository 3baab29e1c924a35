"""gcc_prdc_kth_dist and gcc_prdc_ball_count (gcc_amd/csrc/prdc.hip): k-th nearest-neighbour squared distances and
ball-membership counts without the m x n matrix of distances.

Exact regime: integer-valued rows make every difference, square and partial sum an integer below 2^53 (asserted per case:
tests/_prdc.py's budget), so the kernels must return the integer reference bit for bit -- a diagonal that is not excluded, a tie
at the radius decided the wrong way, a duplicate row dropped or garbage from a ragged edge changes it.  Real-valued regime:
float64 numpy (direct differences, np.partition) as the reference and the bound derived in tests/_prdc.py from d and 2^-53; the
counts are compared exactly, after asserting that the reference's own margin at every pair exceeds both bounds."""
import itertools

import numpy as np
import pytest
import torch

from . import _prdc as P

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3            # include/gcc_hip.h GCC_ERR_*


def _consts():
    from gcc_amd import _lib
    return _lib.PRDC_TILE, _lib.PRDC_COL_TILE, _lib.PRDC_KSTEP, _lib.PRDC_MAX_K


def _dev(a, f64, pad=0, extra_rows=0):
    """the rows of `a` on the device as fp32 / f64 with row stride d + pad; the gap and `extra_rows` rows after the last hold NaN"""
    a = np.asarray(a, dtype=np.float64)
    rows, d = a.shape
    buf = torch.full((rows + extra_rows, d + pad), float('nan'), dtype=torch.float64 if f64 else torch.float32, device=DEV)
    buf[:rows, :d] = torch.from_numpy(a).to(DEV)
    return buf[:rows, :d]


TILES = ('small', 'large')


def _tile(which):
    """the tile side to force: include/gcc_hip.h GCC_PRDC_SMALL_TILE / GCC_PRDC_TILE (rows and columns alike)"""
    from gcc_amd import _lib
    assert _lib.PRDC_COL_TILE == _lib.PRDC_TILE
    return {'small': _lib.PRDC_SMALL_TILE, 'large': _lib.PRDC_TILE}[which]


def _kth(X, Y=None, k=5, chunks=0, tile=0):
    from gcc_amd import ops
    return ops.prdc_kth_dist(X, Y, k=k, chunks=chunks, tile=tile).cpu().numpy()


def _count(Q, C, r2, chunks=0, tile=0):
    from gcc_amd import ops
    r2 = torch.from_numpy(np.ascontiguousarray(r2, dtype=np.float64)).to(DEV)
    return ops.prdc_ball_count(Q, C, r2, chunks=chunks, tile=tile).cpu().numpy()


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


# ---- exact -----------------------------------------------------------------------------------------------------------------------
# (m, n, d, lo, hi): few distinct points (ties and duplicates everywhere), a lattice with some duplicates, a ragged tile pair,
# the network's width
EXACT = ((40, 33, 2, 0, 3), (150, 140, 3, -2, 2), (129, 131, 17, -8, 8), (33, 40, 2048, -2, 2))


def _ints(rng, rows, d, lo, hi):
    a = rng.randint(lo, hi + 1, (rows, d)).astype(np.float64)
    a[0, :] = hi                                   # the extremes meet: the budget is the case's, not the average's
    a[-1, :] = lo
    return a


@pytest.mark.parametrize('case', EXACT, ids=lambda c: 'x'.join(map(str, c[:3])))
@pytest.mark.parametrize('f64', (0, 1), ids=('fp32', 'f64'))
@pytest.mark.parametrize('which', TILES)
def test_integer_rows_give_the_integer_reference_exactly(case, f64, which):
    m, n, d, lo, hi = case
    tile = _tile(which)
    MAXK = _consts()[3]
    rng = np.random.RandomState(m * 131 + n * 17 + d)
    X, Y = _ints(rng, m, d, lo, hi), _ints(rng, n, d, lo, hi)
    Xd, Yd = _dev(X, f64, pad=3, extra_rows=2), _dev(Y, 1 - f64 if d == 17 else f64, pad=1, extra_rows=1)
    zero_radius = ties = diagonal_matters = 0
    for k in (1, 3, 5, MAXK):
        want, budget = P.kth_int(X, None, k)
        assert budget < 2 ** 53
        _same_bits(_kth(Xd, None, k, tile=tile), want, 'symmetric k = %d' % k)
        D, _ = P.sqdist_int(X, X)
        diagonal_matters += int((np.partition(D, k - 1, axis=1)[:, k - 1] != want).sum())
        zero_radius += int((want == 0).sum())
        cross, budget = P.kth_int(Y, X, k)
        assert budget < 2 ** 53
        _same_bits(_kth(Yd, Xd, k, tile=tile), cross, 'Y against X, k = %d' % k)
        counts, _ = P.ball_int(Y, X, want)
        Dyx, _ = P.sqdist_int(Y, X)
        ties += int((Dyx == want[None, :].astype(np.int64)).sum())
        got = _count(Yd, Xd, want, tile=tile)
        assert got.dtype == np.int32 and np.array_equal(got, counts), 'ball count k = %d' % k
    print('%s: %d radii of 0, %d pairs exactly on a sphere, %d rows whose k-th value the diagonal would change'
          % (case, zero_radius, ties, diagonal_matters))
    assert diagonal_matters > 0                    # leaving the diagonal in changes the answer
    if d <= 3:
        assert ties > 0 and zero_radius > 0        # an exclusive < or a dropped duplicate changes the answer


@pytest.mark.parametrize('f64', (0, 1), ids=('fp32', 'f64'))
def test_k_of_every_other_row_and_of_every_column(f64):
    MAXK = _consts()[3]
    rng = np.random.RandomState(4)
    X = _ints(rng, MAXK + 1, 5, -9, 9)             # symmetric k = m - 1: the farthest other row
    want, _ = P.kth_int(X, None, MAXK)
    D, _ = P.sqdist_int(X, X)
    assert np.array_equal(want, D.max(1))
    _same_bits(_kth(_dev(X, f64, pad=2), None, MAXK), want, 'k = m - 1')
    Y = _ints(rng, MAXK, 5, -9, 9)                 # k = n: the farthest column
    cross, _ = P.kth_int(X, Y, MAXK)
    _same_bits(_kth(_dev(X, f64), _dev(Y, f64, extra_rows=3), MAXK), cross, 'k = n')
    one = _ints(rng, 2, 5, -9, 9)[:1]
    _same_bits(_kth(_dev(X, f64), _dev(one, f64, extra_rows=1), 1), P.kth_int(X, one, 1)[0], 'n = 1')
    dup = np.repeat(_ints(rng, 3, 4, -3, 3), 6, axis=0)          # every row has five copies beside it
    assert np.array_equal(P.kth_int(dup, None, 5)[0], np.zeros(18)) and P.kth_int(dup, None, 6)[0].min() > 0
    _same_bits(_kth(_dev(dup, f64), None, 5), np.zeros(18), 'radius 0')
    _same_bits(_kth(_dev(dup, f64), None, 6), P.kth_int(dup, None, 6)[0], 'one past the copies')
    assert np.array_equal(_count(_dev(dup, f64), _dev(dup, f64), np.zeros(18)), np.full(18, 6))      # D == 0 <= 0 counts


# ---- real-valued, around the tiles -----------------------------------------------------------------------------------------------
def _check_kth(got, ref, d, what):
    bound = P.dist_bound(d, ref)
    err = np.abs(got - ref)
    print('%s: worst err / bound %.3g' % (what, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.isfinite(got).all() and (err <= bound).all(), what


def _check_all(R, F, k, xf, yf, what, tile=0):
    """every use prdc makes of the two kernels, on real rows R and generated rows F"""
    d = R.shape[1]
    Drr, Dff, Drf = P.sqdist(R, R), P.sqdist(F, F), P.sqdist(R, F)           # once: everything below is read off these
    margin = P.margin_of(Drr, Dff, Drf, d, k)
    assert margin > 0, (what, margin)              # the reference itself is decided at every pair: exact counts are owed
    Rd, Fd = _dev(R, xf, pad=7, extra_rows=2), _dev(F, yf, pad=2, extra_rows=5)
    rR, rF = P.kth_of(Drr, k, True), P.kth_of(Dff, k, True)
    _check_kth(_kth(Rd, None, k, tile=tile), rR, d, what + ' radii of R')
    _check_kth(_kth(Fd, None, k, tile=tile), rF, d, what + ' radii of F')
    _check_kth(_kth(Rd, Fd, 1, tile=tile), P.kth_of(Drf, 1, False), d, what + ' nearest F')
    _check_kth(_kth(Fd, Rd, k, tile=tile), P.kth_of(Drf.T, k, False), d, what + ' k-th R of F')
    in_real, in_fake = (Drf <= rR[:, None]).sum(0), (Drf <= rF[None, :]).sum(1)
    assert np.array_equal(_count(Fd, Rd, rR, tile=tile), in_real), what + ' balls of R'
    assert np.array_equal(_count(Rd, Fd, rF, tile=tile), in_fake), what + ' balls of F'
    return in_real, in_fake


def _d_values():
    KS = _consts()[2]
    return (1, KS - 1, KS, KS + 1)


@pytest.mark.parametrize('dn', range(4), ids=('d1', 'below-kstep', 'kstep', 'above-kstep'))
@pytest.mark.parametrize('which', TILES)
def test_sizes_around_the_tiles_and_the_k_step(which, dn):
    T = C = _tile(which)                           # the forced tile: its row side and its column side
    d = _d_values()[dn]
    for c, (n, m) in enumerate(itertools.product((T - 1, T, T + 1), (C - 1, C, C + 1))):
        R, F = P.gaussian_sets(n, m, d)
        _check_all(R, F, 3 if c & 1 else 5, c & 1, (c >> 1) & 1, '%dx%dx%d' % (n, m, d), tile=T)


@pytest.mark.parametrize('case', ((129, 127, 17), (257, 130, 70), (300, 260, 64)), ids=lambda c: 'x'.join(map(str, c)))
def test_gaussian_shapes_have_counts_inside_their_range(case):
    n, m, d = case
    R, F = P.gaussian_sets(n, m, d)
    in_real, in_fake = _check_all(R, F, 5, 0, 0, '%dx%dx%d' % case)
    assert 0 < (in_real > 0).sum() < m and 0 < (in_fake > 0).sum() < n          # all or nothing would not pass


@pytest.mark.parametrize('which', TILES)
def test_network_width(which):
    R, F = P.gaussian_sets(260, 257, 2048)
    _check_all(R, F, 5, 0, 1, '260x257x2048', tile=_tile(which))


# ---- chunking, position, determinism -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', TILES)
def test_every_chunking_gives_the_same_bits(which):
    from gcc_amd import ops
    T = C = tile = _tile(which)
    L = ops.lib()
    n, m, d = 2 * C + 1, T + 3, 20                 # three column tiles, the last one column wide
    R, F = P.gaussian_sets(n, m, d)
    Rd, Fd = _dev(R, 0, pad=1), _dev(F, 0, extra_rows=1)
    tiles = -(-n // C)
    assert tiles == 3
    rR = P.kth_ref(R, None, 5)
    base = (_kth(Fd, Rd, 5, 1, tile), _kth(Rd, None, 5, 1, tile), _kth(Fd, Rd, 1, 1, tile), _count(Fd, Rd, rR, 1, tile))
    _check_kth(base[1], rR, d, 'one chunk')
    assert np.array_equal(base[3], P.ball_ref(F, R, rR))
    for chunks in (2, tiles, 0):
        got = (_kth(Fd, Rd, 5, chunks, tile), _kth(Rd, None, 5, chunks, tile), _kth(Fd, Rd, 1, chunks, tile), _count(Fd, Rd, rR, chunks, tile))
        for a, b in zip(base, got):
            _same_bits(a, b, 'chunks = %d' % chunks)
    # the library's own tile and chunks, and the other tile: the same chain per pair, the same bits
    assert L.gcc_prdc_tile(m, n) in (_tile('small'), _tile('large')) and 1 <= L.gcc_prdc_chunks(m, n) <= -(-n // L.gcc_prdc_tile(m, n))
    for other in (0, _tile('small'), _tile('large')):
        got = (_kth(Fd, Rd, 5, 0, other), _kth(Rd, None, 5, 0, other), _kth(Fd, Rd, 1, 0, other), _count(Fd, Rd, rR, 0, other))
        for a, b in zip(base, got):
            _same_bits(a, b, 'tile = %d' % other)
    # a value the sizes do not admit: its code, no launch
    out = torch.full((m,), -7.0, dtype=torch.float64, device=DEV)
    cnt = torch.full((m,), -7, dtype=torch.int32, device=DEV)
    r2 = torch.from_numpy(rR).to(DEV)
    ws = torch.empty(L.gcc_prdc_workspace(m, n, 5), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    before = L.gcc_launch_count(0)
    for chunks in (tiles + 1, -1, 1000):
        assert L.gcc_prdc_kth_dist(Fd.data_ptr(), 0, Fd.stride(0), m, Rd.data_ptr(), 0, Rd.stride(0), n, d, 0, 5, chunks, tile,
                                   out.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream()) == BAD_ARG
        assert L.gcc_prdc_ball_count(Fd.data_ptr(), 0, Fd.stride(0), m, Rd.data_ptr(), 0, Rd.stride(0), n, d, r2.data_ptr(),
                                     chunks, tile, cnt.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream()) == BAD_ARG
    assert L.gcc_launch_count(0) == before
    torch.cuda.synchronize()
    assert float(out.min()) == -7.0 and int(cnt.min()) == -7
    # the workspace query serves the largest legal chunking
    assert L.gcc_prdc_kth_dist(Fd.data_ptr(), 0, Fd.stride(0), m, Rd.data_ptr(), 0, Rd.stride(0), n, d, 0, 5, tiles, tile,
                               out.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream()) == 0
    _same_bits(out.cpu().numpy(), base[0], 'raw call')


@pytest.mark.parametrize('which', TILES)
def test_outputs_do_not_depend_on_where_the_rows_sit(which):
    T = C = tile = _tile(which)
    n, m, d = C + 40, T + 9, 33
    R, F = P.gaussian_sets(n, m, d)
    rng = np.random.RandomState(9)
    pr, pf = rng.permutation(n), rng.permutation(m)
    Rd, Fd, Rp, Fp = _dev(R, 0), _dev(F, 1, pad=3), _dev(R[pr], 0, pad=5), _dev(F[pf], 1)
    rR = _kth(Rd, None, 5, tile=tile)
    _same_bits(_kth(Rp, None, 5, tile=tile), rR[pr], 'symmetric, rows permuted')
    cross = _kth(Fd, Rd, 3, tile=tile)
    _same_bits(_kth(Fd, Rp, 3, tile=tile), cross, 'columns permuted')
    _same_bits(_kth(Fp, Rd, 3, tile=tile), cross[pf], 'rows permuted')
    counts = _count(Fd, Rd, rR, tile=tile)
    _same_bits(_count(Fd, Rp, rR[pr], tile=tile), counts, 'centres permuted with their radii')
    _same_bits(_count(Fp, Rd, rR, tile=tile), counts[pf], 'queries permuted')
    # D(x, y) == D(y, x) bit for bit: the nearest column of the transposed problem
    _same_bits(np.float64(_kth(Fd, Rd, 1, tile=tile).min()), np.float64(_kth(Rd, Fd, 1, tile=tile).min()), 'symmetry of D')


@pytest.mark.parametrize('which', TILES)
def test_two_runs_give_the_same_bits(which):
    T = C = tile = _tile(which)
    R, F = P.gaussian_sets(3 * C + 5, 2 * T + 9, 65)
    Rd, Fd = _dev(R, 0, pad=1), _dev(F, 0)
    rR = P.kth_ref(R, None, 5)
    runs = [(_kth(Rd, None, 5, tile=tile), _kth(Fd, Rd, 1, tile=tile), _count(Fd, Rd, rR, tile=tile)) for _ in range(2)]
    for a, b in zip(*runs):
        _same_bits(a, b, 'second run')


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_their_code_and_launch_nothing():
    from gcc_amd import ops
    L = ops.lib()
    MAXK = _consts()[3]
    m, n, d = 12, 10, 6
    X = torch.ones((m, d), dtype=torch.float32, device=DEV)
    Y = torch.zeros((n, d), dtype=torch.float64, device=DEV)
    r2 = torch.full((n,), float(d), dtype=torch.float64, device=DEV)
    out = torch.full((m,), -7.0, dtype=torch.float64, device=DEV)
    cnt = torch.full((m,), -7, dtype=torch.int32, device=DEV)
    need = L.gcc_prdc_workspace(m, n, 3)
    assert need == m * 1 * 3 * 8
    ws = torch.empty(L.gcc_prdc_workspace(m, m, MAXK), dtype=torch.uint8, device=DEV)        # the largest call below
    assert ws.numel() >= need
    torch.cuda.synchronize()

    def kth(x=X.data_ptr(), ldx=d, m_=m, y=Y.data_ptr(), ldy=d, n_=n, d_=d, sym=0, k=3, o=out.data_ptr(), w=ws.data_ptr(), wb=ws.numel(), tile=0):
        return L.gcc_prdc_kth_dist(x, 0, ldx, m_, y, 1, ldy, n_, d_, sym, k, 0, tile, o, w, wb, ops.stream())

    def ball(q=X.data_ptr(), ldq=d, m_=m, c=Y.data_ptr(), ldc=d, n_=n, d_=d, r=r2.data_ptr(), o=cnt.data_ptr(), w=ws.data_ptr(), wb=ws.numel(), tile=0):
        return L.gcc_prdc_ball_count(q, 0, ldq, m_, c, 1, ldc, n_, d_, r, 0, tile, o, w, wb, ops.stream())
    before = L.gcc_launch_count(0)
    for what, kw, code in (('X NULL', dict(x=None), BAD_ARG), ('Y NULL', dict(y=None), BAD_ARG), ('out NULL', dict(o=None), BAD_ARG),
                           ('ws NULL', dict(w=None), BAD_ARG), ('ldx < d', dict(ldx=d - 1), BAD_ARG), ('ldy < d', dict(ldy=d - 1), BAD_ARG),
                           ('m = 0', dict(m_=0), BAD_ARG), ('n = 0', dict(n_=0), BAD_ARG), ('d = 0', dict(d_=0), BAD_ARG),
                           ('k = 0', dict(k=0), BAD_ARG), ('k > MAX_K', dict(k=MAXK + 1), BAD_ARG), ('k > n', dict(n_=2, k=3), BAD_ARG),
                           ('symmetric k > m - 1', dict(m_=3, sym=1, k=3), BAD_ARG), ('symmetric X NULL', dict(x=None, sym=1), BAD_ARG),
                           ('a tile that is neither', dict(tile=32), BAD_ARG), ('short workspace', dict(wb=need - 1), WORKSPACE)):
        assert kth(**kw) == code, what
    for what, kw, code in (('Q NULL', dict(q=None), BAD_ARG), ('C NULL', dict(c=None), BAD_ARG), ('r2 NULL', dict(r=None), BAD_ARG),
                           ('out NULL', dict(o=None), BAD_ARG), ('ws NULL', dict(w=None), BAD_ARG), ('ldq < d', dict(ldq=d - 1), BAD_ARG),
                           ('ldc < d', dict(ldc=d - 1), BAD_ARG), ('m = 0', dict(m_=0), BAD_ARG), ('n = 0', dict(n_=0), BAD_ARG),
                           ('d = 0', dict(d_=0), BAD_ARG), ('a tile that is neither', dict(tile=-1), BAD_ARG),
                           ('short workspace', dict(wb=m * 4 - 1), WORKSPACE)):
        assert ball(**kw) == code, what
    assert L.gcc_launch_count(0) == before
    torch.cuda.synchronize()
    assert float(out.min()) == -7.0 and int(cnt.min()) == -7
    assert kth() == 0 and L.gcc_launch_count(0) == before + 2
    assert out.cpu().tolist() == [float(d)] * m                   # ones against zeros: every distance is d
    assert kth(sym=1, y=None, k=m - 1 if m - 1 <= MAXK else MAXK) == 0          # Y is X: its own arguments are not read
    assert out.cpu().tolist() == [0.0] * m
    assert ball() == 0 and L.gcc_launch_count(0) == before + 6
    assert cnt.cpu().tolist() == [n] * m                          # D == r2: inclusive


def test_workspace_is_per_row_and_chunk_not_per_pair():
    from gcc_amd import _lib, ops
    L = ops.lib()
    T, S, MAXK, MAXC = _lib.PRDC_TILE, _lib.PRDC_SMALL_TILE, _lib.PRDC_MAX_K, _lib.PRDC_MAX_CHUNKS
    for m, n in ((1, 1), (T, T), (T + 1, T + 1), (120, 140), (500, 500), (1000, 1000), (2048, 2048), (20000, 20000), (3, 20000)):
        tile, chunks = L.gcc_prdc_tile(m, n), L.gcc_prdc_chunks(m, n)
        # the large tile where it can give every compute unit a workgroup, the small one below
        assert tile == (T if -(-m // T) * min(-(-n // T), MAXC) >= _lib.PRDC_SMALL_BELOW else S), (m, n, tile)
        assert chunks == min(-(-_lib.PRDC_FILL_WORKGROUPS // -(-m // tile)), -(-n // tile), MAXC), (m, n, chunks)
        for k in (1, 5, MAXK):
            assert L.gcc_prdc_workspace(m, n, k) == m * min(-(-n // S), MAXC) * k * 8, (m, n, k)
    assert [L.gcc_prdc_tile(*s) for s in ((120, 140), (500, 500), (1000, 1000), (20000, 20000))] == [S, S, S, T]
    assert L.gcc_prdc_chunks(20000, 20000) * -(-20000 // T) >= _lib.PRDC_FILL_WORKGROUPS       # the grid fills the chip
    assert L.gcc_prdc_chunks(500, 500) * -(-500 // S) == 64        # 16 workgroups with the large tile alone
    assert L.gcc_prdc_tile(0, 5) == 0 and L.gcc_prdc_chunks(5, 0) == 0
    big = L.gcc_prdc_workspace(20000, 20000, MAXK)
    assert 0 < big < 0.01 * 8 * 20000 * 20000                      # 3.2 GB of distances never exist
    assert L.gcc_prdc_workspace(0, 5, 5) == 0 and L.gcc_prdc_workspace(5, 5, 0) == 0 and L.gcc_prdc_workspace(5, 5, MAXK + 1) == 0


def test_wrappers_refuse_what_they_cannot_pass_on():
    from gcc_amd import ops
    from gcc_amd._lib import GccError
    X = torch.ones((7, 6), dtype=torch.float32, device=DEV)
    r2 = torch.ones(7, dtype=torch.float64, device=DEV)
    with pytest.raises(GccError, match='k = 7'):
        ops.prdc_kth_dist(X, k=7)                                  # six other rows
    with pytest.raises(GccError, match='k = 9'):
        ops.prdc_kth_dist(torch.ones((20, 6), device=DEV), k=9)
    with pytest.raises(GccError, match='against'):
        ops.prdc_kth_dist(X, X[:, :5], k=1)
    with pytest.raises(GccError, match='fp32 / f64'):
        ops.prdc_kth_dist(X.half(), k=1)
    with pytest.raises(GccError, match='out must be'):
        ops.prdc_kth_dist(X, k=1, out=torch.empty(6, dtype=torch.float64, device=DEV))
    with pytest.raises(GccError, match='r2 must be'):
        ops.prdc_ball_count(X, X, r2.float())
    with pytest.raises(GccError, match='r2 must be'):
        ops.prdc_ball_count(X, X, r2[:6])
    with pytest.raises(GccError, match='against'):
        ops.prdc_ball_count(X, X[:, :5], r2)
    # columns that are not contiguous are copied, not misread
    Xt = torch.arange(24, dtype=torch.float32, device=DEV).reshape(6, 4).t()       # [4, 6], stride (1, 4)
    _same_bits(ops.prdc_kth_dist(Xt, k=2).cpu().numpy(), P.kth_int(Xt.cpu().numpy(), None, 2)[0], 'transposed view')
