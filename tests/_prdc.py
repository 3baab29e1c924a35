"""References and derived bounds of the nearest-neighbour kernels (gcc_prdc_kth_dist, gcc_prdc_ball_count) and of precision /
recall / density / coverage, shared by tests/test_prdc_kernels_gpu.py, tests/test_prdc_score_gpu.py and
tests/test_prdc_score_cpu.py (no tests here).

The bound of D(x, y) = sum_c (x_c - y_c)^2, from the order include/gcc_hip.h documents (the difference form; u = 2^-53):
    t_c = fl(x_c - y_c) = (x_c - y_c)(1 + e1), |e1| <= u (the inputs are float64, or float32 converted exactly)
    acc_c = fl(fma(t_c, t_c, acc_{c-1})) = (acc_{c-1} + t_c^2)(1 + e_c): the square is exact inside the fused multiply-add
so term c carries (1 + e1)^2 and the roundings of the additions c, c + 1, ..., d - 1, at most d of them.  Every term is >= 0, so
    |D_kernel - D| <= ((1 + u)^(d + 2) - 1) D = gamma_{d+2} D.
The float64 reference below (numpy: the difference, its square with one rounding of its own, a sum over c in numpy's pairwise
order, where a term passes at most d - 1 additions) pays 2 + 1 + (d - 1) roundings: gamma_{d+2} D as well.  A kernel is held to
    |D_kernel - D_ref| <= 2 (d + 2) u D_ref, times 1.001 for the second-order terms and for D_ref standing in for D
(d u < 1e-12 at every size used).  Order statistics are monotone in every argument: if every D_j moves by at most a factor
(1 +- e), so does the k-th smallest of them -- it is 1-Lipschitz in the sup norm, and here the tighter relative statement holds --
so the k-th distance of a row is held to the same bound on ITS value.  Nothing in it comes from what a kernel returned."""
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53
KEYS = ('precision', 'recall', 'density', 'coverage')


def dist_bound(d, D):
    return 2 * (d + 2) * U53 * np.asarray(D, dtype=np.float64) * 1.001


def sqdist(X, Y, slab=32):
    """float64 [m, n] of direct differences, in row slabs (the m x n x d intermediate stays small)"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    out = np.empty((X.shape[0], Y.shape[0]), dtype=np.float64)
    for s in range(0, X.shape[0], slab):
        diff = X[s:s + slab, None, :] - Y[None, :, :]
        out[s:s + slab] = (diff * diff).sum(-1)
    return out


def kth_of(D, k, symmetric):
    """the k-th smallest of every row of D; symmetric: without the diagonal"""
    D = np.array(D, dtype=np.float64)                    # a copy: the caller's matrix keeps its diagonal
    if symmetric:
        np.fill_diagonal(D, np.inf)
    return np.partition(D, k - 1, axis=1)[:, k - 1]


def kth_ref(X, Y=None, k=5):
    return kth_of(sqdist(X, X if Y is None else Y), k, Y is None)


def ball_ref(Q, C, r2):
    return (sqdist(Q, C) <= np.asarray(r2)[None, :]).sum(1)


def counts_of(Drr, Dff, Drf, k):
    """(precise, recalled, ball_total, covered) from the three distance matrices (real x real, fake x fake, real x fake), in
    whatever exact or floating type they come"""
    rR, rF = kth_of(Drr, k, True), kth_of(Dff, k, True)
    in_real = Drf <= rR[:, None]                         # [i, j]: F_j in R_i's ball
    in_fake = Drf <= rF[None, :]                         # [i, j]: R_i in F_j's ball
    precise = int(in_real.any(0).sum())
    recalled = int(in_fake.any(1).sum())
    ball_total = int(in_real.sum())
    covered = int((Drf.min(1) <= rR).sum())
    return precise, recalled, ball_total, covered


def prdc_ref(R, F, k):
    """({'precision', ...} by the definitions, in float64 numpy; the four integer counts)"""
    n, m = np.asarray(R).shape[0], np.asarray(F).shape[0]
    c = counts_of(sqdist(R, R), sqdist(F, F), sqdist(R, F), k)
    return {'precision': c[0] / m, 'recall': c[1] / n, 'density': c[2] / (k * m), 'coverage': c[3] / n}, c


def margin(R, F, k):
    """the reference's own margin: min over every pair and every comparison prdc makes of |D_ref - radius| minus the two
    bounds (kernel and reference) on D and on the radius; positive: no decision can fall either way within rounding"""
    return margin_of(sqdist(R, R), sqdist(F, F), sqdist(R, F), np.asarray(R).shape[1], k)


def margin_of(Drr, Dff, Drf, d, k):
    rR, rF = kth_of(Drr, k, True), kth_of(Dff, k, True)
    worst = np.inf
    for rad in (rR[:, None], rF[None, :]):
        worst = min(worst, float((np.abs(Drf - rad) - dist_bound(d, Drf) - dist_bound(d, rad)).min()))
    near = Drf.min(1)
    return min(worst, float((np.abs(near - rR) - dist_bound(d, near) - dist_bound(d, rR)).min()))


# ---- exact: integer-valued rows -----------------------------------------------------------------------------------------------
def sqdist_int(X, Y):
    """int64 [m, n] of integer-valued rows, and the budget: the largest D (every partial sum of a chain is below it)"""
    Xi = np.rint(np.asarray(X, dtype=np.float64)).astype(np.int64)
    Yi = np.rint(np.asarray(Y, dtype=np.float64)).astype(np.int64)
    out = np.empty((Xi.shape[0], Yi.shape[0]), dtype=np.int64)
    for s in range(0, Xi.shape[0], 64):
        diff = Xi[s:s + 64, None, :] - Yi[None, :, :]
        out[s:s + 64] = (diff * diff).sum(-1)
    return out, int(out.max())


def kth_int(X, Y=None, k=5):
    """(the k-th smallest integer distance per row, the budget); Y None: without the diagonal"""
    D, budget = sqdist_int(X, X if Y is None else Y)
    D = D.astype(np.float64)                             # exact below 2^53
    return kth_of(D, k, Y is None), budget


def ball_int(Q, C, r2):
    D, budget = sqdist_int(Q, C)
    return (D <= np.rint(np.asarray(r2)).astype(np.int64)[None, :]).sum(1), budget


def prdc_int(R, F, k):
    (Drr, b0), (Dff, b1), (Drf, b2) = sqdist_int(R, R), sqdist_int(F, F), sqdist_int(R, F)
    return counts_of(Drr.astype(np.float64), Dff.astype(np.float64), Drf.astype(np.float64), k), max(b0, b1, b2)


def counts_fraction(R, F, k):
    """the four counts by brute force in fractions.Fraction and Python lists: no numpy, no partition, sorted() for the k-th"""
    R = [[Fraction(v) for v in row] for row in np.asarray(R).tolist()]
    F = [[Fraction(v) for v in row] for row in np.asarray(F).tolist()]
    D = lambda x, y: sum((a - b) * (a - b) for a, b in zip(x, y))
    rR = [sorted(D(R[i], R[j]) for j in range(len(R)) if j != i)[k - 1] for i in range(len(R))]
    rF = [sorted(D(F[i], F[j]) for j in range(len(F)) if j != i)[k - 1] for i in range(len(F))]
    precise = sum(1 for f in F if any(D(f, R[i]) <= rR[i] for i in range(len(R))))
    recalled = sum(1 for r in R if any(D(r, F[j]) <= rF[j] for j in range(len(F))))
    ball_total = sum(1 for f in F for i in range(len(R)) if D(f, R[i]) <= rR[i])
    covered = sum(1 for i in range(len(R)) if min(D(R[i], f) for f in F) <= rR[i])
    return precise, recalled, ball_total, covered


def gaussian_sets(n, m, d, seed=0):
    """standard-normal real rows [n, d] and 1.1 N(0, 1) + 0.2 generated rows [m, d], representable in float32"""
    rng = np.random.RandomState(seed + 1000 * n + 10 * m + d)
    R = rng.standard_normal((n, d)).astype(np.float32).astype(np.float64)
    F = (1.1 * rng.standard_normal((m, d)) + 0.2).astype(np.float32).astype(np.float64)
    return R, F
