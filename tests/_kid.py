"""References and derived bounds of the polynomial-kernel sums (gcc_kid_poly_sum) and of KID, shared by
tests/test_kid_kernels_gpu.py, tests/test_kid_score_gpu.py and tests/test_kid_score_cpu.py (no tests here).

The bound of a sum S = sum over N pairs of k_ij, k = t^3, t = x_i.y_j / d + 1, evaluated in float64 (u = 2^-53) in ANY order:
with A_ij = sum_k |x_ik| |y_jk| and T_ij = A_ij / d + 1 >= |t_ij|,
    the dot product, a chain of d fused or unfused multiply-adds:      |err| <= d u A_ij                 (Higham, gamma_d)
    t = dot (1 / d) + 1: the reciprocal, the product, the sum (fused or not, at most 3 roundings; a division and a sum: 2)
                                                                      |err t| <= (d + 3) u T_ij
    k = (t t) t, two roundings:                                       |err k| <= 3 T^2 |err t| + 2 u T^3 <= (3 d + 11) u T_ij^3
    the sum of the N computed k in any order (sequential, tree, tiles): |err| <= (N - 1) u sum |k_ij| <= (N - 1) u sum T_ij^3
so |S_computed - S| <= (3 d + 11 + N) u sum T^3.  The float64 reference below pays the first three lines as well (numpy's matmul,
then math.fsum: one rounding of the exact sum of ITS k), so a kernel is held to
    (2 (3 d + 11) + N + 1) u sum T^3,
times 1.001 for the second-order terms (d u < 1e-12 at every size used).  Nothing in it comes from what a kernel returned."""
import math
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53


def poly_ref(X, Y=None):
    """(S, sum T^3, N) in float64 of the rows of X against those of Y; Y None: the pairs i != j of X"""
    X = np.asarray(X, dtype=np.float64)
    Z = X if Y is None else np.asarray(Y, dtype=np.float64)
    d = X.shape[1]
    t = X @ Z.T / d + 1.0
    k = t * t * t
    T = np.abs(X) @ np.abs(Z).T / d + 1.0
    T3 = T * T * T
    n_pairs = X.shape[0] * Z.shape[0]
    if Y is None:
        np.fill_diagonal(k, 0.0)
        np.fill_diagonal(T3, 0.0)
        n_pairs -= X.shape[0]
    return math.fsum(k.ravel().tolist()), math.fsum(T3.ravel().tolist()), n_pairs


def poly_bound(d, n_pairs, sum_T3):
    return (2 * (3 * d + 11) + n_pairs + 1) * U53 * sum_T3 * 1.001


def kid_ref(X, Y):
    """(KID, its bound) of float64 restatements: the three sums by poly_ref, the combination in Python floats.  The bound: each
    sum's over its divisor, and 4 roundings (three quotients, two sums, the doubling is exact: 5 at most) on the terms' magnitudes."""
    m, n, d = X.shape[0], Y.shape[0], X.shape[1]
    (sxx, txx, pxx), (syy, tyy, pyy), (sxy, txy, pxy) = poly_ref(X), poly_ref(Y), poly_ref(X, Y)
    value = sxx / (m * (m - 1)) + syy / (n * (n - 1)) - 2 * sxy / (m * n)
    bound = poly_bound(d, pxx, txx) / (m * (m - 1)) + poly_bound(d, pyy, tyy) / (n * (n - 1)) + 2 * poly_bound(d, pxy, txy) / (m * n)
    mag = abs(sxx) / (m * (m - 1)) + abs(syy) / (n * (n - 1)) + 2 * abs(sxy) / (m * n)
    return value, bound + 2 * 5 * U53 * mag


def poly_exact(X, Y=None):
    """the exact rational sum of integer-valued rows (d a power of two), and the largest integer any evaluation order can meet
    when everything is written over d^3: sum |x.y + d|^3 (every product, square, cube and partial sum is below it)"""
    Xi = np.rint(np.asarray(X, dtype=np.float64)).astype(np.int64)
    Zi = Xi if Y is None else np.rint(np.asarray(Y, dtype=np.float64)).astype(np.int64)
    d = Xi.shape[1]
    num = (Xi @ Zi.T + d).astype(object)             # Python integers from here on
    if Y is None:
        np.fill_diagonal(num, 0)
    cubes = [int(v) ** 3 for v in num.ravel().tolist()]
    budget = max(sum(abs(c) for c in cubes), int(np.abs(Xi).max()) * int(np.abs(Zi).max()) * d + d)
    return Fraction(sum(cubes), d ** 3), budget


def diag_exact(X):
    Xi = np.rint(np.asarray(X, dtype=np.float64)).astype(np.int64)
    d = Xi.shape[1]
    return Fraction(sum((int(v) + d) ** 3 for v in (Xi * Xi).sum(1).tolist()), d ** 3)
