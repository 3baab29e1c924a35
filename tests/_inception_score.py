"""Reference and derived bound of the Inception Score kernels (gcc_is_logits, gcc_is_split_scores), shared by
tests/test_inception_score_kernels_gpu.py, tests/test_inception_score_gpu.py and tests/test_inception_score_cpu.py (no tests here).

The reference is the definition in numpy float64: logits Z = X W^T + b, a max-shifted log-sum-exp, p = exp(log p), per split
    score_s = exp( mean_{i in s} sum_c p_ic (log p_ic - log mbar_c) ),   mbar = mean_{i in s} p_i,
with the terms of p_ic == 0 left out.  The kernels compute the same number as (sum_i h_i) / n_s - sum_c mbar_c log mbar_c with
h_i = sum_c p_ic log p_ic.

The bound (u = 2^-53; C classes, d features, n rows; lC = log C; a library exp or log is taken as faithful to 1 ulp, a relative
2 u, which is what both numpy's libm and the device library document for float64).  Per SIDE, against the exact value:
    logits      a chain (or BLAS's order) of d multiply-adds and the bias: |err z| <= (d + 1) u A,  A = max_ic (|b_c| + sum_k
                |x_ik| |w_ck|), computed from the case                                                             =: dz
    log p       R = the largest max - min of a row of logits, L = R + lC >= |log p|.  t = z - m (one rounding, u R); e = exp(t)
                (relative u R + 2 u); s = sum_c e_c, positive terms in any order (relative (C - 1) u more); log s, s in [1, C]
                (absolute (C + 1 + R) u + 2 u lC); log p = t - log s (one rounding, u L): (C + 1 + 3 L) u in all.  A perturbation
                dz of the logits moves z_c - logsumexp(z) by at most 2 dz.               |err log p| <= 2 dz + (C + 1 + 3 L) u =: dl
    p           exp(log p): relative dl + 2 u                                                                      =: rho
    mbar        a sum of n_s <= n positive terms and a division: relative rho + (n + 1) u                          =: rho_m
    kernel      h_i: sum_c |err(p log p)| <= dl + rho |h| and C + 1 roundings on |h| <= lC; their mean: (n + 1) u lC more; E =
                sum_c mbar log mbar: d(x log x) = dx (log x + 1), so rho_m (|E| + 1) <= rho_m (lC + 1), and 2 u (log), u
                (product), C u (sum) on |E| <= lC; the subtraction: u lC.      dl + rho lC + rho_m (lC + 1) + (2 C + n + 6) u lC
    reference   terms p (log p - log mbar) of mixed sign: sum_c p |log p - log mbar|, averaged over the rows, is at most |h| + |E|
                <= 2 lC; on it rho and the (C + n + 4) u of the subtraction, the product, the sum and the mean; p (dl + |err log
                mbar|) sums to dl + rho_m + 2 u lC.                         dl + 2 rho lC + rho_m + (2 C + 2 n + 10) u lC
Both are below
    e_side = dl + 2 rho lC + rho_m (lC + 1) + (2 C + 2 n + 12) u lC,
so |KL_kernel - KL_ref| <= 2 e_side, and with one exp on each side
    |score_kernel - score_ref| <= score_ref (2 e_side + 4 u) 1.001 + 1e-300
(1.001: the second-order terms, e_side < 1e-6 is asserted; 1e-300: probabilities below 2^-1022 are subnormal or 0, where "relative"
does not hold -- C of them weigh less than that).  Nothing in it comes from what a kernel returned."""
import math

import numpy as np

U53 = 2.0 ** -53


def split_bounds(n, splits):
    """the original code's slicing, generalised by integer divisions of the products"""
    return [(s * n // splits, (s + 1) * n // splits) for s in range(splits)]


def logits_ref(X, W, b):
    """(Z float64 [n, C], A: the largest |b_c| + sum_k |x_ik| |w_ck|)"""
    X, W, b = (np.asarray(a, dtype=np.float64) for a in (X, W, b))
    return X @ W.T + b[None, :], float((np.abs(X) @ np.abs(W).T + np.abs(b)[None, :]).max())


def logits_int(X, W, b):
    """int64 [n, C] of integer-valued operands, and the budget every partial sum of a chain stays below"""
    Xi, Wi, bi = (np.rint(np.asarray(a, dtype=np.float64)).astype(np.int64) for a in (X, W, b))
    budget = int(Xi.shape[1] * np.abs(Xi).max() * np.abs(Wi).max() + np.abs(bi).max())
    return Xi @ Wi.T + bi[None, :], budget


def scores_ref(Z, splits):
    """float64 [splits] of logits Z [n, C] by the definition"""
    Z = np.asarray(Z, dtype=np.float64)
    t = Z - Z.max(axis=1, keepdims=True)
    logp = t - np.log(np.exp(t).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    out = np.empty(splits, dtype=np.float64)
    for s, (lo, hi) in enumerate(split_bounds(Z.shape[0], splits)):
        ps, ls = p[lo:hi], logp[lo:hi]
        mbar = ps.mean(axis=0)
        with np.errstate(divide='ignore', invalid='ignore'):
            terms = np.where(ps > 0, ps * (ls - np.log(mbar)[None, :]), 0.0)
        out[s] = math.exp(terms.sum(axis=1).mean())
    return out


def score_bound(n, d, C, A, Z, ref):
    """the bound on |score_kernel - score_ref| per split, from the sizes, the magnitude A of the case and the spread of the
    reference's logits Z; ``ref``: the reference's scores"""
    Z = np.asarray(Z, dtype=np.float64)
    R = float((Z.max(axis=1) - Z.min(axis=1)).max())
    lC = math.log(C)
    L = R + lC
    dz = (d + 1) * U53 * A
    dl = 2 * dz + (C + 1 + 3 * L) * U53
    rho = dl + 2 * U53
    rho_m = rho + (n + 1) * U53
    e_side = dl + 2 * rho * lC + rho_m * (lC + 1) + (2 * C + 2 * n + 12) * U53 * lC
    assert e_side < 1e-6, e_side
    return np.asarray(ref, dtype=np.float64) * (2 * e_side + 4 * U53) * 1.001 + 1e-300


def mean_std(scores):
    scores = np.asarray(scores, dtype=np.float64)
    return float(np.mean(scores)), float(np.std(scores))


def mean_std_bound(bound, ref):
    """(bound on |mean - mean_ref|, bound on |std - std_ref|) of S scores that each moved by at most ``bound``: the mean moves by
    at most the largest of them, a deviation from the mean by at most twice that, and the root mean square of the deviations
    is 1-Lipschitz in their largest change.  np.mean and np.std round on both sides: S + 1 roundings on the scores' magnitude M
    for the mean, at most 2 S + 8 for the standard deviation (the mean, a subtraction, a square, S additions, a division and a
    root, on values below M), each side."""
    b, M, S = float(np.max(bound)), float(np.max(np.abs(ref))), len(ref)
    return b + 2 * (S + 1) * U53 * M, 2 * b + 2 * (2 * S + 8) * U53 * M


def head_ref(features, weight, bias, splits):
    """(scores, bound) of features [n, d] under the classifier (weight [C, d], bias [C]): the reference and its bound at once"""
    Z, A = logits_ref(features, weight, bias)
    ref = scores_ref(Z, splits)
    n, d = np.asarray(features).shape
    return ref, score_bound(n, d, np.asarray(weight).shape[0], A, Z, ref)
