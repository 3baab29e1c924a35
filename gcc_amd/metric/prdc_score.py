"""Improved precision and recall (Kynkaanniemi, Karras, Laine, Lehtinen, Aila 2019) and density and coverage (Naeem, Oh, Uh,
Choi, Yoo 2020) on the activations FID and KID are computed from.  With real activations R [n, d], generated ones F [m, d],
squared distances D(x, y) = |x - y|^2 and the radii rR[i] (rF[j]) = the k-th smallest D from R_i (F_j) to the OTHER rows of its
own set,

    precision = #{ j : exists i, D(F_j, R_i) <= rR[i] } / m        the generated samples that fall on the real manifold
    recall    = #{ i : exists j, D(R_i, F_j) <= rF[j] } / n        the real samples the generated manifold reaches
    density   = sum_j #{ i : D(F_j, R_i) <= rR[i] } / (k m)        how many real balls hold a generated sample, on average
    coverage  = #{ i : min_j D(R_i, F_j) <= rR[i] } / n            the real samples with a generated one in their own ball

A worse FID with precision held and recall / coverage down is mode loss; the other way round it is a loss of fidelity.  k = 5 is
the density / coverage authors' default, k = 3 the precision / recall paper's.  <= is inclusive and duplicate rows are legal (a
radius may be 0).  The pairwise work is five passes of gcc_amd/csrc/prdc.hip -- two radii, coverage's nearest generated
sample, two ball counts -- in f64 without the m x n matrix ever existing; the last reductions are torch operations on the device
and ONE read of four integers comes back to the host, where prdc_from_counts divides.  No CPU path: a missing library / GPU
raises GccError."""
import os

import torch

from .. import ops
from .._lib import PRDC_MAX_K, GccError
from .kid_score import _rows

ENV = 'GCC_FID_PRDC'
DEFAULT_K = 5
KEYS = ('precision', 'recall', 'density', 'coverage')


def prdc_from_counts(precise, recalled, ball_total, covered, m, n, k):
    """the four numbers from their integer counts: ``precise`` of the m generated rows lie in some real ball, ``recalled`` of
    the n real rows in some generated ball, ``ball_total`` real balls counted over all generated rows, ``covered`` real rows
    have a generated row in their own ball.  Plain Python divisions, each of two integers."""
    precise, recalled, ball_total, covered, m, n, k = (int(v) for v in (precise, recalled, ball_total, covered, m, n, k))
    if k < 1 or m <= k or n <= k:
        raise GccError('precision / recall / density / coverage with k = %d need more than k samples on each side, got %d real '
                       'and %d generated' % (k, n, m))
    if not (0 <= precise <= m and 0 <= recalled <= n and 0 <= covered <= n and 0 <= ball_total <= m * n):
        raise GccError('prdc_from_counts: counts %s do not belong to %d generated and %d real rows'
                       % ((precise, recalled, ball_total, covered), m, n))
    return {'precision': precise / m, 'recall': recalled / n, 'density': ball_total / (k * m), 'coverage': covered / n}


def check_k(k, what='k'):
    k = int(k)
    if not 1 <= k <= PRDC_MAX_K:
        raise GccError('%s = %d: expected 1..%d (GCC_PRDC_MAX_K)' % (what, k, PRDC_MAX_K))
    return k


def env_k(environ=None):
    """the k GCC_FID_PRDC asks for, or None when it is unset, empty or 0; anything but an integer in 1..GCC_PRDC_MAX_K raises"""
    raw = (os.environ if environ is None else environ).get(ENV, '')
    raw = raw.strip()
    if raw == '':
        return None
    try:
        k = int(raw)
    except ValueError:
        raise GccError('%s=%s: expected an integer in 1..%d (the k of the nearest-neighbour balls), or 0 / nothing for off'
                       % (ENV, raw, PRDC_MAX_K))
    if k == 0:
        return None
    return check_k(k, ENV)


def nearest_radii(X, k=DEFAULT_K):
    """f64 [rows] on the device: per row of X the squared distance to its k-th nearest OTHER row (one pass, nothing read back)"""
    X = _rows(X, 'nearest_radii')
    k = check_k(k)
    if X.shape[0] <= k:
        raise GccError('nearest_radii: k = %d needs more than k rows, got %d' % (k, X.shape[0]))
    return ops.prdc_kth_dist(X, k=k)


def prdc(real, fake, k=DEFAULT_K, real_radii=None):
    """{'precision', 'recall', 'density', 'coverage'} as Python floats of real activations [n, d] and generated ones [m, d]
    (fp32 or f64 device tensors; rows may be strided).  Five pairwise passes, four when ``real_radii`` (nearest_radii(real, k),
    computed once for a real set that is scored against again and again) is given, and ONE host read of four integers."""
    real, fake = _rows(real, 'prdc'), _rows(fake, 'prdc')
    k = check_k(k)
    (n, d), (m, df) = real.shape, fake.shape
    if m <= k or n <= k:
        raise GccError('precision / recall / density / coverage with k = %d need more than k samples on each side, got %d real '
                       'and %d generated' % (k, n, m))
    if d != df or real.device != fake.device:
        raise GccError('prdc: %s on %s against %s on %s' % (tuple(real.shape), real.device, tuple(fake.shape), fake.device))
    if real_radii is None:
        real_radii = nearest_radii(real, k)
    if not torch.is_tensor(real_radii) or real_radii.dtype != torch.float64 or tuple(real_radii.shape) != (n,) or \
            real_radii.device != real.device:
        raise GccError('prdc: real_radii must be the f64 [%d] tensor nearest_radii(real, k) returns' % n)
    real_radii = real_radii.contiguous()
    fake_radii = ops.prdc_kth_dist(fake, k=k)
    nearest_fake = ops.prdc_kth_dist(real, fake, k=1)                   # coverage's min_j
    in_real = ops.prdc_ball_count(fake, real, real_radii)               # per generated row: the real balls that hold it
    in_fake = ops.prdc_ball_count(real, fake, fake_radii)               # per real row: the generated balls that hold it
    counts = torch.stack(((in_real > 0).sum(), (in_fake > 0).sum(), in_real.sum(dtype=torch.int64),
                          (nearest_fake <= real_radii).sum()))
    precise, recalled, ball_total, covered = counts.cpu().tolist()
    return prdc_from_counts(precise, recalled, ball_total, covered, m, n, k)


def prdc_text(values):
    return 'Precision: %.4f | Recall: %.4f | Density: %.4f | Coverage: %.4f' % tuple(values[key] for key in KEYS)
