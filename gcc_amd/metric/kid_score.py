"""Kernel Inception Distance (Binkowski, Sutherland, Arbel, Gretton: Demystifying MMD GANs, 2018) on the activations FID is
computed from: the unbiased estimate of MMD^2 with the polynomial kernel k(x, y) = (x.y / d + 1)^3,

    KID = sum_{i != j} k(x_i, x_j) / (m (m - 1)) + sum_{i != j} k(y_i, y_j) / (n (n - 1)) - 2 sum_{i, j} k(x_i, y_j) / (m n)

Unlike FID's its expectation does not depend on the number of samples, which is what makes it the companion number at the set
sizes evaluated here (500 Cityscapes images, 120 / 140 of horse2zebra, against 2048 features).  The three sums are
gcc_kid_poly_sum launches (gcc_amd/csrc/kid.hip: f64, tiled, the Gram matrix never stored, a fixed summation order); the host
reads three doubles and does the last arithmetic in Python floats.  No CPU path: a missing library / GPU raises GccError.

The estimator is the paper's with the block equal to the whole set: every pair counts, once, and the value is deterministic.
torch-fidelity and clean-fid average the same estimator over random subsets of 1000 samples by default: another number."""
import os

import numpy as np
import torch

from .. import ops
from .._lib import GccError


def kid_from_sums(sxx, syy, sxy, m, n):
    """the estimate from its three kernel sums: sxx over the pairs i != j of the m rows of X, syy likewise of the n rows of Y, sxy
    over all m n pairs.  Plain Python arithmetic in this order."""
    m, n = int(m), int(n)
    if m < 2 or n < 2:
        raise GccError('KID needs at least 2 samples on each side, got %d and %d' % (m, n))
    return sxx / (m * (m - 1)) + syy / (n * (n - 1)) - 2 * sxy / (m * n)


def _rows(t, what):
    if torch.is_tensor(t) and t.dim() == 4 and t.shape[2] == 1 and t.shape[3] == 1:
        t = t[:, :, 0, 0]
    if not torch.is_tensor(t) or t.dim() != 2 or t.dtype not in (torch.float32, torch.float64) or not t.is_cuda:
        raise GccError('%s: expected fp32 / f64 activations [n, d] on the GPU, got %s'
                       % (what, '%s %s on %s' % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__))
    return t


def polynomial_self_sum(X):
    """sum_{i != j} k(x_i, x_j) of the rows of X as a Python float: the self term of polynomial_mmd2, for a set that is scored
    against more than once (one launch pair, one host read)"""
    X = _rows(X, 'polynomial_self_sum')
    if X.shape[0] < 2:
        raise GccError('KID needs at least 2 samples on each side, got %d' % X.shape[0])
    return float(ops.kid_poly_sum(X).cpu()[0])


def polynomial_mmd2(X, Y, self_x=None, self_y=None):
    """KID of activations X [m, d] and Y [n, d] (fp32 or f64 device tensors; rows may be strided) as a Python float: three
    gcc_kid_poly_sum calls and ONE host read of three doubles, then kid_from_sums.  ``self_x`` / ``self_y``: the value
    polynomial_self_sum returned for that side (the real set's is computed once per run); that sum is then not launched.
    The paper's unbiased estimator with the block equal to the whole set: deterministic, no random subsets."""
    X, Y = _rows(X, 'polynomial_mmd2'), _rows(Y, 'polynomial_mmd2')
    (m, d), (n, dy) = X.shape, Y.shape
    if m < 2 or n < 2:
        raise GccError('KID needs at least 2 samples on each side, got %d and %d' % (m, n))
    if d != dy or X.device != Y.device:
        raise GccError('polynomial_mmd2: %s on %s against %s on %s' % (tuple(X.shape), X.device, tuple(Y.shape), Y.device))
    out = torch.zeros(3, dtype=torch.float64, device=X.device)
    if self_x is None:
        ops.kid_poly_sum(X, out=out[0:1])
    if self_y is None:
        ops.kid_poly_sum(Y, out=out[1:2])
    ops.kid_poly_sum(X, Y, out=out[2:3])
    sxx, syy, sxy = out.cpu().tolist()
    return kid_from_sums(sxx if self_x is None else float(self_x), syy if self_y is None else float(self_y), sxy, m, n)


class FeatureStore:
    """the activations of one image set on the device: a grow-only fp32 [capacity, d] buffer.  ``append`` takes the [b, d] or
    [b, d, 1, 1] batches ImageStatistics.flush has (a device copy on the current stream, nothing read back), ``rows()`` is a
    view of what was appended so far."""

    def __init__(self, d, device, capacity=256):
        self.d, self.n = int(d), 0
        if self.d <= 0:
            raise GccError('FeatureStore: d must be positive, got %d' % self.d)
        self.device = torch.device(device)
        self.buf = torch.empty((max(1, int(capacity)), self.d), dtype=torch.float32, device=self.device)

    def append(self, act):
        if act.dim() == 4 and act.shape[2] == 1 and act.shape[3] == 1:
            act = act[:, :, 0, 0]
        if act.dim() != 2 or act.shape[1] != self.d or act.dtype != torch.float32 or act.device != self.buf.device:
            raise GccError('FeatureStore.append: expected fp32 activations [b, %d] on %s, got %s %s on %s'
                           % (self.d, self.buf.device, act.dtype, tuple(act.shape), act.device))
        b = act.shape[0]
        if self.n + b > self.buf.shape[0]:
            grown = torch.empty((max(2 * self.buf.shape[0], self.n + b), self.d), dtype=torch.float32, device=self.buf.device)
            grown[:self.n].copy_(self.buf[:self.n])
            self.buf = grown
        self.buf[self.n:self.n + b].copy_(act)
        self.n += b
        return self

    def rows(self):
        return self.buf[:self.n]


# ---- feature files: the real set's activations beside its statistics ----------------------------------------------------------
def features_name(stat_name):
    """real_stat_X.npz -> real_act_X.npz (the same suffix, the same folder); None for a name that is no real_stat*.npz"""
    head, base = os.path.split(str(stat_name))
    if not (base.startswith('real_stat') and base.endswith('.npz')):
        return None
    return os.path.join(head, 'real_act' + base[len('real_stat'):])


def save_features(path, act, network):
    """np.savez(path, act=<fp32 [n, d]>, network=<the network_label string of the network that made them>)"""
    act = act.detach().float().cpu().numpy() if torch.is_tensor(act) else np.asarray(act, dtype=np.float32)
    if act.ndim != 2:
        raise GccError('save_features: expected [n, d] activations, got %s' % (act.shape,))
    np.savez(path, act=np.ascontiguousarray(act, dtype=np.float32), network=np.asarray(str(network)))


def is_features_file(path):
    """does the .npz at `path` hold activations (np.savez(act=, network=)) rather than statistics (mu=, sigma=)"""
    with np.load(path) as z:
        return 'act' in z.files


def load_features(path, d=None, device=None):
    """(act: fp32 [n, d] tensor on `device` (None: a host tensor), network: the label it was written with)"""
    with np.load(path) as z:
        if 'act' not in z.files:
            raise GccError('%s holds %s, not activations (act=, network=)' % (path, ', '.join(z.files)))
        act = np.ascontiguousarray(z['act'], dtype=np.float32)
        network = str(z['network']) if 'network' in z.files else ''
    if act.ndim != 2 or (d is not None and act.shape[1] != d):
        raise GccError('%s holds activations %s; the network\'s have d = %s' % (path, act.shape, d))
    t = torch.from_numpy(act)
    return (t.to(device) if device is not None else t), network
