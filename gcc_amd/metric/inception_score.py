"""Inception Score (Salimans, Goodfellow, Zaremba, Cheung, Radford, Chen: Improved Techniques for Training GANs, 2016) of a
generated set, from the pool features FID is computed from and the classifier the same weight file carries (fc.weight [1008,
2048], fc.bias: inception_fid.parse_classifier).  With p_i = softmax(W x_i + b) and the set cut into ``splits`` consecutive
ranges of rows, range s = [s n // splits, (s + 1) n // splits) -- the original code's slicing --,

    score_s = exp( mean_{i in s} sum_c p_ic (log p_ic - log mbar_sc) ),    mbar_s = mean_{i in s} p_i
    IS = np.mean(score), np.std(score)            (the population standard deviation, as the original returns them)

Higher is better: each image classified with confidence, the set spread over the classes.  It needs no real set.  The reference
has no Inception Score code; the definition is the paper's, and the FID port of the weights reproduces the original network's
logits, so the number is the one published scores are compared with -- on 2048 features of the native network only.

The head is gcc_amd/csrc/inception_score.hip in f64: rows go through in chunks, the n x 1008 logits never exist, every sum has a
fixed order (same input, same bits).  ONE host read of ``splits`` doubles; np.mean and np.std are the host's.  No CPU path: a
missing library / GPU raises GccError."""
import os

import numpy as np

from .. import ops
from .._lib import GccError
from .kid_score import _rows

ENV = 'GCC_FID_IS'
DEFAULT_SPLITS = 10
DIMS = 2048                         # the classifier reads the pool features: output block 3


def check_splits(value, what='splits'):
    """``value`` as the number of splits: an integer >= 1"""
    try:
        splits = int(value)
        if isinstance(value, bool) or splits != value:
            raise ValueError
    except (TypeError, ValueError):
        raise GccError('%s = %r: expected an integer >= 1 (the number of splits of the Inception Score)' % (what, value))
    if splits < 1:
        raise GccError('%s = %d: expected an integer >= 1 (the number of splits of the Inception Score)' % (what, splits))
    return splits


def env_splits(environ=None):
    """the number of splits GCC_FID_IS asks for, or None when it is unset or empty; anything but an integer >= 1 raises"""
    raw = (os.environ if environ is None else environ).get(ENV, '')
    raw = raw.strip()
    if raw == '':
        return None
    try:
        splits = int(raw)
    except ValueError:
        raise GccError('%s=%s: expected an integer >= 1 (the number of splits of the Inception Score; the usual value is %d), or '
                       'nothing for off' % (ENV, raw, DEFAULT_SPLITS))
    return check_splits(splits, ENV)


def split_bounds(n, splits):
    """[(first row, one past the last)] of the ``splits`` ranges of n rows: preds[k * (N // splits): (k + 1) * (N // splits)] of
    the original where splits divides n, and its generalisation to integer divisions of the products elsewhere: every row is
    scored, the sizes differ by at most one"""
    n, splits = int(n), check_splits(splits)
    if n < splits:
        raise GccError('the Inception Score over %d splits needs at least %d images, got %d' % (splits, splits, n))
    return [(s * n // splits, (s + 1) * n // splits) for s in range(splits)]


def classifier_of(network, what):
    """(weight, bias) of a network that has the classifier, else a GccError that says which case it is and what to do"""
    if getattr(network, 'classifier', None) is not None:
        if getattr(network, 'd', DIMS) != network.classifier[0].shape[1]:
            raise GccError('%s: the classifier reads %d features, the network returns %d'
                           % (what, network.classifier[0].shape[1], network.d))
        return network.classifier
    from .fid_eval import ENV as NETWORK_ENV
    if not hasattr(network, 'precision'):
        raise GccError('%s: the network is a TorchScript archive, which returns features only; the Inception Score needs the '
                       'classifier: let %s name the plain weight file (pt_inception-2015-12-05-6726825d.pth), which the native '
                       'network runs' % (what, NETWORK_ENV))
    if getattr(network, 'output_blocks', (3,))[-1] != 3:
        raise GccError('%s: the network stops at %d features; the classifier reads the %d pool features: score with dims %d'
                       % (what, network.d, DIMS, DIMS))
    raise GccError('%s: the weight file %s names has no fc.weight / fc.bias; the Inception Score needs the classifier: use the '
                   'complete pt_inception weight file' % (what, NETWORK_ENV))


def split_scores(features, weight, bias, splits=DEFAULT_SPLITS):
    """f64 [splits] on the device: the score of every split (ops.inception_split_scores); nothing is read back"""
    features = _rows(features, 'inception_score')
    n = features.shape[0]
    splits = check_splits(splits)
    if n < splits:
        raise GccError('the Inception Score over %d splits needs at least %d images, got %d' % (splits, splits, n))
    return ops.inception_split_scores(features, weight, bias, splits=splits)


def inception_score(features, weight, bias, splits=DEFAULT_SPLITS):
    """(mean, std) as Python floats of the split scores of pool features [n, d] (fp32 or f64 device tensors, rows may be
    strided, [n, d, 1, 1] accepted) under the classifier (weight fp32 [C, d], bias fp32 [C], on the same device); ONE host read
    of ``splits`` doubles"""
    scores = split_scores(features, weight, bias, splits).cpu().numpy()
    return float(np.mean(scores)), float(np.std(scores))


def is_text(value):
    return 'IS: %.4f +- %.4f' % tuple(value)
