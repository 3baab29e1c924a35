"""The host half of the Inception Score (gcc_amd.metric.inception_score, inception_fid.parse_classifier, fid_eval.is_line,
fid_score's flag): the slicing, GCC_FID_IS, the classifier's shapes, the log lines, the header's constants and prototypes against
their Python mirrors, and the numpy reference of tests/_inception_score.py on its closed forms.  No GPU."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from . import _inception_emul as E
from . import _inception_score as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_bounds_are_the_original_slicing():
    from gcc_amd._lib import GccError
    from gcc_amd.metric.inception_score import split_bounds
    for n, S in ((10, 10), (151, 7), (5000, 10)):
        got = split_bounds(n, S)
        assert got == R.split_bounds(n, S) == [(s * n // S, (s + 1) * n // S) for s in range(S)]
        assert got[0][0] == 0 and got[-1][1] == n and all(a[1] == b[0] for a, b in zip(got, got[1:]))      # every row, once
        sizes = [hi - lo for lo, hi in got]
        assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1
        if n % S == 0:                                     # preds[k * (N // splits): (k + 1) * (N // splits)]
            assert got == [(k * (n // S), (k + 1) * (n // S)) for k in range(S)]
    assert [hi - lo for lo, hi in split_bounds(151, 7)] == [21, 22, 21, 22, 21, 22, 22]
    with pytest.raises(GccError, match=r'12 splits .*at least 12 images, got 11'):
        split_bounds(11, 12)


def test_splits_are_an_integer_of_at_least_one():
    from gcc_amd._lib import GccError
    from gcc_amd.metric import inception_score as S
    assert S.ENV == 'GCC_FID_IS' and S.DEFAULT_SPLITS == 10
    assert S.check_splits(1, 'x') == 1 and S.check_splits(10, 'x') == 10 and S.check_splits(np.int64(3), 'x') == 3
    for bad in (0, -1, 'x', None, 2.5):
        with pytest.raises(GccError, match='--splits'):
            S.check_splits(bad, '--splits')
    for off in ({}, {S.ENV: ''}, {S.ENV: ' '}):
        assert S.env_splits(off) is None
    assert S.env_splits({S.ENV: '10'}) == 10 and S.env_splits({S.ENV: ' 1 '}) == 1
    for bad in ('0', '-1', 'x', '2.5'):
        with pytest.raises(GccError, match=S.ENV):
            S.env_splits({S.ENV: bad})


def test_parse_classifier_reads_the_head_beside_the_features():
    from gcc_amd._lib import GccError
    from gcc_amd.metric import inception_fid as I
    shapes = E.shapes(8)
    d = E.feature_width(8)
    assert I.parse_classifier(shapes) == ((1008, d), (1008,))
    assert I.parse_classifier(shapes, I.parse_fid_inception(shapes)) == ((1008, d), (1008,))
    bare = {k: v for k, v in shapes.items() if not k.startswith('fc.')}
    assert I.parse_classifier(bare) is None
    assert I.UNUSED_KEYS == ('fc.weight', 'fc.bias')                          # the features' parser still leaves them alone
    assert I.parse_fid_inception(shapes).d == I.parse_fid_inception(bare).d == d
    with pytest.raises(GccError, match=r'fc\.weight has shape \(1008, %d\), expected \(C >= 2, %d\)' % (d + 8, d)):
        I.parse_classifier(dict(shapes, **{'fc.weight': (1008, d + 8)}))
    with pytest.raises(GccError, match=r'fc\.weight has shape'):
        I.parse_classifier(dict(shapes, **{'fc.weight': (1, d), 'fc.bias': (1,)}))
    with pytest.raises(GccError, match=r'fc\.bias has shape \(1000,\), expected \(1008,\)'):
        I.parse_classifier(dict(shapes, **{'fc.bias': (1000,)}))
    with pytest.raises(GccError, match=r'fc\.bias is missing'):
        I.parse_classifier({k: v for k, v in shapes.items() if k != 'fc.bias'})


def test_engine_keeps_the_classifier_only_where_it_can_be_applied():
    import torch
    from gcc_amd.metric.inception_fid import InceptionFidEngine
    sd = E.seeded(8, 3)
    eng = InceptionFidEngine(sd, resize=75)
    w, b = eng.classifier
    assert w.dtype == b.dtype == torch.float32 and tuple(w.shape) == (1008, eng.d) and tuple(b.shape) == (1008,)
    assert torch.equal(w, sd['fc.weight']) and torch.equal(b, sd['fc.bias'])
    assert InceptionFidEngine(sd, resize=75, output_blocks=(2,), pooled=True).classifier is None       # stops below block 3
    assert InceptionFidEngine({k: v for k, v in sd.items() if not k.startswith('fc.')}, resize=75).classifier is None


def test_a_network_without_the_classifier_is_named_for_what_it_is(tmp_path):
    from types import SimpleNamespace
    from gcc_amd._lib import GccError
    from gcc_amd.metric.fid_eval import FidScorer
    from gcc_amd.metric.inception_score import classifier_of
    head = (np.zeros((1008, 2048), dtype=np.float32), np.zeros(1008, dtype=np.float32))
    native = SimpleNamespace(precision='bf16', output_blocks=(3,), d=2048, classifier=head)
    assert classifier_of(native, 'x') is head
    with pytest.raises(GccError, match='TorchScript archive.*GCC_FID_INCEPTION'):
        classifier_of(object(), 'x')
    with pytest.raises(GccError, match='stops at 192 features.*2048'):
        classifier_of(SimpleNamespace(precision='bf16', output_blocks=(1,), d=192, classifier=None), 'x')
    with pytest.raises(GccError, match=r'no fc\.weight / fc\.bias'):
        classifier_of(SimpleNamespace(precision='fp32', output_blocks=(3,), d=2048, classifier=None), 'x')
    # the scorer refuses when it is made, before any image; without the variable nothing is asked of the network
    np.savez(str(tmp_path / 'real_stat_B.npz'), mu=np.zeros(3), sigma=np.eye(3))
    slots = [('real_stat_B.npz', 'AtoB')]
    assert FidScorer(object(), tmp_path, slots).inception_score() is None
    with pytest.raises(GccError, match='GCC_FID_IS=2: the network is a TorchScript archive'):
        FidScorer(object(), tmp_path, slots, is_splits=2)
    with pytest.raises(GccError, match='GCC_FID_IS = 0'):
        FidScorer(native, tmp_path, slots, is_splits=0)
    sc = FidScorer(native, tmp_path, slots, is_splits=2)
    assert sc.is_splits == 2 and sc.kid() is None and sc.prdc() is None and all(st.keep_features for st in sc.stats)
    assert not any(st.keep_features for st in FidScorer(native, tmp_path, slots).stats)


def test_is_text_and_is_line_have_one_form_per_model():
    from gcc_amd.metric.fid_eval import is_line
    from gcc_amd.metric.inception_score import is_text
    assert is_text((9.37219, 0.12345)) == 'IS: 9.3722 +- 0.1235'
    a, b = (2.5, 0.0), (11.23456, 1.5)
    assert is_line([a], ['AtoB'], 'pix2pix') == is_line([a], ['BtoA'], 'sagan') == 'IS: 2.5000 +- 0.0000'
    assert is_line([a, b], ['AtoB', 'BtoA'], 'cyclegan') == 'AtoB IS: 2.5000 +- 0.0000 | BtoA IS: 11.2346 +- 1.5000'


def test_header_constants_and_prototypes_have_their_mirrors():
    from gcc_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gcc_hip.h')).read()
    for name in ('TILE', 'KSTEP', 'CHUNK'):
        assert int(re.search(r'#define\s+GCC_IS_%s\s+(\d+)' % name, hdr).group(1)) == getattr(_lib, 'IS_' + name), name
    assert int(re.search(r'#define\s+GCC_HIP_ABI\s+(\d+)', hdr).group(1)) == 605
    for name, arity in (('gcc_is_workspace', 3), ('gcc_is_logits', 11), ('gcc_is_split_scores', 14)):
        m = re.search(r'\b%s\(([^;]*?)\);' % name, hdr, re.S)
        assert m and name in _lib.PROTOTYPES
        assert len(m.group(1).split(',')) == len(_lib.PROTOTYPES[name][1]) == arity
    src = open(os.path.join(ROOT, 'gcc_amd', 'csrc', 'build.sh')).read()
    assert re.search(r'^SRCS=".*\binception_score\b.*"', src, re.M)
    assert os.path.isfile(os.path.join(ROOT, 'gcc_amd', 'csrc', 'inception_score.hip'))


def test_the_flag_is_parsed_and_off_by_default():
    from gcc_amd.metric import fid_score as F
    args = F.parser.parse_args(['a', 'b', '--inception-score', '--splits', '5'])
    assert args.inception_score is True and args.splits == 5
    args = F.parser.parse_args(['a', 'b'])
    assert args.inception_score is False and args.splits == 10
    sig = inspect.signature(F.calculate_fid_given_paths)
    assert sig.parameters['is_splits'].default is None and list(sig.parameters)[-1] == 'is_splits'


def test_the_reference_knows_its_closed_forms():
    # K classes hit equally often with certainty: K.  Equal logits: 1.  One row per split: 1.
    for K in (2, 8):
        Z = np.full((4 * K, 50), 5.0)
        Z[np.arange(4 * K), (np.arange(4 * K) % K) * 3] = 805.0
        ref = R.scores_ref(Z, 2)
        assert np.isfinite(ref).all() and np.abs(ref - K).max() < 1e-12 * K
    assert np.abs(R.scores_ref(np.full((9, 7), -2.0), 3) - 1.0).max() < 1e-14
    rng = np.random.RandomState(0)
    Z = rng.standard_normal((6, 11)) * 3
    assert np.abs(R.scores_ref(Z, 6) - 1.0).max() < 1e-14
    # against the definition written the long way, in Python floats with math.fsum
    want = []
    for lo, hi in R.split_bounds(6, 2):
        P = [[math.exp(z - max(row) - math.log(math.fsum(math.exp(v - max(row)) for v in row))) for z in row] for row in Z[lo:hi].tolist()]
        mbar = [math.fsum(p[c] for p in P) / len(P) for c in range(11)]
        want.append(math.exp(math.fsum(p[c] * (math.log(p[c]) - math.log(mbar[c])) for p in P for c in range(11)) / len(P)))
    ref = R.scores_ref(Z, 2)
    assert np.abs(ref - np.array(want)).max() < 1e-13 and ref.min() > 1.01
    # the bound grows with every size it is derived from, and is small against the score at the network's sizes
    Zn, A = R.logits_ref(rng.standard_normal((20, 2048)), rng.standard_normal((1008, 2048)) * 0.05, np.zeros(1008))
    b0 = R.score_bound(20, 2048, 1008, A, Zn, np.ones(2))
    assert 0 < b0.max() < 1e-8
    assert (R.score_bound(20, 4096, 1008, A, Zn, np.ones(2)) > b0).all() and (R.score_bound(2000, 2048, 1008, A, Zn, np.ones(2)) > b0).all()
    assert (R.score_bound(20, 2048, 1008, 2 * A, Zn, np.ones(2)) > b0).all() and (R.score_bound(20, 2048, 1008, A, 2 * Zn, np.ones(2)) > b0).all()
    m, s = R.mean_std([1.0, 3.0])
    assert (m, s) == (2.0, 1.0)                                                # the population standard deviation
