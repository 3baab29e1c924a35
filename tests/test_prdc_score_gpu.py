"""Precision / recall / density / coverage end to end (gcc_amd.metric.prdc_score, fid_score --prdc, GCC_FID_PRDC through
fid_eval): the four numbers against the numpy float64 restatement of tests/_prdc.py, to the last bit of the final divisions --
the counts are integers, and each comparison first asserts that the reference's own margin at every pair exceeds the rounding
bounds of both sides, so nothing is left to a tolerance and no pair is left out.

The Inception network, folders and model builders are the stand-ins of tests/test_kid_score_gpu.py."""
import warnings

import numpy as np
import pytest
import torch

from . import _prdc as P
from .test_kid_score_gpu import D, _argv, _inception, _Keep, _Log, _model, _pix2pix_root, _png, _real_act, _real_files, _StandIn

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _launches():
    from gcc_amd import ops
    return ops.lib().gcc_launch_count(0)


def _ref(R, F, k, what):
    """the reference's values, after its own margin: every comparison is decided beyond both sides' rounding"""
    margin = P.margin(R, F, k)
    values, counts = P.prdc_ref(R, F, k)
    print('%s: %s, counts %s, margin %.3g' % (what, values, counts, margin))
    assert margin > 0, (what, margin)
    return values


# ---- the four numbers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', (1, 3, 5, 8))
def test_a_set_against_itself(k):
    from gcc_amd.metric.prdc_score import prdc
    X, _ = P.gaussian_sets(150, 150, 20)
    assert P.prdc_ref(X, X, k)[0] == {'precision': 1.0, 'recall': 1.0, 'density': (k + 1) / k, 'coverage': 1.0}
    got = prdc(_t(X), _t(X), k)
    assert all(type(v) is float for v in got.values())
    assert got == {'precision': 1.0, 'recall': 1.0, 'density': (k + 1) / k, 'coverage': 1.0}


def test_two_far_apart_clusters_share_nothing():
    from gcc_amd.metric.prdc_score import prdc
    R, F = P.gaussian_sets(90, 70, 12)
    assert prdc(_t(R), _t(F + 100.0), 5) == dict.fromkeys(P.KEYS, 0.0)
    assert prdc(_t(R, torch.float64), _t(F + 100.0), 1) == dict.fromkeys(P.KEYS, 0.0)


@pytest.mark.parametrize('case', ((129, 127, 17), (257, 130, 70), (300, 260, 64)), ids=lambda c: 'x'.join(map(str, c)))
def test_gaussian_sets_equal_the_float64_restatement(case):
    from gcc_amd.metric import prdc_score as S
    n, m, d = case
    R, F = P.gaussian_sets(n, m, d)
    want = _ref(R, F, 5, '%dx%dx%d' % case)
    assert all(0.05 < want[key] < 0.999 for key in ('precision', 'recall', 'coverage')) and want['density'] > 0.05
    Rd, Fd = _t(R), _t(F)
    before = _launches()
    got = S.prdc(Rd, Fd, 5)
    assert _launches() == before + 10                    # five passes, two launches each
    assert got == want
    # the real set's radii from a cache: the same values, one pass fewer
    radii = S.nearest_radii(Rd, 5)
    assert radii.dtype == torch.float64 and radii.is_cuda and tuple(radii.shape) == (n,)
    before = _launches()
    assert S.prdc(Rd, Fd, 5, real_radii=radii) == want
    assert _launches() == before + 8
    # f64 rows, [n, d, 1, 1] batches, strided rows, and the other k
    wide = torch.full((m, d + 3), float('nan'), device=DEV)
    wide[:, :d] = Fd
    assert S.prdc(Rd.double()[:, :, None, None], wide[:, :d], 5) == want
    assert S.prdc(Rd, Fd, 3) == _ref(R, F, 3, 'k = 3')
    # the roles are not symmetric: the other order is the other question
    swapped = _ref(F, R, 5, 'swapped')
    assert S.prdc(Fd, Rd, 5) == swapped and swapped != want


def test_too_few_rows_unlike_widths_and_bad_k_raise():
    from gcc_amd._lib import PRDC_MAX_K, GccError
    from gcc_amd.metric import prdc_score as S
    X = torch.rand(9, 6, device=DEV)
    for a, b in ((X[:5], X), (X, X[:5])):
        with pytest.raises(GccError, match='more than k samples'):
            S.prdc(a, b, 5)
    with pytest.raises(GccError, match='more than k rows'):
        S.nearest_radii(X[:3], 3)
    for k in (0, PRDC_MAX_K + 1):
        with pytest.raises(GccError, match='expected 1..%d' % PRDC_MAX_K):
            S.prdc(torch.rand(20, 6, device=DEV), torch.rand(20, 6, device=DEV), k)
    with pytest.raises(GccError, match='against'):
        S.prdc(X, X[:, :5], 3)
    with pytest.raises(GccError, match='on the GPU'):
        S.prdc(X.cpu(), X, 3)
    with pytest.raises(GccError, match='real_radii must be'):
        S.prdc(X, X, 3, real_radii=torch.ones(8, dtype=torch.float64, device=DEV))


# ---- python -m gcc_amd.metric.fid_score --prdc ------------------------------------------------------------------------------------
REAL, FAKE, BATCH = 48, 40, 8


def _folders(tmp_path):
    """images of random brightness: the activations spread along a curve, and the two sets overlap in part"""
    rng = np.random.RandomState(12)
    a, b = tmp_path / 'real', tmp_path / 'fake'
    a.mkdir(), b.mkdir()
    for i in range(REAL):
        _png(a / ('img%03d.png' % i), rng.randint(0, rng.randint(60, 256), (12, 20, 3), dtype=np.uint8))
    for i in range(FAKE):
        _png(b / ('img%03d.png' % i), rng.randint(0, rng.randint(40, 200), (12, 20, 3), dtype=np.uint8))
    return a, b


def test_fid_score_prdc_on_folders_then_on_their_feature_files(tmp_path, capsys):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import fid_score as F
    from gcc_amd.metric.kid_score import save_features
    from gcc_amd.metric.prdc_score import prdc_text
    a, b = _folders(tmp_path)
    keep = _Keep(_StandIn(1, 64).to(DEV))
    argv = [str(a), str(b), '--batch-size', str(BATCH), '--dims', '64']
    plain = F.main(argv, model=keep)
    out = capsys.readouterr().out.splitlines()
    assert len(plain) == 2 and out == ['FID: %.2f' % plain[0], 'KID: %.6f' % plain[1]]       # without the flag: today's output
    act_r, act_f = keep.activations(0, REAL // BATCH), keep.activations(REAL // BATCH, (REAL + FAKE) // BATCH)
    assert act_r.shape == (REAL, 64) and act_f.shape == (FAKE, 64)
    want = _ref(act_r, act_f, 5, 'folders')
    assert all(0.05 < want[key] < 0.999 for key in ('precision', 'recall', 'density', 'coverage'))
    want3 = _ref(act_r, act_f, 3, 'folders, k = 3')
    capsys.readouterr()                                              # the reference's own prints
    fid, kid, got = F.main(argv + ['--prdc'], model=keep)
    out = capsys.readouterr().out.splitlines()
    assert (fid, kid) == plain and got == want
    assert out == ['FID: %.2f' % fid, 'KID: %.6f' % kid, prdc_text(want)]
    assert out[2].startswith('Precision: %.4f | Recall: %.4f | Density: ' % (want['precision'], want['recall']))
    assert F.main(argv + ['--prdc', '--nearest-k', '3'], model=keep)[2] == want3 and want3 != want
    assert capsys.readouterr().out.splitlines()[2] == prdc_text(want3)
    # the feature files of the same activations: no network, the same numbers
    feat_r, feat_f, stat_f = tmp_path / 'real_act_r.npz', tmp_path / 'real_act_f.npz', tmp_path / 'real_stat_f.npz'
    save_features(str(feat_r), act_r.astype(np.float32), '')
    save_features(str(feat_f), act_f.astype(np.float32), '')

    def no_network(x):
        raise AssertionError('files alone need no network')
    assert F.main([str(feat_r), str(feat_f), '--dims', '64', '--prdc'], model=no_network)[2] == want
    assert capsys.readouterr().out.splitlines()[2] == prdc_text(want)
    assert F.main([str(feat_r), str(b), '--batch-size', str(BATCH), '--dims', '64', '--prdc'], model=keep)[2] == want
    # a bare statistics file has no activations: the flag names it, without the flag it still scores
    np.savez(str(stat_f), mu=np.mean(act_f, axis=0), sigma=np.cov(act_f, rowvar=False))
    with pytest.raises(GccError, match=r'real_stat_f\.npz holds statistics'):
        F.main([str(feat_r), str(stat_f), '--dims', '64', '--prdc'], model=no_network)
    capsys.readouterr()
    assert F.main([str(feat_r), str(stat_f), '--dims', '64'], model=no_network)[1] is None
    assert len(capsys.readouterr().out.splitlines()) == 1
    with pytest.raises(GccError, match='--nearest-k = 9'):
        F.main(argv + ['--prdc', '--nearest-k', '9'], model=keep)


# ---- GCC_FID_PRDC through the evaluators -------------------------------------------------------------------------------------------
def _stat_only(root, name, seed):
    a = _real_act(seed).double().numpy()
    np.savez(str(root / name), mu=np.mean(a, axis=0), sigma=np.cov(a, rowvar=False))


def test_pix2pix_evaluator_logs_the_line_only_when_asked(tmp_path, monkeypatch):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import fid_eval as E
    from gcc_amd.metric import prdc_score as S
    root = _pix2pix_root(tmp_path)
    real = _real_files(root, 'real_stat_B.npz', 1)
    model, opt = _model(_argv('pix2pix', root, tmp_path))
    net = torch.jit.load(str(_inception(tmp_path)), map_location=DEV)
    monkeypatch.delenv(S.ENV, raising=False)
    log = _Log()
    E.fid_evaluator(net, log, batch_size=4)(model, opt)
    assert len(log.lines) == 2 and log.lines[0].startswith('FID: ') and log.lines[1].startswith('KID: ')      # today's log
    monkeypatch.setenv(S.ENV, '0')
    log0 = _Log()
    E.fid_evaluator(net, log0, batch_size=4)(model, opt)
    assert log0.lines == log.lines
    monkeypatch.setenv(S.ENV, '3')
    keep, log3, calls = _Keep(net), _Log(), []
    real_radii = S.nearest_radii
    monkeypatch.setattr(S, 'nearest_radii', lambda X, k=S.DEFAULT_K: (calls.append((tuple(X.shape), k)), real_radii(X, k))[1])
    evaluate = E.fid_evaluator(keep, log3, batch_size=4)
    with warnings.catch_warnings():
        warnings.filterwarnings('error', message='.*activations of two networks')
        scores = evaluate(model, opt)
        again = evaluate(model, opt)
    assert scores == again and len(log3.lines) == 6 and log3.lines[:2] == log.lines and log3.lines[3:] == log3.lines[:3]
    fake = keep.activations(0, 2)                                    # the first evaluation's two batches
    assert fake.shape == (6, D)
    want = _ref(real, fake, 3, 'pix2pix evaluator')
    assert log3.lines[2] == S.prdc_text(want) == E.prdc_line([want], ['AtoB'], 'pix2pix')
    assert calls == [((40, D), 3)]                                   # the real set's radii: once over two evaluations
    key = (str(root / 'real_act_B.npz'), 'radii', 3)
    assert key in evaluate.state['kid'] and evaluate.state['kid'][key].dtype == torch.float64
    # a value outside 1..GCC_PRDC_MAX_K, and a slot without its feature file
    monkeypatch.setenv(S.ENV, '9')
    with pytest.raises(GccError, match='GCC_FID_PRDC = 9'):
        E.fid_evaluator(net, _Log(), batch_size=4)(model, opt)
    monkeypatch.setenv(S.ENV, '3')
    (root / 'real_act_B.npz').unlink()
    with pytest.raises(GccError, match=r'real_act_B\.npz missing .*get_real_stat .*--features_path'):
        E.fid_evaluator(net, _Log(), batch_size=4)(model, opt)


def test_cyclegan_evaluator_logs_one_line_with_both_directions(tmp_path, monkeypatch):
    from gcc_amd.metric import fid_eval as E
    from gcc_amd.metric import prdc_score as S
    root = tmp_path / 'h2z'
    rng = np.random.RandomState(5)
    for sub, stem in (('testA', 'h'), ('testB', 'z')):
        (root / sub).mkdir(parents=True)
        for i in range(5):
            _png(root / sub / ('%s%d.png' % (stem, i)), rng.randint(0, 256, (256, 256, 3), dtype=np.uint8))
    real_b = _real_files(root, 'real_stat_B.npz', 2)
    real_a = _real_files(root, 'real_stat_A.npz', 3)
    model, opt = _model(_argv('cyclegan', root, tmp_path))
    net = torch.jit.load(str(_inception(tmp_path, pool=2)), map_location=DEV)
    monkeypatch.setenv(S.ENV, '3')
    log, made = _Log(), []
    real_init = E.FidScorer.__init__
    monkeypatch.setattr(E.FidScorer, '__init__', lambda self, *a, **k: (real_init(self, *a, **k), made.append(self))[0])
    got = E.fid_evaluator(net, log, batch_size=4)(model, opt)
    assert [t for _, t in got] == ['AtoB', 'BtoA'] and len(log.lines) == 3
    assert log.lines[0].startswith('AtoB FID: ') and log.lines[1].startswith('AtoB KID: ')
    wants = []
    for st, real, what in zip(made[0].stats, (real_b, real_a), ('AtoB', 'BtoA')):
        fake = st.features.rows().double().cpu().numpy()
        assert fake.shape == (5, D)
        wants.append(_ref(real, fake, 3, 'cyclegan ' + what))
    assert made[0].prdc() == wants
    assert log.lines[2] == 'AtoB %s | BtoA %s' % (S.prdc_text(wants[0]), S.prdc_text(wants[1]))
