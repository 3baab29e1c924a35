"""The Inception Score end to end (gcc_amd.metric.inception_score, InceptionFidEngine.classifier, fid_score --inception-score,
GCC_FID_IS through fid_eval): the native network's own features and its weight file's classifier, against the float64 numpy
restatement of tests/_inception_score.py applied to THE DEVICE'S OWN FEATURES copied to the host -- what is under test here is the
head and its plumbing; the features have their own tests (tests/test_inception_fid_gpu.py, tests/test_inception_fid_fp32_gpu.py)
-- within the bound derived there."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _inception_emul as E

from . import _inception_score as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DIV, RESIZE, IMAGES = 8, 75, 24              # the thin network of the Inception engine tests; 24 seeded 64 x 64 images
SHARP = 300.0


def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(str(path))


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, line):
        self.lines.append(line)


class _Keep:
    """the engine, keeping every batch of features it returns; everything else (.classifier, .d, .precision) is the engine's"""

    def __init__(self, net):
        self.net, self.outputs = net, []

    def to(self, device):
        self.net = self.net.to(device)
        return self

    def eval(self):
        return self

    def __call__(self, x):
        y = self.net(x)
        self.outputs.append(y[0].clone())
        return y

    def __getattr__(self, name):
        return getattr(self.net, name)

    def features(self, lo=0, hi=None):
        return torch.cat(self.outputs[lo:hi]).flatten(1).double().cpu().numpy()


@pytest.fixture(scope='module')
def thin():
    """(state_dict, {precision: (engine, its features of the 24 images on the device)}), computed once.  The seeded fc.weight is
    small (logits within a few hundredths, every score 1.00000x): it is taken 300 times larger, where the probabilities are far
    enough from uniform for the score's printed digits to say something."""
    from gcc_amd.metric.inception_fid import InceptionFidEngine
    sd = E.seeded(DIV, 22)
    sd['fc.weight'] = sd['fc.weight'] * SHARP
    x = E.seeded_input((IMAGES, 3, 64, 64), 122).to(DEV)
    out = {}
    for precision in ('bf16', 'fp32'):
        eng = InceptionFidEngine(sd, resize=RESIZE, precision=precision).to(DEV).eval()
        out[precision] = (eng, eng(x)[0])
    return sd, out


def _ref(features, sd, splits, what):
    """(mean, std) of the restatement on host copies of the features, and the bounds on both"""
    scores, bound = R.head_ref(features, sd['fc.weight'].double().numpy(), sd['fc.bias'].double().numpy(), splits)
    (mean, std), (bm, bs) = R.mean_std(scores), R.mean_std_bound(bound, scores)
    print('%s: split scores %s, IS %.12g +- %.6g, bounds %.3g / %.3g' % (what, scores, mean, std, bm, bs))
    return (mean, std), (bm, bs)


def _lines(capsys):
    """what was printed, without the Frechet distance's own notice about a singular product (fewer images than features)"""
    return [line for line in capsys.readouterr().out.splitlines() if not line.startswith('fid calculation')]


def _same(a, b):
    """equal, where a FID of fewer images than features may be NaN on both sides"""
    return all(x == y or (x != x and y != y) for x, y in zip(a, b)) and len(a) == len(b)


def _close(got, want, bounds, what):
    errs = [abs(g - w) for g, w in zip(got, want)]
    print('%s: err %.3g / %.3g against %.3g / %.3g' % ((what,) + tuple(errs) + tuple(bounds)))
    assert all(type(g) is float and np.isfinite(g) for g in got) and all(e <= b for e, b in zip(errs, bounds)), what


@pytest.mark.parametrize('precision', ('bf16', 'fp32'))
def test_engine_carries_the_classifier_and_the_head_scores_its_features(thin, precision):
    from gcc_amd.metric.inception_score import inception_score, split_scores
    sd, engines = thin
    eng, feat = engines[precision]
    d = E.feature_width(DIV)
    w, b = eng.classifier
    assert w.dtype == b.dtype == torch.float32 and w.device == b.device == DEV and w.is_contiguous()
    assert tuple(w.shape) == (1008, d) == (1008, eng.d) and tuple(b.shape) == (1008,)
    assert torch.equal(w.cpu(), sd['fc.weight']) and torch.equal(b.cpu(), sd['fc.bias'])
    assert tuple(feat.shape) == (IMAGES, d, 1, 1) and feat.dtype == torch.float32
    host = feat.flatten(1).double().cpu().numpy()
    want, bounds = _ref(host, sd, 3, precision)
    assert want[0] > 1.01 and want[1] > 0
    got = inception_score(feat, w, b, splits=3)                     # [n, d, 1, 1] as the engine returns it
    _close(got, want, bounds, '%s route, 3 splits' % precision)
    assert inception_score(feat.flatten(1), w, b, splits=3) == got  # and as rows; the same bits
    scores = split_scores(feat, w, b, 3)
    assert scores.dtype == torch.float64 and scores.is_cuda and tuple(scores.shape) == (3,)
    _close(inception_score(feat, w, b, splits=IMAGES), *_ref(host, sd, IMAGES, 'one image per split'), 'one image per split')


def test_too_few_images_and_bad_splits_raise(thin):
    from gcc_amd._lib import GccError
    from gcc_amd.metric.inception_score import inception_score
    _, engines = thin
    eng, feat = engines['bf16']
    with pytest.raises(GccError, match='25 splits needs at least 25 images, got 24'):
        inception_score(feat, *eng.classifier, splits=25)
    with pytest.raises(GccError, match='splits = 0'):
        inception_score(feat, *eng.classifier, splits=0)
    with pytest.raises(GccError, match='on the GPU'):
        inception_score(feat.cpu(), *eng.classifier)


# ---- python -m gcc_amd.metric.fid_score --inception-score --------------------------------------------------------------------------
def _folders(tmp_path, n=6, size=48):
    rng = np.random.RandomState(12)
    a, b = tmp_path / 'real', tmp_path / 'fake'
    a.mkdir(), b.mkdir()
    for folder, top in ((a, 256), (b, 180)):
        for i in range(n):
            _png(folder / ('img%03d.png' % i), rng.randint(0, rng.randint(60, top), (size, size, 3), dtype=np.uint8))
    return a, b


def test_fid_score_prints_the_score_of_the_second_folder_last(tmp_path, capsys, thin):
    """--inception-score scores with the 2048 pool features, so this is the full-width seeded network (as tests/
    test_inception_taps_gpu.py's folders are scored), on 6 + 6 small images"""
    from gcc_amd._lib import GccError
    from gcc_amd.metric import fid_score as F
    from gcc_amd.metric.inception_fid import InceptionFidEngine
    from gcc_amd.metric.inception_score import is_text
    sd = E.seeded(1, 31)
    sd['fc.weight'] = sd['fc.weight'] * 30.0
    head = {k: sd[k] for k in ('fc.weight', 'fc.bias')}
    keep = _Keep(InceptionFidEngine(sd).to(DEV).eval())
    del sd
    a, b = _folders(tmp_path)
    argv = [str(a), str(b), '--batch-size', '3']
    plain = F.main(argv, model=keep)
    out = _lines(capsys)
    assert len(plain) == 2 and out == ['FID: %.2f' % plain[0], 'KID: %.6f' % plain[1]]       # without the flag: today's output
    fake = keep.features(2, 4)                                       # two batches per folder, the second folder's
    assert fake.shape == (6, 2048)
    want, bounds = _ref(fake, head, 2, 'fid_score, second folder')
    noted = capsys.readouterr().out                                  # the reference's own print: shown again at the end
    values = F.main(argv + ['--inception-score', '--splits', '2'], model=keep)
    out = _lines(capsys)
    assert len(values) == 3 and _same(values[:2], plain)
    _close(values[2], want, bounds, 'fid_score --inception-score')
    assert out == ['FID: %.2f' % plain[0], 'KID: %.6f' % plain[1], is_text(values[2])] and out[-1] == is_text(want)
    assert out[-1].startswith('IS: ') and ' +- ' in out[-1]
    fid, kid, prdc, score = F.main(argv + ['--prdc', '--nearest-k', '2', '--inception-score', '--splits', '2'], model=keep)
    assert _lines(capsys)[-1] == out[-1] and score == values[2] and set(prdc) == {'precision', 'recall', 'density', 'coverage'}
    assert _same(F.calculate_fid_given_paths([str(a), str(b)], 3, True, 2048, model=keep, is_splits=2), (plain[0], values[2]))
    capsys.readouterr()
    # each thing it needs, named: 2048 features, activations on the second path, a native network, a classifier
    with pytest.raises(GccError, match=r'--inception-score: --dims 64.*--dims 2048'):
        F.main(argv + ['--inception-score', '--dims', '64'], model=keep)
    stat = tmp_path / 'real_stat_f.npz'
    np.savez(str(stat), mu=fake.mean(0), sigma=np.cov(fake, rowvar=False))
    with pytest.raises(GccError, match=r'--inception-score: .*real_stat_f\.npz holds statistics'):
        F.main([str(a), str(stat), '--inception-score'], model=keep)
    assert len(F.main([str(stat), str(b), '--batch-size', '3', '--inception-score', '--splits', '2'], model=keep)) == 3      # the FIRST may
    assert _lines(capsys)[-1] == out[-1]
    with pytest.raises(GccError, match='--inception-score: the network is a TorchScript archive'):
        F.main(argv + ['--inception-score'], model=lambda x: keep.net(x))
    no_head = InceptionFidEngine({k: v for k, v in thin[0].items() if not k.startswith('fc.')}, resize=RESIZE).to(DEV)
    with pytest.raises(GccError, match=r'--inception-score: .*no fc\.weight / fc\.bias'):
        F.main(argv + ['--inception-score'], model=no_head)
    with pytest.raises(GccError, match='--splits = 0'):
        F.main(argv + ['--inception-score', '--splits', '0'], model=keep)
    print(noted)


# ---- GCC_FID_IS through the scorer and the evaluator -------------------------------------------------------------------------------
def _stat(path, d, seed):
    act = np.random.RandomState(seed).rand(300, d) * 0.5
    np.savez(str(path), mu=np.mean(act, axis=0), sigma=np.cov(act, rowvar=False))


def test_scorer_keeps_features_without_a_feature_file_and_scores_every_slot(tmp_path, monkeypatch, thin):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import fid_eval as FE
    from gcc_amd.metric import inception_score as S
    sd, engines = thin
    eng = engines['bf16'][0]
    d = E.feature_width(DIV)
    _stat(tmp_path / 'real_stat_A.npz', d, 1)
    _stat(tmp_path / 'real_stat_B.npz', d, 2)
    assert not list(tmp_path.glob('real_act*.npz'))
    opt = SimpleNamespace(model='cyclegan', dataroot=str(tmp_path), direction='AtoB')
    model = SimpleNamespace(device=DEV)
    monkeypatch.delenv(S.ENV, raising=False)
    off = FE.fid_evaluator(eng, batch_size=4).scorer(model, opt)
    assert off.inception_score() is None and off.kid() is None and not any(st.keep_features for st in off.stats)
    monkeypatch.setenv(S.ENV, '2')
    sc = FE.fid_evaluator(eng, batch_size=4).scorer(model, opt)
    assert sc.is_splits == 2 and sc.tags == ['AtoB', 'BtoA'] and not sc.with_kid
    rng = np.random.RandomState(3)
    for i in range(6):
        for slot in (0, 1):
            sc.add('img%d' % i, torch.from_numpy(rng.randint(0, 256, (40, 40, 3), dtype=np.uint8)).to(DEV), slot)
    assert len(sc.result()) == 2
    got = sc.inception_score()
    assert sc.kid() is None and sc.prdc() is None and len(got) == 2 and got[0] != got[1]
    wants = []
    for st, pair, tag in zip(sc.stats, got, sc.tags):
        rows = st.features.rows()
        assert tuple(rows.shape) == (6, d)
        want, bounds = _ref(rows.double().cpu().numpy(), sd, 2, tag)
        _close(pair, want, bounds, tag)
        wants.append(want)
    assert FE.is_line(got, sc.tags, 'cyclegan') == 'AtoB %s | BtoA %s' % (S.is_text(wants[0]), S.is_text(wants[1]))
    # refused when the scorer is made: a bad value, a network that stops below the pool features, one without the classifier
    monkeypatch.setenv(S.ENV, 'ten')
    with pytest.raises(GccError, match='GCC_FID_IS=ten'):
        FE.fid_evaluator(eng, batch_size=4).scorer(model, opt)
    monkeypatch.setenv(S.ENV, '2')
    from gcc_amd.metric.inception_fid import InceptionFidEngine
    narrow = InceptionFidEngine(sd, resize=RESIZE, output_blocks=(1,), pooled=True)
    with pytest.raises(GccError, match='GCC_FID_IS=2: the network stops at %d features' % narrow.d):
        FE.fid_evaluator(narrow, batch_size=4).scorer(model, opt)
    with pytest.raises(GccError, match='GCC_FID_IS=2: the network is a TorchScript archive'):
        FE.fid_evaluator(torch.nn.Identity(), batch_size=4).scorer(model, opt)


def test_pix2pix_evaluator_logs_the_line_last_and_only_when_asked(tmp_path, monkeypatch, thin):
    from gcc_amd.metric import fid_eval as FE
    from gcc_amd.metric import inception_score as S
    from .test_kid_score_gpu import _argv, _model, _pix2pix_root
    sd, engines = thin
    root = _pix2pix_root(tmp_path)
    _stat(root / 'real_stat_B.npz', E.feature_width(DIV), 1)
    model, opt = _model(_argv('pix2pix', root, tmp_path))
    monkeypatch.delenv(S.ENV, raising=False)
    log = _Log()
    (value, tag), = FE.fid_evaluator(engines['bf16'][0], log, batch_size=4)(model, opt)
    assert log.lines == ['FID: %.2f' % value]                        # today's log
    monkeypatch.setenv(S.ENV, '3')
    keep, log3 = _Keep(engines['bf16'][0]), _Log()
    scores = FE.fid_evaluator(keep, log3, batch_size=4)(model, opt)
    assert [t for _, t in scores] == [tag] and scores[0][0] == pytest.approx(value, rel=1e-9)         # chosen by FID, as before
    assert len(log3.lines) == 2 and log3.lines[0] == log.lines[0]
    want, bounds = _ref(keep.features(), sd, 3, 'pix2pix evaluator')
    assert keep.features().shape == (6, E.feature_width(DIV))
    assert log3.lines[1] == S.is_text(want) == FE.is_line([want], [tag], 'pix2pix')
