"""KID and the path-based FID end to end (gcc_amd.metric.kid_score, fid_score, get_real_stat, fid_eval): the estimate against a
numpy float64 restatement within the bound derived in tests/_kid.py, the feature store, image folders / statistics files /
feature files scored against each other, the module's command line, and the KID line of the evaluators.

The Inception network is the stand-in of tests/test_fid_eval_gpu.py, declared again here: a fixed-seed 1 x 1 projection 3 -> d,
ReLU, adaptive average pool."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from oracle import metric_oracle as M

from . import _kid as K

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 65


class _StandIn(torch.nn.Module):
    def __init__(self, pool: int = 1, d: int = D):
        super().__init__()
        self.pool = pool
        self.proj = torch.nn.Conv2d(3, d, 1)
        g = torch.Generator().manual_seed(29)
        with torch.no_grad():
            self.proj.weight.copy_(torch.randn(self.proj.weight.shape, generator=g))
            self.proj.bias.copy_(torch.randn(d, generator=g) * 0.5 - 0.5)

    def forward(self, x):
        return [torch.nn.functional.adaptive_avg_pool2d(torch.relu(self.proj(x)), self.pool)]


class _Keep:
    """a plain callable around the network that keeps every batch it receives and returns"""

    def __init__(self, net):
        self.net, self.inputs, self.outputs = net, [], []

    def __call__(self, x):
        y = self.net(x)
        self.inputs.append(x.clone())
        self.outputs.append(y[0].clone())
        return y

    def activations(self, lo=0, hi=None):
        return torch.cat([o.mean((2, 3)) for o in self.outputs[lo:hi]]).double().cpu().numpy()


def _inception(tmp_path, pool=1, d=D):
    path = tmp_path / ('inception%d_%d.pt' % (pool, d))
    torch.jit.script(_StandIn(pool, d)).save(str(path))
    return path


def _real_act(seed, n=40):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        return _StandIn()(torch.rand(n, 3, 8, 8, generator=g))[0].reshape(n, D).float()


def _real_files(root, stat_name, seed, label=''):
    """real_stat*.npz and the real_act*.npz beside it, of the stand-in on unrelated random images"""
    from gcc_amd.metric.kid_score import features_name, save_features
    act = _real_act(seed)
    a = act.double().numpy()
    np.savez(str(root / stat_name), mu=np.mean(a, axis=0), sigma=np.cov(a, rowvar=False))
    save_features(features_name(str(root / stat_name)), act, label)
    return a


def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(str(path))


def _close(got, ref, bound, what):
    print('%s: %.12g, float64 restatement %.12g, err / bound %.3g' % (what, got, ref, abs(got - ref) / bound))
    assert np.isfinite(got) and abs(got - ref) <= bound, (what, got, ref, bound)
    assert bound < 1e-6 * max(abs(ref), 1e-3)                       # the bound is a statement about rounding, not a tolerance


# ---- the estimate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ((120, 140, 65), (7, 5, 3)), ids=lambda c: 'x'.join(map(str, c)))
def test_polynomial_mmd2_against_float64(case):
    from gcc_amd.metric import kid_score as S
    m, n, d = case
    rng = np.random.RandomState(m)
    X = (np.abs(rng.standard_normal((m, d))) * 0.5).astype(np.float32)
    Y = (np.abs(rng.standard_normal((n, d))) * 0.7 + 0.1).astype(np.float32)
    ref, bound = K.kid_ref(X.astype(np.float64), Y.astype(np.float64))
    Xd, Yd = torch.from_numpy(X).to(DEV), torch.from_numpy(Y).to(DEV)
    got = S.polynomial_mmd2(Xd, Yd)
    assert isinstance(got, float) and ref > 1e-3
    _close(got, ref, bound, 'KID %dx%dx%d' % case)
    # a cached self term gives the same bits as a recomputed one, on either side, and launches one sum less
    from gcc_amd import ops
    sx, sy = S.polynomial_self_sum(Xd), S.polynomial_self_sum(Yd)
    before = ops.lib().gcc_launch_count(0)
    assert S.polynomial_mmd2(Xd, Yd, self_x=sx) == got
    assert ops.lib().gcc_launch_count(0) == before + 4
    assert S.polynomial_mmd2(Xd, Yd, self_y=sy) == got and S.polynomial_mmd2(Xd, Yd, sx, sy) == got
    # f64 rows, [n, d, 1, 1] batches and the other order of the arguments
    assert S.polynomial_mmd2(Xd.double(), Yd[:, :, None, None]) == got
    _close(S.polynomial_mmd2(Yd, Xd), ref, bound, 'KID swapped')
    assert S.polynomial_mmd2(Xd, Xd) < 0                              # a set against itself: the unbiased estimate is below zero


def test_fewer_than_two_rows_or_unlike_widths_raise():
    from gcc_amd._lib import GccError
    from gcc_amd.metric import kid_score as S
    X = torch.rand(4, 6, device=DEV)
    for a, b in ((X[:1], X), (X, X[:1])):
        with pytest.raises(GccError, match='at least 2'):
            S.polynomial_mmd2(a, b)
    with pytest.raises(GccError, match='at least 2'):
        S.polynomial_self_sum(X[:1])
    with pytest.raises(GccError, match='against'):
        S.polynomial_mmd2(X, X[:, :5])
    with pytest.raises(GccError, match='on the GPU'):
        S.polynomial_mmd2(X.cpu(), X)


def test_feature_store_in_batches_equals_the_one_shot_tensor():
    from gcc_amd._lib import GccError
    from gcc_amd.metric.kid_score import FeatureStore
    g = torch.Generator().manual_seed(1)
    act = torch.rand(1 + 50 + 50 + 23, D, generator=g).to(DEV)
    st = FeatureStore(D, DEV, capacity=8)
    assert st.rows().shape == (0, D)
    st.append(act[:1])
    st.append(act[1:51, :, None, None])                     # what the network returns
    st.append(act[51:101])
    first = st.rows()
    st.append(act[101:])
    assert st.n == 124 and st.rows().dtype == torch.float32 and torch.equal(st.rows(), act)
    assert torch.equal(first, act[:101])                    # an earlier view keeps its rows
    assert st.buf.shape[0] >= 124 and st.rows().data_ptr() == st.buf.data_ptr()
    with pytest.raises(GccError, match='FeatureStore.append'):
        st.append(act[:, :5])
    with pytest.raises(GccError, match='FeatureStore.append'):
        st.append(act.double())


# ---- folders, statistics files, feature files --------------------------------------------------------------------------------
# More images than features on both sides.  The float64 reference has an error of its own: on rank-deficient covariances (fewer
# images than the stand-in's 65 features) the oracle's scipy square root comes back 3e-5 to 7e-5 relative off the value the
# symmetric eigenvalue problem gives, or within 1e-10 of it, from one seeded draw to the next (measured on the host; the kernels
# are not involved).  A bar of 1e-7 against it means something only where the oracle is the accurate one: _fid_ref asserts that.
FAKE, REAL, BATCH = 75, 100, 8
FAKE_USED, REAL_USED = FAKE // BATCH * BATCH, REAL // BATCH * BATCH


def _folders(tmp_path):
    rng = np.random.RandomState(12)
    a, b = tmp_path / 'fake', tmp_path / 'real'
    a.mkdir(), b.mkdir()
    for i in range(FAKE):                                     # batch 8: nine batches, three images dropped
        _png(a / ('img%03d.png' % i), rng.randint(0, 256, (12, 20, 3), dtype=np.uint8))
    for i in range(REAL):                                     # darker: the distance is O(1); twelve batches, four images dropped
        _png(b / ('img%03d.png' % i), rng.randint(0, 90, (12, 20, 3), dtype=np.uint8))
    (a / 'notes.txt').write_text('not an image')
    return a, b


def _fid_ref(a, b):
    """numpy float64 statistics + the oracle's distance, checked against tr sqrt(s1 s2) = sum sqrt(eig(s1^1/2 s2 s1^1/2)) from the
    symmetric eigenvalue problem: the reference's own error has to be well inside the bar it is used for"""
    (m1, s1), (m2, s2) = ((np.mean(x, axis=0), np.cov(x, rowvar=False)) for x in (a, b))
    ref = float(M.calculate_frechet_distance(m1, s1, m2, s2))
    w, V = np.linalg.eigh(s1)
    root = (V * np.sqrt(np.clip(w, 0, None))) @ V.T
    tr = np.sqrt(np.clip(np.linalg.eigvalsh(root @ s2 @ root), 0, None)).sum()
    sym = float(((m1 - m2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * tr)
    print('the oracle\'s distance %.12g, by the symmetric eigenvalue problem %.12g (rel %.2e)' % (ref, sym, abs(ref - sym) / sym))
    assert abs(ref - sym) <= 1e-8 * sym
    return ref


def test_fid_and_kid_of_two_folders_then_of_their_files(tmp_path, capsys):
    from PIL import Image
    from gcc_amd._lib import GccError
    from gcc_amd.metric import fid_score as F
    from gcc_amd.metric.kid_score import save_features
    a, b = _folders(tmp_path)
    keep = _Keep(_StandIn().to(DEV))
    fid, kid = F.calculate_fid_given_paths([str(a), str(b)], BATCH, True, D, model=keep, kid=True)
    assert capsys.readouterr().out.count('not a multiple of the batch size') == 2
    na = FAKE_USED // BATCH
    nb = na + REAL_USED // BATCH
    assert [tuple(x.shape) for x in keep.inputs] == [(BATCH, 3, 12, 20)] * nb
    # what was fed: the files of each folder by name, less the partial last batch, byte / 255
    for folder, lo, hi, used in ((a, 0, na, FAKE_USED), (b, na, nb, REAL_USED)):
        files = np.stack([np.asarray(Image.open(str(folder / ('img%03d.png' % i)))) for i in range(used)])
        want = torch.from_numpy(np.transpose(files.astype(np.float64) / 255, (0, 3, 1, 2)).astype(np.float32))
        fed = torch.cat(keep.inputs[lo:hi]).cpu()
        assert torch.equal(fed.view(torch.int32), want.view(torch.int32))
    act_a, act_b = keep.activations(0, na), keep.activations(na, nb)
    assert act_a.shape == (FAKE_USED, D) and act_b.shape == (REAL_USED, D) and min(FAKE_USED, REAL_USED) > D
    ref = _fid_ref(act_a, act_b)
    print('folders: FID %.10g, numpy float64 statistics + the oracle\'s distance %.10g (rel %.2e)' % (fid, ref, abs(fid - ref) / ref))
    assert ref > 0.05 and abs(fid - ref) <= 1e-7 * ref
    kref, kbound = K.kid_ref(act_a, act_b)
    _close(kid, kref, kbound, 'folders KID')
    assert F.calculate_fid_given_paths([str(a), str(b)], BATCH, True, D, model=keep) == fid        # the reference's return value
    # folder against a statistics file: the same FID, no KID
    stat_b = tmp_path / 'real_stat_b.npz'
    np.savez(str(stat_b), mu=np.mean(act_b, axis=0), sigma=np.cov(act_b, rowvar=False))
    fid2, kid2 = F.calculate_fid_given_paths([str(a), str(stat_b)], BATCH, True, D, model=keep, kid=True)
    assert kid2 is None and abs(fid2 - ref) <= 1e-7 * ref
    m, s = F._compute_statistics_of_path(str(stat_b), None, BATCH, D, True)
    assert np.array_equal(m, np.mean(act_b, axis=0)) and np.array_equal(s, np.cov(act_b, rowvar=False))
    # folder against a feature file, and two files against each other: no network is needed for those
    feat_a, feat_b = tmp_path / 'real_act_a.npz', tmp_path / 'real_act_b.npz'
    save_features(str(feat_a), act_a.astype(np.float32), '')
    save_features(str(feat_b), act_b.astype(np.float32), '')
    fid3, kid3 = F.calculate_fid_given_paths([str(a), str(feat_b)], BATCH, True, D, model=keep, kid=True)
    assert abs(fid3 - ref) <= 1e-7 * ref
    _close(kid3, kref, kbound, 'folder against feature file KID')

    def no_network(x):
        raise AssertionError('files alone need no network')
    fid4, kid4 = F.calculate_fid_given_paths([str(feat_a), str(feat_b)], 50, True, D, model=no_network, kid=True)
    assert abs(fid4 - ref) <= 1e-7 * ref
    _close(kid4, kref, kbound, 'feature files KID')
    stat_a = tmp_path / 'real_stat_a.npz'
    np.savez(str(stat_a), mu=np.mean(act_a, axis=0), sigma=np.cov(act_a, rowvar=False))
    fid5, kid5 = F.calculate_fid_given_paths([str(stat_a), str(stat_b)], 50, True, D, model=no_network, kid=True)
    assert kid5 is None and abs(fid5 - ref) <= 1e-7 * ref
    # get_activations: on the device, the clamp, the width check, the size check
    few = F.list_image_files(a)[:11]
    act = F.get_activations(few, keep, batch_size=50, dims=D)
    assert act.is_cuda and act.dtype == torch.float32 and act.shape == (11, D) and keep.inputs[-1].shape[0] == 11
    assert 'bigger than the datasets size' in capsys.readouterr().out
    n0 = len(keep.outputs)
    mu, sigma = F.calculate_activation_statistics(few, keep, batch_size=3, dims=D)
    full = keep.activations(n0)
    assert full.shape == (9, D)
    assert np.allclose(mu.cpu().numpy(), full.mean(0), rtol=1e-12, atol=1e-13)
    assert np.allclose(sigma.cpu().numpy(), np.cov(full, rowvar=False), rtol=1e-10, atol=1e-13)
    with pytest.raises(GccError, match='d = %d, dims = 2048' % D):
        F.get_activations(few, keep, batch_size=3, dims=2048)
    with pytest.raises(GccError, match='no CPU path'):
        F.get_activations(few, keep, batch_size=3, dims=D, cuda=False)
    _png(a / 'img003b.png', np.zeros((12, 24, 3), dtype=np.uint8))
    with pytest.raises(GccError, match='img003b.png is 24 x 12'):
        F.get_activations(F.list_image_files(a), keep, batch_size=5, dims=D)
    with pytest.raises(RuntimeError, match='Invalid path'):
        F.calculate_fid_given_paths([str(a), str(tmp_path / 'nowhere')], BATCH, True, D, model=keep)


def test_fid_given_ims_takes_the_network_or_loads_it(tmp_path, monkeypatch):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import fid_score as F
    rng = np.random.RandomState(3)
    fake = rng.randint(0, 256, (70, 12, 20, 3)).astype(np.float64)
    real = rng.randint(0, 90, (REAL, 12, 20, 3)).astype(np.float64)
    keep = _Keep(_StandIn().to(DEV))
    fid = F.calculate_fid_given_ims(fake, real, 32, True, D, model=keep)
    assert [x.shape[0] for x in keep.inputs] == [32, 32, 6, 32, 32, 32, 4]          # every image counts here: no batch is dropped
    ref = _fid_ref(keep.activations(0, 3), keep.activations(3, 7))
    assert ref > 0.05 and abs(fid - ref) <= 1e-7 * ref
    path = _inception(tmp_path)
    monkeypatch.setenv('GCC_FID_INCEPTION', str(path))
    want = F.calculate_fid_given_ims(fake, real, 32, True, D, model=torch.jit.load(str(path), map_location=DEV))
    assert F.calculate_fid_given_ims(fake, real, 32, True, D) == want and abs(want - ref) <= 1e-5 * ref      # the scripted copy
    with pytest.raises(GccError, match='d = %d, dims = 2048' % D):
        F.calculate_fid_given_ims(fake, real, 32, True, 2048)
    monkeypatch.delenv('GCC_FID_INCEPTION')
    with pytest.raises(GccError, match='GCC_FID_INCEPTION is not set'):
        F.calculate_fid_given_ims(fake, real, 32, True, D)


def test_module_command_line_prints_both_lines(tmp_path):
    from gcc_amd.metric import fid_score as F
    a, b = _folders(tmp_path)
    inception = _inception(tmp_path, d=64)                    # a width the reference's --dims accepts
    net = torch.jit.load(str(inception), map_location=DEV)
    fid, kid = F.calculate_fid_given_paths([str(a), str(b)], BATCH, True, 64, model=net, kid=True)
    keep = _Keep(net)
    act_b = F.get_activations(F.list_image_files(b), keep, batch_size=BATCH, dims=64).double().cpu().numpy()
    stat_b = tmp_path / 'real_stat.npz'
    np.savez(str(stat_b), mu=np.mean(act_b, axis=0), sigma=np.cov(act_b, rowvar=False))
    env = dict(os.environ, PYTHONPATH=ROOT, GCC_FID_INCEPTION=str(inception))

    def run(*argv):
        r = subprocess.run([sys.executable, '-m', 'gcc_amd.metric.fid_score'] + list(argv), cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return [line for line in r.stdout.splitlines() if 'FID' in line or 'KID' in line]
    assert run(str(a), str(b), '--batch-size', str(BATCH), '--dims', '64', '-c', '0') == ['FID: %.2f' % fid, 'KID: %.6f' % kid]
    lines = run(str(a), str(stat_b), '--batch-size', str(BATCH), '--dims', '64')
    assert len(lines) == 1 and lines[0].startswith('FID: ') and abs(float(lines[0][5:]) - fid) <= 0.011


# ---- python -m gcc_amd.metric.get_real_stat --features_path ---------------------------------------------------------------------
def _pix2pix_root(tmp_path):
    root = tmp_path / 'shoes'
    rng = np.random.RandomState(4)
    (root / 'val').mkdir(parents=True)
    for i in range(6):
        _png(root / 'val' / ('pair%d.png' % i), rng.randint(0, 256, (256, 512, 3), dtype=np.uint8))
    return root


def test_get_real_stat_features_path_round_trips(tmp_path):
    from gcc_amd.metric import get_real_stat as G
    from gcc_amd.metric import kid_score as S
    root = _pix2pix_root(tmp_path)
    net = torch.jit.load(str(_inception(tmp_path)), map_location=DEV)
    plain, out, feat = tmp_path / 'plain.npz', tmp_path / 'real_stat_B.npz', tmp_path / 'real_act_B.npz'
    G.main(['--dataroot', str(root), '--output_path', str(plain)], inception=net)
    assert sorted(p.name for p in tmp_path.glob('*.npz')) == ['plain.npz']            # without the flag nothing changes
    keep = _Keep(net)
    G.main(['--dataroot', str(root), '--output_path', str(out), '--features_path', str(feat)], inception=keep)
    with np.load(str(plain)) as p, np.load(str(out)) as o:
        assert sorted(o.files) == ['mu', 'sigma'] and np.allclose(p['mu'], o['mu'], rtol=1e-6, atol=1e-9)
        assert np.allclose(p['sigma'], o['sigma'], rtol=1e-6, atol=1e-9)
    with np.load(str(feat)) as z:
        assert sorted(z.files) == ['act', 'network'] and z['act'].dtype == np.float32 and str(z['network']) == ''
        act = z['act']
    # the activations the statistics were built from
    assert act.shape == (6, D) and np.array_equal(act.astype(np.float64), keep.activations())
    with np.load(str(out)) as o:
        assert np.allclose(o['mu'], act.astype(np.float64).mean(0), rtol=1e-12, atol=1e-13)
    got, label = S.load_features(str(feat), D, DEV)
    assert label == '' and got.is_cuda and np.array_equal(got.cpu().numpy(), act)


# ---- the evaluators' KID line -------------------------------------------------------------------------------------------------
def _argv(model, root, tmp_path):
    return ['--dataroot', str(root), '--model', model, '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--name', 'exp',
            '--checkpoints_dir', str(tmp_path / 'ck'), '--print_freq', '1000']


def _model(argv):
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    opt = options.parse(argv)
    opt.isTrain = True
    torch.manual_seed(31)
    model = get_model_class(opt)(opt)
    model.model_eval()
    return model, opt


def _stat_only(root, name, seed):
    a = _real_act(seed).double().numpy()
    np.savez(str(root / name), mu=np.mean(a, axis=0), sigma=np.cov(a, rowvar=False))


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, line):
        self.lines.append(line)


def test_pix2pix_evaluator_logs_kid_only_beside_a_feature_file(tmp_path):
    from gcc_amd.metric import fid_eval as E
    root = _pix2pix_root(tmp_path)
    _stat_only(root, 'real_stat_B.npz', 1)
    model, opt = _model(_argv('pix2pix', root, tmp_path))
    net = torch.jit.load(str(_inception(tmp_path)), map_location=DEV)
    log = _Log()
    evaluate = E.fid_evaluator(net, log, batch_size=4)
    (value, tag), = evaluate(model, opt)
    assert log.lines == ['FID: %.2f' % value] and evaluate.state['kid'] == {}        # today's log, nothing kept
    real = _real_files(root, 'real_stat_B.npz', 1)                   # the same statistics, now with their activations beside them
    keep, log2 = _Keep(net), _Log()
    evaluate2 = E.fid_evaluator(keep, log2, batch_size=4)
    made = []
    real_kid = E.FidScorer.kid
    E.FidScorer.kid = lambda self: (made.append(self), real_kid(self))[1]
    try:
        with warnings.catch_warnings():
            warnings.filterwarnings('error', message='.*activations of two networks')      # the labels agree: no warning
            scores = evaluate2(model, opt)
            again = evaluate2(model, opt)
    finally:
        E.FidScorer.kid = real_kid
    assert scores == again and [t for _, t in scores] == [tag] and scores[0][0] == pytest.approx(value, rel=1e-9)     # the return value is untouched
    assert len(log2.lines) == 4 and log2.lines[0] == log2.lines[2] == 'FID: %.2f' % value and log2.lines[1] == log2.lines[3]
    assert log2.lines[1].startswith('KID: ')
    fake = keep.activations(0, 2)                                    # the first evaluation's two batches
    ref, bound = K.kid_ref(real, fake)
    kid, = real_kid(made[0])
    _close(kid, ref, bound, 'pix2pix evaluator KID')
    assert log2.lines[1] == 'KID: %.6f' % kid
    assert made[0].stats[0].features.n == 6 and list(evaluate2.state['kid']) == [str(root / 'real_act_B.npz')]


def test_cyclegan_evaluator_logs_both_kids(tmp_path):
    from gcc_amd.metric import fid_eval as E
    root = tmp_path / 'h2z'
    rng = np.random.RandomState(5)
    for sub, stem in (('testA', 'h'), ('testB', 'z')):
        (root / sub).mkdir(parents=True)
        for i in range(5):
            _png(root / sub / ('%s%d.png' % (stem, i)), rng.randint(0, 256, (256, 256, 3), dtype=np.uint8))
    _stat_only(root, 'real_stat_B.npz', 2)
    _stat_only(root, 'real_stat_A.npz', 3)
    model, opt = _model(_argv('cyclegan', root, tmp_path))
    net = torch.jit.load(str(_inception(tmp_path, pool=2)), map_location=DEV)
    log = _Log()
    scores = E.fid_evaluator(net, log, batch_size=4)(model, opt)
    assert log.lines == ['AtoB FID: %.2f | BtoA FID: %.2f' % (scores[0][0], scores[1][0])]
    real_b = _real_files(root, 'real_stat_B.npz', 2)
    one = E.fid_evaluator(net, log, batch_size=4)(model, opt)
    assert [v for v, _ in one] == pytest.approx([v for v, _ in scores], rel=1e-9) and len(log.lines) == 2      # one of two files: no KID
    real_a = _real_files(root, 'real_stat_A.npz', 3)
    log2, made = _Log(), []
    real_init = E.FidScorer.__init__
    E.FidScorer.__init__ = lambda self, *a, **k: (real_init(self, *a, **k), made.append(self))[0]
    try:
        got = E.fid_evaluator(net, log2, batch_size=4)(model, opt)
    finally:
        E.FidScorer.__init__ = real_init
    assert [t for _, t in got] == ['AtoB', 'BtoA'] and [v for v, _ in got] == pytest.approx([v for v, _ in scores], rel=1e-9)
    assert len(log2.lines) == 2 and log2.lines[0] == log.lines[0]
    kids = []
    for st, real, what in zip(made[0].stats, (real_b, real_a), ('AtoB', 'BtoA')):
        fake = st.features.rows().double().cpu().numpy()
        assert fake.shape == (5, D)
        ref, bound = K.kid_ref(real, fake)
        kids.append(ref)
        _close(made[0].kid()[len(kids) - 1], ref, bound, 'cyclegan %s KID' % what)
    assert log2.lines[1] == 'AtoB KID: %.6f | BtoA KID: %.6f' % tuple(made[0].kid())
    assert abs(kids[0] - kids[1]) > 1e-6


def test_scorer_warns_once_about_another_networks_features(tmp_path):
    from gcc_amd.metric import fid_eval as E
    _real_files(tmp_path, 'real_stat_B.npz', 1, label=' (native, fp32)')
    opt = type('O', (), {'model': 'pix2pix', 'direction': 'AtoB', 'dataroot': str(tmp_path)})
    keep = _Keep(_StandIn().to(DEV))
    g = torch.Generator().manual_seed(8)
    imgs = [(torch.rand(1, 3, 8, 8, generator=g) * 2 - 1).to(DEV) for _ in range(3)]
    cache = {}

    def score():
        sc = E.FidScorer(keep, opt.dataroot, E.real_stat_slots(opt), batch_size=2, kid_cache=cache)
        for i, im in enumerate(imgs):
            sc.add(i, im)
        return sc.result(), sc.kid()
    with pytest.warns(UserWarning, match='activations of two networks') as rec:
        first = score()
    assert len([w for w in rec if 'activations of two networks' in str(w.message)]) == 1
    with warnings.catch_warnings():
        warnings.filterwarnings('error', message='.*activations of two networks')
        assert score() == first                                      # from the cache: the same bits, no second warning
    fake = keep.activations(0, 2)
    ref, bound = K.kid_ref(_real_act(1).double().numpy(), fake)
    _close(first[1][0], ref, bound, 'scorer KID')
