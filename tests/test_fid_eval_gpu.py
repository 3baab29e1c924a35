"""The per-epoch FID evaluation on the GPU (gcc_amd.metric.fid_eval over gcc_fid_input and the streamed statistics) for Pix2Pix off
Cityscapes, CycleGAN and SAGAN: what the network is fed (bit for bit the host route's tensor2imgs(model.infer(..)) / 255), what
comes back (the Frechet distance of numpy's float64 statistics of the very activations the network returned), the slot tags,
and the ways in: gcc_amd.train.main, python -m gcc_amd.test and python -m gcc_amd.metric.get_real_stat.

The Inception network is a stand-in scripted into tmp_path: a fixed-seed 1 x 1 projection 3 -> 65, ReLU, adaptive average pool."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import metric_oracle as M

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 65


class _StandIn(torch.nn.Module):
    """returns [features] as InceptionV3([3]) does; ``pool`` > 1 leaves a map for the evaluator to average"""

    def __init__(self, pool: int = 1):
        super().__init__()
        self.pool = pool
        self.proj = torch.nn.Conv2d(3, D, 1)
        g = torch.Generator().manual_seed(29)
        with torch.no_grad():
            self.proj.weight.copy_(torch.randn(self.proj.weight.shape, generator=g))
            self.proj.bias.copy_(torch.randn(D, generator=g) * 0.5 - 0.5)

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

    def activations(self):
        return torch.cat([o.mean((2, 3)) for o in self.outputs]).double().cpu().numpy()


def _inception(tmp_path, pool=1):
    path = tmp_path / ('inception%d.pt' % pool)
    torch.jit.script(_StandIn(pool)).save(str(path))
    return path


def _real_stat(path, seed):
    """statistics of the stand-in on unrelated random images: the distance to a generator's is O(1), not near zero"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        act = _StandIn()(torch.rand(200, 3, 8, 8, generator=g))[0].reshape(200, D).double().numpy()
    np.savez(str(path), mu=np.mean(act, axis=0), sigma=np.cov(act, rowvar=False))


def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(str(path))


def _pix2pix_root(tmp_path, train=False):
    root = tmp_path / 'shoes'
    rng = np.random.RandomState(4)
    for phase in ('val', 'train') if train else ('val',):
        (root / phase).mkdir(parents=True)
        for i in range(6):
            _png(root / phase / ('pair%d.png' % i), rng.randint(0, 256, (256, 512, 3), dtype=np.uint8))
    _real_stat(root / 'real_stat_B.npz', 1)
    return root


def _cyclegan_root(tmp_path):
    root = tmp_path / 'h2z'
    rng = np.random.RandomState(5)
    for sub, stem in (('testA', 'h'), ('testB', 'z')):
        (root / sub).mkdir(parents=True)
        for i in range(6):
            _png(root / sub / ('%s%d.png' % (stem, i)), rng.randint(0, 256, (256, 256, 3), dtype=np.uint8))
    _real_stat(root / 'real_stat_B.npz', 2)
    _real_stat(root / 'real_stat_A.npz', 3)
    return root


def _sagan_root(tmp_path):
    root = tmp_path / 'faces'
    (root / 'train').mkdir(parents=True)
    rng = np.random.RandomState(6)
    for i in range(25):
        _png(root / 'train' / ('f%02d.png' % i), rng.randint(0, 256, (170, 180, 3), dtype=np.uint8))
    _real_stat(root / 'real_stat.npz', 4)
    return root


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


def _record_infer(model, monkeypatch):
    """every infer_nhwc call's result as model.infer returns it (NCHW fp32, on the host), in call order, with the generator"""
    from gcc_amd import ops
    calls = []
    real = model.infer_nhwc

    def infer_nhwc(*a, **k):
        view = real(*a, **k)
        calls.append((a[1] if len(a) > 1 else k.get('generator', 'A'), ops.nhwc_to_nchw(view, 3).cpu()))
        return view
    monkeypatch.setattr(model, 'infer_nhwc', infer_nhwc)
    return calls


def _host_input(fakes):
    """the host route: util.tensor2imgs(fakes) / 255 in float64, then FloatTensor (metric/__init__.py:8-14, fid_score.py:184-190)"""
    from gcc_amd.utils import util
    return torch.from_numpy(np.transpose(util.tensor2imgs(torch.cat(fakes)).astype(np.float64) / 255, (0, 3, 1, 2)).astype(np.float32))


def _reference_fid(keep, npz_path):
    act = keep.activations()
    with np.load(str(npz_path)) as z:
        return float(M.calculate_frechet_distance(z['mu'], z['sigma'], np.mean(act, axis=0), np.cov(act, rowvar=False)))


def _check_slot(keep, fakes, npz_path, value, what):
    fed = torch.cat(keep.inputs).cpu()
    want = _host_input(fakes)
    assert fed.shape == want.shape and torch.equal(fed.view(torch.int32), want.view(torch.int32)), what
    ref = _reference_fid(keep, npz_path)
    print('%s: FID %.10g, numpy float64 statistics + the oracle\'s distance on the same activations %.10g (rel %.2e)'
          % (what, value, ref, abs(value - ref) / ref))
    assert ref > 0.05 and abs(value - ref) <= 1e-7 * ref, (what, value, ref)


def test_pix2pix_evaluator(tmp_path, monkeypatch):
    from gcc_amd import test as gtest
    from gcc_amd.data import create_dataset
    from gcc_amd.metric import fid_eval as E
    root = _pix2pix_root(tmp_path)
    model, opt = _model(_argv('pix2pix', root, tmp_path))
    keep = _Keep(torch.jit.load(str(_inception(tmp_path)), map_location=DEV))
    lines = []
    evaluate = E.fid_evaluator(keep, type('L', (), {'info': staticmethod(lines.append)}), batch_size=4)
    calls = _record_infer(model, monkeypatch)
    marked = []
    real_record = torch.Tensor.record_stream
    monkeypatch.setattr(torch.Tensor, 'record_stream', lambda t, st: (marked.append(st), real_record(t, st))[1])
    (value, tag), = evaluate(model, opt)
    monkeypatch.undo()
    assert len(marked) == 12 and all(st == torch.cuda.current_stream(DEV) for st in marked)      # A and B of six batches
    assert tag == opt.direction == 'AtoB' and lines == ['FID: %.2f' % value]
    assert [tuple(x.shape) for x in keep.inputs] == [(4, 3, 256, 256), (2, 3, 256, 256)]      # a full batch and the remainder
    fakes = [f for _, f in calls]
    assert len(fakes) == 6
    # the reference's image set: the val split in the loader's order, one image per A path
    again = [model.infer(data).cpu() for data in create_dataset(gtest.test_overrides(opt), model.device)]
    assert len(again) == 6 and all(torch.equal(a, b) for a, b in zip(again, fakes))
    _check_slot(keep, fakes, root / 'real_stat_B.npz', value, 'pix2pix')
    # BtoA reads the other statistics and feeds the other half
    opt.direction = 'BtoA'
    model.opt.direction = 'BtoA'
    _real_stat(root / 'real_stat_A.npz', 9)
    keep2 = _Keep(keep.net)
    (v2, tag2), = E.fid_evaluator(keep2, batch_size=4)(model, opt)
    assert tag2 == 'BtoA' and abs(v2 - _reference_fid(keep2, root / 'real_stat_A.npz')) <= 1e-7 * v2 and v2 != value


def test_cyclegan_evaluator(tmp_path, monkeypatch):
    from gcc_amd import test as gtest
    from gcc_amd.data import create_dataset
    from gcc_amd.metric import fid_eval as E
    root = _cyclegan_root(tmp_path)
    model, opt = _model(_argv('cyclegan', root, tmp_path))
    net = torch.jit.load(str(_inception(tmp_path, pool=2)), map_location=DEV)        # a 2 x 2 map: the evaluator averages it
    keeps = {'A': _Keep(net), 'B': _Keep(net)}
    evaluate = E.fid_evaluator(net, batch_size=4)
    made = []

    class Spy(E.FidScorer):                # one keeper per slot
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.stats[0].inception, self.stats[1].inception = keeps['A'], keeps['B']
            made.append(self)
    monkeypatch.setattr(E, 'FidScorer', Spy)
    calls = _record_infer(model, monkeypatch)
    scores = evaluate(model, opt)
    monkeypatch.undo()
    assert [t for _, t in scores] == ['AtoB', 'BtoA'] and len(made) == 1
    assert [g for g, _ in calls] == ['A', 'B'] * 6
    for gen, slot, npz in (('A', 0, 'real_stat_B.npz'), ('B', 1, 'real_stat_A.npz')):
        fakes = [f for g, f in calls if g == gen]
        again = [model.infer(data, gen).cpu() for data in create_dataset(gtest.test_overrides(opt), model.device)]
        assert all(torch.equal(a, b) for a, b in zip(again, fakes))
        assert keeps[gen].outputs[0].shape[2:] == (2, 2)
        _check_slot(keeps[gen], fakes, root / npz, scores[slot][0], 'cyclegan generator %s' % gen)
    assert scores[0][0] != scores[1][0]


def test_sagan_evaluator_scores_a_tenth(tmp_path, monkeypatch):
    from gcc_amd.metric import fid_eval as E
    root = _sagan_root(tmp_path)
    model, opt = _model(_argv('sagan', root, tmp_path))
    keep = _Keep(torch.jit.load(str(_inception(tmp_path)), map_location=DEV))
    lines = []
    evaluate = E.fid_evaluator(keep, type('L', (), {'info': staticmethod(lines.append)}), batch_size=2)
    calls = _record_infer(model, monkeypatch)
    (value, tag), = evaluate(model, opt)
    monkeypatch.undo()
    assert tag == opt.direction and lines == ['FID: %.2f' % value]
    assert len(calls) == 3 == E.sagan_count(25)                     # i = 0, 1, 2; 3 > 25 * 0.1 stops
    assert [tuple(x.shape) for x in keep.inputs] == [(2, 3, 64, 64), (1, 3, 64, 64)]
    _check_slot(keep, [f for _, f in calls], root / 'real_stat.npz', value, 'sagan')


def test_scorer_counts_a_repeated_key_once_and_names_its_refusals(tmp_path):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import fid_eval as E
    _real_stat(tmp_path / 'real_stat_B.npz', 1)
    opt = type('O', (), {'model': 'pix2pix', 'direction': 'AtoB', 'dataroot': str(tmp_path)})
    keep = _Keep(_StandIn().to(DEV))
    g = torch.Generator().manual_seed(8)
    imgs = [(torch.rand(1, 3, 8, 8, generator=g) * 0.6 - 1).to(DEV) for _ in range(3)]     # dark: far from the statistics' images
    sc = E.FidScorer(keep, opt.dataroot, E.real_stat_slots(opt), batch_size=4)
    for key, im in (('a', imgs[0]), ('b', imgs[1]), ('a', imgs[2]), ('c', imgs[2])):
        sc.add(key, im)
    value, = sc.result()
    assert torch.cat(keep.inputs).shape[0] == 3
    ref = _reference_fid(keep, tmp_path / 'real_stat_B.npz')
    assert ref > 1.0 and abs(value - ref) <= 1e-7 * ref, (value, ref)
    # an output that is not 4-D fp32
    bad = E.FidScorer(lambda x: [x.mean((2, 3))], opt.dataroot, E.real_stat_slots(opt), batch_size=1)
    with pytest.raises(GccError, match='fp32 activations'):
        bad.add('a', imgs[0])
    half = E.FidScorer(lambda x: [x.half()], opt.dataroot, E.real_stat_slots(opt), batch_size=1)
    with pytest.raises(GccError, match='fp32 activations'):
        half.add('a', imgs[0])
    # statistics of another width
    three = E.FidScorer(lambda x: [x], opt.dataroot, E.real_stat_slots(opt), batch_size=2)
    three.add('a', imgs[0])
    three.add('b', imgs[1])
    with pytest.raises(GccError, match='d = 3'):
        three.result()


# ---- gcc_amd.train.main -----------------------------------------------------------------------------------------------------
def test_train_main_logs_fid_and_keeps_best(tmp_path, monkeypatch):
    from gcc_amd import train
    root = _pix2pix_root(tmp_path, train=True)
    monkeypatch.setenv('GCC_FID_INCEPTION', str(_inception(tmp_path)))
    seen = []
    real = train.BestRecord.update
    monkeypatch.setattr(train.BestRecord, 'update', lambda self, metric, epoch, index=0: (seen.append((metric, epoch, index)),
                                                                                          real(self, metric, epoch, index))[1])
    # 250 epochs in the schedule, an evaluation after each (save_epoch_freq 1): the run starts at 248
    model = train.main(_argv('pix2pix', root, tmp_path) + ['--epoch_count', '248', '--batch_size', '1'])
    torch.cuda.synchronize()
    assert model is not None
    log = (tmp_path / 'ck' / 'exp' / 'logger.log').read_text()
    assert 'FID evaluation every 1 epochs with the Inception network' in log
    values = re.findall(r'^.*\bFID: ([0-9.]+)$', log, re.M)
    assert len(values) == 3, log[-2000:]
    assert [(e, i) for _, e, i in seen] == [(248, 0), (249, 0), (250, 0)]
    assert ['%.2f' % v for v, _, _ in seen] == values
    best = list((tmp_path / 'ck' / 'exp' / 'checkpoints').glob('model_best_*.pth'))
    assert [b.name for b in best] == ['model_best_AtoB.pth']
    low = min(v for v, _, _ in seen)
    want_epoch = [e for v, e, _ in seen if v == low][-1]                  # smaller is better; a tie counts as an improvement
    assert re.search(r'slot 0: best epoch %d %.2f / last %s' % (want_epoch, low, values[-1]), log), log[-500:]


def test_train_main_without_the_variable_says_why_and_evaluates_nothing(tmp_path, monkeypatch):
    from gcc_amd import train
    root = _pix2pix_root(tmp_path, train=True)
    monkeypatch.delenv('GCC_FID_INCEPTION', raising=False)
    train.main(_argv('pix2pix', root, tmp_path) + ['--epoch_count', '250', '--batch_size', '1'])
    torch.cuda.synchronize()
    log = (tmp_path / 'ck' / 'exp' / 'logger.log').read_text()
    assert log.count('no FID evaluation: GCC_FID_INCEPTION is not set') == 1
    assert not re.search(r'\bFID: [0-9]', log) and 'evaluation slot' not in log
    assert not list((tmp_path / 'ck' / 'exp' / 'checkpoints').glob('model_best_*.pth'))


# ---- python -m gcc_amd.test ---------------------------------------------------------------------------------------------------
def _cli(argv, ckpt, inception):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop('GCC_FID_INCEPTION', None)
    if inception is not None:
        env['GCC_FID_INCEPTION'] = str(inception)
    r = subprocess.run([sys.executable, '-m', 'gcc_amd.test'] + argv + ['--pretrain_path', ckpt], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _pngs(tmp_path):
    out = tmp_path / 'ck' / 'exp' / 'test_results'
    return sorted(str(p.relative_to(out)) for p in out.rglob('*.png'))


def test_cli_pix2pix_prints_fid_after_the_pngs(tmp_path):
    from gcc_amd.metric import fid_eval as E
    root = _pix2pix_root(tmp_path)
    argv = _argv('pix2pix', root, tmp_path)
    model, opt = _model(argv)
    model.save_models(1, str(tmp_path / 'save'))
    inception = _inception(tmp_path)
    value = E.fid_evaluator(torch.jit.load(str(inception), map_location=DEV))(model, opt)[0][0]
    out = _cli(argv, str(tmp_path / 'save' / 'model_1.pth'), inception)
    assert ('FID: %.2f' % value) in out.splitlines(), out[-2000:]
    names = ['pair%d' % i for i in range(6)]
    assert _pngs(tmp_path) == sorted([n + '.png' for n in names] + [os.path.join('fake_B', n + '_fake_B.png') for n in names])


def test_cli_cyclegan_prints_both_fids_and_writes_the_same_pngs(tmp_path):
    import shutil
    from gcc_amd.metric import fid_eval as E
    root = _cyclegan_root(tmp_path)
    argv = _argv('cyclegan', root, tmp_path)
    model, opt = _model(argv)
    model.save_models(1, str(tmp_path / 'save'))
    ckpt = str(tmp_path / 'save' / 'model_1.pth')
    inception = _inception(tmp_path)
    (a, _), (b, _) = E.fid_evaluator(torch.jit.load(str(inception), map_location=DEV))(model, opt)
    out = _cli(argv, ckpt, inception)
    assert ('AtoB FID: %.2f | BtoA FID: %.2f' % (a, b)) in out.splitlines(), out[-2000:]
    with_fid = _pngs(tmp_path)
    assert len(with_fid) == 12 and not any('fake_A' in f for f in with_fid)
    shutil.rmtree(str(tmp_path / 'ck' / 'exp' / 'test_results'))
    out = _cli(argv, ckpt, None)
    assert 'FID:' not in out and 'no FID evaluation: GCC_FID_INCEPTION is not set' in out
    assert _pngs(tmp_path) == with_fid


# ---- python -m gcc_amd.metric.get_real_stat -----------------------------------------------------------------------------------
def test_get_real_stat_on_the_aligned_root(tmp_path):
    from PIL import Image
    from gcc_amd.data import create_dataset
    from gcc_amd.metric import get_real_stat as G
    from gcc_amd.utils import util
    root = _pix2pix_root(tmp_path)
    keep = _Keep(torch.jit.load(str(_inception(tmp_path)), map_location=DEV))
    out = tmp_path / 'made.npz'
    argv = ['--dataroot', str(root), '--output_path', str(out)]
    assert G.main(argv, inception=keep) == str(out)
    assert [x.shape[0] for x in keep.inputs] == [6]                         # batch 32, the reference's value
    # what was fed: tensor2imgs of the loader's own tensors (direction AtoB: the B half), over 255
    loader = [data['B'].cpu() for data in create_dataset(G.parse(argv), DEV)]
    fed = keep.inputs[0].cpu()
    want = _host_input(loader)
    assert torch.equal(fed.view(torch.int32), want.view(torch.int32))
    # ... which are not the file's bytes: a byte that does not survive (b / 255 - 0.5) / 0.5 -> tensor2imgs comes back one lower
    files = np.stack([np.asarray(Image.open(str(root / 'val' / ('pair%d.png' % i))))[:, 256:] for i in range(6)])
    drift = util.tensor2imgs(torch.cat(loader)).astype(int) - files.astype(int)
    print('get_real_stat: %d of %d bytes fed are one below the file\'s' % (int((drift == -1).sum()), drift.size))
    assert set(np.unique(drift).tolist()) == {-1, 0} and (drift == -1).sum() > 0
    # the file: numpy's statistics of the activations the network returned, f64, the reference's keys
    act = keep.activations()
    with np.load(str(out)) as z:
        assert sorted(z.files) == ['mu', 'sigma'] and z['mu'].dtype == z['sigma'].dtype == np.float64
        mu, sigma = z['mu'], z['sigma']
    mu_ref, sigma_ref = np.mean(act, axis=0), np.cov(act, rowvar=False)
    print('get_real_stat: max |mu err| %.3g, max |sigma err| %.3g' % (np.abs(mu - mu_ref).max(), np.abs(sigma - sigma_ref).max()))
    assert mu.shape == (D,) and sigma.shape == (D, D)
    assert np.allclose(mu, mu_ref, rtol=1e-12, atol=1e-13) and np.allclose(sigma, sigma_ref, rtol=1e-11, atol=1e-13)
