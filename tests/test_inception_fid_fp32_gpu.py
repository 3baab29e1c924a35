"""The native FID Inception network at the reference's own precision (InceptionFidEngine(sd, precision='fp32'),
GCC_FID_PRECISION=fp32) on the GPU: thin seeded nets against the float64 restatement (tests/_inception_f64.py) with the fp32
restatement's own error as the yardstick, repeatability, batch invariance bit for bit, launch count and slab reuse, the bf16 engine
beside it unchanged, the reference's kind of weight file end to end through builtin_inception, gcc_amd.test and get_real_stat, and
the full-width network once."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _inception_emul as E
from tests import _inception_f64 as E64

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (22, 30)
RESIZE, SHAPE = 75, (3, 3, 40, 56)           # the map goes 37, 35, 35, 17, 17, 15, 7, 3, 1: every layer kind, a 1 x 1 final map
MARGIN = 8                                   # tests/test_drn_seg_fp32_gpu.py's, for the same kernel family


def _engine(sd, *a, **kw):
    from gcc_amd.metric.inception_fid import InceptionFidEngine
    return InceptionFidEngine(sd, *a, **kw)


@pytest.fixture(scope='module')
def nets():
    """{seed: (state_dict, input, float64 features, fp32 restatement's features, fp32 engine, native features)}, computed once"""
    out = {}
    for seed in SEEDS:
        sd = E.seeded(8, seed)
        x = E.seeded_input(SHAPE, seed + 100)
        want = E64.forward64(sd, x, RESIZE)
        ref = E.forward(sd, x, RESIZE)
        eng = _engine(sd, resize=RESIZE, precision='fp32').to(DEV).eval()
        got = eng(x.to(DEV))
        assert isinstance(got, list) and len(got) == 1
        out[seed] = (sd, x, want, ref, eng, got[0].cpu())
    return out


@pytest.mark.parametrize('seed', SEEDS)
def test_thin_net_features_within_eight_times_the_fp32_restatement_s_error(nets, seed):
    """max |native fp32 - float64| over the features against 8 x max |fp32 restatement - float64|, the restatement's error measured
    here on the host.  Both sides do the same fp32 arithmetic in another order (the engine: one fixed k-ordered fmaf chain per
    output, BatchNorm folded to a scale and a shift in fp32); two equally valid host evaluations, one thread against many, already
    differ by a factor of 0.7 to 1.5 in that error.  The bf16 route is some 10^4 over this bar (1.4e-2 to 2.9e-2 against a
    yardstick of 0.7e-6 to 1.7e-6 on features of magnitude 2).
    Measured on an MI355X (profiles/r12_inception_fp32.txt): ratio 1.54 at seed 22 (1.43e-6 against the restatement's 9.28e-7)
    and 1.03 at seed 30 (1.09e-6 against 1.06e-6); the bf16 route at seed 30: 0.0169, 15957 x the yardstick."""
    sd, x, want, ref, eng, got = nets[seed]
    assert eng.precision == 'fp32'
    assert got.dtype == torch.float32 and tuple(got.shape) == (SHAPE[0], 256, 1, 1) == tuple(want.shape)
    err, yard = E64.errors(want, ref, got)
    print('seed %d: max |native fp32 - f64| %.3g, max |fp32 restatement - f64| %.3g, ratio %.2f, max |feature| %.3f'
          % (seed, err, yard, err / yard, float(want.abs().max())))
    assert yard > 0 and err <= MARGIN * yard


def test_engine_repeats_itself_is_batch_invariant_counts_its_launches_and_reuses_its_slab(nets):
    from gcc_amd import ops
    from gcc_amd._lib import GccError
    L = ops.lib()
    sd, x, want, ref, eng, got = nets[SEEDS[0]]
    xd = x.to(DEV)
    predicted = eng.infer_launches(*[int(v) for v in (x.shape[0], x.shape[2], x.shape[3])])
    steps = eng._program(x.shape[0]).steps
    assert all(st[0] in ('conv', 'pool') for st in steps)                 # no 'border' step on this route
    assert predicted == 2 + len(steps) == 1 + 94 + 13 + 1                 # resize, convs, pools, mean: one launch each
    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    again = eng(xd)[0]
    torch.cuda.synchronize()
    assert L.gcc_launch_count(1) == predicted
    assert torch.equal(again.cpu(), got)
    # a second input size: the resize kernel's work changes, nothing else -- same slab, same launch count
    slab = eng._slab.data_ptr()
    assert eng._slab.dtype == torch.float32
    big = E.seeded_input((3, 3, 90, 64), 7).to(DEV)
    L.gcc_launch_count(1)
    f_big = eng(big)[0]
    torch.cuda.synchronize()
    assert L.gcc_launch_count(1) == predicted == eng.infer_launches(3, 90, 64)
    assert eng._slab.data_ptr() == slab and torch.isfinite(f_big).all() and not torch.equal(f_big.cpu(), got)
    # no split-K anywhere: an image's features do not depend on the batch it is in, bit for bit
    for n in range(x.shape[0]):
        one = eng(xd[n:n + 1].contiguous())[0]
        assert torch.equal(one.cpu().view(torch.int32), got[n:n + 1].contiguous().view(torch.int32)), n
    assert eng._slab.data_ptr() == slab
    assert torch.equal(eng(xd)[0].cpu(), got)
    eng2 = _engine(sd, resize=RESIZE, precision='fp32').to(DEV)
    a1 = eng2(xd[:1].contiguous())[0]
    small = eng2._slab.numel()
    a2 = eng2(xd)[0]
    assert eng2._slab.numel() > small                                      # the slab grows, and only grows
    a3 = eng2(xd[:1].contiguous())[0]
    assert torch.equal(a1.cpu(), got[:1]) and torch.equal(a2.cpu(), got) and torch.equal(a3, a1)
    with pytest.raises(GccError, match='the input is on cpu'):
        eng(x)
    with pytest.raises(GccError, match=r'expected an NCHW fp32 \[N, 3, H, W\] tensor'):
        eng(xd[:, :2])


def test_bf16_engine_beside_the_fp32_one_is_the_default_engine_bit_for_bit(nets):
    sd, x, want, ref, eng, got = nets[SEEDS[1]]
    xd = x.to(DEV)
    default = _engine(sd, resize=RESIZE).to(DEV)
    named = _engine(sd, resize=RESIZE, precision='bf16').to(DEV)
    assert default.precision == named.precision == 'bf16' and named._slab_dtype == torch.bfloat16
    a, b = default(xd)[0], named(xd)[0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert named.infer_launches(3) == default.infer_launches(3) > eng.infer_launches(3)          # border copies, split-K folds
    assert torch.equal(eng(xd)[0].cpu(), got)                             # and the fp32 engine is not disturbed by them
    err16, yard = E64.errors(want, ref, a)
    print('seed %d: bf16 route max |native - f64| %.3g = %.0f x the fp32 restatement\'s error' % (SEEDS[1], err16, err16 / yard))
    assert err16 > MARGIN * yard                                          # the bar is one the bf16 route does not pass


# ---- end to end: a state_dict file in GCC_FID_INCEPTION, GCC_FID_PRECISION beside it -----------------------------------------------
def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(str(path))


def _root(tmp_path):
    """a tiny aligned root (not Cityscapes: its evaluation is FID) with real statistics of the features' width"""
    root = tmp_path / 'shoes'
    rng = np.random.RandomState(4)
    (root / 'val').mkdir(parents=True)
    for i in range(4):
        _png(root / 'val' / ('pair%d.png' % i), rng.randint(0, 256, (256, 512, 3), dtype=np.uint8))
    act = rng.rand(300, 256) * 0.5
    np.savez(str(root / 'real_stat_B.npz'), mu=np.mean(act, axis=0), sigma=np.cov(act, rowvar=False))
    weights = tmp_path / 'pt_inception_thin.pth'
    torch.save(E.seeded(8, 31), str(weights))                 # a plain state_dict, as the reference's weight file is
    return root, weights


def _argv(root, tmp_path):
    return ['--dataroot', str(root), '--model', 'pix2pix', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--name', 'exp',
            '--checkpoints_dir', str(tmp_path / 'ck'), '--print_freq', '1000']


class _Keep:
    def __init__(self, net):
        self.net, self.outputs, self.precision = net, [], net.precision

    def to(self, device):
        self.net = self.net.to(device)
        return self

    def __call__(self, x):
        y = self.net(x)
        self.outputs.append(y[0].clone())
        return y


def test_the_variable_selects_the_engine_and_the_cli_prints_its_fid(tmp_path, monkeypatch):
    from gcc_amd.metric import fid_eval as FE
    from gcc_amd.metric.inception_fid import InceptionFidEngine
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    root, weights = _root(tmp_path)
    argv = _argv(root, tmp_path)
    opt = options.parse(argv)
    opt.isTrain = True
    torch.manual_seed(31)
    model = get_model_class(opt)(opt)
    model.model_eval()
    model.save_models(1, str(tmp_path / 'save'))
    monkeypatch.setenv(FE.ENV, str(weights))
    monkeypatch.delenv(FE.PRECISION_ENV, raising=False)
    net16, why = FE.builtin_inception(opt)
    assert isinstance(net16, InceptionFidEngine) and why is None and net16.precision == 'bf16'          # unset: today's engine
    monkeypatch.setenv(FE.PRECISION_ENV, 'fp32')
    net, why = FE.builtin_inception(opt)
    assert isinstance(net, InceptionFidEngine) and why is None and net.precision == 'fp32' and net.resize == 299
    value = FE.fid_evaluator(net)(model, opt)[0][0]
    value16 = FE.fid_evaluator(net16)(model, opt)[0][0]
    print('FID of the same four images: fp32 engine %.6f, bf16 engine %.6f' % (value, value16))
    assert np.isfinite(value) and value > 0 and value != value16
    cmd = [sys.executable, '-m', 'gcc_amd.test'] + argv + ['--pretrain_path', str(tmp_path / 'save' / 'model_1.pth')]
    # the child inherits the variable; without it the same command line is tests/test_inception_fid_gpu.py's (the bf16 engine)
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert ('FID: %.2f' % value) in r.stdout.splitlines(), r.stdout[-2000:]


def test_get_real_stat_writes_the_float64_statistics_of_the_fp32_features(tmp_path, monkeypatch):
    from gcc_amd.metric import fid_eval as FE
    from gcc_amd.metric import get_real_stat as G
    root, weights = _root(tmp_path)
    out = tmp_path / 'made.npz'
    argv = ['--dataroot', str(root), '--output_path', str(out)]
    env = dict(os.environ, PYTHONPATH=ROOT, GCC_FID_INCEPTION=str(weights), GCC_FID_PRECISION='fp32')
    r = subprocess.run([sys.executable, '-m', 'gcc_amd.metric.get_real_stat'] + argv, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert '(native, fp32)' in r.stdout, r.stdout[-2000:]                  # the tool says which precision wrote the file
    # the fp32 engine's own features of the same images (it repeats itself bit for bit), numpy's float64 statistics of them
    monkeypatch.setenv(FE.ENV, str(weights))
    monkeypatch.setenv(FE.PRECISION_ENV, 'fp32')
    eng, why = FE.load_inception()
    assert why is None and eng.precision == 'fp32'
    keep = _Keep(eng)
    G.main(['--dataroot', str(root), '--output_path', str(tmp_path / 'again.npz')], inception=keep)
    act = torch.cat(keep.outputs).reshape(-1, 256).double().cpu().numpy()
    assert act.shape == (4, 256) and np.isfinite(act).all() and act.std(axis=0).max() > 0
    with np.load(str(out)) as z:
        assert sorted(z.files) == ['mu', 'sigma'] and z['mu'].dtype == z['sigma'].dtype == np.float64
        mu, sigma = z['mu'], z['sigma']
    mu_ref, sigma_ref = np.mean(act, axis=0), np.cov(act, rowvar=False)
    print('get_real_stat: max |mu err| %.3g, max |sigma err| %.3g' % (np.abs(mu - mu_ref).max(), np.abs(sigma - sigma_ref).max()))
    assert mu.shape == (256,) and sigma.shape == (256, 256)
    assert np.allclose(mu, mu_ref, rtol=1e-12, atol=1e-13) and np.allclose(sigma, sigma_ref, rtol=1e-11, atol=1e-13)
    # unset, the same calls give the bf16 engine (the tool's own run without the variable: tests/test_inception_fid_gpu.py)
    monkeypatch.delenv(FE.PRECISION_ENV)
    eng16, why = FE.load_inception()
    assert why is None and eng16.precision == 'bf16'


# ---- the product's width, once ------------------------------------------------------------------------------------------------------
def test_full_width_network_once_in_fp32():
    from gcc_amd import ops
    sd = E.seeded(1, 404)
    eng = _engine(sd, precision='fp32').to(DEV)
    del sd
    assert len(eng.convs) == 94 and eng.d == 2048 and eng.resize == 299 and eng.precision == 'fp32'
    x = E.seeded_input((2, 3, 256, 256), 405).to(DEV)
    L = ops.lib()
    predicted = eng.infer_launches(2, 256, 256)
    assert predicted == 109                                                # 1 resize, 94 convs, 13 pools, 1 mean
    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    f = eng(x)[0]
    torch.cuda.synchronize()
    n = L.gcc_launch_count(1)
    print('fp32 inception at 2 x 299 x 299: %d launches (predicted %d), %.2f GFLOP per image' % (n, predicted, eng.flops() / 1e9))
    assert n == predicted
    assert tuple(f.shape) == (2, 2048, 1, 1) and f.dtype == torch.float32 and torch.isfinite(f).all()
    assert float(f.min()) >= 0 and float(f.max()) > 0 and not torch.equal(f[0], f[1])         # means of ReLU outputs
    assert torch.equal(eng(x)[0], f)
