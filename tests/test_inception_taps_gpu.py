"""The reference's output blocks on the GPU (InceptionFidEngine(output_blocks=, pooled=), GCC_FID_DIMS, fid_score --dims,
get_real_stat --dims): thin seeded nets, every block's map against the restatements (tests/_inception_taps.py) with the bars of
tests/test_inception_fid_gpu.py (bf16) and tests/test_inception_fid_fp32_gpu.py (fp32) evaluated per tap, truncation bit for bit,
the pooled taps within gcc_map_mean's rounding bound of the engine's own maps, launch counts, and a full-width seeded weight file
tapped at block 0 (three convolutions) end to end through fid_score, get_real_stat and gcc_amd.test."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import metric_oracle as M
from tests import _inception_emul as E
from tests import _inception_taps as T

from . import _kid as K
from . import _prdc as P

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (22, 30)
RESIZE, SHAPE = 75, (3, 3, 40, 56)           # the tap maps are 17 x 17 x 8, 7 x 7 x 24, 3 x 3 x 96; the final map is 1 x 1
MAPS = ((8, 17, 17), (24, 7, 7), (96, 3, 3), (256, 1, 1))
MARGIN_BF16, MARGIN_FP32 = 2, 8              # the two existing files' bars


def _engine(sd, **kw):
    from gcc_amd.metric.inception_fid import InceptionFidEngine
    return InceptionFidEngine(sd, resize=RESIZE, **kw).to(DEV).eval()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def nets():
    """{(seed, precision): (state_dict, input, the restatements' four outputs {fp32, emul, f64}, the engine of all four blocks,
    its outputs)}, computed once and left unchanged"""
    out = {}
    for seed in SEEDS:
        sd = E.seeded(8, seed)
        x = E.seeded_input(SHAPE, seed + 100)
        ref = dict(fp32=T.forward_taps(sd, x, RESIZE), emul=T.forward_taps(sd, x, RESIZE, emulate=True),
                   f64=T.forward_taps64(sd, x, RESIZE))
        for precision in ('bf16', 'fp32'):
            eng = _engine(sd, precision=precision, output_blocks=(0, 1, 2, 3))
            out[seed, precision] = (sd, x, ref, eng, [t.cpu() for t in eng(x.to(DEV))])
    return out


@pytest.mark.parametrize('precision', ('bf16', 'fp32'))
@pytest.mark.parametrize('seed', SEEDS)
def test_all_four_blocks_and_each_truncated_engine_agree_bit_for_bit(nets, seed, precision):
    sd, x, ref, eng, got = nets[seed, precision]
    xd = x.to(DEV)
    assert len(got) == 4 and eng.d == 256 and eng.block_widths == {0: 8, 1: 24, 2: 96, 3: 256}
    for t, shape in zip(got, MAPS):
        assert t.dtype == torch.float32 and tuple(t.shape) == (SHAPE[0],) + shape and t.is_contiguous()
    default = _engine(sd, precision=precision)
    assert torch.equal(_bits(default(xd)[0].cpu()), _bits(got[3]))         # block 3 is today's engine, whatever else is tapped
    for block in (0, 1, 2):
        cut = _engine(sd, precision=precision, output_blocks=(block,))
        only = cut(xd)                                                      # the same batch: the bf16 route may split K by it
        assert len(only) == 1 and cut.d == MAPS[block][0]
        assert torch.equal(_bits(only[0].cpu()), _bits(got[block])), block
        assert cut._slab.numel() <= eng._slab.numel()
    assert torch.equal(_bits(eng(xd)[1].cpu()), _bits(got[1]))              # and the engine repeats itself


@pytest.mark.parametrize('seed', SEEDS)
def test_bf16_maps_within_twice_the_emulation_s_error_at_every_tap(nets, seed):
    """max |native - fp32| over a block's output against 2 x the bf16-emulating restatement's own error at that block
    (tests/test_inception_fid_gpu.py's bar, per tap).  The yardsticks on the host: seed 22 0.0318 / 0.0276 / 0.0196 / 0.0136, seed
    30 0.0175 / 0.0313 / 0.0213 / 0.0169 for blocks 0 .. 3.  Under the 1e-6 perturbation of the restatement's conv results that
    file describes (five draws per seed) the yardsticks of blocks 0 and 1 do not move at all, block 2's moves by a factor of 1.1
    (seed 22) and 1.3 (seed 30): maxima over thousands of elements, steadier than the 1 x 1 final map the seeds were chosen for.
    Both seeds stay."""
    sd, x, ref, eng, got = nets[seed, 'bf16']
    for block in range(4):
        emul = float((ref['emul'][block] - ref['fp32'][block]).abs().max())
        err = float((got[block] - ref['fp32'][block]).abs().max())
        print('seed %d block %d: max |native - fp32| %.5f, emul_err %.5f, ratio %.2f, max |value| %.3f'
              % (seed, block, err, emul, err / emul, float(ref['fp32'][block].abs().max())))
        assert emul > 0 and err <= MARGIN_BF16 * emul, block


@pytest.mark.parametrize('seed', SEEDS)
def test_fp32_maps_within_eight_times_the_fp32_restatement_s_error_at_every_tap(nets, seed):
    """max |native fp32 - float64| over a block's output against 8 x max |fp32 restatement - float64| at that block
    (tests/test_inception_fid_fp32_gpu.py's bar, per tap); the yardsticks on the host: 9.3e-6 / 7.1e-6 / 1.9e-6 / 1.2e-6 at seed
    22, 4.6e-6 / 5.7e-6 / 1.6e-6 / 7.1e-7 at seed 30."""
    sd, x, ref, eng, got = nets[seed, 'fp32']
    for block in range(4):
        want = ref['f64'][block]
        err = float((got[block].double() - want).abs().max())
        yard = float((ref['fp32'][block].double() - want).abs().max())
        print('seed %d block %d: max |native fp32 - f64| %.3g, max |fp32 restatement - f64| %.3g, ratio %.2f'
              % (seed, block, err, yard, err / yard))
        assert yard > 0 and err <= MARGIN_FP32 * yard, block


@pytest.mark.parametrize('precision', ('bf16', 'fp32'))
def test_pooled_taps_are_the_f64_means_of_the_engine_s_own_maps(nets, precision):
    """pooled=True: [N, C, 1, 1] within 2^-24 |m| + P 2^-52 mean|x| of the fsum mean m of the map the unpooled engine returns
    (tests/test_map_mean_kernels_gpu.py's bound); the launches are the prefix's, the resize and gcc_map_mean's one or two -- no
    NCHW copy; on the fp32 route an image alone gives the bits it had in the batch; the slab is reused across batch sizes."""
    from gcc_amd import ops
    L = ops.lib()
    sd, x, ref, eng, got = nets[SEEDS[0], precision]
    xd = x.to(DEV)
    for block in (0, 1, 2):
        Cc, h, w = MAPS[block]
        pooled = _engine(sd, precision=precision, output_blocks=(block,), pooled=True)
        unpooled = _engine(sd, precision=precision, output_blocks=(block,))
        predicted = pooled.infer_launches(SHAPE[0], SHAPE[2], SHAPE[3])
        torch.cuda.synchronize()
        L.gcc_launch_count(1)
        out = pooled(xd)
        torch.cuda.synchronize()
        n = L.gcc_launch_count(1)
        mean_launches = ops.map_mean_launches(h, w, Cc)
        assert n == predicted and 1 <= mean_launches <= 2
        assert predicted == unpooled.infer_launches(SHAPE[0]) - 1 + mean_launches      # the copy's launch is not made
        steps = pooled._program(SHAPE[0]).steps
        if precision == 'fp32':                                            # one launch per step: prefix + resize + the mean
            assert predicted == (len(steps) - 1) + 1 + mean_launches
        assert len(out) == 1 and tuple(out[0].shape) == (SHAPE[0], Cc, 1, 1) and out[0].dtype == torch.float32
        m, bound = T.mean_bound(got[block])                                 # the same batch: the same map, bit for bit
        err = np.abs(out[0].double().cpu().numpy().reshape(SHAPE[0], Cc) - m)
        live = bound > 0                                                    # a channel the ReLU left at zero: mean 0, bound 0
        print('%s block %d: pooled against the fsum means of the engine\'s map, max err / bound %.3f, %d dead channels'
              % (precision, block, float((err[live] / bound[live]).max()), int((~live).sum())))
        assert bool((bound < 1e-6 * np.maximum(np.abs(m), 1e-3)).all()) and bool((err <= bound).all())
        slab = pooled._slab.data_ptr()
        for i in range(SHAPE[0]):
            one = pooled(xd[i:i + 1].contiguous())[0]
            if precision == 'fp32':
                assert torch.equal(_bits(one), _bits(out[0][i:i + 1])), (block, i)
            else:
                assert torch.isfinite(one).all()
        assert pooled._slab.data_ptr() == slab                              # a smaller batch lives in the same slab
        assert torch.equal(_bits(pooled(xd)[0]), _bits(out[0]))
        small = pooled._slab.numel()
        twice = pooled(torch.cat([xd, xd]))[0]                              # a larger one makes it grow; the bits stay (fp32)
        assert pooled._slab.numel() > small
        if precision == 'fp32':
            assert torch.equal(_bits(twice[:SHAPE[0]]), _bits(out[0])) and torch.equal(_bits(twice[SHAPE[0]:]), _bits(out[0]))
        assert torch.equal(_bits(pooled(xd)[0]), _bits(out[0]))


# ---- end to end: a full-width seeded weight file tapped at block 0, --dims 64 ------------------------------------------------------
FAKE, REAL, BATCH = 75, 80, 5                # more images than the 64 features on both sides


def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(str(path))


@pytest.fixture(scope='module')
def weights(tmp_path_factory):
    """the reference's kind of weight file at the real widths: a plain state_dict"""
    path = tmp_path_factory.mktemp('inception') / 'pt_inception_seeded.pth'
    torch.save(E.seeded(1, 31), str(path))
    return path


def _image(rng, top, size=96):
    """gratings of random frequency (up to the pixel grid's limit), direction and colour over noise of random strength: the texture
    survives the resize to 299, so the 64 features of the stem spread in many directions and the covariances are well conditioned
    (condition numbers 1.5e7 and 2.7e7 on the host's restatement; the oracle agrees with the symmetric eigenvalue problem to 2e-12)"""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    img = np.zeros((size, size, 3))
    for _ in range(4):
        f, th, ph = rng.uniform(0.02, 0.5), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        img += np.sin(2 * np.pi * f * (xx * np.cos(th) + yy * np.sin(th)) + ph)[..., None] * rng.uniform(-1, 1, 3) * 0.35
    img += rng.uniform(0, 0.4) * rng.standard_normal((size, size, 3)) + rng.uniform(0.2, 0.8, 3)
    return (np.clip(img, 0, 1) * (top - 1)).astype(np.uint8)


def _folders(tmp_path):
    rng = np.random.RandomState(12)
    a, b = tmp_path / 'real', tmp_path / 'fake'
    a.mkdir(), b.mkdir()
    for folder, n, top in ((a, REAL, 256), (b, FAKE, 200)):              # the second set darker: the distance is O(1)
        for i in range(n):
            _png(folder / ('img%03d.png' % i), _image(rng, top))
    return a, b


class _Keep:
    def __init__(self, net):
        self.net, self.outputs = net, []
        self.precision, self.output_blocks, self.d = net.precision, net.output_blocks, net.d

    def to(self, device):
        self.net = self.net.to(device)
        return self

    def __call__(self, x):
        y = self.net(x)
        self.outputs.append(y[0].clone())
        return y

    def activations(self, lo=0, hi=None):
        return torch.cat(self.outputs[lo:hi]).reshape(-1, self.d).double().cpu().numpy()


def _fid_ref(a, b):
    """tests/test_kid_score_gpu.py's reference: numpy float64 statistics + the oracle's distance, itself checked against the
    symmetric eigenvalue problem"""
    (m1, s1), (m2, s2) = ((np.mean(x, axis=0), np.cov(x, rowvar=False)) for x in (a, b))
    ref = float(M.calculate_frechet_distance(m1, s1, m2, s2))
    w, V = np.linalg.eigh(s1)
    root = (V * np.sqrt(np.clip(w, 0, None))) @ V.T
    tr = np.sqrt(np.clip(np.linalg.eigvalsh(root @ s2 @ root), 0, None)).sum()
    sym = float(((m1 - m2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * tr)
    print('the oracle\'s distance %.12g, by the symmetric eigenvalue problem %.12g (rel %.2e)' % (ref, sym, abs(ref - sym) / sym))
    assert abs(ref - sym) <= 1e-8 * sym
    return ref


def _run(module, argv, env):
    r = subprocess.run([sys.executable, '-m', module] + [str(a) for a in argv], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, **env),
                       capture_output=True, text=True, timeout=600)
    return r


def test_fid_score_dims_64_prints_fid_kid_and_prdc_of_the_native_block(tmp_path, weights, monkeypatch, capsys):
    from gcc_amd.metric import fid_eval as FE
    from gcc_amd.metric import fid_score as F
    from gcc_amd.metric.prdc_score import prdc_text
    a, b = _folders(tmp_path)
    monkeypatch.setenv(FE.ENV, str(weights))
    monkeypatch.delenv(FE.DIMS_ENV, raising=False)
    monkeypatch.delenv(FE.PRECISION_ENV, raising=False)
    eng, why = FE.load_inception(64)
    assert why is None and eng.output_blocks == (0,) and eng.pooled and eng.d == 64 and eng.resize == 299
    assert FE.network_label(eng) == ' (native, bf16, dims 64)'
    assert len(eng._program(BATCH).steps) == 3 + 1 + 1                      # three convolutions, the pool, the tap
    keep = _Keep(eng)
    argv = [str(a), str(b), '--dims', '64', '--batch-size', str(BATCH)]
    fid, kid, prdc = F.main(argv + ['--prdc'], model=keep)
    capsys.readouterr()
    act_r, act_f = keep.activations(0, REAL // BATCH), keep.activations(REAL // BATCH)
    assert act_r.shape == (REAL, 64) and act_f.shape == (FAKE, 64) and np.isfinite(act_r).all() and act_r.std(axis=0).min() > 0
    ref = _fid_ref(act_r, act_f)
    # measured on an MI355X (profiles/r20_inception_taps.txt's run): FID 3.633614862 against 3.633614525, rel 9.3e-8 -- inside
    # the bar by little: the covariances' condition numbers are 1.5e7 and 2.7e7, where tests/test_kid_score_gpu.py's stand-in is milder
    print('--dims 64: FID %.10g, numpy float64 statistics + the oracle\'s distance %.10g (rel %.2e)' % (fid, ref, abs(fid - ref) / ref))
    assert ref > 0 and abs(fid - ref) <= 1e-7 * ref
    kref, kbound = K.kid_ref(act_r, act_f)
    print('--dims 64: KID %.12g, float64 restatement %.12g, err / bound %.3g' % (kid, kref, abs(kid - kref) / kbound))
    assert abs(kid - kref) <= kbound and kbound < 1e-6 * max(abs(kref), 1e-3)
    margin = P.margin(act_r, act_f, 5)
    want, counts = P.prdc_ref(act_r, act_f, 5)
    print('--dims 64 --prdc: %s, counts %s, margin %.3g' % (want, counts, margin))
    assert margin > 0 and prdc == want
    # the module's own command line: the engine repeats itself bit for bit, so the same lines
    r = _run('gcc_amd.metric.fid_score', argv, {})
    assert r.returncode == 0, r.stderr[-3000:]
    assert [s for s in r.stdout.splitlines() if 'FID' in s or 'KID' in s] == ['FID: %.2f' % fid, 'KID: %.6f' % kid]
    r = _run('gcc_amd.metric.fid_score', argv + ['--prdc'], {})
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.splitlines()[-3:] == ['FID: %.2f' % fid, 'KID: %.6f' % kid, prdc_text(want)]
    # the variable stands in for the flag, the flag wins over the variable
    monkeypatch.setenv(FE.DIMS_ENV, '64')
    assert F.main([str(a), str(b), '--batch-size', str(BATCH)], model=None)[:2] == (fid, kid)
    monkeypatch.setenv(FE.DIMS_ENV, '192')
    assert F.main(argv, model=None)[:2] == (fid, kid)


def _root(tmp_path):
    root = tmp_path / 'shoes'
    rng = np.random.RandomState(4)
    (root / 'val').mkdir(parents=True)
    for i in range(4):
        _png(root / 'val' / ('pair%d.png' % i), rng.randint(0, 256, (256, 512, 3), dtype=np.uint8))
    return root


def test_get_real_stat_dims_64_then_gcc_amd_test_under_the_variable(tmp_path, weights, monkeypatch):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import fid_eval as FE
    from gcc_amd.metric import kid_score as S
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    root = _root(tmp_path)
    stat, feat = root / 'real_stat_B.npz', root / 'real_act_B.npz'
    r = _run('gcc_amd.metric.get_real_stat', ['--dataroot', root, '--output_path', stat, '--features_path', feat, '--dims', '64'],
             {FE.ENV: str(weights)})
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'with the Inception network (native, bf16, dims 64)' in r.stdout, r.stdout[-2000:]
    with np.load(str(stat)) as z:
        assert z['mu'].shape == (64,) and z['sigma'].shape == (64, 64) and z['mu'].dtype == np.float64
        mu, sigma = z['mu'], z['sigma']
    act, label = S.load_features(str(feat), 64, DEV)
    assert tuple(act.shape) == (4, 64) and label == ' (native, bf16, dims 64)'
    a64 = act.double().cpu().numpy()
    assert np.allclose(mu, a64.mean(0), rtol=1e-12, atol=1e-13) and np.allclose(sigma, np.cov(a64, rowvar=False), rtol=1e-11, atol=1e-13)
    # GCC_FID_DIMS reaches gcc_amd.test through builtin_inception: the FID against that file, the same value in process
    argv = ['--dataroot', str(root), '--model', 'pix2pix', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--name', 'exp',
            '--checkpoints_dir', str(tmp_path / 'ck'), '--print_freq', '1000']
    opt = options.parse(argv)
    opt.isTrain = True
    torch.manual_seed(31)
    model = get_model_class(opt)(opt)
    model.model_eval()
    model.save_models(1, str(tmp_path / 'save'))
    monkeypatch.setenv(FE.ENV, str(weights))
    monkeypatch.setenv(FE.DIMS_ENV, '64')
    net, why = FE.builtin_inception(opt)
    assert why is None and net.output_blocks == (0,) and net.pooled and net.d == 64
    value = FE.fid_evaluator(net)(model, opt)[0][0]
    assert np.isfinite(value) and value > 0
    r = _run('gcc_amd.test', argv + ['--pretrain_path', str(tmp_path / 'save' / 'model_1.pth')], {})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert ('FID: %.2f' % value) in lines and any(s.startswith('KID: ') for s in lines), r.stdout[-2000:]
    # statistics of another width: the refusal names both widths and the command that writes matching ones
    np.savez(str(stat), mu=np.zeros(2048), sigma=np.eye(2048))
    with pytest.raises(GccError, match=r'mu \(2048,\) and sigma \(2048, 2048\).*d = 64 .*get_real_stat --dims 64'):
        FE.fid_evaluator(net)(model, opt)


class _StandIn(torch.nn.Module):
    """tests/test_kid_score_gpu.py's stand-in at 64 features: a fixed-seed 1 x 1 projection, ReLU, average pool"""

    def __init__(self):
        super().__init__()
        self.proj = torch.nn.Conv2d(3, 64, 1)
        g = torch.Generator().manual_seed(29)
        with torch.no_grad():
            self.proj.weight.copy_(torch.randn(self.proj.weight.shape, generator=g))
            self.proj.bias.copy_(torch.randn(64, generator=g) * 0.5 - 0.5)

    def forward(self, x):
        return [torch.nn.functional.adaptive_avg_pool2d(torch.relu(self.proj(x)), 1)]


def test_a_torchscript_archive_runs_as_exported_whatever_the_variable_says(tmp_path, monkeypatch, capsys):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import fid_eval as FE
    from gcc_amd.metric import fid_score as F
    a, b = _folders(tmp_path)
    archive = tmp_path / 'standin64.pt'
    torch.jit.script(_StandIn()).save(str(archive))
    monkeypatch.setenv(FE.ENV, str(archive))
    monkeypatch.delenv(FE.DIMS_ENV, raising=False)
    argv = [str(a), str(b), '--batch-size', str(BATCH)]
    want = F.main(argv + ['--dims', '64'])
    monkeypatch.setenv(FE.DIMS_ENV, '64')
    net, why = FE.load_inception()
    assert why is None and isinstance(net, torch.jit.ScriptModule) and FE.network_label(net) == ''
    assert F.main(argv) == want                                             # the width asked for is its own 64: it scores
    monkeypatch.setenv(FE.DIMS_ENV, '192')                                  # its width is still checked where it is checked today
    with pytest.raises(GccError, match='d = 64, dims = 192 was asked for'):
        F.main(argv)
    assert F.main(argv + ['--dims', '64']) == want
