"""The SAGAN generator's fp32 inference route (SaganGeneratorEngine.infer(z, 'fp32'): 12 launches -- the coefficient group,
gcc_conv_eval_f32_z4, gcc_conv_eval_f32_unet, gcc_conv_eval_f32_act and gcc_attention_infer_f32) against the oracle's float64
restatement: the reference checkpoint, three seeded nets, tensor2im's bytes, u and v, launches and allocation, repeatability, a
weight change, isolation from the bf16 route and from training, and GCC_SAGAN_PRECISION from SAGANModel.infer_nhwc through the
FID scorer to `python -m gcc_amd.test`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._unet_f64 import tensor2im
from tests.test_sagan_infer_gpu import _eval_forward, _launches, _model, _sd, _step, _uv

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 8                      # the project's bar for its fp32 routes: 8 x the error of an fp32 evaluation of the same network


def _ops():
    from gcc_amd import ops
    return ops


def _oracle(sd, z, dtype):
    """the oracle's eval-mode image from the state_dict sd (copied: its power iteration moves u, v) with everything in dtype"""
    from oracle import gcc_oracle as O
    sd = {k: v.detach().to('cpu', dtype).clone() for k, v in sd.items() if v.is_floating_point()}
    with torch.no_grad():
        return O.sagan_generator_forward(sd, z.to(dtype), train=False)


def _fp32_view(model, z):
    ops = _ops()
    G, N = model.G, z.shape[0]
    x = ops.nchw_to_nhwc_f32(z.to(DEV, torch.float32).reshape(N, -1, 1, 1).contiguous(), G.infer_input(N, 'fp32'))
    out = G.infer(x, 'fp32')
    assert out.dtype is torch.float32 and tuple(out.shape) == (N, 3, 64, 64) and out.stride(1) == 1 and out.stride(3) >= 4
    return out


def _fp32(model, z, sd=None):
    """the fp32 route's image of z as NCHW fp32 on the host; sd: the state (u, v) to start from"""
    if sd is not None:
        model.netG.load_state_dict(sd)
    return _ops().nhwc_to_nchw_f32(_fp32_view(model, z), Cc=3).cpu()


def _bf16(model, z, sd=None):
    ops = _ops()
    if sd is not None:
        model.netG.load_state_dict(sd)
    G, N = model.G, z.shape[0]
    x = G.infer_input(N)
    ops.nchw_to_nhwc(z.to(DEV, torch.float32).reshape(N, -1, 1, 1).contiguous(), x)
    return ops.nhwc_to_nchw(G.infer(x), 3).cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _flip_share(image, f64):
    d = (tensor2im(image).int() - tensor2im(f64).int()).abs()
    return float((d != 0).double().mean()), int(d.max())


NETS = {'ngf64': (64, None), 'ngf64_pruned': (64, [200, 96, 40, 24]), 'ngf8': (8, None)}


def _seeded(ngf, cfg):
    model, opt = _model(ngf, cfg, seed=905, gammas=(0.5, -0.7))
    with torch.no_grad():
        model.netG.last[0].weight.mul_(2.0)
    model.refresh_weights()
    return model, opt


@functools.lru_cache(maxsize=None)
def _net(name):
    model, _ = _seeded(*NETS[name])
    sd0 = _sd(model.netG)
    z = torch.randn(2, 128, generator=torch.Generator().manual_seed(2))
    return model, sd0, z, _oracle(sd0, z, torch.float64)


# ---- 1. the reference checkpoint ----------------------------------------------------------------------------------------------
def test_reference_checkpoint_at_the_references_own_error(golden_dir):
    g = np.load(os.path.join(golden_dir, 'ref_checkpoint_sagan.npz'))
    model, _ = _model(seed=None, gammas=None)
    model.load_models(os.path.join(golden_dir, 'ref_checkpoint_sagan.pth'), load_discriminator=False)
    sd0 = _sd(model.netG)
    z, fake = torch.from_numpy(g['z']), torch.from_numpy(g['fake_img'])
    f64 = _oracle(sd0, z, torch.float64)
    ref = float((fake.double() - f64).abs().max())
    got = float((_fp32(model, z, sd0).double() - f64).abs().max())
    bf16 = float((_bf16(model, z, sd0).double() - f64).abs().max())
    print('reference checkpoint, max |. - f64|: reference fake_img %.3g, native fp32 %.3g, native bf16 %.3g' % (ref, got, bf16))
    assert 0 < ref <= 1e-6 and got <= BAR * ref


# ---- 2. three seeded nets -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(NETS))
def test_seeded_net_error_and_bytes(name):
    model, sd0, z, f64 = _net(name)
    # the condition, on the float64 image: it fills the range and does not sit in tanh's flat ends
    assert float(f64.std()) >= 0.2 and float((f64.abs() > 0.99).double().mean()) <= 0.01
    host = _oracle(sd0, z, torch.float32)
    err_host = float((host.double() - f64).abs().max())
    got = _fp32(model, z, sd0)
    err = float((got.double() - f64).abs().max())
    bf16 = _bf16(model, z, sd0)
    err16 = float((bf16.double() - f64).abs().max())
    share, worst = _flip_share(got, f64)
    share_host, _ = _flip_share(host, f64)
    share16, worst16 = _flip_share(bf16, f64)
    print('%s: std %.3f, max |. - f64|: host fp32 oracle %.3g, native fp32 %.3g, native bf16 %.3g; bytes that differ from float64\'s: '
          'host %.3g, native fp32 %.3g (largest step %d), native bf16 %.3g (largest step %d)'
          % (name, float(f64.std()), err_host, err, err16, share_host, share, worst, share16, worst16))
    assert err <= BAR * err_host
    assert worst <= 1 and share <= 1e-3
    # the bytes the device makes of the fp32 image (gcc_image_to_u8_f32) are tensor2im's
    model.netG.load_state_dict(sd0)
    assert torch.equal(_ops().image_to_u8(_fp32_view(model, z)).cpu(), tensor2im(got))


# ---- 3. u, v ------------------------------------------------------------------------------------------------------------------
def test_uv_move_the_same_bits_under_either_precision():
    model, sd0, z, _ = _net('ngf8')
    _bf16(model, z, sd0)
    uv16 = _uv(model)
    _fp32(model, z, sd0)
    uv32 = _uv(model)
    model.netG.load_state_dict(sd0)
    _eval_forward(model, z)
    for k, v in _uv(model).items():
        assert torch.equal(uv16[k], uv32[k]) and torch.equal(v, uv32[k]), k
        assert not torch.equal(v, sd0[k]), k


# ---- 4. launches and allocation -----------------------------------------------------------------------------------------------
def test_twelve_launches_at_every_batch_and_flat_memory():
    ops = _ops()
    lib = ops.lib()
    model, sd0, _, _ = _net('ngf64')
    G = model.G
    g = torch.Generator().manual_seed(4)
    zs = {N: torch.randn(N, 128, generator=g) for N in (1, 4, 50)}
    _fp32_view(model, zs[50])                                        # the slab has seen the largest batch; the packings are fresh
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    for N in (1, 4, 50):
        x = ops.nchw_to_nhwc_f32(zs[N].to(DEV).reshape(N, -1, 1, 1).contiguous(), G.infer_input(N, 'fp32'))
        torch.cuda.synchronize()
        lib.gcc_launch_count(1)
        assert G.infer_launches(N, 'fp32') == 12
        torch.cuda.synchronize()
        assert lib.gcc_launch_count(1) == 0                          # the route twin launches nothing
        assert _launches(lambda: G.infer(x, 'fp32')) == 12
    for N in (4, 1, 4, 1, 50):
        _fp32_view(model, zs[N])
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == m0, N
    model.netG.load_state_dict(sd0)


def test_engine_names_a_bad_precision():
    from gcc_amd._lib import GccError
    model, _, _, _ = _net('ngf8')
    G = model.G
    assert G.PRECISIONS == ('bf16', 'fp32')
    for call in (lambda: G.infer_input(1, 'fp16'), lambda: G.infer(None, 'fp16'), lambda: G.infer_launches(1, 'fp16')):
        with pytest.raises(GccError, match='fp16'):
            call()


# ---- 5. repeatability ---------------------------------------------------------------------------------------------------------
def test_repeated_runs_and_batches_give_identical_bits():
    model, sd0, z, _ = _net('ngf64_pruned')
    g = torch.Generator().manual_seed(77)
    z4 = torch.cat([z, torch.randn(2, 128, generator=g)])
    first = _fp32(model, z4, sd0)
    assert torch.equal(_bits(first), _bits(_fp32(model, z4, sd0)))
    assert torch.equal(_bits(_fp32(model, z4[:1], sd0)), _bits(first[:1]))
    model.netG.load_state_dict(sd0)


# ---- 6. a weight change -------------------------------------------------------------------------------------------------------
def test_a_training_step_reaches_the_fp32_route():
    model, _ = _seeded(8, None)                                      # a model of its own: the step moves its weights
    z = torch.randn(2, 128, generator=torch.Generator().manual_seed(2))
    before = _fp32(model, z)
    model.model_train()
    _step(model, 3)
    sd1 = _sd(model.netG)
    moved = _fp32(model, z)
    assert torch.isfinite(moved).all() and not torch.equal(moved, before)
    f64 = _oracle(sd1, z, torch.float64)
    err_host = float((_oracle(sd1, z, torch.float32).double() - f64).abs().max())
    err = float((moved.double() - f64).abs().max())
    print('after a training step: host fp32 oracle %.3g, native fp32 %.3g' % (err_host, err))
    assert err <= BAR * err_host


# ---- 7. isolation -------------------------------------------------------------------------------------------------------------
def test_bf16_route_and_training_are_untouched():
    model, _ = _seeded(8, None)
    fresh, _ = _seeded(8, None)                                      # a model that never runs fp32
    sd0 = _sd(model.netG)
    z = torch.randn(2, 128, generator=torch.Generator().manual_seed(2))
    before = _bf16(model, z, sd0)
    slab, packs, ctx, gbuf = model.G._ev_slab, model.G._ev_w, model.G.ctx, model.G.gbuf
    wt = [t.data_ptr() for t in packs.wt + packs.qkv_w]
    _fp32(model, z, sd0)
    _fp32(model, torch.cat([z, z, z]), sd0)
    assert model.G._ev_slab is slab and model.G._ev_w is packs and model.G.ctx is ctx and model.G.gbuf is gbuf
    assert wt == [t.data_ptr() for t in packs.wt + packs.qkv_w]
    assert model.G._ev32_slab is not slab and model.G._ev32_slab.dtype is torch.float32
    again = _bf16(model, z, sd0)
    assert torch.equal(_bits(before), _bits(again))
    assert torch.equal(_bits(_bf16(fresh, z)), _bits(again))
    model.model_train()
    _step(model, 5)
    losses = model.get_current_losses()
    assert losses and all(np.isfinite(v) for v in losses.values()), losses


# ---- 8. the variable, the scorer, the CLI -------------------------------------------------------------------------------------
def test_infer_nhwc_follows_the_variable(monkeypatch):
    from gcc_amd._lib import GccError
    ops = _ops()
    model, sd0, z, _ = _net('ngf8')
    for name in ('GCC_GEN_PRECISION', 'GCC_RESNET_PRECISION', 'GCC_SAGAN_PRECISION'):
        monkeypatch.delenv(name, raising=False)
    model.netG.load_state_dict(sd0)
    view = model.infer_nhwc(z)
    assert view.dtype is torch.bfloat16
    assert torch.equal(_bits(ops.nhwc_to_nchw(view, 3).cpu()), _bits(_bf16(model, z, sd0)))
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'fp32')                # not this generator's variable
    assert model.infer_nhwc(z).dtype is torch.bfloat16
    monkeypatch.setenv('GCC_SAGAN_PRECISION', 'fp32')
    want = _fp32(model, z, sd0)
    model.netG.load_state_dict(sd0)
    view = model.infer_nhwc({'z': z})
    assert view.dtype is torch.float32 and tuple(view.shape) == (2, 3, 64, 64) and view.stride(1) == 1 and view.stride(3) >= 4
    assert torch.equal(_bits(ops.nhwc_to_nchw_f32(view, Cc=3).cpu()), _bits(want))
    model.netG.load_state_dict(sd0)
    nchw = model.infer(z.reshape(2, 128, 1, 1))
    assert nchw.dtype is torch.float32 and nchw.is_contiguous() and torch.equal(_bits(nchw.cpu()), _bits(want))
    monkeypatch.setenv('GCC_SAGAN_PRECISION', 'fp64')
    with pytest.raises(GccError, match='GCC_SAGAN_PRECISION=fp64'):
        model.infer_nhwc(z)
    monkeypatch.setenv('GCC_SAGAN_PRECISION', 'fp32')
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')                   # refused for this model exactly as before
    with pytest.raises(GccError, match=r'GCC_GEN_PRECISION=fp32.*--model sagan'):
        model.infer_nhwc(z)
    model.netG.load_state_dict(sd0)


def test_fid_scorer_scores_the_bytes_of_the_fp32_image(tmp_path, monkeypatch):
    from gcc_amd.metric import fid_eval as FE
    from tests.test_fid_eval_gpu import _Keep, _argv, _inception, _model as _fid_model, _reference_fid, _sagan_root
    ops = _ops()
    root = _sagan_root(tmp_path)
    model, opt = _fid_model(_argv('sagan', root, tmp_path))
    keep = _Keep(torch.jit.load(str(_inception(tmp_path)), map_location=DEV))
    views = []
    real = model.infer_nhwc

    def infer_nhwc(*a, **k):
        view = real(*a, **k)
        views.append((view.dtype, ops.image_to_u8(view).cpu()))
        return view
    monkeypatch.setattr(model, 'infer_nhwc', infer_nhwc)
    monkeypatch.setenv('GCC_SAGAN_PRECISION', 'fp32')
    (value, _), = FE.fid_evaluator(keep, batch_size=2)(model, opt)
    assert len(views) == FE.sagan_count(25) and all(dt is torch.float32 for dt, _ in views)
    want = torch.cat([(u8.double() / 255).float().permute(0, 3, 1, 2) for _, u8 in views])
    got = torch.cat(keep.inputs).cpu()
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))       # the image_to_u8 branch: bytes / 255
    ref = _reference_fid(keep, root / 'real_stat.npz')
    print('stand-in Inception FID of the fp32 generator: %.6f (numpy float64 on the same activations %.6f)' % (value, ref))
    assert abs(value - ref) <= 1e-7 * ref


def test_cli_writes_the_bytes_of_the_fp32_image(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from gcc_amd import data as gdata
    from gcc_amd import test as gtest
    # in process: the PNGs of gcc_amd.test.run under the variable are the fp32 route's bytes, and not the bf16 route's
    model, opt = _seeded(8, None)
    opt.checkpoints_dir, opt.name = str(tmp_path / 'ck'), 'exp'
    model.save_models(3, str(tmp_path / 'save'))
    ckpt = str(tmp_path / 'save' / 'model_3.pth')
    g = torch.Generator().manual_seed(21)
    batches = [{'z': torch.randn(1, 128, generator=g), 'real_img': torch.rand(1, 3, 64, 64, generator=g) * 2 - 1,
                'img_path': ['/x/img%d.png' % i]} for i in range(3)]
    monkeypatch.setattr(gdata, 'create_dataset', lambda o, device=None: iter(batches))
    models = []
    for _ in range(4):
        m, _o = _model(8, seed=None, gammas=None)
        m.load_models(ckpt, load_discriminator=False)
        models.append(m)
    monkeypatch.delenv('GCC_SAGAN_PRECISION', raising=False)
    gtest.run(opt, models[3])
    assert 'generator precision' not in capsys.readouterr().out      # the default run's lines stay as they were
    monkeypatch.setenv('GCC_SAGAN_PRECISION', 'fp32')
    out = gtest.run(opt, models[0])
    assert 'generator precision: fp32' in capsys.readouterr().out.splitlines()
    differ = 0
    for data in batches:
        names = dict(gtest.result_names(['fake_img', 'real_img'], [data['img_path'], data['img_path']], opt.direction))
        png = np.asarray(Image.open(os.path.join(out, names['fake_img'])))
        assert np.array_equal(png, tensor2im(_fp32(models[1], data['z']))[0].numpy()), names['fake_img']
        differ += int((png != tensor2im(_bf16(models[2], data['z']))[0].numpy()).sum())
    assert differ > 0
    # the command line: it announces the precision and writes the images
    root = tmp_path / 'data'
    (root / 'train').mkdir(parents=True)
    rng = np.random.RandomState(0)
    for n in ('a1', 'a2'):
        Image.fromarray(rng.randint(0, 256, (170, 180, 3), dtype=np.uint8)).save(str(root / 'train' / (n + '.jpg')))
    argv = ['--dataroot', str(root), '--model', 'sagan', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--name', 'cli',
            '--checkpoints_dir', str(tmp_path / 'ck')]
    env = dict(os.environ, PYTHONPATH=ROOT, GCC_SAGAN_PRECISION='fp32')
    r = subprocess.run([sys.executable, '-m', 'gcc_amd.test'] + argv + ['--pretrain_path', ckpt], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'generator precision: fp32' in r.stdout.splitlines(), r.stdout[-2000:]
    files = sorted(str(p.relative_to(tmp_path / 'ck' / 'cli' / 'test_results')) for p in (tmp_path / 'ck' / 'cli' / 'test_results').rglob('*.png'))
    assert files == ['a1.png', 'a2.png', 'fake_img/a1_fake_img.png', 'fake_img/a2_fake_img.png'], files
