"""The MobileResnet generator's fp32 inference route (MobileResnetEngine.infer(x, 'fp32')) against the float64 restatement of
tests/_mobile_resnet_f64.py: the reference-written images (CycleGAN's two generators, Pix2Pix --backbone resnet, two pruned
students), seeded nets whose images fill [-1, 1], bytes of tensor2im, launches and allocation, isolation from the bf16 route and
from training, and GCC_RESNET_PRECISION from the models' infer_nhwc to `python -m gcc_amd.test --model cyclegan`."""
import functools
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import _mobile_resnet_f64 as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 8                      # the project's bar for its fp32 routes: 8 x the error of an fp32 evaluation of the same network


def _host_sd(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def _fp32(G, A):
    """the fp32 route's image of the host batch A as NCHW fp32 on the host, through the engine G"""
    from gcc_amd import ops
    N, _, H, W = A.shape
    G.eval_coeffs('fp32')
    out = G.infer(ops.nchw_to_nhwc_f32(A.to(DEV).contiguous(), G.infer_input(N, H, W, 'fp32')), 'fp32')
    assert out.dtype is torch.float32 and tuple(out.shape) == (N, 3, H, W) and out.stride(1) == 1
    return ops.nhwc_to_nchw_f32(out).cpu()


def _bf16(G, A):
    from gcc_amd import ops
    N, _, H, W = A.shape
    G.eval_coeffs()
    x = G.infer_input(N, H, W)
    ops.nchw_to_nhwc(A.to(DEV).contiguous(), x, cfill=8)
    return ops.nhwc_to_nchw(G.infer(x), 3).cpu()


def _flip_share(image, f64):
    """(share of tensor2im bytes that differ from the float64 image's, the largest byte difference)"""
    d = (R.tensor2im(image).int() - R.tensor2im(f64).int()).abs()
    return float((d != 0).double().mean()), int(d.max())


def _against_reference(tag, G, net, A, fake):
    """the fp32 route at <= BAR x the reference-written image's own distance from float64"""
    f64 = R.resnet_eval(_host_sd(net), A)
    ref = float((fake.double() - f64).abs().max())
    got = float((_fp32(G, A).double() - f64).abs().max())
    bf16 = float((_bf16(G, A).double() - f64).abs().max())
    print('%s, max |. - f64|: reference image %.3g, native fp32 %.3g (%.2f x), native bf16 %.3g' % (tag, ref, got, got / ref, bf16))
    # the reference's own distance is its fp32 rounding (1e-6 on these nets); anything larger means image and input do not belong together
    assert 0 < ref <= 5e-6 and got <= BAR * ref, (tag, got, ref)


def _generator_input(z):
    """the batch the fixture's generator saw: A or B by the fixture's --direction"""
    return torch.from_numpy(z['A' if str(z['direction']) == 'AtoB' else 'B'])


# ---- 1. reference-written images -----------------------------------------------------------------------------------------------
def _cycle_model(extra=(), **kw):
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    opt = options.parse(['--dataroot', './database/horse2zebra/', '--model', 'cyclegan', '--gpu_ids', '0', '--ngf', '8',
                         '--ndf', '8'] + list(extra))
    opt.isTrain = True
    return get_model_class(opt)(opt, **kw), opt


def test_cyclegan_reference_checkpoint_at_the_references_own_error(golden_dir):
    z = np.load(os.path.join(golden_dir, 'ref_checkpoint_cyclegan.npz'))
    model, _ = _cycle_model(['--darts_discriminator'])
    model.load_models(os.path.join(golden_dir, 'ref_checkpoint_cyclegan.pth'), load_discriminator=False)
    for gen, net, src, key in (('A', model.netG_A, 'A', 'fake_B'), ('B', model.netG_B, 'B', 'fake_A')):
        _against_reference('cyclegan ' + key, model.G[gen], net, torch.from_numpy(z[src]), torch.from_numpy(z[key]))


def test_pix2pix_resnet_reference_image_at_the_references_own_error(golden_dir):
    from tests.test_pix2pix_gpu import _build_resnet_gcc, load
    z = load(golden_dir, 'pix2pix_resnet_gcc.npz')
    model, _, _ = _build_resnet_gcc(z)
    _against_reference('pix2pix resnet eval.fake_B', model.G, model.netG, _generator_input(z), torch.from_numpy(z['eval.fake_B']))


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_pruned_resnet_reference_image_at_the_references_own_error(golden_dir, tag):
    """a: widths 17, 15, 18, ... (none a multiple of 8); b: a removed block"""
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    from tests.test_pix2pix_gpu import load, load_recipe
    z = load(golden_dir, 'prune_resnet.npz')
    cfg = [int(v) for v in z['pruned_%s.cfg' % tag]]
    opt = options.parse(['--dataroot', './database/cityscapes/', '--model', 'pix2pix', '--gpu_ids', '0', '--backbone', 'resnet',
                         '--ngf', '8', '--ndf', '8'])
    opt.isTrain = True
    model = get_model_class(opt)(opt, filter_cfgs=cfg)
    load_recipe(model.netG, 711)
    load_recipe(model.netD, 712)
    model.refresh_weights()
    B = len(model.G.blocks)
    assert (B < 9) == (tag == 'b')
    _against_reference('pruned ' + tag, model.G, model.netG, _generator_input(z), torch.from_numpy(z['pruned_%s.eval.fake_B' % tag]))
    assert model.G.infer_launches(2, 64, 64, 'fp32') == 10 * B + 16


# ---- 2. seeded nets whose images fill the range ------------------------------------------------------------------------------
def _engine(ngf, n_blocks):
    from gcc_amd import engine
    from gcc_amd.models.Pix2Pix import MobileResnetGenerator
    net = MobileResnetGenerator(ngf=ngf, n_blocks=n_blocks).to(DEV)
    engine.FlatParams(list(net.parameters()), DEV)
    return net, engine.MobileResnetEngine(net, DEV)


def _range_filling(net, eng, seed, N, size):
    """He-normal weights (std = sqrt(2 / fan_in); fan_in = Ci k^2, 9 for a depthwise conv, 9 Ci / 4 for a transposed one, which
    sums a quarter of its taps per output pixel), biases N(0, 0.1^2), a zero bias on the last conv and its weight scaled so that
    the float64 pre-tanh standard deviation is 0.5: the image fills [-1, 1] without saturating.  Returns (input, float64 image)."""
    g = torch.Generator().manual_seed(seed)
    convs = [m for m in net.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
    with torch.no_grad():
        for m in convs:
            if isinstance(m, torch.nn.ConvTranspose2d):
                fan_in = 9 * m.weight.shape[0] / 4
            else:
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]     # depthwise: [C, 1, 3, 3] -> 9
            m.weight.copy_((torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5).to(DEV))
            m.bias.copy_((torch.randn(m.bias.shape, generator=g) * 0.1).to(DEV))
        last = convs[-1]
        assert tuple(last.weight.shape[2:]) == (7, 7) and last.weight.shape[0] == 3
        last.bias.zero_()
        A = torch.rand(N, 3, size, size, generator=g) * 2 - 1
        pre = R.resnet_eval(_host_sd(net), A, pre_tanh=True)
        last.weight.mul_(0.5 / float(pre.std()))
    eng.repack()
    return A, R.resnet_eval(_host_sd(net), A)


NETS = {'ngf8_b9_64': (8, 9, 64, 1), 'ngf16_b9_128': (16, 9, 128, 2), 'ngf8_b3_96': (8, 3, 96, 1)}


@functools.lru_cache(maxsize=None)
def _net(name):
    ngf, blocks, size, N = NETS[name]
    net, eng = _engine(ngf, blocks)
    A, f64 = _range_filling(net, eng, 100 + ngf + blocks, N, size)
    return net, eng, A, f64


@pytest.mark.parametrize('name', list(NETS))
def test_range_filling_net_error_and_bytes(name):
    net, G, A, f64 = _net(name)
    # the condition, on the float64 image: it fills the range and does not sit in tanh's flat ends
    assert float((f64.abs() > 0.99).double().mean()) <= 0.01 and float(f64.std()) >= 0.2
    host = R.resnet_eval(_host_sd(net), A, torch.float32)
    err_host = float((host.double() - f64).abs().max())
    got = _fp32(G, A)
    err = float((got.double() - f64).abs().max())
    bf16 = _bf16(G, A)
    err16 = float((bf16.double() - f64).abs().max())
    share, worst = _flip_share(got, f64)
    share_host, _ = _flip_share(host, f64)
    share16, worst16 = _flip_share(bf16, f64)
    print('%s: std %.3f, max |. - f64|: fp32 torch restatement %.3g, native fp32 %.3g (%.2f x), native bf16 %.3g; bytes that differ '
          'from float64\'s: restatement %.3g, native fp32 %.3g (largest step %d), native bf16 %.3g (largest step %d)'
          % (name, float(f64.std()), err_host, err, err / err_host, err16, share_host, share, worst, share16, worst16))
    assert err <= BAR * err_host
    assert worst <= 1 and share <= 1e-3
    # the bytes the device makes of the fp32 image (gcc_image_to_u8_f32) are tensor2im's
    from gcc_amd import ops
    N, _, H, W = A.shape
    view = G.infer(ops.nchw_to_nhwc_f32(A.to(DEV).contiguous(), G.infer_input(N, H, W, 'fp32')), 'fp32')
    assert torch.equal(ops.image_to_u8(view).cpu(), R.tensor2im(got))


def test_repeated_runs_and_batches_give_identical_bits():
    net, G, A, _ = _net('ngf8_b3_96')
    g = torch.Generator().manual_seed(77)
    B = torch.cat([A, torch.rand(2, 3, 96, 96, generator=g) * 2 - 1])
    first = _fp32(G, B)
    assert torch.equal(first.view(torch.int32), _fp32(G, B).view(torch.int32))
    for n in range(3):
        assert torch.equal(_fp32(G, B[n:n + 1]).view(torch.int32), first[n:n + 1].contiguous().view(torch.int32)), n


# ---- 3. launches and allocation -----------------------------------------------------------------------------------------------
def test_launches_and_no_allocation():
    from gcc_amd import ops
    L = ops.lib()
    net, G, _, _ = _net('ngf8_b9_64')
    B = len(G.blocks)
    G.eval_coeffs('fp32')
    G.infer(G.infer_input(3, 128, 128, 'fp32'), 'fp32')          # the largest geometry first
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    G.eval_coeffs('fp32')                                         # refreshed into the buffers of the first call
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0
    for N, H, W in ((1, 64, 64), (3, 128, 128), (2, 64, 128)):
        x = G.infer_input(N, H, W, 'fp32')
        L.gcc_launch_count(1)
        want = G.infer_launches(N, H, W, 'fp32')
        assert L.gcc_launch_count(1) == 0                         # the route twins launch nothing
        assert want <= 10 * B + 16
        G.infer(x, 'fp32')
        torch.cuda.synchronize()
        assert L.gcc_launch_count(1) == want
    for N, H, W in ((1, 128, 64), (2, 64, 64), (1, 8, 8), (3, 128, 128), (1, 32, 48)):     # nothing larger than the slab has seen
        G.infer(G.infer_input(N, H, W, 'fp32'), 'fp32')
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0
    print('fp32 route: %d launches for %d blocks' % (want, B))


def test_engine_names_a_bad_precision_and_a_missing_refresh():
    from gcc_amd._lib import GccError
    net, G = _engine(8, 2)
    G.repack()
    assert G.PRECISIONS == ('bf16', 'fp32')
    for call in (lambda: G.eval_coeffs('fp16'), lambda: G.infer_input(1, 32, 32, 'fp16'), lambda: G.infer(None, 'fp16'),
                 lambda: G.infer_launches(1, 32, 32, 'fp16')):
        with pytest.raises(GccError, match='fp16'):
            call()
    with pytest.raises(GccError, match=r"eval_coeffs\('fp32'\) first"):
        G.infer(G.infer_input(1, 32, 32, 'fp32'), 'fp32')
    G.eval_coeffs('fp32')
    with pytest.raises(GccError, match='multiples of 4'):
        G.infer(G.infer_input(1, 30, 32, 'fp32'), 'fp32')
    assert G.infer_launches(1, 32, 32, 'fp32') == 36


# ---- 4. isolation ------------------------------------------------------------------------------------------------------------
def test_bf16_route_is_untouched():
    net, G = _engine(8, 3)
    A, _ = _range_filling(net, G, 21, 2, 64)
    before = _bf16(G, A)
    slab = G._ev_slab
    assert G.ctx == {} and G.gbuf == {}
    _fp32(G, A)
    _fp32(G, torch.cat([A, A, A]))
    assert G._ev_slab is slab and G.ctx == {} and G.gbuf == {}
    assert torch.equal(before.view(torch.int32), _bf16(G, A).view(torch.int32))


def test_fp32_inference_between_cyclegan_steps_changes_nothing(monkeypatch):
    """fp32 inference of both generators between two training iterations: losses and weights bit-identical"""
    import random
    from tests.golden.recipe import recipe_state_dict

    def run(with_infer):
        torch.manual_seed(0)
        random.seed(0)
        model, _ = _cycle_model(['--crop_size', '64', '--load_size', '64'])
        for i, net in enumerate((model.netG_A, model.netG_B, model.netD_A, model.netD_B)):
            shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
            net.load_state_dict({k: v.to(DEV) for k, v in recipe_state_dict(shapes, 900 + i).items()})
        model.refresh_weights()
        model.model_train()
        g = torch.Generator().manual_seed(3)
        data = [{'A': torch.rand(1, 3, 64, 64, generator=g) * 2 - 1, 'B': torch.rand(1, 3, 64, 64, generator=g) * 2 - 1,
                 'A_paths': ['a'], 'B_paths': ['b']} for _ in range(2)]
        losses = []
        model.set_input(data[0])
        model.optimize_parameters()
        losses.append(model.get_current_losses())
        if with_infer:
            a, b = model.infer(data[1]['A'].to(DEV), 'A'), model.infer(data[1]['B'].to(DEV), 'B')
            assert a.dtype is torch.float32 and torch.isfinite(a).all() and torch.isfinite(b).all()
            # and it is the image of the weights the step left behind
            f64 = R.resnet_eval(_host_sd(model.netG_A), data[1]['A'])
            host = float((R.resnet_eval(_host_sd(model.netG_A), data[1]['A'], torch.float32).double() - f64).abs().max())
            assert float((a.cpu().double() - f64).abs().max()) <= BAR * host
        model.set_input(data[1])
        model.optimize_parameters()
        losses.append(model.get_current_losses())
        w = [p.detach().clone() for n in (model.netG_A, model.netG_B) for p in n.parameters()]
        return losses, w
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'fp32')
    l0, w0 = run(False)
    l1, w1 = run(True)
    assert l0 == l1
    assert all(torch.equal(a, b) for a, b in zip(w0, w1))


# ---- 5. the variable, the models, the CLI ------------------------------------------------------------------------------------
def _last_conv(net):
    return [m for m in net.modules() if isinstance(m, torch.nn.Conv2d)][-1]


def test_cyclegan_infer_follows_the_variable(monkeypatch):
    from gcc_amd import ops
    from gcc_amd._lib import GccError
    model, _ = _cycle_model()
    model.model_eval()
    g = torch.Generator().manual_seed(4)
    A, B = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1, torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    monkeypatch.delenv('GCC_RESNET_PRECISION', raising=False)
    monkeypatch.delenv('GCC_GEN_PRECISION', raising=False)
    assert model.infer_nhwc(A).dtype is torch.bfloat16
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'fp32')
    for gen, net, src in (('A', model.netG_A, A), ('B', model.netG_B, B)):
        view = model.infer_nhwc(src, gen)
        assert view.dtype is torch.float32 and tuple(view.shape) == tuple(src.shape)
        want = _fp32(model.G[gen], src)
        data = {'A': A, 'B': B, 'A_paths': ['a'], 'B_paths': ['b']}
        assert torch.equal(ops.nhwc_to_nchw_f32(model.infer_nhwc(data, gen)).cpu().view(torch.int32), want.view(torch.int32))
        nchw = model.infer(src, gen)
        assert nchw.dtype is torch.float32 and nchw.is_contiguous() and torch.equal(nchw.cpu().view(torch.int32), want.view(torch.int32))
    # the refresh is keyed to the generation: new weights reach the route after refresh_weights
    want = model.infer(A, 'A').cpu()
    with torch.no_grad():
        _last_conv(model.netG_A).weight.mul_(0.5)
    assert torch.equal(model.infer(A, 'A').cpu(), want)                # not before
    model.refresh_weights()
    half = model.infer(A, 'A').cpu()
    assert not torch.equal(half, want)
    f64 = R.resnet_eval(_host_sd(model.netG_A), A)
    host = float((R.resnet_eval(_host_sd(model.netG_A), A, torch.float32).double() - f64).abs().max())
    assert float((half.double() - f64).abs().max()) <= BAR * host
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'bf16')
    assert model.infer_nhwc(A).dtype is torch.bfloat16
    assert float((model.infer(A, 'A').cpu() - half).abs().max()) < 0.1
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'fp64')
    with pytest.raises(GccError, match='GCC_RESNET_PRECISION=fp64'):
        model.infer_nhwc(A)
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'fp32')
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')                    # the older variable still refuses this model
    with pytest.raises(GccError, match=r'GCC_GEN_PRECISION=fp32.*U-Net only.*--model cyclegan'):
        model.infer_nhwc(A)


def test_pix2pix_resnet_infer_follows_the_variable(monkeypatch):
    from gcc_amd import ops
    from gcc_amd._lib import GccError
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    opt = options.parse(['--dataroot', './database/cityscapes/', '--model', 'pix2pix', '--gpu_ids', '0', '--backbone', 'resnet',
                         '--ngf', '8', '--ndf', '8'])
    opt.isTrain = True
    model = get_model_class(opt)(opt)
    model.model_eval()
    A = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(6)) * 2 - 1
    monkeypatch.delenv('GCC_RESNET_PRECISION', raising=False)
    monkeypatch.delenv('GCC_GEN_PRECISION', raising=False)
    assert model.infer_nhwc(A).dtype is torch.bfloat16
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'fp32')
    view = model.infer_nhwc(A)
    assert view.dtype is torch.float32 and tuple(view.shape) == tuple(A.shape)
    want = _fp32(model.G, A)
    assert torch.equal(ops.nhwc_to_nchw_f32(model.infer_nhwc({'A': A, 'B': A})).cpu().view(torch.int32), want.view(torch.int32))
    nchw = model.infer(A)
    assert nchw.dtype is torch.float32 and nchw.is_contiguous() and torch.equal(nchw.cpu().view(torch.int32), want.view(torch.int32))
    with torch.no_grad():
        _last_conv(model.netG).weight.mul_(0.5)
    model.refresh_weights()
    assert not torch.equal(model.infer(A).cpu(), want)
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'int8')
    with pytest.raises(GccError, match='GCC_RESNET_PRECISION=int8'):
        model.infer_nhwc(A)
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'fp32')
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')
    with pytest.raises(GccError, match=r'GCC_GEN_PRECISION=fp32.*U-Net only.*--backbone resnet'):
        model.infer_nhwc(A)


def test_cli_cyclegan_writes_the_bytes_of_the_fp32_image(tmp_path):
    from PIL import Image
    from gcc_amd import test as gtest
    from gcc_amd.data import create_dataset
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    root = tmp_path / 'data'
    (root / 'testA').mkdir(parents=True)
    (root / 'testB').mkdir(parents=True)
    rng = np.random.RandomState(0)
    for d, names in (('testA', ('h1', 'h2')), ('testB', ('z1', 'z2'))):
        for n in names:
            Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(str(root / d / (n + '.jpg')))
    argv = ['--dataroot', str(root), '--model', 'cyclegan', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--name', 'exp',
            '--checkpoints_dir', str(tmp_path / 'ck'), '--preprocess', 'none']           # the 64 x 64 files as they are
    opt = options.parse(argv)
    opt.isTrain = True
    model = get_model_class(opt)(opt)
    _range_filling(model.netG_A, model.G['A'], 5, 1, 64)
    model.save_models(2, str(tmp_path / 'save'))
    ckpt = str(tmp_path / 'save' / 'model_2.pth')
    env = dict(os.environ, PYTHONPATH=ROOT, GCC_RESNET_PRECISION='fp32')
    env.pop('GCC_GEN_PRECISION', None)
    r = subprocess.run([sys.executable, '-m', 'gcc_amd.test'] + argv + ['--pretrain_path', ckpt], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'generator precision: fp32' in r.stdout.splitlines(), r.stdout[-2000:]
    out = tmp_path / 'ck' / 'exp' / 'test_results'
    model.model_eval()
    n = differ = 0
    for data in create_dataset(gtest.test_overrides(opt), model.device):
        model.set_input(data)
        name = gtest.result_names(['fake_B'], model.image_paths, opt.direction)[0][1]
        png = np.asarray(Image.open(str(out / name)))
        assert np.array_equal(png, R.tensor2im(_fp32(model.G['A'], model.real_A.cpu()))[0].numpy()), name
        differ += int((png != R.tensor2im(_bf16(model.G['A'], model.real_A.cpu()))[0].numpy()).sum())
        n += 1
    assert n >= 2 and differ > 0                                       # and they are not the bf16 route's bytes
