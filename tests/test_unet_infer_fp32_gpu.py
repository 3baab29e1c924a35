"""The U-Net generator's fp32 inference route (UnetEngine.infer(x, 'fp32'): one gcc_conv_eval_f32_unet launch per convolution)
against the float64 restatement of tests/_unet_f64.py: the reference checkpoint, seeded nets whose images fill [-1, 1], bytes of
tensor2im, launches and allocation, repeatability, a pruned student, isolation from the bf16 route and from training, and
GCC_GEN_PRECISION from Pix2PixModel.infer_nhwc through the scorers to `python -m gcc_amd.test`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _unet_f64 as U

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 8                      # the project's bar for its fp32 routes: 8 x the error of an fp32 evaluation of the same network


def _opt(extra=(), ngf=8, num_downs=8, dataroot='./database/cityscapes/'):
    from gcc_amd.options import options
    opt = options.parse(['--dataroot', dataroot, '--model', 'pix2pix', '--gpu_ids', '0', '--ngf', str(ngf), '--ndf', '8',
                         '--num_downs', str(num_downs), '--load_size', '256', '--crop_size', '256'] + list(extra))
    opt.isTrain = True
    return opt


def _model(opt, f=None, c=None):
    from gcc_amd.models import get_model_class
    return get_model_class(opt)(opt, filter_cfgs=f, channel_cfgs=c)


def _host_sd(model):
    return {k: v.detach().cpu().clone() for k, v in model.netG.state_dict().items()}


def _fp32(model, A):
    """the fp32 route's image of the host batch A as NCHW fp32 on the host, through the engine"""
    from gcc_amd import ops
    G = model.G
    N, _, H, W = A.shape
    G.eval_coeffs('fp32')
    out = G.infer(ops.nchw_to_nhwc_f32(A.to(DEV).contiguous(), G.infer_input(N, H, W, 'fp32')), 'fp32')
    assert out.dtype is torch.float32 and tuple(out.shape) == (N, 3, H, W) and out.stride(1) == 1
    return ops.nhwc_to_nchw_f32(out).cpu()


def _bf16(model, A):
    from gcc_amd import ops
    G = model.G
    N, _, H, W = A.shape
    G.eval_coeffs()
    return ops.nhwc_to_nchw(G.infer(ops.nchw_to_nhwc(A.to(DEV).contiguous(), G.infer_input(N, H, W), cfill=8)), 3).cpu()


def _image_conv(model):
    return dict(model.netG.named_modules())['model.model.3']


def _range_filling(model, seed, N, size):
    """He-normal weights, BatchNorms randomized as tests/test_unet_infer_gpu.py's _randomize_bn does, a zero image bias and the
    image conv scaled so that the float64 pre-tanh standard deviation is 0.5: the image fills [-1, 1] without saturating.
    Returns (input, float64 image)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.netG.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                fan_in = (m.weight.shape[1] if isinstance(m, torch.nn.Conv2d) else m.weight.shape[0]) * 16
                # a transposed conv of stride 2 sums a quarter of its taps per output pixel
                std = (2.0 / fan_in) ** 0.5 * (2.0 if isinstance(m, torch.nn.ConvTranspose2d) else 1.0)
                m.weight.copy_((torch.randn(m.weight.shape, generator=g) * std).to(DEV))
                if m.bias is not None:
                    m.bias.zero_()
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_((torch.randn(m.num_features, generator=g) * 0.2).to(DEV))
                m.running_var.copy_((torch.rand(m.num_features, generator=g) * 1.5 + 0.5).to(DEV))
                m.weight.copy_((torch.rand(m.num_features, generator=g) + 0.5).to(DEV))
                m.bias.copy_((torch.randn(m.num_features, generator=g) * 0.1).to(DEV))
        A = torch.rand(N, 3, size, size, generator=g) * 2 - 1
        last = _image_conv(model)
        pre = U.unet_eval(_host_sd(model), A, pre_tanh=True)
        last.weight.mul_(0.5 / float(pre.std()))
    model.refresh_weights()
    return A, U.unet_eval(_host_sd(model), A)


NETS = {'ngf8_d8_256': (8, 8, 256, 2), 'ngf12_d6_64': (12, 6, 64, 1), 'ngf5_d7_128': (5, 7, 128, 1)}


@functools.lru_cache(maxsize=None)
def _net(name):
    ngf, D, size, N = NETS[name]
    model = _model(_opt(['--no_dropout'], ngf=ngf, num_downs=D))
    A, f64 = _range_filling(model, 100 + ngf, N, size)
    return model, A, f64


def _flip_share(image, f64):
    """(share of tensor2im bytes that differ from the float64 image's, the largest byte difference)"""
    d = (U.tensor2im(image).int() - U.tensor2im(f64).int()).abs()
    return float((d != 0).double().mean()), int(d.max())


# ---- 1. the reference checkpoint ----------------------------------------------------------------------------------------------
def test_reference_checkpoint_at_the_references_own_error(golden_dir):
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    from tests.test_checkpoint_gpu import ARGV
    z = np.load(os.path.join(golden_dir, 'ref_checkpoint_pix2pix.npz'))
    opt = options.parse(ARGV)
    opt.isTrain = True
    model = get_model_class(opt)(opt)
    model.load_models(os.path.join(golden_dir, 'ref_checkpoint_pix2pix.pth'))
    A, fake_B = torch.from_numpy(z['A']), torch.from_numpy(z['fake_B'])
    f64 = U.unet_eval(_host_sd(model), A)
    ref = float((fake_B.double() - f64).abs().max())
    got = float((_fp32(model, A).double() - f64).abs().max())
    bf16 = float((_bf16(model, A).double() - f64).abs().max())
    print('reference checkpoint, max |. - f64|: reference fake_B %.3g, native fp32 %.3g, native bf16 %.3g' % (ref, got, bf16))
    assert 0 < ref <= 1e-7 and got <= BAR * ref


# ---- 2. seeded nets whose images fill the range ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(NETS))
def test_range_filling_net_error_and_bytes(name):
    model, A, f64 = _net(name)
    # the condition, on the float64 image: it fills the range and does not sit in tanh's flat ends
    assert float((f64.abs() > 0.99).double().mean()) <= 0.01 and float(f64.std()) >= 0.2
    host = U.unet_eval(_host_sd(model), A, torch.float32)
    err_host = float((host.double() - f64).abs().max())
    got = _fp32(model, A)
    err = float((got.double() - f64).abs().max())
    bf16 = _bf16(model, A)
    err16 = float((bf16.double() - f64).abs().max())
    share, worst = _flip_share(got, f64)
    share_host, _ = _flip_share(host, f64)
    share16, worst16 = _flip_share(bf16, f64)
    print('%s: std %.3f, max |. - f64|: fp32 torch restatement %.3g, native fp32 %.3g, native bf16 %.3g; bytes that differ from '
          'float64\'s: restatement %.3g, native fp32 %.3g (largest step %d), native bf16 %.3g (largest step %d)'
          % (name, float(f64.std()), err_host, err, err16, share_host, share, worst, share16, worst16))
    assert err <= BAR * err_host
    assert worst <= 1 and share <= 1e-3
    # the bytes the device makes of the fp32 image (gcc_image_to_u8_f32) are tensor2im's
    from gcc_amd import ops
    N, _, H, W = A.shape
    view = model.G.infer(ops.nchw_to_nhwc_f32(A.to(DEV).contiguous(), model.G.infer_input(N, H, W, 'fp32')), 'fp32')
    assert torch.equal(ops.image_to_u8(view).cpu(), U.tensor2im(got))


# ---- 3. launches and allocation -----------------------------------------------------------------------------------------------
def test_two_d_launches_and_no_allocation():
    from gcc_amd import ops
    L = ops.lib()
    model, _, _ = _net('ngf8_d8_256')
    G = model.G
    G.eval_coeffs('fp32')
    for N in (1, 3):
        x = G.infer_input(N, 256, 256, 'fp32')
        G.infer(x, 'fp32')
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    L.gcc_launch_count(1)
    G.eval_coeffs('fp32')
    torch.cuda.synchronize()
    coeff_launches = L.gcc_launch_count(1)
    assert torch.cuda.memory_allocated() == m0
    for N in (1, 3):
        x = G.infer_input(N, 256, 256, 'fp32')
        assert G.infer_launches(N, 256, 256, 'fp32') == 2 * G.D == 16
        assert L.gcc_launch_count(1) == 0                         # the route twin launches nothing
        G.infer(x, 'fp32')
        torch.cuda.synchronize()
        assert L.gcc_launch_count(1) == 16
    for N, H, W in ((1, 256, 512), (2, 256, 256), (1, 512, 256), (3, 256, 256)):   # nothing larger than the slab has seen
        G.infer(G.infer_input(N, H, W, 'fp32'), 'fp32')
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0
    print('eval_coeffs(fp32): %d launches besides the weight copies' % coeff_launches)


def test_memory_is_flat_across_two_sizes():
    model, _, _ = _net('ngf12_d6_64')
    G = model.G
    G.eval_coeffs('fp32')
    G.infer(G.infer_input(2, 128, 128, 'fp32'), 'fp32')
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    for N, H, W in ((1, 64, 64), (2, 128, 128), (1, 64, 128), (2, 64, 64)):
        G.infer(G.infer_input(N, H, W, 'fp32'), 'fp32')
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0


def test_engine_names_a_bad_precision_and_a_missing_refresh():
    from gcc_amd._lib import GccError
    model = _model(_opt(['--no_dropout'], ngf=8, num_downs=5))
    G = model.G
    assert G.PRECISIONS == ('bf16', 'fp32')
    for call in (lambda: G.eval_coeffs('fp16'), lambda: G.infer_input(1, 32, 32, 'fp16'), lambda: G.infer(None, 'fp16'),
                 lambda: G.infer_launches(1, 32, 32, 'fp16')):
        with pytest.raises(GccError, match='fp16'):
            call()
    with pytest.raises(GccError, match=r"eval_coeffs\('fp32'\) first"):
        G.infer(G.infer_input(1, 32, 32, 'fp32'), 'fp32')
    G.eval_coeffs('fp32')
    with pytest.raises(GccError, match='multiples of 32'):
        G.infer(G.infer_input(1, 48, 32, 'fp32'), 'fp32')


# ---- 4. repeatability ---------------------------------------------------------------------------------------------------------
def test_repeated_runs_and_batches_give_identical_bits():
    model, A, _ = _net('ngf12_d6_64')
    g = torch.Generator().manual_seed(77)
    B = torch.cat([A, torch.rand(2, 3, 64, 64, generator=g) * 2 - 1])
    first = _fp32(model, B)
    assert torch.equal(first.view(torch.int32), _fp32(model, B).view(torch.int32))
    for n in range(3):
        assert torch.equal(_fp32(model, B[n:n + 1]).view(torch.int32), first[n:n + 1].contiguous().view(torch.int32)), n


# ---- 5. a pruned student ------------------------------------------------------------------------------------------------------
def test_pruned_student_with_a_removed_block(golden_dir):
    z = np.load(os.path.join(golden_dir, 'pix2pix_pruned_removed_d8.npz'))
    f, c = [int(v) for v in z['k6.f']], [int(v) for v in z['k6.c']]
    model = _model(_opt(['--no_dropout'], ngf=32), f, c)
    G = model.G
    assert G.D == 6 and G.inner_identity and any(w % 8 for w in G.width + G.uwidth)
    A, f64 = _range_filling(model, 9, 2, 64)
    assert U.depth(_host_sd(model)) == 6
    err_host = float((U.unet_eval(_host_sd(model), A, torch.float32).double() - f64).abs().max())
    err = float((_fp32(model, A).double() - f64).abs().max())
    print('pruned k6 (widths %s | %s): fp32 torch restatement %.3g, native fp32 %.3g' % (G.width, G.uwidth, err_host, err))
    assert G.infer_launches(2, 64, 64, 'fp32') == 12
    assert err <= BAR * err_host


# ---- 6. isolation ------------------------------------------------------------------------------------------------------------
def test_bf16_route_and_training_are_untouched():
    model = _model(_opt(['--no_dropout'], ngf=12, num_downs=6))     # a model of its own: the training step moves its weights
    A, _ = _range_filling(model, 21, 2, 64)
    before = _bf16(model, A)
    slab, table = model.G._ev_slab, model.G._ev_table.table
    _fp32(model, A)
    _fp32(model, torch.cat([A, A, A]))
    assert model.G._ev_slab is slab and model.G._ev_table.table is table
    N, _, H, W = A.shape
    from gcc_amd import ops
    again = ops.nhwc_to_nchw(model.G.infer(ops.nchw_to_nhwc(A.to(DEV).contiguous(), model.G.infer_input(N, H, W), cfill=8)), 3).cpu()
    assert torch.equal(before.view(torch.int32), again.view(torch.int32))
    # a training step still works afterwards, and the fp32 route follows the new weights
    fake = _fp32(model, A)
    model.model_train()
    model.set_input({'A': A, 'B': A.flip(3).clone(), 'A_paths': ['a'], 'B_paths': ['b']})
    model.optimize_parameters()
    losses = model.get_current_losses()
    assert all(np.isfinite(v) for v in losses.values()), losses
    model.model_eval()
    moved = _fp32(model, A)
    assert torch.isfinite(moved).all() and not torch.equal(moved, fake)
    f64 = U.unet_eval(_host_sd(model), A)
    host = float((U.unet_eval(_host_sd(model), A, torch.float32).double() - f64).abs().max())
    assert float((moved.double() - f64).abs().max()) <= BAR * host


# ---- 7. the variable, the scorers, the CLI ------------------------------------------------------------------------------------
def test_infer_nhwc_follows_the_variable(monkeypatch):
    from gcc_amd import ops
    from gcc_amd._lib import GccError
    model, A, f64 = _net('ngf12_d6_64')
    model.model_eval()
    monkeypatch.delenv('GCC_GEN_PRECISION', raising=False)
    assert model.infer_nhwc(A).dtype is torch.bfloat16
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')
    view = model.infer_nhwc(A)
    assert view.dtype is torch.float32 and tuple(view.shape) == tuple(A.shape)
    want = _fp32(model, A)
    assert torch.equal(ops.nhwc_to_nchw_f32(model.infer_nhwc({'A': A, 'B': A})).cpu().view(torch.int32), want.view(torch.int32))
    nchw = model.infer(A)
    assert nchw.dtype is torch.float32 and nchw.is_contiguous() and torch.equal(nchw.cpu().view(torch.int32), want.view(torch.int32))
    # the refresh is keyed to the generation per precision: new weights reach both routes
    with torch.no_grad():
        _image_conv(model).weight.mul_(0.5)
    model.refresh_weights()
    half = model.infer(A).cpu()
    assert not torch.equal(half, want)
    monkeypatch.setenv('GCC_GEN_PRECISION', 'bf16')
    assert float((model.infer(A).cpu() - half).abs().max()) < 0.05
    with torch.no_grad():
        _image_conv(model).weight.mul_(2.0)
    model.refresh_weights()
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp64')
    with pytest.raises(GccError, match='GCC_GEN_PRECISION=fp64'):
        model.infer_nhwc(A)


def test_fp32_with_the_resnet_backbone_is_refused(monkeypatch):
    from gcc_amd._lib import GccError
    model = _model(_opt(['--backbone', 'resnet'], ngf=8))
    model.model_eval()
    A = torch.rand(1, 3, 64, 64) * 2 - 1
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')
    with pytest.raises(GccError, match=r'GCC_GEN_PRECISION=fp32.*U-Net only.*--backbone resnet'):
        model.infer_nhwc(A)
    monkeypatch.delenv('GCC_GEN_PRECISION')
    assert model.infer_nhwc(A).dtype is torch.bfloat16


def test_cityscapes_scorer_scores_the_bytes_of_the_fp32_image(tmp_path, monkeypatch):
    from gcc_amd import ops
    from gcc_amd import test as gtest
    from gcc_amd.data import create_dataset
    from gcc_amd.metric import cityscapes as CS
    from gcc_amd.metric import mIoU_score
    from tests import _miou_emul as E
    from tests.test_miou_cityscapes_gpu import ARGV, _Keep, _root
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    root, drn, names = _root(tmp_path, np.load(E.GOLDEN))
    opt = options.parse(['--dataroot', str(root), '--drn_path', str(drn), '--checkpoints_dir', str(tmp_path / 'ck')] + ARGV)
    opt.isTrain = True
    torch.manual_seed(3)
    model = get_model_class(opt)(opt)
    model.model_eval()
    keep = _Keep(torch.jit.load(str(drn), map_location=DEV))
    evaluate = CS.cityscapes_evaluator(keep)
    monkeypatch.delenv('GCC_GEN_PRECISION', raising=False)
    v16 = evaluate(model, opt)[0][0]
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')
    value = evaluate(model, opt)[0][0]
    fakes = []
    for data in create_dataset(gtest.test_overrides(opt), model.device):
        view = model.infer_nhwc(data)
        assert view.dtype is torch.float32
        u8 = ops.image_to_u8(view)
        assert torch.equal(CS.seg_input(view).view(torch.int32), CS.seg_input(u8).view(torch.int32))
        fakes.append(u8.cpu().numpy()[0])
    got = mIoU_score.test(fakes, sorted(names), keep.seg, DEV, table_path=str(root / 'table.txt'), data_dir=str(root), use_tqdm=False)
    print('stand-in segmenter mIoU: generator fp32 %.4f, bf16 %.4f' % (value, v16))
    assert got == value


def test_fid_scorer_scores_the_bytes_of_the_fp32_image(tmp_path, monkeypatch):
    from gcc_amd import ops
    from gcc_amd import test as gtest
    from gcc_amd.data import create_dataset
    from gcc_amd.metric import fid_eval as FE
    from tests.test_fid_eval_gpu import _Keep, _argv, _inception, _model as _fid_model, _pix2pix_root
    root = _pix2pix_root(tmp_path)
    model, opt = _fid_model(_argv('pix2pix', root, tmp_path))
    net = torch.jit.load(str(_inception(tmp_path)), map_location=DEV)
    monkeypatch.delenv('GCC_GEN_PRECISION', raising=False)
    v16 = FE.fid_evaluator(net, batch_size=4)(model, opt)[0][0]
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')
    keep = _Keep(net)
    (value, _), = FE.fid_evaluator(keep, batch_size=4)(model, opt)
    topt = gtest.test_overrides(opt)
    sc = FE.fid_evaluator(net, batch_size=4).scorer(model, topt)
    fed = []
    for data in create_dataset(topt, model.device):
        view = model.infer_nhwc(data)
        assert view.dtype is torch.float32
        u8 = ops.image_to_u8(view)
        fed.append((u8.cpu().double() / 255).float().permute(0, 3, 1, 2))
        sc.add(data['A_paths'][0], u8)
    want = torch.cat(fed)
    got = torch.cat(keep.inputs).cpu()
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
    print('stand-in Inception FID: generator fp32 %.6f, bf16 %.6f' % (value, v16))
    assert sc.result()[0] == value


def test_cli_writes_the_bytes_of_the_fp32_image(tmp_path):
    from PIL import Image
    from gcc_amd import test as gtest
    from gcc_amd.data import create_dataset
    from gcc_amd.options import options
    root = tmp_path / 'data'
    (root / 'val').mkdir(parents=True)
    rng = np.random.RandomState(0)
    names = ['frankfurt_1', 'lindau_22']
    for n in names:
        Image.fromarray(rng.randint(0, 256, (256, 512, 3), dtype=np.uint8)).save(str(root / 'val' / (n + '.jpg')))
    argv = ['--dataroot', str(root), '--model', 'pix2pix', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--name', 'exp',
            '--checkpoints_dir', str(tmp_path / 'ck')]
    opt = options.parse(argv)
    opt.isTrain = True
    model = _model(opt)
    _range_filling(model, 5, 1, 256)
    model.save_models(3, str(tmp_path / 'save'))
    ckpt = str(tmp_path / 'save' / 'model_3.pth')
    env = dict(os.environ, PYTHONPATH=ROOT, GCC_GEN_PRECISION='fp32')
    r = subprocess.run([sys.executable, '-m', 'gcc_amd.test'] + argv + ['--pretrain_path', ckpt], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'generator precision: fp32' in r.stdout.splitlines(), r.stdout[-2000:]
    out = tmp_path / 'ck' / 'exp' / 'test_results'
    model.model_eval()
    differ = 0
    for data in create_dataset(gtest.test_overrides(opt), model.device):
        model.set_input(data)
        name = gtest.result_names(['fake_B'], model.image_paths, opt.direction)[0][1]
        png = np.asarray(Image.open(str(out / name)))
        assert np.array_equal(png, U.tensor2im(_fp32(model, model.real_A.cpu()))[0].numpy()), name
        differ += int((png != U.tensor2im(_bf16(model, model.real_A.cpu()))[0].numpy()).sum())
    assert differ > 0                                               # and they are not the bf16 route's bytes
