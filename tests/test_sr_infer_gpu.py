"""SRGAN inference path: the eval-mode conv epilogue (gcc_conv_fprop_eval) on every route against fp32 PyTorch, the generator's
fused forward (SRResNetEngine.infer) against the oracle, its launch count and memory, the PSNR / SSIM evaluator against
oracle.metric_oracle and the built-in evaluation of `python -m gcc_amd.train`."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _rb(t):
    return t.bfloat16().float()


def _nhwc(ops, x):
    buf = ops.new_act(x.shape[0], x.shape[1], x.shape[2], x.shape[3], DEV)
    ops.nchw_to_nhwc(x.to(DEV).contiguous(), buf)
    return buf


# ---- the epilogue on each route ----------------------------------------------------------------------------------------
GEOMS = {'ring3': (1, 128, 85), 'igemm': (1, 17, 23), 'small': (1, 6, 7)}


def _eval_case(ops, _lib, N, H, W, Ci, Co, seed):
    g = torch.Generator().manual_seed(seed)
    x = _rb(torch.randn(N, Ci, H, W, generator=g))
    w = _rb(torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5))
    scale = torch.rand(Co, generator=g) * 1.5 + 0.25
    shift = torch.randn(Co, generator=g) * 0.3
    res = _rb(torch.randn(N, Co, H, W, generator=g))
    wp, _ = ops.pack_weights(w.to(DEV).contiguous(memory_format=torch.channels_last))
    return x, w, scale, shift, res, wp


def _check_variants(ops, _lib, x, w, scale, shift, res, wp, Co):
    N, _, H, W = x.shape
    acc = F.conv2d(x, w, padding=1)
    xd = _nhwc(ops, x)
    # the residual's pad channels hold non-zeros: they must not reach the output's (zero) pad channels
    rbase = torch.full((N, H, W, ops.ceil8(Co)), 1.5, dtype=torch.bfloat16, device=DEV)
    rbase[..., :Co] = res.permute(0, 2, 3, 1).to(DEV).bfloat16()
    rd = rbase.permute(0, 3, 1, 2)[:, :Co]
    sd, hd = scale.to(DEV), shift.to(DEV)
    for act, slope in ((_lib.EVAL_ACT_PRELU, -0.3), (_lib.EVAL_ACT_PRELU, 0.25), (_lib.EVAL_ACT_TANH, None),
                       (_lib.EVAL_ACT_NONE, None)):
        for with_res in (False, True):
            z = scale.view(1, -1, 1, 1) * acc + shift.view(1, -1, 1, 1)
            if act == _lib.EVAL_ACT_PRELU:
                z = F.prelu(z, torch.tensor([slope]))
            elif act == _lib.EVAL_ACT_TANH:
                z = torch.tanh(z)
            if with_res:
                z = z + res
            # every channel of the call's output must be written, the pad channels up to the next multiple of 8 as zeros
            base = torch.full((N, H, W, ops.ceil8(Co)), float('nan'), dtype=torch.bfloat16, device=DEV)
            out = base.permute(0, 3, 1, 2)[:, :Co]
            sl = torch.tensor([slope], device=DEV) if slope is not None else None
            ops.conv_fprop_eval(xd, wp, Co, 3, 1, 1, out, scale=sd, shift=hd, act=act, slope=sl,
                                residual=rd if with_res else None)
            torch.cuda.synchronize()
            got = ops.nhwc_to_nchw(out, Co).cpu()
            err = (got - z).abs()
            bar = 2.0 ** -8 * z.abs() + 1e-3
            assert bool((err <= bar).all()), (act, slope, with_res, float((err - bar).max()))
            assert bool((base[..., Co:] == 0).all())


def _assert_route_only(ops, case, Co, launches):
    """conv_fprop_eval(route_only=True) gives the launches the call would make, and launches nothing"""
    xd, wp = _nhwc(ops, case[0]), case[-1]
    N, _, H, W = xd.shape
    out = ops.new_act(N, Co, H, W, DEV)
    torch.cuda.synchronize()
    L = ops.lib()
    L.gcc_launch_count(1)
    assert ops.conv_fprop_eval(xd, wp, Co, 3, 1, 1, out, route_only=True) == launches
    assert L.gcc_launch_count(0) == 0


@pytest.mark.parametrize('thin', [1, 0])
@pytest.mark.parametrize('Ci,Co', [(64, 64), (64, 24), (24, 64), (13, 64)])
@pytest.mark.parametrize('geom', sorted(GEOMS))
def test_eval_epilogue_each_route(geom, Ci, Co, thin):
    from gcc_amd import _lib, ops
    N, H, W = GEOMS[geom]
    L = ops.lib()
    prev = L.gcc_set_option(_lib.OPT_IGEMM_THIN, thin)
    try:
        d = ops.conv_desc(N, H, W, Ci, Co, 3, 1, 1, ops.ceil8(Ci), ops.ceil8(Co))
        route = L.gcc_conv_eval_route(ctypes.byref(d), L.gcc_conv_eval_workspace(ctypes.byref(d)))
        expect = 4 if (thin and geom == 'ring3' and Ci % 8 == 0) else 0
        assert route == expect, (route, expect)
        case = _eval_case(ops, _lib, N, H, W, Ci, Co, Ci * 131 + Co * 7 + H)
        _assert_route_only(ops, case, Co, 1)                 # route 0 and the ring kernel alike: one launch
        _check_variants(ops, _lib, *case, Co)
    finally:
        L.gcc_set_option(_lib.OPT_IGEMM_THIN, prev)


@pytest.mark.parametrize('Ci,Co', [(128, 64), (128, 13)])
def test_eval_epilogue_split_k(Ci, Co):
    """a small grid with a long K loop runs split over K (partials, then the eval epilogue in the fold kernel)"""
    from gcc_amd import _lib, ops
    N, H, W = 1, 6, 7
    d = ops.conv_desc(N, H, W, Ci, Co, 3, 1, 1, ops.ceil8(Ci), ops.ceil8(Co))
    ws = ops.lib().gcc_conv_eval_workspace(ctypes.byref(d))
    assert ws > 0
    assert ops.lib().gcc_conv_eval_route(ctypes.byref(d), ws) == 5
    assert ops.lib().gcc_conv_eval_route(ctypes.byref(d), 0) == 0
    case = _eval_case(ops, _lib, N, H, W, Ci, Co, 77 + Co)
    _assert_route_only(ops, case, Co, 2)                     # partials, then the fold
    _check_variants(ops, _lib, *case, Co)


def test_eval_epilogue_rejects_bad_arguments():
    from gcc_amd import _lib, ops
    L = ops.lib()
    d = ops.conv_desc(1, 8, 8, 16, 16, 3, 1, 1, 16, 16)
    x, y = ops.new_act(1, 16, 8, 8, DEV), ops.new_act(1, 16, 8, 8, DEV)
    wp, _ = ops.pack_weights(torch.zeros(16, 16, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last))
    ep = _lib.eval_epilogue_t(None, None, None, None, 0, 0, _lib.EVAL_ACT_PRELU, 0, None, 0)       # PReLU without a slope
    assert L.gcc_conv_fprop_eval(ctypes.byref(d), x.data_ptr(), wp.data_ptr(), y.data_ptr(), ctypes.byref(ep), None) == -1
    ep = _lib.eval_epilogue_t(None, None, None, x.data_ptr(), 12, 0, _lib.EVAL_ACT_NONE, 0, None, 0)   # misaligned residual
    assert L.gcc_conv_fprop_eval(ctypes.byref(d), x.data_ptr(), wp.data_ptr(), y.data_ptr(), ctypes.byref(ep), None) == -1


# ---- the generator -------------------------------------------------------------------------------------------------------
def _srgan(ngf=64, filter_cfgs=None, seed=5):
    os.environ['GCC_VGG19_RANDOM'] = '1'
    from gcc_amd.models.SRGAN import SRGAN
    from gcc_amd.options import options
    opt = options.parse(['--dataroot', 'synthetic', '--model', 'srgan', '--ngf', str(ngf), '--ndf', '8', '--gpu_ids', '0'])
    opt.isTrain = True
    model = SRGAN(opt, filter_cfgs=filter_cfgs)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in model.netG.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_((torch.rand(m.num_features, generator=g) - 0.5).to(DEV))
                m.running_var.copy_((torch.rand(m.num_features, generator=g) * 1.5 + 0.5).to(DEV))
                m.weight.copy_((torch.rand(m.num_features, generator=g) + 0.5).to(DEV))
                m.bias.copy_((torch.randn(m.num_features, generator=g) * 0.1).to(DEV))
            elif isinstance(m, torch.nn.PReLU):
                m.weight.copy_((torch.rand(1, generator=g) * 0.6 - 0.3).to(DEV))
    model.refresh_weights()
    model.model_eval()
    return model, opt


def _lr(N, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    return (torch.rand(N, 3, h, w, generator=g) - mean) / std


def _infer(model, lr):
    from gcc_amd import ops
    G = model.G
    G.eval_coeffs()
    N, _, h, w = lr.shape
    x = ops.nchw_to_nhwc(lr.to(DEV).contiguous(), G.infer_input(N, h, w), cfill=8)
    out = G.infer(x)
    return ops.nhwc_to_nchw(out, 3).cpu()


@pytest.mark.parametrize('N,h,w', [(1, 17, 23), (1, 57, 86), (1, 128, 85), (2, 96, 96)])
@pytest.mark.parametrize('pruned', [False, True])
def test_generator_infer_vs_oracle(N, h, w, pruned):
    from oracle import gcc_oracle as O
    cfgs = [13, 24, 64, 8, 40, 64, 17, 32, 64, 48, 9, 64, 56, 64, 16, 24] if pruned else None
    model, _ = _srgan(64, cfgs, seed=11 + N + h)
    lr = _lr(N, h, w, seed=h * w)
    got = _infer(model, lr)
    sd = {k: v.detach().float().cpu() for k, v in model.netG.state_dict().items()}
    prev = O.EMULATE_BF16
    O.EMULATE_BF16 = False
    try:
        with torch.no_grad():
            ref = O.srresnet_forward(sd, _rb(lr), train=False)
    finally:
        O.EMULATE_BF16 = prev
    err = (got - ref).abs()
    assert float(err.max()) <= 3e-2 and float(err.mean()) <= 4e-3, (float(err.max()), float(err.mean()))
    # today's eval route on the same input: the fused path is no less accurate
    model.set_input({'lr': lr, 'hr': torch.zeros(N, 3, 4 * h, 4 * w), 'lr_names': ['a'] * N, 'hr_names': ['b'] * N})
    model.forward()
    old = model.fake_hr.float().cpu()
    old_err = float((old - ref).abs().mean())
    assert float(err.mean()) <= old_err * 1.05 + 1e-6, (float(err.mean()), old_err)


def test_generator_infer_launch_count():
    from gcc_amd import ops
    model, _ = _srgan(64)
    G, L = model.G, ops.lib()
    G.eval_coeffs()
    x = ops.nchw_to_nhwc(_lr(1, 96, 96, 3).to(DEV).contiguous(), G.infer_input(1, 96, 96), cfill=8)
    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    G.infer(x)
    n = L.gcc_launch_count(1)
    torch.cuda.synchronize()
    assert n <= 40, n
    L.gcc_launch_count(1)
    G.eval_coeffs()                  # the coefficients of all 33 BatchNorms and the plain convs' biases: one launch
    assert L.gcc_launch_count(1) == 1


def test_generator_infer_memory_is_flat_across_sizes():
    model, _ = _srgan(64)
    sizes = [(128, 128), (120, 90), (96, 96), (85, 128), (72, 72), (70, 70), (64, 64), (57, 86), (32, 48), (17, 23), (9, 11),
             (6, 7)]
    ctx0, bufs0 = set(model.G.ctx), set(model._bufs)
    _infer(model, _lr(1, *sizes[0], seed=1))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for i, (h, w) in enumerate(sizes[1:]):
        _infer(model, _lr(1, h, w, seed=i + 2))
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() - base <= 1 << 20, ((h, w), torch.cuda.memory_allocated() - base)
    assert set(model.G.ctx) == ctx0 and set(model._bufs) == bufs0


# ---- the evaluator ---------------------------------------------------------------------------------------------------------
SET5_SIZES = [(512, 512), (288, 288), (256, 256), (280, 280), (228, 344)]


def _write_pngs(folder, sizes, seed):
    from PIL import Image
    folder.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(seed)
    for i, (h, w) in enumerate(sizes):
        base = rng.integers(0, 256, size=(h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        img = np.kron(base, np.ones((8, 8, 1), dtype=np.uint8))[:h, :w]          # blocky: some structure to score
        noise = rng.integers(-20, 21, size=img.shape)
        Image.fromarray(np.clip(img.astype(int) + noise, 0, 255).astype(np.uint8)).save(folder / ('img%02d.png' % i))


def test_evaluator_matches_metric_oracle(tmp_path):
    from gcc_amd import metric
    from gcc_amd.data import create_dataset
    from oracle import metric_oracle as M
    _write_pngs(tmp_path / 'test' / 'Set5', SET5_SIZES, 3)
    model, opt = _srgan(16)
    opt.dataroot = str(tmp_path)
    psnr, ssim = metric.test_srgan_psnr(model, opt, 'Set5')
    # the path's own output images, scored by the CPU restatement
    eopt = copy.deepcopy(opt)
    eopt.phase, eopt.batch_size, eopt.serial_batches = 'test/Set5', 1, True
    ps, ss = [], []
    for batch in create_dataset(eopt, DEV):
        torch.cuda.current_stream().wait_event(batch['ready'])
        fake = _infer(model, batch['lr']).numpy()
        real = batch['hr'].float().cpu().numpy()
        ps.append(M.psnr_y(fake, real))
        ss.append(M.ssim_y(fake, real))
    assert len(ps) == 5
    assert abs(psnr - float(np.mean(ps))) <= 1e-3, (psnr, np.mean(ps))
    assert abs(ssim - float(np.mean(ss))) <= 1e-6, (ssim, np.mean(ss))


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def _cli_root(root, with_test):
    _write_pngs(root / 'train', [(48, 48)] * 4, 1)
    if with_test:
        _write_pngs(root / 'test' / 'Set5', [(36, 44), (28, 33)], 2)
        _write_pngs(root / 'test' / 'Set14', [(41, 30)], 4)
    return root


@pytest.mark.parametrize('replay', ['0', '1'])
def test_cli_evaluates_srgan_each_epoch(tmp_path, monkeypatch, replay):
    from gcc_amd import train
    from gcc_amd.options import options
    monkeypatch.setenv('GCC_VGG19_RANDOM', '1')
    monkeypatch.setenv('GCC_REPLAY', replay)
    argv = ['--model', 'srgan', '--ngf', '8', '--ndf', '8', '--image_size', '32', '--batch_size', '2', '--n_epochs', '2',
            '--save_epoch_freq', '1', '--gpu_ids', '0', '--print_freq', '1000', '--name', 'e']
    finals = {}
    for with_test in (True, False):
        root = _cli_root(tmp_path / ('data%d' % with_test), with_test)
        ck = tmp_path / ('ck%d' % with_test)
        torch.manual_seed(0)
        np.random.seed(0)
        import random
        random.seed(0)
        model = train.main(['--dataroot', str(root), '--checkpoints_dir', str(ck)] + argv)
        torch.cuda.synchronize()
        finals[with_test] = {k: v.detach().cpu().clone() for k, v in model.netG.state_dict().items()}
        log = (ck / 'e' / 'logger.log').read_text()
        epochs = options.parse(['--dataroot', str(root)] + argv).n_epochs
        if with_test:
            lines = re.findall(r'(Set5|Set14):PSNR: ([0-9.]+)\| SSIM: ([0-9.]+)', log)
            assert sum(1 for s, _, _ in lines if s == 'Set5') == epochs
            assert sum(1 for s, _, _ in lines if s == 'Set14') == epochs
            for name in ('Set5', 'Set14'):
                path = ck / 'e' / 'checkpoints' / ('model_best_%s.pth' % name)
                assert path.exists()
                value = torch.load(path, map_location='cpu', weights_only=False)['psnr']
                logged = [float(v) for s, p, q in lines if s == name for v in (p, q)]
                assert any(abs(value - v) <= 0.005 for v in logged), (name, value, logged)
        else:
            assert 'PSNR' not in log
            assert not list((ck / 'e').glob('checkpoints/model_best_*.pth'))
        del model
    for k in finals[True]:
        assert torch.equal(finals[True][k], finals[False][k]), k
