"""MobileResnet inference path: gcc_dw_inorm_fwd (depthwise 3x3 + InstanceNorm in one launch) against fp32 PyTorch, the fused
generator (MobileResnetEngine.infer, Pix2PixModel / MobileCycleGANModel.infer) against the reference's images and the oracle,
its launch count, memory and isolation from training, and `python -m gcc_amd.test --model cyclegan` end to end."""
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gcc_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rb(t):
    return t.bfloat16().float()


def _ops():
    from gcc_amd import ops
    return ops


def _nhwc(ops, t):
    N, C, H, W = t.shape
    return ops.nchw_to_nhwc(t.float().contiguous().to(DEV), ops.new_act(N, C, H, W, DEV))


def _err(a, b):
    e = (a.detach().float().cpu() - b.detach().float().cpu()).abs()
    return e.max().item(), e.mean().item()


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------
def _ref(mode, x, w, r=None, eps=1e-5):
    """fp32 torch on bf16-rounded operands; u rounded to bf16 as the kernel (and the training route) store it"""
    if mode == 0:
        u = x
    elif mode == 1:
        u = _rb(F.relu(F.instance_norm(x, eps=eps)))
    else:
        u = _rb(r + F.instance_norm(x, eps=eps))
    d = F.conv2d(F.pad(u, (1, 1, 1, 1), mode='reflect'), w, groups=w.shape[0])
    return F.instance_norm(d, eps=eps), u


def _case(mode, N, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = _rb(torch.randn(N, C, H, W, generator=g) * 1.5 + 0.3)
    r = _rb(torch.randn(N, C, H, W, generator=g))
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.4
    return x, r, w


def _full(t):
    """the whole NHWC storage of an activation view [N, H, W, ld]"""
    N, C, H, W = t.shape
    ld = t.stride(2) // W if H > 1 else t.stride(3)
    return t.as_strided((N, H, W, ld), (H * W * ld, W * ld, ld, 1))


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('HW', [(16, 16), (64, 64), (96, 128)])
def test_dw_inorm_against_fp32(mode, N, HW):
    ops = _ops()
    lib = ops.lib()
    assert lib.gcc_device_error(1) == 0
    H, W = HW
    for C in (3, 15, 17, 96, 192, 256):
        x, r, w = _case(mode, N, H, W, C, 1000 * mode + 10 * N + C + H)
        yref, uref = _ref(mode, x, w, r)
        xd, rd = _nhwc(ops, x), _nhwc(ops, r)
        y, u = ops.new_act(N, C, H, W, DEV), ops.new_act(N, C, H, W, DEV)
        _full(y).fill_(3.0)
        _full(u).fill_(3.0)
        kw = dict(r=rd, u_out=u) if mode == 2 else {}
        route = ops.dw_inorm_route(mode, xd, w.to(DEV), y, **kw)
        if N == 3 and H * W > 64 * 64 and C >= 192:
            # more than 8 pixels per lane and sweep: declined (the engine runs forward()'s launches there)
            assert route == -2
            continue
        assert route == 1, (mode, N, H, W, C)
        ops.dw_inorm(mode, xd, w.to(DEV), y, **kw)
        y1 = _full(y).clone()
        ops.dw_inorm(mode, xd, w.to(DEV), y, **kw)          # a second launch finds the first one's tags: same bits
        torch.cuda.synchronize()
        assert torch.equal(_full(y), y1), (mode, N, H, W, C)
        got = y.float().cpu()
        e = (got - yref).abs()
        # a bar of its own, absolute on a unit-variance map: max 3e-2 (a few bf16 ulps of |y| <= 4), mean 4e-3
        assert e.max().item() <= 3e-2 and e.mean().item() <= 4e-3, (mode, N, H, W, C, e.max().item(), e.mean().item())
        assert not _full(y)[..., C:].any(), 'pad channels of y'
        if mode == 2:
            ug = u.float().cpu()        # one bf16 rounding of r + IN(p): at most one ulp from torch's
            assert ((ug - uref).abs() <= uref.abs() * 2.0 ** -7 + 1e-3).all(), 'u_out != bf16(r + IN(p))'
            assert not _full(u)[..., C:].any(), 'pad channels of u_out'
    assert lib.gcc_device_error(0) == 0


def test_dw_inorm_rejects_bad_arguments_and_short_workspace():
    import ctypes
    from gcc_amd import _lib
    ops = _ops()
    L = ops.lib()
    x = ops.new_act(1, 16, 16, 16, DEV)
    y = ops.new_act(1, 16, 16, 16, DEV)
    w = torch.zeros(16, 1, 3, 3, device=DEV)
    d = ops.dw_inorm_desc(_lib.DWIN_RESIDUAL, x, w, y)           # no r / u_out
    assert L.gcc_dw_inorm_fwd(ctypes.byref(d), None) == -1
    assert L.gcc_dw_inorm_route(ctypes.byref(d)) == -1
    d = ops.dw_inorm_desc(_lib.DWIN_PLAIN, x, w, y)
    d.ldx = 12
    assert L.gcc_dw_inorm_fwd(ctypes.byref(d), None) == -1
    d = ops.dw_inorm_desc(_lib.DWIN_PLAIN, x, w, y)
    d.mode = 3
    assert L.gcc_dw_inorm_fwd(ctypes.byref(d), None) == -1
    short = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    d = ops.dw_inorm_desc(_lib.DWIN_PLAIN, x, w, y, workspace=short)
    assert L.gcc_dw_inorm_route(ctypes.byref(d)) == -3
    assert L.gcc_dw_inorm_fwd(ctypes.byref(d), None) == -3
    big = ops.new_act(65, 16, 8, 8, DEV)
    bigy = ops.new_act(65, 16, 8, 8, DEV)
    d = ops.dw_inorm_desc(_lib.DWIN_PLAIN, big, w, bigy)
    L.gcc_launch_count(1)
    assert L.gcc_dw_inorm_route(ctypes.byref(d)) == -2
    assert L.gcc_dw_inorm_fwd(ctypes.byref(d), None) == -2
    assert L.gcc_launch_count(0) == 0
    torch.cuda.synchronize()
    assert L.gcc_device_error(0) == 0


def test_dw_inorm_on_four_streams_make_progress():
    """four launches with in-launch exchanges on four streams stay resident together: the single-stream bits, no error"""
    ops = _ops()
    lib = ops.lib()
    assert lib.gcc_device_error(1) == 0
    streams = [torch.cuda.Stream() for _ in range(4)]
    cases = []
    for i in range(4):
        C = 64 + 32 * i
        x, r, w = _case(2, 1, 64, 64, C, 50 + i)
        cases.append((_nhwc(ops, x), _nhwc(ops, r), w.to(DEV), C))
    ref = []
    for xd, rd, w, C in cases:
        y, u = ops.new_act(1, C, 64, 64, DEV), ops.new_act(1, C, 64, 64, DEV)
        ops.dw_inorm(2, xd, w, y, r=rd, u_out=u)
        torch.cuda.synchronize()
        ref.append((y.clone(), u.clone()))
    outs = [(ops.new_act(1, C, 64, 64, DEV), ops.new_act(1, C, 64, 64, DEV)) for _, _, _, C in cases]
    for rnd in range(40):
        for s_, (xd, rd, w, C), (y, u) in zip(streams, cases, outs):
            with ops.on_stream(s_):
                ops.dw_inorm(2, xd, w, y, r=rd, u_out=u)
        if rnd % 20 == 19:
            torch.cuda.synchronize()
            assert lib.gcc_device_error(0) == 0, hex(lib.gcc_device_error(0))
            for (y, u), (ry, ru) in zip(outs, ref):
                assert torch.equal(y, ry) and torch.equal(u, ru)


# ---- the generator ----------------------------------------------------------------------------------------------------
def _resnet_engine(ngf, seed, n_blocks=9, cfg=None):
    from gcc_amd import engine
    from gcc_amd.models.Pix2Pix import MobileResnetGenerator
    from tests.golden.recipe import recipe_state_dict
    net = MobileResnetGenerator(ngf=ngf, n_blocks=n_blocks, cfg=cfg) if cfg is not None else \
        MobileResnetGenerator(ngf=ngf, n_blocks=n_blocks)
    net = net.to(DEV)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
    net.load_state_dict({k: v.to(DEV) for k, v in recipe_state_dict(shapes, seed).items()})
    engine.FlatParams(list(net.parameters()), DEV)
    eng = engine.MobileResnetEngine(net, DEV)
    eng.repack()
    return net, eng


def _infer(eng, x):
    ops = _ops()
    N, _, H, W = x.shape
    xin = eng.infer_input(N, H, W)
    ops.nchw_to_nhwc(x.float().contiguous().to(DEV), xin, cfill=8)
    return ops.nhwc_to_nchw(eng.infer(xin), 3).cpu()


def _forward(eng, x):
    ops = _ops()
    N, _, H, W = x.shape
    c = eng._ctx(N, H, W, 'main')
    ops.nhwc_copy(_nhwc(ops, x), 0, c.x_in, 0, 3)
    eng.forward(c, train=False)
    return ops.nhwc_to_nchw(c.out, 3).cpu()


def test_engine_served_and_declined_geometry():
    """a geometry the kernel serves (N = 2) and one it declines (N = 65: the blocks fall back to forward()'s launches)"""
    ops = _ops()
    net, eng = _resnet_engine(8, 31, n_blocks=2)
    g = torch.Generator().manual_seed(5)
    for N, H in ((2, 32), (65, 16)):
        x = _rb(torch.rand(N, 3, H, H, generator=g) * 2 - 1)
        xin = eng.infer_input(N, H, H)
        dw = eng.blocks[0].dw1
        probe = ops.new_act(N, dw.C, H // 4, H // 4, DEV)
        served = ops.dw_inorm_route(0, probe, dw.weight.data, probe) == 1
        assert served == (N <= 64)
        want = eng.infer_launches(N, H, H)
        # declined: block 0's PLAIN dw_inorm takes 2 launches, the other five 3 (the InstanceNorm that makes u first)
        assert want == 4 * 2 + 14 + (0 if served else 1 + 2 + 2 + 2)
        xin = eng.infer_input(N, H, H)
        ops.nchw_to_nhwc(x.contiguous().to(DEV), xin, cfill=8)
        ops.lib().gcc_launch_count(1)
        y = eng.infer(xin)
        assert ops.lib().gcc_launch_count(0) == want
        got = ops.nhwc_to_nchw(y, 3).cpu()
        ref = _forward(eng, x)
        mx, mean = _err(got, ref)
        assert mx <= 4e-2 and mean <= 4e-3, (N, mx, mean)
    assert ops.lib().gcc_device_error(0) == 0


# ---- 2. against the reference's images --------------------------------------------------------------------------------
def _cycle_model(extra=(), **kw):
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    opt = options.parse(['--dataroot', './database/horse2zebra/', '--model', 'cyclegan', '--gpu_ids', '0', '--ngf', '8',
                         '--ndf', '8'] + list(extra))
    opt.isTrain = True
    return get_model_class(opt)(opt, **kw), opt


def test_cyclegan_infer_matches_reference_checkpoint(golden_dir):
    z = np.load(os.path.join(golden_dir, 'ref_checkpoint_cyclegan.npz'))
    model, _ = _cycle_model(['--darts_discriminator'])
    model.load_models(os.path.join(golden_dir, 'ref_checkpoint_cyclegan.pth'), load_discriminator=False)
    A, B = torch.from_numpy(z['A']), torch.from_numpy(z['B'])
    for gen, src, key in (('A', A, 'fake_B'), ('B', B, 'fake_A')):
        ref = torch.from_numpy(z[key])
        got = model.infer(src.to(DEV), gen).cpu()
        mx, mean = _err(got, ref)
        old = _forward(model.G[gen], _rb(src))
        _, old_mean = _err(old, ref)
        print('%s: max %.4g mean %.4g (forward mean %.4g)' % (key, mx, mean, old_mean))
        assert mx <= 4e-2 and mean <= 6.25e-3, (key, mx, mean)
        assert mean <= 1.05 * old_mean + 1e-6, (key, mean, old_mean)
    # the dict form picks each generator's own domain
    got = model.infer({'A': A, 'B': B, 'A_paths': ['a'], 'B_paths': ['b']}, 'B').cpu()
    assert torch.equal(got, model.infer(B.to(DEV), 'B').cpu())


def test_pix2pix_resnet_infer_matches_reference(golden_dir):
    from tests.test_pix2pix_gpu import _build_resnet_gcc, load
    z = load(golden_dir, 'pix2pix_resnet_gcc.npz')
    model, _, _ = _build_resnet_gcc(z)
    data = {'A': torch.from_numpy(z['A']), 'B': torch.from_numpy(z['B']), 'A_paths': ['a'], 'B_paths': ['b']}
    ref = torch.from_numpy(z['eval.fake_B'])
    got = model.infer(data).cpu()
    mx, mean = _err(got, ref)
    model.model_eval()
    model.set_input(data)
    model.forward()
    _, old_mean = _err(model.fake_B.cpu(), ref)
    print('pix2pix resnet: max %.4g mean %.4g (forward mean %.4g)' % (mx, mean, old_mean))
    assert mx <= 4e-2 and mean <= 6.25e-3
    assert mean <= 1.05 * old_mean + 1e-6


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_pruned_resnet_infer_matches_reference(golden_dir, tag):
    from tests.test_pix2pix_gpu import load, load_recipe
    from gcc_amd.options import options
    from gcc_amd.models import get_model_class
    z = load(golden_dir, 'prune_resnet.npz')
    cfg = [int(v) for v in z['pruned_%s.cfg' % tag]]
    opt = options.parse(['--dataroot', './database/cityscapes/', '--model', 'pix2pix', '--gpu_ids', '0', '--backbone', 'resnet',
                         '--ngf', '8', '--ndf', '8'])
    opt.isTrain = True
    model = get_model_class(opt)(opt, filter_cfgs=cfg)
    load_recipe(model.netG, 711)
    load_recipe(model.netD, 712)
    model.refresh_weights()
    data = {'A': torch.from_numpy(z['A']), 'B': torch.from_numpy(z['B']), 'A_paths': ['a'], 'B_paths': ['b']}
    ref = torch.from_numpy(z['pruned_%s.eval.fake_B' % tag])
    mx, mean = _err(model.infer(data), ref)
    model.model_eval()
    model.set_input(data)
    model.forward()
    _, old_mean = _err(model.fake_B.cpu(), ref)
    print('pruned %s: max %.4g mean %.4g (forward mean %.4g)' % (tag, mx, mean, old_mean))
    assert mx <= 4e-2 and mean <= 6.25e-3
    assert mean <= 1.05 * old_mean + 1e-6


# ---- 3. against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ngf,N', [(24, 1), (24, 4), (64, 1), (64, 4)])
def test_infer_against_oracle(ngf, N):
    net, eng = _resnet_engine(ngf, 400 + ngf)
    g = torch.Generator().manual_seed(ngf + N)
    x = _rb(torch.rand(N, 3, 256, 256, generator=g) * 2 - 1)
    sd = OrderedDict((k, v.detach().float().cpu()) for k, v in net.state_dict().items())
    O.EMULATE_BF16 = True
    try:
        ref16 = O.mobile_resnet_forward(sd, x).detach()
    finally:
        O.EMULATE_BF16 = False
    ref32 = O.mobile_resnet_forward(sd, x).detach()
    got = _infer(eng, x)
    mx, mean = _err(got, ref16)
    fmx, fmean = _err(ref16, ref32)
    print('ngf %d N %d: vs bf16-emulating oracle max %.4g mean %.4g (oracle bf16 vs fp32: %.4g %.4g)' % (ngf, N, mx, mean, fmx, fmean))
    # the emulating oracle's own distance from fp32 sets the scale: the fused path stores fewer intermediates
    assert mean <= max(2 * fmean, 2e-3) and mx <= max(2 * fmx, 3e-2), (mx, mean, fmx, fmean)


# ---- 4. launches ------------------------------------------------------------------------------------------------------
def test_infer_launch_count():
    ops = _ops()
    net, eng = _resnet_engine(24, 77)
    B = len(eng.blocks)
    x = _rb(torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(1)) * 2 - 1)
    want = eng.infer_launches(1, 256, 256)
    _infer(eng, x)
    xin = eng.infer_input(1, 256, 256)
    ops.nchw_to_nhwc(x.contiguous().to(DEV), xin, cfill=8)
    ops.lib().gcc_launch_count(1)
    eng.infer(xin)
    got = ops.lib().gcc_launch_count(0)
    _forward(eng, x)
    c = eng._ctx(1, 256, 256, 'main')
    ops.lib().gcc_launch_count(1)
    eng.forward(c, train=False)
    old = ops.lib().gcc_launch_count(0)
    print('infer %d launches, eval forward() %d' % (got, old))
    assert got == want <= 4 * B + 16 and got < old
    # counting another geometry writes nothing: the image infer() returned stays valid
    xin = eng.infer_input(1, 256, 256)
    ops.nchw_to_nhwc(x.contiguous().to(DEV), xin, cfill=8)
    img = eng.infer(xin)
    keep = img.float().cpu()
    assert eng.infer_launches(2, 64, 128) > 0
    torch.cuda.synchronize()
    assert torch.equal(img.float().cpu(), keep)


# ---- 5. memory and isolation ------------------------------------------------------------------------------------------
def test_infer_memory_flat_and_ctx_untouched():
    net, eng = _resnet_engine(16, 91, n_blocks=3)
    g = torch.Generator().manual_seed(2)
    shapes = [(2, 64, 64), (1, 32, 48), (1, 64, 64), (3, 16, 32), (2, 48, 48), (1, 128, 64), (2, 64, 32), (1, 8, 8)]
    _infer(eng, _rb(torch.rand(2, 3, 128, 64, generator=g) * 2 - 1))    # the largest geometry first
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    for N, H, W in shapes:
        x = _rb(torch.rand(N, 3, H, W, generator=g) * 2 - 1)
        got = _infer(eng, x)
        ref = _forward(eng, x)
        mx, _ = _err(got, ref)
        # a 2 x 2 trunk plane (8 x 8 input) normalises over four pixels: the two routes' roundings differ more there
        assert mx <= (4e-2 if H * W >= 256 else 1e-1), (N, H, W, mx)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() <= mem + sum(                      # forward()'s own contexts are the growth
            t.numel() * t.element_size() for c in eng.ctx.values() for t in vars(c).values() if torch.is_tensor(t)) + (64 << 20)
    eng.ctx.clear()
    mem2 = [None]
    for N, H, W in shapes:
        _infer(eng, _rb(torch.rand(N, 3, H, W, generator=g) * 2 - 1))
        torch.cuda.synchronize()
        if mem2[0] is None:
            mem2[0] = torch.cuda.memory_allocated()
        assert torch.cuda.memory_allocated() == mem2[0], (N, H, W)
    assert set(eng.ctx) == set(), 'infer() made a training context'
    from gcc_amd import _lib
    with pytest.raises(_lib.GccError):
        eng.infer(eng.infer_input(1, 30, 32))


def test_infer_between_cyclegan_steps_changes_nothing():
    """infer of both generators between two training iterations: losses and weights bit-identical; host RNG untouched"""
    import random

    def run(with_infer):
        torch.manual_seed(0)
        random.seed(0)
        model, _ = _cycle_model(['--crop_size', '64', '--load_size', '64'])
        from tests.golden.recipe import recipe_state_dict
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
        rng = (random.getstate(), torch.get_rng_state())
        if with_infer:
            a = model.infer(data[1]['A'].to(DEV), 'A')
            b = model.infer(data[1]['B'].to(DEV), 'B')
            assert torch.isfinite(a).all() and torch.isfinite(b).all()
            assert random.getstate() == rng[0] and torch.equal(torch.get_rng_state(), rng[1])
        model.set_input(data[1])
        model.optimize_parameters()
        losses.append(model.get_current_losses())
        w = [p.detach().clone() for n in (model.netG_A, model.netG_B) for p in n.parameters()]
        return losses, w
    l0, w0 = run(False)
    l1, w1 = run(True)
    assert l0 == l1
    assert all(torch.equal(a, b) for a, b in zip(w0, w1))


def test_eval_forward_unchanged_by_infer():
    net, eng = _resnet_engine(16, 93, n_blocks=3)
    x = _rb(torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(8)) * 2 - 1)
    before = _forward(eng, x)
    _infer(eng, x)
    assert torch.equal(_forward(eng, x), before)


# ---- 6. the CLI -------------------------------------------------------------------------------------------------------
def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_cli_cyclegan_end_to_end(tmp_path):
    from PIL import Image
    from gcc_amd import test as gtest
    root = tmp_path / 'data'
    (root / 'testA').mkdir(parents=True)
    (root / 'testB').mkdir(parents=True)
    rng = np.random.RandomState(0)
    for n in ('h1', 'h2'):
        _png(str(root / 'testA' / (n + '.jpg')), rng.randint(0, 256, (256, 256, 3), dtype=np.uint8))
    for n in ('z1', 'z2'):
        _png(str(root / 'testB' / (n + '.jpg')), rng.randint(0, 256, (256, 256, 3), dtype=np.uint8))
    argv = ['--dataroot', str(root), '--model', 'cyclegan', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--name', 'exp',
            '--checkpoints_dir', str(tmp_path / 'ck')]
    from gcc_amd.options import options
    opt = options.parse(argv)
    opt.isTrain = True
    from gcc_amd.models import get_model_class
    model = get_model_class(opt)(opt)
    model.save_models(2, str(tmp_path / 'save'))
    ckpt = str(tmp_path / 'save' / 'model_2.pth')
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-m', 'gcc_amd.test'] + argv + ['--pretrain_path', ckpt], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / 'ck' / 'exp' / 'test_results'
    files = sorted(str(p.relative_to(out)) for p in out.rglob('*.png'))
    assert any(f.startswith('fake_B') for f in files), files
    from gcc_amd.data import create_dataset
    model.model_eval()
    n = 0
    for data in create_dataset(gtest.test_overrides(opt), model.device):
        model.set_input(data)
        fake = model.infer_nhwc(model.real_A, 'A')
        ref = _ops().image_to_u8(fake)[0].cpu().numpy()
        name = gtest.result_names(['fake_B'], model.image_paths, opt.direction)[0][1]
        assert np.array_equal(np.asarray(Image.open(str(out / name))), ref), name
        n += 1
    assert n >= 2
