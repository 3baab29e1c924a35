"""U-Net inference path: the eval-mode epilogue of gcc_conv_eval_ex (forward and transposed, second output, split-K) against
fp32 PyTorch, the fused generator (UnetEngine.infer / Pix2PixModel.infer) against the reference's images and the oracle, its
launch count, memory and isolation from training, gcc_image_to_u8 against numpy, and `python -m gcc_amd.test` end to end."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gcc_oracle as O
from tests.golden.recipe import recipe_state_dict

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rb(t):
    return t.bfloat16().float()


def _opt(extra=(), ngf=8, num_downs=8):
    from gcc_amd.options import options
    opt = options.parse(['--dataroot', './database/cityscapes/', '--model', 'pix2pix', '--gpu_ids', '0', '--ngf', str(ngf),
                         '--ndf', '8', '--num_downs', str(num_downs), '--load_size', '256', '--crop_size', '256'] + list(extra))
    opt.isTrain = True
    return opt


def _model(opt, f=None, c=None):
    from gcc_amd.models import get_model_class
    return get_model_class(opt)(opt, filter_cfgs=f, channel_cfgs=c)


def _load(model, sd):
    model.netG.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    model.refresh_weights()


def _randomize_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.netG.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_((torch.randn(m.num_features, generator=g) * 0.2).to(DEV))
            m.running_var.copy_((torch.rand(m.num_features, generator=g) * 1.5 + 0.5).to(DEV))
            m.weight.data.copy_((torch.rand(m.num_features, generator=g) + 0.5).to(DEV))
            m.bias.data.copy_((torch.randn(m.num_features, generator=g) * 0.1).to(DEV))
    model.refresh_weights()


def _eval_forward(model, A):
    model.model_eval()
    model.set_input({'A': A, 'B': A.clone(), 'A_paths': ['a'], 'B_paths': ['b']})
    model.forward()
    return model.fake_B.cpu()


def _err(a, b):
    e = (a.float().cpu() - b.float().cpu()).abs()
    return float(e.max()), float(e.mean())


# ---- 1. the epilogue on each route ---------------------------------------------------------------------------------------
def _act(z, act, _lib, slope=0.2):
    if act == _lib.EVAL_ACT_RELU:
        return F.relu(z)
    if act == _lib.EVAL_ACT_LRELU:
        return F.leaky_relu(z, slope)
    if act == _lib.EVAL_ACT_TANH:
        return torch.tanh(z)
    return z


CASES = [  # (transposed, N, H_in, W_in, Ci, Co): H_in / W_in of the conv's INPUT
    (False, 1, 256, 256, 3, 64), (False, 1, 16, 16, 64, 128), (False, 3, 8, 8, 13, 512), (False, 1, 2, 2, 512, 512),
    (False, 3, 32, 32, 512, 13), (True, 1, 1, 1, 512, 512), (True, 3, 4, 4, 512, 13), (True, 1, 64, 64, 64, 3),
    (True, 3, 8, 8, 13, 64), (True, 1, 32, 32, 128, 64), (True, 1, 64, 64, 128, 64),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'T' if c is True else ('F' if c is False else str(c)))
def test_eval_ex_epilogue_against_fp32(case):
    from gcc_amd import _lib, ops
    L = ops.lib()
    tr, N, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(H * 7 + Ci + Co)
    x = _rb(torch.randn(N, Ci, H, W, generator=g))
    if not tr:
        w = _rb(torch.randn(Co, Ci, 4, 4, generator=g) / (4 * Ci ** 0.5))
        acc = F.conv2d(x, w, stride=2, padding=1)
        wp, _ = ops.pack_weights(w.to(DEV).contiguous(memory_format=torch.channels_last))
    else:
        w = _rb(torch.randn(Ci, Co, 4, 4, generator=g) / (2 * Ci ** 0.5))          # ConvTranspose2d weight [in, out, k, k]
        acc = F.conv_transpose2d(x, w, stride=2, padding=1)
        _, wp = ops.pack_weights(w.to(DEV).contiguous(memory_format=torch.channels_last))
    Ho, Wo = acc.shape[2:]
    scale = torch.rand(Co, generator=g) * 1.5 + 0.25
    shift = torch.randn(Co, generator=g) * 0.3
    xd = ops.new_act(N, Ci, H, W, DEV)
    ops.nchw_to_nhwc(x.to(DEV).contiguous(), xd)
    C8 = ops.ceil8(Co)
    ld = 2 * C8 + 16                                          # y at [8, 8 + C8), y2 at [C8 + 16, 2 C8 + 16) of a wider buffer
    sd_, hd = scale.to(DEV), shift.to(DEV)
    d = ops.conv_desc(N, Ho, Wo, Co, Ci, 4, 2, 1, ld, ops.ceil8(Ci)) if tr else ops.conv_desc(N, H, W, Ci, Co, 4, 2, 1, ops.ceil8(Ci), ld)
    need = L.gcc_conv_eval_ex_workspace(ctypes.byref(d), int(tr))
    z = scale.view(1, -1, 1, 1) * acc + shift.view(1, -1, 1, 1)
    routes = set()
    for ws_bytes in ([0, need] if need else [0]):
        assert L.gcc_conv_eval_ex_route(ctypes.byref(d), int(tr), ws_bytes) == (5 if ws_bytes else 0)
        routes.add(ws_bytes > 0)
        for act, act2 in ((_lib.EVAL_ACT_LRELU, _lib.EVAL_ACT_RELU), (_lib.EVAL_ACT_RELU, None), (_lib.EVAL_ACT_TANH, None),
                          (_lib.EVAL_ACT_NONE, _lib.EVAL_ACT_TANH)):
            buf = torch.full((N, Ho, Wo, ld), 3.0, dtype=torch.bfloat16, device=DEV)
            y = buf.permute(0, 3, 1, 2)[:, 8:8 + Co]
            y2 = buf.permute(0, 3, 1, 2)[:, C8 + 16:C8 + 16 + Co] if act2 is not None else None
            ws = torch.zeros(max(ws_bytes, 1), dtype=torch.uint8, device=DEV)
            ep = _lib.eval_ex_epilogue_t(sd_.data_ptr(), hd.data_ptr(), y2.data_ptr() if y2 is not None else None, ld if y2 is not None else 0,
                                         0, act, act2 if act2 is not None else 0, 0.2, 0, ws.data_ptr() if ws_bytes else None, ws_bytes)
            rc = L.gcc_conv_eval_ex(ctypes.byref(d), int(tr), xd.data_ptr(), wp.data_ptr(), y.data_ptr(), ctypes.byref(ep), None)
            assert rc == 0
            torch.cuda.synchronize()
            outs = [(y, act)] + ([(y2, act2)] if y2 is not None else [])
            for t, a in outs:
                ref = _act(z, a, _lib)
                got = t.float().cpu()
                e = (got - ref).abs()
                tol = 1e-2 * ref.abs().max().clamp(min=1.0)
                assert float(e.max()) <= float(tol) + 2 ** -7 * float(ref.abs().max()), (case, a, float(e.max()))
            full = buf.float().cpu()
            assert (full[..., 8 + Co:8 + C8] == 0).all() and (full[..., C8 + 16 + Co:2 * C8 + 16] == 0).all() if y2 is not None else \
                (full[..., 8 + Co:8 + C8] == 0).all()
            assert (full[..., :8] == 3.0).all()                # outside the windows nothing is written
    if need:
        assert routes == {False, True}


def test_eval_ex_rejects_bad_arguments():
    from gcc_amd import _lib, ops
    L = ops.lib()
    x = ops.new_act(1, 16, 8, 8, DEV)
    y = torch.zeros((1, 4, 4, 64), dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(32 * 16 * 16, dtype=torch.bfloat16, device=DEV)
    d = ops.conv_desc(1, 8, 8, 16, 16, 4, 2, 1, 16, 64)
    mk = lambda **kw: _lib.eval_ex_epilogue_t(*[kw.get(k, v) for k, v in (('scale', None), ('shift', None), ('y2', None),
                                              ('ldy2', 0), ('y2off', 0), ('act', 0), ('act2', 0), ('slope', 0.2), ('pad_', 0),
                                              ('workspace', None), ('workspace_bytes', 0))])
    call = lambda ep: L.gcc_conv_eval_ex(ctypes.byref(d), 0, x.data_ptr(), w.data_ptr(), y.data_ptr(), ctypes.byref(ep), None)
    L.gcc_launch_count(1)
    yp = y.data_ptr()
    for ep in (mk(act=7), mk(act=_lib.EVAL_ACT_PRELU), mk(y2=yp + 64, ldy2=60), mk(y2=yp + 64, ldy2=64, y2off=4),
               mk(y2=yp + 16, ldy2=64), mk(y2=yp, ldy2=64), mk(y2=yp + 32, ldy2=64, act2=9)):
        assert call(ep) == -1
    assert L.gcc_launch_count(0) == 0
    assert call(mk(y2=yp + 32, ldy2=64, act=_lib.EVAL_ACT_LRELU, act2=_lib.EVAL_ACT_RELU)) == 0
    # gcc_conv_fprop_eval keeps rejecting the new acts
    ev = _lib.eval_epilogue_t(None, None, None, None, 0, 0, _lib.EVAL_ACT_RELU, 0, None, 0)
    d3 = ops.conv_desc(1, 8, 8, 16, 16, 3, 1, 1, 16, 16)
    assert L.gcc_conv_fprop_eval(ctypes.byref(d3), x.data_ptr(), w.data_ptr(), y.data_ptr(), ctypes.byref(ev), None) == -1


def test_eval_ex_route_only_says_when_the_library_declines():
    """ops.conv_eval_ex(route_only=True): -1 for a geometry gcc_conv_eval_ex_route declines, nothing launched.  (conv_eval_ex has
    one k for both directions, so the declined geometries it can state are these: a kernel larger than the padded map, and a
    transposed conv whose kernel is smaller than its stride.)"""
    from gcc_amd import ops
    L = ops.lib()
    w = torch.zeros(16 * 9 * 16, dtype=torch.bfloat16, device=DEV)
    x2, x8, y4, y16 = (ops.new_act(1, 16, s, s, DEV) for s in (2, 8, 4, 16))
    d = ops.conv_desc(1, 2, 2, 16, 16, 3, 1, 0, 16, 16)                      # 3 x 3, no padding, on 2 x 2: no output pixel
    assert L.gcc_conv_eval_ex_route(ctypes.byref(d), 0, 0) < 0
    dt = ops.conv_desc(1, 16, 16, 16, 16, 1, 2, 0, 16, 16)                   # transposed 1 x 1 of stride 2: holes in the output
    assert L.gcc_conv_eval_ex_route(ctypes.byref(dt), 1, 0) < 0
    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    assert ops.conv_eval_ex(x2, w, 16, 3, 1, 0, x2, route_only=True) == -1
    assert ops.conv_eval_ex(x8, w, 16, 1, 2, 0, y16, transposed=True, route_only=True) == -1
    assert ops.conv_eval_ex(x8, w, 16, 4, 2, 1, y4, route_only=True) in (1, 2)          # and an accepted one keeps its count
    assert L.gcc_launch_count(0) == 0


# ---- 2. against the reference's images -------------------------------------------------------------------------------
def test_infer_matches_reference_eval_image(golden_dir):
    z = np.load(os.path.join(golden_dir, 'pix2pix_eval_d8.npz'))
    model = _model(_opt(ngf=8))
    _load(model, recipe_state_dict(O.unet_shapes(8, 8), int(z['seed_G'])))
    A, B = torch.from_numpy(z['A']), torch.from_numpy(z['B'])
    real_A = A if str(z['direction']) == 'AtoB' else B
    ref = torch.from_numpy(z['fake_B'])
    fused = model.infer(real_A.to(DEV)).cpu()
    mx, mean = _err(fused, ref)
    assert mx <= 2e-2 and mean <= 3e-3, (mx, mean)
    _, old_mean = _err(_eval_forward(model, real_A), ref)
    assert mean <= 1.05 * old_mean + 1e-6, (mean, old_mean)


def test_infer_matches_reference_checkpoint(golden_dir):
    from tests.test_checkpoint_gpu import ARGV
    from gcc_amd.options import options
    from gcc_amd.models import get_model_class
    z = np.load(os.path.join(golden_dir, 'ref_checkpoint_pix2pix.npz'))
    opt = options.parse(ARGV)
    opt.isTrain = True
    model = get_model_class(opt)(opt)
    model.load_models(os.path.join(golden_dir, 'ref_checkpoint_pix2pix.pth'))
    A = torch.from_numpy(z['A'])
    mx, mean = _err(model.infer(A.to(DEV)), torch.from_numpy(z['fake_B']))
    assert mx <= 2e-2 and mean <= 3e-3, (mx, mean)


# ---- 3. against the fp32 oracle ---------------------------------------------------------------------------------------
def _oracle_case(model, N, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.rand(N, 3, 256, 256, generator=g) * 2 - 1
    sd = {k: v.detach().float().cpu() for k, v in model.netG.state_dict().items()}
    return A, sd


@pytest.mark.parametrize('N', [1, 4])
def test_infer_full_width_against_oracle(N):
    model = _model(_opt(ngf=64))
    _randomize_bn(model, 11)
    A, sd = _oracle_case(model, N, 5 + N)
    with torch.no_grad():
        ref = O.unet_forward(sd, A, 8, train=False)
    mx, mean = _err(model.infer(A.to(DEV)), ref)
    assert mx <= 3e-2 and mean <= 4e-3, (mx, mean)


def test_infer_pruned_against_oracle(golden_dir):
    z = np.load(os.path.join(golden_dir, 'pix2pix_pruned_d8.npz'))
    f, c = [int(v) for v in z['f']], [int(v) for v in z['c']]
    assert any(v % 8 for v in f)
    model = _model(_opt(['--no_dropout']), f, c)
    _randomize_bn(model, 3)
    A, sd = _oracle_case(model, 2, 9)
    with torch.no_grad():
        ref = O.unet_forward(sd, A, 8, train=False)
    mx, mean = _err(model.infer(A.to(DEV)), ref)
    assert mx <= 3e-2 and mean <= 4e-3, (mx, mean)


@pytest.mark.parametrize('tag', ['k7', 'k6', 'k5'])
def test_infer_removed_block_students(golden_dir, tag):
    """students whose inner blocks were removed (D = 7, 6, 5; the last block wraps Identity, irregular widths): the fused
    image against the reference's eval image (stored at every second pixel), no less accurate than today's eval forward()"""
    from collections import OrderedDict
    z = np.load(os.path.join(golden_dir, 'pix2pix_pruned_removed_d8.npz'))
    f, c = [int(v) for v in z[tag + '.f']], [int(v) for v in z[tag + '.c']]
    model = _model(_opt(['--no_dropout'], ngf=32), f, c)
    assert model.G.D == {'k7': 7, 'k6': 6, 'k5': 5}[tag] and model.G.inner_identity
    i = ('k7', 'k6', 'k5').index(tag)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in model.netG.state_dict().items())
    _load(model, recipe_state_dict(shapes, 411 + 2 * i))
    A, B = torch.from_numpy(z['A']), torch.from_numpy(z['B'])
    real_A = A if str(z['direction']) == 'AtoB' else B
    ref = torch.from_numpy(z[tag + '.eval.fake_B'])
    mx, mean = _err(model.infer(real_A.to(DEV)).cpu()[:, :, ::2, ::2], ref)
    assert mx <= 2e-2 and mean <= 3e-3, (mx, mean)
    _, old_mean = _err(_eval_forward(model, real_A)[:, :, ::2, ::2], ref)
    assert mean <= 1.05 * old_mean + 1e-6, (mean, old_mean)


# ---- 4. launches, 5. memory and isolation --------------------------------------------------------------------------------
def test_infer_launch_count():
    from gcc_amd import ops
    L = ops.lib()
    model = _model(_opt(ngf=64))
    _randomize_bn(model, 1)
    G = model.G
    L.gcc_launch_count(1)
    G.eval_coeffs()
    assert L.gcc_launch_count(1) == 1
    x = G.infer_input(1, 256, 256)
    x.normal_()
    predicted = G.infer_launches(1, 256, 256)
    G.infer(x)
    torch.cuda.synchronize()
    n = L.gcc_launch_count(1)
    assert n == predicted <= 32, (n, predicted)
    A = torch.rand(1, 3, 256, 256) * 2 - 1
    model.model_eval()
    model.set_input({'A': A, 'B': A.clone(), 'A_paths': ['a'], 'B_paths': ['b']})
    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    model.forward()
    torch.cuda.synchronize()
    old = L.gcc_launch_count(1)
    assert n < old, (n, old)


def test_infer_memory_flat_and_ctx_untouched():
    model = _model(_opt(ngf=16))
    G = model.G
    A = torch.rand(2, 3, 512, 512) * 2 - 1
    model.infer(A.to(DEV))
    ctx_keys = list(G.ctx.keys())
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    for N, H, W in ((1, 256, 256), (2, 256, 512), (1, 512, 256), (2, 512, 512), (1, 1024, 256), (1, 256, 1024),
                    (2, 256, 256), (1, 512, 512)):
        model.infer((torch.rand(N, 3, H, W) * 2 - 1).to(DEV))
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - m0 <= 1 << 20
    assert list(G.ctx.keys()) == ctx_keys


def _train_two(model, data, between=None):
    model.model_train()
    losses = []
    for i in range(2):
        model.set_input(data[i])
        model.optimize_parameters()
        losses.append(model.get_current_losses())
        if between is not None and i == 0:
            between()
    torch.cuda.synchronize()
    return losses, {k: v.detach().cpu().clone() for k, v in model.netG.state_dict().items()}


def test_infer_between_training_steps_changes_nothing():
    g = torch.Generator().manual_seed(2)
    data = [{'A': torch.rand(1, 3, 256, 256, generator=g) * 2 - 1, 'B': torch.rand(1, 3, 256, 256, generator=g) * 2 - 1,
             'A_paths': ['a'], 'B_paths': ['b']} for _ in range(2)]
    torch.manual_seed(0)
    a = _model(_opt())
    sd = {k: v.detach().clone() for k, v in a.netG.state_dict().items()}
    sdD = {k: v.detach().clone() for k, v in a.netD.state_dict().items()}
    la, wa = _train_two(a, data)
    b = _model(_opt())
    b.netG.load_state_dict(sd)
    b.netD.load_state_dict(sdD)
    b.refresh_weights()
    seed = [None]

    def between():
        seed[0] = b.G.seed
        b.infer(data[0]['A'].to(DEV))
        assert b.G.seed == seed[0]
    lb, wb = _train_two(b, data, between)
    assert la == lb
    for k in wa:
        assert torch.equal(wa[k], wb[k]), k


def test_eval_forward_unchanged_by_infer():
    model = _model(_opt())
    _randomize_bn(model, 8)
    A = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(1)) * 2 - 1
    before = _eval_forward(model, A)
    model.infer(A.to(DEV))
    model.infer((torch.rand(2, 3, 256, 512) * 2 - 1).to(DEV))
    assert torch.equal(before, _eval_forward(model, A))


# ---- 6. gcc_image_to_u8 -------------------------------------------------------------------------------------------------
def test_image_to_u8_bit_exact():
    from gcc_amd import ops
    vals = torch.tensor([-1.0, 1.0, 0.0, -0.5, 0.5, 0.99609375, -0.99609375], dtype=torch.float32)
    # values just below integer boundaries of ((x + 1) / 2) * 255
    k = torch.arange(1, 255, dtype=torch.float32)
    near = (k / 255.0) * 2 - 1
    extra = torch.cat([near, torch.nextafter(near, torch.tensor(-2.0)), torch.rand(4000) * 2 - 1])
    x = torch.cat([vals, extra]).bfloat16().float()
    n = (x.numel() + 2) // 3 * 3
    x = torch.cat([x, torch.zeros(n - x.numel())]).view(1, 3, 1, n // 3)
    xd = ops.new_act(1, 3, 1, n // 3, DEV)
    ops.nchw_to_nhwc(x.to(DEV).contiguous(), xd)
    got = ops.image_to_u8(xd).cpu().numpy()[0]
    a = np.transpose(x[0].numpy(), (1, 2, 0))
    ref = ((a + np.float32(1)) / np.float32(2.0) * np.float32(255.0)).astype(np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, ref)


# ---- 7. the test CLI ------------------------------------------------------------------------------------------------------
def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_cli_pix2pix_end_to_end(tmp_path):
    from PIL import Image
    from gcc_amd import test as gtest
    root = tmp_path / 'data'
    (root / 'val').mkdir(parents=True)
    rng = np.random.RandomState(0)
    names = ['frankfurt_1', 'lindau_22']
    for n in names:
        _png(str(root / 'val' / (n + '.jpg')), rng.randint(0, 256, (256, 512, 3), dtype=np.uint8))
    argv = ['--dataroot', str(root), '--model', 'pix2pix', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--name', 'exp',
            '--checkpoints_dir', str(tmp_path / 'ck')]
    from gcc_amd.options import options
    opt = options.parse(argv)
    opt.isTrain = True
    model = _model(opt)
    _randomize_bn(model, 5)
    model.save_models(3, str(tmp_path / 'save'))
    ckpt = str(tmp_path / 'save' / 'model_3.pth')
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-m', 'gcc_amd.test'] + argv + ['--pretrain_path', ckpt], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / 'ck' / 'exp' / 'test_results'
    files = sorted(str(p.relative_to(out)) for p in out.rglob('*.png'))
    want = sorted([n + '.png' for n in names] + [os.path.join('fake_B', n + '_fake_B.png') for n in names])
    assert files == want
    # every fake equals tensor2im of model.infer on the loader's input
    from gcc_amd.data import create_dataset
    model.model_eval()
    for data in create_dataset(gtest.test_overrides(opt), model.device):
        model.set_input(data)
        fake = model.infer(model.real_A)
        ref = gtest.tensor2im_host(fake)
        name = gtest.result_names(['fake_B'], model.image_paths, opt.direction)[0][1]
        assert np.array_equal(np.asarray(Image.open(str(out / name))), ref), name
