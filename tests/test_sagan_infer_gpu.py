"""The SAGAN generator's fused eval-mode path (SaganGeneratorEngine.infer, SAGANModel.infer): gcc_attention_infer on each
route against fp32 torch, gcc_spectral_eval_coeffs_group against the grouped power iteration, the reference's images, the
oracle, the state an inference call moves and leaves alone, launches, memory, and python -m gcc_amd.test."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_pix2pix_gpu import DEV, _rel, load, load_recipe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from gcc_amd import ops
    return ops


def _rb(t):
    return t.bfloat16().float()


def _to_nhwc(x, buf=None):
    ops = _ops()
    if buf is None:
        buf = ops.new_act(x.shape[0], x.shape[1], x.shape[2], x.shape[3], DEV)
    ops.nchw_to_nhwc(x.to(DEV, torch.float32).contiguous(), buf)
    return buf


def _err(got, ref):
    e = (got.float() - ref.float()).abs()
    return float(e.max()), float(e.mean())


def _launches(fn):
    lib = _ops().lib()
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    fn()
    torch.cuda.synchronize()
    return lib.gcc_launch_count(0)


# ---- 1. gcc_attention_infer against fp32 torch ---------------------------------------------------------------------------
def _attn_case(B, C, C8, H, gamma, seed, crafted=False):
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    N = H * H
    q, k = _rb(torch.randn(B, C8, H, H, generator=g)), _rb(torch.randn(B, C8, H, H, generator=g))
    if crafted:
        # every row's maximum first appears in the last 32-key block, > 30 above everything before it
        q = torch.ones(B, C8, H, H)
        k = _rb(torch.rand(B, C8, H, H, generator=g) * 0.5 / C8)
        kf = k.reshape(B, C8, N)
        kf[:, :, (N - 1) // 32 * 32:] += 40.0 / C8
        k = _rb(kf.reshape(B, C8, H, H))
    v, x = _rb(torch.randn(B, C, H, H, generator=g)), _rb(torch.randn(B, C, H, H, generator=g))
    attn = torch.softmax(torch.bmm(q.reshape(B, C8, N).permute(0, 2, 1), k.reshape(B, C8, N)), dim=-1)
    o = torch.bmm(v.reshape(B, C, N), attn.permute(0, 2, 1)).reshape(B, C, H, H)
    y_ref = gamma * o + x
    c8p = ops.ceil8(C8)
    offs = (0, c8p, 2 * c8p)
    qkv = ops.new_act(B, 2 * c8p + C, H, H, DEV)
    for t, off in ((q, 0), (k, c8p), (v, 2 * c8p)):
        ops.nhwc_copy(_to_nhwc(t), 0, qkv, off, t.shape[1])
    # x and y as channel slices of wider buffers; y's pad channels start as garbage
    xw = ops.new_act(B, ops.ceil8(C) + 16, H, H, DEV)
    x_d = ops.cslice(xw, 8, C)
    ops.nhwc_copy(_to_nhwc(x), 0, xw, 8, C)
    yw = ops.new_act(B, ops.ceil8(C) + 24, H, H, DEV)
    yw.fill_(7.0)
    y_d = ops.cslice(yw, 16, C)
    return dict(qkv=qkv, offs=offs, x=x_d, x_ref=x, y=y_d, yw=yw, y_ref=y_ref, gamma=torch.tensor([gamma], device=DEV))


def _run_attn(case, C, C8, split):
    ops = _ops()
    return ops.attention_infer(case['qkv'], case['offs'], case['x'], case['gamma'], C, C8, case['y'], split=split)


@pytest.mark.parametrize('B,C,C8,H', [(1, 16, 2, 16), (1, 8, 1, 32), (3, 96, 12, 16), (1, 48, 6, 32), (1, 128, 16, 16),
                                      (64, 64, 8, 32), (2, 24, 2, 9), (1, 96, 40, 7), (3, 512, 64, 8), (1, 64, 16, 32),
                                      (64, 128, 16, 16)])
@pytest.mark.parametrize('gamma', [0.7, -0.45])
def test_attention_infer_against_fp32(B, C, C8, H, gamma):
    ops = _ops()
    lib = ops.lib()
    case = _attn_case(B, C, C8, H, gamma, seed=B * 1000 + C + H)
    N = H * H
    seen = set()
    for split in (False, True):
        route = ops.attention_infer(case['qkv'], case['offs'], case['x'], case['gamma'], C, C8, case['y'], split=split,
                                    route_only=True)
        case['yw'].fill_(7.0)
        n = _launches(lambda: _run_attn(case, C, C8, split))
        assert n == route, (split, n, route)
        seen.add(route)
        got = ops.nhwc_to_nchw(case['y'], C).cpu()
        r = _rel(got, case['y_ref'])
        assert r <= 5e-3, (split, r)
        # channels C .. ceil8(C) - 1 of y are zeros; the channels around the slice are untouched
        full = case['yw'].permute(0, 2, 3, 1).reshape(B * N, -1)
        assert torch.equal(full[:, 16 + C:16 + ops.ceil8(C)].float().cpu(), torch.zeros(B * N, ops.ceil8(C) - C))
        assert bool((full[:, :16] == 7.0).all()) and bool((full[:, 16 + ops.ceil8(C):] == 7.0).all())
    if lib.gcc_attention_infer_workspace(B, N, C, C8) > 0:
        assert seen == {1, 2}


@pytest.mark.parametrize('B,C,C8,H', [(1, 64, 8, 32), (1, 16, 2, 16), (2, 48, 6, 9)])
def test_attention_infer_gamma_zero_is_x(B, C, C8, H):
    ops = _ops()
    case = _attn_case(B, C, C8, H, 0.0, seed=7)
    for split in (False, True):
        _run_attn(case, C, C8, split)
        torch.cuda.synchronize()
        assert torch.equal(ops.nhwc_to_nchw(case['y'], C).cpu(), case['x_ref'])


@pytest.mark.parametrize('B,C,C8,H', [(1, 64, 8, 32), (1, 16, 2, 16), (2, 96, 12, 16), (1, 40, 5, 7)])
def test_attention_infer_late_row_maximum(B, C, C8, H):
    """crafted scores: the row maximum first appears in the last key block, far above the earlier scores"""
    ops = _ops()
    case = _attn_case(B, C, C8, H, 0.8, seed=11, crafted=True)
    for split in (False, True):
        _run_attn(case, C, C8, split)
        torch.cuda.synchronize()
        r = _rel(ops.nhwc_to_nchw(case['y'], C).cpu(), case['y_ref'])
        assert r <= 5e-3, (split, r)


def test_attention_infer_refuses_bad_arguments_before_launching():
    ops = _ops()
    lib = ops.lib()
    case = _attn_case(1, 64, 8, 8, 0.5, seed=3)
    qp, ld = case['qkv'].data_ptr(), 2 * 8 + 64
    xp, yp, gp = case['x'].data_ptr(), case['y'].data_ptr(), case['gamma'].data_ptr()
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    lib.gcc_launch_count(1)
    bad = [
        ((qp, ld, 0, 8, 16, xp, 84, gp, 1, 64, 64, 8, yp, 96, None, 0, None), -1),       # ldx not a multiple of 8
        ((qp, ld + 4, 0, 8, 16, xp, 88, gp, 1, 64, 64, 8, yp, 96, None, 0, None), -1),   # ldq not a multiple of 8
        ((qp, ld, 0, 12, 16, xp, 88, gp, 1, 64, 64, 8, yp, 96, None, 0, None), -1),      # koff
        ((qp, ld, 0, 8, 16, xp, 88, gp, 1, 64, 64, 8, yp, 60, None, 0, None), -1),       # ldy
        ((qp, 64, 0, 8, 16, xp, 88, gp, 1, 64, 64, 8, yp, 96, None, 0, None), -1),       # ldq below voff + C
        ((None, ld, 0, 8, 16, xp, 88, gp, 1, 64, 64, 8, yp, 96, None, 0, None), -1),
        ((qp, ld, 0, 8, 16, xp, 88, None, 1, 64, 64, 8, yp, 96, None, 0, None), -1),
        ((qp, ld, 0, 8, 16, xp, 88, gp, 1, 1025, 64, 8, yp, 96, None, 0, None), -2),     # N > 1024
        ((qp, ld, 0, 8, 16, xp, 88, gp, 1, 64, 64, 0, yp, 96, None, 0, None), -2),       # C8 = 0
        ((qp, ld, 0, 8, 16, xp, 88, gp, 1, 64, 64, 65, yp, 96, None, 0, None), -2),      # C8 > 64
        ((qp, ld, 0, 8, 16, xp, 88, gp, 0, 64, 64, 8, yp, 96, None, 0, None), -2),       # B = 0
        ((qp, ld, 0, 8, 16, xp, 88, gp, 1, 64, 64, 8, yp, 96, ws.data_ptr() + 4, 1024, None), -1),  # misaligned workspace
    ]
    for args, want in bad:
        assert lib.gcc_attention_infer(*args) == want, args
    torch.cuda.synchronize()
    assert lib.gcc_launch_count(0) == 0


# ---- 2. gcc_spectral_eval_coeffs_group ---------------------------------------------------------------------------------------
def _gen_widths(ngf, cfg=None):
    return [int(v) for v in cfg] if cfg is not None else [ngf * 8, ngf * 4, ngf * 2, ngf]


@pytest.mark.parametrize('ngf,cfg', [(8, None), (48, None), (64, None), (64, [200, 96, 40, 24])])
def test_spectral_eval_coeffs_against_grouped_iteration(ngf, cfg):
    ops = _ops()
    g = torch.Generator().manual_seed(ngf)
    w = _gen_widths(ngf, cfg)
    cin = [128] + w[:3]
    layers = []
    for R, Cc in zip(cin, w):
        wb = (torch.randn(R, Cc, 4, 4, generator=g) * 0.05).to(DEV).contiguous(memory_format=torch.channels_last)
        u = torch.randn(R, generator=g)
        v = torch.randn(Cc * 16, generator=g)
        bn = torch.nn.BatchNorm2d(Cc).to(DEV)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(Cc, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(Cc, generator=g) * 0.1)
            bn.running_mean.copy_(torch.randn(Cc, generator=g) * 0.2)
            bn.running_var.copy_(torch.rand(Cc, generator=g) + 0.3)
        layers.append((wb, (u / u.norm()).to(DEV), (v / v.norm()).to(DEV), bn, (torch.randn(Cc, generator=g) * 0.1).to(DEV)))
    uA = [l[1].clone() for l in layers]
    vA = [l[2].clone() for l in layers]
    uB = [l[1].clone() for l in layers]
    vB = [l[2].clone() for l in layers]
    tA = [torch.zeros(l[0].shape[0], device=DEV) for l in layers]
    tB = [torch.zeros(l[0].shape[0], device=DEV) for l in layers]
    sA, sB = torch.zeros(4, device=DEV), torch.zeros(4, device=DEV)
    pw = [torch.zeros((ops.ceil8(l[0].shape[0]), 16, ops.ceil8(l[0].shape[1])), dtype=torch.bfloat16, device=DEV) for l in layers]
    pwt = [torch.zeros((ops.ceil8(l[0].shape[1]), 16, ops.ceil8(l[0].shape[0])), dtype=torch.bfloat16, device=DEV) for l in layers]
    scale = [torch.zeros(l[0].shape[1], device=DEV) for l in layers]
    shift = [torch.zeros(l[0].shape[1], device=DEV) for l in layers]
    items = ops.spectral_eval_items([(l[0], uB[i], vB[i], tB[i], sB[i:i + 1], l[3], l[4], scale[i], shift[i])
                                     for i, l in enumerate(layers)])
    for rep in range(2):          # the second round starts from the moved u, v
        ops.spectral_power_iteration_pack_group([(l[0], uA[i], vA[i], tA[i], sA[i:i + 1], pw[i], pwt[i])
                                                 for i, l in enumerate(layers)])
        n = _launches(lambda: ops.spectral_eval_coeffs_group(items, DEV))
        assert n == 3
        for i in range(4):
            assert torch.equal(uA[i], uB[i]) and torch.equal(vA[i], vB[i]), (rep, i)
            assert torch.equal(tA[i], tB[i]), (rep, i)
        assert torch.equal(sA, sB), rep
        for i, (wb, _, _, bn, bias) in enumerate(layers):
            sig = float(sB[i])
            rstd = 1.0 / torch.sqrt(bn.running_var.double().cpu() + bn.eps)
            gm = bn.weight.detach().double().cpu() * rstd
            want_scale = gm / sig
            want_shift = bn.bias.detach().double().cpu() + (bias.double().cpu() - bn.running_mean.double().cpu()) * gm
            assert torch.allclose(scale[i].double().cpu(), want_scale, rtol=4e-7 * 8, atol=0), (rep, i)
            assert torch.allclose(shift[i].double().cpu(), want_shift, rtol=4e-7 * 8, atol=1e-7 * float(want_shift.abs().max())), (rep, i)


# ---- models ------------------------------------------------------------------------------------------------------------------
def _model(ngf=8, cfg=None, seed=801, gammas=(0.6, -0.4)):
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    opt = options.parse(['--dataroot', './database/celeb/', '--model', 'sagan', '--gpu_ids', '0', '--ngf', str(ngf),
                         '--ndf', '8'])
    opt.isTrain = True
    model = get_model_class(opt)(opt, filter_cfgs=cfg)
    if seed is not None:
        load_recipe(model.netG, seed)
        load_recipe(model.netD, seed + 1)
    with torch.no_grad():
        if gammas is not None:
            model.netG.attn1.gamma.fill_(gammas[0])
            model.netG.attn2.gamma.fill_(gammas[1])
    model.refresh_weights()
    return model, opt


def _eval_forward(model, z):
    """fake_img of an eval-mode forward() (the training route), restoring the model's mode"""
    was = model.netG.training
    model.model_eval()
    N = z.shape[0]
    model.set_input({'z': z, 'real_img': torch.zeros(N, 3, 64, 64), 'img_path': ['p'] * N})
    with torch.no_grad():
        model.forward()
    out = model.fake_img.clone()
    if was:
        model.model_train()
    return out


def _uv(model):
    return {k: v.detach().clone() for k, v in model.netG.state_dict().items() if k.endswith('_u') or k.endswith('_v')}


def _sd(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


# ---- 3. the reference's images ---------------------------------------------------------------------------------------------
def test_infer_matches_reference_checkpoint(golden_dir):
    z = np.load(os.path.join(golden_dir, 'ref_checkpoint_sagan.npz'))
    model, _ = _model(seed=None, gammas=None)
    model.load_models(os.path.join(golden_dir, 'ref_checkpoint_sagan.pth'), load_discriminator=False)
    assert float(model.netG.attn1.gamma.detach()) != 0.0 or float(model.netG.attn2.gamma.detach()) != 0.0
    assert model.G.attn[0].C8 == 2 and model.G.attn[1].C8 == 1
    sd0 = _sd(model.netG)
    ref = torch.from_numpy(z['fake_img'])
    got = model.infer(torch.from_numpy(z['z'])).cpu()
    after = _uv(model)
    model.netG.load_state_dict(sd0)
    old = _eval_forward(model, torch.from_numpy(z['z'])).cpu()
    assert all(torch.equal(after[k], v) for k, v in _uv(model).items())
    mx, mean = _err(got, ref)
    _, old_mean = _err(old, ref)
    print('ref checkpoint: max %.4g mean %.4g (forward mean %.4g)' % (mx, mean, old_mean))
    assert mx <= 2e-2 and mean <= 3e-3, (mx, mean)
    assert mean <= 1.05 * old_mean + 1e-6, (mean, old_mean)


def test_infer_matches_gcc_golden_eval_image(golden_dir):
    z = load(golden_dir, 'sagan_gcc.npz')
    model, _ = _model(gammas=None)
    sd0 = _sd(model.netG)
    ref = torch.from_numpy(z['eval.fake_img'])
    got = model.infer(torch.from_numpy(z['eval.z'])).cpu()
    model.netG.load_state_dict(sd0)
    old = _eval_forward(model, torch.from_numpy(z['eval.z'])).cpu()
    mx, mean = _err(got, ref)
    _, old_mean = _err(old, ref)
    print('sagan_gcc eval: max %.4g mean %.4g (forward mean %.4g)' % (mx, mean, old_mean))
    assert mx <= 2e-2 and mean <= 3e-3, (mx, mean)
    assert mean <= 1.05 * old_mean + 1e-6, (mean, old_mean)


# ---- 4. the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ngf,cfg,N', [(64, None, 1), (64, None, 8), (64, [200, 96, 40, 24], 4)])
def test_infer_against_oracle(ngf, cfg, N):
    from oracle import gcc_oracle as O
    model, _ = _model(ngf, cfg, seed=905, gammas=(0.5, -0.7))
    sd = {k: v.detach().double().cpu().clone() for k, v in model.netG.state_dict().items()}
    z = torch.randn(N, 128, generator=torch.Generator().manual_seed(N))
    got = model.infer(z).cpu()
    ref = O.sagan_generator_forward(sd, z.double(), train=False).float()
    mx, mean = _err(got, ref)
    print('ngf %d cfg %s N %d: max %.4g mean %.4g' % (ngf, cfg, N, mx, mean))
    assert mx <= 2e-2 and mean <= 3e-3, (mx, mean)
    for k, v in _uv(model).items():       # the oracle's power iteration moved its u, v the same way
        assert torch.allclose(v.double().cpu(), sd[k], atol=1e-5), k


# ---- 5. state -----------------------------------------------------------------------------------------------------------------
def _ctx_checksum(model):
    out = []
    for c in model.G.ctx.values():
        for t in [c.z, c.out] + c.raw + c.act + [s.w for s in c.sn] + [s.wt for s in c.sn] + [s.sigma for s in c.sn] + \
                [s.t for s in c.sn] + [a.qkv for a in c.attn] + [a.o for a in c.attn] + [a.y for a in c.attn] + \
                [a.stats for a in c.attn] + [b.scale for b in c.bn if getattr(b, 'scale', None) is not None]:
            out.append(t.detach().float().sum().item())
            out.append(t.detach().float().abs().sum().item())
    return out


def test_infer_moves_uv_like_eval_forward_and_nothing_else():
    model, _ = _model()
    zs = [torch.randn(4, 128, generator=torch.Generator().manual_seed(i)) for i in range(3)]
    model.model_train()
    model.set_input({'z': zs[0], 'real_img': torch.zeros(4, 3, 64, 64), 'img_path': ['p'] * 4})
    model.forward()                             # a training context exists
    sd0 = _sd(model.netG)
    ck0 = _ctx_checksum(model)
    for z in zs:
        model.infer(z)
    torch.cuda.synchronize()
    uv_infer = _uv(model)
    sd1 = _sd(model.netG)
    assert _ctx_checksum(model) == ck0
    for k, v in sd1.items():
        if not (k.endswith('_u') or k.endswith('_v')):
            assert torch.equal(v, sd0[k]), k            # running statistics and parameters unchanged
    assert model.netG.training                          # the mode is left alone
    model.netG.load_state_dict(sd0)
    for z in zs:
        _eval_forward(model, z)
    for k, v in _uv(model).items():
        assert torch.equal(v, uv_infer[k]), k
        assert not torch.equal(v, sd0[k]), k


def _step(model, seed):
    g = torch.Generator().manual_seed(seed)
    model.set_input({'z': torch.randn(4, 128, generator=g), 'real_img': torch.rand(4, 3, 64, 64, generator=g) * 2 - 1,
                     'img_path': ['p'] * 4})
    model.optimize_parameters()


def test_infer_between_steps_equals_eval_forward_between_steps():
    zs = [torch.randn(2, 128, generator=torch.Generator().manual_seed(50 + i)) for i in range(2)]
    runs = []
    for use_infer in (True, False):
        model, _ = _model()
        model.model_train()
        _step(model, 1)
        for z in zs:
            if use_infer:
                model.infer(z)
            else:
                _eval_forward(model, z)
        _step(model, 2)
        torch.cuda.synchronize()
        runs.append((_sd(model.netG), _sd(model.netD)))
    for a, b in zip(runs[0], runs[1]):
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ---- 6. launches and memory ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ngf', [48, 64])
def test_infer_launches_and_memory(ngf):
    ops = _ops()
    model, _ = _model(ngf)
    lib = ops.lib()
    for N in (1, 8, 64):
        z = torch.randn(N, 128, generator=torch.Generator().manual_seed(N)).to(DEV)
        zin = model.G.infer_input(N)
        ops.nchw_to_nhwc(z.reshape(N, 128, 1, 1).contiguous(), zin)
        want = model.G.infer_launches(N)          # the first call after a repack also rebuilds the packings
        got = _launches(lambda: model.G.infer(zin))
        assert got == want, (N, got, want)
        want = model.G.infer_launches(N)
        got = _launches(lambda: model.G.infer(zin))
        assert got == want, (N, got, want)
        c = model.G._ctx(N)
        ops.nchw_to_nhwc(z.reshape(N, 128, 1, 1).contiguous(), c.z)
        fwd = _launches(lambda: model.G.forward(c, train=False))
        print('ngf %d N %d: infer %d launches, eval forward %d' % (ngf, N, got, fwd))
        assert got < fwd, (N, got, fwd)
    # infer_launches writes nothing: the last image stays valid
    z8 = torch.randn(8, 128, generator=torch.Generator().manual_seed(3)).to(DEV)
    out = model.infer_nhwc(z8)
    keep = out.clone()
    lib.gcc_launch_count(1)
    for N in (1, 8, 64):
        model.G.infer_launches(N)
    torch.cuda.synchronize()
    assert lib.gcc_launch_count(0) == 0
    assert torch.equal(out, keep)
    # flat memory over repeated calls and smaller batches
    model.infer_nhwc(torch.randn(64, 128).to(DEV))
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    for N in (64, 1, 8, 3, 64, 1):
        model.infer_nhwc(torch.randn(N, 128).to(DEV))
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == mem, N


def test_infer_sees_weight_changes(tmp_path):
    ops = _ops()
    model, _ = _model()
    model.model_train()
    z = torch.randn(2, 128, generator=torch.Generator().manual_seed(9))
    sd0 = _sd(model.netG)
    a = model.infer(z).cpu()
    # an Adam step: the next infer follows the new weights (matches eval forward on them)
    _step(model, 3)
    sd1 = _sd(model.netG)
    b = model.infer(z).cpu()
    model.netG.load_state_dict(sd1)
    ref = _eval_forward(model, z).cpu()
    assert (b - ref).abs().max() <= 3e-2 and not torch.equal(a, b)
    # load_models
    model.netG.load_state_dict(sd0)
    model.save_models(1, str(tmp_path))
    _step(model, 4)
    model.load_models(os.path.join(str(tmp_path), 'model_1.pth'), load_discriminator=False)
    c = model.infer(z).cpu()
    model.netG.load_state_dict(sd0)
    model.refresh_weights()
    assert torch.equal(c, model.infer(z).cpu())


# ---- 7. python -m gcc_amd.test --model sagan -----------------------------------------------------------------------------
def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_cli_run_writes_infer_bytes(tmp_path, monkeypatch):
    from PIL import Image
    from gcc_amd import data as gdata
    from gcc_amd import test as gtest
    model, opt = _model()
    opt.checkpoints_dir, opt.name = str(tmp_path / 'ck'), 'exp'
    model.save_models(3, str(tmp_path / 'save'))
    ckpt = str(tmp_path / 'save' / 'model_3.pth')
    g = torch.Generator().manual_seed(21)
    batches = [{'z': torch.randn(1, 128, generator=g), 'real_img': torch.rand(1, 3, 64, 64, generator=g) * 2 - 1,
                'img_path': ['/x/img%d.png' % i]} for i in range(3)]
    monkeypatch.setattr(gdata, 'create_dataset', lambda o, device=None: iter(batches))
    m1, _ = _model(seed=None, gammas=None)
    m1.load_models(ckpt, load_discriminator=False)
    out = gtest.run(opt, m1)
    m2, _ = _model(seed=None, gammas=None)
    m2.load_models(ckpt, load_discriminator=False)
    m3, _ = _model(seed=None, gammas=None)
    m3.load_models(ckpt, load_discriminator=False)
    ops = _ops()
    for data in batches:
        names = dict(gtest.result_names(['fake_img', 'real_img'], [data['img_path'], data['img_path']], opt.direction))
        got = np.asarray(Image.open(os.path.join(out, names['fake_img'])))
        want = ops.image_to_u8(m2.infer_nhwc(data['z']))[0].cpu().numpy()
        assert np.array_equal(got, want), names['fake_img']
        fwd = gtest.tensor2im_host(_eval_forward(m3, data['z']).cpu())
        assert np.abs(got.astype(int) - fwd.astype(int)).max() <= 3
        assert os.path.exists(os.path.join(out, names['real_img']))


def test_cli_sagan_end_to_end(tmp_path):
    root = tmp_path / 'data'
    (root / 'train').mkdir(parents=True)
    rng = np.random.RandomState(0)
    for n in ('a1', 'a2'):
        _png(str(root / 'train' / (n + '.jpg')), rng.randint(0, 256, (170, 180, 3), dtype=np.uint8))
    argv = ['--dataroot', str(root), '--model', 'sagan', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--name', 'exp',
            '--checkpoints_dir', str(tmp_path / 'ck')]
    model, _ = _model()
    model.save_models(2, str(tmp_path / 'save'))
    ckpt = str(tmp_path / 'save' / 'model_2.pth')
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-m', 'gcc_amd.test'] + argv + ['--pretrain_path', ckpt], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / 'ck' / 'exp' / 'test_results'
    files = sorted(str(p.relative_to(out)) for p in out.rglob('*.png'))
    assert files == ['a1.png', 'a2.png', 'fake_img/a1_fake_img.png', 'fake_img/a2_fake_img.png'], files
