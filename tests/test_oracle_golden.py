"""Pins oracle/gcc_oracle.py against golden vectors produced by the real reference
(tests/golden/make_fixtures.py).  CPU only."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import gcc_oracle as O
from tests.golden.recipe import recipe_state_dict, recipe_transform, sample_idx

torch.set_num_threads(8)


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def as_dtype(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def sd_from(z, prefix):
    sd = OrderedDict()
    for k in z.files:
        if k.startswith(prefix):
            v = torch.from_numpy(np.array(z[k]))
            sd[k[len(prefix):]] = v
    return sd


def test_eval_generated_images(golden_dir):
    z = load(golden_dir, 'pix2pix_eval_d8.npz')
    G = recipe_state_dict(O.unet_shapes(8, 8), int(z['seed_G']))
    A, B = torch.from_numpy(z['A']), torch.from_numpy(z['B'])
    real_A = A if str(z['direction']) == 'AtoB' else B
    with torch.no_grad():
        out = O.unet_forward(G, real_A, num_downs=8, train=False)
    ref = torch.from_numpy(z['fake_B'])
    assert out.shape == ref.shape
    assert (out - ref).abs().max().item() < 2e-5


def test_state_dict_key_parity(golden_dir):
    z = load(golden_dir, 'ops.npz')
    assert list(O.unet_shapes(4, 6).keys()) == [str(k) for k in z['init.G_keys']]
    assert list(O.patchgan_shapes(4, 6, False).keys()) == [str(k) for k in z['init.D_keys']]
    g = load(golden_dir, 'pix2pix_gcc_d6.npz')
    masked_keys = [k[len('final.sD.'):] for k in g.files if k.startswith('final.sD.')]
    assert list(O.patchgan_shapes(8, 6, True).keys()) == masked_keys
    shp = O.unet_shapes(16, 6)
    for k in [k[len('final.tG.'):] for k in g.files if k.startswith('final.tG.')]:
        n = 1
        for d in shp[k]:
            n *= d
        assert g['final.tG.' + k].size == min(n, 2048), k


def test_gate_fwd_bwd(golden_dir):
    z = load(golden_dir, 'ops.npz')
    x = torch.from_numpy(z['gate.x']).requires_grad_(True)
    a = torch.from_numpy(z['gate.alpha']).requires_grad_(True)
    y = O.gate(x, a, 0.5)
    y.backward(torch.from_numpy(z['gate.dy']))
    assert np.array_equal(O.gate_mask(a.detach(), 0.5).numpy(), z['gate.mask'])
    np.testing.assert_allclose(y.detach().numpy(), z['gate.y'], rtol=0, atol=0)
    np.testing.assert_allclose(x.grad.numpy(), z['gate.dx'], rtol=0, atol=0)
    np.testing.assert_allclose(a.grad.numpy(), z['gate.dalpha'], rtol=1e-6, atol=1e-6)


def test_gan_losses_and_gram(golden_dir):
    z = load(golden_dir, 'ops.npz')
    pred = torch.from_numpy(z['gan.pred'])
    n = 0
    for k in z.files:
        if k.startswith('gan.') and k.count('.') == 3 and not k.endswith('.grad'):
            _, mode, real, ford = k.split('.')
            p = pred.clone().requires_grad_(True)
            l = O.gan_loss(mode, p, bool(int(real)), bool(int(ford)))
            l.backward()
            assert abs(float(l.detach()) - float(z[k])) < 1e-6, k
            np.testing.assert_allclose(p.grad.numpy(), z[k + '.grad'], atol=1e-7)
            n += 1
    assert n == 15
    np.testing.assert_allclose(O.gram(torch.from_numpy(z['gram.x'])).numpy(), z['gram.y'], atol=1e-6)


def test_lr_schedule(golden_dir):
    z = load(golden_dir, 'pix2pix_pretrain_d6.npz')
    ec, ne, nd, lr = z['sched']
    want = z['lr_after_epoch']
    got = [lr * O.lr_lambda_linear(e, int(ec), int(ne), int(nd)) for e in range(1, len(want) + 1)]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)


def test_init_statistics(golden_dir):
    z = load(golden_dir, 'ops.npz')
    sd = O.init_state_dict(O.unet_shapes(4, 6), torch.Generator().manual_seed(3))
    w = torch.cat([v.flatten() for k, v in sd.items() if v.dim() == 4])
    bw = torch.cat([v.flatten() for k, v in sd.items() if k.endswith('.weight') and v.dim() == 1])
    bb = torch.cat([v.flatten() for k, v in sd.items() if k.endswith('.bias') and v.dim() == 1 and
                    not k.startswith('model.model.3')])
    ref = z['init.stats']
    assert abs(float(w.mean()) - ref[0]) < 2e-3 and abs(float(w.std()) - ref[1]) < 2e-3
    assert abs(float(bw.mean()) - ref[2]) < 1e-2 and abs(float(bw.std()) - ref[3]) < 1e-2
    assert abs(float(bb.mean()) - ref[4]) < 0.3 and abs(float(bb.std()) - ref[5]) < 0.3
    assert float(sd['model.model.3.bias'].abs().max()) == 0.0


def _compare_sd(got, z, prefix, atol, rtol=1e-4, skip=None, outliers=0.0, hard=0.0):
    """outliers: admissible fraction of elements above the tolerance, each still within ``hard``"""
    worst = 0.0
    for k in z.files:
        if not k.startswith(prefix):
            continue
        name = k[len(prefix):]
        if skip is not None and skip(name.split('@')[0]):
            continue
        ref = z[k]
        g = got[name].detach().reshape(-1)
        g = g[sample_idx(g.numel())].numpy()
        if ref.dtype.kind in 'iu':
            assert int(g[0]) == int(ref.reshape(-1)[0]), name
            continue
        d = np.abs(g - ref)
        err = d.max()
        tol = atol + rtol * np.abs(ref).max()
        if outliers > 0.0:
            assert (d > tol).sum() <= max(1, int(outliers * d.size)) and err <= hard, (name, err, tol, int((d > tol).sum()))
        else:
            assert err <= tol, (name, err, tol)
        worst = max(worst, err)
    return worst


def test_pretrain_two_iterations(golden_dir):
    z = load(golden_dir, 'pix2pix_pretrain_d6.npz')
    opt = O.Opt(ngf=8, ndf=8, num_downs=6, no_dropout=True, lambda_scale=1e-2, darts_discriminator=False,
                online_distillation=False, direction=str(z['direction']))
    sG, sD = [int(v) for v in z['seeds']]
    m = O.Pix2PixOracle(opt, recipe_state_dict(O.unet_shapes(8, 6), sG),
                        recipe_state_dict(O.patchgan_shapes(8, 6, False), sD), masked=False)
    for it in range(2):
        m.set_input(torch.from_numpy(z['it%d.A' % it]), torch.from_numpy(z['it%d.B' % it]))
        m.optimize_parameters()
        for k in ('G_GAN', 'G_L1', 'D_real', 'D_fake'):
            assert abs(m.losses[k] - float(z['it%d.loss.%s' % (it, k)])) < 1e-4 * max(1, abs(m.losses[k])), (it, k)
    _compare_sd(m.G, z, 'final.G.', atol=2e-5)
    _compare_sd(m.D, z, 'final.D.', atol=2e-5)


def build_gcc_oracle(z):
    """student+teacher oracle with the recipe weights the fixture was generated from"""
    opt = O.Opt(ngf=8, ndf=8, teacher_ngf=16, teacher_ndf=16, num_downs=6, no_dropout=True,
                direction=str(z['direction']), threshold=float(z['threshold']))
    s_sG, s_sD, s_tG, s_tD, s_T = [int(v) for v in z['seeds']]
    teacher = O.Pix2PixOracle(opt, recipe_state_dict(O.unet_shapes(16, 6), s_tG),
                              recipe_state_dict(O.patchgan_shapes(16, 6, False), s_tD), masked=False)
    sD = recipe_state_dict(O.patchgan_shapes(8, 6, True), s_sD)
    for k in z.files:
        if k.startswith('init.sD.'):
            sD[k[len('init.sD.'):]] = torch.from_numpy(np.array(z[k]))
    sw, tw = [16, 64, 128, 32], [32, 128, 256, 64]
    T = [recipe_transform(t, s, s_T + i) for i, (s, t) in enumerate(zip(sw, tw))]
    m = O.Pix2PixOracle(opt, recipe_state_dict(O.unet_shapes(8, 6), s_sG), sD, T, masked=True, teacher=teacher)
    return m, teacher, opt


def test_gcc_two_iterations(golden_dir):
    z = load(golden_dir, 'pix2pix_gcc_d6.npz')
    m, teacher, opt = build_gcc_oracle(z)
    for it in range(2):
        m.set_input(torch.from_numpy(z['it%d.A' % it]), torch.from_numpy(z['it%d.B' % it]))
        m.optimize_parameters()
        if it == 0:
            np.testing.assert_allclose(m.fake_B.numpy(), z['it0.fake_B'], atol=2e-5)
            np.testing.assert_allclose(teacher.fake_B.numpy(), z['it0.Tfake_B'], atol=2e-5)
            for j in range(6):
                ref = z['it0.target.%d' % j]
                np.testing.assert_allclose(m.targets[j].numpy(), ref, atol=2e-5 + 1e-4 * np.abs(ref).max())
            for j in range(4):
                ref = z['it0.sfeat.%d' % j]
                np.testing.assert_allclose(list(m.g_feats.values())[j].detach().numpy(), ref,
                                           atol=2e-5 + 1e-4 * np.abs(ref).max())
            for j in range(2):
                ref = z['it0.tDfeat_on_sfake.%d' % j]
                np.testing.assert_allclose(m.dist_feats[4 + j].numpy(), ref, atol=2e-5 + 1e-4 * np.abs(ref).max())
            _compare_sd(m.G, z, 'it0.afterstep.sG.', atol=2e-5)
            _compare_sd(m.D, z, 'it0.afterstep.sD.', atol=2e-5)
        m.set_input(torch.from_numpy(z['it%d.vA' % it]), torch.from_numpy(z['it%d.vB' % it]))
        m.clipping_mask_alpha()
        m.optimizer_netD_arch()
        for k in z.files:
            if k.startswith('it%d.loss.' % it):
                name = k.split('.')[-1]
                ref = float(z[k])
                assert abs(m.losses[name] - ref) <= 2e-4 * max(1.0, abs(ref)), (it, name, m.losses[name], ref)
            if k.startswith('it%d.tloss.' % it):
                name = k.split('.')[-1]
                ref = float(z[k])
                assert abs(teacher.losses[name] - ref) <= 2e-4 * max(1.0, abs(ref)), (it, name)
    _compare_sd(m.G, z, 'final.sG.', atol=3e-5)
    _compare_sd(m.D, z, 'final.sD.', atol=3e-5)
    _compare_sd(teacher.G, z, 'final.tG.', atol=3e-5)
    _compare_sd(teacher.D, z, 'final.tD.', atol=3e-5)
    for i in range(4):
        np.testing.assert_allclose(m.T[i].detach().numpy(), z['final.T.%d' % i], atol=3e-5)


def test_prune_cfgs_bit_exact(golden_dir):
    z = load(golden_dir, 'prune_d8.npz')
    G = recipe_state_dict(O.unet_shapes(8, 8), int(z['seed_G']))
    gsp = torch.Generator().manual_seed(302)
    # same BN-scale spread the fixture script applied, in the reference's modules() order
    for name in O._unet_bn_names(8):
        G[name + '.weight'] = 1.0 + 0.02 * torch.randn(G[name + '.weight'].shape, generator=gsp)
    mx, mn = O.max_min_bn_scale(G)
    assert [mx, mn] == [float(v) for v in z['bn.max_min']]
    for i, t in enumerate(z['bn.thresholds']):
        f, c = O.scale_prune_cfg(G, float(t), ngf=8)
        assert f == [int(v) for v in z['bn.f.%d' % i]], (i, t)
        assert c == [int(v) for v in z['bn.c.%d' % i]], (i, t)
    mx, mn = O.max_min_conv_norm(G)
    assert [mx, mn] == [float(v) for v in z['norm.max_min']]
    for i, t in enumerate(z['norm.thresholds']):
        f, c = O.norm_prune_cfg(G, float(t), ngf=8)
        assert f == [int(v) for v in z['norm.f.%d' % i]], (i, t)
        assert c == [int(v) for v in z['norm.c.%d' % i]], (i, t)


def test_pruned_student_irregular_widths(golden_dir):
    """generator built from filter_cfgs / channel_cfgs (widths such as 6, 21, 31, 29): eval image and one
    training iteration against the reference"""
    z = load(golden_dir, 'pix2pix_pruned_d8.npz')
    f, c = [int(v) for v in z['f']], [int(v) for v in z['c']]
    sG, sD = [int(v) for v in z['seeds']]
    G = recipe_state_dict(O.unet_shapes_cfg(f, c), sG)
    D = recipe_state_dict(O.patchgan_shapes(8, 6, False), sD)
    A, B = torch.from_numpy(z['A']), torch.from_numpy(z['B'])
    real_A = A if str(z['direction']) == 'AtoB' else B
    with torch.no_grad():
        out = O.unet_forward(G, real_A, 8, train=False)
    np.testing.assert_allclose(out.numpy(), z['eval.fake_B'], atol=2e-5)
    opt = O.Opt(ngf=8, ndf=8, num_downs=8, no_dropout=True, darts_discriminator=False, online_distillation=False,
                direction=str(z['direction']))
    m = O.Pix2PixOracle(opt, G, D, masked=False)
    m.set_input(A, B)
    m.optimize_parameters()
    np.testing.assert_allclose(m.fake_B.numpy(), z['train.fake_B'], atol=2e-5)
    for k in ('G_GAN', 'G_L1', 'D_real', 'D_fake'):
        assert abs(m.losses[k] - float(z['loss.' + k])) < 1e-4 * max(1, abs(m.losses[k]))
    _compare_sd(m.G, z, 'final.G.', atol=2e-5)


@pytest.mark.parametrize('tag', ['k7', 'k6', 'k5'])
def test_pruned_student_removed_blocks(golden_dir, tag):
    """students that lost inner blocks (filter_cfgs with zeros; models/Pix2Pix.py:87, 97 and the Identity submodule :59-67):
    k7 = the innermost block gone (block 6 wraps Identity), k6 = 6 and 7 gone, k5 = 5, 6 and 7 gone.  state_dict keys, eval
    image and one training iteration against the reference"""
    z = load(golden_dir, 'pix2pix_pruned_removed_d8.npz')
    f, c = [int(v) for v in z[tag + '.f']], [int(v) for v in z[tag + '.c']]
    assert f[7] == 0 and f[8] == 0
    i = ('k7', 'k6', 'k5').index(tag)
    shapes = O.unet_shapes_cfg(f, c)
    assert list(shapes.keys()) == [str(k) for k in z[tag + '.keys']]
    G = recipe_state_dict(shapes, 411 + 2 * i)
    D = recipe_state_dict(O.patchgan_shapes(8, 6, False), 412 + 2 * i)
    A, B = torch.from_numpy(z['A']), torch.from_numpy(z['B'])
    with torch.no_grad():
        out = O.unet_forward(G, A if str(z['direction']) == 'AtoB' else B, 8, train=False)
    np.testing.assert_allclose(out.numpy()[:, :, ::2, ::2], z[tag + '.eval.fake_B'], atol=2e-5)
    opt = O.Opt(ngf=32, ndf=8, num_downs=8, no_dropout=True, darts_discriminator=False, online_distillation=False,
                direction=str(z['direction']))
    m = O.Pix2PixOracle(opt, G, D, masked=False)
    m.set_input(A, B)
    m.optimize_parameters()
    np.testing.assert_allclose(m.fake_B.numpy()[:, :, ::2, ::2], z[tag + '.train.fake_B'], atol=2e-5)
    for k in ('G_GAN', 'G_L1', 'D_real', 'D_fake'):
        assert abs(m.losses[k] - float(z[tag + '.loss.' + k])) < 1e-4 * max(1, abs(m.losses[k]))
    # (one sampled element of one deep conv has |gradient| ~ Adam's eps: its first-step update is not +-lr and flips with the
    # summation order -- admitted as an outlier within 2 lr)
    _compare_sd(m.G, z, tag + '.final.G.', atol=2e-5, outliers=0.001, hard=4.1e-4)


def build_removed_gcc_oracle(z):
    """the 6-block student (blocks 6 and 7 pruned away) under distillation from an ngf-48 teacher, recipe weights of
    pix2pix_pruned_removed_d8.npz"""
    f, c = [int(v) for v in z['k6.f']], [int(v) for v in z['k6.c']]
    opt = O.Opt(ngf=32, ndf=8, teacher_ngf=48, teacher_ndf=8, num_downs=8, no_dropout=True, direction=str(z['direction']))
    teacher = O.Pix2PixOracle(opt, recipe_state_dict(O.unet_shapes(48, 8), 423), recipe_state_dict(O.patchgan_shapes(8, 6, False), 424),
                              masked=False)
    sw, tw = [c[1], c[3], c[-4], c[-2]], [96, 384, 768, 192]
    T = [recipe_transform(t, s_, 425 + i) for i, (s_, t) in enumerate(zip(sw, tw))]
    m = O.Pix2PixOracle(opt, recipe_state_dict(O.unet_shapes_cfg(f, c), 421), recipe_state_dict(O.patchgan_shapes(8, 6, True), 422),
                        T, masked=True, teacher=teacher)
    return m, teacher, opt


def test_pruned_student_removed_blocks_gcc_iteration(golden_dir):
    """... and one full GCC iteration of it (teacher step, distillation through the four hooked tensors -- the deepest pair now
    sits directly above the last block -- and the arch step)"""
    z = load(golden_dir, 'pix2pix_pruned_removed_d8.npz')
    m, teacher, opt = build_removed_gcc_oracle(z)
    m.set_input(torch.from_numpy(z['A']), torch.from_numpy(z['B']))
    m.optimize_parameters()
    np.testing.assert_allclose(m.fake_B.numpy()[:, :, ::2, ::2], z['gcc.fake_B'], atol=2e-5)
    for j in range(4):
        t = list(m.g_feats.values())[j]
        assert list(t.shape) == [int(v) for v in z['gcc.sfeat_shape.%d' % j]]
        t = t.detach().reshape(-1)
        ref = z['gcc.sfeat.%d' % j]
        np.testing.assert_allclose(t[sample_idx(t.numel(), 8192)].numpy(), ref, atol=2e-5 + 1e-4 * np.abs(ref).max())
    m.set_input(torch.from_numpy(z['vA']), torch.from_numpy(z['vB']))
    m.clipping_mask_alpha()
    m.optimizer_netD_arch()
    for k in z.files:
        if k.startswith('gcc.loss.'):
            name, ref = k.split('.')[-1], float(z[k])
            assert abs(m.losses[name] - ref) <= 2e-4 * max(1.0, abs(ref)), (name, m.losses[name], ref)
    _compare_sd(m.G, z, 'gcc.final.sG.', atol=3e-5, outliers=0.001, hard=4.1e-4)
    for i in range(4):
        t = m.T[i].detach().reshape(-1)
        np.testing.assert_allclose(t[sample_idx(t.numel())].numpy(), z['gcc.final.T.%d' % i], atol=3e-5)


def build_resnet_gcc_oracle(z):
    """--backbone resnet student (ngf 8) + teacher (ngf 16) with the recipe weights of pix2pix_resnet_gcc.npz"""
    opt = O.Opt(ngf=8, ndf=8, teacher_ngf=16, teacher_ndf=16, direction=str(z['direction']), backbone='resnet')
    s_sG, s_sD, s_tG, s_tD, s_T = [int(v) for v in z['seeds']]
    teacher = O.Pix2PixOracle(opt, recipe_state_dict(O.mobile_resnet_shapes(16), s_tG),
                              recipe_state_dict(O.patchgan_shapes(16, 6, False), s_tD), masked=False)
    sD = recipe_state_dict(O.patchgan_shapes(8, 6, True), s_sD)
    sD['model.2.alpha'][0] = 0.3
    T = [recipe_transform(64, 32, s_T + i) for i in range(4)]
    m = O.Pix2PixOracle(opt, recipe_state_dict(O.mobile_resnet_shapes(8), s_sG), sD, T, masked=True, teacher=teacher)
    return m, teacher, opt


def test_resnet_backbone_gcc_iteration(golden_dir):
    """MobileResnetGenerator (separable convs + InstanceNorm + reflect padding) under the Pix2Pix GCC step"""
    z = load(golden_dir, 'pix2pix_resnet_gcc.npz')
    assert list(O.mobile_resnet_shapes(8).keys()) == [str(k) for k in z['G_keys']]
    m, teacher, opt = build_resnet_gcc_oracle(z)
    A, B = torch.from_numpy(z['A']), torch.from_numpy(z['B'])
    real_A = A if opt.direction == 'AtoB' else B
    with torch.no_grad():
        out = O.mobile_resnet_forward(m.G, real_A)
    np.testing.assert_allclose(out.numpy(), z['eval.fake_B'], atol=2e-5)
    m.set_input(A, B)
    m.optimize_parameters()
    np.testing.assert_allclose(m.fake_B.numpy(), z['train.fake_B'], atol=2e-5)
    np.testing.assert_allclose(teacher.fake_B.numpy(), z['train.Tfake_B'], atol=2e-5)
    for j in range(4):
        ref = z['sfeat.%d' % j]
        np.testing.assert_allclose(list(m.g_feats.values())[j].detach().numpy(), ref, atol=2e-5 + 1e-4 * np.abs(ref).max())
    for j in range(6):
        ref = z['target.%d' % j]
        np.testing.assert_allclose(m.targets[j].numpy(), ref, atol=2e-5 + 1e-4 * np.abs(ref).max())
    m.set_input(torch.from_numpy(z['vA']), torch.from_numpy(z['vB']))
    m.clipping_mask_alpha()
    m.optimizer_netD_arch()
    for k in z.files:
        if k.startswith('loss.'):
            ref = float(z[k])
            assert abs(m.losses[k[5:]] - ref) <= 2e-4 * max(1.0, abs(ref)), (k, m.losses[k[5:]], ref)
    # biases in front of an InstanceNorm have an analytically zero gradient (rounding noise through Adam): skip them
    skip = lambda k: k.endswith('.bias') and not k.startswith('model.26')
    _compare_sd(m.G, z, 'final.sG.', atol=3e-5, skip=skip)
    _compare_sd(teacher.G, z, 'final.tG.', atol=3e-5, skip=skip)
    _compare_sd(m.D, z, 'final.sD.', atol=3e-5)


def build_cyclegan_oracle(z):
    """MobileCycleGAN student (ngf 8, masked BN D ndf 8) + teacher (ngf 16, InstanceNorm D ndf 16): cyclegan_gcc.npz"""
    opt = O.Opt(ngf=8, ndf=8, teacher_ngf=16, teacher_ndf=16, direction=str(z['direction']), gan_mode=str(z['gan_mode']),
                lambda_L1=float(z['lambda_L1']), lambda_A=float(z['lambda_A']), lambda_B=float(z['lambda_B']),
                lambda_identity=float(z['lambda_identity']), lambda_content=0.01, lambda_gram=10.0)
    gs, ds = O.mobile_resnet_shapes(8), O.patchgan_shapes(8, 3, True)
    gt, dt = O.mobile_resnet_shapes(16), O.patchgan_shapes(16, 3, False, norm='instance')
    teacher = O.CycleGANOracle(opt, {'A': recipe_state_dict(gt, 605), 'B': recipe_state_dict(gt, 606)},
                               {'A': recipe_state_dict(dt, 607), 'B': recipe_state_dict(dt, 608)}, masked=False)
    D = {'A': recipe_state_dict(ds, 603), 'B': recipe_state_dict(ds, 604)}
    D['A']['model.2.alpha'][0] = 0.3
    D['B']['model.5.alpha'][1] = 0.45
    T = {'A': [recipe_transform(64, 32, 620 + i) for i in range(4)], 'B': [recipe_transform(64, 32, 630 + i) for i in range(4)]}
    m = O.CycleGANOracle(opt, {'A': recipe_state_dict(gs, 601), 'B': recipe_state_dict(gs, 602)}, D, T, masked=True,
                         teacher=teacher)
    return m, teacher, opt


def _pre_norm_bias(name):
    return name.endswith('.bias') and not name.startswith('model.26')


def test_cyclegan_two_iterations(golden_dir):
    z = load(golden_dir, 'cyclegan_gcc.npz')
    assert list(O.patchgan_shapes(8, 3, True).keys()) == [str(k) for k in z['D_keys']]
    assert list(O.patchgan_shapes(16, 3, False, norm='instance').keys()) == [str(k) for k in z['TD_keys']]
    m, teacher, opt = build_cyclegan_oracle(z)
    for it in range(2):
        m.set_input(torch.from_numpy(z['it%d.A' % it]), torch.from_numpy(z['it%d.B' % it]))
        m.optimize_parameters()
        if it == 0:
            for n in ('fake_A', 'fake_B', 'rec_A', 'rec_B', 'idt_A', 'idt_B'):
                np.testing.assert_allclose(getattr(m, n).numpy(), z['it0.' + n], atol=3e-5, err_msg=n)
            np.testing.assert_allclose(teacher.fake_A.numpy(), z['it0.Tfake_A'], atol=3e-5)
            np.testing.assert_allclose(teacher.fake_B.numpy(), z['it0.Tfake_B'], atol=3e-5)
            for w in 'AB':
                for j in range(6):
                    ref = z['it0.target_%s.%d' % (w, j)]
                    np.testing.assert_allclose(m.targets[w][j].numpy(), ref, atol=2e-5 + 1e-4 * np.abs(ref).max())
                for j in range(4):
                    ref = z['it0.sfeat_%s.%d' % (w, j)]
                    np.testing.assert_allclose(list(m.g_feats[w].values())[j].detach().numpy(), ref,
                                               atol=2e-5 + 1e-4 * np.abs(ref).max())
        m.set_input(torch.from_numpy(z['it%d.vA' % it]), torch.from_numpy(z['it%d.vB' % it]))
        m.clipping_mask_alpha()
        m.optimizer_netD_arch()
        for k in z.files:
            for pre, who in (('it%d.loss.' % it, m), ('it%d.tloss.' % it, teacher)):
                if k.startswith(pre):
                    name, ref = k[len(pre):], float(z[k])
                    assert abs(who.losses[name] - ref) <= 2e-4 * max(1.0, abs(ref)), (it, k, who.losses[name], ref)
    # post-step weights: Adam's first steps are sign-like (|update| ~ lr = 2e-4 whatever the gradient's size), so an
    # element whose gradient is ~0 amplifies fp32 summation-order noise (the oracle sums the gradients of one
    # G_A(real_A) pass where the reference sums two identical passes).  Seen: 1 element in 2048 per tensor (median
    # error 1e-7); allowed: 0.2% of a tensor's elements, each within the two steps' bound 2 * 2.2 * lr
    kw = dict(atol=4e-5, skip=_pre_norm_bias, outliers=2e-3, hard=2 * 2.2 * 2e-4)
    for w in 'AB':
        _compare_sd(m.G[w], z, 'final.sG_%s.' % w, **kw)
        _compare_sd(teacher.G[w], z, 'final.tG_%s.' % w, **kw)
        _compare_sd(m.D[w], z, 'final.sD_%s.' % w, atol=4e-5)
        # the InstanceNorm discriminator's inner conv biases also sit in front of a norm
        _compare_sd(teacher.D[w], z, 'final.tD_%s.' % w, atol=4e-5,
                    skip=lambda n: n in ('model.2.bias', 'model.5.bias', 'model.8.bias'))
        for i in range(4):
            np.testing.assert_allclose(m.T[w][i].detach().numpy(), z['final.T_%s.%d' % (w, i)], atol=1e-4)


def test_cyclegan_pretrain_l1_sparsity_and_image_pool(golden_dir):
    import random
    z = load(golden_dir, 'cyclegan_pretrain.npz')
    opt = O.Opt(ngf=8, ndf=8, direction=str(z['direction']), gan_mode='lsgan', lambda_weight=1e-3)
    gs, ds = O.mobile_resnet_shapes(8), O.patchgan_shapes(8, 3, False, norm='instance')
    # float64, as the fixture (make_fixtures.float64): the first Adam step moves every weight by +-lr, and the sign of a
    # near-zero gradient is float32 summation noise that differs between CPUs
    f64 = torch.float64
    m = O.CycleGANOracle(opt, {'A': as_dtype(recipe_state_dict(gs, 641), f64), 'B': as_dtype(recipe_state_dict(gs, 642), f64)},
                         {'A': as_dtype(recipe_state_dict(ds, 643), f64), 'B': as_dtype(recipe_state_dict(ds, 644), f64)}, masked=False)
    m.set_input(torch.from_numpy(z['A']).double(), torch.from_numpy(z['B']).double())
    m.optimize_parameters()
    for k in z.files:
        if k.startswith('loss.'):
            ref = float(z[k])
            assert abs(m.losses[k[5:]] - ref) <= 2e-4 * max(1.0, abs(ref)), (k, m.losses[k[5:]], ref)
    for w in 'AB':
        _compare_sd(m.G[w], z, 'final.G_%s.' % w, atol=3e-5, skip=_pre_norm_bias)
        _compare_sd(m.D[w], z, 'final.D_%s.' % w, atol=3e-5, skip=lambda n: n in ('model.2.bias', 'model.5.bias', 'model.8.bias'))
    random.seed(1234)
    pool = O.ImagePool(3)
    for step in range(8):
        imgs = torch.arange(2, dtype=torch.float32).reshape(2, 1, 1, 1) + 10 * step
        assert pool.query(imgs).reshape(-1).tolist() == z['pool.returned'][step].tolist(), step


def build_sagan_oracle(z, dtype=torch.float32):
    """SAGAN student (ngf 8, masked D ndf 8) + teacher (ngf 16 / ndf 16) with the recipe weights of sagan_gcc.npz, in `dtype`"""
    opt = O.Opt(ngf=8, ndf=8, teacher_ngf=16, teacher_ndf=16, gan_mode=str(z['gan_mode']), lr=float(z['lr']),
                lambda_L1=1.0, lambda_content=1.0, lambda_gram=1.0)
    teacher = O.SAGANOracle(opt, as_dtype(recipe_state_dict(O.sagan_generator_shapes(16), 803), dtype),
                            as_dtype(recipe_state_dict(O.sagan_discriminator_shapes(16, False), 804), dtype), masked=False)
    sD = as_dtype(recipe_state_dict(O.sagan_discriminator_shapes(8, True), 802), dtype)
    sD['l1.1.alpha'][0] = 0.3
    sD['l3.1.alpha'][2] = 0.5
    T = [recipe_transform(int(t), int(s_), 810 + i).to(dtype) for i, (t, s_) in enumerate(z['T_shapes'])]
    m = O.SAGANOracle(opt, as_dtype(recipe_state_dict(O.sagan_generator_shapes(8), 801), dtype), sD, T, masked=True, teacher=teacher)
    return m, teacher, opt


def test_sagan_two_iterations(golden_dir):
    z = load(golden_dir, 'sagan_gcc.npz')
    assert list(O.sagan_generator_shapes(8).keys()) == [str(k) for k in z['G_keys']]
    assert list(O.sagan_discriminator_shapes(8, True).keys()) == [str(k) for k in z['D_keys']]
    assert list(O.sagan_discriminator_shapes(16, False).keys()) == [str(k) for k in z['TD_keys']]
    # float64 (make_fixtures.float64): iteration 1 sits behind Adam sign steps.  The losses and final states are checked
    # against the reference's float64 run (sagan_gcc_f64.npz), the values ahead of the first step against its float32 run
    z64 = load(golden_dir, 'sagan_gcc_f64.npz')
    m, teacher, opt = build_sagan_oracle(z, torch.float64)
    # duplicated optimizer entries (hazard H5); the generator's u, v are listed too but never receive a gradient
    assert sorted(m.G_dup) == sorted(str(k) for k in z['dup_G'] if not (str(k).endswith('_u') or str(k).endswith('_v')))
    assert sorted(m.D_dup) == sorted(str(k) for k in z['dup_D'])
    # eval image on a copy (the pass moves u, v)
    G0 = {k: v.clone() for k, v in m.G.items()}
    with torch.no_grad():
        out = O.sagan_generator_forward(G0, torch.from_numpy(z['eval.z']).double(), train=False)
    np.testing.assert_allclose(out.numpy(), z['eval.fake_img'], atol=2e-5)
    for it in range(2):
        m.set_input(torch.from_numpy(z['it%d.z' % it]).double(), torch.from_numpy(z['it%d.real' % it]).double())
        m.optimize_parameters()
        if it == 0:
            np.testing.assert_allclose(m.fake_img.numpy(), z['it0.fake_img'], atol=2e-5)
            np.testing.assert_allclose(teacher.fake_img.numpy(), z['it0.Tfake_img'], atol=2e-5)
            for j in range(4):
                ref = z['it0.target.%d' % j]
                np.testing.assert_allclose(m.targets[j].numpy(), ref, atol=2e-5 + 1e-4 * np.abs(ref).max())
            for j in range(2):
                ref = z['it0.sfeat.%d' % j]
                np.testing.assert_allclose(list(m.g_feats.values())[j].detach().numpy(), ref, atol=2e-5 + 1e-4 * np.abs(ref).max())
        m.set_input(torch.from_numpy(z['it%d.vz' % it]).double(), torch.from_numpy(z['it%d.vreal' % it]).double())
        m.clipping_mask_alpha()
        m.optimizer_netD_arch()
        for k in z64.files:
            for pre, who in (('it%d.loss.' % it, m), ('it%d.tloss.' % it, teacher)):
                if k.startswith(pre):
                    name, ref = k[len(pre):], float(z64[k])
                    # iteration 1 sits behind Adam steps with beta1 = 0 (pure sign steps of 4e-4, twice for the
                    # duplicated entries): elements with a ~0 gradient amplify fp32 summation noise into the losses
                    tol = 2e-4 if it == 0 else 1.5e-3
                    assert abs(who.losses[name] - ref) <= tol * max(1.0, abs(ref)), (it, k, who.losses[name], ref)
    kw = dict(atol=4e-5, outliers=5e-3, hard=2 * 2 * 2.2 * 4e-4)
    # biases of the SN convs in front of a BatchNorm (generator l1..l4) have zero gradient
    skipG = lambda n: n.endswith('.module.bias') or n.endswith('key_conv.bias')
    # zero-gradient parameters of the discriminators: key bias (softmax is shift invariant) and, with every hinge term
    # active, the value bias of attn2 (the real and fake passes cancel)
    skipD = lambda n: n.endswith('key_conv.bias') or n == 'attn2.value_conv.bias'
    _compare_sd(m.G, z64, 'final.sG.', skip=skipG, **kw)
    _compare_sd(teacher.G, z64, 'final.tG.', skip=skipG, **kw)
    _compare_sd(m.D, z64, 'final.sD.', skip=skipD, **kw)
    _compare_sd(teacher.D, z64, 'final.tD.', skip=skipD, **kw)
    for i in range(2):
        np.testing.assert_allclose(m.T[i].detach().numpy(), z64['final.T.%d' % i], atol=1e-4)


VGG_STANDIN = (8, 8, 'M', 16, 16, 'M', 32, 32, 32, 32, 'M', 64, 64, 64, 64, 'M', 64, 64, 64, 64)


def build_srgan_oracle(z):
    """SRGAN student (ngf 8, masked D ndf 8) + teacher (ngf 16 / ndf 16) + VGG stand-in with the conditioned recipe
    weights of srgan_gcc.npz"""
    from tests.golden.recipe import srgan_condition
    opt = O.Opt(ngf=8, ndf=8, teacher_ngf=16, teacher_ndf=16, gan_mode=str(z['gan_mode']), lr=float(z['lr']),
                threshold=float(z['threshold']), lambda_L1=0.5, lambda_content=1.0, lambda_gram=1.0, lambda_SR_content=0.5)
    sds = [recipe_state_dict(O.srresnet_shapes(8), 901), recipe_state_dict(O.sr_discriminator_shapes(8, True), 902),
           recipe_state_dict(O.srresnet_shapes(16), 903), recipe_state_dict(O.sr_discriminator_shapes(16, False), 904),
           recipe_state_dict(O.vgg_shapes(VGG_STANDIN), 905)]
    for sd in sds:
        srgan_condition(sd)
    sG, sD, tG, tD, V = sds
    sD['conv_blocks.0.conv_block.1.alpha'][0] = 0.3
    sD['conv_blocks.2.conv_block.2.alpha'][1] = 0.5
    teacher = O.SRGANOracle(opt, tG, tD, V, masked=False, vgg_cfg=VGG_STANDIN)
    T = [recipe_transform(16, 8, 910 + i) for i in range(4)]
    m = O.SRGANOracle(opt, sG, sD, V, T, masked=True, teacher=teacher, vgg_cfg=VGG_STANDIN)
    return m, teacher, opt


def test_srgan_two_iterations(golden_dir):
    z = load(golden_dir, 'srgan_gcc.npz')
    assert list(O.srresnet_shapes(8).keys()) == [str(k) for k in z['G_keys']]
    assert list(O.sr_discriminator_shapes(8, True).keys()) == [str(k) for k in z['D_keys']]
    assert list(O.sr_discriminator_shapes(16, False).keys()) == [str(k) for k in z['TD_keys']]
    assert list(O.vgg_shapes(VGG_STANDIN).keys()) == [str(k) for k in z['V_keys']]
    m, teacher, opt = build_srgan_oracle(z)
    # hazard H5: the distillation optimizer leaves the PReLU slopes out
    assert sorted(m.G_keys) == sorted(str(k) for k in z['G_optimizer_names'])
    with torch.no_grad():
        out = O.srresnet_forward({k: v.clone() for k, v in m.G.items()}, torch.from_numpy(z['eval.lr']), train=False)
    np.testing.assert_allclose(out.numpy(), z['eval.fake_hr'], atol=2e-5)
    for it in range(2):
        m.set_input(torch.from_numpy(z['it%d.lr' % it]), torch.from_numpy(z['it%d.hr' % it]))
        m.optimize_parameters()
        if it == 0:
            np.testing.assert_allclose(m.fake_hr.numpy(), z['it0.fake_hr_norm'], atol=1e-4)
            for j in range(6):
                ref = z['it0.target.%d' % j]
                np.testing.assert_allclose(m.targets[j].numpy(), ref, atol=2e-5 + 1e-4 * np.abs(ref).max())
            for j in range(4):
                ref = z['it0.sfeat.%d' % j]
                np.testing.assert_allclose(list(m.g_feats.values())[j].detach().numpy(), ref, atol=2e-5 + 1e-4 * np.abs(ref).max())
        m.set_input(torch.from_numpy(z['it%d.vlr' % it]), torch.from_numpy(z['it%d.vhr' % it]))
        m.clipping_mask_alpha()
        m.optimizer_netD_arch()
        for k in z.files:
            for pre, who in (('it%d.loss.' % it, m), ('it%d.tloss.' % it, teacher)):
                if k.startswith(pre):
                    name, ref = k[len(pre):], float(z[k])
                    assert abs(who.losses[name] - ref) <= (2e-4 if it == 0 else 1.5e-3) * max(1.0, abs(ref)), (it, k, who.losses[name], ref)
    # (running statistics of iteration 1 are taken behind one Adam step: fp32 summation-order noise through the sign-like
    # first step moves them by ~6e-5)
    kw = dict(atol=2e-4, outliers=5e-3, hard=2 * 2.2 * float(z['lr']))
    # conv biases in front of a BatchNorm have zero gradient
    zero_g = lambda n: n.endswith('.conv_block.0.bias') and not n.startswith('conv_block1.') and not n.startswith('conv_block3.')
    zero_d = lambda n: n.endswith('.conv_block.0.bias') and not n.startswith('conv_blocks.0.')
    _compare_sd(m.G, z, 'final.sG.', skip=zero_g, **kw)
    _compare_sd(teacher.G, z, 'final.tG.', skip=zero_g, **kw)
    _compare_sd(m.D, z, 'final.sD.', skip=zero_d, **kw)
    _compare_sd(teacher.D, z, 'final.tD.', skip=zero_d, **kw)
    for i in range(4):
        np.testing.assert_allclose(m.T[i].detach().numpy(), z['final.T.%d' % i], atol=1e-4)


# ---- the bf16-EMULATING mode of the oracle, pinned ---------------------------------------------------
# oracle.EMULATE_BF16 is the one oracle mode no reference fixture exercises by itself: its rounding points were chosen to follow the
# HIP path, and the GPU tests accept a logged loss that sits within the bar of EITHER the reference or this mode.  This test holds
# the mode itself inside a stated band of the reference's own fixtures, on the CPU, for all four families -- so "within the bar of
# the emulating oracle" can never mean more than "within bar + band of the reference".  Bands (scratch/r6/emul_loss_band.py prints
# the measured values): Pix2Pix, CycleGAN, SRGAN -- the GPU tests' own bar (tests/_updates.loss_tol: 3e-2 relative, floor one flipped
# decision of the fixture's PatchGAN map / 1e-3), measured <= 0.62 bars; SAGAN (Adam with beta1 = 0: every step is a sign step of the
# whole weight, so behind the first update bf16 storage alone moves the hinge terms) -- 5e-2 relative in iteration 0 (measured 3.6e-2),
# 0.25 relative in iteration 1 (measured 0.204 on D_real = 0.194, 0.108 on the others).
_EMUL_FAMILIES = {
    # family: (fixture, builder, input keys, n_map of the fixture's discriminator output, {iteration: relative bar})
    'pix2pix': ('pix2pix_gcc_d6.npz', lambda z: build_gcc_oracle(z), ('A', 'B', 'vA', 'vB'), 72, {0: 3e-2, 1: 3e-2}),
    'cyclegan': ('cyclegan_gcc.npz', lambda z: build_cyclegan_oracle(z), ('A', 'B', 'vA', 'vB'), 36, {0: 3e-2, 1: 3e-2}),
    'sagan': ('sagan_gcc.npz', lambda z: build_sagan_oracle(z), ('z', 'real', 'vz', 'vreal'), 10 ** 9, {0: 5e-2, 1: 0.25}),
    'srgan': ('srgan_gcc.npz', lambda z: build_srgan_oracle(z), ('lr', 'hr', 'vlr', 'vhr'), 10 ** 9, {0: 3e-2, 1: 3e-2}),
}


@pytest.mark.parametrize('family', sorted(_EMUL_FAMILIES))
def test_emulating_oracle_losses_stay_in_a_band_of_the_reference(golden_dir, family):
    from tests import _updates
    fixture, build, ins, n_map, rel = _EMUL_FAMILIES[family]
    z = load(golden_dir, fixture)
    O.EMULATE_BF16 = True
    try:
        m, teacher, _ = build(z)
        worst, n = (0.0, ''), 0
        for it in range(2):
            m.set_input(torch.from_numpy(z['it%d.%s' % (it, ins[0])]), torch.from_numpy(z['it%d.%s' % (it, ins[1])]))
            m.optimize_parameters()
            m.set_input(torch.from_numpy(z['it%d.%s' % (it, ins[2])]), torch.from_numpy(z['it%d.%s' % (it, ins[3])]))
            m.clipping_mask_alpha()
            m.optimizer_netD_arch()
            for k in z.files:
                for pre, who in (('it%d.loss.' % it, m), ('it%d.tloss.' % it, teacher)):
                    if k.startswith(pre):
                        name, ref = k[len(pre):], float(z[k])
                        err = abs(float(who.losses[name]) - ref) / _updates.loss_tol(name, ref, n_map, rel[it])
                        n += 1
                        if err > worst[0]:
                            worst = (err, '%s%s' % (pre, name))
                        assert err <= 1.0, (family, k, float(who.losses[name]), ref, err)
    finally:
        O.EMULATE_BF16 = False
    assert n >= 24
    _updates._report('bf16-emulating oracle vs the reference fixture [%s]: %d logged losses over two iterations, worst |err| / band '
                     '%.3f (%s)' % (family, n, worst[0], worst[1]))
