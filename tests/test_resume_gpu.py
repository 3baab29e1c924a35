"""Resuming a run (--continue_train): HipAdam's state in torch.optim.Adam's format, every model's training_state() round trip,
and gcc_amd.train interrupted at an epoch boundary and resumed -- all BIT-identical to the run that was not interrupted."""
import io
import os
import random
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


# ---- 1. optimizer state ------------------------------------------------------------------------------------------------
def _adam_setup(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(8, 4, 4, 4), (8,), (6, 3)]                    # a 4x4 conv weight (channels_last in the flat slab), a BN vector, a dup
    return [torch.randn(s, generator=g) for s in shapes]


def _grads(step):
    g = torch.Generator().manual_seed(1000 + step)
    return [torch.randn(s, generator=g) * 1e-2 for s in [(8, 4, 4, 4), (8,), (6, 3)]]


def _hip(values):
    from gcc_amd.models.Pix2Pix import HipAdam
    ps = [torch.nn.Parameter(v.clone().to(DEV)) for v in values]
    return ps, HipAdam(ps, lr=2e-3, betas=(0.5, 0.999), dup=[ps[2]])


def _hip_step(ps, o, step):
    for p, g in zip(ps, _grads(step)):
        p.grad.copy_(g.to(DEV))
    o.step()


def test_hip_adam_state_dict_matches_torch_adam_and_round_trips_bit_exactly():
    K1, K2 = 3, 4
    values = _adam_setup(0)
    ps, o = _hip(values)
    assert ps[0].is_contiguous(memory_format=torch.channels_last) and not ps[0].is_contiguous()
    assert o.state_dict()['state'] == {}
    tp = [torch.nn.Parameter(v.clone().to(DEV)) for v in values]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                      # torch warns about the twice-listed parameter
        to = torch.optim.Adam(tp + [tp[2]], lr=2e-3, betas=(0.5, 0.999), foreach=False)
    for k in range(K1):
        _hip_step(ps, o, k)
        for p, g in zip(tp, _grads(k)):
            p.grad = g.to(DEV)
        to.step()
    torch.cuda.synchronize()
    sd, ref = o.state_dict(), to.state_dict()
    assert sorted(sd['state']) == [0, 1, 2]
    for i in range(3):
        mine, theirs = sd['state'][i], to.state[tp[i]]        # (torch numbers the twice-listed parameter by its last place)
        assert any(sorted(e) == sorted(mine) for e in ref['state'].values())
        assert sorted(mine) == sorted(theirs) == ['exp_avg', 'exp_avg_sq', 'step']
        assert float(mine['step']) == float(theirs['step']) == (2 * K1 if i == 2 else K1)
        for key in ('exp_avg', 'exp_avg_sq'):
            assert mine[key].device.type == 'cpu' and mine[key].is_contiguous() and mine[key].shape == theirs[key].shape
            torch.testing.assert_close(mine[key], theirs[key].cpu(), rtol=1e-5, atol=1e-9)
    assert sd['param_groups'][0]['params'] == [0, 1, 2]
    assert sd['param_groups'][0]['betas'] == (0.5, 0.999) and sd['param_groups'][0]['lr'] == 2e-3

    # K1 steps -> state_dict (through torch.save) -> fresh optimizer -> K2 steps  ==  K1 + K2 steps on one optimizer
    buf = io.BytesIO()
    torch.save({'values': [p.detach().cpu() for p in ps], 'opt': sd}, buf)
    buf.seek(0)
    saved = torch.load(buf, weights_only=False)
    ps2, o2 = _hip(_adam_setup(1))
    with torch.no_grad():
        for p, v in zip(ps2, saved['values']):
            p.copy_(v)
    m_ptrs = [t.data_ptr() for t in o2.plan.m + o2.plan_dup.m]
    o2.load_state_dict(saved['opt'])
    assert [t.data_ptr() for t in o2.plan.m + o2.plan_dup.m] == m_ptrs, 'moments must be loaded in place'
    assert (o2.plan.step_count, o2.plan_dup.step_count) == (K1, 2 * K1)
    for k in range(K1, K1 + K2):
        _hip_step(ps, o, k)
        _hip_step(ps2, o2, k)
    torch.cuda.synchronize()
    for a, b in zip(ps, ps2):
        assert torch.equal(a.detach(), b.detach())
    fa, fb = o.state_dict(), o2.state_dict()
    for i in range(3):
        for key in ('step', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(fa['state'][i][key], fb['state'][i][key]), (i, key)


# ---- 2./3. model round trips -------------------------------------------------------------------------------------------
COMMON = ['--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--teacher_ngf', '16', '--online_distillation', '--darts_discriminator',
          '--arch_lr', '1e-4', '--arch_lr_step', '--n_epochs', '4', '--n_epochs_decay', '4']
ARGV = {
    'pix2pix_unet': ['--dataroot', 'synthetic', '--model', 'pix2pix', '--num_downs', '6', '--crop_size', '64', '--batch_size', '2',
                     '--lambda_content', '50', '--lambda_gram', '1e4'] + COMMON,
    'pix2pix_resnet': ['--dataroot', 'synthetic', '--model', 'pix2pix', '--backbone', 'resnet', '--crop_size', '64',
                       '--batch_size', '2', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--n_epochs', '4', '--n_epochs_decay', '4'],
    'cyclegan': ['--dataroot', 'synthetic', '--model', 'cyclegan', '--crop_size', '64', '--batch_size', '1',
                 '--lambda_content', '0.01', '--lambda_gram', '10'] + COMMON,
    'sagan': ['--dataroot', 'synthetic', '--model', 'sagan', '--threshold', '0.1', '--lambda_L1', '1', '--lambda_content', '1',
              '--lambda_gram', '1'] + COMMON,
    'srgan': ['--dataroot', 'synthetic', '--model', 'srgan', '--image_size', '48', '--lambda_content', '1',
              '--lambda_gram', '1'] + COMMON,
}


def _build(which, seed):
    from gcc_amd import train
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    random.seed(seed)
    torch.manual_seed(seed)
    opt = options.parse(ARGV[which])
    opt.isTrain = True
    if which != 'pix2pix_unet':
        opt.teacher_ndf = 16
    if which in ('sagan', 'srgan'):
        opt.batch_size = 2
    if which == 'pix2pix_unet':
        opt.ema_beta = 0.9
    cls = get_model_class(opt)
    model = cls(opt)
    if which == 'cyclegan':
        from gcc_amd.models.CycleGAN import ImagePool
        model.pool = {'A': ImagePool(3), 'B': ImagePool(3)}  # full after three iterations: later ones draw from Python's random
    if opt.online_distillation:
        train.attach_teacher(model, opt, cls)
    model.model_train()
    return model, opt


def _data(opt, n, seed):
    from gcc_amd.train import SyntheticPairs
    return list(SyntheticPairs(opt, n, seed))


def _iterate(model, opt, data, val):
    losses = []
    for d, v in zip(data, val):
        model.set_input(d)
        model.optimize_parameters()
        if opt.darts_discriminator and model.teacher_model is not None:
            model.set_input(v)
            model.clipping_mask_alpha()
            model.optimizer_netD_arch()
        losses.append(dict(model.get_current_losses()))
    return losses


def _flat(prefix, o, acc):
    if torch.is_tensor(o):
        acc[prefix] = o
    elif isinstance(o, dict):
        for k, v in o.items():
            _flat('%s.%s' % (prefix, k), v, acc)
    elif isinstance(o, (list, tuple)):
        for i, v in enumerate(o):
            _flat('%s[%d]' % (prefix, i), v, acc)
    else:
        acc[prefix] = o
    return acc


def _rng():
    return random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state()


def _set_rng(s):
    random.setstate(s[0])
    torch.set_rng_state(s[1])
    torch.cuda.set_rng_state(s[2])


@pytest.mark.parametrize('which', ['pix2pix_unet', 'pix2pix_resnet', 'cyclegan', 'sagan', 'srgan'])
def test_training_state_round_trip_is_bit_exact(which, monkeypatch, tmp_path):
    monkeypatch.setenv('GCC_VGG19_RANDOM', '1')
    K1, K2 = 4, 3
    model, opt = _build(which, 0)
    data, val = _data(opt, K1 + K2, 11), _data(opt, K1 + K2, 12)
    _iterate(model, opt, data[:K1], val[:K1])
    model.update_learning_rate(1)
    if which == 'pix2pix_unet':
        assert model.opt.ema_beta != 0.9 and model.G.seed != 0x5EED
    buf = io.BytesIO()
    torch.save(model.training_state(), buf)
    model.save_models(0, str(tmp_path / 's'))
    if model.teacher_model is not None:
        model.teacher_model.save_models(0, str(tmp_path / 't'))
    rng = _rng()
    straight = _iterate(model, opt, data[K1:], val[K1:])
    final = _flat('', model.training_state(), {})
    del model

    resumed, r_opt = _build(which, 1)                         # other initial weights: everything must come from the state
    buf.seek(0)
    resumed.load_training_state(torch.load(buf, weights_only=False))
    _set_rng(rng)
    got = _iterate(resumed, r_opt, data[K1:], val[K1:])
    final2 = _flat('', resumed.training_state(), {})
    del resumed
    assert got == straight, 'logged losses of the resumed iterations differ'
    assert final.keys() == final2.keys() and len(final) > 20
    bad = [k for k in final if not (torch.equal(final[k], final2[k]) if torch.is_tensor(final[k]) else final[k] == final2[k])]
    assert not bad, bad[:8]

    # control: the weights of save_models alone (fresh optimizer moments, step counts, schedulers, seeds, pools) -- another run
    ctl, c_opt = _build(which, 1)
    ctl.load_models(str(tmp_path / 's' / 'model_0.pth'))
    if ctl.teacher_model is not None:
        ctl.teacher_model.load_models(str(tmp_path / 't' / 'model_0.pth'))
    _set_rng(rng)
    _iterate(ctl, c_opt, data[K1:], val[K1:])
    final3 = _flat('', ctl.training_state(), {})
    del ctl
    differ = [k for k in final if torch.is_tensor(final[k]) and final[k].is_floating_point() and k.startswith('.nets')
              and not torch.equal(final[k], final3[k])]
    assert differ, 'a weights-only restart ended on the same weights: the round trip above would not notice a lost state'


# ---- 4./5. through gcc_amd.train ---------------------------------------------------------------------------------------
class _Killed(Exception):
    pass


class _StopAt:
    """the training set, raising at the first batch of epoch `epoch` (a run killed there)"""

    def __init__(self, inner, epoch):
        self.inner, self.epoch, self.calls = inner, epoch, 0

    def __len__(self):
        return len(self.inner)

    def __iter__(self):
        self.calls += 1
        if self.calls == self.epoch:
            raise _Killed('stopped at epoch %d' % self.epoch)
        return iter(self.inner)


E2E = {
    'pix2pix': ['--dataroot', 'synthetic:2', '--model', 'pix2pix', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--teacher_ngf', '16',
                '--num_downs', '6', '--crop_size', '64', '--online_distillation', '--darts_discriminator', '--lambda_content', '50',
                '--lambda_gram', '1e4', '--n_epochs', '2', '--n_epochs_decay', '1', '--print_freq', '1', '--continue_train', '1'],
    # (SRGAN's schedule is fixed by the option table: 30 epochs at batch 16, the learning rate stepped after 15)
    'srgan': ['--dataroot', 'synthetic:3', '--model', 'srgan', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--teacher_ngf', '16',
              '--online_distillation', '--darts_discriminator', '--image_size', '48', '--print_freq', '100', '--continue_train', '1'],
}


def _run(argv, root, datasets=None):
    from gcc_amd import train
    random.seed(7)
    torch.manual_seed(7)
    model = train.main(argv + ['--checkpoints_dir', str(root), '--name', 'r'], datasets=datasets)
    torch.cuda.synchronize()
    del model


def _last(root):
    ck = root / 'r' / 'checkpoints'
    files = os.listdir(str(ck))
    assert len(files) == 1 and files[0].startswith('model_'), files
    return _flat('', torch.load(str(ck / files[0]), map_location='cpu'), {})


@pytest.mark.parametrize('which,replay', [('pix2pix', '0'), ('srgan', '1')])
def test_train_resumed_at_an_epoch_boundary_ends_on_the_same_bits(tmp_path, monkeypatch, which, replay):
    """A: the whole schedule straight (eager; pix2pix: three epochs).  B: the same argv, killed at the first batch of epoch 3.
    C: B's directory resumed (under GCC_REPLAY=1 for SRGAN).  C's final checkpoint is bit-identical to A's, and nothing but that
    checkpoint is in checkpoints/; a resume with another --ngf is refused first."""
    from gcc_amd import train
    from gcc_amd._lib import GccError
    from gcc_amd.options import options
    monkeypatch.setenv('GCC_VGG19_RANDOM', '1')
    argv = E2E[which]
    monkeypatch.setenv('GCC_REPLAY', '0')
    _run(argv, tmp_path / 'A')
    exp_a = tmp_path / 'A' / 'r'
    assert (exp_a / train.STATE_FILE).exists(), 'a first start with --continue_train leaves a state file'
    log_a = (exp_a / 'logger.log').read_text()
    assert 'resuming' not in log_a and 'training state of epoch 2 written' in log_a
    assert not [f for f in os.listdir(str(exp_a)) if f.endswith('.tmp')]

    monkeypatch.setenv('GCC_REPLAY', replay)
    sets = train.make_datasets(options.parse(argv))
    with pytest.raises(_Killed):
        _run(argv, tmp_path / 'B', datasets=(_StopAt(sets[0], 3), sets[1]))
    exp_b = tmp_path / 'B' / 'r'
    assert torch.load(str(exp_b / train.STATE_FILE), map_location='cpu', weights_only=False)['epoch'] == 2
    assert not (exp_b / 'checkpoints').exists() or not os.listdir(str(exp_b / 'checkpoints'))

    other = list(argv)
    other[other.index('--ngf') + 1] = '16'
    with pytest.raises(GccError, match='ngf'):
        _run(other, tmp_path / 'B')

    _run(argv, tmp_path / 'B')
    log_b = (exp_b / 'logger.log').read_text()
    assert 'resuming from epoch 3' in log_b
    a, c = _last(tmp_path / 'A'), _last(tmp_path / 'B')
    assert a.keys() == c.keys() and len(a) > 20
    bad = [k for k in a if not (torch.equal(a[k], c[k]) if torch.is_tensor(a[k]) else a[k] == c[k])]
    assert not bad, bad[:8]
    assert os.listdir(str(exp_b / 'checkpoints')) == os.listdir(str(exp_a / 'checkpoints'))
