"""The four model families share one base (gcc_amd.models._base.GANModelBase): the reference's public surface is still there on
every class that had it, the optimizer is importable from both its new and its old place, and what all four classes used to
copy is defined once.  Host only: nothing here builds a model."""
import pytest

COMMON = ['set_input', 'forward', 'optimize_parameters', 'optimizer_netD_arch', 'clipping_mask_alpha', 'backward_G', 'backward_D',
          'backward_D_arch', 'get_D_arch_diff', 'save_models', 'load_models', 'model_train', 'model_eval', 'get_current_visuals',
          'get_current_losses', 'init_distillation', 'get_distillation_features', 'get_cfg', 'prune', 'update_learning_rate',
          'set_requires_grad', 'print_sparse_info', 'adaptive_ema_beta', 'refresh_weights', 'init_net', 'max_min_conv_norm',
          'training_state', 'load_training_state', 'set_stream_schedule']
# the public names each class defined itself before the base existed, beyond COMMON
EXTRA = {
    'Pix2Pix.Pix2PixModel': ['infer', 'infer_nhwc', 'finish_G_update', 'max_min_bn_scale', 'norm_prune', 'scale_prune',
                             'scale_prune_cfg', 'resnet_prune', 'replay_supported', 'fake_B', 'Tfake_B'],
    'CycleGAN.MobileCycleGANModel': ['infer', 'infer_nhwc', 'visual_forward', 'get_prunenet_cfg', 'resnet_prune', 'fake_A', 'fake_B',
                                     'rec_A', 'rec_B', 'idt_A', 'idt_B', 'Tfake_A', 'Tfake_B'],
    'SAGAN.SAGANModel': ['infer', 'infer_nhwc', 'max_min_bn_scale', 'norm_prune', 'scale_prune', 'fake_img', 'Tfake_img'],
    'SRGAN.SRGAN': ['get_current_psnr', 'get_current_ssim', 'optimize_content_parameters', 'max_min_bn_scale', 'norm_prune',
                    'scale_prune', 'fake_hr', 'real_hr', 'Tfake_hr'],
}
SHARED_BY_ALL = ['_l', 'adaptive_ema_beta', 'set_requires_grad', 'get_current_visuals']


def _cls(path):
    import importlib
    mod, name = path.split('.')
    return getattr(importlib.import_module('gcc_amd.models.' + mod), name)


@pytest.mark.parametrize('path', sorted(EXTRA))
def test_family_derives_from_the_base_and_keeps_its_surface(path):
    from gcc_amd.models._base import GANModelBase
    cls = _cls(path)
    assert issubclass(cls, GANModelBase) and cls.__mro__[1] is GANModelBase
    for name in COMMON + EXTRA[path]:
        attr = getattr(cls, name, None)
        assert callable(attr) or isinstance(attr, property), '%s lost %s' % (path, name)


def test_what_all_four_copied_is_defined_once():
    from gcc_amd.models._base import GANModelBase
    for name in SHARED_BY_ALL:
        assert name in vars(GANModelBase), name
        for path in EXTRA:
            assert name not in vars(_cls(path)), '%s defines its own %s' % (path, name)


def test_family_declarations():
    """what the shared checkpoint / cfg / distillation code reads from each family"""
    got = {p: (_cls(p).NETS, _cls(p).METRIC, _cls(p).CFGS, [n for _, ns in _cls(p).DISTILL_LOSSES for n in ns],
               list(_cls(p).DISTILL_VISUALS)) for p in EXTRA}
    two = ('filter_cfgs', 'channel_cfgs')
    assert got == {
        'Pix2Pix.Pix2PixModel': (('G', 'D'), 'fid', two, ['content', 'gram'], ['Tfake_B']),
        'CycleGAN.MobileCycleGANModel': (('G_A', 'G_B', 'D_A', 'D_B'), 'fid', ('cfg_AtoB', 'cfg_BtoA'),
                                         ['content_A', 'content_B', 'gram_A', 'gram_B', 'L1_A', 'L1_B'], ['Tfake_A', 'Tfake_B']),
        'SAGAN.SAGANModel': (('G', 'D'), 'fid', two, ['content', 'gram', 'L1'], ['Tfake_img']),
        'SRGAN.SRGAN': (('G', 'D'), 'psnr', two, ['content', 'gram', 'L1'], ['Tfake_hr']),
    }


def test_optimizer_has_one_home_and_the_old_name_still_works():
    from gcc_amd.models import CycleGAN, Pix2Pix, SAGAN, SRGAN, _optim, _resume
    for mod in (Pix2Pix, CycleGAN, SAGAN, SRGAN, _resume):
        assert mod.HipAdam is _optim.HipAdam
    assert _optim.HipAdam.__module__ == 'gcc_amd.models._optim'


def test_chain_wgrad_restores_the_switch(monkeypatch):
    from gcc_amd import engine
    from gcc_amd.models._base import _ChainWgrad
    for start in (True, False):
        monkeypatch.setattr(engine, 'OVERLAP_WGRAD', start)
        with _ChainWgrad():
            assert engine.OVERLAP_WGRAD is False
        assert engine.OVERLAP_WGRAD is start
        with _ChainWgrad(False):
            assert engine.OVERLAP_WGRAD is start
        assert engine.OVERLAP_WGRAD is start
