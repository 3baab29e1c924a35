"""The float64 yardstick of the MobileResnet generator's fp32 inference route (tests/_mobile_resnet_f64.py) held to the reference's
own images, and the host side of GCC_RESNET_PRECISION.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import _mobile_resnet_f64 as R


def _fixture(golden_dir):
    ckpt = torch.load(os.path.join(golden_dir, 'ref_checkpoint_cyclegan.pth'), map_location='cpu', weights_only=False)
    z = np.load(os.path.join(golden_dir, 'ref_checkpoint_cyclegan.npz'))
    t = lambda k: torch.from_numpy(z[k])
    return [('fake_B', ckpt['G_A'], t('A'), t('fake_B')), ('fake_A', ckpt['G_B'], t('B'), t('fake_A'))]


def test_float64_restatement_reproduces_the_reference_images(golden_dir):
    """max |fake - f64| <= 5e-6 for both generators (measured 1.24e-6 and 1.14e-6: the reference's own fp32 rounding through 40
    InstanceNorms).  A wrong restatement -- a missed ReLU, a bias dropped, the wrong output padding -- is off by orders of
    magnitude more."""
    for key, sd, x, fake in _fixture(golden_dir):
        convs, blocks = R.layout(sd)
        assert len(blocks) == 9
        f64 = R.resnet_eval(sd, x)
        assert f64.dtype == torch.float64 and tuple(f64.shape) == tuple(fake.shape)
        err = float((fake.double() - f64).abs().max())
        print('reference %s from float64: %.3g' % (key, err))
        assert 0 < err <= 5e-6, (key, err)


def test_fp32_restatement_is_as_close_as_the_reference(golden_dir):
    for key, sd, x, fake in _fixture(golden_dir):
        f64, f32 = R.resnet_eval(sd, x), R.resnet_eval(sd, x, torch.float32)
        assert f32.dtype == torch.float32
        err = float((f32.double() - f64).abs().max())
        print('fp32 restatement of %s from float64: %.3g' % (key, err))
        assert err <= 5e-6, (key, err)
        pre = R.resnet_eval(sd, x, pre_tanh=True)
        assert torch.equal(torch.tanh(pre), f64)


def test_tensor2im_bytes_match_the_cli_host_form():
    from gcc_amd.test import tensor2im_host
    x = torch.rand(2, 3, 5, 7, generator=torch.Generator().manual_seed(0)) * 2 - 1
    assert np.array_equal(R.tensor2im(x)[0].numpy(), tensor2im_host(x))


def test_resnet_precision_reads_the_variable(monkeypatch):
    from gcc_amd._lib import GccError
    from gcc_amd.models.Pix2Pix import RESNET_PRECISION_ENV, gen_precision, resnet_precision
    assert RESNET_PRECISION_ENV == 'GCC_RESNET_PRECISION'
    monkeypatch.delenv(RESNET_PRECISION_ENV, raising=False)
    monkeypatch.delenv('GCC_GEN_PRECISION', raising=False)
    assert resnet_precision() == 'bf16'
    monkeypatch.setenv(RESNET_PRECISION_ENV, 'bf16')
    assert resnet_precision() == 'bf16'
    monkeypatch.setenv(RESNET_PRECISION_ENV, 'fp32')
    assert resnet_precision() == 'fp32'
    assert gen_precision() == 'bf16' and gen_precision(only_bf16='--backbone resnet') == 'bf16'     # the other variable is untouched
    monkeypatch.setenv(RESNET_PRECISION_ENV, 'fp16')
    with pytest.raises(GccError, match='GCC_RESNET_PRECISION=fp16'):
        resnet_precision()
    monkeypatch.setenv(RESNET_PRECISION_ENV, 'bf16')
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')                  # GCC_GEN_PRECISION does not select the resnet's route
    assert resnet_precision() == 'bf16'


def test_evaluation_announcements_follow_the_resnet_variable(monkeypatch):
    from gcc_amd import train
    from gcc_amd._lib import GccError
    from gcc_amd.options import options
    opt = options.parse(['--dataroot', './database/cityscapes/', '--model', 'pix2pix'])
    monkeypatch.delenv('GCC_GEN_PRECISION', raising=False)
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'fp32')
    assert train._generator_note(opt) == ''                          # a U-Net run ignores the variable
    for model in ('sagan', 'srgan'):
        opt.model = model
        assert train._generator_note(opt) == ''
    opt.model, opt.backbone = 'pix2pix', 'resnet'
    assert train._generator_note(opt) == '; generator images in fp32'
    opt.model = 'cyclegan'
    assert train._generator_note(opt) == '; generator images in fp32'
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'bf16')
    assert train._generator_note(opt) == ''
    monkeypatch.delenv('GCC_RESNET_PRECISION')
    assert train._generator_note(opt) == ''
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'half')
    with pytest.raises(GccError, match='GCC_RESNET_PRECISION=half'):
        train._generator_note(opt)
    # GCC_GEN_PRECISION=fp32 keeps refusing both, whatever the new variable says
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'fp32')
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')
    with pytest.raises(GccError, match='--model cyclegan'):
        train._generator_note(opt)
    opt.model = 'pix2pix'
    with pytest.raises(GccError, match='--backbone resnet'):
        train._generator_note(opt)
