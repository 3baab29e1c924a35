"""The float64 yardstick of the U-Net's fp32 inference route (tests/_unet_f64.py) held to the reference's own image, and the host
side of GCC_GEN_PRECISION.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import _unet_f64 as U


def _fixture(golden_dir):
    ckpt = torch.load(os.path.join(golden_dir, 'ref_checkpoint_pix2pix.pth'), map_location='cpu', weights_only=False)
    z = np.load(os.path.join(golden_dir, 'ref_checkpoint_pix2pix.npz'))
    return ckpt['G'], torch.from_numpy(z['A']), torch.from_numpy(z['fake_B'])


def test_float64_restatement_reproduces_the_reference_image(golden_dir):
    """max |fake_B - f64| <= 1e-7 (measured 3.2e-8: the reference's own fp32 rounding).  A wrong restatement -- a missed in-place
    aliasing, a BatchNorm too many -- is off by orders of magnitude more."""
    sd, A, fake_B = _fixture(golden_dir)
    assert U.depth(sd) == 6
    f64 = U.unet_eval(sd, A)
    assert f64.dtype == torch.float64 and tuple(f64.shape) == tuple(fake_B.shape)
    err = float((fake_B.double() - f64).abs().max())
    print('reference fake_B from float64: %.3g' % err)
    assert err <= 1e-7


def test_fp32_restatement_is_as_close_as_the_reference(golden_dir):
    sd, A, fake_B = _fixture(golden_dir)
    f64, f32 = U.unet_eval(sd, A), U.unet_eval(sd, A, torch.float32)
    assert f32.dtype == torch.float32
    assert float((f32.double() - f64).abs().max()) <= 1e-6
    pre = U.unet_eval(sd, A, pre_tanh=True)
    assert torch.equal(torch.tanh(pre), f64)


def test_tensor2im_bytes_match_the_cli_host_form():
    from gcc_amd.test import tensor2im_host
    x = torch.rand(2, 3, 5, 7, generator=torch.Generator().manual_seed(0)) * 2 - 1
    assert np.array_equal(U.tensor2im(x)[0].numpy(), tensor2im_host(x))


def test_gen_precision_reads_the_variable(monkeypatch):
    from gcc_amd._lib import GccError
    from gcc_amd.models.Pix2Pix import GEN_PRECISION_ENV, gen_precision
    assert GEN_PRECISION_ENV == 'GCC_GEN_PRECISION'
    monkeypatch.delenv(GEN_PRECISION_ENV, raising=False)
    assert gen_precision() == 'bf16' and gen_precision(only_bf16='--backbone resnet') == 'bf16'
    monkeypatch.setenv(GEN_PRECISION_ENV, 'bf16')
    assert gen_precision() == 'bf16'
    monkeypatch.setenv(GEN_PRECISION_ENV, 'fp32')
    assert gen_precision() == 'fp32'
    with pytest.raises(GccError, match=r'GCC_GEN_PRECISION=fp32.*U-Net only.*--backbone resnet'):
        gen_precision(only_bf16='--backbone resnet')
    monkeypatch.setenv(GEN_PRECISION_ENV, 'fp16')
    with pytest.raises(GccError, match='GCC_GEN_PRECISION=fp16'):
        gen_precision()


def test_evaluation_announcements_name_a_non_default_generator_precision(monkeypatch):
    from gcc_amd import train
    from gcc_amd._lib import GccError
    from gcc_amd.options import options
    opt = options.parse(['--dataroot', './database/cityscapes/', '--model', 'pix2pix'])
    monkeypatch.delenv('GCC_GEN_PRECISION', raising=False)
    assert train._generator_note(opt) == ''
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')
    assert train._generator_note(opt) == '; generator images in fp32'
    opt.backbone = 'resnet'
    with pytest.raises(GccError, match='--backbone resnet'):
        train._generator_note(opt)
    opt.model = 'cyclegan'
    with pytest.raises(GccError, match='--model cyclegan'):
        train._generator_note(opt)
