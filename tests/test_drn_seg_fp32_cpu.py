"""Host-only checks of the fp32 evaluator route: GCC_DRN_PRECISION in cityscapes.builtin_segmenter (which needs no device), the
precision argument of DrnSegEngine, and the ctypes mirror of gcc_eval_f32_epilogue_t."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _drn_emul as E


@pytest.fixture(scope='module')
def opt(tmp_path_factory):
    """a Cityscapes root as builtin_segmenter tests for it (table.txt) and the reference's kind of --drn_path file"""
    d = tmp_path_factory.mktemp('cityscapes')
    (d / 'table.txt').write_text('')
    z = np.load(E.GOLDEN)
    torch.save(E.fixture_net(z, 'bneck')[0], str(d / 'drn.pth'))
    return SimpleNamespace(dataroot=str(d), drn_path=str(d / 'drn.pth'))


def test_unset_variable_gives_the_bf16_engine(opt, monkeypatch):
    from gcc_amd.metric import cityscapes as CS
    from gcc_amd.metric.drn_seg import DrnSegEngine
    monkeypatch.delenv('GCC_DRN_PRECISION', raising=False)
    seg, why = CS.builtin_segmenter(opt)
    assert isinstance(seg, DrnSegEngine) and why is None and seg.precision == 'bf16'
    monkeypatch.setenv('GCC_DRN_PRECISION', 'bf16')
    assert CS.builtin_segmenter(opt)[0].precision == 'bf16'


def test_fp32_variable_gives_the_fp32_engine(opt, monkeypatch):
    from gcc_amd.metric import cityscapes as CS
    monkeypatch.setenv('GCC_DRN_PRECISION', 'fp32')
    seg, why = CS.builtin_segmenter(opt)
    assert why is None and seg.precision == 'fp32' and seg.device is None       # still on the host
    assert seg.flops(256, 256) > 0


def test_any_other_value_is_an_error_naming_it(opt, monkeypatch):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import cityscapes as CS
    from gcc_amd.metric.drn_seg import DrnSegEngine
    monkeypatch.setenv('GCC_DRN_PRECISION', 'fp16')
    with pytest.raises(GccError, match='GCC_DRN_PRECISION=fp16'):
        CS.builtin_segmenter(opt)
    sd = torch.load(opt.drn_path, map_location='cpu', weights_only=True)
    with pytest.raises(GccError, match='fp64'):
        DrnSegEngine(sd, precision='fp64')
    with pytest.raises(GccError, match='GPU only'):
        DrnSegEngine(sd, precision='fp32').to('cpu')


def test_epilogue_struct_mirror():
    """gcc_eval_f32_epilogue_t: three pointers and four ints, as include/gcc_hip.h lays them out"""
    from gcc_amd import _lib
    t = _lib.eval_f32_epilogue_t
    assert C.sizeof(t) == 40
    assert [(n, getattr(t, n).offset) for n, _ in t._fields_] == [('scale', 0), ('shift', 8), ('residual', 16), ('ld_residual', 24),
                                                                  ('residual_off', 28), ('act', 32), ('dilation', 36)]
    L = _lib.load()
    assert L.gcc_conv_eval_f32_kp(3, 7, 7) == 208 and L.gcc_conv_eval_f32_kp(8, 3, 3) == 80 and L.gcc_conv_eval_f32_kp(64, 1, 1) == 64
    d = _lib.conv_t(1, 32, 32, 512, 512, 3, 3, 1, 4, 512, 0, 512, 0)
    assert L.gcc_conv_eval_f32_route(C.byref(d), 4) == 1          # 1024 pixels: 64 x 64 tiles
    d.N = 64
    assert L.gcc_conv_eval_f32_route(C.byref(d), 4) == 0          # 65536 pixels x 512 channels fill the chip with 128 x 128 tiles
    assert L.gcc_conv_eval_f32_route(C.byref(d), 2) == -2         # pad 4 is not dilation 2's
