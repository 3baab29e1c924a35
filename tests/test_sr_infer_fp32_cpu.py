"""Host side of SRGAN's fp32 inference route: the GCC_SR_PRECISION parsing, the new ABI struct against the header, and the float64
restatement (tests/_srresnet_f64.py) held to the reference-written fixture, so the yardstick of the GPU test is checked where
there is no GPU."""
import ctypes
import os
import subprocess

import pytest
import torch

from tests import _srresnet_f64 as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_BAR = 2e-8           # the reference's own fp32 image against float64 (1.33e-8 where the fixture was measured)


def test_precision_variable(monkeypatch):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import sr_eval
    assert sr_eval.PRECISION_ENV == 'GCC_SR_PRECISION' and sr_eval.PRECISIONS == ('bf16', 'fp32')
    monkeypatch.delenv('GCC_SR_PRECISION', raising=False)
    assert sr_eval.sr_precision() == 'bf16'
    monkeypatch.setenv('GCC_SR_PRECISION', '')
    assert sr_eval.sr_precision() == 'bf16'
    for v in ('bf16', 'fp32'):
        monkeypatch.setenv('GCC_SR_PRECISION', v)
        assert sr_eval.sr_precision() == v
    for bad in ('fp16', 'FP32', 'float32', '1'):
        monkeypatch.setenv('GCC_SR_PRECISION', bad)
        with pytest.raises(GccError, match='GCC_SR_PRECISION=%s' % bad):
            sr_eval.sr_precision()


def test_the_variable_is_read_in_one_place():
    hits = []
    for folder, _, files in os.walk(os.path.join(ROOT, 'gcc_amd')):
        for f in files:
            if f.endswith('.py'):
                text = open(os.path.join(folder, f)).read()
                if "'GCC_SR_PRECISION'" in text or '"GCC_SR_PRECISION"' in text:
                    hits.append(f)
    assert hits == ['sr_eval.py'], hits


def test_act_epilogue_struct_matches_header(tmp_path):
    from gcc_amd import _lib
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gcc_hip.h"\nint main(void) {\n'
    src += '  typedef gcc_eval_f32_act_epilogue_t T;\n  printf("%zu", sizeof(T));\n'
    fields = [n for n, _ in _lib.eval_f32_act_epilogue_t._fields_]
    for f in fields:
        src += '  printf(" %%zu", offsetof(T, %s));\n' % f
    src += '  printf("\\n%d %d %d %d %d\\n", GCC_EVAL_ACT_NONE, GCC_EVAL_ACT_RELU, GCC_EVAL_ACT_PRELU, GCC_EVAL_ACT_TANH, GCC_HIP_ABI);\n'
    src += '  return 0;\n}\n'
    (tmp_path / 'l.c').write_text(src)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'l.c'), '-o', str(tmp_path / 'l')])
    sizes, consts = subprocess.check_output([str(tmp_path / 'l')], text=True).splitlines()
    sizes = [int(v) for v in sizes.split()]
    ct = _lib.eval_f32_act_epilogue_t
    assert sizes[0] == ctypes.sizeof(ct)
    assert sizes[1:] == [getattr(ct, f).offset for f in fields]
    assert [int(v) for v in consts.split()] == [_lib.EVAL_ACT_NONE, _lib.EVAL_ACT_RELU, _lib.EVAL_ACT_PRELU, _lib.EVAL_ACT_TANH, 605]
    for name in ('gcc_conv_eval_f32_act', 'gcc_conv_eval_f32_act_route', 'gcc_nhwc_f32_to_nchw_f32', 'gcc_image_to_u8_f32'):
        assert name in _lib.PROTOTYPES


def test_float64_restatement_against_the_reference_image():
    sd, lr, fake_hr = S.load_fixture()
    with torch.no_grad():
        f64 = S.forward(sd, lr)
    assert f64.dtype == torch.float64 and tuple(f64.shape) == (2, 3, 48, 48)
    err = float((fake_hr.double() - f64).abs().max())
    print('reference fake_hr against float64: %.3g (image magnitude %.3g)' % (err, float(f64.abs().max())))
    assert err <= FIXTURE_BAR, err
    # the restatement with one bf16 rounding per layer is two orders of magnitude further away: the yardstick tells the routes apart
    with torch.no_grad():
        emul = S.forward(sd, lr, round_bf16=True)
    assert float((emul - f64).abs().max()) > 100 * err
