"""The host side of the SAGAN generator's fp32 inference route: GCC_SAGAN_PRECISION (models/SAGAN.py sagan_precision), what the
training announcement says, the declarations of the two new kernels, and the bound of tests/_attn_f64.py vouched for on the CPU
-- an fp32 torch evaluation of Self_Attn lies inside it on every element, a float64 evaluation with q, k or v rounded to bf16
violates it on more than half of them."""
import os
import re

import pytest
import torch

from tests import _attn_f64 as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sagan_precision_reads_the_variable(monkeypatch):
    from gcc_amd._lib import GccError
    from gcc_amd.models.SAGAN import SAGAN_PRECISION_ENV, sagan_precision
    assert SAGAN_PRECISION_ENV == 'GCC_SAGAN_PRECISION'
    monkeypatch.delenv('GCC_SAGAN_PRECISION', raising=False)
    assert sagan_precision() == 'bf16'
    monkeypatch.setenv('GCC_SAGAN_PRECISION', '')
    assert sagan_precision() == 'bf16'
    for value in ('bf16', 'fp32'):
        monkeypatch.setenv('GCC_SAGAN_PRECISION', value)
        assert sagan_precision() == value
    monkeypatch.setenv('GCC_SAGAN_PRECISION', 'fp16')
    with pytest.raises(GccError, match='GCC_SAGAN_PRECISION=fp16'):
        sagan_precision()
    # the other generators' variables are not its business
    monkeypatch.setenv('GCC_SAGAN_PRECISION', 'bf16')
    monkeypatch.setenv('GCC_RESNET_PRECISION', 'fp32')
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')
    assert sagan_precision() == 'bf16'


def test_generator_note_for_sagan(monkeypatch):
    from gcc_amd import train
    from gcc_amd._lib import GccError
    from gcc_amd.options import options
    opt = options.parse(['--dataroot', './database/celeb/', '--model', 'sagan'])
    for name in ('GCC_GEN_PRECISION', 'GCC_RESNET_PRECISION', 'GCC_SAGAN_PRECISION'):
        monkeypatch.delenv(name, raising=False)
    assert train._generator_note(opt) == ''
    monkeypatch.setenv('GCC_SAGAN_PRECISION', 'fp32')
    assert train._generator_note(opt) == '; generator images in fp32'
    for model in ('pix2pix', 'cyclegan', 'srgan'):                  # nobody else reads it
        opt.model = model
        assert train._generator_note(opt) == ''
    opt.model = 'sagan'
    monkeypatch.setenv('GCC_SAGAN_PRECISION', 'bf16')
    assert train._generator_note(opt) == ''
    monkeypatch.setenv('GCC_SAGAN_PRECISION', 'single')
    with pytest.raises(GccError, match='GCC_SAGAN_PRECISION=single'):
        train._generator_note(opt)
    # GCC_GEN_PRECISION=fp32 keeps refusing the model, whatever the new variable says
    monkeypatch.setenv('GCC_SAGAN_PRECISION', 'fp32')
    monkeypatch.setenv('GCC_GEN_PRECISION', 'fp32')
    with pytest.raises(GccError, match='--model sagan'):
        train._generator_note(opt)


def test_new_symbols_are_declared_and_mirrored():
    from gcc_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'gcc_hip.h')).read()
    names = ('gcc_attention_infer_f32', 'gcc_attention_infer_f32_route', 'gcc_conv_eval_f32_z4', 'gcc_conv_eval_f32_z4_route',
             'gcc_conv_eval_f32_z4_kp')
    source = open(os.path.join(ROOT, 'gcc_amd', '_lib.py')).read()
    for name in names:
        m = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert m, name
        assert re.search(r"'%s': \(_I, \[([^\]]*)\]\)" % name, source), name
        mirrored = re.search(r"'%s': \(_I, \[([^\]]*)\]\)" % name, source).group(1)
        assert len(mirrored.split(',')) == len(m.group(1).split(',')), name
    assert re.search(r'#define GCC_HIP_ABI 605\b', header)           # additions only: no bump
    assert 'sagan_f32' in open(os.path.join(ROOT, 'gcc_amd', 'csrc', 'build.sh')).read()
    for fn in ('attention_infer_f32', 'conv_eval_f32_z4', 'pack_weights_f32_z4'):
        assert callable(getattr(ops, fn))


CPU_CASES = [(1, 16, 2, 16), (1, 8, 1, 32), (2, 24, 3, 32), (2, 48, 6, 9), (1, 64, 8, 32)]


@pytest.mark.parametrize('B,C,C8,H', CPU_CASES)
def test_fp32_torch_lies_inside_the_bound(B, C, C8, H):
    q, k, v, x = A.normal_case(B, C, C8, H, seed=C + H)
    for gamma in (0.5, -0.7):
        y, bound = A.reference_and_bound(q, k, v, x, gamma)
        err = (A.torch_fp32(q, k, v, x, gamma).double() - y).abs()
        worst = float((err / bound).max())
        print('fp32 torch Self_Attn %s gamma %g: worst err / bound %.3g' % ((B, C, C8, H), gamma, worst))
        assert bool((err <= bound).all()), worst


@pytest.mark.parametrize('B,C,C8,H', CPU_CASES)
def test_one_bf16_operand_violates_the_bound(B, C, C8, H):
    q, k, v, x = A.normal_case(B, C, C8, H, seed=C + H)
    y, bound = A.reference_and_bound(q, k, v, x, 0.5)
    rb = lambda t: t.bfloat16().float()
    for name, args in (('q', (rb(q), k, v)), ('k', (q, rb(k), v)), ('v', (q, k, rb(v)))):
        err = (A.reference(*args, x, 0.5) - y).abs()
        share = float((err > bound).double().mean())
        print('%s rounded to bf16 %s: %.3f of the elements outside the bound' % (name, (B, C, C8, H), share))
        assert share > 0.5, (name, share)
