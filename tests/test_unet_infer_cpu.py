"""Host side of the U-Net inference path and `python -m gcc_amd.test`: the new ABI structs against the header, the reference's
result-file names and per-model test options, the missing-checkpoint error (no GPU)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_ex_structs_match_header(tmp_path):
    from gcc_amd import _lib
    ct = _lib.eval_ex_epilogue_t
    fields = ['scale', 'shift', 'y2', 'ldy2', 'y2off', 'act', 'act2', 'slope', 'workspace', 'workspace_bytes']
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gcc_hip.h"\nint main(void) {\n'
    src += '  printf("size %zu\\n", sizeof(gcc_eval_ex_epilogue_t));\n'
    for f in fields:
        src += '  printf("%s %%zu\\n", offsetof(gcc_eval_ex_epilogue_t, %s));\n' % (f, f)
    src += '  printf("acts %d %d %d %d %d\\n", GCC_EVAL_ACT_NONE, GCC_EVAL_ACT_PRELU, GCC_EVAL_ACT_TANH, GCC_EVAL_ACT_RELU, ' \
           'GCC_EVAL_ACT_LRELU);\n'
    src += '  printf("abi %d\\n", GCC_HIP_ABI);\n  return 0;\n}\n'
    (tmp_path / 'l.c').write_text(src)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'l.c'), '-o', str(tmp_path / 'l')])
    out = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([str(tmp_path / 'l')], text=True).splitlines()}
    assert ctypes.sizeof(ct) == int(out['size'][0])
    for f in fields:
        assert getattr(ct, f).offset == int(out[f][0]), f
    assert [int(v) for v in out['acts']] == [_lib.EVAL_ACT_NONE, _lib.EVAL_ACT_PRELU, _lib.EVAL_ACT_TANH,
                                             _lib.EVAL_ACT_RELU, _lib.EVAL_ACT_LRELU]
    assert int(out['abi'][0]) == _lib.GCC_HIP_ABI == 605
    for name in ('gcc_conv_eval_ex', 'gcc_conv_eval_ex_workspace', 'gcc_conv_eval_ex_route', 'gcc_image_to_u8'):
        assert name in _lib.PROTOTYPES


def test_result_names_follow_the_reference():
    from gcc_amd.test import result_names
    paths = [['/data/val/a/1_A.jpg'], ['/data/val/b/7_B.png']]
    assert result_names(['real_A', 'fake_B', 'real_B'], paths, 'AtoB') == [
        ('real_A', '7_B.png'), ('fake_B', os.path.join('fake_B', '1_A_fake_B.png'))]
    # BtoA: set_input stored [B paths, A paths]; imageA is then taken from the second entry
    assert result_names(['real_A', 'fake_B'], paths, 'BtoA') == [
        ('real_A', '1_A.png'), ('fake_B', os.path.join('fake_B', '7_B_fake_B.png'))]
    assert result_names(['fake_A'], paths, 'AtoB') == [('fake_A', os.path.join('fake_A', '7_B_fake_A.png'))]
    # srgan (lr / hr names), sagan (one path twice)
    assert result_names(['real_lr', 'fake_hr', 'real_hr'], [['x/baby.png'], ['y/baby.png']]) == [
        ('fake_hr', os.path.join('fake_hr', 'baby_fake_hr.png'))]
    assert result_names(['fake_img', 'real_img'], [['c\\d\\img.3.png'], ['c\\d\\img.3.png']]) == [
        ('fake_img', os.path.join('fake_img', 'img_fake_img.png')), ('real_img', 'img.png')]


def test_per_model_overrides():
    from gcc_amd.options import options
    from gcc_amd.test import model_kwargs, test_overrides
    o = test_overrides(options.parse(['--model', 'pix2pix', '--batch_size', '4', '--load_size', '286']))
    assert (o.phase, o.batch_size, o.serial_batches, o.no_flip, o.load_size, o.num_threads) == ('val', 1, True, True, 256, 0)
    o = test_overrides(options.parse(['--model', 'cyclegan']))
    assert (o.phase, o.batch_size, o.no_flip, o.load_size) == ('test', 1, True, 256)
    o = test_overrides(options.parse(['--model', 'sagan']))
    assert (o.batch_size, o.serial_batches, o.load_size) == (1, True, 64)
    assert model_kwargs('pix2pix', ([1, 2], [3])) == {'filter_cfgs': [1, 2], 'channel_cfgs': [3]}
    assert model_kwargs('pix2pix', None) == {'filter_cfgs': None, 'channel_cfgs': None}
    assert model_kwargs('cyclegan', ([1], [2])) == {'cfg_AtoB': [1], 'cfg_BtoA': [2]}
    assert model_kwargs('srgan', ([5], None)) == {'filter_cfgs': [5]}


def test_missing_checkpoint_raises(tmp_path):
    from gcc_amd import test as gtest
    with pytest.raises(FileNotFoundError):
        gtest.main(['--model', 'pix2pix', '--dataroot', str(tmp_path), '--checkpoints_dir', str(tmp_path),
                    '--pretrain_path', str(tmp_path / 'missing.pth')])
    with pytest.raises(FileNotFoundError):
        gtest.main(['--model', 'pix2pix', '--dataroot', str(tmp_path), '--checkpoints_dir', str(tmp_path)])
