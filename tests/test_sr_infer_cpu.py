"""Host side of the SRGAN inference path: the new ABI structs against the header, the built-in evaluator's selection rule and
the evaluator's module surface (no GPU)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_structs_match_header(tmp_path):
    from gcc_amd import _lib
    pairs = [('gcc_eval_epilogue_t', _lib.eval_epilogue_t, 'workspace_bytes'), ('gcc_bn_eval_item_t', _lib.bn_eval_item_t, 'eps')]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gcc_hip.h"\nint main(void) {\n'
    for cname, _, last in pairs:
        src += '  printf("%s %%zu %%zu\\n", sizeof(%s), offsetof(%s, %s));\n' % (cname, cname, cname, last)
    src += '  printf("acts %d %d %d\\n", GCC_EVAL_ACT_NONE, GCC_EVAL_ACT_PRELU, GCC_EVAL_ACT_TANH);\n'
    src += '  printf("abi %d 0\\n", GCC_HIP_ABI);\n  return 0;\n}\n'
    (tmp_path / 'l.c').write_text(src)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'l.c'), '-o', str(tmp_path / 'l')])
    out = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([str(tmp_path / 'l')], text=True).splitlines()}
    for cname, ct, last in pairs:
        assert ctypes.sizeof(ct) == int(out[cname][0]) and getattr(ct, last).offset == int(out[cname][1]), cname
    assert [int(v) for v in out['acts']] == [_lib.EVAL_ACT_NONE, _lib.EVAL_ACT_PRELU, _lib.EVAL_ACT_TANH]
    assert int(out['abi'][0]) == _lib.GCC_HIP_ABI == 605
    for name in ('gcc_conv_fprop_eval', 'gcc_conv_eval_route', 'gcc_bn_eval_coeffs_group'):
        assert name in _lib.PROTOTYPES


def test_builtin_evaluator_selection(tmp_path):
    import logging
    from gcc_amd import train
    from gcc_amd.metric import sr_eval
    from gcc_amd.options import options
    log = logging.getLogger('sr_eval_test')
    opt = lambda root, model='srgan': options.parse(['--dataroot', str(root), '--model', model])
    assert train.builtin_evaluator(opt('synthetic'), log) is None
    assert train.builtin_evaluator(opt('synthetic:3'), log) is None
    assert train.builtin_evaluator(opt(tmp_path), log) is None                     # no test/ directory
    (tmp_path / 'test' / 'Urban100').mkdir(parents=True)
    (tmp_path / 'test' / 'Set14').mkdir()
    (tmp_path / 'test' / 'other').mkdir()
    assert sr_eval.available_sets(opt(tmp_path)) == ['Set14', 'Urban100']          # the reference's order, known sets only
    assert callable(train.builtin_evaluator(opt(tmp_path), log))
    assert train.builtin_evaluator(opt(tmp_path, 'pix2pix'), log) is None


def test_evaluator_surface():
    from gcc_amd import metric
    from gcc_amd.metric import sr_eval
    assert metric.test_srgan_psnr is sr_eval.test_srgan_psnr
    assert sr_eval.SR_TEST_SETS == ('Set5', 'Set14', 'B100', 'Urban100')
