"""Host side of the SAGAN generator's inference path (no GPU): gcc_sn_eval_item_t against the header, the bindings, the surfaces."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sn_eval_item_struct_matches_header(tmp_path):
    from gcc_amd import _lib
    ct = _lib.sn_eval_item_t
    fields = [n for n, _ in ct._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gcc_hip.h"\nint main(void) {\n'
    src += '  printf("size %zu\\n", sizeof(gcc_sn_eval_item_t));\n'
    for f in fields:
        src += '  printf("%s %%zu\\n", offsetof(gcc_sn_eval_item_t, %s));\n' % (f, f)
    src += '  printf("max %d\\n", GCC_SPECTRAL_GROUP_MAX);\n'
    src += '  printf("abi %d\\n", GCC_HIP_ABI);\n  return 0;\n}\n'
    (tmp_path / 'l.c').write_text(src)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'l.c'), '-o', str(tmp_path / 'l')])
    out = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([str(tmp_path / 'l')], text=True).splitlines()}
    assert ctypes.sizeof(ct) == int(out['size'][0])
    for f in fields:
        assert getattr(ct, f).offset == int(out[f][0]), f
    assert int(out['max'][0]) == _lib.SPECTRAL_GROUP_MAX
    assert int(out['abi'][0]) == _lib.GCC_HIP_ABI == 605


def test_sagan_infer_entry_points_are_bound():
    from gcc_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gcc_hip.h')).read()
    for name in ('gcc_attention_infer', 'gcc_attention_infer_route', 'gcc_spectral_eval_coeffs_group'):
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert name in _lib.PROTOTYPES
    for name in ('gcc_attention_infer_workspace', 'gcc_spectral_eval_coeffs_workspace'):
        assert re.search(r'\bsize_t\s+%s\s*\(' % name, hdr), name
        assert name in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.gcc_version() == _lib.GCC_HIP_ABI
    # geometry checks answer before any device is looked at
    assert lib.gcc_attention_infer_route(1, 1025, 64, 8, 0) == -2
    assert lib.gcc_attention_infer_route(1, 1024, 513, 8, 0) == -2
    assert lib.gcc_attention_infer_route(1, 1024, 64, 0, 0) == -2
    assert lib.gcc_attention_infer_route(1, 1024, 64, 65, 0) == -2
    assert lib.gcc_attention_infer_route(1, 256, 16, 17, 0) == -2
    assert lib.gcc_attention_infer_route(1, 1024, 64, 8, 0) == 1          # no workspace: never split
    assert lib.gcc_attention_infer_route(64, 1024, 64, 8, 1 << 30) == 1    # a full grid is not split
    need = lib.gcc_attention_infer_workspace(1, 1024, 64, 8)
    assert need > 0
    assert lib.gcc_attention_infer_route(1, 1024, 64, 8, need) == 2
    assert lib.gcc_attention_infer_route(1, 1024, 64, 8, need - 1) == 1
    assert lib.gcc_attention_infer_workspace(64, 1024, 64, 8) == 0
    assert lib.gcc_attention_infer(None, 8, 0, 8, 16, None, 8, None, 1, 64, 8, 1, None, 8, None, 0, None) == -1
    assert lib.gcc_spectral_eval_coeffs_group(None, 1, None, 0, None) == -1
    assert lib.gcc_spectral_eval_coeffs_workspace(None, 1) == 0


def test_sagan_infer_surfaces_exist():
    from gcc_amd import engine, ops
    from gcc_amd.models.SAGAN import SAGANModel
    for name in ('infer', 'infer_input', 'infer_launches'):
        assert callable(getattr(engine.SaganGeneratorEngine, name))
    for name in ('infer', 'infer_nhwc'):
        assert callable(getattr(SAGANModel, name))
    for name in ('attention_infer', 'spectral_eval_coeffs_group', 'spectral_eval_items'):
        assert callable(getattr(ops, name))
