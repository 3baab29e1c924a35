"""Host side of the MobileResnet inference path (no GPU): gcc_dw_inorm_t and its constants against the header, the bindings."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dw_inorm_struct_matches_header(tmp_path):
    from gcc_amd import _lib
    ct = _lib.dw_inorm_t
    fields = [n for n, _ in ct._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gcc_hip.h"\nint main(void) {\n'
    src += '  printf("size %zu\\n", sizeof(gcc_dw_inorm_t));\n'
    for f in fields:
        src += '  printf("%s %%zu\\n", offsetof(gcc_dw_inorm_t, %s));\n' % (f, f)
    src += '  printf("modes %d %d %d\\n", GCC_DWIN_PLAIN, GCC_DWIN_NORM_RELU, GCC_DWIN_RESIDUAL);\n'
    src += '  printf("ws %zu\\n", GCC_DW_INORM_WORKSPACE_BYTES);\n'
    src += '  printf("plan %d %d %d %d %d %d %d %d\\n", GCC_DWIN_PLAN_S, GCC_DWIN_PLAN_S1, GCC_DWIN_PLAN_G, GCC_DWIN_PLAN_ROWS, '
    src += 'GCC_DWIN_PLAN_CG, GCC_DWIN_PLAN_CHG, GCC_DWIN_PLAN_PL, GCC_DWIN_PLAN_TILE);\n'
    src += '  printf("convbn %d %d %d %d %d %d %d %d %d %d %d\\n", GCC_CONVBN_PLAN_ROUTE, GCC_CONVBN_PLAN_KSPLIT, GCC_CONVBN_PLAN_LAUNCHES, '
    src += 'GCC_CONVBN_PLAN_S, GCC_CONVBN_PLAN_S1, GCC_CONVBN_PLAN_G, GCC_CONVBN_PLAN_ROWS, GCC_CONVBN_PLAN_CG, GCC_CONVBN_PLAN_CHG, '
    src += 'GCC_CONVBN_PLAN_PL, GCC_CONVBN_PLAN_PPT);\n'
    src += '  printf("abi %d\\n", GCC_HIP_ABI);\n  return 0;\n}\n'
    (tmp_path / 'l.c').write_text(src)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'l.c'), '-o', str(tmp_path / 'l')])
    out = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([str(tmp_path / 'l')], text=True).splitlines()}
    assert ctypes.sizeof(ct) == int(out['size'][0])
    for f in fields:
        assert getattr(ct, f).offset == int(out[f][0]), f
    assert [int(v) for v in out['modes']] == [_lib.DWIN_PLAIN, _lib.DWIN_NORM_RELU, _lib.DWIN_RESIDUAL]
    assert int(out['ws'][0]) == _lib.DW_INORM_WORKSPACE_BYTES
    assert [int(v) for v in out['plan']] == [_lib.DWIN_PLAN[k] for k in ('S', 'S1', 'G', 'rows', 'CG', 'CHg', 'PL', 'tile')]
    assert [int(v) for v in out['convbn']] == [_lib.CONVBN_PLAN[k] for k in ('route', 'ksplit', 'launches') + _lib.CONVBN_PLAN_GRID]
    assert int(out['abi'][0]) == _lib.GCC_HIP_ABI


def test_dw_inorm_entry_points_are_bound():
    from gcc_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gcc_hip.h')).read()
    for name in ('gcc_dw_inorm_fwd', 'gcc_dw_inorm_route', 'gcc_dw_inorm_plan'):
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert name in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.gcc_version() == _lib.GCC_HIP_ABI
    # the library rejects a descriptor without pointers before it looks at any device
    d = _lib.dw_inorm_t()
    assert lib.gcc_dw_inorm_route(ctypes.byref(d)) == -1
    assert lib.gcc_dw_inorm_route(None) == -1
    assert lib.gcc_dw_inorm_plan(ctypes.byref(d), _lib.DWIN_PLAN['S']) == -1
    assert lib.gcc_dw_inorm_plan(None, _lib.DWIN_PLAN['tile']) == -1


def test_infer_surfaces_exist():
    from gcc_amd import engine
    from gcc_amd.models.CycleGAN import MobileCycleGANModel
    for name in ('infer', 'infer_input', 'infer_launches'):
        assert callable(getattr(engine.MobileResnetEngine, name))
    for name in ('infer', 'infer_nhwc'):
        assert callable(getattr(MobileCycleGANModel, name))
