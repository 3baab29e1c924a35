"""gcc_dw_inorm_fwd without a GPU: the plan restatement of tests/_dwin.py against the regime every case is named for, the
conditions under which the exact-integer data give a result known to the bit, the cap on the ambiguous share, the per-element
bound, and the defect table -- every named defect of the kernel emulation must change bits under the exact check on the case
built for it; the table also records which ones the per-element bound sees and which ones the old whole-tensor bar
(tests/test_resnet_infer_gpu.py test_dw_inorm_against_fp32: max 3e-2, mean 4e-3) accepts."""
import functools

import pytest
import torch

from tests import _dwin as D

CASE_IDS = ['x'.join(map(str, c)) for c, _, _ in D.CASES]


def test_constants_match_the_kernel_source():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'gcc_amd', 'csrc', 'norm_act.hip')).read()
    hdr = open(os.path.join(root, 'include', 'gcc_hip.h')).read()
    assert int(re.search(r'DWIN_LDS_DOUBLES = (\d+);', src).group(1)) == D.LDS_DOUBLES
    assert int(re.search(r'DWIN_CHG = (\d+);', src).group(1)) == D.CHG
    assert 'DWIN_TAP_DOUBLES = 9 * DWIN_CHG * 8 / 2;' in src and '(DWIN_LDS_DOUBLES - DWIN_TAP_DOUBLES) * 8;' in src
    assert int(re.search(r'INORM_WS_HEADER = (\d+);', src).group(1)) == D.WS_HEADER
    assert re.search(r'constexpr int PX = (\d+);', src).group(1) == str(D.PX)
    assert '#define GCC_DW_INORM_WORKSPACE_BYTES ((size_t)4096 + ((size_t)3 << 20))' in hdr and D.WS_BYTES == 4096 + (3 << 20)
    assert D.TILE_BYTES == 37824


@pytest.mark.parametrize('case,regime,why', D.CASES, ids=CASE_IDS)
def test_plan_restatement_gives_the_regime_a_case_is_named_for(case, regime, why):
    C, H, W, N = case
    D.check_regime(case, regime, D.plan(C, H, W, N))


def test_declined_cases_and_the_edges_next_to_them():
    for case, why in D.DECLINED:
        assert D.plan(*case) == D.UNSUPPORTED, (case, why)
    # one step inside each edge is served
    assert D.plan(24, 4, 526, 1)['tile'] == 128 and D.plan(8, 4, 1053, 1)['tile'] == 256
    assert isinstance(D.plan(16, 8, 8, 64), dict) and isinstance(D.plan(2048, 4, 4, 1), dict)
    assert D.plan(192, 96, 128, 1)["rows"] == 640
    assert D.plan(16, 8, 8, 1, ws_bytes=4096) == D.WORKSPACE and D.plan(16, 1, 8, 1) == D.UNSUPPORTED
    # fewer workgroups where the process opens more hardware queues, fewer CUs
    assert D.family_wgs(256, 4) == 256 and D.family_wgs(256, 8) == 128 and D.family_wgs(304, 2) == 256 and D.family_wgs(64, 4) == 64


@functools.lru_cache(maxsize=2)
def _exact(case):
    return D.exact_inputs(case, D.exact_seed(case))


@functools.lru_cache(maxsize=2)
def _normal(case):
    return D.normal_inputs(case, D.normal_seed(case))


@pytest.mark.parametrize('case,regime,why', D.CASES, ids=CASE_IDS)
def test_exactness_conditions_and_ambiguous_share(case, regime, why):
    """exact_ref asserts the conditions (mean of p exactly 0, u an integer far from a tie, d an exact fp32 value, every fp32 sum
    below 2^24); the ambiguous share is capped at 1 %"""
    C, H, W, N = case
    pl = D.plan(C, H, W, N)
    dat = _exact(case)
    assert bool((dat['r'].abs() <= 3).all()) and bool((dat['w'][1:].abs() <= 2).all()) and not dat['w'][D.special_channels(C)[1]].any()
    for mode in D.MODES:
        ref = D.exact_ref(mode, dat, pl)
        assert ref['ambiguous'] <= 0.01, (case, mode, ref['ambiguous'])
        print('EXACT %s %s ambiguous=%.3g largest_fp32_sum=%.3g' % ('x'.join(map(str, case)), D.MODE_NAME[mode], ref['ambiguous'], ref['big']))
        if mode != D.PLAIN:
            assert bool((ref['u'][:, :, D.special_channels(C)[1]].abs() <= 4).all())


@pytest.mark.parametrize('case,regime,why', D.CASES, ids=CASE_IDS)
def test_bound_is_finite_and_positive(case, regime, why):
    C, H, W, N = case
    pl = D.plan(C, H, W, N)
    dat = _normal(case)
    for mode in D.MODES:
        ref = D.normal_ref(mode, dat, pl)
        for name in ('y', 'u') if mode == D.RESIDUAL else ('y',):
            v, b = ref[name]
            assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(b).all()), (case, mode, name)
            live = v != 0
            assert bool((b[live] > 0).all()), (case, mode, name)
            # a bound of a few bf16 roundings, not a tolerance: the median stays below four half-ulps of the value
            assert float((b[live] / v[live].abs()).median()) < 4 * D.BF16, (case, mode, name, float((b[live] / v[live].abs()).median()))


# ---- the defect table ------------------------------------------------------------------------------------------------------------
# defect -> (the case whose plan it is built for, channels emulated under that plan, mode)
NARROW = 16
BUILT_FOR = {
    'halo_top': ((40, 33, 17, 2), 40, D.RESIDUAL),            # S = 3: workgroup 1 starts inside the plane
    'halo_bottom': ((40, 33, 17, 2), 40, D.RESIDUAL),
    'reflect_col': ((17, 5, 7, 3), 17, D.RESIDUAL),
    'reflect_row': ((17, 5, 7, 3), 17, D.RESIDUAL),
    'keep_lo': ((256, 8, 300, 4), NARROW, D.RESIDUAL),        # two tiles per sweep
    'p1_unclipped': ((40, 33, 17, 2), 40, D.RESIDUAL),        # last workgroup 49 of 256 rows
    'u_unrounded': ((256, 64, 64, 1), NARROW, D.RESIDUAL),    # an even plane: rstd_p = 0.999995, r + p rstd_p is not a bf16 number
    'unbiased': ((256, 64, 64, 1), NARROW, D.NORM_RELU),     # HW = 4096: rstd off by 1.2e-4, far below the old bar
    'eps_dropped': ((17, 5, 7, 3), 17, D.NORM_RELU),          # the channel with taps * 2^-9: var(d) of the order of eps
    'own_rows': ((40, 33, 17, 2), 40, D.NORM_RELU),
    'second_reads_first': ((40, 33, 17, 2), 40, D.NORM_RELU),
    'uout_last': ((17, 5, 7, 3), 17, D.RESIDUAL),
    'pad_u': ((17, 5, 7, 3), 17, D.RESIDUAL),
    'bias': ((17, 5, 7, 3), 17, D.RESIDUAL),
}


def _run(dat, mode, pl, defect, exact):
    C, H, W, N = dat['case']
    x = dat['u'] if (exact and mode == D.PLAIN) else (dat['p'] if exact else dat['x'])
    return D.emulate(mode, x, dat['r'], dat['w'], dat['eps'], H, W, pl, defect)


def test_defect_table():
    assert set(BUILT_FOR) == set(D.DEFECTS)
    rows = []
    clean_done = set()
    for defect in D.DEFECTS:
        case, Cn, mode = BUILT_FOR[defect]
        pl = D.plan(*case)
        narrow = (Cn,) + case[1:]
        ex, nd = D.exact_inputs(narrow, 41 + sum(case)), D.normal_inputs(narrow, 43 + sum(case))
        eref = D.exact_ref(mode, ex, pl)
        if (case, mode) not in clean_done:
            # the emulation without a defect passes every check the GPU file applies to the kernel
            clean_done.add((case, mode))
            y, u, pad = _run(ex, mode, pl, None, True)
            assert D.exact_faults(eref, y, u if mode == D.RESIDUAL else None) == (0, 0) and pad == 0.0, (case, mode)
            y, u, pad = _run(nd, mode, pl, None, False)
            ratios = D.normal_check(mode, nd, pl, y, u if mode == D.RESIDUAL else None, 'emulation %r' % (case,))
            assert D.old_bar(y, D.normal_ref(mode, nd, pl)['y'][0])[0]
            print('CLEAN %s %s %s' % ('x'.join(map(str, case)), D.MODE_NAME[mode], ' '.join('%s=%.3g' % kv for kv in sorted(ratios.items()))))
        y, u, pad = _run(ex, mode, pl, defect, True)
        bad_y, bad_u = D.exact_faults(eref, y, u if mode == D.RESIDUAL else None)
        exact_sees = bad_y + bad_u > 0 or pad != 0.0
        y, u, pad = _run(nd, mode, pl, defect, False)
        try:
            D.normal_check(mode, nd, pl, y, u if mode == D.RESIDUAL else None)
            bound_sees = pad != 0.0
        except AssertionError:
            bound_sees = True
        ok, mx, mean = D.old_bar(y, D.normal_ref(mode, nd, pl)['y'][0])
        rows.append((defect, exact_sees, bound_sees, ok, mx, mean))
        print('DEFECT %-18s on %-12s %-9s exact: %d y + %d u_out elements wrong%s | per-element bound %s | old bar %s (max %.2g mean %.2g)'
              % (defect, 'x'.join(map(str, case)), D.MODE_NAME[mode], bad_y, bad_u, ', pad lanes' if pad else '',
                 'sees it' if bound_sees else 'blind', 'accepts' if ok else 'rejects', mx, mean))
    missed = [r[0] for r in rows if not r[1]]
    assert not missed, 'defects that change no bit under the exact check: %r' % missed
    # what the table is for: the old bar lets real defects through that the new checks catch
    accepted = {r[0] for r in rows if r[3]}
    assert {'u_unrounded', 'unbiased', 'uout_last', 'pad_u'} <= accepted, accepted
    assert all(r[2] for r in rows), 'the per-element check (bound, layout, dead channels) misses %r' % [r[0] for r in rows if not r[2]]
