"""The checks of tests/test_convbn_exact_gpu.py examined without a GPU (tests/_convbn.py): the restated plan against the library's
own answer (gcc_conv_bn_act_plan runs on the host) and against the regime every case is named for, the conditions on the exact
data, the ambiguous share, the emulation of the three routes under both checks, and the table of named defects -- which of them
each new check rejects and which the whole-tensor bar of test_conv_bn_act_one_call accepts."""
import ctypes as C
import functools
import os

import pytest
import torch

from tests import _convbn as B
from tests import _conv_exact as X

FAKE = 1 << 20                      # a non-NULL, 16-byte aligned pointer the plan query never follows
TAIL_WS_BYTES = 4096 + (4 << 20) + 4096 + (3 << 19)
IDS = [c['name'] for c in B.CASES]


def lib_plan(case, count=16.0, scale=FAKE, what=None, bn_none=False):
    """the library's answer for a case under its options (no GPU: the device's CU count falls back to 256)"""
    from gcc_amd import _lib
    lib = _lib.load()
    d = X.desc(_lib, case['g'], {})
    tail = FAKE if case['tail_ws'] else None
    bn = _lib.bn_t(None, None, B.EPS, B.MOMENTUM, count, None, None, None, None, scale, FAKE, tail, TAIL_WS_BYTES if tail else 0, 1, 0)
    with X.forced_options(_lib, dict(FUSE_BN=case['fuse'], INORM_GRID=case['inorm_grid'])):
        if what is not None:
            return int(lib.gcc_conv_bn_act_plan(C.byref(d), int(case['dgrad']), None if bn_none else C.byref(bn), what))
        from gcc_amd import ops
        return ops.conv_bn_act_plan_of(d, case['dgrad'], bn)


def same_plan(got, want):
    """the restatement leaves launches (and the head shape's split) to the library"""
    return all(got.get(k) == v for k, v in want.items() if v is not None)


@functools.lru_cache(maxsize=None)
def exact(name):
    case = B.BY_NAME[name]
    d = B.make(case, 'exact', B.seeds(case)[0])
    return d, B.exact_ref(d)


@functools.lru_cache(maxsize=None)
def normal(name):
    case = B.BY_NAME[name]
    return B.make(case, 'normal', B.seeds(case)[1])


def restated(case, cus=256, queues=4):
    return B.plan(case['g'], case['dgrad'], case['fuse'], cus, queues, case['tail_ws'], case['inorm_grid'])


def host_plan_args():
    """what the library plans for in this process: the device's CU count (256 without a device) and GPU_MAX_HW_QUEUES (default 4)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    q = int(os.environ.get('GPU_MAX_HW_QUEUES', '0') or 0)
    return cus, (q if q > 0 else 4)


@pytest.mark.parametrize('case', B.CASES, ids=[c['name'] for c in B.CASES])
def test_plan_restatement_and_regime(case):
    got = lib_plan(case)
    assert isinstance(got, dict), got
    want = restated(case, *host_plan_args())
    assert same_plan(got, want), (got, want)
    B.check_regime(case, restated(case))               # the regime on 256 CUs with 4 queues, from the restatement alone
    if host_plan_args() == (256, 4):
        B.check_regime(case, got)
    if got['route'] != 2:
        from gcc_amd import _lib
        assert lib_plan(case, what=_lib.CONVBN_PLAN['S']) == B.BAD_ARG


def test_plan_declines_what_the_call_declines():
    from gcc_amd import _lib
    case = B.BY_NAME['r2-s1']
    R = _lib.CONVBN_PLAN['route']
    assert lib_plan(case, count=0.0, what=R) == B.BAD_ARG
    assert lib_plan(case, scale=None, what=R) == B.BAD_ARG
    assert lib_plan(case, bn_none=True, what=R) == B.BAD_ARG
    assert lib_plan(case, what=99) == B.BAD_ARG and lib_plan(case, what=-1) == B.BAD_ARG
    bad = dict(case, g=(1, 4, 4, 64, 8, 4, 0, 1))
    assert lib_plan(bad, what=R) == B.BAD_ARG
    k_below_stride = dict(case, g=(1, 8, 8, 256, 256, 2, 4, 0), dgrad=True)          # a data gradient whose kernel is smaller than the stride
    assert lib_plan(k_below_stride, what=R) in (B.UNSUPPORTED, 0)


def test_rows_per_lane_reachable():
    """The plan scanned over every split k4 s2 p1 layer of at most 4096 rows (restatement, 256 CUs, 4 queues): rows per lane of the
    grid fold reach 1, 2, 3 and 4 and never 5 -- the `ppt > 4` fallback of gcc_internal_bn_fold_grid cannot be reached on this
    device (blocks = row tiles x channel tiles < 128 for a split and rows > 128 (256 // CG) for ppt > 4 exclude each other), so no
    case is named for it; the scan fails if a retune makes it reachable."""
    seen = set()
    wgs = B.family_wgs()
    for nk in (16, 64, 66, 256):
        for C_ in list(range(8, 2049, 8)):
            for rows in list(range(16, 4097, 16)):
                BP, BC, ntiles, mtiles, max_slices = B.select_tile(rows, C_, 1, nk)
                if BP != 128 or B.plan_ksplit(mtiles * ntiles, nk, max_slices)[0] <= 1:
                    continue
                gp = B.grid_plan(C_, rows, B.GRID_WS_BYTES, wgs)
                if gp is not None:
                    seen.add(gp['rows'] // gp['PL'])
    assert seen == {1, 2, 3, 4}, seen


@pytest.mark.parametrize('name', IDS)
def test_exact_data_conditions(name):
    """on the float64 reference alone: every raw output is its own bf16 rounding, every sum of r and r^2 stays below 2^24, at
    most 1 % of a case's elements have a tie inside the window, the pre-activations differ from their rounding and have both signs,
    the dead channel is dead, one gamma is negative, shift does not cancel"""
    d, ref = exact(name)
    differ, neg = B.data_conditions(d, ref)
    print('DATA %s ambiguous=%.4g differ=%.3g negative=%.3g' % (name, ref['ambiguous'], differ, neg))


ROUTE_CASES = ('r2-tail5', 'r2-tail6', 'r2-g5', 'r2-convT-n3', 'r1-odd54', 'r1-nogrid', 'r0-unsplit-f2', 'r0-split-f2')


@pytest.mark.parametrize('name', ROUTE_CASES)
def test_emulation_passes_both_checks(name):
    case = B.BY_NAME[name]
    pl = restated(case)
    d, ref = exact(name)
    bad = B.exact_faults(ref, B.emulate(d, pl))
    assert not any(bad.values()), bad
    dn = normal(name)
    ratios = B.normal_check(dn, pl, B.emulate(dn, pl), what=name)
    print('EMUL %s %s' % (name, ' '.join('%s=%.3g' % kv for kv in sorted(ratios.items()))))


# raw is its own bf16 rounding on the exact data (the condition that makes it exact): a defect that only changes HOW raw is rounded,
# or takes the statistics in front of the rounding, cannot show there; the per-element check on normal data rejects both
EXACT_BLIND = ('stats_unrounded', 'raw_truncated')


@pytest.mark.parametrize('defect', B.DEFECTS)
def test_named_defects_are_rejected(defect):
    name = B.DEFECT_CASE[defect]
    case = B.BY_NAME[name]
    pl = restated(case)
    d, ref = exact(name)
    acts = dict(zip(('act', 'act2'), B.DEFECT_ACTS.get(defect, (B.ACT_LRELU, B.ACT_RELU))))
    if defect in B.DEFECT_ACTS:
        ref = B.exact_ref(d, **acts)
    good, wrong = B.emulate(d, pl, **acts), B.emulate(d, pl, defect, **acts)
    changed = any(not torch.equal(good[k], wrong[k]) for k in good)
    bad = B.exact_faults(ref, wrong)
    if defect in EXACT_BLIND:
        assert not changed and not any(bad.values())
    else:
        assert changed and any(bad.values()), (defect, bad)
    dn = normal(name)
    got = B.emulate(dn, pl, defect, **acts)
    if defect == 'fp32_mean_sq':       # a mean that is an fp32 number would hide the cast: the seeds of this case avoid it
        for m in (ref['mean'][0], got['raw'][:, 0].sum() / got['raw'].shape[0]):
            assert float(m.float().double()) != float(m)
    B.normal_check(dn, pl, B.emulate(dn, pl, **acts), what=name, **acts)
    with pytest.raises(AssertionError):
        B.normal_check(dn, pl, got, what=defect, **acts)
    print('DEFECT %-20s case %-12s exact: %s  per element: rejected  old bar: %s' % (
        defect, name, 'blind' if defect in EXACT_BLIND else 'rejected (%s)' % ', '.join(k for k, v in bad.items() if v),
        'accepts' if B.old_bar(got, dn, **acts) else 'rejects'))
    assert B.old_bar(B.emulate(dn, pl, **acts), dn, **acts), 'the old bar rejects the emulation without a defect'
