"""The checks of tests/test_distill_exact_gpu.py examined on the CPU (no GPU, no kernel): the case table's plans against a Python
restatement of plan_splits / select_tile(batch) and against the library's own host code (gcc_distill_plan launches nothing), the
exactness conditions of the 'int' data, a torch emulation of the five kernels that must pass every stage's bound at every case, and
seven wrong variants of it that must each fail at least one stage check at every case where they change anything."""
import pytest
import torch

from tests import _distill as D
from tests._conv_exact import EXACT_LIMIT
from tests._perelem import U24

CASES = D.CASES


@pytest.fixture(scope='module')
def data():
    cache = {}

    def get(case, kind):
        key = (case['name'], kind)
        if key not in cache:
            cache[key] = D.make_data(kind, case)
        return cache[key]
    return get


@pytest.mark.parametrize('case', CASES, ids=D.CASE_IDS)
def test_table_plans_follow_the_restated_plan_functions(case):
    """a changed PLAN_WGRAD_WGS, TP, RED_BLOCKS or tile rule shows here as a named difference"""
    plan = D.plan_py(case['N'], case['C'], case['HW'])
    D.check_plan(case, plan, 'the Python restatement')
    print(D.route_line(case, plan))


@pytest.mark.parametrize('case', CASES, ids=D.CASE_IDS)
def test_library_plan_query_agrees(case):
    """gcc_distill_plan (the dispatch's own functions) against the table and, field by field, against the restatement"""
    from gcc_amd import _lib, ops
    plan = ops.distill_plan(case['N'], case['C'], case['HW'])
    D.check_plan(case, plan, 'gcc_distill_plan')
    mine = D.plan_py(case['N'], case['C'], case['HW'])
    assert set(plan) == set(_lib.DISTILL_PLAN) == set(mine)
    for k in _lib.DISTILL_PLAN:
        assert plan[k] == mine[k], '%s: gcc_distill_plan says %s = %d, the restatement %d' % (case['name'], k, plan[k], mine[k])
    assert plan['ws_bytes'] == ops.distill_workspace_bytes(case['N'], case['C'], case['HW'])


def test_plan_query_refusals():
    from gcc_amd import ops
    for N, C, HW in ((0, 8, 64), (2, 0, 64), (2, 8, 0), (2, 12, 64), (-1, 8, 64), (2, 7, 64)):
        assert ops.distill_plan(N, C, HW) == -1, (N, C, HW)
    assert ops.lib().gcc_distill_plan(2, 8, 64, None) == -1


def test_table_reaches_every_form():
    """the forms the issue lists: every fold kind, every BC, ragged and full tiles, odd batch, batch 1, windows"""
    e = [c['expect'] for c in CASES]
    assert {x['gram_fold'] for x in e} == {0, 1, 2}
    assert {x['bwd_bc'] for x in e} == {16, 32, 64, 128}
    assert any(x['gram_splits'] > 8 for x in e) and any(1 < x['gram_splits'] <= 8 for x in e)
    assert any(x['gram_col_tiles'] > 1 for x in e) and any(x['bwd_ntiles'] > 1 for x in e)
    assert any(c['N'] == 1 for c in CASES) and any(c['N'] % 2 == 1 and c['N'] > 1 for c in CASES)
    assert any(c['win'] for c in CASES) and any(c['HW'] % 128 for c in CASES) and any(c['HW'] % 128 == 0 for c in CASES)
    assert sum(D.pow2(c['C'] * c['HW']) for c in CASES) >= 6


@pytest.mark.parametrize('case', CASES, ids=D.CASE_IDS)
def test_int_data_conditions(case, data):
    """on the data alone: bf16-exact values, Gram magnitudes below 2^24, images that differ; where C HW is a power of two the
    stage-4 condition with the exact S"""
    d = data(case, 'int')
    D.assert_images_differ(d)
    D.assert_images_differ(data(case, 'normal'))
    for x in (d['f'], d['t']):
        assert float(D.gram64(x)[1].max()) < EXACT_LIMIT
    if D.pow2(case['C'] * case['HW']):
        chw = case['C'] * case['HW']
        Sx = ((D.gram64(d['f'])[0] - D.gram64(d['t'])[0]) / chw).float().bfloat16().double()
        assert torch.equal(Sx * chw, (Sx * chw).round())
        assert float(torch.bmm(d['f'].abs(), Sx.abs()).max()) * chw < EXACT_LIMIT


@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('case', CASES, ids=D.CASE_IDS)
def test_emulation_passes_every_stage(case, kind, squared, data):
    d = data(case, kind)
    r = D.emulate(case, d, squared, D.plan_py(case['N'], case['C'], case['HW']))
    ratios = D.run_stages(case, d, kind, r, squared)
    print('RATIO distill-emul %s %s squared=%d %s' % (case['name'], kind, squared, ' '.join('%s=%.3g' % kv for kv in sorted(ratios.items()))))
    assert all(v <= 1.0 for v in ratios.values())


@pytest.mark.parametrize('wrong', D.WRONG)
@pytest.mark.parametrize('case', CASES, ids=D.CASE_IDS)
def test_wrong_variants_fail(case, wrong, data):
    d = data(case, 'normal')
    plan = D.plan_py(case['N'], case['C'], case['HW'])
    applied = 0
    for squared in (False, True):
        if not D.wrong_applies(wrong, case, squared):
            continue
        applied += 1
        bad = D.failing_stages(case, d, 'normal', D.emulate(case, d, squared, plan, wrong=wrong), squared)
        print('%s %s squared=%d: fails %s' % (case['name'], wrong, squared, bad))
        assert bad, '%s: the variant %s (squared=%d) passes every stage check' % (case['name'], wrong, squared)
    if not applied:
        assert not any(D.wrong_applies(wrong, case, s) for s in (False, True))


def test_wrong_variants_apply_somewhere():
    for wrong in D.WRONG:
        n = sum(D.wrong_applies(wrong, c, s) for c in CASES for s in (False, True))
        assert n >= 4, (wrong, n)


def test_depth_counts():
    """the chain counts behind stage 3, at the table's extremes, against the launch arithmetic of misc.hip worked by hand"""
    # 3 x 8 x 8 = 192 entries: one block, one trip; finalize: one partial per thread at most
    assert D.gram_depth(3, 8) == (7, 1 + 10 + 1 + 10)
    # 256 x 256 = 65536 entries: 64 blocks of 256 threads, 4 trips
    assert D.gram_depth(1, 256) == (7, 4 + 10 + 1 + 10)
    # 8192 x 32 pieces = 262144: 256 blocks, 4 trips of 8 channels
    assert D.content_depth(1, 256, 8192) == (3, 32 + 10 + 1 + 10)
    # 2 x 4700 pieces = 9400: 10 blocks, 4 trips
    assert D.content_depth(2, 8, 4700) == (3, 32 + 10 + 1 + 10)
    assert D.scalar_rel_bound(7, 22, True) < 31 * U24 and D.scalar_rel_bound(7, 22, False) < 18 * U24
