"""The checks of tests/test_conv_bf16_exact_gpu.py, examined without a GPU (nothing here runs a kernel):

1. every case of the GPU file is on the route it names -- the library's plan functions are host code --, its 'int' data meets
   the exactness condition on the float64 reference alone, an fp32 emulation on the CPU (another summation order than any
   kernel's) gives the expected bits, its 'tiny' data meets the statistics' condition, and its 'normal' data stays inside its
   own per-element bound when the operation is emulated in fp32 (err / bound <= 1);
2. the defect table: six injected defects (tests/_conv_exact.py conv_emul) against the OLD acceptance rule of
   tests/test_kernels_gpu.py (max |got - ref| <= 1.2e-2 max |ref|), the exact check and the per-element bound.

Outcome of the table (printed by test_defect_table, copied to docs/lab_notebook.md).  Every defect runs on a shallow case
(K = 1024, 4 slices) and a deep one (a 1 x 1 layer of K = 8192, 32 slices, no padded tap):
  - the exact check rejects all six on both;
  - the per-element bound rejects all six on the shallow case (no exception had to be listed); on the deep one it still
    rejects the three that change the sum, but round_partials_bf16, truncate and bias_after_round stay inside it: its
    accumulation term K 2^-24 sum |x w| is several bf16 half-ulps of a typical output there.  That is the bound the fp32
    chain allows, and the reason the exact check stands next to it;
  - the old rule accepts round_partials_bf16, truncate and bias_after_round on every row, and drop_last_kstep at K = 8192 on
    data of one sign (activations behind a ReLU against weights with a mean: every output is about K mean(x) mean(w), the lost
    k-step is 64 / 8192 = 0.8 % of it, under the rule's 1.2 %).  On ZERO-mean data at K = 8192 the old rule does reject a lost
    k-step (its error, sigma / 11 per element, is 6 times the limit somewhere in the tensor): the rule looks at the largest
    error, so "most elements stay within it" does not let the defect through there.  Both rows are in the table.

The checks of tests/test_conv_eval_exact_gpu.py (the inference convolutions) are examined the same way in the last section of
this file: routes, exactness and data conditions, the emulation's bits and bound, and the defect table of the two eval
epilogues against the rule of tests/test_unet_infer_gpu.py test_eval_ex_epilogue_against_fp32."""
import pytest
import torch

from gcc_amd import _lib
from tests import _conv_exact as X
from tests._perelem import ACT_LRELU, report, within

ALL = X.FD_CASES + X.WGRAD_CASES
BY_NAME = {c['name']: c for c in ALL}
assert len(BY_NAME) == len(ALL), 'case names must be unique'


@pytest.mark.parametrize('case', X.FD_CASES, ids=[c['name'] for c in X.FD_CASES])
def test_case_is_on_its_intended_route(case):
    with X.forced_options(_lib, case['opts']):
        X.check_expect(case, X.routing(_lib, case))
        if case['stats']:
            # the statistics launch: the same route, tile, halo mode and split, and the rows of the kernel that forms them
            X.check_stats_expect(case, X.routing(_lib, case, with_stats=True))


@pytest.mark.parametrize('case', X.WGRAD_CASES, ids=[c['name'] for c in X.WGRAD_CASES])
def test_weight_gradient_case_has_its_intended_splits(case):
    with X.forced_options(_lib, case['opts']):
        ws, splits = X.wgrad_splits(_lib, case)
    assert ws > 0
    if case['expect']['splits'] is not None:
        assert splits == case['expect']['splits'], (case['name'], splits)


def _emulate(case, d, S):
    op, g = case['op'], case['g']
    if op == 'F':
        return X.conv_emul(d, g, case['bias'], case['act'], S=S)
    return X.emul_plain(op, d, g, case['bias'], case['act'])


@pytest.mark.parametrize('case', ALL, ids=[c['name'] for c in ALL])
def test_case_meets_the_exactness_condition_and_its_own_bound(case):
    op, g = case['op'], case['g']
    seed = X.case_seed(case)
    with X.forced_options(_lib, case['opts']):
        S = X.routing(_lib, case)['S'] if op != 'W' else 0
    K = X.k_products(g, op)
    if op == 'W':
        K, S = X.wgrad_counts(case)
    # exact data: the condition on the reference alone, then the emulation's bits
    d = X.make_data('int', g, seed)
    ref, _, mag = X.reference(op, d, g, case['bias'], case['act'])
    X.assert_exact_condition(mag, case['name'])
    want = ref if op == 'W' else X.expected_bits(ref).double()
    assert torch.equal(_emulate(case, d, S), want), 'an fp32 sum in another order must give the same bits'
    # statistics: the rounded outputs are the outputs, the sums are exact
    if case['stats']:
        t = X.make_data('tiny', g, seed + 1)
        yt = X.reference(op, t, g)[0]
        _, same = X.stats_reference(yt)
        assert same, 'tiny data: every output equals its bf16 rounding'
        # ... and the 'int' data of the convention test: exact sums of rounded outputs that differ from the unrounded sums
        conv = [X.rounded_sum_reference(X.reference(op, X.make_data('int', g, seed, xmax=m), g)[0]) for m in (3, 1)]
        assert any(ok and differs for _, ok, differs in conv), case['name']
    # normal data: the emulation inside the bound
    n = X.make_data('normal', g, seed + 2)
    ref, _, mag = X.reference(op, n, g, case['bias'], case['act'])
    bound = X.bound_wgrad(mag, K, S) if op == 'W' else X.bound_out(ref, mag, K, S, case['act'])
    worst = within(_emulate(case, n, S), ref, bound, case['name'])
    report('emul', (case['name'],), worst=worst)
    assert worst <= 1.0


# ---- the defect table ------------------------------------------------------------------------------------------------------------
def _one_sign(d):
    """the same data with one sign: activations behind a ReLU, weights with a mean"""
    return dict(d, x=d['x'].abs(), w=d['w'].abs())


# (defect, case, data variant): every defect on a shallow case (K = 1024, 4 slices) and on a deep one (K = 8192, 32 slices)
SHALLOW, DEEP = 't128x128-F', 'splitk-1x1-F'
TABLE = tuple((d, c, 'zero-mean') for d in X.DEFECTS for c in (SHALLOW, DEEP)) + (('drop_last_kstep', DEEP, 'one-sign'),)
# defects that provably stay inside the per-element bound on every case: none -- each is rejected on at least one row.  (On the
# DEEP rows the bound's accumulation term, K 2^-24 sum |x w|, is several bf16 half-ulps of a typical output and hides the
# rounding defects there; that is what the bound is, and why the exact check stands next to it.)
WITHIN_BOUND = ()
OLD_RULE_BLIND = ('drop_last_kstep', 'round_partials_bf16', 'truncate')      # the old rule must accept each on at least one row


def _defect_row(defect, name, variant):
    case = BY_NAME[name]
    g, bias, act = case['g'], True, ACT_LRELU
    with X.forced_options(_lib, case['opts']):
        S = max(2, X.routing(_lib, dict(case, ws=True))['S'])          # the split form of the case (defects of a fold need slices)
    K = X.k_products(g, 'F')
    seed = X.case_seed(case)
    # the new exact check
    d = X.make_data('int', g, seed)
    ref, _, mag = X.ref_fprop(d, g, bias, act)
    X.assert_exact_condition(mag, name)
    exact_fails = not torch.equal(X.conv_emul(d, g, bias, act, S=S, defect=defect), X.expected_bits(ref).double())
    # the old rule and the per-element bound on normal data
    n = X.make_data('normal', g, seed + 2)
    if variant == 'one-sign':
        n = _one_sign(n)
    ref, _, mag = X.ref_fprop(n, g, bias, act)
    got = X.conv_emul(n, g, bias, act, S=S, defect=defect)
    ref32 = X.act_fn(torch.nn.functional.conv2d(n['x'].float(), n['w'].float(), n['bias_y'].float(), stride=g[6], padding=g[7]), act, X.SLOPE)
    old_ok, old_ratio = X.old_rule(got.float(), ref32)
    bound = X.bound_out(ref, mag, K, S, act)
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    assert X.old_rule(X.conv_emul(n, g, bias, act, S=S).float(), ref32)[0] and within(X.conv_emul(n, g, bias, act, S=S), ref, bound, name) <= 1.0
    return dict(defect=defect, case=name, variant=variant, K=K, S=S, exact_fails=exact_fails, old_ok=old_ok, old_ratio=old_ratio,
                bound_ratio=ratio, over=float((err > bound).double().mean()))


def test_defect_table():
    rows = [_defect_row(d, c, v) for d, c, v in TABLE]
    for r in rows:
        print('DEFECT %-20s %-13s %-9s K %5d S %2d | exact check %s | old rule %s (err / limit %.3g) | bound %s (worst err / bound %.3g, '
              '%.2g of the elements over)' % (r['defect'], r['case'], r['variant'], r['K'], r['S'], 'FAILS' if r['exact_fails'] else 'passes',
                                              'passes' if r['old_ok'] else 'FAILS', r['old_ratio'], 'FAILS' if r['bound_ratio'] > 1 else 'passes',
                                              r['bound_ratio'], r['over']))
    for r in rows:
        assert r['exact_fails'], 'the exact check must reject %s on %s' % (r['defect'], r['case'])
    for name in X.DEFECTS:
        mine = [r for r in rows if r['defect'] == name]
        assert any(r['bound_ratio'] > 1.0 for r in mine) == (name not in WITHIN_BOUND), name
        if name in OLD_RULE_BLIND:
            assert any(r['old_ok'] for r in mine), 'the old rule was expected to accept %s somewhere' % name
    deep = [r for r in rows if r['defect'] == 'drop_last_kstep' and r['K'] >= 8192]
    assert any(r['old_ok'] for r in deep), 'a lost k-step at K >= 8192 gets past the old rule'


def test_halo_legs_table_of_the_one_shape_tests():
    """the table tests/test_kernels_gpu.py asserts on its IGEMM_HALO = 2 leg is what the library's host code says (no kernel runs)"""
    import ctypes as C
    from gcc_amd import ops
    lib = _lib.load()
    with X.forced_options(_lib, dict(IGEMM_HALO=2)):
        for (N, H, W, Ci, Co, s), legs in X.HALO_LEGS.items():
            for hc, want in zip((0, 128), legs):
                ops.set_plan(halo_hc=hc)
                try:
                    d = ops.conv_desc(N, H, W, Ci, Co, 4, s, 1, X.ceil8(Ci), X.ceil8(Co))
                    got = (int(lib.gcc_conv_halo_mode(C.byref(d), 0, 1)), int(lib.gcc_conv_halo_mode(C.byref(d), 1, 0)))
                finally:
                    ops.set_plan()
                assert got == want, ((N, H, W, Ci, Co, s), hc, got)
    assert lib.gcc_conv_halo_mode(None, 0, 0) == 0


# ---- the eval-mode convolutions (tests/test_conv_eval_exact_gpu.py), examined without a GPU ------------------------------------
# 1. every case is on the route, tile and K-slice count its row names (host code), its 'int' data meets the exactness condition
#    and the two data conditions on the reference alone, the fp32 emulation gives the expected bits for every variant that has
#    exact bits, and on 'normal' data the emulation stays inside bound_eval;
# 2. the defect table of the two eval epilogues (tests/_conv_exact.py eval_emul): every named defect changes bits of the exact
#    check's expectation; the rule of tests/test_unet_infer_gpu.py test_eval_ex_epilogue_against_fp32 accepts act2_from_act and
#    round_before_residual (asserted) and whatever else the table prints.
EVAL_IDS = [c['name'] for c in X.EVAL_CASES]


def _exact_variant(v):
    """has the variant exact bits on 'int' data?  tanh of a number is no fp32 number: that output is held per element"""
    return v['act'] != X.EV_TANH


@pytest.mark.parametrize('case', X.EVAL_CASES, ids=EVAL_IDS)
def test_eval_case_route_conditions_and_own_bound(case):
    g, name = case['g'], case['name']
    with X.forced_options(_lib, case['opts']):
        r = X.eval_routing(_lib, case)
        X.check_eval_expect(case, r)
        if r['need']:
            assert X.eval_routing(_lib, case, ws=False)['route'] == 0, 'without a workspace the call must run un-split'
    seed = X.eval_seed(case)
    K, S = X.eval_k(g), r['S']
    # exact data: the condition and the data conditions on the reference alone, then the emulation's bits
    d = X.make_eval_data('int', g, seed)
    conv = X.eval_conv(d, g)
    top = X.assert_eval_exact_condition(d, conv, name, residual=case['entry'] == 'eval')
    differ, neg = X.assert_eval_data_conditions(X.eval_z(d, conv)[0], name)
    print('DATA %s route %d tile %d K-slices %d | 2^20 / worst magnitude %.1f | %.0f %% of the outputs differ from their bf16 rounding | '
          '%.0f %% negative pre-activations' % (name, r['route'], r['tile'], S, X.EVAL_LIMIT / top, 100 * differ, 100 * neg))
    parts = X.eval_emul_parts(d, g, max(S, 2))
    for v in case['variants']:
        ref = X.variant_reference(case, d, v, 'int', conv)
        y, y2 = X.variant_emul(case, d, v, 'int', parts=parts)
        if _exact_variant(v):
            assert torch.equal(y, X.eval_expected(ref['y'], g[4])), '%s %s: an fp32 sum in another order must give the same bits' % (name, X.variant_id(v))
        if ref['y2'] is not None and v['act2'] != X.EV_TANH:
            assert torch.equal(y2, X.eval_expected(ref['y2'], g[4])), '%s %s: y2' % (name, X.variant_id(v))
    # normal data: the emulation inside the bound
    n = X.make_eval_data('normal', g, seed + 2)
    conv = X.eval_conv(n, g)
    parts = X.eval_emul_parts(n, g, max(S, 2))
    worst = 0.0
    for v in case['variants']:
        ref = X.variant_reference(case, n, v, 'normal', conv)
        y, y2 = X.variant_emul(case, n, v, 'normal', parts=parts)
        worst = max(worst, within(y[:, :g[4]], ref['y'], X.bound_eval(ref['y'], ref['mag'], K, max(S, 2), v['act'], ref['res']), name + ' ' + X.variant_id(v)))
        if ref['y2'] is not None:
            worst = max(worst, within(y2[:, :g[4]], ref['y2'], X.bound_eval(ref['y2'], ref['mag'], K, max(S, 2), v['act2']), name + ' y2 ' + X.variant_id(v)))
    report('eval-emul', (name,), worst=worst)


# the small exact case of each entry the defects run on: 4 K slices, 13 output channels (three pad lanes), a residual, the negative
# slope.  act2_from_act needs (LRELU, RELU) with the NEGATIVE slope: relu(lrelu(z)) = relu(z) for a positive one.
DEFECT_G = (1, 6, 7, 128, 13, 3, 3, 1, 1, False)
DEFECT_CASE = dict(eval=dict(name='defect-eval', entry='eval', g=DEFECT_G),
                   ex=dict(name='defect-ex', entry='ex', g=DEFECT_G))
DEFECT_VARIANT = dict(eval=dict(act=X.EV_PRELU, slope_i=1, residual=True, scale=True, shift=True),
                      ex=dict(act=X.EV_LRELU, act2=X.EV_RELU, slope_i=1, y2='same', scale=True, shift=True))
# the old test's own variant of the second output: (LRELU, RELU) with its slope 0.2 -- index 0 of NORMAL_SLOPES
OLD_EX_VARIANT = dict(act=X.EV_LRELU, act2=X.EV_RELU, slope_i=0, y2='same', scale=True, shift=True)
OLD_RULE_MUST_ACCEPT = ('act2_from_act', 'round_before_residual')
DEFECT_ROWS = [(df, e) for df in X.EVAL_DEFECTS for e in X.DEFECT_ENTRIES.get(df, ('eval', 'ex'))]


def _old_rule_row(case, n, v, defect, S):
    """the old rule on 'normal' data with positive scales (the old test's), on both outputs: (accepted, worst err / limit)"""
    n = dict(n, scale=n['scale'].abs())
    conv = X.eval_conv(n, case['g'])
    ref = X.variant_reference(case, n, v, 'normal', conv)
    y, y2 = X.variant_emul(case, n, v, 'normal', S=S, defect=defect)
    Co = case['g'][4]
    rows = [X.old_rule_eval_ex(y[:, :Co], ref['y'])] + ([X.old_rule_eval_ex(y2[:, :Co], ref['y2'])] if y2 is not None else [])
    return all(ok for ok, _ in rows), max(ratio for _, ratio in rows)


@pytest.mark.parametrize('defect,entry', DEFECT_ROWS, ids=['%s-%s' % r for r in DEFECT_ROWS])
def test_eval_defect_table(defect, entry):
    case, v, S = DEFECT_CASE[entry], DEFECT_VARIANT[entry], 4
    g, Co = case['g'], DEFECT_G[4]
    K = X.eval_k(g)
    # the defect-free emulation meets the exact check ...
    d = X.make_eval_data('int', g, 4242)
    conv = X.eval_conv(d, g)
    X.assert_eval_exact_condition(d, conv, case['name'])
    X.assert_eval_data_conditions(X.eval_z(d, conv)[0], case['name'])
    ref = X.variant_reference(case, d, v, 'int', conv)
    want = [X.eval_expected(ref['y'], Co)] + ([X.eval_expected(ref['y2'], Co)] if ref['y2'] is not None else [])
    good = [t for t in X.variant_emul(case, d, v, 'int', S=S) if t is not None]
    assert all(torch.equal(a, b) for a, b in zip(good, want)), 'the defect-free emulation must give the expected bits'
    # ... and bound_eval on normal data
    n = X.make_eval_data('normal', g, 4243)
    nconv = X.eval_conv(n, g)
    nref = X.variant_reference(case, n, v, 'normal', nconv)
    ny, ny2 = X.variant_emul(case, n, v, 'normal', S=S)
    assert within(ny[:, :Co], nref['y'], X.bound_eval(nref['y'], nref['mag'], K, S, v['act'], nref['res']), 'defect-free y') <= 1.0
    if ny2 is not None:
        assert within(ny2[:, :Co], nref['y2'], X.bound_eval(nref['y2'], nref['mag'], K, S, v['act2']), 'defect-free y2') <= 1.0
    # every defect changes bits of the exact check's expectation
    bad = [t for t in X.variant_emul(case, d, v, 'int', S=S, defect=defect) if t is not None]
    changed = sum(int((a != b).sum()) for a, b in zip(bad, want))
    assert changed > 0, 'the exact check must reject %s on %s' % (defect, entry)
    # the per-element bound on normal data
    by, by2 = X.variant_emul(case, n, v, 'normal', S=S, defect=defect)
    ratio = float(((by[:, :Co] - nref['y']).abs() / X.bound_eval(nref['y'], nref['mag'], K, S, v['act'], nref['res'])).max())
    if by2 is not None:
        ratio = max(ratio, float(((by2[:, :Co] - nref['y2']).abs() / X.bound_eval(nref['y2'], nref['mag'], K, S, v['act2'])).max()))
    if defect == 'pad_lane_gets_shift':
        ratio = float('inf') if float(by[:, Co:].abs().max()) > 0 else ratio          # the pad lanes' bound is zero
    # the old rule: on this test's variant, and for the second output also on the old test's own variant (slope 0.2)
    assert _old_rule_row(case, n, v, None, S)[0], 'the old rule accepts the defect-free emulation'
    old_ok, old_ratio = _old_rule_row(case, n, v, defect, S)
    line = 'EVAL-DEFECT %-22s %-4s | exact check FAILS (%d elements) | bound %s (worst err / bound %.3g) | old rule %s (err / limit %.3g)' % (
        defect, entry, changed, 'FAILS' if ratio > 1 else 'passes', ratio, 'passes' if old_ok else 'FAILS', old_ratio)
    if defect == 'act2_from_act':
        own_ok, own_ratio = _old_rule_row(case, n, OLD_EX_VARIANT, defect, S)
        line += ' | old rule on the old test\'s own (LRELU 0.2, RELU): %s (err / limit %.3g)' % ('passes' if own_ok else 'FAILS', own_ratio)
        old_ok = own_ok
    print(line)
    if defect in OLD_RULE_MUST_ACCEPT:
        assert old_ok, 'the old rule was expected to accept %s' % defect
