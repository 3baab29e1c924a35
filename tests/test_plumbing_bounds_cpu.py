"""The checks of tests/test_plumbing_exact_gpu.py examined without a GPU (tests/_plumbing.py holds both files' cases):

* the case lists reach what they claim: every fold of channel_sum_kernel with both of its loops in one lane and with a lane that
  has no pixel; every edge of the one-launch kernel's loops; the three routes of gcc_nhwc_copy and gcc_nhwc_add (the library's
  own host-side query against the restated rule over the whole sweep) with the group kernel's three forms; ties, -0.0 and a
  denormal in the copy data; pack kinds 0, 1 and 2 with aligned and misaligned masters, from ops.PackPlan itself on CPU tensors;
* an emulation that walks the kernels' own index arithmetic passes the exact check and the bound at every case;
* kernels that are subtly wrong fail them: a dropped last pixel, a lane whose unrolled trip is counted twice, the CHP = 128 fold
  reading red[q * 64 + ch], a copy that zero-fills one lane too many, a packing that leaves its padding unwritten.

Nothing here launches a kernel."""
import numpy as np
import pytest
import torch

from tests import _plumbing as L
from tests._perelem import layout, within
from tests.test_segmented_conv_gpu import packed_definition

FOLDS = ('shuffle', 'rows', 'walk')


def test_two_launch_cases_reach_every_fold_with_both_loops():
    seen = {f: dict(both=0, none=0, tail_only=0, inactive=0) for f in FOLDS}
    for P, C in L.SUM_TWO:
        u, t = L.sum_trips(P, C)
        s = seen[L.fold_of(C)]
        assert int((u * 4 + t).sum()) == P, 'the walk visits every pixel once'
        s['both'] += bool(((u > 0) & (t > 0)).any())
        s['none'] += bool(((u + t) == 0).any())
        s['tail_only'] += bool(not u.any() and t.max() >= 2)
        s['inactive'] += layout(C)[0] < layout(C)[1]
    for f in FOLDS:
        assert all(seen[f].values()), (f, seen[f])
    assert {C for _, C in L.SUM_TWO} == set(L.SUM_C)
    assert {layout(C)[1] for C in L.SUM_C} == {1, 4, 8, 64, 128, 256}
    # every case keeps its tensors near 16 MB and the refused width is the first one past 256 chunks
    assert max(P * L.ceil8(C) * 2 for P, C in L.SUM_TWO) <= 17 << 20
    assert layout(2048)[0] == 256 and layout(L.SUM_C_REFUSED)[0] == 257


def test_one_launch_cases_reach_the_loop_edges():
    trips = {P: L.small_trips(P) for P, _ in L.SUM_ONE}
    assert all(int((u * 4 + t).sum()) == P for P, (u, t) in trips.items())
    assert (trips[511][1] == 0).any() and not trips[511][0].any()                  # a thread without a pixel
    assert (trips[512][1] == 1).all()
    assert trips[513][1].max() == 2
    assert not trips[1536][0].any() and (trips[1536][1] == 3).all()
    assert trips[1537][0].sum() == 1 and trips[1537][1][0] == 0                    # the first unrolled trip, thread 0 alone
    assert (trips[2048][0] == 1).all() and not trips[2048][1].any()
    assert ((trips[2049][0] > 0) & (trips[2049][1] > 0)).sum() == 1                # an unrolled and a tail trip in one thread
    assert (trips[16384][0] == 8).all()
    assert max(P for P, _ in L.SUM_ONE) == L.SMALL_MAX
    assert [C for P, C in L.SUM_ONE].count(520) == 2


def test_group_items():
    assert len(L.GROUP_ITEMS) == L.GROUP_MAX
    assert L.GROUP_ITEMS[0][0] == 3 and L.GROUP_ITEMS[-1][0] == 3
    assert {C for C, _, _ in L.GROUP_ITEMS} == {C for C in L.SUM_C if C <= 520}
    assert {1, 511, 512, 513, 1536, 1537, 2048, 2049, 16384} <= {P for _, P, _ in L.GROUP_ITEMS}
    assert all(1 <= P <= L.SMALL_MAX for _, P, _ in L.GROUP_ITEMS) and {a for _, _, a in L.GROUP_ITEMS} == {0, 1}


def _sum_check(got, x, P, C, small, prior, what):
    ref, bound = L.sum_bound(x, P, C, small, prior)
    return within(got, ref, bound, what)


@pytest.mark.parametrize('C', L.SUM_C)
def test_channel_sum_emulation_passes(C):
    """the kernel's walk in fp32: exact on the integer data (also onto integer presets), inside the bound on the normal data"""
    for P in L.sum_pixels(C):
        xi = L.sum_int(P, C)
        assert torch.equal(L.sum_emul(xi, C).double(), xi.sum(0))
        pr = L.sum_prior(C, True)
        assert torch.equal(L.sum_emul(xi, C, prior=pr).double(), xi.sum(0) + pr.double())
        xn = L.sum_normal(P, C, seed=P + C)
        assert _sum_check(L.sum_emul(xn, C), xn, P, C, False, None, 'emul %dx%d' % (P, C)) <= 1.0
        pr = L.sum_prior(C, False)
        assert _sum_check(L.sum_emul(xn, C, prior=pr), xn, P, C, False, pr, 'emul acc %dx%d' % (P, C)) <= 1.0


@pytest.mark.parametrize('P,C', L.SUM_ONE)
def test_one_launch_emulation_passes(P, C):
    xi = L.sum_int(P, C)
    assert torch.equal(L.sum_emul_small(xi).double(), xi.sum(0))
    xn = L.sum_normal(P, C, seed=P + C)
    pr = L.sum_prior(C, False)
    assert _sum_check(L.sum_emul_small(xn), xn, P, C, True, None, 'small %dx%d' % (P, C)) <= 1.0
    assert _sum_check(L.sum_emul_small(xn, prior=pr), xn, P, C, True, pr, 'small acc %dx%d' % (P, C)) <= 1.0


def _both_cases():
    return [(P, C) for P, C in L.SUM_TWO if ((lambda u, t: ((u > 0) & (t > 0)).any())(*L.sum_trips(P, C)))]


def _faulty_sum_rejected(P, C, fault):
    xi = L.sum_int(P, C)
    assert not torch.equal(L.sum_emul(xi, C, fault=fault).double(), xi.sum(0)), 'exact check passes %s at %dx%d' % (fault, P, C)
    xn = L.sum_normal(P, C, seed=P + C)
    with pytest.raises(AssertionError):
        _sum_check(L.sum_emul(xn, C, fault=fault), xn, P, C, False, None, '%s %dx%d' % (fault, P, C))


@pytest.mark.parametrize('fault', ['drop_last', 'double_trip'])
def test_wrong_walks_are_rejected(fault):
    """at the largest case of every channel count (the one whose lanes take both loops): one pixel of up to 524289 missing, four
    pixels counted twice"""
    cases = _both_cases()
    assert {C for _, C in cases} == set(L.SUM_C)
    for P, C in cases:
        _faulty_sum_rejected(P, C, fault)
    if fault == 'drop_last':
        for P, C in L.SUM_TWO:
            if P > 1:
                _faulty_sum_rejected(P, C, fault)


def test_wrong_fold_stride_is_rejected():
    cases = [(P, C) for P, C in L.SUM_TWO if layout(C)[1] == 128 and P > 1]
    assert {C for _, C in cases} == {520, 1024}
    for P, C in cases:
        _faulty_sum_rejected(P, C, 'fold64')


def test_the_old_tolerance_misses_a_dropped_pixel():
    """the reason for the exact check: tests/test_kernels_gpu.py test_channel_sum allows 1e-4 max|ref| + 2e-3, which a sum of 16384
    pixels without its last one meets"""
    P, C = 16384, 8
    xn = L.sum_normal(P, C, seed=1)
    ref = xn.sum(0)
    bad = xn[:-1].sum(0)
    assert float((bad - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 2e-3
    with pytest.raises(AssertionError):
        within(bad.float(), ref, L.sum_bound(xn, P, C, False)[1], 'dropped pixel')


# ---- copies --------------------------------------------------------------------------------------------------------------------
def test_copy_sweep_reaches_every_route_and_the_query_agrees():
    """the restated rule over the whole sweep: all three routes for copy and add, the group kernel with d0 != 0, with a whole-group
    store and with a fill; where the library is built, its own gcc_nhwc_copy_route says the same at every point and refuses what
    the entries refuse"""
    from gcc_amd import ops
    lib = ops.lib()
    n = 0
    for add in (0, 1):
        routes, facts = set(), np.zeros(3, dtype=bool)
        for lds in L.COPY_LD:
            for ldd in L.COPY_LD:
                for soff, doff, C, Cfill in L.copy_points(lds, ldd, add):
                    r = L.copy_route(lds, soff, ldd, doff, C, Cfill)
                    assert r == lib.gcc_nhwc_copy_route(lds, soff, ldd, doff, C, Cfill), (lds, soff, ldd, doff, C, Cfill)
                    routes.add(r)
                    n += 1
                    if r == L.GROUP:
                        facts |= np.array(L.group_facts(soff, doff, C, Cfill, add))
                    if r == L.VEC:
                        assert not (lds | ldd | soff | doff | C) & 7
                    if (lds | ldd) & 7:
                        assert r == L.SCALAR
        assert routes == {L.VEC, L.GROUP, L.SCALAR}, (add, routes)
        assert tuple(facts) == ((True, False, False) if add else (True, True, True)), (add, facts)
    print('sweep points', n)
    # a slice that straddles an 8-lane group takes the scalar kernel
    assert L.copy_route(16, 6, 16, 0, 3, 3) == L.SCALAR and L.copy_route(16, 0, 16, 6, 3, 3) == L.SCALAR
    for args in ((8, 0, 8, 0, 0, 0), (8, 6, 8, 0, 3, 3), (8, 0, 8, 4, 3, 5), (8, -8, 8, 0, 8, 8), (16, 0, 16, -8, 8, 8), (8, 0, 8, 0, 9, 9)):
        assert L.copy_route(*args) == L.BAD_ARG == lib.gcc_nhwc_copy_route(*args), args
    for route, (lds, soff, ldd, doff, C, Cfill) in L.LARGE_COPY.items():
        assert L.copy_route(lds, soff, ldd, doff, C, Cfill) == route == L.copy_route(lds, soff, ldd, doff, C, C)
    assert L.LARGE_P > L.GRID_CAP * 256


def test_copy_data_has_ties_signed_zero_and_a_denormal():
    src = L.copy_src(L.COPY_PIXELS, 24)
    for lane in range(24):
        assert {0x8000, 0x0001} <= set(int(v) for v in src[:, lane]), lane
    for C in L.COPY_C:
        for soff, doff in ((0, 0), (5, 3), (8, 1)):
            dst = L.copy_dst(L.COPY_PIXELS, 24, doff, C, True)
            assert L.add_ties(src, dst, soff, doff, C) >= 2, (C, soff, doff)
    # both directions of a tie: 1 + 2^-8 -> 1, (1 + 2^-7) + 2^-8 -> 1 + 2^-6
    f = L.bits_to_f32(np.array([0x3F80, 0x3F81], dtype=np.uint16)) + np.float32(2.0 ** -8)
    assert [int(v) for v in L.f32_to_bits(f)] == [0x3F80, 0x3F82]
    t = torch.randn(4096, generator=torch.Generator().manual_seed(0))
    assert np.array_equal(L.f32_to_bits(t.numpy()), L.bf16_bits(t.bfloat16()))


def test_copy_check_rejects_a_fill_one_lane_too_far():
    """the whole destination row is compared, so a zero over the sentinel behind the window shows; against a zeroed buffer (what the
    old test had) it would not"""
    src = L.copy_src(L.COPY_PIXELS, 16)
    n = 0
    for soff, doff, C, Cfill in L.copy_points(16, 16, 0):
        if doff + Cfill < 16:
            dst = L.copy_dst(L.COPY_PIXELS, 16, doff, C, False)
            good = L.copy_ref(src, dst, soff, doff, C, Cfill, False)
            bad = L.copy_ref(src, dst, soff, doff, C, Cfill, False, fault='fill_one_more')
            assert not np.array_equal(good, bad)
            zeroed = np.zeros_like(dst)
            assert np.array_equal(L.copy_ref(src, zeroed, soff, doff, C, Cfill, False)[:, doff + Cfill:],
                                  L.copy_ref(src, zeroed, soff, doff, C, Cfill, False, fault='fill_one_more')[:, doff + Cfill:])
            n += 1
    assert n > 1000


# ---- weight packing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [1, 0])
def test_pack_plan_schedules_the_kinds(fused, monkeypatch):
    """ops.PackPlan on CPU tensors (it only looks at shapes and pointers): kind 2 for an aligned unsplit master whose width is a
    multiple of 4 when FUSED_PACK is on, kinds 0 and 1 for every other master -- every misaligned one among them"""
    from gcc_amd import engine, ops
    monkeypatch.setattr(ops, 'FUSED_PACK', bool(fused))
    seen = set()
    for offset in range(4):
        flat, spans = L.pack_masters(offset, torch.zeros(1))
        assert flat.data_ptr() % 16 == 0
        convs = [engine.ConvOp(L.master_view(flat, start, w), None, w.shape[2], 1, 0, False, row_split=rs, col_split=cs)
                 for (start, w), (_, _, _, rs, cs) in zip(spans, L.PACK_SHAPES)]
        assert all(c.weight.data_ptr() % 16 == (4 * offset) % 16 for c in convs)
        assert all((c.row_split, c.col_split) == s[3:] for c, s in zip(convs, L.PACK_SHAPES))
        items = ops.PackPlan(convs, 'cpu').d_items
        for i, shape in enumerate(L.PACK_SHAPES):
            kinds = set(int(k) for k in items[items[:, 0] == i][:, 1])
            assert kinds == L.pack_kinds(shape, offset, fused), (shape, offset, fused, kinds)
            seen |= {(k, offset == 0) for k in kinds}
            if shape[1] % 4 or offset:
                assert 2 not in kinds
    assert seen == ({(0, True), (1, True), (2, True), (0, False), (1, False)} if fused else {(0, True), (1, True), (0, False), (1, False)})


def test_pack_check_rejects_unwritten_padding():
    """a packing that writes the real elements only: invisible in buffers that start out as zeros (engine.ConvOp's), visible
    against the sentinel"""
    n = 0
    for rows, cols, k, rs, cs in L.PACK_SHAPES:
        w = torch.randn(rows, cols, k, k, generator=torch.Generator().manual_seed(rows)) * 0.1
        W, Wt = packed_definition(w, rs, cs)
        real, _ = packed_definition(torch.ones_like(w), rs, cs)
        real = real != 0
        if bool(real.all()):
            continue
        n += 1
        for start in (0.0, L.SENTINEL):
            lazy = torch.full(W.shape, start, dtype=torch.bfloat16)
            lazy[real] = W[real]
            assert L.same_bf16(lazy, W) == (start == 0.0)
            lazy_t = torch.full(Wt.shape, start, dtype=torch.bfloat16)
            lazy_t[real.permute(2, 1, 0)] = Wt[real.permute(2, 1, 0)]
            assert L.same_bf16(lazy_t, Wt) == (start == 0.0)
    assert n >= 9


def test_pack_shapes_cover_the_tile_edges():
    shapes = {s[:3] for s in L.PACK_SHAPES}
    assert {(64, 64, 1), (65, 64, 3), (64, 68, 3), (1, 8, 4), (130, 4, 7), (3, 64, 4), (200, 12, 1)} <= shapes
    assert {s[1] % 4 for s in L.PACK_SHAPES if not s[3] and not s[4]} == {0, 2}
    assert {(bool(s[3]), bool(s[4])) for s in L.PACK_SHAPES} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(L.ceil8(s[0]) > s[0] and s[0] > 64 for s in L.PACK_SHAPES)            # rowsp > rows inside the last tile
