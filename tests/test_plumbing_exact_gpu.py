"""The small kernels between the convolutions, each against its definition: gcc_channel_sum and gcc_channel_sum_group (every conv
bias gradient), gcc_nhwc_copy / gcc_nhwc_add / gcc_nhwc_pack_pair and the NCHW <-> NHWC conversions (every input, skip connection,
concatenation and residual), gcc_pack_weights / gcc_pack_weights_multi (the bf16 weights every conv reads), gcc_gate_mask.

Every test asserts the route it took (launch counts, the workspace formula, gcc_nhwc_copy_route, the kinds of a pack plan) before
it compares a number, and prints a ROUTE line.  Everything is compared bit for bit except the channel sums of normal data, which
are held per element to the bound derived in tests/_plumbing.py (RATIO lines: worst err / bound).  Every output buffer starts out
as 7.0, and whatever lies outside the written window must still hold it.  Refusals are checked by return code, launch count and
untouched sentinels only.  Cases, references and emulations: tests/_plumbing.py; the checks themselves are examined in
tests/test_plumbing_bounds_cpu.py."""
import numpy as np
import pytest
import torch

from tests import _plumbing as L
from tests._perelem import bwd_blocks, report, within
from tests.test_kernels_gpu import DEV, _ops
from tests.test_misc_kernels_gpu import SPECIAL
from tests.test_segmented_conv_gpu import packed_definition

pytestmark = pytest.mark.gpu


def _route(name, case, what):
    print('ROUTE %s %s %s' % (name, 'x'.join(map(str, case)), what))


class _small_route:
    """GCC_OPT_BN_BWD_SMALL for the duration of a block: 0 the two-launch channel sum, 1 the one-launch kernel up to 16384 pixels"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from gcc_amd import _lib
        self.prev = _ops().lib().gcc_set_option(_lib.OPT_BN_BWD_SMALL, int(self.on))

    def __exit__(self, *exc):
        from gcc_amd import _lib
        _ops().lib().gcc_set_option(_lib.OPT_BN_BWD_SMALL, self.prev)
        return False


def _sentinel(n, dtype=torch.float32):
    return torch.full((n,), L.SENTINEL, dtype=dtype, device=DEV)


def _untouched(t, what):
    assert bool((t == L.SENTINEL).all()), what + ': a sentinel was overwritten'


def _chansum(x, C_, P, ld, off, fill, prior=None, ws_short=0):
    """one gcc_channel_sum call on x [P, C] in a [P, ld] buffer at lane off: (rc, launches, out[:C] on the CPU)"""
    ops = _ops()
    lib = ops.lib()
    buf = L.sum_buffer(x, C_, ld, off, fill).to(DEV)
    assert buf.data_ptr() % 16 == 0
    need = int(lib.gcc_channel_sum_workspace(C_, P))
    ws = _sentinel(need // 4 + 16)
    out = _sentinel(C_ + 8)
    if prior is not None:
        out[:C_] = prior.to(DEV)
    lib.gcc_launch_count(1)
    rc = lib.gcc_channel_sum(buf.data_ptr(), ld, off, C_, P, out.data_ptr(), int(prior is not None), ws.data_ptr(), need - ws_short, ops.stream())
    launches = int(lib.gcc_launch_count(1))
    torch.cuda.synchronize()
    _untouched(out[C_:], 'out behind channel %d' % C_)
    _untouched(ws[need // 4:], 'workspace behind its %d bytes' % need)
    if rc != 0:
        _untouched(out if prior is None else out[C_:], 'out of a refused call')
        _untouched(ws, 'workspace of a refused call')
    return rc, launches, out[:C_].cpu(), need


def _sum_case(P, C_, small):
    """the three checks of a channel-sum case on the route the option selects"""
    C8 = L.ceil8(C_)
    name = 'chansum_one' if small else 'chansum_two'
    xi, xn = L.sum_int(P, C_), L.sum_normal(P, C_, seed=P + C_)
    with _small_route(small):
        # route: the workspace formula, a workspace one byte short, the launch count
        rc, launches, _, need = _chansum(xi, C_, P, C8, 0, 0.0, ws_short=1)
        assert need == bwd_blocks(P, C_) * C8 * 4
        assert (rc, launches) == (L.ERR_WORKSPACE, 0)
        rc, launches, got, _ = _chansum(xi, C_, P, C8, 0, 0.0)
        assert (rc, launches) == (0, 1 if small else 2), (rc, launches)
        u, t = L.small_trips(P) if small else L.sum_trips(P, C_)
        _route(name, (P, C_), '%s launches=%d blocks=%d unrolled<=%d tail<=%d idle_lanes=%d' % (
            'small' if small else L.fold_of(C_), launches, 1 if small else bwd_blocks(P, C_), u.max(), t.max(), int(((u + t) == 0).sum())))
        # 1. exact
        assert torch.equal(got.double(), xi.sum(0)), 'integer sums'
        pr = L.sum_prior(C_, True)
        rc, _, got, _ = _chansum(xi, C_, P, C8, 0, 0.0, prior=pr)
        assert rc == 0 and torch.equal(got.double(), xi.sum(0) + pr.double()), 'integer sums onto integer presets'
        # 2. per element against float64
        rc, _, tight, _ = _chansum(xn, C_, P, C8, 0, 0.0)
        ref, bound = L.sum_bound(xn, P, C_, small)
        r0 = within(tight, ref, bound, '%s %dx%d' % (name, P, C_))
        pr = L.sum_prior(C_, False)
        rc, _, got, _ = _chansum(xn, C_, P, C8, 0, 0.0, prior=pr)
        ref, bound = L.sum_bound(xn, P, C_, small, pr)
        r1 = within(got, ref, bound, '%s accumulate %dx%d' % (name, P, C_))
        report(name, (P, C_), sum=r0, accumulate=r1, chain=L.sum_chain(P, C_, small)[0])
        # 3. window: large finite values in the pad lanes of the last group and in every lane outside the window
        rc, launches, wide, _ = _chansum(xn, C_, P, C8 + 16, 8, L.GARBAGE)
        assert (rc, launches) == (0, 1 if small else 2)
        assert torch.equal(wide.view(torch.int32), tight.view(torch.int32)), 'window at lane 8 of ld %d' % (C8 + 16)
        rc, _, wide, _ = _chansum(xi, C_, P, C8 + 16, 8, L.GARBAGE)
        assert rc == 0 and torch.equal(wide.double(), xi.sum(0)), 'integer sums in the window'


@pytest.mark.parametrize('P,C_', L.SUM_TWO, ids=lambda v: str(v))
def test_channel_sum_two_launch(P, C_):
    _sum_case(P, C_, small=False)


@pytest.mark.parametrize('P,C_', L.SUM_ONE, ids=lambda v: str(v))
def test_channel_sum_one_launch(P, C_):
    _sum_case(P, C_, small=True)


@pytest.mark.parametrize('small', [0, 1])
def test_channel_sum_refuses_more_than_256_chunks(small):
    lib = _ops().lib()
    C_, P = L.SUM_C_REFUSED, 4
    assert lib.gcc_channel_sum_workspace(C_, P) == 0
    with _small_route(small):
        rc, launches, _, _ = _chansum(L.sum_int(P, C_), C_, P, L.ceil8(C_), 0, 0.0)
    assert (rc, launches) == (L.UNSUPPORTED, 0)
    _route('chansum_refused', (P, C_), 'GCC_ERR_UNSUPPORTED launches=0')


def _group_call(items):
    from gcc_amd import _lib
    ops = _ops()
    arr = (_lib.chansum_item_t * len(items))()
    for it, (x, ld, off, C_, P, out, acc) in zip(arr, items):
        it.x, it.ld, it.off, it.C, it.pixels, it.out, it.accumulate = x.data_ptr(), ld, off, C_, P, out.data_ptr(), acc
    lib = ops.lib()
    lib.gcc_launch_count(1)
    rc = lib.gcc_channel_sum_group(arr, len(items), ops.stream())
    launches = int(lib.gcc_launch_count(1))
    torch.cuda.synchronize()
    return rc, launches


def test_channel_sum_group():
    """24 items of mixed width, size and accumulate flag in one launch: every entry has the bits of its own gcc_channel_sum call
    (the one-launch kernel, held to float64 in test_channel_sum_one_launch) and sits inside the same bound"""
    assert len(L.GROUP_ITEMS) == L.GROUP_MAX
    items, single, refs = [], [], []
    with _small_route(1):
        for i, (C_, P, acc) in enumerate(L.GROUP_ITEMS):
            xn = L.sum_normal(P, C_, seed=100 + i)
            pr = L.sum_prior(C_, False) if acc else None
            ld, off = (L.ceil8(C_) + 16, 8) if i % 3 == 1 else (L.ceil8(C_), 0)
            buf = L.sum_buffer(xn, C_, ld, off, L.GARBAGE if off else 0.0).to(DEV)
            out = _sentinel(C_ + 8)
            if acc:
                out[:C_] = pr.to(DEV)
            items.append((buf, ld, off, C_, P, out, acc))
            rc, launches, got, _ = _chansum(xn, C_, P, ld, off, L.GARBAGE if off else 0.0, prior=pr)
            assert (rc, launches) == (0, 1)
            single.append(got)
            refs.append(L.sum_bound(xn, P, C_, True, pr))
        rc, launches = _group_call(items)
    assert (rc, launches) == (0, 1)
    _route('chansum_group', (len(items),), 'launches=1 workgroups=%d' % sum(L.ceil8(c) // 8 for c, _, _ in L.GROUP_ITEMS))
    worst = 0.0
    for i, ((buf, ld, off, C_, P, out, acc), one, (ref, bound)) in enumerate(zip(items, single, refs)):
        _untouched(out[C_:], 'item %d: out behind channel %d' % (i, C_))
        got = out[:C_].cpu()
        assert torch.equal(got.view(torch.int32), one.view(torch.int32)), 'item %d (C %d, %d pixels, accumulate %d)' % (i, C_, P, acc)
        worst = max(worst, within(got, ref, bound, 'group item %d' % i))
    report('chansum_group', (len(items),), worst=worst)


def test_channel_sum_group_refusals():
    """n = 25, an item of more than 16384 pixels, a misaligned ld: return code only, nothing launched, nothing written.  (Every
    buffer is as large as its item says.)"""
    P = L.SMALL_MAX + 1
    buf = torch.ones(P * 16 + 8, dtype=torch.bfloat16, device=DEV)
    outs = [_sentinel(16) for _ in range(L.GROUP_MAX + 1)]
    ok = lambda i: (buf, 8, 0, 3, 5, outs[i], 0)
    for what, items, want in (('n = 25', [ok(i) for i in range(L.GROUP_MAX + 1)], L.BAD_ARG),
                              ('16385 pixels', [ok(0), (buf, 8, 0, 3, P, outs[1], 0), ok(2)], L.UNSUPPORTED),
                              ('ld 12', [ok(0), ok(1), (buf, 12, 0, 3, 5, outs[2], 0)], L.BAD_ARG),
                              ('off 4', [(buf, 16, 4, 3, 5, outs[0], 0)], L.BAD_ARG)):
        rc, launches = _group_call(items)
        assert (rc, launches) == (want, 0), what
        for o in outs:
            _untouched(o, what)
    _route('chansum_group_refused', (4,), 'launches=0')


@pytest.mark.parametrize('C_', [1, 255, 256, 257])
def test_gate_mask(C_):
    """alpha exactly tau, one ulp above, one ulp below: 0.5, 1, 0"""
    ops = _ops()
    tau = np.float32(0.3)
    vals = np.array([tau, np.nextafter(tau, np.float32(1)), np.nextafter(tau, np.float32(0))], dtype=np.float32)
    want = np.array([0.5, 1.0, 0.0], dtype=np.float32)
    idx = (np.arange(C_) * 2 + np.arange(C_) // 3) % 3
    alpha = torch.from_numpy(vals[idx]).to(DEV)
    mask = _sentinel(C_ + 8)
    lib = ops.lib()
    lib.gcc_launch_count(1)
    rc = lib.gcc_gate_mask(alpha.data_ptr(), float(tau), mask.data_ptr(), C_, ops.stream())
    launches = int(lib.gcc_launch_count(1))
    torch.cuda.synchronize()
    assert (rc, launches) == (0, 1)
    _route('gate_mask', (C_,), 'launches=1 workgroups=%d' % ((C_ + 255) // 256))
    assert torch.equal(mask[:C_].cpu(), torch.from_numpy(want[idx]))
    _untouched(mask[C_:], 'mask behind channel %d' % C_)


# ---- gcc_nhwc_copy / gcc_nhwc_add ---------------------------------------------------------------------------------------------
def _as_dev(bits):
    """uint16 numpy array -> device tensor of the same bits (int16: the kernels are handed a pointer)"""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(DEV)


@pytest.mark.parametrize('add', [0, 1], ids=['copy', 'add'])
@pytest.mark.parametrize('lds', L.COPY_LD)
def test_copy_sweep(lds, add):
    """every window of the decision space at 37 pixels: the route the library reports is the restated one, the destination holds
    the numpy restatement to the bit, every other lane still the sentinel.  One arena per ldd, one launch per point."""
    ops = _ops()
    lib = ops.lib()
    P = L.COPY_PIXELS
    src = L.copy_src(P, lds)
    src_dev = _as_dev(np.concatenate([src.reshape(-1), np.zeros(8, dtype=np.uint16)]))
    stream = ops.stream()
    seen = {L.VEC: 0, L.GROUP: 0, L.SCALAR: 0}
    for ldd in L.COPY_LD:
        pts = L.copy_points(lds, ldd, add)
        slot = L.ceil8(P * ldd) + 8
        arena = np.full((len(pts), slot), 0x40E0, dtype=np.uint16)
        want = arena.copy()
        for i, (soff, doff, C_, Cfill) in enumerate(pts):
            d0 = L.copy_dst(P, ldd, doff, C_, add)
            arena[i, :P * ldd] = d0.reshape(-1)
            want[i, :P * ldd] = L.copy_ref(src, d0, soff, doff, C_, Cfill, add).reshape(-1)
        dev = _as_dev(arena)
        base = dev.data_ptr()
        assert base % 16 == 0 and src_dev.data_ptr() % 16 == 0
        lib.gcc_launch_count(1)
        for i, (soff, doff, C_, Cfill) in enumerate(pts):
            r = lib.gcc_nhwc_copy_route(lds, soff, ldd, doff, C_, Cfill)
            assert r == L.copy_route(lds, soff, ldd, doff, C_, Cfill), (lds, soff, ldd, doff, C_, Cfill)
            seen[r] += 1
            if add:
                rc = lib.gcc_nhwc_add(src_dev.data_ptr(), lds, soff, base + i * slot * 2, ldd, doff, C_, P, stream)
            else:
                rc = lib.gcc_nhwc_copy(src_dev.data_ptr(), lds, soff, base + i * slot * 2, ldd, doff, C_, Cfill, P, stream)
            assert rc == 0, (rc, lds, soff, ldd, doff, C_, Cfill)
        assert int(lib.gcc_launch_count(1)) == len(pts)
        torch.cuda.synchronize()
        got = dev.cpu().numpy().view(np.uint16)
        if not np.array_equal(got, want):
            i = int(np.argwhere((got != want).any(1))[0][0])
            soff, doff, C_, Cfill = pts[i]
            lane = sorted(set(int(v) % ldd if v < P * ldd else -1 for v in np.argwhere(got[i] != want[i])[:, 0]))
            raise AssertionError('%s lds %d soff %d ldd %d doff %d C %d Cfill %d (route %d): lanes %s differ (-1: behind the buffer)'
                                 % ('add' if add else 'copy', lds, soff, ldd, doff, C_, Cfill, L.copy_route(lds, soff, ldd, doff, C_, Cfill), lane))
    _route('nhwc_add' if add else 'nhwc_copy', ('lds', lds), 'vector=%d group=%d scalar=%d' % (seen[L.VEC], seen[L.GROUP], seen[L.SCALAR]))
    assert seen[L.SCALAR] and (lds == 12 or (seen[L.VEC] and seen[L.GROUP]))


@pytest.mark.parametrize('add', [0, 1], ids=['copy', 'add'])
@pytest.mark.parametrize('route', [L.VEC, L.GROUP, L.SCALAR], ids=['vector', 'group', 'scalar'])
def test_copy_past_the_capped_grid(route, add):
    """4096 * 256 + 13 threads' worth of work: the second trip of each kernel's grid-stride loop.  Small integers (sums stay exact
    in bf16), built and compared on the device."""
    ops = _ops()
    lib = ops.lib()
    lds, soff, ldd, doff, C_, Cfill = L.LARGE_COPY[route]
    if add:
        Cfill = C_
    P = L.LARGE_P
    assert lib.gcc_nhwc_copy_route(lds, soff, ldd, doff, C_, Cfill) == route == L.copy_route(lds, soff, ldd, doff, C_, Cfill)
    p = torch.arange(P, dtype=torch.int32, device=DEV)[:, None]
    ls = torch.arange(lds, dtype=torch.int32, device=DEV)[None]
    src = torch.zeros(P * lds + 8, dtype=torch.bfloat16, device=DEV)
    src[:P * lds].view(P, lds).copy_(((p * 3 + ls * 5) % 251 - 125).to(torch.bfloat16))
    dst = _sentinel(P * ldd + 8, torch.bfloat16)
    dv = dst[:P * ldd].view(P, ldd)
    if add:
        ld_ = torch.arange(doff, doff + C_, dtype=torch.int32, device=DEV)[None]
        dv[:, doff:doff + C_] = ((p + ld_ * 2) % 127 - 63).to(torch.bfloat16)
    want = dst.clone()
    wv, sv = want[:P * ldd].view(P, ldd), src[:P * lds].view(P, lds)
    if add:
        wv[:, doff:doff + C_] = (wv[:, doff:doff + C_].float() + sv[:, soff:soff + C_].float()).to(torch.bfloat16)
    else:
        wv[:, doff:doff + C_] = sv[:, soff:soff + C_]
        wv[:, doff + C_:doff + Cfill] = 0
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    lib.gcc_launch_count(1)
    if add:
        rc = lib.gcc_nhwc_add(src.data_ptr(), lds, soff, dst.data_ptr(), ldd, doff, C_, P, ops.stream())
    else:
        rc = lib.gcc_nhwc_copy(src.data_ptr(), lds, soff, dst.data_ptr(), ldd, doff, C_, Cfill, P, ops.stream())
    assert (rc, int(lib.gcc_launch_count(1))) == (0, 1)
    torch.cuda.synchronize()
    _route('nhwc_add_large' if add else 'nhwc_copy_large', (P, lds, soff, ldd, doff, C_, Cfill), ('vector', 'group', 'scalar')[route])
    assert torch.equal(dst.view(torch.int16), want.view(torch.int16))
    assert int((wv[:, doff:doff + C_] != L.SENTINEL).sum()) > P      # the window was written


def test_copy_refusals():
    """windows that do not fit their row: GCC_ERR_BAD_ARG from the query and from both entries, nothing launched"""
    ops = _ops()
    lib = ops.lib()
    src = torch.ones(64 * 24, dtype=torch.bfloat16, device=DEV)
    dst = _sentinel(64 * 24, torch.bfloat16)
    lib.gcc_launch_count(1)
    for lds, soff, ldd, doff, C_, Cfill in ((8, 6, 8, 0, 3, 3), (8, 0, 8, 6, 3, 3), (8, 0, 8, 4, 3, 5), (16, 8, 16, 0, 9, 9), (8, 0, 8, 0, 0, 0),
                                             (16, -8, 16, 0, 8, 8), (16, 0, 16, -8, 8, 8)):
        assert lib.gcc_nhwc_copy_route(lds, soff, ldd, doff, C_, Cfill) == L.BAD_ARG
        assert lib.gcc_nhwc_copy(src.data_ptr(), lds, soff, dst.data_ptr(), ldd, doff, C_, Cfill, 4, ops.stream()) == L.BAD_ARG
        if Cfill == C_:
            assert lib.gcc_nhwc_add(src.data_ptr(), lds, soff, dst.data_ptr(), ldd, doff, C_, 4, ops.stream()) == L.BAD_ARG
    assert lib.gcc_nhwc_copy(src.data_ptr(), 8, 0, dst.data_ptr(), 8, 0, 8, 8, 0, ops.stream()) == L.BAD_ARG          # no pixels
    assert lib.gcc_nhwc_copy(None, 8, 0, dst.data_ptr(), 8, 0, 8, 8, 4, ops.stream()) == L.BAD_ARG
    assert int(lib.gcc_launch_count(1)) == 0
    torch.cuda.synchronize()
    _untouched(dst, 'refused copies')
    _route('nhwc_copy_refused', (7,), 'launches=0')


def test_pack_pair():
    """every (Ca, Cb) with Ca + Cb <= 8, sources at lane 0 and 8 of 16, the group at lane 0 and 8 of 24: the pair and zeros up to
    the group, every other lane still the sentinel"""
    ops = _ops()
    lib = ops.lib()
    P = L.PAIR_PIXELS
    a = L.copy_src(P, 16)
    b = np.ascontiguousarray(np.roll(L.copy_src(P, 16)[:, ::-1], 2, axis=0))
    a_dev, b_dev = _as_dev(a.reshape(-1)), _as_dev(b.reshape(-1))
    pts = L.PAIR_POINTS
    assert len(pts) == 28 * 8
    slot = P * 24 + 8
    arena = np.full((len(pts), slot), 0x40E0, dtype=np.uint16)
    want = arena.copy()
    for i, (Ca, Cb, aoff, boff, doff) in enumerate(pts):
        want[i, :P * 24] = L.pair_ref(a, aoff, b, boff, arena[i, :P * 24].reshape(P, 24), doff, Ca, Cb).reshape(-1)
    dev = _as_dev(arena)
    assert dev.data_ptr() % 16 == 0 and a_dev.data_ptr() % 16 == 0 and b_dev.data_ptr() % 16 == 0
    lib.gcc_launch_count(1)
    for i, (Ca, Cb, aoff, boff, doff) in enumerate(pts):
        rc = lib.gcc_nhwc_pack_pair(a_dev.data_ptr(), 16, aoff, b_dev.data_ptr(), 16, boff, dev.data_ptr() + i * slot * 2, 24, doff, Ca, Cb, P,
                                    ops.stream())
        assert rc == 0, (Ca, Cb, aoff, boff, doff)
    assert int(lib.gcc_launch_count(1)) == len(pts)
    torch.cuda.synchronize()
    _route('nhwc_pack_pair', (len(pts), P), 'launches=%d workgroups=2' % len(pts))
    got = dev.cpu().numpy().view(np.uint16)
    bad = np.argwhere((got != want).any(1))
    assert not len(bad), 'Ca, Cb, aoff, boff, doff = %s' % (pts[int(bad[0][0])] if len(bad) else None,)
    # refusals: nine channels, and each of the six alignment arguments off by 4
    keep = _sentinel(P * 32, torch.bfloat16)
    big = torch.ones(P * 32, dtype=torch.bfloat16, device=DEV)
    lib.gcc_launch_count(1)
    for lda, aoff, ldb, boff, ldd, doff, Ca, Cb in ((16, 0, 16, 0, 24, 0, 4, 5), (20, 0, 16, 0, 24, 0, 3, 3), (16, 4, 16, 0, 24, 0, 3, 3),
                                                    (16, 0, 20, 0, 24, 0, 3, 3), (16, 0, 16, 4, 24, 0, 3, 3), (16, 0, 16, 0, 28, 0, 3, 3),
                                                    (16, 0, 16, 0, 24, 4, 3, 3)):
        rc = lib.gcc_nhwc_pack_pair(big.data_ptr(), lda, aoff, big.data_ptr(), ldb, boff, keep.data_ptr(), ldd, doff, Ca, Cb, P, ops.stream())
        assert rc == L.BAD_ARG, (lda, aoff, ldb, boff, ldd, doff, Ca, Cb)
    assert int(lib.gcc_launch_count(1)) == 0
    torch.cuda.synchronize()
    _untouched(keep, 'refused pack pairs')


# ---- NCHW fp32 <-> NHWC bf16 ---------------------------------------------------------------------------------------------------
def _planted(n, seed):
    """n fp32 values, normal * 3, the special bit patterns at the front, at the end and every 97 values"""
    t = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 3
    k = min(n, len(SPECIAL))
    for start in list(range(0, max(n - k, 0), 97 * 16))[:64] + [n - k]:
        t[start:start + k] = SPECIAL[:k]
    return t


def _to_nhwc(N, C_, H, W, ld, off, Cfill, seed):
    ops = _ops()
    lib = ops.lib()
    P = N * H * W
    src = _planted(N * C_ * H * W, seed).view(N, C_, H, W)
    dst = _sentinel(P * ld + 8, torch.bfloat16)
    sd = src.to(DEV)
    lib.gcc_launch_count(1)
    rc = lib.gcc_nchw_f32_to_nhwc_bf16(sd.data_ptr(), dst.data_ptr(), N, C_, H, W, ld, off, Cfill, ops.stream())
    assert (rc, int(lib.gcc_launch_count(1))) == (0, 1)
    torch.cuda.synchronize()
    want = torch.full((P * ld + 8,), L.SENTINEL, dtype=torch.bfloat16)
    wv = want[:P * ld].view(P, ld)
    wv[:, off:off + C_] = src.permute(0, 2, 3, 1).reshape(P, C_).bfloat16()
    wv[:, off + C_:off + Cfill] = 0
    assert L.same_bf16(dst.cpu(), want), 'to NHWC: N %d C %d HW %d ld %d off %d Cfill %d' % (N, C_, H * W, ld, off, Cfill)


def _to_nchw(N, C_, H, W, ld, off, seed):
    ops = _ops()
    lib = ops.lib()
    P = N * H * W
    src = _planted(P * ld, seed).bfloat16()
    out = _sentinel(N * C_ * H * W + 8)
    sd = src.to(DEV)
    lib.gcc_launch_count(1)
    rc = lib.gcc_nhwc_bf16_to_nchw_f32(sd.data_ptr(), out.data_ptr(), N, C_, H, W, ld, off, ops.stream())
    assert (rc, int(lib.gcc_launch_count(1))) == (0, 1)
    torch.cuda.synchronize()
    want = torch.full((N * C_ * H * W + 8,), L.SENTINEL)
    want[:N * C_ * H * W] = src.view(N, H * W, ld)[:, :, off:off + C_].permute(0, 2, 1).float().reshape(-1)
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)), 'to NCHW: N %d C %d HW %d ld %d off %d' % (N, C_, H * W, ld, off)


@pytest.mark.parametrize('N,C_,H,W', L.LAYOUT_CASES)
def test_layout_conversions(N, C_, H, W):
    """both directions at lane 0, 3 and 8 of a 24-lane buffer, with and without a zero fill; the special values (ties both ways,
    denormals, +-inf, NaNs, the largest float) ride along: NaN stays NaN, the rest has torch's round-to-nearest-even bits"""
    n = 0
    for off in L.LAYOUT_OFFS:
        for Cfill in L.layout_cfills(C_):
            _to_nhwc(N, C_, H, W, L.LAYOUT_LD, off, Cfill, seed=N * 100 + off * 10 + Cfill)
            n += 1
        _to_nchw(N, C_, H, W, L.LAYOUT_LD, off, seed=N * 100 + off)
    _route('layout', (N, C_, H * W), 'nchw_to_nhwc=%d nhwc_to_nchw=%d workgroups=%d' % (n, len(L.LAYOUT_OFFS), -(-N * H * W // 256)))


def test_layout_conversions_past_the_capped_grid():
    N, C_, H, W, ld, off, Cfill = L.LAYOUT_LARGE
    assert N * H * W > L.GRID_CAP * 256 and H * W < L.GRID_CAP * 256          # the second image begins inside the first pass
    _to_nhwc(N, C_, H, W, ld, off, Cfill, seed=5)
    _to_nchw(N, C_, H, W, ld, off, seed=6)
    _route('layout_large', (N, C_, H * W), 'workgroups=%d pixels_per_thread<=2' % L.GRID_CAP)


def test_layout_refusals():
    ops = _ops()
    lib = ops.lib()
    src = torch.ones(2 * 13 * 9 + 64, device=DEV)
    dst = _sentinel(18 * 24, torch.bfloat16)
    out = _sentinel(2 * 13 * 9 + 64)
    lib.gcc_launch_count(1)
    for C_, off, Cfill in ((13, 12, 13), (3, 16, 9), (3, 20, 5)):
        assert lib.gcc_nchw_f32_to_nhwc_bf16(src.data_ptr(), dst.data_ptr(), 2, C_, 3, 3, 24, off, Cfill, ops.stream()) == L.BAD_ARG
    assert lib.gcc_nhwc_bf16_to_nchw_f32(dst.data_ptr(), out.data_ptr(), 2, 13, 3, 3, 24, 12, ops.stream()) == L.BAD_ARG
    assert int(lib.gcc_launch_count(1)) == 0
    torch.cuda.synchronize()
    _untouched(dst, 'refused conversion')
    _untouched(out, 'refused conversion')
    _route('layout_refused', (4,), 'launches=0')


# ---- weight packing ------------------------------------------------------------------------------------------------------------
def test_pack_plan_alignment_and_tile_edges(monkeypatch):
    """ops.PackPlan over masters carved out of one flat fp32 buffer 0, 1, 2 and 3 elements behind a 16-byte boundary, with
    FUSED_PACK on and off: the kinds each master is scheduled with; W and Wt, which start out as 7.0, equal to the definition
    over the WHOLE packed tensors (exact zeros in every padding row, column and gap); the bits of the aligned fused run in
    every other run."""
    from gcc_amd import engine
    ops = _ops()
    lib = ops.lib()
    first = None
    for fused in (1, 0):
        monkeypatch.setattr(ops, 'FUSED_PACK', bool(fused))
        for offset in range(4):
            flat, spans = L.pack_masters(offset, SPECIAL)
            fd = flat.to(DEV)
            assert fd.data_ptr() % 16 == 0
            convs = [engine.ConvOp(L.master_view(fd, start, w), None, w.shape[2], 1, 0, False, row_split=rs, col_split=cs)
                     for (start, w), (_, _, _, rs, cs) in zip(spans, L.PACK_SHAPES)]
            for c in convs:
                assert c.weight.data_ptr() % 16 == (4 * offset) % 16
                c.w.fill_(L.SENTINEL)
                c.wt.fill_(L.SENTINEL)
            plan = ops.PackPlan(convs, DEV)
            items = plan.d_items.cpu()
            sched = []
            for i, shape in enumerate(L.PACK_SHAPES):
                kinds = set(int(k) for k in items[items[:, 0] == i][:, 1])
                assert kinds == L.pack_kinds(shape, offset, fused), (shape, offset, fused, kinds)
                sched.append(''.join(map(str, sorted(kinds))))
            lib.gcc_launch_count(1)
            plan.run()
            assert int(lib.gcc_launch_count(1)) == 1
            torch.cuda.synchronize()
            _route('pack_multi', ('fused', fused, 'offset', offset), 'items=%d kinds=%s' % (plan.n, ','.join(sched)))
            bits = []
            for c, (start, w), shape in zip(convs, spans, L.PACK_SHAPES):
                W, Wt = packed_definition(w, shape[3], shape[4])
                gw, gwt = c.w.cpu(), c.wt.cpu()
                assert gw.shape == W.shape and gwt.shape == Wt.shape
                assert L.same_bf16(gw, W), 'W of %r (fused %d, offset %d)' % (shape, fused, offset)
                assert L.same_bf16(gwt, Wt), 'Wt of %r (fused %d, offset %d)' % (shape, fused, offset)
                bits.append((gw.view(torch.int16), gwt.view(torch.int16)))
            assert torch.equal(fd.cpu().view(torch.int32), flat.view(torch.int32)), 'the masters'
            if first is None:
                first = bits
            for (a, b), (a0, b0), shape in zip(bits, first, L.PACK_SHAPES):
                assert torch.equal(a, a0) and torch.equal(b, b0), 'bits of the aligned fused run: %r (fused %d, offset %d)' % (shape, fused, offset)


@pytest.mark.parametrize('offset', [0, 1])
def test_pack_weights_single_tensor(offset):
    """gcc_pack_weights on the same shapes (unsplit): both packings, W alone, Wt alone, into buffers that start out as 7.0 and
    through ops.pack_weights (torch.empty); both pointers null is refused"""
    ops = _ops()
    lib = ops.lib()
    flat, spans = L.pack_masters(offset, SPECIAL)
    fd = flat.to(DEV)
    for (start, w), shape in zip(spans, L.PACK_SHAPES):
        rows, cols, k = shape[:3]
        taps, rowsp, colsp = k * k, L.ceil8(rows), L.ceil8(cols)
        W, Wt = packed_definition(w, 0, 0)
        W, Wt = W[:rows].contiguous(), Wt[:cols].contiguous()
        m = L.master_view(fd, start, w)
        for want_w, want_wt in ((1, 1), (1, 0), (0, 1)):
            bw, bwt = _sentinel(rows * taps * colsp + 8, torch.bfloat16), _sentinel(cols * taps * rowsp + 8, torch.bfloat16)
            lib.gcc_launch_count(1)
            rc = lib.gcc_pack_weights(m.data_ptr(), rows, taps, cols, bw.data_ptr() if want_w else None, bwt.data_ptr() if want_wt else None,
                                      ops.stream())
            assert (rc, int(lib.gcc_launch_count(1))) == (0, want_w + want_wt)
            torch.cuda.synchronize()
            for want, buf, ref, name in ((want_w, bw, W, 'W'), (want_wt, bwt, Wt, 'Wt')):
                n = ref.numel()
                if want:
                    assert L.same_bf16(buf[:n].cpu(), ref.reshape(-1)), '%s of %r (offset %d)' % (name, shape, offset)
                    _untouched(buf[n:], name + ' behind its end')
                else:
                    _untouched(buf, name + ' that was not asked for')
        gw, gwt = ops.pack_weights(m)
        torch.cuda.synchronize()
        assert gw.shape == W.shape and gwt.shape == Wt.shape and L.same_bf16(gw.cpu(), W) and L.same_bf16(gwt.cpu(), Wt)
        lib.gcc_launch_count(1)
        assert lib.gcc_pack_weights(m.data_ptr(), rows, taps, cols, None, None, ops.stream()) == L.BAD_ARG
        assert int(lib.gcc_launch_count(1)) == 0
    _route('pack_weights', ('offset', offset), 'pack_w_kernel + pack_wt_kernel, %d masters' % len(spans))
