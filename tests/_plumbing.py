"""Data, float64 references, bounds, route restatements and index-walk emulations of the small kernels between the convolutions:
gcc_channel_sum / gcc_channel_sum_group and gcc_gate_mask (norm_act.hip); gcc_nhwc_copy, gcc_nhwc_add, gcc_nhwc_pack_pair, the two
NCHW <-> NHWC conversions, gcc_pack_weights and gcc_pack_weights_multi (misc.hip).  Shared by tests/test_plumbing_exact_gpu.py,
which runs the kernels, and tests/test_plumbing_bounds_cpu.py, which examines the case lists and the checks without a GPU.  No
tests here.

The bound of the channel sums (the only inexact comparison of the two files)
-----------------------------------------------------------------------------
out[c] is a sum of P bf16 values formed in fp32 and finished in double.  A value x_i is rounded once by every fp32 addition its
running sum goes through; to first order |out - sum x| <= u * sum_i d_i |x_i| with u = 2^-24 and d_i the number of those
additions, so with d = max d_i:

    bound[c] = d * u * sum_p |x[p, c]|  +  blocks * 2^-53 * sum_p |x[p, c]|  +  u * |total|  (+ u * |prior + total|)

* the lane chain.  A lane of channel_sum_kernel adds its n pixels in order (the unrolled trips of four add in the same order as
  the tail trips); the first addition is to an exact zero, so n - 1 roundings, n = ceil(P / (gridDim * PPB)) for the longest lane.
  channel_sum_small_kernel: n = ceil(P / 512).
* the fold of the pixel lanes.  CHP < 64: log2(64 / CHP) shuffle steps, then (r0 + r1) + (r2 + r3) over the four waves' rows:
  log2(64 / CHP) + 2.  CHP == 64: the four rows only: 2.  CHP of 128 / 256: t = 0 + red[0] (+ red[1]): PPB - 1.  The one-launch
  kernel: the six steps of wave_sum.
* the workgroups (two-launch route: `blocks` partial rows; one-launch route: the 8 waves) are added in double: 2^-53 each.
* the cast of the double total to fp32: u |total|; with accumulate = 1 the fp32 addition to the prior contents: u |prior + total|.

No factor on top: a measured ratio above 1 means the derivation or the kernel is wrong.  sum_emul / sum_emul_small below walk the
kernels' own index arithmetic (blockIdx, pl, step = gridDim * PPB) with numpy fp32 and stay inside the bound at every case;
three deliberately wrong walks (a dropped last pixel, a lane whose first unrolled trip is counted twice, the CHP = 128 fold
reading red[q * 64 + ch]) fall outside it and fail the exact check (tests/test_plumbing_bounds_cpu.py)."""
import numpy as np
import torch

from tests._perelem import U24, bwd_blocks, layout, rb64

BAD_ARG, UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3        # include/gcc_hip.h GCC_ERR_*
SENTINEL = 7.0
GARBAGE = 1e30
SMALL_NT, SMALL_MAX, GROUP_MAX = 512, 16384, 24          # norm_act.hip SUM_SMALL_NT; gcc_hip.h GCC_CHANSUM_SMALL_MAX_PIXELS / _GROUP_MAX
GRID_CAP = 4096                                         # misc.hip grid_for: workgroups of 256 threads


def ceil8(v):
    return (v + 7) & ~7


# ---- channel sums ------------------------------------------------------------------------------------------------------------
SUM_C = (1, 3, 8, 20, 40, 264, 512, 520, 1024, 1032, 2048)
SUM_C_REFUSED = 2056


def fold_of(C):
    """which of channel_sum_kernel's three folds a channel count takes"""
    CHP = layout(C)[1]
    return 'shuffle' if CHP < 64 else ('rows' if CHP == 64 else 'walk')


def sum_trips(P, C):
    """channel_sum_kernel's two loops walked for every lane: (unrolled, tail) trip counts, each [gridDim, PPB]"""
    PPB = layout(C)[2]
    blocks = bwd_blocks(P, C)
    step = blocks * PPB
    pix = (np.arange(blocks, dtype=np.int64)[:, None] * PPB + np.arange(PPB, dtype=np.int64)[None])
    unrolled, tail = np.zeros_like(pix), np.zeros_like(pix)
    while True:
        go = pix + 3 * step < P
        if not go.any():
            break
        unrolled += go
        pix = np.where(go, pix + 4 * step, pix)
    while True:
        go = pix < P
        if not go.any():
            break
        tail += go
        pix = np.where(go, pix + step, pix)
    return unrolled, tail


def sum_pixels(C):
    """Two-launch pixel counts of a channel count: one pixel; one short of a sweep (a lane has none; not for PPB = 1); and two
    taken from the sizing steps of bwd_blocks, one pixel past k half-sweeps of 512 workgroups (k = 1 .. 16), by walking the
    kernel's loops (sum_trips): the last step before any lane takes the unrolled loop (tail trips only, as many as they get), and
    the first step at which some lane makes an unrolled trip of four AND a tail trip.  (A lane needs five pixels for that, and
    bwd_blocks gives the workgroups `sweeps` half-sweeps each: 9 of them, k = 8, unless the 512-workgroup rule is off, PPB = 1.)"""
    PPB = layout(C)[2]
    lp = max(1, PPB // 2)
    tail_only = both = None
    for k in range(1, 17):
        P = k * 512 * lp + 1
        u, t = sum_trips(P, C)
        if not u.any():
            tail_only = P
        if ((u > 0) & (t > 0)).any():
            both = P
            break
    assert tail_only and both and tail_only < both
    return tuple(sorted({1, max(1, PPB - 1), tail_only, both}))


SUM_TWO = tuple((P, C) for C in SUM_C for P in sum_pixels(C))
# one-launch route: the edges of the 512-thread sweep (511 / 512 / 513), of the unrolled trip of four sweeps (1536 / 1537: three
# tail trips, a fourth; 2048 / 2049: one unrolled trip exactly, and a tail trip behind it) and the largest tensor it takes
SUM_ONE = ((1, 3), (511, 20), (512, 40), (513, 8), (1536, 520), (1537, 1), (2048, 264), (2049, 520), (16384, 3))


def small_trips(P):
    """channel_sum_small_body's two loops: (unrolled, tail) per thread, each [512]"""
    pix = np.arange(SMALL_NT, dtype=np.int64)
    unrolled, tail = np.zeros_like(pix), np.zeros_like(pix)
    while True:
        go = pix + 3 * SMALL_NT < P
        if not go.any():
            break
        unrolled += go
        pix = np.where(go, pix + 4 * SMALL_NT, pix)
    while True:
        go = pix < P
        if not go.any():
            break
        tail += go
        pix = np.where(go, pix + SMALL_NT, pix)
    return unrolled, tail


def sum_int(P, C):
    """[P, C] float64 integers in [-8, 8] without zero (a dropped or doubled pixel moves every channel), a pattern that is not
    symmetric in pixel and channel.  |sum| <= 8 P < 2^24 up to two million pixels: every partial sum is exact in fp32."""
    assert 8 * P < 2 ** 24
    p = torch.arange(P, dtype=torch.int64)[:, None]
    c = torch.arange(C, dtype=torch.int64)[None]
    r = (p * 7 + c * 3 + (p // 5) * (c + 1)) % 16
    return torch.where(r < 8, r - 8, r - 7).double()


def sum_normal(P, C, seed):
    """[P, C] float64, bf16-representable: per-channel mean of either sign in +-[0.5, 1.5], deviation in [0.5, 2]"""
    g = torch.Generator().manual_seed(seed)
    mu = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    std = 0.5 + 1.5 * torch.rand(C, generator=g)
    return rb64(torch.randn(P, C, generator=g) * std + mu)


def sum_prior(C, integer):
    """contents of `out` before an accumulating call"""
    c = torch.arange(C, dtype=torch.float32)
    return (c % 11 - 5) * 3.0 if integer else (c % 7 - 3) * 1.37


def sum_chain(P, C, small):
    """d of the bound: the longest chain of fp32 additions a value goes through, and the number of double additions behind it"""
    if small:
        return (-(-P // SMALL_NT) - 1) + 6, SMALL_NT // 64
    _, CHP, PPB = layout(C)
    blocks = bwd_blocks(P, C)
    n = -(-P // (blocks * PPB))
    fold = (64 // CHP).bit_length() - 1 + 2 if CHP < 64 else (2 if CHP == 64 else PPB - 1)
    return (n - 1) + fold, blocks


def sum_bound(x, P, C, small, prior=None):
    """(float64 reference, bound) of out[c] for x [P, C] float64"""
    d, nd = sum_chain(P, C, small)
    A, tot = x.abs().sum(0), x.sum(0)
    bound = d * U24 * A + nd * 2.0 ** -53 * A + U24 * tot.abs()
    if prior is not None:
        tot = tot + prior.double()
        bound = bound + U24 * tot.abs()
    return tot, bound


def _finish(total64, prior):
    t = total64.astype(np.float32)
    return torch.from_numpy(t if prior is None else prior.numpy().astype(np.float32) + t)


def sum_emul(x, C, prior=None, fault=None):
    """gcc_channel_sum's two launches on the CPU for x [P, C] (fp32 arithmetic in numpy): the lanes' walk in the kernel's order,
    its fold of the pixel lanes, the double fold of the partial rows, the cast and the accumulate.  fault: 'drop_last' (the walk
    stops one pixel early), 'double_trip' (the first lane with an unrolled trip adds its first one twice), 'fold64' (the walk of
    the 128- / 256-chunk fold strides by 64 rows instead of CHP)."""
    P = x.shape[0]
    CH, CHP, PPB = layout(C)
    C8 = CH * 8
    v = np.zeros((P, C8), dtype=np.float32)
    v[:, :C] = x.numpy().astype(np.float32)
    blocks = bwd_blocks(P, C)
    step = blocks * PPB
    end = P - 1 if fault == 'drop_last' else P
    pix = (np.arange(blocks, dtype=np.int64)[:, None] * PPB + np.arange(PPB, dtype=np.int64)[None])
    acc = np.zeros((blocks, PPB, C8), dtype=np.float32)
    pending = fault == 'double_trip'
    while True:
        go = pix + 3 * step < end
        if not go.any():
            break
        for u in range(4):
            acc[go] = acc[go] + v[pix[go] + u * step]
        if pending:
            b, l = np.argwhere(go)[0]
            for u in range(4):
                acc[b, l] = acc[b, l] + v[pix[b, l] + u * step]
            pending = False
        pix = np.where(go, pix + 4 * step, pix)
    assert not pending, 'no lane of this case takes the unrolled loop'
    while True:
        go = pix < end
        if not go.any():
            break
        acc[go] = acc[go] + v[pix[go]]
        pix = np.where(go, pix + step, pix)
    full = np.zeros((blocks, PPB, CHP, 8), dtype=np.float32)
    full[:, :, :CH] = acc.reshape(blocks, PPB, CH, 8)
    red = full.reshape(blocks, 256, 8)                       # row = threadIdx.x = pl * CHP + ch
    if CHP <= 64:
        s = red.reshape(blocks, 4, 64, 8)
        o = 32
        while o >= CHP and CHP < 64:
            s = s + s[:, :, np.arange(64) ^ o]
            o >>= 1
        r = s[:, :, :CHP]
        part = (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])
    else:
        stride = 64 if fault == 'fold64' else CHP
        part = np.zeros((blocks, CHP, 8), dtype=np.float32)
        for q in range(PPB):
            part = part + red[:, q * stride:q * stride + CHP]
    part = part[:, :CH].reshape(blocks, C8)[:, :C]
    return _finish(part.astype(np.float64).sum(0), prior)


def sum_emul_small(x, prior=None):
    """channel_sum_small_kernel (and an entry of channel_sum_group_kernel) on the CPU: 512 threads, wave_sum, eight waves in double"""
    P, C = x.shape
    v = x.numpy().astype(np.float32)
    acc = np.zeros((SMALL_NT, C), dtype=np.float32)
    for k in range(-(-P // SMALL_NT)):
        rows = v[k * SMALL_NT:(k + 1) * SMALL_NT]
        acc[:rows.shape[0]] = acc[:rows.shape[0]] + rows
    s = acc.reshape(SMALL_NT // 64, 64, C)
    o = 32
    while o > 0:
        s = s + s[:, np.arange(64) ^ o]
        o >>= 1
    return _finish(s[:, 0].astype(np.float64).sum(0), prior)


def sum_buffer(x, C, ld, off, fill):
    """a [P, ld] bf16 buffer (plus one 8-lane group behind it) holding x in lanes [off, off + C) and `fill` everywhere else"""
    P = x.shape[0]
    flat = torch.full((P * ld + 8,), fill, dtype=torch.bfloat16)
    flat[:P * ld].view(P, ld)[:, off:off + C] = x.to(torch.bfloat16)
    return flat


# group entry: 24 items, C = 3 at both ends, every one-launch pixel-count edge, wide items kept short
GROUP_ITEMS = tuple(zip((3, 1, 8, 20, 40, 264, 512, 520, 3, 8, 20, 40, 264, 512, 520, 1, 3, 8, 20, 40, 264, 1, 8, 3),
                        (16384, 511, 512, 513, 1536, 1537, 2048, 2049, 1, 16384, 2049, 8191, 1, 513, 5, 2048, 4097, 1537, 16383, 1, 511, 1, 7, 2049),
                        (0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0, 1)))


# ---- gcc_nhwc_copy / gcc_nhwc_add ---------------------------------------------------------------------------------------------
COPY_PIXELS = 37
COPY_LD = (8, 16, 24, 12)
COPY_C = (1, 2, 3, 5, 8, 9, 16)
VEC, GROUP, SCALAR = 0, 1, 2


def copy_route(lds, soff, ldd, doff, C, Cfill):
    """the decision of misc.hip gcc_nhwc_copy_route, restated"""
    Cw = max(C, Cfill)
    if C <= 0 or soff < 0 or doff < 0 or soff + C > lds or doff + Cw > ldd:
        return BAD_ARG
    if all(v % 8 == 0 for v in (lds, soff, ldd, doff, C)) and Cfill <= C:
        return VEC
    if lds % 8 == 0 and ldd % 8 == 0 and soff % 8 + C <= 8 and doff % 8 + Cw <= 8:
        return GROUP
    return SCALAR


def copy_points(lds, ldd, add):
    """the sweep of one (lds, ldd): (soff, doff, C, Cfill) over offsets 0..15, COPY_C and Cfill in {C, C + 1, the next multiple of 8},
    restricted to windows that fit (the add form has no fill: Cfill = C)"""
    pts = []
    for C in COPY_C:
        for Cfill in ((C,) if add else sorted({C, C + 1, ceil8(C)})):
            for soff in range(16):
                for doff in range(16):
                    if soff + C <= lds and doff + Cfill <= ldd:
                        pts.append((soff, doff, C, Cfill))
    return pts


def group_facts(soff, doff, C, Cfill, add):
    """what nhwc_copy_group_kernel does at a point: (d0 != 0, whole-group store without reading the destination, a zero fill)"""
    return doff % 8 != 0, (not add and doff % 8 == 0 and Cfill == 8), Cfill > C


def bf16_bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def bits_to_f32(b):
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bits(f):
    """round to nearest even (finite values)"""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


_SENT_BITS = np.uint16(0x40E0)                            # bf16 7.0
# source lanes: +-2^-8 (half an ulp of 1: the ties), 1.5, -0.0, the smallest bf16 denormal, 3, -2.5
_SRC_POOL = np.array([0x3B80, 0xBB80, 0x3FC0, 0x8000, 0x0001, 0x4040, 0xC020], dtype=np.uint16)
# destination lanes of an add: 1 (1 + 2^-8 ties down to the even 1), 1 + 2^-7 (ties up to the even 1 + 2^-6), -1, 2.5, -3
_DST_POOL = np.array([0x3F80, 0x3F81, 0xBF80, 0x4020, 0xC040], dtype=np.uint16)


def copy_src(P, lds):
    """[P, lds] uint16 bf16 bits"""
    p, l = np.arange(P)[:, None], np.arange(lds)[None]
    return _SRC_POOL[(3 * p + 5 * l + p // 7) % len(_SRC_POOL)]


def copy_dst(P, ldd, doff, C, add):
    """[P, ldd] uint16: the sentinel everywhere; the window of an add holds the values it adds onto"""
    d = np.full((P, ldd), _SENT_BITS, dtype=np.uint16)
    if add:
        p, l = np.arange(P)[:, None], np.arange(doff, doff + C)[None]
        d[:, doff:doff + C] = _DST_POOL[(p + 2 * l) % len(_DST_POOL)]
    return d


def copy_ref(src, dst, soff, doff, C, Cfill, add, fault=None):
    """what gcc_nhwc_copy / gcc_nhwc_add leave in dst: the slice, then zeros up to Cfill; or one bf16 rounding of the fp32 sum.
    fault 'fill_one_more': a kernel that zero-fills one lane too many."""
    out = dst.copy()
    if add:
        out[:, doff:doff + C] = f32_to_bits(bits_to_f32(dst[:, doff:doff + C]) + bits_to_f32(src[:, soff:soff + C]))
        return out
    out[:, doff:doff + C] = src[:, soff:soff + C]
    fill_end = doff + max(C, Cfill) + (1 if fault == 'fill_one_more' else 0)
    out[:, doff + C:min(fill_end, dst.shape[1])] = 0
    return out


def add_ties(src, dst, soff, doff, C):
    """number of window elements whose fp32 sum lies exactly between two bf16 values"""
    s = bits_to_f32(dst[:, doff:doff + C]) + bits_to_f32(src[:, soff:soff + C])
    return int(((s.view(np.uint32) & np.uint32(0xFFFF)) == np.uint32(0x8000)).sum())


def pair_ref(a, aoff, b, boff, dst, doff, Ca, Cb):
    """gcc_nhwc_pack_pair: the group at doff holds a's Ca lanes, b's Cb lanes and zeros up to 8; every other lane as it was"""
    out = dst.copy()
    out[:, doff:doff + 8] = 0
    out[:, doff:doff + Ca] = a[:, aoff:aoff + Ca]
    out[:, doff + Ca:doff + Ca + Cb] = b[:, boff:boff + Cb]
    return out


PAIR_PIXELS = 300                                         # a second workgroup
PAIR_POINTS = tuple((Ca, Cb, aoff, boff, doff) for Ca in range(1, 8) for Cb in range(1, 9 - Ca) for aoff in (0, 8) for boff in (0, 8)
                    for doff in (0, 8))


# one past a full pass of the capped grid: pixels for the group and scalar kernels (a thread per pixel), 8-channel chunks for the
# vector kernel (a thread per chunk; one chunk per pixel here)
LARGE_P = GRID_CAP * 256 + 13
LARGE_COPY = {                                            # route: (lds, soff, ldd, doff, C, Cfill)
    VEC: (8, 0, 8, 0, 8, 8),
    GROUP: (8, 2, 8, 3, 3, 5),
    SCALAR: (12, 9, 8, 2, 3, 5),
}

# ---- NCHW fp32 <-> NHWC bf16 ---------------------------------------------------------------------------------------------------
LAYOUT_CASES = ((1, 1, 1, 1), (2, 3, 5, 7), (3, 13, 3, 3))          # N, C, H, W
LAYOUT_LD = 24
LAYOUT_OFFS = (0, 3, 8)
LAYOUT_LARGE = (2, 3, 1, GRID_CAP * 128 + 7, 8, 3, 5)                # N, C, H, W, ld, off, Cfill: two images past the capped grid


def layout_cfills(C):
    return sorted({C, 8, 5})


# ---- weight packing ------------------------------------------------------------------------------------------------------------
# rows, cols, k, row_split, col_split: the edges of the 64 x 64 tiles of kind 2 (exactly one tile; one row / one 4-column piece
# past it; rowsp > rows inside a tile; a single row; 49 taps of a 4-wide master; more rows than a tile with 12 columns), widths
# that are no multiple of 4 (never kind 2), and a column split, a row split and both (tests/test_segmented_conv_gpu.py cases 1, 3, 5)
PACK_SHAPES = ((64, 64, 1, 0, 0), (65, 64, 3, 0, 0), (64, 68, 3, 0, 0), (1, 8, 4, 0, 0), (130, 4, 7, 0, 0), (3, 64, 4, 0, 0),
               (200, 12, 1, 0, 0), (40, 6, 3, 0, 0), (24, 10, 1, 0, 0), (32, 20, 1, 0, 12), (21, 24, 4, 12, 0), (13, 20, 3, 5, 12))
PACK_SPECIAL = 2                                          # index of the master that carries the special values


def pack_kinds(shape, offset, fused):
    """work-item kinds ops.PackPlan must schedule for a master at `offset` fp32 elements behind a 16-byte boundary"""
    rows, cols, k, rs, cs = shape
    return {2} if (fused and not rs and not cs and cols % 4 == 0 and offset % 4 == 0) else {0, 1}


def pack_masters(offset, special, seed=17):
    """One flat fp32 buffer holding every master of PACK_SHAPES as [rows][taps][cols] at `offset` elements behind a 16-byte
    boundary, and the logical masters [rows, cols, k, k] it holds.  Returns (flat, [(start, logical)])."""
    g = torch.Generator().manual_seed(seed)
    pos, spans = 0, []
    for i, (rows, cols, k, rs, cs) in enumerate(PACK_SHAPES):
        w = torch.randn(rows, cols, k, k, generator=g) * 0.1
        if i == PACK_SPECIAL:
            w.view(-1)[5:5 + special.numel()] = special
            w.view(-1)[-special.numel():] = special
        spans.append((pos + offset, w))
        pos += (w.numel() + offset + 3) // 4 * 4 + 4
    flat = torch.full((pos,), SENTINEL, dtype=torch.float32)
    for start, w in spans:
        flat[start:start + w.numel()] = w.permute(0, 2, 3, 1).reshape(-1)
    return flat, spans


def master_view(flat, start, w):
    """the channels_last parameter [rows, cols, k, k] living at flat[start:]"""
    rows, cols, k, _ = w.shape
    return flat[start:start + w.numel()].view(rows, k, k, cols).permute(0, 3, 1, 2)


def same_bf16(got, want):
    """NaN stays NaN (and nothing else becomes one), everything else bit for bit"""
    nan = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), nan)) and bool(torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16)))
