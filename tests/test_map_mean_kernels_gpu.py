"""gcc_map_mean / gcc_map_mean_f32 (gcc_amd/csrc/inception.hip): the spatial mean of a large NHWC map in f64 with the pixels of
an image split over workgroups -- exact on integer maps at every split, within the rounding bound on Gaussian maps at the three
real tap shapes, the same bits run after run and whatever the batch around an image, every refusal before any launch."""
import numpy as np
import pytest
import torch

from tests import _inception_taps as T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3            # include/gcc_hip.h GCC_ERR_*
# h w: 1, around the 32 pixel rows of a workgroup, two that make the quotient inexact (7, 33), and the real taps' 17^2, 35^2, 73^2
SHAPES = {1: (1, 1), 7: (7, 1), 31: (31, 1), 32: (4, 8), 33: (3, 11), 289: (17, 17), 1225: (35, 35), 5329: (73, 73)}
WIDTHS = {torch.bfloat16: (8, 24, 64, 192), torch.float32: (4, 12, 8, 24, 64, 192)}
TAPS = ((73, 73, 64), (35, 35, 192), (17, 17, 768))


def _ops():
    from gcc_amd import ops
    return ops


def _chunk(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def _window(values, dtype, ld, off, tail=64):
    """the NHWC view [N, C, h, w] of `values` (float tensor [N, h, w, C]) as channels [off, off + C) of pixels of ld elements;
    every other element of the buffer -- the gap lanes and `tail` elements behind the last pixel -- is NaN"""
    N, h, w, Cc = values.shape
    buf = torch.full((N * h * w * ld + tail,), float('nan'), dtype=dtype, device=DEV)
    body = buf[:N * h * w * ld].view(N, h, w, ld)
    body[..., off:off + Cc] = values.to(DEV, dtype)
    return body.permute(0, 3, 1, 2)[:, off:off + Cc]


def _mean(view, segments=0, canary=-7.0):
    """the kernel's [N, C] result on the host, written in front of a canary that must survive"""
    ops = _ops()
    N, Cc = view.shape[:2]
    buf = torch.full((N * Cc + 8,), canary, dtype=torch.float32, device=DEV)
    fn = ops.map_mean if view.dtype == torch.bfloat16 else ops.map_mean_f32
    fn(view, buf[:N * Cc], segments=segments)
    host = buf.cpu()
    assert bool((host[N * Cc:] == canary).all()), 'the canary behind out was overwritten'
    return host[:N * Cc].view(N, Cc)


def _segment_choices(h, w, Cc):
    from gcc_amd import _lib
    most = min(h * w, _lib.MAP_MEAN_MAX_SEGMENTS)
    mine = _ops().map_mean_segments(h, w, Cc)
    assert 1 <= mine <= most
    return sorted({s for s in (1, 2, mine, most) if s <= most})


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('P', sorted(SHAPES))
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float32), ids=('bf16', 'fp32'))
def test_integer_maps_are_averaged_exactly_at_every_split(dtype, P):
    """integer-valued maps (|v| <= 256: bf16 holds them): out must equal float32(float64(S) / float64(P)) bit for bit, S the sum
    in integers, for every width, N in {1, 3}, a window inside wider pixels (ld > C, off > 0) with NaN in every gap lane and
    behind the last pixel, and for `segments` in {1, 2, the library's, the maximum}: a pixel dropped or counted twice at a seam
    changes S."""
    h, w = SHAPES[P]
    ch = _chunk(dtype)
    g = torch.Generator().manual_seed(1000 + P)
    for Cc in WIDTHS[dtype]:
        for N in (1, 3):
            vals = torch.randint(-256, 257, (N, h, w, Cc), generator=g)
            S = vals.to(torch.int64).sum((1, 2)).numpy()
            want = np.array([[np.float32(np.float64(int(s)) / np.float64(P)) for s in row] for row in S], dtype=np.float32)
            want = torch.from_numpy(want)
            views = [_window(vals, dtype, Cc + 2 * ch, ch)]
            if Cc == 24:
                views.append(_window(vals, dtype, Cc, 0))                     # and a map that fills its pixels
            for view in views:
                for seg in [0] + _segment_choices(h, w, Cc):
                    got = _mean(view, seg)
                    assert torch.equal(_bits(got), _bits(want)), (str(dtype), P, Cc, N, seg, view.stride())


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float32), ids=('bf16', 'fp32'))
def test_gaussian_maps_at_the_real_tap_shapes_within_the_rounding_bound(dtype):
    """N = 2 Gaussian maps (mean 0.5, as a map behind a ReLU is not centred) at 73 x 73 x 64, 35 x 35 x 192, 17 x 17 x 768:
    |got - m| <= 2^-24 |m| + P 2^-52 mean|x| with m the fsum mean -- the final rounding plus any-order f64 summation.  The bound
    itself is below 1e-6 max(|m|, 1e-3): a statement about rounding, not a tolerance.  Also: two runs give the same bits, and
    image n alone gives the bits it had in the batch."""
    ops = _ops()
    for h, w, Cc in TAPS:
        g = torch.Generator().manual_seed(h)
        vals = (torch.randn((2, h, w, Cc), generator=g) + 0.5).to(dtype)
        view = _window(vals, dtype, Cc + _chunk(dtype), 0)
        m, bound = T.mean_bound(vals.permute(0, 3, 1, 2))
        assert bool((bound < 1e-6 * np.maximum(np.abs(m), 1e-3)).all())
        got = _mean(view)
        err = np.abs(got.double().numpy() - m)
        print('%s %d x %d x %d: segments %d, max err / bound %.3f, max bound %.3g'
              % (str(dtype), h, w, Cc, ops.map_mean_segments(h, w, Cc), float((err / bound).max()), float(bound.max())))
        assert bool((err <= bound).all())
        assert torch.equal(_bits(_mean(view)), _bits(got))
        for n in range(2):
            alone = _mean(_window(vals[n:n + 1], dtype, Cc, 0))             # another ld as well: the order does not depend on it
            assert torch.equal(_bits(alone), _bits(got[n:n + 1])), (h, w, Cc, n)


def test_launch_counts_and_the_library_s_split():
    """at most two launches per call, one when one range is in use; the split is a function of h w and C alone"""
    ops = _ops()
    L = ops.lib()
    for dtype in (torch.bfloat16, torch.float32):
        for (h, w, Cc) in TAPS + ((3, 3, 96), (1, 1, 8)):
            view = _window(torch.ones((2, h, w, Cc)), dtype, Cc, 0)
            for seg in [0] + _segment_choices(h, w, Cc):
                torch.cuda.synchronize()
                before = L.gcc_launch_count(0)
                _mean(view, seg)
                n = L.gcc_launch_count(0) - before
                used = seg or ops.map_mean_segments(h, w, Cc)
                assert n == (1 if used == 1 else 2) == ops.map_mean_launches(h, w, Cc, seg), (h, w, Cc, seg, n)
    assert ops.map_mean_segments(73, 73, 64) == ops.map_mean_segments(1, 5329, 64) == ops.map_mean_segments(5329, 1, 64)
    assert L.gcc_map_mean_segments(0, 3, 8) == 0 and L.gcc_map_mean_segments(3, 3, 6) == 0
    assert L.gcc_map_mean_workspace(2, 73, 73, 64) == 2 * 64 * 64 * 8 and L.gcc_map_mean_workspace(2, 3, 3, 8) == 2 * 9 * 8 * 8
    assert L.gcc_map_mean_workspace(0, 3, 3, 8) == 0


def test_every_refusal_launches_nothing():
    from gcc_amd import _lib
    ops = _ops()
    L = ops.lib()
    N, h, w, Cc = 2, 6, 6, 16
    most = min(h * w, _lib.MAP_MEAN_MAX_SEGMENTS)
    out = torch.full((N * Cc,), -7.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(L.gcc_map_mean_workspace(N, h, w, Cc), dtype=torch.uint8, device=DEV)
    assert ws.numel() == N * most * Cc * 8
    for fn, dtype, ch in ((L.gcc_map_mean, torch.bfloat16, 8), (L.gcc_map_mean_f32, torch.float32, 4)):
        x = torch.ones((N * h * w * 32,), dtype=dtype, device=DEV)
        es = x.element_size()

        def call(xp=x.data_ptr(), ld=32, off=ch, N=N, h=h, w=w, C=Cc, seg=2, op=out.data_ptr(), wp=ws.data_ptr(), wb=ws.numel()):
            return fn(xp, ld, off, N, h, w, C, seg, op, wp, wb, ops.stream())
        torch.cuda.synchronize()
        before = L.gcc_launch_count(0)
        assert call(xp=0) == BAD_ARG and call(op=0) == BAD_ARG and call(wp=0) == BAD_ARG
        assert call(N=0) == BAD_ARG and call(h=0) == BAD_ARG and call(w=-1) == BAD_ARG and call(C=0) == BAD_ARG
        assert call(ld=32 + ch // 2) == BAD_ARG and call(off=ch // 2) == BAD_ARG                 # off the chunk grid
        assert call(ld=16, off=ch) == BAD_ARG                                                    # ld < off + C
        assert call(xp=x.data_ptr() + es) == BAD_ARG and call(op=out.data_ptr() + 4) == BAD_ARG   # alignment
        assert call(seg=-1) == BAD_ARG and call(seg=most + 1) == BAD_ARG
        assert call(h=1, w=1, seg=2) == BAD_ARG                                                  # more ranges than pixels
        assert call(C=Cc - ch // 2) == UNSUPPORTED                                               # no multiple of the chunk
        assert call(h=1 << 12, w=1 << 12) == UNSUPPORTED and call(N=1 << 20, h=1 << 10, w=1 << 10) == UNSUPPORTED
        assert call(wb=N * 2 * Cc * 8 - 1) == WORKSPACE and call(seg=most, wb=N * most * Cc * 8 - 8) == WORKSPACE
        torch.cuda.synchronize()
        assert L.gcc_launch_count(0) == before
        assert bool((out == -7.0).all())
        # one range writes nothing to ws: it may be absent
        assert call(seg=1, wp=0, wb=0) == 0 and L.gcc_launch_count(0) == before + 1
        assert call(wb=N * 2 * Cc * 8) == 0 and L.gcc_launch_count(0) == before + 3
        torch.cuda.synchronize()
        assert bool((out == 1.0).all())
        out.fill_(-7.0)
