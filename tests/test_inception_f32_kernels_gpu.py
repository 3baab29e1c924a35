"""The fp32 twins of the FID Inception network's streaming kernels (gcc_fid_resize_f32, gcc_pool3x3_f32, gcc_global_avgpool_f32:
gcc_amd/csrc/inception.hip on NHWC fp32 maps), per element against float64 torch on the CPU from the same fp32 inputs, at the
shapes and the ld / off windows tests/test_inception_kernels_gpu.py uses for the bf16 kernels.  There is no rounding of a store
here: every bound counts the fp32 operations in front of it from the element's own terms."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._perelem import report, within

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG, UNSUPPORTED = -1, -2
F32 = 2.0 ** -24
MAX_S2, MAX_S1P1, AVG_S1P1 = 0, 1, 2
SENTINEL = -1234.5625


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- gcc_fid_resize_f32 -------------------------------------------------------------------------------------------------------
def _taps(n_in, n_out):
    """torch's source index of align_corners = False as its fp32 path computes it (area_pixel_compute_source_index<float>:
    max(0, (o + 0.5) (in / out) - 0.5) with the fp32 ratio of the sizes; the product and the subtraction are ONE fused
    multiply-add, as torch's builds and the kernel's compiler contract them -- exact in float64 here, rounded to fp32 once):
    lower tap, upper tap, the upper tap's fp32 weight.  With two roundings instead, 97 of the 268203 values of 64 -> 299 move by
    up to 1.8e-6: the test that the taps are torch's is the first assertion of test_fid_resize_f32_against_float64."""
    scale = np.float32(n_in) / np.float32(n_out)
    s = (np.float64(scale) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5).astype(np.float32)
    s = np.maximum(s, np.float32(0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip(s - i0.astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1)


def _resize64(x, size):
    """2 bilinear(x) - 1 in float64 from the fp32 taps and weights (the weights 1 - l are fp32 values too, as torch forms them)"""
    y0, y1, ly = _taps(x.shape[2], size[0])
    x0, x1, lx = _taps(x.shape[3], size[1])
    ky, kx = (1 - ly).double(), (1 - lx).double()
    ly, lx = ly.double(), lx.double()
    x = x.double()
    r0, r1 = x[:, :, y0], x[:, :, y1]
    top = r0[..., x0] * kx + r0[..., x1] * lx
    bot = r1[..., x0] * kx + r1[..., x1] * lx
    return 2 * (top * ky[:, None] + bot * ly[:, None]) - 1


@pytest.mark.parametrize('shape,size', [((2, 3, 5, 7), (11, 9)), ((1, 3, 20, 13), (7, 9)), ((1, 3, 64, 64), (299, 299)),
                                        ((1, 3, 300, 301), (299, 299)), ((1, 3, 1, 1), (4, 4))])
def test_fid_resize_f32_against_float64(shape, size):
    """2 bilinear(x) - 1 per element against float64 on the CPU, within 8 fp32 ulps of 3 (values of magnitude <= 1, |2 v| + 1 <=
    3: the bound tests/test_inception_kernels_gpu.py gives the fp32 arithmetic in front of its bf16 store), enlarging and
    shrinking.

    The float64 reference blends with the taps and weights of torch's FP32 path, which are the kernel's definition
    (include/gcc_hip.h) and what the fp32 reference network computes.  F.interpolate of the float64 image forms its source index
    in float64 instead: at 300 x 301 -> 299 x 299 that alone moves the result by 6.7e-5 (host measurement, these inputs; 6.4e-6 at
    64 -> 299), 47 times the bound, whatever the kernel does -- and a kernel that followed it would leave the reference's own
    arithmetic.  Where the fp32 index is exact (size ratios that are powers of two) the two references are one, and
    F.interpolate of the float64 image is the reference: test_fid_resize_f32_against_float64_interpolate.  F.interpolate's
    own fp32 result is held to the same bound against the same reference first (host measurement: 0.10 to 0.15 of it), which
    pins the restated taps to torch's; the kernel's distance to it is printed."""
    from gcc_amd import ops
    N, _, H, W = shape
    x = torch.rand(shape, generator=torch.Generator().manual_seed(H * 1000 + W))
    want = _resize64(x, size)
    torch32 = (2 * F.interpolate(x, size=size, mode='bilinear', align_corners=False) - 1).double()
    bound = torch.full(want.shape, 8 * F32 * 3, dtype=torch.float64)
    assert (torch32 - want).abs().max() <= bound.max()                     # the restated taps ARE this torch's fp32 taps
    for ld, off in ((4, 0), (12, 8)):                                      # the 3-in-4 input, and a window of a wider map
        buf = torch.full((N, size[0], size[1], ld), SENTINEL, dtype=torch.float32, device=DEV)
        ops.fid_resize_f32(x.to(DEV), buf.permute(0, 3, 1, 2)[:, off:off + 3])
        got = buf.cpu()
        assert (got[..., off + 3] == 0).all()                              # the pad channel is WRITTEN as zero
        assert (got[..., :off] == SENTINEL).all()                          # nothing in front of the window is touched
        g = got[..., off:off + 3].permute(0, 3, 1, 2)
        worst = within(g.double(), want, bound, 'fid_resize_f32 %s -> %s' % (shape, size))
        report('fid_resize_f32', shape + size, worst=worst, torch32=float((g.double() - torch32).abs().max()) / (8 * F32 * 3))


@pytest.mark.parametrize('hw,size', [((8, 8), (32, 32)), ((32, 16), (8, 4)), ((16, 4), (64, 2))])
def test_fid_resize_f32_against_float64_interpolate(hw, size):
    """F.interpolate of the float64 image as the reference where every source index is exact in fp32 (size ratios that are powers
    of two): 8 fp32 ulps of 3, enlarging, shrinking, and both in one call"""
    from gcc_amd import ops
    x = torch.rand((2, 3) + hw, generator=torch.Generator().manual_seed(hw[0]))
    want = 2 * F.interpolate(x.double(), size=size, mode='bilinear', align_corners=False) - 1
    assert torch.equal(want, _resize64(x, size)) or float((want - _resize64(x, size)).abs().max()) < 1e-15
    out = ops.new_act_f32(2, 3, size[0], size[1], DEV)
    ops.fid_resize_f32(x.to(DEV), out)
    bound = torch.full(want.shape, 8 * F32 * 3, dtype=torch.float64)
    report('fid_resize_f32_f64', hw + size, worst=within(out.cpu().double(), want, bound, 'fid_resize_f32 against float64 interpolate'))


# ---- gcc_pool3x3_f32 ------------------------------------------------------------------------------------------------------------
POOL_CASES = [(2, 24, 32, 8, 7, 5), (1, 8, 8, 0, 3, 3), (1, 16, 16, 0, 1, 1), (3, 40, 40, 0, 17, 17), (1, 8, 8, 0, 8, 8),
              (2, 4, 12, 4, 5, 6)]                                         # the last: one 4-channel chunk on the 4-float grid


@pytest.mark.parametrize('mode', [MAX_S2, MAX_S1P1, AVG_S1P1])
@pytest.mark.parametrize('N,Cc,ld,off,H,W', POOL_CASES)
def test_pool3x3_f32(mode, N, Cc, ld, off, H, W):
    from gcc_amd import ops
    L = ops.lib()
    x = _randn((N, H, W, ld), 7 * H + W + Cc)
    win = x[..., off:off + Cc].permute(0, 3, 1, 2)
    xd = x.to(DEV)
    if mode == MAX_S2 and (H < 3 or W < 3):
        y = torch.zeros((N, 1, 1, ld), dtype=torch.float32, device=DEV)
        L.gcc_launch_count(1)
        assert L.gcc_pool3x3_f32(mode, xd.data_ptr(), ld, off, y.data_ptr(), ld, off, N, H, W, Cc, None) == UNSUPPORTED
        assert L.gcc_launch_count(0) == 0
        return
    Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == MAX_S2 else (H, W)
    before = _randn((N, Ho, Wo, ld), 11)
    y = before.to(DEV)
    assert L.gcc_pool3x3_f32(mode, xd.data_ptr(), ld, off, y.data_ptr(), ld, off, N, H, W, Cc, None) == 0
    got = y.cpu()
    keep = torch.ones(ld, dtype=torch.bool)
    keep[off:off + Cc] = False
    assert _same_bits(got[..., keep], before[..., keep])                  # channels outside the slice are left as found
    g = got[..., off:off + Cc].permute(0, 3, 1, 2)
    if mode != AVG_S1P1:
        want = F.max_pool2d(win, 3, 2, 0) if mode == MAX_S2 else F.max_pool2d(win, 3, 1, 1)
        assert _same_bits(g, want)                                        # a maximum is one of the inputs, bit for bit
        return
    # average excluding the padding: an fp32 sum of `count` terms in tap order (count - 1 roundings of at most sum |x|; the bound
    # allows `count`) and one IEEE division: (taps + 1) 2^-24 sum |x| / count
    ones = torch.ones((1, 1, H, W), dtype=torch.float64)
    count = F.avg_pool2d(ones, 3, 1, 1, count_include_pad=True) * 9
    count = count.round()
    assert count.min() >= 1 and (H > 1 or W > 1 or count.max() == 1)      # corners 4, edges 6, inside 9; the 1 x 1 map: 1
    if H >= 3 and W >= 3:
        assert count[0, 0, 0, 0] == 4 and count[0, 0, 0, 1] == 6 and count[0, 0, 1, 1] == 9
    sums = F.avg_pool2d(win.double(), 3, 1, 1, count_include_pad=True) * 9
    mags = F.avg_pool2d(win.double().abs(), 3, 1, 1, count_include_pad=True) * 9
    want = sums / count
    assert torch.allclose(want, F.avg_pool2d(win.double(), 3, 1, 1, count_include_pad=False), rtol=1e-12, atol=1e-12)
    bound = (count + 1) * F32 * mags / count
    worst = within(g.double(), want, bound + 0 * want, 'avgpool_f32 %s' % ((N, Cc, H, W),))
    report('pool3x3_f32_avg', (N, Cc, H, W), worst=worst)
    if H == 1 and W == 1:
        assert _same_bits(g, win)                                         # count 1: the pixel itself
    out = ops.new_act_f32(N, Cc, H, W, DEV)                               # the wrapper, and the same bits at another ld
    v = ops.new_act_f32(N, Cc, H, W, DEV)
    v.copy_(win.to(DEV))
    assert _same_bits(ops.pool3x3_f32(mode, v, out).cpu(), g)


# ---- gcc_global_avgpool_f32 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,Cc,h,w', [(3, 48, 8, 8), (1, 8, 1, 1), (2, 24, 3, 3), (2, 2048, 8, 8), (2, 4, 3, 3)])
def test_global_avgpool_f32(N, Cc, h, w):
    """(hw + 1) 2^-24 mean |x| per element: a sum of hw fp32 terms takes fewer than hw roundings in any order (eight interleaved
    partial sums and a three-level tree: at most 10 on 64 pixels), the division one more"""
    from gcc_amd import ops
    ld, off = Cc + 8, 8
    x = _randn((N, h, w, ld), Cc + h)
    win = x[..., off:off + Cc]
    xd = x.to(DEV)
    out = torch.full((N, Cc + 4), float('nan'), dtype=torch.float32, device=DEV)
    assert ops.lib().gcc_global_avgpool_f32(xd.data_ptr(), ld, off, N, h, w, Cc, out.data_ptr(), None) == 0
    flat = out.cpu().reshape(-1)
    assert torch.isnan(flat[N * Cc:]).all()                               # [N][C] dense, nothing behind it
    got = flat[:N * Cc].reshape(N, Cc)
    want = win.double().mean((1, 2))
    bound = (h * w + 1) * F32 * win.double().abs().mean((1, 2))
    worst = within(got.double(), want, bound, 'global_avgpool_f32 %s' % ((N, Cc, h, w),))
    report('global_avgpool_f32', (N, Cc, h, w), worst=worst)
    if h == 1 and w == 1:
        assert _same_bits(got, win.reshape(N, Cc))
    v = ops.new_act_f32(N, Cc, h, w, DEV)
    v.copy_(win.permute(0, 3, 1, 2).to(DEV))
    assert _same_bits(ops.global_avgpool_f32(v).cpu(), got)               # the wrapper, and the same bits at another ld


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_the_fp32_inception_kernels_refuse_bad_arguments_without_a_launch():
    from gcc_amd import ops
    L = ops.lib()
    x = torch.zeros(4 * 8 * 8 * 32, dtype=torch.float32, device=DEV)
    y = torch.zeros_like(x)
    f = torch.zeros(3 * 16 * 16, dtype=torch.float32, device=DEV)
    xp, yp, fp = x.data_ptr(), y.data_ptr(), f.data_ptr()
    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    rs = lambda *a: L.gcc_fid_resize_f32(*a, None)
    assert rs(None, 1, 16, 16, yp, 4, 0, 8, 8) == BAD_ARG
    assert rs(fp, 1, 16, 16, None, 4, 0, 8, 8) == BAD_ARG
    assert rs(fp, 0, 16, 16, yp, 4, 0, 8, 8) == BAD_ARG
    assert rs(fp, 1, 16, 0, yp, 4, 0, 8, 8) == BAD_ARG
    assert rs(fp, 1, 16, 16, yp, 4, 0, 8, -1) == BAD_ARG
    assert rs(fp, 1, 16, 16, yp, 6, 0, 8, 8) == BAD_ARG                  # ld no multiple of 4
    assert rs(fp, 1, 16, 16, yp, 8, 2, 8, 8) == BAD_ARG                  # offset no multiple of 4
    assert rs(fp, 1, 16, 16, yp, 4, 4, 8, 8) == BAD_ARG                  # the 4-channel window does not fit its ld
    assert rs(fp, 1, 16, 16, yp + 4, 4, 0, 8, 8) == BAD_ARG              # misaligned pointer
    pl = lambda *a: L.gcc_pool3x3_f32(*a, None)
    assert pl(AVG_S1P1, None, 32, 0, yp, 32, 0, 1, 8, 8, 8) == BAD_ARG
    assert pl(AVG_S1P1, xp, 32, 0, None, 32, 0, 1, 8, 8, 8) == BAD_ARG
    assert pl(3, xp, 32, 0, yp, 32, 0, 1, 8, 8, 8) == BAD_ARG             # no such mode
    assert pl(MAX_S2, xp, 30, 0, yp, 32, 0, 1, 8, 8, 8) == BAD_ARG
    assert pl(MAX_S2, xp, 32, 0, yp, 32, 2, 1, 8, 8, 8) == BAD_ARG
    assert pl(MAX_S2, xp, 32, 16, yp, 32, 0, 1, 8, 8, 24) == BAD_ARG      # the window does not fit its ld
    assert pl(MAX_S2, xp + 8, 32, 0, yp, 32, 0, 1, 8, 8, 8) == BAD_ARG    # misaligned pointer
    assert pl(MAX_S1P1, xp, 32, 0, yp, 32, 0, 0, 8, 8, 8) == BAD_ARG
    assert pl(MAX_S1P1, xp, 32, 0, yp, 32, 0, 1, 8, 8, 0) == BAD_ARG
    assert pl(MAX_S1P1, xp, 32, 0, yp, 32, 0, 1, 8, 8, 6) == UNSUPPORTED  # channels no multiple of 4
    assert pl(MAX_S2, xp, 32, 0, yp, 32, 0, 1, 2, 8, 8) == UNSUPPORTED    # no output pixel
    ga = lambda *a: L.gcc_global_avgpool_f32(*a, None)
    assert ga(None, 32, 0, 1, 4, 4, 8, fp) == BAD_ARG
    assert ga(xp, 32, 0, 1, 4, 4, 8, None) == BAD_ARG
    assert ga(xp, 32, 0, 1, 4, 0, 8, fp) == BAD_ARG
    assert ga(xp, 32, 0, -1, 4, 4, 8, fp) == BAD_ARG
    assert ga(xp, 30, 0, 1, 4, 4, 8, fp) == BAD_ARG
    assert ga(xp, 32, 2, 1, 4, 4, 8, fp) == BAD_ARG
    assert ga(xp, 32, 0, 1, 4, 4, 8, fp + 4) == BAD_ARG                   # the output is written 16 bytes at a time
    assert ga(xp, 32, 0, 1, 4, 4, 6, fp) == UNSUPPORTED
    assert L.gcc_launch_count(0) == 0
    torch.cuda.synchronize()
    assert (x == 0).all() and (y == 0).all() and (f == 0).all()
