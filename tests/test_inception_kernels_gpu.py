"""The streaming kernels of the native FID Inception network (gcc_amd/csrc/inception.hip) and the rectangular-kernel route
(gcc_border_copy + a padding-0 gcc_conv_eval_ex with KH != KW), per element against float64 torch on the CPU from the same
bf16-rounded inputs.  A bf16 store allows 2^-8 relative (half a unit in the last of its 8 significant bits) against the unrounded
reference; what the fp32 arithmetic in front of the store may add is counted from the element's own terms."""
import pytest
import torch
import torch.nn.functional as F

from tests._perelem import report, within

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG, UNSUPPORTED = -1, -2
BF16 = 2.0 ** -8
F32 = 2.0 ** -24
MAX_S2, MAX_S1P1, AVG_S1P1 = 0, 1, 2


def _bits(shape, seed):
    """bf16 tensor of arbitrary finite bit patterns"""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 1 << 16, shape, generator=g, dtype=torch.int32)
    b = torch.where((b & 0x7f80) == 0x7f80, b & 0x807f, b)
    return b.to(torch.int16).view(torch.bfloat16)


def _randn_bf16(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---- gcc_fid_resize ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,size', [((2, 3, 5, 7), (11, 9)), ((1, 3, 20, 13), (7, 9)), ((1, 3, 64, 64), (299, 299)),
                                        ((1, 3, 300, 301), (299, 299)), ((1, 3, 1, 1), (4, 4))])
def test_fid_resize_against_interpolate(shape, size):
    """2 bilinear(x) - 1 against F.interpolate in fp32 on the CPU, then one bf16 rounding.  Both sides evaluate the same fp32
    formula up to the order of a handful of operations on values of magnitude <= 1 (|2 v| + 1 <= 3): 8 fp32 ulps of 3 in front of
    the rounding, 2^-8 relative for the rounding itself (against the unrounded value).  Where both sides' fp32 values round the
    same way the bf16 results are equal: all but the few pixels within an fp32 ulp of a rounding boundary."""
    from gcc_amd import ops
    N, _, H, W = shape
    x = torch.rand(shape, generator=torch.Generator().manual_seed(H * 1000 + W))
    want = (2 * F.interpolate(x, size=size, mode='bilinear', align_corners=False) - 1)
    ref = want.bfloat16().double()
    bound = BF16 * want.abs().double() + 8 * F32 * 3
    buf = ops.new_act(N, 8, size[0], size[1], DEV)
    buf.copy_(_bits((N, 8, size[0], size[1]), 5).to(DEV))                 # pad channels must be WRITTEN as zeros
    ops.fid_resize(x.to(DEV), buf[:, :3])
    got = buf.cpu()
    assert (got[:, 3:].view(torch.int16) == 0).all()
    worst = within(got[:, :3].double(), want.double(), bound, 'fid_resize %s -> %s' % (shape, size))
    exact = float((got[:, :3].double() == ref).double().mean())
    report('fid_resize', shape + size, worst=worst, exact=exact)
    assert exact > 0.99                                   # a shifted tap or a wrong weight would move nearly every pixel


# ---- gcc_pool3x3 ------------------------------------------------------------------------------------------------------------
POOL_CASES = [(2, 24, 32, 8, 7, 5), (1, 8, 8, 0, 3, 3), (1, 16, 16, 0, 1, 1), (3, 40, 40, 0, 17, 17), (1, 8, 8, 0, 8, 8)]


@pytest.mark.parametrize('mode', [MAX_S2, MAX_S1P1, AVG_S1P1])
@pytest.mark.parametrize('N,Cc,ld,off,H,W', POOL_CASES)
def test_pool3x3(mode, N, Cc, ld, off, H, W):
    from gcc_amd import ops
    L = ops.lib()
    x = _randn_bf16((N, H, W, ld), 7 * H + W + Cc)
    win = x[..., off:off + Cc].permute(0, 3, 1, 2)
    xd = x.to(DEV)
    if mode == MAX_S2 and (H < 3 or W < 3):
        y = torch.zeros((N, 1, 1, ld), dtype=torch.bfloat16, device=DEV)
        L.gcc_launch_count(1)
        assert L.gcc_pool3x3(mode, xd.data_ptr(), ld, off, y.data_ptr(), ld, off, N, H, W, Cc, None) == UNSUPPORTED
        assert L.gcc_launch_count(0) == 0
        return
    Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == MAX_S2 else (H, W)
    before = _bits((N, Ho, Wo, ld), 11)
    y = before.to(DEV)
    assert L.gcc_pool3x3(mode, xd.data_ptr(), ld, off, y.data_ptr(), ld, off, N, H, W, Cc, None) == 0
    got = y.cpu()
    keep = torch.ones(ld, dtype=torch.bool)
    keep[off:off + Cc] = False
    assert _same_bits(got[..., keep], before[..., keep])                  # channels outside the slice are left as found
    g = got[..., off:off + Cc].permute(0, 3, 1, 2)
    if mode != AVG_S1P1:
        want = F.max_pool2d(win.float(), 3, 2, 0) if mode == MAX_S2 else F.max_pool2d(win.float(), 3, 1, 1)
        assert _same_bits(g, want.bfloat16())
        return
    # average excluding the padding: an fp32 sum of `count` terms (count - 1 roundings of at most sum |x|), a division, a bf16 store
    ones = torch.ones((1, 1, H, W), dtype=torch.float64)
    count = F.avg_pool2d(ones, 3, 1, 1, count_include_pad=True) * 9
    assert count.min() >= 1 and (H > 1 or W > 1 or count.max() == 1)      # corners 4, edges 6, inside 9; the 1 x 1 map: 1
    sums = F.avg_pool2d(win.double(), 3, 1, 1, count_include_pad=True) * 9
    mags = F.avg_pool2d(win.double().abs(), 3, 1, 1, count_include_pad=True) * 9
    want = sums / count
    assert torch.allclose(want, F.avg_pool2d(win.double(), 3, 1, 1, count_include_pad=False), rtol=1e-12, atol=1e-12)
    bound = BF16 * want.abs() + 10 * F32 * mags / count
    worst = within(g.double(), want, bound + 0 * want, 'avgpool %s' % ((N, Cc, H, W),))
    report('pool3x3_avg', (N, Cc, H, W), worst=worst)
    if H == 1 and W == 1:
        assert _same_bits(g, win)                                         # count 1: the pixel itself


# ---- gcc_border_copy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,Cc,ld,off,H,W,ph,pw', [(2, 24, 32, 8, 5, 4, 0, 3), (2, 24, 32, 8, 5, 4, 3, 0), (1, 8, 8, 0, 1, 1, 1, 1)])
def test_border_copy_bit_exact(N, Cc, ld, off, H, W, ph, pw):
    from gcc_amd import ops
    L = ops.lib()
    src = _bits((N, H, W, ld), 3 * H + ph)
    Hd, Wd = H + 2 * ph, W + 2 * pw
    before = torch.full((N, Hd, Wd, ld), 0x7fc1, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)      # NaN bit patterns
    dst = before.to(DEV)
    assert L.gcc_border_copy(src.to(DEV).data_ptr(), ld, off, dst.data_ptr(), ld, off, N, H, W, Cc, ph, pw, None) == 0
    got = dst.cpu()
    want = before.clone()
    want[..., off:off + Cc] = 0
    want[:, ph:ph + H, pw:pw + W, off:off + Cc] = src[..., off:off + Cc]
    assert _same_bits(got, want)                                          # the middle, the zero border, and nothing else


# ---- gcc_global_avgpool -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,Cc,h,w', [(3, 48, 8, 8), (1, 8, 1, 1), (2, 2048, 8, 8)])
def test_global_avgpool(N, Cc, h, w):
    """1e-6 relative to the mean magnitude of the element's own terms: eight interleaved fp32 partial sums and a three-level
    tree are at most 10 roundings on 64 pixels, and the division one more: 11 x 2^-24 = 6.6e-7"""
    from gcc_amd import ops
    ld, off = Cc + 8, 8
    x = _randn_bf16((N, h, w, ld), Cc + h)
    win = x[..., off:off + Cc]
    xd = x.to(DEV)
    out = torch.full((N, Cc), float('nan'), dtype=torch.float32, device=DEV)
    assert ops.lib().gcc_global_avgpool(xd.data_ptr(), ld, off, N, h, w, Cc, out.data_ptr(), None) == 0
    want = win.double().mean((1, 2))
    bound = 1e-6 * win.double().abs().mean((1, 2))
    worst = within(out.cpu().double(), want, bound, 'global_avgpool %s' % ((N, Cc, h, w),))
    report('global_avgpool', (N, Cc, h, w), worst=worst)
    v = ops.new_act(N, Cc, h, w, DEV)
    v.copy_(win.permute(0, 3, 1, 2).to(DEV))
    assert torch.equal(ops.global_avgpool(v).cpu(), out.cpu())            # the wrapper, and the same bits at another ld


# ---- rectangular convolutions: border copy + a padding-0 call -----------------------------------------------------------------
RECT_CASES = [((1, 7), 2, 16, 24, 6, 9), ((7, 1), 2, 16, 24, 6, 9), ((1, 3), 1, 40, 48, 8, 8), ((3, 1), 1, 40, 48, 8, 8),
              ((1, 7), 3, 128, 192, 17, 17), ((7, 1), 1, 64, 64, 17, 17)]


@pytest.mark.parametrize('kernel,N,Ci,Co,H,W', RECT_CASES)
def test_rectangular_conv_through_the_border_copy(kernel, N, Ci, Co, H, W):
    """relu(scale conv(x, w) + shift) with the kernel's own padding, into a channel slice of a wider buffer.  The products of bf16
    inputs are exact in fp32; K = kh kw Ci of them are summed in fp32 in the kernel's order (K roundings of at most sum |terms|),
    scale and shift add two roundings, the store one bf16 rounding."""
    from gcc_amd import _lib, ops
    kh, kw = kernel
    ph, pw = kh // 2, kw // 2
    g = torch.Generator().manual_seed(kh * 100 + Ci)
    x = torch.randn((N, Ci, H, W), generator=g).bfloat16()
    wgt = (torch.randn((Co, Ci, kh, kw), generator=g) * (2.0 / (Ci * kh * kw)) ** 0.5)
    scale, shift = 0.5 + torch.rand(Co, generator=g), torch.randn(Co, generator=g) * 0.1
    wb = wgt.bfloat16()
    z = F.conv2d(x.double(), wb.double(), None, 1, (ph, pw))
    mag = F.conv2d(x.double().abs(), wb.double().abs(), None, 1, (ph, pw))
    s, b = scale.double()[None, :, None, None], shift.double()[None, :, None, None]
    pre = z * s + b
    want = F.relu(pre)
    K = kh * kw * Ci
    pre_err = (K + 2) * F32 * (mag * s.abs() + b.abs())
    bound = BF16 * (want + pre_err) + pre_err
    xd = ops.new_act(N, Ci, H, W, DEV)
    xd.copy_(x.to(DEV))
    xb = ops.new_act(N, Ci, H + 2 * ph, W + 2 * pw, DEV)
    xb.copy_(_bits((N, Ci, H + 2 * ph, W + 2 * pw), 9).to(DEV))
    wide = ops.new_act(N, Co + 24, H, W, DEV)
    sentinel = _bits((N, Co + 24, H, W), 13)
    wide.copy_(sentinel.to(DEV))
    out = ops.cslice(wide, 16, Co)
    w, _ = ops.pack_weights(wgt.to(DEV).contiguous(memory_format=torch.channels_last), want_w=True, want_wt=False)
    ops.border_copy(xd, xb, ph, pw)
    launches = ops.conv_eval_rect(xb, w, Co, kernel, 1, out, route_only=True)
    assert launches in (1, 2)
    L = ops.lib()
    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    ops.conv_eval_rect(xb, w, Co, kernel, 1, out, scale=scale.to(DEV), shift=shift.to(DEV), act=_lib.EVAL_ACT_RELU)
    torch.cuda.synchronize()
    assert L.gcc_launch_count(1) == launches
    got = wide.cpu()
    assert _same_bits(got[:, :16], sentinel[:, :16]) and _same_bits(got[:, 16 + Co:], sentinel[:, 16 + Co:])
    worst = within(got[:, 16:16 + Co].double(), want, bound, 'conv %s %d -> %d' % (kernel, Ci, Co))
    report('rect_conv', kernel + (N, Ci, Co, H, W), worst=worst)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_the_inception_kernels_refuse_bad_arguments_without_a_launch():
    from gcc_amd import ops
    L = ops.lib()
    x = torch.zeros(4 * 8 * 8 * 32, dtype=torch.bfloat16, device=DEV)
    y = torch.zeros_like(x)
    f = torch.zeros(3 * 16 * 16, dtype=torch.float32, device=DEV)
    xp, yp, fp = x.data_ptr(), y.data_ptr(), f.data_ptr()
    L.gcc_launch_count(1)
    rs = lambda *a: L.gcc_fid_resize(*a, None)
    assert rs(None, 1, 16, 16, yp, 8, 0, 8, 8) == BAD_ARG
    assert rs(fp, 1, 16, 16, None, 8, 0, 8, 8) == BAD_ARG
    assert rs(fp, 0, 16, 16, yp, 8, 0, 8, 8) == BAD_ARG
    assert rs(fp, 1, 16, 0, yp, 8, 0, 8, 8) == BAD_ARG
    assert rs(fp, 1, 16, 16, yp, 8, 0, 8, -1) == BAD_ARG
    assert rs(fp, 1, 16, 16, yp, 12, 0, 8, 8) == BAD_ARG                 # ld no multiple of 8
    assert rs(fp, 1, 16, 16, yp, 16, 4, 8, 8) == BAD_ARG                 # offset no multiple of 8
    assert rs(fp, 1, 16, 16, yp, 8, 8, 8, 8) == BAD_ARG                  # the 8-channel window does not fit its ld
    assert rs(fp, 1, 16, 16, yp + 2, 8, 0, 8, 8) == BAD_ARG              # misaligned pointer
    pl = lambda *a: L.gcc_pool3x3(*a, None)
    assert pl(AVG_S1P1, None, 32, 0, yp, 32, 0, 1, 8, 8, 8) == BAD_ARG
    assert pl(AVG_S1P1, xp, 32, 0, None, 32, 0, 1, 8, 8, 8) == BAD_ARG
    assert pl(3, xp, 32, 0, yp, 32, 0, 1, 8, 8, 8) == BAD_ARG             # no such mode
    assert pl(MAX_S2, xp, 30, 0, yp, 32, 0, 1, 8, 8, 8) == BAD_ARG
    assert pl(MAX_S2, xp, 32, 0, yp, 32, 4, 1, 8, 8, 8) == BAD_ARG
    assert pl(MAX_S2, xp, 32, 16, yp, 32, 0, 1, 8, 8, 24) == BAD_ARG      # the window does not fit its ld
    assert pl(MAX_S1P1, xp, 32, 0, yp, 32, 0, 0, 8, 8, 8) == BAD_ARG
    assert pl(MAX_S1P1, xp, 32, 0, yp, 32, 0, 1, 8, 8, 0) == BAD_ARG
    assert pl(MAX_S1P1, xp, 32, 0, yp, 32, 0, 1, 8, 8, 12) == UNSUPPORTED  # channels no multiple of 8
    assert pl(MAX_S2, xp, 32, 0, yp, 32, 0, 1, 2, 8, 8) == UNSUPPORTED    # no output pixel
    bc = lambda *a: L.gcc_border_copy(*a, None)
    assert bc(None, 32, 0, yp, 32, 0, 1, 4, 4, 8, 1, 1) == BAD_ARG
    assert bc(xp, 32, 0, None, 32, 0, 1, 4, 4, 8, 1, 1) == BAD_ARG
    assert bc(xp, 32, 0, yp, 32, 0, 1, 4, 4, 8, -1, 1) == BAD_ARG
    assert bc(xp, 32, 0, yp, 32, 0, 1, 0, 4, 8, 1, 1) == BAD_ARG
    assert bc(xp, 32, 0, yp, 20, 0, 1, 4, 4, 8, 1, 1) == BAD_ARG
    assert bc(xp, 32, 12, yp, 32, 0, 1, 4, 4, 8, 1, 1) == BAD_ARG
    assert bc(xp, 32, 0, xp, 32, 8, 1, 4, 4, 8, 1, 1) == BAD_ARG          # never in place
    assert bc(xp, 32, 0, yp, 32, 0, 1, 4, 4, 12, 1, 1) == UNSUPPORTED
    ga = lambda *a: L.gcc_global_avgpool(*a, None)
    assert ga(None, 32, 0, 1, 4, 4, 8, fp) == BAD_ARG
    assert ga(xp, 32, 0, 1, 4, 4, 8, None) == BAD_ARG
    assert ga(xp, 32, 0, 1, 4, 0, 8, fp) == BAD_ARG
    assert ga(xp, 32, 0, -1, 4, 4, 8, fp) == BAD_ARG
    assert ga(xp, 28, 0, 1, 4, 4, 8, fp) == BAD_ARG
    assert ga(xp, 32, 4, 1, 4, 4, 8, fp) == BAD_ARG
    assert ga(xp, 32, 0, 1, 4, 4, 8, fp + 4) == BAD_ARG                   # the output is written 16 bytes at a time
    assert ga(xp, 32, 0, 1, 4, 4, 12, fp) == UNSUPPORTED
    assert L.gcc_launch_count(0) == 0
    torch.cuda.synchronize()
    assert (x == 0).all() and (y == 0).all() and (f == 0).all()
