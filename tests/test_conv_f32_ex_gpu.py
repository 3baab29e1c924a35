"""gcc_conv_eval_f32_ex (gcc_conv_eval_f32's kernel with KH, KW and the two paddings independent) against torch-CPU float64 at the
geometries of the FID Inception network: an exact layout check on integer data, a derived per-element bound on seeded normal data,
bit-equality with gcc_conv_eval_f32 where both serve, batch invariance bit for bit, and the refusals, at the smallest shapes at
which the kernel can still go wrong."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG, UNSUPPORTED = -1, -2
NONE, RELU = 0, 3
SENTINEL = -1234.5625
XOFF, YOFF = 4, 8                  # the input is read at channel 4 of an ld of ceil4(Ci) + 8, the output written at 8 of Co + 16

# (kh, kw), (ph, pw), stride: the kernels of the Inception network
GEOMS = {
    'r17': ((1, 7), (0, 3), 1), 'c71': ((7, 1), (3, 0), 1), 'r13': ((1, 3), (0, 1), 1), 'c31': ((3, 1), (1, 0), 1),
    'k5': ((5, 5), (2, 2), 1), 'k3p0': ((3, 3), (0, 0), 1), 'k3s2p0': ((3, 3), (0, 0), 2), 'k1': ((1, 1), (0, 0), 1),
}
# N = 2 on an odd 9 x 11 map: M (198, or 20 at stride 2) is no multiple of a tile and a tile straddles the images; K = 7 * 8 = 56
# and 7 * 24 = 168 end off the 16-wide k step; Co 8: the 128 x 32 tile, 40: a partial 64 x 64 tile, 72: a second column tile
CASES = {'%s_ci%d_co%d' % (g, ci, co): dict(g=g, N=2, H=9, W=11, Ci=ci, Co=co)
         for g in GEOMS for ci in (8, 24) for co in (8, 40, 72)}
CASES['stem'] = dict(g='k3s2p0', N=2, H=9, W=11, Ci=3, Co=8)              # the 3-in-4 input at stride 2, padding 0
CASES['stem_co40'] = dict(g='k3s2p0', N=2, H=9, W=11, Ci=3, Co=40)
CASES['big'] = dict(g='r17', N=2, H=128, W=128, Ci=8, Co=128)             # 32768 pixels x 128 channels: 256 tiles of 128 x 128
SMALL = [n for n in CASES if n != 'big']


class Geom:
    def __init__(self, name):
        c = CASES[name]
        (self.kh, self.kw), (self.ph, self.pw), self.s = GEOMS[c['g']]
        self.N, self.H, self.W, self.Ci, self.Co = (c[k] for k in ('N', 'H', 'W', 'Ci', 'Co'))
        self.Ho, self.Wo = (self.H + 2 * self.ph - self.kh) // self.s + 1, (self.W + 2 * self.pw - self.kw) // self.s + 1
        self.ldx, self.ldy = (self.Ci + 3) // 4 * 4 + 8, self.Co + 16
        self.K = self.kh * self.kw * self.Ci
        self.relu = self.Co == 40


@functools.lru_cache(maxsize=None)
def _data(name, kind):
    """(x, w, scale, shift) on the host in float64.  'int': x in [-3, 3], every weight a distinct integer of magnitude <= 8190
    (asymmetric: a swapped index shows), so every partial sum of the <= 600 products is an integer below 2^24 and exact in fp32;
    'normal': seeded normal data (fp32 values)"""
    q = Geom(name)
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + (1 if kind == 'int' else 2))
    if kind == 'int':
        x = torch.randint(-3, 4, (q.N, q.Ci, q.H, q.W), generator=g).double()
        idx = torch.arange(q.Co * q.Ci * q.kh * q.kw, dtype=torch.int64)
        w = ((idx * 7919) % 16381 - 8190).double().reshape(q.Co, q.Ci, q.kh, q.kw)
        return x, w, None, None
    x = torch.randn((q.N, q.Ci, q.H, q.W), generator=g).float().double()
    w = (torch.randn((q.Co, q.Ci, q.kh, q.kw), generator=g) * 0.2).float().double()
    scale = (torch.rand(q.Co, generator=g) + 0.5).float().double() * torch.where(torch.arange(q.Co) % 3 == 0, -1.0, 1.0)
    shift = (torch.randn(q.Co, generator=g) * 0.3).float().double()
    return x, w, scale, shift


@functools.lru_cache(maxsize=None)
def _want(name, kind):
    """float64 result and the per-element magnitude |scale| sum |x w| + |shift| of a case"""
    q = Geom(name)
    x, w, scale, shift = _data(name, kind)
    y = F.conv2d(x, w, None, q.s, (q.ph, q.pw))
    mag = F.conv2d(x.abs(), w.abs(), None, q.s, (q.ph, q.pw))
    if scale is not None:
        y = y * scale[None, :, None, None] + shift[None, :, None, None]
        mag = mag * scale.abs()[None, :, None, None] + shift.abs()[None, :, None, None]
    if q.relu and kind == 'normal':
        y = torch.relu(y)
    return y, mag


def _pack(w):
    from gcc_amd import ops
    return ops.pack_weights_f32(w.float().to(DEV))


def _nhwc(t, ld, off, fill):
    """[N, C, H, W] float64 host -> NHWC fp32 device buffer [N, H, W, ld] with the channels at `off`, `fill` everywhere else"""
    N, Cc, H, W = t.shape
    buf = torch.full((N, H, W, ld), fill, dtype=torch.float32)
    buf[..., off:off + Cc] = t.permute(0, 2, 3, 1).float()
    return buf.to(DEV)


def _desc(q, N=None, pad=0, **over):
    from gcc_amd import ops
    d = ops.conv_desc(N or q.N, q.H, q.W, q.Ci, q.Co, q.kh, q.s, pad, q.ldx, q.ldy)
    d.KW, d.xoff, d.yoff = q.kw, XOFF, YOFF
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _launch(q, xb, wp, yb, scale, shift, act, N=None):
    from gcc_amd import _lib, ops
    ep = _lib.eval_f32_epilogue_t(scale.data_ptr() if scale is not None else None, shift.data_ptr() if shift is not None else None,
                                  None, 0, 0, act, 1)
    return ops.lib().gcc_conv_eval_f32_ex(C.byref(_desc(q, N)), q.ph, q.pw, xb.data_ptr(), wp.data_ptr(), yb.data_ptr(), C.byref(ep),
                                          None)


def _run(name, kind, image=None):
    """(result [N, Co, Ho, Wo] on the host, the whole output buffer on the host) of a case -- or of its image `image` alone --
    through the library"""
    q = Geom(name)
    x, w, scale, shift = _data(name, kind)
    if image is not None:
        x = x[image:image + 1]
    N = x.shape[0]
    xb = _nhwc(x, q.ldx, XOFF, fill=9.0)                   # nothing outside the window is an input (the stem's 4th channel: ignored)
    yb = torch.full((N, q.Ho, q.Wo, q.ldy), SENTINEL, dtype=torch.float32, device=DEV)
    sc = scale.float().to(DEV) if scale is not None else None
    sh = shift.float().to(DEV) if shift is not None else None
    act = RELU if (q.relu and kind == 'normal') else NONE
    assert _launch(q, xb, _pack(w), yb, sc, sh, act, N=N) == 0, name
    out = yb.cpu()
    return out[..., YOFF:YOFF + q.Co].permute(0, 3, 1, 2).contiguous(), out


def _only_the_window_is_written(q, whole):
    keep = torch.ones(q.ldy, dtype=torch.bool)
    keep[YOFF:YOFF + q.Co] = False
    return bool((whole[..., keep] == SENTINEL).all())


# ---- 1. exact layout check ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_integer_data_is_exact(name):
    q = Geom(name)
    got, whole = _run(name, 'int')
    want, mag = _want(name, 'int')
    assert tuple(want.shape) == (q.N, q.Co, q.Ho, q.Wo)
    assert float(mag.max()) < 2 ** 24                        # every partial sum is exact in fp32
    assert torch.equal(got.double(), want), name
    assert _only_the_window_is_written(q, whole)


# ---- 2. seeded normal data, per element ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_normal_data_within_the_fmaf_chain_bound(name):
    """|got - f64| <= (K + 2) 2^-24 (|scale| sum |x w| + |shift|) per element: K fmaf roundings of the chain and the epilogue's
    fmaf (K + 1; the second-order terms of K = 600 roundings are 0.01 of one more); the inputs are fp32 values, the ReLU does
    not widen a difference"""
    q = Geom(name)
    got, whole = _run(name, 'normal')
    want, mag = _want(name, 'normal')
    bound = (q.K + 2) * 2.0 ** -24 * mag
    err = (got.double() - want).abs()
    print('%s: K %d, worst error / bound %.3f' % (name, q.K, float((err / bound).max())))
    assert (err <= bound).all(), name
    assert _only_the_window_is_written(q, whole)


# ---- 3. the old entry, the batch, the tile --------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,stride,dil,Ci,Co', [(3, 1, 1, 8, 40), (7, 2, 1, 3, 8), (3, 1, 2, 24, 72), (1, 2, 1, 8, 8)])
def test_same_bits_as_conv_eval_f32_where_both_serve(k, stride, dil, Ci, Co):
    from gcc_amd import ops
    g = torch.Generator().manual_seed(k * 10 + Ci)
    N, H, W = 2, 9, 11
    pad = dil * (k // 2)
    x = torch.randn((N, Ci, H, W), generator=g)
    w = ops.pack_weights_f32((torch.randn((Co, Ci, k, k), generator=g) * 0.2).to(DEV))
    scale, shift = (torch.rand(Co, generator=g) + 0.5).to(DEV), torch.randn(Co, generator=g).to(DEV)
    ld = (Ci + 3) // 4 * 4
    xv = _nhwc(x.double(), ld, 0, fill=0.0).permute(0, 3, 1, 2)[:, :Ci]
    Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    old, new = ops.new_act_f32(N, Co, Ho, Wo, DEV), ops.new_act_f32(N, Co, Ho, Wo, DEV)
    ops.conv_eval_f32(xv, w, Co, k, stride, pad, old, dilation=dil, scale=scale, shift=shift, act=RELU)
    ops.conv_eval_f32_ex(xv, w, Co, (k, k), stride, (pad, pad), new, dilation=dil, scale=scale, shift=shift, act=RELU)
    assert ops.conv_eval_f32(xv, w, Co, k, stride, pad, old, dilation=dil, route_only=True) == \
        ops.conv_eval_f32_ex(xv, w, Co, (k, k), stride, (pad, pad), new, dilation=dil, route_only=True) >= 0
    assert float(old.abs().max()) > 0
    assert torch.equal(old.cpu().view(torch.int32), new.cpu().view(torch.int32))


@pytest.mark.parametrize('name', ['r17_ci24_co72', 'c71_ci8_co8', 'k5_ci24_co40', 'k3s2p0_ci8_co72', 'stem'])
def test_an_image_alone_equals_the_image_in_its_batch_bit_for_bit(name):
    q = Geom(name)
    both, _ = _run(name, 'normal')
    for n in range(q.N):
        one, whole = _run(name, 'normal', image=n)
        assert _only_the_window_is_written(q, whole)
        assert torch.equal(one.view(torch.int32), both[n:n + 1].contiguous().view(torch.int32)), (name, n)


def test_every_tile_shape_is_exercised_and_the_tiles_agree():
    from gcc_amd import ops
    L = ops.lib()
    for name, route in (('big', 0), ('r17_ci8_co72', 1), ('r17_ci8_co40', 1), ('r17_ci8_co8', 2)):
        q = Geom(name)
        assert L.gcc_conv_eval_f32_ex_route(C.byref(_desc(q)), q.ph, q.pw, 1) == route, name
    # the first image of 'big' alone is 128 tiles: 64 x 64 ones.  Same bits as inside the batch's 128 x 128 tiles.
    q = Geom('big')
    assert L.gcc_conv_eval_f32_ex_route(C.byref(_desc(q, N=1)), q.ph, q.pw, 1) == 1
    both, _ = _run('big', 'normal')
    one, _ = _run('big', 'normal', image=0)
    assert torch.equal(one.view(torch.int32), both[:1].contiguous().view(torch.int32))


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_happen_before_any_launch():
    from gcc_amd import _lib, ops
    L = ops.lib()
    x = torch.zeros(2 * 8 * 12 * 16, dtype=torch.float32, device=DEV)
    y = torch.full((2 * 8 * 12 * 32,), SENTINEL, dtype=torch.float32, device=DEV)
    w = torch.zeros(32 * 7 * 7 * 16, dtype=torch.float32, device=DEV)
    xp, yp, wp = x.data_ptr(), y.data_ptr(), w.data_ptr()

    def call(xp=xp, wp=wp, yp=yp, ep='default', ph=0, pw=3, dilation=1, act=NONE, res=None, ldr=0, roff=0, **over):
        f = dict(N=2, H=8, W=12, Ci=8, Co=8, KH=1, stride=1, pad=0, ldx=8, ldy=8)
        f.update({k_: v for k_, v in over.items() if k_ in f})
        d = ops.conv_desc(*(f[k_] for k_ in ('N', 'H', 'W', 'Ci', 'Co', 'KH', 'stride', 'pad', 'ldx', 'ldy')))
        d.KW = over.get('KW', 7)
        for k_ in ('xoff', 'yoff'):
            if k_ in over:
                setattr(d, k_, over[k_])
        e = _lib.eval_f32_epilogue_t(None, None, res, ldr, roff, act, dilation)
        return L.gcc_conv_eval_f32_ex(C.byref(d), ph, pw, xp, wp, yp, C.byref(e) if ep == 'default' else None, None), \
            L.gcc_conv_eval_f32_ex_route(C.byref(d), ph, pw, dilation)

    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    assert call(xp=None)[0] == BAD_ARG
    assert call(wp=None)[0] == BAD_ARG
    assert call(yp=None)[0] == BAD_ARG
    assert call(ep=None)[0] == BAD_ARG
    assert L.gcc_conv_eval_f32_ex_route(None, 0, 0, 1) == BAD_ARG
    assert call(xp=xp + 4)[0] == BAD_ARG                                   # not 16-byte aligned
    assert call(pad=1) == (BAD_ARG, BAD_ARG)                               # c->pad must be 0: the paddings are the arguments
    assert call(KH=3, KW=3, ph=1, pw=1, pad=1) == (BAD_ARG, BAD_ARG)       # ... also where it agrees with them
    assert call(ph=-1) == (BAD_ARG, BAD_ARG)
    assert call(pw=-1) == (BAD_ARG, BAD_ARG)
    assert call(ldx=10) == (BAD_ARG, BAD_ARG)                              # ld no multiple of 4
    assert call(ldy=10) == (BAD_ARG, BAD_ARG)
    assert call(xoff=2) == (BAD_ARG, BAD_ARG)
    assert call(ldy=16, yoff=12) == (BAD_ARG, BAD_ARG)                     # the window does not fit its ld
    assert call(ldx=16, xoff=12) == (BAD_ARG, BAD_ARG)
    assert call(Ci=3, ldx=4, xoff=4) == (BAD_ARG, BAD_ARG)
    assert call(res=xp, ldr=8, roff=4)[0] == BAD_ARG                       # the residual's window outside its ld
    assert call(dilation=0) == (BAD_ARG, BAD_ARG)
    assert call(act=2)[0] == BAD_ARG                                       # tanh: not an act of this call
    assert call(KH=3, KW=3, ph=0, pw=0, H=2) == (BAD_ARG, BAD_ARG)         # a map smaller than the kernel and no padding
    assert call(Co=12, ldy=12) == (UNSUPPORTED, UNSUPPORTED)               # Co no multiple of 8
    assert call(Ci=4, ldx=4) == (UNSUPPORTED, UNSUPPORTED)
    assert call(KW=2, pw=0) == (UNSUPPORTED, UNSUPPORTED)                  # even kernels, kernels beyond 7
    assert call(KW=9, pw=4) == (UNSUPPORTED, UNSUPPORTED)
    assert call(KH=4, ph=0) == (UNSUPPORTED, UNSUPPORTED)
    assert call(stride=3) == (UNSUPPORTED, UNSUPPORTED)
    assert call(pw=4) == (UNSUPPORTED, UNSUPPORTED)                        # more than "same"
    assert call(ph=1) == (UNSUPPORTED, UNSUPPORTED)                        # KH = 1 takes no padding
    assert call(dilation=3, pw=3) == (UNSUPPORTED, UNSUPPORTED)
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 0 and (y == SENTINEL).all()
    # what is served: every padding from 0 to "same", under dilation too; and the call itself launches once
    for pw in (0, 1, 2, 3):
        assert call(pw=pw)[1] == 2
    assert call(KH=5, KW=5, ph=2, pw=2)[1] == 2 and call(KH=5, KW=3, ph=4, pw=0, dilation=2)[1] == 2
    y.fill_(SENTINEL)
    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    good = call()
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 1 and good == (0, 2)
    assert (y[8 * 2 * 8 * 12:] == SENTINEL).all() and (y[:8 * 2 * 8 * 12] == 0).all()
