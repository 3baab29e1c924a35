"""gcc_conv_eval_f32_act (gcc_conv_eval_f32_ex's kernel with sides up to 9, PReLU by a device slope, tanh and a PixelShuffle(2)
store) against torch-CPU float64 at SRResNet's geometries: an exact layout check on integer data, a derived per-element bound on
seeded normal data, bit-equality with gcc_conv_eval_f32_ex where both serve, batch invariance bit for bit, and the refusals, at the
smallest shapes at which the kernel can still go wrong."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG, UNSUPPORTED = -1, -2
NONE, PRELU, TANH, RELU = 0, 1, 2, 3
ACTS = {'none': NONE, 'relu': RELU, 'prelu': PRELU, 'tanh': TANH}
SENTINEL = -1234.5625
XOFF, YOFF = 4, 8                  # the input is read at channel 4 of an ld of ceil4(Ci) + 8, the output written at channel 8
# the device library's tanhf is documented (HIP math API, single precision) with a maximum error of 2 ulps; |tanh| <= 1, so an
# ulp of the result is at most the fp32 spacing at 1
TANH_ERR = 2 * float(np.spacing(np.float32(1.0)))

SIZES = {'a': (1, 6, 7), 'b': (2, 9, 11)}         # M = 42 and 198: no multiple of a tile; 198 gives blockIdx.x = 1 at 128 rows
CASES = {}
for s in SIZES:
    CASES['stem_%s' % s] = dict(k=9, Ci=3, Co=8, act='prelu', size=s)
    for ci in (8, 24):
        CASES['image_ci%d_%s' % (ci, s)] = dict(k=9, Ci=ci, Co=8, act='tanh', size=s, rows=3)      # the image conv: 3 real outputs
        for co in (8, 40, 72):
            for act in ACTS:
                CASES['k3_ci%d_co%d_%s_%s' % (ci, co, act, s)] = dict(k=3, Ci=ci, Co=co, act=act, size=s, res=ci == 24)
        for co in (32, 64, 160):
            CASES['shuffle_ci%d_co%d_%s' % (ci, co, s)] = dict(k=3, Ci=ci, Co=co, act='prelu', size=s, shuffle=2)
# 32768 pixels x 128 channels: 256 tiles of 128 x 128, blockIdx.x up to 255
CASES['big'] = dict(k=3, Ci=8, Co=128, act='prelu', size=(2, 128, 128))
CASES['big_shuffle'] = dict(k=3, Ci=8, Co=128, act='prelu', size=(2, 128, 128), shuffle=2)


class Geom:
    def __init__(self, name):
        c = CASES[name]
        self.k, self.Ci, self.Co, self.act = c['k'], c['Ci'], c['Co'], ACTS[c['act']]
        self.N, self.H, self.W = SIZES.get(c['size'], c['size'])
        self.p = self.k // 2
        self.shuffle, self.res, self.rows = c.get('shuffle', 0), c.get('res', False), c.get('rows', c['Co'])
        self.Cy = self.Co // 4 if self.shuffle else self.Co               # channels and map of the output window
        self.Hy, self.Wy = (2 * self.H, 2 * self.W) if self.shuffle else (self.H, self.W)
        self.ldx, self.ldy = (self.Ci + 3) // 4 * 4 + 8, self.Cy + 16
        self.K = self.k * self.k * self.Ci


@functools.lru_cache(maxsize=None)
def _data(name, kind):
    """(x, w, scale, shift, residual or None, slope) on the host in float64.  'int': x in [-3, 3], every weight a distinct integer
    of magnitude <= 4095 (asymmetric: a swapped index shows), scale in {-2, -1, 1, 2}, integer shift and residual, the slope a
    power of two: every partial sum, the epilogue and slope v are integers (or quarters) below 2^24 and exact in fp32;
    'normal': seeded normal data (fp32 values).  Rows >= `rows` of w are zero (the image conv's pad rows)."""
    q = Geom(name)
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + (1 if kind == 'int' else 2))
    if kind == 'int':
        x = torch.randint(-3, 4, (q.N, q.Ci, q.H, q.W), generator=g).double()
        idx = torch.arange(q.Co * q.Ci * q.k * q.k, dtype=torch.int64)
        w = ((idx * 7919) % 8191 - 4095).double().reshape(q.Co, q.Ci, q.k, q.k)
        scale = torch.tensor([1.0, -2.0, 2.0, -1.0]).repeat(q.Co)[:q.Co].double()
        shift = torch.randint(-50, 51, (q.Co,), generator=g).double()
        res = torch.randint(-1000, 1001, (q.N, q.Co, q.H, q.W), generator=g).double() if q.res else None
        slope = -0.25
    else:
        x = torch.randn((q.N, q.Ci, q.H, q.W), generator=g).float().double()
        w = (torch.randn((q.Co, q.Ci, q.k, q.k), generator=g) * (0.2 if q.k == 3 else 0.07)).float().double()
        scale = (torch.rand(q.Co, generator=g) + 0.5).float().double() * torch.where(torch.arange(q.Co) % 3 == 0, -1.0, 1.0)
        shift = (torch.randn(q.Co, generator=g) * 0.3).float().double()
        res = torch.randn((q.N, q.Co, q.H, q.W), generator=g).float().double() if q.res else None
        slope = float(torch.tensor(0.3 if q.Ci == 8 else -1.75).float())
    if q.k == 9 and q.Ci != 3:
        w[:, 3:] = 0                                        # only input channels 0..2 carry weights: 243 products, as the stem
    w[q.rows:] = 0
    return x, w, scale, shift, res, slope


def _act64(v, act, slope):
    if act == RELU:
        return torch.relu(v)
    if act == PRELU:
        return torch.where(v >= 0, v, slope * v)
    return torch.tanh(v) if act == TANH else v


@functools.lru_cache(maxsize=None)
def _want(name, kind):
    """(float64 result in the output's layout, its pre-activation, the per-element magnitude |scale| sum |x w| + |shift| +
    |residual| in the same layout) of a case"""
    q = Geom(name)
    x, w, scale, shift, res, slope = _data(name, kind)
    pre = F.conv2d(x, w, None, 1, q.p) * scale[None, :, None, None] + shift[None, :, None, None]
    mag = F.conv2d(x.abs(), w.abs(), None, 1, q.p) * scale.abs()[None, :, None, None] + shift.abs()[None, :, None, None]
    if res is not None:
        pre, mag = pre + res, mag + res.abs()
    if q.shuffle:
        pre, mag = F.pixel_shuffle(pre, 2), F.pixel_shuffle(mag, 2)
    return _act64(pre, q.act, slope), pre, mag


def _pack(w):
    from gcc_amd import ops
    return ops.pack_weights_f32(w.float().to(DEV))


def _nhwc(t, ld, off, fill):
    N, Cc, H, W = t.shape
    buf = torch.full((N, H, W, ld), fill, dtype=torch.float32)
    buf[..., off:off + Cc] = t.permute(0, 2, 3, 1).float()
    return buf.to(DEV)


def _run(name, kind, image=None):
    """(result [N, Cy, Hy, Wy] on the host, the whole output buffer on the host) of a case -- or of its image `image` alone"""
    from gcc_amd import _lib, ops
    q = Geom(name)
    x, w, scale, shift, res, slope = _data(name, kind)
    if image is not None:
        x, res = x[image:image + 1], (res[image:image + 1] if res is not None else None)
    N = x.shape[0]
    xb = _nhwc(x, q.ldx, XOFF, fill=9.0)
    yb = torch.full((N, q.Hy, q.Wy, q.ldy), SENTINEL, dtype=torch.float32, device=DEV)
    sc, sh = scale.float().to(DEV), shift.float().to(DEV)
    sl = torch.tensor([slope], dtype=torch.float32, device=DEV)
    rb = _nhwc(res, q.Co + 8, 4, fill=7.0) if res is not None else None
    d = ops.conv_desc(N, q.H, q.W, q.Ci, q.Co, q.k, 1, 0, q.ldx, q.ldy)
    d.xoff, d.yoff = XOFF, YOFF
    ep = _lib.eval_f32_act_epilogue_t(sc.data_ptr(), sh.data_ptr(), rb.data_ptr() if rb is not None else None, q.Co + 8, 4, q.act,
                                      q.shuffle, sl.data_ptr(), 1, 0)
    wp = _pack(w)
    assert ops.lib().gcc_conv_eval_f32_act(C.byref(d), q.p, q.p, xb.data_ptr(), wp.data_ptr(), yb.data_ptr(), C.byref(ep), None) == 0, name
    out = yb.cpu()
    return out[..., YOFF:YOFF + q.Cy].permute(0, 3, 1, 2).contiguous(), out


def _only_the_window_is_written(q, whole):
    keep = torch.ones(q.ldy, dtype=torch.bool)
    keep[YOFF:YOFF + q.Cy] = False
    return bool((whole[..., keep] == SENTINEL).all())


# ---- 1. exact layout check ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_integer_data_is_exact(name):
    """every element equals the float64 result, the shuffled placement included.  tanh of an integer is no fp32 number: there
    the pre-activation is exact by the same argument and the element is within the device tanhf's documented error of the
    float64 tanh of it (0 and +-1 come out exactly)"""
    q = Geom(name)
    got, whole = _run(name, 'int')
    want, pre, mag = _want(name, 'int')
    assert tuple(want.shape) == (q.N, q.Cy, q.Hy, q.Wy)
    assert float(mag.max()) < 2 ** 24                        # every partial sum and the epilogue are exact in fp32
    if q.act == TANH:
        assert ((got.double() - want).abs() <= TANH_ERR).all(), name
        assert torch.equal(got.double()[pre == 0], want[pre == 0]) and torch.equal(got.double()[pre.abs() > 20], want[pre.abs() > 20])
    else:
        assert torch.equal(got.double(), want), name
    assert _only_the_window_is_written(q, whole)


# ---- 2. seeded normal data, per element ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_normal_data_within_the_fmaf_chain_bound(name):
    """b = (K + 3) 2^-24 (|scale| sum |x w| + |shift| + |residual|) bounds the pre-activation: K fmaf roundings of the chain, the
    epilogue's fmaf and the residual's add (second-order terms of K = 1944 roundings are 1e-4 of one more).  ReLU does not widen a
    difference; PReLU multiplies it by at most max(1, |slope|) and rounds slope v once more (2^-24 |slope| (|v| + b)); tanh has a
    derivative of at most 1 and adds the device function's documented error"""
    q = Geom(name)
    got, whole = _run(name, 'normal')
    want, pre, mag = _want(name, 'normal')
    slope = _data(name, 'normal')[5]
    bound = (q.K + 3) * 2.0 ** -24 * mag
    if q.act == PRELU:
        bound = max(1.0, abs(slope)) * bound + 2.0 ** -24 * abs(slope) * (pre.abs() + bound)
    elif q.act == TANH:
        bound = bound + TANH_ERR
    err = (got.double() - want).abs()
    print('%s: K %d, worst error / bound %.3f' % (name, q.K, float((err / bound.clamp_min(1e-300)).max())))
    assert (err <= bound).all(), name
    assert _only_the_window_is_written(q, whole)


# ---- 3. the old entry, the batch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,stride,Ci,Co,size,route', [(3, 1, 8, 8, (2, 9, 11), 2), (7, 2, 3, 40, (2, 9, 11), 1),
                                                       (5, 1, 24, 72, (2, 9, 11), 1), (3, 1, 8, 128, (2, 128, 128), 0),
                                                       (1, 1, 24, 32, (1, 6, 7), 2)])
@pytest.mark.parametrize('act', [NONE, RELU])
def test_same_bits_as_conv_eval_f32_ex_where_both_serve(k, stride, Ci, Co, size, route, act):
    from gcc_amd import ops
    g = torch.Generator().manual_seed(k * 10 + Ci)
    N, H, W = size
    pad = k // 2
    x = torch.randn((N, Ci, H, W), generator=g)
    w = ops.pack_weights_f32((torch.randn((Co, Ci, k, k), generator=g) * 0.2).to(DEV))
    scale, shift = (torch.rand(Co, generator=g) + 0.5).to(DEV), torch.randn(Co, generator=g).to(DEV)
    xv = _nhwc(x.double(), (Ci + 3) // 4 * 4, 0, fill=0.0).permute(0, 3, 1, 2)[:, :Ci]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = ops.new_act_f32(N, Co, Ho, Wo, DEV)
    res.copy_(torch.randn((N, Co, Ho, Wo), generator=g).to(DEV))
    old, new = ops.new_act_f32(N, Co, Ho, Wo, DEV), ops.new_act_f32(N, Co, Ho, Wo, DEV)
    ops.conv_eval_f32_ex(xv, w, Co, (k, k), stride, (pad, pad), old, scale=scale, shift=shift, act=act, residual=res)
    ops.conv_eval_f32_act(xv, w, Co, (k, k), (pad, pad), new, stride=stride, scale=scale, shift=shift, act=act, residual=res)
    assert ops.conv_eval_f32_ex(xv, w, Co, (k, k), stride, (pad, pad), old, route_only=True) == route
    assert ops.conv_eval_f32_act(xv, w, Co, (k, k), (pad, pad), new, stride=stride, route_only=True) == route
    assert float(old.abs().max()) > 0
    assert torch.equal(old.cpu().view(torch.int32), new.cpu().view(torch.int32))


@pytest.mark.parametrize('name', ['shuffle_ci24_co64_b', 'stem_b', 'image_ci24_b', 'k3_ci24_co72_prelu_b'])
def test_an_image_alone_equals_the_image_in_its_batch_bit_for_bit(name):
    q = Geom(name)
    both, _ = _run(name, 'normal')
    for n in range(q.N):
        one, whole = _run(name, 'normal', image=n)
        assert _only_the_window_is_written(q, whole)
        assert torch.equal(one.view(torch.int32), both[n:n + 1].contiguous().view(torch.int32)), (name, n)


def test_every_tile_shape_is_exercised():
    from gcc_amd import ops
    L = ops.lib()
    for name, route in (('big', 0), ('big_shuffle', 0), ('k3_ci8_co72_none_b', 1), ('shuffle_ci8_co64_b', 1), ('shuffle_ci8_co160_a', 1),
                        ('stem_b', 2), ('shuffle_ci24_co32_a', 2)):
        q = Geom(name)
        d = ops.conv_desc(q.N, q.H, q.W, q.Ci, q.Co, q.k, 1, 0, q.ldx, q.ldy)
        d.xoff, d.yoff = XOFF, YOFF
        assert L.gcc_conv_eval_f32_act_route(C.byref(d), q.p, q.p, 1, q.shuffle) == route, name


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_happen_before_any_launch():
    from gcc_amd import _lib, ops
    L = ops.lib()
    x = torch.zeros(2 * 8 * 12 * 16, dtype=torch.float32, device=DEV)
    y = torch.full((2 * 8 * 12 * 4 * 16,), SENTINEL, dtype=torch.float32, device=DEV)
    w = torch.zeros(64 * 11 * 11 * 16, dtype=torch.float32, device=DEV)
    slope = torch.full((1,), 0.25, dtype=torch.float32, device=DEV)
    xp, yp, wp, sp = x.data_ptr(), y.data_ptr(), w.data_ptr(), slope.data_ptr()

    def call(xp=xp, ep='default', p=1, dilation=1, act=NONE, slope=sp, shuffle=0, res=None, ldr=0, roff=0, **over):
        f = dict(N=2, H=8, W=12, Ci=8, Co=32, KH=3, stride=1, pad=0, ldx=8, ldy=32)
        f.update({k_: v for k_, v in over.items() if k_ in f})
        d = ops.conv_desc(*(f[k_] for k_ in ('N', 'H', 'W', 'Ci', 'Co', 'KH', 'stride', 'pad', 'ldx', 'ldy')))
        d.KW = over.get('KW', f['KH'])
        d.yoff = over.get('yoff', 0)
        e = _lib.eval_f32_act_epilogue_t(None, None, res, ldr, roff, act, shuffle, slope, dilation, 0)
        return L.gcc_conv_eval_f32_act(C.byref(d), p, p, xp, wp, yp, C.byref(e) if ep == 'default' else None, None), \
            L.gcc_conv_eval_f32_act_route(C.byref(d), p, p, dilation, shuffle)

    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    assert call(act=PRELU, slope=None)[0] == BAD_ARG                       # a learned slope lives on the device: none given
    assert call(shuffle=1) == (BAD_ARG, BAD_ARG)
    assert call(shuffle=3) == (BAD_ARG, BAD_ARG)
    assert call(shuffle=2, ldy=8, res=xp, ldr=32, roff=0)[0] == UNSUPPORTED    # a shuffle with a residual
    assert call(shuffle=2, Co=40, ldy=12) == (UNSUPPORTED, UNSUPPORTED)    # Co % 32: a store group would straddle sub-pixels
    assert call(shuffle=2, Co=64, ldy=12) == (BAD_ARG, BAD_ARG)            # ldy < Co / 4
    assert call(shuffle=2, ldy=12, yoff=8) == (BAD_ARG, BAD_ARG)           # ldy < yoff + Co / 4
    assert call(pad=1) == (BAD_ARG, BAD_ARG)                               # c->pad must be 0: the paddings are the arguments
    assert call(KH=11, p=5) == (UNSUPPORTED, UNSUPPORTED)                  # a kernel side of 11
    assert call(KH=9, KW=11, p=4) == (UNSUPPORTED, UNSUPPORTED)
    assert call(act=4)[0] == BAD_ARG                                       # LeakyReLU, and anything else outside the four
    assert call(act=7)[0] == BAD_ARG
    assert call(act=-1)[0] == BAD_ARG
    assert call(ep=None)[0] == BAD_ARG
    assert call(xp=xp + 4)[0] == BAD_ARG                                   # what gcc_conv_eval_f32_ex refuses, still refused
    assert call(Co=12, ldy=12) == (UNSUPPORTED, UNSUPPORTED)
    assert call(Ci=4, ldx=4) == (UNSUPPORTED, UNSUPPORTED)
    assert call(p=2) == (UNSUPPORTED, UNSUPPORTED)                         # more than "same"
    assert call(ldy=16) == (BAD_ARG, BAD_ARG)                              # the unshuffled window does not fit its ld
    assert call(res=xp, ldr=16, roff=0)[0] == BAD_ARG                      # nor the residual's
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 0 and (y == SENTINEL).all()
    # what is served launches once: a 9 x 9 kernel with a shuffled PReLU store into [2, 16, 24] pixels of 8 channels
    assert call(KH=9, p=4, shuffle=2, ldy=8, act=PRELU) == (0, 2)
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 1
    n = 2 * 16 * 24 * 8
    assert (y[n:] == SENTINEL).all() and (y[:n] == 0).all()
