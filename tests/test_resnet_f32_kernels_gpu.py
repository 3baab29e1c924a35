"""The MobileResnet generator's fp32 kernels (gcc_amd/csrc/resnet_f32.hip) against torch-CPU float64, by the method of
tests/test_conv_f32_unet_gpu.py: gcc_conv_eval_f32_resnet (reflection-padded and transposed convolutions) with an exact layout
check on integer data, a derived per-element bound on seeded normal data, batch invariance bit for bit and the refusals;
gcc_dwconv3x3_reflect_f32 the same way; gcc_inorm_stats_f32 + gcc_inorm_apply_f32 against float64 InstanceNorm at 8 x the error
of an fp32 host evaluation, fed by the stats launch and by the depthwise launch's own partials.  Every buffer is sentinel-filled
around an offset channel window: only the windows are written."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
NONE, PRELU, TANH, RELU, LRELU = 0, 1, 2, 3, 4
REFLECT, TRANSPOSED3 = 0, 1
SENTINEL = -1234.5625
XOFF, YOFF = 4, 8        # x is read at channel 4 of an ld of ceil4(C) + 8; y is written at channel 8 of an ld of C + 24
# the device library's tanhf is documented (HIP math API, single precision) with a maximum error of 2 ulps; |tanh| <= 1
TANH_ERR = 2 * float(np.spacing(np.float32(1.0)))

# name: (kind, N, H, W of the input, Ci, Co, the tile the library takes)
CASES = {
    'rf_4x4': (REFLECT, 1, 4, 4, 3, 8, 2),             # every tap row / column but one is a reflected one somewhere
    'rf_9x13': (REFLECT, 2, 9, 13, 3, 24, 2),          # the stem: the pad channel of x holds a sentinel
    'rf_8x8': (REFLECT, 3, 8, 8, 16, 72, 1),
    'rf_64': (REFLECT, 1, 64, 64, 8, 136, 1),          # 64 x 3 tiles, Co past two tiles
    'rf_128': (REFLECT, 1, 128, 128, 8, 136, 0),       # the 128 x 128 tile (256 of them fill the chip)
    'tr_1x1': (TRANSPOSED3, 1, 1, 1, 8, 8, 2),         # one input pixel: every second tap is beyond the map
    'tr_3x5': (TRANSPOSED3, 2, 3, 5, 16, 24, 2),
    'tr_2x2': (TRANSPOSED3, 3, 2, 2, 72, 16, 2),
    'tr_64': (TRANSPOSED3, 1, 64, 64, 8, 136, 1),
    'tr_128': (TRANSPOSED3, 1, 128, 128, 8, 136, 0),
}
ACTS = {'none': NONE, 'relu': RELU, 'tanh': TANH}


class Geom:
    def __init__(self, name):
        self.kind, self.N, self.H, self.W, self.Ci, self.Co, self.route = CASES[name]
        self.tr = self.kind == TRANSPOSED3
        self.k = 3 if self.tr else 7
        self.Ho, self.Wo = (2 * self.H, 2 * self.W) if self.tr else (self.H, self.W)
        self.ldx, self.ldy = (self.Ci + 3) // 4 * 4 + 8, self.Co + 24

    def products(self):
        """[Ho, Wo]: the number of products of each output element's chain -- 49 Ci behind the reflection (a mirrored tap is a
        real value); transposed, Ci per tap of the element's phase that lies inside the map"""
        if not self.tr:
            return torch.full((self.Ho, self.Wo), 49 * self.Ci, dtype=torch.float64)
        taps = lambda o, n: 1 + (1 if (o & 1) and (o + 1) // 2 < n else 0)
        th = torch.tensor([taps(o, self.H) for o in range(self.Ho)], dtype=torch.float64)
        tw = torch.tensor([taps(o, self.W) for o in range(self.Wo)], dtype=torch.float64)
        return th[:, None] * tw[None, :] * self.Ci


@functools.lru_cache(maxsize=None)
def _data(name, kind):
    """(x, w, scale, shift) on the host in float64; w is Conv2d's [Co, Ci, 7, 7] or ConvTranspose2d's [Ci, Co, 3, 3].
    'int': x in [-3, 3], asymmetric integer weights of magnitude <= 1023 (2047 distinct values: a swapped index shows), scale in
    {-2, -1, 1, 2}, integer shift: every partial sum and the epilogue are exact in fp32; 'normal': seeded normal data."""
    q = Geom(name)
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + (1 if kind == 'int' else 2))
    wshape = (q.Ci, q.Co, 3, 3) if q.tr else (q.Co, q.Ci, 7, 7)
    if kind == 'int':
        x = torch.randint(-3, 4, (q.N, q.Ci, q.H, q.W), generator=g).double()
        idx = torch.arange(q.Co * q.Ci * q.k * q.k, dtype=torch.int64)
        w = ((idx * 7919) % 2047 - 1023).double().reshape(wshape)
        scale = torch.tensor([1.0, -2.0, 2.0, -1.0]).repeat(q.Co)[:q.Co].double()
        shift = torch.randint(-50, 51, (q.Co,), generator=g).double()
    else:
        x = torch.randn((q.N, q.Ci, q.H, q.W), generator=g).float().double()
        w = (torch.randn(wshape, generator=g) * 0.2).float().double()
        scale = (torch.rand(q.Co, generator=g) + 0.5).float().double() * torch.where(torch.arange(q.Co) % 3 == 0, -1.0, 1.0)
        shift = (torch.randn(q.Co, generator=g) * 0.3).float().double()
    return x, w, scale, shift


def _conv64(q, x, w):
    if q.tr:
        return F.conv_transpose2d(x, w, None, 2, 1, 1)
    return F.conv2d(F.pad(x, (3, 3, 3, 3), mode='reflect'), w)


@functools.lru_cache(maxsize=None)
def _want(name, kind):
    """(the float64 pre-activation z, the per-element magnitude |scale| sum |x w| + |shift|) of a case"""
    q = Geom(name)
    x, w, scale, shift = _data(name, kind)
    pre = _conv64(q, x, w) * scale[None, :, None, None] + shift[None, :, None, None]
    mag = _conv64(q, x.abs(), w.abs()) * scale.abs()[None, :, None, None] + shift.abs()[None, :, None, None]
    assert tuple(pre.shape) == (q.N, q.Co, q.Ho, q.Wo)
    return pre, mag


def _act64(v, act):
    if act == RELU:
        return torch.relu(v)
    return torch.tanh(v) if act == TANH else v


def _nhwc(t, ld, off, fill):
    N, Cc, H, W = t.shape
    buf = torch.full((N, H, W, ld), fill, dtype=torch.float32)
    buf[..., off:off + Cc] = t.permute(0, 2, 3, 1).float()
    return buf.to(DEV)


def _cut(buf, off, Cc):
    return buf[..., off:off + Cc].permute(0, 3, 1, 2).contiguous()


def _outside(buf, off, Cc):
    keep = torch.ones(buf.shape[-1], dtype=torch.bool)
    keep[off:off + Cc] = False
    return bool((buf[..., keep] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _packed(name, kind):
    from gcc_amd import ops
    q = Geom(name)
    return ops.pack_weights_f32_resnet(_data(name, kind)[1].float().to(DEV), q.kind)


def _run(name, kind, act, image=None):
    """(y as [N, Co, Ho, Wo] on the host, the whole output buffer on the host) of a case -- or of its image `image`"""
    from gcc_amd import _lib, ops
    q = Geom(name)
    x, w, scale, shift = _data(name, kind)
    if image is not None:
        x = x[image:image + 1]
    N = x.shape[0]
    xb = _nhwc(x, q.ldx, XOFF, fill=9.0)                       # with Ci == 3 channel XOFF + 3, the pad channel, holds 9 too
    yb = torch.full((N, q.Ho, q.Wo, q.ldy), SENTINEL, dtype=torch.float32, device=DEV)
    sc, sh = scale.float().to(DEV), shift.float().to(DEV)
    d = ops.conv_desc(N, q.H, q.W, q.Ci, q.Co, q.k, 2 if q.tr else 1, 1 if q.tr else 0, q.ldx, q.ldy)
    d.xoff, d.yoff = XOFF, YOFF
    ep = _lib.eval_f32_resnet_epilogue_t(sc.data_ptr(), sh.data_ptr(), act, 0)
    L = ops.lib()
    if image is None:
        assert L.gcc_conv_eval_f32_resnet_route(C.byref(d), q.kind) == q.route, name
    assert L.gcc_conv_eval_f32_resnet(C.byref(d), q.kind, xb.data_ptr(), _packed(name, kind).data_ptr(), yb.data_ptr(), C.byref(ep),
                                      None) == 0
    out = yb.cpu()
    return _cut(out, YOFF, q.Co), out


PARAMS = [(n, a) for n in CASES for a in ACTS]


# ---- 1. the convolution: exact layout check ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,act', PARAMS)
def test_conv_integer_data_is_exact(name, act):
    """every element equals the float64 conv2d(pad(reflect)) / conv_transpose2d(.., 2, 1, 1) result.  tanh of an integer is no fp32
    number: there the pre-activation is exact by the same argument and the element is within the device tanhf's documented error
    of the float64 tanh of it (0 and +-1 come out exactly)"""
    q = Geom(name)
    y, whole = _run(name, 'int', ACTS[act])
    pre, mag = _want(name, 'int')
    assert float(mag.max()) < 2 ** 24                        # every partial sum and the epilogue are exact in fp32
    want = _act64(pre, ACTS[act])
    if ACTS[act] == TANH:
        assert ((y.double() - want).abs() <= TANH_ERR).all(), name
        assert torch.equal(y.double()[pre == 0], want[pre == 0]) and torch.equal(y.double()[pre.abs() > 20], want[pre.abs() > 20])
    else:
        assert torch.equal(y.double(), want), name
    assert _outside(whole, YOFF, q.Co)


# ---- 2. the convolution: seeded normal data, per element -----------------------------------------------------------------------
@pytest.mark.parametrize('name,act', PARAMS)
def test_conv_normal_data_within_the_fmaf_chain_bound(name, act):
    """b = (K + 3) 2^-24 (|scale| sum |x w| + |shift|) bounds the pre-activation: K fmaf roundings of the element's own chain
    (Geom.products; zero products round nothing) and the epilogue's fmaf.  ReLU does not widen a difference; tanh has a derivative
    of at most 1 and adds the device function's documented error"""
    q = Geom(name)
    y, whole = _run(name, 'normal', ACTS[act])
    pre, mag = _want(name, 'normal')
    bound = (q.products()[None, None] + 3) * 2.0 ** -24 * mag
    if ACTS[act] == TANH:
        bound = bound + TANH_ERR
    err = (y.double() - _act64(pre, ACTS[act])).abs()
    print('%s %s: worst error / bound %.3f' % (name, act, float((err / bound.clamp_min(1e-300)).max())))
    assert (err <= bound).all(), name
    assert _outside(whole, YOFF, q.Co)


# ---- 3. the convolution: the batch, the tiles ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rf_9x13', 'rf_8x8', 'tr_3x5', 'tr_2x2'])
def test_conv_an_image_alone_equals_the_image_in_its_batch_bit_for_bit(name):
    q = Geom(name)
    y, _ = _run(name, 'normal', TANH)
    for n in range(q.N):
        a, whole = _run(name, 'normal', TANH, image=n)
        assert _outside(whole, YOFF, q.Co)
        assert torch.equal(a.view(torch.int32), y[n:n + 1].contiguous().view(torch.int32)), (name, n)


def test_conv_every_tile_shape_is_exercised_in_both_kinds():
    assert {CASES[n][6] for n in CASES if CASES[n][0] == REFLECT} == {0, 1, 2}
    assert {CASES[n][6] for n in CASES if CASES[n][0] == TRANSPOSED3} == {0, 1, 2}


def test_conv_k3_reflect_through_ops_is_exact():
    """the k = 3 side of the reflect kind, integer data, through the ops wrapper"""
    from gcc_amd import _lib, ops
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (2, 16, 5, 6), generator=g).double()
    w = torch.randint(-2000, 2001, (40, 16, 3, 3), generator=g).double()
    b = torch.randint(-9, 10, (40,), generator=g).double()
    xv = _nhwc(x, 16, 0, 0.0).permute(0, 3, 1, 2)
    out = ops.new_act_f32(2, 40, 5, 6, DEV)
    wp = ops.pack_weights_f32_resnet(w.float().to(DEV), _lib.F32_RESNET_REFLECT)
    assert ops.conv_eval_f32_resnet(xv, wp, 40, _lib.F32_RESNET_REFLECT, 3, out, route_only=True) == 1
    ops.conv_eval_f32_resnet(xv, wp, 40, _lib.F32_RESNET_REFLECT, 3, out, shift=b.float().to(DEV), act=_lib.EVAL_ACT_RELU)
    want = torch.relu(F.conv2d(F.pad(x, (1, 1, 1, 1), mode='reflect'), w, b))
    assert torch.equal(out.cpu().double(), want)


# ---- 4. the convolution: refusals ----------------------------------------------------------------------------------------------
def test_conv_refusals_happen_before_any_launch():
    from gcc_amd import _lib, ops
    L = ops.lib()
    x = torch.zeros(2 * 8 * 12 * 16, dtype=torch.float32, device=DEV)
    y = torch.full((2 * 16 * 24 * 64,), SENTINEL, dtype=torch.float32, device=DEV)
    w = torch.zeros(4 * 32 * 49 * 16, dtype=torch.float32, device=DEV)
    xp, yp, wp = x.data_ptr(), y.data_ptr(), w.data_ptr()

    def call(kind, xp=xp, wp=wp, yp=yp, ep='default', act=NONE, **over):
        f = dict(N=2, H=8, W=12, Ci=8, Co=16, KH=3 if kind == TRANSPOSED3 else 7, stride=2 if kind == TRANSPOSED3 else 1,
                 pad=1 if kind == TRANSPOSED3 else 0, ldx=8, ldy=64)
        f.update({k_: v for k_, v in over.items() if k_ in f})
        d = ops.conv_desc(*(f[k_] for k_ in ('N', 'H', 'W', 'Ci', 'Co', 'KH', 'stride', 'pad', 'ldx', 'ldy')))
        d.KW = over.get('KW', f['KH'])
        d.xoff, d.yoff = over.get('xoff', 0), over.get('yoff', 0)
        e = _lib.eval_f32_resnet_epilogue_t(None, None, act, 0)
        return L.gcc_conv_eval_f32_resnet(C.byref(d), kind, xp, wp, yp, C.byref(e) if ep == 'default' else None, None), \
            L.gcc_conv_eval_f32_resnet_route(C.byref(d), kind)

    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    for kind in (REFLECT, TRANSPOSED3):
        assert call(kind, ldx=10) == (BAD_ARG, BAD_ARG)                    # ld / off: multiples of 4 floats
        assert call(kind, ldy=66) == (BAD_ARG, BAD_ARG)
        assert call(kind, ldx=16, xoff=2) == (BAD_ARG, BAD_ARG)
        assert call(kind, yoff=6) == (BAD_ARG, BAD_ARG)
        assert call(kind, xp=xp + 4)[0] == BAD_ARG                         # pointers: 16 bytes
        assert call(kind, yp=yp + 8)[0] == BAD_ARG
        assert call(kind, wp=wp + 4)[0] == BAD_ARG
        assert call(kind, ldx=8, xoff=4) == (BAD_ARG, BAD_ARG)             # a window outside its ld
        assert call(kind, ldy=64, yoff=52) == (BAD_ARG, BAD_ARG)
        for bad in (PRELU, LRELU, 5, -1):                                  # none, ReLU and tanh only
            assert call(kind, act=bad)[0] == BAD_ARG
        assert call(kind, xp=None)[0] == BAD_ARG
        assert call(kind, wp=None)[0] == BAD_ARG
        assert call(kind, yp=None)[0] == BAD_ARG
        assert call(kind, ep=None)[0] == BAD_ARG
        assert call(kind, N=0) == (BAD_ARG, BAD_ARG)
        assert call(kind, KH=5) == (UNSUPPORTED, UNSUPPORTED)              # geometries nobody serves
        assert call(kind, KH=3, KW=7) == (UNSUPPORTED, UNSUPPORTED)
        assert call(kind, Ci=4, ldx=4) == (UNSUPPORTED, UNSUPPORTED)
        assert call(kind, Co=12) == (UNSUPPORTED, UNSUPPORTED)
    assert call(REFLECT, stride=2) == (UNSUPPORTED, UNSUPPORTED)
    assert call(REFLECT, pad=3) == (BAD_ARG, BAD_ARG)                      # the padding is the reflection's: the conv has none
    assert call(REFLECT, H=3) == (BAD_ARG, BAD_ARG) and call(REFLECT, W=3) == (BAD_ARG, BAD_ARG)    # ReflectionPad2d(3) needs > 3
    assert call(TRANSPOSED3, KH=7) == (UNSUPPORTED, UNSUPPORTED)
    assert call(TRANSPOSED3, stride=1) == (UNSUPPORTED, UNSUPPORTED)
    assert call(TRANSPOSED3, pad=0) == (BAD_ARG, BAD_ARG) and call(TRANSPOSED3, pad=2) == (BAD_ARG, BAD_ARG)
    assert call(TRANSPOSED3, Ci=3, ldx=4) == (UNSUPPORTED, UNSUPPORTED)    # the 3-in-4 stem exists behind the reflection only
    assert call(2) == (BAD_ARG, BAD_ARG) and call(-1) == (BAD_ARG, BAD_ARG)
    assert L.gcc_conv_eval_f32_resnet_route(None, 0) == BAD_ARG
    assert L.gcc_conv_eval_f32_resnet_kp(8, REFLECT, 7) == 392 + 8 and L.gcc_conv_eval_f32_resnet_kp(3, REFLECT, 7) == 208
    assert L.gcc_conv_eval_f32_resnet_kp(8, REFLECT, 3) == 80
    assert L.gcc_conv_eval_f32_resnet_kp(8, TRANSPOSED3, 3) == 32 and L.gcc_conv_eval_f32_resnet_kp(72, TRANSPOSED3, 3) == 288
    assert L.gcc_conv_eval_f32_resnet_kp(0, REFLECT, 7) == BAD_ARG and L.gcc_conv_eval_f32_resnet_kp(8, 2, 3) == BAD_ARG
    assert L.gcc_conv_eval_f32_resnet_kp(8, REFLECT, 5) == BAD_ARG and L.gcc_conv_eval_f32_resnet_kp(8, TRANSPOSED3, 7) == BAD_ARG
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 0 and (y == SENTINEL).all()
    # what is served launches once per call: reflect [2, 8, 12] and transposed [2, 16, 24] into channels 16 .. 31 / 0 .. 15
    assert call(REFLECT, yoff=16) == (0, 2)
    torch.cuda.synchronize()
    assert L.gcc_launch_count(1) == 1
    v = y[:2 * 8 * 12 * 64].view(-1, 64)
    assert (v[:, 16:32] == 0).all() and (v[:, :16] == SENTINEL).all() and (v[:, 32:] == SENTINEL).all()
    assert (y[2 * 8 * 12 * 64:] == SENTINEL).all()
    assert call(TRANSPOSED3, act=TANH) == (0, 2)
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 1
    v = y.view(-1, 64)
    assert (v[:, :16] == 0).all() and (v[:, 32:] == SENTINEL).all() and (v[2 * 8 * 12:, 16:32] == SENTINEL).all()


# ---- 5. the depthwise convolution -----------------------------------------------------------------------------------------------
DW_PLANES = [(2, 2), (5, 7), (24, 24)]
DW_CHANNELS = (8, 20, 72)


def _dw_data(N, H, W, Cc, kind):
    g = torch.Generator().manual_seed(1000 * N + 100 * H + W + Cc + (7 if kind == 'int' else 0))
    if kind == 'int':
        x = torch.randint(-30, 31, (N, Cc, H, W), generator=g).double()
        w = torch.randint(-4000, 4001, (Cc, 1, 3, 3), generator=g).double()
        b = torch.randint(-500, 501, (Cc,), generator=g).double()
    else:
        x = torch.randn((N, Cc, H, W), generator=g).float().double()
        w = (torch.randn((Cc, 1, 3, 3), generator=g) * 0.4).float().double()
        b = (torch.randn(Cc, generator=g) * 0.3).float().double()
    return x, w, b


def _dw64(x, w, b):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode='reflect'), w, b, groups=x.shape[1])


def _dw_run(x, w, b, stats=False):
    """(y [N, C, H, W] on the host, the whole output buffer on the host, the partials or None)"""
    from gcc_amd import ops
    N, Cc, H, W = x.shape
    ldx, ldy = Cc + 8, Cc + 24
    xb = _nhwc(x, ldx, XOFF, fill=9.0)
    yb = torch.full((N, H, W, ldy), SENTINEL, dtype=torch.float32, device=DEV)
    wp, bp = ops.pack_dw_f32(w.float().to(DEV), b.float().to(DEV))
    L = ops.lib()
    ws = None
    if stats:
        ws = torch.full((L.gcc_inorm_f32_workspace(N, Cc, H * W) // 8,), float('nan'), dtype=torch.float64, device=DEV)
    rc = L.gcc_dwconv3x3_reflect_f32(xb.data_ptr() + 4 * XOFF, ldx, yb.data_ptr() + 4 * YOFF, ldy, wp.data_ptr(), bp.data_ptr(), N, H, W,
                                     Cc, ws.data_ptr() if stats else None, ws.numel() * 8 if stats else 0, None)
    assert rc == 0
    out = yb.cpu()
    return _cut(out, YOFF, Cc), out, ws


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('HW', DW_PLANES)
def test_dw_integer_data_is_exact(N, HW):
    for Cc in DW_CHANNELS:
        x, w, b = _dw_data(N, HW[0], HW[1], Cc, 'int')
        assert float(_dw64(x.abs(), w.abs(), b.abs()).max()) < 2 ** 24
        y, whole, _ = _dw_run(x, w, b)
        assert torch.equal(y.double(), _dw64(x, w, b)), (N, HW, Cc)
        assert _outside(whole, YOFF, Cc)


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('HW', DW_PLANES)
def test_dw_normal_data_within_the_fmaf_chain_bound(N, HW):
    """11 * 2^-24 (sum |x w| + |b|): nine fmaf roundings of the chain that starts at the bias, and two to spare"""
    worst = 0.0
    for Cc in DW_CHANNELS:
        x, w, b = _dw_data(N, HW[0], HW[1], Cc, 'normal')
        y, whole, _ = _dw_run(x, w, b)
        bound = 11 * 2.0 ** -24 * _dw64(x.abs(), w.abs(), b.abs())
        err = (y.double() - _dw64(x, w, b)).abs()
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (N, HW, Cc)
        assert _outside(whole, YOFF, Cc)
        # the statistics of the same launch change no output bit
        y2, whole2, _ = _dw_run(x, w, b, stats=True)
        assert torch.equal(y2.view(torch.int32), y.view(torch.int32)) and _outside(whole2, YOFF, Cc)
    print('dw N %d %dx%d: worst error / bound %.3f' % (N, HW[0], HW[1], worst))


def test_dw_and_inorm_refusals_happen_before_any_launch():
    from gcc_amd import ops
    L = ops.lib()
    x = torch.zeros(2 * 6 * 6 * 16, dtype=torch.float32, device=DEV)
    y = torch.full((2 * 6 * 6 * 16,), SENTINEL, dtype=torch.float32, device=DEV)
    w, b = torch.zeros(9 * 16, dtype=torch.float32, device=DEV), torch.zeros(16, dtype=torch.float32, device=DEV)
    need = L.gcc_inorm_f32_workspace(2, 16, 36)
    assert need > 0 and need % 16 == 0
    assert L.gcc_inorm_f32_workspace(5, 16, 36) == need // 2 * 5                 # linear in N: the chunking is the plane's
    assert L.gcc_inorm_f32_workspace(0, 16, 36) == 0
    ws = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    xp, yp, wp, bp, sp = x.data_ptr(), y.data_ptr(), w.data_ptr(), b.data_ptr(), ws.data_ptr()

    def dw(xp=xp, ldx=16, yp=yp, ldy=16, wp=wp, bp=bp, N=2, H=6, W=6, Cc=16, sp=None, sb=0):
        return L.gcc_dwconv3x3_reflect_f32(xp, ldx, yp, ldy, wp, bp, N, H, W, Cc, sp, sb, None)

    def stats(xp=xp, ldx=16, N=2, H=6, W=6, Cc=16, sp=sp, sb=need):
        return L.gcc_inorm_stats_f32(xp, ldx, N, H, W, Cc, sp, sb, None)

    def apply(xp=xp, ldx=16, yp=yp, ldy=16, rp=None, ldr=0, N=2, H=6, W=6, Cc=16, act=NONE, eps=1e-5, sp=sp, sb=need):
        return L.gcc_inorm_apply_f32(xp, ldx, yp, ldy, rp, ldr, N, H, W, Cc, act, eps, sp, sb, None)

    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    assert dw(H=1) == BAD_ARG and dw(W=1) == BAD_ARG                             # ReflectionPad2d(1) needs two pixels a side
    assert dw(ldx=18) == BAD_ARG and dw(ldy=12) == BAD_ARG and dw(xp=xp + 4) == BAD_ARG and dw(yp=yp + 8) == BAD_ARG
    assert dw(wp=None) == BAD_ARG and dw(bp=None) == BAD_ARG and dw(xp=None) == BAD_ARG and dw(yp=None) == BAD_ARG
    assert dw(wp=wp + 4) == BAD_ARG and dw(N=0) == BAD_ARG
    assert dw(Cc=6, ldx=8, ldy=8) == UNSUPPORTED
    assert dw(sp=sp, sb=need - 8) == WORKSPACE and dw(sp=sp + 8, sb=need) == BAD_ARG
    assert stats(ldx=12) == BAD_ARG and stats(xp=None) == BAD_ARG and stats(sp=None) == BAD_ARG and stats(H=0) == BAD_ARG
    assert stats(Cc=6, ldx=8) == UNSUPPORTED and stats(sb=need - 8) == WORKSPACE
    assert apply(ldy=12) == BAD_ARG and apply(yp=None) == BAD_ARG and apply(sp=None) == BAD_ARG and apply(act=TANH) == BAD_ARG
    assert apply(act=LRELU) == BAD_ARG and apply(rp=xp, ldr=12) == BAD_ARG and apply(rp=xp + 4, ldr=16) == BAD_ARG
    assert apply(Cc=6, ldx=8, ldy=8) == UNSUPPORTED and apply(sb=need - 8) == WORKSPACE and apply(eps=-1.0) == BAD_ARG
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 0 and (y == SENTINEL).all()
    assert dw() == 0 and stats() == 0 and apply() == 0
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 3


# ---- 6. InstanceNorm -------------------------------------------------------------------------------------------------------------
IN_BAR = 8               # the project's bar for its fp32 routes: 8 x the error of an fp32 host evaluation of the same thing
IN_PLANES = [(2, 2), (16, 16), (24, 24), (64, 64)]
IN_CHANNELS = (4, 20, 72)


def _in_data(N, H, W, Cc, seed=0):
    """unit-variance normal data around per-channel means from 0 to 50 (where fp32 E[x^2] - E[x]^2 loses its digits), a residual"""
    g = torch.Generator().manual_seed(77 * N + 13 * H + W + Cc + seed)
    means = torch.linspace(0, 50, Cc)[None, :, None, None]
    x = (torch.randn((N, Cc, H, W), generator=g) + means).float()
    r = torch.randn((N, Cc, H, W), generator=g).float()
    return x, r


def _in_ref(x, r, relu, dtype):
    v = F.instance_norm(x.to(dtype), eps=1e-5)
    if relu:
        v = F.relu(v)
    return v + r.to(dtype) if r is not None else v


def _in_run(x, r=None, relu=False, ws=None):
    """gcc_inorm_stats_f32 (unless ws brings partials) + gcc_inorm_apply_f32 on offset windows of sentinel-filled buffers"""
    from gcc_amd import ops
    L = ops.lib()
    N, Cc, H, W = x.shape
    ldx, ldy, ldr = Cc + 8, Cc + 24, Cc + 4
    xb = _nhwc(x, ldx, XOFF, fill=9.0)
    yb = torch.full((N, H, W, ldy), SENTINEL, dtype=torch.float32, device=DEV)
    rb = _nhwc(r, ldr, 4, fill=9.0) if r is not None else None
    if ws is None:
        ws = torch.full((L.gcc_inorm_f32_workspace(N, Cc, H * W) // 8,), float('nan'), dtype=torch.float64, device=DEV)   # no zero-fill contract
        assert L.gcc_inorm_stats_f32(xb.data_ptr() + 4 * XOFF, ldx, N, H, W, Cc, ws.data_ptr(), ws.numel() * 8, None) == 0
    assert L.gcc_inorm_apply_f32(xb.data_ptr() + 4 * XOFF, ldx, yb.data_ptr() + 4 * YOFF, ldy, rb.data_ptr() + 16 if r is not None else None,
                                 ldr if r is not None else 0, N, H, W, Cc, RELU if relu else NONE, 1e-5, ws.data_ptr(), ws.numel() * 8,
                                 None) == 0
    out = yb.cpu()
    assert _outside(out, YOFF, Cc)
    return _cut(out, YOFF, Cc)


def _in_check(x, r, relu, tag, ws=None):
    want = _in_ref(x, r, relu, torch.float64)
    host = float((_in_ref(x, r, relu, torch.float32).double() - want).abs().max())
    got = _in_run(x, r, relu, ws=ws)
    err = float((got.double() - want).abs().max())
    print('%s: error %.3g, fp32 host %.3g (%.2f x)' % (tag, err, host, err / host))
    assert host > 0 and err <= IN_BAR * host, (tag, err, host)
    return got


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('HW', IN_PLANES)
def test_inorm_against_float64(N, HW):
    for Cc in IN_CHANNELS:
        x, r = _in_data(N, HW[0], HW[1], Cc)
        tag = 'inorm N %d %dx%d C %d' % (N, HW[0], HW[1], Cc)
        a = _in_check(x, None, False, tag)
        b = _in_check(x, r, True, tag + ' relu + residual')
        assert torch.equal(_in_run(x).view(torch.int32), a.view(torch.int32)), 'two runs, two results'
        if N > 1:
            for n in range(N):                           # an image alone equals the image in its batch, bit for bit
                alone = _in_run(x[n:n + 1], r[n:n + 1], True)
                assert torch.equal(alone.view(torch.int32), b[n:n + 1].contiguous().view(torch.int32)), (tag, n)


def test_inorm_many_chunks():
    """one 256 x 256 plane at C = 8: the partial fold has 64 chunks of 1024 pixels"""
    x, r = _in_data(1, 256, 256, 8)
    _in_check(x, None, False, 'inorm 256x256 C 8')
    _in_check(x, r, True, 'inorm 256x256 C 8 relu + residual')


def test_inorm_the_naive_variance_would_fail_the_bar():
    """the bar has teeth: fp32 E[x^2] - E[x]^2 on this data is far outside it"""
    x, _ = _in_data(2, 64, 64, 16)
    want = _in_ref(x, None, False, torch.float64)
    host = float((_in_ref(x, None, False, torch.float32).double() - want).abs().max())
    m, m2 = x.mean((2, 3), keepdim=True), (x * x).mean((2, 3), keepdim=True)
    naive = (x - m) * torch.rsqrt((m2 - m * m).clamp_min(0) + 1e-5)
    assert float((naive.double() - want).abs().max()) > IN_BAR * host


def test_inorm_a_zero_channel_stays_zero():
    x, r = _in_data(2, 24, 24, 20)
    x[:, 7] = 0
    x[:, 19] = 0
    got = _in_run(x)
    assert not got[:, 7].any() and not got[:, 19].any() and got[:, 6].any()
    got = _in_run(x, relu=True)
    assert not got[:, 7].any() and not got[:, 19].any()


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('HW', DW_PLANES + [(64, 64)])
def test_inorm_apply_fed_by_the_depthwise_launch(N, HW):
    """gcc_dwconv3x3_reflect_f32 with a statistics pointer, then apply alone: the same bar, on the depthwise output"""
    for Cc in DW_CHANNELS:
        x, w, b = _dw_data(N, HW[0], HW[1], Cc, 'normal')
        x = x + torch.linspace(0, 50, Cc)[None, :, None, None].double()
        y, _, ws = _dw_run(x, w, b, stats=True)
        assert torch.isfinite(ws).all()                  # every partial was written
        _in_check(y, None, False, 'dw + inorm N %d %dx%d C %d' % (N, HW[0], HW[1], Cc), ws=ws)
