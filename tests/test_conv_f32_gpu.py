"""gcc_conv_eval_f32 (fp32 NHWC activations x fp32 weights on the f32-input MFMA) against torch-CPU float64: an exact layout check
on integer data, a derived per-element bound on seeded normal data, batch / tile invariance bit for bit, and the refusals, at
the smallest shapes at which the kernel can still go wrong."""
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

# N, H, W, Ci, Co, k, stride, dilation (pad = dilation (k // 2)); optional: ldx, ldy / yoff, residual ld / off, relu
CASES = {
    'co8': dict(g=(2, 8, 12, 8, 8, 3, 1, 1)),                          # 192 pixels: a tile straddles the images, Co below a tile
    'co24': dict(g=(2, 8, 12, 8, 24, 3, 1, 1)),                        # a partial column tile
    'co136': dict(g=(2, 8, 12, 8, 136, 3, 1, 1)),                      # several column tiles, the last partial
    'ci72': dict(g=(2, 8, 12, 72, 8, 3, 1, 1)),                        # K = 648: the LDS stages wrap many times
    'stem': dict(g=(1, 8, 8, 3, 8, 7, 1, 1), ldx=8),                   # K = 147: no multiple of the K step; borders everywhere
    'stem_ld4': dict(g=(1, 8, 8, 3, 16, 7, 1, 1), ldx=4),
    'dil2': dict(g=(1, 8, 8, 8, 8, 3, 1, 2)),
    'dil4': dict(g=(1, 8, 8, 8, 8, 3, 1, 4)),                          # most pixels see the centre tap and little else
    's2': dict(g=(2, 8, 12, 8, 8, 3, 2, 1)),
    'k1s2': dict(g=(2, 8, 12, 8, 16, 1, 2, 1)),                        # the downsample conv
    'pixel': dict(g=(1, 1, 1, 8, 8, 1, 1, 1)),
    'odd': dict(g=(2, 7, 11, 8, 8, 1, 1, 1)),                          # 154 pixels
    'co72': dict(g=(2, 8, 12, 16, 72, 3, 1, 1)),                       # 64-wide tiles: one full, one partial
    'big': dict(g=(1, 128, 256, 8, 136, 3, 1, 1)),                     # 32768 pixels x 136 channels: the 128 x 128 tile
    'window': dict(g=(2, 8, 12, 8, 8, 3, 1, 1), ldy=32, yoff=8, res=(16, 4)),
    'relu': dict(g=(2, 8, 12, 8, 8, 3, 1, 1), relu=True),
    'res': dict(g=(2, 8, 12, 8, 24, 3, 1, 1), res=(24, 0)),
    'relu_res': dict(g=(2, 8, 12, 8, 24, 3, 1, 1), res=(32, 8), relu=True),
}


def _geometry(name):
    c = CASES[name]
    N, H, W, Ci, Co, k, s, d = c['g']
    pad = d * (k // 2)
    Ho, Wo = (H + 2 * pad - d * (k - 1) - 1) // s + 1, (W + 2 * pad - d * (k - 1) - 1) // s + 1
    return SimpleGeom(N, H, W, Ci, Co, k, s, d, pad, Ho, Wo, c.get('ldx', Ci), c.get('ldy', Co), c.get('yoff', 0), c.get('res'),
                      bool(c.get('relu')))


class SimpleGeom:
    def __init__(self, *a):
        (self.N, self.H, self.W, self.Ci, self.Co, self.k, self.s, self.d, self.pad, self.Ho, self.Wo, self.ldx, self.ldy, self.yoff,
         self.res, self.relu) = a


@functools.lru_cache(maxsize=None)
def _data(name, kind):
    """(x [N, Ci, H, W], w [Co, Ci, k, k], scale, shift, residual [N, Co, Ho, Wo] or None) on the host, float64; kind 'int':
    small integers (x in [-3, 3], every weight a distinct integer of magnitude <= 8190, so every partial sum of the <= 648
    products is an integer below 2^24 and exact in fp32), no scale / shift; kind 'normal': seeded normal data"""
    q = _geometry(name)
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + (1 if kind == 'int' else 2))
    if kind == 'int':
        x = torch.randint(-3, 4, (q.N, q.Ci, q.H, q.W), generator=g).double()
        idx = torch.arange(q.Co * q.Ci * q.k * q.k, dtype=torch.int64)
        w = ((idx * 7919) % 16381 - 8190).double().reshape(q.Co, q.Ci, q.k, q.k)        # asymmetric: a swapped index shows
        scale = shift = None
        res = torch.randint(-40000, 40001, (q.N, q.Co, q.Ho, q.Wo), generator=g).double() if q.res else None
    else:
        x = torch.randn((q.N, q.Ci, q.H, q.W), generator=g).float().double()
        w = (torch.randn((q.Co, q.Ci, q.k, q.k), generator=g) * 0.2).float().double()
        scale = (torch.rand(q.Co, generator=g) + 0.5).float().double() * torch.where(torch.arange(q.Co) % 3 == 0, -1.0, 1.0)
        shift = (torch.randn(q.Co, generator=g) * 0.3).float().double()
        res = torch.randn((q.N, q.Co, q.Ho, q.Wo), generator=g).float().double() if q.res else None
    return x, w, scale, shift, res


def _conv64(q, x, w):
    return F.conv2d(x, w, None, q.s, q.pad, q.d)


@functools.lru_cache(maxsize=None)
def _want(name, kind):
    """float64 result and the per-element magnitude  |scale| sum |x w| + |shift| + |residual|  of a case"""
    q = _geometry(name)
    x, w, scale, shift, res = _data(name, kind)
    y, mag = _conv64(q, x, w), _conv64(q, x.abs(), w.abs())
    if scale is not None:
        y = y * scale[None, :, None, None] + shift[None, :, None, None]
        mag = mag * scale.abs()[None, :, None, None] + shift.abs()[None, :, None, None]
    if res is not None:
        y, mag = y + res, mag + res.abs()
    pre = y
    if q.relu:
        y = torch.relu(y)
    return y, mag, pre


def _pack(w):
    from gcc_amd import ops
    return ops.pack_weights_f32(w.float().to(DEV))


def _nhwc(t, ld, off, fill=0.0):
    """[N, C, H, W] float64 host -> NHWC fp32 device buffer [N, H, W, ld] with the channels at `off`"""
    N, Cc, H, W = t.shape
    buf = torch.full((N, H, W, ld), fill, dtype=torch.float32)
    buf[..., off:off + Cc] = t.permute(0, 2, 3, 1).float()
    return buf.to(DEV)


def _launch(q, xb, wp, yb, scale, shift, resb, N=None, act=None, dilation=None):
    from gcc_amd import _lib, ops
    d = ops.conv_desc(N or q.N, q.H, q.W, q.Ci, q.Co, q.k, q.s, q.pad, q.ldx, q.ldy)
    d.yoff = q.yoff
    ep = _lib.eval_f32_epilogue_t(scale.data_ptr() if scale is not None else None, shift.data_ptr() if shift is not None else None,
                                  resb.data_ptr() if resb is not None else None, q.res[0] if q.res else 0, q.res[1] if q.res else 0,
                                  (RELU if q.relu else NONE) if act is None else act, q.d if dilation is None else dilation)
    return ops.lib().gcc_conv_eval_f32(C.byref(d), xb.data_ptr(), wp.data_ptr(), yb.data_ptr(), C.byref(ep), None)


def _run(name, kind):
    """(result [N, Co, Ho, Wo] on the host, the whole output buffer on the host) of a case through the library"""
    q = _geometry(name)
    x, w, scale, shift, res = _data(name, kind)
    xb = _nhwc(x, q.ldx, 0, fill=9.0)                       # the stem's fourth channel is read and ignored, the rest never read
    yb = torch.full((q.N, q.Ho, q.Wo, q.ldy), SENTINEL, dtype=torch.float32, device=DEV)
    resb = _nhwc(res, q.res[0], q.res[1], fill=5.0) if q.res else None
    sc = scale.float().to(DEV) if scale is not None else None
    sh = shift.float().to(DEV) if shift is not None else None
    assert _launch(q, xb, _pack(w), yb, sc, sh, resb) == 0, name
    out = yb.cpu()
    return out[..., q.yoff:q.yoff + q.Co].permute(0, 3, 1, 2).contiguous(), out


# ---- 1. exact layout check ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_integer_data_is_exact(name):
    q = _geometry(name)
    got, whole = _run(name, 'int')
    want, mag, pre = _want(name, 'int')
    assert float(mag.max()) < 2 ** 24                        # every partial sum is exact in fp32
    assert torch.equal(got.double(), want), name
    keep = torch.ones(q.ldy, dtype=torch.bool)
    keep[q.yoff:q.yoff + q.Co] = False
    assert (whole[..., keep] == SENTINEL).all()              # nothing outside the window is written
    if q.relu and q.res:                                     # the residual is added BEFORE the ReLU: the order changes the sign
        conv = _conv64(q, *_data(name, 'int')[:2])
        flips = (conv > 0) & (pre < 0)
        assert flips.any()
        assert (got.double()[flips] == 0).all()


# ---- 2. seeded normal data, per element ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_normal_data_within_the_fmaf_chain_bound(name):
    """|got - f64| <= (K + 4) 2^-24 (|scale| sum |x w| + |shift| + |residual|) per element: K fmaf roundings of the chain, the
    epilogue's fmaf, the residual add, and the inputs' own conversions are exact (they are fp32 values)"""
    q = _geometry(name)
    got, whole = _run(name, 'normal')
    want, mag, _ = _want(name, 'normal')
    K = q.k * q.k * q.Ci
    bound = (K + 4) * 2.0 ** -24 * mag
    err = (got.double() - want).abs()
    print('%s: K %d, worst error / bound %.3f' % (name, K, float((err / bound).max())))
    assert (err <= bound).all(), name
    keep = torch.ones(q.ldy, dtype=torch.bool)
    keep[q.yoff:q.yoff + q.Co] = False
    assert (whole[..., keep] == SENTINEL).all()


# ---- 3. batch and tile invariance ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['co8', 'co136', 'ci72', 's2', 'odd', 'relu_res'])
def test_two_images_equal_two_single_images_bit_for_bit(name):
    q = _geometry(name)
    x, w, scale, shift, res = _data(name, 'normal')
    both, _ = _run(name, 'normal')
    wp = _pack(w)
    sc, sh = scale.float().to(DEV), shift.float().to(DEV)
    for n in range(q.N):
        xb = _nhwc(x[n:n + 1], q.ldx, 0)
        yb = torch.full((1, q.Ho, q.Wo, q.ldy), SENTINEL, dtype=torch.float32, device=DEV)
        resb = _nhwc(res[n:n + 1], q.res[0], q.res[1]) if q.res else None
        assert _launch(q, xb, wp, yb, sc, sh, resb, N=1) == 0
        one = yb.cpu()[..., q.yoff:q.yoff + q.Co].permute(0, 3, 1, 2)
        assert torch.equal(one.view(torch.int32), both[n:n + 1].view(torch.int32)), (name, n)


def test_every_tile_shape_is_exercised():
    from gcc_amd import ops
    for name, route in (('big', 0), ('co136', 1), ('co72', 1), ('co24', 2), ('co8', 2)):
        q = _geometry(name)
        d = ops.conv_desc(q.N, q.H, q.W, q.Ci, q.Co, q.k, q.s, q.pad, q.ldx, q.ldy)
        assert ops.lib().gcc_conv_eval_f32_route(C.byref(d), q.d) == route, name


def test_tile_shapes_agree_bit_for_bit():
    """the same pixels and channels through the 128 x 32 tile (Co 32) and the 64 x 64 tile (Co 72, its first 32 channels), and
    the first image of 'big' alone (64 x 64 tiles) against the 128 x 128 tiles of the whole: the order of K does not depend on
    the tile"""
    from gcc_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 16, 8, 12), generator=g)
    w = torch.randn((72, 16, 3, 3), generator=g) * 0.2
    xb = _nhwc(x, 16, 0)
    outs = []
    for Co in (32, 72):
        y = ops.new_act_f32(2, Co, 8, 12, DEV)
        ops.conv_eval_f32(xb.permute(0, 3, 1, 2), ops.pack_weights_f32(w[:Co].to(DEV)), Co, 3, 1, 1, y)
        outs.append(y.cpu())
    routes = [ops.conv_eval_f32(xb.permute(0, 3, 1, 2), None, Co, 3, 1, 1, ops.new_act_f32(2, Co, 8, 12, DEV), route_only=True)
              for Co in (32, 72)]
    assert routes == [2, 1]
    assert torch.equal(outs[0].view(torch.int32), outs[1][:, :32].contiguous().view(torch.int32))
    # 'big' (128 x 128 tiles) and its top 16 rows alone (4096 pixels: 64 x 64 tiles); the rows the cut does not touch agree
    q = _geometry('big')
    x, w, scale, shift, _ = _data('big', 'normal')
    whole, _ = _run('big', 'normal')
    y = ops.new_act_f32(1, q.Co, 16, q.W, DEV)
    top = _nhwc(x[:, :, :16], q.ldx, 0).permute(0, 3, 1, 2)
    assert ops.conv_eval_f32(top, None, q.Co, 3, 1, 1, y, route_only=True) == 1
    ops.conv_eval_f32(top, _pack(w), q.Co, 3, 1, 1, y, scale=scale.float().to(DEV), shift=shift.float().to(DEV))
    assert torch.equal(y.cpu()[:, :, :15].contiguous().view(torch.int32), whole[:, :, :15].contiguous().view(torch.int32))


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_happen_before_any_launch():
    from gcc_amd import _lib, ops
    L = ops.lib()
    x = torch.zeros(2 * 8 * 12 * 16, dtype=torch.float32, device=DEV)
    y = torch.full((2 * 8 * 12 * 32,), SENTINEL, dtype=torch.float32, device=DEV)
    w = torch.zeros(32 * 7 * 7 * 16, dtype=torch.float32, device=DEV)
    xp, yp, wp = x.data_ptr(), y.data_ptr(), w.data_ptr()

    def call(xp=xp, wp=wp, yp=yp, ep='default', dilation=1, act=NONE, res=None, ldr=0, roff=0, **over):
        f = dict(N=2, H=8, W=12, Ci=8, Co=8, k=3, stride=1, pad=1, ldx=8, ldy=8)
        f.update({k_: v for k_, v in over.items() if k_ in f})
        d = ops.conv_desc(*(f[k_] for k_ in ('N', 'H', 'W', 'Ci', 'Co', 'k', 'stride', 'pad', 'ldx', 'ldy')))
        for k_ in ('xoff', 'yoff', 'KW'):
            if k_ in over:
                setattr(d, k_, over[k_])
        e = _lib.eval_f32_epilogue_t(None, None, res, ldr, roff, act, dilation)
        return L.gcc_conv_eval_f32(C.byref(d), xp, wp, yp, C.byref(e) if ep == 'default' else None, None), \
            L.gcc_conv_eval_f32_route(C.byref(d), dilation)

    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    assert call(xp=None)[0] == BAD_ARG
    assert call(wp=None)[0] == BAD_ARG
    assert call(yp=None)[0] == BAD_ARG
    assert call(ep=None)[0] == BAD_ARG
    assert L.gcc_conv_eval_f32_route(None, 1) == BAD_ARG
    assert call(xp=xp + 4)[0] == BAD_ARG                                   # not 16-byte aligned
    assert call(ldx=10) == (BAD_ARG, BAD_ARG)                              # ld no multiple of 4
    assert call(ldy=10) == (BAD_ARG, BAD_ARG)
    assert call(xoff=2) == (BAD_ARG, BAD_ARG)
    assert call(ldy=16, yoff=12) == (BAD_ARG, BAD_ARG)                     # the window does not fit its ld
    assert call(ldx=16, xoff=12) == (BAD_ARG, BAD_ARG)
    assert call(Ci=3, ldx=4, xoff=4) == (BAD_ARG, BAD_ARG)
    assert call(res=xp, ldr=8, roff=4)[0] == BAD_ARG                       # the residual's window outside its ld
    assert call(res=xp, ldr=10, roff=0)[0] == BAD_ARG
    assert call(dilation=0) == (BAD_ARG, BAD_ARG)
    assert call(act=2)[0] == BAD_ARG                                       # tanh: not an act of this call
    assert call(Co=12, ldy=12) == (UNSUPPORTED, UNSUPPORTED)               # Co no multiple of 8
    assert call(Ci=4, ldx=4) == (UNSUPPORTED, UNSUPPORTED)
    assert call(KW=1) == (UNSUPPORTED, UNSUPPORTED)                        # KH != KW
    assert call(k=5, pad=2) == (UNSUPPORTED, UNSUPPORTED)
    assert call(stride=3) == (UNSUPPORTED, UNSUPPORTED)
    assert call(pad=0) == (UNSUPPORTED, UNSUPPORTED)                       # pad != dilation (k // 2)
    assert call(dilation=3, pad=3) == (UNSUPPORTED, UNSUPPORTED)
    good = call()
    assert good[1] == 2                                                    # the geometry itself is served (128 x 32 tile)
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 1 and good[0] == 0                     # ... and was the only launch
    assert (y[8 * 2 * 8 * 12:] == SENTINEL).all()
    y.fill_(SENTINEL)
    L.gcc_launch_count(1)
    assert call(Co=12, ldy=12)[0] == UNSUPPORTED and call(dilation=0)[0] == BAD_ARG
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 0 and (y == SENTINEL).all()


def test_input_kernel_and_weight_packing():
    """gcc_nchw_f32_to_nhwc_f32 moves bits and zero-fills its pad channels; pack_weights_f32 is the layout the header states"""
    from gcc_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 3, 7, 11), generator=g)
    buf = torch.full((2, 7, 11, 8), SENTINEL, dtype=torch.float32, device=DEV)
    ops.nchw_to_nhwc_f32(x.to(DEV), buf.permute(0, 3, 1, 2)[:, :3], 4)
    got = buf.cpu()
    assert torch.equal(got[..., :3], x.permute(0, 2, 3, 1)) and (got[..., 3] == 0).all() and (got[..., 4:] == SENTINEL).all()
    w = torch.randn((8, 3, 7, 7), generator=g)
    p = ops.pack_weights_f32(w.to(DEV)).cpu()
    assert tuple(p.shape) == (8, 208)                                      # 49 taps x 4 = 196 -> 208
    assert torch.equal(p[:, :196].view(8, 7, 7, 4)[..., :3], w.permute(0, 2, 3, 1))
    assert (p[:, :196].view(8, 49, 4)[..., 3] == 0).all() and (p[:, 196:] == 0).all()
    L = ops.lib()
    L.gcc_launch_count(1)
    assert L.gcc_nchw_f32_to_nhwc_f32(x.to(DEV).data_ptr(), buf.data_ptr(), 2, 3, 7, 11, 8, 0, 3, None) == BAD_ARG     # cfill
    assert L.gcc_nchw_f32_to_nhwc_f32(x.to(DEV).data_ptr(), buf.data_ptr(), 2, 3, 7, 11, 8, 8, 4, None) == BAD_ARG     # window
    assert L.gcc_nchw_f32_to_nhwc_f32(None, buf.data_ptr(), 2, 3, 7, 11, 8, 0, 4, None) == BAD_ARG
    assert L.gcc_launch_count(0) == 0
