"""gcc_conv_eval_f32_unet (Conv2d / ConvTranspose2d k4 s2 p1 in fp32 with two activated outputs) against torch-CPU float64 at the
U-Net's geometries, by the method of tests/test_conv_f32_act_gpu.py: an exact layout check on integer data (a wrong phase-to-tap
mapping or strided store shows as a wrong integer), a derived per-element bound on seeded normal data, batch invariance bit for
bit, the refusals, and the bits of all five fp32 entries pinned to what the library gave before their kernel bodies were merged."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAD_ARG, UNSUPPORTED = -1, -2
NONE, TANH, RELU, LRELU = 0, 2, 3, 4
SENTINEL = -1234.5625
XOFF, YOFF = 4, 8        # x is read at channel 4 of an ld of ceil4(Ci) + 8; y is written at channel 8, y2 at Co + 16 of ONE buffer
# the device library's tanhf is documented (HIP math API, single precision) with a maximum error of 2 ulps; |tanh| <= 1
TANH_ERR = 2 * float(np.spacing(np.float32(1.0)))

# name: (transposed, N, H, W of the input, Ci, Co, the tile the library takes)
CASES = {
    'fwd_2x2': (0, 1, 2, 2, 8, 8, 2),                  # one output pixel, 12 of its 16 taps in the padding
    'fwd_stem': (0, 2, 6, 10, 3, 24, 2),               # the stem: the pad channel of x holds a sentinel
    'fwd_co72': (0, 3, 4, 4, 16, 72, 1),
    'fwd_big': (0, 1, 256, 256, 8, 136, 0),            # 128 tiles of 128 pixels x 2 of 128 channels, Co past one tile
    'tr_1x1': (1, 1, 1, 1, 8, 8, 2),
    'tr_3x5': (1, 2, 3, 5, 16, 24, 2),
    'tr_ci72': (1, 3, 2, 2, 72, 16, 2),
    'tr_big': (1, 1, 128, 128, 8, 136, 0),
}
# (act of y, act of y2 or None): the U-Net's pair, the two single outputs it uses, and tanh on the second output
ACT_PAIRS = {'lrelu_relu': (LRELU, RELU), 'relu': (RELU, None), 'tanh_none': (TANH, NONE), 'none_tanh': (NONE, TANH)}


class Geom:
    def __init__(self, name):
        self.tr, self.N, self.H, self.W, self.Ci, self.Co, self.route = CASES[name]
        self.Ho, self.Wo = (2 * self.H, 2 * self.W) if self.tr else (self.H // 2, self.W // 2)
        self.K = (4 if self.tr else 16) * self.Ci              # products of one output element's chain
        self.ldx, self.ldy = (self.Ci + 3) // 4 * 4 + 8, 2 * self.Co + 24
        self.y2off = self.Co + 16


@functools.lru_cache(maxsize=None)
def _data(name, kind):
    """(x, w, scale, shift, slope) on the host in float64; w is Conv2d's [Co, Ci, 4, 4] or ConvTranspose2d's [Ci, Co, 4, 4].
    'int': x in [-3, 3], asymmetric integer weights of magnitude <= 4095 (8191 distinct values: a swapped index shows), scale in
    {-2, -1, 1, 2}, integer shift, the slope a power of two: every partial sum, the epilogue and slope z are exact in fp32;
    'normal': seeded normal data (fp32 values)."""
    q = Geom(name)
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + (1 if kind == 'int' else 2))
    wshape = (q.Ci, q.Co, 4, 4) if q.tr else (q.Co, q.Ci, 4, 4)
    if kind == 'int':
        x = torch.randint(-3, 4, (q.N, q.Ci, q.H, q.W), generator=g).double()
        idx = torch.arange(q.Co * q.Ci * 16, dtype=torch.int64)
        w = ((idx * 7919) % 8191 - 4095).double().reshape(wshape)
        scale = torch.tensor([1.0, -2.0, 2.0, -1.0]).repeat(q.Co)[:q.Co].double()
        shift = torch.randint(-50, 51, (q.Co,), generator=g).double()
        slope = 0.25
    else:
        x = torch.randn((q.N, q.Ci, q.H, q.W), generator=g).float().double()
        w = (torch.randn(wshape, generator=g) * 0.2).float().double()
        scale = (torch.rand(q.Co, generator=g) + 0.5).float().double() * torch.where(torch.arange(q.Co) % 3 == 0, -1.0, 1.0)
        shift = (torch.randn(q.Co, generator=g) * 0.3).float().double()
        slope = float(torch.tensor(0.2).float())
    return x, w, scale, shift, slope


def _conv64(q, x, w):
    return F.conv_transpose2d(x, w, None, 2, 1) if q.tr else F.conv2d(x, w, None, 2, 1)


@functools.lru_cache(maxsize=None)
def _want(name, kind):
    """(the float64 pre-activation z, the per-element magnitude |scale| sum |x w| + |shift|) of a case"""
    q = Geom(name)
    x, w, scale, shift, _ = _data(name, kind)
    pre = _conv64(q, x, w) * scale[None, :, None, None] + shift[None, :, None, None]
    mag = _conv64(q, x.abs(), w.abs()) * scale.abs()[None, :, None, None] + shift.abs()[None, :, None, None]
    assert tuple(pre.shape) == (q.N, q.Co, q.Ho, q.Wo)
    return pre, mag


def _act64(v, act, slope):
    if act == RELU:
        return torch.relu(v)
    if act == LRELU:
        return torch.where(v >= 0, v, slope * v)
    return torch.tanh(v) if act == TANH else v


def _nhwc(t, ld, off, fill):
    N, Cc, H, W = t.shape
    buf = torch.full((N, H, W, ld), fill, dtype=torch.float32)
    buf[..., off:off + Cc] = t.permute(0, 2, 3, 1).float()
    return buf.to(DEV)


@functools.lru_cache(maxsize=None)
def _packed(name, kind):
    from gcc_amd import ops
    q = Geom(name)
    return ops.pack_weights_f32_unet(_data(name, kind)[1].float().to(DEV), bool(q.tr))


def _run(name, kind, pair, image=None):
    """(y, y2 or None as [N, Co, Ho, Wo] on the host, the whole output buffer on the host) of a case -- or of its image `image`"""
    from gcc_amd import _lib, ops
    q = Geom(name)
    act, act2 = ACT_PAIRS[pair]
    x, w, scale, shift, slope = _data(name, kind)
    if image is not None:
        x = x[image:image + 1]
    N = x.shape[0]
    xb = _nhwc(x, q.ldx, XOFF, fill=9.0)                       # with Ci == 3 channel XOFF + 3, the pad channel, holds 9 too
    yb = torch.full((N, q.Ho, q.Wo, q.ldy), SENTINEL, dtype=torch.float32, device=DEV)
    sc, sh = scale.float().to(DEV), shift.float().to(DEV)
    d = ops.conv_desc(N, q.H, q.W, q.Ci, q.Co, 4, 2, 1, q.ldx, q.ldy)
    d.xoff, d.yoff = XOFF, YOFF
    ep = _lib.eval_f32_unet_epilogue_t(sc.data_ptr(), sh.data_ptr(), yb.data_ptr() if act2 is not None else None,
                                       q.ldy if act2 is not None else 0, q.y2off if act2 is not None else 0, act,
                                       act2 if act2 is not None else 0, slope, 0)
    L = ops.lib()
    route = L.gcc_conv_eval_f32_unet_route(C.byref(d), q.tr)
    if image is None:
        assert route == q.route, (name, route)
    assert L.gcc_conv_eval_f32_unet(C.byref(d), q.tr, xb.data_ptr(), _packed(name, kind).data_ptr(), yb.data_ptr(), C.byref(ep), None) == 0
    out = yb.cpu()
    cut = lambda off: out[..., off:off + q.Co].permute(0, 3, 1, 2).contiguous()
    return cut(YOFF), (cut(q.y2off) if act2 is not None else None), out


def _only_the_windows_are_written(q, whole, second):
    keep = torch.ones(q.ldy, dtype=torch.bool)
    keep[YOFF:YOFF + q.Co] = False
    if second:
        keep[q.y2off:q.y2off + q.Co] = False
    return bool((whole[..., keep] == SENTINEL).all())


PARAMS = [(n, p) for n in CASES for p in ACT_PAIRS]


# ---- 1. exact layout check ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,pair', PARAMS)
def test_integer_data_is_exact(name, pair):
    """every element of y and y2 equals the float64 conv2d / conv_transpose2d result.  tanh of an integer is no fp32 number:
    there the pre-activation is exact by the same argument and the element is within the device tanhf's documented error of the
    float64 tanh of it (0 and +-1 come out exactly)"""
    q = Geom(name)
    y, y2, whole = _run(name, 'int', pair)
    pre, mag = _want(name, 'int')
    slope = _data(name, 'int')[4]
    assert float(mag.max()) < 2 ** 24                        # every partial sum and the epilogue are exact in fp32
    for got, act in ((y, ACT_PAIRS[pair][0]), (y2, ACT_PAIRS[pair][1])):
        if got is None:
            continue
        want = _act64(pre, act, slope)
        if act == TANH:
            assert ((got.double() - want).abs() <= TANH_ERR).all(), name
            assert torch.equal(got.double()[pre == 0], want[pre == 0]) and torch.equal(got.double()[pre.abs() > 20], want[pre.abs() > 20])
        else:
            assert torch.equal(got.double(), want), name
    assert _only_the_windows_are_written(q, whole, y2 is not None)


# ---- 2. seeded normal data, per element ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,pair', PARAMS)
def test_normal_data_within_the_fmaf_chain_bound(name, pair):
    """b = (K + 3) 2^-24 (|scale| sum |x w| + |shift|) bounds the pre-activation: K fmaf roundings of the chain (K = 16 Ci
    forward, 4 Ci per phase transposed; the zero products of padded taps round nothing) and the epilogue's fmaf.  ReLU does not
    widen a difference; LeakyReLU multiplies it by at most max(1, slope) and rounds slope z once more (2^-24 slope (|z| + b));
    tanh has a derivative of at most 1 and adds the device function's documented error"""
    q = Geom(name)
    y, y2, whole = _run(name, 'normal', pair)
    pre, mag = _want(name, 'normal')
    slope = _data(name, 'normal')[4]
    for got, act in ((y, ACT_PAIRS[pair][0]), (y2, ACT_PAIRS[pair][1])):
        if got is None:
            continue
        bound = (q.K + 3) * 2.0 ** -24 * mag
        if act == LRELU:
            bound = max(1.0, abs(slope)) * bound + 2.0 ** -24 * abs(slope) * (pre.abs() + bound)
        elif act == TANH:
            bound = bound + TANH_ERR
        err = (got.double() - _act64(pre, act, slope)).abs()
        print('%s %s act %d: K %d, worst error / bound %.3f' % (name, pair, act, q.K, float((err / bound.clamp_min(1e-300)).max())))
        assert (err <= bound).all(), name
    assert _only_the_windows_are_written(q, whole, y2 is not None)


# ---- 3. the batch, the tiles --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['fwd_stem', 'fwd_co72', 'tr_3x5', 'tr_ci72'])
def test_an_image_alone_equals_the_image_in_its_batch_bit_for_bit(name):
    q = Geom(name)
    y, y2, _ = _run(name, 'normal', 'lrelu_relu')
    for n in range(q.N):
        a, a2, whole = _run(name, 'normal', 'lrelu_relu', image=n)
        assert _only_the_windows_are_written(q, whole, True)
        assert torch.equal(a.view(torch.int32), y[n:n + 1].contiguous().view(torch.int32)), (name, n)
        assert torch.equal(a2.view(torch.int32), y2[n:n + 1].contiguous().view(torch.int32)), (name, n)


def test_every_tile_shape_is_exercised_in_both_directions():
    from gcc_amd import ops
    seen = set()
    for name in CASES:
        q = Geom(name)
        d = ops.conv_desc(q.N, q.H, q.W, q.Ci, q.Co, 4, 2, 1, q.ldx, q.ldy)
        d.xoff, d.yoff = XOFF, YOFF
        assert ops.lib().gcc_conv_eval_f32_unet_route(C.byref(d), q.tr) == q.route, name
        seen.add(q.route)
    assert seen == {0, 1, 2}
    # 64 x 64 tiles transposed too: the generator's inner up convs (Co > 32 on a small map)
    d = ops.conv_desc(2, 2, 2, 64, 64, 4, 2, 1, 64, 64)
    assert ops.lib().gcc_conv_eval_f32_unet_route(C.byref(d), 1) == 1


def test_transposed_64x64_tile_is_exact():
    """the one tile shape the listed transposed cases do not take: (2, 2x2, 16 -> 40), integer data, through ops"""
    from gcc_amd import _lib, ops
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (2, 16, 2, 2), generator=g).double()
    w = torch.randint(-2000, 2001, (16, 40, 4, 4), generator=g).double()
    xv = _nhwc(x, 16, 0, 0.0).permute(0, 3, 1, 2)
    out, out2 = ops.new_act_f32(2, 40, 4, 4, DEV), ops.new_act_f32(2, 40, 4, 4, DEV)
    wp = ops.pack_weights_f32_unet(w.float().to(DEV), True)
    assert ops.conv_eval_f32_unet(xv, wp, 40, out, transposed=True, route_only=True) == 1
    ops.conv_eval_f32_unet(xv, wp, 40, out, transposed=True, act=_lib.EVAL_ACT_LRELU, y2=out2, act2=_lib.EVAL_ACT_RELU, slope=0.25)
    pre = F.conv_transpose2d(x, w, None, 2, 1)
    assert torch.equal(out.cpu().double(), torch.where(pre >= 0, pre, 0.25 * pre)) and torch.equal(out2.cpu().double(), torch.relu(pre))


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_happen_before_any_launch():
    from gcc_amd import _lib, ops
    L = ops.lib()
    x = torch.zeros(2 * 8 * 12 * 16, dtype=torch.float32, device=DEV)
    y = torch.full((2 * 16 * 24 * 64,), SENTINEL, dtype=torch.float32, device=DEV)
    w = torch.zeros(4 * 32 * 16 * 16, dtype=torch.float32, device=DEV)
    xp, yp, wp = x.data_ptr(), y.data_ptr(), w.data_ptr()

    def call(tr=0, xp=xp, wp=wp, yp=yp, ep='default', act=NONE, act2=NONE, y2=None, ldy2=0, y2off=0, **over):
        f = dict(N=2, H=8, W=12, Ci=8, Co=16, KH=4, stride=2, pad=1, ldx=8, ldy=64)
        f.update({k_: v for k_, v in over.items() if k_ in f})
        d = ops.conv_desc(*(f[k_] for k_ in ('N', 'H', 'W', 'Ci', 'Co', 'KH', 'stride', 'pad', 'ldx', 'ldy')))
        d.KW = over.get('KW', f['KH'])
        d.xoff, d.yoff = over.get('xoff', 0), over.get('yoff', 0)
        e = _lib.eval_f32_unet_epilogue_t(None, None, y2, ldy2, y2off, act, act2, 0.2, 0)
        return L.gcc_conv_eval_f32_unet(C.byref(d), tr, xp, wp, yp, C.byref(e) if ep == 'default' else None, None), \
            L.gcc_conv_eval_f32_unet_route(C.byref(d), tr)

    torch.cuda.synchronize()
    L.gcc_launch_count(1)
    for tr in (0, 1):
        assert call(tr, ldx=10) == (BAD_ARG, BAD_ARG)                      # ld / off: multiples of 4 floats
        assert call(tr, ldy=66) == (BAD_ARG, BAD_ARG)
        assert call(tr, ldx=16, xoff=2) == (BAD_ARG, BAD_ARG)
        assert call(tr, yoff=6) == (BAD_ARG, BAD_ARG)
        assert call(tr, xp=xp + 4)[0] == BAD_ARG                           # pointers: 16 bytes
        assert call(tr, yp=yp + 8)[0] == BAD_ARG
        assert call(tr, wp=wp + 4)[0] == BAD_ARG
        assert call(tr, y2=yp + 8, ldy2=64, y2off=32)[0] == BAD_ARG
        assert call(tr, ldx=8, xoff=4) == (BAD_ARG, BAD_ARG)               # a window outside its ld: x, y, y2
        assert call(tr, ldy=64, yoff=52) == (BAD_ARG, BAD_ARG)
        assert call(tr, y2=yp, ldy2=64, y2off=52)[0] == BAD_ARG
        assert call(tr, y2=yp, ldy2=62, y2off=32)[0] == BAD_ARG            # and y2's own ld / off alignment
        assert call(tr, y2=yp, ldy2=64, y2off=34)[0] == BAD_ARG
        assert call(tr, y2=yp, ldy2=64, y2off=0)[0] == BAD_ARG             # y2 on y's window
        assert call(tr, y2=yp, ldy2=64, y2off=12)[0] == BAD_ARG            # y2 overlapping half of it
        assert call(tr, yoff=16, y2=yp, ldy2=64, y2off=4)[0] == BAD_ARG
        assert call(tr, y2=yp + 64 * 4, ldy2=64, y2off=8)[0] == BAD_ARG    # the same channels one pixel further on
        assert call(tr, y2=yp + 16 * 4, ldy2=32, y2off=0)[0] == BAD_ARG    # interleaved at another stride
        for bad in (1, 5, 7, -1):                                          # PReLU (a device slope) and anything outside the four
            assert call(tr, act=bad)[0] == BAD_ARG
            assert call(tr, y2=yp, ldy2=64, y2off=32, act2=bad)[0] == BAD_ARG
        for pad in (0, 2):
            assert call(tr, pad=pad) == (BAD_ARG, BAD_ARG)
        assert call(tr, xp=None)[0] == BAD_ARG
        assert call(tr, wp=None)[0] == BAD_ARG
        assert call(tr, yp=None)[0] == BAD_ARG
        assert call(tr, ep=None)[0] == BAD_ARG
        assert call(tr, KH=3) == (UNSUPPORTED, UNSUPPORTED)                # geometries nobody serves
        assert call(tr, KH=4, KW=3) == (UNSUPPORTED, UNSUPPORTED)
        assert call(tr, stride=1) == (UNSUPPORTED, UNSUPPORTED)
        assert call(tr, Ci=4, ldx=4) == (UNSUPPORTED, UNSUPPORTED)
        assert call(tr, Co=12) == (UNSUPPORTED, UNSUPPORTED)
    assert call(1, Ci=3, ldx=4) == (UNSUPPORTED, UNSUPPORTED)              # the 3-in-4 stem exists forward only
    assert call(0, H=1) == (BAD_ARG, BAD_ARG)                              # a map smaller than the kernel's span
    assert call(2) == (BAD_ARG, BAD_ARG) and call(-1) == (BAD_ARG, BAD_ARG)
    assert L.gcc_conv_eval_f32_unet_route(None, 0) == BAD_ARG
    assert L.gcc_conv_eval_f32_unet_kp(8, 0) == 128 and L.gcc_conv_eval_f32_unet_kp(3, 0) == 64
    assert L.gcc_conv_eval_f32_unet_kp(8, 1) == 32 and L.gcc_conv_eval_f32_unet_kp(72, 1) == 288
    assert L.gcc_conv_eval_f32_unet_kp(0, 0) == BAD_ARG and L.gcc_conv_eval_f32_unet_kp(8, 2) == BAD_ARG
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 0 and (y == SENTINEL).all()
    # what is served launches once per call: both outputs side by side in one buffer, forward [2, 4, 6] and transposed [2, 16, 24]
    assert call(0, act=LRELU, act2=RELU, y2=yp, ldy2=64, y2off=16) == (0, 2)
    torch.cuda.synchronize()
    assert L.gcc_launch_count(1) == 1
    v = y[:2 * 4 * 6 * 64].view(-1, 64)
    assert (v[:, :32] == 0).all() and (v[:, 32:] == SENTINEL).all() and (y[2 * 4 * 6 * 64:] == SENTINEL).all()
    assert call(1, act=TANH, y2=yp, ldy2=64, y2off=48) == (0, 2)
    torch.cuda.synchronize()
    assert L.gcc_launch_count(0) == 1
    v = y.view(-1, 64)
    assert (v[:, :16] == 0).all() and (v[:, 48:] == 0).all() and (v[2 * 4 * 6:, 16:48] == SENTINEL).all()


# ---- 5. the five entries keep their bits ----------------------------------------------------------------------------------------
# All five fp32 entries run one tile (gcc_amd/csrc/conv_f32_tile.hpp).  What they compute for these seeded inputs was recorded
# with the library built from the parent of the change that merged the kernel bodies (selected with GCC_HIP_LIB=) and must not
# move: the merge kept the order of every fmaf, so equality is the bar.  The first eight were first recorded with the library
# from before gcc_conv_eval_f32_unet existed, and have not moved since.
ENTRY_SHA256 = {
    'f32_k3_s1_co40': '12202ac55194abac',
    'f32_k7_s2_stem': '79bb3e4b9d28c654',
    'f32_k3_d2_co136_big': '586c167c015a1854',
    'ex_k1x7_co72': 'c30239a4acaf5b9d',
    'ex_k5_p0_s2': 'ea894386d9d67800',
    'act_k9_prelu': 'dff694b56f72f959',
    'act_k3_shuffle_co64': '04b5a2fd6fc3a83f',
    'act_k3_tanh_res': '6bb64ef3667d6c25',
    'unet_fwd_stem': '72820a78bc9aec8f',
    'unet_fwd_co72_y2': '44e8d69ac1d6d237',
    'unet_tr_ci72': 'f0167f97ad316794',
    'unet_tr_co136_big': 'ec0be4220eb21fb9',
    'resnet_rf7_stem': '2422d3c0bb840ac6',
    'resnet_rf7_co72_tanh': 'ec675fc3088e1f21',
    'resnet_rf3': 'ff07ccaf4c00aa4d',
    'resnet_tr_ci72': '680dd2d3c7422a6a',
    'resnet_tr_1x1': 'c9918623b1438e0e',
    'resnet_tr_co136_big': '33615ad6db33630c',
}


def entry_outputs(L):
    """name -> sha256 of the output bytes of the five entries of the library handle L, on fixed seeded inputs that take all three
    tile shapes of each kernel, a residual, a dilation, rectangular kernels, PReLU, tanh, the shuffled store, the U-Net's two
    outputs and both of its directions, the reflection at k 7 and k 3 and the four phases of the k3 transposed convolution"""
    from gcc_amd import _lib, ops
    P = C.c_void_p
    L.gcc_conv_eval_f32.argtypes = [C.POINTER(_lib.conv_t), P, P, P, C.POINTER(_lib.eval_f32_epilogue_t), P]
    L.gcc_conv_eval_f32_ex.argtypes = [C.POINTER(_lib.conv_t), C.c_int, C.c_int, P, P, P, C.POINTER(_lib.eval_f32_epilogue_t), P]
    L.gcc_conv_eval_f32_act.argtypes = [C.POINTER(_lib.conv_t), C.c_int, C.c_int, P, P, P, C.POINTER(_lib.eval_f32_act_epilogue_t), P]
    L.gcc_conv_eval_f32_unet.argtypes = [C.POINTER(_lib.conv_t), C.c_int, P, P, P, C.POINTER(_lib.eval_f32_unet_epilogue_t), P]
    L.gcc_conv_eval_f32_unet_route.argtypes = [C.POINTER(_lib.conv_t), C.c_int]
    L.gcc_conv_eval_f32_resnet.argtypes = [C.POINTER(_lib.conv_t), C.c_int, P, P, P, C.POINTER(_lib.eval_f32_resnet_epilogue_t), P]
    L.gcc_conv_eval_f32_resnet_route.argtypes = [C.POINTER(_lib.conv_t), C.c_int]
    out = {}

    def one(name, entry, N, H, W, Ci, Co, kh, kw, stride, ph, pw, dil=1, act=NONE, res=False, shuffle=0, slope=False):
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        x = _nhwc(torch.randn((N, Ci, H, W), generator=g), (Ci + 3) // 4 * 4, 0, 0.0)
        w = ops.pack_weights_f32((torch.randn((Co, Ci, kh, kw), generator=g) * 0.1).to(DEV))
        sc, sh = (torch.rand(Co, generator=g) + 0.5).to(DEV), torch.randn(Co, generator=g).to(DEV)
        Ho, Wo = (H + 2 * ph - dil * (kh - 1) - 1) // stride + 1, (W + 2 * pw - dil * (kw - 1) - 1) // stride + 1
        r = torch.randn((N, Ho, Wo, Co), generator=g).to(DEV) if res else None
        sl = torch.tensor([0.3], device=DEV)
        Cy, s = (Co // 4, 2) if shuffle else (Co, 1)
        y = torch.zeros((N, Ho * s, Wo * s, Cy), dtype=torch.float32, device=DEV)
        d = ops.conv_desc(N, H, W, Ci, Co, kh, stride, ph if entry == 'f32' else 0, x.shape[-1], Cy)
        d.KW = kw
        rp = r.data_ptr() if res else None
        if entry == 'f32':
            ep = _lib.eval_f32_epilogue_t(sc.data_ptr(), sh.data_ptr(), rp, Co if res else 0, 0, act, dil)
            rc = L.gcc_conv_eval_f32(C.byref(d), x.data_ptr(), w.data_ptr(), y.data_ptr(), C.byref(ep), None)
        elif entry == 'ex':
            ep = _lib.eval_f32_epilogue_t(sc.data_ptr(), sh.data_ptr(), rp, Co if res else 0, 0, act, dil)
            rc = L.gcc_conv_eval_f32_ex(C.byref(d), ph, pw, x.data_ptr(), w.data_ptr(), y.data_ptr(), C.byref(ep), None)
        else:
            ep = _lib.eval_f32_act_epilogue_t(sc.data_ptr(), sh.data_ptr(), rp, Co if res else 0, 0, act, shuffle,
                                              sl.data_ptr() if slope else None, dil, 0)
            rc = L.gcc_conv_eval_f32_act(C.byref(d), ph, pw, x.data_ptr(), w.data_ptr(), y.data_ptr(), C.byref(ep), None)
        assert rc == 0, (name, rc)
        host = y.cpu()
        assert float(host.abs().max()) > 0
        out[name] = hashlib.sha256(host.numpy().tobytes()).hexdigest()[:16]

    one('f32_k3_s1_co40', 'f32', 2, 9, 11, 8, 40, 3, 3, 1, 1, 1, act=RELU, res=True)
    one('f32_k7_s2_stem', 'f32', 2, 9, 11, 3, 16, 7, 7, 2, 3, 3)
    one('f32_k3_d2_co136_big', 'f32', 2, 128, 128, 8, 136, 3, 3, 1, 2, 2, dil=2, act=RELU)
    one('ex_k1x7_co72', 'ex', 2, 9, 11, 24, 72, 1, 7, 1, 0, 3, act=RELU)
    one('ex_k5_p0_s2', 'ex', 1, 9, 11, 8, 32, 5, 5, 2, 0, 0, res=True)
    one('act_k9_prelu', 'act', 1, 6, 7, 3, 8, 9, 9, 1, 4, 4, act=1, slope=True)
    one('act_k3_shuffle_co64', 'act', 2, 9, 11, 8, 64, 3, 3, 1, 1, 1, act=1, slope=True, shuffle=2)
    one('act_k3_tanh_res', 'act', 2, 9, 11, 24, 72, 3, 3, 1, 1, 1, act=TANH, res=True)

    def seeded(name, N, H, W, Ci, Co, wshape):
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        x = _nhwc(torch.randn((N, Ci, H, W), generator=g), (Ci + 3) // 4 * 4, 0, 0.0)
        w = (torch.randn(wshape, generator=g) * 0.1).to(DEV)
        return x, w, (torch.rand(Co, generator=g) + 0.5).to(DEV), torch.randn(Co, generator=g).to(DEV)

    def done(name, rc, tile, want_tile, *ys):
        assert rc == 0 and tile == want_tile, (name, rc, tile)
        h = hashlib.sha256()
        for y in ys:
            host = y.cpu()
            assert float(host.abs().max()) > 0
            h.update(host.numpy().tobytes())
        out[name] = h.hexdigest()[:16]

    def unet(name, tr, N, H, W, Ci, Co, tile, act=NONE, act2=None):
        x, w, sc, sh = seeded(name, N, H, W, Ci, Co, (Ci, Co, 4, 4) if tr else (Co, Ci, 4, 4))
        wp = ops.pack_weights_f32_unet(w, bool(tr))
        Ho, Wo = (2 * H, 2 * W) if tr else (H // 2, W // 2)
        y = torch.zeros((N, Ho, Wo, Co), dtype=torch.float32, device=DEV)
        y2 = torch.zeros_like(y) if act2 is not None else None
        d = ops.conv_desc(N, H, W, Ci, Co, 4, 2, 1, x.shape[-1], Co)
        ep = _lib.eval_f32_unet_epilogue_t(sc.data_ptr(), sh.data_ptr(), y2.data_ptr() if y2 is not None else None,
                                           Co if y2 is not None else 0, 0, act, act2 or 0, 0.2, 0)
        rc = L.gcc_conv_eval_f32_unet(C.byref(d), tr, x.data_ptr(), wp.data_ptr(), y.data_ptr(), C.byref(ep), None)
        done(name, rc, L.gcc_conv_eval_f32_unet_route(C.byref(d), tr), tile, *([y] if y2 is None else [y, y2]))

    def resnet(name, kind, N, H, W, Ci, Co, k, tile, act=NONE):
        tr = kind == _lib.F32_RESNET_TRANSPOSED3
        x, w, sc, sh = seeded(name, N, H, W, Ci, Co, (Ci, Co, 3, 3) if tr else (Co, Ci, k, k))
        wp = ops.pack_weights_f32_resnet(w, kind)
        y = torch.zeros((N, 2 * H, 2 * W, Co) if tr else (N, H, W, Co), dtype=torch.float32, device=DEV)
        d = ops.conv_desc(N, H, W, Ci, Co, k, 2 if tr else 1, 1 if tr else 0, x.shape[-1], Co)
        ep = _lib.eval_f32_resnet_epilogue_t(sc.data_ptr(), sh.data_ptr(), act, 0)
        rc = L.gcc_conv_eval_f32_resnet(C.byref(d), kind, x.data_ptr(), wp.data_ptr(), y.data_ptr(), C.byref(ep), None)
        done(name, rc, L.gcc_conv_eval_f32_resnet_route(C.byref(d), kind), tile, y)

    unet('unet_fwd_stem', 0, 2, 10, 12, 3, 16, 2, act=LRELU)
    unet('unet_fwd_co72_y2', 0, 3, 4, 4, 8, 72, 1, act=LRELU, act2=RELU)
    unet('unet_tr_ci72', 1, 3, 2, 2, 72, 16, 2, act=RELU)
    unet('unet_tr_co136_big', 1, 1, 128, 128, 8, 136, 0, act=TANH)
    RF, T3 = _lib.F32_RESNET_REFLECT, _lib.F32_RESNET_TRANSPOSED3
    resnet('resnet_rf7_stem', RF, 1, 4, 4, 3, 8, 7, 2, act=RELU)
    resnet('resnet_rf7_co72_tanh', RF, 3, 8, 8, 16, 72, 7, 1, act=TANH)
    resnet('resnet_rf3', RF, 2, 9, 13, 8, 24, 3, 2)
    resnet('resnet_tr_ci72', T3, 3, 2, 2, 72, 16, 3, 2, act=RELU)
    resnet('resnet_tr_1x1', T3, 1, 1, 1, 72, 16, 3, 2)
    resnet('resnet_tr_co136_big', T3, 1, 128, 128, 8, 136, 3, 0, act=RELU)
    return out


def test_the_entries_keep_their_bits():
    from gcc_amd import ops
    got = entry_outputs(ops.lib())
    print(got)
    assert got == ENTRY_SHA256
