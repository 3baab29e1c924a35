"""Host-side companions of the DRN-D segmenter tests: the key / shape table of an arch-D DRNSeg from the architecture's
constants, a seeded weight recipe (the fixtures store seeds and results, not megabytes of random weights), and a restatement of
the network in torch-CPU -- with true dilated convolutions, so that it also checks the phase-layout route -- either in fp32
or emulating the device path's number formats: bf16 weights, one bf16 rounding per conv + BatchNorm (+ ReLU) and per residual
sum, fp32 head.  Imports nothing from the reference."""
import os
import zlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'drn_seg.npz')
BN = ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')
DILATION = (1, 1, 1, 1, 1, 2, 4, 2, 1)        # base.0 .. base.8 of arch D
STRIDE = (1, 1, 2, 2, 2, 1, 1, 1, 1)
# name -> (block kind, layers, channels, input shape, weight seed, damping of each block's last BatchNorm scale)
NETS = OrderedDict([
    ('bneck', ('bottleneck', [1, 1, 1, 1, 2, 1, 1, 1], (8, 8, 8, 8, 16, 16, 16, 16), (2, 3, 64, 96), 101, 1.0)),
    ('basic', ('basic', [1, 1, 2, 2, 2, 2, 1, 1], (8, 8, 16, 16, 16, 16, 16, 16), (2, 3, 64, 64), 202, 0.5)),
    ('d105thin', ('bottleneck', [1, 1, 3, 4, 23, 3, 1, 1], (8, 8, 8, 8, 16, 16, 16, 16), (1, 3, 64, 64), 303, 0.25)),
])
D105 = ('bottleneck', [1, 1, 3, 4, 23, 3, 1, 1], (16, 32, 64, 128, 256, 512, 512, 512))
D_LAYERS = {'drn_d_22': ('basic', [1, 1, 2, 2, 2, 2, 1, 1]), 'drn_d_38': ('basic', [1, 1, 3, 4, 6, 3, 1, 1]),
            'drn_d_54': ('bottleneck', [1, 1, 3, 4, 6, 3, 1, 1]), 'drn_d_105': ('bottleneck', [1, 1, 3, 4, 23, 3, 1, 1])}


def drn_shapes(kind, layers, channels, classes=19):
    """key -> shape of DRNSeg(arch D).state_dict(), in the module order"""
    exp = 4 if kind == 'bottleneck' else 1
    sh = OrderedDict()

    def bn(prefix, c):
        for f in BN:
            sh['%s.%s' % (prefix, f)] = () if f == 'num_batches_tracked' else (c,)
    sh['base.0.0.weight'] = (channels[0], 3, 7, 7)
    bn('base.0.1', channels[0])
    cin = channels[0]
    for L in range(1, 9):
        c, n = channels[L - 1], layers[L - 1]
        if L in (1, 2, 7, 8):
            for j in range(n):
                sh['base.%d.%d.weight' % (L, 3 * j)] = (c, cin, 3, 3)
                bn('base.%d.%d' % (L, 3 * j + 1), c)
                cin = c
            continue
        for b in range(n):
            p = 'base.%d.%d.' % (L, b)
            if kind == 'bottleneck':
                sh[p + 'conv1.weight'] = (c, cin, 1, 1)
                bn(p + 'bn1', c)
                sh[p + 'conv2.weight'] = (c, c, 3, 3)
                bn(p + 'bn2', c)
                sh[p + 'conv3.weight'] = (c * 4, c, 1, 1)
                bn(p + 'bn3', c * 4)
            else:
                sh[p + 'conv1.weight'] = (c, cin, 3, 3)
                bn(p + 'bn1', c)
                sh[p + 'conv2.weight'] = (c, c, 3, 3)
                bn(p + 'bn2', c)
            if b == 0 and (STRIDE[L] != 1 or cin != c * exp):
                sh[p + 'downsample.0.weight'] = (c * exp, cin, 1, 1)
                bn(p + 'downsample.1', c * exp)
            cin = c * exp
    sh['seg.weight'] = (classes, cin, 1, 1)
    sh['seg.bias'] = (classes,)
    sh['up.weight'] = (classes, 1, 16, 16)
    return sh


def drn_state_dict(shapes, seed, damp=1.0):
    """seeded values for a drn_shapes table, one generator per tensor: conv W ~ N(0, 2 / (k k Cout)) (He), BatchNorm scale
    ~ U(.5, 1.5) (times `damp` for the last BatchNorm of a residual block: a deep net's residual sums otherwise grow without
    bound), shift ~ N(0, .2), running_mean ~ N(0, .2), running_var ~ U(.5, 1.5); seg.bias ~ N(0, .1); up.weight the bilinear
    kernel times (1 + .05 N(0, 1)), so that a head which assumed the bilinear constants would show."""
    last = 'bn3.weight' if any(k.endswith('conv3.weight') for k in shapes) else 'bn2.weight'
    sd = OrderedDict()
    for k, shp in shapes.items():
        g = torch.Generator().manual_seed(seed * 1000003 + zlib.crc32(k.encode()) % 1000003)
        shp = tuple(shp)
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.zeros((), dtype=torch.long)
        elif k == 'up.weight':
            f, c = 8, 7.5 / 8                                        # the bilinear kernel of a 16-tap, stride-8 upsampling
            t = 1 - (torch.arange(16, dtype=torch.float32) / f - c).abs()
            sd[k] = (t[:, None] * t[None, :]).expand(shp).clone() * (1 + 0.05 * torch.randn(shp, generator=g))
        elif k == 'seg.bias':
            sd[k] = torch.randn(shp, generator=g) * 0.1
        elif len(shp) == 4:
            sd[k] = torch.randn(shp, generator=g) * (2.0 / (shp[2] * shp[3] * shp[0])) ** 0.5
        elif k.endswith('running_var'):
            sd[k] = torch.rand(shp, generator=g) + 0.5
        elif k.endswith('running_mean') or k.endswith('.bias'):
            sd[k] = torch.randn(shp, generator=g) * 0.2
        else:
            sd[k] = (torch.rand(shp, generator=g) + 0.5) * (damp if k.endswith(last) else 1.0)
    return sd


def seeded_input(shape, seed):
    """what SegList hands the segmenter looks like: roughly unit-variance channels"""
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * 1.2


def fixture_net(z, name):
    """(state_dict, input) of a fixture net, rebuilt from the stored key table and seeds"""
    keys = [str(k) for k in z[name + '.keys']]
    shapes = OrderedDict((k, tuple(int(v) for v in s if v >= 0)) for k, s in zip(keys, z[name + '.shapes']))
    sd = drn_state_dict(shapes, int(z[name + '.seed']), float(z[name + '.damp']))
    return sd, seeded_input(z[name + '.input_shape'], int(z[name + '.input_seed']))


def _r(t, emulate):
    return t.bfloat16().float() if emulate else t


def forward(sd, x, emulate=True, eps=1e-5):
    """(log-softmax, scores) of the arch-D DRNSeg with the weights sd on x, from the keys alone"""
    def cba(x, wkey, bnp, stride, dil, relu=True, residual=None):
        w = _r(sd[wkey].float(), emulate)
        k = w.shape[2]
        y = F.conv2d(x, w, None, stride, dil * (k // 2), dil)
        scale = sd[bnp + '.weight'].float() / torch.sqrt(sd[bnp + '.running_var'].float() + eps)
        shift = sd[bnp + '.bias'].float() - sd[bnp + '.running_mean'].float() * scale
        y = y * scale[None, :, None, None] + shift[None, :, None, None]
        if residual is not None:
            return torch.relu(_r(y + residual, emulate))
        return _r(torch.relu(y) if relu else y, emulate)

    with torch.no_grad():
        x = cba(_r(x.float(), emulate), 'base.0.0.weight', 'base.0.1', 1, 1)
        for L in range(1, 9):
            d, s = DILATION[L], STRIDE[L]
            if L in (1, 2, 7, 8):
                j = 0
                while 'base.%d.%d.weight' % (L, 3 * j) in sd:
                    x = cba(x, 'base.%d.%d.weight' % (L, 3 * j), 'base.%d.%d' % (L, 3 * j + 1), s if j == 0 else 1, d)
                    j += 1
                continue
            b = 0
            while 'base.%d.%d.conv1.weight' % (L, b) in sd:
                p, sb = 'base.%d.%d.' % (L, b), (s if b == 0 else 1)
                res = x
                if p + 'downsample.0.weight' in sd:
                    res = cba(x, p + 'downsample.0.weight', p + 'downsample.1', sb, 1, relu=False)
                if p + 'conv3.weight' in sd:
                    y = cba(x, p + 'conv1.weight', p + 'bn1', 1, 1)
                    y = cba(y, p + 'conv2.weight', p + 'bn2', sb, d)
                    x = cba(y, p + 'conv3.weight', p + 'bn3', 1, 1, residual=res)
                else:
                    y = cba(x, p + 'conv1.weight', p + 'bn1', sb, d)
                    x = cba(y, p + 'conv2.weight', p + 'bn2', 1, d, residual=res)
                b += 1
        scores = F.conv2d(x, sd['seg.weight'].float(), sd['seg.bias'].float())
        return head(scores, sd['up.weight'].float()), scores


def head(scores, up_w):
    """LogSoftmax(ConvTranspose2d(C, C, 16, stride 8, padding 4, groups C)(scores)) in fp32 on the host"""
    C = scores.shape[1]
    return torch.log_softmax(F.conv_transpose2d(scores, up_w.reshape(C, 1, 16, 16), None, 8, 4, 0, C), dim=1)


def top_two(logp):
    """(arg-max uint8 [N, H, W], top-two margin fp32 [N, H, W]) of a [N, C, H, W] map"""
    v, i = torch.topk(logp, 2, dim=1)
    return i[:, 0].to(torch.uint8).numpy(), (v[:, 0] - v[:, 1]).numpy().astype(np.float32)
