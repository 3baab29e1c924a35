"""Plain-torch restatement of the FID Inception-v3 network, the fp32 truth of the InceptionFidEngine tests.

It restates the module tree from the issue that asked for the native engine and from the reference's metric/inception.py
(fid_inception_v3: torchvision's Inception3(num_classes=1008, aux_logits=False) with the FID patches, under InceptionV3([3])) --
NOT from a run of the reference: torchvision is not available to the tests, so the reference's own module cannot be executed.
Written as torchvision writes its forward passes (one function per block kind, torch.cat of the branches), on purpose unlike the
engine's table of branches.

    forward(sd, x, resize)                     fp32: conv, eval-mode BatchNorm (eps 1e-3) folded to scale / shift, ReLU
    forward(sd, x, resize, emulate=True)       the same arithmetic with a bf16 rounding wherever the engine rounds: the resized
                                               input, the packed weights, every conv + BatchNorm + ReLU output, every average pool
    forward(..., emulate=True, rounding=False) the emulating code path with the roundings switched off: fp32 bit for bit
    seeded(widths_div, seed)                   a state_dict with the reference's key names at 1 / widths_div of its widths"""
import math

import torch
import torch.nn.functional as F

BN_EPS = 1e-3


def _w(full, div):
    """a width of the real network divided by div, rounded up to a multiple of 8"""
    return max(8, (full // div + 7) // 8 * 8)


def conv_table(div=1):
    """[(BasicConv2d name, cin, cout, (kh, kw))] of the whole network in module order, widths / div"""
    w = lambda v: _w(v, div)
    t = [('Conv2d_1a_3x3', 3, w(32), (3, 3)), ('Conv2d_2a_3x3', w(32), w(32), (3, 3)), ('Conv2d_2b_3x3', w(32), w(64), (3, 3)),
         ('Conv2d_3b_1x1', w(64), w(80), (1, 1)), ('Conv2d_4a_3x3', w(80), w(192), (3, 3))]
    cin = w(192)
    for name, pf in (('Mixed_5b', 32), ('Mixed_5c', 64), ('Mixed_5d', 64)):
        p = name + '.'
        t += [(p + 'branch1x1', cin, w(64), (1, 1)), (p + 'branch5x5_1', cin, w(48), (1, 1)), (p + 'branch5x5_2', w(48), w(64), (5, 5)),
              (p + 'branch3x3dbl_1', cin, w(64), (1, 1)), (p + 'branch3x3dbl_2', w(64), w(96), (3, 3)),
              (p + 'branch3x3dbl_3', w(96), w(96), (3, 3)), (p + 'branch_pool', cin, w(pf), (1, 1))]
        cin = w(64) + w(64) + w(96) + w(pf)
    p = 'Mixed_6a.'
    t += [(p + 'branch3x3', cin, w(384), (3, 3)), (p + 'branch3x3dbl_1', cin, w(64), (1, 1)),
          (p + 'branch3x3dbl_2', w(64), w(96), (3, 3)), (p + 'branch3x3dbl_3', w(96), w(96), (3, 3))]
    cin = w(384) + w(96) + cin
    for name, c7 in (('Mixed_6b', 128), ('Mixed_6c', 160), ('Mixed_6d', 160), ('Mixed_6e', 192)):
        p, c = name + '.', w(c7)
        t += [(p + 'branch1x1', cin, w(192), (1, 1)),
              (p + 'branch7x7_1', cin, c, (1, 1)), (p + 'branch7x7_2', c, c, (1, 7)), (p + 'branch7x7_3', c, w(192), (7, 1)),
              (p + 'branch7x7dbl_1', cin, c, (1, 1)), (p + 'branch7x7dbl_2', c, c, (7, 1)), (p + 'branch7x7dbl_3', c, c, (1, 7)),
              (p + 'branch7x7dbl_4', c, c, (7, 1)), (p + 'branch7x7dbl_5', c, w(192), (1, 7)), (p + 'branch_pool', cin, w(192), (1, 1))]
        cin = 4 * w(192)
    p = 'Mixed_7a.'
    t += [(p + 'branch3x3_1', cin, w(192), (1, 1)), (p + 'branch3x3_2', w(192), w(320), (3, 3)),
          (p + 'branch7x7x3_1', cin, w(192), (1, 1)), (p + 'branch7x7x3_2', w(192), w(192), (1, 7)),
          (p + 'branch7x7x3_3', w(192), w(192), (7, 1)), (p + 'branch7x7x3_4', w(192), w(192), (3, 3))]
    cin = w(320) + w(192) + cin
    for name in ('Mixed_7b', 'Mixed_7c'):
        p = name + '.'
        t += [(p + 'branch1x1', cin, w(320), (1, 1)), (p + 'branch3x3_1', cin, w(384), (1, 1)),
              (p + 'branch3x3_2a', w(384), w(384), (1, 3)), (p + 'branch3x3_2b', w(384), w(384), (3, 1)),
              (p + 'branch3x3dbl_1', cin, w(448), (1, 1)), (p + 'branch3x3dbl_2', w(448), w(384), (3, 3)),
              (p + 'branch3x3dbl_3a', w(384), w(384), (1, 3)), (p + 'branch3x3dbl_3b', w(384), w(384), (3, 1)),
              (p + 'branch_pool', cin, w(192), (1, 1))]
        cin = w(320) + 4 * w(384) + w(192)
    return t


def feature_width(div=1):
    return _w(320, div) + 4 * _w(384, div) + _w(192, div)


def shapes(div=1):
    """{key: shape} of the state_dict (fc.* and num_batches_tracked included)"""
    out = {}
    for name, cin, cout, (kh, kw) in conv_table(div):
        out[name + '.conv.weight'] = (cout, cin, kh, kw)
        for f in ('weight', 'bias', 'running_mean', 'running_var'):
            out['%s.bn.%s' % (name, f)] = (cout,)
        out[name + '.bn.num_batches_tracked'] = ()
    out['fc.weight'] = (1008, feature_width(div))
    out['fc.bias'] = (1008,)
    return out


def seeded(widths_div=1, seed=0):
    """a state_dict with the reference's key names: He-scaled conv weights, gamma in [0.5, 1.5], small beta and running means,
    running variances in [0.5, 1.5]; fc.* and num_batches_tracked present (and unused)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, s in shapes(widths_div).items():
        if key.endswith('num_batches_tracked'):
            sd[key] = torch.tensor(1000, dtype=torch.int64)
        elif key.endswith('conv.weight'):
            sd[key] = torch.randn(s, generator=g) * math.sqrt(2.0 / (s[1] * s[2] * s[3]))
        elif key.endswith('bn.weight') or key.endswith('running_var'):
            sd[key] = 0.5 + torch.rand(s, generator=g)
        elif key.startswith('fc.'):
            sd[key] = torch.randn(s, generator=g) * 0.01
        else:
            sd[key] = torch.randn(s, generator=g) * 0.1
    return sd


def seeded_input(shape, seed):
    """images in [0, 1] with structure at several scales (a resize of white noise alone would be nearly flat)"""
    g = torch.Generator().manual_seed(seed)
    N, Cc, H, W = shape
    coarse = F.interpolate(torch.rand((N, Cc, max(2, H // 8), max(2, W // 8)), generator=g), (H, W), mode='bilinear', align_corners=False)
    return (0.7 * coarse + 0.3 * torch.rand(shape, generator=g)).clamp(0, 1).contiguous()


class _Net:
    def __init__(self, sd, emulate, rounding):
        self.sd = sd
        on = emulate and rounding
        self.rnd = (lambda t: t.bfloat16().float()) if on else (lambda t: t)

    def conv(self, name, x, stride=1, padding=0):
        """BasicConv2d: bias-free conv, eval-mode BatchNorm as fp32 scale / shift, ReLU; one rounding"""
        sd = self.sd
        scale = sd[name + '.bn.weight'].float() / torch.sqrt(sd[name + '.bn.running_var'].float() + BN_EPS)
        shift = sd[name + '.bn.bias'].float() - sd[name + '.bn.running_mean'].float() * scale
        z = F.conv2d(x, self.rnd(sd[name + '.conv.weight'].float()), None, stride, padding)
        return self.rnd(F.relu(z * scale[None, :, None, None] + shift[None, :, None, None]))

    def avg(self, x):
        return self.rnd(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False))

    def inception_a(self, p, x):
        b1 = self.conv(p + 'branch1x1', x)
        b5 = self.conv(p + 'branch5x5_2', self.conv(p + 'branch5x5_1', x), padding=2)
        b3 = self.conv(p + 'branch3x3dbl_1', x)
        b3 = self.conv(p + 'branch3x3dbl_2', b3, padding=1)
        b3 = self.conv(p + 'branch3x3dbl_3', b3, padding=1)
        bp = self.conv(p + 'branch_pool', self.avg(x))
        return torch.cat([b1, b5, b3, bp], 1)

    def inception_b(self, p, x):
        b3 = self.conv(p + 'branch3x3', x, stride=2)
        bd = self.conv(p + 'branch3x3dbl_1', x)
        bd = self.conv(p + 'branch3x3dbl_2', bd, padding=1)
        bd = self.conv(p + 'branch3x3dbl_3', bd, stride=2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)

    def inception_c(self, p, x):
        b1 = self.conv(p + 'branch1x1', x)
        b7 = self.conv(p + 'branch7x7_1', x)
        b7 = self.conv(p + 'branch7x7_2', b7, padding=(0, 3))
        b7 = self.conv(p + 'branch7x7_3', b7, padding=(3, 0))
        bd = self.conv(p + 'branch7x7dbl_1', x)
        bd = self.conv(p + 'branch7x7dbl_2', bd, padding=(3, 0))
        bd = self.conv(p + 'branch7x7dbl_3', bd, padding=(0, 3))
        bd = self.conv(p + 'branch7x7dbl_4', bd, padding=(3, 0))
        bd = self.conv(p + 'branch7x7dbl_5', bd, padding=(0, 3))
        bp = self.conv(p + 'branch_pool', self.avg(x))
        return torch.cat([b1, b7, bd, bp], 1)

    def inception_d(self, p, x):
        b3 = self.conv(p + 'branch3x3_2', self.conv(p + 'branch3x3_1', x), stride=2)
        b7 = self.conv(p + 'branch7x7x3_1', x)
        b7 = self.conv(p + 'branch7x7x3_2', b7, padding=(0, 3))
        b7 = self.conv(p + 'branch7x7x3_3', b7, padding=(3, 0))
        b7 = self.conv(p + 'branch7x7x3_4', b7, stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)

    def inception_e(self, p, x, max_pool):
        b1 = self.conv(p + 'branch1x1', x)
        b3 = self.conv(p + 'branch3x3_1', x)
        b3 = torch.cat([self.conv(p + 'branch3x3_2a', b3, padding=(0, 1)), self.conv(p + 'branch3x3_2b', b3, padding=(1, 0))], 1)
        bd = self.conv(p + 'branch3x3dbl_2', self.conv(p + 'branch3x3dbl_1', x), padding=1)
        bd = torch.cat([self.conv(p + 'branch3x3dbl_3a', bd, padding=(0, 1)), self.conv(p + 'branch3x3dbl_3b', bd, padding=(1, 0))], 1)
        pooled = F.max_pool2d(x, 3, 1, 1) if max_pool else self.avg(x)         # Mixed_7c: the FID network's max pool
        return torch.cat([b1, b3, bd, self.conv(p + 'branch_pool', pooled)], 1)

    def forward(self, x, resize):
        x = F.interpolate(x, size=(resize, resize), mode='bilinear', align_corners=False)
        x = self.rnd(2 * x - 1)
        x = self.conv('Conv2d_1a_3x3', x, stride=2)
        x = self.conv('Conv2d_2a_3x3', x)
        x = self.conv('Conv2d_2b_3x3', x, padding=1)
        x = F.max_pool2d(x, 3, 2)
        x = self.conv('Conv2d_3b_1x1', x)
        x = self.conv('Conv2d_4a_3x3', x)
        x = F.max_pool2d(x, 3, 2)
        for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
            x = self.inception_a(n + '.', x)
        x = self.inception_b('Mixed_6a.', x)
        for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
            x = self.inception_c(n + '.', x)
        x = self.inception_d('Mixed_7a.', x)
        x = self.inception_e('Mixed_7b.', x, False)
        x = self.inception_e('Mixed_7c.', x, True)
        return x.mean((2, 3), keepdim=True)


def forward(sd, x, resize=299, emulate=False, rounding=True):
    """[N, d, 1, 1] fp32 features of NCHW fp32 images in [0, 1] (on x's device; sd's tensors are moved there)"""
    sd = {k: v.to(x.device) for k, v in sd.items() if not k.startswith('fc.')}
    with torch.no_grad():
        return _Net(sd, emulate, rounding).forward(x.float(), resize)
