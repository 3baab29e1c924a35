"""The restatements of the FID Inception-v3 network (tests/_inception_emul.py, tests/_inception_f64.py) with the reference's four
output blocks (metric/inception.py:143-163 InceptionV3(output_blocks).forward): block 0 after the stem's first max pool, 1 after
its second, 2 Mixed_6e's output, 3 the final mean.  The module tree, the blocks and the arithmetic are the two files' own (their
_Net / _Net64 classes, imported, not edited); only the forward pass is restated here, returning the four outputs.

    forward_taps(sd, x, resize)                  [b0, b1, b2, b3] fp32 (emulate=True: with the engine's bf16 roundings)
    forward_taps64(sd, x, resize)                the same in float64, on the CPU
    mean_ref(map)                                float64 [N, C] means over the pixels of an [N, C, h, w] map via math.fsum: the
                                                 correctly rounded sum, then one division"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import _inception_emul as E
from tests import _inception_f64 as E64


class _Taps:
    """the forward pass of E._Net.forward, line for line, keeping the map at the end of each output block"""

    def forward(self, x, resize):
        x = F.interpolate(x, size=(resize, resize), mode='bilinear', align_corners=False)
        x = self.rnd(2 * x - 1)
        x = self.conv('Conv2d_1a_3x3', x, stride=2)
        x = self.conv('Conv2d_2a_3x3', x)
        x = self.conv('Conv2d_2b_3x3', x, padding=1)
        b0 = x = F.max_pool2d(x, 3, 2)
        x = self.conv('Conv2d_3b_1x1', x)
        x = self.conv('Conv2d_4a_3x3', x)
        b1 = x = F.max_pool2d(x, 3, 2)
        for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
            x = self.inception_a(n + '.', x)
        x = self.inception_b('Mixed_6a.', x)
        for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
            x = self.inception_c(n + '.', x)
        b2 = x
        x = self.inception_d('Mixed_7a.', x)
        x = self.inception_e('Mixed_7b.', x, False)
        x = self.inception_e('Mixed_7c.', x, True)
        return [b0, b1, b2, x.mean((2, 3), keepdim=True)]


class _TapNet(_Taps, E._Net):
    pass


class _TapNet64(_Taps, E64._Net64):
    pass


def forward_taps(sd, x, resize=299, emulate=False, rounding=True):
    sd = {k: v.to(x.device) for k, v in sd.items() if not k.startswith('fc.')}
    with torch.no_grad():
        return _TapNet(sd, emulate, rounding).forward(x.float(), resize)


def forward_taps64(sd, x, resize=299):
    sd = {k: v.cpu() for k, v in sd.items() if not k.startswith('fc.')}
    with torch.no_grad():
        outs = _TapNet64(sd).forward(x.cpu().double(), resize)
    assert all(o.dtype == torch.float64 for o in outs)
    return outs


def mean_ref(m):
    """float64 [N, C]: fsum over the pixels of [N, C, h, w] (any float dtype; the values converted exactly), over h w"""
    a = np.asarray(m.detach().double().cpu().numpy())
    N, Cc, h, w = a.shape
    rows = a.reshape(N * Cc, h * w)
    return np.array([math.fsum(r.tolist()) / float(h * w) for r in rows], dtype=np.float64).reshape(N, Cc)


def mean_bound(m):
    """(float64 [N, C] fsum means, float64 [N, C] bound) of an [N, C, h, w] map: |any-order f64 mean rounded once to fp32 - mean|
    <= 2^-24 |mean| (the final rounding) + P 2^-52 mean|x| (any-order f64 summation of P terms, the division included)"""
    a = m.detach().double().cpu()
    P = a.shape[2] * a.shape[3]
    mean = mean_ref(m)
    return mean, 2.0 ** -24 * np.abs(mean) + P * 2.0 ** -52 * a.abs().mean((2, 3)).numpy()
