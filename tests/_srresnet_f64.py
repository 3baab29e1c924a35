"""SRResNet's eval-mode forward (models/SRGAN.py:139-199) restated from a generator state_dict, in float64 by default: the yardstick
of the fp32 inference route.  k9 conv + PReLU | n x [conv3 BN PReLU conv3 BN, + x] | conv3 BN + long skip | 2 x [conv3 ->
PixelShuffle(2) -> PReLU] | k9 conv + tanh; BatchNorm from the running statistics with eps 1e-5, one scalar slope per PReLU.
`dtype` / `device` run the same text in fp32 on a device (the test's error unit); `round_bf16` rounds the weights and every
layer's output to bf16 (what the bf16 route does, for the seeded nets' recipe)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = 1e-5


def load_fixture():
    """(generator state_dict, lr [2, 3, 12, 12], the reference's fake_hr [2, 3, 48, 48]) of the reference-written checkpoint"""
    sd = torch.load(os.path.join(GOLDEN_DIR, 'ref_checkpoint_srgan.pth'), map_location='cpu', weights_only=False)['G']
    z = np.load(os.path.join(GOLDEN_DIR, 'ref_checkpoint_srgan.npz'))
    return sd, torch.from_numpy(z['lr']), torch.from_numpy(z['fake_hr'])


def forward(sd, lr, dtype=torch.float64, device='cpu', round_bf16=False, pre_tanh=False):
    p = {k: v.detach().to(device=device, dtype=dtype) for k, v in sd.items() if v.is_floating_point()}
    rb = (lambda t: t.bfloat16().to(dtype)) if round_bf16 else (lambda t: t)

    def conv(x, key, k):
        return F.conv2d(x, rb(p[key + '.weight']), p.get(key + '.bias'), 1, k // 2)

    def bn(x, key):
        scale = p[key + '.weight'] / torch.sqrt(p[key + '.running_var'] + EPS)
        return x * scale.view(1, -1, 1, 1) + (p[key + '.bias'] - p[key + '.running_mean'] * scale).view(1, -1, 1, 1)

    def prelu(x, key):
        return torch.where(x >= 0, x, p[key + '.weight'].reshape(()) * x)

    x = rb(lr.to(device=device, dtype=dtype))
    h0 = rb(prelu(conv(x, 'conv_block1.conv_block.0', 9), 'conv_block1.conv_block.1'))
    h, i = h0, 0
    while 'residual_blocks.%d.conv_block1.conv_block.0.weight' % i in p:
        b = 'residual_blocks.%d.' % i
        a = rb(prelu(bn(conv(h, b + 'conv_block1.conv_block.0', 3), b + 'conv_block1.conv_block.1'), b + 'conv_block1.conv_block.2'))
        h = rb(bn(conv(a, b + 'conv_block2.conv_block.0', 3), b + 'conv_block2.conv_block.1') + h)
        i += 1
    h = rb(bn(conv(h, 'conv_block2.conv_block.0', 3), 'conv_block2.conv_block.1') + h0)
    j = 0
    while 'subpixel_convolutional_blocks.%d.conv.weight' % j in p:
        s = 'subpixel_convolutional_blocks.%d.' % j
        h = rb(prelu(F.pixel_shuffle(conv(h, s + 'conv', 3), 2), s + 'prelu'))
        j += 1
    z = conv(h, 'conv_block3.conv_block.0', 9)
    return z if pre_tanh else rb(torch.tanh(z))


def fill_range(sd, lr, seed):
    """a copy of the generator state_dict `sd` (BatchNorms and slopes as they are) whose image on `lr` fills [-1, 1] without
    saturating tanh: He-normal conv weights; the last BatchNorm of every residual branch (each block's second, conv_block2's)
    with weight and bias times 0.2, so the trunk's variance does not grow through the 17 sums; the image conv's bias 0 and
    its weights scaled so that the float64 pre-tanh standard deviation on `lr` is 0.5"""
    g = torch.Generator().manual_seed(seed)
    out = {k: v.detach().cpu().clone() for k, v in sd.items()}
    for k, v in out.items():
        if v.dim() == 4:
            out[k] = (torch.randn(v.shape, generator=g) * (2.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5).to(v.dtype)
        if k.endswith('conv_block2.conv_block.1.weight') or k.endswith('conv_block2.conv_block.1.bias'):
            out[k] = v * 0.2
    out['conv_block3.conv_block.0.bias'] = torch.zeros_like(out['conv_block3.conv_block.0.bias'])
    with torch.no_grad():
        std = float(forward(out, lr, pre_tanh=True).std())
    out['conv_block3.conv_block.0.weight'] = (out['conv_block3.conv_block.0.weight'].double() * (0.5 / std)).float()
    return out


def fills_range(image):
    """the condition of the seeded nets, on the float64 image: at most 1 % of the values above 0.99 in magnitude and a standard
    deviation of at least 0.2"""
    return float((image.abs() > 0.99).double().mean()) <= 0.01 and float(image.std()) >= 0.2
