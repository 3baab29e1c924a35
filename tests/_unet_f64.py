"""The eval-mode U-Net generator (models/Pix2Pix.py:40-118) restated from a netG state_dict on the host, in float64 by default:
the yardstick of the fp32 inference route (tests/test_unet_infer_fp32_*.py).  Not a test file.

A block at depth d >= 1 is [LeakyReLU(0.2, inplace), conv, BatchNorm, inner block, ReLU(inplace), ConvTranspose, BatchNorm] and
returns cat(x, model(x)).  Both activations work in place, so by the time the concat reads x it holds LeakyReLU(x), and the outer
block's ReLU then runs over both halves of the concat.  The innermost block has no BatchNorm behind its conv; a pruned generator
that lost its inner blocks ends in a block around Identity that keeps it (the up conv is then '.model.5', as in a middle block).
The outermost block is conv | inner | ReLU, ConvTranspose (+ bias), tanh."""
import torch
import torch.nn.functional as F

EPS = 1e-5


def _prefix(d):
    return 'model' if d == 0 else 'model.model.1' + '.model.3' * (d - 1)


def depth(sd):
    """number of blocks of the generator that owns the state_dict"""
    D = 1
    while _prefix(D) + '.model.1.weight' in sd:
        D += 1
    return D


def unet_eval(sd, x, dtype=torch.float64, pre_tanh=False):
    """the generator's eval-mode image of x [N, 3, H, W] (or the last conv's output before tanh) with every parameter, buffer
    and activation in `dtype`, on the host"""
    sd = {k: v.detach().to('cpu', dtype) for k, v in sd.items() if v.is_floating_point()}
    D = depth(sd)

    def bn(t, name):
        return F.batch_norm(t, sd[name + '.running_mean'], sd[name + '.running_var'], sd[name + '.weight'], sd[name + '.bias'],
                            False, 0.0, EPS)

    def block(d, t):
        p = _prefix(d)
        lx = F.leaky_relu(t, 0.2)
        h = F.conv2d(lx, sd[p + '.model.1.weight'], sd.get(p + '.model.1.bias'), 2, 1)
        last = d == D - 1
        around_identity = last and (p + '.model.5.weight') in sd
        if not last or around_identity:
            h = bn(h, p + '.model.2')
        if not last:
            h = block(d + 1, h)
        up, norm = ('.model.3', '.model.4') if last and not around_identity else ('.model.5', '.model.6')
        u = F.conv_transpose2d(F.relu(h), sd[p + up + '.weight'], sd.get(p + up + '.bias'), 2, 1)
        return torch.cat([lx, bn(u, p + norm)], 1)

    t = x.detach().to('cpu', dtype)
    e = F.conv2d(t, sd['model.model.0.weight'], sd.get('model.model.0.bias'), 2, 1)
    z = F.conv_transpose2d(F.relu(block(1, e)), sd['model.model.3.weight'], sd.get('model.model.3.bias'), 2, 1)
    return z if pre_tanh else torch.tanh(z)


def tensor2im(image):
    """the bytes of the reference's util.tensor2im of an NCHW image batch, evaluated in the image's own dtype: uint8 [N, H, W, 3]"""
    a = (image.permute(0, 2, 3, 1) + 1) / 2.0 * 255.0
    return a.clamp(0, 255).to(torch.uint8)
