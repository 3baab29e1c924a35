"""The eval-mode MobileResnet generator (models/Pix2Pix.py:132-265, models/CycleGAN.py:77-138) restated from a netG state_dict on
the host, in float64 by default: the yardstick of the fp32 inference route (tests/test_resnet_infer_fp32_*.py).  Not a test file.

ReflectionPad2d(3), conv7 | 2 x conv3 s2 p1 | residual blocks x + IN(pw(IN(dw(pad1(relu(IN(pw(IN(dw(pad1(x))))))))))) | 2 x
ConvTranspose2d(3, 2, 1, output_padding 1) | ReflectionPad2d(3), conv7, tanh, with InstanceNorm2d(affine=False, eps 1e-5) + ReLU
behind the three stem convs and the two transposed ones.  Dropout has rate 0.  The blocks present (a pruned generator may have lost
some) and every width are read from the keys."""
import re

import torch
import torch.nn.functional as F

EPS = 1e-5


def layout(sd):
    """(indices of the six plain convs, indices of the residual blocks) under 'model.'"""
    convs = sorted(int(m.group(1)) for m in (re.fullmatch(r'model\.(\d+)\.weight', k) for k in sd) if m)
    blocks = sorted(int(m.group(1)) for m in (re.fullmatch(r'model\.(\d+)\.conv_block\.1\.conv\.0\.weight', k) for k in sd) if m)
    assert len(convs) == 6, convs
    return convs, blocks


def resnet_eval(sd, x, dtype=torch.float64, pre_tanh=False):
    """the generator's eval-mode image of x [N, 3, H, W] (or the last conv's output before tanh) with every parameter and
    activation in `dtype`, on the host"""
    sd = {k: v.detach().to('cpu', dtype) for k, v in sd.items() if v.is_floating_point()}
    convs, blocks = layout(sd)
    wb = lambda name: (sd[name + '.weight'], sd.get(name + '.bias'))
    norm = lambda t: F.instance_norm(t, eps=EPS)

    def separable(t, name):
        w, b = wb(name + '.conv.0')
        t = norm(F.conv2d(F.pad(t, (1, 1, 1, 1), mode='reflect'), w, b, groups=t.shape[1]))
        return F.conv2d(t, *wb(name + '.conv.2'))

    h = x.detach().to('cpu', dtype)
    h = F.relu(norm(F.conv2d(F.pad(h, (3, 3, 3, 3), mode='reflect'), *wb('model.%d' % convs[0]))))
    for i in convs[1:3]:
        h = F.relu(norm(F.conv2d(h, *wb('model.%d' % i), stride=2, padding=1)))
    for i in blocks:
        t = F.relu(norm(separable(h, 'model.%d.conv_block.1' % i)))
        h = h + norm(separable(t, 'model.%d.conv_block.6' % i))
    for i in convs[3:5]:
        h = F.relu(norm(F.conv_transpose2d(h, *wb('model.%d' % i), 2, 1, 1)))
    z = F.conv2d(F.pad(h, (3, 3, 3, 3), mode='reflect'), *wb('model.%d' % convs[5]))
    return z if pre_tanh else torch.tanh(z)


def tensor2im(image):
    """the bytes of the reference's util.tensor2im of an NCHW image batch, evaluated in the image's own dtype: uint8 [N, H, W, 3]"""
    a = (image.permute(0, 2, 3, 1) + 1) / 2.0 * 255.0
    return a.clamp(0, 255).to(torch.uint8)
