"""The float64 restatement of the FID Inception-v3 network: the exact-arithmetic yardstick of the fp32 engine's tests.

tests/_inception_emul.py's module tree (its blocks, its concatenations, its forward) with every BasicConv2d evaluated in float64 --
the convolution, the eval-mode BatchNorm from its four fp32 parameters (no fp32 folding), the ReLU -- and with the resize, the
pools and the final mean on float64 tensors.  The only fp32 values in it are the network's parameters and the input image.

    forward64(sd, x, resize)       [N, d, 1, 1] float64 features
    errors(want64, ref32, got)     (max |got - f64|, max |fp32 restatement - f64|): a result, and the yardstick -- E.forward's
                                   own fp32 error on this host, measured, never hard-coded"""
import torch
import torch.nn.functional as F

from tests import _inception_emul as E


class _Net64(E._Net):
    def __init__(self, sd):
        super().__init__(sd, False, False)

    def conv(self, name, x, stride=1, padding=0):
        sd = self.sd
        scale = sd[name + '.bn.weight'].double() / torch.sqrt(sd[name + '.bn.running_var'].double() + E.BN_EPS)
        shift = sd[name + '.bn.bias'].double() - sd[name + '.bn.running_mean'].double() * scale
        z = F.conv2d(x, sd[name + '.conv.weight'].double(), None, stride, padding)
        return F.relu(z * scale[None, :, None, None] + shift[None, :, None, None])


def forward64(sd, x, resize=299):
    """[N, d, 1, 1] float64 features of NCHW fp32 images in [0, 1], on the CPU"""
    sd = {k: v.cpu() for k, v in sd.items() if not k.startswith('fc.')}
    with torch.no_grad():
        out = _Net64(sd).forward(x.cpu().double(), resize)
    assert out.dtype == torch.float64
    return out


def errors(want64, ref32, got):
    """(max |got - f64|, max |fp32 restatement - f64|)"""
    return float((got.double().cpu() - want64).abs().max()), float((ref32.double().cpu() - want64).abs().max())
