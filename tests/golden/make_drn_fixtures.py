#!/usr/bin/env python3
"""Generate tests/golden/drn_seg.npz by IMPORTING THE REAL REFERENCE (metric/drn.py and metric/mIoU_score.py's DRNSeg,
unmodified) through make_fixtures.import_reference().  Runs only in the authoring container; never imported by the tests.
Nothing of the reference is copied: the file holds data (names, shapes, seeds and results).

    python tests/golden/make_drn_fixtures.py

Three small arch-D nets (tests/_drn_emul.NETS).  Their weights are NOT stored: tests/_drn_emul.drn_state_dict rebuilds them
from the stored key table and seed (221 k parameters would be 0.9 MB of incompressible floats), and this script loads exactly
those values INTO the reference's DRNSeg (strict) before running it, after checking that the key / shape table generated from
the architecture's constants is the reference model's own.  The input is seeded the same way.  Per net <name>:
  .keys / .shapes      the reference state_dict's keys and shapes (-1 padded to four dimensions), in its order
  .seed / .damp / .input_seed / .input_shape
  .scores              fp32 [N][19][H/8][W/8]: DRNSeg.forward's second result (fp32, CPU)
  .argmax / .margin    uint8 / fp32 [N][H][W]: arg-max over the classes of DRNSeg.forward's first result (the log-softmax at
                       the input's size, 0.2 - 0.9 MB per net if stored whole) and its top-two margin
  .logp_sample         fp32 [2048]: that log-softmax at tests/golden/recipe.sample_idx positions of the flattened tensor
  .emul_err            max |emul - ref| over the scores, emul = tests/_drn_emul.forward(emulate=True): bf16 weights, one bf16
                       rounding per conv + BatchNorm (+ ReLU) and per residual sum, fp32 head
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import make_fixtures as F
    from recipe import sample_idx
    from tests import _drn_emul as E
    F.import_reference()
    sys.modules['cv2'].imread = None
    base = type('InceptionBlock', (torch.nn.Module,), {})
    sys.modules['torchvision.models'].inception = F._stub('torchvision.models.inception', InceptionA=base, InceptionC=base,
                                                          InceptionE=base)
    sys.modules['torchvision'].models = sys.modules['torchvision.models']
    from metric import drn as RD
    from metric import mIoU_score as R

    out = {}
    for name, (kind, layers, channels, in_shape, seed, damp) in E.NETS.items():
        block = RD.Bottleneck if kind == 'bottleneck' else RD.BasicBlock
        RD.__dict__['fixture_net'] = lambda pretrained=False, num_classes=1000: RD.DRN(
            block, layers, num_classes=num_classes, channels=channels, arch='D')
        net = R.DRNSeg('fixture_net', 19, pretrained=False).eval()
        ref_sd = net.state_dict()
        shapes = E.drn_shapes(kind, layers, channels)
        assert list(shapes) == list(ref_sd), (name, [k for k in ref_sd if k not in shapes], [k for k in shapes if k not in ref_sd])
        assert all(tuple(ref_sd[k].shape) == tuple(s) for k, s in shapes.items()), name
        sd = E.drn_state_dict(shapes, seed, damp)
        net.load_state_dict(sd, strict=True)
        x = E.seeded_input(in_shape, seed + 1)
        with torch.no_grad():
            logp, scores = net(x)
        assert torch.isfinite(logp).all() and float(scores.abs().max()) <= 50.0, (name, float(scores.abs().max()))
        # the restatement in fp32 is the reference up to summation order; in bf16 it is the device path's formats
        lp32, s32 = E.forward(sd, x, emulate=False)
        span = float(scores.max() - scores.min())
        assert float((s32 - scores).abs().max()) <= 1e-4 * span and float((lp32 - logp).abs().max()) <= 1e-4 * span, name
        _, se = E.forward(sd, x, emulate=True)
        emul_err = float((se - scores).abs().max())
        am, margin = E.top_two(logp)
        nparam = sum(v.numel() for k, v in sd.items() if not k.endswith('num_batches_tracked'))
        print('%-9s %6d parameters, scores in [%.2f, %.2f], emul_err %.4f = %.2f %% of the range, %.1f %% of pixels with a '
              'margin above 4 emul_err' % (name, nparam, float(scores.min()), float(scores.max()), emul_err,
                                           100 * emul_err / span, 100 * float((margin > 4 * emul_err).mean())))
        shp = -np.ones((len(shapes), 4), dtype=np.int64)
        for i, s in enumerate(shapes.values()):
            shp[i, :len(s)] = s
        out.update({name + '.keys': np.array(list(shapes)), name + '.shapes': shp, name + '.seed': np.int64(seed),
                    name + '.damp': np.float64(damp), name + '.input_seed': np.int64(seed + 1),
                    name + '.input_shape': np.array(in_shape, dtype=np.int64), name + '.scores': scores.numpy(),
                    name + '.argmax': am, name + '.margin': margin,
                    name + '.logp_sample': logp.reshape(-1)[sample_idx(logp.numel())].numpy(),
                    name + '.emul_err': np.float64(emul_err)})
    path = os.path.join(HERE, 'drn_seg.npz')
    np.savez_compressed(path, **out)
    print('drn_seg ok: %d bytes' % os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    torch.set_num_threads(8)
    main()
