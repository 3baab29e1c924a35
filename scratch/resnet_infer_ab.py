"""A/B of the MobileResnet generator's eval-mode routes in one process: MobileResnetEngine.infer (dw_inorm fused blocks)
against eval forward(), alternating, device events, 256x256, ngf 24 / 64, N 1 / 8.  Prints ms per pass of each arm.
AB_NGF / AB_N restrict the run to one configuration, AB_ARM to one arm (infer | forward: kernel traces of one route)."""
import sys
import os
from collections import OrderedDict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcc_amd import engine, ops  # noqa: E402
from gcc_amd.models.Pix2Pix import MobileResnetGenerator  # noqa: E402
from tests.golden.recipe import recipe_state_dict  # noqa: E402

DEV = torch.device('cuda', 0)
PASSES = int(os.environ.get('AB_PASSES', '200'))


def main():
    only_ngf, only_n, arm = os.environ.get('AB_NGF'), os.environ.get('AB_N'), os.environ.get('AB_ARM')
    for ngf in (24, 64):
        if only_ngf and int(only_ngf) != ngf:
            continue
        net = MobileResnetGenerator(ngf=ngf, n_blocks=9).to(DEV)
        shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
        net.load_state_dict({k: v.to(DEV) for k, v in recipe_state_dict(shapes, 5).items()})
        engine.FlatParams(list(net.parameters()), DEV)
        eng = engine.MobileResnetEngine(net, DEV)
        eng.repack()
        for N in (1, 8):
            if only_n and int(only_n) != N:
                continue
            x = torch.rand(N, 3, 256, 256, device=DEV) * 2 - 1
            xin = eng.infer_input(N, 256, 256)
            ops.nchw_to_nhwc(x, xin, cfill=8)
            c = eng._ctx(N, 256, 256, 'main')
            ops.nchw_to_nhwc(x, c.x_in, cfill=8)
            arms = {'infer': lambda: eng.infer(xin), 'forward': lambda: eng.forward(c, train=False)}
            if arm:
                arms = {arm: arms[arm]}
            for f in arms.values():
                for _ in range(10):
                    f()
            torch.cuda.synchronize()
            tot = {k: 0.0 for k in arms}
            for _ in range(PASSES):
                for k, f in arms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    e1.synchronize()
                    tot[k] += e0.elapsed_time(e1)
            ops.lib().gcc_launch_count(1)
            eng.infer(xin)
            li = ops.lib().gcc_launch_count(1)
            eng.forward(c, train=False)
            lf = ops.lib().gcc_launch_count(0)
            if arm:
                print('ngf %2d N %d: %s %.3f ms' % (ngf, N, arm, tot[arm] / PASSES), flush=True)
                continue
            print('ngf %2d N %d: infer %.3f ms (%d launches)  forward %.3f ms (%d launches)  ratio %.3f' % (
                ngf, N, tot['infer'] / PASSES, li, tot['forward'] / PASSES, lf, tot['infer'] / tot['forward']), flush=True)
        eng.ctx.clear()


if __name__ == '__main__':
    main()
