"""A/B of the SAGAN generator's eval-mode routes in one process: SaganGeneratorEngine.infer against eval forward(), alternating,
device events, ngf 48 (the bench's student) / 64 (the teacher), N 1 / 8 / 64.  Prints ms per pass and per image of each arm and
its launches; then gcc_attention_infer (each route it takes) against gcc_attention_fwd at the generator's four attention
geometries.  AB_NGF / AB_N restrict the run to one configuration, AB_ARM to one arm (infer | forward: kernel traces of one
route); AB_ATTN=0 skips the attention table."""
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcc_amd import ops  # noqa: E402
from gcc_amd.models import get_model_class  # noqa: E402
from gcc_amd.options import options  # noqa: E402
from tests.test_pix2pix_gpu import load_recipe  # noqa: E402

DEV = torch.device('cuda', 0)
PASSES = int(os.environ.get('AB_PASSES', '100'))


def timed(arms, passes=PASSES):
    for f in arms.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    tot = {k: 0.0 for k in arms}
    for _ in range(passes):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            tot[k] += e0.elapsed_time(e1)
    return {k: v / passes for k, v in tot.items()}


def count(f):
    torch.cuda.synchronize()
    ops.lib().gcc_launch_count(1)
    f()
    torch.cuda.synchronize()
    return ops.lib().gcc_launch_count(0)


def main():
    only_ngf, only_n, arm = os.environ.get('AB_NGF'), os.environ.get('AB_N'), os.environ.get('AB_ARM')
    for ngf in (48, 64):
        if only_ngf and int(only_ngf) != ngf:
            continue
        opt = options.parse(['--dataroot', './database/celeb/', '--model', 'sagan', '--gpu_ids', '0', '--ngf', str(ngf),
                             '--ndf', '8'])
        opt.isTrain = True
        model = get_model_class(opt)(opt)
        load_recipe(model.netG, 801)
        with torch.no_grad():
            model.netG.attn1.gamma.fill_(0.5)
            model.netG.attn2.gamma.fill_(-0.3)
        model.refresh_weights()
        G = model.G
        for N in (1, 8, 64):
            if only_n and int(only_n) != N:
                continue
            z = torch.randn(N, 128, device=DEV)
            zin = G.infer_input(N)
            ops.nchw_to_nhwc(z.reshape(N, 128, 1, 1).contiguous(), zin)
            c = G._ctx(N)
            ops.nchw_to_nhwc(z.reshape(N, 128, 1, 1).contiguous(), c.z)
            arms = {'infer': lambda: G.infer(zin), 'forward': lambda: G.forward(c, train=False)}
            if arm:
                arms = {arm: arms[arm]}
            t = timed(arms)
            if arm:
                print('ngf %2d N %2d: %s %.3f ms' % (ngf, N, arm, t[arm]), flush=True)
                continue
            li, lf = count(arms['infer']), count(arms['forward'])
            assert li == G.infer_launches(N)
            print('ngf %2d N %2d: infer %.3f ms (%.4f ms/image, %d launches)  forward %.3f ms (%.4f ms/image, %d launches)  '
                  'ratio %.3f' % (ngf, N, t['infer'], t['infer'] / N, li, t['forward'], t['forward'] / N, lf,
                                  t['infer'] / t['forward']), flush=True)
        G.ctx.clear()
    if os.environ.get('AB_ATTN', '1') == '0' or arm:
        return
    print('attention: gcc_attention_infer (route) vs gcc_attention_fwd, ms per call', flush=True)
    for ngf in (48, 64):
        for C, H in ((2 * ngf, 16), (ngf, 32)):
            C8 = C // 8
            c8p = ops.ceil8(C8)
            for B in (1, 8, 64):
                qkv = ops.new_act(B, 2 * c8p + C, H, H, DEV)
                qkv.copy_(torch.randn(qkv.shape, device=DEV) * 0.5)
                x, y, y2, o = (ops.new_act(B, C, H, H, DEV) for _ in range(4))
                stats = torch.zeros((B, H * H, 2), device=DEV)
                gm = torch.tensor([0.5], device=DEV)
                offs = (0, c8p, 2 * c8p)
                arms = {'fwd': lambda: ops.attention_fwd(qkv, offs, x, gm, C, C8, y, o, stats),
                        'one': lambda: ops.attention_infer(qkv, offs, x, gm, C, C8, y2, split=False)}
                split = ops.attention_infer(qkv, offs, x, gm, C, C8, y2, route_only=True) == 2
                if split:
                    arms['split'] = lambda: ops.attention_infer(qkv, offs, x, gm, C, C8, y2, split=True)
                t = timed(arms, 200)
                print('  C %3d C8 %2d %2dx%-2d B %2d: fwd %.4f  infer one-route %.4f%s' % (
                    C, C8, H, H, B, t['fwd'], t['one'], ('  infer split %.4f' % t['split']) if split else ''), flush=True)


if __name__ == '__main__':
    main()
