"""A/B of the two routes from a segmenter's score maps to the Cityscapes confusion matrix, one process, the arms alternating on
the same seeded [1, 19, 256, 256] score maps and 1024 x 2048 labels, device events around blocks of 20 images, AB_PASSES images per
arm after warm-up, the whole measurement repeated once to show the spread:
  A  the route of mIoU_score.test(dataset=...): torch interpolate -> gcc_argmax_channels -> gcc_confusion_hist
  B  gcc_amd.metric.cityscapes.score (gcc_miou_score: resize + argmax + histogram in one launch, PIL's arithmetic)
Prints ms per image, library launches per image (gcc_launch_count; arm A's interpolate and casts are PyTorch launches on top),
the bytes each arm must move (from shapes) and B's time against the bounds that could apply.  AB_ARM=A|B runs one arm alone
(kernel traces)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcc_amd import ops  # noqa: E402
from gcc_amd.metric import cityscapes as CS  # noqa: E402
from gcc_amd.metric import mIoU_score as G  # noqa: E402

DEV = torch.device('cuda', 0)
PASSES = int(os.environ.get('AB_PASSES', '300'))
C, h, w, H, W = 19, 256, 256, 1024, 2048
HBM_GBS, F64_TFLOPS = 8000.0, 78.6          # datasheet peaks: HBM3E bandwidth, f64 vector rate


BLOCK = 20         # images issued back to back between two events: the queue hides the host's launch path when the GPU is slower


def timed(arms, passes):
    for f in arms.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    tot = {k: 0.0 for k in arms}
    for _ in range(passes // BLOCK):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BLOCK):
                f()
            e1.record()
            e1.synchronize()
            tot[k] += e0.elapsed_time(e1)
    return {k: v / (passes // BLOCK * BLOCK) for k, v in tot.items()}


def count(f):
    torch.cuda.synchronize()
    ops.lib().gcc_launch_count(1)
    f()
    torch.cuda.synchronize()
    return ops.lib().gcc_launch_count(0)


def main():
    rs = np.random.RandomState(8)
    scores = torch.from_numpy((rs.randint(-2 ** 20, 2 ** 20, (1, C, h, w)) / 2 ** 16).astype(np.float32)).to(DEV)
    lab = rs.randint(0, C + 1, (1, H, W)).astype(np.uint8)
    lab[lab == C] = 255
    label_u8 = torch.from_numpy(lab).to(DEV)
    label_i64 = label_u8.to(torch.int64)                      # what a dataset= caller hands arm A
    hist_a = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    hist_b = torch.zeros((C, C), dtype=torch.int64, device=DEV)

    def arm_a():
        final = torch.nn.functional.interpolate(scores, size=(H, W), mode='bilinear', align_corners=False)
        G.fast_hist(G.argmax_classes(final), label_i64, C, hist_a)

    def arm_b():
        CS.score(scores, label_u8, hist=hist_b)

    arms = {'A': arm_a, 'B': arm_b}
    only = os.environ.get('AB_ARM')
    if only:
        arms = {only: arms[only]}
    for rep in range(1 if only else 2):
        t = timed(arms, PASSES)
        print('repetition %d: ' % rep + '  '.join('%s %.4f ms/image' % kv for kv in t.items()) +
              ('  B / A %.3f' % (t['B'] / t['A']) if len(t) == 2 else ''), flush=True)
    if only:
        return
    print('library launches per image: A %d (+ interpolate, the int32 casts of pred / label: PyTorch launches)  B %d' %
          (count(arm_a), count(arm_b)))
    px = H * W
    a_bytes = C * h * w * 4 + 2 * C * px * 4 + px * 4 + px * 8 + 2 * px * 4 + px * 4
    b_bytes = C * h * w * 4 + px
    print('bytes per image from shapes: A %.1f MB (scores in, resized tensor out and in again, int32 class map out and in, int64 '
          'labels in, their int32 copy out and in)  B %.1f MB (scores in, uint8 labels in)' % (a_bytes / 1e6, b_bytes / 1e6))
    flops = C * (px * 2 * 2 + (px // 8) * 10 * 2 * 2)          # vertical taps per pixel; horizontal per source row of a tile
    print('B against its bounds: HBM %.4f ms at %.0f GB/s, f64 vector %.4f ms for %.2e operations at %.1f TFLOP/s; measured %.4f ms'
          % (b_bytes / HBM_GBS / 1e6, HBM_GBS, flops / F64_TFLOPS / 1e9, flops, F64_TFLOPS, t['B']))
    differ = int((hist_a != hist_b).sum().item())
    print('histogram cells in which the arms differ after the run: %d of %d (A resizes with torch\'s fp32 arithmetic, B with PIL\'s)'
          % (differ, C * C))


if __name__ == '__main__':
    main()
