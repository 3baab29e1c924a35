"""SRGAN evaluation (metric/test_metric.py:89-127 test_srgan_psnr, train.py:37-56): PSNR / SSIM of the generator on a test set,
one whole benchmark image at a time, through the generator's inference path (engine.SRResNetEngine.infer: eval-mode BatchNorm
folded into the conv epilogues, one grow-only slab for every image size).  The module is not named test_*.py: a bare pytest
would collect it."""
import copy
import math
import os

import torch

from .. import ops
from .._lib import GccError, check

SR_TEST_SETS = ('Set5', 'Set14', 'B100', 'Urban100')      # train.py:37, in the reference's slot order
PRECISION_ENV = 'GCC_SR_PRECISION'
PRECISIONS = ('bf16', 'fp32')


def sr_precision():
    """the precision of the generator's inference path in every SRGAN evaluation and in gcc_amd.test --model srgan: the
    environment variable GCC_SR_PRECISION, 'bf16' (the default) or 'fp32' (the reference's own arithmetic on the f32-input
    matrix instructions: SRResNetEngine.infer(x, 'fp32')); any other value raises GccError.  The one place that reads it."""
    precision = os.environ.get(PRECISION_ENV) or 'bf16'
    if precision not in PRECISIONS:
        raise GccError('%s=%s: expected one of %s' % (PRECISION_ENV, precision, ', '.join(PRECISIONS)))
    return precision


def infer_image(G, lr, precision):
    """the generator's image (an NHWC view of its slab: bf16, or fp32 with precision 'fp32') of an NCHW fp32 LR batch on the
    device; eval_coeffs(precision) of the current parameters must have run"""
    N, _, h, w = lr.shape
    if precision == 'fp32':
        return G.infer(ops.nchw_to_nhwc_f32(lr, G.infer_input(N, h, w, 'fp32')), 'fp32')
    return G.infer(ops.nchw_to_nhwc(lr, G.infer_input(N, h, w), cfill=8))


class _Scratch:
    """grow-only fp32 buffers of the evaluator (the NCHW image the metric kernels read, their workspace)"""

    def __init__(self, device):
        self.device, self.img, self.ws = device, None, None

    def image(self, n):
        if self.img is None or self.img.numel() < n:
            self.img = None
            self.img = torch.empty(n, dtype=torch.float32, device=self.device)
        return self.img[:n]

    def workspace(self):
        if self.ws is None:
            self.ws = torch.empty(ops.lib().gcc_psnr_workspace(), dtype=torch.uint8, device=self.device)
        return self.ws


def _scratch(model):
    s = getattr(model, '_sr_eval_scratch', None)
    if s is None:
        s = model._sr_eval_scratch = _Scratch(model.device)
    return s


def score_batches(model, batches):
    """(mean PSNR, mean SSIM, number of images) of the generator on a sized iterable of {'lr', 'hr'} batches of ONE image each
    (lr imagenet-normalised, hr in [-1, 1], NCHW fp32 on the device).  Image i's PSNR and SSIM sums go to slot i of one f64
    device table, read once at the end; the result is the mean of the per-image values (the reference's)."""
    G, dev, L = model.G, model.device, ops.lib()
    scratch = _scratch(model)
    precision = sr_precision()
    G.eval_coeffs(precision)
    slots = torch.zeros((2, max(len(batches), 1)), dtype=torch.float64, device=dev)      # [sse | ssim sum][image]
    sizes = []
    cur = torch.cuda.current_stream(dev)
    for batch in batches:
        ev = batch.get('ready')
        if ev is not None:
            cur.wait_event(ev)
        lr, hr = batch['lr'], batch['hr']
        for t in (lr, hr):
            t.record_stream(cur)
        lr, hr = lr.to(dev, torch.float32).contiguous(), hr.to(dev, torch.float32).contiguous()
        N, _, h, w = lr.shape
        if len(sizes) == slots.shape[1]:
            raise ValueError('score_batches: more batches than len(batches) = %d' % slots.shape[1])
        if N != 1:
            raise ValueError('score_batches: one image per batch (got %d)' % N)
        out = infer_image(G, lr, precision)
        H, W = 4 * h, 4 * w
        if tuple(hr.shape[2:]) != (H, W):
            raise ValueError('score_batches: hr %s is not 4 x lr %s' % (tuple(hr.shape[2:]), (h, w)))
        fake = scratch.image(3 * H * W)
        if precision == 'fp32':
            ops.nhwc_to_nchw_f32(out, fake)
        else:
            op, _, _, _, _, ld = ops.geom(out)
            check(L.gcc_nhwc_bf16_to_nchw_f32(op, fake.data_ptr(), 1, 3, H, W, ld, 0, ops.stream()), 'gcc_nhwc_bf16_to_nchw_f32')
        i = len(sizes)
        ws = scratch.workspace()
        check(L.gcc_psnr_y_sse(fake.data_ptr(), hr.data_ptr(), 1, H, W, slots[0, i:].data_ptr(), 0, ws.data_ptr(), ws.numel(),
                               ops.stream()), 'gcc_psnr_y_sse')
        check(L.gcc_ssim_y_sum(fake.data_ptr(), hr.data_ptr(), 1, H, W, slots[1, i:].data_ptr(), 0, ws.data_ptr(), ws.numel(),
                               ops.stream()), 'gcc_ssim_y_sum')
        sizes.append((H, W))
    if not sizes:
        return float('nan'), float('nan'), 0
    s, q = slots[:, :len(sizes)].cpu().tolist()
    psnrs, ssims = [], []
    for e, m, (H, W) in zip(s, q, sizes):
        mse = e / ((H - 8) * (W - 8))
        psnrs.append(10.0 * math.log10(255.0 ** 2 / mse) if mse > 0 else float('inf'))
        ssims.append(m / ((H - 14) * (W - 14)))
    return sum(psnrs) / len(psnrs), sum(ssims) / len(ssims), len(sizes)


def test_srgan_psnr(model, opt, dataset_name='Set5'):
    """metric/test_metric.py:89-127: (mean PSNR, mean SSIM) of the generator over <dataroot>/test/<dataset_name>"""
    from ..data import create_dataset
    opt = copy.deepcopy(opt)
    opt.phase = 'test/' + dataset_name
    opt.batch_size = 1
    opt.serial_batches = True
    psnr, ssim, _ = score_batches(model, create_dataset(opt, model.device))
    return psnr, ssim


test_srgan_psnr.__test__ = False       # a library function, not a test: keeps pytest from collecting it where it is imported


def available_sets(opt):
    """the reference's test sets present under <dataroot>/test, in its order"""
    root = os.path.join(str(opt.dataroot), 'test')
    return [n for n in SR_TEST_SETS if os.path.isdir(os.path.join(root, n))]


def srgan_evaluator(logger, sets):
    """evaluate(model, opt) for gcc_amd.train.run_evaluation: per set the reference's log line; PSNR slots first, then SSIM
    slots, each tagged with the set name"""
    def evaluate(model, opt):
        psnrs, ssims = [], []
        for name in sets:
            psnr, ssim = test_srgan_psnr(model, opt, name)
            logger.info('%s:PSNR: %.2f| SSIM: %.2f' % (name, psnr, ssim))
            psnrs.append((psnr, name))
            ssims.append((ssim, name))
        return psnrs + ssims
    return evaluate
