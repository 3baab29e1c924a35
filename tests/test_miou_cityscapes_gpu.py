"""The Cityscapes mIoU evaluation on the GPU (gcc_amd.metric.cityscapes over gcc_seg_input / gcc_miou_score): bit-exact against
the reference's results (tests/golden/miou_cityscapes.npz) and against PIL + numpy on the same score maps, without an
output-sized score tensor, and end to end through cityscapes_evaluator, gcc_amd.train.main and mIoU_score.test()."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import gcc_oracle as O
from oracle import metric_oracle as M
from tests import _miou_emul as E
from tests.golden.recipe import recipe_state_dict

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def z():
    return np.load(E.GOLDEN)


def _hist(pred, labels):
    return sum(M.fast_hist(p.reshape(-1).astype(np.int64), l.reshape(-1).astype(np.int64), 19) for p, l in zip(pred, labels))


# ---- 1. gcc_seg_input ---------------------------------------------------------------------------------------------------
def test_seg_input_u8_route_matches_reference(z):
    from gcc_amd.metric import cityscapes as CS
    got = CS.seg_input(torch.from_numpy(z['small.fakes']).to(DEV)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == z['small.inputs'].shape
    assert np.array_equal(got.view(np.uint32), z['small.inputs'].view(np.uint32))
    one = CS.seg_input(torch.from_numpy(z['small.fakes'][1]).to(DEV)).cpu().numpy()          # [h, w, 3] is one image
    assert np.array_equal(one.view(np.uint32), z['small.inputs'][1:].view(np.uint32))


def test_seg_input_bf16_route_every_byte_value():
    from gcc_amd import ops
    from gcc_amd.metric import cityscapes as CS
    mid = ((torch.arange(256, dtype=torch.float32) + 0.5) / 255.0 * 2 - 1).bfloat16().float()
    x = torch.stack([mid, mid.roll(85), mid.roll(170)]).view(1, 3, 16, 16)
    x = torch.cat([x, torch.tensor([-1.0, 1.0, 0.0, -3.0, 3.0, 0.99609375] + [0.0] * 762).view(1, 3, 16, 16)])
    a = np.transpose(x.numpy(), (0, 2, 3, 1))
    bytes_ = np.clip((a + np.float32(1)) / np.float32(2.0) * np.float32(255.0), 0, 255).astype(np.uint8)     # util.tensor2im
    for c in range(3):
        assert len(np.unique(bytes_[0, :, :, c])) == 256
    xd = ops.new_act(2, 3, 16, 16, DEV)
    ops.nchw_to_nhwc(x.to(DEV).contiguous(), xd)
    assert np.array_equal(ops.image_to_u8(xd).cpu().numpy(), bytes_)
    got = CS.seg_input(xd).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), E.normalise(bytes_).view(np.uint32))


# ---- 2. gcc_miou_score ----------------------------------------------------------------------------------------------------
def test_score_small_case_matches_reference(z):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import cityscapes as CS
    scores = torch.from_numpy(z['small.scores']).to(DEV)
    labels_h = E.labels_for(z, z['label_list'][:2])
    labels = torch.from_numpy(labels_h).to(DEV)
    pred = torch.full((2, 1024, 2048), 99, dtype=torch.uint8, device=DEV)
    hist = CS.score(scores, labels, pred=pred)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (19, 19)
    assert np.array_equal(hist.cpu().numpy(), z['small.hist'])
    got = pred.cpu().numpy()
    assert E.sha256(got) == str(z['small.pred_sha256'])
    want = E.predict(z['small.scores'])
    assert np.array_equal(got, want)                                                 # element-wise
    assert CS.miou(hist) == float(z['small.miou'])
    # the planted tie and NaN pair land where numpy puts them
    s = z['small.scores']
    r, c = np.argwhere((s[0, 11] == 1.0) & (s[0, 4] == 1.0))[4]
    assert got[0, int((r + 0.5) * 16), int((c + 0.5) * 2048 / 96)] == 4
    r, c = np.argwhere(np.isnan(s[1, 7]) & np.isnan(s[1, 3]))[0]
    assert got[1, int((r + 0.5) * 16), int((c + 0.5) * 2048 / 96)] == 3
    # accumulation; N = 2 in one call against two calls of N = 1; pred is optional
    again = CS.score(scores, labels, hist=hist)
    assert again is hist and np.array_equal(hist.cpu().numpy(), 2 * z['small.hist'])
    h1 = CS.score(scores[:1], labels[:1])
    first = h1.cpu().numpy().copy()
    assert np.array_equal(first, _hist(want[:1], labels_h[:1]))
    CS.score(scores[1:], labels[1], hist=h1)                                         # a [H, W] label map is one image
    assert np.array_equal(h1.cpu().numpy(), z['small.hist'])
    # a label map of all 255 adds nothing
    before = h1.cpu().numpy().copy()
    CS.score(scores, torch.full_like(labels, 255), hist=h1)
    assert np.array_equal(h1.cpu().numpy(), before)
    # no route for a reducing resize: an error that names the sizes, and nothing accumulated
    with pytest.raises(GccError, match='64 x 96'):
        CS.score(scores, labels[:, :32, :2048].contiguous(), hist=h1)
    with pytest.raises(GccError):
        CS.score(scores, labels[:, :, :64].contiguous(), hist=h1)
    assert np.array_equal(h1.cpu().numpy(), before)


def test_score_full_size_matches_reference_without_resized_tensor(z):
    from gcc_amd.metric import cityscapes as CS
    scores = torch.from_numpy(E.full_scores(z['full.seed'])).to(DEV)
    labels = torch.from_numpy(E.labels_for(z, z['label_list'][2:])).to(DEV)
    pred = torch.empty((1, 1024, 2048), dtype=torch.uint8, device=DEV)
    hist = CS.score(scores, labels, pred=pred)
    assert np.array_equal(hist.cpu().numpy(), z['full.hist'])
    assert E.sha256(pred.cpu().numpy()) == str(z['full.pred_sha256'])
    assert CS.miou(hist) == float(z['full.miou'])
    # tables and labels are resident now: a further call may not allocate anything near one fp32 class plane at the output
    # size (the resized tensor of the unfused route is 19 of them, 159 MB)
    hist.zero_()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    CS.score(scores, labels, hist=hist)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(DEV) - base
    print('full-size score call: peak allocation grew by %d bytes' % grown)
    assert grown < 1024 * 2048 * 4
    assert np.array_equal(hist.cpu().numpy(), z['full.hist'])


def _pil_predict(scores, H, W):
    """resize_4d_tensor(scores, W, H).argmax(axis=1) with Pillow itself, one plane at a time"""
    from PIL import Image
    up = np.stack([np.stack([np.array(Image.fromarray(p).resize((W, H), Image.BILINEAR)) for p in img]) for img in scores])
    return up.argmax(axis=1).astype(np.uint8)


@pytest.mark.parametrize('C,h,w,H,W', [(64, 7, 9, 21, 300), (5, 16, 520, 16, 520), (19, 3, 257, 40, 257), (1, 1, 1, 9, 2),
                                       (19, 250, 300, 256, 301), (7, 255, 511, 256, 512)])
def test_score_other_sizes_match_pillow(C, h, w, H, W):
    """tile edges (H not a multiple of 8, W not a multiple of 256), the passes PIL skips, the widest class count, and scales
    just below 1, where a tile of 8 output rows touches the most source rows; expected values from Pillow's own resize"""
    from gcc_amd.metric import cityscapes as CS
    rs = np.random.RandomState(C * 1000 + W)
    scores = (rs.randint(-2 ** 12, 2 ** 12, (2, C, h, w)) / 2 ** 6).astype(np.float32)
    labels = rs.randint(0, 256, (2, H, W)).astype(np.uint8)
    labels[rs.rand(2, H, W) < 0.7] %= max(C, 2)
    pred = torch.empty((2, H, W), dtype=torch.uint8, device=DEV)
    hist = CS.score(torch.from_numpy(scores).to(DEV), torch.from_numpy(labels).to(DEV), pred=pred)
    want = _pil_predict(scores, H, W)
    assert np.array_equal(pred.cpu().numpy(), want)
    ref = sum(M.fast_hist(p.reshape(-1).astype(np.int64), l.reshape(-1).astype(np.int64), C) for p, l in zip(want, labels))
    assert np.array_equal(hist.cpu().numpy(), ref)


def test_score_refuses_outputs_on_another_device(z):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import cityscapes as CS
    scores = torch.from_numpy(z['small.scores'][:1]).to(DEV)
    labels = torch.zeros((1, 64, 96), dtype=torch.uint8, device=DEV)
    with pytest.raises(GccError, match='hist'):
        CS.score(scores, labels, hist=torch.zeros((19, 19), dtype=torch.int64))
    with pytest.raises(GccError, match='pred'):
        CS.score(scores, labels, pred=torch.zeros((1, 64, 96), dtype=torch.uint8))


# ---- 3. end to end --------------------------------------------------------------------------------------------------------
class _StandIn(torch.nn.Module):
    """one seeded convolution + log_softmax in place of DRN; returns (scores, features) as DRNSeg does"""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 19, 3, padding=1)
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(self.conv.weight.shape, generator=g) * 0.5)
            self.conv.bias.copy_(torch.randn(19, generator=g) * 0.1)

    def forward(self, x):
        return torch.log_softmax(self.conv(x), dim=1), x


class _Keep:
    """a plain callable around the segmenter that keeps every call's score maps"""

    def __init__(self, seg):
        self.seg, self.outputs = seg, []

    def __call__(self, x):
        y = self.seg(x)
        self.outputs.append(y[0].clone())
        return y


def _root(tmp_path, z):
    rng = np.random.RandomState(3)
    names = [str(n) for n in z['names']]
    photos = {n: rng.randint(0, 256, (256, 512, 3), dtype=np.uint8) for n in names}
    root = tmp_path / 'cityscapes'
    E.write_root(str(root), z, photos)
    drn = tmp_path / 'segmenter.pt'
    torch.jit.script(_StandIn()).save(str(drn))
    return root, drn, names


ARGV = ['--model', 'pix2pix', '--gpu_ids', '0', '--ngf', '8', '--ndf', '8', '--name', 'exp', '--print_freq', '1000']


def _pil_miou(outputs, labels):
    from PIL import Image
    hist = np.zeros((19, 19), dtype=np.int64)
    for s, lab in zip(outputs, labels):
        s = s.cpu().numpy()
        assert s.shape == (1, 19, 256, 256) and s.dtype == np.float32
        up = np.stack([np.array(Image.fromarray(s[0, c]).resize((2048, 1024), Image.BILINEAR)) for c in range(19)])
        hist += M.fast_hist(up.argmax(axis=0).reshape(-1), lab.reshape(-1).astype(np.int64), 19)
    return E.miou(hist)


def test_evaluator_and_reference_call_end_to_end(tmp_path, z, monkeypatch):
    from gcc_amd import ops
    from gcc_amd import test as gtest
    from gcc_amd.data import create_dataset
    from gcc_amd.metric import cityscapes as CS
    from gcc_amd.metric import mIoU_score
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    root, drn, names = _root(tmp_path, z)
    opt = options.parse(['--dataroot', str(root), '--drn_path', str(drn), '--checkpoints_dir', str(tmp_path / 'ck')] + ARGV)
    opt.isTrain = True
    model = get_model_class(opt)(opt)
    model.netG.load_state_dict({k: v.to(DEV) for k, v in recipe_state_dict(O.unet_shapes(8, 8), 17).items()})
    model.refresh_weights()
    model.model_eval()
    keep = _Keep(torch.jit.load(str(drn), map_location=DEV))
    lines = []
    logger = type('L', (), {'info': staticmethod(lines.append)})
    evaluate = CS.cityscapes_evaluator(keep, logger)
    # the loader builds each batch on its own stream: the evaluator must mark the batch's tensors as used on the stream that
    # reads them, or the allocator may give their memory to a later batch while the generator's launch is still queued
    marked = []
    real_record = torch.Tensor.record_stream
    monkeypatch.setattr(torch.Tensor, 'record_stream', lambda t, st: (marked.append((t.data_ptr(), st)), real_record(t, st))[1])
    # (a) the evaluator's value is what PIL + numpy + fast_hist make of the SAME device score maps
    (value, tag), = evaluate(model, opt)
    monkeypatch.undo()
    assert len(marked) == 6 and all(st == torch.cuda.current_stream(DEV) for _, st in marked)       # A and B of three batches
    assert tag == opt.direction and len(keep.outputs) == 3
    order = sorted(names)                                           # the loader walks val/ in sorted order
    labels = E.labels_for(z, CS.label_list(order, str(root / 'table.txt')))
    want = _pil_miou(keep.outputs, labels)
    print('evaluator mIoU %.2f, PIL + numpy on the same score maps %.2f' % (value, want))
    assert value == want
    assert lines == ['mIoU: %.2f' % value]
    cache = evaluate.state['cache']
    assert cache.decodes == 3
    assert evaluate(model, opt)[0][0] == value and cache.decodes == 3            # the second evaluation decodes nothing
    # (c) the reference's call: mIoU_score.test() without dataset=, on the bytes of the same generated images
    fakes = []
    for data in create_dataset(gtest.test_overrides(opt), model.device):
        fakes.append(ops.image_to_u8(model.infer_nhwc(data)).cpu().numpy()[0])
    got = mIoU_score.test(fakes, order, keep.seg, DEV, table_path=str(root / 'table.txt'), data_dir=str(root), use_tqdm=False)
    assert got == value
    with pytest.raises(Exception, match='no_such'):
        mIoU_score.test(fakes[:1], ['no_such'], keep.seg, DEV, table_path=str(root / 'table.txt'), data_dir=str(root))


def test_train_main_logs_miou_and_keeps_best(tmp_path, z, monkeypatch):
    import shutil
    from gcc_amd import train
    from gcc_amd.metric import cityscapes as CS
    root, drn, names = _root(tmp_path, z)
    shutil.copytree(str(root / 'val'), str(root / 'train'))
    decoded = []
    real = CS.LabelCache._decode
    monkeypatch.setattr(CS.LabelCache, '_decode', lambda self, rel: (decoded.append(rel), real(self, rel))[1])
    ck = tmp_path / 'ck'
    # a Cityscapes root fixes the schedule as the reference's options do (250 epochs, an evaluation every 5, BtoA): the run
    # starts at epoch 245, so it trains six epochs and evaluates after epochs 245 and 250
    model = train.main(['--dataroot', str(root), '--drn_path', str(drn), '--checkpoints_dir', str(ck), '--epoch_count', '245',
                        '--batch_size', '1'] + ARGV)
    torch.cuda.synchronize()
    log = (ck / 'exp' / 'logger.log').read_text()
    values = re.findall(r'^.*mIoU: ([0-9.]+)$', log, re.M)
    assert len(values) == 2, log[-2000:]
    assert 'End of epoch 245 / 250' in log and 'End of epoch 244' not in log
    assert sorted(decoded) == sorted(str(l) for l in z['label_list'])              # two evaluations, each file decoded once
    best = list((ck / 'exp' / 'checkpoints').glob('model_best_*.pth'))
    assert len(best) == 1 and best[0].name == 'model_best_BtoA.pth'
    assert model is not None


def test_cli_prints_miou_after_the_pngs(tmp_path, z):
    from gcc_amd.metric import cityscapes as CS
    from gcc_amd.models import get_model_class
    from gcc_amd.options import options
    root, drn, names = _root(tmp_path, z)
    argv = ['--dataroot', str(root), '--drn_path', str(drn), '--checkpoints_dir', str(tmp_path / 'ck')] + ARGV
    opt = options.parse(argv)
    opt.isTrain = True
    model = get_model_class(opt)(opt)
    model.netG.load_state_dict({k: v.to(DEV) for k, v in recipe_state_dict(O.unet_shapes(8, 8), 23).items()})
    model.refresh_weights()
    model.save_models(1, str(tmp_path / 'save'))
    model.model_eval()
    value = CS.cityscapes_evaluator(torch.jit.load(str(drn), map_location=DEV))(model, opt)[0][0]
    r = subprocess.run([sys.executable, '-m', 'gcc_amd.test'] + argv + ['--pretrain_path', str(tmp_path / 'save' / 'model_1.pth')],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert ('mIoU: %.2f' % value) in r.stdout.splitlines(), r.stdout[-2000:]
    assert len(list((tmp_path / 'ck' / 'exp' / 'test_results' / 'fake_B').glob('*.png'))) == 3
    # without the segmenter the run still writes its PNGs and says why there is no score
    r = subprocess.run([sys.executable, '-m', 'gcc_amd.test'] + argv[:2] + ['--drn_path', str(tmp_path / 'none.pt')] + argv[4:] +
                       ['--pretrain_path', str(tmp_path / 'save' / 'model_1.pth')], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'mIoU:' not in r.stdout and 'does not exist' in r.stdout, r.stdout[-2000:]
