"""Host side of the Cityscapes mIoU evaluation (gcc_amd.metric.cityscapes): the resample tables against Pillow, the scorer's
arithmetic restated in numpy against the reference's results (tests/golden/miou_cityscapes.npz, written by
tests/golden/make_miou_fixtures.py from the reference's own SegList / resize_4d_tensor / fast_hist / test()), the label table
rule, the segmenter-input normalisation, the built-in evaluator's selection rule and the ABI surface.  No GPU."""
import logging
import os
import re

import numpy as np
import pytest
import torch

from tests import _miou_emul as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def z():
    return np.load(E.GOLDEN)


@pytest.mark.parametrize('h,w', [(256, 256), (250, 300), (128, 256), (1024, 2048), (1024, 512), (7, 9), (32, 2048)])
def test_resample_tables_equal_pillow_bit_for_bit(h, w):
    from PIL import Image
    a = (np.random.RandomState(h * 4099 + w).randn(h, w) * 3).astype(np.float32)
    ref = np.array(Image.fromarray(a).resize((E.EVAL_W, E.EVAL_H), Image.BILINEAR))
    got = E.resize(a, E.EVAL_H, E.EVAL_W)
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize('h,w,H,W', [(7, 9, 21, 300), (3, 257, 40, 257), (250, 300, 256, 301), (255, 511, 256, 512), (1, 1, 9, 2)])
def test_resample_tables_equal_pillow_at_other_output_sizes(h, w, H, W):
    from PIL import Image
    a = (np.random.RandomState(H * 4099 + W).randn(h, w) * 3).astype(np.float32)
    ref = np.array(Image.fromarray(a).resize((W, H), Image.BILINEAR))
    assert np.array_equal(E.resize(a, H, W).view(np.uint32), ref.view(np.uint32))


def test_resample_tables_shape_and_sharing():
    from gcc_amd.data import precompute_coeffs, resample_coeffs
    from gcc_amd.metric.cityscapes import resample_tables
    b, c = resample_tables(256, 2048)
    assert b.dtype == np.int32 and b.shape == (2048, 2) and c.dtype == np.float64 and c.shape == (2048, 3)
    assert b[:, 1].max() == 2 and (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 256).all()
    assert resample_tables(256, 2048)[1] is c                                 # cached
    b1, c1 = resample_tables(1024, 1024)                                      # the pass PIL skips
    assert c1.shape == (1024, 1) and (c1 == 1.0).all() and np.array_equal(b1[:, 0], np.arange(1024)) and (b1[:, 1] == 1).all()
    # one routine behind the 8-bit tables and these: the fixed-point coefficients are the rounded doubles
    pb, pk, ksize = precompute_coeffs(178, 64, 'bilinear')
    qb, qc, qk = resample_coeffs(178, 64, 'bilinear')
    assert qk == ksize and [tuple(r) for r in qb] == pb
    assert all(qc[i, j] == int(0.5 + v * (1 << 22)) for i, row in enumerate(pk) for j, v in enumerate(row))


def test_emulation_reproduces_reference_small(z):
    from oracle import metric_oracle as M
    labels = E.labels_for(z, z['label_list'][:2])
    pred = E.predict(z['small.scores'])
    assert E.sha256(pred) == str(z['small.pred_sha256'])
    hist = sum(M.fast_hist(pred[i].reshape(-1).astype(np.int64), labels[i].reshape(-1).astype(np.int64), 19) for i in range(2))
    assert np.array_equal(hist, z['small.hist'])
    assert np.array_equal(M.per_class_iu(hist.astype(np.float64)), z['small.per_class'], equal_nan=True)
    assert E.miou(hist) == float(z['small.miou'])
    # the planted tie and NaN pair resolve to the first class
    s = z['small.scores']
    tie = np.argwhere((s[0, 11] == 1.0) & (s[0, 4] == 1.0))
    assert len(tie) == 9
    r, c = tie[4]
    assert pred[0, int((r + 0.5) * 16), int((c + 0.5) * 2048 / 96)] == 4
    r, c = np.argwhere(np.isnan(s[1, 7]) & np.isnan(s[1, 3]))[0]
    assert pred[1, int((r + 0.5) * 16), int((c + 0.5) * 2048 / 96)] == 3


def test_emulation_reproduces_reference_full_size(z):
    from oracle import metric_oracle as M
    label = E.labels_for(z, z['label_list'][2:])[0]
    pred = E.predict(E.full_scores(z['full.seed']))
    assert E.sha256(pred) == str(z['full.pred_sha256'])
    hist = M.fast_hist(pred.reshape(-1).astype(np.int64), label.reshape(-1).astype(np.int64), 19)
    assert np.array_equal(hist, z['full.hist'])
    assert E.miou(hist) == float(z['full.miou'])


def test_label_list(z, tmp_path):
    from gcc_amd._lib import GccError
    from gcc_amd.metric.cityscapes import label_list
    table = tmp_path / 'table.txt'
    table.write_text('\n'.join(str(l) for l in z['table_lines']) + '\n')
    assert label_list([str(n) for n in z['names']], str(table)) == [str(l) for l in z['label_list']]
    assert label_list([str(n) for n in z['names_more']], str(table)) == [str(l) for l in z['label_list_more']]
    with pytest.raises(GccError, match='no_such_image'):
        label_list(['0', 'no_such_image'], str(table))


def test_normalisation_restated(z):
    got = E.normalise(z['small.fakes'])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), z['small.inputs'].view(np.uint32))
    # every byte value in every channel, against torch's own arithmetic in the reference's order
    from gcc_amd.metric.cityscapes import SEG_MEAN, SEG_STD
    allb = np.broadcast_to(np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1), (1, 16, 16, 3))
    t = torch.from_numpy(np.ascontiguousarray(np.transpose(allb[0], (2, 0, 1)))).float() / 255
    for ch, m, s in zip(t, torch.FloatTensor(SEG_MEAN), torch.FloatTensor(SEG_STD)):
        ch.sub_(m).div_(s)
    assert np.array_equal(E.normalise(allb)[0].view(np.uint32), t.numpy().view(np.uint32))


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


class _StandIn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 19, 1)

    def forward(self, x):
        return torch.log_softmax(self.conv(x), dim=1), x


def test_builtin_evaluator_selection(tmp_path):
    from gcc_amd import train
    from gcc_amd.options import options
    log = logging.getLogger('miou_cityscapes_test')
    log.setLevel(logging.INFO)
    h = _Lines()
    log.addHandler(h)
    root = tmp_path / 'cityscapes'
    drn = tmp_path / 'drn.pt'
    opt = lambda r=root, d=drn, model='pix2pix': options.parse(['--dataroot', str(r), '--model', model, '--drn_path', str(d)])

    def refused(o, word):
        h.lines.clear()
        assert train.builtin_evaluator(o, log) is None
        assert len(h.lines) == 1 and word in h.lines[0], h.lines

    root.mkdir()
    refused(opt(), 'table.txt')
    (root / 'table.txt').write_text('0 a_trainIds.png a.png\n')
    refused(opt(), 'does not exist')
    torch.save(_StandIn().state_dict(), str(drn))
    refused(opt(), 'TorchScript')
    assert 'Error' in h.lines[0] or 'Exception' in h.lines[0]      # the loader's own error is quoted
    torch.jit.script(_StandIn()).save(str(drn))
    h.lines.clear()
    assert callable(train.builtin_evaluator(opt(), log))
    assert len(h.lines) == 1 and 'mIoU' in h.lines[0]
    # other roots and models keep what they had
    other = tmp_path / 'maps'
    other.mkdir()
    (other / 'table.txt').write_text('0 a_trainIds.png a.png\n')
    h.lines.clear()
    assert train.builtin_evaluator(opt(r=other), log) is None
    assert train.builtin_evaluator(opt(model='cyclegan'), log) is None
    assert train.builtin_evaluator(options.parse(['--dataroot', 'synthetic', '--model', 'pix2pix']), log) is None
    log.removeHandler(h)


def test_abi_surface():
    from gcc_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'gcc_hip.h')).read()
    for name in ('gcc_seg_input', 'gcc_miou_score'):
        assert name in _lib.PROTOTYPES
        m = re.search(r'^int %s\(([^;]*)\);' % name, header, re.M)
        assert m, name
        assert len(m.group(1).split(',')) == len(_lib.PROTOTYPES[name][1])
    assert re.search(r'#define GCC_HIP_ABI 605\b', header) and _lib.GCC_HIP_ABI == 605
