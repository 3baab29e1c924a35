#!/usr/bin/env python3
"""Generate tests/golden/miou_cityscapes.npz by IMPORTING THE REAL REFERENCE (metric/mIoU_score.py, unmodified) through
make_fixtures.import_reference(): its SegList, resize_4d_tensor, fast_hist, per_class_iu and test() produce every expected
value below.  Runs only in the authoring container; never imported by the tests.  Nothing of the reference is copied: the file
holds data (inputs and expected outputs).

    python tests/golden/make_miou_fixtures.py

Contents
  label_blocks        uint8 [3][64][128], values 0..18 and 255.  The label images are these expanded to 1024 x 2048 with
                      np.repeat(., 16) along both axes (expand_labels below; recipe and tests alike), written as PNGs
  table_lines, names, label_list        table.txt, the three image names of the cases below and the label files SegList derives
  names_more, label_list_more           a longer name list through SegList.read_lists: both matching branches, first match wins
  small.fakes         uint8 [2][64][96][3]  (image 0 noise, image 1 8 x 8 blocks)
  small.inputs        fp32 [2][3][64][96]   what SegList's transforms (ToTensor, Normalize) hand the segmenter
  small.scores        fp32 [2][19][64][96]  the stand-in segmenter's CPU output for those inputs, with one exact tie (image 0:
                      classes 11 and 4 share the maximum over a 3 x 3 source block) and one NaN pair (image 1: classes 7 and 3 at
                      one source pixel) planted by the stand-in itself, so that the reference's test() sees them
  small.hist / .per_class / .miou / .pred_sha256      the reference's test() result for (fakes, names[:2]) and, from the same
                      score maps through resize_4d_tensor / argmax / fast_hist / per_class_iu, the confusion matrix, the
                      per-class IoU and the SHA-256 of the class maps as uint8 [2][1024][2048]
  full.seed / .hist / .miou / .pred_sha256            one full-size case, 19 x 256 x 256 -> 1024 x 2048 against label 2: the scores
                      are full_scores(seed) below (integers / 2**16: the same bits everywhere), only the results are stored
"""
import hashlib
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

TIE = (0, 11, 4, 20, 30)          # image, class, class, source row, source column of the 3 x 3 block
NAN = (1, 7, 3, 40, 50)           # image, class, class, source row, source column


def expand_labels(blocks):
    return np.repeat(np.repeat(blocks, 16, axis=-2), 16, axis=-1)


def full_scores(seed):
    return (np.random.RandomState(seed).randint(-2 ** 20, 2 ** 20, (1, 19, 256, 256)) / 2 ** 16).astype(np.float32)


def make_inputs():
    rs = np.random.RandomState(20261016)
    blocks = rs.randint(0, 19, (3, 64, 128)).astype(np.uint8)
    blocks[rs.rand(3, 64, 128) < 0.1] = 255
    blocks[:, :4, :8] = np.arange(19, dtype=np.uint8)[(np.arange(32) % 19)].reshape(4, 8)       # every class present
    fakes = np.empty((2, 64, 96, 3), dtype=np.uint8)
    fakes[0] = rs.randint(0, 256, (64, 96, 3))
    fakes[1] = np.repeat(np.repeat(rs.randint(0, 256, (8, 12, 3)), 8, axis=0), 8, axis=1)
    return blocks, fakes


class StandIn(torch.nn.Module):
    """one seeded convolution + log_softmax in place of DRN; plants the tie and the NaN pair and keeps what it saw and returned"""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 19, 3, padding=1)
        g = torch.Generator().manual_seed(7)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(self.conv.weight.shape, generator=g) * 0.5)
            self.conv.bias.copy_(torch.randn(19, generator=g) * 0.1)
        self.inputs, self.outputs = [], []

    def forward(self, x):
        y = torch.log_softmax(self.conv(x), dim=1)
        i = len(self.outputs)
        if i == TIE[0]:
            _, a, b, r, c = TIE
            y[0, a, r:r + 3, c:c + 3] = 1.0
            y[0, b, r:r + 3, c:c + 3] = 1.0
        if i == NAN[0]:
            _, a, b, r, c = NAN
            y[0, a, r, c] = float('nan')
            y[0, b, r, c] = float('nan')
        self.inputs.append(x.clone())
        self.outputs.append(y.clone())
        return y, None


def main():
    np.int = int                   # the reference's ToTensor uses the alias numpy 2 removed; this process only
    from PIL import Image
    import make_fixtures as F
    F.import_reference()
    # import stubs only, as fixture_metric's: metric/fid_score.py imports cv2.imread, metric/inception.py subclasses torchvision's
    # Inception blocks at import time; nothing below touches either
    sys.modules['cv2'].imread = None
    base = type('InceptionBlock', (torch.nn.Module,), {})
    sys.modules['torchvision.models'].inception = F._stub('torchvision.models.inception', InceptionA=base, InceptionC=base,
                                                          InceptionE=base)
    sys.modules['torchvision'].models = sys.modules['torchvision.models']
    from metric import mIoU_score as R

    blocks, fakes = make_inputs()
    table_lines = ['0 labels/zero_trainIds.png photos/val_000027.png',
                   '1 labels/one_trainIds.png photos/val_000032.png',
                   '2 labels/frankfurt_000000_000294_gtFine_labelTrainIds.png photos/frankfurt_000000_000294_leftImg8bit.png']
    names = ['0', '1', 'frankfurt_000000_000294_leftImg8bit']
    # '27' and '000032' match only through endswith; '2' meets line 1 first ("val_000032" ends with it): the first match wins
    names_more = ['2', '27', '000032', '1', '000294_leftImg8bit', '0']
    out = {'label_blocks': blocks, 'table_lines': np.array(table_lines), 'names': np.array(names),
           'names_more': np.array(names_more), 'small.fakes': fakes}
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, 'labels'))
        table = os.path.join(d, 'table.txt')
        with open(table, 'w') as f:
            f.write('\n'.join(table_lines) + '\n')
        labels = expand_labels(blocks)
        by_file = {line.split(' ')[1]: lab for line, lab in zip(table_lines, labels)}
        for rel, lab in by_file.items():
            Image.fromarray(lab).save(os.path.join(d, rel))
        out['label_list'] = np.array(R.SegList([None] * 3, names, table, d).label_list)
        out['label_list_more'] = np.array(R.SegList([None] * len(names_more), names_more, table, d).label_list)

        seg = StandIn()
        miou = R.test(list(fakes), names[:2], seg, torch.device('cpu'), table_path=table, data_dir=d, batch_size=1, num_workers=0,
                      use_tqdm=False)
        out['small.inputs'] = torch.cat(seg.inputs).numpy()
        scores = torch.cat(seg.outputs)
        out['small.scores'] = scores.numpy()
        pred = R.resize_4d_tensor(scores, 2048, 1024).argmax(axis=1)
        hist = sum(R.fast_hist(pred[i].flatten(), by_file[out['label_list'][i]].astype(np.int64).flatten(), 19) for i in range(2))
        with np.errstate(divide='ignore', invalid='ignore'):
            iu = R.per_class_iu(hist.astype(np.float64))
        assert round(np.nanmean(iu * 100), 2) == miou, (round(np.nanmean(iu * 100), 2), miou)
        out['small.hist'], out['small.per_class'], out['small.miou'] = hist.astype(np.int64), iu, np.float64(miou)
        out['small.pred_sha256'] = np.array(hashlib.sha256(pred.astype(np.uint8).tobytes()).hexdigest())
        # the plants did what they are there for
        at = lambda r, c: (int(r * 1024 / 64), int(c * 2048 / 96))           # the output pixel over a source position
        assert pred[(0,) + at(TIE[3] + 1.5, TIE[4] + 1.5)] == min(TIE[1], TIE[2])
        assert pred[(1,) + at(NAN[3] + 0.5, NAN[4] + 0.5)] == min(NAN[1], NAN[2])

        seed = 355
        fs = torch.from_numpy(full_scores(seed))
        fpred = R.resize_4d_tensor(fs, 2048, 1024).argmax(axis=1)
        fhist = R.fast_hist(fpred.flatten(), by_file[out['label_list'][2]].astype(np.int64).flatten(), 19)
        with np.errstate(divide='ignore', invalid='ignore'):
            fiu = R.per_class_iu(fhist.astype(np.float64))
        out['full.seed'], out['full.hist'], out['full.miou'] = np.int64(seed), fhist.astype(np.int64), np.float64(round(np.nanmean(fiu * 100), 2))
        out['full.pred_sha256'] = np.array(hashlib.sha256(fpred.astype(np.uint8).tobytes()).hexdigest())
    path = os.path.join(HERE, 'miou_cityscapes.npz')
    np.savez_compressed(path, **out)
    print('miou_cityscapes ok: small mIoU %.2f, full mIoU %.2f, %d bytes' % (miou, float(out['full.miou']), os.path.getsize(path)))


if __name__ == '__main__':
    torch.set_num_threads(8)
    main()
