"""numpy restatement of the Cityscapes scorer's arithmetic (PIL's 32-bit float BILINEAR resample driven by
gcc_amd.metric.cityscapes.resample_tables, numpy.argmax, the oracle's fast_hist), shared by the CPU and the GPU tests of the
fused scorer.  numpy never fuses a multiply with an add, which is what Pillow's x86-64 build does too."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'miou_cityscapes.npz')
EVAL_H, EVAL_W = 1024, 2048


def expand_labels(blocks):
    return np.repeat(np.repeat(blocks, 16, axis=-2), 16, axis=-1)


def full_scores(seed):
    return (np.random.RandomState(int(seed)).randint(-2 ** 20, 2 ** 20, (1, 19, 256, 256)) / 2 ** 16).astype(np.float32)


def resample_last_axis(src, n_out):
    """one pass of Resample.c for float images along the last axis: f64 accumulation in tap order, every tap inside the bounds
    multiplied whatever its coefficient, fp32 result"""
    from gcc_amd.metric.cityscapes import resample_tables
    bounds, coef = resample_tables(src.shape[-1], n_out)
    acc = np.zeros(src.shape[:-1] + (n_out,), dtype=np.float64)
    with np.errstate(invalid='ignore'):
        for k in range(coef.shape[1]):
            idx = np.minimum(bounds[:, 0] + k, src.shape[-1] - 1)
            acc = np.where(k < bounds[:, 1], acc + src[..., idx].astype(np.float64) * coef[:, k], acc)
    return acc.astype(np.float32)


def resize(a, H, W):
    """Image.fromarray(a).resize((W, H), Image.BILINEAR) for every [h, w] plane of a [..., h, w] fp32 array: horizontal pass,
    then vertical pass"""
    t = resample_last_axis(np.asarray(a, dtype=np.float32), W)
    return np.swapaxes(resample_last_axis(np.ascontiguousarray(np.swapaxes(t, -1, -2)), H), -1, -2)


def predict(scores, H=EVAL_H, W=EVAL_W):
    """resize_4d_tensor(scores, W, H).argmax(axis=1) one class plane at a time, as uint8 [N, H, W]"""
    N, C = scores.shape[:2]
    pred = np.zeros((N, H, W), dtype=np.uint8)
    for n in range(N):
        best = resize(scores[n, 0], H, W)
        for c in range(1, C):
            v = resize(scores[n, c], H, W)
            with np.errstate(invalid='ignore'):
                take = ~np.isnan(best) & ((v > best) | np.isnan(v))       # numpy.argmax: first maximum, first NaN
            best = np.where(take, v, best)
            pred[n][take] = c
    return pred


def sha256(pred):
    return hashlib.sha256(np.ascontiguousarray(pred, dtype=np.uint8).tobytes()).hexdigest()


def normalise(fakes):
    """SegList's ToTensor + Normalize in fp32 on uint8 [N, h, w, 3] -> [N, 3, h, w]"""
    from gcc_amd.metric.cityscapes import SEG_MEAN, SEG_STD
    x = np.transpose(fakes, (0, 3, 1, 2)).astype(np.float32) / np.float32(255)
    m = np.asarray(SEG_MEAN, dtype=np.float32).reshape(1, 3, 1, 1)
    s = np.asarray(SEG_STD, dtype=np.float32).reshape(1, 3, 1, 1)
    return (x - m) / s


def miou(hist):
    from oracle import metric_oracle as M
    return round(float(np.nanmean(M.per_class_iu(np.asarray(hist, dtype=np.float64)) * 100)), 2)


def write_root(root, z, photos=None):
    """table.txt and the label PNGs of the fixture under ``root``; ``photos``: {name: uint8 [h, w, 3]} written under val/"""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, 'table.txt'), 'w') as f:
        f.write('\n'.join(str(l) for l in z['table_lines']) + '\n')
    labels = expand_labels(z['label_blocks'])
    for line, lab in zip(z['table_lines'], labels):
        path = os.path.join(root, str(line).split(' ')[1])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(lab).save(path)
    for name, im in (photos or {}).items():
        os.makedirs(os.path.join(root, 'val'), exist_ok=True)
        Image.fromarray(im).save(os.path.join(root, 'val', name + '.png'))
    return labels


def labels_for(z, rels):
    """the expanded label maps (uint8 [len(rels), 1024, 2048]) of label files named as table.txt names them"""
    files = [str(l).split(' ')[1] for l in z['table_lines']]
    return expand_labels(z['label_blocks'][[files.index(str(r)) for r in rels]])
