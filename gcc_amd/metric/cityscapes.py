"""Cityscapes mIoU of a Pix2Pix generator (metric/test_metric.py:47-87 test_pix2pix_mIoU, metric/mIoU_score.py:70-105, 169-218):
everything around the segmentation network.  The network itself (DRN-D-105 in the reference) is any callable ``segmenter(x)``
whose result's element 0 is the [N, C, h, w] fp32 score map: drn_seg.DrnSegEngine from the reference's own weights file, or a
TorchScript archive.

    generator (model.infer_nhwc) -> gcc_seg_input (tensor2im's byte, ToTensor, Normalize) -> segmenter(x)[0]
        -> gcc_miou_score (PIL's float BILINEAR resize to the labels' size + argmax + fast_hist, one launch, exact)
        -> per_class_iu / nanmean / round(., 2) on the host, once per evaluation

The label images (``table.txt`` names them) are decoded once per training run and stay on the device."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import ops
from .._lib import GccError, check
from ..data import precompute_coeffs
from .mIoU_score import per_class_iu

# metric/mIoU_score.py:80-81; the kernel takes them as fp32, rounded as torch.FloatTensor rounds them
SEG_MEAN = (0.29010095242892997, 0.32808144844279574, 0.28696394422942517)
SEG_STD = (0.1829540508368939, 0.18656561047509476, 0.18447508988480435)
EVAL_SIZE = (1024, 2048)          # metric/mIoU_score.py:212 resize_4d_tensor(final, 2048, 1024): (height, width)
NUM_CLASSES = 19
DECODE_THREADS = 16
_ERR_UNSUPPORTED = -2             # include/gcc_hip.h GCC_ERR_UNSUPPORTED

_tables = {}
_dev_tables = {}


def resample_tables(in_size, out_size):
    """Pillow's precompute_coeffs for BILINEAR in double precision, as its 32-bit float resample uses them (not normalised to
    fixed point): (bounds int32 [out, 2] = first source index and tap count, coefficients float64 [out, ksize]).  Equal sizes
    (a pass PIL skips) give the one-tap table {1.0}: 0.0 + v * 1.0 reproduces v up to the sign of zero, which no comparison sees."""
    key = (int(in_size), int(out_size))
    if key not in _tables:
        if key[0] == key[1]:
            b, k, ksize = [(i, 1) for i in range(key[1])], [[1.0]] * key[1], 1
        else:
            b, k, ksize = precompute_coeffs(key[0], key[1], 'bilinear')
        bounds = np.asarray(b, dtype=np.int32).reshape(key[1], 2)
        coef = np.zeros((key[1], ksize), dtype=np.float64)
        for i, row in enumerate(k):
            coef[i, :len(row)] = row
        _tables[key] = (bounds, coef)
    return _tables[key]


def device_tables(in_size, out_size, device):
    key = (int(in_size), int(out_size), torch.device(device))
    if key not in _dev_tables:
        b, c = resample_tables(in_size, out_size)
        _dev_tables[key] = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device))
    return _dev_tables[key]


def read_table(table_path):
    """the lines of table.txt: "<index> <trainIds png> <photo png>" (written by the reference's dataset preparation)"""
    with open(table_path, 'r') as f:
        return [line.strip().split(' ') for line in f.readlines()]


def _match(name, table, table_path):
    for item in table:
        if item[0] == name or item[2][:-len('.png')].endswith(name):
            return item[1]
    raise GccError('label_list: no line of %s matches the image name %r' % (table_path, name))


def label_list(names, table_path):
    """SegList.read_lists (metric/mIoU_score.py:93-105): per name the label file of the first table line whose index equals the
    name or whose photo path (less '.png') ends with it"""
    table = read_table(table_path)
    return [_match(name, table, table_path) for name in names]


class LabelCache:
    """label images (trainIds PNGs, 8-bit) as uint8 [H, W] device tensors, decoded with PIL on at most 16 host threads and kept
    for the life of the object: a training run decodes each file once (500 x 2 MB for the Cityscapes validation set)"""

    def __init__(self, data_dir, device):
        self.data_dir, self.device = str(data_dir), device
        self.labels = {}
        self.decodes = 0

    def _decode(self, rel):
        from PIL import Image
        a = np.array(Image.open(os.path.join(self.data_dir, rel)))
        if a.dtype != np.uint8 or a.ndim != 2:
            raise GccError('label image %s: expected an 8-bit single-channel PNG, got %s %s' % (rel, a.dtype, a.shape))
        return np.ascontiguousarray(a)

    def prefetch(self, rels):
        todo = [r for r in dict.fromkeys(rels) if r not in self.labels]
        if not todo:
            return
        with ThreadPoolExecutor(min(DECODE_THREADS, len(todo))) as pool:
            for rel, a in zip(todo, pool.map(self._decode, todo)):
                self.labels[rel] = torch.from_numpy(a).to(self.device)
                self.decodes += 1

    def get(self, rel):
        if rel not in self.labels:
            self.prefetch([rel])
        return self.labels[rel]


def _f3(v):
    return (ctypes.c_float * 3)(*v)


def seg_input(image, out=None):
    """the segmenter's input (NCHW fp32 [N, 3, H, W]) of generated images: an NHWC bf16 activation (the generator's output; the
    byte of util.tensor2im first) or a uint8 [N, H, W, 3] device tensor (those bytes themselves); gcc_seg_input.  An NHWC fp32
    activation (the generator's fp32 route) becomes its bytes first (gcc_image_to_u8_f32) and goes on as uint8."""
    if image.dtype == torch.float32:
        image = ops.image_to_u8(image)
    if image.dtype == torch.uint8:
        if image.dim() == 3:
            image = image[None]
        image = image.contiguous()
        N, H, W, c3 = image.shape
        if c3 != 3:
            raise GccError('seg_input: expected uint8 [N, H, W, 3], got %s' % (tuple(image.shape),))
        ptr, is_u8, ld = image.data_ptr(), 1, 0
    else:
        ptr, N, _, H, W, ld = ops.geom(image)
        is_u8 = 0
    if out is None:
        out = torch.empty((N, 3, H, W), dtype=torch.float32, device=image.device)
    check(ops.lib().gcc_seg_input(ptr, is_u8, ld, 0, N, H, W, _f3(SEG_MEAN), _f3(SEG_STD), out.data_ptr(), ops.stream()),
          'gcc_seg_input')
    return out


def score(scores, labels, hist=None, pred=None):
    """gcc_miou_score: the confusion matrix of resize_4d_tensor(scores, W, H).argmax(axis=1) against labels, accumulated into
    (and returned as) the int64 [C, C] device tensor ``hist``.  scores: [N, C, h, w] fp32 device tensor; labels: uint8 [N, H, W]
    (or [H, W]) device tensor; pred: optional uint8 [N, H, W] device tensor that receives the class map."""
    if scores.dtype != torch.float32 or scores.dim() != 4 or not scores.is_cuda:
        raise GccError('score: scores must be a [N, C, h, w] fp32 device tensor')
    if labels.dim() == 2:
        labels = labels[None]
    if labels.dtype != torch.uint8 or labels.dim() != 3 or labels.device != scores.device:
        raise GccError('score: labels must be a uint8 [N, H, W] tensor on the scores\' device')
    scores, labels = scores.contiguous(), labels.contiguous()
    N, C, h, w = scores.shape
    H, W = labels.shape[1:]
    if labels.shape[0] != N:
        raise GccError('score: %d score maps against %d label maps' % (N, labels.shape[0]))
    if hist is None:
        hist = torch.zeros((C, C), dtype=torch.int64, device=scores.device)
    if tuple(hist.shape) != (C, C) or hist.dtype != torch.int64 or not hist.is_contiguous() or hist.device != scores.device:
        raise GccError('score: hist must be a contiguous int64 [%d, %d] tensor on the scores\' device' % (C, C))
    if pred is not None and (pred.dtype != torch.uint8 or pred.numel() != N * H * W or not pred.is_contiguous() or
                             pred.device != scores.device):
        raise GccError('score: pred must be a contiguous uint8 [%d, %d, %d] tensor on the scores\' device' % (N, H, W))
    hb, hc = device_tables(w, W, scores.device)
    vb, vc = device_tables(h, H, scores.device)
    rc = ops.lib().gcc_miou_score(scores.data_ptr(), N, C, h, w, labels.data_ptr(), H, W, hb.data_ptr(), hc.data_ptr(), hc.shape[1],
                                  vb.data_ptr(), vc.data_ptr(), vc.shape[1], hist.data_ptr(),
                                  pred.data_ptr() if pred is not None else None, ops.stream())
    if rc == _ERR_UNSUPPORTED:
        raise GccError('gcc_miou_score: score maps of %d x %d (%d classes) against labels of %d x %d: the fused scorer enlarges '
                       'only (h <= H, w <= W) and takes at most 64 classes; there is no other route' % (h, w, C, H, W))
    check(rc, 'gcc_miou_score')
    return hist


def miou(hist):
    """metric/mIoU_score.py:217-218 (the one host read of an evaluation)"""
    return round(float(np.nanmean(per_class_iu(hist) * 100)), 2)


class _Batcher:
    """segmenter inputs and their labels gathered into batches of ``batch_size``, scored into one histogram"""

    def __init__(self, segmenter, batch_size, num_classes=None):
        self.segmenter, self.bs, self.num_classes = segmenter, max(1, int(batch_size)), num_classes
        self.x, self.l, self.hist = [], [], None

    def add(self, x, label):
        if tuple(label.shape[-2:]) != EVAL_SIZE:
            raise GccError('label map of %d x %d: the Cityscapes evaluation is defined at %d x %d' % (tuple(label.shape[-2:]) + EVAL_SIZE))
        self.x.append(x)
        self.l.append(label.reshape((1,) + EVAL_SIZE))
        if len(self.x) == self.bs:
            self.flush()

    def flush(self):
        if not self.x:
            return
        x = self.x[0] if len(self.x) == 1 else torch.cat(self.x)
        l = self.l[0] if len(self.l) == 1 else torch.cat(self.l)
        self.x, self.l = [], []
        with torch.no_grad():
            final = self.segmenter(x)[0]
        if self.num_classes is not None and final.shape[1] != self.num_classes:
            raise GccError('the segmenter returned %d classes, expected %d' % (final.shape[1], self.num_classes))
        self.hist = score(final.float(), l, self.hist)


def _prepare(segmenter, device):
    if hasattr(segmenter, 'to'):
        segmenter = segmenter.to(device)
    if hasattr(segmenter, 'eval'):
        segmenter.eval()
    return segmenter


def miou_of_fakes(fakes, names, segmenter, device, table_path, data_dir, batch_size=1, num_classes=NUM_CLASSES, cache=None):
    """metric/mIoU_score.py:196-218 test(): fakes[i] (uint8 [h, w, 3], host array or tensor) belongs to names[i]"""
    if len(fakes) != len(names):
        raise GccError('%d images against %d names' % (len(fakes), len(names)))
    cache = cache if cache is not None else LabelCache(data_dir, device)
    rels = label_list(names, table_path)
    cache.prefetch(rels)
    b = _Batcher(_prepare(segmenter, device), batch_size, num_classes)
    for fake, rel in zip(fakes, rels):
        fake = fake if torch.is_tensor(fake) else torch.from_numpy(np.ascontiguousarray(fake))
        b.add(seg_input(fake.to(device)), cache.get(rel))
    b.flush()
    if b.hist is None:
        raise GccError('mIoU of an empty image list')
    return miou(b.hist)


def _stem(path):
    return os.path.splitext(os.path.basename(path.replace('\\', '/')))[0]         # ntpath.basename + splitext, :71-72


class CityscapesScorer:
    """one evaluation: generated images (NHWC bf16 views, one at a time) in, the mIoU out.  ``cache``: the LabelCache of the
    run; ``segmenter`` is used as it is (see _prepare)."""

    def __init__(self, segmenter, dataroot, cache, batch_size=1):
        self.cache = cache
        self.table_path = os.path.join(str(dataroot), 'table.txt')
        self.table = read_table(self.table_path)
        self.batcher = _Batcher(segmenter, batch_size, NUM_CLASSES)
        self.seen = set()

    def label_file(self, path):
        return _match(_stem(path), self.table, self.table_path)

    def prefetch(self, paths):
        """every label of the split decoded up front, in parallel"""
        self.cache.prefetch([self.label_file(p) for p in dict.fromkeys(paths)])

    def add(self, path, fake):
        """fake: the generator's output for the image at ``path`` (read before this returns control to the stream: the view
        may be reused by the next inference).  The reference keys its images by path: a repeated one counts once."""
        if path in self.seen:
            return
        self.seen.add(path)
        self.batcher.add(seg_input(fake), self.cache.get(self.label_file(path)))

    def result(self):
        self.batcher.flush()
        if self.batcher.hist is None:
            raise GccError('Cityscapes evaluation: no image scored against %s' % self.table_path)
        return miou(self.batcher.hist)


def adopt_batch(data, stream):
    """order ``stream`` behind the producer of a loader's batch ('ready') and mark the batch's device tensors as used on it, so
    that the caching allocator does not hand their memory back to the loader's stream while kernels queued here still read
    them (models/_streams.py _note_input does the same for set_input)"""
    ev = data.get('ready')
    if ev is not None:
        stream.wait_event(ev)
    for t in data.values():
        if torch.is_tensor(t) and t.is_cuda:
            t.record_stream(stream)


def cityscapes_evaluator(segmenter, logger=None, batch_size=1):
    """evaluate(model, opt) for gcc_amd.train.run_evaluation: test_pix2pix_mIoU without the PNGs (python -m gcc_amd.test writes
    those, and scores the images it writes through ``evaluate.scorer``).  The label cache lives in the closure: the second and
    later evaluations of a run decode nothing."""
    state = {'segmenter': None, 'cache': None}

    def scorer(model, opt):
        if state['segmenter'] is None:
            state['segmenter'] = _prepare(segmenter, model.device)
            state['cache'] = LabelCache(opt.dataroot, model.device)
        return CityscapesScorer(state['segmenter'], opt.dataroot, state['cache'], batch_size)

    def evaluate(model, opt):
        from ..data import create_dataset
        from ..test import test_overrides
        topt = test_overrides(opt)
        dataset = create_dataset(topt, model.device)
        sc = scorer(model, topt)
        paths = getattr(dataset, 'paths', None)
        if paths is not None:
            sc.prefetch(paths)
        cur = torch.cuda.current_stream(model.device)
        for data in dataset:
            adopt_batch(data, cur)
            sc.add(data['A_paths'][0], model.infer_nhwc(data))
        value = sc.result()
        if logger is not None:
            logger.info('mIoU: %.2f' % value)
        return [(value, opt.direction)]

    evaluate.state = state
    evaluate.scorer = scorer
    return evaluate


PRECISION_ENV = 'GCC_DRN_PRECISION'


def builtin_segmenter(opt):
    """for a Pix2Pix run on a Cityscapes root (the callers' test, the reference's own: 'cityscapes' in --dataroot): (segmenter,
    None) when <dataroot>/table.txt exists and --drn_path is a TorchScript archive (the reference's DRNSeg exported with
    torch.jit) or the reference's own file, the plain state_dict of a DRNSeg over an arch-D DRN (drn_seg.DrnSegEngine, still on the
    host: the scorer moves it to the device); else (None, the condition that failed).  The environment variable
    GCC_DRN_PRECISION ('bf16', the default, or 'fp32': the reference's own arithmetic on the f32-input matrix instructions) chooses
    the precision of the engine built from a plain state_dict; any other value raises GccError.  A TorchScript archive runs as it
    was exported and ignores the variable."""
    root = str(opt.dataroot)
    if not os.path.isfile(os.path.join(root, 'table.txt')):
        return None, '%s holds no table.txt' % root
    path = getattr(opt, 'drn_path', None)
    if not path or not os.path.isfile(path):
        return None, '--drn_path %s does not exist' % path
    try:
        return torch.jit.load(path, map_location='cpu'), None
    except Exception as e:
        first = (str(e).strip().splitlines() or [type(e).__name__])[0]
        reason = 'torch.jit.load could not read --drn_path %s as a TorchScript archive (%s: %s); a plain state_dict needs ' \
                 'the network\'s code: export DRNSeg with torch.jit once' % (path, type(e).__name__, first)
    from .drn_seg import PRECISIONS, DrnSegEngine, is_drn_seg_state_dict
    try:
        sd = torch.load(path, map_location='cpu', weights_only=True)
    except Exception:
        return None, reason
    if not is_drn_seg_state_dict(sd):
        return None, reason
    precision = os.environ.get(PRECISION_ENV) or 'bf16'
    if precision not in PRECISIONS:
        raise GccError('%s=%s: expected one of %s' % (PRECISION_ENV, precision, ', '.join(PRECISIONS)))
    try:
        return DrnSegEngine(sd, precision=precision), None
    except GccError as e:
        return None, '--drn_path %s holds a DRNSeg state_dict this package does not run: %s' % (path, e)
