"""FID arithmetic on the GPU (metric/fid_score.py:150-214, 219-284, 327-328): activation statistics in f64 and the Frechet
distance with a Newton-Schulz matrix square root; and the reference's path-based half (:55-145, 287-322, 332-370): image folders,
statistics files and feature files scored against each other,

    python -m gcc_amd.metric.fid_score PATH PATH [--batch-size N] [--dims 64|192|768|2048] [-c GPU] [--prdc [--nearest-k 5]]
                                                 [--inception-score [--splits 10]]

prints ``FID: %.2f`` and, when both sides have activations (folders, or the feature files get_real_stat --features_path writes),
``KID: %.6f`` (gcc_amd.metric.kid_score); with --prdc one more line, ``Precision: %.4f | Recall: %.4f | Density: %.4f | Coverage:
%.4f`` (gcc_amd.metric.prdc_score) of the second path against the first as the real set; with --inception-score a last line,
``IS: %.4f +- %.4f`` (gcc_amd.metric.inception_score): the Inception Score of the second path, the generated set, from the native
network's 2048 features and the classifier of its weight file.  --dims below 2048 scores with the
reference's narrower output blocks (the native network stops there; unset, GCC_FID_DIMS or 2048).  No CPU path: a missing library / GPU
raises GccError."""
import argparse
import os

import numpy as np
import torch

from .. import ops
from .._lib import GccError, check

NEWTON_SCHULZ_ITERATIONS = 60       # each step is three d^3 f64 GEMMs; small eigenvalues converge linearly (x1.5 per step)
SHIFT_REL = 1e-13                   # delta / |s1 s2|_F of the two shifted solves (see csrc/metric.hip)


def _dev():
    if not torch.cuda.is_available():
        raise GccError('gcc_amd runs on MI355X only (no CPU path): need a visible GPU')
    return torch.device('cuda', torch.cuda.current_device())


def _f64(a, dev):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=torch.float64).contiguous()


def activation_statistics(act):
    """mu = np.mean(act, axis=0), sigma = np.cov(act, rowvar=False) (:327-328) of [n, d] activations (numpy or tensor,
    fp32 or f64) -> (mu [d], sigma [d, d]) f64 device tensors"""
    dev = _dev()
    t = act if torch.is_tensor(act) else torch.from_numpy(np.ascontiguousarray(act))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    t = t.to(dev).contiguous()
    n, d = t.shape
    mu = torch.empty(d, dtype=torch.float64, device=dev)
    sigma = torch.empty((d, d), dtype=torch.float64, device=dev)
    L = ops.lib()
    ws = torch.empty(L.gcc_activation_stats_workspace(n, d), dtype=torch.uint8, device=dev)
    check(L.gcc_activation_stats(t.data_ptr(), int(t.dtype == torch.float64), n, d, mu.data_ptr(), sigma.data_ptr(),
                                 ws.data_ptr(), ws.numel(), ops.stream()), 'gcc_activation_stats')
    return mu, sigma


class ActivationStream:
    """activation_statistics from batches (gcc_activation_stats_update / _finish: Chan et al.'s merge of centred moments in
    f64): ``update(act)`` queues two launches behind whatever produced ``act`` on the current stream and reads nothing back;
    ``result()`` -> (mu [d], sigma [d, d]) f64 device tensors.  The device holds d + d^2 doubles of state and a workspace of
    (max_batch + 1) d doubles, whatever the number of rows; the row count is a host integer."""

    def __init__(self, d, max_batch, device=None):
        self.d, self.max_batch, self.n = int(d), int(max_batch), 0
        if self.d <= 0 or self.max_batch <= 0:
            raise GccError('ActivationStream: d and max_batch must be positive, got %d and %d' % (self.d, self.max_batch))
        self.device = torch.device(device) if device is not None else _dev()
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.mean = torch.empty(self.d, dtype=torch.float64, device=self.device)
        self.m2 = torch.empty((self.d, self.d), dtype=torch.float64, device=self.device)
        self.ws = torch.empty(ops.lib().gcc_activation_stats_stream_workspace(self.max_batch, self.d), dtype=torch.uint8,
                              device=self.device)

    def update(self, act):
        """act: [b, d] or [b, d, 1, 1], fp32 or f64, on the stream's device, 1 <= b <= max_batch; rows may be strided (read
        in place), elements of a row may not"""
        if act.dim() == 4 and act.shape[2] == 1 and act.shape[3] == 1:
            act = act[:, :, 0, 0]
        if act.dim() != 2 or act.shape[1] != self.d or act.dtype not in (torch.float32, torch.float64) or \
                act.device != self.device:
            raise GccError('ActivationStream.update: expected fp32 / f64 activations [b, %d] on %s, got %s %s on %s'
                           % (self.d, self.device, act.dtype, tuple(act.shape), act.device))
        b = act.shape[0]
        if not 1 <= b <= self.max_batch:
            raise GccError('ActivationStream.update: %d rows, the stream was made for 1..%d' % (b, self.max_batch))
        if (self.d > 1 and act.stride(1) != 1) or (b > 1 and act.stride(0) < self.d):
            act = act.contiguous()
        ld = act.stride(0) if b > 1 else self.d
        check(ops.lib().gcc_activation_stats_update(act.data_ptr(), int(act.dtype == torch.float64), ld, b, self.d, self.n,
                                                    self.mean.data_ptr(), self.m2.data_ptr(), self.ws.data_ptr(),
                                                    self.ws.numel(), ops.stream()), 'gcc_activation_stats_update')
        self.n += b
        return self

    def result(self):
        if self.n < 2:
            raise GccError('ActivationStream.result: a covariance needs at least 2 rows, %d were given' % self.n)
        sigma = torch.empty_like(self.m2)
        check(ops.lib().gcc_activation_stats_finish(self.m2.data_ptr(), self.n, self.d, sigma.data_ptr(), ops.stream()),
              'gcc_activation_stats_finish')
        return self.mean, sigma


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6, iterations=None, return_residual=False):
    """metric/fid_score.py:219-284: d^2 = |mu1 - mu2|^2 + Tr(C1 + C2 - 2 sqrt(C1 C2)).  The reference retries with
    eps * I added to both covariances when scipy's sqrtm returns non-finite entries; here that happens when the
    iteration has not produced a finite trace."""
    dev = _dev()
    mu1, mu2 = _f64(np.atleast_1d(mu1) if not torch.is_tensor(mu1) else mu1, dev), _f64(
        np.atleast_1d(mu2) if not torch.is_tensor(mu2) else mu2, dev)
    sigma1, sigma2 = _f64(np.atleast_2d(sigma1) if not torch.is_tensor(sigma1) else sigma1, dev), _f64(
        np.atleast_2d(sigma2) if not torch.is_tensor(sigma2) else sigma2, dev)
    assert mu1.shape == mu2.shape, 'Training and test mean vectors have different lengths'
    assert sigma1.shape == sigma2.shape, 'Training and test covariances have different dimensions'
    d = mu1.numel()
    L = ops.lib()
    ws = torch.empty(L.gcc_frechet_workspace(d), dtype=torch.uint8, device=dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)

    def run(s1, s2):
        check(L.gcc_frechet_distance(mu1.data_ptr(), s1.data_ptr(), mu2.data_ptr(), s2.data_ptr(), d,
                                     int(iterations or NEWTON_SCHULZ_ITERATIONS), SHIFT_REL, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                     ops.stream()), 'gcc_frechet_distance')
        return out.cpu().numpy()
    val = run(sigma1, sigma2)
    if not np.isfinite(val).all():
        print('fid calculation produces singular product; adding %s to diagonal of cov estimates' % eps)
        off = torch.eye(d, dtype=torch.float64, device=dev) * eps
        val = run(sigma1 + off, sigma2 + off)
    return (float(val[0]), float(val[1])) if return_residual else float(val[0])


def get_activations_from_ims(ims, model, batch_size=50, dims=2048, device=None, verbose=False, use_tqdm=True):
    """metric/fid_score.py:150-214: ``model(batch)[0]`` on [0, 1] NCHW batches, global average pooling if the map is not
    1x1; the activations stay on the device (f32)."""
    if hasattr(model, 'eval'):
        model.eval()
    n = len(ims)
    out = []
    for start in range(0, n, batch_size):
        images = np.array(ims[start:start + batch_size], dtype=np.float64)
        if images.shape[1] != 3:
            images = images.transpose((0, 3, 1, 2))
        images = images / 255
        batch = torch.from_numpy(images).type(torch.FloatTensor).to(device)
        with torch.no_grad():
            pred = model(batch)[0]
        if pred.shape[2] != 1 or pred.shape[3] != 1:
            pred = pred.mean((2, 3), keepdim=True)
        out.append(pred.reshape(pred.shape[0], -1).float())
    return torch.cat(out, 0)


def _compute_statistics_of_ims(ims, model, batch_size, dims, device, use_tqdm=True):
    act = get_activations_from_ims(ims, model, batch_size, dims, device, verbose=False, use_tqdm=use_tqdm)
    return activation_statistics(act)


# ---- the path-based half of metric/fid_score.py (:55-145, 287-322, 332-370) ---------------------------------------------------
DIMS = (64, 192, 768, 2048)         # metric/inception.py BLOCK_INDEX_BY_DIM: the widths the reference's --dims accepts

parser = argparse.ArgumentParser(prog='python -m gcc_amd.metric.fid_score', formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                 description='FID (and KID, when both sides have activations) of two image sets')
parser.add_argument('path', type=str, nargs=2,
                    help='two of: a folder of *.jpg / *.png images, a real_stat*.npz statistics file (mu, sigma), '
                         'a real_act*.npz feature file (get_real_stat --features_path)')
parser.add_argument('--batch-size', type=int, default=50, help='images per pass of the network')
parser.add_argument('--dims', type=int, default=2048, choices=list(DIMS),
                    help='width of the network\'s features: the output block the native network is tapped at (not given: '
                         'GCC_FID_DIMS, else the default)')
parser.add_argument('-c', '--gpu', default='', type=str, help='index of the GPU to use (blank: the current device; there is no CPU path)')
parser.add_argument('--prdc', action='store_true',
                    help='also print precision, recall, density and coverage (gcc_amd.metric.prdc_score) of the second path '
                         'against the first as the real set; both sides need activations: folders or real_act*.npz')
parser.add_argument('--nearest-k', type=int, default=5, help='the k of the nearest-neighbour balls of --prdc')
parser.add_argument('--inception-score', action='store_true',
                    help='also print the Inception Score (gcc_amd.metric.inception_score) of the second path, the generated set: '
                         'it needs activations (a folder or a real_act*.npz), --dims 2048 and the native network with its classifier')
parser.add_argument('--splits', type=int, default=10, help='the number of splits of --inception-score')


def list_image_files(path):
    """the *.jpg and *.png files of a folder (metric/fid_score.py:318-319), sorted by name: the reference takes them in
    directory order, which decides nothing but which images a partial last batch drops"""
    names = [f for f in os.listdir(str(path)) if os.path.splitext(f)[1] in ('.jpg', '.png') and os.path.isfile(os.path.join(str(path), f))]
    return [os.path.join(str(path), f) for f in sorted(names)]


def batch_plan(n_files, batch_size, warn=print):
    """(batch size, number of batches) of get_activations (:92-102): the batch size is clamped to the file count, a partial last
    batch is dropped, each with the reference's warning"""
    batch_size = int(batch_size)
    if n_files < 1 or batch_size < 1:
        raise GccError('get_activations: %d files at batch size %d' % (n_files, batch_size))
    if n_files % batch_size != 0:
        warn('Warning: number of images is not a multiple of the batch size. Some samples are going to be ignored.')
    if batch_size > n_files:
        warn('Warning: batch size is bigger than the datasets size. Setting batch size to datasets size')
        batch_size = n_files
    return batch_size, n_files // batch_size


def _cuda_device(cuda):
    if not cuda:
        raise GccError('gcc_amd runs on MI355X only (no CPU path): cuda must be set')
    return cuda if isinstance(cuda, torch.device) else _dev()


def _activation_batches(files, model, batch_size, dims, cuda, verbose=False):
    """the [b, dims] fp32 device activations of get_activations, one batch at a time"""
    from PIL import Image
    from .fid_eval import fid_input
    dev = _cuda_device(cuda)
    if hasattr(model, 'eval'):
        model.eval()
    files = [str(f) for f in files]
    batch_size, n_batches = batch_plan(len(files), batch_size)
    size = None
    for i in range(n_batches):
        if verbose:
            print('\rPropagating batch %d/%d' % (i + 1, n_batches), end='', flush=True)
        images = []
        for f in files[i * batch_size:(i + 1) * batch_size]:
            with Image.open(f) as im:
                a = np.asarray(im.convert('RGB'), dtype=np.uint8)
            size = size or a.shape
            if a.shape != size:
                raise GccError('get_activations: %s is %d x %d, the images before it %d x %d: the images of one call share a size'
                               % (f, a.shape[1], a.shape[0], size[1], size[0]))
            images.append(a)
        batch = fid_input(torch.from_numpy(np.stack(images)).to(dev))
        with torch.no_grad():
            pred = model(batch)[0]
        if not torch.is_tensor(pred) or pred.dim() != 4 or pred.dtype != torch.float32 or pred.shape[0] != batch.shape[0]:
            raise GccError('the Inception network must return [N, d, h, w] fp32 activations as element 0, got %s'
                           % ('%s %s' % (pred.dtype, tuple(pred.shape)) if torch.is_tensor(pred) else type(pred).__name__))
        if pred.shape[1] != dims:
            raise GccError('the network\'s activations have d = %d, dims = %d was asked for' % (pred.shape[1], dims))
        if pred.shape[2] != 1 or pred.shape[3] != 1:
            pred = pred.mean((2, 3), keepdim=True)
        yield pred.reshape(pred.shape[0], -1)
    if verbose:
        print(' done')


def get_activations(files, model, batch_size=50, dims=2048, cuda=True, verbose=False, use_tqdm=False):
    """metric/fid_score.py:69-145: the network's activations of image files, [n_used, dims] fp32, on the device.  The files are
    decoded on the host (PIL, as RGB), go to the device as bytes and become the network's input through gcc_fid_input: byte /
    255, the reference's imread(f).astype(float32) / 255.  As there, the batch size is clamped to the file count and a
    partial last batch is dropped, each with its warning.  The images of one call must share a size (GccError names the file
    that does not).  One difference: the reference decodes with cv2, which hands the network blue first; this decodes as RGB,
    the order every other route of this package (and the real statistics) feeds."""
    return torch.cat(list(_activation_batches(files, model, batch_size, dims, cuda, verbose)), 0)


def calculate_activation_statistics(files, model, batch_size=50, dims=2048, cuda=True, verbose=False, use_tqdm=False, store=None):
    """metric/fid_score.py:287-309 through ActivationStream: (mu [dims], sigma [dims, dims]) f64 device tensors of the files'
    activations, batch by batch; ``store``: a kid_score.FeatureStore that receives the same activations"""
    stream = None
    for act in _activation_batches(files, model, batch_size, dims, cuda, verbose):
        if stream is None:
            stream = ActivationStream(act.shape[1], act.shape[0], act.device)
        stream.update(act)
        if store is not None:
            store.append(act)
    return stream.result()


def _statistics_of_features(act, batch=512):
    stream = ActivationStream(act.shape[1], min(batch, act.shape[0]), act.device)
    for s in range(0, act.shape[0], batch):
        stream.update(act[s:s + batch])
    return stream.result()


def _path_statistics(path, model, batch_size, dims, cuda):
    """(mu, sigma, activations or None) of a folder, a statistics file or a feature file; ``model``: a callable that returns the
    network, called only when a folder has to be scored"""
    from . import kid_score
    path = str(path)
    if path.endswith('.npz'):
        if kid_score.is_features_file(path):
            act, _ = kid_score.load_features(path, dims, _cuda_device(cuda))
            return _statistics_of_features(act) + (act,)
        with np.load(path) as f:
            return f['mu'][:], f['sigma'][:], None
    files = list_image_files(path)
    if not files:
        raise GccError('%s holds no *.jpg or *.png file' % path)
    store = kid_score.FeatureStore(dims, _cuda_device(cuda))
    mu, sigma = calculate_activation_statistics(files, model(), batch_size, dims, cuda, store=store)
    return mu, sigma, store.rows()


def _compute_statistics_of_path(path, model, batch_size, dims, cuda, use_tqdm=False):
    """metric/fid_score.py:312-322: mu / sigma of a .npz as they are stored, else of the folder's *.jpg + *.png"""
    return _path_statistics(path, lambda: model, batch_size, dims, cuda)[:2]


def _network(model, dims, cuda):
    """a callable that returns the scoring network on the device: ``model``, or the file GCC_FID_INCEPTION names (loaded on the
    first call, at the precision GCC_FID_PRECISION names and tapped at the output block of ``dims`` features)"""
    state = {}

    def get():
        if 'net' not in state:
            from .cityscapes import _prepare
            from .fid_eval import load_inception
            net = model
            if net is None:
                net, why = load_inception(dims)
                if net is None:
                    raise GccError('fid_score: %s' % why)
            state['net'] = _prepare(net, _cuda_device(cuda))
        return state['net']
    return get


def calculate_fid_given_ims(ims_fake, ims_real, batch_size, cuda, dims, model=None, use_tqdm=False):
    """metric/fid_score.py:332-347; ``model`` None: the network GCC_FID_INCEPTION names.  A network whose activations are not
    ``dims`` wide is a GccError."""
    net = _network(model, dims, cuda)()
    dev = _cuda_device(cuda)
    stats = []
    for ims in (ims_fake, ims_real):
        act = get_activations_from_ims(ims, net, batch_size, dims, dev, use_tqdm=use_tqdm)
        if act.shape[1] != dims:
            raise GccError('the network\'s activations have d = %d, dims = %d was asked for' % (act.shape[1], dims))
        stats.append(activation_statistics(act))
    return calculate_frechet_distance(*stats[0], *stats[1])


def _classifier_for(paths, dims, net, splits):
    """the (weight, bias) --inception-score scores the second path with, after the three things it needs: 2048 features, a second
    path that has activations, a native network with its classifier; each failing case is a GccError that says which it is"""
    from . import inception_score, kid_score
    if dims != inception_score.DIMS:
        raise GccError('fid_score --inception-score: --dims %d; the classifier reads the %d pool features: score with --dims %d '
                       '(or without --dims and GCC_FID_DIMS)' % (dims, inception_score.DIMS, inception_score.DIMS))
    second = str(paths[1])
    if second.endswith('.npz') and not kid_score.is_features_file(second):
        raise GccError('fid_score --inception-score: %s holds statistics (mu, sigma) only; the Inception Score needs the '
                       'activations: a folder of images or a real_act*.npz (get_real_stat --features_path)' % second)
    inception_score.check_splits(splits, '--splits')
    return inception_score.classifier_of(net(), 'fid_score --inception-score')


def calculate_fid_given_paths(paths, batch_size, cuda, dims, model=None, use_tqdm=False, kid=False, prdc_k=None, is_splits=None):
    """metric/fid_score.py:350-370: the FID of two paths, each a folder of images, a real_stat*.npz or a real_act*.npz feature
    file.  ``kid``: return (FID, KID) instead, KID None unless both sides have activations (folders or feature files).
    ``prdc_k``: return (FID, KID, prdc_score.prdc(first, second, k)) -- the first path is the real set, as the FID's arguments
    are ordered; a side without activations is a GccError that names it.  ``is_splits``: one more element at the end of the
    tuple (behind the FID alone: a pair), the (mean, std) of inception_score.inception_score of the second path's activations
    over that many splits."""
    for p in paths:
        if not os.path.exists(str(p)):
            raise RuntimeError('Invalid path: %s' % p)
    net = _network(model, dims, cuda)
    classifier = _classifier_for(paths, dims, net, is_splits) if is_splits is not None else None
    values = _fid_kid_prdc(paths, batch_size, cuda, dims, net, kid, prdc_k)
    if classifier is None:
        return values[0]
    from .inception_score import inception_score
    score = inception_score(values[1], *classifier, splits=is_splits)
    return (values[0] if isinstance(values[0], tuple) else (values[0],)) + (score,)


def _fid_kid_prdc(paths, batch_size, cuda, dims, net, kid, prdc_k):
    """(what calculate_fid_given_paths returns without is_splits, the second path's activations or None)"""
    (m1, s1, a1), (m2, s2, a2) = (_path_statistics(p, net, batch_size, dims, cuda) for p in paths[:2])
    if tuple(m1.shape) != (dims,) or tuple(m2.shape) != (dims,):
        raise GccError('the statistics have mu %s and %s, dims = %d was asked for' % (tuple(m1.shape), tuple(m2.shape), dims))
    if prdc_k is not None:
        for p, a in zip(paths[:2], (a1, a2)):
            if a is None:
                raise GccError('fid_score --prdc: %s holds statistics (mu, sigma) only; precision / recall / density / coverage '
                               'need the activations: a folder of images or a real_act*.npz (get_real_stat --features_path)' % p)
    fid_value = calculate_frechet_distance(m1, s1, m2, s2)
    if not kid and prdc_k is None:
        return fid_value, a2
    from .kid_score import polynomial_mmd2
    kid_value = polynomial_mmd2(a1, a2) if a1 is not None and a2 is not None else None
    if prdc_k is None:
        return (fid_value, kid_value), a2
    from .prdc_score import prdc
    return (fid_value, kid_value, prdc(a1, a2, prdc_k)), a2


def main(argv=None, model=None):
    args = parser.parse_args(argv, argparse.Namespace(dims=None))       # None: --dims was not given, GCC_FID_DIMS may speak
    if not torch.cuda.is_available():
        raise GccError('gcc_amd runs on MI355X only (no CPU path): need a visible GPU')
    if args.gpu != '':
        torch.cuda.set_device(int(args.gpu))
    prdc_k = None
    if args.prdc:
        from .prdc_score import check_k, prdc_text
        prdc_k = check_k(args.nearest_k, '--nearest-k')
    is_splits = None
    if args.inception_score:
        from .inception_score import check_splits, is_text
        is_splits = check_splits(args.splits, '--splits')
    from .fid_eval import fid_dims
    values = calculate_fid_given_paths(args.path, args.batch_size, True, fid_dims(args.dims), model=model, kid=True, prdc_k=prdc_k,
                                       is_splits=is_splits)
    fid_value, kid_value = values[:2]
    print('FID: %.2f' % fid_value)
    if kid_value is not None:
        print('KID: %.6f' % kid_value)
    if prdc_k is not None:
        print(prdc_text(values[2]))
    if is_splits is not None:
        print(is_text(values[-1]))
    return values


if __name__ == '__main__':
    main()
