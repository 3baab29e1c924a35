"""FID of a Pix2Pix (any root but Cityscapes), CycleGAN or SAGAN generator (metric/test_metric.py:15-45 test_pix2pix_fid, 129-161
test_sagan_fid, 163-204 test_cyclegan_fid): everything around the Inception network.  The network stays an external input, as
DRN does for the Cityscapes mIoU: ``GCC_FID_INCEPTION`` names the reference's own weight file (the plain state_dict of
fid_inception_v3(), run natively by inception_fid.InceptionFidEngine) or a TorchScript archive of the reference's InceptionV3([3])
(exported once with torch.jit where its weights live); fid_evaluator takes any callable with its contract -- NCHW fp32 in [0, 1] at the generator's
resolution in (resizing and normalisation are the network's own), element 0 of the result [N, d, h, w] fp32 out, averaged over
(h, w) when not 1 x 1.

    generator (model.infer_nhwc) -> gcc_fid_input (util.tensor2imgs' byte / 255) into slot k of a persistent batch buffer
        -> inception(batch)[0] when the buffer is full (and once for the remainder) -> gcc_activation_stats_update
        -> gcc_activation_stats_finish -> gcc_frechet_distance against real_stat*.npz -> one host read

Nothing is read back before that last step, and the device holds d^2 doubles of statistics whatever the number of images.

With a feature file real_act*.npz beside every real_stat*.npz the evaluation needs (python -m gcc_amd.metric.get_real_stat
--features_path), the activations are also kept (kid_score.FeatureStore) and a ``KID: %.6f`` line follows the FID line: the
Kernel Inception Distance (kid_score.polynomial_mmd2), three gcc_kid_poly_sum calls per slot, the real set's self term once
per run.  Checkpoints are still chosen by FID alone.  Without the files nothing is stored, launched or logged for it.

``GCC_FID_PRDC=<k>`` (1..GCC_PRDC_MAX_K; unset, empty or 0: off) adds one more line after the KID line: ``Precision: %.4f |
Recall: %.4f | Density: %.4f | Coverage: %.4f`` of the same activations (prdc_score.prdc with k nearest neighbours), the real
set's radii computed once per run.  It needs the feature files: with the variable set and one missing, the scorer raises.

``GCC_FID_IS=<splits>`` (an integer >= 1, usually 10; unset or empty: off) adds a last line, ``IS: %.4f +- %.4f``: the Inception
Score of the generated images (inception_score.inception_score: mean and standard deviation over that many splits) from the same
pool features and the classifier of the native network's weight file.  It needs no real set, so the activations are kept for it
also where no feature file exists.  A network without the classifier -- a TorchScript archive, a weight file without fc.*, a
width below 2048 -- is refused when the scorer is made, before any image is generated.

``GCC_FID_DIMS=<64 | 192 | 768 | 2048>`` (unset or empty: 2048) scores with the reference's narrower output blocks
(metric/inception.py BLOCK_INDEX_BY_DIM, the --dims of metric/fid_score.py): the native network stops after that block and its map
is averaged to 1 x 1 by gcc_map_mean.  With fewer images than features the covariance is rank deficient; a lower width is the
original FID code's own remedy.  The real statistics must be of the same width (get_real_stat --dims).

The one deliberate difference from the reference: it runs Inception at batch 1 (its evaluations set opt.batch_size = 1); this
evaluator batches up to 50 images (get_activations' own default).  An eval-mode network's output for an image does not depend on
its batch neighbours, so the activations are those of the batch-1 run up to the network's own batched arithmetic."""
import os
import warnings

import numpy as np
import torch

from .. import ops
from .._lib import FID_IN_BF16, FID_IN_F32, FID_IN_U8, GccError, check
from .cityscapes import _prepare, adopt_batch
from .fid_score import ActivationStream, calculate_frechet_distance

ENV = 'GCC_FID_INCEPTION'
SAGAN_FRACTION = 0.1              # metric/test_metric.py:144


def wants_fid(opt):
    """the reference's evaluation cases that need FID (train.py:14-73): Pix2Pix off Cityscapes, CycleGAN, SAGAN"""
    if opt.model == 'pix2pix':
        return 'cityscapes' not in str(opt.dataroot)
    return 'cyclegan' in opt.model or opt.model == 'sagan'


def real_stat_slots(opt):
    """[(npz file under --dataroot, slot tag)] in the slot order of train.py:14-73"""
    if 'cyclegan' in opt.model:
        return [('real_stat_B.npz', 'AtoB'), ('real_stat_A.npz', 'BtoA')]
    if opt.model == 'sagan':
        return [('real_stat.npz', opt.direction)]
    return [('real_stat_B.npz' if opt.direction == 'AtoB' else 'real_stat_A.npz', opt.direction)]


def sagan_stops(i, length):
    """metric/test_metric.py:144 as it stands (Python float arithmetic): batch i is not scored, nor any after it"""
    return i > length * SAGAN_FRACTION


def sagan_count(length):
    """the number of batches test_sagan_fid scores out of ``length``"""
    i = 0
    while i < length and not sagan_stops(i, length):
        i += 1
    return i


def fid_input(image, out=None):
    """the network's input (NCHW fp32 [N, 3, H, W] in [0, 1]) through gcc_fid_input: of an NHWC bf16 activation view (a
    generator's output), a uint8 [N, H, W, 3] device tensor, or an NCHW fp32 device tensor in [-1, 1] (a loader's image); the
    byte of util.tensor2imgs over 255.  ``out``: a contiguous fp32 [N, 3, H, W] device tensor, e.g. a slot of a batch buffer.
    An NHWC fp32 activation view (a generator's fp32 route: channels innermost in a pixel stride of at least 4) becomes its
    bytes first (gcc_image_to_u8_f32) and goes on as uint8."""
    if image.dtype == torch.float32 and image.dim() == 4 and image.stride(1) == 1 and image.stride(3) >= 4:
        image = ops.image_to_u8(image)
    if image.dtype == torch.uint8:
        if image.dim() == 3:
            image = image[None]
        image = image.contiguous()
        N, H, W, c3 = image.shape
        ptr, form, ld = image.data_ptr(), FID_IN_U8, 0
    elif image.dtype == torch.bfloat16:
        ptr, N, c3, H, W, ld = ops.geom(image)
        form = FID_IN_BF16
    elif image.dtype == torch.float32 and image.dim() == 4:
        image = image.contiguous()
        N, c3, H, W = image.shape
        ptr, form, ld = image.data_ptr(), FID_IN_F32, 0
    else:
        raise GccError('fid_input: expected an NHWC bf16 view, uint8 [N, H, W, 3] or NCHW fp32, got %s %s'
                       % (image.dtype, tuple(image.shape)))
    if c3 != 3 or not image.is_cuda:
        raise GccError('fid_input: expected 3-channel images on the device, got %s on %s' % (tuple(image.shape), image.device))
    if out is None:
        out = torch.empty((N, 3, H, W), dtype=torch.float32, device=image.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (N, 3, H, W) or not out.is_contiguous() or out.device != image.device:
        raise GccError('fid_input: out must be a contiguous fp32 [%d, 3, %d, %d] tensor on the image\'s device' % (N, H, W))
    check(ops.lib().gcc_fid_input(ptr, form, ld, 0, N, H, W, out.data_ptr(), ops.stream()), 'gcc_fid_input')
    return out


class ImageStatistics:
    """images in (one at a time, keyed), the Inception statistics of the distinct keys out.  The images wait in a persistent
    [batch_size, 3, H, W] buffer; a full buffer (and the remainder at the end) goes through the network and into the streamed
    statistics, all on the current stream."""

    def __init__(self, inception, batch_size=50, keep_features=False):
        self.inception, self.bs = inception, max(1, int(batch_size))
        self.buf, self.k, self.seen, self.stream = None, 0, set(), None
        self.keep_features, self.features = bool(keep_features), None      # a kid_score.FeatureStore, only when asked

    @property
    def count(self):
        return len(self.seen)

    def add(self, key, image):
        """image: one image in any form fid_input takes (read before this returns control to the stream: a generator's view
        may be reused by its next inference).  The reference keeps its images in a dict: a repeated key counts once."""
        if key in self.seen:
            return
        self.seen.add(key)
        if self.buf is None:
            H, W = image.shape[-3:-1] if image.dtype == torch.uint8 else image.shape[-2:]       # [.., H, W, 3] | [N, 3, H, W]
            self.buf = torch.empty((self.bs, 3, int(H), int(W)), dtype=torch.float32, device=image.device)
        fid_input(image, self.buf[self.k:self.k + 1])
        self.k += 1
        if self.k == self.bs:
            self.flush()

    def flush(self):
        if not self.k:
            return
        with torch.no_grad():
            pred = self.inception(self.buf[:self.k])[0]
        if not torch.is_tensor(pred) or pred.dim() != 4 or pred.dtype != torch.float32 or pred.shape[0] != self.k:
            raise GccError('the Inception network must return [N, d, h, w] fp32 activations as element 0, got %s'
                           % ('%s %s' % (pred.dtype, tuple(pred.shape)) if torch.is_tensor(pred) else type(pred).__name__))
        if pred.shape[2] != 1 or pred.shape[3] != 1:
            pred = pred.mean((2, 3), keepdim=True)                  # metric/fid_score.py:205-206
        if self.stream is None:
            self.stream = ActivationStream(pred.shape[1], self.bs, pred.device)
        self.stream.update(pred)
        if self.keep_features:
            if self.features is None:
                from .kid_score import FeatureStore
                self.features = FeatureStore(pred.shape[1], pred.device)
            self.features.append(pred)
        self.k = 0

    def result(self):
        """(mu [d], sigma [d, d]) f64 device tensors"""
        if self.count < 2:
            raise GccError('FID statistics need at least 2 images, %d were scored' % self.count)
        self.flush()
        return self.stream.result()


def load_real_stat(path, d, device):
    """mu [d], sigma [d, d] of a real_stat*.npz as f64 device tensors"""
    with np.load(path) as z:
        mu, sigma = np.asarray(z['mu']), np.asarray(z['sigma'])
    if mu.shape != (d,) or sigma.shape != (d, d):
        raise GccError('%s holds mu %s and sigma %s; the network\'s activations have d = %d (python -m '
                       'gcc_amd.metric.get_real_stat --dims %d --dataroot ... --output_path %s writes statistics of that width)'
                       % (path, mu.shape, sigma.shape, d, d, path))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)
    return f(mu), f(sigma)


class FidScorer:
    """one evaluation: generated images in (per slot), one FID per slot out -- and one KID per slot (``kid()``) when a feature
    file real_act*.npz (get_real_stat --features_path) lies beside every slot's real_stat*.npz; with one missing, no activation
    is kept and nothing is launched for it.  ``kid_cache``: a dict that outlives the scorer (the evaluator's): the real sets'
    activations and self terms are loaded and computed once per run.  ``is_splits`` (GCC_FID_IS): the activations are kept
    whether or not the feature files exist, and ``inception_score()`` gives one (mean, std) per slot; the network must carry
    its classifier (inception_score.classifier_of says what is missing otherwise)."""

    def __init__(self, inception, dataroot, slots, batch_size=50, kid_cache=None, prdc_k=None, is_splits=None):
        from .kid_score import features_name
        from .prdc_score import ENV as PRDC_ENV, check_k
        self.files = [os.path.join(str(dataroot), name) for name, _ in slots]
        self.tags = [tag for _, tag in slots]
        self.feature_files = [features_name(f) for f in self.files]
        self.with_kid = bool(slots) and all(f is not None and os.path.isfile(f) for f in self.feature_files)
        self.prdc_k = None if prdc_k is None else check_k(prdc_k, PRDC_ENV)
        if self.prdc_k is not None and not self.with_kid:
            missing = [(f, s) for f, s in zip(self.feature_files, self.files) if f is None or not os.path.isfile(f)]
            raise GccError('%s=%d needs the real activations of every slot: %s missing (python -m gcc_amd.metric.get_real_stat '
                           '--dataroot ... --output_path %s --features_path %s writes it)'
                           % (PRDC_ENV, self.prdc_k, ', '.join(str(f or s) for f, s in missing), missing[0][1],
                              missing[0][0] or 'real_act*.npz'))
        self.is_splits, self.classifier = None, None
        if is_splits is not None:
            from . import inception_score as IS
            self.is_splits = IS.check_splits(is_splits, IS.ENV)
            self.classifier = IS.classifier_of(inception, '%s=%d' % (IS.ENV, self.is_splits))
        self.kid_cache = kid_cache if kid_cache is not None else {}
        self.label = network_label(inception)
        keep = self.with_kid or self.is_splits is not None
        self.stats = [ImageStatistics(inception, batch_size, keep_features=keep) for _ in slots]

    def add(self, key, fake, slot=0):
        self.stats[slot].add(key, fake)

    def result(self):
        values = []
        for path, st in zip(self.files, self.stats):
            mu, sigma = st.result()
            m1, s1 = load_real_stat(path, mu.numel(), mu.device)
            values.append(float(calculate_frechet_distance(m1, s1, mu, sigma)))         # metric/__init__.py:8-14
        return values

    def _real_features(self, path, d, device):
        """(activations, self term) of a feature file, from the cache after the first evaluation of a run"""
        from . import kid_score
        if path not in self.kid_cache:
            act, label = kid_score.load_features(path, d, device)
            if label != self.label and not self.kid_cache.get('warned'):
                self.kid_cache['warned'] = True
                warnings.warn('%s was written with the Inception network%s, this evaluation scores with the network%s: KID '
                              'compares activations of two networks' % (path, label or ' (TorchScript)', self.label or ' (TorchScript)'))
            self.kid_cache[path] = (act, kid_score.polynomial_self_sum(act))
        return self.kid_cache[path]

    def kid(self):
        """one Kernel Inception Distance per slot (real set first, as the FID's arguments), or None when a slot has no feature
        file"""
        if not self.with_kid:
            return None
        from .kid_score import polynomial_mmd2
        values = []
        for path, st in zip(self.feature_files, self.stats):
            if st.count < 2:
                raise GccError('KID needs at least 2 images, %d were scored' % st.count)
            st.flush()
            fake = st.features.rows()
            real, real_self = self._real_features(path, fake.shape[1], fake.device)
            values.append(polynomial_mmd2(real, fake, self_x=real_self))
        return values

    def prdc(self):
        """one {'precision', 'recall', 'density', 'coverage'} per slot at the scorer's k, or None when it was made without one.
        The real set's radii are computed on the first evaluation of a run and kept beside its KID self term."""
        if self.prdc_k is None:
            return None
        from . import prdc_score
        values = []
        for path, st in zip(self.feature_files, self.stats):
            if st.count <= self.prdc_k:
                raise GccError('precision / recall / density / coverage with k = %d need more than k images, %d were scored'
                               % (self.prdc_k, st.count))
            st.flush()
            fake = st.features.rows()
            real, _ = self._real_features(path, fake.shape[1], fake.device)
            key = (path, 'radii', self.prdc_k)
            if key not in self.kid_cache:
                self.kid_cache[key] = prdc_score.nearest_radii(real, self.prdc_k)
            values.append(prdc_score.prdc(real, fake, self.prdc_k, real_radii=self.kid_cache[key]))
        return values


    def inception_score(self):
        """one Inception Score (mean, std) per slot over the scorer's splits, or None when it was made without them"""
        if self.is_splits is None:
            return None
        from . import inception_score as IS
        values = []
        for st in self.stats:
            if st.count < self.is_splits:
                raise GccError('the Inception Score over %d splits needs at least %d images, %d were scored'
                               % (self.is_splits, self.is_splits, st.count))
            st.flush()
            values.append(IS.inception_score(st.features.rows(), *self.classifier, splits=self.is_splits))
        return values


def fid_line(values, tags, model):
    if 'cyclegan' in model:
        return ' | '.join('%s FID: %.2f' % (t, v) for v, t in zip(values, tags))
    return 'FID: %.2f' % values[0]


def kid_line(values, tags, model):
    if 'cyclegan' in model:
        return ' | '.join('%s KID: %.6f' % (t, v) for v, t in zip(values, tags))
    return 'KID: %.6f' % values[0]


def prdc_line(values, tags, model):
    from .prdc_score import prdc_text
    if 'cyclegan' in model:
        return ' | '.join('%s %s' % (t, prdc_text(v)) for v, t in zip(values, tags))
    return prdc_text(values[0])


def is_line(values, tags, model):
    from .inception_score import is_text
    if 'cyclegan' in model:
        return ' | '.join('%s %s' % (t, is_text(v)) for v, t in zip(values, tags))
    return is_text(values[0])


def fid_evaluator(inception, logger=None, batch_size=50):
    """evaluate(model, opt) for gcc_amd.train.run_evaluation: test_pix2pix_fid / test_cyclegan_fid / test_sagan_fid.
    ``evaluate.scorer(model, opt)`` gives python -m gcc_amd.test the scorer of the images it writes.  Inception runs on batches
    of up to ``batch_size`` images where the reference runs it at batch 1: the one deliberate difference (see the module)."""
    state = {'inception': None, 'kid': {}}

    def scorer(model, opt):
        if state['inception'] is None:
            state['inception'] = _prepare(inception, model.device)
        from .inception_score import env_splits
        from .prdc_score import env_k
        return FidScorer(state['inception'], opt.dataroot, real_stat_slots(opt), batch_size, kid_cache=state['kid'], prdc_k=env_k(),
                         is_splits=env_splits())

    def evaluate(model, opt):
        from ..data import create_dataset
        from ..test import test_overrides
        topt = test_overrides(opt)
        dataset = create_dataset(topt, model.device)
        dataset.shard = False                      # an evaluation walks the whole split on whichever rank runs it
        sc = scorer(model, topt)
        cur = torch.cuda.current_stream(model.device)
        length = len(dataset) if opt.model == 'sagan' else 0
        for i, data in enumerate(dataset):
            if opt.model == 'sagan' and sagan_stops(i, length):
                break
            adopt_batch(data, cur)
            if opt.model == 'sagan':
                sc.add(data['img_path'][0], model.infer_nhwc(data))
            elif 'cyclegan' in opt.model:
                sc.add(data['A_paths'][0], model.infer_nhwc(data, 'A'), 0)
                sc.add(data['B_paths'][0], model.infer_nhwc(data, 'B'), 1)
            else:
                sc.add(data['A_paths'][0], model.infer_nhwc(data))
        values = sc.result()
        if logger is not None:
            logger.info(fid_line(values, sc.tags, opt.model))
        kid = sc.kid()                             # None without a feature file beside every real_stat*.npz: no line, no launch
        if kid is not None and logger is not None:
            logger.info(kid_line(kid, sc.tags, opt.model))
        prdc = sc.prdc()                           # None unless GCC_FID_PRDC names a k
        if prdc is not None and logger is not None:
            logger.info(prdc_line(prdc, sc.tags, opt.model))
        score = sc.inception_score()               # None unless GCC_FID_IS names the splits
        if score is not None and logger is not None:
            logger.info(is_line(score, sc.tags, opt.model))
        return list(zip(values, sc.tags))

    evaluate.state = state
    evaluate.scorer = scorer
    return evaluate


PRECISION_ENV = 'GCC_FID_PRECISION'
DIMS_ENV = 'GCC_FID_DIMS'


def fid_dims(dims=None):
    """the feature width to score with: ``dims``, else GCC_FID_DIMS, else 2048; GccError names the four widths otherwise"""
    from .inception_fid import BLOCK_INDEX_BY_DIM
    what = 'dims'
    if dims is None:
        dims, what = os.environ.get(DIMS_ENV) or 2048, DIMS_ENV
    try:
        value = int(str(dims).strip())
    except ValueError:
        value = None
    if value not in BLOCK_INDEX_BY_DIM:
        raise GccError('%s=%s: expected one of %s' % (what, dims, ', '.join(str(d) for d in sorted(BLOCK_INDEX_BY_DIM))))
    return value


def _native_inception(path, dims=None):
    """(InceptionFidEngine on the host, None) when `path` is the reference's own weight file -- the plain state_dict of
    fid_inception_v3() --, (None, why) when it is one this package does not run, (None, None) for any other file.  The environment
    variable GCC_FID_PRECISION ('bf16', the default, or 'fp32': the reference's own arithmetic on the f32-input matrix
    instructions) chooses the engine's precision; any other value raises GccError.  ``dims`` (else GCC_FID_DIMS, else 2048:
    fid_dims) chooses the output block whose pooled features the engine returns."""
    from .inception_fid import BLOCK_INDEX_BY_DIM, PRECISIONS, InceptionFidEngine, is_fid_inception_state_dict
    try:
        sd = torch.load(path, map_location='cpu', weights_only=True)
    except Exception:
        return None, None
    if not is_fid_inception_state_dict(sd):
        return None, None
    precision = os.environ.get(PRECISION_ENV) or 'bf16'
    if precision not in PRECISIONS:
        raise GccError('%s=%s: expected one of %s' % (PRECISION_ENV, precision, ', '.join(PRECISIONS)))
    block = BLOCK_INDEX_BY_DIM[fid_dims(dims)]
    try:
        return InceptionFidEngine(sd, precision=precision, output_blocks=(block,), pooled=True), None
    except GccError as e:
        return None, '%s %s holds an Inception state_dict this package does not run: %s' % (ENV, path, e)


def load_inception(dims=None):
    """(network, None) from the file GCC_FID_INCEPTION names -- a TorchScript archive of InceptionV3([3]), or the reference's own
    pt_inception weight file (a plain state_dict: InceptionFidEngine runs it natively, at the precision GCC_FID_PRECISION names)
    --, else (None, the condition that failed).  A TorchScript archive runs as it was exported and ignores GCC_FID_PRECISION and
    the width (``dims``, else GCC_FID_DIMS, else 2048: the native network's output block, fid_dims)."""
    path = os.environ.get(ENV)
    if not path:
        return None, '%s is not set (the path of a TorchScript archive of the Inception network)' % ENV
    if not os.path.isfile(path):
        return None, '%s %s does not exist' % (ENV, path)
    try:
        return torch.jit.load(path, map_location='cpu'), None
    except Exception as e:
        first = (str(e).strip().splitlines() or [type(e).__name__])[0]
        engine, refusal = _native_inception(path, dims)
        if engine is not None or refusal is not None:
            return engine, refusal
        return None, 'torch.jit.load could not read %s %s as a TorchScript archive (%s: %s); a plain state_dict needs the ' \
                     'network\'s code: export InceptionV3([3]) with torch.jit once' % (ENV, path, type(e).__name__, first)


def network_label(inception):
    """' (native, bf16|fp32)' for a native engine -- ' (native, bf16, dims 192)' when it is tapped below 2048 --, '' for a
    TorchScript archive: the log lines' word on which network scores"""
    precision = getattr(inception, 'precision', None)
    if not precision:
        return ''
    blocks = getattr(inception, 'output_blocks', (3,))
    return ' (native, %s%s)' % (precision, '' if blocks[-1] == 3 else ', dims %d' % inception.d)


def builtin_inception(opt):
    """for a run whose evaluation is FID (wants_fid): (network, None) when GCC_FID_INCEPTION names a network file (load_inception) and
    --dataroot holds the real statistics the model's slots need, else (None, the condition that failed)"""
    module, why = load_inception()
    if module is None:
        return None, why
    missing = [name for name, _ in real_stat_slots(opt) if not os.path.isfile(os.path.join(str(opt.dataroot), name))]
    if missing:
        return None, '%s holds no %s (python -m gcc_amd.metric.get_real_stat writes it)' % (opt.dataroot, ', '.join(missing))
    return module, None
