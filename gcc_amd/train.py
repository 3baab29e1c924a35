"""Training entry point: the reference's train.py loop (train.py:75-174) on the MI355X path.

    python -m gcc_amd.train --dataroot ./database/cityscapes/ --model pix2pix --ngf 32 --ndf 128 \\
        --online_distillation --darts_discriminator --lambda_content 50 --lambda_gram 1e4 ...
    (data parallel: python -m torch.distributed.run --nproc-per-node 8 -m gcc_amd.train ...)

Batches come from gcc_amd.data (host decode + the GPU transform chain of SURVEY.md 8(f).4) or, with
``--dataroot synthetic[:N]``, from seeded U[-1,1) pairs of the same shape.  Any iterable of the reference's
batch dicts ({'A','B','A_paths','B_paths'} ...) can be passed to main(datasets=...) instead.
The per-epoch evaluation of the reference's loop (train.py:14-73, 160-165) needs third-party evaluator networks
(Inception / DRN weights): main(evaluate=fn) takes the callable that produces the metric(s) -- gcc_amd.metric supplies
the arithmetic downstream of those networks -- and keeps the reference's best-checkpoint bookkeeping around it.  Without
evaluate=, builtin_evaluator picks SRGAN's PSNR / SSIM, given a segmenter at --drn_path (the reference's DRNSeg .pth or a TorchScript archive) the Cityscapes mIoU, or, given
a TorchScript Inception network at GCC_FID_INCEPTION and real_stat*.npz under --dataroot, the FID of the other three cases.
"""
import copy
import os
import random
import tempfile
import time

import torch

from . import dist as gdist
from ._lib import GccError
from .models import get_model_class
from .options import options
from .utils import util


class SyntheticPairs:
    def __init__(self, opt, n_batches, seed):
        self.opt, self.n, self.seed = opt, n_batches, seed

    def __len__(self):
        return self.n * self.opt.batch_size

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        b, s = self.opt.batch_size, self.opt.crop_size
        img = lambda size: torch.rand(b, 3, size, size, generator=g) * 2 - 1
        for _ in range(self.n):
            if self.opt.model == 'sagan':            # data/sa_dataset.py:45
                yield {'z': torch.randn(b, self.opt.z_dim, generator=g), 'real_img': img(s), 'img_path': [''] * b}
            elif self.opt.model == 'srgan':          # data/sr_dataset.py:173
                hr = self.opt.image_size
                yield {'lr': img(hr // self.opt.upscale_factor), 'hr': img(hr), 'lr_names': [''] * b, 'hr_names': [''] * b}
            else:
                yield {'A': img(s), 'B': img(s), 'A_paths': [''] * b, 'B_paths': [''] * b}


def make_datasets(opt):
    root = str(opt.dataroot)
    if root.startswith('synthetic'):
        n = int(root.split(':')[1]) if ':' in root else 8
        r = gdist.rank()
        return SyntheticPairs(opt, n, 1234 + r), SyntheticPairs(opt, n, 4321 + r)
    # host decode + GPU transforms (gcc_amd.data); two loaders over the same phase, as create_split_dataset builds
    # them (data/__init__.py:59-66)
    from .data import create_dataset
    return create_dataset(opt), create_dataset(opt)


def attach_teacher(model, opt, model_class):
    """train.py:92-105"""
    topt = copy.deepcopy(opt)
    topt.ngf, topt.ndf = opt.teacher_ngf, opt.teacher_ndf
    topt.darts_discriminator = topt.online_distillation = False
    topt.generator_only = False
    teacher = model_class(topt)
    teacher.model_train()
    if opt.teacher_initial_path is not None:
        teacher.load_models(opt.teacher_initial_path, load_discriminator=False)
    model.teacher_model = teacher
    model.init_distillation()
    teacher.init_distillation()
    return teacher


class BestRecord:
    """utils/best_information.py:1-33 -- best value and epoch per metric slot.  Larger is better for the SRGAN scores and the
    cityscapes mIoU, smaller for every FID; ties count as an improvement (the reference compares with <= / >=)."""

    def __init__(self, opt):
        self.higher = opt.model == 'srgan' or 'cityscapes' in str(opt.dataroot)
        self.value, self.epoch = {}, {}

    def update(self, metric, epoch, index=0):
        best = self.value.get(index, 0.0 if self.higher else float('inf'))
        if (best <= metric) if self.higher else (best >= metric):
            self.value[index], self.epoch[index] = metric, epoch
            return True
        return False

    def report(self, logger, last):
        last = list(last) if isinstance(last, (list, tuple)) else [last]
        logger.info(' | '.join('slot %d: best epoch %d %.2f / last %.2f' % (i, self.epoch.get(i, 0), self.value.get(i, float('nan')), v)
                               for i, v in enumerate(last)))


def run_evaluation(model, opt, logger, epoch, best, evaluate, ckpt_dir):
    """train.py:14-73: evaluate(model, opt) returns [(metric value, direction tag), ...] in the reference's slot order
    (pix2pix: one mIoU or FID tagged opt.direction; cyclegan: AtoB, BtoA FIDs; sagan: one FID; srgan: 4 PSNR then 4 SSIM
    tagged with the test-set names); a new best in a slot saves model_best_<tag>.pth on rank 0."""
    model.model_eval()
    scores = evaluate(model, copy.deepcopy(opt))
    model.model_train()
    for i, (value, tag) in enumerate(scores):
        logger.info('evaluation slot %d (%s): %.2f' % (i, tag, value))
        if best.update(value, epoch, index=i):
            model.save_models(epoch, ckpt_dir, fid=value, isbest=True, direction=tag)
    return [v for v, _ in scores]


def _generator_note(opt):
    """what an evaluation's announcement says about the generator whose images it scores: nothing on the default bf16 inference
    route, its precision once GCC_GEN_PRECISION -- for a MobileResnet generator GCC_RESNET_PRECISION -- selects another
    (models/Pix2Pix.py gen_precision, resnet_precision; GCC_GEN_PRECISION=fp32 on a generator other than the U-Net raises here,
    before the first epoch), for the SAGAN generator GCC_SAGAN_PRECISION (models/SAGAN.py sagan_precision)"""
    from .models.Pix2Pix import gen_precision, resnet_precision
    if opt.model == 'pix2pix':
        precision = gen_precision(only_bf16='--backbone resnet' if opt.backbone == 'resnet' else None)
    else:
        precision = gen_precision(only_bf16='--model %s' % opt.model)
    if opt.model == 'cyclegan' or (opt.model == 'pix2pix' and opt.backbone == 'resnet'):
        precision = resnet_precision()           # a MobileResnet generator: GCC_RESNET_PRECISION (GCC_GEN_PRECISION=fp32 raised above)
    if opt.model == 'sagan':
        from .models.SAGAN import sagan_precision
        precision = sagan_precision()            # the SAGAN generator: a variable of its own, as the MobileResnet's
    return '' if precision == 'bf16' else '; generator images in %s' % precision


def builtin_evaluator(opt, logger):
    """the evaluation a run gets without an explicit evaluate=: SRGAN's PSNR / SSIM on the reference's test sets found under
    <dataroot>/test (train.py:37-56); Pix2Pix's mIoU on a Cityscapes root that holds table.txt when --drn_path is the reference's
    DRNSeg state_dict or a TorchScript segmenter (train.py:16-25; gcc_amd.metric.cityscapes, .drn_seg); the FID of Pix2Pix on any other root, CycleGAN and SAGAN (train.py:26-36,
    57-73; gcc_amd.metric.fid_eval) when GCC_FID_INCEPTION names a TorchScript Inception network and the root holds the real
    statistics; None otherwise"""
    if opt.model == 'pix2pix' and 'cityscapes' in str(opt.dataroot):
        from .metric.cityscapes import builtin_segmenter, cityscapes_evaluator
        segmenter, why = builtin_segmenter(opt)
        if segmenter is None:
            logger.info('no Cityscapes mIoU evaluation: %s' % why)
            return None
        precision = getattr(segmenter, 'precision', None)          # the native engine's; a TorchScript archive has none
        logger.info('Cityscapes mIoU evaluation every %d epochs with the segmenter %s%s%s'
                    % (opt.save_epoch_freq, opt.drn_path, ' (native, %s)' % precision if precision else '', _generator_note(opt)))
        return cityscapes_evaluator(segmenter, logger)
    if str(opt.dataroot).startswith('synthetic'):
        return None
    from .metric.fid_eval import ENV, builtin_inception, fid_evaluator, network_label, wants_fid
    if wants_fid(opt):
        inception, why = builtin_inception(opt)
        if inception is None:
            logger.info('no FID evaluation: %s' % why)
            return None
        logger.info('FID evaluation every %d epochs with the Inception network %s%s%s'
                    % (opt.save_epoch_freq, os.environ[ENV], network_label(inception), _generator_note(opt)))
        return fid_evaluator(inception, logger)
    if opt.model != 'srgan':
        return None
    from .metric.sr_eval import available_sets, sr_precision, srgan_evaluator
    sets = available_sets(opt)
    if not sets:
        return None
    logger.info('SRGAN evaluation every %d epochs (native, %s) on: %s' % (opt.save_epoch_freq, sr_precision(), ', '.join(sets)))
    return srgan_evaluator(logger, sets)


STATE_FILE = 'training_state.pth'
# options that may differ between the run that wrote a training state and the run that resumes from it: they change neither the
# arithmetic nor the data of an epoch (save_epoch_freq only how often the state is written)
RESUME_FREE = ('print_freq', 'gpu_ids', 'num_threads', 'checkpoints_dir', 'continue_train', 'save_epoch_freq')


def write_atomic(obj, path):
    """torch.save(obj, path) through a temporary file in the same directory and os.replace: a write that fails or is killed
    part way leaves the previous file as it was"""
    fd, tmp = tempfile.mkstemp(prefix='.' + os.path.basename(path) + '.', suffix='.tmp', dir=os.path.dirname(path) or '.')
    try:
        with os.fdopen(fd, 'wb') as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def _host_rng():
    return {'python': random.getstate(), 'torch': torch.get_rng_state(),
            'cuda': torch.cuda.get_rng_state() if torch.cuda.is_available() else None}


def _set_host_rng(state):
    random.setstate(state['python'])
    torch.set_rng_state(state['torch'])
    if state['cuda'] is not None:
        torch.cuda.set_rng_state(state['cuda'])


def save_training_state(path, model, start_opt, epoch, total_iters, best):
    """--continue_train: the run as it stands at the top of epoch + 1, written by rank 0.  Under data parallelism every rank's
    host RNG streams and rank-local model state (the image pools: each rank pools its own fakes) are gathered into it."""
    model._quiesce()
    mine = {'rng': _host_rng(), 'local': model.rank_local_state() if gdist.is_dist() else None}
    if gdist.is_dist():
        ranks = [None] * gdist.world_size()
        torch.distributed.all_gather_object(ranks, mine)
    else:
        ranks = [mine]
    if gdist.rank() != 0:
        return None
    t0 = time.time()
    write_atomic({'model': model.training_state(), 'epoch': epoch, 'total_iters': total_iters, 'best': (best.value, best.epoch),
                  'ranks': ranks, 'opt': start_opt}, path)
    return time.time() - t0


def check_resume_options(stored, opt):
    """GccError naming every option in which the stored run and this one differ (RESUME_FREE aside)"""
    now = vars(opt)
    diff = sorted(k for k in set(stored) | set(now) if k not in RESUME_FREE and stored.get(k, '<unset>') != now.get(k, '<unset>'))
    if diff:
        raise GccError('--continue_train: the saved training state was written by a run with other options: ' +
                       ', '.join('%s (saved %r, now %r)' % (k, stored.get(k, '<unset>'), now.get(k, '<unset>')) for k in diff))


def main(argv=None, datasets=None, evaluate=None):
    gdist.init_from_env()
    opt = options.parse(argv)
    opt.isTrain = True
    start_opt = copy.deepcopy(vars(opt))                   # update_learning_rate moves opt.ema_beta
    exp = os.path.join(opt.checkpoints_dir, opt.name)
    util.mkdirs(exp)
    logger = util.get_logger(os.path.join(exp, 'logger.log' if gdist.rank() == 0 else 'logger.rank%d.log' % gdist.rank()))
    model_class = get_model_class(opt)
    model = model_class(opt)
    if opt.norm_prune or opt.scale_prune:
        from .utils.prune_util import cyclegan_prune, prune
        model = cyclegan_prune(model, opt, logger) if 'cyclegan' in opt.model else prune(model, opt, logger)
    if opt.online_distillation:
        attach_teacher(model, opt, model_class)
    if opt.initial_path is not None:
        model.load_models(opt.initial_path, load_discriminator=False)
    train_set, val_set = datasets if datasets is not None else make_datasets(opt)
    logger.info('The number of training images = %d' % len(train_set))
    if evaluate is None:
        evaluate = builtin_evaluator(opt, logger)
    total_iters = 0
    best, last_scores = BestRecord(opt), None
    first_epoch = opt.epoch_count
    state_path = os.path.join(exp, STATE_FILE) if opt.continue_train else None
    if state_path is not None and os.path.exists(state_path):
        state = torch.load(state_path, map_location='cpu', weights_only=False)
        check_resume_options(state['opt'], opt)
        if len(state['ranks']) != gdist.world_size():
            raise GccError('--continue_train: the saved training state holds %d ranks, this run has %d'
                           % (len(state['ranks']), gdist.world_size()))
        mine = state['ranks'][gdist.rank()]
        model.load_training_state(state['model'])
        if mine['local'] is not None:
            model.load_rank_local_state(mine['local'])
        total_iters = state['total_iters']
        best.value, best.epoch = state['best']
        first_epoch = state['epoch'] + 1
        _set_host_rng(mine['rng'])                       # last: building the model and the loaders drew from them
        logger.info('resuming from epoch %d (iters %d) of %s' % (first_epoch, total_iters, state_path))
        del state
    # GCC_REPLAY=1: the iteration is recorded once per epoch and re-issued from native code (gcc_amd.replay: the launch-bound
    # models -- CycleGAN at batch 1, SAGAN, SRGAN -- train at the GPU's pace instead of the Python host's); same results
    replay = None
    if os.environ.get('GCC_REPLAY', '0') == '1':
        from .replay import IterationReplay
        replay = IterationReplay(model, opt, enabled=True)
    for epoch in range(first_epoch, opt.n_epochs + opt.n_epochs_decay + 1):
        model.model_train()
        logger.info('\nEpoch:%d' % epoch)
        t_epoch = time.time()
        val_iter = iter(val_set)
        epoch_iter = 0
        for data in train_set:
            t0 = time.time()
            total_iters += opt.batch_size
            epoch_iter += opt.batch_size
            if replay is not None:
                arch = opt.darts_discriminator and model.teacher_model is not None
                replay.step(data, next(val_iter) if arch else None)
            else:
                model.set_input(data)
                model.optimize_parameters()
                if opt.darts_discriminator and model.teacher_model is not None:
                    model.set_input(next(val_iter))
                    model.clipping_mask_alpha()
                    model.optimizer_netD_arch()
            if total_iters % opt.print_freq == 0:
                losses = model.get_current_losses()
                msg = '(epoch: %d, iters: %d, time: %.3f) ' % (epoch, epoch_iter, (time.time() - t0) / opt.batch_size)
                logger.info(msg + ' '.join('%s: %.3f' % kv for kv in losses.items()))
        if epoch % opt.save_epoch_freq == 0:            # train.py:160-165
            if evaluate is not None:
                last_scores = run_evaluation(model, opt, logger, epoch, best, evaluate, os.path.join(exp, 'checkpoints'))
            logger.info('saving the model at the end of epoch %d, iters %d' % (epoch, total_iters))
            if epoch == opt.n_epochs + opt.n_epochs_decay:
                model.save_models(epoch, os.path.join(exp, 'checkpoints'))
        model.print_sparse_info(logger)
        logger.info('End of epoch %d / %d \t Time Taken: %d sec' % (epoch, opt.n_epochs + opt.n_epochs_decay,
                                                                    time.time() - t_epoch))
        model.update_learning_rate(epoch)
        if replay is not None:
            replay.invalidate()          # learning rates (and the EMA beta) are launch arguments of the recording
        if state_path is not None and epoch % opt.save_epoch_freq == 0:
            took = save_training_state(state_path, model, start_opt, epoch, total_iters, best)
            if took is not None:
                logger.info('training state of epoch %d written to %s in %.1f s' % (epoch, state_path, took))
    if last_scores is not None:
        best.report(logger, last_scores)
    return model


if __name__ == '__main__':
    main()
