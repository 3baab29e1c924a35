"""Pix2Pix GCC model on MI355X -- the reference's ``models/Pix2Pix.py`` surface
(set_input / forward / optimize_parameters / optimizer_netD_arch / ... ) over the HIP engine.

What is kept name-for-name (callers: train.py:84-172, test.py, metric/test_metric.py,
utils/prune_util.py): class names, constructor signatures, ``netG`` / ``netD`` module trees whose
``state_dict`` keys equal the reference's (module paths such as ``model.model.1.model.2.weight``),
``loss_names`` / ``visual_names``, the optimizers list, schedulers, checkpoint dict layout.

What is different: the module trees only own parameters; every tensor operation of the step is a
hand-written gfx950 kernel scheduled by gcc_amd.engine (no autograd graph).  The step is written
out explicitly in the order of models/Pix2Pix.py:565-593 and its helpers (:464-552).
Under data parallelism (torch.distributed initialised by the launcher) gradients are summed over
ranks on RCCL at the five backward boundaries of the iteration.
"""
import copy
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import dist as gdist
from .. import engine, ops
from .. import _lib
from .._lib import GccError
from ..utils import util
from .DifferentiableOp import DifferentiableOP
from ._base import GANModelBase
from ._optim import HipAdam             # stays importable as gcc_amd.models.Pix2Pix.HipAdam


# ------------------------------------------------------------------------------------------------
# parameter-owning module trees (state_dict-compatible with the reference)
# ------------------------------------------------------------------------------------------------
def _attach(root, dotted, leaf):
    parts = dotted.split('.')
    m = root
    for p in parts[:-1]:
        if not hasattr(m, p):
            m.add_module(p, nn.Module())
        m = getattr(m, p)
    m.add_module(parts[-1], leaf)


def _bn(c):
    return nn.BatchNorm2d(c, affine=True, track_running_stats=True)


class UnetGenertor(nn.Module):
    """Parameter tree of the reference's UnetGenertor (models/Pix2Pix.py:79-130; spelling kept).
    Block at nesting position j: prefix 'model' (j=0) / 'model.model.1' + '.model.3'*(j-1).

    Pruned cfgs may remove blocks (models/Pix2Pix.py:87, 97): the innermost block (depth 7) when filter_cfgs[7] or [8] is 0,
    a loop block (depths 6, 5, 4) when filter_cfgs[6-i] or [9+i] is 0.  `present` lists the depths that are built, outermost
    first; the nesting (and with it every state_dict key) goes by position in that list, as in the reference where a parent
    simply wraps whatever block was built last.  When the innermost block is absent the last block is a loop block around
    Identity (:59-67): conv, BatchNorm, ReLU, transposed conv, BatchNorm -- `inner_identity`."""

    def __init__(self, input_nc, output_nc, num_downs, ngf=64, norm_layer=None, use_dropout=False,
                 filter_cfgs=None, channel_cfgs=None):
        super().__init__()
        D = num_downs
        self.num_downs, self.use_dropout = D, use_dropout
        present = list(range(D))
        if filter_cfgs is None:
            wd = [min(ngf * 2 ** d, ngf * 8) for d in range(D)]
            down_in = [input_nc] + wd[:-1]
            up_in = [2 * wd[d] for d in range(D - 1)] + [wd[D - 1]]
            up_out = [output_nc] + wd[:-1]
        else:
            if D != 8:
                raise NotImplementedError('filter_cfgs describe the num_downs=8 generator')
            f, c = [int(v) for v in filter_cfgs], [int(v) for v in channel_cfgs]
            wd = f[:8]
            down_in = [input_nc] + c[:7]
            up_in = [c[14 - d] for d in range(8)]
            up_out = [output_nc] + [f[15 - d] for d in range(1, 8)]
            present = [0, 1, 2, 3] + [d for d in (4, 5, 6) if f[d] != 0 and f[15 - d] != 0] + \
                      ([7] if f[7] != 0 and f[8] != 0 else [])
            if any(wd[d] <= 0 or up_in[d] <= 0 or (d > 0 and up_out[d] <= 0) or (d > 0 and down_in[d] <= 0) for d in present):
                raise ValueError('filter_cfgs / channel_cfgs give a built block a zero width: %r %r' % (f, c))
        self.present = present
        self.inner_identity = present[-1] != D - 1
        # the blocks torch's Dropout sits in: the loop blocks (models/Pix2Pix.py:101-104: depths D-2 .. 4), by position
        self.dropout_positions = [j for j, d in enumerate(present) if 4 <= d <= D - 2] if use_dropout else []
        K = len(present)

        def prefix(j):
            return 'model' if j == 0 else 'model.model.1' + '.model.3' * (j - 1)
        _attach(self, 'model.model.0', nn.Conv2d(down_in[0], wd[0], 4, 2, 1, bias=False))
        for j in range(1, K):
            d, p = present[j], prefix(j)
            _attach(self, p + '.model.1', nn.Conv2d(down_in[d], wd[d], 4, 2, 1, bias=False))
            if d < D - 1:
                _attach(self, p + '.model.2', _bn(wd[d]))
        for j in range(K - 1, 0, -1):
            d, p = present[j], prefix(j)
            if d == D - 1:
                _attach(self, p + '.model.3', nn.ConvTranspose2d(up_in[d], up_out[d], 4, 2, 1, bias=False))
                _attach(self, p + '.model.4', _bn(up_out[d]))
            else:
                _attach(self, p + '.model.5', nn.ConvTranspose2d(up_in[d], up_out[d], 4, 2, 1, bias=False))
                _attach(self, p + '.model.6', _bn(up_out[d]))
        _attach(self, 'model.model.3', nn.ConvTranspose2d(up_in[0], up_out[0], 4, 2, 1, bias=True))
        # what a block hands to the one inside it must be what that block's conv takes, and what comes back up must be what the
        # transposed conv takes (the reference would fail in forward(); here the engine would read garbage)
        for j in range(1, K):
            d, o = present[j], present[j - 1]
            if down_in[d] != wd[o]:
                raise ValueError('block at depth %d takes %d channels but its parent (depth %d) produces %d' % (d, down_in[d], o, wd[o]))
            inner = wd[d] if j == K - 1 else wd[d] + up_out[present[j + 1]]
            if up_in[d] != inner:
                raise ValueError('up conv at depth %d takes %d channels, its input has %d' % (d, up_in[d], inner))
        if up_in[0] != wd[0] + up_out[present[1]]:
            raise ValueError('outermost up conv takes %d channels, its input has %d' % (up_in[0], wd[0] + up_out[present[1]]))

    def forward(self, x):
        raise GccError('UnetGenertor owns parameters only; run it through Pix2PixModel (gcc_amd.engine.UnetEngine)')


class SeparableConv2d(nn.Module):
    """depthwise kxk (+bias) -> InstanceNorm -> pointwise 1x1 (+bias)   (models/Pix2Pix.py:132-145); parameters only"""

    def __init__(self, in_channels, out_channels, kernel_size=3):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_channels, in_channels, kernel_size, groups=in_channels, bias=True),
                                  nn.InstanceNorm2d(in_channels), nn.Conv2d(in_channels, out_channels, 1, bias=True))


class MobileResnetBlock(nn.Module):
    """conv_block slots: 0 pad, 1 separable, 2 IN, 3 ReLU, 4 dropout, 5 pad, 6 separable, 7 IN
    (models/Pix2Pix.py:147-197); out = x + conv_block(x)"""

    def __init__(self, c_in, c_mid, c_out, dropout_rate=0.0):
        super().__init__()
        self.conv_block = nn.Sequential(nn.ReflectionPad2d(1), SeparableConv2d(c_in, c_mid), nn.InstanceNorm2d(c_mid),
                                        nn.ReLU(True), nn.Dropout(dropout_rate), nn.ReflectionPad2d(1),
                                        SeparableConv2d(c_mid, c_out), nn.InstanceNorm2d(c_out))


class MobileResnetGenerator(nn.Module):
    """Parameter tree of the reference's MobileResnetGenerator (models/Pix2Pix.py:199-265, models/CycleGAN.py:77-138).
    cfg: 23 widths [stem x3, (mid, out) x n_blocks, up x2]; a block whose mid width is 0 is left out, which shifts
    the Sequential indices behind it exactly as in the reference."""

    def __init__(self, input_nc=3, output_nc=3, ngf=64, norm_layer=nn.InstanceNorm2d, dropout_rate=0, n_blocks=9,
                 padding_type='reflect', opt=None, cfg=None):
        super().__init__()
        if norm_layer is not nn.InstanceNorm2d or padding_type != 'reflect' or dropout_rate != 0:
            raise NotImplementedError('the MI355X path implements the configuration the reference trains: InstanceNorm, '
                                      'reflect padding, dropout 0')
        self.opt = opt
        w = [int(v) for v in cfg] if cfg is not None else [ngf, 2 * ngf, 4 * ngf] + [4 * ngf] * (2 * n_blocks) + [2 * ngf, ngf]
        assert len(w) == 5 + 2 * n_blocks, 'cfg must hold %d widths' % (5 + 2 * n_blocks)
        seq = [nn.ReflectionPad2d(3), nn.Conv2d(input_nc, w[0], 7, bias=True), nn.InstanceNorm2d(w[0]), nn.ReLU(True)]
        for i in (1, 2):
            seq += [nn.Conv2d(w[i - 1], w[i], 3, stride=2, padding=1, bias=True), nn.InstanceNorm2d(w[i]), nn.ReLU(True)]
        j = 3
        for _ in range(n_blocks):
            if w[j] != 0:
                seq.append(MobileResnetBlock(w[j - 1], w[j], w[j + 1], dropout_rate))
            j += 2
        for i in (j, j + 1):
            seq += [nn.ConvTranspose2d(w[i - 1], w[i], 3, stride=2, padding=1, output_padding=1, bias=True),
                    nn.InstanceNorm2d(w[i]), nn.ReLU(True)]
        seq += [nn.ReflectionPad2d(3), nn.Conv2d(w[j + 1], output_nc, 7, bias=True), nn.Tanh()]
        self.model = nn.Sequential(*seq)

    def forward(self, x):
        raise GccError('MobileResnetGenerator owns parameters only; run it through the model classes '
                       '(gcc_amd.engine.MobileResnetEngine)')


def _patchgan_tree(self, input_nc, ndf, n_layers, masked, threshold, norm='batch'):
    """norm='instance': the CycleGAN plain discriminator (InstanceNorm2d without parameters, a bias on every conv)"""
    inorm = norm == 'instance'
    ch = [ndf * min(2 ** i, 8) for i in range(n_layers + 1)]
    seq = nn.Module()
    self.add_module('model', seq)
    i = 0
    seq.add_module(str(i), nn.Conv2d(input_nc, ch[0], 4, 2, 1))
    i += 2
    if masked:
        seq.add_module(str(i), DifferentiableOP(ch[0], threshold))
        i += 1
    for n in range(1, n_layers + 1):
        stride = 2 if n < n_layers else 1
        seq.add_module(str(i), nn.Conv2d(ch[n - 1], ch[n], 4, stride, 1, bias=inorm))
        seq.add_module(str(i + 1), nn.InstanceNorm2d(ch[n]) if inorm else _bn(ch[n]))
        i += 2
        if masked:
            seq.add_module(str(i), DifferentiableOP(ch[n], threshold))
            i += 1
        i += 1        # LeakyReLU slot
    seq.add_module(str(i), nn.Conv2d(ch[n_layers], 1, 4, 1, 1))


class NLayerDiscriminator(nn.Module):
    """PatchGAN parameter tree (models/Pix2Pix.py:267-305): convs at model.0/2/5/8/11, BN at 3/6/9."""

    def __init__(self, input_nc=3, ndf=64, n_layers=3):
        super().__init__()
        _patchgan_tree(self, input_nc, ndf, n_layers, False, 0.5)


class MaskNLayerDiscriminator(nn.Module):
    """Selective-activation PatchGAN (models/Pix2Pix.py:307-348): convs at model.0/3/7/11/15,
    BN at 4/8/12, gates (alpha) at 2/5/9/13."""

    def __init__(self, input_nc=3, ndf=64, n_layers=3, threshold=0.5):
        super().__init__()
        _patchgan_tree(self, input_nc, ndf, n_layers, True, threshold)


# ------------------------------------------------------------------------------------------------
# Stream forks of the schedule.  Each is the product's path; False is the serialized form that
# tests/test_replay_gpu.py::test_pix2pix_stream_forks_change_nothing holds it to, bit for bit.
# DISTILL_FORK: the distillation terms on the generator's features run on the auxiliary stream beside the teacher
# discriminator's pass over the student's fake (backward_G's tail): +2.6 % (profiles/r4s_ab_distill_fork.txt)
DISTILL_FORK = True
# ARCH_FORK: the architecture step's two discriminator backward passes (fake, real) side by side on two streams: +1.9 %
# (profiles/r4y_ab_arch_fork.txt)
ARCH_FORK = True
# ARCH_FREE_EARLY: in the architecture step the teacher's stream hands its difference scalar over itself and is released behind
# its own part: +0.6 % (profiles/r4ay_ab_arch_free_early.txt)
ARCH_FREE_EARLY = True
# GCC_DP_TEACHER_UPDATE_EARLY (default 1; data parallelism only): the online teacher's generator update -- wait for its gradient
# buckets, Adam, repack -- is enqueued on the teacher's own stream right behind its backward pass instead of in front of the
# architecture step's teacher forward
DP_TEACHER_UPDATE_EARLY = os.environ.get('GCC_DP_TEACHER_UPDATE_EARLY', '1') != '0'
DP_TEACHER_BUCKETS_LATE = os.environ.get('GCC_DP_TEACHER_BUCKETS_LATE', '1') != '0'


def _drain(gen, stream):
    """every chunk of `gen` with `stream` current (None: the current stream)"""
    if stream:
        with ops.on_stream(stream):
            for _ in gen:
                pass
    else:
        for _ in gen:
            pass


GEN_PRECISION_ENV = 'GCC_GEN_PRECISION'
GEN_PRECISIONS = ('bf16', 'fp32')


def gen_precision(only_bf16=None):
    """the precision of the generator's inference path (Pix2PixModel.infer_nhwc) in gcc_amd.test --model pix2pix and in the
    per-epoch mIoU and FID evaluations: the environment variable GCC_GEN_PRECISION, 'bf16' (the default) or 'fp32' (the
    reference's own arithmetic on the f32-input matrix instructions: UnetEngine.infer(x, 'fp32')); any other value raises
    GccError.  The one place that reads it.  only_bf16: the caller is a generator without an fp32 route and names its backbone or
    model here -- 'fp32' then raises instead of falling back."""
    precision = os.environ.get(GEN_PRECISION_ENV) or 'bf16'
    if precision not in GEN_PRECISIONS:
        raise GccError('%s=%s: expected one of %s' % (GEN_PRECISION_ENV, precision, ', '.join(GEN_PRECISIONS)))
    if precision == 'fp32' and only_bf16:
        raise GccError('%s=fp32: the fp32 generator route exists for the U-Net only (--model pix2pix --backbone unet), not for %s'
                       % (GEN_PRECISION_ENV, only_bf16))
    return precision


RESNET_PRECISION_ENV = 'GCC_RESNET_PRECISION'


def resnet_precision():
    """the precision of a MobileResnet generator's inference path (Pix2PixModel.infer_nhwc with --backbone resnet,
    MobileCycleGANModel.infer_nhwc) in gcc_amd.test and in the per-epoch mIoU and FID evaluations: the environment variable
    GCC_RESNET_PRECISION, 'bf16' (the default) or 'fp32' (the reference's own arithmetic: MobileResnetEngine.infer(x, 'fp32'));
    any other value raises GccError.  The one place that reads it, and only where a MobileResnet generator infers: U-Net, SAGAN
    and SRGAN runs never look at it."""
    precision = os.environ.get(RESNET_PRECISION_ENV) or 'bf16'
    if precision not in GEN_PRECISIONS:
        raise GccError('%s=%s: expected one of %s' % (RESNET_PRECISION_ENV, precision, ', '.join(GEN_PRECISIONS)))
    return precision


def resnet_infer_nhwc(owner, G, real):
    """G (a MobileResnetEngine) in eval mode on the NCHW fp32 batch `real` at resnet_precision(): the NHWC bf16 image, or the
    NHWC fp32 one.  The fp32 packings are refreshed when owner._g_generation moved since this generator's last fp32 call."""
    N, _, H, W = real.shape
    precision = resnet_precision()
    if precision == 'fp32':
        done = owner.__dict__.setdefault('_ev_resnet_generation', {})
        generation = getattr(owner, '_g_generation', 0)
        if done.get(id(G)) != generation:
            G.eval_coeffs('fp32')
            done[id(G)] = generation
        return G.infer(ops.nchw_to_nhwc_f32(real, G.infer_input(N, H, W, 'fp32')), 'fp32')
    x = G.infer_input(N, H, W)
    ops.nchw_to_nhwc(real, x, cfill=8)
    return G.infer(x)


# ------------------------------------------------------------------------------------------------
class Pix2PixModel(GANModelBase):
    DISTILL_LOSSES = GANModelBase.DISTILL_LOSSES[:2]             # no 'L1' entry: G_L1 is always logged
    DISTILL_VISUALS = ('Tfake_B',)
    LR_REPORT = 'learning rate = %(lr).7f\tema beta = %(ema_beta).7f'

    @property
    def replay_supported(self):
        """gcc_amd.replay: the U-Net's dropout seeds are by-value launch arguments that change every iteration and that nothing
        patches, so an iteration with dropout in it stays on the eager host path (--no_dropout, or the resnet backbone whose
        blocks have Dropout(0), can be recorded: tests/test_replay_gpu.py).  The same holds for the online teacher."""
        def dropout(m):
            return (not m.resnet) and bool(getattr(getattr(m, 'G', None), 'drop_depths', None))
        t = getattr(self, 'teacher_model', None)
        return not dropout(self) and not (t is not None and dropout(t))


    def __init__(self, opt, filter_cfgs=None, channel_cfgs=None):
        super().__init__()
        self._init_device(opt)
        self.filter_cfgs, self.channel_cfgs = filter_cfgs, channel_cfgs
        self.loss_names = ['G_GAN', 'G_L1', 'D_real', 'D_fake']
        self.visual_names = ['real_A', 'fake_B', 'real_B']
        self.current_D_arch_diff_loss = 0.0
        self.teacher_model = None

        self.resnet = opt.backbone == 'resnet'
        if self.resnet:
            self.generator_extract_layers = ['model.9', 'model.12', 'model.15', 'model.18']
        else:
            self.generator_extract_layers = ['model.model.1.model.2', 'model.model.1.model.3.model.3.model.2',
                                             'model.model.1.model.3.model.3.model.4', 'model.model.1.model.4']
        self.discriminator_extract_layers = ['model.4', 'model.12'] if opt.darts_discriminator else ['model.3', 'model.9']

        self.optimizers = []
        if self.resnet:
            self.netG = MobileResnetGenerator(input_nc=3, output_nc=3, ngf=opt.ngf, cfg=filter_cfgs, opt=opt)
        else:
            self.netG = UnetGenertor(3, 3, opt.num_downs, ngf=opt.ngf, use_dropout=not opt.no_dropout,
                                     filter_cfgs=filter_cfgs, channel_cfgs=channel_cfgs)
        self.distill = bool(opt.online_distillation or opt.normal_distillation)
        self.transform_convs = []
        if self.distill:
            t_w = [opt.teacher_ngf * 2, opt.teacher_ngf * 8, opt.teacher_ngf * 16, opt.teacher_ngf * 4]
            if self.resnet:         # models/Pix2Pix.py:387-397: the four hooked tensors are all 4*ngf wide
                t_w = [opt.teacher_ngf * 4] * 4
                s_w = [opt.ngf * 4 if filter_cfgs is None else filter_cfgs[2]] * 4
            elif channel_cfgs is None:
                s_w = [opt.ngf * 2, opt.ngf * 8, opt.ngf * 16, opt.ngf * 4]
            else:
                s_w = [channel_cfgs[1], channel_cfgs[3], channel_cfgs[-4], channel_cfgs[-2]]
            self.transform_convs = [nn.Conv2d(s, t, 1, 1, 0, bias=False) for s, t in zip(s_w, t_w)]
        if opt.darts_discriminator:
            self.loss_names += ['D_arch_diff', 'D_arch', 'teacher_D_arch_diff']
            self.netD = MaskNLayerDiscriminator(input_nc=6, ndf=opt.ndf, threshold=opt.threshold)
        else:
            self.netD = NLayerDiscriminator(input_nc=6, ndf=opt.ndf)
        self.init_net()

        # ---- optimizers over flat parameter groups (models/Pix2Pix.py:382,415,430-440)
        dev = self.device
        g_params, g_l1 = [], []
        for m in self.netG.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                for p in m.parameters():
                    g_params.append(p)
                    g_l1.append(opt.lambda_weight if (p.dim() == 4 and opt.lambda_weight > 0.0) else 0.0)
            elif isinstance(m, nn.BatchNorm2d):
                g_params += [m.weight, m.bias]
                g_l1 += [opt.lambda_scale if (opt.lambda_scale > 0.0 and not opt.lambda_weight > 0.0) else 0.0, 0.0]
        for t in self.transform_convs:
            t.to(dev)
            gdist.broadcast_module(t)              # default-initialised from each rank's RNG: replicas must start equal
            g_params.append(t.weight)
            g_l1.append(0.0)
        # storage order of the flat gradient buffers = backward-completion order (transform convs, then the U-Net layer by
        # layer; the PatchGAN from its last conv down): data parallelism all-reduces finished runs while the backward continues
        g_layout = d_layout = None
        if not self.resnet:
            g_layout = ([[t.weight for t in self.transform_convs]] if self.transform_convs else []) + \
                engine.UnetEngine.grad_segments(self.netG, opt.num_downs)
        self.optimizer_G = HipAdam(g_params, lr=opt.lr, betas=(0.5, 0.999), l1=g_l1, layout=g_layout)
        w_params, a_params = [], []
        for m in self.netD.modules():
            if isinstance(m, (nn.Conv2d, nn.BatchNorm2d)):
                w_params += list(m.parameters())
            elif isinstance(m, DifferentiableOP):
                a_params += list(m.parameters())
        self.optimizer_D = HipAdam(w_params, lr=opt.lr, betas=(0.5, 0.999), layout=self._d_layout())
        if opt.darts_discriminator:
            self.optimizer_arch = HipAdam(a_params, lr=opt.arch_lr)
            if opt.arch_lr_step:
                arch_opt = copy.deepcopy(opt)
                arch_opt.lr_policy = 'step'
                arch_opt.lr_decay_iters = opt.n_epochs - 1
                self.arch_scheduler = util.get_scheduler(self.optimizer_arch, arch_opt)

        # ---- engines
        if self.resnet:
            self.G = engine.MobileResnetEngine(self.netG, dev)
            t_split = [0, 0, 0, 0]
        else:
            self.G = engine.UnetEngine(self.netG, opt.num_downs, dev, use_dropout=not opt.no_dropout)
            # the last two hooked features are concat buffers (skip | up path): their channel dimension is split
            t_split = [0, 0, self.G.width[3], self.G.width[1]]
        self.D = engine.PatchGANEngine(self.netD, bool(opt.darts_discriminator), opt.threshold, dev)
        self.D.mask_cache = True          # gate masks are recomputed only after alpha changed (arch step, clip, reload)
        if gdist.buckets_enabled(dev):
            mb = int(os.environ.get('GCC_DP_BUCKET_MB', '32'))
            if g_layout is not None:
                self.optimizer_G.reducer = self.G.reducer = gdist.GradReducer(self.optimizer_G, mb << 20)
                self.G.seg_base = 1 if self.transform_convs else 0
            self.optimizer_D.reducer = self.D.reducer = gdist.GradReducer(self.optimizer_D, mb << 20)
        self.T = [engine.ConvOp(t.weight, None, 1, 1, 0, False, col_split=sp)
                  for t, sp in zip(self.transform_convs, t_split)]
        self.refresh_weights()

        self.optimizers += [self.optimizer_G, self.optimizer_D]
        self.schedulers = [util.get_scheduler(o, opt) for o in self.optimizers]
        if opt.darts_discriminator and opt.arch_lr_step:
            self.schedulers.append(self.arch_scheduler)
        self._init_losses(['G_GAN', 'G_L1', 'D_real', 'D_fake', 'D_arch_fake', 'D_arch_fake_real', 'D_arch_real', 'D_arch_diff',
                           'D_arch', 'teacher_D_arch_diff', 'arch_c_fr', 'arch_c_f', 'scratch0', 'scratch1', 'scratch2', 'ema_prev'])
        self._dist_out = torch.zeros((6, 2), dtype=torch.float32, device=dev)
        self._fake_nchw = None
        if self._world > 1:
            engine.OVERLAP_WGRAD = engine.overlap_wgrad_default(self._world)
        self._defer_G_update = False
        self._pending_G = None
        self._comm_group = None        # gdist.chain_group('teacher') once this model runs as an online teacher on its own stream

    # ---------------------------------------------------------------------------------------
    def _engines(self):
        return [self.G, self.D] + self.T

    def refresh_weights(self):
        self._g_generation = getattr(self, '_g_generation', 0) + 1
        super().refresh_weights()
        self.D.mask_dirty = True

    def init_net(self):
        self.netG.to(self.device)
        self.netD.to(self.device)
        for m in self.netD.modules():
            if isinstance(m, DifferentiableOP):
                m.threshold = m.threshold.to(self.device)
        util.init_weights(self.netG, init_type='normal', init_gain=0.02)
        util.init_weights(self.netD, init_type='normal', init_gain=0.02)
        gdist.broadcast_module(self.netG)
        gdist.broadcast_module(self.netD)

    # ---------------------------------------------------------------------------------------
    def set_input(self, input):
        self.input = input
        self._note_input(input)
        AtoB = self.opt.direction == 'AtoB'
        self.real_A = input['A' if AtoB else 'B'].to(self.device, torch.float32).contiguous()
        self.real_B = input['B' if AtoB else 'A'].to(self.device, torch.float32).contiguous()
        self.image_paths = [input.get('A_paths' if AtoB else 'B_paths'), input.get('B_paths' if AtoB else 'A_paths')]
        N, _, H, W = self.real_A.shape
        if getattr(self, '_A', None) is None or tuple(self._A.shape) != (N, 3, H, W):
            self._A = ops.new_act(N, 3, H, W, self.device)
            self._B = ops.new_act(N, 3, H, W, self.device)
        ops.nchw_to_nhwc(self.real_A, self._A)
        ops.nchw_to_nhwc(self.real_B, self._B)

    def forward(self):
        """fake_B = G(real_A)  (models/Pix2Pix.py:460-462)"""
        self.finish_G_update()
        N, _, H, W = self._A.shape
        c = self.G._ctx(N, H, W, 'main' if self.resnet else 0)
        ops.nhwc_copy(self._A, 0, c.x_in, 0, 3, cfill=8)
        if self.netG.training:
            self._g_generation = getattr(self, '_g_generation', 0) + 1     # running statistics move
        if self.resnet:
            self._gctx = self.G.forward(c, train=self.netG.training)
        else:
            self._gctx = self.G.forward(N, H, W, train=self.netG.training)
        self._fake = self._gctx.out
        self._fake_nchw = None

    def infer_nhwc(self, real):
        """the generator in eval mode on `real` (NCHW fp32: the generator's input, real_A; or a dataset batch dict, whose input
        is picked by --direction as set_input does) through the fused inference path (UnetEngine.infer): an NHWC bf16
        [N, 3, H, W] view valid until the next call -- an NHWC fp32 one with GCC_GEN_PRECISION=fp32 (gen_precision).  Refreshes
        the eval-mode coefficients of that precision (one launch; fp32: and the fp32 weight packings) when the parameters or
        running statistics changed since its last call.  --backbone resnet: MobileResnetEngine.infer at the precision
        GCC_RESNET_PRECISION names (resnet_precision); GCC_GEN_PRECISION=fp32 is refused there as before."""
        if isinstance(real, dict):
            real = real['A' if self.opt.direction == 'AtoB' else 'B']
        real = real.to(self.device, torch.float32).contiguous()
        N, _, H, W = real.shape
        if self.resnet:
            gen_precision(only_bf16='--backbone resnet')
            # InstanceNorm without running statistics: the bf16 route has nothing to refresh (MobileResnetEngine.infer)
            self.finish_G_update()
            return resnet_infer_nhwc(self, self.G, real)
        precision = gen_precision()
        self.finish_G_update()
        done = self.__dict__.setdefault('_ev_generation', {})
        if done.get(precision) != self._g_generation:
            self.G.eval_coeffs(precision)
            done[precision] = self._g_generation
        x = self.G.infer_input(N, H, W, precision)
        if precision == 'fp32':
            return self.G.infer(ops.nchw_to_nhwc_f32(real, x), 'fp32')
        ops.nchw_to_nhwc(real, x, cfill=8)
        return self.G.infer(x)

    def infer(self, real):
        """fake_B = G(real) in eval mode as NCHW fp32 (see infer_nhwc), whatever mode the model is in; forward() in eval mode
        keeps its own route."""
        image = self.infer_nhwc(real)
        return ops.nhwc_to_nchw_f32(image, Cc=3) if image.dtype is torch.float32 else ops.nhwc_to_nchw(image, 3)

    @property
    def fake_B(self):
        if self._fake_nchw is None:
            self._fake_nchw = ops.nhwc_to_nchw(self._fake, 3)
        return self._fake_nchw

    @property
    def Tfake_B(self):
        """the teacher's generated image of the same batch (models/Pix2Pix.py:523; a visual, converted on demand)"""
        return self.teacher_model.fake_B

    # -- helpers ------------------------------------------------------------------------------
    def _pack_pair(self, ctx, second, A=None):
        """ctx.x_in = cat(real_A, second) along channels (3 + 3, zero-filled to 8)"""
        ops.nhwc_pack_pair(self._A if A is None else A, second, ctx.x_in, 3, 3)

    def _d_forward(self, tag, second, refresh=True, A=None):
        """A: the caller's own copy of real_A (the student's, when it runs the teacher's discriminator over its fake: the
        teacher may already hold the next batch)"""
        N, _, H, W = (self._A if A is None else A).shape
        ctx = self.D.new_ctx(N, H, W, tag)
        self._pack_pair(ctx, second, A)
        self.D.forward(ctx, train=True, refresh=refresh)
        return ctx

    def _start_real_pass(self, tag):
        """D(real_A, real_B) does not depend on the generator: start it on the auxiliary stream before the generator's
        forward (the student's stream is the iteration's critical path: ~460 mostly small launches, while the other
        streams idle half the time).  The pass keeps its place in the reference's order for everything that is order
        dependent: its BatchNorm running-statistics updates are applied in _take_real_pass(), after D(fake)'s."""
        self._early = getattr(self, '_early', {})
        # the student only: the online teacher's pass started early too measured slower (833 against 893 images/s: a fifth busy
        # queue on four hardware queues)
        aux = self._aux_stream() if self.teacher_model is not None else False
        if not aux:
            return
        main = ops.current_stream()
        self.D.refresh_masks() if self.D.masked else None
        ops.wait_stream(aux, main)
        with ops.on_stream(aux):
            N, _, H, W = self._A.shape
            ctx = self.D.new_ctx(N, H, W, tag)
            self._pack_pair(ctx, self._B)
            self.D.forward(ctx, train=True, defer_running=True, refresh=False)
        self._early[tag] = (ctx, aux)

    def _take_real_pass(self, tag):
        """the context of D(real) -- from the auxiliary stream if it was started early, else computed here"""
        got = getattr(self, '_early', {}).pop(tag, None)
        if got is None:
            return self._d_forward(tag, self._B)
        ctx, aux = got
        ops.wait_stream(ops.current_stream(), aux)
        self.D.apply_deferred_running(ctx)
        return ctx

    def _d_layout(self):
        """PatchGAN weight parameters in backward-completion order (engine.PatchGANEngine.grad_segments, by module index)"""
        mods = [m for m in self.netD.model.children() if isinstance(m, (nn.Conv2d, nn.BatchNorm2d))]
        segs, cur = [], []
        for m in mods:                       # forward order: conv, [bn], conv, [bn] ... -> one segment per conv (+ its bn)
            if isinstance(m, nn.Conv2d) and cur:
                segs.append(cur)
                cur = []
            cur = (list(m.parameters()) + cur) if isinstance(m, nn.BatchNorm2d) else cur + list(m.parameters())
        segs.append(cur)
        return segs[::-1]

    def _allreduce(self, optimizer):
        """gradient exchange before an optimizer step: buckets the backward pass already launched are waited for, the rest
        is reduced here"""
        if getattr(optimizer, 'reducer', None) is not None:
            optimizer.reducer.finish()
        else:
            gdist.all_reduce_grads(optimizer, group=self._comm_group)

    # -- D step (models/Pix2Pix.py:464-477) --------------------------------------------------------
    def backward_D(self):
        for _ in self._backward_D_steps():
            pass

    def _backward_D_steps(self):
        """backward_D in host-enqueue chunks (one discriminator pass each): the iteration's scheduler alternates the
        chunks of the student with those of the online teacher, so that both streams have work queued at the same time"""
        mode = self.opt.gan_mode
        early = 'd_real' in getattr(self, '_early', {})
        cf = self._d_forward('d_fake', self._fake, refresh=not early)
        yield
        cr = self._take_real_pass('d_real')
        gp = self.D.grad_pred_buffer(cf)
        if self.optimizer_D.reducer is not None:
            self.optimizer_D.reducer.begin()
        ops.gan_loss(mode, cf.pred, False, True, self._l('D_fake'), dpred=gp, grad_weight=0.5)
        yield
        self.D.backward(cf, wgrad=True, need_dx=False)
        yield
        ops.gan_loss(mode, cr.pred, True, True, self._l('D_real'), dpred=gp, grad_weight=0.5)
        self.D.reduce_now = True             # the second pass completes the gradients: its finished layers are exchanged
        self.D.backward(cr, wgrad=True, need_dx=False)
        self.D.reduce_now = False

    # -- G step (models/Pix2Pix.py:513-552) --------------------------------------------------------
    def backward_G(self, ts=None):
        """ts: the online teacher's stream -- joined only where its features are first read (the student's own GAN / L1
        terms and the discriminator's data gradient do not depend on it)"""
        for _ in self._backward_G_head_steps():
            pass
        self._backward_G_tail(ts)

    def _backward_G_head_steps(self):
        """the part of backward_G that does not read the teacher: D(fake) with the updated discriminator, the GAN / L1
        terms and the discriminator's data gradient"""
        opt, mode = self.opt, self.opt.gan_mode
        gc = self._gctx
        cg = self._d_forward('g_fake', self._fake)
        self._dctx_g = cg
        ops.gan_loss(mode, cg.pred, True, False, self._l('G_GAN'), dpred=self.D.grad_pred_buffer(cg))
        yield
        dx = self.D.backward(cg, wgrad=False, need_dx=True)
        ops.l1_loss(self._fake, self._B, self._l('G_L1'), weight=opt.lambda_L1, da=gc.g_out)
        ops.nhwc_add(dx, 3, gc.g_out, 0, 3)

    def _backward_G_tail(self, ts=None):
        opt = self.opt
        gc = self._gctx
        g_feat = None
        if self.optimizer_G.reducer is not None:
            self.optimizer_G.reducer.begin()
        if ts:
            ev = getattr(self.teacher_model, '_head_done', None)
            if ev is not None:
                ops.wait_event(ops.current_stream(), ev)
            else:
                ops.wait_stream(ops.current_stream(), ts)
        if self.distill:
            aux = self._aux_stream() if DISTILL_FORK else False
            if aux:
                # the generator's own terms on the auxiliary stream, beside the teacher discriminator's forward / backward over
                # the student's fake: this stretch of the step has one busy queue otherwise (DISTILL_FORK False: in line).
                # Forking the whole block earlier -- beside the student's discriminator step -- loses 4.7 %: the step is
                # chip-bound there (profiles/r4s_ab_distill_fork.txt)
                ops.wait_stream(aux, ops.current_stream())
                with ops.on_stream(aux):
                    g_feat = self._distill_generator_terms(gc)
            dx2 = self._distill_teacher_d_terms()
            if not aux:
                g_feat = self._distill_generator_terms(gc)
            if aux:
                ops.wait_stream(ops.current_stream(), aux)
            ops.nhwc_add(dx2, 3, gc.g_out, 0, 3)
            self._mark_teacher_free()
            if self.optimizer_G.reducer is not None:
                self.optimizer_G.reducer.segment_done(0)          # the transform convs' gradients (joined above)
        self.G.backward(gc, g_feat=g_feat, wgrad=True)

    def _distill_generator_terms(self, gc):
        """the four distillation terms on the generator's own features (transform conv, gram / content terms, their gradients
        back through the transform; models/Pix2Pix.py:520-533): independent of the teacher discriminator's pass over the
        student's fake.  Returns the gradients w.r.t. the hooked features; runs on the current stream."""
        opt = self.opt
        gfe = self.G.features(gc)
        N = gfe[0].shape[0]
        tf, dtf = [], []
        for i in range(4):
            f = gfe[i]
            buf = self._tbuf(i, N, self.T[i].rows, f.shape[2], f.shape[3])
            self.T[i].forward(f, buf[0])
            tf.append(buf[0])
            dtf.append(buf[1])
        for i in range(4):
            f, t = tf[i], self.target_distillation_features[i]
            ws = self._dws(i, N, f.shape[1], f.shape[2] * f.shape[3])
            ops.distill_fwd(f, t, self._dist_out[i], ws)
            ops.distill_bwd(f, t, opt.lambda_gram, opt.lambda_content, dtf[i], ws)
        out = []
        for i in range(4):
            self.T[i].backward_weight(gfe[i], dtf[i])
            gbuf = self._tbuf(10 + i, N, gfe[i].shape[1], gfe[i].shape[2], gfe[i].shape[3])[0]
            self.T[i].backward_data(dtf[i], gbuf)
            out.append(gbuf)
        ops.SideStream.get(self.device).join()
        return out

    def _distill_teacher_d_terms(self):
        """teacher D (train mode, frozen) on the student's fake, the two terms on its features (:531-533) and their gradient
        back to the image; returns that gradient's buffer (channels 3.. of the pair).  Runs on the current stream."""
        opt = self.opt
        T = self.teacher_model
        # this pass runs where the step has one or two busy queues (the student's tail): its half-chip launches (L3 forward, L4
        # data gradient: 128 workgroups of 256 x 256) take the 128-column halo tiles of the 'alone' plan: +0.3-0.6 %
        # (profiles/r4ao_ab_tail_halo_hc.txt)
        with ops.plan_override(halo_hc=1):
            ct = T._d_forward('on_student', self._fake, A=self._A)
            dfe = T.D.features(ct)
            N = dfe[0].shape[0]
            dtd = [self._tbuf(4 + j, N, dfe[j].shape[1], dfe[j].shape[2], dfe[j].shape[3])[1] for j in range(2)]
            for j in range(2):
                f, t = dfe[j], self.target_distillation_features[4 + j]
                ws = self._dws(4 + j, N, f.shape[1], f.shape[2] * f.shape[3])
                ops.distill_fwd(f, t, self._dist_out[4 + j], ws)
                ops.distill_bwd(f, t, opt.lambda_gram, opt.lambda_content, dtd[j], ws)
            return T.D.backward(ct, has_pred_grad=False, g_feat=dtd, wgrad=False, need_dx=True)

    def _tbuf(self, i, N, C, H, W):
        key = ('t', i, N, C, H, W)
        if key not in self._bufs:
            self._bufs[key] = (ops.new_act(N, C, H, W, self.device), ops.new_act(N, C, H, W, self.device))
        return self._bufs[key]

    # -- one iteration (models/Pix2Pix.py:565-583) ----------------------------------------------------
    def optimize_parameters(self):
        """models/Pix2Pix.py:565-583.  The online teacher's whole iteration (its own stream) is enqueued first, then the
        student's forward + discriminator step + the teacher-independent head of backward_G.  Teacher first is the fastest
        order: its iteration is the critical path (its end gates the student's backward_G), and enqueueing the two networks'
        chunks alternately measured 3.5-6 % slower (profiles/r02_ab_tables.md)."""
        self.finish_G_update()
        ts = None
        if self.opt.online_distillation:
            T = self.teacher_model
            T._defer_G_update = True
            ts = self._teacher_stream()
            T._own_stream = bool(ts)
            if ts and self._world > 1 and T._comm_group is None and not getattr(T, '_comm_group_set', False):
                # the teacher's chain runs beside this one: its gradient buckets travel on a communicator of their own
                T._comm_group_set = True
                T._comm_group = gdist.chain_group('teacher')
                for o in (T.optimizer_G, T.optimizer_D):
                    if getattr(o, 'reducer', None) is not None:
                        o.reducer.set_group(T._comm_group)
            if ts:
                self._release_teacher_stream(ts)                 # after the last launch that reads the teacher's buffers
            _drain(T._iteration_steps(self.input), ts)
        _drain(self._pre_join_steps(), None)
        if ts and getattr(self.teacher_model, '_held_G', False):
            # the student's discriminator buckets are issued: now the teacher generator's, and its update, on the teacher's stream
            self.teacher_model._held_G = False
            with ops.on_stream(ts):
                self.teacher_model.finish_G_update()
        if self.opt.online_distillation:
            # the reference clones; here the teacher's activation buffers of this iteration are
            # simply not overwritten before the student consumes them (separate contexts)
            self.target_distillation_features = self.teacher_model.get_distillation_features()
        self._backward_G_tail(ts)
        if self._defer_G_update and self._world > 1:
            # online teacher under data parallelism: its generator is not read again before the arch
            # step, so its (largest, 218 MB) gradient bucket is reduced while the student's whole
            # iteration runs; finish_G_update() applies it.  Same arithmetic, later in stream order.
            self._pending_G = self.optimizer_G.reducer or gdist.all_reduce_grads(self.optimizer_G, async_op=True, group=self._comm_group)
            return
        self._allreduce(self.optimizer_G)
        self._apply_G_update()

    def _pre_join_steps(self):
        """the student's iteration up to the point where the teacher's features are first read"""
        self._start_real_pass('d_real')
        yield
        self.forward()
        yield
        self.optimizer_D.zero_grad()
        yield from self._backward_D_steps()
        self._allreduce(self.optimizer_D)
        self.optimizer_D.step()
        self.D.repack()
        self.optimizer_G.zero_grad()
        yield
        yield from self._backward_G_head_steps()

    def _iteration_steps(self, input):
        """set_input + optimize_parameters of a model without a teacher of its own (the online teacher), as host-enqueue
        chunks for the student's scheduler"""
        self.set_input(input)
        self.finish_G_update()
        yield
        yield from self._pre_join_steps()
        # everything a student reads from this model is final here: the generator's features (forward), the discriminator's
        # weights (its Adam step + repack) and features (the D(fake) pass of backward_G's head)
        if getattr(self, '_head_done', None) is None:
            self._head_done = ops.Event()
        self._head_done.record()
        yield
        # GCC_DP_TEACHER_BUCKETS_LATE (default 1; data parallelism, teacher on its own stream): the teacher generator's gradient
        # buckets are NOT issued during its backward pass.  A communicator runs its collectives in issue order and the host
        # issues this whole iteration before the student's: buckets issued here would sit in front of the student's discriminator
        # buckets and make the student's main stream wait for the END of this backward pass at its D step's finish() (1.6 ms,
        # profiles/r5_dp_one_rank.txt).  The student issues them -- and the update behind them -- on this stream once its own
        # discriminator buckets are out (optimize_parameters); nothing reads this generator's weights before the arch step.
        red = self.optimizer_G.reducer
        hold = bool(DP_TEACHER_BUCKETS_LATE and self._defer_G_update and self._world > 1 and getattr(self, '_own_stream', False))
        if hold and red is not None:
            red.enabled = False
        try:
            self._backward_G_tail(None)
        finally:
            if red is not None:
                red.enabled = True
        if hold:
            self._pending_G = red or gdist.Deferred(self.optimizer_G, self._comm_group)
            self._held_G = True
            return
        if self._defer_G_update and self._world > 1:
            self._pending_G = self.optimizer_G.reducer or gdist.all_reduce_grads(self.optimizer_G, async_op=True, group=self._comm_group)
            if DP_TEACHER_UPDATE_EARLY and getattr(self, '_own_stream', False):
                # On a stream of its own (the online teacher's) nothing else is queued behind this iteration until the
                # architecture step: the wait for the buckets, Adam and the repack go here, where the stream idles, and not in
                # front of the arch step's forward, where the student's arch backward waits for them (round 5: +0.5 ms on the
                # critical chain of a data-parallel rank, profiles/r5_dp_one_rank.txt).  The main stream never waits for this.
                self.finish_G_update()
            return
        self._allreduce(self.optimizer_G)
        self._apply_G_update()

    def _apply_G_update(self):
        self.optimizer_G.step()          # L1_sparsity() (:554-563) is fused into the Adam kernel
        self._g_generation = getattr(self, '_g_generation', 0) + 1
        if self.T and isinstance(self.G, engine.UnetEngine):     # generator + transform convs: one repack launch (on the iteration's critical chain)
            if getattr(self, '_g_pack', None) is None:
                self._g_pack = ops.PackPlan(list(self.G.convs()) + list(self.T), self.device)
            self._g_pack.run()
        else:
            self.G.repack()
            for t in self.T:
                t.repack()

    def finish_G_update(self):
        if self._pending_G is not None:
            self._pending_G.wait()
            self._pending_G = None
            self._apply_G_update()

    # -- architecture step (models/Pix2Pix.py:479-511, 585-593) -----------------------------------------
    def get_D_arch_diff(self, isTeacher=False):
        """three hinge terms on one fake / real pair; the |.| difference (EMA'd for the teacher)"""
        mode = self.opt.gan_mode
        early = 'a_real' in getattr(self, '_early', {})
        cf = self._d_forward('a_fake', self._fake, refresh=not early)
        cr = self._take_real_pass('a_real')
        ops.gan_loss(mode, cf.pred, False, True, self._l('D_arch_fake'))
        ops.gan_loss(mode, cf.pred, True, False, self._l('D_arch_fake_real'))
        ops.gan_loss(mode, cr.pred, True, True, self._l('D_arch_real'))
        out = self._l('teacher_D_arch_diff' if isTeacher else 'D_arch_diff')
        w = 1.0
        if isTeacher and self._world > 1:
            # the teacher's difference feeds an EMA that every replica must hold identically -> the two hinge
            # means are summed over ranks (in place: the teacher logs neither) and the 1/world goes into the scalar op
            i = self._slot['D_arch_fake']
            assert self._slot['D_arch_fake_real'] == i + 1
            gdist.all_reduce_sum(self._lossvec[i:i + 2], group=self._comm_group)
            w = 1.0 / gdist.world_size()
        if isTeacher and self._ema_started:
            b = float(self.opt.ema_beta)
            ops.scalar_op(1, self._l('D_arch_fake_real'), self._l('D_arch_fake'), out, c=out, k0=b * w, k1=1.0 - b)
        elif w != 1.0:
            ops.scalar_op(1, self._l('D_arch_fake_real'), self._l('D_arch_fake'), out, c=out, k0=w, k1=0.0)
        else:
            ops.scalar_op(0, self._l('D_arch_fake_real'), self._l('D_arch_fake'), out)
        self._ema_started = True
        self.current_D_arch_diff_loss = out
        return cf, cr

    def backward_D_arch(self, ts=None):
        T = self.teacher_model
        if not ts:
            T.get_D_arch_diff(isTeacher=True)
        cf, cr = self.get_D_arch_diff(isTeacher=False)
        if ts:
            ops.wait_stream(ops.current_stream(), ts)          # the teacher's difference was computed on its stream
        if not (ts and ARCH_FREE_EARLY):
            ops.scalar_op(2, T._l('teacher_D_arch_diff'), T._l('teacher_D_arch_diff'), self._l('teacher_D_arch_diff'), k0=0.0)
            self._mark_teacher_free()
        # (else: the teacher's own stream copied the scalar and released itself at the end of its part, optimizer_netD_arch)
        # loss_D_arch = |d_S - d_T| + (L_real + L_fake)/2 ; coefficients of the three hinge gradients
        ops.arch_coeffs(self._l('D_arch_fake_real'), self._l('D_arch_fake'), self._l('D_arch_real'),
                        self._l('teacher_D_arch_diff'), self._l('D_arch'), self._l('arch_c_fr'), self._l('arch_c_f'))
        mode = self.opt.gan_mode
        gp = self.D.grad_pred_buffer(cf)
        ops.gan_loss(mode, cf.pred, True, False, self._l('scratch0'), dpred=gp, weight_dev=self._l('arch_c_fr'))
        ops.gan_loss(mode, cf.pred, False, True, self._l('scratch1'), dpred=gp, weight_dev=self._l('arch_c_f'),
                     dpred_accumulate=True)
        flat = getattr(self.optimizer_arch, 'flat', None)
        aux = self._aux_stream() if (ARCH_FORK and flat is not None and isinstance(self.D, engine.PatchGANEngine)) else False
        if aux:
            # the two passes are independent up to the sum of their alpha gradients: the pass over the real pair runs on the
            # auxiliary stream in gradient buffers of its own and accumulates into a zeroed copy of the arch optimizer's flat
            # gradient, which is added afterwards -- (0 + fake) + (0 + real), the bits of fake-then-real (each layer's sum
            # arrives in one add: bnact_bwd_finalize)
            side = self._arch_side_grads(flat)
            ops.wait_stream(aux, ops.current_stream())
            with ops.on_stream(aux):
                ops.fill(side[0], 0.0)
                gp1 = self.D.grad_pred_buffer(cr, slot=1)
                ops.gan_loss(mode, cr.pred, True, True, self._l('scratch2'), dpred=gp1, grad_weight=0.5)
                self.D.backward(cr, wgrad=False, agrad=True, need_dx=False, gslot=1, dalpha=side[1])
            self.D.backward(cf, wgrad=False, agrad=True, need_dx=False)
            ops.wait_stream(ops.current_stream(), aux)
            ops.add_f32_(flat.grads, side[0])
            return
        self.D.backward(cf, wgrad=False, agrad=True, need_dx=False)
        ops.gan_loss(mode, cr.pred, True, True, self._l('scratch2'), dpred=gp, grad_weight=0.5)
        self.D.backward(cr, wgrad=False, agrad=True, need_dx=False)

    def _arch_side_grads(self, flat):
        """(buffer shaped like the arch optimizer's flat gradient, {layer: view of it where that layer's alpha.grad sits})"""
        got = getattr(self, '_arch_side', None)
        if got is None or got[0].numel() != flat.grads.numel():
            buf = torch.zeros_like(flat.grads)
            views = {}
            for li, gate in enumerate(self.D.gate):
                if gate is not None:
                    g = gate.alpha.grad
                    off = (g.data_ptr() - flat.grads.data_ptr()) // 4
                    assert 0 <= off and off + g.numel() <= buf.numel() and g.is_contiguous()
                    views[li] = buf[off:off + g.numel()].view_as(g)
            got = self._arch_side = (buf, views)
        return got

    def optimizer_netD_arch(self):
        T = self.teacher_model
        ts = self._teacher_stream()

        def hand_over():
            # ARCH_FREE_EARLY: the last thing the student reads of the teacher in this step is its difference scalar -- the
            # teacher's stream copies it into the student's loss vector itself and is free from here (its next iteration then
            # starts behind its own architecture-step part, not behind the student's two discriminator forwards)
            if ts and ARCH_FREE_EARLY:
                ops.scalar_op(2, T._l('teacher_D_arch_diff'), T._l('teacher_D_arch_diff'), self._l('teacher_D_arch_diff'), k0=0.0)
                self._mark_teacher_free()

        def teacher_part():
            T.finish_G_update()
            T.set_input(self.input)
            T.forward()
            T.get_D_arch_diff(isTeacher=True)
            hand_over()

        if ts:
            self._release_teacher_stream(ts)
            with ops.on_stream(ts):
                teacher_part()
            self._start_real_pass('a_real')
            self.forward()
        else:
            self.forward()
            T.finish_G_update()
            T.set_input(self.input)
            T.forward()
        self.optimizer_arch.zero_grad()
        self.backward_D_arch(ts)
        self._allreduce(self.optimizer_arch)
        self.optimizer_arch.step()
        self.D.mask_dirty = True

    def clipping_mask_alpha(self):
        flat = getattr(getattr(self, 'optimizer_arch', None), 'flat', None)
        if flat is not None:
            ops.clamp_(flat.values, 0.0, 1.0)          # every alpha lives in the arch optimizer's flat buffer: one launch
        else:
            super().clipping_mask_alpha()
        self.D.mask_dirty = True

    # -- bookkeeping surface ----------------------------------------------------------------------
    def save_models(self, epoch, save_dir, fid=None, isbest=False, direction='AtoB'):
        self.finish_G_update()
        super().save_models(epoch, save_dir, fid, isbest, direction)

    def get_current_losses(self):
        """host read of the device loss scalars (the only sync of the iteration; print_freq cadence)"""
        v = self._lossvec.cpu()
        d = self._dist_out.cpu()
        ret = OrderedDict()
        for name in self.loss_names:
            if name == 'content':
                val = self.opt.lambda_content * float(d[:, 1].sum())
            elif name == 'gram':
                val = self.opt.lambda_gram * float(d[:, 0].sum())
            else:
                val = float(v[self._slot[name]])
            ret[name] = val
        if self._world > 1:
            ret = gdist.mean_dict(ret, self.device)
        return ret

    def get_distillation_features(self):
        """4 generator features (hooked modules of :366-369) + 2 discriminator features, as the
        tensors the reference's hooks end up holding (post in-place activation, hazard H1)"""
        return self.G.features(self._gctx) + self.D.features(self._dctx_g)

    # -- pruning cfgs (integer logic on host copies of the weights; models/Pix2Pix.py:742-952) -----------
    def _bn_sd(self):
        return {k: v.detach().cpu() for k, v in self.netG.state_dict().items() if k.endswith('.weight') and v.dim() == 1}

    def scale_prune_cfg(self, threshold):
        from ..utils import prune_util
        if torch.is_tensor(threshold):
            threshold = threshold.detach().cpu()
        return prune_util.scale_prune_cfg(self._bn_sd(), threshold, self.opt.ngf, self.opt.num_downs)

    def scale_prune(self, threshold):
        f, c = self.scale_prune_cfg(threshold)
        return Pix2PixModel(self.opt, filter_cfgs=f, channel_cfgs=c)

    def norm_prune(self, threshold):
        from ..utils import prune_util
        f, c = prune_util.norm_prune_cfg(self.netG, threshold, self.opt.ngf)
        return Pix2PixModel(self.opt, filter_cfgs=f, channel_cfgs=c)

    def resnet_prune(self, threshold):
        from ..utils import prune_util
        return Pix2PixModel(self.opt, filter_cfgs=prune_util.resnet_prune_cfg(self.netG, threshold, 'union'))

    def prune(self, threshold, lottery_path=None):
        """lottery_path is accepted and ignored: the reference's prune_util passes it (utils/prune_util.py:57) to a
        method that does not take it (models/Pix2Pix.py:742; SURVEY.md hazard H7)"""
        if self.opt.backbone == 'resnet':
            return self.resnet_prune(threshold)
        if self.opt.scale_prune:
            return self.scale_prune(threshold)
        if self.opt.norm_prune:
            return self.norm_prune(threshold)
        raise NotImplementedError('only scale and norm pruning are supported!!!')

    def max_min_bn_scale(self):
        from ..utils import prune_util
        return prune_util.max_min_bn_scale(self._bn_sd(), self.opt.num_downs)

    def max_min_conv_norm(self):
        from ..utils import prune_util
        if self.opt.backbone == 'resnet':
            return prune_util.max_min_conv_norm_resnet(self.netG, 'union')
        return prune_util.max_min_conv_norm_unet(self.netG)
