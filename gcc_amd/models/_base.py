"""What the four model families (Pix2Pix, CycleGAN, SAGAN, SRGAN) share: the bookkeeping surface of the reference's model
classes, the checkpoint dict, the architecture step and the SAGAN / SRGAN distillation block, once.

A family declares what differs as data -- NETS (its trained networks by checkpoint key: 'G' is ``self.netG``), METRIC (the
checkpoint's score key), CFGS (the attributes of its prune cfg pair), DISTILL_LOSSES / DISTILL_VISUALS (what init_distillation
appends) -- and supplies ``_engines()``, ``schedulers`` and its own slot list.  A method whose families differ by more than
data stays in the family's file."""
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import dist as gdist
from .. import engine, ops
from .._lib import GccError
from ..utils import util
from .DifferentiableOp import DifferentiableOP
from ._optim import _portable
from ._resume import TrainingStateMixin
from ._streams import TeacherStreamMixin

# loss-vector slots of one architecture step (CycleGAN has a set per side: these names + '_A' / '_B', in this order)
ARCH_SLOTS = {'fake': 'D_arch_fake', 'fake_real': 'D_arch_fake_real', 'real': 'D_arch_real', 'diff': 'D_arch_diff',
              'loss': 'D_arch', 'teacher_diff': 'teacher_D_arch_diff', 'c_fr': 'arch_c_fr', 'c_f': 'arch_c_f',
              's0': 'scratch0', 's1': 'scratch1', 's2': 'scratch2'}


class _ChainWgrad:
    """the weight-gradient launches stay on the stream of the chain that needs them instead of a side stream
    (engine.OVERLAP_WGRAD off for the duration of the step; restored afterwards: other model families of the process keep
    their side streams).  enabled=False: a no-op."""

    def __init__(self, enabled=True):
        self.enabled = enabled

    def __enter__(self):
        self.prev = engine.OVERLAP_WGRAD
        if self.enabled:
            engine.OVERLAP_WGRAD = False
        return self

    def __exit__(self, *exc):
        engine.OVERLAP_WGRAD = self.prev
        return False


class GANModelBase(TrainingStateMixin, TeacherStreamMixin, nn.Module):
    NETS = ('G', 'D')
    METRIC = 'fid'
    CFGS = ('filter_cfgs', 'channel_cfgs')
    DISTILL_LOSSES = (('lambda_content', ['content']), ('lambda_gram', ['gram']), ('lambda_L1', ['L1']))
    DISTILL_VISUALS = ()
    LR_REPORT = 'learning rate = %(lr).7f'

    # -- set-up helpers of the families' __init__ ------------------------------------------------------
    def _init_device(self, opt):
        self.opt = opt
        if len(opt.gpu_ids) == 0 or not torch.cuda.is_available():
            raise GccError('gcc_amd runs on MI355X only (no CPU path): need a visible GPU and gpu_ids >= 0')
        self.device = gdist.local_device(opt)
        ops.lib()                      # fail loudly here if libgcc_hip.so is not built

    def _init_losses(self, names, size=32):
        """device scalars: every loss of the iteration lives in one fp32 vector (read on demand)"""
        self._lossvec = torch.zeros(size, dtype=torch.float32, device=self.device)
        self._slot = {n: i for i, n in enumerate(names)}
        self._bufs = {}
        self._ema_started = False
        self._world = gdist.world_size()

    # -- small surface -----------------------------------------------------------------------------------
    def _l(self, name):
        i = self._slot[name]
        return self._lossvec[i:i + 1]

    def _buf(self, key, N, C, H, W):
        key = (key, N, C, H, W)
        if key not in self._bufs:
            self._bufs[key] = ops.new_act(N, C, H, W, self.device)
        return self._bufs[key]

    def _dws(self, i, N, C, HW):
        key = ('ws', i, N, C, HW)
        need = ops.distill_workspace_bytes(N, C, HW)       # depends on the weight-gradient split plan (tuning options)
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < need:
            buf = self._bufs[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return buf

    def _allreduce(self, optimizer):
        gdist.all_reduce_grads(optimizer)

    def adaptive_ema_beta(self, epoch):
        self.opt.ema_beta = 1.0 - epoch / (self.opt.n_epochs + self.opt.n_epochs_decay)

    def set_requires_grad(self, nets, requires_grad=False):
        for net in (nets if isinstance(nets, list) else [nets]):
            if net is not None:
                for p in net.parameters():
                    p.requires_grad = requires_grad

    def get_current_visuals(self):
        ret = OrderedDict()
        for name in self.visual_names:
            ret[name] = getattr(self, name)
        return ret

    def get_cfg(self):
        return tuple(getattr(self, n) for n in self.CFGS)

    # -- over the family's trained networks -----------------------------------------------------------------
    def _nets(self, kind=''):
        """(checkpoint key, module) of the trained networks whose key starts with `kind` ('G', 'D' or '': all)"""
        return [(k, getattr(self, 'net' + k)) for k in self.NETS if k.startswith(kind)]

    def model_train(self):
        for _, net in self._nets():
            net.train()

    def model_eval(self):
        for _, net in self._nets():
            net.eval()

    def save_models(self, epoch, save_dir, fid=None, isbest=False, direction='AtoB'):
        if gdist.rank() != 0:
            return
        util.mkdirs(save_dir)
        ckpt = {k: _portable(net.state_dict()) for k, net in self._nets()}
        ckpt.update({'epoch': epoch, 'cfg': self.get_cfg(), self.METRIC: fid})
        name = 'model_best_%s.pth' % direction if isbest else 'model_%d.pth' % epoch
        torch.save(ckpt, os.path.join(save_dir, name))

    def _load_checkpoint(self, load_path, load_discriminator):
        ckpt = torch.load(load_path, map_location='cpu')
        for k, net in self._nets('G') + (self._nets('D') if load_discriminator else []):
            net.load_state_dict(ckpt[k])
        self.refresh_weights()
        print('loading the model from %s' % load_path)
        return ckpt

    def load_models(self, load_path, load_discriminator=True):
        return self._load_checkpoint(load_path, load_discriminator)[self.METRIC], float('inf')

    def clipping_mask_alpha(self):
        for _, net in self._nets('D'):
            for m in net.modules():
                if isinstance(m, DifferentiableOP):
                    m.clip_alpha()

    def print_sparse_info(self, logger):
        for name, m in self.named_modules():
            if isinstance(m, DifferentiableOP):
                mask = m.get_current_mask()
                logger.info('%s sparsity ratio: %.2f' % (name, float((mask == 0.0).sum()) / mask.numel()))

    def refresh_weights(self):
        """re-derive the bf16 weight packings from the fp32 masters (after init / load / Adam)"""
        for e in self._engines():
            e.repack()

    def update_learning_rate(self, epoch):
        for s in self.schedulers:
            s.step()
        self.adaptive_ema_beta(epoch)
        lr = (self.optimizers or [self.optimizer_G])[0].param_groups[0]['lr']      # SAGAN's optimizers list is empty, as the reference's
        print(self.LR_REPORT % {'lr': lr, 'ema_beta': self.opt.ema_beta})

    def init_distillation(self):
        if self.distill:
            for lam, names in self.DISTILL_LOSSES:
                if getattr(self.opt, lam) > 0.0:
                    self.loss_names += names
            self.visual_names += self.DISTILL_VISUALS

    # -- architecture step ---------------------------------------------------------------------------------
    def _arch_diff(self, cf, cr, isTeacher, s=ARCH_SLOTS):
        """three hinge terms on one fake / real pair of discriminator contexts; the |.| difference (EMA'd for the teacher
        once it has a value: the caller sets _ema_started)"""
        mode = self.opt.gan_mode
        ops.gan_loss(mode, cf.pred, False, True, self._l(s['fake']))
        ops.gan_loss(mode, cf.pred, True, False, self._l(s['fake_real']))
        ops.gan_loss(mode, cr.pred, True, True, self._l(s['real']))
        out = self._l(s['teacher_diff' if isTeacher else 'diff'])
        if isTeacher and self._ema_started:
            b = float(self.opt.ema_beta)
            ops.scalar_op(1, self._l(s['fake_real']), self._l(s['fake']), out, c=out, k0=b, k1=1.0 - b)
        else:
            ops.scalar_op(0, self._l(s['fake_real']), self._l(s['fake']), out)

    def _arch_backward(self, D, cf, cr, s=ARCH_SLOTS, weight=0.5, grad_weight=1.0):
        """loss_D_arch = |d_S - d_T| + weight * (L_real + L_fake): coefficients of the three hinge gradients, then the two
        discriminator passes back to the alpha gates (grad_weight: of the real term)"""
        mode = self.opt.gan_mode
        ops.arch_coeffs(self._l(s['fake_real']), self._l(s['fake']), self._l(s['real']), self._l(s['teacher_diff']),
                        self._l(s['loss']), self._l(s['c_fr']), self._l(s['c_f']), weight=weight)
        gp = D.grad_pred_buffer(cf)
        ops.gan_loss(mode, cf.pred, True, False, self._l(s['s0']), dpred=gp, weight_dev=self._l(s['c_fr']))
        ops.gan_loss(mode, cf.pred, False, True, self._l(s['s1']), dpred=gp, weight_dev=self._l(s['c_f']),
                     dpred_accumulate=True)
        D.backward(cf, wgrad=False, agrad=True, need_dx=False)
        ops.gan_loss(mode, cr.pred, True, True, self._l(s['s2']), dpred=gp, grad_weight=grad_weight)
        D.backward(cr, wgrad=False, agrad=True, need_dx=False)

    def backward_D_arch(self, ts=None):
        T = self.teacher_model
        if not ts:
            T.get_D_arch_diff(isTeacher=True)
        cf, cr = self.get_D_arch_diff(isTeacher=False)
        self._join(ts)
        ops.scalar_op(2, T._l('teacher_D_arch_diff'), T._l('teacher_D_arch_diff'), self._l('teacher_D_arch_diff'), k0=0.0)
        self._mark_teacher_free()
        # loss_D_arch = |d_S - d_T| + L_real + L_fake  (no 1/2 here, models/SAGAN.py:388-389)
        self._arch_backward(self.D, cf, cr, weight=1.0)

    def optimizer_netD_arch(self):
        return self._optimizer_netD_arch()

    def _optimizer_netD_arch(self):
        T = self.teacher_model

        def teacher_part():
            T.set_input(self.input)
            T.forward()
            if self._teacher_stream():
                T.get_D_arch_diff(isTeacher=True)
        ts = self._run_teacher(teacher_part)
        self.forward()
        self.optimizer_arch.zero_grad()
        self.backward_D_arch(ts)
        self._allreduce(self.optimizer_arch)
        self.optimizer_arch.step()

    # -- distillation terms of a generator with one discriminator (SAGAN, SRGAN) ------------------------------------
    def _distill_terms(self, gc, ct, n):
        """gram / content terms on the generator's first n hooked features (through their transform convs) and on the features
        of the teacher discriminator's pass `ct` over the student's fake; returns the gradients w.r.t. the n generator
        features and dL/d(fake) from the teacher discriminator's backward pass"""
        opt, T = self.opt, self.teacher_model
        feats = self.G.features(gc) + T.D.features(ct)
        N = feats[0].shape[0]
        tf, dtf = [], []
        for i in range(n):
            f = feats[i]
            buf = self._buf(('tf', i), N, self.T[i].rows, f.shape[2], f.shape[3])
            self.T[i].forward(f, buf)
            tf.append(buf)
        tf += feats[n:]
        for i in range(len(tf)):
            dtf.append(self._buf(('dtf', i), N, tf[i].shape[1], tf[i].shape[2], tf[i].shape[3]))
            ws = self._dws(i, N, tf[i].shape[1], tf[i].shape[2] * tf[i].shape[3])
            t = self.target_distillation_features[i]
            ops.distill_fwd(tf[i], t, self._dist_out[i], ws)
            ops.distill_bwd(tf[i], t, opt.lambda_gram, opt.lambda_content, dtf[i], ws)
        g_feat = []
        for i in range(n):
            self.T[i].backward_weight(feats[i], dtf[i])
            gbuf = self._buf(('gf', i), N, feats[i].shape[1], feats[i].shape[2], feats[i].shape[3])
            self.T[i].backward_data(dtf[i], gbuf)
            g_feat.append(gbuf)
        ops.SideStream.get(self.device).join()
        return g_feat, T.D.backward(ct, has_pred_grad=False, g_feat=dtf[n:], wgrad=False, need_dx=True)
