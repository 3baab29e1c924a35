"""Training state of a model: everything a run holds between two iterations, captured and restored in place.

training_state() returns a dict of CPU objects (torch.save-able) that, loaded with load_training_state() into a model built the
same way (construction, pruning, teacher attach), continues the run with the same bits as the model it was taken from:
  * every trained net in the portable form save_models writes (NCHW fp32; BatchNorm buffers, SAGAN's weight_u / weight_v),
    and the distillation transform convs;
  * every HipAdam (torch.optim.Adam's state_dict format), every scheduler, the prune cfgs;
  * the host counters and scalars of the step: the U-Net's dropout seed counter, the EMA beta and the EMA's running value (the
    loss-vector slot the teacher's arch difference is averaged into), the CycleGAN image pools (device store + fill count),
    SRGAN's current epoch;
  * the attached online teacher's own training state, nested.
The host RNG streams (Python random, torch CPU / CUDA) belong to the training loop: gcc_amd.train saves them next to this.

Capture first finishes the deferred generator update and waits for every stream of the device; loading copies into the
existing parameter, buffer and optimizer-moment tensors (their addresses are baked into Adam plans, pack plans and recorded
replays) and repacks the bf16 weights."""
from collections import OrderedDict

import torch

from .._lib import GccError
from ._optim import HipAdam

_TRANSFORMS = ('transform_convs', 'transform_A_convs', 'transform_B_convs')
_CFGS = ('filter_cfgs', 'channel_cfgs', 'cfg_AtoB', 'cfg_BtoA')


def _cpu(sd):
    return OrderedDict((k, v.detach().to('cpu').contiguous()) for k, v in sd.items())


class TrainingStateMixin:

    def _state_nets(self):
        """name -> module of every trained network (registered submodules netG / netD / netG_A ..., and the transform convs)"""
        nets = OrderedDict((n, m) for n, m in self._modules.items() if n.startswith('net'))
        for name in _TRANSFORMS:
            for i, t in enumerate(getattr(self, name, None) or []):
                nets['%s.%d' % (name, i)] = t
        return nets

    def _state_optimizers(self):
        return OrderedDict((n, o) for n, o in sorted(vars(self).items()) if isinstance(o, HipAdam))

    def _state_schedulers(self):
        out = list(getattr(self, 'schedulers', []))
        arch = getattr(self, 'arch_scheduler', None)
        if arch is not None and all(arch is not s for s in out):
            out.append(arch)
        return out

    def _state_teacher(self):
        t = getattr(self, 'teacher_model', None)
        return t if (t is not None and self.opt.online_distillation) else None

    def _quiesce(self):
        """the state at an iteration boundary: deferred generator updates applied, every stream of the device drained"""
        for m in (self._state_teacher(), self):
            if m is not None and hasattr(m, 'finish_G_update'):
                m.finish_G_update()
            if m is not None and getattr(m, '_early', None):
                raise GccError('training_state(): a discriminator pass started early is still pending (%s)' % sorted(m._early))
        torch.cuda.synchronize(self.device)

    def training_state(self):
        self._quiesce()
        teacher = self._state_teacher()
        pools = getattr(self, 'pool', None) or {}
        return {
            'nets': OrderedDict((n, _cpu(m.state_dict())) for n, m in self._state_nets().items()),
            'optimizers': OrderedDict((n, o.state_dict()) for n, o in self._state_optimizers().items()),
            'schedulers': [s.state_dict() for s in self._state_schedulers()],
            'cfgs': tuple(getattr(self, n, None) for n in _CFGS),
            'seed': getattr(getattr(self, 'G', None), 'seed', None),
            'ema_beta': self.opt.ema_beta,
            'ema_started': self._ema_started,
            'lossvec': self._lossvec.detach().to('cpu').clone(),
            'current_epoch': getattr(self, 'current_epoch', None),
            'pools': OrderedDict((k, p.state()) for k, p in sorted(pools.items())),
            'teacher': teacher.training_state() if teacher is not None else None,
        }

    def load_training_state(self, state):
        self._quiesce()
        cfgs = tuple(getattr(self, n, None) for n in _CFGS)
        if tuple(state['cfgs']) != cfgs:
            raise GccError('training state was taken from a model pruned to %s, this one is %s' % (state['cfgs'], cfgs))
        nets, opts, scheds = self._state_nets(), self._state_optimizers(), self._state_schedulers()
        for what, mine, theirs in (('nets', nets, state['nets']), ('optimizers', opts, state['optimizers'])):
            if list(mine) != list(theirs):
                raise GccError('training state holds %s %s, this model has %s' % (what, list(theirs), list(mine)))
        if len(scheds) != len(state['schedulers']):
            raise GccError('training state holds %d schedulers, this model has %d' % (len(state['schedulers']), len(scheds)))
        pools = getattr(self, 'pool', None) or {}
        if sorted(pools) != sorted(state['pools']):
            raise GccError('training state holds image pools %s, this model has %s' % (sorted(state['pools']), sorted(pools)))
        teacher = self._state_teacher()
        if (teacher is None) != (state['teacher'] is None):
            raise GccError('training state %s an online teacher, this model %s' % (
                'holds' if state['teacher'] is not None else 'holds no', 'has none' if teacher is None else 'has one'))
        with torch.no_grad():
            for n, m in nets.items():
                m.load_state_dict(state['nets'][n])          # copy_ into the existing (flat-homed) tensors
            for n, o in opts.items():
                o.load_state_dict(state['optimizers'][n])
            self._lossvec.copy_(state['lossvec'])
        for s, sd in zip(scheds, state['schedulers']):
            s.load_state_dict(sd)
        if state['seed'] is not None:
            self.G.seed = int(state['seed'])
        self.opt.ema_beta = state['ema_beta']
        self._ema_started = bool(state['ema_started'])
        if state['current_epoch'] is not None:
            self.current_epoch = state['current_epoch']
        for k, p in pools.items():
            p.load_state(state['pools'][k], self.device)
        if teacher is not None:
            teacher.load_training_state(state['teacher'])
        self.refresh_weights()
        torch.cuda.synchronize(self.device)

    def rank_local_state(self):
        """the part of the state in which data-parallel replicas differ and that later iterations read: the image pools (each
        rank pools its own fakes).  BatchNorm running statistics are rank-local too but no training step reads them: a resumed
        rank takes rank 0's.  Call at an iteration boundary (_quiesce)."""
        teacher = self._state_teacher()
        return {'pools': OrderedDict((k, p.state()) for k, p in sorted((getattr(self, 'pool', None) or {}).items())),
                'teacher': teacher.rank_local_state() if teacher is not None else None}

    def load_rank_local_state(self, state):
        for k, p in (getattr(self, 'pool', None) or {}).items():
            p.load_state(state['pools'][k], self.device)
        teacher = self._state_teacher()
        if teacher is not None:
            teacher.load_rank_local_state(state['teacher'])
        torch.cuda.synchronize(self.device)
