"""The optimizer of every model family and the portable form of a state_dict (what a checkpoint stores)."""
from collections import OrderedDict

import torch

from .. import engine, ops
from .._lib import GccError


class HipAdam(torch.optim.Optimizer):
    """torch.optim.Optimizer facade (so LambdaLR/StepLR schedulers work unchanged) whose step() is
    one multi-tensor gcc_adam_step launch over a FlatParams group."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, l1=None, dup=(), layout=None):
        """dup: parameters (members of params) the reference lists twice in this optimizer (SAGAN, SURVEY.md hazard
        H5): torch's Adam then applies two sequential updates per step to them, with the same gradient and the step
        counter advancing twice -- reproduced by a second plan over those tensors that is stepped twice."""
        params = list(params)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        dev = params[0].device
        self.flat = engine.FlatParams(params, dev, layout=layout)
        self.reducer = None         # dist.GradReducer under data parallelism (Pix2PixModel sets it)
        l1 = list(l1) if l1 is not None else [0.0] * len(params)
        dup_ids = {id(p) for p in dup}
        once = [i for i, p in enumerate(params) if id(p) not in dup_ids]
        twice = [i for i, p in enumerate(params) if id(p) in dup_ids]
        pick = lambda idx, seq: [seq[i] for i in idx]
        self.plan = ops.AdamPlan(pick(once, params), pick(once, self.flat.grad_views), dev, l1=pick(once, l1)) if once else None
        self.plan_dup = ops.AdamPlan(pick(twice, params), pick(twice, self.flat.grad_views), dev, l1=pick(twice, l1)) if twice else None
        # optimizer order -> (plan, index in the plan): where parameter i's exp_avg / exp_avg_sq / step live
        self._where = [None] * len(params)
        for plan, idx in ((self.plan, once), (self.plan_dup, twice)):
            for j, i in enumerate(idx):
                self._where[i] = (plan, j)

    def zero_grad(self, set_to_none=False):
        self.flat.zero_grad()

    def set_grad_scale(self, s):
        for plan in (self.plan, self.plan_dup):
            if plan is not None:
                plan.set_grad_scale(s)

    @torch.no_grad()
    def step(self, closure=None):
        g = self.param_groups[0]
        if self.plan is not None:
            self.plan.step(g['lr'], g['betas'], g['eps'])
        if self.plan_dup is not None:
            self.plan_dup.step(g['lr'], g['betas'], g['eps'])
            self.plan_dup.step(g['lr'], g['betas'], g['eps'])

    def state_dict(self):
        """torch.optim.Adam's format: state[i] = {'step', 'exp_avg', 'exp_avg_sq'} per parameter in optimizer order (logical
        NCHW-contiguous fp32 CPU tensors; none before the first step, as torch), param_groups packed as torch packs them.  A
        parameter of plan_dup is one entry whose step advances twice per step(), as torch's Adam counts a twice-listed one.
        Reads the device moments: the caller orders this behind the last step (a device synchronize)."""
        packed = super().state_dict()
        state = {}
        for i, (plan, j) in enumerate(self._where):
            if plan.step_count > 0:
                state[i] = {'step': torch.tensor(float(plan.step_count)),
                            'exp_avg': plan.m[j].detach().to('cpu').contiguous(),
                            'exp_avg_sq': plan.v[j].detach().to('cpu').contiguous()}
        return {'state': state, 'param_groups': packed['param_groups']}

    def load_state_dict(self, state_dict):
        """the inverse of state_dict(), in place: the moments are COPIED into the existing AdamPlan.m / v tensors (their device
        pointers are baked into the plans' descriptor lists and into recorded replays) and step_count is restored"""
        groups = state_dict['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != len(self._where):
            raise GccError('optimizer state holds %s parameters, this optimizer has %d'
                           % ([len(g['params']) for g in groups], len(self._where)))
        state = state_dict['state']
        steps = {}
        for i, (plan, j) in enumerate(self._where):
            s = state.get(i, state.get(str(i)))
            if s is None:
                steps.setdefault(id(plan), set()).add(0)
                continue
            steps.setdefault(id(plan), set()).add(int(float(s['step'])))
            for dst, key in ((plan.m[j], 'exp_avg'), (plan.v[j], 'exp_avg_sq')):
                src = s[key]
                if tuple(src.shape) != tuple(dst.shape):
                    raise GccError('optimizer state of parameter %d: %s is %s, the parameter is %s'
                                   % (i, key, tuple(src.shape), tuple(dst.shape)))
                dst.copy_(src.to(dst.dtype))
        for plan in (self.plan, self.plan_dup):
            if plan is None:
                continue
            got = steps.get(id(plan), {0})
            if len(got) != 1:
                raise GccError('optimizer state: the parameters of one group disagree on their step count (%s)' % sorted(got))
            plan.step_count = got.pop()
            if plan.step_count == 0:
                for t in plan.m + plan.v:
                    t.zero_()
        self.param_groups[0].update({k: v for k, v in groups[0].items() if k != 'params'})


def _portable(sd):
    """NCHW-contiguous fp32 CPU copies, as a reference checkpoint stores them"""
    return OrderedDict((k, v.detach().to('cpu').contiguous()) for k, v in sd.items())
