"""DRN-D segmentation network (metric/drn.py arch 'D' under DRNSeg, metric/mIoU_score.py:124-157) from the reference's own
``--drn_path`` file, a plain state_dict, on the library's inference convolutions.

    x NCHW fp32 -> gcc_nchw_f32_to_nhwc_bf16 -> 7 x 7 stem, conv levels 1-2, residual levels 3-6, conv levels 7-8
        (gcc_conv_eval_ex: conv + folded BatchNorm + ReLU; a block's last conv: gcc_conv_fprop_eval + residual, gcc_relu_bf16)
        -> gcc_seg_head: 1 x 1 `seg` conv in fp32 -> scores; 8x `up` ConvTranspose2d + LogSoftmax -> log-probabilities

Dilation is a change of layout, not of kernel: a 3 x 3 conv of dilation d and padding d on an H x W map (H, W multiples of d)
is d^2 independent 3 x 3, padding-1 convs on the (H / d) x (W / d) sub-grids of equal (h mod d, w mod d).  In "phase layout" d
logical pixel (n, h, w) sits at batch index n d^2 + (h mod d) d + (w mod d), row h div d, column w div d, and the dilated conv is
the ordinary one with batch N d^2.  1 x 1 convs, BatchNorm, ReLU and residual sums do not care about the order of pixels, and in
arch D every 3 x 3 conv of a level has the level's dilation (level 5: 2, 6: 4, 7: 2, 8: 1), so the whole network needs four
gcc_phase_regroup launches: 1 -> 2, 2 -> 4, 4 -> 2, 2 -> 1.

precision='fp32' is the same network at the reference's own precision: NHWC fp32 activations and fp32 weights through
gcc_conv_eval_f32 (f32-input MFMA), where dilation is index arithmetic and the residual sum and the ReLU behind it are part of
the conv's epilogue -- no regroup and no separate ReLU launches:

    x NCHW fp32 -> gcc_nchw_f32_to_nhwc_f32 -> one gcc_conv_eval_f32 per convolution -> gcc_seg_head_f32

Construction parses the state_dict on the host (no device, no library); .to(device) packs the weights and folds the BatchNorms
once -- the weights of an evaluator never change."""
import re
from types import SimpleNamespace

import torch

from .. import ops
from .._lib import EVAL_ACT_NONE as NONE, EVAL_ACT_RELU as RELU, GccError
from ._native import Act, SlabProgramEngine, _shape, conv_shape

LEVEL_STRIDE = (1, 1, 2, 2, 2, 1, 1, 1, 1)          # base.0 .. base.8 (metric/drn.py:127-158)
LEVEL_DILATION = (1, 1, 1, 1, 1, 2, 4, 2, 1)
CONV_LEVELS = (1, 2, 7, 8)                           # Sequential(conv, BatchNorm, ReLU, ...); 3 .. 6 are residual blocks
HEAD_KEYS = ('base.0.0.weight', 'seg.weight', 'seg.bias', 'up.weight')
PRECISIONS = ('bf16', 'fp32')
BN_EPS = 1e-5                                        # nn.BatchNorm2d's default: a state_dict does not carry it
MAX_CLASSES = 64
WHAT = 'DRNSeg state_dict'
SIZE_MULTIPLE = 32                                   # 8x downsampling, then sub-grids of dilation 4

_BN = r'(?:weight|bias|running_mean|running_var|num_batches_tracked)'
_KEY_RES = [re.compile(p) for p in (
    r'base\.0\.0\.weight$', r'base\.0\.1\.' + _BN + '$',
    r'base\.[3456]\.\d+\.conv[123]\.weight$', r'base\.[3456]\.\d+\.bn[123]\.' + _BN + '$',
    r'base\.[3456]\.\d+\.downsample\.0\.weight$', r'base\.[3456]\.\d+\.downsample\.1\.' + _BN + '$',
    r'seg\.weight$', r'seg\.bias$', r'up\.weight$')]


_CONV_LEVEL_KEY = re.compile(r'base\.[1278]\.(\d+)\.(' + _BN[3:-1] + r')$')


def is_drn_seg_state_dict(sd):
    """a DRNSeg state_dict by its keys (arch D: base.0 is conv / BatchNorm)"""
    return isinstance(sd, dict) and all(k in sd for k in HEAD_KEYS)


def phase_index(n, h, w, d):
    """(batch index, row, column) of logical pixel (n, h, w) in phase layout d (ints or integer tensors)"""
    return n * d * d + (h % d) * d + (w % d), h // d, w // d


def to_phase(x, d):
    """phase layout d of an [N, C, H, W] tensor: [N d^2, C, H / d, W / d] (host restatement of gcc_phase_regroup(1 -> d))"""
    N, Cc, H, W = x.shape
    return x.reshape(N, Cc, H // d, d, W // d, d).permute(0, 3, 5, 1, 2, 4).reshape(N * d * d, Cc, H // d, W // d)


def from_phase(x, d):
    """inverse of to_phase"""
    Nd, Cc, h, w = x.shape
    N = Nd // (d * d)
    return x.reshape(N, d, d, Cc, h, w).permute(0, 3, 4, 1, 5, 2).reshape(N, Cc, h * d, w * d)


class _Conv:
    """one convolution of the network with the BatchNorm behind it: key of its weight, prefix of the BatchNorm's keys"""

    def __init__(self, key, bn, k, stride, pad, relu):
        self.key, self.bn, self.k, self.stride, self.pad, self.relu = key, bn, k, stride, pad, relu
        self.co = self.ci = 0


def parse_drn_seg(sd):
    """the architecture of a DRNSeg state_dict (values: tensors, or bare shapes) from its keys and shapes: SimpleNamespace(kind
    'bottleneck' | 'basic', depths[8] (convs of levels 1, 2, 7, 8; blocks of levels 3-6), widths[8], strides[8], dilations[8],
    classes, levels).  levels[L] (L = 0 .. 8) is a list of _Conv (conv levels) or of blocks SimpleNamespace(convs, downsample).
    Raises GccError naming the first key that does not belong to an arch-D DRNSeg."""
    if not isinstance(sd, dict):
        raise GccError('DRNSeg state_dict: expected a dict, got %s' % type(sd).__name__)
    for key in sd:
        if key == 'base.0.weight':
            raise GccError('DRNSeg state_dict: %s: base.0 is a bare convolution, which is DRN arch C; only arch D (drn_d_*) '
                           'is built here' % key)
        m = _CONV_LEVEL_KEY.match(key)
        if m:       # conv levels are Sequential(conv, BatchNorm, ReLU, ...): 3 j is a bias-free conv, 3 j + 1 its BatchNorm
            slot, field = int(m.group(1)) % 3, m.group(2)
            if (slot == 0 and field == 'weight') or slot == 1:
                continue
        if not any(r.match(key) for r in _KEY_RES):
            raise GccError('DRNSeg state_dict: unknown key %s' % key)
    for key in HEAD_KEYS:
        if key not in sd:
            raise GccError('DRNSeg state_dict: %s is missing' % key)

    def conv(key, bn, k, stride, relu=True):
        c = _Conv(key, bn, k, stride, k // 2, relu)
        c.co, c.ci = conv_shape(sd, WHAT, key, bn, (k, k))
        return c

    def indices(prefix):
        idx = set()
        for key in sd:
            if key.startswith(prefix):
                idx.add(int(key[len(prefix):].split('.')[0]))
        return sorted(idx)

    kind = 'bottleneck' if any(re.match(r'base\.[3456]\.\d+\.conv3\.weight$', k) for k in sd) else 'basic'
    levels = [[conv('base.0.0.weight', 'base.0.1', 7, 1)]]
    cin = 3

    def chain(c):
        nonlocal cin
        if c.ci != cin:
            raise GccError('DRNSeg state_dict: %s takes %d channels, the layer before it gives %d' % (c.key, c.ci, cin))
        cin = c.co
    chain(levels[0][0])
    for L in range(1, 9):
        pre, s = 'base.%d.' % L, LEVEL_STRIDE[L]
        idx = indices(pre)
        if not idx:
            raise GccError('DRNSeg state_dict: %s0 is missing: every level of arch D must be present' % pre)
        items = []
        if L in CONV_LEVELS:
            n = max(idx) // 3 + 1
            for j in range(n):
                c = conv('%s%d.weight' % (pre, 3 * j), '%s%d' % (pre, 3 * j + 1), 3, s if j == 0 else 1)
                chain(c)
                items.append(c)
        else:
            if idx != list(range(len(idx))):
                raise GccError('DRNSeg state_dict: %s%d is missing' % (pre, next(i for i in range(len(idx)) if i not in idx)))
            for b in idx:
                p, sb = '%s%d.' % (pre, b), (s if b == 0 else 1)
                if kind == 'bottleneck':
                    convs = [conv(p + 'conv1.weight', p + 'bn1', 1, 1), conv(p + 'conv2.weight', p + 'bn2', 3, sb),
                             conv(p + 'conv3.weight', p + 'bn3', 1, 1, relu=False)]
                else:
                    if p + 'conv3.weight' in sd:
                        raise GccError('DRNSeg state_dict: unknown key %sconv3.weight' % p)
                    convs = [conv(p + 'conv1.weight', p + 'bn1', 3, sb), conv(p + 'conv2.weight', p + 'bn2', 3, 1, relu=False)]
                block_in = cin
                for c in convs:
                    chain(c)
                ds = None
                if p + 'downsample.0.weight' in sd:
                    ds = conv(p + 'downsample.0.weight', p + 'downsample.1', 1, sb, relu=False)
                    if ds.ci != block_in or ds.co != cin:
                        raise GccError('DRNSeg state_dict: %s maps %d to %d channels, its block maps %d to %d'
                                       % (ds.key, ds.ci, ds.co, block_in, cin))
                elif block_in != cin or sb != 1:
                    raise GccError('DRNSeg state_dict: %sdownsample.0.weight is missing (the block maps %d to %d channels at '
                                   'stride %d)' % (p, block_in, cin, sb))
                items.append(SimpleNamespace(convs=convs, downsample=ds))
        levels.append(items)
    sw, sb_, uw = _shape(sd['seg.weight']), _shape(sd['seg.bias']), _shape(sd['up.weight'])
    if len(sw) != 4 or sw[1:] != (cin, 1, 1):
        raise GccError('DRNSeg state_dict: seg.weight has shape %s, expected (classes, %d, 1, 1)' % (sw, cin))
    classes = sw[0]
    if classes > MAX_CLASSES:
        raise GccError('DRNSeg state_dict: seg.weight has %d classes; the head takes at most %d' % (classes, MAX_CLASSES))
    if sb_ != (classes,):
        raise GccError('DRNSeg state_dict: seg.bias has shape %s, expected (%d,)' % (sb_, classes))
    if uw != (classes, 1, 16, 16):
        raise GccError('DRNSeg state_dict: up.weight has shape %s, expected (%d, 1, 16, 16)' % (uw, classes))
    first = lambda L: levels[L][0] if L in CONV_LEVELS else levels[L][0].convs[0]
    return SimpleNamespace(kind=kind, depths=[len(levels[L]) for L in range(1, 9)], widths=[first(L).co for L in range(1, 9)],
                           strides=list(LEVEL_STRIDE[1:]), dilations=list(LEVEL_DILATION[1:]), classes=classes, levels=levels,
                           out_channels=cin)


def _all_convs(arch):
    out = [arch.levels[0][0]]
    for L in range(1, 9):
        for it in arch.levels[L]:
            if isinstance(it, _Conv):
                out.append(it)
            else:
                out.extend(it.convs)
                if it.downsample is not None:
                    out.append(it.downsample)
    return out


class DrnSegEngine(SlabProgramEngine):
    """segmenter(x) for cityscapes._Batcher / mIoU_score.test: x NCHW fp32 [N, 3, H, W] (H, W multiples of 32) ->
    (log-softmax [N, C, H, W] fp32, scores [N, C, H / 8, W / 8] fp32), DRNSeg.forward's tuple.  Activations are bf16 with one
    rounding per conv + BatchNorm (+ ReLU) and per residual sum; the head is fp32.  precision='fp32': activations, weights and
    every sum are fp32 (the reference's own arithmetic), one launch per convolution.  The engine's scaffold -- .to(), the slab
    and its programs, the route check -- is metric/_native.py's."""
    BN_EPS = BN_EPS

    def __init__(self, state_dict, precision='bf16'):
        if precision not in PRECISIONS:
            raise GccError('DrnSegEngine: precision %r; expected one of %s' % (precision, ', '.join(PRECISIONS)))
        self.precision = precision
        if precision == 'fp32':
            self._slab_dtype = torch.float32
        self.arch = parse_drn_seg(state_dict)
        super().__init__(state_dict, _all_convs(self.arch), HEAD_KEYS)
        self.classes = self.arch.classes

    # ---- host -> device: once -------------------------------------------------------------------------------------------
    def _pack(self, c, master):
        return ops.pack_weights_f32(master) if self.precision == 'fp32' else super()._pack(c, master)

    def _to_extra(self, device):
        self.seg_w = self.host['seg.weight'].reshape(self.classes, -1).contiguous().to(device)
        self.seg_b = self.host['seg.bias'].to(device)
        self.up_w = self.host['up.weight'].reshape(self.classes, 256).contiguous().to(device)

    # ---- the launch program of one input size ---------------------------------------------------------------------------
    def _plan(self, N, H, W):
        """the launches of an [N, 3, H, W] input as a list of tuples over activations of the slab (four regions the layers rotate
        through, behind the input's 3 channels in an ld of 8, or of 4 in fp32).  bf16: ('conv', conv, source, destination,
        residual), ('relu', a) behind a block's last conv, ('regroup', a, b) where the level's dilation changes.  fp32: only
        ('conv', conv, source, destination, residual, dilation, relu): every activation is in the logical layout, and a block's
        last conv adds the residual and applies the ReLU in its own epilogue."""
        f32 = self.precision == 'fp32'
        steps, shapes = [], []                             # sizes first: the largest activation decides the region
        R = 4
        live = SimpleNamespace(h=H, w=W, d=1)

        def act(Cc, region):
            """symbolic activation: Cc channels of the current logical size in the current layout"""
            shapes.append(N * live.h * live.w * Cc)
            return Act(Cc, live.h, live.w, region, d=live.d)

        def pick(*avoid):
            used = set(a.region for a in avoid if a is not None)
            return next(r for r in range(R) if r not in used)

        def run_conv(c, src, dst, residual=None):
            st = ('conv', c, src, dst, residual)
            if f32:                                        # dilation rides on the step, and so does the ReLU behind the sum
                st += (dil if c.k > 1 else 1, c.relu or residual is not None)
            steps.append(st)

        ld_in = 4 if f32 else 8
        x = Act(3, H, W, -1, ld=ld_in)
        for L in range(9):
            dil = LEVEL_DILATION[L]
            if dil != live.d and not f32:                  # bf16: dilation is a change of layout
                live.d = dil
                y = act(x.C, pick(x))
                steps.append(('regroup', x, y))
                x = y
            for it in self.arch.levels[L]:
                blk = [it] if isinstance(it, _Conv) else it.convs
                s = max(c.stride for c in blk)
                if s != 1 and live.d != 1:
                    raise GccError('DrnSegEngine: %s has stride %d inside a dilated level' % (blk[0].key, s))
                cur = x
                for c in blk[:-1]:
                    live.h, live.w = live.h // c.stride, live.w // c.stride
                    y = act(c.co, pick(x, cur))
                    run_conv(c, cur, y)
                    cur = y
                live.h, live.w = live.h // blk[-1].stride, live.w // blk[-1].stride
                res = None
                if not isinstance(it, _Conv):
                    res = x
                    if it.downsample is not None:
                        # the block's inner activations other than `cur` are dead once `cur` exists: their regions may be reused
                        res = act(it.downsample.co, pick(x, cur))
                        run_conv(it.downsample, x, res)
                y = act(blk[-1].co, pick(x, cur, res))
                run_conv(blk[-1], cur, y, residual=res)
                if res is not None and not f32:
                    steps.append(('relu', y))
                x = y
        if live.d != 1:
            raise GccError('DrnSegEngine: the last level leaves phase layout %d' % live.d)
        size_in, size_r = N * H * W * ld_in, max(shapes)
        return SimpleNamespace(steps=steps, size_in=size_in, size_r=size_r, total=size_in + R * size_r, last=x, slab=None,
                               h=live.h, w=live.w, x_in=None)

    def _conv(self, st, route_only=False):
        """launch the 'conv' step st, or with route_only the library's answer for it: its launches, -1 if it declines"""
        c, src, dst, res = st[1:5]
        if self.precision == 'fp32':
            dil, relu = st[5:]
            rc = ops.conv_eval_f32(src.view, c.w, c.co, c.k, c.stride, dil * (c.k // 2), dst.view, dilation=dil, scale=c.scale,
                                   shift=c.shift, act=RELU if relu else NONE, residual=res.view if res is not None else None,
                                   route_only=route_only)
            return (1 if rc >= 0 else -1) if route_only else rc          # the route's answer is a tile: always one launch
        if res is None:
            return ops.conv_eval_ex(src.view, c.w, c.co, c.k, c.stride, c.pad, dst.view, scale=c.scale, shift=c.shift,
                                    act=RELU if c.relu else NONE, slot='drn_eval', route_only=route_only)
        return ops.conv_fprop_eval(src.view, c.w, c.co, c.k, c.stride, c.pad, dst.view, scale=c.scale, shift=c.shift, act=NONE,
                                   residual=res.view, slot='drn_eval', route_only=route_only)

    def _declined(self, st):
        c, src = st[1:3]
        on = tuple(src.view.shape[i] for i in (0, 2, 3))
        if self.precision == 'fp32':
            return ('DrnSegEngine: the library declines the fp32 geometry of %s (%d -> %d channels, %d x %d, stride %d, dilation '
                    '%d, on %d x %d x %d): there is no other route' % ((c.key, c.ci, c.co, c.k, c.k, c.stride, st[5]) + on))
        return ('DrnSegEngine: the library declines the geometry of %s (%d -> %d channels, %d x %d, stride %d, on %d x %d x %d): '
                'there is no other route' % ((c.key, c.ci, c.co, c.k, c.k, c.stride) + on))

    @staticmethod
    def _check_size(H, W):
        if H % SIZE_MULTIPLE or W % SIZE_MULTIPLE or H <= 0 or W <= 0:
            raise GccError('DrnSegEngine: input of %d x %d; H and W must be multiples of %d (8x downsampling, then the sub-grids '
                           'of dilation 4)' % (H, W, SIZE_MULTIPLE))

    def _run(self, x, N, H, W, count_only=False):
        self._check_size(H, W)
        self._check_device()
        prog = self._bind(N, H, W)
        f32 = self.precision == 'fp32'
        if count_only:                                     # the input, the steps, the head's two
            return 1 + sum(self._conv(st, route_only=True) if st[0] == 'conv' else 1 for st in prog.steps) + 2
        if f32:
            ops.nchw_to_nhwc_f32(x, prog.x_in, 4)
        else:
            ops.nchw_to_nhwc(x, prog.x_in, 0, 8)
        for st in prog.steps:
            if st[0] == 'conv':
                try:
                    self._conv(st)
                except GccError as e:
                    raise self._conv_error(st, e)
            elif st[0] == 'relu':
                ops.relu_(st[1].view)
            else:
                _, a, b = st
                ops.phase_regroup(a.view, b.view, a.d, b.d)
        scores = torch.empty((N, self.classes, prog.h, prog.w), dtype=torch.float32, device=self.device)
        logp = torch.empty((N, self.classes, H, W), dtype=torch.float32, device=self.device)
        (ops.seg_head_f32 if f32 else ops.seg_head)(prog.last.view, self.seg_w, self.seg_b, self.up_w, scores, logp)
        return logp, scores

    def __call__(self, x):
        self._check_input(x)
        N, _, H, W = x.shape
        self._check_size(H, W)
        self._check_device(x)
        return self._run(x.contiguous(), N, H, W)

    def infer_launches(self, N, H, W):
        """kernel launches of one call on an [N, 3, H, W] input, from the library's route introspection (launches nothing)"""
        return self._run(None, N, H, W, count_only=True)

    def flops(self, H, W):
        """multiply-adds x 2 of one image from the shapes (convolutions and the seg conv; the streaming kernels not counted)"""
        prog = self._program(1, H, W)
        total = sum(2 * st[3].h * st[3].w * st[1].co * st[1].ci * st[1].k * st[1].k for st in prog.steps if st[0] == 'conv')
        return total + 2 * prog.h * prog.w * self.classes * self.arch.out_channels
