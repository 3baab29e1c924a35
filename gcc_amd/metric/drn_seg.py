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
import ctypes as C
import re
from types import SimpleNamespace

import torch

from .._lib import GccError

LEVEL_STRIDE = (1, 1, 2, 2, 2, 1, 1, 1, 1)          # base.0 .. base.8 (metric/drn.py:127-158)
LEVEL_DILATION = (1, 1, 1, 1, 1, 2, 4, 2, 1)
CONV_LEVELS = (1, 2, 7, 8)                           # Sequential(conv, BatchNorm, ReLU, ...); 3 .. 6 are residual blocks
HEAD_KEYS = ('base.0.0.weight', 'seg.weight', 'seg.bias', 'up.weight')
BN_FIELDS = ('weight', 'bias', 'running_mean', 'running_var')
PRECISIONS = ('bf16', 'fp32')
BN_EPS = 1e-5                                        # nn.BatchNorm2d's default: a state_dict does not carry it
MAX_CLASSES = 64
SIZE_MULTIPLE = 32                                   # 8x downsampling, then sub-grids of dilation 4

_BN = r'(?:weight|bias|running_mean|running_var|num_batches_tracked)'
_KEY_RES = [re.compile(p) for p in (
    r'base\.0\.0\.weight$', r'base\.0\.1\.' + _BN + '$',
    r'base\.[3456]\.\d+\.conv[123]\.weight$', r'base\.[3456]\.\d+\.bn[123]\.' + _BN + '$',
    r'base\.[3456]\.\d+\.downsample\.0\.weight$', r'base\.[3456]\.\d+\.downsample\.1\.' + _BN + '$',
    r'seg\.weight$', r'seg\.bias$', r'up\.weight$')]


_CONV_LEVEL_KEY = re.compile(r'base\.[1278]\.(\d+)\.(' + _BN[3:-1] + r')$')


def _shape(v):
    return tuple(v.shape) if hasattr(v, 'shape') else tuple(v)


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
        if key not in sd:
            raise GccError('DRNSeg state_dict: %s is missing' % key)
        for f in BN_FIELDS:
            if '%s.%s' % (bn, f) not in sd:
                raise GccError('DRNSeg state_dict: %s.%s is missing (BatchNorm behind %s)' % (bn, f, key))
        c = _Conv(key, bn, k, stride, k // 2, relu)
        s = _shape(sd[key])
        if len(s) != 4 or s[2] != k or s[3] != k:
            raise GccError('DRNSeg state_dict: %s has shape %s, expected a %d x %d convolution' % (key, s, k, k))
        c.co, c.ci = s[0], s[1]
        if c.co % 8:
            raise GccError('DRNSeg state_dict: %s has %d output channels; widths must be multiples of 8' % (key, c.co))
        for f in BN_FIELDS:
            if _shape(sd['%s.%s' % (bn, f)]) != (c.co,):
                raise GccError('DRNSeg state_dict: %s.%s has shape %s, expected (%d,)' % (bn, f, _shape(sd['%s.%s' % (bn, f)]), c.co))
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


class DrnSegEngine:
    """segmenter(x) for cityscapes._Batcher / mIoU_score.test: x NCHW fp32 [N, 3, H, W] (H, W multiples of 32) ->
    (log-softmax [N, C, H, W] fp32, scores [N, C, H / 8, W / 8] fp32), DRNSeg.forward's tuple.  Activations are bf16 with one
    rounding per conv + BatchNorm (+ ReLU) and per residual sum; the head is fp32.  precision='fp32': activations, weights and
    every sum are fp32 (the reference's own arithmetic), one launch per convolution."""

    def __init__(self, state_dict, precision='bf16'):
        if precision not in PRECISIONS:
            raise GccError('DrnSegEngine: precision %r; expected one of %s' % (precision, ', '.join(PRECISIONS)))
        self.precision = precision
        self.arch = parse_drn_seg(state_dict)
        self.convs = _all_convs(self.arch)
        keys = set(c.key for c in self.convs) | set('%s.%s' % (c.bn, f) for c in self.convs for f in BN_FIELDS) | set(HEAD_KEYS)
        self.host = {k: state_dict[k].detach().to('cpu', torch.float32).contiguous() for k in keys}
        self.classes = self.arch.classes
        self.device = None
        self._slab, self._programs = None, {}

    # ---- host -> device: once -------------------------------------------------------------------------------------------
    def to(self, device):
        from .. import ops
        device = torch.device(device)
        if device.type != 'cuda':
            raise GccError('DrnSegEngine runs on the GPU only (asked for %s)' % device)
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self.device == device:
            return self
        self.device = device
        self._slab, self._programs = None, {}
        with torch.cuda.device(device):
            n = sum(c.co for c in self.convs)
            self._bn = torch.empty((4, n), dtype=torch.float32)
            off = 0
            for c in self.convs:
                for i, f in enumerate(BN_FIELDS):
                    self._bn[i, off:off + c.co] = self.host['%s.%s' % (c.bn, f)]
                off += c.co
            self._bn = self._bn.to(device)
            entries, off = [], 0
            for c in self.convs:
                g, b, rm, rv = (self._bn[i, off:off + c.co] for i in range(4))
                entries.append((SimpleNamespace(weight=g, bias=b, running_mean=rm, running_var=rv, eps=BN_EPS), None, c.co))
                off += c.co
                if self.precision == 'fp32':
                    c.w = ops.pack_weights_f32(self.host[c.key].to(device))
                    continue
                master = self.host[c.key].to(device).contiguous(memory_format=torch.channels_last)
                c.w, _ = ops.pack_weights(master, want_w=True, want_wt=False)
            self._table = ops.BNEvalTable(entries, device)
            self._table.run()
            for i, c in enumerate(self.convs):
                c.scale, c.shift = self._table.scale[i], self._table.shift[i]
            self.seg_w = self.host['seg.weight'].reshape(self.classes, -1).contiguous().to(device)
            self.seg_b = self.host['seg.bias'].to(device)
            self.up_w = self.host['up.weight'].reshape(self.classes, 256).contiguous().to(device)
        return self

    def eval(self):
        return self

    # ---- the launch program of one input size ---------------------------------------------------------------------------
    def _program(self, N, H, W):
        """the launches of an [N, 3, H, W] input as a list of tuples over views of the activation slab (grow-only; four regions
        the layers rotate through, behind the 8-channel input)"""
        key = (N, H, W)
        prog = self._programs.get(key)
        if prog is not None:
            return prog
        if self.precision == 'fp32':
            prog = self._programs[key] = self._program_f32(N, H, W)
            return prog
        # sizes first: the largest activation decides the region
        steps, shapes = [], []
        size_in = N * H * W * 8
        R = 4
        live = SimpleNamespace(h=H, w=W, d=1)

        def act(Cc, region):
            """symbolic activation: Cc channels of the current logical size in the current layout"""
            shapes.append(N * live.h * live.w * Cc)
            return SimpleNamespace(C=Cc, region=region, h=live.h, w=live.w, d=live.d, view=None)

        def pick(*avoid):
            used = set(a.region for a in avoid if a is not None)
            return next(r for r in range(R) if r not in used)

        def run_conv(c, src, dst, residual=None):
            steps.append(('conv', c, src, dst, residual))

        x = SimpleNamespace(C=3, region=-1, h=H, w=W, d=1, view=None)
        for L in range(9):
            d = LEVEL_DILATION[L]
            if d != live.d:
                y = SimpleNamespace(C=x.C, region=pick(x), h=live.h, w=live.w, d=d, view=None)
                shapes.append(N * live.h * live.w * x.C)
                steps.append(('regroup', x, y))
                live.d, x = d, y
            for it in self.arch.levels[L]:
                blk = [it] if isinstance(it, _Conv) else it.convs
                s = max(c.stride for c in blk)
                if s != 1 and live.d != 1:
                    raise GccError('DrnSegEngine: %s has stride %d inside a dilated level' % (blk[0].key, s))
                if isinstance(it, _Conv):
                    live.h, live.w = live.h // s, live.w // s
                    y = act(it.co, pick(x))
                    run_conv(it, x, y)
                    x = y
                    continue
                cur = x
                for c in blk[:-1]:
                    live.h, live.w = live.h // c.stride, live.w // c.stride
                    y = act(c.co, pick(x, cur))
                    run_conv(c, cur, y)
                    cur = y
                res = x
                if it.downsample is not None:
                    # the block's inner activations other than `cur` are dead once `cur` exists: their regions may be reused
                    res = act(it.downsample.co, pick(x, cur))
                    run_conv(it.downsample, x, res)
                y = act(blk[-1].co, pick(x, cur, res))
                run_conv(blk[-1], cur, y, residual=res)
                steps.append(('relu', y))
                x = y
        if live.d != 1:
            raise GccError('DrnSegEngine: the last level leaves phase layout %d' % live.d)
        size_r = max(shapes)
        prog = SimpleNamespace(steps=steps, size_in=size_in, size_r=size_r, total=size_in + R * size_r, last=x, slab=None,
                               h=live.h, w=live.w)
        self._programs[key] = prog
        return prog

    def _program_f32(self, N, H, W):
        """the fp32 route's launches: ('conv', conv, source, destination, residual, dilation, relu) over views of an fp32 slab
        (the same four regions, behind the input's 3 channels in an ld of 4).  Every activation is in the logical layout; a
        block's last conv adds the residual and applies the ReLU in its own epilogue."""
        steps, shapes = [], []
        R = 4
        live = SimpleNamespace(h=H, w=W)

        def act(Cc, region):
            shapes.append(N * live.h * live.w * Cc)
            return SimpleNamespace(C=Cc, region=region, h=live.h, w=live.w, d=1, view=None)

        def pick(*avoid):
            used = set(a.region for a in avoid if a is not None)
            return next(r for r in range(R) if r not in used)

        x = SimpleNamespace(C=3, region=-1, h=H, w=W, d=1, view=None)
        for L in range(9):
            d = LEVEL_DILATION[L]
            for it in self.arch.levels[L]:
                if isinstance(it, _Conv):
                    live.h, live.w = live.h // it.stride, live.w // it.stride
                    y = act(it.co, pick(x))
                    steps.append(('conv', it, x, y, None, d if it.k > 1 else 1, it.relu))
                    x = y
                    continue
                cur = x
                for c in it.convs[:-1]:
                    live.h, live.w = live.h // c.stride, live.w // c.stride
                    y = act(c.co, pick(x, cur))
                    steps.append(('conv', c, cur, y, None, d if c.k > 1 else 1, c.relu))
                    cur = y
                res = x
                if it.downsample is not None:
                    res = act(it.downsample.co, pick(x, cur))
                    steps.append(('conv', it.downsample, x, res, None, 1, False))
                last = it.convs[-1]
                y = act(last.co, pick(x, cur, res))
                steps.append(('conv', last, cur, y, res, d if last.k > 1 else 1, True))
                x = y
        size_in = N * H * W * 4
        return SimpleNamespace(steps=steps, size_in=size_in, size_r=max(shapes), total=size_in + R * max(shapes), last=x, slab=None,
                               h=live.h, w=live.w)

    def _bind(self, N, H, W):
        """the program of an input size with its views of the slab.  The slab only grows; when it is replaced, the programs
        bound to the old one are dropped with it (their views would keep it alive) and made again on their next use."""
        prog = self._program(N, H, W)
        if self._slab is None or self._slab.numel() < prog.total:
            self._slab, self._programs = None, {}
            self._slab = torch.zeros(prog.total, dtype=torch.float32 if self.precision == 'fp32' else torch.bfloat16,
                                     device=self.device)
            prog = self._program(N, H, W)
        if prog.slab is self._slab:
            return prog
        slab = self._slab

        def view(a):
            if a.view is None:
                off = 0 if a.region < 0 else prog.size_in + a.region * prog.size_r
                ld = (4 if self.precision == 'fp32' else 8) if a.region < 0 else a.C
                nb, h, w = N * a.d * a.d, a.h // a.d, a.w // a.d
                a.view = slab[off:off + nb * h * w * ld].view(nb, h, w, ld).permute(0, 3, 1, 2)[:, :a.C]
            return a.view
        for st in prog.steps:
            for a in st[1:]:
                if isinstance(a, SimpleNamespace) and hasattr(a, 'region'):
                    view(a)
        prog.x_in = prog.steps[0][2].view              # the stem's source: 3 channels in an ld of 8, ahead of the regions
        prog.slab = slab
        self._check_routes(prog)
        return prog

    def _conv_launches(self, c, src, dst, residual):
        from .. import ops
        if residual is None:
            return ops.conv_eval_ex(src.view, c.w, c.co, c.k, c.stride, c.pad, dst.view, slot='drn_eval', route_only=True)
        xp, Nb, Ci, h, w, ldx = ops.geom(src.view)
        d = ops.conv_desc(Nb, h, w, Ci, c.co, c.k, c.stride, c.pad, ldx, ops.geom(dst.view)[5])
        need = ops.lib().gcc_conv_eval_workspace(C.byref(d))
        ws = ops.workspace(need, self.device, 'drn_eval') if need else None
        return 2 if ops.lib().gcc_conv_eval_route(C.byref(d), ws.numel() if ws is not None else 0) == 5 else 1

    def _check_routes(self, prog):
        """every conv geometry asked of the library before anything runs: a declined one names its layer; there is no other route"""
        from .. import ops
        for st in prog.steps:
            if st[0] != 'conv':
                continue
            if self.precision == 'fp32':
                _, c, src, dst, _, dil, _ = st
                if ops.conv_eval_f32(src.view, c.w, c.co, c.k, c.stride, dil * (c.k // 2), dst.view, dilation=dil, route_only=True) < 0:
                    raise GccError('DrnSegEngine: the library declines the fp32 geometry of %s (%d -> %d channels, %d x %d, stride '
                                   '%d, dilation %d, on %d x %d x %d): there is no other route'
                                   % ((c.key, c.ci, c.co, c.k, c.k, c.stride, dil) + tuple(src.view.shape[i] for i in (0, 2, 3))))
                continue
            _, c, src, dst, _ = st
            _, Nb, Ci, h, w, ldx = ops.geom(src.view)
            d = ops.conv_desc(Nb, h, w, Ci, c.co, c.k, c.stride, c.pad, ldx, ops.geom(dst.view)[5])
            rc = ops.lib().gcc_conv_eval_ex_route(C.byref(d), 0, 0) if st[4] is None else ops.lib().gcc_conv_eval_route(C.byref(d), 0)
            if rc < 0:
                raise GccError('DrnSegEngine: the library declines the geometry of %s (%d -> %d channels, %d x %d, stride %d, on '
                               '%d x %d x %d): there is no other route' % (c.key, c.ci, c.co, c.k, c.k, c.stride, Nb, h, w))

    @staticmethod
    def _check_size(H, W):
        if H % SIZE_MULTIPLE or W % SIZE_MULTIPLE or H <= 0 or W <= 0:
            raise GccError('DrnSegEngine: input of %d x %d; H and W must be multiples of %d (8x downsampling, then the sub-grids '
                           'of dilation 4)' % (H, W, SIZE_MULTIPLE))

    def _run(self, x, N, H, W, count_only=False):
        from .. import _lib, ops
        self._check_size(H, W)
        if self.device is None:
            raise GccError('DrnSegEngine: .to(device) first')
        prog = self._bind(N, H, W)
        if self.precision == 'fp32':
            return self._run_f32(prog, x, N, H, W, count_only)
        if count_only:
            n = 1 + 2
            for st in prog.steps:
                n += self._conv_launches(*st[1:]) if st[0] == 'conv' else 1
            return n
        ops.nchw_to_nhwc(x, prog.x_in, 0, 8)
        RELU, NONE = _lib.EVAL_ACT_RELU, _lib.EVAL_ACT_NONE
        for st in prog.steps:
            kind = st[0]
            if kind == 'conv':
                _, c, src, dst, res = st
                try:
                    if res is None:
                        ops.conv_eval_ex(src.view, c.w, c.co, c.k, c.stride, c.pad, dst.view, scale=c.scale, shift=c.shift,
                                         act=RELU if c.relu else NONE, slot='drn_eval')
                    else:
                        ops.conv_fprop_eval(src.view, c.w, c.co, c.k, c.stride, c.pad, dst.view, scale=c.scale, shift=c.shift,
                                            act=NONE, residual=res.view, slot='drn_eval')
                except GccError as e:
                    raise GccError('DrnSegEngine: %s: %s' % (c.key, e))
            elif kind == 'relu':
                ops.relu_(st[1].view)
            else:
                _, a, b = st
                ops.phase_regroup(a.view, b.view, a.d, b.d)
        h, w = prog.h, prog.w
        scores = torch.empty((N, self.classes, h, w), dtype=torch.float32, device=self.device)
        logp = torch.empty((N, self.classes, H, W), dtype=torch.float32, device=self.device)
        ops.seg_head(prog.last.view, self.seg_w, self.seg_b, self.up_w, scores, logp)
        return logp, scores

    def _run_f32(self, prog, x, N, H, W, count_only):
        from .. import _lib, ops
        if count_only:
            return 1 + len(prog.steps) + 2           # the input, one launch per convolution, the head's two
        ops.nchw_to_nhwc_f32(x, prog.x_in, 4)
        RELU, NONE = _lib.EVAL_ACT_RELU, _lib.EVAL_ACT_NONE
        for _, c, src, dst, res, dil, relu in prog.steps:
            try:
                ops.conv_eval_f32(src.view, c.w, c.co, c.k, c.stride, dil * (c.k // 2), dst.view, dilation=dil, scale=c.scale,
                                  shift=c.shift, act=RELU if relu else NONE, residual=res.view if res is not None else None)
            except GccError as e:
                raise GccError('DrnSegEngine: %s: %s' % (c.key, e))
        scores = torch.empty((N, self.classes, prog.h, prog.w), dtype=torch.float32, device=self.device)
        logp = torch.empty((N, self.classes, H, W), dtype=torch.float32, device=self.device)
        ops.seg_head_f32(prog.last.view, self.seg_w, self.seg_b, self.up_w, scores, logp)
        return logp, scores

    def __call__(self, x):
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise GccError('DrnSegEngine: expected an NCHW fp32 [N, 3, H, W] tensor, got %s %s'
                           % (getattr(x, 'dtype', type(x).__name__), tuple(getattr(x, 'shape', ()))))
        N, _, H, W = x.shape
        self._check_size(H, W)
        if self.device is None:
            raise GccError('DrnSegEngine: .to(device) first')
        if x.device != self.device:
            raise GccError('DrnSegEngine: the input is on %s, the engine on %s' % (x.device, self.device))
        return self._run(x.contiguous(), N, H, W)

    def infer_launches(self, N, H, W):
        """kernel launches of one call on an [N, 3, H, W] input, from the library's route introspection (launches nothing)"""
        return self._run(None, N, H, W, count_only=True)

    def flops(self, H, W):
        """multiply-adds x 2 of one image from the shapes (convolutions and the seg conv; the streaming kernels not counted)"""
        total, h, w = 0, H, W
        for L in range(9):
            for it in self.arch.levels[L]:
                if isinstance(it, _Conv):
                    h, w = h // it.stride, w // it.stride
                    total += 2 * h * w * it.co * it.ci * it.k * it.k
                    continue
                if it.downsample is not None:
                    c = it.downsample
                    total += 2 * (h // c.stride) * (w // c.stride) * c.co * c.ci
                for c in it.convs:
                    h, w = h // c.stride, w // c.stride
                    total += 2 * h * w * c.co * c.ci * c.k * c.k
        return total + 2 * h * w * self.classes * self.arch.out_channels
