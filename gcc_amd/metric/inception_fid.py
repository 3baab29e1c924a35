"""The FID Inception-v3 network (metric/inception.py:166-315 fid_inception_v3 under InceptionV3([3]): torchvision's
Inception3(num_classes=1008, aux_logits=False) with the FID patches) from the reference's own weight file, a plain state_dict
(pt_inception-2015-12-05-6726825d.pth), on the library's inference convolutions.

    x NCHW fp32 in [0, 1] -> gcc_fid_resize (bilinear to resize x resize, 2 x - 1, NHWC bf16)
        -> stem, Mixed_5b .. Mixed_7c: gcc_conv_eval_ex (conv + folded BatchNorm (eps 1e-3) + ReLU), gcc_pool3x3; every branch's
           last conv writes its channel slice of the block's output, so no concatenation is ever copied
        -> gcc_global_avgpool -> [N, d, 1, 1] fp32

gcc_conv_t has one padding for both directions, so the (1, 7) / (7, 1) / (1, 3) / (3, 1) convolutions run as gcc_border_copy (the
input inside its own zero border) and a padding-0 call with KH != KW.  Mixed_7c's pooling branch is a MAX pool: the FID network's
known quirk (metric/inception.py:301-304), kept.

precision='fp32' is the same network at the reference's own precision: NHWC fp32 activations and fp32 weights through
gcc_conv_eval_f32_ex (f32-input MFMA), whose two paddings are arguments, so a rectangular kernel is ONE launch and the program has
no 'border' step:

    x NCHW fp32 -> gcc_fid_resize_f32 (3 channels in an ld of 4) -> one gcc_conv_eval_f32_ex per BasicConv2d, gcc_pool3x3_f32
        -> gcc_global_avgpool_f32

There is no split-K on that route: an image's features do not depend on the batch it is in, bit for bit.

output_blocks=(...) asks for the reference's other output blocks (metric/inception.py:24-29 BLOCK_INDEX_BY_DIM, :143-163): 0 after
the stem's first max pool, 1 after its second, 2 Mixed_6e's output, 3 the final mean.  The program stops after the last block
asked for; a block below 3 is a 'tap' step where its map is produced: the NCHW fp32 copy InceptionV3(output_blocks).forward
returns, or with pooled=True its spatial mean [N, C, 1, 1] through gcc_map_mean (what fid_score does with such a map), no copy made.

Every width is read from the shapes: the only constraints are that concatenations match and that widths are multiples of 8, so a
thin seeded network runs through the same code as the real one.  Construction parses the state_dict on the host (no device, no
library); .to(device) packs the weights and folds the BatchNorms once -- the weights of an evaluator never change."""
from types import SimpleNamespace

import torch

from .. import ops
from .._lib import EVAL_ACT_RELU, GccError
from ._native import BN_FIELDS, Act, SlabProgramEngine, conv_shape

BN_EPS = 1e-3                                        # BasicConv2d's BatchNorm2d(eps=0.001): a state_dict does not carry it
UNUSED_KEYS = ('fc.weight', 'fc.bias')
MAX_S2, MAX_S1P1, AVG_S1P1 = 0, 1, 2                 # _lib.POOL3_*
WHAT = 'FID Inception state_dict'
PRECISIONS = ('bf16', 'fp32')
BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}      # metric/inception.py:24-29: feature width -> output block
BLOCKS = (0, 1, 2, 3)


def _c(name, k=1, stride=1, pad=0):
    """a BasicConv2d: name, (kh, kw), stride, (ph, pw)"""
    k = (k, k) if isinstance(k, int) else k
    pad = (pad, pad) if isinstance(pad, int) else pad
    return SimpleNamespace(name=name, k=k, stride=stride, pad=pad, key=name + '.conv.weight', bn=name + '.bn', co=0, ci=0)


def _branch(pre=None, chain=(), tails=()):
    """one branch of a block: an optional pool of the block's input, convs into temporaries, then `tails`, each a conv of the
    chain's result into the next channel slice of the block's output (no tails: the pool itself is the slice)"""
    return SimpleNamespace(pre=pre, chain=list(chain), tails=list(tails))


def _block_a(p):
    return [_branch(tails=[_c(p + 'branch1x1')]),
            _branch(chain=[_c(p + 'branch5x5_1')], tails=[_c(p + 'branch5x5_2', 5, pad=2)]),
            _branch(chain=[_c(p + 'branch3x3dbl_1'), _c(p + 'branch3x3dbl_2', 3, pad=1)], tails=[_c(p + 'branch3x3dbl_3', 3, pad=1)]),
            _branch(pre=AVG_S1P1, tails=[_c(p + 'branch_pool')])]


def _block_b(p):
    return [_branch(tails=[_c(p + 'branch3x3', 3, 2)]),
            _branch(chain=[_c(p + 'branch3x3dbl_1'), _c(p + 'branch3x3dbl_2', 3, pad=1)], tails=[_c(p + 'branch3x3dbl_3', 3, 2)]),
            _branch(pre=MAX_S2)]


def _block_c(p):
    r, c = dict(k=(1, 7), pad=(0, 3)), dict(k=(7, 1), pad=(3, 0))
    return [_branch(tails=[_c(p + 'branch1x1')]),
            _branch(chain=[_c(p + 'branch7x7_1'), _c(p + 'branch7x7_2', **r)], tails=[_c(p + 'branch7x7_3', **c)]),
            _branch(chain=[_c(p + 'branch7x7dbl_1'), _c(p + 'branch7x7dbl_2', **c), _c(p + 'branch7x7dbl_3', **r),
                           _c(p + 'branch7x7dbl_4', **c)], tails=[_c(p + 'branch7x7dbl_5', **r)]),
            _branch(pre=AVG_S1P1, tails=[_c(p + 'branch_pool')])]


def _block_d(p):
    return [_branch(chain=[_c(p + 'branch3x3_1')], tails=[_c(p + 'branch3x3_2', 3, 2)]),
            _branch(chain=[_c(p + 'branch7x7x3_1'), _c(p + 'branch7x7x3_2', (1, 7), pad=(0, 3)),
                           _c(p + 'branch7x7x3_3', (7, 1), pad=(3, 0))], tails=[_c(p + 'branch7x7x3_4', 3, 2)]),
            _branch(pre=MAX_S2)]


def _block_e(p, pool):
    r, c = dict(k=(1, 3), pad=(0, 1)), dict(k=(3, 1), pad=(1, 0))
    return [_branch(tails=[_c(p + 'branch1x1')]),
            _branch(chain=[_c(p + 'branch3x3_1')], tails=[_c(p + 'branch3x3_2a', **r), _c(p + 'branch3x3_2b', **c)]),
            _branch(chain=[_c(p + 'branch3x3dbl_1'), _c(p + 'branch3x3dbl_2', 3, pad=1)],
                    tails=[_c(p + 'branch3x3dbl_3a', **r), _c(p + 'branch3x3dbl_3b', **c)]),
            _branch(pre=pool, tails=[_c(p + 'branch_pool')])]


def _network():
    """the module tree: a list of ('conv', _c) / ('pool', mode) / ('block', name, branches) / ('tap', output block): the place
    where the reference's output block 0, 1 or 2 ends (block 3 is the mean behind the last item)"""
    net = [('conv', _c('Conv2d_1a_3x3', 3, 2)), ('conv', _c('Conv2d_2a_3x3', 3)), ('conv', _c('Conv2d_2b_3x3', 3, pad=1)),
           ('pool', MAX_S2), ('tap', 0), ('conv', _c('Conv2d_3b_1x1')), ('conv', _c('Conv2d_4a_3x3', 3)), ('pool', MAX_S2),
           ('tap', 1)]
    for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
        net.append(('block', n, _block_a(n + '.')))
    net.append(('block', 'Mixed_6a', _block_b('Mixed_6a.')))
    for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
        net.append(('block', n, _block_c(n + '.')))
    net.append(('tap', 2))
    net.append(('block', 'Mixed_7a', _block_d('Mixed_7a.')))
    net.append(('block', 'Mixed_7b', _block_e('Mixed_7b.', AVG_S1P1)))
    net.append(('block', 'Mixed_7c', _block_e('Mixed_7c.', MAX_S1P1)))          # the FID network's max pool
    return net


def _net_convs(net):
    out = []
    for item in net:
        if item[0] == 'conv':
            out.append(item[1])
        elif item[0] == 'block':
            for b in item[2]:
                out.extend(b.chain)
                out.extend(b.tails)
    return out


def is_fid_inception_state_dict(sd):
    """an Inception3 state_dict by its keys (the first and the last convolution of the FID network)"""
    return isinstance(sd, dict) and 'Conv2d_1a_3x3.conv.weight' in sd and 'Mixed_7c.branch_pool.conv.weight' in sd


def parse_fid_inception(sd):
    """the architecture of a fid_inception_v3 state_dict (values: tensors, or bare shapes) from its keys and shapes:
    SimpleNamespace(net (the module tree with every conv's ci / co filled in), convs (in launch order), widths {block: output
    channels}, d (the feature width), block_widths {output block 0..3: its channels}).  Raises GccError naming the first key that does not belong or does not fit."""
    if not isinstance(sd, dict):
        raise GccError('%s: expected a dict, got %s' % (WHAT, type(sd).__name__))
    net = _network()
    convs = _net_convs(net)
    known = set(UNUSED_KEYS)
    for c in convs:
        known.add(c.key)
        known.update('%s.%s' % (c.bn, f) for f in BN_FIELDS + ('num_batches_tracked',))
    for key in sd:
        if key not in known:
            raise GccError('%s: unknown key %s' % (WHAT, key))

    def read(c, cin):
        c.co, c.ci = conv_shape(sd, WHAT, c.key, c.bn, c.k)
        if c.ci != cin:
            raise GccError('%s: %s takes %d channels, the layer before it gives %d' % (WHAT, c.key, c.ci, cin))
        return c.co

    cin, widths, block_widths = 3, {}, {}
    for item in net:
        if item[0] == 'conv':
            cin = read(item[1], cin)
        elif item[0] == 'block':
            total = 0
            for b in item[2]:
                cur = cin
                for c in b.chain:
                    cur = read(c, cur)
                total += sum(read(c, cur) for c in b.tails) if b.tails else cur
            widths[item[1]] = cin = total                 # every slice offset is a sum of multiples of 8 (cin of a pool: checked above)
        elif item[0] == 'tap':
            block_widths[item[1]] = cin
    block_widths[3] = cin
    return SimpleNamespace(net=net, convs=convs, widths=widths, d=cin, block_widths=block_widths)


CLASSIFIER_KEYS = UNUSED_KEYS                        # unused by the features; the Inception Score reads them (inception_score.py)


def parse_classifier(sd, arch=None):
    """the network's classifier head (Inception3.fc: the logits the Inception Score is computed from): (sd['fc.weight'],
    sd['fc.bias']) when the state_dict (values: tensors, or bare shapes) carries both, None when it carries neither.  Their shapes
    must be [C, d] and [C] with C >= 2 and d the feature width of output block 3 (``arch``: parse_fid_inception(sd), made here if
    not given); GccError names the key that is missing or does not fit."""
    from ._native import _shape
    wk, bk = CLASSIFIER_KEYS
    if not isinstance(sd, dict):
        raise GccError('%s: expected a dict, got %s' % (WHAT, type(sd).__name__))
    if wk not in sd and bk not in sd:
        return None
    for key in (wk, bk):
        if key not in sd:
            raise GccError('%s: %s is missing (the classifier has a weight and a bias)' % (WHAT, key))
    d = (arch or parse_fid_inception(sd)).block_widths[3]
    ws, bs = _shape(sd[wk]), _shape(sd[bk])
    if len(ws) != 2 or ws[1] != d or ws[0] < 2:
        raise GccError('%s: %s has shape %s, expected (C >= 2, %d): the classifier reads the %d pool features' % (WHAT, wk, ws, d, d))
    if bs != (ws[0],):
        raise GccError('%s: %s has shape %s, expected (%d,)' % (WHAT, bk, bs, ws[0]))
    return sd[wk], sd[bk]


def check_output_blocks(output_blocks):
    """the blocks asked for, deduplicated and ascending (metric/inception.py:84); GccError names the choices otherwise"""
    try:
        blocks = sorted(set(output_blocks))
    except TypeError:
        blocks = []
    if not blocks or any(isinstance(b, bool) or not isinstance(b, int) or b not in BLOCKS for b in blocks):
        raise GccError('InceptionFidEngine: output_blocks %r; expected one or more of %s (the blocks of %s features)'
                       % (output_blocks, ', '.join(str(b) for b in BLOCKS),
                          ' / '.join(str(d) for d in sorted(BLOCK_INDEX_BY_DIM))))
    return tuple(blocks)


def _out(size, k, stride, pad):
    return (size + 2 * pad - k) // stride + 1


class InceptionFidEngine(SlabProgramEngine):
    """inception(x)[0] for fid_eval.ImageStatistics: x NCHW fp32 [N, 3, H, W] in [0, 1] on the device, any H, W -> [features],
    features fp32 [N, d, 1, 1] (d = 2048 for the real network), InceptionV3([3]).forward's list.  With output_blocks: one fp32
    tensor per block asked for, ascending, InceptionV3(output_blocks).forward's list -- a block below 3 as its contiguous NCHW map
    [N, C, h, w], or with pooled=True as that map's spatial mean [N, C, 1, 1] in f64 (gcc_map_mean: the bf16 route's maps hold
    bf16 values, the mean adds one fp32 rounding); .d is the width of the last block asked for.  Activations are NHWC bf16 with
    one rounding per conv + BatchNorm + ReLU and per average pool; the input resize and the final mean are fp32 arithmetic.
    precision='fp32': activations, weights and every sum are fp32 (the reference's own arithmetic), one launch per convolution.
    .classifier: (fc.weight [C, d], fc.bias [C]) as fp32 tensors, on the device after .to(device) -- the head the Inception Score
    reads (inception_score.py; the engine itself never applies it) --, None when the state_dict has no fc.* or the engine stops
    below block 3.  The engine's scaffold -- .to(), the slab and its programs, the route check -- is metric/_native.py's."""
    BN_EPS = BN_EPS

    def __init__(self, state_dict, resize=299, precision='bf16', output_blocks=(3,), pooled=False):
        if precision not in PRECISIONS:
            raise GccError('InceptionFidEngine: precision %r; expected one of %s' % (precision, ', '.join(PRECISIONS)))
        self.precision = precision
        if precision == 'fp32':
            self._slab_dtype = torch.float32
        self.output_blocks, self.pooled = check_output_blocks(output_blocks), bool(pooled)
        self.arch = parse_fid_inception(state_dict)
        self.block_widths = dict(self.arch.block_widths)
        self.d = self.block_widths[self.output_blocks[-1]]
        self.resize = int(resize)
        if self.resize <= 0:
            raise GccError('InceptionFidEngine: resize must be positive, got %r' % (resize,))
        # the classifier (fc.*: the Inception Score's logits) of an engine that runs to the pool features, when the file has one
        head = parse_classifier(state_dict, self.arch) if self.output_blocks[-1] == 3 else None
        super().__init__(state_dict, self.arch.convs)
        self._head = None if head is None else tuple(t.detach().to('cpu', torch.float32).contiguous() for t in head)
        self.classifier = self._head                   # (weight, bias): fp32, on the host until .to(device)
        self._plan(1)                                  # a resize too small for the network is refused here, on the host

    def _pack(self, c, master):
        return ops.pack_weights_f32(master) if self.precision == 'fp32' else super()._pack(c, master)

    def _to_extra(self, device):
        if self._head is not None:
            self.classifier = tuple(t.to(device) for t in self._head)      # fp32, on the device

    # ---- the launch program ---------------------------------------------------------------------------------------------
    def _plan(self, N):
        """the launches of a batch of N as tuples over symbolic activations of the slab: behind the 8-channel resized input (4 in
        fp32), four regions -- a block's input and output, which swap from layer to layer, and two temporaries the branches
        alternate between.  The input's own H and W appear in no launch but gcc_fid_resize, so a program depends on N alone.
        bf16: ('conv', conv, source, destination), ('pool', mode, source, destination), ('border', source, destination, ph, pw)
        in front of a rectangular kernel.  fp32: no 'border' -- a 'conv' step's (ph, pw) are its conv's own .pad.
        ('tap', block, source): an output block below 3 that was asked for, read where it stands before its region is written
        again; the program ends behind the last block asked for, so it is a prefix of the whole network's."""
        steps, sizes, where = [], [], ['the input']
        R = self.resize
        f32 = self.precision == 'fp32'
        grid = 4 if f32 else 8                         # the channels of a 16-byte chunk: every slice starts and ends on one
        reg = SimpleNamespace(x=0, y=1, t1=2, t2=3)

        def act(Cc, h, w, region, ld=None, off=0):
            if h <= 0 or w <= 0:
                raise GccError('InceptionFidEngine: resize = %d leaves no pixel at %s' % (R, where[0]))
            a = Act(Cc, h, w, region, ld=ld, off=off)
            if a.off % grid or a.ld % grid:
                raise GccError('InceptionFidEngine: a channel slice at %d of %d is off the %d-channel grid' % (a.off, a.ld, grid))
            if off == 0:
                sizes.append(N * h * w * a.ld)
            return a

        def free(a):
            """the temporary `a` is not in"""
            return reg.t2 if a.region == reg.t1 else reg.t1

        def apply(c, cur, dst=None):
            """conv c of `cur` into the slice `dst`, or into a fresh activation of the temporary that is free.  A rectangular
            kernel's padding is a zero border first (in the temporary `cur` is not in: `cur` may have other readers)."""
            where[0] = c.key
            ph, pw = c.pad
            if c.k[0] != c.k[1] and not f32:
                b = act(cur.C, cur.h + 2 * ph, cur.w + 2 * pw, free(cur))
                steps.append(('border', cur, b, ph, pw))
                cur, ph, pw = b, 0, 0
            ho, wo = _out(cur.h, c.k[0], c.stride, ph), _out(cur.w, c.k[1], c.stride, pw)
            if dst is None:
                dst = act(c.co, ho, wo, free(cur))
            elif (dst.h, dst.w) != (ho, wo):
                raise GccError('InceptionFidEngine: %s gives %d x %d, its block %d x %d' % (c.key, ho, wo, dst.h, dst.w))
            steps.append(('conv', c, cur, dst))
            return dst

        def pool(mode, cur, dst):
            steps.append(('pool', mode, cur, dst))
            return dst

        x = Act(3, R, R, -1, ld=grid)
        for item in self.arch.net:
            if item[0] == 'tap':
                if item[1] in self.output_blocks:
                    steps.append(('tap', item[1], x))
                if item[1] == self.output_blocks[-1]:
                    break
                continue
            if item[0] == 'conv':
                c = item[1]
                where[0] = c.key
                y = apply(c, x, act(c.co, _out(x.h, c.k[0], c.stride, c.pad[0]), _out(x.w, c.k[1], c.stride, c.pad[1]), reg.y))
            elif item[0] == 'pool':
                where[0] = 'the stem\'s max pool'
                y = pool(item[1], x, act(x.C, _out(x.h, 3, 2, 0), _out(x.w, 3, 2, 0), reg.y))
            else:
                name, branches = item[1], item[2]
                where[0] = name
                s2 = any(b.pre == MAX_S2 for b in branches)
                ho, wo = (_out(x.h, 3, 2, 0), _out(x.w, 3, 2, 0)) if s2 else (x.h, x.w)
                width = self.arch.widths[name]
                y = act(width, ho, wo, reg.y)
                off = 0
                for b in branches:
                    cur = x
                    if b.pre is not None and not b.tails:                      # the pool is the slice
                        pool(b.pre, x, act(x.C, ho, wo, reg.y, width, off))
                        off += x.C
                        continue
                    if b.pre is not None:
                        cur = pool(b.pre, x, act(x.C, x.h, x.w, reg.t1))
                    for c in b.chain:
                        cur = apply(c, cur)
                    for c in b.tails:
                        if off % grid:
                            raise GccError('InceptionFidEngine: %s would be written at channel %d of %s' % (c.key, off, name))
                        apply(c, cur, act(c.co, ho, wo, reg.y, width, off))
                        off += c.co
                if off != width:
                    raise GccError('InceptionFidEngine: %s concatenates %d channels, expected %d' % (name, off, width))
            x, reg.x, reg.y = y, reg.y, reg.x
        return SimpleNamespace(steps=steps, size_in=N * R * R * grid, size_r=max(sizes), last=x, slab=None, x_in=None,
                               total=N * R * R * grid + 4 * max(sizes))

    def _conv(self, st, route_only=False):
        """launch the 'conv' step st, or with route_only the library's answer for it: its launches, -1 if it declines"""
        _, c, src, dst = st
        if self.precision == 'fp32':
            rc = ops.conv_eval_f32_ex(src.view, c.w, c.co, c.k, c.stride, c.pad, dst.view, scale=c.scale, shift=c.shift,
                                      act=EVAL_ACT_RELU, route_only=route_only)
            return (1 if rc >= 0 else -1) if route_only else rc          # the route's answer is a tile: always one launch
        if c.k[0] != c.k[1]:
            return ops.conv_eval_rect(src.view, c.w, c.co, c.k, c.stride, dst.view, scale=c.scale, shift=c.shift, act=EVAL_ACT_RELU,
                                      slot='inception_eval', route_only=route_only)
        return ops.conv_eval_ex(src.view, c.w, c.co, c.k[0], c.stride, c.pad[0], dst.view, scale=c.scale, shift=c.shift,
                                act=EVAL_ACT_RELU, slot='inception_eval', route_only=route_only)

    def _declined(self, st):
        c, src = st[1:3]
        if self.precision == 'fp32':
            return ('InceptionFidEngine: the library declines the fp32 geometry of %s (%d -> %d channels, %d x %d, stride %d, '
                    'padding (%d, %d), on %d x %d x %d): there is no other route'
                    % ((c.key, c.ci, c.co, c.k[0], c.k[1], c.stride) + tuple(c.pad) + tuple(src.view.shape[i] for i in (0, 2, 3))))
        return ('InceptionFidEngine: the library declines the geometry of %s (%d -> %d channels, %d x %d, stride %d, on %d x %d x '
                '%d): there is no other route' % ((c.key, c.ci, c.co, c.k[0], c.k[1], c.stride)
                                                  + tuple(src.view.shape[i] for i in (0, 2, 3))))

    def _run(self, x, N, count_only=False):
        self._check_device()
        prog = self._bind(N)
        f32 = self.precision == 'fp32'
        if count_only:
            def launches(st):
                if st[0] == 'conv':
                    return self._conv(st, route_only=True)
                if st[0] == 'tap' and self.pooled:
                    return ops.map_mean_launches(st[2].h, st[2].w, st[2].C)
                return 1
            return 1 + sum(launches(st) for st in prog.steps) + (3 in self.output_blocks)
        outs = []
        (ops.fid_resize_f32 if f32 else ops.fid_resize)(x, prog.x_in)
        pool3x3 = ops.pool3x3_f32 if f32 else ops.pool3x3
        for st in prog.steps:
            kind = st[0]
            if kind == 'conv':
                try:
                    self._conv(st)
                except GccError as e:
                    raise self._conv_error(st, e)
            elif kind == 'pool':
                pool3x3(st[1], st[2].view, st[3].view)
            elif kind == 'tap':
                outs.append(self._tap(st[2].view, N))
            else:
                ops.border_copy(st[1].view, st[2].view, st[3], st[4])
        if 3 in self.output_blocks:
            out = torch.empty((N, self.block_widths[3], 1, 1), dtype=torch.float32, device=self.device)
            (ops.global_avgpool_f32 if f32 else ops.global_avgpool)(prog.last.view, out)
            outs.append(out)
        return outs

    def _tap(self, view, N):
        """an output block below 3 from its slab view: the NCHW fp32 map, or pooled its mean over the pixels"""
        f32 = self.precision == 'fp32'
        if not self.pooled:
            return (ops.nhwc_to_nchw_f32 if f32 else ops.nhwc_to_nchw)(view)
        out = torch.empty((N, view.shape[1], 1, 1), dtype=torch.float32, device=self.device)
        (ops.map_mean_f32 if f32 else ops.map_mean)(view, out)
        return out

    def __call__(self, x):
        self._check_input(x, refuse_empty=True)
        self._check_device(x)
        return self._run(x.contiguous(), x.shape[0])

    def infer_launches(self, N, H=None, W=None):
        """kernel launches of one call on an [N, 3, H, W] input, from the library's route introspection (launches nothing); the
        input's size changes the resize kernel's work, not the count"""
        return self._run(None, N, count_only=True)

    def flops(self):
        """multiply-adds x 2 of one image from the shapes (convolutions only; the streaming kernels not counted)"""
        total = 0
        for st in self._program(1).steps:
            if st[0] == 'conv':
                _, c, _, dst = st
                total += 2 * dst.h * dst.w * c.co * c.ci * c.k[0] * c.k[1]
        return total
