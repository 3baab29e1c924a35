"""Host side of the native DRN-D segmenter (gcc_amd.metric.drn_seg): the architecture read from a DRNSeg state_dict's keys and
shapes, every refusal, the phase-layout rule against torch's dilated convolution, the engine's launch program executed
with torch on the host against the reference's results (tests/golden/drn_seg.npz, written by tests/golden/make_drn_fixtures.py
from the reference's own DRNSeg), the launch count and the slab's life against a recording stand-in for gcc_amd.ops,
builtin_segmenter's selection rule and the ABI surface.  No GPU."""
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _drn_emul as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def z():
    return np.load(E.GOLDEN)


# ---- 1. the architecture from the keys ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(E.NETS))
def test_architecture_of_each_fixture(z, name):
    from gcc_amd.metric import drn_seg as D
    kind, layers, channels, _, _, _ = E.NETS[name]
    sd, _ = E.fixture_net(z, name)
    assert D.is_drn_seg_state_dict(sd)
    a = D.parse_drn_seg(sd)
    assert a.kind == kind and a.depths == layers and a.widths == list(channels) and a.classes == 19
    assert a.strides == [1, 2, 2, 2, 1, 1, 1, 1] and a.dilations == [1, 1, 1, 1, 2, 4, 2, 1]
    assert a.out_channels == channels[-1]
    eng = D.DrnSegEngine(sd)                               # host only: no device, no library
    assert eng.device is None and len(eng.convs) == sum(1 for k in sd if k.endswith('weight') and sd[k].dim() == 4) - 2


@pytest.mark.parametrize('name', list(E.D_LAYERS))
def test_architecture_of_the_full_width_nets_from_shapes_alone(name):
    from gcc_amd.metric import drn_seg as D
    kind, layers = E.D_LAYERS[name]
    shapes = E.drn_shapes(kind, layers, E.D105[2])
    a = D.parse_drn_seg(dict(shapes))                      # bare shapes: nothing of 54 M parameters is allocated
    assert a.kind == kind and a.depths == layers and a.widths == list(E.D105[2]) and a.classes == 19
    assert a.out_channels == 512
    blocks = [b for L in (3, 4, 5, 6) for b in a.levels[L]]
    assert sum(b.downsample is not None for b in blocks) == 4          # every residual level changes stride or width
    if name == 'drn_d_105':
        nconv = 1 + sum(layers[i] for i in (0, 1, 6, 7)) + 3 * sum(layers[2:6]) + 4
        assert len(D._all_convs(a)) == nconv == 108


def _bneck(z):
    return E.fixture_net(z, 'bneck')[0]


def test_refusals_name_the_first_offending_key(z):
    from gcc_amd._lib import GccError
    from gcc_amd.metric.drn_seg import DrnSegEngine, is_drn_seg_state_dict, parse_drn_seg
    sd = _bneck(z)

    def refused(change, word):
        bad = OrderedDict(sd)
        change(bad)
        with pytest.raises(GccError, match=re.escape(word)):
            DrnSegEngine(bad)

    # arch C: base.0 is the bare 7 x 7 conv, base.1 its BatchNorm
    def arch_c(d):
        w = d.pop('base.0.0.weight')
        items = [('base.0.weight', w)] + list(d.items())
        d.clear()
        d.update(items)
    refused(arch_c, 'base.0.weight')
    assert not is_drn_seg_state_dict({'base.0.weight': 0, 'seg.weight': 0, 'seg.bias': 0, 'up.weight': 0})
    refused(lambda d: d.update({'base.3.0.conv4.weight': torch.zeros(8, 8, 1, 1)}), 'unknown key base.3.0.conv4.weight')
    refused(lambda d: d.update({'fc.weight': torch.zeros(1)}), 'unknown key fc.weight')
    refused(lambda d: d.update({'base.1.0.bias': torch.zeros(8)}), 'unknown key base.1.0.bias')
    refused(lambda d: d.update({'base.1.2.weight': torch.zeros(8)}), 'unknown key base.1.2.weight')
    refused(lambda d: d.pop('base.5.1.bn2.running_var'), 'base.5.1.bn2.running_var is missing')
    refused(lambda d: d.pop('base.0.1.running_mean'), 'base.0.1.running_mean is missing')
    refused(lambda d: d.pop('base.4.0.downsample.0.weight'), 'base.4.0.downsample.0.weight is missing')
    refused(lambda d: d.pop('seg.bias'), 'seg.bias is missing')

    def odd_width(d):
        d['base.1.0.weight'] = torch.zeros(12, 8, 3, 3)
        for f in E.BN[:4]:
            d['base.1.1.' + f] = torch.ones(12)
    refused(odd_width, 'base.1.0.weight has 12 output channels')
    refused(lambda d: d.update({'base.2.0.weight': torch.zeros(8, 16, 3, 3)}), 'base.2.0.weight takes 16 channels')
    refused(lambda d: d.update({'up.weight': torch.zeros(19, 1, 4, 4)}), 'up.weight has shape')
    refused(lambda d: d.update({'base.7.0.weight': torch.zeros(16, 64, 5, 5)}), 'base.7.0.weight has shape')
    with pytest.raises(GccError, match='expected a dict'):
        parse_drn_seg([1, 2])
    # H, W that are no multiples of 32, and a host engine, are refused before anything is touched
    eng = DrnSegEngine(sd)
    with pytest.raises(GccError, match='to\\(device\\)'):
        eng(torch.zeros(1, 3, 64, 64))
    with pytest.raises(GccError, match='NCHW fp32'):
        eng(torch.zeros(1, 4, 64, 64))
    for hw in ((64, 72), (48, 64), (8, 8)):
        with pytest.raises(GccError, match='multiples of 32'):
            eng(torch.zeros(1, 3, *hw))
    with pytest.raises(GccError, match='GPU only'):
        eng.to('cpu')


# ---- 2. dilation is a change of layout ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,N,H,W', [(2, 2, 8, 12), (4, 2, 8, 12), (4, 1, 4, 4), (2, 1, 2, 6)])
def test_phase_layout_equals_dilated_conv_exactly(d, N, H, W):
    from gcc_amd.metric.drn_seg import from_phase, phase_index, to_phase
    g = torch.Generator().manual_seed(d * 100 + H)
    # small integers: every product and sum is exact in fp32, so the two routes must agree to the bit whatever their order
    x = torch.randint(-8, 9, (N, 5, H, W), generator=g).float()
    w = torch.randint(-4, 5, (7, 5, 3, 3), generator=g).float()
    want = F.conv2d(x, w, None, 1, d, d)
    xp = to_phase(x, d)
    assert tuple(xp.shape) == (N * d * d, 5, H // d, W // d)
    got = from_phase(F.conv2d(xp, w, None, 1, 1, 1), d)
    assert torch.equal(got, want)
    assert torch.equal(from_phase(xp, d), x)
    # the index map the kernel implements, pixel by pixel
    n, h, ww = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), indexing='ij')
    b, r, c = phase_index(n, h, ww, d)
    assert torch.equal(xp[b, :, r, c], x.permute(0, 2, 3, 1))
    # a regrouping between two dilated layouts is the composition through layout 1
    for d2 in (1, 2, 4):
        if H % d2 == 0 and W % d2 == 0:
            assert torch.equal(from_phase(to_phase(from_phase(xp, d), d2), d2), x)


# ---- 3. the launch program, executed with torch on the host -------------------------------------------------------------------
def _execute(eng, sd, x, emulate):
    """run DrnSegEngine's program step by step in torch-CPU over a model of its four slab regions: a read of an activation
    whose region another one has since taken fails"""
    from gcc_amd.metric.drn_seg import from_phase, to_phase
    N, _, H, W = x.shape
    prog = eng._program(N, H, W)
    r = (lambda t: t.bfloat16().float()) if emulate else (lambda t: t)
    val, owner = {}, {}

    def write(a, t):
        assert tuple(t.shape) == (N * a.d * a.d, a.C, a.h // a.d, a.w // a.d), (tuple(t.shape), a.C, a.h, a.w, a.d)
        assert t.numel() <= prog.size_r
        val[id(a)], owner[a.region] = t, id(a)

    def read(a):
        assert owner[a.region] == id(a), 'region %d overwritten while still needed' % a.region
        return val[id(a)]
    first = prog.steps[0][2]
    assert first.region == -1 and first.C == 3
    write(first, r(x))
    counts = {'conv': 0, 'relu': 0, 'regroup': 0}
    for st in prog.steps:
        counts[st[0]] += 1
        if st[0] == 'conv':
            _, c, src, dst, res = st
            assert dst.region not in (src.region, res.region if res is not None else None)
            y = F.conv2d(read(src), r(sd[c.key]), None, c.stride, c.pad, 1)
            scale = sd[c.bn + '.weight'] / torch.sqrt(sd[c.bn + '.running_var'] + 1e-5)
            y = y * scale[None, :, None, None] + (sd[c.bn + '.bias'] - sd[c.bn + '.running_mean'] * scale)[None, :, None, None]
            if res is not None:
                assert not c.relu
                y = y + read(res)
            write(dst, r(torch.relu(y) if c.relu else y))
        elif st[0] == 'relu':
            write(st[1], torch.relu(read(st[1])))
        else:
            _, a, b = st
            assert a.region != b.region
            write(b, to_phase(from_phase(read(a), a.d), b.d))
    last = read(prog.last)
    assert prog.last.d == 1 and (prog.h, prog.w) == (H // 8, W // 8)
    scores = F.conv2d(last, sd['seg.weight'], sd['seg.bias'])
    return E.head(scores, sd['up.weight']), scores, counts


@pytest.mark.parametrize('name', list(E.NETS))
def test_program_on_the_host_reproduces_the_reference(z, name):
    from gcc_amd.metric.drn_seg import DrnSegEngine
    sd, x = E.fixture_net(z, name)
    eng = DrnSegEngine(sd)
    ref = torch.from_numpy(z[name + '.scores'])
    span = float(ref.max() - ref.min())
    # fp32: the phase-layout program is the network up to the convolutions' summation order
    logp, scores, counts = _execute(eng, sd, x, emulate=False)
    err = float((scores - ref).abs().max())
    print('%s: program in fp32 against the reference: max |diff| %.3g of a range of %.3g' % (name, err, span))
    assert err <= 1e-4 * span
    blocks = sum(E.NETS[name][1][2:6])
    assert counts['regroup'] == 4 and counts['relu'] == blocks
    from tests.golden.recipe import sample_idx
    assert float((logp.reshape(-1)[sample_idx(logp.numel())] - torch.from_numpy(z[name + '.logp_sample'])).abs().max()) <= 1e-4 * span
    am = logp.argmax(dim=1).numpy()
    sure = z[name + '.margin'] > 1e-3 * span
    assert np.array_equal(am[sure], z[name + '.argmax'][sure])
    # with the device path's number formats it is the stored emulation error, give or take the order of the fp32 sums
    _, se, _ = _execute(eng, sd, x, emulate=True)
    e2 = float((se - ref).abs().max())
    print('%s: program in bf16 against the reference: %.4f, stored emul_err %.4f' % (name, e2, float(z[name + '.emul_err'])))
    assert e2 <= 2 * float(z[name + '.emul_err'])
    assert eng.flops(*x.shape[2:]) > 0


def test_emulation_error_is_what_the_fixture_stores(z):
    for name in E.NETS:
        sd, x = E.fixture_net(z, name)
        _, se = E.forward(sd, x, emulate=True)
        e = float((se - torch.from_numpy(z[name + '.scores'])).abs().max())
        assert abs(e - float(z[name + '.emul_err'])) <= 0.05 * float(z[name + '.emul_err']), (name, e)


# ---- 3b. the launch count and the slab, against a recording stand-in for gcc_amd.ops -----------------------------------------------
class _Recorder:
    """stands in for gcc_amd.ops under an engine: records what would be launched.  A bf16 conv with 16 or more input channels takes
    the split-K route (two launches), so the count has to come from the route and not from the number of steps; the fp32 conv's
    route answer is a tile index, never a count: it is one launch whatever the answer."""

    def __init__(self):
        self.calls = []

    def route(self, x):
        return 2 if x.shape[1] >= 16 else 1

    def _conv(self, name, x, k, stride, pad, out, dilation, act, residual):
        return (name, k, stride, pad, dilation, act, residual is not None, tuple(x.shape), tuple(out.shape))

    def conv_eval_ex(self, x, w, Co, k, stride, pad, out, act=None, slot=None, route_only=False, **kw):
        assert slot == 'drn_eval'
        if route_only:
            return self.route(x)
        self.calls += [self._conv('conv_eval_ex', x, k, stride, pad, out, 1, act, None)] * self.route(x)

    def conv_fprop_eval(self, x, w, Co, k, stride, pad, out, act=None, residual=None, slot=None, route_only=False, **kw):
        assert slot == 'drn_eval'
        if route_only:
            return self.route(x)
        self.calls += [self._conv('conv_fprop_eval', x, k, stride, pad, out, 1, act, residual)] * self.route(x)

    def conv_eval_f32(self, x, w, Co, k, stride, pad, out, dilation=1, act=None, residual=None, route_only=False, **kw):
        if route_only:
            return self.route(x)
        self.calls.append(self._conv('conv_eval_f32', x, k, stride, pad, out, dilation, act, residual))

    def nchw_to_nhwc(self, src, dst, off=0, cfill=None):
        self.calls.append(('input', tuple(src.shape), tuple(dst.shape), cfill))

    def nchw_to_nhwc_f32(self, src, dst, cfill=None):
        self.calls.append(('input', tuple(src.shape), tuple(dst.shape), cfill))

    def phase_regroup(self, src, dst, d_src, d_dst):
        self.calls.append(('regroup', d_src, d_dst, tuple(src.shape), tuple(dst.shape)))

    def relu_(self, x):
        self.calls.append(('relu', tuple(x.shape)))

    def seg_head(self, x, seg_w, seg_b, up_w, scores, logp=None):
        self.calls += [('head', tuple(x.shape), tuple(scores.shape), tuple(logp.shape))] * 2       # the seg conv, then up + LogSoftmax

    seg_head_f32 = seg_head


def _inside(view, slab):
    """the storage a view can reach lies inside the slab"""
    first = view.data_ptr()
    last = first + sum((n - 1) * s for n, s in zip(view.shape, view.stride())) * view.element_size()
    return slab.data_ptr() <= first and last < slab.data_ptr() + slab.numel() * slab.element_size()


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_infer_launches_and_the_slab_against_a_recording_stand_in(monkeypatch, z, precision):
    from gcc_amd import _lib, ops
    from gcc_amd.metric.drn_seg import DrnSegEngine
    rec = _Recorder()
    for name in ('conv_eval_ex', 'conv_fprop_eval', 'conv_eval_f32', 'nchw_to_nhwc', 'nchw_to_nhwc_f32', 'phase_regroup', 'relu_',
                 'seg_head', 'seg_head_f32'):
        monkeypatch.setattr(ops, name, getattr(rec, name))
    sd, x = E.fixture_net(z, 'bneck')
    N, _, H, W = x.shape
    eng = DrnSegEngine(sd, precision=precision)
    monkeypatch.setattr(eng, '_check_routes', lambda prog: None)          # the library's say: asked on the GPU
    eng.device = torch.device('cpu')                                        # as .to() leaves it, without packing anything
    for c in eng.convs:
        c.w = c.scale = c.shift = None
    eng.seg_w = eng.seg_b = eng.up_w = None
    # the shared _bind on a host slab: N = 1, then the full batch, then N = 1 again
    eng._run(torch.zeros(1, 3, H, W), 1, H, W)
    small, old = eng._slab, eng._program(1, H, W)
    assert old.slab is small
    predicted = eng.infer_launches(N, H, W)
    assert eng._slab is not small and eng._slab.numel() > small.numel()     # replaced by a larger one ...
    assert all(p.slab is eng._slab and p is not old for p in eng._programs.values())       # ... and no program keeps the old
    ptr = eng._slab.data_ptr()
    eng._run(torch.zeros(1, 3, H, W), 1, H, W)
    assert eng._slab.data_ptr() == ptr and sorted(eng._programs) == [(1, H, W), (N, H, W)]
    for prog in eng._programs.values():
        assert prog.slab is eng._slab and _inside(prog.x_in, eng._slab)
        views = [a.view for st in prog.steps for a in st[1:] if hasattr(a, 'region')] + [prog.last.view]
        assert len(views) > len(eng.convs) and all(v is not None and _inside(v, eng._slab) for v in views)
    # the count
    rec.calls.clear()
    assert eng.infer_launches(N, H, W) == predicted and rec.calls == []     # counting launches nothing
    logp, scores = eng._run(x, N, H, W)
    assert tuple(logp.shape) == (N, 19, H, W) and tuple(scores.shape) == (N, 19, H // 8, W // 8)
    assert len(rec.calls) == predicted
    kinds = [c[0] for c in rec.calls]
    assert kinds[0] == 'input' and kinds[-1] == 'head' and kinds.count('input') == 1 and kinds.count('head') == 2
    blocks = [b for L in (3, 4, 5, 6) for b in eng.arch.levels[L]]
    lasts = {b.convs[-1].key for b in blocks}
    convs = [c for c in rec.calls if c[0].startswith('conv')]
    with_res = [c for c in convs if c[6]]
    if precision == 'bf16':
        assert kinds.count('regroup') == 4 and [c[1:3] for c in rec.calls if c[0] == 'regroup'] == [(1, 2), (2, 4), (4, 2), (2, 1)]
        assert kinds.count('relu') == len(blocks)
        assert rec.calls[1][-2][1] == 3 and rec.calls[0][3] == 8            # 3 channels in an ld of 8
        # a residual goes to exactly the blocks' last convs, through conv_fprop_eval, without an activation
        assert {c[0] for c in with_res} == {'conv_fprop_eval'} and all(c[5] == _lib.EVAL_ACT_NONE for c in with_res)
        assert all(c[6] for c in convs if c[0] == 'conv_fprop_eval')
        steps = [st for st in eng._program(N, H, W).steps if st[0] == 'conv']
        assert {st[1].key for st in steps if st[4] is not None} == lasts
        assert len(with_res) == sum(rec.route(st[2].view) for st in steps if st[4] is not None)
        assert 'conv_eval_f32' not in kinds and len(convs) > len(eng.convs)  # some convs took two launches
    else:
        assert len(convs) == len(eng.convs) and {c[0] for c in convs} == {'conv_eval_f32'}
        assert 'regroup' not in kinds and 'relu' not in kinds and rec.calls[0][3] == 4
        steps = eng._program(N, H, W).steps
        assert sorted(st[1].key for st in steps) == sorted(c.key for c in eng.convs)
        assert {st[1].key for st in steps if st[4] is not None} == lasts and len(with_res) == len(blocks)
        assert all(c[5] == _lib.EVAL_ACT_RELU for c in with_res)            # the ReLU behind the sum rides on the conv
        assert {c[4] for c in convs} == {1, 2, 4}
        assert all(c[3] == c[4] for c in convs if c[1] == 3) and all(c[3] == 0 and c[4] == 1 for c in convs if c[1] == 1)
        assert all(c[3] == 3 and c[4] == 1 for c in convs if c[1] == 7)
        assert predicted == 1 + len(eng.convs) + 2


# ---- 4. selection ---------------------------------------------------------------------------------------------------------------
class _StandIn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 19, 1)

    def forward(self, x):
        return torch.log_softmax(self.conv(x), dim=1), x


def test_builtin_segmenter_selection(tmp_path, z):
    from gcc_amd.metric.cityscapes import builtin_segmenter
    from gcc_amd.metric.drn_seg import DrnSegEngine
    from gcc_amd.options import options
    root = tmp_path / 'cityscapes'
    root.mkdir()
    drn = tmp_path / 'drn.pth'
    opt = options.parse(['--dataroot', str(root), '--model', 'pix2pix', '--drn_path', str(drn)])
    seg, why = builtin_segmenter(opt)
    assert seg is None and 'table.txt' in why
    (root / 'table.txt').write_text('0 a_trainIds.png a.png\n')
    seg, why = builtin_segmenter(opt)
    assert seg is None and 'does not exist' in why
    # the reference's own file: a plain state_dict of a DRNSeg
    sd = _bneck(z)
    torch.save(sd, str(drn))
    seg, why = builtin_segmenter(opt)
    assert isinstance(seg, DrnSegEngine) and why is None and seg.device is None and seg.arch.kind == 'bottleneck'
    # a dict without DRNSeg's keys is no candidate: today's refusal, with the loader's error quoted
    torch.save(_StandIn().state_dict(), str(drn))
    seg, why = builtin_segmenter(opt)
    assert seg is None and 'TorchScript' in why and ('Error' in why or 'Exception' in why) and 'export DRNSeg' in why
    torch.save([1, 2, 3], str(drn))
    seg, why = builtin_segmenter(opt)
    assert seg is None and 'TorchScript' in why
    drn.write_bytes(b'not a checkpoint at all')
    seg, why = builtin_segmenter(opt)
    assert seg is None and 'TorchScript' in why
    # a DRNSeg state_dict the package does not run says which key
    bad = OrderedDict(sd)
    bad.pop('base.6.0.bn3.running_var')
    torch.save(bad, str(drn))
    seg, why = builtin_segmenter(opt)
    assert seg is None and 'base.6.0.bn3.running_var' in why
    # a TorchScript archive is still taken first
    torch.jit.script(_StandIn()).save(str(drn))
    seg, why = builtin_segmenter(opt)
    assert isinstance(seg, torch.jit.ScriptModule) and why is None


def test_builtin_evaluator_takes_the_state_dict(tmp_path, z):
    import logging
    from gcc_amd import train
    from gcc_amd.options import options
    root = tmp_path / 'cityscapes'
    root.mkdir()
    (root / 'table.txt').write_text('0 a_trainIds.png a.png\n')
    drn = tmp_path / 'drn-d-105_ms_cityscapes.pth'
    torch.save(_bneck(z), str(drn))
    lines = []
    log = logging.getLogger('drn_seg_test')
    log.setLevel(logging.INFO)
    h = logging.Handler()
    h.emit = lambda record: lines.append(record.getMessage())
    log.addHandler(h)
    try:
        ev = train.builtin_evaluator(options.parse(['--dataroot', str(root), '--model', 'pix2pix', '--drn_path', str(drn)]), log)
    finally:
        log.removeHandler(h)
    assert callable(ev)
    assert len(lines) == 1 and 'mIoU' in lines[0] and str(drn) in lines[0]


# ---- 5. the ABI surface -------------------------------------------------------------------------------------------------------
def test_abi_surface():
    from gcc_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'gcc_hip.h')).read()
    for name in ('gcc_phase_regroup', 'gcc_relu_bf16', 'gcc_seg_head'):
        assert name in _lib.PROTOTYPES
        m = re.search(r'^int %s\(([^;]*)\);' % name, header, re.M)
        assert m, name
        assert len(m.group(1).split(',')) == len(_lib.PROTOTYPES[name][1])
    assert re.search(r'#define GCC_HIP_ABI 605\b', header) and _lib.GCC_HIP_ABI == 605
    build = open(os.path.join(ROOT, 'gcc_amd', 'csrc', 'build.sh')).read()
    assert re.search(r'^SRCS=".*\bsegnet\b.*"', build, re.M)
