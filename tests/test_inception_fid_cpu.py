"""The host side of the native FID Inception network (gcc_amd.metric.inception_fid, fid_eval.load_inception): which file becomes
an engine, what the parser reads and refuses, the identity the rectangular-kernel route rests on, the restatement the GPU tests
measure against, and the launch count against a recording stand-in for gcc_amd.ops.  No device, no library."""
import pytest
import torch
import torch.nn.functional as F

from gcc_amd._lib import GccError
from gcc_amd.metric import fid_eval as FE
from gcc_amd.metric import inception_fid as I
from tests import _inception_emul as E


@pytest.fixture(scope='module')
def thin():
    return E.seeded(8, 11)


# ---- wiring -------------------------------------------------------------------------------------------------------------------
def test_load_inception_takes_the_reference_s_state_dict_file(tmp_path, monkeypatch, thin):
    path = tmp_path / 'pt_inception_thin.pth'
    torch.save(thin, str(path))
    monkeypatch.setenv(FE.ENV, str(path))
    net, why = FE.load_inception()
    assert why is None and isinstance(net, I.InceptionFidEngine)
    assert net.device is None and net.resize == 299 and net.d == 256          # still on the host, the reference's size
    assert I.is_fid_inception_state_dict(thin) and not I.is_fid_inception_state_dict({'w': torch.zeros(2)})
    assert not I.is_fid_inception_state_dict([1, 2])


def test_an_unrelated_dict_keeps_the_torchscript_reason(tmp_path, monkeypatch):
    plain = tmp_path / 'state_dict.pth'
    torch.save({'w': torch.zeros(2)}, str(plain))
    monkeypatch.setenv(FE.ENV, str(plain))
    net, why = FE.load_inception()
    assert net is None and '\n' not in why
    assert why.startswith('torch.jit.load could not read %s %s as a TorchScript archive (' % (FE.ENV, plain))
    assert why.endswith('a plain state_dict needs the network\'s code: export InceptionV3([3]) with torch.jit once')
    monkeypatch.delenv(FE.ENV)
    assert FE.load_inception() == (None, 'GCC_FID_INCEPTION is not set (the path of a TorchScript archive of the Inception network)')


def test_an_inception_dict_the_engine_refuses_says_so(tmp_path, monkeypatch, thin):
    sd = dict(thin)
    sd['AuxLogits.conv0.conv.weight'] = torch.zeros(8, 8, 1, 1)
    path = tmp_path / 'aux.pth'
    torch.save(sd, str(path))
    monkeypatch.setenv(FE.ENV, str(path))
    net, why = FE.load_inception()
    assert net is None
    assert why.startswith('%s %s holds an Inception state_dict this package does not run: ' % (FE.ENV, path))
    assert 'AuxLogits.conv0.conv.weight' in why


# ---- the parser -----------------------------------------------------------------------------------------------------------------
def test_parser_reads_full_and_thin_widths():
    full = I.parse_fid_inception(E.shapes(1))
    assert full.d == 2048 and len(full.convs) == 94
    assert full.widths == {'Mixed_5b': 256, 'Mixed_5c': 288, 'Mixed_5d': 288, 'Mixed_6a': 768, 'Mixed_6b': 768, 'Mixed_6c': 768,
                           'Mixed_6d': 768, 'Mixed_6e': 768, 'Mixed_7a': 1280, 'Mixed_7b': 2048, 'Mixed_7c': 2048}
    by = {c.name: c for c in full.convs}
    assert (by['Mixed_6c.branch7x7dbl_2'].k, by['Mixed_6c.branch7x7dbl_2'].pad, by['Mixed_6c.branch7x7dbl_2'].co) == ((7, 1), (3, 0), 160)
    assert (by['Mixed_7b.branch3x3_2a'].k, by['Mixed_7b.branch3x3_2a'].pad) == ((1, 3), (0, 1))
    assert (by['Conv2d_1a_3x3'].stride, by['Conv2d_1a_3x3'].ci, by['Conv2d_1a_3x3'].co) == (2, 3, 32)
    assert [(c.ci, c.co) for c in full.convs] == [(ci, co) for _, ci, co, _ in E.conv_table(1)]     # module order, every width
    thin = I.parse_fid_inception(E.shapes(8))
    assert thin.d == 256 == E.feature_width(8)
    assert [(c.name, c.ci, c.co, c.k) for c in thin.convs] == E.conv_table(8)
    assert all(w % 8 == 0 for w in thin.widths.values())


def test_parser_ignores_fc_and_num_batches_tracked(thin):
    bare = {k: v for k, v in thin.items() if not k.startswith('fc.') and not k.endswith('num_batches_tracked')}
    assert len(bare) < len(thin)
    a, b = I.parse_fid_inception(thin), I.parse_fid_inception(bare)
    assert a.widths == b.widths and a.d == b.d
    eng = I.InceptionFidEngine(thin, resize=75)
    assert not any(k.startswith('fc.') or k.endswith('num_batches_tracked') for k in eng.host)


def test_parser_names_the_key(thin):
    shapes = E.shapes(8)
    for key in ('Mixed_6b.branch7x7_2.conv.weight', 'Mixed_7c.branch_pool.bn.running_var', 'Conv2d_1a_3x3.conv.weight'):
        sd = dict(shapes)
        del sd[key]
        with pytest.raises(GccError, match=key.replace('.', r'\.') + ' is missing'):
            I.parse_fid_inception(sd)
    with pytest.raises(GccError, match=r'unknown key AuxLogits\.conv0\.conv\.weight'):
        I.parse_fid_inception(dict(shapes, **{'AuxLogits.conv0.conv.weight': (8, 8, 1, 1)}))
    with pytest.raises(GccError, match=r'unknown key Mixed_5b\.branch1x1\.conv\.bias'):
        I.parse_fid_inception(dict(shapes, **{'Mixed_5b.branch1x1.conv.bias': (8,)}))
    with pytest.raises(GccError, match=r'Mixed_6b\.branch7x7_2\.conv\.weight has shape \(16, 16, 7, 1\), expected a 1 x 7'):
        I.parse_fid_inception(dict(shapes, **{'Mixed_6b.branch7x7_2.conv.weight': (16, 16, 7, 1)}))
    with pytest.raises(GccError, match=r'Mixed_5c\.branch5x5_1\.bn\.bias has shape \(9,\), expected \(8,\)'):
        I.parse_fid_inception(dict(shapes, **{'Mixed_5c.branch5x5_1.bn.bias': (9,)}))
    with pytest.raises(GccError, match=r'Mixed_5d\.branch1x1\.conv\.weight takes 48 channels, the layer before it gives 40'):
        I.parse_fid_inception(dict(shapes, **{'Mixed_5d.branch1x1.conv.weight': (8, 48, 1, 1)}))
    sd = dict(shapes)
    sd['Mixed_5b.branch1x1.conv.weight'] = (12, 24, 1, 1)
    for f in ('weight', 'bias', 'running_mean', 'running_var'):
        sd['Mixed_5b.branch1x1.bn.' + f] = (12,)
    with pytest.raises(GccError, match=r'Mixed_5b\.branch1x1\.conv\.weight has 12 output channels; widths must be multiples of 8'):
        I.parse_fid_inception(sd)
    with pytest.raises(GccError, match='expected a dict'):
        I.parse_fid_inception([])
    with pytest.raises(GccError, match='resize = 60 leaves no pixel at Mixed_7a'):
        I.InceptionFidEngine(thin, resize=60)


# ---- the identity behind the rectangular-kernel route -----------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', [(1, 7), (7, 1), (1, 3), (3, 1)])
def test_border_copy_plus_a_padding_0_conv_is_the_padded_conv(kernel):
    kh, kw = kernel
    ph, pw = kh // 2, kw // 2
    g = torch.Generator().manual_seed(kh * 10 + kw)
    x, w = torch.randn((2, 5, 6, 9), generator=g), torch.randn((4, 5, kh, kw), generator=g)
    xb = torch.full((2, 5, 6 + 2 * ph, 9 + 2 * pw), float('nan'))
    xb[:] = 0                                           # gcc_border_copy: the border is written, whatever was there
    xb[:, :, ph:ph + 6, pw:pw + 9] = x
    assert torch.equal(F.conv2d(xb, w), F.conv2d(x, w, padding=(ph, pw)))


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_the_emulating_mode_without_rounding_is_the_fp32_mode(thin):
    x = E.seeded_input((2, 3, 40, 56), 3)
    f = E.forward(thin, x, 75)
    assert tuple(f.shape) == (2, 256, 1, 1) and f.dtype == torch.float32 and torch.isfinite(f).all()
    assert torch.equal(f, E.forward(thin, x, 75, emulate=True, rounding=False))
    e = E.forward(thin, x, 75, emulate=True)
    err = float((e - f).abs().max())
    assert 0 < err < 0.05 * float(f.abs().max())         # the roundings are there, and they are roundings
    assert float((f > 0).float().mean()) > 0.25 and float(f.std()) > 0.01      # features that tell images apart, not a dead net
    assert not torch.equal(f[0], f[1])


# ---- the launch count ---------------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for gcc_amd.ops under an engine: records what would be launched; a conv with 16 or more input channels takes the
    split-K route (two launches), so the count has to come from the route and not from the number of steps"""

    def __init__(self):
        self.calls = []
        self.real_geom = None

    def route(self, x):
        return 2 if x.shape[1] >= 16 else 1

    def conv_eval_ex(self, x, w, Co, k, stride, pad, out, route_only=False, **kw):
        if route_only:
            return self.route(x)
        self.calls += [('conv', k, k, stride, pad, tuple(x.shape), tuple(out.shape))] * self.route(x)

    def conv_eval_rect(self, x, w, Co, kernel, stride, out, route_only=False, **kw):
        if route_only:
            return self.route(x)
        self.calls += [('conv', kernel[0], kernel[1], stride, 0, tuple(x.shape), tuple(out.shape))] * self.route(x)

    def fid_resize(self, x, out):
        self.calls.append(('resize', tuple(x.shape), tuple(out.shape)))

    def pool3x3(self, mode, x, out):
        self.calls.append(('pool', mode, tuple(x.shape), tuple(out.shape)))

    def border_copy(self, src, dst, ph, pw):
        self.calls.append(('border', ph, pw, tuple(src.shape), tuple(dst.shape)))

    def global_avgpool(self, x, out):
        self.calls.append(('gap', tuple(x.shape)))


def test_infer_launches_against_a_recording_stand_in(monkeypatch, thin):
    from gcc_amd import ops
    rec = _Recorder()
    for name in ('conv_eval_ex', 'conv_eval_rect', 'fid_resize', 'pool3x3', 'border_copy', 'global_avgpool'):
        monkeypatch.setattr(ops, name, getattr(rec, name))
    eng = I.InceptionFidEngine(thin, resize=75)
    monkeypatch.setattr(eng, '_check_routes', lambda prog: None)          # the library's say: asked on the GPU
    eng.device = torch.device('cpu')                                        # as .to() leaves it, without packing anything
    for c in eng.convs:
        c.w = c.scale = c.shift = None
    predicted = eng.infer_launches(3, 40, 56)
    assert rec.calls == []                                                  # counting launches nothing
    out = eng._run(torch.zeros(3, 3, 40, 56), 3)
    assert tuple(out[0].shape) == (3, 256, 1, 1)
    assert len(rec.calls) == predicted
    kinds = [c[0] for c in rec.calls]
    assert kinds[0] == 'resize' and kinds[-1] == 'gap' and kinds.count('resize') == kinds.count('gap') == 1
    assert kinds.count('pool') == 2 + 11                                    # the stem's two, one in each of the eleven blocks
    borders = [c for c in rec.calls if c[0] == 'border']
    assert len(borders) == 4 * 6 + 2 + 2 * 4                                # 6c blocks x 6, 7a x 2, 7b / 7c x 4
    assert {(c[1], c[2]) for c in borders} == {(0, 3), (3, 0), (0, 1), (1, 0)}
    # a rectangular conv always reads a border copy and is asked for without padding; the map sizes are the issue's
    for i, c in enumerate(rec.calls):
        if c[0] == 'conv' and c[1] != c[2]:
            prev = next(p for p in reversed(rec.calls[:i]) if p != c)        # a two-launch conv is recorded twice
            assert prev[0] == 'border' and prev[4] == c[5] and c[4] == 0
    assert sorted({c[6][2] for c in rec.calls if c[0] == 'conv'}, reverse=True) == [37, 35, 17, 15, 7, 3, 1]
    assert eng.flops() == sum(2 * co * ci * kh * kw * hw * hw for (_, ci, co, (kh, kw)), hw in zip(E.conv_table(8), _map_sizes()))


def _map_sizes():
    """output map size of each conv of conv_table at resize = 75"""
    return [37, 35, 35, 17, 15] + [7] * 21 + [3, 7, 7, 3] + [3] * 40 + [3, 1, 3, 3, 3, 1] + [1] * 18
