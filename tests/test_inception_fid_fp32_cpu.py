"""The host side of the fp32 FID Inception route (InceptionFidEngine(sd, precision='fp32'), GCC_FID_PRECISION): the validation of
the argument and of the variable, the fp32 launch program of a thin net -- no 'border' step, every slice on the 4-float grid,
every conv step with the reference's own padding --, and the text of the log lines.  No device."""
import numpy as np
import pytest
import torch

from gcc_amd._lib import GccError
from gcc_amd.metric import fid_eval as FE
from gcc_amd.metric.inception_fid import PRECISIONS, InceptionFidEngine
from gcc_amd.options import options
from tests import _inception_emul as E
from tests import _inception_f64 as E64


@pytest.fixture(scope='module')
def sd():
    return E.seeded(8, 22)


class _Tiny(torch.nn.Module):
    def forward(self, x):
        return [x.mean((2, 3), keepdim=True)]


def test_precision_is_validated_and_exposed(sd):
    assert PRECISIONS == ('bf16', 'fp32')
    assert InceptionFidEngine(sd).precision == 'bf16' and InceptionFidEngine(sd)._slab_dtype == torch.bfloat16
    assert InceptionFidEngine(sd, 75, 'bf16').precision == 'bf16'
    eng = InceptionFidEngine(sd, resize=75, precision='fp32')
    assert eng.precision == 'fp32' and eng._slab_dtype == torch.float32 and eng.resize == 75
    for bad in ('fp16', 'FP32', '', None, 32):
        with pytest.raises(GccError, match=r'InceptionFidEngine: precision %s; expected one of bf16, fp32' % repr(bad).replace('\\', '')):
            InceptionFidEngine(sd, precision=bad)
    assert eng.flops() == InceptionFidEngine(sd, resize=75).flops() > 0    # the same convolutions
    with pytest.raises(GccError, match=r'resize = 20 leaves no pixel at'):  # the refusal texts are the bf16 engine's
        InceptionFidEngine(sd, resize=20, precision='fp32')
    with pytest.raises(GccError, match=r'\.to\(device\) first'):
        eng(torch.zeros(1, 3, 8, 8))


def test_the_variable_is_validated_where_the_engine_is_built(tmp_path, monkeypatch, sd):
    weights = tmp_path / 'pt_inception_thin.pth'
    torch.save(sd, str(weights))
    monkeypatch.setenv(FE.ENV, str(weights))
    assert FE.PRECISION_ENV == 'GCC_FID_PRECISION'
    for value, want in ((None, 'bf16'), ('', 'bf16'), ('bf16', 'bf16'), ('fp32', 'fp32')):
        if value is None:
            monkeypatch.delenv(FE.PRECISION_ENV, raising=False)
        else:
            monkeypatch.setenv(FE.PRECISION_ENV, value)
        eng, why = FE.load_inception()
        assert why is None and isinstance(eng, InceptionFidEngine) and eng.precision == want and eng.resize == 299
        assert FE.network_label(eng) == ' (native, %s)' % want
    for bad in ('fp16', 'float32', 'FP32'):
        monkeypatch.setenv(FE.PRECISION_ENV, bad)
        with pytest.raises(GccError, match=r'GCC_FID_PRECISION=%s: expected one of bf16, fp32' % bad):
            FE.load_inception()
        np.savez(str(tmp_path / 'real_stat_B.npz'), mu=np.zeros(256), sigma=np.eye(256))
        with pytest.raises(GccError, match='GCC_FID_PRECISION=%s' % bad):
            FE.builtin_inception(options.parse(['--dataroot', str(tmp_path), '--model', 'pix2pix']))
    # a TorchScript archive runs as it was exported: the variable does not apply to it, not even a bad value
    archive = tmp_path / 'tiny.pt'
    torch.jit.script(_Tiny()).save(str(archive))
    monkeypatch.setenv(FE.ENV, str(archive))
    for value in ('fp32', 'nonsense'):
        monkeypatch.setenv(FE.PRECISION_ENV, value)
        net, why = FE.load_inception()
        assert why is None and isinstance(net, torch.jit.ScriptModule) and FE.network_label(net) == ''
    # a file that is neither is refused as before, whatever the variable says
    plain = tmp_path / 'other.pth'
    torch.save({'w': torch.zeros(2)}, str(plain))
    monkeypatch.setenv(FE.ENV, str(plain))
    net, why = FE.load_inception()
    assert net is None and 'TorchScript archive' in why


class _Recorder(E._Net):
    """the restatement's forward, noting what each BasicConv2d is called with"""

    def __init__(self, sd):
        super().__init__(sd, False, False)
        self.calls = {}

    def conv(self, name, x, stride=1, padding=0):
        self.calls[name] = (stride, (padding, padding) if isinstance(padding, int) else tuple(padding))
        return super().conv(name, x, stride, padding)


def test_the_fp32_program_has_no_border_step_and_carries_the_reference_s_paddings(sd):
    eng = InceptionFidEngine(sd, resize=75, precision='fp32')
    prog = eng._program(3)
    kinds = [st[0] for st in prog.steps]
    assert set(kinds) == {'conv', 'pool'} and kinds.count('conv') == 94 and kinds.count('pool') == 13
    bf16 = InceptionFidEngine(sd, resize=75)._program(3)
    borders = [st for st in bf16.steps if st[0] == 'border']
    assert len(borders) == sum(1 for c in eng.convs if c.k[0] != c.k[1]) > 0           # what the fp32 program does without
    assert len(prog.steps) == len(bf16.steps) - len(borders)
    # the paddings and strides the restatement's forward passes to F.conv2d, layer by layer
    rec = _Recorder({k: v for k, v in sd.items() if not k.startswith('fc.')})
    with torch.no_grad():
        rec.forward(E.seeded_input((1, 3, 40, 56), 1), 75)
    assert len(rec.calls) == 94
    seen = set()
    for st in prog.steps:
        if st[0] != 'conv':
            continue
        _, c, src, dst = st
        assert (c.stride, tuple(c.pad)) == rec.calls[c.name], c.name
        ho = (src.h + 2 * c.pad[0] - c.k[0]) // c.stride + 1
        wo = (src.w + 2 * c.pad[1] - c.k[1]) // c.stride + 1
        assert (dst.h, dst.w) == (ho, wo) and src.C == c.ci and dst.C == c.co, c.name      # the source is the unpadded map
        seen.add(c.name)
    assert len(seen) == 94
    assert prog.last.C == eng.d == 256 and (prog.last.h, prog.last.w) == (1, 1)


def test_the_fp32_program_writes_every_slice_on_the_four_float_grid(sd):
    from gcc_amd.metric._native import Act
    eng = InceptionFidEngine(sd, resize=75, precision='fp32')
    prog = eng._program(2)
    acts = [a for st in prog.steps for a in st[1:] if isinstance(a, Act)]
    assert all(a.off % 4 == 0 and a.ld % 4 == 0 and a.C % 4 == 0 or a.region < 0 for a in acts)
    x_in = prog.steps[0][2]
    assert (x_in.C, x_in.ld, x_in.off, x_in.region) == (3, 4, 0, -1) and prog.size_in == 2 * 75 * 75 * 4       # 3 in 4 channels
    assert InceptionFidEngine(sd, resize=75)._program(2).size_in == 2 * 75 * 75 * 8
    # zero-copy concatenation: a block's branches write their slices of its output in order, from channel 0 to its width, with
    # no gap and no overlap
    open_block, blocks = None, 0
    for st in prog.steps:
        dst = st[3]
        if dst.ld == dst.C:
            continue
        if dst.off == 0:
            assert open_block is None or open_block[1] == open_block[0].ld             # the block before it was written whole
            open_block, blocks = [dst, 0], blocks + 1
        assert open_block is not None and (dst.region, dst.ld, dst.h, dst.w) == tuple(
            getattr(open_block[0], k) for k in ('region', 'ld', 'h', 'w'))
        assert dst.off == open_block[1], (st[0], dst.off, open_block[1])
        open_block[1] += dst.C
    assert blocks == 11 and open_block[1] == open_block[0].ld == eng.d
    assert prog.total == prog.size_in + 4 * prog.size_r


def test_the_float64_restatement_is_the_network_of_the_fp32_one(sd):
    """tests/_inception_f64.py against tests/_inception_emul.py on the host: the same network (a wrong block would show as 1e-1),
    the fp32 restatement within 1e-5 of it -- the yardstick of tests/test_inception_fid_fp32_gpu.py is a rounding-sized number --
    and the bf16-emulating restatement some four orders of magnitude further away"""
    x = E.seeded_input((2, 3, 40, 56), 122)
    want = E64.forward64(sd, x, 75)
    ref = E.forward(sd, x, 75)
    assert want.dtype == torch.float64 and tuple(want.shape) == tuple(ref.shape) == (2, 256, 1, 1)
    err32, _ = E64.errors(want, ref, ref)
    err16, _ = E64.errors(want, ref, E.forward(sd, x, 75, emulate=True))
    print('fp32 restatement %.3g, bf16-emulating restatement %.3g from float64; max |feature| %.3f' % (err32, err16, float(want.abs().max())))
    assert 0 < err32 < 1e-5 and err16 > 1000 * err32


def test_the_log_lines_name_the_native_precision(tmp_path, monkeypatch, sd, capsys):
    from gcc_amd import train
    weights = tmp_path / 'pt_inception_thin.pth'
    torch.save(sd, str(weights))
    np.savez(str(tmp_path / 'real_stat_B.npz'), mu=np.zeros(256), sigma=np.eye(256))
    monkeypatch.setenv(FE.ENV, str(weights))
    opt = options.parse(['--dataroot', str(tmp_path), '--model', 'pix2pix'])
    for value, want in ((None, 'bf16'), ('fp32', 'fp32')):
        if value is None:
            monkeypatch.delenv(FE.PRECISION_ENV, raising=False)
        else:
            monkeypatch.setenv(FE.PRECISION_ENV, value)
        lines = []
        logger = type('L', (), {'info': staticmethod(lines.append)})
        ev = train.builtin_evaluator(opt, logger)
        assert callable(ev)
        assert lines == ['FID evaluation every %d epochs with the Inception network %s (native, %s)' % (opt.save_epoch_freq, weights, want)]
    archive = tmp_path / 'tiny.pt'
    torch.jit.script(_Tiny()).save(str(archive))
    monkeypatch.setenv(FE.ENV, str(archive))
    np.savez(str(tmp_path / 'real_stat_B.npz'), mu=np.zeros(3), sigma=np.eye(3))
    lines = []
    assert callable(train.builtin_evaluator(opt, type('L', (), {'info': staticmethod(lines.append)})))
    assert lines == ['FID evaluation every %d epochs with the Inception network %s' % (opt.save_epoch_freq, archive)]
