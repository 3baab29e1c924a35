"""The host side of the reference's output blocks (InceptionFidEngine(output_blocks=, pooled=), GCC_FID_DIMS, fid_score --dims,
get_real_stat --dims): the validation of the argument and of the variable, the truncated launch programs of a thin net -- prefixes
of the whole network's, with a 'tap' step where a block's map stands --, the block widths, and the text of the labels.  No
device."""
import argparse
from collections import Counter

import numpy as np
import pytest
import torch

from gcc_amd._lib import GccError
from gcc_amd.metric import fid_eval as FE
from gcc_amd.metric import fid_score as F
from gcc_amd.metric import get_real_stat as G
from gcc_amd.metric._native import Act
from gcc_amd.metric.inception_fid import BLOCK_INDEX_BY_DIM, InceptionFidEngine, parse_fid_inception
from tests import _inception_emul as E

RESIZE = 75


@pytest.fixture(scope='module')
def sd():
    return E.seeded(8, 22)


class _Tiny(torch.nn.Module):
    def forward(self, x):
        return [x.mean((2, 3), keepdim=True)]


def test_output_blocks_are_validated_deduplicated_and_sorted(sd):
    assert BLOCK_INDEX_BY_DIM == {64: 0, 192: 1, 768: 2, 2048: 3}
    default = InceptionFidEngine(sd, resize=RESIZE)
    assert default.output_blocks == (3,) and default.pooled is False and default.d == 256
    assert InceptionFidEngine(sd, RESIZE, 'bf16', (3,), False).output_blocks == (3,)
    for given, want in (([2, 0, 2], (0, 2)), ((3, 1), (1, 3)), ((0,), (0,)), ({1, 2}, (1, 2)), ((3, 2, 1, 0), (0, 1, 2, 3))):
        eng = InceptionFidEngine(sd, resize=RESIZE, output_blocks=given)
        assert eng.output_blocks == want and eng.d == eng.block_widths[want[-1]]
    for bad in ((), (4,), (-1,), (0, 4), ('3',), (1.0,), (True,), None, 3):
        with pytest.raises(GccError, match=r'output_blocks .*expected one or more of 0, 1, 2, 3'):
            InceptionFidEngine(sd, resize=RESIZE, output_blocks=bad)
    with pytest.raises(GccError, match=r'\.to\(device\) first'):
        InceptionFidEngine(sd, resize=RESIZE, output_blocks=(0,), pooled=True)(torch.zeros(1, 3, 8, 8))


def test_block_widths_come_from_the_shapes(sd):
    assert InceptionFidEngine(sd, resize=RESIZE, output_blocks=(1,)).block_widths == {0: 8, 1: 24, 2: 96, 3: 256}
    arch = parse_fid_inception(E.shapes(1))                                 # the real widths, as bare shapes
    assert arch.block_widths == {0: 64, 1: 192, 2: 768, 3: 2048} and arch.d == 2048
    assert {d: arch.block_widths[b] for d, b in BLOCK_INDEX_BY_DIM.items()} == {d: d for d in BLOCK_INDEX_BY_DIM}


def _describe(st):
    """a step as plain data: kinds, convs by key, activations by their geometry and region"""
    out = []
    for a in st:
        if isinstance(a, Act):
            out.append((a.C, a.h, a.w, a.region, a.ld, a.off))
        else:
            out.append(getattr(a, 'key', a))
    return tuple(out)


@pytest.mark.parametrize('precision', ('bf16', 'fp32'))
def test_truncated_programs_are_prefixes_of_the_whole_network_s(sd, precision):
    full_eng = InceptionFidEngine(sd, resize=RESIZE, precision=precision)
    full = [_describe(st) for st in full_eng._program(3).steps]
    assert all(st[0] != 'tap' for st in full)                               # the default program is today's: no tap step
    counts = {0: (3, 1), 1: (5, 2), 2: (70, 10), 3: (94, 13)}
    maps = {0: (8, 17, 17), 1: (24, 7, 7), 2: (96, 3, 3)}
    before = None
    for block in (0, 1, 2, 3):
        eng = InceptionFidEngine(sd, resize=RESIZE, precision=precision, output_blocks=(block,), pooled=True)
        prog = eng._program(3)
        steps = [_describe(st) for st in prog.steps]
        kinds = Counter(st[0] for st in steps)
        assert (kinds['conv'], kinds['pool']) == counts[block]
        if precision == 'fp32':
            assert kinds['border'] == 0 and len(steps) == sum(counts[block]) + (block < 3)
        if block < 3:
            assert kinds['tap'] == 1 and steps[-1][:2] == ('tap', block) and steps[-1][2][:3] == maps[block]
            assert steps[:-1] == full[:len(steps) - 1]                      # same kinds, same geometry, same regions
            acts = [a for st in prog.steps for a in st if isinstance(a, Act) and a.region >= 0]
            assert prog.size_r == max(3 * a.h * a.w * a.ld for a in acts)       # the slab is sized for the truncated program
            assert prog.total == prog.size_in + 4 * prog.size_r <= full_eng._program(3).total
            assert eng.flops() < full_eng.flops() and (before is None or eng.flops() > before)
            before = eng.flops()
        else:
            assert steps == full and eng.flops() == full_eng.flops() and prog.total == full_eng._program(3).total
        assert eng.d == eng.block_widths[block]
    # every block at once: the whole program with the three taps where their maps are produced, before the region is reused
    allb = InceptionFidEngine(sd, resize=RESIZE, precision=precision, output_blocks=(0, 1, 2, 3))
    steps = [_describe(st) for st in allb._program(3).steps]
    assert [st for st in steps if st[0] != 'tap'] == full
    for block in (0, 1, 2):
        i = steps.index(next(st for st in steps if st[:2] == ('tap', block)))
        tap, writer = steps[i][2], steps[i - 1][-1]                          # the step before wrote (the last slice of) the map
        assert steps[i - 1][0] in ('conv', 'pool') and (tap[1:4], tap[4]) == (writer[1:4], writer[4])
        assert writer[5] + writer[0] == tap[0]


def test_the_variable_and_the_argument_choose_the_block(tmp_path, monkeypatch, sd):
    weights = tmp_path / 'pt_inception_thin.pth'
    torch.save(sd, str(weights))
    monkeypatch.setenv(FE.ENV, str(weights))
    monkeypatch.delenv(FE.PRECISION_ENV, raising=False)
    assert FE.DIMS_ENV == 'GCC_FID_DIMS'
    thin = {64: 8, 192: 24, 768: 96, 2048: 256}
    for value, want in ((None, 2048), ('', 2048), ('2048', 2048), ('64', 64), ('192', 192), (' 768 ', 768)):
        if value is None:
            monkeypatch.delenv(FE.DIMS_ENV, raising=False)
        else:
            monkeypatch.setenv(FE.DIMS_ENV, value)
        assert FE.fid_dims() == want
        eng, why = FE.load_inception()
        assert why is None and isinstance(eng, InceptionFidEngine) and eng.pooled is True
        assert eng.output_blocks == (BLOCK_INDEX_BY_DIM[want],) and eng.d == thin[want]
        assert FE.network_label(eng) == (' (native, bf16)' if want == 2048 else ' (native, bf16, dims %d)' % thin[want])
        assert FE.load_inception(192)[0].output_blocks == (1,)              # the argument wins over the variable
    monkeypatch.setenv(FE.PRECISION_ENV, 'fp32')
    monkeypatch.setenv(FE.DIMS_ENV, '768')
    assert FE.network_label(FE.load_inception()[0]) == ' (native, fp32, dims 96)'
    monkeypatch.delenv(FE.PRECISION_ENV)
    for bad in ('65', '0', 'wide', '2048.0', '-64'):
        monkeypatch.setenv(FE.DIMS_ENV, bad)
        with pytest.raises(GccError, match=r'GCC_FID_DIMS=%s: expected one of 64, 192, 768, 2048' % bad):
            FE.load_inception()
        np.savez(str(tmp_path / 'real_stat_B.npz'), mu=np.zeros(256), sigma=np.eye(256))
        from gcc_amd.options import options
        with pytest.raises(GccError, match='GCC_FID_DIMS=%s' % bad):        # gcc_amd.train / gcc_amd.test come through here
            FE.builtin_inception(options.parse(['--dataroot', str(tmp_path), '--model', 'pix2pix']))
        assert FE.load_inception(64)[0].output_blocks == (0,)
    with pytest.raises(GccError, match=r'dims=100: expected one of 64, 192, 768, 2048'):
        FE.load_inception(100)
    # a TorchScript archive runs as it was exported: the width does not apply to it, not even a bad value
    archive = tmp_path / 'tiny.pt'
    torch.jit.script(_Tiny()).save(str(archive))
    monkeypatch.setenv(FE.ENV, str(archive))
    for value in ('64', 'nonsense'):
        monkeypatch.setenv(FE.DIMS_ENV, value)
        net, why = FE.load_inception()
        assert why is None and isinstance(net, torch.jit.ScriptModule) and FE.network_label(net) == ''


def test_a_label_names_the_width_only_below_2048():
    full = parse_fid_inception(E.shapes(1))
    for precision in ('bf16', 'fp32'):
        for dims, block in sorted(BLOCK_INDEX_BY_DIM.items()):
            eng = argparse.Namespace(precision=precision, output_blocks=(block,), d=full.block_widths[block])
            want = ' (native, %s)' % precision if dims == 2048 else ' (native, %s, dims %d)' % (precision, dims)
            assert FE.network_label(eng) == want
    assert FE.network_label(argparse.Namespace(precision='bf16')) == ' (native, bf16)' and FE.network_label(_Tiny()) == ''


def test_fid_score_passes_dims_on_and_an_explicit_flag_wins(monkeypatch):
    asked = []

    class _Net:
        pass

    def load(dims=None):
        asked.append(dims)
        return _Net(), None
    monkeypatch.setattr(FE, 'load_inception', load)
    assert isinstance(F._network(None, 192, torch.device('cuda', 0))(), _Net) and asked == [192]
    # the parser's own default stays the reference's; main() tells a flag that was given from one that was not
    assert F.parser.parse_args(['a', 'b']).dims == 2048
    given = lambda argv: F.parser.parse_args(argv, argparse.Namespace(dims=None)).dims
    assert given(['a', 'b']) is None and given(['a', 'b', '--dims', '64']) == 64 and given(['a', 'b', '--dims', '2048']) == 2048
    monkeypatch.setenv(FE.DIMS_ENV, '768')
    assert FE.fid_dims(given(['a', 'b'])) == 768 and FE.fid_dims(given(['a', 'b', '--dims', '64'])) == 64
    assert FE.fid_dims(given(['a', 'b', '--dims', '2048'])) == 2048
    monkeypatch.delenv(FE.DIMS_ENV)
    assert FE.fid_dims(given(['a', 'b'])) == 2048


def test_get_real_stat_has_its_own_dims_flag(monkeypatch):
    base = ['--dataroot', 'r', '--output_path', 'o.npz']
    monkeypatch.delenv(FE.DIMS_ENV, raising=False)
    assert G.parse(base).dims == 2048 and G.parse(base + ['--dims', '192']).dims == 192
    monkeypatch.setenv(FE.DIMS_ENV, '64')
    assert G.parse(base).dims == 64 and G.parse(base + ['--dims', '768', '--features_path', 'f.npz']).dims == 768
    monkeypatch.setenv(FE.DIMS_ENV, '63')
    with pytest.raises(GccError, match='GCC_FID_DIMS=63'):
        G.parse(base)
    assert G.parse(base + ['--dims', '64']).dims == 64
    with pytest.raises(SystemExit):
        G.parse(base + ['--dims', '65'])
    with pytest.raises(SystemExit):                                         # the reference's own surface does not have it
        G.parser.parse_args(base + ['--dims', '64'])
    assert {a.dest for a in G.dims_parser._actions} - {a.dest for a in G.tool_parser._actions} == {'dims'}


def test_statistics_of_another_width_name_the_command_that_writes_matching_ones(tmp_path):
    path = str(tmp_path / 'real_stat_B.npz')
    np.savez(path, mu=np.zeros(2048), sigma=np.eye(2048))
    with pytest.raises(GccError, match=r'mu \(2048,\) and sigma \(2048, 2048\).*d = 64 .*get_real_stat --dims 64 .*--output_path'):
        FE.load_real_stat(path, 64, 'cpu')
