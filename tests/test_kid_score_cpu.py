"""The host side of KID and of the path-based FID (gcc_amd.metric.kid_score, fid_score, get_real_stat): arithmetic, argument
parsing, file names, folder listing, the batch rule, and the C entry points' declaration -- nothing here needs a GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from . import _kid as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kid_from_sums_against_fractions():
    from gcc_amd._lib import GccError
    from gcc_amd.metric.kid_score import kid_from_sums
    rng = np.random.RandomState(0)
    for m, n in ((2, 2), (120, 140), (500, 20000), (7, 5)):
        # dyadic sums: every float below is an exact rational, so the only roundings are kid_from_sums' own five
        sxx, syy, sxy = (float(rng.randint(-2 ** 30, 2 ** 30)) / 64 for _ in range(3))
        want = Fraction(sxx) / (m * (m - 1)) + Fraction(syy) / (n * (n - 1)) - 2 * Fraction(sxy) / (m * n)
        mag = abs(Fraction(sxx)) / (m * (m - 1)) + abs(Fraction(syy)) / (n * (n - 1)) + 2 * abs(Fraction(sxy)) / (m * n)
        got = kid_from_sums(sxx, syy, sxy, m, n)
        assert isinstance(got, float) and abs(Fraction(got) - want) <= 5 * Fraction(2) ** -53 * mag, (m, n)
    assert kid_from_sums(6.0, 2.0, 4.0, 3, 2) == 6.0 / 6 + 2.0 / 2 - 2 * 4.0 / 6
    # identical sets of two points x, y: sxx = syy = 2 k(x, y), sxy = k(x, x) + k(y, y) + 2 k(x, y)
    assert kid_from_sums(2 * 3.0, 2 * 3.0, 5.0 + 7.0 + 2 * 3.0, 2, 2) == 3.0 + 3.0 - 2 * 18.0 / 4
    for m, n in ((1, 5), (5, 1), (0, 0)):
        with pytest.raises(GccError, match='at least 2'):
            kid_from_sums(1.0, 1.0, 1.0, m, n)


@pytest.mark.parametrize('case', ((65, 63, 16, 8), (64, 64, 2048, 2), (33, 33, 64, 4)), ids=lambda c: 'x'.join(map(str, c)))
def test_a_plain_float64_evaluation_is_exact_in_the_exact_regime(case):
    """the premise of tests/test_kid_kernels_gpu.py's exact cases, checked where no kernel is involved"""
    m, n, d, r = case
    rng = np.random.RandomState(d)
    X, Y = (rng.randint(-r, r + 1, (rows, d)).astype(np.float64) for rows in (m, n))
    X[0], Y[0] = r, r
    for a, b in ((X, Y), (X, None)):
        want, budget = K.poly_exact(a, b)
        assert budget < 2 ** 53
        S, T3, pairs = K.poly_ref(a, b)
        assert Fraction(S) == want and pairs == (m * n if b is not None else m * (m - 1))
        assert K.poly_bound(d, pairs, T3) > 0
    assert K.poly_exact(X, X)[0] - K.diag_exact(X) == K.poly_exact(X)[0]


def test_kid_ref_is_the_definition():
    rng = np.random.RandomState(1)
    X, Y = rng.rand(5, 3), rng.rand(4, 3)
    k = lambda a, b: (float(np.dot(a, b)) / 3 + 1) ** 3
    want = sum(k(X[i], X[j]) for i in range(5) for j in range(5) if i != j) / 20 \
        + sum(k(Y[i], Y[j]) for i in range(4) for j in range(4) if i != j) / 12 \
        - 2 * sum(k(x, y) for x in X for y in Y) / 20
    got, bound = K.kid_ref(X, Y)
    assert abs(got - want) <= 1e-13 and 0 < bound < 1e-12


def test_fid_score_parser_is_the_reference_surface():
    from gcc_amd.metric import fid_score as F
    a = F.parser.parse_args(['fake', 'real'])
    assert (a.path, a.batch_size, a.dims, a.gpu) == (['fake', 'real'], 50, 2048, '')
    a = F.parser.parse_args(['x', 'y.npz', '--batch-size', '8', '--dims', '768', '-c', '1'])
    assert (a.path, a.batch_size, a.dims, a.gpu) == (['x', 'y.npz'], 8, 768, '1')
    assert F.parser.parse_args(['x', 'y', '--gpu', '2']).gpu == '2'
    for bad in (['only_one'], ['a', 'b', 'c'], ['a', 'b', '--dims', '65']):
        with pytest.raises(SystemExit):
            F.parser.parse_args(bad)


def test_features_path_is_the_tools_own_flag_and_defaults_to_none():
    from gcc_amd.metric import get_real_stat as G
    base = ['--dataroot', 'd', '--output_path', 'o.npz']
    assert G.parse(base).features_path is None
    assert G.parse(base + ['--features_path', 'real_act_B.npz']).features_path == 'real_act_B.npz'
    # the reference's surface stays what it was; the flag lives on the parser the tool adds around it
    assert 'features_path' not in {a.dest for a in G.parser._actions}
    assert {a.dest for a in G.tool_parser._actions} - {a.dest for a in G.parser._actions} == {'features_path'}
    # no option joins the models' parsed option set
    golden = open(os.path.join(ROOT, 'gcc_amd', 'options', 'options.py')).read()
    assert 'features_path' not in golden


def test_feature_file_name_follows_the_statistics_file():
    from gcc_amd.metric.kid_score import features_name
    assert features_name('real_stat_B.npz') == 'real_act_B.npz'
    assert features_name('real_stat_A.npz') == 'real_act_A.npz'
    assert features_name('real_stat.npz') == 'real_act.npz'
    assert features_name(os.path.join('database', 'real_stat_x', 'real_stat_B.npz')) == os.path.join('database', 'real_stat_x', 'real_act_B.npz')
    assert features_name('stats.npz') is None and features_name('real_stat_B.txt') is None


def test_scorer_looks_for_a_feature_file_beside_every_slot(tmp_path):
    from gcc_amd.metric import fid_eval as E
    from gcc_amd.metric.kid_score import save_features
    opt = type('O', (), {'model': 'cyclegan', 'direction': 'AtoB', 'dataroot': str(tmp_path)})
    sc = E.FidScorer(None, opt.dataroot, E.real_stat_slots(opt))
    assert sc.feature_files == [str(tmp_path / 'real_act_B.npz'), str(tmp_path / 'real_act_A.npz')]
    assert not sc.with_kid and sc.kid() is None and all(not st.keep_features and st.features is None for st in sc.stats)
    save_features(str(tmp_path / 'real_act_B.npz'), np.zeros((3, 4), np.float32), '')
    assert not E.FidScorer(None, opt.dataroot, E.real_stat_slots(opt)).with_kid              # one of two
    save_features(str(tmp_path / 'real_act_A.npz'), np.zeros((3, 4), np.float32), ' (native, fp32)')
    sc = E.FidScorer(None, opt.dataroot, E.real_stat_slots(opt))
    assert sc.with_kid and all(st.keep_features for st in sc.stats)
    assert E.kid_line([0.5, 0.25], ['AtoB', 'BtoA'], 'cyclegan') == 'AtoB KID: 0.500000 | BtoA KID: 0.250000'
    assert E.kid_line([0.0123456789], ['AtoB'], 'pix2pix') == 'KID: 0.012346'


def test_feature_files_round_trip_on_the_host(tmp_path):
    from gcc_amd._lib import GccError
    from gcc_amd.metric import kid_score as S
    act = np.random.RandomState(2).rand(7, 5)
    path = str(tmp_path / 'real_act.npz')
    S.save_features(path, act, ' (native, bf16)')
    with np.load(path) as z:
        assert sorted(z.files) == ['act', 'network'] and z['act'].dtype == np.float32 and z['act'].shape == (7, 5)
        assert str(z['network']) == ' (native, bf16)'
    got, label = S.load_features(path)
    assert label == ' (native, bf16)' and np.array_equal(got.numpy(), act.astype(np.float32)) and S.is_features_file(path)
    with pytest.raises(GccError, match='d = 6'):
        S.load_features(path, d=6)
    stat = str(tmp_path / 'real_stat.npz')
    np.savez(stat, mu=np.zeros(5), sigma=np.eye(5))
    assert not S.is_features_file(stat)
    with pytest.raises(GccError, match='not activations'):
        S.load_features(stat)


def test_folder_listing_is_sorted_and_takes_jpg_and_png_only(tmp_path):
    from gcc_amd.metric.fid_score import list_image_files
    for name in ('b.png', 'a.jpg', 'c.png', 'notes.txt', 'd.jpeg', 'e.PNG', 'a.npz', '10.png', '9.png'):
        (tmp_path / name).write_bytes(b'')
    (tmp_path / 'sub.png').mkdir()
    (tmp_path / 'sub.png' / 'z.png').write_bytes(b'')
    got = [os.path.basename(f) for f in list_image_files(tmp_path)]
    assert got == ['10.png', '9.png', 'a.jpg', 'b.png', 'c.png']
    assert all(os.path.dirname(f) == str(tmp_path) for f in list_image_files(tmp_path))


def test_batch_clamp_and_remainder_rule():
    from gcc_amd._lib import GccError
    from gcc_amd.metric.fid_score import batch_plan
    said = []
    assert batch_plan(100, 50, said.append) == (50, 2) and said == []
    assert batch_plan(11, 4, said.append) == (4, 2) and len(said) == 1 and 'not a multiple' in said[0]       # 3 images dropped
    said.clear()
    assert batch_plan(7, 50, said.append) == (7, 1)                  # clamped: every image is used
    assert len(said) == 2 and 'not a multiple' in said[0] and 'bigger than the datasets size' in said[1]
    said.clear()
    assert batch_plan(1, 1, said.append) == (1, 1) and said == []
    for files, bs in ((0, 4), (4, 0)):
        with pytest.raises(GccError):
            batch_plan(files, bs)


def test_entry_points_are_declared_bound_and_exported():
    import ctypes
    from gcc_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gcc_hip.h')).read()
    assert int(re.search(r'#define\s+GCC_HIP_ABI\s+(\d+)', hdr).group(1)) == 605 == _lib.GCC_HIP_ABI         # additions only
    assert int(re.search(r'#define\s+GCC_KID_TILE\s+(\d+)', hdr).group(1)) == _lib.KID_TILE
    assert int(re.search(r'#define\s+GCC_KID_KSTEP\s+(\d+)', hdr).group(1)) == _lib.KID_KSTEP
    for name in ('gcc_kid_workspace', 'gcc_kid_poly_sum'):
        m = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m and name in _lib.PROTOTYPES
        assert len(m.group(1).split(',')) == len(_lib.PROTOTYPES[name][1])
    lib = _lib.load()
    # a host function: callable without a GPU
    lib.gcc_kid_workspace.restype = ctypes.c_size_t
    T = _lib.KID_TILE
    assert lib.gcc_kid_workspace(20000, 20000, 2048) == (-(-20000 // T)) ** 2 * 8
    assert lib.gcc_kid_workspace(T + 1, 1, 1) == 16 and lib.gcc_kid_workspace(0, 1, 1) == 0
