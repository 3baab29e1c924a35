"""The host half of precision / recall / density / coverage (gcc_amd.metric.prdc_score, fid_eval.prdc_line): the final divisions,
the log line, GCC_FID_PRDC, the header's constants and prototypes against their Python mirrors, and the numpy reference of
tests/_prdc.py against a brute-force fractions.Fraction evaluation.  No GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from . import _prdc as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prdc_from_counts_is_four_integer_divisions():
    from gcc_amd._lib import GccError
    from gcc_amd.metric.prdc_score import KEYS, prdc_from_counts
    got = prdc_from_counts(99, 119, 418, 116, m=129, n=127, k=5)
    assert tuple(got) == KEYS == P.KEYS and all(type(v) is float for v in got.values())
    assert got == {'precision': 99 / 129, 'recall': 119 / 127, 'density': 418 / (5 * 129), 'coverage': 116 / 127}
    for key, frac in zip(KEYS, (Fraction(99, 129), Fraction(119, 127), Fraction(418, 645), Fraction(116, 127))):
        assert abs(Fraction(got[key]) - frac) <= frac * Fraction(1, 2 ** 53)          # one rounding each
    # a set against itself, no ties: every row in its own ball and in those of its k nearest neighbours' ... (k + 1) / k
    assert prdc_from_counts(50, 50, 50 * 6, 50, 50, 50, 5) == {'precision': 1.0, 'recall': 1.0, 'density': 6 / 5, 'coverage': 1.0}
    assert prdc_from_counts(0, 0, 0, 0, 9, 7, 3) == dict.fromkeys(KEYS, 0.0)
    for bad in (dict(m=5, n=9, k=5), dict(m=9, n=5, k=5), dict(m=9, n=9, k=0)):
        with pytest.raises(GccError, match='more than k samples'):
            prdc_from_counts(1, 1, 1, 1, **bad)
    for counts in ((10, 1, 1, 1), (1, 8, 1, 1), (1, 1, 64, 1), (1, 1, 1, 8), (-1, 1, 1, 1)):
        with pytest.raises(GccError, match='do not belong'):
            prdc_from_counts(*counts, m=9, n=7, k=3)


def test_prdc_line_has_one_form_per_model():
    from gcc_amd.metric.fid_eval import prdc_line
    a = {'precision': 0.76744, 'recall': 0.937, 'density': 0.64806, 'coverage': 0.91339}
    b = {'precision': 1.0, 'recall': 0.0, 'density': 1.2, 'coverage': 0.5}
    one = 'Precision: 0.7674 | Recall: 0.9370 | Density: 0.6481 | Coverage: 0.9134'
    assert prdc_line([a], ['AtoB'], 'pix2pix') == one and prdc_line([a], ['BtoA'], 'sagan') == one
    assert prdc_line([a, b], ['AtoB', 'BtoA'], 'cyclegan') == \
        'AtoB ' + one + ' | BtoA Precision: 1.0000 | Recall: 0.0000 | Density: 1.2000 | Coverage: 0.5000'


def test_environment_variable_names_k_or_nothing():
    from gcc_amd import _lib
    from gcc_amd.metric import prdc_score as S
    assert S.ENV == 'GCC_FID_PRDC' and S.DEFAULT_K == 5
    for off in ({}, {S.ENV: ''}, {S.ENV: '0'}, {S.ENV: ' '}):
        assert S.env_k(off) is None
    for k in range(1, _lib.PRDC_MAX_K + 1):
        assert S.env_k({S.ENV: str(k)}) == k
    for bad in (str(_lib.PRDC_MAX_K + 1), '-1', 'five', '2.5'):
        with pytest.raises(_lib.GccError, match=S.ENV):
            S.env_k({S.ENV: bad})


def test_scorer_refuses_a_missing_feature_file_and_a_bad_k(tmp_path):
    from gcc_amd._lib import GccError
    from gcc_amd.metric.fid_eval import FidScorer
    np.savez(str(tmp_path / 'real_stat_B.npz'), mu=np.zeros(3), sigma=np.eye(3))
    slots = [('real_stat_B.npz', 'AtoB')]
    assert FidScorer(None, tmp_path, slots).prdc() is None             # not asked for: no line, nothing needed
    with pytest.raises(GccError, match=r'GCC_FID_PRDC=3 .*real_act_B\.npz missing .*get_real_stat .*--features_path'):
        FidScorer(None, tmp_path, slots, prdc_k=3)
    with pytest.raises(GccError, match='GCC_FID_PRDC = 9'):
        FidScorer(None, tmp_path, slots, prdc_k=9)


def test_header_constants_and_prototypes_have_their_mirrors():
    from gcc_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gcc_hip.h')).read()
    for name in ('TILE', 'COL_TILE', 'SMALL_TILE', 'SMALL_BELOW', 'KSTEP', 'MAX_K', 'MAX_CHUNKS', 'FILL_WORKGROUPS'):
        assert int(re.search(r'#define\s+GCC_PRDC_%s\s+(\d+)' % name, hdr).group(1)) == getattr(_lib, 'PRDC_' + name), name
    assert _lib.PRDC_MAX_K == 8
    assert int(re.search(r'#define\s+GCC_HIP_ABI\s+(\d+)', hdr).group(1)) == 605
    for name in ('gcc_prdc_workspace', 'gcc_prdc_tile', 'gcc_prdc_chunks', 'gcc_prdc_kth_dist', 'gcc_prdc_ball_count'):
        m = re.search(r'\b%s\(([^;]*?)\);' % name, hdr, re.S)
        assert m and name in _lib.PROTOTYPES
        assert len(m.group(1).split(',')) == len(_lib.PROTOTYPES[name][1])
    src = open(os.path.join(ROOT, 'gcc_amd', 'csrc', 'build.sh')).read()
    assert re.search(r'^SRCS=".*\bprdc\b.*"', src, re.M)


def test_numpy_reference_against_brute_force_fractions():
    rng = np.random.RandomState(2)
    # a small lattice: ties at the radii and duplicate rows are certain
    R = rng.randint(0, 4, (13, 2)).astype(np.float64)
    F = rng.randint(1, 6, (11, 2)).astype(np.float64)
    seen = set()
    for k in (1, 3, 5):
        want = P.counts_fraction(R, F, k)
        values, counts = P.prdc_ref(R, F, k)
        exact, budget = P.prdc_int(R, F, k)
        assert counts == want == exact and budget < 2 ** 53
        assert values == {'precision': want[0] / 11, 'recall': want[1] / 13, 'density': want[2] / (k * 11), 'coverage': want[3] / 13}
        seen.add(want)
    assert len(seen) == 3 and all(0 < c for w in seen for c in w)
    # inclusive: with every <= read as < the lattice gives other counts
    D, _ = P.sqdist_int(R, F)
    rR = P.kth_int(R, None, 3)[0]
    assert (D <= rR[:, None]).sum() > (D < rR[:, None]).sum()
    # the k-th value and the counts by the matrix helpers
    assert np.array_equal(P.kth_ref(R, None, 3), rR) and np.array_equal(P.ball_ref(F, R, rR), (D <= rR[:, None]).sum(0))
    assert np.array_equal(P.ball_int(F, R, rR)[0], P.ball_ref(F, R, rR))
    # real-valued rows, float64 against fractions of the same float64 inputs
    Rg, Fg = P.gaussian_sets(12, 10, 3)
    assert P.margin(Rg, Fg, 2) > 0 and P.prdc_ref(Rg, Fg, 2)[1] == P.counts_fraction(Rg, Fg, 2)


def test_a_set_against_itself_and_the_documented_shapes():
    # prdc(X, X, k) without ties: precision = recall = coverage = 1, density = (k + 1) / k
    X, _ = P.gaussian_sets(60, 60, 7)
    for k in (1, 3, 5, 8):
        values, counts = P.prdc_ref(X, X, k)
        assert counts == (60, 60, 60 * (k + 1), 60) and values['density'] == (k + 1) / k
    # the three Gaussian shapes: a reference margin far above the bound, values well inside (0, 1)
    for n, m, d in ((129, 127, 17), (257, 130, 70), (300, 260, 64)):
        R, F = P.gaussian_sets(n, m, d)
        values, _ = P.prdc_ref(R, F, 5)
        margin = P.margin(R, F, 5)
        print((n, m, d), values, 'margin %.3g, bound at D = 2 d: %.3g' % (margin, P.dist_bound(d, 2.0 * d)))
        assert margin > 1e6 * P.dist_bound(d, 2.0 * d)
        assert all(0.05 < values[key] < 0.999 for key in ('precision', 'recall', 'coverage')) and 0.05 < values['density']
