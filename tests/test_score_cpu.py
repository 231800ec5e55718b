"""The fp64 restatement of fsmg_score's contract (tests/score_ref.py) on hand-made rows, the layout of fsmg_score_config, and the
fp32 headroom of the tolerance the GPU tests (tests/test_score.py) hold log-prob and entropy to.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import score_ref as S
from conftest import ROOT

NINF = -np.inf


def test_ties_rank_lower_index_first():
    z = np.array([[1.0, 3.0, 3.0, 0.5, 3.0]])
    for y, want in ((1, 0), (2, 1), (4, 2), (0, 3), (3, 4)):
        lp, rk, en, am = S.score_rows(z, [y])
        assert rk[0] == want and am[0] == 1
    lp, _, _, _ = S.score_rows(z, [0])
    assert abs(lp[0] - (1.0 - np.log(3 * np.exp(3.0) + np.exp(1.0) + np.exp(0.5)))) < 1e-14


def test_neg_inf_columns_contribute_zero_entropy():
    z = np.array([[0.0, NINF, 0.0, NINF]])
    lp, rk, en, am = S.score_rows(z, [2])
    assert abs(en[0] - np.log(2.0)) < 1e-15 and abs(lp[0] + np.log(2.0)) < 1e-15
    assert rk[0] == 1 and am[0] == 0
    lp, rk, en, am = S.score_rows(z, [3])                      # a -inf target: behind every finite column and the -inf one before it
    assert lp[0] == NINF and rk[0] == 3


def test_one_hot_row_has_entropy_zero():
    z = np.full((1, 9), NINF)
    z[0, 4] = 2.5
    lp, rk, en, am = S.score_rows(z, [4])
    assert en[0] == 0.0 and lp[0] == 0.0 and rk[0] == 0 and am[0] == 4


def test_uniform_row():
    V1 = 37
    z = np.full((V1, V1), 0.25)
    lp, rk, en, am = S.score_rows(z, np.arange(V1))
    assert np.allclose(en, np.log(V1), rtol=0, atol=1e-14) and np.allclose(lp, -np.log(V1), rtol=0, atol=1e-14)
    assert np.array_equal(rk, np.arange(V1))                  # rank = index among the ties
    assert np.all(am == 0)


def test_row_nll_window_is_the_fp64_sum_rounded_once():
    lp = np.log(np.random.RandomState(0).uniform(0.01, 1.0, size=(3, 12))).astype(np.float32)
    got = S.row_nll(lp, 4, 5)
    want = np.float32(-lp[:, 4:9].astype(np.float64).sum(axis=1) / 5.0)
    assert np.allclose(got, want, rtol=1e-7, atol=0)
    assert np.array_equal(S.row_nll(lp), np.float32(-np.array([sum(float(x) for x in row) for row in lp]) / 12.0))


def test_rank_band_contains_the_exact_rank():
    rng = np.random.RandomState(1)
    z = rng.normal(size=(50, 98)) * 1e-3
    y = rng.randint(0, 97, size=50)
    _, rk, _, _ = S.score_rows(z, y)
    lo, hi = S.rank_band(z, y)
    assert np.all(lo <= rk) and np.all(rk <= hi)


@pytest.mark.parametrize('V1', [98, 1025, 10001, 50001])
def test_fp32_evaluation_stays_inside_the_gpu_tolerance(V1):
    """the GPU tests hold log-prob and entropy to 1e-5 * max(1, |value|); the same formulas evaluated in fp32 with numpy on the known-answer
    bias rows stay well below it (about 2e-6 absolute)"""
    b, cols = S.known_bias(V1)
    y = S.known_songs(V1, 2, 16, cols).reshape(-1)
    z = np.broadcast_to(b, (y.size, V1))
    lp64, rk64, en64, am64 = S.score_rows(z, y)
    lp32, rk32, en32, am32 = S.score_rows(z, y, np.float32)
    assert np.array_equal(rk64, rk32) and np.array_equal(am64, am32)
    fin = np.isfinite(lp64)
    assert np.array_equal(lp64[~fin], lp32[~fin].astype(np.float64))
    err_lp = np.abs(lp32[fin] - lp64[fin]) / np.maximum(1.0, np.abs(lp64[fin]))
    err_en = np.abs(en32 - en64) / np.maximum(1.0, np.abs(en64))
    print('V1 = %d: fp32 log-prob error %.3g, entropy error %.3g (scaled by max(1, |value|))' % (V1, err_lp.max(), err_en.max()))
    assert err_lp.max() < 1e-5 and err_en.max() < 1e-5


def test_known_bias_has_the_promised_structure():
    for V1 in (98, 1025, 50001):
        b, cols = S.known_bias(V1)
        assert b[cols['pair_a'][0]] == b[cols['pair_a'][1]] and b[cols['pair_b'][0]] == b[cols['pair_b'][1]]
        assert np.isneginf(b[cols['neg_inf']]) and np.isneginf(b).sum() == 1
        u = np.unique(b[np.isfinite(b)])
        assert u.size == V1 - 3 and np.diff(u.astype(np.float64)).min() >= 0.0099
        songs = S.known_songs(V1, 4, 8, cols)
        assert {0, V1 - 2, cols['neg_inf'], *cols['pair_a'], *cols['pair_b']} <= set(songs.reshape(-1).tolist())


def test_score_config_layout():
    from fsmg.binding import FsmgScoreConfig, FSMG_SCORE_CONFIG_VERSION, FSMG_SCORE_PASS_ROWS
    assert C.sizeof(FsmgScoreConfig) == 64
    assert [f[0] for f in FsmgScoreConfig._fields_] == ['version', 'n_rows', 'tokens_on_device', 'nll_first', 'nll_count', 'pass_rows',
                                                         'reserved']
    text = open(os.path.join(ROOT, 'include', 'fsmg.h')).read()
    assert int(re.search(r'#define FSMG_SCORE_CONFIG_VERSION (\d+)', text).group(1)) == FSMG_SCORE_CONFIG_VERSION
    assert int(re.search(r'#define FSMG_SCORE_PASS_ROWS (\d+)', text).group(1)) == FSMG_SCORE_PASS_ROWS


def test_score_entry_points_are_declared_bound_and_exported():
    from fsmg.build import build
    build()
    from fsmg.binding import SIGNATURES, library_path
    out = subprocess.check_output(['nm', '-D', '--defined-only', library_path()], universal_newlines=True)
    text = open(os.path.join(ROOT, 'include', 'fsmg.h')).read()
    for name in ('fsmg_score', 'fsmg_maml_score'):
        assert name in SIGNATURES and re.search(r' T %s$' % name, out, flags=re.M) and re.search(r'\bint %s\(' % name, text)
