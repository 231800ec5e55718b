"""tests/cbeam_ref.py, the fp64 restatement of fsmg_beam_search_constrained, without a GPU: it reduces to beam_ref
under an all-allowing constraint and to constraint_ref's greedy draw at W = 1; its fp32 stand-in agrees with fp64 on every clear
group at the GPU tests' shapes; every planted mistake fails a check the GPU tests use; the dead-end fixtures behave as stated."""
import numpy as np
import pytest

import beam_ref as BR
import cbeam_ref as CB
import constraint_ref as CR
from conftest import small_config
from data.constraints import Constraints

TOL = 1e-4


def _small(input_size=40, H=16, L=1, seed=3):
    cfg = small_config(input_size=input_size, max_len=8, embedding_size=8, hidden_size=H, n_layers=L)
    return cfg, CB.f64(CB.ref_params(cfg, seed))


@pytest.mark.parametrize('W,P', [(1, 0), (4, 3), (9, 0)])
def test_all_allowing_constraint_is_beam_ref(W, P):
    cfg, params = _small()
    V1 = 41
    primer = np.random.RandomState(P).randint(0, 40, size=(2, P)) if P else None
    want = BR.beam_search(params, cfg, 2, W, 4, primer=primer)
    for con in (Constraints(V1), Constraints(V1, bias=np.zeros(V1, np.float32), token_class=np.zeros(V1, np.int32),
                                             next_state=np.zeros((1, 1), np.int32))):
        got = CB.beam_search(params, cfg, con, 2, W, 4, primer=primer)
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert np.allclose(got[3], want[3], rtol=0, atol=0)
        assert np.all(got[4]['dead_ends'] == 0)


@pytest.mark.parametrize('K', [0, 7])
def test_width_one_is_the_constrained_greedy_draw(K):
    cfg, params = _small(input_size=60, H=24, L=2)
    con = CR.mixed_constraint(61, K=K, seed=5)
    primer = CR.allowed_primer(con, 3, 4, seed=1)
    toks, scores, lps, _, cs = CB.beam_search(params, cfg, con, 3, 1, 6, primer=primer)
    want, wlp, wcs = CR.generate(params, cfg, con, 3, 6, temperature=0.0, primer=primer)
    assert np.array_equal(toks[:, 0], want)
    assert np.array_equal(cs['state'][:, 0], wcs['state']) and np.array_equal(cs['dead_ends'][:, 0], wcs['dead_ends'])
    assert np.array_equal(cs['open'][:, 0], wcs['open'])
    # the beam's lp carries the bias, generate's does not
    bias = CR._bias(con)
    assert np.allclose(lps[:, 0] - bias[toks[:, 0]], wlp, rtol=0, atol=1e-12)


def _reference_case(H, L):
    cfg = CB.ref_config(H, L)
    params = CB.ref_params(cfg, H)
    con = CR.mixed_constraint(301, K=33, seed=H)
    return cfg, params, con


@pytest.mark.parametrize('H,L', CB.REF_SHAPES)
def test_fp32_stand_in_agrees_on_clear_groups_at_the_gpu_shapes(H, L):
    cfg, params, con = _reference_case(H, L)
    clear = total = 0
    for G, W, P in CB.REF_CASES:
        primer = CR.allowed_primer(con, G, P, seed=G * W + P) if P else None
        ref = CB.beam_search(CB.f64(params), cfg, con, G, W, 4, primer=primer)
        t32, s32, l32, _, c32 = CB.beam_search(params, cfg, con, G, W, 4, primer=primer, dtype=np.float32)
        CB.check_walk(con, t32, s32, l32, c32, primer=primer)
        c, n = CB.check_against(ref, t32, s32, c32, TOL, 4)
        clear, total = clear + c, total + n
    print('H x L %d x %d: %d clear groups of %d' % (H, L, clear, total))
    assert total == 14 and 2 * clear >= total, (clear, total)


def _fails(check):
    try:
        check()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('mistake', CB.MISTAKES)
def test_every_planted_mistake_fails_a_check(mistake):
    # the mixed constraint of the reference test at its smallest shape, and the dead-end fixture
    cfg, params, con = _reference_case(24, 1)
    p64 = CB.f64(params)
    caught = False
    for G, W, P in ((3, 4, 0), (3, 4, 6), (2, 16, 4)):
        primer = CR.allowed_primer(con, G, P, seed=G * W + P) if P else None
        ref = CB.beam_search(p64, cfg, con, G, W, 4, primer=primer)
        t, s, l, _, c = CB.beam_search(p64, cfg, con, G, W, 4, primer=primer, mistake=mistake)
        s32, l32 = s.astype(np.float32), l.astype(np.float32)
        for g in range(G):          # the score law is the device's: restate it on the fp32 values
            for n in range(W):
                s32[g, n] = BR.fp32_sum(l32[g, n])
        caught |= _fails(lambda: CB.check_walk(con, t, s32, l32, c, primer=primer))
        caught |= _fails(lambda: CB.check_against(ref, t, s, c, TOL, 4))
    cfg2 = small_config(input_size=97, max_len=8, embedding_size=8, hidden_size=16, n_layers=1)
    p2 = CB.f64(CB.ref_params(cfg2, 3))
    for dcon in (CB.dead_end_constraint(), CB.dead_end_constraint(all_dead=True), CB.slot_dead_end_constraint()):
        ref = CB.beam_search(p2, cfg2, dcon, 2, 4, 5)
        t, s, l, _, c = CB.beam_search(p2, cfg2, dcon, 2, 4, 5, mistake=mistake)
        l32 = l.astype(np.float32)
        s32 = np.array([[BR.fp32_sum(l32[g, n]) for n in range(4)] for g in range(2)], np.float32)
        caught |= _fails(lambda: CB.check_walk(dcon, t, s32, l32, c))
        caught |= _fails(lambda: CB.check_against(ref, t, s, c, TOL, 5))
    assert caught, mistake


@pytest.mark.parametrize('H,L', [(16, 1), (48, 2)])
def test_dead_end_fixtures(H, L):
    cfg = small_config(input_size=97, max_len=8, embedding_size=8, hidden_size=H, n_layers=L)
    params = CB.f64(CB.ref_params(cfg, 3))
    num, W, G = 5, 4, 2
    toks, scores, lps, gaps, cs = CB.beam_search(params, cfg, CB.dead_end_constraint(), G, W, num)
    for g in range(G):
        # three live hypotheses, best first, then the one that stepped into the dead-end state at the first position: it ranks
        # last although unconstrained tokens gave it the highest score
        assert cs['dead_ends'][g].tolist() == [0, 0, 0, num - 1], cs['dead_ends'][g]
        assert scores[g, 3] > scores[g, 0] and np.all(np.diff(scores[g, :3]) <= 0)
        assert toks[g, 3, 0] in (20, 30) and np.all(np.isin(toks[g, :3], (10, 20, 30)))
        assert np.all(gaps[g] >= 0.02), gaps[g]
    toks, scores, lps, gaps, cs = CB.beam_search(params, cfg, CB.dead_end_constraint(all_dead=True), G, W, num)
    assert np.all(cs['dead_ends'] == num - 1) and np.all(np.isin(toks[:, :, 0], (20, 30)))


def test_sample_beam_constraints_key():
    """model YAML key sample_beam_constraints: none (default: nothing passed on) | loader; sample_constraints keeps its meaning"""
    import train.train as T
    from data.midi_loader import MIDILoader

    class Sampler(object):
        def constraints(self, **kw):
            return MIDILoader(8, persist=False).constraints(**kw)

    key = 'sample_beam_constraints'
    assert T.sample_constraints({}, Sampler(), key) == {} and T.sample_constraints({key: 'none'}, Sampler(), key) == {}
    assert T.sample_constraints({'sample_constraints': 'loader'}, Sampler(), key) == {}
    assert T.sample_constraints({key: 'loader'}, Sampler()) == {}
    got = T.sample_constraints({key: 'loader'}, Sampler(), key)
    assert list(got) == ['constraints'] and got['constraints'].n_slots == 2048
    with pytest.raises(ValueError, match=key):
        T.sample_constraints({key: 'grammar'}, Sampler(), key)
