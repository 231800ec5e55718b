"""The decode-time half of the self-cache's fp64 restatement (tests/selfcache_ref.py): the union's distribution against
cachegen_ref on the explicit entry list, the free-running decoder with the own-history step against its own teacher-forced check, and
the near-tie counts of the inputs the GPU test uses, for the reference alone.  No GPU."""
import numpy as np
import pytest

import cachegen_ref as CG
import selfcache_ref as SC


def test_distribution_is_cachegen_over_the_explicit_list():
    rng = np.random.RandomState(0)
    n, S, H, V1, W = 5, 9, 6, 12, 4
    q, z = rng.normal(size=(n, H)), rng.normal(size=(n, V1))
    sk, sv = rng.normal(size=(n, S, H)), rng.randint(0, 4, size=(n, S))
    sl = np.array([0, 1, 4, 5, 9])
    keys, vals = rng.normal(size=(2, 3, H)), rng.randint(0, 6, size=(2, 3))
    group = np.array([0, 1, 1, 0, 1])
    for sup in (False, True):
        got = SC.distribution(q, z, sk, sv, sl, W, 1.3, 0.25, keys if sup else None, vals if sup else None, group)
        for i in range(n):
            k, v = SC.union_entries(sk[i], sv[i], sl[i], W, keys[group[i]] if sup else None, vals[group[i]] if sup else None)
            assert len(v) == (3 if sup else 0) + min(sl[i], W)
            if len(v) == 0:
                assert np.all(got['cache_prob'][i] == 0) and np.array_equal(got['logprob'][i], got['lp'][i])     # the empty union
                continue
            assert np.array_equal(k[len(v) - min(sl[i], W):], sk[i, sl[i] - min(sl[i], W):sl[i]])               # the LAST entries
            want = CG.distribution(k[None], v[None], q[i:i + 1], z[i:i + 1], None, 1.3, 0.25)
            assert np.allclose(got['cache_prob'][i], want['cache_prob'][0], rtol=1e-12, atol=0)
            assert np.allclose(got['logprob'][i], want['logprob'][0], rtol=1e-12, atol=0)
            assert abs(got['cache_prob'][i].sum() - 1) < 1e-12
    assert np.array_equal(SC.distribution(q, z, sk, sv, sl, W, 1.3, 0.0)['logprob'], got['lp'])                # lambda = 0


@pytest.mark.parametrize('name', ['H24', 'H200x2', 'H512'])
def test_near_tie_counts_of_the_gpu_tests_inputs(name):
    """The free-running fp64 decoder with the own-history step over the teacher-forced GPU test's shapes, thetas, picks, window and
    seed, with and without the support entries: its own teacher-forced check passes on its own rows, and at most 5 % of the generated
    positions have an fp64 margin below the tie threshold -- the GPU test's cap of 10 % on skipped positions is one these inputs can
    meet.  With lambda = 1 and no support entries every token after position 0 is one the row already holds."""
    case = SC.oracle_case(name)
    params, cfg, primer = case['params'], case['cfg'], case['primer']
    for sup in (False, True):
        kw = dict(keys=case['keys'], vals=case['vals'], group=SC.GROUP) if sup else {}
        for theta in case['thetas'][:2]:
            for temperature, top_k in SC.GEN_PICKS:
                out = SC.generate(params, cfg, SC.GEN_W, theta, SC.GAIN_LAMBDA, 5, SC.GEN_NUM, temperature=temperature, top_k=top_k,
                                  seed=SC.GEN_SEED, primer=primer, **kw)
                near = int((out['margin'] < 2 * out['tol']).sum())
                res = SC.check_margins(params, cfg, SC.GEN_W, theta, SC.GAIN_LAMBDA, out['toks'], out['lps'], temperature, top_k,
                                       SC.GEN_SEED, primer=primer, **kw)
                print('%s support %d theta %.4g T %.1f top_k %d: %d of %d positions near-ties (tolerance %.3g .. %.3g)'
                      % (name, sup, theta, temperature, top_k, near, out['margin'].size, out['tol'].min(), out['tol'].max()))
                assert res['near'] == near and res['total'] == 5 * SC.GEN_NUM and near <= 0.05 * res['total']
    out = SC.generate(params, cfg, SC.GEN_W, case['thetas'][1], 1.0, 5, SC.GEN_NUM, seed=SC.GEN_SEED, primer=primer)
    for b in range(5):
        row = list(primer[b]) + list(out['toks'][b])
        assert all(row[i] in row[:i] for i in range(len(primer[b]), len(row)))
