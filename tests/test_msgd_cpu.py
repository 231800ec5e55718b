"""Meta-SGD on the CPU (no GPU needed): the fp64 restatement tests/msgd_ref.py against independent torch autograd, the exact gradient at
one inner step, the plugin's settings / checkpoint helpers, the data-parallel exchange of the rates' gradient over gloo, and the
planted mistakes -- each shown to move a quantity tests/test_gpu_msgd.py asserts by more than twice that quantity's bound there.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import maml_ref as MR
import msgd_ref as SR
from conftest import ROOT, free_port
from fake_model import FakeModel
from oracle import lstm_oracle as O
from oracle.torch_ref import TorchRef
from test_dist_gloo import CFG, K, N, OracleEngine, Q

LR = MR.INNER_LR
_F64 = torch.float64


# ----------------------------------------------------------------------------- the restatement against torch autograd
def torch_pass(cfg, theta, A, sup, qry, n, lr, mode, detach):
    """theta' = theta - sum_i lr c_i A o g_i and dL_query(theta') / dA by autograd; detach: g_i and c_i are constants (the first-order
    form the library computes) -- otherwise nothing is"""
    ref = TorchRef(cfg, theta, dtype=_F64, clip_norm_mode=mode)
    names = ref.names
    A_t = {k: torch.tensor(np.asarray(A[k]), dtype=_F64, requires_grad=True) for k in names}
    fast = {k: ref.p[k].detach().clone().requires_grad_(True) for k in names}
    Xs, Ys = O.tokens_to_input_and_target(sup, ref.d['start'])
    Xq, Yq = O.tokens_to_input_and_target(qry, ref.d['start'])
    clip = float(cfg['max_grad_norm'])
    for _ in range(n):
        ref.p = {k: v.detach().requires_grad_(True) for k, v in fast.items()} if detach else fast
        rows = ref.p['embedding'][torch.as_tensor(np.asarray(Xs), dtype=torch.long)]
        loss = ref._nll(Xs, Ys, emb_rows=rows)
        gs = torch.autograd.grad(loss, [ref.p[k] for k in names] + [rows], create_graph=not detach)
        g = dict(zip(names, gs[:-1]))
        sq = sum((gs[-1] ** 2).sum() if (k == 'embedding' and mode == 'tf1_slices') else (g[k] ** 2).sum() for k in names)
        c = clip / torch.clamp(torch.sqrt(sq), min=clip)
        if detach:
            g, c = {k: v.detach() for k, v in g.items()}, c.detach()
        fast = {k: fast[k] - lr * c * A_t[k] * g[k] for k in names}
    ref.p = fast
    loss_q = ref._nll(Xq, Yq)
    loss_q.backward()
    return float(loss_q.detach()), {k: v.detach().numpy() for k, v in fast.items()}, {k: A_t[k].grad.numpy() for k in names}


def setup(idx):
    shape = MR.MAML_SHAPES[idx]
    cfg = MR.config_of(shape)
    sup, qry = MR.episode(cfg, shape)
    return shape, cfg, sup, qry, MR.f64(MR.initial_theta(cfg)), MR.f64(SR.draw_rates(cfg))


def close(a, b, tol=1e-9):
    return float(np.abs(a - b).max()) <= tol * max(float(np.abs(b).max()), 1e-300)


@pytest.mark.parametrize('idx,mode', [(1, 'tf1_slices'), (1, 'dense'), (0, 'tf1_slices')], ids=str)
def test_restatement_matches_torch_autograd(idx, mode):
    shape, cfg, sup, qry, theta, A = setup(idx)
    n = shape[4]
    fb = SR.forward_backward(theta, A, sup, qry, cfg, n, LR, mode)
    loss, theta_p, dA = torch_pass(cfg, theta, A, sup, qry, n, LR, mode, detach=True)
    assert abs(fb['loss'] - loss) <= 1e-9 * abs(loss)
    for k in theta:
        assert close(fb['theta_prime'][k], theta_p[k]), ('theta-prime', k)
        assert close(fb['GA'][k], dA[k]), ('GA', k)
        assert np.abs(fb['GA'][k]).max() > 0, k
    assert all(s['gnorm'] > cfg['max_grad_norm'] for s in fb['steps'])          # the clip is active
    # uniform rates of one are the MAML-style oracle's adaptation
    ones = {k: np.ones_like(v) for k, v in A.items()}
    want, _ = O.maml_adapt(theta, sup, cfg, n, LR, clip_norm_mode=mode)
    got, _, _ = SR.adapt(theta, ones, sup, cfg, n, LR, mode)
    for k in want:
        assert close(got[k], want[k], 1e-12), k


def test_one_inner_step_gives_the_exact_gradient():
    shape, cfg, sup, qry, theta, A = setup(0)
    assert shape[4] == 1
    fb = SR.forward_backward(theta, A, sup, qry, cfg, 1, LR)
    _, _, dA = torch_pass(cfg, theta, A, sup, qry, 1, LR, 'tf1_slices', detach=False)       # nothing detached
    for k in A:
        assert close(fb['GA'][k], dA[k]), k
    rng = np.random.RandomState(2)
    h = 1e-4
    for k in ('softmax_b', 'bias_0', 'softmax_w', 'kernel_0'):
        live = np.flatnonzero(np.abs(fb['GA'][k].ravel()) > 0.1 * np.abs(fb['GA'][k]).max())
        for j in rng.choice(live, size=2, replace=False):
            vals = []
            for sgn in (1.0, -1.0):
                Ap = {n: v.copy() for n, v in A.items()}
                Ap[k].ravel()[j] += sgn * h
                vals.append(SR.msgd_eval(theta, Ap, sup, qry, cfg, 1, LR))
            fd = (vals[0] - vals[1]) / (2 * h)
            got = fb['GA'][k].ravel()[j]
            assert abs(fd - got) <= 1e-5 * abs(got) + 1e-12, (k, j, fd, got)


def test_outer_update_of_the_rates():
    """alpha_lr == 0 moves nothing; otherwise one Adam step from zero slots is sign-like with theta's schedule at alpha_lr; the clamp
    comes last"""
    shape, cfg, sup, qry, theta, A = setup(0)
    fb = SR.forward_backward(theta, A, sup, qry, cfg, 1, LR)
    A0, st = {k: v.copy() for k, v in A.items()}, SR.new_rate_state(A)
    SR.alpha_update(A0, st, fb['GA'], 0, cfg, SR.msgd_config(alpha_lr=0.0))
    assert all(np.array_equal(A0[k], A[k]) for k in A) and all(np.all(v == 0) for v in st['m'].values())
    mcfg = SR.msgd_config(alpha_lr=0.05, alpha_min=0.3, alpha_max=1.7)
    SR.alpha_update(A0, st, fb['GA'], 0, cfg, mcfg)
    # from zero slots: m = (1 - b1) g, v = (1 - b2) g^2, so delta = alpha_lr g / (|g| + eps / sqrt(1 - b2)) at step 0
    g = fb['GA']['softmax_b']
    inside = (A['softmax_b'] > 0.4) & (A['softmax_b'] < 1.6)
    want = 0.05 * g / (np.abs(g) + O.ADAM_EPS / np.sqrt(1.0 - O.BETA2))
    assert inside.sum() > 10 and np.allclose((A['softmax_b'] - A0['softmax_b'])[inside], want[inside], rtol=1e-9, atol=0)
    assert np.abs(want[inside]).min() > 0.04                        # sign-like
    assert all(v.min() >= 0.3 and v.max() <= 1.7 for v in A0.values())
    assert any((v == 0.3).any() for v in A0.values()) and any((v == 1.7).any() for v in A0.values())


# ----------------------------------------------------------------------------- the plugin's settings and checkpoint helpers
def test_settings_reach_the_struct_and_refusals():
    import yaml
    from fsmg.binding import FsmgModel, FsmgMsgdConfig
    from models.metasgd_lstm import DEFAULTS, msgd_settings
    shipped = yaml.safe_load(open(os.path.join(ROOT, 'few-shot-music-generation_amd', 'src', 'config', 'metasgd_lstm.yaml')))
    assert shipped['model_module_name'] == 'models.metasgd_lstm' and shipped['model_class_name'] == 'MetaSGDLSTM'
    s = msgd_settings(shipped)
    assert s == dict(alpha_init=1.0, alpha_lr=1e-3, alpha_min=0.0, alpha_max=10.0, alpha_clip_norm=0.0)
    assert msgd_settings({}) == {k: float(v) for k, v in DEFAULTS.items()} and DEFAULTS['alpha_init'] == 1.0
    c = FsmgModel.msgd_config(**msgd_settings(dict(alpha_init=0.5, alpha_lr=0.02, alpha_min=0.1, alpha_max=3.0, alpha_clip_norm=2.0)))
    assert isinstance(c, FsmgMsgdConfig) and c.struct_size == 28 and c.reserved == 0
    assert [c.alpha_init, c.alpha_lr, c.alpha_min, c.alpha_max, c.alpha_clip_norm] == [np.float32(v) for v in (0.5, 0.02, 0.1, 3.0, 2.0)]
    nan, inf = float('nan'), float('inf')
    for bad in (dict(alpha_lr=-1.0), dict(alpha_lr=inf), dict(alpha_clip_norm=-0.5), dict(alpha_clip_norm=inf), dict(alpha_min=2.0, alpha_max=1.0),
                dict(alpha_init=nan), dict(alpha_lr=nan), dict(alpha_min=nan), dict(alpha_max=nan), dict(alpha_clip_norm=nan), dict(alpha_init=inf)):
        with pytest.raises(RuntimeError):
            msgd_settings(bad)


class FakeRatesEngine(object):
    """the members of FsmgModel that models.metasgd_lstm.save_rates / load_rates use"""
    def __init__(self, shapes, seed):
        rng = np.random.RandomState(seed)
        self.param_shapes = {k: (s if len(s) == 2 else (s[0], 1)) for k, s in shapes.items()}
        self._shapes = dict(shapes)
        self.alpha = {k: rng.uniform(0.2, 2.0, s).astype(np.float32) for k, s in shapes.items()}
        self.m = {k: rng.normal(size=s).astype(np.float32) for k, s in shapes.items()}
        self.v = {k: rng.uniform(0, 1, s).astype(np.float32) for k, s in shapes.items()}

    def _shape(self, name):
        return self._shapes[name]

    def msgd_get_alpha(self, name):
        return self.alpha[name].copy()

    def msgd_set_alpha(self, name, value):
        self.alpha[name] = np.array(value, np.float32)

    def msgd_get_opt_state(self, name):
        return self.m[name].copy(), self.v[name].copy()

    def msgd_set_opt_state(self, name, m, v):
        self.m[name], self.v[name] = np.array(m, np.float32), np.array(v, np.float32)


class FakeRatesModel(FakeModel):
    """tests/fake_model.py's plugin with the rates saved beside its checkpoint the way MetaSGDLSTM does it"""
    SHAPES = {'embedding': (7, 3), 'kernel_0': (5, 8), 'bias_0': (8,), 'softmax_w': (2, 7), 'softmax_b': (7,)}

    def __init__(self, config, seed):
        super(FakeRatesModel, self).__init__(config)
        self.engine = FakeRatesEngine(self.SHAPES, seed)

    def _path(self, d):
        return os.path.join(d, self.name + '.metasgd.npz')

    def save(self, checkpt_path):
        from models.metasgd_lstm import save_rates
        super(FakeRatesModel, self).save(checkpt_path)
        save_rates(self.engine, self._path(checkpt_path))

    def recover_or_init(self, init_path):
        from models.metasgd_lstm import load_rates
        super(FakeRatesModel, self).recover_or_init(init_path)
        return bool(init_path) and load_rates(self.engine, self._path(init_path))


def test_checkpoint_round_trip(tmp_path):
    a = FakeRatesModel(dict(name='fake', input_size=7), seed=1)
    b = FakeRatesModel(dict(name='fake', input_size=7), seed=2)
    assert b.recover_or_init(str(tmp_path)) is False                # nothing there: nothing set
    a.save(str(tmp_path))
    assert ('save', str(tmp_path)) in FakeModel.calls
    assert b.recover_or_init(str(tmp_path)) is True
    for k in a.engine.alpha:
        for x, y in ((a.engine.alpha, b.engine.alpha), (a.engine.m, b.engine.m), (a.engine.v, b.engine.v)):
            assert np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)), k
    # a file of another model (a shape differs) sets nothing
    c = FakeRatesModel(dict(name='fake', input_size=7), seed=3)
    c.engine._shapes['bias_0'] = (9,)
    before = {k: v.copy() for k, v in c.engine.alpha.items()}
    assert c.recover_or_init(str(tmp_path)) is False
    assert all(np.array_equal(before[k], c.engine.alpha[k]) for k in before)


# ----------------------------------------------------------------------------- world 2 over gloo
G_LR, G_STEPS = 0.3, 1


class RatesEngine(OracleEngine):
    """tests/test_dist_gloo.py's CPU engine with the Meta-SGD members: maml_forward_backward leaves the query gradient in grad_tensor and
    THIS rank's GA in rate_grad_tensor; apply_update(1 / world) moves theta and the rates"""
    def __init__(self, cfg, params, A, mcfg):
        super(RatesEngine, self).__init__(cfg, params)
        self.A, self.state, self.mcfg = {k: v.copy() for k, v in A.items()}, SR.new_rate_state(A), mcfg
        self.rate_grad_tensor = torch.zeros(sum(self.sizes), dtype=torch.float64)
        self.local = None

    def maml_forward_backward(self, support, query, inner_steps, inner_lr, **kw):
        fb = SR.forward_backward(self.params, self.A, support, query, self.cfg, inner_steps, inner_lr)
        flat = np.concatenate([fb['G'][n].ravel() for n in self.names] + [np.zeros(self.TAIL)])
        flat[-self.TAIL] = fb['aux']['embedding_slices_sq']
        flat[-self.TAIL + 1] = fb['loss']
        self.grad_tensor.copy_(torch.from_numpy(flat))
        self.rate_grad_tensor.copy_(torch.from_numpy(np.concatenate([fb['GA'][n].ravel() for n in self.names])))
        self.local = fb

    def apply_update(self, grad_scale=1.0, want_loss=True):
        step = self.opt['step']
        loss = super(RatesEngine, self).apply_update(grad_scale, want_loss)
        flat, GA, off = self.rate_grad_tensor.numpy() * 1.0, {}, 0
        for n, sz in zip(self.names, self.sizes):
            GA[n] = flat[off:off + sz].reshape(self.params[n].shape)
            off += sz
        self.reduced = {k: v.copy() for k, v in GA.items()}
        SR.alpha_update(self.A, self.state, GA, step, self.cfg, self.mcfg, grad_scale)
        return loss


def _gloo_case():
    theta = O.glorot_init(CFG, 5, np.float64)
    A = MR.f64(SR.draw_rates(CFG))
    eps = O.synthetic_episodes(2, N, K, Q, CFG['max_len'], CFG['input_size'], seed=3)
    return theta, A, eps, SR.msgd_config()


def _rates_worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.join(ROOT, 'few-shot-music-generation_amd', 'src'))
    from fsmg.dist import EpisodeParallel
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    theta, A, eps, mcfg = _gloo_case()
    eng = RatesEngine(CFG, theta, A, mcfg)
    par = EpisodeParallel(eng)
    loss = par.train_step(*eps[rank], maml=(1, G_LR))
    blob = {'A/' + k: v for k, v in eng.A.items()}
    blob.update({'GA/' + k: v for k, v in eng.reduced.items()})
    blob.update({'p/' + k: v for k, v in eng.params.items()})
    np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), loss=loss, **blob)
    dist.destroy_process_group()


def test_two_ranks_reduce_the_rate_gradient_formed_per_rank(tmp_path):
    mp.spawn(_rates_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (np.load(os.path.join(str(tmp_path), 'rank%d.npz' % r)) for r in (0, 1))
    theta, A, eps, mcfg = _gloo_case()
    passes = [SR.forward_backward(theta, A, eps[r][0], eps[r][1], CFG, 1, G_LR) for r in (0, 1)]
    want = SR.reduce_ranks(passes)                                  # the sum of the per-rank products
    wrong = SR.reduce_ranks(passes, wrong='ga_after_reduce')        # what the product of the reduced factors would have given
    A_want, st = {k: v.copy() for k, v in A.items()}, SR.new_rate_state(A)
    SR.alpha_update(A_want, st, want, 0, CFG, mcfg, 0.5)
    for k in A:
        assert np.array_equal(r0['A/' + k], r1['A/' + k]) and np.array_equal(r0['p/' + k], r1['p/' + k]), k      # replicas stay identical
        np.testing.assert_allclose(r0['GA/' + k], want[k], rtol=1e-12, atol=1e-300, err_msg=k)
        np.testing.assert_allclose(r0['A/' + k], A_want[k], rtol=1e-12, err_msg=k)
        assert np.any(r0['A/' + k] != A[k]), k
    # mean of products against product of means, on these inputs: far apart
    k = 'softmax_b'
    assert np.abs(want[k] - wrong[k]).max() > 0.05 * np.abs(want[k]).max()
    assert r0['loss'] == r1['loss'] and abs(float(r0['loss']) - 0.5 * (passes[0]['loss'] + passes[1]['loss'])) < 1e-12


def test_one_rank_exchanges_nothing():
    sys.path.insert(0, os.path.join(ROOT, 'few-shot-music-generation_amd', 'src'))
    from fsmg.dist import EpisodeParallel
    theta, A, eps, mcfg = _gloo_case()
    eng = RatesEngine(CFG, theta, A, mcfg)
    loss = EpisodeParallel(eng).train_step(*eps[0], maml=(1, G_LR))
    params, opt, A1, st = MR.f64(theta), O.new_opt_state(MR.f64(theta)), {k: v.copy() for k, v in A.items()}, SR.new_rate_state(A)
    want, _ = SR.msgd_step(params, opt, A1, st, eps[0][0], eps[0][1], CFG, mcfg, 1, G_LR)
    assert abs(loss - want) < 1e-12
    for k in A:
        np.testing.assert_allclose(eng.A[k], A1[k], rtol=1e-12, err_msg=k)
        np.testing.assert_allclose(eng.params[k], params[k], rtol=1e-12, atol=1e-300, err_msg=k)


# ----------------------------------------------------------------------------- planted mistakes
_RIGHT = {}


def right(idx):
    """the right passes of a shape in fp64, computed once: rank 0 (the shape's episode) and rank 1 (the next seed)"""
    if idx not in _RIGHT:
        shape, cfg, sup, qry, theta, A = setup(idx)
        over, N_, K_, Q_, n, seed = shape
        sup1, qry1 = MR.episode(cfg, (over, N_, K_, Q_, n, seed + 1))
        _RIGHT[idx] = (shape, cfg, theta, A, (sup, qry), (sup1, qry1),
                       SR.forward_backward(theta, A, sup, qry, cfg, n, LR), SR.forward_backward(theta, A, sup1, qry1, cfg, n, LR))
    return _RIGHT[idx]


def worst(diff, tol):
    return max(float((np.abs(diff[k]) / tol[k]).max()) for k in diff)


def steps_of(fb, cfg):
    return [(MR.sgd_step(s['gnorm'], cfg['max_grad_norm'], LR), s['grads']) for s in fb['steps']]


def after_update(A, GA, cfg, mcfg, wrong=None):
    """A after one update from zero slots, and the GPU test's bound on it (64 u |delta| + 2 u |raw|: msgd_ref.alpha_check)"""
    A1, st = {k: v.copy() for k, v in A.items()}, SR.new_rate_state(A)
    SR.alpha_update(A1, st, GA, 0, cfg, mcfg, 1.0, wrong)
    _, _, size = SR.alpha_scalars(GA, 0, cfg, mcfg)
    tol = {}
    for k in A:
        delta = size * st['m'][k] / (np.sqrt(st['v'][k]) + O.ADAM_EPS)
        tol[k] = 64 * SR.U * np.abs(delta) + 2 * SR.U * np.abs(A[k] - delta) + SR.UNDERFLOW
    return A1, tol


@pytest.mark.parametrize('idx', range(len(MR.MAML_SHAPES)))
def test_every_planted_mistake_is_outside_twice_the_gpu_bound(idx):
    shape, cfg, theta, A, ep0, ep1, fb, fb1 = right(idx)
    n = shape[4]
    _, S_tol = SR.sum_reference(steps_of(fb, cfg))
    GA_tol = {k: SR.U * np.abs(v) + SR.UNDERFLOW for k, v in fb['GA'].items()}
    seen = {}
    # 1, 3, 4: what S collects
    for w in ('sum_g', 'sum_st_g') + (('sum_last_only',) if n > 1 else ()):
        _, _, S = SR.adapt(theta, A, ep0[0], cfg, n, LR, wrong=w)
        seen[w] = worst({k: S[k] - fb['S'][k] for k in S}, S_tol)
    # 2: S of the adaptation before is still there
    _, _, S = SR.adapt(theta, A, ep0[0], cfg, n, LR, S0=fb1['S'], wrong='sum_not_zeroed')
    seen['sum_not_zeroed'] = worst({k: S[k] - fb['S'][k] for k in S}, S_tol)
    # 5, 6: GA
    last = fb['steps'][-1]['grads']
    for w in ('ga_sign', 'ga_last_support'):
        GA = SR.rate_gradient(fb['G'], fb['S'], w, last)
        seen[w] = worst({k: GA[k] - fb['GA'][k] for k in GA}, GA_tol)
    # 7: theta' (the bound of msgd_ref.theta_check on the last step)
    tw, _, _ = SR.adapt(theta, A, ep0[0], cfg, n, LR, wrong='rate_additive')
    s = fb['steps'][-1]
    step = MR.sgd_step(s['gnorm'], cfg['max_grad_norm'], LR)
    t_tol = {k: 2 * SR.U * np.abs(fb['theta_prime'][k]) + 8 * SR.U * np.abs(step * A[k] * s['grads'][k]) + SR.UNDERFLOW for k in A}
    seen['rate_additive'] = worst({k: tw[k] - fb['theta_prime'][k] for k in tw}, t_tol)
    # 8, 9: A after the update (8 where both clamp ends bind: tests/test_gpu_msgd.py E2's third case)
    for w, mcfg in (('clamp_before_adam', SR.msgd_config(alpha_min=0.9, alpha_max=1.1)), ('alpha_uses_lr', SR.msgd_config())):
        good, a_tol = after_update(A, fb['GA'], cfg, mcfg)
        bad, _ = after_update(A, fb['GA'], cfg, mcfg, w)
        seen[w] = worst({k: bad[k] - good[k] for k in good}, a_tol)
    # 10: two ranks -- the reduced GA, in the bound of one rank's GA summed over the ranks
    want, got = SR.reduce_ranks([fb, fb1]), SR.reduce_ranks([fb, fb1], wrong='ga_after_reduce')
    r_tol = {k: SR.U * (np.abs(fb['GA'][k]) + np.abs(fb1['GA'][k])) + SR.UNDERFLOW for k in want}
    seen['ga_after_reduce'] = worst({k: got[k] - want[k] for k in want}, r_tol)
    print('PLANTED|%s|%s' % (MR.shape_id(shape), ' '.join('%s %.3g' % kv for kv in sorted(seen.items()))))
    assert set(seen) == set(SR.WRONG) - (set() if n > 1 else {'sum_last_only'})
    for w, ratio in seen.items():
        assert ratio > 2, (w, ratio)
