"""Meta-SGD (include/fsmg.h "Meta-SGD") restated in numpy, and the derived bounds (TEST INFRASTRUCTURE ONLY).

  * adapt / rate_gradient / alpha_update / msgd_step / msgd_eval: the semantics in the dtype of the parameters handed in -- fp64 is the
    reference of tests/test_gpu_msgd.py; adapt is maml_ref.adapt_full with the update line of step 1, S beside it;
  * wrong=: the same with ONE planted mistake (WRONG), for tests/test_msgd_cpu.py to show that the GPU test's bounds see it;
  * theta_check / sum_check / ga_tol / alpha_check: the element-wise bounds of the GPU test, derived operation by operation from fp32
    inputs read back from the device, the way maml_ref.sgd_check and dyneval_ref.update_check do it.
"""
import numpy as np

import maml_ref as MR
from oracle import lstm_oracle as O

U = MR.U
F32 = np.float32
UNDERFLOW = 1e-30
A_LO, A_HI = 0.25, 1.75                 # the range the tests draw the rates from

WRONG = ('sum_g', 'sum_not_zeroed', 'sum_last_only', 'sum_st_g', 'ga_sign', 'ga_last_support', 'rate_additive',
         'clamp_before_adam', 'alpha_uses_lr', 'ga_after_reduce')


def msgd_config(**over):
    c = dict(alpha_init=1.0, alpha_lr=0.05, alpha_min=0.0, alpha_max=10.0, alpha_clip_norm=0.0)
    c.update(over)
    return c


def draw_rates(cfg, seed=11, dtype=np.float32):
    """seeded uniform [0.25, 1.75] per element, by parameter name"""
    rng = np.random.RandomState(seed)
    return {k: rng.uniform(A_LO, A_HI, size=shape).astype(dtype) for k, shape in O.param_shapes(cfg)}


def const_rates(cfg, value, dtype=np.float32):
    return {k: np.full(shape, value, dtype) for k, shape in O.param_shapes(cfg)}


# ----------------------------------------------------------------------------- step 1 and 2
def adapt(params, A, support, config, inner_steps, inner_lr, mode='tf1_slices', S0=None, wrong=None):
    """-> (theta', steps of maml_ref.adapt_full, S).  S0: what S holds when the adaptation begins (zeros unless wrong == 'sum_not_zeroed')"""
    dt = next(iter(params.values())).dtype.type
    S = {k: np.zeros_like(v) for k, v in params.items()}
    if wrong == 'sum_not_zeroed' and S0 is not None:
        S = {k: v.copy() for k, v in S0.items()}
    clip = float(config['max_grad_norm'])

    def update(fast, grads, aux):
        gnorm = O.global_norm(grads, aux, mode)
        step = dt(dt(clip / max(gnorm, clip)) * dt(inner_lr))
        new = {}
        for k in fast:
            a = np.asarray(A[k], fast[k].dtype)
            st = (dt(clip / max(gnorm, clip)) * (dt(inner_lr) + a)) if wrong == 'rate_additive' else step * a
            new[k] = fast[k] - st * grads[k]
            if wrong == 'sum_g':
                S[k] = S[k] + grads[k]
            elif wrong == 'sum_last_only':
                S[k] = step * grads[k]
            elif wrong == 'sum_st_g':
                S[k] = S[k] + st * grads[k]
            else:
                S[k] = S[k] + step * grads[k]
        return new, gnorm

    theta, steps = MR.adapt_full(params, support, config, inner_steps, inner_lr, mode, update=update)
    return theta, steps, S


def query_pass(theta, query, config):
    X, Y = O.tokens_to_input_and_target(query, O.model_dims(config)['start'])
    loss, cache = O.forward(theta, X, Y, config)
    grads, aux = O.backward(theta, cache, config)
    return float(loss), grads, aux


def rate_gradient(G, S, wrong=None, last_support=None):
    if wrong == 'ga_last_support':
        G = last_support
    sign = 1.0 if wrong == 'ga_sign' else -1.0
    return {k: sign * (G[k] * S[k]) for k in G}


def forward_backward(params, A, support, query, config, inner_steps, inner_lr, mode='tf1_slices', S0=None, wrong=None):
    """the train form up to the pending gradients -> dict(theta_prime, steps, S, loss, G, aux, GA)"""
    theta, steps, S = adapt(params, A, support, config, inner_steps, inner_lr, mode, S0, wrong)
    loss, G, aux = query_pass(theta, query, config)
    GA = rate_gradient(G, S, wrong, steps[-1]['grads'] if steps else {k: np.zeros_like(v) for k, v in G.items()})
    return dict(theta_prime=theta, steps=steps, S=S, loss=loss, G=G, aux=aux, GA=GA)


# ----------------------------------------------------------------------------- step 3
def new_rate_state(A):
    return dict(m={k: np.zeros_like(v) for k, v in A.items()}, v={k: np.zeros_like(v) for k, v in A.items()})


def alpha_scalars(GA, step, config, mcfg, grad_scale=1.0, wrong=None):
    """(gnorm_a, scale, step size) as the rates' update derives them: the plain global norm of GA, theta's schedule with alpha_lr"""
    gnorm = float(np.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in GA.values()))) * grad_scale
    clip = float(mcfg['alpha_clip_norm'])
    scale = clip / max(gnorm, clip) * grad_scale if clip > 0 else grad_scale
    lr = float(config['lr']) if wrong == 'alpha_uses_lr' else float(mcfg['alpha_lr'])
    t = step + 1
    size = lr * 0.5 ** (step / float(config['n_decay'])) * np.sqrt(1.0 - O.BETA2 ** t) / (1.0 - O.BETA1 ** t)
    return gnorm, scale, size


def alpha_update(A, state, GA, step, config, mcfg, grad_scale=1.0, wrong=None):
    """clip + Adam (oracle.lstm_oracle.apply_update's element lines) + clamp of the rates; mutates A and state.  alpha_lr == 0: nothing"""
    if float(mcfg['alpha_lr']) == 0.0:
        return
    _, scale, size = alpha_scalars(GA, step, config, mcfg, grad_scale, wrong)
    lo, hi = float(mcfg['alpha_min']), float(mcfg['alpha_max'])
    for k in A:
        dt = A[k].dtype.type
        a = np.clip(A[k], dt(lo), dt(hi)) if wrong == 'clamp_before_adam' else A[k]
        g = GA[k] * dt(scale)
        state['m'][k] = dt(O.BETA1) * state['m'][k] + dt(1.0 - O.BETA1) * g
        state['v'][k] = dt(O.BETA2) * state['v'][k] + dt(1.0 - O.BETA2) * g * g
        a = a - dt(size) * state['m'][k] / (np.sqrt(state['v'][k]) + dt(O.ADAM_EPS))
        A[k] = a if wrong == 'clamp_before_adam' else np.clip(a, dt(lo), dt(hi))


def msgd_step(params, opt, A, state, support, query, config, mcfg, inner_steps, inner_lr, mode='tf1_slices', wrong=None):
    """one outer step on one rank: mutates params / opt / A / state -> (query loss at theta', the pass)"""
    fb = forward_backward(params, A, support, query, config, inner_steps, inner_lr, mode, wrong=wrong)
    step = opt['step']
    O.apply_update(params, fb['G'], fb['aux'], opt, config, mode)          # theta: exactly the MAML-style step's update
    alpha_update(A, state, fb['GA'], step, config, mcfg, 1.0, wrong)
    return fb['loss'], fb


def reduce_ranks(passes, wrong=None):
    """the rates' gradient of R ranks as the wrapper leaves it for apply_update(1 / R): the SUM of the per-rank products
    ('ga_after_reduce': the product of the summed factors, scaled so that 1 / R would give the product of the means)"""
    R = len(passes)
    if wrong == 'ga_after_reduce':
        return {k: -(sum(p['G'][k] for p in passes) * sum(p['S'][k] for p in passes)) / R for k in passes[0]['G']}
    return {k: sum(p['GA'][k] for p in passes) for k in passes[0]['GA']}


def msgd_eval(params, A, support, query, config, inner_steps, inner_lr, mode='tf1_slices'):
    theta, _, _ = adapt(params, A, support, config, inner_steps, inner_lr, mode)
    return O.eval_step(theta, query, config)


# ----------------------------------------------------------------------------- the GPU test's element-wise bounds
def theta_check(label, theta_prev, A, grads, tail, mode, clip, lr, got_theta, got_gnorm, verbose=True):
    """theta'_i against k_msgd_update redone in fp64 from fp32 (theta'_{i-1}, A, gradients, tail) read from the device:
        st = fl(step * A), p_ref = p - st * g in fp64;   |got - p_ref| <= 2 u |p_ref| + 8 u |st * g| + 1e-30
    maml_ref.sgd_check's bound with st for step: the rounding of step * A is redone exactly here, so the allowances are the same -- one
    rounding of the product (none when it is contracted), one of the subtraction, a step known to three roundings.  g == 0: the bits
    of theta'_{i-1}.  -> (gnorm, step, failures)"""
    gnorm = MR.device_gnorm(grads, tail, mode)
    failures = []
    if not abs(float(got_gnorm) - gnorm) <= 2 * U * gnorm:
        failures.append('gnorm %.9g, from the gradients %.9g' % (float(got_gnorm), gnorm))
    step = MR.sgd_step(gnorm, clip, lr)
    for k in sorted(grads):
        p0, g, got, a = (np.asarray(x) for x in (theta_prev[k], grads[k], got_theta[k], A[k]))
        assert p0.dtype == g.dtype == got.dtype == a.dtype == F32, k
        st = (F32(step) * a).astype(np.float64)
        sg = np.abs(st * g.astype(np.float64))
        p_ref = p0.astype(np.float64) - st * g.astype(np.float64)
        tol = 2 * U * np.abs(p_ref) + 8 * U * sg + UNDERFLOW
        frac = np.abs(got.astype(np.float64) - p_ref) / tol
        still = (g == 0) & (got.view(np.uint32) != p0.view(np.uint32))
        if verbose:
            print('MSGD|theta|%s|%s|%.3f' % (label, k, frac.max()))
        if not np.all(np.isfinite(got)) or (frac > 1).any():
            failures.append('theta %s: %d of %d outside the bound (worst %.1f x)' % (k, int((frac > 1).sum()), frac.size, frac.max()))
        if still.any():
            failures.append('theta %s: %d elements without a gradient moved' % (k, int(still.sum())))
    return gnorm, step, failures


def sum_reference(step_grads):
    """step_grads: [(fp32 step, {name: fp32 gradient})] per inner step -> (S_ref fp64, tol):
        S_i = fl(S_{i-1} + step_i g_i), one rounding (an fma): u |S_i|; step_i known to three roundings: 4 u |step_i g_i| -- summed over i"""
    ref, tol = None, None
    for step, grads in step_grads:
        if ref is None:
            ref = {k: np.zeros(g.shape, np.float64) for k, g in grads.items()}
            tol = {k: np.full(g.shape, UNDERFLOW) for k, g in grads.items()}
        for k, g in grads.items():
            sg = float(step) * g.astype(np.float64)
            ref[k] = ref[k] + sg
            tol[k] = tol[k] + U * np.abs(ref[k]) + 4 * U * np.abs(sg)
    return ref, tol


def ga_reference(G, S):
    """GA from the device's own fp32 G and S: one rounding of the product -> (ref fp64, tol = u |ref| + 1e-30)"""
    ref = {k: -(G[k].astype(np.float64) * S[k].astype(np.float64)) for k in G}
    return ref, {k: U * np.abs(v) + UNDERFLOW for k, v in ref.items()}


def alpha_reference(A0, m0, v0, GA, scale, size, lo, hi):
    """the rates' update in fp64 on fp32 inputs with the kernel's fp32 scalars: tests/test_gpu_componentwise.py's adam_reference, the
    parameter line from given (device) m1 / v1 is the caller's; here -> (m_ref, v_ref, m_scale)"""
    b1, b2 = float(F32(0.9)), float(F32(0.999))
    c1, c2 = float(F32(1.0) - F32(0.9)), float(F32(1.0) - F32(0.999))
    g, m, v = (np.asarray(a, np.float64) for a in (GA, m0, v0))
    gc = g * scale
    return b1 * m + c1 * gc, b2 * v + c2 * gc * gc, np.abs(b1 * m) + np.abs(c1 * gc)


def alpha_check(label, A0, slots0, GA, A1, slots1, scale, size, lo, hi, verbose=True):
    """A, AM, AV after the update against the fp64 redo from the DEVICE's own GA, by the bounds of tests/test_gpu_componentwise.py
    (m: 16 u of |b1 m| + |(1 - b1) g scale|; v: 32 u; the rate: 64 u |delta| + 2 u |p|, delta from the device's own new slots), the
    clamp applied to the reference (it is monotone and 1-Lipschitz: the bound carries over; an element the reference puts outside
    [lo, hi] by more than its bound must sit exactly on the end) -> failures"""
    failures = []
    scale, size = float(F32(scale)), float(F32(size))
    for k in sorted(GA):
        (m0, v0), (m1, v1) = slots0[k], slots1[k]
        m_ref, v_ref, m_scale = alpha_reference(A0[k], m0, v0, GA[k], scale, size, lo, hi)
        m_err, v_err = np.abs(m1 - m_ref), np.abs(v1 - v_ref)
        delta = size * m1.astype(np.float64) / (np.sqrt(v1.astype(np.float64)) + float(F32(1e-8)))
        raw = A0[k].astype(np.float64) - delta
        tol = np.abs(delta) * 64 * U + np.abs(raw) * 2 * U + UNDERFLOW
        ref = np.clip(raw, lo, hi)
        err = np.abs(A1[k].astype(np.float64) - ref)
        if verbose:
            print('MSGD|alpha|%s|%s|m %.2f u|v %.2f u|A %.3f of its bound|%d at lo, %d at hi' % (
                label, k, (m_err / np.maximum(m_scale, 1e-300)).max() / U, (v_err / np.maximum(v_ref, 1e-300)).max() / U,
                (err / tol).max(), int((A1[k] == F32(lo)).sum()), int((A1[k] == F32(hi)).sum())))
        if not np.all(m_err <= 16 * U * m_scale + UNDERFLOW):
            failures.append('AM %s' % k)
        if not np.all(v_err <= 32 * U * v_ref + UNDERFLOW):
            failures.append('AV %s' % k)
        if not np.all(err <= tol):
            failures.append('A %s: worst %.1f x' % (k, (err / tol).max()))
        if not (np.all(A1[k][raw < lo - tol] == F32(lo)) and np.all(A1[k][raw > hi + tol] == F32(hi))):
            failures.append('A %s: an element beyond the clamp is not on its end' % k)
    return failures
