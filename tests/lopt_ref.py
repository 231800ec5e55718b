"""The learned optimiser (include/fsmg.h "learned optimiser") restated in numpy, and the derived bounds (TEST
INFRASTRUCTURE ONLY).

  * prep / gate / step_element / adapt / backprop / phi_update / lopt_step / lopt_eval / tasks_forward_backward: the semantics in the
    dtype of the parameters handed in.  fp64 is the reference of tests/test_gpu_lopt.py; fp32 is the stand-in of the device (every
    fused multiply-add of the kernels is one rounding here too: the product and the sum are taken in fp64 and rounded once);
  * wrong=: the same with ONE planted mistake (WRONG), for tests/test_lopt_cpu.py to show that the GPU test's bounds see it;
  * step_check / backprop_check: the element-wise bounds of the GPU test, derived operation by operation from fp32 inputs read back
    from the device (or from the stand-in), the way maml_ref.sgd_check and msgd_ref.theta_check do it.

Phi is an array of 14: wF[0:6], bF[6], wI[7:13], bI[13]; the gate inputs are x = (a1, a2, c1, c2, theta, previous gate).
"""
import numpy as np

import maml_ref as MR
from oracle import lstm_oracle as O

U = MR.U
F32 = np.float32
F64 = np.float64
UNDERFLOW = 1e-30
NPHI = 14
EXP_M10 = float(F32(4.5399929762484854e-05))        # the kernels' fp32 constants (lopt_element.h)
EXP_P10 = float(F32(22026.465794806718))

WRONG = ('gates_not_reset', 'carry_dropped', 'theta_term_dropped', 'prep_swapped', 'loss_previous', 'di_sign', 'di_no_gate_scale',
         'gphi_after_reduce', 'artists_weight_one', 'phi_on_skipped_step')


def lopt_config(**over):
    c = dict(bF_init=6.0, bI_init=0.0, gate_scale=2.0, phi_lr=0.05, phi_clip_norm=0.0, max_train_steps=4)
    c.update(over)
    return c


def draw_phi(seed=5, dtype=np.float32):
    """w uniform in [-0.3, 0.3], bF in [1, 3], bI in [-1, 1]: no gate saturates"""
    rng = np.random.RandomState(seed)
    phi = np.empty(NPHI)
    phi[0:6], phi[6] = rng.uniform(-0.3, 0.3, 6), rng.uniform(1, 3)
    phi[7:13], phi[13] = rng.uniform(-0.3, 0.3, 6), rng.uniform(-1, 1)
    return phi.astype(dtype)


def plain_phi(dtype=np.float32):
    """w = 0, bF = 20 (f is exactly 1.0f), bI = 0: with gate_scale 2 the learned step is the plain step"""
    phi = np.zeros(NPHI, dtype)
    phi[6] = 20.0
    return phi


def initial_phi(lcfg, dtype=np.float32):
    phi = np.zeros(NPHI, dtype)
    phi[6], phi[13] = lcfg['bF_init'], lcfg['bI_init']
    return phi


# ----------------------------------------------------------------------------- the element
def _fma(a, b, c):
    """a * b + c with one rounding in the dtype of the operands (fp64: numpy's own two, 1e-16 apart)"""
    a, b, c = np.asarray(a), np.asarray(b), np.asarray(c)
    if a.dtype == F32 or b.dtype == F32 or c.dtype == F32:
        return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)
    return a * b + c


def prep(x, wrong=None):
    """the paper's preprocessing -> (a1, a2, big): (log|x| / 10, sign x) where |x| >= e^-10, (-1, e^10 x) below"""
    x = np.asarray(x)
    dt = x.dtype.type
    ax = np.abs(x)
    big = ax >= dt(EXP_M10)
    if wrong == 'prep_swapped':
        big = ~big
    lg = np.log(np.maximum(ax, dt(1e-30))) / dt(10)
    a1 = np.where(big, lg, dt(-1))
    a2 = np.where(big, np.sign(x) + (x == 0), dt(EXP_P10) * x)
    return a1.astype(x.dtype), a2.astype(x.dtype), big


def gate(w, b, xs):
    """sigmoid(b + w . xs): fma by fma from the bias, in the order of xs"""
    dt = np.asarray(xs[4]).dtype.type
    z = dt(b)
    for k in range(6):
        z = _fma(dt(w[k]), np.asarray(xs[k], dtype=dt), z)
    with np.errstate(over='ignore'):            # (exp(-z) = inf gives the gate's limit 0, as on the device)
        return (dt(1) / (dt(1) + np.exp(-z))).astype(dt)


def step_element(phi, g, L, theta, F, I, step, gate_scale, wrong=None):
    """one inner step of one tensor -> (f, i, theta_t)"""
    dt = theta.dtype.type
    a1, a2, _ = prep(g, wrong)
    c1, c2, _ = prep(np.asarray(dt(L)), wrong)
    f = gate(phi[0:6], phi[6], (a1, a2, c1, c2, theta, F))
    i = gate(phi[7:13], phi[13], (a1, a2, c1, c2, theta, I))
    q = f * theta
    st = dt(step) * (dt(gate_scale) * i)
    return f, i, _fma(-st, g, q).astype(theta.dtype)


def adapt(params, phi, support, config, inner_steps, inner_lr, gate_scale=2.0, mode='tf1_slices', gates0=None, wrong=None):
    """maml_ref.adapt_full with the learned rule -> (theta', steps); steps[t] = dict(before = theta_{t-1}, Fp, Ip, loss, L (the loss the
    rule saw), grads, aux, gnorm, step, F, I, theta = theta_t).  gates0 = (F, I): what the gate buffers hold when the adaptation
    begins -- used only by wrong == 'gates_not_reset'"""
    d = O.model_dims(config)
    dt = next(iter(params.values())).dtype.type
    fast = {k: v.copy() for k, v in params.items()}
    F = {k: np.ones_like(v) for k, v in params.items()}
    I = {k: np.zeros_like(v) for k, v in params.items()}
    if wrong == 'gates_not_reset' and gates0 is not None:
        F, I = ({k: v.copy() for k, v in x.items()} for x in gates0)
    X, Y = O.tokens_to_input_and_target(support, d['start'])
    clip = float(config['max_grad_norm'])
    steps, prev_loss = [], None
    for _ in range(int(inner_steps)):
        loss, cache = O.forward(fast, X, Y, config)
        grads, aux = O.backward(fast, cache, config)
        gnorm = O.global_norm(grads, aux, mode)
        step = dt(dt(clip / max(gnorm, clip)) * dt(inner_lr))
        L = prev_loss if (wrong == 'loss_previous' and prev_loss is not None) else dt(loss)
        new, nF, nI = {}, {}, {}
        for k in fast:
            nF[k], nI[k], new[k] = step_element(phi.astype(fast[k].dtype), grads[k], L, fast[k], F[k], I[k], step, gate_scale, wrong)
        steps.append(dict(before=fast, Fp=F, Ip=I, loss=float(loss), L=L, grads=grads, aux=aux, gnorm=gnorm, step=step, F=nF, I=nI, theta=new))
        fast, F, I, prev_loss = new, nF, nI, dt(loss)
    return fast, steps


def query_pass(theta, query, config):
    X, Y = O.tokens_to_input_and_target(query, O.model_dims(config)['start'])
    loss, cache = O.forward(theta, X, Y, config)
    grads, aux = O.backward(theta, cache, config)
    return float(loss), grads, aux


# ----------------------------------------------------------------------------- the meta-gradient
def _zero_tol(like):
    return np.zeros(np.shape(like))


def backprop_tensor(phi, steps, G, gate_scale, wrong=None, with_tol=False):
    """The walk back of one tensor.  steps[t] = dict(th, f, i, Fp, Ip, g, step, L): the forward's values of inner step t + 1, in the
    dtype the arithmetic is to run in.  -> (D_0, GPhi sums as fp64 [14]) and, with_tol, the bounds (|D_0 error|, |GPhi error|) of an
    fp32 evaluation with the kernel's operations from exactly these inputs, operation by operation (u = 2^-24):
      dF = fma(D, th, carryF): eD |th| + eCF + u |dF|;   mg = (step gs) g: 2 u;   dI = fma(-D, mg, carryI): eD |mg| + 2 u |D mg| + eCI + u |dI|
      fd = f (1 - f): 2 u;   pf = dF fd: e(dF) fd + 3 u |pf|   (pi alike)
      D <- fma(D, f, fma(pf, wF4, pi wI4)): eD f + e(pf) |wF4| + e(pi) |wI4| + u |pi wI4| + u |through| + u |D|
      carryF = pf wF5: e(pf) |wF5| + u |carryF|   (carryI alike)
      a term pf x of GPhi (the product is exact in fp64): e(pf) |x| + |pf| e(x), e(a1) = e(c1) = 3 u |a1| on the log branch (logf to 1 ulp, the
      division), e(a2) = e(c2) = u |a2| on the linear branch, theta and the previous gates exact; the sums add in fp64 (n 2^-53 of the
      sum of magnitudes) and GPhi is rounded to fp32 once (added by the caller over all tensors)."""
    dt = np.asarray(G).dtype.type
    D = np.asarray(G).copy()
    cF, cI = np.zeros_like(D), np.zeros_like(D)
    eD, eCF, eCI = _zero_tol(D), _zero_tol(D), _zero_tol(D)
    acc, acc_tol = np.zeros(NPHI), np.zeros(NPHI)
    wF, wI = phi[0:6].astype(D.dtype), phi[7:13].astype(D.dtype)
    gs = dt(gate_scale)
    for s in reversed(steps):
        th, f, i, Fp, Ip, g = (np.asarray(s[k], dtype=D.dtype) for k in ('th', 'f', 'i', 'Fp', 'Ip', 'g'))
        a1, a2, gbig = prep(g)
        c1, c2, Lbig = prep(np.asarray(dt(s['L'])))
        dF = _fma(D, th, cF if wrong != 'carry_dropped' else np.zeros_like(cF))
        m = dt(s['step']) * (dt(1) if wrong == 'di_no_gate_scale' else gs)
        mg = m * g
        sign = D if wrong == 'di_sign' else -D
        dI = _fma(sign, mg, cI if wrong != 'carry_dropped' else np.zeros_like(cI))
        fd, idv = f * (dt(1) - f), i * (dt(1) - i)
        pf, pi = dF * fd, dI * idv
        xF = (a1, a2, c1, c2, th, Fp)
        xI = (a1, a2, c1, c2, th, Ip)
        if with_tol:
            a = np.abs
            e_dF = eD * a(th) + eCF + U * a(dF)
            e_dI = eD * a(mg) + 2 * U * a(D * mg) + eCI + U * a(dI)
            e_pf = e_dF * fd + 3 * U * a(pf)
            e_pi = e_dI * idv + 3 * U * a(pi)
            e_x = (np.where(gbig, 3 * U * a(a1), 0.0), np.where(gbig, 0.0, U * a(a2)),
                   float(3 * U * abs(c1)) if Lbig else 0.0, 0.0 if Lbig else float(U * abs(c2)), 0.0, 0.0)
            for k in range(6):
                acc_tol[k] += float((e_pf * a(xF[k]) + a(pf) * e_x[k]).sum())
                acc_tol[7 + k] += float((e_pi * a(xI[k]) + a(pi) * e_x[k]).sum())
            acc_tol[6] += float(e_pf.sum())
            acc_tol[13] += float(e_pi.sum())
        for k in range(6):
            acc[k] += float((pf.astype(F64) * np.asarray(xF[k], F64)).sum())
            acc[7 + k] += float((pi.astype(F64) * np.asarray(xI[k], F64)).sum())
        acc[6] += float(pf.astype(F64).sum())
        acc[13] += float(pi.astype(F64).sum())
        if wrong == 'theta_term_dropped':
            through = np.zeros_like(D)
        else:
            through = _fma(pf, wF[4], pi * wI[4])
        Dn = _fma(D, f, through)
        if with_tol:
            eD = eD * f + e_pf * abs(float(wF[4])) + e_pi * abs(float(wI[4])) + U * a(pi * wI[4]) + U * a(through) + U * a(Dn)
            eCF = e_pf * abs(float(wF[5])) + U * a(pf * wF[5])
            eCI = e_pi * abs(float(wI[5])) + U * a(pi * wI[5])
        D = Dn
        cF, cI = pf * wF[5], pi * wI[5]
    if with_tol:
        return D, acc, eD + UNDERFLOW, acc_tol
    return D, acc


def steps_of_adapt(steps, k):
    """adapt's record of one tensor in backprop_tensor's form"""
    return [dict(th=s['before'][k], f=s['F'][k], i=s['I'][k], Fp=s['Fp'][k], Ip=s['Ip'][k], g=s['grads'][k], step=s['step'], L=s['L']) for s in steps]


def backprop(phi, steps, G, gate_scale=2.0, wrong=None):
    """-> (D = the outer gradient of theta through the learned rule, GPhi [14] in the dtype of G); no steps: (G, 0)"""
    dt = next(iter(G.values())).dtype
    D, acc = {}, np.zeros(NPHI)
    for k in G:
        D[k], a = backprop_tensor(phi, steps_of_adapt(steps, k), G[k], gate_scale, wrong) if steps else (G[k].copy(), np.zeros(NPHI))
        acc += a
    return D, acc.astype(dt)


def forward_backward(params, phi, support, query, config, inner_steps, inner_lr, gate_scale=2.0, mode='tf1_slices', gates0=None, wrong=None):
    """the train form up to the pending gradients -> dict(theta_prime, steps, loss, G (the query gradient at theta'), aux, D, GPhi)"""
    theta, steps = adapt(params, phi, support, config, inner_steps, inner_lr, gate_scale, mode, gates0, wrong)
    loss, G, aux = query_pass(theta, query, config)
    D, GPhi = backprop(phi, steps, G, gate_scale, wrong)
    return dict(theta_prime=theta, steps=steps, loss=loss, G=G, aux=aux, D=D, GPhi=GPhi)


def tasks_forward_backward(params, phi, support, query, config, inner_steps, inner_lr, gate_scale=2.0, mode='tf1_slices', wrong=None):
    """the per-artist train form: one adaptation per artist, D and GPhi folded with weight 1 / N (wrong 'artists_weight_one': 1)"""
    N = support.shape[0]
    w = 1.0 if wrong == 'artists_weight_one' else 1.0 / N
    out = dict(D=None, GPhi=np.zeros(NPHI), loss=0.0, aux=dict(embedding_slices_sq=0.0), passes=[])
    for n in range(N):
        fb = forward_backward(params, phi, support[n:n + 1], query[n:n + 1], config, inner_steps, inner_lr, gate_scale, mode)
        out['passes'].append(fb)
        out['D'] = {k: w * v for k, v in fb['D'].items()} if out['D'] is None else {k: out['D'][k] + w * fb['D'][k] for k in fb['D']}
        out['GPhi'] = out['GPhi'] + w * fb['GPhi'].astype(F64)
        out['loss'] += fb['loss'] / N
    return out


# ----------------------------------------------------------------------------- the outer update
def new_phi_state():
    return dict(m=np.zeros(NPHI), v=np.zeros(NPHI))


def phi_scalars(GPhi, step, config, lcfg, grad_scale=1.0):
    """(gnorm, scale, step size) as k_lopt_phi derives them: the plain global norm of GPhi, theta's schedule with phi_lr"""
    gnorm = float(np.sqrt((np.asarray(GPhi, F64) ** 2).sum())) * grad_scale
    clip = float(lcfg['phi_clip_norm'])
    scale = clip / max(gnorm, clip) * grad_scale if clip > 0 else grad_scale
    t = step + 1
    size = float(lcfg['phi_lr']) * 0.5 ** (step / float(config['n_decay'])) * np.sqrt(1.0 - O.BETA2 ** t) / (1.0 - O.BETA1 ** t)
    return gnorm, scale, size


def phi_update(phi, state, GPhi, step, config, lcfg, grad_scale=1.0, skipped=False, wrong=None):
    """clip + Adam (oracle.lstm_oracle.apply_update's element lines) of Phi -> the new Phi; mutates state.  phi_lr == 0 or a skipped
    step: nothing moves (wrong 'phi_on_skipped_step': it does)"""
    if float(lcfg['phi_lr']) == 0.0 or (skipped and wrong != 'phi_on_skipped_step'):
        return phi.copy()
    _, scale, size = phi_scalars(GPhi, step, config, lcfg, grad_scale)
    dt = phi.dtype.type
    g = np.asarray(GPhi, phi.dtype) * dt(scale)
    state['m'] = (dt(O.BETA1) * state['m'] + dt(1.0 - O.BETA1) * g).astype(phi.dtype)
    state['v'] = (dt(O.BETA2) * state['v'] + dt(1.0 - O.BETA2) * g * g).astype(phi.dtype)
    return (phi - dt(size) * state['m'] / (np.sqrt(state['v']) + dt(O.ADAM_EPS))).astype(phi.dtype)


def lopt_step(params, opt, phi, state, support, query, config, lcfg, inner_steps, inner_lr, mode='tf1_slices'):
    """one outer step on one rank: mutates params / opt / state -> (query loss at theta', the new Phi, the pass)"""
    gs = float(lcfg['gate_scale'])
    fb = forward_backward(params, phi, support, query, config, inner_steps, inner_lr, gs, mode)
    step = opt['step']
    O.apply_update(params, fb['D'], fb['aux'], opt, config, mode)          # theta: the MAML-style step's update on the rewritten gradient
    return fb['loss'], phi_update(phi, state, fb['GPhi'], step, config, lcfg), fb


def lopt_eval(params, phi, support, query, config, inner_steps, inner_lr, gate_scale=2.0, mode='tf1_slices'):
    theta, _ = adapt(params, phi, support, config, inner_steps, inner_lr, gate_scale, mode)
    return O.eval_step(theta, query, config)


def reduce_ranks(phi, passes, gate_scale=2.0, wrong=None):
    """GPhi of R ranks as the wrapper leaves it for apply_update(1 / R): the SUM of the per-rank GPhi ('gphi_after_reduce': formed from
    the summed query gradient on rank 0's stored steps, scaled so that 1 / R would give the mean-gradient form)"""
    if wrong == 'gphi_after_reduce':
        Gsum = {k: sum(p['G'][k] for p in passes) for k in passes[0]['G']}
        return backprop(phi, passes[0]['steps'], Gsum, gate_scale)[1].astype(F64)
    return sum(p['GPhi'].astype(F64) for p in passes)


# ----------------------------------------------------------------------------- the GPU test's element-wise bounds
def gate_reference(w, b, xs, e_x):
    """a gate in fp64 from fp32 inputs, and the bound of the fp32 evaluation:
      z: six fma from the bias, 6 u (|b| + sum |w x|), and the inputs' own errors |w| e(x);
      s = 1 / (1 + exp(-z)): expf to 1 ulp (2 u relative, ROCm device library), its argument's error e(z): s (1 - s) (e(z) + 2 u);
      the addition and the division, one rounding each: 2 u s"""
    w = np.asarray(w, F64)
    z = float(b) + sum(w[k] * np.asarray(xs[k], F64) for k in range(6))
    mag = abs(float(b)) + sum(abs(w[k]) * np.abs(np.asarray(xs[k], F64)) for k in range(6))
    ez = 6 * U * mag + sum(abs(w[k]) * e_x[k] for k in range(6))
    s = 1.0 / (1.0 + np.exp(-z))
    return s, s * (1.0 - s) * (ez + 2 * U) + 2 * U * s + UNDERFLOW


def step_reference(phi, g, L, theta, F, I, step, gate_scale):
    """one inner step of one tensor in fp64 from fp32 inputs -> (f, i, theta_t, tol_f, tol_i, tol_theta):
      q = f theta (one rounding): |theta| e(f) + u |q|;   st = step (gs i) (two roundings): 2 u st + step gs e(i)
      theta_t = fma(-st, g, q): e(q) + |g| e(st) + u |theta_t|"""
    phi = np.asarray(phi, F64)
    g, theta, F, I = (np.asarray(x, F64) for x in (g, theta, F, I))
    a1, a2, gbig = prep(g)
    c1, c2, Lbig = prep(np.asarray(F64(L)))
    e_x = (np.where(gbig, 3 * U * np.abs(a1), 0.0), np.where(gbig, 0.0, U * np.abs(a2)),
           float(3 * U * abs(c1)) if Lbig else 0.0, 0.0 if Lbig else float(U * abs(c2)), 0.0, 0.0)
    f, tf = gate_reference(phi[0:6], phi[6], (a1, a2, c1, c2, theta, F), e_x)
    i, ti = gate_reference(phi[7:13], phi[13], (a1, a2, c1, c2, theta, I), e_x)
    q = f * theta
    st = float(step) * (float(gate_scale) * i)
    new = q - st * g
    tt = np.abs(theta) * tf + U * np.abs(q) + np.abs(g) * (2 * U * st + float(step) * float(gate_scale) * ti) + U * np.abs(new) + UNDERFLOW
    return f, i, new, tf, ti, tt


def step_check(label, phi, theta_prev, F_prev, I_prev, grads, L, step, gate_scale, got_theta, got_F, got_I, verbose=True):
    """F, I and theta_t of one inner step, element by element against step_reference from fp32 (Phi, theta_{t-1}, F_{t-1}, I_{t-1}, g_t,
    L_t, step_t) as read from the device or produced by its stand-in -> (failures, worst error over bound)"""
    failures, worst = [], 0.0
    for k in sorted(grads):
        for x in (theta_prev[k], F_prev[k], I_prev[k], grads[k], got_theta[k], got_F[k], got_I[k]):
            assert np.asarray(x).dtype == F32, k
        f, i, new, tf, ti, tt = step_reference(phi, grads[k], L, theta_prev[k], F_prev[k], I_prev[k], step, gate_scale)
        fr = [np.abs(np.asarray(got, F64) - ref) / tol for got, ref, tol in ((got_F[k], f, tf), (got_I[k], i, ti), (got_theta[k], new, tt))]
        if verbose:
            print('LOPT|step|%s|%s|F %.3f|I %.3f|theta %.3f' % (label, k, fr[0].max(), fr[1].max(), fr[2].max()))
        for name, r, got in zip(('F', 'I', 'theta'), fr, (got_F[k], got_I[k], got_theta[k])):
            worst = max(worst, float(r.max()))
            if not np.all(np.isfinite(got)) or (r > 1).any():
                failures.append('%s %s: %d of %d outside the bound (worst %.2f x)' % (name, k, int((r > 1).sum()), r.size, r.max()))
    return failures, worst


def backprop_check(label, phi, steps, G, gate_scale, got_D, got_GPhi, verbose=True):
    """the rewritten G and GPhi against backprop_tensor in fp64 from fp32 inputs: steps[t] = dict(before, F, I, Fp, Ip, grads, step, L)
    with the DEVICE's forward values (adapt's record layout), G the query gradient before the rewrite -> (failures, worst D, worst GPhi).
    GPhi's bound: the sum of the per-term bounds, n 2^-53 of the sum of magnitudes for the fp64 additions, and u |GPhi| for the one
    rounding to fp32."""
    failures, worst_d = [], 0.0
    ref, tol, n_el = np.zeros(NPHI), np.zeros(NPHI), 0
    phi64 = np.asarray(phi, F64)
    for k in sorted(G):
        assert np.asarray(G[k]).dtype == F32 and np.asarray(got_D[k]).dtype == F32, k
        st = [dict(th=np.asarray(s['before'][k], F64), f=np.asarray(s['F'][k], F64), i=np.asarray(s['I'][k], F64), Fp=np.asarray(s['Fp'][k], F64),
                   Ip=np.asarray(s['Ip'][k], F64), g=np.asarray(s['grads'][k], F64), step=float(s['step']), L=float(s['L'])) for s in steps]
        D, acc, eD, acc_tol = backprop_tensor(phi64, st, np.asarray(G[k], F64), gate_scale, with_tol=True)
        r = np.abs(np.asarray(got_D[k], F64) - D) / eD
        worst_d = max(worst_d, float(r.max()))
        if verbose:
            print('LOPT|D|%s|%s|%.3f' % (label, k, r.max()))
        if not np.all(np.isfinite(got_D[k])) or (r > 1).any():
            failures.append('D %s: %d of %d outside the bound (worst %.2f x)' % (k, int((r > 1).sum()), r.size, r.max()))
        ref += acc
        tol += acc_tol
        n_el += D.size
    tol = tol * (1.0 + n_el * len(steps) * 2.0 ** -53 / U) + U * np.abs(ref) + UNDERFLOW
    rp = np.abs(np.asarray(got_GPhi, F64) - ref) / tol
    if verbose:
        print('LOPT|GPhi|%s|%s' % (label, ' '.join('%.3f' % x for x in rp)))
    if (rp > 1).any() or not np.all(np.isfinite(got_GPhi)):
        failures.append('GPhi: worst %.2f x' % rp.max())
    return failures, worst_d, float(rp.max()), ref, tol


def phi_check(phi0, slots0, GPhi, phi1, slots1, scale, size):
    """Phi and its slots after the update against fp64 from the device's own GPhi, by msgd_ref.alpha_check's bounds without the clamp"""
    import msgd_ref as SR
    A0, A1, G = {'phi': np.asarray(phi0, F32)}, {'phi': np.asarray(phi1, F32)}, {'phi': np.asarray(GPhi, F32)}
    return SR.alpha_check('phi', A0, {'phi': slots0}, G, A1, {'phi': slots1}, scale, size, -np.inf, np.inf, verbose=False)
