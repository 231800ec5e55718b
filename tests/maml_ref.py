"""The MAML-style pass (cfg-E) against fp64, piece by piece (TEST INFRASTRUCTURE ONLY; numpy).

  * sgd_reference / device_gnorm / sgd_check: k_sgd_update's arithmetic (elementwise.hip) redone in fp64 on fp32 inputs, the norm
    as tid 0 of the kernel derives it, and the derived elementwise bound on theta' -- the counterparts of adam_reference /
    adam_scalars of tests/test_gpu_componentwise.py;
  * adapt_full: oracle.lstm_oracle.maml_adapt restated so that it returns every inner step's gradients, norm, scale and theta'_i
    (in fp64 it is the oracle bit for bit, tests/test_maml_componentwise_cpu.py), with the update line replaceable -- the fp32
    stand-in of the device (standin_update) and its wrong-by-construction variants go in there;
  * query_failures: the measures of tests/backward_ref.py over every tensor of the query pass at theta', without printing;
  * MAML_SHAPES: the shapes tests/test_gpu_maml_componentwise.py and the CPU file run.
"""
import numpy as np

import backward_ref as R
from oracle import lstm_oracle as O

U = 2.0 ** -24
F32 = np.float32
PARAM_ORDER_LAST = 'softmax_b'          # the flat buffer ends with it (api_layout.hip build_layout)


# ----------------------------------------------------------------------------- the shapes
# (config overrides, N, K, Q, inner_steps, episode seed); handles are created for N * (K + Q) sequences, as the plugin does, and
# run passes of N * K (support) and N * Q (query) rows
MAML_SHAPES = [
    (dict(hidden_size=20, embedding_size=10, input_size=50, max_len=7), 1, 1, 1, 1, 3),             # nothing a multiple of 16 or 4
    (dict(hidden_size=32, embedding_size=12, input_size=77, max_len=6, n_layers=2), 3, 2, 2, 2, 3),  # stacked; step 2 starts from theta'_1
    (dict(hidden_size=200, embedding_size=24, input_size=90, max_len=7), 5, 3, 2, 1, 3),            # slice kernels; pads beside live units
    (dict(hidden_size=512, embedding_size=16, input_size=60, max_len=6), 5, 3, 2, 2, 3),            # fp32 XCD-local kernels; 15 and 10 rows
    (dict(hidden_size=512, embedding_size=16, input_size=60, max_len=5), 20, 4, 1, 1, 3),           # created for 100: bf16-split passes of 80 and 20
    # support 35 rows: three row groups per weight copy, the smallest count from which the bf16-split pair kernels pay is 33
    # (lstm_xcd.hip lstm_xcd_bx3_pays: ceil(ceil(B / 4) / 4) >= 3); query 10 rows: the fp32 pair chains.  The format changes inside
    # every step -- the test asserts that from the handle
    (dict(hidden_size=1024, embedding_size=16, input_size=60, max_len=4, n_layers=1), 5, 7, 2, 1, 3),
]
INNER_LR = 0.1                          # config/maml_lstm.yaml
# The inner clip must be ACTIVE for its scale and the norm behind it to show in theta'.  From the fp64 oracle at initial_theta():
# the first support gradient has norm 0.59 (shape 1), 0.83, 0.79, 0.81, 0.77, 0.73 (shape 6), under either clip mode to three
# digits, and the second inner step's is within 0.3 % of the first's.  0.3 is below every one of them, 50 above.
MAX_GRAD_NORM, MAX_GRAD_NORM_INACTIVE = 0.3, 50


def config_of(shape, **over):
    from conftest import small_config
    c = dict(shape[0], max_grad_norm=MAX_GRAD_NORM)
    c.update(over)
    return small_config(**c)


def initial_theta(cfg):
    """seeded fp32 parameters, the same on the device and in the oracle (the library's own seeded init has an RNG of its own)"""
    return O.glorot_init(cfg, 0, np.float32)


def f64(params):
    return {k: np.asarray(v, np.float64) for k, v in params.items()}


def shape_id(shape):
    over, N, K, Q, n, seed = shape
    return R.shape_id((over, N, K, Q, seed)) + '-i%d' % n


def episode(cfg, shape):
    over, N, K, Q, n, seed = shape
    return R.episode(cfg, N, K, Q, seed)


# ----------------------------------------------------------------------------- k_sgd_update, from fp32 inputs
def sgd_step(gnorm, clip, lr):
    """the kernel's fp32 step: (float)(clip / fmax(gnorm, clip)) * lr, clip and lr as the fp32 values the kernel holds"""
    clip = float(F32(clip))
    return float(F32(F32(clip / max(float(gnorm), clip)) * F32(lr)))


def sgd_reference(p, g, gnorm, clip, lr):
    """k_sgd_update's element line p - step * g in fp64 on fp32 inputs, with the kernel's fp32 step -> (p_ref, |step * g|)"""
    step = sgd_step(gnorm, clip, lr)
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    return p - step * g, np.abs(step * g)


def device_gnorm(grads, tail, mode):
    """the global norm as tid 0 of k_sgd_update / k_adam_update derives it from fp32 gradients (fp64 sums): under tf1_slices
    the embedding term is tail[0], the squared norm of the un-deduplicated slices, not the dense gradient's"""
    sq = sum(float((np.asarray(g, np.float64) ** 2).sum()) for k, g in grads.items() if not (k == 'embedding' and mode == 'tf1_slices'))
    if mode == 'tf1_slices':
        sq += float(tail[0])
    return float(np.sqrt(sq))


def sgd_check(label, theta_prev, grads, tail, mode, clip, lr, got_theta, got_gnorm, verbose=True):
    """theta' element by element against k_sgd_update redone from (theta_prev, grads, tail), all fp32 as read from a device (or
    from its stand-in):
        |got - p_ref| <= 2 u |p_ref| + 8 u |step * g| + 1e-30,  u = 2^-24
    -- one rounding of the product (none if the compiler contracts it into the subtraction), one of the subtraction, and a step
    that is known to three roundings (the quotient, the product with lr, and the norm it came from); an element with g == 0 must
    be theta_prev's bits (an absent token's embedding row); the norm the kernel reports must be device_gnorm to 2 * 2^-24.
    -> (gnorm, step, failures: list of strings); prints the worst error of every tensor in units of its bound"""
    gnorm = device_gnorm(grads, tail, mode)
    failures = []
    if not abs(float(got_gnorm) - gnorm) <= 2 * U * gnorm:
        failures.append('gnorm %.9g, from the gradients %.9g' % (float(got_gnorm), gnorm))
    step = sgd_step(gnorm, clip, lr)
    for k in sorted(grads):
        p0, g, got = (np.asarray(a) for a in (theta_prev[k], grads[k], got_theta[k]))
        assert p0.dtype == g.dtype == got.dtype == F32, (k, p0.dtype, g.dtype, got.dtype)
        p_ref, sg = sgd_reference(p0, g, gnorm, clip, lr)
        tol = 2 * U * np.abs(p_ref) + 8 * U * sg + R.UNDERFLOW
        frac = np.abs(got.astype(np.float64) - p_ref) / tol
        still = (g == 0) & (got.view(np.uint32) != p0.view(np.uint32))
        if verbose:
            print('SGD|%s|%s|%.3f|%d' % (label, k, frac.max(), int((g == 0).sum())))
        if not np.all(np.isfinite(got)) or (frac > 1).any():
            failures.append('%s: %d of %d outside the bound (worst %.1f x)' % (k, int((frac > 1).sum()), frac.size, frac.max()))
        if still.any():
            failures.append('%s: %d elements without a gradient moved' % (k, int(still.sum())))
    return gnorm, step, failures


# ----------------------------------------------------------------------------- maml_adapt, with everything it computes on the way
def adapt_full(params, support, config, inner_steps=1, inner_lr=0.1, clip_norm_mode='tf1_slices', update=None):
    """oracle.lstm_oracle.maml_adapt in the oracle's order -> (theta', steps); steps[i] = dict(before = theta'_i, loss, grads, aux,
    gnorm, scale, gnorm_out, theta = theta'_{i+1}).  update(fast, grads, aux) -> (new parameters, the norm it reports) replaces
    the oracle's update line (None: the oracle's own; fp64 parameters then give O.maml_adapt bit for bit)."""
    d = O.model_dims(config)
    fast = {k: v.copy() for k, v in params.items()}
    X, Y = O.tokens_to_input_and_target(support, d['start'])
    clip = float(config['max_grad_norm'])
    steps = []
    for _ in range(int(inner_steps)):
        loss, cache = O.forward(fast, X, Y, config)
        grads, aux = O.backward(fast, cache, config)
        gnorm = O.global_norm(grads, aux, clip_norm_mode)
        scale = clip / max(gnorm, clip)
        if update is None:
            new, gnorm_out = {}, gnorm
            for k in fast:
                dt = fast[k].dtype.type
                new[k] = fast[k] - dt(inner_lr) * (grads[k] * dt(scale))
        else:
            new, gnorm_out = update(fast, grads, aux)
        steps.append(dict(before=fast, loss=float(loss), grads=grads, aux=aux, gnorm=gnorm, scale=scale, gnorm_out=gnorm_out, theta=new))
        fast = new
    return fast, steps


def standin_tail(aux):
    """the gradient tail as the device leaves it, as far as the update reads it: tail[0] = the slices' squared norm, fp32"""
    tail = np.zeros(16, F32)
    tail[0] = aux['embedding_slices_sq']
    return tail


WRONG = ('dense_norm', 'no_clip', 'last_float4', 'absent_row_ulp')


def standin_update(config, mode, inner_lr, wrong=None):
    """k_sgd_update in numpy fp32 (the device's stand-in on a machine without one) for adapt_full(update=...), fp32 parameters.
    wrong: one of WRONG -- the same kernel with one planted mistake:
      dense_norm      the dense gradient's norm where tf1_slices is configured (use_slices flipped)
      no_clip         lr applied without the clip scale
      last_float4     the last four elements of the flat buffer left as they were
      absent_row_ulp  one element of an absent token's embedding row moved by one ulp"""
    assert wrong is None or wrong in WRONG, wrong
    clip = float(F32(config['max_grad_norm']))

    def update(fast, grads, aux):
        for k in fast:
            assert fast[k].dtype == grads[k].dtype == F32, k
        norm_mode = 'dense' if (wrong == 'dense_norm' and mode == 'tf1_slices') else mode
        gnorm = device_gnorm(grads, standin_tail(aux), norm_mode)
        step = F32(inner_lr) if wrong == 'no_clip' else F32(F32(clip / max(gnorm, clip)) * F32(inner_lr))
        new = {k: fast[k] - step * grads[k] for k in fast}
        if wrong == 'last_float4':
            new[PARAM_ORDER_LAST].reshape(-1)[-4:] = fast[PARAM_ORDER_LAST].reshape(-1)[-4:]
        if wrong == 'absent_row_ulp':
            absent = np.flatnonzero(np.all(grads['embedding'] == 0, axis=1))
            assert len(absent) > 0, 'every token occurs'
            e = new['embedding']
            e[absent[0], 0] = np.nextafter(e[absent[0], 0], F32(np.inf))
        for k in new:
            assert new[k].dtype == F32, k
        return new, float(F32(gnorm))
    return update


def adapt_failures(label, params32, support, config, inner_steps, inner_lr, mode, wrong=None, verbose=False):
    """the stand-in's adaptation held to sgd_check at every inner step, exactly as the GPU test holds the device
    -> (theta' fp32, failures)"""
    theta, steps = adapt_full(params32, support, config, inner_steps, inner_lr, mode, update=standin_update(config, mode, inner_lr, wrong))
    failures = []
    for i, s in enumerate(steps):
        _, _, bad = sgd_check('%s|%d' % (label, i + 1), s['before'], s['grads'], standin_tail(s['aux']), mode, config['max_grad_norm'],
                              inner_lr, s['theta'], s['gnorm_out'], verbose)
        failures += ['step %d: %s' % (i + 1, b) for b in bad]
    return theta, failures


# ----------------------------------------------------------------------------- the query pass at theta'
def query_reference(theta32, query, config):
    """fp64 oracle pass + fp32 yardstick (backward_ref.Reference) of the query rows at the given fp32 theta', upcast"""
    X, Y = O.tokens_to_input_and_target(query, config['input_size'])
    return R.Reference({k: np.asarray(v, np.float64) for k, v in theta32.items()}, X, Y, config)


def pass_tensors32(params32, query, config):
    """every checked tensor of an fp32 pass over the query rows -> (loss, {(family, layer): array})"""
    X, Y = O.tokens_to_input_and_target(query, config['input_size'])
    loss, _, _, t = R._tensors(params32, X, Y, config)
    return loss, t


def query_failures(ref, got, M):
    """{'family_layer': (elements outside M * e32, worst err in units of e32)} over the tensors of `got`, failures only"""
    out = {}
    for (fam, layer), g in got.items():
        bad = ref.failures(fam, layer, g, M)
        if bad.any():
            out[fam if layer is None else '%s_%d' % (fam, layer)] = (int(bad.sum()), ref.ratio(fam, layer, g)[0])
    return out
