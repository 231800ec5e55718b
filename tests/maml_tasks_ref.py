"""Per-artist MAML (include/fsmg.h "per-artist MAML") restated in numpy (TEST INFRASTRUCTURE ONLY).

  * reference: the fp64 statement -- the mean over the artists n of oracle.lstm_oracle.maml_query_grads / maml_eval (with lengths:
    tests/maml_masked_ref.py's) on the one-artist episodes support[n:n+1], query[n:n+1]; the slice aux is folded with w^2, the
    Meta-SGD rate gradient (rates all one, tests/msgd_ref.py) like the gradient;
  * bounds: what tests/test_gpu_maml_tasks.py holds the device to against it, and distance(): a result's worst error in units of them;
  * fold32 / fold32_pow2: the fold of k_task_fold (csrc/tasks.hip) in numpy float32 -- the stand-in of the device for the CPU file
    and, where N is a power of two and w * g is exact, the bits the device must give;
  * standin: the whole call in fp32 (maml_ref.standin_update for the inner steps), folded by fold32;
  * wrong=: the statement with ONE planted mistake (WRONG), for tests/test_maml_tasks_cpu.py to show that the bounds see it;
  * SHAPES: the shapes both files run.
"""
import numpy as np

import backward_ref as R
import maml_masked_ref as MM
import maml_ref as MR
import msgd_ref as SR
from oracle import lstm_oracle as O

F32 = np.float32
U = MR.U
NLL_RTOL = 1e-4             # the project's bound on a loss (tests/test_gpu_maml_componentwise.py)
REL_MAX = 5e-4              # ... and on a gradient tensor, relative to its largest element
LR = MR.INNER_LR

# name -> (config overrides, N, K, Q, inner_steps, episode seed); max_grad_norm is maml_ref.MAX_GRAD_NORM: every inner clip is active.
# The seeds were chosen here, from the fp64 reference alone: at every shape from B on the joint adaptation of today's
# fsmg_maml_forward_backward is more than 10 bounds away from the per-artist statement (tests/test_maml_tasks_cpu.py asserts it).
SHAPES = {
    'A': (dict(hidden_size=20, embedding_size=10, input_size=50, max_len=7), 1, 1, 1, 1, 3),      # n_flat below one block's sweep
    'B': (dict(hidden_size=32, embedding_size=12, input_size=77, max_len=6, n_layers=2), 2, 2, 2, 2, 3),
    'C': (dict(hidden_size=200, embedding_size=24, input_size=90, max_len=7), 3, 3, 2, 1, 3),     # pads beside live units
    'D': (dict(hidden_size=512, embedding_size=16, input_size=60, max_len=6), 4, 3, 2, 2, 3),     # many blocks, fp32 XCD-local
    'E': (dict(hidden_size=512, embedding_size=16, input_size=60, max_len=5), 5, 4, 1, 1, 3),     # created for 100: bf16-split passes of 4 and 1
    'F': (dict(hidden_size=1024, embedding_size=16, input_size=60, max_len=4, n_layers=1), 2, 3, 2, 1, 3),   # pair chains
}
CREATED_FOR = {'E': 100}    # sequences the handle is created for where that is not N * (K + Q)

WRONG = ('joint_adaptation', 'theta_not_restored_between_artists', 'weight_1_instead_of_1_over_N', 'slice_norm_folded_with_w',
         'first_artist_accumulates_into_stale_acc', 'rate_gradient_from_last_artist_only')


def cut_to_one_artist(shape):
    over, N, K, Q, n, seed = shape
    return (over, 1, K, Q, n, seed)


def rows_of(name, shape):
    over, N, K, Q, n, seed = shape
    return CREATED_FOR.get(name, N * (K + Q))


def config_of(shape, **over):
    return MR.config_of(shape, **over)


def episode(cfg, shape):
    over, N, K, Q, n, seed = shape
    sup, qry = R.episode(cfg, N, K, Q, seed)
    return sup.astype(np.int32), qry.astype(np.int32)


def lengths_of(shape, T):
    return MM.lengths_of(shape, T)


# ----------------------------------------------------------------------------- one artist, in the dtype of the parameters
def _artist(params, sup, qry, cfg, n, lr, mode, sl=None, ql=None, rates=False):
    """artist a's one-artist episode -> dict(loss, grads, aux, theta, [GA])"""
    if sl is None:
        loss, grads, aux = O.maml_query_grads(params, sup, qry, cfg, n, lr, clip_norm_mode=mode)
        theta, _ = O.maml_adapt(params, sup, cfg, n, lr, clip_norm_mode=mode)
    else:
        r = MM.query_grads(params, sup, qry, sl, ql, cfg, n, lr, mode)
        loss, grads, aux, theta = r['loss'], r['grads'], r['aux'], r['theta']
    out = dict(loss=float(loss), grads=grads, aux=float(aux['embedding_slices_sq']), theta=theta)
    if rates:
        assert sl is None
        A = SR.const_rates(cfg, 1.0, next(iter(params.values())).dtype)
        out['GA'] = SR.forward_backward(params, A, sup, qry, cfg, n, lr, mode)['GA']
    return out


def _mean(xs, N, power=1):
    w = (1.0 / N) ** power
    out = xs[0] * w
    for x in xs[1:]:
        out = out + x * w
    return out


def reference(params, sup, qry, cfg, n, lr=LR, mode='tf1_slices', lengths=None, rates=False, wrong=None):
    """the fp64 statement -> dict(loss, grads, aux, task_loss [N], artists, bound {name: float}, aux_bound, [GA, ga_bound])"""
    assert wrong is None or wrong in WRONG, wrong
    N = sup.shape[0]
    sl, ql = lengths if lengths is not None else (None, None)
    artists, start = [], params
    for a in range(N):
        one = _artist(start, sup[a:a + 1], qry[a:a + 1], cfg, n, lr, mode, None if sl is None else sl[a:a + 1],
                      None if ql is None else ql[a:a + 1], rates)
        artists.append(one)
        if wrong == 'theta_not_restored_between_artists':
            start = one['theta']
    names = sorted(artists[0]['grads'])
    out = dict(artists=artists, task_loss=np.array([a['loss'] for a in artists]))
    w_pow = 0 if wrong == 'weight_1_instead_of_1_over_N' else 1
    fold = lambda xs, power=1: _mean(xs, N, power * w_pow)
    out['loss'] = float(fold([a['loss'] for a in artists]))
    out['grads'] = {k: fold([a['grads'][k] for a in artists]) for k in names}
    out['aux'] = float(fold([a['aux'] for a in artists], 1 if wrong == 'slice_norm_folded_with_w' else 2))
    if rates:
        out['GA'] = {k: fold([a['GA'][k] for a in artists]) for k in names}
        if wrong == 'rate_gradient_from_last_artist_only':
            out['GA'] = {k: artists[-1]['GA'][k].copy() for k in names}
    if wrong == 'first_artist_accumulates_into_stale_acc':      # ACC still holds the fold of the call before: the same episode's here
        out['grads'] = {k: 2.0 * v for k, v in out['grads'].items()}
        out['loss'], out['aux'] = 2.0 * out['loss'], 2.0 * out['aux']
    if wrong == 'joint_adaptation':                             # today's semantics: one theta' from all N * K support rows
        one = _artist(params, sup, qry, cfg, n, lr, mode, sl, ql, rates)
        out.update(loss=one['loss'], grads=one['grads'], aux=one['aux'])
        if rates:
            out['GA'] = one['GA']
    # the bounds: every G_n is held to REL_MAX of its own largest element (tests/test_gpu_maml_componentwise.py); the mean of the
    # artists may cancel, so the triangle inequality over the fold is what follows for it -- not a bound relative to the mean's maximum
    w = 1.0 / N
    out['bound'] = {k: REL_MAX * sum(w * float(np.abs(a['grads'][k]).max()) for a in artists) for k in names}
    out['aux_bound'] = REL_MAX * sum(w * w * a['aux'] for a in artists)
    if rates:
        out['ga_bound'] = {k: REL_MAX * sum(w * float(np.abs(a['GA'][k]).max()) for a in artists) for k in names}
    return out


def eval_reference(params, sup, qry, cfg, n, lr=LR, mode='tf1_slices', lengths=None):
    """-> (mean over the artists of the query NLL at that artist's theta', the per-artist NLLs)"""
    N = sup.shape[0]
    if lengths is None:
        per = [O.maml_eval(params, sup[a:a + 1], qry[a:a + 1], cfg, n, lr, clip_norm_mode=mode) for a in range(N)]
    else:
        sl, ql = lengths
        per = [MM.maml_eval(params, sup[a:a + 1], qry[a:a + 1], sl[a:a + 1], ql[a:a + 1], cfg, n, lr, mode) for a in range(N)]
    return float(sum(per) / N), np.array(per)


def distance(ref, got):
    """the worst error of `got` (dict(loss, grads, [aux], [GA])) against reference() `ref`, in units of ref's bounds -> {what: ratio};
    the loss in units of NLL_RTOL * |loss|"""
    b = ref
    out = {'loss': abs(float(got['loss']) - b['loss']) / (NLL_RTOL * abs(b['loss']))}
    for k, bound in b['bound'].items():
        out['grad:' + k] = float(np.abs(np.asarray(got['grads'][k], np.float64) - b['grads'][k]).max()) / bound
    if 'aux' in got:
        out['aux'] = abs(float(got['aux']) - b['aux']) / b['aux_bound']
    if 'GA' in got and 'ga_bound' in b:
        for k, bound in b['ga_bound'].items():
            out['rate:' + k] = float(np.abs(np.asarray(got['GA'][k], np.float64) - b['GA'][k]).max()) / bound
    return out


# ----------------------------------------------------------------------------- the fold of k_task_fold
def _fma32(w, g, acc):
    """fl32(w * g + acc): the product of two fp32 numbers is exact in fp64, the sum is rounded to fp64 and then to fp32 -- the fma's
    single rounding except where the fp64 sum lands on an fp32 tie, which a stand-in may get wrong by one ulp"""
    return (np.asarray(w, np.float64) * np.asarray(g, np.float64) + np.asarray(acc, np.float64)).astype(F32)


def fold32(xs, N, w=None):
    """ACC = w * x_0, then fma(w, x_n, ACC); N == 1: x_0's bits"""
    assert len(xs) == N and all(np.asarray(x).dtype == F32 for x in xs)
    if N == 1:
        return np.array(xs[0], F32, copy=True)
    w = F32(1.0 / N) if w is None else F32(w)
    acc = (w * np.asarray(xs[0])).astype(F32)
    for x in xs[1:]:
        acc = _fma32(w, x, acc)
    return acc


def fold32_pow2(xs, N, w=None):
    """the same in plain float32 arithmetic, bit for bit what the kernel gives where w is a power of two and no w * x underflows:
    the product is exact then, so the fma's rounding is the addition's"""
    assert N & (N - 1) == 0 and len(xs) == N
    if N == 1:
        return np.array(xs[0], F32, copy=True)
    w = F32(1.0 / N) if w is None else F32(w)
    acc = w * np.asarray(xs[0], F32)
    for x in xs[1:]:
        acc = acc + w * np.asarray(x, F32)
    assert acc.dtype == F32
    return acc


def exactness_holds(xs):
    """no non-zero element below 2^-120: w * x is exact for every w >= 2^-6"""
    return all(float(np.abs(x[x != 0]).min()) >= 2.0 ** -120 for x in map(np.asarray, xs) if np.any(x != 0))


def fold_tail32(tails, N):
    """[slice sum of squares, loss] of N tails: w * w for the first, w for the second"""
    w = F32(1.0 / N)
    ww = F32(w * w)
    return (fold32([np.asarray(t[0], F32).reshape(1) for t in tails], N, ww)[0],
            fold32([np.asarray(t[1], F32).reshape(1) for t in tails], N, w)[0])


def rounding_bound(xs, N):
    """|fold32 - the fp64 fold of the fp32 x_n with the fp32 w| <= one fp32 rounding per folded artist: N u sum_n |w x_n| (+ underflow)
    -> (fp64 fold, bound)"""
    w = float(F32(1.0 / N))
    ref = sum(w * np.asarray(x, np.float64) for x in xs)
    return ref, N * U * sum(abs(w) * np.abs(np.asarray(x, np.float64)) for x in xs) + 1e-44


# ----------------------------------------------------------------------------- the whole call in fp32: the device's stand-in
def standin(params32, sup, qry, cfg, n, lr=LR, mode='tf1_slices'):
    """per artist maml_ref's fp32 adaptation and an fp32 query pass, folded by fold32 -> dict(loss, grads, aux, task_loss)"""
    N = sup.shape[0]
    d = O.model_dims(cfg)
    per = []
    for a in range(N):
        theta, _ = MR.adapt_full(params32, sup[a:a + 1], cfg, n, lr, mode, update=MR.standin_update(cfg, mode, lr))
        X, Y = O.tokens_to_input_and_target(qry[a:a + 1], d['start'])
        loss, cache = O.forward(theta, X, Y, cfg)
        grads, aux = O.backward(theta, cache, cfg)
        per.append((F32(loss), {k: np.asarray(g, F32) for k, g in grads.items()}, F32(aux['embedding_slices_sq'])))
    aux, loss = fold_tail32([(p[2], p[0]) for p in per], N)
    return dict(loss=loss, aux=aux, task_loss=np.array([p[0] for p in per], F32),
                grads={k: fold32([p[1][k] for p in per], N) for k in per[0][1]})
