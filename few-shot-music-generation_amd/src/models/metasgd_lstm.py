"""Meta-SGD few-shot LSTM language model (Li et al., arXiv 1707.09835, first order) -- MI355X-native plugin.

MAMLLSTM (models/maml_lstm.py) learns the initialisation theta and fine-tunes it with one hand-set scalar `inner_lr`.  This plugin
also learns the fine-tuning procedure: a rate per parameter element, A, a multiplier of `inner_lr`, trained with theta by the outer
update from the first-order gradient -(query gradient * sum of the applied support steps) (semantics in full: include/fsmg.h
"Meta-SGD"; fp64 restatement tests/msgd_ref.py).  Everything MAMLLSTM offers -- train / train_indexed / eval /
generate / beam_search / score, maml_lengths -- runs unchanged with the learned rates in every adaptation.

  rates()         {parameter name: float32 array of A}

Extra config keys (config/metasgd_lstm.yaml): alpha_init (1.0: the first step is MAMLLSTM's), alpha_lr (the rates' Adam learning
rate on theta's decay schedule; 0: the rates are not trained), alpha_min / alpha_max (clamp after every update), alpha_clip_norm
(global-norm clip of the rates' gradient; 0: none).
The rates and their Adam slots are saved and restored next to the native checkpoint (<name>.metasgd.npz).  Episode-parallel: every
rank starts from alpha_init or the same file, the rates' gradient is all-reduced beside theta's (fsmg/dist.py), so replicas stay
identical; `dp_exchange: 'library'` is refused (the library's own exchange does not carry the rates' gradient).
"""
import os

import numpy as np

from models.maml_lstm import MAMLLSTM

DEFAULTS = dict(alpha_init=1.0, alpha_lr=1e-3, alpha_min=0.0, alpha_max=10.0, alpha_clip_norm=0.0)


def msgd_settings(config):
    """the alpha_* keys of a model config -> the keyword arguments of FsmgModel.msgd_config"""
    c = dict(DEFAULTS)
    c.update({k: config[k] for k in DEFAULTS if k in config and config[k] is not None})
    c = {k: float(v) for k, v in c.items()}
    if any(np.isnan(v) for v in c.values()):
        raise RuntimeError('a Meta-SGD config key is NaN: %r' % (c,))
    if not np.isfinite(c['alpha_init']):
        raise RuntimeError('alpha_init must be finite')
    if not (c['alpha_lr'] >= 0 and np.isfinite(c['alpha_lr'])) or not (c['alpha_clip_norm'] >= 0 and np.isfinite(c['alpha_clip_norm'])):
        raise RuntimeError('alpha_lr and alpha_clip_norm must be finite and >= 0')
    if c['alpha_min'] > c['alpha_max']:
        raise RuntimeError('alpha_min must not exceed alpha_max')
    return c


def save_rates(engine, path):
    """the rates of an engine (FsmgModel) and their Adam slots -> one .npz: alpha/<name>, adam_m/<name>, adam_v/<name>"""
    blob = {}
    for name in engine.param_shapes:
        blob['alpha/' + name] = engine.msgd_get_alpha(name)
        blob['adam_m/' + name], blob['adam_v/' + name] = engine.msgd_get_opt_state(name)
    tmp = path + '.tmp.npz'
    np.savez(tmp, **blob)
    os.replace(tmp, path)


def load_rates(engine, path):
    """-> True when the file exists and every tensor matched (the rates and slots are then the file's), else False with nothing set"""
    if not os.path.isfile(path):
        return False
    with np.load(path) as blob:
        names = list(engine.param_shapes)
        for n in names:
            for key in ('alpha/', 'adam_m/', 'adam_v/'):
                if key + n not in blob or blob[key + n].shape != engine._shape(n):
                    return False
        for n in names:
            engine.msgd_set_alpha(n, blob['alpha/' + n])
            engine.msgd_set_opt_state(n, blob['adam_m/' + n], blob['adam_v/' + n])
    return True


class _DeviceFloats(object):
    """n floats at a device address, for torch.as_tensor (the rates' gradient lives in the library's own allocation)"""
    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = dict(shape=(int(count),), typestr='<f4', data=(int(ptr), False), version=2)


class MetaSGDLSTM(MAMLLSTM):
    def __init__(self, config):
        super(MetaSGDLSTM, self).__init__(config)
        self._msgd = msgd_settings(config)
        self._rate_grad_tensor = None

    def _rates_path(self, checkpt_path):
        return os.path.join(checkpt_path, self.name, self.name + '.metasgd.npz')

    def recover_or_init(self, init_path):
        super(MetaSGDLSTM, self).recover_or_init(init_path)
        # every adaptation of this handle takes the rates from here on (A = alpha_init on the first enable)
        self._model.msgd_enable(**self._msgd)
        if init_path and load_rates(self._model, self._rates_path(init_path)):
            print('recovered the Meta-SGD rates')

    def save(self, checkpt_path):
        super(MetaSGDLSTM, self).save(checkpt_path)
        save_rates(self._model, self._rates_path(checkpt_path))

    def rates(self):
        self._require_init()
        return self._model.msgd_get_alphas()

    @property
    def rate_grad_tensor(self):
        """a torch tensor aliasing the rates' gradient buffer: what fsmg.dist.EpisodeParallel all-reduces beside grad_tensor"""
        if self._rate_grad_tensor is None:
            ptr, count = self._model.msgd_grad_buffer()
            self._rate_grad_tensor = self._torch.as_tensor(_DeviceFloats(ptr, count), device='cuda:%d' % self._device)
        return self._rate_grad_tensor
