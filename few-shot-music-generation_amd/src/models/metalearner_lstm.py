"""Meta-learner LSTM few-shot language model (Ravi & Larochelle, "Optimization as a model for few-shot learning", first order) --
MI355X-native plugin.

MAMLLSTM (models/maml_lstm.py) fine-tunes theta with one hand-set scalar `inner_lr`; MetaSGDLSTM learns a fixed rate per element.
This plugin learns the update RULE: a forget gate and an input gate per parameter element, computed from that element's support
gradient, the support loss, the element's value and the previous gates, with fourteen weights Phi shared by all elements and trained
with theta by the outer update (semantics in full: include/fsmg.h "learned optimiser"; fp64 restatement
tests/lopt_ref.py).  Everything MAMLLSTM offers -- train / train_indexed / eval / generate / beam_search / score, maml_lengths,
maml_per_artist -- runs unchanged with the learned rule in every adaptation.

  phi()           float32 [14]: wF[6], bF, wI[6], bI

Extra config keys (config/metalearner_lstm.yaml): bF_init / bI_init (the biases of the first enable; the weights start at zero),
gate_scale (2: bI = 0 is the plain rate), phi_lr (Phi's Adam learning rate on theta's decay schedule; 0: Phi is not trained),
phi_clip_norm (global-norm clip of GPhi; 0: none), max_train_steps (1 .. 8, at least inner_steps).
Phi and its Adam slots are saved and restored next to the native checkpoint (<name>.lopt.npz).  Episode-parallel: every rank starts
from the same Phi, GPhi is all-reduced beside theta's gradient (fsmg/dist.py), so replicas stay identical; `dp_exchange: 'library'`
is refused (the library's own exchange does not carry GPhi).
"""
import os

import numpy as np

from models.maml_lstm import MAMLLSTM

DEFAULTS = dict(bF_init=6.0, bI_init=0.0, gate_scale=2.0, phi_lr=1e-3, phi_clip_norm=0.0, max_train_steps=1)
NPHI = 14


def lopt_settings(config):
    """the learned optimiser's keys of a model config -> the keyword arguments of FsmgModel.lopt_config"""
    c = dict(DEFAULTS)
    c.update({k: config[k] for k in DEFAULTS if k in config and config[k] is not None})
    steps = c.pop('max_train_steps')
    c = {k: float(v) for k, v in c.items()}
    if not all(np.isfinite(v) for v in c.values()):
        raise RuntimeError('a learned-optimiser config key is NaN or not finite: %r' % (c,))
    if c['phi_lr'] < 0 or c['phi_clip_norm'] < 0:
        raise RuntimeError('phi_lr and phi_clip_norm must be >= 0')
    if not c['gate_scale'] > 0:
        raise RuntimeError('gate_scale must be > 0')
    if int(steps) != steps or not 1 <= int(steps) <= 8:
        raise RuntimeError('max_train_steps must be an integer in [1, 8]')
    c['max_train_steps'] = int(steps)
    return c


def save_phi(engine, path):
    """Phi of an engine (FsmgModel) and its Adam slots -> one .npz: phi, adam_m, adam_v"""
    m, v = engine.lopt_get_opt_state()
    tmp = path + '.tmp.npz'
    np.savez(tmp, phi=engine.lopt_get_phi(), adam_m=m, adam_v=v)
    os.replace(tmp, path)


def load_phi(engine, path):
    """-> True when the file exists and holds three arrays of 14 (Phi and the slots are then the file's), else False with nothing set"""
    if not os.path.isfile(path):
        return False
    with np.load(path) as blob:
        for key in ('phi', 'adam_m', 'adam_v'):
            if key not in blob or blob[key].shape != (NPHI,):
                return False
        engine.lopt_set_phi(blob['phi'])
        engine.lopt_set_opt_state(blob['adam_m'], blob['adam_v'])
    return True


class _DeviceFloats(object):
    """n floats at a device address, for torch.as_tensor (GPhi lives in the library's own allocation)"""
    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = dict(shape=(int(count),), typestr='<f4', data=(int(ptr), False), version=2)


class MetaLearnerLSTM(MAMLLSTM):
    def __init__(self, config):
        super(MetaLearnerLSTM, self).__init__(config)
        self._lopt = lopt_settings(config)
        if int(config.get('inner_steps', 1)) > self._lopt['max_train_steps']:
            raise RuntimeError('inner_steps %d exceeds max_train_steps %d' % (int(config.get('inner_steps', 1)), self._lopt['max_train_steps']))
        self._lopt_grad_tensor = None

    def _phi_path(self, checkpt_path):
        return os.path.join(checkpt_path, self.name, self.name + '.lopt.npz')

    def recover_or_init(self, init_path):
        super(MetaLearnerLSTM, self).recover_or_init(init_path)
        # every adaptation of this handle takes the learned rule from here on (w = 0, bF_init, bI_init on the first enable)
        self._model.lopt_enable(**self._lopt)
        if init_path and load_phi(self._model, self._phi_path(init_path)):
            print('recovered the learned optimiser')

    def save(self, checkpt_path):
        super(MetaLearnerLSTM, self).save(checkpt_path)
        save_phi(self._model, self._phi_path(checkpt_path))

    def phi(self):
        self._require_init()
        return self._model.lopt_get_phi()

    @property
    def lopt_grad_tensor(self):
        """a torch tensor aliasing GPhi: what fsmg.dist.EpisodeParallel all-reduces beside grad_tensor"""
        if self._lopt_grad_tensor is None:
            ptr, count = self._model.lopt_grad_buffer()
            self._lopt_grad_tensor = self._torch.as_tensor(_DeviceFloats(ptr, count), device='cuda:%d' % self._device)
        return self._lopt_grad_tensor
