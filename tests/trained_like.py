"""The trained-like BatchNorm state and its reference fixture (tests/golden/gen_trained_golden.py: signed gamma, one
zero gamma per layer, running variances spread by exp(1.5 N), shifted means; folded |scale| from 0.03 to 95).

Shared by tests/test_trained_like_host.py (CPU), tests/trained_check.py (the GPU child) and
tests/test_gpu_trained_like.py.  Pure numpy; nothing here touches the GPU or the library.

  weights()        the full state dict: weights_seed0.npz with the fixture's `sd/<key>` tensors in place
  costreg_state()  names relative to `cost_regularization.`, as _lib.pack_weights takes them
  feature_state()  names relative to `feature.`, as _lib.pack_feature_weights takes them
  fixture()        inputs, fp32 stages, `<stage>_ref64` (rebuilt from the quantised differences), `e_ref/<stage>`
  extreme_*()      the same states with two channels per layer pushed to the ends: running_var = 0 (scale =
                   gamma / sqrt(eps), about 316 gamma) and scale = 2^-12 exactly (gamma 2^-12 on an identity variance:
                   every folded weight of the channel is below 2^-14, fp16's subnormal range)
"""
import functools
import os

import numpy as np

import featnet_ref
import probes
from conftest import GOLDEN, load_weights
from oracle import oracle as orc

STAGES = ("features", "variance", "cost_reg", "prob_volume", "expected_index", "depth", "photometric_confidence")
BN_EPS = np.float32(1e-5)
TINY_SCALE = np.float32(2.0 ** -12)


def _npz(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _files():
    return _npz("fx_trained.npz"), _npz("fx_trained_ref64.npz")


def fixture():
    fx, fx64 = _files()
    out = {k: v for k, v in fx.items() if not k.startswith("sd/")}
    for k in STAGES:
        if k + "_ref64" in fx64:
            out[k + "_ref64"] = fx64[k + "_ref64"]
        else:
            out[k + "_ref64"] = fx[k].astype(np.float64) + fx64[k + "_ref64_delta"].astype(np.float64) * float(fx64[k + "_ref64_unit"])
    return out


def weights():
    w = dict(load_weights())
    for k, v in _files()[0].items():
        if k.startswith("sd/"):
            assert k[3:] in w and w[k[3:]].shape == v.shape, k
            w[k[3:]] = v
    return w


def costreg_state():
    return orc.costreg_state(weights())


def feature_state():
    return featnet_ref.fstate(weights())


def _extreme(st, prefixes):
    """per BatchNorm, the first two channels with gamma != 0: running_var = 0 on the first; gamma = 2^-12 and an
    identity variance on the second.  Returns (state, {prefix: (channel of var 0, channel of scale 2^-12)})."""
    st = {k: np.array(v, copy=True) for k, v in st.items()}
    where = {}
    for pre in prefixes:
        a, b = np.flatnonzero(st[pre + ".weight"] != 0)[:2]
        st[pre + ".running_var"][a] = 0.0
        st[pre + ".weight"][b] = TINY_SCALE
        st[pre + ".running_var"][b] = probes.identity_var()
        where[pre] = (int(a), int(b))
    return st, where


def extreme_costreg_state():
    from scene_3dreconstruction_mvsnet_amd import _lib
    return _extreme(costreg_state(), _lib.BN_PREFIXES)


def extreme_feature_state():
    return _extreme(feature_state(), [f"conv{l}.bn" for l in range(7)])


def scale64(st, prefix):
    """gamma / sqrt(var + float32(1e-5)) in fp64 of the fp32 parameters"""
    g, v = (np.asarray(st[prefix + s], np.float64) for s in (".weight", ".running_var"))
    return g / np.sqrt(v + np.float64(BN_EPS))
