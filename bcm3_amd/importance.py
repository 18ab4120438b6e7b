"""The importance sampler (sampler.type = is; libbcm3.so bcm3_is_*, csrc/host/SamplerISDevice.cpp).

SamplerIS::RunImpl (src/sampler/SamplerIS.cpp:49-87) in batches on the device: draws from the prior
(csrc/is_kernels.hip is_draw_kernel), one batched likelihood launch per round, and the reference's
weight rule in draw order (is_filter_kernel): a draw is kept unless its log weight is more than
23.02585 below the highest seen so far. The loop is C++; this module configures it, reads results
back, and wraps the two kernels and the filter's host restatement for the tests.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _hip
from .likelihood import Likelihood, lib as host_lib

LOG_WEIGHT_WINDOW = 23.02585  # SamplerIS.cpp:76


class ISState(C.Structure):
    """bcm3hip_is_state (include/bcm3hip.h): the filter's state between batches"""
    _fields_ = [("run_max", C.c_double), ("kept", C.c_int64), ("consumed", C.c_int64), ("nan_flag", C.c_int32),
                ("pad_", C.c_int32)]


STATE_DTYPE = np.dtype([("run_max", "f8"), ("kept", "i8"), ("consumed", "i8"), ("nan_flag", "i4"), ("pad_", "i4")])


def new_state() -> ISState:
    return ISState(-np.inf, 0, -1, 0, 0)


class ISConfig(C.Structure):
    """bcm3_is_config (include/bcm3.h)"""
    _fields_ = [("seed", C.c_uint64), ("learning_rate", C.c_double), ("batch", C.c_int64)]


class ISRunConfig(C.Structure):
    """bcm3_is_run_config (include/bcm3.h): config.txt as the importance sampler reads it"""
    _fields_ = [
        ("is_", ISConfig), ("num_samples", C.c_int64), ("sampler_type", C.c_char * 64), ("prior", C.c_char * 1024),
        ("likelihood", C.c_char * 1024), ("output_folder", C.c_char * 1024), ("likelihood_options", C.c_char * 2048),
    ]


_bound = False


def _kernels():
    global _bound
    L = _hip.lib()
    if not _bound:
        vp, i64, u64 = C.c_void_p, C.c_int64, C.c_uint64
        L.bcm3hip_is_draw.argtypes = [i64, C.c_int, vp, vp, vp, vp, u64, u64, vp, vp, vp]
        L.bcm3hip_is_filter.argtypes = [i64, C.c_int, vp, vp, vp, C.c_double, i64, vp, vp, vp, vp, vp, vp]
        L.bcm3hip_is_filter_host.argtypes = [i64, C.c_int, vp, vp, vp, C.c_double, i64, C.POINTER(ISState), vp, vp,
                                             vp, vp]
        H = host_lib()
        H.bcm3_is_config_default.argtypes = [C.POINTER(ISConfig)]
        H.bcm3_is_config_default.restype = None
        H.bcm3_is_config_from_file.argtypes = [C.c_char_p, C.POINTER(ISRunConfig)]
        H.bcm3_is_create.argtypes = [vp, C.c_char_p, C.POINTER(ISConfig), C.POINTER(vp)]
        H.bcm3_is_run.argtypes = [vp, i64]
        H.bcm3_is_num_samples.argtypes = [vp]
        H.bcm3_is_num_samples.restype = i64
        H.bcm3_is_get_samples.argtypes = [vp, vp, vp, vp, vp]
        H.bcm3_is_get_counters.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double)]
        H.bcm3_is_set_output.argtypes = [vp, C.c_char_p]
        H.bcm3_is_destroy.argtypes = [vp]
        H.bcm3_is_destroy.restype = None
        _bound = True
    return L


def _check(r: int, what: str):
    if r != 0:
        msg = host_lib().bcm3_last_error()
        raise RuntimeError(f"{what} failed ({r}): {msg.decode() if msg else ''}")


# ---- the kernels and the host restatement of the filter ----

def is_draw(n, d, kind, p0, p1, p2, g0, seed, values, lprior, stream=None):
    """bcm3hip_is_draw on device pointers (ints): draws g0 .. g0 + n - 1 of the prior."""
    _hip.check(_kernels().bcm3hip_is_draw(n, d, kind, p0, p1, p2, _hip._u64(g0), _hip._u64(seed), values, lprior,
                                          stream), "is_draw")


def is_filter(n, d, llh, values, lprior, learning_rate, limit, state, out_values, out_lprior, out_llh, out_weight,
              stream=None):
    """bcm3hip_is_filter on device pointers (ints); state: a device bcm3hip_is_state (STATE_DTYPE)."""
    _hip.check(_kernels().bcm3hip_is_filter(n, d, llh, values, lprior, learning_rate, limit, state, out_values,
                                            out_lprior, out_llh, out_weight, stream), "is_filter")


def is_filter_host(llh, values, lprior, learning_rate: float, limit: int, state: Optional[ISState] = None, out=None):
    """bcm3hip_is_filter_host: the filter's rule as a sequential loop on numpy arrays, no device. llh
    [n], values [n, d], lprior [n] are the next batch; state and out (dict of values [limit, d], lprior,
    llh, weight [limit]) carry over from the previous batch (new ones when None). Returns (state, out);
    rows [0, state.kept) of out are filled."""
    ll = np.ascontiguousarray(llh, dtype=np.float64).reshape(-1)
    n = ll.size
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(n, -1) if n else np.zeros((0, 1))
    lp = np.ascontiguousarray(lprior, dtype=np.float64).reshape(n)
    d = v.shape[1] if out is None else out["values"].shape[1]
    if state is None:
        state = new_state()
    if out is None:
        out = dict(values=np.full((limit, d), np.nan), lprior=np.full(limit, np.nan), llh=np.full(limit, np.nan),
                   weight=np.full(limit, np.nan))
    _hip.check(_kernels().bcm3hip_is_filter_host(n, d, ll.ctypes.data, v.ctypes.data, lp.ctypes.data, learning_rate,
                                                 limit, C.byref(state), out["values"].ctypes.data,
                                                 out["lprior"].ctypes.data, out["llh"].ctypes.data,
                                                 out["weight"].ctypes.data), "is_filter_host")
    return state, out


# ---- config.txt ----

def load_is_config(path: str) -> dict:
    """config.txt through bcm3_is_config_from_file: {"seed", "learning_rate", "batch", "num_samples",
    "prior", "likelihood", "output_folder", "likelihood_options", ...}; raises RuntimeError with the
    reader's message for a file it refuses (sampler.type other than is / importance_sampling,
    sampler.use_every_nth != 1, and everything bcm3_run_config_from_file's parser refuses)."""
    _kernels()
    rc = ISRunConfig()
    _check(host_lib().bcm3_is_config_from_file(path.encode(), C.byref(rc)), "bcm3_is_config_from_file")
    out = {"seed": rc.is_.seed, "learning_rate": rc.is_.learning_rate, "batch": rc.is_.batch}
    for k, _ in ISRunConfig._fields_:
        if k == "is_":
            continue
        v = getattr(rc, k)
        out[k] = v.decode() if isinstance(v, bytes) else v
    return out


# ---- the sampler ----

class ImportanceSampler:
    """bcm3_is_*: the importance sampler on the likelihood's device."""

    def __init__(self, likelihood: Likelihood, prior_xml: str, seed: int, learning_rate: float = 1.0,
                 batch: int = 1024):
        _kernels()
        cfg = ISConfig(int(seed) & ((1 << 64) - 1), float(learning_rate), int(batch))
        self.ll = likelihood  # keeps the likelihood alive
        self.d = likelihood.d
        h = C.c_void_p()
        _check(host_lib().bcm3_is_create(likelihood.h, prior_xml.encode(), C.byref(cfg), C.byref(h)), "bcm3_is_create")
        self.h = h

    def set_output(self, filename: str):
        """run() then writes its samples to `filename` (the reference's output.nc schema: one
        temperature, 1.0; weights = exp(log likelihood))."""
        _check(host_lib().bcm3_is_set_output(self.h, filename.encode()), "bcm3_is_set_output")

    def run(self, num_samples: int):
        """Draw until num_samples draws are kept; raises on a NaN log likelihood."""
        _check(host_lib().bcm3_is_run(self.h, int(num_samples)), "bcm3_is_run")

    def samples(self) -> dict:
        """The last run's samples: values [N, d], lprior, llh (times the learning rate), weight [N]."""
        n = host_lib().bcm3_is_num_samples(self.h)
        out = dict(values=np.empty((n, self.d)), lprior=np.empty(n), llh=np.empty(n), weight=np.empty(n))
        _check(host_lib().bcm3_is_get_samples(self.h, out["values"].ctypes.data, out["lprior"].ctypes.data,
                                              out["llh"].ctypes.data, out["weight"].ctypes.data), "bcm3_is_get_samples")
        return out

    def counters(self) -> dict:
        ev, kept, mx, ess = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        _check(host_lib().bcm3_is_get_counters(self.h, C.byref(ev), C.byref(kept), C.byref(mx), C.byref(ess)),
               "bcm3_is_get_counters")
        return dict(draws_evaluated=ev.value, draws_kept=kept.value, highest_log_weight=mx.value,
                    effective_sample_size=ess.value)

    def close(self):
        if getattr(self, "h", None):
            host_lib().bcm3_is_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_is(config_path: str, device: int = -1, batch: int = 1024) -> dict:
    """What `bcminf run` does for sampler.type = is: the likelihood and the prior of config.txt (paths
    relative to the file), the sampler, and <output.folder>/output.nc. Returns the samples and
    counters."""
    cfg = load_is_config(config_path)
    base = os.path.dirname(os.path.abspath(config_path))
    prior = os.path.join(base, cfg["prior"])
    ll = Likelihood(os.path.join(base, cfg["likelihood"]), prior, device=device,
                    options=cfg["likelihood_options"] or None)
    s = None
    try:
        s = ImportanceSampler(ll, prior, cfg["seed"], learning_rate=cfg["learning_rate"], batch=batch)
        folder = os.path.join(base, cfg["output_folder"])
        os.makedirs(folder, exist_ok=True)
        s.set_output(os.path.join(folder, "output.nc"))
        s.run(cfg["num_samples"])
        return dict(samples=s.samples(), counters=s.counters(), output=os.path.join(folder, "output.nc"))
    finally:
        if s is not None:
            s.close()
        ll.close()
