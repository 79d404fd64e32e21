"""Shared series of the periodicity-search tests (tests/test_psearch.py on the emulator, tests/test_gpu_psearch.py on the
device): a plain module of named cases -- (series [ndm][nout] float32, tsamp, keyword arguments of the search) -- and thin
callers of the C ABI.  Expected values are tests/psearch_oracle.py on the same series, computed once per case."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import _lib, post
from tests import psearch_oracle as pso
from tests.hipmem import guarded_for

TSAMP = 1e-3


def noise(ndm, nout, seed):
    rng = np.random.default_rng(seed)
    return (100.0 + 10.0 * rng.standard_normal((ndm, nout))).astype(np.float32)


def add_sine(y, dm, freq, amp, tsamp=TSAMP):
    t = np.arange(y.shape[1], dtype=np.float64) * tsamp
    y[dm] += (amp * np.sin(2.0 * np.pi * freq * t)).astype(np.float32)


def add_train(y, dm, period_samples, phase, amp):
    """one sample of `amp` every period_samples (not an integer: the nearest sample)"""
    t = np.round(phase + period_samples * np.arange(int(y.shape[1] / period_samples) + 1)).astype(np.int64)
    y[dm, t[t < y.shape[1]]] += np.float32(amp)


def signals(ndm, nout, seed, tsamp=TSAMP):
    """noise, a sine in the even series, a pulse train (narrow: sixteen harmonics and more) in the odd ones; every third series
    holds noise alone"""
    y = noise(ndm, nout, seed)
    for d in range(ndm):
        if d % 3 == 2:
            continue
        if d % 2 == 0:
            add_sine(y, d, 37.3 + 1.7 * d, 1.5, tsamp)
        else:
            add_train(y, d, 47.3 + d, 3.0 + d, 25.0)
    return y


def _smallest():
    return signals(2, 4096, 41), TSAMP, dict(sigma=4.0)


def _odd_ndm():
    return signals(3, 4096, 42), TSAMP, dict(sigma=4.0)


def _one_dm():
    y = noise(1, 4096, 43)
    add_train(y, 0, 51.7, 5.0, 25.0)
    return y, TSAMP, dict(sigma=4.0)


def _tail_ignored():
    y = signals(4, 5000, 44)
    y[:, 4096:] = np.float32(1.0e6)                        # beyond n: not even the mean may see it
    return y, TSAMP, dict(sigma=4.0)


def _nfft_given():
    y = signals(3, 9000, 45)                               # the automatic length would be 8192
    y[:, 4096:] = np.float32(-3.0e5)
    return y, TSAMP, dict(sigma=4.0, nfft=4096)


def _nharm(h):
    return lambda: (signals(5, 8192, 46), TSAMP, dict(sigma=4.0, nharm=h))


def _wblock(b):
    return lambda: (signals(4, 8192, 47), TSAMP, dict(sigma=4.0, wblock=b))


def _dead_partner():
    y = signals(4, 4096, 48)
    add_sine(y, 2, 91.1, 1.5)
    y[0, 1234] = np.nan                                   # series 0 is dead, its partner 1 lives
    y[3, 77] = np.inf                                      # series 3 is dead, its partner 2 lives
    return y, TSAMP, dict(sigma=4.0)


def _constant():
    y = signals(3, 4096, 49)
    y[1] = np.float32(7.0)                                 # every power 0, every level 0
    return y, TSAMP, dict(sigma=4.0)


def _high_flo():
    """n tsamp = 4.096 s: flo 40 Hz gives kmin = 164, and 16 x 164 > 2048: the fold of 16 has no bin"""
    y = noise(3, 4096, 50)
    add_train(y, 0, 11.3, 2.0, 25.0)                       # 88.5 Hz and its harmonics
    add_sine(y, 1, 301.7, 2.0)
    return y, TSAMP, dict(sigma=4.0, flo=40.0)


def _n14():
    return signals(3, 1 << 14, 51, 64e-6), 64e-6, dict(sigma=4.0)


CASES = {
    "smallest_2dm_4096": _smallest, "odd_3dm": _odd_ndm, "one_dm": _one_dm, "tail_ignored_nout_5000": _tail_ignored,
    "nfft_4096_of_9000": _nfft_given, "nharm_1": _nharm(1), "nharm_2": _nharm(2), "nharm_4": _nharm(4), "nharm_8": _nharm(8),
    "nharm_16": _nharm(16), "wblock_32": _wblock(32), "wblock_1024": _wblock(1024), "dead_beside_live": _dead_partner,
    "constant_series": _constant, "flo_40hz_no_fold_16": _high_flo, "two_pass_length_3dm": _n14,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (series, tsamp, kwargs, oracle records, oracle raw peaks); built once, never written to"""
    y, tsamp, kw = CASES[name]()
    y.setflags(write=False)
    want, raw = pso.search(y, tsamp, want_raw=True, **kw)
    want.setflags(write=False)
    return y, tsamp, kw, want, raw


def params_of(tsamp, sigma=6.0, nharm=0, flo=0.0, nfft=0, wblock=0):
    return post.ps_params(tsamp, sigma, nharm, flo, nfft, wblock)


def psearch_host(lib, y, tsamp, cap=8192, **kw):
    """frbch_psearch_host -> (rc, records written, ncand, (form, passes), message)"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    params = params_of(tsamp, **kw)
    cands = np.zeros(cap, dtype=post.PS_CAND)
    ncand, used = C.c_uint64(0), (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    rc = lib.frbch_psearch_host(y.ctypes.data, y.shape[0], y.shape[1], C.byref(params), 0, cands.ctypes.data if cap else None, cap,
                                C.byref(ncand), used, err, len(err))
    return rc, cands[: min(cap, ncand.value)], ncand.value, (used[0], used[1]), err.value.decode()


def device_search(lib, y, tsamp, misalign=False, cap=8192, **kw):
    """frbch_psearch_device on a guarded buffer of exactly ndm * nout floats (misalign: one float more, the series from its
    second float on) -> (records, (form, passes)); the input's checksum and both guard bands are checked behind the call.  The
    buffer is device memory for the product library and host memory for the emulator build, whose _device entry points take
    host pointers"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    held = np.concatenate([np.zeros(1, dtype=np.float32), y.reshape(-1)]) if misalign else y
    buf = guarded_for(lib).from_numpy(held)
    ptr = C.c_void_p(buf.ptr.value + (4 if misalign else 0))
    params = params_of(tsamp, **kw)
    npass = C.c_uint32(9)
    form = lib.frbch_psearch_kernel(ptr, y.shape[0], y.shape[1], C.byref(params), C.byref(npass))
    cands = np.zeros(cap, dtype=post.PS_CAND)
    ncand, used = C.c_uint64(0), (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    rc = lib.frbch_psearch_device(ptr, y.shape[0], y.shape[1], C.byref(params), 0, cands.ctypes.data, cap, C.byref(ncand), used, err, len(err))
    assert rc == 0, err.value
    buf.check(contents=True)
    buf.free()
    assert (used[0], used[1]) == (form, npass.value)
    return cands[: ncand.value], (used[0], used[1])


def same_records(got, want):
    """record for record: dm_index, h, k and the float bits of H exactly; sigma and freq_hz -- doubles behind the C library's
    exp, log and erfc -- to psearch_oracle.SIGMA_RTOL"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    for f in ("dm_index", "h", "k"):
        if not np.array_equal(got[f], want[f]):
            return False
    if got["power"].tobytes() != want["power"].tobytes():
        return False
    return bool(np.all(np.abs(got["sigma"] - want["sigma"]) <= pso.SIGMA_RTOL * np.abs(want["sigma"])) and
                np.all(np.abs(got["freq_hz"] - want["freq_hz"]) <= pso.SIGMA_RTOL * np.abs(want["freq_hz"])))


def same_groups(got, want):
    return (got.shape == want.shape and same_records(got["best"], want["best"]) and
            all(np.array_equal(got[f], want[f]) for f in ("nmember", "dm_index_lo", "dm_index_hi")))
