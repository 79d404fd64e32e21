"""Shared cases of the acceleration-search tests (tests/test_accel.py on the emulator, tests/test_gpu_accel.py on the device):
named cases -- (series [ndm][nout] float32, tsamp, trial accelerations, keyword arguments of the search) -- and thin callers of
the C ABI.  Expected values are tests/accel_oracle.py on the same series, computed once per case."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import post
from tests import accel_oracle as ao
from tests import psearch_cases as pc
from tests import psearch_oracle as pso
from tests.hipmem import guarded_for

TSAMP = pc.TSAMP
A12 = 3.0e7           # m/s^2 at n = 2^12, tsamp 1 ms: q n = 0.205 (the largest accepted is c / (n tsamp) = 7.3e7)
A14 = 1.0e8           # at n = 2^14, tsamp 64 us: q n = 0.175
S12, S14 = 2.0e5, 5.0e6   # small trials: the 37 Hz sine of pc.signals moves by less than a bin, so every trial has records


def edge(n, tsamp):
    """the acceleration whose q n is 0.5 EXACTLY in the library's arithmetic: the doubles next to c / (n tsamp) are tried"""
    a = ao.C_LIGHT / (n * tsamp)
    for cand in [a] + [f(a, k) for k in range(1, 65) for f in (_up, _down)]:
        if ao.q_of(cand, tsamp) * float(n) == 0.5:
            return cand
    raise AssertionError("no double gives q n = 0.5 at n = %d, tsamp = %g" % (n, tsamp))


def _up(a, k):
    for _ in range(k):
        a = np.nextafter(a, np.inf)
    return float(a)


def _down(a, k):
    for _ in range(k):
        a = np.nextafter(a, -np.inf)
    return float(a)


def just_above(n, tsamp):
    """the first double beyond the range"""
    a = edge(n, tsamp)
    while ao.accepted(a, n, tsamp):
        a = float(np.nextafter(a, np.inf))
    return a


def _2x3():
    return pc.signals(2, 4096, 141), TSAMP, [-S12, 0.0, S12], dict(sigma=4.0)


def _3x2():
    return pc.signals(3, 4096, 142), TSAMP, [0.0, S12], dict(sigma=3.0)   # (3: the third series is noise alone)


def _1x5():
    y = pc.noise(1, 4096, 143)
    pc.add_train(y, 0, 51.7, 5.0, 25.0)
    return y, TSAMP, [-A12, -S12, 0.0, S12, A12], dict(sigma=3.0)


def nan_position():
    """a sample that the gather of trial +A12 skips (u steps by 2 over it) and every other trial of the case reaches"""
    u = set(ao.index(4096, A12, TSAMP).tolist())
    v = set(ao.index(4096, -A12, TSAMP).tolist())
    return min(t for t in range(4096) if t not in u and t in v)


def _nan():
    y = pc.signals(4, 4096, 144)
    y[1, nan_position()] = np.nan
    return y, TSAMP, [-A12, 0.0, A12], dict(sigma=3.0)


def _constant():
    y = pc.signals(3, 4096, 145)
    y[1] = np.float32(7.0)
    return y, TSAMP, [-S12, S12], dict(sigma=4.0)


def _tail():
    y = pc.signals(3, 5000, 146)
    y[:, 4096:] = np.float32(1.0e6)
    return y, TSAMP, [-A12, 0.0, S12], dict(sigma=3.0)


def _edges():
    e = edge(4096, TSAMP)
    return pc.signals(2, 4096, 147), TSAMP, [-e, e], dict(sigma=3.0)


def _n14():
    return pc.signals(3, 1 << 14, 148, 64e-6), 64e-6, [-S14, S14], dict(sigma=4.0)


CASES = {
    "2dm_3trials_4096": _2x3, "odd_3dm_2trials": _3x2, "1dm_5trials": _1x5, "nan_reached_by_some_trials": _nan,
    "constant_series": _constant, "tail_ignored_nout_5000": _tail, "trials_at_both_edges": _edges, "two_pass_length_3dm": _n14,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (series, tsamp, accs float64 array, kwargs, oracle records); built once, never written to"""
    y, tsamp, accs, kw = CASES[name]()
    y.setflags(write=False)
    accs = np.ascontiguousarray(accs, dtype=np.float64)
    accs.setflags(write=False)
    want = ao.search(y, tsamp, accs, **kw)
    want.setflags(write=False)
    return y, tsamp, accs, kw, want


# ---- the chirped sine of the issue: found only with the feature ----------------------------------------------------------
CHIRP_N, CHIRP_TSAMP, CHIRP_NU, CHIRP_A0, CHIRP_SEED = 1 << 14, 1e-3, 0.0373, 365957.59, 7
CHIRP_ACCS = np.array([-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5]) * CHIRP_A0


@functools.lru_cache(maxsize=None)
def chirp():
    """2^14 samples of 1 ms, noise of sigma 10 around 100, a sine of amplitude 4 whose phase is nu (t - q t^2) cycles: it starts
    at 0.0373 cycles per sample and falls by 12 bins"""
    q = ao.q_of(CHIRP_A0, CHIRP_TSAMP)
    t = np.arange(CHIRP_N, dtype=np.float64)
    y = pc.noise(1, CHIRP_N, CHIRP_SEED)
    y[0] += (4.0 * np.sin(2.0 * np.pi * CHIRP_NU * (t - q * t * t))).astype(np.float32)
    y.setflags(write=False)
    return y


def chirp_checks(groups, records):
    """the three assertions of the issue on the groups and records of a search of chirp() with CHIRP_ACCS at sigma 3"""
    q = ao.q_of(CHIRP_A0, CHIRP_TSAMP)
    best = groups[0]["best"]
    zero = records[records["acc_index"] == 3]
    assert zero.size > 0
    ratio = float(best["sigma"]) / float(zero["sigma"].max())
    print("chirp: best sigma %.2f at a = %.6g, f = %.6f Hz; trial 0 best %.2f; ratio %.2f" %
          (best["sigma"], best["acc_ms2"], best["freq_hz"], zero["sigma"].max(), ratio))
    assert float(best["acc_ms2"]) == CHIRP_A0
    assert abs(float(best["freq_hz"]) - CHIRP_NU * (1.0 - q * CHIRP_N) / CHIRP_TSAMP) <= 1.0 / (CHIRP_N * CHIRP_TSAMP)
    assert ratio >= 3.0


# ---- callers ----------------------------------------------------------------------------------------------------------
def pasearch_host(lib, y, tsamp, accs, cap=8192, batch_rows=0, nacc=None, **kw):
    """frbch_pasearch_host -> (rc, records written, ncand, (resampler, form, passes), message)"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    accs = np.ascontiguousarray(accs, dtype=np.float64)
    params = pc.params_of(tsamp, **kw)
    cands = np.zeros(cap, dtype=post.PA_CAND)
    ncand, used = C.c_uint64(0), (C.c_uint32 * 3)(99, 99, 99)
    err = C.create_string_buffer(512)
    rc = lib.frbch_pasearch_host(y.ctypes.data, y.shape[0], y.shape[1], C.byref(params), accs.ctypes.data,
                                 accs.size if nacc is None else nacc, batch_rows, 0, cands.ctypes.data if cap else None, cap,
                                 C.byref(ncand), used, err, len(err))
    return rc, cands[: min(cap, ncand.value)], ncand.value, (used[0], used[1], used[2]), err.value.decode()


def held(lib, y, misalign):
    """-> (guarded buffer, pointer to the series): misalign puts one float in front, so that the series is 4-byte aligned only.
    Device memory for the product library, host memory for the emulator build"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    buf = guarded_for(lib).from_numpy(np.concatenate([np.zeros(1, dtype=np.float32), y.reshape(-1)]) if misalign else y)
    return buf, C.c_void_p(buf.ptr.value + (4 if misalign else 0))


def device_search(lib, y, tsamp, accs, misalign=False, cap=8192, batch_rows=0, **kw):
    """frbch_pasearch_device on a guarded buffer of exactly ndm * nout floats -> (records, (resampler, form, passes)); the
    input's checksum and both guard bands are checked behind the call"""
    accs = np.ascontiguousarray(accs, dtype=np.float64)
    buf, ptr = held(lib, y, misalign)
    params = pc.params_of(tsamp, **kw)
    cands = np.zeros(cap, dtype=post.PA_CAND)
    ncand, used = C.c_uint64(0), (C.c_uint32 * 3)(99, 99, 99)
    err = C.create_string_buffer(512)
    rc = lib.frbch_pasearch_device(ptr, y.shape[0], y.shape[1], C.byref(params), accs.ctypes.data, accs.size, batch_rows, 0,
                                   cands.ctypes.data, cap, C.byref(ncand), used, err, len(err))
    assert rc == 0, err.value
    buf.check(contents=True)
    buf.free()
    return cands[: ncand.value], (used[0], used[1], used[2])


def same_records(got, want):
    """record for record: the integers and the float bits of H exactly, acc_ms2 exactly (it is the caller's number); sigma and
    freq_hz to psearch_oracle.SIGMA_RTOL"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    for f in ("dm_index", "acc_index", "h", "k", "acc_ms2"):
        if not np.array_equal(got[f], want[f]):
            return False
    if got["power"].tobytes() != want["power"].tobytes():
        return False
    return bool(np.all(np.abs(got["sigma"] - want["sigma"]) <= pso.SIGMA_RTOL * np.abs(want["sigma"])) and
                np.all(np.abs(got["freq_hz"] - want["freq_hz"]) <= pso.SIGMA_RTOL * np.abs(want["freq_hz"])))


def same_groups(got, want):
    return (got.shape == want.shape and same_records(got["best"], want["best"]) and
            all(np.array_equal(got[f], want[f]) for f in ("nmember", "dm_index_lo", "dm_index_hi", "acc_index_lo", "acc_index_hi")))
