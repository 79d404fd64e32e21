"""Shared cases of the periodicity tests (tests/test_rfi_periodic.py on the emulator, tests/test_gpu_rfi_periodic.py on the
device): the grid, the known-answer tone, the kernel rule restated from outside, and thin callers of the C ABI.  Expected
values are tests/rfi_periodic_oracle.py on the same rows, computed once per case and never written to."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import _lib, post
from tests import rfi_cases as rc
from tests import rfi_oracle as ro
from tests import rfi_periodic_oracle as po

FAST, GENERIC = 1, 0
PEAK = po.PEAK


def fast_expected(nchan, nifs, nbits, address, n):
    """the documented rule: the clauses of the fast statistics kernel, and n = 256 .. 2048"""
    return FAST if rc.fast_expected(nchan, nifs, nbits, address) == rc.FAST and n in (256, 512, 1024, 2048) else GENERIC


def fparams(t_pow, chan_frac=0.3):
    f = _lib.FrbchRfiFparams()
    f.size = C.sizeof(_lib.FrbchRfiFparams)
    f.t_pow, f.chan_frac = float(t_pow), float(chan_frac)
    return f


# ---- the grid ----------------------------------------------------------------------------------------------------------
GRID_N = (8, 64, 256, 4096)


def grid():
    """(nchan, nbits, nifs, product, n, nrows): 33 (a lone last channel) / 48 / 64 channels x 8 / 16 / 32 bits x (one product,
    the last of three) x every n, with nrows one short of (a last block with 2 n_b >= n: tested), equal to and one past (a
    last block of one row: not tested) a multiple of n spread over the rest"""
    out = []
    k = 0
    for nchan in (33, 48, 64):
        for nbits in (8, 16, 32):
            for nifs, prod in ((1, 0), (3, 2)):
                for n in GRID_N:
                    nrows = (1 if n == 4096 else 3) * n + (-1, 0, 1)[k % 3]
                    out.append((nchan, nbits, nifs, prod, n, nrows))
                    k += 1
    return out


def grid_id(g):
    return "c%d_b%d_if%d_p%d_n%d_r%d" % g


@functools.lru_cache(maxsize=None)
def rows_case(nchan, nbits, nifs, prod, n, nrows, seed=None):
    """-> (rows, oracle stats of the product, oracle peaks)"""
    rows = rc.make_rows(nrows, nifs, nchan, nbits, seed=nchan + nbits + n if seed is None else seed)
    rows.setflags(write=False)
    st = ro.stats(rows[:, prod, :], n)
    pk = po.peaks(rows[:, prod, :], st, n)
    st.setflags(write=False)
    pk.setflags(write=False)
    return rows, st, pk


def same_peaks(got, want):
    return got.dtype == PEAK and got.shape == want.shape and got.tobytes() == want.tobytes()


# ---- the known answer: a weak tone the cell test on mean and std does not see ----------------------------------------------
KA_TONE = dict(channel=23, blocks=(5, 6, 7, 8), period=8, amp_sigma=0.7, sigma=16.0, t_freq=4.0)
KA_ALL_CHANNEL = 41            # known_answer_rows(all_blocks=True): the tone in every block of this channel as well


@functools.lru_cache(maxsize=None)
def known_answer_rows(seed=0, all_blocks=False):
    """the noise of rfi_cases.ka_noise (N(96, 16), 64 channels, blocks of 256) with a sine of 0.7 sigma amplitude and a period
    of 8 rows in channel 23 over the four blocks 5 .. 8 -- bin k = 256 / 8 = 32 -- quantised to 8 bit"""
    _rng, x = rc.ka_noise(seed)
    t = np.arange(rc.KA_NROWS)
    tone = KA_TONE["amp_sigma"] * KA_TONE["sigma"] * np.sin(2.0 * np.pi * t / KA_TONE["period"])
    b0, b1 = KA_TONE["blocks"][0], KA_TONE["blocks"][-1] + 1
    x[b0 * rc.KA_BLOCK: b1 * rc.KA_BLOCK, KA_TONE["channel"]] += tone[b0 * rc.KA_BLOCK: b1 * rc.KA_BLOCK]
    if all_blocks:
        x[:, KA_ALL_CHANNEL] += tone
    q = rc.ka_quantise(x)
    q.setflags(write=False)
    return q


def ka_t_pow():
    return po.t_pow_of(KA_TONE["t_freq"], rc.KA_BLOCK)


# ---- callers of the C ABI --------------------------------------------------------------------------------------------------
def peaks_host(lib, rows, prod, par, want_stats=True):
    """frbch_rfi_peaks_host -> (rc, peaks, stats, (statistics kernel, peaks kernel), message)"""
    nblk = max(1, rc.nblk_of(lib, rows.shape[0], par.block_rows))
    st = np.zeros((nblk, rows.shape[2], 2), dtype=rc.stats_dtype(rows))
    pk = np.full((nblk, rows.shape[2]), 7, dtype=np.uint64).view(PEAK)
    used = (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    code = lib.frbch_rfi_peaks_host(C.byref(rc.desc_of(rows, prod)), rows.ctypes.data, rows.shape[0], C.byref(par), 0,
                                    st.ctypes.data if want_stats else None, pk.ctypes.data, used, err, len(err))
    return code, pk, st, (used[0], used[1]), err.value.decode()


def periodic_call(lib, st, pk, nrows, nifs, nbits, prod, par, fpar, nblk=None, want_power=True):
    """frbch_rfi_periodic -> (rc, dict(pflag, pchan, power), message)"""
    st, pk = np.ascontiguousarray(st), np.ascontiguousarray(pk)
    nchan = st.shape[1]
    pflag, pchan, power = np.full(st.shape[:2], 9, np.uint8), np.full(nchan, 9, np.uint8), np.full(st.shape[:2], -1.0)
    err = C.create_string_buffer(512)
    desc = post.fil_desc(rc.hdr_of(nchan, nifs, nbits), product=prod)
    code = lib.frbch_rfi_periodic(C.byref(desc), st.ctypes.data, pk.ctypes.data, st.shape[0] if nblk is None else nblk, nrows, C.byref(par),
                                  C.byref(fpar), pflag.ctypes.data, pchan.ctypes.data, power.ctypes.data if want_power else None, err, len(err))
    return code, dict(pflag=pflag, pchan=pchan.astype(bool), power=power), err.value.decode()


def cleanf_host(lib, rows, prod, par, fpar, zap=None, want_peaks=True):
    """frbch_rfi_cleanf_host on a copy -> (rc, the copy, dict(mask, repl, chan_flag, blk_flag, pflag, pchan, peaks), used[2], message)"""
    out = np.array(rows, copy=True)
    nblk = max(1, rc.nblk_of(lib, rows.shape[0], par.block_rows))
    nchan = rows.shape[2]
    z = None if zap is None else np.ascontiguousarray(zap, dtype=np.uint8)
    m, repl = np.full((nblk, nchan), 9, np.uint8), np.full(nchan, -1.0)
    cf, bf = np.full(nchan, 9, np.uint8), np.full(nblk, 9, np.uint8)
    pflag, pchan = np.full((nblk, nchan), 9, np.uint8), np.full(nchan, 9, np.uint8)
    pk = np.full((nblk, nchan), 7, dtype=np.uint64).view(PEAK)
    used = (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    code = lib.frbch_rfi_cleanf_host(C.byref(rc.desc_of(rows, prod)), out.ctypes.data, out.shape[0], C.byref(par), C.byref(fpar),
                                     None if z is None else z.ctypes.data, 0, m.ctypes.data, repl.ctypes.data, cf.ctypes.data,
                                     bf.ctypes.data, pflag.ctypes.data, pchan.ctypes.data, pk.ctypes.data if want_peaks else None,
                                     used, err, len(err))
    res = dict(mask=m, repl=repl, chan_flag=cf.astype(bool), blk_flag=bf.astype(bool), pflag=pflag, pchan=pchan.astype(bool), peaks=pk)
    return code, out, res, (used[0], used[1]), err.value.decode()


def sequence_of_parts(rows, prod, n, nbits, rule, t_pow, chan_frac, zap=None):
    """what frbch_rfi_cleanf_* must return, from the restatements: statistics, peaks, the periodic decision, the mask with it as
    prior, the cleaned rows -> (dict as cleanf_host's, cleaned rows)"""
    x = rows[:, prod, :]
    st = ro.stats(x, n)
    pk = po.peaks(x, st, n)
    dec = po.periodic(st, pk, rows.shape[0], n, t_pow, chan_frac)
    res = ro.mask(st, rows.shape[0], n, nbits, zap=zap, prior=dec["pflag"], **rule)
    cleaned = ro.apply(rows, prod, n, res["mask"], res["repl"])
    return dict(mask=res["mask"], repl=res["repl"], chan_flag=res["chan_flag"] | dec["pchan"], blk_flag=res["blk_flag"],
                pflag=dec["pflag"], pchan=dec["pchan"], peaks=pk, stats=st, power=dec["power"]), cleaned


def same_cleanf(got, want):
    return (rc.same_result(got, want) and np.array_equal(got["pflag"], want["pflag"]) and np.array_equal(got["pchan"], want["pchan"])
            and same_peaks(got["peaks"], want["peaks"]))


# ---- timing (tools/rfi_profile.py) -------------------------------------------------------------------------------------------
def timing_run(lib, d_rows, rounds=5):
    """10 s x 1024 channels of 8-bit rows resident at `d_rows` (16-byte aligned, with one spare byte behind the rows), blocks
    of 1024: after a warm-up of each, the median of `rounds` calls of frbch_rfi_peaks_device with the fast kernel, with the
    generic kernel (the same rows copied one byte further on), of frbch_rfi_stats_device, frbch_rfi_cleanf_device and
    frbch_rfi_clean_device -> dict"""
    import statistics
    import time
    from tests.hipmem import GuardedBuffer as DeviceBuffer, hip
    desc = post.fil_desc(rc.TIMING_HDR)
    par = rc.params()
    fpar = fparams(po.t_pow_of(4.0, par.block_rows))
    nrows, nchan = rc.TIMING_ROWS, rc.TIMING_NCHAN
    nblk = lib.frbch_rfi_nblk(nrows, par.block_rows)
    d_stats, d_peaks = DeviceBuffer(nblk * nchan * 16), DeviceBuffer(nblk * nchan * 8)
    shifted = DeviceBuffer(nrows * nchan + 16)
    d_shift = C.c_void_p(shifted.ptr.value + 1)
    assert hip().hipMemcpy(d_shift, C.c_void_p(d_rows), nrows * nchan, 3) == 0
    m, repl = np.zeros((nblk, nchan), np.uint8), np.zeros(nchan)
    cf, bf = np.zeros(nchan, np.uint8), np.zeros(nblk, np.uint8)
    pflag, pchan = np.zeros((nblk, nchan), np.uint8), np.zeros(nchan, np.uint8)
    err = C.create_string_buffer(256)
    used, used2 = C.c_uint32(99), (C.c_uint32 * 2)(99, 99)
    kernels = {}

    def timed(name, fn):
        def run():
            t0 = time.perf_counter()
            code = fn()
            dt = time.perf_counter() - t0
            assert code == 0, err.value
            return dt
        run()
        kernels[name] = (used.value, used2[0], used2[1])
        return [run() for _ in range(rounds)]

    out = {"rows": nrows, "nchan": nchan, "nbits": 8, "block_rows": int(par.block_rows), "nblk": int(nblk)}
    runs = [
        ("rfi_stats_device", lambda: lib.frbch_rfi_stats_device(C.byref(desc), C.c_void_p(d_rows), nrows, C.byref(par), 0, d_stats.ptr,
                                                                C.byref(used), err, len(err))),
        ("rfi_peaks_device_fast", lambda: lib.frbch_rfi_peaks_device(C.byref(desc), C.c_void_p(d_rows), nrows, C.byref(par), 0, d_stats.ptr,
                                                                     d_peaks.ptr, C.byref(used), err, len(err))),
        ("rfi_peaks_device_generic", lambda: lib.frbch_rfi_peaks_device(C.byref(desc), d_shift, nrows, C.byref(par), 0, d_stats.ptr,
                                                                        d_peaks.ptr, C.byref(used), err, len(err))),
        ("rfi_clean_device", lambda: lib.frbch_rfi_clean_device(C.byref(desc), C.c_void_p(d_rows), nrows, C.byref(par), None, 0,
                                                                m.ctypes.data, repl.ctypes.data, cf.ctypes.data, bf.ctypes.data,
                                                                C.byref(used), err, len(err))),
        ("rfi_cleanf_device", lambda: lib.frbch_rfi_cleanf_device(C.byref(desc), C.c_void_p(d_rows), nrows, C.byref(par), C.byref(fpar),
                                                                  None, 0, m.ctypes.data, repl.ctypes.data, cf.ctypes.data, bf.ctypes.data,
                                                                  pflag.ctypes.data, pchan.ctypes.data, None, used2, err, len(err))),
    ]
    for name, fn in runs:
        t = timed(name, fn)
        out[name + "_median_s"] = statistics.median(t)
        out[name + "_each_s"] = [round(v, 6) for v in t]
    out["kernel_used"] = {"rfi_stats_device": kernels["rfi_stats_device"][0], "rfi_peaks_device_fast": kernels["rfi_peaks_device_fast"][0],
                          "rfi_peaks_device_generic": kernels["rfi_peaks_device_generic"][0],
                          "rfi_cleanf_device": list(kernels["rfi_cleanf_device"][1:])}
    out["periodic_cells_flagged"] = int(pflag.sum())
    for b in (d_stats, d_peaks, shifted):
        b.free()
    return out
