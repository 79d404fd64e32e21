"""Shared cases of the interference tests (tests/test_rfi.py on the emulator, tests/test_gpu_rfi.py on the device): rows whose
products all differ, the known-answer case, the kernel rule restated from outside, and thin callers of the C ABI.  Expected
values are tests/rfi_oracle.py on the same rows, computed once per case and never written to."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import _lib, post
from tests import rfi_oracle as ro

FAST, GENERIC = 1, 0
DTYPES = {8: np.uint8, 16: np.uint16, 32: np.float32}
DEFAULTS = dict(block_rows=1024, t_cell=5.0, t_chan=5.0, chan_frac=0.3, block_frac=0.3)
HDR_KEYS = dict(fch1=1416.0, foff=-0.03125, tsamp=32e-6, tstart=59000.25)


def hdr_of(nchan, nifs, nbits):
    return dict(HDR_KEYS, nchans=nchan, nifs=nifs, nbits=nbits)


def params(**kw):
    return post.rfi_params(dict(DEFAULTS, **kw))


def fast_expected(nchan, nifs, nbits, address):
    """the documented rule: 8- / 16-bit rows, the row piece whole 64-byte channel tiles, the address of the rows and the row
    pitch nifs * nchan * bytes-per-sample 16-byte aligned"""
    bpv = nbits // 8
    return FAST if nbits in (8, 16) and (nchan * bpv) % 64 == 0 and address % 16 == 0 and (nifs * nchan * bpv) % 16 == 0 else GENERIC


def tile_bytes(nchan, nbits):
    """the fast kernel's tile: the largest listed width that divides the row piece"""
    return next(w for w in (1024, 512, 256, 128, 64) if (nchan * nbits // 8) % w == 0)


# ---- rows -----------------------------------------------------------------------------------------------------------
def make_rows(nrows, nifs, nchan, nbits, seed=1):
    """[t][nifs][nchan] rows in which every product has its own level, width and seed (as tests/post_cases.py), a loud
    channel and a broadband burst of its own: a kernel that reads another product, or another row pitch, sums other codes"""
    x = np.empty((nrows, nifs, nchan), dtype=np.float64)
    for p in range(nifs):
        rng = np.random.default_rng(1000 * seed + p)
        x[:, p, :] = rng.integers(40 + 15 * p, 40 + 15 * p + 24 + 8 * p, size=(nrows, nchan))
        x[:, p, (7 + 5 * p) % nchan] += 30 + p
        r0 = int(nrows * (0.3 + 0.1 * p))
        x[r0: r0 + 2 + p, p, :] += 50
    if nbits == 8:
        return x.astype(np.uint8)
    if nbits == 16:
        return (x * 201).astype(np.uint16)
    return (x * 0.37 - 3.0).astype(np.float32)


GRID_BLOCK_ROWS = (1, 7, 256, 5000)              # 5000: larger than any nrows of the grid


def grid():
    """(nchan, nbits, nifs, product, block_rows, nrows): 48 / 64 / 128 channels x 8 / 16 / 32 bits, one product and the last of
    three, every block length, with nrows one short of, equal to and one past a multiple of block_rows spread over the rest"""
    out = []
    k = 0
    for nchan in (48, 64, 128):
        for nbits in (8, 16, 32):
            for nifs, prod in ((1, 0), (3, 2)):
                for br in GRID_BLOCK_ROWS:
                    mult = {1: 5, 7: 21, 256: 512, 5000: 300}[br]
                    nrows = mult + (-1, 0, 1)[k % 3] if br != 5000 else 300 + k % 3
                    out.append((nchan, nbits, nifs, prod, br, nrows))
                    k += 1
    return out


def grid_id(g):
    return "c%d_b%d_if%d_p%d_br%d_n%d" % g


@functools.lru_cache(maxsize=None)
def grid_case(g):
    """-> (rows, oracle stats of the product, oracle mask result with the defaults and t_cell 3, cleaned rows)"""
    nchan, nbits, nifs, prod, br, nrows = g
    rows = make_rows(nrows, nifs, nchan, nbits, seed=nchan + nbits + br)
    rows.setflags(write=False)
    st = ro.stats(rows[:, prod, :], br)
    res = ro.mask(st, nrows, br, nbits, **dict(rule_kw(DEFAULTS), t_cell=3.0))
    cleaned = ro.apply(rows, prod, br, res["mask"], res["repl"])
    for a in (st, cleaned, res["mask"], res["repl"]):
        a.setflags(write=False)
    return rows, st, res, cleaned


def rule_kw(par):
    return {k: v for k, v in par.items() if k != "block_rows"}


# ---- the known answer --------------------------------------------------------------------------------------------------
KA_NCHAN, KA_BLOCK, KA_NROWS = 64, 256, 24 * 256 - 100
KA_ZAP = (0, 1, 63)
KA_CHANNELS, KA_BLOCKS, KA_CELLS = [0, 1, 5, 20, 33, 63], [7], [(12, 40)]


def ka_noise(seed):
    """floor(N(96, 16) + 1/2) clipped to 8 bit comes from this: (the generator after the draw, the float rows)"""
    rng = np.random.default_rng(seed)
    return rng, 96.0 + 16.0 * rng.standard_normal((KA_NROWS, KA_NCHAN))


def ka_quantise(x):
    return np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def known_answer_rows(seed=0):
    """the noise with the injected interference: channel 5 gets +40 sin^2(t / 300) on a random half of the rows, rows
    7 * 256 + 10 .. 7 * 256 + 199 get +30 in all channels, channel 40 gets +120 on rows 12 * 256 + 3 .. 12 * 256 + 39, channel 20
    is constant at 96, channel 33 is N(96, 40)"""
    rng, x = ka_noise(seed)
    t = np.arange(KA_NROWS)
    half = rng.random(KA_NROWS) < 0.5
    x[half, 5] += 40.0 * np.sin(t[half] / 300.0) ** 2
    x[7 * 256 + 10: 7 * 256 + 200, :] += 30.0
    x[12 * 256 + 3: 12 * 256 + 40, 40] += 120.0
    x[:, 33] = 96.0 + 40.0 * rng.standard_normal(KA_NROWS)
    q = ka_quantise(x)
    q[:, 20] = 96
    q.setflags(write=False)
    return q


def ka_zap():
    z = np.zeros(KA_NCHAN, dtype=bool)
    z[list(KA_ZAP)] = True
    return z


def other_cells(res):
    """masked cells outside the wholly flagged channels and blocks"""
    m = res["mask"].astype(bool) & ~np.asarray(res["chan_flag"], bool)[None, :] & ~np.asarray(res["blk_flag"], bool)[:, None]
    return [tuple(int(v) for v in bc) for bc in np.argwhere(m)]


# ---- the end-to-end file: the burst of tests/test_spsearch.py with an intermittent channel and one broadband block -----
E2E = dict(nrows=9000, t0=3000, width=6, amp=30, dm_lo_off=-10.0, dm_hi_off=10.0, dmstep=5.0, threshold=6.0, max_width_s=0.01, block_rows=256,
           loud_channel=11, loud_amp=95, loud_rows=((1200, 1350), (5300, 5450), (7000, 7150)), broad_rows=(8500, 8600), broad_amp=60, zerodm=False)
# (one channel of 64 reaches 6 sigma in the band sum only over about a hundred rows, 95 w / (148 sqrt(w)): hence the wide boxcars;
# the zero-DM filter would take it out again, so the case runs without; the broadband rows are what -clip catches)


def e2e_rows(with_rfi):
    from tests.test_post import DM0, HDR
    from tests.test_spsearch import dispersed_burst_rows
    x = dispersed_burst_rows(E2E["nrows"], HDR, DM0, E2E["t0"], E2E["width"], E2E["amp"]).astype(np.int64)
    if with_rfi:
        for a, b in E2E["loud_rows"]:
            x[a:b, E2E["loud_channel"]] += E2E["loud_amp"]
        a, b = E2E["broad_rows"]
        x[a:b, :] += E2E["broad_amp"]
    return np.clip(x, 0, 255).astype(np.uint8)


# ---- callers of the C ABI ---------------------------------------------------------------------------------------------------
def desc_of(rows, prod=0):
    return post.fil_desc(hdr_of(rows.shape[2], rows.shape[1], rows.dtype.itemsize * 8), product=prod)


def stats_dtype(rows):
    return np.float64 if rows.dtype == np.float32 else np.uint64


def nblk_of(lib, nrows, block_rows):
    return lib.frbch_rfi_nblk(nrows, block_rows)


def stats_host(lib, rows, prod, par):
    """frbch_rfi_stats_host -> (rc, stats, kernel_used, message)"""
    nblk = max(1, nblk_of(lib, rows.shape[0], par.block_rows))
    st = np.zeros((nblk, rows.shape[2], 2), dtype=stats_dtype(rows))
    used = C.c_uint32(99)
    err = C.create_string_buffer(512)
    rc = lib.frbch_rfi_stats_host(C.byref(desc_of(rows, prod)), rows.ctypes.data, rows.shape[0], C.byref(par), 0, st.ctypes.data,
                                  C.byref(used), err, len(err))
    return rc, st, used.value, err.value.decode()


def mask_call(lib, st, nrows, nchan, nifs, nbits, prod, par, zap=None, prior=None, nblk=None):
    """frbch_rfi_mask -> (rc, dict(mask, repl, chan_flag, blk_flag), message)"""
    st = np.ascontiguousarray(st)
    nblk = st.shape[0] if nblk is None else nblk
    z = None if zap is None else np.ascontiguousarray(zap, dtype=np.uint8)
    pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.uint8)
    m, repl = np.full((st.shape[0], nchan), 9, np.uint8), np.full(nchan, -1.0)
    cf, bf = np.full(nchan, 9, np.uint8), np.full(st.shape[0], 9, np.uint8)
    err = C.create_string_buffer(512)
    desc = post.fil_desc(hdr_of(nchan, nifs, nbits), product=prod)
    rc = lib.frbch_rfi_mask(C.byref(desc), st.ctypes.data, nblk, nrows, C.byref(par), None if z is None else z.ctypes.data,
                            None if pr is None else pr.ctypes.data, m.ctypes.data, repl.ctypes.data, cf.ctypes.data, bf.ctypes.data,
                            err, len(err))
    return rc, dict(mask=m, repl=repl, chan_flag=cf.astype(bool), blk_flag=bf.astype(bool)), err.value.decode()


def apply_host(lib, rows, prod, par, m, repl):
    """frbch_rfi_apply_host on a copy -> (rc, the copy, message)"""
    out = np.array(rows, copy=True)
    m, repl = np.ascontiguousarray(m, dtype=np.uint8), np.ascontiguousarray(repl, dtype=np.float64)
    err = C.create_string_buffer(512)
    rc = lib.frbch_rfi_apply_host(C.byref(desc_of(rows, prod)), out.ctypes.data, out.shape[0], C.byref(par), m.ctypes.data,
                                  repl.ctypes.data, 0, err, len(err))
    return rc, out, err.value.decode()


def clean_host(lib, rows, prod, par, zap=None):
    """frbch_rfi_clean_host on a copy -> (rc, the copy, dict(mask, repl, chan_flag, blk_flag), kernel_used, message)"""
    out = np.array(rows, copy=True)
    nblk = max(1, nblk_of(lib, rows.shape[0], par.block_rows))
    nchan = rows.shape[2]
    z = None if zap is None else np.ascontiguousarray(zap, dtype=np.uint8)
    m, repl = np.full((nblk, nchan), 9, np.uint8), np.full(nchan, -1.0)
    cf, bf = np.full(nchan, 9, np.uint8), np.full(nblk, 9, np.uint8)
    used = C.c_uint32(99)
    err = C.create_string_buffer(512)
    rc = lib.frbch_rfi_clean_host(C.byref(desc_of(rows, prod)), out.ctypes.data, out.shape[0], C.byref(par),
                                  None if z is None else z.ctypes.data, 0, m.ctypes.data, repl.ctypes.data, cf.ctypes.data,
                                  bf.ctypes.data, C.byref(used), err, len(err))
    return rc, out, dict(mask=m, repl=repl, chan_flag=cf.astype(bool), blk_flag=bf.astype(bool)), used.value, err.value.decode()


def same_result(got, want):
    """mask, replacement values (to the bit), flagged channels and blocks"""
    return (np.array_equal(got["mask"], want["mask"]) and got["repl"].tobytes() == np.asarray(want["repl"], np.float64).tobytes()
            and np.array_equal(got["chan_flag"], want["chan_flag"]) and np.array_equal(got["blk_flag"], want["blk_flag"]))


# ---- timing (tests/test_gpu_rfi.py and tools/rfi_profile.py) -------------------------------------------------------------
TIMING_ROWS, TIMING_NCHAN = 312500, 1024
TIMING_HDR = dict(nchans=TIMING_NCHAN, nifs=1, nbits=8, fch1=1416.0 - 0.015625, foff=-0.03125, tsamp=32e-6, tstart=59000.0)


TIMING_DEAD_CHANNEL, TIMING_DEAD_CODE = 17, 100


def timing_run(lib, d_rows, rounds=5):
    """10 s x 1024 channels of 8-bit rows resident at `d_rows`, channel TIMING_DEAD_CHANNEL constant at TIMING_DEAD_CODE (dead:
    flagged wholly in every call, and replaced by the same code, so every round uploads a mask and launches the apply kernel on
    the same rows): after one warm-up of each, the median of `rounds` frbch_rfi_clean_device calls (defaults) and of `rounds`
    frbch_dedisperse_device calls over 64 DMs -> dict"""
    import statistics
    import time
    from tests.hipmem import GuardedBuffer as DeviceBuffer
    desc = post.fil_desc(TIMING_HDR)
    dms = np.asarray(post.dm_list(300.0, 363.0, 1.0), dtype=np.float64)
    nout = lib.frbch_dedisperse_nout(C.byref(desc), TIMING_ROWS, dms.ctypes.data, len(dms))
    d_out = DeviceBuffer(len(dms) * nout * 4)
    par = params()
    nblk = lib.frbch_rfi_nblk(TIMING_ROWS, par.block_rows)
    m, repl = np.zeros((nblk, TIMING_NCHAN), np.uint8), np.zeros(TIMING_NCHAN)
    cf, bf = np.zeros(TIMING_NCHAN, np.uint8), np.zeros(nblk, np.uint8)
    err = C.create_string_buffer(256)
    nclip, used = C.c_uint64(0), C.c_uint32(99)

    def clean():
        t0 = time.perf_counter()
        code = lib.frbch_rfi_clean_device(C.byref(desc), C.c_void_p(d_rows), TIMING_ROWS, C.byref(par), None, 0, m.ctypes.data,
                                          repl.ctypes.data, cf.ctypes.data, bf.ctypes.data, C.byref(used), err, len(err))
        dt = time.perf_counter() - t0
        assert code == 0, err.value
        assert np.flatnonzero(cf).tolist() == [TIMING_DEAD_CHANNEL] and int(m.sum()) == nblk and repl[TIMING_DEAD_CHANNEL] == TIMING_DEAD_CODE
        return dt

    def dedisperse():
        t0 = time.perf_counter()
        code = lib.frbch_dedisperse_device(C.byref(desc), C.c_void_p(d_rows), TIMING_ROWS, dms.ctypes.data, len(dms), 0, 0.0, 0,
                                           d_out.ptr, nout, C.byref(nclip), err, len(err))
        dt = time.perf_counter() - t0
        assert code == 0, err.value
        return dt

    clean()
    dedisperse()
    t_clean = [clean() for _ in range(rounds)]
    t_dd = [dedisperse() for _ in range(rounds)]
    d_out.free()
    return {"rows": TIMING_ROWS, "nchan": TIMING_NCHAN, "nbits": 8, "block_rows": int(par.block_rows), "nblk": int(nblk), "ndm": len(dms),
            "kernel_used": used.value, "masked_cells": int(m.sum()), "rfi_clean_device_median_s": statistics.median(t_clean),
            "dedisperse_device_median_s": statistics.median(t_dd), "rfi_clean_device_each_s": [round(t, 6) for t in t_clean],
            "dedisperse_device_each_s": [round(t, 6) for t in t_dd]}
