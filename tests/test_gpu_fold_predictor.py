"""GPU tests of the all-product fold with a phase predictor (frbch_foldp_*): the cases of tests/test_fold_predictor.py on
the device against tests/fold_model_oracle.py, which kernel ran (the LDS kernel for 8- / 16-bit rows without delays, the
generic one otherwise), both kernels bit for bit on the same rows, and BASELINE size (10 s x 4 products x 1024 channels,
1.28 GB of rows): conservation, and the device time of the one call against the four single-product calls it replaces."""
import ctypes as C
import faulthandler
import json
import os
import time

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import fold_model_oracle as fo
from tests.hipmem import GuardedBuffer as DeviceBuffer, hip
from tests.test_fold_predictor import PAR, as_fil_all, check_equal, model_kw, random_rows
from tests.test_post import DM0, HDR, P0

pytestmark = pytest.mark.gpu

HDR1K = dict(HDR, nchans=1024, foff=-0.03125, fch1=1416.0 - 0.015625, tsamp=32e-6)
CALL_LIMIT_S = 120          # a device call that has not come back by then ends the test process (traceback on stderr)


def stats_dir():
    """where the GPU suite leaves its stage statistics: the directory test_gpu_post.test_full_size_scan_rows writes
    post_stages.json to (stated once, there), unless FRBCH_STATS_DIR names another"""
    import inspect
    import re
    from tests import test_gpu_post
    return os.environ.get("FRBCH_STATS_DIR") or re.search(r'os\.makedirs\("([^"]+)"', inspect.getsource(test_gpu_post.test_full_size_scan_rows)).group(1)


def blocks_1k(nrows):
    """three polyco blocks with both boundaries inside `nrows` rows of 32 us, 12 us and 20 us away from a row time"""
    T = nrows * HDR1K["tsamp"]
    offs = [round(T * f / 32e-6) * 32e-6 + 12e-6 for f in (0.15, 0.5, 0.85)]      # boundaries at the means of neighbours
    coeffs = [[0.11, 0.53, -0.31, 2.1], [0.42, -0.77, 0.25], [0.05, 0.9, 0.6, -1.4, 3.0]]
    return [dict(tmid=HDR1K["tstart"] + off / 86400.0, rphase=0.1 + 0.27 * k, f0=(1.0 / P0) * (1.0 + 1e-5 * k), span=1.0,
                 coeff=coeffs[k], site="g") for k, off in enumerate(offs)]


def test_block_boundaries_keep_clear_of_the_rows():
    segs = blocks_1k(40000)
    first = fo.block_first_rows(segs, HDR1K["tstart"], HDR1K["tsamp"], 40000)
    assert 0 < first[1] < first[2] < 40000
    for a, b in zip(segs[:-1], segs[1:]):
        x = (0.5 * (a["tmid"] + b["tmid"]) - HDR1K["tstart"]) * 86400.0
        assert abs(x / HDR1K["tsamp"] - round(x / HDR1K["tsamp"])) * HDR1K["tsamp"] > 1e-6


@pytest.mark.parametrize("nbits,nifs,delays,nbin,kernel", [(8, 4, False, 256, 1), (8, 4, False, 1024, 1), (16, 4, False, 256, 1),
                                                           (16, 1, False, 1024, 1), (8, 1, False, 256, 1), (8, 4, True, 256, 0),
                                                           (16, 4, True, 256, 0), (32, 4, False, 256, 0), (32, 1, True, 256, 0)])
def test_polyco_fold_matches_the_restatement(hip_lib, nbits, nifs, delays, nbin, kernel):
    nrows = 40000
    x = random_rows(nrows, nifs, 1024, nbits)
    segs = blocks_1k(nrows)
    info = {}
    prof, hits, _ = post.fold_all(as_fil_all(x, HDR1K, nbits), PAR, polyco=segs, nbin=nbin, subint_s=0.5, apply_delays=delays,
                                  lib=hip_lib, info=info)
    assert info["kernel_used"] == kernel
    wp, wh = fo.fold_all(x, nbin=nbin, subint_s=0.5, dm=DM0, apply_delays=delays, segs=segs, **model_kw(HDR1K))
    assert prof.shape == (3, nifs, 1024, nbin)
    check_equal(nbits, prof, hits, wp, wh)


@pytest.mark.parametrize("nbits,doppler", [(8, 0.0), (16, 1e-4)])
def test_polynomial_model_on_the_lds_kernel(hip_lib, nbits, doppler):
    """nseg = 0 on the LDS kernel: the restatement, and for doppler = 0 product p of the untouched frbch_fold_host"""
    x = random_rows(40000, 4, 1024, nbits, seed=9)
    fil = as_fil_all(x, HDR1K, nbits)
    info = {}
    prof, hits, _ = post.fold_all(fil, PAR, doppler=doppler, nbin=512, subint_s=0.5, lib=hip_lib, info=info)
    assert info["kernel_used"] == 1
    wp, wh = fo.fold_all(x, nbin=512, subint_s=0.5, f0=PAR["F0"], f1=PAR["F1"], pepoch_mjd=PAR["PEPOCH"], doppler=doppler,
                         **model_kw(HDR1K))
    check_equal(nbits, prof, hits, wp, wh)
    if doppler == 0.0:
        for p in (0, 3):
            desc = post.fil_desc(fil.header, product=p)
            one, oh = np.zeros((3, 512, 1024)), np.zeros((3, 512, 1024), dtype=np.uint32)
            err = C.create_string_buffer(256)
            rc = hip_lib.frbch_fold_host(C.byref(desc), x.ctypes.data, x.shape[0], PAR["F0"], PAR["F1"], PAR["PEPOCH"], PAR["DM"],
                                         0, 512, 0.5, 0, one.ctypes.data, oh.ctypes.data, 3, err, len(err))
            assert rc == 0, err.value
            assert np.array_equal(prof[:, p], one.transpose(0, 2, 1)) and np.array_equal(hits, oh.transpose(0, 2, 1))


def foldp_device(lib, hdr, d_rows_ptr, nrows, model, nsub, nifs):
    desc = post.fil_desc(hdr)
    nslot = nsub * model.nbin * hdr["nchans"]
    d_prof, d_hits = DeviceBuffer(nslot * nifs * 8), DeviceBuffer(nslot * 4)
    used = C.c_uint32(99)
    err = C.create_string_buffer(256)
    faulthandler.dump_traceback_later(CALL_LIMIT_S, exit=True)
    try:
        rc = lib.frbch_foldp_device(C.byref(desc), d_rows_ptr, nrows, C.byref(model), 0, d_prof.ptr, d_hits.ptr, nsub,
                                    C.byref(used), err, len(err))
    finally:
        faulthandler.cancel_dump_traceback_later()
    assert rc == 0, err.value
    prof = d_prof.to_numpy(np.float64).reshape(nsub, nifs, model.nbin, hdr["nchans"])
    hits = d_hits.to_numpy(np.uint32).reshape(nsub, model.nbin, hdr["nchans"])
    d_prof.free()
    d_hits.free()
    return prof, hits, used.value


def test_both_kernels_give_the_same_bits(hip_lib):
    """the same 8-bit rows twice: 4-byte aligned in HBM (the LDS kernel) and one byte further on (dword loads impossible: the
    generic kernel); and an nbin whose smallest tile, 16 channels, does not fit the LDS goes to the generic kernel as well"""
    nrows, nifs = 30000, 4
    x = random_rows(nrows, nifs, 1024, 8, seed=10)
    hdr = dict(HDR1K, nbits=8, nifs=nifs)
    segs = blocks_1k(nrows)
    model, _keep = post.fold_model(PAR, hdr, polyco=segs, nbin=512, subint_s=0.5, apply_delays=False)
    buf = DeviceBuffer(x.nbytes + 4)
    assert buf.ptr.value % 4 == 0
    assert hip().hipMemcpy(buf.ptr, x.ctypes.data, x.nbytes, 1) == 0
    pa, ha, ka = foldp_device(hip_lib, hdr, buf.ptr, nrows, model, 2, nifs)
    assert hip().hipMemcpy(C.c_void_p(buf.ptr.value + 1), x.ctypes.data, x.nbytes, 1) == 0
    pb, hb, kb = foldp_device(hip_lib, hdr, C.c_void_p(buf.ptr.value + 1), nrows, model, 2, nifs)
    buf.free()
    assert (ka, kb) == (1, 0)
    assert np.array_equal(pa, pb) and np.array_equal(ha, hb)
    wp, wh = fo.fold_all(x, nbin=512, subint_s=0.5, segs=segs, **model_kw(HDR1K))
    assert np.array_equal(pa.transpose(0, 1, 3, 2), wp) and np.array_equal(ha.transpose(0, 2, 1), wh)
    info = {}
    prof, hits, _ = post.fold_all(as_fil_all(x, HDR1K, 8), PAR, polyco=segs, nbin=4096, subint_s=0.5, lib=hip_lib, info=info)
    assert info["kernel_used"] == 0                                   # 4096 bins x 16 channels x 4 B = 256 KiB
    wp, wh = fo.fold_all(x, nbin=4096, subint_s=0.5, segs=segs, **model_kw(HDR1K))
    check_equal(8, prof, hits, wp, wh)


@pytest.fixture(scope="module")
def full_size_rows():
    """10 s of a 32 MHz IF in four products as the channeliser writes them (312 500 rows x 4 x 1024 channels, 8 bit),
    seeded random as test_full_size_scan_rows, resident in HBM"""
    rng = np.random.default_rng(7)
    data = rng.integers(100, 156, size=(312500, 4, 1024), dtype=np.uint8)
    buf = DeviceBuffer.from_numpy(data)
    yield data, buf
    buf.free()


def test_full_size_all_products(hip_lib, full_size_rows):
    data, d_rows = full_size_rows
    nrows, nifs, nchan = data.shape
    hdr = dict(HDR1K, nbits=8, nifs=nifs)
    par = dict(F0=1.0 / P0, F1=0.0, PEPOCH=None, DM=DM0, PSR="x")
    model, _keep = post.fold_model(par, hdr, nbin=512, subint_s=10.0, apply_delays=False)
    prof, hits, used = foldp_device(hip_lib, hdr, d_rows.ptr, nrows, model, 1, nifs)
    assert used == 1
    assert int(hits.sum(dtype=np.int64)) == nrows * nchan
    assert np.array_equal(prof.sum(axis=2)[0], data.sum(axis=0, dtype=np.int64).astype(np.float64))   # per product and channel
    b = fo.bins(nrows, 1, nbin=512, f0=par["F0"], **model_kw(HDR1K))[:, 0]
    assert np.array_equal(hits[0, :, 5], np.bincount(b, minlength=512))
    for q, c in ((0, 0), (2, 517), (3, 1023)):
        assert np.array_equal(prof[0, q, :, c], np.bincount(b, weights=data[:, q, c].astype(np.float64), minlength=512))


def test_one_call_is_not_slower_than_four(hip_lib, full_size_rows):
    """device time of ONE frbch_foldp_device over the resident rows (median of 7 calls after a warm-up) against the four
    frbch_fold_device calls, one per product, that gave the same profiles before (that entry point is untouched): printed,
    written to fold_stages.json next to the other stage statistics (profiles/NOTES.md), and the one call
    must not be slower"""
    data, d_rows = full_size_rows
    nrows, nifs, nchan = data.shape
    hdr = dict(HDR1K, nbits=8, nifs=nifs)
    par = dict(F0=1.0 / P0, F1=0.0, PEPOCH=None, DM=DM0, PSR="x")
    nbin, nslot = 512, 512 * nchan
    model, _keep = post.fold_model(par, hdr, nbin=nbin, subint_s=10.0, apply_delays=False)
    d_prof, d_hits = DeviceBuffer(nslot * nifs * 8), DeviceBuffer(nslot * 4)
    err = C.create_string_buffer(256)
    used = C.c_uint32(0)

    def timed(fn):
        faulthandler.dump_traceback_later(CALL_LIMIT_S, exit=True)
        try:
            t0 = time.perf_counter()
            rc = fn()
            dt = time.perf_counter() - t0
        finally:
            faulthandler.cancel_dump_traceback_later()
        assert rc == 0, err.value
        return dt

    def all_products():
        return hip_lib.frbch_foldp_device(C.byref(post.fil_desc(hdr)), d_rows.ptr, nrows, C.byref(model), 0, d_prof.ptr,
                                          d_hits.ptr, 1, C.byref(used), err, len(err))

    def one_product(p):
        return hip_lib.frbch_fold_device(C.byref(post.fil_desc(hdr, product=p)), d_rows.ptr, nrows, par["F0"], 0.0, hdr["tstart"],
                                         DM0, 0, nbin, 10.0, 0, d_prof.ptr, d_hits.ptr, 1, err, len(err))

    timed(all_products)                                                 # warm-up (module load, first allocations)
    t_all = [timed(all_products) for _ in range(7)]
    assert used.value == 1
    got = d_prof.to_numpy(np.float64).reshape(nifs, nbin, nchan)
    timed(lambda: one_product(0))
    t_four = [sum(timed(lambda p=p: one_product(p)) for p in range(nifs)) for _ in range(5)]
    assert np.array_equal(d_prof.to_numpy(np.float64)[:nslot].reshape(nbin, nchan), got[nifs - 1])    # the same sums
    row_bytes = data.nbytes
    stats = {"rows": nrows, "nifs": nifs, "nchan": nchan, "nbin": nbin, "row_bytes": row_bytes,
             "foldp_device_s_median": float(np.median(t_all)), "foldp_device_s_all": t_all,
             "four_fold_device_s_median": float(np.median(t_four)), "four_fold_device_s_all": t_four,
             "speedup": float(np.median(t_four) / np.median(t_all)),
             "foldp_row_read_gb_per_s": row_bytes / float(np.median(t_all)) / 1e9}
    print("FOLD-STAGES " + json.dumps(stats))
    os.makedirs(stats_dir(), exist_ok=True)
    with open(os.path.join(stats_dir(), "fold_stages.json"), "w") as f:
        json.dump(stats, f)
    d_prof.free()
    d_hits.free()
    assert np.median(t_all) <= np.median(t_four), stats
