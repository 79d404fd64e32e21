"""GPU tests of the single-pulse search (frbch_spsearch_*, frbch_dedisperse_search_host): the LDS kernel
frbch_post_sp_search_lds and the generic kernels it falls back to, on the series of tests/spsearch_cases.py against the numpy
restatement tests/spsearch_oracle.py -- record for record, sigma to the bit: the search is integer arithmetic behind a
fixed-order normalisation, so there is no tolerance anywhere.  Every case asserts `kernel_used`."""
import ctypes as C
import json
import os
import statistics
import time

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import post_cases as pc
from tests import spsearch_cases as sc
from tests import spsearch_oracle as so
from tests.hipmem import GuardedBuffer as DeviceBuffer

pytestmark = pytest.mark.gpu

LDS, GENERIC = 1, 0


def kernel_for(widths):
    """the documented condition: the largest LISTED width is at most 512 (every nout here is far below 2^31)"""
    return LDS if max(widths) <= sc.LDS_MAX_WIDTH else GENERIC


def check(lib, y, widths, thr, L, want, kernel):
    rc, got, ncand, used, msg = sc.spsearch_host(lib, y, widths, thr, L)
    assert rc == 0, msg
    assert used == kernel
    assert ncand == want.size and sc.same_records(got, want)


# ---- the grid of the emulator tests, and the tile boundaries of the LDS kernel --------------------------------------
@pytest.mark.parametrize("name", sorted(sc.CASES) + sorted(sc.TILE_CASES))
def test_device_equals_the_oracle(hip_lib, name):
    """nout 777 / 5000 / 20000 / 20011 and T - 1, T, T + 1, 3 T + 5 (T = 2048, the LDS kernel's tile); 1, 3 and 9 DMs; blocks of
    64, 1000, 8192 and one longer than the series; pulses of width 6 and 300 across a tile edge, peaks on the first and last
    sample of a tile (their local-maximum windows cross it), at t = 0 and ending at nout; dead blocks, a NaN, plateaus"""
    y, widths, thr, L, want, _raws = sc.case(name)
    if name in sc.TILE_CASES:
        assert kernel_for(widths) == LDS and y.shape[0] == 9 and want.size >= 9
    check(hip_lib, y, widths, thr, L, want, kernel_for(widths))


def test_tile_cases_hold_what_they_are_written_for():
    y, widths, thr, L, want, raws = sc.case("three_tiles_5")
    found = {(int(c["dm_index"]), int(c["sample"]), int(c["width"])) for c in want}
    T = sc.TILE
    assert any(d == 1 and w == 300 and abs(s - T) <= 20 for d, s, w in found)                # width 300 across the edge
    assert (2, T - 1, 1) in found and any(d == 7 and s in (T, T + 1) for d, s, _w in found)    # last / first sample of a tile
    assert any(d == 0 and w == 6 and T - 3 <= s - 3 < T for d, s, w in found)                # width 6 starts before the edge, ends after
    assert any(t < T <= t + w // 2 for raw in raws for t, w, _s in raw)                      # a local-maximum window crosses the edge
    assert any(d == 6 and w == 6 and s == y.shape[1] - 3 for d, s, w in found)               # ends at nout


# ---- the same inputs on the generic kernel -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_L64_w1"])
def test_generic_kernel_gives_the_lds_kernels_records(hip_lib, name):
    """nout = 777: a listed width of 1024 is skipped by the search but counts for the choice of kernel"""
    y, widths, thr, L, want, _raws = sc.case(name)
    assert y.shape[1] < 1024
    check(hip_lib, y, widths, thr, L, want, LDS)
    check(hip_lib, y, list(widths) + [1024], thr, L, want, GENERIC)


@pytest.mark.parametrize("name", ["blocks_default", "ties", "tile_plus_1", "three_tiles_5"])
def test_width_above_the_lds_limit_takes_the_generic_kernel(hip_lib, name):
    """the series of the LDS cases with a width of 1024 added (generic) and with 512, the largest the LDS kernel takes, and 513"""
    y, widths, thr, L, _want, _raws = sc.case(name)
    for extra, kernel in ((1024, GENERIC), (512, LDS), (513, GENERIC)):
        ws = list(widths) + [extra]
        check(hip_lib, y, ws, thr, L, so.search(y, ws, thr, L), kernel)


# ---- dedispersion and search in one call ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,zerodm,clip", [(8, True, 5.0), (16, True, 0.0), (32, False, 5.0)])
def test_dedisperse_search_equals_the_two_calls(hip_lib, nbits, zerodm, clip):
    hdr = pc.make_hdr(1024)
    x = pc.make_rows(6000, 2, 1024, nbits, seed=21)
    dms = [40.0 + 1.5 * i for i in range(9)]
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    nout = pc.dedisp_nout(hip_lib, hdr, x, 1, dms)
    series, nclip = pc.dedisp_host(hip_lib, hdr, x, 1, dms, zerodm, clip, nout)
    rc, want, nwant, used, msg = sc.spsearch_host(hip_lib, series, sc.DEFAULT, 5.0, 1000)
    assert rc == 0 and used == LDS and nwant > 0, msg
    params = post.sp_params(sc.DEFAULT, 5.0, 1000)
    for with_series in (True, False):
        out = np.zeros((9, nout), dtype=np.float32)
        cands = np.zeros(4096, dtype=post.SP_CAND)
        ncand, k, nc = C.c_uint64(0), C.c_uint32(9), C.c_uint64(0)
        err = C.create_string_buffer(512)
        rc = hip_lib.frbch_dedisperse_search_host(C.byref(pc.desc_of(hdr, x, 1)), x.ctypes.data, x.shape[0], dm_arr.ctypes.data, 9,
                                                  1 if zerodm else 0, clip, C.byref(params), 0, out.ctypes.data if with_series else None,
                                                  nout, C.byref(nc), cands.ctypes.data, 4096, C.byref(ncand), C.byref(k), err, len(err))
        assert rc == 0, err.value
        assert k.value == LDS and nc.value == nclip and ncand.value == nwant
        assert sc.same_records(cands[:nwant], want)
        if with_series:
            assert out.tobytes() == series.tobytes()
    assert sc.same_records(want, so.search(series, sc.DEFAULT, 5.0, 1000))


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_dispersed_burst_end_to_end(hip_lib, tmp_path):
    """a burst of 5 samples at DM 56.7 in 8-bit noise rows of 64 channels, searched over 9 DMs 5 apart through search_fil"""
    from tests.test_fold_predictor import write_fil
    from tests.test_post import DM0, HDR
    from tests.test_spsearch import dispersed_burst_rows
    x = dispersed_burst_rows(9000, HDR, DM0, 3000, 5, 30)
    fil = str(tmp_path / "burst.fil")
    write_fil(fil, x[:, None, :], HDR, 1)
    info = {}
    files, cands = post.search_fil(fil, DM0 - 20.0, dm2=DM0 + 20.0, dmstep=5.0, threshold=6.0, lib=hip_lib, info=info)
    assert len(files) == 9 and info["kernel_used"] == LDS
    top = cands[np.argmax(cands["sigma"])]
    assert int(top["dm_index"]) == 4 and abs(int(top["sample"]) - 3002) <= 1 and int(top["width"]) in (4, 6)
    assert open(files[4]).read().splitlines()[0] == post.SP_HEADER


# ---- timing --------------------------------------------------------------------------------------------------------
def test_search_is_not_what_the_dm_range_waits_for(hip_lib):
    """the documented prepsubband shape -- 10 s x 1024 channels, 8 bit, 64 DMs, rows resident in HBM (made there with torch) --
    dedispersed, then searched at threshold 6 with the default widths: after one warm-up call of each, the median of five
    frbch_spsearch_device calls is at most the median of five frbch_dedisperse_device calls (margin 1.0)"""
    torch = pytest.importorskip("torch")
    nrows, nchan = 312500, 1024
    hdr = dict(nchans=nchan, nifs=1, nbits=8, fch1=1416.0 - 0.015625, foff=-0.03125, tsamp=32e-6, tstart=59000.0)
    gen = torch.Generator(device="cuda").manual_seed(5)
    rows = torch.randint(100, 156, (nrows, nchan), dtype=torch.uint8, device="cuda", generator=gen)
    torch.cuda.synchronize()
    desc = post.fil_desc(hdr)
    dms = np.asarray(post.dm_list(300.0, 363.0, 1.0), dtype=np.float64)
    nout = hip_lib.frbch_dedisperse_nout(C.byref(desc), nrows, dms.ctypes.data, len(dms))
    d_out = DeviceBuffer(len(dms) * nout * 4)
    params = post.sp_params(post.default_widths(hdr["tsamp"]), 6.0, 1000)
    cands = np.zeros(4096, dtype=post.SP_CAND)
    err = C.create_string_buffer(256)
    nclip, ncand, used = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)

    def dedisperse():
        t0 = time.perf_counter()
        rc = hip_lib.frbch_dedisperse_device(C.byref(desc), C.c_void_p(rows.data_ptr()), nrows, dms.ctypes.data, len(dms), 0, 0.0, 0,
                                             d_out.ptr, nout, C.byref(nclip), err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        return dt

    def search():
        t0 = time.perf_counter()
        rc = hip_lib.frbch_spsearch_device(d_out.ptr, len(dms), nout, C.byref(params), 0, cands.ctypes.data, cands.size, C.byref(ncand),
                                           C.byref(used), err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        return dt

    dedisperse()
    search()
    t_dd = statistics.median(dedisperse() for _ in range(5))
    t_sp = statistics.median(search() for _ in range(5))
    stats = {"rows": nrows, "nchan": nchan, "ndm": len(dms), "nout": int(nout), "widths": post.default_widths(hdr["tsamp"]), "threshold": 6.0,
             "kernel_used": used.value, "ncand": int(ncand.value), "dedisperse_device_median_s": t_dd, "spsearch_device_median_s": t_sp}
    print("SPSEARCH-TIMING " + json.dumps(stats))
    assert used.value == LDS
    assert t_sp <= 1.0 * t_dd, stats
