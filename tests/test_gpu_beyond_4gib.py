"""GPU tests of the device entry points behind the filterbank that walk the whole file -- dedispersion, the interference stages,
both folds, the cut-outs, the single-pulse search and frbch_candidates_device -- on rows that pass 2^31 and 2^32, counted in
bytes, in elements and in t * nchan; the entry points that are pointed at a candidate or at sub-bands (burst spectra and RM,
profile, DM scan, burst ACF, scattering, the band series and the band search) are held on the same rows by
tests/test_gpu_beyond_4gib_burst.py.  The shapes are those of the spliced files: A8 (8192 channels x 4 products x 8 bit, config 3's IFall), A16 (8192 x 2 x
16 bit: the same row, the element count passes 2^31) and B8 (65 536 channels of Stokes I, config 4's IFall).  tests/big_rows.py
describes the 4.4 GB of rows by a base of 3001 rows, fills the device buffer by device-to-device copies and rebuilds any window
on the host; tests/test_big_rows.py holds its references to the restatements on a whole small array.  Every stage runs at the
16-byte aligned address (its fast kernel) and a few bytes further on (its generic kernel) and asserts which kernel it took;
outputs are compared at the start, where the input rows straddle each mark, and at the ragged end -- `==`, no tolerance.

Not covered here or in tests/test_gpu_beyond_4gib_burst.py, so not held past the mark: the series readers of the periodicity and
acceleration searches and frbch_resample_device; the `_host` twins other than frbch_dedisperse_host; the band plane past 2^32
ELEMENTS (both modules pass 2^32 bytes of it); the writers whose row count shrinks with `-t` (frbch_k2_scrunch) and the coherent
chain's frbch_k4_fast; the emulator build at this size."""
import ctypes as C
import functools

import numpy as np
import pytest

from frb_baseband_amd import post
from oracle import post_oracle as po
from tests import big_rows as bg
from tests import post_cases as pc
from tests import spsearch_oracle as so
from tests.hipmem import GuardedBuffer, hip

pytestmark = pytest.mark.gpu

TILED = LDS = FAST = 1
GENERIC = 0
BLOCK = 1024
PROD = {"A8": 2, "A16": 1, "B8": 0}


@functools.lru_cache(maxsize=None)
def described(name):
    return bg.big(name)


@pytest.fixture(scope="module", params=list(bg.SHAPES))
def rows(request, hip_lib):
    """(name, the resident rows): one buffer of nbytes + 16 per shape, alive for the tests of that shape only"""
    res = bg.Resident(described(request.param), bg.DeviceMem)
    yield request.param, res
    res.free()


@functools.lru_cache(maxsize=None)
def want_dedisp(name, clip):
    return bg.want_dedisp(described(name), PROD[name], bg.DMS, clip, 512)


@functools.lru_cache(maxsize=None)
def want_cutout(name):
    """(the planes do not depend on where the rows lie: one restatement for both addresses)"""
    br = described(name)
    return bg.want_cutout(br, PROD[name], bg.cut_cands(br))


# ---- dedispersion -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("zerodm,clip", [(True, 5.0), (False, 0.0), (True, 0.0), (False, 5.0)])
def test_dedisperse(hip_lib, rows, zerodm, clip, shift):
    """9 DMs (one whole group, one partial), largest delays of 1014 to 1711 rows; the clip needs the row sums of ALL rows, which
    are those of the base; nclip as well"""
    name, res = rows
    res.lay(shift)
    bg.check_dedisp(hip_lib, res, PROD[name], bg.DMS, zerodm, clip, TILED if shift == 0 else GENERIC, want_dedisp(name, clip))


def test_dedisperse_host_uploads_past_the_mark(hip_lib):
    """frbch_dedisperse_host on A8, the host array built replica by replica from the base"""
    br = described("A8")
    x = np.empty((br.nrows, br.nifs, br.nchan), dtype=br.dtype)
    for r0 in range(0, br.nrows, br.P):
        n = min(br.P, br.nrows - r0)
        x[r0:r0 + n] = br.base[:n]
    nout, wclip, runs = want_dedisp("A8", 5.0)
    dm_arr = np.ascontiguousarray(bg.DMS, dtype=np.float64)
    out = np.empty((dm_arr.size, nout), dtype=np.float32)
    nclip = C.c_uint64(0)
    err = C.create_string_buffer(512)
    with bg.guarded():
        rc = hip_lib.frbch_dedisperse_host(C.byref(br.desc(PROD["A8"])), x.ctypes.data, br.nrows, dm_arr.ctypes.data, dm_arr.size, 1, 5.0, 0,
                                           out.ctypes.data, nout, C.byref(nclip), err, len(err))
    assert rc == 0, err.value
    assert nclip.value == wclip
    for t0, series in runs[True]:
        assert np.array_equal(out[:, t0:t0 + series.shape[1]], series)


# ---- interference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
def test_rfi_stats_and_peaks(hip_lib, rows, shift):
    """blocks of 1024 rows: 0 and 1, those on both sides of each mark, the last three (the last is ragged), after four cells
    became constants"""
    _name, res = rows
    res.lay(shift)
    prod = res.br.nifs - 1
    bg.poke_four_cells(res, prod, BLOCK)
    k = FAST if shift == 0 else GENERIC
    bg.check_stats_and_peaks(hip_lib, res, prod, BLOCK, k, k)


@pytest.mark.parametrize("shift", [0, 4])
def test_rfi_apply_writes_its_cells_and_nothing_else(hip_lib, rows, shift):
    _name, res = rows
    res.lay(shift)
    bg.check_apply(hip_lib, res, res.br.nifs - 1, BLOCK)


@pytest.mark.parametrize("shift", [0, 4])
def test_rfi_clean_is_the_sequence_of_its_parts(hip_lib, rows, shift):
    _name, res = rows
    bg.check_clean_is_its_parts(hip_lib, res, res.br.nifs - 1, BLOCK, shift, FAST if shift == 0 else GENERIC)


@pytest.mark.parametrize("shift", [0, 4])
def test_rfi_cleanf_is_the_sequence_of_its_parts(hip_lib, rows, shift):
    _name, res = rows
    k = FAST if shift == 0 else GENERIC
    bg.check_cleanf_is_its_parts(hip_lib, res, res.br.nifs - 1, BLOCK, shift, (k, k))


@pytest.mark.parametrize("shift", [0, 4])
def test_rfi_cleanp_is_the_sequence_of_its_parts(hip_lib, rows, shift):
    _name, res = rows
    bg.check_cleanp_is_its_parts(hip_lib, res, BLOCK, shift, FAST if shift == 0 else GENERIC)


# ---- fold -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 2])
def test_fold_all_products(hip_lib, rows, shift):
    """tsamp = 2^-14 s, F0 = 16 Hz, 256 bins: bin = (t % 1024) // 4 exactly; three sub-integrations, the last wholly past the 2^32
    mark.  The LDS kernel asks for a 4-byte aligned address only: 2 bytes further on the generic kernel runs."""
    _name, res = rows
    res.lay(shift)
    bg.check_foldp(hip_lib, res, LDS if shift == 0 else GENERIC)


@pytest.mark.parametrize("shift", [0, 2])
def test_fold_one_product(hip_lib, rows, shift):
    _name, res = rows
    res.lay(shift)
    bg.check_fold(hip_lib, res, res.br.nifs - 1)


# ---- cut-outs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
def test_cutout(hip_lib, rows, shift):
    """nt = nf = 64, ndm = 16: a candidate near row 1000, one whose window crosses the 2^32 row, one clamped at nrows"""
    name, res = rows
    res.lay(shift)
    kernel = bg.cut_kernel_expected(res.br, shift)
    assert kernel == (LDS if shift == 0 and name != "B8" else GENERIC)
    bg.check_cutout(hip_lib, res, PROD[name], kernel, want=want_cutout(name))


# ---- the resident chain -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
def test_candidates_chain_finds_a_burst_behind_the_mark(hip_lib, rows, shift):
    """frbch_candidates_device with a dispersed burst (DM 104, 4 rows) written 300 rows behind the 2^32 row: every array equals
    the single stages through the library, and the best candidate sits at the burst's row and DM"""
    name, res = rows
    br = res.br
    res.lay(shift)
    prod, t_top, width = PROD[name], br.byte_mark_rows[-1] + 300, 4
    bg.write_burst(res, prod, 104.0, t_top, width, 3)
    sp = post.sp_params([1, 2, 4, 8], 8.0, 1000)
    want = bg.chain_of_stages(hip_lib, res, prod, bg.DMS, sp, True, 5.0, 2, 8.0)
    with bg.guarded():
        got = post.candidates_resident(None, br.hdr(), bg.DMS, sp=sp, zerodm=True, clip=5.0, dm_gap=2, nt=bg.CUT_NT, nf=bg.CUT_NF,
                                       ndm=bg.CUT_NDM, dm_span=8.0, product=prod, lib=hip_lib, d_rows=res.address, nrows=br.nrows)
    assert got["row_uploads"] == 0 and got["kernel_used"] == want["kernel_used"]
    assert want["kernel_used"] == ([0, TILED, LDS, LDS if name != "B8" else GENERIC] if shift == 0 else [0, GENERIC, LDS, GENERIC])
    for key in ("nout", "nclipped"):
        assert got[key] == want[key]
    for key in ("cands", "groups", "cut_cands", "ft", "ft_hits", "dt", "dt_hits"):
        assert got[key].shape == want[key].shape and got[key].tobytes() == np.ascontiguousarray(want[key]).tobytes(), key
    best = got["groups"][np.argmax(got["groups"]["best"]["sigma"])]["best"]
    assert int(best["dm_index"]) == 4 and abs(int(best["sample"]) - (t_top + width // 2)) <= 1 and int(best["width"]) == 4
    res.check_equals()                                   # frbch_candidates_device never writes the rows


# ---- the output of the dedispersion and the input of the search past the mark ------------------------------------------------
SERIES_ROWS, SERIES_NDM = (1 << 22) + 300, 260
SERIES_CHECKED = (256, 257, 258, 259)                   # row 256 crosses 2^32 bytes of the series
HATS = ((0, 5000, 4, 6.0), (255, 2000000, 8, 5.0), (256, 777, 2, 9.0), (256, 4100000, 16, 3.0), (259, 3000000, 4, 7.0))   # (row, t, w, sigmas)


@pytest.fixture(scope="module")
def long_series(hip_lib):
    """64 channels x 8 bit, 2^22 + 300 rows, 260 DMs: series[260][nout] float32 of 4.36 GB in HBM -> (rows, header, DMs, nout,
    the buffer, kernel)"""
    hdr = pc.make_hdr(64)
    x = np.random.default_rng(77).integers(60, 124, size=(SERIES_ROWS, 1, 64), dtype=np.uint8)
    dms = [0.5 * i for i in range(SERIES_NDM)]            # (64 channels are one tile: its delays must fit the LDS, 393 rows at most)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    desc = pc.desc_of(hdr, x)
    nout = hip_lib.frbch_dedisperse_nout(C.byref(desc), SERIES_ROWS, dm_arr.ctypes.data, dm_arr.size)
    assert 256 * nout * 4 < 1 << 32 < 257 * nout * 4 and SERIES_NDM * nout * 4 > (1 << 32) + (60 << 20)
    d_rows = GuardedBuffer.from_numpy(x)
    d_out = GuardedBuffer(SERIES_NDM * nout * 4)
    kernel = hip_lib.frbch_dedisperse_kernel(C.byref(desc), d_rows.ptr, SERIES_ROWS, dm_arr.ctypes.data, dm_arr.size)
    nclip = C.c_uint64(0)
    err = C.create_string_buffer(512)
    with bg.guarded():
        rc = hip_lib.frbch_dedisperse_device(C.byref(desc), d_rows.ptr, SERIES_ROWS, dm_arr.ctypes.data, dm_arr.size, 0, 0.0, 0, d_out.ptr,
                                             nout, C.byref(nclip), err, len(err))
    assert rc == 0, err.value
    d_rows.free()
    yield x, hdr, dms, nout, d_out, kernel
    d_out.free()


def series_row(d_out, nout, i):
    return bg.DeviceMem.get(d_out.ptr.value + i * nout * 4, nout * 4).view(np.float32)


@pytest.fixture(scope="module")
def hat_rows(long_series):
    """top-hats added to DM rows 0, 255, 256 and 259 where they lie in HBM -> {row: its samples on the host}"""
    _x, _hdr, _dms, nout, d_out, _k = long_series
    host = {}
    for i in sorted({h[0] for h in HATS}):
        y = series_row(d_out, nout, i).copy()
        sig = float(y[:100000].std())
        for r, t, w, amp in HATS:
            if r == i:
                y[t:t + w] += np.float32(amp * sig)
        bg.DeviceMem.put(d_out.ptr.value + i * nout * 4, y)
        host[i] = y
    return host


def test_series_rows_past_the_mark(long_series):
    """DM rows 256 to 259 against the restatement on their own (outside the samples a top-hat of the search test may
    have been added to)"""
    x, hdr, dms, nout, d_out, kernel = long_series
    assert kernel == TILED
    cols = np.asfortranarray(x[:, 0, :])                 # (a channel's rows contiguous: the restatement walks channel by channel)
    dl = [po.delays_samples(hdr["fch1"], hdr["foff"], 64, hdr["tsamp"], dms[i]) for i in SERIES_CHECKED]
    want = po.sum_delayed(cols, None, dl, nout, False)
    for k, i in enumerate(SERIES_CHECKED):
        keep = np.ones(nout, dtype=bool)
        for r, t, w, _amp in HATS:
            if r == i:
                keep[t:t + w] = False
        assert np.array_equal(series_row(d_out, nout, i)[keep], want[k][keep]), "DM row %d" % i


@pytest.mark.parametrize("widths,kernel", [((1, 2, 4, 8, 16), LDS), ((3, 520), GENERIC)])
def test_search_reads_the_series_past_the_mark(hip_lib, long_series, hat_rows, widths, kernel):
    """top-hats in DM rows 0, 255, 256 and 259: the records around them against tests/spsearch_oracle.py on that row alone (the
    normalisation is per DM and block), and ncand against the sum of the library's own calls row by row; widths up to 512 take
    the LDS kernel, a width of 520 the generic ones"""
    _x, _hdr, _dms, nout, d_out, _k = long_series
    sp = post.sp_params(list(widths), 7.0, 1000)
    got, ncand, used = bg.spsearch_device(hip_lib, d_out.ptr.value, SERIES_NDM, nout, sp, cap=1 << 16)
    assert used == kernel
    for i, t, _w, _amp in HATS:
        # the blocks of 1000 samples are normalised one by one: the restatement on 12 whole blocks around the top-hat gives the
        # records of the whole row there, 1500 samples (the widest boxcar, its window and a neighbour's) away from the cut
        lo = max(0, t // 1000 - 5) * 1000
        hi = lo + 12000
        assert hi <= (nout // 1000 - 1) * 1000
        want = so.search(hat_rows[i][lo:hi], list(widths), 7.0, 1000)
        a, b = (0 if lo == 0 else lo + 1500), hi - 1500
        want = want[(want["sample"] + lo >= a) & (want["sample"] + lo < b)].copy()
        want["sample"] += lo
        want["dm_index"] = i
        assert want.size >= 1 or (i, t) == (256, 4100000)                      # (16 samples of 3 sigma: for the narrow boxcars only)
        mine = got[(got["dm_index"] == i) & (got["sample"] >= a) & (got["sample"] < b)]
        assert mine.tobytes() == want.tobytes(), "records of DM row %d near sample %d" % (i, t)
    total = 0
    for i in range(SERIES_NDM):
        _c, n, _u = bg.spsearch_device(hip_lib, d_out.ptr.value + i * nout * 4, 1, nout, sp)
        total += n
    assert ncand == total
