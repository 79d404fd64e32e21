"""GPU tests of the burst and band entry points on rows that pass 2^31 and 2^32 bytes -- frbch_burstspec_device,
frbch_burst_rm_device, frbch_polprof_device, frbch_dmscan_device, frbch_burstacf_device, frbch_burstscat_device,
frbch_dedisperse_bands_device and frbch_bandsearch_device -- at the shapes of tests/test_gpu_beyond_4gib.py: A8 (8192 channels x
4 products x 8 bit), A16 (8192 x 2 x 16 bit) and B8 (65 536 channels of Stokes I).  tests/big_burst_rows.py places four
candidates in every call: one whose earlier off window starts in front of row 0, one whose on-pulse rows run across the row at
2^31 bytes as the delay grows over the band, one likewise at 2^32 bytes, one whose later off window is cut at nrows; a launch
holds t0 values on both sides of both marks.  Expected values are the restatements on the window of rows a candidate can
touch, computed once per shape and shared by the two addresses (tests/test_big_burst_rows.py holds them to the restatements
on a whole small array).  Every call runs at the 16-byte aligned address (the fast form, where the plan rule restated in the
*_cases modules admits it) and 4 bytes further on (the generic form); kernel_used is held to the `_kernel` query and to the form
the case was built for.  Every comparison is the entry point's own comparator: `==` and bytes, libm's slack where its own tests
allow it.  None of these entry points writes the rows: the whole buffer is compared with the base after every call.

A shape an entry point refuses appears as the asserted refusal: more than 16 384 channels (B8) for the profile, the DM scan, the
ACF and the scattering fit; fewer than four products (A16, B8) for the composite, the profile and the coherency order.

The band plane itself past the mark (`long_bands`): out[130 * 10][nout] float32 passes 2^32 BYTES in series 1023, the fp64
zero-DM prefix plane [130][4][nout] passes 2^32 bytes in DM 127; the uint32 prefix plane [130][4][nout] passes 2^31 bytes there
and stays below 2^32; no plane reaches 2^32 ELEMENTS (not held here)."""
import ctypes as C
import functools

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from oracle import post_oracle as po
from tests import acf_cases as ac
from tests import bands_cases as bc
from tests import bands_oracle as bo
from tests import big_burst_rows as bb
from tests import big_rows as bg
from tests import burst_edge_cases as bec
from tests import dmscan_cases as dc
from tests import polprof_cases as pc
from tests import post_cases as poc
from tests import rm_cases as rc
from tests import scat_cases as sc
from tests.hipmem import GuardedBuffer

pytestmark = pytest.mark.gpu

FAST, GENERIC = 1, 0
PROD = {"A8": 2, "A16": 1, "B8": 0}
ACF_FF = {"A8": (16, 64), "A16": (16, 32)}               # below a 64-byte tile's channels (a direct store), and a tile (the join)
SCAN_ORDERS = {"A8": ((2, False), (0, True)), "A16": ((1, False),), "B8": ()}
NCMP = 512
MANY = "more than 16384 channels"
FOUR = "the four products"
COH = "coherency products need nifs = 4"


@functools.lru_cache(maxsize=None)
def described(name):
    return bg.big(name)


@functools.lru_cache(maxsize=None)
def cands_of(name):
    """the four candidates of a shape, their conditions asserted"""
    br = described(name)
    c = bb.burst_cands(br, bb.DM, bb.WIDTH, bb.OFF_GAP, bb.OFF_LEN)
    bb.conditions(br, c)
    c.setflags(write=False)
    return c


@pytest.fixture(scope="module", params=list(bg.SHAPES))
def rows(request, hip_lib):
    """(name, the resident rows): one buffer of nbytes + 16 per shape, alive for the tests of that shape only"""
    res = bg.Resident(described(request.param), bg.DeviceMem)
    yield request.param, res
    res.free()


def form(shift):
    return FAST if shift == 0 else GENERIC


def refused(lib, fn, c, res, caller, text):
    """the call is refused with FRBCH_E_ARG and `text`; the outputs (a few poisoned words) keep their fill"""
    with bg.guarded():
        code, msg, out, _k = caller(fn, c, C.c_void_p(res.address))
    assert code == _lib.E_ARG and text in msg and bb.untouched(out), (code, msg)


# ---- expectations, once per shape ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def want_sums(name):
    return bb.want_sums(described(name), cands_of(name))


@functools.lru_cache(maxsize=None)
def want_spectra(name, coh):
    return bb.want_spectra(want_sums(name), coh)


@functools.lru_cache(maxsize=None)
def want_rm(name):
    return bb.want_rm(described(name), cands_of(name))


@functools.lru_cache(maxsize=None)
def want_prof(name, coh):
    return bb.want_prof(described(name), cands_of(name), coh)


@functools.lru_cache(maxsize=None)
def want_scan(name, prod, coh, ddm):
    return bb.want_scan(described(name), cands_of(name), prod, coh, ddm)


@functools.lru_cache(maxsize=None)
def want_acf(name, ffactor):
    return bb.want_acf(described(name), cands_of(name), PROD[name], ffactor)


@functools.lru_cache(maxsize=None)
def want_scat(name):
    return bb.want_scat(described(name), cands_of(name), PROD[name], bb.SCAT_FFACTOR)


@functools.lru_cache(maxsize=None)
def want_bands(name, clip):
    return bb.want_bands(described(name), PROD[name], bg.DMS, bb.NSUB, clip, NCMP)


# ---- burst sums and spectra -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
def test_burst_sums_and_spectra(hip_lib, rows, shift):
    """every product; d_sums field by field with ==; spec, noise and used in Stokes order everywhere, in coherency order on A8 (two
    products and one: the coherency order is refused)"""
    name, res = rows
    br, cands = res.br, cands_of(name)
    res.lay(shift)
    assert bb.sums_form(hip_lib, br, shift) == form(shift)
    bb.check_spectra(hip_lib, res, cands, False, form(shift), want_sums(name), want_spectra(name, False))
    if br.nifs == 4:
        bb.check_spectra(hip_lib, res, cands, True, form(shift), want_sums(name), want_spectra(name, True))
    else:
        err = C.create_string_buffer(512)
        par = rc.burst_par(True)
        with bg.guarded():
            code = hip_lib.frbch_burstspec_device(C.byref(br.desc()), C.c_void_p(res.address), br.nrows, C.byref(par), cands.ctypes.data, 4, None, 0,
                                                  None, None, None, None, None, err, len(err))
        assert code == _lib.E_ARG and COH in err.value.decode()


# ---- RM ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
def test_burst_rm(hip_lib, rows, shift):
    """nphi = 64, the smallest fast transform: kernel_used[0] is the burst-sums kernel of the address, [1] the fast transform"""
    name, res = rows
    br, cands = res.br, cands_of(name)
    res.lay(shift)
    if br.nifs == 4:
        bb.check_rm(hip_lib, res, cands, form(shift), want_rm(name))
        return
    err = C.create_string_buffer(512)
    par, rpar = rc.burst_par(False), post.rm_params(bb.RM_GRID["nphi"], bb.RM_GRID["phi_lo"], bb.RM_GRID["dphi"])
    with bg.guarded():
        code = hip_lib.frbch_burst_rm_device(C.byref(br.desc()), C.c_void_p(res.address), br.nrows, C.byref(par), cands.ctypes.data, 4, None, None,
                                             C.byref(rpar), 0, None, None, None, None, None, None, err, len(err))
    assert code == _lib.E_ARG and (FOUR in err.value.decode() or MANY in err.value.decode()), err.value


# ---- profile ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("coh", [False, True])
def test_profile(hip_lib, rows, coh, shift):
    """nbin = 64, tfactor = 4, both orders: a 64-byte tile spans at most 16 rows of delay at DM 100, far inside tfactor + range <=
    256"""
    name, res = rows
    br, cands = res.br, cands_of(name)
    res.lay(shift)
    c = bb.prof_case(br, cands, coh)
    if br.nifs != 4:
        refused(hip_lib, hip_lib.frbch_polprof_device, c, res, lambda fn, c, p: pc.call(fn, c, p, out=pc.outputs(4, 4, 4, fill=0xA5)),
                COH if coh else FOUR)
        return
    kernel, _brun, spread = bec.plan(c, shift)
    assert kernel == form(shift) and bb.TFACTOR + spread <= bec.SPAN
    bb.check_prof(hip_lib, res, c, (form(shift), form(shift)), want_prof(name, coh))


# ---- DM scan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("coh", [False, True])
def test_dm_scan(hip_lib, rows, coh, shift):
    """17 trials (a whole trial run of 16 and one of 1) a DM sample step apart, nbin = 64, tfactor = 4: A8 in both orders, A16 in
    Stokes order; the coherency order on two products and 65 536 channels are refused"""
    name, res = rows
    br, cands = res.br, cands_of(name)
    res.lay(shift)
    ddm = bb.sample_step(hip_lib, br)
    prod = 0 if coh else PROD[name]
    c = bb.scan_case(br, cands, prod, coh, ddm)
    if (prod, coh) not in SCAN_ORDERS[name]:
        refused(hip_lib, hip_lib.frbch_dmscan_device, c, res, lambda fn, c, p: dc.call(fn, c, p, out=dc.outputs(4, 4, 4, 4, fill=0xA5)),
                COH if coh and br.nifs != 4 else MANY)
        return
    cap = dc.STAGE_BYTES // (64 * (2 if coh else 1))                    # 1024 rows of stage, 512 with two products read
    assert bb.TFACTOR + dc.tile_range(c["hdr"], br.dtype.itemsize, cands, bb.SCAN_NTRIAL, ddm, dc.TRUN) <= cap
    assert dc.plan_expected(c, shift == 0) == form(shift)
    bb.check_scan(hip_lib, res, c, (form(shift), form(shift)), want_scan(name, prod, coh, ddm))


# ---- burst ACF ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("tile", [False, True])
def test_burst_acf(hip_lib, rows, tile, shift):
    """nbin = 64, tfactor = 4, 8 x 16 lags; ffactor = 16 (below a tile's channels: the store is direct) and a tile's channels (64 | 32:
    the partials go through the join)"""
    name, res = rows
    br, cands = res.br, cands_of(name)
    res.lay(shift)
    if name == "B8":
        c = bb.acf_case(br, cands, 0, 64 if tile else 16)
        refused(hip_lib, hip_lib.frbch_burstacf_device, c, res, lambda fn, c, p: ac.call(fn, c, p, out=ac.outputs(4, 4, 4, 2, 2, 4, fill=0xA5)), MANY)
        return
    ff = ACF_FF[name][1 if tile else 0]
    assert (ff == 64 // br.dtype.itemsize) == tile and (tile or ff < 64 // br.dtype.itemsize)
    c = bb.acf_case(br, cands, PROD[name], ff)
    assert ac.dyn_plan_expected(c, shift == 0) == form(shift)
    bb.check_acf(hip_lib, res, c, (form(shift), form(shift)), want_acf(name, ff))


# ---- scattering -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
def test_burst_scattering(hip_lib, rows, shift):
    """the smallest bank of tests/scat_cases.py, ffactor = 1024: eight subbands of 16 (A8) / 32 (A16) tiles"""
    name, res = rows
    br, cands = res.br, cands_of(name)
    res.lay(shift)
    c = bb.scat_case(br, cands, PROD[name], bb.SCAT_FFACTOR)
    if name == "B8":
        refused(hip_lib, hip_lib.frbch_burstscat_device, c, res, lambda fn, c, p: sc.call(fn, c, p, out=sc.outputs(4, 4, 4, 2, 2, 4, fill=0xA5)), MANY)
        return
    assert sc.dyn_plan_expected(c, shift == 0) == form(shift)
    bb.check_scat(hip_lib, res, c, (form(shift), form(shift)), want_scat(name))


# ---- refusals stay refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_stay_refusals(hip_lib, rows):
    """65 536 channels: "more than 16384 channels" from the profile (asked with four products: on B8's single product its own
    refusal comes first), the DM scan, the ACF and the scattering fit, the outputs still 0xA5; the plan queries refuse as well"""
    name, res = rows
    br, cands = res.br, cands_of(name)
    res.lay(0)
    ddm = bb.sample_step(hip_lib, br)
    ptr = C.c_void_p(res.address)
    q = hip_lib.frbch_polprof_kernel(C.byref(br.desc()), ptr, br.nrows, C.byref(rc.burst_par(False)), cands.ctypes.data, 4,
                                     C.byref(post.prof_params(bb.NBIN, bb.TFACTOR, "mean")))
    if name == "A8":
        assert q == FAST
        return
    assert q < 0
    which = ("prof", "scan", "acf", "scat") if name == "B8" else ("prof",)
    for what, (code, msg, kept) in bb.refusals(hip_lib, res, br.hdr(), cands, ddm, which).items():
        assert code == _lib.E_ARG and ((FOUR if what == "prof" else MANY) in msg) and kept, (what, code, msg)
    if name == "B8":
        for what, (code, msg, kept) in bb.refusals(hip_lib, res, dict(br.hdr(), nifs=4), cands, ddm).items():
            assert code == _lib.E_ARG and MANY in msg and kept, (what, code, msg)
    res.check_equals()


# ---- bands ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("zerodm,clip", [(True, 5.0), (False, 0.0)])
def test_dedisperse_bands(hip_lib, rows, zerodm, clip, shift):
    """nine DMs (a group of 8 and one more), nsub = 8, all 36 bands: nclip and the runs of 512 outputs at the start, where the
    input rows straddle each mark and at the ragged end, of every series; band [0, 8) against frbch_dedisperse_device"""
    name, res = rows
    res.lay(shift)
    bb.check_bands(hip_lib, res, PROD[name], bg.DMS, bb.NSUB, zerodm, clip, bc.TILED if shift == 0 else bc.GENERIC, want_bands(name, clip))


@pytest.mark.parametrize("shift", [0, 4])
def test_bandsearch_finds_a_burst_in_a_quarter_of_the_band_behind_the_mark(hip_lib, rows, shift):
    """a burst of 4 rows at DM 104 in sub-bands 2 and 3 of 8 only, 300 rows behind the 2^32 row; widths 1, 2, 4, 8, threshold 8, L =
    1000: the records are the same bytes with the whole plane and with three DMs a batch, equal frbch_spsearch_device on the plane
    of frbch_dedisperse_bands_device, and the strongest group has band (2, 4), DM index 4, width 4 and the burst's centre"""
    name, res = rows
    res.lay(shift)
    bb.check_bandsearch(hip_lib, res, PROD[name], bg.DMS, bb.NSUB, bc.TILED if shift == 0 else bc.GENERIC, behind=300)


# ---- the band plane itself past the mark --------------------------------------------------------------------------------------------
LONG_ROWS, LONG_NDM, LONG_NSUB, LONG_RUN = (1 << 20) + 300, 130, 4, 4096


@pytest.fixture(scope="module")
def long_bands(hip_lib):
    """256 channels x 8 bit, 2^20 + 300 rows, 130 DMs in steps of 0.5, nsub = 4 (10 bands), zerodm on, no clip: out of 5.45 GB, an
    fp64 prefix plane of 4.36 GB and a uint32 one of 2.18 GB in HBM -> (rows, header, DMs, nout, bands, the buffer, kernel_used)"""
    hdr = poc.make_hdr(256)
    x = np.random.default_rng(78).integers(60, 124, size=(LONG_ROWS, 1, 256), dtype=np.uint8)
    dms = [0.5 * i for i in range(LONG_NDM)]
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    desc = poc.desc_of(hdr, x)
    bands = bo.band_list(LONG_NSUB)
    nband = len(bands)
    nout = hip_lib.frbch_dedisperse_nout(C.byref(desc), LONG_ROWS, dm_arr.ctypes.data, dm_arr.size)
    assert nband == 10 and LONG_NDM * nband * nout * 4 >= (1 << 32) + (64 << 20)           # out passes 2^32 bytes by 64 MiB or more
    assert LONG_NDM * LONG_NSUB * nout * 8 > 1 << 32                                       # the fp64 zero-DM prefix plane passes it as well
    assert 1 << 31 < LONG_NDM * LONG_NSUB * nout * 4 < 1 << 32                             # the uint32 prefix plane: 2^31 only
    assert LONG_NDM * nband * nout < 1 << 32                                               # no plane of 2^32 elements
    assert bc.tile_span(hdr, 8, dms) <= bc.ROWS_CAP - bc.TT
    bp = post.band_params(LONG_NSUB)
    d_rows = GuardedBuffer.from_numpy(x)
    d_out = GuardedBuffer(LONG_NDM * nband * nout * 4)
    assert hip_lib.frbch_dedisperse_bands_kernel(C.byref(desc), d_rows.ptr, LONG_ROWS, dm_arr.ctypes.data, dm_arr.size, C.byref(bp)) == bc.TILED
    nclip, used = C.c_uint64(0), C.c_uint32(99)
    err = C.create_string_buffer(512)
    with bg.guarded():
        code = hip_lib.frbch_dedisperse_bands_device(C.byref(desc), d_rows.ptr, LONG_ROWS, dm_arr.ctypes.data, dm_arr.size, 1, 0.0, C.byref(bp), 0,
                                                     d_out.ptr, nout, C.byref(nclip), C.byref(used), err, len(err))
    assert code == 0, err.value
    d_rows.check(contents=True)
    d_rows.free()
    yield x, hdr, dms, nout, bands, d_out, used.value
    d_out.free()


def test_band_plane_past_the_mark(long_bands):
    """runs of 4096 outputs at the start and the end of: the first and the last series; the series that holds byte 2^32 of `out`
    and its two neighbours; all ten bands of the DM in which the fp64 prefix plane passes 2^32 bytes (the uint32 one 2^31) and of
    the DMs on either side of it -- against the windowed restatement"""
    x, hdr, dms, nout, bands, d_out, used = long_bands
    assert used == bc.TILED
    nband = len(bands)
    s_out = (1 << 30) // nout                              # the series with the float at byte 2^32
    dm_z = (1 << 29) // (LONG_NSUB * nout)                 # the DM with the double at byte 2^32 of the prefix plane
    assert 0 < s_out - 1 and s_out + 1 < LONG_NDM * nband and (s_out, dm_z) == (1023, 127) and dm_z + 1 < LONG_NDM
    series = sorted({0, LONG_NDM * nband - 1, s_out - 1, s_out, s_out + 1} | {i * nband + j for i in (dm_z - 1, dm_z, dm_z + 1) for j in range(nband)})
    cps = 256 // LONG_NSUB
    dl = {i: np.asarray(po.delays_samples(hdr["fch1"], hdr["foff"], 256, hdr["tsamp"], dms[i])) for i in sorted({s // nband for s in series})}
    maxd = nout and LONG_ROWS - nout
    for t0 in (0, nout - LONG_RUN):
        cum = bg.prefix_sums(x[t0:t0 + LONG_RUN + maxd, 0, :])
        for s in series:
            a, b = bands[s % nband]
            want = bb.window_band_series(cum, dl[s // nband], LONG_RUN, a * cps, b * cps, True)
            got = bg.read_series(bg.DeviceMem, d_out, nout, s, t0, LONG_RUN)
            assert np.array_equal(got, want), "DM %d, band %s, outputs %d .. %d" % (s // nband, bands[s % nband], t0, t0 + LONG_RUN)
    d_out.check()
