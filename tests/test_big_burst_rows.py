"""tests/big_burst_rows.py on the emulator: the case builders of tests/test_gpu_beyond_4gib_burst.py with marks of 2^20 / 2^21
bytes and 805 rows of 4 KiB.  Held here: the conditions of the four candidates at the REAL shapes (arithmetic only) and at the
small ones, every windowed expectation equal to the same restatement on the WHOLE small array with the four candidates in one
call, the band series equal to bands_oracle.dedisperse_bands on the whole array; then the same checks the device module runs,
through the emulator's `_device` entry points in host memory, at both addresses (the emulator build has the generic kernels
only: kernel_used is held to each entry point's query and to GENERIC)."""
import ctypes as C
import functools

import numpy as np
import pytest

from frb_baseband_amd import _lib
from tests import acf_cases as ac
from tests import acf_oracle as ao
from tests import bands_oracle as bo
from tests import big_burst_rows as bb
from tests import big_rows as bg
from tests import burst_edge_cases as bec
from tests import dmscan_cases as dc
from tests import dmscan_oracle as do
from tests import polprof_cases as pc
from tests import polprof_oracle as ppo
from tests import rm_cases as rc
from tests import rm_oracle as ro
from tests import scat_cases as sc
from tests import scat_oracle as so

NAMES = ("A8", "A16", "B8")
PROD = {"A8": 2, "A16": 1, "B8": 0}
NBIN, TFACTOR = 16, 2                                    # bins within the small off windows
SCAT = dict(ffactor=128, shift0=4, nshift=8)
ACF_FF = {"A8": (16, 64), "A16": (16, 32)}               # below a 64-byte tile's channels, and a tile
NCMP = 64
SEARCH_DMS = [40.0 + 16.0 * i for i in range(9)]         # 16 rows of delay a step at 1 ms rows, as DM steps of 1 are at 64 us
GEN = (bb.GENERIC, bb.GENERIC)


@functools.lru_cache(maxsize=None)
def small(name):
    return bg.small(name)


@functools.lru_cache(maxsize=None)
def cands_of(name):
    c = bb.burst_cands(small(name), bb.DM, bb.SMALL_WIDTH, bb.SMALL_OFF_GAP, bb.SMALL_OFF_LEN)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def whole_of(name):
    br = small(name)
    x = br.window(0, br.nrows)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module", params=NAMES)
def case(request, emu_lib):
    """(name, BigRows, the four candidates, Resident in host memory)"""
    br = small(request.param)
    res = bg.Resident(br, bg.mem_for(emu_lib)).lay(0)
    yield request.param, br, cands_of(request.param), res
    res.free()


def only(case, *names):
    """the entry points that take the shape; the others are refusals, asserted by test_refusals_stay_refusals"""
    return case[0] in names


# ---- the conditions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_conditions_hold_at_the_real_shapes(name):
    """arithmetic on bg.big(name): no buffer.  DM 100: D = 1584 rows at 64 us (A8, A16), 1014 at 100 us (B8)"""
    br = bg.big(name)
    cands = bb.burst_cands(br, bb.DM, bb.WIDTH, bb.OFF_GAP, bb.OFF_LEN)
    fig = bb.conditions(br, cands)
    assert fig["D"] == (1014 if name == "B8" else 1584) and fig["staged_tiles"] >= 3
    assert fig["both_sides"] == (name != "B8") and not fig["cut_everywhere"]
    m1, m2 = br.byte_mark_rows
    assert cands["sample"].tolist() == [276, m1 - fig["D"] // 2, m2 - fig["D"] // 2, br.nrows - fig["D"] - 276]
    for i in range(4):                                     # a host window of one candidate
        wins = ro.windows(cands[i])
        assert wins[2][0] + wins[2][1] + fig["D"] - wins[0][0] < 3000
    # the plan rules admit the fast forms: the delay range of a 64-byte tile beside one run of bins
    spread = int(bec.tile_spreads(br.hdr(), br.nbits, bb.DM).max())
    assert spread <= 24 and bb.TFACTOR + spread <= 256


@pytest.mark.parametrize("name", NAMES)
def test_conditions_hold_at_the_small_shapes(name):
    br = small(name)
    fig = bb.conditions(br, cands_of(name))
    assert fig["D"] == 101 and fig["both_sides"] and not fig["cut_everywhere"]
    assert cands_of(name)["sample"].tolist() == [28, 206, 462, 676]


def test_a_candidate_off_the_mark_is_refused():
    br = small("A8")
    cands = cands_of("A8").copy()
    cands[bb.HI]["sample"] += 120                          # every on-pulse row behind the mark
    with pytest.raises(AssertionError, match="on-pulse rows"):
        bb.conditions(br, cands)
    cands = cands_of("A8").copy()
    cands[bb.END]["sample"] -= 60                          # the later window ends inside the file in every channel
    with pytest.raises(AssertionError):
        bb.conditions(br, cands)


def test_windows_are_cut_where_the_file_is(case):
    name, br, cands, _res = case
    D = bb.max_delay(br, bb.DM)
    got = [bb.windowed(br, cands[i:i + 1], D) for i in range(4)]
    assert got[bb.START][0] == 0 and got[bb.END][0] + got[bb.END][1].shape[0] == br.nrows
    for i in (bb.LO, bb.HI):
        t0, x, moved = got[i]
        wins = ro.windows(cands[i])
        assert t0 == wins[0][0] and x.shape[0] == wins[2][0] + wins[2][1] + D - t0 and int(moved[0]["sample"]) == int(cands[i]["sample"]) - t0
        assert np.array_equal(x, whole_of(name)[t0:t0 + x.shape[0]])
    with pytest.raises(AssertionError):
        bb.windowed(br, cands[:2], D)


# ---- the windowed expectations against the restatements on the whole array ----------------------------------------------------
def test_windowed_sums_and_spectra_equal_the_restatements_on_the_whole_array(case):
    name, br, cands, _res = case
    whole = whole_of(name)
    sums = bb.want_sums(br, cands, block=512)
    assert sums.tobytes() == bec.window_sums(whole, br.hdr(), cands).tobytes()
    assert sums.tobytes() == ro.burst_sums(whole, br.hdr(), cands).tobytes()
    assert sums["off_hits"][bb.START].min() == sums["off_hits"][bb.END].min() == 3 * bb.SMALL_OFF_LEN // 2
    assert (sums["off_hits"][[bb.LO, bb.HI]] == 2 * bb.SMALL_OFF_LEN).all() and (sums["on_hits"] == bb.SMALL_WIDTH).all()
    for coh in ((False, True) if br.nifs == 4 else (False,)):
        for a, b in zip(bb.want_spectra(sums, coh), ro.burst_spectra(whole, br.hdr(), cands, None, coh)):
            assert a.tobytes() == b.tobytes()


def test_windowed_rm_equals_the_oracle_on_the_whole_array(case):
    name, br, cands, _res = case
    if not only(case, "A8"):
        return
    want = ro.burst_rm(whole_of(name), br.hdr(), cands, **bb.RM_GRID)
    got = bb.want_rm(br, cands)
    for f in ("spec", "noise", "used", "F", "results"):
        assert got[f].tobytes() == want[f].tobytes(), f


def test_windowed_profile_equals_the_oracle_on_the_whole_array(case):
    name, br, cands, _res = case
    if not only(case, "A8"):
        return
    for coh in (False, True):
        want = ppo.profile(whole_of(name), br.hdr(), cands, bb.RM, NBIN, TFACTOR, "mean", None, None, coh)
        got = bb.want_prof(br, cands, coh, NBIN, TFACTOR)
        for f in want:
            assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want[f]).tobytes(), (coh, f)
        assert want["used"].all() and want["hits"].min() > 0


def scan_orders(name):
    return {"A8": ((PROD["A8"], False), (0, True)), "A16": ((PROD["A16"], False),)}.get(name, ())


def test_windowed_scan_equals_the_oracle_on_the_whole_array(case):
    name, br, cands, _res = case
    ddm = do.sample_step(br.hdr())
    for prod, coh in scan_orders(name):
        want = do.scan(whole_of(name), dict(br.hdr(), product=prod), cands, bb.SCAN_NTRIAL, ddm, NBIN, TFACTOR, dc.WIDTHS, dc.SMOOTH, dc.FIT_FRAC,
                       coherency=coh)
        got = bb.want_scan(br, cands, prod, coh, ddm, nbin=NBIN, tfactor=TFACTOR)
        assert dc.same(got, want), (prod, coh)
        assert bb.scan_reach(br, cands, bb.SCAN_NTRIAL, ddm) > bb.max_delay(br, bb.DM)           # the window reaches further than at the candidate's DM


def test_windowed_acf_and_scattering_equal_the_oracles_on_the_whole_array(case):
    name, br, cands, _res = case
    hdr = dict(br.hdr(), product=PROD[name])
    for ff in ACF_FF.get(name, ()):
        want = ao.burst_acf(whole_of(name), hdr, cands, NBIN, TFACTOR, ff, bb.ACF_LAGS["nlagf"], bb.ACF_LAGS["nlagt"], ac.FIT_FRAC)
        assert ac.differing(bb.want_acf(br, cands, PROD[name], ff, NBIN, TFACTOR), want) == [], ff
    if only(case, "A8"):
        bank, bp = bb.scat_bank()
        want = so.burst_scatter(whole_of(name), hdr, cands, NBIN, TFACTOR, SCAT["ffactor"], bank, bp, SCAT["shift0"], SCAT["nshift"], sc.ALPHAS, sc.SNR_MIN)
        assert sc.differing(bb.want_scat(br, cands, PROD[name], SCAT["ffactor"], NBIN, TFACTOR, SCAT["shift0"], SCAT["nshift"]), want) == []


@pytest.mark.parametrize("clip", [5.0, 0.0])
def test_windowed_bands_equal_the_oracle_on_the_whole_array(case, clip):
    name, br, _cands, _res = case
    prod, h = PROD[name], br.hdr()
    nout, nclip, bands, runs = want_bands(name, clip)
    assert bands == bo.band_list(bb.NSUB) and len(bands) == 36
    for zerodm in (True, False):
        want, wclip, wbands = bo.dedisperse_bands(whole_of(name)[:, prod, :], fch1=h["fch1"], foff=h["foff"], tsamp=h["tsamp"], dms=bg.DMS,
                                                  nsub=bb.NSUB, zerodm=zerodm, clip=clip)
        assert want.shape == (9 * 36, nout) and wclip == nclip and wbands == bands
        assert len(runs[zerodm]) == 4
        for t0, plane in runs[zerodm]:
            assert np.array_equal(plane, want[:, t0:t0 + NCMP])
    # the channel range of one series on its own, against big_rows.window_series where the range is the band
    d = bg.delays_of(br, bg.DMS)[8]
    x = whole_of(name)[300:300 + NCMP + int(d.max()), prod, :]
    cum = bg.prefix_sums(x)
    assert np.array_equal(bb.window_band_series(cum, d, NCMP, 0, br.nchan, True), bg.window_series(cum, d, NCMP, True))


@functools.lru_cache(maxsize=None)
def want_bands(name, clip):
    return bb.want_bands(small(name), PROD[name], bg.DMS, bb.NSUB, clip, NCMP)


# ---- the checks of the device module, through the emulator ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def want_sums(name):
    return bb.want_sums(small(name), cands_of(name))


@pytest.mark.parametrize("shift", [0, 4])
def test_spectra_on_the_emulator(emu_lib, case, shift):
    name, br, cands, res = case
    res.lay(shift)
    for coh in ((False, True) if br.nifs == 4 else (False,)):
        bb.check_spectra(emu_lib, res, cands, coh, bb.sums_form(emu_lib, br, shift), want_sums(name), bb.want_spectra(want_sums(name), coh))


@pytest.mark.parametrize("shift", [0, 4])
def test_rm_and_profile_on_the_emulator(emu_lib, case, shift):
    name, br, cands, res = case
    if not only(case, "A8"):
        return
    res.lay(shift)
    bb.check_rm(emu_lib, res, cands, bb.GENERIC, bb.want_rm(br, cands))
    for coh in (False, True):
        bb.check_prof(emu_lib, res, bb.prof_case(br, cands, coh, NBIN, TFACTOR), GEN, bb.want_prof(br, cands, coh, NBIN, TFACTOR))


@pytest.mark.parametrize("shift", [0, 4])
def test_scan_on_the_emulator(emu_lib, case, shift):
    name, br, cands, res = case
    res.lay(shift)
    ddm = bb.sample_step(emu_lib, br)
    for prod, coh in scan_orders(name):
        bb.check_scan(emu_lib, res, bb.scan_case(br, cands, prod, coh, ddm, nbin=NBIN, tfactor=TFACTOR), GEN,
                      bb.want_scan(br, cands, prod, coh, ddm, nbin=NBIN, tfactor=TFACTOR))


@pytest.mark.parametrize("shift", [0, 4])
def test_acf_and_scattering_on_the_emulator(emu_lib, case, shift):
    name, br, cands, res = case
    res.lay(shift)
    for ff in ACF_FF.get(name, ()):
        bb.check_acf(emu_lib, res, bb.acf_case(br, cands, PROD[name], ff, NBIN, TFACTOR), GEN, bb.want_acf(br, cands, PROD[name], ff, NBIN, TFACTOR))
    if only(case, "A8"):
        bb.check_scat(emu_lib, res, bb.scat_case(br, cands, PROD[name], SCAT["ffactor"], NBIN, TFACTOR, SCAT["shift0"], SCAT["nshift"]), GEN,
                      bb.want_scat(br, cands, PROD[name], SCAT["ffactor"], NBIN, TFACTOR, SCAT["shift0"], SCAT["nshift"]))


def test_refusals_stay_refusals(emu_lib, case):
    """65 536 channels: "more than 16384 channels" from the profile (asked with four products), the DM scan, the ACF and the
    scattering fit; two products: the profile's and the coherency order's refusals.  The outputs keep their fill."""
    name, br, cands, res = case
    res.lay(0)
    ddm = do.sample_step(br.hdr())
    if name == "B8":
        wide = bg.big("B8").hdr()
        for what, (code, msg, kept) in bb.refusals(emu_lib, res, dict(wide, nifs=4), cands, ddm).items():
            assert code == _lib.E_ARG and "more than 16384 channels" in msg and kept, (what, code, msg)
        code, msg, kept = bb.refusals(emu_lib, res, wide, cands, ddm, which=("prof",))["prof"]
        assert code == _lib.E_ARG and "needs the four products" in msg and kept
    if name == "A16":
        code, msg, kept = bb.refusals(emu_lib, res, br.hdr(), cands, ddm, which=("prof",))["prof"]
        assert code == _lib.E_ARG and "needs the four products" in msg and kept
        with bg.guarded():
            code, msg, out, _k = dc.call(emu_lib.frbch_dmscan_device, bb.scan_case(br, cands, 0, True, ddm, nbin=NBIN, tfactor=TFACTOR),
                                         C.c_void_p(res.address),
                                         out=dc.outputs(4, bb.SCAN_NTRIAL, NBIN, br.nchan, fill=0xA5))
        assert code == _lib.E_ARG and "coherency products need nifs = 4" in msg and bb.untouched(out)
    res.check_equals()


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("zerodm,clip", [(True, 5.0), (False, 0.0)])
def test_bands_on_the_emulator(emu_lib, case, zerodm, clip, shift):
    name, _br, _cands, res = case
    res.lay(shift)
    bb.check_bands(emu_lib, res, PROD[name], bg.DMS, bb.NSUB, zerodm, clip, bb.GENERIC, want_bands(name, clip))


@pytest.mark.parametrize("shift", [0, 4])
def test_bandsearch_on_the_emulator(emu_lib, case, shift):
    name, _br, _cands, res = case
    res.lay(shift)
    dms = [d if d != 104.0 else bb.BURST_DM for d in SEARCH_DMS]
    assert dms.index(bb.BURST_DM) == 4
    bb.check_bandsearch(emu_lib, res, PROD[name], dms, bb.NSUB, bb.GENERIC, behind=30)
    res.lay(0)
