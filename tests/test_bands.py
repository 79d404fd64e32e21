"""Band-limited single-pulse search (frbch_band_list, frbch_dedisperse_bands_*, frbch_bandsearch_*, frbch_spb_group_cands,
post.band_search / bandsearch_fil) without a GPU: the generic kernel through the TEST-ONLY emulator build against the numpy
restatement tests/bands_oracle.py byte for byte, band [0, nsub) against frbch_dedisperse_device of the same build, the composite
against the oracle and across batch sizes, the grouping against its restatement on hand-built records, every refusal by its
message, and the known answer of the oracle (a burst in a quarter of the band that the full-band search misses).

Grouping: the band neither links nor separates records (include/frbch.h) -- two pulses at one time in disjoint bands join."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import bands_cases as bc
from tests import bands_oracle as bo
from tests import post_cases as pc
from tests.test_fold_predictor import write_fil


# ---- the band list ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsub,lo,hi", [(1, 0, 0), (8, 0, 0), (8, 1, 0), (8, 2, 3), (16, 0, 0), (16, 16, 16), (4, 1, 1)])
def test_band_list_is_the_oracles(emu_lib, nsub, lo, hi):
    got = post.band_list(64, nsub, lo, hi, lib=emu_lib)
    want = bo.band_list(nsub, lo, hi)
    assert [tuple(int(v) for v in ab) for ab in got] == want
    if (lo or 1) <= nsub <= (hi or nsub):
        assert want.index((0, nsub)) == max(j for j, (a, _b) in enumerate(want) if a == 0)     # the last band that starts at 0
    assert len(bo.band_list(8)) == 36 and len(bo.band_list(16)) == 136


def test_band_list_counts_and_reports_capacity(emu_lib):
    bp = post.band_params(8, 0, 0)
    n = C.c_uint32(0)
    err = C.create_string_buffer(256)
    assert emu_lib.frbch_band_list(64, C.byref(bp), None, None, 0, C.byref(n), err, len(err)) == _lib.E_CAPACITY and n.value == 36
    lo, hi = np.zeros(36, np.uint16), np.zeros(36, np.uint16)
    assert emu_lib.frbch_band_list(64, C.byref(bp), lo.ctypes.data, hi.ctypes.data, 36, C.byref(n), err, len(err)) == 0


# ---- the generic kernel against the oracle, and band [0, nsub) against the dedispersion that exists ---------------------
@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_emulator_equals_the_oracle(emu_lib, name):
    c, _got = bc.check_case(emu_lib, name, form=bc.GENERIC)
    if name in bc.CLIP_CASES:
        assert c["nclip"] > 0                                     # a row really clips


def test_rows_four_bytes_off_give_the_same_bytes(emu_lib):
    bc.check_case(emu_lib, "u8_256ch_nsub4", shift=4, form=bc.GENERIC)


def test_nsub_1_is_the_full_band_series_alone(emu_lib):
    c, got = bc.check_case(emu_lib, "u8_64ch_nsub1", form=bc.GENERIC)
    assert c["bands"] == [(0, 1)] and got.shape[0] == len(c["dms"])
    assert got.tobytes() == pc.want_dedisp(c["rows"], c["hdr"], 0, c["dms"], c["zerodm"], c["clip"])[0].tobytes()


def test_the_cases_hold_what_they_are_written_for():
    c = bc.case("u16_full_scale_1024ch")
    j = c["bands"].index((0, 8))
    assert np.all(c["want"][j] == np.float32(2 ** 26 - 1024))      # 1024 x 65535: 16 significant bits, exact in float32
    c = bc.case("u16_alternating_subbands")
    assert np.all(c["want"][c["bands"].index((0, 1))] == 0) and np.all(c["want"][c["bands"].index((1, 2))] == np.float32(128 * 65535))
    assert np.all(c["want"][c["bands"].index((2, 3))] == 0)        # the difference of two equal prefixes
    assert bc.tile_span(bc.case("u8_span_at_the_lds_cap")["hdr"], 8, bc.case("u8_span_at_the_lds_cap")["dms"]) == bc.ROWS_CAP - bc.TT
    assert bc.tile_span(bc.case("u8_span_one_row_more")["hdr"], 8, bc.case("u8_span_one_row_more")["dms"]) == bc.ROWS_CAP - bc.TT + 1
    assert [b - a for a, b in bc.case("u8_512ch_widths_2_3_of_8")["bands"]].count(2) == 7 and len(bc.case("u8_512ch_widths_2_3_of_8")["bands"]) == 13


def test_python_dedisperse_bands(emu_lib):
    c = bc.case("u16_nifs4_product2")
    info = {}
    got, nclip = post.dedisperse_bands(c["rows"], dict(c["hdr"], nifs=4, nbits=16), c["dms"], c["nsub"], zerodm=c["zerodm"], clip=c["clip"],
                                       product=2, lib=emu_lib, info=info)
    assert got.shape == (len(c["dms"]), len(c["bands"]), c["nout"]) and info["kernel_used"] == 0 and nclip == c["nclip"]
    assert got.tobytes() == c["want"].tobytes()


# ---- the composite --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def search_want():
    c = bc.case("u8_7dm_search")
    want = bo.search(c["want"], c["bands"], bc.SEARCH_WIDTHS, bc.SEARCH_THR, bc.SEARCH_L)
    want.setflags(write=False)
    return c, want


def one_dm_bytes(c):
    return len(c["bands"]) * c["nout"] * 4


def test_bandsearch_equals_the_oracle_whatever_the_batch(emu_lib, search_want):
    c, want = search_want
    assert want.size > 20 and len(set(zip(want["sub_lo"].tolist(), want["sub_hi"].tolist()))) > 3
    for plane_bytes, nbatch in ((one_dm_bytes(c), 7), (3 * one_dm_bytes(c) + 5, 3), (7 * one_dm_bytes(c), 1), (0, 1)):
        rc, got, msg, nb, used = bc.bandsearch_host(emu_lib, c, bc.SEARCH_WIDTHS, bc.SEARCH_THR, bc.SEARCH_L, plane_bytes)
        assert rc == 0, msg
        assert nb == nbatch and used == (0, 0)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def test_bandsearch_full_band_records_are_dedisperse_search_hosts(emu_lib, search_want):
    c, want = search_want
    rc, got, msg, _nb, _used = bc.bandsearch_host(emu_lib, c, bc.SEARCH_WIDTHS, bc.SEARCH_THR, bc.SEARCH_L, 2 * one_dm_bytes(c))
    assert rc == 0, msg
    full = bo.full_band(got, c["nsub"])
    ref = bc.dedisperse_search_host(emu_lib, c, bc.SEARCH_WIDTHS, bc.SEARCH_THR, bc.SEARCH_L)
    assert full.size > 0 and full.tobytes() == ref.tobytes()


def test_bandsearch_refuses_a_plane_below_one_dm(emu_lib, search_want):
    c, _want = search_want
    rc, _got, msg, _nb, _used = bc.bandsearch_host(emu_lib, c, bc.SEARCH_WIDTHS, bc.SEARCH_THR, bc.SEARCH_L, one_dm_bytes(c) - 1)
    assert rc == _lib.E_ARG and "holds no DM" in msg and str(one_dm_bytes(c)) in msg


def test_bandsearch_counts_and_reports_capacity(emu_lib, search_want):
    c, want = search_want
    rc, got, msg, _nb, _used = bc.bandsearch_host(emu_lib, c, bc.SEARCH_WIDTHS, bc.SEARCH_THR, bc.SEARCH_L, 0, cap=5)
    assert rc == _lib.E_CAPACITY and "room for 5" in msg and got.tobytes() == want[:5].tobytes()


def test_python_band_search_and_file(emu_lib, search_want, tmp_path):
    c, want = search_want
    hdr = dict(c["hdr"], nbits=8)
    info = {}
    got = post.band_search(c["rows"], hdr, c["dms"], c["nsub"], zerodm=c["zerodm"], clip=c["clip"], widths=bc.SEARCH_WIDTHS,
                           threshold=bc.SEARCH_THR, detrend_len=bc.SEARCH_L, plane_bytes=2 * one_dm_bytes(c), lib=emu_lib, info=info, cap=3)
    assert got.tobytes() == want.tobytes() and info["nbatch"] == 4 and info["nclipped"] == c["nclip"]
    path = str(tmp_path / "b.fil")
    write_fil(path, c["rows"], hdr, 1)
    npz, txt, recs, groups = post.bandsearch_fil(path, c["dms"][0], c["dms"][-1], 1.0, nsub=c["nsub"], zerodm=c["zerodm"], clip=c["clip"],
                                                 widths=bc.SEARCH_WIDTHS, threshold=bc.SEARCH_THR, detrend_len=bc.SEARCH_L, lib=emu_lib)
    assert recs.tobytes() == want.tobytes()
    z = np.load(npz)
    assert z["cands"].tobytes() == want.tobytes() and z["groups"].tobytes() == groups.tobytes() and z["bands"].tolist() == [list(b) for b in c["bands"]]
    lines = open(txt).read().splitlines()
    assert lines[0] == post.BANDS_HEADER and len(lines) == 1 + groups.size
    top = groups[np.argmax(groups["best"]["sigma"])]
    f = lines[1].split()
    assert (float(f[0]), int(f[3]), int(f[4])) == (c["dms"][top["best"]["dm_index"]], int(top["best"]["sample"]), int(top["best"]["width"]))
    flo, fhi = post.band_edges_mhz(hdr, c["nsub"], int(top["best"]["sub_lo"]), int(top["best"]["sub_hi"]))
    assert (float(f[6]), float(f[7])) == (round(flo, 4), round(fhi, 4)) and float(f[9]) == round(float(top["full_sigma"]), 2)


# ---- grouping -----------------------------------------------------------------------------------------------------------------
GROUP_HDR = pc.make_hdr(64)
GROUP_DMS = [50.0, 51.0, 52.0, 53.0, 54.0, 55.0]


def recs_of(rows):
    return np.array(rows, dtype=post.SPB_CAND)


def group_both(lib, recs, nsub=8, dm_gap=2):
    got = post.group_band_candidates(recs, GROUP_HDR, GROUP_DMS, nsub, dm_gap, lib=lib)
    want = bo.group(recs, nsub, fch1=GROUP_HDR["fch1"], foff=GROUP_HDR["foff"], nchan=64, tsamp=GROUP_HDR["tsamp"], dms=GROUP_DMS, dm_gap=dm_gap)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    return got


def test_overlapping_ranges_of_one_pulse_join(emu_lib):
    g = group_both(emu_lib, recs_of([(1, 4, 1000, 9.0, 2, 4), (1, 4, 1001, 8.0, 1, 4), (2, 6, 1002, 7.5, 2, 5), (1, 4, 1000, 6.0, 0, 8),
                                     (4, 2, 9000, 7.0, 5, 6)]))
    assert g.size == 2
    assert (g[0]["nmember"], g[0]["sub_lo_min"], g[0]["sub_hi_max"], g[0]["dm_index_lo"], g[0]["dm_index_hi"]) == (4, 0, 8, 1, 2)
    assert tuple(g[0]["best"])[:3] == (1, 4, 1000) and (g[0]["best"]["sub_lo"], g[0]["best"]["sub_hi"]) == (2, 4)
    assert g[0]["full_sigma"] == np.float32(6.0) and g[1]["full_sigma"] == 0.0             # present, and absent


def test_two_pulses_at_one_time_in_disjoint_bands_join(emu_lib):
    g = group_both(emu_lib, recs_of([(0, 4, 500, 8.0, 0, 2), (0, 4, 501, 9.0, 6, 8)]))
    assert g.size == 1 and g[0]["nmember"] == 2 and (g[0]["sub_lo_min"], g[0]["sub_hi_max"]) == (0, 8) and g[0]["full_sigma"] == 0.0


def test_the_tie_order(emu_lib):
    # equal sigma: the narrower range; then the narrower width; then the lower dm_index; the earlier sample; the lower sub_lo
    g = group_both(emu_lib, recs_of([(1, 4, 700, 8.0, 0, 8), (1, 4, 700, 8.0, 2, 5), (1, 4, 700, 8.0, 3, 5), (1, 4, 700, 8.0, 1, 3)]))
    assert (g[0]["best"]["sub_lo"], g[0]["best"]["sub_hi"]) == (1, 3) and g[0]["full_sigma"] == np.float32(8.0)
    g = group_both(emu_lib, recs_of([(1, 6, 700, 8.0, 2, 4), (1, 4, 701, 8.0, 2, 4), (0, 4, 701, 8.0, 2, 4), (0, 4, 700, 8.0, 3, 5), (0, 4, 700, 8.0, 1, 3)]))
    assert tuple(g[0]["best"]) == (0, 4, 700, np.float32(8.0), 1, 3)
    g = group_both(emu_lib, recs_of([(2, 4, 700, 8.0, 0, 8), (2, 4, 700, 9.5, 0, 8), (2, 4, 700, 9.0, 0, 8)]))
    assert g[0]["full_sigma"] == np.float32(9.5)


def test_group_capacity_counting(emu_lib):
    recs = recs_of([(0, 1, 100 + 500 * k, 8.0, 0, 1) for k in range(5)])
    n = C.c_uint64(0)
    err = C.create_string_buffer(256)
    dm = np.array(GROUP_DMS)
    desc = post.fil_desc(GROUP_HDR)
    args = (C.byref(desc), dm.ctypes.data, dm.size, 8, recs.ctypes.data, recs.size, 2)
    assert emu_lib.frbch_spb_group_cands(*args, None, 0, C.byref(n), err, len(err)) == _lib.E_CAPACITY and n.value == 5
    out = np.zeros(3, dtype=post.SPB_GROUP)
    assert emu_lib.frbch_spb_group_cands(*args, out.ctypes.data, 3, C.byref(n), err, len(err)) == _lib.E_CAPACITY
    assert n.value == 5 and b"5 groups, room for 3" in err.value and out["best"]["sample"].tolist() == [100, 600, 1100]


@pytest.mark.parametrize("recs,nsub,dm_gap,text", [
    ([(0, 1, 5, 8.0, 3, 3)], 8, 2, "not a band"), ([(0, 1, 5, 8.0, 3, 9)], 8, 2, "not a band"), ([(6, 1, 5, 8.0, 0, 1)], 8, 2, "dm_index"),
    ([(0, 1, 5, 8.0, 0, 1)], 17, 2, "nsub"), ([(0, 1, 5, 8.0, 0, 1)], 8, 0, "dm_gap")])
def test_group_refusals(emu_lib, recs, nsub, dm_gap, text):
    with pytest.raises(post.InputError, match=text):
        post.group_band_candidates(recs_of(recs), GROUP_HDR, GROUP_DMS, nsub, dm_gap, lib=emu_lib)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def call_bands(lib, c, bp, dms=None, nout=None, hdr=None):
    dm = np.ascontiguousarray(c["dms"] if dms is None else dms, dtype=np.float64)
    nout = c["nout"] if nout is None else nout
    rows = c["rows"]
    out = np.zeros(max(1, dm.size) * 136 * max(1, nout), dtype=np.float32)
    err = C.create_string_buffer(512)
    rc = lib.frbch_dedisperse_bands_host(C.byref(pc.desc_of(hdr or c["hdr"], rows, c["prod"])), rows.ctypes.data, rows.shape[0], dm.ctypes.data,
                                         dm.size, 1, 5.0, C.byref(bp) if bp is not None else None, 0, out.ctypes.data, nout, None, None, err,
                                         len(err))
    return rc, err.value.decode()


def test_every_refusal_by_its_message(emu_lib):
    c = bc.case("u8_256ch_nsub4")
    bad_size = post.band_params(4)
    bad_size.size -= 4
    for bp, text in ((bad_size, "wrong size"), (None, "wrong size"), (post.band_params(0), "nsub must be 1..16"),
                     (post.band_params(17), "nsub must be 1..16"), (post.band_params(3), "nsub must divide nchan"),
                     (post.band_params(4, 3, 2), "min_sub exceeds max_sub"), (post.band_params(4, 1, 5), "max_sub exceeds nsub"),
                     (post.band_params(4, 5, 0), "min_sub exceeds max_sub")):
        rc, msg = call_bands(emu_lib, c, bp)
        assert rc == _lib.E_ARG and text in msg, (msg, text)
        err = C.create_string_buffer(256)
        n = C.c_uint32(0)
        assert emu_lib.frbch_band_list(256, C.byref(bp) if bp is not None else None, None, None, 0, C.byref(n), err, len(err)) == _lib.E_ARG
        assert text in err.value.decode()
        if bp is not None and bp is not bad_size:               # (the query has no message: refused is all it says)
            assert bc.bands_kernel(emu_lib, dict(c, nsub=bp.nsub, min_sub=bp.min_sub, max_sub=bp.max_sub), 4096) == _lib.E_ARG
    # what frbch_dedisperse_* refuses
    rc, msg = call_bands(emu_lib, c, post.band_params(4), dms=[1.0e5])
    assert rc == _lib.E_ARG and "DM outside" in msg
    rc, msg = call_bands(emu_lib, c, post.band_params(4), dms=[3.0e4])
    assert rc == _lib.E_ARG and "exceeds the data" in msg
    rc, msg = call_bands(emu_lib, c, post.band_params(4), nout=c["nout"] + 1)
    assert rc == _lib.E_CAPACITY and "frbch_dedisperse_nout" in msg
    rc, msg = call_bands(emu_lib, c, post.band_params(4), hdr=dict(c["hdr"], tsamp=0.0))
    assert rc == _lib.E_ARG and "tsamp" in msg
    # the search's limit on series: 6554 DMs x 10 bands
    many = np.linspace(0.0, 1.0, 6554).tolist()
    rc, msg = call_bands(emu_lib, c, post.band_params(4), dms=many, nout=1)
    assert rc == _lib.E_ARG and "65540 series" in msg
    assert bc.bands_kernel(emu_lib, dict(c, dms=many), 4096) == _lib.E_ARG


# ---- the known answer of the oracle -------------------------------------------------------------------------------------------
def test_known_answer_of_the_oracle():
    """the condition tests/test_gpu_bands.py holds the library to, on the restatement alone, for all twelve seeds"""
    h = bc.KA_HDR
    for seed in bc.KA_SEEDS:
        plane, _n, bands = bo.dedisperse_bands(bc.known_answer_rows(seed), fch1=h["fch1"], foff=h["foff"], tsamp=h["tsamp"], dms=[bc.KA_DM],
                                               nsub=bc.KA_NSUB, zerodm=False, clip=0.0)
        recs = bo.search(plane, bands, bc.KA_WIDTHS, bc.KA_THR, 1000)
        groups = bo.group(recs, bc.KA_NSUB, fch1=h["fch1"], foff=h["foff"], nchan=64, tsamp=h["tsamp"], dms=[bc.KA_DM])
        best = groups[np.argmax(groups["best"]["sigma"])]["best"]
        print("seed %d: band [%d, %d) sigma %.2f" % (seed, best["sub_lo"], best["sub_hi"], best["sigma"]))
        assert bc.known_answer_holds(bo.full_band(recs, bc.KA_NSUB), groups), seed
