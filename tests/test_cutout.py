"""Candidates behind the single-pulse search (frbch_sp_group_cands, frbch_cutout_*, post.group_candidates / cutouts /
candidates_fil): the grouping against a union-find over all pairs, the generic cut-out kernel through the TEST-ONLY emulator
build against the numpy restatement tests/cutout_oracle.py, known answers on the dispersed-burst case, argument errors and the
host-side file handling.  Every comparison is `==` or `tobytes()`: there is no tolerance anywhere."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

from frb_baseband_amd import _lib, post, sigproc
from tests import cutout_cases as cc
from tests import cutout_oracle as co
from tests.test_fold_predictor import write_fil
from tests.test_post import DM0, HDR
from tests.test_spsearch import dispersed_burst_rows

BURST_DMS = post.dm_list(DM0 - 20.0, DM0 + 20.0, 5.0)


def recs(*items):
    """(dm_index, width, sample, sigma) ... -> SP_CAND records"""
    out = np.zeros(len(items), dtype=post.SP_CAND)
    for o, (d, w, s, sig) in zip(out, items):
        o["dm_index"], o["width"], o["sample"], o["sigma"] = d, w, s, sig
    return out


def group_call(lib, cands, dms, dm_gap, cap=None, hdr=HDR):
    """frbch_sp_group_cands -> (rc, groups written, ngroup, message)"""
    cands = np.ascontiguousarray(cands, dtype=post.SP_CAND)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    cap = cands.size if cap is None else cap
    out = np.zeros(max(cap, 1), dtype=post.SP_GROUP)
    n = C.c_uint64(12345)
    err = C.create_string_buffer(512)
    rc = lib.frbch_sp_group_cands(C.byref(post.fil_desc(hdr)), dm_arr.ctypes.data, dm_arr.size, cands.ctypes.data, cands.size, dm_gap,
                                  out.ctypes.data if cap else None, cap, C.byref(n), err, len(err))
    return rc, out[: min(cap, n.value)] if rc in (0, _lib.E_CAPACITY) else out[:0], n.value, err.value.decode()


def same_groups(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def burst(emu_lib):
    """the end-to-end case of the search tests: one burst of 5 samples at DM0 in 8-bit noise, 9 DMs 5 apart, threshold 6,
    default widths, zero-DM and clip 5 -> (rows, records)"""
    x = dispersed_burst_rows(9000, HDR, DM0, 3000, 5, 30)
    fil = sigproc.SigprocFile(header=dict(HDR), header_bytes=0, data=x[:, None, :])
    series, _nclip = post.dedisperse(fil, BURST_DMS, zerodm=True, clip=5.0, lib=emu_lib)
    records = post.single_pulse_search(series, threshold=6.0, tsamp=HDR["tsamp"], lib=emu_lib)
    x.setflags(write=False)
    records.setflags(write=False)
    return x, records


# ---- grouping -------------------------------------------------------------------------------------------------------
def test_the_burst_is_one_group(emu_lib, burst):
    _x, records = burst
    assert records["width"].tolist() == [30, 20, 14, 9, 4, 9, 14, 20, 30] and records["dm_index"].tolist() == list(range(9))
    for gap in (1, 2):
        rc, got, n, msg = group_call(emu_lib, records, BURST_DMS, gap)
        assert rc == 0 and n == 1, msg
        g = got[0]
        assert (int(g["best"]["dm_index"]), int(g["best"]["width"]), int(g["best"]["sample"])) == (4, 4, 3002)
        assert "%.2f" % g["best"]["sigma"] == "23.79"
        assert (int(g["nmember"]), int(g["dm_index_lo"]), int(g["dm_index_hi"])) == (9, 0, 8)
        assert (int(g["sample_lo"]), int(g["sample_hi"])) == (int(records["sample"].min()), int(records["sample"].max()))
        assert same_groups(got, co.group(records, HDR, BURST_DMS, gap))
        assert same_groups(post.group_candidates(records, HDR, BURST_DMS, dm_gap=gap, lib=emu_lib), got)


def test_two_bursts_40_samples_apart_are_two_groups(emu_lib):
    r = recs((3, 4, 1000, 9.0), (3, 4, 1040, 8.0), (4, 6, 1001, 7.0), (4, 6, 1041, 7.5))
    rc, got, n, _ = group_call(emu_lib, r, BURST_DMS, 2)
    assert rc == 0 and n == 2 and got["nmember"].tolist() == [2, 2] and got["best"]["sample"].tolist() == [1000, 1040]
    assert same_groups(got, co.group(r, HDR, BURST_DMS, 2))


def test_a_chain_connects_through_its_middle_member(emu_lib):
    D = co.largest_delays(HDR, BURST_DMS)
    far = 1 + int(D[2] - D[0])                                # one past what links DM 0 and DM 2 at width 2 (2 // 2 = 1)
    a, b, c = (0, 2, 5000, 7.0), (1, 2, 5000 + far // 2, 8.0), (2, 2, 5001 + far, 9.0)
    assert not co.linked(recs(a)[0], recs(c)[0], D, 2) and co.linked(recs(a)[0], recs(b)[0], D, 2) and co.linked(recs(b)[0], recs(c)[0], D, 2)
    rc, got, n, _ = group_call(emu_lib, recs(a, c), BURST_DMS, 2)
    assert rc == 0 and n == 2
    for order in ((a, b, c), (c, a, b), (b, c, a)):
        rc, got, n, _ = group_call(emu_lib, recs(*order), BURST_DMS, 2)
        assert rc == 0 and n == 1 and int(got[0]["nmember"]) == 3 and int(got[0]["best"]["dm_index"]) == 2
        assert same_groups(got, co.group(recs(*order), HDR, BURST_DMS, 2))


def test_a_missing_dm_needs_a_gap_of_two(emu_lib):
    r = recs((3, 4, 2000, 9.0), (5, 4, 2001, 8.0))
    for gap, want in ((1, 2), (2, 1)):
        rc, got, n, _ = group_call(emu_lib, r, BURST_DMS, gap)
        assert rc == 0 and n == want
        assert same_groups(got, co.group(r, HDR, BURST_DMS, gap))


@pytest.mark.parametrize("members,best", [
    ([(2, 6, 3000, 8.0), (2, 4, 3001, 8.0), (2, 9, 3000, 8.0)], (2, 4, 3001)),       # equal sigma: the narrower width
    ([(3, 4, 3000, 8.0), (2, 4, 3001, 8.0), (4, 4, 3000, 8.0)], (2, 4, 3001)),       # ... and width: the lower dm_index
    ([(2, 4, 3002, 8.0), (2, 4, 3000, 8.0), (2, 4, 3001, 8.0)], (2, 4, 3000)),       # ... and dm_index: the earlier sample
    ([(2, 1, 3000, 8.0), (3, 30, 3001, 8.5), (1, 1, 2999, 8.0)], (3, 30, 3001)),     # a larger sigma beats them all
])
def test_tie_rules(emu_lib, members, best):
    r = recs(*members)
    rc, got, n, _ = group_call(emu_lib, r, BURST_DMS, 2)
    assert rc == 0 and n == 1
    assert (int(got[0]["best"]["dm_index"]), int(got[0]["best"]["width"]), int(got[0]["best"]["sample"])) == best
    assert same_groups(got, co.group(r, HDR, BURST_DMS, 2))


def test_group_capacity(emu_lib):
    r = recs(*[(i % 9, 4, 1000 * (i + 1), 6.0 + i) for i in range(7)])
    want = co.group(r, HDR, BURST_DMS, 2)
    assert want.size == 7
    rc, got, n, msg = group_call(emu_lib, r, BURST_DMS, 2, cap=3)
    assert rc == _lib.E_CAPACITY and n == 7 and "groups" in msg and same_groups(got, want[:3])
    rc, got, n, msg = group_call(emu_lib, r, BURST_DMS, 2, cap=0)                     # groups = NULL: counts
    assert rc == _lib.E_CAPACITY and n == 7
    rc, got, n, msg = group_call(emu_lib, r, BURST_DMS, 2, cap=7)
    assert rc == 0 and same_groups(got, want)
    rc, got, n, msg = group_call(emu_lib, r[:0], BURST_DMS, 2, cap=0)                 # no records: no groups, no error
    assert rc == 0 and n == 0


@pytest.mark.parametrize("gap,dms,dm_index", [(0, BURST_DMS, 0), (17, BURST_DMS, 0), (2, BURST_DMS, 9), (2, [-1.0, 5.0], 0),
                                              (2, [5.0, 1.0e5], 0), (2, [float("nan")], 0)])
def test_group_bad_arguments(emu_lib, gap, dms, dm_index):
    rc, _got, _n, msg = group_call(emu_lib, recs((dm_index, 4, 100, 7.0)), dms, gap)
    assert rc == _lib.E_ARG and msg


def test_grouping_is_not_quadratic(emu_lib):
    """10^5 records -- 5000 pulses of 20 records on neighbouring DMs, each displaced by the smear of its DM -- in under a second;
    the first 2000 records (100 whole pulses) equal the restatement"""
    rng = np.random.default_rng(77)
    dms = [2.0 * i for i in range(64)]
    D = co.largest_delays(HDR, dms)
    widths = np.array(post.default_widths(HDR["tsamp"]))
    npulse, per = 5000, 20
    d0 = rng.integers(0, 64 - per, npulse)
    s0 = np.sort(rng.integers(1000, 10_000_000, npulse))
    di = (d0[:, None] + np.arange(per)[None, :]).ravel()
    mid = np.repeat(d0 + per // 2, per)
    sample = np.repeat(s0, per) + (D[di] - D[mid]) // 2 + rng.integers(-1, 2, npulse * per)
    r = np.zeros(npulse * per, dtype=post.SP_CAND)
    r["dm_index"], r["sample"] = di, sample
    r["width"] = widths[rng.integers(0, widths.size, r.size)]
    r["sigma"] = np.round(rng.uniform(6.0, 12.0, r.size), 1)                        # (one decimal: ties happen)
    t0 = time.perf_counter()
    rc, got, n, msg = group_call(emu_lib, r, dms, 2)
    dt = time.perf_counter() - t0
    assert rc == 0 and 1000 < n <= npulse * 3, msg
    assert dt < 1.0, dt
    rc, got, n, msg = group_call(emu_lib, r[:2000], dms, 2)
    assert rc == 0 and same_groups(got, co.group(r[:2000], HDR, dms, 2))
    assert int(got["nmember"].max()) >= per // 2


# ---- the planes: the generic kernel against the restatement -------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_emulator_equals_the_restatement(emu_lib, name):
    cs, want = cc.case(name)
    rc, got, used, msg = cc.cutout_host(emu_lib, cs)
    assert rc == 0, msg
    assert used == cc.GENERIC and cc.cutout_kernel(emu_lib, cs, 4096) == cc.GENERIC
    assert cc.same_planes(got, want), cc.which_differ(got, want)


def test_the_cases_hold_what_they_are_written_for():
    _cs, (ft, fth, dt, dth) = cc.case("c64_b8_wholly_outside")
    assert not fth.any() and not dth.any() and not ft.any() and not dt.any()
    cs, (ft, fth, dt, dth) = cc.case("c64_b8_starts_before_row0")
    full = (cs["hdr"]["nchans"] // cs["nf"]) * 3
    assert fth[0, 0, 0] == 0 and 0 < fth[0, 0, 14] < full and fth[0, :, -1].min() == full and dth[0, :, -1].min() == 64 * 3     # rows -43 ..
    cs, (ft, fth, dt, dth) = cc.case("c64_b8_ends_past_nrows")
    assert fth[0, 0, 0] == full and fth[0, -1, 0] == 0 and not fth[0, :, -1].any() and dth[0, 0, 0] == 64 * 3 and 0 < dth[0, 0, 19] < 64 * 3 and dth[0, 0, -1] == 0
    cs, (ft, fth, dt, dth) = cc.case("c64_b8_dm_hi_delay_past_nrows")
    assert co.delays(cs["hdr"], 3000.0).max() > cs["rows"].shape[0] and dth[0, -1].max() < 64 * 2 and dth[0, 0].min() == 64 * 2
    cs, want = cc.case("c64_b8_nifs3_product2")
    other = co.planes_batch(cs["rows"][:, 0, :], cs["hdr"], cs["cands"], cs["nt"], cs["nf"], cs["ndm"])
    assert not np.array_equal(other[0], want[0]) and not np.array_equal(other[2], want[2])     # the products differ
    cs, (ft, fth, dt, dth) = cc.case("c64_b8_tfactor512_nt4")
    assert fth[0].min() == 4 * 512 and dth[0].min() == 64 * 512 and float(dt[0].max()) > 2.0 ** 20


def test_python_entry_point(emu_lib):
    cs, want = cc.case("c64_b8_nf16_nt16_ndm8")
    info = {}
    got = post.cutouts(cs["rows"], cs["hdr"], cs["cands"], nt=16, nf=16, ndm=8, lib=emu_lib, info=info)
    assert info["kernel_used"] == 0 and cc.same_planes(got, want)
    r = recs((4, 6, 3000, 9.0), (1, 1, 2500, 7.0))
    made = post.cutout_cands(r, BURST_DMS)
    assert made["tfactor"].tolist() == [3, 1] and made["dm"].tolist() == [BURST_DMS[4], BURST_DMS[1]]
    assert made["dm_lo"].tolist() == [0.0, 0.0] and made["dm_hi"].tolist() == [2 * BURST_DMS[4], 2 * BURST_DMS[1]]
    span = post.cutout_cands(r, BURST_DMS, dm_span=20.0)
    assert span["dm_lo"].tolist() == [BURST_DMS[4] - 10.0, BURST_DMS[1] - 10.0] and span["dm_hi"].tolist() == [BURST_DMS[4] + 10.0, BURST_DMS[1] + 10.0]
    # nf = 0: the largest divisor of nchans up to 256
    ft, _h, _dt, _dh = post.cutouts(cs["rows"], cs["hdr"], cs["cands"], nt=2, ndm=1, lib=emu_lib)
    assert ft.shape == (1, 64, 2)
    with pytest.raises(post.InputError):
        post.cutouts(cs["rows"], cs["hdr"], cs["cands"], nt=3, lib=emu_lib)


def test_a_long_list_goes_in_several_calls(emu_lib):
    """post.cutouts cuts a list longer than a call takes (here: than `batch`) into calls of whole candidates: the same planes"""
    cs, want = cc.case("c128_b16_nf16_nt32_ndm13_batch5")
    for batch, calls in ((0, 1), (2, 3), (5, 1)):
        info = {}
        got = post.cutouts(cs["rows"], cs["hdr"], cs["cands"], nt=32, nf=16, ndm=13, lib=emu_lib, info=info, batch=batch)
        assert info["calls"] == calls and info["kernel_used"] == 0 and cc.same_planes(got, want), batch


def test_records_that_carry_their_dm(emu_lib):
    """records with dm, sample and width (and a dm_index that no list explains) get cutout_cands' defaults from their own dm"""
    cs, _want = cc.case("c64_b8_nf16_nt16_ndm8")
    r = np.zeros(2, dtype=[("dm_index", "<u4"), ("dm", "<f8"), ("sample", "<u8"), ("width", "<u4")])
    r["dm_index"], r["dm"], r["sample"], r["width"] = [7, 3], [56.7, 20.0], [3000, 2000], [6, 1]
    made = post.cutout_cands(r, None)
    assert made["dm"].tolist() == [56.7, 20.0] and made["dm_hi"].tolist() == [113.4, 40.0] and made["tfactor"].tolist() == [3, 1]
    got = post.cutouts(cs["rows"], cs["hdr"], r, nt=16, nf=16, ndm=8, lib=emu_lib)
    want = co.planes_batch(cs["rows"][:, 0, :], cs["hdr"], made, 16, 16, 8)
    assert cc.same_planes(got, want)
    with pytest.raises(post.InputError):
        post.cutout_cands(recs((4, 6, 3000, 9.0)), None)


# ---- known answer -----------------------------------------------------------------------------------------------------
def burst_planes_hold(ft, fth, dt, dth, nt=32):
    """the planes of the burst's group, nt = 32, nf = 16, ndm = 16, DMs 0 .. 2 DM0, time bins of 2 rows"""
    ftm, dtm = post._plane_mean(ft, fth), post._plane_mean(dt, dth)
    assert all(int(np.argmax(ftm[b])) in (15, 16) for b in range(16))
    k, j = np.unravel_index(int(np.argmax(dtm)), dtm.shape)
    assert k in (7, 8) and abs(int(j) - nt // 2) <= 2
    assert np.all(fth[:, 2:-2] == 8) and np.all(dth[:, 2:-2] == 128)


def test_known_answer_on_the_burst(emu_lib, burst):
    x, records = burst
    best = post.group_candidates(records, HDR, BURST_DMS, dm_gap=2, lib=emu_lib)["best"]
    cands = post.cutout_cands(best, BURST_DMS)
    assert cands.size == 1 and int(cands[0]["tfactor"]) == 2 and cands[0]["dm"] == DM0 and cands[0]["dm_hi"] == 2 * DM0
    ft, fth, dt, dth = post.cutouts(x, HDR, cands, nt=32, nf=16, ndm=16, lib=emu_lib)
    burst_planes_hold(ft[0], fth[0], dt[0], dth[0])
    assert cc.same_planes((ft, fth, dt, dth), co.planes_batch(x, HDR, cands, 32, 16, 16))


# ---- arguments --------------------------------------------------------------------------------------------------------
def refused(lib, hdr=None, nt=16, nf=16, ndm=8, cands=None, size_off=0, nrows=6000):
    hdr = hdr or dict(HDR)
    cands = cc.cands_of((56.7, 3000, 1)) if cands is None else cands
    par = cc.params(nt, nf, ndm)
    par.size += size_off
    return lib.frbch_cutout_kernel(C.byref(post.fil_desc(hdr)), C.c_void_p(4096), nrows, C.byref(par), cands.ctypes.data, cands.size)


def test_cutout_bad_arguments(emu_lib):
    assert refused(emu_lib) == 0                                                     # (the emulator build: generic)
    assert refused(emu_lib, size_off=4) == _lib.E_ARG
    for nt in (0, 1, 3, 15, 1026, 2048):
        assert refused(emu_lib, nt=nt) == _lib.E_ARG, nt
    assert refused(emu_lib, nt=1024, ndm=1) == 0
    for nf in (0, 3, 48, 128):
        assert refused(emu_lib, nf=nf) == _lib.E_ARG, nf
    for ndm in (0, 1025):
        assert refused(emu_lib, ndm=ndm) == _lib.E_ARG, ndm
    assert refused(emu_lib, ndm=1024, nt=2) == 0
    for f in (0, 513):
        assert refused(emu_lib, cands=cc.cands_of((56.7, 3000, f))) == _lib.E_ARG, f
    for dm, lo, hi in ((-1.0, 0.0, 10.0), (1.0e5, 0.0, 10.0), (5.0, -1.0, 10.0), (5.0, 0.0, 1.0e5), (5.0, 6.0, 5.0), (float("nan"), 0.0, 1.0),
                       (5.0, 0.0, float("nan"))):
        assert refused(emu_lib, cands=cc.cands_of((dm, 3000, 1, lo, hi))) == _lib.E_ARG, (dm, lo, hi)
    assert refused(emu_lib, cands=cc.cands_of((5.0, 3000, 1, 5.0, 5.0))) == 0        # dm_hi = dm_lo is allowed
    assert refused(emu_lib, cands=cc.cands_of((56.7, 3000, 1))[:0]) == _lib.E_ARG
    many = np.repeat(cc.cands_of((56.7, 3000, 1)), 65536)
    assert refused(emu_lib, cands=many, nt=2, nf=1, ndm=1) == _lib.E_ARG
    assert refused(emu_lib, cands=many[:65535], nt=1024, nf=1, ndm=33) == _lib.E_ARG   # 65535 * 33 * 1024 >= 2^31 pixels
    assert refused(emu_lib, cands=many[:65535], nt=1024, nf=64, ndm=1) == _lib.E_ARG   # ... in the other plane
    assert refused(emu_lib, nrows=0) == _lib.E_ARG
    assert refused(emu_lib, cands=many[:1024], nt=2, nf=1, ndm=1024) == 0            # 1024 * 1024 * 64 = 2^26 delays: the most a call takes
    assert refused(emu_lib, cands=many[:1025], nt=2, nf=1, ndm=1024) == _lib.E_ARG
    rc, _out, _used, msg = cc.cutout_host(emu_lib, dict(cc.case("c64_b8_nf16_nt16_ndm8")[0], cands=many[:1025], nt=2, nf=1, ndm=1024))
    assert rc == _lib.E_ARG and "2^26" in msg
    # the calls themselves refuse the same, with a message
    cs, _want = cc.case("c64_b8_nf16_nt16_ndm8")
    bad = dict(cs, nt=15)
    rc, _out, _used, msg = cc.cutout_host(emu_lib, bad)
    assert rc == _lib.E_ARG and "nt" in msg
    bad = dict(cs, cands=cc.cands_of((56.7, 3000, 1, 60.0, 50.0)))
    rc, _out, _used, msg = cc.cutout_host(emu_lib, bad)
    assert rc == _lib.E_ARG and "dm_hi" in msg


# ---- candidates_fil ---------------------------------------------------------------------------------------------------
NAME_FIELDS = re.compile(r"_cand_tstart_([0-9.]+)_tcand_([0-9.]+)_dm_([0-9.]+)_snr_([0-9.]+)\.png$")


def parse_name(img):
    """The image name must carry, in this order, the four fields that the reference's image-name parser
    (utils/parse_fetch_image_name.py) looks for: tstart, tcand, dm and snr, each closed by "_" or, for the last, ".png".
    That parser keeps one decimal of dm and snr; so does this."""
    m = NAME_FIELDS.search(os.path.basename(img))
    assert m is not None, img
    tstart, tcand, dm, snr = (float(g) for g in m.groups())
    return tstart, tcand, round(dm, 1), round(snr, 1)


def candidates_round_trip(lib, tmp_path, want_kernel):
    """post.candidates_fil on the burst file: one candidate, its files, its name, its planes; search_fil's files unchanged"""
    x = dispersed_burst_rows(9000, HDR, DM0, 3000, 5, 30)
    os.makedirs(str(tmp_path / "a"))
    os.makedirs(str(tmp_path / "b"))
    fil_a, fil_b = str(tmp_path / "a" / "burst.fil"), str(tmp_path / "b" / "burst.fil")
    write_fil(fil_a, x[:, None, :], HDR, 1)
    write_fil(fil_b, x[:, None, :], HDR, 1)
    sp_files, records = post.search_fil(fil_a, DM0 - 20.0, dm2=DM0 + 20.0, dmstep=5.0, threshold=6.0, lib=lib)
    info = {}
    files, groups = post.candidates_fil(fil_b, DM0 - 20.0, dm2=DM0 + 20.0, dmstep=5.0, threshold=6.0, nt=32, nf=16, ndm=16, lib=lib,
                                        info=info)
    assert info["cutout_kernel_used"] == want_kernel and info["ngroup"] == 1
    assert groups.size == 1 and int(groups[0]["nmember"]) == records.size == 9
    made = sorted(os.listdir(str(tmp_path / "b")))
    assert len([m for m in made if m.endswith(".npz")]) == 1 and len([m for m in made if m.endswith(".png")]) == 1
    assert len(files) == 1 and os.path.basename(files[0]) in made and "burst.cands.txt" in made
    for path in sp_files:                                                            # search_fil's own outputs: byte for byte
        assert open(path, "rb").read() == open(os.path.join(str(tmp_path / "b"), os.path.basename(path)), "rb").read()
    assert sorted(os.path.basename(p) for p in sp_files) == [m for m in made if m.endswith(".singlepulse")]
    png = files[0].replace(".npz", ".png")
    assert open(png, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    best = groups[0]["best"]
    tstart, tcand, dm, snr = parse_name(png)
    assert tstart == HDR["tstart"] and abs(tcand - int(best["sample"]) * HDR["tsamp"]) < 1e-7
    assert dm == round(DM0, 1) and snr == round(float(best["sigma"]), 1)
    z = np.load(files[0])
    assert z["data_freq_time"].shape == (32, 16) and z["data_dm_time"].shape == (16, 32) and z["data_freq_time"].dtype == np.float32
    burst_planes_hold(z["ft"], z["ft_hits"], z["dt"], z["dt_hits"])
    assert np.array_equal(z["data_freq_time"], post._plane_mean(z["ft"], z["ft_hits"]).T)
    assert np.array_equal(z["data_dm_time"], post._plane_mean(z["dt"], z["dt_hits"]))
    for key, val in (("dm", DM0), ("width", 4), ("tfactor", 2), ("tsamp", HDR["tsamp"]), ("fch1", HDR["fch1"]), ("foff", HDR["foff"]),
                     ("nchans", 64), ("tstart", HDR["tstart"]), ("dm_lo", 0.0), ("dm_hi", 2 * DM0), ("snr", float(best["sigma"])),
                     ("tcand", int(best["sample"]) * HDR["tsamp"])):
        assert z[key] == val, key
    lines = open(os.path.join(str(tmp_path / "b"), "burst.cands.txt")).read().splitlines()
    assert lines[0] == post.CANDS_HEADER and len(lines) == 2
    assert lines[1].split() == ["%.2f" % DM0, "%.2f" % best["sigma"], "%.6f" % (int(best["sample"]) * HDR["tsamp"]), str(int(best["sample"])),
                                "4", "9", "0", "8"]
    want = co.planes_batch(x, HDR, post.cutout_cands(groups["best"], BURST_DMS), 32, 16, 16)
    assert cc.same_planes((z["ft"][None], z["ft_hits"][None], z["dt"][None], z["dt_hits"][None]), want)


def test_candidates_fil_round_trip(emu_lib, tmp_path):
    candidates_round_trip(emu_lib, tmp_path, cc.GENERIC)


def test_min_members_and_max_cands(emu_lib, tmp_path):
    x = dispersed_burst_rows(9000, HDR, DM0, 3000, 5, 30)
    fil = str(tmp_path / "burst.fil")
    write_fil(fil, x[:, None, :], HDR, 1)
    files, groups = post.candidates_fil(fil, DM0 - 20.0, dm2=DM0 + 20.0, dmstep=5.0, threshold=6.0, min_members=10, nt=32, nf=16, ndm=16,
                                        lib=emu_lib)
    assert files == [] and groups.size == 0 and open(fil.replace(".fil", ".cands.txt")).read().splitlines() == [post.CANDS_HEADER]
    files, groups = post.candidates_fil(fil, DM0 - 20.0, dm2=DM0 + 20.0, dmstep=5.0, threshold=6.0, dm_gap=1, max_cands=1, nt=2, nf=1, ndm=1,
                                        lib=emu_lib)
    assert len(files) == 1 and groups.size == 1


def test_cli_runs(monkeypatch, tmp_path, capsys):
    x = dispersed_burst_rows(9000, HDR, DM0, 3000, 5, 30)
    fil = str(tmp_path / "a.fil")
    write_fil(fil, x[:, None, :], HDR, 1)
    emu = _lib.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libfrbch_emu.so"))
    monkeypatch.setattr(_lib, "load", lambda path=None: emu)
    assert post.main(["candidates", fil, "--dm", str(DM0 - 20.0), "--dm2", str(DM0 + 20.0), "--dmstep", "5", "--threshold", "6", "--dm-gap", "1",
                      "--min-members", "2", "--max-cands", "3", "--nt", "32", "--nf", "16", "--ndm", "16"]) == 0
    out = capsys.readouterr().out
    assert "a.cands.txt" in out and out.count(".npz") == 1 and "1 candidates above 6.0 sigma" in out
