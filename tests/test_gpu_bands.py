"""GPU tests of the band-limited single-pulse search: frbch_post_dedisp_bands_tiled<BPV, FLAGS, ZERODM> + frbch_post_bands_ranges
and the generic frbch_post_dedisp_bands against tests/bands_oracle.py byte for byte on the cases of tests/bands_cases.py (every
integer case at a 16-byte aligned address -- the form it was written for -- and 4 bytes further on -- the generic form), band
[0, nsub) against frbch_dedisperse_device on the same arguments, the composite across batch sizes and against
frbch_dedisperse_search_host, and the known answer: a burst in a quarter of the band that the full-band search misses in all
twelve files and the band search finds in all twelve, with the right band.  Every device buffer is a tests/hipmem.py
GuardedBuffer of exactly the documented size."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from oracle import post_oracle as po
from tests import bands_cases as bc
from tests import bands_oracle as bo
from tests import post_cases as pc
from tests.hipmem import GUARD, GuardedBuffer
from tests.test_fold_predictor import write_fil

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_device_equals_the_oracle(hip_lib, name):
    """the form the case was written for: the tiled prefix kernel wherever the plan rule allows it"""
    bc.check_case(hip_lib, name)


@pytest.mark.parametrize("name", sorted(n for n in bc.CASES if not n.startswith("f32")))
def test_rows_four_bytes_off_take_the_generic_form_and_give_the_same_bytes(hip_lib, name):
    bc.check_case(hip_lib, name, shift=4, form=bc.GENERIC)


def test_the_host_twin(hip_lib):
    c = bc.case("u16_nifs4_product2")
    info = {}
    got, nclip = post.dedisperse_bands(c["rows"], dict(c["hdr"], nifs=4, nbits=16), c["dms"], c["nsub"], zerodm=c["zerodm"], clip=c["clip"],
                                       product=2, lib=hip_lib, info=info)
    assert info["kernel_used"] == bc.TILED and nclip == c["nclip"] > 0
    assert got.tobytes() == c["want"].tobytes()


# ---- a plane that passes 2^32 bytes -------------------------------------------------------------------------------------------
BIG_NCHAN, BIG_NDM, BIG_NSUB, BIG_NOUT = 512, 64, 8, 466100       # 64 x 36 series of 466 100 floats: 4 295 577 600 bytes


@pytest.mark.parametrize("shift", [0, 4])
def test_a_plane_beyond_4_gib(hip_lib, shift):
    """series 2303 -- the last: DM 63, band [7, 8) -- straddles byte 2^32 of the plane at t = 313 524.  Compared `==` with sums
    formed here from the rows: the first series at its start, the straddling one on both sides of the mark and at its end, the
    full band of the last DM at its end; both forms.  (zero-DM on, no clip: the clip would need the oracle on all rows.)"""
    hdr = pc.make_hdr(BIG_NCHAN)
    dms = [20.0 + 0.25 * i for i in range(BIG_NDM)]
    dly = np.stack([po.delays_samples(hdr["fch1"], hdr["foff"], BIG_NCHAN, hdr["tsamp"], dm) for dm in dms])
    nrows = BIG_NOUT + int(dly.max())
    base = np.random.default_rng(77).integers(60, 200, size=(3001, BIG_NCHAN), dtype=np.uint8)
    x = np.resize(base, (nrows, BIG_NCHAN))                        # the base again and again, row-aligned
    S = x.sum(axis=1, dtype=np.int64)
    bands = bo.band_list(BIG_NSUB)
    nband, cps = len(bands), BIG_NCHAN // BIG_NSUB
    assert BIG_NDM * nband * BIG_NOUT * 4 > 1 << 32
    mark = (1 << 30) - (BIG_NDM * nband - 1) * BIG_NOUT              # the float at byte 2^32, as a sample of the last series
    assert 0 < mark < BIG_NOUT
    raw = np.concatenate([np.zeros(shift, np.uint8), x.reshape(-1), np.zeros(16 - shift, np.uint8)])
    buf = GuardedBuffer.from_numpy(raw)
    d_out = GuardedBuffer(BIG_NDM * nband * BIG_NOUT * 4)
    desc = post.fil_desc(hdr)
    dm_arr, bp = np.ascontiguousarray(dms), post.band_params(BIG_NSUB)
    used = C.c_uint32(9)
    err = C.create_string_buffer(512)
    rc = hip_lib.frbch_dedisperse_bands_device(C.byref(desc), C.c_void_p(buf.ptr.value + shift), nrows, dm_arr.ctypes.data, BIG_NDM, 1, 0.0,
                                               C.byref(bp), 0, d_out.ptr, BIG_NOUT, None, C.byref(used), err, len(err))
    assert rc == 0, err.value
    assert used.value == (bc.TILED if shift == 0 else bc.GENERIC)
    for i, j, t0, n in ((0, 0, 0, 600), (BIG_NDM - 1, nband - 1, mark - 300, 600), (BIG_NDM - 1, nband - 1, BIG_NOUT - 300, 300),
                        (BIG_NDM - 1, bands.index((0, BIG_NSUB)), BIG_NOUT - 300, 300), (31, bands.index((2, 5)), 200000, 300)):
        a, b = bands[j]
        t = np.arange(t0, t0 + n)
        s = sum(x[t + dly[i, c], c].astype(np.int64) for c in range(a * cps, b * cps))
        z = sum(S[t + dly[i, c]] for c in range(a * cps, b * cps))
        want = (s.astype(np.float64) - z.astype(np.float64) / BIG_NCHAN).astype(np.float32)
        got = d_out._peek(GUARD + ((i * nband + j) * BIG_NOUT + t0) * 4, n * 4).view(np.float32)
        assert np.array_equal(got, want), (i, j, t0)
    d_out.check()
    buf.free()
    d_out.free()


# ---- the composite --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def search_want():
    c = bc.case("u8_7dm_search")
    want = bo.search(c["want"], c["bands"], bc.SEARCH_WIDTHS, bc.SEARCH_THR, bc.SEARCH_L)
    want.setflags(write=False)
    return c, want


def one_dm_bytes(c):
    return len(c["bands"]) * c["nout"] * 4


def test_bandsearch_equals_the_oracle_whatever_the_batch(hip_lib, search_want):
    """1 DM, 3 DMs (7 DMs: a ragged last batch) and all of them per batch"""
    c, want = search_want
    for plane_bytes, nbatch in ((one_dm_bytes(c), 7), (3 * one_dm_bytes(c), 3), (7 * one_dm_bytes(c), 1)):
        rc, got, msg, nb, used = bc.bandsearch_host(hip_lib, c, bc.SEARCH_WIDTHS, bc.SEARCH_THR, bc.SEARCH_L, plane_bytes)
        assert rc == 0, msg
        assert nb == nbatch and used == (bc.TILED, 1)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def test_bandsearch_full_band_records_are_dedisperse_search_hosts(hip_lib, search_want):
    c, _want = search_want
    rc, got, msg, _nb, _used = bc.bandsearch_host(hip_lib, c, bc.SEARCH_WIDTHS, bc.SEARCH_THR, bc.SEARCH_L, 2 * one_dm_bytes(c))
    assert rc == 0, msg
    full = bo.full_band(got, c["nsub"])
    ref = bc.dedisperse_search_host(hip_lib, c, bc.SEARCH_WIDTHS, bc.SEARCH_THR, bc.SEARCH_L)
    assert full.size > 0 and full.tobytes() == ref.tobytes()


def test_bandsearch_refuses_a_plane_below_one_dm(hip_lib, search_want):
    c, _want = search_want
    rc, _got, msg, _nb, _used = bc.bandsearch_host(hip_lib, c, bc.SEARCH_WIDTHS, bc.SEARCH_THR, bc.SEARCH_L, one_dm_bytes(c) - 1)
    assert rc == _lib.E_ARG and "holds no DM" in msg


# ---- the known answer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", bc.KA_SEEDS)
def test_a_burst_in_a_quarter_of_the_band(hip_lib, seed):
    """threshold 7: the full-band records hold nothing within 8 rows of the burst; the strongest group of the band search has
    `best` band [2, 4), a centre within 2 rows of 3002 and width 4 -- in every seed"""
    x = bc.known_answer_rows(seed)
    recs = post.band_search(x, bc.KA_HDR, [bc.KA_DM], bc.KA_NSUB, zerodm=False, clip=0.0, widths=bc.KA_WIDTHS, threshold=bc.KA_THR,
                            detrend_len=1000, lib=hip_lib)
    groups = post.group_band_candidates(recs, bc.KA_HDR, [bc.KA_DM], bc.KA_NSUB, lib=hip_lib)
    full = bo.full_band(recs, bc.KA_NSUB)
    today = post.single_pulse_search(post.dedisperse_bands(x, bc.KA_HDR, [bc.KA_DM], 1, zerodm=False, clip=0.0, lib=hip_lib)[0][0],
                                     widths=bc.KA_WIDTHS, threshold=bc.KA_THR, detrend_len=1000, lib=hip_lib)
    assert full.tobytes() == today.tobytes()                       # the full band of the band search IS today's search
    print("seed %d: %d records, best %s" % (seed, recs.size, groups[np.argmax(groups["best"]["sigma"])]["best"] if groups.size else None))
    assert bc.known_answer_holds(full, groups)


def test_the_command(hip_lib, tmp_path, capsys):
    """`post bandsearch` on the file of seed 2: the strongest line is the burst, printed as the burst commands take it"""
    path = str(tmp_path / "r3.fil")
    write_fil(path, bc.known_answer_rows(2).reshape(-1, 1, 64), bc.KA_HDR, 1)
    assert post.main(["bandsearch", path, "--dm", str(bc.KA_DM), "--nsub", "8", "--threshold", "7", "--nozerodm", "--clip", "0",
                      "--max-width", "0.002"]) == 0
    lines = open(str(tmp_path / "r3_bands.txt")).read().splitlines()
    f = lines[1].split()
    assert lines[0] == post.BANDS_HEADER and float(f[0]) == bc.KA_DM and abs(int(f[3]) - 3002) <= 2 and f[8] == "2-4"
    cps, foff = 8, bc.KA_HDR["foff"]
    assert float(f[7]) == round(1500.0 + (2 * cps - 0.5) * foff, 4) and float(f[6]) == round(1500.0 + (4 * cps - 0.5) * foff, 4)
    z = np.load(str(tmp_path / "r3_bands.npz"))
    assert z["bands"].shape == (36, 2) and z["groups"].size == len(lines) - 1 and z["dms"].tolist() == [bc.KA_DM]
