"""Single-pulse search of the dedispersed series (frbch_spsearch_*, frbch_dedisperse_search_host, post.single_pulse_search /
search_fil): known answers of the numpy restatement tests/spsearch_oracle.py, the generic kernels through the TEST-ONLY
emulator build against it record for record (every comparison exact: the search is integer arithmetic behind a fixed-order
normalisation), capacity and argument errors, and the host-side file handling."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from oracle import post_oracle as po
from tests import spsearch_cases as sc
from tests import spsearch_oracle as so
from tests.test_fold_predictor import write_fil
from tests.test_post import DM0, HDR


# ---- the oracle's known answers ------------------------------------------------------------------------------------
def test_oracle_finds_the_four_injected_pulses():
    _y, _w, _thr, _L, want, _raw = sc.case("four_pulses")
    assert [(int(c["sample"]), int(c["width"])) for c in want] == [(4321, 1), (9000, 3), (12503, 6), (19990, 20)]
    assert want["sigma"].min() > 7.0 and np.all(want["dm_index"] == 0)


def test_oracle_finds_nothing_in_noise():
    assert so.search(sc.noise(1, 20000, 16), sc.DEFAULT, 5.0, 1000).size == 0


def dispersed_burst_rows(nrows, hdr, dm, t0, width, amp, seed=31):
    rng = np.random.default_rng(seed)
    x = rng.integers(96, 160, size=(nrows, hdr["nchans"])).astype(np.int64)
    dly = po.delays_samples(hdr["fch1"], hdr["foff"], hdr["nchans"], hdr["tsamp"], dm)
    for c in range(hdr["nchans"]):
        x[t0 + dly[c]: t0 + dly[c] + width, c] += amp
    return x.astype(np.uint8)


def test_oracle_puts_a_dispersed_burst_at_its_dm():
    x = dispersed_burst_rows(9000, HDR, DM0, 3000, 6, 30)
    dms = [DM0 - 20.0, DM0, DM0 + 20.0]
    y, _ = po.dedisperse(x, fch1=HDR["fch1"], foff=HDR["foff"], tsamp=HDR["tsamp"], dms=dms, zerodm=False, clip=0)
    got = so.search(y, sc.DEFAULT, 6.0, 1000)
    top = got[np.argmax(got["sigma"])]
    assert (int(top["dm_index"]), int(top["sample"]), int(top["width"])) == (1, 3003, 6)


def test_the_cases_hold_what_they_are_written_for():
    """the properties the grid is there for, read from the oracle's intermediate results"""
    y, widths, thr, L, want, raws = sc.case("ties")
    q, dead = so.quantise(y, L)
    assert not dead.any() and set(np.unique(q)) == {-1024, 1024, 10240}                       # exact background
    # width 1 has no window (h = 0): both samples are raw peaks; S_4 = 20480 at 1998, 1999 and 2000: the first of the plateau
    assert raws[0] == [(2000, 1, 10240), (2001, 1, 10240), (1998, 4, 20480)]
    assert so.sigma_of(10240, 1) == so.sigma_of(20480, 4) == 10.0                             # one pulse, two widths, equal sigma
    assert [(int(c["sample"]), int(c["width"])) for c in want if c["dm_index"] == 0] == [(2000, 1), (2001, 1)]   # the narrower survive
    assert [r for r in raws[1] if r[1] == 4] == [(3000, 4, 40960)] and len(raws[1]) == 5
    y, widths, thr, L, want, raws = sc.case("blocks_default")
    q, dead = so.quantise(y, L)
    assert dead[0].tolist() == [False, False, False, True, False] and dead[1, 4] and not dead[2].any()
    assert not np.any(q[0, 3000:4000]) and not np.any(q[1, 4000:])
    found = {(int(c["dm_index"]), int(c["sample"]), int(c["width"])) for c in want}
    assert {(0, 1000, 3), (0, 2, 4), (1, 2503, 6), (2, 4990, 20), (2, 1997, 14)} <= found     # block edge, t = 0, end at nout
    assert not any(d == 0 and 3000 <= s < 4000 for d, s, _w in found)
    y, widths, thr, L, want, raws = sc.case("small_L64_w1")
    assert {0, 400, 776} <= {int(c["sample"]) for c in want}
    y, widths, thr, L, want, raws = sc.case("one_block_skipped_width")
    assert len(so.block_edges(y.shape[1], L)) == 1 and max(widths) > y.shape[1] and 300 in want["width"]
    assert sc.case("nothing")[4].size == 0
    y, widths, thr, L, want, raws = sc.case("wide_9dm")
    assert {300, 1024, 7} <= set(want["width"].tolist()) and set(want["dm_index"].tolist()) == set(range(9))
    assert any(c["dm_index"] == 8 and abs(int(c["sample"]) - (20011 - 150)) <= 20 and c["width"] == 300 for c in want)   # ends at nout


# ---- the emulator against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.CASES) + sorted(sc.TILE_CASES))
def test_emulator_equals_the_oracle(emu_lib, name):
    y, widths, thr, L, want, _raws = sc.case(name)
    rc, got, ncand, used, msg = sc.spsearch_host(emu_lib, y, widths, thr, L)
    assert rc == 0, msg
    assert used == 0 and ncand == want.size
    assert sc.same_records(got, want)


def test_python_entry_point(emu_lib):
    y, widths, thr, L, want, _raws = sc.case("blocks_default")
    info = {}
    got = post.single_pulse_search(y, threshold=thr, detrend_len=L, tsamp=64e-6, lib=emu_lib, info=info, cap=2)   # grows past cap
    assert info["kernel_used"] == 0 and sc.same_records(got, want) and want.size > 2
    one = post.single_pulse_search(y[2], widths=widths, threshold=thr, detrend_len=L, lib=emu_lib)
    w2 = want[want["dm_index"] == 2].copy()
    w2["dm_index"] = 0
    assert sc.same_records(one, w2)


def test_default_widths():
    assert post.default_widths(64e-6) == [1, 2, 3, 4, 6, 9, 14, 20, 30]
    assert post.default_widths(64e-6, 0.01) == [1, 2, 3, 4, 6, 9, 14, 20, 30, 45, 70, 100, 150]
    assert post.default_widths(1e-3, 1.0)[-1] == 300 and len(post.default_widths(1e-3, 1.0)) == 15
    assert post.default_widths(1.0, 0.5) == [1]


# ---- capacity and arguments ----------------------------------------------------------------------------------------
def test_capacity(emu_lib):
    y, widths, thr, L, want, _raws = sc.case("wide_9dm")
    assert want.size > 5
    rc, got, ncand, _used, msg = sc.spsearch_host(emu_lib, y, widths, thr, L, cap=5)
    assert rc == _lib.E_CAPACITY and ncand == want.size and "candidates" in msg
    assert sc.same_records(got, want[:5])
    rc, got, ncand, _used, msg = sc.spsearch_host(emu_lib, y, widths, thr, L, cap=want.size)
    assert rc == 0 and sc.same_records(got, want)


def test_raw_peak_list_overflow_is_an_error(emu_lib):
    """threshold 1e-3 on 9 x 300 000 noise samples at width 1: over 2^20 raw peaks (every local maximum above the mean)"""
    y = sc.noise(9, 300000, 17)
    rc, _got, _n, _used, msg = sc.spsearch_host(emu_lib, y, [1, 2], 1e-3, 1000)
    assert rc == _lib.E_CAPACITY and "threshold too low" in msg


@pytest.mark.parametrize("widths,thr,L", [([], 5.0, 1000), (list(range(1, 18)), 5.0, 1000), ([0, 1], 5.0, 1000), ([1, 1025], 5.0, 1000),
                                          ([2, 2], 5.0, 1000), ([3, 2], 5.0, 1000), ([1], 0.0, 1000), ([1], -1.0, 1000),
                                          ([1], float("nan"), 1000), ([1], 5.0, 63), ([1], 5.0, 65537)])
def test_bad_arguments(emu_lib, widths, thr, L):
    y = sc.noise(1, 777, 18)
    p = _lib.FrbchSpParams()
    p.size = C.sizeof(_lib.FrbchSpParams)
    p.nwidth = len(widths)
    for k, w in enumerate(widths[:16]):
        p.widths[k] = w
    p.detrend_len, p.threshold = L, thr
    cands = np.zeros(8, dtype=post.SP_CAND)
    n = C.c_uint64(0)
    err = C.create_string_buffer(256)
    assert emu_lib.frbch_spsearch_host(y.ctypes.data, 1, 777, C.byref(p), 0, cands.ctypes.data, 8, C.byref(n), None, err, len(err)) == _lib.E_ARG
    assert err.value


def test_wrong_struct_size(emu_lib):
    y = sc.noise(1, 777, 18)
    p = post.sp_params([1], 5.0, 1000)
    p.size -= 8
    n = C.c_uint64(0)
    err = C.create_string_buffer(256)
    assert emu_lib.frbch_spsearch_host(y.ctypes.data, 1, 777, C.byref(p), 0, None, 0, C.byref(n), None, err, len(err)) == _lib.E_ARG
    assert b"size" in err.value
    with pytest.raises(post.InputError):
        post.single_pulse_search(y, widths=[4, 2], lib=emu_lib)


# ---- search_fil ----------------------------------------------------------------------------------------------------
def test_search_fil_round_trip(emu_lib, tmp_path):
    x = dispersed_burst_rows(9000, HDR, DM0, 3000, 6, 30)
    fil = str(tmp_path / "pr001a_ef_no0001_IFall.fil")
    write_fil(fil, x[:, None, :], HDR, 1)
    info = {}
    files, cands = post.search_fil(fil, DM0 - 1.0, dm2=DM0 + 1.0, dmstep=1.0, threshold=6.0, write_dat=True, lib=emu_lib, info=info)
    dms = post.dm_list(DM0 - 1.0, DM0 + 1.0, 1.0)
    base = fil.replace(".fil", "")
    assert files == ["%s_DM%.2f.singlepulse" % (base, dm) for dm in dms] and len(dms) == 3 and info["kernel_used"] == 0
    # the library's answer is the two-step answer
    want_y, wclip = po.dedisperse(x, fch1=HDR["fch1"], foff=HDR["foff"], tsamp=HDR["tsamp"], dms=dms, zerodm=True, clip=5.0)
    want = so.search(want_y, post.default_widths(HDR["tsamp"]), 6.0, 1000)
    assert sc.same_records(cands, want) and info["nclipped"] == wclip and info["nout"] == want_y.shape[1]
    top = cands[np.argmax(cands["sigma"])]
    assert (int(top["dm_index"]), int(top["width"])) == (1, 6) and abs(int(top["sample"]) - 3003) <= 1
    # the text parses back to the records (sigma to the two decimals printed)
    for i, (path, dm) in enumerate(zip(files, dms)):
        lines = open(path).read().splitlines()
        assert lines[0] == "# DM      Sigma      Time (s)     Sample    Downfact"
        back = post.read_singlepulse(path, dm_index=i)
        mine = cands[cands["dm_index"] == i]
        assert back.size == mine.size == len(lines) - 1
        for f in ("dm_index", "width", "sample"):
            assert np.array_equal(back[f], mine[f])
        assert np.all(np.abs(back["sigma"] - mine["sigma"]) <= 0.005 + 1e-6)
        for ln, c in zip(lines[1:], mine):
            assert ln == "%7.2f %7.2f %13.6f %10d   %3d" % (dm, c["sigma"], int(c["sample"]) * HDR["tsamp"], c["sample"], c["width"])
    # write_dat: the files of prepdata_gpu, byte for byte
    kept = {p: open(p, "rb").read() for dm in dms for p in ("%s_DM%.2f.dat" % (base, dm), "%s_DM%.2f.inf" % (base, dm))}
    dats = post.prepdata_gpu(fil, DM0 - 1.0, dm2=DM0 + 1.0, dmstep=1.0, lib=emu_lib)
    assert sorted(p for p in kept if p.endswith(".dat")) == sorted(dats)
    for p, data in kept.items():
        assert open(p, "rb").read() == data, p
    # one DM: prepdata's other name, no .dat unless asked for
    one, _c = post.search_fil(fil, DM0, threshold=6.0, lib=emu_lib)
    assert one == [fil.replace(".fil", "_dm{0}.singlepulse".format(DM0))]
    assert not (tmp_path / ("pr001a_ef_no0001_IFall_dm{0}.dat".format(DM0))).exists()


def test_cli_runs(monkeypatch, tmp_path, capsys):
    x = dispersed_burst_rows(9000, HDR, DM0, 3000, 6, 30)
    fil = str(tmp_path / "a.fil")
    write_fil(fil, x[:, None, :], HDR, 1)
    emu = _lib.load(sc_emu_path())
    monkeypatch.setattr(_lib, "load", lambda path=None: emu)
    assert post.main(["search", fil, "--dm", str(DM0 - 1.0), "--dm2", str(DM0 + 1.0), "--dmstep", "1", "--threshold", "6", "--max-width",
                      "0.002", "--detrend", "500", "--nozerodm", "--clip", "0"]) == 0
    out = capsys.readouterr().out
    assert out.count("wrote") == 3 and "candidates above 6.0 sigma" in out
    back = post.read_singlepulse(str(tmp_path / ("a_DM%.2f.singlepulse" % DM0)))
    assert back.size and int(back[np.argmax(back["sigma"])]["width"]) == 6


def sc_emu_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libfrbch_emu.so")
