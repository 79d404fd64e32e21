"""Resident rows (frbch_candidates_host, frbch_rfi_cleanp_host, post.*(resident=True)) through the TEST-ONLY emulator build: every
array of the result view against the sequence of existing calls it replaces (tests/resident_cases.sequence), run through the same
library in the same test.  Every comparison is `==` or `tobytes()`: there is no tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import resident_cases as rs
from tests import rfi_cases as rc
from tests.test_fold_predictor import write_fil
from tests.test_post import DM0, HDR

ZAP = [rs.ZAP_CHANNEL]


# ---- 1. the burst case, no flagging ------------------------------------------------------------------------------------
def test_the_burst_case_equals_the_sequence(emu_lib):
    rows, hdr = rs.burst_rows()
    s = rs.settings(keep_series=True)
    want, got = rs.sequence(emu_lib, rows, hdr, s), rs.resident(emu_lib, rows, hdr, s)
    assert rs.differences(got, want) == []
    assert got["cands"].size == 9 and got["groups"].size == 1 and got["ft"].shape == (1, 16, 32) and got["dt"].shape == (1, 16, 32)
    assert got["mask"] is None and got["nblk"] == 0 and got["series"].shape == (9, got["nout"])
    assert got["kernel_used"] == [0, 0, 0, 0] and got["cutout_calls"] == 1 and got["row_uploads"] == 1          # the emulator has no fast kernel
    assert set(got["wall_ms"]) == set(got["device_ms"]) == set(_lib.CAND_STAGES) and all(t >= 0 for t in got["wall_ms"].values())
    assert got["wall_ms"]["dedisperse"] > 0 and got["wall_ms"]["flag"] == 0


# ---- 2. interference: the apply writes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [dict(nbits=8), dict(nbits=16), dict(nbits=32), dict(nifs=2, product=1), dict(foff_sign=+1)],
                         ids=["b8", "b16", "float", "nifs2_product1", "foff_positive"])
def test_interference_equals_the_sequence(emu_lib, case):
    rows, hdr = rs.burst_rows(interference=True, **case)
    s = rs.settings(rfi=rs.RFI, zap=ZAP, product=case.get("product", 0), dm_span=30.0 if "foff_sign" in case else None)
    want, got = rs.sequence(emu_lib, rows, hdr, s), rs.resident(emu_lib, rows, hdr, s)
    assert rs.differences(got, want) == []
    assert not np.array_equal(want["cleaned"], rows)                                   # the apply really wrote
    assert got["chan_flag"].nonzero()[0].tolist() == [rs.DEAD_CHANNEL, rs.ZAP_CHANNEL] and not got["blk_flag"].any()
    loud = got["mask"][:, rs.LOUD_CHANNEL]                                             # an unflagged channel: one cell set, the others clear
    assert loud.nonzero()[0].tolist() == [5] and got["mask"].sum() == 2 * got["nblk"] + 1
    assert got["groups"].size >= 1 and got["ft"] is not None and got["row_uploads"] == 1


def test_the_rows_given_are_not_written(emu_lib):
    rows, hdr = rs.burst_rows(interference=True)
    x = np.array(rows, copy=True)
    rs.resident(emu_lib, x, hdr, rs.settings(rfi=rs.RFI, zap=ZAP))
    assert x.tobytes() == rows.tobytes()


# ---- 3. the selection ------------------------------------------------------------------------------------------------------
def groups_of(*items):
    """(sigma, nmember) ... -> SP_GROUP records in group order"""
    g = np.zeros(len(items), dtype=post.SP_GROUP)
    for i, (o, (sigma, n)) in enumerate(zip(g, items)):
        o["best"]["sigma"], o["best"]["sample"], o["best"]["width"], o["nmember"] = sigma, 100 * i, 2, n
    return g


def selection_rule(groups, min_members, max_cands):
    """the rule of include/frbch.h, step 4, restated without a sort: a kept group has at most max_cands - 1 groups before it in
    the order (larger sigma; equal sigma: earlier)"""
    ok = [i for i in range(groups.size) if groups[i]["nmember"] >= min_members]
    if max_cands <= 0 or len(ok) <= max_cands:
        return ok
    sig = groups["best"]["sigma"]
    return [i for i in ok if sum(1 for j in ok if sig[j] > sig[i] or (sig[j] == sig[i] and j < i)) < max_cands]


def test_selection_on_hand_made_groups_with_a_tie_across_the_cut(emu_lib):
    """float32 sigmas of real rows do not tie (the six bursts below give six different ones), so the tie is made by hand"""
    g = groups_of((7.5, 2), (9.0, 1), (8.25, 3), (7.5, 2), (8.25, 2), (6.0, 5), (7.5, 4), (9.5, 1))
    for min_members in (1, 2, 3):
        for max_cands in range(0, 9):
            got = post.select_groups(g, min_members, max_cands, lib=emu_lib).tolist()
            assert got == selection_rule(g, min_members, max_cands), (min_members, max_cands)
            kept = g[g["nmember"] >= min_members]
            if max_cands and kept.size > max_cands:                                    # what candidates_fil does with a stable argsort
                idx = np.flatnonzero(g["nmember"] >= min_members)[np.sort(np.argsort(-kept["best"]["sigma"], kind="stable")[:max_cands])]
                assert got == idx.tolist()
    assert post.select_groups(g, 2, 3, lib=emu_lib).tolist() == [0, 2, 4]                # 8.25, 8.25, then the EARLIER of the 7.5s
    assert post.select_groups(g, 2, 4, lib=emu_lib).tolist() == [0, 2, 3, 4]
    assert post.select_groups(g[:0], 1, 3, lib=emu_lib).size == 0
    n = C.c_uint64(0)
    keep = np.zeros(2, np.uint64)
    assert emu_lib.frbch_cand_select(g.ctypes.data, g.size, 1, 0, keep.ctypes.data, 2, C.byref(n)) == _lib.E_CAPACITY and n.value == 8
    assert emu_lib.frbch_cand_select(g.ctypes.data, g.size, 0, 0, keep.ctypes.data, 2, C.byref(n)) == _lib.E_ARG


def test_selection_on_several_bursts(emu_lib):
    rows, hdr = rs.many_bursts_rows()
    base = rs.sequence(emu_lib, rows, hdr, rs.settings(nt=0))
    sig = base["groups"]["best"]["sigma"]
    assert base["groups"].size >= 6 and np.unique(sig).size == sig.size                # (no tie on real rows: see the test above)
    for max_cands in (1, 3, 5):
        s = rs.settings(min_members=2, max_cands=max_cands, nt=2, nf=1, ndm=1)
        want, got = rs.sequence(emu_lib, rows, hdr, s), rs.resident(emu_lib, rows, hdr, s)
        assert rs.differences(got, want) == [] and got["groups"].size == max_cands and got["ngroup_all"] == base["groups"].size
        assert got["groups"].tobytes() == base["groups"][selection_rule(base["groups"], 2, max_cands)].tobytes()


# ---- 4. no candidate, no planes --------------------------------------------------------------------------------------------
def test_no_candidate_and_no_planes(emu_lib):
    rows, hdr = rs.burst_rows()
    s = rs.settings(threshold=1000.0)
    want, got = rs.sequence(emu_lib, rows, hdr, s), rs.resident(emu_lib, rows, hdr, s)
    assert rs.differences(got, want) == []
    assert got["cands"].size == 0 and got["groups"].size == 0 and got["ngroup_all"] == 0 and got["cutout_calls"] == 0
    assert got["ft"] is None and got["ft_hits"] is None and got["dt"] is None and got["dt_hits"] is None
    s = rs.settings(nt=0)
    want, got = rs.sequence(emu_lib, rows, hdr, s), rs.resident(emu_lib, rows, hdr, s)
    assert rs.differences(got, want) == [] and got["cands"].size == 9 and got["groups"].size == 1 and got["cut_cands"].size == 1
    assert got["ft"] is None and got["dt"] is None and got["cutout_calls"] == 0
    s = rs.settings(min_members=10)                                                    # records, but no kept group
    got = rs.resident(emu_lib, rows, hdr, s)
    assert got["cands"].size == 9 and got["ngroup_all"] == 1 and got["groups"].size == 0 and got["ft"] is None


# ---- 5. two cut-out batches ------------------------------------------------------------------------------------------------
def test_two_cutout_batches(emu_lib):
    """64 channels, ndm = 1024: a call takes 2^26 / (1024 * 64) = 1024 candidates.  The existing path gives 1466 groups from
    1466 raw peaks (one DM, width 1, threshold 1: every sample above 1 sigma is a raw peak, a record and a group; far below the
    2^20 raw peaks the search holds), so the cut-outs go in two calls."""
    rows, hdr = rs.crowded_rows()
    s = rs.settings(dms=[10.0], threshold=1.0, widths=[1], nt=2, nf=64, ndm=1024, zerodm=False, clip=0.0)
    want = rs.sequence(emu_lib, rows, hdr, s)
    assert want["groups"].size == want["cands"].size == 1466 and 1024 < want["groups"].size < 2048 and want["cutout_calls"] == 2
    got = rs.resident(emu_lib, rows, hdr, s)
    assert rs.differences(got, want) == [] and got["cutout_calls"] == 2 and got["dt"].shape == (1466, 1024, 2)


# ---- 7. all products in one residency ----------------------------------------------------------------------------------------
CLEANP = [(2, 8, 64, 24 * 256 - 100, 256), (4, 8, 64, 2100, 256), (2, 16, 48, 1500, 256), (4, 16, 64, 1025, 256), (2, 32, 64, 1500, 7 * 64),
          (4, 32, 48, 2049, 256)]


@pytest.mark.parametrize("nifs,nbits,nchan,nrows,block_rows", CLEANP, ids=["if%d_b%d_c%d_n%d_br%d" % c for c in CLEANP])
def test_cleanp_equals_clean(emu_lib, nifs, nbits, nchan, nrows, block_rows):
    rows = rc.make_rows(nrows, nifs, nchan, nbits, seed=nifs + nbits)
    hdr = rc.hdr_of(nchan, nifs, nbits)
    assert nrows % block_rows                                                          # a short last block
    par = dict(block_rows=block_rows, t_cell=3.0)
    zap = [3]
    want_rows, want = post.clean(rows, hdr, par, zap=zap, lib=emu_lib)
    stats = np.stack([post.rfi_stats(rows, hdr, par, product=p, lib=emu_lib) for p in range(nifs)])
    info = {}
    got_rows, got = post.cleanp(rows, hdr, par, zap=zap, lib=emu_lib, info=info, want_stats=True)
    assert got_rows.dtype == want_rows.dtype and got_rows.tobytes() == want_rows.tobytes() and got_rows.tobytes() != rows.tobytes()
    assert got["stats"].dtype == stats.dtype and got["stats"].tobytes() == stats.tobytes()
    for k in ("mask", "repl", "chan_flag", "blk_flag"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    assert info["row_uploads"] == 1 and info["kernel_used"] == 0
    again, res = post.cleanp(rows, hdr, par, zap=zap, lib=emu_lib)                      # without the statistics
    assert again.tobytes() == want_rows.tobytes() and "stats" not in res


@pytest.mark.parametrize("nbits", [8, 16, 32])
def test_cleanp_of_one_product_is_rfi_clean_host(emu_lib, nbits):
    rows = rc.make_rows(1500, 1, 64, nbits, seed=3)
    par = rc.params(block_rows=256, t_cell=3.0)
    code, want_rows, want, _used, msg = rc.clean_host(emu_lib, rows, 0, par, zap=np.arange(64) == 3)
    assert code == 0, msg
    got_rows, got = post.cleanp(rows, rc.hdr_of(64, 1, nbits), par, zap=[3], lib=emu_lib)
    assert got_rows.tobytes() == want_rows.tobytes() and rc.same_result(dict(got, repl=got["repl"][0]), want)


def test_cleanp_bad_arguments(emu_lib):
    rows = rc.make_rows(300, 2, 64, 8)
    with pytest.raises(post.InputError):
        post.cleanp(rows, rc.hdr_of(64, 2, 8), dict(block_rows=0), lib=emu_lib)
    with pytest.raises(post.InputError):
        post.cleanp(rows, rc.hdr_of(64, 2, 8), dict(chan_frac=1.5), lib=emu_lib)


# ---- 8. Python and the command line ----------------------------------------------------------------------------------------
def burst_file(directory, interference=True, name="burst.fil"):
    rows, hdr = rs.burst_rows(interference=interference)
    path = os.path.join(directory, name)
    write_fil(path, rows, hdr, 1)
    return path


KW = dict(dm2=DM0 + 20.0, dmstep=5.0, threshold=6.0)


def values_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("rfi", [False, True], ids=["plain", "rfi"])
def test_candidates_fil_resident(emu_lib, tmp_path, rfi):
    infos = {}

    def run(d, resident):
        infos[resident] = {}
        files, groups = post.candidates_fil(burst_file(d, rfi), DM0 - 20.0, nt=32, nf=16, ndm=16, lib=emu_lib, info=infos[resident],
                                            rfi=dict(rs.RFI) if rfi else None, resident=resident, **KW)
        return [os.path.basename(f) for f in files], groups
    names, off, on = rs.commands_round_trip(emu_lib, tmp_path, run)
    assert off[0] == on[0] and len(on[0]) == 1 and values_equal(off[1], on[1])
    assert sum(n.endswith(".png") for n in names) == 1 and sum(n.endswith(".singlepulse") for n in names) == 9 and "burst.cands.txt" in names
    assert infos[True]["row_uploads"] == 1 and set(infos[True]["wall_ms"]) == set(_lib.CAND_STAGES)
    for k, v in infos[False].items():                                                  # everything the default path reports, the same
        w = infos[True][k]
        assert np.array_equal(v, w) if isinstance(v, np.ndarray) else v == w, k


@pytest.mark.parametrize("write_dat", [False, True], ids=["singlepulse", "write_dat"])
def test_search_fil_resident(emu_lib, tmp_path, write_dat):
    infos = {}

    def run(d, resident):
        infos[resident] = {}
        flag = os.path.join(d, "zap.flag")
        post.write_flag_file(flag, np.arange(64) == rs.ZAP_CHANNEL)
        files, cands = post.search_fil(burst_file(d), DM0 - 20.0, write_dat=write_dat, lib=emu_lib, info=infos[resident], flag_file=flag,
                                       rfi=dict(rs.RFI), resident=resident, **KW)
        return [os.path.basename(f) for f in files], cands
    names, off, on = rs.commands_round_trip(emu_lib, tmp_path, run)
    assert off[0] == on[0] and values_equal(off[1], on[1]) and on[1].size >= 9
    assert sum(n.endswith(".dat") for n in names) == (9 if write_dat else 0) == sum(n.endswith(".inf") for n in names)
    assert infos[True]["row_uploads"] == 1 and infos[True]["rfi_chan_flag"].nonzero()[0].tolist() == [rs.DEAD_CHANNEL, rs.ZAP_CHANNEL]
    for k, v in infos[False].items():
        w = infos[True][k]
        assert np.array_equal(v, w) if isinstance(v, np.ndarray) else v == w, k


def test_the_block_length_warning_is_raised_on_the_resident_path_as_well(emu_lib, tmp_path):
    rows, hdr = rs.burst_rows()
    x = np.array(rows, copy=True)
    x[1024:2048] = np.clip(x[1024:2048].astype(np.int64) + 60, 0, 255).astype(np.uint8)          # one whole block of 1024 rows, broadband
    for resident in (False, True):
        d = str(tmp_path / str(resident))
        os.makedirs(d)
        path = os.path.join(d, "b.fil")
        write_fil(path, x, hdr, 1)
        info = {}
        with pytest.warns(UserWarning, match="flagged wholly"):
            post.search_fil(path, DM0, threshold=6.0, lib=emu_lib, rfi=True, info=info, resident=resident)
        assert info["rfi_blk_flag"].any()
    rs.same_files(str(tmp_path / "False"), str(tmp_path / "True"))


@pytest.mark.parametrize("nifs", [1, 4])
def test_rfifind_fil_resident(emu_lib, tmp_path, nifs):
    rows = rc.make_rows(2100, nifs, 64, 8, seed=9)
    hdr = dict(rc.hdr_of(64, nifs, 8))
    infos = {}

    def run(d, resident):
        infos[resident] = {}
        path = os.path.join(d, "scan.fil")
        write_fil(path, rows, hdr, nifs)
        files, res = post.rfifind_fil(path, block_rows=256, t_cell=3.0, write_clean=True, lib=emu_lib, info=infos[resident], resident=resident)
        return [os.path.basename(f) for f in files], res
    names, off, on = rs.commands_round_trip(emu_lib, tmp_path, run)
    assert names == ["scan.fil", "scan.flag", "scan_clean.fil", "scan_rfi.npz"] and off[0] == on[0]
    assert sorted(off[1]) == sorted(on[1]) and all(values_equal(off[1][k], on[1][k]) for k in off[1])
    assert infos[True]["row_uploads"] == 1 and infos[True]["kernel_used"] == infos[False]["kernel_used"]
    cleaned = open(str(tmp_path / "on" / "scan_clean.fil"), "rb").read()
    want_rows, _res = post.clean(rows, hdr, dict(block_rows=256, t_cell=3.0), lib=emu_lib)
    assert cleaned.endswith(want_rows.tobytes()) and not cleaned.endswith(rows.tobytes())


def test_the_resident_flags_parse(monkeypatch, tmp_path, capsys):
    emu = _lib.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libfrbch_emu.so"))
    monkeypatch.setattr(_lib, "load", lambda path=None: emu)
    fil = burst_file(str(tmp_path))
    dm = ["--dm", str(DM0 - 20.0), "--dm2", str(DM0 + 20.0), "--dmstep", "5", "--threshold", "6"]
    assert post.main(["candidates", fil] + dm + ["--nt", "32", "--nf", "16", "--ndm", "16", "--rfi", "--resident"]) == 0
    assert post.main(["search", fil] + dm + ["--rfi", "--resident"]) == 0
    assert post.main(["rfifind", fil, "--block-rows", "256", "--write-clean", "--resident"]) == 0
    out = capsys.readouterr().out
    assert "burst.cands.txt" in out and out.count(".npz and .png") == 1 and "burst_clean.fil" in out


# ---- 9. argument errors ----------------------------------------------------------------------------------------------------
def test_argument_errors(emu_lib):
    rows, hdr = rs.burst_rows()
    s = rs.settings(rfi=rs.RFI)

    def refused(change=None, **kw):
        par = rs.cand_par(hdr, s)
        if change:
            change(par)
        code, res, msg = rs.raw_call(emu_lib, rows, hdr, rs.BURST_DMS, par, **kw)
        assert code == _lib.E_ARG and msg and not res, (code, msg, res)
        return msg
    assert rs.raw_call(emu_lib, rows, hdr, rs.BURST_DMS, rs.cand_par(hdr, s))[0] == 0                  # the unchanged arguments are taken
    for field in ("size", "rfi.size", "sp.size", "cut.size"):
        def wrong(par, field=field):
            obj = par
            for name in field.split(".")[:-1]:
                obj = getattr(obj, name)
            obj.size += 4
        assert "wrong size" in refused(wrong), field
    bad_desc = post.fil_desc(hdr)
    bad_desc.size -= 4
    assert "wrong size" in refused(desc=bad_desc)
    code, res, msg = rs.raw_call(emu_lib, rows, hdr, rs.BURST_DMS, rs.cand_par(hdr, s), out=False)
    assert code == _lib.E_ARG and "out" in msg
    code, res, msg = rs.raw_call(emu_lib, rows, hdr, rs.BURST_DMS, None)
    assert code == _lib.E_ARG and msg and not res
    assert "min_members" in refused(lambda p: setattr(p, "min_members", 0))
    for gap in (0, 17):
        assert "dm_gap" in refused(lambda p, gap=gap: setattr(p, "dm_gap", gap))
    for name, val in (("nt", 3), ("nt", 1026), ("nf", 5), ("ndm", 1025), ("ndm", 0)):
        refused(lambda p, name=name, val=val: setattr(p.cut, name, val))
    refused(lambda p: setattr(p, "flags", 4))
    refused(lambda p: setattr(p.rfi, "block_rows", 0))
    refused(lambda p: setattr(p.sp, "threshold", 0.0))
    code, res, msg = rs.raw_call(emu_lib, rows, hdr, [1.0e6], rs.cand_par(hdr, s))
    assert code == _lib.E_ARG and msg and not res
    emu_lib.frbch_cand_result_free(None)                                               # a no-op
    v = _lib.FrbchCandView()
    assert emu_lib.frbch_cand_result_view(None, C.byref(v)) == _lib.E_ARG
