"""CPU tests of the DM scan (frbch_dmscan_*) through the emulator build, which runs the generic kernel: acc, hits, the two curves
and the results byte for byte against the numpy restatement tests/dmscan_oracle.py, the _device twin into pre-filled outputs,
every refusal with its message and untouched outputs, the bound of the fixed-point scale in Python integers, the analytic
accuracy bound against a plain fp64 evaluation, a burst of known DM and one whose halves drift, `post dmfit` end to end with
`--dm-from` on `rmsynth` and `polprof`, and a walk of failing device-layer calls."""
import ctypes as C
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import dmscan_cases as dc
from tests import dmscan_oracle as do
from tests import rm_cases as rc


def scan_of(lib, c, info=None, **kw):
    a = dict(widths=c["widths"], smooth=c["smooth"], fit_frac=c["fit_frac"], flag=c["flag"], products="coherency" if c["coh"] else "stokes")
    a.update(kw)
    return post.dm_scan(c["rows"], c["hdr"], c["cands"], c["ntrial"], c["ddm"], c["nbin"], c["tfactor"], lib=lib, info=info, **a)


# ---- the library against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_scan_equals_the_oracle(emu_lib, name):
    c, want = dc.case(name), dc.want(name)
    info = {}
    got = scan_of(emu_lib, c, info)
    assert info == dict(spectra_kernel_used=0, kernel_used=0)
    assert dc.same(got, want), [f for f in dc.FIELDS if np.ascontiguousarray(got[f]).tobytes() != np.ascontiguousarray(want[f]).tobytes()]
    assert dc.query(emu_lib, c, c["rows"].ctypes.data) == 0
    dms = np.array([do.trial_dms(cd["dm"], c["ntrial"], c["ddm"]) for cd in c["cands"]])
    assert got["dm"].tobytes() == dms.tobytes()
    # the _device twin (the emulator's device memory is host memory) writes the same bytes into outputs that held something else
    code, msg, out, k = dc.call(emu_lib.frbch_dmscan_device, c, c["rows"].ctypes.data,
                                out=dc.outputs(c["cands"].size, c["ntrial"], c["nbin"], c["hdr"]["nchans"], fill=0xA5))
    assert code == 0 and k == (0, 0), msg
    for f in out:
        assert out[f].tobytes() == np.ascontiguousarray(got[f]).tobytes(), (name, f)
    # the peaks alone, from the planes
    r = want["results"]
    snr, strc = np.full_like(want["snr"], 7.0), np.full_like(want["struct"], 7.0)
    wd, bn = np.zeros(snr.shape, np.uint32), np.zeros(snr.shape, np.uint32)
    res = np.zeros(r.size, dtype=post.DMSCAN_RESULT)
    err = C.create_string_buffer(256)
    ks, nu = np.ascontiguousarray(want["k"]), np.ascontiguousarray(want["nused"])
    code = emu_lib.frbch_dmscan_peaks(C.byref(dc.par_of(c)), C.byref(dc.peak_par_of(c)), c["cands"].ctypes.data, r.size, ks.ctypes.data, nu.ctypes.data,
                                      want["acc"].ctypes.data, want["hits"].ctypes.data, snr.ctypes.data, strc.ctypes.data, wd.ctypes.data,
                                      bn.ctypes.data, res.ctypes.data, err, len(err))
    assert code == 0, err.value
    assert (snr.tobytes(), strc.tobytes(), wd.tobytes(), bn.tobytes(), res.tobytes()) == (
        want["snr"].tobytes(), want["struct"].tobytes(), want["width"].tobytes(), want["bin"].tobytes(), r.tobytes())


def test_the_cases_reach_their_edges():
    """the restatement alone: what each case is there for"""
    w = dc.want("u8_64ch_33x33x3")                                  # a dead candidate between two live ones
    assert w["nused"].tolist() == [64, 0, 64] and not w["hits"][1].any() and not w["acc"][1].any() and not w["snr"][1].any()
    assert not w["results"][1:2].view(np.uint8).any() and (w["hits"][[0, 2]] == 64 * 3).all()
    r = w["results"][0]
    assert r["k_snr"] == 16 and r["snr_peak"] > 100 and r["nfit_snr"] > 0                          # the centre trial is the burst's own DM
    w = dc.want("u8_64ch_1x1x1")
    assert w["acc"].shape == (1, 1, 1) and w["results"]["fitted_snr"][0] == 0 and w["results"]["dm_struct"][0] == rc.B1["dm"]
    assert w["struct"][0, 0] == 0.0 and w["hits"][0, 0, 0] == 64
    w = dc.want("u8_64ch_windows_leave_the_file")                   # B_EDGE: bins in front of row 0; B_END: behind the last row
    assert 0 < w["hits"][0, 8, 0] < w["hits"][0, 8, 20] < 64 and w["hits"][0, 8, 60:].min() == 64
    assert 0 < w["hits"][1, 8, 150] < w["hits"][1, 8, 0] == w["nused"][1] < 64 and not w["hits"][1, :, -10:].any()
    assert (w["hits"][0, 0] != w["hits"][0, 16]).any()              # the partial hits depend on the trial
    w = dc.want("u8_64ch_4096x2")
    assert w["acc"].shape == (1, 4096, 2) and w["results"]["k_snr"][0] in range(1948, 2148)
    c = dc.case("u8_64ch_4096x2")
    assert do.trial_dms(c["cands"][0]["dm"], 4096, c["ddm"])[0] > 0
    w = dc.want("u8_64ch_3x1024")
    assert not w["hits"][1, :, :330].any() and (w["hits"][0] == 64).all()
    w = dc.want("u8_64ch_tfactor512")
    assert (w["hits"] == 64 * 512).all()
    w = dc.want("u16_64ch_coherency")
    assert w["nused"].tolist() == [64, 64, 64]
    a, b = dc.want("u8_64ch_one_product"), dc.want("u8_64ch_product2")
    assert dc.case("u8_64ch_one_product")["rows"].shape[1] == 1 and a["nused"].tolist() == [64, 64]
    assert dc.case("u8_64ch_product2")["hdr"]["product"] == 2 and b["nused"].tolist() == [64]
    w = dc.want("u8_96ch_ascending")
    assert w["nused"].tolist() == [96, 96, 0] and dc.case("u8_96ch_ascending")["hdr"]["foff"] > 0
    w = dc.want("u8_64ch_flag_constant_dead")                       # flags 0, 17, 63; constant columns 5, 40; B_OUT in the middle
    assert not w["used"][:, [0, 17, 63, 5, 40]].any() and w["nused"].tolist() == [59, 0, 59]
    for name, tf_ok in (("u8_1024ch_spread_exceeds_the_stage", False), ("u8_1024ch_edge_fits", True), ("u8_1024ch_edge_one_more", False)):
        c = dc.case(name)
        rng = dc.tile_range(c["hdr"], 1, c["cands"], c["ntrial"], c["ddm"], 1)
        assert rng == 898 and (c["tfactor"] + rng <= 1024) == tf_ok and dc.plan_expected(c, True) == int(tf_ok), (name, rng)
        assert dc.want(name)["nused"].tolist() == [1024] and dc.want(name)["results"]["snr_peak"][0] > 50
    assert dc.case("u8_1024ch_edge_fits")["tfactor"] + 1 == dc.case("u8_1024ch_edge_one_more")["tfactor"]
    assert dc.case("u8_1024ch_edge_fits")["tfactor"] + dc.tile_range(dc.case("u8_1024ch_edge_fits")["hdr"], 1, dc.case("u8_1024ch_edge_fits")["cands"], 3, 0.05, 1) == 1024
    assert sorted(dc.MUST_RUN_FAST + dc.MUST_RUN_GENERIC) == sorted(dc.CASES)
    for name in dc.CASES:
        assert dc.plan_expected(dc.case(name), True) == int(name in dc.MUST_RUN_FAST), name
        assert dc.plan_expected(dc.case(name), False) == 0


def test_the_bound_of_the_scale():
    """4096 channels at full scale over a baseline of 1 / 2 with one sign: the largest |X| lies within a factor of 2 of 2^40, the
    sums of a bin pass 2^50, and the int64 sums of numpy equal the sums in Python integers (asserted inside the restatement)"""
    w = dc.want("u8_4096ch_full_scale")
    big_x, big_sum = w["largest"]
    print("largest |X| = 2^%.3f, largest sum = 2^%.3f" % (np.log2(big_x), np.log2(big_sum)))
    assert (1 << 39) < big_x <= (1 << 40) and (1 << 50) < big_sum < (1 << 54)
    assert int(np.abs(w["acc"]).max()) == big_sum and w["nused"][0] == 4096


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(emu_lib):
    c = dc.case("u8_64ch_33x33x3")
    hdr, ptr = c["hdr"], c["rows"].ctypes.data
    host = emu_lib.frbch_dmscan_host

    def cand(field, value, i=0):
        cc = c["cands"].copy()
        cc[field][i] = value
        return cc

    assert dc.call(host, c, ptr)[0] == 0
    par, pk = (lambda **kw: dc.par_of(c, **kw)), (lambda **kw: dc.peak_par_of(c, **kw))
    refused = [
        (dict(par=par(size=16)), "frbch_dmscan_params: wrong size"), (dict(par=par(ntrial=0)), "ntrial"), (dict(par=par(ntrial=4097)), "ntrial"),
        (dict(par=par(nbin=0)), "nbin"), (dict(par=par(nbin=1025)), "nbin"), (dict(par=par(tfactor=0)), "tfactor"),
        (dict(par=par(tfactor=513)), "tfactor"), (dict(par=par(ddm=0.0)), "ddm"), (dict(par=par(ddm=-0.1)), "ddm"),
        (dict(par=par(ddm=np.nan)), "ddm"), (dict(par=par(ddm=np.inf)), "ddm"), (dict(par=par(ddm=4.0)), "trial DM outside"),
        (dict(cands=cand("dm", 99999.0, 2)), "trial DM outside"),
        (dict(hdr=dict(hdr, nbits=32)), "not built for float32"), (dict(hdr=dict(hdr, nifs=2), bpar=rc.burst_par(True)), "nifs = 4"),
        (dict(hdr=dict(hdr, nchans=16385)), "16384"), (dict(ncand=0), "candidates"),
        (dict(cands=np.repeat(c["cands"][:1], 4097)), "candidates"), (dict(cands=np.repeat(c["cands"][:1], 32), par=par(ntrial=1024, ddm=0.001, nbin=1024)), "2^24"),
        (dict(cands=np.repeat(c["cands"][:1], 512), par=par(ntrial=4096, ddm=0.001, nbin=1)), "2^26"),
        (dict(pk=pk(size=80)), "frbch_dmscan_peak_params: wrong size"), (dict(pk=pk(nwidth=0)), "nwidth"), (dict(pk=pk(nwidth=17)), "nwidth"),
        (dict(pk=pk(widths=(0,))), "widths"), (dict(pk=pk(widths=(1, 34))), "widths"), (dict(pk=pk(widths=(2, 2))), "widths"),
        (dict(pk=pk(smooth=0)), "smooth"), (dict(pk=pk(smooth=33)), "smooth"), (dict(pk=pk(fit_frac=0.0)), "fit_frac"),
        (dict(pk=pk(fit_frac=1.0)), "fit_frac"), (dict(pk=pk(fit_frac=np.nan)), "fit_frac"),
        (dict(cands=cand("width", 0)), "width"), (dict(cands=cand("off_len", 1)), "off_len"), (dict(cands=cand("dm", -1.0)), "DM"),
        (dict(bpar=rc.burst_par(size=4)), "frbch_burst_params: wrong size"),
    ]
    for kw, text in refused:
        n = kw["cands"].size if "cands" in kw else 3
        out = dc.outputs(min(n, 3), 33, 33, 64, fill=0xA5)
        code, msg, out, _k = dc.call(host, c, ptr, out=out, **kw)
        assert code == _lib.E_ARG and text in msg, (kw, msg)
        assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), kw
        code2 = dc.call(emu_lib.frbch_dmscan_device, c, ptr, out=out, **kw)[0]
        assert code2 == _lib.E_ARG and all((a.view(np.uint8) == 0xA5).all() for a in out.values()), kw
    # the plan query refuses the same and a null pointer; ntrial = 1 does not look at ddm
    assert dc.query(emu_lib, c, ptr, par=par(nbin=1025)) == _lib.E_ARG and dc.query(emu_lib, c, None) == _lib.E_ARG
    assert dc.query(emu_lib, c, ptr, par=par(ddm=4.0)) == _lib.E_ARG and dc.query(emu_lib, c, ptr, cands=cand("dm", np.nan)) == _lib.E_ARG
    assert dc.call(host, c, ptr, par=par(ntrial=1, ddm=np.nan))[0] == 0
    assert dc.call(host, c, None)[0] == _lib.E_ARG
    with pytest.raises(post.InputError, match="float32"):
        post.dm_scan(c["rows"].astype(np.float32), dict(hdr, nbits=32), c["cands"], 3, 0.1, lib=emu_lib)
    assert post.dm_sample_step(hdr, emu_lib) == do.sample_step(hdr) and post.dm_sample_step(dict(hdr, nchans=1), emu_lib) == 0.0


# ---- accuracy: the integer plane against the plain fp64 evaluation -------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_the_integer_plane_stays_within_its_bound(name):
    """|acc 2^-k - the fp64 sum of the same x| <= N 2^-k-1 per bin: every term is rounded to a unit of 2^-k, half a unit off at the
    most (the fp64 sum's own rounding, 2^-53 of sums below 2^14 units, is below that by far).  Measured (largest error / bound
    over all cases): 0.43, in u8_64ch_windows_leave_the_file; 0.30 elsewhere -- the rounding errors of the channels do not line up."""
    w = dc.want(name)
    worst = 0.0
    for i in np.flatnonzero(w["nused"]):
        err = np.abs(w["acc"][i].astype(np.float64) * 2.0 ** -float(w["k"][i]) - w["plain"][i])
        worst = max(worst, float(err.max()) / w["units"][i])
    print("%s: largest error / bound %.4f" % (name, worst))
    assert worst <= 1.0


# ---- the known answers ------------------------------------------------------------------------------------------------
def test_the_oracle_returns_the_injected_dm():
    """before anything relies on it: the restatement alone on the fixed seed.  Over seeds 0 .. 11 of this shape the S/N estimate
    lay within -0.45 .. +0.70 DM sample steps of the injected DM and the structure estimate within +0.10 .. +0.62."""
    out, step = dc.known_oracle(dc.KNOWN_SEED)
    r = out["results"][0]
    print("S/N %+.3f steps, structure %+.3f steps, step %.5f" % ((r["dm_snr"] - dc.KNOWN_DM) / step, (r["dm_struct"] - dc.KNOWN_DM) / step, step))
    assert r["fitted_snr"] == 1 and r["fitted_struct"] == 1 and r["nused"] == 64
    assert abs(r["dm_snr"] - dc.KNOWN_DM) <= 2.0 * step and abs(r["dm_struct"] - dc.KNOWN_DM) <= 2.0 * step
    assert abs(step - 0.0631) < 5e-4 and r["dm_snr_err"] > 0


def test_known_answer(emu_lib):
    hdr, cands, grid, step = dc.known_scan_args()
    want, _ = dc.known_oracle(dc.KNOWN_SEED)
    got = post.dm_scan(dc.known_rows(dc.KNOWN_SEED), hdr, cands, widths=dc.WIDTHS, smooth=dc.SMOOTH, fit_frac=dc.FIT_FRAC, lib=emu_lib, **grid)
    assert dc.same(got, want)
    r = got["results"][0]
    assert abs(r["dm_snr"] - dc.KNOWN_DM) <= 2.0 * step and abs(r["dm_struct"] - dc.KNOWN_DM) <= 2.0 * step


def test_drifting_halves_move_the_snr_dm_and_not_the_structure_dm(emu_lib):
    """two half-band components 8 rows apart, the upper half first: over seeds 0 .. 11 the oracle's S/N estimate lay +10.8 .. +14.1
    DM sample steps from the injected DM and its structure estimate -2.9 .. -0.2, the S/N estimate further off by 8.3 steps at
    the least.  Asserted: further off, by 5 steps or more."""
    hdr, cands, grid, step = dc.known_scan_args()
    want, _ = dc.known_oracle(dc.KNOWN_SEED, dc.DRIFT_ROWS)
    got = post.dm_scan(dc.known_rows(dc.KNOWN_SEED, dc.DRIFT_ROWS), hdr, cands, widths=dc.WIDTHS, smooth=dc.SMOOTH, fit_frac=dc.FIT_FRAC,
                       lib=emu_lib, **grid)
    assert dc.same(got, want)
    r = want["results"][0]
    off_snr, off_struct = abs(r["dm_snr"] - dc.KNOWN_DM) / step, abs(r["dm_struct"] - dc.KNOWN_DM) / step
    print("S/N estimate %.3f steps off, structure estimate %.3f" % (off_snr, off_struct))
    assert r["dm_snr"] > dc.KNOWN_DM and off_snr - off_struct >= 5.0


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_dmfit_end_to_end_and_dm_from(emu_lib, tmp_path, capsys, monkeypatch):
    from tests.test_fold_predictor import write_fil
    from tests import polprof_cases as pc
    c, _injected = pc.known_case()                                   # four products, 1024 channels at 1.2 - 1.5 GHz, a burst at DM 50
    hdr, rows = c["hdr"], c["rows"]
    fil = str(tmp_path / "burst.fil")
    write_fil(fil, rows, hdr, 4)
    base = fil.replace(".fil", "")
    info = {}
    files, scan = post.dmfit_fil(fil, [(50.2, 2000, 40)], nbin=64, tfactor=2, off_len=400, fit_frac=0.9, lib=emu_lib, info=info)      # (a box of 40 rows: a flat top)
    assert files == [base + "_dm.npz", base + "_dm.txt", base + "_dm_burst0.png"] and all(os.path.getsize(f) > 0 for f in files)
    assert info["kernel_used"] == 0
    step = do.sample_step(hdr)
    back = np.load(files[0])
    assert float(back["ddm"]) == step / 4.0 and back["acc"].shape == (1, 257, 64) and back["bursts"]["off_gap"][0] == 80
    want = do.scan(rows, hdr, back["bursts"], 257, step / 4.0, 64, 2, widths=(1, 2, 4, 8, 16, 32), smooth=3, fit_frac=0.9)
    for f in dc.FIELDS:
        assert back[f].tobytes() == np.ascontiguousarray(want[f]).tobytes() == np.ascontiguousarray(scan[f]).tobytes(), f
    r = scan["results"][0]
    assert r["fitted_snr"] == 1 and abs(r["dm_snr"] - 50.0) <= 2.0 * step and abs(r["dm_struct"] - 50.0) <= 2.0 * step
    line = open(files[1]).read().splitlines()
    assert len(line) == 1 and line[0].startswith("burst0") and ("DM_snr %10.4f" % r["dm_snr"]) in line[0]
    # the command line, and --dm-from against --dm with the same value
    monkeypatch.setattr(_lib, "load", lambda path=None: emu_lib)
    for f in files:
        os.remove(f)
    assert post.main(["dmfit", fil, "--dm", "50.2", "--sample", "2000", "--width", "40", "--nbin", "64", "--tfactor", "2", "--off-len", "400", "--fit-frac", "0.9"]) == 0
    assert "wrote " + files[0] in capsys.readouterr().out and np.load(files[0])["results"].tobytes() == scan["results"].tobytes()
    gap, common = str(int(back["bursts"]["off_gap"][0])), ["--sample", "2000", "--width", "40", "--off-len", "400"]
    for kind in ("snr", "struct"):
        dm = repr(float(r["dm_" + kind]))
        outs = {}
        for how, args in (("dm", ["--dm", dm] + common + ["--off-gap", gap]), ("from", ["--dm-from", files[0], "--dm-kind", kind])):
            assert post.main(["rmsynth", fil] + args + ["--nphi", "65"]) == 0
            assert post.main(["polprof", fil] + args + ["--rm", "350", "--nbin", "64"]) == 0
            outs[how] = {f: open(base + f, "rb").read() for f in ("_rm.txt", "_rm_burst0.png", "_polprof.txt", "_polprof_burst0.png")}
            outs[how].update({f + k: v.tobytes() for f in ("_rm.npz", "_polprof.npz") for k, v in np.load(base + f).items()})
        assert outs["dm"] == outs["from"], kind
    assert np.load(base + "_polprof.npz")["bursts"]["dm"][0] == r["dm_struct"]
    capsys.readouterr()
    with pytest.raises(SystemExit):
        post.main(["rmsynth", fil, "--sample", "2000", "--width", "40"])


# ---- failing device-layer calls ---------------------------------------------------------------------------------------
def test_a_failing_device_call_returns_the_error_and_leaves_nothing_behind(emu_lib):
    """every fallible device-layer call of frbch_dmscan_host fails once (n = 1, 2, ... until the call succeeds): an error with a
    message comes back, the outputs are untouched, the blocks and streams alive afterwards are those alive before, and a plain
    call right afterwards writes the expected bytes"""
    emu_lib.frbch_test_emu_fail_at.argtypes, emu_lib.frbch_test_emu_fail_at.restype = [C.c_long], None
    emu_lib.frbch_test_emu_live.argtypes, emu_lib.frbch_test_emu_live.restype = [], C.c_uint64
    c, want = dc.case("u8_64ch_33x33x3"), dc.want("u8_64ch_33x33x3")
    ptr = c["rows"].ctypes.data
    rows0 = c["rows"].tobytes()
    codes = []
    for n in range(1, 200):
        out = dc.outputs(3, 33, 33, 64, fill=0xA5)
        before = emu_lib.frbch_test_emu_live()
        emu_lib.frbch_test_emu_fail_at(n)
        try:
            code, msg, out, _k = dc.call(emu_lib.frbch_dmscan_host, c, ptr, out=out)
        finally:
            emu_lib.frbch_test_emu_fail_at(0)
        assert emu_lib.frbch_test_emu_live() == before, n
        if code == 0:
            assert dc.same(out, want)
            break
        codes.append(code)
        assert code in (_lib.E_DEVICE, _lib.E_NOMEM) and msg, (n, code, msg)
        assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), n
        again = dc.call(emu_lib.frbch_dmscan_host, c, ptr)
        assert again[0] == 0 and dc.same(again[2], want), n
    assert 15 < len(codes) < 199 and c["rows"].tobytes() == rows0
