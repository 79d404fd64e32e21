"""CPU tests of the fold refinement (frbch_foldfit_*, frbch_fold_refine_*) through the emulator build, which runs the generic
kernels: every case of tests/foldfit_cases.py byte for byte against the numpy restatement tests/foldfit_oracle.py, the
single-trial profile against post._scrunched, the peaks alone, every refusal with its message and untouched outputs, the
composite against the two calls in sequence, the commands end to end, and the known answer in twelve noise seeds."""
import ctypes as C
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import foldfit_cases as fc
from tests import foldfit_oracle as fo


def fit_of(lib, c, info=None, **kw):
    return post.fold_fit(c["cube"], c["hits"], c["hdr"], c["nrows"], fc.par_of(c), flag=c["flag"], want_trials=c["want_trials"], lib=lib, info=info, **kw)


# ---- the library against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_generic_kernels_equal_the_oracle(emu_lib, name):
    c, want = fc.case(name), fc.want(name)
    info = {}
    got = fit_of(emu_lib, c, info)
    assert info == dict(kernel_used=(0, 0))
    assert fc.same(got, want), fc.differing(got, want)
    assert fc.query(emu_lib, c, c["cube"].ctypes.data, c["hits"].ctypes.data) == (0, 0)
    # the _device twin (the emulator's device memory is host memory) writes the same bytes into outputs that held something else
    code, msg, out, k = fc.call(emu_lib.frbch_foldfit_device, c, c["cube"].ctypes.data, c["hits"].ctypes.data, out=fc.outputs(c, fill=0xA5))
    assert code == 0 and k == (0, 0), msg
    assert fc.same(out, want), fc.differing(out, want)


def test_the_cases_reach_their_edges():
    """the restatement and the cases alone: what each case is there for"""
    assert sorted(fc.MUST_RUN_FAST_STAGE1 + fc.MUST_RUN_GENERIC_STAGE1) == sorted(fc.MUST_RUN_FAST_STAGE2 + fc.MUST_RUN_GENERIC_STAGE2) == sorted(fc.CASES)
    for name in fc.CASES:
        c = fc.case(name)
        assert fc.plan_expected(c, True) == fc.must_run(name), name
        assert fc.plan_expected(c, False) == (0, 0)
        assert c["hits"].max() <= c["L"] and (c["cube"] <= c["hits"][:, None].astype(np.float64) * ((1 << c["hdr"]["nbits"]) - 1)).all(), name
    assert fc.chunk(64) == 85 and fc.case("nsub_chunk_nbin64")["nsub"] == 85 and fc.case("nsub_chunk_plus1_nbin64")["nsub"] == 86
    assert fc.chunk(1024) == 5 and fc.case("nbin1024_chunk_plus1")["nsub"] == 6
    c = fc.case("nbin1000_zero_bins_many_turns")
    _dms, shd, shp, tau = fo.tables(c["hdr"], c["nrows"], c["nbin"], c["nsub"], c["f0_fold"], c["subint_s"], c["dm0"], c["ndm"], c["ddm"], c["nfreq"],
                                   c["dfreq"], c["nfdot"], c["dfdot"])
    turns = fo.delay_s(c["hdr"], c["dm0"]) * c["f0_fold"]
    assert turns.max() > 50 and len(set(shd[1].tolist())) > 8                    # many turns, wrapped into 0 .. 999
    w = fc.want("nbin1000_zero_bins_many_turns")
    assert (w["prof_hits"] > 0).all() and w["results"]["score_peak"][0] > 0      # (the empty bins of the channels land on different bins)
    c = fc.case("nsub2_nbin64_short_last")
    assert c["nrows"] == 64 + 17
    _dms, _shd, shp, tau = fo.tables(c["hdr"], c["nrows"], c["nbin"], c["nsub"], c["f0_fold"], c["subint_s"], c["dm0"], c["ndm"], c["ddm"], c["nfreq"],
                                    c["dfreq"], c["nfdot"], c["dfdot"])
    assert tau[0] < 0 < tau[1] and abs(tau[0]) != abs(tau[1])                    # the short last sub-integration moves the middle
    assert shp[1, 0].tolist() != shp[1, 4].tolist() and (shp[1, 2] == 0).all()   # negative and positive spin shifts; the centre: none
    w = fc.want("dead_and_flagged_ascending")
    c = fc.case("dead_and_flagged_ascending")
    assert not c["hits"][:, :, 3].any() and c["flag"].tolist().count(1) == 2 and c["hdr"]["foff"] > 0
    assert int(w["plane_hits"].sum()) == int(c["hits"][:, :, [i for i in range(16) if i not in (5, 15)]].sum())
    w, c = fc.want("full_scale_2p53"), fc.case("full_scale_2p53")
    total = 65535 * c["nrows"] * 8 * 4
    assert total < 2 ** 53 <= 65535 * (c["nrows"] + 1) * 8 * 4 and int(w["plane_acc"].sum()) == total
    c = fc.case("full_scale_u32_edge")
    assert 65535 * 4 * c["L"] < 2 ** 32 <= 65535 * 4 * fc.case("u32_edge_one_more")["L"]
    assert fc.case("nchan264_two_tile_runs")["hdr"]["nchans"] // 8 == fc.TILE_RUN + 1 and fc.case("ndm9")["ndm"] == fc.DM_RUN + 1
    assert fc.case("coherency_mask3_u16")["products"] == 0b0011 and fc.case("coherency_mask3_u16")["hdr"]["nifs"] == 4


def test_one_trial_is_the_scrunched_profile(emu_lib):
    """with one trial on every axis B / H is the profile post._scrunched makes of the same cube in numpy, to the bit"""
    c = fc.case("one_trial")
    got = fit_of(emu_lib, c)
    prof = c["cube"][:, 0].transpose(0, 2, 1)                                    # [nsub][nchan][nbin], as fold_all returns it
    hits = c["hits"].transpose(0, 2, 1)
    _mean_f, profile = post._scrunched(prof, hits, c["hdr"], c["f0_fold"], c["dm0"], 16)
    mine = got["prof_acc"][0].astype(np.float64) / got["prof_hits"][0].astype(np.float64)
    assert (got["prof_hits"][0] > 0).all() and mine.tobytes() == profile.tobytes()
    assert got["prof_acc"][0].tobytes() == got["prof_acc"][1].tobytes() and got["score"].shape == (1, 1, 1)
    r = got["results"][0]
    assert (r["kpeak"], r["jpeak"], r["ipeak"], r["fitted_dm"], r["fitted_freq"], r["fitted_fdot"]) == (0, 0, 0, 0, 0, 0)
    assert r["dm"] == c["dm0"] and r["dfreq"] == 0.0 and r["dfdot"] == 0.0 and r["border_median"] == 0.0 and r["dm_res"] == 0.0


@pytest.mark.parametrize("name", ["nsub2_nbin64_short_last", "ndm9", "nspin33", "one_trial"])
def test_the_peaks_alone(emu_lib, name):
    c, want = fc.case(name), fc.want(name)
    res = np.full(1, 0, post.FOLDFIT_RESULT)
    res.view(np.uint8)[:] = 0xA5
    err = C.create_string_buffer(256)
    score, acc, hits = (np.ascontiguousarray(want[f]) for f in ("score", "prof_acc", "prof_hits"))
    code = emu_lib.frbch_foldfit_peaks(C.byref(fc.par_of(c)), score.ctypes.data, acc.ctypes.data, hits.ctypes.data, res.ctypes.data, err, len(err))
    assert code == 0, err.value
    assert res.tobytes() == want["results"].tobytes()


def test_the_steps(emu_lib):
    c = fc.case("nsub2_nbin64_short_last")
    got = post.foldfit_steps(c["hdr"], c["nrows"], c["nbin"], c["f0_fold"], lib=emu_lib)
    assert np.array(got).tobytes() == np.array([float(v) for v in fo.steps(c["hdr"], c["nrows"], c["nbin"], c["f0_fold"])]).tobytes()
    T = c["nrows"] * c["hdr"]["tsamp"]
    assert got[1] == pytest.approx(1.0 / (c["nbin"] * T)) and got[2] == pytest.approx(8.0 / (c["nbin"] * T * T))


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _refused(lib, c, message, par=None, desc=None, nrows=None, fn=None, drop=()):
    out = fc.outputs(c, fill=0x5A)
    for key in drop:
        del out[key]
    before = {f: a.tobytes() for f, a in out.items()}
    code, msg, out, k = fc.call(fn or lib.frbch_foldfit_host, c, c["cube"].ctypes.data, c["hits"].ctypes.data, out=out, par=par, desc=desc, nrows=nrows)
    assert code == _lib.E_ARG and message in msg, (code, msg)
    assert all(out[f].tobytes() == before[f] for f in out) and k == (7, 7)


def test_refusals(emu_lib):
    c = fc.case("nsub2_nbin64_short_last")

    def par(**kw):
        p = fc.par_of(c)
        for key, v in kw.items():
            setattr(p, key, v)
        return p
    for fn in (emu_lib.frbch_foldfit_host, emu_lib.frbch_foldfit_device):
        _refused(emu_lib, c, "frbch_foldfit_params: wrong size", par=par(size=8), fn=fn)
        _refused(emu_lib, c, "ndm must be odd or 1", par=par(ndm=4), fn=fn)
        _refused(emu_lib, c, "nfreq must be odd or 1", par=par(nfreq=2), fn=fn)
        _refused(emu_lib, c, "nfdot must be odd or 1", par=par(nfdot=0), fn=fn)
    _refused(emu_lib, c, "exceeds 2^22", par=par(ndm=2049, nfreq=2049, nfdot=1))
    _refused(emu_lib, c, "nbin must be 2..4096", par=par(nbin=1))
    _refused(emu_lib, c, "nbin must be 2..4096", par=par(nbin=4097))
    _refused(emu_lib, c, "nsub must be 1..4096", par=par(nsub=0))
    _refused(emu_lib, c, "nsub must be 1..4096", par=par(nsub=4097))
    _refused(emu_lib, c, "nsub must be frbch_fold_nsub()", par=par(nsub=3))
    d = fc.desc_of(c)
    d.nchan = 16385
    _refused(emu_lib, c, "more than 16384 channels", desc=d)
    d = fc.desc_of(c)
    d.nbits = 32
    _refused(emu_lib, c, "float rows", desc=d)
    _refused(emu_lib, c, "products: an empty mask", par=par(products=0))
    _refused(emu_lib, c, "products: a product beyond nifs", par=par(products=2))
    _refused(emu_lib, c, "ddm is not finite", par=par(ddm=float("nan")))
    _refused(emu_lib, c, "dfreq is not finite", par=par(dfreq=float("inf")))
    _refused(emu_lib, c, "dfdot must be positive", par=par(dfdot=0.0))
    _refused(emu_lib, c, "ddm must be positive", par=par(ddm=-1.0))
    _refused(emu_lib, c, "DM trial 0 lies outside [0, 1e5)", par=par(dm0=0.0))
    _refused(emu_lib, c, "DM trial 2 lies outside [0, 1e5)", par=par(dm0=1.0e5 - 1e-9))
    _refused(emu_lib, c, "fit_frac must lie in (0, 1]", par=par(fit_frac=0.0))
    _refused(emu_lib, c, "nwidth must be 1..8", par=par(nwidth=9))
    _refused(emu_lib, c, "a width outside 1..nbin / 2", par=par(widths=(C.c_uint32 * 8)(33, 1, 1, 1, 1, 1, 1, 1)))
    _refused(emu_lib, c, "a DM shift beyond 2^52 bins", par=par(f0_fold=1.0e17))
    _refused(emu_lib, c, "reaches 2^53", nrows=2 ** 53 // (255 * 8) + 1)
    _refused(emu_lib, c, "trial_acc and trial_hits come together", drop=("trial_hits",))
    big = dict(c, ndm=1, nfreq=513, nfdot=513, want_trials=True)                                   # 2^18 trials of 64 bins: above 2^24 elements
    code, msg, _out, _k = fc.call(emu_lib.frbch_foldfit_host, c, c["cube"].ctypes.data, c["hits"].ctypes.data, out=fc.outputs(big), par=fc.par_of(big))
    assert code == _lib.E_ARG and "exceed 2^24 elements" in msg
    # the bound exactly: the case at the largest product below 2^53 runs, one row more is refused
    c = fc.case("full_scale_2p53")
    _refused(emu_lib, c, "reaches 2^53", nrows=c["nrows"] + 1)


def test_python_refuses_a_cube_of_the_wrong_shape(emu_lib):
    c = fc.case("one_trial")
    with pytest.raises(post.InputError, match="the cube must be"):
        post.fold_fit(c["cube"].transpose(0, 1, 3, 2), c["hits"], c["hdr"], c["nrows"], fc.par_of(c), lib=emu_lib)


# ---- the composite ----------------------------------------------------------------------------------------------------
def test_fold_refine_equals_fold_then_fit(emu_lib):
    """rows -> fold -> search in one residency: the bytes of frbch_foldp_host followed by frbch_foldfit_host, and of the restatement"""
    hdr, par, _truth, _steps = fc.known_setup()
    rows = fc.known_rows(fc.KNOWN_SEEDS[0])[:8192]
    k = fc.KNOWN
    nsub = emu_lib.frbch_fold_nsub(C.byref(post.fil_desc(hdr)), rows.shape[0], k["subint_s"])
    model, _keep = post.fold_model(par, hdr, nbin=k["nbin"], subint_s=k["subint_s"], apply_delays=False)
    fpar = post.foldfit_params(hdr, rows.shape[0], k["nbin"], nsub, par["F0"], k["subint_s"], par["DM"], ndm=3, nfreq=5, nfdot=3, lib=emu_lib)
    info = {}
    one = post.fold_refine(rows, hdr, model, fpar, want_cube=True, lib=emu_lib, info=info)
    assert info == dict(kernel_used=(0, 0, 0))
    cube = np.zeros((nsub, 1, k["nbin"], k["nchan"]))
    hits = np.zeros((nsub, k["nbin"], k["nchan"]), np.uint32)
    err = C.create_string_buffer(256)
    assert emu_lib.frbch_foldp_host(C.byref(post.fil_desc(hdr)), rows.ctypes.data, rows.shape[0], C.byref(model), 0, cube.ctypes.data, hits.ctypes.data,
                                    nsub, None, err, len(err)) == 0, err.value
    assert one["cube"].tobytes() == cube.tobytes() and one["cube_hits"].tobytes() == hits.tobytes()
    two = post.fold_fit(cube, hits, hdr, rows.shape[0], fpar, lib=emu_lib)
    assert fc.same(one, two) and all(f in one for f in ("score", "prof_acc", "prof_hits", "results", "plane_acc", "plane_hits"))
    ax = post.foldfit_axes(fpar)
    want = fo.fold_fit(cube, hits, hdr, rows.shape[0], f0_fold=par["F0"], subint_s=k["subint_s"], products=1, dm0=par["DM"], ndm=3, ddm=fpar.ddm,
                       nfreq=5, dfreq=fpar.dfreq, nfdot=3, dfdot=fpar.dfdot, fit_frac=0.5, widths=list(fpar.widths[: fpar.nwidth]))
    assert fc.same(one, want), fc.differing(one, want)
    assert ax["dm"][1] == par["DM"] and ax["dfreq"][2] == 0.0
    # without the cube: the same results; a fold with per-channel delays is refused
    assert fc.same(post.fold_refine(rows, hdr, model, fpar, lib=emu_lib), two)
    delayed, _keep2 = post.fold_model(par, hdr, nbin=k["nbin"], subint_s=k["subint_s"], apply_delays=True)
    with pytest.raises(post.InputError, match="apply_delays"):
        post.fold_refine(rows, hdr, delayed, fpar, lib=emu_lib)
    # a refusal that only the tables show (a DM trial below 0) leaves the cube's outputs untouched as well
    low = post.foldfit_params(hdr, rows.shape[0], k["nbin"], nsub, par["F0"], k["subint_s"], 0.0, ndm=3, nfreq=5, nfdot=3, lib=emu_lib)
    cube_out, hits_out = np.full_like(cube, 7.0), np.full_like(hits, 7)
    err = C.create_string_buffer(256)
    sc, pa, ph, rs = np.full((3, 3, 5), 7.0), np.zeros((2, 64), np.int64), np.zeros((2, 64), np.uint64), np.zeros(1, post.FOLDFIT_RESULT)
    code = emu_lib.frbch_fold_refine_host(C.byref(post.fil_desc(hdr)), rows.ctypes.data, rows.shape[0], C.byref(model), C.byref(low), None, 0,
                                          cube_out.ctypes.data, hits_out.ctypes.data, sc.ctypes.data, pa.ctypes.data, ph.ctypes.data, rs.ctypes.data,
                                          None, None, None, err, len(err))
    assert code == _lib.E_ARG and b"DM trial 0" in err.value and (cube_out == 7.0).all() and (hits_out == 7).all() and (sc == 7.0).all()
    other, _keep3 = post.fold_model(par, hdr, nbin=32, subint_s=k["subint_s"], apply_delays=False)
    with pytest.raises(post.InputError, match="differ in nbin or subint_s"):
        post.fold_refine(rows, hdr, other, fpar, lib=emu_lib)


# ---- the known answer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", fc.KNOWN_SEEDS)
def test_known_answer(emu_lib, seed):
    """F0 off by 0.6 / T, F1 by three steps, DM by five: every axis comes back within one grid step of the truth, and the best
    profile's S/N exceeds the nominal one's (tests/foldfit_cases.py says how the amplitude was fixed)"""
    got, info = fc.known_library(emu_lib, seed)
    r = got["results"][0]
    _hdr, _par, truth, (ddm, dfreq, dfdot) = fc.known_setup()
    print("seed %d: dm %.3f (%.3f) dfreq %.6f (%.6f) dfdot %.3e (%.3e)  S/N %.2f -> %.2f" % (seed, r["dm"], truth["dm"], r["dfreq"], truth["dfreq"],
                                                                                            r["dfdot"], truth["dfdot"], r["snr_nominal"], r["snr_best"]))
    assert info == dict(kernel_used=(0, 0, 0))
    assert abs(r["dm"] - truth["dm"]) <= ddm and abs(r["dfreq"] - truth["dfreq"]) <= dfreq and abs(r["dfdot"] - truth["dfdot"]) <= dfdot
    assert r["snr_best"] > r["snr_nominal"]


def test_known_answer_restated():
    """the restatement alone on the first seed: recovered, with the S/N that tests/foldfit_cases.py recorded"""
    r = fc.known_restatement(fc.KNOWN_SEEDS[0])
    assert fc.known_recovered(r)
    assert (round(float(r["snr_nominal"]), 2), round(float(r["snr_best"]), 2)) == fc.KNOWN_RECORD[fc.KNOWN_SEEDS[0]]


# ---- the commands -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def known_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("foldfit")
    hdr, par, _truth, _steps = fc.known_setup()
    path = str(d / "known.fil")
    from tests.test_fold_predictor import write_fil
    write_fil(path, fc.known_rows(fc.KNOWN_SEEDS[0]), hdr, 1)
    parfile = str(d / "known.par")
    with open(parfile, "w") as f:
        f.write("PSRJ known\nF0 %.15g\nF1 %.15g\nPEPOCH %.15f\nDM %.9f\n" % (par["F0"], par["F1"], par["PEPOCH"], par["DM"]))
    return path, parfile


def _snr_of_profile(path):
    x = np.loadtxt(path)[:, 1]
    return fo.snr_of(np.rint(x * 1e6).astype(np.int64), np.full(x.size, 10 ** 6, np.uint64), fc.KNOWN_WIDTHS)[0]


def test_foldfit_command(emu_lib, known_file, monkeypatch, capsys):
    path, parfile = known_file
    monkeypatch.setattr(_lib, "load", lambda *a, **k: emu_lib)
    k = fc.KNOWN
    post.main(["foldfit", path, parfile, "--nbin", "64", "-L", "2.048", "--ndm", "17", "--nfreq", "81", "--nfdot", "9", "--refold"])
    text = capsys.readouterr().out
    base = path + "_foldfit"
    for ext in (".npz", ".txt", ".png", ".par"):
        assert os.path.getsize(base + ext) > 0 and ("wrote " + base + ext) in text
    z = np.load(base + ".npz")
    r = z["results"][0]
    _hdr, _par, truth, (ddm, dfreq, dfdot) = fc.known_setup()
    assert z["score"].shape == (17, 9, 81) and z["plane_acc"].shape == (16, 64) and z["kernel_used"].tolist() == [0, 0, 0]
    # the planes of the plot: phase-time at the best DM adds up to the best profile's totals; phase-frequency has every channel, and
    # its pulse stands straighter than at the nominal trial (a higher peak of the band-summed profile)
    assert z["best_plane_acc"].shape == (16, 64) and z["phase_freq"].shape == (64, 64)
    assert int(z["best_plane_acc"].sum()) == int(z["prof_acc"][1].sum()) and int(z["best_plane_hits"].sum()) == int(z["prof_hits"][1].sum())
    band = z["phase_freq"].mean(axis=0)
    assert int(np.argmax(band)) == int(np.argmax(z["prof_acc"][1] / z["prof_hits"][1]))
    assert abs(r["dm"] - truth["dm"]) <= ddm and abs(r["dfreq"] - truth["dfreq"]) <= dfreq and abs(r["dfdot"] - truth["dfdot"]) <= dfdot
    assert "F0 " in text and "DM  %.6f" % r["dm"] in text and "S/N %.2f -> %.2f" % (r["snr_nominal"], r["snr_best"]) in text
    new = post.read_par(base + ".par")
    T = k["nrows"] * k["tsamp"]
    assert abs(new["F0"] - k["f0"]) <= dfreq and abs(new["F1"] - k["f1"]) <= dfdot and abs(new["DM"] - k["dm"]) <= ddm
    assert abs(new["PEPOCH"] - (60000.0 + 0.5 * T / 86400.0)) < 1e-9
    with open(base + ".png", "rb") as f:
        assert f.read(8) == b"\x89PNG\r\n\x1a\n"
    # the second fold with the refined .par is sharper than the fold with the ephemeris it started from
    post.main(["fold", path, parfile, "--nbin", "64", "-L", "2.048"])
    capsys.readouterr()
    assert _snr_of_profile(path + "_refold.profile.txt") > 1.5 * _snr_of_profile(path + ".profile.txt")
    # --f0 / --dm instead of a .par
    post.main(["foldfit", path, "--f0", "%.15g" % k["f0"], "--dm", "50", "--nbin", "64", "-L", "2.048", "--ndm", "3", "--nfreq", "3", "--nfdot", "1"])
    assert "wrote" in capsys.readouterr().out
    with pytest.raises(post.InputError, match="a .par file, or --f0 and --dm"):
        post.main(["foldfit", path, "--f0", "10"])
    with pytest.raises(post.InputError, match="fold --refine with --doppler"):
        post.main(["fold", path, parfile, "--doppler", "1e-4", "--refine"])


def test_fold_and_psearch_outputs_do_not_change_without_refine(emu_lib, known_file, tmp_path, monkeypatch, capsys):
    """`post fold` writes the same bytes with and without --refine, and no _foldfit file without it; likewise the folds of
    `post psearch --fold-best`"""
    import shutil
    path, parfile = known_file
    monkeypatch.setattr(_lib, "load", lambda *a, **k: emu_lib)
    runs = {}
    for tag, extra in (("plain", []), ("refine", ["--refine"])):
        d = tmp_path / tag
        d.mkdir()
        fil = str(d / "k.fil")
        shutil.copy(path, fil)
        post.main(["fold", fil, parfile, "--nbin", "64", "-L", "2.048"] + extra)
        post.main(["psearch", fil, "--dm", "50", "--fold-best", "1", "--sigma", "8"] + extra)
        runs[tag] = {n: open(str(d / n), "rb").read() for n in sorted(os.listdir(str(d))) if n != "k.fil"}
    capsys.readouterr()
    plain, refined = runs["plain"], runs["refine"]
    assert not any("foldfit" in n for n in plain) and set(plain) < set(refined)
    assert {"k.fil.ar", "k.fil.profile.txt", "k.fil.png", "k_psearch_cand0.ar", "k_psearch_cand0.profile.txt"} <= set(plain)
    for n in plain:
        if not n.endswith(".npz"):                                               # (an .npz carries its time of writing)
            assert plain[n] == refined[n], n
    assert {"k.fil_foldfit.txt", "k.fil_foldfit.par", "k_psearch_cand0_foldfit.txt"} <= set(refined)
