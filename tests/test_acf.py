"""CPU tests of the structure of a burst (frbch_burstacf_*, frbch_acf2d_*, frbch_burstacf_fit) through the emulator build, which
runs the generic kernels: the dynamic spectrum, the ACF, the pair counts and the results byte for byte against the numpy
restatement tests/acf_oracle.py, the _device twin into pre-filled outputs, the ACF stage alone on planes from a formula, the
oracle-free properties, every refusal with its message and untouched outputs, the magnitudes the full-scale cases reach, bursts
of known drift and known decorrelation scale, `post burstacf` end to end, and a walk of failing device-layer calls.

The known answers (tests/acf_cases.py: 64 channels at 1.2 - 1.5 GHz, noise 96 +- 12, bins of 4 rows, 32 x 127 lags, fit_frac 0.25),
measured with the restatement alone on this CPU over the noise seeds 0 .. 11; every tolerance asserted below is twice the largest
deviation seen:
  three sub-bursts 75 MHz and 3.75 ms apart (drift -20 MHz/ms, dt_df -0.05 ms/MHz): dt_df -0.05204 .. -0.04679, largest deviation
    0.00321 -> 0.0065 ms/MHz asserted; drift -21.374 .. -19.217 MHz/ms, largest deviation 1.374 -> 2.75 MHz/ms asserted;
  the same three at one time (the undrifted control): |dt_df| <= 0.00342; |dt_df| of the drifted case less that of the control on
    the same seed 0.04494 .. 0.05172, at most 0.00506 from the 0.05 injected -> a difference of at least 0.0398 asserted;
  one component whose spectrum is four Gaussian scintles of sigma 2 channels and whose profile has sigma 12 rows (the header's rule
    on the noise-free Gaussian ACFs gives half-widths of 16.299 MHz and 1.3042 ms): 15.960 .. 19.231 MHz, largest deviation 2.932
    -> 5.87 MHz asserted; 1.2138 .. 1.4435 ms, largest deviation 0.1393 -> 0.279 ms asserted."""
import ctypes as C
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import acf_cases as ac
from tests import acf_oracle as ao
from tests import rm_cases as rc

TOL_DT_DF, TOL_DRIFT, MIN_GAP, TOL_WF, TOL_WT = 0.0065, 2.75, 0.0398, 5.87, 0.279


def acf_of(lib, c, info=None, **kw):
    a = dict(fit_frac=c["fit_frac"], flag=c["flag"], products="coherency" if c["coh"] else "stokes")
    a.update(kw)
    return post.burst_acf(c["rows"], c["hdr"], c["cands"], c["nbin"], c["tfactor"], c["ffactor"], c["nlagf"], c["nlagt"], lib=lib, info=info, **a)


# ---- the library against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_composite_equals_the_oracle(emu_lib, name):
    c, want = ac.case(name), ac.want(name)
    info = {}
    got = acf_of(emu_lib, c, info)
    assert info == dict(spectra_kernel_used=0, dynspec_kernel_used=0, kernel_used=0)
    assert ac.differing(got, want) == [] and got["norm"].tobytes() == want["norm"].tobytes()
    assert ac.query(emu_lib, c, c["rows"].ctypes.data) == (0, (0, 0, 0))
    # the _device twin (the emulator's device memory is host memory) writes the same bytes into outputs that held something else
    code, msg, out, k = ac.call(emu_lib.frbch_burstacf_device, c, c["rows"].ctypes.data, out=ac.outputs_of(c, fill=0xA5))
    assert code == 0 and k == (0, 0, 0), msg
    assert ac.differing(out, got) == []
    # the fit alone, from the planes
    norm = np.full(want["norm"].shape, 7.0)
    res = np.zeros(want["results"].size, dtype=post.ACF_RESULT)
    err = C.create_string_buffer(256)
    arrs = [np.ascontiguousarray(want[f]) for f in ("k", "r", "nused", "ncomplete", "A", "P")]
    code = emu_lib.frbch_burstacf_fit(C.byref(post.fil_desc(c["hdr"], 0)), C.byref(ac.par_of(c)), C.byref(ac.fit_par_of(c)), res.size,
                                      *[a.ctypes.data for a in arrs], norm.ctypes.data, res.ctypes.data, err, len(err))
    assert code == 0, err.value
    assert norm.tobytes() == want["norm"].tobytes() and res.tobytes() == want["results"].tobytes()
    # the quantised plane of the restatement through the stage alone gives the same A, and the 0 / 1 plane gives P
    for plane, field in ((want["y"], "A"), (want["mask"].astype(np.int32), "P")):
        A = post.acf2d(plane, c["nlagf"], c["nlagt"], lib=emu_lib)
        assert A.astype(want[field].dtype).tobytes() == want[field].tobytes(), field


def test_the_cases_reach_their_edges():
    """the restatement alone: what each case is there for"""
    w = ac.want("u8_64ch_f1_full_lags")
    assert w["A"].shape == (2, 64, 65) and (w["ncomplete"] == 64 * 33).all() and (w["yhits"] == 3).all()
    assert w["A"][0, 63, 0] == int(w["y"][0, 0, 32]) * int(w["y"][0, 63, 0]) and w["P"][0, 63, 0] == 1      # the corner lag: a single product
    assert w["A"][0, 63, 64] == int(w["y"][0, 0, 0]) * int(w["y"][0, 63, 32])
    assert (w["r"] > 0).all() and (1 << 20) <= np.abs(w["y"][0]).max() <= ao.Y_MAX
    w = ac.want("u8_64ch_f4_full_lags")
    assert w["Y"].shape == (2, 16, 33) and (w["yhits"] == 12).all()
    w = ac.want("u8_64ch_1x1x1")
    assert w["A"].shape == (1, 1, 1) and w["A"][0, 0, 0] == int(w["y"][0, 0, 0]) ** 2 > 0 and w["P"][0, 0, 0] == 1
    r = w["results"][0]
    assert (r["fitted_f"], r["fitted_t"], r["fitted_d"], r["ref"]) == (0, 0, 0, 0.0) and r["nused"] == 64
    w = ac.want("u8_64ch_one_subband")
    assert w["Y"].shape == (2, 1, 40) and w["A"].shape == (2, 1, 39)
    w = ac.want("u8_64ch_windows_leave_the_file")                   # B_EDGE: bins in front of row 0; B_END: behind the last row
    full = ao.pairs_closed_form(32, 256, 8, 16)
    assert 0 < w["ncomplete"][1] < w["ncomplete"][0] < 32 * 256 and (w["P"][0] < full).any() and (w["P"] <= full).all()
    assert (w["mask"][0] == 0).any() and ((w["yhits"][0] > 0) & (w["mask"][0] == 0)).any()       # partial cells exist, and are left out
    assert (w["y"][w["mask"] == 0] == 0).all()
    w = ac.want("u8_64ch_flag_constant_dead")                       # flags 0, 16, 17, 63; constant columns 5, 40; B_OUT in the middle
    assert not w["used"][:, [0, 16, 17, 63, 5, 40]].any() and w["nused"].tolist() == [58, 0, 58]
    assert w["nused_s"][0, 8] == 0 and not w["mask"][0, 8].any() and w["nused_s"][0, 0] == 1 and w["mask"][0, 0].all()
    assert not w["results"][1:2].view(np.uint8).any() and not w["A"][1].any() and not w["P"][1].any() and w["ncomplete"][0] == 31 * 33
    w = ac.want("u16_64ch_coherency")
    assert w["nused"].tolist() == [64, 64, 64] and ac.case("u16_64ch_coherency")["rows"].dtype == np.uint16
    w = ac.want("u8_96ch_ascending")
    assert w["nused"].tolist() == [96, 96, 0] and ac.case("u8_96ch_ascending")["hdr"]["foff"] > 0
    assert ac.case("u8_64ch_one_product")["rows"].shape[1] == 1 and ac.case("u8_64ch_product2")["hdr"]["product"] == 2
    for name, fits in (("u8_1024ch_edge_fits", True), ("u8_1024ch_edge_one_more", False)):
        c = ac.case(name)
        rng = ac.dc.tile_range(c["hdr"], 1, c["cands"], 1, 0.0, 1)
        assert rng == 898 and (c["tfactor"] + rng <= 1024) == fits and ac.dyn_plan_expected(c, True) == int(fits), (name, rng)
        assert ac.want(name)["nused"].tolist() == [1024]
    assert ac.case("u8_1024ch_edge_fits")["tfactor"] + 898 == 1024 == ac.case("u8_1024ch_edge_one_more")["tfactor"] + 897
    assert sorted(ac.DYN_FAST + ac.DYN_GENERIC) == sorted(ac.CASES)
    for name in ac.CASES:
        assert ac.dyn_plan_expected(ac.case(name), True) == int(name in ac.DYN_FAST), name
        assert ac.dyn_plan_expected(ac.case(name), False) == 0
    # the ACF stage: the slab of the edge geometry is 78 rows, 75 with one bin more; the partials cap
    assert ac.acf_plan(1, 1000, 64, 8, 16)["sb"] == 78 and ac.acf_plan(1, 1000, 65, 8, 16)["sb"] == 75
    assert ac.acf_plan(1, 78, 64, 8, 16)["nslab"] == 1 and ac.acf_plan(1, 79, 64, 8, 16)["nslab"] == 2 and ac.acf_plan(1, 78, 65, 8, 16)["nslab"] == 2
    assert ac.acf_plan(1, 1024, 1024, 1024, 256) == dict(sb=4, dfr=4, nslab=256) and ac.acf_plan(2, 1024, 1024, 1024, 256) is None
    assert ac.acf_plan(2, 230, 50, 11, 10) == dict(sb=100, dfr=8, nslab=3)


def test_the_magnitudes_of_the_full_scale_cases():
    """2^20 complete cells at one large Y: |y| between 2^20 and 2^21, A[0][0] above 2^60 and equal to the sum in Python integers;
    the planes of +-2^21 reach 2^62, the header's bound, exactly"""
    w = ac.want("u8_1024ch_full_scale")
    y = w["y"][0].astype(np.int64)
    total = sum(int(v) * int(v) for v in y[:, 0]) * 1024 if (y == y[:, :1]).all() else sum(int(v) ** 2 for v in y.reshape(-1))
    print("largest |X| = 2^%.3f, r = %d, |y| = 2^%.3f .. 2^%.3f, A[0][0] = 2^%.3f" % (
        np.log2(w["largest"]), w["r"][0], np.log2(np.abs(y).min()), np.log2(np.abs(y).max()), np.log2(float(total))))
    assert w["ncomplete"][0] == 1 << 20 and (1 << 39) < w["largest"] <= (1 << 40)
    assert (1 << 20) <= np.abs(y).min() and np.abs(y).max() <= (1 << 21)
    assert int(w["A"][0, 0, 1]) == total > (1 << 60)
    assert (w["P"][0] == ao.pairs_closed_form(1024, 1024, 2, 2)).all()
    for name, sign in (("plus_full_scale_1024x1024", 1), ("alternating_full_scale_1024x1024", -1)):
        A = ac.plane_want(name)[0]
        assert int(A[0, 1]) == 1 << 62 and int(A[0, 0]) == sign * (1 << 42) * 1024 * 1023 and int(A[1, 1]) == sign * (1 << 42) * 1023 * 1024
        assert int(A[1, 0]) == (1 << 42) * 1023 * 1023


# ---- the ACF stage alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ac.PLANES))
def test_acf_stage_equals_the_oracle(emu_lib, name):
    n, nsub, nbin, lf, lt, _kind = ac.PLANES[name]
    y, want = ac.plane(name), ac.plane_want(name)
    for fn in (emu_lib.frbch_acf2d_host, emu_lib.frbch_acf2d_device):
        code, msg, A, k = ac.acf2d_call(fn, y.ctypes.data, y.shape, lf, lt)
        assert code == 0 and k == 0, msg
        assert A.tobytes() == want.tobytes()
    assert emu_lib.frbch_acf2d_kernel(n, nsub, nbin, lf, lt, _lib.ACF_PLAN) == 0
    # oracle-free: the row df = 0 is even in dt, and the zero lag is the sum of squares
    assert (want[:, 0, :] == want[:, 0, ::-1]).all()
    assert [int(v) for v in want[:, 0, lt - 1]] == [sum(int(v) ** 2 for v in p.reshape(-1)) for p in y]


def test_acf_stage_refusals(emu_lib):
    y = ac.plane("random_3x5_full_lags")
    host = emu_lib.frbch_acf2d_host
    bad = y.copy()
    bad[1, 2, 3] = ao.Y_MAX + 1
    for arr, shape, lf, lt, form, text in (
            (bad, y.shape, 3, 5, 0, "outside -2^21"), (-bad, y.shape, 3, 5, 0, "outside -2^21"), (y, y.shape, 0, 5, 0, "nlagf"), (y, y.shape, 4, 5, 0, "nlagf"),
            (y, y.shape, 3, 0, 0, "nlagt"), (y, y.shape, 3, 6, 0, "nlagt"), (y, y.shape, 3, 5, 2, "form"), (y, (0, 3, 5), 3, 5, 0, "at least one"),
            (y, (2, 0, 5), 3, 5, 0, "at least one"), (y, (2, 3, 0), 3, 5, 0, "nbin"), (y, (2, 3, 1025), 3, 5, 0, "nbin"), (y, (1, 2048, 1024), 3, 5, 0, "2^20"),
            (y, (17, 1024, 1024), 3, 5, 0, "2^24"), (y, (65536, 16, 16), 16, 9, 0, "2^24"), (y, (1, 2000, 300), 1025, 5, 0, "nlagf"),
            (y, (1, 2, 300), 2, 257, 0, "nlagt")):
        code, msg, A, _k = ac.acf2d_call(host, arr.ctypes.data, shape, lf, lt, form)
        assert code == _lib.E_ARG and text in msg, (shape, lf, lt, form, msg)
        assert (A == 0x5A5A5A5A5A5A5A5A).all()
        assert emu_lib.frbch_acf2d_kernel(shape[0], shape[1], shape[2], lf, lt, form) == (_lib.E_ARG if arr is y else 0)
    assert ac.acf2d_call(host, None, y.shape, 3, 5)[0] == _lib.E_ARG
    code, _msg, A, _k = ac.acf2d_call(host, y.ctypes.data, y.shape, 3, 5, _lib.ACF_GENERIC)
    assert code == 0 and A.tobytes() == ac.plane_want("random_3x5_full_lags").tobytes()
    with pytest.raises(post.InputError, match="outside"):
        post.acf2d(bad, 3, 5, lib=emu_lib)


# ---- oracle-free properties of the composite ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("u8_64ch_f4_full_lags", "u8_64ch_windows_leave_the_file", "u8_64ch_flag_constant_dead", "u16_64ch_coherency",
                                  "u8_192ch_f3_generic"))
def test_properties_that_need_no_oracle(emu_lib, name):
    c = ac.case(name)
    got = acf_of(emu_lib, c)
    check_properties(emu_lib, c, got)


def check_properties(lib, c, got):
    """A[0][dt] = A[0][-dt]; P likewise, and equal to the closed form where every cell is complete; the band sum of Y and yhits is
    the DM scan's plane at one trial, through the library"""
    nsub, nbin = got["Y"].shape[1:]
    assert (got["A"][:, 0, :] == got["A"][:, 0, ::-1]).all() and (got["P"][:, 0, :] == got["P"][:, 0, ::-1]).all()
    closed = ao.pairs_closed_form(nsub, nbin, c["nlagf"], c["nlagt"])
    for i, r in enumerate(got["results"]):
        if r["ncomplete"] == nsub * nbin:
            assert (got["P"][i] == closed).all()
        else:
            assert (got["P"][i] <= closed).all() and (got["P"][i] < closed).any()
        assert got["P"][i, 0, c["nlagt"] - 1] == r["ncomplete"]
    acc, hits = ac.dmscan_band_sums(lib, c)
    assert got["Y"].sum(axis=1).tobytes() == acc.tobytes() and got["yhits"].sum(axis=1, dtype=np.uint32).tobytes() == hits.tobytes()


def test_closed_form_and_counted_pairs_agree(emu_lib):
    """a call whose cells are all complete writes P in closed form; the same candidate beside one that is not complete has its P
    counted by the kernel on the 0 / 1 plane: the two are equal"""
    c = ac.case("u8_64ch_f4_full_lags")
    alone = acf_of(emu_lib, c)
    cands = post.burst_cands([(b["dm"], b["sample"], b["width"]) for b in (ac.B1, ac.B_END)], 16, 200)
    both = post.burst_acf(c["rows"], c["hdr"], cands, c["nbin"], c["tfactor"], c["ffactor"], c["nlagf"], c["nlagt"], lib=emu_lib)
    assert both["results"]["ncomplete"][0] == 16 * 33 > both["results"]["ncomplete"][1]
    assert both["P"][0].tobytes() == alone["P"][0].tobytes() == ao.pairs_closed_form(16, 33, 16, 33).tobytes()
    assert both["A"][0].tobytes() == alone["A"][0].tobytes()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(emu_lib):
    c = ac.case("u8_64ch_f4_full_lags")
    hdr, ptr = c["hdr"], c["rows"].ctypes.data
    host = emu_lib.frbch_burstacf_host

    def cand(field, value, i=0):
        cc = c["cands"].copy()
        cc[field][i] = value
        return cc

    assert ac.call(host, c, ptr)[0] == 0
    par, fp = (lambda **kw: ac.par_of(c, **kw)), (lambda **kw: ac.fit_par_of(c, **kw))
    refused = [
        (dict(par=par(size=28)), "frbch_acf_params: wrong size"), (dict(par=par(nbin=0)), "nbin"), (dict(par=par(nbin=1025)), "nbin"),
        (dict(par=par(tfactor=0)), "tfactor"), (dict(par=par(tfactor=513)), "tfactor"), (dict(par=par(ffactor=0)), "ffactor"),
        (dict(par=par(ffactor=65)), "ffactor"), (dict(par=par(ffactor=3)), "ffactor"), (dict(par=par(nlagf=0)), "nlagf"),
        (dict(par=par(nlagf=17)), "nlagf"), (dict(par=par(nlagt=0)), "nlagt"), (dict(par=par(nlagt=34)), "nlagt"),
        (dict(par=par(nbin=1024, nlagt=257)), "nlagt"),
        (dict(hdr=dict(hdr, nchans=2048), par=par(ffactor=1, nbin=1024)), "2^20"),
        (dict(cands=np.repeat(c["cands"][:1], 257), par=par(ffactor=1, nbin=1024, nlagf=1, nlagt=1)), "ncand * nsub * nbin exceeds 2^24"),
        (dict(cands=np.repeat(c["cands"][:1], 4096), par=par(ffactor=1, nbin=33, nlagf=64, nlagt=33)), "(2 nlagt - 1) exceeds 2^24"),
        (dict(fp=fp(size=8)), "frbch_acf_fit_params: wrong size"), (dict(fp=fp(fit_frac=0.0)), "fit_frac"), (dict(fp=fp(fit_frac=1.0)), "fit_frac"),
        (dict(fp=fp(fit_frac=np.nan)), "fit_frac"),
        (dict(hdr=dict(hdr, nbits=32)), "not built for float32"), (dict(hdr=dict(hdr, nifs=2), bpar=rc.burst_par(True)), "nifs = 4"),
        (dict(hdr=dict(hdr, nchans=16385), par=par(ffactor=16385)), "16384"), (dict(ncand=0), "candidates"),
        (dict(cands=np.repeat(c["cands"][:1], 4097)), "candidates"),
        (dict(cands=cand("width", 0)), "width"), (dict(cands=cand("off_len", 1)), "off_len"), (dict(cands=cand("dm", -1.0)), "DM"),
        (dict(cands=cand("dm", np.nan)), "DM"), (dict(bpar=rc.burst_par(size=4)), "frbch_burst_params: wrong size"),
    ]
    for kw, text in refused:
        out = ac.outputs(2, 16, 33, 16, 33, 64, fill=0xA5)
        code, msg, out, _k = ac.call(host, c, ptr, out=out, **kw)
        assert code == _lib.E_ARG and text in msg, (kw, msg)
        assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), kw
        code2 = ac.call(emu_lib.frbch_burstacf_device, c, ptr, out=out, **kw)[0]
        assert code2 == _lib.E_ARG and all((a.view(np.uint8) == 0xA5).all() for a in out.values()), kw
    assert ac.query(emu_lib, c, ptr, par=par(nbin=1025))[0] == _lib.E_ARG and ac.query(emu_lib, c, None)[0] == _lib.E_ARG
    assert ac.query(emu_lib, c, ptr, par=par(ffactor=3))[0] == _lib.E_ARG and ac.query(emu_lib, c, ptr, cands=cand("dm", np.nan))[0] == _lib.E_ARG
    assert ac.call(host, c, None)[0] == _lib.E_ARG
    with pytest.raises(post.InputError, match="float32"):
        post.burst_acf(c["rows"].astype(np.float32), dict(hdr, nbits=32), c["cands"], lib=emu_lib)
    with pytest.raises(post.InputError, match="ffactor"):
        post.burst_acf(c["rows"], hdr, c["cands"], ffactor=3, lib=emu_lib)


# ---- the known answers ------------------------------------------------------------------------------------------------
def test_the_oracle_returns_the_injected_drift_and_widths():
    """before anything relies on it: the restatement alone on the fixed seed (the module's docstring says where the tolerances
    come from)"""
    dt_df, wf, wt = ac.known_expected()
    d, ctl, s = (ac.known_oracle(ac.KNOWN_SEED, kind)["results"][0] for kind in ("drift", "control", "scint"))
    print("drift: dt_df %+.5f ms/MHz, drift %+.3f MHz/ms; control dt_df %+.5f; scintles: %.4f MHz (expected %.4f), %.4f ms (expected %.4f)" % (
        d["dt_df"], d["drift"], ctl["dt_df"], s["width_f_mhz"], wf, s["width_t_ms"], wt))
    assert d["fitted_d"] == 1 and ctl["fitted_d"] == 1 and s["fitted_f"] == 1 and s["fitted_t"] == 1 and d["nused"] == 64
    assert abs(d["dt_df"] - dt_df) <= TOL_DT_DF and abs(d["drift"] - ac.DRIFT) <= TOL_DRIFT
    assert abs(d["dt_df"]) - abs(ctl["dt_df"]) >= MIN_GAP
    assert abs(s["width_f_mhz"] - wf) <= TOL_WF and abs(s["width_t_ms"] - wt) <= TOL_WT
    assert abs(wf - 16.299) < 1e-3 and abs(wt - 1.3042) < 1e-4


@pytest.mark.parametrize("kind", ("drift", "control", "scint"))
def test_known_answer(emu_lib, kind):
    check_known_answer(emu_lib, kind)


def check_known_answer(lib, kind, info=None):
    g = ac.KNOWN_GRID
    want = ac.known_oracle(ac.KNOWN_SEED, kind)
    got = post.burst_acf(ac.known_rows(ac.KNOWN_SEED, kind), ac.known_hdr(), ac.known_cands(), fit_frac=ac.KNOWN_FIT_FRAC, lib=lib, info=info, **g)
    assert ac.differing(got, want) == [] and got["norm"].tobytes() == want["norm"].tobytes()
    dt_df, wf, wt = ac.known_expected()
    r = got["results"][0]
    if kind == "drift":
        assert r["fitted_d"] == 1 and abs(r["dt_df"] - dt_df) <= TOL_DT_DF and abs(r["drift"] - ac.DRIFT) <= TOL_DRIFT
    elif kind == "control":
        drifted = ac.known_oracle(ac.KNOWN_SEED, "drift")["results"][0]
        assert abs(drifted["dt_df"]) - abs(r["dt_df"]) >= MIN_GAP
    else:
        assert r["fitted_f"] == 1 and r["fitted_t"] == 1 and abs(r["width_f_mhz"] - wf) <= TOL_WF and abs(r["width_t_ms"] - wt) <= TOL_WT


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_burstacf_end_to_end(emu_lib, tmp_path, capsys, monkeypatch):
    from tests.test_fold_predictor import write_fil
    hdr, rows = ac.known_hdr(), ac.known_rows(ac.KNOWN_SEED, "drift")
    fil = str(tmp_path / "burst.fil")
    write_fil(fil, rows, hdr, 1)
    base = fil.replace(".fil", "")
    before = set(os.listdir(tmp_path))
    g = ac.KNOWN_GRID
    info = {}
    files, acf = post.burstacf_fil(fil, [(ac.KNOWN_DM, ac.KNOWN_SAMPLE, 8)], nbin=g["nbin"], tfactor=g["tfactor"], ffactor=g["ffactor"], nlagf=g["nlagf"],
                                   nlagt=g["nlagt"], fit_frac=ac.KNOWN_FIT_FRAC, off_gap=400, off_len=400, lib=emu_lib, info=info)
    assert files == [base + "_acf.npz", base + "_acf.txt", base + "_acf.png"] and all(os.path.getsize(f) > 0 for f in files)
    assert set(os.listdir(tmp_path)) - before == {os.path.basename(f) for f in files} and info["kernel_used"] == 0
    want = ac.known_oracle(ac.KNOWN_SEED, "drift")
    back = np.load(files[0])
    for f in ac.FIELDS + ("norm",):
        assert back[f].tobytes() == np.ascontiguousarray(want[f]).tobytes() == np.ascontiguousarray(acf[f]).tobytes(), f
    line = open(files[1]).read().splitlines()
    assert len(line) == 1 and line[0].startswith("burst0") and ("drift %10.3f MHz/ms" % acf["results"]["drift"][0]) in line[0]
    assert open(files[2], "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    monkeypatch.setattr(_lib, "load", lambda path=None: emu_lib)
    for f in files:
        os.remove(f)
    assert post.main(["burstacf", fil, "--dm", repr(ac.KNOWN_DM), "--sample", str(ac.KNOWN_SAMPLE), "--width", "8", "--nbin", "128", "--tfactor", "4",
                      "--lagf", "32", "--lagt", "64", "--fit-frac", "0.25", "--off-gap", "400", "--off-len", "400"]) == 0
    assert "wrote " + files[0] in capsys.readouterr().out and np.load(files[0])["results"].tobytes() == acf["results"].tobytes()


# ---- failing device-layer calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("u8_64ch_f4_full_lags", "u8_64ch_flag_constant_dead"))
def test_a_failing_device_call_returns_the_error_and_leaves_nothing_behind(emu_lib, name):
    """every fallible device-layer call of frbch_burstacf_host fails once (n = 1, 2, ... until the call succeeds; the second case
    also counts its pairs on the device): an error with a message comes back, the outputs are untouched, the blocks and streams
    alive afterwards are those alive before, and a plain call right afterwards writes the expected bytes"""
    emu_lib.frbch_test_emu_fail_at.argtypes, emu_lib.frbch_test_emu_fail_at.restype = [C.c_long], None
    emu_lib.frbch_test_emu_live.argtypes, emu_lib.frbch_test_emu_live.restype = [], C.c_uint64
    c, want = ac.case(name), ac.want(name)
    ptr = c["rows"].ctypes.data
    rows0 = c["rows"].tobytes()
    codes = []
    for n in range(1, 200):
        out = ac.outputs_of(c, fill=0xA5)
        before = emu_lib.frbch_test_emu_live()
        emu_lib.frbch_test_emu_fail_at(n)
        try:
            code, msg, out, _k = ac.call(emu_lib.frbch_burstacf_host, c, ptr, out=out)
        finally:
            emu_lib.frbch_test_emu_fail_at(0)
        assert emu_lib.frbch_test_emu_live() == before, n
        if code == 0:
            assert ac.differing(out, want) == []
            break
        codes.append(code)
        assert code in (_lib.E_DEVICE, _lib.E_NOMEM) and msg, (n, code, msg)
        assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), n
    again = ac.call(emu_lib.frbch_burstacf_host, c, ptr)
    assert again[0] == 0 and ac.differing(again[2], want) == []
    assert 25 < len(codes) < 199 and c["rows"].tobytes() == rows0
