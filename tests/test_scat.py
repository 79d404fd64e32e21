"""CPU tests of the scattering of a burst (frbch_scat_bank, frbch_tbank_*, frbch_burstscat_*, frbch_burstscat_fit) through the
emulator build, which runs the generic kernels: the bank against its formula, the template-bank stage alone on planes from a
formula, the composite byte for byte against the numpy restatement tests/scat_oracle.py (which takes the library's bank as an
input), Y, yhits and y against frbch_burstacf_* and tests/acf_oracle.py, the closed form of N against the counted one, every
refusal with its message and untouched outputs, a noise-free plane of known template and arrival, bursts of known scattering,
`post scatter` end to end, and a walk of failing device-layer calls.

The known answers (tests/scat_cases.py: 64 channels at 1.2 - 1.5 GHz, noise 96 +- 12, a Gaussian of sigma 2 rows and fluence 500
per channel at DM 350.37, tau = 6 rows (nu / 1350 MHz)^-4; 8 subbands, bins of one row, a bank of 4 sigmas x 48 taus from 0.5
rows in steps of 2^(1/8), alpha 0 .. 8 in steps of 1), measured with the restatement alone over the noise seeds 0 .. 11; every
tolerance asserted below is twice the largest deviation seen:
  scattered: tau_ref 5.657 or 6.169 rows (the two grid values about 6), |ln(tau_ref / 6)| <= 0.0589 -> 0.118 asserted; alpha 3 .. 5,
    largest deviation 1 -> 2 asserted; every subband at S/N >= 21.9 (snr_min 5: all 8 take part); the interval tau_ref_lo ..
    tau_ref_hi holds the injected 6 rows for 2 seeds of 12 -- it is mostly a single grid point, and 6 lies between two --, and
    alpha_lo .. alpha_hi holds 4 for 10 of 12.
  the same burst unscattered: the band fit lands on tau_0 = 0.5 rows, the grid's edge, bounded_lo = 0, for 12 seeds of 12 (asserted);
    per subband either bounded_lo = 0 or dq_unscattered <= 20.7 -> 41.4 asserted."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import acf_oracle as ao
from tests import rm_cases as rc
from tests import scat_cases as sc
from tests import scat_oracle as so

TOL_LN_TAU, TOL_ALPHA, MAX_DQ_UNSCATTERED = 0.118, 2.0, 41.4
ROW_MS = 64e-3


def scat_of(lib, c, info=None, **kw):
    a = dict(alphas=c["alphas"], snr_min=c["snr_min"], flag=c["flag"], products="coherency" if c["coh"] else "stokes")
    a.update(kw)
    return post.burst_scatter(c["rows"], c["hdr"], c["cands"], c["nbin"], c["tfactor"], c["ffactor"], sc.bank_par(c["bp"]), c["shift0"], c["nshift"],
                              lib=lib, info=info, **a)


# ---- the bank ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", (sc.SMALL_BANK, sc.NF_BANK, (2, 3, 1, 0, 0.25, 1.5, 0.25, 3.0), (1, 1, 40, 39, 3.0, 2.0, 5.0, 2.0)))
def test_bank_equals_its_formula_within_one_unit(emu_lib, args):
    bank = post.scat_bank(post.scat_bank_params(*args), emu_lib)
    want = so.bank_formula(*args)
    diff = np.abs(bank["p"].astype(np.int64) - want["p"])
    print("taps that differ from numpy's: %d of %d" % (int((diff != 0).sum()), diff.size))
    assert diff.max() <= 1 and bank["p"].max() == 1 << 15 and bank["p"].min() >= 0
    exact = so.bank_sums(bank["p"])                                  # S1 and the prefix sums: exact for the library's own p
    assert bank["s1"].tobytes() == exact["s1"].tobytes() and bank["cum"].tobytes() == exact["cum"].tobytes()
    assert bank["sigma"].tobytes() == want["sigma"].tobytes() and bank["tau"].tobytes() == want["tau"].tobytes()
    assert np.allclose(bank["tail"], want["tail"], rtol=1e-12, atol=0) and (bank["p"][:, args[3]] > 0).all()
    assert bank["p"].tobytes() == sc.bank_of(*args)[0]["p"].tobytes()       # the emulator build's bank is the one the cases were built from


def test_bank_refusals(emu_lib):
    good = dict(nsig=3, ntau=4, ntap=24, lead=6, sigma0=0.75, rsig=1.5, tau0=0.5, rtau=1.5)
    for kw, text in ((dict(ntap=0), "ntap"), (dict(ntap=1025), "ntap"), (dict(lead=24), "lead"), (dict(nsig=0), "templates"), (dict(nsig=64, ntau=65), "templates"),
                     (dict(sigma0=0.2), "0.25"), (dict(tau0=0.2), "0.25"), (dict(sigma0=math.nan), "finite"), (dict(tau0=math.inf), "finite"),
                     (dict(rsig=1.0), "above 1"), (dict(rtau=0.5), "above 1"), (dict(rtau=math.nan), "finite"), (dict(rsig=1e300, nsig=3), "finite")):
        par = post.scat_bank_params(**dict(good, **kw))
        p = np.full((4096, 24), 7, np.int32)
        err = C.create_string_buffer(256)
        code = emu_lib.frbch_scat_bank(C.byref(par), p.ctypes.data, None, None, None, None, None, err, len(err))
        assert code == _lib.E_ARG and text in err.value.decode() and (p == 7).all(), (kw, err.value)
    par = post.scat_bank_params(**good)
    par.size = 60
    assert emu_lib.frbch_scat_bank(C.byref(par), None, None, None, None, None, None, None, 0) == _lib.E_ARG
    assert emu_lib.frbch_scat_bank(C.byref(post.scat_bank_params(**good)), None, None, None, None, None, None, None, 0) == 0


# ---- the stage alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.PLANES))
def test_stage_equals_the_oracle(emu_lib, name):
    n = sc.PLANES[name][0]
    (y, P), want = sc.plane(name), sc.plane_want(name)
    for fn in (emu_lib.frbch_tbank_host, emu_lib.frbch_tbank_device):
        for form in (_lib.TBANK_PLAN, _lib.TBANK_GENERIC):
            code, msg, Cc, k = sc.tbank_call(fn, y.ctypes.data, P.ctypes.data, n, sc.shape_of(name), form)
            assert code == 0 and k == 0, msg
            assert Cc.tobytes() == want.tobytes()
    assert emu_lib.frbch_tbank_kernel(n, C.byref(sc.shape_of(name)), _lib.TBANK_PLAN) == 0
    assert post.tbank(y, P, *sc.PLANES[name][5:8], lib=emu_lib).tobytes() == want.tobytes()


def test_the_stage_cases_reach_their_edges():
    """the restatement alone: what each plane is there for"""
    assert int(sc.plane_want("full_scale_2_to_61")[0, 0, 0, 0]) == 1 << 61                        # the header's bound, reached exactly
    assert int(sc.plane_want("full_scale_2_to_61")[0, 0, 0, 1]) == -(1 << 51) * 1023
    y, P = sc.plane("nshift_7_window_starts_before_bin_0")                                        # tap 0 of shift 0 lies at bin -1: absent
    assert int(sc.plane_want("nshift_7_window_starts_before_bin_0")[0, 1, 2, 0]) == sum(int(y[0, 1, m - 1]) * int(P[2, m]) for m in range(1, 6))
    y, P = sc.plane("nshift_8_lead_0_window_runs_off_the_end")                                    # the last shift: one tap left in the row
    assert int(sc.plane_want("nshift_8_lead_0_window_runs_off_the_end")[0, 0, 1, 7]) == int(y[0, 0, 15]) * int(P[1, 0])
    y, P = sc.plane("ntap_above_nbin")
    assert int(sc.plane_want("ntap_above_nbin")[0, 1, 1, 0]) == sum(int(y[0, 1, j]) * int(P[1, j + 13]) for j in range(16))
    y, P = sc.plane("ntap_1")
    assert (sc.plane_want("ntap_1")[0, :, 2, :] == y[0].astype(np.int64) * int(P[2, 0])).all()
    one, more = sc.tbank_plan(*sc.PLANES["templates_of_one_run"][:8]), sc.tbank_plan(*sc.PLANES["one_template_and_one_subband_more"][:8])
    assert (one["sw"], one["kr"], one["nkr"], one["lds"]) == (8, 999, 1, 65536) and (more["sw"], more["kr"], more["nkr"]) == (8, 500, 2)
    assert sc.tbank_plan(1, 1, 1024, 4096, 1024, 0, 0, 1024)["sw"] == 1 and sc.tbank_plan(1, 1, 1024, 4, 1024, 0, 0, 1024)["lds"] <= 65536
    assert sc.tbank_plan(1, 64, 1024, 4, 1024, 0, 0, 8)["sw"] == 8 and sc.tbank_plan(65536, 1, 1, 1, 1, 0, 0, 1) is None
    assert all(sc.tbank_plan(*t[:8])["lds"] <= 65536 for t in sc.PLANES.values())
    assert sc.tbank_plan(4, 64, 256, 512, 256, 64, 64, 128) == dict(sw=4, kr=57, nkr=9, lds=65280)        # the measured shape: (16384 - 4 x 432) // 256 = 57


def test_stage_refusals(emu_lib):
    name = "three_planes"
    (y, P), t = sc.plane(name), sc.PLANES[name]
    host = emu_lib.frbch_tbank_host
    bad_y, bad_P = y.copy(), P.copy()
    bad_y[1, 2, 3] = Y = so.Y_MAX + 1
    bad_P[2, 5] = -(so.P_MAX + 1)
    assert Y > so.Y_MAX
    for yy, PP, n, kw, form, text in (
            (bad_y, P, 3, {}, 0, "outside -2^21"), (-bad_y, P, 3, {}, 0, "outside -2^21"), (y, bad_P, 3, {}, 0, "outside -2^30"),
            (y, P, 0, {}, 0, "at least one"), (y, P, 3, dict(nsub=0), 0, "at least one"), (y, P, 3, dict(nbin=0), 0, "nbin"), (y, P, 3, dict(nbin=1025), 0, "nbin"),
            (y, P, 3, dict(ntap=0), 0, "ntap"), (y, P, 3, dict(ntap=1025), 0, "ntap"), (y, P, 3, dict(lead=12), 0, "lead"), (y, P, 3, dict(ntemp=0), 0, "templates"),
            (y, P, 3, dict(ntemp=4097), 0, "templates"), (y, P, 3, dict(nshift=0), 0, "nshift"), (y, P, 3, dict(nshift=36), 0, "nshift"),
            (y, P, 3, dict(shift0=41, nshift=1), 0, "nshift"), (y, P, 3, dict(size=28), 0, "wrong size"), (y, P, 3, {}, 2, "form"),
            (y, P, 17, dict(nsub=1024, nbin=1024, shift0=0, nshift=1), 0, "nsub * nbin exceeds 2^24"),
            (y, P, 3, dict(nsub=4096, ntemp=64, nshift=30), 0, "nshift exceeds 2^24")):
        code, msg, Cc, _k = sc.tbank_call(host, yy.ctypes.data, PP.ctypes.data, n, sc.shape_of(t, **kw), form)
        assert code == _lib.E_ARG and text in msg, (kw, form, msg)
        assert (Cc == 0x5A5A5A5A5A5A5A5A).all()
        assert emu_lib.frbch_tbank_kernel(n, C.byref(sc.shape_of(t, **kw)), form) == (_lib.E_ARG if yy is y and PP is P else 0)
    assert sc.tbank_call(host, None, P.ctypes.data, 3, sc.shape_of(t))[0] == _lib.E_ARG
    assert sc.tbank_call(host, y.ctypes.data, None, 3, sc.shape_of(t))[0] == _lib.E_ARG
    with pytest.raises(post.InputError, match="outside"):
        post.tbank(bad_y, P, 3, 5, 30, lib=emu_lib)


# ---- the composite ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_composite_equals_the_oracle(emu_lib, name):
    c, want = sc.case(name), sc.want(name)
    info = {}
    got = scat_of(emu_lib, c, info)
    assert info == dict(spectra_kernel_used=0, dynspec_kernel_used=0, kernel_used=0)
    assert sc.differing(got, want) == [] and got["q"].tobytes() == want["q"].tobytes()
    assert sc.query(emu_lib, c, c["rows"].ctypes.data) == (0, (0, 0, 0))
    # the _device twin (the emulator's device memory is host memory) writes the same bytes into outputs that held something else
    code, msg, out, k = sc.call(emu_lib.frbch_burstscat_device, c, c["rows"].ctypes.data, out=sc.outputs_of(c, fill=0xA5))
    assert code == 0 and k == (0, 0, 0), msg
    assert sc.differing(out, got) == []
    # Y and yhits are frbch_burstacf_*'s on the same arguments, y is the restatement's quantised plane, to the bit
    acf = sc.acf_of(emu_lib, c)
    assert got["Y"].tobytes() == acf["Y"].tobytes() and got["yhits"].tobytes() == acf["yhits"].tobytes()
    dyn = ao.dynspec(c["rows"], c["hdr"], c["cands"], c["nbin"], c["tfactor"], c["ffactor"], c["flag"], c["coh"])
    assert got["y"].tobytes() == ao.quantise(dyn["Y"], dyn["mask"])[0].tobytes()
    # the fit alone, from the planes
    q = np.full(want["q"].shape, 7.0)
    sub, band = np.zeros(want["sub"].shape, dtype=post.SCAT_SUB), np.zeros(want["band"].size, dtype=post.SCAT_BAND)
    err = C.create_string_buffer(256)
    arrs = [np.ascontiguousarray(want[f]) for f in ("k", "r", "nused", "nused_s", "C", "N")]
    code = emu_lib.frbch_burstscat_fit(C.byref(post.fil_desc(c["hdr"], 0)), C.byref(sc.par_of(c)), C.byref(sc.bank_par(c["bp"])), C.byref(sc.fit_par_of(c)),
                                       band.size, *[a.ctypes.data for a in arrs], q.ctypes.data, sub.ctypes.data, band.ctypes.data, err, len(err))
    assert code == 0, err.value
    assert q.tobytes() == want["q"].tobytes() and sub.tobytes() == want["sub"].tobytes() and band.tobytes() == want["band"].tobytes()
    # the quantised plane and the 0 / 1 plane through the stage alone give C and N
    bp = c["bp"]
    for pl, bank, field in ((want["y"], c["bank"]["p"], "C"), (want["mask"].astype(np.int32), c["bank"]["p"] ** 2, "N")):
        assert post.tbank(pl, bank, bp["lead"], c["shift0"], c["nshift"], lib=emu_lib).tobytes() == want[field].tobytes(), field


def test_the_composite_cases_reach_their_edges():
    """the restatement alone: what each case is there for"""
    for name in sc.CASES:
        w, c = sc.want(name), sc.case(name)
        complete = bool(w["mask"].all())
        assert complete == (name in sc.ALL_COMPLETE), name
        closed = so.energy_closed_form(c["bank"]["cum"], c["nbin"], c["bp"]["lead"], c["shift0"], c["nshift"])
        if complete:                                                 # N from the kernel on the 0 / 1 plane = the closed form
            assert (w["N"] == closed[None, None]).all(), name
        else:
            assert (w["N"] <= closed[None, None]).all() and (w["N"] < closed[None, None]).any(), name
    w = sc.want("u8_64ch_flag_dead_subband")
    assert w["nused"].tolist() == [58, 0, 58] and w["nused_s"][0, 8] == 0 and not w["q"][0, 8].any() and not w["q"][1].any()
    assert not w["sub"][1].view(np.uint8).reshape(32, -1)[:, :104].any() and w["band"]["nfit"].tolist() == [31, 0, 31]
    assert w["sub"]["q"][0, 8] == 0.0 and (w["sub"]["q"][0, :8] > 0).all()
    w = sc.want("u8_64ch_windows_leave_the_file")
    assert (w["mask"][0] == 0).any() and (w["mask"][1] == 0).any() and (w["N"][0] == 0).any()
    assert sc.case("u16_128ch_f4_coherency")["rows"].dtype == np.uint16 and sc.case("u16_128ch_f4_coherency")["hdr"]["nchans"] == 128
    assert sc.want("u8_64ch_f64_one_subband")["Y"].shape == (1, 1, 40) and sc.want("u8_64ch_f1")["Y"].shape == (2, 64, 33)
    assert sc.case("u8_64ch_f4_mixed_dms")["cands"]["dm"].tolist() == [56.7, 20.0]
    assert int(np.abs(sc.want("u8_64ch_f1")["y"]).max()) > 1 << 20


def test_closed_form_and_counted_energies_agree(emu_lib):
    """a call whose cells are all complete writes N in closed form; the same candidate beside one that is not complete has its N
    from the kernel on the 0 / 1 plane: the two are equal"""
    c = sc.case("u8_64ch_f4_mixed_dms")
    alone = scat_of(emu_lib, c)
    cands = post.burst_cands([(b["dm"], b["sample"], b["width"]) for b in (sc.B1, sc.B_END)], 16, 200)
    both = post.burst_scatter(c["rows"], c["hdr"], cands, c["nbin"], c["tfactor"], c["ffactor"], sc.bank_par(c["bp"]), c["shift0"], c["nshift"],
                              alphas=c["alphas"], snr_min=c["snr_min"], lib=emu_lib)
    closed = so.energy_closed_form(c["bank"]["cum"], c["nbin"], c["bp"]["lead"], c["shift0"], c["nshift"])
    assert (both["N"][1] < closed[None]).any()
    assert both["N"][0].tobytes() == alone["N"][0].tobytes() and (alone["N"][0] == closed[None]).all()
    assert both["C"][0].tobytes() == alone["C"][0].tobytes() and both["sub"][0].tobytes() == alone["sub"][0].tobytes()


def test_the_band_fit_shifts_and_clips():
    """the restatement alone, on a q built by hand: three subbands 100 MHz apart whose best tau steps by d_s(alpha) bins"""
    hdr = dict(nchans=3, fch1=1500.0, foff=-100.0, tsamp=1e-3)
    bp = dict(nsig=1, ntau=6, rtau=2.0 ** 0.5, lead=0)
    bank = dict(sigma=[1.0], tau=[0.5 * bp["rtau"] ** b for b in range(6)], s1=[1] * 6)
    nu_ref = 1400.0
    ds = [int(round(d)) for d in so.shifts_of(4.0, (1500.0, 1400.0, 1300.0), nu_ref, bp["rtau"])]
    assert ds == [-1, 0, 1]
    Cc, N = np.zeros((1, 3, 6, 2), np.int64), np.ones((1, 3, 6, 2), np.int64)
    for s, b in enumerate((4, 5, 5)):                              # clip(5 + d_s, 0, 5): b_ref = 5 with the lowest subband clipped
        Cc[0, s, b, 1] = 40 + s
    q, sub, band = so.fit(hdr, Cc, N, np.array([0]), np.array([0]), np.array([3]), np.ones((1, 3), np.uint32), bank, bp, 1, 1, 0, [0.0, 4.0], 5.0)
    assert sub["k"][0].tolist() == [4, 5, 5] and sub["u"][0].tolist() == [1, 1, 1] and band["nfit"][0] == 3
    assert (band["alpha"][0], band["b_ref"][0], band["u"][0]) == (4.0, 5, 1) and band["nclipped"][0] == 1 and band["bounded_hi"][0] == 0
    assert band["q"][0] == (1600.0 + 1681.0) + 1764.0


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(emu_lib):
    c = sc.case("u8_64ch_f4_mixed_dms")
    hdr, ptr = c["hdr"], c["rows"].ctypes.data
    host = emu_lib.frbch_burstscat_host

    def cand(field, value, i=0):
        cc = c["cands"].copy()
        cc[field][i] = value
        return cc

    assert sc.call(host, c, ptr)[0] == 0
    par, fp = (lambda **kw: sc.par_of(c, **kw)), (lambda **kw: sc.fit_par_of(c, **kw))
    bank = lambda **kw: sc.bank_par(dict(c["bp"], **kw))
    nan_alpha = fp()
    nan_alpha.alpha[1] = math.nan
    refused = [
        (dict(par=par(size=28)), "frbch_scat_params: wrong size"), (dict(par=par(nbin=0)), "nbin"), (dict(par=par(nbin=1025)), "nbin"),
        (dict(par=par(tfactor=0)), "tfactor"), (dict(par=par(tfactor=513)), "tfactor"), (dict(par=par(ffactor=0)), "ffactor"),
        (dict(par=par(ffactor=3)), "ffactor"), (dict(par=par(nshift=0)), "nshift"), (dict(par=par(nshift=34)), "nshift"),
        (dict(par=par(shift0=20, nshift=14)), "nshift"), (dict(bp=bank(ntap=0)), "ntap"), (dict(bp=bank(ntap=1025)), "ntap"), (dict(bp=bank(lead=24)), "lead"),
        (dict(bp=bank(nsig=0)), "templates"), (dict(bp=bank(nsig=1025, ntau=4)), "templates"), (dict(bp=bank(sigma0=0.1)), "0.25"),
        (dict(bp=bank(tau0=math.nan)), "finite"), (dict(bp=bank(rtau=1.0)), "above 1"),
        (dict(cands=np.repeat(c["cands"][:1], 2048), bp=bank(nsig=16, ntau=16)), "nshift exceeds 2^24"),
        (dict(fp=fp(size=8)), "frbch_scat_fit_params: wrong size"), (dict(fp=fp(nalpha=0)), "nalpha"), (dict(fp=fp(nalpha=33)), "nalpha"),
        (dict(fp=fp(snr_min=math.inf)), "snr_min"), (dict(fp=nan_alpha), "alpha"),
        (dict(hdr=dict(hdr, nbits=32)), "not built for float32"), (dict(hdr=dict(hdr, nifs=2), bpar=rc.burst_par(True)), "nifs = 4"), (dict(ncand=0), "candidates"),
        (dict(cands=cand("width", 0)), "width"), (dict(cands=cand("dm", math.nan)), "DM"), (dict(bpar=rc.burst_par(size=4)), "frbch_burst_params: wrong size"),
    ]
    for kw, text in refused:
        out = sc.outputs(2, 16, 33, 12, 33, 64, fill=0xA5)
        code, msg, out, _k = sc.call(host, c, ptr, out=out, **kw)
        assert code == _lib.E_ARG and text in msg, (kw, msg)
        assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), kw
        code2 = sc.call(emu_lib.frbch_burstscat_device, c, ptr, out=out, **kw)[0]
        assert code2 == _lib.E_ARG and all((a.view(np.uint8) == 0xA5).all() for a in out.values()), kw
    assert sc.query(emu_lib, c, ptr, par=par(nbin=1025))[0] == _lib.E_ARG and sc.query(emu_lib, c, None)[0] == _lib.E_ARG
    assert sc.query(emu_lib, c, ptr, bp=bank(lead=24))[0] == _lib.E_ARG and sc.call(host, c, None)[0] == _lib.E_ARG
    with pytest.raises(post.InputError, match="float32"):
        post.burst_scatter(c["rows"].astype(np.float32), dict(hdr, nbits=32), c["cands"], lib=emu_lib)
    with pytest.raises(post.InputError, match="ffactor"):
        post.burst_scatter(c["rows"], hdr, c["cands"], ffactor=3, lib=emu_lib)


# ---- the known answers --------------------------------------------------------------------------------------------------------
def test_a_noise_free_plane_returns_its_template_and_arrival(emu_lib):
    """37 times template k with its centre on bin t0, truncated by the window, through the stage and the fit: exactly (k, t0), for
    every template of the 6 x 10 bank at three arrivals (the first and the last trial bin among them)"""
    bank, bp = sc.bank_of(*sc.NF_BANK)
    y = np.concatenate([sc.noise_free_plane(k, t0) for k in range(60) for t0 in sc.NF_ARRIVALS], axis=1)       # one plane of 180 rows
    Cc = post.tbank(y, bank["p"], bp["lead"], sc.NF_SHIFT0, sc.NF_NSHIFT, lib=emu_lib)
    assert Cc.tobytes() == so.tbank(y, bank["p"], bp["lead"], sc.NF_SHIFT0, sc.NF_NSHIFT).tobytes()
    N = np.broadcast_to(so.energy_closed_form(bank["cum"], sc.NF_NBIN, bp["lead"], sc.NF_SHIFT0, sc.NF_NSHIFT), Cc.shape)
    hdr = dict(rc.make_hdr(180), nbits=8, nifs=1)
    q, sub, _band = so.fit(hdr, Cc, np.ascontiguousarray(N), np.array([0]), np.array([0]), np.array([180]), np.ones((1, 180), np.uint32), bank, bp, 1, 1,
                           sc.NF_SHIFT0, [0.0], 5.0)
    want = [(k, t0) for k in range(60) for t0 in sc.NF_ARRIVALS]
    assert [(int(r["k"]), int(r["arrival"])) for r in sub[0]] == want
    got_sub = np.zeros((1, 180), dtype=post.SCAT_SUB)
    err = C.create_string_buffer(256)
    arrs = [np.array([0], np.int32), np.array([0], np.uint32), np.array([180], np.uint32), np.ones((1, 180), np.uint32), Cc, np.ascontiguousarray(N)]
    code = emu_lib.frbch_burstscat_fit(C.byref(post.fil_desc(hdr, 0)), C.byref(post.scat_params(sc.NF_NBIN, 1, 1, sc.NF_SHIFT0, sc.NF_NSHIFT)),
                                       C.byref(sc.bank_par(bp)), C.byref(post.scat_fit_params([0.0], 5.0)), 1, *[a.ctypes.data for a in arrs], None,
                                       got_sub.ctypes.data, None, err, len(err))
    assert code == 0, err.value
    assert got_sub.tobytes() == sub.tobytes()


def test_the_oracle_returns_the_injected_scattering():
    """before anything relies on it: the restatement alone over the twelve seeds (the module's docstring says where the
    tolerances come from)"""
    cover_tau = cover_alpha = 0
    for seed in sc.KNOWN_SEEDS:
        w = sc.known_oracle(seed)
        b, s = w["band"][0], w["sub"][0]
        tau_rows = b["tau_ref_ms"] / ROW_MS
        print("seed %2d: tau_ref %.3f rows (%.3f .. %.3f), alpha %.1f (%.1f .. %.1f), sigma %.2f rows, smallest S/N %.1f" % (
            seed, tau_rows, b["tau_ref_lo"] / ROW_MS, b["tau_ref_hi"] / ROW_MS, b["alpha"], b["alpha_lo"], b["alpha_hi"], b["sigma"], s["snr"].min()))
        assert b["nfit"] == 8 and (s["snr"] >= sc.SNR_MIN).all() and b["nclipped"] == 0 and b["bounded_lo"] == 1 and b["bounded_hi"] == 1
        assert abs(math.log(tau_rows / sc.KNOWN_TAU_REF)) <= TOL_LN_TAU and abs(b["alpha"] - sc.KNOWN_ALPHA) <= TOL_ALPHA
        assert abs(b["sigma"] - 2.0) < 1e-9 and abs(b["arrival"] - 128.0) <= 1.0
        cover_tau += b["tau_ref_lo"] <= sc.KNOWN_TAU_REF * ROW_MS <= b["tau_ref_hi"]
        cover_alpha += b["alpha_lo"] <= sc.KNOWN_ALPHA <= b["alpha_hi"]
    print("the intervals hold the truth: tau_ref %d of 12, alpha %d of 12" % (cover_tau, cover_alpha))


def test_the_oracle_gives_no_confident_tau_to_an_unscattered_burst():
    for seed in sc.KNOWN_SEEDS:
        w = sc.known_oracle(seed, False)
        b, s = w["band"][0], w["sub"][0]
        print("seed %2d: tau_ref %.3f rows, bounded_lo %d; subbands bounded_lo %s, dq_unscattered up to %.1f" % (
            seed, b["tau_ref_ms"] / ROW_MS, b["bounded_lo"], s["bounded_lo"].tolist(), s["dq_unscattered"].max()))
        assert b["nfit"] == 8 and b["bounded_lo"] == 0 and b["b_ref"] == 0
        assert ((s["bounded_lo"] == 0) | (s["dq_unscattered"] <= MAX_DQ_UNSCATTERED)).all()


@pytest.mark.parametrize("scattered", (True, False))
def test_known_answer(emu_lib, scattered):
    check_known_answer(emu_lib, scattered)


def check_known_answer(lib, scattered, info=None, seed=3):
    want = sc.known_oracle(seed, scattered)
    got = sc.known_call(lib, seed, scattered, info)
    assert sc.differing(got, want) == [] and got["q"].tobytes() == want["q"].tobytes()
    b, s = got["band"][0], got["sub"][0]
    if scattered:
        assert abs(math.log(b["tau_ref_ms"] / ROW_MS / sc.KNOWN_TAU_REF)) <= TOL_LN_TAU and abs(b["alpha"] - sc.KNOWN_ALPHA) <= TOL_ALPHA
    else:
        assert b["bounded_lo"] == 0 and ((s["bounded_lo"] == 0) | (s["dq_unscattered"] <= MAX_DQ_UNSCATTERED)).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_scatter_end_to_end(emu_lib, tmp_path, capsys, monkeypatch):
    from tests.test_fold_predictor import write_fil
    hdr, rows = sc.known_hdr(), sc.known_rows(3)
    fil = str(tmp_path / "burst.fil")
    write_fil(fil, rows, hdr, 1)
    base = fil.replace(".fil", "")
    before = set(os.listdir(tmp_path))
    g, (_bank, bp) = sc.KNOWN_GRID, sc.bank_of(*sc.KNOWN_BANK)
    info = {}
    files, got = post.burstscat_fil(fil, [(sc.KNOWN_DM, sc.KNOWN_SAMPLE, 8)], bank=sc.bank_par(bp), alphas=sc.KNOWN_ALPHAS, snr_min=sc.SNR_MIN, off_gap=400,
                                    off_len=400, lib=emu_lib, info=info, **g)
    assert files == [base + "_scat.npz", base + "_scat.txt", base + "_scat.png"] and all(os.path.getsize(f) > 0 for f in files)
    assert set(os.listdir(tmp_path)) - before == {os.path.basename(f) for f in files} and info["kernel_used"] == 0
    want = sc.known_oracle(3)
    back = np.load(files[0])
    for f in sc.FIELDS + ("q",):
        assert back[f].tobytes() == np.ascontiguousarray(want[f]).tobytes() == np.ascontiguousarray(got[f]).tobytes(), f
    lines = open(files[1]).read().splitlines()
    assert len(lines) == 9 and lines[0].startswith("burst0") and ("alpha %6.3f" % got["band"]["alpha"][0]) in lines[0]
    assert open(files[2], "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    monkeypatch.setattr(_lib, "load", lambda path=None: emu_lib)
    for f in files:
        os.remove(f)
    assert post.main(["scatter", fil, "--dm", repr(sc.KNOWN_DM), "--sample", str(sc.KNOWN_SAMPLE), "--width", "8", "--nbin", "256", "--ffactor", "8",
                      "--sigma0", "1.0", "--nsig", "4", "--rsig", repr(bp["rsig"]), "--tau0", "0.5", "--ntau", "48", "--rtau", repr(bp["rtau"]), "--ntap", "128",
                      "--lead", "24", "--shift0", "96", "--nshift", "64", "--alpha"] + [repr(a) for a in sc.KNOWN_ALPHAS] +
                     ["--snr-min", "5", "--off-gap", "400", "--off-len", "400"]) == 0
    assert "wrote " + files[0] in capsys.readouterr().out and np.load(files[0])["band"].tobytes() == got["band"].tobytes()


# ---- failing device-layer calls -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("u8_64ch_f4_mixed_dms", "u8_64ch_flag_dead_subband"))
def test_a_failing_device_call_returns_the_error_and_leaves_nothing_behind(emu_lib, name):
    """every fallible device-layer call of frbch_burstscat_host fails once (n = 1, 2, ... until the call succeeds; the second case
    also forms N on the device): an error with a message comes back, the outputs are untouched, the blocks and streams alive
    afterwards are those alive before, and a plain call right afterwards writes the expected bytes"""
    emu_lib.frbch_test_emu_fail_at.argtypes, emu_lib.frbch_test_emu_fail_at.restype = [C.c_long], None
    emu_lib.frbch_test_emu_live.argtypes, emu_lib.frbch_test_emu_live.restype = [], C.c_uint64
    c, want = sc.case(name), sc.want(name)
    ptr = c["rows"].ctypes.data
    rows0 = c["rows"].tobytes()
    codes = []
    for n in range(1, 200):
        out = sc.outputs_of(c, fill=0xA5)
        before = emu_lib.frbch_test_emu_live()
        emu_lib.frbch_test_emu_fail_at(n)
        try:
            code, msg, out, _k = sc.call(emu_lib.frbch_burstscat_host, c, ptr, out=out)
        finally:
            emu_lib.frbch_test_emu_fail_at(0)
        assert emu_lib.frbch_test_emu_live() == before, n
        if code == 0:
            assert sc.differing(out, want) == []
            break
        codes.append(code)
        assert code in (_lib.E_DEVICE, _lib.E_NOMEM) and msg, (n, code, msg)
        assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), n
    again = sc.call(emu_lib.frbch_burstscat_host, c, ptr)
    assert again[0] == 0 and sc.differing(again[2], want) == []
    assert 25 < len(codes) < 199 and c["rows"].tobytes() == rows0
