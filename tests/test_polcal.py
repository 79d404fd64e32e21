"""CPU tests of the polarisation calibration (frbch_rmdelay_*, frbch_burst_polcal_*, frbch_polprof_cal_*) through the TEST-ONLY
emulator build, which runs the generic kernel: the transform, the peaks and the profile with a delay against
tests/polcal_oracle.py byte for byte, the identity with frbch_rmsynth_*, every refusal with its message, the known answers (the
restatement alone first, then the library), and `post polcal` / `--polcal` end to end."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import polcal_cases as pc
from tests import polcal_oracle as pco
from tests import polprof_cases as ppc
from tests import rm_cases as rc
from tests import rm_oracle as ro


# ---- the transform ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.SHAPES))
def test_transform_equals_the_restatement(emu_lib, name):
    nchan, ncand, _nphi, _pl, _dp, _nt, _tl, _dt, masked = pc.SHAPES[name]
    hdr, q, u, used = rc.spectra(nchan, ncand, 0, masked)
    F, k = pc.host_rmd(emu_lib, hdr, q, u, used, **pc.grid_of(name))
    assert k == (pc.GENERIC, 1)                                   # the emulator build has the generic kernel only
    assert F.tobytes() == pc.want_transform(name).tobytes()


def test_one_trial_at_zero_delay_is_rm_synthesis(emu_lib):
    for nchan, ncand, nphi, phi_lo, dphi, masked in ((64, 3, 63, -3100.0, 100.0, (3, 40)), (96, 3, 257, -3000.0, 23.5, ())):
        hdr, q, u, used = rc.spectra(nchan, ncand, 0, masked)
        want = rc.want_transform(nchan, ncand, nphi, phi_lo, dphi, 0, masked)
        F, _k = pc.host_rmd(emu_lib, hdr, q, u, used, nphi, phi_lo, dphi, 1, 0.0, 1.0e-3)
        assert F[:, 0].tobytes() == want.tobytes()
        plain = post.rm_synthesis(q, u, used, hdr, nphi, phi_lo, dphi, lib=emu_lib)
        assert np.ascontiguousarray(plain).view(np.float32).tobytes() == F[:, 0].tobytes()
        moved, _k = pc.host_rmd(emu_lib, hdr, q, u, used, nphi, phi_lo, dphi, 1, 2.5e-3, 1.0e-3)
        assert moved.tobytes() != F.tobytes()


def test_a_dead_candidate_and_a_grid_across_zero(emu_lib):
    hdr, q, u, used = rc.spectra(96, 3, 1)
    q2, u2, used2 = q.copy(), u.copy(), used.copy()
    q2[1], u2[1] = 0.0, 0.0
    used2[2] = 0                                                   # no used channel
    grid = dict(nphi=70, phi_lo=-3000.0, dphi=90.0, ntau=5, tau_lo=-2.0e-3, dtau=1.0e-3)       # tau = -2 .. +2 ns
    F, _k = pc.host_rmd(emu_lib, hdr, q2, u2, used2, **grid)
    assert F[0].any() and not F[1].any() and not F[2].any()
    assert F.tobytes() == pco.transform(q2, u2, used2, hdr, **grid)[0].tobytes()
    zero = rc.want_transform(96, 3, 70, -3000.0, 90.0, 1)         # trial 2 is tau = 0: the plain transform
    assert F[0, 2].tobytes() == zero[0].tobytes()


def test_nothing_wraps_at_16384_full_scale_channels(emu_lib):
    hdr, q, u, used, grid, want, largest, re_max = pc.full_scale_case()
    print("largest sum of |terms| = 2^%.3f, largest |Re| = 2^%.3f" % (np.log2(float(largest)), np.log2(float(re_max))))
    # 16384 terms of 2^23 2^22 at a phase near 0: 2^59 within the header's bound of 2^60, far from 2^63
    assert (1 << 59) - (1 << 50) < largest <= 1 << 60 and re_max > 1 << 58
    F, _k = pc.host_rmd(emu_lib, hdr, q, u, used, **grid)
    assert F.tobytes() == want.tobytes()


# ---- refusals --------------------------------------------------------------------------------------------------------
def _rmd_call(lib, hdr, ncand=1, size=None, **grid):
    g = dict(nphi=257, phi_lo=-12800.0, dphi=100.0, ntau=3, tau_lo=-1.0e-3, dtau=1.0e-3)
    g.update(grid)
    par = post.rmd_params(**g)
    if size is not None:
        par.size = size
    code, _ = pc.raw_call(lib, "frbch_rmdelay_kernel", hdr, ncand, par)
    if code >= 0:
        return code, ""
    code2, msg = pc.raw_call(lib, "frbch_rmdelay_host", hdr, ncand, par)
    code3, msg3 = pc.raw_call(lib, "frbch_rmdelay_peaks", hdr, ncand, par)
    assert code2 == code3 == code and msg == msg3
    return code, msg


def test_refusals(emu_lib):
    hdr = rc.make_hdr(64)
    assert _rmd_call(emu_lib, hdr)[0] == 0
    assert _rmd_call(emu_lib, hdr, ntau=4096, nphi=1 << 14, dphi=1.0, dtau=1.0e-3, tau_lo=-2.0)[0] == 0         # 2^26 outputs exactly
    for kw, text in ((dict(size=32), "frbch_rmd_params: wrong size"),
                     # every refusal of rm_check
                     (dict(nphi=0), "nphi must be 1..2^20"), (dict(nphi=(1 << 20) + 1), "nphi must be 1..2^20"),
                     (dict(ncand=0), "1..4096 candidates"), (dict(ncand=4097), "1..4096 candidates"),
                     (dict(ncand=65, nphi=1 << 20, dphi=1.0, ntau=1), "ncand * nphi exceeds 2^26"),
                     (dict(dphi=0.0), "dphi must be positive and finite"), (dict(dphi=-1.0), "dphi must be positive and finite"),
                     (dict(dphi=np.inf), "dphi must be positive and finite"), (dict(dphi=np.nan), "dphi must be positive and finite"),
                     (dict(phi_lo=-1.0001e7), "|phi| above 1e7 rad m^-2"), (dict(phi_lo=np.nan), "|phi| above 1e7 rad m^-2"),
                     (dict(phi_lo=9.99e6), "|phi| above 1e7 rad m^-2"),
                     # the tau axis
                     (dict(ntau=0), "ntau must be 1..4096"), (dict(ntau=4097), "ntau must be 1..4096"),
                     (dict(ntau=4096, nphi=(1 << 14) + 1, dphi=1.0, tau_lo=-2.0), "ncand * ntau * nphi exceeds 2^26"),
                     (dict(ncand=2, ntau=4096, nphi=1 << 14, dphi=1.0, tau_lo=-2.0), "ncand * ntau * nphi exceeds 2^26"),
                     (dict(dtau=0.0), "dtau must be positive and finite"), (dict(dtau=-1.0e-3), "dtau must be positive and finite"),
                     (dict(dtau=np.inf), "dtau must be positive and finite"), (dict(dtau=np.nan), "dtau must be positive and finite"),
                     (dict(tau_lo=-100.001), "|tau| above 100 microseconds"), (dict(tau_lo=np.nan), "|tau| above 100 microseconds"),
                     (dict(tau_lo=99.0, ntau=11, dtau=0.1), "|tau| above 100 microseconds")):
        code, msg = _rmd_call(emu_lib, hdr, **kw)
        assert code == _lib.E_ARG and msg == text, (kw, msg)
    assert _rmd_call(emu_lib, hdr, tau_lo=99.0, ntau=10, dtau=0.1)[0] == 0
    code, msg = _rmd_call(emu_lib, dict(rc.make_hdr(16384, bw=256.0), nchans=16385))
    assert code == _lib.E_ARG and msg == "more than 16384 channels"
    code, msg = _rmd_call(emu_lib, dict(hdr, foff=-30.0))
    assert code == _lib.E_ARG and msg == "a channel frequency that is not positive"
    # a q that is not finite in a used channel; null arguments
    q = np.ones((1, 64), np.float32)
    q[0, 17] = np.nan
    par = post.rmd_params(257, -12800.0, 100.0, 3, -1.0e-3, 1.0e-3)
    code, msg = pc.raw_call(emu_lib, "frbch_rmdelay_host", hdr, 1, par, q=q, F=np.zeros((1, 3, 257, 2), np.float32))
    assert code == _lib.E_ARG and msg == "candidate 0: q or u of a used channel is not finite"
    used = np.ones((1, 64), np.uint8)
    used[0, 17] = 0
    assert pc.raw_call(emu_lib, "frbch_rmdelay_host", hdr, 1, par, q=q, used=used, F=np.zeros((1, 3, 257, 2), np.float32))[0] == 0
    err = C.create_string_buffer(256)
    assert emu_lib.frbch_rmdelay_host(C.byref(post.fil_desc(hdr)), None, q.ctypes.data, used.ctypes.data, 1, C.byref(par), 0, q.ctypes.data, None,
                                      err, len(err)) == _lib.E_ARG and err.value == b"null argument"
    assert emu_lib.frbch_rmdelay_kernel(C.byref(post.fil_desc(hdr)), None, 1, C.byref(par), None) == _lib.E_ARG
    assert emu_lib.frbch_rmdelay_kernel(C.byref(post.fil_desc(hdr)), q.ctypes.data, 1, None, None) == _lib.E_ARG
    # the composite: what the burst spectra and the grid refuse, and files of fewer than four products
    bh, rows, cands, _coh = rc.case("u8_64ch")
    with pytest.raises(post.InputError, match="ntau must be 1..4096"):
        post.polcal(rows, bh, cands, 65, -3200.0, 100.0, 0, 0.0, 1.0e-3, lib=emu_lib)
    with pytest.raises(post.InputError, match="nifs = 4"):
        post.polcal(np.ascontiguousarray(rows[:, :2]), dict(bh, nifs=2), cands, 65, -3200.0, 100.0, 3, 0.0, 1.0e-3, lib=emu_lib)
    # the profile: a tau that is not finite or too large
    c = ppc.case("u8_64ch_1x1")
    for bad in (np.nan, 100.5, -np.inf):
        with pytest.raises(post.InputError, match="a tau that is not finite or above 100 microseconds in size"):
            post.pol_profile(c["rows"], dict(c["hdr"], nifs=4), c["cands"], c["rm"], c["nbin"], c["tfactor"], c["ref"], lib=emu_lib, tau=bad)


# ---- peaks -----------------------------------------------------------------------------------------------------------
def test_peaks_equal_the_restatement(emu_lib):
    hdr, q, u, used = rc.spectra(96, 3, 0, (7,))
    grid = dict(nphi=41, phi_lo=600.0 - 1800.0, dphi=90.0, ntau=9, tau_lo=-4.0e-3, dtau=1.0e-3)
    F, _k = pc.host_rmd(emu_lib, hdr, q, u, used, **grid)
    rng = np.random.default_rng(3)
    nq, nu = (rng.uniform(0.2, 0.6, size=q.shape).astype(np.float32) for _ in range(2))
    nq[1], nu[1] = 0.0, 0.0                                        # sigma_f = 0: candidate 1 stays out of the combined record
    want = pco.peaks(F, used, nq, nu, hdr, **grid)
    got = post.rm_delay_peaks(F.view(np.complex64)[..., 0], used, nq, nu, hdr, lib=emu_lib, **grid)
    assert got.shape == (4,) and pc.same_results(got, want)
    assert got["nused"].tolist() == [95, 95, 94, 2] and got["snr"][1] == 0.0 and got["tau_err"][1] == 0.0 and got["sigma_f"][3] == 1.0
    assert (got["nridge"][:3] >= 2).all() and (got["ridge_slope"][:3] != 0.0).all() and got["psi"][3] == 0.0
    # no noise at all: nothing enters the combined record, which is all zeros
    got = post.rm_delay_peaks(F.view(np.complex64)[..., 0], used, None, None, hdr, lib=emu_lib, **grid)
    assert pc.same_results(got, pco.peaks(F, used, None, None, hdr, **grid)) and got[3].tobytes() == bytes(post.RMD_RESULT.itemsize)


def test_a_maximum_on_an_edge_is_not_fitted(emu_lib):
    hdr = rc.make_hdr(64)
    used = np.ones((1, 64), np.uint8)
    grid = dict(nphi=5, phi_lo=-20.0, dphi=10.0, ntau=4, tau_lo=0.0, dtau=1.0e-3)
    for (m, k), (ft, fr) in (((0, 2), (0, 1)), ((3, 2), (0, 1)), ((1, 0), (1, 0)), ((2, 4), (1, 0)), ((0, 0), (0, 0)), ((3, 4), (0, 0)),
                             ((1, 2), (1, 1))):
        F = np.full((1, 4, 5, 2), 0.1, np.float32)
        F[0, m, k] = (3.0, -4.0)
        r = post.rm_delay_peaks(F.view(np.complex64)[..., 0], used, None, None, hdr, lib=emu_lib, **grid)[0]
        assert (int(r["mpeak"]), int(r["kpeak"]), int(r["fitted_tau"]), int(r["fitted_rm"])) == (m, k, ft, fr)
        assert r["peak"] == 5.0 and r["tau"] == m * 1.0e-3 and r["rm"] == -20.0 + 10.0 * k
        assert r["nridge"] == 1 and r["ridge_slope"] == 0.0 and abs(r["psi"] - np.arctan2(-4.0, 3.0)) < 1e-12
    flat = np.ones((1, 4, 5, 2), np.float32)                       # den = 0 everywhere: the first trial, not fitted
    r = post.rm_delay_peaks(flat.view(np.complex64)[..., 0], used, None, None, hdr, lib=emu_lib, **grid)[0]
    assert (r["mpeak"], r["kpeak"], r["fitted_tau"], r["fitted_rm"], r["nridge"]) == (0, 0, 0, 0, 4) and r["ridge_slope"] == 0.0


# ---- the composite ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u8_64ch_3cand", "u16_64ch_coherency", "u8_96ch"])
def test_composite_equals_the_restatement(emu_lib, name):
    hdr, rows, cands, coh = rc.case(name)
    grid = dict(nphi=65, phi_lo=-3200.0, dphi=100.0, ntau=5, tau_lo=-2.0e-3, dtau=1.0e-3)
    flag = np.zeros(hdr["nchans"], np.uint8)
    flag[[2, 33]] = 1
    want = pco.burst_polcal(rows, hdr, cands, flag=flag, coherency=coh, **grid)
    info = {}
    got = post.polcal(rows, dict(hdr, nifs=4), cands, flag=flag, products="coherency" if coh else "stokes", lib=emu_lib, info=info, **grid)
    assert (info["spectra_kernel_used"], info["kernel_used"], info["split"]) == (0, 0, 1)
    for f in ("spec", "noise", "used"):
        assert got[f].tobytes() == want[f].tobytes(), f
    assert np.ascontiguousarray(got["F"]).view(np.float32).tobytes() == want["F"].tobytes()
    assert got["results"].shape == (cands.size + 1,) and pc.same_results(got["results"], want["results"])
    assert not got["used"][:, [2, 33]].any()


# ---- the profile -----------------------------------------------------------------------------------------------------
def _cal_call(lib, twin, c, rows_ptr, tau):
    """frbch_polprof_cal_host / _device with the arguments of a case of tests/polprof_cases.py -> (code, message, outputs, kernels)"""
    fn = getattr(lib, "frbch_polprof_cal_" + twin)
    hdr, n = c["hdr"], c["cands"].size
    out = ppc.outputs(n, max(1, min(c["nbin"], 1024)), hdr["nchans"])
    k = (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    code = fn(C.byref(post.fil_desc(dict(hdr, nifs=4))), rows_ptr, c["rows"].shape[0], C.byref(rc.burst_par(c["coh"])), c["cands"].ctypes.data, n,
              c["rm"].ctypes.data, tau.ctypes.data if tau is not None else None, c["gain"].ctypes.data if c["gain"] is not None else None,
              c["flag"].ctypes.data if c["flag"] is not None else None, C.byref(ppc.par_of(c)), 0, out["acc"].ctypes.data,
              out["hits"].ctypes.data, out["bins"].ctypes.data, out["results"].ctypes.data, out["used"].ctypes.data, k, err, len(err))
    return code, err.value.decode(), out, (k[0], k[1])


@pytest.mark.parametrize("name", sorted(ppc.CASES))
def test_profile_without_a_delay_is_the_existing_call(emu_lib, name):
    c = ppc.case(name)
    code, msg, old, k_old = ppc.call(emu_lib.frbch_polprof_host, c, c["rows"].ctypes.data)
    assert code == 0, msg
    code, msg, new, k_new = _cal_call(emu_lib, "host", c, c["rows"].ctypes.data, None)
    assert code == 0, msg
    assert k_new == k_old and all(new[f].tobytes() == old[f].tobytes() for f in old)
    assert ppc.same(new, ppc.want(name))


@pytest.mark.parametrize("name", ["u8_64ch_33x3", "u8_96ch_ascending", "u16_64ch_coherency", "u8_64ch_flag_gain", "u8_64ch_256x1"])
def test_profile_with_a_delay_equals_the_restatement(emu_lib, name):
    c = ppc.case(name)
    tau = np.array([2.5e-3, -40.0, 0.0][:c["cands"].size] + [1.0e-3] * max(0, c["cands"].size - 3))
    want = pco.profile(c["rows"], c["hdr"], c["cands"], c["rm"], tau, c["nbin"], c["tfactor"], c["ref"], c["gain"], c["flag"], c["coh"])
    code, msg, got, _k = _cal_call(emu_lib, "host", c, c["rows"].ctypes.data, tau)
    assert code == 0, msg
    assert ppc.same(got, want)
    assert got["acc"].tobytes() != ppc.want(name)["acc"].tobytes()           # the delay does something
    zero = pco.profile(c["rows"], c["hdr"], c["cands"], c["rm"], np.zeros(c["cands"].size), c["nbin"], c["tfactor"], c["ref"], c["gain"],
                       c["flag"], c["coh"])
    assert ppc.same(zero, ppc.want(name))                                     # tau = 0 in the restatement: the plain profile


# ---- the known answers -----------------------------------------------------------------------------------------------
def test_the_restatement_recovers_the_injected_delay():
    """(a), before any library is involved: over twelve noise seeds the restatement's peak lies at the trial the plain fp64
    evaluation of the same spectra finds, and its parabola within 2 tau_err of the injected 2.5 ns"""
    worst = 0.0
    for seed in range(12):
        k = pc.known_pulse_oracle(seed)
        r = k["results"][0]
        m64 = int(np.argmax(np.abs(k["F64"][0, :, 0]) ** 2))
        dev = abs(float(r["tau"]) * 1e3 - pc.KNOWN_TAU_NS) / (2.0 * float(r["tau_err"]) * 1e3)
        print("seed %d: tau %.4f +- %.4f ns, trial %d (fp64 %d), S/N %.1f, |dev| / (2 tau_err) = %.2f" % (seed, r["tau"] * 1e3, r["tau_err"] * 1e3,
                                                                                                      r["mpeak"], m64, r["snr"], dev))
        assert int(r["mpeak"]) == m64 == 42 and int(r["fitted_tau"]) == 1 and r["snr"] > 50
        assert dev <= 1.0
        worst = max(worst, dev)
    assert worst > 0.0


def test_the_restatement_shows_the_bias_and_its_cure():
    """(b), before any library is involved: the target's RM without the calibrator's delay misses the injected one by at least
    5 rm_err (it comes out near 245 for 350), with it it lies within the tolerance of rm_cases.rm_tolerance; and the ridge of a
    calibrator pulse runs at the analytic slope within the tolerance of polcal_cases.ridge_tolerance"""
    k = known_target_oracle()
    miss = abs(k["plain_rm"] - pc.KNOWN_TARGET_RM)
    print("calibrator: tau %.4f +- %.4f ns;  target: RM %.3f +- %.3f without it, %.3f +- %.3f with it (injected %.1f, tolerance %.3e + dphi / 2 = %.3f)"
          % (k["tau"] * 1e3, k["tau_err"] * 1e3, k["plain_rm"], k["plain_err"], k["rm"], k["rm_err"], pc.KNOWN_TARGET_RM, k["tol"], 0.5 * k["dphi"]))
    assert abs(k["tau"] * 1e3 - pc.KNOWN_TAU_NS) <= 2.0 * k["tau_err"] * 1e3
    assert miss >= 5.0 * k["plain_err"] and miss > 50.0
    assert abs(k["rm"] - k["fit64"]) <= k["tol"] and abs(k["rm"] - pc.KNOWN_TARGET_RM) <= 0.5 * k["dphi"] + k["tol"]
    s = known_ridge_oracle()
    print("ridge: %.1f rad/m2/us over %d rows, analytic %.1f, tolerance %.1f" % (s["slope"], s["nridge"], s["analytic"], s["tol"]))
    assert s["nridge"] >= 8 and abs(s["slope"] - s["analytic"]) <= s["tol"] < 0.05 * s["analytic"]
    assert 40.0 < s["analytic"] * 1e-3 < 45.0                      # about +43 rad m^-2 per nanosecond


@functools.lru_cache(maxsize=None)
def known_target_oracle():
    hdr, rows, ccal, ctgt = pc.known_target_case()
    gcal = dict(nphi=1, phi_lo=pc.KNOWN_CAL_RM, dphi=1.0, **pc.TAU_GRID)
    cal = pco.burst_polcal(rows, hdr, ccal, **gcal)
    comb = cal["results"][-1]
    nphi, phi_lo, dphi = post.rm_grid(hdr)
    plain = ro.burst_rm(rows, hdr, ctgt, nphi, phi_lo, dphi)
    tau = float(comb["tau"])
    corr = pco.burst_polcal(rows, hdr, ctgt, nphi, phi_lo, dphi, 1, tau, post.POLCAL_DTAU_ONE)
    F = np.ascontiguousarray(corr["F"][:, 0])
    res = ro.peaks(F, corr["used"], corr["noise"][:, 1], corr["noise"][:, 2], hdr, nphi, phi_lo, dphi)
    F64 = pco.transform_fp64(corr["spec"][:, 1], corr["spec"][:, 2], corr["used"], hdr, nphi, phi_lo, dphi, 1, tau, post.POLCAL_DTAU_ONE)[:, 0]
    Fint = F[..., 0].astype(np.float64) + 1j * F[..., 1].astype(np.float64)
    delta = float(np.abs(Fint[0] - F64[0]).max() / np.abs(F64[0]).max())
    P = F64[0].real * F64[0].real + F64[0].imag * F64[0].imag
    k0 = int(np.argmax(P))
    return dict(cal=cal, tau=tau, tau_err=float(comb["tau_err"]), plain=plain, plain_rm=float(plain["results"]["rm"][0]),
                plain_err=float(plain["results"]["rm_err"][0]), corr=corr, F=F, res=res, rm=float(res["rm"][0]), rm_err=float(res["rm_err"][0]),
                fit64=ro.parabola(P, k0, phi_lo, dphi)[0], tol=rc.rm_tolerance(P, k0, dphi, 2.0 * delta), grid=(nphi, phi_lo, dphi), dphi=dphi,
                gcal=gcal)


@functools.lru_cache(maxsize=None)
def known_ridge_oracle():
    hdr, rows, cands = pc.known_pulse(0)
    r = pco.burst_polcal(rows, hdr, cands, **pc.RIDGE_GRID)
    F64 = pco.transform_fp64(r["spec"][:, 1], r["spec"][:, 2], r["used"], hdr, **pc.RIDGE_GRID)
    P = np.abs(F64[0]) ** 2
    return dict(r, slope=float(r["results"]["ridge_slope"][0]), nridge=int(r["results"]["nridge"][0]),
                analytic=pc.analytic_ridge_slope(hdr, r["used"][0]), tol=pc.ridge_tolerance(P, pc.RIDGE_GRID))


def test_known_delay_through_the_library(emu_lib):
    """(a) through frbch_burst_polcal_host: the restatement's bits, hence its trial and its delay, for every seed"""
    for seed in range(12):
        hdr, rows, cands = pc.known_pulse(seed)
        k = pc.known_pulse_oracle(seed)
        got = post.polcal(rows, hdr, cands, lib=emu_lib, **k["grid"])
        assert np.ascontiguousarray(got["F"]).view(np.float32).tobytes() == k["F"].tobytes()
        assert pc.same_results(got["results"], k["results"])
        r = got["results"][0]
        assert int(r["mpeak"]) == int(np.argmax(np.abs(k["F64"][0, :, 0]) ** 2))
        assert abs(float(r["tau"]) * 1e3 - pc.KNOWN_TAU_NS) <= 2.0 * float(r["tau_err"]) * 1e3
    s = known_ridge_oracle()
    hdr, rows, cands = pc.known_pulse(0)
    got = post.polcal(rows, hdr, cands, lib=emu_lib, **pc.RIDGE_GRID)
    assert pc.same_results(got["results"], s["results"])
    assert abs(float(got["results"]["ridge_slope"][0]) - s["analytic"]) <= s["tol"]


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_polcal_then_rmsynth_and_polprof_end_to_end(emu_lib, tmp_path, capsys, monkeypatch):
    """(b) through the commands: `post polcal` on the calibrator's pulses, then `post rmsynth` on the target without and with
    --polcal; the files of `post polcal` against the restatement"""
    hdr, rows, ccal, ctgt = pc.known_target_case()
    k = known_target_oracle()
    fil = pc.write_fil(str(tmp_path / "scan.fil"), hdr, rows)
    base = fil.replace(".fil", "")
    monkeypatch.setattr(_lib, "load", lambda path=None: emu_lib)
    args = ["polcal", fil, "--rm-known", str(pc.KNOWN_CAL_RM), "--tau-half", "8", "--dtau", "0.25", "--off-gap", "32", "--off-len", "300",
            "--width", str(pc.KNOWN_WIDTH)]
    for c in ccal:
        args += ["--dm", str(float(c["dm"])), "--sample", str(int(c["sample"]))]
    assert post.main(args) == 0
    out = capsys.readouterr().out
    files = [base + "_polcal.npz", base + "_polcal.txt", base + "_polcal.png"]
    assert all(("wrote " + f) in out and os.path.getsize(f) > 0 for f in files)
    back = dict(np.load(files[0]))
    assert sorted(back) == sorted(["spec", "noise", "used", "phi", "tau", "F", "results", "bursts", "tau_us", "tau_ns", "tau_err_ns", "rm"])
    cal = k["cal"]
    assert back["tau"].shape == (65,) and abs(back["tau"][42] - 2.5e-3) < 1e-15 and back["phi"].tolist() == [pc.KNOWN_CAL_RM]
    assert back["F"].view(np.float32).tobytes() == cal["F"].tobytes() and pc.same_results(back["results"], cal["results"])
    assert back["spec"].tobytes() == cal["spec"].tobytes() and back["used"].tobytes() == cal["used"].tobytes()
    assert back["bursts"].tobytes() == ccal.tobytes() and float(back["tau_us"]) == k["tau"] and float(back["tau_ns"]) == k["tau"] * 1e3
    assert float(back["rm"]) == pc.KNOWN_CAL_RM and float(back["tau_err_ns"]) == k["tau_err"] * 1e3
    lines = open(files[1]).read().splitlines()
    assert [ln.split()[0] for ln in lines] == ["pulse0", "pulse1", "pulse2", "combined"]
    for ln, r in zip(lines, cal["results"]):
        name = ln.split()[0]
        assert ln == post.POLCAL_ROW % (name, r["tau"] * 1e3, r["tau_err"] * 1e3, r["rm"], r["rm_err"], np.degrees(r["psi"]),
                                        r["ridge_slope"] * 1e-3, r["nridge"], r["snr"])
    assert "tau   +2.5" in lines[3] and lines[3] in out
    # a range of RM trials instead: the map has a ridge, written in rad m^-2 per ns
    assert post.main(args[:2] + ["--rm-lo", "50", "--rm-hi", "650", "--rm-step", "5", "--tau-half", "4", "--dtau", "0.25"] + args[8:]) == 0
    capsys.readouterr()
    back2 = dict(np.load(files[0]))
    assert back2["phi"].shape == (121,) and back2["tau"].shape == (33,)             # (wide enough in RM to hold the ridge over +- 4 ns)
    comb = back2["results"][-1]
    assert abs(comb["ridge_slope"] * 1e-3 - 42.05) < 2.5 and abs(comb["tau"] * 1e3 - 2.5) < 0.1 and abs(comb["rm"] - 350.0) < 2.5
    assert post.main(args) == 0                                    # (the one-trial file again, for what follows)
    capsys.readouterr()
    # the target: without --polcal the RM is off by a hundred units, with it it is the restatement's
    targs = ["rmsynth", fil, "--dm", str(pc.KNOWN_DM), "--sample", str(int(ctgt[0]["sample"])), "--width", str(pc.KNOWN_WIDTH), "--off-gap", "32",
             "--off-len", "300"]
    assert post.main(targs) == 0
    plain = dict(np.load(base + "_rm.npz"))
    assert rc.same_results(plain["results"], k["plain"]["results"]) and plain["F"].view(np.float32).tobytes() == k["plain"]["F"].tobytes()
    r = plain["results"][0]
    assert abs(float(r["rm"]) - pc.KNOWN_TARGET_RM) >= 5.0 * float(r["rm_err"])
    assert post.main(targs + ["--polcal", files[0], "--profile", "--nbin", "32"]) == 0
    capsys.readouterr()
    fixed = dict(np.load(base + "_rm.npz"))
    assert sorted(fixed) == sorted(plain) and fixed["F"].shape == plain["F"].shape and fixed["results"].dtype == post.RM_RESULT
    assert fixed["F"].view(np.float32).tobytes() == k["F"].tobytes() and rc.same_results(fixed["results"], k["res"])
    r = fixed["results"][0]
    assert abs(float(r["rm"]) - k["fit64"]) <= k["tol"] and abs(float(r["rm"]) - pc.KNOWN_TARGET_RM) <= 0.5 * k["dphi"] + k["tol"]
    prof = dict(np.load(base + "_polprof.npz"))
    want = pco.profile(rows, hdr, ctgt, fixed["results"]["rm"], k["tau"], 32, 1)
    assert ppc.same({f: prof[f] for f in ("acc", "hits", "bins", "results", "used")}, want)
    with pytest.raises(post.InputError, match="not a _polcal.npz"):
        post.main(targs + ["--polcal", base + "_rm.npz"])
    with pytest.raises(post.InputError, match="--rm-known"):
        post.main(args[:2] + args[4:])


def test_polprof_with_polcal_returns_the_injected_swing(emu_lib, tmp_path, monkeypatch):
    """the burst of tests/polprof_cases.known_case (PA swinging from -30 to +30 degrees, RM 350) behind a delay of 2.5 ns, next
    to a calibrator pulse: `post polprof --polcal` returns the swing within 4 sigma per bin.  What cannot be separated stays in:
    the phase 2 pi f0 tau0 that the delay leaves at the reference frequency f0 turns every PA by pi f0 tau0 (absolute PA
    calibration is out of scope), so the injected PA is compared with that constant added."""
    c, injected = ppc.known_case()
    hdr = c["hdr"]
    ramp = np.pi * pco.freqs(hdr) * (pc.KNOWN_TAU_NS * 1e-3)
    rng = np.random.default_rng(9100)
    x = 100.0 + rng.integers(-5, 6, size=(4096, 4, 1024)).astype(np.float64)
    l2, d, chans = ro.lambda2(hdr), ro.delays(hdr, 50.0), np.arange(1024)
    pa = np.radians(np.linspace(ppc.KNOWN_SWING[0], ppc.KNOWN_SWING[1], ppc.KNOWN_WIDTH))
    on_lo = 2000 - ppc.KNOWN_WIDTH // 2
    for t in range(ppc.KNOWN_WIDTH):
        ang = 2.0 * (pa[t] + ramp + ppc.KNOWN_RM * l2)
        for p, v in enumerate((np.full(1024, 20.0), 18.0 * np.cos(ang), 18.0 * np.sin(ang), np.full(1024, 2.0))):
            x[on_lo + t + d, p, chans] += v
    for t in range(8):                                             # the calibrator pulse: constant PA, the same RM, the same delay
        ang = 2.0 * (0.3 + ramp + ppc.KNOWN_RM * l2)
        for p, v in enumerate((np.full(1024, 60.0), 54.0 * np.cos(ang), 54.0 * np.sin(ang), np.full(1024, 6.0))):
            x[3200 + t + d, p, chans] += v
    rows = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    fil = pc.write_fil(str(tmp_path / "swing.fil"), hdr, rows)
    base = fil.replace(".fil", "")
    monkeypatch.setattr(_lib, "load", lambda path=None: emu_lib)
    assert post.main(["polcal", fil, "--dm", "50", "--sample", "3204", "--width", "8", "--rm-known", str(ppc.KNOWN_RM), "--tau-half", "8",
                      "--dtau", "0.25", "--off-gap", "32", "--off-len", "400"]) == 0
    tau = post.polcal_tau(base + "_polcal.npz")
    assert abs(tau * 1e3 - pc.KNOWN_TAU_NS) < 0.05
    pargs = ["polprof", fil, "--dm", "50", "--sample", "2000", "--width", str(ppc.KNOWN_WIDTH), "--rm", str(ppc.KNOWN_RM), "--nbin", "64",
             "--ref", "zero", "--off-gap", "32", "--off-len", "400"]
    assert post.main(pargs + ["--polcal", base + "_polcal.npz"]) == 0
    prof = dict(np.load(base + "_polprof.npz"))                    # (read now: the file is written again below)
    f0 = float(pco.freqs(hdr).mean())
    turned = injected + np.pi * f0 * (pc.KNOWN_TAU_NS * 1e-3)
    ppc.check_known(prof["bins"][0], prof["results"][0], turned)
    # without --polcal the ramp winds the band down: nothing like the swing is left
    assert post.main(pargs) == 0
    raw = np.load(base + "_polprof.npz")
    assert raw["bins"]["l"][0].max() < 0.5 * prof["bins"]["l"][0].max()
