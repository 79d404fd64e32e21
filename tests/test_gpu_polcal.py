"""GPU tests of the polarisation calibration: the cases of tests/test_polcal.py on the device, every device buffer a guarded
buffer of exactly the documented size, checksummed (inputs) and guard-checked behind every call.  Both forms of the delay x RM
transform are forced by shape and address -- fewer than 64 phi trials, or an F laid 4 bytes off its 8-byte boundary, take the
generic kernel, so that every shape of the fast kernel runs through the generic one as well -- with kernel_used asserted against
the query and against the plan rule restated in tests/polcal_cases.py; fast = generic = tests/polcal_oracle.py byte for byte."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import post
from tests import big_rows as bg
from tests import polcal_cases as pc
from tests import polcal_oracle as pco
from tests import polprof_cases as ppc
from tests import rm_cases as rc
from tests.hipmem import GuardedBuffer
from tests.test_gpu_polprof import plan_expected
from tests.test_gpu_rm import device_rm, held

pytestmark = pytest.mark.gpu

FAST, GENERIC = pc.FAST, pc.GENERIC


def device_rmd(lib, hdr, q, u, used, nphi, phi_lo, dphi, ntau, tau_lo, dtau, misalign=0):
    """frbch_rmdelay_device -> (F float32 [ncand][ntau][nphi][2], (form, split)); misalign = 4 lays F off its 8-byte boundary,
    which takes the generic kernel at any shape"""
    ncand = q.shape[0]
    bufs = [held(np.ascontiguousarray(a)) for a in (q.astype(np.float32), u.astype(np.float32), used.astype(np.uint8))]
    d_F = GuardedBuffer(ncand * ntau * nphi * 8 + misalign)
    f_ptr = C.c_void_p(d_F.ptr.value + misalign)
    par = post.rmd_params(nphi, phi_lo, dphi, ntau, tau_lo, dtau)
    nsplit = C.c_uint32(99)
    query = lib.frbch_rmdelay_kernel(C.byref(post.fil_desc(hdr)), f_ptr, ncand, C.byref(par), C.byref(nsplit))
    k = (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    with bg.guarded():
        code = lib.frbch_rmdelay_device(C.byref(post.fil_desc(hdr)), bufs[0][1], bufs[1][1], bufs[2][1], ncand, C.byref(par), 0, f_ptr, k,
                                        err, len(err))
    assert code == 0, err.value
    for b, _p in bufs:
        b.check(contents=True)
        b.free()
    d_F.check()
    F = d_F.to_numpy(np.uint8)[misalign:].view(np.float32).reshape(ncand, ntau, nphi, 2).copy()
    d_F.free()
    assert (k[0], k[1]) == (query, nsplit.value)
    return F, (k[0], k[1])


def test_the_cases_reach_every_branch_of_the_plan():
    """what the shapes below are chosen for (no device needed to say so): tau tiles of 1, 2, 4 and 8, the tile of 8 with and
    without a tail, a phi tail, split 1 and splits that do and do not divide the channels"""
    tiles = {n: pc.tau_tile(pc.SHAPES[n][5]) for n in pc.FAST_SHAPES}
    assert tiles == {"k_tail_ntau1": 1, "ntau_T-1": 1, "ntau_T": 8, "ntau_T+1": 2, "ntau_2T+1": 2, "ntau_2T-1_tail": 8, "ntau_12_tile4": 4,
                     "split1_many_cands": 1, "largest": 2}
    plans = {n: pc.expected_plan(*pc.SHAPES[n][:3], pc.SHAPES[n][5]) for n in pc.SHAPES}
    assert plans["generic_nphi1"] == plans["generic_nphi63"] == (GENERIC, 1) and plans["split1_many_cands"] == (FAST, 1)
    assert plans["ntau_T"] == (FAST, 2) and plans["ntau_T-1"] == (FAST, 2) and plans["ntau_T+1"] == (FAST, 16) and plans["ntau_2T+1"] == (FAST, 16)
    assert plans["largest"] == (FAST, 16) and plans["k_tail_ntau1"] == (FAST, 1)


@pytest.mark.parametrize("name", sorted(pc.SHAPES))
def test_transform_equals_the_restatement_in_both_forms(hip_lib, name):
    """at the aligned address (the fast kernel wherever nphi >= 64) and 4 bytes further on (the generic one)"""
    nchan, ncand, nphi, _pl, _dp, ntau, _tl, _dt, masked = pc.SHAPES[name]
    hdr, q, u, used = rc.spectra(nchan, ncand, 0, masked)
    want = pc.want_transform(name).tobytes()
    F, k = device_rmd(hip_lib, hdr, q, u, used, **pc.grid_of(name))
    assert k == pc.expected_plan(nchan, ncand, nphi, ntau) and F.tobytes() == want
    assert (k[0] == FAST) == (name in pc.FAST_SHAPES)
    F, k = device_rmd(hip_lib, hdr, q, u, used, misalign=4, **pc.grid_of(name))
    assert k == (GENERIC, 1) and F.tobytes() == want


def test_one_trial_at_zero_delay_is_rm_synthesis_in_both_forms(hip_lib):
    for nchan, ncand, nphi, phi_lo, dphi, masked in ((64, 3, 63, -3100.0, 100.0, (3, 40)), (96, 3, 257, -3000.0, 23.5, ()),
                                                     (1000, 3, 257, -12800.0, 100.0, ())):
        hdr, q, u, used = rc.spectra(nchan, ncand, 0, masked)
        for misalign in (0, 4):
            plain, k1 = device_rm(hip_lib, hdr, q, u, used, nphi, phi_lo, dphi, misalign=misalign)
            F, k2 = device_rmd(hip_lib, hdr, q, u, used, nphi, phi_lo, dphi, 1, 0.0, 1.0e-3, misalign=misalign)
            assert k1 == k2 == ((FAST if nphi >= 64 and not misalign else GENERIC), k2[1])
            assert F[:, 0].tobytes() == plain.tobytes() == rc.want_transform(nchan, ncand, nphi, phi_lo, dphi, 0, masked).tobytes()


def test_a_dead_candidate_and_a_grid_across_zero_on_the_device(hip_lib):
    hdr, q, u, used = rc.spectra(96, 3, 1)
    q2, u2, used2 = q.copy(), u.copy(), used.copy()
    q2[1], u2[1] = 0.0, 0.0
    used2[2] = 0                                                   # no used channel
    grid = dict(nphi=70, phi_lo=-3000.0, dphi=90.0, ntau=5, tau_lo=-2.0e-3, dtau=1.0e-3)
    want = pco.transform(q2, u2, used2, hdr, **grid)[0]
    for misalign, form in ((0, FAST), (4, GENERIC)):
        F, k = device_rmd(hip_lib, hdr, q2, u2, used2, misalign=misalign, **grid)
        assert k[0] == form and F[0].any() and not F[1].any() and not F[2].any() and F.tobytes() == want.tobytes()


def test_nothing_wraps_at_16384_full_scale_channels_on_the_device(hip_lib):
    hdr, q, u, used, grid, want, largest, _re_max = pc.full_scale_case()
    assert (1 << 59) - (1 << 50) < largest <= 1 << 60
    F, k = device_rmd(hip_lib, hdr, q, u, used, **grid)
    assert k == pc.expected_plan(16384, 1, grid["nphi"], grid["ntau"]) and k[0] == FAST and k[1] > 1 and F.tobytes() == want.tobytes()
    F, k = device_rmd(hip_lib, hdr, q, u, used, misalign=4, **grid)
    assert k == (GENERIC, 1) and F.tobytes() == want.tobytes()


# ---- the composite and the known answer --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u8_64ch_3cand", "u16_64ch_coherency", "u8_96ch", "u8_1024ch"])
def test_composite_equals_the_restatement(hip_lib, name):
    hdr, rows, cands, coh = rc.case(name)
    grid = dict(nphi=65, phi_lo=-3200.0, dphi=100.0, ntau=5, tau_lo=-2.0e-3, dtau=1.0e-3)
    want = pco.burst_polcal(rows, hdr, cands, coherency=coh, **grid)
    n, nchan = cands.size, hdr["nchans"]
    for misalign in (0, 4):
        buf, ptr = held(rows, misalign)
        spec, noise = np.zeros((n, 4, nchan), np.float32), np.zeros((n, 4, nchan), np.float32)
        used = np.zeros((n, nchan), np.uint8)
        F = np.zeros((n, 5, 65, 2), np.float32)
        res = np.zeros(n + 1, dtype=post.RMD_RESULT)
        par, rpar = rc.burst_par(coh), post.rmd_params(**grid)
        k = (C.c_uint32 * 3)(99, 99, 99)
        err = C.create_string_buffer(512)
        with bg.guarded():
            code = hip_lib.frbch_burst_polcal_device(C.byref(post.fil_desc(hdr)), ptr, rows.shape[0], C.byref(par), cands.ctypes.data, n, None, None,
                                                     C.byref(rpar), 0, spec.ctypes.data, noise.ctypes.data, used.ctypes.data, F.ctypes.data,
                                                     res.ctypes.data, k, err, len(err))
        assert code == 0, err.value
        buf.check(contents=True)
        buf.free()
        fast_rows = rows.dtype != np.float32 and (nchan * rows.dtype.itemsize) % 64 == 0 and misalign % 16 == 0
        assert (k[0], k[1]) == (FAST if fast_rows else GENERIC, FAST) and k[2] == pc.expected_plan(nchan, n, 65, 5)[1]
        assert spec.tobytes() == want["spec"].tobytes() and noise.tobytes() == want["noise"].tobytes() and used.tobytes() == want["used"].tobytes()
        assert F.tobytes() == want["F"].tobytes() and pc.same_results(res, want["results"])


def test_known_delay(hip_lib):
    """the injected 2.5 ns at 1.2 - 1.5 GHz through the host entry point, three of the twelve seeds that tests/test_polcal.py
    holds the restatement to: its bits, hence the trial of the plain fp64 evaluation and a delay within 2 tau_err"""
    for seed in (0, 5, 11):
        hdr, rows, cands = pc.known_pulse(seed)
        k = pc.known_pulse_oracle(seed)
        info = {}
        got = post.polcal(rows, hdr, cands, lib=hip_lib, info=info, **k["grid"])
        assert info["spectra_kernel_used"] == FAST and info["kernel_used"] == GENERIC          # --rm-known: one phi trial
        assert np.ascontiguousarray(got["F"]).view(np.float32).tobytes() == k["F"].tobytes() and pc.same_results(got["results"], k["results"])
        r = got["results"][0]
        assert int(r["mpeak"]) == int(np.argmax(np.abs(k["F64"][0, :, 0]) ** 2))
        assert abs(float(r["tau"]) * 1e3 - pc.KNOWN_TAU_NS) <= 2.0 * float(r["tau_err"]) * 1e3
    hdr, rows, cands = pc.known_pulse(0)
    want = pco.burst_polcal(rows, hdr, cands, **pc.RIDGE_GRID)
    info = {}
    got = post.polcal(rows, hdr, cands, lib=hip_lib, info=info, **pc.RIDGE_GRID)
    assert info["kernel_used"] == FAST and pc.same_results(got["results"], want["results"])
    F64 = pco.transform_fp64(want["spec"][:, 1], want["spec"][:, 2], want["used"], hdr, **pc.RIDGE_GRID)
    tol = pc.ridge_tolerance(np.abs(F64[0]) ** 2, pc.RIDGE_GRID)
    assert abs(float(got["results"]["ridge_slope"][0]) - pc.analytic_ridge_slope(hdr, want["used"][0])) <= tol


# ---- the profile -----------------------------------------------------------------------------------------------------
def _cal_device(lib, c, ptr, tau):
    hdr, n = c["hdr"], c["cands"].size
    out = ppc.outputs(n, max(1, min(c["nbin"], 1024)), hdr["nchans"])
    k = (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    with bg.guarded():
        code = lib.frbch_polprof_cal_device(C.byref(post.fil_desc(dict(hdr, nifs=4))), ptr, c["rows"].shape[0], C.byref(rc.burst_par(c["coh"])),
                                            c["cands"].ctypes.data, n, c["rm"].ctypes.data, tau.ctypes.data if tau is not None else None,
                                            c["gain"].ctypes.data if c["gain"] is not None else None,
                                            c["flag"].ctypes.data if c["flag"] is not None else None, C.byref(ppc.par_of(c)), 0,
                                            out["acc"].ctypes.data, out["hits"].ctypes.data, out["bins"].ctypes.data, out["results"].ctypes.data,
                                            out["used"].ctypes.data, k, err, len(err))
    assert code == 0, err.value
    return out, (k[0], k[1])


@pytest.mark.parametrize("name", ["u8_64ch_33x3", "u8_96ch_ascending", "u16_64ch_coherency", "u8_64ch_flag_gain", "u8_1024ch_late"])
def test_profile_with_and_without_a_delay_in_both_kernels(hip_lib, name):
    """tau = NULL: the bytes of frbch_polprof_device; with a delay: the restatement's acc / hits to the bit, at the aligned
    address (the fast profile kernel wherever the layout allows it) and 4 bytes further on (the generic one)"""
    c = ppc.case(name)
    n = c["cands"].size
    tau = np.array(([2.5e-3, -40.0, 0.0] + [1.0e-3] * n)[:n])
    want = pco.profile(c["rows"], c["hdr"], c["cands"], c["rm"], tau, c["nbin"], c["tfactor"], c["ref"], c["gain"], c["flag"], c["coh"])
    kernels = []
    for misalign in (0, 4):
        buf, ptr = held(c["rows"], misalign)
        with bg.guarded():
            code, msg, old, k_old = ppc.call(hip_lib.frbch_polprof_device, c, ptr)
        assert code == 0, msg
        new, k_new = _cal_device(hip_lib, c, ptr, None)
        assert k_new == k_old == (k_old[0], ppc.query(hip_lib, c, ptr)) and all(new[f].tobytes() == old[f].tobytes() for f in old)
        got, k = _cal_device(hip_lib, c, ptr, tau)
        buf.check(contents=True)
        buf.free()
        assert k == k_old and ppc.same(got, want), (name, misalign)
        kernels.append(k[1])
    assert kernels == [plan_expected(c, 0), GENERIC]
    if name != "u8_96ch_ascending" and name != "u8_1024ch_late":
        assert kernels[0] == FAST
