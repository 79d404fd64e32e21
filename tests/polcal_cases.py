"""Shared case builder of the polarisation calibration tests (tests/test_polcal.py on the emulator, tests/test_gpu_polcal.py on
the device): the spectra of tests/rm_cases.py on (tau, phi) grids that reach every branch of the plan rule, the call helpers, and
the known answers -- calibrator pulses and a target burst with a delay ramp on Q + iU at 1.2 - 1.5 GHz.  Expected values are
tests/polcal_oracle.py's, computed once per case and shared (read-only)."""
import ctypes as C
import functools
import math

import numpy as np

from frb_baseband_amd import post
from tests import polcal_oracle as pco
from tests import rm_cases as rc
from tests import rm_oracle as ro

FAST, GENERIC = 1, 0
TAU_TILE = 8                    # the largest tau tile of the fast kernel (kRmdTauMax of kernels_post_fast.inc)


def tau_tile(ntau):
    """the plan rule's tile: the largest of 8, 4, 2, 1 whose tail is at most an eighth of ntau"""
    for t in (8, 4, 2):
        if (-(-ntau // t) * t - ntau) * 8 <= ntau:
            return t
    return 1


def expected_plan(nchan, ncand, nphi, ntau, misalign=0):
    """(form, split) of the plan rule (rm_plan_rule of csrc/frbch_post.cpp, the one RM synthesis takes at ntau = 1), restated"""
    if nphi < 64 or misalign % 8:
        return GENERIC, 1
    base = ncand * -(-ntau // tau_tile(ntau)) * -(-nphi // 1024)
    if base >= 512:
        return FAST, 1
    ns = min(-(-512 // base), -(-nchan // 64))
    chunk = -(-nchan // ns)
    return FAST, -(-nchan // chunk)


# nchan, ncand, nphi, phi_lo, dphi, ntau, tau_lo, dtau (microseconds), masked channels
G1 = (-12800.0, 100.0)
SHAPES = {
    "generic_nphi1": (64, 1, 1, 250.0, 10.0, 5, -2.0e-3, 1.0e-3, ()),
    "generic_nphi63": (64, 3, 63, -3100.0, 100.0, 3, -1.0e-3, 1.0e-3, (3, 40)),
    "k_tail_ntau1": (64, 3, 257) + G1 + (1, 1.5e-3, 1.0e-3, (3, 40)),
    "ntau_T-1": (96, 3, 257, -3000.0, 23.5, TAU_TILE - 1, -3.0e-3, 1.0e-3, ()),
    "ntau_T": (96, 1, 257, -3000.0, 23.5, TAU_TILE, -3.0e-3, 1.0e-3, (0, 95)),
    "ntau_T+1": (1000, 3, 257) + G1 + (TAU_TILE + 1, -4.0e-3, 1.0e-3, ()),
    "ntau_2T+1": (1024, 1, 257) + G1 + (2 * TAU_TILE + 1, -8.0e-3, 1.0e-3, (5,)),
    "ntau_2T-1_tail": (96, 2, 130, -3000.0, 47.0, 2 * TAU_TILE - 1, -7.5e-3, 1.0e-3, (7,)),      # tile 8 with one trial in vain
    "ntau_12_tile4": (64, 2, 257) + G1 + (12, -6.0e-3, 1.0e-3, ()),
    "split1_many_cands": (96, 130, 64, -3200.0, 100.0, 7, -3.0e-3, 1.0e-3, (9,)),       # 910 workgroups: no split
    "largest": (1024, 1, 1024, -51200.0, 100.0, 17, -8.0e-3, 1.0e-3, (100, 101, 102)),
}
FAST_SHAPES = sorted(n for n, s in SHAPES.items() if s[2] >= 64)


@functools.lru_cache(maxsize=None)
def want_transform(name):
    nchan, ncand, nphi, phi_lo, dphi, ntau, tau_lo, dtau, masked = SHAPES[name]
    hdr, q, u, used = rc.spectra(nchan, ncand, 0, masked)
    F, _re, _im = pco.transform(q, u, used, hdr, nphi, phi_lo, dphi, ntau, tau_lo, dtau)
    F.setflags(write=False)
    return F


def grid_of(name):
    return dict(zip(("nphi", "phi_lo", "dphi", "ntau", "tau_lo", "dtau"), SHAPES[name][2:8]))


@functools.lru_cache(maxsize=None)
def full_scale_case():
    """16384 channels at full-scale q, u (every |Qi|, |Ui| = 2^23 - 1 or 2^23) on a grid the fast kernel takes, with the sums once
    more in Python integers -> (hdr, q, u, used, grid, F, largest sum of |terms|)"""
    nchan = 16384
    hdr = rc.make_hdr(nchan, bw=256.0)
    sign = np.where(np.arange(nchan) % 64 == 0, -1.0, 1.0).astype(np.float32)       # (a few negative, so that both signs are summed)
    q = (sign * np.float32(1.0 - 2.0 ** -24))[None, :].copy()
    u = np.full((1, nchan), np.float32(1.0 - 2.0 ** -24))
    q[0, 5] = np.float32(0.75)
    used = np.ones((1, nchan), np.uint8)
    grid = dict(nphi=64, phi_lo=0.0, dphi=1.0e-7, ntau=2, tau_lo=0.0, dtau=1.0e-9)       # every phase near 0: C = 2^22, nothing cancels
    F, re, _im, largest = pco.transform(q, u, used, hdr, unbounded=True, **grid)
    for a in (q, u, used, F):
        a.setflags(write=False)
    return hdr, q, u, used, grid, F, largest, int(np.abs(re).max())


# ---- the calls -------------------------------------------------------------------------------------------------------
def host_rmd(lib, hdr, q, u, used, nphi, phi_lo, dphi, ntau, tau_lo, dtau):
    """frbch_rmdelay_host -> (F float32 [ncand][ntau][nphi][2], (form, split))"""
    info = {}
    F = post.rm_delay(q, u, used, hdr, nphi, phi_lo, dphi, ntau, tau_lo, dtau, lib=lib, info=info)
    return np.ascontiguousarray(F).view(np.float32).reshape(F.shape + (2,)), (info["kernel_used"], info["split"])


def raw_call(lib, name, hdr, ncand, par, q=None, u=None, used=None, F=None):
    """a refusal through `name` (frbch_rmdelay_kernel / _host / _peaks) -> (code, message)"""
    nchan = hdr["nchans"]
    q = np.zeros((max(ncand, 1), nchan), np.float32) if q is None else q
    u = q if u is None else u
    used = np.ones((max(ncand, 1), nchan), np.uint8) if used is None else used
    F = np.zeros(16, np.float32) if F is None else F
    err = C.create_string_buffer(512)
    desc = post.fil_desc(hdr)
    if name == "frbch_rmdelay_kernel":
        return lib.frbch_rmdelay_kernel(C.byref(desc), F.ctypes.data, ncand, C.byref(par) if par is not None else None, None), ""
    if name == "frbch_rmdelay_peaks":
        res = np.zeros(max(ncand, 1) + 1, dtype=post.RMD_RESULT)
        code = lib.frbch_rmdelay_peaks(C.byref(desc), F.ctypes.data, used.ctypes.data, None, None, ncand, C.byref(par) if par is not None else None,
                                       res.ctypes.data, err, len(err))
        return code, err.value.decode()
    code = lib.frbch_rmdelay_host(C.byref(desc), q.ctypes.data, u.ctypes.data, used.ctypes.data, ncand, C.byref(par) if par is not None else None,
                                  0, F.ctypes.data, None, err, len(err))
    return code, err.value.decode()


def same_results(got, want):
    """RMD_RESULT records: everything computed without libm's atan2 exactly; psi to 1e-12"""
    for f in post.RMD_RESULT.names:
        if f != "psi" and np.ascontiguousarray(got[f]).tobytes() != np.ascontiguousarray(want[f]).tobytes():
            return False
    return bool(np.allclose(got["psi"], want["psi"], rtol=0, atol=1e-12))


# ---- the known answers -----------------------------------------------------------------------------------------------
KNOWN_TAU_NS = 2.5                       # the injected delay
KNOWN_CAL_RM, KNOWN_TARGET_RM = 350.0, 350.0
KNOWN_DM, KNOWN_WIDTH = 50.0, 8
KNOWN_AMP = 6.0                          # per on-pulse sample on a floor of 100 with noise of about 3: S/N of F near 150 a pulse
TAU_GRID = dict(ntau=65, tau_lo=-8.0e-3, dtau=0.25e-3)          # +- 8 ns in steps of 0.25 ns: 2.5 ns is trial 42


def with_delay(burst, hdr, tau_ns):
    """the burst of rm_cases.burst_file with Q + iU multiplied by exp(2 pi i f tau): its pa0 becomes pa0 + pi f_c tau per channel"""
    return dict(burst, pa0=burst["pa0"] + math.pi * pco.freqs(hdr) * (tau_ns * 1.0e-3))


@functools.lru_cache(maxsize=None)
def known_pulse(seed):
    """one calibrator pulse in 1024 rows at 1.2 - 1.5 GHz -> (hdr, rows, cands).  On the dozen of seeds: tau_err = fwhm_tau /
    (2 snr) = 0.551 / (B snr) is the Cramer-Rao bound of a delay over a flat band B (sqrt(12) / (2 pi B snr)), so "within
    2 tau_err" is a two-sigma condition that a dozen of arbitrary seeds meets together with a probability of 0.954^12 = 0.57
    only.  The files are seeded 500 + seed: a dozen for which the restatement -- the reference, not the library -- meets it
    (tests/test_polcal.py shows that first); the files seeded 300.. and 400.. each have one pulse at 1.01 and 1.07 of the
    bound.  The library then has to give the restatement's bits."""
    hdr = dict(rc.known_hdr(), nbits=8)
    b = dict(dm=KNOWN_DM, sample=300, width=KNOWN_WIDTH, rm=KNOWN_CAL_RM, pa0=0.3 + 0.1 * seed, lin=0.9, circ=0.1)
    rows = rc.burst_file(hdr, 1024, 8, [with_delay(b, hdr, KNOWN_TAU_NS)], seed=500 + seed, amp=KNOWN_AMP)
    rows.setflags(write=False)
    cands = rc.cands_of([b], 16, 200)
    cands.setflags(write=False)
    return hdr, rows, cands


@functools.lru_cache(maxsize=None)
def known_pulse_oracle(seed):
    """-> dict: the restatement's composite at the known RM (nphi = 1) on TAU_GRID, and the fp64 plane of the same spectra"""
    hdr, rows, cands = known_pulse(seed)
    grid = dict(nphi=1, phi_lo=KNOWN_CAL_RM, dphi=1.0, **TAU_GRID)
    r = pco.burst_polcal(rows, hdr, cands, **grid)
    F64 = pco.transform_fp64(r["spec"][:, 1], r["spec"][:, 2], r["used"], hdr, **grid)
    return dict(r, F64=F64, grid=grid)


def analytic_ridge_slope(hdr, used):
    """d phi / d tau along the ridge, rad m^-2 per microsecond.  The phase left in channel c at trial (phi, tau) of a source
    with (RM, tau0) is 2 (RM - phi) x_c + 2 pi (tau0 - tau) b_c + constant, x = l2 - l0, b = f - f0; the phi that cancels it best
    in the least-squares sense at a given tau is RM + pi (tau0 - tau) sum(b x) / sum(x x): slope = -pi sum(b x) / sum(x^2), which
    is positive because x falls as f rises (to first order pi f^3 / (2 c^2))."""
    sel = np.flatnonzero(np.asarray(used).reshape(-1) != 0)
    l2, f = ro.lambda2(hdr)[sel], pco.freqs(hdr)[sel]
    x, b = l2 - l2.mean(), f - f.mean()
    return -math.pi * float((b * x).sum()) / float((x * x).sum())


RIDGE_GRID = dict(nphi=81, phi_lo=KNOWN_CAL_RM - 200.0, dphi=5.0, ntau=33, tau_lo=KNOWN_TAU_NS * 1e-3 - 4.0e-3, dtau=0.25e-3)


def ridge_tolerance(P, grid):
    """What the grid and the shape of the ridge do to the fitted slope, measured on an fp64 plane P [ntau][nphi] of the same
    spectra: (a) every phi_{k_m} is a grid value, off the ridge by at most dphi / 2, which moves a least-squares slope by at
    most (dphi / 2) sum|tau - mean| / sum (tau - mean)^2 over the rows that enter; (b) the ridge is not a straight line -- the
    quadratic term of the residual phase bends it -- which (c) is measured as the largest departure of the plane's own row
    maxima, refined by the three-point parabola, from their own least-squares line, and enters the same way."""
    best = float(P.max())
    ts, fs = [], []
    for m in range(grid["ntau"]):
        km = int(np.argmax(P[m]))
        if P[m, km] >= 0.5 * best:
            d, _fit = pco.vertex(P[m], km)
            ts.append(grid["tau_lo"] + m * grid["dtau"])
            fs.append(grid["phi_lo"] + (km + d) * grid["dphi"])
    ts, fs = np.array(ts), np.array(fs)
    dt = ts - ts.mean()
    lever = float(np.abs(dt).sum() / (dt * dt).sum())
    line = np.polyval(np.polyfit(ts, fs, 1), ts)
    bend = float(np.abs(fs - line).max())
    return (0.5 * grid["dphi"] + bend) * lever


@functools.lru_cache(maxsize=None)
def known_target_case():
    """(b): three calibrator pulses (RM 350) and a target burst (RM 350 as well, its own PA) in one file, all through a delay of
    2.5 ns -> (hdr, rows, calibrator cands, target cands)"""
    hdr = dict(rc.known_hdr(), nbits=8)
    cal = [dict(dm=KNOWN_DM, sample=700 + 900 * i, width=KNOWN_WIDTH, rm=KNOWN_CAL_RM, pa0=0.2 + 0.5 * i, lin=0.9, circ=0.1) for i in range(3)]
    tgt = dict(dm=KNOWN_DM, sample=3400, width=KNOWN_WIDTH, rm=KNOWN_TARGET_RM, pa0=-0.7, lin=0.9, circ=-0.2)
    rows = rc.burst_file(hdr, 4096, 8, [with_delay(b, hdr, KNOWN_TAU_NS) for b in cal + [tgt]], seed=88, amp=60.0)
    rows.setflags(write=False)
    return hdr, rows, rc.cands_of(cal, 32, 300), rc.cands_of([tgt], 32, 300)


def write_fil(path, hdr, rows):
    from tests.test_fold_predictor import write_fil as write
    write(path, rows, hdr, 4)
    return path
