"""Shared case builder of the burst polarisation tests (tests/test_rm.py on the emulator, tests/test_gpu_rm.py on the device).
Small four-product files built from a formula: a dispersed burst of given DM, width, RM, PA0, linear and circular fraction on a
flat noise floor, as 8-, 16-bit or float32 rows, in either product order (I Q U V, or the coherency products PP QQ Re Im).
Expected values are tests/rm_oracle.py's, computed once per case and shared (read-only)."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import _lib, post
from tests import post_cases as poc
from tests import rm_oracle as ro


def make_hdr(nchan, foff_sign=-1, tsamp=64e-6, bw=32.0, ftop=1416.0):
    return dict(poc.make_hdr(nchan, foff_sign=foff_sign, tsamp=tsamp, bw=bw, ftop=ftop), nifs=4)


def burst_file(hdr, nrows, nbits, bursts, coherency=False, seed=1, amp=60.0, sigma=3.0):
    """rows [nrows][4][nchan].  bursts: dicts(dm, sample, width, rm, pa0, lin, circ).  Per on-pulse sample of channel c:
    I = amp, Q = amp lin cos(2 (pa0 + rm l2_c)), U = amp lin sin(..), V = amp circ; every product sits on a floor of 100 with
    uniform integer noise of about `sigma`.  8 bit: the codes; 16 bit: the same x 200; float32: the same x 0.37 - 3."""
    nchan = hdr["nchans"]
    rng = np.random.default_rng(7000 + seed)
    half = max(1, int(round(sigma * np.sqrt(3.0))))
    x = 100.0 + rng.integers(-half, half + 1, size=(nrows, 4, nchan)).astype(np.float64)
    l2 = ro.lambda2(hdr)
    chans = np.arange(nchan)
    for b in bursts:
        d = ro.delays(hdr, b["dm"])
        ang = 2.0 * (b["pa0"] + b["rm"] * l2)
        i, q, u, v = (np.full(nchan, amp), amp * b["lin"] * np.cos(ang), amp * b["lin"] * np.sin(ang), np.full(nchan, amp * b["circ"]))
        prods = [0.5 * (i + v), 0.5 * (i - v), 0.5 * q, 0.5 * u] if coherency else [i, q, u, v]
        on_lo = b["sample"] - b["width"] // 2
        for t in range(on_lo, on_lo + b["width"]):
            r = t + d
            ok = (r >= 0) & (r < nrows)
            for p in range(4):
                x[r[ok], p, chans[ok]] += prods[p][ok]
    x = np.rint(x)
    if nbits == 8:
        return np.clip(x, 0, 255).astype(np.uint8)
    if nbits == 16:
        return np.clip(x * 200, 0, 65535).astype(np.uint16)
    return (x * 0.37 - 3.0).astype(np.float32)


def cands_of(bursts, off_gap=16, off_len=200):
    return post.burst_cands([(b["dm"], b["sample"], b["width"]) for b in bursts], off_gap, off_len)


def desc_of(hdr, rows):
    return post.fil_desc(dict(hdr, nifs=rows.shape[1], nbits=rows.dtype.itemsize * 8))


def burst_par(coherency=False, size=None):
    return _lib.FrbchBurstParams(C.sizeof(_lib.FrbchBurstParams) if size is None else size,
                                 _lib.BURST_COHERENCY if coherency else _lib.BURST_STOKES)


# ---- the small cases -------------------------------------------------------------------------------------------------
# name -> (nchan, nrows, nbits, coherency, foff_sign, bursts, off_gap, off_len)
B1 = dict(dm=56.7, sample=1500, width=6, rm=900.0, pa0=0.4, lin=0.8, circ=0.2)
B2 = dict(dm=20.0, sample=2600, width=3, rm=-2500.0, pa0=-1.0, lin=0.5, circ=-0.3)
B_EDGE = dict(dm=56.7, sample=90, width=8, rm=300.0, pa0=0.1, lin=0.9, circ=0.0)       # the earlier off window leaves the data
B_LATE = dict(dm=2100.0, sample=800, width=5, rm=100.0, pa0=0.0, lin=0.7, circ=0.1)    # delays up to ~3200 rows: most of the file
B_OUT = dict(dm=56.7, sample=9000, width=4, rm=0.0, pa0=0.0, lin=0.5, circ=0.0)        # wholly outside: no used channel
CASES = {
    "u8_64ch": (64, 4096, 8, False, -1, [B1], 16, 200),
    "u8_64ch_3cand": (64, 4096, 8, False, -1, [B1, B2, B_EDGE], 16, 200),
    "u16_64ch_coherency": (64, 4096, 16, True, -1, [B1, B2, B_EDGE], 16, 200),
    "f32_64ch": (64, 4096, 32, False, -1, [B1, B_EDGE], 16, 200),
    "f32_64ch_coherency": (64, 4096, 32, True, 1, [B2], 16, 200),
    "u8_96ch": (96, 4096, 8, False, 1, [B1, B2, B_OUT], 16, 200),
    "u16_96ch": (96, 4096, 16, False, -1, [B1], 16, 200),
    "u8_1024ch": (1024, 4096, 8, False, -1, [B1, B_EDGE, B_LATE], 16, 300),
    "u16_1024ch_coherency": (1024, 4096, 16, True, 1, [B2], 16, 300),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (hdr, rows, cands, coherency); the arrays are read-only"""
    nchan, nrows, nbits, coh, sign, bursts, gap, length = CASES[name]
    hdr = make_hdr(nchan, foff_sign=sign)
    rows = burst_file(hdr, nrows, nbits, bursts, coherency=coh, seed=len(name))
    rows.setflags(write=False)
    cands = cands_of(bursts, gap, length)
    cands.setflags(write=False)
    return dict(hdr, nbits=nbits), rows, cands, coh


@functools.lru_cache(maxsize=None)
def want_spectra(name):
    """-> (sums, spec, noise, used) of the oracle"""
    hdr, rows, cands, coh = case(name)
    sums = ro.burst_sums(rows, hdr, cands)
    out = (sums,) + ro.derive(sums, None, coh)
    for a in out:
        a.setflags(write=False)
    return out


GRID = dict(nphi=257, phi_lo=-12800.0, dphi=100.0)


@functools.lru_cache(maxsize=None)
def want_rm(name, nphi=GRID["nphi"], phi_lo=GRID["phi_lo"], dphi=GRID["dphi"]):
    """the composite of the oracle on the case, on the given grid"""
    hdr, rows, cands, coh = case(name)
    _sums, spec, noise, used = want_spectra(name)
    F, _re, _im = ro.transform(spec[:, 1], spec[:, 2], used, hdr, nphi, phi_lo, dphi)
    res = ro.peaks(F, used, noise[:, 1], noise[:, 2], hdr, nphi, phi_lo, dphi)
    F.setflags(write=False)
    return F, res


def same_results(got, want):
    """RM_RESULT records: the integers and everything computed without libm's atan2 exactly; pa0 to 1e-12"""
    for f in ("kpeak", "nused", "fitted"):
        if got[f].tobytes() != want[f].tobytes():
            return False
    for f in ("rm", "rm_err", "peak", "snr", "sigma_f", "fwhm"):
        if got[f].tobytes() != want[f].tobytes():
            return False
    return bool(np.allclose(got["pa0"], want["pa0"], rtol=0, atol=1e-12))


# ---- spectra for the transform alone ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spectra(nchan, ncand, seed=0, masked=()):
    """q, u float32 [ncand][nchan] of rotating vectors with noise, used with `masked` channels cleared (every candidate) and one
    more cleared in the last candidate"""
    hdr = make_hdr(nchan)
    rng = np.random.default_rng(500 + seed)
    l2 = ro.lambda2(hdr)
    q = np.zeros((ncand, nchan), np.float32)
    u = np.zeros((ncand, nchan), np.float32)
    for i in range(ncand):
        ang = 2.0 * (0.3 * i + (700.0 - 900.0 * i) * l2)
        q[i] = (3.0 + i) * np.cos(ang) + rng.normal(0, 0.4, nchan)
        u[i] = (3.0 + i) * np.sin(ang) + rng.normal(0, 0.4, nchan)
    used = np.ones((ncand, nchan), np.uint8)
    used[:, list(masked)] = 0
    used[ncand - 1, nchan // 3] = 0
    for a in (q, u, used):
        a.setflags(write=False)
    return hdr, q, u, used


@functools.lru_cache(maxsize=None)
def want_transform(nchan, ncand, nphi, phi_lo, dphi, seed=0, masked=()):
    hdr, q, u, used = spectra(nchan, ncand, seed, masked)
    F, _re, _im = ro.transform(q, u, used, hdr, nphi, phi_lo, dphi)
    F.setflags(write=False)
    return F


# ---- the known answer ------------------------------------------------------------------------------------------------
KNOWN_RMS = (350.0, -1200.0)


def known_hdr():
    return make_hdr(1024, tsamp=256e-6, bw=300.0, ftop=1500.0)


@functools.lru_cache(maxsize=None)
def known_case():
    """1.2 - 1.5 GHz, 1024 channels, two bursts with RM +350 and -1200 rad m^-2 -> (hdr, rows, cands, grid)"""
    hdr = dict(known_hdr(), nbits=8)
    bursts = [dict(dm=50.0, sample=1200, width=8, rm=KNOWN_RMS[0], pa0=0.3, lin=0.9, circ=0.1),
              dict(dm=50.0, sample=2500, width=8, rm=KNOWN_RMS[1], pa0=-0.7, lin=0.9, circ=-0.2)]
    rows = burst_file(hdr, 4096, 8, bursts, seed=77)
    rows.setflags(write=False)
    cands = cands_of(bursts, 32, 400)
    cands.setflags(write=False)
    nphi, phi_lo, dphi = post.rm_grid(hdr)
    return hdr, rows, cands, (nphi, phi_lo, dphi)


@functools.lru_cache(maxsize=None)
def known_oracle():
    """-> dict: the oracle's composite on the known case, the fp64 evaluation of the same spectra, its peak trials and
    parabolas, the measured largest |F_int - F_fp64| / max |F_fp64| (delta) and the tolerance on rm that follows from
    twice that (see rm_tolerance)"""
    hdr, rows, cands, (nphi, phi_lo, dphi) = known_case()
    r = ro.burst_rm(rows, hdr, cands, nphi, phi_lo, dphi)
    F64 = ro.transform_fp64(r["spec"][:, 1], r["spec"][:, 2], r["used"], hdr, nphi, phi_lo, dphi)
    Fint = r["F"][..., 0].astype(np.float64) + 1j * r["F"][..., 1].astype(np.float64)
    delta = float(max(np.abs(Fint[i] - F64[i]).max() / np.abs(F64[i]).max() for i in range(F64.shape[0])))
    P = F64.real * F64.real + F64.imag * F64.imag
    k0 = [int(np.argmax(P[i])) for i in range(P.shape[0])]
    fit = [ro.parabola(P[i], k0[i], phi_lo, dphi) for i in range(P.shape[0])]
    tol = [rm_tolerance(P[i], k0[i], dphi, 2.0 * delta) for i in range(P.shape[0])]
    return dict(r, F64=F64, delta=delta, k0=k0, fit=fit, tol=tol)


def rm_tolerance(P, k, dphi, eps):
    """What an error of at most eps max|F| in every F does to the parabola's vertex, to first order with the denominator taken
    at its worst: every P is off by at most dP = (2 eps + eps^2) Pmax; delta = 0.5 (y- - y+) / den moves by at most
    dP / (|den| - 4 dP) + |0.5 (y- - y+)| 4 dP / (|den| - 4 dP)^2 trial steps."""
    pmax = float(P.max())
    dP = (2.0 * eps + eps * eps) * pmax
    ym, y0, yp = float(P[k - 1]), float(P[k]), float(P[k + 1])
    den = abs((ym - 2.0 * y0) + yp) - 4.0 * dP
    assert den > 0
    return (dP / den + abs(0.5 * (ym - yp)) * 4.0 * dP / (den * den)) * dphi


# ---- rows already on the device (or, for the emulator, in guarded host memory) ---------------------------------------
def device_burst_rm(lib, hdr, rows_ptr, nrows, cands, coh, nphi, phi_lo, dphi, flag=None):
    """frbch_burst_rm_device on rows at `rows_ptr` -> (dict(spec, noise, used, F, results), kernel_used[3])"""
    from tests import big_rows as bg
    n, nchan = cands.size, hdr["nchans"]
    spec, noise = np.zeros((n, 4, nchan), np.float32), np.zeros((n, 4, nchan), np.float32)
    used = np.zeros((n, nchan), np.uint8)
    F = np.zeros((n, nphi, 2), np.float32)
    res = np.zeros(n, dtype=post.RM_RESULT)
    par, rpar = burst_par(coh), post.rm_params(nphi, phi_lo, dphi)
    k = (C.c_uint32 * 3)(99, 99, 99)
    err = C.create_string_buffer(512)
    with bg.guarded():
        code = lib.frbch_burst_rm_device(C.byref(post.fil_desc(hdr)), rows_ptr, nrows, C.byref(par), cands.ctypes.data, n, None,
                                         flag.ctypes.data if flag is not None else None, C.byref(rpar), 0, spec.ctypes.data, noise.ctypes.data,
                                         used.ctypes.data, F.ctypes.data, res.ctypes.data, k, err, len(err))
    assert code == 0, err.value
    return dict(spec=spec, noise=noise, used=used, F=F, results=res), (k[0], k[1], k[2])


def check_beyond_the_mark(lib, br, mem, behind, off_len, kernels):
    """The composite on the rows of a tests/big_rows.BigRows with four products: a burst of DM 104 that reaches the top of the
    band `behind` rows behind the row of the last byte mark, its own amplitude in every product; a second candidate in front of
    the first mark and a third whose later window is cut at nrows.  kernels: (shift of the rows in bytes, the spectra's kernel,
    the transform's form) per pass.  The expected sums are the oracle's on the window of rows each candidate reads."""
    from tests import big_rows as bg
    res = bg.Resident(br, mem)
    try:
        hdr = br.hdr()
        t_top, width, gap = br.byte_mark_rows[-1] + behind, 4, 16
        maxd = int(ro.delays(hdr, 104.0).max())
        reach = gap + off_len
        cands = post.burst_cands([(104.0, t_top + width // 2, width), (104.0, min(1000, br.byte_mark_rows[0] // 2), 6),
                                  (104.0, br.nrows - maxd - 3 * off_len // 4, 5)], gap, off_len)
        for shift, k_spec, k_rm in kernels:
            res.lay(shift)
            for prod, amp in enumerate((9, 5, 3, 2)):
                bg.write_burst(res, prod, 104.0, t_top, width, amp)
            want_sums = np.zeros((3, 4, br.nchan), dtype=post.BURST_SUMS)
            for i, c in enumerate(cands):
                on_lo = int(c["sample"]) - int(c["width"]) // 2
                w0 = max(0, on_lo - reach)
                w1 = min(br.nrows, on_lo + int(c["width"]) + reach + maxd + 1)
                moved = cands[i:i + 1].copy()
                moved["sample"] -= w0
                want_sums[i] = ro.burst_sums(res.window(w0, w1 - w0), hdr, moved)[0]
            assert want_sums["off_hits"][2].min() < 2 * off_len <= want_sums["off_hits"][2].max()
            assert (want_sums["off_hits"][:2] == 2 * off_len).all()
            spec, noise, used = ro.derive(want_sums)
            assert used.all() and abs(float(spec[0, 0].mean()) - 9.0) < 1.0 and abs(float(spec[1, 0].mean())) < 1.0
            F, _re, _im = ro.transform(spec[:, 1], spec[:, 2], used, hdr, **GRID)
            got, k = device_burst_rm(lib, hdr, C.c_void_p(res.address), br.nrows, cands, False, **GRID)
            assert k[:2] == (k_spec, k_rm)
            assert got["spec"].tobytes() == spec.tobytes() and got["noise"].tobytes() == noise.tobytes() and got["used"].tobytes() == used.tobytes()
            assert got["F"].tobytes() == F.tobytes()
            assert same_results(got["results"], ro.peaks(F, used, noise[:, 1], noise[:, 2], hdr, **GRID))
            res.buf.check()
        res.check_equals()                                   # the rows are never written
    finally:
        res.free()
