"""Shared case builder of the scattering tests (tests/test_scat.py on the emulator, tests/test_gpu_scat.py on the device): planes
and banks from a formula for the template-bank stage alone (frbch_tbank_*) at the smallest shapes at which the kernels can still
go wrong, the plan rule of the fast kernel restated, small files with the grids that reach every branch of frbch_burstscat_*,
a noise-free plane of known template and arrival, and bursts of known scattering injected through filterbank rows.  Expected
values are tests/scat_oracle.py's, computed once per case and shared (read-only); the bank is the library's own (frbch_scat_bank is
host code, the same in both builds), an INPUT of the oracle."""
import ctypes as C
import functools
import math

import numpy as np

from frb_baseband_amd import _lib, post
from tests import acf_cases as ac
from tests import dmscan_cases as dc
from tests import dmscan_oracle as do
from tests import rm_cases as rc
from tests import scat_oracle as so

B1, B2, B_EDGE, B_OUT, B_END = rc.B1, rc.B2, rc.B_EDGE, rc.B_OUT, dc.B_END
Y_MAX, P_MAX = so.Y_MAX, so.P_MAX
SNR_MIN = 5.0


@functools.lru_cache(maxsize=None)
def bank_lib():
    """the library that computes the banks of the cases: frbch_scat_bank is host code, the same in both builds (tests/test_scat.py holds
    the two equal) -- the product library where it is built, so that a GPU run compiles nothing, else the emulator build"""
    import os
    import subprocess
    try:
        return _lib.load()
    except _lib.LibraryMissing:
        pass
    emu_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    subprocess.check_call(["make", "-s", "-C", emu_dir])
    return _lib.load(os.path.join(emu_dir, "libfrbch_emu.so"))


@functools.lru_cache(maxsize=None)
def bank_of(nsig, ntau, ntap, lead, sigma0, rsig, tau0, rtau):
    """-> (what post.scat_bank returns, read-only; the parameters as a dict)"""
    par = post.scat_bank_params(nsig, ntau, ntap, lead, sigma0, rsig, tau0, rtau)
    bank = post.scat_bank(par, bank_lib())
    for a in bank.values():
        a.setflags(write=False)
    return bank, dict(nsig=nsig, ntau=ntau, ntap=ntap, lead=lead, sigma0=sigma0, rsig=rsig, tau0=tau0, rtau=rtau)


def bank_par(bp):
    return post.scat_bank_params(bp["nsig"], bp["ntau"], bp["ntap"], bp["lead"], bp["sigma0"], bp["rsig"], bp["tau0"], bp["rtau"])


# ---- the stage alone: planes and banks from a formula ----------------------------------------------------------------------
# name -> (n, nsub, nbin, K, ntap, lead, shift0, nshift, kind)
PLANES = {
    "nshift_1_nbin_9": (1, 3, 9, 2, 5, 2, 4, 1, "random"),
    "nshift_7_window_starts_before_bin_0": (1, 2, 16, 3, 6, 1, 0, 7, "random"),
    "nshift_8_lead_0_window_runs_off_the_end": (1, 2, 16, 3, 6, 0, 8, 8, "random"),
    "nshift_9_lead_is_the_last_tap": (2, 3, 20, 2, 7, 6, 3, 9, "random"),
    "ntap_1": (1, 2, 9, 3, 1, 0, 0, 9, "random"),
    "ntap_is_nbin": (1, 2, 16, 2, 16, 5, 0, 16, "random"),
    "ntap_above_nbin": (1, 2, 16, 2, 40, 13, 0, 16, "random"),
    "nbin_1024_every_shift": (1, 2, 1024, 2, 33, 8, 0, 1024, "random"),
    "one_template": (1, 4, 32, 1, 8, 2, 4, 20, "random"),
    "one_subband": (1, 1, 32, 3, 8, 2, 0, 32, "random"),
    # 16 shifts of 16 taps: 8 subbands a workgroup and 999 templates a run (the plan restated below)
    "templates_of_one_run": (1, 8, 64, 999, 16, 4, 10, 16, "random"),
    "one_template_and_one_subband_more": (1, 9, 64, 1000, 16, 4, 10, 16, "random"),
    "three_planes": (3, 5, 40, 6, 12, 3, 5, 30, "random"),
    "zero_one_plane_squared_bank": (2, 6, 50, 4, 10, 3, 0, 50, "01"),
    "full_scale_2_to_61": (1, 1, 1024, 1, 1024, 0, 0, 8, "alternating"),
}


@functools.lru_cache(maxsize=None)
def plane(name):
    """-> (y int32 [n][nsub][nbin], P int32 [K][ntap]), read-only"""
    n, nsub, nbin, K, ntap, _lead, _s0, _ns, kind = PLANES[name]
    rng = np.random.default_rng(9300 + len(name))
    if kind == "random":
        y = rng.integers(-Y_MAX, Y_MAX + 1, size=(n, nsub, nbin)).astype(np.int32)
        P = rng.integers(-P_MAX, P_MAX + 1, size=(K, ntap)).astype(np.int32)
        y.reshape(-1)[0], y.reshape(-1)[-1] = Y_MAX, -Y_MAX
        P.reshape(-1)[0], P.reshape(-1)[-1] = -P_MAX, P_MAX
    elif kind == "01":
        y = rng.integers(0, 2, size=(n, nsub, nbin)).astype(np.int32)
        P = (rng.integers(0, (1 << 15) + 1, size=(K, ntap)).astype(np.int64) ** 2).astype(np.int32)
        P.reshape(-1)[0] = P_MAX
    else:                                                          # signs that match tap for tap at shift 0, 2, ...
        y = np.where(np.arange(nbin) % 2 == 0, Y_MAX, -Y_MAX).astype(np.int32)[None, None, :].repeat(nsub, axis=1).repeat(n, axis=0)
        P = np.where(np.arange(ntap) % 2 == 0, P_MAX, -P_MAX).astype(np.int32)[None, :].repeat(K, axis=0)
    y.setflags(write=False)
    P.setflags(write=False)
    return y, P


@functools.lru_cache(maxsize=None)
def plane_want(name):
    _n, _nsub, _nbin, _K, _ntap, lead, shift0, nshift, _kind = PLANES[name]
    y, P = plane(name)
    Cc = so.tbank(y, P, lead, shift0, nshift)
    Cc.setflags(write=False)
    return Cc


def shape_of(name_or_tuple, **kw):
    t = PLANES[name_or_tuple] if isinstance(name_or_tuple, str) else name_or_tuple
    sh = post.tbank_shape(*t[1:8])
    for k, v in kw.items():
        setattr(sh, k, v)
    return sh


def tbank_call(fn, y_ptr, P_ptr, n, sh, form=_lib.TBANK_PLAN, Cc=None, C_ptr=None):
    """frbch_tbank_host / _device -> (code, message, C, kernel_used)"""
    if Cc is None and C_ptr is None:                               # (a refused shape writes nothing: a few poisoned words do)
        nel = n * sh.nsub * sh.ntemp * sh.nshift
        Cc = np.full(nel if 0 < nel <= 1 << 24 else 16, 0x5A5A5A5A5A5A5A5A, np.int64)
    k = C.c_uint32(99)
    err = C.create_string_buffer(512)
    code = fn(y_ptr, P_ptr, n, C.byref(sh), form, 0, Cc.ctypes.data if C_ptr is None else C_ptr, C.byref(k), err, len(err))
    return code, err.value.decode(), Cc, k.value


def tbank_plan(n, nsub, nbin, K, ntap, lead, shift0, nshift):
    """the fast kernel's plan restated: None = generic, else dict(sw, kr, nkr, lds): 8 shifts a thread, nrun runs rounded up to a
    power of two, sw = min(max(1, 64 / nrunp), 8, nsub rounded up to a power of two) subbands a workgroup, lines of 8 nrun + ntap8
    positions skewed by one word in eight with a stride = 9 nrunp (mod 32), sw halved until one template fits beside the lines in
    64 KiB, the templates in the fewest runs that fit, of equal length"""
    if n > 65535:
        return None
    nrun = -(-nshift // 8)
    nrunp = 1 << (nrun - 1).bit_length()
    ntap8 = (ntap + 7) // 8 * 8
    sw = min(max(1, 64 // nrunp), 8, 1 << (nsub - 1).bit_length())
    lwl = 8 * nrun + ntap8
    lw = lwl + lwl // 8
    while lw % 32 != (9 * nrunp) % 32:
        lw += 1
    while sw > 1 and 16384 - sw * lw < ntap8:
        sw //= 2
    krmax = (16384 - sw * lw) // ntap8
    if krmax < 1:
        return None
    nkr = -(-K // krmax)
    kr = -(-K // nkr)
    return dict(sw=sw, kr=kr, nkr=nkr, lds=(kr * ntap8 + sw * lw) * 4)


# ---- the composite: small files ---------------------------------------------------------------------------------------------
SMALL_BANK = (3, 4, 24, 6, 0.75, math.sqrt(2.0), 0.5, math.sqrt(2.0))
ALPHAS = (0.0, 2.0, 4.0)
# name -> dict(nchan, nrows, nbits, nifs, bursts, nbin, tfactor, ffactor, shift0, nshift; optional: coh, flag, const)
CASES = {
    "u8_64ch_f1": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1, B2], nbin=33, tfactor=3, ffactor=1, shift0=8, nshift=17),
    "u8_64ch_f4_mixed_dms": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1, B2], nbin=33, tfactor=3, ffactor=4, shift0=0, nshift=33),
    "u8_64ch_f64_one_subband": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1], nbin=40, tfactor=2, ffactor=64, shift0=10, nshift=20),
    "u16_128ch_f4_coherency": dict(nchan=128, nrows=4096, nbits=16, nifs=4, coh=True, bursts=[B1, B2], nbin=48, tfactor=2, ffactor=4,
                                   shift0=12, nshift=24),
    "u16_128ch_f1": dict(nchan=128, nrows=4096, nbits=16, nifs=4, bursts=[B1], nbin=33, tfactor=3, ffactor=1, shift0=8, nshift=9),
    # flags 0, 16, 17, 63 and constant columns 5, 40: subband 8 (channels 16, 17) has no used channel; B_OUT is dead altogether
    "u8_64ch_flag_dead_subband": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1, B_OUT, B2], nbin=33, tfactor=3, ffactor=2,
                                      shift0=8, nshift=17, flag=(0, 16, 17, 63), const=(5, 40)),
    # B_EDGE: bins in front of row 0; B_END: behind the last row: incomplete cells, N from the kernel on the 0 / 1 plane
    "u8_64ch_windows_leave_the_file": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B_EDGE, B_END], nbin=256, tfactor=1, ffactor=2,
                                           shift0=0, nshift=256),
}
ALL_COMPLETE = ("u8_64ch_f1", "u8_64ch_f4_mixed_dms", "u8_64ch_f64_one_subband", "u16_128ch_f4_coherency", "u16_128ch_f1")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(hdr, rows, cands, coh, nbin, tfactor, ffactor, shift0, nshift, flag, bank, bp); the arrays are read-only"""
    s = CASES[name]
    nchan, nrows, nbits, nifs, coh = s["nchan"], s["nrows"], s["nbits"], s["nifs"], s.get("coh", False)
    hdr = dict(rc.make_hdr(nchan), nbits=nbits, nifs=nifs, product=0)
    bursts = s["bursts"]
    cands = post.burst_cands([(b["dm"], b["sample"], b["width"]) for b in bursts], 16, 200)
    rows = np.ascontiguousarray(rc.burst_file(hdr, nrows, nbits, bursts, coherency=coh, seed=len(name))[:, :nifs])
    for c in s.get("const", ()):
        rows[:, :, c] = 100
    flag = None
    if s.get("flag"):
        flag = np.zeros(nchan, np.uint8)
        flag[list(s["flag"])] = 1
    for a in (rows, cands, flag):
        if a is not None:
            a.setflags(write=False)
    bank, bp = bank_of(*SMALL_BANK)
    assert_shifts_off_the_ties(hdr, s["ffactor"], ALPHAS, bp["rtau"])
    return dict(hdr=hdr, rows=rows, cands=cands, coh=coh, nbin=s["nbin"], tfactor=s["tfactor"], ffactor=s["ffactor"], shift0=s["shift0"],
                nshift=s["nshift"], flag=flag, bank=bank, bp=bp, alphas=ALPHAS, snr_min=SNR_MIN)


def assert_shifts_off_the_ties(hdr, ffactor, alphas, rtau):
    """no d_s(alpha) of a case may lie within 1e-6 of a half-integer before it is rounded: rint would hang on the last bit of log"""
    nchan = hdr["nchans"]
    nu_ref = hdr["fch1"] + (float(nchan - 1) / 2.0) * hdr["foff"]
    freqs = [hdr["fch1"] + (float(s * ffactor) + float(ffactor - 1) / 2.0) * hdr["foff"] for s in range(nchan // ffactor)]
    for alpha in alphas:
        for d in so.shifts_of(alpha, freqs, nu_ref, rtau):
            assert abs(abs(d - math.floor(d)) - 0.5) > 1e-6, (alpha, d)


@functools.lru_cache(maxsize=None)
def want(name):
    c = case(name)
    out = so.burst_scatter(c["rows"], c["hdr"], c["cands"], c["nbin"], c["tfactor"], c["ffactor"], c["bank"], c["bp"], c["shift0"], c["nshift"],
                           c["alphas"], c["snr_min"], flag=c["flag"], coherency=c["coh"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


FIELDS = ("Y", "yhits", "y", "C", "N", "sub", "band", "used")


def differing(got, exp):
    """the outputs that are not the expected bytes"""
    return [f for f in FIELDS if np.ascontiguousarray(got[f]).tobytes() != np.ascontiguousarray(exp[f]).tobytes()]


def par_of(c, **kw):
    p = post.scat_params(c["nbin"], c["tfactor"], c["ffactor"], c["shift0"], c["nshift"])
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def fit_par_of(c, **kw):
    p = post.scat_fit_params(c["alphas"], c["snr_min"])
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def outputs(ncand, nsub, nbin, K, nshift, nchan, fill=0):
    out = dict(Y=np.zeros((ncand, nsub, nbin), np.int64), yhits=np.zeros((ncand, nsub, nbin), np.uint32), y=np.zeros((ncand, nsub, nbin), np.int32),
               C=np.zeros((ncand, nsub, K, nshift), np.int64), N=np.zeros((ncand, nsub, K, nshift), np.int64),
               sub=np.zeros((ncand, nsub), dtype=post.SCAT_SUB), band=np.zeros(ncand, dtype=post.SCAT_BAND), used=np.zeros((ncand, nchan), np.uint8))
    if fill:
        for a in out.values():
            a.view(np.uint8).fill(fill)
    return out


def outputs_of(c, fill=0):
    return outputs(c["cands"].size, c["hdr"]["nchans"] // c["ffactor"], c["nbin"], c["bp"]["nsig"] * c["bp"]["ntau"], c["nshift"], c["hdr"]["nchans"], fill)


def call(fn, c, rows_ptr, nrows=None, out=None, par=None, bp=None, fp=None, ncand=None, bpar=None, hdr=None, cands=None):
    """frbch_burstscat_host / _device with the arguments of a case -> (code, message, outputs, kernel_used)"""
    hdr = hdr or c["hdr"]
    cands = c["cands"] if cands is None else cands
    n = cands.size if ncand is None else ncand
    out = out or outputs_of(c)
    k = (C.c_uint32 * 3)(99, 99, 99)
    err = C.create_string_buffer(512)
    code = fn(C.byref(post.fil_desc(hdr, hdr.get("product", 0))), rows_ptr, c["rows"].shape[0] if nrows is None else nrows,
              C.byref(bpar if bpar is not None else rc.burst_par(c["coh"])), cands.ctypes.data, n,
              c["flag"].ctypes.data if c["flag"] is not None else None, C.byref(par if par is not None else par_of(c)),
              C.byref(bp if bp is not None else bank_par(c["bp"])), C.byref(fp if fp is not None else fit_par_of(c)), 0,
              out["Y"].ctypes.data, out["yhits"].ctypes.data, out["y"].ctypes.data, out["C"].ctypes.data, out["N"].ctypes.data,
              out["sub"].ctypes.data, out["band"].ctypes.data, out["used"].ctypes.data, k, err, len(err))
    return code, err.value.decode(), out, (k[0], k[1], k[2])


def query(lib, c, rows_ptr, par=None, bp=None, cands=None, hdr=None):
    """frbch_burstscat_kernel -> (code, the three forms)"""
    cands = c["cands"] if cands is None else cands
    hdr = hdr or c["hdr"]
    k = (C.c_uint32 * 3)(99, 99, 99)
    code = lib.frbch_burstscat_kernel(C.byref(post.fil_desc(hdr, hdr.get("product", 0))), rows_ptr, c["rows"].shape[0], C.byref(rc.burst_par(c["coh"])),
                                      cands.ctypes.data, cands.size, C.byref(par if par is not None else par_of(c)),
                                      C.byref(bp if bp is not None else bank_par(c["bp"])), k)
    return code, (k[0], k[1], k[2])


def dyn_plan_expected(c, aligned):
    """the dynamic-spectrum kernel of a case: acf_cases' rule on the same grid"""
    return ac.dyn_plan_expected(dict(c, nlagf=1, nlagt=1), aligned)


def acf_of(lib, c):
    """frbch_burstacf_host on the same arguments (one lag): its Y and yhits"""
    return post.burst_acf(c["rows"], c["hdr"], c["cands"], c["nbin"], c["tfactor"], c["ffactor"], 1, 1, flag=c["flag"],
                          products="coherency" if c["coh"] else "stokes", lib=lib)


# ---- known answers: a noise-free plane -----------------------------------------------------------------------------------
NF_BANK = (6, 10, 96, 16, 0.75, math.sqrt(2.0), 0.5, math.sqrt(2.0))
NF_NBIN, NF_SHIFT0, NF_NSHIFT, NF_ARRIVALS, NF_AMP = 128, 32, 64, (32, 61, 95), 37


def noise_free_plane(k, t0):
    """37 times template k with its Gaussian centre on bin t0, truncated by the window -> int32 [1][1][NF_NBIN]"""
    bank, bp = bank_of(*NF_BANK)
    y = np.zeros((1, 1, NF_NBIN), np.int32)
    j0 = t0 - bp["lead"]
    lo, hi = max(0, -j0), min(bp["ntap"], NF_NBIN - j0)
    y[0, 0, j0 + lo:j0 + hi] = NF_AMP * bank["p"][k, lo:hi]
    return y


# ---- known answers: a scattered burst through filterbank rows -----------------------------------------------------------
KNOWN_DM, KNOWN_SAMPLE = 350.37, 1100
KNOWN_SIGMA, KNOWN_TAU_REF, KNOWN_ALPHA, KNOWN_AMP = 2.0, 6.0, 4.0, 500.0      # rows, rows at the band's centre, -, fluence per channel in codes x rows
KNOWN_BANK = (4, 48, 128, 24, 1.0, math.sqrt(2.0), 0.5, 2.0 ** 0.125)
KNOWN_GRID = dict(nbin=256, tfactor=1, ffactor=8, shift0=96, nshift=64)
KNOWN_ALPHAS = (0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0)
KNOWN_SEEDS = tuple(range(12))


def known_hdr():
    return dc.known_hdr()


def known_cands():
    cands = post.burst_cands([(KNOWN_DM, KNOWN_SAMPLE, 8)], 400, 400)
    cands.setflags(write=False)
    return cands


@functools.lru_cache(maxsize=None)
def known_rows(seed, scattered=True):
    """64 channels at 1.2 - 1.5 GHz, 64 us rows, 8-bit rows of noise 96 +- 12 at DM 350.37; a Gaussian of sigma 2 rows and fluence
    KNOWN_AMP, convolved per channel with exp(-t / tau_c) / tau_c, tau_c = 6 rows (nu_c / nu_ref)^-4 (`scattered`), or left as it is"""
    hdr = known_hdr()
    nrows, nchan = 7680, 64
    rng = np.random.default_rng(5300 + seed)
    x = 96.0 + 12.0 * rng.standard_normal((nrows, 1, nchan))
    d = do.delays(hdr, KNOWN_DM)
    t = np.arange(nrows, dtype=np.float64)
    fc = hdr["fch1"] + np.arange(nchan) * hdr["foff"]
    nu_ref = hdr["fch1"] + (nchan - 1) / 2.0 * hdr["foff"]
    for ch in range(nchan):
        g = np.exp(-0.5 * ((t - (KNOWN_SAMPLE + d[ch])) / KNOWN_SIGMA) ** 2) / (KNOWN_SIGMA * math.sqrt(2.0 * math.pi))
        if scattered:
            tau = KNOWN_TAU_REF * (fc[ch] / nu_ref) ** (-KNOWN_ALPHA)
            e = np.exp(-np.arange(0, int(20 * tau) + 1) / tau)
            g = np.convolve(g, e / e.sum())[:nrows]
        x[:, 0, ch] += KNOWN_AMP * g
    rows = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def known_oracle(seed, scattered=True):
    g = KNOWN_GRID
    bank, bp = bank_of(*KNOWN_BANK)
    assert_shifts_off_the_ties(known_hdr(), g["ffactor"], KNOWN_ALPHAS, bp["rtau"])
    return so.burst_scatter(known_rows(seed, scattered), known_hdr(), known_cands(), g["nbin"], g["tfactor"], g["ffactor"], bank, bp, g["shift0"],
                            g["nshift"], KNOWN_ALPHAS, SNR_MIN)


def known_call(lib, seed, scattered=True, info=None):
    g = KNOWN_GRID
    _bank, bp = bank_of(*KNOWN_BANK)
    return post.burst_scatter(known_rows(seed, scattered), known_hdr(), known_cands(), bank=bank_par(bp), alphas=KNOWN_ALPHAS, snr_min=SNR_MIN,
                              lib=lib, info=info, **g)
