"""Shared case builder of the burst-structure tests (tests/test_acf.py on the emulator, tests/test_gpu_acf.py on the device): small
files built from a formula with the grids that reach every branch of frbch_burstacf_* -- the smallest shapes at which the kernels
can still go wrong --, planes from a formula for the ACF stage alone (frbch_acf2d_*), the plan rules of the two fast kernels
restated, a file at the bound of the quantisation, and bursts of known drift and known decorrelation scale.  Expected values are
tests/acf_oracle.py's, computed once per case and shared (read-only)."""
import ctypes as C
import functools
import math

import numpy as np

from frb_baseband_amd import _lib, post
from tests import acf_oracle as ao
from tests import dmscan_cases as dc
from tests import dmscan_oracle as do
from tests import rm_cases as rc

B1, B2, B_EDGE, B_OUT, B_END, B_WIDE = rc.B1, rc.B2, rc.B_EDGE, rc.B_OUT, dc.B_END, dc.B_WIDE
FIT_FRAC = 0.5

# name -> dict(nchan, nrows, nbits, nifs, bursts, nbin, tfactor, ffactor, nlagf, nlagt; optional: coh, sign, product, flag, const, kind, bw, gap)
CASES = {
    "u8_64ch_f1_full_lags": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1, B2], nbin=33, tfactor=3, ffactor=1, nlagf=64, nlagt=33),
    "u8_64ch_f4_full_lags": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1, B2], nbin=33, tfactor=3, ffactor=4, nlagf=16, nlagt=33),
    "u8_64ch_1x1x1": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1], nbin=1, tfactor=1, ffactor=64, nlagf=1, nlagt=1),
    "u8_64ch_one_subband": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1, B2], nbin=40, tfactor=2, ffactor=64, nlagf=1, nlagt=20),
    "u8_64ch_windows_leave_the_file": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B_EDGE, B_END], nbin=256, tfactor=1, ffactor=2,
                                           nlagf=8, nlagt=16),
    # flags 0, 16, 17, 63 and constant columns 5, 40: subband 8 (channels 16, 17) has no used channel; B_OUT is dead altogether
    "u8_64ch_flag_constant_dead": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1, B_OUT, B2], nbin=33, tfactor=3, ffactor=2,
                                       nlagf=8, nlagt=8, flag=(0, 16, 17, 63), const=(5, 40)),
    "u16_64ch_coherency": dict(nchan=64, nrows=4096, nbits=16, nifs=4, coh=True, bursts=[B1, B2, B_EDGE], nbin=65, tfactor=2, ffactor=2,
                               nlagf=6, nlagt=9),
    "u8_96ch_ascending": dict(nchan=96, nrows=4096, nbits=8, nifs=4, sign=1, bursts=[B1, B2, B_OUT], nbin=33, tfactor=3, ffactor=3, nlagf=5, nlagt=7),
    "u8_64ch_one_product": dict(nchan=64, nrows=4096, nbits=8, nifs=1, bursts=[B1, B2], nbin=40, tfactor=2, ffactor=1, nlagf=4, nlagt=5),
    "u8_64ch_product2": dict(nchan=64, nrows=4096, nbits=8, nifs=4, product=2, bursts=[B1], nbin=40, tfactor=2, ffactor=8, nlagf=8, nlagt=5),
    "u8_192ch_f3_generic": dict(nchan=192, nrows=4096, nbits=8, nifs=4, bursts=[B1, B2], nbin=20, tfactor=2, ffactor=3, nlagf=9, nlagt=4),
    "u8_192ch_f192_join": dict(nchan=192, nrows=4096, nbits=8, nifs=4, bursts=[B1, B_EDGE], nbin=70, tfactor=2, ffactor=192, nlagf=1, nlagt=12),
    "u8_256ch_f128_join": dict(nchan=256, nrows=4096, nbits=8, nifs=1, bursts=[B1, B2], nbin=24, tfactor=3, ffactor=128, nlagf=2, nlagt=6),
    # 1024 channels over 256 MHz: the delay spread of the lowest 64-byte tile at DM 700 is 898 rows
    "u8_1024ch_edge_fits": dict(nchan=1024, nrows=12288, nbits=8, nifs=1, bw=256.0, bursts=[B_WIDE], nbin=6, tfactor="edge", ffactor=8,
                                nlagf=4, nlagt=3, kind="plain"),
    "u8_1024ch_edge_one_more": dict(nchan=1024, nrows=12288, nbits=8, nifs=1, bw=256.0, bursts=[B_WIDE], nbin=6, tfactor="edge+1", ffactor=8,
                                    nlagf=4, nlagt=3, kind="plain"),
    # 2^20 cells, every one at the same large Y: |y| between 2^20 and 2^21, A[0][0] above 2^60
    "u8_1024ch_full_scale": dict(nchan=1024, nrows=2600, nbits=8, nifs=1, bw=256.0, bursts=[dict(dm=0.002, sample=1000, width=32)], nbin=1024,
                                 tfactor=1, ffactor=1, nlagf=2, nlagt=2, kind="full", gap=(600, 300)),
}
# the dynamic-spectrum kernel that must run at the aligned address (the plan rule restated below decides the rest)
DYN_FAST = ("u8_64ch_f1_full_lags", "u8_64ch_f4_full_lags", "u8_64ch_1x1x1", "u8_64ch_one_subband", "u8_64ch_windows_leave_the_file",
            "u8_64ch_flag_constant_dead", "u16_64ch_coherency", "u8_64ch_one_product", "u8_64ch_product2", "u8_192ch_f192_join",
            "u8_256ch_f128_join", "u8_1024ch_edge_fits", "u8_1024ch_full_scale")
DYN_GENERIC = ("u8_96ch_ascending", "u8_192ch_f3_generic", "u8_1024ch_edge_one_more")
STAGE_BYTES, MAX_TFACTOR = 65536, 256


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(hdr, rows, cands, coh, nbin, tfactor, ffactor, nlagf, nlagt, flag, fit_frac); the arrays are read-only"""
    s = CASES[name]
    nchan, nrows, nbits, nifs, coh = s["nchan"], s["nrows"], s["nbits"], s["nifs"], s.get("coh", False)
    hdr = dict(rc.make_hdr(nchan, foff_sign=s.get("sign", -1), bw=s.get("bw", 32.0)), nbits=nbits, nifs=nifs, product=s.get("product", 0))
    bursts, kind = s["bursts"], s.get("kind", "stokes")
    gap, length = s.get("gap", (16, 300) if nchan >= 1024 else (16, 200))
    cands = post.burst_cands([(b["dm"], b["sample"], b["width"]) for b in bursts], gap, length)
    tfactor = s["tfactor"]
    if isinstance(tfactor, str):                                   # the plan edge: the rows of a tile exactly the stage, or one more
        tfactor = STAGE_BYTES // 64 - dc.tile_range(hdr, nbits // 8, cands, 1, 0.0, 1) + (1 if tfactor.endswith("+1") else 0)
    if kind == "plain":
        rows = dc.plain_file(hdr, nrows, nbits, nifs, bursts, seed=len(name))
    elif kind == "full":
        rows = dc.full_scale_file(hdr, nrows, bursts[0], s["nbin"], tfactor)
    else:
        rows = np.ascontiguousarray(rc.burst_file(hdr, nrows, nbits, bursts, coherency=coh, seed=len(name))[:, :nifs])
    for c in s.get("const", ()):
        rows[:, :, c] = 100                                        # a constant column: var_off = 0
    flag = None
    if s.get("flag"):
        flag = np.zeros(nchan, np.uint8)
        flag[list(s["flag"])] = 1
    for a in (rows, cands, flag):
        if a is not None:
            a.setflags(write=False)
    return dict(hdr=hdr, rows=rows, cands=cands, coh=coh, nbin=s["nbin"], tfactor=tfactor, ffactor=s["ffactor"], nlagf=s["nlagf"],
                nlagt=s["nlagt"], flag=flag, fit_frac=FIT_FRAC)


@functools.lru_cache(maxsize=None)
def want(name):
    c = case(name)
    out = ao.burst_acf(c["rows"], c["hdr"], c["cands"], c["nbin"], c["tfactor"], c["ffactor"], c["nlagf"], c["nlagt"], c["fit_frac"],
                       flag=c["flag"], coherency=c["coh"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


FIELDS = ("Y", "yhits", "A", "P", "results", "used")


def differing(got, exp):
    """the outputs that are not the expected bytes"""
    return [f for f in FIELDS if np.ascontiguousarray(got[f]).tobytes() != np.ascontiguousarray(exp[f]).tobytes()]


# ---- the plan rules, restated ------------------------------------------------------------------------------------------
def dyn_plan_expected(c, aligned):
    """the dynamic-spectrum kernel: the layout of the fast burst-sums kernel, bins of at most 256 rows, an ffactor that is a power
    of two within the 64 / 32 channels of a 64-byte tile or a multiple of them, and room for one bin beside the delay range of
    every tile in 64 KiB of 64-byte rows per product read"""
    itemsize, nchan, ff = c["rows"].dtype.itemsize, c["hdr"]["nchans"], c["ffactor"]
    ct = 64 // itemsize
    if (nchan * itemsize) % 64 or not aligned or c["tfactor"] > MAX_TFACTOR:
        return 0
    if not ((ff & (ff - 1)) == 0 and ff <= ct) and not (ff > ct and ff % ct == 0):
        return 0
    cap = STAGE_BYTES // (64 * (2 if c["coh"] else 1))
    return int(c["tfactor"] + dc.tile_range(c["hdr"], itemsize, c["cands"], 1, 0.0, 1) <= cap)


def acf_plan(n, nsub, nbin, nlagf, nlagt):
    """the ACF kernel: None = generic, else dict(sb, dfr, nslab): 8 time lags a thread, nrun runs rounded up to a power of two,
    dfr = min(256 / nrunp, 8, nlagf rounded up to a power of two) frequency lags a workgroup, b lines of nbin8 + 8 nrun positions
    skewed by one word in eight with a stride = 9 nrunp (mod 32), the largest slab that fits 64 KiB, partials within 2^30 bytes"""
    ndt = 2 * nlagt - 1
    nrun = -(-ndt // 8)
    nrunp = 1 << (nrun - 1).bit_length()
    dfr = min(256 // nrunp, 8, 1 << (nlagf - 1).bit_length())
    nbin8 = (nbin + 7) // 8 * 8
    bwl = nbin8 + 8 * nrun
    bw = bwl + bwl // 8
    while bw % 32 != (9 * nrunp) % 32:
        bw += 1
    sb = (16384 - (dfr - 1) * bw) // (nbin8 + bw)
    if sb < 1 or n > 65535:
        return None
    sb = min(sb, nsub)
    nslab = -(-nsub // sb)
    if n * nslab * nlagf * ndt * 8 > 1 << 30:
        return None
    return dict(sb=sb, dfr=dfr, nslab=nslab)


# ---- the calls -------------------------------------------------------------------------------------------------------
def par_of(c, **kw):
    p = post.acf_params(c["nbin"], c["tfactor"], c["ffactor"], c["nlagf"], c["nlagt"])
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def fit_par_of(c, **kw):
    p = post.acf_fit_params(c["fit_frac"])
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def outputs(ncand, nsub, nbin, nlagf, nlagt, nchan, fill=0):
    out = dict(Y=np.zeros((ncand, nsub, nbin), np.int64), yhits=np.zeros((ncand, nsub, nbin), np.uint32),
               A=np.zeros((ncand, nlagf, 2 * nlagt - 1), np.int64), P=np.zeros((ncand, nlagf, 2 * nlagt - 1), np.uint32),
               results=np.zeros(ncand, dtype=post.ACF_RESULT), used=np.zeros((ncand, nchan), np.uint8))
    if fill:
        for a in out.values():
            a.view(np.uint8).fill(fill)
    return out


def outputs_of(c, fill=0):
    return outputs(c["cands"].size, c["hdr"]["nchans"] // c["ffactor"], c["nbin"], c["nlagf"], c["nlagt"], c["hdr"]["nchans"], fill)


def call(fn, c, rows_ptr, nrows=None, out=None, par=None, fp=None, ncand=None, bpar=None, hdr=None, cands=None):
    """frbch_burstacf_host / _device with the arguments of a case -> (code, message, outputs, kernel_used)"""
    hdr = hdr or c["hdr"]
    cands = c["cands"] if cands is None else cands
    n = cands.size if ncand is None else ncand
    out = out or outputs_of(c)
    k = (C.c_uint32 * 3)(99, 99, 99)
    err = C.create_string_buffer(512)
    code = fn(C.byref(post.fil_desc(hdr, hdr.get("product", 0))), rows_ptr, c["rows"].shape[0] if nrows is None else nrows,
              C.byref(bpar if bpar is not None else rc.burst_par(c["coh"])), cands.ctypes.data, n,
              c["flag"].ctypes.data if c["flag"] is not None else None, C.byref(par if par is not None else par_of(c)),
              C.byref(fp if fp is not None else fit_par_of(c)), 0, out["Y"].ctypes.data, out["yhits"].ctypes.data, out["A"].ctypes.data,
              out["P"].ctypes.data, out["results"].ctypes.data, out["used"].ctypes.data, k, err, len(err))
    return code, err.value.decode(), out, (k[0], k[1], k[2])


def query(lib, c, rows_ptr, par=None, cands=None, hdr=None):
    """frbch_burstacf_kernel -> (code, the three forms)"""
    cands = c["cands"] if cands is None else cands
    hdr = hdr or c["hdr"]
    k = (C.c_uint32 * 3)(99, 99, 99)
    code = lib.frbch_burstacf_kernel(C.byref(post.fil_desc(hdr, hdr.get("product", 0))), rows_ptr, c["rows"].shape[0], C.byref(rc.burst_par(c["coh"])),
                                     cands.ctypes.data, cands.size, C.byref(par if par is not None else par_of(c)), k)
    return code, (k[0], k[1], k[2])


def dmscan_band_sums(lib, c):
    """acc[i][0][j], hits[i][0][j] of frbch_dmscan_host at ntrial = 1 on the arguments of a case, through the library"""
    got = post.dm_scan(c["rows"], c["hdr"], c["cands"], 1, 0.0, c["nbin"], c["tfactor"], widths=(1,), smooth=1, flag=c["flag"],
                       products="coherency" if c["coh"] else "stokes", lib=lib)
    return got["acc"][:, 0, :], got["hits"][:, 0, :]


# ---- the ACF stage alone: planes from a formula ------------------------------------------------------------------------
Y_MAX = 1 << 21
EDGE = dict(nbin=64, nlagf=8, nlagt=16)               # the slab of this geometry is 78 rows; one bin more makes it 75
# name -> (n, nsub, nbin, nlagf, nlagt, kind)
PLANES = {
    "random_3x5_full_lags": (2, 3, 5, 3, 5, "random"),
    "random_64x33_full_lags": (1, 64, 33, 64, 33, "random"),
    "random_1x1": (3, 1, 1, 1, 1, "random"),
    "plus_full_scale_1024x1024": (1, 1024, 1024, 2, 2, "plus"),
    "alternating_full_scale_1024x1024": (1, 1024, 1024, 2, 2, "alternating"),
    "zero_one_40x50": (2, 40, 50, 7, 9, "01"),
    "nlagt_256_of_256_bins": (1, 3, 256, 3, 256, "random"),
    "nlagf_is_nsub": (1, 20, 16, 20, 4, "random"),
    "several_slabs_ragged": (2, 230, 50, 11, 10, "random"),
    "edge_one_slab": (1, 78, 64, 8, 16, "random"),
    "edge_one_row_more": (1, 79, 64, 8, 16, "random"),
    "edge_one_bin_more": (1, 78, 65, 8, 16, "random"),
}


@functools.lru_cache(maxsize=None)
def plane(name):
    n, nsub, nbin, _lf, _lt, kind = PLANES[name]
    if kind == "random":
        y = np.random.default_rng(9100 + len(name)).integers(-Y_MAX, Y_MAX + 1, size=(n, nsub, nbin)).astype(np.int32)
        y.reshape(-1)[0] = Y_MAX
        y.reshape(-1)[-1] = -Y_MAX
    elif kind == "plus":
        y = np.full((n, nsub, nbin), Y_MAX, np.int32)
    elif kind == "alternating":
        y = np.where((np.arange(nsub)[:, None] + np.arange(nbin)[None, :]) % 2 == 0, Y_MAX, -Y_MAX).astype(np.int32)[None].repeat(n, axis=0)
    else:
        y = np.random.default_rng(9200).integers(0, 2, size=(n, nsub, nbin)).astype(np.int32)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def plane_want(name):
    _n, _nsub, _nbin, lf, lt, _kind = PLANES[name]
    A = ao.acf2d_planes(plane(name), lf, lt)
    A.setflags(write=False)
    return A


def acf2d_call(fn, y_ptr, shape, lf, lt, form=_lib.ACF_PLAN, A=None, A_ptr=None):
    """frbch_acf2d_host / _device -> (code, message, A, kernel_used)"""
    n, nsub, nbin = shape
    if A is None and A_ptr is None:
        A = np.full((n, max(lf, 1), 2 * max(lt, 1) - 1), 0x5A5A5A5A5A5A5A5A, np.int64)
    k = C.c_uint32(99)
    err = C.create_string_buffer(512)
    code = fn(y_ptr, n, nsub, nbin, lf, lt, form, 0, A.ctypes.data if A_ptr is None else A_ptr, C.byref(k), err, len(err))
    return code, err.value.decode(), A, k.value


# ---- bursts of known drift and of known decorrelation scale ------------------------------------------------------------
KNOWN_DM, KNOWN_SAMPLE, KNOWN_SEED = 350.37, 1100, 3
KNOWN_GRID = dict(nbin=128, tfactor=4, ffactor=1, nlagf=32, nlagt=64)
KNOWN_FIT_FRAC = 0.25
DRIFT = -20.0                                           # MHz / ms: later sub-bursts at lower frequencies
SUB_F, SUB_SIGMA_F, SUB_SIGMA_T = (1425.0, 1350.0, 1275.0), 15.0, 12.0      # centres and sigma in MHz; sigma in rows
SCINT_CHANS, SCINT_SIGMA, SCINT_SIGMA_T = (8, 24, 41, 57), 2.0, 12.0        # scintle centres and sigma in channels; sigma in rows


def known_hdr():
    return dc.known_hdr()


def known_cands():
    cands = post.burst_cands([(KNOWN_DM, KNOWN_SAMPLE, 8)], 400, 400)
    cands.setflags(write=False)
    return cands


@functools.lru_cache(maxsize=None)
def known_rows(seed, kind):
    """64 channels at 1.2 - 1.5 GHz, 64 us rows, 8-bit rows of noise 96 +- 12 at DM 350.37.  'drift': three sub-bursts, Gaussian in
    frequency and time, whose centre times step with their centre frequencies at DRIFT; 'control': the same three at one time;
    'scint': one component whose spectrum is four Gaussian scintles"""
    hdr = known_hdr()
    nrows, nchan = 7680, 64
    rng = np.random.default_rng(4300 + seed)
    x = 96.0 + 12.0 * rng.standard_normal((nrows, 1, nchan))
    d = do.delays(hdr, KNOWN_DM)
    t = np.arange(nrows, dtype=np.float64)
    fc = hdr["fch1"] + np.arange(nchan) * hdr["foff"]
    for ch in range(nchan):
        if kind == "scint":
            g = sum(math.exp(-0.5 * ((ch - s) / SCINT_SIGMA) ** 2) for s in SCINT_CHANS)
            x[:, 0, ch] += 40.0 * g * np.exp(-0.5 * ((t - (KNOWN_SAMPLE + d[ch])) / SCINT_SIGMA_T) ** 2)
            continue
        for f0 in SUB_F:
            late = 0.0 if kind == "control" else ((f0 - SUB_F[1]) / DRIFT) * 1e-3 / hdr["tsamp"]          # rows
            g = math.exp(-0.5 * ((fc[ch] - f0) / SUB_SIGMA_F) ** 2)
            x[:, 0, ch] += 30.0 * g * np.exp(-0.5 * ((t - (KNOWN_SAMPLE + late + d[ch])) / SUB_SIGMA_T) ** 2)
    rows = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def known_oracle(seed, kind):
    g = KNOWN_GRID
    return ao.burst_acf(known_rows(seed, kind), known_hdr(), known_cands(), g["nbin"], g["tfactor"], g["ffactor"], g["nlagf"], g["nlagt"],
                        KNOWN_FIT_FRAC)


def known_expected():
    """what the rule of the header gives on the noise-free ACFs: the half-width from F[1] / 2 of a Gaussian ACF of sigma s sqrt 2 is
    sqrt(4 s^2 ln 2 + 1) lags -> (dt_df ms per MHz, frequency half-width MHz of 'scint', time half-width ms of 'scint')"""
    hdr = known_hdr()
    wf = math.sqrt(4.0 * SCINT_SIGMA ** 2 * math.log(2.0) + 1.0) * abs(hdr["foff"])
    st = SCINT_SIGMA_T / KNOWN_GRID["tfactor"]
    wt = math.sqrt(4.0 * st ** 2 * math.log(2.0) + 1.0) * KNOWN_GRID["tfactor"] * hdr["tsamp"] * 1e3
    return 1.0 / DRIFT, wf, wt
