"""Shared case builder of the DM scan tests (tests/test_dmscan.py on the emulator, tests/test_gpu_dmscan.py on the device): small
files built from a formula with the scan grids that reach every branch of frbch_dmscan_* -- the smallest shapes at which the
kernels can still go wrong --, the plan edge of the fast kernel, a file at the bound of the fixed-point scale, and the bursts of
known DM.  Expected values are tests/dmscan_oracle.py's, computed once per case and shared (read-only)."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import _lib, post
from tests import dmscan_oracle as do
from tests import rm_cases as rc

B1, B2, B_EDGE, B_OUT = rc.B1, rc.B2, rc.B_EDGE, rc.B_OUT
B_END = dict(dm=56.7, sample=4070, width=6, rm=0.0, pa0=0.0, lin=0.0, circ=0.0)          # the bins run off the end of the file
B_MID = dict(dm=56.7, sample=4000, width=6, rm=0.0, pa0=0.0, lin=0.0, circ=0.0)          # of the 8192-row file
B_WIDE = dict(dm=700.0, sample=600, width=8)                                             # of the 1024-channel, 256 MHz file

WIDTHS, SMOOTH, FIT_FRAC = (1, 2, 4, 8), 3, 0.5

# name -> dict(nchan, nrows, nbits, nifs, coh, sign, bursts, ntrial, ddm, nbin, tfactor; optional: product, flag, const, kind, widths)
CASES = {
    "u8_64ch_33x33x3": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1, B_OUT, B2], ntrial=33, ddm=0.2, nbin=33, tfactor=3),
    "u8_64ch_1x1x1": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1], ntrial=1, ddm=0.0, nbin=1, tfactor=1, widths=(1,)),
    "u8_64ch_windows_leave_the_file": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B_EDGE, B_END], ntrial=17, ddm=0.5, nbin=256, tfactor=1),
    "u8_64ch_4096x2": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1], ntrial=4096, ddm=0.01, nbin=2, tfactor=4, widths=(1, 2), smooth=1),
    "u8_64ch_3x1024": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1, B_EDGE], ntrial=3, ddm=0.7, nbin=1024, tfactor=1),
    "u8_64ch_tfactor512": dict(nchan=64, nrows=8192, nbits=8, nifs=4, bursts=[B_MID], ntrial=5, ddm=0.7, nbin=4, tfactor=512, widths=(1, 2)),
    "u16_64ch_coherency": dict(nchan=64, nrows=4096, nbits=16, nifs=4, coh=True, bursts=[B1, B2, B_EDGE], ntrial=33, ddm=0.2, nbin=65, tfactor=2),
    "u8_64ch_one_product": dict(nchan=64, nrows=4096, nbits=8, nifs=1, bursts=[B1, B2], ntrial=9, ddm=0.3, nbin=40, tfactor=2),
    "u8_64ch_product2": dict(nchan=64, nrows=4096, nbits=8, nifs=4, product=2, bursts=[B1], ntrial=9, ddm=0.3, nbin=40, tfactor=2),
    "u8_96ch_ascending": dict(nchan=96, nrows=4096, nbits=8, nifs=4, sign=1, bursts=[B1, B2, B_OUT], ntrial=33, ddm=0.2, nbin=33, tfactor=3),
    "u8_64ch_flag_constant_dead": dict(nchan=64, nrows=4096, nbits=8, nifs=4, bursts=[B1, B_OUT, B2], ntrial=17, ddm=0.2, nbin=33, tfactor=3,
                                       flag=(0, 17, 63), const=(5, 40)),
    # 1024 channels over 256 MHz: the delay spread of the lowest 64-byte tile at DM 700 is 898 rows
    "u8_1024ch_spread_exceeds_the_stage": dict(nchan=1024, nrows=12288, nbits=8, nifs=1, bw=256.0, bursts=[B_WIDE], ntrial=3, ddm=0.05, nbin=6,
                                               tfactor=200, kind="plain", widths=(1, 2, 4)),
    "u8_1024ch_edge_fits": dict(nchan=1024, nrows=12288, nbits=8, nifs=1, bw=256.0, bursts=[B_WIDE], ntrial=3, ddm=0.05, nbin=6, tfactor="edge",
                                kind="plain", widths=(1, 2, 4)),
    "u8_1024ch_edge_one_more": dict(nchan=1024, nrows=12288, nbits=8, nifs=1, bw=256.0, bursts=[B_WIDE], ntrial=3, ddm=0.05, nbin=6,
                                    tfactor="edge+1", kind="plain", widths=(1, 2, 4)),
    "u8_4096ch_full_scale": dict(nchan=4096, nrows=600, nbits=8, nifs=1, bw=256.0, bursts=[dict(dm=0.002, sample=300, width=32)], ntrial=3, ddm=0.001,
                                 nbin=4, tfactor=8, kind="full", widths=(1, 2)),
}
# what must run in which form at the aligned address (the plan rule restated in tests/test_gpu_dmscan.py decides the rest)
MUST_RUN_FAST = ("u8_64ch_33x33x3", "u8_64ch_1x1x1", "u8_64ch_windows_leave_the_file", "u8_64ch_4096x2", "u8_64ch_3x1024", "u16_64ch_coherency",
                 "u8_64ch_one_product", "u8_64ch_product2", "u8_64ch_flag_constant_dead", "u8_1024ch_edge_fits", "u8_4096ch_full_scale")
MUST_RUN_GENERIC = ("u8_64ch_tfactor512", "u8_96ch_ascending", "u8_1024ch_spread_exceeds_the_stage", "u8_1024ch_edge_one_more")
STAGE_BYTES, TRUN, MAX_TFACTOR = 65536, 16, 256


def plain_file(hdr, nrows, nbits, nifs, bursts, seed, amp=40):
    """rows [nrows][nifs][nchan] made in their own type: uniform integer noise of 94 .. 106 and `amp` on the on-pulse rows of every
    burst at its delays, the same in every product"""
    nchan = hdr["nchans"]
    rng = np.random.default_rng(7100 + seed)
    x = rng.integers(94, 107, size=(nrows, nifs, nchan), dtype=np.uint8 if nbits == 8 else np.uint16)
    chans = np.arange(nchan)
    for b in bursts:
        d = do.delays(hdr, b["dm"])
        on_lo = b["sample"] - b["width"] // 2
        for t in range(on_lo, on_lo + b["width"]):
            r = t + d
            ok = (r >= 0) & (r < nrows)
            for p in range(nifs):
                x[r[ok], p, chans[ok]] += amp
    return x if nbits == 8 else x * 200


def full_scale_file(hdr, nrows, cand, nbin, tfactor):
    """8-bit rows of 0, 1, 0, 1 .. (the same in every channel: an off-pulse variance of about 1 / 4) with 255 on every row of the
    window of the bins: every term is full scale over its baseline, with one sign"""
    x = np.zeros((nrows, 1, hdr["nchans"]), np.uint8)
    x[1::2] = 1
    t0 = cand["sample"] - (nbin // 2) * tfactor
    x[t0:t0 + nbin * tfactor] = 255
    return x


def tile_range(hdr, itemsize, cands, ntrial, ddm, trun):
    """the largest delay range of any (candidate, 64-byte tile, run of `trun` trials)"""
    ct = 64 // itemsize
    worst = 0
    for cd in cands:
        dms = do.trial_dms(cd["dm"], ntrial, ddm)
        d = np.stack([do.delays(hdr, dm) for dm in dms]).reshape(ntrial, -1, ct)
        for k0 in range(0, ntrial, trun):
            run = d[k0:k0 + trun]
            worst = max(worst, int((run.max(axis=(0, 2)) - run.min(axis=(0, 2))).max()))
    return worst


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(hdr, rows, cands, coh, ntrial, ddm, nbin, tfactor, flag, widths, smooth, fit_frac); the arrays are read-only"""
    s = CASES[name]
    nchan, nrows, nbits, nifs, coh = s["nchan"], s["nrows"], s["nbits"], s["nifs"], s.get("coh", False)
    hdr = dict(rc.make_hdr(nchan, foff_sign=s.get("sign", -1), bw=s.get("bw", 32.0)), nbits=nbits, nifs=nifs, product=s.get("product", 0))
    bursts, kind = s["bursts"], s.get("kind", "stokes")
    gap, length = (16, 300) if nchan >= 1024 else (16, 200)
    cands = post.burst_cands([(b["dm"], b["sample"], b["width"]) for b in bursts], gap, length)
    tfactor = s["tfactor"]
    if isinstance(tfactor, str):                                   # the plan edge: the rows of a (tile, run of one trial) exactly the stage, or one more
        tfactor = STAGE_BYTES // 64 - tile_range(hdr, nbits // 8, cands, s["ntrial"], s["ddm"], 1) + (1 if tfactor.endswith("+1") else 0)
    if kind == "plain":
        rows = plain_file(hdr, nrows, nbits, nifs, bursts, seed=len(name))
    elif kind == "full":
        rows = full_scale_file(hdr, nrows, bursts[0], s["nbin"], tfactor)
    else:
        rows = rc.burst_file(hdr, nrows, nbits, bursts, coherency=coh, seed=len(name))[:, :nifs]
        rows = np.ascontiguousarray(rows)
    for c in s.get("const", ()):
        rows[:, :, c] = 100                                        # a constant column: var_off = 0
    flag = None
    if s.get("flag"):
        flag = np.zeros(nchan, np.uint8)
        flag[list(s["flag"])] = 1
    for a in (rows, cands, flag):
        if a is not None:
            a.setflags(write=False)
    return dict(hdr=hdr, rows=rows, cands=cands, coh=coh, ntrial=s["ntrial"], ddm=s["ddm"], nbin=s["nbin"], tfactor=tfactor, flag=flag,
                widths=tuple(s.get("widths", WIDTHS)), smooth=s.get("smooth", SMOOTH), fit_frac=FIT_FRAC)


def oracle_kw(c):
    return dict(widths=c["widths"], smooth=c["smooth"], fit_frac=c["fit_frac"], flag=c["flag"], coherency=c["coh"])


@functools.lru_cache(maxsize=None)
def want(name):
    c = case(name)
    out = do.scan(c["rows"], c["hdr"], c["cands"], c["ntrial"], c["ddm"], c["nbin"], c["tfactor"], unbounded=name == "u8_4096ch_full_scale",
                  fp64=True, **oracle_kw(c))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


FIELDS = ("acc", "hits", "snr", "struct", "results", "used")


def same(got, exp):
    """every output byte for byte"""
    return all(np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(exp[f]).tobytes() for f in FIELDS)


def plan_expected(c, aligned):
    """the plan rule, restated: the layout of the fast burst-sums kernel, bins of at most 256 rows, the largest trial run of 16,
    8, 4, 2, 1 within ntrial whose delay range leaves room for one bin in 64 KiB of 64-byte rows per product read, and partials
    of at most 2^30 bytes"""
    itemsize, nchan = c["rows"].dtype.itemsize, c["hdr"]["nchans"]
    if (nchan * itemsize) % 64 or not aligned or c["tfactor"] > MAX_TFACTOR:
        return 0
    if c["cands"].size * (nchan * itemsize // 64) * c["ntrial"] * c["nbin"] * 12 > 1 << 30:
        return 0
    cap = STAGE_BYTES // (64 * (2 if c["coh"] else 1))
    trun = TRUN
    while trun >= 1:
        if trun <= c["ntrial"] or trun == 1:
            if c["tfactor"] + tile_range(c["hdr"], itemsize, c["cands"], c["ntrial"], c["ddm"], trun) <= cap:
                return 1
        trun //= 2
    return 0


# ---- the calls -------------------------------------------------------------------------------------------------------
def par_of(c, **kw):
    p = post.dmscan_params(c["ntrial"], c["ddm"], c["nbin"], c["tfactor"])
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def peak_par_of(c, **kw):
    p = post.dmscan_peak_params(c["widths"], c["smooth"], c["fit_frac"])
    for k, v in kw.items():
        if k == "widths":
            for i, w in enumerate(v):
                p.widths[i] = w
        else:
            setattr(p, k, v)
    return p


def outputs(ncand, ntrial, nbin, nchan, fill=0):
    out = dict(acc=np.zeros((ncand, ntrial, nbin), np.int64), hits=np.zeros((ncand, ntrial, nbin), np.uint32), snr=np.zeros((ncand, ntrial)),
               struct=np.zeros((ncand, ntrial)), results=np.zeros(ncand, dtype=post.DMSCAN_RESULT), used=np.zeros((ncand, nchan), np.uint8))
    if fill:
        for a in out.values():
            a.view(np.uint8).fill(fill)
    return out


def call(fn, c, rows_ptr, nrows=None, out=None, par=None, pk=None, ncand=None, bpar=None, hdr=None, cands=None):
    """frbch_dmscan_host / _device with the arguments of a case -> (code, message, outputs, kernel_used)"""
    hdr = hdr or c["hdr"]
    cands = c["cands"] if cands is None else cands
    n = cands.size if ncand is None else ncand
    out = out or outputs(max(n, 1), max(1, min(c["ntrial"], 4096)), max(1, min(c["nbin"], 1024)), hdr["nchans"])
    k = (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    code = fn(C.byref(post.fil_desc(hdr, hdr.get("product", 0))), rows_ptr, c["rows"].shape[0] if nrows is None else nrows,
              C.byref(bpar if bpar is not None else rc.burst_par(c["coh"])), cands.ctypes.data, n,
              c["flag"].ctypes.data if c["flag"] is not None else None, C.byref(par if par is not None else par_of(c)),
              C.byref(pk if pk is not None else peak_par_of(c)), 0, out["acc"].ctypes.data, out["hits"].ctypes.data, out["snr"].ctypes.data,
              out["struct"].ctypes.data, out["results"].ctypes.data, out["used"].ctypes.data, k, err, len(err))
    return code, err.value.decode(), out, (k[0], k[1])


def query(lib, c, rows_ptr, par=None, cands=None, hdr=None):
    cands = c["cands"] if cands is None else cands
    hdr = hdr or c["hdr"]
    return lib.frbch_dmscan_kernel(C.byref(post.fil_desc(hdr, hdr.get("product", 0))), rows_ptr, c["rows"].shape[0], C.byref(rc.burst_par(c["coh"])),
                                   cands.ctypes.data, cands.size, C.byref(par if par is not None else par_of(c)))


# ---- bursts of known DM ----------------------------------------------------------------------------------------------
KNOWN_DM, KNOWN_CENTRE, KNOWN_SAMPLE = 350.37, 350.0, 1100
KNOWN_SEED, DRIFT_ROWS = 3, 8


def known_hdr():
    return dict(rc.make_hdr(64, bw=300.0, ftop=1500.0), nbits=8, nifs=1, product=0)


@functools.lru_cache(maxsize=None)
def known_rows(seed, drift=0):
    """64 channels at 1.2 - 1.5 GHz, 64 us rows, 8-bit rows of noise 96 +- 12, a Gaussian burst of sigma 1.5 rows and amplitude 30
    at DM 350.37; `drift` > 0: the lower half of the band arrives that many rows later (two half-band components, upper first)"""
    hdr = known_hdr()
    nrows, nchan = 7680, 64
    rng = np.random.default_rng(4200 + seed)
    x = 96.0 + 12.0 * rng.standard_normal((nrows, 1, nchan))
    d = do.delays(hdr, KNOWN_DM)
    t = np.arange(nrows, dtype=np.float64)
    for ch in range(nchan):
        centre = KNOWN_SAMPLE + d[ch] + (drift if ch >= nchan // 2 else 0)
        x[:, 0, ch] += 30.0 * np.exp(-0.5 * ((t - centre) / 1.5) ** 2)
    rows = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    rows.setflags(write=False)
    return rows


def known_scan_args():
    """the scan of the known-answer tests: ddm a third of a DM sample step, 32 steps either side of the search's DM 350, 96 bins of
    one row, off-pulse windows 64 rows clear of the burst"""
    hdr = known_hdr()
    step = do.sample_step(hdr)
    cands = post.burst_cands([(KNOWN_CENTRE, KNOWN_SAMPLE, 8)], 64, 400)
    cands.setflags(write=False)
    return hdr, cands, dict(ntrial=193, ddm=step / 3.0, nbin=96, tfactor=1), step


def known_oracle(seed, drift=0):
    hdr, cands, grid, step = known_scan_args()
    out = do.scan(known_rows(seed, drift), hdr, cands, grid["ntrial"], grid["ddm"], grid["nbin"], grid["tfactor"], WIDTHS, SMOOTH, FIT_FRAC)
    return out, step
