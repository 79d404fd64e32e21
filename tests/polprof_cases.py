"""Shared case builder of the polarisation profile tests (tests/test_polprof.py on the emulator, tests/test_gpu_polprof.py on the
device): the four-product files of tests/rm_cases.py with the bin grids, reference wavelengths, RMs, gains and flags that reach
every branch of frbch_polprof_*, a file at the int64 bound, and a burst whose PA swings.  Expected values are
tests/polprof_oracle.py's, computed once per case and shared (read-only)."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import _lib, post
from tests import polprof_oracle as ppo
from tests import rm_cases as rc
from tests import rm_oracle as ro

B1, B2, B_EDGE, B_LATE, B_OUT = rc.B1, rc.B2, rc.B_EDGE, rc.B_LATE, rc.B_OUT
B_END = dict(dm=56.7, sample=4070, width=6, rm=-400.0, pa0=0.2, lin=0.7, circ=0.1)       # the bins run off the end of the file
B_MID = dict(dm=56.7, sample=4000, width=6, rm=900.0, pa0=0.4, lin=0.8, circ=0.2)        # of the 8192-row file

# name -> (nchan, nrows, nbits, coherency, foff_sign, bursts, nbin, tfactor, ref, rm per burst, gains, flag)
CASES = {
    "u8_64ch_33x3": (64, 4096, 8, False, -1, [B1, B_OUT, B2], 33, 3, "mean", (900.0, 0.0, -2500.0), False, False),      # one tile; a dead candidate between two live ones
    "u8_64ch_1x1": (64, 4096, 8, False, -1, [B1], 1, 1, "zero", (900.0,), False, False),
    "u8_64ch_2x7": (64, 4096, 8, False, -1, [B1, B_EDGE, B_END], 2, 7, "mean", (0.0, 1.0e7, 900.0), False, False),
    "u8_64ch_256x1": (64, 4096, 8, False, -1, [B_EDGE, B_END, B1], 256, 1, "zero", (900.0, -2500.0, 1.0e7), False, False),   # bins partly in front of row 0 and behind the last
    "u8_64ch_1024x2": (64, 4096, 8, False, -1, [B1, B_EDGE], 1024, 2, "mean", (900.0, 0.0), False, False),
    "u8_64ch_8x512": (64, 8192, 8, False, -1, [B_MID], 8, 512, "mean", (900.0,), False, False),
    "u8_96ch_ascending": (96, 4096, 8, False, 1, [B1, B2, B_OUT], 33, 3, "zero", (900.0, -2500.0, 0.0), False, False),    # no whole tile: generic
    "u16_64ch_coherency": (64, 4096, 16, True, -1, [B1, B2, B_EDGE], 256, 1, "mean", (900.0, -2500.0, 0.0), True, False),   # two tiles
    "u8_1024ch_late": (1024, 4096, 8, False, -1, [B1, B_EDGE, B_LATE], 33, 3, "mean", (900.0, 0.0, -2500.0), False, False),
    "u8_64ch_flag_gain": (64, 4096, 8, False, -1, [B1, B2], 33, 3, "mean", (900.0, -2500.0), True, True),
}


def gains_of(nchan):
    """gains with a negative, a zero and an infinite entry"""
    g = np.random.default_rng(5).uniform(0.5, 2.0, size=(4, nchan)).astype(np.float32)
    g[1, 7], g[2, 9], g[3, 11] = -1.5, 0.0, np.inf
    return g


def flag_of(nchan):
    f = np.zeros(nchan, np.uint8)
    f[[0, 17, nchan - 1]] = 1
    return f


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(hdr, rows, cands, coh, nbin, tfactor, ref, rm, gain, flag); the arrays are read-only"""
    nchan, nrows, nbits, coh, sign, bursts, nbin, tfactor, ref, rms, gains, flagged = CASES[name]
    hdr = dict(rc.make_hdr(nchan, foff_sign=sign), nbits=nbits)
    rows = rc.burst_file(hdr, nrows, nbits, bursts, coherency=coh, seed=len(name))
    cands = rc.cands_of(bursts, 16, 300 if nchan == 1024 else 200)
    rm = np.array(rms, dtype=np.float64)
    gain = gains_of(nchan) if gains else None
    flag = flag_of(nchan) if flagged else None
    for a in (rows, cands, rm, gain, flag):
        if a is not None:
            a.setflags(write=False)
    return dict(hdr=hdr, rows=rows, cands=cands, coh=coh, nbin=nbin, tfactor=tfactor, ref=ref, rm=rm, gain=gain, flag=flag)


def oracle_args(c):
    return (c["rows"], c["hdr"], c["cands"], c["rm"], c["nbin"], c["tfactor"], c["ref"], c["gain"], c["flag"], c["coh"])


@functools.lru_cache(maxsize=None)
def want(name):
    out = ppo.profile(*oracle_args(case(name)))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_fp64(name):
    return ppo.profile_fp64(*oracle_args(case(name)))


def same(got, exp):
    """acc, hits, used, results and every field of the bins byte for byte; pa, which goes through libm's atan2, to 1e-12"""
    for f in ("acc", "hits", "used", "results"):
        if np.ascontiguousarray(got[f]).tobytes() != np.ascontiguousarray(exp[f]).tobytes():
            return False
    for f in post.PROF_BIN.names:
        if f != "pa" and np.ascontiguousarray(got["bins"][f]).tobytes() != np.ascontiguousarray(exp["bins"][f]).tobytes():
            return False
    return bool(np.allclose(got["bins"]["pa"], exp["bins"]["pa"], rtol=0, atol=1e-12))


# ---- the calls -------------------------------------------------------------------------------------------------------
def par_of(c, size=None):
    p = post.prof_params(c["nbin"], c["tfactor"], c["ref"])
    if size is not None:
        p.size = size
    return p


def outputs(ncand, nbin, nchan, fill=0):
    out = dict(acc=np.zeros((ncand, nbin, 4), np.int64), hits=np.zeros((ncand, nbin), np.uint32), bins=np.zeros((ncand, nbin), dtype=post.PROF_BIN),
               results=np.zeros(ncand, dtype=post.PROF_RESULT), used=np.zeros((ncand, nchan), np.uint8))
    if fill:
        for a in out.values():
            a.view(np.uint8).fill(fill)
    return out


def call(fn, c, rows_ptr, nrows=None, out=None, par=None, ncand=None, rm=None, bpar=None, hdr=None):
    """frbch_polprof_host / _device with the arguments of a case -> (code, message, outputs, kernel_used)"""
    hdr = hdr or c["hdr"]
    n = c["cands"].size if ncand is None else ncand
    out = out or outputs(max(n, 1), max(1, min(c["nbin"], 1024)), hdr["nchans"])
    k = (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    rm = c["rm"] if rm is None else rm
    code = fn(C.byref(post.fil_desc(dict(hdr, nifs=hdr.get("nifs", 4)))), rows_ptr, c["rows"].shape[0] if nrows is None else nrows,
              C.byref(bpar if bpar is not None else rc.burst_par(c["coh"])), c["cands"].ctypes.data, n, rm.ctypes.data if rm is not False else None,
              c["gain"].ctypes.data if c["gain"] is not None else None, c["flag"].ctypes.data if c["flag"] is not None else None,
              C.byref(par if par is not None else par_of(c)), 0, out["acc"].ctypes.data, out["hits"].ctypes.data, out["bins"].ctypes.data,
              out["results"].ctypes.data, out["used"].ctypes.data, k, err, len(err))
    return code, err.value.decode(), out, (k[0], k[1])


def query(lib, c, rows_ptr, par=None):
    return lib.frbch_polprof_kernel(C.byref(post.fil_desc(c["hdr"])), rows_ptr, c["rows"].shape[0], C.byref(rc.burst_par(c["coh"])),
                                    c["cands"].ctypes.data, c["cands"].size, C.byref(par if par is not None else par_of(c)))


# ---- the int64 bound -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bound_case(tfactor=512):
    """16384 channels x 16 bit, tfactor 512, nbin 2, DM 0: 1024 rows of 65535 under the two bins on a floor of 0 that both
    off-pulse windows lie on, so that every channel's on-pulse minus baseline is +full scale; gains 1, rm 0: every C = 2^22.
    (tfactor 128: the same sums, 2^57, at a bin length the fast kernel takes.)"""
    nchan, nrows = 16384, 1400
    hdr = dict(rc.make_hdr(nchan, bw=256.0), nbits=16)
    rows = np.zeros((nrows, 4, nchan), np.uint16)
    rows[188:1212] = 65535
    cands = post.burst_cands([(0.0, 700, 1024)], 4, 64)
    c = dict(hdr=hdr, rows=rows, cands=cands, coh=False, nbin=2, tfactor=tfactor, ref="mean", rm=np.zeros(1), gain=None, flag=None)
    for a in (rows, cands, c["rm"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def bound_want(tfactor=512):
    c = bound_case() if tfactor == 512 else bound_case(tfactor)          # (one cached file per call form)
    return ppo.profile(*oracle_args(c), unbounded=tfactor == 512)


# ---- the known answer ------------------------------------------------------------------------------------------------
KNOWN_RM, KNOWN_WIDTH, KNOWN_SWING = 350.0, 40, (-30.0, 30.0)


@functools.lru_cache(maxsize=None)
def known_case(seed=11):
    """1.2 - 1.5 GHz, 1024 channels x 8 bit: a burst of 40 rows at DM 50 with RM +350 rad m^-2 whose PA (at infinite frequency)
    swings linearly from -30 to +30 degrees across it; amplitude 20 on a floor of 100 with integer noise of about 3, L/I 0.9"""
    hdr = dict(rc.known_hdr(), nbits=8)
    nchan, nrows, amp, lin, circ = 1024, 4096, 20.0, 0.9, 0.1
    rng = np.random.default_rng(9000 + seed)
    x = 100.0 + rng.integers(-5, 6, size=(nrows, 4, nchan)).astype(np.float64)
    l2, d, chans = ro.lambda2(hdr), ro.delays(hdr, 50.0), np.arange(nchan)
    sample = 2000
    on_lo = sample - KNOWN_WIDTH // 2
    pa = np.radians(np.linspace(KNOWN_SWING[0], KNOWN_SWING[1], KNOWN_WIDTH))
    for u in range(KNOWN_WIDTH):
        ang = 2.0 * (pa[u] + KNOWN_RM * l2)
        r = on_lo + u + d
        for p, v in enumerate((np.full(nchan, amp), amp * lin * np.cos(ang), amp * lin * np.sin(ang), np.full(nchan, amp * circ))):
            x[r, p, chans] += v
    rows = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    cands = post.burst_cands([(50.0, sample, KNOWN_WIDTH)], 32, 400)
    c = dict(hdr=hdr, rows=rows, cands=cands, coh=False, nbin=64, tfactor=1, ref="zero", rm=np.array([KNOWN_RM]), gain=None, flag=None)
    for a in (rows, cands, c["rm"]):
        a.setflags(write=False)
    injected = np.full(64, np.nan)
    injected[32 - KNOWN_WIDTH // 2:32 - KNOWN_WIDTH // 2 + KNOWN_WIDTH] = pa          # bin j holds row sample - 32 + j
    return c, injected


def check_known(bins, res, injected):
    """every bin with L_db / sigma_L >= 8 lies within 4 pa_err of the injected PA; at least 10 qualify -> their number"""
    sl = float(res["sigma_l"])
    strong = np.flatnonzero(bins["l_db"] >= 8.0 * sl)
    assert strong.size >= 10 and bins["pa_valid"][strong].all() and np.isfinite(injected[strong]).all(), strong
    diff = (bins["pa"][strong] - injected[strong] + np.pi / 2) % np.pi - np.pi / 2
    worst = np.abs(diff) / (4.0 * bins["pa_err"][strong])
    print("known answer: %d bins, largest |PA - injected| / (4 pa_err) = %.3f, sigma_L = %.4f" % (strong.size, worst.max(), sl))
    assert (worst <= 1.0).all(), (strong, diff, bins["pa_err"][strong])
    return strong.size


# ---- rows past a byte mark -------------------------------------------------------------------------------------------
def check_beyond_the_mark(lib, br, mem, behind, front, off_len, nbin, tfactor, kernels):
    """The profile on the rows of a tests/big_rows.BigRows with four products, four candidates of DM 104: one whose bins begin
    `behind` rows behind the row of the last byte mark, one centred `front` rows in front of it -- the delays carry the bins of some
    tiles across the mark inside one run --, one in front of the first mark and one whose bins run off nrows; a burst with its own
    amplitude in every product lies on the first two.  kernels: (shift of the rows in bytes, the burst-sums kernel, the profile
    kernel) per pass.  The expected values are the oracle's on the window of rows each candidate reads, the sample moved."""
    from tests import big_rows as bg
    res = bg.Resident(br, mem)
    try:
        hdr = br.hdr()
        mark, width, gap = br.byte_mark_rows[-1], 4, 16
        d = ro.delays(hdr, 104.0)
        maxd, half, reach = int(d.max()), (nbin // 2) * tfactor, gap + off_len
        samples = [mark + behind + half, mark - front, min(1000, br.byte_mark_rows[0] // 2), br.nrows - maxd - half // 2]
        cands = post.burst_cands([(104.0, s, width) for s in samples], gap, off_len)
        rm = np.array([900.0, -2500.0, 0.0, 1.0e7])
        c = dict(hdr=hdr, rows=None, cands=cands, coh=False, nbin=nbin, tfactor=tfactor, ref="mean", rm=rm, gain=None, flag=None)
        t0 = [s - half for s in samples]
        assert t0[0] >= mark and t0[2] + nbin * tfactor + maxd < br.byte_mark_rows[0] and t0[3] + nbin * tfactor + maxd > br.nrows
        # candidate 1: a run of bins of some tile is staged from rows on both sides of the mark
        ct = 64 // br.dtype.itemsize
        dt = d.reshape(-1, ct)
        spread = int((dt.max(axis=1) - dt.min(axis=1)).max())
        brun = min(nbin, (256 - spread) // tfactor)
        firsts = [t0[1] + j0 * tfactor + dt.min(axis=1) for j0 in range(0, nbin, brun)]
        lasts = [t0[1] + min(nbin, j0 + brun) * tfactor + dt.max(axis=1) for j0 in range(0, nbin, brun)]
        assert brun >= 1 and any(((a < mark) & (mark < b)).any() for a, b in zip(firsts, lasts))
        for shift, k_spec, k_prof in kernels:
            res.lay(shift)
            for i in (0, 1):
                for prod, amp in enumerate((9, 5, 3, 2)):
                    bg.write_burst(res, prod, 104.0, samples[i] - width // 2, width, amp)
            wants = []
            for i, cd in enumerate(cands):
                on_lo = samples[i] - width // 2
                w0 = max(0, min(on_lo - reach, t0[i]))
                w1 = min(br.nrows, max(on_lo + width + reach, t0[i] + nbin * tfactor) + maxd + 1)
                moved = cands[i:i + 1].copy()
                moved["sample"] -= w0
                wants.append(ppo.profile(res.window(w0, w1 - w0), hdr, moved, rm[i:i + 1], nbin, tfactor, "mean"))
            want = {f: np.concatenate([w[f] for w in wants]) for f in wants[0]}
            assert want["used"].all() and (want["hits"][:3] == br.nchan * tfactor).all()
            assert 0 < want["hits"][3, -1] < want["hits"][3, 0] == br.nchan * tfactor                # the last bins lose rows behind nrows
            r = want["results"]
            assert all(want["bins"]["i"][i, r["on_lo_bin"][i]] > 5.0 for i in (0, 1)) and abs(want["bins"]["i"][2]).max() < 1.0      # the burst is seen
            ptr = C.c_void_p(res.address)
            q = lib.frbch_polprof_kernel(C.byref(post.fil_desc(hdr)), ptr, br.nrows, C.byref(rc.burst_par(False)), cands.ctypes.data, cands.size,
                                         C.byref(par_of(c)))
            with bg.guarded():
                code, msg, out, k = call(lib.frbch_polprof_device, c, ptr, nrows=br.nrows, out=outputs(cands.size, nbin, br.nchan, fill=0xA5))
            assert code == 0, msg
            assert k == (k_spec, k_prof) and q == k_prof, (shift, k, q)
            assert same(out, want), shift
            res.buf.check()
        res.check_equals()                                   # the rows are never written
    finally:
        res.free()
