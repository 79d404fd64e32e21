"""The burst and band entry points on rows past the 2^31 and the 2^32 mark (tests/test_gpu_beyond_4gib_burst.py on the device at
the real marks, tests/test_big_burst_rows.py on the emulator at marks of 2^20 / 2^21 bytes).  A plain module beside
tests/big_rows.py, whose description of the rows (BigRows, Resident, the two memories, the shapes) it uses unchanged.

Four candidates go into every call: `start` (the earlier off window partly in front of row 0), `lo` and `hi` (the rows of the
on-pulse window run across the row of the first / the last byte mark as the delay grows over the band), `end` (the later off
window cut at nrows).  What each one is there for is a condition on the restatement's delays (`conditions`), asserted before a
library runs.  Expected values are the existing restatements -- burst_edge_cases.window_sums, rm_oracle, polprof_oracle,
dmscan_oracle, acf_oracle, scat_oracle -- on the window of rows each candidate can touch, the sample moved to the window
(`windowed`); the band series are big_rows.window_series generalised to a channel range.  tests/test_big_burst_rows.py holds
every windowed value equal to the same restatement on the WHOLE small array.  No tolerance is added: every comparison is the
comparator the entry point's own tests use."""
import ctypes as C

import numpy as np

from frb_baseband_amd import post
from tests import acf_cases as ac
from tests import acf_oracle as ao
from tests import bands_oracle as bo
from tests import big_rows as bg
from tests import burst_edge_cases as bec
from tests import dmscan_cases as dc
from tests import dmscan_oracle as do
from tests import polprof_cases as pc
from tests import polprof_oracle as ppo
from tests import rm_cases as rc
from tests import rm_oracle as ro
from tests import scat_cases as sc
from tests import scat_oracle as so

FAST, GENERIC = 1, 0
NAMES = ("start", "lo", "hi", "end")
START, LO, HI, END = range(4)
DM = bg.DMS[0]
WIDTH, OFF_GAP, OFF_LEN = 8, 16, 512                     # at the real shapes: a host window of one candidate stays below 3000 rows
SMALL_WIDTH, SMALL_OFF_GAP, SMALL_OFF_LEN = 8, 8, 32     # at the emulator's: half the largest delay (101 rows at DM 100) still exceeds a window's reach
NBIN, TFACTOR = 64, 4
RM = np.array([900.0, -2500.0, 0.0, 1.0e7])
RM.setflags(write=False)
RM_GRID = dict(nphi=64, phi_lo=-3200.0, dphi=100.0)      # 64 trials: the smallest fast transform
SCAN_NTRIAL = 17                                         # one whole trial run of 16 and one of 1
ACF_LAGS = dict(nlagf=8, nlagt=16)
SCAT_FFACTOR, SCAT_SHIFT0, SCAT_NSHIFT = 1024, 16, 32


def max_delay(br, dm):
    return int(ro.delays(br.hdr(), float(dm)).max())


# ---- the candidates ---------------------------------------------------------------------------------------------------
def burst_cands(br, dm, width, off_gap, off_len):
    """-> four frbch_burst_cand: start, lo, hi, end.  M1, M2 = br.byte_mark_rows, D = the largest delay at `dm`:
    start: on_lo = off_gap + off_len / 2 -- half of the earlier off window lies in front of row 0 at the top of the band;
    lo, hi: sample = M - D / 2 -- the on-pulse rows s + n_c run from before row M to behind it across the band;
    end: the later off window starts off_len / 2 rows in front of nrows in the most delayed channel."""
    D = max_delay(br, dm)
    m1, m2 = br.byte_mark_rows
    half = width // 2
    on_lo_end = br.nrows - D - off_len // 2 - off_gap - width
    samples = [off_gap + off_len // 2 + half, m1 - D // 2, m2 - D // 2, on_lo_end + half]
    return post.burst_cands([(float(dm), s, width) for s in samples], off_gap, off_len)


def rows_of(cand, d, w):
    """first and last row of window w (0 earlier off, 1 on, 2 later off) in every channel, not clipped -> (first [nchan], last [nchan])"""
    w0, length, _which = ro.windows(cand)[w]
    return w0 + d, w0 + length - 1 + d


def _sides(first, last, mark):
    """(a channel's rows end before the mark row, a channel's rows start at or behind it, a channel's rows hold mark - 1 and mark)"""
    return bool((last < mark).any()), bool((first >= mark).any()), bool(((first <= mark - 1) & (last >= mark)).any())


def hits_of(cand, d, w, nrows):
    first, last = rows_of(cand, d, w)
    return np.clip(last + 1, 0, nrows) - np.clip(first, 0, nrows)


def conditions(br, cands):
    """What the four candidates are there for, on the restatement's delays alone -> dict of figures.

    Two of the conditions as one would first write them cannot hold for one DM and one off_len: an off window of `lo` / `hi`
    has channels wholly on BOTH sides of the mark only where D / 2 >= width + off_gap + off_len, and the later window of `end`
    (the earlier of `start`) is cut in EVERY channel only where off_len > D.  Asserted is what always can hold -- the off
    windows of lo / hi straddle the mark in some channel and lie wholly on one side in another; the clipped window loses rows
    in some channel and keeps rows in every channel, so that no channel goes unused -- and the stronger form wherever the
    arithmetic of the shape admits it (`both_sides`, `cut_everywhere`)."""
    assert len(cands) == 4
    hdr = br.hdr()
    d = ro.delays(hdr, float(cands[0]["dm"]))
    D = int(d.max())
    assert (cands["dm"] == cands[0]["dm"]).all() and int(d.min()) == 0
    m1, m2 = br.byte_mark_rows
    width, gap, off_len = (int(cands[0][f]) for f in ("width", "off_gap", "off_len"))
    reach = width + gap + off_len
    both_sides, cut_everywhere = D // 2 >= reach, off_len > D
    # lo, hi: the on-pulse rows, then the off window that points at the mark
    for i, mark, w_off in ((LO, m1, 2), (HI, m2, 0)):
        assert _sides(*rows_of(cands[i], d, 1), mark) == (True, True, True), (NAMES[i], "on-pulse rows")
        before, behind, across = _sides(*rows_of(cands[i], d, w_off), mark)
        assert across and (before or behind), (NAMES[i], "off window", before, behind, across)
        assert not both_sides or (before and behind), (NAMES[i], "off window")
    # hi: the rows a fast workgroup stages, base .. base + span of the burst-sums kernel, hold M2 - 1 and M2 for some 64-byte tile
    ct = 64 // br.dtype.itemsize
    dt = d.reshape(-1, ct)
    staged = 0
    for w in range(3):
        w0, length, _which = ro.windows(cands[HI])[w]
        base, last = w0 + dt.min(axis=1), w0 + length - 1 + dt.max(axis=1)
        staged += int(((base <= m2 - 1) & (last >= m2)).sum())
        assert w != 1 or ((base <= m2 - 1) & (last >= m2)).any()
    # start, end: the clipped off window
    for i, w in ((START, 0), (END, 2)):
        h = hits_of(cands[i], d, w, br.nrows)
        assert int(h.min()) > 0 and int(h.min()) < off_len, (NAMES[i], int(h.min()), int(h.max()))
        assert not cut_everywhere or int(h.max()) < off_len
        for other in (0, 1, 2):
            if other != w:
                assert (hits_of(cands[i], d, other, br.nrows) == int(ro.windows(cands[i])[other][1])).all()
    on_lo = int(cands[START]["sample"]) - width // 2
    assert on_lo - gap - off_len < 0 <= on_lo
    w0_end = ro.windows(cands[END])[2][0]
    assert 0 < w0_end < br.nrows < w0_end + D + off_len
    for i in (LO, HI):                                    # the interior candidates lose no row
        assert all((hits_of(cands[i], d, w, br.nrows) == int(ro.windows(cands[i])[w][1])).all() for w in range(3))
    # pairwise disjoint at the top of the band, and no two a multiple of P rows apart
    ext = [(ro.windows(c)[0][0], ro.windows(c)[2][0] + off_len) for c in cands]
    for i in range(4):
        for j in range(i + 1, 4):
            assert ext[i][1] <= ext[j][0], (NAMES[i], NAMES[j])
            assert (ext[j][0] - ext[i][0]) % br.P != 0
    # a wrapped byte offset reads another row of the base, in every product
    # (the rows of hi at or behind M2 against those 2^32 bytes in front of them, the rows of lo likewise against 2^31: the mark row
    # itself and the first on-pulse row of the most delayed channel)
    for i, mark in ((HI, m2), (LO, m1)):
        for r in (mark, int(cands[i]["sample"]) - width // 2 + D):
            assert r - mark >= 0
            for p in range(br.nifs):
                assert not np.array_equal(br.base[r % br.P, p], br.base[(r - mark) % br.P, p]), (NAMES[i], p)
    return dict(D=D, both_sides=both_sides, cut_everywhere=cut_everywhere, staged_tiles=staged)


def windowed(br, cand, reach):
    """cand: one candidate (an array of one record); reach: the largest delay at any DM the case reads this candidate at
    -> (t0, x, cand'): x = br.window(t0, n) holds every row the candidate can touch, cand' is the candidate with sample - t0.
    The window is cut only where the file is: t0 = 0 for a candidate whose earlier window starts in front of row 0, and a window
    that would pass nrows ends exactly there, so that the restatement's clip at its own first and last row is the file's."""
    cand = np.atleast_1d(cand)
    assert cand.size == 1
    wins = ro.windows(cand[0])
    first, last = wins[0][0], wins[2][0] + wins[2][1] + int(reach)              # rows [first, last) at any delay 0 .. reach
    t0, t1 = max(0, first), min(br.nrows, last)
    assert not (first < 0 and last > br.nrows) and t0 < t1
    assert t0 in (0, first) and t1 in (last, br.nrows) and (t0 == first or first < 0) and (t1 == last or last > br.nrows)
    moved = cand.copy()
    moved["sample"] -= t0
    x = br.window(t0, t1 - t0)
    return t0, x, moved


def _bins_inside(cands, nbin, tfactor):
    """the bins of a candidate lie within its off windows: `windowed` holds their rows as well"""
    for c in cands:
        half = (nbin // 2) * tfactor
        assert half <= int(c["width"]) // 2 + int(c["off_gap"]) + int(c["off_len"]) and nbin * tfactor - half <= int(c["off_gap"]) + int(c["off_len"])


def _concat(parts, fields):
    return {f: np.concatenate([np.asarray(p[f]) for p in parts]) for f in fields}


def _frozen(out):
    for a in (out.values() if isinstance(out, dict) else out):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---- expected values -----------------------------------------------------------------------------------------------------
def want_sums(br, cands, block=16384):
    """burst_edge_cases.window_sums on the window of every candidate, a block of channels at a time -> BURST_SUMS [4][nifs][nchan]"""
    hdr = br.hdr()
    out = np.zeros((len(cands), br.nifs, br.nchan), dtype=post.BURST_SUMS)
    for i in range(len(cands)):
        _t0, x, moved = windowed(br, cands[i:i + 1], max_delay(br, cands[i]["dm"]))
        for c0 in range(0, br.nchan, block):
            out[i, :, c0:c0 + block] = bec.window_sums(x[:, :, c0:c0 + block], hdr, moved, c0)[0]
    out.setflags(write=False)
    return out


def want_spectra(sums, coh):
    return _frozen(ro.derive(sums, None, coh))


def want_rm(br, cands, coh=False, grid=RM_GRID):
    hdr = br.hdr()
    parts = []
    for i in range(len(cands)):
        _t0, x, moved = windowed(br, cands[i:i + 1], max_delay(br, cands[i]["dm"]))
        parts.append(ro.burst_rm(x, hdr, moved, grid["nphi"], grid["phi_lo"], grid["dphi"], coherency=coh))
    return _frozen(_concat(parts, ("spec", "noise", "used", "F", "results")))


def want_prof(br, cands, coh, nbin=NBIN, tfactor=TFACTOR, rm=RM):
    _bins_inside(cands, nbin, tfactor)
    hdr = br.hdr()
    parts = []
    for i in range(len(cands)):
        _t0, x, moved = windowed(br, cands[i:i + 1], max_delay(br, cands[i]["dm"]))
        parts.append(ppo.profile(x, hdr, moved, rm[i:i + 1], nbin, tfactor, "mean", None, None, coh))
    return _frozen(_concat(parts, ("acc", "hits", "bins", "results", "used")))


def scan_reach(br, cands, ntrial, ddm):
    return max(max_delay(br, dm) for c in cands for dm in do.trial_dms(c["dm"], ntrial, ddm))


def want_scan(br, cands, prod, coh, ddm, ntrial=SCAN_NTRIAL, nbin=NBIN, tfactor=TFACTOR):
    _bins_inside(cands, nbin, tfactor)
    hdr = dict(br.hdr(), product=prod)
    parts = []
    for i in range(len(cands)):
        _t0, x, moved = windowed(br, cands[i:i + 1], scan_reach(br, cands[i:i + 1], ntrial, ddm))
        parts.append(do.scan(x, hdr, moved, ntrial, ddm, nbin, tfactor, dc.WIDTHS, dc.SMOOTH, dc.FIT_FRAC, coherency=coh))
    return _frozen(_concat(parts, dc.FIELDS))


def want_acf(br, cands, prod, ffactor, nbin=NBIN, tfactor=TFACTOR, nlagf=ACF_LAGS["nlagf"], nlagt=ACF_LAGS["nlagt"]):
    _bins_inside(cands, nbin, tfactor)
    hdr = dict(br.hdr(), product=prod)
    parts = []
    for i in range(len(cands)):
        _t0, x, moved = windowed(br, cands[i:i + 1], max_delay(br, cands[i]["dm"]))
        parts.append(ao.burst_acf(x, hdr, moved, nbin, tfactor, ffactor, nlagf, nlagt, ac.FIT_FRAC))
    return _frozen(_concat(parts, ac.FIELDS))


def scat_bank():
    return sc.bank_of(*sc.SMALL_BANK)


def want_scat(br, cands, prod, ffactor, nbin=NBIN, tfactor=TFACTOR, shift0=SCAT_SHIFT0, nshift=SCAT_NSHIFT):
    _bins_inside(cands, nbin, tfactor)
    hdr = dict(br.hdr(), product=prod)
    bank, bp = scat_bank()
    sc.assert_shifts_off_the_ties(hdr, ffactor, sc.ALPHAS, bp["rtau"])
    parts = []
    for i in range(len(cands)):
        _t0, x, moved = windowed(br, cands[i:i + 1], max_delay(br, cands[i]["dm"]))
        parts.append(so.burst_scatter(x, hdr, moved, nbin, tfactor, ffactor, bank, bp, shift0, nshift, sc.ALPHAS, sc.SNR_MIN))
    return _frozen(_concat(parts, sc.FIELDS))


# ---- the cases as the callers of the *_cases modules take them (the rows hold no byte: only their type and count are read) -------
def case_of(br, cands, coh=False, prod=0, **kw):
    rows = np.empty((br.nrows, br.nifs, 0), br.dtype)
    return dict(hdr=dict(br.hdr(), product=prod), rows=rows, cands=cands, coh=coh, flag=None, gain=None, **kw)


def prof_case(br, cands, coh, nbin=NBIN, tfactor=TFACTOR):
    return case_of(br, cands, coh, nbin=nbin, tfactor=tfactor, ref="mean", rm=RM)


def scan_case(br, cands, prod, coh, ddm, ntrial=SCAN_NTRIAL, nbin=NBIN, tfactor=TFACTOR):
    return case_of(br, cands, coh, prod, ntrial=ntrial, ddm=ddm, nbin=nbin, tfactor=tfactor, widths=dc.WIDTHS, smooth=dc.SMOOTH, fit_frac=dc.FIT_FRAC)


def acf_case(br, cands, prod, ffactor, nbin=NBIN, tfactor=TFACTOR):
    return case_of(br, cands, False, prod, nbin=nbin, tfactor=tfactor, ffactor=ffactor, fit_frac=ac.FIT_FRAC, **ACF_LAGS)


def scat_case(br, cands, prod, ffactor, nbin=NBIN, tfactor=TFACTOR, shift0=SCAT_SHIFT0, nshift=SCAT_NSHIFT):
    bank, bp = scat_bank()
    return case_of(br, cands, False, prod, nbin=nbin, tfactor=tfactor, ffactor=ffactor, shift0=shift0, nshift=nshift, bank=bank, bp=bp,
                   alphas=sc.ALPHAS, snr_min=sc.SNR_MIN)


def sample_step(lib, br):
    step = lib.frbch_dm_sample_step(C.byref(br.desc()))
    assert step == do.sample_step(br.hdr())
    return step


def emulated(lib):
    return bg.mem_for(lib) is bg.HostMem


def sums_form(lib, br, shift):
    """the burst-sums kernel for rows `shift` bytes off the aligned address (burst_edge_cases.spectra_kernel_expected on the shape)"""
    if emulated(lib):
        return GENERIC
    return FAST if br.nifs <= 4 and (br.nchan * br.dtype.itemsize) % 64 == 0 and shift % 16 == 0 else GENERIC


# ---- callers of the C ABI on the resident rows ---------------------------------------------------------------------------------
def spectra_device(lib, res, cands, coh):
    """frbch_burstspec_device; d_sums in a guarded buffer of exactly ncand * nifs * nchan records -> (sums, spec, noise, used,
    kernel_used, frbch_burstspec_kernel)"""
    br = res.br
    n = cands.size
    d_sums = bg.out_buffer(res.mem, n * br.nifs * br.nchan * post.BURST_SUMS.itemsize)
    spec, noise = np.zeros((n, br.nifs, br.nchan), np.float32), np.zeros((n, br.nifs, br.nchan), np.float32)
    used = np.zeros((n, br.nchan), np.uint8)
    par, desc = rc.burst_par(coh), br.desc()
    ptr = C.c_void_p(res.address)
    query = lib.frbch_burstspec_kernel(C.byref(desc), ptr, br.nrows, C.byref(par), cands.ctypes.data, n)
    k = C.c_uint32(99)
    err = C.create_string_buffer(512)
    try:
        with bg.guarded():
            code = lib.frbch_burstspec_device(C.byref(desc), ptr, br.nrows, C.byref(par), cands.ctypes.data, n, None, 0, d_sums.ptr,
                                              spec.ctypes.data, noise.ctypes.data, used.ctypes.data, C.byref(k), err, len(err))
        assert code == 0, err.value
        d_sums.check()
        sums = d_sums.to_numpy(np.uint8).view(post.BURST_SUMS).reshape(n, br.nifs, br.nchan).copy()
    finally:
        d_sums.free()
    return sums, spec, noise, used, k.value, query


def check_spectra(lib, res, cands, coh, form, sums, derived):
    """every field of the sums with ==, then spec, noise and used byte for byte"""
    got = spectra_device(lib, res, cands, coh)
    assert got[4] == got[5] == form, (got[4], got[5], form)
    for i, name in enumerate(NAMES):
        for f in post.BURST_SUMS.names:
            bad = np.argwhere(got[0][f][i] != sums[f][i])
            assert bad.size == 0, "%s: %s differs in %d (product, channel) records, the first %s: %r, expected %r" % (
                name, f, len(bad), tuple(bad[0]), got[0][f][i][tuple(bad[0])], sums[f][i][tuple(bad[0])])
    for i, name in enumerate(NAMES):
        for a, b, what in zip(got[1:4], derived, ("spec", "noise", "used")):
            assert a[i].tobytes() == b[i].tobytes(), (name, what)
    res.check_equals()


def check_rm(lib, res, cands, form, want, grid=RM_GRID):
    br = res.br
    got, k = rc.device_burst_rm(lib, br.hdr(), C.c_void_p(res.address), br.nrows, cands, False, grid["nphi"], grid["phi_lo"], grid["dphi"])
    assert k[0] == form, k
    assert emulated(lib) or k[1] == FAST, k
    for i, name in enumerate(NAMES):
        for f in ("spec", "noise", "used", "F"):
            assert got[f][i].tobytes() == want[f][i].tobytes(), (name, f)
        assert rc.same_results(got["results"][i:i + 1], want["results"][i:i + 1]), name
    res.check_equals()


def check_prof(lib, res, c, forms, want):
    """forms: (the burst-sums kernel, the profile kernel)"""
    br = res.br
    ptr = C.c_void_p(res.address)
    q = pc.query(lib, c, ptr)
    with bg.guarded():
        code, msg, out, k = pc.call(lib.frbch_polprof_device, c, ptr, out=pc.outputs(c["cands"].size, c["nbin"], br.nchan, fill=0xA5))
    assert code == 0, msg
    assert k == forms and q == forms[1], (k, q, forms)
    for i, name in enumerate(NAMES):
        assert pc.same({f: out[f][i:i + 1] for f in out}, {f: want[f][i:i + 1] for f in want}), name
    res.check_equals()


def check_scan(lib, res, c, forms, want):
    br = res.br
    ptr = C.c_void_p(res.address)
    q = dc.query(lib, c, ptr)
    with bg.guarded():
        code, msg, out, k = dc.call(lib.frbch_dmscan_device, c, ptr, out=dc.outputs(c["cands"].size, c["ntrial"], c["nbin"], br.nchan, fill=0xA5))
    assert code == 0, msg
    assert k == forms and q == forms[1], (k, q, forms)
    for i, name in enumerate(NAMES):
        assert dc.same({f: out[f][i:i + 1] for f in dc.FIELDS}, {f: want[f][i:i + 1] for f in dc.FIELDS}), name
    res.check_equals()


def check_acf(lib, res, c, forms, want):
    """forms: (the burst-sums kernel, the dynamic-spectrum kernel); the ACF kernel is held to the query (its plan does not read the rows)"""
    ptr = C.c_void_p(res.address)
    qc, q = ac.query(lib, c, ptr)
    assert qc == 0
    with bg.guarded():
        code, msg, out, k = ac.call(lib.frbch_burstacf_device, c, ptr, out=ac.outputs_of(c, fill=0xA5))
    assert code == 0, msg
    assert k[:2] == forms and k == q, (k, q, forms)
    for i, name in enumerate(NAMES):
        assert ac.differing({f: out[f][i:i + 1] for f in ac.FIELDS}, {f: want[f][i:i + 1] for f in ac.FIELDS}) == [], name
    res.check_equals()
    return k


def check_scat(lib, res, c, forms, want):
    ptr = C.c_void_p(res.address)
    qc, q = sc.query(lib, c, ptr)
    assert qc == 0
    with bg.guarded():
        code, msg, out, k = sc.call(lib.frbch_burstscat_device, c, ptr, out=sc.outputs_of(c, fill=0xA5))
    assert code == 0, msg
    assert k[:2] == forms and k == q, (k, q, forms)
    for i, name in enumerate(NAMES):
        assert sc.differing({f: out[f][i:i + 1] for f in sc.FIELDS}, {f: want[f][i:i + 1] for f in sc.FIELDS}) == [], name
    res.check_equals()
    return k


def untouched(out):
    return all(bool((np.asarray(a).view(np.uint8) == 0xA5).all()) for a in out.values())


def refusals(lib, res, desc_hdr, cands, ddm, which=("prof", "scan", "acf", "scat")):
    """the windowed entry points named in `which` on a header they refuse -> {name: (code, message, outputs still 0xA5)}.  desc_hdr:
    the header handed to the library (the rows are never read: a refusal comes before any launch); every call must be refused,
    the outputs are a few poisoned words"""
    br = res.br
    ptr = C.c_void_p(res.address)
    base = dict(hdr=dict(desc_hdr, product=0), rows=np.empty((br.nrows, 0, 0), br.dtype), cands=cands, coh=False, flag=None, gain=None)
    bank, bp = scat_bank()
    calls = dict(
        prof=lambda: pc.call(lib.frbch_polprof_device, dict(base, nbin=NBIN, tfactor=TFACTOR, ref="mean", rm=RM), ptr, out=pc.outputs(4, 4, 4, fill=0xA5)),
        scan=lambda: dc.call(lib.frbch_dmscan_device, dict(base, ntrial=SCAN_NTRIAL, ddm=ddm, nbin=NBIN, tfactor=TFACTOR, widths=dc.WIDTHS, smooth=dc.SMOOTH,
                                                          fit_frac=dc.FIT_FRAC), ptr, out=dc.outputs(4, 4, 4, 4, fill=0xA5)),
        acf=lambda: ac.call(lib.frbch_burstacf_device, dict(base, nbin=NBIN, tfactor=TFACTOR, ffactor=16, fit_frac=ac.FIT_FRAC, **ACF_LAGS), ptr,
                            out=ac.outputs(4, 4, 4, 2, 2, 4, fill=0xA5)),
        scat=lambda: sc.call(lib.frbch_burstscat_device, dict(base, nbin=NBIN, tfactor=TFACTOR, ffactor=SCAT_FFACTOR, shift0=SCAT_SHIFT0, nshift=SCAT_NSHIFT,
                                                             bank=bank, bp=bp, alphas=sc.ALPHAS, snr_min=sc.SNR_MIN), ptr,
                             out=sc.outputs(4, 4, 4, 2, 2, 4, fill=0xA5)))
    out = {}
    for name in which:
        with bg.guarded():
            code, msg, o, _k = calls[name]()
        assert code != 0, "%s was not refused: its outputs here hold a few words only" % name
        out[name] = (code, msg, untouched(o))
    return out


# ---- dedispersed bands -----------------------------------------------------------------------------------------------------------
NSUB = 8


def window_band_parts(cum, d, n, c_lo, c_hi):
    """big_rows.window_series on the channels [c_lo, c_hi) -> (a, b) int64 [n]: a[t] = sum_c x[t + d[c]][c], b[t] = sum_c S[t + d[c]]
    over the band's channels, S the row sums of the FULL band; every run of channels of the band that share a delay is one
    difference of two prefix sums, and its zero-DM term the row sum times the number of channels of the run"""
    assert 0 <= c_lo < c_hi <= cum.shape[1] - 1
    assert cum.shape[0] >= n + int(d.max()) and int(d.min()) >= 0
    cuts = np.concatenate(([c_lo], c_lo + np.flatnonzero(np.diff(d[c_lo:c_hi])) + 1, [c_hi]))
    c0, c1 = cuts[:-1], cuts[1:]
    rows = np.arange(n)[:, None] + d[c0][None, :]
    a = (cum[rows, c1[None, :]] - cum[rows, c0[None, :]]).sum(axis=1, dtype=np.int64)
    b = (cum[:, -1].astype(np.int64)[rows] * (c1 - c0)[None, :]).sum(axis=1, dtype=np.int64)
    return a, b


def band_value(a, b, nchan, zerodm):
    """the series of include/frbch.h from the exact sums: (float)(a - b / nchan), as bands_oracle.dedisperse_bands has it"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return (a - b / nchan if zerodm else a).astype(np.float32)


def window_band_series(cum, d, n, c_lo, c_hi, zerodm):
    a, b = window_band_parts(cum, d, n, c_lo, c_hi)
    return band_value(a, b, cum.shape[1] - 1, zerodm)


def band_planes(x, dl, n, nsub, bands):
    """x: n + maxd rows of one product after the clip -> {zerodm: plane [ndm * nband][n]}: the parts of every sub-band once, the
    bands as sums of theirs (exact integers)"""
    nchan = x.shape[1]
    cps = nchan // nsub
    cum = bg.prefix_sums(x)
    out = {True: np.empty((len(dl) * len(bands), n), np.float32), False: np.empty((len(dl) * len(bands), n), np.float32)}
    for i, d in enumerate(dl):
        parts = [window_band_parts(cum, d, n, s * cps, (s + 1) * cps) for s in range(nsub)]
        A = np.concatenate([np.zeros((1, n), np.int64), np.cumsum([p[0] for p in parts], axis=0)])
        B = np.concatenate([np.zeros((1, n), np.int64), np.cumsum([p[1] for p in parts], axis=0)])
        for j, (lo, hi) in enumerate(bands):
            for zerodm in (True, False):
                out[zerodm][i * len(bands) + j] = band_value(A[hi] - A[lo], B[hi] - B[lo], nchan, zerodm)
    return out


def want_bands(br, prod, dms, nsub, clip, ncmp, tsamp=None):
    """-> (nout, nclip, bands, {zerodm: [(t0, plane [ndm * nband][ncmp])]}) for the runs br.runs(maxd, ncmp) and the last ncmp
    outputs; the clip is big_rows.clip_of's"""
    dl = bg.delays_of(br, dms, tsamp)
    maxd = max(int(d.max()) for d in dl)
    nout = br.nrows - maxd
    bands = bo.band_list(nsub)
    flag, repl, nclip = bg.clip_of(br, prod, clip)
    out = {True: [], False: []}
    for t0, n in br.runs(maxd, ncmp) + [(nout - ncmp, ncmp)]:
        x = br.window(t0, n + maxd)[:, prod, :]
        if flag is not None:
            x[flag[t0: t0 + n + maxd]] = repl.astype(x.dtype)
        planes = band_planes(x, dl, n, nsub, bands)
        for zerodm in (True, False):
            out[zerodm].append((t0, planes[zerodm]))
    return nout, nclip, bands, out


def bands_device(lib, res, prod, dms, nsub, zerodm, clip, nout, tsamp=None):
    """frbch_dedisperse_bands_device on the resident rows -> (the output buffer [ndm * nband][nout] float32, nclip, kernel_used,
    frbch_dedisperse_bands_kernel)"""
    br = res.br
    desc = br.desc(prod, tsamp)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    bp = post.band_params(nsub)
    nband = len(bo.band_list(nsub))
    ptr = C.c_void_p(res.address)
    query = lib.frbch_dedisperse_bands_kernel(C.byref(desc), ptr, br.nrows, dm_arr.ctypes.data, dm_arr.size, C.byref(bp))
    d_out = bg.out_buffer(res.mem, dm_arr.size * nband * nout * 4)
    nclip, used = C.c_uint64(0), C.c_uint32(99)
    err = C.create_string_buffer(512)
    with bg.guarded():
        code = lib.frbch_dedisperse_bands_device(C.byref(desc), ptr, br.nrows, dm_arr.ctypes.data, dm_arr.size, 1 if zerodm else 0, float(clip),
                                                 C.byref(bp), 0, d_out.ptr, nout, C.byref(nclip), C.byref(used), err, len(err))
    assert code == 0, err.value
    return d_out, nclip.value, used.value, query


def check_bands(lib, res, prod, dms, nsub, zerodm, clip, form, want, tsamp=None):
    """nclip and the compared runs of every series against `want` (want_bands), and band [0, nsub) against frbch_dedisperse_device
    of the same build at the same runs"""
    nout, wclip, bands, runs = want
    nband = len(bands)
    d_out, nclip, used, query = bands_device(lib, res, prod, dms, nsub, zerodm, clip, nout, tsamp)
    try:
        assert used == query == form, (used, query, form)
        assert nclip == wclip
        d_out.check()
        full = bands.index((0, nsub))
        d_full, fclip, _k = bg.dedisp_device(lib, res, prod, dms, zerodm, clip, nout, tsamp)
        try:
            assert fclip == wclip
            for t0, plane in runs[bool(zerodm)]:
                n = plane.shape[1]
                for s in range(len(dms) * nband):
                    got = bg.read_series(res.mem, d_out, nout, s, t0, n)
                    assert np.array_equal(got, plane[s]), "DM %d, band %s, outputs %d .. %d" % (s // nband, bands[s % nband], t0, t0 + n)
                for i in range(len(dms)):
                    assert np.array_equal(bg.read_series(res.mem, d_out, nout, i * nband + full, t0, n), bg.read_series(res.mem, d_full, nout, i, t0, n))
        finally:
            d_full.free()
    finally:
        d_out.free()
    res.check_equals()


# ---- the band search ------------------------------------------------------------------------------------------------------------
SEARCH_WIDTHS, SEARCH_THR, SEARCH_L = (1, 2, 4, 8), 8.0, 1000
BURST_DM, BURST_WIDTH, BURST_AMP, BURST_SUBS = 104.0, 4, 3, (2, 4)


def write_band_burst(res, prod, dm, t_top, width, amp, c_lo, c_hi, tsamp=None):
    """big_rows.write_burst in the channels [c_lo, c_hi) only: the burst would reach the top of the band at row t_top"""
    br = res.br
    d = bg.delays_of(br, [dm], tsamp)[0]
    c = np.arange(c_lo, c_hi)
    first = int(d[c].min())
    n = int(d[c].max()) - first + width
    rows = res.window(t_top + first, n)
    for k in range(width):
        rows[d[c] - first + k, prod, c] += amp * (201 if br.nbits == 16 else 1)
    res.poke(t_top + first, rows)


def bandsearch_device(lib, res, prod, dms, nsub, zerodm, clip, sp, plane_bytes, nout, cap=1 << 16, tsamp=None):
    """frbch_bandsearch_device -> (records, nclip, kernel_used[2], batches)"""
    br = res.br
    desc = br.desc(prod, tsamp)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    bp = post.band_params(nsub)
    cands = np.zeros(cap, dtype=post.SPB_CAND)
    ncand, nclip, nbatch = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    used = (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    with bg.guarded():
        code = lib.frbch_bandsearch_device(C.byref(desc), C.c_void_p(res.address), br.nrows, dm_arr.ctypes.data, dm_arr.size, 1 if zerodm else 0,
                                           float(clip), C.byref(bp), C.byref(sp), plane_bytes, 0, nout, C.byref(nclip), cands.ctypes.data, cap,
                                           C.byref(ncand), used, C.byref(nbatch), None, err, len(err))
    assert code == 0, err.value
    assert ncand.value <= cap
    return cands[: ncand.value], nclip.value, (used[0], used[1]), nbatch.value


def records_of_plane(recs, bands):
    """the records of frbch_spsearch_device on the plane [ndm * nband][nout] as frbch_bandsearch_* lists them (bands_oracle.search's
    renumbering and order)"""
    out = np.zeros(recs.size, dtype=post.SPB_CAND)
    nband = len(bands)
    ab = np.array(bands, dtype=np.int64).reshape(-1, 2)
    for k in ("width", "sample", "sigma"):
        out[k] = recs[k]
    out["dm_index"] = recs["dm_index"] // nband
    out["sub_lo"] = ab[recs["dm_index"] % nband, 0]
    out["sub_hi"] = ab[recs["dm_index"] % nband, 1]
    return out[np.lexsort((out["width"], out["sample"], out["sub_hi"], out["sub_lo"], out["dm_index"]))]


def check_bandsearch(lib, res, prod, dms, nsub, form, behind, tsamp=None):
    """a burst of BURST_WIDTH rows at BURST_DM in the sub-bands BURST_SUBS only, `behind` rows behind the last byte mark: the
    records whatever the batch, against the library's own stages, and where the strongest group lies"""
    br = res.br
    cps = br.nchan // nsub
    t_top = br.byte_mark_rows[-1] + behind
    write_band_burst(res, prod, BURST_DM, t_top, BURST_WIDTH, BURST_AMP, BURST_SUBS[0] * cps, BURST_SUBS[1] * cps, tsamp)
    sp = post.sp_params(list(SEARCH_WIDTHS), SEARCH_THR, SEARCH_L)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    nout = lib.frbch_dedisperse_nout(C.byref(br.desc(prod, tsamp)), br.nrows, dm_arr.ctypes.data, dm_arr.size)
    bands = bo.band_list(nsub)
    one_dm = len(bands) * nout * 4
    whole, nclip, used, nbatch = bandsearch_device(lib, res, prod, dms, nsub, True, 5.0, sp, 0, nout, tsamp=tsamp)
    cut, nclip3, used3, nbatch3 = bandsearch_device(lib, res, prod, dms, nsub, True, 5.0, sp, 3 * one_dm, nout, tsamp=tsamp)
    assert nbatch3 == -(-len(dms) // 3) and nbatch <= nbatch3 and nclip == nclip3
    assert used == used3 and used[0] == form, (used, used3, form)
    assert whole.size > 0 and whole.tobytes() == cut.tobytes()
    d_out, pclip, k, _q = bands_device(lib, res, prod, dms, nsub, True, 5.0, nout, tsamp)
    try:
        recs, _n, k_sp = bg.spsearch_device(lib, d_out.ptr.value, len(dms) * len(bands), nout, sp, cap=1 << 16)
    finally:
        d_out.free()
    assert k == form and pclip == nclip and k_sp == used[1]
    assert records_of_plane(recs, bands).tobytes() == whole.tobytes()
    groups = post.group_band_candidates(whole, br.hdr(tsamp), dms, nsub=nsub, dm_gap=2, lib=lib)
    best = groups[np.argmax(groups["best"]["sigma"])]["best"]
    assert (int(best["sub_lo"]), int(best["sub_hi"])) == BURST_SUBS and int(best["dm_index"]) == list(dms).index(BURST_DM), best
    assert int(best["width"]) == BURST_WIDTH and abs(int(best["sample"]) - (t_top + BURST_WIDTH // 2)) <= 1, best
    res.check_equals()
    return whole, groups
