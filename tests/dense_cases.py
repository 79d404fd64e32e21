"""Dense cases of the three search stages (frbch_psearch_*, frbch_pasearch_*, frbch_spsearch_*), for tests/test_search_dense.py
on the emulator and tests/test_gpu_search_dense.py on the device.

A record exists only where something crosses a threshold, so a comparison "record for record" at 3 to 7 sigma looks at a few
bins in a thousand.  Here the threshold is so low that the records ARE the spectrum:

* periodicity search, nharm = 1, sigma = SIGMA = 0.01 (T_1 = 0.7011579): every local maximum of p above T_1 is a record whose
  `power` is the float bits of p[k].  Step 8 drops nothing at h = 1 -- it drops records within one bin of each other, and two
  local maxima are never adjacent (strict `>` to the left, `>=` to the right) -- so the expectation is psearch_oracle.powers,
  normalise and raw_peaks, without the quadratic `sift` (test_search_dense.py proves the claim once with `sift` at n = 4096).
  0.29 of all searched bins become bit-exact records, both neighbours of each are held by the inequality, and every block level
  by the ~37 records that divide by it.
* single-pulse search, one width per call, threshold THR = 1e-6 (threshold sum 1): with width 1 every sample with q >= 1 is a
  record with sigma = float32(q / 1024), half of all samples; with one width w every window maximum of S_w is a record, and step
  5 drops nothing (two maxima of one width lie more than w / 2 apart; held with spsearch_oracle.sift on short raw lists).

Every case asserts on the oracle alone, before the library runs, that the raw count is below 2^20 and that at least MIN_SHARE
of the searched bins of every lit series are records (MIN_SHARE_W1 of the samples of live blocks at width 1) -- conditions, so that
a later edit of a case cannot quietly turn it sparse.  The comparisons say what differs: how many records are missing, extra or
differ in bits, and the first differing (dm, h, k) / (acc, dm, h, k) / (dm, w, t)."""
import collections
import functools
import math

import numpy as np
from scipy.special import erfc

from tests import accel_cases as ac
from tests import accel_oracle as ao
from tests import psearch_cases as pc
from tests import psearch_oracle as pso
from tests import spsearch_cases as sc
from tests import spsearch_oracle as so
from tests.hipmem import HostGuardedBuffer, guarded_for

SIGMA = 0.01                       # T_1 = 0.7011579: exp(-T_1) = 0.496, the one-sided tail of 0.01 sigma
THR = 1e-6                         # ceil(1e-6 * 1024 * sqrt(w)) = 1 for every width up to 1024
MIN_SHARE = 0.25                   # of the searched bins of a lit series (measured: 0.293 .. 0.294 at h = 1)
MIN_SHARE_W1 = 0.4                 # of the samples of live blocks, single-pulse width 1 (measured: 0.46)
FAST, GENERIC = 1, 0
T64 = 64e-6


def is_emulator(lib):
    return guarded_for(lib) is HostGuardedBuffer


# ---- the documented plan of the fast transform ----------------------------------------------------------------------
def passes_of(n):
    """one LDS-resident pass up to 2^13, two up to 2^18, three above"""
    return 1 if n <= 1 << 13 else 2 if n <= 1 << 18 else 3


def stages_of(L):
    """how the log2 n stages are dealt to the passes: the first pass takes the larger share"""
    if L <= 13:
        return (L,)
    if L <= 18:
        return ((L + 1) // 2, L - (L + 1) // 2)
    a = (L + 2) // 3
    b = (L - a + 1) // 2
    return (a, b, L - a - b)


def register_passes(R):
    """the R stages of a pass as register passes of 3 stages, the last ones 2 where 3 does not divide R"""
    out = []
    while R:
        chunks = (R + 2) // 3
        rr = (R + chunks - 1) // chunks
        out.append(rr)
        R -= rr
    return tuple(out)


def forms(lib, n):
    """-> [(misalign, (form, passes) expected)]: the fast form at the 16-byte aligned address and the generic one a float
    further on; the emulator build has the generic form alone"""
    if is_emulator(lib):
        return [(False, (GENERIC, 0)), (True, (GENERIC, 0))]
    return [(False, (FAST, passes_of(n))), (True, (GENERIC, 0))]


# ---- sigma of step 8 at h = 1, for a million records ----------------------------------------------------------------
def _log_tail(s):
    with np.errstate(all="ignore"):
        out = np.log(0.5 * erfc(s / math.sqrt(2.0)))
    far = np.flatnonzero(~(s < 30.0))
    if far.size:
        f = s[far]
        f2 = f * f
        out[far] = -0.5 * f2 - np.log(f) - 0.5 * math.log(2.0 * math.pi) + np.log1p(-1.0 / f2 + 3.0 / (f2 * f2))
    return out


def sigma_h1(H):
    """psearch_oracle.sigma_of(1, H) on an array: log Q(1, x) is -x on both branches of log_q (the sum is 1.0, its logarithm
    0.0), and the 64 bisection steps are the same steps on vectors.  erfc is scipy's, not the C library's: a few units in
    the last place of the tail move sigma by 1e-16 absolute (d lt / d s is -0.8 at s = 0 and falls from there), 1e-14 of the
    smallest sigma here; ps_dense holds a sample of every case to sigma_of itself at 1e-12, a thousandth of SIGMA_RTOL"""
    x = np.minimum(np.asarray(H, dtype=np.float64), float(np.finfo(np.float32).max))
    lq = -x
    lo, hi = np.zeros_like(x), np.sqrt(-2.0 * lq) + 2.0
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        up = _log_tail(mid) > lq
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return np.where(lq < 0.0, 0.5 * (lo + hi), 0.0)


# ---- periodicity search ---------------------------------------------------------------------------------------------
# want: CAND records in output order; nraw: raw peaks of the whole call; share[d]: records of series d per searched bin;
# lit[d]: series d has a nonzero p (a dead or constant series has none and must give no record)
PsCase = collections.namedtuple("PsCase", "y tsamp kw want n kmin nraw share lit")


def ps_dense(y, tsamp, flo=0.0, nfft=0, wblock=0):
    """the expectation at nharm = 1, sigma = SIGMA without `sift` -> PsCase"""
    n = pso.nfft_of(y.shape[1], nfft)
    N, _live = pso.powers(y, n)
    kmin = pso.kmin_of(n, tsamp, flo)
    p = pso.normalise(N, n, wblock, kmin)
    raw = pso.raw_peaks(p, kmin, 1, pso.thresholds(SIGMA))
    want = np.zeros(len(raw), dtype=pso.CAND)
    if raw:
        d, h, k, H = zip(*raw)
        want["dm_index"], want["h"], want["k"], want["power"] = d, h, k, np.array(H, dtype=np.float32)
        want["sigma"] = sigma_h1(want["power"])
        want["freq_hz"] = want["k"].astype(np.float64) / (1.0 * (float(n) * tsamp))
        for i in np.unique(np.linspace(0, want.size - 1, 64).astype(np.int64)).tolist() + [int(np.argmax(want["power"]))]:
            ref = pso.sigma_of(1, want["power"][i])
            assert abs(want["sigma"][i] - ref) <= 1e-12 * ref, (i, want["sigma"][i], ref)
    kw = dict(sigma=SIGMA, nharm=1, flo=flo, nfft=nfft, wblock=wblock)
    share = np.bincount(want["dm_index"], minlength=y.shape[0]) / float(n // 2 - kmin)
    y.setflags(write=False)
    want.setflags(write=False)
    return PsCase(y, tsamp, kw, want, n, kmin, len(raw), share, (p > 0).any(axis=1))


def ps_folds(y, tsamp, nharm, flo):
    """the oracle's full search at sigma = SIGMA with all folds up to nharm (small n: `sift` is quadratic) -> PsCase"""
    n = pso.nfft_of(y.shape[1])
    kmin = pso.kmin_of(n, tsamp, flo)
    want, raw = pso.search(y, tsamp, sigma=SIGMA, nharm=nharm, flo=flo, want_raw=True)
    share = np.bincount(want["dm_index"], minlength=y.shape[0]) / float(n // 2 - kmin)
    y.setflags(write=False)
    want.setflags(write=False)
    return PsCase(y, tsamp, dict(sigma=SIGMA, nharm=nharm, flo=flo), want, n, kmin, len(raw), share, np.ones(y.shape[0], dtype=bool))


def ps_conditions(case, quiet=()):
    """what every dense case asserts on the oracle alone, before the library is called"""
    assert case.nraw < pso.RAW_CAP, case.nraw
    assert [d for d in range(case.y.shape[0]) if not case.lit[d]] == sorted(quiet), (case.lit, quiet)
    for d in range(case.y.shape[0]):
        if d in quiet:
            assert case.share[d] == 0.0, (d, case.share[d])
        else:
            assert case.share[d] >= MIN_SHARE, (d, case.share[d])


# the lengths: L -> (ndm, samples beyond n).  ndm alternates between even and odd, so that the zero partner of an odd last
# series appears in every pass structure (13; 15 and 17; 19 and 22); the raw cap leaves two series at 2^21 and one at 2^22;
# nout = n + 5 at the odd L: rows that are not 16-byte aligned, and a tail
PS_GRID = {12: (2, 0), 13: (3, 5), 14: (2, 0), 15: (3, 5), 16: (2, 0), 17: (3, 5), 18: (2, 0), 19: (3, 5), 20: (2, 0), 21: (2, 5),
           22: (1, 0)}


@functools.lru_cache(maxsize=None)
def ps_length(L):
    ndm, extra = PS_GRID[L]
    return ps_dense(pc.signals(ndm, (1 << L) + extra, 200 + L, T64), T64)


@functools.lru_cache(maxsize=None)
def ps_wblock(L, B):
    """B = 32: a workgroup of the level kernel owns 256 blocks; B = 1024: 8, and its last workgroup the long last block"""
    return ps_dense(pc.signals(3 if L <= 14 else 2, 1 << L, 230 + L, T64), T64, wblock=B)


@functools.lru_cache(maxsize=None)
def ps_kmin_inside(L):
    """kmin = 100 with B = 128: inside block 0 = [1, 129).  p is 0 below kmin, the level still counts those bins"""
    tsamp, flo = {12: (pc.TSAMP, 24.3), 15: (T64, 47.5)}[L]
    case = ps_dense(pc.signals(3, 1 << L, 250 + L, tsamp), tsamp, flo=flo)
    assert case.kmin == 100 and pso.block_edges(case.n // 2 - 1, 128)[0] == (1, 129)
    return case


DEAD_QUIET = (0, 3, 4)


@functools.lru_cache(maxsize=None)
def ps_dead(L):
    """a NaN series beside a live one (0, 1), a live one beside an Inf series (2, 3), a constant one beside a live one (4, 5)"""
    tsamp = pc.TSAMP if L == 12 else T64
    y = pc.signals(6, 1 << L, 260 + L, tsamp)
    y[0, 1234] = np.nan
    y[3, 77] = np.inf
    y[4] = np.float32(7.0)
    return ps_dense(y, tsamp)


@functools.lru_cache(maxsize=None)
def ps_all_folds():
    """all five folds at n = 4096, kmin = 5: every survivor is a 1-, 2-, 4-, 8- or 16-term float sum held to the bit"""
    return ps_folds(pc.signals(2, 4096, 41), pc.TSAMP, 16, 1.2)


@functools.lru_cache(maxsize=None)
def ps_fold_edge(nharm):
    """the edges of the harmonic sums: a train of one-sample pulses with period n / kmin in series 0 and 2 -- the record
    (h, h kmin) is the FIRST bin of fold h, where no left neighbour is tested -- and a sine at bin n / 2 - 1 in series 1, the
    LAST bin, with no right neighbour"""
    y = pc.noise(3, 4096, 91)
    for d in (0, 2):
        pc.add_train(y, d, 4096 / 5, 3.0, 400.0)
    pc.add_sine(y, 1, 2047 / 4.096, 3.0)
    case = ps_folds(y, pc.TSAMP, nharm, 1.2)
    assert case.kmin == 5
    found = {(int(r["dm_index"]), int(r["h"]), int(r["k"])) for r in case.want}
    assert {(0, nharm, 5 * nharm), (2, nharm, 5 * nharm), (1, 1, 2047)} <= found, sorted(found)[:8]
    return case


def _ps_key(r):
    return (r["dm_index"].astype(np.int64) * 17 + r["h"]) * (1 << 22) + r["k"]


def _ps_label(key):
    return "(dm, h, k) = (%d, %d, %d)" % ((key >> 22) // 17, (key >> 22) % 17, key & ((1 << 22) - 1))


def _pa_key(r):
    return ((r["acc_index"].astype(np.int64) * 65536 + r["dm_index"]) * 17 + r["h"]) * (1 << 22) + r["k"]


def _pa_label(key):
    top = key >> 22
    return "(acc, dm, h, k) = (%d, %d, %d, %d)" % (top // 17 // 65536, top // 17 % 65536, top % 17, key & ((1 << 22) - 1))


def _sp_key(r):
    return (r["dm_index"].astype(np.int64) * (1 << 32) + r["sample"].astype(np.int64)) * 2048 + r["width"]


def _sp_label(key):
    w, c = key % 2048, (key >> 11) % (1 << 32)
    return "(dm, w, t) = (%d, %d, %d)" % (key >> 43, w, c - w // 2)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view("u%d" % a.dtype.itemsize) if a.dtype.kind == "f" else a


def differences(got, want, key_of, label_of, exact, close=()):
    """-> "" when the two record lists are equal (the fields `exact` to the bit, the fields `close` to
    psearch_oracle.SIGMA_RTOL), else what differs: the counts of missing and extra records and of records that differ per
    field, and the first differing key with both records"""
    if got.dtype != want.dtype:
        return "record type %s, expected %s" % (got.dtype, want.dtype)
    kg, kw = key_of(got), key_of(want)
    notes = []
    if np.any(np.diff(kg) <= 0):
        notes.append("%d records out of output order or twice" % int(np.count_nonzero(np.diff(kg) <= 0)))
    missing, extra = np.setdiff1d(kw, kg), np.setdiff1d(kg, kw)
    _common, ig, iw = np.intersect1d(kg, kw, return_indices=True)
    g, w = got[ig], want[iw]
    bad = np.zeros(g.size, dtype=bool)
    fields = []
    for f in exact:
        b = _bits(g[f]) != _bits(w[f])
        if b.any():
            fields.append("%s in %d" % (f, int(b.sum())))
        bad |= b
    for f in close:
        with np.errstate(invalid="ignore"):
            b = ~(np.abs(g[f] - w[f]) <= pso.SIGMA_RTOL * np.abs(w[f]))
        if b.any():
            fields.append("%s beyond %g in %d" % (f, pso.SIGMA_RTOL, int(b.sum())))
        bad |= b
    if not (notes or missing.size or extra.size or bad.any()):
        return ""
    firsts = [int(x[0]) for x in (missing, extra, kw[iw][bad]) if x.size]
    first = min(firsts) if firsts else None
    text = "%d records, %d expected: %d missing, %d extra, %d of the %d common ones differ (%s)" % (
        got.size, want.size, missing.size, extra.size, int(bad.sum()), g.size, ", ".join(fields) or "none")
    if first is not None:
        text += "; first at %s: got %s, expected %s" % (label_of(first), got[kg == first].tolist(), want[kw == first].tolist())
    return "; ".join(notes + [text])


def ps_differences(got, want):
    return differences(got, want, _ps_key, _ps_label, ("dm_index", "h", "k", "power"), ("sigma", "freq_hz"))


def pa_differences(got, want):
    return differences(got, want, _pa_key, _pa_label, ("dm_index", "acc_index", "h", "k", "power", "reserved", "acc_ms2"), ("sigma", "freq_hz"))


def sp_differences(got, want):
    return differences(got, want, _sp_key, _sp_label, ("dm_index", "width", "sample", "sigma", "reserved"))


def ps_hold(lib, case, quiet=(), aligned_only=False):
    """the conditions on the oracle, then the library in both forms against the one expectation"""
    ps_conditions(case, quiet)
    for misalign, plan in forms(lib, case.n)[: 1 if aligned_only else 2]:
        got, used = pc.device_search(lib, case.y, case.tsamp, misalign=misalign, cap=case.want.size + 16, **case.kw)
        assert used == plan, (used, plan)
        report = ps_differences(got, case.want)
        assert not report, "%s form: %s" % ("generic" if plan[0] == GENERIC else "fast", report)


# ---- acceleration search --------------------------------------------------------------------------------------------
PaCase = collections.namedtuple("PaCase", "y tsamp accs kw want n nraw share")


def pa_dense(y, tsamp, accs):
    """per trial: accel_oracle.resample, then ps_dense on that plane -> PaCase (share: [trial][series])"""
    accs = np.ascontiguousarray(accs, dtype=np.float64)
    n = pso.nfft_of(y.shape[1])
    planes = ao.resample(y, n, tsamp, accs)
    parts, shares, nraw = [], [], 0
    for i, a in enumerate(accs):
        c = ps_dense(np.ascontiguousarray(planes[i]), tsamp, nfft=n)
        part = np.zeros(c.want.size, dtype=ao.CAND)
        for f in ("dm_index", "h", "k", "power", "sigma", "freq_hz"):
            part[f] = c.want[f]
        part["acc_index"], part["acc_ms2"] = i, a
        parts.append(part)
        shares.append(c.share)
        nraw += c.nraw
    want = np.concatenate(parts)
    y.setflags(write=False)
    want.setflags(write=False)
    return PaCase(y, tsamp, accs, dict(sigma=SIGMA, nharm=1), want, n, nraw, np.array(shares))


def pa_conditions(case):
    """nraw is that of ALL trials: below the cap even when they share a batch"""
    assert case.nraw < pso.RAW_CAP and np.all(case.share >= MIN_SHARE), (case.nraw, case.share)
    assert not np.any(case.want["dm_index"] >= case.y.shape[0])


def pa_hold(lib, case, batch_rows=(0,)):
    """the conditions on the oracle, then the library with every batch_rows: the expectation each time, and the same bytes"""
    pa_conditions(case)
    plan = (GENERIC, GENERIC, 0) if is_emulator(lib) else (FAST if case.y.shape[1] % 4 == 0 else GENERIC, FAST, passes_of(case.n))
    first = None
    for rows in batch_rows:
        got, used = ac.device_search(lib, case.y, case.tsamp, case.accs, cap=case.want.size + 16, batch_rows=rows, **case.kw)
        assert used == plan, (used, plan)
        report = pa_differences(got, case.want)
        assert not report, "batch_rows %d: %s" % (rows, report)
        assert not np.any(got["dm_index"] >= case.y.shape[0])          # the zero row behind an odd ndm gives no record
        first = got if first is None else first
        assert got.tobytes() == first.tobytes(), rows


@functools.lru_cache(maxsize=None)
def pa_n14():
    return pa_dense(pc.signals(3, 1 << 14, 148, T64), T64, [-ac.A14, 0.0, ac.A14])


@functools.lru_cache(maxsize=None)
def pa_n19():
    """n tsamp = 33.6 s: the largest accepted |a| is 8.9e6; q n = +-0.22"""
    return pa_dense(pc.signals(2, (1 << 19) + 4, 281, T64), T64, [-4.0e6, 4.0e6])


# ---- single-pulse search --------------------------------------------------------------------------------------------
SpCase = collections.namedtuple("SpCase", "y width L want nraw live_samples")
SP_SHAPES = {"3dm_2tiles_5": (3, 2, 31), "9dm_3tiles_5": (9, 3, 32)}
SP_L = 1000
SP_WIDTHS = (1, 2, 16, 511, 512, 520, 1024)
SIFT_BELOW = 1000                  # raw peaks of one DM up to which spsearch_oracle.sift (quadratic) holds "step 5 drops nothing"


@functools.lru_cache(maxsize=None)
def sp_series(shape):
    """ndm x (tiles x 2048 + 5) samples, the TILE edges of spsearch_cases; a NaN kills block 1 of DM 0, the last block of the
    last DM is constant"""
    ndm, tiles, seed = SP_SHAPES[shape]
    nout = tiles * sc.TILE + 5
    y = sc.noise(ndm, nout, seed)
    y[0, 1500] = np.nan
    y[ndm - 1, (nout // SP_L - 1) * SP_L:] = np.float32(7.0)
    y.setflags(write=False)
    q, dead = so.quantise(y, SP_L)
    assert dead[0, 1] and dead[ndm - 1, -1] and dead.sum() == 2
    q.setflags(write=False)
    return y, q, dead


@functools.lru_cache(maxsize=None)
def sp_dense(shape, w):
    """the expectation with the one width w at THR from spsearch_oracle.quantise and raw_peaks: every raw peak is a record"""
    y, q, dead = sp_series(shape)
    assert so.threshold_sum(THR, w) == 1
    rows, nraw = [], 0
    for d in range(q.shape[0]):
        raw = so.raw_peaks(q[d], [w], THR)
        nraw += len(raw)
        if len(raw) < SIFT_BELOW:
            assert sorted(so.sift(raw)) == sorted((t + w // 2, w, so.sigma_of(s, w)) for t, _w, s in raw)
        rows += [(d, w, t + w // 2, np.float32(so.sigma_of(s, w)), 0) for t, _w, s in raw]
    want = np.array(rows, dtype=so.CAND)
    want = want[np.lexsort((want["width"], want["sample"], want["dm_index"]))]
    want.setflags(write=False)
    edges = so.block_edges(y.shape[1], SP_L)
    live = np.array([sum(hi - lo for (lo, hi), dd in zip(edges, dead[d]) if not dd) for d in range(q.shape[0])])
    return SpCase(y, w, SP_L, want, nraw, live)


def sp_conditions(case):
    assert case.nraw < 1 << 20
    per_dm = np.bincount(case.want["dm_index"], minlength=case.y.shape[0])
    assert np.all(per_dm >= 1), per_dm
    if case.width == 1:
        assert np.all(per_dm >= MIN_SHARE_W1 * case.live_samples), (per_dm, case.live_samples)


def sp_kernel(lib, w):
    return sc.LDS_MAX_WIDTH >= w and not is_emulator(lib)


def sp_hold(lib, case):
    """the LDS kernel up to width 512, the generic ones above; the address of the series does not enter the choice, and both
    addresses must give the records"""
    sp_conditions(case)
    for misalign in (False, True):
        got, used = sc.device_search(lib, case.y, [case.width], THR, case.L, misalign=misalign, cap=case.want.size + 16)
        assert used == (1 if sp_kernel(lib, case.width) else 0), (used, case.width)
        report = sp_differences(got, case.want)
        assert not report, "series %s: %s" % ("one float further on" if misalign else "aligned", report)
