"""Numpy restatement of the single-pulse search (frbch_spsearch_*): the arithmetic include/frbch.h states, step by step,
with nothing shared with the library.  Doubles are added in the stated order (64 partial sums per block, position j, j + 64,
... ascending, then the partials in ascending j; numpy adds elementwise, never contracted), everything after the
quantisation is int64.  Slow and plain on purpose: the tests compare the library with it record for record."""
import math

import numpy as np

CAND = np.dtype([("dm_index", "<u4"), ("width", "<u4"), ("sample", "<u8"), ("sigma", "<f4"), ("reserved", "<u4")])
NPART = 64


def block_edges(nout, detrend_len=0):
    L = detrend_len or 1000
    nblk = max(1, nout // L)
    return [(b * L, nout if b == nblk - 1 else (b + 1) * L) for b in range(nblk)]


def _moments(x, keep):
    """x, keep: [ndm][n] of one block -> mean, sigma [ndm] (sigma 0 where var > 0 is false or nothing is kept)"""
    ndm, n = x.shape
    rows = -(-n // NPART)
    xp = np.zeros((ndm, rows * NPART))
    kp = np.zeros((ndm, rows * NPART), dtype=bool)
    xp[:, :n] = x
    kp[:, :n] = keep
    xp, kp = xp.reshape(ndm, rows, NPART), kp.reshape(ndm, rows, NPART)
    s1, s2, cnt = np.zeros((ndm, NPART)), np.zeros((ndm, NPART)), np.zeros((ndm, NPART))
    for r in range(rows):                                  # partial j: positions j, j + 64, ... in ascending order
        v, k = xp[:, r, :], kp[:, r, :]
        with np.errstate(invalid="ignore", over="ignore"):
            s1 = np.where(k, s1 + v, s1)
            s2 = np.where(k, s2 + v * v, s2)
        cnt = cnt + k
    a1, a2, an = np.zeros(ndm), np.zeros(ndm), np.zeros(ndm)
    for j in range(NPART):                                 # the partials in ascending j
        with np.errstate(invalid="ignore"):
            a1, a2, an = a1 + s1[:, j], a2 + s2[:, j], an + cnt[:, j]
    mean, sig = np.zeros(ndm), np.zeros(ndm)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        some = an > 0
        m = a1 / np.where(some, an, 1.0)
        var = a2 / np.where(some, an, 1.0) - m * m
        good = some & (var > 0)                            # a NaN compares false
        mean = np.where(some, m, 0.0)
        sig = np.where(good, np.sqrt(np.where(good, var, 1.0)), 0.0)
    return mean, sig


def quantise(series, detrend_len=0):
    """-> (q int64 [ndm][nout], dead bool [ndm][nblk])"""
    x = np.asarray(series, dtype=np.float32).astype(np.float64)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    ndm, nout = x.shape
    q = np.zeros((ndm, nout), dtype=np.int64)
    edges = block_edges(nout, detrend_len)
    dead = np.zeros((ndm, len(edges)), dtype=bool)
    for b, (lo, hi) in enumerate(edges):
        xb = x[:, lo:hi]
        mean1, sig1 = _moments(xb, np.ones(xb.shape, dtype=bool))
        with np.errstate(invalid="ignore"):
            keep = np.abs(xb - mean1[:, None]) <= (3.0 * sig1)[:, None]
        keep &= (sig1 > 0)[:, None]
        mean2, sig2 = _moments(xb, keep)
        live = (sig1 > 0) & keep.any(axis=1) & (sig2 > 0)
        dead[:, b] = ~live
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            inv = 1.0 / np.where(live, sig2, 1.0)
            z = (xb - mean2[:, None]) * inv[:, None]
            z = np.minimum(np.maximum(z, -65536.0), 65536.0)
            qq = np.floor(z * 1024.0 + 0.5)
        qq = np.where(live[:, None], qq, 0.0)              # (a dead block may hold NaN)
        q[:, lo:hi] = np.nan_to_num(qq).astype(np.int64)
    return q, dead


def threshold_sum(threshold, w):
    return int(math.ceil((float(threshold) * 1024.0) * math.sqrt(float(w))))


def boxcar(q, w):
    """S_w[t], 0 <= t <= nout - w, of one DM"""
    c = np.concatenate([[0], np.cumsum(q, dtype=np.int64)])
    return c[w:] - c[:-w]


def raw_peaks(q, widths, threshold):
    """one DM -> list of (t, w, S)"""
    out = []
    nout = q.size
    for w in widths:
        if w > nout:
            continue
        s = boxcar(q, w)
        h = w // 2
        for t in np.nonzero(s >= threshold_sum(threshold, w))[0]:
            lo, hi = max(0, t - h), min(s.size - 1, t + h)
            if np.all(s[t] > s[lo:t]) and np.all(s[t] >= s[t + 1:hi + 1]):
                out.append((int(t), int(w), int(s[t])))
    return out


def sigma_of(s, w):
    return float(s) / (1024.0 * math.sqrt(float(w)))


def sift(raw):
    """step 5 on the raw list of one DM, one pass -> survivors as (centre, w, sigma)"""
    pk = [(t + w // 2, w, sigma_of(s, w)) for t, w, s in raw]
    keep = []
    for i, (c, w, sg) in enumerate(pk):
        dropped = False
        for j, (c2, w2, sg2) in enumerate(pk):
            if j == i or abs(c - c2) > max(w, w2) // 2:
                continue
            if sg2 > sg or (sg2 == sg and (w2 < w or (w2 == w and c2 < c))):
                dropped = True
                break
        if not dropped:
            keep.append((c, w, sg))
    return keep


def search(series, widths, threshold, detrend_len=0, want_raw=False):
    """-> candidates (CAND records sorted by dm index, sample, width) [, the raw lists per DM]"""
    widths = [int(w) for w in widths]
    assert 1 <= len(widths) <= 16 and all(1 <= w <= 1024 for w in widths) and all(a < b for a, b in zip(widths, widths[1:]))
    q, _dead = quantise(series, detrend_len)
    rows, raws = [], []
    for d in range(q.shape[0]):
        raw = raw_peaks(q[d], widths, threshold)
        raws.append(raw)
        for c, w, sg in sorted(sift(raw)):
            rows.append((d, w, c, np.float32(sg), 0))
    out = np.array(rows, dtype=CAND) if rows else np.zeros(0, dtype=CAND)
    out = out[np.lexsort((out["width"], out["sample"], out["dm_index"]))]
    return (out, raws) if want_raw else out
