"""Numpy restatement of the acceleration search (frbch_resample_*, frbch_pasearch_*, frbch_pa_group_cands): the index rule
include/frbch.h states, the search of every trial by calling tests/psearch_oracle.search on the resampled plane y[:, u], and
the grouping across DMs and trials.  Nothing is shared with the library."""
import functools

import numpy as np

from tests import psearch_oracle as pso

C_LIGHT = 299792458.0
CAND = np.dtype([("dm_index", "<u4"), ("acc_index", "<u4"), ("h", "<u4"), ("k", "<u4"), ("power", "<f4"), ("reserved", "<u4"),
                 ("sigma", "<f8"), ("freq_hz", "<f8"), ("acc_ms2", "<f8")])
GROUP = np.dtype([("best", CAND), ("nmember", "<u4"), ("dm_index_lo", "<u4"), ("dm_index_hi", "<u4"), ("acc_index_lo", "<u4"),
                  ("acc_index_hi", "<u4"), ("reserved", "<u4")])


def q_of(a, tsamp):
    return (float(a) * float(tsamp)) / (2.0 * 299792458.0)


def accepted(a, n, tsamp):
    return bool(np.isfinite(a)) and abs(q_of(a, tsamp)) * float(n) <= 0.5


def index_of_q(n, q):
    """u(t) = t + (int64) rint(q * (double)(t (t - n))), t = 0 .. n - 1: np.rint rounds ties to even, the product of the two
    integers is exact in int64, and one double multiplication follows"""
    t = np.arange(n, dtype=np.int64)
    g = np.rint(np.float64(q) * (t * (t - np.int64(n))).astype(np.float64))
    return t + g.astype(np.int64)


def index(n, a, tsamp):
    assert accepted(a, n, tsamp)
    return index_of_q(n, q_of(a, tsamp))


def resample(series, n, tsamp, accs):
    """-> [nacc][ndm][n] float32: numpy indexing, the bytes of the input"""
    x = np.asarray(series, dtype=np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    return np.stack([x[:, :n][:, index(n, a, tsamp)] for a in accs])


def search(series, tsamp, accs, nfft=0, **kw):
    """-> CAND records sorted by (acc_index, dm_index, h, k): psearch_oracle.search on every trial's plane [ndm][n]"""
    x = np.asarray(series, dtype=np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    n = pso.nfft_of(x.shape[1], nfft)
    out = []
    for i, a in enumerate(accs):
        plane = np.ascontiguousarray(x[:, :n][:, index(n, a, tsamp)])
        for r in pso.search(plane, tsamp, nfft=n, **kw).tolist():
            out.append((r[0], i, r[1], r[2], r[3], 0, r[4], r[5], float(a)))
    return np.array(out, dtype=CAND) if out else np.zeros(0, dtype=CAND)


def group(cands, dm_gap=2, acc_gap=1):
    """-> GROUP records sorted by best.sigma descending, then f, dm_index, acc_index, h"""
    c = [tuple(r) for r in np.asarray(cands, dtype=CAND).tolist()]
    DM, ACC, H, K, SIG = 0, 1, 2, 3, 6
    parent = list(range(len(c)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, a in enumerate(c):
        for j in range(i + 1, len(c)):
            b = c[j]
            if (abs(a[DM] - b[DM]) <= dm_gap and abs(a[ACC] - b[ACC]) <= acc_gap and
                    2 * abs(a[K] * b[H] - b[K] * a[H]) <= 3 * a[H] * b[H]):
                ra, rb = find(i), find(j)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    groups = {}
    for i, a in enumerate(c):
        groups.setdefault(find(i), []).append(a)
    out = []
    for members in groups.values():
        best = sorted(members, key=lambda r: (-r[SIG], r[H], r[DM], r[ACC], r[K]))[0]
        out.append((best, len(members), min(m[DM] for m in members), max(m[DM] for m in members),
                    min(m[ACC] for m in members), max(m[ACC] for m in members), 0))

    def order(x, y):
        a, b = x[0], y[0]
        if a[SIG] != b[SIG]:
            return -1 if a[SIG] > b[SIG] else 1
        fa, fb = a[K] * b[H], b[K] * a[H]
        if fa != fb:
            return -1 if fa < fb else 1
        for f in (DM, ACC, H):
            if a[f] != b[f]:
                return -1 if a[f] < b[f] else 1
        return 0
    out.sort(key=functools.cmp_to_key(order))
    return np.array(out, dtype=GROUP) if out else np.zeros(0, dtype=GROUP)
