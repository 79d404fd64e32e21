"""Numpy restatement of the periodicity search of the dedispersed series (frbch_psearch_*, frbch_ps_group_cands): the
arithmetic include/frbch.h states, step by step, with nothing shared with the library.  float32 operations are numpy's
element-wise ones (each rounded on its own, never contracted), doubles are added in the stated order.  Plain and literal on
purpose: the tests compare the library with it record for record, the integer fields and the float bits of H exactly.

sigma and freq_hz of a record are doubles that pass through exp / log / erfc of the C library (here: of Python's math); the
header says they are equal to the last bits only on the same library, so the tests hold them to SIGMA_RTOL."""
import math

import numpy as np

F32 = np.float32
NPART = 64
FOLDS = (1, 2, 4, 8, 16)
RAW_CAP = 1 << 20
CAND = np.dtype([("dm_index", "<u4"), ("h", "<u4"), ("k", "<u4"), ("power", "<f4"), ("sigma", "<f8"), ("freq_hz", "<f8")])
GROUP = np.dtype([("best", CAND), ("nmember", "<u4"), ("dm_index_lo", "<u4"), ("dm_index_hi", "<u4"), ("reserved", "<u4")])
# exp, log and erfc of two C libraries agree to a few units in the last place (1e-15); the 64 bisection steps of step 8 end an
# interval of (sqrt(-2 lq) + 2) 2^-64 wide, far below that; 1e-9 leaves six decimal orders for the conditioning of the inverse
SIGMA_RTOL = 1e-9


class Capacity(Exception):
    pass


def nfft_of(nout, nfft=0):
    n = nfft
    if not n:
        n = 1
        while n * 2 <= nout and n < 1 << 22:
            n *= 2
    assert n & (n - 1) == 0 and 1 << 12 <= n <= 1 << 22 and n <= nout
    return n


# ---- step 1 ----------------------------------------------------------------------------------------------------------
def means(x, n):
    """x [ndm][>= n] float32 -> mean [ndm] double: 64 partial sums, partial j over positions j, j + 64, ... ascending"""
    v = x[:, :n].astype(np.float64).reshape(x.shape[0], n // NPART, NPART)
    part = np.zeros((x.shape[0], NPART))
    with np.errstate(all="ignore"):
        for r in range(n // NPART):
            part = part + v[:, r, :]
        s = np.zeros(x.shape[0])
        for j in range(NPART):
            s = s + part[:, j]
        return s / np.float64(n)


# ---- step 2 ----------------------------------------------------------------------------------------------------------
def twiddles(n):
    k = np.arange(n // 2, dtype=np.float64)
    a = 2.0 * np.pi * k / np.float64(n)
    return np.cos(a).astype(F32), (-np.sin(a)).astype(F32)


def bitrev(n):
    bits = n.bit_length() - 1
    i = np.arange(n)
    r = np.zeros(n, dtype=np.int64)
    for q in range(bits):
        r |= ((i >> q) & 1) << (bits - 1 - q)
    return r


def fft(zr, zi):
    """Z = DFT_n(z) of float32 arrays [..., n]: decimation in time on the bit-reversed input, stages s = 1 .. log2 n,
    t = (wr vr - wi vi, wr vi + wi vr), u' = u + t, v' = u - t"""
    n = zr.shape[-1]
    wr, wi = twiddles(n)
    rev = bitrev(n)
    xr, xi = np.array(zr[..., rev]), np.array(zi[..., rev])
    L = n.bit_length() - 1
    i = np.arange(n // 2)
    with np.errstate(all="ignore"):
        for s in range(1, L + 1):
            half = 1 << (s - 1)
            j = i & (half - 1)
            u = ((i >> (s - 1)) << s) + j
            v = u + half
            cr, ci = wr[j << (L - s)], wi[j << (L - s)]
            ur, ui, vr, vi = xr[..., u], xi[..., u], xr[..., v], xi[..., v]
            a = cr * vr
            b = ci * vi
            c = cr * vi
            d = ci * vr
            tr = a - b
            ti = c + d
            xr[..., u], xi[..., u] = ur + tr, ui + ti
            xr[..., v], xi[..., v] = ur - tr, ui - ti
    assert xr.dtype == F32 and xi.dtype == F32
    return xr, xi


# ---- step 3 ----------------------------------------------------------------------------------------------------------
def powers(series, n):
    """-> (N float32 [ndm][n / 2] with N[:, 0] = 0, live bool [ndm])"""
    x = np.asarray(series, dtype=F32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    ndm = x.shape[0]
    mean = means(x, n)
    live = np.isfinite(mean)
    npair = (ndm + 1) // 2
    z = np.zeros((2 * npair, n), dtype=F32)
    with np.errstate(all="ignore"):
        d = (x[:, :n].astype(np.float64) - mean[:, None]).astype(F32)
    d[~live] = 0.0
    z[:ndm] = d
    Zr, Zi = fft(np.ascontiguousarray(z[0::2]), np.ascontiguousarray(z[1::2]))
    k = np.arange(1, n // 2)
    Ar, Ai, Br, Bi = Zr[:, k], Zi[:, k], Zr[:, n - k], Zi[:, n - k]
    N = np.zeros((2 * npair, n // 2), dtype=F32)
    with np.errstate(all="ignore"):
        s0, d0, s1, d1 = Ar + Br, Ai - Bi, Ai + Bi, Br - Ar
        N[0::2, 1:] = s0 * s0 + d0 * d0
        N[1::2, 1:] = s1 * s1 + d1 * d1
    N = N[:ndm]
    N[~live] = 0.0
    return N, live


# ---- step 4 ----------------------------------------------------------------------------------------------------------
def block_edges(nb, B):
    """blocks of the nb bins 1 .. nb -> [(k0, k1)]: whole blocks of B, the rest on its own when it has B / 2 bins or more"""
    nblk, rest = nb // B, nb % B
    edges = [[1 + b * B, 1 + (b + 1) * B] for b in range(nblk)]
    if rest:
        if rest >= B // 2 or not edges:
            edges.append([1 + nblk * B, 1 + nb])
        else:
            edges[-1][1] = 1 + nb
    return [tuple(e) for e in edges]


def kmin_of(n, tsamp, flo=0.0):
    kf = math.ceil((flo or 0.5) * float(n) * tsamp)
    return int(min(max(kf, 1), n // 2))


def normalise(N, n, wblock, kmin):
    """-> p float32 [ndm][n / 2].  S of a block is the sum in ascending k: np.cumsum adds along the axis one element after the
    other (it is not a pairwise sum), so its last element is that sum"""
    B = wblock or 128
    p = np.zeros_like(N)
    for k0, k1 in block_edges(n // 2 - 1, B):
        v = N[:, k0:k1]
        with np.errstate(all="ignore"):
            S = np.cumsum(v.astype(np.float64), axis=1)[:, -1]
            mx = np.where(np.isnan(v), F32(0.0), v).max(axis=1)          # the walk from 0: a NaN never replaces
            m = (S - mx.astype(np.float64)) / np.float64(k1 - k0 - 1)
            ok = np.isfinite(m) & (m > 0.0)
            q = (v.astype(np.float64) / np.where(ok, m, 1.0)[:, None]).astype(F32)
        p[:, k0:k1] = np.where(ok[:, None], q, F32(0.0))
    p[:, :kmin] = 0.0
    return p


# ---- steps 5 - 7 -----------------------------------------------------------------------------------------------------
def harmonic_sum(p, h, kmin):
    """-> (k [cnt], H float32 [ndm][cnt]) over k = h kmin .. n/2 - 1; cnt may be 0"""
    nh = p.shape[1]
    k = np.arange(h * kmin, nh, dtype=np.int64)
    H = np.zeros((p.shape[0], k.size), dtype=F32)
    with np.errstate(all="ignore"):
        for j in range(1, h + 1):
            H = H + p[:, (j * k + h // 2) // h]
    assert H.dtype == F32
    return k, H


def q_of(h, x):
    term, s = 1.0, 1.0
    for i in range(1, h):
        term = term * x / float(i)
        s = s + term
    return math.exp(-x) * s


def tail_of(sigma):
    return 0.5 * math.erfc(sigma / math.sqrt(2.0))


def thresholds(sigma):
    """T_1, T_2, T_4, T_8, T_16 as float32: bisection in double on [0, 1000], the upper end rounded up"""
    tail = tail_of(sigma)
    out = []
    for h in FOLDS:
        lo, hi = 0.0, 1000.0
        while True:
            mid = 0.5 * (lo + hi)
            if not (lo < mid < hi):
                break
            if q_of(h, mid) > tail:
                lo = mid
            else:
                hi = mid
        t = F32(hi)
        if float(t) < hi:
            t = np.nextafter(t, F32(np.inf))
        out.append(t)
    return np.array(out, dtype=F32)


def raw_peaks(p, kmin, nharm, thr):
    """-> list of (dm, h, k, H float32)"""
    out = []
    for f, h in enumerate(FOLDS):
        if h > (nharm or 16):
            break
        k, H = harmonic_sum(p, h, kmin)
        if not k.size:
            continue
        with np.errstate(all="ignore"):
            ok = H >= thr[f]
            ok[:, 1:] &= H[:, 1:] > H[:, :-1]
            ok[:, :-1] &= H[:, :-1] >= H[:, 1:]
        for d, i in zip(*np.nonzero(ok)):
            out.append((int(d), h, int(k[i]), H[d, i]))
    if len(out) > RAW_CAP:
        raise Capacity(len(out))
    return out


# ---- step 8 ----------------------------------------------------------------------------------------------------------
def log_q(h, x):
    if x < 1.0:
        s = 1.0
        for i in range(h - 1, 0, -1):
            s = s * x / float(i) + 1.0
        return -x + math.log(s)
    r, lf = 1.0, 0.0
    for i in range(1, h):
        r = r * float(i) / x + 1.0
    for i in range(2, h):
        lf = lf + math.log(float(i))
    return -x + (float(h - 1) * math.log(x) - lf + math.log(r))


def log_tail(s):
    if s < 30.0:
        return math.log(0.5 * math.erfc(s / math.sqrt(2.0)))
    s2 = s * s
    return -0.5 * s2 - math.log(s) - 0.5 * math.log(2.0 * math.pi) + math.log1p(-1.0 / s2 + 3.0 / (s2 * s2))


def sigma_of(h, H):
    x = float(H)
    fmax = float(np.finfo(F32).max)
    if not x <= fmax:
        x = fmax
    lq = log_q(h, x)
    if not lq < 0.0:
        return 0.0
    lo, hi = 0.0, math.sqrt(-2.0 * lq) + 2.0
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        if log_tail(mid) > lq:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def sift(raw, n, tsamp):
    """raw: list of (dm, h, k, H) of all series -> CAND records, survivors sorted by (dm_index, h, k)"""
    recs = [(d, h, k, H, sigma_of(h, H), float(k) / (float(h) * (float(n) * tsamp))) for d, h, k, H in raw]
    keep = []
    by_dm = {}
    for r in recs:
        by_dm.setdefault(r[0], []).append(r)
    for d, rs in by_dm.items():
        for a in rs:
            dropped = False
            for b in rs:
                if b is a or abs(a[2] * b[1] - b[2] * a[1]) > a[1] * b[1]:
                    continue
                if b[4] > a[4] or (b[4] == a[4] and (b[1] < a[1] or (b[1] == a[1] and b[2] < a[2]))):
                    dropped = True
                    break
            if not dropped:
                keep.append(a)
    keep.sort(key=lambda r: (r[0], r[1], r[2]))
    return np.array(keep, dtype=CAND) if keep else np.zeros(0, dtype=CAND)


def search(series, tsamp, sigma=6.0, nharm=0, flo=0.0, nfft=0, wblock=0, want_raw=False):
    """-> CAND records [, the raw peaks]; raises Capacity beyond 2^20 raw peaks"""
    x = np.asarray(series, dtype=F32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    n = nfft_of(x.shape[1], nfft)
    N, _live = powers(x, n)
    kmin = kmin_of(n, tsamp, flo)
    p = normalise(N, n, wblock, kmin)
    raw = raw_peaks(p, kmin, nharm, thresholds(sigma))
    out = sift(raw, n, tsamp)
    return (out, raw) if want_raw else out


# ---- step 9 ----------------------------------------------------------------------------------------------------------
def group(cands, dm_gap=2):
    """-> GROUP records sorted by best.sigma descending, then f, dm_index, h"""
    c = [tuple(r) for r in np.asarray(cands, dtype=CAND).tolist()]
    parent = list(range(len(c)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, a in enumerate(c):
        for j in range(i + 1, len(c)):
            b = c[j]
            if abs(a[0] - b[0]) <= dm_gap and 2 * abs(a[2] * b[1] - b[2] * a[1]) <= 3 * a[1] * b[1]:
                ra, rb = find(i), find(j)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    groups = {}
    for i, a in enumerate(c):
        groups.setdefault(find(i), []).append(a)
    out = []
    for members in groups.values():
        best = sorted(members, key=lambda r: (-r[4], r[1], r[0], r[2]))[0]
        out.append((best, len(members), min(m[0] for m in members), max(m[0] for m in members), 0))
    import functools

    def order(x, y):
        a, b = x[0], y[0]
        if a[4] != b[4]:
            return -1 if a[4] > b[4] else 1
        fa, fb = a[2] * b[1], b[2] * a[1]
        if fa != fb:
            return -1 if fa < fb else 1
        return (a[0] > b[0]) - (a[0] < b[0]) or (a[1] > b[1]) - (a[1] < b[1])
    out.sort(key=functools.cmp_to_key(order))
    return np.array(out, dtype=GROUP) if out else np.zeros(0, dtype=GROUP)
