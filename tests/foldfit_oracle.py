"""Numpy restatement of the fold refinement (frbch_foldfit_*; include/frbch.h states the arithmetic): the shift tables in
float64 with every operation on its own, the two stages in int64 / uint64, the score with its 64 partial sums, the peaks with the
parabola of the DM scan (tests/dmscan_oracle.py restates that one) and the S/N of a profile.  Nothing here calls the library."""
import numpy as np

DM_K = 2.41e-4
FIELDS = ("score", "prof_acc", "prof_hits", "results")
RESULT = np.dtype([("dm", "<f8"), ("dm_res", "<f8"), ("dfreq", "<f8"), ("dfreq_res", "<f8"), ("dfdot", "<f8"), ("dfdot_res", "<f8"),
                   ("score_peak", "<f8"), ("score_nominal", "<f8"), ("border_median", "<f8"), ("snr_nominal", "<f8"), ("snr_best", "<f8"),
                   ("kpeak", "<u4"), ("jpeak", "<u4"), ("ipeak", "<u4"), ("fitted_dm", "<u4"), ("fitted_freq", "<u4"), ("fitted_fdot", "<u4"),
                   ("nfit_dm", "<u4"), ("nfit_freq", "<u4"), ("nfit_fdot", "<u4"), ("width_nominal", "<u4"), ("bin_nominal", "<u4"),
                   ("width_best", "<u4"), ("bin_best", "<u4"), ("reserved", "<u4")])
assert RESULT.itemsize == 144


def rows_per_sub(hdr, subint_s):
    return max(1, int(np.floor(subint_s / hdr["tsamp"] + 0.5)))                 # llround of a positive number


def axis(n, step):
    return (np.arange(n, dtype=np.int64) - n // 2).astype(np.float64) * np.float64(step)


def delay_s(hdr, dm):
    """delay of every channel against the highest channel frequency, seconds: the expression of frbch_dedisperse_*"""
    fc = np.float64(hdr["fch1"]) + np.arange(hdr["nchans"], dtype=np.float64) * np.float64(hdr["foff"])
    fhi = fc[0] if hdr["foff"] < 0 else fc[-1]
    return np.float64(dm) / np.float64(DM_K) * (1.0 / (fc * fc) - 1.0 / (fhi * fhi))


def reduce_bins(y, nbin):
    assert np.all(np.abs(y) <= 2.0 ** 52)
    return (np.rint(y).astype(np.int64) % nbin).astype(np.int32)                 # (numpy's % takes the sign of the divisor)


def tables(hdr, nrows, nbin, nsub, f0_fold, subint_s, dm0, ndm, ddm, nfreq, dfreq, nfdot, dfdot):
    """-> (dms [ndm], shD [ndm][nchan], (-shP) mod nbin [nfdot][nfreq][nsub], tau [nsub])"""
    L = rows_per_sub(hdr, subint_s)
    assert nsub == (nrows + L - 1) // L
    dms = np.float64(dm0) + axis(ndm, ddm)
    shd = np.stack([reduce_bins((delay_s(hdr, dm) * np.float64(f0_fold)) * np.float64(nbin), nbin) for dm in dms])
    first = np.arange(nsub, dtype=np.int64) * L
    r = np.minimum(L, nrows - first)
    tau = ((first.astype(np.float64) + 0.5 * r.astype(np.float64)) - 0.5 * np.float64(nrows)) * np.float64(hdr["tsamp"])
    df, hd = axis(nfreq, dfreq), 0.5 * axis(nfdot, dfdot)
    lin = df[None, :, None] * tau[None, None, :]
    quad = (hd[:, None, None] * tau[None, None, :]) * tau[None, None, :]
    shp = reduce_bins(-((lin + quad) * np.float64(nbin)), nbin)                  # bin b reads (b - shP): kept negated, as (-shP) mod nbin
    return dms, shd, shp, tau


def stage1(cube, hits, use, products, shd):
    """cube [nsub][nifs][nbin][nchan] float64, hits [nsub][nbin][nchan] -> A int64, HA uint64, both [ndm][nsub][nbin]"""
    nsub, nifs, nbin, nchan = cube.shape
    icube = cube.astype(np.int64)
    assert np.array_equal(icube.astype(np.float64), cube)
    val = sum(icube[:, q] for q in range(nifs) if (products >> q) & 1)           # [nsub][nbin][nchan]
    A = np.zeros((shd.shape[0], nsub, nbin), np.int64)
    HA = np.zeros((shd.shape[0], nsub, nbin), np.uint64)
    for k in range(shd.shape[0]):
        for c in np.flatnonzero(use):
            A[k] += np.roll(val[:, :, c], -int(shd[k, c]), axis=1)
            HA[k] += np.roll(hits[:, :, c], -int(shd[k, c]), axis=1).astype(np.uint64)
    return A, HA


def stage2(A, HA, shp_trial):
    """one DM's planes [nsub][nbin] and one trial's shifts [nsub] -> (B int64 [nbin], H uint64 [nbin])"""
    B = np.zeros(A.shape[1], np.int64)
    H = np.zeros(A.shape[1], np.uint64)
    for s in range(A.shape[0]):
        B += np.roll(A[s], -int(shp_trial[s]))
        H += np.roll(HA[s], -int(shp_trial[s]))
    return B, H


def score_of(B, H, M, any_hits):
    """the 64 partial sums of the header; M and any_hits are the DM's"""
    term = np.zeros(B.size, np.float64)
    on = H > 0
    x = B[on].astype(np.float64) / H[on].astype(np.float64)
    d = x - M
    term[on] = H[on].astype(np.float64) * (d * d)
    total = np.float64(0.0)
    for q in range(64):
        part = np.float64(0.0)
        for v in term[q::64]:
            part = part + v
        total = total + part
    return total if any_hits and int(on.sum()) >= 2 else np.float64(0.0)


def scores(A, HA, shp):
    """-> score [ndm][nfdot][nfreq]"""
    ndm = A.shape[0]
    out = np.zeros((ndm,) + shp.shape[:2], np.float64)
    for k in range(ndm):
        ta, th = int(A[k].sum(dtype=np.int64)), int(HA[k].sum(dtype=np.uint64))
        M = np.float64(ta) / np.float64(th) if th else np.float64(0.0)
        for j in range(shp.shape[0]):
            for i in range(shp.shape[1]):
                B, H = stage2(A[k], HA[k], shp[j, i])
                out[k, j, i] = score_of(B, H, M, th != 0)
    return out


def parabola(v, fit_frac, x, step):
    """the fit of frbch_dmscan_peaks along one cut -> (peak index, nfit, fitted, value, half-width at 1 below the vertex)"""
    kp = int(np.argmax(v))
    if not v[kp] > 0.0:
        return kp, 0, 0, x[kp], 0.0
    thr = np.float64(fit_frac) * v[kp]
    lo = hi = kp
    while lo > 0 and v[lo - 1] >= thr:
        lo -= 1
    while hi + 1 < len(v) and v[hi + 1] >= thr:
        hi += 1
    nfit = hi - lo + 1
    if nfit < 3 or lo == 0 or hi == len(v) - 1:
        return kp, nfit, 0, x[kp], 0.0
    s = [0, 0, 0, 0, 0]
    T0 = T1 = T2 = np.float64(0.0)
    for k in range(lo, hi + 1):
        d = k - kp
        for n in range(5):
            s[n] += d ** n
        T0 = T0 + v[k]
        T1 = T1 + np.float64(d) * v[k]
        T2 = T2 + np.float64(d * d) * v[k]
    S0, S1, S2, S3, S4 = (np.float64(t) for t in s)
    m0, m1, m2 = S2 * S0 - S1 * S1, S3 * S0 - S1 * S2, S3 * S1 - S2 * S2
    D = (S4 * m0 - S3 * m1) + S2 * m2
    p1, p2, p3 = T1 * S0 - S1 * T0, T1 * S1 - S2 * T0, S3 * T0 - S2 * T1
    Da = (T2 * m0 - S3 * p1) + S2 * p2
    Db = (S4 * p1 - T2 * m1) + S2 * p3
    a, b = Da / D, Db / D
    if not a < 0.0:
        return kp, nfit, 0, x[kp], 0.0
    vertex = (-b) / (2.0 * a)
    return kp, nfit, 1, x[kp] + vertex * np.float64(step), np.sqrt(-1.0 / a) * np.float64(step)


def snr_of(B, H, widths):
    nb = B.size
    nw = nb // 2
    x = np.zeros(nb, np.float64)
    on = H > 0
    x[on] = B[on].astype(np.float64) / H[on].astype(np.float64)
    xx = np.concatenate([x, x])

    def window(j, w):
        s = np.float64(0.0)
        for v in xx[j: j + w]:
            s = s + v
        return s
    sums = [window(j, nw) for j in range(nb)]
    off = int(np.argmin(sums))
    base = sums[off] / np.float64(nw)
    ss = np.float64(0.0)
    for v in xx[off: off + nw]:
        d = v - base
        ss = ss + d * d
    rms = np.sqrt(ss / np.float64(nw))
    best, bw, bj = np.float64(0.0), int(widths[0]), 0
    if not rms > 0.0:
        return best, bw, bj
    first = True
    for w in widths:
        rw = np.sqrt(np.float64(w))
        for j in range(nb):
            v = ((window(j, int(w)) / np.float64(w) - base) * rw) / rms
            if first or v > best:
                best, bw, bj, first = v, int(w), j, False
    return best, bw, bj


def peaks(score, dm0, ddm, dfreq, dfdot, fit_frac, widths, prof_acc, prof_hits):
    """-> a RESULT record from the score grid [ndm][nfdot][nfreq] and the two profiles"""
    r = np.zeros(1, RESULT)[0]
    n = score.shape
    flat = score.reshape(-1)
    at = int(np.argmax(flat))
    kp, jp, ip = np.unravel_index(at, n)
    r["kpeak"], r["jpeak"], r["ipeak"] = kp, jp, ip
    r["score_peak"], r["score_nominal"] = flat[at], score[n[0] // 2, n[1] // 2, n[2] // 2]
    idx = np.indices(n)
    edge = np.zeros(n, bool)
    for a in range(3):
        if n[a] > 1:
            edge |= (idx[a] == 0) | (idx[a] == n[a] - 1)
    border = np.sort(score[edge])
    if border.size:
        m = border.size
        r["border_median"] = border[m // 2] if m % 2 else 0.5 * (border[m // 2 - 1] + border[m // 2])
    wide = np.sqrt(r["border_median"]) if r["border_median"] > 0.0 else np.float64(0.0)
    cuts = (("dm", score[:, jp, ip], np.float64(dm0) + axis(n[0], ddm), ddm), ("fdot", score[kp, :, ip], axis(n[1], dfdot), dfdot),
            ("freq", score[kp, jp, :], axis(n[2], dfreq), dfreq))
    for name, v, x, step in cuts:
        _k, nfit, fitted, value, unit = parabola(v, fit_frac, x, step)
        r["d" + name if name != "dm" else "dm"] = value
        r[("d" + name if name != "dm" else "dm") + "_res"] = unit * wide if fitted else 0.0
        r["nfit_" + name], r["fitted_" + name] = nfit, fitted
    r["snr_nominal"], r["width_nominal"], r["bin_nominal"] = snr_of(prof_acc[0], prof_hits[0], widths)
    r["snr_best"], r["width_best"], r["bin_best"] = snr_of(prof_acc[1], prof_hits[1], widths)
    return r


def steps(hdr, nrows, nbin, f0_fold):
    """-> (ddm, dfreq, dfdot), the natural steps"""
    T = np.float64(nrows) * np.float64(hdr["tsamp"])
    fc = np.float64(hdr["fch1"]) + np.arange(hdr["nchans"], dtype=np.float64) * np.float64(hdr["foff"])
    flo, fhi = (fc[-1], fc[0]) if hdr["foff"] < 0 else (fc[0], fc[-1])
    d = np.float64(1.0) / np.float64(DM_K) * (1.0 / (flo * flo) - 1.0 / (fhi * fhi))
    return 1.0 / ((np.float64(nbin) * np.float64(f0_fold)) * d), 1.0 / (np.float64(nbin) * T), 8.0 / ((np.float64(nbin) * T) * T)


def fold_fit(cube, hits, hdr, nrows, *, f0_fold, subint_s, products, dm0, ndm, ddm, nfreq, dfreq, nfdot, dfdot, fit_frac, widths, flag=None,
             want_trials=False):
    """everything frbch_foldfit_* give for one cube -> dict of score, prof_acc, prof_hits, results, plane_acc, plane_hits (and
    trial_acc, trial_hits)"""
    nsub, _nifs, nbin, nchan = cube.shape
    use = np.ones(nchan, bool) if flag is None else ~np.asarray(flag, bool)
    _dms, shd, shp, _tau = tables(hdr, nrows, nbin, nsub, f0_fold, subint_s, dm0, ndm, ddm, nfreq, dfreq, nfdot, dfdot)
    A, HA = stage1(cube, hits, use, products, shd)
    assert int(np.abs(A).max(initial=0)) < 2 ** 53
    score = scores(A, HA, shp)
    best = int(np.argmax(score.reshape(-1)))
    kb, jb, ib = np.unravel_index(best, score.shape)
    two = [stage2(A[ndm // 2], HA[ndm // 2], shp[nfdot // 2, nfreq // 2]), stage2(A[kb], HA[kb], shp[jb, ib])]
    prof_acc, prof_hits = np.stack([t[0] for t in two]), np.stack([t[1] for t in two])
    out = dict(score=score, prof_acc=prof_acc, prof_hits=prof_hits, plane_acc=A[ndm // 2].copy(), plane_hits=HA[ndm // 2].copy(),
               results=np.array([peaks(score, dm0, ddm, dfreq, dfdot, fit_frac, widths, prof_acc, prof_hits)], RESULT))
    if want_trials:
        t = [[[stage2(A[k], HA[k], shp[j, i]) for i in range(nfreq)] for j in range(nfdot)] for k in range(ndm)]
        out["trial_acc"] = np.array([[[c[0] for c in b] for b in a] for a in t], np.int64)
        out["trial_hits"] = np.array([[[c[1] for c in b] for b in a] for a in t], np.uint64)
    return out
