"""Numpy restatement of the burst polarisation stage (include/frbch.h, "burst polarisation"): the sums of a burst's three
windows, the spectra, noise and `used` derived from them, the table, the records and the integer transform of RM synthesis
(Python ints / int64), and the peaks.  Beside it `transform_fp64`: the same transform in plain double precision with no
table and no quantisation, which the known-answer tests measure the integer form against.  Delays are
oracle.post_oracle.delays_samples.  Test infrastructure only."""
import math

import numpy as np

from frb_baseband_amd import post
from oracle import post_oracle as po

C_MHZ_M = 299.792458
TWO64 = 18446744073709551616.0
MASK64 = (1 << 64) - 1


def delays(hdr, dm):
    return np.asarray(po.delays_samples(hdr["fch1"], hdr["foff"], hdr["nchans"], hdr["tsamp"], dm), dtype=np.int64)


def cumsum_rows(x, out):
    """out[r + 1] = out[r] + x[r] with out[0] as it stands: np.cumsum(x, axis=0, out=out[1:]) on integers, a row at a time (numpy
    walks axis 0 of a C-ordered array column by column, several times slower at 8192 channels)"""
    for r in range(x.shape[0]):
        np.add(out[r], x[r], out=out[r + 1])
    return out


def windows(cand):
    """-> [(first row at the top of the band, rows, which)] in ascending order; which: 0 = on, 1 = off"""
    on_lo = int(cand["sample"]) - int(cand["width"]) // 2
    w, g, n = int(cand["width"]), int(cand["off_gap"]), int(cand["off_len"])
    return [(on_lo - g - n, n, 1), (on_lo, w, 0), (on_lo + w + g, n, 1)]


# ---- step 1 ----------------------------------------------------------------------------------------------------------
def burst_sums(x, hdr, cands):
    """x [nrows][nifs][nchan] -> BURST_SUMS [ncand][nifs][nchan]: integer rows in int64 (exact), float rows in double, one row
    at a time in ascending row order"""
    nrows, nifs, nchan = x.shape
    integer = x.dtype != np.float32
    out = np.zeros((len(cands), nifs, nchan), dtype=post.BURST_SUMS)
    chans = np.arange(nchan)
    for i, cd in enumerate(cands):
        d = delays(hdr, float(cd["dm"]))
        s = np.zeros((2, nifs, nchan), dtype=np.int64 if integer else np.float64)
        q = np.zeros((nifs, nchan), dtype=np.int64 if integer else np.float64)
        hits = np.zeros((2, nchan), dtype=np.int64)
        for w0, length, which in windows(cd):
            for t in range(w0, w0 + length):
                r = t + d
                ok = (r >= 0) & (r < nrows)
                if not ok.any():
                    continue
                v = x[r[ok], :, chans[ok]].T.astype(np.int64 if integer else np.float64)     # [nifs][present channels]
                s[which][:, ok] = s[which][:, ok] + v
                if which:
                    q[:, ok] = q[:, ok] + v * v
                hits[which][ok] += 1
        out[i]["on_sum"], out[i]["off_sum"], out[i]["off_sumsq"] = s[0], s[1], q
        out[i]["on_hits"], out[i]["off_hits"] = hits[0][None, :], hits[1][None, :]
    return out


def derive(sums, gain=None, coherency=False):
    """-> spec, noise [ncand][nifs][nchan] float32, used [ncand][nchan] uint8: double, every operation on its own"""
    ncand, nifs, nchan = sums.shape
    g = np.ones((nifs, nchan)) if gain is None else np.asarray(gain, dtype=np.float32).astype(np.float64)
    non, noff = sums["on_hits"].astype(np.float64), sums["off_hits"].astype(np.float64)
    bad = (sums["on_hits"] == 0) | (sums["off_hits"] < 2)
    with np.errstate(all="ignore"):
        d = sums["on_sum"] / non - sums["off_sum"] / noff
        spec = (d * g[None]).astype(np.float32)
        var = (sums["off_sumsq"] - (sums["off_sum"] * sums["off_sum"]) / noff) / (noff - 1.0)
        var = np.where(var < 0.0, 0.0, var)
        noise = (np.sqrt(var / non) * np.abs(g)[None]).astype(np.float32)
    bad |= ~np.isfinite(spec) | ~np.isfinite(noise)
    ok = ~bad.any(axis=1)
    if coherency:
        with np.errstate(all="ignore"):
            pp, qq, re, im = (spec[:, k].copy() for k in range(4))
            npp, nqq, nre, nim = (noise[:, k].copy() for k in range(4))
            spec = np.stack([pp + qq, np.float32(2) * re, np.float32(2) * im, pp - qq], axis=1)
            a, b = npp.astype(np.float64) * npp.astype(np.float64), nqq.astype(np.float64) * nqq.astype(np.float64)
            nq = np.sqrt(a + b).astype(np.float32)
            noise = np.stack([nq, np.float32(2) * nre, np.float32(2) * nim, nq], axis=1)
        ok &= np.isfinite(spec).all(axis=1) & np.isfinite(noise).all(axis=1)
    spec = np.where(ok[:, None, :], spec, np.float32(0)).astype(np.float32)
    noise = np.where(ok[:, None, :], noise, np.float32(0)).astype(np.float32)
    return spec, noise, ok.astype(np.uint8)


def burst_spectra(x, hdr, cands, gain=None, coherency=False):
    return derive(burst_sums(x, hdr, cands), gain, coherency)


# ---- step 2 ----------------------------------------------------------------------------------------------------------
def table():
    j = np.arange(4096, dtype=np.float64)
    c = np.zeros(16384, dtype=np.int64)
    c[:4096] = np.rint(np.cos((2.0 * math.pi * j) / 16384.0) * 4194304.0).astype(np.int64)
    c[4096] = 0
    k = np.arange(4097, 8193)
    c[k] = -c[8192 - k]
    k = np.arange(8193, 16384)
    c[k] = c[16384 - k]
    return c.astype(np.int32)


def lambda2(hdr):
    f = hdr["fch1"] + np.arange(hdr["nchans"], dtype=np.float64) * hdr["foff"]
    t = C_MHZ_M / f
    return t * t


def fix(x):
    """frac(x) 2^64 as a Python int; 2^64 counts as 0"""
    fr = x - math.floor(x)
    v = fr * TWO64
    return 0 if not v < TWO64 else int(v)


def records(q, u, used, hdr, phi_lo, dphi):
    """one candidate -> (Qi, Ui int64 arrays, P0, D lists of Python ints, N, exponent e) over the used channels; None: F = 0"""
    l2 = lambda2(hdr)
    sel = np.flatnonzero(np.asarray(used) != 0)
    N = sel.size
    if N == 0:
        return None
    total = 0.0
    for c in sel:
        total = total + float(l2[c])
    l0 = total / float(N)
    qs, us = np.asarray(q, dtype=np.float32)[sel], np.asarray(u, dtype=np.float32)[sel]
    m = float(max(np.abs(qs).max(), np.abs(us).max()))
    if m == 0.0:
        return None
    _f, e = math.frexp(m)
    scale = 2.0 ** (23 - e)
    qi = np.rint(qs.astype(np.float64) * scale).astype(np.int64)
    ui = np.rint(us.astype(np.float64) * scale).astype(np.int64)
    a = [(float(l2[c]) - l0) / math.pi for c in sel]
    return qi, ui, [fix(phi_lo * x) for x in a], [fix(dphi * x) for x in a], N, e


def transform(q, u, used, hdr, nphi, phi_lo, dphi):
    """-> (F [ncand][nphi][2] float32, Re, Im as int64 [ncand][nphi]): the integer transform; uint64 arithmetic wraps as the
    rule's mod 2^64 does"""
    q, u, used = (np.asarray(a).reshape(-1, hdr["nchans"]) for a in (q, u, used))
    tab = table().astype(np.int64)
    k = np.arange(nphi, dtype=np.uint64)
    F = np.zeros((q.shape[0], nphi, 2), dtype=np.float32)
    RE, IM = np.zeros((q.shape[0], nphi), dtype=np.int64), np.zeros((q.shape[0], nphi), dtype=np.int64)
    for i in range(q.shape[0]):
        rec = records(q[i], u[i], used[i], hdr, phi_lo, dphi)
        if rec is None:
            continue
        qi, ui, p0, d, N, e = rec
        re, im = np.zeros(nphi, dtype=np.int64), np.zeros(nphi, dtype=np.int64)
        with np.errstate(over="ignore"):
            for c in range(N):
                ph = np.uint64(p0[c]) + k * np.uint64(d[c])
                j = (((ph + np.uint64(1 << 49)) >> np.uint64(50)) & np.uint64(16383)).astype(np.int64)
                cj, sj = tab[j], tab[(j - 4096) & 16383]
                re += qi[c] * cj + ui[c] * sj
                im += ui[c] * cj - qi[c] * sj
        inv = 1.0 / (float(N) * 2.0 ** (45 - e))
        F[i, :, 0] = (re.astype(np.float64) * inv).astype(np.float32)
        F[i, :, 1] = (im.astype(np.float64) * inv).astype(np.float32)
        RE[i], IM[i] = re, im
    return F, RE, IM


def transform_fp64(q, u, used, hdr, nphi, phi_lo, dphi):
    """the same sum in plain double precision: no table, no quantisation -> complex128 [ncand][nphi]"""
    q, u, used = (np.asarray(a).reshape(-1, hdr["nchans"]) for a in (q, u, used))
    l2 = lambda2(hdr)
    phi = phi_lo + np.arange(nphi, dtype=np.float64) * dphi
    F = np.zeros((q.shape[0], nphi), dtype=np.complex128)
    for i in range(q.shape[0]):
        sel = np.flatnonzero(used[i] != 0)
        if sel.size == 0:
            continue
        l0 = l2[sel].mean()
        p = (q[i, sel].astype(np.float64) + 1j * u[i, sel].astype(np.float64))
        for c, pc in zip(sel, p):
            F[i] += pc * np.exp(-2j * phi * (l2[c] - l0))
        F[i] /= sel.size
    return F


# ---- step 3 ----------------------------------------------------------------------------------------------------------
def parabola(P, kp, phi_lo, dphi):
    """-> (rm, peak, fitted) of the rule, on double powers P"""
    y0 = float(P[kp])
    if 0 < kp < len(P) - 1:
        ym, yp = float(P[kp - 1]), float(P[kp + 1])
        den = (ym - 2.0 * y0) + yp
        if den < 0.0:
            diff = ym - yp
            delta = (0.5 * diff) / den
            return phi_lo + (float(kp) + delta) * dphi, math.sqrt(y0 - (0.25 * diff) * delta), 1
    return phi_lo + float(kp) * dphi, math.sqrt(y0), 0


def peaks(F, used, noise_q, noise_u, hdr, nphi, phi_lo, dphi):
    F = np.asarray(F, dtype=np.float32).reshape(-1, nphi, 2)
    used = np.asarray(used).reshape(-1, hdr["nchans"])
    l2 = lambda2(hdr)
    out = np.zeros(F.shape[0], dtype=post.RM_RESULT)
    for i in range(F.shape[0]):
        re, im = F[i, :, 0].astype(np.float64), F[i, :, 1].astype(np.float64)
        P = re * re + im * im
        kp = int(np.argmax(P))                                  # the first largest
        r = out[i]
        r["kpeak"] = kp
        r["rm"], r["peak"], r["fitted"] = parabola(P, kp, phi_lo, dphi)
        r["pa0"] = math.atan2(float(im[kp]), float(re[kp])) / 2.0
        sel = np.flatnonzero(used[i] != 0)
        r["nused"] = sel.size
        acc = 0.0
        if noise_q is not None and noise_u is not None:
            nq = np.asarray(noise_q, dtype=np.float32).reshape(-1, hdr["nchans"])[i].astype(np.float64)
            nu = np.asarray(noise_u, dtype=np.float32).reshape(-1, hdr["nchans"])[i].astype(np.float64)
            for c in sel:
                acc = acc + (nq[c] * nq[c] + nu[c] * nu[c])
        if sel.size:
            r["sigma_f"] = math.sqrt(acc / 2.0) / float(sel.size)
            lo, hi = float(l2[sel].min()), float(l2[sel].max())
            if hi > lo:
                r["fwhm"] = (2.0 * math.sqrt(3.0)) / (hi - lo)
        if r["sigma_f"] > 0.0:
            r["snr"] = math.sqrt(float(P[kp])) / float(r["sigma_f"])
        if r["snr"] > 0.0:
            r["rm_err"] = float(r["fwhm"]) / (2.0 * float(r["snr"]))
    return out


def burst_rm(x, hdr, cands, nphi, phi_lo, dphi, gain=None, flag=None, coherency=False):
    """the composite -> dict(spec, noise, used, F, results)"""
    spec, noise, used = burst_spectra(x, hdr, cands, gain, coherency)
    if flag is not None:
        used = np.where(np.asarray(flag)[None, :] != 0, 0, used).astype(np.uint8)
    F, _re, _im = transform(spec[:, 1], spec[:, 2], used, hdr, nphi, phi_lo, dphi)
    res = peaks(F, used, noise[:, 1], noise[:, 2], hdr, nphi, phi_lo, dphi)
    return dict(spec=spec, noise=noise, used=used, F=F, results=res)
