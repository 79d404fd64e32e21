"""Numpy restatement of the polarisation profile of a burst (include/frbch.h, "polarisation profile of a burst"): the host
preparation (used channels, baselines, gains, the scale 2^k, the rotation of every channel from the table), the integer sums
per (candidate, bin) in int64 -- and, on request, once more in Python integers of unbounded size --, and the derivation of the
bins and the per-candidate results.  Beside it `profile_fp64`: the same definition in plain double precision, phases by cos /
sin, nothing quantised, which the accuracy tests hold the integer form against.  The burst sums, `used`, lambda^2, the table and
frac() are tests/rm_oracle.py's.  Test infrastructure only."""
import math

import numpy as np

from frb_baseband_amd import post
from tests import rm_oracle as ro

CHUNK = 1024                  # channels per cumulative sum


def bin_sums(x, d, t0, nbin, tfactor):
    """x [nrows][4][nchan] integers, d [nchan] delays -> (S int64 [4][nchan][nbin], h int64 [nchan][nbin]): the sums and the
    numbers of the present rows of every bin in every channel"""
    nrows, _nifs, nchan = x.shape
    edges = t0 + np.arange(nbin + 1, dtype=np.int64) * tfactor
    S = np.zeros((4, nchan, nbin), np.int64)
    h = np.zeros((nchan, nbin), np.int64)
    for c0 in range(0, nchan, CHUNK):
        c1 = min(nchan, c0 + CHUNK)
        e = np.clip(edges[None, :] + d[c0:c1, None], 0, nrows)                       # [channels][nbin + 1]
        lo = int(e.min())
        hi = max(lo, int(e.max()))
        cs = np.zeros((hi - lo + 1, 4, c1 - c0), np.int64)
        ro.cumsum_rows(x[lo:hi, :, c0:c1], cs)
        cc = np.arange(c1 - c0)[:, None]
        for p in range(4):
            S[p, c0:c1] = cs[e[:, 1:] - lo, p, cc] - cs[e[:, :-1] - lo, p, cc]
        h[c0:c1] = e[:, 1:] - e[:, :-1]
    return S, h


def prepare(x, hdr, cands, rm, nbin, tfactor, ref="mean", gain=None, flag=None, coherency=False):
    """the host preparation -> one dict per candidate (live False: every output 0) and `used` [ncand][nchan]"""
    nchan, nbits = hdr["nchans"], x.dtype.itemsize * 8
    sums = ro.burst_sums(x, hdr, cands)
    _spec, _noise, used = ro.derive(sums, gain, coherency)
    if flag is not None:
        used = np.where(np.asarray(flag)[None, :] != 0, 0, used).astype(np.uint8)
    g = np.ones((4, nchan)) if gain is None else np.asarray(gain, dtype=np.float32).astype(np.float64)
    l2 = ro.lambda2(hdr)
    tab = ro.table().astype(np.int64)
    rm = np.broadcast_to(np.asarray(rm, dtype=np.float64), (len(cands),))
    out = []
    for i, cd in enumerate(cands):
        on_lo = int(cd["sample"]) - int(cd["width"]) // 2
        t0 = int(cd["sample"]) - (nbin // 2) * tfactor
        sel = np.flatnonzero(used[i] != 0)
        N = sel.size
        c = dict(t0=t0, N=N, live=False, k=0, lref=0.0, d=ro.delays(hdr, float(cd["dm"])), sel=sel,
                 on_lo_bin=min(nbin - 1, max(0, (on_lo - t0) // tfactor)),
                 on_hi_bin=min(nbin - 1, max(0, (on_lo + int(cd["width"]) - 1 - t0) // tfactor)))
        out.append(c)
        gmax = float(np.abs(g[:, sel]).max()) if N else 0.0
        if N == 0 or gmax == 0.0:
            continue
        total = 0.0
        for ch in sel:
            total = total + float(l2[ch])
        lref = total / float(N) if ref in ("mean", 0) else 0.0
        M = (float(tfactor) * 2.0 ** nbits) * gmax
        _f, e = math.frexp(M)
        with np.errstate(all="ignore"):
            noff = sums["off_hits"][i].astype(np.float64)
            mean = sums["off_sum"][i] / noff
            var = (sums["off_sumsq"][i] - (sums["off_sum"][i] * sums["off_sum"][i]) / noff) / (noff - 1.0)
            var = np.where(var < 0.0, 0.0, var)
            w = (g * g) * var
        cc, sc = np.zeros(nchan, np.int64), np.zeros(nchan, np.int64)
        theta = np.zeros(nchan)
        for ch in sel:
            a = (float(l2[ch]) - lref) / math.pi
            j = ((ro.fix(float(rm[i]) * a) + (1 << 49)) >> 50) % 16384
            cc[ch], sc[ch] = tab[j], tab[(j - 4096) & 16383]
            theta[ch] = 2.0 * float(rm[i]) * (float(l2[ch]) - lref)
        c.update(live=True, k=22 - e, lref=lref, mean=mean, g=g, w=w, cc=cc, sc=sc, theta=theta)
    return out, used


def stokes_x(S, h, c, coherency):
    """x_I, x_Q, x_U, x_V [nchan][nbin] of the rule, double, every operation rounded on its own; garbage where unused"""
    with np.errstate(all="ignore"):
        x = [(S[p].astype(np.float64) - h.astype(np.float64) * c["mean"][p][:, None]) * c["g"][p][:, None] for p in range(4)]
        if coherency:
            x = [x[0] + x[1], 2.0 * x[2], 2.0 * x[3], x[0] - x[1]]
    return x


def derive(acc, hits, prep, cands, tfactor, coherency):
    """-> (PROF_BIN [ncand][nbin], PROF_RESULT [ncand]) from the sums"""
    ncand, nbin = hits.shape
    bins = np.zeros((ncand, nbin), dtype=post.PROF_BIN)
    res = np.zeros(ncand, dtype=post.PROF_RESULT)
    tf = float(tfactor)
    for i, c in enumerate(prep):
        r = res[i]
        r["nused"], r["on_lo_bin"], r["on_hi_bin"] = c["N"], c["on_lo_bin"], c["on_hi_bin"]
        if not c["live"]:
            continue
        r["k"], r["lref"] = c["k"], c["lref"]
        w = c["w"][:, c["sel"]]
        if coherency:
            wi = w[0] + w[1]
            W = [np.cumsum(wi)[-1], np.cumsum(4.0 * w[2])[-1], np.cumsum(4.0 * w[3])[-1], np.cumsum(wi)[-1]]      # (cumsum: in ascending order)
        else:
            W = [np.cumsum(w[p])[-1] for p in range(4)]
        sg = [math.sqrt(tf * float(v)) / (float(c["N"]) * tf) for v in W]
        r["sigma_i"], r["sigma_q"], r["sigma_u"], r["sigma_v"] = sg
        sl = math.sqrt((sg[1] * sg[1] + sg[2] * sg[2]) / 2.0)
        r["sigma_l"] = sl
        b = bins[i]
        b["hits"] = hits[i]
        ok = hits[i] > 0
        h = np.where(ok, hits[i], 1).astype(np.float64)
        a = acc[i].astype(np.float64)
        inv, inv22 = 2.0 ** -c["k"], 2.0 ** -(c["k"] + 22)
        I, Q, U, V = ((a[:, 0] * inv) / h, (a[:, 1] * inv22) / h, (a[:, 2] * inv22) / h, (a[:, 3] * inv) / h)
        L = np.sqrt(Q * Q + U * U)
        big = L >= 1.57 * sl
        Ldb = np.where(big, np.sqrt(np.where(big, L * L - sl * sl, 0.0)), 0.0)
        valid = ok & (Ldb > 0.0)
        with np.errstate(all="ignore"):
            pa_err = np.where(valid, sl / (2.0 * np.where(valid, Ldb, 1.0)), 0.0)
        for name, v in (("i", I), ("q", Q), ("u", U), ("v", V), ("l", L), ("l_db", Ldb), ("pa", np.arctan2(U, Q) / 2.0), ("pa_err", pa_err)):
            b[name] = np.where(ok, v, 0.0)
        b["pa_valid"] = valid
    return bins, res


def profile(x, hdr, cands, rm, nbin, tfactor, ref="mean", gain=None, flag=None, coherency=False, unbounded=False):
    """-> dict(acc int64 [ncand][nbin][4], hits uint32 [ncand][nbin], bins, results, used; and with `unbounded` `largest`: the
    largest sum of |terms| of any acc, added up in Python integers)"""
    prep, used = prepare(x, hdr, cands, rm, nbin, tfactor, ref, gain, flag, coherency)
    ncand = len(cands)
    acc = np.zeros((ncand, nbin, 4), np.int64)
    hits = np.zeros((ncand, nbin), np.uint32)
    largest = 0
    for i, c in enumerate(prep):
        if not c["live"]:
            continue
        S, h = bin_sums(x, c["d"], c["t0"], nbin, tfactor)
        live = (used[i] != 0)[:, None] & (h > 0)
        scale = 2.0 ** c["k"]
        with np.errstate(all="ignore"):
            X = [np.where(live, np.rint(v * scale), 0.0).astype(np.int64) for v in stokes_x(S, h, c, coherency)]
        cc, sc = c["cc"][:, None], c["sc"][:, None]
        terms = [X[0], X[1] * cc + X[2] * sc, X[2] * cc - X[1] * sc, X[3]]
        for k, t in enumerate(terms):
            acc[i, :, k] = t.sum(axis=0)
        hits[i] = np.where(live, h, 0).sum(axis=0)
        if unbounded:
            for t in terms:
                tot = [sum(int(v) for v in col) for col in np.abs(t).T]
                largest = max(largest, max(tot))
                assert all(abs(int(v)) < 1 << 47 for v in (t.max(), t.min()))
    bins, res = derive(acc, hits, prep, cands, tfactor, coherency)
    out = dict(acc=acc, hits=hits, bins=bins, results=res, used=used)
    if unbounded:
        out["largest"] = largest
    return out


def profile_fp64(x, hdr, cands, rm, nbin, tfactor, ref="mean", gain=None, flag=None, coherency=False):
    """the same definition in plain double precision: phases by cos / sin, no table, no rounding to integers ->
    dict(I, Q, U, V [ncand][nbin]; absqu: the sum over the used channels of |xQ| + |xU|; hits, N, k per candidate; xq, xu
    [ncand][nchan][nbin] of the live terms)"""
    prep, used = prepare(x, hdr, cands, rm, nbin, tfactor, ref, gain, flag, coherency)
    ncand, nchan = len(cands), hdr["nchans"]
    out = {k: np.zeros((ncand, nbin)) for k in ("I", "Q", "U", "V", "absqu")}
    out.update(hits=np.zeros((ncand, nbin), np.int64), N=np.array([c["N"] for c in prep]), k=np.array([c["k"] for c in prep]),
               live=np.array([c["live"] for c in prep]), xq=np.zeros((ncand, nchan, nbin)), xu=np.zeros((ncand, nchan, nbin)), used=used)
    for i, c in enumerate(prep):
        if not c["live"]:
            continue
        S, h = bin_sums(x, c["d"], c["t0"], nbin, tfactor)
        live = (used[i] != 0)[:, None] & (h > 0)
        xi, xq, xu, xv = (np.where(live, v, 0.0) for v in stokes_x(S, h, c, coherency))
        co, si = np.cos(c["theta"])[:, None], np.sin(c["theta"])[:, None]
        hits = np.where(live, h, 0).sum(axis=0)
        hh = np.where(hits > 0, hits, 1).astype(np.float64)
        out["I"][i], out["V"][i] = xi.sum(axis=0) / hh, xv.sum(axis=0) / hh
        out["Q"][i] = (xq * co + xu * si).sum(axis=0) / hh
        out["U"][i] = (xu * co - xq * si).sum(axis=0) / hh
        out["absqu"][i] = (np.abs(xq) + np.abs(xu)).sum(axis=0)
        out["hits"][i] = hits
        out["xq"][i], out["xu"][i] = xq, xu
    return out
