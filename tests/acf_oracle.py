"""Numpy restatement of the structure of a burst (include/frbch.h, "structure of a burst"): the dedispersed dynamic spectrum per
(candidate, subband, bin) from the DM scan's terms, the complete cells, the quantised int32 plane, the two-dimensional
autocorrelation of a plane in int64 -- with the bound of the header restated as assertions in Python integers --, the pair
counts, and the derivation of the widths and the drift in plain Python floats (every operation rounded on its own).  The host
preparation and the bin sums are tests/dmscan_oracle.py's.  Test infrastructure only."""
import numpy as np

from frb_baseband_amd import post
from tests import dmscan_oracle as do

Y_MAX = 1 << 21


def dynspec(x, hdr, cands, nbin, tfactor, ffactor, flag=None, coherency=False):
    """-> dict(Y int64 [ncand][nsub][nbin], yhits uint32, mask uint8, used, k, nused, nused_s, largest: the largest |X| seen)"""
    prep, used, xs = do.prepare(x, hdr, cands, nbin, tfactor, flag, coherency)
    ncand, nchan = len(cands), hdr["nchans"]
    assert nchan % ffactor == 0
    nsub = nchan // ffactor
    Y = np.zeros((ncand, nsub, nbin), np.int64)
    yhits = np.zeros((ncand, nsub, nbin), np.uint32)
    mask = np.zeros((ncand, nsub, nbin), np.uint8)
    nused_s = used.reshape(ncand, nsub, ffactor).sum(axis=2).astype(np.uint32)
    largest = 0
    for i, c in enumerate(prep):
        if not c["N"]:
            continue
        S, h = do.bin_sums(xs, do.delays(hdr, cands[i]["dm"]), c["t0"], nbin, tfactor)
        live = c["ok"][:, None] & (h > 0)
        xv = (S.astype(np.float64) - h.astype(np.float64) * c["mean"][:, None]) * c["w"][:, None]
        X = np.where(live, np.rint(xv * 2.0 ** c["k"]), 0.0).astype(np.int64)
        largest = max(largest, int(np.abs(X).max()))
        assert largest <= 1 << 40                                   # |X| <= 2^40: |Y| <= 2^40 ffactor <= 2^54
        Y[i] = X.reshape(nsub, ffactor, nbin).sum(axis=1)
        yhits[i] = np.where(live, h, 0).reshape(nsub, ffactor, nbin).sum(axis=1)
        mask[i] = (nused_s[i][:, None] > 0) & (yhits[i] == tfactor * nused_s[i][:, None])
    return dict(Y=Y, yhits=yhits, mask=mask, used=used, k=np.array([c["k"] for c in prep], np.int32),
                nused=np.array([c["N"] for c in prep], np.uint32), nused_s=nused_s, largest=largest)


def quantise(Y, mask):
    """-> (y int32 [ncand][nsub][nbin], r uint32 [ncand])"""
    y = np.zeros(Y.shape, np.int32)
    r = np.zeros(Y.shape[0], np.uint32)
    for i in range(Y.shape[0]):
        ok = mask[i] != 0
        m = int(np.abs(Y[i][ok]).max()) if ok.any() else 0
        r[i] = max(0, m.bit_length() - 21)
        ri = int(r[i])
        q = (Y[i] + (1 << (ri - 1))) >> ri if ri > 0 else Y[i]
        y[i] = np.where(ok, q, 0)
        assert int(np.abs(y[i].astype(np.int64)).max()) <= Y_MAX     # the contract of the ACF stage
    return y, r


def acf2d(y, nlagf, nlagt):
    """y int [nsub][nbin] with |y| <= 2^21 -> A int64 [nlagf][2 nlagt - 1]; the header's bound asserted: the sum of |products|
    of the lag with the most terms, in Python integers, stays below 2^63, and no int64 dot product may then wrap"""
    y = np.asarray(y).astype(np.int64)
    nsub, nbin = y.shape
    assert nsub * nbin <= 1 << 20 and int(np.abs(y).max()) <= Y_MAX
    # every |A| <= the sum of y^2 (Cauchy-Schwarz), formed here in Python integers from row sums (<= 2^10 2^42 each)
    assert sum(int(v) for v in (y * y).sum(axis=1)) <= (1 << 42) * nsub * nbin <= 1 << 62
    A = np.zeros((nlagf, 2 * nlagt - 1), np.int64)
    for df in range(nlagf):
        a, b = y[:nsub - df], y[df:]
        for dt in range(-(nlagt - 1), nlagt):
            if dt >= 0:
                A[df, dt + nlagt - 1] = np.vdot(a[:, :nbin - dt], b[:, dt:])
            else:
                A[df, dt + nlagt - 1] = np.vdot(a[:, -dt:], b[:, :nbin + dt])
    return A


def acf2d_planes(y, nlagf, nlagt):
    return np.stack([acf2d(p, nlagf, nlagt) for p in y])


def pairs_closed_form(nsub, nbin, nlagf, nlagt):
    df = np.arange(nlagf)[:, None]
    dt = np.abs(np.arange(-(nlagt - 1), nlagt))[None, :]
    return ((nsub - df) * (nbin - dt)).astype(np.uint32)


def half_width(v):
    """-> (x, fitted) of a cut v[0 .. nl - 1] whose lag 0 is left out"""
    nl = len(v)
    if nl < 2 or not v[1] > 0.0:
        return 0.0, 0
    h = v[1] / 2.0
    for d in range(2, nl):
        if v[d] < h:
            a, b = v[d - 1] - h, v[d - 1] - v[d]
            return float(d - 1) + a / b, 1
    return float(nl - 1), 0


def fit(hdr, A, P, k, r, nused, ncomplete, tfactor, ffactor, fit_frac):
    """-> (norm float64 like A, results ACF_RESULT [ncand]); plain Python floats, every operation rounded on its own"""
    ncand, nlf, ndt = A.shape
    L = ndt // 2
    nlt = L + 1
    norm = np.zeros(A.shape)
    res = np.zeros(ncand, dtype=post.ACF_RESULT)
    unit_t = (float(tfactor) * float(hdr["tsamp"])) * 1000.0
    unit_f = float(ffactor) * float(hdr["foff"])
    for i in range(ncand):
        if not nused[i]:
            continue
        R = res[i]
        R["k"], R["r"], R["nused"], R["ncomplete"] = k[i], r[i], nused[i], ncomplete[i]
        q = 2.0 ** (-2 * (int(k[i]) - int(r[i])))
        nm = [[(float(int(A[i, df, x])) * q) / float(int(P[i, df, x])) if P[i, df, x] else 0.0 for x in range(ndt)] for df in range(nlf)]
        norm[i] = nm
        xf, R["fitted_f"] = half_width([nm[d][L] for d in range(nlf)])
        R["width_f_mhz"] = xf * abs(unit_f)
        xt, R["fitted_t"] = half_width([nm[0][L + d] for d in range(nlt)])
        R["width_t_ms"] = xt * unit_t
        others = [nm[df][x] for df in range(nlf) for x in range(ndt) if not (df == 0 and x == L)]
        ref = max(others) if others else 0.0
        R["ref"] = ref
        if not ref > 0.0:
            continue
        thr = fit_frac * ref
        mff = mtf = mtt = 0.0
        for df in range(nlf):
            for x in range(ndt):
                dt = x - L
                if (df == 0 and dt <= 0) or not nm[df][x] >= thr:
                    continue
                v = nm[df][x]
                mff = mff + v * float(df * df)
                mtf = mtf + v * float(df * dt)
                mtt = mtt + v * float(dt * dt)
        R["mff"], R["mtf"], R["mtt"] = 2.0 * mff, 2.0 * mtf, 2.0 * mtt
        if not R["mff"] > 0.0:
            continue
        ms = (float(R["mtf"]) / float(R["mff"])) * unit_t
        R["dt_df"] = ms / unit_f
        R["drift"] = 1.0 / float(R["dt_df"]) if R["dt_df"] != 0.0 else 0.0
        R["fitted_d"] = 1
    return norm, res


def burst_acf(x, hdr, cands, nbin, tfactor, ffactor, nlagf, nlagt, fit_frac=0.5, flag=None, coherency=False):
    """everything -> dict(Y, yhits, mask, y, A, P, norm, results, used, k, r, nused, ncomplete, largest)"""
    out = dynspec(x, hdr, cands, nbin, tfactor, ffactor, flag, coherency)
    y, r = quantise(out["Y"], out["mask"])
    A = acf2d_planes(y, nlagf, nlagt)
    P = acf2d_planes(out["mask"], nlagf, nlagt).astype(np.uint32)
    ncomplete = out["mask"].reshape(len(cands), -1).sum(axis=1).astype(np.uint32)
    norm, res = fit(hdr, A, P, out["k"], r, out["nused"], ncomplete, tfactor, ffactor, fit_frac)
    out.update(y=y, r=r, A=A, P=P, ncomplete=ncomplete, norm=norm, results=res)
    return out
