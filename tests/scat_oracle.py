"""Numpy restatement of the scattering of a burst (include/frbch.h, "scattering of a burst"): the bank of scattered Gaussians by
its formula (for the bank test only -- everything downstream TAKES the bank as an input, the library's own, so that it can be
held to the bit), the template-bank stage in int64 -- with the bound of the header restated as assertions in Python integers --,
the closed form of N, and the fit in plain Python floats (every operation rounded on its own).  The dynamic spectrum and the
quantised plane are tests/acf_oracle.py's.  Test infrastructure only."""
import math

import numpy as np

from frb_baseband_amd import post
from tests import acf_oracle as ao

Y_MAX, P_MAX = 1 << 21, 1 << 30


def bank_formula(nsig, ntau, ntap, lead, sigma0, rsig, tau0, rtau):
    """the header's formula in numpy (exp may differ from the library's in a last bit) -> dict(p, s1, cum, tail, sigma, tau)"""
    sigma, tau = [float(sigma0)], [float(tau0)]
    for _ in range(1, nsig):
        sigma.append(sigma[-1] * float(rsig))
    for _ in range(1, ntau):
        tau.append(tau[-1] * float(rtau))
    K = nsig * ntau
    p = np.zeros((K, ntap), np.int32)
    tail = np.zeros(K)
    d = np.arange(ntap, dtype=np.float64) - float(lead)
    n = np.arange(ntap, dtype=np.float64)
    for a in range(nsig):
        g = np.exp(-(d * d) / (2.0 * (sigma[a] * sigma[a])))
        for b in range(ntau):
            e = np.exp(-n / tau[b])
            f = np.zeros(ntap)
            for m in range(ntap):
                acc = 0.0
                for t in (g[m::-1] * e[:m + 1]).tolist():           # n ascending: g[m - n] e[n]
                    acc = acc + t
                f[m] = acc
            fmax = f.max()
            p[a * ntau + b] = np.rint((f / fmax) * 32768.0).astype(np.int32)
            tail[a * ntau + b] = f[-1] / fmax
    out = dict(p=p, tail=tail, sigma=np.array(sigma), tau=np.array(tau))
    out.update(bank_sums(p))
    return out


def bank_sums(p):
    """S1 and the prefix sums of p^2 of a bank, exactly"""
    p = np.asarray(p).astype(np.int64)
    cum = np.zeros((p.shape[0], p.shape[1] + 1), np.int64)
    np.cumsum(p * p, axis=1, out=cum[:, 1:])
    return dict(s1=p.sum(axis=1), cum=cum)


def tbank(y, P, lead, shift0, nshift):
    """y int [n][nsub][nbin] with |y| <= 2^21, P int [K][ntap] with |P| <= 2^30 -> C int64 [n][nsub][K][nshift]; the header's
    bound asserted in Python integers: the sum of |products| of any output stays below 2^61 < 2^63"""
    y, P = np.asarray(y).astype(np.int64), np.asarray(P).astype(np.int64)
    n, nsub, nbin = y.shape
    K, ntap = P.shape
    assert 0 <= lead < ntap <= 1024 and shift0 >= 0 and nshift >= 1 and shift0 + nshift <= nbin
    assert int(np.abs(y).max()) <= Y_MAX and int(np.abs(P).max()) <= P_MAX
    assert int(np.abs(y).max()) * int(np.abs(P).max()) * ntap <= 1 << 61
    # the rows laid out so that tap m of shift u reads column u + m; bins outside the row are zero terms, i.e. absent
    padded = np.zeros((n, nsub, nshift + ntap - 1), np.int64)
    j = shift0 - lead + np.arange(nshift + ntap - 1)
    ok = (j >= 0) & (j < nbin)
    padded[:, :, ok] = y[:, :, j[ok]]
    C = np.zeros((n, nsub, K, nshift), np.int64)
    for u in range(nshift):
        C[:, :, :, u] = padded[:, :, u:u + ntap] @ P.T
    return C


def energy_closed_form(cum, nbin, lead, shift0, nshift):
    """N of a complete row: cum[hi] - cum[lo] -> int64 [K][nshift]"""
    ntap = cum.shape[1] - 1
    out = np.zeros((cum.shape[0], nshift), np.int64)
    for u in range(nshift):
        j0 = shift0 + u - lead
        out[:, u] = cum[:, min(ntap, nbin - j0)] - cum[:, max(0, -j0)]
    return out


def noise_variance(tfactor, nused_s, k, r):
    """v_s: a term of one row of one used channel has unit variance in the DM scan's S/N, a complete cell holds tfactor nused_s"""
    return (float(tfactor) * float(nused_s)) * 2.0 ** (2 * (int(k) - int(r)))


def shifts_of(alpha, freqs, nu_ref, rtau):
    """the unrounded d_s(alpha) -- the case builder keeps them off the half-integers"""
    lrt = math.log(float(rtau))
    return [((-float(alpha)) * math.log(float(f) / nu_ref)) / lrt for f in freqs]


def fit(hdr, C, N, k, r, nused, nused_s, bank, bankpar, tfactor, ffactor, shift0, alphas, snr_min):
    """-> (q float64 like C, sub SCAT_SUB [ncand][nsub], band SCAT_BAND [ncand]); plain Python floats"""
    ncand, nsub, K, nsh = C.shape
    nsig, ntau, rtau = bankpar["nsig"], bankpar["ntau"], float(bankpar["rtau"])
    sigma, tau, s1 = [float(v) for v in bank["sigma"]], [float(v) for v in bank["tau"]], [int(v) for v in bank["s1"]]
    q = np.zeros(C.shape)
    sub = np.zeros((ncand, nsub), dtype=post.SCAT_SUB)
    band = np.zeros(ncand, dtype=post.SCAT_BAND)
    unit = (float(tfactor) * float(hdr["tsamp"])) * 1000.0
    fch1, foff, nchan = float(hdr["fch1"]), float(hdr["foff"]), hdr["nchans"]
    nu_ref = fch1 + (float(nchan - 1) / 2.0) * foff
    lrt = math.log(rtau)
    for i in range(ncand):
        B = band[i]
        B["k"], B["r"], B["nused"], B["nu_ref_mhz"] = k[i], r[i], nused[i], nu_ref
        kr = int(k[i]) - int(r[i])
        part = []
        for s in range(nsub):
            R = sub[i, s]
            nu = int(nused_s[i, s])
            R["nused"] = nu
            R["freq_mhz"] = fch1 + (float(s * ffactor) + float(ffactor - 1) / 2.0) * foff
            if nu:
                c, nn = C[i, s].astype(np.float64), N[i, s].astype(np.float64)          # exact: |C| < 2^53 is asserted by the callers' cases
                assert int(np.abs(C[i, s]).max()) < 1 << 53 and int(N[i, s].max()) < 1 << 53
                vs = noise_variance(tfactor, nu, k[i], r[i])
                with np.errstate(all="ignore"):
                    q[i, s] = np.where((N[i, s] > 0) & (C[i, s] > 0), ((c * c) / nn) / vs, 0.0)
            qs = q[i, s]
            best = int(np.argmax(qs))                                # the first largest, k then u ascending
            qb = float(qs.reshape(-1)[best])
            if not qb > 0.0:
                continue
            kb, ub = divmod(best, nsh)
            ab, bb = divmod(kb, ntau)
            R["k"], R["u"], R["q"], R["snr"] = kb, ub, qb, math.sqrt(qb)
            R["sigma"], R["tau"], R["arrival"] = sigma[ab], tau[bb], float(shift0 + ub)
            R["sigma_ms"], R["tau_ms"], R["arrival_ms"] = sigma[ab] * unit, tau[bb] * unit, float(shift0 + ub) * unit
            amp = float(int(C[i, s, kb, ub])) / float(int(N[i, s, kb, ub]))
            R["amp"] = amp * 2.0 ** (15 - kr)
            R["area"] = (amp * float(s1[kb])) * 2.0 ** (-kr)
            prof = qs.reshape(nsig, ntau, nsh).max(axis=(0, 2))
            within = np.nonzero(prof >= qb - 1.0)[0]
            lo, hi = min(int(within.min()), bb), max(int(within.max()), bb)
            R["tau_lo"], R["tau_hi"] = tau[lo] * unit, tau[hi] * unit
            R["bounded_lo"], R["bounded_hi"] = int(lo > 0), int(hi + 1 < ntau)
            R["dq_unscattered"] = qb - float(prof[0])
            if float(R["snr"]) >= snr_min:
                part.append(s)
        B["nfit"] = len(part)
        if not part:
            continue
        qp = q[i][part].reshape(len(part), nsig, ntau, nsh)
        freqs = [float(sub[i, s]["freq_mhz"]) for s in part]
        Qb, arg = -1.0, None
        prof_b, prof_a = np.zeros(ntau), np.zeros(len(alphas))
        for ia, alpha in enumerate(alphas):
            ds = [int(np.rint(((-float(alpha)) * math.log(f / nu_ref)) / lrt)) for f in freqs]
            for br in range(ntau):
                Q = np.zeros((nsig, nsh))
                for x, d in enumerate(ds):                           # s ascending, from 0.0
                    Q = Q + qp[x, :, min(max(br + d, 0), ntau - 1), :]
                m = float(Q.max())
                if m > Qb:
                    a, u = divmod(int(np.argmax(Q)), nsh)
                    Qb, arg = m, (ia, br, a, u)
                prof_b[br] = max(prof_b[br], m)
                prof_a[ia] = max(prof_a[ia], m)
        ia, br, a, u = arg
        B["q"], B["ialpha"], B["b_ref"], B["a"], B["u"] = Qb, ia, br, a, u
        B["alpha"], B["tau_ref"], B["tau_ref_ms"] = float(alphas[ia]), tau[br], tau[br] * unit
        B["sigma"], B["sigma_ms"], B["arrival"], B["arrival_ms"] = sigma[a], sigma[a] * unit, float(shift0 + u), float(shift0 + u) * unit
        ds = [int(np.rint(((-float(alphas[ia])) * math.log(f / nu_ref)) / lrt)) for f in freqs]
        B["nclipped"] = sum(1 for d in ds if not 0 <= br + d <= ntau - 1)
        within = np.nonzero(prof_b >= Qb - 1.0)[0]
        lo, hi = min(int(within.min()), br), max(int(within.max()), br)
        B["tau_ref_lo"], B["tau_ref_hi"] = tau[lo] * unit, tau[hi] * unit
        B["bounded_lo"], B["bounded_hi"] = int(lo > 0), int(hi + 1 < ntau)
        ok = [float(alphas[x]) for x in range(len(alphas)) if prof_a[x] >= Qb - 1.0] + [float(alphas[ia])]
        B["alpha_lo"], B["alpha_hi"] = min(ok), max(ok)
    return q, sub, band


def burst_scatter(x, hdr, cands, nbin, tfactor, ffactor, bank, bankpar, shift0, nshift, alphas, snr_min, flag=None, coherency=False):
    """everything, with the bank (what post.scat_bank returns) and its parameters (a dict with nsig, ntau, rtau, lead) as inputs ->
    dict(Y, yhits, mask, y, C, N, q, sub, band, used, k, r, nused, nused_s)"""
    out = ao.dynspec(x, hdr, cands, nbin, tfactor, ffactor, flag, coherency)
    y, r = ao.quantise(out["Y"], out["mask"])
    lead = bankpar["lead"]
    C = tbank(y, bank["p"], lead, shift0, nshift)
    psq = bank["p"].astype(np.int64) ** 2
    N = tbank(out["mask"], psq, lead, shift0, nshift)
    assert int(np.abs(C).max()) < 1 << 46 and int(N.max()) < 1 << 40       # the composite's products are small
    q, sub, band = fit(hdr, C, N, out["k"], r, out["nused"], out["nused_s"], bank, bankpar, tfactor, ffactor, shift0, list(alphas), snr_min)
    out.update(y=y, r=r, C=C, N=N, q=q, sub=sub, band=band)
    return out
