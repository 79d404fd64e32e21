"""numpy restatement of the all-product fold with a phase model (include/frbch.h, frbch_foldp_*).  TEST INFRASTRUCTURE
ONLY: it imports nothing of the product.  Every step is one numpy operation on float64 arrays -- one IEEE operation
rounded on its own, as the kernels compute it -- so bins agree bit for bit.

  model                 rule
  --------------------  -----------------------------------------------------------------------------------------
  polynomial (nseg 0)   tau = (tstart - PEPOCH) 86400 + t tsamp [- delay_c];  doppler != 0: tau = tau + tau doppler;
                        turns = F0 tau + ((F1 / 2) tau) tau
  polyco block s        sec = t tsamp [- delay_c];  dt = (tstart - TMID_s) 1440 + sec / 60;
                        turns = (rphase + (dt 60) F0_s) + horner(coeff_s, dt)      (TEMPO: DT in minutes)
  block of a row        block s >= 1 starts at ceil(((0.5 (TMID_{s-1} + TMID_s) - tstart) 86400) / tsamp), clamped to
                        [0, nrows]; row t uses the last block that has started
  bin                   min(int((turns - floor(turns)) nbin), nbin - 1)
"""
from __future__ import annotations

import numpy as np

DM_CONST = 1.0 / 2.41e-4


def delays_seconds(fch1, foff, nchan, dm):
    fc = fch1 + np.arange(nchan, dtype=np.float64) * foff
    fhi = fch1 if foff < 0 else fc[-1]
    return dm * DM_CONST * (1.0 / (fc * fc) - 1.0 / (fhi * fhi))


def block_first_rows(segs, tstart_mjd, tsamp, nrows):
    first = [0]
    for a, b in zip(segs[:-1], segs[1:]):
        x = ((0.5 * (a["tmid"] + b["tmid"]) - tstart_mjd) * 86400.0) / tsamp
        first.append(0 if x <= 0 else int(min(np.ceil(x), nrows)))
    return np.asarray(first, dtype=np.int64)


def polyco_turns(seg, tstart_mjd, sec):
    """turns of one block at `sec` seconds after the start of the file (array)"""
    dt = (tstart_mjd - seg["tmid"]) * 1440.0 + sec / 60.0
    c = seg["coeff"]
    h = np.full_like(dt, c[-1])
    for k in range(len(c) - 2, -1, -1):
        h = h * dt
        h = h + c[k]
    lin = (dt * 60.0) * seg["f0"]
    return (seg["rphase"] + lin) + h


def bins(nrows, nchan, *, fch1, foff, tsamp, tstart_mjd, nbin, dm=0.0, apply_delays=False, segs=None, f0=0.0, f1=0.0,
         pepoch_mjd=None, doppler=0.0):
    """-> int64 [nrows][nchan] phase bins"""
    t = np.arange(nrows, dtype=np.float64)
    tt = t * tsamp
    dly = delays_seconds(fch1, foff, nchan, dm) if (apply_delays and dm != 0.0) else None
    out = np.empty((nrows, nchan), dtype=np.int64)
    if segs:
        which = np.searchsorted(block_first_rows(segs, tstart_mjd, tsamp, nrows)[1:], np.arange(nrows), side="right")
    for c in range(nchan):
        if segs:
            sec = tt - dly[c] if dly is not None else tt
            turns = np.empty(nrows)
            for s, seg in enumerate(segs):
                m = which == s
                turns[m] = polyco_turns(seg, tstart_mjd, sec[m])
        else:
            tau = (tstart_mjd - (tstart_mjd if pepoch_mjd is None else pepoch_mjd)) * 86400.0 + tt
            if dly is not None:
                tau = tau - dly[c]
            if doppler != 0.0:
                tau = tau + tau * doppler
            turns = f0 * tau + ((0.5 * f1) * tau) * tau
        fr = turns - np.floor(turns)
        out[:, c] = np.minimum((fr * nbin).astype(np.int64), nbin - 1)
    return out


def fold_all(x, *, tsamp, nbin, subint_s, **model):
    """x: [nrows][nifs][nchan].  -> (sums float64 [nsub][nifs][nchan][nbin], hits uint32 [nsub][nchan][nbin])"""
    x = np.asarray(x)
    nrows, nifs, nchan = x.shape
    rps = max(1, int(round(subint_s / tsamp)))
    nsub = (nrows + rps - 1) // rps
    b = bins(nrows, nchan, tsamp=tsamp, nbin=nbin, **model)
    sub = (np.arange(nrows) // rps).astype(np.int64)
    prof = np.zeros((nsub, nifs, nchan, nbin))
    hits = np.zeros((nsub, nchan, nbin), dtype=np.uint32)
    for c in range(nchan):
        flat = sub * nbin + b[:, c]
        hits[:, c, :] = np.bincount(flat, minlength=nsub * nbin).reshape(nsub, nbin)
        for q in range(nifs):
            prof[:, q, c, :] = np.bincount(flat, weights=x[:, q, c].astype(np.float64), minlength=nsub * nbin).reshape(nsub, nbin)
    return prof, hits
