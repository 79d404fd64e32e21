"""numpy restatement of the periodicity test of the interference stage (frbch_rfi_peaks_*, frbch_rfi_periodic; include/frbch.h
states it): the radix-2 transform of every (block, channel pair) in float32 with every operation rounded on its own -- which
numpy's element-wise float32 operations are --, the per-channel peak, and the decision in double.  Plain, slow and literal:
every comparison against it is `==`.

x is ONE product of the rows, [nrows][nchan]; st is tests/rfi_oracle.stats of the same rows and block length."""
import numpy as np

from tests.rfi_oracle import block_edges

PEAK = np.dtype([("num", "<f4"), ("k", "<u4")])
F32 = np.float32


def valid_n(n):
    return 8 <= n <= 4096 and n & (n - 1) == 0


def twiddles(n):
    """W[k] = ((float)cos(a), (float)(-sin(a))), a = 2.0 pi k / n in double -> (wr, wi) float32 [n / 2]"""
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
    """Z = DFT_n(z) of float32 arrays [..., n] (the last axis is the transform's): decimation in time on the bit-reversed input,
    stages s = 1 .. log2 n, t = (wr vr - wi vi, wr vi + wi vr), u' = u + t, v' = u - t -> (Zr, Zi)"""
    n = zr.shape[-1]
    assert valid_n(n) and zr.dtype == F32 and zi.dtype == F32
    wr, wi = twiddles(n)
    rev = bitrev(n)
    xr, xi = np.array(zr[..., rev]), np.array(zi[..., rev])
    L = n.bit_length() - 1
    with np.errstate(all="ignore"):
        for s in range(1, L + 1):
            half = 1 << (s - 1)
            i = np.arange(n // 2)
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


def cell_moments(st, nrows, block_rows):
    """step 1 of frbch_rfi_mask -> (n_b [nblk], mean [nblk][nchan], var [nblk][nchan]) in double"""
    st = np.asarray(st)
    n_b = np.array([r1 - r0 for r0, r1 in block_edges(nrows, block_rows)], dtype=np.float64)
    with np.errstate(all="ignore"):
        S, Q = st[:, :, 0].astype(np.float64), st[:, :, 1].astype(np.float64)
        mean = S / n_b[:, None]
        var = Q / n_b[:, None] - mean * mean
        var = np.where(var < 0.0, 0.0, var)
    return n_b, mean, var


def tested_cells(st, nrows, block_rows):
    n_b, mean, var = cell_moments(st, nrows, block_rows)
    return (2 * n_b[:, None] >= block_rows) & np.isfinite(mean) & np.isfinite(var) & (var != 0.0)


def peaks(x, st, block_rows):
    """-> PEAK [nblk][nchan]: the largest N[k], k = 1 .. n/2 - 1, and the lowest k that attains it; {0, 0} where not tested"""
    x = np.asarray(x)
    nrows, nchan = x.shape
    n = block_rows
    assert valid_n(n)
    edges = block_edges(nrows, n)
    _n_b, mean, _var = cell_moments(st, nrows, n)
    tested = tested_cells(st, nrows, n)
    out = np.zeros((len(edges), nchan), dtype=PEAK)
    npair = (nchan + 1) // 2
    for b, (r0, r1) in enumerate(edges):
        z = np.zeros((2 * npair, n), dtype=F32)                       # [channel][j]; an odd last channel has a zero partner
        with np.errstate(all="ignore"):
            d = (x[r0:r1].astype(np.float64) - mean[b][None, :]).astype(F32)
        d[:, ~tested[b]] = 0.0
        z[:nchan, : r1 - r0] = d.T
        Zr, Zi = fft(np.ascontiguousarray(z[0::2]), np.ascontiguousarray(z[1::2]))
        k = np.arange(1, n // 2)
        Ar, Ai, Br, Bi = Zr[:, k], Zi[:, k], Zr[:, n - k], Zi[:, n - k]
        with np.errstate(all="ignore"):
            s0, d0, s1, d1 = Ar + Br, Ai - Bi, Ai + Bi, Br - Ar
            N = np.empty((2 * npair, k.size), dtype=F32)
            N[0::2] = s0 * s0 + d0 * d0
            N[1::2] = s1 * s1 + d1 * d1
        assert N.dtype == F32
        for c in range(nchan):                                         # the walk over ascending k: a NaN never replaces
            row = np.where(np.isnan(N[c]), F32(0.0), N[c])
            best = row.max()
            if best > 0.0:
                out[b, c] = (best, int(k[np.flatnonzero(row == best)[0]]))
    return out


def periodic(st, pk, nrows, block_rows, t_pow, chan_frac):
    """the decision -> dict(pflag uint8 [nblk][nchan], pchan bool [nchan], power float64 [nblk][nchan])"""
    n_b, _mean, var = cell_moments(st, nrows, block_rows)
    tested = tested_cells(st, nrows, block_rows)
    nblk = len(n_b)
    with np.errstate(all="ignore"):
        den = (np.float64(4.0) * n_b)[:, None] * var
        power = np.where(tested, pk["num"].astype(np.float64) / den, 0.0)
    cell = power > np.float64(t_pow)
    pchan = cell.sum(axis=0).astype(np.float64) > np.float64(chan_frac) * np.float64(nblk)
    return dict(pflag=(cell | pchan[None, :]).astype(np.uint8), pchan=pchan, power=power)


def t_pow_of(sigma, n):
    """-ln(q / (n/2 - 1)), q = erfc(sigma / sqrt 2) / 2: the power one of n/2 - 1 exponential bins exceeds with the probability of
    `sigma` Gaussian sigma"""
    import math
    return -math.log(0.5 * math.erfc(sigma / math.sqrt(2.0)) / (n // 2 - 1))
