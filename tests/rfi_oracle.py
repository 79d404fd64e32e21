"""numpy restatement of the interference stage (frbch_rfi_*; include/frbch.h states it): the block statistics, the mask rule
step by step, and the replacement of the masked cells.  Plain, slow and literal: every comparison against it is `==`.

x is ONE product of the rows, [nrows][nchan].  Integer rows: the sums are exact.  Float rows: S and Q are added row by row in
ascending order, every operation an IEEE double operation of its own -- which numpy's element-wise operations are."""
import numpy as np


def block_edges(nrows, block_rows):
    """[(first row, one past the last)] -- the last block may be short"""
    return [(r0, min(nrows, r0 + block_rows)) for r0 in range(0, nrows, block_rows)]


def stats(x, block_rows):
    """-> [nblk][nchan][2] = (S, Q): uint64 for integer rows, float64 for float rows"""
    x = np.asarray(x)
    edges = block_edges(x.shape[0], block_rows)
    if x.dtype == np.float32:
        out = np.zeros((len(edges), x.shape[1], 2), dtype=np.float64)
        for b, (r0, r1) in enumerate(edges):
            s = np.zeros(x.shape[1], dtype=np.float64)
            q = np.zeros(x.shape[1], dtype=np.float64)
            with np.errstate(all="ignore"):
                for t in range(r0, r1):
                    v = x[t].astype(np.float64)
                    vv = v * v
                    s = s + v
                    q = q + vv
            out[b, :, 0], out[b, :, 1] = s, q
        return out
    out = np.zeros((len(edges), x.shape[1], 2), dtype=np.uint64)
    for b, (r0, r1) in enumerate(edges):
        xb = x[r0:r1].astype(np.uint64)
        out[b, :, 0] = xb.sum(axis=0, dtype=np.uint64)
        out[b, :, 1] = (xb * xb).sum(axis=0, dtype=np.uint64)
    return out


def median(v):
    """0.5 * (lower middle + upper middle) of the sorted values"""
    s = np.sort(np.asarray(v, dtype=np.float64))
    n = s.size
    return np.float64(0.5) * (s[(n - 1) // 2] + s[n // 2])


def mask(st, nrows, block_rows, nbits, t_cell=5.0, t_chan=5.0, chan_frac=0.3, block_frac=0.3, zap=None, prior=None, want_steps=False):
    """the rule, steps 1 to 8 -> dict(mask uint8 [nblk][nchan], repl float64 [nchan], chan_flag, blk_flag bool)"""
    st = np.asarray(st)
    nblk, nchan = st.shape[:2]
    edges = block_edges(nrows, block_rows)
    assert len(edges) == nblk
    n_b = np.array([r1 - r0 for r0, r1 in edges], dtype=np.float64)
    nan = np.float64("nan")
    with np.errstate(all="ignore"):
        # 1. per cell
        S, Q = st[:, :, 0].astype(np.float64), st[:, :, 1].astype(np.float64)
        mean = S / n_b[:, None]
        var = Q / n_b[:, None] - mean * mean
        var = np.where(var < 0.0, 0.0, var)
        std = np.sqrt(var)
        bad = ~(np.isfinite(mean) & np.isfinite(std))
        # 2. per channel, over its non-bad blocks
        m_c, s_c, dm_c, ds_c = (np.full(nchan, nan) for _ in range(4))
        for c in range(nchan):
            ok = ~bad[:, c]
            if ok.any():
                m_c[c] = median(mean[ok, c])
                s_c[c] = median(std[ok, c])
                dm_c[c] = np.float64(1.4826) * median(np.abs(mean[ok, c] - m_c[c]))
                ds_c[c] = np.float64(1.4826) * median(np.abs(std[ok, c] - s_c[c]))
        # 3. cells
        cell = bad.copy()
        for b in range(nblk):
            fm = s_c / np.sqrt(n_b[b])
            fs = s_c / np.sqrt(np.float64(2.0) * n_b[b])
            lim_m = np.float64(t_cell) * np.where(dm_c > fm, dm_c, fm)
            lim_s = np.float64(t_cell) * np.where(ds_c > fs, ds_c, fs)
            hit = (np.abs(mean[b] - m_c) > lim_m) | (np.abs(std[b] - s_c) > lim_s)
            cell[b] |= hit & ~bad[b]
        # 4. whole channels: zapped, dead, nothing to measure
        chan = np.zeros(nchan, dtype=bool) if zap is None else np.asarray(zap).astype(bool).copy()
        chan |= s_c == 0.0
        chan |= bad.all(axis=0)
        after4 = chan.copy()
        # 5. across channels
        if t_chan > 0.0 and (~chan).any():
            rest = ~chan
            M = median(s_c[rest])
            D = np.float64(1.4826) * median(np.abs(s_c[rest] - M))
            chan |= rest & (np.abs(s_c - M) > np.float64(t_chan) * D)
        after5 = chan.copy()
        # 6. fractions
        ncell = cell.sum(axis=0)
        chan |= ~chan & (ncell.astype(np.float64) > np.float64(chan_frac) * np.float64(nblk))
        rest = ~chan
        n_u = int(rest.sum())
        blk = cell[:, rest].sum(axis=1).astype(np.float64) > np.float64(block_frac) * np.float64(n_u)
        # 7. the mask
        m = cell | chan[None, :] | blk[:, None]
        if prior is not None:
            m = m | np.asarray(prior).astype(bool)
        # 8. replacement values
        repl = np.zeros(nchan, dtype=np.float64)
        for c in range(nchan):
            keep = ~m[:, c]
            r = median(mean[keep, c]) if keep.any() else m_c[c]
            if not np.isfinite(r):
                r = np.float64(0.0)
            if nbits != 32:
                r = min(max(np.floor(r + np.float64(0.5)), 0.0), float(2 ** nbits - 1))
            repl[c] = r
    out = dict(mask=m.astype(np.uint8), repl=repl, chan_flag=chan, blk_flag=blk)
    if want_steps:
        out.update(mean=mean, std=std, bad=bad, cell=cell, m_c=m_c, s_c=s_c, after4=after4, after5=after5, ncell=ncell, n_u=n_u)
    return out


def apply(rows, prod, block_rows, m, repl):
    """a copy of rows [nrows][nifs][nchan] with every sample of product `prod` in a masked cell set to repl[c]"""
    out = np.array(rows, copy=True)
    for b, (r0, r1) in enumerate(block_edges(out.shape[0], block_rows)):
        cols = np.flatnonzero(m[b])
        if cols.size:
            out[r0:r1, prod, cols] = np.asarray(repl)[cols].astype(out.dtype)
    return out
