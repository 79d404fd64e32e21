"""Numpy restatement of the band-limited single-pulse search (include/frbch.h, "band-limited single-pulse search"): the list
of bands, the series of every band, the search of the plane and the grouping of its records.  The delays, the clip and the
zero-DM row sums are oracle/post_oracle.py's, the search of one series tests/spsearch_oracle.py's: nothing of the library is
used here."""
import numpy as np

from oracle import post_oracle as po
from tests import spsearch_oracle as so

SPB_CAND = np.dtype([("dm_index", "<u4"), ("width", "<u4"), ("sample", "<u8"), ("sigma", "<f4"), ("sub_lo", "<u2"), ("sub_hi", "<u2")])
SPB_GROUP = np.dtype([("best", SPB_CAND), ("nmember", "<u4"), ("dm_index_lo", "<u4"), ("dm_index_hi", "<u4"), ("sub_lo_min", "<u2"),
                      ("sub_hi_max", "<u2"), ("sample_lo", "<u8"), ("sample_hi", "<u8"), ("full_sigma", "<f4"), ("reserved", "<u4")])


def band_list(nsub, min_sub=0, max_sub=0):
    """-> [(a, b)] by ascending a, then ascending b"""
    lo, hi = min_sub or 1, max_sub or nsub
    return [(a, b) for a in range(nsub) for b in range(a + 1, nsub + 1) if lo <= b - a <= hi]


def clipped(x, clip, integer=True):
    """rows after the clip, their row sums S over the full band, the number of clipped rows (post_oracle.dedisperse's steps)"""
    x = np.asarray(x, dtype=np.float64)
    nrows = x.shape[0]
    S = po.seq_sum(x, 1)
    nclip = 0
    if clip > 0:
        flag = po.clip_flags(S, clip)
        nclip = int(flag.sum())
        if 0 < nclip < nrows:
            xg = np.where(flag[:, None], 0.0, x)
            part = [po.seq_sum(xg[r0:r0 + po.CHUNK_ROWS], 0) for r0 in range(0, nrows, po.CHUNK_ROWS)]
            repl = po.clip_replacement(po.seq_sum(np.stack(part), 0), float(nrows - nclip), integer)
            x = np.where(flag[:, None], repl[None, :], x)
            S = po.seq_sum(x, 1)
        else:
            nclip = 0
    return x, S, nclip


def dedisperse_bands(x, *, fch1, foff, tsamp, dms, nsub, min_sub=0, max_sub=0, zerodm=True, clip=5.0, integer=True):
    """x: [nrows][nchan] samples of one product -> (float32 [ndm * nband][nout], clipped rows, [(a, b)]).  Band [a, b) is summed
    in double from its own first channel upwards; the delays are those of the FULL band."""
    x, S, nclip = clipped(x, clip, integer)
    nrows, nchan = x.shape
    assert nchan % nsub == 0
    cps = nchan // nsub
    bands = band_list(nsub, min_sub, max_sub)
    dl = [po.delays_samples(fch1, foff, nchan, tsamp, dm) for dm in dms]
    nout = nrows - max(int(d.max()) for d in dl)
    out = np.empty((len(dl) * len(bands), nout), dtype=np.float32)
    for i, d in enumerate(dl):
        for j, (a, b) in enumerate(bands):
            s = np.zeros(nout)
            z = np.zeros(nout)
            for c in range(a * cps, b * cps):
                s += x[d[c]: d[c] + nout, c]
                if zerodm:
                    z += S[d[c]: d[c] + nout]
            out[i * len(bands) + j] = (s - z / nchan if zerodm else s).astype(np.float32)
    return out, nclip, bands


def search(plane, bands, widths, threshold, detrend_len=0):
    """spsearch_oracle.search on every series of the plane -> SPB_CAND records sorted by (dm_index, sub_lo, sub_hi, sample, width)"""
    got = so.search(plane, widths, threshold, detrend_len)
    out = np.zeros(got.size, dtype=SPB_CAND)
    nband = len(bands)
    ab = np.array(bands, dtype=np.int64).reshape(-1, 2)
    for k in ("width", "sample", "sigma"):
        out[k] = got[k]
    out["dm_index"] = got["dm_index"] // nband
    out["sub_lo"] = ab[got["dm_index"] % nband, 0]
    out["sub_hi"] = ab[got["dm_index"] % nband, 1]
    return out[np.lexsort((out["width"], out["sample"], out["sub_hi"], out["sub_lo"], out["dm_index"]))]


def full_band(recs, nsub):
    """the records of band [0, nsub) as spsearch_oracle.CAND records"""
    r = recs[(recs["sub_lo"] == 0) & (recs["sub_hi"] == nsub)]
    out = np.zeros(r.size, dtype=so.CAND)
    for k in ("dm_index", "width", "sample", "sigma"):
        out[k] = r[k]
    return out


def group(recs, nsub, *, fch1, foff, nchan, tsamp, dms, dm_gap=2):
    """the link rule of frbch_sp_group_cands on (dm_index, sample, width) -- the band plays no part -- and the summary of every
    connected component -> SPB_GROUP sorted by best's (dm_index, sample, width, sub_lo, sub_hi)"""
    n = recs.size
    D = [int(po.delays_samples(fch1, foff, nchan, tsamp, dm).max()) for dm in dms]
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            i = parent[i]
        return i

    for i in range(n):
        for j in range(i + 1, n):
            a, b = recs[i], recs[j]
            if abs(int(a["dm_index"]) - int(b["dm_index"])) > dm_gap:
                continue
            tol = max(int(a["width"]), int(b["width"])) // 2 + abs(D[a["dm_index"]] - D[b["dm_index"]])
            if abs(int(a["sample"]) - int(b["sample"])) <= tol:
                ri, rj = find(i), find(j)
                parent[max(ri, rj)] = min(ri, rj)
    out = []
    for r in sorted({find(i) for i in range(n)}):
        m = recs[[i for i in range(n) if find(i) == r]]
        key = sorted(range(m.size), key=lambda k: (-float(m[k]["sigma"]), int(m[k]["sub_hi"]) - int(m[k]["sub_lo"]), int(m[k]["width"]),
                                                   int(m[k]["dm_index"]), int(m[k]["sample"]), int(m[k]["sub_lo"])))
        g = np.zeros((), dtype=SPB_GROUP)
        g["best"] = m[key[0]]
        g["nmember"] = m.size
        g["dm_index_lo"], g["dm_index_hi"] = m["dm_index"].min(), m["dm_index"].max()
        g["sub_lo_min"], g["sub_hi_max"] = m["sub_lo"].min(), m["sub_hi"].max()
        g["sample_lo"], g["sample_hi"] = m["sample"].min(), m["sample"].max()
        full = m[(m["sub_lo"] == 0) & (m["sub_hi"] == nsub)]
        g["full_sigma"] = full["sigma"].max() if full.size else 0.0
        out.append(g)
    out = np.array(out, dtype=SPB_GROUP) if out else np.zeros(0, dtype=SPB_GROUP)
    b = out["best"]
    return out[np.lexsort((out["sample_lo"], b["sub_hi"], b["sub_lo"], b["width"], b["sample"], b["dm_index"]))]
