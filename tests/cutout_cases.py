"""Shared cases of the candidate cut-out tests (tests/test_cutout.py on the emulator, tests/test_gpu_cutout.py on the device):
named cases -- rows, header, product, plane shape, candidates -- thin callers of the C ABI, and the kernel's tile constants.
Expected planes are tests/cutout_oracle.py on the same rows, computed once per case and never written to."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import _lib, post
from tests import cutout_oracle as co
from tests import post_cases as pc

TILE = 256                      # rows (time samples) a workgroup of the LDS kernel owns: 256 // tfactor whole bins
NR = 8                          # plane rows (trial DMs / frequency bins) of a workgroup
ROWS_CAP = 900                  # rows of one (row group, channel tile, time tile) the LDS holds
LDS, GENERIC = 1, 0


def cands_of(*items):
    """(dm, sample, tfactor[, dm_lo, dm_hi]) ... -> CUT_CAND records; the DM-time plane defaults to 0 .. 2 dm"""
    out = np.zeros(len(items), dtype=post.CUT_CAND)
    for o, it in zip(out, items):
        dm, sample, f = it[:3]
        o["dm"], o["sample"], o["tfactor"] = dm, sample, f
        o["dm_lo"], o["dm_hi"] = (it[3], it[4]) if len(it) > 3 else (0.0, 2.0 * dm)
    return out


def _case(nchan, nbits, nrows, nt, nf, ndm, cands, nifs=1, prod=0, foff_sign=-1, seed=41):
    hdr = pc.make_hdr(nchan, foff_sign)
    rows = pc.make_rows(nrows, nifs, nchan, nbits, seed=seed, hdr=hdr)
    return dict(hdr=dict(hdr, nifs=nifs, nbits=nbits), rows=rows, prod=prod, nt=nt, nf=nf, ndm=ndm, cands=cands_of(*cands))


MIXED5 = [(56.7, 3500, 1), (20.0, 2000, 2, 5.0, 60.0), (90.5, 4100, 3), (56.7, 3600, 7), (33.3, 3500, 150, 10.0, 40.0)]

# ---- the grid of the CPU suite (generic kernel there; the device takes the LDS kernel where the layout allows) ------------
CASES = {
    "c64_b8_nf16_nt16_ndm8": lambda: _case(64, 8, 6000, 16, 16, 8, [(56.7, 3000, 1)]),
    "c48_b16_nf48_nt32_ndm9_batch5": lambda: _case(48, 16, 7000, 32, 48, 9, MIXED5),
    "c128_b32_nf1_nt16_ndm13": lambda: _case(128, 32, 6000, 16, 1, 13, [(56.7, 3000, 1), (40.0, 2500, 3, 30.0, 50.0), (12.0, 900, 7)]),
    "c64_b8_nf64_nt2_ndm1": lambda: _case(64, 8, 6000, 2, 64, 1, [(56.7, 3000, 7)]),
    "c128_b16_nf16_nt32_ndm13_batch5": lambda: _case(128, 16, 9000, 32, 16, 13, MIXED5),
    "c64_b8_tfactor512_nt4": lambda: _case(64, 8, 9000, 4, 16, 8, [(56.7, 4000, 512), (56.7, 4000, 150)]),
    "c64_b16_foff_positive": lambda: _case(64, 16, 6000, 16, 16, 9, [(56.7, 3000, 2), (80.0, 3100, 3)], foff_sign=+1),
    "c64_b8_nifs3_product2": lambda: _case(64, 8, 6000, 16, 16, 8, [(56.7, 3000, 1), (56.7, 2610, 2)], nifs=3, prod=2),
    "c64_b8_starts_before_row0": lambda: _case(64, 8, 6000, 32, 16, 8, [(56.7, 5, 3), (56.7, 40, 7)]),
    "c64_b8_ends_past_nrows": lambda: _case(64, 8, 6000, 32, 16, 8, [(56.7, 5990, 3), (56.7, 5800, 7)]),
    "c64_b8_wholly_outside": lambda: _case(64, 8, 6000, 16, 16, 8, [(56.7, 6000 + 100000, 3), (56.7, -100000, 2)]),
    "c64_b8_dm_hi_delay_past_nrows": lambda: _case(64, 8, 6000, 16, 16, 9, [(56.7, 3000, 2, 0.0, 3000.0)]),
    "c128_b32_batch5": lambda: _case(128, 32, 6000, 2, 128, 8, MIXED5[:4]),
}

# ---- shapes that reach the LDS kernel's own paths (device only) -----------------------------------------------------------
# nt is even, so nt * tfactor is even too: the nearest products on both sides of TILE and of 3 TILE + 5 stand in for the odd ones;
# f = 127 / 128 / 129 and 255 / 256 / 257: two bins, one bin and a bin longer than the tile (walked in chunks of TILE rows)
EDGE_F = [(2, 127), (2, 128), (2, 129), (256, 1), (258, 1), (86, 3), (4, 193), (18, 43), (2, 255), (2, 256), (2, 257), (4, 300)]


def _edge(nt, f):
    return lambda: _case(64, 8, 9000, nt, 16, 9, [(56.7, 4500, f), (30.0, 300, f), (56.7, 8900, f)])


DEVICE_CASES = {
    "c1024_b8_nf256": lambda: _case(1024, 8, 6000, 32, 256, 9, MIXED5[:4]),
    "c1024_b8_nf16": lambda: _case(1024, 8, 6000, 32, 16, 9, MIXED5[:4]),
    "c1024_b8_nf8": lambda: _case(1024, 8, 6000, 32, 8, 13, MIXED5[:4]),
    "c1024_b8_nf1": lambda: _case(1024, 8, 6000, 32, 1, 8, MIXED5[:4]),
    "c512_b16_nf64": lambda: _case(512, 16, 6000, 32, 64, 13, MIXED5),
    "c192_b8_nf2_bins_across_tiles": lambda: _case(192, 8, 6000, 16, 2, 9, MIXED5[:3]),
    "c64_b8_nt256_ndm256": lambda: _case(64, 8, 9000, 256, 64, 256, [(56.7, 4000, 2)]),
    "c64_b8_batch33": lambda: _case(64, 8, 9000, 16, 16, 9, [(20.0 + 2.5 * i, 500 + 250 * i, 1 + (7 * i) % 30) for i in range(33)]),
    "c64_b8_ndm8_dm_hi_3000_spans_more_than_the_lds": lambda: _case(64, 8, 6000, 16, 16, 8, [(56.7, 3000, 2, 0.0, 3000.0), (56.7, 2000, 1)]),
    "c1024_b8_nifs2_product1": lambda: _case(1024, 8, 6000, 16, 16, 9, MIXED5[:2], nifs=2, prod=1),
}
DEVICE_CASES.update({"edge_nt%d_f%d" % (nt, f): _edge(nt, f) for nt, f in EDGE_F})


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (case dict, (ft, ft_hits, dt, dt_hits) of the restatement); built once, never written to"""
    cs = (CASES.get(name) or DEVICE_CASES[name])()
    cs["rows"].setflags(write=False)
    want = co.planes_batch(cs["rows"][:, cs["prod"], :], cs["hdr"], cs["cands"], cs["nt"], cs["nf"], cs["ndm"])
    for w in want:
        w.setflags(write=False)
    return cs, want


def params(nt, nf, ndm):
    return _lib.FrbchCutoutParams(C.sizeof(_lib.FrbchCutoutParams), nt, nf, ndm)


def desc_of(cs):
    return post.fil_desc(cs["hdr"], product=cs["prod"])


def cutout_kernel(lib, cs, address):
    """frbch_cutout_kernel for the rows at `address` (only the address is examined)"""
    par = params(cs["nt"], cs["nf"], cs["ndm"])
    cands = np.ascontiguousarray(cs["cands"])
    return lib.frbch_cutout_kernel(C.byref(desc_of(cs)), C.c_void_p(address), cs["rows"].shape[0], C.byref(par), cands.ctypes.data,
                                   cands.size)


def empty_planes(cs):
    n = cs["cands"].size
    return (np.full((n, cs["nf"], cs["nt"]), -1.0, np.float32), np.full((n, cs["nf"], cs["nt"]), 0xFFFFFFFF, np.uint32),
            np.full((n, cs["ndm"], cs["nt"]), -1.0, np.float32), np.full((n, cs["ndm"], cs["nt"]), 0xFFFFFFFF, np.uint32))


def cutout_host(lib, cs):
    """frbch_cutout_host -> (rc, (ft, ft_hits, dt, dt_hits), kernel_used, message)"""
    par = params(cs["nt"], cs["nf"], cs["ndm"])
    cands = np.ascontiguousarray(cs["cands"])
    rows = cs["rows"]
    out = empty_planes(cs)
    used = C.c_uint32(99)
    err = C.create_string_buffer(512)
    rc = lib.frbch_cutout_host(C.byref(desc_of(cs)), rows.ctypes.data, rows.shape[0], C.byref(par), cands.ctypes.data, cands.size, 0,
                               out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, C.byref(used), err,
                               len(err))
    return rc, out, used.value, err.value.decode()


def same_planes(got, want):
    """every plane to the bit"""
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def which_differ(got, want):
    return [name for name, g, w in zip(("ft", "ft_hits", "dt", "dt_hits"), got, want) if g.tobytes() != w.tobytes()]


def lds_expected(cs):
    """the documented selection rule restated: integer rows, whole 64-byte channel tiles (hipMalloc'ed rows are aligned), and
    every (group of NR plane rows, channel tile) of both planes spans at most ROWS_CAP - TILE rows"""
    hdr, nbits, nchan = cs["hdr"], cs["hdr"]["nbits"], cs["hdr"]["nchans"]
    if nbits == 32 or (nchan * nbits // 8) % 64 or (cs["hdr"]["nifs"] * nchan * nbits // 8) % 16:
        return GENERIC
    ct, cpb = 64 * 8 // nbits, nchan // cs["nf"]
    for c in cs["cands"]:
        d = np.stack([co.delays(hdr, dm) for dm in co.trial_dms(c["dm_lo"], c["dm_hi"], cs["ndm"])])
        for g in range(0, cs["ndm"], NR):
            for k in range(0, nchan, ct):
                if int(d[g:g + NR, k:k + ct].max() - d[g:g + NR, k:k + ct].min()) + TILE > ROWS_CAP:
                    return GENERIC
        d = co.delays(hdr, float(c["dm"]))
        for g in range(0, cs["nf"], NR):
            lo, hi = g * cpb, min(nchan, (g + NR) * cpb)
            for k in range(lo // ct, (hi - 1) // ct + 1):
                part = d[max(lo, k * ct):min(hi, (k + 1) * ct)]
                if int(part.max() - part.min()) + TILE > ROWS_CAP:
                    return GENERIC
    return LDS


# ---- the timing shape: 10 s x 1024 channels of 8-bit rows in HBM, 32 candidates, nt = ndm = 256 ---------------------------
TIMING_HDR = dict(nchans=1024, nifs=1, nbits=8, fch1=1416.0 - 0.015625, foff=-0.03125, tsamp=32e-6, tstart=59000.0)
TIMING_ROWS, TIMING_NT, TIMING_NDM, TIMING_NF = 312500, 256, 256, 256


def timing_cands():
    """32 candidates well inside the data: widths round-robin from the default list (tfactor 1 .. 15), DMs 300 .. 331"""
    widths = post.default_widths(TIMING_HDR["tsamp"])
    r = np.zeros(32, dtype=post.SP_CAND)
    r["dm_index"], r["sample"] = np.arange(32), 20000 + 9000 * np.arange(32)
    r["width"] = [widths[i % len(widths)] for i in range(32)]
    return post.cutout_cands(r, [300.0 + i for i in range(32)])


def timing_run(lib, rows_ptr, rounds=5):
    """median of `rounds` frbch_cutout_device calls for all 32 candidates against the median of `rounds` rounds of 32
    frbch_dedisperse_device calls, one per candidate on its row window with the same 256 DMs (no time binning, no
    frequency-time plane); one warm-up of each side first.  rows_ptr: device address of the TIMING_ROWS x 1024 rows."""
    import statistics
    import time
    from tests.hipmem import GuardedBuffer as DeviceBuffer
    cands = timing_cands()
    n, nt, ndm, nf, nchan = cands.size, TIMING_NT, TIMING_NDM, TIMING_NF, TIMING_HDR["nchans"]
    desc = post.fil_desc(TIMING_HDR)
    par = params(nt, nf, ndm)
    err = C.create_string_buffer(512)
    used, nclip = C.c_uint32(9), C.c_uint64(0)
    bufs = [DeviceBuffer(n * rows * nt * 4) for rows in (nf, nf, ndm, ndm)]
    assert lib.frbch_cutout_kernel(C.byref(desc), C.c_void_p(rows_ptr), TIMING_ROWS, C.byref(par), cands.ctypes.data, n) == LDS

    def cutout():
        t0 = time.perf_counter()
        rc = lib.frbch_cutout_device(C.byref(desc), C.c_void_p(rows_ptr), TIMING_ROWS, C.byref(par), cands.ctypes.data, n, 0, bufs[0].ptr,
                                     bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, C.byref(used), err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        return dt

    windows = []
    for c in cands:
        f = int(c["tfactor"])
        t0 = int(c["sample"]) - (nt // 2) * f
        dms = np.ascontiguousarray(co.trial_dms(c["dm_lo"], c["dm_hi"], ndm), dtype=np.float64)
        nout = nt * f
        nrows = nout + int(co.delays(TIMING_HDR, float(dms[-1])).max())
        assert t0 >= 0 and t0 + nrows <= TIMING_ROWS
        ptr = rows_ptr + t0 * nchan
        assert lib.frbch_dedisperse_nout(C.byref(desc), nrows, dms.ctypes.data, ndm) == nout
        assert lib.frbch_dedisperse_kernel(C.byref(desc), C.c_void_p(ptr), nrows, dms.ctypes.data, ndm) == 1
        windows.append((ptr, nrows, dms, nout))
    d_out = DeviceBuffer(ndm * max(w[3] for w in windows) * 4)

    def composed():
        t0 = time.perf_counter()
        for ptr, nrows, dms, nout in windows:
            rc = lib.frbch_dedisperse_device(C.byref(desc), C.c_void_p(ptr), nrows, dms.ctypes.data, ndm, 0, 0.0, 0, d_out.ptr, nout,
                                             C.byref(nclip), err, len(err))
            assert rc == 0, err.value
        return time.perf_counter() - t0

    cutout()
    composed()
    t_cut = statistics.median(cutout() for _ in range(rounds))
    t_dd = statistics.median(composed() for _ in range(rounds))
    for b in bufs + [d_out]:            # (free() checks the buffer's guards)
        b.free()
    return {"rows": TIMING_ROWS, "nchan": nchan, "ncand": int(n), "nt": nt, "nf": nf, "ndm": ndm, "tfactor": cands["tfactor"].tolist(),
            "kernel_used": used.value, "cutout_device_median_s": t_cut, "dedisperse_device_x32_median_s": t_dd}
