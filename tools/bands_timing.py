#!/usr/bin/env python3
"""Time of the band-limited dedispersion and search on the GPU box, for profiles/bands_timing.json.

Shape: 10 s x 1024 channels x 1 product x 8 bit at 100 us (100 000 rows, 98 MiB), 1.2 - 1.5 GHz, 64 DMs 300 .. 363, nsub 8
(36 bands): a plane of 2304 series.  Timed in one run, alternating, `--calls` host-synchronous calls each after one warm-up
call, medians and spread on the host's clock:

* (a) `dedisperse_bands_device` on the rows as the device allocator aligns them (the tiled prefix kernel + the range kernel)
  and (b) on the same rows 4 bytes further on (the generic kernel);
* (c) `dedisperse_device` on the same rows and DMs, the yardstick: it reads the same bytes and writes 1 / 36 of them;
* (d) the whole `bandsearch_device` call at threshold 7 with its own split into pre-pass, dedispersion and search (the
  search's figure includes the download of its raw peaks);
* once, tests/bands_oracle.dedisperse_bands in numpy on the host for ONE DM (a 64th of the work).

The planes of (a) and (b) are compared byte for byte.  Kernel times come from a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bands_timing.py --calls 3 --no-numpy
    python tools/bands_timing.py --kernel-stats DIR --out profiles/bands_timing.json

What must hold is the project's standing rule: the plan rule sends a shape to the tiled form only where (a) is below (b) in this
file; the exit status says whether it is."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
NCHAN, NROWS, NDM, NSUB, TSAMP = 1024, 100000, 64, 8, 100e-6


def spread(v):
    return dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3), calls=len(v))


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def kernel_stats(directory):
    """average microseconds and calls per kernel of the dedispersion and the search from rocprofv3's kernel_stats.csv"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Name"].split("(")[0]
            if "dedisp" in name or "bands" in name or "post_sp_" in name or "rowsum" in name:
                out[name] = dict(calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1e3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--no-numpy", action="store_true", help="leave the numpy evaluation out (the run under the profiler)")
    ap.add_argument("--kernel-stats", default=None, help="directory of a run under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    import numpy as np
    from frb_baseband_amd import _lib, post
    from oracle import post_oracle as po
    from tests import bands_oracle as bo
    lib, h = _lib.load(), hip()
    held = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert h.hipMalloc(C.byref(p), nbytes) == 0, "hipMalloc of %d bytes" % nbytes
        held.append(p.value)
        return p.value

    hdr = dict(nchans=NCHAN, nifs=1, nbits=8, fch1=1500.0 - 150.0 / NCHAN, foff=-300.0 / NCHAN, tsamp=TSAMP, tstart=59000.0)
    dms = [300.0 + i for i in range(NDM)]
    rng = np.random.default_rng(12)
    rows = np.clip(np.rint(rng.normal(96.0, 12.0, size=(NROWS, 1, NCHAN))), 0, 255).astype(np.uint8)
    dly = po.delays_samples(hdr["fch1"], hdr["foff"], NCHAN, TSAMP, 330.0)
    for ch in range(256, 512):                                  # a 4-row burst in sub-bands 2 and 3 of 8 at DM 330
        rows[30000 + dly[ch]: 30004 + dly[ch], 0, ch] += 6
    desc = post.fil_desc(hdr)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    nout = lib.frbch_dedisperse_nout(C.byref(desc), NROWS, dm_arr.ctypes.data, NDM)
    bp, sp = post.band_params(NSUB), post.sp_params(post.default_widths(TSAMP), 7.0, 1000)
    nband = post.band_list(NCHAN, NSUB, lib=lib).shape[0]
    d_rows = alloc(rows.nbytes + 16)
    assert h.hipMemcpy(d_rows, rows.ctypes.data, rows.nbytes, 1) == 0
    d_rows4 = alloc(rows.nbytes + 16)
    assert h.hipMemcpy(d_rows4 + 4, rows.ctypes.data, rows.nbytes, 1) == 0
    d_plane, d_series = alloc(NDM * nband * nout * 4), alloc(NDM * nout * 4)
    err = C.create_string_buffer(512)

    def bands(ptr):
        used = C.c_uint32(9)
        t0 = time.perf_counter()
        rc = lib.frbch_dedisperse_bands_device(C.byref(desc), C.c_void_p(ptr), NROWS, dm_arr.ctypes.data, NDM, 1, 5.0, C.byref(bp), 0,
                                               C.c_void_p(d_plane), nout, None, C.byref(used), err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        return dt, used.value

    def plain():
        t0 = time.perf_counter()
        rc = lib.frbch_dedisperse_device(C.byref(desc), C.c_void_p(d_rows), NROWS, dm_arr.ctypes.data, NDM, 1, 5.0, 0, C.c_void_p(d_series), nout,
                                         None, err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        return dt, lib.frbch_dedisperse_kernel(C.byref(desc), C.c_void_p(d_rows), NROWS, dm_arr.ctypes.data, NDM)

    split = []

    def search():
        cands = np.zeros(1 << 16, dtype=post.SPB_CAND)
        ncand, nb = C.c_uint64(0), C.c_uint32(0)
        used, ms = (C.c_uint32 * 2)(9, 9), (C.c_double * 3)()
        t0 = time.perf_counter()
        rc = lib.frbch_bandsearch_device(C.byref(desc), C.c_void_p(d_rows), NROWS, dm_arr.ctypes.data, NDM, 1, 5.0, C.byref(bp), C.byref(sp), 0,
                                         0, nout, None, cands.ctypes.data, cands.size, C.byref(ncand), used, C.byref(nb), ms, err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        split.append((ms[0], ms[1], ms[2], nb.value, ncand.value))
        return dt, (used[0], used[1])

    def plane_bytes():
        out = np.empty(NDM * nband * nout, dtype=np.float32)
        assert h.hipMemcpy(out.ctypes.data, d_plane, out.nbytes, 2) == 0
        return out

    runs = {"a_bands_tiled": lambda: bands(d_rows), "b_bands_generic": lambda: bands(d_rows4 + 4), "c_dedisperse_device": plain,
            "d_bandsearch_device": search}
    times = {name: [] for name in runs}
    kernels, planes = {}, {}
    for name, fn in runs.items():                    # warm-up
        _dt, kernels[name] = fn()
        if name[0] in "ab":
            planes[name] = plane_bytes()
    split.clear()
    for _ in range(a.calls):
        for name, fn in runs.items():
            times[name].append(fn()[0])
    assert kernels["b_bands_generic"] == 0, kernels
    same = planes["a_bands_tiled"].tobytes() == planes["b_bands_generic"].tobytes()
    ms = {name: spread(v) for name, v in times.items()}
    out = dict(shape=dict(nchan=NCHAN, nrows=NROWS, nifs=1, nbits=8, tsamp=TSAMP, ndm=NDM, dms=[dms[0], dms[-1]], nsub=NSUB, nband=nband, nout=nout,
                          rows_bytes=rows.nbytes, plane_bytes=NDM * nband * nout * 4, series_bytes=NDM * nout * 4),
               kernel_used={k: list(v) if isinstance(v, tuple) else v for k, v in kernels.items()}, ms=ms, outputs_equal=dict(tiled_vs_generic=same),
               tiled_is_faster=ms["a_bands_tiled"]["median_ms"] < ms["b_bands_generic"]["median_ms"],
               a_over_c=round(ms["a_bands_tiled"]["median_ms"] / ms["c_dedisperse_device"]["median_ms"], 2), bytes_written_a_over_c=nband,
               bandsearch_split_ms=dict(prepass=round(statistics.median(s[0] for s in split), 3), dedisperse=round(statistics.median(s[1] for s in split), 3),
                                        search_with_download=round(statistics.median(s[2] for s in split), 3), nbatch=split[0][3], records=split[0][4]))
    if not a.no_numpy:
        t0 = time.perf_counter()
        w, _n, _b = bo.dedisperse_bands(rows[: nout + int(po.delays_samples(hdr["fch1"], hdr["foff"], NCHAN, TSAMP, dms[0]).max()), 0, :],
                                        fch1=hdr["fch1"], foff=hdr["foff"], tsamp=TSAMP, dms=dms[:1], nsub=NSUB, zerodm=False, clip=0.0)
        out["numpy_one_dm_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    if a.kernel_stats:
        out["kernels"] = kernel_stats(a.kernel_stats)
        out["kernels_how"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bands_timing.py --calls 3 --no-numpy, a run of its own (same shape)"
    out["how"] = "python tools/bands_timing.py --calls %d: host clock around host-synchronous calls, alternating, one warm-up each" % a.calls
    for p in held:
        h.hipFree(p)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same and out["tiled_is_faster"] else 1


if __name__ == "__main__":
    raise SystemExit(main())
