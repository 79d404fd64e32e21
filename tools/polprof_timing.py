#!/usr/bin/env python3
"""Time of the polarisation profile on the GPU box, for profiles/polprof_timing.json.

Shape: 8 bursts x 1024 channels x 4 products x 8 bit x 256 bins x tfactor 4, 32768 rows (128 MiB), 1.2 - 1.5 GHz, DMs 50 .. 400
(delay spreads of up to 141 rows per 64-channel tile), RMs -1400 .. +1400, two off-pulse windows of 1024 rows.  Timed in one
run, alternating, `--calls` host-synchronous calls each after one warm-up call, medians and spread on the host's clock (a call
includes the burst sums, its small uploads and downloads and the host's part: delays, records, derivation):

* `polprof_device` on the rows as the device allocator aligns them (the fast kernels) and on the same rows 4 bytes further on
  (the generic kernels of both the burst sums and the profile);
* `polprof_host`: the same with the upload of the rows;
* once, tests/polprof_oracle.profile_fp64 in numpy on the host.

The outputs of the two forms are compared byte for byte.  Kernel times come from a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/polprof_timing.py --calls 3 --no-fp64
    python tools/polprof_timing.py --kernel-stats DIR --out profiles/polprof_timing.json

Nothing is required of the ratios: the file says which form was faster, and DESIGN.md section 10 says what follows from it."""
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
NCHAN, NROWS, NCAND, NBIN, TFACTOR = 1024, 32768, 8, 256, 4


def spread(v):
    return dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3), calls=len(v))


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def kernel_stats(directory):
    """average microseconds and calls per kernel of the profile and the burst sums from rocprofv3's kernel_stats.csv"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Name"].split("(")[0]
            if "polprof" in name or "burst_sums" in name:
                out[name] = dict(calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1e3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--no-fp64", action="store_true", help="leave the numpy evaluation out (the run under the profiler)")
    ap.add_argument("--kernel-stats", default=None, help="directory of a run under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    import numpy as np
    from frb_baseband_amd import _lib, post
    lib, h = _lib.load(), hip()
    held = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert h.hipMalloc(C.byref(p), nbytes) == 0, "hipMalloc of %d bytes" % nbytes
        held.append(p.value)
        return p.value

    hdr = dict(nchans=NCHAN, nifs=4, nbits=8, fch1=1500.0 - 150.0 / NCHAN, foff=-300.0 / NCHAN, tsamp=256e-6, tstart=59000.0)
    rng = np.random.default_rng(12)
    rows = rng.integers(90, 111, size=(NROWS, 4, NCHAN), dtype=np.uint8)
    l2 = post.lambda2(hdr)
    bursts, rms = [], []
    for i in range(NCAND):
        dm, sample, rm = 50.0 * (i + 1), 6000 + 2500 * i, -1400.0 + 400.0 * i
        d = np.rint(dm * post.DM_CONST * ((hdr["fch1"] + np.arange(NCHAN) * hdr["foff"]) ** -2.0 - hdr["fch1"] ** -2.0) / hdr["tsamp"]).astype(np.int64)
        amp = [40.0 * np.ones(NCHAN), 30.0 * np.cos(2.0 * rm * l2), 30.0 * np.sin(2.0 * rm * l2), 5.0 * np.ones(NCHAN)]
        for t in range(sample - 8, sample + 8):
            r = t + d
            for p in range(4):
                rows[r, p, np.arange(NCHAN)] += np.rint(amp[p]).astype(np.int64).astype(np.uint8)
        bursts.append((dm, sample, 16))
        rms.append(rm)
    cands = post.burst_cands(bursts, 64, 1024)
    rm = np.array(rms)
    d_rows = alloc(rows.nbytes + 16)
    assert h.hipMemcpy(d_rows, rows.ctypes.data, rows.nbytes, 1) == 0
    d_rows4 = alloc(rows.nbytes + 16)
    assert h.hipMemcpy(d_rows4 + 4, rows.ctypes.data, rows.nbytes, 1) == 0
    desc = post.fil_desc(hdr)
    bpar = _lib.FrbchBurstParams(C.sizeof(_lib.FrbchBurstParams), _lib.BURST_STOKES)
    ppar = post.prof_params(NBIN, TFACTOR, "mean")
    err = C.create_string_buffer(512)

    def call(fn, ptr):
        acc, hits = np.zeros((NCAND, NBIN, 4), np.int64), np.zeros((NCAND, NBIN), np.uint32)
        bins, res = np.zeros((NCAND, NBIN), dtype=post.PROF_BIN), np.zeros(NCAND, dtype=post.PROF_RESULT)
        k = (C.c_uint32 * 2)(9, 9)
        t0 = time.perf_counter()
        rc = fn(C.byref(desc), C.c_void_p(ptr), NROWS, C.byref(bpar), cands.ctypes.data, NCAND, rm.ctypes.data, None, None, C.byref(ppar), 0,
                acc.ctypes.data, hits.ctypes.data, bins.ctypes.data, res.ctypes.data, None, k, err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        return dt, (k[0], k[1]), (acc, hits, bins, res)

    runs = {"polprof_device_fast": lambda: call(lib.frbch_polprof_device, d_rows), "polprof_device_generic": lambda: call(lib.frbch_polprof_device, d_rows4 + 4),
            "polprof_host": lambda: call(lib.frbch_polprof_host, rows.ctypes.data)}
    times = {name: [] for name in runs}
    kernels, last = {}, {}
    for name, fn in runs.items():                    # warm-up
        _dt, kernels[name], last[name] = fn()
    for _ in range(a.calls):
        for name, fn in runs.items():
            dt, _k, _o = fn()
            times[name].append(dt)
    assert kernels["polprof_device_generic"] == (0, 0), kernels
    same = all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(last["polprof_device_fast"], last["polprof_device_generic"], last["polprof_host"]))
    bins = last["polprof_device_fast"][2]
    out = dict(shape=dict(nchan=NCHAN, nrows=NROWS, nifs=4, nbits=8, ncand=NCAND, nbin=NBIN, tfactor=TFACTOR, width=16, off_len=1024,
                          dms=[b[0] for b in bursts], samples_per_call=NCAND * NCHAN * NBIN * TFACTOR * 4),
               kernel_used={k: list(v) for k, v in kernels.items()}, ms={name: spread(v) for name, v in times.items()},
               outputs_equal=dict(fast_vs_generic_vs_host=same),
               pa_deg_at_the_peak=[round(float(np.degrees(bins["pa"][i, NBIN // 2])), 2) for i in range(NCAND)],
               l_over_i_at_the_peak=[round(float(bins["l_db"][i, NBIN // 2] / bins["i"][i, NBIN // 2]), 3) for i in range(NCAND)])
    if not a.no_fp64:
        from tests import polprof_oracle as ppo
        t0 = time.perf_counter()
        fp = ppo.profile_fp64(rows, hdr, cands, rm, NBIN, TFACTOR, "mean")
        out["numpy_profile_fp64_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        out["largest_abs_q_minus_fp64"] = float(np.abs(bins["q"] - fp["Q"]).max())
    if a.kernel_stats:
        out["kernels"] = kernel_stats(a.kernel_stats)
        out["kernels_how"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/polprof_timing.py --calls 3 --no-fp64, a run of its own (same shape)"
    out["how"] = "python tools/polprof_timing.py --calls %d: host clock around host-synchronous calls, alternating, one warm-up each" % a.calls
    for p in held:
        h.hipFree(p)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    raise SystemExit(main())
