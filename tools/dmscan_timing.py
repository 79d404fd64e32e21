#!/usr/bin/env python3
"""Time of the DM scan on the GPU box, for profiles/dmscan_timing.json.

Shape: 8 bursts x 1024 channels x 1 product x 8 bit, 257 trials x 256 bins x tfactor 4, 32768 rows (32 MiB), 1.2 - 1.5 GHz, DMs
50 .. 400, ddm a quarter of a DM sample step, two off-pulse windows of 1024 rows.  Timed in one run, alternating, `--calls`
host-synchronous calls each after one warm-up call, medians and spread on the host's clock (a call includes the burst sums, its
small uploads and downloads and the host's part: the delay table, the records, the peaks):

* `dmscan_device` on the rows as the device allocator aligns them (the fast kernels) and on the same rows 4 bytes further on
  (the generic kernels of both the burst sums and the scan);
* `dmscan_host`: the same with the upload of the rows;
* once, tests/dmscan_oracle.planes in numpy on the host, for the first burst alone (an eighth of the work).

The outputs of the two forms are compared byte for byte.  Kernel times come from a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/dmscan_timing.py --calls 3 --no-numpy
    python tools/dmscan_timing.py --kernel-stats DIR --out profiles/dmscan_timing.json

What must hold is the project's standing rule: the plan rule sends a shape to the fast kernel only where its kernel time, join
included, is below the generic kernel's of the same build; the exit status says whether it does here."""
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
NCHAN, NROWS, NCAND, NTRIAL, NBIN, TFACTOR = 1024, 32768, 8, 257, 256, 4


def spread(v):
    return dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3), calls=len(v))


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def kernel_stats(directory):
    """average microseconds and calls per kernel of the scan and the burst sums from rocprofv3's kernel_stats.csv"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Name"].split("(")[0]
            if "dmscan" in name or "burst_sums" in name:
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
    from tests import dmscan_oracle as do
    lib, h = _lib.load(), hip()
    held = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert h.hipMalloc(C.byref(p), nbytes) == 0, "hipMalloc of %d bytes" % nbytes
        held.append(p.value)
        return p.value

    hdr = dict(nchans=NCHAN, nifs=1, nbits=8, fch1=1500.0 - 150.0 / NCHAN, foff=-300.0 / NCHAN, tsamp=256e-6, tstart=59000.0, product=0)
    step = post.dm_sample_step(hdr, lib)
    ddm = step / 4.0
    rng = np.random.default_rng(12)
    rows = rng.integers(90, 111, size=(NROWS, 1, NCHAN), dtype=np.uint8)
    bursts = []
    for i in range(NCAND):
        dm, sample = 50.0 * (i + 1), 6000 + 2500 * i
        d = do.delays(hdr, dm + 3.3 * step)                     # the burst lies 3.3 steps above the DM the scan is centred on
        for t in range(sample - 2, sample + 2):
            rows[t + d, 0, np.arange(NCHAN)] += 12
        bursts.append((dm, sample, 4))
    cands = post.burst_cands(bursts, 64, 1024)
    d_rows = alloc(rows.nbytes + 16)
    assert h.hipMemcpy(d_rows, rows.ctypes.data, rows.nbytes, 1) == 0
    d_rows4 = alloc(rows.nbytes + 16)
    assert h.hipMemcpy(d_rows4 + 4, rows.ctypes.data, rows.nbytes, 1) == 0
    desc = post.fil_desc(hdr)
    bpar = _lib.FrbchBurstParams(C.sizeof(_lib.FrbchBurstParams), _lib.BURST_STOKES)
    par, pk = post.dmscan_params(NTRIAL, ddm, NBIN, TFACTOR), post.dmscan_peak_params((1, 2, 4, 8), 3, 0.5)
    err = C.create_string_buffer(512)

    def call(fn, ptr):
        acc, hits = np.zeros((NCAND, NTRIAL, NBIN), np.int64), np.zeros((NCAND, NTRIAL, NBIN), np.uint32)
        snr, strc, res = np.zeros((NCAND, NTRIAL)), np.zeros((NCAND, NTRIAL)), np.zeros(NCAND, dtype=post.DMSCAN_RESULT)
        k = (C.c_uint32 * 2)(9, 9)
        t0 = time.perf_counter()
        rc = fn(C.byref(desc), C.c_void_p(ptr), NROWS, C.byref(bpar), cands.ctypes.data, NCAND, None, C.byref(par), C.byref(pk), 0, acc.ctypes.data,
                hits.ctypes.data, snr.ctypes.data, strc.ctypes.data, res.ctypes.data, None, k, err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        return dt, (k[0], k[1]), (acc, hits, snr, strc, res)

    runs = {"dmscan_device_fast": lambda: call(lib.frbch_dmscan_device, d_rows), "dmscan_device_generic": lambda: call(lib.frbch_dmscan_device, d_rows4 + 4),
            "dmscan_host": lambda: call(lib.frbch_dmscan_host, rows.ctypes.data)}
    times = {name: [] for name in runs}
    kernels, last = {}, {}
    for name, fn in runs.items():                    # warm-up
        _dt, kernels[name], last[name] = fn()
    for _ in range(a.calls):
        for name, fn in runs.items():
            dt, _k, _o = fn()
            times[name].append(dt)
    assert kernels["dmscan_device_generic"] == (0, 0), kernels
    same = all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(last["dmscan_device_fast"], last["dmscan_device_generic"], last["dmscan_host"]))
    res = last["dmscan_device_fast"][4]
    out = dict(shape=dict(nchan=NCHAN, nrows=NROWS, nifs=1, nbits=8, ncand=NCAND, ntrial=NTRIAL, nbin=NBIN, tfactor=TFACTOR, width=4, off_len=1024,
                          dms=[b[0] for b in bursts], dm_sample_step=step, ddm=ddm, terms_per_call=NCAND * NCHAN * NTRIAL * NBIN),
               kernel_used={k: list(v) for k, v in kernels.items()}, ms={name: spread(v) for name, v in times.items()},
               outputs_equal=dict(fast_vs_generic_vs_host=same),
               dm_snr_minus_injected_steps=[round(float((res["dm_snr"][i] - bursts[i][0]) / step - 3.3), 3) for i in range(NCAND)],
               dm_struct_minus_injected_steps=[round(float((res["dm_struct"][i] - bursts[i][0]) / step - 3.3), 3) for i in range(NCAND)])
    if not a.no_numpy:
        t0 = time.perf_counter()
        w = do.planes(rows, hdr, cands[:1], NTRIAL, ddm, NBIN, TFACTOR)
        out["numpy_planes_of_one_burst_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        same = same and w["acc"].tobytes() == last["dmscan_device_fast"][0][:1].tobytes()
        out["outputs_equal"]["numpy_first_burst"] = w["acc"].tobytes() == last["dmscan_device_fast"][0][:1].tobytes()
    faster = None
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        out["kernels"] = ks
        out["kernels_how"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/dmscan_timing.py --calls 3 --no-numpy, a run of its own (same shape)"
        fast_us = sum(v["average_us"] for n, v in ks.items() if "dmscan_fast" in n or "dmscan_join" in n)
        gen_us = sum(v["average_us"] for n, v in ks.items() if n.endswith("frbch_post_dmscan"))
        if fast_us and gen_us:
            faster = fast_us < gen_us
            out["scan_kernel_us"] = dict(fast_with_join=round(fast_us, 2), generic=round(gen_us, 2), fast_is_faster=faster)
    out["how"] = "python tools/dmscan_timing.py --calls %d: host clock around host-synchronous calls, alternating, one warm-up each" % a.calls
    for p in held:
        h.hipFree(p)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same and faster is not False else 1


if __name__ == "__main__":
    raise SystemExit(main())
