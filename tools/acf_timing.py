#!/usr/bin/env python3
"""Time of the burst ACF on the GPU box, for profiles/acf_timing.json.

Shape: 8 bursts x 1024 channels (ffactor 1) x 1 product x 8 bit, 256 bins x tfactor 4, 128 x 255 lags, 32768 rows (32 MiB), 1.2 -
1.5 GHz, DMs 50 .. 400, two off-pulse windows of 1024 rows: 8 x 128 x 255 lags of 1024 x 256 cells, 6.8e10 multiply-adds less the
edges.  Timed in one run, alternating, `--calls` host-synchronous calls each after one warm-up call, medians and spread on the
host's clock (a call includes the burst sums, its small uploads and downloads and the host's part):

* `burstacf_device` on the rows as the device allocator aligns them (every kernel fast) and on the same rows 4 bytes further on
  (the generic burst sums and dynamic spectrum; the ACF runs on the library's own plane and stays fast);
* `burstacf_host`: the same with the upload of the rows;
* the ACF stage alone on the quantised planes of that call, `acf2d_device` as the plan rule has it (fast) and with
  FRBCH_ACF_GENERIC -- the composite has no switch for its ACF kernel, so this pair is the comparison of the two ACF kernels;
* once, tests/acf_oracle.acf2d in numpy on the host, for the first burst alone (an eighth of the work).

The outputs of all forms are compared byte for byte.  Kernel times come from a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/acf_timing.py --calls 3 --no-numpy
    python tools/acf_timing.py --kernel-stats DIR --out profiles/acf_timing.json

What must hold is the project's standing rule: the plan rule sends a shape to a fast kernel only where its kernel time, join
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
NCHAN, NROWS, NCAND, NBIN, TFACTOR, FFACTOR, NLAGF, NLAGT = 1024, 32768, 8, 256, 4, 1, 128, 128


def spread(v):
    return dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3), calls=len(v))


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def kernel_stats(directory):
    """average microseconds and calls per kernel of this stage and the burst sums from rocprofv3's kernel_stats.csv"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Name"].split("(")[0]
            if "acf" in name or "dynspec" in name or "burst_sums" in name:
                out[name] = dict(calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1e3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true", help="leave the numpy evaluation out (the run under the profiler)")
    ap.add_argument("--kernel-stats", default=None, help="directory of a run under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    import numpy as np
    from frb_baseband_amd import _lib, post
    from tests import acf_oracle as ao
    from tests import dmscan_oracle as do
    lib, h = _lib.load(), hip()
    held = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert h.hipMalloc(C.byref(p), nbytes) == 0, "hipMalloc of %d bytes" % nbytes
        held.append(p.value)
        return p.value

    hdr = dict(nchans=NCHAN, nifs=1, nbits=8, fch1=1500.0 - 150.0 / NCHAN, foff=-300.0 / NCHAN, tsamp=256e-6, tstart=59000.0, product=0)
    rng = np.random.default_rng(13)
    rows = rng.integers(90, 111, size=(NROWS, 1, NCHAN), dtype=np.uint8)
    bursts = []
    chans = np.arange(NCHAN)
    for i in range(NCAND):
        dm, sample = 50.0 * (i + 1), 6000 + 2500 * i
        d = do.delays(hdr, dm)
        for t in range(sample - 40, sample + 40):                # a burst that drifts: lower channels later by up to 60 rows
            rows[t + d + (60 * chans) // NCHAN, 0, chans] += 10
        bursts.append((dm, sample, 80))
    cands = post.burst_cands(bursts, 600, 1024)
    d_rows = alloc(rows.nbytes + 16)
    assert h.hipMemcpy(d_rows, rows.ctypes.data, rows.nbytes, 1) == 0
    d_rows4 = alloc(rows.nbytes + 16)
    assert h.hipMemcpy(d_rows4 + 4, rows.ctypes.data, rows.nbytes, 1) == 0
    desc = post.fil_desc(hdr)
    bpar = _lib.FrbchBurstParams(C.sizeof(_lib.FrbchBurstParams), _lib.BURST_STOKES)
    par, fp = post.acf_params(NBIN, TFACTOR, FFACTOR, NLAGF, NLAGT), post.acf_fit_params(0.5)
    nsub, ndt = NCHAN // FFACTOR, 2 * NLAGT - 1
    err = C.create_string_buffer(512)

    def call(fn, ptr):
        Y, yhits = np.zeros((NCAND, nsub, NBIN), np.int64), np.zeros((NCAND, nsub, NBIN), np.uint32)
        A, P, res = np.zeros((NCAND, NLAGF, ndt), np.int64), np.zeros((NCAND, NLAGF, ndt), np.uint32), np.zeros(NCAND, dtype=post.ACF_RESULT)
        k = (C.c_uint32 * 3)(9, 9, 9)
        t0 = time.perf_counter()
        rc = fn(C.byref(desc), C.c_void_p(ptr), NROWS, C.byref(bpar), cands.ctypes.data, NCAND, None, C.byref(par), C.byref(fp), 0, Y.ctypes.data,
                yhits.ctypes.data, A.ctypes.data, P.ctypes.data, res.ctypes.data, None, k, err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        return dt, (k[0], k[1], k[2]), (Y, yhits, A, P, res)

    # the planes of the ACF stage alone: the quantised planes of the composite, restated on the host from its Y and yhits
    _dt, _k, first = call(lib.frbch_burstacf_device, d_rows)
    mask = (first[1] == TFACTOR * FFACTOR).astype(np.uint8)        # (no flags, no dead channels: every used subband has ffactor channels)
    y, _r = ao.quantise(first[0], mask)
    d_y, d_A = alloc(y.nbytes), alloc(first[2].nbytes)
    assert h.hipMemcpy(d_y, y.ctypes.data, y.nbytes, 1) == 0

    def stage(form):
        k = C.c_uint32(9)
        t0 = time.perf_counter()
        rc = lib.frbch_acf2d_device(C.c_void_p(d_y), NCAND, nsub, NBIN, NLAGF, NLAGT, form, 0, C.c_void_p(d_A), C.byref(k), err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        A = np.zeros((NCAND, NLAGF, ndt), np.int64)
        assert h.hipMemcpy(A.ctypes.data, d_A, A.nbytes, 2) == 0
        return dt, (k.value,), (A,)

    runs = {"burstacf_device_fast": lambda: call(lib.frbch_burstacf_device, d_rows),
            "burstacf_device_generic_sums_and_spectrum": lambda: call(lib.frbch_burstacf_device, d_rows4 + 4),
            "burstacf_host": lambda: call(lib.frbch_burstacf_host, rows.ctypes.data),
            "acf2d_device_fast": lambda: stage(_lib.ACF_PLAN), "acf2d_device_generic": lambda: stage(_lib.ACF_GENERIC)}
    times = {name: [] for name in runs}
    kernels, last = {}, {}
    for name, fn in runs.items():                    # warm-up
        _dt, kernels[name], last[name] = fn()
    for _ in range(a.calls):
        for name, fn in runs.items():
            dt, _k, _o = fn()
            times[name].append(dt)
    assert kernels["burstacf_device_fast"] == (1, 1, 1) and kernels["burstacf_device_generic_sums_and_spectrum"] == (0, 0, 1), kernels
    assert kernels["acf2d_device_fast"] == (1,) and kernels["acf2d_device_generic"] == (0,), kernels
    ref = last["burstacf_device_fast"]
    same = all(x.tobytes() == yv.tobytes() == z.tobytes() for x, yv, z in zip(ref, last["burstacf_device_generic_sums_and_spectrum"], last["burstacf_host"]))
    same = same and ref[2].tobytes() == last["acf2d_device_fast"][0].tobytes() == last["acf2d_device_generic"][0].tobytes()
    res = ref[4]
    out = dict(shape=dict(nchan=NCHAN, nrows=NROWS, nifs=1, nbits=8, ncand=NCAND, nbin=NBIN, tfactor=TFACTOR, ffactor=FFACTOR, nlagf=NLAGF, nlagt=NLAGT,
                          dms=[b[0] for b in bursts], multiply_adds_per_call=NCAND * NLAGF * ndt * nsub * NBIN),
               kernel_used={k: list(v) for k, v in kernels.items()}, ms={name: spread(v) for name, v in times.items()},
               outputs_equal=dict(all_forms=same), r=[int(v) for v in res["r"]], drift_mhz_per_ms=[round(float(v), 3) for v in res["drift"]],
               width_t_ms=[round(float(v), 3) for v in res["width_t_ms"]])
    if not a.no_numpy:
        t0 = time.perf_counter()
        w = ao.acf2d(y[0], NLAGF, NLAGT)
        out["numpy_acf_of_one_burst_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        out["outputs_equal"]["numpy_first_burst"] = w.tobytes() == ref[2][0].tobytes()
        same = same and out["outputs_equal"]["numpy_first_burst"]
    faster = None
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        out["kernels"] = ks
        out["kernels_how"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/acf_timing.py --calls 3 --no-numpy, a run of its own (same shape)"
        fast_us = sum(v["average_us"] for n, v in ks.items() if "acf2d_fast" in n or "acf2d_join" in n)
        gen_us = sum(v["average_us"] for n, v in ks.items() if n.endswith("frbch_post_acf2d"))
        if fast_us and gen_us:
            faster = fast_us < gen_us
            out["acf_kernel_us"] = dict(fast_with_join=round(fast_us, 2), generic=round(gen_us, 2), fast_is_faster=faster)
            out["acf_fast_multiply_adds_per_s"] = round(NCAND * NLAGF * ndt * nsub * NBIN / (fast_us * 1e-6), -9)
    out["how"] = "python tools/acf_timing.py --calls %d: host clock around host-synchronous calls, alternating, one warm-up each" % a.calls
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
