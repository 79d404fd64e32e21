#!/usr/bin/env python3
"""Time of the acceleration search (frbch_pasearch_device) on the GPU box, for profiles/accel_timing.json.

Shape: 64 series of 2^18 noise samples (tsamp 64 us), 33 trial accelerations.  Timed in one run, alternating, `--calls`
host-synchronous calls each after one warm-up call, medians and spread on the host's clock:

* `pasearch_device`: one call for all trials, the series as the device allocator aligns them (the fast resampler), and the same
  series one float further on (the generic resampler);
* `resample_device`: the resampler alone, fast and generic, all 33 trials into one [33][64][n] array;
* `psearch_device_x33`: 33 calls of frbch_psearch_device, one per plane of that array -- what a caller had to do before, with the
  planes resampled beforehand (their resampling is NOT in this figure).

The one requirement: the single call is faster than the 33 calls (`single_call_faster`; the tool exits 1 otherwise).  The
records of the two routes are compared as well.

Kernel times come from a run of their own under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o pa -- python tools/accel_timing.py --trace
    python tools/accel_timing.py --out profiles/accel_timing.json --stats DIR/.../pa_kernel_stats.csv
"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
NDM, LOG2N, NACC, TSAMP = 64, 18, 33, 64e-6
TRACE_CALLS = 3


def spread(v):
    return dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3), calls=len(v))


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


class Case:
    def __init__(self, lib):
        import numpy as np
        from frb_baseband_amd import post
        self.lib, self.hip, self.held, self.post = lib, hip(), [], post
        self.n = self.nout = 1 << LOG2N
        rng = np.random.default_rng(5)
        y = (100.0 + 10.0 * rng.standard_normal((NDM, self.nout))).astype(np.float32)
        self.plane = self.alloc(y.nbytes)
        assert self.hip.hipMemcpy(self.plane, y.ctypes.data, y.nbytes, 1) == 0
        self.shifted = self.alloc(y.nbytes + 4)
        assert self.hip.hipMemcpy(self.shifted + 4, self.plane, y.nbytes, 3) == 0
        self.params = post.ps_params(TSAMP, 6.0)
        # a bin of drift at 100 Hz per step, 16 steps either side of 0
        self.accs = post.acc_list(16.0 * post.accel_step(self.n, TSAMP, 100.0), post.accel_step(self.n, TSAMP, 100.0))
        assert self.accs.size == NACC
        self.resampled = self.alloc(NACC * y.nbytes)
        self.pa = np.zeros(1 << 16, dtype=post.PA_CAND)
        self.ps = np.zeros(1 << 16, dtype=post.PS_CAND)

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), nbytes) == 0, "hipMalloc of %d bytes" % nbytes
        self.held.append(p.value)
        return p.value

    def free(self):
        for p in self.held:
            self.hip.hipFree(p)
        self.held = []

    def series(self, form):
        return self.plane if form == "fast" else self.shifted + 4

    def pasearch(self, form):
        ncand, used = C.c_uint64(0), (C.c_uint32 * 3)(9, 9, 9)
        err = C.create_string_buffer(512)
        t0 = time.perf_counter()
        rc = self.lib.frbch_pasearch_device(C.c_void_p(self.series(form)), NDM, self.nout, C.byref(self.params), self.accs.ctypes.data, NACC,
                                            0, 0, self.pa.ctypes.data, self.pa.size, C.byref(ncand), used, err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        assert used[0] == (1 if form == "fast" else 0), (form, used[0])
        return dt, self.pa[: ncand.value].copy(), (used[0], used[1], used[2])

    def resample(self, form):
        used = (C.c_uint32 * 1)(9)
        err = C.create_string_buffer(512)
        t0 = time.perf_counter()
        rc = self.lib.frbch_resample_device(C.c_void_p(self.series(form)), NDM, self.nout, self.n, TSAMP, self.accs.ctypes.data, NACC, 0,
                                            C.c_void_p(self.resampled), used, err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        assert used[0] == (1 if form == "fast" else 0), (form, used[0])
        return dt

    def psearch_x33(self):
        """-> (seconds for the 33 calls, their records as [(trial, PS_CAND records)])"""
        recs = []
        ncand, used = C.c_uint64(0), (C.c_uint32 * 2)(9, 9)
        err = C.create_string_buffer(512)
        t0 = time.perf_counter()
        for i in range(NACC):
            rc = self.lib.frbch_psearch_device(C.c_void_p(self.resampled + i * 4 * NDM * self.n), NDM, self.n, C.byref(self.params), 0,
                                               self.ps.ctypes.data, self.ps.size, C.byref(ncand), used, err, len(err))
            assert rc == 0, err.value
            recs.append(self.ps[: ncand.value].copy())
        return time.perf_counter() - t0, recs


def kernel_stats(path, calls):
    """-> milliseconds per frbch_pasearch_device call: the resampler, the search kernels, all of them"""
    rows = list(csv.DictReader(open(path)))
    name_key = next(k for k in rows[0] if k.lower() == "name")
    total_key = next(k for k in rows[0] if "total" in k.lower() and "duration" in k.lower())
    by = {}
    for r in rows:
        nm = r[name_key].split("(")[0].split(" ")[-1]
        if "frbch_post_ps_" in nm or "frbch_post_resample" in nm:
            by[nm] = by.get(nm, 0.0) + float(r[total_key]) * 1e-6 / calls
    res = sum(v for k, v in by.items() if "resample" in k)
    return dict(resampler_ms=round(res, 4), search_kernels_ms=round(sum(by.values()) - res, 4), all_kernels_ms=round(sum(by.values()), 4),
                by_kernel_ms={k: round(v, 4) for k, v in sorted(by.items())})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--trace", action="store_true", help="one warm-up call and %d calls of frbch_pasearch_device, nothing else (for the profiler)" % TRACE_CALLS)
    ap.add_argument("--stats", default=None, help="CSV of a --trace run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from frb_baseband_amd import _lib
    lib = _lib.load()
    c = Case(lib)
    if a.trace:
        for _ in range(1 + TRACE_CALLS):
            c.pasearch("fast")
        return 0
    n, rows, nb, sb = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    assert lib.frbch_pasearch_plan(NDM, c.nout, C.byref(c.params), NACC, 0, C.byref(n), C.byref(rows), C.byref(nb), C.byref(sb), None, 0) == 0
    out = dict(device="AMD Instinct MI355X (gfx950)", library=lib.frbch_version().decode(), clock="host clock around host-synchronous calls",
               calls=a.calls, shape=dict(ndm=NDM, nout=c.nout, nfft=n.value, nacc=NACC, tsamp=TSAMP, sigma=6.0),
               plan=dict(rows_per_batch=rows.value, batches=nb.value, scratch_bytes=sb.value))
    _t, rec_f, used = c.pasearch("fast")
    _t, rec_g, _u = c.pasearch("generic")
    c.resample("generic")
    c.resample("fast")
    _t, planes = c.psearch_x33()
    out["kernel_used"] = list(used)
    out["records"] = int(rec_f.size)
    out["resamplers_agree"] = bool(rec_f.tobytes() == rec_g.tobytes())
    out["routes_agree"] = all(
        all(rec_f[rec_f["acc_index"] == i][f].tobytes() == p[f].tobytes() for f in ("dm_index", "h", "k", "power", "sigma", "freq_hz"))
        for i, p in enumerate(planes))
    tf, tg, rf, rg, tx = [], [], [], [], []
    for _ in range(a.calls):
        tf.append(c.pasearch("fast")[0])
        tg.append(c.pasearch("generic")[0])
        rf.append(c.resample("fast"))
        rg.append(c.resample("generic"))
        tx.append(c.psearch_x33()[0])
    out["pasearch_device_fast_resampler"] = spread(tf)
    out["pasearch_device_generic_resampler"] = spread(tg)
    out["resample_device_fast"] = spread(rf)
    out["resample_device_generic"] = spread(rg)
    out["psearch_device_x33"] = spread(tx)
    out["single_call_over_33_calls"] = round(statistics.median(tf) / statistics.median(tx), 4)
    out["single_call_faster"] = bool(statistics.median(tf) < statistics.median(tx))
    if a.stats:
        out["kernels"] = dict(kernel_stats(a.stats, 1 + TRACE_CALLS),
                              source="rocprofv3 --kernel-trace --stats, a run of its own; per call over %d calls" % (1 + TRACE_CALLS))
        out["kernels"]["share_of_call"] = round(out["kernels"]["all_kernels_ms"] / out["pasearch_device_fast_resampler"]["median_ms"], 4)
        out["kernels"]["resampler_share_of_kernels"] = round(out["kernels"]["resampler_ms"] / out["kernels"]["all_kernels_ms"], 4)
    c.free()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0 if out["single_call_faster"] and out["routes_agree"] and out["resamplers_agree"] else 1


if __name__ == "__main__":
    sys.exit(main())
