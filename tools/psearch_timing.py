#!/usr/bin/env python3
"""Time of the periodicity search (frbch_psearch_device) on the GPU box, for profiles/psearch_timing.json:

* `post`: the README's post workload -- 10 s x 1024 channels of 8-bit noise rows, dedispersed at 64 DMs
  (frbch_dedisperse_device), the plane searched where it lies; the dedispersion is timed beside the search;
* `large`: 1024 series of 2^20 noise samples (16 distinct ones, 64 times over).

For each: the fast form (the series as the device allocator aligns them) against the generic form (the same series one float
further on, which the fast form refuses), `--calls` host-synchronous calls after one warm-up call each, alternating; medians and
spread on the host's clock.  The records of the two forms are compared as well.

Kernel times come from a run of their own under the profiler, one per form so that the shared kernels' times are the form's:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o fast -- python tools/psearch_timing.py --trace fast --case post
    python tools/psearch_timing.py --out profiles/psearch_timing.json --stats post:fast=DIR/.../fast_kernel_stats.csv ...

`--stats case:form=CSV` folds the kernel statistics of such a run into the result: total time per call of the transform's kernels
(frbch_post_ps_fft_* or frbch_post_ps_load / _stage) and of all frbch_post_ps_* kernels.
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
HDR = dict(nchans=1024, nifs=1, nbits=8, fch1=1416.0 - 0.015625, foff=-0.03125, tsamp=32e-6, tstart=59000.0)
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
    """the series of a case on the device, aligned and one float further on"""

    def __init__(self, name, lib):
        import numpy as np
        from frb_baseband_amd import post
        self.lib, self.name, self.hip, self.held = lib, name, hip(), []
        rng = np.random.default_rng(5)
        self.dedisperse = None
        if name == "post":
            nrows, nchan = 312500, HDR["nchans"]
            rows_h = rng.integers(100, 156, size=(nrows, nchan), dtype=np.uint8)
            rows = self.alloc(rows_h.nbytes)
            self.put(rows, rows_h)
            desc = post.fil_desc(HDR)
            dms = np.asarray(post.dm_list(300.0, 363.0, 1.0), dtype=np.float64)
            self.ndm = len(dms)
            self.nout = lib.frbch_dedisperse_nout(C.byref(desc), nrows, dms.ctypes.data, len(dms))
            self.tsamp = HDR["tsamp"]
            self.plane = self.alloc(4 * self.ndm * self.nout)
            err = C.create_string_buffer(256)
            nclip = C.c_uint64(0)

            def dedisperse():
                t0 = time.perf_counter()
                rc = lib.frbch_dedisperse_device(C.byref(desc), C.c_void_p(rows), nrows, dms.ctypes.data, len(dms), 0, 0.0, 0,
                                                 C.c_void_p(self.plane), self.nout, C.byref(nclip), err, len(err))
                dt = time.perf_counter() - t0
                assert rc == 0, err.value
                return dt
            self.dedisperse = dedisperse
            dedisperse()
            self.shape = dict(rows=nrows, nchan=nchan, nbits=8, ndm=self.ndm, nout=int(self.nout))
        else:
            self.ndm, self.nout, self.tsamp = 1024, 1 << 20, 64e-6
            self.plane = self.alloc(4 * self.ndm * self.nout)
            block = (100.0 + 10.0 * rng.standard_normal((16, self.nout))).astype(np.float32)      # 16 noise series, 64 times over
            for i in range(self.ndm // 16):
                self.put(self.plane + i * block.nbytes, block)
            self.shape = dict(ndm=self.ndm, nout=self.nout, distinct_series=16)
        count = self.ndm * self.nout
        self.shifted = self.alloc(4 * (count + 1))
        assert self.hip.hipMemcpy(self.shifted + 4, self.plane, 4 * count, 3) == 0          # device to device
        self.params = post.ps_params(self.tsamp, 6.0)
        self.n = lib.frbch_psearch_nfft(self.nout, C.byref(self.params))
        self.cands = np.zeros(1 << 16, dtype=post.PS_CAND)

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), nbytes) == 0, "hipMalloc of %d bytes" % nbytes
        self.held.append(p.value)
        return p.value

    def put(self, dst, arr):
        assert self.hip.hipMemcpy(dst, arr.ctypes.data, arr.nbytes, 1) == 0

    def free(self):
        for p in self.held:
            self.hip.hipFree(p)
        self.held = []

    def search(self, form):
        ptr = self.plane if form == "fast" else self.shifted + 4
        ncand, used = C.c_uint64(0), (C.c_uint32 * 2)(9, 9)
        err = C.create_string_buffer(512)
        t0 = time.perf_counter()
        rc = self.lib.frbch_psearch_device(C.c_void_p(ptr), self.ndm, self.nout, C.byref(self.params), 0, self.cands.ctypes.data, self.cands.size,
                                           C.byref(ncand), used, err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        assert used[0] == (1 if form == "fast" else 0), (form, used[0])
        return dt, self.cands[: ncand.value].copy(), (used[0], used[1])


def kernel_stats(path, calls):
    """-> milliseconds per call: {transform, all_psearch_kernels, by_kernel}"""
    rows = list(csv.DictReader(open(path)))
    name_key = next(k for k in rows[0] if k.lower() == "name")
    total_key = next(k for k in rows[0] if "total" in k.lower() and "duration" in k.lower())
    by = {}
    for r in rows:
        nm = r[name_key].split("(")[0].split(" ")[-1]
        if "frbch_post_ps_" in nm:
            by[nm] = by.get(nm, 0.0) + float(r[total_key]) * 1e-6 / calls
    fft = sum(v for k, v in by.items() if "_fft_" in k or k.endswith("_load") or k.endswith("_stage"))
    return dict(transform_ms=round(fft, 4), all_psearch_kernels_ms=round(sum(by.values()), 4), by_kernel_ms={k: round(v, 4) for k, v in sorted(by.items())})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--cases", default="post,large")
    ap.add_argument("--trace", default=None, choices=("fast", "generic"), help="one warm-up call and %d calls of this form, nothing else (for the profiler)" % TRACE_CALLS)
    ap.add_argument("--case", default="post", help="the case of --trace")
    ap.add_argument("--stats", action="append", default=[], help="case:form=CSV of a --trace run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from frb_baseband_amd import _lib
    lib = _lib.load()
    if a.trace:
        c = Case(a.case, lib)
        for _ in range(1 + TRACE_CALLS):
            c.search(a.trace)
        return
    out = dict(device="AMD Instinct MI355X (gfx950)", library=lib.frbch_version().decode(), clock="host clock around host-synchronous calls",
               calls=a.calls, cases={})
    for name in a.cases.split(","):
        c = Case(name, lib)
        r = out["cases"][name] = dict(shape=c.shape, nfft=int(c.n), sigma=6.0, nharm=16, wblock=128)
        _t, rec_f, used = c.search("fast")
        _t, rec_g, _u = c.search("generic")
        r["passes"] = used[1]
        r["records"] = int(rec_f.size)
        r["forms_agree"] = bool(rec_f.tobytes() == rec_g.tobytes())
        tf, tg, td = [], [], []
        for _ in range(a.calls):
            tf.append(c.search("fast")[0])
            tg.append(c.search("generic")[0])
            if c.dedisperse:
                td.append(c.dedisperse())
        r["psearch_device_fast"] = spread(tf)
        r["psearch_device_generic"] = spread(tg)
        if td:
            r["dedisperse_device"] = spread(td)
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        c.free()
    for spec in a.stats:
        key, path = spec.split("=", 1)
        case, form = key.split(":")
        out["cases"].setdefault(case, {})["kernels_" + form] = dict(kernel_stats(path, 1 + TRACE_CALLS), source="rocprofv3 --kernel-trace --stats, a run of its own; per call over %d calls" % (1 + TRACE_CALLS))
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
