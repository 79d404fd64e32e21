#!/usr/bin/env python3
"""Time of the scattering fit on the GPU box, for profiles/scat_timing.json.

Shape: 8 bursts x 1024 channels (ffactor 16: 64 subbands) x 1 product x 8 bit, 256 bins x tfactor 4, a bank of 16 sigmas x 32 taus
x 256 taps, 128 trial arrival bins, 32768 rows (32 MiB), 1.2 - 1.5 GHz, DMs 50 .. 400: 8 x 64 x 512 x 128 sums of 256 taps,
8.6e9 multiply-adds.  The entry points take at most 2^24 sums a call, so the 8 bursts are two calls of 4; every figure below
is of ONE such call (4 bursts, 4.3e9 multiply-adds).  Timed in one run, alternating, `--calls` host-synchronous calls each after
one warm-up call, medians and spread on the host's clock (a composite call includes the burst sums, the dynamic spectrum, both
uses of the bank where cells are incomplete, 2 x 128 MiB of downloads and the host's fit):

* `burstscat_device` on the rows as the device allocator aligns them, and `burstscat_host` with the upload of the rows;
* the stage alone on the quantised planes of that call, `tbank_device` as the plan rule has it (fast) and with
  FRBCH_TBANK_GENERIC -- the composite has no switch for its kernel, so this pair is the comparison of the two kernels;
* once, tests/scat_oracle.tbank in numpy on the host, for the first burst alone.

The outputs of all forms are compared byte for byte.  Kernel times come from a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/scat_timing.py --calls 3 --no-numpy
    python tools/scat_timing.py --kernel-stats DIR --out profiles/scat_timing.json

What must hold is the project's standing rule: the plan rule sends a shape to the fast kernel only where its kernel time is
below the generic kernel's of the same build; the exit status says whether it does here."""
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
NCHAN, NROWS, NBURST, NCAND, NBIN, TFACTOR, FFACTOR, NSHIFT, SHIFT0 = 1024, 32768, 8, 4, 256, 4, 16, 128, 64
BANK = dict(nsig=16, ntau=32, ntap=256, lead=64, sigma0=0.5, rsig=2.0 ** 0.25, tau0=0.5, rtau=2.0 ** 0.25)


def spread(v):
    return dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3), calls=len(v))


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def kernel_stats(directory):
    """average microseconds and calls per kernel of this stage from rocprofv3's kernel_stats.csv"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Name"].split("(")[0]
            if "tbank" in name or "dynspec" in name or "burst_sums" in name or "acf_quant" in name:
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
    from tests import dmscan_oracle as do
    from tests import scat_oracle as so
    lib, h = _lib.load(), hip()
    held = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert h.hipMalloc(C.byref(p), nbytes) == 0, "hipMalloc of %d bytes" % nbytes
        held.append(p.value)
        return p.value

    hdr = dict(nchans=NCHAN, nifs=1, nbits=8, fch1=1500.0 - 150.0 / NCHAN, foff=-300.0 / NCHAN, tsamp=256e-6, tstart=59000.0, product=0)
    rng = np.random.default_rng(17)
    rows = rng.integers(90, 111, size=(NROWS, 1, NCHAN), dtype=np.uint8)
    bursts = []
    fc = hdr["fch1"] + np.arange(NCHAN) * hdr["foff"]
    t = np.arange(400, dtype=np.float64)
    for i in range(NBURST):
        dm, sample = 50.0 * (i + 1), 6000 + 2500 * i
        d = do.delays(hdr, dm)
        for c in range(NCHAN):                                       # a Gaussian of sigma 8 rows with a tail of 24 rows (nu / 1350)^-4
            tau = 24.0 * (fc[c] / 1350.0) ** -4.0
            prof = np.convolve(np.exp(-0.5 * ((t - 40.0) / 8.0) ** 2), np.exp(-t / tau))[:400]
            rows[sample - 40 + d[c]:sample - 40 + d[c] + 400, 0, c] += np.rint(12.0 * prof / prof.max()).astype(np.uint8)
        bursts.append((dm, sample, 80))
    cands = post.burst_cands(bursts[:NCAND], 600, 1024)
    d_rows = alloc(rows.nbytes + 16)
    assert h.hipMemcpy(d_rows, rows.ctypes.data, rows.nbytes, 1) == 0
    desc = post.fil_desc(hdr)
    bpar = _lib.FrbchBurstParams(C.sizeof(_lib.FrbchBurstParams), _lib.BURST_STOKES)
    bank = post.scat_bank_params(**BANK)
    par, fp = post.scat_params(NBIN, TFACTOR, FFACTOR, SHIFT0, NSHIFT), post.scat_fit_params(post.SCAT_ALPHAS, 5.0)
    nsub, K = NCHAN // FFACTOR, BANK["nsig"] * BANK["ntau"]
    err = C.create_string_buffer(512)

    def call(fn, ptr):
        Y, yhits, y = np.zeros((NCAND, nsub, NBIN), np.int64), np.zeros((NCAND, nsub, NBIN), np.uint32), np.zeros((NCAND, nsub, NBIN), np.int32)
        Cc, Nn = np.zeros((NCAND, nsub, K, NSHIFT), np.int64), np.zeros((NCAND, nsub, K, NSHIFT), np.int64)
        sub, band = np.zeros((NCAND, nsub), dtype=post.SCAT_SUB), np.zeros(NCAND, dtype=post.SCAT_BAND)
        k = (C.c_uint32 * 3)(9, 9, 9)
        t0 = time.perf_counter()
        rc = fn(C.byref(desc), C.c_void_p(ptr), NROWS, C.byref(bpar), cands.ctypes.data, NCAND, None, C.byref(par), C.byref(bank), C.byref(fp), 0,
                Y.ctypes.data, yhits.ctypes.data, y.ctypes.data, Cc.ctypes.data, Nn.ctypes.data, sub.ctypes.data, band.ctypes.data, None, k, err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        return dt, (k[0], k[1], k[2]), (Y, yhits, y, Cc, Nn, sub, band)

    _dt, _k, first = call(lib.frbch_burstscat_device, d_rows)
    y = first[2]
    p = post.scat_bank(bank, lib)["p"]
    sh = post.tbank_shape(nsub, NBIN, K, BANK["ntap"], BANK["lead"], SHIFT0, NSHIFT)
    d_y, d_P, d_C = alloc(y.nbytes), alloc(p.nbytes), alloc(first[3].nbytes)
    assert h.hipMemcpy(d_y, y.ctypes.data, y.nbytes, 1) == 0 and h.hipMemcpy(d_P, p.ctypes.data, p.nbytes, 1) == 0

    def stage(form):
        k = C.c_uint32(9)
        t0 = time.perf_counter()
        rc = lib.frbch_tbank_device(C.c_void_p(d_y), C.c_void_p(d_P), NCAND, C.byref(sh), form, 0, C.c_void_p(d_C), C.byref(k), err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        Cc = np.zeros((NCAND, nsub, K, NSHIFT), np.int64)
        assert h.hipMemcpy(Cc.ctypes.data, d_C, Cc.nbytes, 2) == 0
        return dt, (k.value,), (Cc,)

    runs = {"burstscat_device": lambda: call(lib.frbch_burstscat_device, d_rows), "burstscat_host": lambda: call(lib.frbch_burstscat_host, rows.ctypes.data),
            "tbank_device_fast": lambda: stage(_lib.TBANK_PLAN), "tbank_device_generic": lambda: stage(_lib.TBANK_GENERIC)}
    times = {name: [] for name in runs}
    kernels, last = {}, {}
    for name, fn in runs.items():                    # warm-up
        _dt, kernels[name], last[name] = fn()
    for _ in range(a.calls):
        for name, fn in runs.items():
            dt, _k, _o = fn()
            times[name].append(dt)
    assert kernels["burstscat_device"] == (1, 1, 1) and kernels["tbank_device_fast"] == (1,) and kernels["tbank_device_generic"] == (0,), kernels
    ref = last["burstscat_device"]
    same = all(x.tobytes() == z.tobytes() for x, z in zip(ref, last["burstscat_host"]))
    same = same and ref[3].tobytes() == last["tbank_device_fast"][0].tobytes() == last["tbank_device_generic"][0].tobytes()
    band = ref[6]
    macs = NCAND * nsub * K * NSHIFT * BANK["ntap"]
    out = dict(shape=dict(nchan=NCHAN, nrows=NROWS, nifs=1, nbits=8, bursts=NBURST, ncand_per_call=NCAND, nbin=NBIN, tfactor=TFACTOR, ffactor=FFACTOR,
                          shift0=SHIFT0, nshift=NSHIFT, bank=BANK, dms=[b[0] for b in bursts[:NCAND]], multiply_adds_per_call=macs),
               kernel_used={k: list(v) for k, v in kernels.items()}, ms={name: spread(v) for name, v in times.items()},
               outputs_equal=dict(all_forms=same), tau_ref_ms=[round(float(v), 3) for v in band["tau_ref_ms"]], alpha=[float(v) for v in band["alpha"]],
               injected=dict(tau_ref_ms_at_1350=24.0 * 0.256, alpha=4.0))
    if not a.no_numpy:
        t0 = time.perf_counter()
        w = so.tbank(y[:1], p, BANK["lead"], SHIFT0, NSHIFT)
        out["numpy_stage_of_one_burst_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        out["outputs_equal"]["numpy_first_burst"] = w.tobytes() == ref[3][:1].tobytes()
        same = same and out["outputs_equal"]["numpy_first_burst"]
    faster = None
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        out["kernels"] = ks
        out["kernels_how"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/scat_timing.py --calls 3 --no-numpy, a run of its own (same shape)"
        fast_us = sum(v["average_us"] for n, v in ks.items() if "tbank_fast" in n)
        gen_us = sum(v["average_us"] for n, v in ks.items() if n.endswith("frbch_post_tbank"))
        if fast_us and gen_us:
            faster = fast_us < gen_us
            out["tbank_kernel_us"] = dict(fast=round(fast_us, 2), generic=round(gen_us, 2), fast_is_faster=faster)
            out["tbank_fast_multiply_adds_per_s"] = round(macs / (fast_us * 1e-6), -9)
    out["how"] = "python tools/scat_timing.py --calls %d: host clock around host-synchronous calls, alternating, one warm-up each" % a.calls
    for ptr in held:
        h.hipFree(ptr)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same and faster is not False else 1


if __name__ == "__main__":
    raise SystemExit(main())
