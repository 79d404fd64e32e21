#!/usr/bin/env python3
"""Time of the burst polarisation stage on the GPU box, for profiles/rm_timing.json.

Shape: 1024 channels x 4 products x 8 bit, 32768 rows (128 MiB), 8 bursts (16 on-pulse rows, two off-pulse windows of 4096
rows, DMs 100 .. 800), nphi = 16384 trials.  Timed in one run, alternating, `--calls` host-synchronous calls each after one
warm-up call, medians and spread on the host's clock (a call includes its small uploads, its downloads and the host's part:
delays, records, spectra, peaks):

* `burstspec_device`: the rows as the device allocator aligns them (the fast kernel), and the same rows 4 bytes further on (the
  generic kernel);
* `rmsynth_device`: F at an 8-byte aligned address (the fast kernel) and 4 bytes further on (the generic kernel);
* `burst_rm_device`: the composite, next to the sum of the two fast stages.

The outputs of the two forms of each stage are compared byte for byte.  Nothing is required of the ratios: the file says which
form was faster, and DESIGN.md section 10 says what follows from it for the plan rule.

    python tools/rm_timing.py --out profiles/rm_timing.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
NCHAN, NROWS, NCAND, NPHI = 1024, 32768, 8, 16384


def spread(v):
    return dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3), calls=len(v))


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
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
    rng = np.random.default_rng(11)
    rows = rng.integers(90, 111, size=(NROWS, 4, NCHAN), dtype=np.uint8)
    l2 = post.lambda2(hdr)
    bursts = []
    for i in range(NCAND):
        dm, sample, rm = 100.0 * (i + 1), 6000 + 2500 * i, -1400.0 + 400.0 * i
        d = np.rint(dm * post.DM_CONST * ((hdr["fch1"] + np.arange(NCHAN) * hdr["foff"]) ** -2.0 - hdr["fch1"] ** -2.0) / hdr["tsamp"]).astype(np.int64)
        amp = [40.0 * np.ones(NCHAN), 30.0 * np.cos(2.0 * rm * l2), 30.0 * np.sin(2.0 * rm * l2), 5.0 * np.ones(NCHAN)]
        for t in range(sample - 8, sample + 8):
            r = t + d
            ok = r < NROWS
            for p in range(4):
                rows[r[ok], p, np.arange(NCHAN)[ok]] += np.rint(amp[p][ok]).astype(np.int64).astype(np.uint8)
        bursts.append((dm, sample, 16))
    cands = post.burst_cands(bursts, 64, 4096)
    d_rows = alloc(rows.nbytes + 16)
    assert h.hipMemcpy(d_rows, rows.ctypes.data, rows.nbytes, 1) == 0
    d_rows4 = alloc(rows.nbytes + 16)
    assert h.hipMemcpy(d_rows4 + 4, rows.ctypes.data, rows.nbytes, 1) == 0
    nsum = NCAND * 4 * NCHAN
    d_sums = alloc(nsum * post.BURST_SUMS.itemsize)
    desc = post.fil_desc(hdr)
    bpar = _lib.FrbchBurstParams(C.sizeof(_lib.FrbchBurstParams), _lib.BURST_STOKES)
    nphi, phi_lo, dphi = NPHI, -(NPHI // 2) * 0.5, 0.5
    rpar = post.rm_params(nphi, phi_lo, dphi)
    err = C.create_string_buffer(512)
    out = {}

    def spectra(ptr):
        spec, noise = np.zeros((NCAND, 4, NCHAN), np.float32), np.zeros((NCAND, 4, NCHAN), np.float32)
        used = np.zeros((NCAND, NCHAN), np.uint8)
        k = C.c_uint32(9)
        t0 = time.perf_counter()
        rc = lib.frbch_burstspec_device(C.byref(desc), C.c_void_p(ptr), NROWS, C.byref(bpar), cands.ctypes.data, NCAND, None, 0, C.c_void_p(d_sums),
                                        spec.ctypes.data, noise.ctypes.data, used.ctypes.data, C.byref(k), err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        return dt, k.value, (spec, noise, used)

    _dt, _k, (spec, noise, used) = spectra(d_rows)
    q, u = np.ascontiguousarray(spec[:, 1]), np.ascontiguousarray(spec[:, 2])
    d_q, d_u, d_used = alloc(q.nbytes), alloc(u.nbytes), alloc(used.nbytes)
    for dst, src in ((d_q, q), (d_u, u), (d_used, used)):
        assert h.hipMemcpy(dst, src.ctypes.data, src.nbytes, 1) == 0
    d_F = alloc(NCAND * nphi * 8 + 16)

    def synth(off):
        k = (C.c_uint32 * 2)(9, 9)
        t0 = time.perf_counter()
        rc = lib.frbch_rmsynth_device(C.byref(desc), C.c_void_p(d_q), C.c_void_p(d_u), C.c_void_p(d_used), NCAND, C.byref(rpar), 0,
                                      C.c_void_p(d_F + off), k, err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        F = np.zeros((NCAND, nphi, 2), np.float32)
        assert h.hipMemcpy(F.ctypes.data, d_F + off, F.nbytes, 2) == 0
        return dt, (k[0], k[1]), F

    def composite():
        s, n = np.zeros((NCAND, 4, NCHAN), np.float32), np.zeros((NCAND, 4, NCHAN), np.float32)
        us = np.zeros((NCAND, NCHAN), np.uint8)
        F = np.zeros((NCAND, nphi, 2), np.float32)
        res = np.zeros(NCAND, dtype=post.RM_RESULT)
        k = (C.c_uint32 * 3)(9, 9, 9)
        t0 = time.perf_counter()
        rc = lib.frbch_burst_rm_device(C.byref(desc), C.c_void_p(d_rows), NROWS, C.byref(bpar), cands.ctypes.data, NCAND, None, None, C.byref(rpar), 0,
                                       s.ctypes.data, n.ctypes.data, us.ctypes.data, F.ctypes.data, res.ctypes.data, k, err, len(err))
        dt = time.perf_counter() - t0
        assert rc == 0, err.value
        return dt, (k[0], k[1], k[2]), (F, res)

    runs = {"burstspec_fast": lambda: spectra(d_rows), "burstspec_generic": lambda: spectra(d_rows4 + 4), "rmsynth_fast": lambda: synth(0),
            "rmsynth_generic": lambda: synth(4), "burst_rm": composite}
    times = {name: [] for name in runs}
    kernels, last = {}, {}
    for name, fn in runs.items():                    # warm-up
        _dt, kernels[name], last[name] = fn()
    for _ in range(a.calls):
        for name, fn in runs.items():
            dt, _k, _o = fn()
            times[name].append(dt)
    assert kernels["burstspec_fast"] == 1 and kernels["burstspec_generic"] == 0, kernels
    assert kernels["rmsynth_fast"][0] == 1 and kernels["rmsynth_generic"] == (0, 1), kernels
    same_spec = all(x.tobytes() == y.tobytes() for x, y in zip(last["burstspec_fast"], last["burstspec_generic"]))
    same_F = last["rmsynth_fast"].tobytes() == last["rmsynth_generic"].tobytes() == last["burst_rm"][0].tobytes()
    res = last["burst_rm"][1]
    out = dict(shape=dict(nchan=NCHAN, nrows=NROWS, nifs=4, nbits=8, ncand=NCAND, nphi=nphi, dphi=dphi, width=16, off_len=4096,
                          terms=NCAND * NCHAN * nphi),
               kernel_used={k: list(v) if isinstance(v, tuple) else v for k, v in kernels.items()},
               ms={name: spread(v) for name, v in times.items()},
               outputs_equal=dict(spectra_fast_vs_generic=same_spec, F_fast_vs_generic_vs_composite=same_F),
               recovered_rm=[round(float(x), 3) for x in res["rm"]], injected_rm=[-1400.0 + 400.0 * i for i in range(NCAND)])
    m = out["ms"]
    out["burstspec_fast_over_generic"] = round(m["burstspec_fast"]["median_ms"] / m["burstspec_generic"]["median_ms"], 3)
    out["rmsynth_fast_over_generic"] = round(m["rmsynth_fast"]["median_ms"] / m["rmsynth_generic"]["median_ms"], 3)
    out["sum_of_fast_stages_ms"] = round(m["burstspec_fast"]["median_ms"] + m["rmsynth_fast"]["median_ms"], 3)
    out["how"] = "python tools/rm_timing.py --calls %d: host clock around host-synchronous calls, alternating, one warm-up each" % a.calls
    for p in held:
        h.hipFree(p)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same_spec and same_F else 1


if __name__ == "__main__":
    raise SystemExit(main())
