#!/usr/bin/env python3
"""Time of the delay x RM transform on the GPU box, for profiles/polcal_timing.json.

Two shapes of the transform alone, spectra of 1024 channels already on the device: 8 pulses x 1024 phi x 257 tau (2.2e9 terms)
and 1 pulse x 4096 phi x 33 tau.  Timed in one run, alternating, `--calls` host-synchronous calls each after one warm-up call,
medians and spread on the host's clock (a call includes its downloads of q, u and used, the records and their upload):

* `fast`: frbch_rmdelay_device with F at an 8-byte aligned address;
* `generic`: the same with F 4 bytes further on;
* `loop`: what anyone could write without this entry point -- ntau calls of frbch_rmsynth_device, one per trial delay, on spectra
  rotated by exp(-2 pi i tau (f - f0)) on the host beforehand and already on the device (neither is in the time).

fast and generic are compared byte for byte; the loop rotates in float32 before the quantisation, so it is compared by the
largest |F_loop - F_fast| / max |F|.  The condition the fast form has to meet: not slower than the loop at both shapes
(`fast_not_slower_than_loop`).  Then the composite frbch_burst_polcal_host on 128 MiB of rows next to its stages called one after
the other (frbch_burstspec_host, frbch_rmdelay_host, frbch_rmdelay_peaks).

    python tools/polcal_timing.py --out profiles/polcal_timing.json
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
NCHAN = 1024
SHAPES = {"8x1024x1024x257": (8, 1024, 257), "1x1024x4096x33": (1, 4096, 33)}        # ncand, nphi, ntau
NROWS, NCAND = 32768, 8


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
    ap.add_argument("--calls", type=int, default=5)
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

    def put(arr):
        p = alloc(arr.nbytes)
        assert h.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0
        return p

    hdr = dict(nchans=NCHAN, nifs=4, nbits=8, fch1=1500.0 - 150.0 / NCHAN, foff=-300.0 / NCHAN, tsamp=256e-6, tstart=59000.0)
    desc = post.fil_desc(hdr)
    f = hdr["fch1"] + np.arange(NCHAN) * hdr["foff"]
    l2 = post.lambda2(hdr)
    err = C.create_string_buffer(512)
    out = dict(shapes={}, how="python tools/polcal_timing.py --calls %d: host clock around host-synchronous calls, alternating, one warm-up each" % a.calls)
    ok = True
    for name, (ncand, nphi, ntau) in SHAPES.items():
        rng = np.random.default_rng(21)
        ang = 2.0 * (0.3 + 350.0 * l2)[None, :] + 2.0 * np.pi * f[None, :] * 2.5e-3 + 0.2 * np.arange(ncand)[:, None]
        q = (3.0 * np.cos(ang) + rng.normal(0, 0.4, (ncand, NCHAN))).astype(np.float32)
        u = (3.0 * np.sin(ang) + rng.normal(0, 0.4, (ncand, NCHAN))).astype(np.float32)
        used = np.ones((ncand, NCHAN), np.uint8)
        used[:, 100:103] = 0
        dphi, dtau = 2.0, 0.125e-3
        phi_lo, tau_lo = 350.0 - (nphi // 2) * dphi, -(ntau // 2) * dtau
        par = post.rmd_params(nphi, phi_lo, dphi, ntau, tau_lo, dtau)
        rpar = post.rm_params(nphi, phi_lo, dphi)
        d_q, d_u, d_used = put(q), put(u), put(used)
        nF = ncand * ntau * nphi * 8
        d_F, d_L = alloc(nF + 16), alloc(nF)
        f0 = np.array([f[used[i] != 0].mean() for i in range(ncand)])
        rot = []
        for m in range(ntau):                                   # the baseline's spectra, rotated on the host beforehand
            w = np.exp(-2j * np.pi * (tau_lo + m * dtau) * (f[None, :] - f0[:, None]))
            z = (q.astype(np.float64) + 1j * u.astype(np.float64)) * w
            rot.append((put(np.ascontiguousarray(z.real.astype(np.float32))), put(np.ascontiguousarray(z.imag.astype(np.float32)))))

        def transform(off):
            k = (C.c_uint32 * 2)(9, 9)
            t0 = time.perf_counter()
            rc = lib.frbch_rmdelay_device(C.byref(desc), C.c_void_p(d_q), C.c_void_p(d_u), C.c_void_p(d_used), ncand, C.byref(par), 0,
                                          C.c_void_p(d_F + off), k, err, len(err))
            dt = time.perf_counter() - t0
            assert rc == 0, err.value
            F = np.zeros((ncand, ntau, nphi, 2), np.float32)
            assert h.hipMemcpy(F.ctypes.data, d_F + off, F.nbytes, 2) == 0
            return dt, (k[0], k[1]), F

        def loop():
            # F of trial m of every candidate lies behind one another here: [ntau][ncand][nphi][2]
            t0 = time.perf_counter()
            for m, (dq, du) in enumerate(rot):
                rc = lib.frbch_rmsynth_device(C.byref(desc), C.c_void_p(dq), C.c_void_p(du), C.c_void_p(d_used), ncand, C.byref(rpar), 0,
                                              C.c_void_p(d_L + m * ncand * nphi * 8), None, err, len(err))
                assert rc == 0, err.value
            dt = time.perf_counter() - t0
            F = np.zeros((ntau, ncand, nphi, 2), np.float32)
            assert h.hipMemcpy(F.ctypes.data, d_L, F.nbytes, 2) == 0
            return dt, None, np.ascontiguousarray(F.transpose(1, 0, 2, 3))

        runs = {"fast": lambda: transform(0), "generic": lambda: transform(4), "loop": loop}
        times = {n: [] for n in runs}
        kernels, last = {}, {}
        for n, fn in runs.items():
            _dt, kernels[n], last[n] = fn()
        for _ in range(a.calls):
            for n, fn in runs.items():
                times[n].append(fn()[0])
        assert kernels["fast"][0] == 1 and kernels["generic"] == (0, 1), kernels
        same = last["fast"].tobytes() == last["generic"].tobytes()
        scale = float(np.abs(last["fast"]).max())
        loop_diff = float(np.abs(last["loop"] - last["fast"]).max()) / scale
        P = (last["fast"].astype(np.float64) ** 2).sum(axis=-1)[0]
        mp, kp = np.unravel_index(int(np.argmax(P)), P.shape)
        ms = {n: spread(v) for n, v in times.items()}
        s = dict(ncand=ncand, nchan=NCHAN, nphi=nphi, ntau=ntau, terms=ncand * NCHAN * nphi * ntau, kernel_used=dict(fast=list(kernels["fast"]), generic=[0, 1]),
                 ms=ms, fast_equals_generic=same, loop_max_diff_over_max=loop_diff, peak_tau_ns=round((tau_lo + mp * dtau) * 1e3, 4),
                 peak_rm=phi_lo + kp * dphi, fast_over_generic=round(ms["fast"]["median_ms"] / ms["generic"]["median_ms"], 3),
                 fast_over_loop=round(ms["fast"]["median_ms"] / ms["loop"]["median_ms"], 4),
                 fast_not_slower_than_loop=ms["fast"]["median_ms"] <= ms["loop"]["median_ms"])
        out["shapes"][name] = s
        ok = ok and same and loop_diff < 2.0e-3 and s["fast_not_slower_than_loop"]
        for p in held:
            h.hipFree(p)
        del held[:]

    # the composite against its stages, host pointers throughout
    rng = np.random.default_rng(11)
    rows = rng.integers(90, 111, size=(NROWS, 4, NCHAN), dtype=np.uint8)
    bursts = []
    for i in range(NCAND):
        dm, sample = 100.0 * (i + 1), 6000 + 2500 * i
        d = np.rint(dm * post.DM_CONST * (f ** -2.0 - hdr["fch1"] ** -2.0) / hdr["tsamp"]).astype(np.int64)
        ang = 2.0 * (0.3 * i + 350.0 * l2) + 2.0 * np.pi * f * 2.5e-3
        amp = [40.0 * np.ones(NCHAN), 30.0 * np.cos(ang), 30.0 * np.sin(ang), 5.0 * np.ones(NCHAN)]
        for t in range(sample - 8, sample + 8):
            r = t + d
            sel = r < NROWS
            for p in range(4):
                rows[r[sel], p, np.arange(NCHAN)[sel]] += np.rint(amp[p][sel]).astype(np.int64).astype(np.uint8)
        bursts.append((dm, sample, 16))
    cands = post.burst_cands(bursts, 64, 4096)
    grid = dict(nphi=1024, phi_lo=350.0 - 512 * 2.0, dphi=2.0, ntau=33, tau_lo=-16 * 0.25e-3, dtau=0.25e-3)

    def composite():
        t0 = time.perf_counter()
        r = post.polcal(rows, hdr, cands, lib=lib, **grid)
        return time.perf_counter() - t0, r

    def stages():
        t0 = time.perf_counter()
        spec, noise, used = post.burst_spectra(rows, hdr, cands, lib=lib)
        F = post.rm_delay(spec[:, 1], spec[:, 2], used, hdr, lib=lib, **grid)
        res = post.rm_delay_peaks(F, used, noise[:, 1], noise[:, 2], hdr, lib=lib, **grid)
        return time.perf_counter() - t0, dict(F=F, results=res)

    runs = {"burst_polcal_host": composite, "stages_one_after_the_other": stages}
    times = {n: [] for n in runs}
    last = {n: fn()[1] for n, fn in runs.items()}
    for _ in range(a.calls):
        for n, fn in runs.items():
            times[n].append(fn()[0])
    same = last["burst_polcal_host"]["F"].tobytes() == last["stages_one_after_the_other"]["F"].tobytes() and \
        last["burst_polcal_host"]["results"].tobytes() == last["stages_one_after_the_other"]["results"].tobytes()
    comb = last["burst_polcal_host"]["results"][-1]
    ms = {n: spread(v) for n, v in times.items()}
    out["composite"] = dict(shape=dict(nchan=NCHAN, nrows=NROWS, nifs=4, nbits=8, ncand=NCAND, width=16, off_len=4096, **grid), ms=ms, outputs_equal=same,
                            composite_over_stages=round(ms["burst_polcal_host"]["median_ms"] / ms["stages_one_after_the_other"]["median_ms"], 3),
                            combined_tau_ns=round(float(comb["tau"]) * 1e3, 4), combined_rm=round(float(comb["rm"]), 3),
                            ridge_slope_per_ns=round(float(comb["ridge_slope"]) * 1e-3, 3))
    ok = ok and same
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
