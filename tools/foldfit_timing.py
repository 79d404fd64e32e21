#!/usr/bin/env python3
"""Time of the fold refinement on the GPU box, for profiles/foldfit_timing.json.

The shape: 60 sub-integrations x 1024 channels x 1024 bins x 1 product (a cube of 0.5 GB and 0.25 GB of hits, folded on the device
from 8-bit rows of 256 us), 65 DMs x 65 frequencies x 33 derivatives.  Timed in one run on the host's clock, host-synchronous
calls, forms alternating, the median of `--calls` calls after one warm-up call each:

* `fast` / `generic`: frbch_foldfit_device on the resident cube at a 16-byte aligned address and 4 bytes further on (the plan rule
  then takes the generic kernels in both stages); the scores are compared byte for byte;
* `kernel_ms`: the time of every kernel of the two forms, per stage, from a kernel trace of a run of its own (`rocprofv3
  --kernel-trace --stats -d DIR -o ff -- python tools/foldfit_timing.py --kernels-only --calls 2`, then `--trace-db
  DIR/ff_results.db` here): the host clock cannot part the stages of one call;
* `composite`: frbch_fold_refine_host on the rows against `sequence`: frbch_foldp_host (rows up, cube down) then frbch_foldfit_host
  (cube up);
* `numpy_one_dm`: tests/foldfit_oracle.py, both stages and the scores for ONE DM of the 65.

    python tools/foldfit_timing.py --out profiles/foldfit_timing.json
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
NSUB, NCHAN, NBIN = 60, 1024, 1024
NDM, NFREQ, NFDOT = 65, 65, 33
TSAMP, SUBINT, F0, DM = 256.0e-6, 10.0, 3.9, 60.0


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
    ap.add_argument("--kernels-only", action="store_true", help="the device calls alone, for a run under a kernel trace")
    ap.add_argument("--trace-db", default=None, help="the database a kernel trace of a --kernels-only run left: its kernel times go into the result")
    a = ap.parse_args()
    import numpy as np
    from frb_baseband_amd import _lib, post
    from tests import foldfit_oracle as fo
    lib, h = _lib.load(), hip()
    hdr = dict(nchans=NCHAN, nifs=1, nbits=8, fch1=1500.0, foff=-300.0 / NCHAN, tsamp=TSAMP, tstart=60000.0, product=0)
    desc = post.fil_desc(hdr)
    L = fo.rows_per_sub(hdr, SUBINT)
    nrows = NSUB * L
    assert lib.frbch_fold_nsub(C.byref(desc), nrows, SUBINT) == NSUB
    rng = np.random.default_rng(7)
    rows = rng.integers(80, 120, (nrows, 1, NCHAN), dtype=np.uint8)
    par = {"F0": F0, "F1": 0.0, "DM": DM, "PEPOCH": hdr["tstart"], "PSR": "timing"}
    model, _keep = post.fold_model(par, hdr, nbin=NBIN, subint_s=SUBINT, apply_delays=False)
    fpar = post.foldfit_params(hdr, nrows, NBIN, NSUB, F0, SUBINT, DM, ndm=NDM, nfreq=NFREQ, nfdot=NFDOT, lib=lib)
    err = C.create_string_buffer(512)

    # the cube: folded by the library, kept on the host for the sequence and the restatement
    cube = np.zeros((NSUB, 1, NBIN, NCHAN), np.float64)
    hits = np.zeros((NSUB, NBIN, NCHAN), np.uint32)
    kf = C.c_uint32(9)
    assert lib.frbch_foldp_host(C.byref(desc), rows.ctypes.data, nrows, C.byref(model), 0, cube.ctypes.data, hits.ctypes.data, NSUB, C.byref(kf), err,
                                len(err)) == 0, err.value

    def resident(arr, off):
        p = C.c_void_p()
        assert h.hipMalloc(C.byref(p), arr.nbytes + 16) == 0
        assert h.hipMemcpy(C.c_void_p(p.value + off), arr.ctypes.data, arr.nbytes, 1) == 0
        return p, C.c_void_p(p.value + off)
    bufs = {off: (resident(cube, off), resident(hits, off)) for off in (0, 4)}

    def outputs(p):
        return dict(score=np.zeros((p.ndm, p.nfdot, p.nfreq)), acc=np.zeros((2, NBIN), np.int64), hits=np.zeros((2, NBIN), np.uint64),
                    res=np.zeros(1, post.FOLDFIT_RESULT), k=(C.c_uint32 * 3)(9, 9, 9))

    def device_call(p, off, o):
        (_c, cp), (_h, hp) = bufs[off]
        t = time.perf_counter()
        rc = lib.frbch_foldfit_device(C.byref(desc), nrows, C.byref(p), cp, hp, None, 0, o["score"].ctypes.data, o["acc"].ctypes.data, o["hits"].ctypes.data,
                                      o["res"].ctypes.data, None, None, None, None, o["k"], err, len(err))
        dt = time.perf_counter() - t
        assert rc == 0, err.value
        return dt

    arms = {"fast": (fpar, 0), "generic": (fpar, 4)}
    outs = {name: outputs(p) for name, (p, _off) in arms.items()}
    times = {name: [] for name in arms}
    for name, (p, off) in arms.items():
        device_call(p, off, outs[name])                                          # warm-up
    for _ in range(a.calls):
        for name, (p, off) in arms.items():
            times[name].append(device_call(p, off, outs[name]))
    kernels = {name: [int(outs[name]["k"][0]), int(outs[name]["k"][1])] for name in arms}
    assert kernels["fast"] == [1, 1] and kernels["generic"] == [0, 0], kernels
    same = outs["fast"]["score"].tobytes() == outs["generic"]["score"].tobytes() and outs["fast"]["res"].tobytes() == outs["generic"]["res"].tobytes()
    med = {name: statistics.median(v) for name, v in times.items()}
    result = {
        "shape": dict(nsub=NSUB, nchan=NCHAN, nbin=NBIN, products=1, ndm=NDM, nfreq=NFREQ, nfdot=NFDOT, rows=int(nrows), tsamp_s=TSAMP,
                      cube_mib=round(cube.nbytes / 2 ** 20, 1), hits_mib=round(hits.nbytes / 2 ** 20, 1), fold_kernel=int(kf.value),
                      adds_stage1=NDM * NSUB * NBIN * NCHAN, adds_stage2=NDM * NFREQ * NFDOT * NSUB * NBIN),
        "clock": "host, time.perf_counter around host-synchronous calls; one warm-up call, then %d calls an arm, arms alternating" % a.calls,
        "calls": {name: dict(spread(v), kernel_used=kernels[name]) for name, v in times.items()},
        "fast_equals_generic_bytes": bool(same),
    }
    result["fast_is_faster"] = {"whole": med["fast"] < med["generic"]}
    if a.trace_db:
        import sqlite3
        cur = sqlite3.connect(a.trace_db).cursor()
        full = {"frbch_post_ff_dm": NDM * NSUB * NBIN, "frbch_post_ff_spin": -(-NDM * NFREQ * NFDOT // 256) * 256}     # grid.x of the full launches
        km = {}
        for name, gx, n, lo, mid, hi in cur.execute("select name, grid_x, count(*), min(duration), avg(duration), max(duration) from kernels "
                                                    "where name like '%frbch_post_ff_%' group by name, grid_x"):
            short = name.replace("void ", "").replace("(FfParams)", "")
            if short in full and gx != full[short]:
                continue
            km[short] = dict(launches=n, min_ms=round(lo / 1e6, 3), mean_ms=round(mid / 1e6, 3), max_ms=round(hi / 1e6, 3))
        result["kernel_ms"] = km
        s1f = km["fast::frbch_post_ff_dm_fast<4>"]["mean_ms"] + km["fast::frbch_post_ff_dm_join"]["mean_ms"]
        result["stage_ms"] = {"stage1_fast": round(s1f, 3), "stage1_generic": km["frbch_post_ff_dm"]["mean_ms"],
                              "stage2_fast": km["fast::frbch_post_ff_spin_fast<4>"]["mean_ms"], "stage2_generic": km["frbch_post_ff_spin"]["mean_ms"],
                              "source": "kernel trace of a run of its own (rocprofv3 --kernel-trace --stats), mean of the launches; stage 1 fast = the tile kernel + the join"}
        st = result["stage_ms"]
        result["fast_is_faster"].update(stage1=st["stage1_fast"] < st["stage1_generic"], stage2=st["stage2_fast"] < st["stage2_generic"])
    if not a.kernels_only:
        # the composite against the two calls in sequence
        n = max(3, a.calls // 2)
        comp, seq = [], []
        o1, o2 = outputs(fpar), outputs(fpar)
        cube2, hits2 = np.zeros_like(cube), np.zeros_like(hits)
        for i in range(n + 1):
            t = time.perf_counter()
            rc = lib.frbch_fold_refine_host(C.byref(desc), rows.ctypes.data, nrows, C.byref(model), C.byref(fpar), None, 0, None, None, o1["score"].ctypes.data,
                                            o1["acc"].ctypes.data, o1["hits"].ctypes.data, o1["res"].ctypes.data, None, None, o1["k"], err, len(err))
            t1 = time.perf_counter()
            assert rc == 0, err.value
            rc = lib.frbch_foldp_host(C.byref(desc), rows.ctypes.data, nrows, C.byref(model), 0, cube2.ctypes.data, hits2.ctypes.data, NSUB, None, err, len(err))
            assert rc == 0, err.value
            rc = lib.frbch_foldfit_host(C.byref(desc), nrows, C.byref(fpar), cube2.ctypes.data, hits2.ctypes.data, None, 0, o2["score"].ctypes.data,
                                        o2["acc"].ctypes.data, o2["hits"].ctypes.data, o2["res"].ctypes.data, None, None, None, None, o2["k"], err, len(err))
            t2 = time.perf_counter()
            assert rc == 0, err.value
            if i:
                comp.append(t1 - t)
                seq.append(t2 - t1)
        result["composite"] = dict(spread(comp), kernel_used=[int(v) for v in o1["k"]], rows_mib=round(rows.nbytes / 2 ** 20, 1))
        result["sequence"] = dict(spread(seq), note="frbch_foldp_host (rows up, cube down) then frbch_foldfit_host (cube up)")
        result["composite_equals_sequence_bytes"] = bool(o1["score"].tobytes() == o2["score"].tobytes() == outs["fast"]["score"].tobytes())
        # numpy, one DM
        t = time.perf_counter()
        _dms, shd, shp, _tau = fo.tables(hdr, nrows, NBIN, NSUB, F0, SUBINT, DM, 1, fpar.ddm, NFREQ, fpar.dfreq, NFDOT, fpar.dfdot)
        A, HA = fo.stage1(cube, hits, np.ones(NCHAN, bool), 1, shd)
        t1 = time.perf_counter()
        sc = fo.scores(A, HA, shp)
        t2 = time.perf_counter()
        result["numpy_one_dm"] = dict(stage1_s=round(t1 - t, 2), stage2_and_scores_s=round(t2 - t1, 2),
                                      equals_library_bytes=bool(sc[0].tobytes() == outs["fast"]["score"][NDM // 2].tobytes()))
    for (c, _cp), (hh, _hp) in bufs.values():
        h.hipFree(c)
        h.hipFree(hh)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    # the plan rule sends this shape to the fast forms: that stands only where they are measured faster
    slower = [k for k, v in result["fast_is_faster"].items() if not v]
    if slower or not same:
        sys.exit("the fast form is not faster (%s) or differs from the generic one: the plan rule must not take it" % ", ".join(slower))


if __name__ == "__main__":
    main()
