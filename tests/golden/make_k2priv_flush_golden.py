#!/usr/bin/env python3
"""Record tests/golden/k2priv_flush.npz: offset / scale ([2][nif * nchan] float32 per case) of the cases of
tests/test_gpu_k2priv_flush.py, as the library of the commit BEFORE the flush of frbch_k2_priv's rescale sums became write-only
computes them (every flush added into the fp64 partial table in place).  Run once, on the GPU, with that commit's build:

    FRBCH_LIB=<build of the parent commit>/libfrbch.so python3 -B tests/golden/make_k2priv_flush_golden.py [out.npz]

(the recorded file: parent commit 744ae6d, MI355X, 512 workgroups, ten blocks).  "grid" and "nblocks" say what the bits belong to.
The test holds every later build to them.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from frb_baseband_amd import _lib, synth  # noqa: E402
from tests import test_gpu_k2priv_flush as t  # noqa: E402
from tests.hipmem import GuardedBuffer as DeviceBuffer  # noqa: E402


def main():
    lib = _lib.load()
    raw = synth.make_vdif(t.secs_of(t.MIN_BLOCKS), bw_mhz=t.BW, nchan=t.NCHAN)
    d_raw, nfr = DeviceBuffer.from_numpy(raw), raw.size // 8032
    grid = t.probe_grid(lib, d_raw, nfr)
    nblocks = t.blocks_for(grid)
    assert nblocks == t.MIN_BLOCKS and t.trips_of(nblocks, grid) >= t.MIN_TRIPS, (grid, nblocks)
    out = {"grid": np.int64(grid), "nblocks": np.int64(nblocks)}
    for name, (bw, kw, kernel, irows) in sorted(t.cases(nblocks, grid).items()):
        ((before, first), (before2, again)), record = t.measure(lib, d_raw, nfr, nblocks, bw, kw, runs=2, interval_rows=irows)
        assert kernel in record and record[kernel]["grid_x"] == grid, (name, record)
        assert np.isfinite(first).all() and t.same_bits(first, again), name
        out[name] = first
        if name.endswith("_t4_rows"):   # ... and the first interval's (the one frbch_k2_priv summed), read in front of the flush
            assert np.isfinite(before).all() and t.same_bits(before, before2) and not t.same_bits(before, first), name
            out[name + "__first"] = before
        print(name, first.shape, float(first[0].mean()), float(first[1].mean()), "closed in the launch" if before is not None else "open")
    bw, kw = t.add_case(nblocks)
    ((before, first), (_, again)), record = t.measure(lib, d_raw, nfr, nblocks, bw, kw, runs=2, calls=(1, nblocks - 1))
    assert "frbch_k2_priv<5, 2>" in record and record["frbch_k2_priv<5, 1>"]["launches"] >= 2, record
    assert before is None and np.isfinite(first).all() and t.same_bits(first, again), t.ADD_CASE
    out[t.ADD_CASE] = first
    print(t.ADD_CASE, first.shape, float(first[0].mean()), float(first[1].mean()), {k: v["launches"] for k, v in record.items() if "k2" in k})
    path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes, library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
