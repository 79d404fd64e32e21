#!/usr/bin/env python3
"""Record tests/golden/k2priv_stats.npz: offset / scale ([2][nif * nchan] float32 per case) of the cases of
tests/test_gpu_k2priv_stats.py, as the library of the commit BEFORE the statistics pass of frbch_k2_priv was trimmed computes
them.  Run once, on the GPU, with that commit's build:

    FRBCH_LIB=<build of the parent commit>/libfrbch.so python3 -B tests/golden/make_k2priv_stats_golden.py [out.npz]

(the recorded file: parent commit 2302363, MI355X).  The test holds every later build to these bits.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from frb_baseband_amd import _lib, synth  # noqa: E402
from tests import test_gpu_k2priv_stats as t  # noqa: E402
from tests.hipmem import GuardedBuffer as DeviceBuffer  # noqa: E402


def main():
    lib = _lib.load()
    raw = synth.make_vdif(t.SECS, bw_mhz=t.BW, nchan=t.NCHAN)
    d_raw, nfr = DeviceBuffer.from_numpy(raw), raw.size // 8032
    out = {}
    for name, (bw, kw, kernel) in sorted(t.CASES.items()):
        (first, again), record = t.measure(lib, d_raw, nfr, bw, kw, runs=2)
        assert kernel in record, (name, sorted(record))
        assert np.isfinite(first).all() and t.same_bits(first, again), name
        out[name] = first
        if name.endswith("_two_intervals"):   # ... and the first interval's, read between the two batches
            one, last, _ = t.measure_first_interval(lib, d_raw, nfr, bw, kw, nb_first=2)
            assert np.isfinite(one).all() and t.same_bits(last, first) and not t.same_bits(one, last), name
            out[name + "__first"] = one
        print(name, first.shape, float(first[0].mean()), float(first[1].mean()))
    path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes, library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
