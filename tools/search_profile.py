#!/usr/bin/env python3
"""Device-resident runs of the DM-range stage and the single-pulse search behind it (run on the GPU box, alone or under
`rocprofv3 --kernel-trace --stats -- <python> tools/search_profile.py`): 10 s x 1024 channels of 8-bit rows, 64 DMs, one warm-up
call and then five frbch_dedisperse_device and five frbch_spsearch_device calls (default widths, threshold 6), once more with a
width list that takes the generic kernels.  Prints the medians as JSON and, with an argument, writes them to that file
(profiles/spsearch_timing.json)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from frb_baseband_amd import _lib, post                      # noqa: E402
from tests.hipmem import DeviceBuffer                        # noqa: E402

lib = _lib.load()
rng = np.random.default_rng(3)
nrows, nchan = 312500, 1024
hdr = dict(nchans=nchan, nifs=1, nbits=8, fch1=1416.0 - 0.015625, foff=-0.03125, tsamp=32e-6, tstart=59000.0)
data = rng.integers(100, 156, size=(nrows, nchan), dtype=np.uint8)
d_rows = DeviceBuffer.from_numpy(data)
desc = post.fil_desc(hdr)
err = C.create_string_buffer(256)
dms = np.asarray(post.dm_list(300.0, 363.0, 1.0), dtype=np.float64)
nout = lib.frbch_dedisperse_nout(C.byref(desc), nrows, dms.ctypes.data, len(dms))
d_out = DeviceBuffer(len(dms) * nout * 4)
nclip, ncand, used = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
cands = np.zeros(4096, dtype=post.SP_CAND)


def timed(call, n=5):
    call()
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def dedisperse():
    assert lib.frbch_dedisperse_device(C.byref(desc), d_rows.ptr, nrows, dms.ctypes.data, len(dms), 0, 0.0, 0, d_out.ptr, nout,
                                       C.byref(nclip), err, len(err)) == 0, err.value


def search(params):
    assert lib.frbch_spsearch_device(d_out.ptr, len(dms), nout, C.byref(params), 0, cands.ctypes.data, cands.size, C.byref(ncand),
                                     C.byref(used), err, len(err)) == 0, err.value


out = {"rows_bytes": int(data.nbytes), "ndm": len(dms), "nout": int(nout), "plane_bytes": int(len(dms) * nout * 4), "threshold": 6.0,
       "dedisperse_device_median_ms": round(1e3 * timed(dedisperse), 3), "search": []}
for widths in (post.default_widths(hdr["tsamp"]), post.default_widths(hdr["tsamp"], 300 * hdr["tsamp"]),
               post.default_widths(hdr["tsamp"]) + [1024]):
    params = post.sp_params(widths, 6.0, 1000)
    ms = round(1e3 * timed(lambda: search(params)), 3)
    out["search"].append({"widths": widths, "kernel_used": used.value, "ncand": int(ncand.value), "spsearch_device_median_ms": ms})
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
