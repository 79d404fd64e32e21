#!/usr/bin/env python3
"""Device-resident runs of the interference stage in front of the DM range (run on the GPU box, alone or under
`rocprofv3 --kernel-trace --stats -- <python> tools/rfi_profile.py`): 10 s x 1024 channels of 8-bit rows, one warm-up call and then
five frbch_rfi_clean_device calls (default parameters, one dead channel in the rows: statistics, download, the host decision,
upload of the mask, apply) and five
frbch_dedisperse_device calls over 64 DMs of the same rows, then the pieces of a clean on their own -- frbch_rfi_stats_device,
frbch_rfi_mask on the host, frbch_rfi_apply_device with one channel and one block masked.  Prints the medians as JSON and, with
an argument, writes them to that file (profiles/rfi_timing.json)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from frb_baseband_amd import _lib, post                      # noqa: E402
from tests import rfi_cases as rc                            # noqa: E402
from tests.hipmem import DeviceBuffer                        # noqa: E402

lib = _lib.load()
rng = np.random.default_rng(3)
nrows, nchan = rc.TIMING_ROWS, rc.TIMING_NCHAN
data = rng.integers(100, 156, size=(nrows, nchan), dtype=np.uint8)
data[:, rc.TIMING_DEAD_CHANNEL] = rc.TIMING_DEAD_CODE         # one dead channel: every clean flags it, uploads the mask and applies
d_rows = DeviceBuffer.from_numpy(data)


def to_ms(v):
    return [round(1e3 * x, 3) for x in v] if isinstance(v, list) else round(1e3 * v, 3)


def in_ms(out):
    return {(k[:-2] + "_ms" if k.endswith("_s") else k): (to_ms(v) if k.endswith("_s") else v) for k, v in out.items()}


if "--periodic" in sys.argv[1:]:
    # the periodicity test on the same rows (blocks of 1024): the median of five frbch_rfi_peaks_device calls with the fast kernel,
    # with the generic one (the rows one byte further on), of frbch_rfi_stats_device, and of frbch_rfi_cleanf_device against
    # frbch_rfi_clean_device; `tools/rfi_profile.py --periodic [profiles/rfi_periodic_timing.json]`
    from tests import rfi_periodic_cases as pc               # noqa: E402
    out = in_ms(pc.timing_run(lib, d_rows.ptr.value))
    out["rows_bytes"] = int(data.nbytes)
    print(json.dumps(out))
    paths = [a for a in sys.argv[1:] if a != "--periodic"]
    if paths:
        with open(paths[0], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    raise SystemExit(0)

out = in_ms(rc.timing_run(lib, d_rows.ptr.value))

desc = post.fil_desc(rc.TIMING_HDR)
par = rc.params()
nblk = out["nblk"]
err = C.create_string_buffer(256)
used = C.c_uint32(0)
d_stats = DeviceBuffer(nblk * nchan * 16)
stats = np.zeros((nblk, nchan, 2), np.uint64)
mask, repl = np.zeros((nblk, nchan), np.uint8), np.zeros(nchan)
cf, bf = np.zeros(nchan, np.uint8), np.zeros(nblk, np.uint8)


def timed(call, n=5):
    call()
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return round(1e3 * statistics.median(times), 3)


def stats_device():
    assert lib.frbch_rfi_stats_device(C.byref(desc), d_rows.ptr, nrows, C.byref(par), 0, d_stats.ptr, C.byref(used), err, len(err)) == 0, err.value


def mask_host():
    assert lib.frbch_rfi_mask(C.byref(desc), stats.ctypes.data, nblk, nrows, C.byref(par), None, None, mask.ctypes.data, repl.ctypes.data,
                              cf.ctypes.data, bf.ctypes.data, err, len(err)) == 0, err.value


out["rfi_stats_device_median_ms"] = timed(stats_device)
stats[:] = d_stats.to_numpy(np.uint64).reshape(stats.shape)
out["rfi_mask_host_median_ms"] = timed(mask_host)
mask[:, 17] = 1
mask[nblk // 2, :] = 1
d_mask, d_repl = DeviceBuffer.from_numpy(mask), DeviceBuffer.from_numpy(np.full(nchan, 128.0))


def apply_device():
    assert lib.frbch_rfi_apply_device(C.byref(desc), d_rows.ptr, nrows, C.byref(par), d_mask.ptr, d_repl.ptr, 0, err, len(err)) == 0, err.value


out["rfi_apply_device_median_ms"] = timed(apply_device)
out["rows_bytes"] = int(data.nbytes)
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
