#!/usr/bin/env python3
"""Device-resident run of the candidate cut-outs (run on the GPU box, alone or under
`rocprofv3 --kernel-trace --stats -- <python> tools/cutout_profile.py`): 10 s x 1024 channels of 8-bit rows, 32 candidates with
tfactor 1 .. 15 at DMs 300 .. 331, nt = ndm = 256 -- one warm-up, then the median of five frbch_cutout_device calls for all 32
against the median of five rounds of 32 frbch_dedisperse_device calls on the candidates' row windows (the shape of
tests/cutout_cases.timing_run, which the GPU suite asserts on).  Prints the pair as JSON and, with an argument, writes it to
that file (profiles/cutout_timing.json)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from frb_baseband_amd import _lib                            # noqa: E402
from tests import cutout_cases as cc                         # noqa: E402
from tests.hipmem import DeviceBuffer                        # noqa: E402

lib = _lib.load()
rng = np.random.default_rng(5)
data = rng.integers(100, 156, size=(cc.TIMING_ROWS, cc.TIMING_HDR["nchans"]), dtype=np.uint8)
d_rows = DeviceBuffer.from_numpy(data)
out = cc.timing_run(lib, d_rows.ptr.value)
out = {k: (round(1e3 * v, 3) if k.endswith("_s") else v) for k, v in out.items()}
out = {(k[:-2] + "_ms" if k.endswith("_s") else k): v for k, v in out.items()}
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
