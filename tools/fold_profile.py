#!/usr/bin/env python3
"""Device-resident runs of the all-product fold for `rocprofv3 --kernel-trace --stats` (run on the GPU box): 10 s x 4 products x
1024 channels of 8-bit rows (1.28 GB) through frbch_foldp_device at 256 / 512 / 1024 bins, and the four single-product
frbch_fold_device calls the 512-bin call replaces.  Prints the bytes of rows so that GB/s follow from the profiler's durations."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from frb_baseband_amd import _lib, post                      # noqa: E402
from tests.hipmem import DeviceBuffer                        # noqa: E402

lib = _lib.load()
rng = np.random.default_rng(3)
nrows, nifs, nchan = 312500, 4, 1024
hdr = dict(nchans=nchan, nifs=nifs, nbits=8, fch1=1416.0 - 0.015625, foff=-0.03125, tsamp=32e-6, tstart=59000.0)
data = rng.integers(100, 156, size=(nrows, nifs, nchan), dtype=np.uint8)
d_rows = DeviceBuffer.from_numpy(data)
err = C.create_string_buffer(256)
par = dict(F0=1.0 / 0.0334, F1=0.0, PEPOCH=58999.0, DM=56.7, PSR="x")
d_prof = DeviceBuffer(1024 * nchan * nifs * 8)
d_hits = DeviceBuffer(1024 * nchan * 4)
used = C.c_uint32(0)
out = {"rows_bytes": int(data.nbytes), "foldp": []}
for nbin in (512, 256, 1024):
    model, _keep = post.fold_model(par, hdr, nbin=nbin, subint_s=10.0, apply_delays=False)
    for _ in range(5):
        assert lib.frbch_foldp_device(C.byref(post.fil_desc(hdr)), d_rows.ptr, nrows, C.byref(model), 0, d_prof.ptr, d_hits.ptr, 1,
                                      C.byref(used), err, len(err)) == 0, err.value
    out["foldp"].append({"nbin": nbin, "kernel_used": used.value, "calls": 5})
for p in range(nifs):
    assert lib.frbch_fold_device(C.byref(post.fil_desc(hdr, product=p)), d_rows.ptr, nrows, par["F0"], 0.0, par["PEPOCH"], par["DM"], 0, 512,
                                 10.0, 0, d_prof.ptr, d_hits.ptr, 1, err, len(err)) == 0, err.value
out["fold_single_product_calls"] = nifs
print(json.dumps(out))
