"""Shared case builder of the layout / shape tests of the stages behind the filterbank (tests/test_post_shapes.py on the
emulator, tests/test_gpu_post_shapes.py on the device).  A plain module: rows whose products all differ, headers with
`foff` of either sign, thin callers of the C ABI that take a product, and the expected values -- which are nothing but
oracle/post_oracle.py and tests/fold_model_oracle.py applied to ONE product of the rows (no restatement here)."""
import ctypes as C

import numpy as np

from frb_baseband_amd import post
from oracle import post_oracle as po
from tests import fold_model_oracle as fo

P0, DM0 = 0.0334, 56.7
F0 = 1.0 / P0
TSTART = 59000.25
PAR = dict(F0=F0, F1=-2.5e-9, PEPOCH=TSTART - 300.0, DM=DM0, PSR="J0000+00")
DTYPES = {8: np.uint8, 16: np.uint16, 32: np.float32}


def make_hdr(nchan, foff_sign=-1, tsamp=32e-6, bw=32.0, ftop=1416.0):
    """SIGPROC header of `nchan` channels over [ftop - bw, ftop] MHz.  foff < 0: fch1 is the centre of the top channel (as the
    channeliser writes it); foff > 0: fch1 is the centre of the BOTTOM channel of the same band."""
    step = bw / nchan
    fch1 = ftop - 0.5 * step if foff_sign < 0 else ftop - bw + 0.5 * step
    return dict(nchans=nchan, nifs=1, nbits=8, fch1=fch1, foff=-step if foff_sign < 0 else step, tsamp=tsamp, tstart=TSTART,
                source_name="J0000+00", src_raj=12345.6, src_dej=-123456.7)


def burst_rows(nrows, prod):
    """the rows of product `prod`'s broadband burst"""
    start = int(nrows * (0.29 + 0.13 * prod))
    return np.arange(start, min(nrows, start + 3 + prod))


def make_rows(nrows, nifs, nchan, nbits, seed=3, hdr=None):
    """[t][nifs][nchan] rows in which every product is DIFFERENT: its own noise seed, floor and width, its own dispersed
    pulse train (its own period and amplitude; the delays of `hdr`, so of its `foff` sign) and its own broadband burst of
    3 + p rows at its own row indices -- a kernel that reads another product meets other clip flags, another nclip and
    other sums.  8 bit: codes <= 222; 16 bit: the same x 201; 32: the same x 0.37 - 3 as float32."""
    hdr = hdr or make_hdr(nchan)
    dly = po.delays_seconds(hdr["fch1"], hdr["foff"], nchan, DM0)
    chans = np.arange(nchan)
    x = np.empty((nrows, nifs, nchan), dtype=np.float64)
    for p in range(nifs):
        rng = np.random.default_rng(1000 * seed + p)
        x[:, p, :] = rng.integers(40 + 15 * p, 40 + 15 * p + 24 + 8 * p, size=(nrows, nchan))
        period, k = P0 * (1.0 + 0.13 * p), 0
        while (k + 0.254 + 0.1 * p) * period < nrows * hdr["tsamp"]:
            i = np.rint(((k + 0.254 + 0.1 * p) * period + dly) / hdr["tsamp"]).astype(np.int64)
            ok = i < nrows
            x[i[ok], p, chans[ok]] += 25 + 5 * p
            k += 1
        x[burst_rows(nrows, p), p, :] += 50
    if nbits == 8:
        return x.astype(np.uint8)
    if nbits == 16:
        return (x * 201).astype(np.uint16)
    return (x * 0.37 - 3.0).astype(np.float32)


def desc_of(hdr, rows, prod=0):
    nbits = rows.dtype.itemsize * 8
    return post.fil_desc(dict(hdr, nifs=rows.shape[1], nbits=nbits), product=prod)


def model_kw(hdr):
    return dict(fch1=hdr["fch1"], foff=hdr["foff"], tsamp=hdr["tsamp"], tstart_mjd=hdr["tstart"])


# ---- expected values: the oracles on one product --------------------------------------------------------------------
def want_dedisp(rows, hdr, prod, dms, zerodm, clip):
    return po.dedisperse(rows[:, prod, :], fch1=hdr["fch1"], foff=hdr["foff"], tsamp=hdr["tsamp"], dms=list(dms), zerodm=zerodm,
                         clip=clip, integer=rows.dtype != np.float32)


def want_fold(rows, hdr, prod, par, nbin, subint_s, apply_delays):
    return po.fold(rows[:, prod, :], fch1=hdr["fch1"], foff=hdr["foff"], tsamp=hdr["tsamp"], tstart_mjd=hdr["tstart"], f0=par["F0"],
                   f1=par["F1"], pepoch_mjd=par["PEPOCH"] if par["PEPOCH"] is not None else hdr["tstart"], dm=par["DM"], nbin=nbin,
                   subint_s=subint_s, apply_delays=apply_delays)


def want_fold_all(rows, hdr, par, nbin, subint_s, apply_delays=False, segs=None, doppler=0.0):
    if segs:
        return fo.fold_all(rows, nbin=nbin, subint_s=subint_s, dm=par["DM"], apply_delays=apply_delays, segs=segs, **model_kw(hdr))
    return fo.fold_all(rows, nbin=nbin, subint_s=subint_s, dm=par["DM"], apply_delays=apply_delays, f0=par["F0"], f1=par["F1"],
                       pepoch_mjd=par["PEPOCH"], doppler=doppler, **model_kw(hdr))


def polyco_blocks(hdr, nrows):
    """three polyco blocks with both boundaries inside `nrows` rows and 1/8 of a row (at least 1 us: an MJD double
    resolves about that) away from every row time"""
    ts = hdr["tsamp"]
    offs = [round(nrows * f) * ts + 0.375 * ts for f in (0.15, 0.5, 0.85)]
    coeffs = [[0.11, 0.53, -0.31, 2.1], [0.42, -0.77, 0.25], [0.05, 0.9, 0.6, -1.4, 3.0]]
    segs = [dict(tmid=hdr["tstart"] + off / 86400.0, rphase=0.1 + 0.27 * k, f0=F0 * (1.0 + 1e-5 * k), span=1.0, coeff=coeffs[k],
                 site="g") for k, off in enumerate(offs)]
    first = fo.block_first_rows(segs, hdr["tstart"], ts, nrows)
    assert 0 < first[1] < first[2] < nrows
    for a, b in zip(segs[:-1], segs[1:]):
        x = (0.5 * (a["tmid"] + b["tmid"]) - hdr["tstart"]) * 86400.0
        assert abs(x / ts - round(x / ts)) * ts > 1e-6
    return segs


# ---- callers of the C ABI that take a product -----------------------------------------------------------------------
def dedisp_nout(lib, hdr, rows, prod, dms):
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    return lib.frbch_dedisperse_nout(C.byref(desc_of(hdr, rows, prod)), rows.shape[0], dm_arr.ctypes.data, dm_arr.size)


def dedisp_kernel(lib, hdr, rows, prod, dms, address):
    """frbch_dedisperse_kernel for rows at `address` (only the address is examined)"""
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    return lib.frbch_dedisperse_kernel(C.byref(desc_of(hdr, rows, prod)), C.c_void_p(address), rows.shape[0], dm_arr.ctypes.data,
                                       dm_arr.size)


def dedisp_host(lib, hdr, rows, prod, dms, zerodm, clip, nout):
    """frbch_dedisperse_host on product `prod`.  `nout` is the ORACLE's: a library that disagrees about the delays is
    caught here, before any kernel indexes the rows with them."""
    assert dedisp_nout(lib, hdr, rows, prod, dms) == nout
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    out = np.empty((dm_arr.size, nout), dtype=np.float32)
    nclip = C.c_uint64(0)
    err = C.create_string_buffer(512)
    rc = lib.frbch_dedisperse_host(C.byref(desc_of(hdr, rows, prod)), rows.ctypes.data, rows.shape[0], dm_arr.ctypes.data,
                                   dm_arr.size, 1 if zerodm else 0, float(clip), 0, out.ctypes.data, nout, C.byref(nclip), err,
                                   len(err))
    assert rc == 0, err.value
    return out, nclip.value


def fold_host(lib, hdr, rows, prod, par, nbin, subint_s, apply_delays):
    """frbch_fold_host on product `prod` -> (sums [nsub][nchan][nbin], hits), the oracle's axes"""
    desc = desc_of(hdr, rows, prod)
    nsub = lib.frbch_fold_nsub(C.byref(desc), rows.shape[0], float(subint_s))
    assert nsub > 0
    prof = np.zeros((nsub, nbin, desc.nchan), dtype=np.float64)
    hits = np.zeros((nsub, nbin, desc.nchan), dtype=np.uint32)
    err = C.create_string_buffer(512)
    pepoch = par["PEPOCH"] if par["PEPOCH"] is not None else hdr["tstart"]
    rc = lib.frbch_fold_host(C.byref(desc), rows.ctypes.data, rows.shape[0], par["F0"], par["F1"], pepoch, par["DM"],
                             1 if apply_delays else 0, nbin, float(subint_s), 0, prof.ctypes.data, hits.ctypes.data, nsub, err,
                             len(err))
    assert rc == 0, err.value
    return prof.transpose(0, 2, 1), hits.transpose(0, 2, 1)


def fold_all(lib, hdr, rows, par, nbin, subint_s, apply_delays=False, segs=None, doppler=0.0):
    """post.fold_all -> (sums [nsub][nifs][nchan][nbin], hits [nsub][nchan][nbin], kernel_used)"""
    from frb_baseband_amd import sigproc
    fil = sigproc.SigprocFile(header=dict(hdr, nifs=rows.shape[1], nbits=rows.dtype.itemsize * 8), header_bytes=0, data=rows)
    info = {}
    prof, hits, _ = post.fold_all(fil, par, polyco=segs, doppler=doppler, nbin=nbin, subint_s=subint_s, apply_delays=apply_delays,
                                  lib=lib, info=info)
    return prof, hits, info["kernel_used"]


def check_fold(rows, prof, hits, wp, wh):
    """integer rows: equal to the bit; float rows: rtol 1e-12 (atomics in any order)"""
    assert prof.shape == wp.shape and hits.shape == wh.shape
    assert np.array_equal(hits, wh)
    if rows.dtype == np.float32:
        np.testing.assert_allclose(prof, wp, rtol=1e-12)
    else:
        assert np.array_equal(prof, wp)
