"""Shared cases of the resident-rows tests (tests/test_candidates_resident.py on the emulator, tests/test_gpu_candidates_resident.py
on the device): rows, the sequence of existing calls that frbch_candidates_* must reproduce (include/frbch.h), run through the SAME
library, and the comparison -- `==` on bytes, no tolerance anywhere."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import _lib, post
from tests.test_post import DM0, HDR
from tests.test_spsearch import dispersed_burst_rows

BURST_DMS = post.dm_list(DM0 - 20.0, DM0 + 20.0, 5.0)            # the 9 DMs of tests/test_cutout.py
DEAD_CHANNEL, ZAP_CHANNEL, LOUD_CHANNEL, LOUD_ROWS = 20, 41, 50, (5 * 256 + 30, 5 * 256 + 200)
RFI = dict(block_rows=256)
ARRAYS = ("cands", "groups", "cut_cands", "ft", "ft_hits", "dt", "dt_hits", "mask", "repl", "chan_flag", "blk_flag", "series")


def hdr_of(nbits=8, nifs=1, foff_sign=-1, nchan=64):
    h = dict(HDR, nbits=nbits, nifs=nifs, nchans=nchan)
    if foff_sign > 0:
        h.update(fch1=HDR["fch1"] + (nchan - 1) * HDR["foff"], foff=-HDR["foff"])
    return h


def as_bits(x, nbits):
    """8-bit codes -> the same signal as 16-bit codes or floats"""
    if nbits == 8:
        return x.astype(np.uint8)
    if nbits == 16:
        return (x.astype(np.int64) * 201).astype(np.uint16)
    return (x.astype(np.float64) * 0.37 - 3.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def burst_rows(nbits=8, nifs=1, product=0, foff_sign=-1, interference=False):
    """[9000][nifs][64]: the burst of tests/test_cutout.py (5 samples at DM0, row 3000) in product `product`, other noise in the
    others; `interference`: a dead channel, a loud narrow-band stretch inside block 5 of 256 rows (and ZAP_CHANNEL is for the
    caller to zap) -> (rows, header), never written to"""
    hdr = hdr_of(nbits, nifs, foff_sign)
    x = dispersed_burst_rows(9000, hdr, DM0, 3000, 5, 30).astype(np.int64)
    if interference:
        x[:, DEAD_CHANNEL] = 100
        x[LOUD_ROWS[0]:LOUD_ROWS[1], LOUD_CHANNEL] += 90
    rows = np.empty((9000, nifs, 64), np.int64)
    for p in range(nifs):
        rows[:, p, :] = x if p == product else np.random.default_rng(70 + p).integers(60, 90, size=x.shape)
    rows = as_bits(np.clip(rows, 0, 255), nbits)
    rows.setflags(write=False)
    return rows, hdr


@functools.lru_cache(maxsize=None)
def many_bursts_rows():
    """six bursts of different strengths and DMs, 1200 rows apart: several groups of several members each"""
    hdr = hdr_of()
    x = np.random.default_rng(5).integers(96, 160, size=(9000, 64)).astype(np.int64)
    for k, (dm, amp) in enumerate([(DM0, 30), (DM0 - 10.0, 18), (DM0 + 10.0, 18), (DM0, 12), (DM0 + 5.0, 25), (DM0 - 5.0, 12)]):
        b = dispersed_burst_rows(9000, hdr, dm, 800 + 1200 * k, 5, amp, seed=5).astype(np.int64)
        x += b - np.random.default_rng(5).integers(96, 160, size=(9000, 64))
    rows = np.clip(x, 0, 255).astype(np.uint8)[:, None, :]
    rows.setflags(write=False)
    return rows, hdr


@functools.lru_cache(maxsize=None)
def crowded_rows():
    """9000 x 64 of 8-bit noise for the two-batch case: one DM, width 1, threshold 1 -> every sample above 1 sigma is a record
    and, with one DM, a group of its own"""
    rows = np.random.default_rng(11).integers(96, 160, size=(9000, 1, 64)).astype(np.uint8)
    rows.setflags(write=False)
    return rows, hdr_of()


def settings(**kw):
    """the arguments of a case: those of the burst case of tests/test_cutout.py unless overridden"""
    s = dict(dms=BURST_DMS, threshold=6.0, widths=None, detrend_len=1000, zerodm=True, clip=5.0, rfi=None, zap=None, dm_gap=2,
             min_members=1, max_cands=0, nt=32, nf=16, ndm=16, dm_span=None, keep_series=False, product=0)
    assert set(kw) <= set(s), set(kw) - set(s)
    s.update(kw)
    return s


def sp_of(s, hdr):
    return post.sp_params(s["widths"] if s["widths"] is not None else post.default_widths(hdr["tsamp"]), s["threshold"], s["detrend_len"])


def zap_of(s, hdr):
    return None if s["zap"] is None else post._zap_array(s["zap"], hdr["nchans"])


def sequence(lib, rows, hdr, s):
    """Steps 1 to 6 of include/frbch.h with the calls that existed before frbch_candidates_*: frbch_rfi_clean_host,
    frbch_dedisperse_search_host, frbch_sp_group_cands, the selection and the cut-out candidates as post.candidates_fil makes
    them, post.cutouts (frbch_cutout_host in batches) -> dict with the keys of post.candidates_resident"""
    out = dict.fromkeys(ARRAYS)
    x = np.array(rows, copy=True)
    nrows, nchan = x.shape[0], hdr["nchans"]
    desc = post.fil_desc(hdr, s["product"])
    err = C.create_string_buffer(512)
    if s["rfi"] is not None or s["zap"] is not None:
        par = post.rfi_params(s["rfi"] if isinstance(s["rfi"], dict) else None)
        nblk = lib.frbch_rfi_nblk(nrows, par.block_rows)
        z = zap_of(s, hdr)
        out.update(mask=np.zeros((nblk, nchan), np.uint8), repl=np.zeros(nchan), chan_flag=np.zeros(nchan, np.uint8),
                   blk_flag=np.zeros(nblk, np.uint8))
        used = C.c_uint32(0)
        rc = lib.frbch_rfi_clean_host(C.byref(desc), x.ctypes.data, nrows, C.byref(par), None if z is None else z.ctypes.data, 0,
                                      out["mask"].ctypes.data, out["repl"].ctypes.data, out["chan_flag"].ctypes.data,
                                      out["blk_flag"].ctypes.data, C.byref(used), err, len(err))
        assert rc == 0, err.value
        out["nblk"] = nblk
    out["cleaned"] = x
    dm_arr = np.ascontiguousarray(s["dms"], dtype=np.float64)
    nout = lib.frbch_dedisperse_nout(C.byref(desc), nrows, dm_arr.ctypes.data, dm_arr.size)
    assert nout > 0
    series = np.zeros((dm_arr.size, nout), np.float32)
    nclip = C.c_uint64(0)
    sp = sp_of(s, hdr)
    out["cands"], out["search_kernel"] = post._sp_call(lambda c, n, nc, u, e, ne: lib.frbch_dedisperse_search_host(
        C.byref(desc), x.ctypes.data, nrows, dm_arr.ctypes.data, dm_arr.size, 1 if s["zerodm"] else 0, float(s["clip"]), C.byref(sp), 0,
        series.ctypes.data, nout, C.byref(nclip), c, n, nc, u, e, ne), 4096)
    out.update(nout=nout, nclipped=nclip.value)
    if s["keep_series"]:
        out["series"] = series
    groups = post.group_candidates(out["cands"], hdr, s["dms"], dm_gap=s["dm_gap"], lib=lib)
    out["ngroup_all"] = int(groups.size)
    groups = groups[groups["nmember"] >= s["min_members"]]
    if s["max_cands"] > 0 and groups.size > s["max_cands"]:
        groups = groups[np.sort(np.argsort(-groups["best"]["sigma"], kind="stable")[:s["max_cands"]])]
    out["groups"] = groups
    out["cut_cands"] = post.cutout_cands(groups["best"], s["dms"], s["dm_span"])
    out["cutout_calls"] = 0
    if s["nt"] and groups.size:
        info = {}
        out["ft"], out["ft_hits"], out["dt"], out["dt_hits"] = post.cutouts(x, dict(hdr, product=s["product"]), out["cut_cands"], nt=s["nt"],
                                                                            nf=s["nf"], ndm=s["ndm"], lib=lib, info=info)
        out["cutout_calls"], out["cutout_kernel"] = info["calls"], info["kernel_used"]
    return out


def resident(lib, rows, hdr, s, d_rows=None):
    """post.candidates_resident with the arguments of a case (frbch_candidates_host, or _device on the rows at `d_rows`)"""
    return post.candidates_resident(None if d_rows is not None else rows, hdr, s["dms"], sp=sp_of(s, hdr), rfi=s["rfi"], zap=s["zap"],
                                    zerodm=s["zerodm"], clip=s["clip"], dm_gap=s["dm_gap"], min_members=s["min_members"],
                                    max_cands=s["max_cands"], nt=s["nt"], nf=s["nf"], ndm=s["ndm"], dm_span=s["dm_span"],
                                    keep_series=s["keep_series"], product=s["product"], lib=lib, d_rows=d_rows, nrows=rows.shape[0])


def differences(got, want):
    """names of the view's arrays and counts that differ from the sequence's (arrays: dtype, shape and bytes)"""
    bad = [k for k in ("nout", "nclipped", "ngroup_all", "cutout_calls") if got[k] != want[k]]
    for k in ARRAYS:
        g, w = got[k], want[k]
        if (g is None) != (w is None):
            bad.append(k + " (one is missing)")
        elif g is not None and (g.dtype.itemsize != w.dtype.itemsize or g.shape != w.shape or g.tobytes() != np.ascontiguousarray(w).tobytes()):
            bad.append(k)
    return bad


def raw_call(lib, rows, hdr, dms, par, device_rows=None, out=True, desc=None):
    """frbch_candidates_host (or _device) as given -> (rc, result pointer value, message); frees a result it got"""
    desc = desc or post.fil_desc(hdr)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    res = C.c_void_p(0xDEAD)
    err = C.create_string_buffer(2048)
    fn = lib.frbch_candidates_host if device_rows is None else lib.frbch_candidates_device
    rc = fn(C.byref(desc), rows.ctypes.data if device_rows is None else device_rows, rows.shape[0], dm_arr.ctypes.data, dm_arr.size,
            None if par is None else C.byref(par), 0, C.byref(res) if out else None, err, len(err))
    got = res.value
    if out and res.value:
        lib.frbch_cand_result_free(res)
    return rc, got, err.value.decode()


def cand_par(hdr, s):
    """the frbch_cand_params of a case"""
    par = _lib.FrbchCandParams()
    par.size = C.sizeof(_lib.FrbchCandParams)
    par.flags = _lib.CAND_RFI if s["rfi"] is not None else 0
    par.rfi = post.rfi_params(s["rfi"] if isinstance(s["rfi"], dict) else None)
    par.zerodm, par.clip_sigma = 1 if s["zerodm"] else 0, s["clip"]
    par.sp = sp_of(s, hdr)
    par.dm_gap, par.min_members, par.max_cands = s["dm_gap"], s["min_members"], s["max_cands"]
    par.cut = _lib.FrbchCutoutParams(C.sizeof(_lib.FrbchCutoutParams), s["nt"], s["nf"], s["ndm"])
    return par


# ---- the three commands, resident off and on, into two directories ---------------------------------------------------------
def same_files(dir_a, dir_b):
    """the two directories hold the same names; text and .png files (and .fil / .dat) the same bytes, .npz files the same arrays"""
    import os
    names = sorted(os.listdir(dir_a))
    assert names == sorted(os.listdir(dir_b)), (names, sorted(os.listdir(dir_b)))
    for n in names:
        a, b = os.path.join(dir_a, n), os.path.join(dir_b, n)
        if n.endswith(".npz"):
            za, zb = np.load(a), np.load(b)
            assert sorted(za.files) == sorted(zb.files), n
            for k in za.files:
                assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes(), (n, k)
        else:
            assert open(a, "rb").read() == open(b, "rb").read(), n
    return names


def commands_round_trip(lib, tmp_path, run):
    """run(directory, resident) writes into `directory` and returns its values -> (names, values off, values on)"""
    import os
    out = []
    for sub, resident in (("off", False), ("on", True)):
        d = str(tmp_path / sub)
        os.makedirs(d)
        out.append(run(d, resident))
    return same_files(str(tmp_path / "off"), str(tmp_path / "on")), out[0], out[1]
