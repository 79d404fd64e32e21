"""GPU tests of the resident rows (frbch_candidates_host / _device, frbch_rfi_cleanp_*, post.*(resident=True)): every array of the
result view against the sequence of existing calls it replaces (tests/resident_cases.sequence), run through the same library on
the same device -- `==` on bytes, no tolerance anywhere -- and `kernel_used` of the four stages against frbch_rfi_stats_kernel,
frbch_dedisperse_kernel and frbch_cutout_kernel for the address the stage read."""
import contextlib
import ctypes as C
import faulthandler
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import resident_cases as rs
from tests import rfi_cases as rc
from tests.hipmem import POISON, GuardedBuffer, hip
from tests.test_fold_predictor import write_fil
from tests.test_post import DM0
from tests.test_spsearch import dispersed_burst_rows

pytestmark = pytest.mark.gpu

CALL_LIMIT_S = 120          # a device call that has not come back by then ends the test process (traceback on stderr)
ALIGNED = 0x7F0000000000    # an address as hipMalloc gives them: the kernel queries look at nothing but the address
ZAP = [rs.ZAP_CHANNEL]
LDS, GENERIC = 1, 0


@contextlib.contextmanager
def guarded():
    faulthandler.dump_traceback_later(CALL_LIMIT_S, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def kernels_said(lib, rows, hdr, s, got, stats_address, rows_address):
    """what the three queries say for the addresses the stages read: [RFI statistics, dedispersion, cut-out] (0 where the stage
    does not run)"""
    desc = post.fil_desc(hdr, s["product"])
    dm_arr = np.ascontiguousarray(s["dms"], dtype=np.float64)
    said = [0, lib.frbch_dedisperse_kernel(C.byref(desc), C.c_void_p(rows_address), rows.shape[0], dm_arr.ctypes.data, dm_arr.size), 0]
    if s["rfi"] is not None:
        par = post.rfi_params(s["rfi"])
        said[0] = lib.frbch_rfi_stats_kernel(C.byref(desc), C.c_void_p(stats_address), rows.shape[0], C.byref(par))
    if s["nt"] and got["groups"].size:
        cut = _lib.FrbchCutoutParams(C.sizeof(_lib.FrbchCutoutParams), s["nt"], s["nf"], s["ndm"])
        cc = np.ascontiguousarray(got["cut_cands"][:1024])
        said[2] = lib.frbch_cutout_kernel(C.byref(desc), C.c_void_p(rows_address), rows.shape[0], C.byref(cut), cc.ctypes.data, cc.size)
    assert min(said) >= 0, said
    return said


def run_both(lib, rows, hdr, s):
    with guarded():
        want = rs.sequence(lib, rows, hdr, s)
    with guarded():
        got = rs.resident(lib, rows, hdr, s)
    assert rs.differences(got, want) == []
    assert got["row_uploads"] == 1
    said = kernels_said(lib, rows, hdr, s, got, ALIGNED, ALIGNED)
    assert got["kernel_used"] == [said[0], said[1], want["search_kernel"], said[2]]
    if "cutout_kernel" in want:
        assert got["kernel_used"][3] == want["cutout_kernel"]
    return want, got


# ---- 1. the burst case, and the shape that reaches the tiled dedispersion, the LDS search and the LDS cut-out ---------------
def test_the_burst_case_equals_the_sequence(hip_lib):
    rows, hdr = rs.burst_rows()
    _want, got = run_both(hip_lib, rows, hdr, rs.settings(keep_series=True))
    assert got["cands"].size == 9 and got["groups"].size == 1 and got["cutout_calls"] == 1
    assert all(t > 0 for k, t in got["device_ms"].items() if k != "flag") and got["device_ms"]["flag"] == 0


def test_1024_channels_take_the_three_fast_kernels(hip_lib):
    hdr = dict(rs.hdr_of(nchan=1024), fch1=1416.0 - 0.015625, foff=-0.03125, tsamp=32e-6)
    x = dispersed_burst_rows(20000, hdr, 307.0, 9000, 5, 12, seed=3)
    rows = np.ascontiguousarray(x[:, None, :])
    s = rs.settings(dms=post.dm_list(300.0, 315.0, 1.0), rfi=dict(block_rows=1024), nt=64, nf=256, ndm=64)
    _want, got = run_both(hip_lib, rows, hdr, s)
    assert got["kernel_used"] == [1, LDS, LDS, LDS]
    assert got["groups"].size >= 1 and int(got["groups"]["nmember"].max()) >= 3


# ---- 2. interference: the apply writes ------------------------------------------------------------------------------------
CASES = dict(b8=dict(nbits=8), b16=dict(nbits=16), float=dict(nbits=32), nifs2_product1=dict(nifs=2, product=1), foff_positive=dict(foff_sign=+1))


def interference_case(name):
    case = CASES[name]
    rows, hdr = rs.burst_rows(interference=True, **case)
    return rows, hdr, rs.settings(rfi=rs.RFI, zap=ZAP, product=case.get("product", 0), dm_span=30.0 if "foff_sign" in case else None)


@pytest.mark.parametrize("name", list(CASES))
def test_interference_equals_the_sequence(hip_lib, name):
    rows, hdr, s = interference_case(name)
    want, got = run_both(hip_lib, rows, hdr, s)
    assert not np.array_equal(want["cleaned"], rows)                                   # the apply really wrote
    assert got["chan_flag"].nonzero()[0].tolist() == [rs.DEAD_CHANNEL, rs.ZAP_CHANNEL] and not got["blk_flag"].any()
    assert got["mask"][:, rs.LOUD_CHANNEL].nonzero()[0].tolist() == [5] and got["mask"].sum() == 2 * got["nblk"] + 1
    assert got["groups"].size >= 1 and got["ft"] is not None


# ---- 5. two cut-out batches ------------------------------------------------------------------------------------------------
def test_two_cutout_batches(hip_lib):
    """the case of tests/test_candidates_resident.py: 1466 groups, 1024 candidates a call"""
    rows, hdr = rs.crowded_rows()
    s = rs.settings(dms=[10.0], threshold=1.0, widths=[1], nt=2, nf=64, ndm=1024, zerodm=False, clip=0.0)
    want, got = run_both(hip_lib, rows, hdr, s)
    assert want["groups"].size == 1466 and got["cutout_calls"] == want["cutout_calls"] == 2


# ---- 6. rows that are on the device already --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b8", "b16", "nifs2_product1"])
def test_device_rows_keep_every_byte(hip_lib, name):
    rows, hdr, s = interference_case(name)
    with guarded():
        want = rs.sequence(hip_lib, rows, hdr, s)
    buf = GuardedBuffer.from_numpy(rows)                                               # exactly the documented size
    assert buf.nbytes == rows.nbytes and buf.ptr.value % 16 == 0
    with guarded():
        got = rs.resident(hip_lib, rows, hdr, s, d_rows=buf.ptr.value)
    buf.check(contents=True)                                                           # the guards, and the checksum of the upload
    assert buf.to_numpy(rows.dtype).tobytes() == rows.tobytes()
    assert rs.differences(got, want) == [] and got["row_uploads"] == 0 and got["wall_ms"]["upload"] == 0
    said = kernels_said(hip_lib, rows, hdr, s, got, buf.ptr.value, ALIGNED)            # a cell is masked: the stages read the library's copy
    assert got["kernel_used"] == [said[0], said[1], want["search_kernel"], said[2]]
    buf.free()


def test_device_rows_four_bytes_off_alignment(hip_lib):
    rows, hdr, s = interference_case("b8")
    with guarded():
        want = rs.sequence(hip_lib, rows, hdr, s)
        plain = rs.sequence(hip_lib, rows, hdr, rs.settings())
    buf = GuardedBuffer(rows.nbytes + 16)
    address = buf.ptr.value + 4
    assert buf.ptr.value % 16 == 0 and hip().hipMemcpy(C.c_void_p(address), rows.ctypes.data, rows.nbytes, 1) == 0
    with guarded():
        got = rs.resident(hip_lib, rows, hdr, s, d_rows=address)
    assert rs.differences(got, want) == [] and got["row_uploads"] == 0
    assert got["kernel_used"][0] == GENERIC == kernels_said(hip_lib, rows, hdr, s, got, address, ALIGNED)[0]
    with guarded():
        got = rs.resident(hip_lib, rows, hdr, rs.settings(), d_rows=address)           # no flagging: every stage reads the caller's rows
    assert rs.differences(got, plain) == []
    assert got["kernel_used"] == [0, GENERIC, plain["search_kernel"], GENERIC]
    assert kernels_said(hip_lib, rows, hdr, rs.settings(), got, address, address) == [0, GENERIC, GENERIC]
    back = buf.to_numpy(np.uint8)
    assert back[4:4 + rows.nbytes].tobytes() == rows.tobytes() and (back[:4] == POISON).all() and (back[4 + rows.nbytes:] == POISON).all()
    buf.free()


# ---- 7. all products in one residency ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nifs,nbits,nchan,nrows", [(2, 8, 64, 24 * 256 - 100), (4, 8, 128, 2100), (4, 16, 64, 1025), (2, 32, 64, 1500), (1, 8, 64, 1500)])
def test_cleanp_equals_clean(hip_lib, nifs, nbits, nchan, nrows):
    rows = rc.make_rows(nrows, nifs, nchan, nbits, seed=nifs + nbits)
    hdr = rc.hdr_of(nchan, nifs, nbits)
    par = dict(block_rows=256, t_cell=3.0)
    with guarded():
        want_rows, want = post.clean(rows, hdr, par, zap=[3], lib=hip_lib)
        stats = np.stack([post.rfi_stats(rows, hdr, par, product=p, lib=hip_lib) for p in range(nifs)])
    info = {}
    with guarded():
        got_rows, got = post.cleanp(rows, hdr, par, zap=[3], lib=hip_lib, info=info, want_stats=True)
    assert got_rows.tobytes() == want_rows.tobytes() and got_rows.tobytes() != rows.tobytes()
    assert got["stats"].dtype == stats.dtype and got["stats"].tobytes() == stats.tobytes()
    for k in ("mask", "repl", "chan_flag", "blk_flag"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    assert info["kernel_used"] == rc.fast_expected(nchan, nifs, nbits, ALIGNED)
    # the _device form, in place, in a buffer of exactly the rows
    buf = GuardedBuffer.from_numpy(rows)
    nblk = want["mask"].shape[0]
    m, repl = np.zeros((nblk, nchan), np.uint8), np.zeros((nifs, nchan))
    cf, bf = np.zeros(nchan, np.uint8), np.zeros(nblk, np.uint8)
    z = post._zap_array([3], nchan)
    used = C.c_uint32(9)
    err = C.create_string_buffer(512)
    desc, p = post.fil_desc(hdr), post.rfi_params(par)
    with guarded():
        code = hip_lib.frbch_rfi_cleanp_device(C.byref(desc), buf.ptr, nrows, C.byref(p), z.ctypes.data, 0, m.ctypes.data, repl.ctypes.data,
                                               cf.ctypes.data, bf.ctypes.data, None, C.byref(used), err, len(err))
    assert code == 0, err.value
    assert buf.to_numpy(rows.dtype).tobytes() == want_rows.tobytes() and m.tobytes() == want["mask"].tobytes() and repl.tobytes() == want["repl"].tobytes()
    assert used.value == rc.fast_expected(nchan, nifs, nbits, buf.ptr.value)
    buf.free()


# ---- 8. the commands, once ---------------------------------------------------------------------------------------------------
def test_the_commands_write_the_same_files(hip_lib, tmp_path):
    rows, hdr = rs.burst_rows(interference=True)
    infos = {}

    def run(d, resident):
        path = os.path.join(d, "burst.fil")
        write_fil(path, rows, hdr, 1)
        infos[resident] = [{}, {}, {}]
        kw = dict(dm2=DM0 + 20.0, dmstep=5.0, threshold=6.0, lib=hip_lib, rfi=dict(rs.RFI), resident=resident)
        with guarded():
            files, groups = post.candidates_fil(path, DM0 - 20.0, nt=32, nf=16, ndm=16, info=infos[resident][0], **kw)
            _files, cands = post.search_fil(path, DM0 - 20.0, write_dat=True, info=infos[resident][1], **kw)
        four = os.path.join(d, "four.fil")
        write_fil(four, rc.make_rows(2100, 4, 64, 8, seed=9), rc.hdr_of(64, 4, 8), 4)
        with guarded():
            _f, res = post.rfifind_fil(four, block_rows=256, t_cell=3.0, write_clean=True, lib=hip_lib, info=infos[resident][2], resident=resident)
        return groups, cands, res
    names, off, on = rs.commands_round_trip(hip_lib, tmp_path, run)
    assert off[0].tobytes() == on[0].tobytes() and off[1].tobytes() == on[1].tobytes() and on[0].size >= 1
    assert all(off[2][k].tobytes() == on[2][k].tobytes() for k in off[2])
    assert [i["row_uploads"] for i in infos[True]] == [1, 1, 1]
    assert sum(n.endswith(".png") for n in names) == on[0].size and "four_clean.fil" in names and sum(n.endswith(".dat") for n in names) == 9
