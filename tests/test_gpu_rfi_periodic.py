"""GPU tests of the periodicity test of the interference stage (frbch_rfi_peaks_*, frbch_rfi_cleanf_*): the fast kernel
frbch_post_rfi_peaks_fast (both sample widths, every transform length it has a plan for) and the generic kernel it falls back
to, against the numpy restatement tests/rfi_periodic_oracle.py -- peak values and bins to the bit: the operation graph of the
transform is fixed and every operation is rounded on its own, so there is no tolerance anywhere.  Every case asserts
`kernel_used`, against frbch_rfi_peaks_kernel for the same address and against the rule restated in
rfi_periodic_cases.fast_expected.  Device buffers are guarded (tests/hipmem.GuardedBuffer) and of exactly the documented sizes."""
import ctypes as C
import contextlib
import faulthandler

import numpy as np
import pytest

from tests import rfi_cases as rc
from tests import rfi_periodic_cases as pc
from tests.hipmem import GuardedBuffer as DeviceBuffer, hip

pytestmark = pytest.mark.gpu

CALL_LIMIT_S = 120          # a device call that has not come back by then ends the test process (traceback on stderr)


@contextlib.contextmanager
def guarded():
    faulthandler.dump_traceback_later(CALL_LIMIT_S, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def upload(rows, shift):
    """the rows `shift` bytes behind a 16-byte aligned device address, in a buffer of exactly their size (+ 16 when shifted)"""
    if not shift:
        buf = DeviceBuffer.from_numpy(rows)
        assert buf.ptr.value % 16 == 0
        return buf, C.c_void_p(buf.ptr.value)
    buf = DeviceBuffer(rows.nbytes + 16)
    assert buf.ptr.value % 16 == 0
    d_rows = C.c_void_p(buf.ptr.value + shift)
    assert hip().hipMemcpy(d_rows, rows.ctypes.data, rows.nbytes, 1) == 0
    return buf, d_rows


def peaks_on_device(lib, rows, prod, par, shift=0):
    """frbch_rfi_stats_device and frbch_rfi_peaks_device on resident rows -> dict(stats, peaks, used, says, address); the rows and
    the statistics keep their checksums, every guard its pattern"""
    nrows, _nifs, nchan = rows.shape
    desc = rc.desc_of(rows, prod)
    nblk = lib.frbch_rfi_nblk(nrows, par.block_rows)
    buf, d_rows = upload(rows, shift)
    d_stats, d_peaks = DeviceBuffer(nblk * nchan * 16), DeviceBuffer(nblk * nchan * 8)
    used, used_s = C.c_uint32(99), C.c_uint32(99)
    err = C.create_string_buffer(512)
    out = dict(address=d_rows.value, says=lib.frbch_rfi_peaks_kernel(C.byref(desc), d_rows, nrows, C.byref(par)))
    with guarded():
        code = lib.frbch_rfi_stats_device(C.byref(desc), d_rows, nrows, C.byref(par), 0, d_stats.ptr, C.byref(used_s), err, len(err))
    assert code == 0, err.value
    out["stats"] = d_stats.to_numpy(rc.stats_dtype(rows)).reshape(nblk, nchan, 2)
    d_stats.expect(out["stats"])
    with guarded():
        code = lib.frbch_rfi_peaks_device(C.byref(desc), d_rows, nrows, C.byref(par), 0, d_stats.ptr, d_peaks.ptr, C.byref(used), err, len(err))
    assert code == 0, err.value
    out["used"] = used.value
    out["peaks"] = d_peaks.to_numpy(np.uint64).view(pc.PEAK).reshape(nblk, nchan)
    buf.check(contents=True)
    d_stats.check(contents=True)
    for b in (buf, d_stats, d_peaks):
        b.free()
    return out


def check(lib, c, kernel, shift=0):
    nchan, nbits, nifs, prod, n, nrows = c
    rows, st, pk = pc.rows_case(*c)
    got = peaks_on_device(lib, rows, prod, rc.params(block_rows=n), shift=shift)
    assert got["used"] == got["says"] == pc.fast_expected(nchan, nifs, nbits, got["address"], n) == kernel
    assert got["stats"].tobytes() == st.tobytes()
    assert pc.same_peaks(got["peaks"], pk), np.argwhere(got["peaks"] != pk)[:8]
    return got


#             nchan nbits nifs prod  n   nrows
FAST_CASES = [(64, 8, 1, 0, 256, 2 * 256 + 131),              # a ragged last block that is tested (2 x 131 >= 256)
              (128, 16, 3, 2, 256, 3 * 256 - 1),
              (128, 8, 1, 0, 512, 2 * 512 + 300),
              (64, 16, 3, 2, 512, 512 + 255),                 # a last block that is not tested (2 x 255 < 512)
              (64, 16, 1, 0, 1024, 1024 + 700),
              (128, 8, 3, 2, 1024, 2 * 1024 + 100),           # a last block that is not tested
              (64, 8, 3, 2, 2048, 2048 + 1500),
              (128, 16, 1, 0, 2048, 2 * 2048 + 5)]
# the other side of every clause (aligned address unless shifted)
GENERIC_CASES = [((48, 8, 1, 0, 256, 2 * 256 + 131), 0),      # not whole 64-byte tiles
                 ((64, 8, 1, 0, 256, 2 * 256 + 131), 1),      # an address shifted by one byte
                 ((64, 8, 1, 0, 64, 3 * 64 + 40), 0),         # below the fast range
                 ((64, 8, 1, 0, 4096, 4096 + 2100), 0),       # above it
                 ((64, 32, 1, 0, 256, 2 * 256 + 131), 0)]     # float rows


@pytest.mark.parametrize("c", FAST_CASES, ids=pc.grid_id)
def test_fast_kernel_equals_the_restatement(hip_lib, c):
    got = check(hip_lib, c, pc.FAST)
    assert int((got["peaks"]["k"] > 0).sum()) > 0


@pytest.mark.parametrize("c,shift", GENERIC_CASES, ids=[pc.grid_id(c) + "_s%d" % s for c, s in GENERIC_CASES])
def test_the_other_side_of_every_clause(hip_lib, c, shift):
    check(hip_lib, c, pc.GENERIC, shift=shift)


@pytest.mark.parametrize("c", [FAST_CASES[0], FAST_CASES[1], FAST_CASES[4], FAST_CASES[6]], ids=pc.grid_id)
def test_both_kernels_give_the_same_bits(hip_lib, c):
    """the same rows at an aligned address (fast kernel) and one sample behind it (generic)"""
    fast = check(hip_lib, c, pc.FAST)
    slow = check(hip_lib, c, pc.GENERIC, shift=c[1] // 8)
    assert slow["peaks"].tobytes() == fast["peaks"].tobytes() and slow["stats"].tobytes() == fast["stats"].tobytes()


def cleanf_on_device(lib, rows, prod, par, fpar, zap=None):
    """frbch_rfi_cleanf_device on resident rows in a guarded buffer of exactly their size -> (dict as pc.cleanf_host's, rows, used)"""
    nrows, _nifs, nchan = rows.shape
    nblk = lib.frbch_rfi_nblk(nrows, par.block_rows)
    buf, d_rows = upload(rows, 0)
    z = None if zap is None else np.ascontiguousarray(zap, dtype=np.uint8)
    m, repl = np.full((nblk, nchan), 9, np.uint8), np.full(nchan, -1.0)
    cf, bf = np.full(nchan, 9, np.uint8), np.full(nblk, 9, np.uint8)
    pflag, pchan = np.full((nblk, nchan), 9, np.uint8), np.full(nchan, 9, np.uint8)
    pk = np.full((nblk, nchan), 7, dtype=np.uint64).view(pc.PEAK)
    used = (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    with guarded():
        code = lib.frbch_rfi_cleanf_device(C.byref(rc.desc_of(rows, prod)), d_rows, nrows, C.byref(par), C.byref(fpar),
                                           None if z is None else z.ctypes.data, 0, m.ctypes.data, repl.ctypes.data, cf.ctypes.data,
                                           bf.ctypes.data, pflag.ctypes.data, pchan.ctypes.data, pk.ctypes.data, used, err, len(err))
    assert code == 0, err.value
    back = buf.to_numpy(rows.dtype).reshape(rows.shape)
    buf.free()
    return dict(mask=m, repl=repl, chan_flag=cf.astype(bool), blk_flag=bf.astype(bool), pflag=pflag, pchan=pchan.astype(bool), peaks=pk), back, (used[0], used[1])


@pytest.mark.parametrize("all_blocks", [False, True])
def test_known_answer_on_the_device(hip_lib, all_blocks):
    """the 0.7 sigma tone of period 8 rows: the four cells and nothing else, k = 32; in every block: the channel, wholly"""
    q = np.ascontiguousarray(pc.known_answer_rows(0, all_blocks)[:, None, :])
    par = rc.params(block_rows=rc.KA_BLOCK)
    want, cleaned = pc.sequence_of_parts(q, 0, rc.KA_BLOCK, 8, rc.rule_kw(rc.DEFAULTS), pc.ka_t_pow(), 0.3)
    got, back, used = cleanf_on_device(hip_lib, q, 0, par, pc.fparams(pc.ka_t_pow()))
    assert used == (rc.FAST, pc.FAST)
    assert pc.same_cleanf(got, want) and back.tobytes() == cleaned.tobytes()
    ch = pc.KA_TONE["channel"]
    cells = [(b, ch) for b in pc.KA_TONE["blocks"]]
    if not all_blocks:
        assert [tuple(v) for v in np.argwhere(got["pflag"]).tolist()] == cells and not got["pchan"].any()
    else:
        assert got["pchan"][pc.KA_ALL_CHANNEL] and got["chan_flag"][pc.KA_ALL_CHANNEL] and got["pflag"][:, pc.KA_ALL_CHANNEL].all()
        assert all(got["pflag"][b, c] for b, c in cells) and int(got["pchan"].sum()) == 1
    assert all(int(got["peaks"]["k"][b, c]) == rc.KA_BLOCK // pc.KA_TONE["period"] for b, c in cells)


@pytest.mark.parametrize("c", [FAST_CASES[5], GENERIC_CASES[0][0], GENERIC_CASES[4][0]], ids=pc.grid_id)
def test_cleanf_host_is_cleanf_device_and_a_download(hip_lib, c):
    nchan, nbits, nifs, prod, n, nrows = c
    rows, _st, _pk = pc.rows_case(*c)
    par = rc.params(block_rows=n, t_cell=3.0)
    fpar = pc.fparams(8.0, 0.5)
    want, cleaned = pc.sequence_of_parts(rows, prod, n, nbits, dict(rc.rule_kw(rc.DEFAULTS), t_cell=3.0), 8.0, 0.5)
    dev, back, used = cleanf_on_device(hip_lib, rows, prod, par, fpar)
    assert pc.same_cleanf(dev, want) and back.tobytes() == cleaned.tobytes()
    assert 0 < int(dev["pflag"].sum()) < dev["pflag"].size
    with guarded():
        code, out, res, used_h, msg = pc.cleanf_host(hip_lib, rows, prod, par, fpar)
    assert code == 0, msg
    assert used_h == used and pc.same_cleanf(res, dev) and out.tobytes() == back.tobytes()
    with guarded():
        code, pk, st, used_p, msg = pc.peaks_host(hip_lib, rows, prod, par)
    assert code == 0 and used_p == used and pc.same_peaks(pk, dev["peaks"]) and st.tobytes() == want["stats"].tobytes(), msg
