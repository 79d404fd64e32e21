"""GPU tests of the interference stage (frbch_rfi_*): the fast statistics kernel frbch_post_rfi_stats_fast<BPV> (both sample
widths, every tile width), the generic kernels it falls back to and the apply kernel, on the cases of tests/rfi_cases.py against
the numpy restatement tests/rfi_oracle.py -- statistics, mask and cleaned rows to the bit: integer sums are exact, float rows are
summed in the stated order, the decision is one sequence of double operations, so there is no tolerance anywhere.  Every case
asserts `kernel_used`, against frbch_rfi_stats_kernel for the same address and against the rule restated in rfi_cases.fast_expected."""
import ctypes as C
import contextlib
import faulthandler
import functools
import io
import json

import numpy as np
import pytest

from frb_baseband_amd import process_vdif as pv, sigproc, synth
from tests import rfi_cases as rc
from tests import rfi_oracle as ro
from tests.hipmem import GuardedBuffer as DeviceBuffer, hip
from tests.test_rfi import same_stats

pytestmark = pytest.mark.gpu

CALL_LIMIT_S = 120          # a device call that has not come back by then ends the test process (traceback on stderr)


@contextlib.contextmanager
def guarded():
    faulthandler.dump_traceback_later(CALL_LIMIT_S, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def on_device(lib, rows, prod, par, zap=None, shift=0):
    """The whole stage on rows resident `shift` bytes behind a 16-byte aligned device address: frbch_rfi_stats_device, the mask of
    those statistics (frbch_rfi_mask), frbch_rfi_apply_device twice (the second must change nothing), and frbch_rfi_clean_device on
    a second copy -> dict(stats, used, says, address, res, cleaned, cleaned_twice, clean_res, clean_rows, clean_used)"""
    nrows, nifs, nchan = rows.shape
    nbits = rows.dtype.itemsize * 8
    desc = rc.desc_of(rows, prod)
    nblk = lib.frbch_rfi_nblk(nrows, par.block_rows)
    assert nblk == -(-nrows // par.block_rows)
    bufs = [DeviceBuffer(rows.nbytes + 16) for _ in range(2)]
    d_rows = []
    for b in bufs:
        assert b.ptr.value % 16 == 0
        d_rows.append(C.c_void_p(b.ptr.value + shift))
        assert hip().hipMemcpy(d_rows[-1], rows.ctypes.data, rows.nbytes, 1) == 0
    out = dict(address=d_rows[0].value)
    out["says"] = lib.frbch_rfi_stats_kernel(C.byref(desc), d_rows[0], nrows, C.byref(par))
    assert out["says"] == lib.frbch_rfi_stats_kernel(C.byref(desc), d_rows[1], nrows, C.byref(par))
    d_stats = DeviceBuffer(nblk * nchan * 16)
    used = C.c_uint32(99)
    err = C.create_string_buffer(512)
    with guarded():
        code = lib.frbch_rfi_stats_device(C.byref(desc), d_rows[0], nrows, C.byref(par), 0, d_stats.ptr, C.byref(used), err, len(err))
    assert code == 0, err.value
    out["used"] = used.value
    out["stats"] = d_stats.to_numpy(rc.stats_dtype(rows)).reshape(nblk, nchan, 2)
    code, res, msg = rc.mask_call(lib, out["stats"], nrows, nchan, nifs, nbits, prod, par, zap=zap)
    assert code == 0, msg
    out["res"] = res
    d_mask, d_repl = DeviceBuffer.from_numpy(res["mask"]), DeviceBuffer.from_numpy(res["repl"])
    for key in ("cleaned", "cleaned_twice"):
        with guarded():
            code = lib.frbch_rfi_apply_device(C.byref(desc), d_rows[0], nrows, C.byref(par), d_mask.ptr, d_repl.ptr, 0, err, len(err))
        assert code == 0, err.value
        back = np.empty_like(rows)
        assert hip().hipMemcpy(back.ctypes.data, d_rows[0], rows.nbytes, 2) == 0
        out[key] = back
    z = None if zap is None else np.ascontiguousarray(zap, dtype=np.uint8)
    m, repl = np.full((nblk, nchan), 9, np.uint8), np.full(nchan, -1.0)
    cf, bf = np.full(nchan, 9, np.uint8), np.full(nblk, 9, np.uint8)
    with guarded():
        code = lib.frbch_rfi_clean_device(C.byref(desc), d_rows[1], nrows, C.byref(par), None if z is None else z.ctypes.data, 0,
                                          m.ctypes.data, repl.ctypes.data, cf.ctypes.data, bf.ctypes.data, C.byref(used), err, len(err))
    assert code == 0, err.value
    back = np.empty_like(rows)
    assert hip().hipMemcpy(back.ctypes.data, d_rows[1], rows.nbytes, 2) == 0
    out.update(clean_rows=back, clean_used=used.value, clean_res=dict(mask=m, repl=repl, chan_flag=cf.astype(bool), blk_flag=bf.astype(bool)))
    for b in bufs + [d_stats, d_mask, d_repl]:
        b.free()
    return out


def check(lib, rows, prod, par, rule, kernel, zap=None, shift=0, want=None):
    """everything on_device returns against the restatement; -> what on_device returned"""
    nrows, nifs, nchan = rows.shape
    nbits = rows.dtype.itemsize * 8
    got = on_device(lib, rows, prod, par, zap=zap, shift=shift)
    assert got["used"] == got["says"] == got["clean_used"] == rc.fast_expected(nchan, nifs, nbits, got["address"]) == kernel
    if want is None:
        st = ro.stats(rows[:, prod, :], par.block_rows)
        res = ro.mask(st, nrows, par.block_rows, nbits, zap=zap, **rule)
        want = (st, res, ro.apply(rows, prod, par.block_rows, res["mask"], res["repl"]))
    st, res, cleaned = want
    assert same_stats(got["stats"], st)
    assert rc.same_result(got["res"], res) and rc.same_result(got["clean_res"], res)
    assert got["cleaned"].tobytes() == cleaned.tobytes()
    assert got["cleaned_twice"].tobytes() == cleaned.tobytes()
    assert got["clean_rows"].tobytes() == cleaned.tobytes()
    return got


RULE3 = dict(rc.rule_kw(rc.DEFAULTS), t_cell=3.0)


# ---- the grid of the emulator tests ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", rc.grid(), ids=rc.grid_id)
def test_device_equals_the_restatement(hip_lib, g):
    """48 / 64 / 128 channels x 8 / 16 / 32 bits x (one product, product 2 of 3) x blocks of 1, 7, 256 rows and one longer than
    the data, nrows around a multiple of the block: the fast kernel where the rule says so (64 and 128 channels of 8 and 16 bit; 3 x
    48 ... are generic), the generic one elsewhere"""
    nchan, nbits, nifs, prod, br, nrows = g
    rows, st, res, cleaned = rc.grid_case(g)
    kernel = rc.FAST if nbits in (8, 16) and nchan in (64, 128) else rc.GENERIC
    check(hip_lib, rows, prod, rc.params(block_rows=br, t_cell=3.0), RULE3, kernel, want=(st, res, cleaned))


# ---- shapes that reach the fast kernel ------------------------------------------------------------------------------------
#            nchan nbits nifs prod block_rows nrows  rows
FAST_CASES = [(64, 8, 1, 0, 1, 9, "noise"),                   # fewer rows than lane groups (64 groups of 4 lanes)
              (128, 8, 1, 0, 63, 200, "noise"),               # around the lane groups' share
              (192, 8, 1, 0, 64, 129, "noise"),               # 3 x 64 bytes: the narrowest tile, three of them; a last block of one row
              (1024, 8, 1, 0, 65, 300, "noise"),              # one 1024-byte tile: 4 lane groups
              (4096, 8, 1, 0, 1000, 2001, "noise"),           # four 1024-byte tiles; a last block of one row
              (64, 8, 1, 0, 4096, 4097, "noise"),             # long runs; a last block of one row
              (512, 16, 1, 0, 1000, 1500, "noise"),
              (32, 16, 1, 0, 64, 200, "noise"),               # exactly one 64-byte tile
              (512, 16, 1, 0, 4096, 4100, "noise"),
              (1024, 8, 1, 0, 4096, 4096, "max"),             # all 255
              (64, 8, 1, 0, 4096, 4096, "max"),
              (512, 16, 1, 0, 4096, 4096, "max"),             # all 65535
              (128, 8, 4, 3, 65, 200, "noise"),               # the last of four products
              (64, 16, 4, 3, 63, 190, "noise"),
              (1024, 8, 1, 0, 20000, 20001, "noise"),         # a block longer than one register run of the 1024-byte tile (4 x 4096 rows)
              (1024, 8, 1, 0, 20000, 20000, "max"),           # ... every lane's uint32 partials at their largest
              (512, 16, 1, 0, 20000, 20000, "max")]
# the other side of every clause
GENERIC_CASES = [(48, 8, 1, 0, 64, 200, "noise"),             # not whole 64-byte tiles
                 (40, 8, 3, 0, 64, 200, "noise"),             # a pitch of 120 bytes
                 (64, 32, 1, 0, 64, 200, "noise"),            # float rows
                 (1024, 32, 2, 1, 65, 300, "noise")]


def case_id(c):
    return "c%d_b%d_if%d_p%d_br%d_n%d_%s" % c


@functools.lru_cache(maxsize=None)
def case_rows(c):
    nchan, nbits, nifs, _prod, _br, nrows, kind = c
    if kind == "max":
        rows = np.full((nrows, nifs, nchan), 2 ** nbits - 1, dtype=rc.DTYPES[nbits])
    else:
        rows = rc.make_rows(nrows, nifs, nchan, nbits, seed=nchan + nrows)
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize("c", FAST_CASES + GENERIC_CASES, ids=case_id)
def test_fast_kernel_shapes_and_the_other_side_of_every_clause(hip_lib, c):
    nchan, nbits, nifs, prod, br, nrows, kind = c
    rows = case_rows(c)
    got = check(hip_lib, rows, prod, rc.params(block_rows=br, t_cell=3.0), RULE3, rc.FAST if c in FAST_CASES else rc.GENERIC)
    if kind == "max":
        code = 2 ** nbits - 1
        assert np.all(got["stats"][0, :, 0] == code * br) and np.all(got["stats"][0, :, 1] == code * code * br)
        assert got["res"]["chan_flag"].all() and np.all(got["res"]["repl"] == code)


def test_tile_widths_of_the_cases():
    """every listed tile width is some case's: 64 (64, 192 channels and 32 of 16 bit), 128, 256 (128 of 16 bit), 1024 (1024, 4096
    and 512 of 16 bit), and 512 in test_the_tile_widths_in_between"""
    widths = {rc.tile_bytes(c[0], c[1]) for c in FAST_CASES} | {rc.tile_bytes(g[0], g[1]) for g in rc.grid() if g[1] != 32 and g[0] != 48}
    assert widths == {64, 128, 256, 1024}
    assert rc.tile_bytes(192, 8) == 64 and rc.tile_bytes(256, 8) == 256 and rc.tile_bytes(256, 16) == 512


@pytest.mark.parametrize("nchan,nbits", [(256, 8), (256, 16)])
def test_the_tile_widths_in_between(hip_lib, nchan, nbits):
    """256- and 512-byte tiles (16 and 8 lane groups)"""
    rows = rc.make_rows(700, 2, nchan, nbits, seed=5)
    check(hip_lib, rows, 1, rc.params(block_rows=300, t_cell=3.0), RULE3, rc.FAST)


@pytest.mark.parametrize("c", [FAST_CASES[1], FAST_CASES[3], FAST_CASES[6], FAST_CASES[12], FAST_CASES[5]], ids=case_id)
def test_both_kernels_give_the_same_bits(hip_lib, c):
    """the same rows at an aligned address (fast kernel) and 4 bytes behind one (generic): the same statistics, mask and rows"""
    nchan, nbits, nifs, prod, br, nrows, _kind = c
    rows = case_rows(c)
    par = rc.params(block_rows=br, t_cell=3.0)
    fast = check(hip_lib, rows, prod, par, RULE3, rc.FAST)
    slow = on_device(hip_lib, rows, prod, par, shift=4)
    assert slow["used"] == slow["says"] == slow["clean_used"] == rc.fast_expected(nchan, nifs, nbits, slow["address"]) == rc.GENERIC
    assert slow["stats"].tobytes() == fast["stats"].tobytes() and rc.same_result(slow["res"], fast["res"])
    assert slow["cleaned"].tobytes() == fast["cleaned"].tobytes() and slow["clean_rows"].tobytes() == fast["clean_rows"].tobytes()


@pytest.mark.parametrize("c", [FAST_CASES[3], GENERIC_CASES[0], GENERIC_CASES[2]], ids=case_id)
def test_clean_host_is_clean_device_and_a_download(hip_lib, c):
    nchan, nbits, nifs, prod, br, nrows, _kind = c
    rows = case_rows(c)
    par = rc.params(block_rows=br, t_cell=3.0)
    dev = on_device(hip_lib, rows, prod, par)
    with guarded():
        code, out, res, used, msg = rc.clean_host(hip_lib, rows, prod, par)
    assert code == 0, msg
    assert used == dev["clean_used"] and rc.same_result(res, dev["clean_res"]) and out.tobytes() == dev["clean_rows"].tobytes()
    with guarded():
        code, st, used_s, msg = rc.stats_host(hip_lib, rows, prod, par)
    assert code == 0 and used_s == dev["used"] and st.tobytes() == dev["stats"].tobytes(), msg
    with guarded():
        code, out2, msg = rc.apply_host(hip_lib, rows, prod, par, res["mask"], res["repl"])
    assert code == 0 and out2.tobytes() == out.tobytes(), msg


# ---- the rule on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_known_answer_on_the_device(hip_lib, seed):
    q = np.ascontiguousarray(rc.known_answer_rows(seed)[:, None, :])
    got = check(hip_lib, q, 0, rc.params(block_rows=rc.KA_BLOCK), rc.rule_kw(rc.DEFAULTS), rc.FAST, zap=rc.ka_zap())
    res = got["clean_res"]
    assert np.flatnonzero(res["chan_flag"]).tolist() == rc.KA_CHANNELS and np.flatnonzero(res["blk_flag"]).tolist() == rc.KA_BLOCKS
    assert rc.other_cells(res) == rc.KA_CELLS


def test_nan_and_inf_on_the_device(hip_lib):
    rng = np.random.default_rng(7)
    rows = (10.0 + rng.standard_normal((64 * 6, 1, 48))).astype(np.float32)
    rows[70, 0, 5] = np.nan
    rows[200, 0, 9] = np.inf
    got = check(hip_lib, rows, 0, rc.params(block_rows=64), rc.rule_kw(rc.DEFAULTS), rc.GENERIC)
    assert got["res"]["mask"][1, 5] == 1 and got["res"]["mask"][3, 9] == 1 and int(got["res"]["mask"].sum()) == 2
    assert np.isfinite(got["clean_rows"]).all()


def test_the_rows_the_channeliser_writes(hip_lib, tmp_path):
    """0.3 s of a 32 MHz IF through the channeliser with pol = 4, 8 bit, 1024 channels; the .fil read back: statistics, mask and
    cleaned rows of product 0 and of product 3 against the restatement"""
    vd = str(tmp_path / "pr001a_ef_no0001_IF1.vdif")
    synth.make_vdif(0.3, bw_mhz=32.0, nchan=1024).tofile(vd)
    hdr = pv.make_hdr("J0000+00", 1400.0, vd, pol=4, usb=True, ra="00:00:00", dec="00:00:00", bw=32.0, telescope="effelsberg")
    with contextlib.redirect_stdout(io.StringIO()):
        path = pv.run_digifil(hdr, str(tmp_path), 0, 0.3, 1024, overwrite=True, pol=4, nbit=8)
    fil = sigproc.read_fil(path)
    h = fil.header
    rows = np.ascontiguousarray(fil.data)
    assert h["nifs"] == 4 and h["nchans"] == 1024 and h["nbits"] == 8 and rows.shape[0] >= 5000
    for prod in (0, 3):
        check(hip_lib, rows, prod, rc.params(block_rows=512), rc.rule_kw(rc.DEFAULTS), rc.FAST)
    assert not np.array_equal(rows[:, 0], rows[:, 3])


# ---- timing -------------------------------------------------------------------------------------------------------------------
def test_flagging_is_not_what_the_dm_range_waits_for(hip_lib):
    """the documented prepsubband shape -- 10 s x 1024 channels, 8 bit, rows resident in HBM (made there with torch), one channel
    dead so that every call flags it, uploads the mask and runs the apply kernel (306 masked cells; cleaning leaves the channel
    as it was, so every round does the same work): after one warm-up of each, the median of five frbch_rfi_clean_device calls
    (statistics, download, the host decision, upload, apply) is at most the median of five frbch_dedisperse_device calls over 64
    DMs of the same rows.  Margin 1.0: one read of the rows against 64 dedispersions of them."""
    torch = pytest.importorskip("torch")
    gen = torch.Generator(device="cuda").manual_seed(5)
    rows = torch.randint(100, 156, (rc.TIMING_ROWS, rc.TIMING_NCHAN), dtype=torch.uint8, device="cuda", generator=gen)
    rows[:, rc.TIMING_DEAD_CHANNEL] = rc.TIMING_DEAD_CODE
    torch.cuda.synchronize()
    with guarded():
        stats = rc.timing_run(hip_lib, rows.data_ptr())
    print("RFI-TIMING " + json.dumps(stats))
    assert stats["kernel_used"] == rc.FAST and stats["masked_cells"] == stats["nblk"]
    assert stats["rfi_clean_device_median_s"] <= 1.0 * stats["dedisperse_device_median_s"], stats
