"""frbch_k2_priv with MORE THAN ONE FLUSH of its rescale sums inside a launch: offset and scale bit for bit.

The kernel's fp32 sums leave the registers every 8 trips.  Since the flush became write-only (a slot of fp32 sums per flush in the
workgroup's slice, folded into the fp64 partial table when the workgroup ends: csrc/kernels_k2priv.inc) the second and later
flushes of a launch are where the change lives -- and the shapes of tests/test_gpu_k2priv_stats.py (three blocks on 512 workgroups:
2 - 3 trips, ONE flush) never get there.  Here: 32 MHz, 1024 channels, TEN blocks of 2^22 samples in one launch (maxb = 10), 5120
tiles on 512 workgroups = 10 trips each: a full flush behind trip 7 and a short one behind trip 9, the smallest shape with two
slots.  (Another CU count: the block count that gives >= 9 trips, see `shape`; more than 16 blocks: skipped.)

Every case must reproduce, bit for bit, the offset / scale the library computed BEFORE that change, when every flush added into
the table in place: tests/golden/k2priv_flush.npz (tests/golden/make_k2priv_flush_golden.py, run once on the GPU with the build of
the commit before the change).  The recorded bits belong to the grid they were recorded on (the rows of the table are the
workgroups); on another grid the comparisons with them are skipped, the others run.
  * pol 5 and 2, USB and LSB (`flip`: the statistics pass reorders its sums on the way out), two-pass (1 << 28), interval 10 s: the
    interval stays open, frbch_flush_device closes it;
  * the same with an interval that ends inside one workgroup's SECOND slot and inside a tile (`mid_interval`; 512 workgroups:
    workgroup 300 owns rows 12000 .. 12039, row 12033 lies in its trip 8): the workgroups below take every row, this one the per-row
    path in its second slot, those behind it flush zeros;
  * -t 4, no -c, 1 << 27: frbch_k2_priv<PM, 1>, the float-row form, with the same two slots; the interval closes inside the launch,
    offset / scale are read behind frbch_process_device (keys "<case>__first": the interval frbch_k2_priv summed) and behind the
    flush (the rest of the rows, summed by the separate statistics kernel);
  * every case runs twice on its handle (frbch_reset in between): a fold that starts an interval must see neither the table nor the
    slices the first run left;
  * `iquv_usb_t4_add`: 1 + 9 blocks in two calls, -t 4, two-pass, interval open.  The first call's statistics pass starts the
    interval; the second call writes the deferred batch's float rows (no sums) and then sums its own nine blocks INTO the interval:
    that fold starts from the table (KParams::stat_first == 0) and has two slots.  frbch_k2_priv<5, 2> and <5, 1> both in the record;
  * -t 4, 1 << 28 against 1 << 27: the statistics-only and the float-row form agree bit for bit at this shape too.
"""
import os

import numpy as np
import pytest

from frb_baseband_amd import channeliser as ch
from frb_baseband_amd import synth
from tests import parity_util as pu
from tests.hipmem import GuardedBuffer as DeviceBuffer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k2priv_flush.npz")
BW, NCHAN = 32.0, 1024
BLOCK_SAMPLES, RATE = 1 << 22, 64.0e6         # real samples per block and per second (2 x 32 MHz)
ROWS_PER_BLOCK, TILE_ROWS = 2048, 4
TILES_PER_BLOCK = ROWS_PER_BLOCK // TILE_ROWS
TSAMP = 2.0 * NCHAN / RATE                    # 32 us per row
TWO_PASS, BUFFERED = 1 << 28, 1 << 27
MIN_TRIPS, MIN_BLOCKS, MAX_BLOCKS = 9, 10, 16
MID_WG_OF_512 = 300                           # the workgroup whose second slot the `mid` interval ends in (scaled with the grid)


def secs_of(nblocks):
    return nblocks * BLOCK_SAMPLES / RATE + 0.004


def trips_of(nblocks, grid):
    return -(-nblocks * TILES_PER_BLOCK // grid)


def blocks_for(grid):
    """smallest block count >= MIN_BLOCKS at which a workgroup of `grid` runs MIN_TRIPS trips (two slots)"""
    nb = MIN_BLOCKS
    while trips_of(nb, grid) < MIN_TRIPS and nb <= MAX_BLOCKS:
        nb += 1
    return nb


def mid_interval(nblocks, grid):
    """(rows, seconds) of an interval that ends behind the first row of trip 8 of workgroup MID_WG_OF_512 * grid / 512"""
    ntiles = nblocks * TILES_PER_BLOCK
    per, extra = divmod(ntiles, grid)
    wg = MID_WG_OF_512 * grid // 512
    first = wg * per + min(wg, extra)
    rows = (first + 8) * TILE_ROWS + 1
    return rows, (rows + 0.25) * TSAMP         # (the way 0.097321 s gives 3041 rows; a quarter row past: -t 4 takes rows // 4)


def cases(nblocks, grid):
    """name -> (bw, keyword arguments of parity_util.lib_cfg, kernel the launch record must show, interval rows or None)"""
    rows, secs = mid_interval(nblocks, grid)
    out = {}
    for pol, pname in ((5, "iquv"), (2, "i")):
        for bw, sense in ((BW, "usb"), (-BW, "lsb")):
            kern = f"frbch_k2_priv<{pol}, 2>"
            out[f"{pname}_{sense}_open"] = (bw, dict(pol=pol, flags=TWO_PASS, interval=10.0, maxb=nblocks), kern, None)
            out[f"{pname}_{sense}_mid"] = (bw, dict(pol=pol, flags=TWO_PASS, interval=secs, maxb=nblocks), kern, rows)
    # -t 4: output rows of four; the interval ends with trip 7 of that workgroup (rows // 4 output rows)
    out["iquv_lsb_t4_rows"] = (-BW, dict(pol=5, tscr=4, const=0, flags=BUFFERED, interval=secs, maxb=nblocks), "frbch_k2_priv<5, 1>", rows // 4)
    out["i_usb_t4_rows"] = (BW, dict(pol=2, tscr=4, const=0, flags=BUFFERED, interval=secs, maxb=nblocks), "frbch_k2_priv<2, 1>", rows // 4)
    return out


ADD_CASE = "iquv_usb_t4_add"


def add_case(nblocks):
    # an interval 40 ms longer than the stream: it stays open until the flush (and the buffer of float rows stays small)
    return BW, dict(pol=5, tscr=4, flags=TWO_PASS, interval=secs_of(nblocks) + 0.04, maxb=nblocks)


def pair(c):
    off, sc = c.get_rescale()
    return np.stack([off.reshape(-1), sc.reshape(-1)])


def measure(lib, d_raw, nfr, nblocks, bw, kw, runs=1, interval_rows=None, calls=None):
    """`runs` passes of one handle over the first `nblocks` blocks of the frames, frbch_reset between them; `calls`: the blocks of
    each frbch_process_device call (default: all at once).  Returns, per pass, offset / scale ([2][nif * nchan]) behind the last
    frbch_process_device (None while no interval has closed) and behind the flush, and the kernels the first pass launched."""
    out_pairs = []
    with ch.Channeliser(pu.lib_cfg(lib, bw, NCHAN, secs_of(nblocks), **kw), lib) as c:
        info = c.info
        assert (nfr * 8000) // info.block_payload_bytes >= nblocks and info.rows_per_block * kw.get("tscr", 1) == ROWS_PER_BLOCK
        if interval_rows is not None:
            assert info.rescale_interval_rows == interval_rows, (info.rescale_interval_rows, interval_rows)
        rows = nblocks * info.rows_per_block
        out = DeviceBuffer(rows * info.row_bytes)
        c.set_profiling(True)
        record = None
        for _ in range(runs):
            r, b0 = 0, 0
            for nb in calls or (nblocks,):
                r += c.process_device(d_raw.ptr.value, nfr, 8032, 32, b0 * info.block_payload_bytes, nb,
                                      out.ptr.value + r * info.row_bytes, out.nbytes - r * info.row_bytes)
                b0 += nb
            assert b0 == nblocks
            before = pair(c) if c.get_info().have_rescale else None
            r += c.flush_device(out.ptr.value + r * info.row_bytes, out.nbytes - r * info.row_bytes)
            assert r == rows
            out_pairs.append((before, pair(c)))
            if record is None:
                record = c.get_launch_record()
            c.reset()
    return out_pairs, record


def same_bits(a, b):
    return a is not None and b is not None and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ndiff(a, b):
    return int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))) if a is not None and a.shape == b.shape else -1


def probe_grid(lib, d_raw, nfr):
    """workgroups of frbch_k2_priv on this device (2 x CUs), read off a launch of two blocks (1024 tiles: grids up to 1024 show)"""
    _, record = measure(lib, d_raw, nfr, 2, BW, dict(pol=2, flags=TWO_PASS, interval=10.0, maxb=2))
    return record["frbch_k2_priv<2, 2>"]["grid_x"]


@pytest.fixture(scope="module")
def shape(hip_lib):
    """the input of every case, uploaded once (both band senses read the same samples): (device frames, frames, blocks, grid)"""
    raw = synth.make_vdif(secs_of(MIN_BLOCKS), bw_mhz=BW, nchan=NCHAN)
    d_raw, nfr = DeviceBuffer.from_numpy(raw), raw.size // 8032
    grid = probe_grid(hip_lib, d_raw, nfr)
    nblocks = blocks_for(grid)
    if nblocks > MAX_BLOCKS:
        pytest.skip(f"{grid} workgroups: more than {MAX_BLOCKS} blocks for {MIN_TRIPS} trips")
    if nblocks > MIN_BLOCKS:
        raw = synth.make_vdif(secs_of(nblocks), bw_mhz=BW, nchan=NCHAN)
        d_raw, nfr = DeviceBuffer.from_numpy(raw), raw.size // 8032
    assert trips_of(nblocks, grid) >= MIN_TRIPS
    return d_raw, nfr, nblocks, grid


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def recorded(golden, shape, key):
    _, _, nblocks, grid = shape
    if (int(golden["grid"]), int(golden["nblocks"])) != (grid, nblocks):
        pytest.skip(f"the bits were recorded on {int(golden['grid'])} workgroups and {int(golden['nblocks'])} blocks, here {grid} and {nblocks}")
    return golden[key]


CASE_NAMES = sorted(cases(MIN_BLOCKS, 512))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_offset_and_scale_are_the_recorded_bits(hip_lib, shape, golden, name):
    d_raw, nfr, nblocks, grid = shape
    bw, kw, kernel, irows = cases(nblocks, grid)[name]
    ((before, first), (before2, again)), record = measure(hip_lib, d_raw, nfr, nblocks, bw, kw, runs=2, interval_rows=irows)
    assert kernel in record and record[kernel]["grid_x"] == grid, f"{kernel} did not run on {grid} workgroups: {record}"
    assert np.isfinite(first).all()
    assert same_bits(again, first), "the second pass of the handle (table and slices hold the first one's sums) differs"
    if name.endswith("_t4_rows"):
        assert before is not None and not same_bits(before, first), "the launch did not close an interval of its own"
        assert same_bits(before2, before), "first interval: the second pass of the handle differs"
        want = recorded(golden, shape, name + "__first")
        print(f"{name}: first interval, {ndiff(before, want)} of {want.size} values differ from the recorded bits")
        assert same_bits(before, want), f"{ndiff(before, want)} of {want.size} offset / scale values of the first interval differ from the recorded ones"
    want = recorded(golden, shape, name)
    print(f"{name}: {ndiff(first, want)} of {want.size} values differ from the recorded bits")
    assert same_bits(first, want), f"{ndiff(first, want)} of {want.size} offset / scale values differ from the recorded ones"


def test_second_launch_adds_into_the_interval(hip_lib, shape, golden):
    """1 + (n - 1) blocks: the second call's frbch_k2_priv<5, 1> folds two slots on top of what the first call left in the table"""
    d_raw, nfr, nblocks, grid = shape
    bw, kw = add_case(nblocks)
    assert trips_of(nblocks - 1, grid) >= MIN_TRIPS
    ((before, first), (_, again)), record = measure(hip_lib, d_raw, nfr, nblocks, bw, kw, runs=2, calls=(1, nblocks - 1))
    assert "frbch_k2_priv<5, 2>" in record and record.get("frbch_k2_priv<5, 1>", {}).get("launches", 0) >= 2, record
    assert before is None, "the interval closed before the flush"
    assert np.isfinite(first).all()
    assert same_bits(again, first), "the second pass of the handle differs"
    want = recorded(golden, shape, ADD_CASE)
    print(f"{ADD_CASE}: {ndiff(first, want)} of {want.size} values differ from the recorded bits")
    assert same_bits(first, want), f"{ndiff(first, want)} of {want.size} offset / scale values differ from the recorded ones"


@pytest.mark.parametrize("bw,pol", [(BW, 5), (-BW, 5), (-BW, 2)])
def test_statistics_only_and_float_row_form_agree_at_t4(hip_lib, shape, bw, pol):
    """-t 4: both forms take frbch_k2_priv's rolled emit over the same rows in the same order, two slots each: the same offset / scale"""
    d_raw, nfr, nblocks, grid = shape
    rows, secs = mid_interval(nblocks, grid)
    kw = dict(pol=pol, tscr=4, interval=secs, maxb=nblocks)
    ((_, two),), rec2 = measure(hip_lib, d_raw, nfr, nblocks, bw, dict(kw, flags=TWO_PASS), interval_rows=rows // 4)
    ((_, buf),), rec1 = measure(hip_lib, d_raw, nfr, nblocks, bw, dict(kw, flags=BUFFERED), interval_rows=rows // 4)
    assert f"frbch_k2_priv<{pol}, 2>" in rec2 and f"frbch_k2_priv<{pol}, 1>" in rec1, (sorted(rec2), sorted(rec1))
    assert np.isfinite(two).all()
    assert same_bits(two, buf), f"{ndiff(two, buf)} values differ"
