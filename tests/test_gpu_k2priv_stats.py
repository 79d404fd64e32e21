"""frbch_k2_priv, the statistics it sums (MODE 2: the first pass of the two-pass rescale; MODE 1: the buffered form at -t 4):
offset and scale bit for bit.

The kernel's flush of the fp32 sums into the fp64 partial table, the order of the sums in a thread's registers, the test of the
interval's end and who clears the table changed with no float operation on a sample changed: every case below must reproduce, bit
for bit, the offset / scale the library computed before that change.  Those are recorded in tests/golden/k2priv_stats.npz
(tests/golden/make_k2priv_stats_golden.py, run once on the GPU with the library of the commit before the change).

The shapes are the smallest that reach the kernel (tests/kernel_table.py, the frbch_k2_priv rows): 32 MHz, 1024 channels, three
blocks of 2^22 samples (2048 rows each), 512 tiles a block.
  * interval 0.097321 s = 3041 rows: ends inside the second block and inside a tile (3041 = 4 * 760 + 1) -- tiles wholly below the
    end, the one that straddles it (the per-row path) and tiles behind it (not read) in one launch of two blocks; the interval
    closes inside its first launch, so nothing clears the table and frbch_stats_final reads the launch's rows only;
  * interval 10 s, one launch of three blocks: the interval does not close, the batch stays deferred, frbch_flush_device runs the
    statistics over what there is (again the launch's rows only: the rows behind them are cleared when a second launch adds to the
    interval, which tests/test_gpu_parity.py and tests/test_gpu_stream_order.py reach with their 3 + 1 block sequences);
  * every case runs twice on its handle (frbch_reset in between): the second run finds the first one's sums in the table, which a
    first flush that stores, and does not add, must not see;
  * no -c, -t 4, interval 760 rows, batches of 1024 and 512 rows (the *_t4_two_intervals cases): the buffered form on
    frbch_k2_priv<PM, 1>.  The first batch starts and closes the first interval: its sums are frbch_k2_priv's (a first flush that
    stores, frbch_stats_final over the launch's rows).  The second interval starts on the 264 rows left in the buffer, so its sums
    come from the separate statistics kernel, not from frbch_k2_priv.  test_offset_and_scale_are_the_recorded_bits sees the
    second interval's offset / scale only (whatever is current after the flush): for these two cases it pins the path and the kernel
    name, little more.  test_first_interval_of_the_buffered_form feeds the two batches in two calls and compares the first
    interval's offset / scale, read between them, with the recorded bits (keys "<case>__first");
  * -t 4, 1 << 28 against 1 << 27: the statistics-only and the float-row form (both rolled, both frbch_k2_priv) agree bit for bit.
"""
import os

import numpy as np
import pytest

from frb_baseband_amd import channeliser as ch
from frb_baseband_amd import synth
from tests import parity_util as pu
from tests.hipmem import GuardedBuffer as DeviceBuffer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k2priv_stats.npz")
BW, NCHAN, SECS = 32.0, 1024, 0.216269
TWO_PASS, BUFFERED = 1 << 28, 1 << 27

# name -> (bw, keyword arguments of parity_util.lib_cfg, kernel the launch record must show)
CASES = {
    "iquv_usb": (BW, dict(pol=5, flags=TWO_PASS, interval=0.097321, maxb=2), "frbch_k2_priv<5, 2>"),
    "iquv_lsb": (-BW, dict(pol=5, flags=TWO_PASS, interval=0.097321, maxb=2), "frbch_k2_priv<5, 2>"),
    "i_usb": (BW, dict(pol=2, flags=TWO_PASS, interval=0.097321, maxb=2), "frbch_k2_priv<2, 2>"),
    "i_lsb": (-BW, dict(pol=2, flags=TWO_PASS, interval=0.097321, maxb=2), "frbch_k2_priv<2, 2>"),
    "iquv_usb_open": (BW, dict(pol=5, flags=TWO_PASS, interval=10.0, maxb=4), "frbch_k2_priv<5, 2>"),
    "i_lsb_open": (-BW, dict(pol=2, flags=TWO_PASS, interval=10.0, maxb=4), "frbch_k2_priv<2, 2>"),
    "iquv_lsb_t4_two_intervals": (-BW, dict(pol=5, tscr=4, const=0, flags=BUFFERED, interval=0.097321, maxb=2), "frbch_k2_priv<5, 1>"),
    "i_usb_t4_two_intervals": (BW, dict(pol=2, tscr=4, const=0, flags=BUFFERED, interval=0.097321, maxb=2), "frbch_k2_priv<2, 1>"),
}


@pytest.fixture(scope="module")
def frames():
    """the input of every case, uploaded once (both band senses read the same samples)"""
    raw = synth.make_vdif(SECS, bw_mhz=BW, nchan=NCHAN)
    return DeviceBuffer.from_numpy(raw), raw.size // 8032


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def measure(lib, d_raw, nfr, bw, kw, runs=1):
    """offset / scale ([2][nif * nchan]) of `runs` passes of one handle over the frames, and the kernels the first pass launched"""
    out_pairs = []
    with ch.Channeliser(pu.lib_cfg(lib, bw, NCHAN, SECS, **kw), lib) as c:
        info = c.info
        nblocks = (nfr * 8000) // info.block_payload_bytes
        rows = nblocks * info.rows_per_block
        out = DeviceBuffer(rows * info.row_bytes)
        c.set_profiling(True)
        record = None
        for _ in range(runs):
            r = c.process_device(d_raw.ptr.value, nfr, 8032, 32, 0, nblocks, out.ptr.value, out.nbytes)
            r += c.flush_device(out.ptr.value + r * info.row_bytes, out.nbytes - r * info.row_bytes)
            assert r == rows
            off, sc = c.get_rescale()
            out_pairs.append(np.stack([off.reshape(-1), sc.reshape(-1)]))
            if record is None:
                record = c.get_launch_record()
            c.reset()
    return out_pairs, record


def measure_first_interval(lib, d_raw, nfr, bw, kw, nb_first):
    """the same frames in two calls of nb_first blocks and the rest: offset / scale after the first call (the first interval's, when
    it closes there) and at the end, and the kernels launched"""
    with ch.Channeliser(pu.lib_cfg(lib, bw, NCHAN, SECS, **kw), lib) as c:
        info = c.info
        nblocks = (nfr * 8000) // info.block_payload_bytes
        rows = nblocks * info.rows_per_block
        out = DeviceBuffer(rows * info.row_bytes)
        c.set_profiling(True)
        r = c.process_device(d_raw.ptr.value, nfr, 8032, 32, 0, nb_first, out.ptr.value, out.nbytes)
        off, sc = c.get_rescale()
        first = np.stack([off.reshape(-1), sc.reshape(-1)])
        r += c.process_device(d_raw.ptr.value, nfr, 8032, 32, nb_first * info.block_payload_bytes, nblocks - nb_first,
                              out.ptr.value + r * info.row_bytes, out.nbytes - r * info.row_bytes)
        r += c.flush_device(out.ptr.value + r * info.row_bytes, out.nbytes - r * info.row_bytes)
        assert r == rows
        off, sc = c.get_rescale()
        return first, np.stack([off.reshape(-1), sc.reshape(-1)]), c.get_launch_record()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_offset_and_scale_are_the_recorded_bits(hip_lib, frames, golden, name):
    bw, kw, kernel = CASES[name]
    (first, again), record = measure(hip_lib, frames[0], frames[1], bw, kw, runs=2)
    assert kernel in record, f"{kernel} did not run: {sorted(record)}"
    want = golden[name]
    assert np.isfinite(first).all()
    ndiff = int(np.count_nonzero(first.view(np.uint32) != want.view(np.uint32))) if first.shape == want.shape else -1
    print(f"{name}: {ndiff} of {want.size} values differ from the recorded bits")
    assert same_bits(first, want), f"{ndiff} of {want.size} offset / scale values differ from the recorded ones"
    assert same_bits(again, want), "the second pass of the handle (the table holds the first one's sums) differs"


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.endswith("_two_intervals")))
def test_first_interval_of_the_buffered_form(hip_lib, frames, golden, name):
    """the first interval of the *_t4_two_intervals cases is summed by frbch_k2_priv<PM, 1> from an uncleared table row"""
    bw, kw, kernel = CASES[name]
    first, last, record = measure_first_interval(hip_lib, frames[0], frames[1], bw, kw, nb_first=2)
    assert kernel in record, f"{kernel} did not run: {sorted(record)}"
    want = golden[name + "__first"]
    assert np.isfinite(first).all() and not same_bits(first, last), "the first call did not close an interval of its own"
    ndiff = int(np.count_nonzero(first.view(np.uint32) != want.view(np.uint32))) if first.shape == want.shape else -1
    print(f"{name}: first interval, {ndiff} of {want.size} values differ from the recorded bits")
    assert same_bits(first, want), f"{ndiff} of {want.size} offset / scale values of the first interval differ from the recorded ones"
    assert same_bits(last, golden[name]), "fed in two calls, the second interval differs from the recorded one"


@pytest.mark.parametrize("bw,pol", [(BW, 5), (-BW, 5), (-BW, 2)])
def test_statistics_only_and_float_row_form_agree_at_t4(hip_lib, frames, bw, pol):
    """-t 4: both forms take frbch_k2_priv's rolled emit; the same rows in the same order, so the same offset / scale"""
    kw = dict(pol=pol, tscr=4, interval=0.097321, maxb=2)
    (two,), rec2 = measure(hip_lib, frames[0], frames[1], bw, dict(kw, flags=TWO_PASS))
    (buf,), rec1 = measure(hip_lib, frames[0], frames[1], bw, dict(kw, flags=BUFFERED))
    assert f"frbch_k2_priv<{pol}, 2>" in rec2 and f"frbch_k2_priv<{pol}, 1>" in rec1, (sorted(rec2), sorted(rec1))
    assert np.isfinite(two).all()
    assert same_bits(two, buf), f"{int(np.count_nonzero(two.view(np.uint32) != buf.view(np.uint32)))} values differ"
