"""Stream order of the device-resident entry points (the contract above them in include/frbch.h) on the emulator's deferred
scheduler (tests/emu/dev_emu.h): every sequence runs once in mode 0 (call order: the expected bytes), then in mode 1 (lazy: a
host sync runs the synced stream and only what its waits demand) and in mode 2 (others first: every other stream runs as far
as its own waits allow before the synced one).  Both are schedules a device may produce; a missing event edge shows as rows
that differ, or as poison left in the output.

A case is a generator over a Run: it opens its handles, queues its calls and yields (outputs, stream to synchronise or None
when the sequence itself ended in a host-synchronous call); the harness then
  1. synchronises that stream only,  2. compares the output bytes with ==,  3. drains everything,
  4. asserts that nothing is pending and nothing was counted as a violation;
the generator is then resumed to close its handles.  Input frames arrive late: the frame buffer first holds another IF's
valid frames, the real ones come by an asynchronous copy queued on the caller's stream just before the call."""
import ctypes as C
import functools

import numpy as np
import pytest

from frb_baseband_amd import channeliser as ch
from frb_baseband_amd import multi_if, synth
from tests import bounds_cases as bc
from tests import parity_util as pu
from tests.hipmem import GUARD, POISON, HostGuardedBuffer

MODES = (1, 2)
NCHAN, FREQ_RES, BW, NIF = 128, 512, 16.0, 3        # the chain's smallest shape (tests/test_multi_if.py)
LANES = 176 | (3 << 24)                             # frbch_config.overlap: the digitiser beside the next IF's K1


def hooks(lib):
    if not getattr(lib, "_emu_hooks", False):
        for name, res, args in (("set_mode", None, [C.c_int]), ("mode", C.c_int, []), ("stream_create", C.c_void_p, []),
                                ("stream_destroy", None, [C.c_void_p]), ("memcpy_async", None, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
                                ("stream_sync", None, [C.c_void_p]), ("drain", None, []), ("pending", C.c_uint64, []),
                                ("violations", C.c_uint64, []), ("queued_on_lane", C.c_uint64, [C.c_int, C.c_int])):
            fn = getattr(lib, "frbch_test_emu_" + name)
            fn.restype, fn.argtypes = res, args
        lib._emu_hooks = True
    return lib


@functools.lru_cache(maxsize=None)
def frames(secs, if_index):
    raw = synth.make_vdif(secs, bw_mhz=BW, nchan=NCHAN, if_index=if_index)
    raw.setflags(write=False)
    return raw


class Run:
    def __init__(self, lib, mode):
        self.lib, self.mode = hooks(lib), mode
        self.bufs, self.streams = [], []
        self.elsewhere = 0

    def stream(self):
        self.streams.append(self.lib.frbch_test_emu_stream_create())
        return self.streams[-1]

    def out(self, nbytes):
        self.bufs.append(HostGuardedBuffer(nbytes))
        return self.bufs[-1]

    def late(self, secs, if_index, stream):
        """a frame buffer that holds IF `if_index + 7`'s frames; those of `if_index` are queued behind what `stream` holds"""
        real = frames(secs, if_index)
        buf = HostGuardedBuffer.from_numpy(frames(secs, if_index + 7))
        self.bufs.append(buf)
        self.copy(buf, real, stream)
        return buf

    def copy(self, buf, arr, stream):
        assert arr.nbytes == buf.nbytes
        self.lib.frbch_test_emu_memcpy_async(buf.ptr, arr.ctypes.data, arr.nbytes, stream)
        buf.expect(arr)

    def chan(self, secs, **kw):
        overlap = kw.pop("overlap", 0)
        cfg = pu.lib_cfg(self.lib, kw.pop("bw", BW), NCHAN, secs, freq_res=FREQ_RES, **kw)
        cfg.overlap = overlap
        return ch.Channeliser(cfg, self.lib)


def geometry(c, raw):
    info = c.info
    nfr = raw.size // 8032
    nblocks = (nfr * 8000 - info.block_payload_bytes) // info.block_stride_bytes + 1
    return info, nfr, nblocks


def execute(lib, case, mode):
    """-> (output bytes after the sync of the caller's stream alone, after the drain, ops queued on the chain's second stream)"""
    lib = hooks(lib)
    assert lib.frbch_test_emu_mode() == 0 and lib.frbch_test_emu_pending() == 0
    lib.frbch_test_emu_set_mode(mode)
    try:
        v0 = lib.frbch_test_emu_violations()
        lib.frbch_test_emu_queued_on_lane(LANES & 0xFFFF, 1)
        run = Run(lib, mode)
        gen = case(run)
        outs, sync = next(gen)
        if sync is not None:
            lib.frbch_test_emu_stream_sync(sync)
        first = [o.to_numpy(np.uint8).copy() for o in outs]
        run.elsewhere = lib.frbch_test_emu_queued_on_lane(LANES & 0xFFFF, 0)
        lib.frbch_test_emu_drain()
        assert lib.frbch_test_emu_pending() == 0
        after = [o.to_numpy(np.uint8).copy() for o in outs]
        for _ in gen:                                   # the case closes its handles
            pass
        for b in run.bufs:
            b.check(contents=True)
        for s in run.streams:
            lib.frbch_test_emu_stream_destroy(s)
        assert lib.frbch_test_emu_pending() == 0
        assert lib.frbch_test_emu_violations() == v0, "a stream was destroyed, or memory freed, with work pending on it"
        return first, after, run.elsewhere
    finally:
        lib.frbch_test_emu_set_mode(0)


_EXPECTED = {}


def hold(lib, name, case, mode, lanes=False):
    if name not in _EXPECTED:
        want, again, _n = execute(lib, case, 0)
        for w, a in zip(want, again):
            assert w.tobytes() == a.tobytes()
            w.setflags(write=False)
        assert any((w != POISON).any() for w in want), "the sequence wrote nothing: the case proves nothing"
        _EXPECTED[name] = want
    want = _EXPECTED[name]
    first, after, elsewhere = execute(lib, case, mode)
    if lanes:
        assert elsewhere > 0, "nothing was queued on the chain's second stream: the case proves nothing about it"
    for i, (w, f, a) in enumerate(zip(want, first, after)):
        differ = np.flatnonzero(f != w)
        assert differ.size == 0, ("output %d behind the sync of the caller's stream: %d of %d bytes differ from the synchronous run, the first at %d "
                                  "(%d of them still poison)" % (i, differ.size, w.size, differ[0], int((f[differ] == POISON).sum())))
        assert a.tobytes() == w.tobytes(), "output %d changed between the sync of the caller's stream and the drain" % i


# ---- process, then flush, on one caller stream ------------------------------------------------------------------------------
def process_flush(secs, feeds, streams="AAA", then=None, **kw):
    """process_device in calls of feeds[i] blocks (-1: the rest) and a flush, call i on stream streams[i] ('N': NULL);
    then: what the host calls last when the last stream is NULL ('reset' or 'get_rescale')"""
    def case(run):
        named = {k: run.stream() for k in sorted(set(streams)) if k != "N"}
        named["N"] = 0
        c = run.chan(secs, **kw)
        first = named[streams[0]]
        d_raw = run.late(secs, 1, first) if first else HostGuardedBuffer.from_numpy(frames(secs, 1))
        if not first:
            run.bufs.append(d_raw)
        info, nfr, nblocks = geometry(c, frames(secs, 1))
        out = run.out(nblocks * info.rows_per_block * info.row_bytes)
        rows = b0 = 0
        for feed, s in zip(feeds, streams):
            nb = nblocks - b0 if feed < 0 else feed
            assert 0 < nb <= nblocks - b0
            rows += c.process_device(d_raw.ptr.value, nfr, 8032, 32, b0 * info.block_stride_bytes, nb, out.ptr.value + rows * info.row_bytes,
                                     out.nbytes - rows * info.row_bytes, stream=named[s])
            b0 += nb
        assert b0 == nblocks and len(streams) == len(feeds) + 1
        last = named[streams[-1]]
        rows += c.flush_device(out.ptr.value + rows * info.row_bytes, out.nbytes - rows * info.row_bytes, stream=last)
        assert rows == nblocks * info.rows_per_block
        if not last:                                    # rows of a NULL-stream call: complete once reset / get_rescale has returned
            c.get_rescale() if then == "get_rescale" else c.reset()
        yield [out], last or None
        c.close()
    return case


SECS = 0.03                                             # 7 blocks of 4.096 ms
SINGLE = {
    # the interval ends inside the first call (two batches), the second call digitises as it goes (the fused path)
    "process_flush_interval_inside": process_flush(SECS, (4, -1), interval=0.006, maxb=2),
    # an interval per 1.5 blocks, measured again each time
    "process_flush_interval_each": process_flush(SECS, (4, -1), interval=0.006, const=0, maxb=2),
    # four products, the interval beyond the data: everything is digitised in the flush
    "process_flush_pol4_in_the_flush": process_flush(SECS, (3, -1), pol=4, maxb=2),
    # no rescale (-I 0): the digitiser reads the offset 0 / scale 1 that frbch_open queued on the handle's own stream
    "process_flush_no_rescale": process_flush(SECS, (4, -1), interval=0.0, maxb=2),
    # stream switches on one handle: between process_device and flush_device ...
    "switch_flush_A_B": process_flush(SECS, (-1,), "AB", maxb=2),
    "switch_flush_A_NULL": process_flush(SECS, (-1,), "AN", maxb=2),
    "switch_flush_A_NULL_get_rescale": process_flush(SECS, (-1,), "AN", then="get_rescale", maxb=2),
    "switch_flush_NULL_A": process_flush(SECS, (-1,), "NA", maxb=2),
    # ... and between two process_device calls of a handle that is measuring its interval
    "switch_process_A_B": process_flush(SECS, (3, -1), "ABB", interval=0.02, maxb=2),
    "switch_process_A_NULL": process_flush(SECS, (3, -1), "ANN", interval=0.02, maxb=2),
    "switch_process_NULL_A": process_flush(SECS, (3, -1), "NAA", interval=0.02, maxb=2),
    "switch_process_A_B_each_interval": process_flush(SECS, (3, -1), "ABA", interval=0.006, const=0, maxb=2),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_process_and_flush_in_stream_order(emu_lib, name, mode):
    hold(emu_lib, name, SINGLE[name], mode)


# ---- frbch_scan_device on a caller stream -----------------------------------------------------------------------------------
def scan(secs, flush, twice=False, null=False, tail=False, steady=False, streams="AA", pre=False, **kw):
    """three IFs through the chain in two calls (the second one flushes, or not) into one row buffer.  twice: a second pair of
    calls right behind on the same stream, other late inputs, a second row buffer, no host sync between.  null: on the NULL
    stream with the inputs in place, then get_rescale of the last handle and the resets, last handle first.  tail: a last call
    of no blocks that flushes.  streams: those of the two calls ('N': NULL; the resets follow when the second is).  pre: the first call is a frbch_process_device per handle
    into rows of its own instead (no chain: nothing but the caller's stream orders the scan behind it).  steady: offset / scale set beforehand, as bench.py's steady state has them"""
    def case(run):
        named = {k: run.stream() for k in sorted(set(streams)) if k != "N" and not null}
        A, B = (named.get(k, 0) for k in streams)
        chans = [run.chan(secs, bw=-BW if i % 2 else BW, **kw) for i in range(NIF)]
        info, nfr, nblocks = geometry(chans[0], frames(secs, 1))
        rows = nblocks * info.rows_per_block
        outs = []
        for i, c in enumerate(chans if steady else []):
            shape = (info.nif, NCHAN)
            c.set_rescale(np.full(shape, 10.0 + i, np.float32), np.full(shape, 0.5, np.float32))
        for rep in range(2 if twice else 1):
            if not A:                                   # a NULL-stream call: its inputs are complete beforehand
                bufs = [HostGuardedBuffer.from_numpy(frames(secs, i + 1 + 3 * rep)) for i in range(NIF)]
                run.bufs += bufs
            else:
                bufs = [run.late(secs, i + 1 + 3 * rep, A) for i in range(NIF)]
            ptrs = [b.ptr.value for b in bufs]
            out = run.out(rows * NIF * info.row_bytes)
            half = nblocks // 2
            if pre:
                got = 0
                for c, b in zip(chans, bufs):
                    outs.append(run.out(half * info.rows_per_block * info.row_bytes))
                    c.process_device(b.ptr.value, nfr, 8032, 32, 0, half, outs[-1].ptr.value, outs[-1].nbytes, stream=A)
            else:
                got = multi_if.scan_device(chans, ptrs, nfr, 8032, 32, 0, half, out.ptr.value, rows, flush=False, stream=A)
            got += multi_if.scan_device(chans, ptrs, nfr, 8032, 32, half * info.block_stride_bytes, nblocks - half,
                                        out.ptr.value + got * NIF * info.row_bytes, rows - got, flush=bool(flush), stream=B)
            if tail:
                got += multi_if.scan_device(chans, [0] * NIF, 0, 8032, 32, 0, 0, out.ptr.value + got * NIF * info.row_bytes, rows - got, flush=True, stream=A)
            assert got <= rows and (got == rows or not (flush or tail or steady) or pre)
            outs.append(out)
        if not null and not B:
            for c in chans:
                c.reset()
        if null:
            off, sc = chans[-1].get_rescale()           # the last handle first: its own stream is idle
            outs.append(run.out(off.nbytes + sc.nbytes))
            outs[-1]._poke(GUARD, np.concatenate([off.reshape(-1), sc.reshape(-1)]))
            for c in reversed(chans):
                c.reset()
        yield outs, B or None
        for c in chans:
            c.close()
    return case


CHAIN = dict(overlap=LANES, pol=5, flags=1 << 27)
SCANS = {}
for _flush in (0, 1):
    SCANS["scan_interval_inside_flush%d" % _flush] = scan(SECS, _flush, interval=0.006, maxb=2, **CHAIN)
SCANS["scan_interval_beyond_flush1"] = scan(SECS, 1, maxb=2, **CHAIN)
# an interval per 1.5 blocks: finalize_interval meets the digitiser of the interval before, still pending on the second stream
SCANS["scan_interval_each_flush1"] = scan(SECS, 1, interval=0.006, const=0, maxb=2, **CHAIN)
# ... and, at an interval of 0.73 blocks, the digitiser of the interval before in the same batch
SCANS["scan_intervals_within_a_batch"] = scan(SECS, 1, interval=0.003, const=0, maxb=2, **CHAIN)
# the stream changes between the two calls
SCANS["scan_switch_A_B"] = scan(SECS, 1, streams="AB", interval=0.006, const=0, maxb=2, **CHAIN)
SCANS["scan_switch_A_NULL"] = scan(SECS, 1, streams="AN", interval=0.006, const=0, maxb=2, **CHAIN)
SCANS["scan_switch_NULL_A"] = scan(SECS, 1, streams="NA", interval=0.006, const=0, maxb=2, **CHAIN)
SCANS["scan_behind_process_A_B"] = scan(SECS, 1, streams="AB", pre=True, interval=0.006, const=0, maxb=2, **CHAIN)
SCANS["scan_twice_interval_inside"] = scan(SECS, 0, twice=True, interval=0.006, maxb=2, **CHAIN)
SCANS["scan_twice_interval_each"] = scan(SECS, 1, twice=True, interval=0.006, const=0, maxb=2, **CHAIN)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(SCANS))
def test_scan_on_a_caller_stream(emu_lib, name, mode):
    hold(emu_lib, name, SCANS[name], mode, lanes=True)


def test_the_second_lane_assertion_fails_without_a_second_lane(emu_lib):
    """what test_scan_on_a_caller_stream asserts of every case is no formality: the same scan with the overlap off, a scan whose
    interval is still open behind the last front stage and a single handle all queue nothing on the chain's second stream (their
    handles' own streams and a second caller stream do hold ops), and a chain case queues a wait and a digitiser per interval"""
    off = dict(CHAIN, overlap=1)
    for name, case in (("overlap_off", scan(SECS, 1, interval=0.006, maxb=2, **off)), ("steady", PLAIN_SCANS["scan_twice_steady_state_flush0"]),
                       ("single", SINGLE["switch_flush_A_B"])):
        with pytest.raises(AssertionError, match="nothing was queued on the chain's second stream"):
            hold(emu_lib, "no_lane_" + name, case, 1, lanes=True)
        assert execute(emu_lib, case, 1)[2] == 0
    assert execute(emu_lib, SCANS["scan_interval_each_flush1"], 2)[2] >= 2 * 4     # (IFs 0 and 1: 4 intervals each in 7 blocks)


# no digitiser runs beside a K1 in these two: the interval is still open when the last front stage is queued; offset / scale are set
PLAIN_SCANS = {
    "scan_interval_beyond_flush0_then_flush": scan(SECS, 0, tail=True, maxb=2, **CHAIN),
    "scan_twice_steady_state_flush0": scan(SECS, 0, twice=True, steady=True, maxb=2, **CHAIN),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(PLAIN_SCANS))
def test_scan_on_a_caller_stream_without_a_second_lane(emu_lib, name, mode):
    hold(emu_lib, name, PLAIN_SCANS[name], mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,kw", [("null_scan_interval_beyond", dict(pol=5)),
                                     ("null_scan_chain_interval_each", dict(interval=0.006, const=0, maxb=2, **CHAIN))])
def test_null_stream_scan_then_the_last_handle_first(emu_lib, name, kw, mode):
    """tests/test_multi_if.py's test of the same name, on a schedule that can fail it: the rows and the last handle's offset /
    scale once get_rescale of the last handle and the resets, last handle first, have returned"""
    hold(emu_lib, name, scan(SECS, 1, twice=True, null=True, **kw), mode)


# ---- the taps ---------------------------------------------------------------------------------------------------------------
def power_tap(run):
    A = run.stream()
    c = run.chan(SECS, pol=4, maxb=2)
    d_raw = run.late(SECS, 1, A)
    info, nfr, nblocks = geometry(c, frames(SECS, 1))
    out = run.out(nblocks * info.rows_per_block * info.nif * NCHAN * 4)
    c.power_device(d_raw.ptr.value, nfr, 8032, 32, 0, nblocks, out.ptr.value, out.nbytes, stream=A)
    yield [out], A
    c.close()


def unpack_tap(run):
    A = run.stream()
    c = run.chan(SECS)
    d_raw = run.late(SECS, 1, A)
    out = run.out(2 * 1001 * 4)
    c.unpack_device(d_raw.ptr.value, d_raw.nbytes // 8032, 8032, 32, 7990, 1001, 0, out.ptr.value, out.nbytes, stream=A)
    yield [out], A
    c.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,case", [("power_tap", power_tap), ("unpack_tap", unpack_tap)])
def test_taps_on_a_caller_stream(emu_lib, name, case, mode):
    hold(emu_lib, name, case, mode)


# ---- behind and in front of the filterbank: host-synchronous ------------------------------------------------------------------
POST = ["dedisp_tiled_b8_nout1_ndm1", "dedisp_generic_48ch_b16_nout1_ndm1", "fold_c16_if1_b8_nbin2_plain", "spsearch_small_L64_w1",
        "cutout_lds_b16_1cand_ndm1_nf2_nt2", "rfi_fast_64ch_b8", "cornerturn_%s_1frames" % sorted(bc.ct.MODES)[0]]


@pytest.mark.parametrize("name", POST)
def test_post_entry_points_are_complete_on_return(emu_lib, name):
    """the smallest bounds case of every family on the lazy schedule with no sync by the test: the case's own == comparisons
    (the values mode 0 is held to in tests/test_bounds.py) on outputs it reads right behind the call"""
    assert name in bc.ids(emu_only=True)
    lib = hooks(emu_lib)
    lib.frbch_test_emu_set_mode(1)
    try:
        v0 = lib.frbch_test_emu_violations()
        bc.run(lib, name)
        assert lib.frbch_test_emu_pending() == 0 and lib.frbch_test_emu_violations() == v0
    finally:
        lib.frbch_test_emu_set_mode(0)


def test_mode_0_ignores_streams_and_leaves_nothing_pending(emu_lib):
    lib = hooks(emu_lib)
    assert lib.frbch_test_emu_mode() == 0
    a, b = lib.frbch_test_emu_stream_create(), lib.frbch_test_emu_stream_create()
    assert a == b == 1                                  # as before: one stream for all
    x, y = np.arange(16, dtype=np.uint8), np.zeros(16, np.uint8)
    lib.frbch_test_emu_memcpy_async(y.ctypes.data, x.ctypes.data, 16, a)
    assert np.array_equal(x, y) and lib.frbch_test_emu_pending() == 0


def test_the_scheduler_itself(emu_lib):
    """mode 1 leaves an unsynced stream pending, mode 2 runs it first; a wait takes the event's record at the time of the
    wait; a destroyed stream with work pending is counted"""
    lib = hooks(emu_lib)
    for mode in MODES:
        lib.frbch_test_emu_set_mode(mode)
        try:
            a, b = lib.frbch_test_emu_stream_create(), lib.frbch_test_emu_stream_create()
            assert a != b
            x, y, z = np.full(8, 1, np.uint8), np.zeros(8, np.uint8), np.zeros(8, np.uint8)
            lib.frbch_test_emu_memcpy_async(y.ctypes.data, x.ctypes.data, 8, a)
            x[:] = 2                                    # (the source was read at the call)
            lib.frbch_test_emu_memcpy_async(z.ctypes.data, x.ctypes.data, 8, b)
            assert lib.frbch_test_emu_pending() == 2 and not y.any() and not z.any()
            lib.frbch_test_emu_stream_sync(b)
            assert (z == 2).all() and (y == 1).all() == (mode == 2) and lib.frbch_test_emu_pending() == (mode == 1)
            v0 = lib.frbch_test_emu_violations()
            lib.frbch_test_emu_stream_destroy(a)
            assert lib.frbch_test_emu_violations() == v0 + (mode == 1) and (y == 1).all()
            lib.frbch_test_emu_stream_destroy(b)
            assert lib.frbch_test_emu_pending() == 0
        finally:
            lib.frbch_test_emu_set_mode(0)
