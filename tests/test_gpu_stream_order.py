"""Stream order of the device-resident entry points (the contract above them in include/frbch.h) on the real runtime: what
tests/test_stream_order.py holds on the emulator's adversary schedules, with time in place of the adversary.

On the caller's stream A a case queues, in this order: a stall (repeated hipMemsetAsync over a 1 GiB scratch buffer: plain
runtime work, no kernel of ours), the asynchronous copy that delivers the real frames into a buffer that held another IF's, the
library call or calls, and an asynchronous copy of every output into a poisoned snapshot.  Then hipStreamSynchronize(A) and
nothing wider; the snapshot is read without a device-wide sync (hipmem.StreamOrderBuffer) and compared with == against the
same sequence run synchronously (a hipDeviceSynchronize behind every step, timed with events once the kernels are loaded).  The host queues the calls in well under a
millisecond, so work that is not ordered behind A starts while the stall still runs -- before its input has arrived -- and work
that A does not wait for has not written its rows when the snapshot is taken.  The stall is sized per case: at least 10x the
device time of the synchronous run and at least 20 ms.  A control without any library code shows that an unordered copy does
overtake the stall on this runtime; if it cannot, the module's other results mean nothing and the control fails.

Sequences that end on the NULL stream are observed as the contract says: frbch_reset / frbch_get_rescale of every handle,
then the outputs themselves, read without a device-wide sync.  A racy result is a failing comparison on allocated memory."""
import functools
import math
import time

import numpy as np
import pytest

from frb_baseband_amd import channeliser as ch
from frb_baseband_amd import multi_if, synth
from tests import bounds_cases as bc
from tests import parity_util as pu
from tests.hipmem import H2D, POISON, DeviceBuffer, Event, GuardedBuffer, PinnedArray, Stream, StreamOrderBuffer, hip

pytestmark = pytest.mark.gpu

SCRATCH = 1 << 30
MIN_STALL_MS, STALL_FACTOR = 20.0, 10.0


class Ctx:
    """the module's streams, the scratch buffer of the stall and the measured time of one memset over it"""

    def __init__(self, lib):
        self.lib = lib
        self.A, self.B = Stream(), Stream()
        self.scratch = DeviceBuffer(SCRATCH)
        self.A.memset_async(self.scratch.ptr.value, 0, SCRATCH)        # (the first one pays for the runtime's set-up)
        self.A.synchronize()
        e0 = Event().record(self.A)
        for _ in range(8):
            self.A.memset_async(self.scratch.ptr.value, 0, SCRATCH)
        e1 = Event().record(self.A)
        self.memset_ms = e1.ms_since(e0) / 8
        e0.destroy()
        e1.destroy()
        print("\nstream order: one hipMemsetAsync over %d MiB takes %.3f ms" % (SCRATCH >> 20, self.memset_ms))
        assert self.memset_ms > 0.02, "the memset is too short to build a stall from"

    def stall(self, stream, ms):
        n = int(math.ceil(ms / self.memset_ms))
        for _ in range(n):
            stream.memset_async(self.scratch.ptr.value, 0, SCRATCH)
        return n

    def close(self):
        hip().hipDeviceSynchronize()
        self.A.destroy()
        self.B.destroy()
        self.scratch.free()


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = Ctx(hip_lib)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def vdif(secs, bw, nchan, if_index):
    raw = synth.make_vdif(secs, bw_mhz=bw, nchan=nchan, if_index=if_index)
    raw.setflags(write=False)
    return raw


def barrier():
    assert hip().hipDeviceSynchronize() == 0


class Run:
    """one execution of a case: ref = the synchronous one (a device-wide sync behind every step, device time summed),
    else the asynchronous one with `stall_ms` of memsets at the head of the first caller stream"""

    def __init__(self, ctx, ref, stall_ms=0.0):
        self.ctx, self.lib, self.ref, self.stall_ms = ctx, ctx.lib, ref, stall_ms
        self.bufs, self.pinned, self.snaps, self.pending = [], [], {}, {}
        self.ms = 0.0
        self.stalled = False
        self.ev = (Event(), Event())

    def stream(self, key):
        return {"A": self.ctx.A, "B": self.ctx.B, "N": None}[key]

    def begin(self, stream):
        """the stall, at the head of the first stream of the sequence (nothing can be queued in front of a NULL-stream call)"""
        if not self.ref and stream is not None and not self.stalled:
            self.ctx.stall(stream, self.stall_ms)
        self.stalled = True

    def out(self, nbytes):
        """a poisoned output, and (asynchronous run) the poisoned snapshot it is copied into: allocated before the stall"""
        self.bufs.append(StreamOrderBuffer(nbytes))
        if not self.ref:
            self.snaps[id(self.bufs[-1])] = StreamOrderBuffer(nbytes)
        return self.bufs[-1]

    def late(self, real, other, stream):
        """a frame buffer that holds `other` (another IF's frames) until deliver() queues `real` on `stream`; allocated before the stall"""
        assert real.nbytes == other.nbytes and real.tobytes() != other.tobytes()
        if self.ref or stream is None:
            buf = GuardedBuffer.from_numpy(real)
        else:
            buf = GuardedBuffer.from_numpy(other)
            self.pinned.append(PinnedArray(real))
            self.pending[id(buf)] = (self.pinned[-1], stream, real)
        self.bufs.append(buf)
        return buf

    def deliver(self, *bufs):
        for buf in bufs:
            if id(buf) in self.pending:
                pinned, stream, real = self.pending.pop(id(buf))
                stream.memcpy_async(buf.ptr.value, pinned.ptr.value, real.nbytes, H2D)
                buf.expect(real)

    def call(self, stream, fn):
        """one library call on `stream` (None: NULL)"""
        if not self.ref:
            return fn()
        barrier()
        t0 = time.perf_counter()
        if stream is not None:
            self.ev[0].record(stream)
        got = fn()
        if stream is not None:
            self.ev[1].record(stream)
            self.ms += self.ev[1].ms_since(self.ev[0])
        barrier()
        if stream is None:                              # (the handle's own stream takes no event of ours: host time to the device's idle)
            self.ms += (time.perf_counter() - t0) * 1e3
        return got

    def observe(self, outs, stream):
        if self.ref:
            barrier()
            return [o.to_numpy(np.uint8).copy() for o in outs]
        if stream is None:                              # the sequence ended in reset / get_rescale: the rows themselves
            return [o.to_numpy(np.uint8).copy() for o in outs]
        snaps = [self.snaps[id(o)] for o in outs]
        for s, o in zip(snaps, outs):
            stream.memcpy_async(s.ptr.value, o.ptr.value, o.nbytes)
        stream.synchronize()                            # the caller's stream, and nothing wider
        return [s.to_numpy(np.uint8).copy() for s in snaps]

    def done(self):
        barrier()
        assert not self.pending, "a late input was never delivered"
        for b in self.bufs + list(self.snaps.values()):
            b.check(contents=True)
        for b in self.bufs + list(self.snaps.values()):
            b.free()
        for p in self.pinned:
            p.free()
        for e in self.ev:
            e.destroy()


def execute(ctx, case, ref, stall_ms=0.0):
    run = Run(ctx, ref, stall_ms)
    gen = case(run)
    try:
        outs, last = next(gen)
        got = run.observe(outs, last)
        barrier()
        after = [o.to_numpy(np.uint8).copy() for o in outs]
        for _ in gen:                                   # the case closes its handles
            pass
        run.done()
    finally:
        barrier()
        for b in run.bufs + list(run.snaps.values()):
            b._release()
    return got, after, run.ms


def hold(ctx, name, case, refs=2):
    """refs = 2: the synchronous run a second time, because the first pays for loading the kernels while its events wait on the
    stream; 1 for a case that warms itself up before its first timed call"""
    t0 = time.perf_counter()
    want, again, cold_ms = execute(ctx, case, True)
    warm, _again, ref_ms = execute(ctx, case, True) if refs == 2 else (want, again, cold_ms)
    ref_ms = min(ref_ms, cold_ms)
    for w, a, b in zip(want, again, warm):
        assert w.tobytes() == a.tobytes() == b.tobytes(), "two synchronous runs of the sequence differ"
    assert any((w != POISON).any() for w in want), "the sequence wrote nothing: the case proves nothing"
    stall_ms = max(MIN_STALL_MS, STALL_FACTOR * ref_ms)
    got, after, _ms = execute(ctx, case, False, stall_ms)
    print("\nstream order %s: synchronous run %.3f ms of device time, stall %.1f ms (%d memsets of %.3f ms), case %.2f s"
          % (name, ref_ms, stall_ms, math.ceil(stall_ms / ctx.memset_ms), ctx.memset_ms, time.perf_counter() - t0))
    for i, (w, g, a) in enumerate(zip(want, got, after)):
        differ = np.flatnonzero(g != w)
        assert differ.size == 0, ("output %d behind the sync of the caller's stream: %d of %d bytes differ from the synchronous run, the first at %d "
                                  "(%d of them still poison)" % (i, differ.size, w.size, differ[0], int((g[differ] == POISON).sum())))
        assert a.tobytes() == w.tobytes(), "output %d differs from the synchronous run once the device is idle" % i


# ---- the control: no library code -----------------------------------------------------------------------------------------
def _control(ctx, ordered):
    n = 1 << 20
    x = np.random.default_rng(5).integers(0, 256, n, dtype=np.uint8)
    d_x, d_y, d_z = GuardedBuffer.from_numpy(x), StreamOrderBuffer(n), StreamOrderBuffer(n)
    barrier()
    nset = ctx.stall(ctx.A, 3 * MIN_STALL_MS)
    ctx.A.memcpy_async(d_y.ptr.value, d_x.ptr.value, n)
    ev = Event().record(ctx.A)
    if ordered:
        ctx.B.wait(ev)
    ctx.B.memcpy_async(d_z.ptr.value, d_y.ptr.value, n)
    ctx.B.synchronize()
    z = d_z.to_numpy(np.uint8).copy()                   # (a read that does not wait for A)
    a_was_done = ev.done()
    barrier()
    y = d_y.to_numpy(np.uint8).copy()
    ev.destroy()
    for b in (d_x, d_y, d_z):
        b.free()
    return x, y, z, a_was_done, nset


def test_control_an_unordered_copy_overtakes_the_stall(ctx):
    """X -> Y on A behind the stall, Y -> Z on B with no event between, B synchronised: Z is what Y held before -- poison.  With an
    event wait Z is X.  Without the first half nothing in this module could see a missing edge."""
    x, y, z, a_was_done, nset = _control(ctx, ordered=False)
    print("\nstream order control: %d memsets of %.3f ms in front; A %s when Z had been read" % (nset, ctx.memset_ms, "had finished" if a_was_done else "was still running"))
    assert np.array_equal(y, x)
    assert not a_was_done, "the stall had run out (or the read waited for stream A) before Z was read: the method cannot see an overtaking"
    assert np.all(z == POISON), "the unordered copy did NOT overtake the stall: %d of %d bytes of Z are X's" % (int((z == x).sum()), z.size)
    x, y, z, _done, _n = _control(ctx, ordered=True)
    assert np.array_equal(y, x) and np.array_equal(z, x)


# ---- frbch_process_device / frbch_flush_device ------------------------------------------------------------------------------
def _names(c):
    return set(c.get_launch_record())


def process_flush(bw, nchan, secs, feeds, streams, families, **kw):
    """process_device in calls of feeds[i] blocks (-1: the rest) and a flush; call i on streams[i] ('A', 'B', 'N': NULL)"""
    def case(run):
        real, other = vdif(secs, bw, nchan, 0), vdif(secs, bw, nchan, 5)
        with ch.Channeliser(pu.lib_cfg(run.lib, bw, nchan, secs, **kw), run.lib) as c:
            c.set_profiling(True)
            info = c.info
            nfr = real.size // 8032
            nblocks = (nfr * 8000) // info.block_payload_bytes
            first, last = run.stream(streams[0]), run.stream(streams[-1])
            out = run.out(nblocks * info.rows_per_block * info.row_bytes)
            d_raw = run.late(real, other, first)
            barrier()
            run.begin(first)
            run.deliver(d_raw)
            rows = b0 = 0
            assert len(streams) == len(feeds) + 1
            for feed, key in zip(feeds, streams):
                nb = nblocks - b0 if feed < 0 else feed
                assert 0 < nb <= nblocks - b0
                run.begin(run.stream(key))
                s = run.stream(key)
                rows += run.call(s, lambda: c.process_device(d_raw.ptr.value, nfr, 8032, 32, b0 * info.block_stride_bytes, nb,
                                                             out.ptr.value + rows * info.row_bytes, out.nbytes - rows * info.row_bytes,
                                                             stream=s.handle if s else 0))
                b0 += nb
            assert b0 == nblocks
            run.begin(last)
            rows += run.call(last, lambda: c.flush_device(out.ptr.value + rows * info.row_bytes, out.nbytes - rows * info.row_bytes,
                                                          stream=last.handle if last else 0))
            assert rows == nblocks * info.rows_per_block
            if last is None:                            # rows of a NULL-stream call: complete once reset has returned
                c.reset()
            yield [out], last
            names = _names(c)
            assert bc._holds(names, families) and not bc.FALLBACKS & names, sorted(names)
    return case


TWOPASS = dict(flags=1 << 28, pol=4, tscr=2, nbit=16, maxb=3)
SWITCH = dict(pol=4, maxb=2)
SINGLE = {
    # the two-pass deferred sequences of tests/bounds_cases.py: 3 + 1 blocks (the second call materialises the deferred batch) ...
    "process_1024ch_twopass_pol4_t2_16bit_maxb3": process_flush(32.0, 1024, 0.27, (3, -1), "AAA", bc.PRIV, **TWOPASS),
    # ... and the interval that ends inside the batch
    "process_1024ch_twopass_t4_2bit_interval": process_flush(32.0, 1024, 0.27, (-1,), "AA", bc.PRIV, flags=1 << 28, pol=2, tscr=4, nbit=2,
                                                             interval=0.1, maxb=2),
    # buffered, an interval per 10 ms
    "process_128ch_buffered_interval_each": process_flush(16.0, 128, 0.05, (-1,), "AA", ["frbch_k1_wave", "frbch_k2_"], interval=0.01, const=0, maxb=2),
    # the stream changes between process_device and flush_device ...
    "switch_flush_A_B": process_flush(32.0, 1024, 0.27, (-1,), "AB", ["frbch_k1_wave", "frbch_k2_"], **SWITCH),
    "switch_flush_A_NULL": process_flush(32.0, 1024, 0.27, (-1,), "AN", ["frbch_k1_wave", "frbch_k2_"], **SWITCH),
    # (NULL -> A, here and below: WEAKER than the others.  Nothing can be queued in front of a NULL-stream call, so there is no
    # stall; a missing edge shows only while the first call's own work outlasts the host's next call.  A green result is not the
    # evidence the A -> NULL results are: the edge is held deterministically by tests/test_stream_order.py's cases of the same name)
    "switch_flush_NULL_A": process_flush(32.0, 1024, 0.27, (-1,), "NA", ["frbch_k1_wave", "frbch_k2_"], **SWITCH),
    # ... and between two process_device calls of a handle that is measuring its interval
    "switch_process_A_B": process_flush(32.0, 1024, 0.27, (2, -1), "ABB", ["frbch_k1_wave", "frbch_k2_"], **SWITCH),
    "switch_process_A_NULL": process_flush(32.0, 1024, 0.27, (2, -1), "ANN", ["frbch_k1_wave", "frbch_k2_"], **SWITCH),
    "switch_process_NULL_A": process_flush(32.0, 1024, 0.27, (2, -1), "NAA", ["frbch_k1_wave", "frbch_k2_"], **SWITCH),
}


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_process_and_flush_in_stream_order(ctx, name):
    hold(ctx, name, SINGLE[name])


# ---- frbch_scan_device ----------------------------------------------------------------------------------------------------
NIF = 3


def scan(overlap, families, null=False, steady=False, **kw):
    """3 IFs x 32 MHz -> 1024 channels, 0.27 s: a scan, and a second one right behind it on the same stream with other late
    inputs into a second row buffer.  steady: offset / scale measured by a first, synchronous scan and set again behind a
    reset, then two scans with flush = 0 (bench.py's steady state).  null: on the NULL stream with the inputs in place, then
    reset() of every handle (bench.py's step)"""
    def case(run):
        bw, nchan, secs = 32.0, 1024, 0.27
        raws = [vdif(secs, bw, nchan, i + 1) for i in range(2 * NIF + 1)]
        chans = []
        for i in range(NIF):
            cfg = pu.lib_cfg(run.lib, bw if i % 2 else -bw, nchan, secs, **kw)
            cfg.overlap = overlap
            chans.append(ch.Channeliser(cfg, run.lib))
            chans[-1].set_profiling(True)
        info = chans[0].info
        nfr = raws[0].size // 8032
        nblocks = (nfr * 8000) // info.block_payload_bytes
        rows = nblocks * info.rows_per_block
        A = None if null else run.stream("A")
        outs = [run.out(rows * NIF * info.row_bytes) for _ in range(2)]
        late = [[run.late(raws[rep * NIF + i], raws[rep * NIF + i + 1], A) for i in range(NIF)] for rep in range(2)]
        # a first, synchronous scan and a reset: the kernels are loaded and every handle has its power buffer (gigabytes at an interval
        # of 10 s: a quarter of a second of hipMalloc per handle) before the stall is queued -- the host must not take longer to queue
        # the calls than the stall lasts.  steady: its offset / scale are set again behind the reset
        bufs = [GuardedBuffer.from_numpy(raws[i]) for i in range(NIF)]
        first = GuardedBuffer(outs[0].nbytes)
        run.bufs += bufs + [first]
        assert multi_if.scan_device(chans, [b.ptr.value for b in bufs], nfr, 8032, 32, 0, nblocks, first.ptr.value, rows) == rows
        scales = [c.get_rescale() for c in chans]
        for c, (off, sc) in zip(chans, scales):
            c.reset()
            if steady:
                c.set_rescale(off, sc)
        barrier()
        run.begin(A)
        for rep, out in enumerate(outs):
            bufs = late[rep]
            run.deliver(*bufs)
            got = run.call(A, lambda: multi_if.scan_device(chans, [b.ptr.value for b in bufs], nfr, 8032, 32, 0, nblocks, out.ptr.value, rows,
                                                           flush=not steady, stream=A.handle if A else 0))
            assert got == rows
        if null:
            for c in chans:
                c.reset()
        yield outs, A
        for c in chans:
            names = _names(c)
            assert bc._holds(names, families) and not bc.FALLBACKS & names, sorted(names)
            c.close()
    return case


WAVE, PRIV = ["frbch_k1_wave", "frbch_k2_wave"], ["frbch_k1_wave", "frbch_k2_priv"]
SCANS = {       # the four parameter sets of tests/test_gpu_pins.py::test_scan_device_lanes_give_the_same_rows
    "scan_lanes_buffered_pol5": scan(192 | (3 << 24), WAVE, pol=5, flags=1 << 27),
    "scan_lanes_interval_each_pol2": scan(160 | (3 << 24), ["frbch_k1_wave", "frbch_k2_"], pol=2, interval=0.1, const=0, maxb=2),
    "scan_automatic_interval_inside_pol5": scan(0, WAVE, pol=5, interval=0.1, maxb=2, flags=1 << 27),
    "scan_automatic_twopass_pol5": scan(0, PRIV, pol=5),
    # ... the steady state, and the NULL-stream step
    "scan_steady_state_flush0": scan(0, ["frbch_k1_wave", "frbch_k2_"], steady=True, pol=5),
    "scan_null_stream_then_reset": scan(0, ["frbch_k1_wave", "frbch_k2_"], null=True, pol=5, interval=0.1, maxb=2, flags=1 << 27),
}


@pytest.mark.parametrize("name", sorted(SCANS))
def test_scan_in_stream_order(ctx, name):
    hold(ctx, name, SCANS[name], refs=1)


# ---- the taps ---------------------------------------------------------------------------------------------------------------
def power_tap(run):
    bw, nchan = 32.0, 1024
    with ch.Channeliser(pu.lib_cfg(run.lib, bw, nchan, 10.0, pol=5, tscr=4), run.lib) as c:
        info = c.info
        real, other = bc._raw_for(bw, nchan, 3, info), bc._raw_for(bw, nchan, 3, info, if_index=5)
        A = run.stream("A")
        out = run.out(3 * info.rows_per_block * info.nif * nchan * 4)
        d_raw = run.late(real, other, A)
        barrier()
        run.begin(A)
        run.deliver(d_raw)
        run.call(A, lambda: c.power_device(d_raw.ptr.value, real.size // 8032, 8032, 32, 0, 3, out.ptr.value, out.nbytes, stream=A.handle))
        yield [out], A


def unpack_tap(run):
    real, _p = bc._frames(2)
    other = real.copy()
    other[32:] ^= 0x55                                  # (the same frames with every payload byte changed)
    with ch.Channeliser(ch.new_config(run.lib, bw_mhz=32.0, nchan=64, input_bits=2), run.lib) as c:
        A = run.stream("A")
        outs = [run.out(2 * 257 * 4), run.out(4 * 514 * 4)]
        d_raw = run.late(real, other, A)
        barrier()
        run.begin(A)
        run.deliver(d_raw)
        run.call(A, lambda: c.unpack_device(d_raw.ptr.value, 3, 8032, 32, 7990, 257, 0, outs[0].ptr.value, outs[0].nbytes, stream=A.handle))
        run.call(A, lambda: c.unpack_device(d_raw.ptr.value, 3, 8032, 32, 7988, 514, 1, outs[1].ptr.value, outs[1].nbytes, stream=A.handle))
        yield outs, A


@pytest.mark.parametrize("name,case", [("power_tap", power_tap), ("unpack_tap", unpack_tap)])
def test_taps_in_stream_order(ctx, name, case):
    hold(ctx, name, case)


# ---- behind and in front of the filterbank: host-synchronous ------------------------------------------------------------------
POST = [n for n in bc.ids() if n.split("_")[0] in ("dedisp", "fold", "spsearch", "cutout", "rfi", "cornerturn")]


def test_the_post_cases_are_all_here():
    assert len(POST) == 66


@pytest.mark.parametrize("name", POST)
def test_post_entry_points_are_complete_on_return(hip_lib, name):
    """the bounds case as it is (the same == comparisons, guards and poison), its buffers read without a device-wide sync:
    what the call left in its outputs when it returned"""
    bc.run(hip_lib, name, StreamOrderBuffer)
