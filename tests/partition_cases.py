"""How a stream is cut must not show in the rows: shared cases of tests/test_partition.py (emulator build) and
tests/test_gpu_partition.py (device).  A plain module: cut generators, drivers over the C ABI that work with either library
(emulator: host pointers; device: tests/hipmem.GuardedBuffer) and the assertions both test modules hold a configuration to.
Everything is library against library and byte for byte; no oracle runs here.

Cuts of a BYTE STREAM for frbch_push (lists of piece lengths that concatenate to the stream): PUSH_CUTS.
Cuts of a RUN OF BLOCKS for the device entry points (lists of block counts): DEVICE_CUTS.

The assertions, for one configuration K (hold()):  W = the `whole` push run with its interval measured, S_W its get_rescale().
  (a) frozen: every cut of every route with set_rescale(S_W) first gives the header and the row bytes of the `whole` push run with
      set_rescale(S_W); -I0 configurations the same without a scale.  No statistics are taken: nothing but identity is acceptable.
  (b) measured: every cut of every route without a scale gives rows M_R and a scale S_R; the `whole` push run with
      set_rescale(S_R) gives M_R byte for byte ("the SAME float arithmetic in both passes", frbch_stream.cpp).
  (c) scale: S_R against S_W within twice the bounds tests/test_gpu_pins.py holds a measured pair to against the fp64 moments of
      the same floats (two runs within a bound are within twice it); bit for bit where the statistics cannot depend on the cut
      (exact=True: every emulator run, every run with flag 1 << 20).
  (d) power tap: frbch_power_device per block against one call over the run, identical floats.
  (e) a rescale per interval (const=0: get_rescale returns the last pair only, (a) and (b) do not apply): with exact statistics
      the rows and the last pair are identical across all cuts; else codes differ by at most 1 in fewer than 1e-4 of the values.
  (f) no silent fallback: a cut launches no generic kernel of a stage that W did not launch.
Every run checks its row count and, for the device routes, the guards of every buffer it handed out."""
import os
from collections import namedtuple

import numpy as np

from frb_baseband_amd import channeliser as ch
from frb_baseband_amd import multi_if, sigproc, synth
from tests import parity_util as pu
from tests.hipmem import guarded_for

RAGGED_SEEDS = (11, 12)
OFF_ATOL_REL = 2 * 4e-7                # (c): twice tests/test_gpu_pins.py's bound on the offset ...
SCALE_RTOL = 2 * 2e-6                  # ... and on the scale
PER_INTERVAL_FRAC = 1e-4               # (e): the bound of test_statistics_summed_by_k2_equal_the_separate_pass
SEPARATE_STATS = 1 << 20
GENERIC_OF_A_STAGE = ("frbch_k1_branch", "frbch_kc_dcfix", "frbch_k2_chan")


# ---- cuts of a byte stream ----------------------------------------------------------------------------------------------------
def _pieces(total, cuts):
    """piece lengths from cut positions (sorted, deduplicated, strictly inside the stream)"""
    at = sorted({int(c) for c in cuts if 0 < c < total})
    edges = [0] + at + [total]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


def cut_whole(total, **_geo):
    return [total]


def cut_per_frame(total, frame_bytes, **_geo):
    return _pieces(total, range(frame_bytes, total, frame_bytes))


def cut_ragged(total, frame_bytes, header_bytes, seed=RAGGED_SEEDS[0], **_geo):
    """seeded lengths between 1 byte and 3 frames, not frame-aligned: a quarter of them shorter than a header, a quarter longer
    than a frame"""
    rng = np.random.default_rng(seed)
    out, left = [], total
    while left:
        kind = int(rng.integers(0, 4))
        lo, hi = (1, header_bytes - 1) if kind == 0 else ((frame_bytes + 1, 3 * frame_bytes) if kind == 1 else (1, 3 * frame_bytes))
        n = min(left, int(rng.integers(lo, hi + 1)))
        out.append(n)
        left -= n
    return out


def cut_headers(total, frame_bytes, header_bytes, **_geo):
    """every cut falls 1 .. header_bytes - 1 bytes into a frame header (a frame is looked at once its whole header is there)"""
    return _pieces(total, [k * frame_bytes + 1 + (7 * k + 4) % (header_bytes - 1) for k in range(total // frame_bytes + 1)])


def block_edge_bytes(total, frame_bytes, header_bytes, skip, block_stride_bytes, **_geo):
    """stream byte of the payload byte skip + k * block_stride_bytes, k = 1, 2, ...: where a block starts"""
    pb = frame_bytes - header_bytes
    out, k = [], 1
    while True:
        e = skip + k * block_stride_bytes
        at = e // pb * frame_bytes + header_bytes + e % pb
        if at + 1 >= total:
            return out
        out.append(at)
        k += 1


def cut_block_edges(total, **geo):
    return _pieces(total, [e + d for e in block_edge_bytes(total, **geo) for d in (-1, 0, 1)])


def cut_last_byte(total, **_geo):
    return [total - 1, 0, 1]


PUSH_CUTS = {"whole": cut_whole, "per_frame": cut_per_frame, "ragged": cut_ragged, "headers": cut_headers,
             "block_edges": cut_block_edges, "last_byte": cut_last_byte}


# ---- cuts of a run of blocks --------------------------------------------------------------------------------------------------
def device_cuts(nblocks):
    """name -> block counts per call (cuts that coincide on a short run are listed once)"""
    cuts = {"whole": [nblocks], "per_block": [1] * nblocks, "one_then_rest": [1, nblocks - 1], "rest_then_one": [nblocks - 1, 1]}
    out, seen = {}, set()
    for name, cut in cuts.items():
        cut = [n for n in cut if n > 0]
        if tuple(cut) not in seen:
            seen.add(tuple(cut))
            out[name] = cut
    return out


DEVICE_CUTS = ("whole", "per_block", "one_then_rest", "rest_then_one")


def batches(nblocks, maxb):
    """block counts of the launches plan_batches (frbch_stream.cpp) cuts one run of blocks into"""
    if not nblocks:
        return []
    nb = max(1, min(-(-nblocks // maxb), nblocks))
    per = -(-nblocks // nb)
    return [min(per, nblocks - b0) for b0 in range(0, nblocks, per)]


def launch_edges(calls, maxb):
    """block index at which every launch of a sequence of calls (block counts) ends"""
    out, at = [], 0
    for nblocks in calls:
        for nb in batches(nblocks, maxb):
            at += nb
            out.append(at)
    return out


def check_interval_ends(info, nblocks, maxb):
    """what (e) asks of its stream, from the library's own geometry: at least three intervals, and one of them ends strictly
    inside a launch of the `whole` push (which hands the engine maxb blocks at a time) and on a launch boundary when every call
    carries one block"""
    rpb, ir = int(info.rows_per_block), int(info.rescale_interval_rows)
    ends = [j * ir for j in range(1, nblocks * rpb // ir + 1)]
    whole = {e * rpb for e in launch_edges([maxb] * (nblocks // maxb) + [nblocks % maxb], maxb)}
    per_block = {b * rpb for b in range(1, nblocks + 1)}
    assert ir > 0 and len(ends) >= 3, f"{len(ends)} intervals of {ir} rows in {nblocks} blocks of {rpb}"
    assert any(e not in whole and e in per_block for e in ends), (ends, sorted(whole), rpb)


# ---- a configuration ----------------------------------------------------------------------------------------------------------
class Config:
    """bw, nchan, secs, kw in the vocabulary of parity_util.run_streaming_case; what of kw makes the STREAM (bits, payload_bytes,
    legacy, frames) is split from what makes the library's configuration"""

    def __init__(self, bw, nchan, secs, kw, frames=None, if_index=0, overlap=0, total=None, raw=None):
        kw = dict(kw)
        self.bw, self.nchan, self.secs = bw, nchan, secs
        self.gen = {k: kw.pop(k) for k in ("bits", "payload_bytes", "legacy") if k in kw}
        self.frames = frames or kw.pop("frames", None)
        self.kw, self.if_index, self.overlap = kw, if_index, overlap
        self.total = secs if total is None else total          # -T
        self.bits = self.gen.get("bits", 2)
        self.header_bytes = 16 if self.gen.get("legacy") else 32
        self.frame_bytes = self.gen.get("payload_bytes", 8000) + self.header_bytes
        self._raw = raw

    @property
    def raw(self):
        if self._raw is None:
            raw = synth.make_vdif(self.secs + self.kw.get("start", 0.0), bw_mhz=abs(self.bw), nchan=self.nchan,
                                  **self.gen, **({"if_index": self.if_index} if self.if_index else {}))
            if self.frames:
                raw = pu.hurt_frames(raw, self.frames, self.frame_bytes)
            self._raw = np.ascontiguousarray(raw)
        return self._raw

    @property
    def measures(self):
        return self.kw.get("interval", 10.0) > 0

    @property
    def per_interval(self):
        return self.measures and not self.kw.get("const", 1)

    @property
    def push_only(self):
        """the device entry points read neither the invalid bit nor a 1-bit stream opened with input_bits = 0"""
        return bool(self.frames) or self.bits != 2

    @property
    def skip(self):
        """payload bytes -S skips (stream_begin, frbch_file.cpp)"""
        spb = 4 // self.bits
        s0 = int(round(self.kw.get("start", 0.0) * 2.0e6 * abs(self.bw)))
        return (s0 - s0 % spb) // spb

    def open(self, lib, maxb=None):
        kw = dict(self.kw)
        if maxb is not None:
            kw["maxb"] = maxb
        cfg = pu.lib_cfg(lib, self.bw, self.nchan, self.total, **kw)
        cfg.overlap = self.overlap
        return ch.Channeliser(cfg, lib)

    def geometry(self, info):
        """what the byte cuts need, from the info of a handle that has seen the stream"""
        return dict(frame_bytes=self.frame_bytes, header_bytes=self.header_bytes, skip=self.skip,
                    block_stride_bytes=int(info.block_stride_bytes))


def per_interval_config(bw, nchan, kw, flags, blocks=5.3):
    """a configuration for (e): a rescale per interval, an interval of a block and a half, a stream of `blocks` blocks (cut to whole
    frames), two blocks per launch"""
    freq_res = kw.get("freq_res", 0) or (512 if nchan <= 128 else 2 * nchan)
    tscr = kw.get("tscr", 1)
    block_s = 2.0 * nchan * freq_res / (2.0e6 * abs(bw))
    rate_out = abs(bw) * 1.0e6 / (nchan * tscr)
    interval = (freq_res // tscr * 3 // 2 + 0.5) / rate_out        # (the library truncates interval x rate to rows)
    return Config(bw, nchan, round(blocks * block_s, 6), dict(kw, interval=interval, const=0, maxb=2, flags=flags))


Result = namedtuple("Result", "header rows rescale record nrows")


def _begin(c, frozen):
    c.reset()
    c.timing_reset()                                            # (the launch record starts empty)
    c.set_profiling(True)
    if frozen is not None:
        c.set_rescale(*frozen)


def _end(c, header, rows, nrows):
    info = c.get_info()
    resc = c.get_rescale() if info.have_rescale and info.rescale_interval_rows else None
    return Result(header, bytes(rows), resc, c.get_launch_record(), nrows)


# ---- drivers ------------------------------------------------------------------------------------------------------------------
def run_push(c, raw, cut, frozen=None):
    """push / flush / pull, pull() behind every push"""
    assert sum(cut) == raw.size
    _begin(c, frozen)
    pos, body = 0, bytearray()
    for n in cut:
        c.push(raw[pos:pos + n])
        pos += n
        body += c.pull(1 << 24)
    c.flush()
    while True:
        chunk = c.pull(1 << 24)
        if not chunk:
            break
        body += chunk
    info = c.get_info()
    assert len(body) == info.rows_out * info.row_bytes
    return _end(c, c.sigproc_header(), body, info.rows_out)


def run_file(c, path, out_path, frozen=None):
    """frbch_run_file into a regular file"""
    _begin(c, frozen)
    if os.path.exists(out_path):
        os.unlink(out_path)
    c.run_file(path, out_path)
    data = open(out_path, "rb").read()
    nh = sigproc.read_fil(data).header_bytes
    info = c.get_info()
    assert len(data) - nh == info.rows_out * info.row_bytes
    return _end(c, data[:nh], data[nh:], info.rows_out)


class DeviceRun:
    """the frames of one configuration on the device (the emulator: guarded host memory) and the geometry of its run of blocks"""

    def __init__(self, lib, K, info, nblocks):
        self.cls = guarded_for(lib)
        self.frames = self.cls.from_numpy(K.raw)
        self.nfr = K.raw.size // K.frame_bytes
        self.fb, self.hb, self.skip = K.frame_bytes, K.header_bytes, K.skip
        self.stride, self.rpb, self.row_bytes = int(info.block_stride_bytes), int(info.rows_per_block), int(info.row_bytes)
        self.ncol = int(info.nif) * int(info.nchan)
        self.nblocks = nblocks
        self.rows = nblocks * self.rpb

    def check(self, *outs):
        for o in outs:
            o.check()
        self.frames.check(contents=True)

    def free(self):
        self.frames.free()


def run_device(c, d, cut, frozen=None):
    """frbch_process_device per piece of the cut, the rows of a call behind those of the calls before it; frbch_flush_device last"""
    assert sum(cut) == d.nblocks
    _begin(c, frozen)
    out = d.cls(d.rows * d.row_bytes)
    rows = b0 = 0
    for nb in cut:
        rows += c.process_device(d.frames.ptr.value, d.nfr, d.fb, d.hb, d.skip + b0 * d.stride, nb,
                                 out.ptr.value + rows * d.row_bytes, out.nbytes - rows * d.row_bytes)
        b0 += nb
    rows += c.flush_device(out.ptr.value + rows * d.row_bytes, out.nbytes - rows * d.row_bytes)
    assert rows == d.rows == c.get_info().rows_out
    res = _end(c, None, out.to_numpy(np.uint8).tobytes(), rows)
    d.check(out)
    out.free()
    return res


def run_power(c, d, cut):
    """frbch_power_device per piece of the cut: float32 [t][nif][chan] of the whole run"""
    assert sum(cut) == d.nblocks
    _begin(c, None)
    out = d.cls(d.rows * d.ncol * 4)
    b0 = 0
    for nb in cut:
        at = b0 * d.rpb * d.ncol * 4
        c.power_device(d.frames.ptr.value, d.nfr, d.fb, d.hb, d.skip + b0 * d.stride, nb, out.ptr.value + at, out.nbytes - at)
        b0 += nb
    res = Result(None, out.to_numpy(np.uint8).tobytes(), None, c.get_launch_record(), d.rows)
    d.check(out)
    out.free()
    return res


def run_scan(chans, ds, cut, frozen=None):
    """frbch_scan_device over the IFs of `chans`: the cut's calls with flush off, then a call of no blocks that flushes.
    -> one Result per IF (its columns of the scan's rows)"""
    nif, d = len(chans), ds[0]
    assert sum(cut) == d.nblocks
    for i, c in enumerate(chans):
        _begin(c, None if frozen is None else frozen[i])
    out = d.cls(d.rows * nif * d.row_bytes)
    ptrs = [x.frames.ptr.value for x in ds]
    rows = b0 = 0
    for nb in list(cut) + [0]:
        rows += multi_if.scan_device(chans, ptrs if nb else [0] * nif, d.nfr if nb else 0, d.fb, d.hb, d.skip + b0 * d.stride if nb else 0, nb,
                                     out.ptr.value + rows * nif * d.row_bytes, d.rows - rows, flush=not nb)
        b0 += nb
    assert rows == d.rows
    nprod = int(chans[0].info.nif)
    seg = d.row_bytes // nprod
    data = out.to_numpy(np.uint8).reshape(rows, nprod, nif, seg)
    res = [_end(c, None, np.ascontiguousarray(data[:, :, i, :]).tobytes(), rows) for i, c in enumerate(chans)]
    for x in ds:
        x.check(out)
    out.free()
    return res


# ---- the assertions -----------------------------------------------------------------------------------------------------------
def _same_pair(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def check_scale(s_r, s_w, exact, what):
    """(c)"""
    if exact:
        assert _same_pair(s_r, s_w), f"{what}: offset / scale differ from the whole push run's, where the statistics cannot depend on the cut"
        return
    assert np.abs(s_r[0] - s_w[0]).max() <= OFF_ATOL_REL * np.abs(s_w[0]).max(), f"{what}: offset"
    np.testing.assert_allclose(s_r[1], s_w[1], rtol=SCALE_RTOL, err_msg=f"{what}: scale")


def check_record(rec, rec_w, what):
    """(f)"""
    for name in GENERIC_OF_A_STAGE:
        assert name not in rec or name in rec_w, f"{what}: launched {name}, which the whole push run did not: {sorted(rec)}"


def _differing(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    bad = np.flatnonzero(a != b)
    return "%d of %d bytes differ, the first at %d" % (bad.size, a.size, bad[0]) if bad.size else "equal"


def check_codes_close(got, want, nbit, what):
    """(e) without exact statistics: codes differ by at most 1 in fewer than PER_INTERVAL_FRAC of the values"""
    assert len(got) == len(want) and nbit != -32, what
    a = sigproc.unpack_samples(got, nbit).astype(np.int64)
    b = sigproc.unpack_samples(want, nbit).astype(np.int64)
    d = np.abs(a - b)
    assert d.max() <= 1, f"{what}: a code differs by {d.max()}"
    assert np.count_nonzero(d) < PER_INTERVAL_FRAC * d.size, f"{what}: {np.count_nonzero(d)} of {d.size} codes differ"


class Reference:
    """the `whole` push runs of one configuration: W (measured) and, per scale, the frozen run -- each computed once"""

    def __init__(self, c, K):
        self.c, self.K = c, K
        self.W = run_push(c, K.raw, [K.raw.size])
        assert self.W.nrows > 0, "the configuration delivers no rows: the case proves nothing"
        assert (self.W.rescale is not None) == K.measures
        self._frozen = {}
        if not K.measures:
            self._frozen[None] = self.W

    def frozen(self, scale):
        key = None if scale is None else scale[0].tobytes() + scale[1].tobytes()
        if key not in self._frozen:
            self._frozen[key] = run_push(self.c, self.K.raw, [self.K.raw.size], frozen=scale)
        return self._frozen[key]


def hold(ref, run, what, exact, has_header=True):
    """(a), (b), (c), (f) -- or (e) -- for one cut of one route: run(frozen) -> Result"""
    K, W = ref.K, ref.W
    if K.per_interval:
        r = run(None)
        assert r.nrows == W.nrows, f"{what}: {r.nrows} rows, the whole push run {W.nrows}"
        check_record(r.record, W.record, what)
        if exact:
            assert r.rows == W.rows, f"{what}: rows of a per-interval rescale, {_differing(r.rows, W.rows)}"
            assert _same_pair(r.rescale, W.rescale), f"{what}: the last offset / scale differ"
        else:
            check_codes_close(r.rows, W.rows, K.kw.get("nbit", 8), what)
            check_scale(r.rescale, W.rescale, False, what)
        if has_header:
            assert r.header == W.header, f"{what}: header"
        return
    s_w = W.rescale
    f_w = ref.frozen(s_w)
    # (a)
    r = run(s_w)
    assert r.nrows == f_w.nrows, f"{what}, frozen: {r.nrows} rows, the whole push run {f_w.nrows}"
    assert r.rows == f_w.rows, f"{what}, frozen: {_differing(r.rows, f_w.rows)}"
    if has_header:
        assert r.header == f_w.header, f"{what}, frozen: header"
    check_record(r.record, f_w.record, what + ", frozen")
    if not K.measures:
        return
    assert _same_pair(r.rescale, s_w), f"{what}, frozen: get_rescale does not return the scale that was set"
    # (b), (c)
    m = run(None)
    assert m.nrows == W.nrows, f"{what}, measured: {m.nrows} rows, the whole push run {W.nrows}"
    check_scale(m.rescale, s_w, exact, what)
    f_r = ref.frozen(m.rescale)
    assert m.rows == f_r.rows, f"{what}, measured: against the whole push run under the scale this run measured, {_differing(m.rows, f_r.rows)}"
    if has_header:
        assert m.header == W.header, f"{what}, measured: header"
    check_record(m.record, W.record, what + ", measured")


def hold_power(c, d, what):
    """(d)"""
    whole = run_power(c, d, [d.nblocks])
    assert np.frombuffer(whole.rows, np.uint8).size == d.rows * d.ncol * 4
    per = run_power(c, d, [1] * d.nblocks)
    assert per.rows == whole.rows, f"{what}: power tap per block against one call, {_differing(per.rows, whole.rows)}"
    return whole


def hold_scan(refs, chans, ds, cut, what, exact):
    """hold() for every IF of a scan: one frbch_scan_device sequence serves all IFs (frozen once, measured once), every IF reads
    its columns and is held to its own push run"""
    got = {}

    def run(i, frozen):
        key = frozen is None
        if key not in got:
            got[key] = run_scan(chans, ds, cut, None if key else [r.W.rescale for r in refs])
        return got[key][i]
    for i, ref in enumerate(refs):
        hold(ref, lambda frozen, i=i: run(i, frozen), f"{what}, IF {i}", exact, has_header=False)
