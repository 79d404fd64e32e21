"""Patterns of bad frames (flagged invalid, or missing), built from the library's own geometry: shared cases of
tests/test_frame_faults.py (emulator build) and tests/test_gpu_frame_faults.py (device).  A plain module: the geometry of a stream
(Geometry, from the frbch_info of a handle that has seen the stream's first frame), the patterns, the driver that runs a pattern
against the fp64 oracle, and the sharper statements that hold where the input makes them exact.

A pattern is a function of the geometry, so that it means the same thing at every shape: "the frame that holds the first byte of
block 2" and not "frame 16".  It returns a Fault: frames = dict(invalid=[...], drop=[...]) for parity_util.hurt_frames (indices
into the CLEAN stream) and facts = the host-side predicate the tests assert, as a list of (statement, bool) -- computed from the
bad frames alone (Geometry.dirty / Geometry.dead), never from the way the pattern chose them.  A pattern that cannot be built
at a shape (a launch of three blocks cannot read dirty, clean, dirty where a frame is longer than two blocks) returns None;
tests/test_frame_faults.py lists these and holds every pattern to at least one shape there, tests/test_gpu_frame_faults.py
accepts no None for the masked kernels.

Expected values are always oracle.frb_oracle.channelise on the same hurt bytes, compared under parity_util.check_codes as it
stands; the frame counters against the oracle's frame_counters."""
from collections import namedtuple

import numpy as np

from frb_baseband_amd import sigproc, synth, vdif
from oracle import frb_oracle as o
from tests import parity_util as pu
from tests import partition_cases as pc

Fault = namedtuple("Fault", "frames facts frame0")            # frame0: frames into a second the stream starts (None: 0)


def fault(facts, invalid=(), drop=(), frame0=None):
    return Fault(dict(invalid=sorted(int(f) for f in invalid), drop=sorted(int(f) for f in drop)), facts, frame0)


class Geometry:
    """payload bytes of frames and blocks.  Frame f of the clean stream holds payload bytes [f pb, (f + 1) pb); whole block b reads
    [skip + b stride, skip + b stride + block) -- stride < block with overlap-save (coherent)."""

    def __init__(self, info, K, nfr):
        self.pb = K.frame_bytes - K.header_bytes
        self.nfr, self.skip = int(nfr), int(K.skip)
        self.block, self.stride = int(info.block_payload_bytes), int(info.block_stride_bytes)
        self.rpb, self.interval_rows = int(info.rows_per_block), int(info.rescale_interval_rows)
        self.maxb = int(K.kw.get("maxb", 0)) or 256
        spb = 4 // K.bits
        have = self.nfr * self.pb - self.skip
        want = int(round(K.total * 2.0e6 * abs(K.bw))) // spb        # -T, in payload bytes
        n = min(have, want)
        self.nblocks = (n - self.block) // self.stride + 1 if n >= self.block else 0
        self.fps = vdif.frames_per_second(abs(K.bw), self.pb, K.bits)

    def start(self, b):
        return self.skip + b * self.stride

    def end(self, b):
        return self.start(b) + self.block

    def frame_of(self, byte):
        return byte // self.pb

    def frames_of(self, b):
        """the frames block b reads a byte of"""
        return list(range(self.frame_of(self.start(b)), self.frame_of(self.end(b) - 1) + 1))

    def blocks_of(self, f):
        return [b for b in range(self.nblocks) if f in self.frames_of(b)]

    def dirty(self, bad):
        """whole blocks that read a byte of a bad frame"""
        bad = set(bad)
        return [b for b in range(self.nblocks) if bad & set(self.frames_of(b))]

    def dead(self, bad):
        """whole blocks that read bad frames only"""
        bad = set(bad)
        return [b for b in range(self.nblocks) if set(self.frames_of(b)) <= bad]

    @property
    def last_frame(self):
        """the last frame the last whole block reads"""
        return self.frame_of(self.end(self.nblocks - 1) - 1)

    def launches(self):
        """[first block, behind the last block) of the engine calls of one push: the host hands over maxb blocks at a time"""
        return [(b0, min(b0 + self.maxb, self.nblocks)) for b0 in range(0, self.nblocks, self.maxb)]

    def interval_blocks(self):
        """number of blocks that hold a row of the first rescale interval"""
        return -(-self.interval_rows // self.rpb)


def _bad(f):
    return set(f.frames["invalid"]) | set(f.frames["drop"])


# ---- the patterns -------------------------------------------------------------------------------------------------------------
def first(g):
    """the frame that holds the first byte the first block reads: frame 0 without -S"""
    f = g.frame_of(g.start(0))
    return fault([("frame 0 where nothing is skipped", f == 0 or g.skip >= g.pb), ("block 0 reads it", 0 in g.dirty([f])),
                  ("it holds the stream's first byte read", f * g.pb <= g.skip < (f + 1) * g.pb)], invalid=[f])


def last(g):
    f = g.last_frame
    return fault([("the last whole block reads it", g.nblocks - 1 in g.dirty([f])), ("no whole block reads a later frame", g.dirty(range(f + 1, g.nfr)) == []),
                  ("it is a frame of the stream", f < g.nfr)], invalid=[f])


def tail(g):
    """a frame wholly behind the last whole block: the rows are the clean stream's, only the counter moves"""
    f = g.last_frame + 1
    if f >= g.nfr:
        return None
    return fault([("no whole block reads it", g.dirty([f]) == []), ("it starts behind the last whole block", f * g.pb >= g.end(g.nblocks - 1)),
                  ("it is a frame of the stream", f < g.nfr)], invalid=[f])


def _edge(g, k):
    e = g.start(k)
    f = g.frame_of(e)
    return fault([(f"the frame holds the first byte of block {k}", f * g.pb <= e < (f + 1) * g.pb),
                  (f"... and the byte in front of it, which block {k - 1} reads", f * g.pb <= e - 1 and g.start(k - 1) <= e - 1 < g.end(k - 1)),
                  (f"blocks {k - 1} and {k} both read it", {k - 1, k} <= set(g.dirty([f])))], invalid=[f])


def block_edge(g):
    """the frame that straddles the edge of blocks 1 | 2 (edge_name() says whether a launch ends there)"""
    return _edge(g, 2) if g.nblocks > 2 else None


def launch_edge(g):
    """the frame that straddles the first edge between two engine calls, where block_edge does not already"""
    k = g.launches()[0][1]
    if k >= g.nblocks or k == 2:
        return None
    f = _edge(g, k)
    return f._replace(facts=f.facts + [("a launch ends at the edge", any(b1 == k for _b0, b1 in g.launches()))])


def edge_name(g):
    """block_edge is called launch_edge where the edge of blocks 1 | 2 is also an edge between two engine calls"""
    return "launch_edge" if any(b1 == 2 for _b0, b1 in g.launches()) and g.nblocks > 2 else "block_edge"


def word(g):
    """both sides of a word of the frame bitmap: the pairs 31 | 32 and 63 | 64 that the whole blocks reach"""
    pairs = [(a, a + 1) for a in (31, 63) if a + 1 <= g.last_frame and g.frame_of(g.start(0)) <= a]
    if not pairs:
        return None
    bad = [f for p in pairs for f in p]
    return fault([("a pair is reached", len(pairs) >= 1), ("whole blocks read every flagged frame", all(g.dirty([f]) for f in bad)),
                  ("the pairs lie on both sides of a multiple of 32", all(b % 32 == 0 and a == b - 1 for a, b in pairs))], invalid=bad)


def alternate(g):
    """every second frame of block 1"""
    if g.nblocks < 2:
        return None
    fr = g.frames_of(1)
    bad = fr[::2]
    return fault([("block 1 reads every flagged frame", all(f in fr for f in bad) and 1 in g.dirty(bad)),
                  ("no two flagged frames are neighbours", all(b - a == 2 for a, b in zip(bad[:-1], bad[1:]))),
                  ("flagged and clean frames alternate where the block reads three frames or more", len(fr) < 3 or (len(bad) >= 2 and len(fr) - len(bad) >= 1))],
                 invalid=bad)


def dead_block(g):
    """every frame block 1 reads"""
    if g.nblocks < 3:
        return None
    bad = g.frames_of(1)
    dead = g.dead(bad)
    if len(dead) == g.nblocks:
        return None
    return fault([("block 1 reads bad frames only", 1 in dead), ("a block of the stream is not dead", len(dead) < g.nblocks),
                  ("the dead blocks are one run", dead == list(range(dead[0], dead[-1] + 1)))], invalid=bad)


def dirty_clean_dirty(g):
    """blocks 0 and 2 hold one flagged frame each, block 1 none; the three go to the engine in one call"""
    if g.nblocks < 3 or g.launches()[0][1] < 3:
        return None
    bad = [g.frames_of(0)[0], g.frames_of(2)[-1]]
    if 1 in g.dirty(bad):
        return None
    return fault([("blocks 0 and 2 read a flagged frame, block 1 none", [b for b in g.dirty(bad) if b < 3] == [0, 2]),
                  ("one flagged frame each", len(set(bad) & set(g.frames_of(0))) == 1 and len(set(bad) & set(g.frames_of(2))) == 1),
                  ("one engine call holds the three", g.launches()[0][1] >= 3)], invalid=bad)


def _dead_interval(g, extra):
    nb = g.interval_blocks() + extra
    if not g.interval_rows or nb >= g.nblocks:
        return None
    bad = sorted({f for b in range(nb) for f in g.frames_of(b)})
    dead = g.dead(bad)
    if len(dead) == g.nblocks:
        return None
    return fault([("every block of the first interval reads bad frames only", set(range(g.interval_blocks())) <= set(dead)),
                  (f"... and {extra} further block(s)", set(range(nb)) <= set(dead)),
                  ("the dead rows cover the interval", len(dead) * g.rpb >= g.interval_rows), ("live blocks follow", len(dead) < g.nblocks)], invalid=bad)


def dead_interval(g):
    """every frame the blocks of the first rescale interval read"""
    return _dead_interval(g, 0)


def dead_interval_plus(g):
    """... and those of one further block"""
    return _dead_interval(g, 1)


def all_dead(g):
    bad = list(range(g.nfr))
    return fault([("every whole block reads bad frames only", g.dead(bad) == list(range(g.nblocks))), ("there is a whole block", g.nblocks > 0)], invalid=bad)


def long_gap(g):
    """missing frames worth more than one block, from the middle of block 1 on"""
    n = g.block // g.pb + 2
    f0 = max(1, g.frame_of(g.start(1) + g.block // 2))
    bad = list(range(f0, f0 + n))
    if bad[-1] + 1 >= g.nfr:
        return None
    return fault([("the gap is longer than a block", n * g.pb > g.block), ("frames of the stream on both sides", bad[0] >= 1 and bad[-1] + 1 < g.nfr),
                  ("whole blocks read the gap", len(g.dirty(bad)) >= 2), ("the library fills it (at most 16 s)", n <= 16 * g.fps)], drop=bad)


def gap_at_1(g):
    return fault([("frame 0 and a frame behind the gap exist", g.nfr > 2), ("a whole block reads the gap, where nothing is skipped", bool(g.dirty([1])) or g.skip >= g.pb)], drop=[1])


def gap_beside_flags(g):
    """two missing frames with a flagged neighbour on each side, around the middle of block 1"""
    f = max(2, g.frame_of(g.start(1) + g.block // 2))
    if f + 3 >= g.nfr:
        return None
    return fault([("flag, gap, gap, flag are neighbours", True), ("a whole block reads one of them", bool(g.dirty([f - 1, f, f + 1, f + 2]))),
                  ("a frame of the stream follows", f + 3 < g.nfr)], invalid=[f - 1, f + 2], drop=[f, f + 1])


def second_boundary(g):
    """the stream starts fps - k frames into a second: frame k is the first of the next second and starts inside a block behind
    block 0 (block 1 where a block reads three frames or more); the frames on both sides of the rollover are missing, the next one
    is flagged"""
    hit = [(b, f) for b in range(1, g.nblocks) for f in g.frames_of(b) if f >= 2 and g.start(b) < f * g.pb < g.end(b)]
    if not hit:
        return None
    b, k = hit[0]
    if k + 2 >= g.nfr or k >= g.fps:
        return None
    return fault([("the rollover falls inside a block behind block 0", b >= 1 and g.start(b) < k * g.pb < g.end(b)),
                  ("... block 1, where a block reads three frames or more", b == 1 or len(g.frames_of(1)) < 3),
                  ("frames k - 1 (old second) and k (new second) are missing", k - 1 >= 1),
                  ("the stream starts inside a second", 0 < g.fps - k < g.fps), ("a frame follows the flagged one", k + 2 < g.nfr)],
                 invalid=[k + 1], drop=[k - 1, k], frame0=g.fps - k)


PATTERNS = {"first": first, "last": last, "tail": tail, "block_edge": block_edge, "launch_edge": launch_edge, "word": word, "alternate": alternate,
            "dead_block": dead_block, "dirty_clean_dirty": dirty_clean_dirty, "dead_interval": dead_interval, "dead_interval_plus": dead_interval_plus,
            "all_dead": all_dead, "long_gap": long_gap, "gap_at_1": gap_at_1, "gap_beside_flags": gap_beside_flags,
            "second_boundary": second_boundary}
FLAG_ONLY = ("first", "last", "tail", "block_edge", "launch_edge", "word", "alternate", "dead_block", "dirty_clean_dirty", "dead_interval",
             "dead_interval_plus", "all_dead")
DEAD_INTERVAL = ("dead_interval", "dead_interval_plus")


def needs(name, kw):
    """what a pattern needs of the configuration (it overrides the shape's own values).
    dead_block: float rows without a rescale, for check_dead_rows.
    dead_interval under -c with cross products (pol 4, 5): float rows.  The dead interval's pair (offset 0, scale 1) then stays for
    the live rows, which are raw powers of 1e5 .. 1e7: integer codes of a product that is never negative all clip to the largest
    code, in the library as in the oracle, but a cross product near zero does not clip, and one fp32 ulp of a power of 1e6 (0.06)
    is 1.3 codes at 8 bit and 340 at 16 bit.  check_codes' tie model is for values rescaled to unit variance; its float branch
    scales the bound with the pair applied, so the float rows are what can be held here."""
    if name == "dead_block":
        return dict(nbit=-32, interval=0.0)
    if name in DEAD_INTERVAL and kw.get("const", 1) and kw.get("pol", 2) in (4, 5) and kw.get("interval", 10.0) > 0:
        return dict(nbit=-32)
    return {}


def check_facts(name, f):
    for what, ok in f.facts:
        assert ok, f"pattern {name}: {what}"
    assert not set(f.frames["invalid"]) & set(f.frames["drop"]), name


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def probe(lib, K):
    """Geometry of K's stream: the info of a handle that has seen the first frame (the plan follows the stream's bits per sample)"""
    fps = vdif.frames_per_second(abs(K.bw), K.frame_bytes - K.header_bytes, K.bits)
    head = synth.make_vdif(1.5 / fps, bw_mhz=abs(K.bw), nchan=K.nchan, **K.gen)
    with K.open(lib) as c:
        c.push(head[:K.frame_bytes])
        return Geometry(c.get_info(), K, int(round((K.secs + K.kw.get("start", 0.0)) * fps)))     # (synth.make_vdif's frame count)


def clean_stream(K, frame0=None):
    """the stream of K without faults; frame0: its first frame is frame0 frames into a second (the headers rewritten)"""
    raw = synth.make_vdif(K.secs + K.kw.get("start", 0.0), bw_mhz=abs(K.bw), nchan=K.nchan, **K.gen, **({"if_index": K.if_index} if K.if_index else {}))
    if frame0:
        payload = o.strip_frames(raw, K.frame_bytes, K.header_bytes)
        raw = vdif.frame_payload(np.ascontiguousarray(payload), bw_mhz=abs(K.bw), seconds0=1000, frame0=frame0, payload_bytes=K.frame_bytes - K.header_bytes,
                                 legacy=K.gen.get("legacy", 0), bits=K.bits)
    return raw


Run = namedtuple("Run", "got ref ocfg info rescale record nbad")


def run(lib, K, f, record=False):
    """K's stream with the fault f through push / flush / pull against the oracle on the same bytes (parity_util.run_streaming_case:
    check_codes and the rescale check), and the frame counters against the oracle's"""
    out, rec = {}, ({} if record else None)
    frame0 = f.frame0 if f is not None else None
    kw = dict(K.kw, **K.gen)
    kw.update(raw=clean_stream(K, frame0), raw_key=("stream of", K.secs, "s, frame0", frame0))      # (K.total = -T may be less than the stream)
    nbad = pu.run_streaming_case(lib, K.bw, K.nchan, K.total, frames=f.frames if f is not None else None, record=rec, out=out, **kw)
    r = Run(out["got"], out["ref"], out["ocfg"], out["info"], out["rescale"], rec, nbad)
    check_counters(r.info, r.ocfg)
    return r


def check_counters(info, ocfg):
    want = ocfg.result["frame_counters"]
    got = dict(gaps=int(info.frame_gaps), filled=int(info.frames_filled), invalid=int(info.frames_invalid))
    assert got == want, f"frame counters {got}, the oracle's {want}"


def rows_of(fil_bytes):
    return sigproc.read_fil(fil_bytes).data


def check_dead_rows(g, f, r):
    """float rows under -I0: the rows of a block that reads bad frames only are == 0.0, those of every other block are not"""
    assert r.ocfg.nbit == -32 and r.ocfg.rescale_interval_s == 0.0
    data = rows_of(r.got)
    assert data.shape[0] == g.nblocks * g.rpb
    dead = set(g.dead(_bad(f)))
    for b in range(g.nblocks):
        rows = data[b * g.rpb:(b + 1) * g.rpb]
        if b in dead:
            assert np.all(rows == 0.0), f"block {b} reads bad frames only: {np.count_nonzero(rows)} of its values are not 0"
        else:
            assert np.any(rows != 0.0, axis=(1, 2)).all(), f"block {b} reads live frames and has a row of zeros"


def check_dead_scale(r):
    """the pair of an interval without a live sample: offset +-0 and scale exactly 1.0 for every (product, channel)"""
    off, sc = r.rescale
    assert np.all(off == 0.0) and np.all(sc == 1.0), (np.abs(off).max(), sc.min(), sc.max())


def check_single_code(r, nrows):
    """the first nrows rows hold one code: the one the oracle gives"""
    got, want = rows_of(r.got)[:nrows], rows_of(r.ref)[:nrows]
    assert nrows > 0 and np.unique(want).size == 1 and np.array_equal(got, want), (np.unique(want), np.unique(got))


def check_sharper(g, name, f, r, K):
    """the three statements that are exact where the input makes them so (the module's docstring; tail: check_tail)"""
    if name == "dead_block":
        check_dead_rows(g, f, r)
    measured = K.measures and K.kw.get("nbit", 8) != -32
    if name == "all_dead" and K.measures:
        check_dead_scale(r)
        if measured:
            check_single_code(r, g.nblocks * g.rpb)
    if name in DEAD_INTERVAL and K.measures:
        if K.kw.get("const", 1):
            check_dead_scale(r)               # (-c: the pair of the first interval is the one get_rescale returns)
        if measured:
            check_single_code(r, g.interval_rows)   # (a rescale per interval: get_rescale returns the last pair, the codes speak for the first)


def check_tail(lib, K, r):
    """tail: the clean stream's .fil byte for byte"""
    with K.open(lib) as c:
        clean = c.channelise_bytes(clean_stream(K))
    assert r.got == clean, "a flagged frame behind the last whole block changes the rows"


def hold_pattern(lib, K, g, name, record=False):
    """everything the module asks of one pattern at one configuration -> (Fault, Run), or None where the pattern cannot be built"""
    f = PATTERNS[name](g)
    if f is None:
        return None
    check_facts(name, f)
    r = run(lib, K, f, record=record)
    assert rows_of(r.got).shape[0] == g.nblocks * g.rpb > 0
    check_sharper(g, name, f, r, K)
    if name == "tail":
        check_tail(lib, K, r)
    return f, r


def config(bw, nchan, secs, kw, name, total=None):
    """the configuration of a shape for a pattern: what the pattern needs overrides the shape's own values"""
    return pc.Config(bw, nchan, secs, dict(kw, **needs(name, kw)), total=total)
