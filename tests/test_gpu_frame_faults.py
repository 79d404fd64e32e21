"""Patterns of bad frames (tests/frame_fault_cases.py) through the kernels that run in production: the masked form of the staged
wave K1 (frbch_k1_wave<L, 8, WPS, true, COH, true>: a flag per row beside the stage, a flag BIT per row at R = 8192), the
fallbacks of a dirty run to the generic K1 where that kernel cannot run, the whole-file paths and the scan.  Expected values are
the fp64 oracle's on the same hurt bytes under parity_util.check_codes as it stands; the frame counters are the oracle's; the
launch record says which kernels ran.  tests/test_frame_faults.py holds the emulator build to the same patterns and this
module's case list to the masked instantiations of the built library.

 (a) every masked instantiation (the MSK rows of tests/kernel_table.py, lengthened to five blocks, three blocks per engine call)
     x every pattern; output width, products and band sense rotate over the patterns; one launch of 20 dirty blocks, in which
     workgroups of the persistent loop take a second block;
 (b) 1024 channels / R = 2048 with pol = 5 (the two-pass rescale: frbch_k2_priv reads the masked K1's paired spill), buffered
     (1 << 27) and not, four blocks per call; one 4096-channel case (2^26-sample blocks);
 (c) the fallbacks: the coherent chain in front of the barrier K1, an unaligned -S, 1-bit input, 1000-byte payloads, dynamic levels;
 (d) frbch_run_file, frbch_run_scan over two IFs, and the cuts of tests/partition_cases.py."""
import numpy as np
import pytest

from frb_baseband_amd import multi_if, sigproc
from oracle import frb_oracle as o
from tests import frame_fault_cases as fc
from tests import kernel_table as kt
from tests import parity_util as pu
from tests import partition_cases as pc

pytestmark = pytest.mark.gpu

NBLOCKS = 5
MSK_ROWS = [r for r in kt.ROWS if kt.family(r.name) == "frbch_k1_wave" and r.name.endswith(", true>")]
A_CASES = [(r.name, p) for r in MSK_ROWS for p in fc.PATTERNS]
_NBIT, _POL = (2, 8, 16, -32), (2, 4, 1, 5, 3, 0)
_CONST = {"dead_interval": 0, "dead_interval_plus": 1}      # without -c and with it (tests/test_frame_faults.py: both for both)
_MOSTLY_DEAD = fc.DEAD_INTERVAL + ("all_dead",)
BRANCH, DEDISP = "frbch_k1_branch", "frbch_k3_dedisp"


def _five_blocks(r, blocks_now):
    """the row's stream lengthened to five blocks and 0.3 of a block (at least two frames behind the last whole block)"""
    return round(r.secs / blocks_now * (NBLOCKS + 0.3), 6)


def msk_config(r, name):
    """the shape of a masked row for a pattern: five blocks, three per engine call, an interval of 0.45 of the stream (it ends
    inside the first call); nbit, products and band sense by the pattern's place in the list.
    Two combinations the rotation leaves out, because check_codes' FLOAT bound is relative to the mean power of a channel's whole
    series and so does not describe them (measured on the MI355X on the clean stream and the hurt one):
    float rows of a stream whose blocks are mostly dead (the dead rows pull the mean, and with it the bound, down to a fifth; the
    live rows err exactly as the clean stream's do) -- the patterns of _MOSTLY_DEAD take integer codes of one product, which are
    exact under the tie model; and float rows of pol 3 without a rescale ((PP + QQ)^2: samples of 30 x the mean, whose own fp32
    rounding exceeds a mean-relative bound on the clean stream already) -- pol 2 instead."""
    i = list(fc.PATTERNS).index(name) + MSK_ROWS.index(r)
    secs = _five_blocks(r, 4.3)
    kw = dict(r.kw, maxb=3, interval=round(0.45 * secs, 6), nbit=_NBIT[i % 4], pol=_POL[i % 6])
    if name in _MOSTLY_DEAD:
        kw.update(nbit=(2, 8, 16)[i % 3], pol=(2, 1, 0)[i % 3])
    if name in _CONST:
        kw["const"] = _CONST[name]
    kw.update(fc.needs(name, kw))
    if kw["nbit"] == -32 and kw["pol"] == 3:
        kw["pol"] = 2
    return fc.config(r.bw if i % 2 else -r.bw, r.nchan, secs, kw, name)


_GEO: dict = {}


def _geometry(lib, key, K):
    if key not in _GEO:
        _GEO[key] = fc.probe(lib, K)
    return _GEO[key]


def _ran(rec, *names):
    for n in names:
        assert n in rec and rec[n]["launches"] >= 1, f"{n} did not run: {sorted(rec)}"


def _k0_ran(rec):
    assert any(n.startswith("frbch_k0_stage<") for n in rec), f"no frbch_k0_stage ran: {sorted(rec)}"


def _unmasked(name):
    return name[:-len("true>")] + "false>"


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,name", A_CASES, ids=[f"{n}|{p}" for n, p in A_CASES])
def test_masked_k1_matches_the_oracle(hip_lib, row, name):
    r = next(x for x in MSK_ROWS if x.name == row)
    K = msk_config(r, name)
    g = _geometry(hip_lib, (row, K.kw["interval"]), K)
    assert g.nblocks == NBLOCKS and g.launches() == [(0, 3), (3, 5)]
    done = fc.hold_pattern(hip_lib, K, g, name, record=True)
    assert done is not None, f"{name} cannot be built at the shape of {row}"
    f, run = done
    rec, dirty = run.record, g.dirty(fc._bad(f))
    _k0_ran(rec)
    assert BRANCH not in rec, f"{BRANCH} ran beside {row}: {sorted(rec)}"
    if dirty:
        _ran(rec, row)
    if len(dirty) < g.nblocks:
        _ran(rec, _unmasked(row))
    assert (row in rec) == bool(dirty), f"{name}: dirty blocks {dirty}, record {sorted(rec)}"


def one_per_block(g):
    """one flagged frame in every block, the k-th frame of block b with k moving along with b (and once more every eight blocks: k
    does not come round again after 15 or 16 blocks, the frames a block reads less two)"""
    bad = sorted({g.frames_of(b)[1 + (b + b // 8) % (len(g.frames_of(b)) - 2)] for b in range(g.nblocks)})
    return fc.fault([("every block reads a flagged frame", g.dirty(bad) == list(range(g.nblocks))),
                     ("one each", all(len(set(bad) & set(g.frames_of(b))) == 1 for b in range(g.nblocks)))], invalid=bad)


def test_masked_k1_second_trip_of_the_persistent_loop(hip_lib):
    """20 dirty blocks in one launch at 256 channels, R = 512: 32 branch groups x min(20, resident workgroups / 32) block slots
    (16 on the 256 CUs of an MI355X), so the first slots take a second block whose flags lie elsewhere than their first block's:
    flags left over from the trip before would show.  (The five-block cases above are one trip for every workgroup.)"""
    r = MSK_ROWS[0]
    secs = round(r.secs / 4.3 * 20.3, 6)
    K = pc.Config(-r.bw, r.nchan, secs, dict(r.kw, maxb=20, interval=round(0.45 * secs, 6), nbit=16))
    g = _geometry(hip_lib, "second_trip", K)
    assert g.nblocks == 20 and g.launches() == [(0, 20)]
    f = one_per_block(g)
    fc.check_facts("one_per_block", f)
    run = fc.run(hip_lib, K, f, record=True)
    _ran(run.record, r.name)
    slots = run.record[r.name]["grid_y"]
    assert slots < g.nblocks, f"every workgroup makes one trip: {run.record[r.name]}"
    where = [[(x - g.frames_of(b)[0]) for x in f.frames["invalid"] if x in g.frames_of(b)] for b in range(g.nblocks)]
    assert all(where[b] != where[b + slots] for b in range(g.nblocks - slots)), "a slot's second block carries its first block's flags"
    assert BRANCH not in run.record and _unmasked(r.name) not in run.record, sorted(run.record)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
_PROD = (-32.0, 1024, 0.347341, dict(pol=5, maxb=4, interval=0.1563))       # 5.3 blocks of 2^22 samples; the interval: 2.4 blocks
_B_CASES = [(p, flags) for p in ("dirty_clean_dirty", "block_edge", "dead_interval") for flags in (1 << 27, 0)]


@pytest.mark.parametrize("name,flags", _B_CASES, ids=[f"{p}|flags={f}" for p, f in _B_CASES])
def test_production_shape_two_pass_rescale(hip_lib, name, flags):
    """the runs engine_feed cuts end inside a call of four blocks: the conditions of the two-pass rescale are evaluated per run"""
    bw, nchan, secs, kw = _PROD
    K = fc.config(bw, nchan, secs, dict(kw, flags=flags), name)     # (dead_interval: float rows, frame_fault_cases.needs; a rescale per interval would take frbch_k2_priv out of the plan)
    g = _geometry(hip_lib, "prod", K)
    assert g.nblocks == NBLOCKS and g.launches()[0] == (0, 4)
    done = fc.hold_pattern(hip_lib, K, g, name, record=True)
    assert done is not None
    rec = done[1].record
    _ran(rec, "frbch_k1_wave<3, 8, 1, true, false, true>", "frbch_k1_wave<3, 8, 1, true, false, false>")
    _k0_ran(rec)
    assert any(n.startswith("frbch_k2_priv<5, ") for n in rec), sorted(rec)
    assert BRANCH not in rec and "frbch_k2_chan" not in rec, sorted(rec)


def test_alternate_frames_at_4096_channels(hip_lib):
    """2^26-sample blocks (the stream of tests/test_gpu_pins.py::test_invalid_frame_at_4096_channels): every second frame of
    block 1 -- a frame covers fewer rows than a thread holds, the bits alternate inside a thread's flag word.  11 s on an MI355X,
    nearly all of it the oracle over two blocks of this size: the one case of the module above 5 s (the others: 2.9 s at most)"""
    K = fc.config(64.0, 4096, 1.1, {}, "alternate")
    g = _geometry(hip_lib, "4096", K)
    assert g.nblocks == 2
    f, run = fc.hold_pattern(hip_lib, K, g, "alternate", record=True)
    assert len(f.frames["invalid"]) > 2000 and g.dirty(f.frames["invalid"]) == [0, 1]       # (the first frame of block 1 holds the end of block 0)
    _ran(run.record, "frbch_k1_wave<5, 8, 4, true, false, true>")
    assert BRANCH not in run.record, sorted(run.record)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
def in_block_2(g):
    """one flagged frame that block 2 alone reads"""
    f = g.frame_of(g.start(2) + g.block // 2)
    return fc.fault([("block 2 alone reads it", g.dirty([f]) == [2])], invalid=[f])


def in_the_overlap(g):
    """the frame that holds the first byte blocks 2 and 3 of an overlap-save stream share"""
    f = g.frame_of(g.start(3))
    return fc.fault([("blocks overlap", g.stride < g.block), ("the frame holds a byte both blocks read", f * g.pb <= g.start(3) < min((f + 1) * g.pb, g.end(2))),
                     ("blocks 2 and 3 read it, blocks 0 and 1 do not", g.dirty([f])[:2] == [2, 3])], invalid=[f])


_COHERENT = [(r, fn) for r in kt.ROWS if kt.family(r.name) == "frbch_k1_fast" for fn in (in_block_2, in_the_overlap)]


@pytest.mark.parametrize("r,build", _COHERENT, ids=[f"{r.name}|{fn.__name__}" for r, fn in _COHERENT])
def test_coherent_chain_falls_back_mid_stream(hip_lib, r, build):
    """the barrier K1 of the coherent chain has no masked form: the clean head runs the register chain, from the dirty block on the
    handle runs the generic K1 / K3 in their bin order (launch_front: build_chirp(h, 0))"""
    K = pc.Config(r.bw, r.nchan, _five_blocks(r, 3.3), dict(r.kw, maxb=3, interval=round(0.45 * _five_blocks(r, 3.3), 6)))
    g = _geometry(hip_lib, r.name, K)
    assert g.nblocks == NBLOCKS
    f = build(g)
    fc.check_facts(build.__name__, f)
    run = fc.run(hip_lib, K, f, record=True)
    _ran(run.record, r.name, *r.also, BRANCH, DEDISP)


_MASKED_512 = "frbch_k1_wave<1, 8, 1, true, false, true>"
_FALLBACKS = {
    # name: (bw, nchan, secs, kw, pattern, the K1 that runs the dirty blocks); five blocks and 0.3 of a block each
    "unaligned_start": (32.0, 1024, 0.086837, dict(freq_res=512, start=10 / 64e6, maxb=3, interval=0.039), "dirty_clean_dirty", BRANCH),
    "one_bit": (32.0, 256, 0.021709, dict(bits=1, maxb=3, interval=0.00977), "block_edge", BRANCH),
    "payload_1000": (-32.0, 256, 0.021709, dict(payload_bytes=1000, maxb=3, interval=0.00977), "long_gap", _MASKED_512),
    "payload_1000_legacy": (32.0, 256, 0.021709, dict(payload_bytes=1000, legacy=1, nbit=2, maxb=3, interval=0.00977), "word", _MASKED_512),
    "dynamic_levels": (32.0, 256, 0.021709, dict(dynamic={}, maxb=3, interval=0.00977), "gap_beside_flags", BRANCH),
}
@pytest.mark.parametrize("case", list(_FALLBACKS))
def test_fallbacks_match_the_oracle(hip_lib, case):
    """where the masked wave K1 cannot run a dirty run goes to the generic K1 (no staged input, an unaligned -S); 1000-byte payloads
    are aligned to every row piece: the masked wave K1 takes them"""
    bw, nchan, secs, kw, name, k1 = _FALLBACKS[case]
    K = fc.config(bw, nchan, secs, kw, name)
    g = _geometry(hip_lib, case, K)
    assert g.nblocks == NBLOCKS, g.nblocks
    done = fc.hold_pattern(hip_lib, K, g, name, record=True)
    assert done is not None
    rec = done[1].record
    print(case, sorted(rec))
    _ran(rec, k1)
    if k1 == BRANCH:
        assert not any(n.endswith(", true>") and kt.family(n) == "frbch_k1_wave" for n in rec), sorted(rec)
    else:
        assert BRANCH not in rec, sorted(rec)


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
def _small():
    """the R = 512 masked row, five blocks, three per call"""
    r = MSK_ROWS[0]
    secs = _five_blocks(r, 4.3)
    return r.bw, r.nchan, secs, dict(r.kw, maxb=3, interval=round(0.45 * secs, 6))


def _hurt(K, f):
    return np.ascontiguousarray(pu.hurt_frames(fc.clean_stream(K, f.frame0), f.frames, K.frame_bytes))


@pytest.mark.parametrize("name", ("alternate", "word", "long_gap", "second_boundary"))
def test_run_file_matches_the_oracle(hip_lib, tmp_path, name):
    """frbch_run_file: flags alone stay on the overlapped whole-file path (its own header checks), missing frames take the stream
    path (gap filling)"""
    bw, nchan, secs, kw = _small()
    K = fc.config(bw, nchan, secs, kw, name)
    g = _geometry(hip_lib, "small", K)
    f = fc.PATTERNS[name](g)
    fc.check_facts(name, f)
    raw = _hurt(K, f)
    ocfg = pu.oracle_cfg(K.bw, K.nchan, K.total, **{k: v for k, v in K.kw.items() if k not in ("maxb", "flags")})
    ref = o.channelise(raw, ocfg)
    path, out = str(tmp_path / "in.vdif"), str(tmp_path / "out.fil")
    raw.tofile(path)
    with K.open(hip_lib) as c:
        c.set_profiling(True)
        c.run_file(path, out)
        info, rec = c.get_info(), c.get_launch_record()
    pu.check_codes(ref, open(out, "rb").read(), ocfg)
    fc.check_counters(info, ocfg)
    assert (name in fc.FLAG_ONLY) == (info.frames_filled == 0)
    _ran(rec, "frbch_k1_wave<1, 8, 1, true, false, true>")
    assert BRANCH not in rec, sorted(rec)


@pytest.mark.parametrize("names", (("dirty_clean_dirty", None), ("alternate", "block_edge")), ids=("one_hurt_if", "two_hurt_ifs"))
def test_run_scan_of_two_ifs_matches_the_oracle(hip_lib, tmp_path, names):
    """frbch_run_scan keeps its own flags per IF (bad_all, frbch_file.cpp): every IF's columns against its own oracle run, the
    counters per IF"""
    bw, nchan, secs, kw = _small()
    Ks = [pc.Config(bw, nchan, secs, kw, if_index=i + 1) for i in range(2)]
    g = _geometry(hip_lib, "small", Ks[0])
    chans, want, paths = [], [], []
    try:
        for i, (K, name) in enumerate(zip(Ks, names)):
            raw = fc.clean_stream(K)
            if name is not None:
                f = fc.PATTERNS[name](g)
                fc.check_facts(name, f)
                raw = pu.hurt_frames(raw, f.frames, K.frame_bytes)
            ocfg = pu.oracle_cfg(bw, nchan, secs, **{k: v for k, v in kw.items() if k not in ("maxb", "flags")})
            want.append((sigproc.read_fil(o.channelise(raw, ocfg)).data, ocfg))
            paths.append(str(tmp_path / f"if{i}.vdif"))
            np.ascontiguousarray(raw).tofile(paths[-1])
            chans.append(K.open(hip_lib))
        out = str(tmp_path / "ifall.fil")
        multi_if.run_scan(chans, paths, out)
        infos = [c.get_info() for c in chans]
    finally:
        for c in chans:
            c.close()
    got = sigproc.read_fil(open(out, "rb").read()).data
    assert got.shape == (g.nblocks * g.rpb, 1, 2 * nchan)
    for i, (data, ocfg) in enumerate(want):
        pu.check_code_arrays(data, got[:, :, i * nchan:(i + 1) * nchan], ocfg)
        assert int(infos[i].frames_invalid) == ocfg.result["frame_counters"]["invalid"] == (0 if names[i] is None else len(fc.PATTERNS[names[i]](g).frames["invalid"]))
        assert (int(infos[i].frame_gaps), int(infos[i].frames_filled)) == (0, 0)


_CUT_SHAPES = {"block_edge": 0, "dirty_clean_dirty": 1, "long_gap": 2}      # pattern -> the masked row whose shape it is cut at


@pytest.mark.parametrize("name", list(_CUT_SHAPES))
def test_cuts_of_a_hurt_stream_give_the_rows_of_one_push(hip_lib, name):
    """one frame per push, and cuts one byte in front of, at and behind every block edge: the bytes of the whole push
    (tests/partition_cases.py: (a), (b), (c), (f))"""
    r = MSK_ROWS[_CUT_SHAPES[name]]
    K0 = msk_config(r, name)
    g = _geometry(hip_lib, (r.name, K0.kw["interval"]), K0)
    f = fc.PATTERNS[name](g)
    fc.check_facts(name, f)
    K = pc.Config(K0.bw, K0.nchan, K0.secs, dict(K0.kw, **K0.gen), frames=f.frames)
    with K.open(hip_lib) as c:
        ref = pc.Reference(c, K)
        _ran(ref.W.record, r.name)
        geo = dict(total=K.raw.size, **K.geometry(c.get_info()))
        for cut in ("per_frame", "block_edges"):
            pieces = pc.PUSH_CUTS[cut](**geo)
            pc.hold(ref, lambda frozen: pc.run_push(c, K.raw, pieces, frozen), f"{name}, cut {cut}", exact=False)
