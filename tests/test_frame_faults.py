"""Patterns of bad frames (tests/frame_fault_cases.py) on the emulator build: every pattern at the smallest shapes, against the
fp64 oracle on the same hurt bytes under parity_util.check_codes, with the frame counters and the sharper statements.  This
module proves the pattern builders, their predicates and the oracle's agreement with the generic kernels and the host logic
(check_headers, process_carry, engine_feed's runs of dirty and clean blocks); it is also where "the reference stays inside
check_codes' caps on these inputs" is kept true.  tests/test_gpu_frame_faults.py holds the register kernels to the same.

Three blocks per engine call everywhere; a shape is bw, nchan, seconds of stream, configuration, -T (less than the stream holds:
a frame lies wholly behind the last whole block).  Where a frame is longer than a block (8000-byte frames in front of 2 KiB blocks) some
patterns cannot be built: NOT_BUILT lists them, and every pattern is built at one shape at least."""
import pytest

from tests import frame_fault_cases as fc
from tests import kernel_table as kt
from tests import partition_cases as pc

SHAPES = {
    # 32 channels, R = 64: blocks of 2 KiB, a frame holds 3.9 of them
    "32ch": (16.0, 32, 0.0305, dict(freq_res=64, maxb=3, interval=0.004), 0.03),
    # the coherent 64-channel shape of tests/test_engine_emulated.py: blocks of 8 KiB that overlap
    "coherent64": (16.0, 64, 0.0205, dict(dm=56.7, coherent=1, freq=1400.0, nbit=16, freq_res=128, maxb=3, interval=0.004), 0.02),
    "pol4_16bit": (-16.0, 32, 0.0305, dict(pol=4, nbit=16, freq_res=64, maxb=3, interval=0.004), 0.03),
    # 1000-byte legacy frames: a block reads two or three frames
    "legacy1000": (16.0, 32, 0.0121, dict(freq_res=64, payload_bytes=1000, legacy=1, maxb=3, interval=0.002), 0.012),
    # -S 20 frames and 4800 bytes into the stream
    "start": (16.0, 32, 0.0305, dict(freq_res=64, start=0.0103, maxb=3, interval=0.004), 0.03),
}
# patterns that cannot be built at a shape (frame_fault_cases: the pattern returns None), and why
_LONG_FRAMES = "a frame is longer than two blocks: no engine call of three blocks reads dirty, clean, dirty"
NOT_BUILT = {
    ("32ch", "dirty_clean_dirty"): _LONG_FRAMES, ("pol4_16bit", "dirty_clean_dirty"): _LONG_FRAMES, ("start", "dirty_clean_dirty"): _LONG_FRAMES,
    ("coherent64", "dirty_clean_dirty"): "a frame is as long as two blocks and blocks overlap: block 1 reads the frames of blocks 0 and 2",
}
_CONST = {"dead_interval": (0, 1), "dead_interval_plus": (0, 1), "all_dead": (0, 1)}       # without -c and with it
_CASES = [(s, p, const) for s in SHAPES for p in fc.PATTERNS for const in _CONST.get(p, (None,))]

_GEO: dict = {}


def _geometry(lib, shape):
    if shape not in _GEO:
        bw, nchan, secs, kw, total = SHAPES[shape]
        _GEO[shape] = fc.probe(lib, pc.Config(bw, nchan, secs, kw, total=total))
    return _GEO[shape]


@pytest.mark.parametrize("shape,name,const", _CASES, ids=[f"{s}-{p}" + ("" if c is None else f"-const{c}") for s, p, c in _CASES])
def test_pattern_matches_the_oracle(emu_lib, shape, name, const):
    bw, nchan, secs, kw, total = SHAPES[shape]
    K = fc.config(bw, nchan, secs, dict(kw, **({} if const is None else {"const": const})), name, total=total)
    g = _geometry(emu_lib, shape)
    done = fc.hold_pattern(emu_lib, K, g, name)
    assert (done is None) == ((shape, name) in NOT_BUILT), f"{name} at {shape}: built or not against NOT_BUILT"


def test_every_pattern_is_built_somewhere_and_flags_what_it_says():
    assert set(fc.FLAG_ONLY) <= set(fc.PATTERNS)
    for name in fc.PATTERNS:
        assert any((s, name) not in NOT_BUILT for s in SHAPES), name
    assert {p for _s, p in NOT_BUILT} <= set(fc.PATTERNS) and {s for s, _p in NOT_BUILT} <= set(SHAPES)


def test_edge_of_blocks_1_and_2_is_named_after_what_ends_there(emu_lib):
    """block_edge is launch_edge where an engine call ends at the edge: two blocks per call, not three"""
    bw, nchan, secs, kw, total = SHAPES["legacy1000"]
    assert fc.edge_name(_geometry(emu_lib, "legacy1000")) == "block_edge"
    g2 = fc.probe(emu_lib, pc.Config(bw, nchan, secs, dict(kw, maxb=2), total=total))
    assert fc.edge_name(g2) == "launch_edge" and fc.launch_edge(g2) is None


def test_geometry_is_the_oracles(emu_lib):
    """the number of whole blocks Geometry works with is the number the library delivers and the oracle computes"""
    for shape, (bw, nchan, secs, kw, total) in SHAPES.items():
        g = _geometry(emu_lib, shape)
        r = fc.run(emu_lib, pc.Config(bw, nchan, secs, kw, total=total), None)
        assert fc.rows_of(r.got).shape[0] == g.nblocks * g.rpb, shape
        assert (r.info.frames_invalid, r.info.frame_gaps, r.info.frames_filled) == (0, 0, 0)


# ---- the device module's case list against the masked instantiations ----------------------------------------------------------
def test_every_masked_instantiation_runs_every_pattern(hip_lib, emu_lib):
    """every frbch_k1_wave<..., MSK = true> the built library lists has a row in tests/kernel_table.py, and
    tests/test_gpu_frame_faults.py runs every pattern at that row's shape: a new masked instantiation without cases fails here.
    The patterns are built (and their predicates asserted) at those shapes on the emulator's geometry, which is the library's"""
    from tests import test_gpu_frame_faults as tg
    from tests.test_kernel_table import library_kernels
    masked = {n for n in library_kernels() if kt.family(n) == "frbch_k1_wave" and n.endswith(", true>")}
    assert masked and masked == {r.name for r in tg.MSK_ROWS}, sorted(masked ^ {r.name for r in tg.MSK_ROWS})
    for r in tg.MSK_ROWS:
        assert {p for n, p in tg.A_CASES if n == r.name} == set(fc.PATTERNS), r.name
        g = fc.probe(emu_lib, tg.msk_config(r, "first"))
        assert g.nblocks == 5 and g.launches() == [(0, 3), (3, 5)], (r.name, g.nblocks)
        for name in fc.PATTERNS:
            f = fc.PATTERNS[name](g)
            assert f is not None, f"{name} cannot be built at the shape of {r.name}"
            fc.check_facts(name, f)
