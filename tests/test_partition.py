"""The channeliser gives the same rows however its stream is cut (tests/partition_cases.py), on the emulator build: the frame
carry, gap filling and bad-frame bitmap of frbch_file.cpp, the rescale-interval state machine of frbch_stream.cpp and its batch
planner, under every cut of frbch_push and of the device entry points.  The emulator has one statistics path (sums over the
buffered rows, chunked by the interval's row count alone): everything here is held to identity, offset / scale included."""
import numpy as np
import pytest

from tests import kernel_table as kt
from tests import partition_cases as pc
from tests.test_engine_emulated import CASES

ROUTES = ("push", "device", "file")


@pytest.fixture(scope="module")
def shared():
    """the configuration the module's cases are at: its handle, its reference runs and its frames for the device routes, shared by
    the cases of one configuration (which run one behind the other) and released when the next one starts or the module ends"""
    state = {}
    yield state
    _release(state)


def _release(state):
    if state.get("d") is not None:
        state["d"].free()
    if state.get("c") is not None:
        state["c"].close()
    state.clear()


def _at(state, lib, key, make):
    if state.get("key") != key:
        _release(state)
        K = make()
        state.update(key=key, K=K, c=K.open(lib), d=None)
        state["ref"] = pc.Reference(state["c"], K)
    return state["K"], state["c"], state["ref"]


def _device(state, lib):
    if state["d"] is None:
        info = state["c"].get_info()
        state["d"] = pc.DeviceRun(lib, state["K"], info, int(state["ref"].W.nrows // info.rows_per_block))
    return state["d"]


def _push_cuts(K, c):
    geo = dict(total=K.raw.size, **K.geometry(c.get_info()))
    cuts = {name: fn(**geo) for name, fn in pc.PUSH_CUTS.items() if name != "whole"}
    cuts["ragged_b"] = pc.cut_ragged(seed=pc.RAGGED_SEEDS[1], **geo)
    return cuts


def _hold_route(state, lib, route, tmp_path, extra_cuts=None):
    K, c, ref = state["K"], state["c"], state["ref"]
    if route == "push":
        cuts = _push_cuts(K, c)
        cuts.update(extra_cuts or {})
        for name, cut in cuts.items():
            pc.hold(ref, lambda frozen: pc.run_push(c, K.raw, cut, frozen), f"push, cut {name}", exact=True)
        return
    assert not K.push_only
    if route == "file":
        path, out = str(tmp_path / "in.vdif"), str(tmp_path / "out.fil")
        K.raw.tofile(path)
        pc.hold(ref, lambda frozen: pc.run_file(c, path, out, frozen), "run_file", exact=True)
        return
    d = _device(state, lib)
    for name, cut in pc.device_cuts(d.nblocks).items():
        pc.hold(ref, lambda frozen: pc.run_device(c, d, cut, frozen), f"process_device, cut {name}", exact=True, has_header=False)
    tap = pc.hold_power(c, d, "power_device")
    assert np.isfinite(np.frombuffer(tap.rows, np.float32)).all()


_CASE_ROUTES = [(i, route) for i, (bw, nchan, secs, kw) in enumerate(CASES) for route in ROUTES
                if route == "push" or not pc.Config(bw, nchan, secs, kw).push_only]       # (1-bit streams: the push route only)
# per-interval entries of CASES whose stream is too short for what (e) asks of it (they run all the same)
_SHORT_PER_INTERVAL = {17: "two intervals of 500 rows in its six blocks of 218"}


@pytest.mark.parametrize("i,route", _CASE_ROUTES, ids=[f"case{i}-{route}" for i, route in _CASE_ROUTES])
def test_every_cut_gives_the_rows_of_one_push(emu_lib, shared, tmp_path, i, route):
    bw, nchan, secs, kw = CASES[i]
    K, c, ref = _at(shared, emu_lib, ("case", i), lambda: pc.Config(bw, nchan, secs, kw))
    if K.per_interval and i not in _SHORT_PER_INTERVAL:
        info = c.get_info()
        nblocks = int(ref.W.nrows // info.rows_per_block)
        assert kw.get("maxb", 0) == 0 and nblocks <= 256       # (automatic: at least 256 blocks a launch, one launch per push)
        pc.check_interval_ends(info, nblocks, nblocks)
    _hold_route(shared, emu_lib, route, tmp_path)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kw", (dict(pol=1, freq_res=64), dict(pol=4, nbit=2, tscr=2, freq_res=64)), ids=("pol1", "pol4_t2_2bit"))
def test_a_rescale_per_interval_in_every_cut(emu_lib, shared, tmp_path, kw, route):
    """(e) at two blocks per launch: an interval is a block and a half, the stream five frames = 19 blocks of 1 KiB samples -- every
    second interval ends inside a launch of one push and between two calls of one block"""
    K, c, ref = _at(shared, emu_lib, ("per_interval", kw["pol"]), lambda: pc.per_interval_config(16.0, 32, kw, 0, blocks=21.3))
    info = c.get_info()
    pc.check_interval_ends(info, int(ref.W.nrows // info.rows_per_block), 2)
    _hold_route(shared, emu_lib, route, tmp_path)


def test_hurt_stream_with_the_gap_at_inside_and_behind_a_push_boundary(emu_lib, shared, tmp_path, monkeypatch):
    """the stream of test_frame_header_checks (frame 3 invalid, frames 7 and 8 missing): the gap on a push boundary, a push that
    ends 5 bytes into the header behind the gap, and one that ends inside the frame in front of it; the counters of every run.
    Three blocks of 1 KiB per launch: the engine calls of one push start behind frames the calls before them consumed, so the
    bad-frame flags of a call are found at an offset into the carry's flags (process_carry)"""
    K, c, ref = _at(shared, emu_lib, "hurt", lambda: pc.Config(16.0, 32, 0.012, dict(freq_res=64, maxb=3), frames=dict(invalid=[3], drop=[7, 8])))
    fb, n = K.frame_bytes, K.raw.size
    extra = {"gap_on_the_boundary": [7 * fb, n - 7 * fb], "into_the_header_behind": [7 * fb + 5, n - 7 * fb - 5],
             "inside_the_frame_in_front": [7 * fb - 3000, n - 7 * fb + 3000],
             "all_three": [7 * fb - 3000, 3000, 5, n - 7 * fb - 5]}
    counted = []

    def counting(run):
        def go(*a, **k):
            r = run(*a, **k)
            info = c.get_info()
            counted.append((info.frames_seen, info.frames_invalid, info.frame_gaps, info.frames_filled))
            return r
        return go
    monkeypatch.setattr(pc, "run_push", counting(pc.run_push))
    _hold_route(shared, emu_lib, "push", tmp_path, extra)
    assert len(counted) > 2 * len(extra) and set(counted) == {(n // fb, 1, 1, 2)}


@pytest.mark.parametrize("route", ROUTES)
def test_skip_that_ends_inside_a_frame_and_budget_that_ends_inside_a_push(emu_lib, shared, tmp_path, route):
    """-S 0.0103 s = 20 frames and 4800 payload bytes; -T 0.0101 s: the budget of blocks is used up with a third of the stream
    still to come"""
    K, c, ref = _at(shared, emu_lib, "skip_budget", lambda: pc.Config(16.0, 32, 0.03, dict(freq_res=64, start=0.0103), total=0.0101))
    assert K.skip % (K.frame_bytes - K.header_bytes) == 4800
    info = c.get_info()
    nblocks = ref.W.nrows // info.rows_per_block
    assert 0 < nblocks and K.skip + nblocks * info.block_stride_bytes < 0.7 * (K.raw.size // K.frame_bytes) * 8000
    _hold_route(shared, emu_lib, route, tmp_path)


LANES = 176 | (3 << 24)


def test_scan_of_two_ifs_in_every_cut(emu_lib):
    """frbch_scan_device over two IFs with the digitiser's lane on: every IF's columns against that IF's own push run"""
    Ks = [pc.Config(-16.0 if i % 2 else 16.0, 128, 0.03, dict(freq_res=512, pol=5, flags=1 << 27, interval=0.006, maxb=2),
                    if_index=i + 1, overlap=LANES) for i in range(2)]
    chans = [K.open(emu_lib) for K in Ks]
    ds = []
    try:
        refs = [pc.Reference(c, K) for c, K in zip(chans, Ks)]
        info = chans[0].get_info()
        ds = [pc.DeviceRun(emu_lib, K, info, int(refs[0].W.nrows // info.rows_per_block)) for K in Ks]
        for name, cut in pc.device_cuts(ds[0].nblocks).items():
            pc.hold_scan(refs, chans, ds, cut, f"scan, cut {name}", exact=True)
    finally:
        for d in ds:
            d.free()
        for c in chans:
            c.close()


# ---- the cut generators themselves --------------------------------------------------------------------------------------------
def _smallest_stream():
    r = min((r for r in kt.ROWS if r.kind == "stream"), key=lambda r: r.secs * abs(r.bw))
    K = pc.Config(r.bw, r.nchan, r.secs, r.kw, frames=r.frames)
    freq_res = r.kw.get("freq_res", 0) or (512 if r.nchan <= 128 else 2 * r.nchan)
    return K, dict(total=K.raw.size, frame_bytes=K.frame_bytes, header_bytes=K.header_bytes, skip=K.skip, block_stride_bytes=r.nchan * freq_res)


@pytest.mark.parametrize("legacy", (0, 1))
def test_cuts_concatenate_to_the_stream_and_are_what_they_say(legacy):
    K, geo = _smallest_stream()
    if legacy:
        geo.update(header_bytes=16, frame_bytes=8016, total=geo["total"] // 8032 * 8016)
    total, fb, hb = geo["total"], geo["frame_bytes"], geo["header_bytes"]
    assert total % fb == 0 and total // fb >= 4
    cuts = {name: fn(**geo) for name, fn in pc.PUSH_CUTS.items()}
    cuts["ragged_b"] = pc.cut_ragged(seed=pc.RAGGED_SEEDS[1], **geo)
    for name, cut in cuts.items():
        assert sum(cut) == total and all(n >= 0 for n in cut), name
        assert all(n > 0 for n in cut) or name == "last_byte", name
    assert cuts["whole"] == [total]
    assert cuts["per_frame"] == [fb] * (total // fb)
    assert cuts["last_byte"] == [total - 1, 0, 1]
    ends = np.cumsum(cuts["headers"])[:-1]
    assert ends.size == total // fb and ((ends % fb >= 1) & (ends % fb <= hb - 1)).all()
    assert 5 in set(ends % fb) and len(set(ends % fb)) >= 4
    for name in ("ragged", "ragged_b"):
        assert min(cuts[name]) < hb and max(cuts[name]) > fb and max(cuts[name]) <= 3 * fb, (name, cuts[name])
        assert any(e % fb for e in np.cumsum(cuts[name])[:-1]), name
    edges = pc.block_edge_bytes(**geo)
    ends = set(np.cumsum(cuts["block_edges"])[:-1])
    assert len(edges) >= 2 and all({e - 1, e, e + 1} <= ends for e in edges)
    pb = fb - hb
    for k, e in enumerate(edges):                          # an edge is the stream byte of payload byte skip + (k + 1) x stride
        assert (e // fb) * pb + (e % fb - hb) == geo["skip"] + (k + 1) * geo["block_stride_bytes"] and e % fb >= hb


def test_block_cuts_and_the_batch_planner_mirror():
    assert pc.device_cuts(3) == {"whole": [3], "per_block": [1, 1, 1], "one_then_rest": [1, 2], "rest_then_one": [2, 1]}
    assert pc.device_cuts(1) == {"whole": [1]}
    assert list(pc.device_cuts(2)) == ["whole", "per_block"]
    assert set(pc.device_cuts(5)) == set(pc.DEVICE_CUTS)
    # plan_batches: equal sizes, no short tail launch
    assert pc.batches(3, 2) == [2, 1] and pc.batches(3, 1) == [1, 1, 1] and pc.batches(3, 3) == [3]
    assert pc.batches(7, 3) == [3, 3, 1] and pc.batches(5, 4) == [3, 2] and pc.batches(0, 2) == []
    assert pc.launch_edges([1, 2], 2) == [1, 3] and pc.launch_edges([5], 2) == [2, 4, 5]

