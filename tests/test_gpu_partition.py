"""The kernels that run in production give the same rows however the stream is cut (tests/partition_cases.py has the cuts, the
drivers and the assertions (a) - (f); tests/test_partition.py holds the emulator build to the same).

Every `stream` row of tests/kernel_table.py -- the smallest block that reaches each register-pass instantiation --, grouped by
configuration as tests/test_gpu_instantiations.py groups them, one case per (configuration, route): push / device / file.  The
cuts run at the row's own batch size (two blocks per launch), at one block per launch and, for the `whole` cuts, at three: the
same blocks are seen as 2 + 1, as 1 + 1 + 1 and as one launch of 3.  One handle per (configuration, batch size), reset between
the runs (frbch_reset keeps the staging areas: a run finds those of the cut before it).  No oracle run: library against library,
byte for byte; test_every_route_matches_the_oracle_digitiser ties three of the configurations to the oracle's digitiser."""
import numpy as np
import pytest

from tests import kernel_table as kt
from tests import parity_util as pu
from tests import partition_cases as pc
from tests.test_gpu_instantiations import _key

pytestmark = pytest.mark.gpu

ROUTES = ("push", "device", "file")
LANES = 192 | (3 << 24)                     # the lane setting of tests/test_gpu_instantiations.py::_run_scan


def _id(bw, nchan, kw, frames=None):
    text = ",".join(f"{k}={v}" for k, v in kw.items() if k not in ("interval", "dm", "coherent", "freq"))
    return f"{bw:g}|{nchan}|{text}" + ("|frames" if frames else "")


def _stream_configs():
    out, seen = [], set()
    for r in kt.ROWS:
        if r.kind == "stream" and _key(r) not in seen:
            seen.add(_key(r))
            out.append(r)
    return out


_STREAMS = _stream_configs()
_STREAM_CASES = [(i, route) for i, r in enumerate(_STREAMS) for route in ROUTES
                 if route == "push" or not pc.Config(r.bw, r.nchan, r.secs, r.kw, frames=r.frames).push_only]

# (e): a rescale per interval on the fast kernels; an interval is a block and a half, the stream 5.3 blocks.  128 and 1024
# channels, one and four products, the two-stage scrunch (1024 channels, -t 16); each with the statistics summed by K2 and in the
# separate pass (1 << 20)
_PER_INTERVAL = [
    (16.0, 128, dict(pol=2, nbit=8)),
    (-16.0, 128, dict(pol=4, nbit=16, tscr=8)),
    (32.0, 1024, dict(pol=1, nbit=2, tscr=2, freq_res=512)),
    (-32.0, 1024, dict(pol=4, nbit=8, tscr=16)),
]

_E_CASES = [(i, flags, route) for i in range(len(_PER_INTERVAL)) for flags in (0, pc.SEPARATE_STATS) for route in ROUTES]


@pytest.fixture(scope="module")
def shared():
    """the configuration the module's cases are at: its handles (one per batch size), its reference runs and its device frames,
    shared by the cases of one configuration (which run one behind the other) and released when the next one starts or the
    module ends"""
    state = {}
    yield state
    _release(state)


def _release(state):
    if state.get("d") is not None:
        state["d"].free()
    for c in state.get("handles", {}).values():
        c.close()
    state.clear()


def _at(state, lib, key, make, maxbs):
    """maxbs[0] = the configuration's own batch size: the reference runs are made at it"""
    if state.get("key") != key:
        _release(state)
        K = make()
        state.update(key=key, K=K, d=None, own=maxbs[0], handles={})
        for m in maxbs:
            state["handles"][m] = K.open(lib, maxb=m)
        state["ref"] = pc.Reference(state["handles"][maxbs[0]], K)
        state["info"] = state["handles"][maxbs[0]].get_info()
        state["nblocks"] = int(state["ref"].W.nrows // state["info"].rows_per_block)
    return state["K"], state["handles"], state["ref"]


def _device(state, lib):
    if state["d"] is None:
        state["d"] = pc.DeviceRun(lib, state["K"], state["info"], state["nblocks"])
    return state["d"]


def _hold_route(state, lib, route, tmp_path, exact):
    K, handles, ref, own = state["K"], state["handles"], state["ref"], state["own"]
    whole_only = [m for m in handles if m > own]             # the batch size that takes the whole run in one launch
    if route == "push":
        geo = dict(total=K.raw.size, **K.geometry(state["info"]))
        for m, c in handles.items():
            for name, fn in pc.PUSH_CUTS.items():
                if (m == own and name == "whole") or (m in whole_only and name != "whole"):
                    continue                                    # (the reference itself; cuts that never hold three blocks)
                cut = fn(**geo)
                pc.hold(ref, lambda frozen: pc.run_push(c, K.raw, cut, frozen), f"push, cut {name}, maxb {m}", exact)
    elif route == "file":
        path, out = str(tmp_path / "in.vdif"), str(tmp_path / "out.fil")
        K.raw.tofile(path)
        for m, c in handles.items():
            pc.hold(ref, lambda frozen: pc.run_file(c, path, out, frozen), f"run_file, maxb {m}", exact)
    else:
        d = _device(state, lib)
        for m, c in handles.items():
            for name, cut in pc.device_cuts(d.nblocks).items():
                if m in whole_only and name != "whole":
                    continue
                pc.hold(ref, lambda frozen: pc.run_device(c, d, cut, frozen), f"process_device, cut {name}, maxb {m}", exact, has_header=False)
        taps = [pc.hold_power(c, d, f"power_device, maxb {m}").rows for m, c in handles.items()]
        assert all(t == taps[0] for t in taps), "power tap: the floats depend on the blocks per launch"


@pytest.mark.parametrize("i,route", _STREAM_CASES, ids=[f"{_id(_STREAMS[i].bw, _STREAMS[i].nchan, _STREAMS[i].kw, _STREAMS[i].frames)}|{route}"
                                                        for i, route in _STREAM_CASES])
def test_every_cut_gives_the_rows_of_one_push(hip_lib, shared, tmp_path, i, route):
    r = _STREAMS[i]
    own = r.kw.get("maxb", 2)
    _at(shared, hip_lib, ("stream", i), lambda: pc.Config(r.bw, r.nchan, r.secs, r.kw, frames=r.frames), (own, 1, max(3, own + 1)))
    _hold_route(shared, hip_lib, route, tmp_path, exact=bool(r.kw.get("flags", 0) & pc.SEPARATE_STATS))


@pytest.mark.parametrize("i,flags,route", _E_CASES, ids=[f"{_id(*_PER_INTERVAL[i])}|flags={flags}|{route}" for i, flags, route in _E_CASES])
def test_a_rescale_per_interval_in_every_cut(hip_lib, shared, tmp_path, i, flags, route):
    """(e).  The stream holds at least three intervals; one of them ends strictly inside a launch of the `whole` push and at a
    launch boundary when every call carries one block"""
    bw, nchan, kw = _PER_INTERVAL[i]
    K, handles, ref = _at(shared, hip_lib, ("per_interval", i, flags), lambda: pc.per_interval_config(bw, nchan, kw, flags), (2, 1, 3))
    assert K.per_interval
    pc.check_interval_ends(shared["info"], shared["nblocks"], 2)
    for name in ("frbch_k1_branch", "frbch_k2_chan"):          # (128 channels have no register-pass Kc: frbch_kc_dcfix is theirs)
        assert name not in ref.W.record, f"(e) is for the fast kernels: {sorted(ref.W.record)}"
    _hold_route(shared, hip_lib, route, tmp_path, exact=bool(flags & pc.SEPARATE_STATS))


_SCANS = [r for r in kt.ROWS if r.kind == "scan"]


@pytest.mark.parametrize("overlap", (LANES, 0), ids=("lanes", "automatic"))
@pytest.mark.parametrize("i", range(len(_SCANS)), ids=[_id(r.bw, r.nchan, r.kw) for r in _SCANS])
def test_scan_of_two_ifs_in_every_cut(hip_lib, shared, i, overlap):
    """the `scan` rows through frbch_scan_device over two IFs: every IF's columns against that IF's own push run, under (a), (b),
    (c) and (f), the digitiser of a completed interval on the second lane included.  Batch sizes as for the stream rows: the row's
    own, 1, and 3 for the `whole` cut (the row's own is 1 and its run two blocks: 3 takes both in one launch)"""
    _release(shared)
    r = _SCANS[i]
    own = r.kw.get("maxb", 2)
    Ks = [pc.Config(r.bw if j % 2 else -r.bw, r.nchan, r.secs, r.kw, if_index=j + 1, overlap=overlap) for j in range(2)]
    sets = {m: [K.open(hip_lib, maxb=m) for K in Ks] for m in dict.fromkeys((own, 1, max(3, own + 1)))}
    ds = []
    try:
        refs = [pc.Reference(c, K) for c, K in zip(sets[own], Ks)]
        info = sets[own][0].get_info()
        ds = [pc.DeviceRun(hip_lib, K, info, int(refs[0].W.nrows // info.rows_per_block)) for K in Ks]
        exact = bool(r.kw.get("flags", 0) & pc.SEPARATE_STATS)
        for m, chans in sets.items():
            for name, cut in pc.device_cuts(ds[0].nblocks).items():
                if m > max(own, 1) and name != "whole":
                    continue
                pc.hold_scan(refs, chans, ds, cut, f"scan, cut {name}, maxb {m}", exact)
    finally:
        for d in ds:
            d.free()
        for chans in sets.values():
            for c in chans:
                c.close()


@pytest.mark.parametrize("bw,nchan,secs,kw", [
    (16.0, 128, 0.013517, dict(pol=2, nbit=8, interval=0.006083, maxb=2)),
    (-32.0, 1024, 0.216269, dict(pol=5, nbit=8, interval=0.097321, maxb=2)),                                  # two-pass (automatic with four products)
    (32.0, 256, 0.013517, dict(nbit=16, freq_res=512, dm=1.0, coherent=1, freq=1400.0, interval=0.006083, maxb=2)),
], ids=("128ch_pol2_8bit", "1024ch_pol5_two_pass", "256ch_coherent_16bit"))
def test_every_route_matches_the_oracle_digitiser(hip_lib, shared, bw, nchan, secs, kw):
    """one block per call and one frame per push: the integer codes of the run are the oracle's digitiser applied to the power tap
    of the whole run under the offset / scale that run measured"""
    _release(shared)
    K = pc.Config(bw, nchan, secs, kw)
    nbit = kw["nbit"]
    with K.open(hip_lib) as c:
        whole = pc.run_push(c, K.raw, [K.raw.size])
        info = c.get_info()
        if nchan == 1024:
            assert "frbch_k2_priv<5, 2>" in whole.record, sorted(whole.record)
        d = pc.DeviceRun(hip_lib, K, info, int(whole.nrows // info.rows_per_block))
        try:
            tap = pc.run_power(c, d, [d.nblocks])
            power = np.frombuffer(tap.rows, np.float32).reshape(d.rows, info.nif, nchan)
            runs = {"per_block": pc.run_device(c, d, [1] * d.nblocks),
                    "per_frame": pc.run_push(c, K.raw, pc.cut_per_frame(K.raw.size, K.frame_bytes))}
            for name, r in runs.items():
                assert r.nrows == d.rows
                got = pu.unpack_codes(np.frombuffer(r.rows, np.uint8), nbit, (d.rows, info.nif, nchan))
                want = pu.codes_from_hip_floats(power, r.rescale[0], r.rescale[1], nbit, usb=bw > 0)
                assert np.count_nonzero(got != want) == 0, f"{name}: codes differ from the oracle digitiser on the floats of the power tap"
        finally:
            d.free()

