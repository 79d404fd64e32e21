"""Every register-pass kernel instantiation of the channeliser, run against the fp64 oracle (tests/kernel_table.py).

Each row runs its configuration through the C ABI with profiling on, compares the output with the oracle under the bounds of
parity_util (check_codes, the rescale check; nothing new, nothing wider), and then reads the library's launch record: the row's
instantiation was launched, and the generic kernel of its stage was not.  The record names what ran (the full template
arguments, the fallbacks), where a timing slot names what was planned.

Rows with the same configuration share one run.  The rows that point at tests/test_gpu_parity.py::CASES (2^26-sample blocks) are
asserted there, on the run those cases pay for anyway."""
import numpy as np
import pytest

from frb_baseband_amd import channeliser as ch
from frb_baseband_amd import multi_if, sigproc, synth
from oracle import frb_oracle as o
from tests import kernel_table as kt
from tests import parity_util as pu
from tests.hipmem import GuardedBuffer as DeviceBuffer
from tests.test_kernel_table import library_kernels

pytestmark = pytest.mark.gpu

_RUNS: dict = {}       # configuration -> launch record, or the exception its run raised
_ALL_NAMES: set = set()


def _key(r):
    return (r.kind, r.bw, r.nchan, r.secs, tuple(sorted(r.kw.items())), repr(r.frames))


def _run_stream(lib, r):
    rec = {}
    pu.run_streaming_case(lib, r.bw, r.nchan, r.secs, record=rec, **r.kw, **({"frames": r.frames} if r.frames else {}))
    return rec


def _run_scan(lib, r, nif=2):
    """two IFs through frbch_scan_device with the digitiser of a completed rescale interval beside the next IF's K1 (192 CUs left
    to K1, the rest held by the digitiser's LDS reservation), every IF's columns against the oracle"""
    raws = [synth.make_vdif(r.secs, bw_mhz=r.bw, nchan=r.nchan, if_index=i + 1) for i in range(nif)]
    bufs = [DeviceBuffer.from_numpy(x) for x in raws]
    okw = {k: v for k, v in r.kw.items() if k not in ("maxb", "flags")}
    chans, ocfgs, rec = [], [], {}
    try:
        for i in range(nif):
            sbw = r.bw if i % 2 else -r.bw
            cfg = pu.lib_cfg(lib, sbw, r.nchan, r.secs, **r.kw)
            cfg.overlap = 192 | (3 << 24)
            chans.append(ch.Channeliser(cfg, lib))
            chans[-1].set_profiling(True)
            ocfgs.append(pu.oracle_cfg(sbw, r.nchan, r.secs, **okw))
        info = chans[0].info
        nfr = raws[0].size // 8032
        nblocks = (nfr * 8000) // info.block_payload_bytes
        rows = nblocks * info.rows_per_block
        out = DeviceBuffer(rows * nif * info.row_bytes)
        assert multi_if.scan_device(chans, [b.ptr.value for b in bufs], nfr, 8032, 32, 0, nblocks, out.ptr.value, rows) == rows
        data = out.to_numpy(np.uint8).reshape(rows, info.nif, nif * r.nchan)
        for c in chans:
            for name, v in c.get_launch_record().items():
                rec.setdefault(name, v)
    finally:
        for c in chans:
            c.close()
    for i, (raw, ocfg) in enumerate(zip(raws, ocfgs)):
        want = sigproc.read_fil(o.channelise(raw, ocfg)).data[:rows]
        pu.check_code_arrays(want, data[:, :, i * r.nchan:(i + 1) * r.nchan], ocfg)
    return rec


def _run_tap(lib, r):
    """the unpack tap with the register decoders (decoder 1: the nibble table of frbch_k1_wave, the select chain of frbch_k1_fast)
    on frames that hold every byte value: exactly the oracle's voltages"""
    from frb_baseband_amd import vdif
    payload = (np.arange(16000, dtype=np.uint32) * 37 % 256).astype(np.uint8)
    payload[:256] = np.arange(256, dtype=np.uint8)
    raw = vdif.frame_payload(payload, bw_mhz=32.0, bits=2)
    d_raw = DeviceBuffer.from_numpy(raw)
    nsamp = payload.size * 2
    want = o.unpack_2bit(payload, np.array([-3.3359, -1.0, 1.0, 3.3359], np.float32)).astype(np.float32)
    with ch.Channeliser(pu.lib_cfg(lib, 32.0, 1024, 1.0), lib) as c:
        c.set_profiling(True)
        v1 = DeviceBuffer(4 * nsamp * 4)
        c.unpack_device(d_raw.ptr.value, 2, 8032, 32, 0, nsamp, 1, v1.ptr.value, v1.nbytes)
        got = v1.to_numpy(np.float32).reshape(2, 2, nsamp)
        rec = c.get_launch_record()
    assert set(np.unique(payload)) == set(range(256))
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    return rec


_RUNNERS = {"stream": _run_stream, "scan": _run_scan, "tap": _run_tap}
_ROWS = [r for r in kt.ROWS if r.kind != "case"]


def _id(r):
    kw = ",".join(f"{k}={v}" for k, v in r.kw.items() if k not in ("interval", "dm", "coherent", "freq"))
    return f"{r.name}|{r.bw:g}|{r.nchan}|{kw}" + ("|frames" if r.frames else "")


@pytest.mark.parametrize("r", _ROWS, ids=[_id(r) for r in _ROWS])
def test_instantiation_matches_oracle_and_is_the_kernel_that_ran(hip_lib, r):
    key = _key(r)
    if key not in _RUNS:
        try:
            _RUNS[key] = _RUNNERS[r.kind](hip_lib, r)
        except BaseException as exc:   # (rows that share the run fail with it)
            _RUNS[key] = exc
    rec = _RUNS[key]
    if isinstance(rec, BaseException):
        raise rec
    _ALL_NAMES.update(rec)
    for name in (r.name,) + r.also:
        assert name in rec and rec[name]["launches"] >= 1, (name, sorted(rec))
    generic = kt.STAGE_GENERIC[kt.family(r.name)]
    if generic is not None and generic not in r.also:
        assert generic not in rec, f"{generic} ran beside {r.name}: {sorted(rec)}"
    # persistent loops: the grid is at its cap, so the tiles of the launch exceed it (the row's comment has the arithmetic)
    if r.grid_x is not None:
        assert rec[r.name]["grid_x"] == r.grid_x, rec[r.name]
    if r.grid_y is not None:
        assert rec[r.name]["grid_y"] == r.grid_y, rec[r.name]


def test_every_recorded_name_is_a_kernel_of_the_library():
    """a name a selector misspells would be recorded, but is no symbol of the library (the union of the records of all rows above)"""
    assert _ALL_NAMES, "runs behind the rows of this module"
    assert _ALL_NAMES <= library_kernels(), sorted(_ALL_NAMES - library_kernels())
