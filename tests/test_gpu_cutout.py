"""GPU tests of the candidate cut-outs (frbch_cutout_*): the LDS kernel frbch_post_cutout_lds<BPV, KIND> (both sample widths,
both plane kinds) and the generic kernel it falls back to, on the cases of tests/cutout_cases.py against the numpy restatement
tests/cutout_oracle.py -- every plane to the bit: integer sums are exact, float rows are summed in the stated order, so there
is no tolerance anywhere.  Every case asserts `kernel_used`, against frbch_cutout_kernel for the same address and against the
documented rule restated in cutout_cases.lds_expected."""
import ctypes as C
import contextlib
import faulthandler
import io
import json

import numpy as np
import pytest

from frb_baseband_amd import post, process_vdif as pv, sigproc, synth
from tests import cutout_cases as cc
from tests import cutout_oracle as co
from tests.hipmem import GuardedBuffer as DeviceBuffer, hip
from tests.test_cutout import candidates_round_trip

pytestmark = pytest.mark.gpu

CALL_LIMIT_S = 120          # a device call that has not come back by then ends the test process (traceback on stderr)

# what the rule says of every case: a predicate that fell back to "never" (or "always") turns these red
GENERIC_CASES = {"c48_b16_nf48_nt32_ndm9_batch5", "c128_b32_nf1_nt16_ndm13", "c128_b32_batch5", "c64_b8_dm_hi_delay_past_nrows",
                 "c64_b8_ndm8_dm_hi_3000_spans_more_than_the_lds"}


def cutout_device(lib, cs, shift=0):
    """frbch_cutout_device on rows resident `shift` bytes behind a 16-byte aligned device address
    -> (planes, kernel_used, what frbch_cutout_kernel says of that address)"""
    rows, cands = cs["rows"], np.ascontiguousarray(cs["cands"])
    buf = DeviceBuffer(rows.nbytes + 16)
    assert buf.ptr.value % 16 == 0
    d_rows = C.c_void_p(buf.ptr.value + shift)
    assert hip().hipMemcpy(d_rows, rows.ctypes.data, rows.nbytes, 1) == 0
    host = cc.empty_planes(cs)
    dev = [DeviceBuffer.from_numpy(h) for h in host]
    par = cc.params(cs["nt"], cs["nf"], cs["ndm"])
    says = cc.cutout_kernel(lib, cs, d_rows.value)
    used = C.c_uint32(99)
    err = C.create_string_buffer(512)
    faulthandler.dump_traceback_later(CALL_LIMIT_S, exit=True)
    try:
        rc = lib.frbch_cutout_device(C.byref(cc.desc_of(cs)), d_rows, rows.shape[0], C.byref(par), cands.ctypes.data, cands.size, 0,
                                     dev[0].ptr, dev[1].ptr, dev[2].ptr, dev[3].ptr, C.byref(used), err, len(err))
    finally:
        faulthandler.cancel_dump_traceback_later()
    assert rc == 0, err.value
    got = tuple(d.to_numpy(h.dtype).reshape(h.shape) for d, h in zip(dev, host))
    for d in dev + [buf]:
        d.free()
    return got, used.value, says


# ---- the grid of the emulator tests, and the shapes that reach the LDS kernel -------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES) + sorted(cc.DEVICE_CASES))
def test_device_equals_the_restatement(hip_lib, name):
    """64 / 48 / 128 / 192 / 512 / 1024 channels of 8 / 16 / 32 bits; frequency bins smaller than, equal to, larger than and across a
    64-byte channel tile; 1 .. 256 trial DMs (partial groups of 8); tfactor 1 .. 512 with whole and partial time tiles, two bins,
    one bin and a bin longer than the tile; batches of 1 .. 33 with mixed tfactor; windows that start before row 0, end past
    nrows or lie wholly outside; another product of several; foff of both signs"""
    cs, want = cc.case(name)
    kernel = cc.lds_expected(cs)
    assert kernel == (cc.GENERIC if name in GENERIC_CASES else cc.LDS)
    got, used, says = cutout_device(hip_lib, cs)
    assert used == says == kernel
    assert cc.same_planes(got, want), cc.which_differ(got, want)


@pytest.mark.parametrize("name", ["c64_b8_nf16_nt16_ndm8", "c1024_b8_nf16", "c512_b16_nf64", "c64_b8_starts_before_row0",
                                  "c64_b8_ends_past_nrows", "edge_nt4_f300"])
def test_rows_off_a_16_byte_boundary_take_the_generic_kernel(hip_lib, name):
    """the same rows at an aligned address (LDS kernel) and 4 bytes behind one (generic): the same bits, which are also
    frbch_cutout_host's"""
    cs, want = cc.case(name)
    got, used, says = cutout_device(hip_lib, cs, 0)
    assert used == says == cc.LDS and cc.same_planes(got, want), cc.which_differ(got, want)
    got4, used4, says4 = cutout_device(hip_lib, cs, 4)
    assert used4 == says4 == cc.GENERIC and cc.same_planes(got4, got), cc.which_differ(got4, got)
    rc, host, used_h, msg = cc.cutout_host(hip_lib, cs)
    assert rc == 0 and used_h == cc.LDS and cc.same_planes(host, got), msg


# ---- end to end ---------------------------------------------------------------------------------------------------------
def test_candidates_fil_end_to_end(hip_lib, tmp_path):
    """the burst file through post.candidates_fil: one candidate, its planes show the burst where the known answer says"""
    candidates_round_trip(hip_lib, tmp_path, cc.LDS)


def test_cutouts_of_the_rows_the_channeliser_writes(hip_lib, tmp_path):
    """0.3 s of a 32 MHz IF through the channeliser with pol = 4, 8 bit, 1024 channels; the .fil read back: the planes of three
    candidates on product 0 and on product 1 of its rows against the restatement"""
    vd = str(tmp_path / "pr001a_ef_no0001_IF1.vdif")
    synth.make_vdif(0.3, bw_mhz=32.0, nchan=1024).tofile(vd)
    hdr = pv.make_hdr("J0000+00", 1400.0, vd, pol=4, usb=True, ra="00:00:00", dec="00:00:00", bw=32.0, telescope="effelsberg")
    with contextlib.redirect_stdout(io.StringIO()):
        path = pv.run_digifil(hdr, str(tmp_path), 0, 0.3, 1024, overwrite=True, pol=4, nbit=8)
    fil = sigproc.read_fil(path)
    h = fil.header
    rows = np.ascontiguousarray(fil.data)
    assert h["nifs"] == 4 and h["nchans"] == 1024 and h["nbits"] == 8 and rows.shape[0] >= 5000
    cands = cc.cands_of((56.7, 2500, 1), (30.0, 40, 3), (40.0, rows.shape[0] - 100, 7))
    for prod in (0, 1):
        info = {}
        got = post.cutouts(fil, dict(h, product=prod), cands, nt=32, nf=0, ndm=16, lib=hip_lib, info=info)
        assert cc.lds_expected(dict(hdr=h, cands=cands, nf=256, ndm=16)) == cc.LDS
        assert info["kernel_used"] == cc.LDS and got[0].shape == (3, 256, 32)
        want = co.planes_batch(rows[:, prod, :], h, cands, 32, 256, 16)
        assert cc.same_planes(got, want), cc.which_differ(got, want)
        dev, used, says = cutout_device(hip_lib, dict(hdr=h, rows=rows, prod=prod, nt=32, nf=256, ndm=16, cands=cands))
        assert used == says == cc.LDS and cc.same_planes(dev, want), cc.which_differ(dev, want)
    assert not np.array_equal(rows[:, 0], rows[:, 1])


# ---- timing -------------------------------------------------------------------------------------------------------------
def test_one_batched_call_beats_a_dedispersion_per_candidate(hip_lib):
    """10 s x 1024 channels of 8-bit rows resident in HBM (made there with torch), 32 candidates with tfactor 1 .. 15 at DMs
    300 .. 331, nt = ndm = 256: after one warm-up of each side, the median of five frbch_cutout_device calls for all 32 is at most
    the median of five rounds of what the library offered before -- 32 frbch_dedisperse_device calls, one per candidate on its
    row window with the same 256 DMs, which do strictly less (no time binning, no frequency-time plane).  Margin 1.0."""
    torch = pytest.importorskip("torch")
    gen = torch.Generator(device="cuda").manual_seed(5)
    rows = torch.randint(100, 156, (cc.TIMING_ROWS, cc.TIMING_HDR["nchans"]), dtype=torch.uint8, device="cuda", generator=gen)
    torch.cuda.synchronize()
    stats = cc.timing_run(hip_lib, rows.data_ptr())
    print("CUTOUT-TIMING " + json.dumps(stats))
    assert stats["kernel_used"] == cc.LDS
    assert stats["cutout_device_median_s"] <= 1.0 * stats["dedisperse_device_x32_median_s"], stats
