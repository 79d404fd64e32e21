"""GPU tests of the DM scan (frbch_dmscan_*): the cases of tests/dmscan_cases.py on the device.  The rows -- the only device
buffer of these entry points -- lie in a guarded buffer of exactly their size, checksummed and guard-checked behind every call.
Each case runs at the aligned address (the fast kernel wherever the plan rule allows it) and 4 bytes off it (the generic one),
kernel_used asserted against frbch_dmscan_kernel and against the plan rule restated in dmscan_cases.plan_expected; fast =
generic = tests/dmscan_oracle.py byte for byte, and the _host twin writes the same bytes as the _device one."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import post
from tests import big_rows as bg
from tests import dmscan_cases as dc
from tests.hipmem import GuardedBuffer

pytestmark = pytest.mark.gpu

FAST, GENERIC = 1, 0
RAN = {}                      # case -> the form that ran at the aligned address


def held(arr, misalign=0):
    """-> (guarded buffer of exactly the array's bytes (+ misalign in front), pointer to the array)"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = GuardedBuffer.from_numpy(np.concatenate([np.zeros(misalign, np.uint8), raw]) if misalign else raw)
    assert buf.ptr.value % 16 == 0
    return buf, C.c_void_p(buf.ptr.value + misalign)


def fast_layout(c, misalign):
    return (c["hdr"]["nchans"] * c["rows"].dtype.itemsize) % 64 == 0 and misalign % 16 == 0


def on_device(lib, c, misalign):
    """frbch_dmscan_device on the case's rows -> (outputs, kernel_used, the plan query's answer)"""
    buf, ptr = held(c["rows"], misalign)
    want_kernel = dc.query(lib, c, ptr)
    with bg.guarded():
        code, msg, out, k = dc.call(lib.frbch_dmscan_device, c, ptr,
                                    out=dc.outputs(c["cands"].size, c["ntrial"], c["nbin"], c["hdr"]["nchans"], fill=0xA5))
    assert code == 0, msg
    buf.check(contents=True)
    buf.free()
    return out, k, want_kernel


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_both_kernels_equal_the_oracle(hip_lib, name):
    c, want = dc.case(name), dc.want(name)
    for misalign in (0, 4):
        out, k, q = on_device(hip_lib, c, misalign)
        assert k[1] == q == dc.plan_expected(c, misalign == 0), (name, misalign, k, q)
        assert k[0] == (FAST if fast_layout(c, misalign) else GENERIC), (name, misalign, k)
        assert dc.same(out, want), (name, misalign, [f for f in dc.FIELDS if out[f].tobytes() != np.ascontiguousarray(want[f]).tobytes()])
        if misalign == 0:
            RAN[name] = q
            print("%s: the %s scan kernel at the aligned address" % (name, "fast" if q else "generic"))
    assert RAN[name] == (FAST if name in dc.MUST_RUN_FAST else GENERIC) and (name in dc.MUST_RUN_FAST) != (name in dc.MUST_RUN_GENERIC)


def test_host_and_device_twins_write_the_same_bytes(hip_lib):
    for name in ("u8_64ch_33x33x3", "u16_64ch_coherency"):
        c = dc.case(name)
        out, k, _q = on_device(hip_lib, c, 0)
        code, msg, out2, k2 = dc.call(hip_lib.frbch_dmscan_host, c, c["rows"].ctypes.data)
        assert code == 0, msg
        assert k2 == k == (FAST, FAST)
        for f in out:
            assert out[f].tobytes() == out2[f].tobytes(), (name, f)


def test_the_python_call_reports_its_kernels(hip_lib):
    c = dc.case("u8_64ch_flag_constant_dead")
    info = {}
    got = post.dm_scan(c["rows"], c["hdr"], c["cands"], c["ntrial"], c["ddm"], c["nbin"], c["tfactor"], widths=c["widths"], smooth=c["smooth"],
                       fit_frac=c["fit_frac"], flag=c["flag"], lib=hip_lib, info=info)
    assert info == dict(spectra_kernel_used=FAST, kernel_used=FAST)                    # (the upload is 16-byte aligned)
    assert dc.same(got, dc.want("u8_64ch_flag_constant_dead"))


def test_known_answer(hip_lib):
    """the library's estimates are the oracle's bits, through the host entry point, and lie within two DM sample steps of the
    injected DM (64 channels over 300 MHz are one 64-byte tile whose delays span 5600 rows: the plan rule sends this shape to the
    generic scan kernel; the burst sums run fast)"""
    hdr, cands, grid, step = dc.known_scan_args()
    want, _ = dc.known_oracle(dc.KNOWN_SEED)
    info = {}
    rows = dc.known_rows(dc.KNOWN_SEED)
    got = post.dm_scan(rows, hdr, cands, widths=dc.WIDTHS, smooth=dc.SMOOTH, fit_frac=dc.FIT_FRAC, lib=hip_lib, info=info, **grid)
    assert info == dict(spectra_kernel_used=FAST, kernel_used=dc.plan_expected(dict(grid, hdr=hdr, rows=rows, cands=cands, coh=False), True))
    assert info["kernel_used"] == GENERIC and dc.same(got, want)
    r = got["results"][0]
    assert r["fitted_snr"] == 1 and r["fitted_struct"] == 1
    assert abs(r["dm_snr"] - dc.KNOWN_DM) <= 2.0 * step and abs(r["dm_struct"] - dc.KNOWN_DM) <= 2.0 * step


def test_drifting_halves(hip_lib):
    """two half-band components 8 rows apart: the S/N estimate lies further from the injected DM than the structure estimate, by 5
    DM sample steps or more (tests/test_dmscan.py says where the 5 comes from)"""
    hdr, cands, grid, step = dc.known_scan_args()
    want, _ = dc.known_oracle(dc.KNOWN_SEED, dc.DRIFT_ROWS)
    got = post.dm_scan(dc.known_rows(dc.KNOWN_SEED, dc.DRIFT_ROWS), hdr, cands, widths=dc.WIDTHS, smooth=dc.SMOOTH, fit_frac=dc.FIT_FRAC,
                       lib=hip_lib, **grid)
    assert dc.same(got, want)
    r = got["results"][0]
    assert abs(r["dm_snr"] - dc.KNOWN_DM) / step - abs(r["dm_struct"] - dc.KNOWN_DM) / step >= 5.0
