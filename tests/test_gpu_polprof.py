"""GPU tests of the polarisation profile (frbch_polprof_*): the cases of tests/polprof_cases.py on the device.  The rows -- the
only device buffer of these entry points -- lie in a guarded buffer of exactly their size, checksummed and guard-checked behind
every call.  Each case runs at the aligned address (the fast kernel wherever the plan rule allows it) and 4 bytes off it (the
generic one), kernel_used asserted against frbch_polprof_kernel; fast = generic = tests/polprof_oracle.py byte for byte, and the
_host twin writes the same bytes as the _device one."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import post
from tests import big_rows as bg
from tests import polprof_cases as pc
from tests import rm_oracle as ro
from tests.hipmem import GuardedBuffer

pytestmark = pytest.mark.gpu

FAST, GENERIC = 1, 0
RAN = {}                      # case -> the forms that ran at the aligned address


def held(arr, misalign=0):
    """-> (guarded buffer of exactly the array's bytes (+ misalign in front), pointer to the array)"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = GuardedBuffer.from_numpy(np.concatenate([np.zeros(misalign, np.uint8), raw]) if misalign else raw)
    assert buf.ptr.value % 16 == 0
    return buf, C.c_void_p(buf.ptr.value + misalign)


def fast_layout(c, misalign):
    return (c["hdr"]["nchans"] * c["rows"].dtype.itemsize) % 64 == 0 and misalign % 16 == 0


def plan_expected(c, misalign):
    """the plan rule, restated: the layout of the fast burst-sums kernel, and tfactor + the largest delay spread of any 64-byte
    tile of any candidate <= 256 rows"""
    if not fast_layout(c, misalign):
        return GENERIC
    ct = 64 // c["rows"].dtype.itemsize
    spread = 0
    for cd in c["cands"]:
        d = ro.delays(c["hdr"], float(cd["dm"])).reshape(-1, ct)
        spread = max(spread, int((d.max(axis=1) - d.min(axis=1)).max()))
    return FAST if c["tfactor"] + spread <= 256 else GENERIC


def on_device(lib, c, misalign):
    """frbch_polprof_device on the case's rows -> (outputs, kernel_used, the plan query's answer)"""
    buf, ptr = held(c["rows"], misalign)
    want_kernel = pc.query(lib, c, ptr)
    with bg.guarded():
        code, msg, out, k = pc.call(lib.frbch_polprof_device, c, ptr, out=pc.outputs(c["cands"].size, c["nbin"], c["hdr"]["nchans"], fill=0xA5))
    assert code == 0, msg
    buf.check(contents=True)
    buf.free()
    return out, k, want_kernel


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_both_kernels_equal_the_oracle(hip_lib, name):
    c, want = pc.case(name), pc.want(name)
    for misalign in (0, 4):
        out, k, q = on_device(hip_lib, c, misalign)
        assert k[1] == q == plan_expected(c, misalign) and k[0] == (FAST if fast_layout(c, misalign) else GENERIC), (name, misalign, k, q)
        assert pc.same(out, want), (name, misalign)
        if misalign == 0:
            RAN[name] = q
            print("%s: the %s profile kernel at the aligned address" % (name, "fast" if q else "generic"))
    # 512 rows per bin never fit the stage of 256; 96 8-bit channels hold no whole tile
    if name in ("u8_64ch_8x512", "u8_96ch_ascending"):
        assert RAN[name] == GENERIC
    if name in ("u8_64ch_33x3", "u8_64ch_1x1", "u8_64ch_256x1", "u8_64ch_1024x2", "u16_64ch_coherency", "u8_64ch_flag_gain"):
        assert RAN[name] == FAST


def test_host_and_device_twins_write_the_same_bytes(hip_lib):
    for name in ("u8_64ch_33x3", "u16_64ch_coherency"):
        c = pc.case(name)
        out, k, _q = on_device(hip_lib, c, 0)
        code, msg, out2, k2 = pc.call(hip_lib.frbch_polprof_host, c, c["rows"].ctypes.data)
        assert code == 0, msg
        assert k2 == k == (FAST, FAST)
        for f in out:
            assert out[f].tobytes() == out2[f].tobytes(), (name, f)


def test_the_python_call_reports_its_kernels(hip_lib):
    c = pc.case("u8_1024ch_late")
    info = {}
    got = post.pol_profile(c["rows"], c["hdr"], c["cands"], c["rm"], nbin=c["nbin"], tfactor=c["tfactor"], ref=c["ref"], lib=hip_lib, info=info)
    assert info["spectra_kernel_used"] == FAST and info["kernel_used"] == plan_expected(c, 0)       # (the upload is 16-byte aligned)
    assert pc.same(got, pc.want("u8_1024ch_late"))


def test_the_int64_bound(hip_lib):
    """16384 channels x 16 bit at full scale with one sign, tfactor 512: the restatement, added up in Python integers, stays
    below 2^62, and the library agrees to the bit (512 rows per bin: the generic kernel at either address)"""
    c, want = pc.bound_case(), pc.bound_want()
    assert (1 << 56) < want["largest"] < (1 << 62) and int(np.abs(want["acc"]).max()) == want["largest"]
    out, k, q = on_device(hip_lib, c, 0)
    assert k == (FAST, GENERIC) and q == GENERIC
    assert pc.same(out, want)


def test_the_fast_kernel_near_the_int64_bound(hip_lib):
    """the same rows at tfactor 128: 512 tiles of 32 channels, sums of 2^57 through the shuffles, the partials and the join"""
    c, want = pc.bound_case(128), pc.bound_want(128)
    assert int(np.abs(want["acc"]).max()) == 16384 * (128 * 65535 // 4) * (1 << 22) and want["results"]["k"][0] == -2
    out, k, q = on_device(hip_lib, c, 0)
    assert k == (FAST, FAST) and q == FAST
    assert pc.same(out, want)


def test_known_answer(hip_lib):
    """the injected PA swing comes back within 4 pa_err on every strong bin, through the host entry point and the fast kernel"""
    c, injected = pc.known_case()
    info = {}
    got = post.pol_profile(c["rows"], c["hdr"], c["cands"], c["rm"], nbin=c["nbin"], tfactor=c["tfactor"], ref=c["ref"], lib=hip_lib, info=info)
    assert info["kernel_used"] == FAST
    assert pc.check_known(got["bins"][0], got["results"][0], injected) == pc.KNOWN_WIDTH
