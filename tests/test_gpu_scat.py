"""GPU tests of the scattering of a burst (frbch_tbank_*, frbch_burstscat_*): the cases of tests/scat_cases.py on the device.  The
planes, the banks and the outputs of the stage and the rows of the composite lie in guarded, poisoned buffers of exactly their
size, checksummed and guard-checked behind every call, at the aligned address and 4 bytes off it.  The stage runs in its fast
form (the plan rule places every case) and, asked for by `form`, in its generic form; kernel_used is asserted against the plan
queries and against the rules restated in scat_cases; every form = tests/scat_oracle.py byte for byte."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import big_rows as bg
from tests import scat_cases as sc
from tests import scat_oracle as so
from tests.hipmem import GuardedBuffer
from tests.test_scat import check_known_answer

pytestmark = pytest.mark.gpu

FAST, GENERIC = 1, 0


def held(arr, misalign=0):
    """-> (guarded buffer of exactly the array's bytes (+ misalign in front), pointer to the array)"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = GuardedBuffer.from_numpy(np.concatenate([np.zeros(misalign, np.uint8), raw]) if misalign else raw)
    assert buf.ptr.value % 16 == 0
    return buf, C.c_void_p(buf.ptr.value + misalign)


@pytest.mark.parametrize("name", sorted(sc.PLANES))
def test_stage_both_kernels_equal_the_oracle(hip_lib, name):
    t = sc.PLANES[name]
    n = t[0]
    (y, P), want = sc.plane(name), sc.plane_want(name)
    assert sc.tbank_plan(*t[:8]) is not None
    for form, ran in ((_lib.TBANK_PLAN, FAST), (_lib.TBANK_GENERIC, GENERIC)):
        assert hip_lib.frbch_tbank_kernel(n, C.byref(sc.shape_of(name)), form) == ran
        for misalign in (0, 4):
            ybuf, yptr = held(y, misalign)
            pbuf, pptr = held(P, misalign)
            cbuf = GuardedBuffer(want.nbytes)
            with bg.guarded():
                code, msg, _C, k = sc.tbank_call(hip_lib.frbch_tbank_device, yptr, pptr, n, sc.shape_of(name), form, C_ptr=cbuf.ptr)
            assert code == 0 and k == ran, (msg, k)
            ybuf.check(contents=True)
            pbuf.check(contents=True)
            cbuf.check()
            got = cbuf.to_numpy(np.int64)
            for b in (ybuf, pbuf, cbuf):
                b.free()
            assert got.tobytes() == want.tobytes(), (name, form, misalign)
    code, msg, Cc, k = sc.tbank_call(hip_lib.frbch_tbank_host, y.ctypes.data, P.ctypes.data, n, sc.shape_of(name))
    assert code == 0 and k == FAST and Cc.tobytes() == want.tobytes(), msg


def test_the_full_scale_plane_reaches_2_to_61(hip_lib):
    y, P = sc.plane("full_scale_2_to_61")
    Cc = post.tbank(y, P, 0, 0, 8, lib=hip_lib)
    assert int(Cc[0, 0, 0, 0]) == 1 << 61 and int(Cc[0, 0, 0, 1]) == -(1 << 51) * 1023


def test_the_plan_query_of_the_largest_shapes(hip_lib):
    """what no test runs: the largest shapes the entry points accept, and more planes than the grid's third dimension, as plan
    queries alone"""
    for n, shape, ran in ((1, (1, 1024, 4096, 1024, 0, 0, 1024), FAST), (4, (64, 256, 512, 256, 64, 64, 128), FAST), (65536, (1, 1, 1, 1, 0, 0, 1), GENERIC),
                          (65535, (1, 1, 1, 1, 0, 0, 1), FAST)):
        assert hip_lib.frbch_tbank_kernel(n, C.byref(post.tbank_shape(*shape)), _lib.TBANK_PLAN) == ran
        assert (sc.tbank_plan(n, *shape) is not None) == (ran == FAST)
    assert hip_lib.frbch_tbank_kernel(8, C.byref(post.tbank_shape(64, 256, 512, 256, 64, 64, 128)), _lib.TBANK_PLAN) == _lib.E_ARG      # 2^25 sums


def test_a_plane_or_a_bank_that_breaks_the_contract_is_refused(hip_lib):
    y, P = (a.copy() for a in sc.plane("three_planes"))
    y[0, 1, 1] = -(so.Y_MAX + 1)
    code, msg, Cc, _k = sc.tbank_call(hip_lib.frbch_tbank_host, y.ctypes.data, P.ctypes.data, 3, sc.shape_of("three_planes"))
    assert code == _lib.E_ARG and "outside -2^21" in msg and (Cc == 0x5A5A5A5A5A5A5A5A).all()
    y[0, 1, 1] = 0
    P[0, 0] = so.P_MAX + 1
    code, msg, Cc, _k = sc.tbank_call(hip_lib.frbch_tbank_host, y.ctypes.data, P.ctypes.data, 3, sc.shape_of("three_planes"))
    assert code == _lib.E_ARG and "outside -2^30" in msg and (Cc == 0x5A5A5A5A5A5A5A5A).all()


def fast_layout(c, misalign):
    return (c["hdr"]["nchans"] * c["rows"].dtype.itemsize) % 64 == 0 and misalign % 16 == 0


def on_device(lib, c, misalign):
    """frbch_burstscat_device on the case's rows -> (outputs, kernel_used, the plan query's answer)"""
    buf, ptr = held(c["rows"], misalign)
    code, want_kernels = sc.query(lib, c, ptr)
    assert code == 0
    with bg.guarded():
        code, msg, out, k = sc.call(lib.frbch_burstscat_device, c, ptr, out=sc.outputs_of(c, fill=0xA5))
    assert code == 0, msg
    buf.check(contents=True)
    buf.free()
    return out, k, want_kernels


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_every_form_equals_the_oracle(hip_lib, name):
    c, want = sc.case(name), sc.want(name)
    for misalign in (0, 4):
        out, k, q = on_device(hip_lib, c, misalign)
        expected = (FAST if fast_layout(c, misalign) else GENERIC, sc.dyn_plan_expected(c, misalign == 0), FAST)
        assert k == q == expected, (name, misalign, k, q, expected)
        assert sc.differing(out, want) == [], (name, misalign)
    acf = sc.acf_of(hip_lib, c)                                      # Y and yhits are frbch_burstacf_*'s, to the bit
    assert out["Y"].tobytes() == acf["Y"].tobytes() and out["yhits"].tobytes() == acf["yhits"].tobytes()


def test_host_twin_and_python_call(hip_lib):
    c, want = sc.case("u8_64ch_flag_dead_subband"), sc.want("u8_64ch_flag_dead_subband")
    code, msg, out, k = sc.call(hip_lib.frbch_burstscat_host, c, c["rows"].ctypes.data)
    assert code == 0 and k == (FAST, FAST, FAST), msg
    assert sc.differing(out, want) == []
    info = {}
    got = post.burst_scatter(c["rows"], c["hdr"], c["cands"], c["nbin"], c["tfactor"], c["ffactor"], sc.bank_par(c["bp"]), c["shift0"], c["nshift"],
                             alphas=c["alphas"], snr_min=c["snr_min"], flag=c["flag"], lib=hip_lib, info=info)
    assert info == dict(spectra_kernel_used=FAST, dynspec_kernel_used=FAST, kernel_used=FAST)
    assert sc.differing(got, want) == [] and got["q"].tobytes() == want["q"].tobytes()
    assert got["bank"]["p"].tobytes() == c["bank"]["p"].tobytes()


def test_refusals_leave_the_outputs_alone(hip_lib):
    c = sc.case("u8_64ch_f4_mixed_dms")
    for kw, text in ((dict(par=sc.par_of(c, ffactor=3)), "ffactor"), (dict(par=sc.par_of(c, nshift=34)), "nshift"),
                     (dict(bp=sc.bank_par(dict(c["bp"], lead=24))), "lead"), (dict(fp=sc.fit_par_of(c, nalpha=0)), "nalpha"),
                     (dict(hdr=dict(c["hdr"], nbits=32)), "float32")):
        code, msg, out, _k = sc.call(hip_lib.frbch_burstscat_host, c, c["rows"].ctypes.data, out=sc.outputs_of(c, fill=0xA5), **kw)
        assert code == _lib.E_ARG and text in msg, (kw, msg)
        assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), kw


@pytest.mark.parametrize("scattered", (True, False))
def test_known_answer(hip_lib, scattered):
    """the library's results are the oracle's bits and lie within the tolerances tests/test_scat.py derives (64 channels over 300
    MHz are one 64-byte tile whose delays span 5600 rows: the plan rule sends the dynamic spectrum of this shape to the generic
    kernel)"""
    info = {}
    check_known_answer(hip_lib, scattered, info)
    assert info == dict(spectra_kernel_used=FAST, dynspec_kernel_used=GENERIC, kernel_used=FAST)
