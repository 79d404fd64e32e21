"""GPU tests of the structure of a burst (frbch_burstacf_*, frbch_acf2d_*): the cases of tests/acf_cases.py on the device.  The rows
of the composite and the planes of the ACF stage lie in guarded buffers of exactly their size, checksummed and guard-checked
behind every call.  Each composite case runs at the aligned address (the fast burst-sums and dynamic-spectrum kernels wherever
their plan rules allow) and 4 bytes off it (the generic ones); kernel_used is asserted against frbch_burstacf_kernel and against
the plan rules restated in acf_cases; every form = tests/acf_oracle.py byte for byte.  The ACF stage runs in its fast form (the
plan rule places every case) and, asked for by `form`, in its generic form."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import acf_cases as ac
from tests import big_rows as bg
from tests.hipmem import GuardedBuffer
from tests.test_acf import check_known_answer, check_properties

pytestmark = pytest.mark.gpu

FAST, GENERIC = 1, 0


def held(arr, misalign=0):
    """-> (guarded buffer of exactly the array's bytes (+ misalign in front), pointer to the array)"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = GuardedBuffer.from_numpy(np.concatenate([np.zeros(misalign, np.uint8), raw]) if misalign else raw)
    assert buf.ptr.value % 16 == 0
    return buf, C.c_void_p(buf.ptr.value + misalign)


def fast_layout(c, misalign):
    return (c["hdr"]["nchans"] * c["rows"].dtype.itemsize) % 64 == 0 and misalign % 16 == 0


def acf_form(c):
    return FAST if ac.acf_plan(c["cands"].size, c["hdr"]["nchans"] // c["ffactor"], c["nbin"], c["nlagf"], c["nlagt"]) else GENERIC


def on_device(lib, c, misalign):
    """frbch_burstacf_device on the case's rows -> (outputs, kernel_used, the plan query's answer)"""
    buf, ptr = held(c["rows"], misalign)
    code, want_kernels = ac.query(lib, c, ptr)
    assert code == 0
    with bg.guarded():
        code, msg, out, k = ac.call(lib.frbch_burstacf_device, c, ptr, out=ac.outputs_of(c, fill=0xA5))
    assert code == 0, msg
    buf.check(contents=True)
    buf.free()
    return out, k, want_kernels


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_every_form_equals_the_oracle(hip_lib, name):
    c, want = ac.case(name), ac.want(name)
    for misalign in (0, 4):
        out, k, q = on_device(hip_lib, c, misalign)
        expected = (FAST if fast_layout(c, misalign) else GENERIC, ac.dyn_plan_expected(c, misalign == 0), acf_form(c))
        assert k == q == expected, (name, misalign, k, q, expected)
        assert ac.differing(out, want) == [], (name, misalign)
        if misalign == 0:
            print("%s: burst sums %d, dynamic spectrum %d, ACF %d (1 = fast)" % ((name,) + k))
            assert k[1] == (FAST if name in ac.DYN_FAST else GENERIC) and k[2] == FAST


def test_the_full_scale_case_reaches_its_magnitudes(hip_lib):
    c = ac.case("u8_1024ch_full_scale")
    out, k, _q = on_device(hip_lib, c, 0)
    r = out["results"][0]
    y = (out["Y"][0] + (1 << (int(r["r"]) - 1))) >> int(r["r"])
    print("r = %d, |y| = 2^%.3f .. 2^%.3f, A[0][0] = 2^%.3f" % (r["r"], np.log2(np.abs(y).min()), np.log2(np.abs(y).max()), np.log2(float(out["A"][0, 0, 1]))))
    assert k == (FAST, FAST, FAST) and r["ncomplete"] == 1 << 20 and r["r"] > 0
    assert (1 << 20) <= np.abs(y).min() and np.abs(y).max() <= (1 << 21) and int(out["A"][0, 0, 1]) > (1 << 60)


@pytest.mark.parametrize("name", sorted(ac.PLANES))
def test_acf_stage_both_kernels_equal_the_oracle(hip_lib, name):
    n, nsub, nbin, lf, lt, _kind = ac.PLANES[name]
    y, want = ac.plane(name), ac.plane_want(name)
    assert ac.acf_plan(n, nsub, nbin, lf, lt) is not None
    for form, ran in ((_lib.ACF_PLAN, FAST), (_lib.ACF_GENERIC, GENERIC)):
        assert hip_lib.frbch_acf2d_kernel(n, nsub, nbin, lf, lt, form) == ran
        ybuf = GuardedBuffer.from_numpy(y.view(np.uint8).reshape(-1))
        abuf = GuardedBuffer(want.nbytes)
        with bg.guarded():
            code, msg, _A, k = ac.acf2d_call(hip_lib.frbch_acf2d_device, ybuf.ptr, y.shape, lf, lt, form, A_ptr=abuf.ptr)
        assert code == 0 and k == ran, (msg, k)
        ybuf.check(contents=True)
        abuf.check()
        got = abuf.to_numpy(np.int64)
        ybuf.free()
        abuf.free()
        assert got.tobytes() == want.tobytes(), (name, form)
    # the _host twin, and the oracle-free properties on what the device wrote
    code, msg, A, k = ac.acf2d_call(hip_lib.frbch_acf2d_host, y.ctypes.data, y.shape, lf, lt)
    assert code == 0 and k == FAST and A.tobytes() == want.tobytes(), msg
    assert (A[:, 0, :] == A[:, 0, ::-1]).all()
    assert [int(v) for v in A[:, 0, lt - 1]] == [sum(int(v) ** 2 for v in p.reshape(-1)) for p in y]


def test_the_partials_cap_of_the_acf_plan(hip_lib):
    """the one shape class the fast ACF kernel does not take: partials of the slabs above 2^30 bytes (the plan query alone: such a
    call is hours of generic kernel)"""
    assert ac.acf_plan(1, 1024, 1024, 1024, 256) is not None and hip_lib.frbch_acf2d_kernel(1, 1024, 1024, 1024, 256, _lib.ACF_PLAN) == FAST
    assert ac.acf_plan(2, 1024, 1024, 1024, 256) is None and hip_lib.frbch_acf2d_kernel(2, 1024, 1024, 1024, 256, _lib.ACF_PLAN) == GENERIC


def test_a_plane_that_breaks_the_contract_is_refused(hip_lib):
    y = ac.plane("random_3x5_full_lags").copy()
    y[0, 1, 1] = -(ac.Y_MAX + 1)
    code, msg, A, _k = ac.acf2d_call(hip_lib.frbch_acf2d_host, y.ctypes.data, y.shape, 3, 5)
    assert code == _lib.E_ARG and "outside -2^21" in msg and (A == 0x5A5A5A5A5A5A5A5A).all()


@pytest.mark.parametrize("name", ("u8_64ch_f4_full_lags", "u8_64ch_windows_leave_the_file", "u8_64ch_flag_constant_dead", "u16_64ch_coherency"))
def test_properties_that_need_no_oracle(hip_lib, name):
    c = ac.case(name)
    info = {}
    got = post.burst_acf(c["rows"], c["hdr"], c["cands"], c["nbin"], c["tfactor"], c["ffactor"], c["nlagf"], c["nlagt"], fit_frac=c["fit_frac"],
                         flag=c["flag"], products="coherency" if c["coh"] else "stokes", lib=hip_lib, info=info)
    assert info == dict(spectra_kernel_used=FAST, dynspec_kernel_used=FAST, kernel_used=FAST)      # the Python call reports its kernels
    check_properties(hip_lib, c, got)


def test_host_and_device_twins_write_the_same_bytes(hip_lib):
    for name in ("u8_64ch_f1_full_lags", "u16_64ch_coherency", "u8_64ch_flag_constant_dead"):
        c = ac.case(name)
        out, k, _q = on_device(hip_lib, c, 0)
        code, msg, out2, k2 = ac.call(hip_lib.frbch_burstacf_host, c, c["rows"].ctypes.data)
        assert code == 0, msg
        assert k2 == k == (FAST, FAST, FAST)
        for f in out:
            assert out[f].tobytes() == out2[f].tobytes(), (name, f)


def test_refusals_leave_the_outputs_alone(hip_lib):
    c = ac.case("u8_64ch_f4_full_lags")
    for kw, text in ((dict(par=ac.par_of(c, ffactor=3)), "ffactor"), (dict(par=ac.par_of(c, nlagt=34)), "nlagt"),
                     (dict(fp=ac.fit_par_of(c, fit_frac=1.0)), "fit_frac"), (dict(hdr=dict(c["hdr"], nbits=32)), "float32")):
        code, msg, out, _k = ac.call(hip_lib.frbch_burstacf_host, c, c["rows"].ctypes.data, out=ac.outputs_of(c, fill=0xA5), **kw)
        assert code == _lib.E_ARG and text in msg, (kw, msg)
        assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), kw


@pytest.mark.parametrize("kind", ("drift", "control", "scint"))
def test_known_answer(hip_lib, kind):
    """the library's results are the oracle's bits and lie within the tolerances tests/test_acf.py derives (64 channels over 300 MHz
    are one 64-byte tile whose delays span 5600 rows: the plan rule sends the dynamic spectrum of this shape to the generic kernel)"""
    info = {}
    check_known_answer(hip_lib, kind, info)
    assert info == dict(spectra_kernel_used=FAST, dynspec_kernel_used=GENERIC, kernel_used=FAST)
