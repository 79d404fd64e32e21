"""GPU tests of the fold refinement (frbch_foldfit_*, frbch_fold_refine_*): the cases of tests/foldfit_cases.py on the device.
The cube and its hits -- the only device buffers of these entry points -- lie in guarded buffers of exactly their size,
checksummed and guard-checked behind every call.  Each case runs at the aligned address (the fast kernels wherever the plan rule
allows them) and 4 bytes off it (the generic ones in both stages), kernel_used asserted against frbch_foldfit_kernel and against
the plan rule restated in foldfit_cases.plan_expected; fast = generic = tests/foldfit_oracle.py byte for byte, the _host twin
writes the same bytes as the _device one, the composite equals the two calls in sequence, and the known answer comes back."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import post
from tests import big_rows as bg
from tests import foldfit_cases as fc
from tests.hipmem import GuardedBuffer

pytestmark = pytest.mark.gpu

RAN = {}                      # case -> the forms that ran at the aligned address


def held(arr, misalign=0):
    """-> (guarded buffer of exactly the array's bytes (+ misalign in front), pointer to the array)"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = GuardedBuffer.from_numpy(np.concatenate([np.zeros(misalign, np.uint8), raw]) if misalign else raw)
    assert buf.ptr.value % 16 == 0
    return buf, C.c_void_p(buf.ptr.value + misalign)


def on_device(lib, c, misalign):
    """frbch_foldfit_device on the case's cube -> (outputs, kernel_used, the plan query's answer)"""
    cube, cube_ptr = held(c["cube"], misalign)
    hits, hits_ptr = held(c["hits"], misalign)
    q = fc.query(lib, c, cube_ptr, hits_ptr)
    with bg.guarded():
        code, msg, out, k = fc.call(lib.frbch_foldfit_device, c, cube_ptr, hits_ptr, out=fc.outputs(c, fill=0xA5))
    assert code == 0, msg
    for buf in (cube, hits):
        buf.check(contents=True)
        buf.free()
    return out, k, q


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_both_forms_equal_the_oracle(hip_lib, name):
    c, want = fc.case(name), fc.want(name)
    for misalign in (0, 4):
        out, k, q = on_device(hip_lib, c, misalign)
        assert k == q == fc.plan_expected(c, misalign == 0), (name, misalign, k, q)
        assert fc.same(out, want), (name, misalign, fc.differing(out, want))
        if misalign == 0:
            RAN[name] = k
            print("%s: stage 1 %s, stage 2 %s at the aligned address" % ((name,) + tuple("fast" if f else "generic" for f in k)))
    assert RAN[name] == fc.must_run(name)
    assert (name in fc.MUST_RUN_FAST_STAGE1) != (name in fc.MUST_RUN_GENERIC_STAGE1) and (name in fc.MUST_RUN_FAST_STAGE2) != (name in fc.MUST_RUN_GENERIC_STAGE2)


def test_host_and_device_twins_write_the_same_bytes(hip_lib):
    for name in ("nsub2_nbin64_short_last", "coherency_mask3_u16"):
        c = fc.case(name)
        out, k, _q = on_device(hip_lib, c, 0)
        code, msg, out2, k2 = fc.call(hip_lib.frbch_foldfit_host, c, c["cube"].ctypes.data, c["hits"].ctypes.data)
        assert code == 0, msg
        assert k2 == k == (1, 1)
        for f in out:
            assert out[f].tobytes() == out2[f].tobytes(), (name, f)


def test_the_python_call_reports_its_kernels(hip_lib):
    c = fc.case("dead_and_flagged_ascending")
    info = {}
    got = post.fold_fit(c["cube"], c["hits"], c["hdr"], c["nrows"], fc.par_of(c), flag=c["flag"], want_trials=True, lib=hip_lib, info=info)
    assert info == dict(kernel_used=(1, 1))                                      # (the upload is 16-byte aligned)
    assert fc.same(got, fc.want("dead_and_flagged_ascending"))


def test_known_answer_and_the_composite(hip_lib):
    """rows -> fold -> search in one residency on the device: the bytes of the two calls in sequence, every axis within one grid
    step of the truth, a better S/N than the nominal fold's"""
    seed = fc.KNOWN_SEEDS[0]
    got, info = fc.known_library(hip_lib, seed)
    assert info["kernel_used"][1:] == (1, 1)
    assert fc.known_recovered(got["results"][0])
    hdr, par, _truth, _steps = fc.known_setup()
    k, g = fc.KNOWN, fc.known_grid()
    rows = fc.known_rows(seed)
    cube, hits, _nbin = post.fold_all(type("F", (), dict(header=hdr, data=rows))(), par, nbin=k["nbin"], subint_s=k["subint_s"], lib=hip_lib)
    cube, hits = np.ascontiguousarray(cube.transpose(0, 1, 3, 2)), np.ascontiguousarray(hits.transpose(0, 2, 1))   # the library's layout
    fpar = post.foldfit_params(hdr, rows.shape[0], k["nbin"], cube.shape[0], g["f0_fold"], k["subint_s"], g["dm0"], products=1, ndm=g["ndm"],
                               nfreq=g["nfreq"], nfdot=g["nfdot"], ddm=g["ddm"], dfreq=g["dfreq"], dfdot=g["dfdot"], fit_frac=0.5,
                               widths=fc.KNOWN_WIDTHS)
    two = post.fold_fit(cube, hits, hdr, rows.shape[0], fpar, lib=hip_lib)
    assert fc.same(got, two), fc.differing(got, two)
