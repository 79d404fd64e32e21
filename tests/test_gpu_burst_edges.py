"""GPU tests of the burst polarisation kernels at the edges of their plans: the cases of tests/burst_edge_cases.py on the device.
The rows lie in a guarded buffer of exactly their size, checksummed and guard-checked behind every call, the sums in another.
Each case runs at the aligned address (the fast kernel wherever the plan allows it) and 4 bytes off it (the generic one);
kernel_used is asserted against the query and against the restated plan rule; sums, spectra, acc, hits, bins and results are
compared byte for byte (pa, which goes through libm's atan2, to 1e-12 as everywhere).  One case reads the profile across the
2^32-byte mark of 4.4 GB of rows."""
import time

import pytest

from tests import big_rows as bg
from tests import burst_edge_cases as bc
from tests import polprof_cases as pc
from tests.hipmem import GuardedBuffer

pytestmark = pytest.mark.gpu

FAST, GENERIC = bc.FAST, bc.GENERIC


# ---- burst sums ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bc.BURST_CASES))
def test_burst_sums_equal_the_restatement_in_both_kernels(hip_lib, name):
    """documented_maximum (2.16 x 10^6 rows, 132 MiB) is the one case that may take more than a few seconds: measured 1.9 s on the
    device's host with both kernels, most of it the case and its restatement (4.5 s of them on a slower host)"""
    t = time.time()
    assert bc.check_burst_case(hip_lib, name) == [FAST, GENERIC]
    print("%s: %.1f s" % (name, time.time() - t))


# ---- the profile -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bc.PROF_CASES))
def test_profile_equals_the_oracle_in_both_kernels(hip_lib, name):
    ran = bc.check_prof_case(hip_lib, name)
    assert ran == [bc.PROF_CASES[name][1], GENERIC]
    print("%s: the %s profile kernel at the aligned address" % (name, "fast" if ran[0] else "generic"))


def test_host_and_device_twins_write_the_same_bytes(hip_lib):
    c = bc.prof_case("spread_255_t1")
    out, k, _q = bc.profile_on(hip_lib, c)
    code, msg, out2, k2 = pc.call(hip_lib.frbch_polprof_host, c, c["rows"].ctypes.data)
    assert code == 0 and k2 == k == (FAST, FAST), msg
    for f in out:
        assert out[f].tobytes() == out2[f].tobytes(), f


def test_the_partials_cap(hip_lib):
    """the plan query alone, nothing is launched: 56 candidates' partials fit 2^30 bytes, 57 candidates' do not; only the address
    of the rows is examined (a buffer of 64 bytes stands for them)"""
    buf = GuardedBuffer(64)
    try:
        for ncand, kernel in ((56, FAST), (57, GENERIC)):
            c = bc.partials_cap(ncand)
            assert bc.plan(c)[0] == kernel and pc.query(hip_lib, c, buf.ptr) == kernel, ncand
            assert bc.plan(c, 4)[0] == GENERIC and pc.query(hip_lib, c, buf.ptr.value + 4) == GENERIC
    finally:
        buf.free()


# ---- past the 4 GiB mark ---------------------------------------------------------------------------------------------
def test_the_profile_beyond_the_4gib_mark(hip_lib):
    """8192 channels x 4 products x 8 bit, 4.4 GB of rows, DM 104 (tile spread 17, delays up to 1648 rows): bins wholly behind the
    2^32-byte row, bins 800 rows in front of it whose delayed tiles are staged from both sides of it, a candidate near row 1000
    and one whose bins run off nrows.  The fast kernels at the aligned address, the generic ones 4 bytes further on."""
    br = bg.big("A8")
    assert (br.byte_mark_rows[-1] + 300) * br.row_bytes > 1 << 32
    pc.check_beyond_the_mark(hip_lib, br, bg.DeviceMem, behind=300, front=800, off_len=200, nbin=64, tfactor=3,
                             kernels=((0, FAST, FAST), (4, GENERIC, GENERIC)))
