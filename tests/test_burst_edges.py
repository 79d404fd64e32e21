"""CPU tests of the burst polarisation kernels at the edges of their plans (tests/burst_edge_cases.py): the second restatement of
the burst sums held to tests/rm_oracle.py, every oracle-side condition of the cases -- tile spreads, rows walked and trips of
the chunk loop, the 2^53 bound, the sample floors, the plan's answers --, and the same cases through the emulator build, which
runs the generic kernels (kernel_used 0 at either address), byte for byte.  tests/test_gpu_burst_edges.py runs them on the
device."""
import time

import numpy as np
import pytest

from tests import big_rows as bg
from tests import burst_edge_cases as bc
from tests import polprof_cases as pc
from tests import rm_cases as rc
from tests import rm_oracle as ro

SMALL = sorted(set(bc.BURST_CASES) - set(bc.LARGE))


# ---- the second restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in rc.CASES if not n.startswith("f32")))
def test_window_sums_equal_the_row_walk(name):
    hdr, rows, cands, _coh = rc.case(name)
    assert bc.window_sums(rows, hdr, cands).tobytes() == rc.want_spectra(name)[0].tobytes()


@pytest.mark.parametrize("name", SMALL)
def test_window_sums_equal_the_row_walk_on_the_small_cases_here(name):
    """one to three products, ascending bands, and the two windows of 16384 and 16385 walked rows"""
    hdr, rows, cands, _coh = bc.burst_case(name)
    assert bc.burst_want(name)[0].tobytes() == ro.burst_sums(rows, hdr, cands).tobytes()


def test_window_sums_on_windows_cut_at_both_ends_and_wholly_outside():
    """a file shorter than its windows, a candidate in front of row 0 and one behind the last row"""
    hdr, rows, _cands, _coh = rc.case("u8_64ch_3cand")
    x = rows[:700]
    cands = rc.cands_of([dict(rc.B1, sample=300), dict(rc.B1, sample=-5000), dict(rc.B1, sample=1 << 62), dict(rc.B1, sample=690)], 16, 400)
    got, want = bc.window_sums(x, hdr, cands), ro.burst_sums(x, hdr, cands)
    assert got.tobytes() == want.tobytes()
    assert 0 < want["off_hits"][0].max() < 800 and not want["off_hits"][1:3].any() and want["on_hits"][3].min() == 0 < want["on_hits"][3].max()


# ---- the conditions --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bc.BURST_CASES))
def test_burst_conditions(name):
    bc.burst_conditions(name)


@pytest.mark.parametrize("name", sorted(bc.PROF_CASES))
def test_profile_conditions(name):
    bc.prof_conditions(name)


def test_the_limit_of_the_plan_is_met_from_both_sides():
    """DM 171.1 / 171.8 give tile spreads of 255 / 256 rows in either band sense; the stage takes tfactor + spread <= 256"""
    for sign in (-1, 1):
        hdr = dict(rc.make_hdr(64, foff_sign=sign), nbits=8)
        assert int(bc.tile_spreads(hdr, 8, 171.1).max()) == 255 and int(bc.tile_spreads(hdr, 8, 171.8).max()) == 256
    table = {n: bc.plan(bc.prof_case(n))[:2] for n in bc.PROF_CASES}
    assert table["spread_255_t1"] == (bc.FAST, 1) and table["spread_256_t1"] == table["spread_255_t2"] == (bc.GENERIC, None)
    assert table["t256_dm0"] == (bc.FAST, 1) and table["t257_dm0"] == (bc.GENERIC, None)


def test_the_partials_cap_on_the_restated_plan(emu_lib):
    """56 candidates x 512 tiles x 1024 bins x 36 bytes = 1 056 964 608 <= 2^30 < 1 075 838 976 for 57; the emulator build answers
    generic to both"""
    a, b = bc.partials_cap(56), bc.partials_cap(57)
    assert 56 * 512 * 1024 * 36 == 1056964608 <= bc.PART_CAP < 57 * 512 * 1024 * 36 == 1075838976
    assert bc.plan(a) == (bc.FAST, 256, 0) and bc.plan(b) == (bc.GENERIC, None, 0)
    rows = np.zeros(16, np.uint8)
    assert pc.query(emu_lib, a, rows.ctypes.data) == 0 and pc.query(emu_lib, b, rows.ctypes.data) == 0


# ---- the emulator build: the generic kernels on the same cases -------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bc.BURST_CASES))
def test_burst_sums_on_the_emulator(emu_lib, name):
    """documented_maximum: 2.16 x 10^6 rows; measured 4.5 s for the case and its restatement (test_burst_conditions pays them, the
    cache keeps them) and 1.0 s for the emulator's call and the comparison: the twin stays"""
    t = time.time()
    ran = bc.check_burst_case(emu_lib, name, misaligns=(0,) if name == "documented_maximum" else (0, 4))
    print("%s: %.1f s" % (name, time.time() - t))
    assert set(ran) == {bc.GENERIC}


@pytest.mark.parametrize("name", sorted(bc.PROF_CASES))
def test_profile_on_the_emulator(emu_lib, name):
    assert bc.check_prof_case(emu_lib, name) == [bc.GENERIC, bc.GENERIC]


def test_host_and_device_twins_write_the_same_bytes(emu_lib):
    c = bc.prof_case("spread_255_t1")
    out, k, _q = bc.profile_on(emu_lib, c)
    code, msg, out2, k2 = pc.call(emu_lib.frbch_polprof_host, c, c["rows"].ctypes.data)
    assert code == 0 and k2 == k == (0, 0), msg
    for f in out:
        assert out[f].tobytes() == out2[f].tobytes(), f


# ---- rows past a mark: the builder of tests/test_gpu_burst_edges.py's 4 GiB case at marks of 2^20 / 2^21 bytes ---------
def test_the_profile_beyond_the_mark_on_the_emulator(emu_lib):
    br = bg.small("A8")
    assert (br.byte_mark_rows[-1] + 20) * br.row_bytes > 1 << 21
    pc.check_beyond_the_mark(emu_lib, br, bg.mem_for(emu_lib), behind=20, front=50, off_len=40, nbin=16, tfactor=2, kernels=((0, 0, 0), (4, 0, 0)))
