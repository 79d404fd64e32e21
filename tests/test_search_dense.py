"""The dense cases of tests/dense_cases.py through the TEST-ONLY emulator build (generic kernels): the twins of
tests/test_gpu_search_dense.py that run without a GPU, and the tests of the case module itself -- that `sift` drops nothing
at h = 1, that the vectorised sigma is psearch_oracle.sigma_of, that the comparison says what differs, and that the plan the
device module asserts is the documented one."""
import numpy as np
import pytest

from tests import dense_cases as dn
from tests import psearch_cases as pc
from tests import psearch_oracle as pso
from tests import spsearch_oracle as so


# ---- the case module ------------------------------------------------------------------------------------------------
def test_step_8_drops_nothing_at_one_harmonic():
    """the claim ps_dense rests on, with the oracle's own quadratic `sift` at n = 4096: the raw peaks ARE the records"""
    case = dn.ps_length(12)
    raw = [(int(r["dm_index"]), 1, int(r["k"]), r["power"]) for r in case.want]
    assert np.diff(case.want["k"].astype(np.int64))[np.diff(case.want["dm_index"].astype(np.int64)) == 0].min() == 2
    sifted = pso.sift(raw, case.n, case.tsamp)
    assert sifted.size == len(raw) and pc.same_records(sifted, case.want) and not dn.ps_differences(sifted, case.want)
    full = pso.search(case.y, case.tsamp, sigma=dn.SIGMA, nharm=1)
    assert not dn.ps_differences(full, case.want)
    assert abs(float(pso.thresholds(dn.SIGMA)[0]) - 0.7011579) < 1e-7


def test_vector_sigma_is_the_oracles():
    rng = np.random.default_rng(5)
    H = np.concatenate([np.float32(0.7011579) + rng.exponential(1.0, 200).astype(np.float32), rng.uniform(20.0, 3000.0, 50).astype(np.float32),
                        np.array([0.7011579, 1.0, 449.0, 451.0, 2.3e4, 3.0e38, np.inf], dtype=np.float32)])
    got = dn.sigma_h1(H)
    want = np.array([pso.sigma_of(1, h) for h in H])
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= 1e-12 * want)
    assert want.min() < 0.011 and want.max() > 1e18                     # both branches of log_tail, and the clamp at FLT_MAX


def test_the_comparison_says_what_differs():
    want = dn.ps_length(12).want
    assert dn.ps_differences(want.copy(), want) == ""
    got = want.copy()
    got["power"][7] = np.nextafter(got["power"][7], np.float32(9.0))
    got["sigma"][9] *= 1.0 + 1e-8
    text = dn.ps_differences(np.delete(got, 3), want)
    r = want[3]
    assert "1 missing, 0 extra, 2 of the %d common ones differ" % (want.size - 1) in text and "power in 1" in text and "sigma beyond" in text
    assert "first at (dm, h, k) = (%d, 1, %d)" % (r["dm_index"], r["k"]) in text
    extra = np.insert(want, 5, want[5])
    extra["k"][5] -= 1
    text = dn.ps_differences(extra, want)
    assert "0 missing, 1 extra" in text and "(dm, h, k) = (0, 1, %d)" % extra["k"][5] in text
    assert "out of output order" in dn.ps_differences(want[::-1].copy(), want)
    sp = dn.sp_dense("3dm_2tiles_5", 16).want
    got = sp.copy()
    got["sigma"][4] = np.nextafter(got["sigma"][4], np.float32(99.0))
    text = dn.sp_differences(got, sp)
    assert "sigma in 1" in text and "(dm, w, t) = (0, 16, %d)" % (int(sp["sample"][4]) - 8) in text
    pa = dn.pa_n14().want
    got = pa[pa["acc_index"] != 1]
    text = dn.pa_differences(got, pa)
    first = pa[pa["acc_index"] == 1][0]
    assert "%d missing" % (pa.size - got.size) in text and "(acc, dm, h, k) = (1, 0, 1, %d)" % first["k"] in text


def test_the_plan_the_device_module_asserts():
    """passes of at most 2^13 values, 9 stages a pass with 16 columns; the first pass takes the larger
    share.  Eight stages in a FIRST pass with 16 columns -- register passes 3 + 3 + 2 -- occur at L = 15, 16 and 22 only"""
    assert [dn.passes_of(1 << L) for L in range(12, 23)] == [1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3]
    assert {L: dn.stages_of(L) for L in (13, 14, 15, 16, 18, 19, 20, 21, 22)} == {
        13: (13,), 14: (7, 7), 15: (8, 7), 16: (8, 8), 18: (9, 9), 19: (7, 6, 6), 20: (7, 7, 6), 21: (7, 7, 7), 22: (8, 7, 7)}
    for L in range(12, 23):
        assert sum(dn.stages_of(L)) == L and len(dn.stages_of(L)) == dn.passes_of(1 << L)
        assert L <= 13 or max(dn.stages_of(L)) <= 9
    assert [L for L in range(14, 23) if dn.stages_of(L)[0] == 8] == [15, 16, 22]
    assert dn.register_passes(8) == (3, 3, 2) and dn.register_passes(7) == (3, 2, 2) and dn.register_passes(9) == (3, 3, 3)
    assert dn.register_passes(6) == (3, 3) and dn.register_passes(13) == (3, 3, 3, 2, 2)
    # ndm alternates, and every pass structure meets an odd ndm
    assert all(dn.PS_GRID[L][0] % 2 != dn.PS_GRID[L + 1][0] % 2 for L in range(12, 20))
    assert {dn.passes_of(1 << L) for L in dn.PS_GRID if dn.PS_GRID[L][0] % 2} == {1, 2, 3} and sorted(dn.PS_GRID) == list(range(12, 23))


def test_single_pulse_step_5_drops_nothing_at_width_1():
    """sp_dense runs the quadratic `sift` on raw lists below SIFT_BELOW only; width 1 has the longest lists and the plainest
    argument (|c - c'| <= 0 never holds between two samples): here the sift itself, on one DM"""
    case = dn.sp_dense("3dm_2tiles_5", 1)
    _y, q, _dead = dn.sp_series("3dm_2tiles_5")
    raw = so.raw_peaks(q[1], [1], dn.THR)
    assert len(raw) > dn.SIFT_BELOW and len(so.sift(raw)) == len(raw) == int((case.want["dm_index"] == 1).sum())
    assert int((q[1] >= 1).sum()) == len(raw)                          # every sample with q >= 1


# ---- periodicity search ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [12, 13, 14, 15, 16, 17, 18])
def test_every_bin_of_the_spectrum(emu_lib, L):
    dn.ps_hold(emu_lib, dn.ps_length(L), aligned_only=L >= 15)


@pytest.mark.parametrize("B", [32, 1024])
def test_block_lengths(emu_lib, B):
    dn.ps_hold(emu_lib, dn.ps_wblock(14, B))


@pytest.mark.parametrize("L", [12, 15])
def test_kmin_inside_a_block(emu_lib, L):
    case = dn.ps_kmin_inside(L)
    assert case.want["k"].min() >= 100 and (case.want["k"] < 129).any()
    dn.ps_hold(emu_lib, case, aligned_only=L >= 15)


@pytest.mark.parametrize("L", [12, 14])
def test_dead_and_constant_partners(emu_lib, L):
    dn.ps_hold(emu_lib, dn.ps_dead(L), quiet=dn.DEAD_QUIET)


def test_all_five_folds(emu_lib):
    case = dn.ps_all_folds()
    assert case.kmin == 5 and case.nraw > 3 * case.want.size and {1, 2, 4, 8, 16} == set(case.want["h"].tolist())
    dn.ps_hold(emu_lib, case)


@pytest.mark.parametrize("nharm", [1, 2, 4, 8, 16])
def test_fold_edges(emu_lib, nharm):
    dn.ps_hold(emu_lib, dn.ps_fold_edge(nharm))


# ---- acceleration search --------------------------------------------------------------------------------------------
def test_every_bin_of_every_trial(emu_lib):
    """batch_rows 4: one trial (three series and the zero row) a batch"""
    dn.pa_hold(emu_lib, dn.pa_n14(), batch_rows=(0, 4))


# ---- single-pulse search --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", dn.SP_WIDTHS)
@pytest.mark.parametrize("shape", sorted(dn.SP_SHAPES))
def test_every_sample_of_the_quantised_series(emu_lib, shape, w):
    dn.sp_hold(emu_lib, dn.sp_dense(shape, w))
