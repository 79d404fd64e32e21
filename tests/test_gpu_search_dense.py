"""GPU tests of the three search stages at every bin, not only at peaks: the dense cases of tests/dense_cases.py
(periodicity search at nharm = 1 and sigma 0.01, where every local maximum of the normalised spectrum is a record that carries
its float bits; single-pulse search with one width at threshold 1e-6, where every window maximum of the quantised series is
one) on the device.  Each case first asserts on the oracle alone that it is dense -- the raw count below 2^20, at least a quarter
of the searched bins of every lit series a record -- then runs the fast form at the 16-byte aligned address and the generic form one
float further on against ONE cached expectation, and asserts `kernel_used` against frbch_psearch_kernel and the documented
plan.  Integers and the float bits of `power` / `sigma` (single pulse) are exact, the doubles sigma / freq_hz of the periodicity
search are held to psearch_oracle.SIGMA_RTOL as everywhere else.  Device buffers are guarded buffers of exactly the documented
size, checksummed behind every call (the callers of tests/psearch_cases.py, accel_cases.py and spsearch_cases.py)."""
import numpy as np
import pytest

from tests import dense_cases as dn

pytestmark = pytest.mark.gpu

FAST, GENERIC = dn.FAST, dn.GENERIC


# ---- periodicity search ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", range(12, 23))
def test_every_bin_of_the_spectrum_at_every_length(hip_lib, L):
    """n = 2^12 .. 2^22, the documented maximum.  15, 16 and 22 are the lengths whose FIRST pass has 8 stages with 16 columns
    (register passes 3 + 3 + 2), 22 the one split (8, 7, 7); ndm alternates between even and odd; nout = n + 5 at the odd L"""
    assert not dn.is_emulator(hip_lib)
    assert dn.forms(hip_lib, 1 << L) == [(False, (FAST, 1 if L <= 13 else 2 if L <= 18 else 3)), (True, (GENERIC, 0))]
    assert {15: (8, 7), 16: (8, 8), 21: (7, 7, 7), 22: (8, 7, 7)}.get(L, dn.stages_of(L)) == dn.stages_of(L)
    assert dn.register_passes(8) == (3, 3, 2) and (dn.stages_of(L)[0] == 8) == (L in (15, 16, 22))
    case = dn.ps_length(L)
    assert case.n == 1 << L and case.y.shape == (dn.PS_GRID[L][0], (1 << L) + (5 if L % 2 else 0))
    dn.ps_hold(hip_lib, case)


@pytest.mark.parametrize("L,B", [(14, 32), (14, 1024), (19, 32), (19, 1024)])
def test_block_lengths(hip_lib, L, B):
    """frbch_post_ps_norm_lds gives a workgroup 8192 / B blocks: 256 and 8; its last workgroup owns the long last block"""
    dn.ps_hold(hip_lib, dn.ps_wblock(L, B))


@pytest.mark.parametrize("L", [12, 15])
def test_kmin_inside_a_block(hip_lib, L):
    """kmin = 100 in block [1, 129): p is 0 below kmin, the level still counts those bins"""
    case = dn.ps_kmin_inside(L)
    assert case.want["k"].min() >= 100 and (case.want["k"] < 129).any()
    dn.ps_hold(hip_lib, case)


@pytest.mark.parametrize("L", [12, 14])
def test_dead_and_constant_partners(hip_lib, L):
    """a NaN series, an Inf series and a constant one, each beside a live one whose whole spectrum is held; they give no record"""
    dn.ps_hold(hip_lib, dn.ps_dead(L), quiet=dn.DEAD_QUIET)


def test_all_five_folds(hip_lib):
    case = dn.ps_all_folds()
    assert case.kmin == 5 and case.nraw > 3 * case.want.size and {1, 2, 4, 8, 16} == set(case.want["h"].tolist())
    dn.ps_hold(hip_lib, case)


@pytest.mark.parametrize("nharm", [1, 2, 4, 8, 16])
def test_fold_edges(hip_lib, nharm):
    """(h, k = h kmin), the first bin of fold h (no left neighbour), in series 0 and 2 and (1, n / 2 - 1), the last bin (no right
    neighbour), in series 1: asserted on the oracle by the case, then the full record lists in both forms"""
    dn.ps_hold(hip_lib, dn.ps_fold_edge(nharm))


# ---- acceleration search --------------------------------------------------------------------------------------------
def test_every_bin_of_every_trial(hip_lib):
    """n = 2^14, three series, trials -A, 0, +A at nharm 1: accel_oracle.resample, then the dense expectation of each plane;
    batch_rows 0 and 4 (one trial -- three series and the zero row -- a batch) give the same bytes, and no record carries
    dm_index 3"""
    case = dn.pa_n14()
    assert case.y.shape == (3, 1 << 14) and case.accs.tolist() == [-dn.ac.A14, 0.0, dn.ac.A14]
    dn.pa_hold(hip_lib, case, batch_rows=(0, 4))


def test_every_bin_of_two_trials_at_three_pass_length(hip_lib):
    """n = 2^19, two series, two trials: three passes on the library's own resampled plane"""
    case = dn.pa_n19()
    assert case.n == 1 << 19 and dn.passes_of(case.n) == 3 and set(np.unique(case.want["acc_index"]).tolist()) == {0, 1}
    dn.pa_hold(hip_lib, case)


# ---- single-pulse search --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", dn.SP_WIDTHS)
@pytest.mark.parametrize("shape", sorted(dn.SP_SHAPES))
def test_every_sample_of_the_quantised_series(hip_lib, shape, w):
    """3 DMs x (2 x 2048 + 5) and 9 DMs x (3 x 2048 + 5) samples, one width a call: 1, 2, 16, 511 and 512 take the LDS kernel,
    520 and 1024 the generic ones (asserted by sp_hold); width 1 exposes the whole quantisation"""
    assert dn.sp_kernel(hip_lib, w) == (w <= 512)
    dn.sp_hold(hip_lib, dn.sp_dense(shape, w))
