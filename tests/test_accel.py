"""Acceleration search of the dedispersed series (frbch_resample_*, frbch_pasearch_*, frbch_pa_group_cands, post.accel_search /
group_accel / psearch_fil(amax=...)): the generic kernels through the TEST-ONLY emulator build against the numpy restatement
tests/accel_oracle.py -- the resampler byte for byte, the records with the integers and the float bits of H exactly -- the
library against itself where two routes must agree, the refusals, the failure walk, and the grouping rules."""
import ctypes as C
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from oracle import post_oracle as po
from tests import accel_cases as ac
from tests import accel_oracle as ao
from tests import psearch_cases as pc
from tests import psearch_oracle as pso
from tests.test_fold_predictor import write_fil
from tests.test_post import HDR


# ---- the index rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1 << 12, 1 << 22])
@pytest.mark.parametrize("qn", [0.5, -0.5])
def test_index_rule_stays_inside_the_series_at_the_edge_of_the_range(n, qn):
    """what include/frbch.h promises for every accepted trial, at the extreme ones: both ends pinned, 0 <= u <= n - 1, steps of
    0, 1 or 2, and |u - t| <= n / 8"""
    u = ao.index_of_q(n, qn / n)
    d = np.diff(u)
    assert u[0] == 0 and u[-1] == n - 1 and u.min() == 0 and u.max() == n - 1
    assert d.min() >= 0 and d.max() <= 2
    assert np.abs(u - np.arange(n)).max() <= n // 8


def test_the_edge_is_exact_and_the_sign_is_the_stated_one():
    e = ac.edge(4096, ac.TSAMP)
    assert ao.q_of(e, ac.TSAMP) * 4096.0 == 0.5 and ao.accepted(e, 4096, ac.TSAMP) and not ao.accepted(ac.just_above(4096, ac.TSAMP), 4096, ac.TSAMP)
    # positive a: u(t) <= t -- the series is re-read EARLIER, a falling frequency is levelled at its value in the middle
    u = ao.index(4096, ac.A12, ac.TSAMP)
    assert np.all(u <= np.arange(4096)) and np.array_equal(ao.index(4096, 0.0, ac.TSAMP), np.arange(4096))


# ---- the resampler alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndm,nout", [(2, 4096), (3, 4096), (3, 5000), (2, 4099)])
def test_resampler_equals_numpy_indexing(emu_lib, ndm, nout):
    y = pc.noise(ndm, nout, 150 + ndm)
    y[:, 4096:] = np.float32(1.0e6)
    e = ac.edge(4096, ac.TSAMP)
    accs = [-e, -ac.A12, 0.0, ac.A12, e]
    info = {}
    got = post.resample(y, ac.TSAMP, accs, lib=emu_lib, info=info)
    assert info == dict(resampler=0) and got.shape == (5, ndm, 4096)
    assert got.tobytes() == ao.resample(y, 4096, ac.TSAMP, accs).tobytes()
    assert got[2].tobytes() == y[:, :4096].tobytes() and float(got.max()) < 1.0e6


# ---- the search against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_emulator_equals_the_oracle(emu_lib, name):
    y, tsamp, accs, kw, want = ac.case(name)
    rc, got, ncand, used, msg = ac.pasearch_host(emu_lib, y, tsamp, accs, **kw)
    assert rc == 0, msg
    assert used == (0, 0, 0) and ncand == want.size
    assert ac.same_records(got, want)
    assert ac.same_groups(post.group_accel(got, 2, 1, lib=emu_lib), ao.group(want, 2, 1))


def test_the_cases_hold_what_they_are_written_for():
    for name in ac.CASES:
        want = ac.case(name)[4]
        assert want.size > 0 and len(set(want["acc_index"].tolist())) == ac.case(name)[2].size, name
    # the NaN: series 1 is dead in the trials whose gather reaches the sample, and alive in the one that skips it
    y, tsamp, accs, kw, want = ac.case("nan_reached_by_some_trials")
    p = ac.nan_position()
    reached = [p in set(ao.index(4096, a, tsamp).tolist()) for a in accs]
    assert reached == [True, True, False]
    alive = [bool(np.any((want["acc_index"] == i) & (want["dm_index"] == 1))) for i in range(3)]
    assert alive == [False, False, True]
    # pairing inside the trial: series 2 of the odd case is searched beside a zero partner in EVERY trial
    y, tsamp, accs, kw, want = ac.case("odd_3dm_2trials")
    for i, a in enumerate(accs):
        alone = pso.search(y[2:3, :4096][:, ao.index(4096, a, tsamp)], tsamp, **kw)
        mine = want[(want["acc_index"] == i) & (want["dm_index"] == 2)]
        assert mine.size == alone.size > 0 and mine["power"].tobytes() == alone["power"].tobytes()
    y, tsamp, accs, kw, want = ac.case("constant_series")
    assert 1 not in want["dm_index"]
    # trial 0 is the search without accelerations
    y, tsamp, accs, kw, want = ac.case("2dm_3trials_4096")
    zero = want[want["acc_index"] == 1]
    plain = pso.search(y, tsamp, **kw)
    assert zero.size == plain.size and all(np.array_equal(zero[f], plain[f]) for f in ("dm_index", "h", "k", "power", "sigma", "freq_hz"))


# ---- the library against itself ----------------------------------------------------------------------------------------
def test_zero_acceleration_equals_psearch_field_for_field(emu_lib):
    y, tsamp, kw, _want, _raw = pc.case("odd_3dm")
    rc, plain, n, _used, msg = pc.psearch_host(emu_lib, y, tsamp, **kw)
    assert rc == 0 and n > 0, msg
    rc, got, ncand, _used, msg = ac.pasearch_host(emu_lib, y, tsamp, [0.0], **kw)
    assert rc == 0 and ncand == n, msg
    for f in ("dm_index", "h", "k", "power", "sigma", "freq_hz"):
        assert got[f].tobytes() == plain[f].tobytes(), f
    assert not got["acc_index"].any() and not got["acc_ms2"].any() and not got["reserved"].any()


def test_records_do_not_depend_on_batch_rows(emu_lib):
    y, tsamp, accs, kw, want = ac.case("odd_3dm_2trials")
    rc, whole, _n, _u, msg = ac.pasearch_host(emu_lib, y, tsamp, accs, batch_rows=0, **kw)
    assert rc == 0, msg
    assert want.size > 0
    for rows in (1, 3, 4, 7, 8):                      # below a trial, a trial without its pad row, one trial, almost two, two
        rc, got, _n, _u, msg = ac.pasearch_host(emu_lib, y, tsamp, accs, batch_rows=rows, **kw)
        assert rc == 0 and got.tobytes() == whole.tobytes(), (rows, msg)
    params = pc.params_of(tsamp, **kw)
    n, rows, nb, sb = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    err = C.create_string_buffer(256)
    for batch_rows, expect in ((0, (8, 1)), (3, (4, 2)), (4, (4, 2)), (8, (8, 1)), (100, (8, 1))):
        assert emu_lib.frbch_pasearch_plan(3, 4096, C.byref(params), 2, batch_rows, C.byref(n), C.byref(rows), C.byref(nb), C.byref(sb),
                                           err, len(err)) == 0, err.value
        assert (n.value, rows.value, nb.value) == (4096,) + expect
        assert sb.value == rows.value * (10 * 4096 + 12) + 4096 * 4 + 2 * 8 + (1 << 20) * 16 + 4
    # the library's own choice: whole trials within 2 GiB of per-row scratch
    assert emu_lib.frbch_pasearch_plan(64, 1 << 18, C.byref(pc.params_of(64e-6)), 33, 0, C.byref(n), C.byref(rows), C.byref(nb),
                                       C.byref(sb), err, len(err)) == 0
    assert rows.value % 64 == 0 and rows.value * (10 * (1 << 18) + 12) <= 2 << 30 < (rows.value + 64) * (10 * (1 << 18) + 12)
    assert nb.value == -(-33 // (rows.value // 64))


FHDR = dict(HDR, tsamp=256e-6)


def test_dedisperse_pasearch_equals_the_two_calls(emu_lib):
    rng = np.random.default_rng(160)
    x = rng.integers(96, 160, size=(4096 + 40, 64)).astype(np.uint8)
    dms = np.ascontiguousarray([0.0, 20.0, 40.0])
    desc = post.fil_desc(FHDR)
    nout = emu_lib.frbch_dedisperse_nout(C.byref(desc), x.shape[0], dms.ctypes.data, 3)
    assert nout >= 4096
    series = np.zeros((3, nout), dtype=np.float32)
    nclip = C.c_uint64(0)
    err = C.create_string_buffer(512)
    assert emu_lib.frbch_dedisperse_host(C.byref(desc), x.ctypes.data, x.shape[0], dms.ctypes.data, 3, 1, 5.0, 0, series.ctypes.data, nout,
                                         C.byref(nclip), err, len(err)) == 0, err.value
    accs = np.ascontiguousarray([-1.0e8, 0.0, 1.0e8])
    rc, want, nwant, used, msg = ac.pasearch_host(emu_lib, series, FHDR["tsamp"], accs, sigma=3.0)
    assert rc == 0 and nwant > 0, msg
    params = pc.params_of(0.0, sigma=3.0)                     # tsamp_s = 0: the file's
    out = np.zeros((3, nout), dtype=np.float32)
    cands = np.zeros(8192, dtype=post.PA_CAND)
    ncand, k, nc = C.c_uint64(0), (C.c_uint32 * 3)(9, 9, 9), C.c_uint64(0)
    rc = emu_lib.frbch_dedisperse_pasearch_host(C.byref(desc), x.ctypes.data, x.shape[0], dms.ctypes.data, 3, 1, 5.0, C.byref(params),
                                                accs.ctypes.data, 3, 0, 0, out.ctypes.data, nout, C.byref(nc), cands.ctypes.data, 8192,
                                                C.byref(ncand), k, err, len(err))
    assert rc == 0, err.value
    assert (k[0], k[1], k[2]) == used and nc.value == nclip.value and ncand.value == nwant
    assert cands[:nwant].tobytes() == want.tobytes() and out.tobytes() == series.tobytes()


# ---- found only with the feature -------------------------------------------------------------------------------------
def test_chirped_sine_is_found_at_its_acceleration(emu_lib):
    """a sine that drifts by 12 bins: the search without accelerations sees it at about 5 sigma, trial a0 at over 30.  The seed
    is one for which the ORACLE alone meets the factor of 3 -- asserted first, as a condition on the input"""
    y = ac.chirp()
    want = ao.search(y, ac.CHIRP_TSAMP, ac.CHIRP_ACCS, sigma=3.0)
    ac.chirp_checks(ao.group(want, 2, 1), want)
    got = post.accel_search(y, ac.CHIRP_TSAMP, ac.CHIRP_ACCS, sigma=3.0, lib=emu_lib)
    assert ac.same_records(got, want)
    ac.chirp_checks(post.group_accel(got, 2, 1, lib=emu_lib), got)
    # what the search without accelerations makes of it: the records of trial 0, and nothing near the factor
    plain = post.periodicity_search(y, ac.CHIRP_TSAMP, sigma=3.0, lib=emu_lib)
    assert plain["sigma"].tobytes() == got[got["acc_index"] == 3]["sigma"].tobytes()


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals(emu_lib):
    y = pc.noise(2, 4096, 170)
    ok = [-ac.A12, 0.0, ac.A12]
    for accs, word in (([0.0, -1.0], "ascending"), ([0.0, 0.0], "ascending"), ([1.0, 2.0, 2.0], "ascending"),
                       ([0.0, float("nan")], "finite"), ([float("-inf"), 0.0], "finite"), ([0.0, float("inf")], "finite"),
                       ([0.0, ac.just_above(4096, ac.TSAMP)], "largest"), ([-ac.just_above(4096, ac.TSAMP), 0.0], "largest")):
        rc, _g, _n, _u, msg = ac.pasearch_host(emu_lib, y, ac.TSAMP, accs)
        assert rc == _lib.E_ARG and word in msg, (accs, msg)
    rc, _g, _n, _u, msg = ac.pasearch_host(emu_lib, y, ac.TSAMP, [0.0, ac.just_above(4096, ac.TSAMP)])
    assert "the largest is 73191518.1 m/s^2" in msg                                  # c / (n tsamp): the largest acceptable |a| is named
    rc, _g, _n, _u, msg = ac.pasearch_host(emu_lib, y, ac.TSAMP, [ac.edge(4096, ac.TSAMP)])
    assert rc == 0, msg
    for nacc in (0, 1025):
        rc, _g, _n, _u, msg = ac.pasearch_host(emu_lib, y, ac.TSAMP, np.arange(1025, dtype=np.float64), nacc=nacc)
        assert rc == _lib.E_ARG and "1..1024" in msg
    p = pc.params_of(ac.TSAMP)
    p.size -= 8
    a = np.ascontiguousarray(ok)
    n = C.c_uint64(0)
    err = C.create_string_buffer(256)
    assert emu_lib.frbch_pasearch_host(y.ctypes.data, 2, 4096, C.byref(p), a.ctypes.data, 3, 0, 0, None, 0, C.byref(n), None, err,
                                       len(err)) == _lib.E_ARG and b"size" in err.value
    assert emu_lib.frbch_pasearch_plan(2, 4096, C.byref(p), 3, 0, None, None, None, None, err, len(err)) == _lib.E_ARG
    p = pc.params_of(ac.TSAMP)
    assert emu_lib.frbch_pasearch_host(y.ctypes.data, 65535, 4096, C.byref(p), a.ctypes.data, 3, 0, 0, None, 0, C.byref(n), None, err,
                                       len(err)) == _lib.E_ARG and b"65534" in err.value
    out = np.zeros((3, 2, 4096), dtype=np.float32)
    for bad_n in (2048, 5000, 8192):
        assert emu_lib.frbch_resample_host(y.ctypes.data, 2, 4096, bad_n, ac.TSAMP, a.ctypes.data, 3, 0, out.ctypes.data, None, err,
                                           len(err)) == _lib.E_ARG
    with pytest.raises(post.InputError):
        post.accel_search(y, ac.TSAMP, [1.0, 0.0], lib=emu_lib)
    with pytest.raises(post.InputError):
        post.resample(y, ac.TSAMP, [0.0, float("nan")], lib=emu_lib)
    used = emu_lib.frbch_resample_kernel(y.ctypes.data, 4096, out.ctypes.data)
    assert used == 0                                                # the emulator has no fast form


def test_capacity_of_the_record_list(emu_lib):
    y, tsamp, accs, kw, want = ac.case("2dm_3trials_4096")
    rc, got, ncand, _used, msg = ac.pasearch_host(emu_lib, y, tsamp, accs, cap=5, **kw)
    assert rc == _lib.E_CAPACITY and ncand == want.size > 5 and "candidates" in msg and ac.same_records(got, want[:5])
    assert ac.same_records(post.accel_search(y, tsamp, accs, lib=emu_lib, cap=2, **kw), want)        # grows past cap


def test_raw_peak_overflow_is_an_error(emu_lib):
    """sigma 0.01 (T_1 = 0.70: a third of all noise bins are raw peaks) on 8 x 2^16 noise samples gives some 2^17.4 raw peaks a
    trial: seven trials in one batch overflow the list of 2^20.  (tests/test_gpu_accel.py also runs them one trial to a batch,
    where they fit: the one thing that may depend on batch_rows.)"""
    y = pc.noise(8, 1 << 16, 171)
    accs = [-3.0e6, -2.0e6, -1.0e6, 0.0, 1.0e6, 2.0e6, 3.0e6]
    rc, got, ncand, _used, msg = ac.pasearch_host(emu_lib, y, 64e-6, accs, sigma=0.01, cap=0)
    assert rc == _lib.E_CAPACITY and "threshold too low" in msg and "per batch" in msg and ncand == 0


# ---- the failure walk ------------------------------------------------------------------------------------------------
def test_failure_walk(emu_lib):
    """every fallible device-layer call of frbch_pasearch_host fails once, n = 1, 2, ... until the call succeeds: a negative code
    with a message, no block or stream left behind, the inputs unchanged, and the oracle's records from a plain call afterwards"""
    from tests.test_post_failures import Entry
    emu_lib.frbch_test_emu_fail_at.argtypes, emu_lib.frbch_test_emu_fail_at.restype = [C.c_long], None
    emu_lib.frbch_test_emu_live.argtypes, emu_lib.frbch_test_emu_live.restype = [], C.c_uint64
    y, tsamp, accs, kw, want = ac.case("odd_3dm_2trials")
    e = Entry(emu_lib, "frbch_pasearch_host")
    cap = 4096
    ncand, used = C.c_uint64(0), (C.c_uint32 * 3)(0, 0, 0)
    cands = e.out(cap * post.PA_CAND.itemsize)
    e.args = [e.inp(y), 3, y.shape[1], e.hold(pc.params_of(tsamp, **kw)), e.inp(accs), accs.size, 4, 0, cands, cap, e.hold(ncand), used]

    def records():
        return np.frombuffer(e.out_bytes()[0], dtype=post.PA_CAND)[: ncand.value]

    codes = []
    for n in range(1, 200):
        code, msg, before, after = e.call(n)
        codes.append(code)
        assert after == before, (n, "device blocks / streams alive: %#x before, %#x after" % (before, after))
        e.unchanged()
        if code == 0:
            break
        assert code < 0 and msg, n
        code, msg, before, after = e.call(0)
        assert code == 0 and after == before and ac.same_records(records(), want), (n, msg)
        e.unchanged()
    # two batches: the allocations, two uploads, and per batch a memset, the launches, two copies and two syncs
    assert codes[-1] == 0 and len(codes) > 30 and all(c < 0 for c in codes[:-1])
    assert ac.same_records(records(), want)


# ---- grouping --------------------------------------------------------------------------------------------------------
def rec_of(rows):
    out = np.zeros(len(rows), dtype=post.PA_CAND)
    for i, (dm, acc, h, k, sigma) in enumerate(rows):
        out[i] = (dm, acc, h, k, 30.0, 0, sigma, 0.0, 1000.0 * acc)
    return out


def test_grouping_rules(emu_lib):
    rec = rec_of([(0, 0, 1, 100, 7.0),        # 0
                  (0, 1, 1, 101, 8.0),        # 1: one trial and one bin from 0 -> joined
                  (0, 2, 1, 102, 9.0),        # 2: two trials from 0, linked only through 1
                  (0, 4, 1, 102, 6.0),        # 3: two trials from 2: alone with acc_gap 1
                  (4, 1, 1, 101, 6.5),        # 4: three DMs from 5 and four from 1: alone with dm_gap 2
                  (1, 2, 2, 205, 5.0),        # 5: 102.5 bins: within 1.5 of 1 and 2, one DM away -> joined
                  (1, 2, 1, 104, 5.5)])       # 6: 2 bins from 2, 1.5 from 5 exactly -> joined through 5
    got = post.group_accel(rec, 2, 1, lib=emu_lib)
    assert ac.same_groups(got, ao.group(rec, 2, 1))
    assert [(int(g["best"]["k"]), int(g["nmember"]), int(g["dm_index_lo"]), int(g["dm_index_hi"]), int(g["acc_index_lo"]),
             int(g["acc_index_hi"])) for g in got] == [(102, 5, 0, 1, 0, 2), (101, 1, 4, 4, 1, 1), (102, 1, 0, 0, 4, 4)]
    assert post.group_accel(rec, 2, 2, lib=emu_lib)["nmember"].tolist() == [6, 1]       # record 3 joins through record 2
    assert post.group_accel(rec, 3, 1, lib=emu_lib)["nmember"].tolist() == [6, 1]       # record 4 joins through record 5
    assert post.group_accel(rec[:0], 2, 1, lib=emu_lib).size == 0
    for gaps in ((0, 1), (17, 1), (2, 0), (2, 17)):
        with pytest.raises(post.InputError):
            post.group_accel(rec, *gaps, lib=emu_lib)
    bad = rec.copy()
    bad["h"][0] = 3
    with pytest.raises(post.InputError):
        post.group_accel(bad, 2, 1, lib=emu_lib)


def test_every_tie_rule(emu_lib):
    # best of a group at equal sigma: the smaller h, then the lower dm_index, then the lower acc_index, then the smaller k
    for rows, best in (([(1, 1, 2, 200, 7.0), (1, 1, 1, 100, 7.0)], 1), ([(1, 1, 1, 100, 7.0), (0, 1, 1, 100, 7.0)], 1),
                       ([(1, 1, 1, 100, 7.0), (1, 0, 1, 100, 7.0)], 1), ([(1, 1, 1, 101, 7.0), (1, 1, 1, 100, 7.0)], 1)):
        rec = rec_of(rows)
        got = post.group_accel(rec, 2, 1, lib=emu_lib)
        assert got.size == 1 and got[0]["best"].tobytes() == rec[best].tobytes() and ac.same_groups(got, ao.group(rec, 2, 1)), rows
    # order of the groups at equal sigma: f ascending, then dm_index, then acc_index, then h
    rec = rec_of([(9, 9, 2, 1000, 7.0), (9, 9, 1, 500, 7.0), (9, 5, 1, 500, 7.0), (4, 9, 1, 500, 7.0), (12, 12, 1, 300, 7.0),
                  (12, 12, 1, 700, 8.0)])
    got = post.group_accel(rec, 1, 1, lib=emu_lib)
    assert ac.same_groups(got, ao.group(rec, 1, 1))
    assert [(int(g["best"]["dm_index"]), int(g["best"]["acc_index"]), int(g["best"]["h"]), int(g["best"]["k"])) for g in got] == \
        [(12, 12, 1, 700), (12, 12, 1, 300), (4, 9, 1, 500), (9, 5, 1, 500), (9, 9, 1, 500)]


# ---- the Python layer ------------------------------------------------------------------------------------------------
def test_acc_list_and_accel_step():
    assert post.acc_list(0.0, 0.0).tolist() == [0.0] and post.acc_list(10.0, 4.0).tolist() == [-8.0, -4.0, 0.0, 4.0, 8.0]
    assert post.acc_list(8.0, 4.0).tolist() == [-8.0, -4.0, 0.0, 4.0, 8.0] and post.acc_list(3.0, 4.0).tolist() == [0.0]
    assert 0.0 in post.acc_list(1.0, 0.3).tolist() and np.all(np.diff(post.acc_list(1.0, 0.3)) > 0)
    for bad in ((-1.0, 1.0), (1.0, 0.0), (float("nan"), 1.0), (1000.0, 1.0)):
        with pytest.raises(post.InputError):
            post.acc_list(*bad)
    # one bin of drift: 2 nu q n^2 = 1 with nu = f tsamp and q = a tsamp / (2 c)
    a = post.accel_step(1 << 14, 1e-3, 37.3)
    assert abs(2.0 * (37.3 * 1e-3) * ao.q_of(a, 1e-3) * (1 << 14) ** 2 - 1.0) < 1e-12
    assert post.accel_step(1 << 14, 1e-3, 37.3, 2.0) == 2.0 * a


def chirped_train_rows(a, seed=3, amp=14, nrows=8192 + 40, f0=1.0 / 0.0334, dm=40.0):
    """noise 96 .. 159 and a pulse of one sample in every channel at the times where f0 (t - (a / 2 c) t^2) passes an integer + 1/4
    (t in seconds from the start: the frequency falls), dispersed at `dm`"""
    rng = np.random.default_rng(seed)
    x = rng.integers(96, 160, size=(nrows, FHDR["nchans"])).astype(np.int64)
    dly = po.delays_seconds(FHDR["fch1"], FHDR["foff"], FHDR["nchans"], dm)
    t = np.arange(nrows * 8, dtype=np.float64) * (FHDR["tsamp"] / 8.0)
    turns = f0 * (t - a / (2.0 * ao.C_LIGHT) * t * t) - 0.25
    at = t[1:][np.floor(turns[1:]) > np.floor(turns[:-1])]
    for c in range(FHDR["nchans"]):
        i = np.round((at + dly[c]) / FHDR["tsamp"]).astype(np.int64)
        np.add.at(x[:, c], i[i < nrows], amp)
    return x.astype(np.uint8)


TRAIN_A = 2.0e6       # m/s^2: 29.94 Hz over 2.1 s falls by 0.42 Hz, nearly a bin (0.477 Hz); its 16th harmonic by 14


def test_psearch_fil_with_accelerations(emu_lib, tmp_path, monkeypatch, capsys):
    fil = str(tmp_path / "chirp.fil")
    write_fil(fil, chirped_train_rows(TRAIN_A)[:, None, :], FHDR, 1)
    monkeypatch.setattr(_lib, "load", lambda path=None: emu_lib)
    base = fil.replace(".fil", "")
    # without --amax: the files of the search without accelerations, byte for byte (and no acceleration column)
    assert post.main(["psearch", fil, "--dm", "30", "--dm2", "50", "--dmstep", "10"]) == 0
    plain_txt = open(base + "_psearch.txt").read()
    plain = np.load(base + "_psearch.npz")
    assert plain_txt.splitlines()[0] == post.PS_HEADER and "accs" not in plain.files and plain["candidates"].dtype == post.PS_GROUP
    _files, g0 = post.psearch_fil(fil, 30.0, dm2=50.0, dmstep=10.0, lib=emu_lib, amax=0.0)
    assert open(base + "_psearch.txt").read() == plain_txt and g0.tobytes() == plain["candidates"].tobytes()
    capsys.readouterr()
    assert post.main(["psearch", fil, "--dm", "30", "--dm2", "50", "--dmstep", "10", "--amax", "4e6", "--astep", "1e6", "--fold-best", "1"]) == 0
    out = capsys.readouterr().out
    assert "wrote %s_psearch_cand0.ar" % base in out
    back = np.load(base + "_psearch.npz")
    assert back["accs"].tolist() == [k * 1e6 for k in range(-4, 5)] and back["candidates"].dtype == post.PA_GROUP
    lines = open(base + "_psearch.txt").read().splitlines()
    assert lines[0] == post.PA_HEADER and len(lines) == 1 + back["candidates"].size
    best = back["candidates"][0]["best"]
    assert float(best["acc_ms2"]) == TRAIN_A and int(best["dm_index"]) == 1 and int(best["h"]) > 1
    assert float(best["sigma"]) > float(plain["candidates"][0]["best"]["sigma"])
    # freq_hz is the frequency in the middle of the searched span
    n, tsamp = int(back["nfft"]), FHDR["tsamp"]
    mid = (1.0 / 0.0334) * (1.0 - TRAIN_A * (n * tsamp / 2.0) / ao.C_LIGHT)
    m = int(round(float(best["freq_hz"]) / mid))          # (harmonically related candidates are not merged: the ladder of 2 f may lead)
    assert m in (1, 2) and abs(float(best["freq_hz"]) - m * mid) <= 1.0 / (n * tsamp) / int(best["h"])
    first = lines[1].split()
    assert float(first[8]) == TRAIN_A and float(first[2]) == 40.0
    # the records are the oracle's on the dedispersed plane
    x = np.fromfile(fil, dtype=np.uint8)[-(8192 + 40) * 64:].reshape(8192 + 40, 64)
    y, _nclip = po.dedisperse(x, fch1=FHDR["fch1"], foff=FHDR["foff"], tsamp=tsamp, dms=[30.0, 40.0, 50.0], zerodm=True, clip=5.0)
    assert ac.same_records(back["records"], ao.search(y, tsamp, back["accs"], sigma=6.0, nharm=16, flo=0.5, wblock=128))
    # the fold: F1 = -F0 a / c at the middle of the span, and the pulse stays in one region of phase
    prof, hits, meta = post.read_archive(base + "_psearch_cand0.ar")
    assert meta["f0"] == float(best["freq_hz"]) and meta["f1"] == -meta["f0"] * TRAIN_A / ao.C_LIGHT and meta["dm"] == 40.0
    assert meta["pepoch"] == FHDR["tstart"] + (n * tsamp / 2.0) / 86400.0
    assert os.path.getsize(base + "_psearch_cand0.png") > 0
