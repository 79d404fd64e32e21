"""GPU tests of the acceleration search (frbch_resample_*, frbch_pasearch_*, frbch_dedisperse_pasearch_host): the fast
resampler -- the window of a tile staged through the LDS -- and the generic one it falls back to, byte for byte against numpy
indexing and against each other; the search against the numpy restatement tests/accel_oracle.py record for record (the
integers and the float bits of H exactly, sigma and freq_hz to psearch_oracle.SIGMA_RTOL); the library against itself where two
routes must agree.  Device inputs are guarded buffers of exactly ndm * nout floats, checksummed behind every call."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import accel_cases as ac
from tests import accel_oracle as ao
from tests import post_cases as poc
from tests import psearch_cases as pc
from tests.hipmem import GuardedBuffer

pytestmark = pytest.mark.gpu

FAST, GENERIC = 1, 0


def passes_of(n):
    return 1 if n <= 1 << 13 else 2 if n <= 1 << 18 else 3


device_search = ac.device_search          # (shared with tests/test_gpu_search_dense.py and the emulator twins)


def device_resample(lib, y, n, tsamp, accs, misalign=False):
    """frbch_resample_device -> ([nacc][ndm][n], form); the output buffer is guarded too"""
    accs = np.ascontiguousarray(accs, dtype=np.float64)
    buf, ptr = ac.held(lib, y, misalign)
    out = GuardedBuffer(accs.size * y.shape[0] * n * 4)
    form = lib.frbch_resample_kernel(ptr, y.shape[1], out.ptr)
    used = (C.c_uint32 * 1)(99)
    err = C.create_string_buffer(512)
    rc = lib.frbch_resample_device(ptr, y.shape[0], y.shape[1], n, tsamp, accs.ctypes.data, accs.size, 0, out.ptr, used, err, len(err))
    assert rc == 0, err.value
    buf.check(contents=True)
    out.check()
    got = out.to_numpy(np.float32, accs.size * y.shape[0] * n).reshape(accs.size, y.shape[0], n)
    buf.free()
    out.free()
    assert used[0] == form
    return got, used[0]


# ---- the resampler alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndm,nout,misalign,form", [(2, 4096, False, FAST), (3, 4096, False, FAST), (3, 5000, False, FAST),
                                                    (2, 4096, True, GENERIC), (3, 4099, False, GENERIC), (3, 5001, True, GENERIC)])
def test_resampler_equals_numpy_indexing(hip_lib, ndm, nout, misalign, form):
    """n = 4096: four tiles of the fast form a row; trials {-A, 0, +A} and q n = +-0.5 exactly; 1e6 beyond n; a misaligned
    d_series and an odd nout take the generic form"""
    y = pc.noise(ndm, nout, 150 + ndm)
    y[:, 4096:] = np.float32(1.0e6)
    e = ac.edge(4096, ac.TSAMP)
    accs = [-e, -ac.A12, 0.0, ac.A12, e]
    got, used = device_resample(hip_lib, y, 4096, ac.TSAMP, accs, misalign)
    assert used == form
    assert got.tobytes() == ao.resample(y, 4096, ac.TSAMP, accs).tobytes()


def test_fast_resampler_equals_the_generic_one_at_two_pass_length(hip_lib):
    y = pc.noise(3, (1 << 14) + 4, 155)
    e = ac.edge(1 << 14, 64e-6)
    accs = [-e, -ac.A14, ac.A14, e]
    fast, used = device_resample(hip_lib, y, 1 << 14, 64e-6, accs)
    assert used == FAST
    generic, used = device_resample(hip_lib, y, 1 << 14, 64e-6, accs, misalign=True)
    assert used == GENERIC and fast.tobytes() == generic.tobytes()
    assert fast.tobytes() == ao.resample(y, 1 << 14, 64e-6, accs).tobytes()


# ---- the search against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_device_equals_the_oracle(hip_lib, name):
    y, tsamp, accs, kw, want = ac.case(name)
    n = 4096 if y.shape[1] < 8192 else 1 << 14
    got, used = device_search(hip_lib, y, tsamp, accs, **kw)
    assert used == (FAST if y.shape[1] % 4 == 0 else GENERIC, FAST, passes_of(n)) and ac.same_records(got, want)
    got, used = device_search(hip_lib, y, tsamp, accs, misalign=True, **kw)
    assert used == (GENERIC, FAST, passes_of(n)) and ac.same_records(got, want)       # the resampled plane is the library's: aligned


@functools.lru_cache(maxsize=None)
def three_pass_case():
    tsamp = 64e-6
    y = pc.signals(2, (1 << 19) + 4, 181, tsamp)
    y.setflags(write=False)
    accs = np.array([0.0, 2.0e4])                       # n tsamp = 33.6 s: the 37 Hz sine moves by a tenth of a bin
    return y, tsamp, accs, ao.search(y, tsamp, accs, sigma=4.0)


def test_three_pass_length(hip_lib):
    y, tsamp, accs, want = three_pass_case()
    assert want.size > 0 and set(want["acc_index"].tolist()) == {0, 1}
    got, used = device_search(hip_lib, y, tsamp, accs, sigma=4.0)
    assert used == (FAST, FAST, 3) and ac.same_records(got, want)


# ---- the library against itself --------------------------------------------------------------------------------------
def test_zero_acceleration_equals_psearch_field_for_field(hip_lib):
    y, tsamp, kw, _want, _raw = pc.case("odd_3dm")
    rc, plain, n, _used, msg = pc.psearch_host(hip_lib, y, tsamp, **kw)
    assert rc == 0 and n > 0, msg
    rc, got, ncand, used, msg = ac.pasearch_host(hip_lib, y, tsamp, [0.0], **kw)
    assert rc == 0 and ncand == n and used == (FAST, FAST, 1), msg
    for f in ("dm_index", "h", "k", "power", "sigma", "freq_hz"):
        assert got[f].tobytes() == plain[f].tobytes(), f


def test_records_do_not_depend_on_batch_rows(hip_lib):
    y, tsamp, accs, kw, want = ac.case("1dm_5trials")
    whole, _used = device_search(hip_lib, y, tsamp, accs, batch_rows=0, **kw)
    assert ac.same_records(whole, want)
    for rows in (1, 2, 5, 10):                          # ndm = 1: a trial is two rows; one, one, two and five trials a batch
        got, _used = device_search(hip_lib, y, tsamp, accs, batch_rows=rows, **kw)
        assert got.tobytes() == whole.tobytes(), rows
    y, tsamp, accs, kw, want = ac.case("odd_3dm_2trials")
    whole, _used = device_search(hip_lib, y, tsamp, accs, **kw)
    got, _used = device_search(hip_lib, y, tsamp, accs, batch_rows=3, **kw)          # batch_rows = ndm
    assert got.tobytes() == whole.tobytes() and ac.same_records(got, want)


def test_raw_peak_overflow_depends_on_the_batch_and_on_nothing_else(hip_lib):
    y = pc.noise(8, 1 << 16, 171)
    accs = [-3.0e6, -2.0e6, -1.0e6, 0.0, 1.0e6, 2.0e6, 3.0e6]
    rc, got, ncand, _used, msg = ac.pasearch_host(hip_lib, y, 64e-6, accs, sigma=0.01, cap=0)
    assert rc == _lib.E_CAPACITY and "threshold too low" in msg and "per batch" in msg and ncand == 0
    rc, got, ncand, _used, msg = ac.pasearch_host(hip_lib, y, 64e-6, accs, sigma=0.01, cap=0, batch_rows=8)
    assert rc == _lib.E_CAPACITY and "candidates" in msg and ncand > 100000      # one trial a batch: the raw peaks fit


def test_dedisperse_pasearch_equals_the_two_calls(hip_lib):
    hdr = poc.make_hdr(1024)
    x = poc.make_rows(20000, 2, 1024, 8, seed=21)
    dms = [40.0 + 1.5 * i for i in range(5)]
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    nout = poc.dedisp_nout(hip_lib, hdr, x, 1, dms)
    series, nclip = poc.dedisp_host(hip_lib, hdr, x, 1, dms, True, 5.0, nout)
    accs = np.ascontiguousarray([-1.0e6, 0.0, 1.0e6])
    rc, want, nwant, used, msg = ac.pasearch_host(hip_lib, series, hdr["tsamp"], accs, sigma=3.0)
    assert rc == 0 and nwant > 0 and used[1:] == (FAST, 2), msg
    params = pc.params_of(0.0, sigma=3.0)                     # tsamp_s = 0: the file's
    out = np.zeros((5, nout), dtype=np.float32)
    cands = np.zeros(16384, dtype=post.PA_CAND)
    ncand, k, nc = C.c_uint64(0), (C.c_uint32 * 3)(9, 9, 9), C.c_uint64(0)
    err = C.create_string_buffer(512)
    rc = hip_lib.frbch_dedisperse_pasearch_host(C.byref(poc.desc_of(hdr, x, 1)), x.ctypes.data, x.shape[0], dm_arr.ctypes.data, 5, 1, 5.0,
                                                C.byref(params), accs.ctypes.data, 3, 0, 0, out.ctypes.data, nout, C.byref(nc),
                                                cands.ctypes.data, 16384, C.byref(ncand), k, err, len(err))
    assert rc == 0, err.value
    assert (k[0], k[1], k[2]) == used and nc.value == nclip and ncand.value == nwant
    assert cands[:nwant].tobytes() == want.tobytes() and out.tobytes() == series.tobytes()
    assert ac.same_records(want, ao.search(series, hdr["tsamp"], accs, sigma=3.0))


# ---- found only with the feature -------------------------------------------------------------------------------------
def test_chirped_sine_is_found_at_its_acceleration(hip_lib):
    """tests/test_accel.py has the same test on the emulator; the oracle alone meets the factor for this seed (asserted first)"""
    y = ac.chirp()
    want = ao.search(y, ac.CHIRP_TSAMP, ac.CHIRP_ACCS, sigma=3.0)
    ac.chirp_checks(ao.group(want, 2, 1), want)
    info = {}
    got = post.accel_search(y, ac.CHIRP_TSAMP, ac.CHIRP_ACCS, sigma=3.0, lib=hip_lib, info=info)
    assert info == dict(resampler=FAST, kernel_used=FAST, passes=2) and ac.same_records(got, want)
    ac.chirp_checks(post.group_accel(got, 2, 1, lib=hip_lib), got)


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_chirped_pulse_train_end_to_end(hip_lib, tmp_path, capsys):
    """the chirped pulse train of tests/test_accel.py (29.94 Hz falling by 0.42 Hz over 2.1 s, DM 40, 8-bit noise) through
    `post psearch --amax .. --fold-best 1`; the same command without --amax writes what the search without accelerations
    writes"""
    from tests import test_accel as ta
    from tests.test_fold_predictor import write_fil
    fil = str(tmp_path / "chirp.fil")
    write_fil(fil, ta.chirped_train_rows(ta.TRAIN_A)[:, None, :], ta.FHDR, 1)
    base = fil.replace(".fil", "")
    assert post.main(["psearch", fil, "--dm", "30", "--dm2", "50", "--dmstep", "10"]) == 0
    plain_txt, plain_npz = open(base + "_psearch.txt", "rb").read(), open(base + "_psearch.npz", "rb").read()
    _files, g0 = post.psearch_fil(fil, 30.0, dm2=50.0, dmstep=10.0, lib=hip_lib)
    assert open(base + "_psearch.txt", "rb").read() == plain_txt and plain_txt.decode().splitlines()[0] == post.PS_HEADER
    back0 = np.load(base + "_psearch.npz")
    assert back0["candidates"].tobytes() == g0.tobytes() and "accs" not in back0.files and len(plain_npz) > 0
    assert post.main(["psearch", fil, "--dm", "30", "--dm2", "50", "--dmstep", "10", "--amax", "4e6", "--astep", "1e6", "--fold-best", "1"]) == 0
    assert "periodic candidates above 6.0 sigma" in capsys.readouterr().out
    back = np.load(base + "_psearch.npz")
    best = back["candidates"][0]["best"]
    assert float(best["acc_ms2"]) == ta.TRAIN_A and int(best["dm_index"]) == 1
    assert float(best["sigma"]) > float(back0["candidates"][0]["best"]["sigma"])
    # the folded profile peaks in one region of phase: split in four sub-integrations, the peak stays within nbin / 8
    prof, hits, meta = post.read_archive(base + "_psearch_cand0.ar")
    assert meta["f1"] == -meta["f0"] * ta.TRAIN_A / ao.C_LIGHT
    f = post.sigproc.read_fil(fil)
    par = {"F0": meta["f0"], "F1": meta["f1"], "DM": 40.0, "PEPOCH": meta["pepoch"], "PSR": "cand0"}
    p4, h4, nbin = post.fold(f, par, subint_s=0.5, lib=hip_lib)
    peaks = [int(np.argmax(post._scrunched(p4[s:s + 1], h4[s:s + 1], ta.FHDR, par["F0"], par["DM"], 64)[1])) for s in range(4)]
    spread = [min((a - peaks[0]) % nbin, (peaks[0] - a) % nbin) for a in peaks]
    assert max(spread) <= nbin // 8, (peaks, nbin)
    # without F1 the same fold drifts: the frequency changes by nearly a bin of the 2.1 s transform over the file
    assert os.path.getsize(base + "_psearch_cand0.png") > 0
