"""GPU tests of the periodicity search (frbch_psearch_*, frbch_dedisperse_psearch_host): the fast form -- the transform in
one, two or three LDS-resident passes -- and the generic form it falls back to, against the numpy restatement
tests/psearch_oracle.py record for record: dm_index, h, k and the float bits of H exactly (the transform is a fixed graph of
float32 operations, the sums have a fixed order), sigma and freq_hz to psearch_oracle.SIGMA_RTOL.  Every case asserts the form
and the number of passes it aimed at, and that the _device form leaves its input and the guard bands as they were."""
import ctypes as C
import functools

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import post_cases as poc
from tests import psearch_cases as pc
from tests import psearch_oracle as pso

pytestmark = pytest.mark.gpu

FAST, GENERIC = 1, 0


def passes_of(n):
    """the documented plan: one pass up to 2^13, two up to 2^18, three above"""
    return 1 if n <= 1 << 13 else 2 if n <= 1 << 18 else 3


device_search = pc.device_search          # (shared with tests/test_gpu_search_dense.py and the emulator twins)


@functools.lru_cache(maxsize=None)
def big_case(ndm, log2n, seed, extra=0, sigma=4.0):
    """-> (series, tsamp, oracle records at `sigma`); built once, never written to"""
    tsamp = 64e-6
    y = pc.signals(ndm, (1 << log2n) + extra, seed, tsamp)
    y.setflags(write=False)
    return y, tsamp, pso.search(y, tsamp, sigma=sigma)


# ---- every case of the emulator grid, fast and generic -------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_device_equals_the_oracle(hip_lib, name):
    """n = 2^12, 2^13 (one pass) and 2^14 (two); 1 .. 5 series; every nharm and both extreme wblock; a tail beyond n, a dead
    series beside a live one, a constant one, a fold without a bin"""
    y, tsamp, kw, want, _raw = pc.case(name)
    n = pso.nfft_of(y.shape[1], kw.get("nfft", 0))
    got, used = device_search(hip_lib, y, tsamp, **kw)
    assert used == (FAST, passes_of(n)) and pc.same_records(got, want)
    got, used = device_search(hip_lib, y, tsamp, misalign=True, **kw)
    assert used == (GENERIC, 0) and pc.same_records(got, want)


# ---- the smallest n of every pass structure, odd and even ndm ------------------------------------------------------
@pytest.mark.parametrize("log2n,ndm", [(12, 2), (12, 3), (14, 2), (14, 3), (19, 2), (19, 3)])
def test_fast_form_at_the_first_length_of_every_pass_count(hip_lib, log2n, ndm):
    """2^12: one pass; 2^14: the first length with two; 2^19: the first with three.  nout = n + 5: rows that are not 64-byte
    aligned, and a tail"""
    y, tsamp, want = big_case(ndm, log2n, 60 + log2n + ndm, extra=5)
    assert want.size > 0 and passes_of(1 << log2n) == {12: 1, 14: 2, 19: 3}[log2n]
    assert log2n == 12 or passes_of(1 << (log2n - 1)) == passes_of(1 << log2n) - 1
    got, used = device_search(hip_lib, y, tsamp, sigma=4.0)
    assert used == (FAST, passes_of(1 << log2n)) and pc.same_records(got, want)


@pytest.mark.parametrize("log2n", [13, 18, 20])
def test_fast_form_at_the_last_length_of_a_pass_count_and_beyond(hip_lib, log2n):
    """2^13 and 2^18: the longest one- and two-pass transforms (9 stages a pass); 2^20: three passes of 7, 7 and 6"""
    y, tsamp, want = big_case(2, log2n, 70 + log2n)
    got, used = device_search(hip_lib, y, tsamp, sigma=4.0)
    assert used == (FAST, passes_of(1 << log2n)) and pc.same_records(got, want)


def test_64_series_of_2_17(hip_lib):
    y, tsamp, want = big_case(64, 17, 80, sigma=5.0)
    assert len(set(want["dm_index"].tolist())) >= 40
    got, used = device_search(hip_lib, y, tsamp, sigma=5.0, cap=1 << 16)
    assert used == (FAST, 2) and pc.same_records(got, want)


def test_generic_form_at_three_pass_length(hip_lib):
    y, tsamp, want = big_case(3, 19, 60 + 19 + 3, extra=5)
    got, used = device_search(hip_lib, y, tsamp, misalign=True, sigma=4.0)
    assert used == (GENERIC, 0) and pc.same_records(got, want)


def test_raw_peak_list_overflow_is_an_error(hip_lib):
    y = pc.noise(24, 1 << 17, 52)
    rc, got, ncand, _used, msg = pc.psearch_host(hip_lib, y, 64e-6, sigma=0.01)
    assert rc == _lib.E_CAPACITY and "threshold too low" in msg and got.size == 0 and ncand == 0


# ---- dedispersion and search in one call ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,zerodm,clip", [(8, True, 5.0), (32, False, 0.0)])
def test_dedisperse_psearch_equals_the_two_calls(hip_lib, nbits, zerodm, clip):
    hdr = poc.make_hdr(1024)
    x = poc.make_rows(20000, 2, 1024, nbits, seed=21)
    dms = [40.0 + 1.5 * i for i in range(9)]
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    nout = poc.dedisp_nout(hip_lib, hdr, x, 1, dms)
    series, nclip = poc.dedisp_host(hip_lib, hdr, x, 1, dms, zerodm, clip, nout)
    rc, want, nwant, used, msg = pc.psearch_host(hip_lib, series, hdr["tsamp"], sigma=3.0)
    assert rc == 0 and used == (FAST, 2) and nwant > 0, msg
    params = pc.params_of(0.0, sigma=3.0)                     # tsamp_s = 0: the file's
    for with_series in (True, False):
        out = np.zeros((9, nout), dtype=np.float32)
        cands = np.zeros(8192, dtype=post.PS_CAND)
        ncand, k, nc = C.c_uint64(0), (C.c_uint32 * 2)(9, 9), C.c_uint64(0)
        err = C.create_string_buffer(512)
        rc = hip_lib.frbch_dedisperse_psearch_host(C.byref(poc.desc_of(hdr, x, 1)), x.ctypes.data, x.shape[0], dm_arr.ctypes.data, 9,
                                                   1 if zerodm else 0, clip, C.byref(params), 0, out.ctypes.data if with_series else None,
                                                   nout, C.byref(nc), cands.ctypes.data, 8192, C.byref(ncand), k, err, len(err))
        assert rc == 0, err.value
        assert (k[0], k[1]) == (FAST, 2) and nc.value == nclip and ncand.value == nwant
        assert cands[:nwant].tobytes() == want.tobytes()          # the same library twice: every byte
        if with_series:
            assert out.tobytes() == series.tobytes()
    assert pc.same_records(want, pso.search(series, hdr["tsamp"], sigma=3.0))


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_pulse_train_end_to_end(hip_lib, tmp_path, monkeypatch, capsys):
    """the pulse train of tests/test_psearch.py (P = 33.4 ms at DM 40 in 8-bit noise, 64 channels) through `post psearch`"""
    from tests import test_psearch as tp
    fil = tp.fil_of(tmp_path, "train.fil", tp.train_rows())
    assert post.main(["psearch", fil, "--dm", "0", "--dm2", "70", "--dmstep", "10", "--fold-best", "1"]) == 0
    assert "periodic candidates above 6.0 sigma" in capsys.readouterr().out
    back = np.load(fil.replace(".fil", "_psearch.npz"))
    best = back["candidates"][0]["best"]
    h = int(best["h"])
    assert h > 1 and int(best["dm_index"]) == 4 and abs(best["freq_hz"] - 1.0 / tp.P_TRAIN) <= 1.0 / (8192 * tp.FHDR["tsamp"]) / h
    info = {}
    _files, groups = post.psearch_fil(fil, lib=hip_lib, info=info, **tp.DMS)
    assert (info["kernel_used"], info["passes"], info["nfft"]) == (FAST, 1, 8192)
    assert groups.tobytes() == back["candidates"].tobytes()
    import os
    assert os.path.getsize(fil.replace(".fil", "_psearch_cand0.ar")) > 0
