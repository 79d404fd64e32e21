"""Periodicity search of the dedispersed series (frbch_psearch_*, frbch_ps_group_cands, post.periodicity_search /
group_periodic / psearch_fil): the generic kernels through the TEST-ONLY emulator build against the numpy restatement
tests/psearch_oracle.py record for record (dm_index, h, k and the float bits of H exactly), the thresholds against the closed
form, capacity and argument errors, and known answers on synthetic 8-bit filterbanks through the file-level entry point."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from oracle import post_oracle as po
from tests import psearch_cases as pc
from tests import psearch_oracle as pso
from tests.test_fold_predictor import write_fil
from tests.test_post import HDR

FHDR = dict(HDR, tsamp=256e-6)          # 64 channels of 0.5 MHz below 1400 MHz; 8192 samples are 2.1 s, a bin 0.477 Hz
P_TRAIN, DM_TRAIN = 0.0334, 40.0
DMS = dict(dm1=0.0, dm2=70.0, dmstep=10.0)      # 8 trial DMs; DM_TRAIN is trial 4
NROWS = 8192 + 40                       # the delay across the band at DM 70 is 27 samples: nout stays above 8192


# ---- the emulator against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_emulator_equals_the_oracle(emu_lib, name):
    y, tsamp, kw, want, _raw = pc.case(name)
    rc, got, ncand, used, msg = pc.psearch_host(emu_lib, y, tsamp, **kw)
    assert rc == 0, msg
    assert used == (0, 0) and ncand == want.size
    assert pc.same_records(got, want)
    groups = post.group_periodic(got, 2, lib=emu_lib)
    assert pc.same_groups(groups, pso.group(want, 2))


def test_the_cases_hold_what_they_are_written_for():
    """the properties the grid is there for, read from the oracle's results"""
    for name in pc.CASES:
        assert pc.case(name)[3].size > 0 or name == "never", name
    y, tsamp, kw, want, raw = pc.case("odd_3dm")
    assert y.shape[0] == 3 and set(want["dm_index"].tolist()) >= {0, 1}
    top0 = want[want["dm_index"] == 0]
    top0 = top0[np.argmax(top0["sigma"])]
    assert int(top0["h"]) == 1 and abs(top0["freq_hz"] - 37.3) <= 1.0 / (4096 * tsamp)          # the sine: one harmonic
    top1 = want[want["dm_index"] == 1]
    top1 = top1[np.argmax(top1["sigma"])]
    assert int(top1["h"]) >= 8 and abs(top1["freq_hz"] - 1.0 / (48.3 * tsamp)) <= 1.0 / (4096 * tsamp) / int(top1["h"]) + 1e-9
    assert len(raw) > want.size                                                                 # step 8 dropped something
    # the tail: the same records as the series cut at n
    for name in ("tail_ignored_nout_5000", "nfft_4096_of_9000"):
        y, tsamp, kw, want, _ = pc.case(name)
        assert pc.same_records(pso.search(y[:, :4096], tsamp, sigma=4.0), want)
    # nharm: the records of nharm = h are those of nharm = 16 before step 8, fold by fold
    raws = {h: pc.case("nharm_%d" % h)[4] for h in (1, 2, 4, 8, 16)}
    for h in (1, 2, 4, 8):
        assert raws[h] == [r for r in raws[16] if r[1] <= h] and len(raws[h]) < len(raws[2 * h])
    # a dead series yields nothing and its partner what it yields beside a zero series
    y, tsamp, kw, want, _ = pc.case("dead_beside_live")
    assert not np.isin(want["dm_index"], [0, 3]).any() and {1, 2} <= set(want["dm_index"].tolist())
    z = np.array(y)
    z[0] = 5.0
    z[3] = 5.0
    assert pc.same_records(pso.search(z, tsamp, sigma=4.0), want)
    y, tsamp, kw, want, _ = pc.case("constant_series")
    assert 1 not in want["dm_index"] and {0} <= set(want["dm_index"].tolist())
    y, tsamp, kw, want, raw = pc.case("flo_40hz_no_fold_16")
    assert pso.kmin_of(4096, tsamp, 40.0) == 164 and 16 * 164 > 2048 >= 8 * 164
    assert {r[1] for r in raw} == {1, 2, 4, 8} and min(r[2] // r[1] for r in raw) >= 164
    assert want["freq_hz"].min() >= 40.0


def test_block_rule():
    """the rest of the bins on either side of B / 2 (stated for any count of bins; with n and B powers of two the rest of
    n / 2 - 1 bins is always B - 1, a block of its own)"""
    assert pso.block_edges(2047, 128)[-2:] == [(1793, 1921), (1921, 2048)] and len(pso.block_edges(2047, 128)) == 16
    assert pso.block_edges(128 * 3 + 63, 128) == [(1, 129), (129, 257), (257, 448)]           # 63 < 64: joined
    assert pso.block_edges(128 * 3 + 64, 128) == [(1, 129), (129, 257), (257, 385), (385, 449)]   # 64: on its own
    for L in range(12, 23):
        for B in (32, 128, 1024):
            assert ((1 << (L - 1)) - 1) % B == B - 1


# ---- thresholds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 3.0, 6.0, 10.0, 30.0])
def test_thresholds_against_the_closed_form(emu_lib, sigma):
    thr = np.zeros(5, dtype=np.float32)
    assert emu_lib.frbch_psearch_thresholds(sigma, thr.ctypes.data) == 0
    tail = 0.5 * math.erfc(sigma / math.sqrt(2.0))

    def q(h, x):
        return math.exp(-x) * sum(x ** i / math.factorial(i) for i in range(h))

    for h, t in zip((1, 2, 4, 8, 16), thr):
        below = float(np.nextafter(t, np.float32(0.0)))
        assert q(h, float(t)) <= tail * (1.0 + 1e-12)                   # (1e-12: the closed form summed in another order)
        # the bisection stops at one step of double: the float below T_h lies below the whole last interval
        assert q(h, below) > tail
        assert q(h, below) <= tail * math.exp(2.0 * (float(t) - below))  # ... and not further than two float steps' worth of exp(-x)
    assert np.array_equal(thr, pso.thresholds(sigma))
    assert emu_lib.frbch_psearch_thresholds(0.0, thr.ctypes.data) == _lib.E_ARG
    assert emu_lib.frbch_psearch_thresholds(31.0, thr.ctypes.data) == _lib.E_ARG


def test_sigma_of_a_record_is_the_inverse_of_the_threshold(emu_lib):
    """a record exactly at T_h(6 sigma) has sigma 6 to the float rounding of T_h; a huge H stays finite"""
    thr = pso.thresholds(6.0)
    raw = np.zeros(7, dtype=post.PS_CAND)
    for i, (h, t) in enumerate(zip((1, 2, 4, 8, 16), thr)):
        raw[i] = (i, h, 100 * h, t, 0.0, 0.0)
    raw[5] = (5, 16, 1000, np.float32(3.0e38), 0.0, 0.0)
    raw[6] = (6, 1, 1000, np.float32(np.inf), 0.0, 0.0)
    out = np.zeros(7, dtype=post.PS_CAND)
    n = C.c_uint64(0)
    err = C.create_string_buffer(256)
    assert emu_lib.frbch_psearch_sift(raw.ctypes.data, 7, 4096, 1e-3, out.ctypes.data, 7, C.byref(n), err, len(err)) == 0, err.value
    assert n.value == 7 and np.all(np.abs(out["sigma"][:5] - 6.0) < 1e-5) and np.all(np.isfinite(out["sigma"]))
    assert out["sigma"][5] > 1e18 and out["sigma"][6] > 1e18
    assert np.allclose(out["freq_hz"][:5], 100.0 / 4.096)
    assert pc.same_records(out, pso.sift([tuple(r)[:4] for r in raw.tolist()], 4096, 1e-3))


# ---- capacity and arguments ----------------------------------------------------------------------------------------
def test_capacity_of_the_record_list(emu_lib):
    y, tsamp, kw, want, _raw = pc.case("odd_3dm")
    assert want.size > 5
    rc, got, ncand, _used, msg = pc.psearch_host(emu_lib, y, tsamp, cap=5, **kw)
    assert rc == _lib.E_CAPACITY and ncand == want.size and "candidates" in msg and pc.same_records(got, want[:5])
    rc, got, ncand, _used, msg = pc.psearch_host(emu_lib, y, tsamp, cap=0, **kw)
    assert rc == _lib.E_CAPACITY and ncand == want.size
    info = {}
    assert pc.same_records(post.periodicity_search(y, tsamp, lib=emu_lib, info=info, cap=2, **kw), want)    # grows past cap
    assert info == dict(kernel_used=0, passes=0)


def test_raw_peak_list_overflow_is_an_error(emu_lib):
    """sigma 0.01 (T_1 = 0.70: half of all noise bins pass, a third of them are local maxima) on 24 x 2^17 noise samples:
    over 2^20 raw peaks in the five folds"""
    y = pc.noise(24, 1 << 17, 52)
    rc, got, ncand, _used, msg = pc.psearch_host(emu_lib, y, 64e-6, sigma=0.01)
    assert rc == _lib.E_CAPACITY and "threshold too low" in msg and got.size == 0 and ncand == 0


BAD = [dict(nfft=2048), dict(nfft=1 << 23), dict(nfft=8192), dict(nfft=5000), dict(nharm=3), dict(nharm=32), dict(wblock=48),
       dict(wblock=16), dict(wblock=2048), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=31.0),
       dict(flo=-1.0), dict(flo=float("inf")), dict(tsamp=0.0), dict(tsamp=-1e-3)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "%s=%s" % next(iter(b.items())))
def test_bad_arguments(emu_lib, bad):
    y = pc.noise(1, 5000, 53)                                    # nfft 8192 is above nout
    kw = dict(sigma=6.0)
    kw.update({k: v for k, v in bad.items() if k != "tsamp"})
    rc, _got, _n, _used, msg = pc.psearch_host(emu_lib, y, bad.get("tsamp", 1e-3), **kw)
    assert rc == _lib.E_ARG and msg
    p = pc.params_of(bad.get("tsamp", 1e-3), **kw)
    if "tsamp" not in bad:
        assert emu_lib.frbch_psearch_nfft(5000, C.byref(p)) == _lib.E_ARG
    assert emu_lib.frbch_psearch_kernel(y.ctypes.data, 1, 5000, C.byref(p), None) == _lib.E_ARG or "tsamp" in bad


def test_short_series_wrong_size_and_too_many_dms(emu_lib):
    y = pc.noise(1, 4095, 54)
    rc, _g, _n, _u, msg = pc.psearch_host(emu_lib, y, 1e-3)
    assert rc == _lib.E_ARG and "2^12" in msg                    # no power of two in range fits 4095 samples
    y = pc.noise(1, 4096, 54)
    p = pc.params_of(1e-3)
    assert emu_lib.frbch_psearch_nfft(4096, C.byref(p)) == 4096 and emu_lib.frbch_psearch_nfft(1 << 23, C.byref(p)) == 1 << 22
    p.size -= 8
    n = C.c_uint64(0)
    err = C.create_string_buffer(256)
    assert emu_lib.frbch_psearch_host(y.ctypes.data, 1, 4096, C.byref(p), 0, None, 0, C.byref(n), None, err, len(err)) == _lib.E_ARG
    assert b"size" in err.value and emu_lib.frbch_psearch_nfft(4096, C.byref(p)) == _lib.E_ARG
    p = pc.params_of(1e-3)
    # the limit the single-pulse search states: 65535 series (refused before anything is read)
    assert emu_lib.frbch_psearch_host(y.ctypes.data, 65536, 4096, C.byref(p), 0, None, 0, C.byref(n), None, err, len(err)) == _lib.E_ARG
    assert b"65535" in err.value
    with pytest.raises(post.InputError):
        post.periodicity_search(y, 1e-3, nharm=3, lib=emu_lib)
    used = C.c_uint32(7)
    assert emu_lib.frbch_psearch_kernel(y.ctypes.data, 1, 4096, C.byref(p), C.byref(used)) == 0 and used.value == 0   # the emulator has no fast form


def test_grouping_rules(emu_lib):
    rec = np.zeros(6, dtype=post.PS_CAND)
    #          dm h  k    H    sigma  f
    rec[0] = (0, 1, 100, 30., 7.0, 0.0)
    rec[1] = (1, 2, 201, 40., 9.0, 0.0)        # 100.5 bins: within 1.5 of record 0, one trial apart -> joined
    rec[2] = (4, 1, 100, 30., 8.0, 0.0)        # three trials from record 1: not with dm_gap 2
    rec[3] = (2, 1, 102, 30., 6.5, 0.0)        # 1.5 bins from record 1 exactly -> joined; 2 from record 0
    rec[4] = (2, 4, 800, 30., 9.0, 0.0)        # the second harmonic's ladder: 200 bins, its own group (harmonics are not merged)
    rec[5] = (3, 1, 104, 30., 6.0, 0.0)        # 2 bins from record 3: alone
    got = post.group_periodic(rec, 2, lib=emu_lib)
    want = pso.group(rec, 2)
    assert pc.same_groups(got, want)
    assert [(int(g["best"]["dm_index"]), int(g["best"]["k"]), int(g["nmember"]), int(g["dm_index_lo"]), int(g["dm_index_hi"])) for g in got] == \
        [(1, 201, 3, 0, 2), (2, 800, 1, 2, 2), (4, 100, 1, 4, 4), (3, 104, 1, 3, 3)]
    assert post.group_periodic(rec, 3, lib=emu_lib)["nmember"].tolist() == [4, 1, 1]            # record 2 joins through record 1
    assert post.group_periodic(rec[:0], 2, lib=emu_lib).size == 0
    for gap in (0, 17):
        with pytest.raises(post.InputError):
            post.group_periodic(rec, gap, lib=emu_lib)
    rec["h"][0] = 3
    with pytest.raises(post.InputError):
        post.group_periodic(rec, 2, lib=emu_lib)


# ---- known answers through the file-level entry point --------------------------------------------------------------
def train_rows(seed=3, amp=12):
    """noise 96 .. 159 and a pulse of one sample, `amp` high, every P_TRAIN in every channel, dispersed at DM_TRAIN"""
    rng = np.random.default_rng(seed)
    x = rng.integers(96, 160, size=(NROWS, FHDR["nchans"])).astype(np.int64)
    dly = po.delays_seconds(FHDR["fch1"], FHDR["foff"], FHDR["nchans"], DM_TRAIN)
    for k in range(int(NROWS * FHDR["tsamp"] / P_TRAIN) + 1):
        for c in range(FHDR["nchans"]):
            i = int(round(((k + 0.25) * P_TRAIN + dly[c]) / FHDR["tsamp"]))
            if i < NROWS:
                x[i, c] += amp
    return x.astype(np.uint8)


def fil_of(tmp_path, name, x):
    path = str(tmp_path / name)
    write_fil(path, x[:, None, :], FHDR, 1)
    return path


def test_pulse_train_comes_back_at_its_period_and_dm(emu_lib, tmp_path):
    fil = fil_of(tmp_path, "train.fil", train_rows())
    info = {}
    files, groups = post.psearch_fil(fil, lib=emu_lib, info=info, **DMS)
    assert info["nfft"] == 8192 and info["kernel_used"] == 0 and groups.size >= 1
    best = groups[0]["best"]
    h = int(best["h"])
    assert h > 1 and int(best["dm_index"]) == 4
    assert abs(best["freq_hz"] - 1.0 / P_TRAIN) <= 1.0 / (8192 * FHDR["tsamp"]) / h
    assert np.all(np.diff(groups["best"]["sigma"]) <= 0)
    # the library's answer is the answer of the two steps restated
    dms = post.dm_list(DMS["dm1"], DMS["dm2"], DMS["dmstep"])
    x = np.fromfile(fil, dtype=np.uint8)[-NROWS * 64:].reshape(NROWS, 64)
    y, _nclip = po.dedisperse(x, fch1=FHDR["fch1"], foff=FHDR["foff"], tsamp=FHDR["tsamp"], dms=dms, zerodm=True, clip=5.0)
    want = pso.search(y, FHDR["tsamp"], sigma=6.0, nharm=16, flo=0.5, wblock=128)
    assert pc.same_records(info["records"], want) and pc.same_groups(groups, pso.group(want, 2))
    # the files
    base = fil.replace(".fil", "")
    assert files == [base + "_psearch.txt", base + "_psearch.npz"]
    lines = open(files[0]).read().splitlines()
    assert lines[0] == post.PS_HEADER and len(lines) == 1 + groups.size
    first = lines[1].split()
    assert abs(float(first[0]) - P_TRAIN) < 2e-5 and float(first[2]) == DM_TRAIN and int(first[4]) == h
    back = np.load(files[1])
    assert pc.same_records(back["records"], want) and back["candidates"].size == groups.size and int(back["nfft"]) == 8192


def test_mains_hum_comes_back_at_dm_zero_with_one_harmonic(emu_lib, tmp_path):
    rng = np.random.default_rng(5)
    t = np.arange(NROWS) * FHDR["tsamp"]
    x = rng.integers(96, 160, size=(NROWS, 64)) + np.round(4.0 * np.sin(2 * np.pi * 50.0 * t))[:, None]
    fil = fil_of(tmp_path, "hum.fil", x.astype(np.uint8))
    _files, groups = post.psearch_fil(fil, dm1=0.0, dm2=350.0, dmstep=50.0, zerodm=False, lib=emu_lib)
    best = groups[0]["best"]
    assert int(best["dm_index"]) == 0 and int(best["h"]) == 1 and abs(best["freq_hz"] - 50.0) <= 1.0 / (8192 * FHDR["tsamp"])


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_noise_gives_no_candidate(emu_lib, tmp_path, seed):
    """about 2^12 bins x 5 folds x 8 DMs at 6 sigma (1e-9 a trial): 2e-4 expected.  The seeds are those for which the oracle
    alone finds nothing -- a condition on the input, checked here first"""
    rng = np.random.default_rng(seed)
    x = rng.integers(96, 160, size=(NROWS, 64)).astype(np.uint8)
    dms = post.dm_list(DMS["dm1"], DMS["dm2"], DMS["dmstep"])
    y, _ = po.dedisperse(x, fch1=FHDR["fch1"], foff=FHDR["foff"], tsamp=FHDR["tsamp"], dms=dms, zerodm=True, clip=5.0)
    assert pso.search(y, FHDR["tsamp"], sigma=6.0).size == 0
    files, groups = post.psearch_fil(fil_of(tmp_path, "noise.fil", x), lib=emu_lib, **DMS)
    assert groups.size == 0 and open(files[0]).read() == post.PS_HEADER + "\n"


def test_fold_best_and_the_fold_seam(emu_lib, tmp_path, monkeypatch, capsys):
    fil = fil_of(tmp_path, "train.fil", train_rows())
    emu = emu_lib
    monkeypatch.setattr(_lib, "load", lambda path=None: emu)
    assert post.main(["psearch", fil, "--dm", "0", "--dm2", "70", "--dmstep", "10", "--fold-best", "1", "--max-cands", "3"]) == 0
    out = capsys.readouterr().out
    base = fil.replace(".fil", "")
    assert "wrote %s_psearch_cand0.ar" % base in out and "3 periodic candidates above 6.0 sigma" in out
    for ext in (".ar", ".profile.txt", ".png"):
        assert os.path.getsize(base + "_psearch_cand0" + ext) > 0
    prof, hits, meta = post.read_archive(base + "_psearch_cand0.ar")
    groups = np.load(base + "_psearch.npz")["candidates"]
    assert meta["f0"] == float(groups[0]["best"]["freq_hz"]) and meta["dm"] == DM_TRAIN and meta["f1"] == 0.0 and meta["pepoch"] == FHDR["tstart"]
    # one sub-integration of 10 s holds the 2.1 s file: split the fold in four and see the peak stay where it is
    f = post.sigproc.read_fil(fil)
    par = {"F0": meta["f0"], "F1": 0.0, "DM": DM_TRAIN, "PEPOCH": FHDR["tstart"], "PSR": "cand0"}
    p4, h4, nbin = post.fold(f, par, subint_s=0.5, lib=emu)
    assert p4.shape[0] >= 4
    peaks = []
    for s in range(4):
        mean_f, profile = post._scrunched(p4[s:s + 1], h4[s:s + 1], FHDR, par["F0"], par["DM"], 64)
        peaks.append(int(np.argmax(profile)))
    spread = [min((a - peaks[0]) % nbin, (peaks[0] - a) % nbin) for a in peaks]
    # the peak bin k is the nearest to h f: the frequency is good to half a bin / h, so over the n samples the pulse drifts by at
    # most 0.5 / h turns, nbin / (2 h) phase bins; one more for the rounding of a peak to its bin
    h = int(groups[0]["best"]["h"])
    assert max(spread) <= math.ceil(nbin / (2.0 * h)) + 1 <= nbin // 8, (peaks, nbin, h)
    # fold_fil with a par file: what it wrote before the seam was cut, byte for byte -- _fold_par IS its former body, so the
    # two ways in must agree on every file
    par_path = str(tmp_path / "x.par")
    with open(par_path, "w") as fh:
        fh.write("PSRJ cand0\nF0 %.17g\nF1 0\nDM %.17g\nPEPOCH %.17g\n" % (meta["f0"], DM_TRAIN, FHDR["tstart"]))
    ar, _profile = post.fold_fil(fil, par_path, lib=emu, out_base=str(tmp_path / "viapar"))
    for ext in (".ar", ".profile.txt", ".png"):
        assert open(str(tmp_path / "viapar") + ext, "rb").read() == open(base + "_psearch_cand0" + ext, "rb").read(), ext


def test_fold_fil_writes_what_it_wrote_before_the_seam(emu_lib, tmp_path):
    """fold_fil with a par file on the pulse-train file: the archive and the text profile byte for byte, the image pixel for
    pixel, as the commit before the seam (_fold_par) wrote them -- the hashes were taken with that commit's code"""
    import hashlib
    from tests.test_fold_predictor import png_pixels
    fil = fil_of(tmp_path, "train.fil", train_rows())
    par = str(tmp_path / "x.par")
    with open(par, "w") as fh:
        fh.write("PSRJ J0000+00\nF0 29.94\nF1 0\nDM 40\nPEPOCH 59000.25\n")
    post.fold_fil(fil, par, lib=emu_lib, out_base=str(tmp_path / "out"))
    sha = {ext: hashlib.sha256(open(str(tmp_path / "out") + ext, "rb").read()).hexdigest() for ext in (".ar", ".profile.txt")}
    assert sha == {".ar": "d8dd52e8698a704152c895d5b90935fcd312834b560dc81e78559cd7857fb4a7",
                   ".profile.txt": "f3c7733ad2055fdc5b3d022e98a110ef29b0a9d097b01735f09a8d15d657db45"}
    assert png_pixels(str(tmp_path / "out.png")) == (128, 72, "ed7ae871ad746c93ed259487d4bfaec72ceb10bf27be04b6d8a698d6c1215a25")
