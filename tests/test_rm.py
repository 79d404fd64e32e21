"""CPU tests of the burst polarisation stage (frbch_burstspec_*, frbch_rmsynth_*, frbch_burst_rm_*, frbch_rm_peaks) through the
emulator build, which runs the generic kernels: sums, spectra, `used`, F and the results byte for byte against the numpy
restatement tests/rm_oracle.py (pa0, which goes through libm's atan2, to 1e-12), the table against numpy's, every refusal,
windows partly and wholly outside the data, masked channels, a dead candidate, the RMSF, the known answer (an injected RM
recovered at the trial the plain fp64 evaluation finds, within a measured tolerance), and `post rmsynth` end to end."""
import ctypes as C
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import rm_cases as rc
from tests import rm_oracle as ro


# ---- the table -------------------------------------------------------------------------------------------------------
def test_table_equals_numpy(emu_lib):
    t = np.full(16384, 12345, dtype=np.int32)
    assert emu_lib.frbch_rm_table(t.ctypes.data) == 0
    want = ro.table()
    assert t.tobytes() == want.tobytes()
    j = np.arange(16384)
    assert t[0] == 1 << 22 and t[4096] == 0 and t[8192] == -(1 << 22) and t[12288] == 0
    assert np.array_equal(t[(8192 - j) % 16384], -t) and np.array_equal(t[(16384 - j) % 16384], t)     # exact symmetry
    assert np.abs(t - np.cos(2 * np.pi * j / 16384) * 2 ** 22).max() <= 0.5 + 1e-6
    assert emu_lib.frbch_rm_table(None) == _lib.E_ARG


# ---- step 1: sums and spectra ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_spectra_equal_the_oracle(emu_lib, name):
    hdr, rows, cands, coh = rc.case(name)
    sums, spec, noise, used = rc.want_spectra(name)
    info = {}
    got = post.burst_spectra(rows, hdr, cands, products="coherency" if coh else "stokes", lib=emu_lib, info=info)
    assert info["kernel_used"] == 0
    assert info["sums"].tobytes() == sums.tobytes()
    assert got[0].tobytes() == spec.tobytes() and got[1].tobytes() == noise.tobytes() and got[2].tobytes() == used.tobytes()
    assert emu_lib.frbch_burstspec_kernel(C.byref(rc.desc_of(hdr, rows)), rows.ctypes.data, rows.shape[0], C.byref(rc.burst_par(coh)),
                                          cands.ctypes.data, cands.size) == 0


def test_the_cases_see_their_bursts_and_their_edges():
    """the oracle alone: a burst stands out in I, windows partly outside count fewer rows, one wholly outside leaves nothing"""
    sums, spec, noise, used = rc.want_spectra("u8_64ch_3cand")
    assert used.all() and (spec[:, 0] > 10 * noise[:, 0]).all()
    assert (sums["off_hits"][0] == 400).all() and (sums["on_hits"][0] == 6).all()
    assert sums["off_hits"][2].max() < 400 and sums["off_hits"][2].min() >= 200            # B_EDGE: the earlier window is cut
    sums, spec, noise, used = rc.want_spectra("u8_96ch")
    assert not used[2].any() and not spec[2].any() and (sums["on_hits"][2] == 0).all()     # B_OUT
    sums, _s, _n, used = rc.want_spectra("u8_1024ch")
    assert sums["off_hits"][2].min() < 600 and used[2].all()                               # B_LATE: the later window leaves the data
    hdr = rc.case("u8_1024ch")[0]
    assert ro.delays(hdr, rc.B_LATE["dm"]).max() > 3000


def test_gains_scale_the_spectra_and_can_drop_a_channel(emu_lib):
    hdr, rows, cands, coh = rc.case("u8_64ch_3cand")
    rng = np.random.default_rng(5)
    gain = rng.uniform(0.5, 2.0, size=(4, 64)).astype(np.float32)
    gain[1, 7] = -1.5
    gain[2, 9] = 0.0
    gain[3, 11] = np.inf
    sums = rc.want_spectra("u8_64ch_3cand")[0]
    spec, noise, used = ro.derive(sums, gain, False)
    got = post.burst_spectra(rows, hdr, cands, gains=gain, lib=emu_lib)
    assert got[0].tobytes() == spec.tobytes() and got[1].tobytes() == noise.tobytes() and got[2].tobytes() == used.tobytes()
    assert not used[:, 11].any() and used[:, 9].all() and (noise[:, 1, 7] > 0).all() and not spec[:, :, 11].any()


def test_a_float_row_that_is_not_finite_drops_its_channel(emu_lib):
    hdr, rows, cands, _coh = rc.case("f32_64ch")
    x = rows.copy()
    on_lo = int(cands[0]["sample"]) - int(cands[0]["width"]) // 2
    x[on_lo + int(ro.delays(hdr, float(cands[0]["dm"]))[5]), 2, 5] = np.nan
    spec, noise, used = ro.burst_spectra(x, hdr, cands)
    got = post.burst_spectra(x, hdr, cands, lib=emu_lib)
    assert used[0, 5] == 0 and used[0].sum() == 63
    assert got[0].tobytes() == spec.tobytes() and got[1].tobytes() == noise.tobytes() and got[2].tobytes() == used.tobytes()


# ---- step 2: the transform ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan,ncand,nphi,phi_lo,dphi,masked", [(64, 1, 1, 250.0, 10.0, ()), (64, 3, 257, -12800.0, 100.0, (3, 40)),
                                                                 (96, 3, 257, -3000.0, 23.5, ()), (96, 1, 4096, -1.0e5, 48.8, (0, 95))])
def test_transform_equals_the_oracle(emu_lib, nchan, ncand, nphi, phi_lo, dphi, masked):
    hdr, q, u, used = rc.spectra(nchan, ncand, 0, masked)
    info = {}
    F = post.rm_synthesis(q, u, used, hdr, nphi, phi_lo, dphi, lib=emu_lib, info=info)
    assert info == dict(kernel_used=0, split=1)
    assert np.ascontiguousarray(F).view(np.float32).tobytes() == rc.want_transform(nchan, ncand, nphi, phi_lo, dphi, 0, masked).tobytes()
    par = post.rm_params(nphi, phi_lo, dphi)
    assert emu_lib.frbch_rmsynth_kernel(C.byref(post.fil_desc(hdr)), F.ctypes.data, ncand, C.byref(par), None) == 0


def test_a_masked_channel_is_not_read(emu_lib):
    """NaN in a channel that `used` clears changes nothing; the same NaN in a used channel is refused"""
    hdr, q, u, used = rc.spectra(64, 3, 0, (3, 40))
    q2 = q.copy()
    q2[:, 3] = np.nan
    a = post.rm_synthesis(q, u, used, hdr, 257, -12800.0, 100.0, lib=emu_lib)
    b = post.rm_synthesis(q2, u, used, hdr, 257, -12800.0, 100.0, lib=emu_lib)
    assert a.tobytes() == b.tobytes()
    with pytest.raises(post.InputError, match="not finite"):
        post.rm_synthesis(q2, u, np.ones_like(used), hdr, 257, -12800.0, 100.0, lib=emu_lib)


def test_a_dead_candidate_gives_zeros(emu_lib):
    hdr, q, u, used = rc.spectra(64, 3, 1)
    q2, u2, used2 = q.copy(), u.copy(), used.copy()
    q2[1], u2[1] = 0.0, 0.0                                       # m = 0
    used2[2] = 0                                                  # N = 0
    F = post.rm_synthesis(q2, u2, used2, hdr, 257, -12800.0, 100.0, lib=emu_lib)
    want, _re, _im = ro.transform(q2, u2, used2, hdr, 257, -12800.0, 100.0)
    assert np.ascontiguousarray(F).view(np.float32).tobytes() == want.tobytes()
    assert F[0].any() and not F[1].any() and not F[2].any()
    res = post.rm_peaks(F, used2, None, None, hdr, 257, -12800.0, 100.0, lib=emu_lib)
    assert res["kpeak"].tolist()[1:] == [0, 0] and res["fitted"].tolist()[1:] == [0, 0] and res["nused"].tolist() == [64, 64, 0]
    assert res["rm"][1] == -12800.0 and res["peak"][1] == 0.0 and not res["snr"].any()


def test_rmsf_is_exactly_one_at_zero_depth(emu_lib):
    hdr, _q, _u, used = rc.spectra(96, 3, 0, (10, 11))
    nphi, phi_lo, dphi = 257, -128 * 37.5, 37.5
    ones = used.astype(np.float32)
    F = post.rm_synthesis(ones, np.zeros_like(ones), used, hdr, nphi, phi_lo, dphi, lib=emu_lib)
    assert (F[:, 128] == np.complex64(1.0)).all()
    assert (np.abs(F) <= 1.0).all() and (np.argmax(np.abs(F), axis=1) == 128).all()
    _F, re, im = ro.transform(ones, np.zeros_like(ones), used, hdr, nphi, phi_lo, dphi)
    n = used.sum(axis=1).astype(np.int64)
    assert np.array_equal(re[:, 128], n * (1 << 22) * (1 << 22)) and not im[:, 128].any()


# ---- step 3 and the composite -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_composite_equals_the_oracle(emu_lib, name):
    hdr, rows, cands, coh = rc.case(name)
    _sums, spec, noise, used = rc.want_spectra(name)
    F, res = rc.want_rm(name)
    info = {}
    got = post.burst_rm(rows, hdr, cands, lib=emu_lib, info=info, products="coherency" if coh else "stokes", **rc.GRID)
    assert info == dict(spectra_kernel_used=0, kernel_used=0, split=1)
    assert got["spec"].tobytes() == spec.tobytes() and got["noise"].tobytes() == noise.tobytes() and got["used"].tobytes() == used.tobytes()
    assert np.ascontiguousarray(got["F"]).view(np.float32).tobytes() == F.tobytes()
    assert rc.same_results(got["results"], res), (got["results"], res)
    # the stages one by one give the same
    F2 = post.rm_synthesis(spec[:, 1], spec[:, 2], used, hdr, lib=emu_lib, **rc.GRID)
    assert F2.tobytes() == got["F"].tobytes()
    res2 = post.rm_peaks(F2, used, noise[:, 1], noise[:, 2], hdr, lib=emu_lib, **rc.GRID)
    assert res2.tobytes() == got["results"].tobytes()


def test_composite_with_flagged_channels(emu_lib):
    hdr, rows, cands, _coh = rc.case("u8_64ch_3cand")
    flag = np.zeros(64, np.uint8)
    flag[[0, 17, 63]] = 1
    want = ro.burst_rm(rows, hdr, cands, flag=flag, **rc.GRID)
    got = post.burst_rm(rows, hdr, cands, flag=flag, lib=emu_lib, **rc.GRID)
    assert got["used"].tobytes() == want["used"].tobytes() and not got["used"][:, 17].any() and got["used"].sum() == 3 * 61
    assert np.ascontiguousarray(got["F"]).view(np.float32).tobytes() == want["F"].tobytes()
    assert rc.same_results(got["results"], want["results"])
    assert not np.array_equal(want["F"], rc.want_rm("u8_64ch_3cand")[0])


def test_peaks_at_the_ends_of_the_grid_have_no_fit(emu_lib):
    hdr = rc.make_hdr(64)
    F = np.zeros((2, 5), np.complex64)
    F[0, 0], F[0, 1] = 3 + 4j, 1.0
    F[1, 4], F[1, 2] = -2j, 1.0
    used = np.ones((2, 64), np.uint8)
    res = post.rm_peaks(F, used, None, None, hdr, 5, -20.0, 10.0, lib=emu_lib)
    assert res["kpeak"].tolist() == [0, 4] and res["fitted"].tolist() == [0, 0]
    assert res["rm"].tolist() == [-20.0, 20.0] and res["peak"].tolist() == [5.0, 2.0]
    assert rc.same_results(res, ro.peaks(np.ascontiguousarray(F).view(np.float32), used, None, None, hdr, 5, -20.0, 10.0))
    F[0, 0] = 1.0                                                 # a tie: the first largest wins
    assert post.rm_peaks(F, used, None, None, hdr, 5, -20.0, 10.0, lib=emu_lib)["kpeak"][0] == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _spec_call(lib, hdr, rows, cands, par=None, ncand=None, nrows=None):
    n = cands.size if ncand is None else ncand
    err = C.create_string_buffer(256)
    sums = np.zeros((max(n, 1), 4, hdr["nchans"]), dtype=post.BURST_SUMS)
    par = par if par is not None else rc.burst_par()
    rc_ = lib.frbch_burstspec_host(C.byref(rc.desc_of(hdr, rows)), rows.ctypes.data, rows.shape[0] if nrows is None else nrows, C.byref(par),
                                   cands.ctypes.data, n, None, 0, sums.ctypes.data, None, None, None, None, err, len(err))
    return rc_, err.value.decode()


def test_burstspec_refusals(emu_lib):
    hdr, rows, cands, _coh = rc.case("u8_64ch")
    assert _spec_call(emu_lib, hdr, rows, cands)[0] == 0
    assert _spec_call(emu_lib, hdr, rows, cands, par=rc.burst_par(size=4)) == (_lib.E_ARG, "frbch_burst_params: wrong size")
    bad = rc.burst_par()
    bad.products = 2
    assert _spec_call(emu_lib, hdr, rows, cands, par=bad)[0] == _lib.E_ARG
    assert _spec_call(emu_lib, hdr, rows, cands, ncand=0)[0] == _lib.E_ARG
    many = np.repeat(cands, 4097)
    assert _spec_call(emu_lib, hdr, rows, many)[0] == _lib.E_ARG
    assert _spec_call(emu_lib, hdr, rows, np.repeat(cands, 4096))[0] == 0
    for field, value, text in (("width", 0, "width"), ("width", 65537, "width"), ("off_len", 1, "off_len"), ("off_len", (1 << 20) + 1, "off_len"),
                               ("dm", -1.0, "DM"), ("dm", 1.0e5, "DM"), ("dm", np.nan, "DM")):
        c = cands.copy()
        c[field] = value
        code, msg = _spec_call(emu_lib, hdr, rows, c)
        assert code == _lib.E_ARG and text in msg, (field, value, msg)
        assert emu_lib.frbch_burstspec_kernel(C.byref(rc.desc_of(hdr, rows)), rows.ctypes.data, rows.shape[0], C.byref(rc.burst_par()),
                                              c.ctypes.data, 1) == _lib.E_ARG
    c = cands.copy()
    c["dm"] = 9.0e4                                               # 8 .. 40 MHz: the delay across the band passes 2^30 samples
    code, msg = _spec_call(emu_lib, dict(rc.make_hdr(64, ftop=40.0), nbits=8), rows, c)
    assert code == _lib.E_ARG and "2^30" in msg
    # ncand * nchan > 2^26: 4096 candidates of 16385 channels (nothing is read before the refusal)
    wide = dict(hdr, nchans=16385)
    d = post.fil_desc(dict(wide, nifs=4, nbits=8))
    err = C.create_string_buffer(256)
    code = emu_lib.frbch_burstspec_host(C.byref(d), rows.ctypes.data, 1 << 20, C.byref(rc.burst_par()), np.repeat(cands, 4096).ctypes.data, 4096,
                                        None, 0, None, None, None, None, None, err, len(err))
    assert code == _lib.E_ARG and b"2^26" in err.value
    # ncand * nifs > 65535: 4096 candidates of a 16-product file
    code, msg = _spec_call(emu_lib, dict(hdr, nifs=16), np.zeros((8, 16, 64), np.uint8), np.repeat(cands, 4096))
    assert code == _lib.E_ARG and "65535" in msg
    # coherency products need four of them; the composite needs four in any order
    two = np.ascontiguousarray(rows[:, :2])
    assert _spec_call(emu_lib, dict(hdr, nifs=2), two, cands, par=rc.burst_par(True))[0] == _lib.E_ARG
    assert _spec_call(emu_lib, dict(hdr, nifs=2), two, cands)[0] == 0
    with pytest.raises(post.InputError, match="nifs = 4"):
        post.burst_rm(two, dict(hdr, nifs=2), cands, lib=emu_lib, **rc.GRID)


def _rm_call(lib, hdr, ncand=1, size=None, **grid):
    g = dict(rc.GRID, **grid)
    par = post.rm_params(**g)
    if size is not None:
        par.size = size
    nchan = hdr["nchans"]
    q = np.ones((max(ncand, 1), nchan), np.float32)
    used = np.ones((max(ncand, 1), nchan), np.uint8)
    nphi = min(int(g["nphi"]), 1 << 12) if 0 < g["nphi"] else 1
    F = np.zeros((max(ncand, 1), nphi, 2), np.float32)
    err = C.create_string_buffer(256)
    code = lib.frbch_rmsynth_kernel(C.byref(post.fil_desc(hdr)), F.ctypes.data, ncand, C.byref(par), None)
    if code >= 0:
        return code, ""
    code2 = lib.frbch_rmsynth_host(C.byref(post.fil_desc(hdr)), q.ctypes.data, q.ctypes.data, used.ctypes.data, ncand, C.byref(par), 0,
                                   F.ctypes.data, None, err, len(err))
    assert code2 == code
    res = np.zeros(max(ncand, 1), dtype=post.RM_RESULT)
    assert lib.frbch_rm_peaks(C.byref(post.fil_desc(hdr)), F.ctypes.data, used.ctypes.data, None, None, ncand, C.byref(par), res.ctypes.data,
                              err, len(err)) == code
    return code, err.value.decode()


def test_rmsynth_refusals(emu_lib):
    hdr = rc.make_hdr(64)
    assert _rm_call(emu_lib, hdr)[0] == 0
    assert _rm_call(emu_lib, hdr, nphi=1 << 20, dphi=1.0)[0] == 0
    for kw, text in ((dict(size=8), "wrong size"), (dict(nphi=0), "nphi"), (dict(nphi=(1 << 20) + 1), "nphi"), (dict(ncand=0), "candidates"),
                     (dict(ncand=4097), "candidates"), (dict(ncand=65, nphi=1 << 20, dphi=1.0), "2^26"), (dict(dphi=0.0), "dphi"),
                     (dict(dphi=-1.0), "dphi"), (dict(dphi=np.inf), "dphi"), (dict(dphi=np.nan), "dphi"), (dict(phi_lo=-1.0001e7), "1e7"),
                     (dict(phi_lo=np.nan), "1e7"), (dict(phi_lo=9.99e6, dphi=100.0, nphi=257), "1e7")):
        code, msg = _rm_call(emu_lib, hdr, **kw)
        assert code == _lib.E_ARG and text in msg, (kw, msg)
    assert _rm_call(emu_lib, dict(rc.make_hdr(16384, bw=256.0)))[0] == 0
    code, msg = _rm_call(emu_lib, dict(rc.make_hdr(16384, bw=256.0), nchans=16385))
    assert code == _lib.E_ARG and "16384" in msg
    code, msg = _rm_call(emu_lib, dict(hdr, foff=-30.0))                   # the band runs below 0 MHz
    assert code == _lib.E_ARG and "frequency" in msg


# ---- the known answer -----------------------------------------------------------------------------------------------------
def test_the_oracle_recovers_the_injected_rm():
    """before anything relies on it: the fp64 evaluation of the oracle's own spectra puts its parabola within half a trial step
    of the injected RM, and the integer form differs from it by what the two quantisations allow.  Bound: a phase off by at
    most pi 2^-14 rad moves a term by at most 1.92e-4 of its modulus and the spectra are rounded to 2^-23 of their largest
    value, so |F_int - F_fp64| <= (1.92e-4 + 2^-23 sqrt 2) mean|p| + float32 rounding of F, about 2.0e-4 max|p|; the rounding
    errors of the channels are not aligned, so the measured value is far smaller."""
    k = rc.known_oracle()
    _hdr, _rows, _cands, (nphi, phi_lo, dphi) = rc.known_case()
    for i, rm in enumerate(rc.KNOWN_RMS):
        assert abs(k["fit"][i][0] - rm) <= 0.5 * dphi, (k["fit"][i], rm, dphi)
        assert k["fit"][i][2] == 1 and 0 < k["k0"][i] < nphi - 1
        assert k["results"]["snr"][i] > 20
    print("measured delta = %.3e, rm tolerances %s rad/m2, dphi = %.4f, nphi = %d" % (k["delta"], k["tol"], dphi, nphi))
    assert 0 < k["delta"] < 2.0e-4


def test_known_answer(emu_lib):
    hdr, rows, cands, (nphi, phi_lo, dphi) = rc.known_case()
    k = rc.known_oracle()
    got = post.burst_rm(rows, hdr, cands, nphi, phi_lo, dphi, lib=emu_lib)
    assert np.ascontiguousarray(got["F"]).view(np.float32).tobytes() == k["F"].tobytes()
    for i in range(2):
        r = got["results"][i]
        print("burst %d: rm %.4f (fp64 parabola %.4f, injected %.1f), tolerance %.3e" % (i, r["rm"], k["fit"][i][0], rc.KNOWN_RMS[i], k["tol"][i]))
        assert int(r["kpeak"]) == k["k0"][i] and int(r["fitted"]) == 1
        assert abs(float(r["rm"]) - k["fit"][i][0]) <= k["tol"][i]
        assert abs(float(r["rm"]) - rc.KNOWN_RMS[i]) <= 0.5 * dphi + k["tol"][i]
        assert abs(float(r["rm"]) - rc.KNOWN_RMS[i]) <= 3 * float(r["rm_err"]) + 0.05 * dphi


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_rmsynth_fil_end_to_end(emu_lib, tmp_path, capsys, monkeypatch):
    from tests.test_fold_predictor import write_fil
    hdr, rows, cands, (nphi, phi_lo, dphi) = rc.known_case()
    fil = str(tmp_path / "burst.fil")
    write_fil(fil, rows, hdr, 4)
    bursts = [(float(c["dm"]), int(c["sample"]), int(c["width"])) for c in cands]
    info = {}
    files, res = post.rmsynth_fil(fil, bursts, off_gap=32, off_len=400, lib=emu_lib, info=info)
    base = fil.replace(".fil", "")
    assert files[:2] == [base + "_rm.npz", base + "_rm.txt"] and all(os.path.getsize(f) > 0 for f in files) and len(files) == 4
    assert (info["nphi"], info["phi_lo"], info["dphi"]) == (nphi, phi_lo, dphi)
    k = rc.known_oracle()
    back = np.load(files[0])
    assert back["results"].tobytes() == res.tobytes() and rc.same_results(res, k["results"])
    assert back["F"].view(np.float32).tobytes() == k["F"].tobytes() and back["spec"].tobytes() == k["spec"].tobytes()
    assert back["used"].tobytes() == k["used"].tobytes() and back["noise"].tobytes() == k["noise"].tobytes()
    assert back["phi"].shape == (nphi,) and back["phi"][(nphi - 1) // 2] == 0.0 and back["bursts"].tobytes() == cands.tobytes()
    assert (back["rmsf"][:, (nphi - 1) // 2] == 1.0).all()
    lines = open(files[1]).read().splitlines()
    assert len(lines) == 2 and lines[0].startswith("burst0") and "RM +3" in lines[0] and "RM -1" in lines[1]
    li = float(lines[0].split("L/I")[1].split()[0])
    vi = float(lines[0].split("V/I")[1].split()[0])
    assert abs(li - 0.9) < 0.05 and abs(vi - 0.1) < 0.03
    # the command line: the same files; a flag file takes channels out; the searched form finds both bursts itself
    monkeypatch.setattr(_lib, "load", lambda path=None: emu_lib)
    flagf = str(tmp_path / "x.flag")
    post.write_flag_file(flagf, np.arange(1024) < 40)
    args = ["rmsynth", fil, "--off-gap", "32", "--off-len", "400", "--width", "8"]
    for dm, s, _w in bursts:
        args += ["--dm", str(dm), "--sample", str(s)]
    assert post.main(args) == 0
    out = capsys.readouterr().out
    assert "RM +3" in out and np.load(files[0])["results"].tobytes() == res.tobytes()
    assert post.main(args + ["--flag", flagf, "--nphi", "2001", "--dphi", "2.0"]) == 0
    back = np.load(files[0])
    assert not back["used"][:, :40].any() and back["used"][:, 40:].all() and back["phi"].size == 2001
    assert abs(back["results"]["rm"][0] - 350.0) < 2.0 and abs(back["results"]["rm"][1] + 1200.0) < 2.0
    assert post.main(["rmsynth", fil, "--dm", "40", "--dm2", "60", "--dmstep", "10", "--off-gap", "32", "--off-len", "400", "--width", "8"]) == 0
    found = sorted(np.load(files[0])["results"]["rm"].tolist())
    assert len(found) == 2 and abs(found[0] + 1200.0) < dphi and abs(found[1] - 350.0) < dphi
    with pytest.raises(post.InputError):
        post.main(["rmsynth", fil, "--dm", "50", "--width", "8"])


# ---- rows past a mark: the builder of tests/test_gpu_rm.py's 4 GiB case at marks of 2^20 / 2^21 bytes --------------------
def test_a_burst_beyond_the_mark_on_the_emulator(emu_lib):
    from tests import big_rows as bg
    br = bg.small("A8")
    assert (br.byte_mark_rows[-1] + 20) * br.row_bytes > 1 << 21
    rc.check_beyond_the_mark(emu_lib, br, bg.mem_for(emu_lib), behind=20, off_len=40, kernels=((0, 0, 0), (4, 0, 0)))
