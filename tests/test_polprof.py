"""CPU tests of the polarisation profile (frbch_polprof_*) through the emulator build, which runs the generic kernel: acc, hits,
the bins and the results byte for byte against the numpy restatement tests/polprof_oracle.py (pa, which goes through libm's
atan2, to 1e-12), every refusal with its message and untouched outputs, the int64 bound at full scale, the analytic accuracy
bound against a plain fp64 evaluation, consistency with the RM transform, a PA swing recovered, `post polprof` and `post
rmsynth --profile` end to end, and a walk of failing device-layer calls."""
import ctypes as C
import os

import numpy as np
import pytest

from frb_baseband_amd import _lib, post
from tests import polprof_cases as pc
from tests import polprof_oracle as ppo
from tests import rm_cases as rc
from tests import rm_oracle as ro


def profile_of(lib, c, info=None, **kw):
    a = dict(nbin=c["nbin"], tfactor=c["tfactor"], ref=c["ref"], gains=c["gain"], flag=c["flag"], products="coherency" if c["coh"] else "stokes")
    a.update(kw)
    return post.pol_profile(c["rows"], c["hdr"], c["cands"], a.pop("rm", c["rm"]), lib=lib, info=info, **a)


# ---- the library against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_profile_equals_the_oracle(emu_lib, name):
    c, want = pc.case(name), pc.want(name)
    info = {}
    got = profile_of(emu_lib, c, info)
    assert info == dict(spectra_kernel_used=0, kernel_used=0)
    assert pc.same(got, want), name
    assert pc.query(emu_lib, c, c["rows"].ctypes.data) == 0
    # the _device twin (the emulator's device memory is host memory) writes the same bytes into outputs that held something else
    code, msg, out, k = pc.call(emu_lib.frbch_polprof_device, c, c["rows"].ctypes.data,
                                out=pc.outputs(c["cands"].size, c["nbin"], c["hdr"]["nchans"], fill=0xA5))
    assert code == 0 and k == (0, 0), msg
    for f in out:
        assert out[f].tobytes() == np.ascontiguousarray(got[f]).tobytes(), (name, f)


def test_the_cases_reach_their_edges():
    """the restatement alone: what each case is there for"""
    w = pc.want("u8_64ch_33x3")                                     # a dead candidate between two live ones
    assert w["results"]["nused"].tolist() == [64, 0, 64] and not w["hits"][1].any() and not w["acc"][1].any()
    assert not w["bins"][1].view(np.uint8).any() and w["results"]["k"][1] == 0
    assert (w["hits"][[0, 2]] == 64 * 3).all() and w["bins"]["pa_valid"][0].any() and w["bins"]["pa_valid"][2].any()
    on = w["results"][0]
    assert (on["on_lo_bin"], on["on_hi_bin"]) == (15, 16) and w["bins"]["i"][0, 16] > 20 * on["sigma_i"]
    w = pc.want("u8_64ch_256x1")                                    # B_EDGE: bins in front of row 0; B_END: behind the last row
    assert 0 < w["hits"][0, 0] < w["hits"][0, 20] < 64 and w["hits"][0, 38:].min() == 64          # (the delayed channels reach row 0 first)
    # (B_END's on-pulse rows leave the file in the delayed channels, which are unused for that)
    assert 0 < w["hits"][1, 150] < w["hits"][1, 0] == w["results"]["nused"][1] < 64 and not w["hits"][1, -10:].any()
    assert not w["bins"][1, -10:].view(np.uint8).any()
    w = pc.want("u8_64ch_1024x2")
    assert not w["hits"][1, :400].any() and (w["hits"][0] == 128).all()
    w = pc.want("u8_64ch_8x512")
    assert (w["hits"] == 64 * 512).all()
    w = pc.want("u8_96ch_ascending")                                # B_OUT last: wholly outside
    assert not w["hits"][2].any() and w["results"]["nused"].tolist() == [96, 96, 0]
    assert pc.case("u8_96ch_ascending")["hdr"]["foff"] > 0
    w = pc.want("u8_1024ch_late")
    assert ro.delays(pc.case("u8_1024ch_late")["hdr"], rc.B_LATE["dm"]).max() > 3000 and w["hits"][2].min() > 0
    w = pc.want("u8_64ch_flag_gain")                                # flags 0, 17, 63; gains: -1.5 at [1][7], 0 at [2][9], inf at [3][11]
    assert not w["used"][:, [0, 17, 63, 11]].any() and w["used"][:, [7, 9]].all() and w["results"]["nused"].tolist() == [60, 60]
    w = pc.want("u16_64ch_coherency")
    assert w["results"]["nused"].tolist() == [63, 63, 63] and w["results"]["k"][0] == 5          # 2^16 x a largest gain in (1, 2): e = 17
    for name in pc.CASES:                                           # rm = 0, 900, -2500 and 1e7; both references
        assert set(pc.case(name)["rm"].tolist()) <= {0.0, 900.0, -2500.0, 1.0e7}
    assert {pc.case(n)["ref"] for n in pc.CASES} == {"mean", "zero"}
    assert {(pc.case(n)["nbin"], pc.case(n)["tfactor"]) for n in pc.CASES} >= {(1, 1), (2, 7), (33, 3), (256, 1), (1024, 2), (8, 512)}


def test_the_reference_wavelength_turns_the_pa_and_nothing_else(emu_lib):
    c = pc.case("u8_64ch_33x3")
    a, b = profile_of(emu_lib, c, ref="mean"), profile_of(emu_lib, c, ref="zero")
    assert a["acc"][..., [0, 3]].tobytes() == b["acc"][..., [0, 3]].tobytes() and a["hits"].tobytes() == b["hits"].tobytes()
    assert b["results"]["lref"].tolist() == [0.0, 0.0, 0.0] and abs(a["results"]["lref"][0] - ro.lambda2(c["hdr"]).mean()) < 1e-15
    j = 16
    turn = 900.0 * a["results"]["lref"][0]
    diff = (b["bins"]["pa"][0, j] - a["bins"]["pa"][0, j] + turn + np.pi / 2) % np.pi - np.pi / 2
    assert abs(diff) < 1e-3 and abs(a["bins"]["l"][0, j] - b["bins"]["l"][0, j]) < 1e-3 * a["bins"]["l"][0, j]
    assert abs(((a["bins"]["pa"][0, j] - rc.B1["pa0"] - turn + np.pi / 2) % np.pi) - np.pi / 2) < 0.05


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(emu_lib):
    c = pc.case("u8_64ch_33x3")
    hdr, rows, ptr = c["hdr"], c["rows"], c["rows"].ctypes.data
    host = emu_lib.frbch_polprof_host

    def par(**kw):
        p = pc.par_of(c)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def cand(field, value):
        cc = c["cands"].copy()
        cc[field] = value
        return dict(c, cands=cc)

    def rm(i, value):
        r = c["rm"].copy()
        r[i] = value
        return r

    assert pc.call(host, c, ptr)[0] == 0
    many = dict(c, cands=np.repeat(c["cands"][:1], 4097), rm=np.zeros(4097))
    refused = [
        (dict(par=par(size=16)), "frbch_prof_params: wrong size"), (dict(par=par(nbin=0)), "nbin"), (dict(par=par(nbin=1025)), "nbin"),
        (dict(par=par(tfactor=0)), "tfactor"), (dict(par=par(tfactor=513)), "tfactor"), (dict(par=par(ref=2)), "ref"),
        (dict(hdr=dict(hdr, nifs=2)), "nifs = 4"), (dict(hdr=dict(hdr, nbits=32)), "not built for float32"),
        (dict(hdr=dict(hdr, nchans=16385)), "16384"), (dict(ncand=0), "candidates"), (dict(c=many), "candidates"),
        (dict(rm=rm(1, np.nan)), "rm"), (dict(rm=rm(2, np.inf)), "rm"), (dict(rm=rm(0, -1.0001e7)), "rm"), (dict(rm=False), "null argument"),
        (dict(c=cand("width", 0)), "width"), (dict(c=cand("off_len", 1)), "off_len"), (dict(c=cand("dm", -1.0)), "DM"),
        (dict(bpar=rc.burst_par(size=4)), "frbch_burst_params: wrong size"), (dict(hdr=dict(hdr, foff=-30.0)), "frequency"),
    ]
    for kw, text in refused:
        cc = kw.pop("c", c)
        n = cc["cands"].size if "ncand" not in kw else 1
        out = pc.outputs(n, c["nbin"], 16385 if kw.get("hdr", hdr)["nchans"] > 64 else 64, fill=0xA5)
        code, msg, out, _k = pc.call(host, cc, ptr, out=out, **kw)
        assert code == _lib.E_ARG and text in msg, (kw, msg)
        assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), kw
        code2 = pc.call(emu_lib.frbch_polprof_device, cc, ptr, out=out, **kw)[0]
        assert code2 == _lib.E_ARG and all((a.view(np.uint8) == 0xA5).all() for a in out.values()), kw
    # the plan query refuses the same (it takes no rm) and a null pointer
    assert pc.query(emu_lib, c, ptr, par=par(nbin=1025)) == _lib.E_ARG and pc.query(emu_lib, c, None) == _lib.E_ARG
    assert pc.query(emu_lib, cand("dm", np.nan), ptr) == _lib.E_ARG
    # the largest batch passes the checks: 4096 candidates x 1024 bins = 2^22 (the query runs nothing)
    assert pc.query(emu_lib, dict(c, cands=np.repeat(c["cands"][:1], 4096)), ptr, par=par(nbin=1024)) == 0
    assert pc.call(host, c, ptr, rm=rm(0, 1.0e7))[0] == 0 and pc.call(host, c, ptr, rm=rm(0, -1.0e7))[0] == 0
    with pytest.raises(post.InputError, match="float32"):
        post.pol_profile(rows.astype(np.float32), dict(hdr, nbits=32), c["cands"], c["rm"], lib=emu_lib)
    with pytest.raises(post.InputError, match="ref"):
        post.pol_profile(rows, hdr, c["cands"], c["rm"], ref="middle", lib=emu_lib)


# ---- the int64 bound --------------------------------------------------------------------------------------------------
def test_the_int64_bound(emu_lib):
    """16384 channels x 16 bit, every channel at +full scale over its baseline, tfactor 512, rm 0 (C = 2^22): the restatement adds
    the terms up in Python integers and stays below 2^62; int64 numpy and the library agree with it to the bit"""
    c, want = pc.bound_case(), pc.bound_want()
    assert want["largest"] == 16384 * 2097120 * (1 << 22) and (1 << 56) < want["largest"] < (1 << 62)
    assert int(want["acc"][0, 0, 1]) == want["largest"] and want["results"]["k"][0] == -4 and (want["hits"] == 16384 * 512).all()
    assert want["bins"]["q"][0, 0] == 65535.0 * 2097120 * 16 / (512 * 65535)
    got = profile_of(emu_lib, c)
    assert pc.same(got, want)


# ---- accuracy: the restatement against the plain fp64 evaluation ----------------------------------------------------------
def accuracy_ratios(want, fp):
    """-> the largest |error| / bound over the live bins, for (Q, U) and for (I, V); asserts nothing"""
    worst_qu, worst_iv = 0.0, 0.0
    for i in np.flatnonzero(fp["live"]):
        ok = fp["hits"][i] > 0
        assert np.array_equal(fp["hits"][i], want["hits"][i])
        h = fp["hits"][i][ok].astype(np.float64)
        unit = float(fp["N"][i]) * 2.0 ** -float(fp["k"][i])
        b_qu = (1.93e-4 * fp["absqu"][i][ok] + unit) / h
        b_iv = unit / h
        bins = want["bins"][i][ok]
        worst_qu = max(worst_qu, float((np.abs(bins["q"] - fp["Q"][i][ok]) / b_qu).max()), float((np.abs(bins["u"] - fp["U"][i][ok]) / b_qu).max()))
        worst_iv = max(worst_iv, float((np.abs(bins["i"] - fp["I"][i][ok]) / b_iv).max()), float((np.abs(bins["v"] - fp["V"][i][ok]) / b_iv).max()))
    return worst_qu, worst_iv


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_the_integer_form_stays_within_its_bound(name):
    """For every live bin |Q - Q_fp64| and |U - U_fp64| <= (1.93e-4 sum over used c of (|xQ| + |xU|) + N 2^-k) / hits: the phase is
    off by at most half a table step (2 pi 2^-15 = 1.92e-4 rad), the table entries by 2^-23 of a unit, and every X by half a
    unit, with |C| + |S| <= sqrt 2 units per channel; I and V: N 2^-k / hits (half a unit per channel, at most).  Measured
    (largest error / bound over all cases): 0.20 for (Q, U) -- the phase errors of the channels are not aligned --, 0.16 for
    (I, V)."""
    qu, iv = accuracy_ratios(pc.want(name), pc.want_fp64(name))
    print("%s: largest error / bound: (Q, U) %.4f, (I, V) %.4f" % (name, qu, iv))
    assert qu <= 1.0 and iv <= 1.0


# ---- consistency with the RM transform ---------------------------------------------------------------------------------
def test_one_bin_on_the_pulse_equals_the_transform_at_that_trial(emu_lib):
    """nbin = 1, tfactor = width, the bin laid on the on-pulse rows, ref = mean, rm = trial 137 of the grid (900 rad m^-2): (Q, U)
    is F at that trial of the per-channel spectra x / width.  Tolerance: the analytic bound of the profile, the RM stage's own
    quantisation ((1.92e-4 + 2^-22) of the largest |q| + |u|, and 2^-23 of |F| for the float32 F) and 2^-24 of the mean |q| + |u|
    for the float32 spectra; the two fp64 evaluations agree far closer."""
    hdr, rows, _cands, _coh = rc.case("u8_64ch")
    w = rc.B1["width"]
    on_lo = rc.B1["sample"] - w // 2
    cands = post.burst_cands([(rc.B1["dm"], on_lo, w)], 16, 200)         # nbin = 1: t0 = sample
    k = 137
    rm = rc.GRID["phi_lo"] + k * rc.GRID["dphi"]
    assert rm == 900.0
    fp = ppo.profile_fp64(rows, hdr, cands, [rm], 1, w, "mean")
    assert fp["hits"][0, 0] == 64 * w and fp["used"].all()
    q, u = (fp["xq"][0, :, 0] / w).astype(np.float32), (fp["xu"][0, :, 0] / w).astype(np.float32)
    F, _re, _im = ro.transform(q[None], u[None], fp["used"], hdr, **rc.GRID)
    F64 = ro.transform_fp64(q[None], u[None], fp["used"], hdr, **rc.GRID)[0, k]
    got = post.pol_profile(rows, hdr, cands, [rm], nbin=1, tfactor=w, ref="mean", lib=emu_lib)
    b = got["bins"][0, 0]
    amp = np.abs(q.astype(np.float64)) + np.abs(u.astype(np.float64))
    b_prof = (1.93e-4 * fp["absqu"][0, 0] + 64 * 2.0 ** -float(fp["k"][0])) / (64 * w)
    b_rm = (1.92e-4 + 2.0 ** -22) * amp.max() + 2.0 ** -23 * abs(F64)
    b_f32 = 2.0 ** -24 * amp.mean()
    assert abs(fp["Q"][0, 0] - F64.real) <= b_f32 and abs(fp["U"][0, 0] - F64.imag) <= b_f32
    assert abs(F[0, k, 0] - F64.real) <= b_rm and abs(F[0, k, 1] - F64.imag) <= b_rm
    print("Q %.6f U %.6f, F %.6f %+.6fi, tolerance %.3e" % (b["q"], b["u"], F[0, k, 0], F[0, k, 1], b_prof + b_rm + b_f32))
    assert abs(b["q"] - float(F[0, k, 0])) <= b_prof + b_rm + b_f32 and abs(b["u"] - float(F[0, k, 1])) <= b_prof + b_rm + b_f32
    assert abs(F64) > 30 and abs(b["l"] - abs(F64)) < 1e-3 * abs(F64)


# ---- the known answer -------------------------------------------------------------------------------------------------
def test_the_oracle_recovers_the_injected_swing():
    """before anything relies on it: the restatement alone, on the seed of the case"""
    c, injected = pc.known_case()
    w = ppo.profile(*pc.oracle_args(c))
    assert pc.check_known(w["bins"][0], w["results"][0], injected) == pc.KNOWN_WIDTH
    r = w["results"][0]
    assert (r["on_lo_bin"], r["on_hi_bin"], r["nused"], r["lref"]) == (12, 51, 1024, 0.0)


def test_known_answer(emu_lib):
    c, injected = pc.known_case()
    got = profile_of(emu_lib, c)
    assert pc.same(got, ppo.profile(*pc.oracle_args(c)))
    assert pc.check_known(got["bins"][0], got["results"][0], injected) == pc.KNOWN_WIDTH
    swing = np.degrees(got["bins"]["pa"][0, 51] - got["bins"]["pa"][0, 12])
    assert abs(swing - 60.0) < 1.0
    flat = profile_of(emu_lib, c, rm=[0.0])                          # not derotated: the band depolarises itself
    assert flat["bins"]["l_db"][0].sum() < 0.2 * got["bins"]["l_db"][0].sum()
    assert flat["acc"][..., [0, 3]].tobytes() == got["acc"][..., [0, 3]].tobytes()


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_polprof_and_rmsynth_profile_end_to_end(emu_lib, tmp_path, capsys, monkeypatch):
    from tests.test_fold_predictor import write_fil
    c, _injected = pc.known_case()
    hdr, rows, cands = c["hdr"], c["rows"], c["cands"]
    fil = str(tmp_path / "swing.fil")
    write_fil(fil, rows, hdr, 4)
    base = fil.replace(".fil", "")
    bursts = [(float(cands[0]["dm"]), int(cands[0]["sample"]), int(cands[0]["width"]))]
    info = {}
    files, prof = post.polprof_fil(fil, bursts, rm=pc.KNOWN_RM, nbin=64, tfactor=1, ref="zero", off_gap=32, off_len=400, lib=emu_lib, info=info)
    assert files == [base + "_polprof.npz", base + "_polprof.txt", base + "_polprof_burst0.png"] and all(os.path.getsize(f) > 0 for f in files)
    assert info["kernel_used"] == 0
    want = profile_of(emu_lib, c)
    back = np.load(files[0])
    for f in ("acc", "hits", "bins", "results", "used"):
        assert back[f].tobytes() == want[f].tobytes() == prof[f].tobytes(), f
    assert back["bursts"].tobytes() == cands.tobytes() and back["rm"].tolist() == [pc.KNOWN_RM] and int(back["tfactor"]) == 1
    lines = open(files[1]).read().splitlines()
    assert lines[0].startswith("# burst0") and "RM +350.000" in lines[0] and len(lines) == 65
    table = np.array([[float(v) for v in ln.split()] for ln in lines[1:]])
    assert table.shape == (64, 6)
    valid = want["bins"]["pa_valid"][0] != 0
    assert np.array_equal(np.isnan(table[:, 4]), ~valid) and np.array_equal(np.isnan(table[:, 5]), ~valid)
    assert np.allclose(table[valid, 4], np.degrees(want["bins"]["pa"][0][valid]), atol=1e-3)
    assert np.allclose(table[:, 1], want["bins"]["i"][0], rtol=1e-5, atol=1e-9)
    assert np.allclose(table[:, 0], (2000 - 32 + np.arange(64) + 0.5) * hdr["tsamp"], atol=1e-9)
    assert (np.abs(table[valid, 4]) <= 90.0).all()
    # rmsynth: without --profile its present files, with it the profile files as well, and the same _rm.npz either way
    plain, res = post.rmsynth_fil(fil, bursts, off_gap=32, off_len=400, lib=emu_lib)
    assert plain == [base + "_rm.npz", base + "_rm.txt", base + "_rm_burst0.png"]
    rm_arrays = {k: v.tobytes() for k, v in np.load(plain[0]).items()}
    rm_txt = open(plain[1]).read()
    for f in files:
        os.remove(f)
    both, res2 = post.rmsynth_fil(fil, bursts, off_gap=32, off_len=400, lib=emu_lib, profile=True, nbin=64, tfactor=1)
    assert both == plain + files and res2.tobytes() == res.tobytes() and open(plain[1]).read() == rm_txt
    assert {k: v.tobytes() for k, v in np.load(plain[0]).items()} == rm_arrays
    back = np.load(files[0])
    fitted = profile_of(emu_lib, c, rm=res["rm"], ref="mean")
    assert back["bins"].tobytes() == fitted["bins"].tobytes() and back["rm"].tobytes() == res["rm"].tobytes()
    assert abs(res["rm"][0] - pc.KNOWN_RM) < 5.0 and back["bins"]["pa_valid"][0, 12:52].all()
    # the command line
    monkeypatch.setattr(_lib, "load", lambda path=None: emu_lib)
    for f in files:
        os.remove(f)
    args = ["polprof", fil, "--dm", "50", "--sample", "2000", "--width", "40", "--rm", "350", "--nbin", "64", "--ref", "zero", "--off-gap", "32",
            "--off-len", "400"]
    assert post.main(args) == 0
    assert "wrote " + files[0] in capsys.readouterr().out and np.load(files[0])["bins"].tobytes() == want["bins"].tobytes()
    assert post.main(["polprof", fil, "--rm-from", plain[0], "--nbin", "64"]) == 0
    assert np.load(files[0])["bins"].tobytes() == fitted["bins"].tobytes()
    assert post.main(["rmsynth", fil, "--dm", "50", "--sample", "2000", "--width", "40", "--off-gap", "32", "--off-len", "400", "--profile", "--nbin", "64"]) == 0
    out = capsys.readouterr().out
    assert all("wrote " + f in out for f in both) and np.load(files[0])["bins"].tobytes() == fitted["bins"].tobytes()
    with pytest.raises(post.InputError):
        post.main(["polprof", fil, "--dm", "50", "--sample", "2000", "--width", "40"])


# ---- failing device-layer calls ---------------------------------------------------------------------------------------
def test_a_failing_device_call_returns_the_error_and_leaves_nothing_behind(emu_lib):
    """every fallible device-layer call of frbch_polprof_host fails once (n = 1, 2, ... until the call succeeds): an error with a
    message comes back, the outputs are untouched, the blocks and streams alive afterwards are those alive before, and a plain
    call right afterwards writes the expected bytes"""
    emu_lib.frbch_test_emu_fail_at.argtypes, emu_lib.frbch_test_emu_fail_at.restype = [C.c_long], None
    emu_lib.frbch_test_emu_live.argtypes, emu_lib.frbch_test_emu_live.restype = [], C.c_uint64
    c, want = pc.case("u8_64ch_33x3"), pc.want("u8_64ch_33x3")
    ptr = c["rows"].ctypes.data
    rows0 = c["rows"].tobytes()
    codes = []
    for n in range(1, 200):
        out = pc.outputs(3, c["nbin"], 64, fill=0xA5)
        before = emu_lib.frbch_test_emu_live()
        emu_lib.frbch_test_emu_fail_at(n)
        try:
            code, msg, out, _k = pc.call(emu_lib.frbch_polprof_host, c, ptr, out=out)
        finally:
            emu_lib.frbch_test_emu_fail_at(0)
        assert emu_lib.frbch_test_emu_live() == before, n
        if code == 0:
            assert pc.same(out, want)
            break
        codes.append(code)
        assert code in (_lib.E_DEVICE, _lib.E_NOMEM) and msg, (n, code, msg)
        assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), n
        again = pc.call(emu_lib.frbch_polprof_host, c, ptr)
        assert again[0] == 0 and pc.same(again[2], want), n
    assert 15 < len(codes) < 199 and c["rows"].tobytes() == rows0
