"""The periodicity test of the interference stage (frbch_rfi_peaks_*, frbch_rfi_periodic, frbch_rfi_cleanf_*, post.rfi_peaks /
rfi_periodic / clean(periodic=) / rfifind_fil(periodic=), `post rfifind --periodic`): the numpy restatement
tests/rfi_periodic_oracle.py against numpy.fft, the generic kernel and the host decision through the TEST-ONLY emulator build
against the restatement (every comparison `==` or `tobytes()`), argument errors, failing device calls, the emulator's adversary
schedules, and the Python layer's files."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import _lib, post, sigproc
from tests import rfi_cases as rc
from tests import rfi_oracle as ro
from tests import rfi_periodic_cases as pc
from tests import rfi_periodic_oracle as po
from tests.test_fold_predictor import write_fil
from tests.test_post import DM0, HDR


# ---- the restatement itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 256, 4096])
def test_oracle_against_numpy_fft(n):
    """the normalised peak power of noise cells agrees with a float64 numpy.fft of the same float32 input to 1e-5 relative: the
    float32 rounding of a 12-stage transform (log2 n x 6e-8 x a few) with margin -- a sanity check of the restatement only"""
    rng = np.random.default_rng(n)
    x = (96.0 + 16.0 * rng.standard_normal((n, 32))).astype(np.float32)
    st = ro.stats(x, n)
    pk = po.peaks(x, st, n)
    dec = po.periodic(st, pk, n, n, 1.0, 1.0)
    _n_b, mean, var = po.cell_moments(st, n, n)
    d = (x.astype(np.float64) - mean[0][None, :]).astype(np.float32).astype(np.float64)
    spec = np.abs(np.fft.fft(d, axis=0)[1: n // 2]) ** 2
    want = spec.max(axis=0) / (n * var[0])
    rel = np.abs(dec["power"][0] - want) / want
    print("n = %d: largest relative difference %.2e" % (n, rel.max()))
    assert rel.max() <= 1e-5
    assert np.array_equal(pk["k"][0], 1 + spec.argmax(axis=0))


def test_t_pow_of():
    assert post.t_pow_of(4.0, 256) == po.t_pow_of(4.0, 256) and abs(post.t_pow_of(4.0, 256) - 15.2) < 0.01
    assert post.t_pow_of(4.0, 1024) > post.t_pow_of(4.0, 256) > post.t_pow_of(3.0, 256) > 0


# ---- the generic kernel through the emulator ---------------------------------------------------------------------------------
@pytest.mark.parametrize("g", pc.grid(), ids=pc.grid_id)
def test_emulator_equals_the_restatement(emu_lib, g):
    """n in 8, 64, 256, 4096 x 33 / 48 / 64 channels x 8 / 16 / 32 bits x (one product, the last of three), nrows around a
    multiple of n: peaks and bins, the statistics beside them, and the decision on them"""
    nchan, nbits, nifs, prod, n, nrows = g
    rows, st, pk = pc.rows_case(*g)
    par = rc.params(block_rows=n)
    assert emu_lib.frbch_rfi_peaks_kernel(C.byref(rc.desc_of(rows, prod)), C.c_void_p(rows.ctypes.data), nrows, C.byref(par)) == pc.GENERIC
    code, got, got_st, used, msg = pc.peaks_host(emu_lib, rows, prod, par)
    assert code == 0 and used == (rc.GENERIC, pc.GENERIC), msg
    assert got_st.tobytes() == st.tobytes() and pc.same_peaks(got, pk)
    last = nrows - (st.shape[0] - 1) * n
    assert np.all(got["k"][-1] > 0) == (2 * last >= n) and (2 * last >= n or not got["num"][-1].any())
    want = po.periodic(st, pk, nrows, n, 6.0, 0.4)
    code, dec, msg = pc.periodic_call(emu_lib, got_st, got, nrows, nifs, nbits, prod, par, pc.fparams(6.0, 0.4))
    assert code == 0, msg
    assert np.array_equal(dec["pflag"], want["pflag"]) and np.array_equal(dec["pchan"], want["pchan"])
    assert dec["power"].tobytes() == want["power"].tobytes()
    code, alone, _st, _used, msg = pc.peaks_host(emu_lib, rows, prod, par, want_stats=False)
    assert code == 0 and pc.same_peaks(alone, pk), msg


def test_the_grid_has_tested_and_untested_last_blocks_and_flags_something():
    last = [(g[5] - (-(-g[5] // g[4]) - 1) * g[4]) * 2 >= g[4] for g in pc.grid()]
    assert any(last) and not all(last)
    frac = [float(po.periodic(pc.rows_case(*g)[1], pc.rows_case(*g)[2], g[5], g[4], 6.0, 0.4)["pflag"].mean()) for g in pc.grid()[::5]]
    assert any(0.0 < f < 1.0 for f in frac)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_bad_channel_does_not_reach_its_partner(emu_lib, bad):
    """float rows with a NaN / an Inf in channel 5 of block 1: its cell gives {0, 0}, and channel 4 -- its partner in the
    transform -- the peaks of channel 4 alone (those of the same rows with channel 5 finite)"""
    rng = np.random.default_rng(7)
    rows = (10.0 + rng.standard_normal((64 * 6, 1, 48))).astype(np.float32)
    good = rows.copy()
    rows[70, 0, 5] = bad
    par = rc.params(block_rows=64)
    code, pk, st, _used, msg = pc.peaks_host(emu_lib, rows, 0, par)
    assert code == 0, msg
    want = po.peaks(rows[:, 0], ro.stats(rows[:, 0], 64), 64)
    assert pc.same_peaks(pk, want)
    assert tuple(pk[1, 5]) == (0.0, 0) and pk["k"][0, 5] > 0 and pk["k"][2, 5] > 0
    clean = po.peaks(good[:, 0], ro.stats(good[:, 0], 64), 64)
    keep = np.ones(pk.shape, bool)
    keep[1, 5] = False
    assert pk[keep].tobytes() == clean[keep].tobytes() and np.isfinite(pk["num"]).all()
    code, dec, msg = pc.periodic_call(emu_lib, st, pk, rows.shape[0], 1, 32, 0, par, pc.fparams(5.0))
    assert code == 0 and dec["power"][1, 5] == 0.0 and dec["pflag"][1, 5] == 0 and np.isfinite(dec["power"]).all(), msg


@pytest.mark.parametrize("nbits,value", [(8, 77), (16, 40000), (32, 2.5)])
def test_a_constant_channel_gives_no_peak(emu_lib, nbits, value):
    rows = rc.make_rows(700, 1, 48, nbits, seed=3)
    rows[:, 0, 10] = value
    rows[256:512, 0, 11] = value                   # and one constant cell beside it (channels 10 and 11 are a pair)
    code, pk, st, _used, msg = pc.peaks_host(emu_lib, rows, 0, rc.params(block_rows=256))
    assert code == 0 and pc.same_peaks(pk, po.peaks(rows[:, 0], ro.stats(rows[:, 0], 256), 256)), msg
    assert not pk["num"][:, 10].any() and not pk["k"][:, 10].any() and tuple(pk[1, 11]) == (0.0, 0) and pk["k"][0, 11] > 0


# ---- the known answer --------------------------------------------------------------------------------------------------------
KA_CELLS = [(b, pc.KA_TONE["channel"]) for b in pc.KA_TONE["blocks"]]


def test_known_answer_of_the_restatement():
    """the cell test on mean and std flags none of the tone's cells; the periodic test exactly those four, at k = 256 / 8"""
    q = pc.known_answer_rows(0)
    st = ro.stats(q, rc.KA_BLOCK)
    time_only = ro.mask(st, q.shape[0], rc.KA_BLOCK, 8, **rc.rule_kw(rc.DEFAULTS))
    assert int(time_only["mask"].sum()) == 0
    pk = po.peaks(q, st, rc.KA_BLOCK)
    dec = po.periodic(st, pk, q.shape[0], rc.KA_BLOCK, pc.ka_t_pow(), 0.3)
    assert [tuple(v) for v in np.argwhere(dec["pflag"]).tolist()] == KA_CELLS and not dec["pchan"].any()
    assert all(int(pk["k"][b, c]) == 32 for b, c in KA_CELLS)
    power = np.array(dec["power"])
    assert all(19.0 < power[b, c] for b, c in KA_CELLS)
    for b, c in KA_CELLS:
        power[b, c] = 0.0
    assert power.max() < 14.0 < pc.ka_t_pow()                    # the noise cells stay well below the threshold


def test_known_answer_through_the_library(emu_lib):
    q = np.ascontiguousarray(pc.known_answer_rows(0)[:, None, :])
    par = rc.params(block_rows=rc.KA_BLOCK)
    code, _out, plain, _used, msg = rc.clean_host(emu_lib, q, 0, par)
    assert code == 0 and int(plain["mask"].sum()) == 0, msg
    want, cleaned = pc.sequence_of_parts(q, 0, rc.KA_BLOCK, 8, rc.rule_kw(rc.DEFAULTS), pc.ka_t_pow(), 0.3)
    code, out, got, used, msg = pc.cleanf_host(emu_lib, q, 0, par, pc.fparams(pc.ka_t_pow()))
    assert code == 0 and used == (rc.GENERIC, pc.GENERIC) and pc.same_cleanf(got, want) and out.tobytes() == cleaned.tobytes(), msg
    assert [tuple(v) for v in np.argwhere(got["mask"]).tolist()] == KA_CELLS
    assert all(int(got["peaks"]["k"][b, c]) == 32 for b, c in KA_CELLS)
    ch = pc.KA_TONE["channel"]
    assert np.all(out[5 * 256: 9 * 256, 0, ch] == got["repl"][ch]) and out[: 5 * 256].tobytes() == q[: 5 * 256].tobytes()


def test_a_tone_in_every_block_flags_its_channel(emu_lib, tmp_path):
    """... wholly, through chan_frac, whatever the across-channel rule makes of it (t_chan = 0: off), and the channel is in
    the flag file"""
    q = np.ascontiguousarray(pc.known_answer_rows(0, True)[:, None, :])
    rule = dict(rc.rule_kw(rc.DEFAULTS), t_chan=0.0)
    st = ro.stats(q[:, 0], rc.KA_BLOCK)
    assert int(ro.mask(st, q.shape[0], rc.KA_BLOCK, 8, **rule)["mask"].sum()) == 0
    want, cleaned = pc.sequence_of_parts(q, 0, rc.KA_BLOCK, 8, rule, pc.ka_t_pow(), 0.3)
    code, out, got, _used, msg = pc.cleanf_host(emu_lib, q, 0, rc.params(block_rows=rc.KA_BLOCK, t_chan=0.0), pc.fparams(pc.ka_t_pow()))
    assert code == 0 and pc.same_cleanf(got, want) and out.tobytes() == cleaned.tobytes(), msg
    assert np.flatnonzero(got["pchan"]).tolist() == [pc.KA_ALL_CHANNEL] == np.flatnonzero(got["chan_flag"]).tolist()
    assert got["mask"][:, pc.KA_ALL_CHANNEL].all() and all(got["mask"][b, c] for b, c in KA_CELLS)
    fil = str(tmp_path / "tone.fil")
    write_fil(fil, q, dict(HDR, nchans=64), 1)
    files, res = post.rfifind_fil(fil, block_rows=rc.KA_BLOCK, t_chan=0.0, periodic=True, lib=emu_lib)
    assert np.flatnonzero(post.read_flag_file(files[1], 64)).tolist() == [pc.KA_ALL_CHANNEL]
    assert np.array_equal(res["mask"], want["mask"]) and np.array_equal(res["pflag"], want["pflag"])


# ---- the composite ---------------------------------------------------------------------------------------------------------
COMPOSITE = [(48, 8, 1, 0, 64, 64 * 5 + 40), (64, 16, 3, 2, 256, 256 * 3 - 1), (33, 32, 3, 1, 8, 8 * 9 + 1)]
COMPOSITE_T_POW = {64: 5.0, 256: 5.0, 8: 2.5}      # (the three bins of n = 8 share a total power of 4: p stays below that)


@pytest.mark.parametrize("c", COMPOSITE, ids=pc.grid_id)
def test_cleanf_is_the_sequence_of_its_parts(emu_lib, c):
    """frbch_rfi_cleanf_host against statistics, peaks, the decision, the mask with `prior` and apply run one by one through
    the library, and against the restatements"""
    nchan, nbits, nifs, prod, n, nrows = c
    rows, st, pk = pc.rows_case(*c)
    par = rc.params(block_rows=n, t_cell=3.0)
    t_pow = COMPOSITE_T_POW[n]
    fpar = pc.fparams(t_pow, 0.5)
    zap = np.zeros(nchan, bool)
    zap[3] = True
    code, got_pk, got_st, _used, msg = pc.peaks_host(emu_lib, rows, prod, par)
    assert code == 0, msg
    code, dec, msg = pc.periodic_call(emu_lib, got_st, got_pk, nrows, nifs, nbits, prod, par, fpar)
    assert code == 0, msg
    code, res, msg = rc.mask_call(emu_lib, got_st, nrows, nchan, nifs, nbits, prod, par, zap=zap, prior=dec["pflag"])
    assert code == 0, msg
    code, parts_rows, msg = rc.apply_host(emu_lib, rows, prod, par, res["mask"], res["repl"])
    assert code == 0, msg
    code, out, got, used, msg = pc.cleanf_host(emu_lib, rows, prod, par, fpar, zap=zap)
    assert code == 0 and used == (rc.GENERIC, pc.GENERIC), msg
    assert out.tobytes() == parts_rows.tobytes() and np.array_equal(got["mask"], res["mask"]) and got["repl"].tobytes() == res["repl"].tobytes()
    assert np.array_equal(got["chan_flag"], res["chan_flag"] | dec["pchan"]) and np.array_equal(got["blk_flag"], res["blk_flag"])
    assert np.array_equal(got["pflag"], dec["pflag"]) and np.array_equal(got["pchan"], dec["pchan"]) and pc.same_peaks(got["peaks"], got_pk)
    assert 0 < int(dec["pflag"].sum()) < dec["pflag"].size
    want, cleaned = pc.sequence_of_parts(rows, prod, n, nbits, dict(rc.rule_kw(rc.DEFAULTS), t_cell=3.0), t_pow, 0.5, zap=zap)
    assert pc.same_cleanf(got, want) and out.tobytes() == cleaned.tobytes()
    code, out2, got2, _used, msg = pc.cleanf_host(emu_lib, rows, prod, par, fpar, zap=zap, want_peaks=False)
    assert code == 0 and out2.tobytes() == out.tobytes() and np.array_equal(got2["pflag"], got["pflag"]), msg


@pytest.mark.parametrize("c", COMPOSITE, ids=pc.grid_id)
def test_a_threshold_out_of_reach_is_clean(emu_lib, c):
    """t_pow = 1e300: rows, mask and repl of frbch_rfi_clean_host, byte for byte"""
    nchan, nbits, nifs, prod, n, nrows = c
    rows, _st, _pk = pc.rows_case(*c)
    par = rc.params(block_rows=n, t_cell=3.0)
    code, out, res, used, msg = rc.clean_host(emu_lib, rows, prod, par)
    assert code == 0, msg
    code, outf, resf, usedf, msg = pc.cleanf_host(emu_lib, rows, prod, par, pc.fparams(1e300))
    assert code == 0 and usedf[0] == used, msg
    assert outf.tobytes() == out.tobytes() and rc.same_result(resf, res) and not resf["pflag"].any() and not resf["pchan"].any()
    assert int(res["mask"].sum()) > 0


# ---- refused arguments -----------------------------------------------------------------------------------------------------
def call_all(lib, rows, nrows, desc, par, fpar):
    """every new entry point on the same arguments -> (codes, messages, the kernel query's answer)"""
    nblk = 5
    st = np.zeros((nblk, 64, 2), np.uint64)
    pk = np.zeros((nblk, 64), pc.PEAK)
    m, repl, cf, bf = np.zeros((nblk, 64), np.uint8), np.zeros(64), np.zeros(64, np.uint8), np.zeros(nblk, np.uint8)
    pflag, pchan = np.zeros((nblk, 64), np.uint8), np.zeros(64, np.uint8)
    used = (C.c_uint32 * 2)(0, 0)
    e = [C.create_string_buffer(256) for _ in range(6)]
    out = rows.copy()
    tail = (m.ctypes.data, repl.ctypes.data, cf.ctypes.data, bf.ctypes.data, pflag.ctypes.data, pchan.ctypes.data, pk.ctypes.data, used)
    codes = [
        lib.frbch_rfi_peaks_host(C.byref(desc), rows.ctypes.data, nrows, C.byref(par), 0, st.ctypes.data, pk.ctypes.data, used, e[0], 256),
        lib.frbch_rfi_peaks_device(C.byref(desc), rows.ctypes.data, nrows, C.byref(par), 0, st.ctypes.data, pk.ctypes.data, used, e[1], 256),
        lib.frbch_rfi_periodic(C.byref(desc), st.ctypes.data, pk.ctypes.data, nblk, nrows, C.byref(par), C.byref(fpar), pflag.ctypes.data,
                               pchan.ctypes.data, None, e[2], 256),
        lib.frbch_rfi_cleanf_host(C.byref(desc), out.ctypes.data, nrows, C.byref(par), C.byref(fpar), None, 0, *tail, e[3], 256),
        lib.frbch_rfi_cleanf_device(C.byref(desc), out.ctypes.data, nrows, C.byref(par), C.byref(fpar), None, 0, *tail, e[4], 256),
    ]
    assert out.tobytes() == rows.tobytes() or all(c == 0 for c in codes)
    return codes, [x.value.decode() for x in e[:5]], lib.frbch_rfi_peaks_kernel(C.byref(desc), rows.ctypes.data, nrows, C.byref(par))


BAD = [("block_rows", 0), ("block_rows", 4), ("block_rows", 7), ("block_rows", 48), ("block_rows", 1000), ("block_rows", 8192),
       ("block_rows", 1 << 20), ("nrows", 0), ("nbits", 4), ("product", 1), ("t_cell", -1.0), ("chan_frac", 1.5), ("size", 8), ("fil_size", 8)]
BAD_F = [("t_pow", 0.0), ("t_pow", -1.0), ("t_pow", float("nan")), ("t_pow", float("inf")), ("fchan_frac", -0.1), ("fchan_frac", 1.01),
         ("fchan_frac", float("nan")), ("fsize", 8)]


@pytest.mark.parametrize("what,value", BAD + BAD_F, ids=["%s_%s" % b for b in BAD + BAD_F])
def test_bad_arguments(emu_lib, what, value):
    rows = rc.make_rows(40, 1, 64, 8)
    nrows, kw = 40, dict(block_rows=8)
    if what in rc.DEFAULTS:
        kw[what] = value
    par = post.rfi_params(dict(rc.DEFAULTS, **kw))
    fpar = pc.fparams(10.0, 0.3)
    desc = rc.desc_of(rows, 0)
    if what == "nrows":
        nrows = value
    elif what == "nbits":
        desc.nbits = value
    elif what == "product":
        desc.product = value
    elif what == "size":
        par.size -= value
    elif what == "fil_size":
        desc.size -= value
    elif what == "t_pow":
        fpar.t_pow = value
    elif what == "fchan_frac":
        fpar.chan_frac = value
    elif what == "fsize":
        fpar.size -= value
    codes, msgs, says = call_all(emu_lib, rows, nrows, desc, par, fpar)
    takes_fpar = [False, False, True, True, True]
    for code, msg, f in zip(codes, msgs, takes_fpar):
        if (what, value) in BAD_F and not f:
            assert code == 0, msg
        else:
            assert code == _lib.E_ARG and msg, (code, msg)
            if what == "block_rows" and value:
                assert "power of two" in msg and "8 .. 4096" in msg
            if what in ("size", "fil_size", "fsize"):
                assert "size" in msg
            if what == "t_pow":
                assert "t_pow" in msg
    assert says == (_lib.E_ARG if (what, value) in BAD else pc.GENERIC)


def test_the_arguments_of_the_bad_cases_are_good_otherwise(emu_lib):
    rows = rc.make_rows(40, 1, 64, 8)
    codes, msgs, says = call_all(emu_lib, rows, 40, rc.desc_of(rows, 0), rc.params(block_rows=8), pc.fparams(10.0, 0.3))
    assert codes == [0] * 5 and says == pc.GENERIC, msgs
    code, _dec, msg = pc.periodic_call(emu_lib, np.zeros((4, 64, 2), np.uint64), np.zeros((4, 64), pc.PEAK), 40, 1, 8, 0,
                                       rc.params(block_rows=8), pc.fparams(10.0), nblk=4)
    assert code == _lib.E_ARG and "nblk" in msg


def test_python_refusals(emu_lib, tmp_path):
    rows = rc.make_rows(600, 1, 64, 8)
    hdr = rc.hdr_of(64, 1, 8)
    for br in (1000, 4, 8192):
        with pytest.raises(post.InputError, match="power of two in 8 .. 4096"):
            post.rfi_peaks(rows, hdr, dict(block_rows=br), lib=emu_lib)
        with pytest.raises(post.InputError, match="power of two in 8 .. 4096"):
            post.clean(rows, hdr, dict(block_rows=br), lib=emu_lib, periodic=True)
    with pytest.raises(post.InputError, match="t_freq OR t_pow"):
        post.clean(rows, hdr, dict(block_rows=256), lib=emu_lib, periodic=dict(t_freq=4.0, t_pow=3.0))
    with pytest.raises(post.InputError, match="unknown"):
        post.clean(rows, hdr, dict(block_rows=256), lib=emu_lib, periodic=dict(t_frq=4.0))
    fil = str(tmp_path / "r.fil")
    write_fil(fil, rows, dict(HDR, nchans=64), 1)
    with pytest.raises(post.InputError, match="not built for resident rows.*without --resident"):
        post.rfifind_fil(fil, block_rows=256, periodic=True, resident=True, lib=emu_lib)
    with pytest.raises(post.InputError, match="not built for resident rows"):
        post.search_fil(fil, DM0, rfi=True, periodic=True, resident=True, lib=emu_lib)
    with pytest.raises(post.InputError, match="--rfi"):
        post.candidates_fil(fil, DM0, periodic=True, lib=emu_lib)
    with pytest.raises(post.InputError, match="power of two"):
        post.rfifind_fil(fil, block_rows=300, periodic=True, lib=emu_lib)


# ---- failing device calls ----------------------------------------------------------------------------------------------------
def emu_hooks(lib):
    lib.frbch_test_emu_fail_at.argtypes, lib.frbch_test_emu_fail_at.restype = [C.c_long], None
    lib.frbch_test_emu_live.argtypes, lib.frbch_test_emu_live.restype = [], C.c_uint64
    lib.frbch_test_emu_set_mode.argtypes, lib.frbch_test_emu_set_mode.restype = [C.c_int], None
    lib.frbch_test_emu_pending.argtypes, lib.frbch_test_emu_pending.restype = [], C.c_uint64
    lib.frbch_test_emu_violations.argtypes, lib.frbch_test_emu_violations.restype = [], C.c_uint64
    return lib


WALK_ROWS = (64, 16, 3, 2, 64, 64 * 3 + 40)


def entry_points(lib):
    """name -> (call() -> (rc, message, outputs as bytes), the host arrays the call must not change)"""
    nchan, nbits, nifs, prod, n, nrows = WALK_ROWS
    rows, st, pk = pc.rows_case(*WALK_ROWS)
    par, fpar = rc.params(block_rows=n, t_cell=3.0), pc.fparams(5.0, 0.5)

    def peaks_host():
        code, got, got_st, _used, msg = pc.peaks_host(lib, rows, prod, par)
        return code, msg, got.tobytes() + got_st.tobytes()

    def peaks_device():                                   # (the emulator's device memory is host memory)
        got = np.zeros(pk.shape, pc.PEAK)
        used = C.c_uint32(9)
        err = C.create_string_buffer(512)
        code = lib.frbch_rfi_peaks_device(C.byref(rc.desc_of(rows, prod)), rows.ctypes.data, nrows, C.byref(par), 0, st.ctypes.data,
                                          got.ctypes.data, C.byref(used), err, len(err))
        return code, err.value.decode(), got.tobytes()

    def cleanf_host():
        code, out, res, _used, msg = pc.cleanf_host(lib, rows, prod, par, fpar)
        return code, msg, out.tobytes() + res["mask"].tobytes() + res["repl"].tobytes() + res["peaks"].tobytes() + res["pflag"].tobytes()

    def cleanf_device():
        out = np.array(rows, copy=True)
        nblk = st.shape[0]
        m, repl, cf, bf = np.zeros((nblk, nchan), np.uint8), np.zeros(nchan), np.zeros(nchan, np.uint8), np.zeros(nblk, np.uint8)
        pflag, pchan, got = np.zeros((nblk, nchan), np.uint8), np.zeros(nchan, np.uint8), np.zeros(pk.shape, pc.PEAK)
        used = (C.c_uint32 * 2)(9, 9)
        err = C.create_string_buffer(512)
        code = lib.frbch_rfi_cleanf_device(C.byref(rc.desc_of(rows, prod)), out.ctypes.data, nrows, C.byref(par), C.byref(fpar), None, 0,
                                           m.ctypes.data, repl.ctypes.data, cf.ctypes.data, bf.ctypes.data, pflag.ctypes.data,
                                           pchan.ctypes.data, got.ctypes.data, used, err, len(err))
        return code, err.value.decode(), out.tobytes() + m.tobytes() + repl.tobytes() + got.tobytes() + pflag.tobytes()

    def periodic():
        code, dec, msg = pc.periodic_call(lib, st, pk, nrows, nifs, nbits, prod, par, fpar)
        return code, msg, dec["pflag"].tobytes() + dec["power"].tobytes()
    return dict(peaks_host=peaks_host, peaks_device=peaks_device, cleanf_host=cleanf_host, cleanf_device=cleanf_device, periodic=periodic), rows


@pytest.mark.parametrize("name", ["peaks_host", "peaks_device", "cleanf_host", "cleanf_device", "periodic"])
def test_every_failing_device_call_is_reported_and_leaves_nothing_alive(emu_lib, name):
    """the n-th fallible call of the device layer fails, n = 1, 2, ... until the entry point succeeds: a non-zero code with a
    message, the blocks and streams alive after the call those alive before it, the caller's rows unchanged; the call that
    goes through and a plain call afterwards give the plain call's bytes"""
    lib = emu_hooks(emu_lib)
    calls, rows = entry_points(lib)
    call = calls[name]
    before_bytes = rows.tobytes()
    code, msg, plain = call()
    assert code == 0, msg
    walk = 0
    for n in range(1, 200):
        live = lib.frbch_test_emu_live()
        lib.frbch_test_emu_fail_at(n)
        try:
            code, msg, got = call()
        finally:
            lib.frbch_test_emu_fail_at(0)
        assert lib.frbch_test_emu_live() == live, (n, msg)
        assert rows.tobytes() == before_bytes
        if code == 0:
            assert got == plain
            break
        assert code in (_lib.E_DEVICE, _lib.E_NOMEM) and msg, (n, code, msg)
        walk += 1
    else:
        raise AssertionError("the walk did not end")
    assert (walk == 0) == (name == "periodic") and (name == "periodic" or walk >= 5)
    code, msg, again = call()
    assert code == 0 and again == plain, msg


@pytest.mark.parametrize("mode", [1, 2])
def test_adversary_schedules_give_the_outputs_of_mode_0(emu_lib, mode):
    """the emulator's deferring schedulers (lazy; others first): every new entry point returns what it returns when every call
    runs at once, nothing is left pending, and no stream is destroyed or block freed with work pending on it"""
    lib = emu_hooks(emu_lib)
    calls, _rows = entry_points(lib)
    plain = {name: call() for name, call in calls.items()}
    assert all(v[0] == 0 for v in plain.values())
    lib.frbch_test_emu_set_mode(mode)
    try:
        v0 = lib.frbch_test_emu_violations()
        for name, call in calls.items():
            code, msg, got = call()
            assert code == 0 and got == plain[name][2], (name, msg)
            assert lib.frbch_test_emu_pending() == 0, name
        assert lib.frbch_test_emu_violations() == v0
    finally:
        lib.frbch_test_emu_set_mode(0)


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
def test_python_peaks_periodic_and_clean_of_several_products(emu_lib):
    """post.clean(periodic=) on three products: pass one hands every product's periodic flags to its mask as `prior`; the union
    and pass two are those of the plain clean"""
    rows = rc.make_rows(513, 3, 64, 8, seed=9)
    hdr = rc.hdr_of(64, 3, 8)
    kw = dict(block_rows=64, t_cell=3.0)
    rule = dict(rc.rule_kw(rc.DEFAULTS), t_cell=3.0)
    per = dict(t_pow=6.0, chan_frac=0.5)
    sts = [ro.stats(rows[:, p], 64) for p in range(3)]
    pks = [po.peaks(rows[:, p], sts[p], 64) for p in range(3)]
    decs = [po.periodic(sts[p], pks[p], 513, 64, 6.0, 0.5) for p in range(3)]
    info = {}
    for p in range(3):
        pk, st = post.rfi_peaks(rows, hdr, kw, product=p, lib=emu_lib, info=info, want_stats=True)
        assert pc.same_peaks(pk, pks[p]) and st.tobytes() == sts[p].tobytes() and info["kernel_used"] == (rc.GENERIC, pc.GENERIC)
        dec = post.rfi_periodic(st, pk, hdr, 513, kw, per, product=p, lib=emu_lib)
        assert np.array_equal(dec["pflag"], decs[p]["pflag"]) and np.array_equal(dec["pchan"], decs[p]["pchan"]) and dec["t_pow"] == 6.0
        assert dec["power"].tobytes() == decs[p]["power"].tobytes()
    first = [ro.mask(sts[p], 513, 64, 8, prior=decs[p]["pflag"], **rule) for p in range(3)]
    union = np.bitwise_or.reduce([r["mask"] for r in first])
    want = np.array(rows, copy=True)
    repl = []
    for p in range(3):
        r = ro.mask(sts[p], 513, 64, 8, prior=union, **rule)
        want = ro.apply(want, p, 64, union, r["repl"])
        repl.append(r["repl"])
    out, res = post.clean(rows, hdr, kw, lib=emu_lib, info=info, periodic=per)
    assert out.tobytes() == want.tobytes() and np.array_equal(res["mask"], union) and res["repl"].tobytes() == np.array(repl).tobytes()
    assert np.array_equal(res["pflag"], np.bitwise_or.reduce([d["pflag"] for d in decs])) and res["peaks"].tobytes() == np.stack(pks).tobytes()
    assert np.array_equal(res["pchan"], np.logical_or.reduce([d["pchan"] for d in decs]))
    assert np.array_equal(res["chan_flag"], np.logical_or.reduce([r["chan_flag"] for r in first]) | res["pchan"])
    assert info["peaks_kernel_used"] == pc.GENERIC and 0 < int(res["pflag"].sum()) and not np.array_equal(union, post.clean(rows, hdr, kw, lib=emu_lib)[1]["mask"])
    one, res1 = post.clean(rows, hdr, kw, lib=emu_lib, products=[1], periodic=per)
    alone, cleaned = pc.sequence_of_parts(rows, 1, 64, 8, rule, 6.0, 0.5)
    assert one.tobytes() == cleaned.tobytes() and np.array_equal(res1["mask"], alone["mask"]) and pc.same_peaks(res1["peaks"][1], pks[1])
    assert np.array_equal(res1["pflag"], alone["pflag"]) and np.array_equal(res1["chan_flag"], alone["chan_flag"])
    t4, _ = post.clean(rows, hdr, kw, lib=emu_lib, products=[1], periodic=True)
    same, _ = post.clean(rows, hdr, kw, lib=emu_lib, products=[1], periodic=dict(t_pow=post.t_pow_of(4.0, 64), chan_frac=0.3))
    assert t4.tobytes() == same.tobytes()


def files_of(d):
    got = {}
    for p in sorted(d.iterdir()):
        if p.suffix == ".npz":
            z = np.load(str(p))
            got[p.name] = {k: z[k].tobytes() for k in z.files}
        elif not p.name.endswith("in.fil"):
            got[p.name] = p.read_bytes()
    return got


def test_cli_rfifind_periodic_writes_its_files_and_changes_nothing_without_the_option(emu_lib, monkeypatch, tmp_path, capsys):
    """`post rfifind --periodic`: the .npz gains peaks, pflag, pchan and t_pow, the tone's cells are masked in the cleaned file.
    Without the option every file has the bytes of a run in which the new code cannot be reached at all (every new function of
    post and every new binding raises) -- and lacks the four keys."""
    q = np.ascontiguousarray(pc.known_answer_rows(0)[:, None, :])
    monkeypatch.setattr(_lib, "load", lambda path=None: emu_lib)
    d = {}
    for sub in ("with", "plain", "guarded"):
        d[sub] = tmp_path / sub
        d[sub].mkdir()
        write_fil(str(d[sub] / "in.fil"), q, dict(HDR, nchans=64), 1)
    assert post.main(["rfifind", str(d["with"] / "in.fil"), "--block-rows", "256", "--write-clean", "--periodic", "--t-freq", "4"]) == 0
    assert capsys.readouterr().out.count("wrote") == 3
    z = np.load(str(d["with"] / "in_rfi.npz"))
    want, cleaned = pc.sequence_of_parts(q, 0, rc.KA_BLOCK, 8, rc.rule_kw(rc.DEFAULTS), pc.ka_t_pow(), 0.3)
    assert {"peaks", "pflag", "pchan", "t_pow"} <= set(z.files) and float(z["t_pow"]) == pc.ka_t_pow()
    assert z["peaks"].tobytes() == want["peaks"][None].tobytes() and np.array_equal(z["pflag"], want["pflag"]) and not z["pchan"].any()
    assert np.array_equal(z["mask"], want["mask"]) and [tuple(v) for v in np.argwhere(z["mask"]).tolist()] == KA_CELLS
    assert np.ascontiguousarray(sigproc.read_fil(str(d["with"] / "in_clean.fil")).data).tobytes() == cleaned.tobytes()
    assert post.main(["rfifind", str(d["plain"] / "in.fil"), "--block-rows", "256", "--write-clean"]) == 0

    def unreachable(*_a, **_k):
        raise AssertionError("the periodic path was entered")

    class Guarded:
        def __getattr__(self, name):
            if name.startswith(("frbch_rfi_peaks", "frbch_rfi_periodic", "frbch_rfi_cleanf")):
                unreachable()
            return getattr(emu_lib, name)
    for name in ("rfi_peaks", "rfi_periodic", "rfi_fparams", "t_pow_of", "_periodic_pass", "_periodic_block"):
        monkeypatch.setattr(post, name, unreachable)
    monkeypatch.setattr(_lib, "load", lambda path=None: Guarded())
    assert post.main(["rfifind", str(d["guarded"] / "in.fil"), "--block-rows", "256", "--write-clean"]) == 0
    plain, guarded = files_of(d["plain"]), files_of(d["guarded"])
    assert sorted(plain) == sorted(guarded) == ["in.flag", "in_clean.fil", "in_rfi.npz"]
    assert plain == guarded and not {"peaks", "pflag", "pchan", "t_pow"} & set(plain["in_rfi.npz"])
    assert plain["in_clean.fil"] == open(str(d["plain"] / "in.fil"), "rb").read()      # the time-domain rule alone misses the tone
    with pytest.raises(AssertionError):
        post.main(["rfifind", str(d["guarded"] / "in.fil"), "--block-rows", "256", "--periodic"])


# ---- end to end on the emulator --------------------------------------------------------------------------------------------
E2E_WAVE = dict(channels=(40, 41), period=256, on=100, amp=95)


def e2e_rows():
    """the burst of rfi_cases.E2E with a square wave in two adjacent channels (one channel of 64 does not reach 6 sigma in the band
    sum once the search has taken the mean out): a period of one block, so that every block of such a channel has the same
    mean and the same std and the medians of the cell test absorb it"""
    x = rc.e2e_rows(False).astype(np.int64)
    t = np.arange(x.shape[0])
    for c in E2E_WAVE["channels"]:
        x[(t % E2E_WAVE["period"]) < E2E_WAVE["on"], c] += E2E_WAVE["amp"]
    return np.clip(x, 0, 255).astype(np.uint8)


def e2e_groups(tmp_path, sub, lib, rows, **kw):
    d = tmp_path / sub
    d.mkdir()
    fil = str(d / "burst.fil")
    write_fil(fil, rows[:, None, :], HDR, 1)
    info = {}
    dms = post.dm_list(DM0 + rc.E2E["dm_lo_off"], DM0 + rc.E2E["dm_hi_off"], rc.E2E["dmstep"])
    _files, groups = post.candidates_fil(fil, dms[0], dm2=dms[-1], dmstep=rc.E2E["dmstep"], threshold=rc.E2E["threshold"],
                                         zerodm=rc.E2E["zerodm"], max_width_s=rc.E2E["max_width_s"], nt=32, ndm=8, lib=lib, info=info, **kw)
    return groups, info, dms


def test_the_search_loses_a_periodic_channel_only_with_the_periodic_test(emu_lib, tmp_path):
    """The end-to-end case of rfi_cases.E2E with a square wave of one block's period in channels 40 and 41 and the across-channel
    rule off (t_chan = 0, as a band whose channels differ in level needs it; with it, the channels' std gives them away): the
    cell test sees every whole block of such a channel alike and flags none of them, and the search reports the wave's periods;
    with the periodic test the two channels are flagged wholly and the burst's group is all that is left."""
    clean_groups, _info, dms = e2e_groups(tmp_path, "clean", emu_lib, rc.e2e_rows(False))
    assert clean_groups.size == 1
    ref = clean_groups[0]["best"]

    def is_burst(g):
        b = g["best"]
        return int(b["dm_index"]) == int(ref["dm_index"]) and abs(int(b["sample"]) - int(ref["sample"])) <= int(ref["width"]) // 2
    rfi = dict(block_rows=rc.E2E["block_rows"], t_chan=0.0)
    rows = e2e_rows()
    dirty, info, _dms = e2e_groups(tmp_path, "time_only", emu_lib, rows, rfi=rfi)
    assert not info["rfi_chan_flag"].any() and not info["rfi_mask"][:-1].any() and sum(1 for g in dirty if not is_burst(g)) >= 10
    got, info, _dms = e2e_groups(tmp_path, "periodic", emu_lib, rows, rfi=rfi, periodic=dict(t_freq=4.0))
    assert got.size == 1 and is_burst(got[0]) and int(got[0]["best"]["width"]) == int(ref["width"])
    assert np.flatnonzero(info["rfi_pchan"]).tolist() == list(E2E_WAVE["channels"]) == np.flatnonzero(info["rfi_chan_flag"]).tolist()
    assert info["rfi_peaks_kernel_used"] == pc.GENERIC
