"""Interference flagging (frbch_rfi_*, post.rfi_stats / rfi_mask / clean / rfifind_fil, the flag file): the numpy restatement
tests/rfi_oracle.py on its known answers, the generic kernels and the host decision through the TEST-ONLY emulator build against
it (every comparison `==` or `tobytes()`: integer sums are exact, float sums have a fixed order, the decision is one sequence of
double operations), argument errors, and the Python layer's files."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import _lib, post, sigproc
from tests import rfi_cases as rc
from tests import rfi_oracle as ro
from tests.test_fold_predictor import write_fil
from tests.test_post import DM0, HDR


def same_stats(got, want):
    """integer sums to the bit; float sums to the bit where finite, not-finite in the same places"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == np.uint64:
        return got.tobytes() == want.tobytes()
    fin = np.isfinite(want)
    return (np.array_equal(fin, np.isfinite(got)) and got[fin].tobytes() == want[fin].tobytes()
            and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]))


# ---- the restatement's known answers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_known_answer(seed):
    """64 channels, blocks of 256, 24 * 256 - 100 rows of 8-bit noise with the injected interference: wholly flagged channels
    exactly {0, 1, 5, 20, 33, 63}, wholly flagged blocks exactly {7}, the only other masked cell (12, 40)"""
    q = rc.known_answer_rows(seed)
    res = ro.mask(ro.stats(q, rc.KA_BLOCK), q.shape[0], rc.KA_BLOCK, 8, zap=rc.ka_zap(), **rc.rule_kw(rc.DEFAULTS))
    assert np.flatnonzero(res["chan_flag"]).tolist() == rc.KA_CHANNELS
    assert np.flatnonzero(res["blk_flag"]).tolist() == rc.KA_BLOCKS
    assert rc.other_cells(res) == rc.KA_CELLS


def test_oracle_masks_nothing_in_noise():
    """the same noise without the injections, seeds 0 .. 19: no cell, no channel, no block -- a condition on the rule's false alarms"""
    for seed in range(20):
        q = rc.ka_quantise(rc.ka_noise(seed)[1])
        res = ro.mask(ro.stats(q, rc.KA_BLOCK), q.shape[0], rc.KA_BLOCK, 8, **rc.rule_kw(rc.DEFAULTS))
        assert int(res["mask"].sum()) == 0, seed


# ---- statistics and apply through the emulator ---------------------------------------------------------------------------
@pytest.mark.parametrize("g", rc.grid(), ids=rc.grid_id)
def test_emulator_equals_the_restatement(emu_lib, g):
    """48 / 64 / 128 channels x 8 / 16 / 32 bits x (one product, product 2 of 3) x blocks of 1, 7, 256 rows and one longer than
    the data, nrows one short of, equal to and one past a multiple: statistics, mask, cleaned rows, and clean in one call"""
    nchan, nbits, nifs, prod, br, nrows = g
    rows, st, want, cleaned = rc.grid_case(g)
    par = rc.params(block_rows=br, t_cell=3.0)
    assert emu_lib.frbch_rfi_nblk(nrows, br) == st.shape[0] == -(-nrows // br)
    assert emu_lib.frbch_rfi_stats_kernel(C.byref(rc.desc_of(rows, prod)), C.c_void_p(rows.ctypes.data), nrows, C.byref(par)) == rc.GENERIC
    code, got_st, used, msg = rc.stats_host(emu_lib, rows, prod, par)
    assert code == 0 and used == rc.GENERIC, msg
    assert same_stats(got_st, st)
    code, got, msg = rc.mask_call(emu_lib, got_st, nrows, nchan, nifs, nbits, prod, par)
    assert code == 0 and rc.same_result(got, want), msg
    code, out, msg = rc.apply_host(emu_lib, rows, prod, par, got["mask"], got["repl"])
    assert code == 0 and out.tobytes() == cleaned.tobytes(), msg
    for p in range(nifs):
        if p != prod:
            assert out[:, p].tobytes() == rows[:, p].tobytes()                 # other products keep their bytes
    keep = np.repeat(want["mask"] == 0, br, axis=0)[:nrows]
    assert np.array_equal(out[:, prod][keep], rows[:, prod][keep])             # and so do unmasked cells
    code, again, msg = rc.apply_host(emu_lib, out, prod, par, got["mask"], got["repl"])
    assert code == 0 and again.tobytes() == out.tobytes(), msg                 # idempotent
    code, out2, got2, used2, msg = rc.clean_host(emu_lib, rows, prod, par)
    assert code == 0 and used2 == rc.GENERIC and rc.same_result(got2, want) and out2.tobytes() == cleaned.tobytes(), msg


def test_the_grid_masks_something_but_not_everything():
    frac = [float(rc.grid_case(g)[2]["mask"].mean()) for g in rc.grid()]
    assert any(0.0 < f < 1.0 for f in frac) and any(f == 1.0 for f in frac) and any(f == 0.0 for f in frac)


def test_a_full_block_of_maximum_codes_does_not_wrap(emu_lib):
    """2^20 rows of 65535 on one 64-byte channel tile: Q = 65535^2 * 2^20 in every cell"""
    rows = np.full((1 << 20, 1, 32), 65535, dtype=np.uint16)
    par = rc.params(block_rows=1 << 20)
    code, st, _used, msg = rc.stats_host(emu_lib, rows, 0, par)
    assert code == 0, msg
    assert st.shape == (1, 32, 2) and np.all(st[:, :, 0] == 65535 << 20) and np.all(st[:, :, 1] == (65535 * 65535) << 20)


def test_nan_and_inf_make_their_cell_bad_and_leave_the_channel_alone(emu_lib):
    rng = np.random.default_rng(7)
    rows = (10.0 + rng.standard_normal((64 * 6, 1, 48))).astype(np.float32)
    rows[70, 0, 5] = np.nan
    rows[200, 0, 9] = np.inf
    par = rc.params(block_rows=64)
    want_st = ro.stats(rows[:, 0], 64)
    code, st, _used, msg = rc.stats_host(emu_lib, rows, 0, par)
    assert code == 0 and same_stats(st, want_st), msg
    want = ro.mask(want_st, rows.shape[0], 64, 32, **rc.rule_kw(rc.DEFAULTS))
    code, got, msg = rc.mask_call(emu_lib, st, rows.shape[0], 48, 1, 32, 0, par)
    assert code == 0 and rc.same_result(got, want), msg
    assert got["mask"][1, 5] == 1 and got["mask"][3, 9] == 1 and int(got["mask"].sum()) == 2
    assert not got["chan_flag"].any() and not got["blk_flag"].any() and np.isfinite(got["repl"]).all()
    code, out, msg = rc.apply_host(emu_lib, rows, 0, par, got["mask"], got["repl"])
    assert code == 0 and np.isfinite(out).all() and np.all(out[64:128, 0, 5] == np.float32(got["repl"][5])), msg


# ---- the rule --------------------------------------------------------------------------------------------------------------
def ka_stats(seed=0):
    q = rc.known_answer_rows(seed)
    return q, ro.stats(q, rc.KA_BLOCK)


@pytest.mark.parametrize("seed", [0, 1])
def test_known_answer_through_the_library(emu_lib, seed):
    q, st = ka_stats(seed)
    par = rc.params(block_rows=rc.KA_BLOCK)
    want = ro.mask(st, q.shape[0], rc.KA_BLOCK, 8, zap=rc.ka_zap(), **rc.rule_kw(rc.DEFAULTS))
    code, out, got, _used, msg = rc.clean_host(emu_lib, q[:, None, :], 0, par, zap=rc.ka_zap())
    assert code == 0 and rc.same_result(got, want), msg
    assert np.flatnonzero(got["chan_flag"]).tolist() == rc.KA_CHANNELS and np.flatnonzero(got["blk_flag"]).tolist() == rc.KA_BLOCKS
    assert rc.other_cells(got) == rc.KA_CELLS
    assert out.tobytes() == ro.apply(q[:, None, :], 0, rc.KA_BLOCK, want["mask"], want["repl"]).tobytes()
    assert np.all(out[:, 0, 20] == 96) and np.all(out[:, 0, 33] == got["repl"][33]) and 90 <= got["repl"][33] <= 102


def test_noise_masks_nothing_through_the_library(emu_lib):
    par = rc.params(block_rows=rc.KA_BLOCK)
    for seed in range(20):
        q = rc.ka_quantise(rc.ka_noise(seed)[1])
        code, out, got, _used, msg = rc.clean_host(emu_lib, q[:, None, :], 0, par)
        assert code == 0 and int(got["mask"].sum()) == 0 and out.tobytes() == q.tobytes(), (seed, msg)


def test_prior_is_ored_in_and_changes_no_count(emu_lib):
    """a prior of a whole block, most of a channel and scattered cells: the result is the mask without it ORed with it, the same
    channels and blocks flagged -- counted, it would flag channel 9 (20 of 24 blocks) and block 3"""
    q, st = ka_stats()
    par = rc.params(block_rows=rc.KA_BLOCK)
    nblk = st.shape[0]
    prior = np.zeros((nblk, rc.KA_NCHAN), np.uint8)
    prior[3, :] = 1
    prior[:20, 9] = 1
    prior[15:18, 50] = 1
    code, base, msg = rc.mask_call(emu_lib, st, q.shape[0], 64, 1, 8, 0, par, zap=rc.ka_zap())
    assert code == 0, msg
    code, got, msg = rc.mask_call(emu_lib, st, q.shape[0], 64, 1, 8, 0, par, zap=rc.ka_zap(), prior=prior)
    assert code == 0, msg
    assert np.array_equal(got["mask"], base["mask"] | prior)
    assert np.array_equal(got["chan_flag"], base["chan_flag"]) and np.array_equal(got["blk_flag"], base["blk_flag"])
    want = ro.mask(st, q.shape[0], rc.KA_BLOCK, 8, zap=rc.ka_zap(), prior=prior, **rc.rule_kw(rc.DEFAULTS))
    assert rc.same_result(got, want)
    assert got["repl"][9] == want["repl"][9] and not np.array_equal(got["repl"], base["repl"])   # repl: the cells left


def test_zapped_channels_stay_out_of_the_across_channel_medians(emu_lib):
    """channels 34 .. 63 are N(96, 40): zapped, the rest is judged among itself and 33 stands out; not zapped, they are nearly
    half of the band, widen D, and 33 passes step 5"""
    rng = np.random.default_rng(3)
    x = np.array(rc.known_answer_rows(0), dtype=np.float64)
    x[:, 34:] = 96.0 + 40.0 * rng.standard_normal((x.shape[0], 30))
    q = rc.ka_quantise(x)
    st = ro.stats(q, rc.KA_BLOCK)
    zap = np.zeros(64, bool)
    zap[34:] = True
    par = rc.params(block_rows=rc.KA_BLOCK)
    want = ro.mask(st, q.shape[0], rc.KA_BLOCK, 8, zap=zap, want_steps=True, **rc.rule_kw(rc.DEFAULTS))
    code, got, msg = rc.mask_call(emu_lib, st, q.shape[0], 64, 1, 8, 0, par, zap=zap)
    assert code == 0 and rc.same_result(got, want), msg
    assert np.flatnonzero(got["chan_flag"]).tolist() == [5, 20, 33] + list(range(34, 64))
    free = ro.mask(st, q.shape[0], rc.KA_BLOCK, 8, want_steps=True, **rc.rule_kw(rc.DEFAULTS))
    assert want["after5"][33] and not free["after5"][33]
    code, got, msg = rc.mask_call(emu_lib, st, q.shape[0], 64, 1, 8, 0, par)
    assert code == 0 and rc.same_result(got, free), msg


def test_t_chan_zero_switches_the_across_channel_rule_off(emu_lib):
    q, st = ka_stats()
    par = rc.params(block_rows=rc.KA_BLOCK, t_chan=0.0)
    want = ro.mask(st, q.shape[0], rc.KA_BLOCK, 8, zap=rc.ka_zap(), **dict(rc.rule_kw(rc.DEFAULTS), t_chan=0.0))
    code, got, msg = rc.mask_call(emu_lib, st, q.shape[0], 64, 1, 8, 0, par, zap=rc.ka_zap())
    assert code == 0 and rc.same_result(got, want), msg
    assert not got["chan_flag"][33] and got["chan_flag"][20] and got["chan_flag"][[0, 1, 63]].all()


@pytest.mark.parametrize("nbits,value", [(8, 77), (16, 40000), (32, 2.5)])
def test_constant_rows_are_dead_everywhere(emu_lib, nbits, value):
    rows = np.full((700, 1, 64), value, dtype=rc.DTYPES[nbits])
    par = rc.params(block_rows=256)
    code, out, got, _used, msg = rc.clean_host(emu_lib, rows, 0, par)
    assert code == 0, msg
    assert got["chan_flag"].all() and got["mask"].all() and np.all(got["repl"] == value) and out.tobytes() == rows.tobytes()
    assert rc.same_result(got, ro.mask(ro.stats(rows[:, 0], 256), 700, 256, nbits, **rc.rule_kw(rc.DEFAULTS)))


@pytest.mark.parametrize("nrows", [256, 100, 257, 512])
def test_one_and_two_blocks(emu_lib, nrows):
    q = rc.known_answer_rows(0)[:nrows]
    par = rc.params(block_rows=rc.KA_BLOCK)
    st = ro.stats(q, rc.KA_BLOCK)
    assert st.shape[0] == (1 if nrows <= 256 else 2)
    want = ro.mask(st, nrows, rc.KA_BLOCK, 8, zap=rc.ka_zap(), **rc.rule_kw(rc.DEFAULTS))
    code, out, got, _used, msg = rc.clean_host(emu_lib, np.ascontiguousarray(q[:, None, :]), 0, par, zap=rc.ka_zap())
    assert code == 0 and rc.same_result(got, want), msg
    assert out.tobytes() == ro.apply(q[:, None, :], 0, rc.KA_BLOCK, want["mask"], want["repl"]).tobytes()


def boundary_stats():
    """float statistics of 8 blocks x 9 channels of 4 rows each, every cell the same (mean 10, std 2) but for the bad ones
    (S = NaN): channel 0 has 3 bad cells, channel 1 has 2; block 5 has 2 bad cells, block 6 has 3"""
    st = np.zeros((8, 9, 2), dtype=np.float64)
    st[:, :, 0] = 40.0
    st[:, :, 1] = 4.0 * (100.0 + 4.0)
    for b, c in [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1), (5, 2), (5, 3), (6, 4), (6, 5), (6, 6)]:
        st[b, c, 0] = np.nan
    return st


def test_fraction_rules_at_their_boundary(emu_lib):
    """chan_frac = block_frac = 0.25 with 8 blocks and 8 channels left: a count of 2 = 0.25 * 8 does not flag, 3 does"""
    st = boundary_stats()
    par = rc.params(block_rows=4, chan_frac=0.25, block_frac=0.25)
    code, got, msg = rc.mask_call(emu_lib, st, 32, 9, 1, 32, 0, par)
    assert code == 0, msg
    assert np.flatnonzero(got["chan_flag"]).tolist() == [0] and np.flatnonzero(got["blk_flag"]).tolist() == [6]
    assert got["mask"][3, 1] and got["mask"][4, 1] and not got["mask"][0, 1] and got["mask"][5, 2] and not got["mask"][5, 4]
    want = ro.mask(st, 32, 4, 32, **dict(rc.rule_kw(rc.DEFAULTS), chan_frac=0.25, block_frac=0.25))
    assert rc.same_result(got, want)


# ---- argument errors -----------------------------------------------------------------------------------------------------
BAD = [("block_rows", 0), ("block_rows", (1 << 20) + 1), ("nrows", 0), ("nbits", 4), ("nbits", 64), ("product", 1), ("t_cell", -1.0),
       ("t_cell", float("nan")), ("t_cell", float("inf")), ("t_chan", -0.5), ("t_chan", float("nan")), ("t_chan", float("inf")),
       ("chan_frac", -0.1), ("chan_frac", float("nan")), ("chan_frac", 1.5), ("block_frac", -0.1), ("block_frac", float("nan")),
       ("block_frac", 1.01), ("size", 8), ("fil_size", 8)]


@pytest.mark.parametrize("what,value", BAD, ids=["%s_%s" % b for b in BAD])
def test_bad_arguments(emu_lib, what, value):
    rows = rc.make_rows(40, 1, 64, 8)
    nrows, kw = 40, dict(block_rows=8)
    if what in rc.DEFAULTS:
        kw[what] = value
    par = post.rfi_params(dict(rc.DEFAULTS, **kw))
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
    st = np.zeros((5, 64, 2), np.uint64)
    m, repl, cf, bf = np.zeros((5, 64), np.uint8), np.zeros(64), np.zeros(64, np.uint8), np.zeros(5, np.uint8)
    used = C.c_uint32(0)

    def err():
        return C.create_string_buffer(256)
    e = [err() for _ in range(5)]
    out = rows.copy()
    codes = [
        emu_lib.frbch_rfi_stats_host(C.byref(desc), rows.ctypes.data, nrows, C.byref(par), 0, st.ctypes.data, C.byref(used), e[0], 256),
        emu_lib.frbch_rfi_mask(C.byref(desc), st.ctypes.data, 5, nrows, C.byref(par), None, None, m.ctypes.data, repl.ctypes.data,
                               cf.ctypes.data, bf.ctypes.data, e[1], 256),
        emu_lib.frbch_rfi_apply_host(C.byref(desc), out.ctypes.data, nrows, C.byref(par), m.ctypes.data, repl.ctypes.data, 0, e[2], 256),
        emu_lib.frbch_rfi_clean_host(C.byref(desc), out.ctypes.data, nrows, C.byref(par), None, 0, m.ctypes.data, repl.ctypes.data,
                                     cf.ctypes.data, bf.ctypes.data, C.byref(used), e[3], 256),
        emu_lib.frbch_rfi_stats_device(C.byref(desc), rows.ctypes.data, nrows, C.byref(par), 0, st.ctypes.data, C.byref(used), e[4], 256),
    ]
    assert codes == [_lib.E_ARG] * 5 and all(x.value for x in e)
    assert emu_lib.frbch_rfi_stats_kernel(C.byref(desc), rows.ctypes.data, nrows, C.byref(par)) == _lib.E_ARG
    assert out.tobytes() == rows.tobytes()
    if what in ("size", "fil_size"):
        assert all(b"size" in x.value for x in e)


def test_nblk_and_its_refusals(emu_lib):
    assert emu_lib.frbch_rfi_nblk(1, 1) == 1 and emu_lib.frbch_rfi_nblk(1025, 1024) == 2 and emu_lib.frbch_rfi_nblk(1 << 20, 1 << 20) == 1
    assert emu_lib.frbch_rfi_nblk(0, 8) < 0 and emu_lib.frbch_rfi_nblk(8, 0) < 0 and emu_lib.frbch_rfi_nblk(8, (1 << 20) + 1) < 0
    rows = rc.make_rows(40, 1, 64, 8)
    code, _got, msg = rc.mask_call(emu_lib, np.zeros((4, 64, 2), np.uint64), 40, 64, 1, 8, 0, rc.params(block_rows=8), nblk=4)
    assert code == _lib.E_ARG and "nblk" in msg and rows.shape[0] == 40
    with pytest.raises(post.InputError):
        post.rfi_params(dict(t_cel=3.0))
    with pytest.raises(post.InputError):
        post.rfi_stats(rows, rc.hdr_of(64, 1, 8), dict(t_cell=-1.0), lib=emu_lib)


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_flag_file_round_trip(tmp_path):
    path = str(tmp_path / "Ef.flag_1200-1500MHz_64chan")
    with open(path, "w") as f:
        f.write("# hand-made\n0 1, 5:7\n10-12,20   # the birdie\n\n63\n30:30\n")
    flags = post.read_flag_file(path, 64)
    assert np.flatnonzero(flags).tolist() == [0, 1, 5, 6, 7, 10, 11, 12, 20, 30, 63]
    out = str(tmp_path / "back.flag")
    post.write_flag_file(out, flags)
    assert np.array_equal(post.read_flag_file(out, 64), flags)
    assert [ln for ln in open(out).read().splitlines() if not ln.startswith("#")] == ["0:1", "5:7", "10:12", "20", "30", "63"]
    for arr in (np.zeros(7, bool), np.ones(7, bool)):
        post.write_flag_file(out, arr)
        assert np.array_equal(post.read_flag_file(out, 7), arr)


@pytest.mark.parametrize("text,token", [("3 64", "64"), ("1, 60:64", "60:64"), ("7-x", "7-x"), ("9:3", "9:3"), ("-3", "-3")])
def test_flag_file_errors_name_the_token(tmp_path, text, token):
    path = str(tmp_path / "bad.flag")
    open(path, "w").write(text + "\n")
    with pytest.raises(post.InputError) as ei:
        post.read_flag_file(path, 64)
    assert "'%s'" % token in str(ei.value)


def test_python_stats_mask_and_clean_of_several_products(emu_lib):
    """post.clean on three products: the masks of the products ORed, every product cleaned in those cells with its own values"""
    rows = rc.make_rows(513, 3, 64, 8, seed=9)
    hdr = rc.hdr_of(64, 3, 8)
    kw = dict(block_rows=64, t_cell=3.0)
    rule = dict(rc.rule_kw(rc.DEFAULTS), t_cell=3.0)
    sts = [ro.stats(rows[:, p], 64) for p in range(3)]
    info = {}
    for p in range(3):
        st = post.rfi_stats(rows, hdr, kw, product=p, lib=emu_lib, info=info)
        assert st.tobytes() == sts[p].tobytes() and info["kernel_used"] == rc.GENERIC
        got = post.rfi_mask(st, hdr, 513, kw, product=p, lib=emu_lib)
        assert rc.same_result(got, ro.mask(sts[p], 513, 64, 8, **rule))
    union = np.bitwise_or.reduce([ro.mask(st, 513, 64, 8, **rule)["mask"] for st in sts])
    assert len({ro.mask(st, 513, 64, 8, **rule)["mask"].tobytes() for st in sts}) == 3          # the products differ
    want = np.array(rows, copy=True)
    repl = []
    for p in range(3):
        r = ro.mask(sts[p], 513, 64, 8, prior=union, **rule)
        assert np.array_equal(r["mask"], union)
        want = ro.apply(want, p, 64, union, r["repl"])
        repl.append(r["repl"])
    out, res = post.clean(rows, hdr, kw, lib=emu_lib, info=info)
    assert out.tobytes() == want.tobytes() and np.array_equal(res["mask"], union) and res["repl"].tobytes() == np.array(repl).tobytes()
    one, res1 = post.clean(rows, hdr, kw, lib=emu_lib, products=[1])
    alone = ro.mask(sts[1], 513, 64, 8, **rule)
    assert one.tobytes() == ro.apply(rows, 1, 64, alone["mask"], alone["repl"]).tobytes() and np.array_equal(res1["mask"], alone["mask"])


@pytest.mark.parametrize("form", ["indices", "bool", "uint8"])
def test_zap_list_with_several_products(emu_lib, tmp_path, form):
    """a zap list on a file of three products, as indices, as a bool mask and as the uint8 mask the library takes: the channels
    named are the channels zapped, in `clean`, in `rfi_mask` and in the files `rfifind_fil` writes"""
    rows = rc.make_rows(513, 3, 64, 8, seed=9)
    hdr = rc.hdr_of(64, 3, 8)
    kw = dict(block_rows=64, t_cell=3.0)
    rule = dict(rc.rule_kw(rc.DEFAULTS), t_cell=3.0)
    names = [5, 30, 63]
    zmask = np.zeros(64, bool)
    zmask[names] = True
    zap = {"indices": names, "bool": zmask, "uint8": zmask.astype(np.uint8)}[form]
    sts = [ro.stats(rows[:, p], 64) for p in range(3)]
    first = [ro.mask(st, 513, 64, 8, zap=zmask, **rule) for st in sts]
    union = np.bitwise_or.reduce([r["mask"] for r in first])
    chan = np.logical_or.reduce([r["chan_flag"] for r in first])
    assert chan[names].all() and not chan[[0, 1]].any() and 3 <= chan.sum() < 64
    want = np.array(rows, copy=True)
    repl = []
    for p in range(3):
        r = ro.mask(sts[p], 513, 64, 8, zap=zmask, prior=union, **rule)
        want = ro.apply(want, p, 64, union, r["repl"])
        repl.append(r["repl"])
    got = post.rfi_mask(sts[1], hdr, 513, kw, zap=zap, product=1, lib=emu_lib)
    assert rc.same_result(got, first[1])
    out, res = post.clean(rows, hdr, kw, zap=zap, lib=emu_lib)
    assert out.tobytes() == want.tobytes() and np.array_equal(res["mask"], union) and np.array_equal(res["chan_flag"], chan)
    assert res["repl"].tobytes() == np.array(repl).tobytes()
    # the same through the files
    fil = str(tmp_path / "pol4.fil")
    write_fil(fil, rows, dict(HDR, nchans=64), 3)
    flag = str(tmp_path / "zap.flag")
    post.write_flag_file(flag, zmask)
    files, fres = post.rfifind_fil(fil, flag_file=flag, write_clean=True, lib=emu_lib, **kw)
    assert np.array_equal(post.read_flag_file(files[1], 64), chan) and np.array_equal(fres["mask"], union)
    z = np.load(files[0])
    assert z["stats"].tobytes() == np.stack(sts).tobytes() and np.array_equal(z["zap"], zmask)
    assert np.ascontiguousarray(sigproc.read_fil(files[2]).data).tobytes() == want.tobytes()


def test_zap_forms():
    z = post._zap_array([5, 7, 63], 64)
    assert z.dtype == np.uint8 and np.flatnonzero(z).tolist() == [5, 7, 63]
    assert post._zap_array(z, 64).tobytes() == z.tobytes() and post._zap_array(z.astype(bool), 64).tobytes() == z.tobytes()
    assert post._zap_array([], 64).sum() == 0 and post._zap_array(None, 64) is None
    for bad in ([64], [-1], [1.5]):
        with pytest.raises(post.InputError):
            post._zap_array(bad, 64)


def test_apply_clamps_a_replacement_value_outside_the_code_range(emu_lib):
    """frbch_rfi_apply_* takes the caller's repl: beyond the codes, negative or NaN it is clamped (NaN: 0), never converted as is"""
    for nbits, top in ((8, 255), (16, 65535)):
        rows = rc.make_rows(20, 1, 64, nbits)
        m = np.zeros((2, 64), np.uint8)
        m[0, :4] = 1
        repl = np.full(64, 100.0)
        repl[:4] = [1e9, -7.0, np.nan, np.inf]
        code, out, msg = rc.apply_host(emu_lib, rows, 0, rc.params(block_rows=10), m, repl)
        assert code == 0, msg
        assert [int(out[r, 0, c]) for c in range(4) for r in (0, 9)] == [top, top, 0, 0, 0, 0, top, top]
        assert out[10:].tobytes() == rows[10:].tobytes() and out[:, :, 4:].tobytes() == rows[:, :, 4:].tobytes()


def ka_file(tmp_path, name="pr001a_ef_no0001_IFall.fil"):
    hdr = dict(HDR, nchans=64)
    fil = str(tmp_path / name)
    write_fil(fil, np.ascontiguousarray(rc.known_answer_rows(0)[:, None, :]), hdr, 1)
    return fil


def test_rfifind_fil_writes_its_files(emu_lib, tmp_path):
    fil = ka_file(tmp_path)
    zap = str(tmp_path / "zap.flag")
    open(zap, "w").write("0:1, 63\n")
    files, res = post.rfifind_fil(fil, block_rows=rc.KA_BLOCK, flag_file=zap, write_clean=True, lib=emu_lib)
    base = fil.replace(".fil", "")
    assert files == [base + "_rfi.npz", base + ".flag", base + "_clean.fil"]
    assert np.flatnonzero(post.read_flag_file(base + ".flag", 64)).tolist() == rc.KA_CHANNELS
    z = np.load(base + "_rfi.npz")
    q = rc.known_answer_rows(0)
    want = ro.mask(ro.stats(q, rc.KA_BLOCK), q.shape[0], rc.KA_BLOCK, 8, zap=rc.ka_zap(), **rc.rule_kw(rc.DEFAULTS))
    assert np.array_equal(z["mask"], want["mask"]) and np.array_equal(z["chan_flag"], want["chan_flag"])
    assert np.array_equal(z["blk_flag"], want["blk_flag"]) and z["repl"].tobytes() == want["repl"][None].tobytes()
    assert z["stats"].tobytes() == ro.stats(q, rc.KA_BLOCK)[None].tobytes()
    assert int(z["block_rows"]) == rc.KA_BLOCK and float(z["t_cell"]) == 5.0 and float(z["block_frac"]) == 0.3 and int(z["nrows"]) == rc.KA_NROWS
    src, dst = sigproc.read_fil(fil), sigproc.read_fil(base + "_clean.fil")
    raw, clean = open(fil, "rb").read(), open(base + "_clean.fil", "rb").read()
    assert raw[: src.header_bytes] == clean[: src.header_bytes] and dst.header_bytes == src.header_bytes and len(raw) == len(clean)
    assert np.ascontiguousarray(dst.data).tobytes() == ro.apply(q[:, None, :], 0, rc.KA_BLOCK, want["mask"], want["repl"]).tobytes()


def emu_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libfrbch_emu.so")


def test_cli_rfifind_and_candidates_with_rfi(emu_lib, monkeypatch, tmp_path, capsys):
    """`post rfifind` writes a .flag that read_flag_file reads back, and `post candidates --rfi --flag` runs through"""
    fil = str(tmp_path / "a.fil")
    write_fil(fil, rc.e2e_rows(True)[:, None, :], HDR, 1)
    monkeypatch.setattr(_lib, "load", lambda path=None: emu_lib)
    assert post.main(["rfifind", fil, "--block-rows", "256", "--t-cell", "5", "--write-clean"]) == 0
    out = capsys.readouterr().out
    assert out.count("wrote") == 3 and "channels and" in out
    flags = post.read_flag_file(str(tmp_path / "a.flag"), 64)
    assert flags.shape == (64,)
    with pytest.warns(UserWarning, match="flagged wholly"):
        assert post.main(["candidates", fil, "--dm", str(DM0 - 1.0), "--dm2", str(DM0 + 1.0), "--threshold", "6", "--rfi", "--flag",
                          str(tmp_path / "a.flag"), "--nt", "32", "--ndm", "8"]) == 0
    assert "candidates above 6.0 sigma" in capsys.readouterr().out
    with pytest.warns(UserWarning, match="flagged wholly"):
        assert post.main(["search", fil, "--dm", str(DM0), "--threshold", "6", "--rfi"]) == 0


def outputs(tmp_path, sub, lib, **kw):
    d = tmp_path / sub
    d.mkdir()
    fil = str(d / "b.fil")
    write_fil(fil, rc.e2e_rows(True)[:, None, :], HDR, 1)
    files, _groups = post.candidates_fil(fil, DM0 - 1.0, dm2=DM0 + 1.0, dmstep=1.0, threshold=6.0, nt=32, ndm=8, lib=lib, **kw)
    post.search_fil(fil, DM0, threshold=6.0, write_dat=True, lib=lib, **kw)
    got = {}
    for p in sorted(d.iterdir()):
        if p.suffix == ".npz":
            z = np.load(str(p))
            got[p.name] = {k: z[k].tobytes() for k in z.files}
        elif p.name != "b.fil":
            got[p.name] = p.read_bytes()
    return got


def test_defaults_write_the_files_they_wrote_before(emu_lib, tmp_path, monkeypatch):
    """search_fil and candidates_fil without flag_file / rfi: byte for byte the files of a run in which the new code path
    cannot be reached at all (every new function of post and every frbch_rfi_* binding raises)"""
    with_new = outputs(tmp_path, "with", emu_lib)

    def unreachable(*_a, **_k):
        raise AssertionError("the flagging path was entered")

    class Guarded:
        def __getattr__(self, name):
            if name.startswith("frbch_rfi_"):
                unreachable()
            return getattr(emu_lib, name)
    for name in ("clean", "rfi_stats", "rfi_mask", "rfi_params", "read_flag_file", "rfifind_fil"):
        monkeypatch.setattr(post, name, unreachable)
    without = outputs(tmp_path, "without", Guarded())
    assert sorted(with_new) == sorted(without) and len(with_new) >= 8
    for name in with_new:
        assert with_new[name] == without[name], name
    with pytest.raises(AssertionError):
        outputs(tmp_path, "third", Guarded(), rfi=True)


# ---- end to end on the emulator ---------------------------------------------------------------------------------------------
def groups_of(tmp_path, sub, lib, with_rfi, **kw):
    d = tmp_path / sub
    d.mkdir()
    fil = str(d / "burst.fil")
    write_fil(fil, rc.e2e_rows(with_rfi)[:, None, :], HDR, 1)
    info = {}
    dms = post.dm_list(DM0 + rc.E2E["dm_lo_off"], DM0 + rc.E2E["dm_hi_off"], rc.E2E["dmstep"])
    _files, groups = post.candidates_fil(fil, dms[0], dm2=dms[-1], dmstep=rc.E2E["dmstep"], threshold=rc.E2E["threshold"],
                                         zerodm=rc.E2E["zerodm"], max_width_s=rc.E2E["max_width_s"],
                                         nt=32, ndm=8, lib=lib, info=info, **kw)
    return groups, info, dms


def test_cleaning_leaves_the_burst_and_nothing_else(emu_lib, tmp_path):
    """the dispersed burst of the search tests with an intermittent loud channel and one broadband block added: uncleaned, the
    grouping reports more than the burst; with rfi=True it reports the burst's group only -- the best DM index and width of the
    interference-free file, its sample within half the width.  (The broadband rows lie in the last block of the file: a wholly
    flagged block is a flat stretch of the series, see DESIGN 10 on what the search's normalisation makes of one mid-file.)"""
    clean_groups, _info, dms = groups_of(tmp_path, "clean", emu_lib, False)
    assert clean_groups.size == 1
    ref = clean_groups[0]["best"]
    assert abs(dms[int(ref["dm_index"])] - DM0) < 1e-9 and abs(int(ref["sample"]) - (rc.E2E["t0"] + 3)) <= 1

    def is_burst(g):
        b = g["best"]
        return int(b["dm_index"]) == int(ref["dm_index"]) and abs(int(b["sample"]) - int(ref["sample"])) <= int(ref["width"]) // 2
    dirty, _info, _dms = groups_of(tmp_path, "dirty", emu_lib, True)
    assert sum(1 for g in dirty if not is_burst(g)) >= 1
    got, info, _dms = groups_of(tmp_path, "flagged", emu_lib, True, rfi=dict(block_rows=rc.E2E["block_rows"]))
    assert got.size == 1 and is_burst(got[0]) and int(got[0]["best"]["width"]) == int(ref["width"])
    loud_blocks = sorted({r // rc.E2E["block_rows"] for a, b in rc.E2E["loud_rows"] for r in (a, b - 1)})
    assert all(info["rfi_mask"][b, rc.E2E["loud_channel"]] for b in loud_blocks) and len(loud_blocks) >= 3
    assert info["rfi_blk_flag"][rc.E2E["broad_rows"][0] // rc.E2E["block_rows"]]
    with pytest.warns(UserWarning, match="flagged wholly"):                  # 1024-row blocks against detrend_len 1000
        got_true, _info, _dms = groups_of(tmp_path, "flagged_defaults", emu_lib, True, rfi=True)
    assert got_true.size == 1 and is_burst(got_true[0]) and int(got_true[0]["best"]["width"]) == int(ref["width"])
