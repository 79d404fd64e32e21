"""tests/big_rows.py on the emulator: the case builders of tests/test_gpu_beyond_4gib.py with marks of 2^20 / 2^21 bytes and 805
rows of 4 KiB.  Held here: the aliasing assertions at the REAL marks, the window arithmetic, and every reference that
big_rows.py restates for windows -- the dedispersed series, the clip, the count-matrix fold, the shifted cut-outs, the block
windows of the interference stage -- equal to the existing restatements on the WHOLE small array; then the same checks the
device module runs, through the emulator's `_device` entry points, at both addresses."""
import numpy as np
import pytest

from oracle import post_oracle as po
from tests import big_rows as bg
from tests import cutout_oracle as co
from tests import fold_model_oracle as fo
from tests import rfi_oracle as ro
from tests import rfi_periodic_oracle as rpo

NAMES = ("A8", "A16", "B8")
PROD = {"A8": 2, "A16": 1, "B8": 0}
BLOCK = 256
NCMP = 64


@pytest.fixture(scope="module", params=NAMES)
def case(request, emu_lib):
    """(name, BigRows, the whole small array, Resident in host memory)"""
    br = bg.small(request.param)
    res = bg.Resident(br, bg.mem_for(emu_lib)).lay(0)
    whole = br.window(0, br.nrows)
    whole.setflags(write=False)
    yield request.param, br, whole, res
    res.free()


# ---- the description ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_aliasing_holds_at_the_real_marks(name):
    """2^31 and 2^32 counted in bytes, in elements and in t * nchan: the row at each one that lies inside the buffer is not row
    0 of the base again"""
    br = bg.big(name)
    assert br.P == 3001 and br.nrows * br.row_bytes >= (1 << 32) + (128 << 20) > (br.nrows - 38) * br.row_bytes
    assert 131072 % 3001 == 2029 and 65536 % 3001 == 2515 and 32768 % 3001 == 2758
    want = {"A8": [65536, 131072], "A16": [65536, 131072], "B8": [32768, 65536]}[name]
    assert br.mark_rows == want and br.byte_mark_rows == want
    assert br.nrows % 1024 != 0 and (br.nrows - 1711) % 256 != 0          # a ragged last block, a ragged last time tile
    if name == "A16":
        assert (1 << 31) // br.row_elems == 131072                       # the element count passes 2^31 at the 2^32 byte mark
    if name == "B8":
        assert (1 << 32) // br.nchan == 65536 and br.nchan > 16384       # t * nchan passes 2^32 there; beyond the LDS cut-out kernel
    br.check_aliasing()


def test_a_base_length_that_divides_a_mark_is_refused():
    with pytest.raises(AssertionError, match="row 0 of the base again"):
        bg.BigRows(1024, 4, 8, 1e-3, P=2, marks=bg.MARKS_SMALL, tail_bytes=bg.TAIL_SMALL)
    with pytest.raises(AssertionError, match="row 0 of the base again"):
        bg.BigRows(8192, 4, 8, 64e-6, P=4096)


def test_small_shapes_pass_their_marks():
    for name in NAMES:
        br = bg.small(name)
        assert br.byte_mark_rows == [256, 512] and br.nrows == 805 and br.row_bytes == 4096 and br.P == 101


def test_windows_replicas_and_both_addresses(case):
    _name, br, whole, res = case
    for shift in (4, 0):
        res.lay(shift)
        assert res.address % 16 == shift
        assert np.array_equal(res.read(0, br.nrows), whole)
        res.check_equals()
    for t0, n in ((0, 1), (100, 2), (95, 300), (br.nrows - 7, 7), (256, 256)):
        assert np.array_equal(br.window(t0, n), whole[t0:t0 + n])
        assert np.array_equal(whole[t0], br.base[t0 % br.P])
    with pytest.raises(AssertionError):
        br.window(br.nrows - 3, 4)


def test_a_changed_row_is_seen_replica_by_replica(case):
    _name, br, whole, res = case
    res.lay(0)
    rows = res.window(600, 2)
    rows[1, br.nifs - 1, 17] ^= 1
    res.mem.put(res.address + 600 * br.row_bytes, rows)
    with pytest.raises(AssertionError, match="rows 601 .. 601"):
        res.check_equals()
    res.check_equals([(600, rows)])                    # named as expected: accepted
    res.lay(0)
    res.poke_cell(250, 260, 0, 9, 200)
    assert np.all(res.read(250, 10)[:, 0, 9] == 200) and np.array_equal(res.window(0, br.nrows), res.read(0, br.nrows))
    res.check_equals()
    res.lay(0)


# ---- dedispersion -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [5.0, 0.0])
def test_windowed_series_and_clip_equal_the_oracle_on_the_whole_array(case, clip):
    name, br, whole, _res = case
    prod = PROD[name]
    h = br.hdr()
    nout, nclip, runs = bg.want_dedisp(br, prod, bg.DMS, clip, NCMP)
    maxd = nout and br.nrows - nout
    assert 100 <= maxd <= 300 and [t0 for t0, _ in runs[True]] == [0, 256 - maxd // 2 - NCMP // 2, 512 - maxd // 2 - NCMP // 2, nout - NCMP]
    for zerodm in (True, False):
        want, wclip = po.dedisperse(whole[:, prod, :], fch1=h["fch1"], foff=h["foff"], tsamp=h["tsamp"], dms=bg.DMS, zerodm=zerodm, clip=clip)
        assert want.shape == (9, nout) and wclip == nclip and (clip == 0 or nclip >= (1 + prod // 2) * (br.nrows // br.P))
        for t0, series in runs[zerodm]:
            assert np.array_equal(series, want[:, t0:t0 + NCMP])
    # the literal loop on one window as well
    d = bg.delays_of(br, bg.DMS)[8]
    x = whole[300:300 + NCMP + maxd, prod, :]
    S = x.sum(axis=1, dtype=np.int64).astype(np.float64)
    lit = po.sum_delayed(x, S, [d], NCMP, True)[0]
    assert np.array_equal(bg.window_series(bg.prefix_sums(x), d, NCMP, True), lit)


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("zerodm,clip", [(True, 5.0), (False, 0.0), (True, 0.0), (False, 5.0)])
def test_dedisperse_on_the_emulator(emu_lib, case, zerodm, clip, shift):
    name, br, _whole, res = case
    res.lay(shift)
    want = bg.want_dedisp(br, PROD[name], bg.DMS, clip, NCMP)
    bg.check_dedisp(emu_lib, res, PROD[name], bg.DMS, zerodm, clip, bg.GENERIC, want)


# ---- interference -----------------------------------------------------------------------------------------------------------
def test_block_windows_equal_the_oracles_on_the_whole_array(case):
    name, br, _whole, res = case
    prod = br.nifs - 1
    res.lay(0)
    cells = bg.poke_four_cells(res, prod, BLOCK)
    assert [c[:2] for c in cells] == [(0, 256), (384, 640), (512, 768), (768, 805)]
    whole = res.window(0, br.nrows)
    st = ro.stats(whole[:, prod, :], BLOCK)
    chans = bg.peak_channels(br.nchan)
    pk = rpo.peaks(whole[:, prod, :][:, chans], st[:, chans], BLOCK)
    assert br.blocks(BLOCK) == [0, 1, 2, 3]
    for b in br.blocks(BLOCK):
        _r0, rows = bg.block_window(res, b, BLOCK)
        sb = ro.stats(rows[:, prod, :], BLOCK)
        assert np.array_equal(sb[0], st[b])
        assert rpo.peaks(rows[:, prod, :][:, chans], sb[:, chans], BLOCK).tobytes() == pk[b:b + 1].tobytes()
    m, repl = bg.chosen_mask(br, BLOCK)
    cleaned = ro.apply(whole, prod, BLOCK, m, repl)
    for b in br.blocks(BLOCK):
        r0, rows = bg.block_window(res, b, BLOCK)
        assert np.array_equal(ro.apply(rows, prod, BLOCK, m[b:b + 1], repl), cleaned[r0:r0 + rows.shape[0]])
    res.lay(0)


@pytest.mark.parametrize("shift", [0, 4])
def test_interference_stage_on_the_emulator(emu_lib, case, shift):
    name, br, _whole, res = case
    prod = br.nifs - 1
    res.lay(shift)
    bg.poke_four_cells(res, prod, BLOCK)
    bg.check_stats_and_peaks(emu_lib, res, prod, BLOCK, bg.GENERIC, bg.GENERIC)
    res.lay(shift)
    bg.check_apply(emu_lib, res, prod, BLOCK)
    bg.check_clean_is_its_parts(emu_lib, res, prod, BLOCK, shift, bg.GENERIC)
    bg.check_cleanf_is_its_parts(emu_lib, res, prod, BLOCK, shift, (bg.GENERIC, bg.GENERIC))
    bg.check_cleanp_is_its_parts(emu_lib, res, BLOCK, shift, bg.GENERIC)
    res.lay(0)


# ---- fold -------------------------------------------------------------------------------------------------------------------
def test_count_matrix_fold_equals_the_fold_oracle(case):
    _name, br, whole, _res = case
    rps = bg.fold_rps(br)
    assert rps == 320
    chans = bg.fold_channels(br.nchan)
    assert chans.size == 64 and np.unique(chans).size == 64 and chans.max() < br.nchan
    sums, hits = bg.want_fold(br, chans)
    h = br.hdr(bg.FOLD_TSAMP)
    wp, wh = fo.fold_all(whole, nbin=bg.FOLD_NBIN, subint_s=rps * bg.FOLD_TSAMP, f0=bg.FOLD_F0, f1=0.0, pepoch_mjd=None, fch1=h["fch1"],
                         foff=h["foff"], tsamp=bg.FOLD_TSAMP, tstart_mjd=h["tstart"])
    assert wp.shape == (3, br.nifs, br.nchan, 256)
    assert np.array_equal(sums, wp[:, :, chans, :])
    assert np.array_equal(np.broadcast_to(hits[:, None, :], wh.shape), wh)
    t = np.arange(br.nrows)                              # the bins are exact in binary
    assert np.array_equal(fo.bins(br.nrows, 1, fch1=h["fch1"], foff=h["foff"], tsamp=bg.FOLD_TSAMP, tstart_mjd=h["tstart"], nbin=256,
                                  f0=16.0)[:, 0], (t % 1024) // 4)


@pytest.mark.parametrize("shift", [0, 2])
def test_fold_on_the_emulator(emu_lib, case, shift):
    _name, br, _whole, res = case
    res.lay(shift)
    bg.check_foldp(emu_lib, res, bg.GENERIC)
    bg.check_fold(emu_lib, res, br.nifs - 1)
    res.lay(0)


# ---- cut-outs ---------------------------------------------------------------------------------------------------------------
def test_shifted_cutouts_equal_the_oracle_on_the_whole_array(case):
    name, br, whole, res = case
    res.lay(0)
    prod = PROD[name]
    cands = bg.cut_cands(br)
    want = co.planes_batch(whole[:, prod, :], br.hdr(), cands, bg.CUT_NT, bg.CUT_NF, bg.CUT_NDM)
    parts = bg.want_cutout(res, prod, cands)
    assert parts[0][4][0] == 96 and parts[1][4][0] < 512 < parts[1][4][1] and parts[2][4][1] == br.nrows
    for i, p in enumerate(parts):
        for g, w in zip(p[:4], want):
            assert g.tobytes() == w[i].tobytes()


@pytest.mark.parametrize("shift", [0, 4])
def test_cutout_on_the_emulator(emu_lib, case, shift):
    name, _br, _whole, res = case
    res.lay(shift)
    bg.check_cutout(emu_lib, res, PROD[name], bg.GENERIC)
    res.lay(0)
