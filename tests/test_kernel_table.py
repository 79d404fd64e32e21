"""tests/kernel_table.py against the kernels the built library holds (CPU: needs the library built, no GPU)."""
import functools
import re
import subprocess

from frb_baseband_amd import _lib
from tests import kernel_table as kt


@functools.lru_cache(maxsize=None)
def library_kernels():
    """The channeliser's kernels by name: `nm -C` on libfrbch.so, which keeps the host-side launch stub of every kernel
    (`fast::__device_stub__frbch_k2_wave<3, 8, 4, 2, true>(KParams)`; the shared library carries them just as frbch_launch.o does,
    beside those of frbch_post.o).  Names only: nothing else is read out of the binary.  The
    post-filterbank kernels (frbch_post_*) have their own tests (test_gpu_post_shapes.py) and are left out.  A missing `nm` raises."""
    out = subprocess.check_output(["nm", "-C", _lib.LIB_PATH]).decode()
    names = set()
    for m in re.finditer(r"__device_stub__(frbch_\w+(?:<[^>]*>)?)", out):
        if not m.group(1).startswith("frbch_post_"):
            names.add(m.group(1))
    assert names, "no kernel stubs listed in " + _lib.LIB_PATH
    return names


def test_table_rows_and_generic_kernels_are_the_librarys_kernels(hip_lib):
    """every register-pass instantiation has a row, every row (and every kernel a row also asserts) names a kernel of the library;
    an instantiation that no configuration reaches is taken out of its selector, not listed here"""
    lib = library_kernels()
    table = {r.name for r in kt.ROWS}
    assert table.isdisjoint(kt.GENERIC)
    assert sorted(lib - table - kt.GENERIC) == [], "kernels without a row"
    assert sorted((table | kt.GENERIC) - lib) == [], "rows that name no kernel of the library"
    also = {n for r in kt.ROWS for n in r.also}
    assert also <= lib, sorted(also - lib)


def test_every_family_has_its_stage(hip_lib):
    fams = {kt.family(n) for n in library_kernels() - kt.GENERIC}
    assert fams == set(kt.STAGE_GENERIC), fams ^ set(kt.STAGE_GENERIC)
    assert {g for g in kt.STAGE_GENERIC.values() if g} <= kt.GENERIC


def _cfg(r):
    return (r.case[0], r.case[3]) if r.kind == "case" else (r.bw, r.kw)


def test_code_families_cover_every_output_width_and_both_band_senses():
    for fam in kt.CODE_FAMILIES:
        rows = [_cfg(r) for r in kt.ROWS if fam in {kt.family(n) for n in (r.name,) + r.also}]
        assert {kw.get("nbit", 8) for _bw, kw in rows} == {2, 8, 16, -32}, fam
        assert {bw > 0 for bw, _kw in rows} == {True, False}, fam


def test_rows_are_small_and_launch_twice():
    """blocks of at most 2^23 samples (the 2^26 rows point at CASES), at least three of them, and -- but for the rows whose one
    launch has to exceed a persistent grid -- at most two per launch"""
    for r in kt.ROWS:
        if r.kind != "stream":
            continue
        res = r.kw.get("freq_res") or (512 if r.nchan <= 128 else 2 * r.nchan)
        n = 2 * r.nchan * res
        assert n <= 1 << 23, r
        blocks = r.secs * 2e6 * abs(r.bw) / n
        assert blocks >= 3.0, r
        if r.grid_x is None and r.grid_y is None:
            assert r.kw.get("maxb") == 2, r


def test_case_rows_point_at_cases():
    from tests import test_gpu_parity as tp
    for r in kt.ROWS:
        if r.kind == "case":
            assert r.case in tp.CASES, r


def test_launch_record_counts_launches_and_grids(emu_lib):
    """the record itself, on the emulator build (generic kernels only): nothing without profiling, one entry per kernel with its
    launches and largest grid with it, cleared by frbch_timing_reset"""
    from frb_baseband_amd import channeliser as ch, synth
    from tests import parity_util as pu
    raw = synth.make_vdif(0.02, bw_mhz=16.0, nchan=32)
    cfg = pu.lib_cfg(emu_lib, 16.0, 32, 0.02, maxb=2, interval=0.0)
    with ch.Channeliser(cfg, emu_lib) as c:
        c.channelise_bytes(raw)
        blocks = c.get_info().blocks_done
        assert c.get_launch_record() == {}
    with ch.Channeliser(cfg, emu_lib) as c:
        c.set_profiling(True)
        c.channelise_bytes(raw)
        rec = c.get_launch_record()
        assert set(rec) == {"frbch_k1_branch", "frbch_kc_dcfix", "frbch_k2_chan"}, rec
        launches = (blocks + 1) // 2
        info = c.get_info()
        assert rec["frbch_k1_branch"] == dict(launches=launches, grid_x=2 * 32 // 16, grid_y=2), rec
        assert rec["frbch_kc_dcfix"] == dict(launches=launches, grid_x=1, grid_y=2), rec
        assert rec["frbch_k2_chan"]["launches"] == launches and rec["frbch_k2_chan"]["grid_y"] == 2, rec
        assert set(rec) <= kt.GENERIC and info.blocks_done == blocks
        c.timing_reset()
        assert c.get_launch_record() == {}
