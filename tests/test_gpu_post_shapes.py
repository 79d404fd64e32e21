"""GPU tests of the HIP-only kernels behind the filterbank across file layouts and shapes: frbch_post_dedisp_tiled<BPV, FLAGS,
ZERODM> (all 12 instantiations), frbch_post_foldp_slots / _hits / _lds<BPV> (both widths, channel tiles of 256, 128, 64, 32
and 16) and the generic kernels they fall back to -- several products with `product` != 0, `foff` of both signs, partial DM
groups, channel counts from 32 to 4096, nbin that is no power of two, odd and prime sub-integration lengths, one-row edges.
Rows come from tests/post_cases.py (every product differs), expected values from oracle/post_oracle.py and
tests/fold_model_oracle.py on ONE product of the rows; integer rows and float dedispersion compare with array_equal, float
folds with rtol 1e-12.  Every dedispersion case asserts frbch_dedisperse_kernel, every all-product fold `kernel_used`: a
predicate that fell back to "never" turns the case red.  (frbch_fold_* has one kernel only: nothing to tell apart.)"""
import ctypes as C
import contextlib
import faulthandler
import io

import numpy as np
import pytest

from frb_baseband_amd import post, process_vdif as pv, sigproc, synth
from tests import post_cases as pc
from tests.hipmem import GuardedBuffer as DeviceBuffer, hip

pytestmark = pytest.mark.gpu

CALL_LIMIT_S = 120          # a device call that has not come back by then ends the test process (traceback on stderr)
TILED, GENERIC = 1, 0


def dedisp_device(lib, hdr, rows, prod, dms, zerodm, clip, nout, shift=0):
    """frbch_dedisperse_device on rows resident `shift` bytes behind a 16-byte aligned device address
    -> (series, nclip, what frbch_dedisperse_kernel says of that address)"""
    assert pc.dedisp_nout(lib, hdr, rows, prod, dms) == nout
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    buf = DeviceBuffer(rows.nbytes + 16)
    assert buf.ptr.value % 16 == 0
    d_rows = C.c_void_p(buf.ptr.value + shift)
    assert hip().hipMemcpy(d_rows, rows.ctypes.data, rows.nbytes, 1) == 0
    d_out = DeviceBuffer(dm_arr.size * nout * 4)
    kernel = pc.dedisp_kernel(lib, hdr, rows, prod, dms, d_rows.value)
    nclip = C.c_uint64(0)
    err = C.create_string_buffer(512)
    faulthandler.dump_traceback_later(CALL_LIMIT_S, exit=True)
    try:
        rc = lib.frbch_dedisperse_device(C.byref(pc.desc_of(hdr, rows, prod)), d_rows, rows.shape[0], dm_arr.ctypes.data, dm_arr.size,
                                         1 if zerodm else 0, float(clip), 0, d_out.ptr, nout, C.byref(nclip), err, len(err))
    finally:
        faulthandler.cancel_dump_traceback_later()
    assert rc == 0, err.value
    out = d_out.to_numpy(np.float32).reshape(dm_arr.size, nout)
    buf.free()
    d_out.free()
    return out, nclip.value, kernel


def check_dedisp(lib, hdr, rows, prod, dms, zerodm, clip, kernel):
    """both entry points against the oracle on product `prod`, and the kernel the case was written for"""
    want, wclip = pc.want_dedisp(rows, hdr, prod, dms, zerodm, clip)
    nout = want.shape[1]
    assert nout % 256 != 0                                     # the last time tile is partial
    assert clip == 0 or wclip >= 3 + prod                      # the burst of this product, at least
    got, nclip, k = dedisp_device(lib, hdr, rows, prod, dms, zerodm, clip, nout)
    assert k == kernel
    assert nclip == wclip
    assert np.array_equal(got, want)
    # the host entry point uploads to memory of its own: hipMalloc aligns to 256 bytes at least, which is all the query looks at
    assert pc.dedisp_kernel(lib, hdr, rows, prod, dms, 4096) == kernel
    got, nclip = pc.dedisp_host(lib, hdr, rows, prod, dms, zerodm, clip, nout)
    assert nclip == wclip
    assert np.array_equal(got, want)
    return want


def dm_range(lo, n, step=1.0):
    return [lo + step * i for i in range(n)]


# ---- dedispersion ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zerodm", [True, False])
@pytest.mark.parametrize("clip", [5.0, 0.0])
@pytest.mark.parametrize("nbits", [8, 16, 32])
def test_every_tiled_instantiation(hip_lib, nbits, clip, zerodm):
    """frbch_post_dedisp_tiled<nbits / 8, clip on, zerodm> once each (FLAGS is on when rows were clipped, which the burst of
    the product sees to), on product 1 of 2, 16 DMs = two whole groups"""
    hdr = pc.make_hdr(1024)
    x = pc.make_rows(6000, 2, 1024, nbits, seed=4)
    check_dedisp(hip_lib, hdr, x, 1, dm_range(20.0, 16), zerodm, clip, TILED)


@pytest.mark.parametrize("nifs,prod,nbits", [(2, 0, 8), (2, 1, 16), (4, 0, 16), (4, 3, 8), (4, 2, 8), (4, 1, 32), (3, 2, 8)])
def test_tiled_products_of_a_several_product_file(hip_lib, nifs, prod, nbits):
    hdr = pc.make_hdr(1024)
    x = pc.make_rows(5000, nifs, 1024, nbits, seed=5)
    check_dedisp(hip_lib, hdr, x, prod, dm_range(40.0, 12, 1.5), True, 5.0, TILED)


@pytest.mark.parametrize("nifs,prod,nbits,nchan,kernel", [(2, 1, 8, 1024, TILED), (4, 2, 32, 1024, TILED), (1, 0, 16, 1024, TILED),
                                                          (4, 3, 8, 1000, GENERIC), (2, 0, 16, 1000, GENERIC)])
def test_ascending_band(hip_lib, nifs, prod, nbits, nchan, kernel):
    """foff > 0: fch1 is the bottom of the band, the delays FALL with channel index -- post_delay_s's other branch, and tile
    ranges whose smallest delay belongs to the tile's last channel"""
    hdr = pc.make_hdr(nchan, +1)
    x = pc.make_rows(5000, nifs, nchan, nbits, seed=6, hdr=hdr)
    want = check_dedisp(hip_lib, hdr, x, prod, dm_range(50.0, 10), True, 5.0, kernel)
    down = pc.make_hdr(nchan, -1)
    other, _ = pc.want_dedisp(x, down, prod, dm_range(50.0, 10), True, 5.0)
    assert not np.array_equal(other, want)                     # the sign matters for these rows


@pytest.mark.parametrize("ndm", [1, 8, 9, 13])
def test_partial_dm_groups(hip_lib, ndm):
    hdr = pc.make_hdr(1024)
    x = pc.make_rows(4000, 2, 1024, 8, seed=7)
    check_dedisp(hip_lib, hdr, x, 1, dm_range(30.0, ndm, 1.5), ndm % 2 == 1, 5.0, TILED)


@pytest.mark.parametrize("nbits,zerodm,clip", [(8, True, 5.0), (32, False, 0.0)])
def test_last_time_tile_reads_past_the_rows(hip_lib, nbits, zerodm, clip):
    """nout = 300 against a largest delay of over 900 rows: the second time tile stages rows beyond nrows, which must read
    as zeros (and never be addressed by a thread with t < nout)"""
    hdr = pc.make_hdr(1024)
    dms = dm_range(300.0, 8)
    maxd = int(pc.po.delays_samples(hdr["fch1"], hdr["foff"], 1024, hdr["tsamp"], dms[-1]).max())
    assert maxd > 900
    x = pc.make_rows(maxd + 300, 2, 1024, nbits, seed=8)
    want = check_dedisp(hip_lib, hdr, x, 1, dms, zerodm, clip, TILED)
    assert want.shape[1] == 300


@pytest.mark.parametrize("nchan,nifs,prod,nbits,nrows", [(64, 4, 2, 8, 6000), (64, 2, 1, 32, 3000), (2048, 2, 1, 8, 4000),
                                                         (4096, 2, 1, 16, 3000), (4096, 1, 0, 8, 3000)])
def test_tiled_channel_counts(hip_lib, nchan, nifs, prod, nbits, nrows):
    hdr = pc.make_hdr(nchan)
    x = pc.make_rows(nrows, nifs, nchan, nbits, seed=9)
    check_dedisp(hip_lib, hdr, x, prod, dm_range(20.0, 9), True, 5.0, TILED)


@pytest.mark.parametrize("nchan,nifs,prod", [(1000, 4, 3), (48, 2, 1)])
def test_channel_counts_without_whole_tiles_take_the_generic_kernel(hip_lib, nchan, nifs, prod):
    """8-bit rows, nchan % 64 != 0"""
    hdr = pc.make_hdr(nchan)
    x = pc.make_rows(5000, nifs, nchan, 8, seed=10)
    check_dedisp(hip_lib, hdr, x, prod, dm_range(20.0, 9), True, 5.0, GENERIC)


def test_coarse_dm_step_takes_the_generic_kernel(hip_lib):
    """8 DMs 40 apart: the group's delays span over 900 rows in the lowest tile, more than the LDS holds"""
    hdr = pc.make_hdr(1024)
    dms = dm_range(20.0, 8, 40.0)
    d = [pc.po.delays_samples(hdr["fch1"], hdr["foff"], 1024, hdr["tsamp"], dm)[-1] for dm in (dms[0], dms[-1])]
    assert d[1] - d[0] > 900 - 256
    x = pc.make_rows(5000, 2, 1024, 8, seed=11)
    check_dedisp(hip_lib, hdr, x, 1, dms, True, 5.0, GENERIC)
    check_dedisp(hip_lib, hdr, x, 1, dm_range(20.0, 8, 5.0), True, 5.0, TILED)      # the same rows, a step that fits


@pytest.mark.parametrize("nbits", [8, 32])
def test_alignment_decides_and_both_kernels_give_the_same_bits(hip_lib, nbits):
    """the same rows at a 16-byte aligned device address (tiled) and 4 bytes further on (generic)"""
    hdr = pc.make_hdr(1024)
    x = pc.make_rows(5000, 2, 1024, nbits, seed=12)
    dms = dm_range(60.0, 11)
    want, wclip = pc.want_dedisp(x, hdr, 1, dms, True, 5.0)
    a, na, ka = dedisp_device(hip_lib, hdr, x, 1, dms, True, 5.0, want.shape[1])
    b, nb, kb = dedisp_device(hip_lib, hdr, x, 1, dms, True, 5.0, want.shape[1], shift=4)
    assert (ka, kb) == (TILED, GENERIC)
    assert na == nb == wclip and wclip > 0
    assert np.array_equal(a, b) and np.array_equal(a, want)


# ---- single-product fold --------------------------------------------------------------------------------------------
# (nifs, product, foff sign, nchan, nbits, apply_delays, nbin, nrows, rows per sub-integration)
FOLD = [(2, 1, -1, 1024, 8, False, 256, 9001, 4096), (4, 3, -1, 1024, 16, False, 100, 9001, 3000), (4, 2, +1, 1000, 8, True, 256, 8193, 4099),
        (4, 1, +1, 200, 32, True, 1000, 5000, 1031), (3, 2, +1, 1024, 8, True, 128, 4097, 4096), (1, 0, +1, 48, 16, True, 37, 9001, 9000)]


@pytest.mark.parametrize("nifs,prod,sign,nchan,nbits,delays,nbin,nrows,rps", FOLD)
def test_single_product_fold_layouts(hip_lib, nifs, prod, sign, nchan, nbits, delays, nbin, nrows, rps):
    """frbch_fold_host on product `prod` against po.fold of that product: nchan no multiple of 256, nrows no multiple of the
    row chunks, a short (down to one row) last sub-integration, nbin no power of two, and foff > 0 with the delays applied"""
    hdr = pc.make_hdr(nchan, sign)
    x = pc.make_rows(nrows, nifs, nchan, nbits, seed=13, hdr=hdr)
    subint_s = (rps + 0.25) * hdr["tsamp"]
    assert nrows % rps != 0
    prof, hits = pc.fold_host(hip_lib, hdr, x, prod, pc.PAR, nbin, subint_s, delays)
    wp, wh = pc.want_fold(x, hdr, prod, pc.PAR, nbin, subint_s, delays)
    assert wp.shape[0] == -(-nrows // rps)
    pc.check_fold(x, prof, hits, wp, wh)


# ---- all-product fold -----------------------------------------------------------------------------------------------
def lds_tile(nchan, nbin):
    """the channel tile the LDS kernel is documented to take: the largest power of two in 16..256 that divides nchan and
    holds nbin uint32 sums per channel in 128 KiB; 0 = none (the generic kernel)"""
    for ct in (256, 128, 64, 32, 16):
        if nchan % ct == 0 and nbin * ct * 4 <= 128 * 1024:
            return ct
    return 0


# (nchan, nbin, nifs, nbits, nrows, rows per sub-integration, model, foff sign, apply_delays, channel tile, kernel_used)
FOLD_ALL = [
    (1024, 128, 4, 8, 20000, 6250, "polyco", -1, False, 256, 1),
    (4096, 100, 2, 16, 3000, 1031, "poly", -1, False, 256, 1),
    (2048, 256, 3, 8, 5000, 2503, "doppler", -1, False, 128, 1),
    (2048, 1000, 1, 8, 3000, 997, "polyco", -1, False, 32, 1),
    (64, 100, 4, 8, 20000, 6007, "polyco", -1, False, 64, 1),
    (1024, 512, 2, 16, 6000, 2999, "poly", +1, False, 64, 1),
    (32, 1000, 1, 16, 777, 40000, "poly", -1, False, 32, 1),
    (1024, 1000, 4, 8, 12000, 4001, "polyco", -1, False, 32, 1),
    (48, 256, 4, 8, 20000, 1031, "polyco", -1, False, 16, 1),
    (1024, 2048, 2, 16, 8000, 3001, "poly", -1, False, 16, 1),
    (4096, 2000, 1, 8, 2500, 2503, "doppler", -1, False, 16, 1),
    (1024, 128, 4, 8, 1, 6250, "poly", -1, False, 256, 1),
    (1024, 128, 3, 16, 777, 31250, "poly", -1, False, 256, 1),
    (1024, 256, 4, 8, 6001, 2000, "polyco", -1, False, 128, 1),
    (1000, 128, 4, 8, 6000, 2503, "polyco", -1, False, 0, 0),
    (1024, 256, 4, 8, 6000, 2503, "poly", +1, True, 128, 0),
    (1024, 256, 2, 16, 6000, 2503, "polyco", +1, True, 128, 0),
]


@pytest.mark.parametrize("nchan,nbin,nifs,nbits,nrows,rps,model,sign,delays,ct,kernel", FOLD_ALL)
def test_fold_all_shapes(hip_lib, nchan, nbin, nifs, nbits, nrows, rps, model, sign, delays, ct, kernel):
    """frbch_foldp_host against tests/fold_model_oracle.py: every channel tile of the LDS kernel with the polynomial and the
    polyco model, 32 to 4096 channels, nbin of 100 / 1000 / 2000 (the column rotation `& (ct - 1)` with rows of nbin that are no
    power of two), 1 to 4 products, odd and prime sub-integration lengths (lane groups whose rows are no multiple of the
    unroll, second row runs of a few rows), one sub-integration longer than the data, 1 and 777 rows, a last
    sub-integration of one row; 1000 channels and per-channel delays go to the generic kernel"""
    assert lds_tile(nchan, nbin) == ct
    hdr = pc.make_hdr(nchan, sign)
    x = pc.make_rows(nrows, nifs, nchan, nbits, seed=14, hdr=hdr)
    subint_s = (rps + 0.25) * hdr["tsamp"]
    segs = pc.polyco_blocks(hdr, nrows) if model == "polyco" else None
    doppler = 1e-4 if model == "doppler" else 0.0
    prof, hits, used = pc.fold_all(hip_lib, hdr, x, pc.PAR, nbin, subint_s, apply_delays=delays, segs=segs, doppler=doppler)
    assert used == kernel
    wp, wh = pc.want_fold_all(x, hdr, pc.PAR, nbin, subint_s, apply_delays=delays, segs=segs, doppler=doppler)
    assert wp.shape == (-(-nrows // rps), nifs, nchan, nbin)
    pc.check_fold(x, prof, hits, wp, wh)
    if nifs > 1 and nrows > 1:
        assert not np.array_equal(wp[:, 0], wp[:, nifs - 1])   # the products differ: one read in another's place would show


@pytest.mark.parametrize("nbits,nchan,nifs,ct", [(8, 64, 2, 64), (16, 48, 4, 16), (16, 1024, 1, 256)])
def test_all_maximum_codes_in_long_runs(hip_lib, nbits, nchan, nifs, ct):
    """every sample 0xFF / 0xFFFF, two bins that last 4000 rows each: the longest same-bin runs and the largest uint32 run
    sums the rows of a workgroup can give"""
    nbin, nrows = 2, 30000
    assert lds_tile(nchan, nbin) == ct
    hdr = pc.make_hdr(nchan)
    x = np.full((nrows, nifs, nchan), 0xFF if nbits == 8 else 0xFFFF, dtype=pc.DTYPES[nbits])
    par = dict(F0=1.0 / (8000 * hdr["tsamp"]), F1=0.0, PEPOCH=None, DM=0.0, PSR="x")
    prof, hits, used = pc.fold_all(hip_lib, hdr, x, par, nbin, 10.0)
    assert used == 1
    wp, wh = pc.want_fold_all(x, hdr, par, nbin, 10.0)
    assert wh.min() >= 12000 and wp.max() >= 12000 * float(x[0, 0, 0])
    pc.check_fold(x, prof, hits, wp, wh)


# ---- the layout the product itself writes ---------------------------------------------------------------------------
def test_post_stage_on_the_rows_the_channeliser_writes(hip_lib, tmp_path):
    """0.3 s of a 32 MHz IF through the channeliser with pol = 4 (PP, QQ, Re, Im), 8 bit, 1024 channels; the .fil read back with
    sigproc.read_fil: post.dedisperse (product 0) and post.fold_all of its rows against the oracles on fil.data[:, p, :]"""
    vd = str(tmp_path / "pr001a_ef_no0001_IF1.vdif")
    synth.make_vdif(0.3, bw_mhz=32.0, nchan=1024).tofile(vd)
    hdr = pv.make_hdr("J0000+00", 1400.0, vd, pol=4, usb=True, ra="00:00:00", dec="00:00:00", bw=32.0, telescope="effelsberg")
    with contextlib.redirect_stdout(io.StringIO()):
        path = pv.run_digifil(hdr, str(tmp_path), 0, 0.3, 1024, overwrite=True, pol=4, nbit=8)
    fil = sigproc.read_fil(path)
    h = fil.header
    rows = np.ascontiguousarray(fil.data)
    assert h["nifs"] == 4 and h["nchans"] == 1024 and h["nbits"] == 8 and rows.shape[1:] == (4, 1024) and rows.shape[0] >= 5000
    assert rows.dtype == np.uint8 and all(not np.array_equal(rows[:, 0], rows[:, p]) for p in (1, 2, 3))
    dms = post.dm_list(50.0, 61.0, 1.0)
    assert pc.dedisp_kernel(hip_lib, h, rows, 0, dms, 4096) == TILED
    got, nclip = post.dedisperse(fil, dms, zerodm=True, clip=5.0, lib=hip_lib)
    want, wclip = pc.want_dedisp(rows, h, 0, dms, True, 5.0)
    assert nclip == wclip and np.array_equal(got, want)
    par = dict(pc.PAR, PEPOCH=h["tstart"] - 300.0)
    info = {}
    prof, hits, _ = post.fold_all(fil, par, nbin=256, subint_s=0.1, lib=hip_lib, info=info)
    assert info["kernel_used"] == 1
    wp, wh = pc.fo.fold_all(rows, nbin=256, subint_s=0.1, f0=par["F0"], f1=par["F1"], pepoch_mjd=par["PEPOCH"], **pc.model_kw(h))
    pc.check_fold(rows, prof, hits, wp, wh)
