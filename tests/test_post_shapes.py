"""Layouts and shapes of the stages behind the filterbank on the TEST-ONLY emulator build (the generic kernels
frbch_post_rowsum / _colsum / _dedisp / _fold / _foldp): several products with `product` != 0, `foff` of both signs, channel
counts that are no multiple of anything, partial chunks, nbin that is no power of two -- the case builder of
tests/post_cases.py against oracle/post_oracle.py and tests/fold_model_oracle.py, bit-exact on integer rows.  The HIP-only
kernels meet the same builder in tests/test_gpu_post_shapes.py."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import _lib
from tests import post_cases as pc


def test_every_product_of_the_rows_differs():
    """what the builder promises: other levels, other pulse trains, other burst rows per product -- and so other clip flags"""
    hdr = pc.make_hdr(64, tsamp=64e-6)
    x = pc.make_rows(3000, 4, 64, 8, hdr=hdr)
    assert x.shape == (3000, 4, 64) and x.dtype == np.uint8 and x.max() <= 222
    flags = []
    for p in range(4):
        S = x[:, p, :].sum(axis=1, dtype=np.float64)
        flags.append(pc.po.clip_flags(S, 5.0))
        assert np.all(flags[-1][pc.burst_rows(3000, p)]) and flags[-1].sum() >= 3 + p
    for p in range(4):
        for q in range(p + 1, 4):
            assert not np.array_equal(flags[p], flags[q])
            assert abs(float(x[:, p].mean()) - float(x[:, q].mean())) > 5
    up = pc.make_hdr(64, +1, tsamp=64e-6)
    assert up["foff"] == -hdr["foff"] and up["fch1"] == hdr["fch1"] + 63 * hdr["foff"]        # the bottom of the same band
    assert not np.array_equal(pc.make_rows(3000, 1, 64, 8, hdr=up), x[:, :1])                  # the train follows the header


# (nifs, product, foff sign, nchan, nbits, zerodm, clip, nrows)
DEDISP = [(1, 0, -1, 64, 8, True, 5.0, 5000), (2, 1, -1, 64, 8, True, 5.0, 5000), (4, 0, -1, 64, 8, False, 4.0, 5000),
          (4, 2, +1, 64, 16, True, 5.0, 5000), (4, 3, -1, 50, 8, True, 0.0, 4097), (3, 1, +1, 7, 32, True, 5.0, 4500),
          (2, 0, +1, 64, 32, False, 0.0, 3000), (4, 3, +1, 50, 16, False, 5.0, 8193), (1, 0, +1, 7, 8, True, 3.0, 4096)]


@pytest.mark.parametrize("nifs,prod,sign,nchan,nbits,zerodm,clip,nrows", DEDISP)
def test_dedisperse_layouts_on_the_emulator(emu_lib, nifs, prod, sign, nchan, nbits, zerodm, clip, nrows):
    hdr = pc.make_hdr(nchan, sign, tsamp=64e-6)
    x = pc.make_rows(nrows, nifs, nchan, nbits, hdr=hdr)
    dms = [0.0, 12.5, pc.DM0, 150.0, 301.0]
    want, wclip = pc.want_dedisp(x, hdr, prod, dms, zerodm, clip)
    assert pc.dedisp_kernel(emu_lib, hdr, x, prod, dms, x.ctypes.data) == 0          # the emulator has the generic kernel only
    got, nclip = pc.dedisp_host(emu_lib, hdr, x, prod, dms, zerodm, clip, want.shape[1])
    assert nclip == wclip and (clip == 0 or nclip >= 3 + prod)
    assert np.array_equal(got, want)


# (nifs, product, foff sign, nchan, nbits, apply_delays, nbin, nrows, subint_s)
FOLD = [(2, 1, -1, 64, 8, False, 128, 9000, 0.2), (4, 3, +1, 64, 8, True, 100, 9000, 0.2), (4, 2, +1, 50, 16, True, 37, 4097, 0.1),
        (3, 0, -1, 7, 32, True, 128, 5000, 0.3), (4, 1, +1, 64, 16, False, 1000, 6000, 0.37), (1, 0, +1, 7, 8, True, 3, 513, 10.0)]


@pytest.mark.parametrize("nifs,prod,sign,nchan,nbits,delays,nbin,nrows,subint_s", FOLD)
def test_fold_layouts_on_the_emulator(emu_lib, nifs, prod, sign, nchan, nbits, delays, nbin, nrows, subint_s):
    hdr = pc.make_hdr(nchan, sign, tsamp=64e-6)
    x = pc.make_rows(nrows, nifs, nchan, nbits, hdr=hdr)
    prof, hits = pc.fold_host(emu_lib, hdr, x, prod, pc.PAR, nbin, subint_s, delays)
    wp, wh = pc.want_fold(x, hdr, prod, pc.PAR, nbin, subint_s, delays)
    pc.check_fold(x, prof, hits, wp, wh)


# (nifs, foff sign, nchan, nbits, apply_delays, nbin, nrows, subint_s, polyco)
FOLD_ALL = [(4, +1, 64, 8, True, 100, 9000, 0.2, True), (3, -1, 50, 16, False, 1000, 4097, 0.1, True),
            (2, +1, 7, 8, True, 37, 5000, 10.0, False), (4, +1, 64, 32, True, 128, 3000, 0.0961, False),
            (1, -1, 64, 8, False, 2, 777, 0.0201, False), (4, -1, 48, 16, False, 128, 1, 0.2, False)]


@pytest.mark.parametrize("nifs,sign,nchan,nbits,delays,nbin,nrows,subint_s,polyco", FOLD_ALL)
def test_fold_all_layouts_on_the_emulator(emu_lib, nifs, sign, nchan, nbits, delays, nbin, nrows, subint_s, polyco):
    hdr = pc.make_hdr(nchan, sign, tsamp=64e-6)
    x = pc.make_rows(nrows, nifs, nchan, nbits, hdr=hdr)
    segs = pc.polyco_blocks(hdr, nrows) if polyco else None
    prof, hits, used = pc.fold_all(emu_lib, hdr, x, pc.PAR, nbin, subint_s, apply_delays=delays, segs=segs)
    assert used == 0
    wp, wh = pc.want_fold_all(x, hdr, pc.PAR, nbin, subint_s, apply_delays=delays, segs=segs)
    pc.check_fold(x, prof, hits, wp, wh)


def test_foff_sign_changes_the_delays():
    """the two headers of one band: the same delays, mirrored in channel index (so a library that took fch1 for the top of
    an ascending band would fold and dedisperse other rows)"""
    dn, up = pc.make_hdr(64, -1), pc.make_hdr(64, +1)
    a = pc.po.delays_samples(dn["fch1"], dn["foff"], 64, dn["tsamp"], 300.0)
    b = pc.po.delays_samples(up["fch1"], up["foff"], 64, up["tsamp"], 300.0)
    assert a[0] == 0 and b[-1] == 0 and a[-1] > 500 and np.all(np.diff(a) >= 0) and np.all(np.abs(a - b[::-1]) <= 1)


def test_kernel_query_refuses_bad_arguments(emu_lib):
    hdr = pc.make_hdr(64, tsamp=64e-6)
    x = pc.make_rows(500, 2, 64, 8, hdr=hdr)
    dms = np.asarray([0.0, 20.0])
    good = pc.desc_of(hdr, x, 1)

    def ask(desc=good, addr=x.ctypes.data, nrows=500, dm_arr=dms, ndm=2):
        return emu_lib.frbch_dedisperse_kernel(C.byref(desc) if desc is not None else None, C.c_void_p(addr), nrows,
                                               dm_arr.ctypes.data if dm_arr is not None else None, ndm)

    assert ask() == 0
    assert ask(desc=None) == _lib.E_ARG
    assert ask(addr=0) == _lib.E_ARG                                           # null rows
    assert ask(nrows=0) == _lib.E_ARG
    assert ask(dm_arr=None) == _lib.E_ARG and ask(ndm=0) == _lib.E_ARG
    assert ask(dm_arr=np.asarray([0.0, -1.0])) == _lib.E_ARG
    assert ask(dm_arr=np.asarray([0.0, 5000.0])) == _lib.E_ARG                 # the delay exceeds the data: the launch refuses it too
    for field, value in (("size", good.size - 4), ("product", 2), ("nbits", 4), ("nchan", 0), ("foff_mhz", 0.0), ("tsamp_s", 0.0)):
        bad = pc.desc_of(hdr, x, 1)
        setattr(bad, field, value)
        assert ask(desc=bad) == _lib.E_ARG, field
