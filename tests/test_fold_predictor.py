"""Fold of every polarisation product with a phase predictor (frbch_foldp_*, post.fold_all / read_polyco / stokes /
fold_fil): the generic kernel through the TEST-ONLY emulator build against the numpy restatement of
tests/fold_model_oracle.py (bit-exact on integer rows), against the untouched frbch_fold_host for the trivial model,
analytic known answers (a Doppler-shifted train, a train that follows a cubic polyco), and the host-side file handling."""
import ctypes as C
import hashlib
import os
import struct
import zlib

import numpy as np
import pytest

from frb_baseband_amd import _lib, post, sigproc
from tests import fold_model_oracle as fo
from tests.test_post import DM0, HDR, P0, pulse_train_rows

F0 = 1.0 / P0


def as_fil_all(x, hdr, nbits):
    """x: [nrows][nifs][nchan]"""
    h = dict(hdr, nbits=nbits, nifs=x.shape[1])
    return sigproc.SigprocFile(header=h, header_bytes=0, data=np.ascontiguousarray(x))


def random_rows(nrows, nifs, nchan, nbits, seed=5):
    rng = np.random.default_rng(seed)
    if nbits == 8:
        return rng.integers(0, 256, size=(nrows, nifs, nchan), dtype=np.uint8)
    if nbits == 16:
        return rng.integers(0, 65536, size=(nrows, nifs, nchan), dtype=np.uint16)
    return (rng.random((nrows, nifs, nchan)) * 37.5).astype(np.float32)       # non-negative


def three_blocks(hdr, offsets_s=(0.1003, 0.3001, 0.5002), span_min=1.0):
    """three polyco blocks whose two boundaries (0.2002 s and 0.40015 s: rows 3128.1 and 6252.3 at 64 us) fall inside
    9000 rows, each at least 1e-6 s away from a row time"""
    coeffs = [[0.11, 0.53, -0.31, 2.1], [0.42, -0.77, 0.25], [0.05, 0.9, 0.6, -1.4, 3.0]]
    return [dict(tmid=hdr["tstart"] + off / 86400.0, rphase=0.1 + 0.27 * k, f0=F0 * (1.0 + 1e-5 * k), span=span_min,
                 coeff=coeffs[k], site="g") for k, off in enumerate(offsets_s)]


def model_kw(hdr):
    return dict(fch1=hdr["fch1"], foff=hdr["foff"], tsamp=hdr["tsamp"], tstart_mjd=hdr["tstart"])


PAR = dict(F0=F0, F1=-2.5e-9, PEPOCH=HDR["tstart"] - 300.0, DM=DM0, PSR="J0000+00")


def check_equal(nbits, prof, hits, wp, wh):
    assert prof.shape == wp.shape and hits.shape == wh.shape
    assert np.array_equal(hits, wh)
    if nbits == 32:
        np.testing.assert_allclose(prof, wp, rtol=1e-12)                  # float rows: atomics in any order
    else:
        assert np.array_equal(prof, wp)                                   # integer rows: exact


# ---- bit-exact against the restatement -----------------------------------------------------------------------------
def test_block_boundaries_keep_clear_of_the_rows():
    first = fo.block_first_rows(three_blocks(HDR), HDR["tstart"], HDR["tsamp"], 9000)
    assert list(first) == [0, 3129, 6253]
    for a, b in zip(three_blocks(HDR)[:-1], three_blocks(HDR)[1:]):
        x = (0.5 * (a["tmid"] + b["tmid"]) - HDR["tstart"]) * 86400.0
        assert abs(x / HDR["tsamp"] - round(x / HDR["tsamp"])) * HDR["tsamp"] > 1e-6


@pytest.mark.parametrize("nbits,nifs,delays", [(8, 1, False), (8, 4, False), (8, 4, True), (16, 1, True), (16, 4, False),
                                               (32, 1, False), (32, 4, True)])
def test_polyco_fold_matches_the_restatement(emu_lib, nbits, nifs, delays):
    x = random_rows(9000, nifs, 64, nbits)
    segs = three_blocks(HDR)
    info = {}
    prof, hits, nbin = post.fold_all(as_fil_all(x, HDR, nbits), PAR, polyco=segs, nbin=128, subint_s=0.2, apply_delays=delays,
                                     lib=emu_lib, info=info)
    wp, wh = fo.fold_all(x, nbin=128, subint_s=0.2, dm=DM0, apply_delays=delays, segs=segs, **model_kw(HDR))
    assert prof.shape == (3, nifs, 64, 128) and info["kernel_used"] == 0
    check_equal(nbits, prof, hits, wp, wh)
    # the blocks matter: one block alone gives other bins
    w1, _ = fo.fold_all(x, nbin=128, subint_s=0.2, dm=DM0, apply_delays=delays, segs=segs[:1], **model_kw(HDR))
    assert not np.array_equal(w1, wp)


@pytest.mark.parametrize("nbits,nifs,delays", [(8, 4, False), (8, 4, True), (16, 2, True), (8, 1, False)])
def test_trivial_model_equals_the_single_product_fold(emu_lib, nbits, nifs, delays):
    """nseg = 0, doppler = 0: product p is frbch_fold_host(product = p) to the bit (the cross-check against untouched code)"""
    x = random_rows(9000, nifs, 64, nbits, seed=8)
    fil = as_fil_all(x, HDR, nbits)
    prof, hits, nbin = post.fold_all(fil, PAR, nbin=128, subint_s=0.2, apply_delays=delays, lib=emu_lib)
    nsub = prof.shape[0]
    for p in range(nifs):
        desc = post.fil_desc(fil.header, product=p)
        one = np.zeros((nsub, 128, 64), dtype=np.float64)
        oh = np.zeros((nsub, 128, 64), dtype=np.uint32)
        err = C.create_string_buffer(256)
        rc = emu_lib.frbch_fold_host(C.byref(desc), x.ctypes.data, x.shape[0], PAR["F0"], PAR["F1"], PAR["PEPOCH"], PAR["DM"],
                                     1 if delays else 0, 128, 0.2, 0, one.ctypes.data, oh.ctypes.data, nsub, err, len(err))
        assert rc == 0, err.value
        assert np.array_equal(prof[:, p], one.transpose(0, 2, 1))
        assert np.array_equal(hits, oh.transpose(0, 2, 1))


# ---- Doppler factor ------------------------------------------------------------------------------------------------
HDR_LONG = dict(HDR, nchans=16, tsamp=256e-6)        # (8 s sub-integrations: 31250 rows, no rounding tie)


def excess_near_peak(profile):
    """fraction of the on-pulse excess (mean profile minus its median) that sits in the peak bin +- 1"""
    e = profile - np.median(profile)
    e[e < 0] = 0.0
    k = int(np.argmax(e))
    n = e.size
    return (e[(k - 1) % n] + e[k] + e[(k + 1) % n]) / e.sum()


def mean_profile(prof, hits, product=0):
    return prof[:, product].sum(axis=(0, 1)) / hits.sum(axis=(0, 1))


def train_from_turns(turns, nifs, nchan, phi0=0.3, amp=90, seed=4):
    """constant floor of 20 plus a pulse of `amp` in every row in which turns - phi0 passes an integer"""
    k = np.floor(turns - phi0)
    hit = np.nonzero(np.diff(k) > 0)[0] + 1
    x = np.full((turns.size, nifs, nchan), 20, dtype=np.uint8)
    x[hit] += amp
    return x


def test_doppler_factor(emu_lib):
    d, nrows, nbin = 1e-4, 117000, 128                                     # 30 s: the train drifts 1e-4 x 30 s x 29.9 Hz = 0.09 turns
    t = np.arange(nrows) * HDR_LONG["tsamp"]
    x = train_from_turns(F0 * (1.0 + d) * t, 1, 16)                        # period P / (1 + d)
    par = dict(F0=F0, F1=0.0, PEPOCH=None, DM=0.0, PSR="x")
    fil = as_fil_all(x, HDR_LONG, 8)
    prof, hits, _ = post.fold_all(fil, par, doppler=d, nbin=nbin, subint_s=8.0, lib=emu_lib)
    wp, wh = fo.fold_all(x, nbin=nbin, subint_s=8.0, f0=F0, f1=0.0, doppler=d, **model_kw(HDR_LONG))
    check_equal(8, prof, hits, wp, wh)
    assert excess_near_peak(mean_profile(prof, hits)) > 0.99               # one bin (two when the pulse straddles an edge)
    prof0, hits0, _ = post.fold_all(fil, par, nbin=nbin, subint_s=8.0, lib=emu_lib)
    assert excess_near_peak(mean_profile(prof0, hits0)) < 0.5              # 11 bins of drift without it
    # away from PEPOCH = tstart the factor stretches the whole elapsed time: still the restatement
    par2 = dict(par, PEPOCH=HDR_LONG["tstart"] - 2.0, F1=-3e-7)
    prof2, hits2, _ = post.fold_all(fil, par2, doppler=-3e-5, nbin=nbin, subint_s=8.0, apply_delays=True, lib=emu_lib)
    wp2, wh2 = fo.fold_all(x, nbin=nbin, subint_s=8.0, f0=F0, f1=-3e-7, pepoch_mjd=par2["PEPOCH"], doppler=-3e-5,
                           **model_kw(HDR_LONG))
    check_equal(8, prof2, hits2, wp2, wh2)


# ---- known answer for the predictor --------------------------------------------------------------------------------
def test_cubic_polyco_known_answer(emu_lib):
    """a train whose arrival phases follow a polyco with a cubic term: 20 turns / min^3 over +-0.25 min leaves, after the
    best quadratic, 0.8 x 20 x 0.25^3 = 0.25 turns peak to peak = 32 of 128 bins"""
    nrows, nbin = 117000, 128
    tmid = HDR_LONG["tstart"] + 15.0 / 86400.0
    seg = dict(tmid=tmid, rphase=0.37, f0=F0, span=1.0, coeff=[0.2, 0.05, -0.4, 20.0], site="g")
    sec = np.arange(nrows) * HDR_LONG["tsamp"]
    turns = fo.polyco_turns(seg, HDR_LONG["tstart"], sec)
    q = np.polyfit(sec, turns, 2)
    resid = turns - np.polyval(q, sec)
    assert (resid.max() - resid.min()) * nbin > 8                          # beyond any F0 / F1
    x = train_from_turns(turns, 4, 16)
    x[:, 1] //= 2                                                          # the products differ
    # the restatement first: the predictor holds the pulse in place
    wp, wh = fo.fold_all(x, nbin=nbin, subint_s=8.0, segs=[seg], **model_kw(HDR_LONG))
    assert excess_near_peak(mean_profile(wp, wh)) >= 0.9
    fil = as_fil_all(x, HDR_LONG, 8)
    par = dict(F0=F0, F1=0.0, PEPOCH=None, DM=0.0, PSR="x")
    prof, hits, _ = post.fold_all(fil, par, polyco=[seg], nbin=nbin, subint_s=8.0, lib=emu_lib)
    check_equal(8, prof, hits, wp, wh)
    for p in range(4):
        assert excess_near_peak(mean_profile(prof, hits, p)) >= 0.9
    assert abs(int(np.argmax(mean_profile(prof, hits))) - int(0.3 * nbin)) <= 1       # phi0 = 0.3 by construction
    # the best-fit F0 / F1 through the untouched single-product fold: smeared
    best = dict(F0=float(q[1]), F1=float(2.0 * q[0]), PEPOCH=None, DM=0.0, PSR="x")
    one = sigproc.SigprocFile(header=dict(HDR_LONG, nbits=8, nifs=1), header_bytes=0, data=np.ascontiguousarray(x[:, :1]))
    p1, h1, _ = post.fold(one, best, nbin=nbin, subint_s=8.0, lib=emu_lib)
    assert excess_near_peak(p1.sum(axis=(0, 1)) / h1.sum(axis=(0, 1))) < 0.5


# ---- read_polyco ---------------------------------------------------------------------------------------------------
POLYCO_TEXT = """\
0332+5434   7-Apr-20  120000.00   58946.50000000000            26.764  0.123 -6.789
       10000000000.123456789        1.399541538720    g  120   12  1400.000   0.2512  13.2907
  1.23456789012345678D-05 -2.34567890123456789D-01  3.45678901234567890D-03
 -4.56789012345678901D-05  5.67890123456789012D-07 -6.78901234567890123D-09
  7.89012345678901234D-11 -8.90123456789012345D-13  9.01234567890123456D-15
 -1.01234567890123456D-16  1.11234567890123456D-18 -1.21234567890123456D-20
0332+5434   7-Apr-20  140000.00   58946.58333333333            26.764  0.124 -6.701
             -12345.75              1.399541538720    g  120    2  1400.000
  1.5D+00 -2.5e-01
"""


def test_read_polyco_round_trip(tmp_path):
    f = tmp_path / "polyco.dat"
    f.write_text(POLYCO_TEXT)
    a, b = post.read_polyco(str(f))
    assert a["psr"] == "0332+5434" and a["tmid"] == 58946.5 and a["dm"] == 26.764 and a["doppler"] == 0.123 and a["log10rms"] == -6.789
    assert abs(a["rphase"] - 0.123456789) < 1e-9 and a["rphase_turns"] == 10000000000      # float(1e10 + .123456789) keeps 1e-6 only
    assert a["f0"] == 1.39954153872 and a["site"] == "g" and a["span"] == 120.0 and a["ncoeff"] == 12 and a["obsfreq"] == 1400.0
    assert a["binphase"] == 0.2512 and a["binfreq"] == 13.2907
    assert len(a["coeff"]) == 12 and a["coeff"][0] == 1.23456789012345678e-05 and a["coeff"][11] == -1.21234567890123456e-20
    assert a["coeff"][4] == 5.67890123456789012e-07
    assert b["tmid"] == 58946.58333333333 and b["rphase"] == 0.25 and b["rphase_turns"] == -12346       # fraction in [0, 1)
    assert b["ncoeff"] == 2 and b["coeff"] == [1.5, -0.25] and b["binphase"] is None and b["binfreq"] is None
    bad = tmp_path / "bad.dat"
    bad.write_text("\n".join(POLYCO_TEXT.splitlines()[:4]) + "\n")                             # coefficients cut short
    with pytest.raises(post.InputError):
        post.read_polyco(str(bad))


def test_polyco_file_folds_like_its_blocks(emu_lib, tmp_path):
    """read_polyco -> fold_all: a written file gives the fold of the blocks it states (D exponents, 1e10-turn RPHASE)"""
    segs = three_blocks(HDR)
    lines = []
    for k, g in enumerate(segs):
        lines.append("J0000+00  1-Jan-20  000000.00  %.15f  56.7  0.0 -6.0" % g["tmid"])
        lines.append("  %d%s  %.12f  g  %g  %d  1400.0" % (10 ** 10 + k, ("%.12f" % g["rphase"])[1:], g["f0"], g["span"], len(g["coeff"])))
        cs = [("%.17e" % c).replace("e", "D") for c in g["coeff"]]
        lines += ["  ".join(cs[i:i + 3]) for i in range(0, len(cs), 3)]
    f = tmp_path / "polyco.dat"
    f.write_text("\n".join(lines) + "\n")
    back = post.read_polyco(str(f))
    for g, r in zip(segs, back):
        assert r["tmid"] == float("%.15f" % g["tmid"]) and r["coeff"] == g["coeff"] and abs(r["rphase"] - g["rphase"]) < 1e-12
    x = random_rows(9000, 4, 64, 8, seed=12)
    prof, hits, _ = post.fold_all(as_fil_all(x, HDR, 8), PAR, polyco=str(f), nbin=64, subint_s=0.2, lib=emu_lib)
    wp, wh = fo.fold_all(x, nbin=64, subint_s=0.2, segs=back, **model_kw(HDR))
    check_equal(8, prof, hits, wp, wh)


# ---- errors --------------------------------------------------------------------------------------------------------
def test_model_errors(emu_lib):
    fil = as_fil_all(random_rows(9000, 4, 64, 8), HDR, 8)
    kw = dict(nbin=64, subint_s=0.2, lib=emu_lib)
    with pytest.raises(post.InputError, match="outside the span"):
        post.fold_all(fil, PAR, polyco=three_blocks(HDR, span_min=0.002), **kw)            # 0.12 s blocks 0.2 s apart: the last row
    late = three_blocks(HDR, offsets_s=(100.0, 100.2, 100.4), span_min=1.0)
    with pytest.raises(post.InputError, match="the first row lies outside the span"):
        post.fold_all(fil, PAR, polyco=late, **kw)
    with pytest.raises(post.InputError, match="ncoeff"):
        post.fold_all(fil, PAR, polyco=[dict(three_blocks(HDR)[0], coeff=[0.0] * 16)], **kw)
    with pytest.raises(post.InputError, match="ncoeff"):
        post.fold_all(fil, PAR, polyco=[dict(three_blocks(HDR)[0], coeff=[])], **kw)
    with pytest.raises(post.InputError, match="ascending"):
        post.fold_all(fil, PAR, polyco=three_blocks(HDR)[::-1], **kw)
    with pytest.raises(post.InputError, match="doppler together with a polyco"):
        post.fold_all(fil, PAR, polyco=three_blocks(HDR), doppler=1e-4, **kw)
    with pytest.raises(post.InputError):
        post.fold_all(fil, dict(PAR, F0=-1.0), **kw)
    m, _keep = post.fold_model(PAR, fil.header, nbin=64, subint_s=0.2, apply_delays=False)
    m.size -= 8                                                                            # another layout of the struct
    desc = post.fil_desc(fil.header)
    err = C.create_string_buffer(256)
    out, hits = np.zeros((3, 4, 64, 64)), np.zeros((3, 64, 64), np.uint32)
    rows = fil.data
    assert emu_lib.frbch_foldp_host(C.byref(desc), rows.ctypes.data, rows.shape[0], C.byref(m), 0, out.ctypes.data,
                                    hits.ctypes.data, 3, None, err, len(err)) == _lib.E_ARG and b"size" in err.value


# ---- Stokes parameters ---------------------------------------------------------------------------------------------
def test_stokes_formulas_and_position_angle(emu_lib):
    """rows with known PP, QQ, Re(PQ*), Im(PQ*): the I, Q, U, V of include/frbch.h; a pulse linearly polarised at angle psi
    (Q = L cos 2 psi, U = L sin 2 psi) returns PA = psi"""
    nrows, nchan, nbin, psi = 9000, 8, 64, np.radians(-35.0)
    hdr = dict(HDR, nchans=nchan)
    on = fo.bins(nrows, 1, nbin=nbin, f0=F0, **model_kw(hdr)) == 20                        # the rows of bin 20, [nrows][1]
    i_on, l_on, v_on = 8.0, 5.0, -2.0
    x = np.empty((nrows, 4, nchan), dtype=np.float32)
    x[:, 0] = 3.0 + on * 0.5 * (i_on + v_on)                                               # PP = (I + V) / 2
    x[:, 1] = 2.0 + on * 0.5 * (i_on - v_on)                                               # QQ = (I - V) / 2
    x[:, 2] = 1.0 + on * 0.5 * l_on * np.cos(2 * psi)                                      # Re(PQ*) = Q / 2
    x[:, 3] = 0.5 + on * 0.5 * l_on * np.sin(2 * psi)                                      # Im(PQ*) = U / 2
    par = dict(F0=F0, F1=0.0, PEPOCH=None, DM=0.0, PSR="x")
    prof, hits, _ = post.fold_all(as_fil_all(x, hdr, 32), par, nbin=nbin, subint_s=10.0, lib=emu_lib)
    s = post.stokes(prof, "coherency")
    assert s.shape == prof.shape
    assert np.array_equal(s[:, 0], prof[:, 0] + prof[:, 1]) and np.array_equal(s[:, 3], prof[:, 0] - prof[:, 1])
    assert np.array_equal(s[:, 1], 2.0 * prof[:, 2]) and np.array_equal(s[:, 2], 2.0 * prof[:, 3])
    mean = s.sum(axis=(0, 2)) / hits.sum(axis=(0, 1))                                      # [4][nbin]
    off = np.array([5.0, 2.0, 1.0, 1.0])                                                   # I, Q, U, V of the floor
    np.testing.assert_allclose(mean[:, 3], off, rtol=1e-6)
    np.testing.assert_allclose(mean[:, 20] - off, [i_on, l_on * np.cos(2 * psi), l_on * np.sin(2 * psi), v_on], rtol=1e-5)
    i, l, v, pa = post.linear_pa(mean)
    assert abs(pa[20] - psi) < 1e-6 and abs(l[20] - l_on) < 1e-5 and abs(v[20] - v_on) < 1e-5 and abs(i[20] - i_on) < 1e-5
    assert np.abs(l[np.arange(nbin) != 20]).max() < 1e-5
    assert post.stokes(prof, "stokes") is prof                                             # an IQUV file passes through
    with pytest.raises(post.InputError):
        post.stokes(prof[:, :2])
    with pytest.raises(post.InputError):
        post.stokes(prof, "linear")


# ---- fold_fil ------------------------------------------------------------------------------------------------------
def write_fil(path, x, hdr, nifs):
    from oracle import frb_oracle as o
    head = o.sigproc_header(telescope="effelsberg", source="J0000+00", ra="01:23:45.6", dec="-12:34:56.7", rawdatafile="x",
                            tstart_mjd=hdr["tstart"], tsamp_s=hdr["tsamp"], nbits=8, fch1=hdr["fch1"], foff=hdr["foff"],
                            nchans=hdr["nchans"], nifs=nifs)
    with open(path, "wb") as f:
        f.write(head + x.tobytes())


def png_pixels(path):
    """(width, height, sha256 of the decompressed image data)"""
    buf = open(path, "rb").read()
    assert buf[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(buf):
        (n,) = struct.unpack_from(">I", buf, pos)
        tag, data = buf[pos + 4: pos + 8], buf[pos + 8: pos + 8 + n]
        if tag == b"IHDR":
            size = struct.unpack(">II", data[:8])
        elif tag == b"IDAT":
            idat += data
        pos += 12 + n
    return size[0], size[1], hashlib.sha256(zlib.decompress(idat)).hexdigest()


def test_fold_fil_full_polarisation(emu_lib, tmp_path):
    """a four-product file: archive with nprod = 4 that reads back, the 2x2 plot of base2fil.sh:483-490, I / L / V / PA columns"""
    rng = np.random.default_rng(6)
    nrows, nchan = 12000, 64
    m = np.zeros((nrows, 1), dtype=np.int64)                                               # one-sample pulses at the centre of bin 32
    k = np.arange(int(nrows * HDR["tsamp"] / P0))
    m[np.rint((k + 32.5 / 128) * P0 / HDR["tsamp"]).astype(int)] = 1
    n = rng.integers(96, 104, size=(4, nrows, nchan))
    x = np.stack([n[0] + 60 * m, n[1] + 30 * m, n[2] + 24 * m, n[3] - 24 * m], axis=1).astype(np.uint8)   # PP, QQ, Re, Im
    fil = str(tmp_path / "pr001a_ef_no0001_IFall_vdif_pol4.fil")
    write_fil(fil, x, HDR, 4)
    par = tmp_path / "J0000+00.psrcat.par"
    par.write_text("PSRJ J0000+00\nP0 %.6f\nDM 0.0\n" % P0)
    ar, profile = post.fold_fil(fil, str(par), nbin=128, subint_s=0.3, lib=emu_lib)
    prof, hits, meta = post.read_archive(ar)
    assert meta["nprod"] == 4 and meta["products"] == "coherency" and prof.shape == (3, 4, 64, 128) and hits.shape == (3, 64, 128)
    wp, wh = fo.fold_all(x, nbin=128, subint_s=0.3, f0=1.0 / float("%.6f" % P0), **model_kw(HDR))
    assert np.array_equal(prof, wp) and np.array_equal(hits, wh)
    w, h, _ = png_pixels(fil + "_fullPol.png")
    assert w == 2 * 128 + 4 and h >= 2 * 64 + 4
    assert png_pixels(fil + ".png")[0] == 128
    txt = open(fil + ".profile.txt").read().splitlines()
    assert len(txt) == 129 and txt[0].startswith("# bin  mean_sample  I  L  V  PA_deg")
    cols = np.array([[float(v) for v in ln.split()] for ln in txt[1:]])
    peak = int(np.argmax(profile))
    assert abs(peak - 32) <= 1 and int(np.argmax(cols[:, 2])) == peak
    # I = 90, Q = 2 Re = 48, U = 2 Im = -48 per pulse: L = 68 = 0.75 I at PA = -22.5 degrees; V = PP - QQ = 30 = I / 3
    assert abs(cols[peak, 5] + 22.5) < 2.0 and cols[peak, 3] > 0.6 * cols[peak, 2] and cols[peak, 4] > 0.2 * cols[peak, 2]
    # the same rows declared as I, Q, U, V: Stokes I is product 0 as it stands
    ar2, profile2 = post.fold_fil(fil, str(par), nbin=128, subint_s=0.3, lib=emu_lib, products="stokes", out_base=str(tmp_path / "iquv"))
    p0 = prof[:, 0].sum(axis=(0, 1)) / hits.sum(axis=(0, 1))
    np.testing.assert_allclose(profile2, p0, rtol=1e-12)
    assert os.path.exists(str(tmp_path / "iquv_fullPol.png"))


# outputs of the parent commit's fold_fil for the file of test_single_product_outputs_are_unchanged (recorded results)
PARENT_SHA256 = {
    "ar": "33bbb36e971d9958332622c13ba0e7604f40620de6f372859915bb9357b8af6a",
    "profile.txt": "6b4a1f7041076dc9469482bf12f3cc9fe446fda0d9253af64c8881bb8479668b",
    "png": "128 x 72 abc1220b6720d8b4a2e460792a1b5a8b092ccdbf520af5da38b209dfe7051fcc",
}


def test_single_product_outputs_are_unchanged(emu_lib, tmp_path):
    """a one-product file: .ar and .profile.txt byte for byte, and the .png pixel for pixel, what fold_fil wrote before
    the all-product path existed; no _fullPol.png"""
    x = pulse_train_rows(12000, HDR)
    fil = str(tmp_path / "pr001a_ef_no0001_IFall_vdif_pol2.fil")
    write_fil(fil, x, HDR, 1)
    par = tmp_path / "J0000+00.psrcat.par"
    par.write_text("PSRJ J0000+00\nP0 %.6f\nDM %.1f\n" % (P0, DM0))
    post.fold_fil(fil, str(par), nbin=128, subint_s=0.3, lib=emu_lib)
    assert hashlib.sha256(open(fil + ".ar", "rb").read()).hexdigest() == PARENT_SHA256["ar"]
    assert hashlib.sha256(open(fil + ".profile.txt", "rb").read()).hexdigest() == PARENT_SHA256["profile.txt"]
    assert "%d x %d %s" % png_pixels(fil + ".png") == PARENT_SHA256["png"]
    assert not os.path.exists(fil + "_fullPol.png")
    # the same file through the all-product path (a Doppler factor too small to move a sample): the same archive payload
    prof, hits, meta = post.read_archive(fil + ".ar")
    post.fold_fil(fil, str(par), nbin=128, subint_s=0.3, lib=emu_lib, doppler=1e-300, out_base=str(tmp_path / "dop"))
    prof2, hits2, meta2 = post.read_archive(str(tmp_path / "dop.ar"))
    assert "nprod" not in meta2 and "Doppler" in meta2["timing"]
    assert np.array_equal(prof, prof2) and np.array_equal(hits, hits2)


def test_cli_takes_the_new_options(monkeypatch, tmp_path):
    seen = {}
    monkeypatch.setattr(post, "fold_fil", lambda *a, **k: seen.update(a=a, k=k) or ("x.ar", np.zeros(4)))
    post.main(["fold", "a.fil", "b.par", "--polyco", "polyco.dat", "--products", "stokes"])
    assert seen["a"] == ("a.fil", "b.par") and seen["k"]["polyco"] == "polyco.dat" and seen["k"]["products"] == "stokes"
    post.main(["fold", "a.fil", "b.par", "--doppler", "1e-4"])
    assert seen["k"]["doppler"] == 1e-4 and seen["k"]["polyco"] is None and seen["k"]["products"] == "coherency"
