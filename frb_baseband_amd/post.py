"""After the filterbank: GPU incoherent dedispersion (the reference's `prepdata` stage) and GPU phase fold (the
reference's `dspsr -E <par> ... <IFall.fil>` stage) of SIGPROC filterbank files, through the C ABI (include/frbch.h).

* ``prepdata_gpu`` mirrors ``process_vdif.prepdata`` (process_vdif.py:202-229): same arguments, same output names
  (PRESTO's ``<outfile>.dat`` / ``.inf`` for one DM, ``<outfile>_DM<dm>.dat`` / ``.inf`` for a DM range), data
  dedispersed on the GPU instead of by PRESTO.  `-nobary -noweights -noscales` are what the reference always passes:
  topocentric, unweighted.
* ``search_fil`` / ``candidates_fil`` search the DM range for single pulses, join the records of a pulse across DMs and cut
  the frequency-time and DM-time planes a FETCH-style classifier reads (the hand-over of base2fil.sh:118-122, 425-432).
* ``psearch_fil`` searches the same DM range for PERIODIC signals (``periodicity_search``: frbch_psearch_host; one long
  transform per series, red-noise normalisation, harmonic sums, peaks), joins the records across DMs (``group_periodic``)
  and can fold the strongest candidates at their own frequency and DM: from a filterbank to a period without an ephemeris.
* ``fold_fil`` mirrors base2fil.sh:465-493: spin parameters from a psrcat-style .par file, 10-s sub-integrations,
  the filterbank's channels, plus the plot (PNG) of the dedispersed, time- and frequency-scrunched profile that
  ``psrplot -pF ... -j dedisperse,tscrunch,pscrunch,"fscrunch 128"`` draws.  Files with several products (``--pol 4``)
  are folded in ALL products in one pass (``fold_all``), optionally with the TEMPO polyco predictor that tempo / tempo2
  make from the .par file (``read_polyco``: barycentric, binary and position terms, as dspsr folds) or a constant
  Doppler factor, and give the 2x2 full-polarisation plot of base2fil.sh:481-491 as well.
* ``rfifind_fil`` / ``clean`` flag interference per (block of rows, channel) from block statistics taken on the GPU, write
  and read the flag file the reference carries to Heimdall and FETCH (create_config.py:54-56 ``-F/--flag``), and replace the
  masked samples: ``search_fil`` and ``candidates_fil`` take ``flag_file`` / ``rfi`` and then work on the cleaned rows.
  ``periodic`` (``--periodic``) adds the periodicity test: the largest bin of the power spectrum of every cell
  (``rfi_peaks``: frbch_rfi_peaks_host) against a threshold (``rfi_periodic``, ``t_pow_of``), for interference too weak for
  the test on mean and std that still adds up in every dedispersed series.
* ``resident=True`` (``--resident``) of ``search_fil``, ``candidates_fil`` and ``rfifind_fil``: the rows cross to the device
  once per command and stay there from flagging to cut-outs (``candidates_resident``: frbch_candidates_host; ``cleanp``:
  frbch_rfi_cleanp_host); the files and the returned values are those of the default path, byte for byte.
* ``rmsynth_fil`` (``post rmsynth``) answers what a full-Stokes file is written for: the on-pulse minus off-pulse spectra of all
  four products of every burst (``burst_spectra``: frbch_burstspec_host), the Faraday dispersion function of Q and U by an
  integer, bit-reproducible transform (``rm_synthesis``: frbch_rmsynth_host), its peak -- the rotation measure -- with PA0,
  L/I and V/I (``rm_peaks``), or all of it on rows uploaded once (``burst_rm``: frbch_burst_rm_host).
* ``polprof_fil`` (``post polprof``, ``post rmsynth --profile``) draws the burst against time at that RM: I, debiased L, V and the
  position angle per time bin, (Q, U) of every channel rotated back and summed over the band (``pol_profile``: frbch_polprof_host).
* ``polcal_fil`` (``post polcal``) measures what both need first with dual circular feeds, the delay between the R and L paths,
  on the pulses of a calibrator of known RM: RM synthesis at a grid of trial delays (``rm_delay``: frbch_rmdelay_host), the peak
  of the (delay, RM) plane with the slope of its ridge and one combined estimate (``rm_delay_peaks``), or all of it on rows
  uploaded once (``polcal``: frbch_burst_polcal_host); ``post rmsynth`` and ``post polprof`` take the result with ``--polcal``.
* ``dmfit_fil`` (``post dmfit``) measures the DM those stages take as given: the burst's noise-weighted profile at a fine grid of
  trial DMs, the S/N- and the structure-maximising DM by a parabola over each curve's peak (``dm_scan``: frbch_dmscan_host);
  ``post rmsynth`` and ``post polprof`` take the result with ``--dm-from``.
* ``burstacf_fil`` (``post burstacf``) keeps frequency and time together: the dedispersed, noise-weighted dynamic spectrum of a
  burst, its two-dimensional autocorrelation in exact integers, and from it the scintillation bandwidth, the sub-burst duration
  and the drift of sub-bursts in frequency (``burst_acf``: frbch_burstacf_host).
* ``burstscat_fil`` (``post scatter``) fits a pulse shape: every subband of that dynamic spectrum is correlated with a bank of
  Gaussians convolved with one-sided exponentials at every trial arrival bin, in exact integers; the best template gives the
  subband's scattering time, and tau(nu) = tau_ref (nu / nu_ref)^-alpha is fitted across the band (``burst_scatter``:
  frbch_burstscat_host).
There is no CPU fallback: the sums run in libfrbch.so on a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import struct
import zlib

import numpy as np

from . import _lib, sigproc
from .channeliser import InputError, RunError

DM_CONST = 1.0 / 2.41e-4      # s MHz^2 per pc cm^-3 (DSPSR / PRESTO)


def fil_desc(hdr: dict, product: int = 0) -> _lib.FrbchFilDesc:
    d = _lib.FrbchFilDesc()
    d.size = C.sizeof(_lib.FrbchFilDesc)
    d.nchan = hdr["nchans"]
    d.nifs = hdr.get("nifs", 1)
    d.nbits = hdr["nbits"]
    d.product = product
    d.fch1_mhz = hdr["fch1"]
    d.foff_mhz = hdr["foff"]
    d.tsamp_s = hdr["tsamp"]
    d.tstart_mjd = hdr["tstart"]
    return d


def _rows_of(fil: sigproc.SigprocFile) -> np.ndarray:
    if fil.header["nbits"] not in (8, 16, 32):
        raise InputError(f"nbits = {fil.header['nbits']}: the GPU stages take 8-, 16-bit or float32 filterbanks")
    return np.ascontiguousarray(fil.data)


def _check(rc: int, err) -> None:
    if rc < 0:
        msg = err.value.decode() if err is not None else ""
        raise (InputError if rc == _lib.E_ARG else RunError)(f"{_lib.load().frbch_strerror(rc).decode()}: {msg}")


def dm_list(dm1: float, dm2: float = 0.0, dmstep: float = 1.0):
    """the DMs of process_vdif.prepdata: one, or numdms = int((dm2-dm1)//dmstep + 1) from dm1 (process_vdif.py:209-214)"""
    if dm2 > 0.0:
        if dm2 < dm1:
            raise InputError("DM2 must be larger than DM1.")
        numdms = int((dm2 - dm1) // dmstep + 1)
        return [dm1 + i * dmstep for i in range(numdms)]
    return [dm1]


def dedisperse(fil: sigproc.SigprocFile, dms, zerodm: bool = True, clip: float = 5.0, device: int = 0, lib=None):
    """-> (float32 [ndm][nout], number of clipped time samples)"""
    lib = lib or _lib.load()
    rows = _rows_of(fil)
    desc = fil_desc(fil.header)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    nout = lib.frbch_dedisperse_nout(C.byref(desc), rows.shape[0], dm_arr.ctypes.data, dm_arr.size)
    if nout <= 0:
        raise InputError("the dispersion delay across the band exceeds the length of the filterbank")
    out = np.empty((dm_arr.size, nout), dtype=np.float32)
    nclip = C.c_uint64(0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_dedisperse_host(C.byref(desc), rows.ctypes.data, rows.shape[0], dm_arr.ctypes.data, dm_arr.size,
                                     1 if zerodm else 0, float(clip), device, out.ctypes.data, nout, C.byref(nclip),
                                     err, len(err)), err)
    return out, nclip.value


def write_inf(path: str, *, basename: str, hdr: dict, nsamp: int, dm: float, clipped: int) -> None:
    """PRESTO .inf side file (the keys `readfile` / `accelsearch` read), topocentric"""
    lo = hdr["fch1"] + (hdr["nchans"] - 1) * hdr["foff"] if hdr["foff"] < 0 else hdr["fch1"]
    bw = abs(hdr["foff"]) * hdr["nchans"]
    lines = [
        (" Data file name without suffix", basename),
        (" Telescope used", "Unknown"),
        (" Instrument used", "frbch (MI355X)"),
        (" Object being observed", hdr.get("source_name", "Unknown")),
        (" J2000 Right Ascension (hh:mm:ss.ssss)", _sex(hdr.get("src_raj", 0.0))),
        (" J2000 Declination     (dd:mm:ss.ssss)", _sex(hdr.get("src_dej", 0.0))),
        (" Data observed by", "unset"),
        (" Epoch of observation (MJD)", "%.15f" % hdr["tstart"]),
        (" Barycentered?           (1=yes, 0=no)", "0"),
        (" Number of bins in the time series", str(nsamp)),
        (" Width of each time series bin (sec)", "%.15g" % hdr["tsamp"]),
        (" Any breaks in the data? (1=yes, 0=no)", "0"),
        (" Type of observation (EM band)", "Radio"),
        (" Beam diameter (arcsec)", "0"),
        (" Dispersion measure (cm-3 pc)", "%.12g" % dm),
        (" Central freq of low channel (MHz)", "%.12g" % (lo - 0.0)),
        (" Total bandwidth (MHz)", "%.12g" % bw),
        (" Number of channels", str(hdr["nchans"])),
        (" Channel bandwidth (MHz)", "%.12g" % abs(hdr["foff"])),
        (" Data analyzed by", "frb_baseband_amd"),
        (" Any additional notes", "\n    GPU incoherent dedispersion, %d time samples clipped" % clipped),
    ]
    with open(path, "w") as f:
        for key, val in lines:
            f.write("%-40s=  %s\n" % (key, val))


def _sex(packed: float) -> str:
    sign = "-" if packed < 0 else ""
    p = abs(packed)
    hh = int(p // 10000)
    mm = int((p - hh * 10000) // 100)
    ss = p - hh * 10000 - mm * 100
    return "%s%02d:%02d:%07.4f" % (sign, hh, mm, ss)


def prepdata_gpu(filterbankfile, dm1, zerodm=True, clip=5, dm2=0, dmstep=1.0, ncpus=1, device=0, lib=None):
    """GPU replacement of process_vdif.prepdata (same signature; ``ncpus`` is accepted and ignored).  Returns the list of
    .dat files written."""
    fil = sigproc.read_fil(filterbankfile)
    dms = dm_list(dm1, dm2, dmstep)
    series, nclip = dedisperse(fil, dms, zerodm=zerodm, clip=float(clip), device=device, lib=lib)
    if dm2 > 0.0:
        base = filterbankfile.replace(".fil", "")
        names = ["%s_DM%.2f" % (base, dm) for dm in dms]          # prepsubband's naming
    else:
        names = [filterbankfile.replace(".fil", "_dm{0}".format(dm1))]   # process_vdif.py:216
    out = []
    for name, dm, y in zip(names, dms, series):
        y.astype("<f4").tofile(name + ".dat")
        write_inf(name + ".inf", basename=os.path.basename(name), hdr=fil.header, nsamp=y.size, dm=dm, clipped=nclip)
        out.append(name + ".dat")
    return out


# ------------------------------------------------------------------------------------------------------------------
# interference: block statistics, the mask, the flag file, cleaned rows
# ------------------------------------------------------------------------------------------------------------------
RFI_DEFAULTS = dict(block_rows=1024, t_cell=5.0, t_chan=5.0, chan_frac=0.3, block_frac=0.3)


def rfi_params(params=None) -> _lib.FrbchRfiParams:
    """``RFI_DEFAULTS`` overridden by the dict ``params`` (``True`` / ``None``: the defaults) as the library's struct"""
    if isinstance(params, _lib.FrbchRfiParams):
        return params
    kw = dict(RFI_DEFAULTS)
    if isinstance(params, dict):
        unknown = set(params) - set(kw)
        if unknown:
            raise InputError("unknown flagging parameters: " + ", ".join(sorted(unknown)))
        kw.update(params)
    if not 0 <= int(kw["block_rows"]) < 1 << 32:
        raise InputError("block_rows must be a non-negative 32-bit integer")
    p = _lib.FrbchRfiParams()
    p.size = C.sizeof(_lib.FrbchRfiParams)
    p.block_rows = int(kw["block_rows"])
    p.t_cell, p.t_chan, p.chan_frac, p.block_frac = (float(kw[k]) for k in ("t_cell", "t_chan", "chan_frac", "block_frac"))
    return p


def read_flag_file(path: str, nchan: int) -> np.ndarray:
    """Flag file -> bool [nchan], True = flagged.  Tokens separated by whitespace, commas or newlines; a token is a channel
    index ``a`` or an inclusive range ``a:b`` / ``a-b``, in the FILE's channel order (index 0 = fch1); ``#`` starts a
    comment.  The reference only passes the path on (base2fil.sh:425-432): the format Heimdall and FETCH take at a given
    site is not pinned by it -- this function and ``write_flag_file`` are the two to adapt."""
    flags = np.zeros(nchan, dtype=bool)
    with open(path) as f:
        for line in f:
            for tok in line.split("#", 1)[0].replace(",", " ").split():
                parts = tok.replace("-", ":").split(":")
                try:
                    a, b = (int(parts[0]), int(parts[-1])) if len(parts) in (1, 2) else (None, None)
                except ValueError:
                    a = b = None
                if a is None or a > b:
                    raise InputError(f"{path}: bad token '{tok}' (a channel index a, or a range a:b / a-b)")
                if b >= nchan:
                    raise InputError(f"{path}: token '{tok}' names a channel outside 0..{nchan - 1}")
                flags[a: b + 1] = True
    return flags


def write_flag_file(path: str, chan_flag) -> None:
    """the wholly flagged channels as ``a`` / ``a:b`` tokens, one per line, in the format ``read_flag_file`` reads"""
    flags = np.asarray(chan_flag).astype(bool)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], flags.astype(np.int8), [0]])))
    with open(path, "w") as f:
        f.write("# flagged channels (file order, inclusive ranges a:b): %d of %d\n" % (int(flags.sum()), flags.size))
        for a, b in zip(edges[0::2], edges[1::2] - 1):
            f.write("%d\n" % a if a == b else "%d:%d\n" % (a, b))


def _rows3(rows, hdr: dict) -> np.ndarray:
    """rows as a C-contiguous [nrows][nifs][nchans] array of the header's sample type"""
    rows = np.ascontiguousarray(rows)
    nifs, nchan = hdr.get("nifs", 1), hdr["nchans"]
    if hdr["nbits"] not in (8, 16, 32) or rows.dtype.itemsize * 8 != hdr["nbits"] or rows.size == 0 or rows.size % (nifs * nchan):
        raise InputError("the rows do not match the header's nbits / nchans / nifs (8-, 16-bit or float32 rows)")
    return rows.reshape(-1, nifs, nchan)


def _zap_array(zap, nchan: int):
    """``zap`` as the library's uint8 [nchan] mask.  A bool or uint8 array of shape [nchan] IS a mask (non-zero = flagged;
    what this function returns is one, so a second pass changes nothing); anything else is a list of channel indices."""
    if zap is None:
        return None
    z = np.asarray(zap)
    if z.dtype in (np.dtype(bool), np.dtype(np.uint8)) and z.shape == (nchan,):
        return np.ascontiguousarray(z != 0, dtype=np.uint8)
    if z.size and z.dtype.kind not in "iu":
        raise InputError("zap: a bool / uint8 mask of nchans entries, or a list of integer channel indices")
    idx = z.astype(np.int64).ravel()
    if idx.size and (idx.min() < 0 or idx.max() >= nchan):
        raise InputError(f"zap: a channel outside 0..{nchan - 1}")
    out = np.zeros(nchan, dtype=np.uint8)
    out[idx] = 1
    return out


def rfi_stats(rows, hdr: dict, params=None, product: int = 0, device: int = 0, lib=None, info: dict | None = None) -> np.ndarray:
    """Block statistics of one product (frbch_rfi_stats_host) -> [nblk][nchan][2] = (sum x, sum x^2): uint64 for integer
    rows, float64 for float rows.  ``info['kernel_used']``: 1 = the fast kernel, 0 = the generic one."""
    lib = lib or _lib.load()
    x = _rows3(rows, hdr)
    par = rfi_params(params)
    desc = fil_desc(hdr, product)
    nblk = lib.frbch_rfi_nblk(x.shape[0], par.block_rows)
    if nblk <= 0:
        raise InputError("block_rows must be 1..2^20")
    stats = np.zeros((nblk, hdr["nchans"], 2), dtype=np.float64 if hdr["nbits"] == 32 else np.uint64)
    used = C.c_uint32(0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_rfi_stats_host(C.byref(desc), x.ctypes.data, x.shape[0], C.byref(par), device, stats.ctypes.data, C.byref(used),
                                    err, len(err)), err)
    if info is not None:
        info["kernel_used"] = used.value
    return stats


def rfi_mask(stats, hdr: dict, nrows: int, params=None, zap=None, prior=None, product: int = 0, lib=None) -> dict:
    """The mask decision (frbch_rfi_mask, host only; include/frbch.h states the rule) -> dict(mask uint8 [nblk][nchan],
    repl float64 [nchan], chan_flag bool [nchan], blk_flag bool [nblk])."""
    lib = lib or _lib.load()
    par = rfi_params(params)
    desc = fil_desc(hdr, product)
    nchan = hdr["nchans"]
    st = np.ascontiguousarray(stats, dtype=np.float64 if hdr["nbits"] == 32 else np.uint64)
    if st.ndim != 3 or st.shape[1:] != (nchan, 2):
        raise InputError("stats must be [nblk][nchans][2]")
    nblk = st.shape[0]
    z = _zap_array(zap, nchan)
    pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.uint8)
    if pr is not None and pr.shape != (nblk, nchan):
        raise InputError("prior must be [nblk][nchans]")
    mask, repl = np.zeros((nblk, nchan), np.uint8), np.zeros(nchan, np.float64)
    cf, bf = np.zeros(nchan, np.uint8), np.zeros(nblk, np.uint8)
    err = C.create_string_buffer(512)
    _check(lib.frbch_rfi_mask(C.byref(desc), st.ctypes.data, nblk, int(nrows), C.byref(par), None if z is None else z.ctypes.data,
                              None if pr is None else pr.ctypes.data, mask.ctypes.data, repl.ctypes.data, cf.ctypes.data,
                              bf.ctypes.data, err, len(err)), err)
    return dict(mask=mask, repl=repl, chan_flag=cf.astype(bool), blk_flag=bf.astype(bool))


PEAK = np.dtype([("num", "<f4"), ("k", "<u4")])                 # frbch_rfi_peak


def t_pow_of(sigma: float, n: int) -> float:
    """The normalised spectral power that one of the n/2 - 1 bins of a noise cell (each exponentially distributed with mean 1)
    exceeds with the one-sided probability of ``sigma`` Gaussian sigma: -ln(q / (n/2 - 1)), q = erfc(sigma / sqrt 2) / 2."""
    import math
    if n < 8:
        raise InputError("t_pow_of: a transform of at least 8 rows")
    return -math.log(0.5 * math.erfc(float(sigma) / math.sqrt(2.0)) / (n // 2 - 1))


def _periodic_block(block_rows: int) -> int:
    n = int(block_rows)
    if not (8 <= n <= 4096 and n & (n - 1) == 0):
        raise InputError("the periodic test transforms whole blocks: block_rows must be a power of two in 8 .. 4096 (it is %d); "
                         "choose such a block_rows (1024 is the default) or leave the periodic test out" % n)
    return n


def rfi_fparams(periodic, par: _lib.FrbchRfiParams) -> _lib.FrbchRfiFparams:
    """``periodic``: ``True`` / ``dict(t_freq=4.0)`` (Gaussian sigma, turned into a power by ``t_pow_of``) or ``dict(t_pow=...)``,
    with an optional ``chan_frac`` (default: the time-domain one) -> the library's struct"""
    if isinstance(periodic, _lib.FrbchRfiFparams):
        return periodic
    kw = dict(periodic) if isinstance(periodic, dict) else {}
    unknown = set(kw) - {"t_freq", "t_pow", "chan_frac"}
    if unknown or ("t_freq" in kw and "t_pow" in kw):
        raise InputError("periodic: t_freq OR t_pow, and chan_frac" + (" (unknown: %s)" % ", ".join(sorted(unknown)) if unknown else ""))
    n = _periodic_block(par.block_rows)
    f = _lib.FrbchRfiFparams()
    f.size = C.sizeof(_lib.FrbchRfiFparams)
    f.t_pow = float(kw["t_pow"]) if "t_pow" in kw else t_pow_of(kw.get("t_freq", 4.0), n)
    f.chan_frac = float(kw.get("chan_frac", par.chan_frac))
    return f


def rfi_peaks(rows, hdr: dict, params=None, product: int = 0, device: int = 0, lib=None, info: dict | None = None,
              want_stats: bool = False):
    """The spectral peak of every (block, channel) cell of one product (frbch_rfi_peaks_host: one upload, the block statistics
    and the peaks) -> ``PEAK`` [nblk][nchan] (num = four times the largest power of the cell's own transform, k = its bin;
    {0, 0}: not tested), or (peaks, stats) with ``want_stats``.  ``info['kernel_used']``: (statistics, peaks), 1 = fast."""
    lib = lib or _lib.load()
    x = _rows3(rows, hdr)
    par = rfi_params(params)
    _periodic_block(par.block_rows)
    desc = fil_desc(hdr, product)
    nblk = lib.frbch_rfi_nblk(x.shape[0], par.block_rows)
    stats = np.zeros((nblk, hdr["nchans"], 2), dtype=np.float64 if hdr["nbits"] == 32 else np.uint64)
    peaks = np.zeros((nblk, hdr["nchans"]), dtype=PEAK)
    used = (C.c_uint32 * 2)(0, 0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_rfi_peaks_host(C.byref(desc), x.ctypes.data, x.shape[0], C.byref(par), device, stats.ctypes.data,
                                    peaks.ctypes.data, used, err, len(err)), err)
    if info is not None:
        info["kernel_used"] = (used[0], used[1])
    return (peaks, stats) if want_stats else peaks


def rfi_periodic(stats, peaks, hdr: dict, nrows: int, params=None, periodic=None, product: int = 0, lib=None) -> dict:
    """The decision on the peaks (frbch_rfi_periodic, host only; include/frbch.h states it) -> dict(pflag uint8 [nblk][nchan],
    pchan bool [nchan], power float64 [nblk][nchan], t_pow)."""
    lib = lib or _lib.load()
    par = rfi_params(params)
    fpar = rfi_fparams(periodic, par)
    desc = fil_desc(hdr, product)
    nchan = hdr["nchans"]
    st = np.ascontiguousarray(stats, dtype=np.float64 if hdr["nbits"] == 32 else np.uint64)
    pk = np.ascontiguousarray(peaks, dtype=PEAK)
    if st.ndim != 3 or st.shape[1:] != (nchan, 2) or pk.shape != st.shape[:2]:
        raise InputError("stats must be [nblk][nchans][2] and peaks [nblk][nchans]")
    nblk = st.shape[0]
    pflag, pchan, power = np.zeros((nblk, nchan), np.uint8), np.zeros(nchan, np.uint8), np.zeros((nblk, nchan), np.float64)
    err = C.create_string_buffer(512)
    _check(lib.frbch_rfi_periodic(C.byref(desc), st.ctypes.data, pk.ctypes.data, nblk, int(nrows), C.byref(par), C.byref(fpar),
                                  pflag.ctypes.data, pchan.ctypes.data, power.ctypes.data, err, len(err)), err)
    return dict(pflag=pflag, pchan=pchan.astype(bool), power=power, t_pow=fpar.t_pow)


def _clean_from_stats(lib, x, hdr, par, stats, prods, z, repl, device, priors=None):
    """The two passes of ``clean`` on statistics already taken: the mask of every listed product (with ``priors[i]``, the
    periodic flags of product i, as its ``prior``), their union, then frbch_rfi_mask per product with ``prior`` = the union
    and frbch_rfi_apply_host on ``x`` in place; ``repl[p]`` is filled.
    -> (mask, chan_flag, blk_flag)"""
    err = C.create_string_buffer(512)
    priors = priors or [None] * len(prods)
    first = [rfi_mask(st, hdr, x.shape[0], par, zap=z, prior=pr, product=p, lib=lib) for st, p, pr in zip(stats, prods, priors)]
    mask = np.bitwise_or.reduce([r["mask"] for r in first])
    cf = np.logical_or.reduce([r["chan_flag"] for r in first])
    bf = np.logical_or.reduce([r["blk_flag"] for r in first])
    for st, p, one in zip(stats, prods, first):
        r = one if len(prods) == 1 else rfi_mask(st, hdr, x.shape[0], par, zap=z, prior=mask, product=p, lib=lib)
        repl[p] = r["repl"]
        desc = fil_desc(hdr, p)
        _check(lib.frbch_rfi_apply_host(C.byref(desc), x.ctypes.data, x.shape[0], C.byref(par), mask.ctypes.data,
                                        repl[p].ctypes.data, device, err, len(err)), err)
    return mask, cf, bf


def _periodic_pass(lib, x, hdr, par, fpar, prods, device):
    """statistics and peaks of every listed product (one upload each) and the periodic decision on them
    -> (stats list, pflag list, dict(pflag, pchan, peaks [nifs][nblk][nchan], t_pow), statistics kernels, peaks kernels)"""
    stats, pflags, ks, kp = [], [], [], []
    peaks = None
    pchan = np.zeros(x.shape[2], bool)
    for p in prods:
        i = {}
        pk, st = rfi_peaks(x, hdr, par, product=p, device=device, lib=lib, info=i, want_stats=True)
        if peaks is None:
            peaks = np.zeros((x.shape[1],) + pk.shape, dtype=PEAK)
        peaks[p] = pk
        dec = rfi_periodic(st, pk, hdr, x.shape[0], par, fpar, product=p, lib=lib)
        stats.append(st)
        pflags.append(dec["pflag"])
        pchan |= dec["pchan"]
        ks.append(i["kernel_used"][0])
        kp.append(i["kernel_used"][1])
    return stats, pflags, dict(pflag=np.bitwise_or.reduce(pflags), pchan=pchan, peaks=peaks, t_pow=fpar.t_pow), ks, kp


def clean(rows, hdr: dict, params=None, zap=None, device: int = 0, lib=None, info: dict | None = None, products=None, periodic=None):
    """Flag and replace -> (cleaned copy of the rows, dict(mask [nblk][nchan], repl [nifs][nchan], chan_flag, blk_flag)).
    One product (``nifs = 1``, or ``products = [p]``): one frbch_rfi_clean_host call.  Several: pass one takes the mask of
    every product, the masks are ORed, pass two asks frbch_rfi_mask again per product with ``prior`` = the union -- all
    products are cleaned in the same cells, each with its own replacement values (frbch_rfi_apply_host per product).
    Products not listed keep their bytes.  ``info['kernel_used']``: the statistics kernel (the smallest over the products).
    ``periodic`` (``True``, ``dict(t_freq=4.0)`` or ``dict(t_pow=...)``, optionally with ``chan_frac``): the periodicity test as
    well -- one product: one frbch_rfi_cleanf_host call; several: pass one takes every product's spectral peaks and hands its
    periodic flags to frbch_rfi_mask as ``prior``.  The result gains ``pflag`` [nblk][nchan], ``pchan`` [nchan] (ORed over the
    products, and into ``chan_flag``), ``peaks`` [nifs][nblk][nchan] and ``t_pow``; ``info['peaks_kernel_used']``."""
    lib = lib or _lib.load()
    x = _rows3(rows, hdr).copy()
    par = rfi_params(params)
    nifs, nchan = x.shape[1], x.shape[2]
    prods = list(range(nifs)) if products is None else [int(p) for p in products]
    z = _zap_array(zap, nchan)
    err = C.create_string_buffer(512)
    repl = np.zeros((nifs, nchan), np.float64)
    kernels = []
    if periodic:
        fpar = rfi_fparams(periodic, par)
        if len(prods) == 1:
            nblk = lib.frbch_rfi_nblk(x.shape[0], par.block_rows)
            mask, cf, bf = np.zeros((nblk, nchan), np.uint8), np.zeros(nchan, np.uint8), np.zeros(nblk, np.uint8)
            pflag, pchan, peaks = np.zeros((nblk, nchan), np.uint8), np.zeros(nchan, np.uint8), np.zeros((nifs, nblk, nchan), PEAK)
            used = (C.c_uint32 * 2)(0, 0)
            desc = fil_desc(hdr, prods[0])
            _check(lib.frbch_rfi_cleanf_host(C.byref(desc), x.ctypes.data, x.shape[0], C.byref(par), C.byref(fpar),
                                             None if z is None else z.ctypes.data, device, mask.ctypes.data,
                                             repl[prods[0]].ctypes.data, cf.ctypes.data, bf.ctypes.data, pflag.ctypes.data,
                                             pchan.ctypes.data, peaks[prods[0]].ctypes.data, used, err, len(err)), err)
            ks, kp = [used[0]], [used[1]]
            cf, bf = cf.astype(bool), bf.astype(bool)
            extra = dict(pflag=pflag, pchan=pchan.astype(bool), peaks=peaks, t_pow=fpar.t_pow)
        else:
            stats, pflags, extra, ks, kp = _periodic_pass(lib, x, hdr, par, fpar, prods, device)
            mask, cf, bf = _clean_from_stats(lib, x, hdr, par, stats, prods, z, repl, device, priors=pflags)
            cf = cf | extra["pchan"]
        if info is not None:
            info["kernel_used"], info["peaks_kernel_used"] = min(ks), min(kp)
        return x.reshape(np.shape(rows)), dict(mask=mask, repl=repl, chan_flag=cf, blk_flag=bf, **extra)
    if len(prods) == 1:
        nblk = lib.frbch_rfi_nblk(x.shape[0], par.block_rows)
        if nblk <= 0:
            raise InputError("block_rows must be 1..2^20")
        mask, cf, bf = np.zeros((nblk, nchan), np.uint8), np.zeros(nchan, np.uint8), np.zeros(nblk, np.uint8)
        used = C.c_uint32(0)
        desc = fil_desc(hdr, prods[0])
        _check(lib.frbch_rfi_clean_host(C.byref(desc), x.ctypes.data, x.shape[0], C.byref(par), None if z is None else z.ctypes.data,
                                        device, mask.ctypes.data, repl[prods[0]].ctypes.data, cf.ctypes.data, bf.ctypes.data,
                                        C.byref(used), err, len(err)), err)
        kernels.append(used.value)
        cf, bf = cf.astype(bool), bf.astype(bool)
    else:
        stats = []
        for p in prods:
            i = {}
            stats.append(rfi_stats(x, hdr, par, product=p, device=device, lib=lib, info=i))
            kernels.append(i["kernel_used"])
        mask, cf, bf = _clean_from_stats(lib, x, hdr, par, stats, prods, z, repl, device)
    if info is not None:
        info["kernel_used"] = min(kernels)
    return x.reshape(np.shape(rows)), dict(mask=mask, repl=repl, chan_flag=cf, blk_flag=bf)


def rfifind_fil(filterbankfile, block_rows=1024, t_cell=5.0, t_chan=5.0, chan_frac=0.3, block_frac=0.3, flag_file=None,
                write_clean=False, device=0, lib=None, info: dict | None = None, resident=False, periodic=False, t_freq=4.0):
    """Flag a filterbank: ``<base>_rfi.npz`` (mask, chan_flag, blk_flag, repl, the block statistics [nifs][nblk][nchan][2] and
    the parameters), ``<base>.flag`` (the wholly flagged channels, ``write_flag_file``) and, with ``write_clean``,
    ``<base>_clean.fil`` -- the header bytes unchanged, every product cleaned in the same cells.  ``flag_file``: channels
    to flag whatever the statistics say.  ``resident``: all products in one library call on rows uploaded once and downloaded
    once (frbch_rfi_cleanp_host) -- the same files and values.  ``periodic``: the periodicity test as well (``clean``), at
    ``t_freq`` Gaussian sigma over the bins of a cell; the ``.npz`` then gains ``peaks``, ``pflag``, ``pchan`` and ``t_pow``, and the
    channels it flags wholly are in the ``.flag`` file.  Returns (list of files written, the result dict of ``clean``)."""
    lib = lib or _lib.load()
    if periodic and resident:
        raise InputError("the periodic test is not built for resident rows: run rfifind with --periodic and without --resident "
                         "(the resident path is unchanged without --periodic)")
    fil = sigproc.read_fil(filterbankfile)
    hdr = fil.header
    rows = _rows_of(fil)
    params = dict(block_rows=int(block_rows), t_cell=float(t_cell), t_chan=float(t_chan), chan_frac=float(chan_frac),
                  block_frac=float(block_frac))
    zap = read_flag_file(flag_file, hdr["nchans"]) if flag_file else None
    par = rfi_params(params)
    nifs, nchan = hdr.get("nifs", 1), hdr["nchans"]
    extra = {}
    if periodic:
        fpar = rfi_fparams(periodic if isinstance(periodic, dict) else dict(t_freq=float(t_freq)), par)
        cleaned = _rows3(rows, hdr).copy()
        stats, pflags, extra, ks, kp = _periodic_pass(lib, cleaned, hdr, par, fpar, list(range(nifs)), device)
        repl = np.zeros((nifs, nchan), np.float64)
        mask, cf, bf = _clean_from_stats(lib, cleaned, hdr, par, stats, list(range(nifs)), _zap_array(zap, nchan), repl, device,
                                         priors=pflags)
        res = dict(mask=mask, repl=repl, chan_flag=cf | extra["pchan"], blk_flag=bf, **extra)
        stats = np.stack(stats)
        if info is not None:
            info["kernel_used"], info["peaks_kernel_used"] = min(ks), min(kp)
    elif resident:
        cleaned, res = cleanp(rows, hdr, par, zap=zap, device=device, lib=lib, info=info, want_stats=True)
        cleaned, stats = _rows3(cleaned, hdr), res.pop("stats")
    else:
        cleaned = _rows3(rows, hdr).copy()
        stats, kernels = [], []
        for p in range(nifs):                                    # taken once: they go into the .npz and into the decision
            i = {}
            stats.append(rfi_stats(cleaned, hdr, par, product=p, device=device, lib=lib, info=i))
            kernels.append(i["kernel_used"])
        repl = np.zeros((nifs, nchan), np.float64)
        mask, cf, bf = _clean_from_stats(lib, cleaned, hdr, par, stats, list(range(nifs)), _zap_array(zap, nchan), repl, device)
        res = dict(mask=mask, repl=repl, chan_flag=cf, blk_flag=bf)
        stats = np.stack(stats)
        if info is not None:
            info["kernel_used"] = min(kernels)
    base = filterbankfile.replace(".fil", "")
    np.savez(base + "_rfi.npz", mask=res["mask"], chan_flag=res["chan_flag"], blk_flag=res["blk_flag"], repl=res["repl"], stats=stats,
             zap=np.zeros(hdr["nchans"], bool) if zap is None else zap, nrows=rows.shape[0], **params, **extra)
    write_flag_file(base + ".flag", res["chan_flag"])
    out = [base + "_rfi.npz", base + ".flag"]
    if write_clean:
        with open(filterbankfile, "rb") as f:
            head = f.read(fil.header_bytes)
        with open(base + "_clean.fil", "wb") as f:
            f.write(head)
            f.write(np.ascontiguousarray(cleaned).tobytes())
        out.append(base + "_clean.fil")
    return out, res


def _periodic_args(periodic, rfi, resident):
    """``periodic`` of search_fil / candidates_fil: goes with ``rfi``, and not with ``resident``"""
    if not periodic:
        return
    if resident:
        raise InputError("the periodic test is not built for resident rows: use --periodic without --resident "
                         "(the resident path is unchanged without --periodic)")
    if not rfi:
        raise InputError("the periodic test is part of the flagging: give --rfi (rfi=True) with --periodic")


def _read_rows(filterbankfile, flag_file, rfi, device, lib, info, detrend_len=1000, periodic=None):
    """the file; with ``flag_file`` or ``rfi`` its product-0 rows cleaned once (frbch_rfi_clean_host; with ``periodic``
    frbch_rfi_cleanf_host) in a copy"""
    fil = sigproc.read_fil(filterbankfile)
    if flag_file is None and not rfi:
        return fil
    hdr = fil.header
    zap = read_flag_file(flag_file, hdr["nchans"]) if flag_file is not None else None
    rinfo = {}
    cleaned, res = clean(_rows_of(fil), hdr, rfi if isinstance(rfi, dict) else None, zap=zap, device=device, lib=lib, info=rinfo,
                         products=[0], **(dict(periodic=periodic) if periodic else {}))
    if info is not None:
        info.update(rfi_kernel_used=rinfo["kernel_used"], rfi_chan_flag=res["chan_flag"], rfi_blk_flag=res["blk_flag"],
                    rfi_mask=res["mask"], rfi_masked_cells=int(res["mask"].sum()))
        if periodic:
            info.update(rfi_pflag=res["pflag"], rfi_pchan=res["pchan"], rfi_peaks_kernel_used=rinfo["peaks_kernel_used"])
    block_rows = rfi_params(rfi if isinstance(rfi, dict) else None).block_rows
    if res["blk_flag"].any() and not res["chan_flag"].all() and 2 * block_rows > (detrend_len or 1000):
        import warnings
        warnings.warn("%d block(s) of %d rows flagged wholly: each is a flat stretch of every dedispersed series, longer than half a "
                      "normalisation block of the search (detrend_len = %d), which can then report the noise at the stretch's edges; "
                      "use shorter blocks, e.g. rfi=dict(block_rows=256)" % (int(res["blk_flag"].sum()), block_rows, detrend_len or 1000))
    return sigproc.SigprocFile(header=hdr, header_bytes=fil.header_bytes, data=cleaned)


# ------------------------------------------------------------------------------------------------------------------
# single-pulse search
# ------------------------------------------------------------------------------------------------------------------
SP_WIDTHS = [1, 2, 3, 4, 6, 9, 14, 20, 30, 45, 70, 100, 150, 220, 300]
SP_CAND = np.dtype([("dm_index", "<u4"), ("width", "<u4"), ("sample", "<u8"), ("sigma", "<f4"), ("reserved", "<u4")])
SP_HEADER = "# DM      Sigma      Time (s)     Sample    Downfact"
SP_ROW = "%7.2f %7.2f %13.6f %10d   %3d"


def default_widths(tsamp: float, max_width_s: float = 0.0) -> list:
    """Boxcar widths in samples: the downsampling factors of PRESTO's single_pulse_search.py, 1 2 3 4 6 9 14 20 30 45 70
    100 150 220 300, AS REMEMBERED [EXT-UNVERIFIED: PRESTO is not at hand to check the list against].  Without a maximum
    width the list is cut at 30 (PRESTO's default); with one it keeps the widths with w * tsamp <= max_width_s."""
    if max_width_s > 0.0:
        return [w for w in SP_WIDTHS if w * tsamp <= max_width_s] or [1]
    return [w for w in SP_WIDTHS if w <= 30]


def sp_params(widths, threshold: float = 5.0, detrend_len: int = 1000) -> _lib.FrbchSpParams:
    widths = [int(w) for w in widths]
    if not 1 <= len(widths) <= 16:
        raise InputError("the search takes 1..16 boxcar widths")
    if min(widths) < 0 or max(widths) >= 1 << 32 or not 0 <= int(detrend_len) < 1 << 32:
        raise InputError("widths and detrend_len must be non-negative 32-bit integers")
    p = _lib.FrbchSpParams()
    p.size = C.sizeof(_lib.FrbchSpParams)
    p.nwidth = len(widths)
    for k, w in enumerate(widths):
        p.widths[k] = w
    p.detrend_len = int(detrend_len)
    p.threshold = float(threshold)
    return p


def _sp_call(call, cap: int):
    """run call(cands pointer, cap, ncand, used, err) with room for `cap` candidates; once more with the reported total"""
    while True:
        cands = np.zeros(cap, dtype=SP_CAND)
        ncand, used = C.c_uint64(0), C.c_uint32(0)
        err = C.create_string_buffer(512)
        rc = call(cands.ctypes.data, cap, C.byref(ncand), C.byref(used), err, len(err))
        if rc == _lib.E_CAPACITY and ncand.value > cap:
            cap = ncand.value
            continue
        _check(rc, err)
        return cands[: ncand.value].copy(), used.value


def single_pulse_search(series, widths=None, threshold: float = 5.0, detrend_len: int = 1000, tsamp: float = 0.0,
                        max_width_s: float = 0.0, device: int = 0, lib=None, info: dict | None = None, cap: int = 4096):
    """Boxcar search of dedispersed series ([ndm][nout] or [nout] float32) on the GPU (frbch_spsearch_host; the arithmetic
    is stated in include/frbch.h) -> structured array (dm_index, width, sample = centre of the boxcar, sigma, reserved),
    sorted by (dm_index, sample, width).  ``widths`` defaults to ``default_widths(tsamp, max_width_s)``;
    ``info['kernel_used']`` receives 1 when the LDS kernel ran, 0 for the generic one."""
    lib = lib or _lib.load()
    y = np.ascontiguousarray(series, dtype=np.float32)
    y = y.reshape(1, -1) if y.ndim == 1 else y
    if y.ndim != 2 or y.size == 0:
        raise InputError("series must be [ndm][nout] with at least one sample")
    params = sp_params(widths if widths is not None else default_widths(tsamp, max_width_s), threshold, detrend_len)
    out, used = _sp_call(lambda c, n, nc, u, e, ne: lib.frbch_spsearch_host(y.ctypes.data, y.shape[0], y.shape[1], C.byref(params),
                                                                            device, c, n, nc, u, e, ne), cap)
    if info is not None:
        info["kernel_used"] = used
    return out


def write_singlepulse(path: str, cands, dm: float, tsamp: float) -> None:
    """PRESTO's .singlepulse text: DM, sigma, time of the boxcar's centre, its sample, the boxcar width (`Downfact`)"""
    with open(path, "w") as f:
        f.write(SP_HEADER + "\n")
        for c in cands:
            f.write(SP_ROW % (dm, c["sigma"], int(c["sample"]) * tsamp, int(c["sample"]), int(c["width"])) + "\n")


def read_singlepulse(path: str, dm_index: int = 0) -> np.ndarray:
    """a .singlepulse file back as candidate records (sigma as printed: two decimals)"""
    rows = []
    with open(path) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            _dm, sigma, _time, sample, width = line.split()
            rows.append((dm_index, int(width), int(sample), float(sigma), 0))
    return np.array(rows, dtype=SP_CAND) if rows else np.zeros(0, dtype=SP_CAND)


def _series_names(filterbankfile, dm1, dm2, dms):
    if dm2 > 0.0:
        base = filterbankfile.replace(".fil", "")
        return ["%s_DM%.2f" % (base, dm) for dm in dms]           # prepsubband's naming
    return [filterbankfile.replace(".fil", "_dm{0}".format(dm1))]    # process_vdif.py:216


def search_fil(filterbankfile, dm1, dm2=0, dmstep=1.0, zerodm=True, clip=5, threshold=5.0, max_width_s=0.0, detrend_len=1000,
               write_dat=False, widths=None, device=0, lib=None, info: dict | None = None, flag_file=None, rfi=None, resident=False,
               periodic=None):
    """Dedisperse a filterbank over the DMs of ``prepdata_gpu`` and search every series for single pulses in one library
    call (frbch_dedisperse_search_host: the DM x time plane never leaves the GPU unless ``write_dat`` asks for the .dat /
    .inf files, which are then ``prepdata_gpu``'s).  Writes one ``<name>.singlepulse`` per DM, names as ``prepdata_gpu``.
    ``flag_file`` (channels to flag, ``read_flag_file``) and / or ``rfi`` (``True`` or a dict of ``RFI_DEFAULTS`` keys): the
    rows are flagged and cleaned once (``clean``, frbch_rfi_clean_host) and the cleaned rows searched; with neither, every
    file is what it was without them.  ``resident``: flagging and search in one library call on rows uploaded once
    (frbch_candidates_host) -- the same files and values; ``info`` gains ``row_uploads`` and the stage times.
    ``periodic`` (with ``rfi``; ``True`` or the dict ``clean`` takes): the periodicity test is part of the flagging.
    Returns (list of .singlepulse files, candidates of all DMs as a structured array)."""
    lib = lib or _lib.load()
    _periodic_args(periodic, rfi, resident)
    if resident:
        return _search_fil_resident(filterbankfile, dm1, dm2, dmstep, zerodm, clip, threshold, max_width_s, detrend_len, write_dat, widths,
                                    device, lib, info, flag_file, rfi)
    fil = _read_rows(filterbankfile, flag_file, rfi, device, lib, info, detrend_len, periodic)
    return _search(fil, filterbankfile, dm1, dm2, dmstep, zerodm, clip, threshold, max_width_s, detrend_len, write_dat, widths, device,
                   lib, info)


def _search(fil, filterbankfile, dm1, dm2, dmstep, zerodm, clip, threshold, max_width_s, detrend_len, write_dat, widths, device, lib,
            info):
    """``search_fil`` on a file already read (and cleaned, where asked for)"""
    hdr = fil.header
    dms = dm_list(dm1, dm2, dmstep)
    rows = _rows_of(fil)
    desc = fil_desc(hdr)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    nout = lib.frbch_dedisperse_nout(C.byref(desc), rows.shape[0], dm_arr.ctypes.data, dm_arr.size)
    if nout <= 0:
        raise InputError("the dispersion delay across the band exceeds the length of the filterbank")
    params = sp_params(widths if widths is not None else default_widths(hdr["tsamp"], max_width_s), threshold, detrend_len)
    series = np.empty((dm_arr.size, nout), dtype=np.float32) if write_dat else None
    nclip = C.c_uint64(0)
    cands, used = _sp_call(lambda c, n, nc, u, e, ne: lib.frbch_dedisperse_search_host(
        C.byref(desc), rows.ctypes.data, rows.shape[0], dm_arr.ctypes.data, dm_arr.size, 1 if zerodm else 0, float(clip),
        C.byref(params), device, series.ctypes.data if write_dat else None, nout, C.byref(nclip), c, n, nc, u, e, ne), 4096)
    if info is not None:
        info.update(kernel_used=used, nclipped=nclip.value, nout=nout)
    names = _series_names(filterbankfile, dm1, dm2, dms)
    out = []
    for i, (name, dm) in enumerate(zip(names, dms)):
        write_singlepulse(name + ".singlepulse", cands[cands["dm_index"] == i], dm, hdr["tsamp"])
        out.append(name + ".singlepulse")
        if write_dat:
            series[i].astype("<f4").tofile(name + ".dat")
            write_inf(name + ".inf", basename=os.path.basename(name), hdr=hdr, nsamp=nout, dm=dm, clipped=nclip.value)
    return out, cands


# ------------------------------------------------------------------------------------------------------------------
# band-limited single-pulse search
# ------------------------------------------------------------------------------------------------------------------
SPB_CAND = np.dtype([("dm_index", "<u4"), ("width", "<u4"), ("sample", "<u8"), ("sigma", "<f4"), ("sub_lo", "<u2"), ("sub_hi", "<u2")])
SPB_GROUP = np.dtype([("best", SPB_CAND), ("nmember", "<u4"), ("dm_index_lo", "<u4"), ("dm_index_hi", "<u4"), ("sub_lo_min", "<u2"),
                      ("sub_hi_max", "<u2"), ("sample_lo", "<u8"), ("sample_hi", "<u8"), ("full_sigma", "<f4"), ("reserved", "<u4")])
BANDS_HEADER = "# DM      Sigma      Time (s)     Sample    Downfact  Members   Flo (MHz)   Fhi (MHz)  Sub  FullSigma"
BANDS_ROW = "%7.2f %7.2f %13.6f %10d   %3d %8d %11.4f %11.4f  %d-%d %9.2f"


def band_params(nsub: int = 8, min_sub: int = 1, max_sub: int = 0) -> _lib.FrbchBandParams:
    if not all(0 <= int(v) < 1 << 32 for v in (nsub, min_sub, max_sub)):
        raise InputError("nsub, min_sub and max_sub must be non-negative 32-bit integers")
    p = _lib.FrbchBandParams()
    p.size = C.sizeof(_lib.FrbchBandParams)
    p.nsub, p.min_sub, p.max_sub = int(nsub), int(min_sub), int(max_sub)
    return p


def band_list(nchan: int, nsub: int = 8, min_sub: int = 1, max_sub: int = 0, lib=None) -> np.ndarray:
    """The bands of frbch_band_list: every range [a, b) of the ``nsub`` equal sub-bands of ``nchan`` channels with
    ``min_sub <= b - a <= max_sub`` (0 = ``nsub``), by ascending a, then b -> uint16 [nband][2]."""
    lib = lib or _lib.load()
    bp = band_params(nsub, min_sub, max_sub)
    lo, hi = np.zeros(136, dtype=np.uint16), np.zeros(136, dtype=np.uint16)
    n = C.c_uint32(0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_band_list(int(nchan), C.byref(bp), lo.ctypes.data, hi.ctypes.data, lo.size, C.byref(n), err, len(err)), err)
    return np.stack([lo[: n.value], hi[: n.value]], axis=1)


def band_edges_mhz(hdr: dict, nsub: int, sub_lo: int, sub_hi: int):
    """(lowest, highest) frequency in MHz of the channels of band [sub_lo, sub_hi), channel edges included"""
    cps = hdr["nchans"] // nsub
    f = [hdr["fch1"] + (c - 0.5) * hdr["foff"] for c in (sub_lo * cps, sub_hi * cps)]
    return min(f), max(f)


def _bands_nout(lib, desc, rows, dm_arr):
    nout = lib.frbch_dedisperse_nout(C.byref(desc), rows.shape[0], dm_arr.ctypes.data, dm_arr.size)
    if nout <= 0:
        raise InputError("the dispersion delay across the band exceeds the length of the filterbank" if nout == 0 else
                         "bad header, or a DM outside [0, 1e5)")
    return nout


def dedisperse_bands(rows, hdr: dict, dms, nsub: int = 8, min_sub: int = 1, max_sub: int = 0, zerodm: bool = True, clip: float = 5.0,
                     product: int = 0, device: int = 0, lib=None, info: dict | None = None):
    """The series of every band of ``band_list`` on the GPU (frbch_dedisperse_bands_host; include/frbch.h states the
    arithmetic) -> (float32 [ndm][nband][nout], number of clipped time samples).  Band [0, nsub) is ``dedisperse``'s series
    to the bit.  ``info['kernel_used']``: 1 = the tiled prefix kernel, 0 = the generic one."""
    lib = lib or _lib.load()
    x = _rows3(rows, hdr)
    desc = fil_desc(dict(hdr, nifs=x.shape[1], nbits=x.dtype.itemsize * 8), product)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    bp = band_params(nsub, min_sub, max_sub)
    nband = band_list(desc.nchan, nsub, min_sub, max_sub, lib).shape[0]
    nout = _bands_nout(lib, desc, x, dm_arr)
    out = np.empty((dm_arr.size, nband, nout), dtype=np.float32)
    nclip, used = C.c_uint64(0), C.c_uint32(0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_dedisperse_bands_host(C.byref(desc), x.ctypes.data, x.shape[0], dm_arr.ctypes.data, dm_arr.size, 1 if zerodm else 0,
                                           float(clip), C.byref(bp), device, out.ctypes.data, nout, C.byref(nclip), C.byref(used), err,
                                           len(err)), err)
    if info is not None:
        info.update(kernel_used=used.value, nout=nout, nband=nband)
    return out, nclip.value


def band_search(rows, hdr: dict, dms, nsub: int = 8, min_sub: int = 1, max_sub: int = 0, zerodm: bool = True, clip: float = 5.0,
                widths=None, threshold: float = 5.0, detrend_len: int = 1000, max_width_s: float = 0.0, plane_bytes: int = 0,
                product: int = 0, device: int = 0, lib=None, info: dict | None = None, cap: int = 4096) -> np.ndarray:
    """Single-pulse search of every band's series over the DMs (frbch_bandsearch_host: one upload of the rows, one clip /
    zero-DM pre-pass, batches of DMs whose plane fits ``plane_bytes`` -- 0 = 1 GiB -- searched where they lie in HBM) ->
    SPB_CAND records sorted by (dm_index, sub_lo, sub_hi, sample, width); the list does not depend on ``plane_bytes``.
    ``info`` receives kernel_used (dedispersion, search), nbatch, nclipped, nout and the stage times in ms."""
    lib = lib or _lib.load()
    x = _rows3(rows, hdr)
    desc = fil_desc(dict(hdr, nifs=x.shape[1], nbits=x.dtype.itemsize * 8), product)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    bp = band_params(nsub, min_sub, max_sub)
    params = sp_params(widths if widths is not None else default_widths(hdr["tsamp"], max_width_s), threshold, detrend_len)
    nout = _bands_nout(lib, desc, x, dm_arr)
    while True:
        cands = np.zeros(cap, dtype=SPB_CAND)
        ncand, nclip, nbatch = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        used, ms = (C.c_uint32 * 2)(), (C.c_double * 3)()
        err = C.create_string_buffer(512)
        rc = lib.frbch_bandsearch_host(C.byref(desc), x.ctypes.data, x.shape[0], dm_arr.ctypes.data, dm_arr.size, 1 if zerodm else 0,
                                       float(clip), C.byref(bp), C.byref(params), int(plane_bytes), device, nout, C.byref(nclip),
                                       cands.ctypes.data, cap, C.byref(ncand), used, C.byref(nbatch), ms, err, len(err))
        if rc == _lib.E_CAPACITY and ncand.value > cap:
            cap = ncand.value
            continue
        _check(rc, err)
        break
    if info is not None:
        info.update(kernel_used=(used[0], used[1]), nbatch=nbatch.value, nclipped=nclip.value, nout=nout,
                    stage_ms=dict(prepass=ms[0], dedisperse=ms[1], search=ms[2]))
    return cands[: ncand.value].copy()


def group_band_candidates(cands, hdr: dict, dms, nsub: int = 8, dm_gap: int = 2, lib=None) -> np.ndarray:
    """Join the records of one pulse across trial DMs AND bands (frbch_spb_group_cands, host only: the link rule of
    ``group_candidates`` on (dm_index, sample, width); the band plays no part in it) -> SPB_GROUP sorted by the best member's
    (dm_index, sample, width, sub_lo, sub_hi); ``full_sigma`` is the strongest full-band member's sigma, 0 without one."""
    lib = lib or _lib.load()
    recs = np.ascontiguousarray(cands, dtype=SPB_CAND)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    desc = fil_desc(hdr)
    out = np.zeros(max(1, recs.size), dtype=SPB_GROUP)
    n = C.c_uint64(0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_spb_group_cands(C.byref(desc), dm_arr.ctypes.data, dm_arr.size, int(nsub), recs.ctypes.data, recs.size,
                                     int(dm_gap), out.ctypes.data, out.size, C.byref(n), err, len(err)), err)
    return out[: n.value].copy()


def bandsearch_fil(filterbankfile, dm1, dm2=0, dmstep=1.0, nsub=8, min_sub=1, max_sub=0, zerodm=True, clip=5, threshold=5.0,
                   max_width_s=0.0, detrend_len=1000, widths=None, dm_gap=2, plane_bytes=0, device=0, lib=None,
                   info: dict | None = None, flag_file=None, rfi=None, periodic=None):
    """Band-limited search of a filterbank over the DMs of ``prepdata_gpu``: ``band_search`` on the rows -- cleaned first where
    ``flag_file`` / ``rfi`` / ``periodic`` ask for it, exactly as ``search_fil`` does -- then ``group_band_candidates``.
    Writes ``<base>_bands.npz`` (cands, groups, bands, dms, nsub) and ``<base>_bands.txt``: one line per group, strongest
    first, with the band's frequency edges and the full-band sigma next to the band's; DM, sample and width are what
    ``--dm --sample --width`` of the burst commands take.  Returns (npz, txt, records, groups)."""
    lib = lib or _lib.load()
    _periodic_args(periodic, rfi, False)
    fil = _read_rows(filterbankfile, flag_file, rfi, device, lib, info, detrend_len, periodic)
    hdr = fil.header
    dms = dm_list(dm1, dm2, dmstep)
    cands = band_search(_rows_of(fil), hdr, dms, nsub, min_sub, max_sub, zerodm, clip, widths, threshold, detrend_len, max_width_s,
                        plane_bytes, 0, device, lib, info)
    groups = group_band_candidates(cands, hdr, dms, nsub, dm_gap, lib)
    bands = band_list(hdr["nchans"], nsub, min_sub, max_sub, lib)
    base = filterbankfile.replace(".fil", "")
    np.savez(base + "_bands.npz", cands=cands, groups=groups, bands=bands, dms=np.asarray(dms, dtype=np.float64), nsub=np.int64(nsub))
    with open(base + "_bands.txt", "w") as f:
        f.write(BANDS_HEADER + "\n")
        for g in groups[np.argsort(-groups["best"]["sigma"], kind="stable")]:
            b = g["best"]
            flo, fhi = band_edges_mhz(hdr, nsub, int(b["sub_lo"]), int(b["sub_hi"]))
            f.write(BANDS_ROW % (dms[b["dm_index"]], b["sigma"], int(b["sample"]) * hdr["tsamp"], int(b["sample"]), int(b["width"]),
                                 int(g["nmember"]), flo, fhi, int(b["sub_lo"]), int(b["sub_hi"]), g["full_sigma"]) + "\n")
    return base + "_bands.npz", base + "_bands.txt", cands, groups


# ------------------------------------------------------------------------------------------------------------------
# periodicity search
# ------------------------------------------------------------------------------------------------------------------
PS_CAND = np.dtype([("dm_index", "<u4"), ("h", "<u4"), ("k", "<u4"), ("power", "<f4"), ("sigma", "<f8"), ("freq_hz", "<f8")])
PS_GROUP = np.dtype([("best", PS_CAND), ("nmember", "<u4"), ("dm_index_lo", "<u4"), ("dm_index_hi", "<u4"), ("reserved", "<u4")])
PS_HEADER = "# Period (s)      Freq (Hz)        DM    Sigma  Fold  Members  DMlo  DMhi"
PS_ROW = "%14.9f %14.7f %9.2f %8.2f %5d %8d %5d %5d"


def ps_params(tsamp: float, sigma: float = 6.0, nharm: int = 16, flo: float = 0.5, nfft: int = 0,
              wblock: int = 128) -> _lib.FrbchPsParams:
    for name, v in (("nharm", nharm), ("nfft", nfft), ("wblock", wblock)):
        if not 0 <= int(v) < 1 << 32:
            raise InputError("%s must be a non-negative 32-bit integer" % name)
    p = _lib.FrbchPsParams()
    p.size = C.sizeof(_lib.FrbchPsParams)
    p.nfft, p.nharm, p.wblock = int(nfft), int(nharm), int(wblock)
    p.sigma, p.flo_hz, p.tsamp_s = float(sigma), float(flo), float(tsamp)
    return p


def _ps_call(call, cap: int):
    """run call(cands pointer, cap, ncand, used, err) with room for `cap` records; once more with the reported total"""
    while True:
        cands = np.zeros(cap, dtype=PS_CAND)
        ncand, used = C.c_uint64(0), (C.c_uint32 * 2)(0, 0)
        err = C.create_string_buffer(512)
        rc = call(cands.ctypes.data, cap, C.byref(ncand), used, err, len(err))
        if rc == _lib.E_CAPACITY and ncand.value > cap:
            cap = ncand.value
            continue
        _check(rc, err)
        return cands[: ncand.value].copy(), (used[0], used[1])


def periodicity_search(series, tsamp: float, sigma: float = 6.0, nharm: int = 16, flo: float = 0.5, nfft: int = 0,
                       wblock: int = 128, device: int = 0, lib=None, info: dict | None = None, cap: int = 4096):
    """Periodicity search of dedispersed series ([ndm][nout] or [nout] float32) on the GPU (frbch_psearch_host; the
    arithmetic is stated in include/frbch.h): one transform of ``nfft`` points (0: the largest power of two not above nout)
    per series, red-noise normalisation in blocks of ``wblock`` bins, harmonic sums of up to ``nharm`` harmonics, peaks above
    ``sigma`` -> structured array PS_CAND (dm_index, h = harmonics summed, k = bin of the highest of them, power, sigma,
    freq_hz of the fundamental), sorted by (dm_index, h, k).  ``info['kernel_used']`` receives 1 for the fast form, 0 for the
    generic one, ``info['passes']`` the LDS passes of the fast transform."""
    lib = lib or _lib.load()
    y = np.ascontiguousarray(series, dtype=np.float32)
    y = y.reshape(1, -1) if y.ndim == 1 else y
    if y.ndim != 2 or y.size == 0:
        raise InputError("series must be [ndm][nout] with at least one sample")
    params = ps_params(tsamp, sigma, nharm, flo, nfft, wblock)
    out, used = _ps_call(lambda c, n, nc, u, e, ne: lib.frbch_psearch_host(y.ctypes.data, y.shape[0], y.shape[1], C.byref(params),
                                                                           device, c, n, nc, u, e, ne), cap)
    if info is not None:
        info.update(kernel_used=used[0], passes=used[1])
    return out


def group_periodic(cands, dm_gap: int = 2, lib=None) -> np.ndarray:
    """Join the records of one signal across trial DMs (frbch_ps_group_cands, host only; include/frbch.h states the rule) ->
    structured array PS_GROUP, the strongest first.  Harmonically related groups are NOT merged."""
    lib = lib or _lib.load()
    recs = np.ascontiguousarray(cands, dtype=PS_CAND)
    out = np.zeros(max(1, recs.size), dtype=PS_GROUP)
    n = C.c_uint64(0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_ps_group_cands(recs.ctypes.data, recs.size, int(dm_gap), out.ctypes.data, out.size, C.byref(n), err, len(err)), err)
    return out[: n.value].copy()


# ---- trial accelerations ---------------------------------------------------------------------------------------------
C_LIGHT = 299792458.0
PA_CAND = np.dtype([("dm_index", "<u4"), ("acc_index", "<u4"), ("h", "<u4"), ("k", "<u4"), ("power", "<f4"), ("reserved", "<u4"),
                    ("sigma", "<f8"), ("freq_hz", "<f8"), ("acc_ms2", "<f8")])
PA_GROUP = np.dtype([("best", PA_CAND), ("nmember", "<u4"), ("dm_index_lo", "<u4"), ("dm_index_hi", "<u4"), ("acc_index_lo", "<u4"),
                     ("acc_index_hi", "<u4"), ("reserved", "<u4")])
PA_HEADER = "# Period (s)      Freq (Hz)        DM    Sigma  Fold  Members  DMlo  DMhi    Acc (m/s^2)  Alo  Ahi"
PA_ROW = "%14.9f %14.7f %9.2f %8.2f %5d %8d %5d %5d %14.6g %4d %4d"


def acc_list(amax: float, astep: float) -> np.ndarray:
    """Trial accelerations -amax .. 0 .. +amax in steps of ``astep`` (m/s^2), 0 always a member: k astep for
    |k| <= floor(amax / astep); ``amax`` = 0 gives [0]."""
    amax, astep = float(amax), float(astep)
    if not (amax >= 0.0 and np.isfinite(amax)):
        raise InputError("amax must be finite and not negative")
    if amax == 0.0:
        return np.zeros(1, dtype=np.float64)
    if not (astep > 0.0 and np.isfinite(astep)):
        raise InputError("astep must be positive when amax is")
    m = int(np.floor(amax / astep * (1.0 + 1e-12)))
    if 2 * m + 1 > 1024:
        raise InputError("%d trial accelerations: the library takes 1024 at the most (raise astep)" % (2 * m + 1))
    return np.arange(-m, m + 1, dtype=np.float64) * astep


def accel_step(n: int, tsamp: float, f_hz: float, bins: float = 1.0) -> float:
    """The acceleration (m/s^2) that moves a signal of ``f_hz`` by ``bins`` Fourier bins over a scan of ``n`` samples:
    bins c / (f_hz (n tsamp)^2)."""
    return float(bins) * C_LIGHT / (float(f_hz) * (float(n) * float(tsamp)) ** 2)


def _pa_call(call, cap: int):
    """_ps_call for frbch_pa_cand records and kernel_used[3]"""
    while True:
        cands = np.zeros(cap, dtype=PA_CAND)
        ncand, used = C.c_uint64(0), (C.c_uint32 * 3)(0, 0, 0)
        err = C.create_string_buffer(512)
        rc = call(cands.ctypes.data, cap, C.byref(ncand), used, err, len(err))
        if rc == _lib.E_CAPACITY and ncand.value > cap:
            cap = ncand.value
            continue
        _check(rc, err)
        return cands[: ncand.value].copy(), (used[0], used[1], used[2])


def _accs_of(accs) -> np.ndarray:
    a = np.ascontiguousarray(accs, dtype=np.float64).reshape(-1)
    if not 1 <= a.size <= 1024:
        raise InputError("1 .. 1024 trial accelerations")
    return a


def resample(series, tsamp: float, accs, nfft: int = 0, device: int = 0, lib=None, info: dict | None = None) -> np.ndarray:
    """The resampler of the acceleration search alone (frbch_resample_host; include/frbch.h states the index rule) ->
    [nacc][ndm][n] float32, n = ``nfft`` or the largest power of two not above nout."""
    lib = lib or _lib.load()
    y = np.ascontiguousarray(series, dtype=np.float32)
    y = y.reshape(1, -1) if y.ndim == 1 else y
    if y.ndim != 2 or y.size == 0:
        raise InputError("series must be [ndm][nout] with at least one sample")
    a = _accs_of(accs)
    params = ps_params(tsamp, nfft=nfft)
    n = lib.frbch_psearch_nfft(y.shape[1], C.byref(params))
    if n <= 0:
        raise InputError("the transform length must be a power of two in 2^12..2^22 and at most nout")
    out = np.zeros((a.size, y.shape[0], n), dtype=np.float32)
    used = (C.c_uint32 * 1)(0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_resample_host(y.ctypes.data, y.shape[0], y.shape[1], n, float(tsamp), a.ctypes.data, a.size, device,
                                   out.ctypes.data, used, err, len(err)), err)
    if info is not None:
        info.update(resampler=used[0])
    return out


def accel_search(series, tsamp: float, accs, sigma: float = 6.0, nharm: int = 16, flo: float = 0.5, nfft: int = 0,
                 wblock: int = 128, batch_rows: int = 0, device: int = 0, lib=None, info: dict | None = None, cap: int = 4096):
    """``periodicity_search`` for every trial acceleration of ``accs`` (m/s^2, strictly ascending) on the GPU
    (frbch_pasearch_host): every series is resampled per trial and searched as before -> structured array PA_CAND sorted by
    (acc_index, dm_index, h, k); freq_hz is the frequency at the middle of the scan.  ``info`` receives ``resampler``,
    ``kernel_used`` and ``passes``."""
    lib = lib or _lib.load()
    y = np.ascontiguousarray(series, dtype=np.float32)
    y = y.reshape(1, -1) if y.ndim == 1 else y
    if y.ndim != 2 or y.size == 0:
        raise InputError("series must be [ndm][nout] with at least one sample")
    a = _accs_of(accs)
    params = ps_params(tsamp, sigma, nharm, flo, nfft, wblock)
    out, used = _pa_call(lambda c, n, nc, u, e, ne: lib.frbch_pasearch_host(
        y.ctypes.data, y.shape[0], y.shape[1], C.byref(params), a.ctypes.data, a.size, int(batch_rows), device, c, n, nc, u, e, ne), cap)
    if info is not None:
        info.update(resampler=used[0], kernel_used=used[1], passes=used[2])
    return out


def group_accel(cands, dm_gap: int = 2, acc_gap: int = 1, lib=None) -> np.ndarray:
    """Join the records of one signal across trial DMs and trial accelerations (frbch_pa_group_cands, host only) ->
    structured array PA_GROUP, the strongest first."""
    lib = lib or _lib.load()
    recs = np.ascontiguousarray(cands, dtype=PA_CAND)
    out = np.zeros(max(1, recs.size), dtype=PA_GROUP)
    n = C.c_uint64(0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_pa_group_cands(recs.ctypes.data, recs.size, int(dm_gap), int(acc_gap), out.ctypes.data, out.size, C.byref(n),
                                    err, len(err)), err)
    return out[: n.value].copy()


def psearch_fil(filterbankfile, dm1, dm2=0, dmstep=1.0, zerodm=True, clip=5, sigma=6.0, nharm=16, flo=0.5, nfft=0, wblock=128,
                dm_gap=2, max_cands=0, fold_best=0, device=0, lib=None, info: dict | None = None, flag_file=None, rfi=None,
                periodic=None, amax=0.0, astep=0.0, acc_gap=1, refine=False):
    """Dedisperse a filterbank over the DMs of ``prepdata_gpu`` and search every series for periodic signals in one library
    call (frbch_dedisperse_psearch_host: the DM x time plane never leaves the GPU), then join the records across DMs.
    Writes ``<base>_psearch.txt`` (one line per candidate: period, frequency, DM, sigma, harmonics summed, members and DM span)
    and ``<base>_psearch.npz`` (the records, the candidates, the DMs).  ``flag_file`` / ``rfi`` / ``periodic`` as
    ``search_fil``.  ``max_cands`` > 0 keeps the strongest N candidates.  ``fold_best`` = K folds the K strongest candidates
    with the ephemeris {F0 = the candidate's frequency, F1 = 0, DM = its trial DM, PEPOCH = tstart} through ``fold_fil``'s
    machinery; their outputs are ``<base>_psearch_cand<i>.ar`` / ``.profile.txt`` / ``.png``.
    ``refine``: every folded candidate also goes through ``foldfit_fil`` (``<base>_psearch_cand<i>_foldfit.*``): a frequency known
    to half a Fourier bin lets the pulse drift by up to half a turn over the observation.
    ``amax`` > 0 adds trial accelerations ``acc_list(amax, astep)`` (m/s^2; ``astep`` = 0: two bins of drift at 100 Hz,
    ``accel_step(n, tsamp, 100.0, 2.0)``): one call of frbch_dedisperse_pasearch_host, records joined across DMs and trials
    (``acc_gap``), a text file with acceleration columns under PA_HEADER, ``accs`` in the ``.npz``, and folds with
    F1 = -F0 a / c at PEPOCH = the middle of the searched span.  With ``amax`` = 0 nothing differs from before.
    Returns (list of files written, candidates as PS_GROUP, or PA_GROUP with ``amax`` > 0)."""
    lib = lib or _lib.load()
    _periodic_args(periodic, rfi, False)
    fil = _read_rows(filterbankfile, flag_file, rfi, device, lib, info, periodic=periodic)
    hdr = fil.header
    dms = dm_list(dm1, dm2, dmstep)
    rows = _rows_of(fil)
    desc = fil_desc(hdr)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    nout = lib.frbch_dedisperse_nout(C.byref(desc), rows.shape[0], dm_arr.ctypes.data, dm_arr.size)
    if nout <= 0:
        raise InputError("the dispersion delay across the band exceeds the length of the filterbank")
    params = ps_params(hdr["tsamp"], sigma, nharm, flo, nfft, wblock)
    nclip = C.c_uint64(0)
    if amax > 0.0:
        return _pasearch_fil(fil, filterbankfile, rows, desc, dms, dm_arr, nout, params, zerodm, clip, dm_gap, max_cands, fold_best,
                             device, lib, info, amax, astep, acc_gap, refine)
    recs, used = _ps_call(lambda c, n, nc, u, e, ne: lib.frbch_dedisperse_psearch_host(
        C.byref(desc), rows.ctypes.data, rows.shape[0], dm_arr.ctypes.data, dm_arr.size, 1 if zerodm else 0, float(clip),
        C.byref(params), device, None, nout, C.byref(nclip), c, n, nc, u, e, ne), 4096)
    groups = group_periodic(recs, dm_gap, lib=lib)
    if max_cands > 0:
        groups = groups[:max_cands]
    n = lib.frbch_psearch_nfft(nout, C.byref(params))
    if info is not None:
        info.update(kernel_used=used[0], passes=used[1], nclipped=nclip.value, nout=nout, nfft=n, records=recs)
    base = filterbankfile.replace(".fil", "")
    with open(base + "_psearch.txt", "w") as f:
        f.write(PS_HEADER + "\n")
        for g in groups:
            b = g["best"]
            f.write(PS_ROW % (1.0 / b["freq_hz"], b["freq_hz"], dms[int(b["dm_index"])], b["sigma"], int(b["h"]), int(g["nmember"]),
                              int(g["dm_index_lo"]), int(g["dm_index_hi"])) + "\n")
    np.savez(base + "_psearch.npz", records=recs, candidates=groups, dms=dm_arr, nfft=n, tsamp=hdr["tsamp"])
    files = [base + "_psearch.txt", base + "_psearch.npz"]
    for i, g in enumerate(groups[: max(0, int(fold_best))]):
        b = g["best"]
        par = {"F0": float(b["freq_hz"]), "F1": 0.0, "DM": float(dms[int(b["dm_index"])]), "PEPOCH": float(hdr["tstart"]),
               "PSR": "cand%d" % i}
        ar, _profile = _fold_par(fil, filterbankfile, par, 0, 10.0, 128, device, lib, "%s_psearch_cand%d" % (base, i), None, 0.0,
                                 "coherency")
        files.append(ar)
        if refine:
            files += foldfit_fil(filterbankfile, fil=fil, par=par, device=device, lib=lib, out_base="%s_psearch_cand%d" % (base, i))[0]
    return files, groups


def _pasearch_fil(fil, filterbankfile, rows, desc, dms, dm_arr, nout, params, zerodm, clip, dm_gap, max_cands, fold_best, device, lib,
                  info, amax, astep, acc_gap, refine=False):
    """``psearch_fil`` with trial accelerations, from the point where the two part"""
    hdr = fil.header
    n = lib.frbch_psearch_nfft(nout, C.byref(params))
    if n <= 0:
        raise InputError("the transform length must be a power of two in 2^12..2^22 and at most the dedispersed length")
    accs = acc_list(amax, astep if astep > 0.0 else accel_step(n, hdr["tsamp"], 100.0, 2.0))
    nclip = C.c_uint64(0)
    recs, used = _pa_call(lambda c, m, nc, u, e, ne: lib.frbch_dedisperse_pasearch_host(
        C.byref(desc), rows.ctypes.data, rows.shape[0], dm_arr.ctypes.data, dm_arr.size, 1 if zerodm else 0, float(clip),
        C.byref(params), accs.ctypes.data, accs.size, 0, device, None, nout, C.byref(nclip), c, m, nc, u, e, ne), 4096)
    groups = group_accel(recs, dm_gap, acc_gap, lib=lib)
    if max_cands > 0:
        groups = groups[:max_cands]
    if info is not None:
        info.update(resampler=used[0], kernel_used=used[1], passes=used[2], nclipped=nclip.value, nout=nout, nfft=n, records=recs,
                    accs=accs)
    base = filterbankfile.replace(".fil", "")
    with open(base + "_psearch.txt", "w") as f:
        f.write(PA_HEADER + "\n")
        for g in groups:
            b = g["best"]
            f.write(PA_ROW % (1.0 / b["freq_hz"], b["freq_hz"], dms[int(b["dm_index"])], b["sigma"], int(b["h"]), int(g["nmember"]),
                              int(g["dm_index_lo"]), int(g["dm_index_hi"]), b["acc_ms2"], int(g["acc_index_lo"]),
                              int(g["acc_index_hi"])) + "\n")
    np.savez(base + "_psearch.npz", records=recs, candidates=groups, dms=dm_arr, nfft=n, tsamp=hdr["tsamp"], accs=accs)
    files = [base + "_psearch.txt", base + "_psearch.npz"]
    for i, g in enumerate(groups[: max(0, int(fold_best))]):
        b = g["best"]
        f0 = float(b["freq_hz"])
        par = {"F0": f0, "F1": -f0 * float(b["acc_ms2"]) / C_LIGHT, "DM": float(dms[int(b["dm_index"])]),
               "PEPOCH": float(hdr["tstart"]) + (n * hdr["tsamp"] / 2.0) / 86400.0, "PSR": "cand%d" % i}
        ar, _profile = _fold_par(fil, filterbankfile, par, 0, 10.0, 128, device, lib, "%s_psearch_cand%d" % (base, i), None, 0.0,
                                 "coherency")
        files.append(ar)
        if refine:
            files += foldfit_fil(filterbankfile, fil=fil, par=par, device=device, lib=lib, out_base="%s_psearch_cand%d" % (base, i))[0]
    return files, groups


# ------------------------------------------------------------------------------------------------------------------
# candidates: grouping across DMs and the two planes a classifier reads
# ------------------------------------------------------------------------------------------------------------------
SP_GROUP = np.dtype([("best", SP_CAND), ("nmember", "<u4"), ("dm_index_lo", "<u4"), ("dm_index_hi", "<u4"), ("reserved", "<u4"),
                     ("sample_lo", "<u8"), ("sample_hi", "<u8")])
CUT_CAND = np.dtype([("dm", "<f8"), ("dm_lo", "<f8"), ("dm_hi", "<f8"), ("sample", "<i8"), ("tfactor", "<u4"), ("reserved", "<u4")])
CANDS_HEADER = "# DM      Sigma      Time (s)     Sample    Downfact  Members  DMlo  DMhi"
CANDS_ROW = "%7.2f %7.2f %13.6f %10d   %3d %8d %5d %5d"


def group_candidates(cands, hdr: dict, dms, dm_gap: int = 2, lib=None) -> np.ndarray:
    """Join the records of one pulse across trial DMs (frbch_sp_group_cands, host only; include/frbch.h states the rule) ->
    structured array SP_GROUP sorted by the best member's (dm_index, sample, width)."""
    lib = lib or _lib.load()
    recs = np.ascontiguousarray(cands, dtype=SP_CAND)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    desc = fil_desc(hdr)
    out = np.zeros(max(1, recs.size), dtype=SP_GROUP)
    n = C.c_uint64(0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_sp_group_cands(C.byref(desc), dm_arr.ctypes.data, dm_arr.size, recs.ctypes.data, recs.size, int(dm_gap),
                                    out.ctypes.data, out.size, C.byref(n), err, len(err)), err)
    return out[: n.value].copy()


def cutout_cands(records, dms, dm_span=None) -> np.ndarray:
    """Search records (SP_CAND, e.g. ``groups['best']``) -> the candidates of ``cutouts`` with the defaults
    ``tfactor = max(1, width // 2)``, ``dm_lo = 0``, ``dm_hi = 2 * dm`` -- FETCH's / `your`'s candmaker as remembered
    [EXT-UNVERIFIED: neither is at hand].  ``dm_span``: the DM-time plane spans ``dm - dm_span / 2 .. dm + dm_span / 2``
    (cut at 0) instead.  ``dms = None``: the records carry their DM in a field ``dm``."""
    records = np.asarray(records)
    out = np.zeros(records.size, dtype=CUT_CAND)
    if dms is not None and "dm_index" in records.dtype.names:
        dm = np.asarray(dms, dtype=np.float64)[records["dm_index"].astype(np.int64)]
    elif "dm" in records.dtype.names:
        dm = records["dm"].astype(np.float64)
    else:
        raise InputError("records with dm_index need the DM list; without it they need a field dm")
    out["dm"] = dm
    if dm_span is None:
        out["dm_lo"], out["dm_hi"] = 0.0, 2.0 * dm
    else:
        out["dm_lo"] = np.maximum(0.0, dm - 0.5 * float(dm_span))
        out["dm_hi"] = out["dm_lo"] + float(dm_span)
    out["sample"] = records["sample"].astype(np.int64)
    out["tfactor"] = np.clip(records["width"].astype(np.int64) // 2, 1, 512)
    return out


CUT_TABLE_CAP = 1 << 26       # ncand * ndm * nchans a library call takes (include/frbch.h)


def cutouts(fil_or_rows, hdr: dict, cands, nt: int = 256, nf: int = 0, ndm: int = 256, dm_span=None, device: int = 0, lib=None,
            info: dict | None = None, batch: int = 0):
    """The frequency-time and DM-time planes of every candidate in one library call (frbch_cutout_host; include/frbch.h
    states the arithmetic: plain sums, no clip, no zero-DM filter) -> ``ft [n][nf][nt]``, ``ft_hits``, ``dt [n][ndm][nt]``,
    ``dt_hits``.  ``fil_or_rows``: a SigprocFile or its rows; ``cands``: CUT_CAND records (``cutout_cands`` makes them
    from search records and the DM list), or records with the fields ``dm``, ``sample`` and ``width``, which get the
    defaults of ``cutout_cands``.  ``nf = 0``: the largest divisor of nchans that is at most 256.  ``info['kernel_used']``: 1 = the
    LDS kernel, 0 = the generic one (in any call).  A list longer than one call takes (65535 candidates, 2^31 plane elements,
    2^26 delays) or than ``batch`` (0: no limit of its own) goes in several calls of whole candidates, each of which uploads
    the rows again; ``info['calls']`` counts them."""
    lib = lib or _lib.load()
    rows = _rows_of(fil_or_rows) if isinstance(fil_or_rows, sigproc.SigprocFile) else np.ascontiguousarray(fil_or_rows)
    if rows.dtype.itemsize * 8 != hdr["nbits"] or rows.size % (hdr["nchans"] * hdr.get("nifs", 1)):
        raise InputError("the rows do not match the header's nbits / nchans / nifs")
    nrows = rows.size // (hdr["nchans"] * hdr.get("nifs", 1))
    cands = np.asarray(cands)
    if cands.dtype != CUT_CAND:
        if cands.dtype.names is None or not {"dm", "sample", "width"} <= set(cands.dtype.names):
            raise InputError("candidates need the fields dm, sample and width (cutout_cands makes them from search records)")
        cands = cutout_cands(cands, None, dm_span)
    cands = np.ascontiguousarray(cands)
    if nf == 0:
        nf = max(d for d in range(1, min(256, hdr["nchans"]) + 1) if hdr["nchans"] % d == 0)
    par = _lib.FrbchCutoutParams(C.sizeof(_lib.FrbchCutoutParams), int(nt), int(nf), int(ndm))
    n = cands.size
    if n < 1 or not (0 < nt <= 1024 and 0 < nf <= hdr["nchans"] and 0 < ndm <= 1024):
        raise InputError("at least one candidate, nt and ndm in 1..1024, nf in 1..nchans")
    per_call = max(1, min(65535, ((1 << 31) - 1) // (max(nf, ndm) * nt), CUT_TABLE_CAP // (ndm * hdr["nchans"])))
    if batch > 0:
        per_call = min(per_call, int(batch))
    ft, ft_hits = np.zeros((n, nf, nt), np.float32), np.zeros((n, nf, nt), np.uint32)
    dt, dt_hits = np.zeros((n, ndm, nt), np.float32), np.zeros((n, ndm, nt), np.uint32)
    err = C.create_string_buffer(512)
    desc = fil_desc(hdr, hdr.get("product", 0))
    kernels = []
    for a in range(0, n, per_call):
        b = min(n, a + per_call)
        used = C.c_uint32(0)
        part = np.ascontiguousarray(cands[a:b])
        _check(lib.frbch_cutout_host(C.byref(desc), rows.ctypes.data, nrows, C.byref(par), part.ctypes.data, b - a, device,
                                     ft[a:b].ctypes.data, ft_hits[a:b].ctypes.data, dt[a:b].ctypes.data, dt_hits[a:b].ctypes.data,
                                     C.byref(used), err, len(err)), err)
        kernels.append(used.value)
    if info is not None:
        info["kernel_used"] = min(kernels)
        info["calls"] = len(kernels)
    return ft, ft_hits, dt, dt_hits


def _plane_mean(sums, hits):
    return np.where(hits > 0, sums.astype(np.float64) / np.maximum(hits, 1), 0.0).astype(np.float32)


def cand_name(base: str, tstart: float, tcand: float, dm: float, snr: float) -> str:
    """the image name utils/parse_fetch_image_name.py splits: tstart_, tcand_, dm_, snr_"""
    return "%s_cand_tstart_%.12f_tcand_%.7f_dm_%.5f_snr_%.5f" % (base, tstart, tcand, dm, snr)


def candidates_fil(filterbankfile, dm1, dm2=0, dmstep=1.0, zerodm=True, clip=5, threshold=5.0, max_width_s=0.0, detrend_len=1000,
                   widths=None, dm_gap=2, min_members=1, max_cands=0, nt=256, nf=0, ndm=256, dm_span=None, device=0, lib=None,
                   info: dict | None = None, flag_file=None, rfi=None, resident=False, periodic=None):
    """``search_fil``, then one candidate per pulse: the records are grouped across DMs (``group_candidates``), groups of
    fewer than ``min_members`` records are dropped, the ``max_cands`` strongest kept (0: all), and ONE frbch_cutout_host
    call cuts the two planes of all of them (``cutouts``: several calls only for a list longer than a call takes).  Writes, next to ``search_fil``'s own files (which are unchanged),
    ``<base>.cands.txt`` (one line per kept group) and per group ``<base>_cand_tstart_<mjd>_tcand_<s>_dm_<dm>_snr_<sigma>``
    ``.npz`` (data_freq_time [nt][nf] and data_dm_time [ndm][nt] as means = sums / hits, 0 where hits is 0; the four raw
    planes; the scalars) and ``.png`` (the frequency-time plane above the DM-time plane).
    ``flag_file`` / ``rfi`` as in ``search_fil``: the search AND the planes then see the cleaned rows (cleaned once; they
    travel to the device again for the search and for the cut-outs).  ``resident``: every stage in one library call on rows
    uploaded once (frbch_candidates_host) -- the same files and values; ``info`` gains ``row_uploads`` and the stage times.
    ``periodic`` as in ``search_fil``.
    Returns (list of .npz files, kept groups as a structured array)."""
    lib = lib or _lib.load()
    _periodic_args(periodic, rfi, resident)
    if resident:
        return _candidates_fil_resident(filterbankfile, dm1, dm2, dmstep, zerodm, clip, threshold, max_width_s, detrend_len, widths, dm_gap,
                                        min_members, max_cands, nt, nf, ndm, dm_span, device, lib, info, flag_file, rfi)
    sinfo = {}
    fil = _read_rows(filterbankfile, flag_file, rfi, device, lib, sinfo, detrend_len, periodic)
    _files, recs = _search(fil, filterbankfile, dm1, dm2, dmstep, zerodm, clip, threshold, max_width_s, detrend_len, False, widths,
                           device, lib, sinfo)
    hdr = fil.header
    dms = dm_list(dm1, dm2, dmstep)
    groups = group_candidates(recs, hdr, dms, dm_gap=dm_gap, lib=lib)
    groups = groups[groups["nmember"] >= min_members]
    if max_cands > 0 and groups.size > max_cands:
        keep = np.sort(np.argsort(-groups["best"]["sigma"], kind="stable")[:max_cands])
        groups = groups[keep]
    base = filterbankfile.replace(".fil", "")
    with open(base + ".cands.txt", "w") as f:
        f.write(CANDS_HEADER + "\n")
        for g in groups:
            b = g["best"]
            f.write(CANDS_ROW % (dms[int(b["dm_index"])], b["sigma"], int(b["sample"]) * hdr["tsamp"], int(b["sample"]), int(b["width"]),
                                 int(g["nmember"]), int(g["dm_index_lo"]), int(g["dm_index_hi"])) + "\n")
    if info is not None:
        info.update(sinfo, ngroup=int(groups.size), search_kernel_used=sinfo.get("kernel_used"))
    out = []
    if groups.size == 0:
        return out, groups
    cc = cutout_cands(groups["best"], dms, dm_span)
    cinfo = {}
    ft, ft_hits, dt, dt_hits = cutouts(fil, hdr, cc, nt=nt, nf=nf, ndm=ndm, device=device, lib=lib, info=cinfo)
    if info is not None:
        info["cutout_kernel_used"] = cinfo["kernel_used"]
    for i, (g, c) in enumerate(zip(groups, cc)):
        b = g["best"]
        tcand = int(b["sample"]) * hdr["tsamp"]
        name = cand_name(base, hdr["tstart"], tcand, c["dm"], float(b["sigma"]))
        ft_mean, dt_mean = _plane_mean(ft[i], ft_hits[i]), _plane_mean(dt[i], dt_hits[i])
        np.savez(name + ".npz", data_freq_time=ft_mean.T.copy(), data_dm_time=dt_mean, ft=ft[i], ft_hits=ft_hits[i], dt=dt[i],
                 dt_hits=dt_hits[i], tcand=tcand, dm=c["dm"], snr=float(b["sigma"]), width=int(b["width"]), tfactor=int(c["tfactor"]),
                 tsamp=hdr["tsamp"], fch1=hdr["fch1"], foff=hdr["foff"], nchans=hdr["nchans"], tstart=hdr["tstart"],
                 dm_lo=c["dm_lo"], dm_hi=c["dm_hi"])

        def unit(img):
            img = img - img.mean(axis=1, keepdims=True)
            return (img - img.min()) / max(1e-30, float(img.max() - img.min()))
        write_png(name + ".png", np.concatenate([unit(ft_mean), np.zeros((4, ft_mean.shape[1])), unit(dt_mean)], axis=0))
        out.append(name + ".npz")
    return out, groups


# ------------------------------------------------------------------------------------------------------------------
# resident rows: one upload per command (frbch_candidates_host, frbch_rfi_cleanp_host)
# ------------------------------------------------------------------------------------------------------------------
def _from_ptr(ptr, dtype, shape):
    """a copy of the library's array at ``ptr``; None for a NULL pointer"""
    if not ptr:
        return None
    dtype = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64))
    if n == 0:
        return np.zeros(shape, dtype)
    return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(ptr), dtype=dtype).reshape(shape).copy()


def select_groups(groups, min_members: int = 1, max_cands: int = 0, lib=None) -> np.ndarray:
    """The selection of ``candidates_fil`` as the library makes it (frbch_cand_select): indices, ascending, of the groups
    with at least ``min_members`` records, cut to the ``max_cands`` strongest (0: all; equal sigmas: the earlier group)."""
    lib = lib or _lib.load()
    g = np.ascontiguousarray(groups, dtype=SP_GROUP)
    keep = np.zeros(max(1, g.size), np.uint64)
    n = C.c_uint64(0)
    rc = lib.frbch_cand_select(g.ctypes.data if g.size else None, g.size, int(min_members), int(max_cands), keep.ctypes.data, keep.size,
                               C.byref(n))
    if rc < 0:
        raise InputError("min_members must be at least 1")
    return keep[: n.value].astype(np.int64)


def candidates_resident(rows, hdr: dict, dms, *, sp, rfi=None, zap=None, zerodm=True, clip=5.0, dm_gap=2, min_members=1, max_cands=0,
                        nt=256, nf=0, ndm=256, dm_span=None, keep_series=False, product=0, device=0, lib=None, d_rows=None,
                        nrows=None) -> dict:
    """Flagging (``rfi``: ``True`` or a dict of ``RFI_DEFAULTS`` keys; ``zap`` alone flags as well), the search of the DMs,
    grouping, selection and the cut-outs in ONE library call on rows that cross to the device once (frbch_candidates_host),
    or -- ``d_rows``: a device address, with ``nrows`` -- not at all (frbch_candidates_device, which leaves them as they
    are).  ``sp``: ``sp_params(...)``; ``nt = 0``: no planes.  -> dict of copies of everything in the library's result view
    (include/frbch.h): nout, nclipped, cands, ngroup_all, groups, cut_cands, ft / ft_hits / dt / dt_hits (None without
    planes), mask / repl / chan_flag / blk_flag (None without flagging), series (None unless ``keep_series``), kernel_used
    (RFI statistics, dedispersion, search, cut-out), cutout_calls, row_uploads, wall_ms and device_ms by stage name."""
    lib = lib or _lib.load()
    nchan, nifs = hdr["nchans"], hdr.get("nifs", 1)
    if d_rows is None:
        x = _rows3(rows, hdr)
        nrows, ptr = x.shape[0], x.ctypes.data
    else:
        ptr = int(d_rows)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    par = _lib.FrbchCandParams()
    par.size = C.sizeof(_lib.FrbchCandParams)
    z = _zap_array(zap, nchan)
    flag = bool(rfi) or z is not None
    par.flags = (_lib.CAND_RFI if flag else 0) | (_lib.CAND_SERIES if keep_series else 0)
    par.rfi = rfi_params(rfi if isinstance(rfi, (dict, _lib.FrbchRfiParams)) else None)
    par.zap = None if z is None else z.ctypes.data
    par.zerodm, par.clip_sigma = (1 if zerodm else 0), float(clip)
    par.sp = sp
    if min(int(dm_gap), int(min_members), int(max_cands)) < 0:
        raise InputError("dm_gap, min_members and max_cands must not be negative")
    par.dm_gap, par.min_members, par.max_cands = int(dm_gap), int(min_members), int(max_cands)
    if nt and nf == 0:
        nf = max(d for d in range(1, min(256, nchan) + 1) if nchan % d == 0)
    if min(int(nt), int(nf), int(ndm)) < 0:
        raise InputError("nt, nf and ndm must not be negative")
    par.cut = _lib.FrbchCutoutParams(C.sizeof(_lib.FrbchCutoutParams), int(nt), int(nf), int(ndm))
    if dm_span is not None and not float(dm_span) > 0.0:
        raise InputError("dm_span must be positive (None: the plane spans 0 .. 2 dm)")
    par.dm_span = 0.0 if dm_span is None else float(dm_span)
    desc = fil_desc(hdr, product)
    res = C.c_void_p(None)
    err = C.create_string_buffer(2048)
    call = lib.frbch_candidates_host if d_rows is None else lib.frbch_candidates_device
    _check(call(C.byref(desc), ptr, int(nrows), dm_arr.ctypes.data, dm_arr.size, C.byref(par), device, C.byref(res), err, len(err)), err)
    try:
        v = _lib.FrbchCandView()
        v.size = C.sizeof(_lib.FrbchCandView)
        if lib.frbch_cand_result_view(res, C.byref(v)) != 0:
            raise RunError("frbch_cand_result_view refused the view")
        n = int(v.ngroup)
        out = dict(nout=int(v.nout), nclipped=int(v.nclipped), ngroup_all=int(v.ngroup_all),
                   cands=_from_ptr(v.cands, SP_CAND, (int(v.ncand),)) if v.ncand else np.zeros(0, SP_CAND),
                   groups=_from_ptr(v.groups, SP_GROUP, (n,)) if n else np.zeros(0, SP_GROUP),
                   cut_cands=_from_ptr(v.cut_cands, CUT_CAND, (n,)) if n else np.zeros(0, CUT_CAND),
                   ft=_from_ptr(v.ft, np.float32, (n, int(nf), int(nt))), ft_hits=_from_ptr(v.ft_hits, np.uint32, (n, int(nf), int(nt))),
                   dt=_from_ptr(v.dt, np.float32, (n, int(ndm), int(nt))), dt_hits=_from_ptr(v.dt_hits, np.uint32, (n, int(ndm), int(nt))),
                   nblk=int(v.nblk), mask=_from_ptr(v.mask, np.uint8, (int(v.nblk), nchan)), repl=_from_ptr(v.repl, np.float64, (nchan,)),
                   chan_flag=_from_ptr(v.chan_flag, np.uint8, (nchan,)), blk_flag=_from_ptr(v.blk_flag, np.uint8, (int(v.nblk),)),
                   series=_from_ptr(v.series, np.float32, (dm_arr.size, int(v.nout))), kernel_used=[int(k) for k in v.kernel_used],
                   cutout_calls=int(v.cutout_calls), row_uploads=int(v.row_uploads),
                   wall_ms=dict(zip(_lib.CAND_STAGES, [float(t) for t in v.wall_ms])),
                   device_ms=dict(zip(_lib.CAND_STAGES, [float(t) for t in v.device_ms])))
    finally:
        lib.frbch_cand_result_free(res)
    return out


def _resident_run(filterbankfile, dm1, dm2, dmstep, zerodm, clip, threshold, max_width_s, detrend_len, widths, device, lib, info,
                  flag_file, rfi, **kw):
    """``_read_rows`` and ``_search`` of the resident commands: the file, its DMs and ``candidates_resident`` of its rows;
    ``info`` receives what the two give it, plus row_uploads and the stage times"""
    fil = sigproc.read_fil(filterbankfile)
    hdr = fil.header
    dms = dm_list(dm1, dm2, dmstep)
    rows = _rows_of(fil)
    desc = fil_desc(hdr)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    if lib.frbch_dedisperse_nout(C.byref(desc), rows.shape[0], dm_arr.ctypes.data, dm_arr.size) <= 0:
        raise InputError("the dispersion delay across the band exceeds the length of the filterbank")
    zap = read_flag_file(flag_file, hdr["nchans"]) if flag_file is not None else None
    flag = flag_file is not None or bool(rfi)
    params = sp_params(widths if widths is not None else default_widths(hdr["tsamp"], max_width_s), threshold, detrend_len)
    r = candidates_resident(rows, hdr, dms, sp=params, rfi=(rfi if isinstance(rfi, dict) else True) if flag else None, zap=zap,
                            zerodm=zerodm, clip=float(clip), device=device, lib=lib, **kw)
    if flag:
        if info is not None:
            info.update(rfi_kernel_used=r["kernel_used"][0], rfi_chan_flag=r["chan_flag"].astype(bool), rfi_blk_flag=r["blk_flag"].astype(bool),
                        rfi_mask=r["mask"], rfi_masked_cells=int(r["mask"].sum()))
        block_rows = rfi_params(rfi if isinstance(rfi, dict) else None).block_rows
        if r["blk_flag"].any() and not r["chan_flag"].all() and 2 * block_rows > (detrend_len or 1000):
            import warnings
            warnings.warn("%d block(s) of %d rows flagged wholly: each is a flat stretch of every dedispersed series, longer than half a "
                          "normalisation block of the search (detrend_len = %d), which can then report the noise at the stretch's edges; "
                          "use shorter blocks, e.g. rfi=dict(block_rows=256)" % (int(r["blk_flag"].sum()), block_rows, detrend_len or 1000))
    if info is not None:
        info.update(kernel_used=r["kernel_used"][2], nclipped=r["nclipped"], nout=r["nout"], row_uploads=r["row_uploads"],
                    dedisperse_kernel_used=r["kernel_used"][1], wall_ms=r["wall_ms"], device_ms=r["device_ms"])
    return hdr, dms, r


def _resident_singlepulse(filterbankfile, dm1, dm2, dms, hdr, r, write_dat):
    """the files of ``_search`` from a resident result"""
    out = []
    for i, (name, dm) in enumerate(zip(_series_names(filterbankfile, dm1, dm2, dms), dms)):
        write_singlepulse(name + ".singlepulse", r["cands"][r["cands"]["dm_index"] == i], dm, hdr["tsamp"])
        out.append(name + ".singlepulse")
        if write_dat:
            r["series"][i].astype("<f4").tofile(name + ".dat")
            write_inf(name + ".inf", basename=os.path.basename(name), hdr=hdr, nsamp=r["nout"], dm=dm, clipped=r["nclipped"])
    return out


def _search_fil_resident(filterbankfile, dm1, dm2, dmstep, zerodm, clip, threshold, max_width_s, detrend_len, write_dat, widths, device,
                         lib, info, flag_file, rfi):
    hdr, dms, r = _resident_run(filterbankfile, dm1, dm2, dmstep, zerodm, clip, threshold, max_width_s, detrend_len, widths, device, lib,
                                info, flag_file, rfi, nt=0, keep_series=bool(write_dat))
    return _resident_singlepulse(filterbankfile, dm1, dm2, dms, hdr, r, write_dat), r["cands"]


def _candidates_fil_resident(filterbankfile, dm1, dm2, dmstep, zerodm, clip, threshold, max_width_s, detrend_len, widths, dm_gap,
                             min_members, max_cands, nt, nf, ndm, dm_span, device, lib, info, flag_file, rfi):
    sinfo = {}
    hdr, dms, r = _resident_run(filterbankfile, dm1, dm2, dmstep, zerodm, clip, threshold, max_width_s, detrend_len, widths, device, lib,
                                sinfo, flag_file, rfi, dm_gap=dm_gap, min_members=min_members, max_cands=max_cands, nt=nt, nf=nf, ndm=ndm,
                                dm_span=dm_span)
    _resident_singlepulse(filterbankfile, dm1, dm2, dms, hdr, r, False)
    groups, cc = r["groups"], r["cut_cands"]
    base = filterbankfile.replace(".fil", "")
    with open(base + ".cands.txt", "w") as f:
        f.write(CANDS_HEADER + "\n")
        for g in groups:
            b = g["best"]
            f.write(CANDS_ROW % (dms[int(b["dm_index"])], b["sigma"], int(b["sample"]) * hdr["tsamp"], int(b["sample"]), int(b["width"]),
                                 int(g["nmember"]), int(g["dm_index_lo"]), int(g["dm_index_hi"])) + "\n")
    if info is not None:
        info.update(sinfo, ngroup=int(groups.size), search_kernel_used=sinfo.get("kernel_used"))
    out = []
    if groups.size == 0:
        return out, groups
    if info is not None:
        info["cutout_kernel_used"] = r["kernel_used"][3]
        info["cutout_calls"] = r["cutout_calls"]
    ft, ft_hits, dt, dt_hits = r["ft"], r["ft_hits"], r["dt"], r["dt_hits"]
    for i, (g, c) in enumerate(zip(groups, cc)):
        b = g["best"]
        tcand = int(b["sample"]) * hdr["tsamp"]
        name = cand_name(base, hdr["tstart"], tcand, c["dm"], float(b["sigma"]))
        ft_mean, dt_mean = _plane_mean(ft[i], ft_hits[i]), _plane_mean(dt[i], dt_hits[i])
        np.savez(name + ".npz", data_freq_time=ft_mean.T.copy(), data_dm_time=dt_mean, ft=ft[i], ft_hits=ft_hits[i], dt=dt[i],
                 dt_hits=dt_hits[i], tcand=tcand, dm=c["dm"], snr=float(b["sigma"]), width=int(b["width"]), tfactor=int(c["tfactor"]),
                 tsamp=hdr["tsamp"], fch1=hdr["fch1"], foff=hdr["foff"], nchans=hdr["nchans"], tstart=hdr["tstart"],
                 dm_lo=c["dm_lo"], dm_hi=c["dm_hi"])
        img = [u - u.mean(axis=1, keepdims=True) for u in (ft_mean, dt_mean)]
        img = [(u - u.min()) / max(1e-30, float(u.max() - u.min())) for u in img]
        write_png(name + ".png", np.concatenate([img[0], np.zeros((4, ft_mean.shape[1])), img[1]], axis=0))
        out.append(name + ".npz")
    return out, groups


def cleanp(rows, hdr: dict, params=None, zap=None, device: int = 0, lib=None, info: dict | None = None, want_stats: bool = False):
    """``clean`` of ALL products in one residency (frbch_rfi_cleanp_host: one upload, one download of the rows) -> (cleaned copy
    of the rows, dict(mask, repl [nifs][nchan], chan_flag, blk_flag and, with ``want_stats``, stats [nifs][nblk][nchan][2]))."""
    lib = lib or _lib.load()
    x = _rows3(rows, hdr).copy()
    par = rfi_params(params)
    nifs, nchan = x.shape[1], x.shape[2]
    nblk = lib.frbch_rfi_nblk(x.shape[0], par.block_rows)
    if nblk <= 0:
        raise InputError("block_rows must be 1..2^20")
    z = _zap_array(zap, nchan)
    mask, repl = np.zeros((nblk, nchan), np.uint8), np.zeros((nifs, nchan), np.float64)
    cf, bf = np.zeros(nchan, np.uint8), np.zeros(nblk, np.uint8)
    stats = np.zeros((nifs, nblk, nchan, 2), np.float64 if hdr["nbits"] == 32 else np.uint64) if want_stats else None
    used = C.c_uint32(0)
    err = C.create_string_buffer(512)
    desc = fil_desc(hdr)
    _check(lib.frbch_rfi_cleanp_host(C.byref(desc), x.ctypes.data, x.shape[0], C.byref(par), None if z is None else z.ctypes.data, device,
                                     mask.ctypes.data, repl.ctypes.data, cf.ctypes.data, bf.ctypes.data,
                                     None if stats is None else stats.ctypes.data, C.byref(used), err, len(err)), err)
    if info is not None:
        info.update(kernel_used=used.value, row_uploads=1, row_downloads=1)
    res = dict(mask=mask, repl=repl, chan_flag=cf.astype(bool), blk_flag=bf.astype(bool))
    if want_stats:
        res["stats"] = stats
    return x.reshape(np.shape(rows)), res


# ------------------------------------------------------------------------------------------------------------------
# fold
# ------------------------------------------------------------------------------------------------------------------
def read_par(path: str) -> dict:
    """F0 / F1 / PEPOCH / DM of a psrcat -e style ephemeris (base2fil.sh:465: `psrcat -e <target> > <target>.psrcat.par`);
    P0 / P1 are accepted instead of F0 / F1."""
    vals = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if len(parts) >= 2:
                try:
                    vals[parts[0].upper()] = float(parts[1].replace("D", "E"))
                except ValueError:
                    vals[parts[0].upper()] = parts[1]
    if "F0" not in vals:
        if "P0" not in vals or not isinstance(vals["P0"], float):
            raise InputError(f"{path}: neither F0 nor P0")
        p0, p1 = vals["P0"], float(vals.get("P1", 0.0) or 0.0)
        vals["F0"] = 1.0 / p0
        vals["F1"] = -p1 / (p0 * p0)
    out = {"F0": float(vals["F0"]), "F1": float(vals.get("F1", 0.0) or 0.0), "DM": float(vals.get("DM", 0.0) or 0.0)}
    out["PEPOCH"] = float(vals["PEPOCH"]) if isinstance(vals.get("PEPOCH"), float) else None
    out["PSR"] = str(vals.get("PSRJ", vals.get("PSRB", vals.get("PSR", "unknown"))))
    return out


def default_nbin(f0: float, tsamp: float, cap: int = 1024) -> int:
    """largest power of two not above period / tsamp (no bin narrower than a sample), at most ``cap``"""
    n = max(2.0, 1.0 / (f0 * tsamp))
    nb = 2
    while nb * 2 <= n and nb * 2 <= cap:
        nb *= 2
    return nb


def fold(fil: sigproc.SigprocFile, par: dict, nbin: int = 0, subint_s: float = 10.0, apply_delays: bool = False,
         device: int = 0, lib=None):
    """-> (profile float64 [nsub][nchan][nbin] sums, hits uint32 same shape, nbin).  PEPOCH defaults to tstart."""
    lib = lib or _lib.load()
    rows = _rows_of(fil)
    desc = fil_desc(fil.header)
    nbin = nbin or default_nbin(par["F0"], fil.header["tsamp"])
    pepoch = par["PEPOCH"] if par.get("PEPOCH") is not None else fil.header["tstart"]
    nsub = lib.frbch_fold_nsub(C.byref(desc), rows.shape[0], float(subint_s))
    if nsub <= 0:
        raise InputError("bad sub-integration length")
    prof = np.zeros((nsub, nbin, desc.nchan), dtype=np.float64)
    hits = np.zeros((nsub, nbin, desc.nchan), dtype=np.uint32)
    err = C.create_string_buffer(512)
    _check(lib.frbch_fold_host(C.byref(desc), rows.ctypes.data, rows.shape[0], par["F0"], par["F1"], pepoch, par["DM"],
                               1 if apply_delays else 0, nbin, float(subint_s), device, prof.ctypes.data, hits.ctypes.data,
                               nsub, err, len(err)), err)
    return prof.transpose(0, 2, 1).copy(), hits.transpose(0, 2, 1).copy(), nbin


def _num(text: str) -> float:
    return float(text.replace("D", "E").replace("d", "e"))


def read_polyco(path: str) -> list:
    """Blocks of a TEMPO ``polyco.dat`` (what ``tempo -z`` and ``tempo2 -f <par> -polyco "..." -tempo1`` write), parsed by
    whitespace, ``D`` exponents accepted.  Line 1: name, date, UTC, TMID, DM, Doppler, log10 rms; line 2: RPHASE, F0,
    site, span (minutes), ncoeff, observing frequency, then the optional binary phase and frequency; then
    ceil(ncoeff / 3) lines of coefficients.  ``rphase`` is the FRACTION of RPHASE in [0, 1), taken from the text in
    decimal arithmetic: a 1e10-turn RPHASE keeps all of its fraction (``rphase_turns`` is the whole number dropped)."""
    import decimal
    with open(path) as f:
        lines = [ln.split() for ln in f if ln.strip()]
    segs, i = [], 0
    while i < len(lines):
        if i + 1 >= len(lines) or len(lines[i]) < 5 or len(lines[i + 1]) < 6:
            raise InputError(f"{path}: truncated polyco block at line {i + 1}")
        a, b = lines[i], lines[i + 1]
        try:
            ncoeff = int(b[4])
            if not 1 <= ncoeff <= 15:
                raise InputError(f"{path}: {ncoeff} coefficients in a block (1..15)")
            nlines = (ncoeff + 2) // 3
            coeff = [_num(w) for ln in lines[i + 2: i + 2 + nlines] for w in ln]
            if len(coeff) != ncoeff:
                raise InputError(f"{path}: block at line {i + 1} holds {len(coeff)} coefficients, header says {ncoeff}")
            with decimal.localcontext() as ctx:
                ctx.prec = 60
                r = decimal.Decimal(b[0].replace("D", "E").replace("d", "e"))
                whole = r.to_integral_value(rounding=decimal.ROUND_FLOOR)
                frac = float(r - whole)
            if frac >= 1.0:                       # (a negative fraction below 1 ulp of 1.0)
                frac = 0.0
            seg = {"psr": a[0], "date": a[1], "utc": a[2], "tmid": _num(a[3]), "dm": _num(a[4]),
                   "doppler": _num(a[5]) if len(a) > 5 else 0.0, "log10rms": _num(a[6]) if len(a) > 6 else 0.0,
                   "rphase": frac, "rphase_turns": int(whole), "f0": _num(b[1]), "site": b[2], "span": _num(b[3]),
                   "ncoeff": ncoeff, "obsfreq": _num(b[5]),
                   "binphase": _num(b[6]) if len(b) > 6 else None, "binfreq": _num(b[7]) if len(b) > 7 else None,
                   "coeff": coeff}
        except ValueError as exc:
            raise InputError(f"{path}: bad number in the polyco block at line {i + 1}: {exc}") from exc
        segs.append(seg)
        i += 2 + nlines
    if not segs:
        raise InputError(f"{path}: no polyco blocks")
    return segs


def fold_model(par: dict, hdr: dict, *, polyco=None, doppler: float = 0.0, nbin: int, subint_s: float, apply_delays: bool):
    """-> (FrbchFoldModel, the ctypes block array it points to: keep it alive for the call)"""
    m = _lib.FrbchFoldModel()
    m.size = C.sizeof(_lib.FrbchFoldModel)
    segs = read_polyco(polyco) if isinstance(polyco, (str, os.PathLike)) else (polyco or [])
    arr = (_lib.FrbchPolycoSeg * max(1, len(segs)))()
    for dst, g in zip(arr, segs):
        dst.tmid_mjd, dst.rphase_frac, dst.f0_hz, dst.span_min = g["tmid"], g["rphase"], g["f0"], g["span"]
        dst.ncoeff = g.get("ncoeff", len(g["coeff"]))          # (the library refuses anything outside 1..15)
        for k, v in enumerate(g["coeff"][:15]):
            dst.coeff[k] = v
    m.nseg = len(segs)
    m.seg = C.cast(arr, C.POINTER(_lib.FrbchPolycoSeg)) if segs else None
    m.f0_hz = par.get("F0") or (segs[0]["f0"] if segs else 0.0)
    m.f1 = par.get("F1", 0.0) or 0.0
    m.pepoch_mjd = par["PEPOCH"] if par.get("PEPOCH") is not None else hdr["tstart"]
    m.doppler = float(doppler)
    m.dm = par.get("DM", 0.0) or 0.0
    m.apply_delays = 1 if apply_delays else 0
    m.nbin = nbin
    m.subint_s = float(subint_s)
    return m, arr


def fold_all(fil: sigproc.SigprocFile, par: dict, *, polyco=None, doppler: float = 0.0, nbin: int = 0, subint_s: float = 10.0,
             apply_delays: bool = False, device: int = 0, lib=None, info: dict | None = None):
    """Every product of the file in one pass -> (profile float64 [nsub][nprod][nchan][nbin] sums, hits uint32
    [nsub][nchan][nbin] shared by the products, nbin).  ``polyco``: a TEMPO polyco file or the blocks ``read_polyco``
    returns -- the phase then follows the predictor (``par`` supplies DM, and F0 for the default nbin); otherwise the
    F0 / F1 / PEPOCH polynomial of ``fold``, with ``doppler`` = observed / intrinsic spin frequency - 1 applied to the
    elapsed time.  ``info['kernel_used']`` receives 1 when the LDS kernel ran, 0 for the generic one."""
    lib = lib or _lib.load()
    rows = _rows_of(fil)
    desc = fil_desc(fil.header)
    segs = read_polyco(polyco) if isinstance(polyco, (str, os.PathLike)) else polyco
    f0 = par.get("F0") or (segs[0]["f0"] if segs else 0.0)
    nbin = nbin or default_nbin(f0, fil.header["tsamp"])
    model, _keep = fold_model(par, fil.header, polyco=segs, doppler=doppler, nbin=nbin, subint_s=subint_s, apply_delays=apply_delays)
    nsub = lib.frbch_fold_nsub(C.byref(desc), rows.shape[0], float(subint_s))
    if nsub <= 0:
        raise InputError("bad sub-integration length")
    prof = np.zeros((nsub, desc.nifs, nbin, desc.nchan), dtype=np.float64)
    hits = np.zeros((nsub, nbin, desc.nchan), dtype=np.uint32)
    err = C.create_string_buffer(512)
    used = C.c_uint32(0)
    _check(lib.frbch_foldp_host(C.byref(desc), rows.ctypes.data, rows.shape[0], C.byref(model), device, prof.ctypes.data,
                                hits.ctypes.data, nsub, C.byref(used), err, len(err)), err)
    if info is not None:
        info["kernel_used"] = used.value
    return prof.transpose(0, 1, 3, 2).copy(), hits.transpose(0, 2, 1).copy(), nbin


def stokes(prof: np.ndarray, products: str = "coherency", axis: int = 1) -> np.ndarray:
    """Folded products -> Stokes I, Q, U, V along ``axis`` (4 long).  ``coherency``: PP, QQ, Re(PQ*), Im(PQ*) of a `-d4`
    file, circular basis (include/frbch.h): I = PP + QQ, Q = 2 Re(PQ*), U = 2 Im(PQ*), V = PP - QQ.  ``stokes``: the file
    holds I, Q, U, V already (the IQUV extension) and passes through.

    A rescaled 8- or 16-bit file has had the bandpass offset and scale of EVERY product removed separately before
    digitising, so the products no longer share one flux scale: the Stokes parameters keep their shape in phase (pulse
    position, PA swing sign changes), but polarisation FRACTIONS (L / I, V / I) are faithful only for `-I0` (no rescale)
    or float output."""
    prof = np.asarray(prof)
    if prof.shape[axis] != 4:
        raise InputError(f"Stokes parameters need 4 products, not {prof.shape[axis]}")
    if products == "stokes":
        return prof
    if products != "coherency":
        raise InputError("products must be 'coherency' or 'stokes'")
    pp, qq, re, im = (np.take(prof, k, axis=axis) for k in range(4))
    return np.stack([pp + qq, 2.0 * re, 2.0 * im, pp - qq], axis=axis)


def remove_baseline(profiles: np.ndarray) -> np.ndarray:
    """subtract each product's off-pulse level (the median over phase: the pulse fills well under half a turn) -- last axis = bins"""
    p = np.asarray(profiles, dtype=np.float64)
    return p - np.median(p, axis=-1, keepdims=True)


def linear_pa(iquv: np.ndarray):
    """[4][nbin] Stokes profiles -> (I, L, V, PA in radians) with the off-pulse baseline of every product removed;
    L = sqrt(Q^2 + U^2), PA = atan2(U, Q) / 2"""
    i, q, u, v = remove_baseline(iquv)
    return i, np.hypot(q, u), v, 0.5 * np.arctan2(u, q)


def dedisperse_profile(prof: np.ndarray, hdr: dict, f0: float, dm: float) -> np.ndarray:
    """rotate every channel's profile by its dispersion delay (nearest bin): `psrplot -j dedisperse`"""
    nsub, nchan, nbin = prof.shape
    fc = hdr["fch1"] + np.arange(nchan) * hdr["foff"]
    fhi = fc.max()
    delay = dm * DM_CONST * (fc ** -2 - fhi ** -2)
    shift = np.rint(delay * f0 * nbin).astype(np.int64) % nbin
    out = np.empty_like(prof)
    for c in range(nchan):
        out[:, c, :] = np.roll(prof[:, c, :], -int(shift[c]), axis=1)
    return out


ARCHIVE_MAGIC = b"FRBFOLD1"


def write_archive(path: str, prof: np.ndarray, hits: np.ndarray, meta: dict) -> None:
    """one file: magic, JSON header (length-prefixed), float64 sums [nsub][nchan][nbin] -- [nsub][nprod][nchan][nbin] when
    the header has "nprod" --, uint32 hits [nsub][nchan][nbin]"""
    head = json.dumps(meta, sort_keys=True).encode()
    with open(path, "wb") as f:
        f.write(ARCHIVE_MAGIC + struct.pack("<I", len(head)) + head)
        f.write(np.ascontiguousarray(prof, dtype="<f8").tobytes())
        f.write(np.ascontiguousarray(hits, dtype="<u4").tobytes())


def read_archive(path: str):
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:8] != ARCHIVE_MAGIC:
        raise InputError(f"{path}: not a FRBFOLD1 archive")
    (n,) = struct.unpack_from("<I", buf, 8)
    meta = json.loads(buf[12:12 + n].decode())
    shape = (meta["nsub"], meta["nchan"], meta["nbin"])
    cnt = shape[0] * shape[1] * shape[2]
    if "nprod" in meta:       # every product: sums [nsub][nprod][nchan][nbin], then the hits they share
        pshape = (meta["nsub"], meta["nprod"], meta["nchan"], meta["nbin"])
        prof = np.frombuffer(buf, dtype="<f8", count=cnt * meta["nprod"], offset=12 + n).reshape(pshape)
        hits = np.frombuffer(buf, dtype="<u4", count=cnt, offset=12 + n + 8 * cnt * meta["nprod"]).reshape(shape)
        return prof, hits, meta
    prof = np.frombuffer(buf, dtype="<f8", count=cnt, offset=12 + n).reshape(shape)
    hits = np.frombuffer(buf, dtype="<u4", count=cnt, offset=12 + n + 8 * cnt).reshape(shape)
    return prof, hits, meta


def write_png(path: str, img: np.ndarray) -> None:
    """minimal 8-bit greyscale PNG writer (no plotting library in the pipeline image)"""
    a = np.asarray(img, dtype=np.float64)
    lo, hi = float(a.min()), float(a.max())
    g = np.zeros(a.shape, np.uint8) if hi <= lo else np.clip((a - lo) / (hi - lo) * 255.0 + 0.5, 0, 255).astype(np.uint8)
    raw = b"".join(b"\x00" + g[r].tobytes() for r in range(g.shape[0]))

    def chunk(tag, data):
        c = struct.pack(">I", len(data)) + tag + data
        return c + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", g.shape[1], g.shape[0], 8, 0, 0, 0, 0))
    png += chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(png)


def _scrunched(prof, hits, hdr, f0, dm, fscrunch_to):
    """`psrplot -j dedisperse,tscrunch,"fscrunch N"`: [nsub][nchan][nbin] sums and hits -> (mean sample [nf][nbin], the
    frequency-scrunched mean profile [nbin])"""
    nbin = prof.shape[2]
    dd = dedisperse_profile(prof, hdr, f0, dm)
    hh = dedisperse_profile(hits.astype(np.float64), hdr, f0, dm)
    tot, cnt = dd.sum(axis=0), hh.sum(axis=0)                                   # tscrunch
    nchan = tot.shape[0]
    fs = max(1, nchan // max(1, min(fscrunch_to, nchan)))
    nf = nchan // fs
    tot_f = tot[: nf * fs].reshape(nf, fs, nbin).sum(axis=1)
    cnt_f = cnt[: nf * fs].reshape(nf, fs, nbin).sum(axis=1)
    mean_f = np.where(cnt_f > 0, tot_f / np.maximum(cnt_f, 1), 0.0)
    profile = np.where(cnt.sum(axis=0) > 0, tot.sum(axis=0) / np.maximum(cnt.sum(axis=0), 1), 0.0)
    return mean_f, profile


def _unit(img):
    """an image scaled to 0 .. 1, for the plots"""
    return (img - img.min()) / max(1e-30, float(img.max() - img.min()))


def _trace_panel(i, l, v, pa, height):
    """the Stokes profile panel of `psrplot -p stokes`-style plots as a raster: PA (where L stands out of its off-pulse
    scatter) in the top quarter, I (white), L (light grey) and V (mid grey) below on one flux scale"""
    nbin = i.size
    img = np.zeros((height, nbin))
    top = max(4, height // 4)
    sig = 1.4826 * np.median(np.abs(l - np.median(l)))
    for b in np.nonzero(l > np.median(l) + 5.0 * max(sig, 1e-30))[0]:
        img[int(round((0.5 - pa[b] / np.pi) * (top - 1))), b] = 1.0
    lo, hi = min(i.min(), v.min(), 0.0), max(i.max(), l.max(), v.max())
    rows = height - top - 1
    for curve, grey in ((v, 0.45), (l, 0.7), (i, 1.0)):
        y = top + rows - np.rint((curve - lo) / max(1e-30, hi - lo) * rows).astype(int)
        for b in range(nbin):
            y0, y1 = sorted((y[b], y[min(b + 1, nbin - 1)]))                     # (joined to the next bin)
            img[y0: y1 + 1, b] = grey
    return img


def fold_fil(filterbankfile: str, parfile: str, nbin: int = 0, subint_s: float = 10.0, fscrunch_to: int = 128,
             device: int = 0, lib=None, out_base: str | None = None, polyco: str | None = None, doppler: float = 0.0,
             products: str = "coherency"):
    """base2fil.sh:465-493 for one filterbank: fold with the ephemeris, write ``<fil>.ar`` (FRBFOLD1), the profile as
    text (``<fil>.profile.txt``: bin, mean flux of the dedispersed, scrunched profile) and the phase-frequency plot
    ``<fil>.png`` (dedispersed, time-scrunched, frequency-scrunched to ``fscrunch_to`` channels, profile strip on top).

    ``polyco``: a TEMPO polyco file made from the same .par -- the fold follows the predictor, as dspsr's does
    (barycentric, binary and position terms); ``doppler``: a constant Doppler factor for the polynomial instead.  A file
    with several products (nifs > 1) is folded in all of them in one pass: the archive holds them (header ``nprod``),
    the total-intensity outputs use Stokes I, and a four-product file (``products``: ``coherency`` = the `-d4` products,
    ``stokes`` = an IQUV file) also gives ``<fil>_fullPol.png`` -- pol 0, pol 1, Stokes I phase-frequency, and the
    I / L / V profile with the position angle: the 2x2 plot of base2fil.sh:483-490 -- and I, L, V, PA columns in the text
    profile (off-pulse baseline removed per product; see ``stokes`` on what a rescaled file keeps of the fractions)."""
    return _fold_par(sigproc.read_fil(filterbankfile), filterbankfile, read_par(parfile), nbin, subint_s, fscrunch_to, device, lib,
                     out_base, polyco, doppler, products)


def _fold_par(fil, filterbankfile, par, nbin, subint_s, fscrunch_to, device, lib, out_base, polyco, doppler, products):
    """``fold_fil`` on a file already read, with the ephemeris as the dict ``read_par`` gives (``psearch_fil`` builds one from a
    candidate)"""
    hdr = fil.header
    nprod = hdr.get("nifs", 1)
    timing = "topocentric polynomial F0, F1 about PEPOCH (no barycentric, binary or position terms)"
    prof_all = None
    if nprod > 1 or polyco is not None or doppler != 0.0:
        segs = read_polyco(polyco) if polyco is not None else None
        prof_all, hits, nbin = fold_all(fil, par, polyco=segs, doppler=doppler, nbin=nbin, subint_s=subint_s, apply_delays=False,
                                        device=device, lib=lib)
        if segs:
            timing = "TEMPO polyco predictor, %d blocks, site %s (%s)" % (len(segs), segs[0]["site"], os.path.basename(polyco))
        elif doppler != 0.0:
            timing = "polynomial F0, F1 about PEPOCH, elapsed time stretched by the Doppler factor %.12g" % doppler
        prof = stokes(prof_all, products)[:, 0] if nprod == 4 else prof_all[:, 0]
    else:
        prof, hits, nbin = fold(fil, par, nbin=nbin, subint_s=subint_s, apply_delays=False, device=device, lib=lib)
    base = out_base or filterbankfile
    meta = {"source": par["PSR"], "f0": par["F0"], "f1": par["F1"], "dm": par["DM"],
            "pepoch": par["PEPOCH"] if par["PEPOCH"] is not None else hdr["tstart"], "dedispersed": False,
            "nsub": int(prof.shape[0]), "nchan": int(prof.shape[1]), "nbin": int(nbin), "subint_s": subint_s,
            "tstart": hdr["tstart"], "tsamp": hdr["tsamp"], "fch1": hdr["fch1"], "foff": hdr["foff"],
            "timing": timing}
    if nprod > 1:
        meta["nprod"] = int(nprod)
        meta["products"] = products
        write_archive(base + ".ar", prof_all, hits, meta)
    else:
        write_archive(base + ".ar", prof, hits, meta)
    mean_f, profile = _scrunched(prof, hits, hdr, par["F0"], par["DM"], fscrunch_to)
    nf = mean_f.shape[0]
    pol = None
    if nprod == 4:
        iquv = stokes(prof_all, products)
        flat = [_scrunched(iquv[:, k], hits, hdr, par["F0"], par["DM"], fscrunch_to) for k in range(4)]
        pol = linear_pa(np.stack([f[1] for f in flat]))
        if products == "coherency":
            pol01 = [_scrunched(prof_all[:, k], hits, hdr, par["F0"], par["DM"], fscrunch_to)[0] for k in (0, 1)]
        else:                                                                   # circular feeds: I = PP + QQ, V = PP - QQ
            pol01 = [0.5 * (flat[0][0] + flat[3][0]), 0.5 * (flat[0][0] - flat[3][0])]
    with open(base + ".profile.txt", "w") as f:
        if pol is None:
            f.write("# bin  mean_sample   (dedispersed DM=%g, tscrunched, fscrunched; %s)\n" % (par["DM"], par["PSR"]))
            for i, v in enumerate(profile):
                f.write("%d %.9g\n" % (i, v))
        else:
            f.write("# bin  mean_sample  I  L  V  PA_deg   (dedispersed DM=%g, tscrunched, fscrunched, baselines removed; %s)\n"
                    % (par["DM"], par["PSR"]))
            for i, v in enumerate(profile):
                f.write("%d %.9g %.9g %.9g %.9g %.6f\n" % (i, v, pol[0][i], pol[1][i], pol[2][i], np.degrees(pol[3][i])))
    strip = np.tile((profile - profile.min()) / max(1e-30, profile.max() - profile.min()), (max(8, nf // 8), 1))
    wf = mean_f - mean_f.mean(axis=1, keepdims=True)
    wf = (wf - wf.min()) / max(1e-30, wf.max() - wf.min())
    write_png(base + ".png", np.concatenate([strip, wf], axis=0))
    if pol is not None:
        height = max(nf, 32)
        rep = -(-height // nf)
        panels = [np.repeat(_unit(m), rep, axis=0)[:height] for m in (pol01[0], pol01[1], flat[0][0])]
        panels.append(_trace_panel(*pol, height))
        gap_v, gap_h = np.zeros((height, 4)), np.zeros((4, 2 * nbin + 4))
        write_png(base + "_fullPol.png", np.concatenate([np.concatenate([panels[0], gap_v, panels[1]], axis=1), gap_h,
                                                         np.concatenate([panels[2], gap_v, panels[3]], axis=1)], axis=0))
    return base + ".ar", profile


# ------------------------------------------------------------------------------------------------------------------
# refinement of a fold: DM, spin frequency and frequency derivative (frbch_foldfit_*, frbch_fold_refine_*)
# ------------------------------------------------------------------------------------------------------------------
FOLDFIT_RESULT = np.dtype([("dm", "<f8"), ("dm_res", "<f8"), ("dfreq", "<f8"), ("dfreq_res", "<f8"), ("dfdot", "<f8"), ("dfdot_res", "<f8"),
                           ("score_peak", "<f8"), ("score_nominal", "<f8"), ("border_median", "<f8"), ("snr_nominal", "<f8"),
                           ("snr_best", "<f8"), ("kpeak", "<u4"), ("jpeak", "<u4"), ("ipeak", "<u4"), ("fitted_dm", "<u4"),
                           ("fitted_freq", "<u4"), ("fitted_fdot", "<u4"), ("nfit_dm", "<u4"), ("nfit_freq", "<u4"), ("nfit_fdot", "<u4"),
                           ("width_nominal", "<u4"), ("bin_nominal", "<u4"), ("width_best", "<u4"), ("bin_best", "<u4"), ("reserved", "<u4")])
FOLDFIT_WIDTHS = (1, 2, 4, 8, 16, 32)


def foldfit_steps(hdr: dict, nrows: int, nbin: int, f0_fold: float, lib=None):
    """-> (ddm, dfreq, dfdot): one bin at the bottom of the band, over the span, at the ends of the span (frbch_foldfit_steps)"""
    lib = lib or _lib.load()
    ddm, dfreq, dfdot = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    if lib.frbch_foldfit_steps(C.byref(fil_desc(hdr)), int(nrows), int(nbin), float(f0_fold), C.byref(ddm), C.byref(dfreq), C.byref(dfdot)) < 0:
        raise InputError("foldfit_steps: bad header, nrows, nbin or f0_fold")
    return ddm.value, dfreq.value, dfdot.value


def foldfit_params(hdr: dict, nrows: int, nbin: int, nsub: int, f0_fold: float, subint_s: float, dm0: float, *, products=None, ndm=1,
                   nfreq=1, nfdot=1, ddm=None, dfreq=None, dfdot=None, fit_frac=0.5, widths=None, lib=None) -> _lib.FrbchFoldfitParams:
    """the search's parameters; a step left at None is the natural one (``foldfit_steps``), ``products`` the mask of the products
    that are added (None: ``hdr['product']``, or product 0), ``widths`` the boxcar widths of the S/N (None: the powers of two up
    to 32 that fit into half a turn)"""
    p = _lib.FrbchFoldfitParams()
    p.size = C.sizeof(_lib.FrbchFoldfitParams)
    p.nbin, p.nsub, p.ndm, p.nfreq, p.nfdot = int(nbin), int(nsub), int(ndm), int(nfreq), int(nfdot)
    p.products = int(products) if products is not None else 1 << int(hdr.get("product", 0))
    p.f0_fold, p.subint_s, p.dm0, p.fit_frac = float(f0_fold), float(subint_s), float(dm0), float(fit_frac)
    if ddm is None or dfreq is None or dfdot is None:
        nat = foldfit_steps(hdr, nrows, nbin, f0_fold, lib=lib)
        ddm, dfreq, dfdot = (nat[0] if ddm is None else ddm), (nat[1] if dfreq is None else dfreq), (nat[2] if dfdot is None else dfdot)
    p.ddm, p.dfreq, p.dfdot = float(ddm), float(dfreq), float(dfdot)
    ws = [int(w) for w in (widths if widths is not None else [w for w in FOLDFIT_WIDTHS if w <= max(1, nbin // 2)])]
    if not 1 <= len(ws) <= 8:
        raise InputError("foldfit: 1..8 boxcar widths")
    p.nwidth = len(ws)
    for i, w in enumerate(ws):
        p.widths[i] = w
    return p


def _foldfit_outputs(par, nchan, nifs, want_trials, want_plane, want_cube):
    nt = (par.ndm, par.nfdot, par.nfreq)
    out = dict(score=np.zeros(nt, np.float64), prof_acc=np.zeros((2, par.nbin), np.int64), prof_hits=np.zeros((2, par.nbin), np.uint64),
               results=np.zeros(1, FOLDFIT_RESULT))
    if want_trials:
        out.update(trial_acc=np.zeros(nt + (par.nbin,), np.int64), trial_hits=np.zeros(nt + (par.nbin,), np.uint64))
    if want_plane:
        out.update(plane_acc=np.zeros((par.nsub, par.nbin), np.int64), plane_hits=np.zeros((par.nsub, par.nbin), np.uint64))
    if want_cube:
        out.update(cube=np.zeros((par.nsub, nifs, par.nbin, nchan), np.float64), cube_hits=np.zeros((par.nsub, par.nbin, nchan), np.uint32))
    return out


def _ptr(out, key):
    return out[key].ctypes.data if key in out else None


def foldfit_axes(par) -> dict:
    """the trial values of a search: dm [ndm], dfreq [nfreq], dfdot [nfdot]"""
    ax = lambda n, step: (np.arange(n, dtype=np.int64) - n // 2).astype(np.float64) * np.float64(step)    # noqa: E731
    return dict(dm=np.float64(par.dm0) + ax(par.ndm, par.ddm), dfreq=ax(par.nfreq, par.dfreq), dfdot=ax(par.nfdot, par.dfdot))


def fold_fit(cube, hits, hdr: dict, nrows: int, par, flag=None, want_trials=False, want_plane=True, device: int = 0, lib=None,
             info: dict | None = None) -> dict:
    """Search the folded cube over DM, spin frequency and frequency derivative (frbch_foldfit_host).  ``cube`` float64
    [nsub][nifs][nbin][nchan] and ``hits`` uint32 [nsub][nbin][nchan] in the library's layout, as frbch_foldp_* leave them for a
    fold WITHOUT per-channel delays; ``par`` from ``foldfit_params``.  -> dict(score [ndm][nfdot][nfreq], prof_acc / prof_hits
    [2][nbin] (the nominal and the best trial), results FOLDFIT_RESULT [1], plane_acc / plane_hits [nsub][nbin] of the central DM,
    trial_acc / trial_hits when asked for).  ``info['kernel_used']``: (stage 1, stage 2), 1 = the fast kernel."""
    lib = lib or _lib.load()
    cube = np.ascontiguousarray(cube, dtype=np.float64)
    hits = np.ascontiguousarray(hits, dtype=np.uint32)
    nchan, nifs = hdr["nchans"], hdr.get("nifs", 1)
    if cube.shape != (par.nsub, nifs, par.nbin, nchan) or hits.shape != (par.nsub, par.nbin, nchan):
        raise InputError("fold_fit: the cube must be [nsub][nifs][nbin][nchan] and the hits [nsub][nbin][nchan]")
    fl = _flag_arg(flag, nchan)
    out = _foldfit_outputs(par, nchan, nifs, want_trials, want_plane, False)
    k = (C.c_uint32 * 2)(0, 0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_foldfit_host(C.byref(fil_desc(hdr, hdr.get("product", 0))), int(nrows), C.byref(par), cube.ctypes.data, hits.ctypes.data,
                                  fl.ctypes.data if fl is not None else None, device, out["score"].ctypes.data, out["prof_acc"].ctypes.data,
                                  out["prof_hits"].ctypes.data, out["results"].ctypes.data, _ptr(out, "trial_acc"), _ptr(out, "trial_hits"),
                                  _ptr(out, "plane_acc"), _ptr(out, "plane_hits"), k, err, len(err)), err)
    if info is not None:
        info.update(kernel_used=(k[0], k[1]))
    return out


def fold_refine(fil_or_rows, hdr: dict, model, par, flag=None, want_cube=False, want_plane=True, device: int = 0, lib=None,
                info: dict | None = None) -> dict:
    """Fold and search in one residency (frbch_fold_refine_host): the rows go up once, the cube stays on the device unless
    ``want_cube``.  ``model`` from ``fold_model`` with ``apply_delays=False`` and the ``nbin`` / ``subint_s`` of ``par``.
    -> the dict of ``fold_fit`` (and cube, cube_hits).  ``info['kernel_used']``: (fold, stage 1, stage 2)."""
    lib = lib or _lib.load()
    rows = _rows_of(fil_or_rows) if isinstance(fil_or_rows, sigproc.SigprocFile) else np.ascontiguousarray(fil_or_rows)
    nchan, nifs = hdr["nchans"], hdr.get("nifs", 1)
    fl = _flag_arg(flag, nchan)
    out = _foldfit_outputs(par, nchan, nifs, False, want_plane, want_cube)
    k = (C.c_uint32 * 3)(0, 0, 0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_fold_refine_host(C.byref(fil_desc(hdr, hdr.get("product", 0))), rows.ctypes.data, rows.shape[0], C.byref(model), C.byref(par),
                                      fl.ctypes.data if fl is not None else None, device, _ptr(out, "cube"), _ptr(out, "cube_hits"),
                                      out["score"].ctypes.data, out["prof_acc"].ctypes.data, out["prof_hits"].ctypes.data,
                                      out["results"].ctypes.data, _ptr(out, "plane_acc"), _ptr(out, "plane_hits"), k, err, len(err)), err)
    if info is not None:
        info.update(kernel_used=(k[0], k[1], k[2]))
    return out


def _mean_of(acc, hits):
    return np.where(hits > 0, acc / np.maximum(hits, 1).astype(np.float64), 0.0)


def foldfit_planes(cube, hits, hdr: dict, nrows: int, par, r, flag=None):
    """The two planes of the plot from the cube in the library's layout, in numpy, at the PEAK trial of the record ``r``:
    phase against time at its DM (sums int64 and hits uint64 [nsub][nbin], what the library's plane_acc / plane_hits are at the
    central DM) and phase against frequency at its spin and DM (mean sample [nchan][nbin]; flagged channels 0)."""
    nsub, nifs, nbin, nchan = cube.shape
    ax = foldfit_axes(par)
    use = np.ones(nchan, bool) if flag is None else ~np.asarray(flag, bool)
    val = sum(cube[:, q] for q in range(nifs) if (par.products >> q) & 1).astype(np.int64)      # [nsub][nbin][nchan]
    fc = hdr["fch1"] + np.arange(nchan) * hdr["foff"]
    delay = ax["dm"][r["kpeak"]] / 2.41e-4 * (1.0 / (fc * fc) - 1.0 / (fc.max() * fc.max()))
    shd = np.rint((delay * par.f0_fold) * nbin).astype(np.int64) % nbin
    L = max(1, int(np.floor(par.subint_s / hdr["tsamp"] + 0.5)))
    first = np.arange(nsub, dtype=np.int64) * L
    tau = ((first + 0.5 * np.minimum(L, nrows - first)) - 0.5 * nrows) * hdr["tsamp"]
    df, hd = ax["dfreq"][r["ipeak"]], 0.5 * ax["dfdot"][r["jpeak"]]
    shp = np.rint((df * tau + (hd * tau) * tau) * nbin).astype(np.int64) % nbin
    pt_acc, pt_hits = np.zeros((nsub, nbin), np.int64), np.zeros((nsub, nbin), np.uint64)
    pf_acc, pf_hits = np.zeros((nchan, nbin), np.int64), np.zeros((nchan, nbin), np.uint64)
    for c in np.flatnonzero(use):
        v, h = np.roll(val[:, :, c], -int(shd[c]), axis=1), np.roll(hits[:, :, c], -int(shd[c]), axis=1).astype(np.uint64)
        pt_acc += v
        pt_hits += h
        for s in range(nsub):
            pf_acc[c] += np.roll(v[s], int(shp[s]))
            pf_hits[c] += np.roll(h[s], int(shp[s]))
    return pt_acc, pt_hits, _mean_of(pf_acc, pf_hits)


def foldfit_fil(filterbankfile: str, parfile: str | None = None, f0: float | None = None, dm: float | None = None, f1: float = 0.0,
                nbin: int = 0, subint_s: float = 10.0, ndm: int = 33, nfreq: int = 33, nfdot: int = 17, ddm=None, dfreq=None, dfdot=None,
                fit_frac: float = 0.5, flag_file: str | None = None, polyco: str | None = None, refold: bool = False,
                products: str = "coherency", device: int = 0, lib=None, out_base: str | None = None, fil=None, par: dict | None = None):
    """`post foldfit`: fold a filterbank with an ephemeris (a .par file, or F0 / F1 / DM) and refine it on the device.

    Writes ``<base>_foldfit.npz`` (score, the axes, both profiles, the phase-time plane of the nominal and of the best DM, the
    phase-frequency plane of the best trial, results), ``<base>_foldfit.txt`` (the best F0 / F1 / DM with their resolutions, the
    S/N of the nominal and of the best profile, the kernels used), ``<base>_foldfit.png`` (top to bottom: phase against time at
    the best DM, phase against frequency at the best spin and DM, the nominal and the best profile, and the three score cuts
    through the peak: DM, F1, F0) and ``<base>_foldfit.par`` with the polynomial model: PEPOCH = mid-observation, F0' = F0 + F1 (t_mid - PEPOCH) + df,
    F1' = F1 + dfd, DM' (under a polyco only the offsets are reported: the predictor stays the timing model).  ``refold``: fold
    once more with that .par -- integer bin shifts cannot undo the smear inside a sub-integration, a second fold can -- and
    write its outputs as ``fold_fil`` does under ``<base>_refold``.  -> (files, results record)"""
    lib = lib or _lib.load()
    fil = fil or sigproc.read_fil(filterbankfile)
    hdr = fil.header
    if par is None:
        if parfile is not None:
            par = read_par(parfile)
        elif f0 is not None and dm is not None:
            par = {"F0": float(f0), "F1": float(f1), "DM": float(dm), "PEPOCH": None, "PSR": "unknown"}
        else:
            raise InputError("foldfit: a .par file, or --f0 and --dm")
    rows = _rows_of(fil)
    nrows, nifs = rows.shape[0], hdr.get("nifs", 1)
    segs = read_polyco(polyco) if polyco is not None else None
    f0_fold = par.get("F0") or (segs[0]["f0"] if segs else 0.0)
    nbin = nbin or default_nbin(f0_fold, hdr["tsamp"])
    model, _keep = fold_model(par, hdr, polyco=segs, nbin=nbin, subint_s=subint_s, apply_delays=False)
    nsub = lib.frbch_fold_nsub(C.byref(fil_desc(hdr)), nrows, float(subint_s))
    if nsub <= 0:
        raise InputError("bad sub-integration length")
    mask = 3 if (nifs == 4 and products == "coherency") else 1 << int(hdr.get("product", 0))
    fpar = foldfit_params(hdr, nrows, nbin, nsub, f0_fold, subint_s, par["DM"], products=mask, ndm=ndm, nfreq=nfreq, nfdot=nfdot, ddm=ddm,
                          dfreq=dfreq, dfdot=dfdot, fit_frac=fit_frac, lib=lib)
    flag = read_flag_file(flag_file, hdr["nchans"]) if flag_file else None
    info = {}
    out = fold_refine(rows, hdr, model, fpar, flag=flag, want_cube=True, device=device, lib=lib, info=info)     # (the cube: for the two planes of the plot)
    r = out["results"][0]
    ax = foldfit_axes(fpar)
    pt_acc, pt_hits, pf_mean = foldfit_planes(out["cube"], out["cube_hits"], hdr, nrows, fpar, r, flag=flag)
    base = (out_base or filterbankfile) + "_foldfit"
    span = nrows * hdr["tsamp"]
    t_mid = hdr["tstart"] + 0.5 * span / 86400.0
    pepoch = par["PEPOCH"] if par.get("PEPOCH") is not None else hdr["tstart"]
    f0_new = par["F0"] + par["F1"] * (t_mid - pepoch) * 86400.0 + r["dfreq"] if not segs else None
    f1_new = par["F1"] + r["dfdot"] if not segs else None
    np.savez(base + ".npz", score=out["score"], dm=ax["dm"], dfreq=ax["dfreq"], dfdot=ax["dfdot"], prof_acc=out["prof_acc"],
             prof_hits=out["prof_hits"], plane_acc=out["plane_acc"], plane_hits=out["plane_hits"], best_plane_acc=pt_acc,
             best_plane_hits=pt_hits, phase_freq=pf_mean, results=out["results"],
             kernel_used=np.array(info["kernel_used"], np.uint32), f0_fold=f0_fold, t_mid=t_mid)
    with open(base + ".txt", "w") as f:
        f.write("# %s: fold refinement, %d x %d x %d trials (DM x F1 x F0), nbin %d, %d sub-integrations of %g s\n"
                % (par["PSR"], fpar.ndm, fpar.nfdot, fpar.nfreq, nbin, nsub, subint_s))
        f.write("# resolutions, not error bars: how far the grid tells two values apart\n")
        if segs:
            f.write("polyco %s: offsets from the predictor\n" % os.path.basename(polyco))
        else:
            f.write("F0  %.12f Hz   (nominal at mid-observation %.12f)\n" % (f0_new, f0_new - r["dfreq"]))
            f.write("F1  %.6e Hz/s   (nominal %.6e)\n" % (f1_new, par["F1"]))
        f.write("dF0 %+.6e +- %.2e Hz%s\n" % (r["dfreq"], r["dfreq_res"], "" if r["fitted_freq"] else "   (grid value)"))
        f.write("dF1 %+.6e +- %.2e Hz/s%s\n" % (r["dfdot"], r["dfdot_res"], "" if r["fitted_fdot"] else "   (grid value)"))
        f.write("DM  %.6f +- %.6f pc cm-3   (nominal %.6f)%s\n" % (r["dm"], r["dm_res"], par["DM"], "" if r["fitted_dm"] else "   (grid value)"))
        f.write("S/N %.2f -> %.2f   (boxcar %d -> %d bins; score %.6g -> %.6g)\n"
                % (r["snr_nominal"], r["snr_best"], r["width_nominal"], r["width_best"], r["score_nominal"], r["score_peak"]))
        f.write("kernels: fold %d, DM stage %d, spin stage %d   (1 = fast, 0 = generic)\n" % tuple(info["kernel_used"]))
    files = [base + ".npz", base + ".txt", base + ".png"]
    plane = _mean_of(pt_acc, pt_hits)
    plane = _unit(plane - plane.mean(axis=1, keepdims=True))
    nf = max(1, pf_mean.shape[0] // max(1, min(128, pf_mean.shape[0])))
    pf = pf_mean[: pf_mean.shape[0] // nf * nf].reshape(-1, nf, nbin).mean(axis=1)
    pf = _unit(pf - pf.mean(axis=1, keepdims=True))
    strips = [np.tile(_unit(_mean_of(out["prof_acc"][t], out["prof_hits"][t])), (8, 1)) for t in (0, 1)]
    cuts = []
    for v in (out["score"][:, r["jpeak"], r["ipeak"]], out["score"][r["kpeak"], :, r["ipeak"]], out["score"][r["kpeak"], r["jpeak"], :]):
        cut = np.zeros((16, nbin))
        y = _unit(np.interp(np.linspace(0, v.size - 1, nbin), np.arange(v.size), v))
        cut[15 - np.rint(y * 15).astype(int), np.arange(nbin)] = 1.0
        cuts.append(cut)
    gap = np.zeros((2, nbin))
    write_png(files[2], np.concatenate([plane, gap, pf, gap, strips[0], gap, strips[1], gap, cuts[0], gap, cuts[1], gap, cuts[2]], axis=0))
    if not segs:
        files.append(base + ".par")
        with open(files[-1], "w") as f:
            f.write("PSR %s\nF0 %.15g\nF1 %.15g\nPEPOCH %.15f\nDM %.9f\n" % (par["PSR"], f0_new, f1_new, t_mid, r["dm"]))
        if refold:
            ar, _prof = _fold_par(fil, filterbankfile, read_par(files[-1]), nbin, subint_s, 128, device, lib, (out_base or filterbankfile) + "_refold",
                                  None, 0.0, products)
            files.append(ar)
    return files, r


# ------------------------------------------------------------------------------------------------------------------
# burst polarisation: spectra of every product, RM synthesis (frbch_burstspec_*, frbch_rmsynth_*, frbch_burst_rm_*)
# ------------------------------------------------------------------------------------------------------------------
BURST_CAND = np.dtype([("dm", "<f8"), ("sample", "<i8"), ("width", "<u4"), ("off_gap", "<u4"), ("off_len", "<u4"), ("reserved", "<u4")])
BURST_SUMS = np.dtype([("on_sum", "<f8"), ("off_sum", "<f8"), ("off_sumsq", "<f8"), ("on_hits", "<u4"), ("off_hits", "<u4")])
RM_RESULT = np.dtype([("rm", "<f8"), ("rm_err", "<f8"), ("peak", "<f8"), ("pa0", "<f8"), ("snr", "<f8"), ("sigma_f", "<f8"),
                      ("fwhm", "<f8"), ("kpeak", "<u4"), ("nused", "<u4"), ("fitted", "<u4"), ("reserved", "<u4")])
RM_C = 299.792458             # c in m MHz: lambda = RM_C / f_MHz
RM_NPHI_CAP = 1 << 17         # trials of the default grid
RM_ROW = "%s  DM %.3f  sample %d  RM %+.3f +- %.3f rad/m2  L/I %.4f  V/I %+.4f  PA0 %.2f deg  S/N %.1f"


def burst_cands(bursts, off_gap=None, off_len=None) -> np.ndarray:
    """BURST_CAND records from (dm, sample, width[, off_gap, off_len]) tuples, dicts or records; the defaults keep the
    off-pulse windows two widths (at least 16 rows) clear of the burst and make each 1024 rows long"""
    bursts = np.asarray(bursts) if isinstance(bursts, np.ndarray) else bursts
    if isinstance(bursts, np.ndarray) and bursts.dtype == BURST_CAND:
        return np.ascontiguousarray(bursts)
    out = np.zeros(len(bursts), dtype=BURST_CAND)
    for i, b in enumerate(bursts):
        if isinstance(b, dict) or (hasattr(b, "dtype") and b.dtype.names):
            dm, sample, width = float(b["dm"]), int(b["sample"]), int(b["width"])
            names = b.keys() if isinstance(b, dict) else b.dtype.names
            gap = int(b["off_gap"]) if "off_gap" in names else None
            length = int(b["off_len"]) if "off_len" in names else None
        else:
            dm, sample, width = float(b[0]), int(b[1]), int(b[2])
            gap = int(b[3]) if len(b) > 3 else None
            length = int(b[4]) if len(b) > 4 else None
        gap = gap if gap is not None else (off_gap if off_gap is not None else max(16, 2 * width))
        length = length if length is not None else (off_len if off_len is not None else 1024)
        out[i] = (dm, sample, width, gap, length, 0)
    return out


def _burst_args(fil_or_rows, hdr, cands, gains, products):
    rows = _rows_of(fil_or_rows) if isinstance(fil_or_rows, sigproc.SigprocFile) else np.ascontiguousarray(fil_or_rows)
    nifs, nchan = hdr.get("nifs", 1), hdr["nchans"]
    if rows.dtype.itemsize * 8 != hdr["nbits"] or rows.size % (nchan * nifs):
        raise InputError("the rows do not match the header's nbits / nchans / nifs")
    cands = burst_cands(cands)
    if products not in ("stokes", "coherency"):
        raise InputError("products must be 'stokes' or 'coherency'")
    par = _lib.FrbchBurstParams(C.sizeof(_lib.FrbchBurstParams), _lib.BURST_COHERENCY if products == "coherency" else _lib.BURST_STOKES)
    g = None
    if gains is not None:
        g = np.ascontiguousarray(gains, dtype=np.float32)
        if g.shape != (nifs, nchan):
            raise InputError("gains must have the shape [nifs][nchans]")
    return rows, rows.size // (nchan * nifs), cands, par, g


def burst_spectra(fil_or_rows, hdr: dict, cands, gains=None, products: str = "stokes", device: int = 0, lib=None,
                  info: dict | None = None):
    """On-pulse minus off-pulse spectra of every product for every burst (frbch_burstspec_host; include/frbch.h states the
    arithmetic) -> ``spec [n][nifs][nchans]`` float32, ``noise`` (the off-pulse scatter scaled to the on-pulse mean), ``used
    [n][nchans]`` bytes.  ``cands``: BURST_CAND records or what ``burst_cands`` takes.  ``gains [nifs][nchans]`` multiply the
    spectra.  ``products='coherency'``: the file holds PP, QQ, Re, Im and the spectra come back as I, Q, U, V.
    ``info['kernel_used']``: 1 = the fast kernel, 0 = the generic one; ``info['sums']``: the BURST_SUMS records."""
    lib = lib or _lib.load()
    rows, nrows, cands, par, g = _burst_args(fil_or_rows, hdr, cands, gains, products)
    n, nifs, nchan = cands.size, hdr.get("nifs", 1), hdr["nchans"]
    sums = np.zeros((n, nifs, nchan), dtype=BURST_SUMS)
    spec, noise = np.zeros((n, nifs, nchan), np.float32), np.zeros((n, nifs, nchan), np.float32)
    used = np.zeros((n, nchan), np.uint8)
    k = C.c_uint32(0)
    err = C.create_string_buffer(512)
    desc = fil_desc(hdr, hdr.get("product", 0))
    _check(lib.frbch_burstspec_host(C.byref(desc), rows.ctypes.data, nrows, C.byref(par), cands.ctypes.data, n,
                                    g.ctypes.data if g is not None else None, device, sums.ctypes.data, spec.ctypes.data,
                                    noise.ctypes.data, used.ctypes.data, C.byref(k), err, len(err)), err)
    if info is not None:
        info.update(kernel_used=k.value, sums=sums)
    return spec, noise, used


def _flag_arg(flag, nchan: int):
    """``flag`` of the burst analyses as the library's uint8 [nchan] mask, or None"""
    if flag is None:
        return None
    fl = np.ascontiguousarray(flag, dtype=np.uint8)
    if fl.shape != (nchan,):
        raise InputError("flag must have the shape [nchans]")
    return fl


def rm_params(nphi: int, phi_lo: float, dphi: float) -> _lib.FrbchRmParams:
    return _lib.FrbchRmParams(C.sizeof(_lib.FrbchRmParams), int(nphi), float(phi_lo), float(dphi))


def lambda2(hdr: dict) -> np.ndarray:
    """lambda^2 of every channel, m^2, as the library computes it"""
    f = hdr["fch1"] + np.arange(hdr["nchans"], dtype=np.float64) * hdr["foff"]
    t = RM_C / f
    return t * t


def rm_grid(hdr: dict, used=None, phi_max: float = 0.0, dphi: float = 0.0, nphi: int = 0):
    """The default grid of Faraday depths -> (nphi, phi_lo, dphi): dphi = fwhm / 8 with fwhm = 2 sqrt(3) / (span of lambda^2
    over the used channels); phi_max = sqrt(3) / (the largest lambda^2 step between adjacent channels), lowered until
    nphi = 2 round(phi_max / dphi) + 1 <= 2^17.  The grid is symmetric about 0, which is one of its trials."""
    l2 = lambda2(hdr)
    sel = l2 if used is None else l2[np.asarray(used).reshape(-1, hdr["nchans"]).any(axis=0)]
    if sel.size < 2:
        raise InputError("RM synthesis needs at least two used channels")
    if dphi <= 0.0:
        dphi = 2.0 * np.sqrt(3.0) / float(sel.max() - sel.min()) / 8.0
    if nphi > 0:
        half = (int(nphi) - 1) // 2
    else:
        if phi_max <= 0.0:
            phi_max = np.sqrt(3.0) / float(np.abs(np.diff(l2)).max())
        half = min(int(round(phi_max / dphi)), (RM_NPHI_CAP - 1) // 2)
    half = max(half, 1)
    return 2 * half + 1, -half * dphi, float(dphi)


# ---- RM synthesis and the delay x RM transform share their calls: the second is the first with a tau axis in front of phi ----
def _qu_args(q, u, used, nchan: int):
    """``q``, ``u``, ``used`` of a transform as contiguous float32, float32, uint8 [n][nchans]"""
    q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, nchan)
    u = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, nchan)
    used = np.ascontiguousarray(used, dtype=np.uint8).reshape(-1, nchan)
    if not q.shape == u.shape == used.shape:
        raise InputError("q, u and used must have the same shape [n][nchans]")
    return q, u, used


def _rmd_plane(n: int, ntau: int, nphi: int):
    """(ntau, nphi) of an F the delay x RM transform can return for ``n`` candidates, clamped to what the library takes (it
    refuses the rest by name)"""
    nt, nk = max(1, min(int(ntau), 4096)), max(1, min(int(nphi), 1 << 20))
    if n * nt * nk > 1 << 26:
        raise InputError("ncand * ntau * nphi exceeds 2^26: cut the batch or the grid")
    return nt, nk


def _transform_call(entry, q, u, used, hdr, par, plane, device, info):
    """frbch_rmsynth_host / frbch_rmdelay_host -> complex64 F [n] + plane"""
    F = np.zeros((q.shape[0],) + plane + (2,), np.float32)
    k = (C.c_uint32 * 2)(0, 1)
    err = C.create_string_buffer(512)
    _check(entry(C.byref(fil_desc(hdr)), q.ctypes.data, u.ctypes.data, used.ctypes.data, q.shape[0], C.byref(par), device, F.ctypes.data, k,
                 err, len(err)), err)
    if info is not None:
        info.update(kernel_used=k[0], split=k[1])
    return F.view(np.complex64)[..., 0]


def _peaks_call(entry, F, plane, used, noise_q, noise_u, hdr, par, dtype, extra):
    """frbch_rm_peaks / frbch_rmdelay_peaks -> records [n + extra]"""
    nchan = hdr["nchans"]
    Ff = np.ascontiguousarray(np.asarray(F, dtype=np.complex64).reshape((-1,) + plane)).view(np.float32)
    used = np.ascontiguousarray(used, dtype=np.uint8).reshape(-1, nchan)
    nq = None if noise_q is None else np.ascontiguousarray(noise_q, dtype=np.float32).reshape(-1, nchan)
    nu = None if noise_u is None else np.ascontiguousarray(noise_u, dtype=np.float32).reshape(-1, nchan)
    res = np.zeros(used.shape[0] + extra, dtype=dtype)
    err = C.create_string_buffer(512)
    _check(entry(C.byref(fil_desc(hdr)), Ff.ctypes.data, used.ctypes.data, nq.ctypes.data if nq is not None else None,
                 nu.ctypes.data if nu is not None else None, used.shape[0], C.byref(par), res.ctypes.data, err, len(err)), err)
    return res


def _composite_call(entry, fil_or_rows, hdr, cands, gains, flag, products, plane_of, make_par, grid, dtype, extra, device, info):
    """frbch_burst_rm_host / frbch_burst_polcal_host -> dict(spec, noise, used, F [n] + plane_of(n), results [n + extra])"""
    rows, nrows, cands, par, g = _burst_args(fil_or_rows, hdr, cands, gains, products)
    n, nchan = cands.size, hdr["nchans"]
    plane = plane_of(n)
    spec, noise = np.zeros((n, 4, nchan), np.float32), np.zeros((n, 4, nchan), np.float32)
    used = np.zeros((n, nchan), np.uint8)
    F = np.zeros((n,) + plane + (2,), np.float32)
    res = np.zeros(n + extra, dtype=dtype)
    fl = _flag_arg(flag, nchan)
    rpar = make_par(*grid)
    k = (C.c_uint32 * 3)(0, 0, 1)
    err = C.create_string_buffer(512)
    _check(entry(C.byref(fil_desc(hdr, hdr.get("product", 0))), rows.ctypes.data, nrows, C.byref(par), cands.ctypes.data, n,
                 g.ctypes.data if g is not None else None, fl.ctypes.data if fl is not None else None, C.byref(rpar), device,
                 spec.ctypes.data, noise.ctypes.data, used.ctypes.data, F.ctypes.data, res.ctypes.data, k, err, len(err)), err)
    if info is not None:
        info.update(spectra_kernel_used=k[0], kernel_used=k[1], split=k[2])
    return dict(spec=spec, noise=noise, used=used, F=F.view(np.complex64)[..., 0], results=res)


def rm_synthesis(q, u, used, hdr: dict, nphi: int, phi_lo: float, dphi: float, device: int = 0, lib=None, info: dict | None = None):
    """F(phi) of ``q``, ``u`` [n][nchans] over the channels with ``used != 0`` at phi_k = phi_lo + k dphi (frbch_rmsynth_host;
    include/frbch.h states the integer transform) -> complex64 ``F [n][nphi]``.  The RMSF is ``rm_synthesis(used, 0, used,
    ...)``.  ``info['kernel_used']``: 1 = the fast kernel, 0 = the generic one; ``info['split']``: the channel split."""
    lib = lib or _lib.load()
    q, u, used = _qu_args(q, u, used, hdr["nchans"])
    return _transform_call(lib.frbch_rmsynth_host, q, u, used, hdr, rm_params(nphi, phi_lo, dphi), (int(nphi),), device, info)


def rm_peaks(F, used, noise_q, noise_u, hdr: dict, nphi: int, phi_lo: float, dphi: float, lib=None) -> np.ndarray:
    """RM_RESULT records from F (frbch_rm_peaks: the first largest trial, a three-point parabola, PA0, the noise in F)"""
    lib = lib or _lib.load()
    return _peaks_call(lib.frbch_rm_peaks, F, (int(nphi),), used, noise_q, noise_u, hdr, rm_params(nphi, phi_lo, dphi), RM_RESULT, 0)


def burst_rm(fil_or_rows, hdr: dict, cands, nphi: int, phi_lo: float, dphi: float, gains=None, flag=None, products: str = "stokes",
             device: int = 0, lib=None, info: dict | None = None):
    """Rows -> spectra -> RM synthesis of Q and U -> peaks in one library call on rows uploaded once (frbch_burst_rm_host)
    -> dict(spec, noise, used, F, results).  ``flag [nchans]``: non-zero clears the channel in ``used``."""
    lib = lib or _lib.load()
    return _composite_call(lib.frbch_burst_rm_host, fil_or_rows, hdr, cands, gains, flag, products, lambda n: (int(nphi),), rm_params,
                           (nphi, phi_lo, dphi), RM_RESULT, 0, device, info)


# ---- polarisation calibration: the delay x RM transform (frbch_rmdelay_*, frbch_burst_polcal_*) ------------------
RMD_RESULT = np.dtype([("tau", "<f8"), ("tau_err", "<f8"), ("rm", "<f8"), ("rm_err", "<f8"), ("peak", "<f8"), ("psi", "<f8"),
                       ("snr", "<f8"), ("sigma_f", "<f8"), ("fwhm", "<f8"), ("fwhm_tau", "<f8"), ("ridge_slope", "<f8"),
                       ("mpeak", "<u4"), ("kpeak", "<u4"), ("nused", "<u4"), ("fitted_tau", "<u4"), ("fitted_rm", "<u4"),
                       ("nridge", "<u4")])
POLCAL_DTAU_ONE = 1.0e-3      # dtau of a one-trial tau axis (it must be positive; no trial uses it), microseconds
POLCAL_ROW = "%-9s tau %+9.4f +- %.4f ns  RM %+10.3f +- %.3f rad/m2  psi %+8.2f deg  ridge %+8.3f rad/m2/ns (%d rows)  S/N %.1f"


def rmd_params(nphi: int, phi_lo: float, dphi: float, ntau: int, tau_lo: float, dtau: float) -> _lib.FrbchRmdParams:
    """the grid of the delay x RM transform: phi in rad m^-2, tau in MICROSECONDS"""
    return _lib.FrbchRmdParams(C.sizeof(_lib.FrbchRmdParams), int(nphi), int(ntau), 0, float(phi_lo), float(dphi), float(tau_lo), float(dtau))


def rm_delay(q, u, used, hdr: dict, nphi: int, phi_lo: float, dphi: float, ntau: int, tau_lo: float, dtau: float, device: int = 0,
             lib=None, info: dict | None = None):
    """F(tau, phi) of ``q``, ``u`` [n][nchans]: RM synthesis at ``ntau`` trial delays tau_m = tau_lo + m dtau (microseconds)
    between the two circular feeds, each taken out as a phase ramp across the band before the transform (frbch_rmdelay_host;
    include/frbch.h states the arithmetic) -> complex64 ``F [n][ntau][nphi]``.  ``ntau = 1, tau_lo = 0`` is ``rm_synthesis``
    to the bit.  ``info['kernel_used']``: 1 = the fast kernel, 0 = the generic one; ``info['split']``: the channel split."""
    lib = lib or _lib.load()
    q, u, used = _qu_args(q, u, used, hdr["nchans"])
    par = rmd_params(nphi, phi_lo, dphi, ntau, tau_lo, dtau)
    return _transform_call(lib.frbch_rmdelay_host, q, u, used, hdr, par, _rmd_plane(q.shape[0], ntau, nphi), device, info)


def rm_delay_peaks(F, used, noise_q, noise_u, hdr: dict, nphi: int, phi_lo: float, dphi: float, ntau: int, tau_lo: float, dtau: float,
                   lib=None) -> np.ndarray:
    """RMD_RESULT records [n + 1] from F [n][ntau][nphi] (frbch_rmdelay_peaks): per pulse the first largest trial of the plane,
    a parabola along each axis, psi, the noise and the slope of the ridge; the last record is the combined estimate of all
    pulses (their planes added with weights 1 / sigma_f^2)"""
    lib = lib or _lib.load()
    return _peaks_call(lib.frbch_rmdelay_peaks, F, (int(ntau), int(nphi)), used, noise_q, noise_u, hdr,
                       rmd_params(nphi, phi_lo, dphi, ntau, tau_lo, dtau), RMD_RESULT, 1)


def polcal(fil_or_rows, hdr: dict, cands, nphi: int, phi_lo: float, dphi: float, ntau: int, tau_lo: float, dtau: float, gains=None,
           flag=None, products: str = "stokes", device: int = 0, lib=None, info: dict | None = None):
    """Rows -> spectra -> the delay x RM transform of Q and U -> peaks and the combined record, in one library call on rows
    uploaded once (frbch_burst_polcal_host) -> dict(spec, noise, used, F [n][ntau][nphi], results RMD_RESULT [n + 1])."""
    lib = lib or _lib.load()
    return _composite_call(lib.frbch_burst_polcal_host, fil_or_rows, hdr, cands, gains, flag, products, lambda n: _rmd_plane(n, ntau, nphi),
                           rmd_params, (nphi, phi_lo, dphi, ntau, tau_lo, dtau), RMD_RESULT, 1, device, info)


def polcal_tau(polcal_file) -> float:
    """the delay (microseconds) of a ``<base>_polcal.npz`` that ``polcal_fil`` wrote: the combined estimate of its pulses"""
    try:
        return float(np.load(polcal_file)["tau_us"])
    except (OSError, KeyError, ValueError) as ex:
        raise InputError("%s: not a _polcal.npz of `post polcal` (%s)" % (polcal_file, ex))


def tau_grid(hdr: dict, used=None, tau_half_ns: float = 0.0, dtau_ns: float = 0.0):
    """The default grid of delays -> (ntau, tau_lo, dtau) in microseconds: dtau = fwhm_tau / 8 with fwhm_tau = 2 sqrt(3) / (pi x
    the span of the used channels' frequencies), tau_half = 8 fwhm_tau either side of 0, which is one of its trials; at most
    4096 trials"""
    f = hdr["fch1"] + np.arange(hdr["nchans"], dtype=np.float64) * hdr["foff"]
    sel = f if used is None else f[np.asarray(used).reshape(-1, hdr["nchans"]).any(axis=0)]
    if sel.size < 2:
        raise InputError("the delay search needs at least two used channels")
    fwhm = 2.0 * np.sqrt(3.0) / (np.pi * float(sel.max() - sel.min()))
    dtau = dtau_ns * 1e-3 if dtau_ns > 0.0 else fwhm / 8.0
    half_us = tau_half_ns * 1e-3 if tau_half_ns > 0.0 else 8.0 * fwhm
    half = max(1, min(int(round(half_us / dtau)), 2047))
    return 2 * half + 1, -half * dtau, float(dtau)


def _polcal_png(path, P, results_i):
    """|F|^2 of the (tau, RM) plane, tau bottom to top against the RM trials about the peak, with the ridge's trials marked"""
    width, height = 512, 192
    nt, nk = P.shape
    span = max(8, min(nk, 4 * nt))
    k0 = min(max(0, int(results_i["kpeak"]) - span // 2), max(0, nk - span))
    win = P[:, k0:k0 + span]
    rows = np.clip((np.arange(height) * nt) // height, 0, nt - 1)[::-1]
    cols = np.clip((np.arange(width) * win.shape[1]) // width, 0, win.shape[1] - 1)
    img = win[rows][:, cols]
    img = img / max(1e-30, float(img.max()))
    ridge = np.argmax(win, axis=1)
    for y, m in enumerate(rows):
        if win[m, ridge[m]] >= 0.5 * float(win.max()):
            img[y, min(width - 1, int((ridge[m] + 0.5) * width / win.shape[1]))] = 1.0
    write_png(path, img)


def polcal_fil(filterbankfile, bursts=None, dm1=None, dm2=0.0, dmstep=1.0, width=0, off_gap=None, off_len=None, rm_known=None,
               rm_lo=None, rm_hi=None, rm_step=None, tau_half=0.0, dtau=0.0, flag_file=None, gains=None, products="stokes", threshold=8.0,
               max_cands=8, device=0, lib=None, info: dict | None = None):
    """The delay between the two circular feeds from the pulses of a calibrator of known RM in a full-Stokes filterbank.
    ``bursts`` or a DM range as ``rmsynth_fil`` takes them; ``rm_known`` (one RM trial) or ``rm_lo .. rm_hi`` in steps of
    ``rm_step`` (the ionosphere moves an RM by a few units); ``tau_half`` and ``dtau`` in NANOSECONDS (defaults: ``tau_grid``).
    Writes ``<base>_polcal.npz`` (spec, noise, used, phi, tau [microseconds], F, results [the pulses, then the combined
    record], bursts, tau_us = the combined delay, tau_ns, tau_err_ns, rm), ``<base>_polcal.txt`` (one line per pulse and one for
    the combined record: tau +- err in ns, RM, psi, the ridge slope in rad m^-2 per ns) and ``<base>_polcal.png`` (the summed
    plane with its ridge).  Returns (files, RMD_RESULT records)."""
    lib = lib or _lib.load()
    fil = sigproc.read_fil(filterbankfile)
    hdr = fil.header
    if hdr.get("nifs", 1) != 4:
        raise InputError("polcal needs a four-product file (pol_mode 4 or 5)")
    if rm_known is None and (rm_lo is None or rm_hi is None or rm_step is None):
        raise InputError("give --rm-known R, or --rm-lo A --rm-hi B --rm-step S")
    if rm_known is not None:
        n_phi, phi_lo, d_phi = 1, float(rm_known), 1.0
    else:
        if not (rm_step > 0.0 and rm_hi >= rm_lo):
            raise InputError("--rm-step must be positive and --rm-hi not below --rm-lo")
        n_phi, phi_lo, d_phi = int(np.floor((rm_hi - rm_lo) / rm_step + 1e-9)) + 1, float(rm_lo), float(rm_step)
    if not bursts:
        if dm1 is None:
            raise InputError("give bursts (--dm --sample/--time --width) or a DM range to search")
        dms = dm_list(dm1, dm2, dmstep)
        _files, recs = _search(fil, filterbankfile, dm1, dm2, dmstep, True, 5, threshold, 0.0, 1000, False, None, device, lib, {})
        groups = group_candidates(recs, hdr, dms, lib=lib)
        groups = groups[np.argsort(-groups["best"]["sigma"], kind="stable")[:max_cands]]
        bursts = [(dms[int(g["best"]["dm_index"])], int(g["best"]["sample"]), max(int(width), int(g["best"]["width"]))) for g in groups]
        if not bursts:
            raise InputError("the search found no burst above the threshold")
    cands = burst_cands(bursts, off_gap, off_len)
    flag = read_flag_file(flag_file, hdr["nchans"]).astype(np.uint8) if flag_file else None
    if isinstance(gains, str):
        gains = np.load(gains)
    keep = None if flag is None else (flag == 0)[None, :]
    n_tau, tau_lo, d_tau = tau_grid(hdr, keep, tau_half, dtau)
    rinfo = {}
    r = polcal(fil, hdr, cands, n_phi, phi_lo, d_phi, n_tau, tau_lo, d_tau, gains=gains, flag=flag, products=products, device=device,
               lib=lib, info=rinfo)
    res = r["results"]
    phi = phi_lo + np.arange(n_phi) * d_phi
    tau = tau_lo + np.arange(n_tau) * d_tau
    base = filterbankfile.replace(".fil", "")
    files = [base + "_polcal.npz", base + "_polcal.txt", base + "_polcal.png"]
    comb = res[-1]
    np.savez(files[0], spec=r["spec"], noise=r["noise"], used=r["used"], phi=phi, tau=tau, F=r["F"], results=res, bursts=cands,
             tau_us=np.float64(comb["tau"]), tau_ns=np.float64(comb["tau"] * 1e3), tau_err_ns=np.float64(comb["tau_err"] * 1e3),
             rm=np.float64(comb["rm"]))
    with open(files[1], "w") as f:
        for i, x in enumerate(res):
            name = "pulse%d" % i if i < cands.size else "combined"
            f.write(POLCAL_ROW % (name, x["tau"] * 1e3, x["tau_err"] * 1e3, x["rm"], x["rm_err"], np.degrees(x["psi"]), x["ridge_slope"] * 1e-3,
                                  x["nridge"], x["snr"]) + "\n")
    P = np.zeros((n_tau, n_phi))
    for i in range(cands.size):
        if res[i]["sigma_f"] > 0 and res[i]["nused"] > 0:
            P += np.abs(r["F"][i].astype(np.complex128)) ** 2 / float(res[i]["sigma_f"]) ** 2
    _polcal_png(files[2], P, comb)
    if info is not None:
        info.update(rinfo, nphi=n_phi, phi_lo=phi_lo, dphi=d_phi, ntau=n_tau, tau_lo=tau_lo, dtau=d_tau)
    return files, res


def pol_fractions(spec, noise, used, res):
    """-> (L/I debiased as sqrt(L^2 - sigma_L^2), V/I) of one burst, from the band-averaged spectra: L is the peak of |F|"""
    m = used != 0
    if not m.any():
        return 0.0, 0.0
    imean = float(spec[0][m].astype(np.float64).mean())
    vmean = float(spec[3][m].astype(np.float64).mean())
    lin2 = float(res["peak"]) ** 2 - float(res["sigma_f"]) ** 2
    lin = np.sqrt(lin2) if lin2 > 0 else 0.0
    return (lin / imean, vmean / imean) if imean != 0 else (0.0, 0.0)


def _curve_panel(curves, width, height):
    """curves (each resampled to `width` columns) drawn on one scale, the later ones brighter"""
    img = np.zeros((height, width))
    ok = [np.asarray(c, dtype=np.float64) for c in curves if len(c)]
    if not ok:
        return img
    lo, hi = min(float(c.min()) for c in ok), max(float(c.max()) for c in ok)
    for i, c in enumerate(ok):
        x = np.interp(np.linspace(0, c.size - 1, width), np.arange(c.size), c)
        y = (height - 1) - np.rint((x - lo) / max(1e-30, hi - lo) * (height - 1)).astype(int)
        img[y, np.arange(width)] = 0.5 + 0.5 * (i + 1) / len(ok)
    return img


def _rm_png(path, hdr, r, i, rmsf, phi):
    """|F| with the RMSF; Q/I and U/I against lambda^2 with the fitted rotation; the PA after de-rotation"""
    width, height = 512, 96
    m = r["used"][i] != 0
    l2 = lambda2(hdr)[m]
    order = np.argsort(l2)
    l2 = l2[order]
    res = r["results"][i]
    I = np.maximum(np.abs(r["spec"][i, 0][m][order].astype(np.float64)), 1e-30)
    qi, ui = r["spec"][i, 1][m][order] / I, r["spec"][i, 2][m][order] / I
    lin = float(res["peak"]) / max(1e-30, float(np.mean(I)))
    l0 = float(l2.mean()) if l2.size else 0.0
    ang = 2.0 * (float(res["pa0"]) + float(res["rm"]) * (l2 - l0))
    pa = 0.5 * np.arctan2(ui, qi) - float(res["rm"]) * (l2 - l0)
    pa = (pa + np.pi / 2) % np.pi - np.pi / 2
    shift = np.abs(rmsf) * float(res["peak"])
    panels = [_curve_panel([np.roll(shift, int(res["kpeak"]) - int(np.argmin(np.abs(phi)))), np.abs(r["F"][i])], width, height),
              _curve_panel([lin * np.cos(ang), qi], width, height), _curve_panel([lin * np.sin(ang), ui], width, height),
              _curve_panel([np.full(l2.size, -np.pi / 2), np.full(l2.size, np.pi / 2), pa], width, height)]
    gap = np.zeros((4, width))
    write_png(path, np.concatenate([panels[0], gap, panels[1], gap, panels[2], gap, panels[3]], axis=0))


def rmsynth_fil(filterbankfile, bursts=None, dm1=None, dm2=0.0, dmstep=1.0, width=0, off_gap=None, off_len=None, phi_max=0.0, dphi=0.0,
                nphi=0, flag_file=None, gains=None, products="stokes", threshold=8.0, max_cands=8, device=0, lib=None,
                info: dict | None = None, profile=False, nbin=256, tfactor=1, polcal_file=None):
    """Rotation measure of the bursts of a full-Stokes filterbank: ``bursts`` = (dm, sample, width) tuples; or, with ``dm1 ..
    dm2 .. dmstep`` and no bursts, the ``max_cands`` strongest groups ``candidates_fil``'s search finds on product 0 above
    ``threshold`` (the search writes its ``.singlepulse`` files, as ``search_fil`` does).  ``gains``: an .npy file or an array [4][nchans]; ``flag_file``: channels left out of the transform.  The
    grid: ``rm_grid``.  Writes ``<base>_rm.npz`` (spec, noise, used, phi, F, rmsf, results, bursts), ``<base>_rm.txt`` (one
    line per burst: RM +- err, L/I debiased, V/I, PA0) and ``<base>_rm_burst<i>.png``.  ``profile=True``: each burst's
    polarisation profile at its fitted RM as well (``nbin`` bins of ``tfactor`` rows), in the files of ``polprof_fil``.
    ``polcal_file``: the ``<base>_polcal.npz`` of a calibrator (``polcal_fil``); its delay between the two circular feeds is
    taken out of Q + iU before the transform (and of the profile), every file keeps its layout.  Returns (files, RM_RESULT
    records)."""
    lib = lib or _lib.load()
    fil = sigproc.read_fil(filterbankfile)
    hdr = fil.header
    if hdr.get("nifs", 1) != 4:
        raise InputError("rmsynth needs a four-product file (pol_mode 4 or 5)")
    if not bursts:
        if dm1 is None:
            raise InputError("give bursts (--dm --sample/--time --width) or a DM range to search")
        dms = dm_list(dm1, dm2, dmstep)
        _files, recs = _search(fil, filterbankfile, dm1, dm2, dmstep, True, 5, threshold, 0.0, 1000, False, None, device, lib, {})
        groups = group_candidates(recs, hdr, dms, lib=lib)
        groups = groups[np.argsort(-groups["best"]["sigma"], kind="stable")[:max_cands]]
        bursts = [(dms[int(g["best"]["dm_index"])], int(g["best"]["sample"]), max(int(width), int(g["best"]["width"]))) for g in groups]
        if not bursts:
            raise InputError("the search found no burst above the threshold")
    cands = burst_cands(bursts, off_gap, off_len)
    flag = read_flag_file(flag_file, hdr["nchans"]).astype(np.uint8) if flag_file else None
    if isinstance(gains, str):
        gains = np.load(gains)
    keep = None if flag is None else (flag == 0)[None, :]
    n_phi, phi_lo, d_phi = rm_grid(hdr, keep, phi_max=phi_max, dphi=dphi, nphi=nphi)
    rinfo = {}
    tau = polcal_tau(polcal_file) if polcal_file else None
    if tau is None:
        r = burst_rm(fil, hdr, cands, n_phi, phi_lo, d_phi, gains=gains, flag=flag, products=products, device=device, lib=lib, info=rinfo)
    else:
        r = polcal(fil, hdr, cands, n_phi, phi_lo, d_phi, 1, tau, POLCAL_DTAU_ONE, gains=gains, flag=flag, products=products,
                   device=device, lib=lib, info=rinfo)
        r["F"] = np.ascontiguousarray(r["F"][:, 0])
        r["results"] = rm_peaks(r["F"], r["used"], r["noise"][:, 1], r["noise"][:, 2], hdr, n_phi, phi_lo, d_phi, lib=lib)
    rmsf = rm_synthesis(r["used"], np.zeros_like(r["spec"][:, 0]), r["used"], hdr, n_phi, phi_lo, d_phi, device=device, lib=lib)
    phi = phi_lo + np.arange(n_phi) * d_phi
    base = filterbankfile.replace(".fil", "")
    files = [base + "_rm.npz", base + "_rm.txt"]
    np.savez(files[0], spec=r["spec"], noise=r["noise"], used=r["used"], phi=phi, F=r["F"], rmsf=rmsf, results=r["results"], bursts=cands)
    with open(files[1], "w") as f:
        for i, (c, res) in enumerate(zip(cands, r["results"])):
            li, vi = pol_fractions(r["spec"][i], r["noise"][i], r["used"][i], res)
            f.write(RM_ROW % ("burst%d" % i, c["dm"], int(c["sample"]), res["rm"], res["rm_err"], li, vi, np.degrees(res["pa0"]), res["snr"]) + "\n")
            _rm_png(base + "_rm_burst%d.png" % i, hdr, r, i, rmsf[i], phi)
            files.append(base + "_rm_burst%d.png" % i)
    if profile:
        prof = pol_profile(fil, hdr, cands, r["results"]["rm"], nbin=nbin, tfactor=tfactor, gains=gains, flag=flag, products=products,
                           device=device, lib=lib, tau=tau)
        files += _polprof_write(base, hdr, cands, r["results"]["rm"], prof, tfactor)
    if info is not None:
        info.update(rinfo, nphi=n_phi, phi_lo=phi_lo, dphi=d_phi)
    return files, r["results"]


# ------------------------------------------------------------------------------------------------------------------
# polarisation profile of a burst: derotated I, L, V and PA per time bin (frbch_polprof_*)
# ------------------------------------------------------------------------------------------------------------------
PROF_BIN = np.dtype([("i", "<f8"), ("q", "<f8"), ("u", "<f8"), ("v", "<f8"), ("l", "<f8"), ("l_db", "<f8"), ("pa", "<f8"),
                     ("pa_err", "<f8"), ("hits", "<u4"), ("pa_valid", "<u4")])
PROF_RESULT = np.dtype([("sigma_i", "<f8"), ("sigma_q", "<f8"), ("sigma_u", "<f8"), ("sigma_v", "<f8"), ("sigma_l", "<f8"),
                        ("lref", "<f8"), ("k", "<i4"), ("nused", "<u4"), ("on_lo_bin", "<u4"), ("on_hi_bin", "<u4")])
PROF_ROW = "%.9f %.6g %.6g %.6g %.4f %.4f"


def prof_params(nbin: int, tfactor: int, ref="mean") -> _lib.FrbchProfParams:
    if ref not in ("mean", "zero", _lib.PROF_REF_MEAN, _lib.PROF_REF_ZERO):
        raise InputError("ref must be 'mean' or 'zero'")
    code = {"mean": _lib.PROF_REF_MEAN, "zero": _lib.PROF_REF_ZERO}.get(ref, ref)
    return _lib.FrbchProfParams(C.sizeof(_lib.FrbchProfParams), int(nbin), int(tfactor), int(code), 0)


def pol_profile(fil_or_rows, hdr: dict, cands, rm, nbin: int = 256, tfactor: int = 1, ref="mean", gains=None, flag=None,
                products: str = "stokes", device: int = 0, lib=None, info: dict | None = None, tau=None):
    """The polarisation profile of every burst at its RM (frbch_polprof_host; include/frbch.h states the arithmetic): ``nbin``
    bins of ``tfactor`` rows about ``sample`` at the burst's DM, every channel's baseline removed, (Q, U) rotated back by
    ``rm[i]`` to ``ref`` ('mean': the mean lambda^2 of the used channels, 'zero': infinite frequency) and summed over the band
    -> dict(acc int64 [n][nbin][4], hits [n][nbin], bins PROF_BIN [n][nbin], results PROF_RESULT [n], used [n][nchans]).
    ``tau`` (microseconds, one value or one per burst; None: none): the delay between the two circular feeds that ``polcal_fil``
    measures, taken out with the rotation (frbch_polprof_cal_host).
    ``info['kernel_used']``: 1 = the fast kernel, 0 = the generic one; ``info['spectra_kernel_used']``: the burst sums'."""
    lib = lib or _lib.load()
    rows, nrows, cands, par, g = _burst_args(fil_or_rows, hdr, cands, gains, products)
    n, nchan = cands.size, hdr["nchans"]
    rm = np.ascontiguousarray(np.broadcast_to(np.asarray(rm, dtype=np.float64), (n,)))
    tau = None if tau is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tau, dtype=np.float64), (n,)))
    fl = _flag_arg(flag, nchan)
    ppar = prof_params(nbin, tfactor, ref)
    nb = max(1, min(int(nbin), 1024))
    acc = np.zeros((n, nb, 4), np.int64)
    hits = np.zeros((n, nb), np.uint32)
    bins = np.zeros((n, nb), dtype=PROF_BIN)
    res = np.zeros(n, dtype=PROF_RESULT)
    used = np.zeros((n, nchan), np.uint8)
    k = (C.c_uint32 * 2)(0, 0)
    err = C.create_string_buffer(512)
    desc, tail = fil_desc(hdr, hdr.get("product", 0)), (g.ctypes.data if g is not None else None, fl.ctypes.data if fl is not None else None,
                                                         C.byref(ppar), device, acc.ctypes.data, hits.ctypes.data, bins.ctypes.data,
                                                         res.ctypes.data, used.ctypes.data, k, err, len(err))
    if tau is None:
        _check(lib.frbch_polprof_host(C.byref(desc), rows.ctypes.data, nrows, C.byref(par), cands.ctypes.data, n, rm.ctypes.data, *tail), err)
    else:
        _check(lib.frbch_polprof_cal_host(C.byref(desc), rows.ctypes.data, nrows, C.byref(par), cands.ctypes.data, n, rm.ctypes.data,
                                          tau.ctypes.data, *tail), err)
    if info is not None:
        info.update(spectra_kernel_used=k[0], kernel_used=k[1])
    return dict(acc=acc, hits=hits, bins=bins, results=res, used=used)


def _polprof_png(path, bins):
    """above: the PA of the bins with a valid one, -90 .. 90 degrees bottom to top; below: I, L (debiased) and V on one scale"""
    width, height = 512, 96
    n = bins.size
    top = np.zeros((height, width))
    for j in np.flatnonzero(bins["pa_valid"] != 0):
        x = min(width - 1, int((j + 0.5) * width / n))
        deg = min(90.0, max(-90.0, float(np.degrees(bins["pa"][j]))))
        top[(height - 1) - int(round((deg + 90.0) / 180.0 * (height - 1))), x] = 1.0
    low = _curve_panel([bins["i"], bins["l_db"], bins["v"]], width, height)
    write_png(path, np.concatenate([top, np.zeros((4, width)), low], axis=0))


def _polprof_write(base, hdr, cands, rm, prof, tfactor, ref="mean"):
    """-> the files: <base>_polprof.npz, <base>_polprof.txt (per burst a '#' line, then one line per bin: the time of the bin's
    centre at the top of the band in seconds, I, L debiased, V, PA and its error in degrees, nan without a valid PA) and
    <base>_polprof_burst<i>.png"""
    files = [base + "_polprof.npz", base + "_polprof.txt"]
    rm = np.broadcast_to(np.asarray(rm, dtype=np.float64), (cands.size,))
    nbin = prof["bins"].shape[1]
    np.savez(files[0], acc=prof["acc"], hits=prof["hits"], bins=prof["bins"], results=prof["results"], used=prof["used"], bursts=cands,
             rm=np.array(rm), tfactor=np.int64(tfactor), ref=np.array(str(ref)))
    with open(files[1], "w") as f:
        for i, c in enumerate(cands):
            r = prof["results"][i]
            f.write("# burst%d  DM %.3f  sample %d  RM %+.3f  nbin %d  tfactor %d  ref %s  sigma_I %.6g  sigma_L %.6g  on-pulse bins %d..%d\n"
                    % (i, c["dm"], int(c["sample"]), rm[i], nbin, tfactor, ref, r["sigma_i"], r["sigma_l"], r["on_lo_bin"], r["on_hi_bin"]))
            t0 = int(c["sample"]) - (nbin // 2) * int(tfactor)
            for j, b in enumerate(prof["bins"][i]):
                ok = b["pa_valid"] != 0
                f.write(PROF_ROW % ((t0 + (j + 0.5) * tfactor) * hdr["tsamp"], b["i"], b["l_db"], b["v"],
                                    np.degrees(b["pa"]) if ok else np.nan, np.degrees(b["pa_err"]) if ok else np.nan) + "\n")
            _polprof_png(base + "_polprof_burst%d.png" % i, prof["bins"][i])
            files.append(base + "_polprof_burst%d.png" % i)
    return files


def polprof_fil(filterbankfile, bursts=None, rm=None, nbin=256, tfactor=1, ref="mean", off_gap=None, off_len=None, flag_file=None,
                gains=None, products="stokes", rm_from=None, device=0, lib=None, info: dict | None = None, polcal_file=None):
    """Polarisation profiles of the bursts of a full-Stokes filterbank: ``bursts`` = (dm, sample, width) tuples with ``rm`` (one
    value or one per burst), or ``rm_from`` = the ``<base>_rm.npz`` that ``rmsynth_fil`` wrote (its bursts and fitted RMs).
    ``polcal_file``: the ``<base>_polcal.npz`` of a calibrator, whose delay between the two circular feeds is taken out.
    Writes ``<base>_polprof.npz / .txt`` and ``<base>_polprof_burst<i>.png``.  Returns (files, what ``pol_profile`` returns)."""
    lib = lib or _lib.load()
    fil = sigproc.read_fil(filterbankfile)
    hdr = fil.header
    if hdr.get("nifs", 1) != 4:
        raise InputError("polprof needs a four-product file (pol_mode 4 or 5)")
    if rm_from:
        back = np.load(rm_from)
        cands, rm = np.ascontiguousarray(back["bursts"]), back["results"]["rm"]
    else:
        if not bursts or rm is None:
            raise InputError("give bursts (--dm --sample/--time --width) with --rm, or --rm-from")
        cands = burst_cands(bursts, off_gap, off_len)
    flag = read_flag_file(flag_file, hdr["nchans"]).astype(np.uint8) if flag_file else None
    if isinstance(gains, str):
        gains = np.load(gains)
    prof = pol_profile(fil, hdr, cands, rm, nbin=nbin, tfactor=tfactor, ref=ref, gains=gains, flag=flag, products=products,
                       device=device, lib=lib, info=info, tau=polcal_tau(polcal_file) if polcal_file else None)
    return _polprof_write(filterbankfile.replace(".fil", ""), hdr, cands, rm, prof, tfactor, ref), prof


# ------------------------------------------------------------------------------------------------------------------
# DM of a burst: fine DM scan, S/N and structure maxima (frbch_dmscan_*)
# ------------------------------------------------------------------------------------------------------------------
DMSCAN_RESULT = np.dtype([("dm_snr", "<f8"), ("dm_snr_err", "<f8"), ("dm_struct", "<f8"), ("snr_peak", "<f8"), ("struct_peak", "<f8"),
                          ("snr_at_struct", "<f8"), ("k_snr", "<u4"), ("width_snr", "<u4"), ("bin_snr", "<u4"), ("nfit_snr", "<u4"),
                          ("fitted_snr", "<u4"), ("k_struct", "<u4"), ("width_struct", "<u4"), ("bin_struct", "<u4"),
                          ("nfit_struct", "<u4"), ("fitted_struct", "<u4"), ("k", "<i4"), ("nused", "<u4")])
DM_ROW = "%-8s DM0 %9.3f sample %10d  DM_snr %10.4f +- %7.4f (S/N %7.2f, width %3d bins%s)  DM_struct %10.4f (S/N %7.2f%s)"


def dm_sample_step(hdr: dict, lib=None) -> float:
    """The change of DM that moves the bottom of the band by one row (frbch_dm_sample_step), pc cm^-3"""
    lib = lib or _lib.load()
    return float(lib.frbch_dm_sample_step(C.byref(fil_desc(hdr, hdr.get("product", 0)))))


def dmscan_params(ntrial: int, ddm: float, nbin: int, tfactor: int) -> _lib.FrbchDmscanParams:
    return _lib.FrbchDmscanParams(C.sizeof(_lib.FrbchDmscanParams), int(ntrial), int(nbin), int(tfactor), float(ddm))


def dmscan_peak_params(widths=(1, 2, 4, 8), smooth: int = 3, fit_frac: float = 0.5) -> _lib.FrbchDmscanPeakParams:
    widths = [int(w) for w in widths]
    if not 1 <= len(widths) <= 16:
        raise InputError("1..16 boxcar widths")
    p = _lib.FrbchDmscanPeakParams(C.sizeof(_lib.FrbchDmscanPeakParams), len(widths))
    for i, w in enumerate(widths):
        p.widths[i] = w
    p.smooth, p.fit_frac = int(smooth), float(fit_frac)
    return p


def dm_scan(fil_or_rows, hdr: dict, cands, ntrial: int, ddm: float, nbin: int = 64, tfactor: int = 1, widths=(1, 2, 4, 8),
            smooth: int = 3, fit_frac: float = 0.5, flag=None, products: str = "stokes", device: int = 0, lib=None,
            info: dict | None = None):
    """The DM of every burst (frbch_dmscan_host; include/frbch.h states the arithmetic): its noise-weighted, band-summed profile
    in ``nbin`` bins of ``tfactor`` rows about ``sample`` at ``ntrial`` DMs ``ddm`` apart about the burst's own, the largest
    boxcar S/N (over ``widths``, in bins) and the structure (squared differences of the profile smoothed over ``smooth`` bins)
    of every trial, and a parabola over the part of each curve above ``fit_frac`` of its peak -> dict(acc int64
    [n][ntrial][nbin], hits, snr and struct [n][ntrial], dm [n][ntrial], results DMSCAN_RESULT [n], used [n][nchans]).
    ``products='stokes'`` reads product ``hdr['product']`` (0), ``'coherency'`` PP + QQ of a four-product file.
    ``info['kernel_used']``: 1 = the fast kernel, 0 = the generic one; ``info['spectra_kernel_used']``: the burst sums'."""
    lib = lib or _lib.load()
    rows, nrows, cands, par, _g = _burst_args(fil_or_rows, hdr, cands, None, products)
    n, nchan = cands.size, hdr["nchans"]
    fl = _flag_arg(flag, nchan)
    dpar, pk = dmscan_params(ntrial, ddm, nbin, tfactor), dmscan_peak_params(widths, smooth, fit_frac)
    nt, nb = max(1, min(int(ntrial), 4096)), max(1, min(int(nbin), 1024))
    if n * nt * nb > 1 << 24:
        raise InputError("ncand * ntrial * nbin exceeds 2^24: cut the batch or the scan")
    acc = np.zeros((n, nt, nb), np.int64)
    hits = np.zeros((n, nt, nb), np.uint32)
    snr, strc = np.zeros((n, nt)), np.zeros((n, nt))
    res = np.zeros(n, dtype=DMSCAN_RESULT)
    used = np.zeros((n, nchan), np.uint8)
    k = (C.c_uint32 * 2)(0, 0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_dmscan_host(C.byref(fil_desc(hdr, hdr.get("product", 0))), rows.ctypes.data, nrows, C.byref(par), cands.ctypes.data, n,
                                 fl.ctypes.data if fl is not None else None, C.byref(dpar), C.byref(pk), device, acc.ctypes.data,
                                 hits.ctypes.data, snr.ctypes.data, strc.ctypes.data, res.ctypes.data, used.ctypes.data, k, err, len(err)), err)
    if info is not None:
        info.update(spectra_kernel_used=k[0], kernel_used=k[1])
    dm = cands["dm"][:, None] + (np.arange(nt, dtype=np.float64) - float(nt // 2))[None, :] * (float(ddm) if nt > 1 else 0.0)
    return dict(acc=acc, hits=hits, snr=snr, struct=strc, dm=dm, results=res, used=used)


def _dm_parabola(v, kpeak, nfit_lo_hi, width):
    """the least-squares parabola over trials lo .. hi of a curve, drawn over all `width` columns (nan outside lo .. hi)"""
    lo, hi = nfit_lo_hi
    out = np.full(v.size, np.nan)
    if hi - lo >= 2:
        x = np.arange(lo, hi + 1) - kpeak
        out[lo:hi + 1] = np.polyval(np.polyfit(x, v[lo:hi + 1], 2), x)
    return out


def _dm_fit_range(v, kpeak, fit_frac):
    lo = hi = int(kpeak)
    thr = fit_frac * v[kpeak]
    while lo > 0 and v[lo - 1] >= thr:
        lo -= 1
    while hi + 1 < v.size and v[hi + 1] >= thr:
        hi += 1
    return lo, hi


def _dm_png(path, scan, i, fit_frac):
    """above: the bow tie, trials bottom to top against the bins; below: the S/N and the structure curve against the trial, each
    with its fitted parabola"""
    width, height = 512, 96
    res = scan["results"][i]
    a = scan["acc"][i].astype(np.float64) / np.sqrt(np.maximum(scan["hits"][i], 1))
    nt, nb = a.shape
    rows = np.clip((np.arange(2 * height) * nt) // (2 * height), 0, nt - 1)[::-1]
    cols = np.clip((np.arange(width) * nb) // width, 0, nb - 1)
    tie = a[rows][:, cols]
    tie = (tie - tie.min()) / max(1e-30, float(tie.max() - tie.min()))
    panels = [tie]
    for name, kname, fname in (("snr", "k_snr", "fitted_snr"), ("struct", "k_struct", "fitted_struct")):
        v = scan[name][i]
        curves = [v]
        if res[fname]:
            fit = _dm_parabola(v, int(res[kname]), _dm_fit_range(v, int(res[kname]), fit_frac), width)
            curves = [np.where(np.isnan(fit), v, fit), v]
        panels += [np.zeros((4, width)), _curve_panel(curves, width, height)]
    write_png(path, np.concatenate(panels, axis=0))


def dmfit_fil(filterbankfile, bursts=None, dm1=None, dm2=0.0, dmstep=1.0, width=0, dm_half=None, ddm=None, nbin=None, tfactor=None,
              smooth=3, fit_frac=0.5, off_gap=None, off_len=None, flag_file=None, products="stokes", threshold=8.0, max_cands=8,
              device=0, lib=None, info: dict | None = None):
    """The DM of the bursts of a filterbank: ``bursts`` = (dm, sample, width) tuples; or, with ``dm1 .. dm2 .. dmstep`` and no
    bursts, the strongest groups of the search, exactly as ``rmsynth_fil`` finds them.  Defaults, in DM sample steps (one step
    moves the bottom of the band by one row: ``dm_sample_step``): ``ddm`` a quarter of a step, ``dm_half`` 32 steps either side
    (cut so that no trial lies below DM 0); ``tfactor`` an eighth of the largest width (at least 1 row) and ``nbin`` so that the
    window holds four widths plus the sweep of the edge trial on either side (16 .. 1024 bins); the boxcars are 1, 2, 4 .. bins up
    to half the window; ``off_gap`` is at least that sweep, so that no trial drags the burst into an off-pulse window.  The S/N
    curve of a burst much wider than the sweep has a flat top: give it a larger ``dm_half`` or ``fit_frac``.  Writes
    ``<base>_dm.npz`` (acc, hits, snr, struct, dm, results, used, bursts, ddm, tfactor, smooth, fit_frac), ``<base>_dm.txt`` (one line
    per burst: the S/N-maximising DM +- its error and the structure-maximising DM) and ``<base>_dm_burst<i>.png`` (the bow tie and
    the two curves with their fits).  Returns (files, what ``dm_scan`` returns)."""
    lib = lib or _lib.load()
    fil = sigproc.read_fil(filterbankfile)
    hdr = fil.header
    if not bursts:
        if dm1 is None:
            raise InputError("give bursts (--dm --sample/--time --width) or a DM range to search")
        dms = dm_list(dm1, dm2, dmstep)
        _files, recs = _search(fil, filterbankfile, dm1, dm2, dmstep, True, 5, threshold, 0.0, 1000, False, None, device, lib, {})
        groups = group_candidates(recs, hdr, dms, lib=lib)
        groups = groups[np.argsort(-groups["best"]["sigma"], kind="stable")[:max_cands]]
        bursts = [(dms[int(g["best"]["dm_index"])], int(g["best"]["sample"]), max(int(width), int(g["best"]["width"]))) for g in groups]
        if not bursts:
            raise InputError("the search found no burst above the threshold")
    step = dm_sample_step(hdr, lib)
    if not step > 0:
        raise InputError("dmfit needs at least two channels")
    ddm = float(ddm) if ddm else step / 4.0
    half = float(dm_half) if dm_half else 32.0 * step
    lowest = min(float(b["dm"] if isinstance(b, dict) or hasattr(b, "dtype") else b[0]) for b in bursts)
    ntrial = 2 * int(min(2047, max(0, min(half, lowest) // ddm))) + 1
    sweep = int(np.ceil((ntrial // 2) * ddm / step))
    wmax = max(int(b["width"] if isinstance(b, dict) or hasattr(b, "dtype") else b[2]) for b in bursts)
    tfactor = int(tfactor) if tfactor else max(1, min(512, wmax // 8))
    nbin = int(nbin) if nbin else int(min(1024, max(16, -(-(4 * wmax + 2 * sweep) // tfactor))))
    cands = burst_cands(bursts, off_gap, off_len)
    if off_gap is None:
        cands = cands.copy()
        cands["off_gap"] = np.maximum(cands["off_gap"], sweep)
    flag = read_flag_file(flag_file, hdr["nchans"]).astype(np.uint8) if flag_file else None
    widths = [w for w in (1, 2, 4, 8, 16, 32, 64) if w <= max(1, nbin // 2)]
    scan = dm_scan(fil, hdr, cands, ntrial, ddm, nbin, tfactor, widths=widths, smooth=min(int(smooth), max(1, nbin - 1)), fit_frac=fit_frac,
                   flag=flag, products=products, device=device, lib=lib, info=info)
    base = filterbankfile.replace(".fil", "")
    files = [base + "_dm.npz", base + "_dm.txt"]
    np.savez(files[0], acc=scan["acc"], hits=scan["hits"], snr=scan["snr"], struct=scan["struct"], dm=scan["dm"], results=scan["results"],
             used=scan["used"], bursts=cands, ddm=np.float64(ddm), tfactor=np.int64(tfactor), smooth=np.int64(smooth),
             fit_frac=np.float64(fit_frac), step=np.float64(step))
    with open(files[1], "w") as f:
        for i, (c, r) in enumerate(zip(cands, scan["results"])):
            f.write(DM_ROW % ("burst%d" % i, c["dm"], int(c["sample"]), r["dm_snr"], r["dm_snr_err"], r["snr_peak"], int(r["width_snr"]),
                              "" if r["fitted_snr"] else ", not fitted", r["dm_struct"], r["snr_at_struct"],
                              "" if r["fitted_struct"] else ", not fitted") + "\n")
            _dm_png(base + "_dm_burst%d.png" % i, scan, i, fit_frac)
            files.append(base + "_dm_burst%d.png" % i)
    return files, scan


def bursts_from_dm(path, kind="snr") -> np.ndarray:
    """The BURST_CAND records of a ``<base>_dm.npz`` with the DM that ``dmfit_fil`` measured in place of the one it was given;
    ``kind``: 'snr' or 'struct'"""
    if kind not in ("snr", "struct"):
        raise InputError("--dm-kind must be snr or struct")
    back = np.load(path)
    cands = np.ascontiguousarray(back["bursts"]).copy()
    res = back["results"]
    cands["dm"] = np.where(res["nused"] > 0, res["dm_" + kind], cands["dm"])       # (a dead burst keeps the DM it came with)
    return cands


# ------------------------------------------------------------------------------------------------------------------
# Structure of a burst: dynamic spectrum and its two-dimensional ACF (frbch_burstacf_*, frbch_acf2d_*)
# ------------------------------------------------------------------------------------------------------------------
ACF_RESULT = np.dtype([("width_f_mhz", "<f8"), ("width_t_ms", "<f8"), ("dt_df", "<f8"), ("drift", "<f8"), ("ref", "<f8"), ("mff", "<f8"),
                       ("mtf", "<f8"), ("mtt", "<f8"), ("k", "<i4"), ("r", "<u4"), ("nused", "<u4"), ("ncomplete", "<u4"),
                       ("fitted_f", "<u4"), ("fitted_t", "<u4"), ("fitted_d", "<u4"), ("reserved", "<u4")])
ACF_ROW = "%-8s DM %9.3f sample %10d  bandwidth %9.4f MHz%s  duration %9.4f ms%s  drift %10.3f MHz/ms (%+.5f ms/MHz%s)"


def acf_params(nbin: int, tfactor: int, ffactor: int, nlagf: int, nlagt: int) -> _lib.FrbchAcfParams:
    return _lib.FrbchAcfParams(C.sizeof(_lib.FrbchAcfParams), int(nbin), int(tfactor), int(ffactor), int(nlagf), int(nlagt))


def acf_fit_params(fit_frac: float = 0.5) -> _lib.FrbchAcfFitParams:
    return _lib.FrbchAcfFitParams(C.sizeof(_lib.FrbchAcfFitParams), 0, float(fit_frac))


def acf2d(y, nlagf: int, nlagt: int, form: int = _lib.ACF_PLAN, device: int = 0, lib=None, info: dict | None = None) -> np.ndarray:
    """The two-dimensional autocorrelation of int32 planes ``y [n][nsub][nbin]`` with |y| <= 2^21 (frbch_acf2d_host) -> int64
    ``[n][nlagf][2 nlagt - 1]``: A[df][dt + nlagt - 1] = the sum of y[s][j] y[s + df][j + dt].  ``info['kernel_used']``: 1 = the
    fast kernel, 0 = the generic one; ``form=_lib.ACF_GENERIC`` asks for the generic one."""
    lib = lib or _lib.load()
    y = np.ascontiguousarray(y, dtype=np.int32)
    if y.ndim != 3:
        raise InputError("y must have the shape [n][nsub][nbin]")
    n, nsub, nbin = y.shape
    lf, lt = max(1, min(int(nlagf), 1024)), max(1, min(int(nlagt), 256))
    if n * lf * (2 * lt - 1) > 1 << 24:
        raise InputError("ncand * nlagf * (2 nlagt - 1) exceeds 2^24: cut the batch or the lags")
    A = np.zeros((n, lf, 2 * lt - 1), np.int64)
    k = C.c_uint32(0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_acf2d_host(y.ctypes.data, n, nsub, nbin, int(nlagf), int(nlagt), int(form), device, A.ctypes.data, C.byref(k), err, len(err)), err)
    if info is not None:
        info.update(kernel_used=k.value)
    return A


def burst_acf(fil_or_rows, hdr: dict, cands, nbin: int = 256, tfactor: int = 1, ffactor: int = 1, nlagf: int | None = None,
              nlagt: int | None = None, fit_frac: float = 0.5, flag=None, products: str = "stokes", device: int = 0, lib=None,
              info: dict | None = None):
    """The structure of every burst (frbch_burstacf_host; include/frbch.h states the arithmetic): the dedispersed, baseline-free,
    noise-weighted dynamic spectrum in ``nchans / ffactor`` subbands and ``nbin`` bins of ``tfactor`` rows about ``sample``, its
    two-dimensional autocorrelation at ``nlagf`` frequency lags and ``-(nlagt - 1) .. nlagt - 1`` time lags (defaults: half the
    plane, at most 1024 and 256), and from it the half-widths of the two cuts and the drift -> dict(Y int64 [n][nsub][nbin], yhits,
    A int64 [n][nlagf][2 nlagt - 1], P uint32 (complete pairs per lag), norm float64 (A scaled back and divided by P), results
    ACF_RESULT [n], used [n][nchans]).  ``info``: ``spectra_kernel_used``, ``dynspec_kernel_used``, ``kernel_used`` (the ACF's): 1 =
    the fast kernel, 0 = the generic one."""
    lib = lib or _lib.load()
    rows, nrows, cands, par, _g = _burst_args(fil_or_rows, hdr, cands, None, products)
    n, nchan = cands.size, hdr["nchans"]
    fl = _flag_arg(flag, nchan)
    ffactor = int(ffactor)
    if ffactor < 1 or ffactor > nchan or nchan % ffactor:
        raise InputError("ffactor must be 1..nchans and divide nchans")
    nsub, nb = nchan // ffactor, max(1, min(int(nbin), 1024))
    nlagf = max(1, min(nsub // 2, 1024)) if nlagf is None else int(nlagf)
    nlagt = max(1, min(nb // 2, 256)) if nlagt is None else int(nlagt)
    lf, lt = max(1, min(nlagf, 1024)), max(1, min(nlagt, 256))
    if nsub * nb > 1 << 20 or n * nsub * nb > 1 << 24 or n * lf * (2 * lt - 1) > 1 << 24:
        raise InputError("nsub * nbin exceeds 2^20, or ncand * nsub * nbin or ncand * nlagf * (2 nlagt - 1) exceeds 2^24: cut the batch, the window or the lags")
    apar, fpar = acf_params(nbin, tfactor, ffactor, nlagf, nlagt), acf_fit_params(fit_frac)
    Y, yhits = np.zeros((n, nsub, nb), np.int64), np.zeros((n, nsub, nb), np.uint32)
    A, P = np.zeros((n, lf, 2 * lt - 1), np.int64), np.zeros((n, lf, 2 * lt - 1), np.uint32)
    res = np.zeros(n, dtype=ACF_RESULT)
    used = np.zeros((n, nchan), np.uint8)
    k = (C.c_uint32 * 3)(0, 0, 0)
    err = C.create_string_buffer(512)
    desc = fil_desc(hdr, hdr.get("product", 0))
    _check(lib.frbch_burstacf_host(C.byref(desc), rows.ctypes.data, nrows, C.byref(par), cands.ctypes.data, n,
                                   fl.ctypes.data if fl is not None else None, C.byref(apar), C.byref(fpar), device, Y.ctypes.data,
                                   yhits.ctypes.data, A.ctypes.data, P.ctypes.data, res.ctypes.data, used.ctypes.data, k, err, len(err)), err)
    if info is not None:
        info.update(spectra_kernel_used=k[0], dynspec_kernel_used=k[1], kernel_used=k[2])
    norm = np.zeros(A.shape)
    ks, rs, nu, nc = (np.ascontiguousarray(res[f]) for f in ("k", "r", "nused", "ncomplete"))
    _check(lib.frbch_burstacf_fit(C.byref(desc), C.byref(apar), C.byref(fpar), n, ks.ctypes.data, rs.ctypes.data, nu.ctypes.data,
                                  nc.ctypes.data, A.ctypes.data, P.ctypes.data, norm.ctypes.data, None, err, len(err)), err)
    return dict(Y=Y, yhits=yhits, A=A, P=P, norm=norm, results=res, used=used)


def _resample(img, height, width):
    r = np.clip((np.arange(height) * img.shape[0]) // height, 0, img.shape[0] - 1)
    c = np.clip((np.arange(width) * img.shape[1]) // width, 0, img.shape[1] - 1)
    return img[r][:, c]


def _acf_panels(acf, i):
    """above: the dynamic spectrum, subbands top to bottom against the bins; then the ACF (both half-planes, df top to bottom,
    the lag (0, 0) taken out) with its ridge line dt = dt_df df; below: the frequency cut and the time cut"""
    width, height = 512, 96
    res = acf["results"][i]
    dyn = acf["Y"][i].astype(np.float64) / np.maximum(acf["yhits"][i], 1)
    nm = acf["norm"][i].copy()
    nlf, ndt = nm.shape
    L = ndt // 2
    nm[0, L] = 0.0
    full = np.concatenate([nm[:0:-1, ::-1], nm], axis=0)               # df = -(nlagf - 1) .. nlagf - 1
    img = _unit(_resample(full, 2 * height, width))
    if res["fitted_d"] and res["mff"] > 0:
        slope = res["mtf"] / res["mff"]                                  # bins per subband
        for row in range(2 * height):
            df = (row * full.shape[0]) // (2 * height) - (nlf - 1)
            col = int(round((slope * df + L) * width / ndt))
            if 0 <= col < width:
                img[row, col] = 1.0
    panels = [_unit(_resample(dyn, 2 * height, width)), np.zeros((4, width)), img, np.zeros((4, width)),
              _curve_panel([nm[1:, L]] if nlf > 1 else [np.zeros(1)], width, height), np.zeros((4, width)),
              _curve_panel([nm[0, L + 1:]] if L > 0 else [np.zeros(1)], width, height)]
    return np.concatenate(panels + [np.zeros((8, width))], axis=0)


def burstacf_fil(filterbankfile, bursts, nbin=256, tfactor=1, ffactor=1, nlagf=None, nlagt=None, fit_frac=0.5, off_gap=None,
                 off_len=None, flag_file=None, products="stokes", device=0, lib=None, info: dict | None = None):
    """The structure of the bursts of a filterbank: ``bursts`` = (dm, sample, width) tuples or BURST_CAND records.  Writes
    ``<base>_acf.npz`` (Y, yhits, A, P, norm, results, used, bursts, nbin, tfactor, ffactor, fit_frac), ``<base>_acf.txt`` (one line
    per burst: the half-widths at half maximum of the frequency and the time cut of the ACF, and the drift) and ``<base>_acf.png``
    (per burst, one below the other: the dynamic spectrum, the ACF with its ridge line, the two cuts).  Returns (files, what
    ``burst_acf`` returns)."""
    lib = lib or _lib.load()
    fil = sigproc.read_fil(filterbankfile)
    hdr = fil.header
    cands = burst_cands(bursts, off_gap, off_len)
    flag = read_flag_file(flag_file, hdr["nchans"]).astype(np.uint8) if flag_file else None
    acf = burst_acf(fil, hdr, cands, nbin, tfactor, ffactor, nlagf, nlagt, fit_frac=fit_frac, flag=flag, products=products, device=device,
                    lib=lib, info=info)
    base = filterbankfile.replace(".fil", "")
    files = [base + "_acf.npz", base + "_acf.txt", base + "_acf.png"]
    np.savez(files[0], bursts=cands, nbin=np.int64(nbin), tfactor=np.int64(tfactor), ffactor=np.int64(ffactor), fit_frac=np.float64(fit_frac), **acf)
    with open(files[1], "w") as f:
        for i, (c, r) in enumerate(zip(cands, acf["results"])):
            f.write(ACF_ROW % ("burst%d" % i, c["dm"], int(c["sample"]), r["width_f_mhz"], "" if r["fitted_f"] else " (not fitted)", r["width_t_ms"],
                               "" if r["fitted_t"] else " (not fitted)", r["drift"], r["dt_df"], "" if r["fitted_d"] else ", not fitted") + "\n")
    write_png(files[2], np.concatenate([_acf_panels(acf, i) for i in range(cands.size)], axis=0))
    return files, acf


# ------------------------------------------------------------------------------------------------------------------
# Scattering of a burst: a bank of scattered Gaussians per subband, tau(nu) across the band (frbch_burstscat_*, frbch_tbank_*)
# ------------------------------------------------------------------------------------------------------------------
SCAT_SUB = np.dtype([("sigma", "<f8"), ("tau", "<f8"), ("arrival", "<f8"), ("sigma_ms", "<f8"), ("tau_ms", "<f8"), ("arrival_ms", "<f8"),
                     ("amp", "<f8"), ("area", "<f8"), ("snr", "<f8"), ("q", "<f8"), ("tau_lo", "<f8"), ("tau_hi", "<f8"),
                     ("dq_unscattered", "<f8"), ("freq_mhz", "<f8"), ("k", "<u4"), ("u", "<u4"), ("nused", "<u4"), ("bounded_lo", "<u4"),
                     ("bounded_hi", "<u4"), ("reserved", "<u4")])
SCAT_BAND = np.dtype([("tau_ref", "<f8"), ("tau_ref_ms", "<f8"), ("alpha", "<f8"), ("sigma", "<f8"), ("sigma_ms", "<f8"), ("arrival", "<f8"),
                      ("arrival_ms", "<f8"), ("q", "<f8"), ("tau_ref_lo", "<f8"), ("tau_ref_hi", "<f8"), ("alpha_lo", "<f8"),
                      ("alpha_hi", "<f8"), ("nu_ref_mhz", "<f8"), ("k", "<i4"), ("r", "<u4"), ("nused", "<u4"), ("nfit", "<u4"),
                      ("nclipped", "<u4"), ("b_ref", "<u4"), ("a", "<u4"), ("u", "<u4"), ("ialpha", "<u4"), ("bounded_lo", "<u4"),
                      ("bounded_hi", "<u4"), ("reserved", "<u4")])
SCAT_ROW = "%-8s DM %9.3f sample %10d  tau(%.1f MHz) %9.4f ms (%.4f .. %.4f%s)  alpha %6.3f (%.3f .. %.3f)  sigma %8.4f ms  %d subbands, %d clipped"
SCAT_SUB_ROW = "  %10.3f MHz  snr %8.2f  tau %9.4f ms (%.4f .. %.4f%s)  sigma %8.4f ms  arrival %9.4f ms  dq(unscattered) %8.2f"
SCAT_ALPHAS = (0.0, 1.0, 2.0, 3.0, 4.0, 4.4, 5.0, 6.0)


def scat_bank_params(nsig=16, ntau=32, ntap=256, lead=None, sigma0=0.5, rsig=2.0 ** 0.25, tau0=0.5, rtau=2.0 ** 0.25) -> _lib.FrbchScatBankParams:
    lead = int(ntap) // 4 if lead is None else int(lead)
    return _lib.FrbchScatBankParams(C.sizeof(_lib.FrbchScatBankParams), int(nsig), int(ntau), int(ntap), lead, (C.c_uint32 * 3)(0, 0, 0),
                                    float(sigma0), float(rsig), float(tau0), float(rtau))


def scat_params(nbin: int, tfactor: int, ffactor: int, shift0: int, nshift: int) -> _lib.FrbchScatParams:
    return _lib.FrbchScatParams(C.sizeof(_lib.FrbchScatParams), int(nbin), int(tfactor), int(ffactor), int(shift0), int(nshift))


def scat_fit_params(alphas=SCAT_ALPHAS, snr_min: float = 5.0) -> _lib.FrbchScatFitParams:
    alphas = [float(a) for a in np.atleast_1d(alphas)]
    if not 1 <= len(alphas) <= 32:
        raise InputError("1..32 values of alpha")
    return _lib.FrbchScatFitParams(C.sizeof(_lib.FrbchScatFitParams), len(alphas), float(snr_min), (C.c_double * 32)(*alphas))


def tbank_shape(nsub, nbin, ntemp, ntap, lead, shift0, nshift) -> _lib.FrbchTbankShape:
    return _lib.FrbchTbankShape(C.sizeof(_lib.FrbchTbankShape), int(nsub), int(nbin), int(ntemp), int(ntap), int(lead), int(shift0), int(nshift))


def scat_bank(bank: _lib.FrbchScatBankParams, lib=None) -> dict:
    """The bank of scattered Gaussians, from the library (frbch_scat_bank, host only) -> dict(p int32 [K][ntap], s1 int64 [K], cum
    int64 [K][ntap + 1], tail float64 [K], sigma [nsig], tau [ntau], in bins)."""
    lib = lib or _lib.load()
    nsig, ntau, ntap = bank.nsig, bank.ntau, bank.ntap
    if not (1 <= ntap <= 1024 and nsig >= 1 and ntau >= 1 and nsig * ntau <= 4096):
        raise InputError("ntap must be 1..1024 and nsig * ntau 1..4096")
    K = nsig * ntau
    out = dict(p=np.zeros((K, ntap), np.int32), s1=np.zeros(K, np.int64), cum=np.zeros((K, ntap + 1), np.int64), tail=np.zeros(K),
               sigma=np.zeros(nsig), tau=np.zeros(ntau))
    err = C.create_string_buffer(512)
    _check(lib.frbch_scat_bank(C.byref(bank), out["p"].ctypes.data, out["s1"].ctypes.data, out["cum"].ctypes.data, out["tail"].ctypes.data,
                               out["sigma"].ctypes.data, out["tau"].ctypes.data, err, len(err)), err)
    return out


def tbank(y, P, lead: int, shift0: int, nshift: int, form: int = _lib.TBANK_PLAN, device: int = 0, lib=None, info: dict | None = None) -> np.ndarray:
    """The correlation of int32 planes ``y [n][nsub][nbin]`` (|y| <= 2^21) with a bank ``P [K][ntap]`` (|P| <= 2^30) at ``nshift``
    arrival bins from ``shift0`` (frbch_tbank_host) -> int64 ``[n][nsub][K][nshift]``.  ``info['kernel_used']``: 1 = the fast kernel,
    0 = the generic one; ``form=_lib.TBANK_GENERIC`` asks for the generic one."""
    lib = lib or _lib.load()
    y, P = np.ascontiguousarray(y, dtype=np.int32), np.ascontiguousarray(P, dtype=np.int32)
    if y.ndim != 3 or P.ndim != 2:
        raise InputError("y must have the shape [n][nsub][nbin] and P the shape [K][ntap]")
    n, nsub, nbin = y.shape
    sh = tbank_shape(nsub, nbin, P.shape[0], P.shape[1], lead, shift0, nshift)
    if int(nshift) < 1 or n * nsub * P.shape[0] * int(nshift) > 1 << 24:
        raise InputError("nshift must be at least 1 and n * nsub * templates * nshift at most 2^24")
    Cc = np.zeros((n, nsub, P.shape[0], int(nshift)), np.int64)
    k = C.c_uint32(0)
    err = C.create_string_buffer(512)
    _check(lib.frbch_tbank_host(y.ctypes.data, P.ctypes.data, n, C.byref(sh), int(form), device, Cc.ctypes.data, C.byref(k), err, len(err)), err)
    if info is not None:
        info.update(kernel_used=k.value)
    return Cc


def burst_scatter(fil_or_rows, hdr: dict, cands, nbin: int = 256, tfactor: int = 1, ffactor: int = 1, bank=None, shift0: int | None = None,
                  nshift: int | None = None, alphas=SCAT_ALPHAS, snr_min: float = 5.0, flag=None, products: str = "stokes",
                  device: int = 0, lib=None, info: dict | None = None):
    """The scattering of every burst (frbch_burstscat_host; include/frbch.h states the arithmetic): the dedispersed dynamic spectrum
    in ``nchans / ffactor`` subbands and ``nbin`` bins of ``tfactor`` rows, every subband correlated with the bank of scattered
    Gaussians ``bank`` (``scat_bank_params``) at ``nshift`` arrival bins from ``shift0`` (default: the middle half of the window),
    the best template per subband and tau(nu) = tau_ref (nu / nu_ref)^-alpha over the listed ``alphas`` -> dict(Y, yhits, y
    [n][nsub][nbin], C, N int64 [n][nsub][K][nshift], q float64 of that shape, sub SCAT_SUB [n][nsub], band SCAT_BAND [n], used,
    bank: what ``scat_bank`` returns).  The intervals are profile intervals on the grid and claim no more (see the header).
    ``info``: ``spectra_kernel_used``, ``dynspec_kernel_used``, ``kernel_used`` (the template bank's): 1 = fast, 0 = generic."""
    lib = lib or _lib.load()
    rows, nrows, cands, par, _g = _burst_args(fil_or_rows, hdr, cands, None, products)
    n, nchan = cands.size, hdr["nchans"]
    fl = _flag_arg(flag, nchan)
    ffactor = int(ffactor)
    if ffactor < 1 or ffactor > nchan or nchan % ffactor:
        raise InputError("ffactor must be 1..nchans and divide nchans")
    bank = bank if bank is not None else scat_bank_params()
    bk = scat_bank(bank, lib)
    nsub, nb, K = nchan // ffactor, max(1, min(int(nbin), 1024)), bank.nsig * bank.ntau
    shift0 = nb // 4 if shift0 is None else int(shift0)
    nshift = max(1, nb // 2) if nshift is None else int(nshift)
    if shift0 < 0 or nshift < 1 or shift0 + nshift > nb:
        raise InputError("nshift must be at least 1 and shift0 + nshift at most nbin")
    if n * nsub * nb > 1 << 24 or n * nsub * K * nshift > 1 << 24:
        raise InputError("ncand * nsub * nbin or ncand * nsub * templates * nshift exceeds 2^24: cut the batch, the bank or the shifts")
    spar, fpar = scat_params(nbin, tfactor, ffactor, shift0, nshift), scat_fit_params(alphas, snr_min)
    Y, yhits, y = np.zeros((n, nsub, nb), np.int64), np.zeros((n, nsub, nb), np.uint32), np.zeros((n, nsub, nb), np.int32)
    Cc, Nn = np.zeros((n, nsub, K, nshift), np.int64), np.zeros((n, nsub, K, nshift), np.int64)
    sub, band = np.zeros((n, nsub), dtype=SCAT_SUB), np.zeros(n, dtype=SCAT_BAND)
    used = np.zeros((n, nchan), np.uint8)
    k = (C.c_uint32 * 3)(0, 0, 0)
    err = C.create_string_buffer(512)
    desc = fil_desc(hdr, hdr.get("product", 0))
    _check(lib.frbch_burstscat_host(C.byref(desc), rows.ctypes.data, nrows, C.byref(par), cands.ctypes.data, n,
                                    fl.ctypes.data if fl is not None else None, C.byref(spar), C.byref(bank), C.byref(fpar), device,
                                    Y.ctypes.data, yhits.ctypes.data, y.ctypes.data, Cc.ctypes.data, Nn.ctypes.data, sub.ctypes.data,
                                    band.ctypes.data, used.ctypes.data, k, err, len(err)), err)
    if info is not None:
        info.update(spectra_kernel_used=k[0], dynspec_kernel_used=k[1], kernel_used=k[2])
    q = np.zeros(Cc.shape)
    ks, rs, nu = (np.ascontiguousarray(band[f]) for f in ("k", "r", "nused"))
    nus = np.ascontiguousarray(sub["nused"])
    _check(lib.frbch_burstscat_fit(C.byref(desc), C.byref(spar), C.byref(bank), C.byref(fpar), n, ks.ctypes.data, rs.ctypes.data, nu.ctypes.data,
                                   nus.ctypes.data, Cc.ctypes.data, Nn.ctypes.data, q.ctypes.data, None, None, err, len(err)), err)
    return dict(Y=Y, yhits=yhits, y=y, C=Cc, N=Nn, q=q, sub=sub, band=band, used=used, bank=bk)


def _scat_panels(sc, i, shift0, lead, tfactor, tsamp):
    """above: the dynamic spectrum, subbands top to bottom against the bins; then one strip per subband (at most 16, evenly
    picked): its profile with the fitted template over it; below: log tau against log nu of the subbands in the band fit with
    the fitted power law"""
    width, height = 512, 96
    dyn = sc["Y"][i].astype(np.float64) / np.maximum(sc["yhits"][i], 1)
    nsub, nbin = dyn.shape
    panels = [_unit(_resample(dyn, 2 * height, width)), np.zeros((4, width))]
    p, ntap = sc["bank"]["p"], sc["bank"]["p"].shape[1]
    for s in np.unique(np.linspace(0, nsub - 1, min(nsub, 16)).astype(int)):
        r = sc["sub"][i, s]
        prof = sc["y"][i, s].astype(np.float64)
        model = np.zeros(nbin)
        if r["q"] > 0:
            j0 = shift0 + int(r["u"]) - lead
            lo, hi = max(0, -j0), min(ntap, nbin - j0)
            amp = float(sc["C"][i, s, r["k"], r["u"]]) / float(sc["N"][i, s, r["k"], r["u"]])
            model[j0 + lo:j0 + hi] = amp * p[r["k"], lo:hi]
        panels += [_curve_panel([prof, model], width, height // 2), np.zeros((2, width))]
    band = sc["band"][i]
    ok = sc["sub"][i]["snr"] > 0
    law = np.zeros((height, width))
    if band["nfit"] and ok.any():
        f = sc["sub"][i]["freq_mhz"][ok]
        order = np.argsort(f)
        fit = band["tau_ref_ms"] * (f[order] / band["nu_ref_mhz"]) ** (-band["alpha"])
        law = _curve_panel([np.log(np.maximum(sc["sub"][i]["tau_ms"][ok][order], 1e-30)), np.log(np.maximum(fit, 1e-30))], width, height)
    return np.concatenate(panels + [law, np.zeros((8, width))], axis=0)


def burstscat_fil(filterbankfile, bursts, nbin=256, tfactor=1, ffactor=1, bank=None, shift0=None, nshift=None, alphas=SCAT_ALPHAS,
                  snr_min=5.0, off_gap=None, off_len=None, flag_file=None, products="stokes", device=0, lib=None, info: dict | None = None):
    """The scattering of the bursts of a filterbank: ``bursts`` = (dm, sample, width) tuples or BURST_CAND records.  Writes
    ``<base>_scat.npz`` (Y, yhits, y, C, N, q, sub, band, used, the bank, bursts and the grid), ``<base>_scat.txt`` (per burst the band
    fit, then one line per subband) and ``<base>_scat.png`` (per burst: the dynamic spectrum, the per-subband fits over the
    profiles, tau against nu with the fitted power law).  Returns (files, what ``burst_scatter`` returns)."""
    lib = lib or _lib.load()
    fil = sigproc.read_fil(filterbankfile)
    hdr = fil.header
    cands = burst_cands(bursts, off_gap, off_len)
    flag = read_flag_file(flag_file, hdr["nchans"]).astype(np.uint8) if flag_file else None
    bank = bank if bank is not None else scat_bank_params()
    sc = burst_scatter(fil, hdr, cands, nbin, tfactor, ffactor, bank, shift0, nshift, alphas, snr_min, flag=flag, products=products,
                       device=device, lib=lib, info=info)
    nshift_used = sc["C"].shape[3]
    shift0_used = int(nbin) // 4 if shift0 is None else int(shift0)
    base = filterbankfile.replace(".fil", "")
    files = [base + "_scat.npz", base + "_scat.txt", base + "_scat.png"]
    arrays = {f: sc[f] for f in ("Y", "yhits", "y", "C", "N", "q", "sub", "band", "used")}
    np.savez(files[0], bursts=cands, nbin=np.int64(nbin), tfactor=np.int64(tfactor), ffactor=np.int64(ffactor), shift0=np.int64(shift0_used),
             nshift=np.int64(nshift_used), lead=np.int64(bank.lead), alphas=np.asarray(alphas, np.float64), snr_min=np.float64(snr_min),
             **arrays, **{"bank_" + f: v for f, v in sc["bank"].items()})
    with open(files[1], "w") as f:
        for i, (c, b) in enumerate(zip(cands, sc["band"])):
            edge = "" if b["bounded_lo"] and b["bounded_hi"] else ", at the grid's edge"
            f.write(SCAT_ROW % ("burst%d" % i, c["dm"], int(c["sample"]), b["nu_ref_mhz"], b["tau_ref_ms"], b["tau_ref_lo"], b["tau_ref_hi"], edge,
                                b["alpha"], b["alpha_lo"], b["alpha_hi"], b["sigma_ms"], b["nfit"], b["nclipped"]) + "\n")
            for r in sc["sub"][i]:
                edge = "" if r["bounded_lo"] and r["bounded_hi"] else ", at the grid's edge"
                f.write(SCAT_SUB_ROW % (r["freq_mhz"], r["snr"], r["tau_ms"], r["tau_lo"], r["tau_hi"], edge, r["sigma_ms"], r["arrival_ms"],
                                        r["dq_unscattered"]) + "\n")
    write_png(files[2], np.concatenate([_scat_panels(sc, i, shift0_used, bank.lead, tfactor, hdr["tsamp"]) for i in range(cands.size)], axis=0))
    return files, sc


def main(argv=None):
    """``python -m frb_baseband_amd.post fold <fil> <par> [--polyco FILE] [--doppler X] [--products coherency|stokes] [...]`` / ``... prepdata <fil> --dm <dm> [...]`` /
    ``... search <fil> --dm <dm> [--dm2 --dmstep --threshold --max-width --detrend ...]`` /
    ``... bandsearch <fil> --dm <dm> [--dm2 --dmstep --nsub N --min-sub A --max-sub B --dm-gap G --plane-mib M, search options]`` /
    ``... candidates <fil> --dm <dm> [search options] [--dm-gap --min-members --max-cands --nt --nf --ndm]`` /
    ``... psearch <fil> --dm <dm> [--dm2 --dmstep --sigma --nharm --flo --nfft --wblock --dm-gap --max-cands --fold-best K --amax A --astep S --acc-gap G]`` /
    ``... rfifind <fil> [--block-rows --t-cell --t-chan --chan-frac --block-frac --flag FILE --write-clean]`` /
    ``... rmsynth <fil> (--dm D --sample S | --time T) --width W [--off-gap G --off-len L] [--phi-max X --dphi Y | --nphi N] [--flag FILE]
    [--gains FILE.npy] [--products stokes|coherency] [--profile --nbin N --tfactor F] [--polcal BASE_polcal.npz]`` (burst options repeatable; or ``--dm .. --dm2 .. --dmstep ..`` to search for them) /
    ``... polcal <fil> --dm D (--sample S | --time T) --width W (--rm-known R | --rm-lo A --rm-hi B --rm-step S) [--tau-half NS --dtau NS --flag FILE --gains FILE.npy]``
    (pulses of a calibrator of known RM, repeatable or searched as for ``rmsynth``: the delay between the two circular feeds, which ``rmsynth`` and ``polprof`` take with ``--polcal``) /
    ``... dmfit <fil> --dm D (--sample S | --time T) --width W [--dm-half H --ddm X --nbin N --tfactor F --smooth S --fit-frac R --flag FILE --coherency]``
    (or ``--dm .. --dm2 .. --dmstep ..`` to search for the bursts; ``rmsynth`` and ``polprof`` take ``--dm-from BASE_dm.npz [--dm-kind snr|struct]`` in place of ``--dm``) /
    ``... burstacf <fil> (--dm D (--sample S | --time T) --width W | --dm-from BASE_dm.npz [--dm-kind snr|struct]) [--nbin N --tfactor F --ffactor F --lagf N --lagt N --fit-frac R --flag FILE --coherency]`` /
    ``... scatter <fil> (--dm D (--sample S | --time T) --width W | --dm-from BASE_dm.npz [--dm-kind snr|struct]) [--nbin N --tfactor F --ffactor F --sigma0 S --nsig N --rsig R --tau0 T --ntau N --rtau R --ntap N --lead M --shift0 J --nshift N --alpha A [A ...] --snr-min S --flag FILE --coherency]`` /
    ``... polprof <fil> (--dm D (--sample S | --time T) --width W --rm R | --rm-from BASE_rm.npz) [--nbin N --tfactor F --ref mean|zero --flag FILE --gains FILE.npy --coherency]``
    (``search`` and ``candidates`` take ``--flag FILE`` and ``--rfi``; ``search``, ``candidates`` and ``rfifind`` take ``--resident``:
    one upload of the rows per command; ``rfifind --periodic [--t-freq S]`` and ``--rfi --periodic`` add the periodicity test): the stages
    as commands, for the places where base2fil.sh / process_vdif.py launch dspsr and prepdata"""
    import argparse
    ap = argparse.ArgumentParser(prog="frb_baseband_amd.post")
    sub = ap.add_subparsers(dest="cmd", required=True)
    f = sub.add_parser("fold", help="fold a filterbank with a .par file (base2fil.sh:465-493)")
    f.add_argument("fil")
    f.add_argument("par")
    f.add_argument("--nbin", type=int, default=0, help="phase bins (0: largest power of two <= period / tsamp, at most 1024)")
    f.add_argument("-L", "--subint", type=float, default=10.0, help="sub-integration length, s (dspsr -L 10)")
    f.add_argument("--fscrunch", type=int, default=128, help='channels of the plot (psrplot -j "fscrunch 128")')
    f.add_argument("--polyco", default=None, help="TEMPO polyco file of the same .par (tempo2 -polyco ... -tempo1): fold with the predictor")
    f.add_argument("--doppler", type=float, default=0.0, help="constant Doppler factor (observed / intrinsic spin frequency - 1) for the F0 / F1 polynomial")
    f.add_argument("--products", choices=("coherency", "stokes"), default="coherency", help="what a four-product file holds: the -d4 products, or I, Q, U, V")
    f.add_argument("--refine", action="store_true", help="search DM, F0 and F1 about the ephemeris behind the fold: the outputs of `foldfit`")
    f.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    ff = sub.add_parser("foldfit", help="fold with an ephemeris and refine it: a search over DM, spin frequency and its derivative on the folded cube")
    ff.add_argument("fil")
    ff.add_argument("par", nargs="?", default=None, help=".par file (or --f0 and --dm)")
    ff.add_argument("--f0", type=float, default=None, help="spin frequency, Hz")
    ff.add_argument("--f1", type=float, default=0.0, help="frequency derivative, Hz / s")
    ff.add_argument("--dm", type=float, default=None)
    ff.add_argument("--nbin", type=int, default=0, help="phase bins (0: as `fold`)")
    ff.add_argument("-L", "--subint", type=float, default=10.0, help="sub-integration length, s")
    ff.add_argument("--ndm", type=int, default=33, help="DM trials (odd, or 1)")
    ff.add_argument("--nfreq", type=int, default=33, help="frequency trials (odd, or 1)")
    ff.add_argument("--nfdot", type=int, default=17, help="frequency derivative trials (odd, or 1)")
    ff.add_argument("--ddm", type=float, default=None, help="DM step (default: one bin at the bottom of the band)")
    ff.add_argument("--dfreq", type=float, default=None, help="frequency step, Hz (default: one bin of drift over the span)")
    ff.add_argument("--dfdot", type=float, default=None, help="derivative step, Hz / s (default: one bin at the ends of the span)")
    ff.add_argument("--fit-frac", type=float, default=0.5, help="the parabola is fitted over the points at or above this fraction of the peak")
    ff.add_argument("--flag", default=None, help="flag file: channels left out")
    ff.add_argument("--polyco", default=None, help="TEMPO polyco file: fold with the predictor, report the offsets from it")
    ff.add_argument("--refold", action="store_true", help="fold once more with the refined .par (integer bin shifts cannot undo smear inside a sub-integration)")
    ff.add_argument("--products", choices=("coherency", "stokes"), default="coherency", help="what a four-product file holds")
    ff.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    d = sub.add_parser("prepdata", help="incoherent dedispersion (process_vdif.py:202-229)")
    d.add_argument("fil")
    d.add_argument("--dm", type=float, required=True)
    d.add_argument("--dm2", type=float, default=0.0)
    d.add_argument("--dmstep", type=float, default=1.0)
    d.add_argument("--nozerodm", action="store_false", help="do not subtract the zero-DM series")
    d.add_argument("--clip", type=float, default=5.0)
    d.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    q = sub.add_parser("search", help="dedisperse over a DM range and search for single pulses (what single_pulse_search.py does with the .dat files)")
    q.add_argument("fil")
    q.add_argument("--dm", type=float, required=True)
    q.add_argument("--dm2", type=float, default=0.0)
    q.add_argument("--dmstep", type=float, default=1.0)
    q.add_argument("--threshold", type=float, default=5.0, help="sigma a boxcar sum must reach")
    q.add_argument("--max-width", type=float, default=0.0, help="widest boxcar, s (0: widths up to 30 samples)")
    q.add_argument("--detrend", type=int, default=1000, help="samples per normalisation block")
    q.add_argument("--nozerodm", action="store_false", help="do not subtract the zero-DM series")
    q.add_argument("--clip", type=float, default=5.0)
    q.add_argument("--write-dat", action="store_true", help="also write the .dat / .inf files of prepdata")
    q.add_argument("--flag", default=None, help="flag file (channels to flag): the rows are cleaned before the search")
    q.add_argument("--rfi", action="store_true", help="flag interference from block statistics and clean the rows first")
    q.add_argument("--resident", action="store_true", help="flag and search in one library call on rows uploaded once")
    q.add_argument("--periodic", action="store_true", help="with --rfi: also flag cells whose power spectrum has a peak (periodic interference)")
    q.add_argument("--t-freq", type=float, default=4.0, help="threshold of --periodic, Gaussian sigma over the bins of a cell")
    q.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    b = sub.add_parser("bandsearch", help="search every contiguous range of sub-bands over a DM range for single pulses: bursts that fill only part of the band")
    b.add_argument("fil")
    b.add_argument("--dm", type=float, required=True)
    b.add_argument("--dm2", type=float, default=0.0)
    b.add_argument("--dmstep", type=float, default=1.0)
    b.add_argument("--nsub", type=int, default=8, help="equal sub-bands the band is cut into (1..16, a divisor of nchans)")
    b.add_argument("--min-sub", type=int, default=1, help="narrowest range searched, in sub-bands")
    b.add_argument("--max-sub", type=int, default=0, help="widest range searched, in sub-bands (0: the full band)")
    b.add_argument("--threshold", type=float, default=5.0, help="sigma a boxcar sum must reach")
    b.add_argument("--max-width", type=float, default=0.0, help="widest boxcar, s (0: widths up to 30 samples)")
    b.add_argument("--detrend", type=int, default=1000, help="samples per normalisation block")
    b.add_argument("--nozerodm", action="store_false", help="do not subtract the zero-DM series")
    b.add_argument("--clip", type=float, default=5.0)
    b.add_argument("--dm-gap", type=int, default=2, help="records at most this many trial DMs apart can join")
    b.add_argument("--plane-mib", type=int, default=0, help="device memory of the (DM, band) x time plane of one batch of DMs, MiB (0: 1024)")
    b.add_argument("--flag", default=None, help="flag file (channels to flag): the rows are cleaned before the search")
    b.add_argument("--rfi", action="store_true", help="flag interference from block statistics and clean the rows first")
    b.add_argument("--periodic", action="store_true", help="with --rfi: also flag cells whose power spectrum has a peak (periodic interference)")
    b.add_argument("--t-freq", type=float, default=4.0, help="threshold of --periodic, Gaussian sigma over the bins of a cell")
    b.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    z = sub.add_parser("psearch", help="dedisperse over a DM range and search every series for periodic signals (what realfft + accelsearch -zmax 0 do with the .dat files)")
    z.add_argument("fil")
    z.add_argument("--dm", type=float, required=True)
    z.add_argument("--dm2", type=float, default=0.0)
    z.add_argument("--dmstep", type=float, default=1.0)
    z.add_argument("--sigma", type=float, default=6.0, help="Gaussian sigma a harmonic sum must reach")
    z.add_argument("--nharm", type=int, default=16, help="harmonics summed at most: 1, 2, 4, 8 or 16")
    z.add_argument("--flo", type=float, default=0.5, help="lowest frequency searched, Hz")
    z.add_argument("--nfft", type=int, default=0, help="transform length, a power of two in 2^12..2^22 (0: the largest that fits the series)")
    z.add_argument("--wblock", type=int, default=128, help="bins per normalisation block, a power of two in 32..1024")
    z.add_argument("--dm-gap", type=int, default=2, help="records at most this many trial DMs apart can join")
    z.add_argument("--nozerodm", action="store_false", help="do not subtract the zero-DM series")
    z.add_argument("--clip", type=float, default=5.0)
    z.add_argument("--flag", default=None, help="flag file (channels to flag): the rows are cleaned before the search")
    z.add_argument("--rfi", action="store_true", help="flag interference from block statistics and clean the rows first")
    z.add_argument("--periodic", action="store_true", help="with --rfi: also flag cells whose power spectrum has a peak (periodic interference)")
    z.add_argument("--t-freq", type=float, default=4.0, help="threshold of --periodic, Gaussian sigma over the bins of a cell")
    z.add_argument("--max-cands", type=int, default=0, help="keep the strongest N candidates (0: all)")
    z.add_argument("--fold-best", type=int, default=0, help="fold the K strongest candidates at their frequency and DM")
    z.add_argument("--refine", action="store_true", help="with --fold-best: refine every folded candidate in DM, F0 and F1 (the outputs of `foldfit`)")
    z.add_argument("--amax", type=float, default=0.0, help="largest trial acceleration, m/s^2 (0: no acceleration search)")
    z.add_argument("--astep", type=float, default=0.0, help="step of the trial accelerations, m/s^2 (0: two bins of drift at 100 Hz)")
    z.add_argument("--acc-gap", type=int, default=1, help="records at most this many trial accelerations apart can join")
    z.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    k = sub.add_parser("candidates", help="search, group the records across DMs, cut the frequency-time and DM-time planes of every group")
    k.add_argument("fil")
    k.add_argument("--dm", type=float, required=True)
    k.add_argument("--dm2", type=float, default=0.0)
    k.add_argument("--dmstep", type=float, default=1.0)
    k.add_argument("--threshold", type=float, default=5.0, help="sigma a boxcar sum must reach")
    k.add_argument("--max-width", type=float, default=0.0, help="widest boxcar, s (0: widths up to 30 samples)")
    k.add_argument("--detrend", type=int, default=1000, help="samples per normalisation block")
    k.add_argument("--nozerodm", action="store_false", help="do not subtract the zero-DM series (search only: the planes are plain sums)")
    k.add_argument("--clip", type=float, default=5.0)
    k.add_argument("--dm-gap", type=int, default=2, help="records at most this many trial DMs apart can join")
    k.add_argument("--min-members", type=int, default=1, help="drop groups of fewer records")
    k.add_argument("--max-cands", type=int, default=0, help="keep the strongest N groups (0: all)")
    k.add_argument("--nt", type=int, default=256)
    k.add_argument("--nf", type=int, default=0, help="frequency bins (0: the largest divisor of nchans up to 256)")
    k.add_argument("--ndm", type=int, default=256)
    k.add_argument("--flag", default=None, help="flag file (channels to flag): the rows are cleaned before the search and the cut-outs")
    k.add_argument("--rfi", action="store_true", help="flag interference from block statistics and clean the rows first")
    k.add_argument("--resident", action="store_true", help="flag, search and cut in one library call on rows uploaded once")
    k.add_argument("--periodic", action="store_true", help="with --rfi: also flag cells whose power spectrum has a peak (periodic interference)")
    k.add_argument("--t-freq", type=float, default=4.0, help="threshold of --periodic, Gaussian sigma over the bins of a cell")
    k.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    r = sub.add_parser("rfifind", help="flag interference per (block of rows, channel): <base>_rfi.npz, <base>.flag, optionally <base>_clean.fil")
    r.add_argument("fil")
    r.add_argument("--block-rows", type=int, default=RFI_DEFAULTS["block_rows"], help="rows per block")
    r.add_argument("--t-cell", type=float, default=RFI_DEFAULTS["t_cell"], help="threshold of a cell's mean and std against its channel")
    r.add_argument("--t-chan", type=float, default=RFI_DEFAULTS["t_chan"], help="threshold of a channel's std against the band (0: off)")
    r.add_argument("--chan-frac", type=float, default=RFI_DEFAULTS["chan_frac"], help="flag a channel with more than this fraction of its blocks flagged")
    r.add_argument("--block-frac", type=float, default=RFI_DEFAULTS["block_frac"], help="flag a block with more than this fraction of its channels flagged")
    r.add_argument("--flag", default=None, help="flag file: channels to flag whatever the statistics say")
    r.add_argument("--write-clean", action="store_true", help="also write <base>_clean.fil")
    r.add_argument("--resident", action="store_true", help="clean all products in one library call on rows uploaded and downloaded once")
    r.add_argument("--periodic", action="store_true", help="also flag cells whose power spectrum has a peak (periodic interference); block-rows a power of two in 8..4096")
    r.add_argument("--t-freq", type=float, default=4.0, help="threshold of --periodic, Gaussian sigma over the bins of a cell")
    r.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    m = sub.add_parser("rmsynth", help="rotation measure of the bursts of a full-Stokes filterbank: spectra of every product, RM synthesis of Q and U")
    m.add_argument("fil")
    m.add_argument("--dm", type=float, action="append", default=None, help="DM of a burst (repeatable, one per burst); with --dm2: the first DM of the search")
    m.add_argument("--dm-from", default=None, help="<base>_dm.npz of `dmfit`: its bursts at their measured DMs instead of --dm .. --width")
    m.add_argument("--dm-kind", choices=("snr", "struct"), default="snr", help="which DM of --dm-from: the S/N- or the structure-maximising one")
    m.add_argument("--sample", type=int, action="append", default=None, help="centre of a burst, row at the top of the band (repeatable)")
    m.add_argument("--time", type=float, action="append", default=None, help="the same in seconds from the start of the file (repeatable)")
    m.add_argument("--width", type=int, action="append", default=None, help="on-pulse rows (repeatable; one value serves every burst)")
    m.add_argument("--dm2", type=float, default=0.0, help="search DM .. DM2 for the bursts instead (the groups of `candidates` on product 0)")
    m.add_argument("--dmstep", type=float, default=1.0)
    m.add_argument("--threshold", type=float, default=8.0, help="sigma of the search of --dm2")
    m.add_argument("--max-cands", type=int, default=8, help="bursts kept from the search of --dm2")
    m.add_argument("--off-gap", type=int, default=None, help="rows between the burst and each off-pulse window (default: 2 widths, at least 16)")
    m.add_argument("--off-len", type=int, default=None, help="rows of each off-pulse window (default 1024)")
    m.add_argument("--phi-max", type=float, default=0.0, help="largest |Faraday depth|, rad/m2 (0: sqrt(3) / the largest lambda^2 step)")
    m.add_argument("--dphi", type=float, default=0.0, help="step of the Faraday depth (0: fwhm / 8)")
    m.add_argument("--nphi", type=int, default=0, help="trials, instead of --phi-max")
    m.add_argument("--flag", default=None, help="flag file: channels left out of the transform")
    m.add_argument("--gains", default=None, help=".npy file [4][nchans] of gains that multiply the spectra")
    m.add_argument("--products", choices=("coherency", "stokes"), default="stokes", help="what the file holds: I, Q, U, V or the -d4 products")
    m.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    m.add_argument("--profile", action="store_true", help="also write each burst's polarisation profile at its fitted RM (the files of `polprof`)")
    m.add_argument("--nbin", type=int, default=256, help="bins of --profile")
    m.add_argument("--tfactor", type=int, default=1, help="rows per bin of --profile")
    m.add_argument("--polcal", default=None, help="<base>_polcal.npz of `polcal` on a calibrator: its R/L delay is taken out before the transform")
    pc = sub.add_parser("polcal", help="delay between the two circular feeds from the pulses of a calibrator of known RM: the delay x RM transform")
    pc.add_argument("fil")
    pc.add_argument("--dm", type=float, action="append", default=None, help="DM of a pulse (repeatable, one per pulse); with --dm2: the first DM of the search")
    pc.add_argument("--dm-from", default=None, help="<base>_dm.npz of `dmfit`: its bursts at their measured DMs instead of --dm .. --width")
    pc.add_argument("--dm-kind", choices=("snr", "struct"), default="snr", help="which DM of --dm-from: the S/N- or the structure-maximising one")
    pc.add_argument("--sample", type=int, action="append", default=None, help="centre of a pulse, row at the top of the band (repeatable)")
    pc.add_argument("--time", type=float, action="append", default=None, help="the same in seconds from the start of the file (repeatable)")
    pc.add_argument("--width", type=int, action="append", default=None, help="on-pulse rows (repeatable; one value serves every pulse)")
    pc.add_argument("--dm2", type=float, default=0.0, help="search DM .. DM2 for the pulses instead (the groups of `candidates` on product 0)")
    pc.add_argument("--dmstep", type=float, default=1.0)
    pc.add_argument("--threshold", type=float, default=8.0, help="sigma of the search of --dm2")
    pc.add_argument("--max-cands", type=int, default=8, help="pulses kept from the search of --dm2")
    pc.add_argument("--off-gap", type=int, default=None, help="rows between the pulse and each off-pulse window (default: 2 widths, at least 16)")
    pc.add_argument("--off-len", type=int, default=None, help="rows of each off-pulse window (default 1024)")
    pc.add_argument("--rm-known", type=float, default=None, help="the calibrator's RM, rad/m2: one RM trial")
    pc.add_argument("--rm-lo", type=float, default=None, help="or a range of RM trials: first")
    pc.add_argument("--rm-hi", type=float, default=None, help="last")
    pc.add_argument("--rm-step", type=float, default=None, help="step")
    pc.add_argument("--tau-half", type=float, default=0.0, help="delays searched either side of 0, NANOSECONDS (0: 8 fwhm_tau)")
    pc.add_argument("--dtau", type=float, default=0.0, help="step of the delay, NANOSECONDS (0: fwhm_tau / 8)")
    pc.add_argument("--flag", default=None, help="flag file: channels left out of the transform")
    pc.add_argument("--gains", default=None, help=".npy file [4][nchans] of gains that multiply the spectra")
    pc.add_argument("--products", choices=("coherency", "stokes"), default="stokes", help="what the file holds: I, Q, U, V or the -d4 products")
    pc.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    f = sub.add_parser("polprof", help="polarisation profile of the bursts of a full-Stokes filterbank: derotated I, L, V and PA per time bin")
    f.add_argument("fil")
    f.add_argument("--dm", type=float, action="append", default=None, help="DM of a burst (repeatable, one per burst)")
    f.add_argument("--sample", type=int, action="append", default=None, help="centre of a burst, row at the top of the band (repeatable)")
    f.add_argument("--time", type=float, action="append", default=None, help="the same in seconds from the start of the file (repeatable)")
    f.add_argument("--width", type=int, action="append", default=None, help="on-pulse rows (repeatable; one value serves every burst)")
    f.add_argument("--rm", type=float, action="append", default=None, help="rotation measure, rad/m2 (repeatable; one value serves every burst)")
    f.add_argument("--rm-from", default=None, help="<base>_rm.npz of `rmsynth`: its bursts and fitted RMs instead of --dm .. --rm")
    f.add_argument("--dm-from", default=None, help="<base>_dm.npz of `dmfit`: its bursts at their measured DMs instead of --dm .. --width (with --rm)")
    f.add_argument("--dm-kind", choices=("snr", "struct"), default="snr", help="which DM of --dm-from: the S/N- or the structure-maximising one")
    f.add_argument("--nbin", type=int, default=256, help="time bins (1..1024)")
    f.add_argument("--tfactor", type=int, default=1, help="rows per bin (1..512)")
    f.add_argument("--ref", choices=("mean", "zero"), default="mean", help="the PA refers to the mean lambda^2 of the used channels, or to lambda = 0")
    f.add_argument("--off-gap", type=int, default=None, help="rows between the burst and each off-pulse window (default: 2 widths, at least 16)")
    f.add_argument("--off-len", type=int, default=None, help="rows of each off-pulse window (default 1024)")
    f.add_argument("--flag", default=None, help="flag file: channels left out")
    f.add_argument("--gains", default=None, help=".npy file [4][nchans] of gains")
    f.add_argument("--coherency", action="store_true", help="the file holds the -d4 products PP, QQ, Re, Im")
    f.add_argument("--polcal", default=None, help="<base>_polcal.npz of `polcal` on a calibrator: its R/L delay is taken out with the rotation")
    f.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    d = sub.add_parser("dmfit", help="DM of the bursts of a filterbank: a fine DM scan, the S/N- and the structure-maximising DM")
    d.add_argument("fil")
    d.add_argument("--dm", type=float, action="append", required=True, help="DM of a burst (repeatable, one per burst); with --dm2: the first DM of the search")
    d.add_argument("--sample", type=int, action="append", default=None, help="centre of a burst, row at the top of the band (repeatable)")
    d.add_argument("--time", type=float, action="append", default=None, help="the same in seconds from the start of the file (repeatable)")
    d.add_argument("--width", type=int, action="append", default=None, help="on-pulse rows (repeatable; one value serves every burst)")
    d.add_argument("--dm2", type=float, default=0.0, help="search DM .. DM2 for the bursts instead (the groups of `candidates` on product 0)")
    d.add_argument("--dmstep", type=float, default=1.0)
    d.add_argument("--threshold", type=float, default=8.0, help="sigma of the search of --dm2")
    d.add_argument("--max-cands", type=int, default=8, help="bursts kept from the search of --dm2")
    d.add_argument("--dm-half", type=float, default=None, help="half range of the scan, pc cm^-3 (default: 32 DM sample steps)")
    d.add_argument("--ddm", type=float, default=None, help="step of the scan, pc cm^-3 (default: a quarter of a DM sample step)")
    d.add_argument("--nbin", type=int, default=None, help="time bins (1..1024; default: four widths plus twice the sweep of the edge trial)")
    d.add_argument("--tfactor", type=int, default=None, help="rows per bin (1..512; default: an eighth of the width)")
    d.add_argument("--smooth", type=int, default=3, help="bins the profile is smoothed over before the structure metric")
    d.add_argument("--fit-frac", type=float, default=0.5, help="the parabola is fitted to the trials above this fraction of the peak")
    d.add_argument("--off-gap", type=int, default=None, help="rows between the burst and each off-pulse window (default: 2 widths, at least 16 and the sweep)")
    d.add_argument("--off-len", type=int, default=None, help="rows of each off-pulse window (default 1024)")
    d.add_argument("--flag", default=None, help="flag file: channels left out")
    d.add_argument("--coherency", action="store_true", help="the file holds the -d4 products: PP + QQ is scanned")
    d.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    c = sub.add_parser("burstacf", help="structure of the bursts of a filterbank: dedispersed dynamic spectrum, its 2-D autocorrelation, bandwidth, duration and drift")
    c.add_argument("fil")
    c.add_argument("--dm", type=float, action="append", default=None, help="DM of a burst (repeatable, one per burst)")
    c.add_argument("--dm-from", default=None, help="<base>_dm.npz of `dmfit`: its bursts at their measured DMs instead of --dm .. --width")
    c.add_argument("--dm-kind", choices=("snr", "struct"), default="struct", help="which DM of --dm-from: the S/N- or the structure-maximising one")
    c.add_argument("--sample", type=int, action="append", default=None, help="centre of a burst, row at the top of the band (repeatable)")
    c.add_argument("--time", type=float, action="append", default=None, help="the same in seconds from the start of the file (repeatable)")
    c.add_argument("--width", type=int, action="append", default=None, help="on-pulse rows (repeatable; one value serves every burst)")
    c.add_argument("--nbin", type=int, default=256, help="time bins (1..1024)")
    c.add_argument("--tfactor", type=int, default=1, help="rows per bin (1..512)")
    c.add_argument("--ffactor", type=int, default=1, help="channels per subband (divides nchans)")
    c.add_argument("--lagf", type=int, default=None, help="frequency lags 0 .. lagf - 1, in subbands (default: half the subbands, at most 1024)")
    c.add_argument("--lagt", type=int, default=None, help="time lags -(lagt - 1) .. lagt - 1, in bins (default: half the bins, at most 256)")
    c.add_argument("--fit-frac", type=float, default=0.5, help="the drift is fitted to the lags above this fraction of the largest one")
    c.add_argument("--off-gap", type=int, default=None, help="rows between the burst and each off-pulse window (default: 2 widths, at least 16)")
    c.add_argument("--off-len", type=int, default=None, help="rows of each off-pulse window (default 1024)")
    c.add_argument("--flag", default=None, help="flag file: channels left out")
    c.add_argument("--coherency", action="store_true", help="the file holds the -d4 products: PP + QQ is used")
    c.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    c = sub.add_parser("scatter", help="scattering of the bursts of a filterbank: a bank of scattered Gaussians fitted per subband, tau(nu) across the band")
    c.add_argument("fil")
    c.add_argument("--dm", type=float, action="append", default=None, help="DM of a burst (repeatable, one per burst)")
    c.add_argument("--dm-from", default=None, help="<base>_dm.npz of `dmfit`: its bursts at their measured DMs instead of --dm .. --width")
    c.add_argument("--dm-kind", choices=("snr", "struct"), default="struct", help="which DM of --dm-from: the S/N- or the structure-maximising one")
    c.add_argument("--sample", type=int, action="append", default=None, help="centre of a burst, row at the top of the band (repeatable)")
    c.add_argument("--time", type=float, action="append", default=None, help="the same in seconds from the start of the file (repeatable)")
    c.add_argument("--width", type=int, action="append", default=None, help="on-pulse rows (repeatable; one value serves every burst)")
    c.add_argument("--nbin", type=int, default=256, help="time bins (1..1024)")
    c.add_argument("--tfactor", type=int, default=1, help="rows per bin (1..512)")
    c.add_argument("--ffactor", type=int, default=1, help="channels per subband (divides nchans)")
    c.add_argument("--sigma0", type=float, default=0.5, help="the smallest Gaussian sigma of the bank, in bins")
    c.add_argument("--nsig", type=int, default=16, help="values of sigma")
    c.add_argument("--rsig", type=float, default=2.0 ** 0.25, help="ratio of neighbouring sigmas")
    c.add_argument("--tau0", type=float, default=0.5, help="the smallest scattering time of the bank, in bins")
    c.add_argument("--ntau", type=int, default=32, help="values of tau")
    c.add_argument("--rtau", type=float, default=2.0 ** 0.25, help="ratio of neighbouring taus")
    c.add_argument("--ntap", type=int, default=256, help="taps of a template (1..1024)")
    c.add_argument("--lead", type=int, default=None, help="the tap of the Gaussian's centre (default: ntap / 4)")
    c.add_argument("--shift0", type=int, default=None, help="first trial arrival bin (default: nbin / 4)")
    c.add_argument("--nshift", type=int, default=None, help="trial arrival bins (default: nbin / 2)")
    c.add_argument("--alpha", type=float, nargs="+", default=list(SCAT_ALPHAS), help="the trial indices of tau ~ nu^-alpha (1..32 values)")
    c.add_argument("--snr-min", type=float, default=5.0, help="subbands below this S/N stay out of the band fit")
    c.add_argument("--off-gap", type=int, default=None, help="rows between the burst and each off-pulse window (default: 2 widths, at least 16)")
    c.add_argument("--off-len", type=int, default=None, help="rows of each off-pulse window (default 1024)")
    c.add_argument("--flag", default=None, help="flag file: channels left out")
    c.add_argument("--coherency", action="store_true", help="the file holds the -d4 products: PP + QQ is used")
    c.add_argument("--device", type=int, default=int(os.environ.get("FRBCH_DEVICE", "0")))
    a = ap.parse_args(argv)
    if a.cmd == "scatter":
        if a.dm_from:
            bursts = list(bursts_from_dm(a.dm_from, a.dm_kind))
        else:
            tsamp = sigproc.read_fil(a.fil).header["tsamp"]
            centres = list(a.sample or []) + [int(round(t / tsamp)) for t in (a.time or [])]
            widths, dms = a.width or [], a.dm or []
            if not centres or len(centres) != len(dms) or len(widths) not in (1, len(centres)):
                raise InputError("scatter: one --sample or --time per --dm, and --width once or once per burst (or --dm-from)")
            bursts = [(dm, s, widths[i if len(widths) > 1 else 0]) for i, (dm, s) in enumerate(zip(dms, centres))]
        bank = scat_bank_params(a.nsig, a.ntau, a.ntap, a.lead, a.sigma0, a.rsig, a.tau0, a.rtau)
        files, _sc = burstscat_fil(a.fil, bursts, nbin=a.nbin, tfactor=a.tfactor, ffactor=a.ffactor, bank=bank, shift0=a.shift0, nshift=a.nshift,
                                   alphas=a.alpha, snr_min=a.snr_min, off_gap=a.off_gap, off_len=a.off_len, flag_file=a.flag,
                                   products="coherency" if a.coherency else "stokes", device=a.device)
        for path in files:
            print("wrote", path)
        print(open(files[1]).read(), end="")
    elif a.cmd == "burstacf":
        if a.dm_from:
            bursts = list(bursts_from_dm(a.dm_from, a.dm_kind))
        else:
            tsamp = sigproc.read_fil(a.fil).header["tsamp"]
            centres = list(a.sample or []) + [int(round(t / tsamp)) for t in (a.time or [])]
            widths, dms = a.width or [], a.dm or []
            if not centres or len(centres) != len(dms) or len(widths) not in (1, len(centres)):
                raise InputError("burstacf: one --sample or --time per --dm, and --width once or once per burst (or --dm-from)")
            bursts = [(dm, s, widths[i if len(widths) > 1 else 0]) for i, (dm, s) in enumerate(zip(dms, centres))]
        files, _acf = burstacf_fil(a.fil, bursts, nbin=a.nbin, tfactor=a.tfactor, ffactor=a.ffactor, nlagf=a.lagf, nlagt=a.lagt,
                                   fit_frac=a.fit_frac, off_gap=a.off_gap, off_len=a.off_len, flag_file=a.flag,
                                   products="coherency" if a.coherency else "stokes", device=a.device)
        for path in files:
            print("wrote", path)
        print(open(files[1]).read(), end="")
    elif a.cmd == "dmfit":
        bursts = None
        if a.dm2 <= 0.0:
            tsamp = sigproc.read_fil(a.fil).header["tsamp"]
            centres = list(a.sample or []) + [int(round(t / tsamp)) for t in (a.time or [])]
            widths = a.width or []
            if not centres or len(centres) != len(a.dm) or len(widths) not in (1, len(centres)):
                raise InputError("dmfit: one --sample or --time per --dm, and --width once or once per burst")
            bursts = [(dm, s, widths[i if len(widths) > 1 else 0]) for i, (dm, s) in enumerate(zip(a.dm, centres))]
        files, _scan = dmfit_fil(a.fil, bursts, dm1=a.dm[0], dm2=a.dm2, dmstep=a.dmstep, width=(a.width or [0])[0], dm_half=a.dm_half, ddm=a.ddm,
                                 nbin=a.nbin, tfactor=a.tfactor, smooth=a.smooth, fit_frac=a.fit_frac, off_gap=a.off_gap, off_len=a.off_len,
                                 flag_file=a.flag, products="coherency" if a.coherency else "stokes", threshold=a.threshold,
                                 max_cands=a.max_cands, device=a.device)
        for path in files:
            print("wrote", path)
        print(open(files[1]).read(), end="")
    elif a.cmd == "polprof":
        bursts, rm = None, None
        if a.dm_from and not a.rm_from:
            bursts = list(bursts_from_dm(a.dm_from, a.dm_kind))
            rms = a.rm or []
            if len(rms) not in (1, len(bursts)):
                raise InputError("polprof --dm-from: --rm once or once per burst")
            rm = [rms[i if len(rms) > 1 else 0] for i in range(len(bursts))]
        elif not a.rm_from:
            tsamp = sigproc.read_fil(a.fil).header["tsamp"]
            centres = list(a.sample or []) + [int(round(t / tsamp)) for t in (a.time or [])]
            widths, rms, dms = a.width or [], a.rm or [], a.dm or []
            if not centres or len(centres) != len(dms) or len(widths) not in (1, len(centres)) or len(rms) not in (1, len(centres)):
                raise InputError("polprof: one --sample or --time per --dm, --width and --rm once or once per burst (or --rm-from)")
            bursts = [(dm, s, widths[i if len(widths) > 1 else 0]) for i, (dm, s) in enumerate(zip(dms, centres))]
            rm = [rms[i if len(rms) > 1 else 0] for i in range(len(centres))]
        files, _prof = polprof_fil(a.fil, bursts, rm=rm, nbin=a.nbin, tfactor=a.tfactor, ref=a.ref, off_gap=a.off_gap, off_len=a.off_len,
                                   flag_file=a.flag, gains=a.gains, products="coherency" if a.coherency else "stokes", rm_from=a.rm_from,
                                   device=a.device, **(dict(polcal_file=a.polcal) if a.polcal else {}))
        for path in files:
            print("wrote", path)
    elif a.cmd == "rmsynth":
        bursts = None
        if a.dm_from:
            bursts = list(bursts_from_dm(a.dm_from, a.dm_kind))
            a.dm = [float(bursts[0]["dm"])]
        elif not a.dm:
            m.error("the following arguments are required: --dm")
        elif a.dm2 <= 0.0:
            tsamp = sigproc.read_fil(a.fil).header["tsamp"]
            centres = list(a.sample or []) + [int(round(t / tsamp)) for t in (a.time or [])]
            widths = a.width or []
            if not centres or len(centres) != len(a.dm) or len(widths) not in (1, len(centres)):
                raise InputError("rmsynth: one --sample or --time per --dm, and --width once or once per burst")
            bursts = [(dm, s, widths[i if len(widths) > 1 else 0]) for i, (dm, s) in enumerate(zip(a.dm, centres))]
        files, res = rmsynth_fil(a.fil, bursts, dm1=a.dm[0], dm2=a.dm2, dmstep=a.dmstep, width=(a.width or [0])[0], off_gap=a.off_gap,
                                 off_len=a.off_len, phi_max=a.phi_max, dphi=a.dphi, nphi=a.nphi, flag_file=a.flag, gains=a.gains,
                                 products=a.products, threshold=a.threshold, max_cands=a.max_cands, device=a.device,
                                 **(dict(profile=True, nbin=a.nbin, tfactor=a.tfactor) if a.profile else {}),
                                 **(dict(polcal_file=a.polcal) if a.polcal else {}))
        for path in files:
            print("wrote", path)
        print(open(files[1]).read(), end="")
    elif a.cmd == "polcal":
        bursts = None
        if a.dm_from:
            bursts = list(bursts_from_dm(a.dm_from, a.dm_kind))
            a.dm = [float(bursts[0]["dm"])]
        elif not a.dm:
            pc.error("the following arguments are required: --dm")
        elif a.dm2 <= 0.0:
            tsamp = sigproc.read_fil(a.fil).header["tsamp"]
            centres = list(a.sample or []) + [int(round(t / tsamp)) for t in (a.time or [])]
            widths = a.width or []
            if not centres or len(centres) != len(a.dm) or len(widths) not in (1, len(centres)):
                raise InputError("polcal: one --sample or --time per --dm, and --width once or once per pulse")
            bursts = [(dm, s, widths[i if len(widths) > 1 else 0]) for i, (dm, s) in enumerate(zip(a.dm, centres))]
        files, res = polcal_fil(a.fil, bursts, dm1=a.dm[0], dm2=a.dm2, dmstep=a.dmstep, width=(a.width or [0])[0], off_gap=a.off_gap,
                                off_len=a.off_len, rm_known=a.rm_known, rm_lo=a.rm_lo, rm_hi=a.rm_hi, rm_step=a.rm_step, tau_half=a.tau_half,
                                dtau=a.dtau, flag_file=a.flag, gains=a.gains, products=a.products, threshold=a.threshold,
                                max_cands=a.max_cands, device=a.device)
        for path in files:
            print("wrote", path)
        print(open(files[1]).read(), end="")
    elif a.cmd == "rfifind":
        files, res = rfifind_fil(a.fil, block_rows=a.block_rows, t_cell=a.t_cell, t_chan=a.t_chan, chan_frac=a.chan_frac,
                                 block_frac=a.block_frac, flag_file=a.flag, write_clean=a.write_clean, device=a.device, resident=a.resident,
                                 **(dict(periodic=True, t_freq=a.t_freq) if a.periodic else {}))
        for path in files:
            print("wrote", path)
        print("{0} of {1} channels and {2} of {3} blocks flagged wholly, {4} cells masked".format(
            int(res["chan_flag"].sum()), res["chan_flag"].size, int(res["blk_flag"].sum()), res["blk_flag"].size, int(res["mask"].sum())))
    elif a.cmd == "candidates":
        files, groups = candidates_fil(a.fil, a.dm, dm2=a.dm2, dmstep=a.dmstep, zerodm=a.nozerodm, clip=a.clip, threshold=a.threshold,
                                       max_width_s=a.max_width, detrend_len=a.detrend, dm_gap=a.dm_gap, min_members=a.min_members,
                                       max_cands=a.max_cands, nt=a.nt, nf=a.nf, ndm=a.ndm, device=a.device, flag_file=a.flag,
                                       rfi=a.rfi or None, resident=a.resident,
                                       **(dict(periodic=dict(t_freq=a.t_freq)) if a.periodic else {}))
        print("wrote", a.fil.replace(".fil", "") + ".cands.txt")
        for path in files:
            print("wrote", path, "and .png")
        print("{0} candidates above {1} sigma".format(groups.size, a.threshold))
    elif a.cmd == "psearch":
        files, groups = psearch_fil(a.fil, a.dm, dm2=a.dm2, dmstep=a.dmstep, zerodm=a.nozerodm, clip=a.clip, sigma=a.sigma, nharm=a.nharm,
                                    flo=a.flo, nfft=a.nfft, wblock=a.wblock, dm_gap=a.dm_gap, max_cands=a.max_cands, fold_best=a.fold_best, refine=a.refine,
                                    device=a.device, flag_file=a.flag, rfi=a.rfi or None, amax=a.amax, astep=a.astep, acc_gap=a.acc_gap,
                                    **(dict(periodic=dict(t_freq=a.t_freq)) if a.periodic else {}))
        for path in files:
            print("wrote", path)
        print("{0} periodic candidates above {1} sigma".format(groups.size, a.sigma))
    elif a.cmd == "fold":
        if a.refine and a.doppler != 0.0:
            raise InputError("fold --refine with --doppler: the refinement folds with the F0 / F1 polynomial alone; put the Doppler factor into F0 "
                             "(F0 (1 + doppler)) or fold with a polyco")
        ar, profile = fold_fil(a.fil, a.par, nbin=a.nbin, subint_s=a.subint, fscrunch_to=a.fscrunch, device=a.device,
                               polyco=a.polyco, doppler=a.doppler, products=a.products)
        print("wrote {0}, {1}.profile.txt, {1}.png; peak bin {2} of {3}".format(ar, a.fil, int(np.argmax(profile)), profile.size))
        if a.refine:
            files, _r = foldfit_fil(a.fil, a.par, nbin=a.nbin, subint_s=a.subint, polyco=a.polyco, products=a.products, device=a.device)
            for path in files:
                print("wrote", path)
            print(open(files[1]).read(), end="")
    elif a.cmd == "foldfit":
        files, _r = foldfit_fil(a.fil, a.par, f0=a.f0, dm=a.dm, f1=a.f1, nbin=a.nbin, subint_s=a.subint, ndm=a.ndm, nfreq=a.nfreq, nfdot=a.nfdot,
                                ddm=a.ddm, dfreq=a.dfreq, dfdot=a.dfdot, fit_frac=a.fit_frac, flag_file=a.flag, polyco=a.polyco, refold=a.refold,
                                products=a.products, device=a.device)
        for path in files:
            print("wrote", path)
        print(open(files[1]).read(), end="")
    elif a.cmd == "bandsearch":
        npz, txt, cands, groups = bandsearch_fil(a.fil, a.dm, dm2=a.dm2, dmstep=a.dmstep, nsub=a.nsub, min_sub=a.min_sub, max_sub=a.max_sub,
                                                 zerodm=a.nozerodm, clip=a.clip, threshold=a.threshold, max_width_s=a.max_width,
                                                 detrend_len=a.detrend, dm_gap=a.dm_gap, plane_bytes=a.plane_mib << 20, device=a.device,
                                                 flag_file=a.flag, rfi=a.rfi or None,
                                                 **(dict(periodic=dict(t_freq=a.t_freq)) if a.periodic else {}))
        print("wrote", npz)
        print("wrote", txt)
        print("{0} records in {1} groups above {2} sigma".format(cands.size, groups.size, a.threshold))
    elif a.cmd == "search":
        files, cands = search_fil(a.fil, a.dm, dm2=a.dm2, dmstep=a.dmstep, zerodm=a.nozerodm, clip=a.clip, threshold=a.threshold,
                                  max_width_s=a.max_width, detrend_len=a.detrend, write_dat=a.write_dat, device=a.device,
                                  flag_file=a.flag, rfi=a.rfi or None, resident=a.resident,
                                  **(dict(periodic=dict(t_freq=a.t_freq)) if a.periodic else {}))
        for path in files:
            print("wrote", path)
        print("{0} candidates above {1} sigma".format(cands.size, a.threshold))
    else:
        for path in prepdata_gpu(a.fil, a.dm, zerodm=a.nozerodm, clip=a.clip, dm2=a.dm2, dmstep=a.dmstep, device=a.device):
            print("wrote", path)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
