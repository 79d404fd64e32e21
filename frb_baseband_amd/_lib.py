"""ctypes binding of the C-ABI library (include/frbch.h).

The product path is the HIP library ``csrc/libfrbch.so``.  If it is missing or cannot be loaded
this module raises -- there is no Python/CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FRBCH_LIB: another build of the same library for this process (an A/B run against another commit, tools/ab.sh); default: the product
LIB_PATH = os.environ.get("FRBCH_LIB") or os.path.join(_HERE, "csrc", "libfrbch.so")

ABI_VERSION = 5

OK, E_ARG, E_IO, E_FORMAT, E_DEVICE, E_NOMEM, E_STATE, E_CAPACITY = 0, -1, -2, -3, -4, -5, -6, -7


class FrbchConfig(C.Structure):
    _fields_ = [
        ("size", C.c_uint32), ("abi_version", C.c_uint32),
        ("freq_mhz", C.c_double), ("bw_mhz", C.c_double),
        ("start_s", C.c_double), ("total_s", C.c_double),
        ("nchan", C.c_uint32), ("freq_res", C.c_uint32), ("tscrunch", C.c_uint32),
        ("nbit_out", C.c_int32), ("pol_mode", C.c_int32), ("rescale_constant", C.c_uint32),
        ("rescale_interval_s", C.c_double), ("dm", C.c_double),
        ("coherent", C.c_uint32), ("device", C.c_int32),
        ("max_blocks_per_launch", C.c_uint32), ("flags", C.c_uint32),
        ("telescope", C.c_char * 64), ("source", C.c_char * 64),
        ("ra", C.c_char * 32), ("dec", C.c_char * 32), ("datafile", C.c_char * 512),
        ("input_bits", C.c_uint32), ("overlap", C.c_uint32),
        ("levels", C.c_float * 4),
        ("unpack_mode", C.c_uint32), ("dls_nsample", C.c_uint32),
        ("dls_cutoff_sigma", C.c_float), ("dls_threshold", C.c_float),
    ]


class FrbchInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint32), ("nchan", C.c_uint32), ("freq_res", C.c_uint32),
        ("tscrunch", C.c_uint32), ("nif", C.c_uint32),
        ("block_samples", C.c_uint64), ("block_payload_bytes", C.c_uint64),
        ("rows_per_block", C.c_uint64), ("row_bytes", C.c_uint64),
        ("rescale_interval_rows", C.c_uint64), ("rows_out", C.c_uint64),
        ("blocks_done", C.c_uint64),
        ("tsamp_s", C.c_double), ("tstart_mjd", C.c_double),
        ("fch1_mhz", C.c_double), ("foff_mhz", C.c_double),
        ("frame_bytes", C.c_uint32), ("header_bytes", C.c_uint32),
        ("have_rescale", C.c_uint32), ("diag", C.c_uint32),
        ("frames_seen", C.c_uint64), ("frames_invalid", C.c_uint64), ("frame_gaps", C.c_uint64),
        ("block_stride_bytes", C.c_uint64), ("nfilt_pos", C.c_uint32), ("nfilt_neg", C.c_uint32),
        ("frames_filled", C.c_uint64),
    ]


class FrbchFilDesc(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nchan", C.c_uint32), ("nifs", C.c_uint32), ("nbits", C.c_int32),
                ("product", C.c_uint32), ("reserved", C.c_uint32),
                ("fch1_mhz", C.c_double), ("foff_mhz", C.c_double), ("tsamp_s", C.c_double), ("tstart_mjd", C.c_double)]


class FrbchPolycoSeg(C.Structure):
    _fields_ = [("tmid_mjd", C.c_double), ("rphase_frac", C.c_double), ("f0_hz", C.c_double), ("span_min", C.c_double),
                ("ncoeff", C.c_uint32), ("reserved", C.c_uint32), ("coeff", C.c_double * 15)]


class FrbchFoldModel(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nseg", C.c_uint32), ("seg", C.POINTER(FrbchPolycoSeg)),
                ("f0_hz", C.c_double), ("f1", C.c_double), ("pepoch_mjd", C.c_double), ("doppler", C.c_double),
                ("dm", C.c_double), ("apply_delays", C.c_uint32), ("nbin", C.c_uint32), ("subint_s", C.c_double)]


class FrbchFoldfitParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nbin", C.c_uint32), ("nsub", C.c_uint32), ("products", C.c_uint32), ("ndm", C.c_uint32),
                ("nfreq", C.c_uint32), ("nfdot", C.c_uint32), ("nwidth", C.c_uint32), ("f0_fold", C.c_double), ("subint_s", C.c_double),
                ("dm0", C.c_double), ("ddm", C.c_double), ("dfreq", C.c_double), ("dfdot", C.c_double), ("fit_frac", C.c_double),
                ("widths", C.c_uint32 * 8)]


class FrbchSpParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nwidth", C.c_uint32), ("widths", C.c_uint32 * 16), ("detrend_len", C.c_uint32),
                ("reserved", C.c_uint32), ("threshold", C.c_double)]


class FrbchSpCand(C.Structure):
    _fields_ = [("dm_index", C.c_uint32), ("width", C.c_uint32), ("sample", C.c_uint64), ("sigma", C.c_float),
                ("reserved", C.c_uint32)]


class FrbchSpGroup(C.Structure):
    _fields_ = [("best", FrbchSpCand), ("nmember", C.c_uint32), ("dm_index_lo", C.c_uint32), ("dm_index_hi", C.c_uint32),
                ("reserved", C.c_uint32), ("sample_lo", C.c_uint64), ("sample_hi", C.c_uint64)]


class FrbchBandParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nsub", C.c_uint32), ("min_sub", C.c_uint32), ("max_sub", C.c_uint32)]


class FrbchSpbCand(C.Structure):
    _fields_ = [("dm_index", C.c_uint32), ("width", C.c_uint32), ("sample", C.c_uint64), ("sigma", C.c_float),
                ("sub_lo", C.c_uint16), ("sub_hi", C.c_uint16)]


class FrbchSpbGroup(C.Structure):
    _fields_ = [("best", FrbchSpbCand), ("nmember", C.c_uint32), ("dm_index_lo", C.c_uint32), ("dm_index_hi", C.c_uint32),
                ("sub_lo_min", C.c_uint16), ("sub_hi_max", C.c_uint16), ("sample_lo", C.c_uint64), ("sample_hi", C.c_uint64),
                ("full_sigma", C.c_float), ("reserved", C.c_uint32)]


class FrbchPsParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nfft", C.c_uint32), ("nharm", C.c_uint32), ("wblock", C.c_uint32),
                ("sigma", C.c_double), ("flo_hz", C.c_double), ("tsamp_s", C.c_double)]


class FrbchPsCand(C.Structure):
    _fields_ = [("dm_index", C.c_uint32), ("h", C.c_uint32), ("k", C.c_uint32), ("power", C.c_float),
                ("sigma", C.c_double), ("freq_hz", C.c_double)]


class FrbchPsGroup(C.Structure):
    _fields_ = [("best", FrbchPsCand), ("nmember", C.c_uint32), ("dm_index_lo", C.c_uint32), ("dm_index_hi", C.c_uint32),
                ("reserved", C.c_uint32)]


class FrbchPaCand(C.Structure):
    _fields_ = [("dm_index", C.c_uint32), ("acc_index", C.c_uint32), ("h", C.c_uint32), ("k", C.c_uint32), ("power", C.c_float),
                ("reserved", C.c_uint32), ("sigma", C.c_double), ("freq_hz", C.c_double), ("acc_ms2", C.c_double)]


class FrbchPaGroup(C.Structure):
    _fields_ = [("best", FrbchPaCand), ("nmember", C.c_uint32), ("dm_index_lo", C.c_uint32), ("dm_index_hi", C.c_uint32),
                ("acc_index_lo", C.c_uint32), ("acc_index_hi", C.c_uint32), ("reserved", C.c_uint32)]


class FrbchCutoutParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nt", C.c_uint32), ("nf", C.c_uint32), ("ndm", C.c_uint32)]


class FrbchCutoutCand(C.Structure):
    _fields_ = [("dm", C.c_double), ("dm_lo", C.c_double), ("dm_hi", C.c_double), ("sample", C.c_int64),
                ("tfactor", C.c_uint32), ("reserved", C.c_uint32)]


BURST_STOKES, BURST_COHERENCY = 0, 1


class FrbchBurstParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("products", C.c_uint32)]


class FrbchBurstCand(C.Structure):
    _fields_ = [("dm", C.c_double), ("sample", C.c_int64), ("width", C.c_uint32), ("off_gap", C.c_uint32),
                ("off_len", C.c_uint32), ("reserved", C.c_uint32)]


class FrbchBurstSums(C.Structure):
    _fields_ = [("on_sum", C.c_double), ("off_sum", C.c_double), ("off_sumsq", C.c_double), ("on_hits", C.c_uint32),
                ("off_hits", C.c_uint32)]


class FrbchRmParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nphi", C.c_uint32), ("phi_lo", C.c_double), ("dphi", C.c_double)]


class FrbchRmResult(C.Structure):
    _fields_ = [("rm", C.c_double), ("rm_err", C.c_double), ("peak", C.c_double), ("pa0", C.c_double), ("snr", C.c_double),
                ("sigma_f", C.c_double), ("fwhm", C.c_double), ("kpeak", C.c_uint32), ("nused", C.c_uint32),
                ("fitted", C.c_uint32), ("reserved", C.c_uint32)]


class FrbchRmdParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nphi", C.c_uint32), ("ntau", C.c_uint32), ("reserved", C.c_uint32), ("phi_lo", C.c_double),
                ("dphi", C.c_double), ("tau_lo", C.c_double), ("dtau", C.c_double)]


class FrbchRmdResult(C.Structure):
    _fields_ = [("tau", C.c_double), ("tau_err", C.c_double), ("rm", C.c_double), ("rm_err", C.c_double), ("peak", C.c_double),
                ("psi", C.c_double), ("snr", C.c_double), ("sigma_f", C.c_double), ("fwhm", C.c_double), ("fwhm_tau", C.c_double),
                ("ridge_slope", C.c_double), ("mpeak", C.c_uint32), ("kpeak", C.c_uint32), ("nused", C.c_uint32),
                ("fitted_tau", C.c_uint32), ("fitted_rm", C.c_uint32), ("nridge", C.c_uint32)]


PROF_REF_MEAN, PROF_REF_ZERO = 0, 1


class FrbchProfParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nbin", C.c_uint32), ("tfactor", C.c_uint32), ("ref", C.c_uint32), ("reserved", C.c_uint32)]


class FrbchProfBin(C.Structure):
    _fields_ = [("i", C.c_double), ("q", C.c_double), ("u", C.c_double), ("v", C.c_double), ("l", C.c_double), ("l_db", C.c_double),
                ("pa", C.c_double), ("pa_err", C.c_double), ("hits", C.c_uint32), ("pa_valid", C.c_uint32)]


class FrbchProfResult(C.Structure):
    _fields_ = [("sigma_i", C.c_double), ("sigma_q", C.c_double), ("sigma_u", C.c_double), ("sigma_v", C.c_double),
                ("sigma_l", C.c_double), ("lref", C.c_double), ("k", C.c_int32), ("nused", C.c_uint32), ("on_lo_bin", C.c_uint32),
                ("on_hi_bin", C.c_uint32)]


class FrbchDmscanParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("ntrial", C.c_uint32), ("nbin", C.c_uint32), ("tfactor", C.c_uint32), ("ddm", C.c_double)]


class FrbchDmscanPeakParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nwidth", C.c_uint32), ("widths", C.c_uint32 * 16), ("smooth", C.c_uint32),
                ("reserved", C.c_uint32), ("fit_frac", C.c_double)]


class FrbchDmscanResult(C.Structure):
    _fields_ = [("dm_snr", C.c_double), ("dm_snr_err", C.c_double), ("dm_struct", C.c_double), ("snr_peak", C.c_double),
                ("struct_peak", C.c_double), ("snr_at_struct", C.c_double), ("k_snr", C.c_uint32), ("width_snr", C.c_uint32),
                ("bin_snr", C.c_uint32), ("nfit_snr", C.c_uint32), ("fitted_snr", C.c_uint32), ("k_struct", C.c_uint32),
                ("width_struct", C.c_uint32), ("bin_struct", C.c_uint32), ("nfit_struct", C.c_uint32), ("fitted_struct", C.c_uint32),
                ("k", C.c_int32), ("nused", C.c_uint32)]


class FrbchAcfParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nbin", C.c_uint32), ("tfactor", C.c_uint32), ("ffactor", C.c_uint32), ("nlagf", C.c_uint32),
                ("nlagt", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class FrbchAcfFitParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32), ("fit_frac", C.c_double)]


class FrbchAcfResult(C.Structure):
    _fields_ = [("width_f_mhz", C.c_double), ("width_t_ms", C.c_double), ("dt_df", C.c_double), ("drift", C.c_double),
                ("ref", C.c_double), ("mff", C.c_double), ("mtf", C.c_double), ("mtt", C.c_double), ("k", C.c_int32),
                ("r", C.c_uint32), ("nused", C.c_uint32), ("ncomplete", C.c_uint32), ("fitted_f", C.c_uint32),
                ("fitted_t", C.c_uint32), ("fitted_d", C.c_uint32), ("reserved", C.c_uint32)]


ACF_PLAN, ACF_GENERIC = 0, 1


class FrbchScatBankParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nsig", C.c_uint32), ("ntau", C.c_uint32), ("ntap", C.c_uint32), ("lead", C.c_uint32),
                ("reserved", C.c_uint32 * 3), ("sigma0", C.c_double), ("rsig", C.c_double), ("tau0", C.c_double), ("rtau", C.c_double)]


class FrbchTbankShape(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nsub", C.c_uint32), ("nbin", C.c_uint32), ("ntemp", C.c_uint32), ("ntap", C.c_uint32),
                ("lead", C.c_uint32), ("shift0", C.c_uint32), ("nshift", C.c_uint32)]


class FrbchScatParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nbin", C.c_uint32), ("tfactor", C.c_uint32), ("ffactor", C.c_uint32), ("shift0", C.c_uint32),
                ("nshift", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class FrbchScatFitParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nalpha", C.c_uint32), ("snr_min", C.c_double), ("alpha", C.c_double * 32)]


TBANK_PLAN, TBANK_GENERIC = 0, 1


class FrbchRfiParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("block_rows", C.c_uint32), ("t_cell", C.c_double), ("t_chan", C.c_double),
                ("chan_frac", C.c_double), ("block_frac", C.c_double)]


class FrbchRfiFparams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32), ("t_pow", C.c_double), ("chan_frac", C.c_double)]


class FrbchRfiPeak(C.Structure):
    _fields_ = [("num", C.c_float), ("k", C.c_uint32)]


CAND_RFI, CAND_SERIES = 1, 2
CAND_STAGES = ("upload", "flag", "dedisperse", "search", "cut", "download")      # FRBCH_CAND_T_*


class FrbchCandParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("rfi", FrbchRfiParams), ("zap", C.c_void_p),
                ("zerodm", C.c_uint32), ("reserved", C.c_uint32), ("clip_sigma", C.c_double), ("sp", FrbchSpParams),
                ("dm_gap", C.c_uint32), ("min_members", C.c_uint32), ("max_cands", C.c_uint32), ("reserved2", C.c_uint32),
                ("cut", FrbchCutoutParams), ("dm_span", C.c_double)]


class FrbchCandView(C.Structure):
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32), ("nout", C.c_uint64), ("nclipped", C.c_uint64),
                ("ncand", C.c_uint64), ("cands", C.c_void_p), ("ngroup_all", C.c_uint64), ("ngroup", C.c_uint64),
                ("groups", C.c_void_p), ("cut_cands", C.c_void_p), ("ft", C.c_void_p), ("ft_hits", C.c_void_p),
                ("dt", C.c_void_p), ("dt_hits", C.c_void_p), ("nblk", C.c_uint32), ("reserved2", C.c_uint32),
                ("mask", C.c_void_p), ("repl", C.c_void_p), ("chan_flag", C.c_void_p), ("blk_flag", C.c_void_p),
                ("series", C.c_void_p), ("kernel_used", C.c_uint32 * 4), ("cutout_calls", C.c_uint32),
                ("row_uploads", C.c_uint32), ("wall_ms", C.c_double * 6), ("device_ms", C.c_double * 6)]


class _KTiming(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double),
                ("algorithmic_bytes", C.c_double)]


class FrbchTiming(C.Structure):
    _fields_ = [("size", C.c_uint32), ("nkernels", C.c_uint32), ("k", _KTiming * 12)]


# every symbol include/frbch.h declares: (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "frbch_config_init": (C.c_int, [C.POINTER(FrbchConfig)]),
    "frbch_config_from_hdr": (C.c_int, [C.c_char_p, C.POINTER(FrbchConfig)]),
    "frbch_parse_digifil_argv": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(FrbchConfig),
                                           C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t,
                                           C.c_char_p, C.c_size_t]),
    "frbch_open": (C.c_int, [C.POINTER(FrbchConfig), C.POINTER(_P)]),
    "frbch_close": (None, [_P]),
    "frbch_last_error": (C.c_char_p, [_P]),
    "frbch_strerror": (C.c_char_p, [C.c_int]),
    "frbch_get_info": (C.c_int, [_P, C.POINTER(FrbchInfo)]),
    "frbch_reset": (C.c_int, [_P]),
    "frbch_run_file": (C.c_int, [_P, C.c_char_p, C.c_char_p]),
    "frbch_run_scan": (C.c_int, [C.POINTER(_P), C.c_uint32, C.POINTER(C.c_char_p), C.c_char_p]),
    "frbch_scan_device": (C.c_int, [C.POINTER(_P), C.c_uint32, C.POINTER(_P), C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64,
                                    C.c_uint64, C.c_int, _P, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64), _P]),
    "frbch_push": (C.c_int, [_P, _P, C.c_size_t]),
    "frbch_flush": (C.c_int, [_P]),
    "frbch_pull": (C.c_long, [_P, _P, C.c_size_t]),
    "frbch_sigproc_header": (C.c_long, [_P, _P, C.c_size_t]),
    "frbch_process_device": (C.c_int, [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64,
                                       C.c_uint64, _P, C.c_size_t, C.POINTER(C.c_uint64), _P]),
    "frbch_flush_device": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_uint64), _P]),
    "frbch_power_device": (C.c_int, [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64,
                                     C.c_uint64, _P, C.c_size_t, _P]),
    "frbch_unpack_device": (C.c_int, [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int,
                                      _P, C.c_size_t, _P]),
    "frbch_get_rescale": (C.c_int, [_P, _P, _P]),
    "frbch_set_rescale": (C.c_int, [_P, _P, _P]),
    "frbch_dedisperse_nout": (C.c_long, [C.POINTER(FrbchFilDesc), C.c_uint64, _P, C.c_uint32]),
    "frbch_dedisperse_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32]),
    "frbch_dedisperse_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_double,
                                        C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    "frbch_dedisperse_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_double,
                                          C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    "frbch_fold_nsub": (C.c_long, [C.POINTER(FrbchFilDesc), C.c_uint64, C.c_double]),
    "frbch_fold_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double,
                                  C.c_uint32, C.c_uint32, C.c_double, C.c_int, _P, _P, C.c_uint32, C.c_char_p, C.c_size_t]),
    "frbch_fold_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double,
                                    C.c_uint32, C.c_uint32, C.c_double, C.c_int, _P, _P, C.c_uint32, C.c_char_p, C.c_size_t]),
    "frbch_foldp_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchFoldModel), C.c_int, _P, _P,
                                   C.c_uint32, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_foldp_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchFoldModel), C.c_int, _P, _P,
                                     C.c_uint32, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_foldfit_steps": (C.c_int, [C.POINTER(FrbchFilDesc), C.c_uint64, C.c_uint32, C.c_double, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "frbch_foldfit_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), C.c_uint64, C.POINTER(FrbchFoldfitParams), _P, _P, C.POINTER(C.c_uint32)]),
    "frbch_foldfit_device": (C.c_int, [C.POINTER(FrbchFilDesc), C.c_uint64, C.POINTER(FrbchFoldfitParams), _P, _P, _P, C.c_int, _P, _P, _P,
                                       _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_foldfit_host": (C.c_int, [C.POINTER(FrbchFilDesc), C.c_uint64, C.POINTER(FrbchFoldfitParams), _P, _P, _P, C.c_int, _P, _P, _P,
                                     _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_foldfit_peaks": (C.c_int, [C.POINTER(FrbchFoldfitParams), _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_fold_refine_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchFoldModel), C.POINTER(FrbchFoldfitParams),
                                           _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_fold_refine_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchFoldModel), C.POINTER(FrbchFoldfitParams),
                                         _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_spsearch_host": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.POINTER(FrbchSpParams), C.c_int, _P, C.c_uint64,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_spsearch_device": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.POINTER(FrbchSpParams), C.c_int, _P, C.c_uint64,
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_dedisperse_search_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_double,
                                               C.POINTER(FrbchSpParams), C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64), _P,
                                               C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_psearch_nfft": (C.c_long, [C.c_uint64, C.POINTER(FrbchPsParams)]),
    "frbch_psearch_thresholds": (C.c_int, [C.c_double, _P]),
    "frbch_psearch_kernel": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.POINTER(FrbchPsParams), C.POINTER(C.c_uint32)]),
    "frbch_psearch_device": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.POINTER(FrbchPsParams), C.c_int, _P, C.c_uint64,
                                       C.POINTER(C.c_uint64), _P, C.c_char_p, C.c_size_t]),
    "frbch_psearch_host": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.POINTER(FrbchPsParams), C.c_int, _P, C.c_uint64,
                                     C.POINTER(C.c_uint64), _P, C.c_char_p, C.c_size_t]),
    "frbch_dedisperse_psearch_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_double,
                                                C.POINTER(FrbchPsParams), C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64), _P,
                                                C.c_uint64, C.POINTER(C.c_uint64), _P, C.c_char_p, C.c_size_t]),
    "frbch_psearch_sift": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_double, _P, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p,
                                     C.c_size_t]),
    "frbch_ps_group_cands": (C.c_int, [_P, C.c_uint64, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    "frbch_resample_kernel": (C.c_int, [_P, C.c_uint64, _P]),
    "frbch_resample_device": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.c_uint32, C.c_double, _P, C.c_uint32, C.c_int, _P, _P,
                                        C.c_char_p, C.c_size_t]),
    "frbch_resample_host": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.c_uint32, C.c_double, _P, C.c_uint32, C.c_int, _P, _P,
                                      C.c_char_p, C.c_size_t]),
    "frbch_pasearch_plan": (C.c_int, [C.c_uint32, C.c_uint64, C.POINTER(FrbchPsParams), C.c_uint32, C.c_uint32,
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                      C.c_char_p, C.c_size_t]),
    "frbch_pasearch_device": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.POINTER(FrbchPsParams), _P, C.c_uint32, C.c_uint32, C.c_int,
                                        _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.c_char_p, C.c_size_t]),
    "frbch_pasearch_host": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.POINTER(FrbchPsParams), _P, C.c_uint32, C.c_uint32, C.c_int,
                                      _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.c_char_p, C.c_size_t]),
    "frbch_dedisperse_pasearch_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_double,
                                                 C.POINTER(FrbchPsParams), _P, C.c_uint32, C.c_uint32, C.c_int, _P, C.c_uint64,
                                                 C.POINTER(C.c_uint64), _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.c_char_p,
                                                 C.c_size_t]),
    "frbch_pa_group_cands": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p,
                                       C.c_size_t]),
    "frbch_sp_group_cands": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint32, _P, C.c_uint64, C.c_uint32, _P, C.c_uint64,
                                       C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    "frbch_band_list": (C.c_int, [C.c_uint32, C.POINTER(FrbchBandParams), _P, _P, C.c_uint32, C.POINTER(C.c_uint32), C.c_char_p,
                                  C.c_size_t]),
    "frbch_dedisperse_bands_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.POINTER(FrbchBandParams)]),
    "frbch_dedisperse_bands_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_double,
                                                C.POINTER(FrbchBandParams), C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64),
                                                C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_dedisperse_bands_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_double,
                                              C.POINTER(FrbchBandParams), C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_bandsearch_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_double,
                                          C.POINTER(FrbchBandParams), C.POINTER(FrbchSpParams), C.c_uint64, C.c_int, C.c_uint64,
                                          C.POINTER(C.c_uint64), _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.POINTER(C.c_uint32),
                                          _P, C.c_char_p, C.c_size_t]),
    "frbch_bandsearch_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_double,
                                        C.POINTER(FrbchBandParams), C.POINTER(FrbchSpParams), C.c_uint64, C.c_int, C.c_uint64,
                                        C.POINTER(C.c_uint64), _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.POINTER(C.c_uint32),
                                        _P, C.c_char_p, C.c_size_t]),
    "frbch_spb_group_cands": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.c_uint32, _P,
                                        C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    "frbch_cutout_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchCutoutParams), _P, C.c_uint32, C.c_int,
                                      _P, _P, _P, _P, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_cutout_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchCutoutParams), _P, C.c_uint32, C.c_int,
                                    _P, _P, _P, _P, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_cutout_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchCutoutParams), _P, C.c_uint32]),
    "frbch_burstspec_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32]),
    "frbch_burstspec_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P,
                                         C.c_int, _P, _P, _P, _P, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_burstspec_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P,
                                       C.c_int, _P, _P, _P, _P, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_rm_table": (C.c_int, [_P]),
    "frbch_rmsynth_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint32, C.POINTER(FrbchRmParams), C.POINTER(C.c_uint32)]),
    "frbch_rmsynth_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, _P, _P, C.c_uint32, C.POINTER(FrbchRmParams), C.c_int, _P, _P,
                                       C.c_char_p, C.c_size_t]),
    "frbch_rmsynth_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, _P, _P, C.c_uint32, C.POINTER(FrbchRmParams), C.c_int, _P, _P,
                                     C.c_char_p, C.c_size_t]),
    "frbch_rm_peaks": (C.c_int, [C.POINTER(FrbchFilDesc), _P, _P, _P, _P, C.c_uint32, C.POINTER(FrbchRmParams), _P, C.c_char_p,
                                 C.c_size_t]),
    "frbch_burst_rm_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P, _P,
                                        C.POINTER(FrbchRmParams), C.c_int, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_burst_rm_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P, _P,
                                      C.POINTER(FrbchRmParams), C.c_int, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_rmdelay_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint32, C.POINTER(FrbchRmdParams), C.POINTER(C.c_uint32)]),
    "frbch_rmdelay_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, _P, _P, C.c_uint32, C.POINTER(FrbchRmdParams), C.c_int, _P, _P,
                                       C.c_char_p, C.c_size_t]),
    "frbch_rmdelay_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, _P, _P, C.c_uint32, C.POINTER(FrbchRmdParams), C.c_int, _P, _P,
                                     C.c_char_p, C.c_size_t]),
    "frbch_rmdelay_peaks": (C.c_int, [C.POINTER(FrbchFilDesc), _P, _P, _P, _P, C.c_uint32, C.POINTER(FrbchRmdParams), _P, C.c_char_p,
                                      C.c_size_t]),
    "frbch_burst_polcal_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P, _P,
                                            C.POINTER(FrbchRmdParams), C.c_int, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_burst_polcal_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P, _P,
                                          C.POINTER(FrbchRmdParams), C.c_int, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_polprof_cal_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P, _P, _P,
                                           _P, C.POINTER(FrbchProfParams), C.c_int, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_polprof_cal_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P, _P, _P,
                                         _P, C.POINTER(FrbchProfParams), C.c_int, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_polprof_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32,
                                       C.POINTER(FrbchProfParams)]),
    "frbch_polprof_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P, _P, _P,
                                       C.POINTER(FrbchProfParams), C.c_int, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_polprof_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P, _P, _P,
                                     C.POINTER(FrbchProfParams), C.c_int, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_dm_sample_step": (C.c_double, [C.POINTER(FrbchFilDesc)]),
    "frbch_dmscan_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32,
                                      C.POINTER(FrbchDmscanParams)]),
    "frbch_dmscan_peaks": (C.c_int, [C.POINTER(FrbchDmscanParams), C.POINTER(FrbchDmscanPeakParams), _P, C.c_uint32, _P, _P, _P, _P, _P, _P,
                                     _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_dmscan_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P,
                                      C.POINTER(FrbchDmscanParams), C.POINTER(FrbchDmscanPeakParams), C.c_int, _P, _P, _P, _P, _P, _P, _P,
                                      C.c_char_p, C.c_size_t]),
    "frbch_dmscan_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P,
                                    C.POINTER(FrbchDmscanParams), C.POINTER(FrbchDmscanPeakParams), C.c_int, _P, _P, _P, _P, _P, _P, _P,
                                    C.c_char_p, C.c_size_t]),
    "frbch_acf2d_kernel": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "frbch_acf2d_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _P,
                                     C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_acf2d_host": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _P,
                                   C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_burstacf_fit": (C.c_int, [C.POINTER(FrbchFilDesc), C.POINTER(FrbchAcfParams), C.POINTER(FrbchAcfFitParams), C.c_uint32, _P, _P,
                                     _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_burstacf_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32,
                                        C.POINTER(FrbchAcfParams), _P]),
    "frbch_burstacf_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P,
                                        C.POINTER(FrbchAcfParams), C.POINTER(FrbchAcfFitParams), C.c_int, _P, _P, _P, _P, _P, _P, _P,
                                        C.c_char_p, C.c_size_t]),
    "frbch_burstacf_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P,
                                      C.POINTER(FrbchAcfParams), C.POINTER(FrbchAcfFitParams), C.c_int, _P, _P, _P, _P, _P, _P, _P,
                                      C.c_char_p, C.c_size_t]),
    "frbch_scat_bank": (C.c_int, [C.POINTER(FrbchScatBankParams), _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_tbank_kernel": (C.c_int, [C.c_uint32, C.POINTER(FrbchTbankShape), C.c_uint32]),
    "frbch_tbank_device": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(FrbchTbankShape), C.c_uint32, C.c_int, _P, C.POINTER(C.c_uint32),
                                     C.c_char_p, C.c_size_t]),
    "frbch_tbank_host": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(FrbchTbankShape), C.c_uint32, C.c_int, _P, C.POINTER(C.c_uint32),
                                   C.c_char_p, C.c_size_t]),
    "frbch_burstscat_fit": (C.c_int, [C.POINTER(FrbchFilDesc), C.POINTER(FrbchScatParams), C.POINTER(FrbchScatBankParams),
                                      C.POINTER(FrbchScatFitParams), C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_burstscat_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32,
                                         C.POINTER(FrbchScatParams), C.POINTER(FrbchScatBankParams), _P]),
    "frbch_burstscat_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P,
                                         C.POINTER(FrbchScatParams), C.POINTER(FrbchScatBankParams), C.POINTER(FrbchScatFitParams), C.c_int,
                                         _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_burstscat_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchBurstParams), _P, C.c_uint32, _P,
                                       C.POINTER(FrbchScatParams), C.POINTER(FrbchScatBankParams), C.POINTER(FrbchScatFitParams), C.c_int,
                                       _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_rfi_nblk": (C.c_long, [C.c_uint64, C.c_uint32]),
    "frbch_rfi_stats_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams)]),
    "frbch_rfi_stats_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), C.c_int, _P,
                                         C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_rfi_stats_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), C.c_int, _P,
                                       C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_rfi_mask": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint32, C.c_uint64, C.POINTER(FrbchRfiParams), _P, _P, _P, _P, _P,
                                 _P, C.c_char_p, C.c_size_t]),
    "frbch_rfi_apply_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), _P, _P, C.c_int,
                                         C.c_char_p, C.c_size_t]),
    "frbch_rfi_apply_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), _P, _P, C.c_int,
                                       C.c_char_p, C.c_size_t]),
    "frbch_rfi_clean_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), _P, C.c_int, _P, _P, _P,
                                         _P, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_rfi_clean_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), _P, C.c_int, _P, _P, _P,
                                       _P, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_rfi_cleanp_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), _P, C.c_int, _P, _P, _P,
                                          _P, _P, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_rfi_cleanp_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), _P, C.c_int, _P, _P, _P,
                                        _P, _P, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_rfi_peaks_kernel": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams)]),
    "frbch_rfi_peaks_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), C.c_int, _P, _P,
                                         C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_rfi_peaks_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), C.c_int, _P, _P,
                                       C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_rfi_periodic": (C.c_int, [C.POINTER(FrbchFilDesc), _P, _P, C.c_uint32, C.c_uint64, C.POINTER(FrbchRfiParams),
                                     C.POINTER(FrbchRfiFparams), _P, _P, _P, C.c_char_p, C.c_size_t]),
    "frbch_rfi_cleanf_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), C.POINTER(FrbchRfiFparams),
                                          _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_rfi_cleanf_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, C.POINTER(FrbchRfiParams), C.POINTER(FrbchRfiFparams),
                                        _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_candidates_host": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.POINTER(FrbchCandParams), C.c_int,
                                        C.POINTER(_P), C.c_char_p, C.c_size_t]),
    "frbch_candidates_device": (C.c_int, [C.POINTER(FrbchFilDesc), _P, C.c_uint64, _P, C.c_uint32, C.POINTER(FrbchCandParams), C.c_int,
                                          C.POINTER(_P), C.c_char_p, C.c_size_t]),
    "frbch_cand_result_view": (C.c_int, [_P, C.POINTER(FrbchCandView)]),
    "frbch_cand_result_free": (None, [_P]),
    "frbch_cand_select": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "frbch_cornerturn_info": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "frbch_cornerturn_host": (C.c_int, [C.c_char_p, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(_P), C.c_uint32,
                                        C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]),
    "frbch_cornerturn_device": (C.c_int, [C.c_char_p, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(_P), C.c_uint32,
                                          C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]),
    "frbch_set_profiling": (C.c_int, [_P, C.c_int]),
    "frbch_timing_reset": (C.c_int, [_P]),
    "frbch_get_timing": (C.c_int, [_P, C.POINTER(FrbchTiming)]),
    "frbch_get_launch_record": (C.c_long, [_P, C.c_char_p, C.c_size_t]),
    "frbch_version": (C.c_char_p, []),
}

_cache: dict = {}


class LibraryMissing(RuntimeError):
    pass


def load(path: str | None = None) -> C.CDLL:
    """Load the C-ABI library and bind every declared symbol.  Raises LibraryMissing loudly."""
    path = path or LIB_PATH
    if path in _cache:
        return _cache[path]
    if not os.path.exists(path):
        raise LibraryMissing(
            f"{path} not found: build the HIP extension first (python -c 'import __graft_entry__ as "
            f"g; g.build()' or make -C frb_baseband_amd/csrc).  There is no CPU fallback.")
    try:
        lib = C.CDLL(path)
    except OSError as exc:  # missing libamdhip64 etc.
        raise LibraryMissing(f"cannot load {path}: {exc}.  There is no CPU fallback.") from exc
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _cache[path] = lib
    return lib
