/* frbch.h -- C ABI of the MI355X VDIF -> SIGPROC-filterbank channeliser.
 *
 * Drop-in boundary.  The reference (pharaofranz/frb-baseband) has no FFI for this path: the
 * boundary is a subprocess plus two files -- process_vdif.py:157-182 builds a `digifil` argv,
 * :191 launches it, the input is the `.hdr` written by make_hdr (:115-139) whose DATAFILE is the
 * per-IF VDIF, the output is the SIGPROC `.fil` named at :143-145 (possibly a FIFO,
 * base2fil.sh:348-350).  Each entry point below cites the piece of that interface it replaces.
 * Plain pointers and sizes only; no C++/torch types.  Handles are single-threaded, one per IF
 * (base2fil.sh:60-66 runs one process per IF).  The library never calls exit().
 *
 * There is NO CPU fallback: every compute entry point needs a gfx950 device and fails with
 * FRBCH_E_DEVICE otherwise.
 */
#ifndef FRBCH_H
#define FRBCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRBCH_ABI_VERSION 5

/* error codes (negative); 0 = ok.  process_vdif.py:193-198 turns a non-zero digifil exit status
 * into RunError; the CLI shim maps any of these to exit status 1 with frbch_strerror on stderr. */
enum {
  FRBCH_OK = 0,
  FRBCH_E_ARG = -1,      /* bad argument / unsupported configuration (InputError territory)   */
  FRBCH_E_IO = -2,       /* open/read/write failure                                           */
  FRBCH_E_FORMAT = -3,   /* not the VDIF / .hdr we understand                                 */
  FRBCH_E_DEVICE = -4,   /* no usable GPU, HIP error                                          */
  FRBCH_E_NOMEM = -5,
  FRBCH_E_STATE = -6,    /* call sequence error (e.g. pull before any push)                   */
  FRBCH_E_CAPACITY = -7  /* caller buffer too small                                           */
};

/* pol_mode: what run_digifil maps --pol to (process_vdif.py:163-176):
 *   0,1 -> -P0/-P1 single polarisation power; 2 -> -d1 PP+QQ; 3 -> -d3 (PP+QQ)^2;
 *   4 -> -d4 PP,QQ,Re(PQ*),Im(PQ*)  (help text :58-64; base2fil.sh:214-217);
 *   5 -> Stokes I,Q,U,V formed from the -d4 products for the circular feeds make_hdr declares ("BASIS Circular",
 *        process_vdif.py:131): I = PP+QQ, Q = 2 Re(PQ*), U = 2 Im(PQ*), V = PP-QQ.  An extension (north_star "IQUV
 *        formation"): the reference's --pol stops at 4 (:175-176); the shim spells it `-d4 -iquv`. */
typedef struct frbch_config {
  uint32_t size;               /* = sizeof(frbch_config); versioning                          */
  uint32_t abi_version;        /* = FRBCH_ABI_VERSION                                         */
  double freq_mhz;             /* .hdr FREQ (centre, process_vdif.py:127)                     */
  double bw_mhz;               /* .hdr BW, signed: < 0 = LSB (process_vdif.py:117-118,128)    */
  double start_s;              /* -S (process_vdif.py:157,160)                                */
  double total_s;              /* -T                                                          */
  uint32_t nchan;              /* -F<nchan>:...  (process_vdif.py:162-171)                    */
  uint32_t freq_res;           /* -F...:<freq_res>; 0 = 512 if nchan<=128 else 2*nchan (:162) */
  uint32_t tscrunch;           /* -t (only passed when > 1, process_vdif.py:156-158)          */
  int32_t nbit_out;            /* -b: 2, 8, 16, -32 (process_vdif.py:153-155)                 */
  int32_t pol_mode;            /* see above                                                   */
  uint32_t rescale_constant;   /* -c (always passed, process_vdif.py:157,160)                 */
  double rescale_interval_s;   /* -I secs; 0 = -I0 = keepBP (process_vdif.py:181-182)         */
  double dm;                   /* -D (last one wins; header refdm; process_vdif.py:177-178)   */
  uint32_t coherent;           /* -F<nchan>:D (process_vdif.py:179-180): dedisperse in the filterbank */
  int32_t device;              /* GPU ordinal (>= 0)                                          */
  uint32_t max_blocks_per_launch; /* 0 = auto; filterbank blocks batched per kernel launch    */
  uint32_t flags;              /* 0 in production.  Four kernel-selection switches, every one produces the same (correct) output and
                                * has parity cases: 1 generic (radix-2) K1, 2 generic K2 and back end -- the cross-check family of
                                * tests/test_gpu_stress.py --, 1<<20 rescale statistics in a separate pass over the buffered power
                                * rows instead of inside K2, and the form of a first `-c` rescale interval (bits 27 / 28: neither =
                                * automatic, 1<<27 buffered -- float rows written, then digitised --, 1<<28 two-pass -- K2 runs twice
                                * over the resident spill, no float rows; automatic = two-pass for four products at 1024 channels,
                                * DESIGN.md section 5b; both at once is an error).
                                * Any other bit makes frbch_open fail with FRBCH_E_ARG. */
  char telescope[64];          /* .hdr TELESCOPE  (process_vdif.py:123)                       */
  char source[64];             /* .hdr SOURCE     (:124)                                      */
  char ra[32];                 /* .hdr RA         (:125)                                      */
  char dec[32];                /* .hdr DEC        (:126)                                      */
  char datafile[512];          /* .hdr DATAFILE   (:129)                                      */
  uint32_t input_bits;         /* bits per sample of the VDIF: 2, or 1 (mode VDIF_8000-1024-16-1, spif2file.sh:58-61);
                                * 0 = take it from the first frame header (host paths) / 2 (device paths)            */
  uint32_t overlap;            /* 0 in production (automatic).  The digitiser of a completed rescale interval may run beside the K1 of
                                * the next IF of a scan, on plain streams, holding its CUs by an LDS reservation (DESIGN.md section
                                * 4b; automatic: four products at 8 bits, 11/16 of the CUs for K1; else off).  1 = off: every kernel
                                * on the whole chip, one after the other.  (3 << 24) | n = that mode with n CUs (a multiple of 8)
                                * left to K1.  Every setting produces the same output.  Any other mode in bits 24..31 and any
                                * non-zero bits 16..23 make frbch_open fail with FRBCH_E_ARG. */
  float levels[4];             /* 2-bit level table, state 0..3 -> voltage (process_vdif.py:157 passes the bare `-2`: DSPSR's
                                * static table); all four 0 = the default -3.3359, -1, +1, +3.3359.  A run-time table in
                                * every kernel, so another level scheme is a data change.                                  */
  uint32_t unpack_mode;        /* 0 = the static table above (what this build takes the bare `-2` of process_vdif.py:157,160 to
                                * mean).  1 = DYNAMIC LEVEL SETTING after Jenet & Anderson (1998): per window of dls_nsample
                                * consecutive samples of one polarisation the number of low-state samples estimates the undigitised
                                * power, and the window's two output levels are the power-conserving ones for that estimate (formulas:
                                * DESIGN.md section 2a, restated in oracle/frb_oracle.py dls_table).  An OPTION for sites that find
                                * their digifil does this (SURVEY section 7 hard part 2; unpinnable here: DSPSR is absent): 2-bit
                                * input only, through the generic K1 (slower, section 2a).  The digifil shim selects it with
                                * `-2n<nsample>`, `-2c<cutoff>` or `-2t<threshold>` (DSPSR's spelling of the unpacker options).       */
  uint32_t dls_nsample;        /* window length in samples; 0 = 512.  A power of two in 16..8192 that divides the block length   */
  float dls_cutoff_sigma;      /* windows whose low-state count lies further than this many standard deviations from the count a
                                * Gaussian signal at the nominal threshold gives are zeroed (impulsive interference); 0 = 10; < 0 = off */
  float dls_threshold;         /* sampler threshold in units of the nominal rms; 0 = 0.9674 (the optimum for four levels)        */
} frbch_config;

typedef struct frbch_handle frbch_handle;

/* geometry/result info, valid after frbch_open (time fields after the first frame was seen) */
typedef struct frbch_info {
  uint32_t size;
  uint32_t nchan, freq_res, tscrunch, nif;
  uint64_t block_samples;      /* N = 2*nchan*freq_res real samples per pol per block          */
  uint64_t block_payload_bytes;/* N/2                                                          */
  uint64_t rows_per_block;     /* freq_res / tscrunch output time samples per block            */
  uint64_t row_bytes;          /* nif*nchan*|nbit|/8                                           */
  uint64_t rescale_interval_rows; /* 0 = rescale disabled                                      */
  uint64_t rows_out;           /* output time samples produced so far                          */
  uint64_t blocks_done;
  double tsamp_s;              /* nchan*tscrunch/|bw| us (create_config.py:561)                */
  double tstart_mjd;
  double fch1_mhz, foff_mhz;
  uint32_t frame_bytes, header_bytes;
  uint32_t have_rescale;       /* offset/scale are defined                                     */
  uint32_t diag;               /* diagnostics of the last call: bit 0 = the whole-file path wrote a regular output file through its
                                  preallocated shared mapping (parallel copies) instead of write() calls; bit 1 = a FIFO output
                                  took the rows by reference (vmsplice of the pinned ring; FRBCH_FIFO_COPY=1 forces write())   */
  uint64_t frames_seen;        /* host streaming path: frames whose header was checked           */
  uint64_t frames_invalid;     /* ... with the VDIF invalid bit set: their samples enter the filterbank as 0 (the level table's
                                  mean), extract_baseband_chunk.py:56-69 reads the same bit                            */
  uint64_t frame_gaps;         /* ... frame-number discontinuities; forward jumps are filled with zero samples so that the
                                  stream stays contiguous in time (-cont, process_vdif.py:157), see frames_filled       */
  uint64_t block_stride_bytes; /* payload bytes between block starts: = block_payload_bytes, less with -F C:D */
  uint32_t nfilt_pos, nfilt_neg; /* -F C:D overlap-save: channel samples dropped at the start / end of a block */
  uint64_t frames_filled;      /* zero frames inserted for missing frame numbers (host paths)                              */
} frbch_info;

/* per-kernel device time accumulated since the last frbch_timing_reset (HIP events recorded on
 * the stream the kernels are launched on); enabled by frbch_set_profiling(h, 1). */
typedef struct frbch_timing {
  uint32_t size;
  uint32_t nkernels;
  struct {
    char name[48];
    uint64_t launches;
    double total_ms;
    double algorithmic_bytes;  /* sum over launches of the DESIGN.md per-launch byte model      */
  } k[12];                     /* nkernels of them are in use                                    */
} frbch_timing;

/* ---- configuration helpers ------------------------------------------------------------- */
/* defaults = digifil's as the reference relies on them (nbit 8, -d1, 10 s rescale interval) */
int frbch_config_init(frbch_config* cfg);
/* parse the ASCII side file make_hdr writes (process_vdif.py:115-139, keys :122-133) */
int frbch_config_from_hdr(const char* hdr_path, frbch_config* cfg);
/* parse the digifil argv run_digifil builds (process_vdif.py:156-182):
 * -cont -c -b<n> -S<s> -T<s> -2 -D <dm> [-t <T>] -o <out> <hdr> -threads <n>
 * (-P<p> | -d<n>) -F<C>:<R|D> [-I<secs>]; -D and -F may repeat, last wins.  argv[0] is skipped.
 * hdr_path/out_path receive the positional .hdr and the -o value. */
int frbch_parse_digifil_argv(int argc, const char* const* argv, frbch_config* cfg,
                             char* hdr_path, size_t hdr_cap, char* out_path, size_t out_cap,
                             char* err, size_t err_cap);

/* ---- lifecycle --------------------------------------------------------------------------- */
int frbch_open(const frbch_config* cfg, frbch_handle** out);   /* replaces: digifil start-up  */
void frbch_close(frbch_handle* h);
const char* frbch_last_error(frbch_handle* h);                 /* replaces: digifil's stderr  */
const char* frbch_strerror(int code);
int frbch_get_info(frbch_handle* h, frbch_info* info);
/* forget stream + rescale state (as if freshly opened; buffers and tables are kept) */
int frbch_reset(frbch_handle* h);

/* ---- whole-file path: what `digifil ... -o <out> <hdr>` does (process_vdif.py:191) ---------
 * Reads cfg.datafile-style VDIF at `vdif_path`, honours -S/-T, writes SIGPROC header + samples to
 * `out_fil` strictly sequentially.  out_fil may be an existing FIFO: opened
 * O_WRONLY|O_CREAT|O_TRUNC without O_EXCL (INSTALL.md:32-35), never unlinked, never seeked. */
int frbch_run_file(frbch_handle* h, const char* vdif_path, const char* out_fil);

/* ---- one scan, several IFs on one GPU -------------------------------------
 * What base2fil.sh does with N digifil processes, N FIFOs and sigproc `splice`
 * (base2fil.sh:348-350,404-448), in one call: `ifs` are freshly opened handles on the same device with the same
 * nchan / tscrunch / nbit / products, listed like base2fil's splice_list: highest IF first (:350,367);
 * vdif_paths[i] is the per-IF VDIF of ifs[i].  Every IF's rows are copied into its columns of one pitched device
 * buffer (the frequency concatenation happens in HBM), and ONE SIGPROC file is written -- the
 * <exp>_<st>_no0<scan>_IFall_vdif_pol<pol>.fil of base2fil.sh:389: nchans = nif*nchan, fch1 of ifs[0], rows cut
 * to the shortest IF as splice does.  out_fil may be a FIFO (same open flags as frbch_run_file).
 * Errors are reported through frbch_last_error(ifs[0]). */
int frbch_run_scan(frbch_handle* const* ifs, uint32_t nif, const char* const* vdif_paths, const char* out_fil);

/* The same scan with everything resident in HBM (the device-side form of frbch_run_scan): d_frames[i] holds
 * the per-IF VDIF frames of ifs[i] (same frame geometry and length for all), `nblocks` filterbank blocks of every IF are
 * transformed starting `payload_byte_offset` bytes into the payload streams, and the rows land in ONE row buffer
 * d_rows[row][product][IF-major channels] -- ifs[0] (the highest IF, base2fil.sh:350,367) in the first nchan columns of every
 * (row, product) line: the frequency concatenation `splice` does on the host (base2fil.sh:422) happens in the store
 * addresses of the last kernel.  row_pitch_bytes = nif * (row_bytes of one IF); rows_cap rows fit in d_rows.  With `flush`
 * the pending rescale interval of every IF is closed too (the end of the scan).  *rows_written = rows every IF delivered.
 * The IFs go through the two lanes of DESIGN.md section 4b one behind the other: the front half of IF i + 1 overlaps the
 * back half of IF i.  `stream` as in frbch_process_device.  Errors are reported through frbch_last_error(ifs[0]). */
int frbch_scan_device(frbch_handle* const* ifs, uint32_t nif, const void* const* d_frames, size_t nframes,
                      uint32_t frame_bytes, uint32_t header_bytes, uint64_t payload_byte_offset, uint64_t nblocks,
                      int flush, void* d_rows, size_t row_pitch_bytes, uint64_t rows_cap, uint64_t* rows_written, void* stream);

/* ---- streaming host path ----------------------------------------------------------------- */
/* How the stream is cut.  frbch_push takes any byte count (partial frames and partial headers included), frbch_process_device
 * and frbch_scan_device any run of blocks at any payload_byte_offset, frbch_run_file batches on its own, and
 * max_blocks_per_launch decides how many blocks a kernel launch sees.  What depends on none of that:
 *   - the SIGPROC header, the number of rows, and the rows themselves under a GIVEN scale (frbch_set_rescale, or -I0) or a
 *     FROZEN one (`-c`, once the first interval is measured): bit for bit the rows of one frbch_push of the whole stream;
 *   - the rows of a measuring run relative to ITS scale: they are the rows of a run that is given the frbch_get_rescale of the
 *     measuring run beforehand, bit for bit -- whether the interval was buffered, summed inside K2, deferred as a two-pass
 *     batch or digitised on a scan's second lane, and whichever launch it ended in;
 *   - frbch_power_device: it has no state, a block's floats do not depend on the blocks beside it in the call;
 *   - the frame counters of frbch_info.
 * What can depend on it: a MEASURED offset / scale, in the last bits only -- sums that K2 accumulates per launch are added in an
 * order that follows the launches (every cut within 8e-7 of the largest offset and 4e-6 of a scale of one push of the whole stream).  With
 * flags = 1 << 20 (statistics in a separate pass over the buffered rows, chunked by the interval's row count alone) the measured
 * pair, and with it every row, is bit-identical across cuts; with a rescale per interval (no `-c`) and without that flag, the codes
 * of a cut differ from those of one push of the whole stream by at most 1 in fewer than 1e-4 of the values.
 * tests/test_partition.py (emulator build) and tests/test_gpu_partition.py (every register-pass instantiation) hold this. */
/* push whole or partial frames (byte stream starting at a frame boundary on the first call) */
int frbch_push(frbch_handle* h, const uint8_t* frames, size_t nbytes);
/* signal end of input: flushes a pending rescale interval */
int frbch_flush(frbch_handle* h);
/* copy out quantised [t][nif][chan] rows that are ready; returns bytes written, <0 on error */
long frbch_pull(frbch_handle* h, uint8_t* dst, size_t cap);
/* SIGPROC header bytes for the stream (valid once the first frame has been seen) */
long frbch_sigproc_header(frbch_handle* h, uint8_t* dst, size_t cap);

/* ---- device-resident path (inputs and outputs already in HBM) ----------------------------- */
/* Stream order.  frbch_process_device, frbch_flush_device, frbch_power_device, frbch_unpack_device and frbch_scan_device
 * take a `stream` (a hipStream_t) and queue their work; with a non-NULL `stream`:
 *  (a) every read of d_frames and every write of d_out / d_rows / d_power / d_volt is ordered behind all work queued on
 *      `stream` before the call (an asynchronous copy that delivers the frames, for one);
 *  (b) all work queued on `stream` after the call has returned sees the complete rows -- those a second lane wrote (DESIGN.md
 *      section 4b), those of a completed rescale interval and those of a deferred two-pass batch once it is emitted included;
 *  (c) consecutive calls on one handle behave as if issued synchronously, whichever streams they name: A then B, A then NULL,
 *      NULL then A (a call that changes the stream waits on the host for the work of the call before it);
 *  (d) with stream == NULL the work runs on the handle's own non-blocking stream (a scan: that of ifs[0]); the inputs must be
 *      complete on the host's side before the call, and the rows are complete once frbch_reset, frbch_get_rescale or
 *      frbch_close of every handle of the call has returned, or after a device-wide synchronisation;
 *  (e) the frbch_*_device entry points behind and in front of the filterbank (dedisperse, fold, foldp, spsearch, psearch, cutout,
 *      rfi_stats / rfi_peaks / rfi_apply / rfi_clean / rfi_cleanf, cornerturn) are host-synchronous: they take no stream, run on one of their own, and
 *      their outputs are complete on return.  A caller that produced d_rows asynchronously (frbch_scan_device on a stream)
 *      synchronises that stream first.
 * tests/test_stream_order.py (adversary schedules of the emulator build) and tests/test_gpu_stream_order.py hold (a) - (e). */
/* d_frames: device pointer to whole VDIF frames (frame geometry taken from `frame_bytes`,
 * `header_bytes`); the payload stream is entered `payload_byte_offset` bytes after the first
 * payload byte (any value; the fast gather needs it and the payload size to be multiples of the
 * per-row piece, 2..16 bytes, and d_frames 16-byte aligned, else the generic kernel is used);
 * `nblocks` filterbank blocks are transformed.  d_out / d_power must be 16-byte aligned.
 * d_out receives rows_per_block*nblocks rows of row_bytes (fewer while a rescale interval is still
 * being measured; *rows_written says how many).  `stream` is a hipStream_t (NULL = the handle's
 * own stream).  Asynchronous with respect to the host except when a rescale interval completes. */
int frbch_process_device(frbch_handle* h, const void* d_frames, size_t nframes,
                         uint32_t frame_bytes, uint32_t header_bytes, uint64_t payload_byte_offset,
                         uint64_t nblocks, void* d_out, size_t out_cap_bytes,
                         uint64_t* rows_written, void* stream);
/* finish a pending rescale interval into d_out (device) */
int frbch_flush_device(frbch_handle* h, void* d_out, size_t out_cap_bytes, uint64_t* rows_written,
                       void* stream);
/* detected + scrunched power of `nblocks` blocks as float32 [t][nif][chan] (channel order of the
 * output file), no rescale/digitise: the "-b-32 -I0" data product and the parity-test tap. */
int frbch_power_device(frbch_handle* h, const void* d_frames, size_t nframes, uint32_t frame_bytes,
                       uint32_t header_bytes, uint64_t payload_byte_offset, uint64_t nblocks,
                       float* d_power, size_t cap_bytes, void* stream);

/* The unpack stage (A4) in isolation: `nsamples` dual-pol samples starting `payload_byte_offset` bytes into the payload
 * stream, decoded with the handle's level table (frbch_config::levels) exactly as the filterbank's first kernel decodes
 * them: float32 d_volt[pol][nsamples].  decoder 0 = the generic K1's decode (1- and 2-bit input); 1 = the register
 * kernels' two decodes (nibble table of frbch_k1_wave, select chain of frbch_k1_fast; 2-bit input, nsamples even):
 * d_volt[2][pol][nsamples].  The `-2` of process_vdif.py:157,160 selects this static table. */
int frbch_unpack_device(frbch_handle* h, const void* d_frames, size_t nframes, uint32_t frame_bytes,
                        uint32_t header_bytes, uint64_t payload_byte_offset, uint64_t nsamples, int decoder,
                        float* d_volt, size_t cap_bytes, void* stream);

/* ---- rescale state (the one stateful stage; SURVEY 7 hard part 6) ------------------------- */
/* offset/scale are [nif][nchan] in INPUT channel order k (ascending FFT bin), float32 */
int frbch_get_rescale(frbch_handle* h, float* offset, float* scale);
int frbch_set_rescale(frbch_handle* h, const float* offset, const float* scale);

/* ---- after the filterbank ------------------------------------------------
 * The rows of a SIGPROC filterbank -- [t][nifs][nchan] samples of 8 or 16 bit (unsigned) or float32, as frbch_run_file /
 * frbch_run_scan write them -- dedispersed incoherently or folded on the GPU.  The reference delegates both to external
 * programs: PRESTO's prepdata / prepsubband (process_vdif.py:202-229: `-dm`, `-lodm -numdms -dmstep`, `-zerodm`,
 * `-clip`, always `-nobary -noweights -noscales`) and `dspsr -E <par> -L 10 -A -d1 <IFall.fil>` (base2fil.sh:474).
 * Neither program is in the reference tree: the conventions are this library's (oracle/post_oracle.py states them).
 * `_host` variants take host pointers and move the data themselves; `_device` variants work on rows already in HBM. */
typedef struct frbch_fil_desc {
  uint32_t size;               /* = sizeof(frbch_fil_desc)                                                      */
  uint32_t nchan, nifs;        /* SIGPROC nchans, nifs                                                           */
  int32_t nbits;               /* 8, 16 (unsigned codes) or 32 (float32)                                         */
  uint32_t product;            /* which of the nifs products is used (0 = PP+QQ of -d1, or I of IQUV)            */
  uint32_t reserved;
  double fch1_mhz, foff_mhz;   /* SIGPROC fch1 / foff (centre of channel 0, channel step; foff < 0 as written here) */
  double tsamp_s, tstart_mjd;
} frbch_fil_desc;

/* Output samples per DM: nrows minus the largest delay of any requested DM (delay of channel c = DM / 2.41e-4 *
 * (f_c^-2 - f_top^-2) s, rounded to samples as int(x + 0.5)).  < 0: bad arguments. */
long frbch_dedisperse_nout(const frbch_fil_desc* fil, uint64_t nrows, const double* dms, uint32_t ndm);
/* Which kernel frbch_dedisperse_device takes for these arguments (host only, nothing runs): 1 = the LDS-tiled kernel,
 * 0 = the generic one, < 0 = bad arguments; only the ADDRESS of d_rows is examined. */
int frbch_dedisperse_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms, uint32_t ndm);
/* out[dm][t] = sum_c x[t + delay_c(dm)][c]  (float32), after the optional time-domain clip (`-clip <sigma>`: a time
 * sample whose zero-DM sum lies more than clip_sigma sigma off the mean -- two rounds -- is replaced by the channel means
 * of the unclipped samples) and the optional zero-DM filter (`-zerodm`: the mean over channels of every time sample is
 * subtracted).  *nclipped receives the number of clipped time samples.  Integer rows: every sum is exact. */
int frbch_dedisperse_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms, uint32_t ndm,
                          uint32_t zerodm, double clip_sigma, int device, float* out, uint64_t nout,
                          uint64_t* nclipped, char* err, size_t err_cap);
int frbch_dedisperse_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms, uint32_t ndm,
                            uint32_t zerodm, double clip_sigma, int device, float* d_out, uint64_t nout,
                            uint64_t* nclipped, char* err, size_t err_cap);
/* Sub-integrations of subint_s seconds (dspsr -L): ceil(nrows / round(subint_s / tsamp)). */
long frbch_fold_nsub(const frbch_fil_desc* fil, uint64_t nrows, double subint_s);
/* Phase fold with the spin of a .par file: turns(tau) = F0 tau + F1 tau^2 / 2, tau = (tstart - PEPOCH) + t tsamp
 * [- delay_c(dm) when apply_delays: incoherent inter-channel dedispersion at fold time; 0 = what dspsr does with a
 * filterbank: channels are folded as they arrive and the archive keeps DM for a later `dedisperse`].  Topocentric: no
 * barycentric, binary or position terms.  profile[sub][bin][chan] = sum of the samples, hits[...] = their number. */
int frbch_fold_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, double f0_hz, double f1, double pepoch_mjd,
                    double dm, uint32_t apply_delays, uint32_t nbin, double subint_s, int device, double* profile,
                    uint32_t* hits, uint32_t nsub, char* err, size_t err_cap);
int frbch_fold_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, double f0_hz, double f1,
                      double pepoch_mjd, double dm, uint32_t apply_delays, uint32_t nbin, double subint_s, int device,
                      double* d_profile, uint32_t* d_hits, uint32_t nsub, char* err, size_t err_cap);

/* ---- fold of every product, with a phase predictor ------------------------------------------------
 * dspsr folds with a predictor that tempo / tempo2 make from the .par file (base2fil.sh:474: `-E <par>`), which carries
 * the barycentric, binary and position terms, and for `--pol 4` scans the reference plots pol 0, pol 1, Stokes I and a
 * Stokes profile from the folded archive (base2fil.sh:481-491).  frbch_foldp_* fold ALL nifs (1..4) products of the rows
 * in one pass (`fil->product` is ignored) with either phase model:
 *   nseg = 0: the polynomial of frbch_fold_*, tau = (tstart - PEPOCH) 86400 + t tsamp [- delay_c], and when doppler != 0
 *             tau := tau + tau * doppler  (doppler = observed / intrinsic spin frequency - 1, a constant for the scan);
 *   nseg > 0: TEMPO polyco blocks (topocentric already: doppler must be 0).  Row t, channel c, block s:
 *               sec   = t * tsamp [- delay_c]
 *               dt    = (tstart_mjd - tmid_s) * 1440.0 + sec / 60.0                        (minutes)
 *               turns = (rphase_frac + (dt * 60.0) * f0_hz) + horner(coeff, dt)
 *             -- TEMPO's PHASE = RPHASE + DT 60 F0 + C1 + DT C2 + DT^2 C3 + ... -- Horner from the highest coefficient
 *             down: h = coeff[n-1]; h = h * dt + coeff[i] for i = n-2 .. 0.
 *   bin = min((int)((turns - floor(turns)) * nbin), nbin - 1).
 * Every operation is an IEEE double operation rounded on its own (no fused multiply-add).
 * The block of a row: block s >= 1 starts at the first row at or after the midpoint of tmid_{s-1} and tmid_s,
 *   x = ((0.5 * (tmid_{s-1} + tmid_s) - tstart_mjd) * 86400.0) / tsamp_s;   first_row_s = x <= 0 ? 0 : min(ceil(x), nrows)
 * computed by the host; row t uses the last block whose first_row <= t (channel delays do not move a row to another block).
 * FRBCH_E_ARG: blocks not in ascending tmid, ncoeff outside 1..15, a span <= 0, doppler != 0 with nseg > 0, or the first
 * or the last row (t tsamp, no delay) outside every block's span, |dt| <= span_min / 2 (where dspsr refuses as well).
 *
 * Coherency products to Stokes parameters of a folded `-d4` file (post.stokes), circular basis as pol_mode 5 above
 * (products in file order PP, QQ, Re(PQ*), Im(PQ*)):   I = PP + QQ,  Q = 2 Re(PQ*),  U = 2 Im(PQ*),  V = PP - QQ;
 * linear polarisation L = sqrt(Q^2 + U^2), position angle PA = atan2(U, Q) / 2. */
typedef struct frbch_polyco_seg {      /* one TEMPO polyco block                                                         */
  double tmid_mjd;                     /* TMID                                                                           */
  double rphase_frac;                  /* RPHASE reduced to [0, 1) by the parser (from the text: 1e10 turns lose no fraction) */
  double f0_hz;                        /* reference rotation frequency of the block                                      */
  double span_min;                     /* validity: |T - TMID| <= span / 2, minutes                                      */
  uint32_t ncoeff, reserved;           /* 1..15                                                                          */
  double coeff[15];
} frbch_polyco_seg;

typedef struct frbch_fold_model {
  uint32_t size, nseg;                 /* = sizeof(frbch_fold_model); nseg = 0: the F0 / F1 / PEPOCH polynomial           */
  const frbch_polyco_seg* seg;         /* [nseg], ascending tmid                                                         */
  double f0_hz, f1, pepoch_mjd;        /* used when nseg = 0                                                             */
  double doppler;                      /* nseg = 0 only                                                                  */
  double dm;                           /* as frbch_fold_*                                                                */
  uint32_t apply_delays, nbin;
  double subint_s;
} frbch_fold_model;

/* profile[sub][product][bin][chan] = sums (double; exact for integer rows), hits[sub][bin][chan] = rows, shared by the
 * products; nsub as frbch_fold_nsub gives it.  *kernel_used (may be NULL): 0 = the generic kernel, 1 = the LDS kernel
 * (8- / 16-bit rows, no per-channel delays, nbin small enough for a tile of >= 16 channels in the LDS).  Both give the
 * same bits on integer rows.  With nseg = 0 and doppler = 0, product p equals frbch_fold_* with product = p exactly on
 * integer rows. */
int frbch_foldp_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_fold_model* model, int device,
                     double* profile, uint32_t* hits, uint32_t nsub, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_foldp_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_fold_model* model,
                       int device, double* d_profile, uint32_t* d_hits, uint32_t nsub, uint32_t* kernel_used, char* err,
                       size_t err_cap);

/* ---- single-pulse search of the dedispersed series -------------------------------------------------
 * process_vdif.py:84-98,202-229 offers a DM range (`--dm --dm2 --dmstep`) so that the .dat files can be searched for
 * single pulses, usually with PRESTO's single_pulse_search.py by hand.  frbch_spsearch_* do that search on the GPU, on
 * series[dm][t] (float32, t < nout) still in HBM: boxcar matched filters of the listed widths over block-normalised
 * samples.  PRESTO is not in the reference tree: the conventions are this library's (tests/spsearch_oracle.py restates
 * them in numpy), chosen so that every result is reproducible to the bit:
 *  1. Block statistics.  L = detrend_len (0 means 1000; 64..65536), nblk = max(1, nout / L), block b = [bL, (b+1)L), the
 *     last block runs to nout.  Per (dm, block) two rounds of mean and sigma in double, every operation rounded on its
 *     own (no fused multiply-add): s1 = sum x, s2 = sum x*x and the count n as 64 partial sums -- partial j adds the
 *     samples at block positions j, j + 64, ... in ascending order -- added in ascending j; mean = s1 / n,
 *     var = s2 / n - mean * mean, sigma = var > 0 ? sqrt(var) : 0.  Round 2 uses only the samples with
 *     |x - mean1| <= 3.0 * sigma1, each in its own partial.  A block with sigma1 = 0, no kept sample or sigma2 = 0 is
 *     dead (a NaN or infinite sample makes `var > 0` false: dead as well).
 *  2. z = (x - mean2) * (1 / sigma2) in double, clipped to +-65536;  q = (int64)floor(z * 1024 + 0.5);  q = 0 in dead
 *     blocks.  Everything below is integer arithmetic, exact in any order.
 *  3. S_w[t] = sum_{i<w} q[t + i] for 0 <= t <= nout - w (a width above nout is skipped) is held against
 *     T_w = ceil((threshold * 1024) * sqrt(w)), computed by the host:  S_w[t] >= T_w.
 *  4. Peaks per width, h = w / 2 (integer): t is a raw peak iff it passes the threshold, S_w[t] > S_w[t'] for
 *     t - h <= t' < t and S_w[t] >= S_w[t'] for t < t' <= t + h (windows cut to 0 .. nout - w).  Its centre is
 *     c = t + w / 2, its sigma = (double)S / (1024.0 * sqrt((double)w)).
 *  5. Across widths, on the host, over the raw list of one DM, in ONE pass (a dropped peak still drops others): a raw peak
 *     (c, w, sigma) is dropped iff another raw peak (c', w', sigma') of that DM has |c - c'| <= max(w, w') / 2 and
 *     sigma' > sigma, or sigma' == sigma and (w' < w, or w' == w and c' < c).
 *  6. The survivors, sorted by (dm_index, sample, width), are the candidates.
 * The device list of raw peaks holds 2^20 entries per call; a search that finds more returns FRBCH_E_CAPACITY with a
 * "threshold too low" message -- never a cut list. */
typedef struct frbch_sp_params {
  uint32_t size, nwidth;               /* = sizeof(frbch_sp_params); 1..16 widths                                        */
  uint32_t widths[16];                 /* boxcar widths in samples, strictly ascending, each 1..1024                     */
  uint32_t detrend_len, reserved;      /* L of step 1: 0 = 1000, else 64..65536                                          */
  double threshold;                    /* sigma, > 0 (at most 1e6)                                                       */
} frbch_sp_params;

typedef struct frbch_sp_cand {
  uint32_t dm_index, width;            /* row of the series, boxcar width in samples                                     */
  uint64_t sample;                     /* centre c = t + w / 2                                                           */
  float sigma;                         /* float32 of the double of step 4                                                */
  uint32_t reserved;
} frbch_sp_cand;

/* cands[cap] (host memory) receives the first `cap` candidates in output order, *ncand their total number; more than
 * `cap`: FRBCH_E_CAPACITY (cap = 0 with cands = NULL counts them).  *kernel_used (may be NULL): 0 = the generic kernels
 * (a quantise pass, then a thread per (dm, t) with direct sums), 1 = the LDS kernel (a workgroup per DM and tile of 2048
 * samples: one load, one prefix sum, two LDS reads per S_w[t]), taken when the largest listed width is at most 512 and
 * nout < 2^31.  Both give the same records.  FRBCH_E_ARG: widths not ascending or outside 1..1024, nwidth outside 1..16,
 * threshold or detrend_len outside their ranges, a wrong `size`, ndm above 65535. */
int frbch_spsearch_device(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_sp_params* params, int device,
                          frbch_sp_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, char* err,
                          size_t err_cap);
int frbch_spsearch_host(const float* series, uint32_t ndm, uint64_t nout, const frbch_sp_params* params, int device,
                        frbch_sp_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, char* err, size_t err_cap);
/* The production call: one upload of the rows, frbch_dedisperse_device, then frbch_spsearch_device on the plane where it
 * lies in HBM.  The series is downloaded only when series_out != NULL ([ndm][nout], the bits of frbch_dedisperse_host). */
int frbch_dedisperse_search_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms, uint32_t ndm,
                                 uint32_t zerodm, double clip_sigma, const frbch_sp_params* params, int device,
                                 float* series_out, uint64_t nout, uint64_t* nclipped, frbch_sp_cand* cands, uint64_t cap,
                                 uint64_t* ncand, uint32_t* kernel_used, char* err, size_t err_cap);

/* ---- periodicity search of the dedispersed series --------------------------------------------------
 * The other search people run on the .dat files of a DM range (process_vdif.py:78-98,202-229) is `realfft` + `accelsearch`.
 * frbch_psearch_* do the zero-acceleration part of it on the GPU (frbch_pasearch_*, below, add trial accelerations), on series[dm][t] (float32, t < nout) still in HBM: one long
 * transform per series, a red-noise normalisation, incoherent harmonic sums of 1, 2, 4, 8 and 16 harmonics, and a list of
 * peaks.  PRESTO is not in the reference tree: the conventions are this library's [EXT-UNVERIFIED: parity with accelsearch is
 * not pinned] (tests/psearch_oracle.py restates them in numpy), chosen so that every record is reproducible to the bit.
 * NOT done: jerk search (trial accelerations are frbch_pasearch_*, below), barycentring, transform lengths that are no power of two, and the merging of
 * harmonically related candidates (a strong signal appears at f, and at f/2, 2f/3 ... with less significance: the output says
 * what was found and a reader can see the ladder).
 *  0. Length.  n = nfft, or with nfft = 0 the largest power of two not above nout (frbch_psearch_nfft); 2^12 <= n <= 2^22 and
 *     n <= nout.  Only the samples t < n are used.
 *  1. Mean, per series, in double: 64 partial sums, partial j adds the samples at positions j, j + 64, ... in ascending
 *     order, the partials are added in ascending j (the rule of frbch_spsearch_* step 1); mean = sum / n;
 *     z[t] = (float)((double)x[t] - mean).  A series whose mean is not finite is DEAD: all its powers are 0, it yields no record.
 *  2. Series are transformed in pairs (2m, 2m + 1) as the real and the imaginary part of one complex sequence; the missing
 *     partner of an odd last series and a dead series are 0 throughout, so that a bad series never reaches its partner.
 *     Z = DFT_n(z) exactly as in the periodicity test of frbch_rfi_peaks_*: radix 2, decimation in time, float32, no fused
 *     multiply-add, input in bit-reversed order, the same butterfly, W[k] = ((float)cos(a), (float)(-sin(a))), a = 2.0 pi k / n
 *     in double ON THE HOST.  The operation graph is fixed, the schedule is free.
 *  3. Powers, k = 1 .. n/2 - 1, float32: N_c0[k], N_c1[k] of that section (four times the power).  Bins 0 and n/2 are not used.
 *  4. Normalisation.  The nb = n/2 - 1 bins 1 .. n/2 - 1 are cut into blocks of B = wblock bins (0 = 128; a power of two in
 *     32 .. 1024), block b = [1 + b B, 1 + (b + 1) B); the rest of r = nb mod B bins is a block of its own when r >= B / 2 and
 *     belongs to the last whole block otherwise.  (With n and B powers of two r is always B - 1: the last block is always the
 *     short one.  The rule is stated, and coded, for any nb.)  Level of a block of cnt bins: S = the sum of its powers in double in
 *     ascending k; max = its largest power (a walk over ascending k that starts at 0 and replaces when N[k] > max: a NaN never
 *     replaces); m = (S - (double)max) / (double)(cnt - 1): one strong line does not lift its own floor.
 *     p[k] = (float)((double)N[k] / m); a block whose m is not finite or <= 0 has p = 0 (a constant or dead series: all of them).
 *     kmin = max(1, ceil(flo_hz * (double)n * tsamp_s)) (left to right; flo_hz 0 = 0.5): p[k] = 0 for k < kmin.  For noise p is
 *     exponentially distributed with mean 1.
 *  5. Harmonic sums.  For every fold h in {1, 2, 4, 8, 16} with h <= nharm (1, 2, 4, 8 or 16; 0 = 16):
 *         H_h[k] = sum over j = 1 .. h of p[(j k + h / 2) / h]          (integer divisions)
 *     in float, starting from 0, j ascending, every addition rounded; k = h kmin .. n/2 - 1 (a fold whose range is empty is
 *     skipped).  k counts bins of the HIGHEST summed harmonic; the fundamental is f = k / (h n tsamp).
 *  6. Thresholds, frbch_psearch_thresholds, on the host: T_h is the power at which the survival function of a sum of h unit
 *     exponentials, Q(h, x) = exp(-x) sum_{i<h} x^i / i!, equals the one-sided Gaussian tail 0.5 erfc(sigma / sqrt 2)
 *     (0 < sigma <= 30): bisection in double on [0, 1000] until the interval is one step of double wide, the upper end -- where
 *     Q <= tail -- rounded UP to float.  A bin passes when H_h[k] >= T_h.
 *  7. Raw peaks.  A passing bin is a raw peak iff H_h[k] > H_h[k - 1] and H_h[k] >= H_h[k + 1]; a neighbour outside the range
 *     of step 5 counts as smaller.  The device list holds 2^20 raw peaks {dm_index, h, k, H} per call; more: FRBCH_E_CAPACITY
 *     with a "threshold too low" message -- never a cut list.
 *  8. On the host, in double, one pass each.  sigma of a record: with x = (double)H (an infinite H counts as FLT_MAX),
 *     lq = log Q(h, x) = -x + log(sum_{i<h} x^i / i!) -- for x < 1 the sum by Horner, s = 1, then s = s x / i + 1 for
 *     i = h - 1 .. 1; from x = 1 on with the largest term taken out so that nothing overflows:
 *     lq = -x + ((h - 1) log x - sum_{i=2}^{h-1} log i + log r), r = 1, then r = r i / x + 1 for i = 1 .. h - 1 -- sigma is
 *     the s with lt(s) = lq (0 when lq >= 0), lt(s) = log(0.5 erfc(s / sqrt 2)) for s < 30 and -0.5 s s - log(s) - 0.5 log(2 pi) + log1p(-1 / (s s)
 *     + 3 / (s s s s)) from there on (finite for every float H): 64 bisection steps on [0, sqrt(-2 lq) + 2], sigma = the middle
 *     of the last interval.  (It goes through the C library's exp / log / erfc: equal to the last bits only on the same
 *     library.)  freq_hz = (double)k / ((double)h * ((double)n * tsamp_s)).
 *     Within one series a record is dropped iff another record (h', k') OF THAT SERIES -- dropped itself or not -- lies within one
 *     bin of the fundamental, |f - f'| <= 1 / (n tsamp) evaluated exactly as |k h' - k' h| <= h h', and has a larger sigma, or
 *     the same sigma and (h' < h, or h' = h and k' < k).  The survivors, sorted by (dm_index, h, k), are the records.
 *  9. frbch_ps_group_cands (host only) joins the records of one signal across trial DMs: a and b are LINKED iff
 *     |dm_index_a - dm_index_b| <= dm_gap (1..16, the rule of frbch_sp_group_cands) and |f - f'| <= 1.5 / (n tsamp), exactly
 *     2 |k h' - k' h| <= 3 h h'; groups are the connected components.  `best` has the largest sigma; ties: the smaller h, the
 *     lower dm_index, the smaller k.  Groups come sorted by best.sigma descending, then f ascending (exactly: k h' < k' h),
 *     then dm_index, then h. */
typedef struct frbch_ps_params {
  uint32_t size, nfft;                 /* = sizeof(frbch_ps_params); n of step 0, 0 = the largest power of two <= nout      */
  uint32_t nharm, wblock;              /* 1, 2, 4, 8, 16 (0 = 16); B of step 4 (0 = 128)                                  */
  double sigma;                        /* Gaussian sigma of the thresholds, in (0, 30]                                    */
  double flo_hz;                       /* lowest frequency searched, >= 0 and finite (0 = 0.5 Hz)                         */
  double tsamp_s;                      /* sampling time of the series, > 0                                                */
} frbch_ps_params;

typedef struct frbch_ps_cand {
  uint32_t dm_index, h, k;             /* row of the series, fold, bin of the highest summed harmonic                     */
  float power;                         /* H_h[k]                                                                          */
  double sigma, freq_hz;               /* of step 8                                                                       */
} frbch_ps_cand;

typedef struct frbch_ps_group {
  frbch_ps_cand best;
  uint32_t nmember, dm_index_lo, dm_index_hi, reserved;
} frbch_ps_group;

/* n of step 0 for these arguments; < 0: refused (FRBCH_E_ARG). */
long frbch_psearch_nfft(uint64_t nout, const frbch_ps_params* params);
/* thr[5] receives T_1, T_2, T_4, T_8, T_16 of step 6 (all five, whatever nharm says). */
int frbch_psearch_thresholds(double sigma, float* thr);
/* Which form frbch_psearch_device takes for these arguments (host only, nothing runs; only the ADDRESS of d_series is
 * examined): 1 = the fast form (d_series 16-byte aligned: the transform in LDS-resident passes, *npass of them -- 1 for
 * n <= 2^13, 2 up to 2^18, 3 above; every global access of a pass is 16 consecutive values), 0 = the generic form (the
 * transform stage by stage through global memory; *npass = 0), < 0 = refused.  npass may be NULL.  Both give the same records. */
int frbch_psearch_kernel(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_ps_params* params, uint32_t* npass);
/* cands[cap] (host memory) receives the first `cap` records in output order, *ncand their total number; more than `cap`:
 * FRBCH_E_CAPACITY (cap = 0 with cands = NULL counts them).  kernel_used[2] (may be NULL): the form and the passes, as
 * frbch_psearch_kernel.  d_series holds ndm * nout floats and is never written; the call allocates its scratch -- the work
 * array [ceil(ndm / 2)][n] complex, p [ndm][n / 2], the table, the raw list -- and frees it before it returns; like the other
 * post-filterbank _device entry points it works on a stream of its own and returns when its work is done.
 * FRBCH_E_ARG: n outside 2^12 .. 2^22, no power of two or above nout; nharm not 0, 1, 2, 4, 8, 16; wblock not 0 or a power of
 * two in 32 .. 1024; sigma outside (0, 30]; flo_hz negative or not finite; tsamp_s not positive; a wrong `size`; ndm above 65535. */
int frbch_psearch_device(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_ps_params* params, int device,
                         frbch_ps_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_psearch_host(const float* series, uint32_t ndm, uint64_t nout, const frbch_ps_params* params, int device,
                       frbch_ps_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, char* err, size_t err_cap);
/* The production call, the sibling of frbch_dedisperse_search_host: one upload of the rows, frbch_dedisperse_device, then
 * frbch_psearch_device on the plane where it lies in HBM (params->tsamp_s = 0 takes fil->tsamp_s).  The series is downloaded
 * only when series_out != NULL ([ndm][nout], the bits of frbch_dedisperse_host). */
int frbch_dedisperse_psearch_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms, uint32_t ndm,
                                  uint32_t zerodm, double clip_sigma, const frbch_ps_params* params, int device,
                                  float* series_out, uint64_t nout, uint64_t* nclipped, frbch_ps_cand* cands, uint64_t cap,
                                  uint64_t* ncand, uint32_t* kernel_used, char* err, size_t err_cap);
/* Step 8 alone (host only), on raw peaks given as records whose dm_index, h, k and power are set: sigma and freq_hz are
 * filled in, the survivors written in output order.  FRBCH_E_ARG: n no power of two in 2^12 .. 2^22, tsamp_s not positive, an
 * h other than 1, 2, 4, 8, 16, a k outside 1 .. n/2 - 1. */
int frbch_psearch_sift(const frbch_ps_cand* raw, uint64_t nraw, uint32_t n, double tsamp_s, frbch_ps_cand* cands, uint64_t cap,
                       uint64_t* ncand, char* err, size_t err_cap);
/* Step 9.  More groups than `cap`: FRBCH_E_CAPACITY with *ngroup set (cap = 0 with groups = NULL counts).  FRBCH_E_ARG:
 * dm_gap outside 1..16, an h other than 1, 2, 4, 8, 16, k = 0. */
int frbch_ps_group_cands(const frbch_ps_cand* cands, uint64_t ncand, uint32_t dm_gap, frbch_ps_group* groups, uint64_t cap,
                         uint64_t* ngroup, char* err, size_t err_cap);

/* ---- acceleration search of the dedispersed series --------------------------------------------------
 * A pulsar in a binary changes its apparent frequency during the scan and smears over many Fourier bins; the search above
 * loses it.  frbch_pasearch_* repeat that search for a list of trial accelerations: for every trial each series is re-read
 * at quadratically stretched sample positions (time-domain resampling, a pure gather with an integer index rule), and the
 * resampled series go through steps 1 to 8 above unchanged.  The conventions are this library's own [EXT-UNVERIFIED: parity
 * with accelsearch or PEASOUP is not pinned] (tests/accel_oracle.py restates them in numpy); every record is reproducible to
 * the bit.  NOT done: jerk search, barycentring, interpolation between samples (the nearest sample is taken).
 *  A0. Given n of step 0, tsamp_s and a trial acceleration a in m/s^2:
 *          q    = (a * tsamp_s) / (2.0 * 299792458.0)        double, on the host, evaluated as written
 *          g(t) = rint( q * (double)( (int64)t * ((int64)t - (int64)n) ) )
 *                 one double multiplication, rounded to the nearest integer, ties to even; the integer product is exact
 *          u(t) = t + (int64) g(t)                           an integer addition: nothing can contract into a multiply-add
 *          r_a[t] = x[u(t)],  0 <= t < n
 *      Both ends are pinned: u(0) = 0 and u(n - 1) = n - 1.  A trial is accepted iff a is finite and |q| * n <= 0.5, i.e. up
 *      to |a| = c / (n tsamp_s); otherwise FRBCH_E_ARG with a message that names that largest |a|.  Within the range
 *      0 <= u(t) <= n - 1, u never steps back and never by more than 2, and |u(t) - t| <= n / 8 (tests/test_accel.py checks all
 *      three at n = 2^12 and 2^22 for q n = +-0.5).  Samples at t >= n never influence anything, and no address outside
 *      d_series[0, ndm * nout) is read.
 *      Meaning: a signal of nu (t - q t^2) cycles (t in samples) becomes one of nu (1 - q n) t cycles, a steady tone.  POSITIVE
 *      a therefore removes a frequency that FALLS during the scan (a source accelerating away from the observer), and
 *      freq_hz of a record is the frequency at the MIDDLE of the n * tsamp_s span.  A fold of such a record takes F0 = freq_hz,
 *      F1 = -F0 a / c and PEPOCH = the start + (n tsamp_s / 2).
 *  A1. The records of trial i are exactly those of frbch_psearch_* on the plane [ndm][n] of that trial's resampled series:
 *      the series are paired (2m, 2m + 1) WITHIN the trial, the missing partner of an odd last series is zero, every trial
 *      goes through steps 1 to 8 on its own (a NaN sample makes a series dead only in the trials whose gather reaches it).
 *      A trial a = 0 reproduces the records of frbch_psearch_*.  accs[nacc], 1 <= nacc <= 1024, is strictly ascending.
 *      The records, frbch_pa_cand, come sorted by (acc_index, dm_index, h, k).
 *  A2. Work.  The scratch is allocated once and the table uploaded once per call; the trials are searched in batches: a
 *      resampled plane with an even number of rows per trial (ndm, and a zero row when ndm is odd) is handed to the kernels of
 *      the periodicity search as one plane of trials * rows series.  batch_rows bounds the series rows of a batch (a batch
 *      always holds at least one whole trial and at most 65534 rows); 0 leaves the choice to the library: as many whole
 *      trials as 2 GiB of per-row scratch hold (10 n + 12 bytes a row: the resampled samples, the work array, the powers, the
 *      mean, the live word).  The records never depend on batch_rows.  The raw-peak list of step 7 holds 2^20 peaks PER BATCH;
 *      more is FRBCH_E_CAPACITY, never a cut list -- and that overflow is the one thing that may depend on batch_rows (a
 *      smaller batch holds fewer peaks).  frbch_pasearch_plan says what a call will do.
 *  A3. frbch_pa_group_cands (host only) joins the records of one signal across trial DMs and trial accelerations: a and b
 *      are LINKED iff |dm_index_a - dm_index_b| <= dm_gap and |acc_index_a - acc_index_b| <= acc_gap (both 1..16) and
 *      2 |k h' - k' h| <= 3 h h' (step 9); groups are the connected components.  `best` has the largest sigma; ties: the
 *      smaller h, the lower dm_index, the lower acc_index, the smaller k.  Groups come sorted by best.sigma descending, then f
 *      ascending (exactly: k h' < k' h), then dm_index, then acc_index, then h. */
typedef struct frbch_pa_cand {
  uint32_t dm_index, acc_index, h, k;  /* row of the series, trial, fold, bin of the highest summed harmonic               */
  float power;                         /* H_h[k]                                                                          */
  uint32_t reserved;
  double sigma, freq_hz, acc_ms2;      /* of step 8; accs[acc_index]                                                      */
} frbch_pa_cand;

typedef struct frbch_pa_group {
  frbch_pa_cand best;
  uint32_t nmember, dm_index_lo, dm_index_hi, acc_index_lo, acc_index_hi, reserved;
} frbch_pa_group;

/* Which form the resampler takes for these addresses (host only, nothing runs; only the ADDRESSES are examined): 1 = the
 * fast form (d_series and d_out 16-byte aligned and nout a multiple of 4, so that every row is aligned: the contiguous input
 * window of 1024 outputs -- at most 2047 samples, since u steps by 0, 1 or 2 -- is staged through the LDS with 16-byte loads
 * and the outputs leave in 16-byte stores), 0 = the generic form (a plain gather, one output per thread, any alignment, any
 * nout), < 0 = refused.  Both give the same bytes.  Inside frbch_pasearch_* d_out is the library's own, aligned, plane. */
int frbch_resample_kernel(const float* d_series, uint64_t nout, const float* d_out);
/* Step A0 alone: d_out [nacc][ndm][n] receives r_a of every series for every trial.  n is a power of two in 2^12 .. 2^22 and
 * at most nout.  kernel_used[1] (may be NULL): the form, as frbch_resample_kernel.  d_series is never written. */
int frbch_resample_device(const float* d_series, uint32_t ndm, uint64_t nout, uint32_t n, double tsamp_s, const double* accs,
                          uint32_t nacc, int device, float* d_out, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_resample_host(const float* series, uint32_t ndm, uint64_t nout, uint32_t n, double tsamp_s, const double* accs,
                        uint32_t nacc, int device, float* out, uint32_t* kernel_used, char* err, size_t err_cap);
/* What frbch_pasearch_* will do for these arguments (host only): *n of step 0, the series rows of a batch (a whole number of
 * trials, pad rows included), the number of batches and the bytes of device scratch.  Every pointer may be NULL. */
int frbch_pasearch_plan(uint32_t ndm, uint64_t nout, const frbch_ps_params* params, uint32_t nacc, uint32_t batch_rows,
                        uint32_t* n, uint32_t* rows_per_batch, uint32_t* nbatch, uint64_t* scratch_bytes, char* err,
                        size_t err_cap);
/* The siblings of the three frbch_psearch_* calls.  cands / cap / ncand as there.  kernel_used[3] (may be NULL): the form of
 * the resampler, the form of the transform, its passes.  d_series holds ndm * nout floats and is never written; like the
 * other post-filterbank _device entry points the call works on a stream of its own and returns when its work is done.
 * FRBCH_E_ARG: what frbch_psearch_device refuses; ndm above 65534; nacc outside 1..1024; accs not strictly ascending; a
 * trial that is not finite or beyond |q| n <= 0.5. */
int frbch_pasearch_device(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_ps_params* params, const double* accs,
                          uint32_t nacc, uint32_t batch_rows, int device, frbch_pa_cand* cands, uint64_t cap, uint64_t* ncand,
                          uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_pasearch_host(const float* series, uint32_t ndm, uint64_t nout, const frbch_ps_params* params, const double* accs,
                        uint32_t nacc, uint32_t batch_rows, int device, frbch_pa_cand* cands, uint64_t cap, uint64_t* ncand,
                        uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_dedisperse_pasearch_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms, uint32_t ndm,
                                   uint32_t zerodm, double clip_sigma, const frbch_ps_params* params, const double* accs,
                                   uint32_t nacc, uint32_t batch_rows, int device, float* series_out, uint64_t nout,
                                   uint64_t* nclipped, frbch_pa_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used,
                                   char* err, size_t err_cap);
/* Step A3.  More groups than `cap`: FRBCH_E_CAPACITY with *ngroup set (cap = 0 with groups = NULL counts).  FRBCH_E_ARG:
 * dm_gap or acc_gap outside 1..16, an h other than 1, 2, 4, 8, 16, k = 0. */
int frbch_pa_group_cands(const frbch_pa_cand* cands, uint64_t ncand, uint32_t dm_gap, uint32_t acc_gap, frbch_pa_group* groups,
                         uint64_t cap, uint64_t* ngroup, char* err, size_t err_cap);

/* ---- candidates: grouping across DMs, and the two planes a classifier reads -------------------------
 * The search above returns one record per DM for a pulse that stands out at several trial DMs.  frbch_sp_group_cands
 * joins them (host only, no device), and frbch_cutout_* cut, for every kept candidate, the two small images a FETCH-style
 * classifier reads [EXT-UNVERIFIED: FETCH, `your` and heimdall are not in the reference tree; the reference only hands
 * the spliced filterbank over (base2fil.sh:118-122, 425-432) and parses the resulting image names
 * (utils/parse_fetch_image_name.py)]: the dedispersed frequency-time plane and the DM-time "bow tie".  The conventions
 * are this library's own, restated in numpy in tests/cutout_oracle.py, and every result is reproducible to the bit.
 *
 * Grouping, integer arithmetic only.  D_i = the largest per-channel delay n_c(dms[i]) in samples (the delays of
 * frbch_dedisperse_*).  Two records a, b are LINKED iff
 *     |dm_index_a - dm_index_b| <= dm_gap   and   |sample_a - sample_b| <= max(width_a, width_b) / 2 + |D_a - D_b|
 * (integer division; the second term is the smear of a pulse dedispersed at the wrong DM -- the series are referenced to
 * the top of the band).  Groups are the connected components of the link graph.  `best` is the member with the largest
 * sigma; ties: the narrower width, then the lower dm_index, then the earlier sample.  Groups come sorted by best's
 * (dm_index, sample, width).  More groups than `cap`: FRBCH_E_CAPACITY with *ngroup set (cap = 0 with groups = NULL
 * counts).  FRBCH_E_ARG: dm_gap outside 1..16, a dm_index >= ndm, a DM frbch_dedisperse_nout would refuse. */
typedef struct frbch_sp_group {
  frbch_sp_cand best;                  /* the member that represents the group                                            */
  uint32_t nmember, dm_index_lo, dm_index_hi, reserved;
  uint64_t sample_lo, sample_hi;       /* over the members' centres                                                       */
} frbch_sp_group;
int frbch_sp_group_cands(const frbch_fil_desc* fil, const double* dms, uint32_t ndm, const frbch_sp_cand* cands, uint64_t ncand,
                         uint32_t dm_gap, frbch_sp_group* groups, uint64_t cap, uint64_t* ngroup, char* err, size_t err_cap);

/* Cut-outs.  For candidate i with f = tfactor, t0 = sample - (nt / 2) * f (signed 64 bit) and cpb = nchan / nf:
 *   trial DMs   dm_k = dm_lo + (double)k * ((dm_hi - dm_lo) / (double)(ndm - 1)), every operation rounded on its own
 *               (ndm = 1: dm_lo);
 *   delays      n_c(.) exactly as frbch_dedisperse_* compute them;
 *   samples     V(s, c) = the sample of product fil->product at row s, channel c, PRESENT iff 0 <= s < nrows.  Absent
 *               samples add nothing and are not counted: a window partly or wholly outside the data is no error, its
 *               hits say so;
 *   FT[i][b][j] = sum over c = b cpb .. (b + 1) cpb - 1 (ascending), over u = 0 .. f - 1 (ascending, the inner loop) of
 *               V(t0 + j f + u + n_c(dm), c);  ft_hits[i][b][j] = the number of present terms.  Frequency bins are in
 *               file channel order;
 *   DT[i][k][j] = the same sum over ALL channels at the delays n_c(dm_k);  dt_hits likewise.
 * Sums are in double and stored as float32, as in frbch_dedisperse_*: on integer rows every sum is exact in any order
 * (at most 65535 * 512 * 4096 < 2^53), on float rows the order is the stated one and the result bit-identical.
 * NO clip and NO zero-DM filter are applied: the classifier normalises the planes itself.
 * FRBCH_E_ARG: a wrong `size`, nt odd or outside 2..1024, nf not dividing nchan, ndm outside 1..1024, tfactor outside
 * 1..512, ncand outside 1..65535, a DM outside [0, 1e5), dm_hi < dm_lo, a plane set of 2^31 elements or more, a delay
 * of more than 2^30 samples, and ncand * ndm * nchan > 2^26 (the delay table of a call, 256 MiB; the same query and the
 * same tables serve frbch_cutout_kernel): cut a longer batch into several calls of whole candidates.
 * *kernel_used (may be NULL): 1 = the LDS kernel (8- / 16-bit rows, whole 64-byte channel tiles, d_rows and the row pitch
 * 16-byte aligned, and the rows of every (group of 8 plane rows, channel tile, time tile) fit the LDS), 0 = the generic
 * kernel (one thread per pixel); both give the same bits.  One choice holds for both planes of all candidates. */
typedef struct frbch_cutout_params { uint32_t size, nt, nf, ndm; } frbch_cutout_params;   /* size = sizeof(frbch_cutout_params) */
typedef struct frbch_cutout_cand {
  double dm, dm_lo, dm_hi;             /* DM of the frequency-time plane; the DM-time plane spans dm_lo .. dm_hi           */
  int64_t sample;                      /* centre, in samples of the dedispersed series (row index at the top of the band)  */
  uint32_t tfactor, reserved;          /* rows per time bin, 1..512                                                        */
} frbch_cutout_cand;
int frbch_cutout_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_cutout_params* par,
                        const frbch_cutout_cand* cands /* host */, uint32_t ncand, int device,
                        float* d_ft, uint32_t* d_ft_hits,   /* [ncand][nf][nt]  */
                        float* d_dt, uint32_t* d_dt_hits,   /* [ncand][ndm][nt] */
                        uint32_t* kernel_used, char* err, size_t err_cap);
/* the same with host pointers: one upload of the rows, one download of the planes */
int frbch_cutout_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_cutout_params* par,
                      const frbch_cutout_cand* cands, uint32_t ncand, int device, float* ft, uint32_t* ft_hits, float* dt,
                      uint32_t* dt_hits, uint32_t* kernel_used, char* err, size_t err_cap);
/* Which kernel frbch_cutout_device takes for these arguments (host only, nothing runs): 1 = the LDS kernel, 0 = the
 * generic one, < 0 = refused; only the ADDRESS of d_rows is examined. */
int frbch_cutout_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_cutout_params* par,
                        const frbch_cutout_cand* cands, uint32_t ncand);

/* ---- burst polarisation: spectra of every product, rotation measure synthesis ------------------------
 * What a full-Stokes file (pol_mode 4 / 5 above) is written for: the spectra of a burst in all nifs products, and from Q and
 * U the Faraday dispersion function F(phi), its peak (the rotation measure) and the position angle.  The conventions are
 * this library's own, restated in numpy in tests/rm_oracle.py; every result but frbch_rm_peaks' libm calls is reproducible
 * to the bit, and the transform itself is integer arithmetic, exact in any order of summation.
 *
 * 1. Burst spectra.  Candidate i: on_lo = sample - width / 2 (integer division, signed 64 bit); the on-pulse rows are
 *    on_lo .. on_lo + width - 1 at the top of the band; the off-pulse windows are the off_len rows that end off_gap rows
 *    before on_lo (on_lo - off_gap - off_len .. on_lo - off_gap - 1) and the off_len rows that start off_gap rows behind
 *    the last on-pulse row (on_lo + width + off_gap ..).  Channel c is read at row s + n_c(dm), n_c exactly as
 *    frbch_dedisperse_* compute it; a row outside 0 .. nrows - 1 is absent, adds nothing and is not counted.  For every
 *    product p < nifs and channel c (frbch_burst_sums, [ncand][nifs][nchan]):
 *      on_sum = sum of the on-pulse samples, off_sum / off_sumsq = sum of x / of x x over both off-pulse windows,
 *      on_hits / off_hits = the numbers of present rows.
 *    8- / 16-bit rows: every sum is exact in any order (width <= 65536, off_len <= 2^20: 65535^2 2^21 < 2^53).  float32
 *    rows: double sums in ascending row order (the earlier off window, then the later one), x x rounded before it is added.
 *    Derived on the host in double, every operation rounded on its own (no FMA), g = gain[p][c] (NULL: 1):
 *      spec[i][p][c]  = (float)((on_sum / on_hits - off_sum / off_hits) * g)
 *      var_off        = (off_sumsq - off_sum off_sum / off_hits) / (off_hits - 1), a negative value counts as 0
 *      noise[i][p][c] = (float)(sqrt(var_off / on_hits) * |g|)
 *    used[i][c] = 1 unless, in any product, on_hits = 0, off_hits < 2, or spec or noise (as float) is not finite; an unused
 *    channel has spec = noise = 0 in every product.  products = FRBCH_BURST_COHERENCY (file order PP, QQ, Re, Im; needs
 *    nifs = 4): afterwards, in float, I = PP + QQ, Q = 2 Re, U = 2 Im, V = PP - QQ (the relation of pol_mode 5 above), and
 *    noise_I = noise_V = (float)sqrt((double)nPP nPP + (double)nQQ nQQ), noise_Q = 2 nRe, noise_U = 2 nIm; a channel whose
 *    converted values are not finite becomes unused.  FRBCH_BURST_STOKES (0) leaves the products as they are.
 *    *kernel_used: 1 = the fast kernel (8- / 16-bit rows, nifs <= 4, whole 64-byte channel tiles, d_rows and the row pitch
 *    16-byte aligned), 0 = the generic one (one thread per (candidate, product, channel)); both give the same bits.
 *    FRBCH_E_ARG: a wrong `size`, products > 1 (or 1 with nifs != 4), ncand outside 1..4096, width 0 or above 65536,
 *    off_len < 2 or above 2^20, a DM outside [0, 1e5), a delay beyond 2^30 samples, ncand * nchan > 2^26, ncand * nifs > 65535.
 *
 * 2. RM synthesis of q[ncand][nchan], u[ncand][nchan] (float32) over the channels with used[i][c] != 0.
 *    Host, double, ascending c, every operation rounded on its own:
 *      f_c = fch1 + c foff (MHz);  l2_c = (299.792458 / f_c)^2 (m^2);  N_i = the number of used channels;
 *      l0_i = (sum over used c of l2_c) / N_i;  a_ic = (l2_c - l0_i) / pi  (turns per rad m^-2).
 *    Phase in 64-bit fixed point, 2^64 = one turn; frac(x) = x - floor(x), and a product frac(x) 2^64 of 2^64 counts as 0:
 *      P0_ic = (uint64)(frac(phi_lo a_ic) 2^64),  D_ic = (uint64)(frac(dphi a_ic) 2^64),
 *      ph_ick = P0_ic + k D_ic mod 2^64,  table index j = ((ph + 2^49) >> 50) mod 2^14   (phi_k = phi_lo + k dphi).
 *    Table (frbch_rm_table, 16384 int32): C[j] = (int32)rint(cos(2 pi j / 2^14) 2^22) for j = 0 .. 4096 in double, with
 *    C[4096] = 0; C[8192 - j] = -C[j], C[8192 + j] = -C[j], C[16384 - j] = C[j]: the symmetry is exact.  S[j] = C[(j - 4096)
 *    mod 2^14].
 *    Quantisation per candidate: m = the largest |q_c|, |u_c| over used channels = f 2^e, f in [0.5, 1) (frexp);
 *      Qi_c = (int32)rintf(q_c 2^(23 - e)), Ui_c likewise (the scaling by a power of two is exact, ties to even).
 *    Transform, exact in int64 (2^23 2^22 2 2^14 = 2^60):
 *      Re_ik = sum over used c of (Qi C[j] + Ui S[j]),  Im_ik = sum over used c of (Ui C[j] - Qi S[j]),
 *    that is (q + i u) exp(-2 i phi_k (l2_c - l0_i)).  F[i][k] = ((float)((double)Re inv_i), (float)((double)Im inv_i)),
 *    inv_i = 1 / (2^(23 - e) 2^22 N_i) in double.  m = 0 or N_i = 0: F = 0 for that candidate.
 *    Two costs: the phase is quantised to 2^-14 turn (at most 1.9e-4 rad off), the spectra to 2^-23 of their largest value.
 *    The RMSF is the transform of q = used, u = 0; its value at phi = 0 is exactly 1.
 *    kernel_used[2] (may be NULL): the form (1 = the fast kernel: table in the LDS, lanes along k, channels split over
 *    kernel_used[1] workgroups whose int64 partials a second kernel joins; taken for nphi >= 64 and an 8-byte aligned d_F;
 *    0 = the generic one, one thread per (i, k), split 1).  Both give the same bits.  FRBCH_E_ARG: a wrong `size`, nchan > 16384, ncand outside 1..4096, nphi outside
 *    1..2^20, ncand * nphi > 2^26, dphi <= 0 or not finite, |phi_lo| or |phi_lo + nphi dphi| above 1e7, a q or u that is
 *    not finite in a used channel.
 *
 * 3. Peaks (frbch_rm_peaks, host only).  P_k = re re + im im in double; kp = the first largest k.  With 0 < kp < nphi - 1,
 *    y- = P[kp-1], y0 = P[kp], y+ = P[kp+1], den = y- - 2 y0 + y+ < 0:  delta = 0.5 (y- - y+) / den,
 *    rm = phi_lo + (kp + delta) dphi,  peak = sqrt(y0 - 0.25 (y- - y+) delta),  fitted = 1;  otherwise rm = phi_lo + kp dphi,
 *    peak = sqrt(y0), fitted = 0.  pa0 = atan2(im, re) / 2 at kp (rad);  sigma_f = sqrt(sum over used c of (noise_q^2 +
 *    noise_u^2) / 2) / N;  snr = sqrt(P[kp]) / sigma_f (0 when sigma_f = 0);  fwhm = 2 sqrt(3) / (l2_max - l2_min) over
 *    used channels;  rm_err = fwhm / (2 snr).  noise_q / noise_u may be NULL (sigma_f = snr = rm_err = 0). */
#define FRBCH_BURST_STOKES 0u
#define FRBCH_BURST_COHERENCY 1u
typedef struct frbch_burst_params { uint32_t size, products; } frbch_burst_params;      /* size = sizeof(frbch_burst_params) */
typedef struct frbch_burst_cand {
  double dm;
  int64_t sample;                      /* centre, row index at the top of the band (as frbch_cutout_cand)                  */
  uint32_t width, off_gap, off_len, reserved;
} frbch_burst_cand;
typedef struct frbch_burst_sums { double on_sum, off_sum, off_sumsq; uint32_t on_hits, off_hits; } frbch_burst_sums;
typedef struct frbch_rm_params { uint32_t size, nphi; double phi_lo, dphi; } frbch_rm_params;   /* size = sizeof(frbch_rm_params) */
typedef struct frbch_rm_result {
  double rm, rm_err, peak, pa0, snr, sigma_f, fwhm;
  uint32_t kpeak, nused, fitted, reserved;
} frbch_rm_result;
/* Which kernel frbch_burstspec_device takes (host only, nothing runs): 1 = fast, 0 = generic, < 0 = refused; only the
 * ADDRESS of d_rows is examined. */
int frbch_burstspec_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* par,
                           const frbch_burst_cand* cands, uint32_t ncand);
/* d_rows (never written) and d_sums [ncand][nifs][nchan] are device memory; cands, gain [nifs][nchan] (may be NULL) and
 * the outputs spec, noise [ncand][nifs][nchan] and used [ncand][nchan] are host arrays (each output may be NULL). */
int frbch_burstspec_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* par,
                           const frbch_burst_cand* cands, uint32_t ncand, const float* gain, int device,
                           frbch_burst_sums* d_sums, float* spec, float* noise, uint8_t* used, uint32_t* kernel_used,
                           char* err, size_t err_cap);
/* the same with host pointers: one upload of the rows; sums may be NULL */
int frbch_burstspec_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* par,
                         const frbch_burst_cand* cands, uint32_t ncand, const float* gain, int device, frbch_burst_sums* sums,
                         float* spec, float* noise, uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_rm_table(int32_t* out /* [16384] */);
/* The plan rule (host only, nothing runs): 1 = fast, 0 = generic, < 0 = refused; *nsplit (may be NULL): the channel split.
 * Only the ADDRESS of d_F is examined: the fast kernel stores a trial as one 8-byte piece and wants d_F 8-byte aligned. */
int frbch_rmsynth_kernel(const frbch_fil_desc* fil, const float* d_F, uint32_t ncand, const frbch_rm_params* par, uint32_t* nsplit);
/* d_q, d_u [ncand][nchan] float32, d_used [ncand][nchan] bytes (read, never written) and d_F [ncand][nphi][2] float32 are
 * device memory. */
int frbch_rmsynth_device(const frbch_fil_desc* fil, const float* d_q, const float* d_u, const uint8_t* d_used, uint32_t ncand,
                         const frbch_rm_params* par, int device, float* d_F, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_rmsynth_host(const frbch_fil_desc* fil, const float* q, const float* u, const uint8_t* used, uint32_t ncand,
                       const frbch_rm_params* par, int device, float* F, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_rm_peaks(const frbch_fil_desc* fil, const float* F, const uint8_t* used, const float* noise_q, const float* noise_u,
                   uint32_t ncand, const frbch_rm_params* par, frbch_rm_result* results, char* err, size_t err_cap);
/* The composite: rows -> spectra (step 1; nifs must be 4) -> RM synthesis of Q and U (products 1 and 2 after the
 * conversion) of every candidate -> peaks, in one device scope.  _host: one upload of the rows; _device: rows already in
 * HBM, never written.  flag [nchan] (may be NULL): a non-zero byte clears the channel in `used` of every candidate before
 * the transform.  Outputs are host arrays: spec, noise [ncand][4][nchan], used [ncand][nchan], F [ncand][nphi][2],
 * results [ncand].  kernel_used[3] (may be NULL): the spectra's kernel, the transform's form and its split. */
int frbch_burst_rm_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                          const frbch_burst_cand* cands, uint32_t ncand, const float* gain, const uint8_t* flag,
                          const frbch_rm_params* par, int device, float* spec, float* noise, uint8_t* used, float* F,
                          frbch_rm_result* results, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_burst_rm_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                        const frbch_burst_cand* cands, uint32_t ncand, const float* gain, const uint8_t* flag,
                        const frbch_rm_params* par, int device, float* spec, float* noise, uint8_t* used, float* F,
                        frbch_rm_result* results, uint32_t* kernel_used, char* err, size_t err_cap);

/* ---- polarisation calibration: the delay x RM transform ------------------------------------------------
 * Dual circular feeds: a cable or sampler delay tau between the R and L paths multiplies Q + iU by exp(2 pi i f tau), a phase
 * ramp across the band that RM synthesis cannot tell from Faraday rotation (at 1.2 - 1.5 GHz the ridge of |F|^2 in the
 * (RM, tau) plane runs at about +43 rad m^-2 per nanosecond; to first order pi f^3 / (2 c^2)).  A calibrator of known RM is
 * searched over tau (and a narrow range of RM), and the delay found is taken out of the target's bursts (frbch_polprof_cal_*
 * below; this transform at ntau = 1, tau_lo = tau).  Which feed lags for positive tau depends on the backend's sign
 * convention, which is not pinned here: the correction is consistent with the search, and that is all it needs to be.
 * Absolute PA calibration is out of scope: psi below is twice the PA plus the R/L phase offset, which cannot be separated.
 * tests/polcal_oracle.py restates what follows in numpy.
 *
 * Transform.  f_c, l2_c, used, N_i, l0_i, a_ic, frac(), the fix to 2^64, the table C[] / S[], the index rule, the
 * quantisation Qi / Ui and inv_i are those of step 2 of the burst polarisation section, unchanged.  New, on the host in
 * double, ascending c, every operation rounded on its own:
 *      f0_i = (sum over used c of f_c) / N_i;   b_ic = f_c - f0_i  (MHz; tau is in MICROSECONDS, so tau b is in turns);
 *      T0_ic = (uint64)(frac(tau_lo b_ic) 2^64),  E_ic = (uint64)(frac(dtau b_ic) 2^64),
 *      ph_ickm = P0_ic + k D_ic + T0_ic + m E_ic mod 2^64   (tau_m = tau_lo + m dtau);
 *    Re, Im are the sums of step 2 at that phase, that is (q + i u) exp(-2 i phi_k (l2_c - l0_i)) exp(-2 pi i tau_m (f_c -
 *    f0_i)), exact in int64 in any order (the same 2^60 bound);  F[ncand][ntau][nphi][2] float32 through inv_i.
 *    ntau = 1, tau_lo = 0 gives the bits of frbch_rmsynth_* on the same phi grid.
 *    kernel_used[2] (may be NULL): the form (1 = the fast kernel: table in the LDS, lanes along k, a tile of tau trials in
 *    registers next to each thread's k trials, channels split over kernel_used[1] workgroups whose int64 partials a second
 *    kernel joins; taken for nphi >= 64 and an 8-byte aligned d_F; 0 = the generic one, one thread per (i, m, k), split 1).
 *    Both give the same bits.  FRBCH_E_ARG: every refusal of step 2 above, a wrong `size`, ntau outside 1..4096,
 *    ncand * ntau * nphi > 2^26, dtau <= 0 or not finite, |tau_lo| or |tau_lo + ntau dtau| above 100.
 *
 * Peaks (frbch_rmdelay_peaks, host only, double, no FMA).  Per candidate P[m][k] = re re + im im; (mp, kp) = the first
 *    largest in row-major order.  Along each axis on its own the parabola of step 3 (interior and den < 0: delta = 0.5 (y- -
 *    y+) / den, fitted = 1; else the grid value): tau = tau_lo + (mp + delta_m) dtau, rm = phi_lo + (kp + delta_k) dphi.
 *    peak = sqrt(P[mp][kp]);  psi = atan2(im, re) there;  sigma_f, snr, fwhm, rm_err as in step 3;  fwhm_tau = 2 sqrt(3) /
 *    (pi (f_max - f_min)) over the used channels;  tau_err = fwhm_tau / (2 snr).
 *    Ridge: k_m = the first largest k of row m; over the rows with P[m][k_m] >= 0.5 P[mp][kp], in ascending m, the
 *    least-squares line of phi_{k_m} on tau_m:  n = nridge, mt = (sum tau) / n, mf = (sum phi) / n, sxx = sum (tau - mt)^2,
 *    sxy = sum (tau - mt)(phi - mf), ridge_slope = sxy / sxx (rad m^-2 per microsecond; 0 if nridge < 2 or sxx = 0): what an
 *    error in the delay does to an RM.
 *    results[ncand] (one extra record), several pulses of one calibrator (one tau and RM, a PA each):  Psum[m][k] = sum over
 *    i of P_i[m][k] / sigma_f_i^2 in ascending i, candidates with sigma_f = 0 or nused = 0 skipped; the same peak and ridge
 *    rule on Psum; there peak = snr = sqrt(Psum[mp][kp]), sigma_f = 1, psi = 0, nused = the number of candidates that
 *    entered, fwhm and fwhm_tau over the channels used by any of them; all 0 if none entered. */
typedef struct frbch_rmd_params { uint32_t size, nphi, ntau, reserved; double phi_lo, dphi, tau_lo, dtau; } frbch_rmd_params;   /* size = sizeof(frbch_rmd_params) */
typedef struct frbch_rmd_result {
  double tau, tau_err, rm, rm_err, peak, psi, snr, sigma_f, fwhm, fwhm_tau, ridge_slope;
  uint32_t mpeak, kpeak, nused, fitted_tau, fitted_rm, nridge;
} frbch_rmd_result;
/* The plan rule (host only, nothing runs): 1 = fast, 0 = generic, < 0 = refused; *nsplit (may be NULL): the channel split.
 * Only the ADDRESS of d_F is examined. */
int frbch_rmdelay_kernel(const frbch_fil_desc* fil, const float* d_F, uint32_t ncand, const frbch_rmd_params* par, uint32_t* nsplit);
/* d_q, d_u [ncand][nchan] float32, d_used [ncand][nchan] bytes (read, never written) and d_F [ncand][ntau][nphi][2] float32
 * are device memory. */
int frbch_rmdelay_device(const frbch_fil_desc* fil, const float* d_q, const float* d_u, const uint8_t* d_used, uint32_t ncand,
                         const frbch_rmd_params* par, int device, float* d_F, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_rmdelay_host(const frbch_fil_desc* fil, const float* q, const float* u, const uint8_t* used, uint32_t ncand,
                       const frbch_rmd_params* par, int device, float* F, uint32_t* kernel_used, char* err, size_t err_cap);
/* results [ncand + 1]: the candidates, then the combined record */
int frbch_rmdelay_peaks(const frbch_fil_desc* fil, const float* F, const uint8_t* used, const float* noise_q, const float* noise_u,
                        uint32_t ncand, const frbch_rmd_params* par, frbch_rmd_result* results, char* err, size_t err_cap);
/* The composite: rows -> spectra (step 1 of the burst polarisation section; nifs must be 4) -> `flag` -> the delay x RM
 * transform of Q and U -> peaks and the combined record, in one device scope (_host: one upload of the rows).  The arguments
 * are those of frbch_burst_rm_*, with F [ncand][ntau][nphi][2] and results [ncand + 1].  kernel_used[3] (may be NULL): the
 * spectra's kernel, the transform's form and its split. */
int frbch_burst_polcal_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                              const frbch_burst_cand* cands, uint32_t ncand, const float* gain, const uint8_t* flag,
                              const frbch_rmd_params* par, int device, float* spec, float* noise, uint8_t* used, float* F,
                              frbch_rmd_result* results, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_burst_polcal_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                            const frbch_burst_cand* cands, uint32_t ncand, const float* gain, const uint8_t* flag,
                            const frbch_rmd_params* par, int device, float* spec, float* noise, uint8_t* used, float* F,
                            frbch_rmd_result* results, uint32_t* kernel_used, char* err, size_t err_cap);

/* ---- polarisation profile of a burst: derotated I, L, V and PA per time bin ---------------------------
 * What an RM is measured for: the burst against time at its DM, Q and U of every channel rotated back by the RM and summed
 * over the band.  n_c(dm), the windows, frbch_burst_sums, used, l2_c, the table C[] / S[] and frac() are those of the burst
 * polarisation section above; tests/polprof_oracle.py restates what follows in numpy.  Rows must be 8 or 16 bit and nifs 4:
 * the fixed-point scale below needs an a-priori bound on the samples, which float32 rows do not have.
 *
 * Window.  Candidate i: t0_i = sample - (nbin / 2) tfactor (integer division, signed 64 bit).  Bin j < nbin holds the rows
 *    t0_i + j tfactor + u, u < tfactor, at the top of the band; channel c is read n_c(dm) rows later; a row outside
 *    0 .. nrows - 1 is absent, adds nothing and is not counted.
 *
 * Host preparation (double, ascending c, every operation rounded on its own):
 *    the burst sums of the candidates (step 1 above, the same kernel), used[i][c] by its rule (gains included), then
 *    used[i][c] = 0 where flag[c] != 0;  N_i = the number of used channels;
 *    mean_pc = off_sum / off_hits;  g_pc = gain[p][c] (NULL: 1);  gmax_i = the largest |g_pc| over used c and p < 4;
 *    M_i = (double)tfactor 2^nbits gmax_i = f 2^e, f in [0.5, 1) (frexp);  k_i = 22 - e;
 *    N_i = 0 or gmax_i = 0: every acc, hit and bin of the candidate is 0, and of its result only nused and on_lo_bin /
 *    on_hi_bin are set.
 *    lref_i = l0_i of step 2 above (ref = FRBCH_PROF_REF_MEAN) or 0 (FRBCH_PROF_REF_ZERO: the PA at infinite frequency);
 *    a_ic = (l2_c - lref_i) / pi;  ph_ic = (uint64)(frac(rm_i a_ic) 2^64), a product of 2^64 counts as 0;
 *    j_ic = ((ph_ic + 2^49) >> 50) mod 2^14;  Cc_ic = C[j_ic], Sc_ic = S[j_ic].
 *
 * Device.  For every used c and every bin j with h > 0, h = the number of present rows of the bin in channel c (the same
 *    in all four products):
 *      S_p = the integer sum of the present samples of product p (exact: 512 x 65535 < 2^25);
 *      x_p = ((double)S_p - (double)h mean_pc) g_pc   (three roundings, no FMA);
 *      coherency order: xI = x0 + x1, xQ = 2 x2, xU = 2 x3, xV = x0 - x1;  Stokes order: as they are;
 *      X_p = (int64)rint(x_p 2^k_i), ties to even (the scaling by a power of two is exact);
 *      acc[i][j] += (X_I,  X_Q Cc + X_U Sc,  X_U Cc - X_Q Sc,  X_V);   hits[i][j] += h.
 *    |x_p| <= tfactor 2^nbits gmax < 2^e, so |X| <= 2^22 (2^23 after the coherency combinations) and |C| <= 2^22: at most
 *    2^46 per channel and 2^60 over nchan <= 16384 channels.  acc (int64 [ncand][nbin][4]: I, Re, Im, V) and hits (uint32
 *    [ncand][nbin]) are exact in any order of summation: both kernels and the restatement give the same bits.
 *
 * Host derivation into frbch_prof_bin [ncand][nbin] (double, every operation rounded on its own; 0 where hits = 0):
 *      I = acc_I 2^-k / hits,  V = acc_V 2^-k / hits,  Q = acc_Re 2^-(k+22) / hits,  U = acc_Im 2^-(k+22) / hits;
 *      L = sqrt(Q Q + U U);  L_db = sqrt(L L - sigma_L^2) where L >= 1.57 sigma_L, else 0;  pa = atan2(U, Q) / 2;
 *      pa_err = sigma_L / (2 L_db) and pa_valid = 1 where L_db > 0, else both 0.
 *    frbch_prof_result [ncand]: w_pc = (g_pc g_pc) var_off_pc (var_off of step 1 above); Stokes order: W_p = w_p; coherency
 *    order: W_I = W_V = w_0 + w_1, W_Q = 4 w_2, W_U = 4 w_3;
 *      sigma_p = sqrt((double)tfactor sum over used c of W_pc) / ((double)N_i (double)tfactor)   (the noise of a complete bin),
 *      sigma_l = sqrt((sigma_q^2 + sigma_u^2) / 2);  nused = N_i;  lref;  k;
 *      on_lo_bin / on_hi_bin = floor((on_lo - t0) / tfactor) and floor((on_lo + width - 1 - t0) / tfactor), each limited to
 *      0 .. nbin - 1: the bins that the candidate's on-pulse window covers.
 *    Only pa goes through libm's atan2.
 *
 * kernel_used[2] (may be NULL): the burst-sums kernel, and the profile kernel: 1 = the fast one (the conditions of the fast
 * burst-sums kernel; one workgroup per (64-byte channel tile, run of bins, candidate) stages the rows its bins need -- the
 * run plus the tile's delay spread -- into the LDS, one thread per (channel, bin), a join adds the tiles), 0 = the generic
 * one (one thread per (candidate, bin)).  A tile whose delay spread leaves no room for one bin in the LDS (tfactor + spread >
 * 256 rows) sends the whole call to the generic kernel, and so do tile partials of more than 2^30 bytes (ncand x tiles x nbin
 * x 36).  Both give the same bits.
 * FRBCH_E_ARG: a wrong `size`, nifs != 4, float rows, nbin outside 1..1024, tfactor outside 1..512, ref > 1, nchan > 16384,
 * ncand outside 1..4096, ncand * nbin > 2^22, an rm that is not finite or beyond 1e7 in size, and every refusal of step 1. */
#define FRBCH_PROF_REF_MEAN 0u
#define FRBCH_PROF_REF_ZERO 1u
typedef struct frbch_prof_params { uint32_t size, nbin, tfactor, ref, reserved; } frbch_prof_params;   /* size = sizeof(frbch_prof_params) */
typedef struct frbch_prof_bin { double i, q, u, v, l, l_db, pa, pa_err; uint32_t hits, pa_valid; } frbch_prof_bin;
typedef struct frbch_prof_result {
  double sigma_i, sigma_q, sigma_u, sigma_v, sigma_l, lref;
  int32_t k;
  uint32_t nused, on_lo_bin, on_hi_bin;
} frbch_prof_result;
/* The plan rule (host only, nothing runs): 1 = fast, 0 = generic, < 0 = refused; only the ADDRESS of d_rows is examined. */
int frbch_polprof_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                         const frbch_burst_cand* cands, uint32_t ncand, const frbch_prof_params* par);
/* d_rows is device memory, never written; everything else is host memory: rm [ncand], gain [4][nchan] and flag [nchan] (each
 * may be NULL), and the outputs acc [ncand][nbin][4], hits [ncand][nbin], bins [ncand][nbin], results [ncand], used
 * [ncand][nchan] (each may be NULL).  One device scope. */
int frbch_polprof_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                         const frbch_burst_cand* cands, uint32_t ncand, const double* rm, const float* gain, const uint8_t* flag,
                         const frbch_prof_params* par, int device, int64_t* acc, uint32_t* hits, frbch_prof_bin* bins,
                         frbch_prof_result* results, uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap);
/* the same with host rows: one upload */
int frbch_polprof_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                       const frbch_burst_cand* cands, uint32_t ncand, const double* rm, const float* gain, const uint8_t* flag,
                       const frbch_prof_params* par, int device, int64_t* acc, uint32_t* hits, frbch_prof_bin* bins,
                       frbch_prof_result* results, uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap);
/* The same with the R/L delay of the polarisation calibration section taken out: tau [ncand] (microseconds; NULL: none, the
 * bits of the calls above, which pass NULL).  Only the host preparation changes:
 *    ph_ic = fix(rm_i a_ic) + fix(tau_i b_ic) mod 2^64,  b_ic = f_c - f0_i as defined there, for either `ref`.
 * FRBCH_E_ARG besides: a tau that is not finite or above 100 in size. */
int frbch_polprof_cal_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                             const frbch_burst_cand* cands, uint32_t ncand, const double* rm, const double* tau, const float* gain,
                             const uint8_t* flag, const frbch_prof_params* par, int device, int64_t* acc, uint32_t* hits,
                             frbch_prof_bin* bins, frbch_prof_result* results, uint8_t* used, uint32_t* kernel_used, char* err,
                             size_t err_cap);
int frbch_polprof_cal_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                           const frbch_burst_cand* cands, uint32_t ncand, const double* rm, const double* tau, const float* gain,
                           const uint8_t* flag, const frbch_prof_params* par, int device, int64_t* acc, uint32_t* hits,
                           frbch_prof_bin* bins, frbch_prof_result* results, uint8_t* used, uint32_t* kernel_used, char* err,
                           size_t err_cap);

/* ---- DM of a burst: fine DM scan, S/N and structure maxima -------------------------------------------
 * The stages above take the DM of a burst as given; this one measures it: the burst's band-summed, noise-weighted profile at
 * ntrial DMs about cand.dm (the DM-time "bow tie"), and from it the DM of the largest boxcar S/N and the DM of the most
 * structure, each with a least-squares parabola over the peak of its curve.  frbch_burst_cand, frbch_burst_params, n_c(.),
 * the windows, frbch_burst_sums and "a row outside 0 .. nrows - 1 is absent" are those of the burst polarisation section
 * above; tests/dmscan_oracle.py restates what follows in numpy.  Rows must be 8 or 16 bit: the fixed-point scale below needs
 * an a-priori bound on the samples, which float32 rows do not have.
 *
 * Trials.  kc = ntrial / 2;  dm_k = cand.dm + ((double)k - (double)kc) ddm, every operation rounded on its own (ntrial = 1:
 *    dm_0 = cand.dm, ddm is not looked at).  Channel c of trial k is read n_c(dm_k) rows later.
 * Window.  t0_i = sample - (nbin / 2) tfactor (integer division, signed 64 bit).  Bin j < nbin holds the rows t0_i + j tfactor
 *    + u, u < tfactor, at the top of the band, which has delay 0 at every trial: `sample` stays put and the bow tie is centred.
 *
 * Host preparation (double, ascending c, every operation rounded on its own):
 *    the burst sums of the candidates at cand.dm (step 1 of the burst polarisation section, the same kernel).  Products read:
 *    FRBCH_BURST_STOKES: P = {fil->product} (a one-product file works); FRBCH_BURST_COHERENCY (needs nifs = 4): P = {0, 1}.
 *    mean_pc = off_sum / off_hits;  var_pc = var_off of step 1;  mean_c = the sum over p in P of mean_pc, var_c likewise
 *    (ascending p);  used[i][c] = 1 unless on_hits = 0 or off_hits < 2 in a product of P (step 1's rule on the products read:
 *    with integer rows and no gains nothing there can be non-finite), or var_c is not > 0, or flag[c] != 0.
 *    w_c = 1 / sqrt(var_c): every used channel has unit off-pulse variance per row.  N_i = the number of used channels;
 *    wmax_i = the largest w_c over them;  M_i = (double)tfactor 2^nbits wmax_i, doubled in coherency order, = f 2^e, f in
 *    [0.5, 1) (frexp);  k_i = 40 - e.  N_i = 0: every acc, hit, curve value and result field of the candidate is 0.
 *
 * Device.  For every used c, trial k and bin j with h > 0, h = the number of present rows of the bin in channel c at dm_k:
 *      S = the integer sum of the present samples over the products of P (exact: 2 x 512 x 65535 < 2^27);
 *      x = ((double)S - (double)h mean_c) w_c   (three roundings, no FMA);
 *      X = (int64)rint(x 2^k_i), ties to even (the scaling by a power of two is exact);
 *      acc[i][k][j] += X;   hits[i][k][j] += h.
 *    |x| <= tfactor 2^nbits w_c (twice that in coherency order) < 2^e, so |X| <= 2^40 and |acc| <= 2^54 over nchan <= 16384:
 *    acc (int64 [ncand][ntrial][nbin]) and hits (uint32, the same shape) are exact in any order of summation; both kernels
 *    and the restatement give the same bits.
 *
 * Peaks (frbch_dmscan_peaks, host only, double, every operation rounded on its own; sqrt is the only function called).
 *    Boxcar of w bins at j <= nbin - w: A = the sum of acc[i][k][j .. j + w - 1], H = the sum of the hits (integers, exact);
 *      B(w, j) = ((double)A 2^-k_i) / sqrt((double)H), 0 where H = 0.
 *    snr[i][k] = the first largest B over the listed widths (in their order, which must ascend) and j ascending, with its
 *      width and bin.
 *    Structure, s = smooth, nbin > 1: z_j = B(s, j);  struct[i][k] = (the sum over ascending j < nbin - s of (z_{j+1} - z_j)^2)
 *      - (2 (double)(nbin - s)) / (double)s; the term taken off is the expectation of the sum for unit-variance noise.
 *      nbin = 1: struct = 0, smooth is not looked at, and the structure DM is not fitted.
 *    Fit of a curve v[0 .. ntrial - 1] (snr, then struct): kp = the first largest trial;  thr = fit_frac v[kp];  lo .. hi = the
 *      contiguous trials about kp with v >= thr;  n = hi - lo + 1.  With x = k - kp:  S_m = the sums of x^m, m = 0 .. 4, in
 *      int64 and then converted;  T_0 = sum v, T_1 = sum (double)x v, T_2 = sum (double)(x x) v (ascending k, each product
 *      rounded before it is added);
 *        m0 = S2 S0 - S1 S1,  m1 = S3 S0 - S1 S2,  m2 = S3 S1 - S2 S2,  D  = (S4 m0 - S3 m1) + S2 m2;
 *        p1 = T1 S0 - S1 T0,  p2 = T1 S1 - S2 T0,                       Da = (T2 m0 - S3 p1) + S2 p2;
 *        p3 = S3 T0 - S2 T1,                                           Db = (S4 p1 - T2 m1) + S2 p3;
 *        a = Da / D,  b = Db / D,  vertex = (-b) / (2 a),  dm = dm_kp + vertex ddm,  fitted = 1
 *      (y = a x^2 + b x + c by the normal equations, Cramer's rule).  Not fitted -- dm = dm_kp, fitted = 0 -- where v[kp] is
 *      not > 0, n < 3, lo = 0 or hi = ntrial - 1 (the peak is not bracketed), or a is not < 0.
 *    dm_snr_err = sqrt(-1 / a) ddm of the fitted S/N parabola: the half-width at which it lies 1 below its vertex (0 where not
 *    fitted).  The structure DM gets no error: its curve is not in units of a variance, and none is claimed.
 *    frbch_dmscan_result: for each curve the peak's trial, the S/N, width and bin of that trial, the number of points n and
 *    `fitted`; struct_peak = struct at its peak;  k = k_i;  nused = N_i.
 *
 * frbch_dm_sample_step: tsamp / ((1 / 2.41e-4) (f_lo^-2 - f_hi^-2)), f_lo / f_hi the lowest and highest channel frequency:
 * the change of DM that moves the bottom of the band by one row (0 for a bad descriptor or one channel).
 *
 * kernel_used[2] (may be NULL): the burst-sums kernel, and the scan kernel: 1 = the fast one (the conditions of the fast
 * burst-sums kernel and tfactor <= 256; one workgroup per (64-byte channel tile, run of bins, run of trials, candidate)
 * stages the rows that its bins need over the delay range of its tile and trials into 64 KiB of the LDS once and forms the
 * terms of all its trials from there; a join adds the tiles), 0 = the generic one (one thread per (candidate, trial, bin)).
 * The trial run is the largest of 16, 8, 4, 2, 1 (at most ntrial) for which every (candidate, tile, run) leaves room for one
 * bin: tfactor + delay range <= 1024 rows (512 in coherency order, which stages two products); no such run, or tile partials
 * of more than 2^30 bytes (ncand x tiles x ntrial x nbin x 12), send the whole call to the generic kernel.  Both give the
 * same bits.
 * FRBCH_E_ARG (outputs untouched): a wrong `size`, ntrial outside 1..4096, nbin outside 1..1024, tfactor outside 1..512, ddm
 * not finite or <= 0 (ntrial > 1), a dm_k outside [0, 1e5), float rows, coherency order without nifs = 4, nchan > 16384, ncand
 * outside 1..4096, ncand * ntrial * nchan > 2^26, ncand * ntrial * nbin > 2^24, nwidth outside 1..16, a width outside 1..nbin
 * or not above the one before it, smooth outside 1..nbin - 1 (nbin > 1), fit_frac outside (0, 1), and every refusal of step 1. */
typedef struct frbch_dmscan_params { uint32_t size, ntrial, nbin, tfactor; double ddm; } frbch_dmscan_params;   /* size = sizeof(frbch_dmscan_params) */
typedef struct frbch_dmscan_peak_params {
  uint32_t size, nwidth;               /* size = sizeof(frbch_dmscan_peak_params) */
  uint32_t widths[16];                 /* boxcar widths in bins, ascending; the first nwidth count */
  uint32_t smooth, reserved;
  double fit_frac;
} frbch_dmscan_peak_params;
typedef struct frbch_dmscan_result {
  double dm_snr, dm_snr_err, dm_struct;
  double snr_peak, struct_peak, snr_at_struct;   /* snr[k_snr], struct[k_struct], snr[k_struct] */
  uint32_t k_snr, width_snr, bin_snr, nfit_snr, fitted_snr;
  uint32_t k_struct, width_struct, bin_struct, nfit_struct, fitted_struct;
  int32_t k;
  uint32_t nused;
} frbch_dmscan_result;
double frbch_dm_sample_step(const frbch_fil_desc* fil);
/* The plan rule (host only, nothing runs): 1 = fast, 0 = generic, < 0 = refused; only the ADDRESS of d_rows is examined. */
int frbch_dmscan_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                        const frbch_burst_cand* cands, uint32_t ncand, const frbch_dmscan_params* par);
/* Host only: snr, strc [ncand][ntrial] (double), width, bin [ncand][ntrial] (uint32) and results [ncand] from acc and hits
 * [ncand][ntrial][nbin], k and nused [ncand] (what frbch_dmscan_* put into their results); every output may be NULL. */
int frbch_dmscan_peaks(const frbch_dmscan_params* par, const frbch_dmscan_peak_params* pk, const frbch_burst_cand* cands,
                       uint32_t ncand, const int32_t* k, const uint32_t* nused, const int64_t* acc, const uint32_t* hits,
                       double* snr, double* strc, uint32_t* width, uint32_t* bin, frbch_dmscan_result* results, char* err,
                       size_t err_cap);
/* d_rows is device memory, never written; everything else is host memory: flag [nchan] (may be NULL) and the outputs acc, hits
 * [ncand][ntrial][nbin], snr, strc [ncand][ntrial], results [ncand], used [ncand][nchan] (each may be NULL).  One device scope. */
int frbch_dmscan_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                        const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_dmscan_params* par,
                        const frbch_dmscan_peak_params* pk, int device, int64_t* acc, uint32_t* hits, double* snr, double* strc,
                        frbch_dmscan_result* results, uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap);
/* the same with host rows: one upload */
int frbch_dmscan_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                      const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_dmscan_params* par,
                      const frbch_dmscan_peak_params* pk, int device, int64_t* acc, uint32_t* hits, double* snr, double* strc,
                      frbch_dmscan_result* results, uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap);

/* ---- structure of a burst: dedispersed dynamic spectrum and its two-dimensional autocorrelation ------------------
 * The stages above sum over the band before they look at a burst.  This one keeps frequency and time: the dedispersed,
 * baseline-free, noise-weighted dynamic spectrum Y of a burst, its two-dimensional autocorrelation (ACF) A, and from A the
 * scintillation bandwidth, the sub-burst duration and the drift of sub-bursts in frequency.  frbch_burst_cand,
 * frbch_burst_params, n_c(.), the windows, frbch_burst_sums and "a row outside 0 .. nrows - 1 is absent" are those of the burst
 * sections above; tests/acf_oracle.py restates what follows in numpy.  Rows must be 8 or 16 bit, for the DM scan's reason.
 *
 * Grid.  ffactor divides nchan, nsub = nchan / ffactor; subband s holds the channels s ffactor .. (s + 1) ffactor - 1.  The
 *    window is the DM scan's: t0_i = sample - (nbin / 2) tfactor; bin j holds the rows t0_i + j tfactor + u, u < tfactor, at
 *    the top of the band; channel c is read n_c(cand.dm) rows later.
 * Host preparation.  Exactly the DM scan's at cand.dm (one function serves both): the burst sums, the products read, mean_c,
 *    var_c, used, flag, w_c = 1 / sqrt(var_c), M_i = (double)tfactor 2^nbits wmax_i (doubled in coherency order; NOT
 *    multiplied by ffactor), k_i = 40 - e.  N_i = 0: every output of the candidate is 0.
 * 1. Dynamic spectrum (device).  Y[i][s][j] (int64) = the sum over the used channels c of subband s with h > 0 present rows in
 *    bin j of X = (int64)rint(((double)S - (double)h mean_c) w_c 2^k_i) -- the DM scan's term, the same function in every
 *    kernel --, yhits[i][s][j] (uint32) = the sum of h.  |X| <= 2^40, so |Y| <= 2^40 ffactor <= 2^54: exact in any order.
 *    Consequence: the sum over s of Y[i][s][j] and of yhits[i][s][j] equals acc[i][0][j] and hits[i][0][j] of frbch_dmscan_*
 *    called with ntrial = 1 on the same arguments, bit for bit.
 *    Complete cells.  nused_s = the used channels of subband s.  A cell is complete when nused_s > 0 and yhits = tfactor
 *    nused_s: every used channel of the subband has all its rows.  mask[i][s][j] = 1 for complete cells, else 0.
 * 2. Quantisation (device).  m_i = the largest |Y| over the complete cells (an integer maximum: order-free); b = the bit
 *    length of m_i (0 for m_i = 0); r_i = max(0, b - 21).  Complete cells: y[i][s][j] (int32) = (Y + 2^(r-1)) >> r (arithmetic
 *    shift) for r > 0 and Y for r = 0; incomplete cells: y = 0.  m_i < 2^b gives |y| <= 2^21 (the rounding can reach 2^21
 *    itself), so a product of two cells is <= 2^42 and a sum over nsub nbin <= 2^20 cells is <= 2^62 < 2^63: int64 sums of
 *    products of y cannot overflow, in any order.  The resolution is 2^-21 of the brightest cell of the burst itself.
 * 3. ACF (device).  For 0 <= df < nlagf and -(nlagt - 1) <= dt <= nlagt - 1:
 *      A[i][df][dt + nlagt - 1] (int64) = the sum over s, j of y[i][s][j] y[i][s + df][j + dt],
 *    over 0 <= s, s + df < nsub, 0 <= j, 0 <= j + dt < nbin.  The other half-plane is A[-df][-dt] = A[df][dt] and is not
 *    stored.  Incomplete cells are zero and drop out.  P[i][df][.] (uint32), the number of complete pairs at a lag, is the
 *    same sum over mask: the same kernel on the 0 / 1 plane.  When every cell of every candidate of the call is complete the
 *    library writes the closed form (nsub - df)(nbin - |dt|) instead; the two are equal.
 *    Direct sums, not an FFT: the sums are exact integers, and the lag window is a small part of the plane.
 *    frbch_acf2d_* are this stage alone on int32 planes y [n][nsub][nbin] with the contract |y| <= 2^21 (n nsub nbin <= 2^24,
 *    nsub nbin <= 2^20, nbin 1..1024, nlagf 1..min(nsub, 1024), nlagt 1..min(nbin, 256), n nlagf (2 nlagt - 1) <= 2^24);
 *    frbch_acf2d_host checks the contract on the host and refuses a plane that breaks it; frbch_acf2d_device cannot look.
 * 4. Derivation (frbch_burstacf_fit, host only; double, every operation rounded on its own, no FMA; this library's own rule,
 *    no error bars are claimed).  q = 2^(-2 (k_i - r_i));  norm[df][dt] = ((double)A q) / (double)P, 0 where P = 0.  The lag
 *    (0, 0) carries the noise variance and is left out of everything below.
 *    Frequency width.  F[df] = norm[df][0].  With nlagf >= 2 and F[1] > 0: the first df >= 2 with F[df] < h, h = F[1] / 2;
 *      x = (double)(df - 1) + (F[df - 1] - h) / (F[df - 1] - F[df]), the half-width at half maximum in subbands;
 *      width_f_mhz = x ((double)ffactor |foff|), fitted_f = 1.  No such df below nlagf: x = (double)(nlagf - 1), the last lag
 *      looked at as it is, fitted_f = 0.  nlagf < 2 or F[1] not > 0: x = 0, fitted_f = 0.
 *    Time width.  The same on T[dt] = norm[0][dt], dt >= 1, with nlagt: width_t_ms = x (((double)tfactor tsamp) 1000).
 *    Drift.  ref = the largest norm over the stored lags other than (0, 0).  w = norm where ref > 0 and norm >= fit_frac ref,
 *      else 0.  Second moments over the mirrored plane, each half counted once and doubled: over H = {df = 0, dt > 0} and
 *      {df > 0, every dt}, df then dt ascending, Mff = 2 sum w (double)(df df), Mtf = 2 sum w (double)(df dt), Mtt = 2 sum w
 *      (double)(dt dt) (the integer products exact in int64, each term rounded before it is added).  Mff > 0:  q = Mtf / Mff
 *      (bins per subband: the regression of time on frequency, the ridge line of a drifting burst);  dt_df = (q (((double)
 *      tfactor tsamp) 1000)) / ((double)ffactor foff), ms per MHz with the sign of foff;  drift = 1 / dt_df (MHz / ms) where
 *      dt_df != 0, else 0;  fitted_d = 1.  Mff not > 0: dt_df = drift = 0, fitted_d = 0.
 *    frbch_acf_result also holds k = k_i, r = r_i, nused = N_i, ncomplete = the number of complete cells, ref, and the moments.
 *
 * kernel_used[3] (may be NULL): the burst-sums kernel, the dynamic-spectrum kernel, the ACF kernel; 1 = fast, 0 = generic.
 *    Dynamic spectrum, fast: the conditions of the fast burst-sums kernel, tfactor <= 256, ffactor a power of two <= the 64
 *    (8 bit) / 32 (16 bit) channels of a 64-byte tile (a shuffle reduction over ffactor lanes) or a multiple of them (the whole
 *    tile by shuffles, a join over the ffactor / 64 tiles of a subband), every (candidate, tile) leaving room for one bin in
 *    the stage (tfactor + delay range <= 1024 rows, 512 in coherency order), and join partials of at most 2^30 bytes (ncand x
 *    tiles x nbin x 12); everything else: generic, one thread per (candidate, subband, bin).
 *    ACF, fast: a workgroup owns a plane, a run of up to 8 df and a slab of subbands, stages the slab's rows and the rows df
 *    further on into 64 KiB of the LDS, every thread owns 8 consecutive dt and walks j with a sliding register window, a join
 *    adds the slabs.  The staging rule places every shape these entry points accept (the smallest slab is 4 rows, at 1024 bins
 *    and 256 lags); the fast kernel is not taken where the partials of the slabs would exceed 2^30 bytes (n x slabs x nlagf x
 *    (2 nlagt - 1) x 8): generic, one thread per (plane, df, dt).  frbch_acf2d_* take `form`: FRBCH_ACF_PLAN = the plan rule
 *    decides, FRBCH_ACF_GENERIC = the generic kernel whatever the rule says (for comparing the two).  Both give the same bits.
 * FRBCH_E_ARG (outputs untouched): a wrong `size`, nbin outside 1..1024, tfactor outside 1..512, ffactor outside 1..nchan or
 * not dividing nchan, nsub nbin > 2^20, ncand nsub nbin > 2^24, nlagf outside 1..min(nsub, 1024), nlagt outside 1..min(nbin,
 * 256), ncand nlagf (2 nlagt - 1) > 2^24, fit_frac outside (0, 1), float rows, coherency order without nifs = 4, nchan > 16384,
 * and every refusal of the burst sums. */
#define FRBCH_ACF_PLAN 0u
#define FRBCH_ACF_GENERIC 1u
typedef struct frbch_acf_params { uint32_t size, nbin, tfactor, ffactor, nlagf, nlagt, reserved[2]; } frbch_acf_params;   /* size = sizeof(frbch_acf_params) */
typedef struct frbch_acf_fit_params { uint32_t size, reserved; double fit_frac; } frbch_acf_fit_params;                   /* size = sizeof(frbch_acf_fit_params) */
typedef struct frbch_acf_result {
  double width_f_mhz, width_t_ms;      /* half-widths at half maximum of the two cuts */
  double dt_df, drift;                 /* ms per MHz, MHz per ms */
  double ref, mff, mtf, mtt;
  int32_t k;
  uint32_t r, nused, ncomplete, fitted_f, fitted_t, fitted_d, reserved;
} frbch_acf_result;
/* The plan rule of the ACF stage (host only, nothing runs): 1 = fast, 0 = generic, < 0 = refused. */
int frbch_acf2d_kernel(uint32_t n, uint32_t nsub, uint32_t nbin, uint32_t nlagf, uint32_t nlagt, uint32_t form);
/* d_y [n][nsub][nbin] int32 and d_A [n][nlagf][2 nlagt - 1] int64 are device memory; d_y is never written.  Synchronised. */
int frbch_acf2d_device(const int32_t* d_y, uint32_t n, uint32_t nsub, uint32_t nbin, uint32_t nlagf, uint32_t nlagt, uint32_t form,
                       int device, int64_t* d_A, uint32_t* kernel_used, char* err, size_t err_cap);
/* the same with host arrays; refuses a plane with a |y| above 2^21 */
int frbch_acf2d_host(const int32_t* y, uint32_t n, uint32_t nsub, uint32_t nbin, uint32_t nlagf, uint32_t nlagt, uint32_t form,
                     int device, int64_t* A, uint32_t* kernel_used, char* err, size_t err_cap);
/* Host only: norm [ncand][nlagf][2 nlagt - 1] (double) and results [ncand] from A (int64) and P (uint32) of that shape and
 * k, r, nused, ncomplete [ncand]; norm and results may be NULL.  Only nchan, foff_mhz and tsamp_s of `fil` are looked at. */
int frbch_burstacf_fit(const frbch_fil_desc* fil, const frbch_acf_params* par, const frbch_acf_fit_params* fp, uint32_t ncand,
                       const int32_t* k, const uint32_t* r, const uint32_t* nused, const uint32_t* ncomplete, const int64_t* A,
                       const uint32_t* P, double* norm, frbch_acf_result* results, char* err, size_t err_cap);
/* The plan rules (host only, nothing runs): 0 and kernel_used[3] filled, or < 0 = refused; only the ADDRESS of d_rows is examined. */
int frbch_burstacf_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                          const frbch_burst_cand* cands, uint32_t ncand, const frbch_acf_params* par, uint32_t* kernel_used);
/* d_rows is device memory, never written; everything else is host memory: flag [nchan] (may be NULL) and the outputs Y (int64),
 * yhits (uint32) [ncand][nsub][nbin], A (int64), P (uint32) [ncand][nlagf][2 nlagt - 1], results [ncand], used [ncand][nchan],
 * kernel_used[3] (each may be NULL).  One device scope. */
int frbch_burstacf_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                          const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_acf_params* par,
                          const frbch_acf_fit_params* fp, int device, int64_t* Y, uint32_t* yhits, int64_t* A, uint32_t* P,
                          frbch_acf_result* results, uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap);
/* the same with host rows: one upload */
int frbch_burstacf_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                        const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_acf_params* par,
                        const frbch_acf_fit_params* fp, int device, int64_t* Y, uint32_t* yhits, int64_t* A, uint32_t* P,
                        frbch_acf_result* results, uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap);

/* ---- scattering of a burst: a bank of scattered Gaussians fitted to every subband, tau(nu) across the band ---------
 * The stages above measure where a burst is and how wide; none fits a pulse SHAPE.  This one fits a Gaussian convolved with
 * a one-sided exponential -- the thin-screen scattering tail -- to every subband of the dedispersed dynamic spectrum by
 * correlating the subband's profile with a bank of templates at every trial arrival bin, and then tau(nu) = tau_ref
 * (nu / nu_ref)^-alpha across the band.  frbch_burst_cand, frbch_burst_params, the window, the host preparation, the dynamic
 * spectrum Y, yhits, the complete cells, the 0 / 1 plane `mask` and the quantised plane y (|y| <= 2^21, shift r_i) are those of
 * the section above -- the same functions, the same bits; tests/scat_oracle.py restates what follows in numpy.
 *
 * Bank (frbch_scat_bank, host only, nothing runs on the device).  sigma_0 = sigma0, sigma_a = sigma_(a-1) rsig, a < nsig;
 *    tau_0 = tau0, tau_b = tau_(b-1) rtau, b < ntau; both in bins, rsig, rtau > 1.  Template k = a ntau + b, K = nsig ntau.
 *    g[j] = exp(-(d d) / (2 (sigma sigma))), d = (double)(j - lead), j < ntap: a Gaussian with its centre at tap `lead`;
 *    e[n] = exp(-(double)n / tau), n >= 0;  f[m] = the sum over n = 0 .. m, ascending from 0.0, of g[m - n] e[n].  Double,
 *    every operation rounded on its own, no FMA; only exp comes from libm.  fmax = the largest f;
 *    p_k[m] (int32) = rint((f[m] / fmax) 32768.0), 0 <= p <= 2^15;  S1_k (int64) = the sum of p;  cum_k[m] (int64), m = 0 ..
 *    ntap, = the sum of p[m'] p[m'] over m' < m (cum[0] = 0);  tail_k = f[ntap - 1] / fmax, the last tap's share of the peak:
 *    a caller sees a truncated tail there.  exp is libm's, so two machines may differ in a last bit of f and, rarely, in a
 *    unit of p: everything below takes the bank as it is, and the Python side takes it from this library.
 * 1. Stage (device; frbch_tbank_* are this stage alone).  For planes y [n][nsub][nbin] (int32) and a bank P [ntemp][ntap] (int32):
 *      C[i][s][k][u] (int64) = the sum over m < ntap of y[i][s][shift0 + u - lead + m] P[k][m],  u < nshift:
 *    the template's Gaussian centre laid on bin shift0 + u.  Terms whose bin lies outside 0 .. nbin - 1 are absent.
 *    Contract: |y| <= 2^21, |P| <= 2^30, ntap <= 1024: every sum is below 2^21 2^30 2^10 = 2^61 and exact in any order.
 *    frbch_tbank_host checks the contract and refuses; frbch_tbank_device cannot look.  Limits: n, nsub >= 1, nbin 1..1024,
 *    ntap 1..1024, lead < ntap, ntemp 1..4096, nshift >= 1, shift0 + nshift <= nbin, n nsub nbin <= 2^24, n nsub ntemp nshift
 *    <= 2^24.  Direct sums, not an FFT: exact integers.
 * 2. Composite (frbch_burstscat_*).  The preparation at cand.dm, Y, yhits, mask, y as above;  C = the stage on y with p;
 *    N[i][s][k][u] (int64) = the stage on the 0 / 1 plane with the squared bank p p (<= 2^30): the template's energy over the
 *    complete cells it covers.  When every cell of every candidate of the call is complete the library writes the closed form
 *    cum_k[hi] - cum_k[lo], lo = max(0, lead - shift0 - u), hi = min(ntap, nbin - (shift0 + u - lead)), instead; the two are
 *    equal.  In the composite the products are small (|C| < 2^46, N < 2^40).
 * 3. Fit (frbch_burstscat_fit, host only; double, every operation rounded on its own, no FMA, fixed loop order, ties to the
 *    lowest index; only log, exp and sqrt come from libm).
 *    Noise scale.  The DM scan's boxcar S/N divides a sum of X 2^-k over H samples by sqrt(H): a term of one row of one used
 *      channel has unit variance.  A complete cell of subband s holds tfactor nused_s of them and y = Y 2^-r, so
 *      v_s = ((double)tfactor (double)nused_s) 2^(2 (k_i - r_i)) is the variance of a complete cell in units of y.
 *      q[s][k][u] = (((double)C (double)C) / (double)N) / v_s, and 0 where N = 0 or C <= 0 or nused_s = 0: the drop of chi^2 of
 *      the least-squares amplitude C / N of template k at shift u (negative amplitudes are not bursts).
 *    Per subband (frbch_scat_sub).  The first largest q over k, then u, ascending; all of q zero: the record stays zero but for
 *      nused and freq_mhz.  sigma, tau (bins) of template k; arrival = (double)(shift0 + u), bins from the window's first;
 *      unit = ((double)tfactor tsamp) 1000: sigma_ms, tau_ms, arrival_ms = the three times unit;  amp = (C / N) 2^(15 - (k_i -
 *      r_i)), the fitted template's peak in the DM scan's units;  area = ((C / N) (double)S1_k) 2^-(k_i - r_i);  snr = sqrt(q).
 *      prof[b] = the largest q over (a, u) at tau_b.  tau_lo / tau_hi (ms) = the smallest / largest tau_b with prof[b] >= q -
 *      1;  bounded_lo = 0 where that is b = 0, bounded_hi = 0 where it is b = ntau - 1, else 1;  dq_unscattered = q - prof[0].
 *    Band (frbch_scat_band).  Subbands with snr >= snr_min take part (nfit of them; none: the record stays zero but for k, r,
 *      nused, nu_ref).  nu_s = fch1 + ((double)(s ffactor) + (double)(ffactor - 1) / 2.0) foff;  nu_ref = fch1 + ((double)(nchan
 *      - 1) / 2.0) foff.  d_s(alpha) = rint(((-alpha) log(nu_s / nu_ref)) / log(rtau)).  For every alpha of the list, in its
 *      order, every b_ref < ntau, every a < nsig, every u < nshift:
 *        Q = the sum over the participating s, ascending from 0.0, of q[s][a ntau + clip(b_ref + d_s(alpha), 0, ntau - 1)][u].
 *      The first largest Q gives alpha, tau_ref = tau_(b_ref), sigma_a, the arrival; nclipped = the participating subbands whose
 *      b_ref + d_s left 0 .. ntau - 1 there.  tau_ref_lo / _hi (ms) = the smallest / largest tau_b whose largest Q over (alpha,
 *      a, u) is >= Q - 1, bounded_lo / _hi as above;  alpha_lo / _hi = the smallest / largest listed alpha whose largest Q over
 *      (b_ref, a, u) is >= Q - 1 (with one alpha: that alpha).  ONE sigma and ONE arrival bin for all subbands is an assumption
 *      of the band fit: a residual DM error or a frequency-dependent width goes into alpha.
 *    No claim beyond these profile intervals: they are the grid points within 1 of the maximum of a chi^2 drop profiled over
 *    the other grid parameters, for the noise scale above; nothing accounts for the grid's step, for correlated noise, or for
 *    a template that does not describe the burst.
 *
 * kernel_used[3] (may be NULL): the burst-sums kernel, the dynamic-spectrum kernel, the template-bank kernel; 1 = fast, 0 =
 *    generic.  Template bank, fast: a workgroup owns a plane, sw <= 8 subbands and a run of templates; it stages the subbands'
 *    lines, zero-padded so that the inner loop has no bounds, and the templates of its run into 64 KiB of the LDS; a thread
 *    owns 8 consecutive shifts of one (subband, template) and walks the taps with a sliding register window; no join.  The
 *    staging rule places every shape these entry points accept; not fast: more than 65535 planes, `form` =
 *    FRBCH_TBANK_GENERIC (one thread per (plane, s, k, u); for comparing the two), the emulator build.  Both give the same bits.
 * FRBCH_E_ARG (outputs untouched): a wrong `size`, the limits of the stage, ntap outside 1..1024, lead >= ntap, nsig ntau
 * outside 1..4096, a grid value that is not finite and positive, rsig or rtau not > 1, sigma0 or tau0 < 0.25, nalpha outside
 * 1..32, an alpha or snr_min that is not finite, and every refusal of the section above. */
#define FRBCH_TBANK_PLAN 0u
#define FRBCH_TBANK_GENERIC 1u
typedef struct frbch_scat_bank_params { uint32_t size, nsig, ntau, ntap, lead, reserved[3]; double sigma0, rsig, tau0, rtau; } frbch_scat_bank_params;
typedef struct frbch_tbank_shape { uint32_t size, nsub, nbin, ntemp, ntap, lead, shift0, nshift; } frbch_tbank_shape;
typedef struct frbch_scat_params { uint32_t size, nbin, tfactor, ffactor, shift0, nshift, reserved[2]; } frbch_scat_params;
typedef struct frbch_scat_fit_params { uint32_t size, nalpha; double snr_min; double alpha[32]; } frbch_scat_fit_params;
typedef struct frbch_scat_sub {
  double sigma, tau, arrival;               /* bins */
  double sigma_ms, tau_ms, arrival_ms;
  double amp, area, snr, q;
  double tau_lo, tau_hi, dq_unscattered;    /* ms, ms, chi^2 */
  double freq_mhz;
  uint32_t k, u, nused, bounded_lo, bounded_hi, reserved;
} frbch_scat_sub;
typedef struct frbch_scat_band {
  double tau_ref, tau_ref_ms, alpha, sigma, sigma_ms, arrival, arrival_ms, q;
  double tau_ref_lo, tau_ref_hi, alpha_lo, alpha_hi;    /* ms, ms */
  double nu_ref_mhz;
  int32_t k;
  uint32_t r, nused, nfit, nclipped, b_ref, a, u, ialpha, bounded_lo, bounded_hi, reserved;
} frbch_scat_band;
/* Host only: p (int32) [K][ntap], s1 (int64) [K], cum (int64) [K][ntap + 1], tail (double) [K], sigma (double) [nsig], tau
 * (double) [ntau]; each may be NULL. */
int frbch_scat_bank(const frbch_scat_bank_params* bp, int32_t* p, int64_t* s1, int64_t* cum, double* tail, double* sigma,
                    double* tau, char* err, size_t err_cap);
/* The plan rule of the stage (host only, nothing runs): 1 = fast, 0 = generic, < 0 = refused. */
int frbch_tbank_kernel(uint32_t n, const frbch_tbank_shape* sh, uint32_t form);
/* d_y [n][nsub][nbin] int32, d_P [ntemp][ntap] int32 and d_C [n][nsub][ntemp][nshift] int64 are device memory; d_y and d_P are
 * never written.  Synchronised. */
int frbch_tbank_device(const int32_t* d_y, const int32_t* d_P, uint32_t n, const frbch_tbank_shape* sh, uint32_t form, int device,
                       int64_t* d_C, uint32_t* kernel_used, char* err, size_t err_cap);
/* the same with host arrays; refuses a |y| above 2^21 or a |P| above 2^30 */
int frbch_tbank_host(const int32_t* y, const int32_t* P, uint32_t n, const frbch_tbank_shape* sh, uint32_t form, int device,
                     int64_t* C, uint32_t* kernel_used, char* err, size_t err_cap);
/* Host only: q [ncand][nsub][K][nshift] (double), sub [ncand][nsub], band [ncand] from C and N (int64) of q's shape, k, r,
 * nused [ncand] and nused_s [ncand][nsub]; q, sub and band may be NULL.  Only nchan, fch1_mhz, foff_mhz and tsamp_s of `fil`
 * are looked at. */
int frbch_burstscat_fit(const frbch_fil_desc* fil, const frbch_scat_params* par, const frbch_scat_bank_params* bp,
                        const frbch_scat_fit_params* fp, uint32_t ncand, const int32_t* k, const uint32_t* r, const uint32_t* nused,
                        const uint32_t* nused_s, const int64_t* C, const int64_t* N, double* q, frbch_scat_sub* sub,
                        frbch_scat_band* band, char* err, size_t err_cap);
/* The plan rules (host only, nothing runs): 0 and kernel_used[3] filled, or < 0 = refused; only the ADDRESS of d_rows is examined. */
int frbch_burstscat_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                           const frbch_burst_cand* cands, uint32_t ncand, const frbch_scat_params* par,
                           const frbch_scat_bank_params* bp, uint32_t* kernel_used);
/* d_rows is device memory, never written; everything else is host memory: flag [nchan] (may be NULL) and the outputs Y (int64),
 * yhits (uint32), y (int32) [ncand][nsub][nbin], C, N (int64) [ncand][nsub][K][nshift], sub [ncand][nsub], band [ncand], used
 * [ncand][nchan], kernel_used[3] (each may be NULL).  One device scope. */
int frbch_burstscat_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                           const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_scat_params* par,
                           const frbch_scat_bank_params* bp, const frbch_scat_fit_params* fp, int device, int64_t* Y,
                           uint32_t* yhits, int32_t* y, int64_t* C, int64_t* N, frbch_scat_sub* sub, frbch_scat_band* band,
                           uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap);
/* the same with host rows: one upload */
int frbch_burstscat_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                         const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_scat_params* par,
                         const frbch_scat_bank_params* bp, const frbch_scat_fit_params* fp, int device, int64_t* Y,
                         uint32_t* yhits, int32_t* y, int64_t* C, int64_t* N, frbch_scat_sub* sub, frbch_scat_band* band,
                         uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap);

/* ---- interference: block statistics, the mask, cleaned rows --------------------------------------
 * The reference carries a flag file through to Heimdall and FETCH (create_config.py:54-56 `-F/--flag`, frb.conf:50,
 * base2fil.sh:226,425-432, submit_job.py:117 `<Tel>.flag_<fmin>-<fmax>MHz_<nchan>chan`) and leaves making one to a person.
 * frbch_rfi_* measure the rows, decide a mask and replace the masked samples IN PLACE: the cleaned rows are ordinary rows,
 * which every entry point above takes unchanged.  The flagging rule is this library's own, rfifind-like [EXT-UNVERIFIED:
 * PRESTO is not in the reference tree]; tests/rfi_oracle.py restates it in numpy and every result is reproducible to the bit.
 *
 * Blocks.  Block b holds the rows [b block_rows, min((b + 1) block_rows, nrows)), n_b of them: a short last block is an
 * ordinary block.  nblk = frbch_rfi_nblk(nrows, block_rows) = ceil(nrows / block_rows); < 0: block_rows outside 1..2^20
 * or nrows = 0.
 * Statistics of product fil->product: stats[b][c] = {S, Q} = {sum x, sum x x} over the rows of block b, 16 bytes a cell.
 * Integer rows: two uint64, exact in any order (65535^2 2^20 < 2^53).  Float rows: two doubles, x = (double)sample,
 * S += x and Q += x * x row by row in ascending order, every operation rounded on its own (no fused multiply-add).
 *
 * The mask, frbch_rfi_mask: host only, double precision, every operation rounded on its own.  `median` of n >= 1 values is
 * 0.5 * (lower middle + upper middle) of the sorted values (the middle one twice when n is odd).
 *  1. Per cell: mean = S / n_b, var = max(0, Q / n_b - mean * mean), std = sqrt(var).  A cell whose mean or std is not
 *     finite is BAD: it is flagged and left out of every median.
 *  2. Per channel, over its non-bad blocks: m_c = median(mean), s_c = median(std), dm_c = 1.4826 * median|mean - m_c|,
 *     ds_c = 1.4826 * median|std - s_c|.
 *  3. A non-bad cell is flagged when |mean - m_c| > t_cell * max(dm_c, s_c / sqrt(n_b)) or
 *     |std - s_c| > t_cell * max(ds_c, s_c / sqrt(2 n_b)): the floors are the sampling scatter of a block's mean and std,
 *     so that quantised data with a zero MAD does not flag itself.
 *  4. A channel is flagged wholly when zap[c] != 0, when s_c == 0 (dead), or when it has no non-bad cell.
 *  5. When t_chan > 0, over the channels step 4 left (at least one): M = median(s_c), D = 1.4826 * median|s_c - M|, and
 *     channel c of them is flagged wholly when |s_c - M| > t_chan * D.
 *  6. A channel not yet flagged is flagged wholly when its flagged cells (steps 1 and 3) number more than
 *     chan_frac * nblk.  Then, over the channels still unflagged, n_u of them: block b is flagged wholly when its flagged
 *     cells among them number more than block_frac * n_u.
 *  7. mask[b][c] = cell flag | chan_flag[c] | blk_flag[b] | prior[b][c].  `prior` is ORed into the result only: it enters
 *     no count and no median.
 *  8. repl[c] = median of mean[b][c] over the cells with mask = 0; none: m_c; not finite: 0.  Integer rows:
 *     floor(repl + 0.5), clamped to 0 .. 2^nbits - 1.
 * Apply: every sample of product fil->product in a cell with mask != 0 becomes repl[c] (float rows: (float)repl[c]; integer
 * rows: a caller's repl[c] below 0 or not a number is taken as 0, one above the largest code as that code); no
 * other byte is written, so other products and unmasked cells keep theirs, and a second apply changes nothing.
 * FRBCH_E_ARG: a wrong `size`, block_rows outside 1..2^20, nrows = 0, nbits not 8 / 16 / 32, product >= nifs, a threshold
 * or fraction x with !(x >= 0) or infinite, a fraction above 1, nblk other than frbch_rfi_nblk(). */
typedef struct frbch_rfi_params {
  uint32_t size, block_rows;           /* = sizeof(frbch_rfi_params); rows per block, 1..2^20                             */
  double t_cell, t_chan;               /* thresholds of steps 3 and 5; t_chan = 0: no step 5                              */
  double chan_frac, block_frac;        /* fractions of step 6, 0..1                                                       */
} frbch_rfi_params;
long frbch_rfi_nblk(uint64_t nrows, uint32_t block_rows);
/* Which kernel frbch_rfi_stats_device takes for these arguments (host only, nothing runs): 1 = the fast kernel (8- / 16-bit
 * rows of whole 64-byte channel tiles, d_rows and the row pitch nifs nchan bytes-per-sample 16-byte aligned), 0 = the
 * generic one (a thread per channel; the only one for float rows), < 0 = refused; only the ADDRESS of d_rows is examined. */
int frbch_rfi_stats_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_rfi_params* par);
/* stats: [nblk][nchan][2] as above; *kernel_used (may be NULL) as frbch_rfi_stats_kernel.  Both kernels give the same bits. */
int frbch_rfi_stats_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                           int device, void* d_stats, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_rfi_stats_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_rfi_params* par, int device,
                         void* stats, uint32_t* kernel_used, char* err, size_t err_cap);
/* zap [nchan] and prior [nblk][nchan] may be NULL; mask [nblk][nchan] receives 0 / 1, repl [nchan], chan_flag [nchan] and
 * blk_flag [nblk] the channels and blocks flagged wholly (0 / 1). */
int frbch_rfi_mask(const frbch_fil_desc* fil, const void* stats, uint32_t nblk, uint64_t nrows, const frbch_rfi_params* par,
                   const uint8_t* zap, const uint8_t* prior, uint8_t* mask, double* repl, uint8_t* chan_flag,
                   uint8_t* blk_flag, char* err, size_t err_cap);
int frbch_rfi_apply_device(const frbch_fil_desc* fil, void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                           const uint8_t* d_mask, const double* d_repl, int device, char* err, size_t err_cap);
int frbch_rfi_apply_host(const frbch_fil_desc* fil, void* rows, uint64_t nrows, const frbch_rfi_params* par,
                         const uint8_t* mask, const double* repl, int device, char* err, size_t err_cap);
/* Statistics, mask and apply on resident rows; zap, mask, repl, chan_flag and blk_flag are HOST arrays as in frbch_rfi_mask
 * (there is no prior).  The _host form uploads the rows, cleans them and downloads them into `rows` again. */
int frbch_rfi_clean_device(const frbch_fil_desc* fil, void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                           const uint8_t* zap, int device, uint8_t* mask, double* repl, uint8_t* chan_flag, uint8_t* blk_flag,
                           uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_rfi_clean_host(const frbch_fil_desc* fil, void* rows, uint64_t nrows, const frbch_rfi_params* par,
                         const uint8_t* zap, int device, uint8_t* mask, double* repl, uint8_t* chan_flag, uint8_t* blk_flag,
                         uint32_t* kernel_used, char* err, size_t err_cap);

/* All nifs products cleaned in one residency (`fil->product` is ignored): the statistics of every product, each product's own
 * mask (frbch_rfi_mask without a prior), the OR of the masks and of the channel and block flags across the products, then --
 * for nifs > 1 -- frbch_rfi_mask again per product with `prior` = the union, which gives repl[p], and the union mask applied
 * to every product with its own repl[p].  nifs = 1 is frbch_rfi_clean_*.  mask [nblk][nchan], repl [nifs][nchan], chan_flag
 * [nchan], blk_flag [nblk] and stats [nifs][nblk][nchan][2] (may be NULL) are HOST arrays; *kernel_used (may be NULL): the
 * smallest over the products.  The _device form cleans d_rows in place; the _host form uploads the rows once, cleans them
 * and downloads them once into `rows`. */
int frbch_rfi_cleanp_device(const frbch_fil_desc* fil, void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                            const uint8_t* zap, int device, uint8_t* mask, double* repl, uint8_t* chan_flag, uint8_t* blk_flag,
                            void* stats, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_rfi_cleanp_host(const frbch_fil_desc* fil, void* rows, uint64_t nrows, const frbch_rfi_params* par,
                          const uint8_t* zap, int device, uint8_t* mask, double* repl, uint8_t* chan_flag, uint8_t* blk_flag,
                          void* stats, uint32_t* kernel_used, char* err, size_t err_cap);

/* ---- interference: the periodicity test (the spectral peak of every block and channel) -----------
 * A weak repeating signal (radar, mains harmonics, a switching supply) can stay below the cell test of frbch_rfi_mask on
 * mean and std and still appear in every dedispersed series.  frbch_rfi_peaks_* take the power spectrum of every (block,
 * channel) cell on the device and return its largest bin; frbch_rfi_periodic decides on the host; frbch_rfi_cleanf_* are
 * frbch_rfi_clean_* with that decision handed to frbch_rfi_mask as `prior`.  tests/rfi_periodic_oracle.py restates all of it
 * in numpy and every result is reproducible to the bit.
 *
 * Blocks and the untested cells.  The blocks are those of frbch_rfi_nblk; the transform length is n = block_rows, which the
 * periodic test requires to be a power of two in 8 .. 4096 (anything else: FRBCH_E_ARG).  Block b has n_b rows.  A cell is
 * NOT TESTED and gets the peak {0, 0} when 2 n_b < n, when its mean S / n_b is not finite, or when
 * var = max(0, Q / n_b - mean * mean) is not finite or 0: S, Q, mean and var exactly as in step 1 of frbch_rfi_mask.
 * Channel pairing.  Channels are transformed in pairs (c0, c1) = (2m, 2m + 1): one complex transform of length n carries two
 * real channels.  For j < n_b: z[j] = ((float)((double)x[r0 + j][c0] - mean_c0), (float)((double)x[r0 + j][c1] - mean_c1));
 * for j >= n_b: z[j] = (0, 0).  A component is 0 throughout for a channel that is not tested and for the missing partner
 * of an odd last channel, so that a bad channel never reaches its partner.
 * The transform Z = DFT_n(z): radix 2, decimation in time, float32, every operation rounded on its own (no fused
 * multiply-add).  The input is taken in bit-reversed order; stages s = 1 .. log2 n with half = 2^(s-1); the butterfly on
 * (u, v), v = u's partner `half` further on, j = u's index mod half, uses w = W[j n / 2^s]:
 *     t = (wr vr - wi vi, wr vi + wi vr) (the two products first),  u' = u + t,  v' = u - t.
 * W[k] = ((float)cos(a), (float)(-sin(a))) with a = 2.0 pi k / n evaluated in double ON THE HOST: the kernels take the table
 * from the host and compute no sines.  The operation graph is fixed, the schedule is free: a radix-4, -8 or -16 register
 * pass is these radix-2 butterflies with these table entries; twiddles merged into products and the three-multiplier forms
 * give other bits and are not used.
 * The per-channel peak.  For k = 1 .. n/2 - 1, A = Z[k], B = Z[n - k], all float32:
 *     N_c0[k] = (Ar + Br)^2 + (Ai - Bi)^2,    N_c1[k] = (Ai + Bi)^2 + (Br - Ar)^2
 * (four times the power of the channel's own transform).  The peak {num, k} of a cell starts at {0, 0} and walks k ascending,
 * replacing when N[k] > num: the largest value and the lowest k that attains it; a NaN never replaces.
 * peaks: frbch_rfi_peak [nblk][nchan].
 * The decision, frbch_rfi_periodic: host only, double, every operation rounded on its own.  A tested cell has
 * p = (double)num / ((4.0 n_b) var), a cell that is not tested p = 0 (for noise p is exponentially distributed with mean 1).
 * A cell is flagged when p > t_pow; a channel is flagged wholly (pchan) when its flagged cells number more than
 * chan_frac nblk; pflag[b][c] = cell flag | pchan[c].  `power` ([nblk][nchan] doubles, may be NULL) receives p.
 * FRBCH_E_ARG: what frbch_rfi_mask refuses, a block_rows that is not a power of two in 8 .. 4096, a wrong `size` of
 * frbch_rfi_fparams, a t_pow that is not positive or is infinite, a chan_frac outside 0 .. 1. */
typedef struct frbch_rfi_peak { float num; uint32_t k; } frbch_rfi_peak;
typedef struct frbch_rfi_fparams {
  uint32_t size, reserved;             /* = sizeof(frbch_rfi_fparams)                                                     */
  double t_pow, chan_frac;             /* threshold on p; fraction of a channel's blocks, 0..1                            */
} frbch_rfi_fparams;
/* Which kernel frbch_rfi_peaks_device takes (host only, nothing runs): 1 = the fast kernel (8- / 16-bit rows of whole 64-byte
 * channel tiles, d_rows and the row pitch 16-byte aligned, n = 256 .. 2048: the columns of a piece of the row staged in the
 * LDS, register passes of radix 8 and 16), 0 = the generic one (a workgroup per block and channel pair; the only one for
 * float rows), < 0 = refused; only the ADDRESS of d_rows is examined.  Both kernels give the same bits. */
int frbch_rfi_peaks_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_rfi_params* par);
/* d_stats: what frbch_rfi_stats_device wrote for the same arguments; d_peaks: [nblk][nchan] frbch_rfi_peak. */
int frbch_rfi_peaks_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                           int device, const void* d_stats, void* d_peaks, uint32_t* kernel_used, char* err, size_t err_cap);
/* One upload of the rows, then the statistics and the peaks; `stats` may be NULL; kernel_used[2] (may be NULL): the
 * statistics kernel, the peaks kernel. */
int frbch_rfi_peaks_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_rfi_params* par, int device,
                         void* stats, void* peaks, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_rfi_periodic(const frbch_fil_desc* fil, const void* stats, const void* peaks, uint32_t nblk, uint64_t nrows,
                       const frbch_rfi_params* par, const frbch_rfi_fparams* fpar, uint8_t* pflag, uint8_t* pchan,
                       double* power, char* err, size_t err_cap);
/* frbch_rfi_clean_* with the periodicity test: statistics, peaks, frbch_rfi_periodic, frbch_rfi_mask with `prior` = pflag,
 * apply.  pflag [nblk][nchan] and pchan [nchan] are HOST arrays, `peaks` a host array that may be NULL; the returned
 * chan_flag is that of the mask ORed with pchan (what a flag file lists).  kernel_used[2] (may be NULL) as in
 * frbch_rfi_peaks_host.  The _host form uploads the rows once and downloads them once. */
int frbch_rfi_cleanf_device(const frbch_fil_desc* fil, void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                            const frbch_rfi_fparams* fpar, const uint8_t* zap, int device, uint8_t* mask, double* repl,
                            uint8_t* chan_flag, uint8_t* blk_flag, uint8_t* pflag, uint8_t* pchan, void* peaks,
                            uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_rfi_cleanf_host(const frbch_fil_desc* fil, void* rows, uint64_t nrows, const frbch_rfi_params* par,
                          const frbch_rfi_fparams* fpar, const uint8_t* zap, int device, uint8_t* mask, double* repl,
                          uint8_t* chan_flag, uint8_t* blk_flag, uint8_t* pflag, uint8_t* pchan, void* peaks,
                          uint32_t* kernel_used, char* err, size_t err_cap);

/* ---- resident rows: flagging, DM-range search, grouping, selection and cut-outs in one call --------
 * The production call for a DM-range search with candidates: the rows cross to the device ONCE (frbch_candidates_host) or
 * not at all (frbch_candidates_device) and every stage above runs on them where they lie.  Every array of the result is
 * byte-identical to what this sequence of the calls above returns for the same arguments:
 *  1. With FRBCH_CAND_RFI: frbch_rfi_clean_host for fil->product (`rfi`, `zap`); otherwise the rows as given.
 *  2. frbch_dedisperse_search_host on those rows (`zerodm`, `clip_sigma`, `sp`): nout, nclipped, the records and -- with
 *     FRBCH_CAND_SERIES -- series[ndm][nout].
 *  3. frbch_sp_group_cands with `dm_gap`: ngroup_all groups.
 *  4. The selection (frbch_cand_select): the groups with nmember >= min_members (min_members >= 1); when max_cands > 0 and
 *     more remain, the max_cands of them with the largest best.sigma, among equal sigmas the group that comes earlier in
 *     group order; the kept groups stay in group order.
 *  5. The cut-out candidate of kept group g, every operation an IEEE double operation rounded on its own:
 *     dm = dms[best.dm_index], sample = best.sample, tfactor = min(max(best.width / 2, 1), 512) (integer division);
 *     dm_span <= 0: dm_lo = 0, dm_hi = 2 dm;  dm_span > 0: dm_lo = max(0, dm - 0.5 dm_span), dm_hi = dm_lo + dm_span.
 *  6. frbch_cutout_host in batches of whole candidates, in order, each of
 *     max(1, min(65535, (2^31 - 1) / (max(nf, ndm) nt), 2^26 / (ndm nchan))) candidates (integer divisions; the three
 *     per-call limits of frbch_cutout_*), the last one shorter.  No kept group, or cut.nt = 0 (the search-only use: `cut` is
 *     then not looked at): no planes, the four plane pointers are NULL, cutout_calls = 0 and the call returns FRBCH_OK.
 * The library owns the result (frbch_cand_result_free; NULL is a no-op), so no capacity is negotiated and nothing runs
 * twice; the one capacity error left is the search's own (more than 2^20 raw peaks: FRBCH_E_CAPACITY).
 * frbch_candidates_device never writes d_rows: with FRBCH_CAND_RFI the statistics are read from d_rows, and when the mask
 * has a cell set the rows are copied device to device and the copy is cleaned (frbch_rfi_apply_device) and used from then
 * on.  So kernel_used[0] is frbch_rfi_stats_kernel for the address of d_rows, and kernel_used[1] / [3] are
 * frbch_dedisperse_kernel / frbch_cutout_kernel for the address of the rows the stage read -- d_rows, or a buffer of the
 * library's (hipMalloc: 256-byte aligned), which is what the _host form always reads.  kernel_used of a stage that did not
 * run is 0; of the cut-out the smallest over the batches.
 * Errors: FRBCH_E_ARG with a message and *out = NULL for a wrong `size` in any struct, an unknown flag, NULL arguments,
 * min_members = 0, and whatever a stage refuses (a dm_gap outside 1..16, a `cut` frbch_cutout_* refuses, ...);
 * FRBCH_E_NOMEM when device memory runs out, the message lists every buffer of the call with its size.  Everything
 * allocated is freed on every path; the call is host-synchronous. */
#define FRBCH_CAND_RFI 1u
#define FRBCH_CAND_SERIES 2u
typedef struct frbch_cand_params {
  uint32_t size, flags;                /* = sizeof(frbch_cand_params); FRBCH_CAND_*                                       */
  frbch_rfi_params rfi;                /* used with FRBCH_CAND_RFI                                                        */
  const uint8_t* zap;                  /* host [nchan] or NULL, as frbch_rfi_clean_*                                      */
  uint32_t zerodm, reserved;           /* as frbch_dedisperse_*                                                           */
  double clip_sigma;
  frbch_sp_params sp;
  uint32_t dm_gap, min_members, max_cands, reserved2;   /* max_cands = 0: all                                             */
  frbch_cutout_params cut;             /* cut.nt = 0: no planes                                                           */
  double dm_span;                      /* <= 0: dm_lo = 0, dm_hi = 2 dm                                                   */
} frbch_cand_params;
typedef struct frbch_cand_result frbch_cand_result;     /* opaque; owns the host arrays of the view                        */
enum { FRBCH_CAND_T_UPLOAD = 0, FRBCH_CAND_T_FLAG, FRBCH_CAND_T_DEDISPERSE, FRBCH_CAND_T_SEARCH, FRBCH_CAND_T_CUT,
       FRBCH_CAND_T_DOWNLOAD, FRBCH_CAND_NSTAGE };
typedef struct frbch_cand_view {
  uint32_t size, reserved;             /* = sizeof(frbch_cand_view), set by the caller                                    */
  uint64_t nout, nclipped;
  uint64_t ncand;                      /* all search records                                                              */
  const frbch_sp_cand* cands;          /* [ncand]; NULL when ncand = 0                                                    */
  uint64_t ngroup_all, ngroup;         /* groups of step 3, kept groups of step 4                                         */
  const frbch_sp_group* groups;        /* [ngroup]; NULL when ngroup = 0                                                  */
  const frbch_cutout_cand* cut_cands;  /* [ngroup]; NULL when ngroup = 0                                                  */
  const float* ft;                     /* [ngroup][nf][nt]; the four planes are NULL when there are none                  */
  const uint32_t* ft_hits;
  const float* dt;                     /* [ngroup][ndm][nt]                                                               */
  const uint32_t* dt_hits;
  uint32_t nblk, reserved2;            /* with FRBCH_CAND_RFI (otherwise 0 and NULL):                                     */
  const uint8_t* mask;                 /* [nblk][nchan]                                                                   */
  const double* repl;                  /* [nchan]                                                                         */
  const uint8_t* chan_flag;            /* [nchan]                                                                         */
  const uint8_t* blk_flag;             /* [nblk]                                                                          */
  const float* series;                 /* [ndm][nout] with FRBCH_CAND_SERIES, otherwise NULL                              */
  uint32_t kernel_used[4];             /* RFI statistics, dedispersion, search, cut-out                                   */
  uint32_t cutout_calls, row_uploads;  /* batches of step 6; 1 for _host, 0 for _device                                   */
  /* milliseconds per stage, indexed by FRBCH_CAND_T_*: upload of the rows, flagging (with the mask decision on the host),
   * dedispersion, search (with the host's merge of the raw peaks), cut-outs, downloads (series and planes) */
  double wall_ms[FRBCH_CAND_NSTAGE];   /* on the host's clock                                                             */
  double device_ms[FRBCH_CAND_NSTAGE]; /* between two events on the stage's stream, summed over its device calls          */
} frbch_cand_view;
int frbch_candidates_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms, uint32_t ndm,
                          const frbch_cand_params* par, int device, frbch_cand_result** out, char* err, size_t err_cap);
int frbch_candidates_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms, uint32_t ndm,
                            const frbch_cand_params* par, int device, frbch_cand_result** out, char* err, size_t err_cap);
/* counts and host pointers, valid until frbch_cand_result_free */
int frbch_cand_result_view(const frbch_cand_result* res, frbch_cand_view* view);
void frbch_cand_result_free(frbch_cand_result* res);
/* Step 4 alone (host only): keep[cap] receives the indices of the kept groups in ascending order, *nkeep their number
 * (never more than ngroup: cap = ngroup always suffices; fewer: FRBCH_E_CAPACITY). */
int frbch_cand_select(const frbch_sp_group* groups, uint64_t ngroup, uint32_t min_members, uint32_t max_cands,
                      uint64_t* keep, uint64_t cap, uint64_t* nkeep);

/* ---- band-limited single-pulse search ---------------------------------------------------------------
 * Every search above sums the whole band first; a burst that fills 1/k of the band loses sqrt(k) of its S/N there.  Bursts
 * of repeaters are often band-limited, so frbch_dedisperse_bands_* make, next to the full-band series, the series of every
 * contiguous RANGE of sub-bands, and frbch_bandsearch_* search them all with frbch_spsearch_device (every series is
 * normalised on its own: a range gets its own noise scale).  The conventions are this library's; tests/bands_oracle.py
 * restates them in numpy.  Every sum stays exact (this is not an approximate sub-band dedispersion).
 *
 * Bands.  nsub (1..16) divides nchan; cps = nchan / nsub; sub-band s holds channels s cps .. (s + 1) cps - 1.  A band is a
 * range [a, b) of sub-bands with min_sub <= b - a <= max_sub (min_sub = 0 means 1, max_sub = 0 means nsub), numbered by
 * ascending a, then ascending b: the full band [0, nsub), where it is listed, is the last band that starts at 0.
 *
 * Series.  For band j = [a, b), with n_c, value (the clip's replacement), S (the zero-DM row sums over the FULL band),
 * nout and the clip exactly those of frbch_dedisperse_*:
 *     y[dm][j][t] = (float)( sum_{c in [a cps, b cps)} value(t + n_c(dm), c)
 *                            - (zerodm ? (sum over the same c of S[t + n_c(dm)]) / nchan : 0) )
 * both sums in double over ascending c.  The delays stay referenced to the top of the FULL band, so that ranges add up,
 * and band [0, nsub) is frbch_dedisperse_*'s series to the bit for every row type.  On 8- / 16-bit rows every sum is an
 * exact integer in any order.  The plane is out[dm * nband + j][t], float32: the layout frbch_spsearch_device reads, with
 * ndm * nband series.
 *
 * FRBCH_E_ARG, each with its own message: a wrong `size`; nsub outside 1..16 or no divisor of nchan; min_sub > max_sub;
 * max_sub > nsub; ndm * nband above 65535 (the search's limit on series); everything frbch_dedisperse_* refuses. */
typedef struct frbch_band_params {
  uint32_t size, nsub;                 /* = sizeof(frbch_band_params); 1..16, a divisor of nchan                         */
  uint32_t min_sub, max_sub;           /* widths b - a that are listed; 0 = 1 and 0 = nsub                                */
} frbch_band_params;
/* Host only.  *nband receives the number of bands; sub_lo[cap] / sub_hi[cap] (either may be NULL with cap = 0, which counts)
 * receive a and b of the first `cap` bands.  More bands than `cap`: FRBCH_E_CAPACITY with *nband set. */
int frbch_band_list(uint32_t nchan, const frbch_band_params* bands, uint16_t* sub_lo, uint16_t* sub_hi, uint32_t cap,
                    uint32_t* nband, char* err, size_t err_cap);
/* Which kernels frbch_dedisperse_bands_device takes for these arguments (host only, nothing runs): 1 = the tiled prefix
 * kernel and the range kernel behind it (8- / 16-bit rows, nchan <= 65536, a sub-band a whole number of 64-byte channel
 * tiles, and what frbch_dedisperse_kernel asks of the tiled dedispersion: 16-byte aligned d_rows and row pitch, every
 * (DM group, channel tile) within the rows the LDS holds), 0 = the generic kernel (a thread per (dm, t) that walks the
 * channels once per first sub-band), < 0 = refused.  Only the ADDRESS of d_rows is examined.  Both give the same bytes. */
int frbch_dedisperse_bands_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms, uint32_t ndm,
                                  const frbch_band_params* bands);
/* d_out / out is [ndm * nband][nout] with nout = frbch_dedisperse_nout(); *kernel_used (may be NULL) as above.  The tiled
 * form allocates its scratch itself: the prefix plane [ndm][nsub][nout] of uint32, and with zerodm one of double. */
int frbch_dedisperse_bands_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms, uint32_t ndm,
                                  uint32_t zerodm, double clip_sigma, const frbch_band_params* bands, int device, float* d_out,
                                  uint64_t nout, uint64_t* nclipped, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_dedisperse_bands_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms, uint32_t ndm,
                                uint32_t zerodm, double clip_sigma, const frbch_band_params* bands, int device, float* out,
                                uint64_t nout, uint64_t* nclipped, uint32_t* kernel_used, char* err, size_t err_cap);

typedef struct frbch_spb_cand {
  uint32_t dm_index, width;            /* index into dms, boxcar width in samples                                        */
  uint64_t sample;                     /* centre c = t + w / 2                                                           */
  float sigma;
  uint16_t sub_lo, sub_hi;             /* the band [sub_lo, sub_hi) whose series holds the record                        */
} frbch_spb_cand;
/* The production call.  The rows cross to the device once (_host) or lie in HBM already and are never written (_device);
 * the clip / zero-DM pre-pass runs once; then batches of consecutive DMs: frbch_dedisperse_bands_device's kernels and
 * frbch_spsearch_device on a plane that stays on the device.  A batch holds the largest number of DMs whose plane
 * (nband * nout floats per DM) fits plane_bytes (0 means 1 GiB; fewer bytes than one DM's plane: FRBCH_E_ARG); the scratch
 * of the tiled form comes on top.  The records -- those of frbch_spsearch_device on every series, sorted by (dm_index,
 * sub_lo, sub_hi, sample, width) -- do not depend on the batch size.  The search's cap of 2^20 raw peaks holds per batch
 * and is reported as FRBCH_E_CAPACITY ("threshold too low"), never as a cut list; more records than `cap`:
 * FRBCH_E_CAPACITY with *ncand set (cap = 0 with cands = NULL counts).  kernel_used (may be NULL) receives [0] the
 * dedispersion form (1 only if every batch took the tiled form) and [1] the search kernel; *nbatch (may be NULL) the number
 * of batches; stage_ms (may be NULL) the host's clock around [0] the pre-pass, [1] the dedispersion of all batches and
 * [2] their searches, each with the download of its raw peaks. */
int frbch_bandsearch_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms, uint32_t ndm,
                            uint32_t zerodm, double clip_sigma, const frbch_band_params* bands, const frbch_sp_params* params,
                            uint64_t plane_bytes, int device, uint64_t nout, uint64_t* nclipped, frbch_spb_cand* cands,
                            uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, uint32_t* nbatch, double* stage_ms, char* err,
                            size_t err_cap);
int frbch_bandsearch_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms, uint32_t ndm,
                          uint32_t zerodm, double clip_sigma, const frbch_band_params* bands, const frbch_sp_params* params,
                          uint64_t plane_bytes, int device, uint64_t nout, uint64_t* nclipped, frbch_spb_cand* cands,
                          uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, uint32_t* nbatch, double* stage_ms, char* err,
                          size_t err_cap);
/* Grouping (host only): the link rule of frbch_sp_group_cands on (dm_index, sample, width).  The band plays NO part in
 * linking -- a pulse shows in every range that overlaps it, and two pulses at one time in disjoint bands join as well.
 * `best` is the member with the largest sigma; ties: the narrower range (sub_hi - sub_lo), then frbch_sp_group_cands'
 * order (narrower width, lower dm_index, earlier sample), then the lower sub_lo.  full_sigma is the largest sigma among
 * the members whose band is [0, nsub), 0 if there is none.  Groups come sorted by best's (dm_index, sample, width, sub_lo,
 * sub_hi).  FRBCH_E_ARG: what frbch_sp_group_cands refuses, nsub outside 1..16, a record with sub_lo >= sub_hi or
 * sub_hi > nsub. */
typedef struct frbch_spb_group {
  frbch_spb_cand best;
  uint32_t nmember, dm_index_lo, dm_index_hi;
  uint16_t sub_lo_min, sub_hi_max;     /* over the members' bands                                                         */
  uint64_t sample_lo, sample_hi;       /* over the members' centres                                                       */
  float full_sigma;
  uint32_t reserved;
} frbch_spb_group;
int frbch_spb_group_cands(const frbch_fil_desc* fil, const double* dms, uint32_t ndm, uint32_t nsub, const frbch_spb_cand* cands,
                          uint64_t ncand, uint32_t dm_gap, frbch_spb_group* groups, uint64_t cap, uint64_t* ngroup, char* err,
                          size_t err_cap);

/* ---- in front of the filterbank: the corner turn -------------------------------
 * jive5ab's spif2file splits the recorder's stream -- every W-bit word holds one time sample of ALL channels -- into one
 * 2-channel stream per IF, driven by the recipe strings of spif2file.sh:31-113, e.g. the 16-channel 2-bit mode
 * `32>[24,25,16,17][8,9,0,1]...[14,15,6,7]:0-7`: output stream ("tag") g takes the listed bits of every word, in that
 * order, LSB first; `swap_sign_mag+` (Mark5B modes, :79-94) first exchanges the two bits of every 2-bit sample.  Doing
 * it on the GPU lets frbch_process_device read the result straight from HBM (header_bytes = 0) without per-IF files.
 * jive5ab is not in the reference tree: the bit order is this library's restatement (oracle/post_oracle.py). */
int frbch_cornerturn_info(const char* recipe, uint32_t* word_bits, uint32_t* ntags, uint32_t* bits_per_word,
                          uint32_t* first_tag, char* err, size_t err_cap);
/* frames: nframes recorder frames; out[g]: payload bytes of tag first_tag + g, out_bytes_each = words * bits_per_word / 8 */
int frbch_cornerturn_host(const char* recipe, const void* frames, size_t nframes, uint32_t frame_bytes,
                          uint32_t header_bytes, void* const* out, uint32_t ntags, size_t out_bytes_each, int device,
                          char* err, size_t err_cap);
int frbch_cornerturn_device(const char* recipe, const void* d_frames, size_t nframes, uint32_t frame_bytes,
                            uint32_t header_bytes, void* const* d_out, uint32_t ntags, size_t out_bytes_each, int device,
                            char* err, size_t err_cap);

/* ---- refinement of a fold: period, period derivative and DM search ---------------------------------
 * A fold follows the ephemeris it is handed; a topocentric polynomial from a catalogue is off by the Earth's Doppler factor,
 * a candidate of the periodicity search by up to half a Fourier bin.  frbch_foldfit_* shift the sub-integrations and the
 * channels of the folded cube against each other over a grid of DM, spin frequency and frequency derivative and score every
 * trial profile (what pdmp / prepfold do behind a fold).  Neither program is in the reference tree: the conventions are this
 * library's (tests/foldfit_oracle.py restates them in numpy), chosen so that every result is reproducible to the bit: the
 * host works in double with every operation rounded on its own (no fused multiply-add), the device adds integers, exact in
 * any order, and scores in double in one fixed order.
 *
 * Input.  The cube d_cube[nsub][nifs][nbin][nchan] (double) and d_hits[nsub][nbin][nchan] (uint32) exactly as
 * frbch_foldp_device leaves them for 8- or 16-bit rows folded WITHOUT per-channel delays (apply_delays = 0): every value an
 * exact integer, 0 <= cube <= (2^nbits - 1) hits, and a (sub-integration, bin, channel) holds at most L rows.  `fil`, `nrows`
 * and par->nsub / nbin / subint_s are the fold's; f0_fold is the frequency the cube was folded at (the polynomial's F0, or
 * the polyco's reference frequency).  par->products is a mask over the nifs products: those that are added (1 << fil->product
 * for one product, 3 for PP + QQ of a coherency file).  flag[nchan] (host, may be NULL): a non-zero byte leaves a channel out.
 *
 * Trials.  Three axes, each count odd or 1, centred on the nominal value (kc = ndm / 2, ic = nfreq / 2, jc = nfdot / 2):
 *   dm_k  = dm0 + (double)(k - kc) * ddm,    df_i = (double)(i - ic) * dfreq,    dfd_j = (double)(j - jc) * dfdot.
 * Sub-integration times.  L = max(1, round(subint_s / tsamp)) as frbch_fold_nsub has it, r_s = min(L, nrows - s L),
 *   tau_s = ((double)(s L) + 0.5 * (double)r_s - 0.5 * (double)nrows) * tsamp
 * -- the middle of sub-integration s about the middle of the observation, which keeps the two spin axes decoupled.
 * Shift tables (host, int64 reduced to 0 .. nbin - 1; rint rounds ties to even):
 *   shD[k][c]    = rint((delay_c(dm_k) * f0_fold) * (double)nbin),  delay_c the delay of frbch_dedisperse_* in seconds
 *                  (post.dedisperse_profile rotates by the same number);
 *   shP[j][i][s] = rint((df_i * tau_s + ((0.5 * dfd_j) * tau_s) * tau_s) * (double)nbin).
 * The two shifts are rounded separately and added: the separability is the convention.  Its cost: a trial's total shift is
 * off by at most one bin where a single rounding would be off by at most half a bin.
 * Stage 1, DM: for every k, s and bin b, over the unflagged channels c and the masked products p,
 *   A[k][s][b]  = sum (int64)cube[s][p][(b + shD[k][c]) mod nbin][c]          (int64)
 *   HA[k][s][b] = sum over the unflagged channels of hits[s][(b + shD[k][c]) mod nbin][c]   (uint64; once a channel: the
 *                 products share their hits).
 * Stage 2, spin: for every trial (k, j, i) and bin b,
 *   B[b] = sum over s of A[k][s][(b - shP[j][i][s]) mod nbin],     H[b] likewise from HA.
 * The signs: a channel's delay puts its pulse at a LATER phase, which stage 1 reads from (b + shD); a trial frequency above the
 * fold's moves what the fold put into bin b' on to bin b' + shP, so bin b of the trial reads from (b - shP): with these the
 * best trial is the correction to ADD, DM' = dm_k, F0' = f0_fold + df_i, F1' = F1 + dfd_j.
 * Score of a trial (double, every operation rounded on its own): M_k = (double)(sum of all B) / (double)(sum of all H) --
 * both totals are those of A[k] and HA[k], the same for every spin trial --; a bin with H[b] > 0 gives
 * d = (double)B[b] / (double)H[b] - M_k and the term (double)H[b] * (d * d); the terms are added as 64 partial sums --
 * partial q adds the bins q, q + 64, ... in ascending order -- which are then added in ascending q (the summation rule of
 * the single-pulse search's block statistics).  Fewer than two bins with hits: score 0.  This is the numerator of
 * prepfold's chi-squared with the hits as weights.
 *
 * Consequence: with one trial on every axis B / H is the dedispersed, scrunched profile that post.py makes of the same cube
 * in numpy (post._scrunched), to the bit.
 *
 * Peaks (frbch_foldfit_peaks, host only).  The first largest score in the order [ndm][nfdot][nfreq] is the peak trial.  Along
 * each axis through it the least-squares parabola of frbch_dmscan_peaks (its normal equations, its code) is fitted over the
 * contiguous points at or above fit_frac times the peak; the refined value is the vertex; an axis whose points reach the
 * edge of the grid, with fewer than three points or without a maximum keeps its grid value with fitted = 0.  *_res is the
 * half-width at which that parabola lies below its vertex by the median score of the grid's border trials (a trial with index
 * 0 or n - 1 on an axis with n > 1; sorted ascending, the middle one, or 0.5 * (the two middle ones added)):
 * (sqrt(-1.0 / a) * step) * sqrt(median), 0 on an unfitted axis.  It is a resolution -- how far the grid tells two values
 * apart -- not an error bar.
 * S/N of a profile x[b] = B[b] / H[b] (0 without hits): the off-pulse region is the nbin / 2 circularly contiguous bins with
 * the smallest sum (added from its first bin on; the first such start), baseline = its mean, rms = sqrt(sum (x - baseline)^2
 * / (nbin / 2)); S/N is the first largest of ((boxcar sum / w) - baseline) * sqrt(w) / rms over the listed widths w (in list
 * order) and the start bins ascending, the boxcar taken circularly; rms = 0: S/N 0.  Computed for the nominal (central) trial
 * and for the peak trial.
 *
 * frbch_foldfit_steps gives the natural steps for a span T = nrows tsamp: dfreq = 1 / (nbin T), a drift of one bin over the
 * span; dfdot = 8 / (nbin T^2), one bin at the ends; ddm = 1 / (nbin f0 (1 / 2.41e-4) (f_lo^-2 - f_hi^-2)), one bin at the
 * bottom of the band.
 *
 * FRBCH_E_ARG, each with its own message and every output untouched: a wrong `size`; an even count above 1; ndm nfdot nfreq
 * above 2^22; nbin outside 2..4096; nsub outside 1..4096 or not frbch_fold_nsub(); nchan above 16384; float rows; an empty
 * `products` or one beyond nifs; a step that is not finite, or not positive where its count exceeds 1; a dm_k outside
 * [0, 1e5); fit_frac outside (0, 1]; nwidth outside 1..8 or a width outside 1..nbin / 2; a shift beyond 2^52 bins; and
 * (2^nbits - 1) nrows nchan popcount(products) >= 2^53, the bound that keeps every sum an exact double.
 *
 * Not built: no orbital or jerk axis, no barycentring (the offsets are topocentric), no channel weights beyond the flag, no
 * sub-bin interpolation -- integer bin shifts cannot undo the smear inside a sub-integration: fold again with the refined
 * values for that --, and resolutions, not error bars. */
typedef struct frbch_foldfit_params {
  uint32_t size;               /* = sizeof(frbch_foldfit_params)                                                 */
  uint32_t nbin, nsub;         /* of the cube                                                                    */
  uint32_t products;           /* mask of the products that are added                                            */
  uint32_t ndm, nfreq, nfdot;  /* trial counts, each odd or 1                                                    */
  uint32_t nwidth;             /* 1..8 boxcar widths of the S/N                                                  */
  double f0_fold, subint_s;    /* of the fold                                                                    */
  double dm0, ddm;             /* nominal DM and its step                                                        */
  double dfreq, dfdot;         /* steps of the spin axes, Hz and Hz / s                                          */
  double fit_frac;             /* (0, 1]                                                                         */
  uint32_t widths[8];
} frbch_foldfit_params;

typedef struct frbch_foldfit_result {
  double dm, dm_res;           /* refined DM                                                                     */
  double dfreq, dfreq_res;     /* refined offset from f0_fold, Hz                                                */
  double dfdot, dfdot_res;     /* refined offset of the frequency derivative, Hz / s                             */
  double score_peak, score_nominal, border_median;
  double snr_nominal, snr_best;
  uint32_t kpeak, jpeak, ipeak;                      /* the peak trial: DM, derivative, frequency index          */
  uint32_t fitted_dm, fitted_freq, fitted_fdot;
  uint32_t nfit_dm, nfit_freq, nfit_fdot;            /* points at or above fit_frac times the peak               */
  uint32_t width_nominal, bin_nominal, width_best, bin_best, reserved;
} frbch_foldfit_result;

int frbch_foldfit_steps(const frbch_fil_desc* fil, uint64_t nrows, uint32_t nbin, double f0_fold, double* ddm, double* dfreq,
                        double* dfdot);
/* Which form each stage of frbch_foldfit_device takes (host only, nothing runs): kernel[0] stage 1, kernel[1] stage 2, 1 = the
 * fast kernel, 0 = the generic one; only the ADDRESSES of d_cube and d_hits are examined.  The fast forms want both 16-byte
 * aligned and the sums of a sub-integration in 32 bits ((2^nbits - 1) popcount(products) L < 2^32, L nchan < 2^32); stage 1
 * also whole tiles of 8 channels and nbin <= 1024 (a tile of all bins in the LDS), stage 2 at least two spin trials a DM. */
int frbch_foldfit_kernel(const frbch_fil_desc* fil, uint64_t nrows, const frbch_foldfit_params* par, const double* d_cube,
                         const uint32_t* d_hits, uint32_t* kernel);
/* score[ndm][nfdot][nfreq]; prof_acc / prof_hits [2][nbin]: B and H of the nominal and of the peak trial; result; and, each
 * where not NULL: trial_acc / trial_hits [ndm][nfdot][nfreq][nbin], the profiles of every trial (at most 2^24 elements, else
 * FRBCH_E_ARG); plane_acc / plane_hits [nsub][nbin], A and HA of the central DM (the phase-time plane).  All host arrays; the
 * cube and its hits are device memory, never written.  Host-synchronous on a stream of its own, as the other _device entry
 * points behind the filterbank.  kernel_used[2] as frbch_foldfit_kernel.  Both forms give the same bytes. */
int frbch_foldfit_device(const frbch_fil_desc* fil, uint64_t nrows, const frbch_foldfit_params* par, const double* d_cube,
                         const uint32_t* d_hits, const uint8_t* flag, int device, double* score, int64_t* prof_acc,
                         uint64_t* prof_hits, frbch_foldfit_result* result, int64_t* trial_acc, uint64_t* trial_hits,
                         int64_t* plane_acc, uint64_t* plane_hits, uint32_t* kernel_used, char* err, size_t err_cap);
/* the same with the cube and its hits in host memory: one upload, one download of the results */
int frbch_foldfit_host(const frbch_fil_desc* fil, uint64_t nrows, const frbch_foldfit_params* par, const double* cube,
                       const uint32_t* hits, const uint8_t* flag, int device, double* score, int64_t* prof_acc,
                       uint64_t* prof_hits, frbch_foldfit_result* result, int64_t* trial_acc, uint64_t* trial_hits,
                       int64_t* plane_acc, uint64_t* plane_hits, uint32_t* kernel_used, char* err, size_t err_cap);
/* The peaks alone, from a score grid and the two profiles (host only). */
int frbch_foldfit_peaks(const frbch_foldfit_params* par, const double* score, const int64_t* prof_acc, const uint64_t* prof_hits,
                        frbch_foldfit_result* result, char* err, size_t err_cap);
/* Rows -> frbch_foldp_device -> frbch_foldfit_device in one residency: the cube stays in HBM and is downloaded only where
 * cube / cube_hits are not NULL ([nsub][nifs][nbin][nchan] and [nsub][nbin][nchan]).  The model must fold without per-channel
 * delays (apply_delays = 0: FRBCH_E_ARG otherwise) with par's nbin and subint_s.  The results are the bytes of the two calls in
 * sequence.  kernel_used[3]: the fold, stage 1, stage 2. */
int frbch_fold_refine_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_fold_model* model,
                             const frbch_foldfit_params* par, const uint8_t* flag, int device, double* cube, uint32_t* cube_hits,
                             double* score, int64_t* prof_acc, uint64_t* prof_hits, frbch_foldfit_result* result,
                             int64_t* plane_acc, uint64_t* plane_hits, uint32_t* kernel_used, char* err, size_t err_cap);
int frbch_fold_refine_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_fold_model* model,
                           const frbch_foldfit_params* par, const uint8_t* flag, int device, double* cube, uint32_t* cube_hits,
                           double* score, int64_t* prof_acc, uint64_t* prof_hits, frbch_foldfit_result* result,
                           int64_t* plane_acc, uint64_t* plane_hits, uint32_t* kernel_used, char* err, size_t err_cap);

/* ---- measurement -------------------------------------------------------------------------- */
int frbch_set_profiling(frbch_handle* h, int enable);
int frbch_timing_reset(frbch_handle* h);
int frbch_get_timing(frbch_handle* h, frbch_timing* t);
/* Launch record: while profiling is on, every kernel launch of the channeliser path is counted under the full name of the
 * instantiation, spelled as the demangled symbol ("frbch_k2_wave<3, 8, 4, 2, true>", "frbch_k2_chan"): what ran, where a timing
 * slot names what was planned.  Writes one line per kernel, "name\tlaunches\tlargest grid.x\tlargest grid.y\n", NUL-terminated,
 * and returns the text's length; FRBCH_E_CAPACITY when `cap` is too small.  frbch_timing_reset clears the record, and so does a
 * stream that makes the handle plan anew. */
long frbch_get_launch_record(frbch_handle* h, char* buf, size_t cap);

/* library self-description: "frbch <abi> gfx950 ..." */
const char* frbch_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FRBCH_H */
