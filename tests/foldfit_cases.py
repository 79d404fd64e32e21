"""Named cases of the fold refinement (frbch_foldfit_*) with cached expectations from tests/foldfit_oracle.py, the plan rule
restated, the calls through the C ABI and the known answer.  The cubes are the smallest that can still break a tile rule: a cube
is random, but one that frbch_foldp_* could have left (0 <= cube <= (2^nbits - 1) hits, hits <= L).

The plan rule (csrc/frbch_post.cpp, ff_plan_rule), restated in plan_expected: the fast forms want the cube and its hits 16-byte
aligned -- a call that fails this runs the generic form in both stages -- and (2^nbits - 1) popcount(products) L < 2^32,
L nchan < 2^32.  Stage 1 fast: nchan a multiple of 8, nbin <= 1024; a workgroup takes TILE_RUN = 32 tiles of 8 channels and
DM_RUN = 8 DMs.  Stage 2 fast: at least two spin trials a DM; its LDS holds chunk(nbin) = min(nsub, 65536 // (12 nbin))
sub-integrations."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import _lib, post
from tests import foldfit_oracle as fo

TILE_RUN, DM_RUN, STAGE2_BYTES = 32, 8, 65536
FIELDS = ("score", "prof_acc", "prof_hits", "results", "plane_acc", "plane_hits", "trial_acc", "trial_hits")


def chunk(nbin):
    return STAGE2_BYTES // (12 * nbin)


def hdr_of(nchan, nifs=1, nbits=8, tsamp=1.0e-3, foff=None, fch1=1500.0, product=0):
    foff = -300.0 / nchan if foff is None else foff
    return dict(nchans=nchan, nifs=nifs, nbits=nbits, fch1=fch1, foff=foff, tsamp=tsamp, tstart=60000.0, product=product)


def make(seed, nsub, nbin, nchan, *, nifs=1, nbits=8, L=64, last=None, ndm=3, nfreq=3, nfdot=3, f0=7.0, dm0=30.0, step_scale=(1.0, 1.0, 1.0),
         products=None, flag=None, dead=(), zero_bins=(), full=False, want_trials=True, hmax=3, foff=None):
    """one case: a random cube with `hmax` rows at most in a (sub-integration, bin, channel), sub-integrations of L rows (the last
    one `last`), steps = step_scale times the natural ones"""
    rng = np.random.default_rng(seed)
    hdr = hdr_of(nchan, nifs, nbits, foff=foff)
    last = L if last is None else last
    nrows = (nsub - 1) * L + last
    code = (1 << nbits) - 1
    hits = rng.integers(0, hmax + 1, (nsub, nbin, nchan)).astype(np.uint32)
    for b in zero_bins:
        hits[:, b, :] = 0
    for c in dead:
        hits[:, :, c] = 0
    if full:
        cube = np.repeat((hits.astype(np.float64) * code)[:, None], nifs, axis=1)
    else:
        cube = np.floor(rng.random((nsub, nifs, nbin, nchan)) * (hits[:, None].astype(np.float64) * code + 1.0))
    subint_s = L * hdr["tsamp"]
    nat = fo.steps(hdr, nrows, nbin, f0)
    return dict(hdr=hdr, nrows=nrows, cube=np.ascontiguousarray(cube), hits=hits, nbin=nbin, nsub=nsub, L=L, f0_fold=f0, subint_s=subint_s,
                dm0=dm0, ndm=ndm, nfreq=nfreq, nfdot=nfdot, ddm=float(nat[0] * step_scale[0]), dfreq=float(nat[1] * step_scale[1]),
                dfdot=float(nat[2] * step_scale[2]), products=(1 << hdr["product"]) if products is None else products, fit_frac=0.5,
                widths=[w for w in (1, 2, 4) if w <= nbin // 2], flag=flag, want_trials=want_trials)


def _flag(nchan, *chans):
    f = np.zeros(nchan, np.uint8)
    f[list(chans)] = 1
    return f


CASES = {
    # nsub of 1 and 2, nbin of 2: the smallest of everything
    "nsub1_nbin2": lambda: make(1, 1, 2, 8, dm0=300.0),
    "nsub2_nbin64_short_last": lambda: make(2, 2, 64, 8, last=17, nfreq=5),
    # the stage-2 chunk of the LDS at nbin = 64 (85 sub-integrations) and one more; negative spin shifts on both sides
    "nsub_chunk_nbin64": lambda: make(3, chunk(64), 64, 8, L=8, ndm=1, nfreq=3, nfdot=3, want_trials=False),
    "nsub_chunk_plus1_nbin64": lambda: make(4, chunk(64) + 1, 64, 8, L=8, ndm=1, nfreq=3, nfdot=3, want_trials=False),
    # nbin not a power of two, bins without hits, DM shifts of many turns (a fast spin), which wrap
    "nbin1000_zero_bins_many_turns": lambda: make(5, 3, 1000, 16, f0=641.0, dm0=300.0, zero_bins=(0, 1, 500, 999), want_trials=False),
    # nbin = 1024: the largest tile of stage 1, 4 bins a thread; 6 sub-integrations are one more than its stage-2 chunk of 5
    "nbin1024_chunk_plus1": lambda: make(6, chunk(1024) + 1, 1024, 8, nfdot=1, want_trials=False),
    # 72 channels are nine whole tiles of 8; 76 are no multiple of the tile: the generic stage 1 in front of the fast stage 2
    "nchan72_nine_tiles": lambda: make(7, 2, 64, 72),
    "nchan76_generic_stage1": lambda: make(17, 2, 64, 76),
    # 33 tiles of 8 channels: one more than a workgroup takes, two runs joined
    "nchan264_two_tile_runs": lambda: make(8, 2, 64, 8 * (TILE_RUN + 1), nfdot=1, want_trials=False),
    # four products of 16 bits, PP + QQ
    "coherency_mask3_u16": lambda: make(9, 2, 64, 8, nifs=4, nbits=16, products=0b0011),
    "product2_of_4": lambda: make(10, 2, 32, 8, nifs=4, products=0b0100),
    # one trial on each axis: the anchor to post._scrunched; the generic stage 2 by the plan rule
    "one_trial": lambda: make(11, 3, 64, 16, ndm=1, nfreq=1, nfdot=1),
    # one DM run more than the fast kernel's run of 8
    "ndm9": lambda: make(12, 2, 64, 8, ndm=DM_RUN + 1, nfdot=1),
    # a dead channel (no hits), a flagged one, ascending frequencies
    "dead_and_flagged_ascending": lambda: make(13, 2, 64, 16, dead=(3,), flag=_flag(16, 5, 15), foff=300.0 / 16),
    # 33 spin trials a DM: one more than the largest run of stage 2 (32 at nbin <= 256)
    "nspin33": lambda: make(14, 2, 32, 8, ndm=1, nfreq=11, nfdot=3, want_trials=False),
    # full scale at the 32-bit edge of the fast forms: 65535 * 4 * 16384 < 2^32, every sample at full scale; one row more: generic
    "full_scale_u32_edge": lambda: make(15, 2, 2, 8, nifs=4, nbits=16, products=0b1111, L=16384, hmax=8192, full=True, dm0=300.0),
    "u32_edge_one_more": lambda: make(16, 2, 2, 8, nifs=4, nbits=16, products=0b1111, L=16385, hmax=8192, full=True, dm0=300.0),
}
# what must run at the aligned address, per stage, as test_gpu_dmscan.py has it for its one stage: every case is in exactly one set
# of each pair
MUST_RUN_FAST_STAGE1 = ["nsub1_nbin2", "nsub2_nbin64_short_last", "nsub_chunk_nbin64", "nsub_chunk_plus1_nbin64", "nbin1000_zero_bins_many_turns",
                        "nbin1024_chunk_plus1", "nchan72_nine_tiles", "nchan264_two_tile_runs", "coherency_mask3_u16", "product2_of_4", "one_trial",
                        "ndm9", "dead_and_flagged_ascending", "nspin33", "full_scale_u32_edge"]
MUST_RUN_GENERIC_STAGE1 = ["nchan76_generic_stage1", "u32_edge_one_more", "full_scale_2p53"]
MUST_RUN_FAST_STAGE2 = ["nsub1_nbin2", "nsub2_nbin64_short_last", "nsub_chunk_nbin64", "nsub_chunk_plus1_nbin64", "nbin1000_zero_bins_many_turns",
                        "nbin1024_chunk_plus1", "nchan72_nine_tiles", "nchan76_generic_stage1", "nchan264_two_tile_runs", "coherency_mask3_u16",
                        "product2_of_4", "ndm9", "dead_and_flagged_ascending", "nspin33", "full_scale_u32_edge"]
MUST_RUN_GENERIC_STAGE2 = ["one_trial", "u32_edge_one_more", "full_scale_2p53"]


def must_run(name):
    """-> (stage 1, stage 2) at the aligned address, 1 = the fast kernel"""
    return (int(name in MUST_RUN_FAST_STAGE1), int(name in MUST_RUN_FAST_STAGE2))


def full_scale_2p53():
    """a cube at the bound exactly: 65535 * nrows * 8 channels * 4 products is the largest such product below 2^53, every sample
    at full scale, so the sum of all A is that number; L nchan >= 2^32 sends it to the generic forms"""
    nchan, nifs, code = 8, 4, 65535
    nrows = (2 ** 53 - 1) // (code * nchan * nifs)
    assert code * nrows * nchan * nifs < 2 ** 53 <= code * (nrows + 1) * nchan * nifs
    L = (nrows + 1) // 2
    hdr = hdr_of(nchan, nifs, 16, tsamp=1.0e-6)
    hits = np.zeros((2, 2, nchan), np.uint32)
    rows = [L, nrows - L]
    for s in range(2):
        hits[s, 0, :] = rows[s] // 2
        hits[s, 1, :] = rows[s] - rows[s] // 2
    cube = np.repeat((hits.astype(np.float64) * code)[:, None], nifs, axis=1)
    subint_s = L * hdr["tsamp"]
    assert fo.rows_per_sub(hdr, subint_s) == L
    nat = fo.steps(hdr, nrows, 2, 3.0)
    return dict(hdr=hdr, nrows=nrows, cube=np.ascontiguousarray(cube), hits=hits, nbin=2, nsub=2, L=L, f0_fold=3.0, subint_s=subint_s, dm0=500.0,
                ndm=3, nfreq=3, nfdot=1, ddm=float(nat[0]), dfreq=float(nat[1]), dfdot=float(nat[2]), products=0b1111, fit_frac=0.5,
                widths=[1], flag=None, want_trials=True)


CASES["full_scale_2p53"] = full_scale_2p53


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    for a in (c["cube"], c["hits"]):
        a.setflags(write=False)
    return c


def oracle(c):
    return fo.fold_fit(c["cube"], c["hits"], c["hdr"], c["nrows"], f0_fold=c["f0_fold"], subint_s=c["subint_s"], products=c["products"], dm0=c["dm0"],
                       ndm=c["ndm"], ddm=c["ddm"], nfreq=c["nfreq"], dfreq=c["dfreq"], nfdot=c["nfdot"], dfdot=c["dfdot"], fit_frac=c["fit_frac"],
                       widths=c["widths"], flag=c["flag"], want_trials=c["want_trials"])


@functools.lru_cache(maxsize=None)
def want(name):
    return oracle(case(name))


def plan_expected(c, aligned):
    """-> (stage 1, stage 2): 1 = the fast kernel"""
    hdr = c["hdr"]
    np_ = bin(c["products"]).count("1")
    if not aligned or ((1 << hdr["nbits"]) - 1) * np_ * c["L"] >= 2 ** 32 or c["L"] * hdr["nchans"] >= 2 ** 32:
        return (0, 0)
    return (int(hdr["nchans"] % 8 == 0 and c["nbin"] <= 1024), int(c["nfreq"] * c["nfdot"] >= 2))


def par_of(c, **over):
    a = dict(c, **over)
    return post.foldfit_params(a["hdr"], a["nrows"], a["nbin"], a["nsub"], a["f0_fold"], a["subint_s"], a["dm0"], products=a["products"],
                               ndm=a["ndm"], nfreq=a["nfreq"], nfdot=a["nfdot"], ddm=a["ddm"], dfreq=a["dfreq"], dfdot=a["dfdot"],
                               fit_frac=a["fit_frac"], widths=a["widths"])


def desc_of(c):
    return post.fil_desc(c["hdr"], c["hdr"].get("product", 0))


def outputs(c, fill=0, trials=None):
    """the output arrays of a call, every byte `fill`"""
    nt = (c["ndm"], c["nfdot"], c["nfreq"])
    out = dict(score=np.zeros(nt, np.float64), prof_acc=np.zeros((2, c["nbin"]), np.int64), prof_hits=np.zeros((2, c["nbin"]), np.uint64),
               results=np.zeros(1, post.FOLDFIT_RESULT), plane_acc=np.zeros((c["nsub"], c["nbin"]), np.int64),
               plane_hits=np.zeros((c["nsub"], c["nbin"]), np.uint64))
    if c["want_trials"] if trials is None else trials:
        out.update(trial_acc=np.zeros(nt + (c["nbin"],), np.int64), trial_hits=np.zeros(nt + (c["nbin"],), np.uint64))
    for a in out.values():
        a.view(np.uint8).reshape(-1)[:] = fill
    return out


def call(fn, c, cube_ptr, hits_ptr, out=None, par=None, desc=None, nrows=None):
    """frbch_foldfit_device / _host -> (code, message, outputs, kernel_used)"""
    out = outputs(c) if out is None else out
    k = (C.c_uint32 * 2)(7, 7)
    err = C.create_string_buffer(512)
    fl = None if c["flag"] is None else np.ascontiguousarray(c["flag"], np.uint8)
    p = lambda key: out[key].ctypes.data if key in out else None                                   # noqa: E731
    code = fn(C.byref(desc_of(c) if desc is None else desc), c["nrows"] if nrows is None else nrows, C.byref(par_of(c) if par is None else par),
              cube_ptr, hits_ptr, fl.ctypes.data if fl is not None else None, 0, p("score"), p("prof_acc"), p("prof_hits"), p("results"),
              p("trial_acc"), p("trial_hits"), p("plane_acc"), p("plane_hits"), k, err, len(err))
    return code, err.value.decode(), out, (k[0], k[1])


def query(lib, c, cube_ptr, hits_ptr):
    k = (C.c_uint32 * 2)(7, 7)
    assert lib.frbch_foldfit_kernel(C.byref(desc_of(c)), c["nrows"], C.byref(par_of(c)), cube_ptr, hits_ptr, k) == 0
    return (k[0], k[1])


def same(got, wanted):
    return all(np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(wanted[f]).tobytes() for f in FIELDS if f in wanted and f in got)


def differing(got, wanted):
    return [f for f in FIELDS if f in wanted and f in got and np.ascontiguousarray(got[f]).tobytes() != np.ascontiguousarray(wanted[f]).tobytes()]


# ---- the known answer -------------------------------------------------------------------------------------------------
# A pulsar of 10 Hz in 8-bit noise (mean 96, sigma 16), 64 channels at 1.2 - 1.5 GHz, 32768 rows of 1 ms, folded into 64 bins
# and 16 sub-integrations about PEPOCH = mid-observation with F0 too low by 0.6 / T, F1 too low by three natural steps (three
# bins of quadratic drift at the ends) and the DM too high by five natural steps.  The grid: natural steps, 17 x 9 x 81 trials
# (DM x F1 x F0), which holds the truth 5, 3 and 38.4 steps from its centre.
# The amplitude was fixed with the numpy restatement alone (known_restatement, the twelve seeds below) before the library ran:
# with a Gaussian pulse of sigma 0.015 turns it recovers 10 of 12 at 2.5 codes at the peak (seed 106 one DM step out, seed 107 one
# frequency step) and twelve of twelve at KNOWN_AMP = 4.0; KNOWN_RECORD holds what it gave there, S/N nominal -> best per seed.
KNOWN = dict(f0=10.0, f1=-2.0e-6, dm=50.0, nbin=64, nchan=64, nrows=32768, tsamp=1.0e-3, subint_s=2.048, sigma_turns=0.015,
             ndm=17, nfdot=9, nfreq=81, off_f0=0.6, off_f1_steps=3.0, off_dm_steps=5.0)
KNOWN_AMP = 4.0
KNOWN_RECORD = {101: (5.09, 52.00), 102: (9.33, 42.48), 103: (6.92, 45.31), 104: (7.06, 42.86), 105: (9.92, 46.32), 106: (5.59, 45.65),
                107: (6.63, 44.59), 108: (6.86, 51.96), 109: (7.08, 40.74), 110: (6.86, 59.30), 111: (7.00, 46.06), 112: (11.24, 49.50)}
KNOWN_SEEDS = tuple(range(101, 113))
KNOWN_WIDTHS = (1, 2, 4, 8)


def known_hdr():
    k = KNOWN
    return dict(nchans=k["nchan"], nifs=1, nbits=8, fch1=1500.0 - 150.0 / k["nchan"], foff=-300.0 / k["nchan"], tsamp=k["tsamp"], tstart=60000.0,
                product=0)


def known_setup():
    """-> (hdr, the ephemeris folded with, the truth as offsets (dm, dfreq, dfdot), the natural steps)"""
    k, hdr = KNOWN, known_hdr()
    T = k["nrows"] * k["tsamp"]
    ddm, dfreq, dfdot = (float(v) for v in fo.steps(hdr, k["nrows"], k["nbin"], k["f0"]))
    pepoch = hdr["tstart"] + 0.5 * T / 86400.0
    par = {"F0": k["f0"] - k["off_f0"] / T, "F1": k["f1"] - k["off_f1_steps"] * dfdot, "DM": k["dm"] + k["off_dm_steps"] * ddm, "PEPOCH": pepoch,
           "PSR": "known"}
    steps_at = fo.steps(hdr, k["nrows"], k["nbin"], par["F0"])
    truth = dict(dm=k["dm"], dfreq=k["off_f0"] / T, dfdot=k["off_f1_steps"] * dfdot)
    return hdr, par, truth, tuple(float(v) for v in steps_at)


@functools.lru_cache(maxsize=None)
def known_rows(seed, amp=KNOWN_AMP):
    """uint8 rows [nrows][1][nchan]: noise and the dispersed pulse train of the TRUE ephemeris about mid-observation"""
    k, hdr = KNOWN, known_hdr()
    rng = np.random.default_rng(seed)
    t = (np.arange(k["nrows"], dtype=np.float64) - 0.5 * k["nrows"]) * k["tsamp"]
    delay = fo.delay_s(hdr, k["dm"])
    tt = t[:, None] - delay[None, :]
    ph = k["f0"] * tt + 0.5 * k["f1"] * tt * tt
    ph = ph - np.rint(ph)
    x = 96.0 + 16.0 * rng.standard_normal((k["nrows"], k["nchan"])) + amp * np.exp(-0.5 * (ph / k["sigma_turns"]) ** 2)
    rows = np.clip(np.rint(x), 0, 255).astype(np.uint8)[:, None, :]
    rows.setflags(write=False)
    return rows


def known_fold_numpy(rows, hdr, par):
    """the fold restated: cube [nsub][1][nbin][nchan], hits (polynomial about PEPOCH, no channel delays)"""
    k = KNOWN
    nrows, nbin = rows.shape[0], k["nbin"]
    L = fo.rows_per_sub(hdr, k["subint_s"])
    nsub = (nrows + L - 1) // L
    tau = (hdr["tstart"] - par["PEPOCH"]) * 86400.0 + np.arange(nrows, dtype=np.float64) * hdr["tsamp"]
    turns = par["F0"] * tau + (0.5 * par["F1"]) * tau * tau
    b = np.minimum(((turns - np.floor(turns)) * nbin).astype(np.int64), nbin - 1)
    slot = (np.arange(nrows) // L) * nbin + b
    cube = np.zeros((nsub * nbin, k["nchan"]), np.float64)
    np.add.at(cube, slot, rows[:, 0, :].astype(np.float64))
    hits = np.bincount(slot, minlength=nsub * nbin).astype(np.uint32)
    return cube.reshape(nsub, 1, nbin, k["nchan"]), np.repeat(hits.reshape(nsub, nbin, 1), k["nchan"], axis=2).copy(), nsub


def known_grid():
    hdr, par, _truth, (ddm, dfreq, dfdot) = known_setup()
    k = KNOWN
    return dict(f0_fold=par["F0"], subint_s=k["subint_s"], dm0=par["DM"], ndm=k["ndm"], ddm=ddm, nfreq=k["nfreq"], dfreq=dfreq, nfdot=k["nfdot"],
                dfdot=dfdot)


def known_restatement(seed, amp=KNOWN_AMP):
    """numpy alone: fold, search, peaks -> the RESULT record"""
    hdr, par, _truth, _steps = known_setup()
    cube, hits, _nsub = known_fold_numpy(known_rows(seed, amp), hdr, par)
    return fo.fold_fit(cube, hits, hdr, KNOWN["nrows"], products=1, fit_frac=0.5, widths=KNOWN_WIDTHS, **known_grid())["results"][0]


def known_recovered(r):
    """within one grid step of the truth on every axis, and a better S/N than the nominal fold's"""
    _hdr, _par, truth, (ddm, dfreq, dfdot) = known_setup()
    return (abs(r["dm"] - truth["dm"]) <= ddm and abs(r["dfreq"] - truth["dfreq"]) <= dfreq and abs(r["dfdot"] - truth["dfdot"]) <= dfdot
            and r["snr_best"] > r["snr_nominal"])


def known_library(lib, seed):
    """the library: frbch_fold_refine_host on the rows -> (the dict of post.fold_refine, info)"""
    hdr, par, _truth, _steps = known_setup()
    g, k = known_grid(), KNOWN
    rows = known_rows(seed)
    nsub = lib.frbch_fold_nsub(C.byref(post.fil_desc(hdr)), rows.shape[0], k["subint_s"])
    model, _keep = post.fold_model(par, hdr, nbin=k["nbin"], subint_s=k["subint_s"], apply_delays=False)
    fpar = post.foldfit_params(hdr, rows.shape[0], k["nbin"], nsub, g["f0_fold"], k["subint_s"], g["dm0"], products=1, ndm=g["ndm"], nfreq=g["nfreq"],
                               nfdot=g["nfdot"], ddm=g["ddm"], dfreq=g["dfreq"], dfdot=g["dfdot"], fit_frac=0.5, widths=KNOWN_WIDTHS)
    info = {}
    return post.fold_refine(rows, hdr, model, fpar, lib=lib, info=info), info


if __name__ == "__main__":                 # how KNOWN_AMP was fixed: python -m tests.foldfit_cases [amplitude ...]
    import sys
    for amp in [float(a) for a in sys.argv[1:]] or [KNOWN_AMP]:
        rs = [known_restatement(s, amp) for s in KNOWN_SEEDS]
        print("amplitude %.2f: %d of %d recovered" % (amp, sum(known_recovered(r) for r in rs), len(rs)))
        for s, r in zip(KNOWN_SEEDS, rs):
            print("  seed %d: dm %.3f dfreq %.5f dfdot %.3e  S/N %.2f -> %.2f  %s" % (s, r["dm"], r["dfreq"], r["dfdot"], r["snr_nominal"], r["snr_best"],
                                                                                 "ok" if known_recovered(r) else "MISSED"))
