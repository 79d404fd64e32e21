"""Every failure return of the entry points behind the filterbank (csrc/frbch_post.cpp), on the TEST-ONLY emulator build: the
emulator's device layer makes its n-th fallible call (dev_malloc, the copies, the memsets, dev_sync, dev_stream_create,
dev_check_launch) fail once (frbch_test_emu_fail_at), for n = 1, 2, ... until the call succeeds.  tests/golden/post_failure_walk.json
holds, for every entry point, the (n, return code, message) of that walk and the checksum of the outputs of a plain call, as
recorded on the commit BEFORE the entry points were rewritten around PostScope / HostStage (this module run as a program writes
the file).  A case is one (entry point, n):
  * the return code and the message are the recorded ones -- and the walk has the recorded length, since its last entry, and
    no earlier one, returns 0: no allocation, copy or sync was added or lost on any path;
  * the device blocks and streams alive after the call are those alive before it (frbch_test_emu_live);
  * no input of the caller has changed, and no guard band around any buffer;
  * a plain call right afterwards returns 0 and the recorded bytes (a checksum; dedispersion, search, cut-outs and block
    statistics are held to their restatements as well, in a test of their own).
The shapes are the smallest of each family in tests/bounds_cases.py (whose expected bytes the plain call's are: that suite holds
the same calls to the restatements), the interference case of tests/resident_cases.py cut to 3000 rows for frbch_candidates_*,
and two products for frbch_rfi_cleanp_*.  Integer rows throughout: their sums have one value in any order.
The burst family (frbch_burstspec_* to frbch_burstscat_*, both twins of each) joined the table later, recorded in the same way
on the commit BEFORE its entry points were rewritten around burst_device_call / burst_host_twin: each family in the shape of its
own walk test (tests/test_polprof.py, test_dmscan.py, test_acf.py, test_scat.py, both cases of the last two), the three-candidate
case of tests/test_rm.py, and the small planes of tests/test_acf.py and tests/test_scat.py for the two stages.
The delay x RM transform (frbch_rmdelay_*, frbch_burst_polcal_*) joined last, recorded on the commit BEFORE it and RM synthesis
were given one host path: the "generic_nphi63" grid of tests/polcal_cases.py, on its own spectra and on the three-candidate case."""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

from frb_baseband_amd import _lib, cornerturn as ct, post
from tests import acf_cases as ac
from tests import cutout_cases as cc
from tests import cutout_oracle as co
from tests import dmscan_cases as dmc
from tests import polcal_cases as plc
from tests import polprof_cases as ppc
from tests import post_cases as pc
from tests import resident_cases as rs
from tests import rfi_cases as rc
from tests import rfi_oracle as ro
from tests import rm_cases as rmc
from tests import scat_cases as scc
from tests import spsearch_cases as sc
from tests.hipmem import GUARD, POISON, HostGuardedBuffer
from tests.test_spsearch import dispersed_burst_rows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_failure_walk.json")
WALK_LIMIT = 400


class Entry:
    """one entry point with its arguments: call(err) -> rc; ins stay as they are, inouts are put back before every call, outs
    (or result()) are what a plain call is held to"""

    def __init__(self, lib, name):
        self.lib, self.fn = lib, getattr(lib, name)
        self.ins, self.outs, self.inouts, self.keep = [], [], [], []
        self.args = None
        self.result = None                                  # frbch_candidates_*: bytes of the result object, which it frees
        self.want = None                                    # the restatement's bytes of every `out`, where the family has one at hand

    def inp(self, arr):
        self.ins.append(HostGuardedBuffer.from_numpy(arr))
        return self.ins[-1].ptr

    def out(self, nbytes):
        self.outs.append(HostGuardedBuffer(nbytes))
        return self.outs[-1].ptr

    def inout(self, arr):
        self.inouts.append((HostGuardedBuffer.from_numpy(arr), np.ascontiguousarray(arr).copy()))
        return self.inouts[-1][0].ptr

    def hold(self, obj):
        """a ctypes object the arguments point at"""
        self.keep.append(obj)
        return C.byref(obj)

    def call(self, fail_at):
        """-> (rc, message, live before, live after), with the fail_at-th fallible device-layer call failing (0: none)"""
        for buf, arr in self.inouts:
            buf._poke(GUARD, arr)
        for buf in self.outs:
            buf._poke(GUARD, np.full(buf.nbytes, POISON, np.uint8))
        err = C.create_string_buffer(2048)
        before = self.lib.frbch_test_emu_live()
        self.lib.frbch_test_emu_fail_at(fail_at)
        try:
            code = self.fn(*self.args, err, len(err))
        finally:
            self.lib.frbch_test_emu_fail_at(0)
        after = self.lib.frbch_test_emu_live()
        self.got = self.result() if self.result else None
        return code, err.value.decode() if code else "", before, after

    def unchanged(self):
        for buf in self.ins:
            buf.check(contents=True)
        for buf in self.outs + [b for b, _ in self.inouts]:
            buf.check()

    def out_bytes(self):
        return [buf._peek(GUARD, buf.nbytes).tobytes() for buf in self.outs]

    def crc(self):
        """checksum of everything a successful call wrote"""
        c = zlib.crc32(self.got) if self.result else 0
        for buf in self.outs + [b for b, _ in self.inouts]:
            c = zlib.crc32(buf._peek(GUARD, buf.nbytes), c)
        for obj in self.keep:
            if isinstance(obj, (C.c_uint32, C.c_uint64)):               # nclipped, ncand, kernel_used
                c = zlib.crc32(bytes(obj), c)
        return c


def _dms(e, dms):
    arr = np.ascontiguousarray(dms, dtype=np.float64)
    e.keep.append(arr)
    return arr.ctypes.data, arr.size


# ---- the entry points ---------------------------------------------------------------------------------------------------------
def _dedisp_rows(nout, ndm):
    hdr = pc.make_hdr(64)
    dms = [20.0 + 1.5 * i for i in range(ndm)]
    from oracle import post_oracle as po
    nrows = nout + int(po.delays_samples(hdr["fch1"], hdr["foff"], 64, hdr["tsamp"], dms[-1]).max())
    return hdr, dms, pc.make_rows(nrows, 2, 64, 8, seed=31, hdr=hdr)


def _dedisperse(twin, nout, ndm, zerodm, clip):
    def make(lib):
        e = Entry(lib, "frbch_dedisperse_" + twin)
        hdr, dms, rows = _dedisp_rows(nout, ndm)
        dm_ptr, _ = _dms(e, dms)
        e.args = [e.hold(pc.desc_of(hdr, rows, 1)), e.inp(rows), rows.shape[0], dm_ptr, ndm, 1 if zerodm else 0, float(clip), 0,
                  e.out(ndm * nout * 4), nout, e.hold(C.c_uint64(1 << 40))]
        e.want = lambda: [pc.want_dedisp(rows, hdr, 1, dms, zerodm, clip)[0].astype(np.float32).tobytes()]
        return e
    return make


def _dedisperse_search(lib):
    e = Entry(lib, "frbch_dedisperse_search_host")
    nout, ndm = 257, 9
    hdr, dms, rows = _dedisp_rows(nout, ndm)
    dm_ptr, _ = _dms(e, dms)
    cap = 4096
    e.args = [e.hold(pc.desc_of(hdr, rows, 1)), e.inp(rows), rows.shape[0], dm_ptr, ndm, 1, 5.0, e.hold(post.sp_params([1, 2, 4], 5.0, 64)), 0,
              e.out(ndm * nout * 4), nout, e.hold(C.c_uint64(1 << 40)), e.out(cap * post.SP_CAND.itemsize), cap, e.hold(C.c_uint64(0)),
              e.hold(C.c_uint32(99))]
    return e


def _fold(twin, all_products, nchan, nifs, nbits, nbin, nrows, rps, delays):
    def make(lib):
        e = Entry(lib, ("frbch_foldp_" if all_products else "frbch_fold_") + twin)
        hdr = pc.make_hdr(nchan)
        rows = pc.make_rows(nrows, nifs, nchan, nbits, seed=32, hdr=hdr)
        subint_s = (rps + 0.25) * hdr["tsamp"]
        nsub = -(-nrows // rps)
        nslot = nsub * nbin * nchan
        full = dict(hdr, nifs=nifs, nbits=nbits)
        if all_products:
            model, keep = post.fold_model(pc.PAR, full, nbin=nbin, subint_s=subint_s, apply_delays=delays)
            e.keep.append(keep)
            e.args = [e.hold(post.fil_desc(full)), e.inp(rows), nrows, e.hold(model), 0, e.out(nslot * nifs * 8), e.out(nslot * 4), nsub,
                      e.hold(C.c_uint32(99))]
        else:
            e.args = [e.hold(post.fil_desc(full, product=nifs - 1)), e.inp(rows), nrows, pc.PAR["F0"], pc.PAR["F1"], pc.PAR["PEPOCH"], pc.PAR["DM"],
                      1 if delays else 0, nbin, subint_s, 0, e.out(nslot * 8), e.out(nslot * 4), nsub]
        return e
    return make


def _spsearch(twin):
    def make(lib):
        e = Entry(lib, "frbch_spsearch_" + twin)
        y, widths, thr, L, want, _raws = sc.case("small_L64_w1")
        e.args = [e.inp(y), y.shape[0], y.shape[1], e.hold(post.sp_params(list(widths), thr, L)), 0, e.out(want.size * post.SP_CAND.itemsize),
                  want.size, e.hold(C.c_uint64(0)), e.hold(C.c_uint32(99))]
        e.want = lambda: [np.ascontiguousarray(want).tobytes()]
        return e
    return make


def _cutout(twin):
    def make(lib):
        e = Entry(lib, "frbch_cutout_" + twin)
        cs = cc._case(64, 16, 3000, 2, 2, 1, [(56.7, 1500, 3)])
        n, nf, nt, ndm = cs["cands"].size, cs["nf"], cs["nt"], cs["ndm"]
        e.args = [e.hold(cc.desc_of(cs)), e.inp(cs["rows"]), cs["rows"].shape[0], e.hold(cc.params(nt, nf, ndm)), e.inp(cs["cands"]), n, 0,
                  e.out(n * nf * nt * 4), e.out(n * nf * nt * 4), e.out(n * ndm * nt * 4), e.out(n * ndm * nt * 4), e.hold(C.c_uint32(99))]
        e.want = lambda: [np.ascontiguousarray(w).tobytes() for w in co.planes_batch(cs["rows"][:, cs["prod"], :], cs["hdr"], cs["cands"], nt, nf, ndm)]
        return e
    return make


def _rfi(stage, twin, nifs=1):
    def make(lib):
        e = Entry(lib, "frbch_rfi_%s_%s" % (stage, twin))
        nchan, br, nrows = 64, 64, 200
        rows = rc.make_rows(nrows, nifs, nchan, 8, seed=nchan + nrows + nifs - 1)
        nblk = -(-nrows // br)
        head = [e.hold(rc.desc_of(rows, 0)), None, nrows, e.hold(rc.params(block_rows=br, t_cell=3.0))]
        if stage == "stats":
            head[1] = e.inp(rows)
            e.args = head + [0, e.out(nblk * nchan * 16), e.hold(C.c_uint32(99))]
            e.want = lambda: [ro.stats(rows[:, 0, :], br).tobytes()]
        elif stage == "apply":
            res = ro.mask(ro.stats(rows[:, 0, :], br), nrows, br, 8, **dict(rc.rule_kw(rc.DEFAULTS), t_cell=3.0))
            assert res["mask"].any()
            head[1] = e.inout(rows)
            e.args = head + [e.inp(res["mask"]), e.inp(res["repl"]), 0]
        else:
            head[1] = e.inout(rows)
            e.args = head + [None, 0, e.out(nblk * nchan), e.out((nifs if stage == "cleanp" else 1) * nchan * 8), e.out(nchan), e.out(nblk)]
            if stage == "cleanp":
                e.args.append(e.out(nifs * nblk * nchan * 16))
            e.args.append(e.hold(C.c_uint32(99)))
        return e
    return make


def _cornerturn(twin):
    def make(lib):
        e = Entry(lib, "frbch_cornerturn_" + twin)
        mode = "VDIF_8000-32-4-2"
        _fps, recipe, _bits = ct.MODES[mode]
        hb, pin, _ = ct.frame_geometry(mode)
        frames = np.random.default_rng(1).integers(0, 256, size=(1, hb + pin), dtype=np.uint8)
        info = ct.recipe_info(recipe, lib)
        each = pin * 8 // info["word_bits"] * info["bits_per_word"] // 8
        ptrs = (C.c_void_p * info["ntags"])(*[e.out(each).value for _ in range(info["ntags"])])
        e.keep.append(ptrs)
        e.args = [recipe.encode(), e.inp(frames), 1, hb + pin, hb, ptrs, info["ntags"], each, 0]
        return e
    return make


def _candidates(twin):
    def make(lib):
        e = Entry(lib, "frbch_candidates_" + twin)
        hdr = rs.hdr_of()
        x = dispersed_burst_rows(3000, hdr, rs.BURST_DMS[4], 800, 5, 30).astype(np.int64)
        x[:, rs.DEAD_CHANNEL] = 100
        x[rs.LOUD_ROWS[0]:rs.LOUD_ROWS[1], rs.LOUD_CHANNEL] += 90
        rows = np.clip(x, 0, 255).astype(np.uint8)[:, None, :]
        s = rs.settings(rfi=rs.RFI, zap=[rs.ZAP_CHANNEL], keep_series=True)
        par = rs.cand_par(hdr, s)
        zap = rs.zap_of(s, hdr)
        e.keep.append(zap)
        par.flags |= _lib.CAND_SERIES
        par.zap = zap.ctypes.data
        dm_ptr, ndm = _dms(e, s["dms"])
        res = C.c_void_p(0)
        e.keep.append(res)
        e.args = [e.hold(post.fil_desc(hdr, 0)), e.inp(rows), rows.shape[0], dm_ptr, ndm, e.hold(par), 0, C.byref(res)]

        def result():
            if not res.value:
                return b""
            v = _lib.FrbchCandView()
            v.size = C.sizeof(v)
            assert lib.frbch_cand_result_view(res, C.byref(v)) == 0
            assert v.ngroup >= 1 and v.ft and v.mask and v.series and v.row_uploads == (1 if twin == "host" else 0)
            ft, dt, ncell = v.ngroup * s["nf"] * s["nt"] * 4, v.ngroup * s["ndm"] * s["nt"] * 4, v.nblk * hdr["nchans"]
            assert any(C.string_at(v.mask, ncell))
            parts = [(v.cands, v.ncand * C.sizeof(_lib.FrbchSpCand)), (v.groups, v.ngroup * C.sizeof(_lib.FrbchSpGroup)),
                     (v.cut_cands, v.ngroup * C.sizeof(_lib.FrbchCutoutCand)), (v.ft, ft), (v.ft_hits, ft), (v.dt, dt), (v.dt_hits, dt),
                     (v.mask, ncell), (v.repl, hdr["nchans"] * 8), (v.chan_flag, hdr["nchans"]), (v.blk_flag, v.nblk), (v.series, ndm * v.nout * 4)]
            got = b"".join(C.string_at(p, n) for p, n in parts) + bytes(C.c_uint64(v.nclipped)) + bytes(C.c_uint64(v.ngroup_all))
            lib.frbch_cand_result_free(res)
            res.value = 0
            return got
        e.result = result
        return e
    return make


# ---- the burst family: the shapes of each family's own walk test (tests/test_polprof.py, test_dmscan.py, test_acf.py, test_scat.py),
# ---- the three-candidate case of tests/test_rm.py and the small planes of the two stages -------------------------------------------
def _kused(e, n):
    k = (C.c_uint32 * n)(*([99] * n))
    e.keep.append(k)
    return k


def _opt(e, arr):
    return e.inp(arr) if arr is not None else None


def _burst_head(e, hdr, rows, cands, coh, product=0):
    """fil, rows, nrows, burst params, cands, ncand: what every composite of the family begins with"""
    fil = post.fil_desc(dict(hdr, nifs=rows.shape[1], nbits=rows.dtype.itemsize * 8), product)
    return [e.hold(fil), e.inp(rows), rows.shape[0], e.hold(rmc.burst_par(coh)), e.inp(cands), cands.size]


def _burstspec(twin):
    def make(lib):
        e = Entry(lib, "frbch_burstspec_" + twin)
        hdr, rows, cands, coh = rmc.case("u8_64ch_3cand")
        n = cands.size * 4 * 64
        e.args = _burst_head(e, hdr, rows, cands, coh) + [None, 0, e.out(n * 32), e.out(n * 4), e.out(n * 4), e.out(cands.size * 64),
                                                          e.hold(C.c_uint32(99))]
        e.want = lambda: [np.ascontiguousarray(a).tobytes() for a in rmc.want_spectra("u8_64ch_3cand")]
        return e
    return make


def _rmsynth(twin):
    def make(lib):
        e = Entry(lib, "frbch_rmsynth_" + twin)
        hdr, q, u, used = rmc.spectra(64, 3, 0, (3, 40))
        e.args = [e.hold(post.fil_desc(hdr)), e.inp(q), e.inp(u), e.inp(used), 3, e.hold(post.rm_params(**rmc.GRID)), 0,
                  e.out(3 * rmc.GRID["nphi"] * 8), _kused(e, 2)]
        e.want = lambda: [rmc.want_transform(64, 3, rmc.GRID["nphi"], rmc.GRID["phi_lo"], rmc.GRID["dphi"], 0, (3, 40)).tobytes()]
        return e
    return make


def _burst_rm(twin):
    def make(lib):
        e = Entry(lib, "frbch_burst_rm_" + twin)
        hdr, rows, cands, coh = rmc.case("u8_64ch_3cand")
        n, nphi = cands.size * 64, rmc.GRID["nphi"]
        e.args = _burst_head(e, hdr, rows, cands, coh) + [None, None, e.hold(post.rm_params(**rmc.GRID)), 0, e.out(n * 16), e.out(n * 16), e.out(n),
                                                          e.out(cands.size * nphi * 8), e.out(cands.size * post.RM_RESULT.itemsize), _kused(e, 3)]
        return e
    return make


def _rmdelay(twin):
    def make(lib):
        e = Entry(lib, "frbch_rmdelay_" + twin)
        nchan, ncand, _nphi, _lo, _d, _ntau, _tlo, _dt, masked = plc.SHAPES["generic_nphi63"]
        grid = plc.grid_of("generic_nphi63")
        hdr, q, u, used = rmc.spectra(nchan, ncand, 0, masked)
        e.args = [e.hold(post.fil_desc(hdr)), e.inp(q), e.inp(u), e.inp(used), ncand, e.hold(post.rmd_params(**grid)), 0,
                  e.out(ncand * grid["ntau"] * grid["nphi"] * 8), _kused(e, 2)]
        e.want = lambda: [plc.want_transform("generic_nphi63").tobytes()]
        return e
    return make


def _burst_polcal(twin):
    def make(lib):
        e = Entry(lib, "frbch_burst_polcal_" + twin)
        hdr, rows, cands, coh = rmc.case("u8_64ch_3cand")
        grid = plc.grid_of("generic_nphi63")
        n, per = cands.size * 64, grid["ntau"] * grid["nphi"]
        e.args = _burst_head(e, hdr, rows, cands, coh) + [None, None, e.hold(post.rmd_params(**grid)), 0, e.out(n * 16), e.out(n * 16), e.out(n),
                                                          e.out(cands.size * per * 8), e.out((cands.size + 1) * post.RMD_RESULT.itemsize), _kused(e, 3)]
        return e
    return make


def _polprof(twin):
    def make(lib):
        e = Entry(lib, "frbch_polprof_" + twin)
        c = ppc.case("u8_64ch_33x3")
        n, nbin = c["cands"].size, c["nbin"]
        e.args = _burst_head(e, c["hdr"], c["rows"], c["cands"], c["coh"]) + [
            e.inp(c["rm"]), _opt(e, c["gain"]), _opt(e, c["flag"]), e.hold(ppc.par_of(c)), 0, e.out(n * nbin * 32), e.out(n * nbin * 4),
            e.out(n * nbin * post.PROF_BIN.itemsize), e.out(n * post.PROF_RESULT.itemsize), e.out(n * 64), _kused(e, 2)]
        return e
    return make


def _dmscan(twin):
    def make(lib):
        e = Entry(lib, "frbch_dmscan_" + twin)
        c = dmc.case("u8_64ch_33x33x3")
        n, nt, nbin = c["cands"].size, c["ntrial"], c["nbin"]
        e.args = _burst_head(e, c["hdr"], c["rows"], c["cands"], c["coh"], c["hdr"].get("product", 0)) + [
            _opt(e, c["flag"]), e.hold(dmc.par_of(c)), e.hold(dmc.peak_par_of(c)), 0, e.out(n * nt * nbin * 8), e.out(n * nt * nbin * 4),
            e.out(n * nt * 8), e.out(n * nt * 8), e.out(n * post.DMSCAN_RESULT.itemsize), e.out(n * c["hdr"]["nchans"]), _kused(e, 2)]
        w = dmc.want("u8_64ch_33x33x3")
        e.want = lambda: [np.ascontiguousarray(w[f]).tobytes() for f in ("acc", "hits", "snr", "struct", "results", "used")]
        return e
    return make


def _acf2d(twin):
    def make(lib):
        e = Entry(lib, "frbch_acf2d_" + twin)
        name = "random_3x5_full_lags"
        n, nsub, nbin, lf, lt, _kind = ac.PLANES[name]
        e.args = [e.inp(ac.plane(name)), n, nsub, nbin, lf, lt, _lib.ACF_PLAN, 0, e.out(n * lf * (2 * lt - 1) * 8), e.hold(C.c_uint32(99))]
        e.want = lambda: [ac.plane_want(name).tobytes()]
        return e
    return make


def _burstacf(twin, name):
    def make(lib):
        e = Entry(lib, "frbch_burstacf_" + twin)
        c = ac.case(name)
        out = ac.outputs_of(c)
        e.args = _burst_head(e, c["hdr"], c["rows"], c["cands"], c["coh"], c["hdr"].get("product", 0)) + [
            _opt(e, c["flag"]), e.hold(ac.par_of(c)), e.hold(ac.fit_par_of(c)), 0] + [
            e.out(out[f].nbytes) for f in ("Y", "yhits", "A", "P", "results", "used")] + [_kused(e, 3)]
        return e
    return make


def _tbank(twin):
    def make(lib):
        e = Entry(lib, "frbch_tbank_" + twin)
        name = "three_planes"
        y, P = scc.plane(name)
        e.args = [e.inp(y), e.inp(P), scc.PLANES[name][0], e.hold(scc.shape_of(name)), _lib.TBANK_PLAN, 0, e.out(scc.plane_want(name).nbytes),
                  e.hold(C.c_uint32(99))]
        e.want = lambda: [scc.plane_want(name).tobytes()]
        return e
    return make


def _burstscat(twin, name):
    def make(lib):
        e = Entry(lib, "frbch_burstscat_" + twin)
        c = scc.case(name)
        out = scc.outputs_of(c)
        e.args = _burst_head(e, c["hdr"], c["rows"], c["cands"], c["coh"], c["hdr"].get("product", 0)) + [
            _opt(e, c["flag"]), e.hold(scc.par_of(c)), e.hold(scc.bank_par(c["bp"])), e.hold(scc.fit_par_of(c)), 0] + [
            e.out(out[f].nbytes) for f in ("Y", "yhits", "y", "C", "N", "sub", "band", "used")] + [_kused(e, 3)]
        return e
    return make


ENTRIES = {}
for _twin in ("device", "host"):
    ENTRIES["dedisperse_" + _twin] = _dedisperse(_twin, 1, 1, False, 0.0)
    ENTRIES["dedisperse_zerodm_clip_" + _twin] = _dedisperse(_twin, 257, 9, True, 5.0)
    for _all in (False, True):
        ENTRIES["fold%s_%s" % ("p" if _all else "", _twin)] = _fold(_twin, _all, 16, 1, 8, 2, 777, 300, False)
        ENTRIES["fold%s_delays_%s" % ("p" if _all else "", _twin)] = _fold(_twin, _all, 48, 3, 8, 256, 1001, 400, True)
    ENTRIES["spsearch_" + _twin] = _spsearch(_twin)
    ENTRIES["cutout_" + _twin] = _cutout(_twin)
    for _stage in ("stats", "apply", "clean"):
        ENTRIES["rfi_%s_%s" % (_stage, _twin)] = _rfi(_stage, _twin)
    ENTRIES["rfi_cleanp_2products_" + _twin] = _rfi("cleanp", _twin, nifs=2)
    ENTRIES["cornerturn_" + _twin] = _cornerturn(_twin)
    ENTRIES["candidates_rfi_planes_" + _twin] = _candidates(_twin)
    for _name, _make in (("burstspec", _burstspec), ("rmsynth", _rmsynth), ("burst_rm", _burst_rm), ("rmdelay", _rmdelay), ("burst_polcal", _burst_polcal),
                         ("polprof", _polprof), ("dmscan", _dmscan), ("acf2d", _acf2d), ("tbank", _tbank)):
        ENTRIES["%s_%s" % (_name, _twin)] = _make(_twin)
    for _case in ("u8_64ch_f4_full_lags", "u8_64ch_flag_constant_dead"):                        # (the second counts its pairs on the device)
        ENTRIES["burstacf_%s_%s" % (_case, _twin)] = _burstacf(_twin, _case)
    for _case in ("u8_64ch_f4_mixed_dms", "u8_64ch_flag_dead_subband"):                         # (the second forms N on the device)
        ENTRIES["burstscat_%s_%s" % (_case, _twin)] = _burstscat(_twin, _case)
ENTRIES["dedisperse_search_host"] = _dedisperse_search

_made = {}


def entry(lib, name):
    if name not in _made:
        _made.clear()                                       # (the cases come entry point by entry point: one set of buffers at a time)
        lib.frbch_test_emu_fail_at.argtypes, lib.frbch_test_emu_fail_at.restype = [C.c_long], None
        lib.frbch_test_emu_live.argtypes, lib.frbch_test_emu_live.restype = [], C.c_uint64
        _made[name] = ENTRIES[name](lib)
    return _made[name]


def record(lib):
    """the walk of every entry point on the library as it is -> what the golden file holds"""
    table = {}
    for name in ENTRIES:
        e = entry(lib, name)
        code, msg, _, _ = e.call(0)
        assert code == 0, (name, msg)
        crc = e.crc()
        walk = []
        for n in range(1, WALK_LIMIT):
            code, msg, _, _ = e.call(n)
            walk.append([n, code, msg])
            if code == 0:
                break
        assert walk[-1][1] == 0, name
        table[name] = dict(crc32=crc, walk=walk)
    return table


def dump(table):
    """the golden file: one walk entry per line"""
    parts = []
    for name in sorted(table):
        walk = ",\n".join("   " + json.dumps(w) for w in table[name]["walk"])
        parts.append(' %s: {"crc32": %d, "walk": [\n%s\n  ]}' % (json.dumps(name), table[name]["crc32"], walk))
    return "{\n" + ",\n".join(parts) + "\n}\n"


TABLE = {}
if os.path.exists(GOLDEN):                                  # (absent only while this module, as a program, records it)
    with open(GOLDEN) as _f:
        TABLE = json.load(_f)


def test_the_table_covers_every_entry_point():
    assert sorted(TABLE) == sorted(ENTRIES)
    for name, t in TABLE.items():
        codes = [w[1] for w in t["walk"]]
        assert [w[0] for w in t["walk"]] == list(range(1, len(codes) + 1)) and codes[-1] == 0 and all(codes[:-1]), name
        if name.endswith("_device"):                        # the two twins of a stage write the same bytes
            assert t["crc32"] == TABLE[name[:-len("device")] + "host"]["crc32"], name


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_a_plain_call_writes_what_the_restatement_expects(emu_lib, name):
    """the bytes behind the recorded checksum, against the restatements tests/bounds_cases.py uses, for the families that have
    one at hand for these arguments (dedispersion, search, cut-outs, block statistics); the other entry points have the
    checksum alone, and tests/test_bounds.py for their bytes"""
    e = entry(emu_lib, name)
    code, msg, _, _ = e.call(0)
    assert code == 0, msg
    assert e.crc() == TABLE[name]["crc32"]
    if e.want:
        got, want = e.out_bytes(), e.want()
        assert [len(g) for g in got] == [len(w) for w in want]
        assert [i for i, (g, w) in enumerate(zip(got, want)) if g != w] == [], "outputs (by position) that differ from the restatement"


@pytest.mark.parametrize("name,n", [(name, w[0]) for name, t in sorted(TABLE.items()) for w in t["walk"]])
def test_a_failing_device_call_returns_as_recorded_and_leaves_nothing_behind(emu_lib, name, n):
    e = entry(emu_lib, name)
    _, want_code, want_msg = TABLE[name]["walk"][n - 1]
    code, msg, before, after = e.call(n)
    assert (code, msg) == (want_code, want_msg)
    assert after == before, "device blocks / streams alive: %#x before the call, %#x after it" % (before, after)
    e.unchanged()
    if code == 0:
        assert e.crc() == TABLE[name]["crc32"]
        return
    assert not e.got                                        # (no result object from a failed frbch_candidates_*)
    code, msg, before, after = e.call(0)
    assert code == 0, msg
    assert e.crc() == TABLE[name]["crc32"], "the plain call after the failed one gave other bytes"
    assert after == before
    e.unchanged()


if __name__ == "__main__":
    import subprocess
    emu_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    subprocess.check_call(["make", "-s", "-C", emu_dir])
    with open(GOLDEN, "w") as f:
        f.write(dump(record(_lib.load(os.path.join(emu_dir, "libfrbch_emu.so")))))
