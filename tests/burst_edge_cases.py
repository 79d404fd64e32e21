"""Shared case builder of the burst polarisation kernels at the edges of their plans (tests/test_burst_edges.py on the emulator
build, tests/test_gpu_burst_edges.py on the device): windows of the burst sums that take more than one chunk of
kBsGroups * kBsRun = 16384 rows, samples at full scale up to the documented maximum of off_len and width, one to three
products, ascending bands; and the profile where its plan rule turns (tfactor + spread = 256 | 257), with delays that fall with
the channel index, candidates of very different DM in one call, a tile without a used channel, candidates 2^62 rows away and
the cap on the partials.  Every case states what it is there for as a condition on the restatement (`burst_conditions`,
`prof_conditions`), asserted before a library runs.

The burst sums are expected from `window_sums`, a second restatement by per-channel prefix sums (tests/rm_oracle.burst_sums
walks the rows in Python: minutes at 2 x 10^6 rows); tests/test_burst_edges.py holds the two equal on every case of
tests/rm_cases.py and on the small cases here.  The profile is tests/polprof_oracle.py's."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import post
from tests import big_rows as bg
from tests import hipmem
from tests import polprof_cases as pc
from tests import polprof_oracle as ppo
from tests import rm_cases as rc
from tests import rm_oracle as ro

FAST, GENERIC = 1, 0
CHUNK = 64 * 256              # kBsGroups * kBsRun: the rows of one trip of the fast burst-sums kernel's chunk loop
SPAN = 256                    # kPpSpan: the rows of the fast profile kernel's stage
PART_CAP = 1 << 30            # kPolPartCap: bytes of tile partials
DTYPES = {8: np.uint8, 16: np.uint16}


# ---- the second restatement of the burst sums ------------------------------------------------------------------------
def window_sums(x, hdr, cands, c0=0):
    """x [nrows][nifs][nchan] integers -> BURST_SUMS [ncand][nifs][nchan]: per-channel prefix sums of x and of x x in int64,
    differenced at clip(w0 + d, 0, nrows) and clip(w0 + d + len, 0, nrows) of every window.  x may hold a block of the header's
    channels, c0 .. c0 + nchan - 1 (a block at a time keeps the int64 plane of 65 536 channels small)"""
    nrows, nifs, nchan = x.shape
    assert x.dtype in (np.uint8, np.uint16)
    out = np.zeros((len(cands), nifs, nchan), dtype=post.BURST_SUMS)
    chans = np.arange(nchan)
    edges = []
    for i, cd in enumerate(cands):
        d = ro.delays(hdr, float(cd["dm"]))[c0:c0 + nchan]
        edges.append([(which, np.clip(w0 + d, 0, nrows), np.clip(w0 + d + length, 0, nrows)) for w0, length, which in ro.windows(cd)])
        hits = np.zeros((2, nchan), np.int64)
        for which, lo, hi in edges[-1]:
            hits[which] += hi - lo
        out[i]["on_hits"], out[i]["off_hits"] = hits[0][None, :], hits[1][None, :]
    cs = np.zeros((nrows + 1, nchan), np.int64)
    for p in range(nifs):
        for square in (False, True):
            if square:
                v = x[:, p, :].astype(np.int64)
                v *= v
                ro.cumsum_rows(v, cs)
                del v
            else:
                ro.cumsum_rows(x[:, p, :], cs)
            for i, e in enumerate(edges):
                tot = np.zeros((2, nchan), np.int64)
                for which, lo, hi in e:
                    tot[which] += cs[hi, chans] - cs[lo, chans]
                assert int(tot.max()) < 1 << 53                     # exact as doubles
                if square:
                    out[i]["off_sumsq"][p] = tot[1]
                else:
                    out[i]["on_sum"][p], out[i]["off_sum"][p] = tot[0], tot[1]
    return out


def walked(hdr, nbits, nrows, cand):
    """what the fast burst-sums kernel walks, from the restatement's delays -> [(tile, window, rows, trips of the chunk loop)]:
    a workgroup takes the rows w0 + dmin .. w0 + len - 1 + dmax of its 64-byte tile, clipped to the file, CHUNK rows a trip"""
    ct = 64 // (nbits // 8)
    d = ro.delays(hdr, float(cand["dm"])).reshape(-1, ct)
    out = []
    for t in range(d.shape[0]):
        dmin, dmax = int(d[t].min()), int(d[t].max())
        for w, (w0, length, _which) in enumerate(ro.windows(cand)):
            first, last = max(0, w0 + dmin), min(nrows - 1, w0 + length - 1 + dmax)
            n = max(0, last - first + 1)
            out.append((t, w, n, -(-n // CHUNK)))
    return out


def tile_spreads(hdr, nbits, dm):
    """largest minus smallest delay of every whole 64-byte tile of a row"""
    ct = 64 // (nbits // 8)
    d = ro.delays(hdr, float(dm))
    d = d[: d.size // ct * ct].reshape(-1, ct)
    return d.max(axis=1) - d.min(axis=1)


# ---- burst-sums cases ------------------------------------------------------------------------------------------------
DM = 56.7
BURSTS = [rc.B1, rc.B2, rc.B_EDGE]


def near_full_scale(nrows, nifs, nchan, nbits, seed):
    """codes within 300 (16 bit) / 5 (8 bit) of the largest, never constant: a row taken twice for one missed changes a sum"""
    rng = np.random.default_rng(4000 + seed)
    top, depth = (65535, 300) if nbits == 16 else (255, 5)
    return (top - rng.integers(0, depth + 1, size=(nrows, nifs, nchan), dtype=np.uint16)).astype(DTYPES[nbits])


def _one_chunk(extra):
    hdr = dict(rc.make_hdr(64), nbits=8)
    spread = int(tile_spreads(hdr, 8, DM).max())
    off_len, gap, width = CHUNK - spread + extra, 16, 6
    on_lo = 40 + off_len + gap
    burst = dict(rc.B1, sample=on_lo + width // 2)
    nrows = on_lo + width + gap + off_len + int(ro.delays(hdr, DM).max()) + 40
    return hdr, rc.burst_file(hdr, nrows, 8, [burst], seed=3 + extra), rc.cands_of([burst], gap, off_len), False


def _three_chunks(nbits):
    nchan = 32 if nbits == 16 else 64                      # one 64-byte tile either way
    hdr = dict(rc.make_hdr(nchan), nbits=nbits)
    nrows = 110000
    # an interior candidate; one whose earlier off window starts 20000 rows in front of row 0; one whose later off window
    # starts at row 90000 and is cut at nrows, 20000 rows on: inside the second trip
    cands = post.burst_cands([(DM, 52000, 20000), (DM, 30016, 20000), (DM, 79984, 20000)], 16, 40000)
    return hdr, near_full_scale(nrows, 4, nchan, nbits, nbits), cands, False


def _documented_maximum():
    hdr = dict(rc.make_hdr(32), nbits=16)
    off_len, width, gap = 1 << 20, 65536, 16
    on_lo = off_len + gap                                  # the earlier off window starts at row 0
    nrows = on_lo + width + gap + off_len + int(ro.delays(hdr, DM).max())       # the later one ends with the file in the most delayed channel
    return hdr, near_full_scale(nrows, 1, 32, 16, 99), post.burst_cands([(DM, on_lo + width // 2, width)], gap, off_len), False


def _nifs(nifs, nbits):
    hdr = dict(rc.make_hdr(64), nbits=nbits)
    rows = np.ascontiguousarray(rc.burst_file(hdr, 4096, nbits, BURSTS, seed=10 * nifs + nbits)[:, :nifs])
    return hdr, rows, rc.cands_of(BURSTS), False


def _ascending(nchan, nbits, bursts, off_len):
    hdr = dict(rc.make_hdr(nchan, foff_sign=1), nbits=nbits)
    return hdr, rc.burst_file(hdr, 4096, nbits, bursts, seed=nchan), rc.cands_of(bursts, 16, off_len), False


BURST_CASES = {
    "one_chunk_exactly": lambda: _one_chunk(0),
    "one_row_into_the_second": lambda: _one_chunk(1),
    "three_chunks_full_scale_u16": lambda: _three_chunks(16),
    "three_chunks_full_scale_u8": lambda: _three_chunks(8),
    "documented_maximum": _documented_maximum,
    "nifs_1": lambda: _nifs(1, 8),
    "nifs_2": lambda: _nifs(2, 8),
    "nifs_2_u16": lambda: _nifs(2, 16),
    "nifs_3": lambda: _nifs(3, 8),
    "ascending_u8": lambda: _ascending(64, 8, BURSTS, 200),
    "ascending_u16_1024": lambda: _ascending(1024, 16, [rc.B2, rc.B_LATE], 300),
}
LARGE = ("three_chunks_full_scale_u16", "three_chunks_full_scale_u8", "documented_maximum")      # window_sums only: too many rows for the row walk


@functools.lru_cache(maxsize=None)
def burst_case(name):
    """-> (hdr, rows, cands, coherency); the arrays are read-only"""
    hdr, rows, cands, coh = BURST_CASES[name]()
    rows.setflags(write=False)
    cands.setflags(write=False)
    return hdr, rows, cands, coh


@functools.lru_cache(maxsize=None)
def burst_want(name):
    """-> (sums, spec, noise, used): window_sums and the oracle's derivation"""
    hdr, rows, cands, coh = burst_case(name)
    sums = window_sums(rows, hdr, cands)
    out = (sums,) + ro.derive(sums, None, coh)
    for a in out:
        a.setflags(write=False)
    return out


def burst_conditions(name):
    """what the case is there for, on the restatement alone"""
    hdr, rows, cands, _coh = burst_case(name)
    nrows, nbits = rows.shape[0], hdr["nbits"]
    walks = [walked(hdr, nbits, nrows, cd) for cd in cands]
    spread = int(tile_spreads(hdr, nbits, float(cands[0]["dm"])).max())
    trips = lambda i, w: [k for _t, ww, _n, k in walks[i] if ww == w]
    rows_of = lambda i, w: [n for _t, ww, n, _k in walks[i] if ww == w]
    if name in ("one_chunk_exactly", "one_row_into_the_second"):
        extra = 0 if name == "one_chunk_exactly" else 1
        assert spread == 84 and int(cands[0]["off_len"]) == CHUNK - spread + extra
        for w in (0, 2):                                   # both off windows lie inside the file
            assert rows_of(0, w) == [CHUNK + extra] and trips(0, w) == [1 + extra]
        assert trips(0, 1) == [1]
    elif name.startswith("three_chunks"):
        assert int(rows.min()) >= (65000 if nbits == 16 else 250) and int(rows.max()) == (65535 if nbits == 16 else 255)
        assert len(walks[0]) == 3                          # one tile
        assert rows_of(0, 0) == rows_of(0, 2) == [40000 + spread] and trips(0, 0) == trips(0, 2) == [3] and trips(0, 1) == [2]
        w0 = ro.windows(cands[1])[0][0]
        assert w0 < -CHUNK and 0 < rows_of(1, 0)[0] < 40000 and trips(1, 0) == [2]          # starts more than a chunk in front of row 0
        w0 = ro.windows(cands[2])[2][0]
        assert w0 + 40000 > nrows and rows_of(2, 2) == [nrows - w0] and trips(2, 2) == [2] and (nrows - w0) % CHUNK != 0     # cut inside a trip
    elif name == "documented_maximum":
        assert int(cands[0]["off_len"]) == 1 << 20 and int(cands[0]["width"]) == 65536 and rows.shape[1] == 1 and int(rows.min()) >= 65000
        assert trips(0, 0) == trips(0, 2) == [-(-((1 << 20) + spread) // CHUNK)] == [65] and trips(0, 1) == [5]
        sums = burst_want(name)[0]
        assert (sums["off_hits"] == 1 << 21).all() and (sums["on_hits"] == 65536).all()
        assert float(1 << 52) < float(sums["off_sumsq"].max()) < float(1 << 53)
    elif name.startswith("nifs_"):
        assert rows.shape[1] == int(name[5]) and rows.shape[0] == 4096
    else:
        d = ro.delays(hdr, float(cands[-1]["dm"]))
        assert hdr["foff"] > 0 and (np.diff(d) <= 0).all() and d[0] == d.max() > 0 and d[-1] == 0       # delays fall with the channel index
        if name == "ascending_u16_1024":
            assert d.max() > 3000 and len(walks[0]) == 3 * 32
    return walks


def spectra_kernel_expected(lib, hdr, rows, misalign):
    if hipmem.guarded_for(lib) is hipmem.HostGuardedBuffer:
        return GENERIC                                     # the emulator build has no fast kernel
    return FAST if rows.shape[1] <= 4 and (hdr["nchans"] * rows.dtype.itemsize) % 64 == 0 and misalign % 16 == 0 else GENERIC


# ---- the calls: rows and sums in guarded buffers of exactly their size (host memory for the emulator build) ------------
def held(lib, arr, misalign=0):
    """-> (guarded buffer of exactly the array's bytes (+ misalign in front), pointer to the array)"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = hipmem.guarded_for(lib).from_numpy(np.concatenate([np.zeros(misalign, np.uint8), raw]) if misalign else raw)
    assert buf.ptr.value % 16 == 0
    return buf, C.c_void_p(buf.ptr.value + misalign)


def device_spectra(lib, hdr, rows, cands, coh, misalign=0):
    """frbch_burstspec_device -> (sums, spec, noise, used, kernel_used); kernel_used is held to frbch_burstspec_kernel"""
    n, nifs, nchan = cands.size, rows.shape[1], hdr["nchans"]
    buf, ptr = held(lib, rows, misalign)
    d_sums = hipmem.guarded_for(lib)(n * nifs * nchan * post.BURST_SUMS.itemsize)
    spec, noise = np.zeros((n, nifs, nchan), np.float32), np.zeros((n, nifs, nchan), np.float32)
    used = np.zeros((n, nchan), np.uint8)
    par, desc = rc.burst_par(coh), rc.desc_of(hdr, rows)
    query = lib.frbch_burstspec_kernel(C.byref(desc), ptr, rows.shape[0], C.byref(par), cands.ctypes.data, n)
    k = C.c_uint32(99)
    err = C.create_string_buffer(512)
    try:
        with bg.guarded():
            code = lib.frbch_burstspec_device(C.byref(desc), ptr, rows.shape[0], C.byref(par), cands.ctypes.data, n, None, 0, d_sums.ptr,
                                              spec.ctypes.data, noise.ctypes.data, used.ctypes.data, C.byref(k), err, len(err))
        assert code == 0, err.value
        buf.check(contents=True)
        d_sums.check()
        sums = d_sums.to_numpy(np.uint8).view(post.BURST_SUMS).reshape(n, nifs, nchan).copy()
    finally:
        buf.free()
        d_sums.free()
    assert k.value == query
    return sums, spec, noise, used, k.value


def check_burst_case(lib, name, misaligns=(0, 4)):
    """the conditions, then the library at every address against the restatement, byte for byte"""
    burst_conditions(name)
    hdr, rows, cands, coh = burst_case(name)
    want = burst_want(name)
    ran = []
    for misalign in misaligns:
        got = device_spectra(lib, hdr, rows, cands, coh, misalign)
        assert got[4] == spectra_kernel_expected(lib, hdr, rows, misalign), (name, misalign)
        for a, b, what in zip(got[:4], want, ("sums", "spec", "noise", "used")):
            if a.tobytes() != b.tobytes():
                raise AssertionError("%s, %d bytes off the aligned address: %s differ%s" % (name, misalign, what, _first_sums(a, b) if what == "sums" else ""))
        ran.append(got[4])
    return ran


def _first_sums(got, want):
    for f in post.BURST_SUMS.names:
        bad = np.argwhere(got[f] != want[f])
        if bad.size:
            i = tuple(int(v) for v in bad[0])
            return " in %d records; the first: %s of (candidate, product, channel) %s is %r, expected %r" % (len(bad), f, i, got[f][i], want[f][i])
    return ""


# ---- profile cases ---------------------------------------------------------------------------------------------------
def _prof(hdr, rows, cands, nbin, tfactor, rm, coh=False, flag=None, ref="mean"):
    return dict(hdr=hdr, rows=rows, cands=cands, coh=coh, nbin=nbin, tfactor=tfactor, ref=ref, rm=np.array(rm, dtype=np.float64), gain=None, flag=flag)


def _prof_64(dm, nbin, tfactor, seed):
    hdr = dict(rc.make_hdr(64), nbits=8)
    burst = dict(rc.B1, dm=dm)
    return _prof(hdr, rc.burst_file(hdr, 4096, 8, [burst], seed=seed), rc.cands_of([burst]), nbin, tfactor, (900.0,))


def _ascending_fast_u8():
    hdr = dict(rc.make_hdr(64, foff_sign=1), nbits=8)
    return _prof(hdr, rc.burst_file(hdr, 4096, 8, [rc.B1], seed=21), rc.cands_of([rc.B1]), 33, 3, (900.0,), ref="zero")


def _ascending_fast_u16_1024():
    hdr = dict(rc.make_hdr(1024, foff_sign=1), nbits=16)
    burst = dict(rc.B_LATE, sample=500)
    return _prof(hdr, rc.burst_file(hdr, 4096, 16, [burst], coherency=True, seed=22), rc.cands_of([burst], 16, 300), 256, 1, (100.0,), coh=True)


def _mixed_dm():
    hdr = dict(rc.make_hdr(64), nbits=8)
    bursts = [dict(rc.B1, dm=0.0, sample=800), rc.B1, dict(rc.B2, dm=171.1)]
    return _prof(hdr, rc.burst_file(hdr, 4096, 8, bursts, seed=23), rc.cands_of(bursts), 256, 1, (900.0, 900.0, -2500.0))


def _dead_tile():
    hdr = dict(rc.make_hdr(1024), nbits=8)
    flag = np.zeros(1024, np.uint8)
    flag[3 * 64: 4 * 64] = 1                               # all of tile 3
    flag[7 * 64: 8 * 64] = 1                               # and all but one channel of tile 7
    flag[7 * 64 + 22] = 0
    return _prof(hdr, rc.burst_file(hdr, 4096, 8, [rc.B1], seed=24), rc.cands_of([rc.B1], 16, 300), 33, 3, (900.0,), flag=flag)


def _far_away():
    hdr = dict(rc.make_hdr(64), nbits=8)
    cands = post.burst_cands([(DM, 1 << 62, 6), (rc.B1["dm"], rc.B1["sample"], rc.B1["width"]), (DM, -(1 << 62), 6)], 16, 200)
    return _prof(hdr, rc.burst_file(hdr, 4096, 8, [rc.B1], seed=25), cands, 33, 3, (900.0, 900.0, 900.0))


def partials_cap(ncand):
    """16384 channels x 16 bit, nbin 1024, DM 0, `ncand` identical candidates: for the plan query alone (the rows hold no byte)"""
    hdr = dict(rc.make_hdr(16384, bw=256.0), nbits=16)
    cands = np.repeat(post.burst_cands([(0.0, 2000, 6)], 16, 200), ncand)
    return _prof(hdr, np.empty((4096, 4, 0), np.uint16), cands, 1024, 1, np.zeros(ncand))


# name -> (builder, the profile kernel at the aligned address, brun (fast only), the largest tile spread of any candidate)
PROF_CASES = {
    "spread_255_t1": (lambda: _prof_64(171.1, 9, 1, 11), FAST, 1, 255),
    "spread_256_t1": (lambda: _prof_64(171.8, 9, 1, 12), GENERIC, None, 256),
    "spread_255_t2": (lambda: _prof_64(171.1, 9, 2, 13), GENERIC, None, 255),
    "t256_dm0": (lambda: _prof_64(0.0, 3, 256, 14), FAST, 1, 0),
    "t257_dm0": (lambda: _prof_64(0.0, 3, 257, 15), GENERIC, None, 0),
    "ascending_fast_u8": (_ascending_fast_u8, FAST, 33, 84),
    "ascending_fast_u16_1024": (_ascending_fast_u16_1024, FAST, 156, 100),
    "mixed_dm": (_mixed_dm, FAST, 1, 255),
    "dead_tile": (_dead_tile, FAST, 33, 6),
    "far_away": (_far_away, FAST, 33, 84),
}


@functools.lru_cache(maxsize=None)
def prof_case(name):
    c = PROF_CASES[name][0]()
    for a in (c["rows"], c["cands"], c["rm"], c["flag"]):
        if a is not None:
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def prof_want(name):
    out = ppo.profile(*pc.oracle_args(prof_case(name)))
    for a in out.values():
        a.setflags(write=False)
    return out


def plan(c, misalign=0):
    """the plan rule of the fast build, restated -> (kernel, brun or None, the largest tile spread of any candidate): the layout of
    the fast burst-sums kernel, tfactor + spread <= 256 rows, partials of at most 2^30 bytes; brun = the bins of a run that fit
    behind the spread, at most nbin, the same for every candidate"""
    item = c["rows"].dtype.itemsize
    nchan, ncand = c["hdr"]["nchans"], c["cands"].size
    spread = max(int(tile_spreads(c["hdr"], 8 * item, dm).max(initial=0)) for dm in sorted(set(c["cands"]["dm"].tolist())))
    if (nchan * item) % 64 != 0 or misalign % 16 != 0:
        return GENERIC, None, spread
    if c["tfactor"] + spread > SPAN or ncand * (nchan * item // 64) * c["nbin"] * 36 > PART_CAP:
        return GENERIC, None, spread
    return FAST, min(c["nbin"], (SPAN - spread) // c["tfactor"]), spread


def prof_conditions(name):
    """what the case is there for, on the restatements alone"""
    c, (_b, kernel, brun, spread) = prof_case(name), PROF_CASES[name]
    assert plan(c) == (kernel, brun, spread), (name, plan(c))
    assert plan(c, 4) == (GENERIC, None, spread)
    w = prof_want(name)
    if name == "spread_255_t1":                            # a run of one bin fills the stage: 1 + 255 rows
        assert brun * c["tfactor"] + spread == SPAN and c["nbin"] == 9 and (w["hits"] == 64).all()
    elif name == "t256_dm0":
        assert brun * c["tfactor"] + spread == SPAN and (w["hits"] == 64 * 256).all()
    elif name.startswith("ascending"):
        d = ro.delays(c["hdr"], float(c["cands"][0]["dm"]))
        assert c["hdr"]["foff"] > 0 and (np.diff(d) <= 0).all() and d[0] > 0
        if name == "ascending_fast_u16_1024":
            s = tile_spreads(c["hdr"], 16, float(c["cands"][0]["dm"]))
            assert s.size == 32 and (int(s.min()), int(s.max())) == (93, 100) and c["coh"] and brun < c["nbin"]      # two runs of bins
            assert w["results"]["nused"][0] == 1024 and w["hits"].min() > 0
    elif name == "mixed_dm":
        spreads = [int(tile_spreads(c["hdr"], 8, float(cd["dm"])).max()) for cd in c["cands"]]
        assert spreads == [0, 84, 255] and brun == 1
        assert plan(dict(c, cands=c["cands"][:1]))[1] == 256 and plan(dict(c, cands=c["cands"][:2]))[1] == 172      # alone, and without the third
        assert w["results"]["nused"].tolist() == [64, 64, 64] and (w["hits"] == 64).all()
    elif name == "dead_tile":
        assert not w["used"][0, 192:256].any() and w["used"][0, 448:512].sum() == 1 and w["results"]["nused"][0] == 1024 - 127
    elif name == "far_away":
        assert c["cands"]["sample"].tolist() == [1 << 62, 1500, -(1 << 62)]
        assert w["results"]["nused"].tolist() == [0, 64, 0] and not w["used"][[0, 2]].any()
        for f in ("acc", "hits", "bins"):
            assert not w[f][[0, 2]].view(np.uint8).any() and w[f][1].view(np.uint8).any()
        assert not any(w["results"][f][[0, 2]].any() for f in ("sigma_i", "sigma_q", "sigma_u", "sigma_v", "sigma_l", "lref", "k"))


def profile_on(lib, c, misalign=0):
    """frbch_polprof_device on the case's rows in a guarded buffer -> (outputs, kernel_used, the plan query's answer)"""
    buf, ptr = held(lib, c["rows"], misalign)
    try:
        want_kernel = pc.query(lib, c, ptr)
        with bg.guarded():
            code, msg, out, k = pc.call(lib.frbch_polprof_device, c, ptr, out=pc.outputs(c["cands"].size, c["nbin"], c["hdr"]["nchans"], fill=0xA5))
        assert code == 0, msg
        buf.check(contents=True)
    finally:
        buf.free()
    return out, k, want_kernel


def check_prof_case(lib, name):
    """the conditions, then the library at the aligned address and 4 bytes off it against the restatement"""
    prof_conditions(name)
    c, want = prof_case(name), prof_want(name)
    emulated = hipmem.guarded_for(lib) is hipmem.HostGuardedBuffer
    ran = []
    for misalign in (0, 4):
        out, k, q = profile_on(lib, c, misalign)
        exp = GENERIC if emulated else plan(c, misalign)[0]
        assert k[1] == q == exp and k[0] == spectra_kernel_expected(lib, c["hdr"], c["rows"], misalign), (name, misalign, k, q, exp)
        assert pc.same(out, want), (name, misalign)
        ran.append(k[1])
    return ran
