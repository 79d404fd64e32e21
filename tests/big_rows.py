"""Rows past the 2^31 and the 2^32 mark that cost nothing to describe (tests/test_gpu_beyond_4gib.py on the device at the
real marks, tests/test_big_rows.py on the emulator at marks of 2^20 / 2^21 bytes).  A plain module, like tests/post_cases.py.

The buffer holds row(t) = base[t % P] for t < nrows: `base` is P rows of seeded random codes [P][nifs][nchan], P a prime, so
that the row at every mark and row 0 are DIFFERENT rows of the base -- an offset that wraps at a mark reads or writes other
codes, and the comparison sees it.  The host never holds the whole array: window(t0, n) rebuilds any run of rows from the
base, the device buffer is filled by one upload of the base and device-to-device copies of whole replicas.

Expected values are the existing restatements (oracle/post_oracle.py, tests/rfi_oracle.py, tests/rfi_periodic_oracle.py,
tests/cutout_oracle.py, tests/fold_model_oracle.py) applied to windows; the three that are restated here for windows -- the
dedispersed series from per-channel prefix sums, the clip from the row sums of the base, the fold from a count matrix --
are held equal to those restatements on the WHOLE small array by tests/test_big_rows.py.  Everything is integer: every
comparison is `==`."""
import contextlib
import ctypes as C
import faulthandler

import numpy as np

from frb_baseband_amd import _lib, post
from oracle import post_oracle as po
from tests import cutout_oracle as co
from tests import fold_model_oracle as fo
from tests import hipmem
from tests import rfi_oracle as ro
from tests import rfi_periodic_oracle as rpo

LO, HI = 1 << 31, 1 << 32
CALL_LIMIT_S = 120          # a device call that has not come back by then ends the test process (traceback on stderr)
FAST, GENERIC = 1, 0
DTYPES = {8: np.uint8, 16: np.uint16}
TSTART = 59000.25

# the spliced files of BASELINE configs[2] and configs[3]: (nchan, nifs, nbits, tsamp of the dedispersion cases)
SHAPES = {"A8": (8192, 4, 8, 64e-6), "A16": (8192, 2, 16, 64e-6), "B8": (65536, 1, 8, 100e-6)}
P_REAL, TAIL_REAL = 3001, 128 << 20
# the same builders on the emulator: 4 KiB rows, marks at rows 256 and 512
SMALL = {"A8": (1024, 4, 8, 1e-3), "A16": (1024, 2, 16, 1e-3), "B8": (4096, 1, 8, 1e-3)}
P_SMALL, TAIL_SMALL, MARKS_SMALL = 101, 1 << 20, (1 << 20, 1 << 21)


@contextlib.contextmanager
def guarded():
    faulthandler.dump_traceback_later(CALL_LIMIT_S, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


# ---- memory: the device through the HIP runtime, the emulator's host pointers through memmove ------------------------
class DeviceMem:
    Buffer = hipmem.GuardedBuffer

    @staticmethod
    def put(dst, arr):
        arr = np.ascontiguousarray(arr)
        assert hipmem.hip().hipMemcpy(C.c_void_p(dst), arr.ctypes.data, arr.nbytes, 1) == 0

    @staticmethod
    def get(src, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        hipmem.hip().hipDeviceSynchronize()
        assert hipmem.hip().hipMemcpy(out.ctypes.data, C.c_void_p(src), nbytes, 2) == 0
        return out

    @staticmethod
    def copy(dst, src, nbytes):
        assert hipmem.hip().hipMemcpy(C.c_void_p(dst), C.c_void_p(src), nbytes, 3) == 0     # device to device


class HostMem:
    Buffer = hipmem.HostGuardedBuffer

    @staticmethod
    def put(dst, arr):
        arr = np.ascontiguousarray(arr)
        C.memmove(dst, arr.ctypes.data, arr.nbytes)

    @staticmethod
    def get(src, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        C.memmove(out.ctypes.data, src, nbytes)
        return out

    @staticmethod
    def copy(dst, src, nbytes):
        C.memmove(dst, src, nbytes)


def mem_for(lib):
    return HostMem if hipmem.guarded_for(lib) is hipmem.HostGuardedBuffer else DeviceMem


# ---- the description ------------------------------------------------------------------------------------------------------
def make_base(P, nifs, nchan, nbits, seed):
    """P rows [P][nifs][nchan]: per product its own seed, floor and width as post_cases.make_rows (codes <= 222, x 201 for
    16 bit), and 1 + p // 2 broadband rows of + 50 at base rows of its own (what `-clip` flags: one or two rows in P stay
    beyond 5 sigma of a scatter they dominate, for P = 101 as well)"""
    x = np.empty((P, nifs, nchan), dtype=np.uint16)
    for p in range(nifs):
        rng = np.random.default_rng(1000 * seed + p)
        x[:, p, :] = rng.integers(40 + 15 * p, 40 + 15 * p + 24 + 8 * p, size=(P, nchan), dtype=np.uint16)
        r0 = int(P * (0.29 + 0.13 * p))
        x[r0: r0 + 1 + p // 2, p, :] += 50
    assert x.max() <= 222
    return x.astype(np.uint8) if nbits == 8 else x * np.uint16(201)


class BigRows:
    """row(t) = base[t % P], t < nrows; nrows is the smallest count whose bytes reach marks[-1] + tail_bytes, plus 37 (a
    ragged last block and last time tile).  `marks` are counted in bytes, in elements and in t * nchan: mark_rows holds every
    row index at which one of them falls inside the buffer, and none of them is a multiple of P."""

    def __init__(self, nchan, nifs, nbits, tsamp, P=P_REAL, marks=(LO, HI), tail_bytes=TAIL_REAL, seed=7):
        self.nchan, self.nifs, self.nbits, self.tsamp, self.P, self.marks = nchan, nifs, nbits, tsamp, P, tuple(marks)
        self.dtype = np.dtype(DTYPES[nbits])
        self.row_elems = nifs * nchan
        self.row_bytes = self.row_elems * self.dtype.itemsize
        self.nrows = -(-(self.marks[-1] + tail_bytes) // self.row_bytes) + 37
        self.nbytes = self.nrows * self.row_bytes
        self.base = make_base(P, nifs, nchan, nbits, seed)
        self.base.setflags(write=False)
        per_row = {self.row_bytes, self.row_elems, nchan}          # bytes, elements, t * nchan
        self.mark_rows = sorted({m // u for m in self.marks for u in per_row if m % u == 0 and 0 < m // u < self.nrows})
        self.byte_mark_rows = [m // self.row_bytes for m in self.marks]
        self.check_aliasing()

    def check_aliasing(self):
        """the row at every mark and row 0 are different rows of the base, and differ in every product"""
        assert all(m * self.row_bytes < self.nbytes for m in self.byte_mark_rows), "the buffer ends before a byte mark"
        assert set(self.byte_mark_rows) <= set(self.mark_rows)
        for m in self.mark_rows:
            assert m % self.P != 0, "row %d at a mark is row 0 of the base again (P = %d)" % (m, self.P)
            for p in range(self.nifs):
                assert not np.array_equal(self.base[m % self.P, p], self.base[0, p])

    def hdr(self, tsamp=None):
        """a 256 MHz band below 1416 MHz, foff < 0"""
        step = 256.0 / self.nchan
        return dict(nchans=self.nchan, nifs=self.nifs, nbits=self.nbits, fch1=1416.0 - 0.5 * step, foff=-step,
                    tsamp=self.tsamp if tsamp is None else tsamp, tstart=TSTART, source_name="J0000+00", src_raj=12345.6, src_dej=-123456.7)

    def desc(self, prod=0, tsamp=None):
        return post.fil_desc(self.hdr(tsamp), product=prod)

    def window(self, t0, n):
        """rows [t0, t0 + n) as the buffer holds them after a fill, a fresh array"""
        assert 0 <= t0 and t0 + n <= self.nrows
        return self.base[np.arange(t0, t0 + n) % self.P]

    def row_sums(self, prod):
        """the zero-DM sum of every row of the buffer, float64 [nrows] (exact)"""
        s = self.base[:, prod, :].sum(axis=1, dtype=np.int64).astype(np.float64)
        return s[np.arange(self.nrows) % self.P]

    def runs(self, reach, n):
        """(first index, n) of the runs of outputs that are compared: the first n, n whose `reach` input rows straddle each byte
        mark, and (by the caller, which knows nout) the last n"""
        out = [(0, n)]
        for m in self.byte_mark_rows:
            t0 = m - reach // 2 - n // 2
            assert t0 > 0 and t0 < m < t0 + reach, "the inputs of this run do not straddle row %d" % m
            out.append((t0, n))
        return out

    def blocks(self, block_rows):
        """the blocks that are compared: 0 and 1, the two on either side of (or the one across) each byte mark, the last three"""
        nblk = -(-self.nrows // block_rows)
        out = {0, 1, nblk - 3, nblk - 2, nblk - 1}
        for m in self.byte_mark_rows:
            out |= {(m - 1) // block_rows, m // block_rows}
        return sorted(out)


def big(name):
    return BigRows(*SHAPES[name])


def small(name):
    return BigRows(*SMALL[name], P=P_SMALL, marks=MARKS_SMALL, tail_bytes=TAIL_SMALL)


# ---- the buffer -------------------------------------------------------------------------------------------------------------
class Resident:
    """the rows of a BigRows in a guarded buffer of nbytes + 16, laid `shift` bytes behind its first byte"""

    def __init__(self, br, mem):
        self.br, self.mem = br, mem
        self.buf = mem.Buffer(br.nbytes + 16, poison=False)
        assert self.buf.ptr.value % 16 == 0
        self.shift = None
        self.patches = []                       # [(first row, rows)]: what poke() wrote since the last lay()

    def lay(self, shift=0):
        """upload the base at `shift`, then whole replicas to consecutive offsets, the last one partial"""
        br = self.br
        assert 0 <= shift <= 16 and shift % br.dtype.itemsize == 0
        self.shift, self.patches = shift, []
        rep = br.P * br.row_bytes
        self.mem.put(self.address, br.base)
        at = rep
        while at < br.nbytes:
            n = min(rep, br.nbytes - at)
            self.mem.copy(self.address + at, self.address, n)
            at += n
        return self

    @property
    def address(self):
        return self.buf.ptr.value + self.shift

    def read(self, t0, n):
        br = self.br
        assert 0 <= t0 and t0 + n <= br.nrows
        raw = self.mem.get(self.address + t0 * br.row_bytes, n * br.row_bytes)
        return raw.view(br.dtype).reshape(n, br.nifs, br.nchan)

    def poke(self, t0, rows):
        rows = np.ascontiguousarray(rows, dtype=self.br.dtype)
        assert 0 <= t0 and t0 + rows.shape[0] <= self.br.nrows and rows.shape[1:] == (self.br.nifs, self.br.nchan)
        self.mem.put(self.address + t0 * self.br.row_bytes, rows)
        self.patches.append((t0, rows.copy()))

    def poke_cell(self, t0, t1, prod, chan, value):
        """rows [t0, t1) of one product and channel become `value`"""
        rows = self.window(t0, t1 - t0)
        rows[:, prod, chan] = value
        self.poke(t0, rows)

    def window(self, t0, n):
        """what the buffer holds in rows [t0, t0 + n) if nothing but lay() and poke() wrote it"""
        rows = self.br.window(t0, n)
        for p0, pr in self.patches:
            a, b = max(t0, p0), min(t0 + n, p0 + pr.shape[0])
            if a < b:
                rows[a - t0: b - t0] = pr[a - p0: b - p0]
        return rows

    def check_equals(self, expected=()):
        """every replica against the base, chunk by chunk (no checksum of 4 GB): `expected` [(first row, rows)] says what the
        buffer must hold elsewhere than the base's rows; the patches of poke() count as well"""
        br = self.br
        over = list(self.patches) + list(expected)
        for r0 in range(0, br.nrows, br.P):
            n = min(br.P, br.nrows - r0)
            want = br.base[:n]
            if any(p0 < r0 + n and r0 < p0 + pr.shape[0] for p0, pr in over):
                want = np.array(want)
                for p0, pr in over:
                    a, b = max(r0, p0), min(r0 + n, p0 + pr.shape[0])
                    if a < b:
                        want[a - r0: b - r0] = pr[a - p0: b - p0]
            got = self.read(r0, n)
            if not np.array_equal(got, want):
                bad = np.flatnonzero((got != want).reshape(n, -1).any(axis=1))
                raise AssertionError("rows %d .. %d of the buffer are not what they should be (%d rows of replica %d)"
                                     % (r0 + int(bad[0]), r0 + int(bad[-1]), bad.size, r0 // br.P))
        self.buf.check()

    def free(self):
        self.buf.free()


def out_buffer(mem, nbytes):
    return mem.Buffer(nbytes)


# ---- dedispersion -----------------------------------------------------------------------------------------------------------
# 9 DMs, one whole group and one partial: largest delays of 1000 to 3000 rows at the real sampling times (a hundred rows at
# the emulator's)
DMS = [100.0 + i for i in range(9)]


def delays_of(br, dms, tsamp=None):
    h = br.hdr(tsamp)
    return [po.delays_samples(h["fch1"], h["foff"], br.nchan, h["tsamp"], dm) for dm in dms]


def clip_of(br, prod, clip):
    """the clip of the WHOLE buffer from the row sums of the base -> (flag [nrows] bool, repl [nchan] or None, nclip):
    po.clip_flags on the row sums, the replacement values from how often every base row stays unclipped"""
    if not clip > 0:
        return None, None, 0
    flag = po.clip_flags(br.row_sums(prod), clip)
    nclip = int(flag.sum())
    if not 0 < nclip < br.nrows:
        return None, None, 0
    good = np.bincount(np.arange(br.nrows)[~flag] % br.P, minlength=br.P).astype(np.int64)
    colsum = good @ br.base[:, prod, :].astype(np.int64)                           # exact
    repl = po.clip_replacement(colsum.astype(np.float64), float(br.nrows - nclip), True)
    return flag, repl, nclip


def prefix_sums(x):
    """cum[r][c] = sum of x[r][:c]: [rows][nchan + 1], int32 where the largest row sum fits"""
    nchan = x.shape[1]
    wide = np.int64 if int(np.iinfo(x.dtype).max) * nchan >= 1 << 31 else np.int32
    cum = np.zeros((x.shape[0], nchan + 1), dtype=wide)
    np.cumsum(x, axis=1, dtype=wide, out=cum[:, 1:])
    return cum


def window_series(cum, d, n, zerodm):
    """sum_c x[t + d[c]][c] for t < n, minus the mean over channels of the row sums at the same rows with zerodm, as float32 --
    po.sum_delayed through the prefix sums `cum` of x over channels: every run of channels that share a delay is one
    difference of two of them (exact integers).  x: at least n + d.max() rows of one product after the clip."""
    nchan = cum.shape[1] - 1
    assert cum.shape[0] >= n + int(d.max()) and int(d.min()) >= 0
    cuts = np.concatenate(([0], np.flatnonzero(np.diff(d)) + 1, [nchan]))           # runs of channels with one delay
    c0, c1 = cuts[:-1], cuts[1:]
    rows = np.arange(n)[:, None] + d[c0][None, :]
    a = (cum[rows, c1[None, :]] - cum[rows, c0[None, :]]).sum(axis=1, dtype=np.int64).astype(np.float64)
    if not zerodm:
        return a.astype(np.float32)
    b = (cum[:, -1].astype(np.int64)[rows] * (c1 - c0)[None, :]).sum(axis=1, dtype=np.int64).astype(np.float64)
    return (a - b / nchan).astype(np.float32)


def want_dedisp(br, prod, dms, clip, ncmp, tsamp=None):
    """-> (nout, nclip, {zerodm: [(t0, series [ndm][n])]}) for the compared runs of outputs: the first ncmp, ncmp whose input
    rows straddle each byte mark, the last ncmp"""
    dl = delays_of(br, dms, tsamp)
    maxd = max(int(d.max()) for d in dl)
    nout = br.nrows - maxd
    flag, repl, nclip = clip_of(br, prod, clip)
    out = {True: [], False: []}
    for t0, n in br.runs(maxd, ncmp) + [(nout - ncmp, ncmp)]:
        x = br.window(t0, n + maxd)[:, prod, :]
        if flag is not None:
            x[flag[t0: t0 + n + maxd]] = repl.astype(x.dtype)
        cum = prefix_sums(x)
        for zerodm in (True, False):
            out[zerodm].append((t0, np.stack([window_series(cum, d, n, zerodm) for d in dl])))
    return nout, nclip, out


def dedisp_device(lib, res, prod, dms, zerodm, clip, nout, tsamp=None):
    """frbch_dedisperse_device on the resident rows -> (the output buffer [ndm][nout] float32, nclip, frbch_dedisperse_kernel)"""
    br = res.br
    desc = br.desc(prod, tsamp)
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    assert lib.frbch_dedisperse_nout(C.byref(desc), br.nrows, dm_arr.ctypes.data, dm_arr.size) == nout
    kernel = lib.frbch_dedisperse_kernel(C.byref(desc), C.c_void_p(res.address), br.nrows, dm_arr.ctypes.data, dm_arr.size)
    d_out = out_buffer(res.mem, dm_arr.size * nout * 4)
    nclip = C.c_uint64(0)
    err = C.create_string_buffer(512)
    with guarded():
        rc = lib.frbch_dedisperse_device(C.byref(desc), C.c_void_p(res.address), br.nrows, dm_arr.ctypes.data, dm_arr.size,
                                         1 if zerodm else 0, float(clip), 0, d_out.ptr, nout, C.byref(nclip), err, len(err))
    assert rc == 0, err.value
    return d_out, nclip.value, kernel


def read_series(mem, d_out, nout, i, t0, n):
    """series[i][t0 : t0 + n] of an output buffer [ndm][nout] float32"""
    return mem.get(d_out.ptr.value + (i * nout + t0) * 4, n * 4).view(np.float32)


def check_dedisp(lib, res, prod, dms, zerodm, clip, kernel, want, tsamp=None):
    """`want`: want_dedisp(br, prod, dms, clip, ...) -- computed once per shape and clip, shared by the cases"""
    nout, wclip, runs = want
    assert clip == 0 or wclip >= (1 + prod // 2) * (res.br.nrows // res.br.P)    # the broadband rows of this product, in every replica
    d_out, nclip, k = dedisp_device(lib, res, prod, dms, zerodm, clip, nout, tsamp)
    try:
        assert k == kernel
        assert nclip == wclip
        for t0, series in runs[bool(zerodm)]:
            for i in range(len(dms)):
                got = read_series(res.mem, d_out, nout, i, t0, series.shape[1])
                assert np.array_equal(got, series[i]), "DM %d, outputs %d .. %d" % (i, t0, t0 + series.shape[1])
    finally:
        d_out.free()


# ---- interference -----------------------------------------------------------------------------------------------------------
def rfi_par(block_rows):
    return post.rfi_params(dict(post.RFI_DEFAULTS, block_rows=block_rows))


def block_window(res, b, block_rows):
    """(first row, the rows of block b as the buffer should hold them)"""
    r0 = b * block_rows
    return r0, res.window(r0, min(block_rows, res.br.nrows - r0))


def poke_four_cells(res, prod, block_rows):
    """four cells become constants: one below the first mark, one across the row of the last mark, one in the last whole
    block, one in the ragged block -> [(t0, t1, channel, value)]"""
    br = res.br
    lo, hi = br.byte_mark_rows[0], br.byte_mark_rows[-1]
    nblk = -(-br.nrows // block_rows)
    assert br.nrows % block_rows != 0
    cells = [(lo - block_rows, lo, 5, 77), (hi - block_rows // 2, hi + block_rows // 2, br.nchan // 2 + 1, 91),
             ((nblk - 2) * block_rows, (nblk - 1) * block_rows, br.nchan - 2, 33), ((nblk - 1) * block_rows, br.nrows, 64, 120)]
    for t0, t1, c, v in cells:
        res.poke_cell(t0, t1, prod, c, v * (201 if br.nbits == 16 else 1))
    return cells


def rfi_stats_device(lib, res, prod, par):
    """-> (buffer [nblk][nchan][2] uint64, kernel_used, frbch_rfi_stats_kernel)"""
    br = res.br
    nblk = lib.frbch_rfi_nblk(br.nrows, par.block_rows)
    d_stats = out_buffer(res.mem, nblk * br.nchan * 16)
    used = C.c_uint32(99)
    err = C.create_string_buffer(512)
    desc = br.desc(prod)
    query = lib.frbch_rfi_stats_kernel(C.byref(desc), C.c_void_p(res.address), br.nrows, C.byref(par))
    with guarded():
        rc = lib.frbch_rfi_stats_device(C.byref(desc), C.c_void_p(res.address), br.nrows, C.byref(par), 0, d_stats.ptr, C.byref(used), err,
                                        len(err))
    assert rc == 0, err.value
    return d_stats, used.value, query


def rfi_peaks_device(lib, res, prod, par, d_stats):
    br = res.br
    nblk = lib.frbch_rfi_nblk(br.nrows, par.block_rows)
    d_peaks = out_buffer(res.mem, nblk * br.nchan * 8)
    used = C.c_uint32(99)
    err = C.create_string_buffer(512)
    desc = br.desc(prod)
    query = lib.frbch_rfi_peaks_kernel(C.byref(desc), C.c_void_p(res.address), br.nrows, C.byref(par))
    with guarded():
        rc = lib.frbch_rfi_peaks_device(C.byref(desc), C.c_void_p(res.address), br.nrows, C.byref(par), 0, d_stats.ptr, d_peaks.ptr,
                                        C.byref(used), err, len(err))
    assert rc == 0, err.value
    return d_peaks, used.value, query


def peak_channels(nchan):
    """the channels whose peaks are compared: four runs of 64 (whole pairs) spread over the band -- the transform of a block
    of every channel in numpy takes seconds"""
    if nchan <= 1024:
        return np.arange(nchan)
    starts = [0, (nchan // 3) & ~63, (2 * nchan // 3) & ~63, nchan - 64]
    return np.concatenate([np.arange(s, s + 64) for s in starts])


def check_stats_and_peaks(lib, res, prod, block_rows, kernel, peaks_kernel):
    """frbch_rfi_stats_device and frbch_rfi_peaks_device on the rows as they lie (the caller poked its cells), block by block
    against ro.stats / rpo.peaks on the windows"""
    br = res.br
    par = rfi_par(block_rows)
    d_stats, used, query = rfi_stats_device(lib, res, prod, par)
    d_peaks, pused, pquery = rfi_peaks_device(lib, res, prod, par, d_stats)
    try:
        assert used == query == kernel and pused == pquery == peaks_kernel
        chans = peak_channels(br.nchan)
        for b in br.blocks(block_rows):
            _r0, rows = block_window(res, b, block_rows)
            x = rows[:, prod, :]
            st = ro.stats(x, block_rows)
            got = res.mem.get(d_stats.ptr.value + b * br.nchan * 16, br.nchan * 16).view(np.uint64).reshape(1, br.nchan, 2)
            assert np.array_equal(got, st), "statistics of block %d" % b
            pk = rpo.peaks(x[:, chans], st[:, chans], block_rows)
            gp = res.mem.get(d_peaks.ptr.value + b * br.nchan * 8, br.nchan * 8).view(rpo.PEAK).reshape(1, br.nchan)
            assert gp[:, chans].tobytes() == pk.tobytes(), "peaks of block %d" % b
    finally:
        d_stats.free()
        d_peaks.free()


def chosen_mask(br, block_rows, seed=5):
    """a mask and replacement values of the test's own: in every compared block 40 random channels, and channel 3 everywhere
    in the blocks across the marks"""
    nblk = -(-br.nrows // block_rows)
    rng = np.random.default_rng(seed)
    m = np.zeros((nblk, br.nchan), dtype=np.uint8)
    for b in br.blocks(block_rows):
        m[b, rng.choice(br.nchan, 40, replace=False)] = 1
    top = 222 * (201 if br.nbits == 16 else 1)
    repl = rng.integers(0, top, size=br.nchan).astype(np.float64)
    return m, repl


def rfi_apply_device(lib, res, prod, par, m, repl):
    mem = res.mem
    d_m, d_r = mem.Buffer(m.nbytes, poison=False), mem.Buffer(repl.nbytes, poison=False)
    mem.put(d_m.ptr.value, m)
    mem.put(d_r.ptr.value, repl)
    err = C.create_string_buffer(512)
    with guarded():
        rc = lib.frbch_rfi_apply_device(C.byref(res.br.desc(prod)), C.c_void_p(res.address), res.br.nrows, C.byref(par), d_m.ptr, d_r.ptr,
                                        0, err, len(err))
    d_m.free()
    d_r.free()
    assert rc == 0, err.value


def check_apply(lib, res, prod, block_rows):
    """frbch_rfi_apply_device with chosen_mask: the compared blocks against ro.apply on their windows, and every replica
    outside them still the base"""
    br = res.br
    par = rfi_par(block_rows)
    m, repl = chosen_mask(br, block_rows)
    expected = []
    for b in br.blocks(block_rows):
        r0, rows = block_window(res, b, block_rows)
        expected.append((r0, ro.apply(rows, prod, block_rows, m[b:b + 1], repl)))
        assert not np.array_equal(expected[-1][1], rows)
    rfi_apply_device(lib, res, prod, par, m, repl)
    res.check_equals(expected)


def mask_of_stats(lib, br, prod, par, st, prior=None):
    """frbch_rfi_mask on downloaded statistics -> dict(mask, repl, chan_flag, blk_flag)"""
    nblk = st.shape[0]
    m, repl = np.full((nblk, br.nchan), 9, np.uint8), np.full(br.nchan, -1.0)
    cf, bf = np.full(br.nchan, 9, np.uint8), np.full(nblk, 9, np.uint8)
    pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.uint8)
    err = C.create_string_buffer(512)
    rc = lib.frbch_rfi_mask(C.byref(br.desc(prod)), st.ctypes.data, nblk, br.nrows, C.byref(par), None, None if pr is None else pr.ctypes.data,
                            m.ctypes.data, repl.ctypes.data, cf.ctypes.data, bf.ctypes.data, err, len(err))
    assert rc == 0, err.value
    return dict(mask=m, repl=repl, chan_flag=cf, blk_flag=bf)


def same_mask(a, b):
    return (np.array_equal(a["mask"], b["mask"]) and a["repl"].tobytes() == b["repl"].tobytes() and np.array_equal(a["chan_flag"], b["chan_flag"])
            and np.array_equal(a["blk_flag"], b["blk_flag"]))


def read_blocks(res, block_rows):
    return [res.read(*_span(res.br, b, block_rows)) for b in res.br.blocks(block_rows)]


def _span(br, b, block_rows):
    r0 = b * block_rows
    return r0, min(block_rows, br.nrows - r0)


def host_arrays(br, nblk, nprod=1):
    m, repl = np.full((nblk, br.nchan), 9, np.uint8), np.full((nprod, br.nchan), -1.0)
    return m, repl, np.full(br.nchan, 9, np.uint8), np.full(nblk, 9, np.uint8)


def check_clean_is_its_parts(lib, res, prod, block_rows, shift, kernel):
    """frbch_rfi_clean_device = statistics, frbch_rfi_mask, apply through the library on the same buffer: the same mask, and
    the same rows in the compared blocks"""
    br = res.br
    par = rfi_par(block_rows)
    res.lay(shift)
    poke_four_cells(res, prod, block_rows)
    nblk = lib.frbch_rfi_nblk(br.nrows, block_rows)
    d_stats, used, _q = rfi_stats_device(lib, res, prod, par)
    st = res.mem.get(d_stats.ptr.value, nblk * br.nchan * 16).view(np.uint64).reshape(nblk, br.nchan, 2)
    d_stats.free()
    assert used == kernel
    parts = mask_of_stats(lib, br, prod, par, st)
    assert parts["mask"].any() and not parts["mask"].all()
    rfi_apply_device(lib, res, prod, par, parts["mask"], parts["repl"])
    rows_parts = read_blocks(res, block_rows)
    res.lay(shift)
    cells = poke_four_cells(res, prod, block_rows)
    m, repl, cf, bf = host_arrays(br, nblk)
    used = C.c_uint32(99)
    err = C.create_string_buffer(512)
    with guarded():
        rc = lib.frbch_rfi_clean_device(C.byref(br.desc(prod)), C.c_void_p(res.address), br.nrows, C.byref(par), None, 0, m.ctypes.data,
                                        repl.ctypes.data, cf.ctypes.data, bf.ctypes.data, C.byref(used), err, len(err))
    assert rc == 0, err.value
    assert used.value == kernel
    assert same_mask(dict(mask=m, repl=repl[0], chan_flag=cf, blk_flag=bf), parts)
    for t0, _t1, c, _v in cells:                      # a block that is constant has no scatter: flagged, where it lies
        assert t0 % block_rows != 0 or m[t0 // block_rows, c] == 1
    for a, b in zip(read_blocks(res, block_rows), rows_parts):
        assert np.array_equal(a, b)
    return parts


def check_cleanf_is_its_parts(lib, res, prod, block_rows, shift, kernels):
    """frbch_rfi_cleanf_device = statistics, peaks, frbch_rfi_periodic, frbch_rfi_mask with that prior, apply"""
    br = res.br
    par = rfi_par(block_rows)
    fpar = _lib.FrbchRfiFparams()
    fpar.size = C.sizeof(_lib.FrbchRfiFparams)
    fpar.t_pow, fpar.chan_frac = post.t_pow_of(4.0, block_rows), 0.3
    res.lay(shift)
    poke_four_cells(res, prod, block_rows)
    nblk = lib.frbch_rfi_nblk(br.nrows, block_rows)
    d_stats, used, _q = rfi_stats_device(lib, res, prod, par)
    d_peaks, pused, _q = rfi_peaks_device(lib, res, prod, par, d_stats)
    st = res.mem.get(d_stats.ptr.value, nblk * br.nchan * 16).view(np.uint64).reshape(nblk, br.nchan, 2)
    pk = res.mem.get(d_peaks.ptr.value, nblk * br.nchan * 8).view(rpo.PEAK).reshape(nblk, br.nchan)
    d_stats.free()
    d_peaks.free()
    assert (used, pused) == kernels
    pflag, pchan = np.full((nblk, br.nchan), 9, np.uint8), np.full(br.nchan, 9, np.uint8)
    err = C.create_string_buffer(512)
    rc = lib.frbch_rfi_periodic(C.byref(br.desc(prod)), st.ctypes.data, pk.ctypes.data, nblk, br.nrows, C.byref(par), C.byref(fpar),
                                pflag.ctypes.data, pchan.ctypes.data, None, err, len(err))
    assert rc == 0, err.value
    parts = mask_of_stats(lib, br, prod, par, st, prior=pflag)
    rfi_apply_device(lib, res, prod, par, parts["mask"], parts["repl"])
    rows_parts = read_blocks(res, block_rows)
    res.lay(shift)
    poke_four_cells(res, prod, block_rows)
    m, repl, cf, bf = host_arrays(br, nblk)
    gflag, gchan = np.full((nblk, br.nchan), 9, np.uint8), np.full(br.nchan, 9, np.uint8)
    gpk = np.full((nblk, br.nchan), 7, dtype=np.uint64).view(rpo.PEAK)
    used2 = (C.c_uint32 * 2)(99, 99)
    with guarded():
        rc = lib.frbch_rfi_cleanf_device(C.byref(br.desc(prod)), C.c_void_p(res.address), br.nrows, C.byref(par), C.byref(fpar), None, 0,
                                         m.ctypes.data, repl.ctypes.data, cf.ctypes.data, bf.ctypes.data, gflag.ctypes.data,
                                         gchan.ctypes.data, gpk.ctypes.data, used2, err, len(err))
    assert rc == 0, err.value
    assert (used2[0], used2[1]) == kernels
    assert np.array_equal(gflag, pflag) and np.array_equal(gchan, pchan) and gpk.tobytes() == pk.tobytes()
    want = dict(parts, chan_flag=parts["chan_flag"] | pchan)
    assert same_mask(dict(mask=m, repl=repl[0], chan_flag=cf, blk_flag=bf), want)
    for a, b in zip(read_blocks(res, block_rows), rows_parts):
        assert np.array_equal(a, b)


def check_cleanp_is_its_parts(lib, res, block_rows, shift, kernel):
    """frbch_rfi_cleanp_device = per product the statistics and the mask, the union as prior of a second frbch_rfi_mask per
    product, the union mask applied to every product with its own replacement values"""
    br = res.br
    par = rfi_par(block_rows)
    nblk = lib.frbch_rfi_nblk(br.nrows, block_rows)

    def lay():
        res.lay(shift)
        for p in range(br.nifs):
            poke_four_cells(res, p, block_rows)
    lay()
    stats, first = [], []
    for p in range(br.nifs):
        d_stats, used, _q = rfi_stats_device(lib, res, p, par)
        stats.append(res.mem.get(d_stats.ptr.value, nblk * br.nchan * 16).view(np.uint64).reshape(nblk, br.nchan, 2))
        d_stats.free()
        assert used == kernel
        first.append(mask_of_stats(lib, br, p, par, stats[-1]))
    union = np.bitwise_or.reduce([f["mask"] for f in first])
    cfu = np.bitwise_or.reduce([f["chan_flag"] for f in first])
    bfu = np.bitwise_or.reduce([f["blk_flag"] for f in first])
    repls = []
    for p in range(br.nifs):
        second = mask_of_stats(lib, br, p, par, stats[p], prior=union) if br.nifs > 1 else first[p]
        assert np.array_equal(second["mask"], union)
        repls.append(second["repl"])
        rfi_apply_device(lib, res, p, par, union, second["repl"])
    rows_parts = read_blocks(res, block_rows)
    lay()
    m, repl, cf, bf = host_arrays(br, nblk, br.nifs)
    gst = np.zeros((br.nifs, nblk, br.nchan, 2), dtype=np.uint64)
    used = C.c_uint32(99)
    err = C.create_string_buffer(512)
    with guarded():
        rc = lib.frbch_rfi_cleanp_device(C.byref(br.desc(0)), C.c_void_p(res.address), br.nrows, C.byref(par), None, 0, m.ctypes.data,
                                         repl.ctypes.data, cf.ctypes.data, bf.ctypes.data, gst.ctypes.data, C.byref(used), err, len(err))
    assert rc == 0, err.value
    assert used.value == kernel
    assert np.array_equal(gst, np.stack(stats))
    assert np.array_equal(m, union) and repl.tobytes() == np.stack(repls).tobytes() and np.array_equal(cf, cfu) and np.array_equal(bf, bfu)
    for a, b in zip(read_blocks(res, block_rows), rows_parts):
        assert np.array_equal(a, b)


# ---- fold -------------------------------------------------------------------------------------------------------------------
FOLD_TSAMP, FOLD_F0, FOLD_NBIN = 2.0 ** -14, 16.0, 256       # turns = t / 1024 exactly: bin = (t % 1024) // 4


def fold_rps(br):
    """rows per sub-integration: three sub-integrations, the last wholly past the last byte mark"""
    rps = br.byte_mark_rows[-1] // 2 + 64
    assert 2 * rps >= br.byte_mark_rows[-1] and 2 * rps < br.nrows <= 3 * rps
    return rps


def fold_par():
    return dict(F0=FOLD_F0, F1=0.0, PEPOCH=None, DM=0.0, PSR="x")


def fold_channels(nchan):
    """64 channels spread over the band"""
    return (np.arange(64) * (nchan // 64) + (np.arange(64) % 7)).astype(np.int64)


def want_fold(br, chans, nbin=FOLD_NBIN, tsamp=FOLD_TSAMP, rps=None):
    """sums [nsub][nifs][len(chans)][nbin] float64 and hits [nsub][nbin] from a count matrix count[sub][bin][t % P] times
    the base; the bins are fold_model_oracle.bins of one channel (no delays: every channel has the same)"""
    rps = rps or fold_rps(br)
    h = br.hdr(tsamp)
    b = fo.bins(br.nrows, 1, fch1=h["fch1"], foff=h["foff"], tsamp=tsamp, tstart_mjd=h["tstart"], nbin=nbin, f0=FOLD_F0, f1=0.0,
                pepoch_mjd=None)[:, 0]
    t = np.arange(br.nrows)
    nsub = -(-br.nrows // rps)
    flat = ((t // rps) * nbin + b) * br.P + t % br.P
    count = np.bincount(flat, minlength=nsub * nbin * br.P).reshape(nsub, nbin, br.P)
    hits = count.sum(axis=2).astype(np.uint32)
    cols = br.base[:, :, chans].astype(np.float64).reshape(br.P, -1)                 # [P][nifs * nch]; every sum is below 2^53
    sums = (count.reshape(nsub * nbin, br.P).astype(np.float64) @ cols).reshape(nsub, nbin, br.nifs, len(chans))
    return sums.transpose(0, 2, 3, 1), hits


def foldp_device(lib, res, nbin=FOLD_NBIN, tsamp=FOLD_TSAMP, rps=None):
    """frbch_foldp_device -> (profile [nsub][nifs][nbin][nchan] float64, hits [nsub][nbin][nchan] uint32, kernel_used)"""
    br = res.br
    rps = rps or fold_rps(br)
    desc = br.desc(0, tsamp)
    subint_s = rps * tsamp
    model, _keep = post.fold_model(fold_par(), br.hdr(tsamp), nbin=nbin, subint_s=subint_s, apply_delays=False)
    nsub = lib.frbch_fold_nsub(C.byref(desc), br.nrows, subint_s)
    assert nsub == -(-br.nrows // rps)
    d_prof = out_buffer(res.mem, nsub * br.nifs * nbin * br.nchan * 8)
    d_hits = out_buffer(res.mem, nsub * nbin * br.nchan * 4)
    used = C.c_uint32(99)
    err = C.create_string_buffer(512)
    with guarded():
        rc = lib.frbch_foldp_device(C.byref(desc), C.c_void_p(res.address), br.nrows, C.byref(model), 0, d_prof.ptr, d_hits.ptr, nsub,
                                    C.byref(used), err, len(err))
    assert rc == 0, err.value
    prof = d_prof.to_numpy(np.float64).reshape(nsub, br.nifs, nbin, br.nchan)
    hits = d_hits.to_numpy(np.uint32).reshape(nsub, nbin, br.nchan)
    d_prof.free()
    d_hits.free()
    return prof, hits, used.value


def fold_device(lib, res, prod, nbin=FOLD_NBIN, tsamp=FOLD_TSAMP, rps=None):
    """frbch_fold_device on one product -> (profile [nsub][nbin][nchan], hits [nsub][nbin][nchan])"""
    br = res.br
    rps = rps or fold_rps(br)
    desc = br.desc(prod, tsamp)
    subint_s = rps * tsamp
    nsub = lib.frbch_fold_nsub(C.byref(desc), br.nrows, subint_s)
    d_prof = out_buffer(res.mem, nsub * nbin * br.nchan * 8)
    d_hits = out_buffer(res.mem, nsub * nbin * br.nchan * 4)
    err = C.create_string_buffer(512)
    with guarded():
        rc = lib.frbch_fold_device(C.byref(desc), C.c_void_p(res.address), br.nrows, FOLD_F0, 0.0, TSTART, 0.0, 0, nbin, subint_s, 0,
                                   d_prof.ptr, d_hits.ptr, nsub, err, len(err))
    assert rc == 0, err.value
    prof = d_prof.to_numpy(np.float64).reshape(nsub, nbin, br.nchan)
    hits = d_hits.to_numpy(np.uint32).reshape(nsub, nbin, br.nchan)
    d_prof.free()
    d_hits.free()
    return prof, hits


def check_foldp(lib, res, kernel, **kw):
    br = res.br
    chans = fold_channels(br.nchan)
    sums, hits = want_fold(br, chans, **kw)
    assert sums.shape[0] == 3 and hits[2].sum() > 0
    prof, ghits, used = foldp_device(lib, res, **kw)
    assert used == kernel
    assert np.array_equal(ghits, np.broadcast_to(hits[:, :, None], ghits.shape))
    assert np.array_equal(prof[:, :, :, chans].transpose(0, 1, 3, 2), sums)


def check_fold(lib, res, prod, **kw):
    br = res.br
    chans = fold_channels(br.nchan)
    sums, hits = want_fold(br, chans, **kw)
    prof, ghits = fold_device(lib, res, prod, **kw)
    assert np.array_equal(ghits, np.broadcast_to(hits[:, :, None], ghits.shape))
    assert np.array_equal(prof[:, :, chans].transpose(0, 2, 1), sums[:, prod])


# ---- cut-outs ---------------------------------------------------------------------------------------------------------------
CUT_NT, CUT_NF, CUT_NDM = 64, 64, 16


def cut_cands(br, tsamp=None):
    """three candidates: near row 1000, a window across the row of the last byte mark, a window clamped at nrows"""
    hi = br.byte_mark_rows[-1]
    maxd = int(delays_of(br, [104.0], tsamp)[0].max())
    out = np.zeros(3, dtype=post.CUT_CAND)
    for o, (sample, f) in zip(out, ((min(1000, br.byte_mark_rows[0] // 2), 1), (hi - maxd // 2, 2), (br.nrows - maxd // 3, 3))):
        o["dm"], o["dm_lo"], o["dm_hi"], o["sample"], o["tfactor"] = 100.0, 96.0, 104.0, sample, f
    return out


def want_cutout(res, prod, cands, nt=CUT_NT, nf=CUT_NF, ndm=CUT_NDM, tsamp=None):
    """cutout_oracle.planes on the window of every candidate, the sample index shifted to the window's first row; `res`: the
    resident rows (with what poke() wrote) or their description"""
    br = getattr(res, "br", res)
    h = br.hdr(tsamp)
    parts = []
    for c in cands:
        f = int(c["tfactor"])
        t0 = int(c["sample"]) - (nt // 2) * f
        reach = max(int(co.delays(h, float(dm)).max()) for dm in (c["dm"], c["dm_hi"]))
        w0, w1 = max(0, t0), min(br.nrows, t0 + nt * f + reach + 1)
        moved = c.copy()
        moved["sample"] = int(c["sample"]) - w0
        x = res.window(w0, w1 - w0)[:, prod, :]
        assert w0 == 0 or t0 >= w0                       # no row in front of the window is asked for
        parts.append(co.planes(x, h, moved, nt, nf, ndm) + ((w0, w1),))
    return parts


def cutout_device(lib, res, prod, cands, nt=CUT_NT, nf=CUT_NF, ndm=CUT_NDM, tsamp=None):
    """-> ((ft, ft_hits, dt, dt_hits), kernel_used, frbch_cutout_kernel)"""
    br = res.br
    desc = br.desc(prod, tsamp)
    par = _lib.FrbchCutoutParams(C.sizeof(_lib.FrbchCutoutParams), nt, nf, ndm)
    cands = np.ascontiguousarray(cands)
    n = cands.size
    query = lib.frbch_cutout_kernel(C.byref(desc), C.c_void_p(res.address), br.nrows, C.byref(par), cands.ctypes.data, n)
    bufs = [out_buffer(res.mem, n * r * nt * 4) for r in (nf, nf, ndm, ndm)]
    used = C.c_uint32(99)
    err = C.create_string_buffer(512)
    with guarded():
        rc = lib.frbch_cutout_device(C.byref(desc), C.c_void_p(res.address), br.nrows, C.byref(par), cands.ctypes.data, n, 0, bufs[0].ptr,
                                     bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, C.byref(used), err, len(err))
    assert rc == 0, err.value
    out = tuple(b.to_numpy(dt).reshape(n, r, nt) for b, dt, r in zip(bufs, (np.float32, np.uint32, np.float32, np.uint32), (nf, nf, ndm, ndm)))
    for b in bufs:
        b.free()
    return out, used.value, query


def cut_kernel_expected(br, shift, tsamp=None):
    """the documented rule of the LDS cut-out kernel restated (tests/cutout_cases.lds_expected), with its two further clauses:
    at most 16 384 channels, and the rows at a 16-byte aligned address"""
    from tests import cutout_cases as cc
    cs = dict(hdr=br.hdr(tsamp), cands=cut_cands(br, tsamp), nt=CUT_NT, nf=CUT_NF, ndm=CUT_NDM)
    return cc.LDS if shift % 16 == 0 and br.nchan <= 16384 and cc.lds_expected(cs) == cc.LDS else cc.GENERIC


def check_cutout(lib, res, prod, kernel, tsamp=None, want=None):
    br = res.br
    cands = cut_cands(br, tsamp)
    want = want or want_cutout(res, prod, cands, tsamp=tsamp)
    hi = br.byte_mark_rows[-1]
    assert want[1][4][0] < hi < want[1][4][1] and want[2][4][1] == br.nrows
    assert want[2][3].min() < want[2][3].max()           # the clamped window: some pixels lost rows
    got, used, query = cutout_device(lib, res, prod, cands, tsamp=tsamp)
    assert used == query == kernel
    for i, w in enumerate(want):
        for name, g, x in zip(("ft", "ft_hits", "dt", "dt_hits"), got, w[:4]):
            assert g[i].tobytes() == x.tobytes(), "candidate %d, plane %s" % (i, name)


# ---- the search, and the chain --------------------------------------------------------------------------------------------
def spsearch_device(lib, series_address, ndm, nout, sp, cap=4096):
    """frbch_spsearch_device on series[ndm][nout] at `series_address` -> (records, ncand, kernel_used)"""
    cands = np.zeros(cap, dtype=post.SP_CAND)
    ncand, used = C.c_uint64(0), C.c_uint32(99)
    err = C.create_string_buffer(512)
    with guarded():
        rc = lib.frbch_spsearch_device(C.c_void_p(series_address), ndm, nout, C.byref(sp), 0, cands.ctypes.data, cap, C.byref(ncand),
                                       C.byref(used), err, len(err))
    assert rc == 0, err.value
    return cands[: ncand.value], ncand.value, used.value


def write_burst(res, prod, dm, t_top, width, amp, tsamp=None):
    """a dispersed burst of `width` rows, + amp per channel, that reaches the top of the band at row t_top"""
    br = res.br
    d = delays_of(br, [dm], tsamp)[0]
    n = int(d.max()) + width
    rows = res.window(t_top, n)
    c = np.arange(br.nchan)
    for k in range(width):
        rows[d + k, prod, c] += amp * (201 if br.nbits == 16 else 1)
    res.poke(t_top, rows)


def chain_of_stages(lib, res, prod, dms, sp, zerodm, clip, dm_gap, dm_span, tsamp=None):
    """dedispersion, search, grouping, selection of every group, cut-out candidates and cut-outs as single calls through the
    library on the resident rows -> dict with the keys of post.candidates_resident that the stages give"""
    br = res.br
    dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
    nout = lib.frbch_dedisperse_nout(C.byref(br.desc(prod, tsamp)), br.nrows, dm_arr.ctypes.data, dm_arr.size)
    d_out, nclip, k_dd = dedisp_device(lib, res, prod, dms, zerodm, clip, nout, tsamp)
    cands, _n, k_sp = spsearch_device(lib, d_out.ptr.value, len(dms), nout, sp)
    d_out.free()
    groups = post.group_candidates(cands, br.hdr(tsamp), dms, dm_gap=dm_gap, lib=lib)
    cut = post.cutout_cands(groups["best"], dms, dm_span)
    planes, k_cut, _q = cutout_device(lib, res, prod, cut, tsamp=tsamp)
    return dict(nout=nout, nclipped=nclip, cands=cands, groups=groups, cut_cands=cut, ft=planes[0], ft_hits=planes[1], dt=planes[2],
                dt_hits=planes[3], kernel_used=[0, k_dd, k_sp, k_cut])
