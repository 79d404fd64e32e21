"""Shared series of the single-pulse search tests (tests/test_spsearch.py on the emulator, tests/test_gpu_spsearch.py on the
device): a plain module of named cases -- (series [ndm][nout] float32, widths, threshold, detrend_len) -- and thin callers of
the C ABI.  Expected values are tests/spsearch_oracle.py on the same series, computed once per case."""
import ctypes as C
import functools

import numpy as np

from frb_baseband_amd import _lib, post
from tests import spsearch_oracle as so
from tests.hipmem import guarded_for

DEFAULT = post.default_widths(64e-6)                      # 1 .. 30
WIDE = [1, 7, 300, 1024]
TILE = 2048                                               # time tile of the LDS kernel
LDS_MAX_WIDTH = 512                                       # the largest width the LDS kernel takes


def noise(ndm, nout, seed):
    rng = np.random.default_rng(seed)
    return (100.0 + 10.0 * rng.standard_normal((ndm, nout))).astype(np.float32)


def add(y, dm, t, w, amp_sigma):
    """a top-hat of `w` samples from sample t, amp_sigma noise sigmas high per sample"""
    y[dm, t:t + w] += np.float32(10.0 * amp_sigma)


def alternating(ndm, nout):
    """+1, -1, +1, ...: mean 0 and sigma 1 exactly in every block of even length, q = +-1024"""
    return np.tile(np.where(np.arange(nout) % 2 == 0, 1.0, -1.0).astype(np.float32), (ndm, 1))


def _small():
    y = noise(1, 777, 11)
    add(y, 0, 0, 1, 9.0)                                  # at t = 0
    add(y, 0, 400, 1, 8.0)
    add(y, 0, 776, 1, 9.0)                                # the last sample
    return y, [1], 5.0, 64


def _blocks():
    y = noise(3, 5000, 12)
    add(y, 0, 999, 3, 6.0)                                # straddles the block edge at 1000
    add(y, 0, 0, 4, 5.0)                                  # starts at t = 0
    y[0, 3500] = np.nan                                   # block 3 of DM 0 is dead ...
    add(y, 0, 3600, 2, 9.0)                               # ... and hides this pulse
    add(y, 1, 2500, 6, 4.0)
    y[1, 4000:] = np.float32(7.0)                         # a constant (dead) last block
    add(y, 2, 4980, 20, 3.0)                              # ends at nout
    add(y, 2, 1990, 14, 3.0)                              # straddles the block edge at 2000
    return y, DEFAULT, 5.0, 1000


def _wide():
    y = noise(9, 20011, 13)
    for d in range(9):
        add(y, d, 1500 + 2000 * d, 300, 0.7 + 0.05 * d)   # 300 wide: 12 sigma and more in the 300-sample boxcar
        add(y, d, 700 + 1900 * d, 7, 4.0)
    add(y, 4, 12000, 1024, 0.5)                           # 16 sigma at width 1024
    add(y, 8, 20011 - 300, 300, 0.8)                      # ends at nout
    return y, WIDE, 5.0, 8192                             # (blocks of 1000 would normalise a 1024-sample pulse away)


def _short_block():
    y = noise(3, 777, 14)                                 # detrend_len > nout: one block; 1024 > nout: skipped
    add(y, 1, 300, 7, 4.0)
    add(y, 2, 200, 300, 0.8)
    return y, WIDE, 5.0, 1000


def _ties():
    """a plateau of equal samples on an exact background: two samples of 10 at 2000, 2001 (even, odd: the background they
    replace cancels, and round 2 drops them, so mean 0 and sigma 1 stay exact).  S_1 = 10240 at both (width 1
    has no window: two raw peaks); S_4 = 20480 at t = 1998, 1999, 2000 (the first is the peak, centre 2000): sigma 10.0 at
    widths 1 and 4 alike, the narrower ones survive.  DM 1 holds a plateau of four."""
    y = alternating(2, 5000)
    y[0, 2000:2002] = 10.0
    y[1, 3000:3004] = 10.0
    return y, [1, 4], 5.0, 1000


def _nothing():
    return noise(3, 5000, 15), DEFAULT, 50.0, 1000


def _four_pulses():
    """20 000 Gaussian samples: width 1 inside a block, width 3 across a block edge, width 6 inside, width 20 ending at nout"""
    y = noise(1, 20000, 16)
    add(y, 0, 4321, 1, 9.0)
    add(y, 0, 8999, 3, 6.0)
    add(y, 0, 12500, 6, 4.5)
    add(y, 0, 19980, 20, 3.0)
    return y, DEFAULT, 5.0, 1000


def _tile(nout, seed):
    def build():
        y = noise(9, nout, seed)
        for d in range(9):
            add(y, d, max(0, min(nout, TILE) - 3 - (d % 3)), 6, 4.0)      # width 6 across (or up to) the first tile edge
        if nout > TILE + 400:
            add(y, 1, TILE - 150, 300, 0.8)                               # width 300 across the edge
            add(y, 2, TILE - 1, 1, 9.0)                                   # the last sample of tile 0, its window crosses
            add(y, 3, TILE - 2, 4, 5.0)
            add(y, 4, 2 * TILE - 100, 300, 0.8)
            add(y, 5, 3 * TILE - 2, 6, 4.0)
            add(y, 6, nout - 6, 6, 4.0)
            add(y, 7, TILE, 2, 7.0)                                       # the first sample of tile 1
        return y, [1, 2, 4, 6, 30, 300], 5.0, 1000
    return build


CASES = {
    "small_L64_w1": _small, "blocks_default": _blocks, "wide_9dm": _wide, "one_block_skipped_width": _short_block, "ties": _ties,
    "nothing": _nothing, "four_pulses": _four_pulses,
}
TILE_CASES = {"tile_minus_1": _tile(TILE - 1, 21), "tile": _tile(TILE, 22), "tile_plus_1": _tile(TILE + 1, 23),
              "three_tiles_5": _tile(3 * TILE + 5, 24)}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (series, widths, threshold, detrend_len, oracle candidates, oracle raw lists); built once, never written to"""
    y, widths, thr, L = (CASES.get(name) or TILE_CASES[name])()
    y.setflags(write=False)
    want, raws = so.search(y, widths, thr, L, want_raw=True)
    want.setflags(write=False)
    return y, tuple(widths), thr, L, want, raws


def spsearch_host(lib, y, widths, thr, L, cap=4096):
    """frbch_spsearch_host -> (rc, candidates written, ncand, kernel_used, message)"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    params = post.sp_params(widths, thr, L)
    cands = np.zeros(cap, dtype=post.SP_CAND)
    ncand, used = C.c_uint64(0), C.c_uint32(99)
    err = C.create_string_buffer(512)
    rc = lib.frbch_spsearch_host(y.ctypes.data, y.shape[0], y.shape[1], C.byref(params), 0, cands.ctypes.data, cap, C.byref(ncand),
                                 C.byref(used), err, len(err))
    return rc, cands[: min(cap, ncand.value)], ncand.value, used.value, err.value.decode()


def device_search(lib, y, widths, thr, L, misalign=False, cap=4096):
    """frbch_spsearch_device on a guarded buffer of exactly ndm * nout floats (misalign: one float more, the series from its
    second float on) -> (candidates, kernel_used); the input's checksum and both guard bands are checked behind the call.
    Device memory for the product library, host memory for the emulator build"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    buf = guarded_for(lib).from_numpy(np.concatenate([np.zeros(1, dtype=np.float32), y.reshape(-1)]) if misalign else y)
    ptr = C.c_void_p(buf.ptr.value + (4 if misalign else 0))
    params = post.sp_params(widths, thr, L)
    cands = np.zeros(cap, dtype=post.SP_CAND)
    ncand, used = C.c_uint64(0), C.c_uint32(99)
    err = C.create_string_buffer(512)
    rc = lib.frbch_spsearch_device(ptr, y.shape[0], y.shape[1], C.byref(params), 0, cands.ctypes.data, cap, C.byref(ncand),
                                   C.byref(used), err, len(err))
    assert rc == 0, err.value
    buf.check(contents=True)
    buf.free()
    return cands[: ncand.value], used.value


def same_records(got, want):
    """record for record, every field, sigma to the bit"""
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
