"""Tiny ctypes view of the HIP runtime for tests: device buffers without torch.

DeviceBuffer is a bare hipMalloc (tools/*.py time with it).  GuardedBuffer is what the suite allocates: the same interface
with GUARD bytes of a position-dependent pattern on both sides of the interior, an interior that starts as POISON bytes, and
a checksum of whatever from_numpy uploaded -- so that a store past either end, an output byte that was never written and a
changed input are all seen.  HostGuardedBuffer is its twin in host memory for the emulator build, whose `_device` entry points
take host pointers; guarded_for(lib) picks the class by library."""
import ctypes as C
import sys
import weakref
import zlib

import numpy as np

_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipFree.argtypes = [C.c_void_p]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        _hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        _hip.hipStreamDestroy.argtypes = [C.c_void_p]
        _hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        _hip.hipStreamWaitEvent.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
        _hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        _hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        _hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        _hip.hipEventDestroy.argtypes = [C.c_void_p]
        _hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        _hip.hipEventSynchronize.argtypes = [C.c_void_p]
        _hip.hipEventQuery.argtypes = [C.c_void_p]
        _hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        _hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        _hip.hipHostFree.argtypes = [C.c_void_p]
    return _hip


def gpu_visible() -> bool:
    """torch.cuda.is_available(), asked in a child process.  torch brings its own HIP runtime; initialised in the test
    process before the product library's (the system one, loaded first), it leaves the library seeing no device."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.split()[-1] == "True"


class DeviceBuffer:
    def __init__(self, nbytes: int):
        self.ptr = C.c_void_p()
        self.nbytes = nbytes
        rc = hip().hipMalloc(C.byref(self.ptr), max(1, nbytes))
        if rc != 0:
            raise RuntimeError(f"hipMalloc failed ({rc})")

    @classmethod
    def from_numpy(cls, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        buf = cls(arr.nbytes)
        rc = hip().hipMemcpy(buf.ptr, arr.ctypes.data, arr.nbytes, 1)  # hipMemcpyHostToDevice
        assert rc == 0
        return buf

    def to_numpy(self, dtype, count=None) -> np.ndarray:
        hip().hipDeviceSynchronize()
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize if count is None else count, dtype=dtype)
        rc = hip().hipMemcpy(out.ctypes.data, self.ptr, out.nbytes, 2)  # hipMemcpyDeviceToHost
        assert rc == 0
        return out

    def free(self):
        if self.ptr:
            hip().hipFree(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- guarded buffers ------------------------------------------------------------------------------------------------------
GUARD = 1 << 20                 # bytes a side: 16 rows of the widest row of the suite (4096 channels x 4 products x 4 bytes), more
#                                 than any tile of rows a kernel stores at once; a multiple of every alignment a kernel choice looks at
POISON = 0xCB                   # float32 -2.67e7, float64 -7.8e58, uint32 3419130827, uint64 1.5e19: no case expects any of them, and
#                                 a sum accumulated on top of one stays as far off
_PATTERN = ((7 + 131 * np.arange(GUARD, dtype=np.int64)) & 0xFF).astype(np.uint8)
_PATTERN.setflags(write=False)
_LIVE = weakref.WeakSet()       # every guarded buffer not yet freed


def check_all_live():
    """the guards of every live guarded buffer (a failed test's buffers stay alive in its saved traceback: the message names
    the address and the line that allocated the buffer, so a guard that trips later is traced to its owner)"""
    for b in list(_LIVE):
        b.check()


def _site():
    """file:line of the nearest caller outside this module"""
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == __file__:
        f = f.f_back
    return "?" if f is None else "%s:%d" % (f.f_code.co_filename.rsplit("/", 1)[-1], f.f_lineno)


class _Guards:
    """The checking code both twins share.  A subclass provides _peek(offset, n) -> uint8 array and _poke(offset, uint8
    array), offsets counted from the START OF THE ALLOCATION (the interior begins at GUARD), and sets ptr / nbytes."""
    crc = None                  # zlib.crc32 of the uploaded bytes (from_numpy / expect), None for an output
    site = "?"                  # where the buffer was allocated

    def _arm(self):
        self.site = _site()
        self._poke(0, _PATTERN)
        self._poke(GUARD + self.nbytes, _PATTERN)
        _LIVE.add(self)

    @classmethod
    def from_numpy(cls, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        buf = cls(arr.nbytes, poison=False)
        buf._poke(GUARD, arr.view(np.uint8).reshape(-1))
        buf.expect(arr)
        return buf

    def expect(self, arr):
        """what check(contents=True) holds the interior against from now on: the bytes of `arr`"""
        self.crc = zlib.crc32(np.ascontiguousarray(arr).view(np.uint8).reshape(-1))

    def __str__(self):
        return "buffer of %d bytes at 0x%x (allocated at %s)" % (self.nbytes, self.ptr.value or 0, self.site)

    def check(self, contents=False):
        """both guards against their pattern; contents=True: the interior against the checksum of the upload as well
        (a buffer that was never uploaded to has none: its guards only)"""
        if not self.ptr:
            return
        for side, at, base in (("below", 0, -GUARD), ("above", GUARD + self.nbytes, self.nbytes)):
            dirty = np.flatnonzero(self._peek(at, GUARD) != _PATTERN)
            if dirty.size:
                raise AssertionError("guard %s a %s overwritten: %d dirty bytes, offsets %d .. %d relative to the buffer's first byte"
                                     % (side, self, dirty.size, base + int(dirty[0]), base + int(dirty[-1])))
        if contents and self.crc is not None:
            now = self._peek(GUARD, self.nbytes)
            if zlib.crc32(now) != self.crc:
                raise AssertionError("an input %s was changed (checksum %08x, uploaded %08x)" % (self, zlib.crc32(now), self.crc))

    def to_numpy(self, dtype, count=None) -> np.ndarray:
        check_all_live()
        n = self.nbytes if count is None else count * np.dtype(dtype).itemsize
        return self._peek(GUARD, n).view(dtype)

    def free(self):
        if self.ptr:
            try:
                self.check()
            finally:
                _LIVE.discard(self)
                self._release()

    def __del__(self):
        try:
            _LIVE.discard(self)
            self._release()
        except Exception:
            pass


class GuardedBuffer(_Guards, DeviceBuffer):
    """hipMalloc of nbytes + 2 GUARD; `ptr` is the interior, which keeps the alignment hipMalloc gave modulo 1 MiB"""

    def __init__(self, nbytes: int, poison=True):
        self.ptr = C.c_void_p()
        self.base = C.c_void_p()
        self.nbytes = nbytes
        rc = hip().hipMalloc(C.byref(self.base), nbytes + 2 * GUARD)
        if rc != 0:
            raise RuntimeError(f"hipMalloc failed ({rc})")
        self.ptr = C.c_void_p(self.base.value + GUARD)
        if poison and nbytes:
            assert hip().hipMemset(self.ptr, POISON, nbytes) == 0
        self._arm()

    def _peek(self, offset, n):
        hip().hipDeviceSynchronize()
        out = np.empty(n, dtype=np.uint8)
        if n:
            assert hip().hipMemcpy(out.ctypes.data, C.c_void_p(self.base.value + offset), n, 2) == 0
        return out

    def _poke(self, offset, data):
        data = np.ascontiguousarray(data)
        if data.nbytes:
            assert hip().hipMemcpy(C.c_void_p(self.base.value + offset), data.ctypes.data, data.nbytes, 1) == 0

    def _release(self):
        if self.base:
            hip().hipFree(self.base)
        self.base = C.c_void_p()
        self.ptr = C.c_void_p()


# StreamOrderBuffer's reads: a non-blocking stream of their own and a pinned staging area that grows to the largest read.  Both are
# kept for the life of the test process on purpose (one stream, one area): they go with the process, like the runtime itself
_reader = None
_staging = [C.c_void_p(), 0]


class StreamOrderBuffer(GuardedBuffer):
    """a GuardedBuffer read WITHOUT hipDeviceSynchronize: an asynchronous copy on a non-blocking stream of the reader's own
    into pinned memory, and a synchronise of that stream alone.  What a read sees is what the streams the test synchronised
    have written."""

    def _peek(self, offset, n):
        global _reader
        out = np.empty(n, dtype=np.uint8)
        if n:
            if _reader is None:
                _reader = Stream()
            if _staging[1] < n:
                if _staging[0]:
                    hip().hipHostFree(_staging[0])
                assert hip().hipHostMalloc(C.byref(_staging[0]), n, 0) == 0
                _staging[1] = n
            _reader.memcpy_async(_staging[0].value, self.base.value + offset, n, 2)   # hipMemcpyDeviceToHost
            _reader.synchronize()
            C.memmove(out.ctypes.data, _staging[0], n)
        return out

    def to_numpy(self, dtype, count=None) -> np.ndarray:
        for b in list(_LIVE):                       # (the guards of every live buffer of this class: the others' reads synchronise)
            if isinstance(b, StreamOrderBuffer):
                b.check()
        n = self.nbytes if count is None else count * np.dtype(dtype).itemsize
        return self._peek(GUARD, n).view(dtype)


# ---- streams, events, asynchronous copies -----------------------------------------------------------------------------------
D2D, H2D = 3, 1                  # hipMemcpyDeviceToDevice, hipMemcpyHostToDevice


class Stream:
    """a non-blocking stream (hipStreamNonBlocking): `handle` is what the `stream` argument of the C ABI takes"""

    def __init__(self):
        s = C.c_void_p()
        assert hip().hipStreamCreateWithFlags(C.byref(s), 1) == 0
        self.handle = s.value

    def synchronize(self):
        assert hip().hipStreamSynchronize(C.c_void_p(self.handle)) == 0

    def memcpy_async(self, dst, src, nbytes, kind=D2D):
        """dst, src: addresses; a host source must be pinned (PinnedArray) and stay as it is until the copy has run"""
        assert hip().hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), nbytes, kind, C.c_void_p(self.handle)) == 0

    def memset_async(self, dst, value, nbytes):
        assert hip().hipMemsetAsync(C.c_void_p(dst), value, nbytes, C.c_void_p(self.handle)) == 0

    def wait(self, event):
        assert hip().hipStreamWaitEvent(C.c_void_p(self.handle), event.handle, 0) == 0

    def destroy(self):
        if self.handle:
            hip().hipStreamDestroy(C.c_void_p(self.handle))
            self.handle = None


class Event:
    """a timing event"""

    def __init__(self):
        self.handle = C.c_void_p()
        assert hip().hipEventCreate(C.byref(self.handle)) == 0

    def record(self, stream=None):
        assert hip().hipEventRecord(self.handle, C.c_void_p(stream.handle if stream else None)) == 0
        return self

    def synchronize(self):
        assert hip().hipEventSynchronize(self.handle) == 0

    def done(self) -> bool:
        """hipEventQuery: False while work in front of the record is still running (hipErrorNotReady)"""
        rc = hip().hipEventQuery(self.handle)
        assert rc in (0, 600), rc
        return rc == 0

    def ms_since(self, start) -> float:
        """device time between `start` and this event, both recorded; waits for this one"""
        self.synchronize()
        ms = C.c_float()
        assert hip().hipEventElapsedTime(C.byref(ms), start.handle, self.handle) == 0
        return float(ms.value)

    def destroy(self):
        if self.handle:
            hip().hipEventDestroy(self.handle)
            self.handle = C.c_void_p()


class PinnedArray:
    """page-locked host memory holding a copy of `arr`: the source of an asynchronous upload"""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.nbytes = arr.nbytes
        self.ptr = C.c_void_p()
        assert hip().hipHostMalloc(C.byref(self.ptr), max(1, self.nbytes), 0) == 0
        C.memmove(self.ptr, arr.ctypes.data, self.nbytes)

    def free(self):
        if self.ptr:
            hip().hipHostFree(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HostGuardedBuffer(_Guards):
    """the same in host memory, one numpy array: for the emulator build, whose `_device` entry points take host pointers"""
    ALIGN = 256                                     # what hipMalloc gives at least

    def __init__(self, nbytes: int, poison=True):
        self.nbytes = nbytes
        self._mem = np.empty(nbytes + 2 * GUARD + self.ALIGN, dtype=np.uint8)
        self._at = -self._mem.ctypes.data % self.ALIGN
        self.base = C.c_void_p(self._mem.ctypes.data + self._at)
        self.ptr = C.c_void_p(self.base.value + GUARD)
        if poison:
            self._mem[self._at + GUARD: self._at + GUARD + nbytes] = POISON
        self._arm()

    def _peek(self, offset, n):
        return self._mem[self._at + offset: self._at + offset + n].copy()

    def _poke(self, offset, data):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self._mem[self._at + offset: self._at + offset + data.size] = data

    def _release(self):
        self._mem = None
        self.base = C.c_void_p()
        self.ptr = C.c_void_p()


def guarded_for(lib):
    """the guarded buffer class for a library: host memory for the emulator build (tests/emu), device memory otherwise"""
    return HostGuardedBuffer if "libfrbch_emu" in str(getattr(lib, "_name", "")) else GuardedBuffer
