"""Shared case table of the bounds tests (tests/test_bounds.py on the emulator, tests/test_gpu_bounds.py on the device): the
smallest shapes of every `_device` entry point that still have a ragged edge in every output dimension, run on guarded
buffers (tests/hipmem.py).  Every case does the same five things:
 1. outputs are guarded, poisoned and of exactly the documented size; inputs are guarded and checksummed;
 2. the call returns 0;
 3. the output equals the expected value to the bit (a poisoned byte left unwritten fails here).  Expected values are the
    existing restatements -- post_cases, spsearch_cases, cutout_cases / cutout_oracle, rfi_cases / rfi_oracle,
    post_oracle.cornerturn, the oracle's unpackers, the host path of the channeliser -- there is no oracle here;
 4. every guard is intact and every input unchanged (Env.done);
 5. stateless entry points (everything but process / flush / scan of a channeliser handle) are called a second time into the
    same, now dirty, output and must give the same bytes.
A case is a function of an Env, which knows the library, the buffer class that goes with it and whether the hand-written
kernels exist (`env.gpu`): where an entry point says which kernel ran, the case asserts the one it was written for on the
device, and the generic one on the emulator build, which has no other."""
import contextlib
import ctypes as C
import faulthandler
import functools

import numpy as np

from frb_baseband_amd import _lib, channeliser as ch, cornerturn as ct, multi_if, post, synth, vdif
from oracle import frb_oracle as o, post_oracle as po
from tests import cutout_cases as cc
from tests import cutout_oracle as co
from tests import kernel_table as kt
from tests import parity_util as pu
from tests import post_cases as pc
from tests import rfi_cases as rc
from tests import rfi_oracle as ro
from tests import spsearch_cases as sc
from tests import spsearch_oracle as so
from tests.hipmem import POISON, GuardedBuffer, guarded_for

CALL_LIMIT_S = 120          # a device call that has not come back by then ends the test process (traceback on stderr)
FAST, GENERIC = 1, 0


@contextlib.contextmanager
def guarded():
    faulthandler.dump_traceback_later(CALL_LIMIT_S, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


class Env:
    def __init__(self, lib, Buffer=None):
        self.lib = lib
        self.Buffer = Buffer or guarded_for(lib)
        self.gpu = issubclass(self.Buffer, GuardedBuffer)
        self.bufs = []

    def out(self, nbytes):
        """a guarded, poisoned output of exactly nbytes"""
        self.bufs.append(self.Buffer(nbytes))
        return self.bufs[-1]

    def inp(self, arr):
        """a guarded, checksummed input"""
        self.bufs.append(self.Buffer.from_numpy(arr))
        return self.bufs[-1]

    def inp_shifted(self, arr, shift):
        """`arr` resident `shift` bytes behind an aligned address: (buffer, address of the first byte of arr)"""
        raw = np.full(arr.nbytes + 16, POISON, np.uint8)
        raw[shift:shift + arr.nbytes] = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf = self.inp(raw)
        assert buf.ptr.value % 16 == 0
        return buf, C.c_void_p(buf.ptr.value + shift)

    def kernel(self, want):
        return want if self.gpu else GENERIC

    def done(self):
        """step 4, then the buffers go"""
        for b in self.bufs:
            b.check(contents=True)
        for b in self.bufs:
            b.free()
        self.bufs = []


def twice(env, call, compare):
    """steps 2, 3 and 5 of a stateless entry point: call() -> tuple of output arrays; compare(outputs) asserts step 3"""
    first = call()
    compare(first)
    second = call()
    compare(second)
    return first, second


def same_bytes(first, second):
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes(), "a second identical call into the dirty output gave other bytes"


CASES = []                  # (id, function of an Env, runs on the emulator build)


def add(name, emu=True):
    def deco(fn):
        CASES.append((name, fn, emu))
        return fn
    return deco


def ids(emu_only=False):
    return [c[0] for c in CASES if c[2] or not emu_only]


def run(lib, name, Buffer=None):
    """Buffer: the guarded buffer class of the case's buffers, if not the library's own (guarded_for)"""
    fn = next(c[1] for c in CASES if c[0] == name)
    env = Env(lib, Buffer)
    try:
        fn(env)
        env.done()
    finally:
        for b in env.bufs:                                  # (a failed case: free without a second verdict)
            b._release()


# ---- frbch_unpack_device ------------------------------------------------------------------------------------------------
def _frames(bits):
    """three 8032-byte frames whose payload walks through all 256 byte values"""
    payload = (np.arange(24000, dtype=np.uint32) * 37 % 256).astype(np.uint8)
    return vdif.frame_payload(payload, bw_mhz=32.0, bits=bits), payload


def _unpack(bits, decoder, nsamples, offset):
    def case(env):
        raw, payload = _frames(bits)
        spb = 4 // bits                                     # dual-pol samples per payload byte
        assert offset > 0 and (offset + -(-nsamples // spb) > 8000 or offset >= 8000) and offset < 8000 * 2
        volts = o.unpack_2bit(payload, np.array([-3.3359, -1.0, 1.0, 3.3359], np.float32)) if bits == 2 else o.unpack_1bit(payload)
        want = np.ascontiguousarray(volts.astype(np.float32)[:, offset * spb: offset * spb + nsamples])
        if decoder == 1:
            want = np.stack([want, want])                   # the nibble table and the select chain
        d_raw = env.inp(raw)
        d_v = env.out(want.nbytes)
        with ch.Channeliser(ch.new_config(env.lib, bw_mhz=32.0, nchan=64, input_bits=bits), env.lib) as c:
            c.set_profiling(True)

            def call():
                with guarded():
                    c.unpack_device(d_raw.ptr.value, 3, 8032, 32, offset, nsamples, decoder, d_v.ptr.value, d_v.nbytes)
                return (d_v.to_numpy(np.float32).reshape(want.shape),)

            def compare(got):
                assert np.array_equal(got[0], want)
            same_bytes(*twice(env, call, compare))
            if env.gpu:                                     # decoder 0 is the generic tap by definition, decoder 1 the register one
                assert _launched(c) & {"frbch_unpack_tap", "frbch_unpack_tap_fast"} == {("frbch_unpack_tap", "frbch_unpack_tap_fast")[decoder]}
    return case


# an offset that crosses a frame boundary: the short runs start behind the first frame's last byte, the long ones straddle it
for _n in (1, 255, 257):
    add("unpack_2bit_dec0_n%d" % _n)(_unpack(2, 0, _n, 8003 if _n == 1 else 7990))
for _n in (2, 510, 514):
    # (the register kernels' decoders are not part of the emulator build)
    add("unpack_2bit_dec1_n%d" % _n, emu=False)(_unpack(2, 1, _n, 8004 if _n == 2 else 7988))
add("unpack_1bit_dec0_n1001")(_unpack(1, 0, 1001, 7990))


# ---- frbch_power_device -------------------------------------------------------------------------------------------------
def _raw_for(bw, nchan, nblocks, info, **gen):
    """frames that hold `nblocks` blocks and a little more"""
    need = (nblocks - 1) * info.block_stride_bytes + info.block_payload_bytes + 8000
    return synth.make_vdif(need / (abs(bw) * 1e6) * (2 // gen.get("bits", 2)), bw_mhz=abs(bw), nchan=nchan, **gen)


def _launched(c):
    return set(c.get_launch_record())


def _holds(names, families):
    """every prefix of `families` begins a kernel name of the launch record"""
    return all(any(n.startswith(f) for n in names) for f in families)


# the generic K1 and K2 (frbch_kc_dcfix is no fallback everywhere: at 2C = 256 the wave K2 has no register-pass Kc beside it)
FALLBACKS = {"frbch_k1_branch", "frbch_k2_chan"}


def _power(bw, nchan, kw, families, generic=()):
    """three blocks in one call, then the middle block alone at its payload offset into a buffer of exactly one block.
    families: kernel name prefixes the launch record must hold; generic: the fallbacks it must hold (and no others)"""
    def case(env):
        cfg = pu.lib_cfg(env.lib, bw, nchan, 10.0, **kw)
        with ch.Channeliser(cfg, env.lib) as c:
            info = c.info
            assert info.block_stride_bytes == info.block_payload_bytes
            raw = _raw_for(bw, nchan, 3, info)
            nfr = raw.size // 8032
            d_raw = env.inp(raw)
            one = info.rows_per_block * info.nif * nchan * 4
            whole, block = env.out(3 * one), env.out(one)
            c.set_profiling(True)
            with guarded():
                c.power_device(d_raw.ptr.value, nfr, 8032, 32, 0, 3, whole.ptr.value, whole.nbytes)
            want = whole.to_numpy(np.uint8)
            # the expected rows are the library's own: none of their words is still the poison (whose float32 reading is finite)
            assert np.isfinite(want.view(np.float32)).all() and not (want.view(np.uint32) == POISON * 0x01010101).any()

            def call():
                with guarded():
                    c.power_device(d_raw.ptr.value, nfr, 8032, 32, info.block_payload_bytes, 1, block.ptr.value, block.nbytes)
                return (block.to_numpy(np.uint8),)

            def compare(got):
                assert got[0].tobytes() == want[one:2 * one].tobytes()
            same_bytes(*twice(env, call, compare))
            assert want.tobytes() == whole.to_numpy(np.uint8).tobytes()          # the first call's rows are as they were
            if env.gpu:
                names = _launched(c)
                assert _holds(names, families) and FALLBACKS & names == set(generic), sorted(names)
    return case


add("power_16MHz_32ch_lane")(_power(16.0, 32, {}, ["frbch_k2_lane"]))
add("power_16MHz_128ch_pol4_t8_wave")(_power(16.0, 128, dict(pol=4, tscr=8), ["frbch_k2_wave"]))
# float rows of four products at -t 1 stay on the two-wave frbch_k2_wave (priv_takes in frbch_launch.cpp: it writes them faster), so the
# power tap reaches frbch_k2_priv at the nearest shape that does not: -t 4
add("power_32MHz_1024ch_pol5_wave")(_power(32.0, 1024, dict(pol=5), ["frbch_k2_wave"]))
add("power_32MHz_1024ch_pol5_t4_priv")(_power(32.0, 1024, dict(pol=5, tscr=4), ["frbch_k2_priv"]))
add("power_32MHz_1024ch_t16_scrunch")(_power(32.0, 1024, dict(tscr=16), ["frbch_k2_", "frbch_k2_scrunch"]))
add("power_32MHz_1024ch_generic")(_power(32.0, 1024, dict(flags=3), [], generic=("frbch_k1_branch", "frbch_k2_chan")))


# ---- frbch_process_device + frbch_flush_device ---------------------------------------------------------------------------
def _device_rows(env, c, d_raw, nfr, offset, nblocks, feed=0):
    """process (in calls of `feed` blocks; 0: one call) + flush into ONE guarded row buffer of exactly rows * row_bytes, every
    call behind the rows of the one before -> the bytes"""
    info = c.info
    rows = nblocks * info.rows_per_block
    out = env.out(rows * info.row_bytes)
    r1 = 0
    with guarded():
        for b0 in range(0, nblocks, feed or nblocks):
            nb = min(feed or nblocks, nblocks - b0)
            r1 += c.process_device(d_raw.ptr.value, nfr, 8032, 32, offset + b0 * info.block_stride_bytes, nb, out.ptr.value + r1 * info.row_bytes,
                                   out.nbytes - r1 * info.row_bytes)
        r2 = c.flush_device(out.ptr.value + r1 * info.row_bytes, out.nbytes - r1 * info.row_bytes)
    assert r1 + r2 == rows
    return out.to_numpy(np.uint8)


# the generic kernels of the coherent filterbank's stages
COH_FALLBACKS = {"frbch_k2c_chirp", "frbch_k3_dedisp", "frbch_k4_out"}


def _process(bw, nchan, secs, kw, families, generic=(), feed=0):
    """the rows of the device path against the rows of the host path (channelise_bytes) of the same configuration, which the
    parity suite holds against the oracle.  families: kernel name prefixes the launch record must hold (the kernels the case was
    chosen for, by the rules of make_plan and priv_takes); generic: the fallbacks it must hold (and no others)"""
    def case(env):
        kw_ = dict(kw)
        start = kw_.get("start", 0.0)
        raw = synth.make_vdif(secs + start, bw_mhz=abs(bw), nchan=nchan)
        with ch.Channeliser(pu.lib_cfg(env.lib, bw, nchan, secs, **kw_), env.lib) as c:
            fil = c.channelise_bytes(raw)
            body = np.frombuffer(fil, np.uint8)[len(c.sigproc_header()):]
        kw_.pop("start", None)
        with ch.Channeliser(pu.lib_cfg(env.lib, bw, nchan, secs, **kw_), env.lib) as c:
            info = c.info
            assert body.size % info.row_bytes == 0 and (body.size // info.row_bytes) % info.rows_per_block == 0
            nblocks = body.size // info.row_bytes // info.rows_per_block
            offset = int(round(start * 2e6 * abs(bw))) // 2           # -S as the host path takes it: whole payload bytes
            nfr = raw.size // 8032
            assert nblocks >= 1 and offset + (nblocks - 1) * info.block_stride_bytes + info.block_payload_bytes <= nfr * 8000
            d_raw = env.inp(raw)
            c.set_profiling(True)
            got = _device_rows(env, c, d_raw, nfr, offset, nblocks, feed)
            differ = np.flatnonzero(got != body)
            assert differ.size == 0, "%d of %d bytes differ from the host path's, the first at %d" % (differ.size, body.size, differ[0])
            if env.gpu:
                names = _launched(c)
                assert _holds(names, families) and (FALLBACKS | COH_FALLBACKS) & names == set(generic), sorted(names)
    return case


# 1024 channels behind the paired K1 (R = 2048) at -t <= 4: frbch_k2_priv takes codes, statistics passes and, at -t 4, float rows
PRIV = ["frbch_k1_wave", "frbch_k2_priv"]
add("process_32ch_pol4_2bit")(_process(32.0, 32, 0.02, dict(pol=4, nbit=2), ["frbch_k1_wave", "frbch_k2_lane"]))
add("process_32ch_pol0_interval")(_process(16.0, 32, 0.02, dict(pol=0, interval=0.004, const=0, maxb=5), ["frbch_k1_wave", "frbch_k2_lane"]))
add("process_128ch_pol4_t8")(_process(16.0, 128, 0.05, dict(pol=4, tscr=8), ["frbch_k1_wave", "frbch_k2_wave<0, 2, 4,"]))
add("process_128ch_t64_2bit")(_process(16.0, 128, 0.1, dict(tscr=64, nbit=2), ["frbch_k1_wave", "frbch_k2_wave", "frbch_k2_scrunch"]))
# four blocks in calls of three and one, as the host path stages them with maxb = 3: the first call's batch is deferred, the second
# call writes its float rows after all (one call of four blocks would be cut into two batches of two, and nothing deferred)
add("process_1024ch_twopass_pol4_t2_16bit_maxb3")(_process(32.0, 1024, 0.27, dict(flags=1 << 28, pol=4, tscr=2, nbit=16, maxb=3), PRIV, feed=3))
add("process_1024ch_twopass_t4_2bit_interval")(
    _process(32.0, 1024, 0.27, dict(flags=1 << 28, pol=2, tscr=4, nbit=2, interval=0.1, maxb=2), PRIV))
add("process_1024ch_float_pol4_t4")(_process(-32.0, 1024, 0.14, dict(pol=4, tscr=4, nbit=-32), PRIV))
add("process_1024ch_start_off_the_piece")(_process(32.0, 1024, 0.2, dict(start=10 / 64e6), ["frbch_k2_wave<3,"], generic=("frbch_k1_branch",)))
# 16 channels: 2C = 32 is below what frbch_k2c_fast (2C >= 512) and frbch_k4_fast (64-column tiles) take, so those two stages are
# the generic kernels by plan; K1 and K3 are the register-pass ones.  256 channels: M = 2 / 2, all four stages register-pass
add("process_coherent_16ch_dm1")(_process(16.0, 16, 0.012, dict(dm=1.0, coherent=1, freq=316.0), ["frbch_k1_", "frbch_k3_"],
                                       generic=("frbch_k2c_chirp", "frbch_k4_out")))
add("process_coherent_256ch_dm20")(_process(16.0, 256, 0.2, dict(dm=20.0, coherent=1, freq=600.0, pol=0, nbit=16),
                                        ["frbch_k1_fast<1>", "frbch_k2c_fast<1,", "frbch_k3_fast<1,", "frbch_k4_fast"]))
# (one block of 2^26 samples: several seconds of the emulator's loops, so on the device only)
add("process_4096ch_t4_2bit", emu=False)(_process(-64.0, 4096, 0.55, dict(tscr=4, nbit=2), kt.case_kernels(-64.0, 4096, 0.55, dict(tscr=4, nbit=2))))


# ---- frbch_scan_device --------------------------------------------------------------------------------------------------
def _scan(nif, bw, nchan, secs, kw, overlaps, families):
    """every IF's columns of the scan's row buffer (rows_cap exact) against that IF's own frbch_process_device rows, for
    every lane setting"""
    def case(env):
        raws = [synth.make_vdif(secs, bw_mhz=bw, nchan=nchan, if_index=i + 1) for i in range(nif)]
        bufs = [env.inp(r) for r in raws]
        nfr = raws[0].size // 8032
        scans = []
        for overlap in overlaps:
            chans = []
            for i in range(nif):
                cfg = pu.lib_cfg(env.lib, bw if i % 2 else -bw, nchan, secs, **kw)
                cfg.overlap = overlap
                chans.append(ch.Channeliser(cfg, env.lib))
                chans[-1].set_profiling(True)
            info = chans[0].info
            nblocks = (nfr * 8000) // info.block_payload_bytes
            rows = nblocks * info.rows_per_block
            out = env.out(rows * nif * info.row_bytes)
            with guarded():
                assert multi_if.scan_device(chans, [b.ptr.value for b in bufs], nfr, 8032, 32, 0, nblocks, out.ptr.value, rows) == rows
            seg = info.row_bytes // info.nif                                   # bytes of one product line of one IF
            scans.append(out.to_numpy(np.uint8).reshape(rows, info.nif, nif * seg))
            for c in chans:
                if env.gpu:
                    names = _launched(c)
                    assert _holds(names, families) and not FALLBACKS & names, sorted(names)
                c.close()
        for i in range(nif):
            with ch.Channeliser(pu.lib_cfg(env.lib, bw if i % 2 else -bw, nchan, secs, **kw), env.lib) as c:
                single = _device_rows(env, c, bufs[i], nfr, 0, nblocks).reshape(rows, info.nif, seg)
            for s in scans:
                assert s[:, :, i * seg:(i + 1) * seg].tobytes() == single.tobytes()
    return case


add("scan_3if_32ch_pol4_2bit")(_scan(3, 16.0, 32, 0.02, dict(pol=4, nbit=2), (1, 0), ["frbch_k1_wave", "frbch_k2_lane"]))
# (1 << 27, the buffered form, writes float rows at -t 1: those stay on the two-wave frbch_k2_wave, priv_takes in frbch_launch.cpp)
add("scan_2if_1024ch_pol5_8bit")(_scan(2, 32.0, 1024, 0.14, dict(pol=5, flags=1 << 27), (1, 192 | (3 << 24)), ["frbch_k1_wave", "frbch_k2_wave<3,"]))


# ---- frbch_dedisperse_device --------------------------------------------------------------------------------------------
def _dedisp(nchan, nbits, nout, ndm, zerodm, clip, kernel, shift=0, nifs=2, prod=1):
    def case(env):
        hdr = pc.make_hdr(nchan)
        dms = [20.0 + 1.5 * i for i in range(ndm)]
        nrows = nout + int(po.delays_samples(hdr["fch1"], hdr["foff"], nchan, hdr["tsamp"], dms[-1]).max())
        rows = pc.make_rows(nrows, nifs, nchan, nbits, seed=31, hdr=hdr)
        want, wclip = pc.want_dedisp(rows, hdr, prod, dms, zerodm, clip)
        assert want.shape == (ndm, nout) and pc.dedisp_nout(env.lib, hdr, rows, prod, dms) == nout
        dm_arr = np.ascontiguousarray(dms, dtype=np.float64)
        _buf, d_rows = env.inp_shifted(rows, shift)
        d_out = env.out(ndm * nout * 4)
        assert pc.dedisp_kernel(env.lib, hdr, rows, prod, dms, d_rows.value) == env.kernel(kernel)
        desc = pc.desc_of(hdr, rows, prod)

        def call():
            nclip = C.c_uint64(1 << 40)
            err = C.create_string_buffer(512)
            with guarded():
                code = env.lib.frbch_dedisperse_device(C.byref(desc), d_rows, nrows, dm_arr.ctypes.data, ndm, 1 if zerodm else 0, float(clip), 0,
                                                       d_out.ptr, nout, C.byref(nclip), err, len(err))
            assert code == 0, err.value
            return d_out.to_numpy(np.float32).reshape(ndm, nout), np.uint64(nclip.value)

        def compare(got):
            assert int(got[1]) == wclip and got[0].tobytes() == want.tobytes()
        same_bytes(*twice(env, call, compare))
    return case


# the time tile is 256, DMs go in groups of 8; 64 channels is the narrowest row the tiled kernel takes
for _nbits, _nout, _ndm, _z, _clip in [(8, 1, 1, False, 0.0), (8, 255, 9, False, 0.0), (8, 257, 9, True, 5.0), (16, 257, 1, True, 0.0),
                                        (16, 255, 9, False, 5.0), (32, 1, 9, True, 5.0), (32, 257, 9, False, 0.0)]:
    add("dedisp_tiled_b%d_nout%d_ndm%d" % (_nbits, _nout, _ndm))(_dedisp(64, _nbits, _nout, _ndm, _z, _clip, FAST))
# (48 channels of 8 and 16 bits are no whole 64-byte tiles; 48 floats are: float rows meet the generic kernel through the shift)
for _nbits, _nout, _ndm, _z, _clip in [(8, 257, 9, True, 5.0), (16, 255, 9, False, 0.0), (16, 1, 1, False, 0.0)]:
    add("dedisp_generic_48ch_b%d_nout%d_ndm%d" % (_nbits, _nout, _ndm))(_dedisp(48, _nbits, _nout, _ndm, _z, _clip, GENERIC))
for _nbits, _nout, _ndm, _z, _clip in [(8, 257, 9, True, 5.0), (32, 255, 1, False, 0.0)]:
    add("dedisp_generic_shift4_b%d_nout%d_ndm%d" % (_nbits, _nout, _ndm))(_dedisp(64, _nbits, _nout, _ndm, _z, _clip, GENERIC, shift=4))


# ---- frbch_fold_device, frbch_foldp_device -------------------------------------------------------------------------------
def _fold(nchan, nifs, nbits, nbin, nrows, rps, delays, kernel):
    """all products in one call (frbch_foldp_device) and the last product alone (frbch_fold_device); the last
    sub-integration is short; profile and hits buffers are exact"""
    def case(env):
        assert nrows % rps != 0
        hdr = pc.make_hdr(nchan)
        rows = pc.make_rows(nrows, nifs, nchan, nbits, seed=32, hdr=hdr)
        subint_s = (rps + 0.25) * hdr["tsamp"]
        wp, wh = pc.want_fold_all(rows, hdr, pc.PAR, nbin, subint_s, apply_delays=delays)
        nsub = -(-nrows // rps)
        assert wp.shape == (nsub, nifs, nchan, nbin)
        prod = nifs - 1
        w1p, w1h = pc.want_fold(rows, hdr, prod, pc.PAR, nbin, subint_s, delays)
        d_rows = env.inp(rows)
        full = dict(hdr, nifs=nifs, nbits=nbits)
        model, _keep = post.fold_model(pc.PAR, full, nbin=nbin, subint_s=subint_s, apply_delays=delays)
        desc, desc1 = post.fil_desc(full), post.fil_desc(full, product=prod)
        assert env.lib.frbch_fold_nsub(C.byref(desc), nrows, subint_s) == nsub
        nslot = nsub * nbin * nchan
        d_prof, d_hits = env.out(nslot * nifs * 8), env.out(nslot * 4)
        d_prof1, d_hits1 = env.out(nslot * 8), env.out(nslot * 4)

        def call_all():
            used = C.c_uint32(99)
            err = C.create_string_buffer(512)
            with guarded():
                code = env.lib.frbch_foldp_device(C.byref(desc), d_rows.ptr, nrows, C.byref(model), 0, d_prof.ptr, d_hits.ptr, nsub,
                                                  C.byref(used), err, len(err))
            assert code == 0, err.value
            assert used.value == env.kernel(kernel)
            return (d_prof.to_numpy(np.float64).reshape(nsub, nifs, nbin, nchan), d_hits.to_numpy(np.uint32).reshape(nsub, nbin, nchan))

        def call_one():
            err = C.create_string_buffer(512)
            with guarded():
                code = env.lib.frbch_fold_device(C.byref(desc1), d_rows.ptr, nrows, pc.PAR["F0"], pc.PAR["F1"], pc.PAR["PEPOCH"], pc.PAR["DM"],
                                                 1 if delays else 0, nbin, subint_s, 0, d_prof1.ptr, d_hits1.ptr, nsub, err, len(err))
            assert code == 0, err.value
            return (d_prof1.to_numpy(np.float64).reshape(nsub, nbin, nchan), d_hits1.to_numpy(np.uint32).reshape(nsub, nbin, nchan))

        # integer rows: to the bit; float rows: rtol 1e-12, the project's stated rule (atomic adds in any order), which the
        # second call is held to as well
        twice(env, call_all, lambda got: pc.check_fold(rows, got[0].transpose(0, 1, 3, 2), got[1].transpose(0, 2, 1), wp, wh))
        twice(env, call_one, lambda got: pc.check_fold(rows, got[0].transpose(0, 2, 1), got[1].transpose(0, 2, 1), w1p, w1h))
    return case


#                 nchan nifs nbits nbin nrows rps  delays kernel
for _f in [(16, 1, 8, 2, 777, 300, False, FAST), (48, 3, 16, 256, 1001, 400, False, FAST), (1024, 4, 8, 2, 300, 128, False, FAST),
           (16, 4, 16, 256, 777, 300, False, FAST), (48, 3, 8, 256, 1001, 400, True, GENERIC), (16, 1, 32, 2, 777, 300, True, GENERIC),
           (1024, 4, 32, 2, 300, 128, True, GENERIC), (48, 3, 32, 256, 1001, 400, False, GENERIC)]:
    add("fold_c%d_if%d_b%d_nbin%d_%s" % (_f[0], _f[1], _f[2], _f[3], "delays" if _f[6] else "plain"))(_fold(*_f))


# ---- frbch_spsearch_device ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sp_case(name, extra):
    y, widths, thr, L, want, _raws = sc.case(name)
    if extra:
        widths = tuple(widths) + (extra,)
        want = so.search(y, list(widths), thr, L)
        want.setflags(write=False)
    return y, widths, thr, L, want


def _spsearch(name, extra=0):
    """the series guarded and unchanged; the host records land in a slice of a larger poisoned array: the records around the
    slice and beyond `cap` stay poison, with cap == ncand and with cap < ncand (FRBCH_E_CAPACITY, the first cap records)"""
    def case(env):
        y, widths, thr, L, want = _sp_case(name, extra)
        assert want.size >= 2
        kernel = env.kernel(FAST if max(widths) <= sc.LDS_MAX_WIDTH else GENERIC)
        d_y = env.inp(y)
        params = post.sp_params(list(widths), thr, L)
        rec = post.SP_CAND.itemsize
        for cap in (want.size, want.size // 2):
            raw = np.full((want.size + 8) * rec, POISON, np.uint8)   # one array per cap: the second call writes into the first's records

            def call(raw=raw, cap=cap):
                ncand, used = C.c_uint64(0), C.c_uint32(99)
                err = C.create_string_buffer(512)
                with guarded():
                    code = env.lib.frbch_spsearch_device(d_y.ptr, y.shape[0], y.shape[1], C.byref(params), 0, raw.ctypes.data + 4 * rec, cap,
                                                         C.byref(ncand), C.byref(used), err, len(err))
                assert code == (0 if cap == want.size else _lib.E_CAPACITY), err.value
                assert used.value == kernel and ncand.value == want.size
                return (raw.copy(),)

            def compare(got, cap=cap):
                raw = got[0]
                assert np.all(raw[:4 * rec] == POISON) and np.all(raw[(4 + cap) * rec:] == POISON)
                assert sc.same_records(raw[4 * rec:(4 + cap) * rec].view(post.SP_CAND), want[:cap])
            same_bytes(*twice(env, call, compare))
    return case


add("spsearch_small_L64_w1")(_spsearch("small_L64_w1"))
add("spsearch_tile_plus_1")(_spsearch("tile_plus_1"))
add("spsearch_three_tiles_5")(_spsearch("three_tiles_5"))
add("spsearch_tile_plus_1_w1024_generic")(_spsearch("tile_plus_1", 1024))


# ---- frbch_cutout_device ------------------------------------------------------------------------------------------------
EDGES3 = [(56.7, 5, 3), (30.0, 1500, 512), (56.7, 2990, 1)]        # starts before row 0; a bin of 512 rows; ends past nrows
CUTOUTS = {
    "cutout_lds_b8_3cands_ndm9_nf16_nt6": (lambda: cc._case(64, 8, 3000, 6, 16, 9, EDGES3), 0),
    "cutout_lds_b16_1cand_ndm1_nf2_nt2": (lambda: cc._case(64, 16, 3000, 2, 2, 1, [(56.7, 1500, 3)]), 0),
    "cutout_lds_b16_3cands_ndm9_nf2_nt6_product": (lambda: cc._case(64, 16, 3000, 6, 2, 9, EDGES3, nifs=3, prod=2), 0),
    "cutout_generic_b32_3cands_ndm9_nf16_nt6": (lambda: cc._case(64, 32, 3000, 6, 16, 9, EDGES3), 0),
    "cutout_generic_b32_1cand_ndm1_nf2_nt2": (lambda: cc._case(64, 32, 3000, 2, 2, 1, [(56.7, 2999, 1)]), 0),
    "cutout_generic_shift4_b8_3cands_ndm9_nf16_nt6": (lambda: cc._case(64, 8, 3000, 6, 16, 9, EDGES3), 4),
}


@functools.lru_cache(maxsize=None)
def _cut_case(name):
    cs = CUTOUTS[name][0]()
    cs["rows"].setflags(write=False)
    want = co.planes_batch(cs["rows"][:, cs["prod"], :], cs["hdr"], cs["cands"], cs["nt"], cs["nf"], cs["ndm"])
    return cs, want


def _cutout(name):
    def case(env):
        cs, want = _cut_case(name)
        shift = CUTOUTS[name][1]
        kernel = GENERIC if shift else cc.lds_expected(cs)
        assert kernel == (GENERIC if "generic" in name else FAST)
        rows, cands = cs["rows"], np.ascontiguousarray(cs["cands"])
        _buf, d_rows = env.inp_shifted(rows, shift)
        dev = [env.out(w.nbytes) for w in want]                                  # all four planes, exact
        par = cc.params(cs["nt"], cs["nf"], cs["ndm"])
        assert cc.cutout_kernel(env.lib, cs, d_rows.value) == env.kernel(kernel)

        def call():
            used = C.c_uint32(99)
            err = C.create_string_buffer(512)
            with guarded():
                code = env.lib.frbch_cutout_device(C.byref(cc.desc_of(cs)), d_rows, rows.shape[0], C.byref(par), cands.ctypes.data, cands.size, 0,
                                                   dev[0].ptr, dev[1].ptr, dev[2].ptr, dev[3].ptr, C.byref(used), err, len(err))
            assert code == 0, err.value
            assert used.value == env.kernel(kernel)
            return tuple(d.to_numpy(w.dtype).reshape(w.shape) for d, w in zip(dev, want))

        def compare(got):
            assert cc.same_planes(got, want), cc.which_differ(got, want)
        same_bytes(*twice(env, call, compare))
    return case


for _name in CUTOUTS:
    add(_name)(_cutout(_name))


# ---- frbch_rfi_stats_device, frbch_rfi_apply_device, frbch_rfi_clean_device -------------------------------------------------
RULE3 = dict(rc.rule_kw(rc.DEFAULTS), t_cell=3.0)


def _rfi(nchan, nbits, nifs, prod, br, nrows, kernel, shift=0):
    """statistics into an exact buffer with the rows unchanged; apply and clean in place: the rows become the restatement's
    cleaned rows (every other product's bytes with them) and stay so under a second call"""
    def case(env):
        assert nrows % br != 0                                                   # a short last block
        rows = rc.make_rows(nrows, nifs, nchan, nbits, seed=nchan + nrows)
        par = rc.params(block_rows=br, t_cell=3.0)
        st = ro.stats(rows[:, prod, :], br)
        res = ro.mask(st, nrows, br, nbits, **RULE3)
        cleaned = ro.apply(rows, prod, br, res["mask"], res["repl"])
        assert res["mask"].any() and cleaned.tobytes() != rows.tobytes()
        desc = rc.desc_of(rows, prod)
        nblk = -(-nrows // br)
        in_place = [env.inp_shifted(rows, shift) for _ in range(3)]
        (b_apply, d_apply), (b_clean, d_clean), (b_again, d_again) = in_place
        d_stats = env.out(nblk * nchan * 16)
        want_kernel = env.kernel(kernel)
        assert want_kernel == (rc.fast_expected(nchan, nifs, nbits, d_apply.value) if env.gpu else GENERIC)
        assert env.lib.frbch_rfi_stats_kernel(C.byref(desc), d_apply, nrows, C.byref(par)) == want_kernel

        def call_stats():
            used = C.c_uint32(99)
            err = C.create_string_buffer(512)
            with guarded():
                code = env.lib.frbch_rfi_stats_device(C.byref(desc), d_apply, nrows, C.byref(par), 0, d_stats.ptr, C.byref(used), err, len(err))
            assert code == 0, err.value
            assert used.value == want_kernel
            return (d_stats.to_numpy(rc.stats_dtype(rows)).reshape(nblk, nchan, 2),)

        def compare_stats(got):
            assert got[0].dtype == st.dtype and got[0].tobytes() == st.tobytes()
        same_bytes(*twice(env, call_stats, compare_stats))
        b_apply.check(contents=True)                                             # statistics leave the rows alone
        d_mask, d_repl = env.inp(res["mask"]), env.inp(res["repl"])

        def cleaned_bytes():
            raw = np.full(rows.nbytes + 16, POISON, np.uint8)
            raw[shift:shift + rows.nbytes] = cleaned.view(np.uint8).reshape(-1)
            return raw

        def call_apply():
            err = C.create_string_buffer(512)
            with guarded():
                code = env.lib.frbch_rfi_apply_device(C.byref(desc), d_apply, nrows, C.byref(par), d_mask.ptr, d_repl.ptr, 0, err, len(err))
            assert code == 0, err.value
            return (b_apply.to_numpy(np.uint8),)

        # the host outputs of the clean: values no decision gives, so a cell left unwritten shows
        m, repl = np.full((nblk, nchan), 9, np.uint8), np.full(nchan, -1.0)
        cf, bf = np.full(nchan, 9, np.uint8), np.full(nblk, 9, np.uint8)

        def call_clean(b_clean, d_clean):
            used = C.c_uint32(99)
            err = C.create_string_buffer(512)
            with guarded():
                code = env.lib.frbch_rfi_clean_device(C.byref(desc), d_clean, nrows, C.byref(par), None, 0, m.ctypes.data, repl.ctypes.data,
                                                      cf.ctypes.data, bf.ctypes.data, C.byref(used), err, len(err))
            assert code == 0, err.value
            assert used.value == want_kernel
            return b_clean.to_numpy(np.uint8), m.copy(), repl.copy(), cf.copy(), bf.copy()

        def compare_rows(got):
            assert got[0].tobytes() == cleaned_bytes().tobytes()
        same_bytes(*twice(env, call_apply, compare_rows))
        # a clean works in place, and a second clean of cleaned rows sees other statistics: step 5 is a second call on a fresh copy
        # of the rows into the same, now dirty, host outputs
        first, second = call_clean(b_clean, d_clean), call_clean(b_again, d_again)
        for got in (first, second):
            compare_rows(got)
            assert rc.same_result(dict(mask=got[1], repl=got[2], chan_flag=got[3].astype(bool), blk_flag=got[4].astype(bool)), res)
        same_bytes(first, second)
        for b in (b_apply, b_clean, b_again):                                    # "unchanged" from here on: the cleaned rows
            b.expect(cleaned_bytes())
    return case


#                 nchan nbits nifs prod br nrows kernel
add("rfi_fast_64ch_b8")(_rfi(64, 8, 1, 0, 64, 200, FAST))
add("rfi_fast_1024ch_b8_if4_p2")(_rfi(1024, 8, 4, 2, 65, 150, FAST))              # the widest tile, 1024 bytes
add("rfi_fast_512ch_b16_if4_p2")(_rfi(512, 16, 4, 2, 64, 130, FAST))              # ... of 16-bit rows
add("rfi_generic_48ch_b8")(_rfi(48, 8, 1, 0, 64, 200, GENERIC))
add("rfi_generic_64ch_float_if4_p2")(_rfi(64, 32, 4, 2, 64, 200, GENERIC))
add("rfi_generic_shift4_64ch_b8")(_rfi(64, 8, 1, 0, 64, 200, GENERIC, shift=4))


# ---- frbch_cornerturn_device --------------------------------------------------------------------------------------------
def _cornerturn(mode, nframes):
    """(the corner turn is one kernel for every recipe, with no handle and no kernel_used: there is no kernel choice to assert)"""
    def case(env):
        _fps, recipe, _bits = ct.MODES[mode]
        hb, pin, _ = ct.frame_geometry(mode)
        frames = np.random.default_rng(nframes).integers(0, 256, size=(nframes, hb + pin), dtype=np.uint8)
        want = po.cornerturn(frames[:, hb:].reshape(-1), recipe)
        info = ct.recipe_info(recipe, env.lib)
        each = nframes * pin * 8 // info["word_bits"] * info["bits_per_word"] // 8
        assert len(want) == info["ntags"] and all(w.size == each for w in want)
        d_in = env.inp(frames)
        outs = [env.out(each) for _ in want]                                     # every tag's output, exact
        ptrs = (C.c_void_p * len(outs))(*[b.ptr.value for b in outs])

        def call():
            err = C.create_string_buffer(256)
            with guarded():
                code = env.lib.frbch_cornerturn_device(recipe.encode(), d_in.ptr, nframes, hb + pin, hb, ptrs, len(outs), each, 0, err, len(err))
            assert code == 0, err.value
            return tuple(b.to_numpy(np.uint8) for b in outs)

        def compare(got):
            for g, w in zip(got, want):
                assert np.array_equal(g, w)
        same_bytes(*twice(env, call, compare))
    return case


for _mode in sorted(ct.MODES):
    for _nfr in (1, 3):
        add("cornerturn_%s_%dframes" % (_mode, _nfr))(_cornerturn(_mode, _nfr))


# ---- the checker itself -------------------------------------------------------------------------------------------------
def poke_byte(Buffer, address, value):
    """one byte to `address`: a one-byte hipMemcpy on the device twin, a plain copy on the host twin"""
    one = np.array([value], np.uint8)
    if Buffer is GuardedBuffer:
        from tests.hipmem import hip
        assert hip().hipMemcpy(C.c_void_p(address), one.ctypes.data, 1, 1) == 0
    else:
        C.memmove(address, one.ctypes.data, 1)


def checker_self_test(Buffer):
    """a byte changed in the first byte behind the interior and in the last byte before it makes check() name the side and
    the offset; a changed byte of an uploaded input fails check(contents=True) and nothing else.  Every copy stays inside the
    allocation, and every byte is put back before the buffer is freed."""
    import pytest
    from tests.hipmem import _PATTERN
    n = 1000
    b = Buffer(n)
    assert np.all(b.to_numpy(np.uint8) == POISON) and b.nbytes == n
    b.check(contents=True)
    for side, offset, good in (("above", n, int(_PATTERN[0])), ("below", -1, int(_PATTERN[-1]))):
        poke_byte(Buffer, b.ptr.value + offset, good ^ 0xFF)
        with pytest.raises(AssertionError, match=r"guard %s a buffer of 1000 bytes at 0x[0-9a-f]+ \(allocated at bounds_cases\.py:\d+\) overwritten: 1 dirty bytes, "
                                                 r"offsets %d \.\. %d " % (side, offset, offset)):
            b.check()
        with pytest.raises(AssertionError, match="guard " + side):
            b.to_numpy(np.uint8)                            # any download checks every live buffer
        poke_byte(Buffer, b.ptr.value + offset, good)
        b.check()
    b.free()
    assert not b.ptr
    x = np.arange(n, dtype=np.uint8)
    b = Buffer.from_numpy(x)
    b.check(contents=True)
    poke_byte(Buffer, b.ptr.value + 3, 200)
    b.check()                                               # the guards are whole
    with pytest.raises(AssertionError, match=r"input buffer of 1000 bytes at 0x[0-9a-f]+ \(allocated at bounds_cases\.py:\d+\) was changed"):
        b.check(contents=True)
    poke_byte(Buffer, b.ptr.value + 3, 3)
    b.check(contents=True)
    assert np.array_equal(b.to_numpy(np.uint8), x)
    b.free()
