"""GPU tests of the burst polarisation stage: the cases of tests/test_rm.py on the device, every device buffer a guarded buffer
of exactly the documented size, checksummed (inputs) and guard-checked behind every call.  Both kernels of both stages are
forced by shape and address -- 8-bit rows of 96 channels hold no whole 64-byte tile, rows laid 4 bytes off a 16-byte boundary
and float rows take the generic burst kernel; fewer than 64 trials, or an F laid 4 bytes off its 8-byte boundary, take the
generic transform, so that every shape of the fast transform runs through the generic one as well -- with kernel_used asserted;
fast = generic = tests/rm_oracle.py byte for byte.  One case reads a burst beyond the 2^32-byte mark of 4.4 GB of rows, built
as tests/test_gpu_beyond_4gib.py builds its own."""
import ctypes as C

import numpy as np
import pytest

from frb_baseband_amd import post
from tests import big_rows as bg
from tests import rm_cases as rc
from tests import rm_oracle as ro
from tests.hipmem import GuardedBuffer

pytestmark = pytest.mark.gpu

FAST, GENERIC = 1, 0


def held(arr, misalign=0):
    """-> (guarded buffer of exactly the array's bytes (+ misalign in front), pointer to the array)"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = GuardedBuffer.from_numpy(np.concatenate([np.zeros(misalign, np.uint8), raw]) if misalign else raw)
    assert buf.ptr.value % 16 == 0
    return buf, C.c_void_p(buf.ptr.value + misalign)


def spectra_kernel_expected(hdr, rows, misalign):
    return FAST if rows.dtype != np.float32 and (hdr["nchans"] * rows.dtype.itemsize) % 64 == 0 and misalign % 16 == 0 else GENERIC


def device_spectra(lib, hdr, rows, cands, coh, misalign=0, gain=None):
    """frbch_burstspec_device -> (sums, spec, noise, used, kernel)"""
    n, nifs, nchan = cands.size, rows.shape[1], hdr["nchans"]
    buf, ptr = held(rows, misalign)
    d_sums = GuardedBuffer(n * nifs * nchan * post.BURST_SUMS.itemsize)
    spec, noise = np.zeros((n, nifs, nchan), np.float32), np.zeros((n, nifs, nchan), np.float32)
    used = np.zeros((n, nchan), np.uint8)
    par, desc = rc.burst_par(coh), rc.desc_of(hdr, rows)
    query = lib.frbch_burstspec_kernel(C.byref(desc), ptr, rows.shape[0], C.byref(par), cands.ctypes.data, n)
    k = C.c_uint32(99)
    err = C.create_string_buffer(512)
    with bg.guarded():
        code = lib.frbch_burstspec_device(C.byref(desc), ptr, rows.shape[0], C.byref(par), cands.ctypes.data, n,
                                          gain.ctypes.data if gain is not None else None, 0, d_sums.ptr, spec.ctypes.data, noise.ctypes.data,
                                          used.ctypes.data, C.byref(k), err, len(err))
    assert code == 0, err.value
    buf.check(contents=True)
    d_sums.check()
    sums = d_sums.to_numpy(np.uint8).view(post.BURST_SUMS).reshape(n, nifs, nchan).copy()
    buf.free()
    d_sums.free()
    assert k.value == query
    return sums, spec, noise, used, k.value


def device_rm(lib, hdr, q, u, used, nphi, phi_lo, dphi, misalign=0):
    """frbch_rmsynth_device -> (F float32 [ncand][nphi][2], (form, split)); misalign = 4 lays F off its 8-byte boundary, which
    takes the generic kernel at any shape"""
    ncand = q.shape[0]
    bufs = [held(np.ascontiguousarray(a)) for a in (q.astype(np.float32), u.astype(np.float32), used.astype(np.uint8))]
    d_F = GuardedBuffer(ncand * nphi * 8 + misalign)
    f_ptr = C.c_void_p(d_F.ptr.value + misalign)
    par = post.rm_params(nphi, phi_lo, dphi)
    nsplit = C.c_uint32(99)
    query = lib.frbch_rmsynth_kernel(C.byref(post.fil_desc(hdr)), f_ptr, ncand, C.byref(par), C.byref(nsplit))
    k = (C.c_uint32 * 2)(99, 99)
    err = C.create_string_buffer(512)
    with bg.guarded():
        code = lib.frbch_rmsynth_device(C.byref(post.fil_desc(hdr)), bufs[0][1], bufs[1][1], bufs[2][1], ncand, C.byref(par), 0, f_ptr, k,
                                        err, len(err))
    assert code == 0, err.value
    for b, _p in bufs:
        b.check(contents=True)
        b.free()
    d_F.check()
    F = d_F.to_numpy(np.uint8)[misalign:].view(np.float32).reshape(ncand, nphi, 2).copy()
    d_F.free()
    assert (k[0], k[1]) == (query, nsplit.value)
    return F, (k[0], k[1])


# ---- step 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_spectra_equal_the_oracle_in_both_kernels(hip_lib, name):
    """at the aligned address (the fast kernel wherever the layout allows it) and 4 bytes further on (the generic one)"""
    hdr, rows, cands, coh = rc.case(name)
    want = rc.want_spectra(name)
    for misalign in (0, 4):
        got = device_spectra(hip_lib, hdr, rows, cands, coh, misalign)
        assert got[4] == spectra_kernel_expected(hdr, rows, misalign), (name, misalign)
        for a, b, what in zip(got[:4], want, ("sums", "spec", "noise", "used")):
            assert a.tobytes() == b.tobytes(), (name, misalign, what)
    kernels = {n: spectra_kernel_expected(rc.case(n)[0], rc.case(n)[1], 0) for n in rc.CASES}
    assert kernels["u8_96ch"] == GENERIC and kernels["f32_64ch"] == GENERIC and kernels["u8_64ch"] == kernels["u8_1024ch"] == FAST


def test_gains_on_the_device(hip_lib):
    hdr, rows, cands, coh = rc.case("u16_64ch_coherency")
    gain = np.random.default_rng(5).uniform(0.5, 2.0, size=(4, 64)).astype(np.float32)
    gain[1, 7], gain[3, 11] = -1.5, np.inf
    want = ro.derive(rc.want_spectra("u16_64ch_coherency")[0], gain, True)
    got = device_spectra(hip_lib, hdr, rows, cands, coh, 0, gain)
    assert got[4] == FAST
    for a, b in zip(got[1:4], want):
        assert a.tobytes() == b.tobytes()


# ---- step 2 ----------------------------------------------------------------------------------------------------------
# nchan, ncand, nphi, phi_lo, dphi, masked channels, (form, split)
RM_SHAPES = [(64, 1, 1, 250.0, 10.0, (), (GENERIC, 1)), (64, 3, 63, -3100.0, 100.0, (3, 40), (GENERIC, 1)),
             (64, 1, 257, -12800.0, 100.0, (), (FAST, 1)), (64, 3, 257, -12800.0, 100.0, (3, 40), (FAST, 1)),
             (96, 3, 257, -3000.0, 23.5, (), (FAST, 2)), (96, 1, 4096, -1.0e5, 48.8, (0, 95), (FAST, 2)),
             (1024, 1, 257, -12800.0, 100.0, (5,), (FAST, 16)), (1000, 3, 257, -12800.0, 100.0, (), (FAST, 16)),
             (1024, 3, 4096, -2.0e5, 97.7, (100, 101, 102), (FAST, 16))]


@pytest.mark.parametrize("nchan,ncand,nphi,phi_lo,dphi,masked,kernel", RM_SHAPES)
def test_transform_equals_the_oracle(hip_lib, nchan, ncand, nphi, phi_lo, dphi, masked, kernel):
    """splits of 48 of 96 and 64 of 1024 channels divide them, 63 of 1000 does not (the last piece is shorter, and shorter
    again where a candidate has masked channels: the records are packed)"""
    hdr, q, u, used = rc.spectra(nchan, ncand, 0, masked)
    want = rc.want_transform(nchan, ncand, nphi, phi_lo, dphi, 0, masked).tobytes()
    F, k = device_rm(hip_lib, hdr, q, u, used, nphi, phi_lo, dphi)
    assert k == kernel and F.tobytes() == want
    F, k = device_rm(hip_lib, hdr, q, u, used, nphi, phi_lo, dphi, misalign=4)
    assert k == (GENERIC, 1) and F.tobytes() == want


def test_dead_candidates_and_the_rmsf_on_the_device(hip_lib):
    hdr, q, u, used = rc.spectra(96, 3, 1)
    q2, u2, used2 = q.copy(), u.copy(), used.copy()
    q2[1], u2[1] = 0.0, 0.0
    used2[2] = 0
    F, k = device_rm(hip_lib, hdr, q2, u2, used2, 257, -12800.0, 100.0)
    assert k == (FAST, 2) and F[0].any() and not F[1].any() and not F[2].any()
    assert F.tobytes() == ro.transform(q2, u2, used2, hdr, 257, -12800.0, 100.0)[0].tobytes()
    ones = used.astype(np.float32)
    F, k = device_rm(hip_lib, hdr, ones, np.zeros_like(ones), used, 257, -128 * 37.5, 37.5)
    assert (F[:, 128, 0] == 1.0).all() and not F[:, 128, 1].any() and (np.hypot(F[..., 0], F[..., 1]) <= 1.0).all()


# ---- the composite ---------------------------------------------------------------------------------------------------
device_burst_rm = rc.device_burst_rm


@pytest.mark.parametrize("name", ["u8_64ch_3cand", "u16_64ch_coherency", "f32_64ch", "u8_96ch", "u8_1024ch"])
def test_composite_equals_the_oracle(hip_lib, name):
    hdr, rows, cands, coh = rc.case(name)
    _sums, spec, noise, used = rc.want_spectra(name)
    F, res = rc.want_rm(name)
    for misalign in (0, 4):
        buf, ptr = held(rows, misalign)
        got, k = device_burst_rm(hip_lib, hdr, ptr, rows.shape[0], cands, coh, **rc.GRID)
        buf.check(contents=True)
        buf.free()
        assert k[0] == spectra_kernel_expected(hdr, rows, misalign) and k[1] == FAST
        assert got["spec"].tobytes() == spec.tobytes() and got["noise"].tobytes() == noise.tobytes() and got["used"].tobytes() == used.tobytes()
        assert got["F"].tobytes() == F.tobytes() and rc.same_results(got["results"], res)


def test_known_answer(hip_lib):
    """the injected RMs at 1.2 - 1.5 GHz through the host entry point: the trial of the plain fp64 evaluation, its parabola
    within the tolerance measured in tests/rm_cases.known_oracle (twice the largest |F_int - F_fp64| / max|F_fp64|, carried
    through the parabola), and the bytes of the oracle's F"""
    hdr, rows, cands, (nphi, phi_lo, dphi) = rc.known_case()
    k = rc.known_oracle()
    info = {}
    got = post.burst_rm(rows, hdr, cands, nphi, phi_lo, dphi, lib=hip_lib, info=info)
    assert info["spectra_kernel_used"] == FAST and info["kernel_used"] == FAST
    assert np.ascontiguousarray(got["F"]).view(np.float32).tobytes() == k["F"].tobytes()
    assert rc.same_results(got["results"], k["results"])
    for i in range(2):
        r = got["results"][i]
        print("burst %d: rm %.4f (fp64 parabola %.4f, injected %.1f), tolerance %.3e, delta %.3e" % (i, r["rm"], k["fit"][i][0], rc.KNOWN_RMS[i],
                                                                                                    k["tol"][i], k["delta"]))
        assert int(r["kpeak"]) == k["k0"][i] and int(r["fitted"]) == 1
        assert abs(float(r["rm"]) - k["fit"][i][0]) <= k["tol"][i]
        assert abs(float(r["rm"]) - rc.KNOWN_RMS[i]) <= 0.5 * dphi + k["tol"][i]


# ---- past the 4 GiB mark ---------------------------------------------------------------------------------------------
def test_a_burst_beyond_the_4gib_mark(hip_lib):
    """8192 channels x 4 products x 8 bit, 4.4 GB of rows: a burst of DM 104 that reaches the top of the band 300 rows behind
    the 2^32-byte row, its own amplitude in every product; a second candidate near row 1000 and a third whose later window is
    cut at nrows.  The fast kernel at the aligned address, the generic one 4 bytes further on; the expected sums are the
    oracle's on the window of rows each candidate reads."""
    br = bg.big("A8")
    assert (br.byte_mark_rows[-1] + 300) * br.row_bytes > 1 << 32
    rc.check_beyond_the_mark(hip_lib, br, bg.DeviceMem, behind=300, off_len=200, kernels=((0, FAST, FAST), (4, GENERIC, FAST)))
