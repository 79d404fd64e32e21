"""One row per register-pass kernel instantiation of the channeliser: its full name (as the demangled symbol spells it, which is
what the library's launch record reports) and the smallest configuration that reaches it, in the vocabulary of
parity_util.run_streaming_case: bw, nchan, secs, kwargs.

"Smallest": the smallest 2C x R block that make_plan maps to the instantiation, three blocks (four where a frame is flagged), two
blocks per launch (maxb = 2: two launches) and a rescale interval of 0.45 x secs, which ends inside the first launch: the
measuring form (float rows / statistics) and the digitising form of a kernel are both launched.  secs = 3 blocks + 0.3 of a block
(at least two frames).

tests/test_kernel_table.py (CPU) holds the table against the kernels the built library lists; tests/test_gpu_instantiations.py
(GPU) runs every row against the fp64 oracle with the launch record on.  Rows with the same configuration share one run.

Beyond one row per instantiation:
  * every K1 layout group in front of every K2 family (the "pairing" rows);
  * every family that emits codes at nbit 2, 8, 16 and -32 and in both band senses (asserted by test_kernel_table.py);
  * more than one trip, and unequal trip counts, of the persistent loops (the rows with grid_x / grid_y);
  * frbch_quantise_fast<8, 512> through a scan, frbch_unpack_tap_fast through the unpack tap;
  * frbch_k2_wave<5, ...> needs the 2^26-sample block (2C = R = 8192): its rows point at tests/test_gpu_parity.py::CASES entries,
    which run with the record on and carry the assertion there.
A row: name, bw, nchan, secs, kw; also = further kernels the same run must launch; frames = frames to flag invalid (parity_util.hurt_frames);
grid_x / grid_y = the largest grid the record must show; kind = stream | scan (frbch_scan_device, two IFs) | tap (unpack tap) | case.
"""
from collections import namedtuple

Row = namedtuple("Row", "name bw nchan secs kw also frames grid_x grid_y kind case")


def row(name, bw=0.0, nchan=0, secs=0.0, kw=None, also=(), frames=None, grid_x=None, grid_y=None, kind="stream", case=None):
    return Row(name, bw, nchan, secs, dict(kw or {}), tuple(also), frames, grid_x, grid_y, kind, case)


_COH = dict(dm=1.0, coherent=1, freq=1400.0)

ROWS = [
    # ---- K0: frbch_k0_stage<RB, WIDE>.  RB = half the K1 layout group; it runs where nchan % 256 == 0 (256 channels: blocks of
    # 2^18 .. 2^22 samples).  WIDE = false: a start (-S) of 4 (RB = 8: 8) payload bytes, aligned to RB but not to 16 bytes.
    # RB = 16 is the barrier K1 of the coherent chain at R = 512 (group of 32 branches)
    row("frbch_k0_stage<8, true>", 32.0, 256, 0.013517, dict(interval=0.006083, maxb=2)),
    row("frbch_k0_stage<8, false>", -32.0, 256, 0.013517, dict(interval=0.006083, maxb=2, start=8 / 32e6)),
    row("frbch_k0_stage<4, true>", 32.0, 256, 0.054068, dict(freq_res=2048, interval=0.024331, maxb=2)),
    row("frbch_k0_stage<4, false>", -32.0, 256, 0.054068, dict(freq_res=2048, interval=0.024331, maxb=2, start=4 / 32e6)),
    row("frbch_k0_stage<2, true>", 32.0, 256, 0.108135, dict(freq_res=4096, interval=0.048661, maxb=2)),
    row("frbch_k0_stage<2, false>", -32.0, 256, 0.108135, dict(freq_res=4096, interval=0.048661, maxb=2, start=4 / 32e6)),
    row("frbch_k0_stage<1, true>", 32.0, 256, 0.216269, dict(freq_res=8192, interval=0.097321, maxb=2)),
    row("frbch_k0_stage<1, false>", -32.0, 256, 0.216269, dict(freq_res=8192, interval=0.097321, maxb=2, start=4 / 32e6)),
    row("frbch_k0_stage<16, true>", 32.0, 256, 0.013517, dict(freq_res=512, **_COH, interval=0.006083, maxb=2)),
    # ---- K1: frbch_k1_wave<L, 8, WPS, STG, COH, MSK> (R = 256 << L).  STG = false: 128 / 16 channels (no K0 below 256);
    # MSK: one frame flagged invalid inside block 1 of 4, blocks 0, 2, 3 clean.  frbch_k1_fast<L>: the coherent chain (R != 4096)
    row("frbch_k1_wave<1, 8, 1, false, false, false>", 16.0, 128, 0.013517, dict(interval=0.006083, maxb=2)),
    row("frbch_k1_wave<1, 8, 1, true, false, false>", -32.0, 256, 0.013517, dict(interval=0.006083, maxb=2)),
    row("frbch_k1_wave<1, 8, 1, true, false, true>", 32.0, 256, 0.017613, dict(interval=0.007926, maxb=2), frames=dict(invalid=[24])),
    row("frbch_k1_wave<2, 8, 1, false, false, false>", -16.0, 128, 0.027034, dict(freq_res=1024, interval=0.012165, maxb=2)),
    row("frbch_k1_wave<2, 8, 1, true, false, false>", 32.0, 256, 0.027034, dict(freq_res=1024, interval=0.012165, maxb=2)),
    row("frbch_k1_wave<2, 8, 1, true, false, true>", -32.0, 256, 0.035226, dict(freq_res=1024, interval=0.015852, maxb=2), frames=dict(invalid=[49])),
    row("frbch_k1_wave<3, 8, 1, false, false, false>", 16.0, 128, 0.054068, dict(freq_res=2048, interval=0.024331, maxb=2)),
    row("frbch_k1_wave<3, 8, 1, true, false, false>", -32.0, 256, 0.054068, dict(freq_res=2048, interval=0.024331, maxb=2)),
    row("frbch_k1_wave<3, 8, 1, true, false, true>", 32.0, 256, 0.070452, dict(freq_res=2048, interval=0.031703, maxb=2), frames=dict(invalid=[98])),
    row("frbch_k1_wave<4, 8, 2, false, false, false>", -16.0, 128, 0.108135, dict(freq_res=4096, interval=0.048661, maxb=2)),
    row("frbch_k1_wave<4, 8, 2, true, false, false>", 32.0, 256, 0.108135, dict(freq_res=4096, interval=0.048661, maxb=2)),
    row("frbch_k1_wave<4, 8, 2, true, false, true>", -32.0, 256, 0.140903, dict(freq_res=4096, interval=0.063406, maxb=2), frames=dict(invalid=[196])),
    row("frbch_k1_wave<5, 8, 4, false, false, false>", 16.0, 128, 0.216269, dict(freq_res=8192, interval=0.097321, maxb=2)),
    row("frbch_k1_wave<5, 8, 4, true, false, false>", -32.0, 256, 0.216269, dict(freq_res=8192, interval=0.097321, maxb=2)),
    row("frbch_k1_wave<5, 8, 4, true, false, true>", 32.0, 256, 0.281805, dict(freq_res=8192, interval=0.126812, maxb=2), frames=dict(invalid=[393])),
    row("frbch_k1_wave<4, 8, 2, false, true, false>", -32.0, 16, 0.006759, dict(freq_res=4096, **_COH, interval=0.003042, maxb=2)),
    row("frbch_k1_wave<4, 8, 2, true, true, false>", 32.0, 256, 0.108135, dict(freq_res=4096, **_COH, interval=0.048661, maxb=2)),
    row("frbch_k1_wave<4, 8, 2, true, true, true>", -32.0, 256, 0.140903, dict(freq_res=4096, **_COH, interval=0.063406, maxb=2), frames=dict(invalid=[196])),
    row("frbch_k1_fast<1>", 32.0, 64, 0.00338, dict(freq_res=512, **_COH, interval=0.001521, maxb=2), also=("frbch_k3_fast<1, 1024>",)),
    row("frbch_k1_fast<2>", -32.0, 64, 0.006759, dict(freq_res=1024, **_COH, interval=0.003042, maxb=2), also=("frbch_k3_fast<2, 1024>",)),
    row("frbch_k1_fast<3>", 32.0, 64, 0.013517, dict(freq_res=2048, **_COH, interval=0.006083, maxb=2), also=("frbch_k3_fast<3, 1024>",)),
    row("frbch_k1_fast<5>", -32.0, 64, 0.054068, dict(freq_res=8192, **_COH, interval=0.024331, maxb=2), also=("frbch_k3_fast<5, 1024>",)),
    # ---- Kc: frbch_kc_fast<L> (2C = 256 << L) behind the R = 512 K1: blocks of 2^18 .. 2^22 samples
    row("frbch_kc_lane", 16.0, 32, 0.003572, dict(interval=0.001607, maxb=2)),
    row("frbch_kc_fast<1>", 32.0, 256, 0.013517, dict(interval=0.006083, maxb=2)),
    row("frbch_kc_fast<2>", -32.0, 512, 0.027034, dict(freq_res=512, interval=0.012165, maxb=2)),
    row("frbch_kc_fast<3>", 32.0, 1024, 0.054068, dict(freq_res=512, interval=0.024331, maxb=2)),
    row("frbch_kc_fast<4>", -32.0, 2048, 0.108135, dict(freq_res=512, interval=0.048661, maxb=2)),
    row("frbch_kc_fast<5>", 32.0, 4096, 0.216269, dict(freq_res=512, interval=0.097321, maxb=2)),
    # ---- K2, a sequence per lane (pair): 32 / 64 channels, blocks of 2^15 / 2^16 samples
    row("frbch_k2_lane<1, 0>", 16.0, 32, 0.003572, dict(pol=1, interval=0.001607, maxb=2)),
    row("frbch_k2_lane<1, 2>", -16.0, 32, 0.003572, dict(nbit=2, interval=0.001607, maxb=2)),
    row("frbch_k2_lane<1, 4>", 16.0, 32, 0.003572, dict(pol=4, nbit=16, interval=0.001607, maxb=2)),
    row("frbch_k2_lane<2, 0>", -16.0, 64, 0.006759, dict(pol=1, nbit=-32, interval=0.003042, maxb=2)),
    row("frbch_k2_lane<2, 2>", 16.0, 64, 0.006759, dict(interval=0.003042, maxb=2)),
    row("frbch_k2_lane<2, 4>", -16.0, 64, 0.006759, dict(pol=4, nbit=2, interval=0.003042, maxb=2)),
    # ---- K2 behind the paired K1 (1024 channels, R = 2048, blocks of 2^22 samples): frbch_k2_priv<PM, MODE>, MODE 0 codes,
    # 1 float rows (-t 4, buffered form: 1 << 27), 2 the statistics pass of the two-pass rescale (automatic with four products,
    # 1 << 28 with one; its digitising pass is MODE 0)
    row("frbch_k2_priv<0, 0>", 32.0, 1024, 0.216269, dict(pol=1, interval=0.097321, maxb=2)),
    row("frbch_k2_priv<0, 1>", -32.0, 1024, 0.216269, dict(pol=1, tscr=4, nbit=2, flags=1 << 27, interval=0.097321, maxb=2)),
    row("frbch_k2_priv<0, 2>", 32.0, 1024, 0.216269, dict(pol=1, nbit=16, flags=1 << 28, interval=0.097321, maxb=2), also=("frbch_k2_priv<0, 0>",)),
    row("frbch_k2_priv<2, 0>", -32.0, 1024, 0.216269, dict(pol=2, nbit=-32, interval=0.097321, maxb=2)),
    row("frbch_k2_priv<2, 1>", 32.0, 1024, 0.216269, dict(pol=2, tscr=4, flags=1 << 27, interval=0.097321, maxb=2)),
    row("frbch_k2_priv<2, 2>", -32.0, 1024, 0.216269, dict(pol=2, nbit=2, flags=1 << 28, interval=0.097321, maxb=2), also=("frbch_k2_priv<2, 0>",)),
    row("frbch_k2_priv<4, 0>", 32.0, 1024, 0.216269, dict(pol=4, nbit=16, flags=1 << 27, interval=0.097321, maxb=2)),
    row("frbch_k2_priv<4, 1>", -32.0, 1024, 0.216269, dict(pol=4, tscr=4, nbit=-32, flags=1 << 27, interval=0.097321, maxb=2)),
    row("frbch_k2_priv<4, 2>", 32.0, 1024, 0.216269, dict(pol=4, interval=0.097321, maxb=2), also=("frbch_k2_priv<4, 0>",)),
    row("frbch_k2_priv<5, 0>", -32.0, 1024, 0.216269, dict(pol=5, nbit=2, flags=1 << 27, interval=0.097321, maxb=2)),
    row("frbch_k2_priv<5, 1>", 32.0, 1024, 0.216269, dict(pol=5, tscr=4, nbit=16, flags=1 << 27, interval=0.097321, maxb=2)),
    row("frbch_k2_priv<5, 2>", -32.0, 1024, 0.216269, dict(pol=5, nbit=-32, interval=0.097321, maxb=2), also=("frbch_k2_priv<5, 0>",)),
    # ---- K2, wave form: frbch_k2_wave<L, NW, PM, WPS, MSTAT> behind the R = 512 K1 (blocks of 2^17 .. 2^21 samples).  NW follows
    # -t: 2, 4 or 8 sequences (x 4 / 2 a wave holds at L = 0 / 1).  L = 3: the four-sequence and the MSTAT = false four-product
    # forms run only where frbch_k2_priv does not (R != 2048); MSTAT = false with four products: separate statistics (1 << 20)
    row("frbch_k2_wave<0, 2, 0, 1, false>", 16.0, 128, 0.013517, dict(pol=1, tscr=8, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<0, 2, 2, 1, false>", -16.0, 128, 0.013517, dict(pol=2, tscr=8, nbit=2, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<0, 2, 4, 1, false>", 16.0, 128, 0.013517, dict(pol=4, tscr=8, nbit=16, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<0, 4, 0, 1, false>", -16.0, 128, 0.013517, dict(pol=1, tscr=16, nbit=-32, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<0, 4, 2, 1, false>", 16.0, 128, 0.013517, dict(pol=2, tscr=16, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<0, 4, 4, 1, false>", -16.0, 128, 0.013517, dict(pol=4, tscr=16, nbit=2, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<0, 8, 0, 1, false>", 16.0, 128, 0.013517, dict(pol=1, tscr=32, nbit=16, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<0, 8, 2, 1, false>", -16.0, 128, 0.013517, dict(pol=2, tscr=32, nbit=-32, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<0, 8, 4, 1, false>", 16.0, 128, 0.013517, dict(pol=4, tscr=32, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<1, 2, 0, 1, false>", -32.0, 256, 0.013517, dict(pol=1, tscr=4, nbit=2, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<1, 2, 2, 1, false>", 32.0, 256, 0.013517, dict(pol=2, tscr=4, nbit=16, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<1, 2, 4, 1, false>", -32.0, 256, 0.013517, dict(pol=4, tscr=4, nbit=-32, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<1, 4, 0, 1, false>", 32.0, 256, 0.013517, dict(pol=1, tscr=8, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<1, 4, 2, 1, false>", -32.0, 256, 0.013517, dict(pol=2, tscr=8, nbit=2, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<1, 4, 4, 1, false>", 32.0, 256, 0.013517, dict(pol=4, tscr=8, nbit=16, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<1, 8, 0, 1, false>", -32.0, 256, 0.013517, dict(pol=1, tscr=16, nbit=-32, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<1, 8, 2, 1, false>", 32.0, 256, 0.013517, dict(pol=2, tscr=16, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<1, 8, 4, 1, false>", -32.0, 256, 0.013517, dict(pol=4, tscr=16, nbit=2, interval=0.006083, maxb=2)),
    row("frbch_k2_wave<2, 2, 0, 1, false>", 32.0, 512, 0.027034, dict(pol=1, tscr=2, nbit=16, freq_res=512, interval=0.012165, maxb=2)),
    row("frbch_k2_wave<2, 2, 2, 1, false>", -32.0, 512, 0.027034, dict(pol=2, tscr=2, nbit=-32, freq_res=512, interval=0.012165, maxb=2)),
    row("frbch_k2_wave<2, 2, 4, 1, false>", 32.0, 512, 0.027034, dict(pol=4, tscr=2, freq_res=512, interval=0.012165, maxb=2)),
    row("frbch_k2_wave<2, 4, 0, 1, false>", -32.0, 512, 0.027034, dict(pol=1, tscr=4, nbit=2, freq_res=512, interval=0.012165, maxb=2)),
    row("frbch_k2_wave<2, 4, 2, 1, false>", 32.0, 512, 0.027034, dict(pol=2, tscr=4, nbit=16, freq_res=512, interval=0.012165, maxb=2)),
    row("frbch_k2_wave<2, 4, 4, 1, false>", -32.0, 512, 0.027034, dict(pol=4, tscr=4, nbit=-32, freq_res=512, interval=0.012165, maxb=2)),
    row("frbch_k2_wave<2, 8, 0, 1, false>", 32.0, 512, 0.027034, dict(pol=1, tscr=8, freq_res=512, interval=0.012165, maxb=2)),
    row("frbch_k2_wave<2, 8, 2, 1, false>", -32.0, 512, 0.027034, dict(pol=2, tscr=8, nbit=2, freq_res=512, interval=0.012165, maxb=2)),
    row("frbch_k2_wave<2, 8, 4, 1, false>", 32.0, 512, 0.027034, dict(pol=4, tscr=8, nbit=16, freq_res=512, interval=0.012165, maxb=2)),
    row("frbch_k2_wave<3, 4, 0, 2, false>", -32.0, 1024, 0.054068, dict(pol=1, tscr=2, nbit=-32, freq_res=512, interval=0.024331, maxb=2)),
    row("frbch_k2_wave<3, 4, 2, 2, false>", 32.0, 1024, 0.054068, dict(pol=2, tscr=2, freq_res=512, interval=0.024331, maxb=2)),
    row("frbch_k2_wave<3, 4, 4, 2, false>", -32.0, 1024, 0.054068, dict(pol=4, tscr=2, nbit=2, freq_res=512, flags=1 << 20, interval=0.024331, maxb=2)),
    row("frbch_k2_wave<3, 4, 4, 2, true>", 32.0, 1024, 0.054068, dict(pol=5, tscr=2, nbit=16, freq_res=512, interval=0.024331, maxb=2)),
    row("frbch_k2_wave<3, 8, 0, 2, false>", -32.0, 1024, 0.054068, dict(pol=1, tscr=4, nbit=-32, freq_res=512, interval=0.024331, maxb=2)),
    row("frbch_k2_wave<3, 8, 2, 2, false>", 32.0, 1024, 0.054068, dict(pol=2, tscr=4, freq_res=512, interval=0.024331, maxb=2)),
    row("frbch_k2_wave<3, 8, 4, 2, false>", -32.0, 1024, 0.054068, dict(pol=4, tscr=4, nbit=2, freq_res=512, flags=1 << 20, interval=0.024331, maxb=2)),
    row("frbch_k2_wave<3, 8, 4, 2, true>", 32.0, 1024, 0.054068, dict(pol=5, tscr=4, nbit=16, freq_res=512, interval=0.024331, maxb=2)),
    row("frbch_k2_wave<3, 8, 0, 1, false>", -32.0, 1024, 0.054068, dict(pol=1, tscr=8, nbit=-32, freq_res=512, interval=0.024331, maxb=2)),
    row("frbch_k2_wave<3, 8, 2, 1, false>", 32.0, 1024, 0.054068, dict(pol=2, tscr=8, freq_res=512, interval=0.024331, maxb=2)),
    row("frbch_k2_wave<3, 8, 4, 1, false>", -32.0, 1024, 0.054068, dict(pol=4, tscr=8, nbit=2, freq_res=512, interval=0.024331, maxb=2)),
    row("frbch_k2_wave<4, 8, 0, 2, false>", 32.0, 2048, 0.108135, dict(pol=1, tscr=4, nbit=16, freq_res=512, interval=0.048661, maxb=2)),
    row("frbch_k2_wave<4, 8, 2, 2, false>", -32.0, 2048, 0.108135, dict(pol=2, tscr=4, nbit=-32, freq_res=512, interval=0.048661, maxb=2)),
    row("frbch_k2_wave<4, 8, 4, 2, false>", 32.0, 2048, 0.108135, dict(pol=4, tscr=2, freq_res=512, interval=0.048661, maxb=2)),
    # ---- K2, barrier form (2C = 8192 behind any K1 but the R = 8192 one: R = 512, blocks of 2^22 samples)
    row("frbch_k2_fast<5, 512>", 32.0, 4096, 0.216269, dict(freq_res=512, interval=0.097321, maxb=2)),
    row("frbch_k2_fast<5, 1024>", -32.0, 4096, 0.216269, dict(pol=2, tscr=2, nbit=2, freq_res=512, interval=0.097321, maxb=2)),
    row("frbch_k2_fast<5, 512>", 32.0, 4096, 0.216269, dict(nbit=16, freq_res=512, interval=0.097321, maxb=2)),
    row("frbch_k2_fast<5, 1024>", -32.0, 4096, 0.216269, dict(pol=4, tscr=2, nbit=-32, freq_res=512, interval=0.097321, maxb=2)),
    # ---- two-stage tscrunch: the wave K2 at its largest tile + frbch_k2_scrunch
    row("frbch_k2_scrunch", 16.0, 128, 0.013517, dict(tscr=64, interval=0.006083, maxb=2)),
    row("frbch_k2_scrunch", -32.0, 1024, 0.216269, dict(pol=4, tscr=16, nbit=2, interval=0.097321, maxb=2)),
    row("frbch_k2_scrunch", 32.0, 2048, 0.108135, dict(tscr=8, nbit=16, freq_res=512, interval=0.048661, maxb=2)),
    row("frbch_k2_scrunch", -32.0, 256, 0.013517, dict(pol=5, tscr=32, nbit=-32, interval=0.006083, maxb=2)),
    # ---- coherent chain: frbch_k2c_fast<L, 1024> (2C = 256 << L, R = 512), frbch_k3_fast<L, 1024> / frbch_k3_wave<4> (R = 256 << L,
    # 64 channels), frbch_k4_fast
    row("frbch_k2c_fast<1, 1024>", 32.0, 256, 0.013517, dict(freq_res=512, **_COH, interval=0.006083, maxb=2)),
    row("frbch_k2c_fast<2, 1024>", -32.0, 512, 0.027034, dict(freq_res=512, **_COH, interval=0.012165, maxb=2)),
    row("frbch_k2c_fast<3, 1024>", 32.0, 1024, 0.054068, dict(freq_res=512, **_COH, interval=0.024331, maxb=2)),
    row("frbch_k2c_fast<4, 1024>", -32.0, 2048, 0.108135, dict(freq_res=512, **_COH, interval=0.048661, maxb=2)),
    row("frbch_k2c_fast<5, 1024>", 32.0, 4096, 0.216269, dict(freq_res=512, **_COH, interval=0.097321, maxb=2)),
    row("frbch_k3_fast<1, 1024>", 32.0, 64, 0.00338, dict(pol=5, tscr=2, freq_res=512, **_COH, interval=0.001521, maxb=2)),
    row("frbch_k3_fast<2, 1024>", -32.0, 64, 0.006759, dict(pol=5, tscr=2, freq_res=1024, **_COH, interval=0.003042, maxb=2)),
    row("frbch_k3_fast<3, 1024>", 32.0, 64, 0.013517, dict(pol=5, tscr=2, freq_res=2048, **_COH, interval=0.006083, maxb=2)),
    row("frbch_k3_fast<5, 1024>", -32.0, 64, 0.054068, dict(pol=5, tscr=2, freq_res=8192, **_COH, interval=0.024331, maxb=2)),
    row("frbch_k3_wave<4>", 32.0, 64, 0.027034, dict(pol=2, tscr=1, freq_res=4096, **_COH, interval=0.012165, maxb=2)),
    row("frbch_k3_wave<4>", -32.0, 64, 0.027034, dict(pol=5, tscr=2, nbit=2, freq_res=4096, **_COH, interval=0.012165, maxb=2)),
    row("frbch_k3_wave<4>", 32.0, 64, 0.027034, dict(pol=0, tscr=4, nbit=16, freq_res=4096, **_COH, interval=0.012165, maxb=2)),
    row("frbch_k3_wave<4>", -32.0, 64, 0.027034, dict(pol=4, tscr=1, nbit=-32, freq_res=4096, **_COH, interval=0.012165, maxb=2)),
    row("frbch_k4_fast", 32.0, 64, 0.006759, dict(pol=2, tscr=1, freq_res=1024, **_COH, interval=0.003042, maxb=2)),
    row("frbch_k4_fast", -32.0, 64, 0.006759, dict(pol=5, tscr=1, nbit=2, freq_res=1024, **_COH, interval=0.003042, maxb=2)),
    row("frbch_k4_fast", 32.0, 64, 0.006759, dict(pol=1, tscr=1, nbit=16, freq_res=1024, **_COH, interval=0.003042, maxb=2)),
    row("frbch_k4_fast", -32.0, 64, 0.006759, dict(pol=4, tscr=1, nbit=-32, freq_res=1024, **_COH, interval=0.003042, maxb=2)),
    # ---- digitiser
    row("frbch_quantise_fast<8, 256>", 16.0, 128, 0.013517, dict(interval=0.006083, maxb=2)),
    # ---- every K1 layout group (R = 512: 16 branches, 1024 / 2048: 8, 4096: 4, 8192: 2, and the generic K1, flags = 1) in front of
    # every K2 family and LOG2M, blocks up to 2^23 samples (PAIRINGS_LEFT_OUT below)
    row("frbch_k2_lane<1, 2>", 16.0, 32, 0.003572, dict(nbit=16, interval=0.001607, maxb=2), also=("frbch_k1_wave<1, 8, 1, false, false, false>",)),
    row("frbch_k2_lane<1, 2>", -16.0, 32, 0.003572, dict(nbit=-32, flags=1, interval=0.001607, maxb=2), also=("frbch_k1_branch",)),
    row("frbch_k2_lane<2, 2>", 16.0, 64, 0.006759, dict(interval=0.003042, maxb=2), also=("frbch_k1_wave<1, 8, 1, false, false, false>",)),
    row("frbch_k2_lane<2, 2>", -16.0, 64, 0.006759, dict(nbit=2, flags=1, interval=0.003042, maxb=2), also=("frbch_k1_branch",)),
    row("frbch_k2_wave<0, 2, 2, 1, false>", -16.0, 128, 0.013517, dict(nbit=2, interval=0.006083, maxb=2), also=("frbch_k1_wave<1, 8, 1, false, false, false>",)),
    row("frbch_k2_wave<0, 2, 2, 1, false>", 16.0, 128, 0.027034, dict(nbit=16, freq_res=1024, interval=0.012165, maxb=2), also=("frbch_k1_wave<2, 8, 1, false, false, false>",)),
    row("frbch_k2_wave<0, 2, 2, 1, false>", -16.0, 128, 0.054068, dict(nbit=-32, freq_res=2048, interval=0.024331, maxb=2), also=("frbch_k1_wave<3, 8, 1, false, false, false>",)),
    row("frbch_k2_wave<0, 2, 2, 1, false>", 16.0, 128, 0.108135, dict(freq_res=4096, interval=0.048661, maxb=2), also=("frbch_k1_wave<4, 8, 2, false, false, false>",)),
    row("frbch_k2_wave<0, 2, 2, 1, false>", -16.0, 128, 0.216269, dict(nbit=2, freq_res=8192, interval=0.097321, maxb=2), also=("frbch_k1_wave<5, 8, 4, false, false, false>",)),
    row("frbch_k2_wave<0, 2, 2, 1, false>", 16.0, 128, 0.013517, dict(nbit=16, flags=1, interval=0.006083, maxb=2), also=("frbch_k1_branch",)),
    row("frbch_k2_wave<1, 2, 2, 1, false>", -32.0, 256, 0.013517, dict(nbit=-32, interval=0.006083, maxb=2), also=("frbch_k1_wave<1, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<1, 2, 2, 1, false>", 32.0, 256, 0.027034, dict(freq_res=1024, interval=0.012165, maxb=2), also=("frbch_k1_wave<2, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<1, 2, 2, 1, false>", -32.0, 256, 0.054068, dict(nbit=2, freq_res=2048, interval=0.024331, maxb=2), also=("frbch_k1_wave<3, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<1, 2, 2, 1, false>", 32.0, 256, 0.108135, dict(nbit=16, freq_res=4096, interval=0.048661, maxb=2), also=("frbch_k1_wave<4, 8, 2, true, false, false>",)),
    row("frbch_k2_wave<1, 2, 2, 1, false>", -32.0, 256, 0.216269, dict(nbit=-32, freq_res=8192, interval=0.097321, maxb=2), also=("frbch_k1_wave<5, 8, 4, true, false, false>",)),
    row("frbch_k2_wave<1, 2, 2, 1, false>", 32.0, 256, 0.013517, dict(flags=1, interval=0.006083, maxb=2), also=("frbch_k1_branch",)),
    row("frbch_k2_wave<2, 2, 2, 1, false>", -32.0, 512, 0.027034, dict(nbit=2, freq_res=512, interval=0.012165, maxb=2), also=("frbch_k1_wave<1, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<2, 2, 2, 1, false>", 32.0, 512, 0.054068, dict(nbit=16, interval=0.024331, maxb=2), also=("frbch_k1_wave<2, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<2, 2, 2, 1, false>", -32.0, 512, 0.108135, dict(nbit=-32, freq_res=2048, interval=0.048661, maxb=2), also=("frbch_k1_wave<3, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<2, 2, 2, 1, false>", 32.0, 512, 0.216269, dict(freq_res=4096, interval=0.097321, maxb=2), also=("frbch_k1_wave<4, 8, 2, true, false, false>",)),
    row("frbch_k2_wave<2, 2, 2, 1, false>", -32.0, 512, 0.432538, dict(nbit=2, freq_res=8192, interval=0.194642, maxb=2), also=("frbch_k1_wave<5, 8, 4, true, false, false>",)),
    row("frbch_k2_wave<2, 2, 2, 1, false>", 32.0, 512, 0.027034, dict(nbit=16, freq_res=512, flags=1, interval=0.012165, maxb=2), also=("frbch_k1_branch",)),
    row("frbch_k2_wave<3, 4, 2, 2, false>", -32.0, 1024, 0.054068, dict(nbit=-32, freq_res=512, interval=0.024331, maxb=2), also=("frbch_k1_wave<1, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<3, 4, 2, 2, false>", 32.0, 1024, 0.108135, dict(freq_res=1024, interval=0.048661, maxb=2), also=("frbch_k1_wave<2, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<3, 4, 2, 2, false>", -32.0, 1024, 0.216269, dict(nbit=2, interval=0.097321, maxb=2), also=("frbch_k1_wave<3, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<3, 4, 2, 2, false>", 32.0, 1024, 0.432538, dict(nbit=16, freq_res=4096, interval=0.194642, maxb=2), also=("frbch_k1_wave<4, 8, 2, true, false, false>",)),
    row("frbch_k2_wave<3, 4, 2, 2, false>", -32.0, 1024, 0.054068, dict(nbit=-32, freq_res=512, flags=1, interval=0.024331, maxb=2), also=("frbch_k1_branch",)),
    row("frbch_k2_wave<4, 8, 2, 2, false>", 32.0, 2048, 0.108135, dict(freq_res=512, interval=0.048661, maxb=2), also=("frbch_k1_wave<1, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<4, 8, 2, 2, false>", -32.0, 2048, 0.216269, dict(nbit=2, freq_res=1024, interval=0.097321, maxb=2), also=("frbch_k1_wave<2, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<4, 8, 2, 2, false>", 32.0, 2048, 0.432538, dict(nbit=16, freq_res=2048, interval=0.194642, maxb=2), also=("frbch_k1_wave<3, 8, 1, true, false, false>",)),
    row("frbch_k2_wave<4, 8, 2, 2, false>", -32.0, 2048, 0.108135, dict(nbit=-32, freq_res=512, flags=1, interval=0.048661, maxb=2), also=("frbch_k1_branch",)),
    row("frbch_k2_fast<5, 512>", 32.0, 4096, 0.216269, dict(freq_res=512, interval=0.097321, maxb=2), also=("frbch_k1_wave<1, 8, 1, true, false, false>",)),
    row("frbch_k2_fast<5, 512>", -32.0, 4096, 0.432538, dict(nbit=2, freq_res=1024, interval=0.194642, maxb=2), also=("frbch_k1_wave<2, 8, 1, true, false, false>",)),
    row("frbch_k2_fast<5, 512>", 32.0, 4096, 0.216269, dict(nbit=16, freq_res=512, flags=1, interval=0.097321, maxb=2), also=("frbch_k1_branch",)),
    # ---- more than one trip of every persistent loop, workgroups making different numbers of trips (grids for the 256 CUs of an
    # MI355X).  128 channels, R = 512: a block is 2^17 samples.
    # frbch_k2_wave: a tile = 2 waves x 4 sequences, 512 / 8 = 64 tiles per block; -I0 digitises from the first block, no sums:
    # the cap is 8192 workgroups; one launch of 131 blocks = 8384 tiles: 192 workgroups make two trips, 8000 one
    row("frbch_k2_wave<0, 2, 2, 1, false>", 16.0, 128, 0.5378, dict(interval=0.0, maxb=131), grid_x=8192),
    # frbch_k1_wave: 16 branch groups x ny, ny = min(blocks, 2 x 256 resident / 16) = 32; 100 blocks in launches of 34, 34, 32:
    # block slots 0 and 1 of 32 make two trips, the others one
    row("frbch_k1_wave<1, 8, 1, false, false, false>", -16.0, 128, 0.4109, dict(interval=0.18, maxb=40), grid_y=32),
    # frbch_k2_priv: 2 x 256 workgroups, R / 4 = 512 tiles per block: every launch of nb blocks is nb trips for all of them (a
    # launch cannot make their trips unequal on 256 CUs); the three-block launch here: three trips each
    row("frbch_k2_priv<2, 0>", 32.0, 1024, 0.216269, dict(interval=0.0, maxb=3), grid_x=512),
    # frbch_k3_wave: 2048 workgroups over blocks x channels tiles: 9 blocks of 256 channels = 2304 tiles, 256 workgroups make two
    # trips; frbch_k2c_fast on the same run: 4096 / 32 = 128 position tiles x gy, gy = min(9, 4 x 256 / 128) = 8: block slot 0 two trips
    row("frbch_k3_wave<4>", 32.0, 256, 0.3048, dict(freq_res=4096, maxb=9, **_COH), grid_x=2048),
    row("frbch_k2c_fast<1, 1024>", 32.0, 256, 0.3048, dict(freq_res=4096, maxb=9, **_COH), grid_y=8),
    # ---- the digitiser holding CUs beside the next IF's K1: two IFs through frbch_scan_device, each IF's columns against the oracle
    # (two blocks per IF, one per launch; the interval ends inside the first, its digitiser runs beside the front stage that follows)
    row("frbch_quantise_fast<8, 512>", 32.0, 1024, 0.15, dict(pol=5, interval=0.05, maxb=1, flags=1 << 27), kind="scan"),
    # ---- the unpack tap's register decoder: every byte value (as tests/test_gpu_pins.py::test_unpack_tap_all_byte_values)
    row("frbch_unpack_tap_fast", kind="tap"),
    # ---- 2C = R = 8192, blocks of 2^26 samples: rows that point at CASES entries of tests/test_gpu_parity.py
    row("frbch_k2_wave<5, 8, 2, 4, true>", kind="case", case=(-64.0, 4096, 0.55, {})),
    row("frbch_k2_wave<5, 8, 0, 4, true>", kind="case", case=(64.0, 4096, 0.55, dict(pol=1, nbit=16))),
    row("frbch_k2_wave<5, 8, 2, 4, false>", kind="case", case=(-64.0, 4096, 0.55, dict(tscr=4, nbit=2)), also=("frbch_k2_scrunch",)),
    row("frbch_k2_wave<5, 8, 0, 4, false>", kind="case", case=(64.0, 4096, 0.55, dict(pol=3, nbit=2))),
]

# pairings of a K1 layout group with a K2 family left out for size (blocks above 2^23 samples)
PAIRINGS_LEFT_OUT = [
    ("frbch_k2_wave<3, ...>", "R = 8192 (2^24)"),
    ("frbch_k2_wave<4, ...>", "R = 4096 (2^24), R = 8192 (2^25)"),
    ("frbch_k2_wave<5, ...>", "R = 8192 only (2^26): the CASES rows above"),
    ("frbch_k2_fast<5, ...>", "R = 2048 (2^24), R = 4096 (2^25)"),
]

# the generic kernels of frbch_launch.cpp (extern "C": listed without template or parameter list)
GENERIC = {
    "frbch_chirp_build", "frbch_dls_count", "frbch_k1_branch", "frbch_k2_chan", "frbch_k2c_chirp", "frbch_k3_dedisp", "frbch_k4_out",
    "frbch_kc_dcfix", "frbch_quantise", "frbch_stats_final", "frbch_stats_partial", "frbch_unpack_tap",
}

# families that emit codes: every one runs at nbit 2, 8, 16 and -32 and in both band senses somewhere in ROWS
CODE_FAMILIES = ("frbch_k2_wave", "frbch_k2_priv", "frbch_k2_lane", "frbch_k2_fast", "frbch_k2_scrunch", "frbch_k3_wave", "frbch_k4_fast")

# the generic kernel of each register-pass family's stage: a row's run must not launch it (a silent fallback)
STAGE_GENERIC = {
    "frbch_k0_stage": "frbch_k1_branch", "frbch_k1_wave": "frbch_k1_branch", "frbch_k1_fast": "frbch_k1_branch",
    "frbch_kc_fast": "frbch_kc_dcfix", "frbch_kc_lane": "frbch_kc_dcfix",
    "frbch_k2_wave": "frbch_k2_chan", "frbch_k2_priv": "frbch_k2_chan", "frbch_k2_lane": "frbch_k2_chan",
    "frbch_k2_fast": "frbch_k2_chan", "frbch_k2_scrunch": "frbch_k2_chan",
    "frbch_k2c_fast": "frbch_k2c_chirp", "frbch_k3_fast": "frbch_k3_dedisp", "frbch_k3_wave": "frbch_k3_dedisp",
    "frbch_k4_fast": "frbch_k4_out", "frbch_quantise_fast": "frbch_quantise", "frbch_unpack_tap_fast": None,
}


def family(name):
    return name.split("<")[0]


def case_kernels(bw, nchan, secs, kw):
    """kernels the table asserts on the CASES entry (bw, nchan, secs, kw) of tests/test_gpu_parity.py"""
    return [n for r in ROWS if r.kind == "case" and r.case == (bw, nchan, secs, kw) for n in (r.name,) + r.also]
