# TEST INFRASTRUCTURE ONLY: the burst polarisation stage and the polarisation calibration, which share one host path
# (frbch_burstspec_*, frbch_rm_table, frbch_rmsynth_* / frbch_rmdelay_*, frbch_rm_peaks / frbch_rmdelay_peaks, frbch_burst_rm_host /
# frbch_burst_polcal_host, the refusals, the failure walks) under AddressSanitizer and UBSan, as a stand-alone program linked
# against the emulator sources (CPU only; never loaded into python, never run on a GPU).
#   make -C tests/sanitize -f rm.mk run
CSRC := ../../frb_baseband_amd/csrc
EMU := ../emu
CXX ?= g++
UNITS := $(CSRC)/frbch_launch.cpp $(CSRC)/frbch_stream.cpp $(CSRC)/frbch_api.cpp $(CSRC)/frbch_file.cpp $(CSRC)/frbch_post.cpp $(CSRC)/frbch_host.cpp $(EMU)/emu_hooks.cpp
FLAGS := -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -fopenmp -ffp-contract=off -std=c++17 -Wall \
         -Wno-unused-function -DFRBCH_DEV_HEADER='"dev_emu.h"' -DFRBCH_TEST_HOOKS -I$(EMU) -I$(CSRC) -I../../include
rm_sanitize: rm_main.cpp $(UNITS) $(CSRC)/kernels_post.inc $(EMU)/dev_emu.h ../../include/frbch.h
	$(CXX) $(FLAGS) rm_main.cpp $(UNITS) -o $@ -pthread
run: rm_sanitize
	ASAN_OPTIONS=detect_leaks=1 ./rm_sanitize
