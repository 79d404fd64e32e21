# TEST INFRASTRUCTURE ONLY: the fold refinement (frbch_foldfit_kernel / _host / _peaks / _steps, frbch_fold_refine_host, the
# refusals, a failure walk) under AddressSanitizer and UBSan, as a stand-alone program linked against the emulator sources (CPU
# only; never loaded into python, never run on a GPU).
#   make -C tests/sanitize -f foldfit.mk run
CSRC := ../../frb_baseband_amd/csrc
EMU := ../emu
CXX ?= g++
UNITS := $(CSRC)/frbch_launch.cpp $(CSRC)/frbch_stream.cpp $(CSRC)/frbch_api.cpp $(CSRC)/frbch_file.cpp $(CSRC)/frbch_post.cpp $(CSRC)/frbch_host.cpp $(EMU)/emu_hooks.cpp
FLAGS := -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -fopenmp -ffp-contract=off -std=c++17 -Wall \
         -Wno-unused-function -DFRBCH_DEV_HEADER='"dev_emu.h"' -DFRBCH_TEST_HOOKS -I$(EMU) -I$(CSRC) -I../../include
foldfit_sanitize: foldfit_main.cpp $(UNITS) $(CSRC)/kernels_post.inc $(EMU)/dev_emu.h ../../include/frbch.h
	$(CXX) $(FLAGS) foldfit_main.cpp $(UNITS) -o $@ -pthread
run: foldfit_sanitize
	ASAN_OPTIONS=detect_leaks=1 ./foldfit_sanitize
