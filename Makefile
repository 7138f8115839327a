# Top-level build: the product library (HIP, gfx950) and the parity checkers (oracle/).
#
#   make            -> gr-fosphor_amd/libfosphor_amd.so  (hipcc cross-compiles without a GPU)
#   make oracle     -> oracle/libfosphor_oracle.so, oracle/pm_check   (gcc)
#   make ref        -> oracle/_ref/libfosphor_ref.so (needs /root/reference)
#
# -ffp-contract=off is part of the numerical contract: the FFT must round
# exactly where the reference's expressions round.

HIPCC   ?= hipcc
ARCH    ?= gfx950
CSRC    := gr-fosphor_amd/csrc
LIB     := gr-fosphor_amd/libfosphor_amd.so
HIPFLAGS := --offload-arch=$(ARCH) -O3 -ffp-contract=off -std=c++17 -fPIC -pthread -Wall -Wno-unused-function

SRCS := $(CSRC)/fosphor_kernels.hip $(CSRC)/fosphor_cmap.hip $(CSRC)/fosphor_view.hip $(CSRC)/fosphor_detect.hip $(CSRC)/fosphor_mask.hip $(CSRC)/fosphor_burst.hip $(CSRC)/fosphor_extract.hip $(CSRC)/fosphor_measure.hip $(CSRC)/fosphor_demod.hip $(CSRC)/fosphor_correlate.hip $(CSRC)/fosphor_resample.hip $(CSRC)/fosphor_psd.hip $(CSRC)/fosphor_symbols.hip $(CSRC)/fosphor_carrier.hip $(CSRC)/fosphor_decide.hip $(CSRC)/fosphor_decode.hip $(CSRC)/fosphor_soft.hip $(CSRC)/fosphor_rs.hip $(CSRC)/fosphor_rs_host.cpp $(CSRC)/fosphor_wire.hip $(CSRC)/fosphor_api.cpp $(CSRC)/fosphor_shard.cpp $(CSRC)/fosphor_prof.cpp $(CSRC)/fosphor_tables.cpp $(CSRC)/fosphor_render.cpp $(CSRC)/fosphor_sink.cpp $(CSRC)/fosphor_exchange.cpp
HDRS := $(wildcard $(CSRC)/*.inc) $(CSRC)/fosphor_internal.h $(CSRC)/fosphor_instance.h $(CSRC)/fosphor_jobs.h $(CSRC)/fosphor_pass.h $(CSRC)/fosphor_ring.h $(CSRC)/fosphor_trellis.h $(CSRC)/fosphor_rs.h $(CSRC)/fosphor_cmap_dev.h include/fosphor.h include/fosphor_amd.h include/fosphor_amd_sink.h include/fosphor_amd_cmap.h include/fosphor_amd_view.h include/fosphor_amd_detect.h include/fosphor_amd_mask.h include/fosphor_amd_burst.h include/fosphor_amd_extract.h include/fosphor_amd_measure.h include/fosphor_amd_demod.h include/fosphor_amd_correlate.h include/fosphor_amd_resample.h include/fosphor_amd_psd.h include/fosphor_amd_symbols.h include/fosphor_amd_carrier.h include/fosphor_amd_decide.h include/fosphor_amd_decode.h include/fosphor_amd_soft.h include/fosphor_amd_rs.h include/fosphor_amd_wire.h include/fosphor_amd_axis.h include/fosphor_portable_math.h

all: $(LIB)

$(LIB): $(SRCS) $(HDRS) Makefile
	$(HIPCC) $(HIPFLAGS) -x hip -shared -o $@ $(SRCS) -ldl

oracle:
	$(MAKE) -C oracle all

ref:
	$(MAKE) -C oracle ref

clean:
	rm -f $(LIB)
	$(MAKE) -C oracle clean

.PHONY: all oracle ref clean
