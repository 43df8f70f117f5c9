# oracle/hd_pipelined.mk — the Gloo-side program of the pipelined
# halving-doubling bridge case (tests/bridge/hd_pipelined_test.cc), built like
# bridge_test: against the reference's own headers and objects (the variables
# and object rules of oracle/Makefile) and libgloo_amd.so's C-ABI.
#   make -C oracle -f hd_pipelined.mk hd_pipelined
# builds _ref/hd_pipelined_test where the reference is present, else nothing.
include Makefile

.PHONY: hd_pipelined
hd_pipelined: $(if $(wildcard $(REF)/gloo/math.h),$(OUT)/hd_pipelined_test,)

$(OUT)/hd_pipelined_test: ../tests/bridge/hd_pipelined_test.cc ../gloo_amd/include/gloo_amd/gloo_bridge.h \
		../include/gloo_amd.h $(REF_OBJS) ../gloo_amd/libgloo_amd.so
	$(CXX) -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -I$(REF) -I../include -I../gloo_amd/include -w \
	  ../tests/bridge/hd_pipelined_test.cc $(REF_OBJS) -o $@ -L../gloo_amd -lgloo_amd -L$(ROCM)/lib -lamdhip64 \
	  -Wl,-rpath,'$$ORIGIN/../../gloo_amd' -Wl,-rpath,$(ROCM)/lib -pthread
