# Builds the MI355X linearization library and (optionally) the test-only oracle.
#
#   make            -> moptimizer_0_amd/lib/libmoptimizer_hip.so   (gfx950 code object + C ABI)
#   make oracle     -> oracle/_build/{liboracle.so,replay_reference_tests}   (CPU checker)
#   make cpptests   -> tests/cpp/_build/*                           (C++ drop-in programs)
#
# hipcc cross-compiles for gfx950 without a GPU present.
HIPCC      ?= /opt/rocm/bin/hipcc
ARCH       ?= gfx950
ROCM       ?= /opt/rocm
HIPFLAGS   ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function
INCLUDES    = -Iinclude -Imoptimizer_0_amd/csrc
CSRC        = moptimizer_0_amd/csrc
OBJDIR      = build/obj
LIBDIR      = moptimizer_0_amd/lib
LIB         = $(LIBDIR)/libmoptimizer_hip.so

PUBLIC_HEADERS = include/moptimizer_hip.h include/moptimizer_amd/so3.hpp $(CSRC)/sweep.hpp $(CSRC)/fd_device.hpp \
                 $(CSRC)/sweep_device.hpp $(CSRC)/jit_model.hpp $(CSRC)/cost_state.hpp $(CSRC)/lm_device.hpp $(CSRC)/aql.hpp \
                 $(CSRC)/dispatch.hpp $(CSRC)/sweep_choice.hpp $(CSRC)/publish_device.hpp $(CSRC)/normals_device.hpp \
                 $(CSRC)/cell_order.hpp $(CSRC)/cell_lattice.hpp

all: $(LIB)

$(OBJDIR) $(LIBDIR):
	mkdir -p $@

# One code object per device unit; the host units are compiled as HIP too.
DEVICE_UNITS = sweep_kernels finalize_kernels icp_match layout_kernels fd_kernels cell_order lm_kernels cloud_voxel cloud_normals
HOST_UNITS   = c_abi cost sweep_launch blocking resident icp group aql jit_model device_pool combine lm batch cloud
OBJS         = $(DEVICE_UNITS:%=$(OBJDIR)/%.o) $(HOST_UNITS:%=$(OBJDIR)/%.o)

# leading scalar kernel arguments preloaded into SGPRs at wave launch (gfx940+): the sweeps and what
# shares their argument conventions; cell_order, lm_kernels, cloud_voxel and cloud_normals are built without it
PRELOAD = -mllvm -amdgpu-kernarg-preload-count=4
$(OBJDIR)/sweep_kernels.o $(OBJDIR)/finalize_kernels.o $(OBJDIR)/icp_match.o $(OBJDIR)/layout_kernels.o: UNITFLAGS = $(PRELOAD)
# forward-difference sweeps: without the SLP vectorizer (fd_kernels.hip says why)
$(OBJDIR)/fd_kernels.o: UNITFLAGS = $(PRELOAD) -fno-slp-vectorize

$(OBJDIR)/%.o: $(CSRC)/%.hip $(PUBLIC_HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(INCLUDES) $(UNITFLAGS) -c $< -o $@

$(OBJDIR)/%.o: $(CSRC)/%.cpp $(PUBLIC_HEADERS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(INCLUDES) -x hip -c $< -o $@

# the list scripts/check_spills.py checks
print-device-units:
	@echo $(DEVICE_UNITS)

$(LIB): $(OBJS) | $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -L$(ROCM)/lib -lrccl -lhiprtc -lhsa-runtime64 -lpthread -lrt \
	    -Wl,-rpath,$(ROCM)/lib -Wl,--no-undefined

oracle:
	$(MAKE) -C oracle all

cpptests: $(LIB)
	$(MAKE) -C tests/cpp all

clean:
	rm -rf build $(LIBDIR) tests/cpp/_build
	$(MAKE) -C oracle clean

.PHONY: all oracle cpptests clean print-device-units
