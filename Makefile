# Builds the product library (gfx950 only) and the CPU oracle (test infrastructure).
HIPCC ?= hipcc
ARCH ?= gfx950
# -ffp-contract=off: the arithmetic contract forbids fused multiply-add,
# so correspondence indices are bit-identical to the oracle's.
HIPFLAGS = --offload-arch=$(ARCH) -O3 -ffp-contract=off -fPIC -std=c++17 -Iinclude -Ipgslam_amd/csrc -Wall -Wno-unused-result
CSRC = pgslam_amd/csrc
LIB = pgslam_amd/lib/libpgicp.so
OBJS = $(CSRC)/kernels.o $(CSRC)/pgicp_api.o $(CSRC)/pgicp_comm.o

all: $(LIB) oracle

$(CSRC)/kernels.o: $(CSRC)/kernels.hip $(wildcard $(CSRC)/k_*.inc) $(CSRC)/kernels.hpp $(CSRC)/tile_map.hpp $(CSRC)/device_types.hpp $(CSRC)/icp_math.hpp include/pgslam_amd/octree_host.hpp include/pgslam_amd/elipsoids_host.hpp include/pgicp_sensor_chain.h include/pgslam_amd/sensor_chain_host.hpp include/pgicp_descriptor_filters.h include/pgslam_amd/descriptor_filters_host.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/pgicp_api.o: $(CSRC)/pgicp_api.cpp $(wildcard $(CSRC)/api_*.inc) $(CSRC)/kernels.hpp $(CSRC)/seed_source.hpp $(CSRC)/device_types.hpp $(CSRC)/icp_math.hpp include/pgicp.h include/pgicp_noise.h include/pgicp_vardist.h include/pgicp_robust.h include/pgicp_density.h include/pgicp_covsample.h include/pgslam_amd/covsample_host.hpp include/pgicp_octree.h include/pgslam_amd/octree_host.hpp include/pgicp_normalspace.h include/pgslam_amd/normalspace_host.hpp include/pgicp_normals_ext.h include/pgicp_quantile.h include/pgicp_ssn_ext.h include/pgicp_elipsoids.h include/pgslam_amd/elipsoids_host.hpp include/pgicp_sensor_chain.h include/pgslam_amd/sensor_chain_host.hpp include/pgicp_descriptor_filters.h include/pgslam_amd/descriptor_filters_host.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/pgicp_comm.o: $(CSRC)/pgicp_comm.cpp include/pgicp.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(LIB): $(OBJS)
	@mkdir -p pgslam_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -ldl -pthread

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(OBJS) $(LIB)
	$(MAKE) -C oracle clean

# the C++ tests of RobustOutlierFilter's settings (include/pgicp_robust.h); tests/test_cpp_robust_ext.py builds them the same way
CPPTEST = g++ -std=c++17 -O1 -Wall -Wno-unused-local-typedefs -Wno-unused-variable -pthread -Iinclude
CPPLINK = -Lpgslam_amd/lib -lpgicp -Wl,-rpath,$(CURDIR)/pgslam_amd/lib -Wl,-rpath,/opt/rocm/lib
tests/cpp/test_robust_ext_cpu tests/cpp/test_robust_ext_gpu: tests/cpp/%: tests/cpp/%.cpp tests/cpp/common.hpp $(wildcard include/pgslam_amd/*.hpp) include/pgicp_robust.h $(LIB)
	$(CPPTEST) $< -o $@ $(CPPLINK)
robust-ext-tests: tests/cpp/test_robust_ext_cpu tests/cpp/test_robust_ext_gpu

.PHONY: all oracle clean robust-ext-tests
