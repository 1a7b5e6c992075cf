# Builds libgulon_hip.so (gfx950 only) and the CPU oracle.
# -ffp-contract=off: every kernel reproduces the JVM's unfused binary32 arithmetic;
# the only fused arithmetic in the library is the explicit MFMA in the k-means filter.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC = gulon_amd/csrc
OBJDIR = build/obj
LIB = gulon_amd/lib/libgulon_hip.so
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math \
           -fvisibility=hidden -Wall -Wno-unused-function -Iinclude
SRCS = $(CSRC)/api_core.hip $(CSRC)/index_handle.hip $(CSRC)/scan.hip $(CSRC)/merge.hip $(CSRC)/knn.hip $(CSRC)/kmeans.hip $(CSRC)/kmeans_assign.hip $(CSRC)/kmeans_update.hip $(CSRC)/kmeans_stream.hip $(CSRC)/kmeans_mfma.hip $(CSRC)/replay.hip $(CSRC)/filter.hip $(CSRC)/filter_query.hip $(CSRC)/grouped.hip $(CSRC)/grouped_filter.hip $(CSRC)/wide.hip $(CSRC)/wide_filter.hip $(CSRC)/conflict_order.hip $(CSRC)/sharded.hip $(CSRC)/literal.hip $(CSRC)/decode.hip $(CSRC)/ingest.hip $(CSRC)/recall.hip $(CSRC)/refine.hip $(CSRC)/compose.hip $(CSRC)/subset.hip $(CSRC)/inspect.hip $(CSRC)/update.hip $(CSRC)/fine.hip $(CSRC)/rotate.hip $(CSRC)/exact.hip $(CSRC)/dataset_compose.hip $(CSRC)/analogy.hip $(CSRC)/cosmul.hip $(CSRC)/pairs.hip $(CSRC)/offset.hip $(CSRC)/rank.hip $(CSRC)/logsumexp.hip $(CSRC)/alignment.hip $(CSRC)/grouped_offset.hip
OBJS = $(patsubst $(CSRC)/%.hip,$(OBJDIR)/%.o,$(SRCS))
HDRS = $(CSRC)/common.hpp $(CSRC)/scan.hpp $(CSRC)/kmeans.hpp include/gulon_hip.h $(CSRC)/grouped_filter.hpp $(CSRC)/topk_heap.hpp $(CSRC)/normalize.hpp $(CSRC)/ingest_parse.h $(CSRC)/row_tile.hpp $(CSRC)/row_decode.hpp $(CSRC)/refine_replay.hpp $(CSRC)/select.hpp $(CSRC)/exact.hpp $(CSRC)/compose.hpp $(CSRC)/cosmul.hpp $(CSRC)/offset.hpp $(CSRC)/rank.hpp $(CSRC)/logsumexp.hpp $(CSRC)/moment.hpp $(CSRC)/grouped_offset.hpp $(CSRC)/table_scan.hpp
# The product library carries no test code.  The self-tests of the kernels (gulon_selftest_*) live in a second library
# that only tests/ loads: the same objects, with the files that have hooks compiled again under -DGULON_TEST_HOOKS.
HOOKLIB = gulon_amd/lib/libgulon_hip_testhooks.so
HOOKED = kmeans_update kmeans_stream kmeans_mfma conflict_order grouped grouped_filter filter_query wide_filter cosmul exact
HOOKOBJS = $(patsubst %,$(OBJDIR)/%.hooks.o,$(HOOKED)) $(filter-out $(patsubst %,$(OBJDIR)/%.o,$(HOOKED)),$(OBJS))

all: $(LIB) $(HOOKLIB) oracle build/test_host_api

# MFMA results are consumed by VALU/permlane code: keep accumulators in VGPRs (no v_accvgpr moves)
$(OBJDIR)/kmeans_mfma.o $(OBJDIR)/kmeans_mfma.hooks.o: HIPFLAGS += -mllvm -amdgpu-mfma-vgpr-form

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJDIR)/%.hooks.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -DGULON_TEST_HOOKS -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p gulon_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -ldl

$(HOOKLIB): $(HOOKOBJS)
	@mkdir -p gulon_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(HOOKOBJS) -ldl

oracle:
	$(MAKE) -C oracle

# C++ host-API parity test (tests/cpp): gulon.hpp over the C ABI, checked against the oracle
build/test_host_api: tests/cpp/test_host_api.cpp include/gulon/gulon.hpp include/gulon_hip.h $(LIB) oracle
	@mkdir -p build
	g++ -O2 -std=c++17 -Iinclude tests/cpp/test_host_api.cpp -o $@ -Lgulon_amd/lib -lgulon_hip -Loracle/build -lgulon_oracle \
	    -Wl,-rpath,'$$ORIGIN/../gulon_amd/lib' -Wl,-rpath,'$$ORIGIN/../oracle/build'

clean:
	rm -rf build $(LIB) $(HOOKLIB)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
