# libsfmcore.so: hand-written HIP for gfx950 + host C++ (C-ABI in include/sfmcore.h)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := 3dreconstruction_amd
CSRC := $(PKG)/csrc
LIB := $(PKG)/lib/libsfmcore.so
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -mcode-object-version=5 \
            -Wall -Wno-unused-result -I/opt/rocm/include
SRCS := $(wildcard $(CSRC)/*.cpp $(CSRC)/*.hip)
OBJS := $(patsubst $(CSRC)/%,build/%.o,$(SRCS))
HDRS := $(wildcard $(CSRC)/*.h) include/sfmcore.h $(wildcard $(PKG)/include/sfm/*.hpp)

all: $(LIB) oracle/liboracle.so tests/cpp/facade_test tests/cpp/plan_pool_test tests/cpp/triangulate_test \
     tests/cpp/triangulate_host_test tests/cpp/tracks_test tests/cpp/tracks_facade_test tests/cpp/resect_test \
     tests/cpp/relpose_test tests/cpp/sift_test tests/cpp/recon_test tests/cpp/colorize_test \
     tests/cpp/batch_points_test tests/cpp/undistort_test tests/cpp/depthmap_test \
     tests/cpp/depthfuse_test tests/cpp/mesh_test tests/cpp/texture_test

build/%.hip.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/%.cpp.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -fvisibility=hidden -fvisibility-inlines-hidden -x hip -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p $(PKG)/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -ldl

oracle/liboracle.so: FORCE
	$(MAKE) -C oracle

FORCE:

clean:
	rm -rf build $(LIB)
	$(MAKE) -C oracle clean

.PHONY: all clean FORCE

# C++ façade test (links the product and, as the checker, the oracle)
tests/cpp/facade_test: tests/cpp/facade_test.cpp 3dreconstruction_amd/include/sfm/sfm.hpp 3dreconstruction_amd/include/sfm/world.hpp $(LIB) oracle/liboracle.so
	g++ -O2 -std=c++17 -Wall -o $@ $< -I/opt/rocm/include -L3dreconstruction_amd/lib -Loracle -lsfmcore -loracle \
	    -Wl,-rpath,'$$ORIGIN/../../3dreconstruction_amd/lib' -Wl,-rpath,'$$ORIGIN/../../oracle'

# planner worker-pool stress test (host only, no GPU)
tests/cpp/plan_pool_test: tests/cpp/plan_pool_test.cpp $(CSRC)/ba_plan.cpp $(HDRS)
	g++ -O2 -std=c++17 -w -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $< -L/opt/rocm/lib -lamdhip64 -lpthread \
	    -Wl,-rpath,/opt/rocm/lib

# sfm::Triangulator façade test (links the product), and the same file with
# csrc/tri.cpp's host path compiled in (no library, no HIP runtime: host only)
tests/cpp/triangulate_test: tests/cpp/triangulate_test.cpp $(wildcard $(PKG)/include/sfm/*.hpp) $(LIB)
	g++ -O2 -std=c++17 -Wall -o $@ $< -I/opt/rocm/include -L3dreconstruction_amd/lib -lsfmcore \
	    -Wl,-rpath,'$$ORIGIN/../../3dreconstruction_amd/lib'

tests/cpp/triangulate_host_test: tests/cpp/triangulate_test.cpp $(CSRC)/tri.cpp $(HDRS)
	g++ -O2 -std=c++17 -w -DTRI_STANDALONE -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $<

# sfm::TracksBuilder: csrc/tracks.cpp's host path compiled in (no library, no
# HIP runtime: host only), and the same file over the product (--gpu: the GPU façade)
tests/cpp/tracks_test: tests/cpp/tracks_test.cpp $(CSRC)/tracks.cpp $(HDRS)
	g++ -O2 -std=c++17 -Wall -DTRACKS_STANDALONE -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $<

tests/cpp/tracks_facade_test: tests/cpp/tracks_test.cpp $(wildcard $(PKG)/include/sfm/*.hpp) $(LIB)
	g++ -O2 -std=c++17 -Wall -o $@ $< -I/opt/rocm/include -L3dreconstruction_amd/lib -lsfmcore \
	    -Wl,-rpath,'$$ORIGIN/../../3dreconstruction_amd/lib'

# sfm::Localizer on the host backend: csrc/resect.cpp's host path compiled in
# (no library, no HIP runtime: host only)
tests/cpp/resect_test: tests/cpp/resect_test.cpp $(CSRC)/resect.cpp $(HDRS)
	g++ -O2 -std=c++17 -w -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $<

# sfm::RelativePoser on the host backend: csrc/relpose.cpp's host path compiled
# in (no library, no HIP runtime: host only)
tests/cpp/relpose_test: tests/cpp/relpose_test.cpp $(CSRC)/relpose.cpp $(HDRS)
	g++ -O2 -std=c++17 -w -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $<

# sfm::HostSIFT_Image_describer and detectFeature(): csrc/sift.cpp's host path,
# the image generator and the file formats compiled in (no library, no HIP
# runtime: host only)
tests/cpp/sift_test: tests/cpp/sift_test.cpp $(CSRC)/sift.cpp $(CSRC)/synth.cpp $(CSRC)/mvg_io.cpp $(HDRS)
	g++ -O2 -std=c++17 -w -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $<

# sfm::SequentialSfMReconstructionEngine on the host backend: the host paths of
# csrc/recon.cpp and of the stages it drives compiled in, one translation unit
# each (no library, no HIP runtime: host only)
RECON_HOST_SRCS := $(CSRC)/recon.cpp $(CSRC)/relpose.cpp $(CSRC)/resect.cpp $(CSRC)/tri.cpp
RECON_HOST_DEFS := -DSFM_RECON_HOST_ONLY -DSFM_RELPOSE_HOST_ONLY -DSFM_RESECT_HOST_ONLY -DSFM_TRI_HOST_ONLY
tests/cpp/recon_test: tests/cpp/recon_test.cpp $(RECON_HOST_SRCS) $(HDRS)
	g++ -O2 -std=c++17 -w $(RECON_HOST_DEFS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $< $(RECON_HOST_SRCS)

# sfm::ColorizeTracks on the host backend: csrc/colorize.cpp's host path (the
# serial twin, the sampling, the PLY writer) compiled in (no library, no HIP
# runtime: host only)
tests/cpp/colorize_test: tests/cpp/colorize_test.cpp $(CSRC)/colorize.cpp $(HDRS)
	g++ -O2 -std=c++17 -Wall -DSFM_COLORIZE_HOST_ONLY -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $< $(CSRC)/colorize.cpp

# the Schur kernel's batch rule (csrc/ba_types.h batch_fits / batch_count) walked on the host
tests/cpp/batch_points_test: tests/cpp/batch_points_test.cpp $(CSRC)/ba_types.h
	g++ -O2 -std=c++17 -Wall -o $@ $<

# the dense hand-off on the host backend: the host paths of csrc/undistort.cpp
# (checks, chunk plan, host twin, PNM writer) and csrc/dense_scene.cpp and the
# façade of include/sfm/dense.hpp compiled in (no library, no HIP runtime: host
# only).  UNDISTORT_TEST_FLAGS=-fsanitize=address,undefined gives the sanitizer build.
UNDISTORT_HOST_SRCS := $(CSRC)/undistort.cpp $(CSRC)/dense_scene.cpp
tests/cpp/undistort_test: tests/cpp/undistort_test.cpp $(UNDISTORT_HOST_SRCS) $(HDRS)
	g++ -O2 -std=c++17 -Wall -Wno-unknown-pragmas $(UNDISTORT_TEST_FLAGS) -DSFM_UNDISTORT_HOST_ONLY -D__HIP_PLATFORM_AMD__ \
	    -I/opt/rocm/include -o $@ $< $(UNDISTORT_HOST_SRCS) -lpthread

# the dense depth maps on the host backend: the host paths of csrc/depthmap.cpp
# (checks, view selection, the host twins of the estimation and of the filter),
# csrc/dense_views.cpp (the images' checks, the thread pool) and
# csrc/dense_scene.cpp and the façade of include/sfm/dense.hpp compiled in
# (no library, no HIP runtime: host only).
# DEPTHMAP_TEST_FLAGS=-fsanitize=address,undefined gives the sanitizer build.
DEPTHMAP_HOST_SRCS := $(CSRC)/depthmap.cpp $(CSRC)/dense_views.cpp $(CSRC)/undistort.cpp $(CSRC)/dense_scene.cpp
tests/cpp/depthmap_test: tests/cpp/depthmap_test.cpp $(DEPTHMAP_HOST_SRCS) $(HDRS)
	g++ -O2 -std=c++17 -Wall -Wno-unknown-pragmas $(DEPTHMAP_TEST_FLAGS) -DSFM_DEPTHMAP_HOST_ONLY -DSFM_UNDISTORT_HOST_ONLY \
	    -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $< $(DEPTHMAP_HOST_SRCS) -lpthread

# the dense fusion on the host backend: the host paths of csrc/fuse.cpp (checks,
# pair lists, the host twin, the view lists, sfm_densify_host) and
# csrc/dense_ply.cpp (the PLY writer) over those of the depth maps, and the façade of include/sfm/dense.hpp compiled
# in (no library, no HIP runtime: host only).  fuse.cpp and depthmap.cpp switch
# contraction off themselves (#pragma at their top), as the .hip files do.
# DEPTHFUSE_TEST_FLAGS=-fsanitize=address,undefined gives the sanitizer build.
DEPTHFUSE_HOST_SRCS := $(CSRC)/fuse.cpp $(CSRC)/dense_ply.cpp $(DEPTHMAP_HOST_SRCS)
tests/cpp/depthfuse_test: tests/cpp/depthfuse_test.cpp $(DEPTHFUSE_HOST_SRCS) $(HDRS)
	g++ -O2 -std=c++17 -Wall -Wno-unknown-pragmas -ffp-contract=off $(DEPTHFUSE_TEST_FLAGS) -DSFM_DEPTHMAP_HOST_ONLY \
	    -DSFM_UNDISTORT_HOST_ONLY -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $< $(DEPTHFUSE_HOST_SRCS) -lpthread

# the mesh stage on the host backend: the host paths of csrc/mesh.cpp (checks,
# the grid fit, the host twins of the integration and the extraction),
# csrc/dense_views.cpp (the images' checks, the thread pool) and
# csrc/dense_ply.cpp (the PLY writer), and the façade of include/sfm/mesh.hpp
# compiled in (no library, no HIP runtime: host only).
# mesh.cpp switches contraction off itself (#pragma at its top), as mesh.hip does.
# MESH_TEST_FLAGS=-fsanitize=address,undefined gives the sanitizer build.
MESH_HOST_SRCS := $(CSRC)/mesh.cpp $(CSRC)/dense_views.cpp $(CSRC)/dense_ply.cpp
tests/cpp/mesh_test: tests/cpp/mesh_test.cpp $(MESH_HOST_SRCS) $(HDRS)
	g++ -O2 -std=c++17 -Wall -Wno-unknown-pragmas -ffp-contract=off $(MESH_TEST_FLAGS) -DSFM_DEPTHMAP_HOST_ONLY \
	    -DSFM_UNDISTORT_HOST_ONLY -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $< $(MESH_HOST_SRCS) -lpthread

# the mesh texturing on the host backend: the host paths of csrc/texture.cpp
# (checks, the atlas fit, the host twins of the view choice and the bake),
# csrc/dense_views.cpp and csrc/dense_ply.cpp as the mesh stage's test,
# csrc/undistort.cpp (sfm::TexturedMesh::write stores the atlas with its PNM
# writer), and the façade of include/sfm/mesh.hpp compiled in (no library, no
# HIP runtime: host only).  texture.cpp switches contraction off itself.
# TEXTURE_TEST_FLAGS=-fsanitize=address,undefined gives the sanitizer build.
TEXTURE_HOST_SRCS := $(CSRC)/texture.cpp $(CSRC)/dense_views.cpp $(CSRC)/dense_ply.cpp $(CSRC)/undistort.cpp
tests/cpp/texture_test: tests/cpp/texture_test.cpp $(TEXTURE_HOST_SRCS) $(HDRS)
	g++ -O2 -std=c++17 -Wall -Wno-unknown-pragmas -ffp-contract=off $(TEXTURE_TEST_FLAGS) -DSFM_DEPTHMAP_HOST_ONLY \
	    -DSFM_UNDISTORT_HOST_ONLY -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $< $(TEXTURE_HOST_SRCS) -lpthread
