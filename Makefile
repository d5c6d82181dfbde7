# Build of libsimilarity_transform.so (gfx950) and the CPU oracle.
# Usage: make [-j16]      (the same recipe __graft_entry__.build() runs)
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
# -fvisibility=hidden: the dynamic ABI is exactly what include/*.h declares
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off \
            -fno-fast-math -fvisibility=hidden -fvisibility-inlines-hidden \
            -Wall -Wextra -Wno-unused-parameter -Iinclude -Ieigen_value_amd/csrc
SRC      := eigen_value_amd/csrc/st_kernels.hip eigen_value_amd/csrc/st_solve.hip \
            eigen_value_amd/csrc/st_multi.hip eigen_value_amd/csrc/st_rendezvous.hip \
            eigen_value_amd/csrc/st_half.hip eigen_value_amd/csrc/st_csr.hip \
            eigen_value_amd/csrc/st_csr_batch.hip eigen_value_amd/csrc/st_csr_transpose.hip \
            eigen_value_amd/csrc/st_csr_terms.hip eigen_value_amd/csrc/st_csr_multi.hip \
            eigen_value_amd/csrc/st_csr_product.hip eigen_value_amd/csrc/st_csr_pattern.hip \
            eigen_value_amd/csrc/st_left.hip eigen_value_amd/csrc/st_pair.hip
OBJ     := $(patsubst eigen_value_amd/csrc/%.hip,build/%.o,$(SRC))
LIB      := eigen_value_amd/lib/libsimilarity_transform.so
# the tuning build (tools and the knob tests only): the same objects, with
# st_kernels and st_left compiled to also export the launch-table setters of
# include/st_tuning.h
TUNING_OBJ := build/st_kernels_tuning.o build/st_left_tuning.o \
              $(filter-out build/st_kernels.o build/st_left.o,$(OBJ))
LIB_TUNING := eigen_value_amd/lib/libsimilarity_transform_tuning.so
HDRS     := include/similarity_transform.h include/st_tuning.h eigen_value_amd/csrc/st_internal.h \
            eigen_value_amd/csrc/st_device.h eigen_value_amd/csrc/st_rendezvous.h \
            eigen_value_amd/csrc/st_half.h eigen_value_amd/csrc/st_csr.h \
            eigen_value_amd/csrc/st_csr_host.h eigen_value_amd/csrc/st_csr_batch.h \
            eigen_value_amd/csrc/st_csr_plan.h eigen_value_amd/csrc/st_csr_transpose.h \
            eigen_value_amd/csrc/st_csr_terms.h eigen_value_amd/csrc/st_csr_multi.h \
            eigen_value_amd/csrc/st_csr_product.h eigen_value_amd/csrc/st_csr_pattern.h \
            eigen_value_amd/csrc/st_left.h eigen_value_amd/csrc/st_left_host.h \
            eigen_value_amd/csrc/st_pair.h eigen_value_amd/csrc/st_pair_host.h

all: $(LIB) $(LIB_TUNING) oracle

build/%.o: eigen_value_amd/csrc/%.hip $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/%_tuning.o: eigen_value_amd/csrc/%.hip $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -DST_TUNING_ABI=1 -c $< -o $@

$(LIB): $(OBJ)
	@mkdir -p eigen_value_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJ) -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

$(LIB_TUNING): $(TUNING_OBJ)
	@mkdir -p eigen_value_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(TUNING_OBJ) -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

# an A/B probe build of the launch-shape / kernel-code switches
# (st_kernels.hip, st_device.h): make probe PROBE="-DST_FLAT_ALT=0"; run a
# tool with EIGEN_VALUE_LIB pointing at the result (st_version names the
# switches); never a product build
PROBE_LIB := eigen_value_amd/lib/variants/libsimilarity_transform_probe.so
probe: $(SRC) $(HDRS)
	@mkdir -p build/probe eigen_value_amd/lib/variants
	for f in $(SRC); do $(HIPCC) $(HIPFLAGS) -DST_TUNING_ABI=1 -DST_PROBES=1 $(PROBE) \
	  -c $$f -o build/probe/$$(basename $$f .hip).o || exit 1; done
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $(PROBE_LIB) build/probe/*.o \
	  -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

oracle:
	$(MAKE) -C oracle

# the host side of the CSR solve with terms and empty rows (st_csr_host.h)
# under the host sanitizers: a stand-alone program, run on the CPU, on the
# table matrices of tests/csr_cases.py (needs the library for the class table)
PYTHON ?= python
csr_terms_sanitize: $(LIB) tests/cpp/csr_terms_sanitize.cpp eigen_value_amd/csrc/st_csr_host.h
	@mkdir -p build/csr_tables
	$(PYTHON) tests/csr_cases.py build/csr_tables
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	  -fno-omit-frame-pointer -Ieigen_value_amd/csrc tests/cpp/csr_terms_sanitize.cpp \
	  -o build/csr_terms_sanitize
	./build/csr_terms_sanitize build/csr_tables/table0.bin build/csr_tables/table1.bin \
	  build/csr_tables/table2.bin

# the host side of the multi-column solve (st_csr_host.h: the packing and the
# per-column validation in its fixed order) under the host sanitizers, as
# csr_terms_sanitize
csr_multi_sanitize: $(LIB) tests/cpp/csr_multi_sanitize.cpp eigen_value_amd/csrc/st_csr_host.h
	@mkdir -p build/csr_tables
	$(PYTHON) tests/csr_cases.py build/csr_tables
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	  -fno-omit-frame-pointer -Ieigen_value_amd/csrc tests/cpp/csr_multi_sanitize.cpp \
	  -o build/csr_multi_sanitize
	./build/csr_multi_sanitize build/csr_tables/table0.bin build/csr_tables/table1.bin \
	  build/csr_tables/table2.bin

# the host side of the product operator B A (st_csr_host.h: the validation of
# two triples and of the rows of the product) under the host sanitizers, as
# csr_terms_sanitize
csr_product_sanitize: $(LIB) tests/cpp/csr_product_sanitize.cpp eigen_value_amd/csrc/st_csr_host.h
	@mkdir -p build/csr_tables
	$(PYTHON) tests/csr_cases.py build/csr_tables
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	  -fno-omit-frame-pointer -Ieigen_value_amd/csrc tests/cpp/csr_product_sanitize.cpp \
	  -o build/csr_product_sanitize
	./build/csr_product_sanitize build/csr_tables/table0.bin build/csr_tables/table1.bin \
	  build/csr_tables/table2.bin

# the host side of the pattern-only operator (st_csr_host.h: the scales'
# predicate and messages, the pattern's host check and the rows of the operator
# with terms) under the host sanitizers, as csr_terms_sanitize
csr_pattern_sanitize: $(LIB) tests/cpp/csr_pattern_sanitize.cpp eigen_value_amd/csrc/st_csr_host.h
	@mkdir -p build/csr_tables
	$(PYTHON) tests/csr_cases.py build/csr_tables
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	  -fno-omit-frame-pointer -Ieigen_value_amd/csrc tests/cpp/csr_pattern_sanitize.cpp \
	  -o build/csr_pattern_sanitize
	./build/csr_pattern_sanitize build/csr_tables/table0.bin build/csr_tables/table1.bin \
	  build/csr_tables/table2.bin

# the host arithmetic of the dense left-vector solve (st_left_host.h: rows
# per block, scratch layout, launch grid, the host twin's staging) under the
# host sanitizers: a stand-alone program, run on the CPU, that needs nothing
left_sanitize: tests/cpp/left_sanitize.cpp eigen_value_amd/csrc/st_left_host.h
	@mkdir -p build
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	  -fno-omit-frame-pointer -Ieigen_value_amd/csrc tests/cpp/left_sanitize.cpp \
	  -o build/left_sanitize
	./build/left_sanitize

# the host arithmetic of the dense pair solve (st_pair_host.h: the strip, the
# scratch layout and the launch grid, every tile walked as the kernel's lanes
# walk it) under the host sanitizers, as left_sanitize
pair_sanitize: tests/cpp/pair_sanitize.cpp eigen_value_amd/csrc/st_pair_host.h \
               eigen_value_amd/csrc/st_left_host.h
	@mkdir -p build
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	  -fno-omit-frame-pointer -Ieigen_value_amd/csrc tests/cpp/pair_sanitize.cpp \
	  -o build/pair_sanitize
	./build/pair_sanitize

clean:
	rm -rf build eigen_value_amd/lib
	$(MAKE) -C oracle clean

.PHONY: all oracle clean probe csr_terms_sanitize csr_multi_sanitize csr_product_sanitize \
        csr_pattern_sanitize left_sanitize pair_sanitize
