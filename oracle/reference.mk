# oracle/reference.mk -- the reference's own programs, for the GPU tests that run them
# (tests/test_reference_examples_gpu.py) and for `bench.py --full`: LegoSNARK's UNCHANGED sources,
# read in place and never copied, compiled against the libff-compatible shim and linked with the
# MI355X library.  The finished programs land in oracle/_ref/, a build product (kept out of git)
# that holds nothing else -- no objects, no links into the reference -- so that it can be carried
# to a machine without the reference:
#   _ref/reference, _ref/reference_mc                legosnark_amd/shim/Makefile, default and MULTICORE=1
#   _ref/reference_cmake{,_mc}/src/examples          the reference's own CMakeLists.txt (default,
#                                                    -DMULTICORE=ON) over the drop-in packages of
#                                                    legosnark_amd/shim/cmake
# Objects and CMake trees stay in build/ (also ignored).
# REF is the reference's src/ directory, as for legosnark_amd/shim/Makefile, whose default it takes.
#   make -C oracle -f reference.mk [REF=/path/to/legosnark/src] [makefile | cmake]
# The programs find liblegosnark_amd.so through LD_LIBRARY_PATH=<checkout>/legosnark_amd, so that
# they still run after the tree has been moved (their build-time run path is absolute).
SHIM := $(abspath ../legosnark_amd/shim)
BUILD := $(abspath ../build)
OUT := $(abspath _ref)
REF ?= $(shell sed -n 's/^REF ?= //p' $(SHIM)/Makefile)
EXAMPLES := cplink hadamard matrixsc
CHECKS := keygen_check spmd_prover_check pairing_check shim_check omp_check domain_check fr_check
CMAKE_CONFIG := -G Ninja -DWITH_PROCPS=OFF -DCMAKE_POLICY_VERSION_MINIMUM=3.5 -Wno-dev

.PHONY: all makefile cmake single multicore cmake_single cmake_multicore
all: makefile cmake
makefile: single multicore
single:
	$(MAKE) -C $(SHIM) REF=$(REF) OUT=$(BUILD)/reference
	mkdir -p $(OUT)/reference
	cp -p $(addprefix $(BUILD)/reference/,$(EXAMPLES) $(CHECKS) resident_prover_check) $(OUT)/reference/
multicore:
	$(MAKE) -C $(SHIM) REF=$(REF) OUT=$(BUILD)/reference_mc MULTICORE=1
	mkdir -p $(OUT)/reference_mc
	cp -p $(addprefix $(BUILD)/reference_mc/,$(EXAMPLES) $(CHECKS)) $(OUT)/reference_mc/

# the reference's default configuration (OPT_FLAGS "-O3 -ggdb", MULTICORE=OFF) and its -DMULTICORE=ON one;
# CMake's and the compiler's output go to a log beside the build, shown when the build fails
cmake: cmake_single cmake_multicore
$(BUILD)/reference_cmake_tree/CMakeLists.txt:
	$(SHIM)/cmake/stage_tree.sh $(REF)/.. $(BUILD)/reference_cmake_tree > /dev/null
cmake_single: $(BUILD)/reference_cmake_tree/CMakeLists.txt
	{ cmake -S $(BUILD)/reference_cmake_tree -B $(BUILD)/reference_cmake $(CMAKE_CONFIG) && cmake --build $(BUILD)/reference_cmake --target $(EXAMPLES); } \
		> $(BUILD)/reference_cmake.log 2>&1 || { tail -40 $(BUILD)/reference_cmake.log; exit 1; }
	mkdir -p $(OUT)/reference_cmake/src/examples
	cp -p $(addprefix $(BUILD)/reference_cmake/src/examples/,$(EXAMPLES)) $(OUT)/reference_cmake/src/examples/
cmake_multicore: $(BUILD)/reference_cmake_tree/CMakeLists.txt
	{ cmake -S $(BUILD)/reference_cmake_tree -B $(BUILD)/reference_cmake_mc $(CMAKE_CONFIG) -DMULTICORE=ON && cmake --build $(BUILD)/reference_cmake_mc --target $(EXAMPLES); } \
		> $(BUILD)/reference_cmake_mc.log 2>&1 || { tail -40 $(BUILD)/reference_cmake_mc.log; exit 1; }
	mkdir -p $(OUT)/reference_cmake_mc/src/examples
	cp -p $(addprefix $(BUILD)/reference_cmake_mc/src/examples/,$(EXAMPLES)) $(OUT)/reference_cmake_mc/src/examples/
