# Top-level helper targets (the library itself is built by `python -m imageexperiments_amd.build`, hipcc for gfx950).
#
#   make asan        host code of the product + the oracle under AddressSanitizer and UBSan (g++, CPU only):
#                      1. tests/cpp/asan_host: the product's host sources (entropy stage, container parser, dictionary, statistics)
#                         in one translation unit, driven through round trips and a corpus of truncated / bit-flipped containers
#                      2. the oracle built with the sanitizers, its golden-fixture tests run with libasan preloaded
#   make asan-host   step 1 only (what tests/test_asan_host.py runs)
#   make asan-index  tests/cpp/asan_index: the seek index's builder, validator and host chunk decoder on damaged containers and
#                    damaged indexes (what tests/test_asan_index.py runs)
#   make asan-encode-index  tests/cpp/asan_encode_index: the encoder's seek index on the host -- the by-plan route that records the
#                    checkpoints, index_from_plan -- against the parsed index (what tests/test_asan_encode_index.py runs)
#   make asan-encode-index2  tests/cpp/asan_encode_index2: index version 2 as the encoder emits it -- the by-plan route's aux entries,
#                    index_from_plan's check of them -- against the parsed index, and aux arrays that contradict the plans (what
#                    tests/test_asan_encode_index2.py runs)
#   make asan-region  tests/cpp/asan_region: the windowed parse on the host (a pixel rectangle through the seek index) on damaged
#                    indexes, damaged containers and rectangles of every kind (what tests/test_asan_region.py runs)
#   make asan-index2  tests/cpp/asan_index2: index version 2 on the host -- the aux section's builder and reader, the extension of a
#                    version-1 index, the windowed parse through the aux entries -- on damaged indexes and damaged containers
#                    (what tests/test_asan_index2.py runs)
#   make asan-view   tests/cpp/asan_view: the views on the host -- the truncation to the first steps, the view's parse through the
#                    seek index -- on damaged indexes, damaged containers and views of every kind (what tests/test_asan_view.py runs)
#   make asan-index-scan  tests/cpp/asan_index_scan: the seek index from a bit scan on the host -- step table, segment maps, chain and
#                    walk, the proposal and its acceptance -- on damaged and truncated containers, at sizes that make codes span
#                    segments and streams span windows (what tests/test_asan_index_scan.py runs)
#   make asan-delta  tests/cpp/asan_delta: the delta encoder's host definitions -- the changed tiles of two frames, the packed frame's
#                    geometry -- on exact-size frames of every stride, the extreme shapes among them (what tests/test_asan_delta.py runs)
#   make asan-budget  tests/cpp/asan_budget: the rate control's host definitions -- the multiplier table, the rate weights from seek
#                    indexes whole and damaged, the allocation at one multiplier -- on exact-size buffers (what tests/test_asan_budget.py runs)
#   make asan-quality  tests/cpp/asan_quality: the target-quality encode's host definitions -- the allocation's totals at all 256
#                    multipliers, the pick, the squared error of a PSNR -- on exact-size buffers and hostile arguments (what
#                    tests/test_asan_quality.py runs)
#   make asan-emphasis  tests/cpp/asan_emphasis: the emphasis maps' host definitions -- the allocation, the sweep and the floor allocation
#                    with a map, the map from a pixel mask -- on exact-size buffers and hostile values (what tests/test_asan_emphasis.py runs)
#   make asan-group  tests/cpp/asan_group: the group encodes' host definitions -- the allocation and the sweep over a group of frames with a
#                    weight table each, the squared error of a PSNR over a group -- on exact-size buffers and hostile values (what
#                    tests/test_asan_group.py runs)
#   make asan-tolerance  tests/cpp/asan_tolerance: the delta encoder's change tolerance -- a tile's summed squared difference, the tolerant
#                    list -- on exact-size frames of widths 1 to 1041, odd bases and padded rows (what tests/test_asan_tolerance.py runs)
#   make asan-patch  tests/cpp/asan_patch: the delta stream's patch format -- its one writer and its one parser -- on exact-size buffers:
#                    the hostile corpus of tests/patch_cases.py and every single-bit flip of valid patches' headers and lists (what
#                    tests/test_asan_patch.py runs)
#   make asan-patch-index  tests/cpp/asan_patch_index: patch format version 2 -- writer, parser, add and strip of the index section -- on
#                    exact-size buffers: valid and hostile blobs, every single-bit flip of a version-2 header, and the index section read
#                    by the host's index reader at each of the 8 byte alignments (what tests/test_asan_patch_index.py runs)
#
# GPU AddressSanitizer is not available on the test pool; the kernels are covered by the parity suite instead.
SAN = -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer
GOLDEN_MN = tests/golden/r0c1de5e1t_3_5.mn

tests/cpp/asan_host_bin: tests/cpp/asan_host.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_host.cpp -o $@

asan-host: tests/cpp/asan_host_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_host_bin $(GOLDEN_MN)

tests/cpp/asan_index_bin: tests/cpp/asan_index.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_index.cpp -o $@

asan-index: tests/cpp/asan_index_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_index_bin $(GOLDEN_MN)

tests/cpp/asan_encode_index_bin: tests/cpp/asan_encode_index.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_encode_index.cpp -o $@

asan-encode-index: tests/cpp/asan_encode_index_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_encode_index_bin

tests/cpp/asan_encode_index2_bin: tests/cpp/asan_encode_index2.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_encode_index2.cpp -o $@

asan-encode-index2: tests/cpp/asan_encode_index2_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_encode_index2_bin

tests/cpp/asan_region_bin: tests/cpp/asan_region.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_region.cpp -o $@

asan-region: tests/cpp/asan_region_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_region_bin

tests/cpp/asan_index2_bin: tests/cpp/asan_index2.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_index2.cpp -o $@

asan-index2: tests/cpp/asan_index2_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_index2_bin

tests/cpp/asan_view_bin: tests/cpp/asan_view.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_view.cpp -o $@

asan-view: tests/cpp/asan_view_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_view_bin

tests/cpp/asan_transcode_bin: tests/cpp/asan_transcode.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_transcode.cpp -o $@

asan-transcode: tests/cpp/asan_transcode_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_transcode_bin

tests/cpp/asan_compose_bin: tests/cpp/asan_compose.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_compose.cpp -o $@

asan-compose: tests/cpp/asan_compose_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_compose_bin

tests/cpp/asan_index_scan_bin: tests/cpp/asan_index_scan.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_index_scan.cpp -o $@

asan-index-scan: tests/cpp/asan_index_scan_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_index_scan_bin $(GOLDEN_MN)

tests/cpp/asan_delta_bin: tests/cpp/asan_delta.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_delta.cpp -o $@

asan-delta: tests/cpp/asan_delta_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 ./tests/cpp/asan_delta_bin

tests/cpp/asan_budget_bin: tests/cpp/asan_budget.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_budget.cpp -o $@

asan-budget: tests/cpp/asan_budget_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_budget_bin $(GOLDEN_MN)

tests/cpp/asan_quality_bin: tests/cpp/asan_quality.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_quality.cpp -o $@

asan-quality: tests/cpp/asan_quality_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_quality_bin

tests/cpp/asan_emphasis_bin: tests/cpp/asan_emphasis.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_emphasis.cpp -o $@

asan-emphasis: tests/cpp/asan_emphasis_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_emphasis_bin

tests/cpp/asan_group_bin: tests/cpp/asan_group.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_group.cpp -o $@

asan-group: tests/cpp/asan_group_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_group_bin

tests/cpp/asan_tolerance_bin: tests/cpp/asan_tolerance.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_tolerance.cpp -o $@

asan-tolerance: tests/cpp/asan_tolerance_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 ./tests/cpp/asan_tolerance_bin

tests/cpp/asan_patch_bin: tests/cpp/asan_patch.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_patch.cpp -o $@

asan-patch: tests/cpp/asan_patch_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_patch_bin

tests/cpp/asan_patch_index_bin: tests/cpp/asan_patch_index.cpp $(wildcard imageexperiments_amd/csrc/host_*.cpp imageexperiments_amd/csrc/host_*.h)
	g++ -std=c++17 -O1 -g $(SAN) -ffp-contract=off -pthread -Wall -Wno-unused-function tests/cpp/asan_patch_index.cpp -o $@

asan-patch-index: tests/cpp/asan_patch_index_bin
	ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 MPC_HOST_THREADS=4 ./tests/cpp/asan_patch_index_bin

oracle/_build/liboracle_asan.so: $(wildcard oracle/*.c oracle/*.h)
	mkdir -p oracle/_build
	gcc -std=c11 -O1 -g $(SAN) -ffp-contract=off -fPIC -shared -o $@ oracle/mpo_*.c -lm

asan-oracle: oracle/_build/liboracle_asan.so
	LD_PRELOAD=$$(gcc -print-file-name=libasan.so) ASAN_OPTIONS=detect_leaks=0 ORACLE_LIB=$(CURDIR)/oracle/_build/liboracle_asan.so \
	    python -m pytest tests/test_oracle_golden.py -x -q -p no:cacheprovider

asan: asan-host asan-index asan-encode-index asan-encode-index2 asan-region asan-index2 asan-view asan-transcode asan-compose asan-index-scan asan-delta asan-budget asan-quality asan-emphasis asan-group asan-tolerance asan-patch asan-patch-index asan-oracle

.PHONY: asan asan-host asan-index asan-encode-index asan-encode-index2 asan-region asan-index2 asan-view asan-transcode asan-compose asan-index-scan asan-delta asan-budget asan-quality asan-emphasis asan-group asan-tolerance asan-patch asan-patch-index asan-oracle
