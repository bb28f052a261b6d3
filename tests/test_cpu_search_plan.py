"""CPU suite: which beam-search kernel a call runs (leann-rs_amd/csrc/search_plan.h: the one place where the width map, the rows in
flight, the wave count, the visited-table size and the LDS figure are decided).  host/search_plan_selftest.cpp is built with the host
compiler under AddressSanitizer + UBSan and (a) plans every point of a grid — every ld in 4..4100 step 4 as f32 and as bf16 rows and
every feat_h in 1..1100; nq in {1, 384, 385, 512, 513, 640, 641, 4096}; ef in {1, 64, 65, 341, 342, 683, 5000}; lists of 16, 64, 65, 128
ids; filtered / construction / planes ready on and off; the knobs unset, LEANN_DEBUG_HASH_BITS=8, LEANN_DEBUG_NW=1, 8, 16 and
LEANN_DEBUG_NO_FEAT256 — and checks: an accepted plan's LDS is search_lds_bytes of its own fields with two buffers iff more than 4
waves, and at most 160 KiB; 4, 8 or 16 waves; the screen kernel under its six conditions and only then; wide iff lists of more than 64
ids, and never 8 waves; a table of 2^6..2^15 slots; T x 256 covers the row; the kernel's name parses back to the plan's fields; every
refusal is one of the three the library knows.  (b) EXPECTED below: plans written by hand from the rules as they stood in api.hip and
search_bf16.hip before there was a plan, not computed by a second copy of them — the family, the kernel's name as a profiler prints it,
hash_bits and the LDS bytes, or the error code and its message.  No GPU, no library."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "leann-rs_amd", "host", "search_plan_selftest")
INVALID, UNSUPPORTED = 1, 5

# (ld, d, feat_h, bf16, max(M0, M), planes ready, nq, k, ef, filtered, construction, LEANN_DEBUG_HASH_BITS, LEANN_DEBUG_NW, LEANN_DEBUG_NO_FEAT256)
#   -> family, kernel, hash_bits, lds_bytes   or   -> error code, message
EXPECTED = [
    # stored f32 rows: every width of the GPU suites at 16 / 8 / 4 waves, plain and filtered
    ((128, 128, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<1, 4, 16, false>", 12, 18368),
    ((128, 128, 0, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<1, 4, 16>", 12, 19168),
    ((128, 128, 0, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<1, 4, 8, false>", 12, 18368),
    ((128, 128, 0, 0, 32, 0, 512, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<1, 4, 8>", 12, 19168),
    ((128, 128, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<1, 4, 4, false>", 12, 17920),
    ((128, 128, 0, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<1, 4, 4>", 12, 18400),
    ((384, 384, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<2, 4, 16, false>", 12, 18368),
    ((384, 384, 0, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<2, 4, 16>", 12, 19168),
    ((384, 384, 0, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<2, 4, 8, false>", 12, 18368),
    ((384, 384, 0, 0, 32, 0, 512, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<2, 4, 8>", 12, 19168),
    ((384, 384, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<2, 4, 4, false>", 12, 17920),
    ((384, 384, 0, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<2, 4, 4>", 12, 18400),
    ((768, 768, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 16, false>", 13, 34752),
    ((768, 768, 0, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<3, 4, 16>", 13, 35552),
    ((768, 768, 0, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 8, false>", 13, 34752),
    ((768, 768, 0, 0, 32, 0, 512, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<3, 4, 8>", 13, 35552),
    ((768, 768, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 4, false>", 13, 34304),
    ((768, 768, 0, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<3, 4, 4>", 13, 34784),
    ((1024, 1024, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<4, 3, 16, false>", 13, 34752),
    ((1024, 1024, 0, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<4, 3, 16>", 13, 35552),
    ((1024, 1024, 0, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<4, 3, 8, false>", 13, 34752),
    ((1024, 1024, 0, 0, 32, 0, 512, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<4, 3, 8>", 13, 35552),
    ((1024, 1024, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<4, 3, 4, false>", 13, 34304),
    ((1024, 1024, 0, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<4, 3, 4>", 13, 34784),
    ((1100, 1100, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<6, 2, 16, false>", 13, 34752),
    ((1100, 1100, 0, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<6, 2, 16>", 13, 35552),
    ((1100, 1100, 0, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<6, 2, 8, false>", 13, 34752),
    ((1100, 1100, 0, 0, 32, 0, 512, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<6, 2, 8>", 13, 35552),
    ((1100, 1100, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<6, 2, 4, false>", 13, 34304),
    ((1100, 1100, 0, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<6, 2, 4>", 13, 34784),
    ((1536, 1536, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<6, 2, 16, false>", 13, 34752),
    ((1536, 1536, 0, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<6, 2, 16>", 13, 35552),
    ((1536, 1536, 0, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<6, 2, 8, false>", 13, 34752),
    ((1536, 1536, 0, 0, 32, 0, 512, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<6, 2, 8>", 13, 35552),
    ((1536, 1536, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<6, 2, 4, false>", 13, 34304),
    ((1536, 1536, 0, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<6, 2, 4>", 13, 34784),
    ((1600, 1600, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<8, 2, 16, false>", 13, 34752),
    ((1600, 1600, 0, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<8, 2, 16>", 13, 35552),
    ((1600, 1600, 0, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<8, 2, 8, false>", 13, 34752),
    ((1600, 1600, 0, 0, 32, 0, 512, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<8, 2, 8>", 13, 35552),
    ((1600, 1600, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<8, 2, 4, false>", 13, 34304),
    ((1600, 1600, 0, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<8, 2, 4>", 13, 34784),
    ((2820, 2820, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<12, 1, 16, false>", 13, 34752),
    ((2820, 2820, 0, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<12, 1, 16>", 13, 35552),
    ((2820, 2820, 0, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<12, 1, 8, false>", 13, 34752),
    ((2820, 2820, 0, 0, 32, 0, 512, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<12, 1, 8>", 13, 35552),
    ((2820, 2820, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<12, 1, 4, false>", 13, 34304),
    ((2820, 2820, 0, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<12, 1, 4>", 13, 34784),
    ((3400, 3400, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<16, 1, 16, false>", 13, 34752),
    ((3400, 3400, 0, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<16, 1, 16>", 13, 35552),
    ((3400, 3400, 0, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<16, 1, 8, false>", 13, 34752),
    ((3400, 3400, 0, 0, 32, 0, 512, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<16, 1, 8>", 13, 35552),
    ((3400, 3400, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<16, 1, 4, false>", 13, 34304),
    ((3400, 3400, 0, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<16, 1, 4>", 13, 34784),
    ((4096, 4096, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<16, 1, 16, false>", 13, 34752),
    ((4096, 4096, 0, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<16, 1, 16>", 13, 35552),
    ((4096, 4096, 0, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<16, 1, 8, false>", 13, 34752),
    ((4096, 4096, 0, 0, 32, 0, 512, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<16, 1, 8>", 13, 35552),
    ((4096, 4096, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<16, 1, 4, false>", 13, 34304),
    ((4096, 4096, 0, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<16, 1, 4>", 13, 34784),
    # partial chunks: ld 260 -> T = 2, 900 -> 4, 2048 -> 8
    ((260, 260, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<2, 4, 4, false>", 12, 17920),
    ((900, 900, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<4, 3, 4, false>", 13, 34304),
    ((2048, 2048, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<8, 2, 4, false>", 13, 34304),
    # past 4 096 floats: refused
    ((4100, 4100, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), 1, "search: dims 4100 > 4096 not supported"),
    ((4100, 4097, 0, 1, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), 1, "search: dims 4097 > 4096 not supported"),
    # batch thresholds 384 | 385 and 640 | 641
    ((128, 128, 0, 0, 32, 0, 384, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<1, 4, 16, false>", 12, 18368),
    ((128, 128, 0, 0, 32, 0, 385, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<1, 4, 8, false>", 12, 18368),
    ((128, 128, 0, 0, 32, 0, 640, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<1, 4, 8, false>", 12, 18368),
    ((128, 128, 0, 0, 32, 0, 641, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<1, 4, 4, false>", 12, 17920),
    # visited table: 12 bits up to ld 512 and ef 64
    ((512, 512, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<2, 4, 16, false>", 12, 18368),
    ((512, 512, 0, 0, 32, 0, 64, 10, 65, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<2, 4, 16, false>", 13, 34784),
    ((516, 516, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 16, false>", 13, 34752),
    ((516, 516, 0, 0, 32, 0, 64, 10, 65, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 16, false>", 13, 34784),
    # ... pick(ef): 2^13 >= 24 x 341, 2^14 >= 24 x 682, then 15
    ((768, 768, 0, 0, 32, 0, 64, 10, 341, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 16, false>", 13, 39200),
    ((768, 768, 0, 0, 32, 0, 64, 10, 342, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 16, false>", 14, 71968),
    ((768, 768, 0, 0, 32, 0, 64, 10, 682, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 16, false>", 14, 77408),
    ((768, 768, 0, 0, 32, 0, 64, 10, 683, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 16, false>", 15, 142976),
    # ... the knob wins, at any width
    ((384, 384, 0, 0, 32, 0, 64, 10, 64, 0, 0, 8, 0, 0), "F32", "beam_search_kernel<2, 4, 16, false>", 8, 3008),
    ((384, 384, 0, 0, 32, 0, 704, 10, 64, 0, 0, 8, 0, 0), "F32", "beam_search_kernel<2, 4, 4, false>", 8, 2560),
    ((768, 768, 0, 0, 32, 0, 64, 10, 5000, 0, 0, 9, 0, 0), "F32", "beam_search_kernel<3, 4, 16, false>", 9, 83008),
    # more than 160 KiB of LDS: refused
    ((768, 768, 0, 0, 32, 0, 64, 10, 5000, 0, 0, 0, 0, 0), 1, "search: complexity 5000 needs 212032 B of LDS per query (> 160 KiB)"),
    # construction searches: the 13-bit table at any width; an allow mask takes the filtered kernel
    ((128, 128, 0, 0, 32, 0, 64, 10, 64, 0, 1, 0, 0, 0), "F32", "beam_search_kernel<1, 4, 16, true>", 13, 34752),
    ((768, 768, 0, 0, 32, 0, 704, 10, 64, 0, 1, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 4, true>", 13, 34304),
    ((128, 128, 0, 0, 32, 0, 64, 10, 64, 1, 1, 0, 0, 0), "F32", "beam_search_filtered_kernel<1, 4, 16>", 13, 35552),
    # lists of 64 | 65 ids: wide kernels, which have no 8-wave form
    ((128, 128, 0, 0, 64, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<1, 4, 8, false>", 12, 19136),
    ((128, 128, 0, 0, 65, 0, 512, 10, 64, 0, 0, 0, 0, 0), "F32", "wide_beam_search_kernel<1, 4, 16, false>", 12, 19168),
    ((128, 128, 0, 0, 128, 0, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "wide_beam_search_filtered_kernel<1, 4, 4>", 12, 20320),
    ((768, 768, 0, 0, 128, 0, 64, 10, 64, 0, 1, 0, 0, 0), "F32", "wide_beam_search_kernel<3, 4, 16, true>", 13, 37056),
    # LEANN_DEBUG_NW: >= 16 -> 16, 8..15 -> 8, 1..7 -> 4; wide lists 8 -> 16
    ((128, 128, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 1, 0), "F32", "beam_search_kernel<1, 4, 4, false>", 12, 17920),
    ((128, 128, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 7, 0), "F32", "beam_search_kernel<1, 4, 4, false>", 12, 17920),
    ((128, 128, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 8, 0), "F32", "beam_search_kernel<1, 4, 8, false>", 12, 18368),
    ((128, 128, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 15, 0), "F32", "beam_search_kernel<1, 4, 8, false>", 12, 18368),
    ((128, 128, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 16, 0), "F32", "beam_search_kernel<1, 4, 16, false>", 12, 18368),
    ((128, 128, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 64, 0), "F32", "beam_search_kernel<1, 4, 16, false>", 12, 18368),
    ((128, 128, 0, 0, 65, 0, 704, 10, 64, 0, 0, 0, 8, 0), "F32", "wide_beam_search_kernel<1, 4, 16, false>", 12, 19168),
    ((128, 128, 0, 0, 65, 0, 64, 10, 64, 0, 0, 0, 4, 0), "F32", "wide_beam_search_kernel<1, 4, 4, false>", 12, 18320),
    # row screen: 4 waves, T 3 / 6, planes ready, plain, narrow lists: all six or the whole-row kernel
    ((768, 768, 0, 0, 32, 1, 704, 10, 64, 0, 0, 0, 0, 0), "SCREEN", "beam_search_screen_kernel<3, 4>", 13, 34304),
    ((1100, 1100, 0, 0, 32, 1, 704, 10, 64, 0, 0, 0, 0, 0), "SCREEN", "beam_search_screen_kernel<6, 2>", 13, 34304),
    ((1536, 1536, 0, 0, 32, 1, 641, 10, 64, 0, 0, 0, 0, 0), "SCREEN", "beam_search_screen_kernel<6, 2>", 13, 34304),
    ((768, 768, 0, 0, 32, 1, 64, 10, 64, 0, 0, 0, 4, 0), "SCREEN", "beam_search_screen_kernel<3, 4>", 13, 34304),
    ((768, 768, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 4, false>", 13, 34304),
    ((768, 768, 0, 0, 32, 1, 640, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 8, false>", 13, 34752),
    ((768, 768, 0, 0, 32, 1, 64, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 16, false>", 13, 34752),
    ((768, 768, 0, 0, 32, 1, 704, 10, 64, 1, 0, 0, 0, 0), "F32", "beam_search_filtered_kernel<3, 4, 4>", 13, 34784),
    ((768, 768, 0, 0, 32, 1, 704, 10, 64, 0, 1, 0, 0, 0), "F32", "beam_search_kernel<3, 4, 4, true>", 13, 34304),
    ((768, 768, 0, 0, 65, 1, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "wide_beam_search_kernel<3, 4, 4, false>", 13, 34704),
    ((1024, 1024, 0, 0, 32, 1, 704, 10, 64, 0, 0, 0, 0, 0), "F32", "beam_search_kernel<4, 3, 4, false>", 13, 34304),
    # bf16 rows: every width, 4 waves (nq > 512) and 16 waves; T = 16 has no 16-wave form
    ((128, 128, 0, 1, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<1, 8, 4>", 12, 17920),
    ((128, 128, 0, 1, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<1, 4, 16>", 12, 18368),
    ((260, 260, 0, 1, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<2, 8, 4>", 12, 17920),
    ((260, 260, 0, 1, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<2, 4, 16>", 12, 18368),
    ((768, 768, 0, 1, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<3, 8, 4>", 13, 34304),
    ((768, 768, 0, 1, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<3, 4, 16>", 13, 34752),
    ((900, 900, 0, 1, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<4, 6, 4>", 13, 34304),
    ((900, 900, 0, 1, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<4, 4, 16>", 13, 34752),
    ((1100, 1100, 0, 1, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<6, 4, 4>", 13, 34304),
    ((1100, 1100, 0, 1, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<6, 3, 16>", 13, 34752),
    ((1600, 1600, 0, 1, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<8, 4, 4>", 13, 34304),
    ((1600, 1600, 0, 1, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<8, 2, 16>", 13, 34752),
    ((2820, 2820, 0, 1, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<12, 2, 4>", 13, 34304),
    ((2820, 2820, 0, 1, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<12, 1, 16>", 13, 34752),
    ((3400, 3400, 0, 1, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<16, 2, 4>", 13, 34304),
    ((3400, 3400, 0, 1, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<16, 2, 4>", 13, 34304),
    ((4096, 4096, 0, 1, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "BF16", "bf16_beam_search_filtered_kernel<16, 2, 4>", 13, 34784),
    # ... threshold 512 | 513, LEANN_DEBUG_NW ignored, filtered, wide, knob, construction refused
    ((768, 768, 0, 1, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<3, 4, 16>", 13, 34752),
    ((768, 768, 0, 1, 32, 0, 513, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<3, 8, 4>", 13, 34304),
    ((128, 128, 0, 1, 32, 0, 64, 10, 64, 0, 0, 0, 1, 0), "BF16", "bf16_beam_search_kernel<1, 4, 16>", 12, 18368),
    ((128, 128, 0, 1, 32, 0, 704, 10, 64, 0, 0, 0, 16, 0), "BF16", "bf16_beam_search_kernel<1, 8, 4>", 12, 17920),
    ((768, 768, 0, 1, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "BF16", "bf16_beam_search_filtered_kernel<3, 8, 4>", 13, 34784),
    ((768, 768, 0, 1, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "BF16", "bf16_beam_search_filtered_kernel<3, 4, 16>", 13, 35552),
    ((128, 128, 0, 1, 65, 0, 64, 10, 64, 0, 0, 0, 0, 0), "BF16", "wide_bf16_beam_search_kernel<1, 4, 16>", 12, 19168),
    ((384, 384, 0, 1, 128, 0, 704, 10, 64, 1, 0, 0, 0, 0), "BF16", "wide_bf16_beam_search_filtered_kernel<2, 8, 4>", 12, 20320),
    ((768, 768, 0, 1, 32, 1, 704, 10, 64, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<3, 8, 4>", 13, 34304),
    ((384, 384, 0, 1, 32, 0, 64, 10, 65, 0, 0, 0, 0, 0), "BF16", "bf16_beam_search_kernel<2, 4, 16>", 13, 34784),
    ((384, 384, 0, 1, 32, 0, 64, 10, 64, 0, 0, 8, 0, 0), "BF16", "bf16_beam_search_kernel<2, 4, 16>", 8, 3008),
    ((768, 768, 0, 1, 32, 0, 64, 10, 64, 0, 1, 0, 0, 0), 5, "bf16 rows: construction searches are not supported"),
    # recompute-on graphs: feat_h 100, 256 (with and without LEANN_DEBUG_NO_FEAT256), 300, 640, 1025; 16 waves up to 512 queries
    ((768, 768, 100, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "FEAT", "beam_search_feat_kernel<1, 5, 16>", 12, 18368),
    ((768, 768, 100, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "FEAT", "beam_search_feat_kernel<1, 5, 4>", 12, 17920),
    ((768, 768, 100, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "FEAT", "beam_search_feat_filtered_kernel<1, 5, 16>", 12, 19168),
    ((768, 768, 100, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "FEAT", "beam_search_feat_filtered_kernel<1, 5, 4>", 12, 18400),
    ((768, 768, 256, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "FEAT256", "beam_search_feat256_kernel<1, 16>", 12, 18368),
    ((768, 768, 256, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "FEAT256", "beam_search_feat256_kernel<1, 4>", 12, 17920),
    ((768, 768, 256, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "FEAT256", "beam_search_feat256_filtered_kernel<1, 16>", 12, 19168),
    ((768, 768, 256, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "FEAT256", "beam_search_feat256_filtered_kernel<1, 4>", 12, 18400),
    ((768, 768, 256, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 1), "FEAT", "beam_search_feat_kernel<1, 5, 16>", 12, 18368),
    ((768, 768, 256, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 1), "FEAT", "beam_search_feat_kernel<1, 5, 4>", 12, 17920),
    ((768, 768, 256, 0, 128, 0, 704, 10, 64, 0, 0, 0, 0, 0), "FEAT256", "wide_beam_search_feat256_kernel<1, 4>", 12, 19072),
    ((768, 768, 256, 0, 65, 0, 64, 10, 64, 1, 0, 0, 0, 0), "FEAT256", "wide_beam_search_feat256_filtered_kernel<1, 16>", 12, 20496),
    ((768, 768, 300, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "FEAT", "beam_search_feat_kernel<2, 6, 16>", 12, 18368),
    ((768, 768, 300, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "FEAT", "beam_search_feat_kernel<2, 6, 4>", 12, 17920),
    ((768, 768, 300, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "FEAT", "beam_search_feat_filtered_kernel<2, 6, 16>", 12, 19168),
    ((768, 768, 300, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "FEAT", "beam_search_feat_filtered_kernel<2, 6, 4>", 12, 18400),
    ((768, 768, 640, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), "FEAT", "beam_search_feat_kernel<4, 4, 16>", 12, 18368),
    ((768, 768, 640, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0), "FEAT", "beam_search_feat_kernel<4, 4, 4>", 12, 17920),
    ((768, 768, 640, 0, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0), "FEAT", "beam_search_feat_filtered_kernel<4, 4, 16>", 12, 19168),
    ((768, 768, 640, 0, 32, 0, 704, 10, 64, 1, 0, 0, 0, 0), "FEAT", "beam_search_feat_filtered_kernel<4, 4, 4>", 12, 18400),
    ((768, 768, 1024, 0, 65, 0, 704, 10, 64, 1, 0, 0, 0, 0), "FEAT", "wide_beam_search_feat_filtered_kernel<4, 4, 4>", 12, 19064),
    ((768, 768, 100, 0, 128, 0, 64, 10, 64, 0, 0, 0, 0, 0), "FEAT", "wide_beam_search_feat_kernel<1, 5, 16>", 12, 20672),
    ((768, 768, 1025, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0), 1, "recompute-on index: feature width 1025 > 1024 not supported"),
    ((768, 768, 256, 0, 32, 0, 64, 10, 64, 0, 1, 0, 0, 0), 5, "recompute-on index: construction searches are not supported"),
    # ... threshold 512 | 513 (not 384 / 640), LEANN_DEBUG_NW ignored, 12 bits up to ef 64 at any width
    ((768, 768, 100, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0), "FEAT", "beam_search_feat_kernel<1, 5, 16>", 12, 18368),
    ((768, 768, 100, 0, 32, 0, 513, 10, 64, 0, 0, 0, 0, 0), "FEAT", "beam_search_feat_kernel<1, 5, 4>", 12, 17920),
    ((768, 768, 100, 0, 32, 0, 64, 10, 64, 0, 0, 0, 1, 0), "FEAT", "beam_search_feat_kernel<1, 5, 16>", 12, 18368),
    ((768, 768, 640, 0, 32, 0, 64, 10, 65, 0, 0, 0, 0, 0), "FEAT", "beam_search_feat_kernel<4, 4, 16>", 13, 34784),
    ((768, 768, 256, 0, 32, 0, 64, 10, 342, 0, 0, 0, 0, 0), "FEAT256", "beam_search_feat256_kernel<1, 16>", 14, 71968),
    ((768, 768, 256, 0, 32, 0, 64, 10, 64, 0, 0, 8, 0, 0), "FEAT256", "beam_search_feat256_kernel<1, 16>", 8, 3008),
    ((768, 768, 256, 0, 32, 0, 64, 10, 5000, 0, 0, 0, 0, 0), 1, "search: complexity 5000 needs 212032 B of LDS per query (> 160 KiB)"),
]


@pytest.fixture(scope="module")
def selftest():
    subprocess.check_call(["make", "-s", "-C", ROOT, "leann-rs_amd/host/search_plan_selftest"])  # a no-op when up to date
    return EXE


def test_invariants_over_the_grid(selftest):
    p = subprocess.run([selftest], stdout=subprocess.PIPE, check=False)
    r = json.loads(p.stdout)
    assert r["cases"] == (2 * 1025 + 1100) * 8 * 7 * 4 * 8 * 6
    assert r["accepted"] + r["refused_build"] + r["refused_width"] + r["refused_lds"] == r["cases"]
    assert r["accepted"] > 0 and r["refused_build"] > 0 and r["refused_width"] > 0 and r["refused_lds"] > 0
    for key in ("bad_family", "bad_lds", "bad_limit", "bad_nw", "bad_nbuf", "bad_screen", "bad_wide", "bad_hash", "bad_width", "bad_name",
                "bad_refusal"):
        assert r[key] == 0, r
    assert r["kernels"] == 154 + 60, r  # the grid reaches every kernel api.hip and search_bf16.hip compile, and names no other
    assert p.returncode == 0


def test_plans_written_by_hand(selftest):
    cases = "".join(" ".join(str(v) for v in row[0]) + "\n" for row in EXPECTED)
    p = subprocess.run([selftest, "--plans"], input=cases.encode(), stdout=subprocess.PIPE, check=True)
    got = [json.loads(line) for line in p.stdout.decode().splitlines()]
    assert len(got) == len(EXPECTED)
    for row, g in zip(EXPECTED, got):
        if len(row) == 3:
            assert (g["err"], g["msg"]) == row[1:], (row, g)
        else:
            assert (g["err"], g["family"], g["name"], g["hash_bits"], g["lds_bytes"]) == (0,) + row[1:], (row, g)


def test_expected_rows_name_the_kernels_of_the_gpu_suites():
    """every kernel the docstrings of test_gpu_kernel_matrix.py and test_gpu_bf16_rows.py name is an expected name above"""
    names = {row[2] for row in EXPECTED if len(row) == 5}
    for T, R in {1: 4, 2: 4, 3: 4, 4: 3, 6: 2, 8: 2, 12: 1, 16: 1}.items():
        for nw in (16, 8, 4):
            assert f"beam_search_kernel<{T}, {R}, {nw}, false>" in names and f"beam_search_filtered_kernel<{T}, {R}, {nw}>" in names
    for T, (r4, r16) in {1: (8, 4), 2: (8, 4), 3: (8, 4), 4: (6, 4), 6: (4, 3), 8: (4, 2), 12: (2, 1), 16: (2, None)}.items():
        assert f"bf16_beam_search_kernel<{T}, {r4}, 4>" in names and (r16 is None or f"bf16_beam_search_kernel<{T}, {r16}, 16>" in names)
    for name in ("beam_search_screen_kernel<3, 4>", "beam_search_screen_kernel<6, 2>", "beam_search_kernel<3, 4, 4, true>",
                 "wide_beam_search_kernel<3, 4, 16, true>", "wide_beam_search_kernel<1, 4, 16, false>", "wide_beam_search_filtered_kernel<1, 4, 4>",
                 "beam_search_feat256_kernel<1, 16>", "beam_search_feat256_kernel<1, 4>", "beam_search_feat256_filtered_kernel<1, 16>",
                 "beam_search_feat256_filtered_kernel<1, 4>", "wide_beam_search_feat256_kernel<1, 4>", "wide_beam_search_feat_kernel<1, 5, 16>",
                 "bf16_beam_search_filtered_kernel<3, 8, 4>", "wide_bf16_beam_search_kernel<1, 4, 16>"):
        assert name in names
    for T, R in ((1, 5), (2, 6), (4, 4)):
        for nw in (16, 4):
            assert f"beam_search_feat_kernel<{T}, {R}, {nw}>" in names and f"beam_search_feat_filtered_kernel<{T}, {R}, {nw}>" in names
