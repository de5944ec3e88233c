"""The dispatch decisions of scv_aggregate_i32 / scv_aggregate_prefix_i32 on the CPU: csrc/scvote_plan.h (plain C++, the code launch_aggregate and
launch_prefix of csrc/scvote.hip run) is compiled with g++ through tests/plan_check.cpp, asked once for every case below, and compared with the
regimes stated HERE by hand -- from DESIGN.md section 3 and the comments of the dispatch -- on both sides of every boundary.  Nothing here is a
port of the C++: an expectation is a literal, with the arithmetic that gives it beside it where it is not obvious.

Defaults of a context on an MI355X: 256 CUs, 160 KiB of LDS, tiny_n_max 32, sort_n_min 8, sort_n_max 64, reg_n_max 8192, fused_counters_max 512,
split_seg_kb 256."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# (options, query, expected output line)
CASES = []


def case(query, want, **opts):
    CASES.append((opts, query, " ".join(str(w) for w in want) if isinstance(want, (tuple, list)) else str(want)))


# ---- vote-count roundings: N -> scv_lane_cells | scv_lane_prefix | scv_sort_cells (8 .. 64 in steps of 8) | scv_sort_prefix (32 / 64 / 128)
for n, want in ((1, (4, 4, 8, 32)), (4, (4, 4, 8, 32)), (5, (8, 8, 8, 32)), (8, (8, 8, 8, 32)), (9, (16, 16, 16, 32)), (16, (16, 16, 16, 32)),
                (17, (32, 32, 24, 32)), (24, (32, 32, 24, 32)), (25, (32, 32, 32, 32)), (32, (32, 32, 32, 32)), (33, (32, 64, 40, 64)),
                (40, (32, 64, 40, 64)), (41, (32, 64, 48, 64)), (48, (32, 64, 48, 64)), (49, (32, 64, 56, 64)), (56, (32, 64, 56, 64)),
                (57, (32, 64, 64, 64)), (64, (32, 64, 64, 64)), (65, (32, 64, 64, 128)), (128, (32, 64, 64, 128))):
    case(f"nv {n}", want)
case("lanelds 1 4", 40)            # 5 classes -> 6 words (even) = 24 bytes, + 2 sums of 8 bytes
case("lanelds 8 32", 1184)         # 8 * 33 = 264 words = 1056 bytes, + 16 sums = 128 bytes

# ---- kernel kind: kind N B rows_aligned tok pool_rows ---------------------------------------------------------------------------------
# the sort range, aligned rows: from sort_n_min = 8 (below: one lane per cell), to 64
case("kind 4 1 1 0 0", "LANE")
case("kind 8 1 1 0 0", "SORT")
case("kind 64 1 1 0 0", "SORT")
case("kind 68 1 1 0 0", "REG")
case("kind 65 1 0 0 0", "REG")
# ... rows that are not 16-byte aligned: from 5
case("kind 4 1 0 0 0", "LANE")
case("kind 5 1 0 0 0", "SORT")
case("kind 63 1 0 0 0", "SORT")
case("kind 3 1 0 0 0", "SORT", sort_n_min=3)      # a lower sort_n_min moves both ends
case("kind 2 1 0 0 0", "LANE", sort_n_min=3)
case("kind 4 1 1 0 0", "SORT", sort_n_min=4)
# path = 5 (forced): every length the kernel can take -- 4 aligned, 1 unaligned
case("kind 4 1 1 0 0", "SORT", path=5)
case("kind 1 1 0 0 0", "SORT", path=5)
case("kind 68 1 1 0 0", "REG", path=5)
case("kind 8196 1 1 0 0", "STREAM", path=5)
case("kind 32 1 1 0 0", "SORT", sort_n_max=32)
case("kind 36 1 1 0 0", "REG", sort_n_max=32)
# tiny_n_max = 32: visible with the sort off, and for pool rows (never sorted)
case("kind 32 1 1 0 0", "LANE", sort_n_max=0)
case("kind 33 1 0 0 0", "REG", sort_n_max=0)
case("kind 32 4 1 0 1", "LANE")
case("kind 64 4 1 0 1", "REG")
# tokens: one lane per cell up to 16 votes, the register-resident kernels from 17
case("kind 16 1 1 1 0", "LANE", sort_n_max=0)
case("kind 17 1 0 1 0", "REG", sort_n_max=0)
case("kind 17 1 0 0 0", "LANE", sort_n_max=0)
case("kind 16 4 1 1 1", "LANE")
case("kind 20 4 1 1 1", "REG")
# reg_n_max, and the 8192 slots of the largest register shape (unaligned rows need N + 3)
case("kind 8192 1 1 0 0", "REG")
case("kind 8196 1 1 0 0", "STREAM")
case("kind 8193 1 0 0 0", "STREAM")
case("kind 8189 1 0 0 0", "REG")          # 8192 slots
case("kind 8190 1 0 0 0", "STREAM")       # 8193
case("kind 1024 1 1 0 0", "REG", reg_n_max=1024)
case("kind 1028 1 1 0 0", "STREAM", reg_n_max=1024)
case("kind 100 1 1 0 0", "STREAM", reg_n_max=0)
case("kind 8192 1 1 0 0", "REG", path=4)
case("kind 8190 1 0 0 0", "STREAM", path=4)
for p in (1, 2, 3):
    case("kind 8 1 1 0 0", "STREAM", path=p)
# many budgets: a lane kernel's tables ((B (nv + 1) words, even) + 16 B bytes) pass 60 KiB = 61440 bytes
#   nv = 4:  B = 1706: 8530 words = 34120, + 27296 = 61416;  B = 1707: 8536 words = 34144, + 27312 = 61456
case("kind 4 1706 1 0 0", "LANE")
case("kind 4 1707 1 0 0", "REG")
#   nv = 32: B = 415: 13696 words = 54784, + 6640 = 61424;   B = 416: 13728 words = 54912, + 6656 = 61568
case("kind 32 415 1 0 1", "LANE")
case("kind 32 416 1 0 1", "REG")
# the sorted-cells launch did not fit: one lane per cell while its tables fit (nv = 8: B = 1181: 10630 words = 42520, + 18896 = 61416;
# B = 1182: 10638 words = 42552, + 18912 = 61464), else the register-resident kernels
case("sortfb 8 1181", "LANE")
case("sortfb 8 1182", "REG")
case("sortfb 40 1", "REG")

# ---- 4-byte records (SCV_FLAG_PACKED_CELLS, N <= 127): packed kind g v h -> served; kind 0 LANE 1 SORT 2 REG 3 STREAM.  Only the kernels that call
# pack_cell write them: one lane per cell, sorted cells, the sparse register shapes.  The rows below walk the options that move such cells to
# another kernel, on both sides: kind says who runs, shape which register shape, packed whether launch_cells serves the call.
case("packed 0 0 0 0", 1)
case("packed 1 0 0 0", 1)
case("packed 2 16 1 0", 1)
case("packed 2 8 3 0", 1)
case("packed 2 8 4 0", 1)
case("packed 2 16 2 0", 1)
case("packed 2 0 4 1", 0)                 # the dense parts write 16-byte records
case("packed 2 0 4 8", 0)
case("packed 3 0 0 0", 0)                 # so does the streaming kernel (and scv_reduce_cells reads them)
case("packed 3 16 1 0", 0)
# reg_n_max at N and at N - 1, N = 100 (aligned rows) and N = 101 (unaligned)
case("kind 100 1 1 0 0", "REG", reg_n_max=100)
case("kind 100 1 1 0 0", "STREAM", reg_n_max=99)
case("kind 101 1 0 0 0", "REG", reg_n_max=101)
case("kind 101 1 0 0 0", "STREAM", reg_n_max=100)
case("kind 65 1 0 0 0", "STREAM", reg_n_max=64)
case("kind 127 1 0 0 0", "STREAM", reg_n_max=0)
# N = 40: the sort on / off, reg_n_max at N and at N - 1 (tiny_n_max = 32 is below)
case("kind 40 1 1 0 0", "SORT", reg_n_max=39)                   # the sort is asked first: reg_n_max does not matter
case("kind 40 1 1 0 0", "REG", sort_n_max=0, reg_n_max=40)
case("kind 40 1 1 0 0", "STREAM", sort_n_max=0, reg_n_max=39)
case("kind 40 1 1 0 0", "STREAM", sort_n_max=32, reg_n_max=39)   # (switched off for this N by its upper bound)
case("kind 32 1 1 0 0", "LANE", sort_n_max=0, reg_n_max=0)      # up to tiny_n_max one lane per cell whatever reg_n_max
case("kind 33 1 0 0 0", "STREAM", sort_n_max=0, reg_n_max=32)
case("kind 20 1 1 1 0", "REG", sort_n_max=0, reg_n_max=0)       # tokens from 17 votes: LANE hands over to REG after reg_n_max was asked
# the sorted launch that does not fit falls back to LANE or REG, never to the streaming kernel
case("sortfb 40 1", "REG", reg_n_max=0)
case("sortfb 100 1", "REG", reg_n_max=0)
# forced dense codes are honoured at N = 100 (1024 .. 8192 slots), forced sparse codes give sparse shapes, codes too small fall back to sparse
for code, h in ((1041, 1), (1042, 2), (1044, 4), (1048, 8)):
    case(f"shape 100 {code} 0", (0, 4, h))
    case(f"shape 103 {code} 0", (0, 4, h))                       # N = 100 in unaligned rows
for code, want in ((1601, (8, 4, 0)), (1602, (16, 2, 0)), (1604, (16, 4, 0)), (3204, (32, 4, 0)), (6404, (64, 4, 0)), (803, (8, 4, 0)), (804, (8, 4, 0))):
    case(f"shape 100 {code} 1", want)                            # (1601 / 803: 64 / 96 slots are too few for 100 -> the auto shape (8, 4))
case("shape 100 0 0", (8, 4, 0))
case("shape 64 1041 0", (0, 4, 1))
case("shape 1 1048 0", (0, 4, 8))

# ---- register shape: shape Nreg forced have_g8 -> g v h ---------------------------------------------------------------------------------
for nreg, want in ((64, (16, 1, 0)), (65, (8, 3, 0)), (96, (8, 3, 0)), (97, (8, 4, 0)), (128, (8, 4, 0)), (129, (16, 4, 0)), (256, (16, 4, 0)),
                   (257, (32, 4, 0)), (512, (32, 4, 0)), (513, (64, 4, 0)), (896, (64, 4, 0)), (897, (0, 4, 1)), (1024, (0, 4, 1)),
                   (1025, (0, 4, 2)), (2048, (0, 4, 2)), (2049, (0, 4, 4)), (4096, (0, 4, 4)), (4097, (0, 4, 8)), (8192, (0, 4, 8))):
    case(f"shape {nreg} 0 0", want)
# forced shapes that are honoured
case("shape 100 1602 0", (16, 2, 0))       # 128 slots
case("shape 64 804 1", (8, 4, 0))
case("shape 64 3204 0", (32, 4, 0))
case("shape 64 6404 0", (64, 4, 0))
case("shape 500 1041 0", (0, 4, 1))
case("shape 500 1042 0", (0, 4, 2))
case("shape 500 1044 0", (0, 4, 4))
case("shape 500 1048 0", (0, 4, 8))
# ... and ignored: too small for the row, not instantiated, unknown
case("shape 129 1602 0", (16, 4, 0))
case("shape 1025 1041 0", (0, 4, 2))
case("shape 64 804 0", (16, 1, 0))         # (8, 4) exists in A/B builds only
case("shape 64 1603 0", (16, 1, 0))
case("shape 500 1043 0", (32, 4, 0))
case("shape 500 1050 0", (32, 4, 0))
case("shape 500 999 0", (32, 4, 0))
case("shape 500 6408 0", (32, 4, 0))
# the grid: what is needed when that is resident; else the stride grid * WPG is kept coprime with B (or grid itself is)
case("reggrid 512 100 16 8", 7)
case("reggrid 256 1000000 16 1", 256)
case("reggrid 256 1000000 16 3", 256)
case("reggrid 256 1000000 16 8", 255)

# ---- streaming bands: band N ncells -> copies threads wg_per_cu unroll lds; lds = (1024 copies + 96 + 512) words ----------------------
case("band 4095 10000", (4, 256, 8, 2, 18816))
case("band 4096 10000", (8, 256, 4, 4, 35200))
case("band 32767 10000", (8, 256, 4, 4, 35200))
case("band 32768 10000", (16, 512, 2, 4, 67968))
case("band 262143 10000", (16, 512, 2, 4, 67968))
case("band 262144 10000", (16, 1024, 1, 4, 67968))
# no more cells than CUs: the widest workgroup, from 4096 votes
case("band 4096 256", (16, 1024, 1, 4, 67968))
case("band 4096 257", (8, 256, 4, 4, 35200))
case("band 4095 256", (4, 256, 8, 2, 18816))
# scv_set_tuning: the geometry as given, workgroups per CU capped by 160 KiB / lds = 2 and by 2048 / threads
case("band 100 10000", (16, 256, 2, 4, 67968), user_tuned=1, copies=16, threads=256, wg_per_cu=8, unroll=4)
case("band 100 10000", (4, 1024, 2, 4, 18816), user_tuned=1, copies=4, threads=1024, wg_per_cu=8, unroll=4)

# ---- split-N: split N ncells slots -> S seg_len ---------------------------------------------------------------------------------------
case("split 1048576 128 256", (2, 524288))          # 2 * 128 <= 256 slots: two segments of 2 MiB
case("split 1048576 129 256", (1, 1048576))
case("split 262144 1 256", (4, 65536))              # N * 4 = 2^20: on; segments of at least 256 KiB -> 4
case("split 262143 1 256", (1, 262143))
case("split 1048576 512 2048", (4, 262144))         # one arrival counter per split cell: 512 of them
case("split 1048576 513 2048", (1, 1048576))
case("split 65536 2 256", (1, 65536), split_seg_kb=64)
case("split 65536 2 256", (4, 16384), split_seg_kb=64, path=2)       # path = 2 splits whatever the size; 256 KiB / 64 KiB = 4
case("split 1048576 513 2048", (1, 1048576), path=2)                   # ... but not more than 512 cells
case("split 1000 2 256", (3, 336), path=2, segs_override=3)          # ceil(1000 / 3) = 334 -> 336: a multiple of 4 votes
case("split 1000 2 256", (1, 1000), segs_override=3)                 # (the override counts only where the split is on)
case("split 16777216 1 256", (4096, 4096), path=2, segs_override=5000)
case("split 1073741824 1 8192", (4096, 262144))                       # min(8192 slots, 2^32 / 2^18 = 16384) -> the cap of 4096
case("split 1048578 1 256", (16, 65540))                              # ceil(1048578 / 16) = 65537 -> 65540
for p in (1, 3):
    case("split 1048576 1 256", (1, 1048576), path=p)

# ---- the smallest grid with the same number of rounds; the dispenser ------------------------------------------------------------------
case("grid 10000 256 0", 250)              # 40 rounds either way
case("grid 100 256 0", 100)
case("grid 257 256 0", 129)                # 2 rounds
case("grid 10000 256 100", 100)            # a forced grid is taken as it is ...
case("grid 50 256 100", 50)                # ... up to the number of items
case("disp 10000 250 1048576", 1)
case("disp 10000 250 1048575", 0)          # items of 2^20 votes at least
case("disp 250 250 1048576", 0)            # one item per workgroup: nothing to hand out
case("disp 2147483647 256 1048576", 1)
case("disp 2147483648 256 1048576", 0)     # tickets are 32-bit
case("disp 10000 250 1048576", 0, path=3)

# ---- counters: where they are computed ------------------------------------------------------------------------------------------------
# reduce want streaming ncells B N
case("reduce 1 1 512 1 1000", 0)
case("reduce 1 1 513 1 1000", 1)
case("reduce 1 1 513 1 1048576", 0)        # rows of 4 MiB: fused whatever the number of cells
case("reduce 1 0 100000 1 100", 0)         # the cell kernels count in LDS
case("reduce 0 1 513 1 1000", 0)
case("reduce 1 0 10 1 100", 1, fused_counters_max=0)
case("reduce 0 0 10 1 100", 0, fused_counters_max=0)
# overwrite inside the launch: few cells, few budgets, whole cells, a geometry with the epilogue
case("owfew 1 8192 64", 1, overwrite_counters=1)
case("owfew 1 8193 64", 0, overwrite_counters=1)
case("owfew 1 8192 65", 0, overwrite_counters=1)
case("owfew 0 8192 64", 0, overwrite_counters=1)
case("owfew 1 8192 64", 0)
# chunks of scv_reduce_cells: 2048 problems each, at most ceil(8 * 256 CUs / B)
case("chunks 2048 1", 1)
case("chunks 2049 1", 2)
case("chunks 10000000 1", 2048)
case("chunks 100000 512", 4)
case("chunks 0 4", 1)
# tie classes in LDS: tcl spare_words B N -> (spare - 4 B - 2) / B, at most min(N, 1024) + 1; kept from 8, or when it is all of them
case("tcl 554 8 64", 65)
case("tcl 553 8 64", 64)                   # below full
case("tcl 98 8 64", 8)
case("tcl 97 8 64", 0)                     # 7: below 8
case("tcl 74 8 4", 5)                      # all 5 classes of 4 votes
case("tcl 73 8 4", 0)
case("tcl 34 8 64", 0)
case("tcl 100000 8 5000", 1025)
# grid * cells per workgroup a multiple of B
case("bgrid 256 1024 3", 255)
case("bgrid 256 1024 4", 256)
case("bgrid 2 1024 3", 2)                  # (not below B workgroups)

# bytes of those classes: (B tcl words, even) + 4 B words
case("tclds 8 65", 2208)                   # 520 + 32 words
case("tclds 3 5", 112)                     # 15 -> 16 words, + 12
# the n_valid cache of the cell kernels: B rounded up to 4 words, none without n_valid or above 512 budgets
case("nvc 1 8", 8)
case("nvc 1 9", 12)
case("nvc 1 512", 512)
case("nvc 1 513", 0)
case("nvc 0 8", 0)
# one lane per cell: lanegrid ncells nv tok B -> workgroups of 1024 threads (512 with 32 votes, or 16 and tokens), one per CU at most,
# grid * threads a multiple of B when the grid is above B
case("lanegrid 2048 4 0 1", 2)
case("lanegrid 2049 4 0 1", 3)
case("lanegrid 2048 32 0 1", 4)
case("lanegrid 2048 16 1 1", 4)
case("lanegrid 2048 16 0 1", 2)
case("lanegrid 10000000 8 0 1", 256)
case("lanegrid 10000000 8 0 3", 255)
case("lanegrid 2048 4 0 3", 2)

# ---- cells of exactly 1 / 2 / 4 votes: few N B ncells bases_aligned pool_rows grid_override -> ok one grid -------------------------------
case("few 1 8 32768 1 0 0", (1, 1, 8))                 # 128 blocks of 256 cells, 16 per workgroup
case("few 2 8 32768 1 0 0", (1, 1, 16))
case("few 4 1 128 1 0 0", (1, 0, 1))
case("few 4 1 100 1 0 0", (0, 0, 1))                   # a ragged last block: scv_lane_cells
case("few 1 1 1000 1 0 0", (0, 0, 1))
case("few 1 1 65537 1 0 0", (1, 1, 16))                # large launches: the one-vote kernel takes the ragged end too
case("few 1 3 3145728 1 0 0", (1, 1, 510))             # 512 workgroups x 4096 cells is no multiple of 3: 510
case("few 1 3 3145728 1 0 7", (1, 0, 7))               # forced grid: 7 x 4096 is no multiple of 3 -> scv_few_votes (whole blocks only)
case("few 1 3 3145728 1 0 6", (1, 1, 6))
case("few 3 1 768 1 0 0", (0, 0, 0))
case("few 1 8 32768 0 0 0", (0, 0, 0))
case("few 1 8 32768 1 1 0", (0, 0, 0))
# the one-vote kernel keeps 32 bytes per budget in LDS, 60 KiB at most: 1920 budgets (forced grids whose step, grid x 4096 cells, is a multiple of B)
case("few 1 1920 7864320 1 0 15", (1, 1, 15))
case("few 1 1921 7868416 1 0 1921", (1, 0, 1921))      # 61472 bytes: scv_few_votes

# ---- sorted cells: sortw waves N tok lin has_n_valid B -> region_words tail_words W ------------------------------------------------------
case("sortw 16 64 0 0 1 8", (4416, 560, 8))            # 17 x 256 + 64 words a wave; 9 fit 160 KiB -> whole waves per SIMD: 8
case("sortw 16 64 1 0 1 8", (8768, 560, 4))
case("sortw 16 40 0 0 0 1", (2880, 46, 12))            # 14 fit -> 12
case("sortw 16 30 0 1 0 1", (2112, 38, 16))            # linear image: 7696 bytes -> 8 KiB; tail: 33 classes -> 34 words, + 4
case("sortw 16 64 0 0 1 512", (4416, 35840, 0))        # 512 budgets x 65 classes: one wave fits, four are needed
case("sortw 8 64 0 0 1 512", (4416, 35840, 0))
case("sortw 8 64 0 0 0 400", (4416, 27600, 3))         # 110400 + 3 x 17664 = 163392 bytes fit 163840, 4 do not
# sort-prefix: spw waves N tail_words -> region_words W (at least 2 waves)
case("spw 16 64 1000", (4416, 8))
case("spw 16 128 1000", (4416, 8))
case("spw 16 20 1000", (1344, 16))
case("spw 16 64 1000", (4416, 0), lds_max=32768)

# ---- prefix budgets -------------------------------------------------------------------------------------------------------------------
# plane B N tok -> ok nv threads lds lds_total
case("plane 4 64 0", (1, 64, 256, 1136, 17520))
case("plane 4 65 0", (0, 0, 0, 0, 0))
case("plane 8 16 0", (1, 16, 1024, 736, 131808))
case("plane 37 64 0", (1, 64, 256, 10512, 162064))     # snapshots of 4 waves: 4 x 64 x 37 x 16 bytes
case("plane 38 64 0", (0, 64, 0, 10792, 0))
case("plane 25 64 1", (1, 64, 256, 7104, 160704))      # 24 bytes a snapshot with tokens
case("plane 26 64 1", (0, 64, 0, 7384, 0))
case("plane 86 64 0", (1, 64, 256, 24424, 376688), lds_max=1 << 20)      # the 24 KiB table limit (seen only with more LDS than 160 KiB)
case("plane 87 64 0", (0, 64, 0, 24712, 0), lds_max=1 << 20)
case("plane 513 4 0", (0, 0, 0, 0, 0))
case("plane 4 64 0", (0, 0, 0, 0, 0), path=1)
# served n N: 0, a power of two <= np (16 / 32 / 64 for pools up to 32 / 64 / 128), or the whole row
for n, N, want in ((0, 64, 1), (64, 64, 1), (100, 64, 1), (32, 64, 1), (33, 64, 0), (48, 64, 0), (1, 64, 1), (16, 24, 1), (12, 24, 0), (32, 48, 1),
                   (40, 48, 0), (64, 128, 1), (96, 128, 0), (128, 128, 1), (32, 32, 1), (128, 200, 0), (64, 200, 1), (-1, 64, 1)):
    case(f"served {n} {N}", want)
# spe P B N rows_aligned
case("spe 10 4 64 1", 1)
case("spe 10 4 20 1", 1)
case("spe 10 4 16 1", 0)
case("spe 10 4 64 0", 0)
case("spe 57343 4 128 1", 0)
case("spe 57344 4 128 1", 1)
case("spe 57343 4 68 1", 0)
case("spe 10 4 128 1", 1, prefix_path=5)
case("spe 10 4 132 1", 0, prefix_path=5)
case("spe 10 513 64 1", 0)
case("spe 10 4 64 1", 0, sort_n_max=32)
case("spe 10 4 64 1", 0, fused_counters_max=0)
case("spe 10 4 64 1", 0, path=1)
case("spe 10 4 64 1", 0, prefix_path=1)
# form B N rows_aligned lane_fits skip_sortable
case("form 4 64 1 1 0", "LANE")
case("form 4 64 1 1 1", "LANE")
case("form 40 64 1 0 0", "POOL")
case("form 4 100 1 0 0", "POOL")
case("form 4 4096 1 0 0", "POOL")
case("form 4 4100 1 0 0", "HIST")
case("form 513 100 1 0 0", "CELLS")
case("form 4 256 1 0 0", "CELLS", prefix_path=2)
case("form 4 4094 0 0 0", "HIST", prefix_path=2)       # 4097 slots
case("form 4 8 1 1 0", "CELLS", prefix_path=2)
case("form 4 8 1 1 0", "POOL", prefix_path=4)
case("form 4 8 1 1 0", "LANE", prefix_path=1)
case("form 4 100 1 0 0", "HIST", prefix_path=1)
case("form 4 8 1 1 0", "HIST", prefix_path=3)
case("form 4 8 1 1 0", "LANE", prefix_path=5)
# rows B N rows_aligned: pool rows through the cell kernels
case("rows 415 32 1", 1)
case("rows 416 32 1", 0)
case("rows 1 33 0", 1)
case("rows 1 4096 1", 1)
case("rows 1 4100 1", 0)
case("rows 1 4093 0", 1)
case("rows 1 4094 0", 0)
case("rows 1 1028 1", 0, reg_n_max=1024)
case("rows 1 64 1", 0, path=1)
# ppl N rows_aligned: lanes per problem of scv_prefix_pool
case("ppl 1024 1", 16)
case("ppl 1028 1", 32)
case("ppl 2000 0", 16)
case("ppl 100 1", 32, reg_shape=32)
case("ppl 2048 1", 16, reg_shape=16)
case("ppl 2048 1", 32, reg_shape=64)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "plan_check.cpp")])
    lines = []
    for opts, query, _ in CASES:
        lines.append("reset")
        lines += [f"opt {k} {int(v)}" for k, v in opts.items()]
        lines.append(query)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert len(out) == len(CASES)
    return out


def test_every_decision_is_the_stated_one(answers):
    wrong = [(opts, query, want, got) for (opts, query, want), got in zip(CASES, answers) if got != want]
    assert not wrong, "\n".join(f"{q} {o}: stated {w}, plan says {g}" for o, q, w, g in wrong)


def test_the_boundaries_of_the_issue_are_covered():
    """Every family of decisions is asked, and each on more than one side."""
    by = {}
    for _, query, want in CASES:
        by.setdefault(query.split()[0], set()).add(want)
    for q in ("nv", "kind", "sortfb", "packed", "shape", "reggrid", "band", "split", "grid", "disp", "reduce", "owfew", "chunks", "tcl", "tclds", "nvc", "lanegrid", "bgrid",
              "few", "sortw", "spw", "plane", "served", "spe", "form", "rows", "ppl"):
        assert len(by.get(q, ())) >= 2, q
    assert by["kind"] == {"LANE", "SORT", "REG", "STREAM"} and by["form"] == {"POOL", "CELLS", "LANE", "HIST"}


def test_split_segments_are_multiples_of_four_and_capped(answers):
    for (_, query, _), got in zip(CASES, answers):
        if query.startswith("split "):
            S, seg = (int(x) for x in got.split())
            N = int(query.split()[1])
            assert 1 <= S <= 4096 and (S == 1 or (seg % 4 == 0 and seg * S >= N)), query


def test_the_plan_header_has_no_hip_and_no_context_in_it():
    src = open(os.path.join(os.path.dirname(HERE), "o1_inference_scaling_laws_amd", "csrc", "scvote_plan.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.split("\n"))
    assert "hip" not in code.lower() and "scv_ctx" not in code and "#include \"" not in code
    hip = open(os.path.join(os.path.dirname(HERE), "o1_inference_scaling_laws_amd", "csrc", "scvote.hip")).read()
    assert '#include "scvote_plan.h"' in hip and "plan::cell_kind(" in hip and "plan::prefix_form(" in hip      # the library runs this header
