/*
 * scvote.h -- C ABI of the MI355X-native self-consistency aggregation engine.
 *
 * This is the drop-in boundary for ONE hot path of hughbzhang/o1_inference_scaling_laws:
 * the majority-vote / tie-aware scoring / per-budget reduction behind
 *
 *     o1.py:167  process_single_example(example, token_limit, cache, N) -> (score, total_tokens)
 *     o1.py:216  run_experiments(dataset, cache, token_limit, N)        -> (accuracy, avg_tokens_used)
 *
 * The reference has no FFI of its own (it is 421 lines of Python); these entry points are what a
 * ctypes binding for that path binds (see INTEGRATION.md for the stub a maintainer adds to o1.py).
 * Everything here is plain C: pointers, sizes, fixed-width integers.  No torch / numpy types.
 *
 * Data model:
 *   answers  int32 [P, B, N]  row-major, N contiguous.  One element = one sample-vote.
 *                             Value domain: bins 0..1023 (AIME answers 0..999 + 24 spare bins the
 *                             host-side extractor uses to dictionary-encode out-of-domain ints).
 *   tokens   int32 [P, B, N]  optional second stream (completion tokens of each sample).
 *   n_valid  int32 [B]        optional: budget b votes over the prefix answers[p,b,0:n_valid[b]]
 *                             (o1.py:274-276: N = token_limit // min(2**11, token_limit)).
 *   truth    int32 [P]        ground-truth bin of each problem (o1.py:206 int(example['answer'])).
 *
 * Per (problem, budget) cell the engine produces one scv_cell; per budget it produces integer
 * counters from which the host computes the reference's floats in ONE canonical order
 * (o1.py:244-245).  All device outputs are integers => bit-exact at any GPU count.
 */
#ifndef SCVOTE_H
#define SCVOTE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCV_NUM_BINS 1024         /* histogram bins per cell (0..999 answers + 24 spare)        */
#define SCV_TIE_CLASSES 1025      /* tie_class_hits[b][m], m = n_modes in 0..1024               */

/* mem_kind: where every pointer argument of a call lives. */
#define SCV_MEM_HOST 0            /* host pointers; staged through HBM in problem-chunks by a 3-stage
                                     pipeline (threads -> pinned bounce -> DMA -> kernel); blocking */
#define SCV_MEM_DEVICE 1          /* device pointers; async on the ctx stream, caller syncs     */

/* scv_create flags */
#define SCV_FLAG_TIMING 0x1u      /* record hipEvents around every aggregation kernel launch    */
#define SCV_FLAG_CLAMP_TO_INVALID_BIN 0x2u /* out-of-domain votes go to bin 1023, no error      */
#define SCV_FLAG_PACKED_CELLS 0x4u /* OPT-IN: scv_aggregate_i32 (DEVICE memory, N <= 127) writes its cell table as uint32_t [P, B], 4 bytes per cell:
                                      max_count | truth_count << 7 | n_modes << 14 | min_mode << 21 | hit << 31 (7 + 7 + 7 + 10 + 1 bits; an empty cell
                                      -- max_count 0 -- has min_mode field 1023 and means -1).  The reference's most common call is N = 1
                                      (o1.py:302) and N = 1, 2, 4, 8 (o1.py:276): a 16-byte scv_cell per 4-byte vote is 80 % of such a launch's traffic.
                                      Everything else (counters, cell_tokens) is unchanged; a call the flag does not cover (prefix budgets, HOST memory,
                                      N > 127, a forced streaming path, vote + bootstrap) with cells_out != NULL is SCV_ERR_ARG -- and so is one
                                      whose options send the cells to a kernel that writes 16-byte records only: the streaming kernel ("reg_n_max"
                                      below N, with the sort off or N > 64) or a dense register shape ("reg_shape" 1041 .. 1048); nothing is queued.
                                      The 4-byte record is written by the one-lane-per-cell kernels, the sorted cells and the sparse register
                                      shapes (csrc/scvote_plan.h packed_ok).  Without a cell table every kernel serves such a context.  Decoder:
                                      o1_inference_scaling_laws_amd/engine.py unpack_cells */

#define SCV_FLAG_OPEN_DOMAIN 0x8u /* OPT-IN: the pool-ordering entries (scv_resample_prefix_i32, scv_expected_majority_i32, scv_token_budget_prefix_i32,
                                      scv_weighted_prefix_i32, scv_adaptive_prefix_i32, scv_iid_prefix_i32, scv_resample_wide_i32 and scv_token_budget_wide_i32 -- rows of up to 4096
                                      values, see there for tie classes beyond the table --, and scv_shortest_prefix_i32, which reaches
                                      the same row encoder and whose cells_out[..].min_mode is then the CODE) take ANY int32 as an answer value: negative
                                      numbers, large integers, 32-bit hashes of normalised answer strings.  Two votes are the same value only when
                                      the integers are equal.  A vote's code is the rank of its value among the distinct values of the whole row
                                      pool[p, 0:N] in ascending SIGNED order -- what the byte codes of these entries already are for rows inside
                                      0..1023 -- and everything downstream walks codes, so nothing else changes: the permutation for (seed, pg, r),
                                      the draw streams, the token sums; slices of r and shards of p still add up bit for bit; HOST mode and hipGraph
                                      capture work as without the flag.  The truth hits exactly when it equals a modal value, whatever its
                                      magnitude.  Under the flag these entries never set error bit 0 (no SCV_ERR_DOMAIN), and
                                      SCV_FLAG_CLAMP_TO_INVALID_BIN has no effect on them; every other error bit (1, 4, 5, 6, 7, 8) keeps its meaning.
                                      cells_out[..].min_mode (SCV_ORDER_POOL calls of the token-budget, weighted and adaptive entries) is then the
                                      CODE of the smallest modal value, 0 .. distinct - 1, or -1 for the empty cell -- not the value, which an
                                      int16 cannot hold; o1_inference_scaling_laws_amd/engine.py decode_min_mode turns it back into the value.
                                      With the flag off every entry behaves as before.  The dense entries (scv_aggregate_i32, scv_aggregate_prefix_i32,
                                      scv_aggregate_bootstrap_i32, scv_bootstrap, scv_synth_fill_i32) ignore the flag in both states: they keep
                                      the 1024 bins, and an out-of-domain vote is SCV_ERR_DOMAIN there as always.  Cost: the row encoder ranks by
                                      counting in registers (csrc/scvote_resample.hip.h resample_encode_row_open), N broadcast steps per row. */

/* synthetic distributions */
#define SCV_DIST_UNIFORM 0        /* D0: uniform over 0..999                                    */
#define SCV_DIST_PEAKED 1         /* D1: truth w.p. q_p in {.1...7}, 4 distractors at .05, rest uniform */
#define SCV_DIST_DEGENERATE 2     /* D2: every vote == truth[p]                                 */
#define SCV_DIST_TIE 3            /* D3: exact 2-/3-way ties, with and without truth among them */
#define SCV_DIST_PEAKED_WRONG 4   /* D4: D1 with the roles swapped: a WRONG value w.p. q_p, truth at .05 -- a confidently
                                     wrong majority, an ordinary outcome of the reference (o1.py:204-213 scores it 0)    */
#define SCV_DIST_DEGENERATE_WRONG 5 /* D5: every vote == one wrong value (truth + 500) % 1000                            */

/* error codes: 0 ok; -(hipError_t) for HIP failures; the following for argument/data errors. */
#define SCV_OK 0
#define SCV_ERR_ARG (-2001)           /* null/negative/oversized argument                       */
#define SCV_ERR_DOMAIN (-2002)        /* a vote outside 0..1023 was seen (results are invalid)  */
#define SCV_ERR_NO_DEVICE (-2003)     /* no HIP device visible                                  */
#define SCV_ERR_NOT_TIMED (-2004)     /* scv_last_kernel_ns without SCV_FLAG_TIMING / no launch */
#define SCV_ERR_ALLOC (-2005)         /* device allocation failed                               */

/*
 * Result of one (problem, budget) cell.  Replaces the return value of
 * statistics.multimode(answers) + the scoring at o1.py:202-213:
 *   score = hit ? 1.0 / n_modes : 0          (o1.py:206,210)
 * truth_count (= histogram[truth]) is the c of the pass@k estimator.
 */
typedef struct scv_cell {
    uint32_t max_count;   /* count of the modal value(s); 0 iff the cell had no valid votes   */
    uint32_t truth_count; /* votes equal to truth[p]                                           */
    uint16_t n_modes;     /* len(statistics.multimode(answers)); 0 iff max_count == 0          */
    int16_t  min_mode;    /* smallest modal bin, -1 iff max_count == 0                         */
    uint8_t  hit;         /* truth[p] in multimode(answers)                                    */
    uint8_t  pad[3];
} scv_cell;               /* 16 bytes */

typedef struct scv_ctx scv_ctx;   /* opaque: device, stream, scratch, timing events           */

/* Create a context bound to `device` (-1 = current HIP device).  One ctx per GPU per process. */
int scv_create(scv_ctx** out, int device, uint32_t flags);
int scv_destroy(scv_ctx* ctx);

/* A new ctx launches on a private non-blocking stream.  scv_set_stream BORROWS the caller's
 * hipStream_t instead (e.g. torch.cuda.current_stream().cuda_stream); NULL is the device's default
 * stream -- which is what torch hands out until the user opens a stream of their own.  Does not
 * synchronise (legal while the new stream is being captured into a hipGraph): every DEVICE-mode
 * entry point only enqueues work, so aggregation + bootstrap can be captured once and replayed. */
int scv_set_stream(scv_ctx* ctx, void* hip_stream);
/* Block until everything queued on the ctx stream has finished; reports SCV_ERR_DOMAIN if a
 * DEVICE-mode aggregation since the last sync saw an out-of-domain vote. */
int scv_sync(scv_ctx* ctx);

/*
 * Streaming-kernel geometry (for A/B measurement; 0 / negative = keep current).  By default the library picks the geometry
 * from the shape (measured bands); any explicit value here switches that off until ALL FOUR arguments are negative
 * (scv_set_tuning(ctx, -1, -1, -1, -1): back to the library's own choice).  Instantiated: (copies, threads) in (4, 256) with unroll 2; (8, 256) (8, 512)
 * (16, 256) (16, 512) (16, 1024) with unroll 4 -- anything else is SCV_ERR_ARG.
 *   copies        LDS sub-histogram replication R        threads     workgroup size
 *   wg_per_cu     persistent workgroups per CU (clamped by LDS and wave capacity)
 *   unroll        16-byte loads in flight per lane
 */
int scv_set_tuning(scv_ctx* ctx, int copies, int threads, int wg_per_cu, int unroll);
/*
 * Launch options.  None is needed for correct results: the defaults are the measured choices (DESIGN_HISTORY.md 4).  The keys exist
 * so that every kernel of the family can be forced (parity tests) and the dispatch bounds re-measured; every choice that was
 * measured slower in rounds 1-3 is gone from the library (DESIGN_HISTORY.md 4 lists them with their numbers).
 *   "overwrite_counters"  default 0; 1: DEVICE-mode per-budget counters are OVERWRITTEN, not accumulated into (with few long cells the
 *                         streaming kernel's last workgroup does it and the call is one launch, otherwise a memset precedes the launch)
 *   "path"                0 auto | 1 streaming, whole cells | 2 streaming, split-N + merge | 4 register-resident cells | 5 sorted cells |
 *                         3 streaming, whole cells, items round-robin over the workgroups.  (0 .. 2: when the items outnumber the workgroups and
 *                         are at least 2^20 votes long, a device counter hands out each workgroup's items after its first, so that the early
 *                         finishers take more; 3 is the order before that, for A/B runs)
 *   "sort_n_min" / "sort_n_max"   defaults 8 / 64: cells of that many votes run one lane per cell, the wave's rows staged through LDS
 *                         by LDS-DMA and sorted in registers (rows that are not 16-byte aligned: from 5); "sort_n_max" = 0: off
 *   "reg_n_max"           default 8192 = its maximum: 32 < N <= this uses the register-resident cell kernels; 0: the streaming kernel
 *   "reg_shape"           force a register-resident shape: g * 100 + v (g lanes per cell, v vectors per lane: 1601 803 804 1602 1604 3204 6404;
 *                         803 / 804 = 8 lanes x 3 / 4 vectors with 8-bit LDS bins, the auto choice for 65 .. 96 / 97 .. 128 slots since round 6 --
 *                         1602 there is round 5's 128-slot shape) or 1041 / 1042 / 1044 / 1048 (dense scan, 1, 2, 4, 8 parts of 4 KiB); a shape too
 *                         small for N is ignored
 *   "auto_geometry"       DEPRECATED alias kept for callers of rounds 1-4: 1 = scv_set_tuning(ctx, -1, -1, -1, -1) (the library picks the
 *                         streaming geometry from the shape), 0 = pin the current geometry
 *   "fused_counters_max"  default 512 (4096 until round 6; re-measured by tools/crossovers.py): streaming kernel -- at or below this many cells (or problem rows >= 4 MiB) per-cell atomics inside
 *                         the hot kernel, otherwise a separate reduction of the cell table; 0: EVERY kernel leaves the counters to that
 *                         reduction (the cell kernels otherwise keep per-workgroup LDS tables and flush them in the same launch)
 *   "grid"                > 0: exact persistent grid (0: from the CU count, balanced so that all workgroups stream the same number of items)
 *   "segs"                split-N segments per cell (0 auto)
 *   "prefix_path"         scv_aggregate_prefix_i32: 0 auto | 1 one lane per problem, every budget out of one pass (pools <= 64) |
 *                         2 the cell kernels on pool rows (pools <= 4096) | 3 one streaming pass, a histogram snapshot per boundary |
 *                         4 one pass per problem over its pool row, 16 / 32 / 64 lanes per problem, every budget a snapshot of the running
 *                         mode statistics (pools <= 4096: auto above 64 votes and for budget lists too long for path 1; "reg_shape" = 16 / 32 forces the lanes per problem)
 *                         auto includes: pools of 17 .. 128 votes (N % 4 == 0, 16-byte aligned bases) whose budgets are all 0, a power of two <= 16 / 32 / 64
 *                         (pools <= 32 / 64 / 128), or >= N come out of ONE sort per problem (scv_sort_prefix) -- pools of 17 .. 64 votes always, pools of
 *                         68 .. 128 votes (scv_sort_prefix2: ~27 us for a launch of one step per wave) from 57 344 pools per call; with tokens their sums
 *                         come from token steps of the same launch (scv_sort_prefix2<true>).  A HOST-mode call reads the budgets; a DEVICE-mode call queues that
 *                         kernel in front of the general one and the two decide from n_valid which of them does the work (~4 us for the one that
 *                         leaves).  | 5 = auto, and the caller PROMISES budgets of that form for such pools (any number of them, with or without
 *                         tokens): a DEVICE-mode call queues scv_sort_prefix alone; a list that breaks the promise computes nothing and is
 *                         SCV_ERR_ARG (at the call in HOST mode, at the next synchronisation in DEVICE mode).  1 .. 4 switch the kernel off
 *   "boot_path"           scv_aggregate_bootstrap_i32: 0 auto (ONE cooperative launch when the shape allows it) | 1 one ORDINARY launch |
 *                         2 two launches, LDS-resident code table | 3 two launches, global gathers (also scv_bootstrap's kernel)
 *   "boot_spin_limit"     default 2^20: polls at the grid barrier before a workgroup of an ordinary one-launch form gives up and leaves
 *                         the bootstrap to scv_sync; tests set 1
 *   "stage_mb"            HOST mode: chunk size of the staging pipeline (default 128)
 *   "host_small_kb"       HOST mode: calls whose inputs + outputs fit in this many KiB (default 1024 -- every call the reference itself
 *                         makes: P = 30, N <= 128, o1.py:277,302) skip the pipeline: one pinned block, one H2D, the kernel, one D2H, one
 *                         stream sync, no threads and no per-call allocation; 0: every HOST call goes through the pipeline
 *   "copy_threads"        HOST mode: threads filling the pinned bounce slots (default 6)
 */
int scv_set_option(scv_ctx* ctx, const char* key, int64_t value);

/*
 * The hot path.  Replaces, for all P problems and B budgets at once,
 *   o1.py:181-195 (vote collection + token sum), o1.py:202 (statistics.multimode),
 *   o1.py:204-213 (tie-aware score) and the integer part of o1.py:229-245 (per-budget sums).
 *
 * Outputs (any may be NULL):
 *   cells_out            scv_cell [P, B]                                                    DEVICE memory: 16-byte aligned
 *   cell_tokens_out      int64    [P, B]   sum of tokens over the valid prefix (o1.py:195); DEVICE memory: 16-byte aligned;
 *                                           written only by a call with tokens, untouched without
 *   tie_class_hits_out   int64    [B, 1025] #problems with hit and n_modes == m  (o1.py:238-239)  DEVICE memory: 8-byte aligned
 *   token_sum_out        int64    [B]       sum over problems of cell_tokens     (o1.py:240,245)  DEVICE memory: 8-byte aligned
 *   truth_count_sum_out  int64    [B]       sum over problems of truth_count                      DEVICE memory: 8-byte aligned
 * In DEVICE mode the three per-budget outputs are ACCUMULATED INTO (+=), so a caller streaming
 * problem-chunks (or ranks before an all-reduce) zeroes them once; in HOST mode they are overwritten.
 * In DEVICE mode the kernels store into the caller's arrays directly, and the alignment above is the widest store each output receives:
 * 16 bytes for the cell tables (whole records; with SCV_FLAG_PACKED_CELLS four / two consecutive 4-byte records per lane at N = 1 / 2 -- a
 * uint32 [P, B] table needs 16 bytes too; two consecutive cell_tokens per lane at N = 1 / 2 and in scv_sort_prefix), 8 bytes for the
 * counters (64-bit atomics and stores).  A pointer below its alignment is SCV_ERR_ARG with nothing queued -- also through
 * scv_aggregate_prefix_i32 and scv_aggregate_bootstrap_i32.  (A row of a larger scv_cell table is always aligned when the table is; a row
 * of a cell_tokens table is when P_row * B is even.)  HOST memory has no such requirement.
 */
int scv_aggregate_i32(scv_ctx* ctx,
                      const int32_t* answers, const int32_t* tokens,
                      const int32_t* n_valid, const int32_t* truth,
                      int64_t P, int32_t B, int64_t N, int mem_kind,
                      scv_cell* cells_out, int64_t* cell_tokens_out,
                      int64_t* tie_class_hits_out, int64_t* token_sum_out,
                      int64_t* truth_count_sum_out);

/*
 * Prefix budgets over ONE sample pool per problem.  The reference's budgets
 * T >= 2^11 vote over prefixes of the same samples (o1.py:274-277 with the idx-keyed cache of
 * o1.py:85-88).  pool / tokens are int32 [P, N]; cell (p, b) votes over pool[p, 0:n_valid[b]]
 * (n_valid required, any order, B <= 512).  Outputs and conventions are exactly those of
 * scv_aggregate_i32 called on the dense expansion answers[p, b, :] = pool[p, :], but the pool is
 * read from HBM once: 4 * max_b n_valid[b] algorithmic bytes per problem instead of 4 * sum_b n_valid[b].
 * Dispatch by pool length: N <= 64 (the reference's pools) one lane per problem, every budget a snapshot of one
 * pass over its votes; N <= 4096 the cell kernels, each cell reading its prefix of the problem's row; longer pools
 * the streaming kernel with a snapshot of the histogram at every boundary (option "prefix_path" forces one).
 */
int scv_aggregate_prefix_i32(scv_ctx* ctx,
                             const int32_t* pool, const int32_t* tokens,
                             const int32_t* n_valid, const int32_t* truth,
                             int64_t P, int32_t B, int64_t N, int mem_kind,
                             scv_cell* cells_out, int64_t* cell_tokens_out,
                             int64_t* tie_class_hits_out, int64_t* token_sum_out,
                             int64_t* truth_count_sum_out);

/*
 * Problem-level bootstrap (new semantics, not in the reference).  For resample
 * r in [r_begin, r_end): draw P problem indices idx_j = mulhi32(hi32(mix64(seed + G*(r*P+j+1))), P)
 * and count, per budget, hits by tie class.  counts_out int64 [r_end-r_begin, B, M]; a drawn hit
 * with n_modes >= M returns SCV_ERR_ARG (pick M = 1 + largest class present in tie_class_hits).
 * cells is scv_cell [P, B].  Pointers follow mem_kind.
 */
int scv_bootstrap(scv_ctx* ctx, const scv_cell* cells, int64_t P, int32_t B,
                  int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int mem_kind,
                  int64_t* counts_out);

/*
 * Vote + bootstrap in ONE call (DEVICE pointers; BASELINE config 5 on one GPU): scv_aggregate_i32 followed by
 * scv_bootstrap over the cell table it has just written, with the same outputs as the two calls.  When the shape
 * allows it (whole-cell streaming kernel, the [P, B] code table fits the workgroup's LDS, the persistent grid is
 * resident at once) both run in ONE kernel launch: all workgroups meet at a grid barrier after their last cell and
 * then share the resamples.  Otherwise (or with option "boot_path" >= 2) the bootstrap kernel is queued behind the
 * vote kernel on the same stream.  cells_out and counts_out are required.  Asynchronous like every DEVICE-mode call.
 * Co-tenancy cannot make a valid call fail: the one-launch form is started with hipLaunchCooperativeKernel (the
 * runtime starts it only when the whole grid is resident, whatever other streams, RCCL or other processes run; a
 * refused cooperative launch becomes two launches; option "boot_path" = 1 uses an ordinary launch, as does a
 * call made while the stream is being captured into a hipGraph).  Under an ordinary launch a workgroup gives up at the
 * barrier after "boot_spin_limit" polls; the vote outputs are complete by then, and the next scv_sync resets the
 * barrier, runs scv_bootstrap over cells_out as a separate launch and returns its status (stat "boot_recovered").
 * Until that scv_sync counts_out is undefined -- as after any asynchronous call that has not been synchronised.
 */
int scv_aggregate_bootstrap_i32(scv_ctx* ctx,
                                const int32_t* answers, const int32_t* tokens,
                                const int32_t* n_valid, const int32_t* truth,
                                int64_t P, int32_t B, int64_t N,
                                scv_cell* cells_out, int64_t* cell_tokens_out,
                                int64_t* tie_class_hits_out, int64_t* token_sum_out,
                                int64_t* truth_count_sum_out,
                                int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M,
                                int64_t* counts_out);

/*
 * Closed-form integer synthetic generator, evaluated ON DEVICE (config C3 is 335.5 GB and cannot
 * be shipped).  Element (p, b, i) depends only on (seed, dist, p_offset + p, b, i, B, N), so shards
 * and the CPU mirror (o1_inference_scaling_laws_amd/synth.py) produce identical tensors.
 *   mix64 = splitmix64 finaliser, G = 0x9E3779B97F4A7C15, mulhi32(a, n) = (a * n) >> 32
 *   k_p   = mix64((seed ^ 0x5851F42D4C957F2D) + G * (p + 1))
 *   truth = mulhi32(lo32(k_p), 1000);  q_num = 1 + hi32(k_p) % 7;  d_j = mulhi32(lo32(mix64(k_p + G*(j+1))), 1000)
 *   u     = mix64(seed + G * (((p*B + b) * N + i) + 1)),  uv = mulhi32(lo32(u), 1000)
 *   D0: uv.  D1: x = hi32(u); x < q_num*429496729 -> truth; else (x - that) < 4*214748364 -> d_[(x-that)/214748364]; else uv.
 *   D2: truth.  D3: m = 2 + (p & 1); base = ((p >> 1) & 1) ? (truth + 500) % 1000 : truth;
 *       i < (N / m) * m -> (base + 37 * (i % m)) % 1000, else (base + 999) % 1000.
 *   D4: D1 with hot = (d_0 == truth ? (truth + 500) % 1000 : d_0) in the truth's place and truth in d_0's:
 *       x < q_num*429496729 -> hot; else j = (x-that)/214748364 < 4 -> (j == 0 ? truth : d_j); else uv.
 *   D5: (truth + 500) % 1000.
 *   tokens: 100 + mulhi32(hi32(mix64(u ^ G)), 11901)                       (100..12000)
 * All pointers are DEVICE pointers (any may be NULL); async on the ctx stream.
 */
int scv_synth_fill_i32(scv_ctx* ctx, int32_t* answers, int32_t* tokens, int32_t* truth,
                       int64_t P, int32_t B, int64_t N, int64_t p_offset,
                       uint64_t seed, int dist);

/*
 * Resampled majority vote: the EXPECTED maj@k over random orderings of one sample pool per problem (new semantics, not in the
 * reference).  The reference's budgets T >= 2^11 vote over the FIRST N_b samples of one pool (o1.py:274-277 with the idx-keyed
 * cache of o1.py:85-88), so each point of its curve is one draw that depends on the order the samples sit in the cache.  Here
 * each problem's pool is shuffled R times and every budget votes over the prefixes of each ordering.
 *   pool / tokens  int32 [P, N] (tokens may be NULL); n_valid int32 [B] (required, any order, duplicates fine); truth int32 [P]
 * For problem p (global index pg = p_offset + p) and resample r in [r_begin, r_end):
 *   s      = mix64((seed ^ 0xD6E8FEB86659FD93) + G * (pg + 1))                       (uint64, wrapping; mix64, G, mulhi32 as above)
 *   perm   = [0, 1, ..., N-1];  for i in 0 .. N-2:  u = mix64(s + G * ((uint64)r * N + i + 1)),  j = i + mulhi32(hi32(u), N - i),
 *            swap(perm[i], perm[j])                                                   (partial Fisher-Yates)
 *   cell (p, r, b) = statistics.multimode over pool[p, perm[0 : k_b]],  k_b = clamp(n_valid[b], 0, N)
 * A prefix of length k depends only on the first k steps (the implementation stops at max_b k_b); each is a uniformly random
 * k-subset, and the subsets of one resample are nested across budgets, as in the reference.  Cells follow the conventions of
 * scv_aggregate_prefix_i32: an empty subset has no hit; a vote outside 0..1023 sets error bit 0 (SCV_ERR_DOMAIN at the call in HOST
 * mode, at scv_sync in DEVICE mode) or counts in bin 1023 under SCV_FLAG_CLAMP_TO_INVALID_BIN; a truth outside the bins never hits.
 * Under SCV_FLAG_OPEN_DOMAIN every int32 is a value of its own: no domain error, no clamp, and a truth of any magnitude hits when it is a mode.
 * Outputs, summed over the P x (r_end - r_begin) cells of a budget:
 *   tie_class_hits_out   int64 [B, 1025]  (required) cells with hit and n_modes == m: accuracy_from_tie_classes(tie[b], P * R)
 *                        (o1_inference_scaling_laws_amd/scoring.py) is the expected maj@k_b, exact_accuracy_... its exact rational
 *   token_sum_out        int64 [B]        (NULL ok; requires tokens) tokens of the votes in the subsets
 *   truth_count_sum_out  int64 [B]        (NULL ok) votes equal to the truth in the subsets
 *   per_resample_out     int64 [r_end - r_begin, B, M] (NULL ok) the same class counts per resample, summed over problems only
 *                        (m < M): the spread of the curve across orderings -- the reference's curve is one such draw.  A hit with
 *                        n_modes >= M sets error bit 1 (SCV_ERR_ARG at scv_sync, as in scv_bootstrap); nothing is dropped silently.
 * DEVICE mode ACCUMULATES into every output (+=) and only enqueues: no allocation, no synchronisation, legal under hipGraph capture.
 * HOST mode overwrites and blocks.  Slices of r and shards of p (p_offset) add up to the whole call bit for bit, so chunked and
 * multi-GPU use needs nothing more.  Limits: 1 <= N <= 256, 1 <= B <= 32, 0 <= r_begin <= r_end < 2^31, p_offset >= 0, M >= 1 when
 * per_resample_out is given; anything else is SCV_ERR_ARG.  One lane per (problem, resample), P * R * max_b k_b shuffle steps:
 * VALU / LDS-bound, the pool is read once (csrc/scvote_resample.hip.h).  Stat "resample_calls" counts the launches.
 */
int scv_resample_prefix_i32(scv_ctx* ctx,
                            const int32_t* pool, const int32_t* tokens,
                            const int32_t* n_valid, const int32_t* truth,
                            int64_t P, int32_t B, int64_t N, int64_t p_offset,
                            int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int mem_kind,
                            int64_t* tie_class_hits_out, int64_t* token_sum_out,
                            int64_t* truth_count_sum_out, int64_t* per_resample_out);

/*
 * Token-budget majority vote: the vote over the longest prefix of a pool ordering that fits a budget of TOKENS (new semantics, not in the
 * reference; its maj@N tail buys N = T // 2^11 samples whatever they cost, o1.py:274-277).
 *   pool / tokens  int32 [P, N] (both required; a negative token count is an error); token_budget int64 [B] (required, any order,
 *   duplicates fine); truth int32 [P]
 * For problem p (global index pg = p_offset + p), an ordering pi and budget T_b:
 *   n_b    = max { n <= N : sum_{i<n} tokens[p, pi(i)] <= T_b }   voting stops at the first sample that does not fit (later, cheaper
 *            samples are not skipped to); samples of 0 tokens always fit; a negative T_b gives an empty prefix
 *   cell (p, pi, b) = statistics.multimode over pool[p, pi(0 : n_b)], scored as everywhere (1 / n_modes on a hit; an empty prefix has
 *            no hit); its tokens sum_{i<n_b} tokens[p, pi(i)] <= T_b
 *   order  SCV_ORDER_POOL (0): pi is the identity, the cache order (one draw): r_begin = 0, r_end = 1 required
 *          SCV_ORDER_SHUFFLED (1): pi is EXACTLY the partial Fisher-Yates permutation of scv_resample_prefix_i32 for (seed, pg, r),
 *          r in [r_begin, r_end)
 * Votes and truths follow scv_resample_prefix_i32: a vote outside 0..1023 sets error bit 0 (SCV_ERR_DOMAIN at the call in HOST mode, at
 * scv_sync in DEVICE mode) or counts as 1023 under SCV_FLAG_CLAMP_TO_INVALID_BIN; a truth outside the bins never hits.  A negative token
 * count sets error bit 4: SCV_ERR_ARG at the call in HOST mode, at scv_sync in DEVICE mode.
 * Under SCV_FLAG_OPEN_DOMAIN every int32 is a value of its own (no domain error, no clamp) and cells_out[..].min_mode is the CODE of the smallest modal value.
 * Outputs, summed over the P x (r_end - r_begin) cells of a budget:
 *   tie_class_hits_out   int64 [B, 1025]  (required) cells with hit and n_modes == m (scoring.py: accuracy / exact rational)
 *   token_sum_out        int64 [B]        (NULL ok) tokens actually spent
 *   vote_count_sum_out   int64 [B]        (NULL ok) sum of n_b
 *   truth_count_sum_out  int64 [B]        (NULL ok) votes equal to the truth in the prefixes
 *   per_resample_out     int64 [r_end - r_begin, B, M] (NULL ok) class counts per ordering, summed over problems only (m < M; a hit with
 *                        n_modes >= M sets error bit 1: SCV_ERR_ARG at scv_sync)
 *   cells_out            scv_cell [P, B] (NULL ok; SCV_ORDER_POOL only) and cell_tokens_out int64 [P, B] (NULL ok; SCV_ORDER_POOL
 *                        only): the cells of the cache order, as scv_aggregate_prefix_i32 writes them; OVERWRITTEN in both modes
 * DEVICE mode ACCUMULATES into the per-budget outputs and per_resample (+=) and only enqueues: no allocation, no synchronisation, legal
 * under hipGraph capture.  HOST mode overwrites, stages chunks of problems through device memory and blocks.  Slices of r and shards of p
 * (p_offset) add up to the whole call bit for bit.  Limits: 1 <= N <= 256, 1 <= B <= 32, 0 <= r_begin <= r_end, p_offset >= 0, M >= 1
 * when per_resample_out is given; anything else -- a bad order, SCV_ORDER_POOL with r-range other than [0, 1), cell outputs with
 * SCV_ORDER_SHUFFLED -- is SCV_ERR_ARG.  One lane per (problem, ordering) walks until its largest budget is spent
 * (csrc/scvote_budget.hip.h).  Stat "token_budget_calls" counts the launches.
 */
#define SCV_ORDER_POOL 0
#define SCV_ORDER_SHUFFLED 1
int scv_token_budget_prefix_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens,
                                const int64_t* token_budget, const int32_t* truth,
                                int64_t P, int32_t B, int64_t N, int64_t p_offset, int order,
                                int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int mem_kind,
                                int64_t* tie_class_hits_out, int64_t* token_sum_out,
                                int64_t* vote_count_sum_out, int64_t* truth_count_sum_out,
                                int64_t* per_resample_out, scv_cell* cells_out, int64_t* cell_tokens_out);

/*
 * short-m@k: the majority vote over the m SHORTEST of the first k samples of a pool ordering (new semantics, not in the reference): k samples
 * are launched in parallel, the m that finish first vote, and the others are cut off when the m-th finishes.
 *   pool / tokens  int32 [P, N] (both required; a negative token count is an error); n_valid / m_keep int32 [B] (both required, any order,
 *   duplicates fine); truth int32 [P]
 * For problem p (global index pg = p_offset + p), an ordering pi and budget b:
 *   k_b = clamp(n_valid[b], 0, N), m_b = clamp(m_keep[b], 0, k_b)
 *   S   = the first k_b samples of pi
 *   V   = the m_b elements of S that come first when S is sorted ascending by the pair (tokens, pool index); the pool-index tie-break makes
 *         V a function of the SET S, not of the order inside it
 *   cell (p, pi, b) = statistics.multimode over the votes of V, scored as everywhere (1 / n_modes on a hit); m_b = 0 gives the empty cell:
 *         no hit, and 0 in every sum
 *   order  SCV_ORDER_POOL (0): pi is the identity (one draw): r_begin = 0, r_end = 1 required
 *          SCV_ORDER_SHUFFLED (1): pi is EXACTLY the partial Fisher-Yates permutation of scv_resample_prefix_i32 for (seed, pg, r),
 *          r in [r_begin, r_end)
 * Votes and truths follow scv_resample_prefix_i32: a vote outside 0..1023 sets error bit 0 (SCV_ERR_DOMAIN at the call in HOST mode, at
 * scv_sync in DEVICE mode) or counts as 1023 under SCV_FLAG_CLAMP_TO_INVALID_BIN; a truth outside the bins never hits.  A negative token
 * count sets error bit 4: SCV_ERR_ARG at the call in HOST mode, at scv_sync in DEVICE mode.
 * Under SCV_FLAG_OPEN_DOMAIN every int32 is a value of its own (no domain error, no clamp) and cells_out[..].min_mode is the CODE of the smallest modal value.
 * Outputs, summed over the P x (r_end - r_begin) cells of a budget; t_(m) is the token count of the last element of V (0 when m_b = 0):
 *   tie_class_hits_out   int64 [B, 1025]  (required) cells with hit and n_modes == m (scoring.py: accuracy / exact rational)
 *   voted_token_sum_out  int64 [B]        (NULL ok) sum over V of tokens
 *   spent_token_sum_out  int64 [B]        (NULL ok) sum over V of tokens + (k_b - m_b) * t_(m): every sample not kept is cut off when the
 *                        m-th finishes; the arithmetic is int64
 *   latency_sum_out      int64 [B]        (NULL ok) sum of t_(m)
 *   truth_count_sum_out  int64 [B]        (NULL ok) kept votes equal to the truth
 *   per_resample_out     int64 [r_end - r_begin, B, M] (NULL ok) class counts per ordering, summed over problems only (m < M; a hit with
 *                        n_modes >= M sets error bit 1: SCV_ERR_ARG at scv_sync)
 *   cells_out            scv_cell [P, B] (NULL ok; SCV_ORDER_POOL only) and cell_tokens_out int64 [P, B] (NULL ok; SCV_ORDER_POOL
 *                        only; the cell's spent tokens): OVERWRITTEN in both modes
 * Identities: with m_b >= k_b the call is scv_resample_prefix_i32 with tokens, bit for bit (tie classes, truth counts, voted = spent = its
 * token sum; the latency is the largest token count of the prefix); with k_b = N the cell does not depend on the ordering; with all tokens
 * equal V is the m_b lowest pool indices of S.
 * DEVICE mode ACCUMULATES into the per-budget outputs and per_resample (+=) and only enqueues: one launch, no allocation, no
 * synchronisation, legal under hipGraph capture.  HOST mode overwrites, stages chunks of problems through device memory and blocks.  Slices
 * of r and shards of p (p_offset) add up to the whole call bit for bit.  Limits: 1 <= N <= 256, 1 <= B <= 32, 0 <= r_begin <= r_end,
 * p_offset >= 0, M >= 1 when per_resample_out is given; anything else -- a bad order, SCV_ORDER_POOL with r-range other than [0, 1), cell
 * outputs with SCV_ORDER_SHUFFLED -- is SCV_ERR_ARG.  One lane per (problem, ordering): a shuffle step sets one bit of the lane's bitmap over
 * token ranks, a boundary walks its first m_b set bits (csrc/scvote_shortest.hip.h).
 */
int scv_shortest_prefix_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens,
                            const int32_t* n_valid, const int32_t* m_keep, const int32_t* truth,
                            int64_t P, int32_t B, int64_t N, int64_t p_offset, int order,
                            int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int mem_kind,
                            int64_t* tie_class_hits_out, int64_t* voted_token_sum_out,
                            int64_t* spent_token_sum_out, int64_t* latency_sum_out,
                            int64_t* truth_count_sum_out, int64_t* per_resample_out,
                            scv_cell* cells_out, int64_t* cell_tokens_out);

/*
 * Weighted majority vote and best-of-N over the prefixes of a pool ordering (new semantics, not in the reference, whose every rule counts a
 * sample once: statistics.multimode, o1.py:202-213).  Each sample votes with an integer weight -- a verifier or reward-model score, a
 * confidence, quantised by the caller (o1_inference_scaling_laws_amd/weighted.py: quantize_weights).
 *   pool int32 [P, N]; weights int32 [P, N] (required), each in 0 .. SCV_WEIGHT_MAX = 2^24 - 1; tokens int32 [P, N] (NULL ok);
 *   n_valid int32 [B] (required, any order, duplicates fine); truth int32 [P]
 * For problem p (global index pg = p_offset + p), an ordering pi and budget k_b = clamp(n_valid[b], 0, N), over the samples pi(0 : k_b):
 *   W(v)   = the SUM of the weights of the samples whose vote is v          rule SCV_RULE_WEIGHT_SUM (0): weighted majority vote
 *          = the MAXIMUM of those weights                                    rule SCV_RULE_BEST_OF (1): the answer of the best-scored sample
 *   modes  = the values with W(v) == max_v W(v) > 0.  A value of weight 0 is never a mode; an empty prefix, or one whose weights are all 0,
 *            has no mode and no hit (max_count 0, n_modes 0, min_mode -1), like the empty cell everywhere else
 *   score  = 1 / n_modes if the truth is a mode, else 0 (as everywhere: tie_class_hits, per_resample and scoring.py are used unchanged).
 *            Under rule 1 a tie for the top weight between samples of different votes is a tie between those votes
 *   order  SCV_ORDER_POOL (0): pi is the identity, the cache order (one draw): r_begin = 0, r_end = 1 required
 *          SCV_ORDER_SHUFFLED (1): pi is EXACTLY the partial Fisher-Yates permutation of scv_resample_prefix_i32 for (seed, pg, r),
 *          r in [r_begin, r_end)
 * With every weight 1 and rule 0 the call is the plain vote of scv_resample_prefix_i32 / scv_aggregate_prefix_i32.  With N <= 256 every W
 * is below 2^32: all sums are exact.  A weight outside 0 .. SCV_WEIGHT_MAX sets error bit 5: SCV_ERR_ARG at the call in HOST mode, at
 * scv_sync in DEVICE mode.  Votes and truths follow scv_resample_prefix_i32: a vote outside 0..1023 sets error bit 0 (SCV_ERR_DOMAIN) or
 * counts as 1023 under SCV_FLAG_CLAMP_TO_INVALID_BIN; a truth outside the bins never hits.
 * Under SCV_FLAG_OPEN_DOMAIN every int32 is a value of its own (no domain error, no clamp) and cells_out[..].min_mode is the CODE of the smallest modal value.
 * Outputs, summed over the P x (r_end - r_begin) cells of a budget:
 *   tie_class_hits_out   int64 [B, 1025]  (required) cells with hit and n_modes == m (scoring.py: accuracy / exact rational)
 *   token_sum_out        int64 [B]        (NULL ok; requires tokens) tokens of the samples in the prefixes
 *   per_resample_out     int64 [r_end - r_begin, B, M] (NULL ok) class counts per ordering, summed over problems only (m < M; a hit with
 *                        n_modes >= M sets error bit 1: SCV_ERR_ARG at scv_sync)
 *   cells_out            scv_cell [P, B] (NULL ok; SCV_ORDER_POOL only): the cells of the cache order.  Here max_count and truth_count
 *                        carry WEIGHTS: max_count = the top W, truth_count = W(truth); n_modes, min_mode and hit as always
 *   cell_tokens_out      int64 [P, B] (NULL ok; SCV_ORDER_POOL only; requires tokens).  Both cell outputs are OVERWRITTEN in both modes
 * DEVICE mode ACCUMULATES into the per-budget outputs and per_resample (+=) and only enqueues: no allocation, no synchronisation, legal
 * under hipGraph capture.  HOST mode overwrites, stages chunks of problems through device memory and blocks.  Slices of r and shards of p
 * (p_offset) add up to the whole call bit for bit.  Limits: 1 <= N <= 256, 1 <= B <= 32, 0 <= r_begin <= r_end, p_offset >= 0, M >= 1
 * when per_resample_out is given; anything else -- a bad rule or order, NULL weights, SCV_ORDER_POOL with an r-range other than [0, 1), cell
 * outputs with SCV_ORDER_SHUFFLED -- is SCV_ERR_ARG.  One lane per (problem, ordering), one launch per DEVICE call
 * (csrc/scvote_weighted.hip.h).
 */
#define SCV_RULE_WEIGHT_SUM 0
#define SCV_RULE_BEST_OF 1
#define SCV_WEIGHT_MAX 16777215   /* 2^24 - 1 */
int scv_weighted_prefix_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* weights, const int32_t* tokens,
                            const int32_t* n_valid, const int32_t* truth,
                            int64_t P, int32_t B, int64_t N, int64_t p_offset, int rule, int order,
                            int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int mem_kind,
                            int64_t* tie_class_hits_out, int64_t* token_sum_out, int64_t* per_resample_out,
                            scv_cell* cells_out, int64_t* cell_tokens_out);

/*
 * Adaptive (early-stopping) majority vote: sample until the vote is settled, then stop (new semantics, not in the reference, which fixes
 * the number of samples in advance; Adaptive-Consistency and early-stopping self-consistency are such policies).  One call scores B stopping
 * rules on the prefixes of each pool ordering and returns, per rule, the accuracy counters and what the rule spent.
 *   pool int32 [P, N]; tokens int32 [P, N] (NULL ok; they decide nothing, so a negative count is not an error); truth int32 [P]
 *   cap int32 [B] (required): n_max_b = clamp(cap[b], 0, N), the most samples rule b may draw
 *   need int32 [B, N + 1] (required): the stopping table, each value clamped to 0 .. N + 1 on the device
 *   rule_flags int32 [B] (NULL: all 0): bit 0 SCV_STOP_DECIDED; any other bit is SCV_ERR_ARG (at the call in HOST mode; error bit 6,
 *   at scv_sync, in DEVICE mode)
 * For problem p (global index pg = p_offset + p), an ordering pi and rule b the samples pool[p, pi(0)], pool[p, pi(1)], ... are counted one
 * at a time.  After the n-th sample, 1 <= n <= n_max_b:
 *   c1 = the largest count of any value
 *   c2 = the count of the second value in descending order of count: c1 when two or more values tie for the top, 0 when only one distinct
 *        value has been seen
 * and the vote stops at the first n for which one of these holds:
 *   (a) c1 >= need[b][c2]
 *   (b) SCV_STOP_DECIDED is set and c1 - c2 > n_max_b - n: the unique mode can no longer be caught or tied before the cap
 *   (c) n == n_max_b
 * n_max_b == 0 gives the empty cell: no hit, 0 votes, 0 tokens (it stopped after 0 samples).
 *   cell (p, pi, b) = statistics.multimode over the n samples counted, scored as everywhere (1 / n_modes on a hit)
 *   order  SCV_ORDER_POOL (0): pi is the identity, the cache order (one draw): r_begin = 0, r_end = 1 required
 *          SCV_ORDER_SHUFFLED (1): pi is EXACTLY the partial Fisher-Yates permutation of scv_resample_prefix_i32 for (seed, pg, r),
 *          r in [r_begin, r_end)
 * need[b][c2] = N + 1 never stops by (a) (with flag 0 the rule is the fixed vote over n_max_b samples); need[b][c2] = c2 + m stops at a lead
 * of m; o1_inference_scaling_laws_amd/adaptive.py builds these and the Beta criterion of Adaptive-Consistency.  Votes and truths follow
 * scv_resample_prefix_i32: a vote outside 0..1023 sets error bit 0 (SCV_ERR_DOMAIN at the call in HOST mode, at scv_sync in DEVICE mode) or
 * counts as 1023 under SCV_FLAG_CLAMP_TO_INVALID_BIN; a truth outside the bins never hits.
 * Under SCV_FLAG_OPEN_DOMAIN every int32 is a value of its own (no domain error, no clamp) and cells_out[..].min_mode is the CODE of the smallest modal value.
 * Outputs, summed over the P x (r_end - r_begin) cells of a rule:
 *   tie_class_hits_out   int64 [B, 1025]  (required) cells with hit and n_modes == m (scoring.py: accuracy / exact rational)
 *   token_sum_out        int64 [B]        (NULL ok; requires tokens) tokens of the samples drawn
 *   vote_count_sum_out   int64 [B]        (NULL ok) the samples drawn
 *   truth_count_sum_out  int64 [B]        (NULL ok) votes equal to the truth among them
 *   stop_hist_out        int64 [B, N + 1] (NULL ok) cells that stopped after exactly n samples: the cost distribution of the rule
 *   per_resample_out     int64 [r_end - r_begin, B, M] (NULL ok) class counts per ordering, summed over problems only (m < M; a hit with
 *                        n_modes >= M sets error bit 1: SCV_ERR_ARG at scv_sync)
 *   cells_out            scv_cell [P, B], cell_tokens_out int64 [P, B] (requires tokens), cell_votes_out int32 [P, B] (each NULL ok;
 *                        SCV_ORDER_POOL only): the cells of the cache order, their tokens and the samples they drew; OVERWRITTEN in both modes
 * DEVICE mode ACCUMULATES into every other output (+=) and only enqueues: no allocation, no synchronisation, legal under hipGraph capture.
 * HOST mode overwrites, stages chunks of problems through device memory and blocks.  Slices of r and shards of p (p_offset) add up to the
 * whole call bit for bit.  Limits: 1 <= N <= 256, 1 <= B <= 32, 0 <= r_begin <= r_end, p_offset >= 0, M >= 1 when per_resample_out is
 * given; anything else -- a bad order, NULL cap or need, SCV_ORDER_POOL with an r-range other than [0, 1), cell outputs with
 * SCV_ORDER_SHUFFLED, token outputs without tokens -- is SCV_ERR_ARG.  One lane per (problem, ordering) walks until its last rule has
 * stopped, one launch per DEVICE call (csrc/scvote_adaptive.hip.h).
 */
#define SCV_STOP_DECIDED 0x1
int scv_adaptive_prefix_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens,
                            const int32_t* cap, const int32_t* need, const int32_t* rule_flags, const int32_t* truth,
                            int64_t P, int32_t B, int64_t N, int64_t p_offset, int order,
                            int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int mem_kind,
                            int64_t* tie_class_hits_out, int64_t* token_sum_out,
                            int64_t* vote_count_sum_out, int64_t* truth_count_sum_out, int64_t* stop_hist_out,
                            int64_t* per_resample_out, scv_cell* cells_out, int64_t* cell_tokens_out, int32_t* cell_votes_out);

/*
 * Majority vote over draws WITH replacement, past the size of the pool: the plug-in (bootstrap) estimate of maj@k (new semantics, not in
 * the reference, whose curve ends at its largest pool, 128 samples, o1.py:266-276).  A problem's pool is taken for the model's answer
 * distribution; k answers are drawn from it with replacement and voted on.  This is defined for any k and smooth in k; its limit as k grows
 * is the score of the vote over the whole pool (scv_aggregate_prefix_i32 at k = N).
 *   pool / tokens  int32 [P, N] (tokens may be NULL); truth int32 [P]; n_draws int32 [B] (required, any order, duplicates fine)
 * The budget is k_b = max(n_draws[b], 0).  It is NOT clamped to N.  The limit is k_b <= SCV_IID_MAX_DRAWS = 65535, so a count fits 16 bits.
 * For problem p (global index pg = p_offset + p) and resample r in [r_begin, r_end):
 *   s      = mix64((seed ^ 0xA0761D6478BD642F) + G * (pg + 1))                       (uint64, wrapping; mix64, G, mulhi32 as above)
 *            The salt differs from scv_resample_prefix_i32's, so this call's draws are independent of that call's for the same seed.
 *   draw i = 0, 1, ...:  u = mix64(s + G * ((uint64)r * 65536 + i + 1)),  x_i = pool[p, mulhi32(hi32(u), N)]
 *            The stride per resample is 65536 > SCV_IID_MAX_DRAWS, so the streams of different r never overlap.
 *   cell (p, r, b) = statistics.multimode(x_0 ... x_{k_b - 1}), scored as everywhere else (1 / n_modes on a hit); k = 0 is the empty cell
 *            (no hit).  The budgets of one resample are nested prefixes of one draw sequence.
 * Votes, truths and the clamp flag follow scv_resample_prefix_i32: a vote outside 0..1023 sets error bit 0 (SCV_ERR_DOMAIN at the call in
 * HOST mode, at scv_sync in DEVICE mode) or counts in bin 1023 under SCV_FLAG_CLAMP_TO_INVALID_BIN; a truth outside the bins never hits.
 * Under SCV_FLAG_OPEN_DOMAIN every int32 is a value of its own: no domain error, no clamp, and a truth of any magnitude hits when it is a mode.
 * Outputs and their accumulation rules are those of scv_resample_prefix_i32, summed over the P x (r_end - r_begin) cells of a budget:
 *   tie_class_hits_out   int64 [B, 1025]  (required) cells with hit and n_modes == m (scoring.py: accuracy / exact rational);
 *                        n_modes <= min(distinct values, k) <= N, so the table keeps its shape for k > N
 *   token_sum_out        int64 [B]        (NULL ok; requires tokens) tokens of the draws (a sample drawn twice is paid twice)
 *   truth_count_sum_out  int64 [B]        (NULL ok) draws equal to the truth
 *   per_resample_out     int64 [r_end - r_begin, B, M] (NULL ok) class counts per resample, summed over problems only (m < M; a hit with
 *                        n_modes >= M sets error bit 1: SCV_ERR_ARG at scv_sync)
 * DEVICE mode ACCUMULATES into every output (+=) and only enqueues: no allocation, no synchronisation, legal under hipGraph capture.
 * HOST mode overwrites, stages chunks of problems through device memory and blocks.  Slices of r and shards of p (p_offset) add up to the
 * whole call bit for bit.  Limits: 1 <= N <= 256, 1 <= B <= 32, 0 <= r_begin <= r_end < 2^31, p_offset >= 0, M >= 1 when per_resample_out
 * is given, token_sum_out only with tokens; anything else is SCV_ERR_ARG.  A budget k_b > SCV_IID_MAX_DRAWS is SCV_ERR_ARG at the call in
 * HOST mode; in DEVICE mode the kernel raises error bit 7 and computes nothing for that call (SCV_ERR_ARG at scv_sync, outputs untouched).
 * One lane per (problem, resample), P * R * max_b k_b steps of one draw, one 16-bit count in LDS and one running-mode update
 * (csrc/scvote_iid.hip.h); the pool is read once.
 */
#define SCV_IID_MAX_DRAWS 65535
int scv_iid_prefix_i32(scv_ctx* ctx,
                       const int32_t* pool, const int32_t* tokens,
                       const int32_t* n_draws, const int32_t* truth,
                       int64_t P, int32_t B, int64_t N, int64_t p_offset,
                       int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int mem_kind,
                       int64_t* tie_class_hits_out, int64_t* token_sum_out,
                       int64_t* truth_count_sum_out, int64_t* per_resample_out);

/*
 * Resampled majority vote over WIDE pools: the expected maj@k over random orderings of one pool of up to SCV_WIDE_MAX_N = 4096 samples per
 * problem (new semantics, not in the reference).  scv_resample_prefix_i32 keeps one lane per (problem, ordering) and stops at N = 256; beyond
 * that only the pool-order curve of scv_aggregate_prefix_i32 was left, which is one draw.  Arguments, outputs and modes are exactly those of
 * scv_resample_prefix_i32; the ORDERING is not: a Fisher-Yates walk is sequential, so the order is defined by sort keys.
 *   pool / tokens  int32 [P, N] (tokens may be NULL); n_valid int32 [B] (required, any order, duplicates fine); truth int32 [P]
 * For problem p (global index pg = p_offset + p) and resample r in [r_begin, r_end):
 *   s     = mix64((seed ^ 0x8EBC6AF09C88C6E3) + G * (pg + 1))                       (uint64, wrapping; mix64, G as above)
 *   u_i   = mix64(s + G * ((uint64)r * 4096 + i + 1))                               i = 0 .. N-1
 *   w_i   = (u_i & ~4095) | i                                                       52 random bits, the pool index below them
 *   order = the samples sorted ascending by w_i                                     (the w_i are distinct: every sort gives the same order)
 *   cell (p, r, b) = statistics.multimode over pool[p, order[0 : k_b]],  k_b = clamp(n_valid[b], 0, N)
 * The stride of 4096 per resample keeps the streams of different r apart, and the salt differs from every other entry's, so this call's
 * orderings are independent of theirs for the same seed.  The prefixes of one resample are nested across budgets.  Each prefix is a uniformly
 * random k-subset EXCEPT when two of the 52-bit keys of an ordering tie (the pool index then decides): the probability of any tie in one
 * ordering is below N^2 / 2^53 (< 2^-29 at N = 4096), far under the resolution of any R a call can draw.
 * NOT bit-compatible with scv_resample_prefix_i32 at N <= 256: the orderings differ, only the expectation is the same (at k_b = N every
 * output is the same: the ordering cannot matter there).  At N <= 256 scv_resample_prefix_i32 is the entry to call: one lane per ordering
 * beats one workgroup per ordering there (csrc/scvote_wide.hip.h).
 * Votes, truths, the empty prefix, error bit 0 / SCV_ERR_DOMAIN, SCV_FLAG_CLAMP_TO_INVALID_BIN and error bit 1 for a hit with n_modes >= M
 * are as in scv_resample_prefix_i32.
 * Under SCV_FLAG_OPEN_DOMAIN every int32 is a value of its own, exactly as the flag is defined for the other pool-ordering entries: a vote's
 * code is the rank of its value among the D distinct values of the whole row pool[p, 0:N] in ascending signed order, 1 <= D <= N -- there is
 * no limit of 1024 --, the truth hits when it equals a modal value, whatever its magnitude, and a truth absent from the row never hits.  No
 * domain error (never error bit 0) and SCV_FLAG_CLAMP_TO_INVALID_BIN has no effect.  Orderings, key streams, the salt, token sums, slices of
 * r, shards of p, the HOST / DEVICE rules, graph capture, the argument list and the limits are unchanged, and a flag-on call on a pool inside
 * 0..1023 gives the same bits in every output as the flag-off call (the relabelling preserves equality).  tie_class_hits_out stays [B, 1025]:
 * with D > 1024 a hit can have n_modes >= 1025, which has no column -- such a hit is counted in NEITHER table and sets error bit 1 (the rule
 * for n_modes >= M, applied to the main table): SCV_ERR_ARG at the call in HOST mode, at scv_sync in DEVICE mode, nothing dropped silently;
 * truth_count_sum_out and token_sum_out of that cell are still added.  A budget of at most 1024 samples can never reach it.
 * Outputs, summed over the P x (r_end - r_begin) cells of a budget, as in scv_resample_prefix_i32:
 *   tie_class_hits_out int64 [B, 1025] (required), token_sum_out int64 [B] (NULL ok; requires tokens), truth_count_sum_out int64 [B] (NULL ok),
 *   per_resample_out int64 [r_end - r_begin, B, M] (NULL ok; a hit with n_modes >= M sets error bit 1)
 * DEVICE mode ACCUMULATES into every output (+=) and only enqueues: one launch, no allocation, no synchronisation, legal under hipGraph
 * capture.  HOST mode overwrites, stages chunks of problems through device memory and blocks.  Slices of r and shards of p (p_offset) add
 * up to the whole call bit for bit.  Limits: 1 <= N <= SCV_WIDE_MAX_N, 1 <= B <= 32, 0 <= r_begin <= r_end < 2^31, p_offset >= 0, M >= 1
 * when per_resample_out is given, token_sum_out only with tokens; anything else is SCV_ERR_ARG with nothing queued.  One workgroup per
 * (problem, resample): a bitonic sort of the padded words in LDS, then one 1024-bin histogram walked budget by budget (open domain: one
 * more sort per problem of a workgroup's run encodes the row, and the histogram has the row's D bins).
 */
#define SCV_WIDE_MAX_N 4096
int scv_resample_wide_i32(scv_ctx* ctx,
                          const int32_t* pool, const int32_t* tokens,
                          const int32_t* n_valid, const int32_t* truth,
                          int64_t P, int32_t B, int64_t N, int64_t p_offset,
                          int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int mem_kind,
                          int64_t* tie_class_hits_out, int64_t* token_sum_out,
                          int64_t* truth_count_sum_out, int64_t* per_resample_out);

/*
 * Token-budget majority vote over WIDE pools: the vote over the longest prefix of an ordering of one pool of up to SCV_WIDE_MAX_N = 4096
 * samples per problem that fits a budget of TOKENS (new semantics, not in the reference).  scv_token_budget_prefix_i32 stops at N = 256 and
 * scv_resample_wide_i32 buys k samples whatever they cost; this entry has the argument list of the first and the orderings of the second.
 *   pool / tokens  int32 [P, N] (both required; a negative token count is an error); token_budget int64 [B] (required, any order,
 *   duplicates fine); truth int32 [P]
 * For problem p (global index pg = p_offset + p), an ordering pi and budget T_b:
 *   n_b    = max { n <= N : sum_{i<n} tokens[p, pi(i)] <= T_b }   voting stops at the first sample that does not fit (later, cheaper
 *            samples are not skipped to); samples of 0 tokens always fit; a negative T_b gives the empty prefix; T_b is any int64 and every
 *            comparison is 64-bit (a running sum of a row is below 4096 * 2^31 = 2^43)
 *   cell (p, pi, b) = statistics.multimode over pool[p, pi(0 : n_b)], scored as everywhere (1 / n_modes on a hit); its tokens are
 *            sum_{i<n_b} tokens[p, pi(i)] <= T_b; an empty prefix has no hit and adds 0 to every output
 *   order  SCV_ORDER_POOL (0): pi is the identity, the cache order (one draw): r_begin = 0, r_end = 1 required
 *          SCV_ORDER_SHUFFLED (1): pi is EXACTLY the ordering of scv_resample_wide_i32 for (seed, pg, r), r in [r_begin, r_end): the same
 *          salt, the same stride of 4096 per resample, the same sort words w_i -- NOT the Fisher-Yates orderings of
 *          scv_token_budget_prefix_i32, with which only the expectation is shared.  In SCV_ORDER_POOL the two entries agree in every output
 *          at N <= 256.
 * Votes, truths, error bit 0 / SCV_ERR_DOMAIN, SCV_FLAG_CLAMP_TO_INVALID_BIN and SCV_FLAG_OPEN_DOMAIN are as in scv_resample_wide_i32.  Under
 * SCV_FLAG_OPEN_DOMAIN D is the number of distinct values of the problem's row; with D > 1024 a hit can tie in 1025 or more ways, and such a
 * hit has no column: it sets error bit 1 and is counted in NEITHER table (its token, vote and truth-count sums are still added).
 * A negative token count sets error bit 4: SCV_ERR_ARG at the call in HOST mode, at scv_sync in DEVICE mode.  The kernel adds such a count as 0
 * after raising the bit, so the running sum stays monotone and no walk leaves the row; the outputs of such a call are otherwise not specified.
 * Outputs, summed over the P x (r_end - r_begin) cells of a budget:
 *   tie_class_hits_out   int64 [B, 1025]  (required) cells with hit and n_modes == m
 *   token_sum_out        int64 [B]        (NULL ok) tokens actually spent
 *   vote_count_sum_out   int64 [B]        (NULL ok) sum of n_b
 *   truth_count_sum_out  int64 [B]        (NULL ok) votes equal to the truth in the prefixes
 *   per_resample_out     int64 [r_end - r_begin, B, M] (NULL ok) class counts per ordering, summed over problems only (m < M; a hit with
 *                        n_modes >= M sets error bit 1)
 *   cells_out            scv_cell [P, B] (NULL ok; SCV_ORDER_POOL only) and cell_tokens_out int64 [P, B] (NULL ok; SCV_ORDER_POOL only): the
 *                        cells of the cache order; OVERWRITTEN in both modes.  min_mode is the smallest modal value (clamped into the bins);
 *                        under SCV_FLAG_OPEN_DOMAIN it is the CODE of that value (a code of up to 4095 fits the int16; engine.decode_min_mode
 *                        turns it back); -1 in an empty cell.
 * DEVICE mode ACCUMULATES into the per-budget outputs and per_resample_out (+=) and only enqueues: ONE launch, no allocation, no
 * synchronisation, legal under hipGraph capture.  HOST mode overwrites, stages chunks of problems through device memory (the path the lane
 * entries share) and blocks.  Slices of r and shards of p (p_offset) add up to the whole call bit for bit.
 * Limits: 1 <= N <= SCV_WIDE_MAX_N, 1 <= B <= 32, 0 <= r_begin <= r_end < 2^31, p_offset >= 0, M >= 1 when per_resample_out is given.
 * SCV_ERR_ARG with nothing queued: a NULL tokens (with P > 0), token_budget or tie_class_hits_out; a bad order; SCV_ORDER_POOL with an r-range
 * other than [0, 1); cell outputs with SCV_ORDER_SHUFFLED; a limit broken.  One workgroup per (problem, ordering): the sort of
 * scv_resample_wide_i32, then a workgroup-wide int64 scan writes the running token sum over the dead random bits of every sorted word, n_b
 * is a binary search per budget, and the sorted budgets are walked over one histogram (csrc/scvote_wide_budget.hip.h).
 */
int scv_token_budget_wide_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* tokens,
                              const int64_t* token_budget, const int32_t* truth,
                              int64_t P, int32_t B, int64_t N, int64_t p_offset, int order,
                              int32_t r_begin, int32_t r_end, uint64_t seed, int32_t M, int mem_kind,
                              int64_t* tie_class_hits_out, int64_t* token_sum_out,
                              int64_t* vote_count_sum_out, int64_t* truth_count_sum_out,
                              int64_t* per_resample_out, scv_cell* cells_out, int64_t* cell_tokens_out);

/*
 * Exact expected majority vote: maj@k over ALL k-subsets of one pool per problem (new semantics, not in the reference) -- the
 * R -> infinity limit of scv_resample_prefix_i32 (the prefix of a uniformly random ordering is a uniformly random k-subset), with no
 * seed and nothing left to converge.
 *   pool int32 [P, N]; n_valid int32 [B] (required, any order, duplicates fine); truth int32 [P]
 * Per problem p with budgets k_b = clamp(n_valid[b], 0, N), c_v the votes of value v in pool[p, 0:N] and c_t those of the truth (0 when
 * absent):
 *   E_k = C(N,k)^-1 sum_{j=1..min(c_t,k)} C(c_t,j) sum_u A_j(k-j,u) / (1+u)    the expected score (o1.py:202-213: 1 / n_modes on a hit)
 *   H_k = C(N,k)^-1 sum_{j=1..min(c_t,k)} C(c_t,j) sum_u A_j(k-j,u)            the probability that the truth is among the modes
 *   A_j(s,u) = [x^s y^u] prod_{v != t} ( sum_{i=0..min(c_v, j-1)} C(c_v,i) x^i + [c_v >= j] C(c_v,j) x^j y )
 * (j truth votes in the subset; every other value at most j votes, u of them tied at exactly j).  Cells follow scv_resample_prefix_i32:
 * a vote outside 0..1023 counts as value 1023 and sets error bit 0 (SCV_ERR_DOMAIN at the call in HOST mode, at scv_sync in DEVICE mode;
 * no error under SCV_FLAG_CLAMP_TO_INVALID_BIN); a truth outside the bins never hits; k = 0 scores 0.
 * Under SCV_FLAG_OPEN_DOMAIN every int32 is a value of its own: no domain error, no clamp, and a truth of any magnitude counts as c_t when it is in the row.
 *   expected_score_out  float64 [P, B] (required)  E_k_b;  mean over p is the expected maj@k_b (curves.exact_majority_records)
 *   hit_prob_out        float64 [P, B] (NULL ok)   H_k_b
 * Computed in float64 with no subtraction anywhere (sum_u A / (1+u) = integral_0^1 A(s,y) dy by an exact Gauss-Legendre rule;
 * csrc/scvote_expected.hip.h): every output is within 1e-12 relative of the exact rational, and exactly 0.0 when that is 0.  Each (p, b)
 * is summed in one fixed order: repeated calls, HOST and DEVICE mode, and shards of p (pool + p0 * N, truth + p0, out + p0 * B) give the
 * same bits.  Outputs are OVERWRITTEN in both modes.  DEVICE mode only enqueues: no allocation, no synchronisation, legal under hipGraph
 * capture.  HOST mode stages chunks of problems through device memory and blocks.  Limits: 1 <= N <= 256, 1 <= B <= 32, P >= 0 (P = 0 does
 * nothing); anything else is SCV_ERR_ARG.  One workgroup per problem; the cost grows with the classes that can tie, not with a sample count.
 * Stat "expected_calls" counts the launches.
 */
int scv_expected_majority_i32(scv_ctx* ctx, const int32_t* pool, const int32_t* n_valid, const int32_t* truth,
                              int64_t P, int32_t B, int64_t N, int mem_kind,
                              double* expected_score_out, double* hit_prob_out);

/*
 * The device error word (bit 0: a vote outside bins 0..1023 -- exported as 0 under SCV_FLAG_CLAMP_TO_INVALID_BIN, where
 * scv_sync does not treat it as an error either; bit 1: a drawn bootstrap hit, or a resampled hit with per_resample_out, had n_modes >= M; bit 4: a negative token count in scv_token_budget_prefix_i32, scv_token_budget_wide_i32 or scv_shortest_prefix_i32; bit 5: a weight outside 0 .. SCV_WEIGHT_MAX in scv_weighted_prefix_i32; bit 6: an unknown rule flag in scv_adaptive_prefix_i32; bit 7: a draw budget above SCV_IID_MAX_DRAWS in a DEVICE-mode scv_iid_prefix_i32, which then computed nothing; bit 2: the one-launch vote +
 * bootstrap of a NON-cooperative launch gave up at its grid barrier -- not an error: the next scv_sync repairs it), widened to
 * int64 and written to *dst_device IN STREAM ORDER behind everything queued so far; it is not cleared (scv_sync does
 * that).  For multi-GPU callers: the reference sums scores over problems in one process (o1.py:236-245); when the
 * problems are sharded over ranks, the word goes into one extra element behind the packed counters so that the ONE
 * all-reduce of the evaluation also tells every rank whether any rank's counters are invalid -- no host round trip,
 * no rank left waiting in a collective (o1_inference_scaling_laws_amd/passk.py, dist.py).
 */
int scv_export_error_word(scv_ctx* ctx, int64_t* dst_device);

/*
 * Several GPUs from ONE process (the reference is one process, o1.py:312-315): a communicator owns one scv_ctx per device and
 * the exchange step of the path -- the sum over problems of o1.py:236-245, which becomes ONE all-reduce of the packed int64
 * per-budget counters when the problems are sharded by contiguous block over the devices.  No launcher, no
 * torch.distributed: a ctypes / C caller shards its problems, calls scv_aggregate_i32 (DEVICE mode) on every rank's ctx, then
 * scv_allreduce_counters, then scv_comm_sync.
 *
 *   devices      HIP device index of every rank (NULL or n == 0: all visible devices, rank r = device r); an index may
 *                repeat (several contexts on one GPU: how a 1-GPU box exercises the path); at most 16 ranks
 *   ctx_flags    SCV_FLAG_* for every rank's context
 *   comm_flags   SCV_COMM_PEER (default): one-shot all-reduce over xGMI peer access, pure HIP -- every rank's kernel reads the
 *                other ranks' buffers directly, sums them into a staging buffer, and the sums replace the buffers when every
 *                rank has finished reading; the devices' streams are ordered by events, the host never blocks.
 *                SCV_COMM_RCCL: ncclCommInitAll + grouped ncclAllReduce(ncclInt64, ncclSum); librccl is resolved at run time
 *                (the copy the process already holds, else /opt/rocm's); distinct devices only.
 *
 * scv_comm_create with more than one rank -- or with SCV_COMM_RCCL and any rank count -- ends with a SELF-TEST (first contact with
 * the devices is loud, not a wrong accuracy later): two rounds of known int64 patterns -- (PEER) every rank reads every other rank's
 * buffer directly, ordered by the all-reduce's own cross-device events, once with nontemporal loads and once with ordinary loads,
 * then one whole scv_allreduce_counters of the production payload (8217 words) and one scv_allgather_i64, each verified on every
 * device.  The peer reads decide how this communicator reads its peers (nontemporal loads when they were right in both rounds,
 * else ordinary loads when those were; "peer_loads" says which); when neither kind was right, or a collective's result is wrong,
 * the create fails with SCV_ERR_ARG and a message ("... self-test ...") that names the device pair (peer read) or the device
 * (collective) -- the caller then creates the communicator with SCV_COMM_RCCL (the Python MultiDeviceEngine does that by
 * itself, with a warning).  The second round catches a reader that kept stale lines of a peer's first-round buffer.
 *
 * scv_allreduce_counters: buffers[r] is a DEVICE pointer on rank r's device (count int64 each, e.g. the packed counters
 * tie_class_hits | token_sum | truth_count_sum, optionally one more word from scv_export_error_word); in place, SUM, ordered
 * behind everything queued on the ranks' ctx streams, asynchronous.  Integer sums => the same bits at any device count.
 * The one-shot form stages through a buffer allocated at create (1 MiB per rank: no allocation on the launch path, legal
 * under hipGraph capture); a larger count grows it (synchronising), which is refused while a rank's stream is being captured.
 *
 * BASELINE config 5 (pass@k + bootstrap) on several GPUs without torch: the bootstrap resamples over ALL
 * problems, so after the vote every rank needs every rank's cells --
 * scv_allgather_cells: tables[r] is a DEVICE pointer on rank r's device to the WHOLE table scv_cell [sum(rows), B] in which rank r
 *   has written its own block (rows[r] problems, starting at row rows[0] + ... + rows[r - 1]: pass cells_out = that row to
 *   scv_aggregate_i32); afterwards every rank's table holds every block.  PEER: every rank pulls the other blocks over its own
 *   links (device-to-device copies ordered by the same events); RCCL: one grouped ncclBroadcast per block.
 * then every rank runs scv_bootstrap over its slice [r_begin, r_end) of the resamples, and
 * scv_allgather_i64: the same in-place all-gather for int64 blocks (counts[r] words per rank, rank r's block at word offset
 *   counts[0] + ... + counts[r - 1] of buffers[r]) -- the gather of the resample slices counts_out [r_end - r_begin, B, M].
 * Both are asynchronous and ordered behind everything queued on the ranks' ctx streams.
 * scv_comm_sync = scv_sync on every rank (first error wins).  scv_comm_get_stat: "selftest_words" (words verified per rank at
 * create; 0 with one SCV_COMM_PEER rank), "staging_bytes" (current size of the all-reduce's staging buffer), "peer_loads" (0: the
 * one-shot all-reduce reads its peers with nontemporal loads, 1: with ordinary loads, -1: no peer reads -- RCCL or one rank),
 * "selftest_nt_ok" / "selftest_plain_ok" (pairwise peer reads of the self-test with either load kind: 1 all right, 0 some wrong,
 * -1 not run).
 */
typedef struct scv_comm scv_comm;
#define SCV_COMM_PEER 0x0u
#define SCV_COMM_RCCL 0x1u
int scv_comm_create(scv_comm** out, const int* devices, int n, uint32_t ctx_flags, uint32_t comm_flags);
int scv_comm_destroy(scv_comm* comm);
int scv_comm_size(const scv_comm* comm);
scv_ctx* scv_comm_ctx(scv_comm* comm, int rank);       /* owned by the communicator: do not scv_destroy it */
int scv_allreduce_counters(scv_comm* comm, int64_t* const* buffers, int64_t count);
int scv_allgather_cells(scv_comm* comm, scv_cell* const* tables, const int64_t* rows, int32_t B);
int scv_allgather_i64(scv_comm* comm, int64_t* const* buffers, const int64_t* counts);
int scv_comm_sync(scv_comm* comm);
int scv_comm_get_stat(scv_comm* comm, const char* key, int64_t* out);

/* Duration of the most recent aggregation kernel launch on this ctx, from hipEvents recorded on
 * the launch stream (needs SCV_FLAG_TIMING).  Blocks until that launch has finished. */
int scv_last_kernel_ns(scv_ctx* ctx, uint64_t* ns_out);
/* Sum and count of all timed launches since the previous call (resets the accumulators). */
int scv_drain_kernel_ns(scv_ctx* ctx, uint64_t* total_ns_out, uint64_t* launches_out);

/*
 * Pinned (page-locked) host memory for HOST-mode inputs.  The reference keeps its samples in one JSON cache
 * (o1.py:50-68); an extractor that writes the answers / tokens tensors straight into a buffer from here lets
 * SCV_MEM_HOST calls DMA them in place (the staging pipeline otherwise copies pageable memory into pinned
 * bounce slots with worker threads first).  Any hipHostMalloc / hipHostRegister'ed buffer is recognised the
 * same way; these two entry points only spare a ctypes caller a HIP binding of its own.
 */
int scv_host_alloc(void** out, size_t bytes);
int scv_host_free(void* p);

/* How often this ctx took a form (monotonic counters, for tests and bench lines): "boot_fused" / "boot_separate"
 * (scv_aggregate_bootstrap_i32: one launch / two), "boot_cooperative" (one-launch forms started as cooperative launches),
 * "boot_recovered" (grid-barrier timeouts repaired by scv_sync with a separate bootstrap launch), "overwrite_fused" (counters
 * overwritten by the vote kernel's last workgroup), "lds_counters" (register-resident launches that produced their counters
 * themselves), "sort_cells" (sorted-cells launches), "few_votes" (launches of the kernels for cells of exactly 1, 2 or 4 votes), "one_vote" (those of them served by scv_one_vote / scv_two_votes: N = 1, 2), "prefix_cells" / "prefix_lane" / "prefix_pool" (prefix calls served by the cell kernels / by
 * the one-lane-per-problem kernel / by the one-pass-per-problem kernel), "prefix_sort" (launches of scv_sort_prefix: every power-of-two budget out of one
 * sort per problem -- queued, that is: a DEVICE-mode launch may find budgets it does not serve and leave them to the kernel behind it), "prefix_tokens" (launches of
 * scv_sort_prefix2<true>: the token sums of pools of 68 .. 128 votes out of token steps of the sort kernel's launch), "host_small_calls" / "host_pipelined_calls" (HOST-mode calls served by the one-block small path / by
 * the staging pipeline), "host_thread_start_failures" (worker threads of the staging pipeline the system refused to start: the
 * pipeline runs with the threads it has, the calling thread at least), "resample_calls" (launches of scv_resample_prefix_i32), "expected_calls" (launches of scv_expected_majority_i32), "token_budget_calls" (launches of
 * scv_token_budget_prefix_i32). */
int scv_get_stat(scv_ctx* ctx, const char* key, int64_t* out);

int scv_device_count(void);
/* Static properties of the ctx device: [0]=CU count, [1]=LDS bytes per workgroup max, [2]=clock kHz, [3]=HBM bytes. */
int scv_device_info(scv_ctx* ctx, int64_t info_out[4]);
const char* scv_last_error(void);   /* thread-local, never NULL */
const char* scv_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SCVOTE_H */
