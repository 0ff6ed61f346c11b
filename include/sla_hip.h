/*
 * sla_hip.h -- batched C-ABI of the MI355X (gfx950) SLA encode hot path.
 *
 * Plain C: pointers, sizes, an opaque stream handle.  No torch / C++ types.
 * Two layers:
 *
 *  (1) kernel launchers  sla_hip_launch_*  -- one call = one HIP kernel over a
 *      batch of descriptors that already live in device memory.  These are
 *      what replaces the reference's per-block inner functions:
 *        prepass  : SLAEncoder_CalculateLeftShiftOffset  src/SLAEncoder.c:425-455
 *                   + silence test                       src/SLAEncoder.c:392-408, 520-528
 *        lpc      : LPC_CalculateAutoCorrelation         src/SLAPredictor.c:331-388
 *                   LPC_LevinsonDurbinRecursion          src/SLAPredictor.c:253-328
 *                   (A0 staging: src/SLAEncoder.c:505-515, 540-543; src/SLAUtility.c:370-412)
 *                   Sum x^2 of SLALPCCalculator_EstimateCodeLength src/SLAPredictor.c:432-436
 *                   coefficient quantiser                src/SLAEncoder.c:567-589
 *        lattice  : SLAEmphasisFilter_PreEmphasisInt32   src/SLAPredictor.c:1741-1765
 *                   SLALPCSynthesizer_PredictByParcorCoefInt32 src/SLAPredictor.c:557-607
 *        ltm_acf  : FFT autocorrelation of SLALongTermCalculator_CalculateCoef src/SLAPredictor.c:827-853
 *        tail     : SLALongTermSynthesizer_PredictInt32  src/SLAPredictor.c:1031-1119
 *                   SLALMSFilter_PredictInt32            src/SLAPredictor.c:1202-1331
 *                   SLACoder_CalculateInitialRecursiveRiceParameter src/SLACoder.c:361-385
 *
 *  (2) the whole-file driver behind SLAEncoder_EncodeWhole (SLAEncoder.h),
 *      also callable on PCM that is already resident in HBM
 *      (sla_hip_analyze_device) -- this is what bench.py times.
 *
 * All functions return 0 on success, a negative hipError_t-derived code on a
 * HIP failure, or a positive SLAApiResult for API-level errors.
 */
#ifndef SLA_HIP_H_INCLUDED
#define SLA_HIP_H_INCLUDED

#include <stdint.h>
#include "SLA.h"
#include "SLAEncoder.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sla_hip_stream_t;          /* a hipStream_t, or NULL for the default stream */

/* ---- descriptors (device-resident arrays of these feed the kernels) ----- */

/* One LPC work-group: a window of one channel staged once in LDS, analysed
 * over `cand_count` sub-ranges ("candidates" of the partition search, or the
 * single whole range of a chosen block). */
typedef struct sla_hip_lpc_group {
  uint64_t pcm_off;        /* first sample of the window inside a channel plane          */
  uint32_t num_samples;    /* window length W                                              */
  uint32_t channel;        /* output channel index (after mid/side when MS is on)         */
  uint32_t win_off;        /* offset of the analysis window table in the window pool, or
                              SLA_HIP_NO_WINDOW: rectangular, no pre-emphasis (search)     */
  uint32_t int_shift;      /* right shift of the integer path: 32 - bps + offset_lshift   */
  uint32_t cand_first;     /* first entry in the candidate table                          */
  uint32_t cand_count;
  uint32_t slot_first;     /* output slot of candidate 0; candidate c writes slot_first+c */
  uint32_t pad_;
} sla_hip_lpc_group;
#define SLA_HIP_NO_WINDOW 0xFFFFFFFFu
/* LDS one LPC work-group may use: window doubles + (order+1) doubles per candidate.
 * 160 KiB per CU on gfx950, minus a small static allocation. */
#define SLA_HIP_LDS_BUDGET (160u * 1024u - 256u)

typedef struct sla_hip_lpc_cand {
  uint32_t start;          /* relative to the group's window */
  uint32_t len;
} sla_hip_lpc_cand;

/* One lattice wave: `count` output samples of one (block, channel). */
typedef struct sla_hip_lattice_chunk {
  uint64_t blk_off;        /* first sample of the block inside a channel plane */
  uint32_t blk_len;
  uint32_t chunk_start;    /* first output sample of this chunk, relative to the block */
  uint32_t count;
  uint32_t channel;
  uint32_t slot;           /* (block, channel) slot: coefficients live at kint[slot*(order+1)] */
  uint32_t int_shift;
} sla_hip_lattice_chunk;

/* One (block, channel) of the long-term analysis FFT. */
typedef struct sla_hip_acf_job {
  uint64_t blk_off;
  uint32_t blk_len;
  uint32_t channel;
} sla_hip_acf_job;

/* One (block, channel) of the serial tail (long-term filter + LMS + Rice sum). */
typedef struct sla_hip_tail_job {
  uint64_t blk_off;
  uint32_t blk_len;        /* 0 is allowed: nothing is read or written for the job but fold_sum[j] = 0 */
  uint32_t channel;
  uint32_t pitch;          /* 0 = long-term stage bypassed */
  int32_t  ltm_coef[5];    /* Q31 taps (<<16 form), longterm_order of them used */
  uint32_t pad_[2];
} sla_hip_tail_job;

/* One (block, channel) of the Rice code-length pass. */
typedef struct sla_hip_rice_job {
  uint64_t blk_off;
  uint32_t blk_len;
  uint32_t channel;
  uint32_t rice_init;      /* initial parameter (mean of the folded residual, >= 1)            */
  uint32_t golomb_m;       /* != 0: block is in fixed-parameter Golomb mode with this modulus */
} sla_hip_rice_job;

/* One block of the output image. */
typedef struct sla_hip_pack_block {
  uint64_t blk_off;        /* first sample inside a channel plane                              */
  uint64_t out_off;        /* byte offset of the block inside the .sla image                  */
  uint32_t num_samples;
  uint32_t type;           /* 0 compressed, 1 silent, 2 raw                                    */
  uint32_t header_off;     /* offset of the pre-packed header bytes in the header pool         */
  uint32_t header_bytes;
  uint32_t out_bytes;      /* total encoded size of the block                                  */
  uint32_t raw_bits;       /* RAW blocks: bits per sample of channel 0 (bps - offset_lshift)   */
  uint32_t golomb_m[8];    /* per channel: 0 = adaptive recursive Rice, else Golomb modulus    */
} sla_hip_pack_block;

/* ---- (1) kernel launchers ----------------------------------------------- */

/* Tuning knobs of the launchers.  Nothing on the launch path reads the environment: an encoder handle owns one of
 * these (filled once in SLAEncoder_Create, changed through sla_hip_encoder_set_option) and names it to the
 * launchers of the calling host thread before it launches; a thread that never called sla_hip_use_tuning (or
 * passed NULL) gets the defaults = all zeros.  None of the knobs changes a result, only how the work is laid out --
 * the three certification margins ("plan_margin", "cert_safety", "block_cert_safety") may only be WIDENED beyond their
 * built-in values (1e-4, 64, 16; plan_margin / cert_safety also take 0 = built-in value / no certificate): smaller
 * values would weaken the certificates byte-identity rests on, and sla_hip_encoder_set_option refuses them (a
 * plan_margin below 1e-4 in a sla_hip_tuning handed to sla_hip_use_tuning is read as 0). */
typedef struct sla_hip_tuning {
  uint32_t lpc_pack;            /* windows per workgroup of k_lpc / k_lpc_blocks, 0 = automatic                      */
  uint32_t lpc_threads;         /* 256 or 512 threads per k_lpc workgroup, 0 = automatic                             */
  uint32_t lpc_blocks_chains;   /* 1: chosen blocks through k_lpc's serial chains instead of k_lpc_blocks            */
  uint32_t tail_waves;          /* waves per tail workgroup (1..4), 0 = automatic (4)                                */
  uint32_t lpc_tile;            /* steps per tile of k_lpc_blocks' wide packs: 24, or 0 / 48 = 48 where it fits         */
  uint32_t tail_taps;           /* k_tailk: taps of each history per lane, 1 / 2 / 4; 0 = by the number of jobs (default) */
  double   plan_margin;         /* certification margin of k_plan, 0 = 1e-4 (tests raise it to force the host plan)  */
  uint32_t rice_lanes;          /* Rice parameter walk: 1 = one lane per job (k_rice_k), 2 = the two-lane pipeline (k_rice_k2), 0 = by the number of jobs */
  uint32_t lattice_plain;       /* 1: every lattice stage in the wrapping four-instruction form (round 3); 0 = the shortest form each stage's
                                   operand bound allows (same results: tests run both) */
  uint32_t cert_audit;          /* N > 0: every N-th (block, channel) pair that sla_hip_launch_lpc_blocks_cert CERTIFIES is analysed by the
                                   exact kernels as well, which compare codes, lattice coefficients and the RAW side with what the certified
                                   run stored: d_cert_flag 4 = audited and equal, 5 = the certificate was wrong (the encoder fails the call) */
  uint32_t ltm_int;             /* 1: sla_hip_launch_ltm_cert_x takes its autocorrelation from exact integer sums on the int8 matrix pipe
                                   (k_ltm_acf_int) instead of the FMA transform (k_ltm_acf_fast); the encoder's default.  (The field fills
                                   what was the struct's tail padding: its size is unchanged.) */
} sla_hip_tuning;
void sla_hip_use_tuning(const sla_hip_tuning* tuning);

/* Optional extras of ONE launch, for the launchers that have an `_x` twin (same arguments + `const sla_hip_launch_extra*`, NULL =
 * none; the plain name is the twin with NULL).  What the encoder's driver needs and a caller of a single launcher usually
 * does not: */
typedef struct sla_hip_launch_extra {
  unsigned long long* d_span;       /* two device words (zeroed by the caller): [0] = max(~start), [1] = max(end) of the launch's execution on
                                       the device's constant 100 MHz clock -- first workgroup in to last workgroup out, without the time the
                                       launch waits for resources behind kernels of other streams (sla_hip_last_kernel_ms) */
  const uint32_t* d_group_count;    /* sla_hip_launch_lpc_blocks_cert_x: num_groups is an upper bound, the kernels take the number of groups from
                                       the running numbers sla_hip_launch_expand keeps on the device (the launch can be queued before the host
                                       has seen the count) */
  uint32_t* clear_ptr[3];           /* sla_hip_launch_search_exact_x: up to three regions of device words that the first workgroup of its first */
  uint32_t  clear_words[3];         /* kernel zeroes on the way (instead of one fill kernel each in front of it) */
  uint32_t* d_rice_init;            /* sla_hip_launch_tail_x: num_jobs device words; the kernel stores every job's initial Rice parameter beside
                                       fold_sum[j] -- the mean fold_sum[j] / blk_len, at least 1, as it survives the coder's 24.8 fixed-point word
                                       (1 for a job with blk_len 0).  NULL: only fold_sum is written */
} sla_hip_launch_extra;
int sla_hip_launch_lpc_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                         const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window, uint32_t max_cands_per_group,
                         const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                         double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                         sla_hip_stream_t stream, const sla_hip_launch_extra* extra);
int sla_hip_launch_lpc_blocks_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                                double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                                int32_t* d_lattice_residual, sla_hip_stream_t stream, const sla_hip_launch_extra* extra);
int sla_hip_launch_lpc_blocks_cert_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                     const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                     const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                                     double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                                     uint32_t* d_cert_flag, uint32_t* d_fallback_list, uint32_t* d_fallback_count,
                                     double safety, uint32_t bits_per_sample, sla_hip_stream_t stream, const sla_hip_launch_extra* extra);

/* d_or_mask[0] = OR of every input word, d_or_mask[1] = number of all-zero words of the mask; d_nz_mask: one
 * bit per sample "any channel non-zero after right-justify / mid-side", ceil(num_samples/64) words. */
int sla_hip_launch_prepass(const int32_t* d_pcm, uint64_t plane_stride, uint32_t num_channels,
                           uint32_t num_samples, uint32_t bits_per_sample, uint32_t mid_side,
                           uint32_t* d_or_mask, uint64_t* d_nz_mask, sla_hip_stream_t stream);
/* Search beside the prepass (option "search_early"): d_early names SLA_HIP_EARLY_WORDS device words that the prepass and
 * the kernels started beside it share.  d_early[SLA_HIP_EARLY_CANCEL] must be 0 before either is launched (nothing here
 * clears it: the encoder clears it with the first search kernel of a launch that does not run beside a prepass); k_prepass
 * sets it to 1 the moment it meets an all-zero mask word, and one thread behind it on the same stream sets it for an OR
 * word of 0 or samples wider than bits_per_sample and stores the file's offset_lshift in d_early[SLA_HIP_EARLY_LSHIFT]
 * (0 in those two cases).  Every kernel of the `_early` launchers below reads the flag once at its start (the tile sums:
 * once per wave) and returns when it is set; no kernel ever waits for a word in memory.
 * sla_hip_launch_search_exact_early: exact_limit is the limit of offset_lshift 0; the tile sums are queued at once, then
 * the stream waits for prepass_done (a hipEvent_t recorded behind sla_hip_launch_prepass_early on its stream) and the
 * kernels behind the wait scale the limit by 4^offset_lshift.  sla_hip_launch_expand_early: int_shift is the shift of
 * offset_lshift 0, the kernel adds the stored one; cancelled, it leaves d_run and counts alone.  Both, and
 * sla_hip_launch_plan_early, must be queued on that stream behind that wait.  d_early == NULL (where allowed: plan, expand)
 * is the plain launcher.
 * max_workgroups (0: no limit) caps the prepass's grid, its waves walking on through the file: the tile sums beside it read
 * the same samples, and a prepass that takes all the memory bandwidth there is slows them by more than it gains. */
#define SLA_HIP_EARLY_CANCEL 0
#define SLA_HIP_EARLY_LSHIFT 1
#define SLA_HIP_EARLY_WORDS  2
int sla_hip_launch_prepass_early(const int32_t* d_pcm, uint64_t plane_stride, uint32_t num_channels,
                                 uint32_t num_samples, uint32_t bits_per_sample, uint32_t mid_side,
                                 uint32_t* d_or_mask, uint64_t* d_nz_mask, uint32_t* d_early, uint32_t max_workgroups,
                                 sla_hip_stream_t stream);
/* The same pass that also stores the OR of every 1024-sample tile (d_tile_or: ceil(num_samples / 4096) * 4 words):
 * a batch of files laid out back to back on 1024-sample boundaries gets its offset_lshift per file from them. */
#define SLA_HIP_PREPASS_TILE 1024u
int sla_hip_launch_prepass_tiles(const int32_t* d_pcm, uint64_t plane_stride, uint32_t num_channels,
                                 uint32_t num_samples, uint32_t bits_per_sample, uint32_t mid_side,
                                 uint32_t* d_or_mask, uint64_t* d_nz_mask, uint32_t* d_tile_or, sla_hip_stream_t stream);

/* Per file of a batch laid out back to back on SLA_HIP_PREPASS_TILE boundaries (sla_hip_analyze_batch_device), from the results
 * of sla_hip_launch_prepass_tiles: d_info[3 i] = OR of the file's words, [3 i + 1] = all-zero 64-sample mask words inside it,
 * [3 i + 2] = 1 when its last super-frame (fewer than 127 samples left of it) is all zero.  No zero word and no such tail
 * anywhere: no block of the batch can be SILENT (reference src/SLAEncoder.c:392-408), the mask never has to leave the device. */
int sla_hip_launch_batch_scan(const uint64_t* d_nz_mask, const uint32_t* d_tile_or, const uint32_t* d_file_start,
                              const uint32_t* d_file_len, uint32_t num_files, uint32_t max_block_samples,
                              uint32_t* d_info, sla_hip_stream_t stream);

/* The run list of a silence mask: what the host's super-frame hop and its "is this block all zero" test need to know
 * instead of the mask itself (option "silence_runs").
 * d_nz_mask: the prepass mask, 16-byte aligned, ceil(span / 64) words, bits at or above span zero.  Segments (the files of a
 * batch): device arrays d_seg_start / d_seg_len of num_segs entries, ascending, not overlapping, starts multiples of
 * SLA_HIP_PREPASS_TILE, every bit outside them zero; d_seg_start == NULL: one segment [0, span) (d_seg_len, num_segs ignored).
 * The list holds every maximal run of zero bits inside a segment that is at least min_run samples long or ends at the
 * segment's end (any length; an empty segment has none).  A run never crosses a segment boundary: the zero gap between two
 * files neither joins their runs nor makes one.  Whoever treats every sample outside the listed runs as non-zero gets, for
 * min_run = SLA_HIP_ZERO_RUN_MIN, the hop tables and the block types of the true mask: a super-frame or block can only be
 * SILENT when it is at least SLA's minimum block long or ends at its file's end (reference src/SLAEncoder.c:392-408,
 * src/SLAPredictor.c:1623-1630).
 * d_count[0] = number of such runs, exact also beyond `capacity`; nothing is written at or behind d_runs[capacity]; when the
 * count exceeds the capacity the list's content is unspecified.  The order of the entries is unspecified: sort on the host.
 * min_run >= 64 (a run inside one mask word then never qualifies); span <= SLA_HIP_ZERO_RUN_MAX_SPAN.
 * d_scratch: SLA_HIP_ZERO_RUN_SCRATCH_BYTES(span) bytes, 4-byte aligned; the launcher initialises what it needs of it and of
 * d_count (two kernels on `stream`, no memset, no synchronisation).
 * Returns SLA_APIRESULT_INVALID_ARGUMENT before any launch for a NULL mask, runs, count or scratch pointer, a mask that is
 * not 16-byte aligned, capacity == 0, min_run < 64, a span over the limit, or a table (d_seg_start != NULL) without
 * d_seg_len or with num_segs == 0. */
typedef struct sla_hip_zero_run { uint32_t start; uint32_t length; } sla_hip_zero_run;   /* 8 bytes */
#define SLA_HIP_ZERO_RUN_MIN 2048u      /* what the encoder passes: SLA's minimum block */
#define SLA_HIP_ZERO_RUN_TILE 1024u     /* mask words one workgroup scans (65536 samples) */
#define SLA_HIP_ZERO_RUN_MAX_SPAN 0xFFFF0000u
#define SLA_HIP_ZERO_RUN_SCRATCH_BYTES(span) \
  (4u * (size_t)(SLA_HIP_ZERO_RUN_TILE / 128u + 1u) * (size_t)((((uint64_t)(span) + 63u) / 64u + SLA_HIP_ZERO_RUN_TILE - 1u) / SLA_HIP_ZERO_RUN_TILE + 1u))
int sla_hip_launch_zero_runs(const uint64_t* d_nz_mask, uint32_t span,
                             const uint32_t* d_seg_start, const uint32_t* d_seg_len, uint32_t num_segs,
                             uint32_t min_run, sla_hip_zero_run* d_runs, uint32_t capacity,
                             uint32_t* d_count, uint32_t* d_scratch, sla_hip_stream_t stream);

/* Autocorrelation + Levinson-Durbin for every candidate of every group.
 * d_out: per slot (order+2) doubles = { r[0], parcor[0..order] }.
 * When d_code/d_kint/d_rshift are non-NULL (chosen blocks: one candidate per
 * group covering the whole window) the coefficient quantiser runs too. */
int sla_hip_launch_lpc(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                       const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                       uint32_t max_cands_per_group,
                       const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                       double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                       sla_hip_stream_t stream);

/* Chosen blocks in one launch: sla_hip_launch_lpc in its quantiser form (one candidate per group = the whole
 * block) followed, inside the same workgroups, by the PARCOR lattice of sla_hip_launch_lattice with the
 * coefficients just quantised -> d_lattice_residual (plane layout of d_pcm).  Orders up to
 * SLA_HIP_FUSED_LATTICE_MAX_ORDER (the recursion runs with one lane of a wave per coefficient, k[0] included);
 * SLA_APIRESULT_INVALID_ARGUMENT above. */
#define SLA_HIP_FUSED_LATTICE_MAX_ORDER 63u
int sla_hip_launch_lpc_blocks(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                              const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                              const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                              double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                              int32_t* d_lattice_residual, sla_hip_stream_t stream);

/* Chosen blocks, certified route (the default of the block stage; option "block_cert"): the autocorrelation of every
 * windowed block in ANY summation order (k_acf_blocks: FMAs, one wave per block and channel), the reference's
 * Levinson-Durbin recursion on it and a per-block certificate that the quantised PARCOR codes (reference
 * src/SLAEncoder.c:567-589) and the RAW decision (:553-565) cannot differ from the reference's although the doubles may
 * differ in their last bits; blocks that do not certify are appended to d_fallback_list (group indices, count in
 * *d_fallback_count) and redone by the exact chain kernels of sla_hip_launch_lpc before the call's work on `stream`
 * ends.  d_cert_flag[slot]: 0 = certified, 2 = exact (4 / 5: audited, see sla_hip_tuning.cert_audit).  safety >= 1 scales the
 * certificate's bound (the encoder: 16).  The bound is a FIRST-ORDER perturbation bound of the Levinson-Durbin recursion times
 * that factor, validated empirically -- not a proof; the audit is the standing check on it.
 * Orders above 51 (more than 52 lags) are not covered (SLA_APIRESULT_EXCEED_HANDLE_CAPACITY): use sla_hip_launch_lpc. */
int sla_hip_launch_lpc_blocks_cert(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                   const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                   const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                                   double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                                   uint32_t* d_cert_flag, uint32_t* d_fallback_list, uint32_t* d_fallback_count,
                                   double safety, uint32_t bits_per_sample, sla_hip_stream_t stream);
/* k_acf_blocks alone, in the instantiation sla_hip_launch_lpc_blocks_cert picks for `order`, and nothing behind it: the
 * launch stores the sums themselves -- d_out[slot * (order + 2) + 1 + lag] = r[lag], lag = 0 .. order (element 0 of the slot
 * is not written) -- and d_rshift[slot], the quantiser's shift.  For tests that hold the sums against exact ones
 * (tests/test_gpu_acf_error.py).  The same refusals as sla_hip_launch_lpc_blocks_cert: orders above 51 return
 * SLA_APIRESULT_EXCEED_HANDLE_CAPACITY before anything is launched. */
int sla_hip_launch_acf_blocks(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                              const sla_hip_lpc_group* d_groups, uint32_t num_groups, const double* d_window_pool,
                              double* d_out, uint32_t* d_rshift, sla_hip_stream_t stream);

/* sla_hip_launch_lpc restricted to the groups that sla_hip_launch_search_exact flagged (NaN in r[0] of the group's
 * first slot): everything else returns at once and keeps its result.  *d_rerun_counter (may be NULL) is
 * incremented by the number of groups that were analysed. */
int sla_hip_launch_lpc_rerun(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                             const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                             uint32_t max_cands_per_group, const sla_hip_lpc_cand* d_cands,
                             double* d_out, uint32_t* d_rerun_counter, sla_hip_stream_t stream);

/* The far-window LPC stage: sla_hip_launch_lpc -- same arguments, same outputs in both of its forms, bit for bit -- for windows
 * that do not fit the LDS: max_window up to SLA_HIP_LPC_FAR_MAX_WINDOW, orders 1 to 255, any number of candidates per group
 * (no LDS bound on them).  The windows are staged as doubles into d_scratch (scratch_slots x max_window doubles; groups beyond
 * the slots are taken in passes of scratch_slots groups, group g in slot g % scratch_slots) and the reference's serial chains
 * (src/SLAPredictor.c:331-388) run on them out of the L2: one thread per (candidate, lag), a window's chains spread over as many
 * workgroups as they fill; Levinson-Durbin (and, with d_code / d_kint / d_rshift, the quantiser) with one lane per candidate.
 * Search form (d_code == NULL): d_window_pool may be NULL when every group is SLA_HIP_NO_WINDOW.  Block form: one candidate per
 * group; d_window_pool must be given.  Both forms stage through the scratch (the chains take a pointer to doubles).
 * Returns SLA_APIRESULT_INVALID_ARGUMENT before any launch for a NULL d_pcm, d_groups, d_cands, d_out or d_scratch,
 * scratch_slots == 0, order outside 1..255, max_window == 0 or above SLA_HIP_LPC_FAR_MAX_WINDOW, max_cands_per_group == 0, some
 * but not all of d_code / d_kint / d_rshift, or a block form with max_cands_per_group != 1 or without d_window_pool.
 * A group's num_samples must not exceed max_window and a candidate must lie inside its group's window (one that does not is
 * analysed as empty; nothing is read or written outside the slots).  Slots of groups not in the launch are not touched.
 * extra->d_span: first kernel in to last kernel out.  Slower per chain than k_lpc wherever both apply: the encoder takes it
 * only for encode parameters above 16 384 samples. */
#define SLA_HIP_LPC_FAR_MAX_WINDOW 65535u
int sla_hip_launch_lpc_far(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                           const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                           uint32_t max_cands_per_group,
                           const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                           double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                           double* d_scratch, uint32_t scratch_slots, sla_hip_stream_t stream);
int sla_hip_launch_lpc_far_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                             const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                             uint32_t max_cands_per_group,
                             const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                             double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                             double* d_scratch, uint32_t scratch_slots, sla_hip_stream_t stream,
                             const sla_hip_launch_extra* extra);

/* Partition search without serial chains (reference src/SLAPredictor.c:1615-1649 + :331-388).
 * The search analyses the un-windowed samples: integers times a power of two.  As long as the energy of
 * a group's window stays below `exact_limit` (= 2^51 units^2, unit = the common power-of-two factor of
 * the samples) every product and every partial sum of the reference's autocorrelation is exactly
 * representable, so the order of summation is free: each wave sums one SLA_HIP_XTILE-sample tile per lag,
 * candidates are prefix differences of tile sums minus the pairs that straddle the candidate's end, and
 * the result is bit-identical to the serial order.  Groups: one per (super-frame, channel) listing ALL its
 * candidates; candidates must start on a tile boundary and end on one or at the end of the window.
 * d_tile_sums: num_groups * SLA_HIP_XTILES * 2 * sla_hip_search_exact_lags(order) doubles of scratch
 * (per tile P[lags] | X[lags]; only the entries of the lags <= order are defined afterwards).
 * A group whose energy reaches the limit: with cert_safety <= 0 it gets NaN in r[0] of every candidate and the
 * caller reruns it through sla_hip_launch_lpc_rerun.  With cert_safety > 0 (the encoder passes 64) its candidates
 * keep their tile-sum results -- close to, but no longer bit-identical with, the reference's serially rounded sums --
 * in the slot layout { r0, w, log2(e_p / r0), 0, .. }: parcor[0] (0 for every exact candidate) holds the half width w
 * of log2(e_p), e_p = r0 * prod(1 - k_j^2), parcor[1] the logarithm itself instead of a coefficient (orders <= 64):
 * the reference's own value of log2(e_p) provably lies within +-w (Loewner-order bracket of the prediction error over
 * every Toeplitz matrix within cert_safety x the summation error bounds of both sides; see k_search_finish), or
 * +inf when no such bracket exists.  The code-length estimate depends on the autocorrelation only through e_p, so
 * sla_hip_launch_plan can decide whether the partition is certain. */
#define SLA_HIP_XTILE  1024u
#define SLA_HIP_XTILES 16u
uint32_t sla_hip_search_exact_lags(uint32_t order);      /* padded lag count, 0: order not supported */
int sla_hip_launch_search_exact(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                uint32_t max_cands_per_group,
                                const sla_hip_lpc_cand* d_cands, double* d_tile_sums, double* d_out,
                                double exact_limit, double cert_safety, uint32_t* d_any_exact /* one scratch word, may be NULL */,
                                sla_hip_stream_t stream);
int sla_hip_launch_search_exact_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                uint32_t max_cands_per_group,
                                const sla_hip_lpc_cand* d_cands, double* d_tile_sums, double* d_out,
                                double exact_limit, double cert_safety, uint32_t* d_any_exact /* one scratch word, may be NULL */,
                                sla_hip_stream_t stream, const sla_hip_launch_extra* extra);
/* (beside the prepass: see sla_hip_launch_prepass_early; num_groups == 0 is refused -- nothing would queue the wait) */
int sla_hip_launch_search_exact_early(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                uint32_t max_cands_per_group,
                                const sla_hip_lpc_cand* d_cands, double* d_tile_sums, double* d_out,
                                double exact_limit, double cert_safety, uint32_t* d_any_exact /* one scratch word, may be NULL */,
                                sla_hip_stream_t stream, const sla_hip_launch_extra* extra,
                                const uint32_t* d_early, void* prepass_done /* hipEvent_t */);

/* The tile-sum search for windows of up to SLA_HIP_LPC_FAR_MAX_WINDOW samples (64 tiles): sla_hip_launch_search_exact's exact
 * form -- the same tile kernels, the same group and candidate rules, the same strict limit (energy < exact_limit is exact) --
 * without a certificate: a group whose energy reaches the limit gets NaN in r[0] of every candidate's slot and nothing else
 * written, and the caller reruns it through sla_hip_launch_lpc_far_rerun.  The exactness argument does not depend on the
 * number of tiles: every partial sum of any order of summation is bounded by the window's energy.
 * d_tile_sums: num_groups * SLA_HIP_XTILES_FAR * 2 * sla_hip_search_exact_lags(order) doubles of scratch, per tile
 * P[lags] | X[lags] as above with that stride.  k_search_finish_far spreads a group's candidates over workgroups of 256, each
 * of which stages the running prefix of the group's P over the tiles and its X in LDS: a candidate's r[lag] is
 * prefix[last + 1] - prefix[first] - X[last].  Any max_cands_per_group.  For windows of at most 16 384 samples every output
 * word equals sla_hip_launch_search_exact's with cert_safety = 0.
 * Returns SLA_APIRESULT_INVALID_ARGUMENT for a NULL d_pcm, d_groups, d_cands, d_tile_sums or d_out, max_window == 0 or
 * max_cands_per_group == 0, and SLA_APIRESULT_EXCEED_HANDLE_CAPACITY for orders above 51 (or 0) or max_window above
 * SLA_HIP_LPC_FAR_MAX_WINDOW, before any launch.  num_groups == 0 is success.  A group's num_samples must not exceed
 * max_window; a candidate that leaves its window is analysed as empty.  Slots of groups not in the launch are not touched.
 * extra->clear_ptr as sla_hip_launch_search_exact_x; extra->d_span: the execution span of k_search_finish_far. */
#define SLA_HIP_XTILES_FAR 64u
int sla_hip_launch_search_far(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                              const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                              uint32_t max_cands_per_group,
                              const sla_hip_lpc_cand* d_cands, double* d_tile_sums, double* d_out,
                              double exact_limit, sla_hip_stream_t stream);
int sla_hip_launch_search_far_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                uint32_t max_cands_per_group,
                                const sla_hip_lpc_cand* d_cands, double* d_tile_sums, double* d_out,
                                double exact_limit, sla_hip_stream_t stream, const sla_hip_launch_extra* extra);
/* sla_hip_launch_lpc_far's search form restricted to the groups that sla_hip_launch_search_far flagged (NaN in r[0] of the
 * group's first slot): every candidate of such a group is analysed as sla_hip_launch_lpc_far analyses it, everything else keeps
 * its result word for word.  *d_rerun_counter (may be NULL) is incremented by the number of groups analysed.  The verdict on a
 * group is taken from its first slot by the kernels that run BEFORE any slot's r[0] is rewritten (they hand it on in r[0] of
 * every candidate's own slot, which the last kernel decides by); r[0] of the other slots of an unflagged group must not be NaN.
 * Arguments, scratch and refusals as sla_hip_launch_lpc_far's search form. */
int sla_hip_launch_lpc_far_rerun(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                 const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                 uint32_t max_cands_per_group, const sla_hip_lpc_cand* d_cands,
                                 double* d_out, double* d_scratch, uint32_t scratch_slots,
                                 uint32_t* d_rerun_counter, sla_hip_stream_t stream);

/* The scalar tail of the partition search on the device: estimated code length per candidate, adjacency
 * matrix, shortest path (reference src/SLAPredictor.c:416-468, 1521-1581, 1615-1692).  d_groups: the groups of
 * sla_hip_launch_search_exact, num_channels consecutive entries per super-frame; d_lpc_out: their (or
 * sla_hip_launch_lpc's) output.  Per super-frame: d_status 0 = d_num_parts block lengths in d_parts
 * (SLA_HIP_PLAN_NODES entries per super-frame) are exactly what the reference's host arithmetic decides;
 * 1 = a comparison came closer than the device logarithm can be trusted (or the input was flagged / not
 * finite): the caller must redo this super-frame on the host from the candidates' doubles; 2 = the super-frame's
 * candidates were certified tile sums (parcor[0] = width > 0) and some comparison came closer than the widths allow:
 * every candidate of the super-frame has been flagged (NaN in r[0]) -- the caller reruns them as serial chains
 * (sla_hip_launch_lpc_rerun) and decides on the host. */
#define SLA_HIP_PLAN_NODES 17u
int sla_hip_launch_plan(const sla_hip_lpc_group* d_groups, uint32_t num_superframes, uint32_t num_channels,
                        uint32_t order, uint32_t bits_per_sample, const sla_hip_lpc_cand* d_cands,
                        double* d_lpc_out, uint32_t* d_parts, uint32_t* d_num_parts, uint32_t* d_status,
                        sla_hip_stream_t stream);
int sla_hip_launch_plan_early(const sla_hip_lpc_group* d_groups, uint32_t num_superframes, uint32_t num_channels,
                              uint32_t order, uint32_t bits_per_sample, const sla_hip_lpc_cand* d_cands,
                              double* d_lpc_out, uint32_t* d_parts, uint32_t* d_num_parts, uint32_t* d_status,
                              sla_hip_stream_t stream, const uint32_t* d_early);

/* Block table of one run of super-frames from sla_hip_launch_plan's partitions, written on the device, so that the
 * block-stage kernels can follow the partition search without the host building and uploading their descriptors
 * (the host part of src/SLAEncoder.c:846-869: the walk over the super-frames that numbers the blocks).
 * d_superframes: the run, in file order.  A live super-frame names its row of d_parts / d_num_parts / d_status; one
 * that is a single SILENT block (live == SLA_HIP_NOT_LIVE) takes one block index and produces no group.
 * sla_hip_launch_expand treats no block of a live super-frame as silent: for input whose non-zero mask has no all-zero
 * word (sla_hip_launch_prepass: d_or_mask[1] == 0), where a block of SLA's minimum length cannot be.
 * sla_hip_launch_expand_masked (round 4) also takes the prepass mask (d_nonzero_mask, bit s of word s / 64 = some
 * channel's sample s is not zero; NULL = the plain call): a block of a live super-frame whose samples are all zero is
 * a SILENT block (src/SLAEncoder.c:392-408) -- it takes a block index and produces no group, exactly as the host's walk
 * numbers it -- so that files WITH silence get device-written tables too.
 * d_run: 4 words, zeroed by the caller before the first run of a file; d_prefix: 2 * num_superframes words of scratch (the
 * numbering is done by one workgroup, k_expand_scan, the descriptors are written by the whole device, k_expand_write).
 * Per (block, channel), numbered on from d_run[0] blocks / d_run[1] groups: d_groups[g] (windowed form: win_off looked
 * up by block length in the d_win_len / d_win_off list, cand_first = g, slot_first = block * num_channels + channel),
 * d_cands[g] = {0, length}, d_acf_jobs[g].  counts (which may be page-locked host memory: the caller can poll
 * counts[3]): [0] blocks and [1] groups of this run, [2] 1 = tables valid, 0 = some super-frame was not certified
 * (d_status != 0), a length has no window, the tables are full or an earlier run failed (d_run[2] != 0) -- nothing
 * may be launched from them, and every later run on the same d_run fails too; [3] = sequence, written last. */
#define SLA_HIP_NOT_LIVE 0xFFFFFFFFu
typedef struct sla_hip_superframe {
  uint32_t start;          /* first sample */
  uint32_t window;         /* samples (a SILENT one: the length of the zero run) */
  uint32_t live;           /* row of the plan's arrays, or SLA_HIP_NOT_LIVE */
  uint32_t pad_;
} sla_hip_superframe;
int sla_hip_launch_expand(const sla_hip_superframe* d_superframes, uint32_t num_superframes,
                          const uint32_t* d_parts, const uint32_t* d_num_parts, const uint32_t* d_status,
                          uint32_t num_channels, uint32_t int_shift,
                          const uint32_t* d_win_len, const uint32_t* d_win_off, uint32_t num_windows,
                          uint32_t* d_run, uint32_t* d_prefix, sla_hip_lpc_group* d_groups, sla_hip_lpc_cand* d_cands,
                          sla_hip_acf_job* d_acf_jobs, uint32_t group_capacity,
                          uint32_t* counts, uint32_t sequence, sla_hip_stream_t stream);
int sla_hip_launch_expand_masked(const sla_hip_superframe* d_superframes, uint32_t num_superframes,
                          const uint32_t* d_parts, const uint32_t* d_num_parts, const uint32_t* d_status,
                          uint32_t num_channels, uint32_t int_shift,
                          const uint32_t* d_win_len, const uint32_t* d_win_off, uint32_t num_windows,
                          uint32_t* d_run, uint32_t* d_prefix, sla_hip_lpc_group* d_groups, sla_hip_lpc_cand* d_cands,
                          sla_hip_acf_job* d_acf_jobs, uint32_t group_capacity,
                          uint32_t* counts, uint32_t sequence, const uint64_t* d_nonzero_mask, sla_hip_stream_t stream);
int sla_hip_launch_expand_early(const sla_hip_superframe* d_superframes, uint32_t num_superframes,
                          const uint32_t* d_parts, const uint32_t* d_num_parts, const uint32_t* d_status,
                          uint32_t num_channels, uint32_t int_shift,
                          const uint32_t* d_win_len, const uint32_t* d_win_off, uint32_t num_windows,
                          uint32_t* d_run, uint32_t* d_prefix, sla_hip_lpc_group* d_groups, sla_hip_lpc_cand* d_cands,
                          sla_hip_acf_job* d_acf_jobs, uint32_t group_capacity,
                          uint32_t* counts, uint32_t sequence, const uint64_t* d_nonzero_mask, sla_hip_stream_t stream,
                          const uint32_t* d_early);

/* Building blocks of the per-call predictor API (include/SLAPredictor.h), also usable on their own:
 *   sla_hip_launch_lpc_f64      sla_hip_launch_lpc in its search form on samples that already are doubles
 *                               (group.pcm_off indexes d_samples; no conversion, window or pre-emphasis)
 *   sla_hip_launch_lattice_raw  sla_hip_launch_lattice on samples that already are the lattice input (no shift,
 *                               no mid/side, no pre-emphasis)
 *   sla_hip_launch_tail_stages  sla_hip_launch_tail with the LMS stage optional (job.pitch = 0 switches the
 *                               long-term stage off as always); d_fold_sum still receives the zig-zag sums
 *   sla_hip_launch_emphasis_*   pre-emphasis as a pass of its own, out[n] = in[n] - ((in[n-1] * (2^s - 1)) >> s) */
int sla_hip_launch_lpc_f64(const double* d_samples, uint32_t order,
                           const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                           uint32_t max_cands_per_group, const sla_hip_lpc_cand* d_cands,
                           double* d_out, sla_hip_stream_t stream);
int sla_hip_launch_lattice_raw(const int32_t* d_samples, uint64_t plane_stride, uint32_t order,
                               const sla_hip_lattice_chunk* d_chunks, uint32_t num_chunks,
                               const int32_t* d_kint, int32_t* d_residual, sla_hip_stream_t stream);
int sla_hip_launch_tail_stages(const int32_t* d_res_in, int32_t* d_res_out, uint64_t plane_stride,
                               const sla_hip_tail_job* d_jobs, uint32_t num_jobs, uint32_t longterm_order,
                               uint32_t lms_order, uint32_t skip_lms, uint64_t* d_fold_sum, sla_hip_stream_t stream);
int sla_hip_launch_emphasis_i32(const int32_t* d_in, int32_t* d_out, uint32_t num_samples, int32_t previous,
                                uint32_t coef_shift, sla_hip_stream_t stream);
int sla_hip_launch_emphasis_f64(const double* d_in, double* d_out, uint32_t num_samples, uint32_t coef_shift,
                                sla_hip_stream_t stream);

/* Integer pre-emphasis + PARCOR lattice; one wave per chunk. */
int sla_hip_launch_lattice(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                           const sla_hip_lattice_chunk* d_chunks, uint32_t num_chunks,
                           const int32_t* d_kint, int32_t* d_residual, sla_hip_stream_t stream);

/* The same lattice, the waves derived on the device from block descriptors (one sla_hip_lpc_group per (block, channel):
 * pcm_off, num_samples, channel, int_shift, slot_first -> coefficients at d_kint[slot_first * (order + 1)]); max_window =
 * the longest block.  What the whole-file driver uses: no per-chunk descriptors to build and upload. */
int sla_hip_launch_lattice_groups(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                  const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                  const int32_t* d_kint, int32_t* d_residual, sla_hip_stream_t stream);
int sla_hip_launch_lattice_groups_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                  const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                  const int32_t* d_kint, int32_t* d_residual, sla_hip_stream_t stream, const sla_hip_launch_extra* extra);

/* Autocorrelation of each job's residual, computed exactly as the reference's real-FFT route does
 * (zero-padded to fft_size, forward, |.|^2, inverse).  head == SLA_HIP_ACF_RECORD: per job a 12-double
 * record {code (0 silent, 1 ok, 2 no candidate), chosen pitch lag, acf[0..4], acf[chosen-2..chosen+2]}
 * after the reference's peak scan (src/SLAPredictor.c:866-924); any other head: the first `head` lags.  d_twiddles holds the
 * SLA_HIP_TWIDDLE_DOUBLES(fft_size) doubles produced by the host with the reference's recurrence (layout: sla_kernels.hip).
 * fft_size*8 bytes must fit SLA_HIP_LDS_BUDGET, otherwise d_scratch (scratch_slots x fft_size doubles
 * of device memory) is used as the work area. */
#define SLA_HIP_ACF_RECORD 12u
#define SLA_HIP_TWIDDLE_DOUBLES(fft_size) (6u * (size_t)(fft_size))
int sla_hip_launch_ltm_acf(const int32_t* d_residual, uint64_t plane_stride,
                           const sla_hip_acf_job* d_jobs, uint32_t num_jobs, uint32_t fft_size,
                           const double* d_twiddles, double* d_scratch, uint32_t scratch_slots,
                           double* d_acf_head, uint32_t head, sla_hip_stream_t stream);
int sla_hip_launch_ltm_acf_x(const int32_t* d_residual, uint64_t plane_stride,
                           const sla_hip_acf_job* d_jobs, uint32_t num_jobs, uint32_t fft_size,
                           const double* d_twiddles, double* d_scratch, uint32_t scratch_slots,
                           double* d_acf_head, uint32_t head, sla_hip_stream_t stream, const sla_hip_launch_extra* extra);

/* Long-term pitch and taps on the device: one lane per job solves the Wiener system around the lag k_ltm_acf chose
 * (d_acf_records: num_jobs compact records, head SLA_HIP_ACF_RECORD) and writes the job k_tail reads -- position and
 * channel from d_groups[job], pitch (0: stage bypassed) and the quantised taps (src/SLAPredictor.c:855-863, 913-979;
 * src/SLAUtility.c:487-674; src/SLAEncoder.c:629-640).  The reference's long double refinement residual is computed
 * in integer arithmetic with a 64-bit significand, so the taps are the reference's bit for bit.  longterm_order: 1, 3, 5. */
int sla_hip_launch_ltm_solve(const double* d_acf_records, const sla_hip_lpc_group* d_groups, uint32_t num_jobs,
                             uint32_t longterm_order, sla_hip_tail_job* d_jobs, sla_hip_stream_t stream);

/* The certified long-term stage: the same job table as above, but the autocorrelation comes from an any-order FMA
 * transform of half the reference's size or less (k_ltm_acf_fast) and carries an error bound
 *     |r'[j] - r_ref[j]| <= eps = safety * SLA_HIP_LTM_CERT_C * 2^-53 * log2(fft_size) * r'[0]       (j <= 261)
 * that covers the fast transform's error and the reference's own (first order; DESIGN section 2 has the derivation and
 * the measured errors).  A job whose every decision -- pitch scan, arg-max, the solver's branches, sum|coef| >= 1, the
 * 15-bit tap quantiser -- is safe under +-eps gets the pitch and taps of sla_hip_launch_ltm_solve by proof; every other
 * job is recomputed by the exact kernels from a device-resident list, in the same call and on the same stream.
 *   d_fast_twiddles  SLA_HIP_FAST_TWIDDLE_DOUBLES(fft_size) doubles from sla_hip_ltm_fast_twiddles
 *   d_eps            num_jobs doubles (work area: the bound of every job, < 0 = pick not certified)
 *   d_list           num_jobs words (work area), d_counters: 4 words, ZERO before the call; afterwards {list entries,
 *                    uncertified jobs, audited jobs found equal, audited jobs found different} (tuning cert_audit = N
 *                    sends every N-th certified job through the exact kernels as well and compares pitch and taps)
 *   safety           >= SLA_HIP_LTM_CERT_SAFETY_MIN
 * fft_size (the reference's: roundup2(2 * capacity)) must satisfy sla_hip_ltm_cert_supported. */
#define SLA_HIP_LTM_CERT_C 64.0
#define SLA_HIP_LTM_CERT_SAFETY_MIN 16.0
#define SLA_HIP_FAST_TWIDDLE_DOUBLES(fft_size) (6u * (size_t)(fft_size))      /* (an upper bound: the sizes below fft_size / 2 add up to less) */
int    sla_hip_ltm_cert_supported(uint32_t fft_size);
double sla_hip_ltm_cert_eps_rel(uint32_t fft_size, double safety);
int    sla_hip_ltm_fast_twiddles(uint32_t fft_size, double* out);
int sla_hip_launch_ltm_cert_x(const int32_t* d_residual, uint64_t plane_stride, const sla_hip_acf_job* d_acf_jobs,
                              const sla_hip_lpc_group* d_groups, uint32_t num_jobs, uint32_t fft_size,
                              const double* d_twiddles, const double* d_fast_twiddles, double* d_scratch, uint32_t scratch_slots,
                              double* d_acf_records, double* d_eps, uint32_t longterm_order, double safety,
                              sla_hip_tail_job* d_jobs, uint32_t* d_list, uint32_t* d_counters,
                              sla_hip_stream_t stream, const sla_hip_launch_extra* extra);
/* With tuning ltm_int = 1 the autocorrelation of the certified route comes from k_ltm_acf_int instead: every sample split
 * into balanced base-256 digits, the lags 0 .. 263 as int8 matrix products (v_mfma_i32_16x16x64_i8) summed exactly in
 * integers and rounded to double once -- its own error is at most half an ulp, eps is unchanged (it still covers the
 * reference's error).  sla_hip_launch_ltm_acf_int runs that kernel without the pick and stores the sums themselves:
 * d_out[job * 264 + k] = 2^-62 * fft_size / 2 * sum_m x[m] x[m + k], k = 0 .. 263 (exact where |sum| < 2^53). */
#define SLA_HIP_ACF_INT_LAGS 264u
int sla_hip_launch_ltm_acf_int(const int32_t* d_residual, uint64_t plane_stride, const sla_hip_acf_job* d_acf_jobs,
                               uint32_t num_jobs, uint32_t fft_size, double* d_out, sla_hip_stream_t stream);

/* Long-term filter + sign-log LMS + folded-residual sum, one lane per job.
 * d_res_in/d_res_out are channel planes with the same stride as the PCM. */
int sla_hip_launch_tail(const int32_t* d_res_in, int32_t* d_res_out, uint64_t plane_stride,
                        const sla_hip_tail_job* d_jobs, uint32_t num_jobs, uint32_t longterm_order,
                        uint32_t lms_order, uint64_t* d_fold_sum, sla_hip_stream_t stream);
int sla_hip_launch_tail_x(const int32_t* d_res_in, int32_t* d_res_out, uint64_t plane_stride,
                        const sla_hip_tail_job* d_jobs, uint32_t num_jobs, uint32_t longterm_order,
                        uint32_t lms_order, uint64_t* d_fold_sum, sla_hip_stream_t stream, const sla_hip_launch_extra* extra);

/* Rice code lengths: per job the log2 of both adaptive moduli for every sample (d_kk, same plane layout
 * as the residual, uint16: k0 | k1 << 8) and the channel's total body bits (d_chan_bits[job]).
 * replaces the parameter walk of SLACoder_PutDataArray (src/SLACoder.c:224-270, 429-467). */
int sla_hip_launch_rice_len(const int32_t* d_residual, uint64_t plane_stride, const sla_hip_rice_job* d_jobs,
                            uint32_t num_jobs, uint16_t* d_kk, uint64_t* d_chan_bits, sla_hip_stream_t stream);

/* Block assembly into a zero-initialised .sla image (32-bit words, 4-byte aligned at file offset 0):
 * pre-packed header bytes, channel-interleaved Rice/Golomb/gamma or RAW bodies, then CRC16 + size patch.
 * replaces src/SLAEncoder.c:740-798 and src/SLACoder.c:45-82,120-138,429-467. */
int sla_hip_launch_rice_write(const int32_t* d_residual, const int32_t* d_pcm, uint64_t plane_stride,
                              const uint16_t* d_kk, const sla_hip_pack_block* d_blocks, uint32_t num_blocks,
                              const uint8_t* d_headers, uint32_t num_channels, uint32_t raw_shift,
                              uint32_t mid_side, uint32_t* d_image, sla_hip_stream_t stream);

/* int16 -> left-justified int32 (<< 16); d_in must be 8-byte aligned.  Used by the host-PCM path of
 * SLAEncoder_EncodeWhole to halve the PCIe bytes of <= 16-bit input. */
int sla_hip_launch_unpack16(const int16_t* d_in, int32_t* d_out, uint64_t count, sla_hip_stream_t stream);
/* the same for <= 24 significant bits carried as three bytes per sample (little-endian, the int32's upper three bytes) */
int sla_hip_launch_unpack24(const uint8_t* d_in, int32_t* d_out, uint64_t count, sla_hip_stream_t stream);

/* ---- decode side (kernels in sla_decode.hip, driver: SLADecoder.h) -----------------
 * The stream image is the .sla file's bytes in device memory (hipMalloc alignment, viewed as 32-bit words).
 * The host walks the block chain (sync code, size field, sample count: 10 bytes per block) into a table of
 * sla_hip_dec_block; everything behind those fields is parsed on the device.  All stages work in place on
 * one set of channel planes [C][plane_stride] int32:
 *   dec_bits    : block header fields + entropy decode (src/SLADecoder.c:355-412, 440-481; src/SLACoder.c:84-163,
 *                 272-318, 406-427, 469-506) -> right-justified residual / raw samples / zeros; per block
 *                 sla_hip_dec_info, per (block, channel) sla_hip_dec_chan and the PARCOR coefficients
 *                 d_kint[(block * C + ch) * (order + 1) + m]; with want_crc also the CRC16 of every block
 *   dec_lms     : SLALMSFilter_SynthesizeInt32              src/SLAPredictor.c:1334-1463
 *   dec_ltm     : SLALongTermSynthesizer_SynthesizeInt32    src/SLAPredictor.c:1034-1119
 *   dec_lattice : SLALPCSynthesizer_SynthesizeByParcorCoefInt32 src/SLAPredictor.c:610-740
 *                 + SLAEmphasisFilter_DeEmphasisInt32       src/SLAPredictor.c:1768-1791 (deemphasis != 0)
 *   dec_finish  : SLAUtility_MStoLRInt32 src/SLAUtility.c:415-433 + left-justification src/SLADecoder.c:540-547
 * The synthesis kernels skip blocks whose decoded type is not "compressed". */
#define SLA_HIP_DEC_HEADER_ONLY 1u       /* sla_hip_dec_block.flags: parse the header (and CRC), decode no samples */
typedef struct sla_hip_dec_block {
  uint64_t byte_off;        /* offset of the block's sync code in the image */
  uint32_t byte_len;        /* size field + 6, clipped to the end of the stream (CRC16 covers [8, byte_len)) */
  uint32_t smp_off;         /* first sample of the block in the planes */
  uint32_t num_samples;     /* samples per channel, from the block header */
  uint32_t flags;
} sla_hip_dec_block;
typedef struct sla_hip_dec_info {
  uint32_t type;            /* 0 compressed, 1 silent, 2 raw, 3 not a block type */
  uint32_t used_bytes;      /* bytes from the sync code to the byte-aligned end of what the reader consumed */
  uint32_t crc;             /* CRC16-IBM of [8, byte_len) when requested */
  uint32_t overrun;         /* 1: the reader ran off the end of the stream */
} sla_hip_dec_info;
typedef struct sla_hip_dec_chan {
  uint32_t pitch;           /* 0: no long-term stage */
  int32_t  ltm_coef[5];     /* Q31 */
  uint32_t rice_init;
  uint32_t reserved;
} sla_hip_dec_chan;
int sla_hip_launch_dec_bits(const uint32_t* d_image, uint64_t image_bytes,
                            const sla_hip_dec_block* d_blocks, uint32_t num_blocks,
                            uint32_t num_channels, uint32_t bits_per_sample, uint32_t offset_lshift,
                            uint32_t mid_side, uint32_t parcor_order, uint32_t longterm_order,
                            uint32_t want_crc, int32_t* d_planes, uint64_t plane_stride,
                            sla_hip_dec_info* d_info, sla_hip_dec_chan* d_chan, int32_t* d_kint,
                            sla_hip_stream_t stream);
/* dec_bits over blocks of several files concatenated in one image: d_block_end[b] (device, one per block) is the byte
 * end of block b's file in the image, and the block's reader treats it as the end of the stream -- zeros past it, the
 * same give-up limit -- so that it decodes exactly as its file would on its own.  NULL: every block is bounded by
 * image_bytes (sla_hip_launch_dec_bits).
 * The launch gives every wave `lanes` blocks, a number it takes from the size of the launch alone:
 *   lanes = ceil(num_blocks / 1024), at least 1, at most 64 / num_channels
 * (one block per wave up to 1024 blocks: every SIMD of the chip gets a wave before a wave takes a second block;
 * lanes * num_channels <= 64 rows of LDS staging).  sla_hip_dec_bits_lanes is that rule, a pure host function. */
uint32_t sla_hip_dec_bits_lanes(uint32_t num_blocks, uint32_t num_channels);
int sla_hip_launch_dec_bits_x(const uint32_t* d_image, uint64_t image_bytes,
                              const sla_hip_dec_block* d_blocks, uint32_t num_blocks,
                              uint32_t num_channels, uint32_t bits_per_sample, uint32_t offset_lshift,
                              uint32_t mid_side, uint32_t parcor_order, uint32_t longterm_order,
                              uint32_t want_crc, int32_t* d_planes, uint64_t plane_stride,
                              sla_hip_dec_info* d_info, sla_hip_dec_chan* d_chan, int32_t* d_kint,
                              sla_hip_stream_t stream, const uint64_t* d_block_end);
int sla_hip_launch_dec_lms(int32_t* d_planes, uint64_t plane_stride, const sla_hip_dec_block* d_blocks,
                           const sla_hip_dec_info* d_info, uint32_t num_blocks, uint32_t num_channels,
                           uint32_t lms_order, sla_hip_stream_t stream);
/* dec_ltm: one 64-lane workgroup per (block, channel), in place on [smp_off, smp_off + num_samples); only
 * [pitch + longterm_order / 2, num_samples) of compressed blocks with a pitch is written.  Which kernel runs is decided by
 * max_block_samples (>= the longest block of the table) alone:
 *   max_block_samples * 4 <= SLA_HIP_LDS_BUDGET (40 896 samples)  the whole block staged in that much dynamic LDS;
 *   above                                                           the block slides through a fixed 16 KiB ring of LDS in
 *                                                                   chunks of sla_hip_dec_ltm_window() samples (a pure host
 *                                                                   function), any block length the 16-bit field can hold.
 * Both compute the same samples, taps at or past the current sample (pitch 1 or 2 with 3 to 5 taps) reading input that is
 * not yet synthesised; the ring kernel leaves a channel whose pitch exceeds the format's 10 bits (1023) untouched. */
uint32_t sla_hip_dec_ltm_window(void);
int sla_hip_launch_dec_ltm(int32_t* d_planes, uint64_t plane_stride, const sla_hip_dec_block* d_blocks,
                           const sla_hip_dec_info* d_info, const sla_hip_dec_chan* d_chan,
                           uint32_t num_blocks, uint32_t num_channels, uint32_t longterm_order,
                           uint32_t max_block_samples, sla_hip_stream_t stream);
int sla_hip_launch_dec_lattice(int32_t* d_planes, uint64_t plane_stride, const sla_hip_dec_block* d_blocks,
                               const sla_hip_dec_info* d_info, uint32_t num_blocks, uint32_t num_channels,
                               const int32_t* d_kint, uint32_t parcor_order, uint32_t deemphasis, sla_hip_stream_t stream);
/* de-emphasis alone (per-call API): in place, y[-1] = previous */
int sla_hip_launch_dec_deemphasis(int32_t* d_data, uint32_t num_samples, int32_t previous, uint32_t coef_shift,
                                  sla_hip_stream_t stream);
int sla_hip_launch_dec_finish(int32_t* d_planes, uint64_t plane_stride, uint32_t num_channels,
                              uint32_t num_samples, uint32_t mid_side, uint32_t shift, sla_hip_stream_t stream);
/* dec_finish for the files of a batch pass, out of place: file f's region of the planes starts at plane_off, and its
 * num_samples finished samples per channel go to d_out[out_off + ch * num_samples + i] (packed [file][ch][n]).
 * max_samples: the largest num_samples of the table (sizes the grid). */
typedef struct sla_hip_dec_file {
  uint64_t plane_off;       /* first sample of the file's region in every plane */
  uint64_t out_off;         /* first element of the file's [C][num_samples] block in d_out */
  uint32_t num_samples;     /* samples per channel to finish */
  uint32_t mid_side;        /* 1: planes 0 / 1 are mid / side (two channels only) */
  uint32_t shift;           /* left shift of the left-justification: 32 - bits_per_sample + offset_lshift */
  uint32_t reserved;
} sla_hip_dec_file;
int sla_hip_launch_dec_finish_batch(const int32_t* d_planes, uint64_t plane_stride, uint32_t num_channels,
                                    const sla_hip_dec_file* d_files, uint32_t num_files, uint32_t max_samples,
                                    int32_t* d_out, sla_hip_stream_t stream);

/* Many .sla files decoded in one call, the decode-side counterpart of sla_hip_encode_batch.  Every item gets exactly
 * what SLADecoder_DecodeWhole of that file alone on this handle would give: result, output_num_samples and the samples
 * (those before a failing block included).  Files are grouped by the header fields the kernels are launched with
 * (channels, bits, mid/side, PARCOR / long-term / LMS order, offset_lshift); a group goes through the kernels in passes
 * of at most SLA_HIP_DEC_BATCH_PASS sample-channels (a single larger file is a pass of its own), each pass with one
 * upload of the images, one of the block table, one launch per kernel and one download of the samples.  A file whose
 * block body does not end where its size field says (the reference then resyncs where its reader stopped) is decoded
 * again on its own.  Afterwards the handle's wave format and encode parameter are those DecodeWhole of the items, in
 * order, would have left; sla_hip_decoder_last_timing holds the batch's split, [5] = the number of passes.
 * Returns 0 when the batch ran, SLA_APIRESULT_INVALID_ARGUMENT for a NULL decoder or NULL items with num_items > 0. */
#define SLA_HIP_DEC_BATCH_PASS (1u << 28)
struct SLADecoder;
typedef struct sla_hip_decode_item {
  const uint8_t* data;            /* in : a whole .sla stream (header + blocks) */
  uint32_t data_size;             /* in  */
  uint32_t buffer_num_samples;    /* in : capacity of every buffer[ch] */
  int32_t** buffer;               /* in : one plane per channel of this file, receives left-justified PCM */
  uint32_t output_num_samples;    /* out */
  int32_t  result;                /* out: SLAApiResult */
} sla_hip_decode_item;            /* 32 bytes */
int sla_hip_decode_batch(struct SLADecoder* decoder, sla_hip_decode_item* items, uint32_t num_items);

/* Many .sla files in host memory decoded into caller-owned DEVICE memory, in the sample format a tensor consumer wants.
 * The decode is sla_hip_decode_batch's (same header pass, walk, grouping and passes): every item gets the result and
 * output_num_samples that sla_hip_decode_batch gives the same file with buffer_num_samples = capacity, and its samples
 * [0, output_num_samples) are that call's, converted as sample_format says.  Instead of a download, a kernel
 * (sla_hip_launch_dec_emit_batch) writes every file's samples straight from the decode planes to its destination:
 * sample i of channel c goes to element c * channel_stride + i * sample_stride of dst.  Nothing outside that region
 * ([0, C) x [0, capacity), C from the file's header) is written; without SLA_HIP_DEC_ZERO_FILL nothing past
 * output_num_samples either, with it every channel's [output_num_samples, capacity) is written zero for every item
 * whose header gave a channel count, failed items included.
 * Per item, before any device work on it, INVALID_ARGUMENT (and nothing written) for: NULL data or dst,
 * sample_stride == 0, channel_stride == 0 on a file of more than one channel, dst not aligned to the element size, a
 * region whose byte extent overflows, a dst that is not device memory, a region outside dst's allocation.
 * The handle's stream waits on an event recorded on `stream` (NULL: the null stream) before the first write; the call
 * returns when every write has completed.  Overlapping destinations are undefined.  sla_hip_decoder_last_timing holds
 * sla_hip_decode_batch's split with [3] = the emit / zero-fill stage.
 * Returns 0 when the batch ran; INVALID_ARGUMENT for a NULL decoder, NULL items with num_items > 0, an unknown format
 * or unknown flag bits (then no item is touched). */
#define SLA_HIP_PCM_S32_LEFT  0u   /* int32, left-justified: exactly what sla_hip_decode_batch writes */
#define SLA_HIP_PCM_S32       1u   /* int32, the sample as a bit_per_sample-bit integer: left >> (32 - bps) */
#define SLA_HIP_PCM_S16       2u   /* int16: left >> 16 (arithmetic; exact for files of <= 16 bits) */
#define SLA_HIP_PCM_F32       3u   /* float: (float)left * 2^-31, int -> float rounded to nearest even */
#define SLA_HIP_DEC_ZERO_FILL 1u   /* flag: also write zeros to [output_num_samples, capacity) of each channel */
typedef struct sla_hip_decode_device_item {
  const uint8_t* data;            /* in : a whole .sla stream in host memory */
  void*    dst;                   /* in : device memory */
  uint64_t channel_stride;        /* in : elements */
  uint64_t sample_stride;         /* in : elements (>= 1) */
  uint32_t data_size;             /* in  */
  uint32_t capacity;              /* in : samples per channel (buffer_num_samples of sla_hip_decode_batch) */
  uint32_t output_num_samples;    /* out */
  int32_t  result;                /* out: SLAApiResult */
} sla_hip_decode_device_item;     /* 48 bytes */
int sla_hip_decode_batch_device(struct SLADecoder* decoder, sla_hip_decode_device_item* items, uint32_t num_items,
                                uint32_t sample_format, uint32_t flags, sla_hip_stream_t stream);

/* The emit kernel of sla_hip_decode_batch_device: for every file of the table, mid/side and left-justification of its
 * region of the planes (as dec_finish_batch), the conversion to sample_format and the store to its own destination;
 * [done, fill_end) of every channel is written zero in the same launch.  A file with mid_side = 0 and shift = 0 emits
 * planes that are already finished.  max_samples: the largest max(done, fill_end) of the table (sizes the grid). */
typedef struct sla_hip_dec_emit {
  uint64_t plane_off;             /* first sample of the file's region in every plane */
  uint64_t channel_stride;        /* elements of dst */
  uint64_t sample_stride;         /* elements of dst */
  void*    dst;                   /* device */
  uint32_t done;                  /* samples per channel decoded (read from the planes) */
  uint32_t fill_end;              /* [done, fill_end) is written zero; <= done: nothing */
  uint32_t num_channels;          /* of the file; <= 8 unless done == 0 */
  uint32_t mid_side;              /* 1: planes 0 / 1 are mid / side (two channels only) */
  uint32_t shift;                 /* left shift of the left-justification: 32 - bits_per_sample + offset_lshift */
  uint32_t bits_per_sample;       /* SLA_HIP_PCM_S32 shifts the left-justified sample right by 32 - bits_per_sample */
} sla_hip_dec_emit;               /* 56 bytes */
int sla_hip_launch_dec_emit_batch(const int32_t* d_planes, uint64_t plane_stride, const sla_hip_dec_emit* d_files,
                                  uint32_t num_files, uint32_t max_samples, uint32_t sample_format, sla_hip_stream_t stream);

/* Many .sla files whose BYTES ARE IN DEVICE MEMORY decoded into caller-owned device memory: sla_hip_decode_batch_device
 * without a host copy of the streams, without staging and without an upload.  The item struct is that call's and `data`
 * is a device pointer (any byte alignment: slices of one big uint8 buffer are fine); sources are only read.
 * Every item gets exactly what sla_hip_decode_batch_device on this handle gives for the same bytes in host memory: result,
 * output_num_samples, the contents of dst in every format, the zero fill, nothing written outside [0, C) x [0, capacity),
 * the handle's wave format and encode parameter afterwards, the call-level refusals.
 * Per item, on the host and before anything of the item is read or written, INVALID_ARGUMENT (nothing written) also
 * for: NULL data, a data the runtime does not report as device memory, a [data, data + data_size) that does not lie
 * inside its allocation.  The destination checks need the header's channel count: they run once the headers are home
 * and before anything is written to dst.
 * How it runs: (a) a gather kernel (sla_hip_launch_dec_gather) collects the first min(data_size, 43) bytes of every
 * admissible item, one copy brings them home and the header pass of sla_hip_decode_batch runs on that copy; (b) a walk
 * kernel (sla_hip_launch_dec_walk, count mode) follows every file's block chain on the device and returns its block
 * count, stop reason and extent, from which the host cuts the passes as ever; (c) per pass the gather copies the files
 * into the handle's pass image at their 4-byte offsets, the walk in write mode fills the block table, every block's end
 * of stream and stored CRC field, and the decode kernels run unchanged; (d) table, CRC fields and block infos come home
 * in the pass's one wait and are examined with the host call's code; a file that needs a resync is copied to the host
 * and decoded again on its own.  A single long file walks its blocks serially on one lane, about 0.7 us per block and
 * walk on an MI355X (two walks: 10 ms of the 16 ms a ten-minute file takes; 125 ten-second clips: 0.4 ms of 9.3 ms;
 * DESIGN section 4b).  For such a file there is a second walker, sla_hip_launch_dec_walk_wide below: with the handle
 * option "wide_walk" (sla_hip_decoder_set_option, include/SLADecoder.h; default 16 000 000 bytes) the call sends the streams of at
 * least that many bytes, at most the 8 longest, through it in both modes -- the lane launch carries them with total = 0
 * and writes their empty result and rows, the wide launches behind it overwrite both -- and a count whose nodes overflow
 * the capacity is repeated on a lane.  Results, codes and samples are the same; sla_hip_decoder_last_walk counts the route.
 * The handle's stream waits on an event recorded on `stream` before the first read of any source and before the first
 * write; the call returns when every write has completed and no kernel reads a source any more.
 * sla_hip_decoder_last_timing: [0] = the gathers, [1] = the walks (kernels and their copies), the rest as for
 * sla_hip_decode_batch_device. */
int sla_hip_decode_batch_resident(struct SLADecoder* decoder, sla_hip_decode_device_item* items, uint32_t num_items,
                                  uint32_t sample_format, uint32_t flags, sla_hip_stream_t stream);

/* The headers of `num` resident streams (d_data[i]: device pointer, data_size[i] bytes), for a caller that shapes its
 * destinations from them: results[i] is SLADecoder_DecodeHeader's code on item i's first bytes and headers[i] what it
 * delivered (zero when nothing), INVALID_ARGUMENT for a source sla_hip_decode_batch_resident would refuse.  One gather,
 * one copy home, ordered behind `stream` as above.  The handle's wave format and encode parameter are left alone.
 * INVALID_ARGUMENT for a NULL decoder, or NULL arrays with num > 0. */
int sla_hip_resident_headers(struct SLADecoder* decoder, const uint8_t* const* d_data, const uint32_t* data_size,
                             uint32_t num, struct SLAHeaderInfo* headers, int32_t* results, sla_hip_stream_t stream);

/* The block-chain walk on the device: the host's walk of whole files (from byte 43, sample 0) restated one file per
 * lane -- same checks, same order, same 32-bit arithmetic, the wrap of `size field + 6` included.  A block whose sample
 * count exceeds capacity - pos or max_block_samples ends the walk; with crc_check 1 it is kept, flagged
 * SLA_HIP_DEC_HEADER_ONLY, with crc_check 0 it is not.  d_results[f].stop is the SLAApiResult that says why the walk
 * stopped short of `total` samples (OK when it did not), extent the highest smp_off + num_samples over the blocks that
 * are not header-only (positions in the file).
 * Count mode (d_blocks NULL): only d_results is written.  Write mode (d_blocks, d_block_end and d_crc_field all given):
 * file f's rows go to [first, first + max_rows) of the three tables -- sla_hip_dec_block with byte_off + img_off and
 * smp_off + plane_off, img_off + data_size, and the big-endian 16-bit field at byte 6 of the block -- and never at or
 * behind first + max_rows, which the caller sets to the count of a count-mode walk.  Should a file yield fewer rows
 * than max_rows (its bytes changed in between) the rest become empty header-only rows at the file's start, so that no
 * row of the range is left as it was; d_results tells.
 * The walk reads bytes, at any alignment, and none outside [src, src + data_size).  One dependent load per block: a
 * file of tens of thousands of blocks walks them serially.
 * INVALID_ARGUMENT before any launch for a NULL file table or result table, or for write mode with a table missing. */
typedef struct sla_hip_dec_walk_file {
  const uint8_t* src;             /* device: the whole .sla stream */
  uint64_t img_off;               /* write mode: the file's offset in the pass image */
  uint32_t data_size;
  uint32_t total;                 /* the header's num_samples */
  uint32_t capacity;              /* samples per channel of the destination */
  uint32_t first;                 /* write mode: the file's first row */
  uint32_t max_rows;              /* write mode: its rows */
  uint32_t plane_off;             /* write mode: the file's first sample in the pass planes */
} sla_hip_dec_walk_file;          /* 40 bytes */
typedef struct sla_hip_dec_walk_result {
  uint32_t num_blocks;            /* rows the walk kept */
  uint32_t stop;                  /* SLAApiResult */
  uint32_t extent;                /* samples per channel the kept blocks write */
  uint32_t reserved;
} sla_hip_dec_walk_result;        /* 16 bytes */
int sla_hip_launch_dec_walk(const sla_hip_dec_walk_file* d_files, uint32_t num_files, uint32_t max_block_samples,
                            uint32_t crc_check, sla_hip_dec_walk_result* d_results, sla_hip_dec_block* d_blocks,
                            uint64_t* d_block_end, uint32_t* d_crc_field, sla_hip_stream_t stream);

/* The wide walk: the same table for ONE file, built by the whole device instead of one lane -- for the long file whose
 * thousands of blocks sla_hip_launch_dec_walk follows one dependent load at a time.  `file` is a HOST struct (its src a
 * device pointer); d_result[0] and the rows [first, first + max_rows) of the three tables are byte for byte what
 * sla_hip_launch_dec_walk writes for the same file, max_block_samples and crc_check, in count mode (all three tables
 * NULL) and in write mode: num_blocks, stop, extent, reserved 0, img_off / plane_off, the header-only row of a block
 * that fails the capacity test under crc_check 1, the empty header-only rows of rows not reached, nothing at or behind
 * first + max_rows.
 * How: every byte position is tested on its own for "a block could start here" (a NODE: 43 <= p, p + 11 <= data_size,
 * FF FF at p, 8 <= size field + 6 mod 2^32 <= data_size - p); the nodes are numbered by a scan, each gets its successor
 * (the node at p + size field + 6, strictly ahead, or none), and the path from byte 43 is ranked by pointer doubling
 * in sla_hip_dec_wide_rounds(data_size, node_capacity) launches -- about log2 of the block count -- before a last
 * kernel cuts the ranked path where the lane walk would stop and writes the rows in rank order.  Sample positions are
 * 64-bit sums.  Launches on `stream` are the only ordering: no kernel waits for another workgroup, the launcher issues
 * no memset and no synchronisation, and every loop runs a count known on entry.
 * Reads are byte-exact in effect: wide loads touch only the aligned 16-byte words that overlap [src, src + data_size).
 * OVERFLOW: a stream with more nodes than node_capacity yields {0, OK, 0, SLA_HIP_DEC_WIDE_OVERFLOW} and, in write
 * mode, max_rows empty header-only rows; the caller walks that file on a lane.  The node count is exact beyond the
 * capacity: once the launches have completed, the first 16 bytes of d_scratch are a sla_hip_dec_wide_info.
 * d_scratch: SLA_HIP_DEC_WIDE_SCRATCH_BYTES(data_size, node_capacity) bytes, 16-byte aligned, contents arbitrary; it
 * may be reused by the next launch on the same stream.  A file with total == 0 or data_size < 54 launches one kernel.
 * INVALID_ARGUMENT before any launch for a NULL file, result or scratch, node_capacity 0, write mode with a table
 * missing, a scratch that is not 16-byte aligned, or a NULL src of a file that has to be read. */
#define SLA_HIP_DEC_WIDE_OVERFLOW 1u     /* sla_hip_dec_walk_result.reserved */
#define SLA_HIP_DEC_WIDE_TILES(data_size) ((((uint64_t)(data_size) + 46u) / 32u + 255u) / 256u)   /* tiles of 256 32-byte words */
#define SLA_HIP_DEC_WIDE_SCRATCH_BYTES(data_size, node_capacity) \
  (64u + SLA_HIP_DEC_WIDE_TILES(data_size) * 2048u + ((SLA_HIP_DEC_WIDE_TILES(data_size) * 4u + 15u) & ~(uint64_t)15) \
   + (((uint64_t)(node_capacity) + 3u) & ~(uint64_t)3) * 64u)
typedef struct sla_hip_dec_wide_info {
  uint32_t nodes;                 /* nodes of the stream, exact also above node_capacity */
  uint32_t path_len;              /* nodes on the path from byte 43 (0 after an overflow) */
  uint32_t cut;                   /* 0xFFFFFFFF: the whole path is kept; else rank * 2 + (1: a capacity stop) of the cut */
  uint32_t reserved;
} sla_hip_dec_wide_info;          /* 16 bytes */
int sla_hip_launch_dec_walk_wide(const sla_hip_dec_walk_file* file, uint32_t max_block_samples, uint32_t crc_check,
                                 sla_hip_dec_walk_result* d_result, sla_hip_dec_block* d_blocks, uint64_t* d_block_end,
                                 uint32_t* d_crc_field, uint32_t node_capacity, void* d_scratch, sla_hip_stream_t stream);
uint64_t sla_hip_dec_wide_scratch_bytes(uint32_t data_size, uint32_t node_capacity);   /* the macro, for callers without it */
uint32_t sla_hip_dec_wide_rounds(uint32_t data_size, uint32_t node_capacity);          /* doubling rounds a launch issues */

/* Decode THROUGH damage: one resident .sla stream salvaged on the device.  Every other decode call stops at the first block
 * that fails, as the reference does; this one delivers all N samples of the header, each either decoded or zero, and says
 * which ranges are silence and why.  It can, because every block resets its filters and its coder and carries a CRC16 over
 * its own bytes.  Nothing that the other calls return changes.
 *
 * THE RULE (executable: tests/salvagemodel.py).  S = data_size; N, C from the header.
 *   NODE         the wide walk's: 43 <= p, p + 11 <= S, FF FF at p, 8 <= size field + 6 (mod 2^32) <= S - p.
 *   SOUND BLOCK  a node whose sample count n (bytes p + 8..9) is <= the handle's max_num_block_samples, whose byte length
 *                is <= SLA_HIP_SALVAGE_MAX_BLOCK_BYTES(C, n) = 64 + 16 C max(n, 1) -- four times a RAW block of 32-bit
 *                samples: no block an encoder writes is longer, and the cap bounds the CRC work that the size field of
 *                a decoy (FF FF in a payload) can cause -- and whose CRC16 over [p + 8, p + length) equals the field at
 *                p + 6.  Soundness is always judged with the CRC, whatever the handle's enable_crc_check says.
 *   MODE 1, chain intact: the plain walk from byte 43 with capacity N stops with OK and extent N.  Every block of the
 *                chain keeps its position.  A block whose stored CRC differs is not entropy-decoded at all (its row is
 *                SLA_HIP_DEC_HEADER_ONLY) and becomes n samples of silence, reason CRC; a block whose CRC holds and whose
 *                decode fails by the whole-file decode's criteria -- type > 2, reader overrun, a body that does not end
 *                where the size field says -- becomes silence, reason UNDECODABLE.  Decoding goes on at the next block of
 *                the chain: there is no resync from where a reader stopped.
 *   MODE 2, chain broken (everything else): two anchored pieces are delivered, what lies between them is lost.
 *                PREFIX: from byte 43, sample 0, sound blocks while one starts exactly where the one before ended and
 *                s + n <= N; it ends at byte p0, sample s0.  SUFFIX: over links from a sound block to the sound block
 *                that starts exactly at its end, the smallest sound q >= p0 whose chain ends exactly at byte S with a
 *                sample sum T <= N - s0; it is placed at sample N - T.  [s0, N - T) is one range of silence, reason GAP
 *                ([s0, N) when no q qualifies).  Prefix and suffix blocks that then fail in the decoder are concealed as
 *                in mode 1.
 * The chain is trusted for positions (mode 1) only when it accounts for exactly N samples: sample counts and size fields
 * are chain data, and a damaged one that still leads somewhere would shift everything behind it.
 * ACCEPTED LIMITS.  A second break in the middle loses the sound blocks between the two breaks.  Bytes appended behind
 * the last block defeat the right anchor (no suffix).  A CRC16 passes a decoy with probability 2^-16.  A complete valid
 * block embedded in another block's payload and chained to the end can be picked as q when the block around it is not
 * sound: its samples are then delivered, right-aligned with the suffix.
 *
 * THE CALL.  d_data / data_size: the stream in device memory, any alignment, only read.  dst, channel_stride,
 * sample_stride, capacity, sample_format: as an item of sla_hip_decode_batch_resident, and so are the source and
 * destination checks (INVALID_ARGUMENT, nothing read or written), the header's failures and format verdicts (that call's
 * code and nothing else; a file of no samples is OK) and the ordering behind `stream`; the handle's wave format and encode
 * parameter become the stream's.  An LMS order the kernels do not run is refused whole: FAILED_TO_SYNTHESIZE, nothing
 * written.  capacity < N: INSUFFICIENT_BUFFER_SIZE, nothing written.  Otherwise exactly [0, C) x [0, N) is written, and
 * nothing outside it.  Returns OK when nothing was concealed or lost -- dst then equals sla_hip_decode_batch_resident's
 * bit for bit -- and DETECT_DATA_CORRUPTION when something was; the data is delivered either way.  NG: a device failure.
 * INVALID_ARGUMENT before anything else for a NULL decoder, d_data, dst or report, an unknown format, or NULL ranges
 * with range_capacity > 0.
 * report: see the struct.  ranges: the first min(num_ranges, range_capacity) silent ranges in ascending order, one per
 * concealed block that has samples and one for the gap; num_ranges is exact beyond the capacity.
 * How it runs: header gather; the lane walk in count mode (the wide walk from the handle's "wide_walk" size on) decides the
 * mode.  Mode 1: gather, walk in write mode, k_salvage_crc flags the rows whose CRC differs.  Mode 2: the salvage scan
 * below in count mode (repeated once with the exact capacity when the nodes overflow the handle's), the gather, the scan
 * in write mode.  Then the decode kernels unchanged; the infos come home in that wait, the list of silent regions goes up,
 * k_dec_conceal zeroes them in the planes (zero planes stay zero through mid/side and shift) and the emit kernel writes
 * dst.  No byte of the stream behind its header is copied to the host.
 * sla_hip_decoder_last_timing: [0] the gathers, [1] the count walk and the count-mode scan, [2] the decode kernels, [3]
 * conceal and emit, [4] the call.  sla_hip_decoder_last_walk: the count walk's figures and, in mode 2, one more walk, the
 * scan's nodes and two sets of doubling rounds per scan; [1] counts a scan whose nodes overflowed. */
#define SLA_HIP_SALVAGE_MAX_BLOCK_BYTES(C, n) (64u + 16u * (uint32_t)(C) * (((uint32_t)(n) > 1u) ? (uint32_t)(n) : 1u))
#define SLA_HIP_SALVAGE_CRC         1u    /* sla_hip_salvage_range.reason: the block's stored CRC differs */
#define SLA_HIP_SALVAGE_UNDECODABLE 2u    /* the CRC holds, the decoder failed on the block */
#define SLA_HIP_SALVAGE_GAP         3u    /* mode 2: between prefix and suffix */
typedef struct sla_hip_salvage_report {
  uint32_t mode;                  /* 0: nothing decoded (refused, or no samples), 1: chain intact, 2: chain broken */
  uint32_t blocks_decoded;
  uint32_t blocks_concealed;
  uint32_t samples_lost;          /* per channel: the sum of the ranges' lengths */
  uint32_t num_ranges;            /* exact, also beyond range_capacity */
  uint32_t prefix_blocks;         /* mode 2 from here on; 0 in mode 1 */
  uint32_t suffix_blocks;
  uint32_t suffix_byte;           /* q; 0: no suffix */
  uint32_t suffix_sample;         /* N - T; 0 without a suffix */
  uint32_t nodes;
  uint32_t sound_nodes;
  uint32_t reserved;
} sla_hip_salvage_report;         /* 48 bytes */
typedef struct sla_hip_salvage_range {
  uint32_t start;                 /* first sample */
  uint32_t length;
  uint32_t reason;                /* SLA_HIP_SALVAGE_* */
} sla_hip_salvage_range;          /* 12 bytes */
struct SLADecoder;
int sla_hip_salvage_resident(struct SLADecoder* decoder, const uint8_t* d_data, uint32_t data_size,
                             void* dst, uint64_t channel_stride, uint64_t sample_stride, uint32_t capacity,
                             uint32_t sample_format, sla_hip_salvage_report* report,
                             sla_hip_salvage_range* ranges, uint32_t range_capacity, sla_hip_stream_t stream);

/* The salvage scan: mode 2 of the rule above for ONE stream, by the whole device.  `file` is a HOST struct as for
 * sla_hip_launch_dec_walk_wide (src, data_size, total = N; capacity is not read; write mode: img_off, first, max_rows,
 * plane_off).  d_result[0] receives the prefix, the suffix and the counts.  Count mode (all three tables NULL) writes
 * nothing else; write mode puts the prefix rows and behind them the suffix rows -- flags 0, smp_off the block's sample
 * position + plane_off, the suffix at N - T -- into rows [first, first + max_rows) of the three tables as
 * sla_hip_launch_dec_walk does, rows behind the last block become empty header-only rows, and nothing is written at or
 * behind first + max_rows, which the caller sets to prefix_blocks + suffix_blocks of a count-mode scan.
 * How: the node bitmap, scan and numbering of the wide walk; one wave per node judges soundness (the n test and the
 * length cap first, then the CRC16 of the block by crc16_wave); sound-successor links are doubled to the END in
 * sla_hip_dec_wide_rounds(data_size, node_capacity) launches, after which every sound node knows the last node of its
 * all-sound chain, that chain's end byte and its 64-bit sample sum, and the path from byte 43 is ranked; a cut ends the
 * prefix; an atomicMin over the qualifying nodes picks q; a second set of rounds ranks q's chain; a last kernel writes the
 * rows and the result.  Launches on `stream` are the only ordering: no kernel waits for another workgroup, the launcher
 * issues no memset and no synchronisation, every loop runs a count known on entry.  Reads touch only the aligned 16-byte
 * words that overlap [src, src + data_size).
 * OVERFLOW: more nodes than node_capacity yield overflow = 1, the exact node count, every other field as for an empty
 * scan and, in write mode, empty rows only; the caller repeats with that capacity.
 * d_scratch: SLA_HIP_DEC_SALVAGE_SCRATCH_BYTES(data_size, node_capacity) bytes, 16-byte aligned, contents arbitrary,
 * reusable by the next launch on the same stream.  A stream of fewer than 54 bytes launches one kernel.
 * INVALID_ARGUMENT before any launch for a NULL file, result or scratch, node_capacity 0, num_channels 0 or > 8, write
 * mode with a table missing, a scratch that is not 16-byte aligned, or a NULL src of a file that has to be read. */
#define SLA_HIP_DEC_SALVAGE_SCRATCH_BYTES(data_size, node_capacity) \
  (SLA_HIP_DEC_WIDE_SCRATCH_BYTES(data_size, node_capacity) + 64u + (((uint64_t)(node_capacity) + 3u) & ~(uint64_t)3) * 28u)
typedef struct sla_hip_salvage_scan {
  uint32_t prefix_blocks;
  uint32_t prefix_samples;        /* s0 */
  uint32_t prefix_end;            /* p0: the byte behind the prefix, 43 when it is empty */
  uint32_t suffix_byte;           /* q; 0: no suffix */
  uint32_t suffix_samples;        /* T */
  uint32_t suffix_blocks;
  uint32_t nodes;                 /* exact, also above node_capacity */
  uint32_t sound_nodes;
  uint32_t overflow;              /* 1: nodes > node_capacity, nothing else was found */
  uint32_t reserved[3];
} sla_hip_salvage_scan;           /* 48 bytes */
int sla_hip_launch_dec_salvage_scan(const sla_hip_dec_walk_file* file, uint32_t num_channels, uint32_t max_block_samples,
                                    sla_hip_salvage_scan* d_result, sla_hip_dec_block* d_blocks, uint64_t* d_block_end,
                                    uint32_t* d_crc_field, uint32_t node_capacity, void* d_scratch, sla_hip_stream_t stream);
uint64_t sla_hip_dec_salvage_scratch_bytes(uint32_t data_size, uint32_t node_capacity);   /* the macro, for callers without it */

/* Mode 1's CRC pass over a block table in a pass image (kernel k_salvage_crc): row b gets d_bad[b] = 1 and the flag
 * SLA_HIP_DEC_HEADER_ONLY when the CRC16 of its bytes [byte_off + 8, byte_off + byte_len) of the image differs from
 * d_crc_field[b], else d_bad[b] = 0.  INVALID_ARGUMENT before any launch for a NULL pointer. */
int sla_hip_launch_salvage_crc(const uint8_t* d_image, sla_hip_dec_block* d_blocks, const uint32_t* d_crc_field,
                               uint32_t num_blocks, uint32_t* d_bad, sla_hip_stream_t stream);

/* Silence in the decode planes (kernel k_dec_conceal): samples [smp_off, smp_off + num_samples) of all num_channels planes
 * are written zero for every entry of the device list, clipped to plane_stride.  Launched before the emit kernel: zero
 * planes stay zero through mid/side and the left shift.  max_samples: the largest num_samples of the list (sizes the
 * grid).  INVALID_ARGUMENT before any launch for a NULL pointer, num_channels 0 or > 8. */
typedef struct sla_hip_dec_conceal {
  uint32_t smp_off;
  uint32_t num_samples;
} sla_hip_dec_conceal;            /* 8 bytes */
int sla_hip_launch_dec_conceal(int32_t* d_planes, uint64_t plane_stride, uint32_t num_channels,
                               const sla_hip_dec_conceal* d_list, uint32_t count, uint32_t max_samples, sla_hip_stream_t stream);

/* The byte-granular gather into an image: entry k copies `bytes` bytes from src (device, any alignment) to
 * d_image + dst_off (dst_off a multiple of 4) and writes zeros from there to the next 4-byte boundary.  Nothing outside
 * each entry's padded range is written; an entry whose dst_off is no multiple of 4 or whose padded range does not lie
 * inside [0, image_bytes) is skipped.  max_bytes: the largest `bytes` of the table (sizes the grid).
 * Loads touch only the aligned 16-byte words that overlap [src, src + bytes).
 * INVALID_ARGUMENT before any launch for a NULL table or image. */
typedef struct sla_hip_dec_gather {
  const uint8_t* src;             /* device */
  uint64_t dst_off;               /* bytes from d_image, a multiple of 4 */
  uint32_t bytes;
  uint32_t reserved;
} sla_hip_dec_gather;             /* 24 bytes */
int sla_hip_launch_dec_gather(const sla_hip_dec_gather* d_table, uint32_t num_entries, uint32_t max_bytes,
                              uint8_t* d_image, uint64_t image_bytes, sla_hip_stream_t stream);

/* The block-chain walk for a WINDOW of samples [win_start, min(win_start + win_len, total)) of each file (the end in 64
 * bits), one file per lane like sla_hip_launch_dec_walk and with its chain checks, in its order and its 32-bit
 * arithmetic: off > data_size or fewer than 11 bytes left -> INSUFFICIENT_DATA_SIZE, no sync code ->
 * FAILED_TO_FIND_SYNC_CODE, a wrapped `size field + 6` above the bytes left or below 8 -> INSUFFICIENT_DATA_SIZE.
 * The walk starts at byte 43, sample 0, or, with seek_byte != 0, at (seek_byte, seek_sample) -- the caller's promise that
 * a block starts there -- and runs while the sample position (carried in 64 bits, it never wraps) is below the window's
 * end.  A block with no samples, or one that ends at or before win_start, is PASSED OVER: counted in `skipped`, no row,
 * no further check.  Every other block is KEPT, unless its sample count exceeds max_block_samples: that stops the walk
 * with INSUFFICIENT_BUFFER_SIZE and the block is not kept (there are no header-only rows and no capacity test here: the
 * window is clipped, not the file).  Blocks behind the window are never read.
 * Result: the blocks kept and passed over, the stop code, the file position (byte, sample) of the first kept block and
 * the position behind the last one; all four positions 0 when no block was kept.
 * Write mode (d_blocks, d_block_end and d_crc_field all given; count mode: all NULL) lays the kept blocks out for a pass
 * that gathered the bytes [base_byte, base_byte + range_bytes) of the file to img_off and gave it the plane region at
 * plane_off for the samples from base_sample on: row first + k is a sla_hip_dec_block with byte_off = img_off + (off -
 * base_byte), smp_off = plane_off + (pos - base_sample), flags 0; its block end is img_off + range_bytes; its CRC field
 * the big-endian 16-bit field at byte 6 of the block.  Nothing is written at or behind first + max_rows; rows the walk
 * did not reach become empty header-only rows at img_off, as in sla_hip_launch_dec_walk.
 * The walk reads bytes, at any alignment, and none outside [src, src + data_size), whatever the hint.
 * INVALID_ARGUMENT before any launch for a NULL file table or result table, or for write mode with a table missing. */
typedef struct sla_hip_dec_window_file {
  const uint8_t* src;             /* device: the whole .sla stream */
  uint64_t img_off;               /* write mode: where the pass image holds the file's byte range */
  uint32_t data_size;
  uint32_t total;                 /* the header's num_samples */
  uint32_t win_start;             /* first sample of the window */
  uint32_t win_len;               /* its length */
  uint32_t seek_byte;             /* 0: walk from the header; else the byte of a block's sync code */
  uint32_t seek_sample;           /* the first sample of that block */
  uint32_t range_bytes;           /* write mode: bytes of the file's range in the image */
  uint32_t base_byte;             /* write mode: the file position of the range's first byte */
  uint32_t base_sample;           /* write mode: the file position of the region's first sample */
  uint32_t plane_off;             /* write mode: the file's region in the pass planes */
  uint32_t first;                 /* write mode: the file's first row */
  uint32_t max_rows;              /* write mode: its rows */
} sla_hip_dec_window_file;        /* 64 bytes */
typedef struct sla_hip_dec_window_result {
  uint32_t num_blocks;            /* blocks kept */
  uint32_t stop;                  /* SLAApiResult */
  uint32_t skipped;               /* blocks passed over */
  uint32_t first_byte;            /* file position of the first kept block */
  uint32_t first_sample;
  uint32_t end_byte;              /* file position behind the last kept block */
  uint32_t end_sample;
  uint32_t reserved;
} sla_hip_dec_window_result;      /* 32 bytes */
int sla_hip_launch_dec_walk_window(const sla_hip_dec_window_file* d_files, uint32_t num_files, uint32_t max_block_samples,
                                   sla_hip_dec_window_result* d_results, sla_hip_dec_block* d_blocks,
                                   uint64_t* d_block_end, uint32_t* d_crc_field, sla_hip_stream_t stream);

/* Windows of samples of resident .sla streams decoded into caller-owned device memory: what a pipeline that keeps its
 * compressed corpus in device memory needs for a crop.  Item i delivers the samples [start, start + length) of its stream,
 * clipped to the file: sample start + k of channel c goes to element c * channel_stride + k * sample_stride of dst.
 * Blocks reset their filters and their coder, so a window needs exactly the blocks it overlaps, and the 10-byte chain
 * headers in front of them to find where they start: only those are read, gathered and decoded.  Consequently damage in
 * a block the window does not need is NOT SEEN -- neither a flipped bit in a block in front of the window nor anything
 * behind its last block.
 * Formats, SLA_HIP_DEC_ZERO_FILL, the strides, the call-level refusals, the per-item source and destination checks (made
 * on the host before anything of the item is read or written, `length` in the part of `capacity`), the header failures
 * and format verdicts, the ordering behind `stream` and the handle's wave format and encode parameter afterwards are
 * sla_hip_decode_batch_resident's.  Per item also INVALID_ARGUMENT (nothing written) for: a seek_byte that is neither 0
 * nor at least 43, seek_byte == 0 with seek_sample != 0, seek_sample > start, and, once the header is home,
 * start > num_samples.
 * A window is delivered whole or not at all.  Result OK: output_num_samples = min(length, num_samples - start) samples
 * (none, and nothing decoded, for start == num_samples or length == 0); with the flag [output_num_samples, length) of
 * every channel is zero.  The kept blocks are examined in file order with the whole-file decode's criteria and the first
 * failure is the item's result: with enable_crc_check a CRC that differs from the stored field ->
 * DETECT_DATA_CORRUPTION, a block type above 2 -> INVALID_HEADER_FORMAT, a compressed block with an LMS order the
 * kernels do not run -> FAILED_TO_SYNTHESIZE, a body that does not end where the size field says or a reader that ran
 * off the end -> DETECT_DATA_CORRUPTION (windows do NO RESYNC: where the whole-file decode would continue from where
 * its reader stopped, the window fails); after the blocks the walk's stop code.  A failed item gets output_num_samples
 * 0; with the flag its whole [0, C) x [0, length) is zero, without it nothing of it is written.
 * The hint: seek_byte / seek_sample name a block start at or before the window (seek_byte 0: none, the walk starts at
 * the header).  first_block_byte / first_block_sample return the first kept block's position (0, 0 when the walk kept
 * none), a valid hint for any later window of the same bytes with start >= first_block_sample; a long file is served by
 * hints the caller keeps (this call takes no index object: sla_hip_decode_windows_indexed does).  A hint is the caller's
 * promise: a wrong one gives an error code or wrong samples, never a read outside the source or a write outside the
 * destination.
 * The same source may appear in any number of items; each is decoded on its own.
 * How it runs: the header gather; the window walk in count mode over all items; items grouped by launch parameters and
 * cut into passes by sla_hip_decode_batch's caps, an item costing the bytes from its first kept block to the end of its
 * last and the samples of those blocks; per pass one gather of the ranges, the window walk in write mode, the decode
 * kernels unchanged, the examination, and the emit kernel reading each region from the window's first sample.  A
 * write-mode walk that differs from the count fails the call.
 * sla_hip_decoder_last_timing keeps sla_hip_decode_batch_resident's split. */
typedef struct sla_hip_decode_window_item {
  const uint8_t* data;            /* in : a whole .sla stream in device memory, any byte alignment */
  void*    dst;                   /* in : device memory */
  uint64_t channel_stride;        /* in : elements */
  uint64_t sample_stride;         /* in : elements (>= 1) */
  uint32_t data_size;             /* in  */
  uint32_t start;                 /* in : first sample of the window */
  uint32_t length;                /* in : samples per channel of the window and of dst */
  uint32_t seek_byte;             /* in : hint, 0 for none */
  uint32_t seek_sample;           /* in : hint */
  uint32_t output_num_samples;    /* out */
  int32_t  result;                /* out: SLAApiResult */
  uint32_t first_block_byte;      /* out: a hint for later windows at or behind this one */
  uint32_t first_block_sample;    /* out */
  uint32_t reserved;
} sla_hip_decode_window_item;     /* 72 bytes */
int sla_hip_decode_windows_resident(struct SLADecoder* decoder, sla_hip_decode_window_item* items, uint32_t num_items,
                                    uint32_t sample_format, uint32_t flags, sla_hip_stream_t stream);
/* Summed over the last sla_hip_decode_windows_resident: [0] blocks passed over, [1] blocks decoded, [2] stream bytes
 * gathered, [3] plane samples per channel reserved.  INVALID_ARGUMENT for a NULL argument. */
int sla_hip_decoder_last_window_stats(const struct SLADecoder* decoder, uint64_t counters[4]);

/* ---- A block index, and windows decoded from it without a host wait ----
 * sla_hip_index is the block chain of one .sla stream, kept on the host: opaque, immutable, shareable between threads and
 * handles.  It holds the stream's data_size, its first 43 bytes (fewer for a shorter stream), what SLADecoder_DecodeHeader
 * made of them (result and SLAHeaderInfo), and -- when the header could be read (OK or DETECT_DATA_CORRUPTION) -- the chain
 * walked from byte 43 by the whole-file walk's rules (sla_hip_launch_dec_walk) with capacity = the header's num_samples,
 * NO cap on the block length (the format's 65 535) and enable_crc_check 0: rows {byte_off, byte_len, smp_off, num_samples} in
 * file positions, no header-only rows, the walk's stop code and extent.
 *   sla_hip_index_build           from host bytes; pure host code, no device.
 *   sla_hip_index_build_resident  from device bytes, on the handle's stream behind `stream`: the header gather, then the walk
 *                                 in count and in write mode; a stream of at least the handle's "wide_walk" bytes is walked
 *                                 by sla_hip_launch_dec_walk_wide, an overflow of its nodes falls back to the lane.  Waits
 *                                 for the device (it brings rows home).  INVALID_ARGUMENT for a source that is not device
 *                                 memory or not inside its allocation.
 * Both give byte-identical serialisations for the same bytes.  Return 0 and *index, INVALID_ARGUMENT for a NULL argument,
 * NG for a device or allocation failure.
 *   sla_hip_index_info            gives a sla_hip_index_summary; sla_hip_index_blocks copies rows [first, first + count)
 *                                 (INVALID_ARGUMENT when that is not inside [0, num_blocks)); sla_hip_index_destroy (NULL
 *                                 allowed).
 *   sla_hip_index_serialized_bytes / _serialize / _deserialize: a little-endian blob, so that a data set can keep a sidecar
 *   next to each file: magic "SLAX", version 1, data_size, header bytes held, header result, stop, extent, num_blocks, the 43
 *   header bytes (zero padded to 44), the rows, and in its last two bytes the library's CRC16 (slai_crc16) of everything
 *   before them.  _serialize returns the bytes written, 0 when `capacity` is too small.
 * Deserialise refuses with INVALID_ARGUMENT, and keeps no allocation, for: a wrong magic or version; a wrong checksum; a
 * truncated (or over-long) blob; rows that are not strictly ascending in bytes WITHOUT OVERLAP (a row starts at or behind the
 * end of the one before it, so that the byte range from a window's first row to the end of its last holds every row of it
 * whole) and cumulative in samples from sample 0; a row with byte_off < 43, byte_len < 11 or byte_off + byte_len > data_size;
 * num_samples > 65535; an extent that is not the end of the last row or lies above the header's total; header fields that
 * are not what DecodeHeader makes of the stored bytes.
 * After this an index can be wrong about the bytes it is used with; it can never name a range outside [0, data_size).
 * The shortest block: the builders follow the walk, which keeps a block whose size field + 6 is 8, 9 or 10 when 11 bytes are
 * left (no encoder writes one; no decoder decodes one).  An index with such a row is built, read and used like any other,
 * and serialises; its blob is one the deserialiser refuses (byte_len < 11), so it has no sidecar. */
typedef struct sla_hip_index sla_hip_index;
typedef struct sla_hip_index_block {
  uint32_t byte_off;              /* the block's sync code in the file */
  uint32_t byte_len;              /* size field + 6 */
  uint32_t smp_off;               /* its first sample in the file */
  uint32_t num_samples;
} sla_hip_index_block;            /* 16 bytes */
typedef struct sla_hip_index_summary {
  uint32_t data_size;
  uint32_t header_bytes;          /* bytes of the stream's head held: min(data_size, 43) */
  int32_t  header_result;         /* SLADecoder_DecodeHeader's SLAApiResult */
  uint32_t stop;                  /* why the walk ended: an SLAApiResult, OK when it reached the header's num_samples */
  uint32_t extent;                /* samples per channel the rows cover */
  uint32_t num_blocks;
  struct SLAHeaderInfo header;    /* zero unless header_result is OK or DETECT_DATA_CORRUPTION */
} sla_hip_index_summary;
int      sla_hip_index_build(const uint8_t* data, uint32_t data_size, sla_hip_index** index);
int      sla_hip_index_build_resident(struct SLADecoder* decoder, const uint8_t* d_data, uint32_t data_size,
                                      sla_hip_stream_t stream, sla_hip_index** index);
int      sla_hip_index_info(const sla_hip_index* index, sla_hip_index_summary* info);
int      sla_hip_index_blocks(const sla_hip_index* index, uint32_t first, uint32_t count, sla_hip_index_block* out);
void     sla_hip_index_destroy(sla_hip_index* index);
uint64_t sla_hip_index_serialized_bytes(const sla_hip_index* index);
uint64_t sla_hip_index_serialize(const sla_hip_index* index, uint8_t* out, uint64_t capacity);
int      sla_hip_index_deserialize(const uint8_t* blob, uint64_t blob_bytes, sla_hip_index** index);

/* The judge kernel of sla_hip_decode_windows_indexed (k_dec_judge): the examination of the synchronous window call, on the
 * device.  One wave per item over its rows [first, first + nb) of the pass table.  A row's code is that of the first rule
 * that applies:
 *   1. stale index: the ten chain-header bytes at d_image + byte_off are not FF FF, size field + 6 == byte_len, sample
 *      count == num_samples, or do not lie inside [0, image_bytes)                  -> DETECT_DATA_CORRUPTION
 *   2. crc_check != 0 and d_info.crc != the big-endian field at byte 6              -> DETECT_DATA_CORRUPTION
 *   3. d_info.type > 2                                                              -> INVALID_HEADER_FORMAT
 *   4. d_info.type == 0 and lms_ok == 0                                             -> FAILED_TO_SYNTHESIZE
 *   5. d_info.overrun or d_info.used_bytes != byte_len                              -> DETECT_DATA_CORRUPTION
 * The item's result is the code of its LOWEST failing row, with none its `stop`; d_outcomes[outcome] = {result, result == OK
 * ? ok_samples : 0}.  A failed item's emit entry d_emit[emit] (emit = 0xFFFFFFFF: it has none) gets done = 0 and fill_end =
 * the item's fill_end, so that sla_hip_launch_dec_emit_batch behind it delivers nothing of it but the zero fill; entries of
 * clean items are not touched.  Items with nb = 0 get their stop code.  An item whose rows do not lie inside [0, num_blocks)
 * is judged NG; an outcome or emit position outside its table is not written.
 * INVALID_ARGUMENT before any launch for a NULL item or outcome table, a NULL emit table with num_emit > 0, or a NULL image,
 * block or info table with num_blocks > 0. */
typedef struct sla_hip_window_outcome { int32_t result; uint32_t output_num_samples; } sla_hip_window_outcome;   /* 8 bytes */
typedef struct sla_hip_dec_judge_item {
  uint32_t first;                 /* the item's rows in d_blocks / d_info: [first, first + nb) */
  uint32_t nb;
  uint32_t stop;                  /* its result when no row fails: an SLAApiResult */
  uint32_t ok_samples;            /* its output_num_samples when the result is OK */
  uint32_t outcome;               /* where in d_outcomes */
  uint32_t emit;                  /* its entry of d_emit, 0xFFFFFFFF for none */
  uint32_t fill_end;              /* what a failed item's emit entry gets: the window's length with the zero fill, else 0 */
  uint32_t reserved;
} sla_hip_dec_judge_item;         /* 32 bytes */
int sla_hip_launch_dec_judge(const uint8_t* d_image, uint64_t image_bytes, const sla_hip_dec_block* d_blocks,
                             const sla_hip_dec_info* d_info, uint32_t num_blocks, const sla_hip_dec_judge_item* d_items,
                             uint32_t num_items, uint32_t crc_check, uint32_t lms_ok, sla_hip_dec_emit* d_emit,
                             uint32_t num_emit, sla_hip_window_outcome* d_outcomes, uint32_t num_outcomes,
                             sla_hip_stream_t stream);

/* sla_hip_decode_windows_resident from block indexes, QUEUED: the call returns when its work is enqueued, not when it has
 * run.  Item i names a resident stream, its index (sla_hip_index_build* of those bytes, or a sidecar) and a window; d_outcomes
 * is device memory for num_items outcomes.
 * Contract: once the work `stream` holds at the time of the call has run, d_outcomes[i] and item i's destination hold exactly
 * what sla_hip_decode_windows_resident gives the same bytes, window, format, flags and handle configuration, provided the
 * index was built from those bytes: result and output_num_samples, every bit of [0, C) x [0, length), the zero fill, nothing
 * written outside that region, whole-or-nothing delivery, no resync, enable_crc_check honoured, the per-item refusals (source
 * and destination checks, start > num_samples, header failures, format verdicts, an LMS order the kernels do not run), and the
 * handle's wave format and encode parameter afterwards.  The header is the index's, not the device's: the host reads no byte
 * of the stream.  Also per item INVALID_ARGUMENT (nothing written) for a NULL index or index->data_size != data_size.
 * A needed block longer than the handle's max_num_block_samples ends the item's rows there with INSUFFICIENT_BUFFER_SIZE, as
 * the window walk does; for a window that reaches past the index's extent the index's stop code plays the walk's part.
 * Outcomes the host knows at once (refusals, empty windows) travel through d_outcomes too: the caller reads one place.
 * AN INDEX IS THE CALLER'S PROMISE, as a seek hint is.  Blocks in front of the window are not looked at.  Every needed
 * block's chain header is compared with its row on the device (k_dec_judge, rule 1), so bytes that changed under an old index
 * fail the window with DETECT_DATA_CORRUPTION or decode a block that still parses; whatever the index says, nothing outside
 * [data, data + data_size) is read and nothing outside the destination is written.
 * Ordering: the handle's stream waits on an event of `stream` before it reads or writes anything of the call; `stream` then
 * waits on the handle's closing event, so work queued on `stream` after the call sees the destinations and outcomes written.
 * How it runs, per pass (grouping and caps as in sla_hip_decode_windows_resident): the host lays out the gather table (one
 * range per item, first needed block to the end of the last), the block rows and ends, the judge and the emit table straight
 * from the indexes, into one slot of a ring of SLA_HIP_DEC_QUEUE_SLOTS page-locked staging slots, each guarded by an event; it
 * queues the table upload, the gather, the decode kernels, the judge, the emit.  No stream synchronisation, no copy home.
 * THE HOST MAY WAIT in two places only: a call that finds every ring slot still in flight waits for the oldest slot's
 * upload; a call that must grow a device buffer (or a staging slot) waits for the device as the allocator does.  Every OTHER
 * entry point of the handle first drains the handle's queued work: their staging is not ring-guarded.
 * sla_hip_decoder_last_timing: [4] = the host's queueing time, zeros elsewhere.
 * Returns 0; INVALID_ARGUMENT (nothing queued, nothing written) for a NULL decoder, a NULL d_outcomes or NULL items with
 * num_items > 0, an unknown format or flag, d_outcomes that is not device memory for num_items outcomes; NG on a device or
 * allocation failure. */
#define SLA_HIP_DEC_QUEUE_SLOTS 4u
typedef struct sla_hip_indexed_window_item {
  const uint8_t* data;            /* in : a whole .sla stream in device memory, any byte alignment */
  void*    dst;                   /* in : device memory */
  uint64_t channel_stride;        /* in : elements */
  uint64_t sample_stride;         /* in : elements (>= 1) */
  const sla_hip_index* index;     /* in : the stream's block index */
  uint32_t data_size;             /* in  */
  uint32_t start;                 /* in : first sample of the window */
  uint32_t length;                /* in : samples per channel of the window and of dst */
  uint32_t reserved;
} sla_hip_indexed_window_item;    /* 56 bytes */
int sla_hip_decode_windows_indexed(struct SLADecoder* decoder, const sla_hip_indexed_window_item* items, uint32_t num_items,
                                   uint32_t sample_format, uint32_t flags, sla_hip_window_outcome* d_outcomes,
                                   sla_hip_stream_t stream);

/* ---- Cut and join resident streams without re-encoding ----
 * Every block resets its filters and its coder and carries its own CRC16, so a new .sla stream is made from parts of old ones
 * by copying whole blocks byte for byte; only the blocks a cut passes through are decoded, and what remains of them is stored
 * as a RAW block (SILENT where the source block was).  Needs a decoder handle and the sources' block indexes only.
 *
 * THE LAYOUT RULE (sla_hip_splice_plan; pure host code, no device, no byte of any stream).  An output stream is the
 * concatenation of num_segments >= 1 segments; a segment names a stream, its index and the samples [start, start + length).
 * For every index row with samples that overlaps the segment, in order, with [a, b) the overlap:
 *   the whole row lies inside the segment   its byte_len bytes, verbatim;
 *   otherwise, byte_len == 11               an 11-byte SILENT block of b - a samples (only a SILENT block is 11 bytes long);
 *   otherwise                               a RAW block of n = b - a samples, 11 + ceil(n * W / 8) bytes, W the sum over the
 *                                           channels of bit_per_sample - offset_lshift (+ 1 for channel 1 under mid/side).
 * A segment inside one block gives one such block; adjacent partial blocks of two segments are not merged; length 0
 * contributes nothing; an output of no samples is the 43 header bytes with num_blocks 0.  Header: num_samples = the sum of
 * the lengths, num_blocks = blocks emitted, max_block_size = the largest of them, max_bit_per_second = the largest
 * (8 * bytes * sampling_rate mod 2^32) / samples over them, every other field the first segment's, the CRC slai_write_header's.
 * Refusals, in this order (then *layout is zero): INVALID_ARGUMENT for a NULL argument, no segments, a segment with a NULL
 * index, index->data_size != data_size, a header result other than OK, or header bytes 14, 19..28 or 33..34 (channels; rate,
 * bits, offset_lshift, the three orders, the channel process method; max_num_block_samples) that differ from the first
 * segment's; INVAILD_CHPROCESSMETHOD for mid/side with other than 2 channels, INVALID_HEADER_FORMAT for 0 or more than 8
 * channels, 0 or more than 32 bits or offset_lshift >= bits; for the first segment with length > 0 that reaches past its
 * index's extent the index's stop code (INSUFFICIENT_DATA_SIZE when that is OK); EXCEED_HANDLE_CAPACITY when bytes, samples or
 * blocks do not fit 32 bits.  `data` is not looked at.
 * The cost, plainly: edge blocks are stored uncompressed -- at most two per segment, each shorter than one block and never
 * larger than its PCM at the file's depth plus the 11 header bytes (and one bit per frame under mid/side). */
typedef struct sla_hip_splice_segment {
  const uint8_t* data;            /* in : a whole .sla stream in device memory, any byte alignment */
  const sla_hip_index* index;     /* in : its block index */
  uint32_t data_size;             /* in  */
  uint32_t start;                 /* in : first sample */
  uint32_t length;                /* in : samples */
  uint32_t reserved;
} sla_hip_splice_segment;         /* 32 bytes */
typedef struct sla_hip_splice_item {
  const sla_hip_splice_segment* segments;     /* in  */
  uint8_t* data;                  /* per-buffer mode: in, the destination (device); arena mode: out */
  uint32_t num_segments;          /* in  */
  uint32_t data_size;             /* per-buffer mode: in, the destination's capacity */
  uint32_t output_size;           /* out */
  int32_t  result;                /* out: SLAApiResult */
} sla_hip_splice_item;            /* 32 bytes */
typedef struct sla_hip_splice_layout {
  uint64_t verbatim_bytes;        /* bytes of the blocks copied as they are */
  uint32_t bytes;                 /* the output stream, header included */
  uint32_t num_samples;
  uint32_t num_blocks;
  uint32_t edge_blocks;           /* blocks written anew (RAW or SILENT) */
  uint32_t max_block_size;
  uint32_t max_bit_per_second;
  uint8_t  header[48];            /* the 43 header bytes; the rest zero */
} sla_hip_splice_layout;          /* 80 bytes */
int sla_hip_splice_plan(const sla_hip_splice_item* item, sla_hip_splice_layout* layout);

/* The streams sla_hip_splice_plan lays out, written to device memory.  Synchronous: it returns when every write has completed.
 * Item i gets result and output_size; a delivered item has exactly [data, data + output_size) written, byte for byte what the
 * layout rule says, the edge blocks holding the decoded samples of their range; a refused or failed item has NOTHING written
 * and output_size 0, the clean items of the same call are delivered.
 * Per-buffer mode (d_arena NULL) and arena mode are sla_hip_encode_batch_resident's: a destination of any byte alignment with
 * capacity data_size, INVALID_ARGUMENT for one that is NULL, not memory of the device or not inside its allocation,
 * INSUFFICIENT_BUFFER_SIZE for one that is too small; in arena mode the delivered streams lie back to back from a running
 * cursor in delivery order (passes by launch parameters as the decode calls sort them, items ascending inside a pass: a call
 * whose items share one format lies in item order), a stream that does not fit gets INSUFFICIENT_BUFFER_SIZE, data NULL and
 * the cursor stays, a failed item takes no space and gets data NULL; an arena that is not device memory inside one allocation
 * returns INVALID_ARGUMENT and touches no item.
 * Per item also: sla_hip_splice_plan's refusals; INVALID_ARGUMENT for a segment source that is NULL, not device memory or not
 * inside its allocation (sla_hip_decode_windows_indexed's source check, made before anything is read); the handle's
 * EXCEED_HANDLE_CAPACITY for a format it was not created for; INSUFFICIENT_BUFFER_SIZE for an edge block longer than the
 * handle's max_num_block_samples; EXCEED_HANDLE_CAPACITY for an item with more edge samples than one pass holds (2^28).
 * The host reads no byte of any stream: AN INDEX IS THE CALLER'S PROMISE, checked on the device.  Every verbatim block's ten
 * chain-header bytes are compared with its row (sync code, size field + 6 == byte_len, sample count; a row of 11 bytes must be
 * of type 1, a longer one must not), with enable_crc_check its CRC16 is recomputed; edge blocks are gathered, decoded by the
 * decode kernels and judged by k_dec_judge, and every folded sample they keep must fit its channel's width.  Any failure
 * gives the item DETECT_DATA_CORRUPTION, or for an edge block the judge's code; several failures: the first in output order.
 * With enable_crc_check 0 a damaged verbatim block is copied as it is.  Whatever the index says, nothing outside
 * [data, data + data_size) of a source is read.
 * Ordering behind `stream` as in sla_hip_decode_windows_indexed; the handle's wave format and encode parameter are afterwards
 * those of the last item whose header was accepted.
 * How it runs, per pass (items of one set of launch parameters): one gather of the edge blocks into the pass image, the decode
 * kernels, k_dec_judge one row per item, k_splice_check over every block; the verdicts come home in the pass's one wait; the
 * host places the clean items and uploads the delivery tables; k_splice_edges writes the edge blocks from the planes,
 * k_splice_copy the headers and the verbatim runs (touching rows are one entry).
 * sla_hip_decoder_last_timing: [2] the execution span of k_splice_edges and [3] of k_splice_copy, summed over the passes, [4]
 * the call, [5] the passes, zeros elsewhere.
 * Returns 0; INVALID_ARGUMENT (no item touched) for a NULL decoder, NULL items with num_items > 0 or a bad arena; NG on a
 * device or allocation failure. */
int sla_hip_splice_resident(struct SLADecoder* decoder, sla_hip_splice_item* items, uint32_t num_items, uint8_t* d_arena,
                            uint64_t arena_bytes, sla_hip_stream_t stream);

/* The check kernel of sla_hip_splice_resident (k_splice_check): one wave per entry, as described there.  d_verdicts: one
 * 64-bit word per item, set to all ones by the caller; a failing entry lowers word `verdict` to (ordinal << 8) | code.
 * edge == SLA_HIP_SPLICE_NO_EDGE: a verbatim block (src: its first byte in the source; byte_len, num_samples: its row).
 * Otherwise an edge block: d_outcomes[edge] is what k_dec_judge gave its row, the samples kept are [plane_off, plane_off + keep)
 * of every plane (an entry that names rows or samples outside the tables is judged NG).  Entries with byte_len < 11 fail.
 * INVALID_ARGUMENT before any launch for a NULL table, plane, outcome or verdict pointer, num_channels 0 or > 8, width 0 or
 * > 32, mid_side with num_channels != 2. */
#define SLA_HIP_SPLICE_NO_EDGE 0xFFFFFFFFu
typedef struct sla_hip_splice_check {
  const uint8_t* src;             /* device: the block's sync code in its source */
  uint64_t plane_off;             /* edge: the first kept sample in the planes */
  uint32_t byte_len;              /* the row's */
  uint32_t num_samples;           /* the row's */
  uint32_t verdict;               /* the item's word of d_verdicts */
  uint32_t ordinal;               /* the block's position in its output */
  uint32_t edge;                  /* SLA_HIP_SPLICE_NO_EDGE, or the block's outcome in d_outcomes */
  uint32_t keep;                  /* edge: samples kept */
} sla_hip_splice_check;           /* 40 bytes */
int sla_hip_launch_splice_check(const sla_hip_splice_check* d_table, uint32_t num_entries, uint32_t crc_check,
                                const int32_t* d_planes, uint64_t plane_stride, uint32_t num_channels, uint32_t width,
                                uint32_t mid_side, const sla_hip_window_outcome* d_outcomes, uint32_t num_outcomes,
                                uint64_t* d_verdicts, uint32_t num_verdicts, sla_hip_stream_t stream);

/* The edge kernel (k_splice_edges): entry k writes one whole block to [dst, dst + len) at any byte alignment -- sync code,
 * size field, CRC16 over [8, len), sample count, type, and for a RAW block (silent == 0) the frames of samples
 * [plane_off, plane_off + num_samples) of the planes (decoded, right-justified, mid/side still folded): per frame and channel the
 * zig-zag fold in `width` bits (+ 1 for channel 1 with mid_side; a 33-bit field is a zero bit and the 32 bits of the fold, as
 * slai_pack_block writes it), zero bits up to the byte boundary; len = 11 + ceil(num_samples * W / 8).  silent != 0: the 11 bytes
 * of a SILENT block.  No byte outside [dst, dst + len) is written, not even with its old value: entries may lie back to back
 * and beside ranges sla_hip_launch_splice_copy writes.  An entry with a NULL dst, num_samples 0 or > 65535, or samples outside
 * [0, plane_stride) is skipped.
 * INVALID_ARGUMENT before any launch for a NULL table or planes, num_channels 0 or > 8, width 0 or > 32, mid_side with
 * num_channels != 2. */
typedef struct sla_hip_splice_edge {
  uint8_t* dst;                   /* device, any alignment: the block's first byte */
  uint64_t plane_off;             /* the block's first sample in the planes */
  uint32_t num_samples;
  uint32_t silent;
} sla_hip_splice_edge;            /* 24 bytes */
int sla_hip_launch_splice_edges(const int32_t* d_planes, uint64_t plane_stride, const sla_hip_splice_edge* d_table,
                                uint32_t num_entries, uint32_t num_channels, uint32_t width, uint32_t mid_side,
                                sla_hip_stream_t stream);

/* The copy kernel (k_splice_copy): entry k writes exactly [dst, dst + bytes) from [src, src + bytes), device to device at any
 * pair of byte alignments.  No byte outside the destination range is written, not even with its old value; heads and tails go
 * out as guarded byte stores, the interior as 16-byte stores to aligned chunks, each made from the two aligned 16-byte words
 * of the source that hold it (loads touch only aligned 16-byte words that hold at least one byte of the source range).
 * Source and destination ranges must not overlap.  Entries with a NULL pointer are skipped.  max_bytes: the largest `bytes`
 * (sizes the grid).  INVALID_ARGUMENT before any launch for a NULL table. */
typedef struct sla_hip_splice_copy {
  const uint8_t* src;             /* device, any alignment */
  uint8_t* dst;                   /* device, any alignment */
  uint32_t bytes;
  uint32_t reserved;
} sla_hip_splice_copy;            /* 24 bytes */
int sla_hip_launch_splice_copy(const sla_hip_splice_copy* d_table, uint32_t num_entries, uint32_t max_bytes,
                               sla_hip_stream_t stream);

/* Decode-and-compare of blocks (option "verify" of the encoder; kernel k_verify_blocks): for every block of the table and
 * every channel, the decoded plane samples [smp_off, smp_off + num_samples) -- what dec_bits / dec_lms / dec_ltm /
 * dec_lattice left, right-justified, mid/side still folded -- are finished as sla_hip_launch_dec_finish_batch finishes them
 * (mid/side undone where mid_side = 1, left shift by `shift`) and compared with the words of d_source (planar int32,
 * left-justified, [C][source_stride]) at the same positions.  Equality is on all 32 bits: stray low bits of the source
 * count.  Nothing outside the blocks' sample ranges is read; blocks flagged SLA_HIP_DEC_HEADER_ONLY are skipped altogether.
 * A block is BAD when d_info[b].type != d_expect[b].type, d_info[b].used_bytes != d_expect[b].bytes, d_info[b].overrun is
 * set, or -- with a non-NULL d_image, the image dec_bits read, of image_bytes bytes -- the CRC16 dec_bits computed
 * (want_crc) differs from the big-endian 16-bit field at byte 6 of the block (or the block's first 8 bytes do not lie
 * inside the image).
 * d_report: three 64-bit words per segment (d_seg_of_block[b] = the segment of block b; NULL: everything is segment 0),
 * initialised by the caller to {0, ~0, 0}; afterwards {differing sample-channels, smallest (plane position << 3 | channel)
 * of a differing one, bad blocks}.  Waves reduce first and touch the words (64-bit vector atomics) only when they have
 * something to report: a clean table leaves them as they were.  16-byte loads wherever a row of the planes / the source is
 * 16-byte aligned and the group of four lies inside the block, guarded 4-byte loads at block heads and tails and otherwise.
 * INVALID_ARGUMENT before any launch for a NULL table, num_channels 0 or > 8, mid_side with num_channels != 2, shift > 31. */
typedef struct sla_hip_verify_expect {
  uint32_t type;            /* the block type the packer wrote */
  uint32_t bytes;           /* the block's size in the image */
} sla_hip_verify_expect;
int sla_hip_launch_verify_blocks(const int32_t* d_planes, uint64_t plane_stride, const int32_t* d_source,
                                 uint64_t source_stride, const sla_hip_dec_block* d_blocks,
                                 const sla_hip_dec_info* d_info, const sla_hip_verify_expect* d_expect,
                                 const uint32_t* d_seg_of_block, uint32_t num_blocks, uint32_t num_channels,
                                 uint32_t mid_side, uint32_t shift, const uint32_t* d_image, uint64_t image_bytes,
                                 uint64_t* d_report, sla_hip_stream_t stream);

/* ---- (2) whole-file driver ---------------------------------------------- */

/* Long blocks: encode parameters with max_num_block_samples of 16 385 to 65 535 (the format's 16-bit block length; the
 * reference's library writes such blocks as soon as the parameter asks for them).  SLAEncoder_SetEncodeParameter accepts up to
 * min(the handle's capacity, 65 535), SLAEncoder_EncodeBlock blocks up to the handle's capacity once such a parameter is set.
 * While such a parameter is set the handle takes, WHATEVER its options say (they are neither changed nor consulted, and hold
 * again for the next ordinary parameter), the routes that are exact and host-planned at any block length:
 *   search          sla_hip_launch_lpc_far, search form: one group per (super-frame, channel) with all its candidates
 *   planner         the host's (sla_plan.c: up to 66 nodes); k_plan is sized for 17
 *   block tables    built on the host: no "device_plan", "device_expand", "search_early", no kept tables, no speculation, one chunk
 *   block stage     sla_hip_launch_lpc_far, block form; no "block_cert" (the certificate's constants were validated for n <= 16 384)
 *                   and no fused lattice; the lattice, tail, Rice and pack kernels are general in the block length
 *   long-term stage the exact route (no "ltm_cert" / "ltm_int"): transforms of 65 536 and 131 072 points through the global scratch
 *   silence         through the mask (no "silence_runs")
 * and the sla_hip_last_* reports say so (no tile sums, no device plan, no device tables, no certificate).  Output is the
 * reference's, byte for byte.  Slower per sample than ordinary parameters (profiles/long_enc.json).
 * Option "long_tile_search" (0 or 1, default 0; consulted only while such a parameter is set): with 1 and an order of at most 51
 * the search takes 64-tile sums -- sla_hip_launch_search_far over the same groups, at the ordinary route's limit ("exact_bits",
 * the samples' unit, mid/side), then sla_hip_launch_lpc_far_rerun for the groups at or over it -- and sla_hip_last_counters
 * reports [2] = 1 and [0] = the groups rerun as chains; the planner, the other stages and the other reports are as above, and so
 * are the bytes.  16-bit material has no group over the limit and its search all but disappears (profiles/long_search.json);
 * loud material wider than 16 bits (a 65 535-sample window above about -31 dBFS rms at 24 bits) has every group over it and
 * keeps the chains' cost: there is no certificate for 64 tiles.  Orders above 51 keep the far chains ([2] = 0).  The calls
 * that reach the search: SLAEncoder_EncodeWhole, sla_hip_analyze_device with either pack, sla_hip_encode_batch.
 * Calls that take long blocks:      SLAEncoder_EncodeWhole (never streamed over worker lanes), SLAEncoder_EncodeBlock,
 *                                   sla_hip_analyze_device with sla_hip_pack or sla_hip_pack_device, sla_hip_encode_batch (no lanes).
 * Calls that refuse them, with SLA_APIRESULT_EXCEED_HANDLE_CAPACITY before anything is launched: sla_hip_encode_batch_device,
 *                                   sla_hip_encode_batch_resident, sla_hip_encode_wav_batch, sla_hip_encode_wav_batch_resident,
 *                                   sla_hip_analyze_batch_device, sla_hip_pack_resident, sla_hip_shard_analyze,
 *                                   sla_hip_shard_analyze_no_silence, sla_hip_verify_last_image, and each of the four calls above while
 *                                   option "verify" is on.
 * A handle of a capacity above 16 384 that is given an ordinary parameter is an ordinary handle, except that its long-term FFT
 * follows the capacity, as the reference's does: above 32 768 points (capacity above 16 384) sla_hip_ltm_cert_supported is 0
 * and its long-term stage takes the exact route at every parameter.  The per-call SLAPredictor API keeps its 16 384 samples. */

/* Per-block results of the last analyze call, copied into caller arrays
 * (layout identical to the oracle's trace so tests can diff them). */
typedef struct sla_hip_trace {
  uint32_t  max_blocks;      /* in  */
  uint32_t  order_stride;    /* in: parcor_order + 1 */
  uint32_t  ltm_stride;      /* in: longterm_order   */
  uint32_t  sample_stride;   /* in: per-channel stride of res_* (>= num_samples) */
  uint32_t  num_blocks;      /* out */
  uint32_t  offset_lshift;   /* out */
  uint32_t* blk_start; uint32_t* blk_nsmpl; uint32_t* blk_type; uint32_t* blk_bytes;
  double*   parcor; int32_t* code; int32_t* kint;
  uint32_t* rshift; uint32_t* pitch; int32_t* ltm_coef; uint32_t* rice_init;
  int32_t*  res_lattice; int32_t* res_final;    /* may be NULL: not copied back */
  uint32_t* parcor_exact;    /* may be NULL; per (block, channel): 1 = parcor[] are the reference's doubles bit for bit (exact
                                chain kernel), 0 = certified: code[], kint[] and the RAW decision are the reference's, the
                                doubles agree to the certificate's bound (option "block_cert") */
} sla_hip_trace;

/* Hot path on PCM resident in device memory: planar int32 [C][plane_stride],
 * left-justified.  On return the encoder holds, on the device, the final
 * residual planes and, on the host, the block table and per-block parameters.
 * `timing_ms` (may be NULL) receives 12 floats [ms]: HIP-event durations of k_prepass, k_lpc (search),
 * k_lpc (blocks), k_lattice, k_tail; host wall time of planning and of the long-term solve; total
 * wall time; HIP-event duration of k_ltm_acf; number of pipeline chunks; search groups that had to rerun
 * as serial chains; 1 if the search ran on tile sums (sla_hip_launch_search_exact), else 0. */
int sla_hip_analyze_device(struct SLAEncoder* encoder, const int32_t* d_pcm, uint64_t plane_stride,
                           uint32_t num_samples, sla_hip_stream_t stream, float* timing_ms);

/* Bit-serial pack of the analysed file into `data` (host): D2H of the final
 * residual, block headers, Rice body, CRC16 (reference src/SLAEncoder.c:682-798,
 * src/SLACoder.c:429-467).  Needs a preceding sla_hip_analyze_device.  These bytes are made on the host and
 * never exist on the device: option "verify" does not cover them (SLAEncoder_EncodeBlock packs this way too). */
int sla_hip_pack(struct SLAEncoder* encoder, uint8_t* data, uint32_t data_size, uint32_t* output_size);

/* Same bytes as sla_hip_pack, but the Rice coding, block assembly and CRC16 run on the device and one
 * D2H copy brings the finished image back.  Used by SLAEncoder_EncodeWhole. */
int sla_hip_pack_device(struct SLAEncoder* encoder, uint8_t* data, uint32_t data_size, uint32_t* output_size);

/* Many files in one call (BASELINE C4: a batch of short clips).  Each file is encoded exactly as
 * SLAEncoder_EncodeWhole would encode it on its own -- same bytes, own header, own offset_lshift -- but the blocks
 * of all files travel through the kernels together (they are as independent as the blocks of one file), so a
 * 10-second clip no longer costs the fixed latency of the whole pipeline.  All files share the encoder's wave format
 * and parameters.  Returns 0 when the batch ran; each item carries its own SLAApiResult (e.g. a buffer too small). */
typedef struct sla_hip_batch_item {
  const int32_t* const* input;     /* in : [num_channels] planes, left-justified in 32 bits */
  uint32_t num_samples;            /* in  */
  uint32_t data_size;              /* in : capacity of `data` */
  uint8_t* data;                   /* in : receives the .sla bytes */
  uint32_t output_size;            /* out */
  int32_t  result;                 /* out: SLAApiResult of this file */
} sla_hip_batch_item;
int sla_hip_encode_batch(struct SLAEncoder* encoder, sla_hip_batch_item* items, uint32_t num_items);
/* The analysis of such a batch when the planes already live in device memory ([C][plane_stride] int32, files at
 * file_start[i] -- multiples of SLA_HIP_PREPASS_TILE, ascending, gaps zero -- of file_samples[i] samples, all inside
 * [0, span)): the batch counterpart of sla_hip_analyze_device.  file_lshift (may be NULL) receives every file's
 * offset_lshift; files that share a value share a pipeline pass.  After a single pass sla_hip_get_trace describes the
 * blocks of all files (positions relative to the planes). */
int sla_hip_analyze_batch_device(struct SLAEncoder* encoder, const int32_t* d_pcm, uint64_t plane_stride, uint32_t span,
                                 const uint32_t* file_start, const uint32_t* file_samples, uint32_t num_files,
                                 uint32_t* file_lshift, float* timing_ms);

/* Many files whose PCM already lives in caller-owned DEVICE memory, encoded to .sla bytes in host memory: the encode-side
 * mirror of sla_hip_decode_batch_device.  Sample i of channel c of an item is the element c * channel_stride +
 * i * sample_stride of src, for c < C (the handle's channel count) and i < num_samples.  With bps the handle's
 * bit_per_sample, sample_format turns the element v into the left-justified word L of the file's plane:
 *   SLA_HIP_PCM_S32_LEFT  int32  L = v
 *   SLA_HIP_PCM_S32       int32  L = (uint32)v << (32 - bps); any v outside [-2^(bps-1), 2^(bps-1) - 1] refuses the item
 *   SLA_HIP_PCM_S16       int16  L = (uint32)v << 16
 *   SLA_HIP_PCM_F32       float  L = q << (32 - bps), q = rint(v * 2^(bps-1)) (ties to even) saturated to
 *                                [-2^(bps-1), 2^(bps-1) - 1], +-inf saturate; any NaN refuses the item
 * Every item gets exactly the result, output_size and bytes that sla_hip_encode_batch on this handle gives for host planes
 * holding those L words: low bits below bps give INVALID_ARGUMENT, a buffer too small INSUFFICIENT_BUFFER_SIZE, an empty
 * file the 43-byte header, and every file has its own offset_lshift.  A refused item gets INVALID_ARGUMENT, output_size 0
 * and nothing in its data.  Round trips are exact: the SLA_HIP_PCM_S32_LEFT or SLA_HIP_PCM_S32 output of
 * sla_hip_decode_batch_device fed back in the same format, its SLA_HIP_PCM_S16 output when bps <= 16, its SLA_HIP_PCM_F32
 * output when bps <= 24.
 * Per item, on the host before any device work (nothing is then read from its src), INVALID_ARGUMENT for: NULL data, NULL
 * src with num_samples > 0, sample_stride == 0, channel_stride == 0 with more than one channel, src not aligned to the
 * element size, a region whose byte extent overflows, a src the runtime does not report as device memory of the handle's
 * device (host and page-locked host memory included), a region outside src's allocation.
 * Passes are those of sla_hip_encode_batch (files back to back on SLA_HIP_PREPASS_TILE starts, at most 2^28 samples per
 * channel, a larger file in a pass of its own), run in one piece -- no worker lanes: they overlap host uploads, and there
 * are none -- with one sla_hip_launch_enc_ingest_batch per pass in place of the staging and upload.  The handle's stream
 * waits on an event recorded on `stream` (NULL: the null stream) before the first read; the call returns when every byte
 * is in the host buffers and no kernel reads src any more.  src is never written.  Afterwards the handle is where
 * sla_hip_encode_batch leaves it: no analysis to trace or pack, offset_lshift of the last pass.
 * Returns 0 when the batch ran; INVALID_ARGUMENT for a NULL encoder, NULL items with num_items > 0 or an unknown format,
 * the code sla_hip_encode_batch gives for parameters that are not set, EXCEED_HANDLE_CAPACITY for a num_samples above the
 * pass cap -- then no item is touched. */
typedef struct sla_hip_encode_device_item {
  const void* src;                /* in : device memory */
  uint64_t channel_stride;        /* in : elements */
  uint64_t sample_stride;         /* in : elements (>= 1) */
  uint8_t* data;                  /* in : HOST buffer that receives the .sla bytes */
  uint32_t num_samples;           /* in : samples per channel */
  uint32_t data_size;             /* in : capacity of data */
  uint32_t output_size;           /* out */
  int32_t  result;                /* out: SLAApiResult */
} sla_hip_encode_device_item;     /* 48 bytes */
int sla_hip_encode_batch_device(struct SLAEncoder* encoder, sla_hip_encode_device_item* items, uint32_t num_items,
                                uint32_t sample_format, sla_hip_stream_t stream);

/* The ingest kernel of sla_hip_encode_batch_device: for every file of the table, its num_samples samples of each of
 * num_channels channels are read from src, converted as sample_format says (bits_per_sample = bps of the table above) and
 * stored to d_planes[c * plane_stride + plane_off + i]; [num_samples, fill_end) of every plane is written zero in the same
 * launch.  Refusals only the samples can show are ORed into d_error[file] (zeroed by the caller): 1 = an SLA_HIP_PCM_S32
 * element out of range, 2 = an SLA_HIP_PCM_F32 NaN.  plane_off, plane_stride and d_planes aligned to 4 words give 16-byte
 * plane stores.  max_samples: the largest max(num_samples, fill_end) of the table (sizes the grid). */
typedef struct sla_hip_enc_ingest {
  uint64_t plane_off;             /* first sample of the file's region in every plane */
  uint64_t channel_stride;        /* elements of src */
  uint64_t sample_stride;         /* elements of src */
  const void* src;                /* device */
  uint32_t num_samples;           /* samples per channel read from src */
  uint32_t fill_end;              /* [num_samples, fill_end) is written zero; <= num_samples: nothing */
  uint32_t bits_per_sample;
  uint32_t reserved;
} sla_hip_enc_ingest;             /* 48 bytes */
int sla_hip_launch_enc_ingest_batch(const sla_hip_enc_ingest* d_files, uint32_t num_files, uint32_t max_samples,
                                    uint32_t num_channels, uint32_t sample_format, int32_t* d_planes, uint64_t plane_stride,
                                    uint32_t* d_error, sla_hip_stream_t stream);

/* sla_hip_encode_batch_device with the .sla bytes delivered to DEVICE memory: nothing of a file ever crosses the bus, so
 * Decoder-side sla_hip_decode_batch_resident (or a collective, or a GPUDirect write) can take the files where they are.
 * The item struct, the source side and the formats, the per-item source refusals, the pass grouping, the ingest, the
 * ordering behind `stream` and the run in one piece (no worker lanes) are sla_hip_encode_batch_device's.  Result code,
 * output_size and every byte of every file equal what that call on this handle gives for the same sources with a host
 * buffer of the same capacity.
 * Per-buffer mode (d_arena NULL): items[i].data is a device pointer of any byte alignment (slices of one big uint8 buffer
 * are fine) with capacity data_size.  Per item, on the host before any device work, INVALID_ARGUMENT also for: NULL data, a
 * data the runtime does not report as memory of the handle's device, a [data, data + data_size) that does not lie inside
 * its allocation.  INSUFFICIENT_BUFFER_SIZE exactly where the host call gives it (data_size < 43, or the file does not fit).
 * A refused or failed item gets output_size 0 and nothing of its buffer is written; a delivered one has exactly
 * [data, data + output_size) written.  Overlapping destinations are undefined.
 * Arena mode (d_arena non-NULL): data and data_size of every item are ignored on input; the delivered files are placed back
 * to back, no padding, in [d_arena, d_arena + arena_bytes), and on output data is the file's first byte and output_size its
 * size.  Placement follows delivery order: passes in item order; inside a pass the groups of equal offset_lshift in the
 * order of each group's first item, items ascending inside a group -- a batch whose files share one offset_lshift and one
 * pass lies in item order.  A running cursor starts at 0; a file that does not fit the remaining bytes gets
 * INSUFFICIENT_BUFFER_SIZE, data NULL and output_size 0, the cursor stays and later files are still tried.  Refused items
 * take no space and get data NULL.  An arena that is not memory of the handle's device or does not lie in one allocation:
 * the call returns INVALID_ARGUMENT and touches no item.
 * How it runs: per pack of a pass (one per offset_lshift group) the host builds every delivered file's 43-byte header into
 * a table of sla_hip_enc_emit, one upload brings the table to the device and one sla_hip_launch_enc_emit_batch copies the
 * files out of the pack image, headers in front, before the next group's pack reuses the image.  No block byte is copied to
 * the host.  With option "verify" the decode-and-compare runs on the image as ever and the emit is launched only after the
 * verdict is home: a file that fails gets SLA_APIRESULT_NG, nothing written and (arena mode) no arena space; the files that
 * did not fit the arena were settled before the verdict and are not tried again in the room a failing file leaves.
 * sla_hip_last_verify reports as for the host route.
 * The call returns when every write has completed and no kernel reads a source any more.  Call-level refusals as for
 * sla_hip_encode_batch_device -- then no item is touched. */
int sla_hip_encode_batch_resident(struct SLAEncoder* encoder, sla_hip_encode_device_item* items, uint32_t num_items,
                                  uint32_t sample_format, uint8_t* d_arena, uint64_t arena_bytes, sla_hip_stream_t stream);

/* sla_hip_pack_device of the analysed file into a DEVICE buffer (any byte alignment): same preconditions, result codes and
 * bytes, plus INVALID_ARGUMENT for a d_data that is not memory of the handle's device or whose [d_data, d_data + data_size)
 * does not lie inside its allocation.  The blocks are written in a single run (no overlapped download: there is none) and
 * one sla_hip_launch_enc_emit_batch delivers the file; on a refusal nothing is written.  Afterwards the handle holds the
 * image as after sla_hip_pack_device: sla_hip_verify_last_image works on it. */
int sla_hip_pack_resident(struct SLAEncoder* encoder, uint8_t* d_data, uint32_t data_size, uint32_t* output_size);

/* The emit kernel of sla_hip_encode_batch_resident (k_enc_emit), the mirror of sla_hip_launch_dec_gather: entry k writes
 * exactly [dst, dst + bytes): byte i is header[i] for i < header_bytes and d_image[img_off + i] otherwise.  No byte outside
 * that range is written, not even with the value it already holds -- entries may be packed back to back, sharing 4-byte
 * words and 16-byte chunks that other lanes write in the same launch: the head (with the header) and the tail of every
 * destination go out as guarded byte stores, the interior as 16-byte stores to 16-byte-aligned chunks, each made from two
 * aligned 16-byte loads.  Loads touch only the 16-byte words, aligned by ADDRESS, that hold at least one byte of
 * [img_off, img_off + bytes) of the image: such a word may reach up to 15 bytes before d_image + img_off or past the file's
 * end, so the image's allocation must be readable from the 16-byte boundary at or before its first file to the one at or
 * behind its last (a d_image aligned to 16 bytes in an allocation padded to a multiple of 16 is; the driver's is).
 * An entry is skipped whole when img_off + bytes exceeds image_bytes, when header_bytes is neither 0 nor 43, or when
 * header_bytes > bytes.  max_bytes: the largest `bytes` of the table (sizes the grid).  d_image and the destinations must
 * not overlap.  INVALID_ARGUMENT before any launch for a NULL table or image. */
typedef struct sla_hip_enc_emit {
  uint64_t img_off;               /* first byte of the file in d_image (any alignment) */
  uint8_t* dst;                   /* device, any alignment */
  uint32_t bytes;                 /* size of the file, header included */
  uint32_t header_bytes;          /* 0 (bare image: copy everything) or 43 */
  uint8_t  header[48];            /* the first header_bytes bytes of the file; the rest of the array is ignored */
} sla_hip_enc_emit;               /* 72 bytes */
int sla_hip_launch_enc_emit_batch(const sla_hip_enc_emit* d_table, uint32_t num_entries, uint32_t max_bytes,
                                  const uint8_t* d_image, uint64_t image_bytes, sla_hip_stream_t stream);

/* ---- WAV files (sla_wav.c; kernels/wav.inc) ------------------------------------------------------------------
 * A reader and a writer of RIFF/WAVE headers on the host, and the byte work of the data chunk -- unpack, de-interleave,
 * widen on the way in; finish, narrow, interleave, pack on the way out -- on the device.  With L the left-justified plane
 * word, little-endian samples, frames interleaved:
 *     8-bit (unsigned byte u)  L = (u - 128) << 24      u = (L >> 24) + 128
 *     16-bit                   L = s << 16              s = L >> 16 (arithmetic)
 *     24-bit                   L = s << 8               s = L >> 8  (arithmetic)
 *     32-bit                   L = s                    s = L
 *
 * sla_hip_wav_parse accepts: `RIFF`, a size field that is ignored, `WAVE`; chunks walked from byte 12 (id, little-endian
 * size, body, and the pad byte RIFF prescribes after a body of odd size); a `fmt ` chunk of at least 16 bytes somewhere
 * before `data`, other chunks before and between them skipped; format tag 1, or 0xFFFE (extensible) with the extension
 * present (chunk >= 40 bytes, cbSize >= 22), a sub-format whose first two bytes are 1 and valid bits equal to the container
 * bits; 8, 16, 24 or 32 bits; at least one channel.  Byte rate and block align are ignored.  A data chunk that is no whole
 * number of frames is floored.  Result codes: INVALID_ARGUMENT for a NULL argument; INVALID_HEADER_FORMAT for a missing
 * signature (a file shorter than 12 bytes has none), `data` before `fmt `, a `fmt ` shorter than 16 bytes, any other tag,
 * depth, or zero channels; INSUFFICIENT_DATA_SIZE when the chunk chain runs off the end of the file before `data` or the
 * data chunk claims more bytes than the file holds.  Offsets are computed in 64 bits, no byte outside [data, data + size)
 * is read.  On any failure *info is zero.
 * sla_hip_wav_header writes the canonical 44-byte header: `RIFF`, 36 + data_bytes, `WAVEfmt `, 16, tag 1, channels, rate,
 * byte rate, block align, bits, `data`, data_bytes. */
#define SLA_HIP_WAV_HEADER_BYTES 44u
typedef struct sla_hip_wav_info {
  uint32_t num_channels, bits_per_sample, sampling_rate;
  uint32_t num_samples;     /* frames = data_bytes / (num_channels * bits_per_sample / 8), floored */
  uint32_t data_off;        /* file position of the first sample byte */
  uint32_t data_bytes;      /* num_samples * num_channels * bits_per_sample / 8 */
} sla_hip_wav_info;
int sla_hip_wav_parse(const uint8_t* data, uint32_t size, sla_hip_wav_info* info);
int sla_hip_wav_header(const sla_hip_wav_info* info, uint8_t out[SLA_HIP_WAV_HEADER_BYTES]);

/* The ingest kernel of the WAV encode calls, the mirror of sla_hip_launch_enc_ingest_batch for packed frames.  One launch
 * serves files that share num_channels (1 .. 8) and bytes_per_sample (1 .. 4).  Sample i of channel c of an entry is the
 * bytes_per_sample bytes at src + (i * num_channels + c) * bytes_per_sample (src: device, ANY byte alignment); it is
 * converted as the table above says and stored to d_planes[c * plane_stride + plane_off + i]; [num_samples, fill_end) of
 * every plane is written zero in the same launch; nothing else is written.  Loads touch only the aligned 16-byte words
 * that overlap [src, src + num_samples * num_channels * bytes_per_sample): a data chunk may end at the last byte of an
 * allocation.  plane_off, plane_stride and d_planes aligned to 4 words give 16-byte plane stores.  One and two channels: a
 * lane takes 4 whole frames from the 2 or 3 aligned words that hold them, realigned in registers; more channels: one frame
 * per lane, byte loads.  max_samples: the largest max(num_samples, fill_end) of the table (sizes the grid).
 * INVALID_ARGUMENT before any launch for a NULL table or planes, num_channels outside 1 .. 8, bytes_per_sample outside
 * 1 .. 4. */
typedef struct sla_hip_wav_ingest {
  const uint8_t* src;             /* device: the first byte of frame 0 */
  uint64_t plane_off;             /* first sample of the file's region in every plane */
  uint32_t num_samples;           /* frames read from src */
  uint32_t fill_end;              /* [num_samples, fill_end) is written zero; <= num_samples: nothing */
} sla_hip_wav_ingest;             /* 24 bytes */
int sla_hip_launch_wav_ingest_batch(const sla_hip_wav_ingest* d_files, uint32_t num_files, uint32_t max_samples,
                                    uint32_t num_channels, uint32_t bytes_per_sample, int32_t* d_planes,
                                    uint64_t plane_stride, sla_hip_stream_t stream);

/* The emit kernel of the WAV decode calls, the mirror of sla_hip_launch_dec_emit_batch and of k_enc_emit for WAV files.
 * Entry k writes exactly [dst, dst + header_bytes + num_samples * num_channels * bytes_per_sample): byte i is header[i] for
 * i < header_bytes, then the frames of the file's region of the planes, finished as sla_hip_launch_dec_emit_batch finishes
 * them (mid/side undone, left shift by `shift`) and converted as the table above says.  No byte outside that range is
 * written, not even with the value it already holds -- destinations may be packed back to back and share 4-byte words and
 * 16-byte chunks with neighbours written in the same launch: heads (with the header) and tails go out as guarded byte
 * stores, interiors as 16-byte stores to 16-byte-aligned chunks.  An entry is skipped whole when header_bytes is neither 0
 * nor 44 (or dst is NULL).  mid_side (the launch's): 0 = the entries' mid_side fields are ignored, 1 = they apply.
 * max_samples: the largest num_samples of the table (sizes the grid).
 * INVALID_ARGUMENT before any launch for a NULL table or planes, num_channels outside 1 .. 8, bytes_per_sample outside
 * 1 .. 4, mid_side != 0 with num_channels != 2. */
typedef struct sla_hip_wav_emit {
  uint64_t plane_off;             /* first sample of the file's region in every plane */
  uint8_t* dst;                   /* device, any alignment */
  uint32_t num_samples;           /* frames read from the planes */
  uint32_t mid_side;              /* 1: planes 0 / 1 are mid / side (two channels only) */
  uint32_t shift;                 /* left shift of the left-justification: 32 - bits_per_sample + offset_lshift */
  uint32_t header_bytes;          /* 0 (frames only) or 44 */
  uint8_t  header[48];            /* the first header_bytes bytes of the file; the rest of the array is ignored */
} sla_hip_wav_emit;               /* 80 bytes */
int sla_hip_launch_wav_emit_batch(const int32_t* d_planes, uint64_t plane_stride, const sla_hip_wav_emit* d_table,
                                  uint32_t num_entries, uint32_t max_samples, uint32_t num_channels,
                                  uint32_t bytes_per_sample, uint32_t mid_side, sla_hip_stream_t stream);

/* Whole WAV files in, whole .sla files out, and back.  Plain = host memory to host memory, _resident = device memory to
 * device memory (pointers of any byte alignment).
 *
 * Encode.  Host sources are parsed in place; device sources are probed: one sla_hip_launch_dec_gather of the first
 * min(size, 4096) bytes of every admissible item and one copy home, again at the chunk offset reached for files whose `data`
 * chunk header lies beyond the probe, in rounds of one gather and one copy for all unresolved files; after 64 rounds an
 * unresolved file gets INVALID_HEADER_FORMAT.  Per item: the code of sla_hip_wav_parse; INVALID_ARGUMENT for a NULL src, a
 * NULL dst outside arena mode and, on the resident call, a src or dst that sla_hip_encode_batch_resident's pointer and
 * allocation checks refuse; EXCEED_HANDLE_CAPACITY for more channels than the handle's max_num_channels or more frames than
 * the pass cap.  Items are grouped by (channels, bits, rate) in order of first appearance; for each group the call does what
 * SLAEncoder_SetWaveFormat does and runs the group as sla_hip_encode_batch_device runs a batch, with
 * sla_hip_launch_wav_ingest_batch as the ingest.  A file of other than two channels is encoded with ch_process_method NONE
 * when the handle's parameter says STEREO_MS, as the reference's tool does; the handle's encode parameter is unchanged
 * afterwards, its wave format is the last group's.  The host call stages the data chunks of each pass -- and only those -- in
 * page-locked memory and brings them to the device in one transfer; from there on it is the resident call with host
 * delivery.  The resident call reads the data chunk where it lies.
 * Every item gets exactly the result code, size and bytes that sla_hip_encode_batch on a handle with that wave format and
 * that parameter gives for the planes of the sample map above: its own offset_lshift, the 43-byte header for an empty data
 * chunk, INSUFFICIENT_BUFFER_SIZE where that call gives it; options "verify" and "silence_runs" work as on the device
 * route.  A refused item gets output_size 0 and nothing written.  Arena mode (d_arena non-NULL) is
 * sla_hip_encode_batch_resident's, group after group: dst and dst_capacity are ignored on input, dst is the file's place
 * on output (NULL when nothing was delivered).
 * Returns 0 when the batch ran; INVALID_ARGUMENT for a NULL encoder, NULL items with num_items > 0 or an arena that is not
 * device memory; PARAMETER_NOT_SET without an encode parameter; what sla_hip_encode_batch gives for a parameter it refuses.
 *
 * Decode.  The items go through the batch decode as sla_hip_decode_batch_device / _resident run them, every item's capacity
 * the num_samples of its header; the last leg is sla_hip_launch_wav_emit_batch -- for the host call into a device staging
 * image that one download per pass brings home.  A WAV is delivered whole or not at all: when the decode's result is OK and
 * every sample of the header's num_samples was produced, [dst, dst + 44 + num_samples * C * B) is written, output_size is
 * that size and num_samples is set; on any decode failure the item carries that failure's code, output_size 0, and nothing
 * is written.  INSUFFICIENT_BUFFER_SIZE when dst_capacity is smaller than the file (computed in 64 bits: a file of 4 GiB or
 * more cannot be delivered); INVALID_HEADER_FORMAT for a stream whose bit_per_sample is not 8, 16, 24 or 32;
 * INVALID_ARGUMENT for NULL src or dst and, on the resident call, what sla_hip_decode_batch_resident's pointer checks
 * refuse.  The handle's wave format and encode parameter afterwards are what sla_hip_decode_batch_resident leaves;
 * sla_hip_decoder_last_timing keeps its split with [3] = the WAV emit (and the download). */
typedef struct sla_hip_wav_item {
  const uint8_t* src;  uint8_t* dst;
  uint32_t src_size;   uint32_t dst_capacity;
  uint32_t output_size;   /* out */
  int32_t  result;        /* out: SLAApiResult */
  uint32_t num_samples;   /* out: frames of the file */
  uint32_t reserved;
} sla_hip_wav_item;       /* 40 bytes */
int sla_hip_encode_wav_batch(struct SLAEncoder* encoder, sla_hip_wav_item* items, uint32_t num_items);
int sla_hip_encode_wav_batch_resident(struct SLAEncoder* encoder, sla_hip_wav_item* items, uint32_t num_items,
                                      uint8_t* d_arena, uint64_t arena_bytes, sla_hip_stream_t stream);
int sla_hip_decode_wav_batch(struct SLADecoder* decoder, sla_hip_wav_item* items, uint32_t num_items);
int sla_hip_decode_wav_batch_resident(struct SLADecoder* decoder, sla_hip_wav_item* items, uint32_t num_items,
                                      sla_hip_stream_t stream);

/* ---- one file, several GPUs ------------------------------------------------------------------------------
 * Blocks are independent (every filter and the coder reset per block, src/SLAEncoder.c:594-659), so the super-frames
 * of ONE file shard over the GPUs of a node, one process and one encoder handle per GPU.  Three facts of the whole
 * file have to be agreed on first, and the library leaves the exchange to the caller (RCCL from C, or
 * torch.distributed as in sla_amd/dist.py -- the library itself links no collective library):
 *   offset_lshift   comes from the OR of EVERY sample (src/SLAEncoder.c:425-455)      -> OR of 4 bytes per rank (all-gathered: RCCL has no bitwise reduction)
 *   super-frames    hop over silence runs, so where one starts depends on everything before it
 *                   (src/SLAEncoder.c:392-408, 846-869)                                -> all-gather of the 1-bit mask
 *   the header      counts blocks and keeps the largest block / bit rate (:920-926)   -> gathered with the bytes
 * Sequence on rank r of `world` (file of N samples per channel, pieces cut at multiples of 1024):
 *   1. scan pieces tile [0, N): piece r = [cut(r), cut(r+1)), cut(r) = ceil(N*r/world) floored to a multiple of 1024.
 *      Upload [cut(r), min(N, cut(r+1) + 1023 + max_num_block_samples)): bounds[r+1] of step 3 is the first
 *      super-frame start at or behind the UNFLOORED target ceil(N*(r+1)/world), i.e. less than one maximum block
 *      behind it (sla_amd/dist.py: upload_range);
 *      sla_hip_shard_scan on exactly the piece  ->  OR word, mask bits of the piece
 *   2. all-gather the OR words and OR them, all-gather the mask pieces (N/8 bytes in total)
 *   3. sla_hip_shard_bounds (pure host arithmetic, every rank computes the same table): rank r owns
 *      [bounds[r], bounds[r+1]), both super-frame starts of the whole file's hop
 *   4. sla_hip_shard_analyze on the planes of that range with the file's OR word (the hot path: exactly
 *      sla_hip_analyze_device, but offset_lshift and the sample unit are the file's), then sla_hip_pack_device:
 *      a complete .sla image of the range, 43-byte header + blocks
 *   5. gather sizes and bytes on one rank (all-gather over xGMI: compressed bytes, less than the residual planes the
 *      north star's variant gathers -- sla_amd/dist.py keeps both); that rank drops the headers of ranks > 0 and
 *      writes the file's header with sla_hip_shard_header.
 * The result is byte-identical to SLAEncoder_EncodeWhole of the whole file on one GPU. */
int sla_hip_shard_scan(struct SLAEncoder* encoder, const int32_t* d_pcm, uint64_t plane_stride, uint32_t num_samples,
                       uint32_t* or_word, uint64_t* nz_mask /* host, ceil(num_samples / 64) words */);
/* Steps 1-3 without the mask when the file has no silence (the usual case): the scan only brings home the OR word and
 * the number of all-zero 64-sample mask words of the piece; a silence run moves a super-frame start only when it is at
 * least 2048 samples long, so if NO rank counts an all-zero word the hop is plain (nz_mask = NULL below) and the
 * ranks all-gather 12 bytes each (OR word as two int32 halves + the count) instead of N/8 in total.  Otherwise fall back to sla_hip_shard_scan + the mask. */
int sla_hip_shard_scan_counts(struct SLAEncoder* encoder, const int32_t* d_pcm, uint64_t plane_stride, uint32_t num_samples,
                              uint32_t* or_word, uint32_t* zero_mask_words);
int sla_hip_shard_bounds(uint32_t num_samples, uint32_t max_num_block_samples, const uint64_t* nz_mask /* NULL: no silence */,
                         uint32_t world, uint32_t* bounds /* world + 1 entries */);
int sla_hip_shard_analyze(struct SLAEncoder* encoder, const int32_t* d_pcm, uint64_t plane_stride, uint32_t num_samples,
                          uint32_t file_or_word, float* timing_ms);
/* sla_hip_shard_analyze when the counts of step 1 showed no all-zero mask word anywhere in the file (and its OR word is
 * not 0): nothing the range's own prepass could find, so it is skipped (one kernel and one host wait per call less).
 * The caller vouches for the counts; a range WITH silence analysed through this call gives a valid but different file. */
int sla_hip_shard_analyze_no_silence(struct SLAEncoder* encoder, const int32_t* d_pcm, uint64_t plane_stride, uint32_t num_samples,
                                     uint32_t file_or_word, float* timing_ms);
int sla_hip_shard_header(const uint8_t* const* shard_headers /* world x 43 bytes */, uint32_t world, uint8_t* data, uint32_t data_size);

/* Device pointers of the last analysis (for RCCL gathers / tests). */
const int32_t* sla_hip_final_residual(const struct SLAEncoder* encoder, uint64_t* plane_stride);
const int32_t* sla_hip_lattice_residual(const struct SLAEncoder* encoder, uint64_t* plane_stride);

/* Make the analysis write its residual planes into caller-owned device memory ([C][plane_stride]
 * int32 each; plane_stride must equal the one later passed to sla_hip_analyze_device).  Used when
 * the planes feed a collective (RCCL all-gather of the residual stream).  NULL, NULL unbinds. */
int sla_hip_bind_residual_planes(struct SLAEncoder* encoder, int32_t* d_lattice, int32_t* d_final,
                                 uint64_t plane_stride);

/* Copy the last analysis into caller arrays. */
int sla_hip_get_trace(struct SLAEncoder* encoder, sla_hip_trace* trace);

/* Options of one encoder handle, by name.  A handle starts with the defaults below; nothing is read from the environment
 * (SLA_HIP_TRACE=1 alone, at SLAEncoder_Create: a host-side timeline of every analysis on stderr).
 * Layout knobs: "lpc_pack", "lpc_threads" (256 / 512), "lpc_tile" (24 / 48 / 0 = automatic), "tail_waves" (waves per tail
 * workgroup, 1..4, 0 = 4), "tail_taps" (k_tailk: taps of each history per lane, 1 / 2 / 4, 0 = by the number of jobs), "chunks"
 * (pipeline chunks, 1..8), "threads" (host pool; default min(6, CPUs of the process): a one-process-per-GPU launcher that
 * shares few cores between its ranks sets it), "rice_lanes" (Rice parameter walk of the device pack: 0 = by the number of
 * jobs, 1 = one lane per job, 2 = two-lane pipeline), "lattice_plain" (1: every lattice stage in the wrapping
 * four-instruction form).
 * Route switches -- every route gives the same bytes; tests force the slower exact ones through these: "search_exact" (0: no
 * tile-sum search), "exact_bits" (log2 of the tile-sum energy limit, 1..53), "cert_safety" (safety factor of the certificate
 * for windows over that limit, default 64; 0: no certificate, such windows are rerun as serial chains), "device_plan" (0:
 * partitions decided on the host), "block_cert" (0: every chosen block through the exact chain kernel; 1 = default: the
 * certified route of sla_hip_launch_lpc_blocks_cert), "block_cert_safety" (default 16), "cert_audit" (N > 0: every N-th
 * certified pair is re-analysed by the exact kernels and compared, a difference fails the call; default 0), "plan_margin",
 * "lpc_blocks_chains", "fuse_lattice", "device_ltm" (0: long-term pitch + taps solved on the host threads from the downloaded
 * autocorrelations, one tail launch per pipeline chunk), "single_tail" (0: one tail launch per pipeline chunk instead of one
 * for the file), "first_chunk" (1/1000 of the super-frames in pipeline chunk 0; 0: built-in shares), "alt_streams" (block
 * stages of odd and even pipeline chunks on two streams: 0 never, 1 / 2 = default: whenever the file is cut into chunks),
 * "device_expand" (1 = default: block tables of certified partitions written on the device, sla_hip_launch_expand, the
 * host's copy following under the kernels; 0: host tables first), "expand_silence" (1 = default: input with silence takes
 * the device tables too, sla_hip_launch_expand_masked; 0: host tables for such input), "table_cache" (1 = default: the search tables of a file --
 * or batch -- without silence are kept for the next one of the same layout and parameters), "prelaunch" (1 = default: short
 * files queue the certified block kernels together with the searches, sized for the most groups there can be, the kernels
 * reading the number from the device), "one_stream" (1: a one-chunk file keeps search, block stage and tail on one stream;
 * measured slower, default 0), "upload24" (1 = default: pageable input of 17..24 significant bits crosses the bus as three
 * bytes per sample; DESIGN section 7 has the A/B).
 * "ltm_int" (1 = default: the certified long-term stage takes its autocorrelation from exact integer sums on the int8
 * matrix pipe, k_ltm_acf_int; 0: from the FMA transform k_ltm_acf_fast.  Same bytes either way; every route that reaches
 * sla_hip_launch_ltm_cert_x honours it, worker lanes included).
 * "verify" (0 = default, 1): every call that packs on the device (sla_hip_pack_device, SLAEncoder_EncodeWhole plain and
 * streamed, sla_hip_encode_batch, sla_hip_encode_batch_device, sla_hip_encode_batch_resident, sla_hip_pack_resident)
 * decodes the finished block bytes on the device with the decoder's kernels, while they cross the bus (the resident calls:
 * before they are emitted), and compares the result with the source planes; a file whose bytes do not
 * decode back to its samples gets SLA_APIRESULT_NG (output_size 0 in a batch).  See sla_hip_last_verify; DESIGN section 2d.
 * "silence_runs" (0 = default: off; 1..65536: capacity of the list): input with silence no longer brings the prepass mask
 * (num_samples / 8 bytes, and a second wait) to the host: sla_hip_launch_zero_runs lists the zero runs that can matter
 * behind the prepass, count and list (8 + 8 x capacity bytes) come home in the prepass's own wait, and the super-frame hop and
 * the block types are decided from the list.  More runs than the capacity: the mask route, as with 0.  Same bytes either way.
 * Covers sla_hip_analyze_device / SLAEncoder_EncodeWhole (not streamed), sla_hip_encode_batch (lanes included),
 * sla_hip_encode_batch_device and sla_hip_analyze_batch_device; the pieces of a streamed file, the sla_hip_shard_* calls and
 * SLAEncoder_EncodeBlock keep the mask.  See sla_hip_last_silence; DESIGN section 2e.
 * "search_early" (1 = default, 0): a single file whose predecessor on this handle had no silence starts its whole search
 * chain (tile sums, certificate, plan, block tables) BESIDE the prepass, on another stream, instead of behind the host's look
 * at the prepass result: the chain reads offset_lshift from a device word the prepass stores, and a prepass that finds
 * silence (or an OR word of 0) raises a device flag at which every kernel of the chain returns at once; the host then
 * launches the search again with the right tables.  Files of any length.  0: the search follows the prepass (short files:
 * on the guess "like the last file").  Same bytes either way.  Batches, the sla_hip_shard_* calls and the pieces of a
 * streamed file are not affected.  See sla_hip_launch_prepass_early, sla_hip_last_search_early; DESIGN section 2.
 * "early_prepass_groups" (0 = default: three per two compute units; 1..2^20): most workgroups of the prepass that runs beside
 * such a search (sla_hip_launch_prepass_early's max_workgroups; a value of at least the file's 4096-sample tiles is "no cap").
 * SLAEncoder_EncodeWhole of long files: "stream" (0: never streamed), "stream_piece" (samples per piece, all channels
 * together; default 32 Mi; a file of fewer than two pieces is not streamed), "stream_lanes" (worker lanes, 1..6, default 6; pieces are handed to whichever lane is free),
 * "batch_lanes" (sla_hip_encode_batch: a batch of at least 8 files and 16 Mi samples is dealt out in groups of consecutive files to
 * that many worker lanes, uploads taking turns, everything behind them overlapping; 1..6, default 4; 1 = the batch in one piece).
 * After a streamed call the handle holds no analysis tables: sla_hip_get_trace / sla_hip_pack / sla_hip_final_residual answer
 * SLA_APIRESULT_PARAMETER_NOT_SET (NULL).
 * Returns SLA_APIRESULT_INVALID_ARGUMENT for an unknown name or a value out of range. */
int sla_hip_encoder_set_option(struct SLAEncoder* encoder, const char* name, double value);

/* Name of the device the library bound to ("" when none). */
const char* sla_hip_device_name(void);

/* The 12 floats of the last analysis (sla_hip_analyze_device or SLAEncoder_EncodeWhole/Block). */
int sla_hip_last_timing(const struct SLAEncoder* encoder, float* timing_ms);

/* 6 counters of the last analysis: search groups rerun as serial chains; super-frames whose partition the host
 * had to decide (device plan not certified); 1 if the search ran on tile sums; 1 if the device plan is enabled;
 * k_tail launches (1: one for the file, else one per pipeline chunk); 1 if pitch + taps were solved on the device. */
int sla_hip_last_counters(const struct SLAEncoder* encoder, uint32_t* counters);

/* 2 counters of the last analysis: 1 if the block stage took the certified route (sla_hip_launch_lpc_blocks_cert);
 * (block, channel) pairs its certificate handed to the exact chain kernels. */
int sla_hip_last_block_cert(const struct SLAEncoder* encoder, uint32_t* counters);
/* 2 counters of the last analysis under option "cert_audit": certified pairs the exact kernels re-analysed and found equal;
 * pairs they found DIFFERENT (the analysis that saw one returned SLA_APIRESULT_NG). */
int sla_hip_last_cert_audit(const struct SLAEncoder* encoder, uint32_t* counters);
/* 5 words of the last analysis' certified long-term stage (option ltm_cert, default 1; device_ltm = 1 only): jobs,
 * certified, sent through the exact kernels (fallback), audited jobs found equal / different (cert_audit; also summed
 * into sla_hip_last_cert_audit, and like there an analysis that saw a different one returns SLA_APIRESULT_NG).  All zero
 * when the stage ran the exact route.  A batch dealt out to worker lanes sums its lanes' counters into this handle; the
 * pieces of a streamed file (option stream) run on lanes whose counters are not collected: the counters then describe the
 * handle's own last analysis only. */
int sla_hip_last_ltm_cert(const struct SLAEncoder* encoder, uint32_t* counters);

/* Option "verify": 5 counters of the last call that packed on the device -- sample-channels compared (channels x block
 * samples of the delivered files), sample-channels that differed, the first differing position ((sample << 3) | channel,
 * the sample counted in the planes of the pass that saw it; ~0 when none differed), blocks decoded, bad blocks (type,
 * size, overrun or CRC16 not what the packer laid out).  All zero when that call did not verify.  A batch's passes and
 * worker lanes, and the pieces of a streamed file, are summed (the first position: the smallest).
 * The check proves that the delivered block bytes decode, with this library's decoder kernels, to the source planes.  It
 * does not prove identity with the reference encoder's bytes (option "cert_audit" and the tests cover that) and does not
 * look at the 43-byte file header, which the host writes after the download. */
int sla_hip_last_verify(const struct SLAEncoder* encoder, uint64_t counters[5]);
/* The same pass on demand, against caller-given planes (planar int32, left-justified, [C][plane_stride], sample 0 = the
 * file's sample 0): the image that the handle's last sla_hip_pack_device -- or SLAEncoder_EncodeWhole that was not
 * streamed -- left on the device is decoded and compared with d_pcm; counters as above.  Works with option "verify" on or
 * off and leaves sla_hip_last_verify alone.  Returns 0 when the pass ran, whatever it found (the verdict is in the
 * counters); SLA_APIRESULT_PARAMETER_NOT_SET when the handle holds no such image (before any pack, after a batch, a
 * streamed call, a new analysis or new parameters); SLA_APIRESULT_INVALID_ARGUMENT for NULL arguments or planes that are
 * not device memory of the handle's device covering [C][num_samples]. */
int sla_hip_verify_last_image(struct SLAEncoder* encoder, const int32_t* d_pcm, uint64_t plane_stride, uint64_t counters[5]);

/* Option "silence_runs": 4 counters of the last analysis (or batch call) -- the route: 0 = nothing silent was found and no mask
 * was needed, 1 = the tables came from the device's run list, 2 = the mask was downloaded (option off, or the list
 * overflowed); zero runs the device found (0 with the option off); the capacity of the list; mask bytes downloaded beyond
 * the fixed tail words of a single file.  A batch's passes and worker lanes are summed: the route is the maximum, runs and
 * bytes add up. */
int sla_hip_last_silence(const struct SLAEncoder* encoder, uint32_t counters[4]);

/* 4 counters: pipeline chunks of the last analysis whose block stage was launched from device-written tables
 * (sla_hip_launch_expand; option "device_expand"), its pipeline chunks in all; since the handle was created: the analyses
 * that found their search tables kept from the file before (same length and parameters, no silence; option
 * "table_cache"), and the analyses whose searches were launched before the host had seen the prepass result -- on the guess
 * that the file is like the last one -- and whose prepass then said otherwise: silence, or another OR word.  (With option
 * "search_early" another OR word costs nothing -- the chain reads the shift from the device -- but is still counted here;
 * the starts that were really thrown away are sla_hip_last_search_early's.) */
int sla_hip_last_expand(const struct SLAEncoder* encoder, uint32_t* counters);

/* Option "search_early", 4 counters: 1 if the last analysis started its search beside the prepass; since the handle was
 * created: the analyses that did, and those among them whose start was cancelled (the prepass found silence, an OR word of
 * 0 or samples wider than declared, or the host found the file's short last super-frame silent) and whose search went out
 * a second time; 0 (reserved). */
int sla_hip_last_search_early(const struct SLAEncoder* encoder, uint32_t counters[4]);

/* 4 floats [ms]: execution time of k_lpc_blocks, k_lattice, k_ltm_acf, k_tail in the last analysis, summed over
 * its launches and measured ON the device (first wave in to last wave out, constant 100 MHz clock) -- what
 * rocprofv3 --kernel-trace reports, without the time a launch spends queued behind kernels of other streams
 * that a pair of stream events includes. */
int sla_hip_last_kernel_ms(const struct SLAEncoder* encoder, float* kernel_ms);

#ifdef __cplusplus
}
#endif

#endif /* SLA_HIP_H_INCLUDED */
