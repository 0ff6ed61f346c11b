/*
 * sla_internal.h -- declarations shared by the C host side of libsla_hip.so.
 * Host code is plain C (the reference is C89/C99); device code lives in
 * sla_kernels.hip behind the launchers of include/sla_hip.h.
 */
#ifndef SLA_INTERNAL_H_INCLUDED
#define SLA_INTERNAL_H_INCLUDED

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <stddef.h>
#include <stdint.h>

#include "SLA.h"
#include "SLAEncoder.h"
#include "sla_hip.h"

/* format constants (reference src/include/private/SLAInternal.h:6-38) */
#define SLAI_MAX_CHANNELS         8
#define SLAI_SYNC_CODE            0xFFFFu
#define SLAI_LTM_MAX_PERIOD       256u
#define SLAI_LTM_MIN_PITCH        3u
#define SLAI_LTM_PERIOD_BITS      10u
#define SLAI_MIN_BLOCK            2048u
#define SLAI_SEARCH_DELTA         1024u
#define SLAI_RICE_PARAMS          2u
#define SLAI_RICE_LOW_THRESHOLD   8u
#define SLAI_QUOT_THRESHOLD       16u
#define SLAI_PATH_PENALTY         300.0
#define SLAI_EST_BLOCK_HEADER     50.0
#define SLAI_RAW_THRESHOLD        0.95f
#define SLAI_BIG_WEIGHT           ((double)(1UL << 24))
#define SLAI_HDR_CRC_START        10
#define SLAI_BLK_CRC_START        8
#define SLAI_MAX_ORDER            255
#define SLAI_MAX_TAPS             5
#define SLAI_STREAM_LANES         6       /* worker lanes of a streamed SLAEncoder_EncodeWhole, at most */
#define SLAI_MAX_NODES            66      /* 65535 / 1024 + 2 */
enum { SLAI_BLK_COMPRESS = 0, SLAI_BLK_SILENT = 1, SLAI_BLK_RAW = 2 };

/* ---- sla_plan.c: host-side decisions fed by device results ---------------- */
int      slai_make_window(SLAWindowFunctionType type, double* w, uint32_t n);
double   slai_code_length(double sumsq, uint32_t n, uint32_t bps, const double* parcor, uint32_t order);
int      slai_shortest_path(const double* adj, uint32_t nodes, uint32_t* path);
int      slai_host_check(void);       /* 0: long double / double arithmetic of this host is the reference build's */
uint32_t slai_zero_run(const uint64_t* nz_mask, uint64_t from, uint64_t limit);
int      slai_range_is_zero(const uint64_t* nz_mask, uint64_t from, uint64_t count);
/* where the host's questions about silence are answered from: the mask (by_runs == 0; nz == NULL: nothing is silent) or the
 * device's run list, sorted by start (slai_sort_runs) */
typedef struct slai_silence { const uint64_t* nz; const sla_hip_zero_run* runs; uint32_t num_runs; int by_runs; } slai_silence;
void     slai_sort_runs(sla_hip_zero_run* runs, uint32_t num_runs);
uint32_t slai_runs_zero_run(const sla_hip_zero_run* runs, uint32_t num_runs, uint64_t from, uint64_t limit);
uint32_t slai_silence_run(const slai_silence* s, uint64_t from, uint64_t limit);      /* s == NULL: nothing is silent */
int      slai_silence_is_zero(const slai_silence* s, uint64_t from, uint64_t count);

/* ---- sla_ltm.c: long-term predictor analysis ------------------------------ */
typedef struct slai_fft_plan slai_fft_plan;
slai_fft_plan* slai_fft_plan_create(uint32_t fft_size);
void           slai_fft_plan_destroy(slai_fft_plan* plan);
uint32_t       slai_fft_plan_size(const slai_fft_plan* plan);
void           slai_fft_plan_export(const slai_fft_plan* plan, double* out /* 3*fft_size doubles */);
/* pitch + taps from the device's compact autocorrelation record; returns 0 ok, 4 analysis failed */
int  slai_ltm_solve(const double* rec, uint32_t ntaps, uint32_t* pitch, double* coef);
#define SLAI_LTM_ACF_HEAD SLA_HIP_ACF_RECORD

/* ---- sla_pack.c: bit-serial block writer ---------------------------------- */
typedef struct slai_block_params {
  uint32_t num_samples;
  uint32_t type;
  uint32_t num_channels, order, ntaps, bps, lshift, mid_side;
  const int32_t*  code;        /* [C][order+1] */
  const uint32_t* rshift;      /* [C] */
  const uint32_t* pitch;       /* [C] */
  const int32_t*  ltm_q;       /* [C][SLAI_MAX_TAPS] */
  const uint32_t* rice_init;   /* [C] */
  const int32_t*  res[SLAI_MAX_CHANNELS];   /* final residual (COMPRESS) or right-justified PCM (RAW) */
} slai_block_params;
/* returns bytes written, or 0 when `cap` is too small */
uint32_t slai_pack_block(const slai_block_params* bp, uint8_t* out, uint32_t cap);
uint32_t slai_pack_header(const slai_block_params* bp, uint8_t* out, uint32_t cap);
void     slai_coding_mode(const uint32_t* rice_init, uint32_t num_channels, uint32_t* golomb_m);
uint32_t slai_crc16(const uint8_t* data, size_t n);
int      slai_write_header(const struct SLAHeaderInfo* h, uint8_t* data, uint32_t data_size);

/* ---- sla_verify.c: tables of the encoder's verification pass (no device calls) --------- */
typedef struct slai_verify_seg {
  uint64_t img_off;      /* where the file (43-byte header + blocks, or bare blocks) starts in the device image */
  uint64_t img_bytes;    /* its size there */
  int      deliver;      /* 0: the file is not delivered (e.g. its buffer is too small): its blocks are left out */
} slai_verify_seg;
/* From the pack table (blocks ascending in the image) and the files of the pass (ascending, back to back; files without
 * blocks allowed anywhere): the decoder's block table, every block's end of stream (the end of its file), what the parser
 * must find, and the block's file index -- for the blocks of delivered files only, in order.  Returns the number of blocks
 * written (<= num_blocks: the arrays' capacity); *compared = channels x samples of those blocks, *max_block_samples their
 * longest. */
uint32_t slai_verify_tables(const sla_hip_pack_block* pb, uint32_t num_blocks, const slai_verify_seg* segs, uint32_t num_segs,
                            uint32_t num_channels, sla_hip_dec_block* blocks, uint64_t* block_end,
                            sla_hip_verify_expect* expect, uint32_t* seg_of_block, uint64_t* compared,
                            uint32_t* max_block_samples);

/* ---- sla_dec_plan.c: the pass arithmetic of the batch decoder (no device calls) --------- */
#define SLAI_DEC_BATCH_ALIGN 64u         /* samples: every file's plane region starts on a 256-byte boundary */
#define SLAI_DEC_WIDE_MAX    8u          /* resident files of one call that are walked wide, at most */
typedef struct slai_dec_format { uint32_t C, total, bps, lshift, order, ntaps, lms, ms; } slai_dec_format;
typedef struct slai_dec_file {
  uint32_t        item;       /* index into the caller's items */
  slai_dec_format f;          /* from its header */
  uint32_t        bytes;      /* what a pass image holds of it: the whole stream, or the byte range of a window */
  uint32_t        first, nb;  /* its blocks: rows [first, first + nb) of the host tables, positions in the file */
  SLAApiResult    walk_err;
  uint32_t        extent;     /* samples per channel its blocks write */
  int             alone;      /* decoded on its own, in no pass */
  int             wide;       /* resident: its chain is walked by sla_hip_launch_dec_walk_wide, not on a lane */
  uint64_t        img_off;    /* its bytes in the pass image */
  uint64_t        plane_off;  /* its region in the pass planes */
} slai_dec_file;              /* 80 bytes */
int      slai_dec_same_launch(const slai_dec_format* a, const slai_dec_format* b);
int      slai_dec_file_cmp(const void* a, const void* b);
uint32_t slai_dec_cut(const slai_dec_file* files, uint32_t p0, uint32_t n, uint64_t cap_samples, uint64_t cap_bytes);
void     slai_dec_layout(slai_dec_file* files, uint32_t nf, uint64_t* img_bytes, uint64_t* span, uint32_t* nb);
uint32_t slai_dec_wide_capacity(uint32_t option, uint32_t data_size);
uint32_t slai_dec_pick_wide(const slai_dec_file* files, uint32_t nf, uint32_t threshold, uint32_t pick[SLAI_DEC_WIDE_MAX]);

/* ---- sla_dec_index.c: the block index of a stream (sla_hip_index; no device calls) --------- */
#define SLAI_INDEX_HEAD 44u              /* bytes kept of a stream's head: the 43 of the header, padded */
struct sla_hip_index {
  sla_hip_index_summary info;
  uint8_t              head[SLAI_INDEX_HEAD];
  sla_hip_index_block* rows;             /* info.num_blocks of them, in the same allocation */
};
/* an index of `head_bytes` (<= 43) header bytes of a stream of data_size bytes with room for num_blocks rows: info's
 * data_size, header_bytes, header_result and header are set, the rest is zero; NULL when memory is short */
sla_hip_index* slai_index_new(const uint8_t* head, uint32_t head_bytes, uint32_t data_size, uint32_t num_blocks);
/* 1 when the header was delivered, so that a chain is walked */
int      slai_index_has_header(const sla_hip_index* index);
/* The planned rows of the window [start, start + length) (clipped to `total`) of an index: k_dec_walk_window's rules over
 * the index's rows instead of the bytes.  *row0 / *nrows: the run of index rows from the first kept one to the last (rows
 * of no samples inside it are passed over, *kept counts the others); *stop: OK when the window's end was reached, BUF at a
 * block of more than max_block_samples samples, else -- the rows ran out -- the index's stop code (DATA when that is OK). */
void     slai_index_window(const sla_hip_index* index, uint32_t total, uint32_t start, uint32_t length, uint32_t max_block_samples,
                           uint32_t* row0, uint32_t* nrows, uint32_t* kept, uint32_t* stop);

/* ---- sla_splice.c: the layout rule of sla_hip_splice_resident (no device calls) --------- */
#define SLAI_SPLICE_VERBATIM     0u      /* the block's bytes as they are */
#define SLAI_SPLICE_SILENT       1u      /* an 11-byte SILENT block of the kept samples */
#define SLAI_SPLICE_RAW          2u      /* a RAW block of the kept samples */
#define SLAI_SPLICE_SILENT_BYTES 11u
/* called for every emitted block in output order: segment, its index row, the kept samples [first, first + n) of the row,
 * the kind, and where the block lies in the output stream */
typedef void (*slai_splice_visit)(void* ctx, uint32_t segment, const sla_hip_index_block* row, uint32_t first, uint32_t n,
                                  uint32_t kind, uint64_t out_off, uint32_t out_len);
/* sla_hip_splice_plan with a visitor (NULL: none); on a refusal *layout is zero and the blocks visited so far are void */
int      slai_splice_walk(const sla_hip_splice_item* item, sla_hip_splice_layout* layout, slai_splice_visit visit, void* ctx);

/* ---- sla_decoder.c: caller-owned device memory of the batch calls --------- */
/* 1 when [0, C) x [0, n) of esize-byte elements at p (element (c, i) at c * channel_stride + i * sample_stride) is aligned,
 * its byte extent does not overflow, the runtime reports p as device memory (of `device` when >= 0) and the region lies
 * inside p's allocation.  NULL p, zero strides: the caller's checks. */
int      slai_device_region_ok(const void* p, uint32_t C, uint32_t n, uint64_t channel_stride, uint64_t sample_stride,
                               uint64_t esize, int device);

/* ---- sla_wav.c: the RIFF/WAVE reader as a scan over windows of the file (no device calls) --------- */
/* slai_wav_scan_step reads the window [win_off, win_off + win_len) of a file of file_size bytes and walks the chunk chain
 * from scan->pos on.  It returns the SLAApiResult of sla_hip_wav_parse (OK: scan->info is filled), or SLAI_WAV_NEED_MORE
 * when the next chunk header (8 bytes, up to 48 for `fmt `) is inside the file but not inside the window: call again with
 * a window that starts at scan->pos.  A window that starts at scan->pos and holds min(4096, what is left) bytes always
 * makes progress. */
#define SLAI_WAV_NEED_MORE (-1)
typedef struct slai_wav_scan {
  uint64_t pos;            /* the next chunk header (0: the signature has not been read) */
  uint32_t have_fmt;
  sla_hip_wav_info info;
} slai_wav_scan;
void     slai_wav_scan_init(slai_wav_scan* scan);
int      slai_wav_scan_step(slai_wav_scan* scan, const uint8_t* win, uint64_t win_off, uint32_t win_len, uint64_t file_size);

#endif
