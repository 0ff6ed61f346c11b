/*
 * sla_decoder.c -- host side of the whole-file decoder (include/SLADecoder.h).
 *
 * The host reads 10 bytes per block (sync code, size field, sample count) to lay the block chain out as a
 * table; every other byte of the stream is consumed by the kernels of sla_decode.hip, all blocks at once.
 * Results are then examined in file order so that the first failing block decides the return code exactly
 * as the reference's block-by-block loop does (reference src/SLADecoder.c:660-732).
 * There is no CPU decode path in this file: without a HIP device SLADecoder_Create returns NULL.
 */
#include "sla_internal.h"
#include "SLADecoder.h"

#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define DEC_MAX_BLOCK_SAMPLES 65535u     /* the format's: a 16-bit field */
#define DEC_MIN_BLOCK_HEADER  11u        /* SLA_MINIMUM_BLOCK_HEADER_SIZE, reference src/include/private/SLAInternal.h:35 */
#define STATUS_WAVE_FORMAT    1u
#define STATUS_ENCODE_PARAM   2u
/* Resident files of at least this many bytes have their block chain walked by sla_hip_launch_dec_walk_wide (0 = none).
 * The smallest rung of the ladder of tests/tools/bench_walk_wide.py (0.25, 1, 4, 16, 82 MB) at which the wide walk took at
 * most half the lane walk's time on an MI355X (profiles/walk_wide.json: 0.075 ms against 0.58 ms; at 4 MB 0.078 against
 * 0.139).  Half and not break-even: in a batch a file's lane walk runs beside the others', wide launches add up. */
#define DEC_WIDE_WALK_DEFAULT 16000000u

typedef struct { void* ptr; size_t cap; } dbuf_t;
typedef struct { void* ptr; size_t cap; } hbuf_t;

struct SLADecoder {
  struct SLADecoderConfig   cfg;
  struct SLAWaveFormat      wave_format;
  struct SLAEncodeParameter encode_param;
  uint32_t                  status_flag;
  hipStream_t               stream;
  hipEvent_t                ev[2];
  hipEvent_t                ev_order;                   /* sla_hip_decode_batch_device: the caller's stream, recorded */
  dbuf_t                    d_image, d_planes, d_blocks, d_info, d_chan, d_kint;
  dbuf_t                    d_ftab, d_out;              /* sla_hip_decode_batch: file table, packed samples */
  dbuf_t                    d_wav; hbuf_t h_wav;        /* the WAV calls: the emit table */
  hbuf_t                    h_img, h_ptab, h_out;       /* sla_hip_decode_batch: page-locked staging */
  dbuf_t                    d_src, d_wres, d_crcf;      /* sla_hip_decode_batch_resident: gather / walk tables, walk results, CRC fields */
  hbuf_t                    h_src, h_hdr;               /* the same: tables and results, the headers brought home */
  hipEvent_t                ev_src[3];                  /* the same: around a pass's gather and walk */
  sla_hip_dec_block*        h_blocks;
  sla_hip_dec_info*         h_info;
  uint32_t*                 h_crcf;                     /* every block's stored CRC field, next to h_blocks */
  uint32_t                  h_cap;
  float                     timing[6];
  uint64_t                  win_stats[4];               /* sla_hip_decode_windows_resident: sla_hip_decoder_last_window_stats */
  dbuf_t                    d_wide; hbuf_t h_wide;      /* the wide walk of long resident files: its scratch; info words and rerun results home */
  uint32_t                  wide_walk, wide_nodes;      /* options "wide_walk" (bytes, 0 = off) and "wide_walk_nodes" (0 = by file size) */
  uint64_t                  walk_stats[4];              /* sla_hip_decoder_last_walk */
  /* sla_hip_decode_windows_indexed: a ring of page-locked staging slots for a pass's tables, each guarded by an event that
   * the handle's stream passes once the slot's upload is done; the closing event; work queued and not known to have run */
  struct { hbuf_t h; hipEvent_t ev; int busy; } q_slot[SLA_HIP_DEC_QUEUE_SLOTS];
  uint32_t                  q_next;
  hipEvent_t                ev_close;
  int                       queued;
  dbuf_t                    d_qtab;                     /* the same: judge and emit table of a pass */
  dbuf_t                    d_splice; hbuf_t h_splice;  /* sla_hip_splice_resident: a pass's judge, check and verdict tables; its staging */
};

/* Every entry point but sla_hip_decode_windows_indexed opens with this: what that call left queued on the handle's stream
 * runs to its end before host staging that no event guards is written again. */
static int drain(struct SLADecoder* d)
{
  if (!d->queued) { return 0; }
  d->queued = 0;
  return (hipStreamSynchronize(d->stream) == hipSuccess) ? 0 : -1;
}

static double now_ms(void)
{
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

static int dbuf_reserve(dbuf_t* b, size_t bytes)
{
  if (bytes <= b->cap) { return 0; }
  /* (work that sla_hip_decode_windows_indexed left queued may still use the old buffer: hipFree waits for the device) */
  if (b->ptr != NULL) { (void)hipFree(b->ptr); b->ptr = NULL; b->cap = 0; }
  bytes += bytes / 4 + 256;
  if (hipMalloc(&b->ptr, bytes) != hipSuccess) { b->ptr = NULL; return -1; }
  b->cap = bytes;
  return 0;
}
static void dbuf_free(dbuf_t* b) { if (b->ptr != NULL) { (void)hipFree(b->ptr); } b->ptr = NULL; b->cap = 0; }
static int hbuf_reserve(hbuf_t* b, size_t bytes)
{
  if (bytes <= b->cap) { return 0; }
  if (b->ptr != NULL) { (void)hipHostFree(b->ptr); b->ptr = NULL; b->cap = 0; }
  bytes += bytes / 4 + 256;
  if (hipHostMalloc(&b->ptr, bytes, hipHostMallocDefault) != hipSuccess) { b->ptr = NULL; return -1; }
  b->cap = bytes;
  return 0;
}
static void hbuf_free(hbuf_t* b) { if (b->ptr != NULL) { (void)hipHostFree(b->ptr); } b->ptr = NULL; b->cap = 0; }

/* the time between two recorded events that the stream has passed (0 when the runtime cannot tell), added to *acc */
static float ev_ms(hipEvent_t a, hipEvent_t b) { float ms = 0.0f; return (hipEventElapsedTime(&ms, a, b) == hipSuccess) ? ms : 0.0f; }
#define ev_add_ms(acc, a, b) (*(acc) += ev_ms(a, b))

static uint32_t rd_be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }
static uint32_t rd_be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

/* reference src/SLADecoder.c:171-251 */
SLAApiResult SLADecoder_DecodeHeader(const uint8_t* data, uint32_t data_size, struct SLAHeaderInfo* header_info)
{
  struct SLAHeaderInfo h;
  SLAApiResult ret = SLA_APIRESULT_OK;
  if (data == NULL || header_info == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (data_size < SLA_HEADER_SIZE) { return SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; }
  if (data[0] != 'S' || data[1] != 'L' || data[2] != '*' || data[3] != 1) { return SLA_APIRESULT_INVALID_HEADER_FORMAT; }
  if (rd_be16(data + 8) != slai_crc16(data + SLAI_HDR_CRC_START, SLA_HEADER_SIZE - SLAI_HDR_CRC_START)) {
    ret = SLA_APIRESULT_DETECT_DATA_CORRUPTION;          /* reported, but the fields are still delivered */
  }
  if (rd_be32(data + 10) != SLA_FORMAT_VERSION) { return SLA_APIRESULT_INVALID_HEADER_FORMAT; }
  memset(&h, 0, sizeof(h));
  h.wave_format.num_channels          = data[14];
  h.num_samples                       = rd_be32(data + 15);
  h.wave_format.sampling_rate         = rd_be32(data + 19);
  h.wave_format.bit_per_sample        = data[23];
  h.wave_format.offset_lshift         = data[24];
  h.encode_param.parcor_order         = data[25];
  h.encode_param.longterm_order       = data[26];
  h.encode_param.lms_order_per_filter = data[27];
  h.encode_param.ch_process_method    = (SLAChannelProcessMethod)data[28];
  h.num_blocks                        = rd_be32(data + 29);
  h.encode_param.max_num_block_samples = rd_be16(data + 33);
  h.max_block_size                    = rd_be32(data + 35);
  h.max_bit_per_second                = rd_be32(data + 39);
  *header_info = h;
  return ret;
}

struct SLADecoder* SLADecoder_Create(const struct SLADecoderConfig* config)
{
  struct SLADecoder* d;
  int ndev = 0;
  if (config == NULL) { return NULL; }
  if (config->max_num_channels == 0 || config->max_num_channels > SLAI_MAX_CHANNELS
      || config->max_num_block_samples > DEC_MAX_BLOCK_SAMPLES || config->max_parcor_order > SLAI_MAX_ORDER
      || config->max_longterm_order > SLAI_MAX_TAPS) { return NULL; }
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    fprintf(stderr, "libsla_hip: no HIP device available -- the decode path has no CPU fallback\n");
    return NULL;
  }
  d = (struct SLADecoder*)calloc(1, sizeof(*d));
  if (d == NULL) { return NULL; }
  d->cfg = *config;
  d->wide_walk = DEC_WIDE_WALK_DEFAULT;
  if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) { free(d); return NULL; }
  if (hipEventCreate(&d->ev[0]) != hipSuccess || hipEventCreate(&d->ev[1]) != hipSuccess) { (void)hipStreamDestroy(d->stream); free(d); return NULL; }
  return d;
}

void SLADecoder_Destroy(struct SLADecoder* d)
{
  if (d == NULL) { return; }
  (void)hipStreamSynchronize(d->stream);
  dbuf_free(&d->d_image); dbuf_free(&d->d_planes); dbuf_free(&d->d_blocks);
  dbuf_free(&d->d_info); dbuf_free(&d->d_chan); dbuf_free(&d->d_kint);
  dbuf_free(&d->d_ftab); dbuf_free(&d->d_out);
  dbuf_free(&d->d_wav); hbuf_free(&d->h_wav);
  hbuf_free(&d->h_img); hbuf_free(&d->h_ptab); hbuf_free(&d->h_out);
  dbuf_free(&d->d_src); dbuf_free(&d->d_wres); dbuf_free(&d->d_crcf);
  hbuf_free(&d->h_src); hbuf_free(&d->h_hdr);
  dbuf_free(&d->d_wide); hbuf_free(&d->h_wide);
  { int k; for (k = 0; k < 3; k++) { if (d->ev_src[k] != NULL) { (void)hipEventDestroy(d->ev_src[k]); } } }
  { uint32_t k; for (k = 0; k < SLA_HIP_DEC_QUEUE_SLOTS; k++) { hbuf_free(&d->q_slot[k].h); if (d->q_slot[k].ev != NULL) { (void)hipEventDestroy(d->q_slot[k].ev); } } }
  dbuf_free(&d->d_qtab);
  dbuf_free(&d->d_splice); hbuf_free(&d->h_splice);
  if (d->ev_close != NULL) { (void)hipEventDestroy(d->ev_close); }
  if (d->h_blocks != NULL) { (void)hipHostFree(d->h_blocks); }
  if (d->h_info != NULL) { (void)hipHostFree(d->h_info); }
  if (d->h_crcf != NULL) { (void)hipHostFree(d->h_crcf); }
  (void)hipEventDestroy(d->ev[0]); (void)hipEventDestroy(d->ev[1]);
  if (d->ev_order != NULL) { (void)hipEventDestroy(d->ev_order); }
  (void)hipStreamDestroy(d->stream);
  free(d);
}

SLAApiResult SLADecoder_SetWaveFormat(struct SLADecoder* d, const struct SLAWaveFormat* wave_format)
{
  if (d == NULL || wave_format == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (wave_format->num_channels > d->cfg.max_num_channels || wave_format->bit_per_sample > 32) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  d->wave_format = *wave_format;
  d->status_flag |= STATUS_WAVE_FORMAT;
  return SLA_APIRESULT_OK;
}

SLAApiResult SLADecoder_SetEncodeParameter(struct SLADecoder* d, const struct SLAEncodeParameter* ep)
{
  if (d == NULL || ep == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (ep->parcor_order > d->cfg.max_parcor_order || ep->longterm_order > d->cfg.max_longterm_order
      || ep->lms_order_per_filter > d->cfg.max_lms_order_per_filter
      || ep->max_num_block_samples > d->cfg.max_num_block_samples
      || ep->max_num_block_samples < SLAI_MIN_BLOCK) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  d->encode_param = *ep;
  d->status_flag |= STATUS_ENCODE_PARAM;
  return SLA_APIRESULT_OK;
}

static int host_tables_reserve(struct SLADecoder* d, uint32_t blocks)
{
  sla_hip_dec_block* nb = NULL;
  sla_hip_dec_info* ni = NULL;
  uint32_t* nc = NULL;
  uint32_t cap;
  if (blocks <= d->h_cap) { return 0; }
  cap = blocks + blocks / 2 + 64;
  if (hipHostMalloc((void**)&nb, sizeof(*nb) * cap, hipHostMallocDefault) != hipSuccess) { return -1; }
  if (hipHostMalloc((void**)&ni, sizeof(*ni) * cap, hipHostMallocDefault) != hipSuccess) { (void)hipHostFree(nb); return -1; }
  if (hipHostMalloc((void**)&nc, sizeof(*nc) * cap, hipHostMallocDefault) != hipSuccess) { (void)hipHostFree(nb); (void)hipHostFree(ni); return -1; }
  if (d->h_blocks != NULL) { memcpy(nb, d->h_blocks, sizeof(*nb) * d->h_cap); (void)hipHostFree(d->h_blocks); }
  if (d->h_info != NULL) { (void)hipHostFree(d->h_info); }
  if (d->h_crcf != NULL) { memcpy(nc, d->h_crcf, sizeof(*nc) * d->h_cap); (void)hipHostFree(d->h_crcf); }
  d->h_blocks = nb; d->h_info = ni; d->h_crcf = nc; d->h_cap = cap;
  return 0;
}

#define HIPCHK(call) do { if ((call) != hipSuccess) { return SLA_APIRESULT_NG; } } while (0)
#define RCCHK(call)  do { const int rc_ = (call); if (rc_ != 0) { return (rc_ > 0) ? (SLAApiResult)rc_ : SLA_APIRESULT_NG; } } while (0)

/* Walk a file's block chain from byte `off`, sample `pos` (positions in the file) and append the blocks to
 * d->h_blocks[*nb ...], their stored CRC fields to d->h_crcf[*nb ...]; *walk_err says why the walk stopped short of `total` samples.    src/SLADecoder.c:696-722
 * Returns -1 when the host table could not grow. */
static int walk_chain(struct SLADecoder* d, const uint8_t* data, uint32_t data_size, uint32_t off, uint32_t pos,
                      uint32_t total, uint32_t buffer_num_samples, uint32_t* nb, SLAApiResult* walk_err)
{
  const uint32_t cap_n = d->cfg.max_num_block_samples;
  *walk_err = SLA_APIRESULT_OK;
  while (pos < total) {
    const uint8_t* p;
    uint32_t left, bsize, n, flags = 0;
    if (off > data_size) { *walk_err = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    left = data_size - off;
    if (left < DEC_MIN_BLOCK_HEADER) { *walk_err = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    p = data + off;
    if (rd_be16(p) != SLAI_SYNC_CODE) { *walk_err = SLA_APIRESULT_FAILED_TO_FIND_SYNC_CODE; break; }
    bsize = rd_be32(p + 2) + 6u;
    n = rd_be16(p + 8);
    if (bsize > left || bsize < SLAI_BLK_CRC_START) { *walk_err = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }   /* no CRC check on a clipped block (:343) */
    if (n > buffer_num_samples - pos || n > cap_n) {
      /* the CRC of this block is still checked first (:343-352 precede :633-636): keep it, header only */
      *walk_err = SLA_APIRESULT_INSUFFICIENT_BUFFER_SIZE;
      if (d->cfg.enable_crc_check != 1) { break; }
      flags = SLA_HIP_DEC_HEADER_ONLY;
    }
    if (host_tables_reserve(d, *nb + 1) != 0) { return -1; }
    d->h_blocks[*nb].byte_off = off; d->h_blocks[*nb].byte_len = bsize; d->h_blocks[*nb].smp_off = pos;
    d->h_blocks[*nb].num_samples = n; d->h_blocks[*nb].flags = flags;
    d->h_crcf[*nb] = rd_be16(p + 6);
    (*nb)++;
    if (flags != 0) { break; }
    off += bsize; pos += n;
  }
  return 0;
}

/* Examine the decoded blocks of one file in file order: the first failure decides (*result), *done_samples counts the
 * samples of the blocks before it.  Table positions are the file's own; crc_field[i] is block i's stored CRC field (the
 * walk's, host or device).  Returns 1 when a
 * block's body did not end where its size field says: the reference continues from where its reader stopped (:715),
 * so the walk resumes at (*off, *pos). */
static int examine_blocks(const struct SLADecoder* d, const uint32_t* crc_field, const sla_hip_dec_block* blocks,
                          const sla_hip_dec_info* info, uint32_t nb, int lms_ok, SLAApiResult walk_err,
                          uint32_t* one_block_size, uint32_t* done_samples, uint32_t* off, uint32_t* pos, SLAApiResult* result)
{
  uint32_t i;
  *result = SLA_APIRESULT_OK;
  for (i = 0; i < nb; i++) {
    const sla_hip_dec_block* b = &blocks[i];
    const sla_hip_dec_info* in = &info[i];
    if (d->cfg.enable_crc_check == 1 && in->crc != crc_field[i]) { *result = SLA_APIRESULT_DETECT_DATA_CORRUPTION; return 0; }
    if (b->flags & SLA_HIP_DEC_HEADER_ONLY) { *result = walk_err; return 0; }
    if (in->type > 2) { *result = SLA_APIRESULT_INVALID_HEADER_FORMAT; return 0; }
    if (in->type == 0 && !lms_ok) { *result = SLA_APIRESULT_FAILED_TO_SYNTHESIZE; return 0; }
    *done_samples = b->smp_off + b->num_samples;
    if (one_block_size != NULL) { *one_block_size = in->used_bytes; return 0; }     /* src/SLADecoder.c:651 */
    if (in->used_bytes != b->byte_len) {
      *off = (uint32_t)b->byte_off + in->used_bytes; *pos = *done_samples;
      return 1;
    }
  }
  *result = walk_err;
  return 0;
}

/* The kernel launch parameters of a file, from its header; SLA_APIRESULT_OK when the kernels can run on it.  Sets the
 * handle's wave format and encode parameter as it goes, as the reference's DecodeWhole does. */
typedef slai_dec_format dec_format_t;

static SLAApiResult file_format(struct SLADecoder* d, const uint8_t* data, uint32_t data_size, dec_format_t* f)
{
  struct SLAHeaderInfo header;
  SLAApiResult ret;
  if ((ret = SLADecoder_DecodeHeader(data, data_size, &header)) != SLA_APIRESULT_OK) { return ret; }
  if ((ret = SLADecoder_SetWaveFormat(d, &header.wave_format)) != SLA_APIRESULT_OK) { return ret; }
  if ((ret = SLADecoder_SetEncodeParameter(d, &header.encode_param)) != SLA_APIRESULT_OK) { return ret; }
  f->C = header.wave_format.num_channels; f->total = header.num_samples;
  f->bps = header.wave_format.bit_per_sample; f->lshift = header.wave_format.offset_lshift;
  f->order = header.encode_param.parcor_order; f->ntaps = header.encode_param.longterm_order;
  f->lms = header.encode_param.lms_order_per_filter;
  f->ms = (header.encode_param.ch_process_method == SLA_CHPROCESSMETHOD_STEREO_MS) ? 1u : 0u;
  return SLA_APIRESULT_OK;
}

/* what a file with a valid header but nothing the kernels can run on returns (SLA_APIRESULT_OK and no samples for an
 * empty file), or -1 when the kernels are to run */
static int format_verdict(const dec_format_t* f)
{
  if (f->total == 0) { return SLA_APIRESULT_OK; }
  if (f->ms && f->C != 2) { return SLA_APIRESULT_INVAILD_CHPROCESSMETHOD; }                   /* src/SLADecoder.c:605-613 */
  if (f->C == 0 || f->bps == 0 || f->lshift >= f->bps) { return SLA_APIRESULT_INVALID_HEADER_FORMAT; }   /* the reference asserts (src/SLADecoder.c:541-542) */
  return -1;
}
static int lms_order_ok(uint32_t lms) { return (lms == 4 || lms == 8 || lms == 16 || lms == 32); }

/* the plane stride decode_run gives the handle's own planes */
static uint64_t run_plane_stride(uint32_t total, uint32_t buffer_num_samples)
{
  const uint64_t want = (uint64_t)total + 65535u;
  const uint64_t stride = (buffer_num_samples < want) ? buffer_num_samples : want;
  return (stride == 0) ? 1 : stride;
}

/* The decode proper.  `host_data` is always the stream in host memory (the walk reads it); the image in device
 * memory is either uploaded from it or supplied by the caller, the planes likewise are the handle's or the caller's. */
static SLAApiResult decode_run(struct SLADecoder* d, const uint8_t* data, uint32_t data_size, const uint32_t* d_image_user,
                               int32_t* d_planes_user, uint64_t stride_user, int32_t** buffer,
                               uint32_t buffer_num_samples, uint32_t* output_num_samples, uint32_t* one_block_size)
{
  /* one_block_size == NULL: a whole file (header, then blocks until header.num_samples samples are out);
   * otherwise `data` starts at a block's sync code and exactly that block is decoded with the handle's current
   * format / parameters (the streaming decoder's unit; reference SLADecoder_DecodeBlock, src/SLADecoder.c:583-657) */
  dec_format_t f;
  SLAApiResult ret, result = SLA_APIRESULT_OK;
  uint32_t C, total, order, ntaps, lms, ms, bps, lshift, cap_n;
  uint32_t off = SLA_HEADER_SIZE, pos = 0, done_samples = 0, batches = 0, ch;
  uint64_t stride;
  const uint32_t* d_image;
  int32_t* d_planes;
  int lms_ok, verdict;
  float kernel_ms = 0.0f;
  double t0 = now_ms(), t_up = 0.0, t_walk = 0.0, t1;

  if (drain(d) != 0) { return SLA_APIRESULT_NG; }
  memset(d->timing, 0, sizeof(d->timing));
  if (one_block_size == NULL) {
    if ((ret = file_format(d, data, data_size, &f)) != SLA_APIRESULT_OK) { return ret; }
  } else {
    if (!(d->status_flag & STATUS_WAVE_FORMAT) || !(d->status_flag & STATUS_ENCODE_PARAM)) { return SLA_APIRESULT_PARAMETER_NOT_SET; }
    f.C = d->wave_format.num_channels; f.bps = d->wave_format.bit_per_sample; f.lshift = d->wave_format.offset_lshift;
    f.order = d->encode_param.parcor_order; f.ntaps = d->encode_param.longterm_order; f.lms = d->encode_param.lms_order_per_filter;
    f.ms = (d->encode_param.ch_process_method == SLA_CHPROCESSMETHOD_STEREO_MS) ? 1u : 0u;
    f.total = 1;                          /* the walk stops behind the first block */
    off = 0; *one_block_size = 0;
  }
  C = f.C; total = f.total; bps = f.bps; lshift = f.lshift; order = f.order; ntaps = f.ntaps; lms = f.lms; ms = f.ms;
  cap_n = d->cfg.max_num_block_samples;
  *output_num_samples = 0;
  if ((verdict = format_verdict(&f)) >= 0) { return (SLAApiResult)verdict; }
  lms_ok = lms_order_ok(lms);

  /* the stream image on the device */
  if (d_image_user != NULL) { d_image = d_image_user; }
  else {
    const size_t padded = ((size_t)data_size + 3) & ~(size_t)3;
    if (dbuf_reserve(&d->d_image, padded + 16) != 0) { return SLA_APIRESULT_NG; }
    HIPCHK(hipMemsetAsync((uint8_t*)d->d_image.ptr + (padded - 4), 0, 4, d->stream));
    HIPCHK(hipMemcpyAsync(d->d_image.ptr, data, data_size, hipMemcpyHostToDevice, d->stream));
    d_image = (const uint32_t*)d->d_image.ptr;
  }
  if (d_planes_user != NULL) { d_planes = d_planes_user; stride = stride_user; }
  else {
    stride = run_plane_stride(total, buffer_num_samples);
    if (dbuf_reserve(&d->d_planes, (size_t)stride * C * sizeof(int32_t)) != 0) { return SLA_APIRESULT_NG; }
    d_planes = (int32_t*)d->d_planes.ptr;
  }
  t_up = now_ms() - t0;

  for (;;) {
    uint32_t nb = 0;
    SLAApiResult walk_err;
    double tw = now_ms();
    if (walk_chain(d, data, data_size, off, pos, total, buffer_num_samples, &nb, &walk_err) != 0) { return SLA_APIRESULT_NG; }
    t_walk += now_ms() - tw;
    batches++;

    /* ---- all blocks of the batch through the kernels */
    if (nb > 0) {
      if (dbuf_reserve(&d->d_blocks, sizeof(sla_hip_dec_block) * nb) != 0 || dbuf_reserve(&d->d_info, sizeof(sla_hip_dec_info) * nb) != 0
          || dbuf_reserve(&d->d_chan, sizeof(sla_hip_dec_chan) * (size_t)nb * C) != 0
          || dbuf_reserve(&d->d_kint, sizeof(int32_t) * (size_t)nb * C * (order + 1)) != 0) { return SLA_APIRESULT_NG; }
      HIPCHK(hipMemcpyAsync(d->d_blocks.ptr, d->h_blocks, sizeof(sla_hip_dec_block) * nb, hipMemcpyHostToDevice, d->stream));
      HIPCHK(hipMemsetAsync(d->d_info.ptr, 0, sizeof(sla_hip_dec_info) * nb, d->stream));
      HIPCHK(hipEventRecord(d->ev[0], d->stream));
      RCCHK(sla_hip_launch_dec_bits(d_image, data_size, (const sla_hip_dec_block*)d->d_blocks.ptr, nb, C, bps, lshift, ms, order, ntaps,
                                    d->cfg.enable_crc_check == 1, d_planes, stride, (sla_hip_dec_info*)d->d_info.ptr,
                                    (sla_hip_dec_chan*)d->d_chan.ptr, (int32_t*)d->d_kint.ptr, d->stream));
      HIPCHK(hipMemcpyAsync(d->h_info, d->d_info.ptr, sizeof(sla_hip_dec_info) * nb, hipMemcpyDeviceToHost, d->stream));
      if (lms_ok) {
        RCCHK(sla_hip_launch_dec_lms(d_planes, stride, (const sla_hip_dec_block*)d->d_blocks.ptr, (const sla_hip_dec_info*)d->d_info.ptr,
                                     nb, C, lms, d->stream));
        RCCHK(sla_hip_launch_dec_ltm(d_planes, stride, (const sla_hip_dec_block*)d->d_blocks.ptr, (const sla_hip_dec_info*)d->d_info.ptr,
                                     (const sla_hip_dec_chan*)d->d_chan.ptr, nb, C, ntaps, cap_n, d->stream));
        RCCHK(sla_hip_launch_dec_lattice(d_planes, stride, (const sla_hip_dec_block*)d->d_blocks.ptr, (const sla_hip_dec_info*)d->d_info.ptr,
                                         nb, C, (const int32_t*)d->d_kint.ptr, order, 1, d->stream));
      }
      HIPCHK(hipEventRecord(d->ev[1], d->stream));
      HIPCHK(hipStreamSynchronize(d->stream));
      ev_add_ms(&kernel_ms, d->ev[0], d->ev[1]);
    }

    /* ---- examine the blocks in file order: the first failure decides */
    if (!examine_blocks(d, d->h_crcf, d->h_blocks, d->h_info, nb, lms_ok, walk_err, one_block_size, &done_samples, &off, &pos, &result)) { break; }
  }

  /* ---- mid/side, left-justification, copy-out of everything before the failing block */
  if (done_samples > 0) {
    HIPCHK(hipEventRecord(d->ev[0], d->stream));
    RCCHK(sla_hip_launch_dec_finish(d_planes, stride, C, done_samples, ms, 32u - bps + lshift, d->stream));
    HIPCHK(hipEventRecord(d->ev[1], d->stream));
    t1 = now_ms();
    if (buffer != NULL) {
      for (ch = 0; ch < C; ch++) {
        HIPCHK(hipMemcpyAsync(buffer[ch], d_planes + (uint64_t)ch * stride, sizeof(int32_t) * (size_t)done_samples, hipMemcpyDeviceToHost, d->stream));
      }
    }
    HIPCHK(hipStreamSynchronize(d->stream));
    ev_add_ms(&kernel_ms, d->ev[0], d->ev[1]);
    d->timing[3] = (float)(now_ms() - t1);
  }
  *output_num_samples = done_samples;
  d->timing[0] = (float)t_up; d->timing[1] = (float)t_walk; d->timing[2] = kernel_ms;
  d->timing[4] = (float)(now_ms() - t0); d->timing[5] = (float)batches;
  return result;
}

SLAApiResult SLADecoder_DecodeWhole(struct SLADecoder* decoder, const uint8_t* data, uint32_t data_size,
                                    int32_t** buffer, uint32_t buffer_num_samples, uint32_t* output_num_samples)
{
  if (decoder == NULL || buffer == NULL || data == NULL || output_num_samples == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  return decode_run(decoder, data, data_size, NULL, NULL, 0, buffer, buffer_num_samples, output_num_samples, NULL);
}

SLAApiResult sla_hip_decode_device(struct SLADecoder* decoder, const uint8_t* host_data, const uint32_t* d_image,
                                   uint32_t data_size, int32_t* d_planes, uint64_t plane_stride,
                                   uint32_t* output_num_samples)
{
  if (decoder == NULL || host_data == NULL || d_image == NULL || d_planes == NULL || output_num_samples == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  return decode_run(decoder, host_data, data_size, d_image, d_planes, plane_stride, NULL,
                    (plane_stride > 0xFFFFFFFFull) ? 0xFFFFFFFFu : (uint32_t)plane_stride, output_num_samples, NULL);
}

/* ------------------------------------------------------------------------------------------------------------
 * The batch calls (include/sla_hip.h): the blocks of many files through the kernels together.  One pipeline, its
 * arithmetic in sla_dec_plan.c: the headers in item order with decode_run's code (the handle's format moves as under
 * DecodeWhole of one item after the other; fmt_mark / call_close leave it there); every file's block chain walked into rows
 * of the host tables; the files sorted so that equal launch parameters are neighbours and cut into passes (pass_cut).  A
 * pass lays its files out and reserves its scratch (pass_begin: images at 4-byte offsets, each block's reader bounded by the
 * end of its own file, a plane region per file), stages image and block table, runs each kernel once (pass_kernels),
 * examines every file with decode_run's code and delivers.  A file with a block body that does not end where its size
 * field says is decoded again, alone, through decode_run.  What each call adds:
 *   sla_hip_decode_batch           host sources and destinations: walk_chain, staging copies, one upload and one packed
 *                                  download (sla_hip_launch_dec_finish_batch) per pass.
 *   sla_hip_decode_batch_device    device destinations, written by the emit kernel (emit_run), zero fill included -- for items
 *                                  that reached no pass in a launch of its own (zero_fill_pending).
 *   sla_hip_decode_batch_resident  device sources the host never reads: the headers come home through a gather
 *                                  (res_fetch_headers), the walk runs on the device: in count mode before the passes are cut
 *                                  (res_count_walk), in write mode in each pass behind the gather that fills the pass image.
 *                                  That is the resident stage (stage_tables, stage_queue), one for whole files, windows and
 *                                  salvage; the examination reads the rows and stored CRC fields it brought home.
 * Device-destination calls keep their per-item arrays in one allocation (call_mem_t) and open with call_open.
 * ------------------------------------------------------------------------------------------------------------ */
#define DEC_BATCH_PASS_BYTES (1ull << 30)    /* stream bytes of one pass (staging and device image) */
#define DEC_COPY_THREADS     4u              /* host threads of a staging copy, the caller's own among them */
#define DEC_COPY_PIECE       ((size_t)4 << 20)

typedef struct { void* dst; const void* src; size_t bytes; } copy_job_t;
typedef struct { copy_job_t* v; uint32_t n, cap, next; size_t bytes; } copy_list_t;

static int copy_add(copy_list_t* l, void* dst, const void* src, size_t bytes)
{
  while (bytes > 0) {
    const size_t take = (bytes < DEC_COPY_PIECE) ? bytes : DEC_COPY_PIECE;
    if (l->n == l->cap) {
      const uint32_t cap = l->cap * 2 + 64;
      copy_job_t* v = (copy_job_t*)realloc(l->v, sizeof(*v) * cap);
      if (v == NULL) { return -1; }
      l->v = v; l->cap = cap;
    }
    l->v[l->n].dst = dst; l->v[l->n].src = src; l->v[l->n].bytes = take;
    l->n++; l->bytes += take;
    dst = (uint8_t*)dst + take; src = (const uint8_t*)src + take; bytes -= take;
  }
  return 0;
}

static void* copy_worker(void* arg)
{
  copy_list_t* l = (copy_list_t*)arg;
  for (;;) {
    const uint32_t k = __atomic_fetch_add(&l->next, 1u, __ATOMIC_RELAXED);
    if (k >= l->n) { return NULL; }
    memcpy(l->v[k].dst, l->v[k].src, l->v[k].bytes);
  }
}

/* the listed copies on at most DEC_COPY_THREADS threads; small lists stay on the caller's thread */
static void copy_run(copy_list_t* l)
{
  pthread_t tid[DEC_COPY_THREADS - 1];
  uint32_t nt = 0, t, want = (l->bytes >= 2 * DEC_COPY_PIECE) ? DEC_COPY_THREADS : 1u;
  if (want > l->n) { want = l->n; }
  l->next = 0;
  for (t = 1; t < want; t++) { if (pthread_create(&tid[nt], NULL, copy_worker, l) == 0) { nt++; } }
  (void)copy_worker(l);
  for (t = 0; t < nt; t++) { pthread_join(tid[t], NULL); }
  l->n = 0; l->bytes = 0;
}

typedef slai_dec_file bfile_t;       /* a file of a call: its rows are d->h_blocks[first, first + nb) */

/* where the pass that starts at files[p0] ends; files[0, n) are the sorted files that are not alone */
#define pass_cut(files, p0, n) slai_dec_cut(files, p0, n, SLA_HIP_DEC_BATCH_PASS, DEC_BATCH_PASS_BYTES)

#define BCHK(call) do { if ((call) != hipSuccess) { return -1; } } while (0)
#define BRC(call)  do { if ((call) != 0) { return -1; } } while (0)

/* The layout of the pass files[0, nf) (slai_dec_layout; planes of no sample still get one) and its scratch: the image, the
 * block table (nb rows, then nb block ends), infos, channel records, PARCOR integers, planes, CRC words (the stored fields
 * and, for salvage, as many verdicts).  The slack lets a kernel's last vector access run over. */
typedef struct { uint64_t img_bytes, regions, span; uint32_t nb; } pass_t;      /* regions: their sum; span: the plane stride */
static int pass_begin(struct SLADecoder* d, bfile_t* files, uint32_t nf, pass_t* p)
{
  const size_t nb_C = (size_t)files[0].f.C;
  slai_dec_layout(files, nf, &p->img_bytes, &p->regions, &p->nb);
  p->span = (p->regions == 0) ? 1 : p->regions;
  return (dbuf_reserve(&d->d_image, p->img_bytes + 16) != 0
          || dbuf_reserve(&d->d_blocks, (sizeof(sla_hip_dec_block) + sizeof(uint64_t)) * (size_t)p->nb + 16) != 0
          || dbuf_reserve(&d->d_info, sizeof(sla_hip_dec_info) * (size_t)p->nb + 16) != 0
          || dbuf_reserve(&d->d_chan, sizeof(sla_hip_dec_chan) * (size_t)p->nb * nb_C + 16) != 0
          || dbuf_reserve(&d->d_kint, sizeof(int32_t) * (size_t)p->nb * nb_C * (files[0].f.order + 1) + 16) != 0
          || dbuf_reserve(&d->d_planes, sizeof(int32_t) * (size_t)p->span * nb_C) != 0
          || dbuf_reserve(&d->d_crcf, sizeof(uint32_t) * 2 * (size_t)p->nb + 16) != 0) ? -1 : 0;
}

/* sla_hip_decode_batch_device: where the samples go.  The internal items (sla_hip_decode_item, buffer NULL) are the
 * caller's device items one to one. */
#define DEV_PENDING 0u     /* not (yet) in a pass: a failed header gets the zero fill alone */
#define DEV_REFUSED 1u     /* refused before its header: nothing written */
#define DEV_DECODED 2u     /* in a pass or decoded on its own: emitted there */
typedef struct {
  const sla_hip_decode_device_item* items;
  uint32_t  format, zero_fill;
  int       resident;        /* items[].data are device pointers; the internal items' data is the host copy of each header */
  const struct wav_out* wav; /* the WAV calls: whole files through the WAV emit instead (format, zero_fill unused) */
} dev_out_t;

/* sla_hip_decode_wav_batch / _resident: a file is delivered -- 44-byte header and frames, by sla_hip_launch_wav_emit_batch --
 * when its decode ended OK with every sample of its header and nothing kept it from delivery beforehand (hold[i] != 0: the
 * code the item gets, e.g. a destination that is too small; the decode itself still runs, so that the handle's format moves as
 * under the device calls).  host: the destinations are host memory -- the emit goes into a device staging image (d->d_out)
 * and one download per pass brings the files home. */
typedef struct wav_out {
  sla_hip_wav_item* items;
  int32_t*  hold;
  uint32_t* rate;            /* per item: the header's sampling rate */
  uint8_t*  delivered;       /* out, per item */
  int       host;
} wav_out_t;

/* The per-item arrays of one call, each num_items long and zero, in one allocation (call_mem_new); free(m.base) ends them. */
typedef struct {
  void* base;
  sla_hip_decode_item*        bi;       /* batch_run's items, where the caller's are of another kind */
  sla_hip_decode_device_item* dv;       /* the items as device items, likewise */
  sla_hip_dec_emit*           fill;     /* zero_fill_pending's table */
  bfile_t*                    files;
  const uint8_t**             src;      /* call_open: what res_fetch_headers reads */
  sla_hip_dec_window_result*  wres;     /* windows: every item's count-mode walk */
  uint32_t *size, *chans, *done;        /* chans: the channel count the item's header gave, 0 when none; done: by files[] */
  uint32_t *rate, *fbytes, *wbits; int32_t* hold;      /* the WAV calls: from each header; wav_out_t */
  uint8_t  *ok, *state, *delivered;     /* ok: the source may be read; state: DEV_* */
} call_mem_t;

static int call_mem_new(call_mem_t* m, uint32_t n)
{
  uint8_t* p;
  memset(m, 0, sizeof(*m));
  p = (uint8_t*)calloc(n, sizeof(*m->bi) + sizeof(*m->dv) + sizeof(*m->fill) + sizeof(*m->files) + sizeof(*m->src) + sizeof(*m->wres)
                          + 6 * sizeof(uint32_t) + sizeof(*m->hold) + 3);
  if ((m->base = p) == NULL) { return -1; }
#define CARVE(field) do { m->field = (void*)p; p += sizeof(*m->field) * (size_t)n; } while (0)
  CARVE(bi); CARVE(dv); CARVE(fill); CARVE(files); CARVE(src);      /* (sizes that are multiples of 8 first) */
  CARVE(wres); CARVE(size); CARVE(chans); CARVE(done); CARVE(rate); CARVE(fbytes); CARVE(wbits); CARVE(hold);
  CARVE(ok); CARVE(state); CARVE(delivered);
#undef CARVE
  return 0;
}

/* ---- resident sources: the device walk and the gather stand in for walk_chain and the staging copies ---- */
#define RES_HDR_SLOT 48u     /* bytes of one header in the gathered header image (43, padded, a multiple of 4) */

static int res_events(struct SLADecoder* d)
{
  int k;
  for (k = 0; k < 3; k++) { if (d->ev_src[k] == NULL && hipEventCreate(&d->ev_src[k]) != hipSuccess) { d->ev_src[k] = NULL; return -1; } }
  return 0;
}

/* 1 when [p, p + size) may be read by a kernel: the source check of the resident calls, before anything is read */
static int src_region_ok(const uint8_t* p, uint32_t size)
{
  return p != NULL && slai_device_region_ok(p, 1, size, 0, 1, 1, -1);
}

/* The first min(size, 43) bytes of every source with ok[i] set, gathered into one device buffer and brought home in one
 * copy: header i is at d->h_hdr + i * RES_HDR_SLOT.  On the handle's stream, waited for. */
static int res_fetch_headers(struct SLADecoder* d, const uint8_t* const* src, const uint32_t* size, const uint8_t* ok, uint32_t n)
{
  sla_hip_dec_gather* gt;
  uint32_t i, ng = 0;
  const size_t img = (size_t)n * RES_HDR_SLOT;
  if (hbuf_reserve(&d->h_hdr, img) != 0 || hbuf_reserve(&d->h_src, sizeof(*gt) * (size_t)n) != 0
      || dbuf_reserve(&d->d_src, sizeof(*gt) * (size_t)n) != 0 || dbuf_reserve(&d->d_image, img + 16) != 0) { return -1; }
  gt = (sla_hip_dec_gather*)d->h_src.ptr;
  for (i = 0; i < n; i++) {
    if (!ok[i]) { continue; }
    gt[ng].src = src[i]; gt[ng].dst_off = (uint64_t)i * RES_HDR_SLOT;
    gt[ng].bytes = (size[i] < SLA_HEADER_SIZE) ? size[i] : SLA_HEADER_SIZE; gt[ng].reserved = 0;
    ng++;
  }
  if (ng == 0) { return 0; }
  BCHK(hipMemcpyAsync(d->d_src.ptr, gt, sizeof(*gt) * ng, hipMemcpyHostToDevice, d->stream));
  BRC(sla_hip_launch_dec_gather((const sla_hip_dec_gather*)d->d_src.ptr, ng, SLA_HEADER_SIZE, (uint8_t*)d->d_image.ptr, img, d->stream));
  BCHK(hipMemcpyAsync(d->h_hdr.ptr, d->d_image.ptr, img, hipMemcpyDeviceToHost, d->stream));
  BCHK(hipStreamSynchronize(d->stream));
  return 0;
}

/* ---- long files: the wide walk (sla_hip_launch_dec_walk_wide) in place of a lane ----
 * Files of at least d->wide_walk bytes, the RES_WIDE_MAX longest of a call (ties: item order; slai_dec_pick_wide), are
 * walked by the whole device one after the other behind the lane launch, in whose table they stand with total = 0: the lane
 * writes their empty result and rows, the wide launches overwrite both.  The launches of a file are serial, so more of them
 * would only queue up, and a batch of many mid-size files is what the lane walk is good at.  A file's node capacity is
 * slai_dec_wide_capacity of the option "wide_walk_nodes" and its size. */
#define RES_WIDE_MAX SLAI_DEC_WIDE_MAX

/* room for the wide walks of the listed table entries: one scratch for the largest, the words that come home */
static int res_wide_reserve(struct SLADecoder* d, const sla_hip_dec_walk_file* wt, const uint32_t* list, uint32_t n)
{
  uint64_t need = 0;
  uint32_t j;
  for (j = 0; j < n; j++) {
    const uint32_t size = wt[list[j]].data_size;
    const uint64_t b = SLA_HIP_DEC_WIDE_SCRATCH_BYTES(size, slai_dec_wide_capacity(d->wide_nodes, size));
    if (b > need) { need = b; }
  }
  return (dbuf_reserve(&d->d_wide, (size_t)need) != 0
          || hbuf_reserve(&d->h_wide, (sizeof(sla_hip_dec_wide_info) + sizeof(sla_hip_dec_walk_result)) * RES_WIDE_MAX) != 0) ? -1 : 0;
}

/* one file's wide walk queued on the handle's stream: its result to d->d_wres[slot], rows (write mode) to the tables;
 * info != NULL: the scratch's info words go home to it */
static int res_wide_launch(struct SLADecoder* d, const sla_hip_dec_walk_file* wf, uint32_t slot, sla_hip_dec_block* db,
                           uint64_t* dend, uint32_t* dcrc, sla_hip_dec_wide_info* info)
{
  const uint32_t cap = slai_dec_wide_capacity(d->wide_nodes, wf->data_size);
  BRC(sla_hip_launch_dec_walk_wide(wf, d->cfg.max_num_block_samples, d->cfg.enable_crc_check, (sla_hip_dec_walk_result*)d->d_wres.ptr + slot,
                                   db, dend, dcrc, cap, d->d_wide.ptr, d->stream));
  if (info != NULL) { BCHK(hipMemcpyAsync(info, d->d_wide.ptr, sizeof(*info), hipMemcpyDeviceToHost, d->stream)); }
  d->walk_stats[3] += sla_hip_dec_wide_rounds(wf->data_size, cap);
  return 0;
}

/* The count-mode walk of files[0, nf): one launch, one small copy home; sets every file's first / nb / walk_err / extent
 * and *nblocks, and makes room for that many rows in the host tables.  Long files go wide behind the lane launch; one
 * whose nodes overflow the capacity is walked on a lane after all, in a second launch, and stays on the lane. */
static int res_count_walk(struct SLADecoder* d, const sla_hip_decode_item* items, const dev_out_t* dev, bfile_t* files, uint32_t nf,
                          uint32_t* nblocks)
{
  sla_hip_dec_walk_file* wt;
  sla_hip_dec_walk_result* wr;
  uint64_t total = 0;
  uint32_t i, j, npick, nover = 0, pick[RES_WIDE_MAX], over[RES_WIDE_MAX];
  if (nf == 0) { return 0; }
  if (hbuf_reserve(&d->h_src, (sizeof(*wt) + sizeof(*wr)) * (size_t)nf) != 0 || dbuf_reserve(&d->d_src, sizeof(*wt) * (size_t)nf) != 0
      || dbuf_reserve(&d->d_wres, sizeof(*wr) * (size_t)nf) != 0) { return -1; }
  wt = (sla_hip_dec_walk_file*)d->h_src.ptr;
  wr = (sla_hip_dec_walk_result*)(wt + nf);
  for (i = 0; i < nf; i++) {
    const sla_hip_decode_item* it = &items[files[i].item];
    memset(&wt[i], 0, sizeof(wt[i]));
    wt[i].src = dev->items[files[i].item].data; wt[i].data_size = it->data_size;
    wt[i].total = files[i].f.total; wt[i].capacity = it->buffer_num_samples;
  }
  npick = slai_dec_pick_wide(files, nf, d->wide_walk, pick);
  if (npick > 0 && res_wide_reserve(d, wt, pick, npick) != 0) { return -1; }
  for (j = 0; j < npick; j++) { wt[pick[j]].total = 0; }
  BCHK(hipMemcpyAsync(d->d_src.ptr, wt, sizeof(*wt) * nf, hipMemcpyHostToDevice, d->stream));
  BRC(sla_hip_launch_dec_walk((const sla_hip_dec_walk_file*)d->d_src.ptr, nf, d->cfg.max_num_block_samples, d->cfg.enable_crc_check,
                              (sla_hip_dec_walk_result*)d->d_wres.ptr, NULL, NULL, NULL, d->stream));
  for (j = 0; j < npick; j++) {
    sla_hip_dec_walk_file wf = wt[pick[j]];               /* (a copy: the table is on its way to the device) */
    wf.total = files[pick[j]].f.total;
    if (res_wide_launch(d, &wf, pick[j], NULL, NULL, NULL, (sla_hip_dec_wide_info*)d->h_wide.ptr + j) != 0) { return -1; }
  }
  BCHK(hipMemcpyAsync(wr, d->d_wres.ptr, sizeof(*wr) * nf, hipMemcpyDeviceToHost, d->stream));
  BCHK(hipStreamSynchronize(d->stream));
  for (j = 0; j < npick; j++) {
    d->walk_stats[0]++;
    d->walk_stats[2] += ((const sla_hip_dec_wide_info*)d->h_wide.ptr)[j].nodes;
    if (wr[pick[j]].reserved == SLA_HIP_DEC_WIDE_OVERFLOW) { d->walk_stats[1]++; over[nover++] = pick[j]; }
    else { files[pick[j]].wide = 1; }
  }
  if (nover > 0) {
    /* more nodes than the capacity: those files on lanes, in a launch of their own (the tables are free again) */
    sla_hip_dec_walk_file* ot = (sla_hip_dec_walk_file*)d->h_src.ptr;
    sla_hip_dec_walk_result* orr = (sla_hip_dec_walk_result*)((sla_hip_dec_wide_info*)d->h_wide.ptr + RES_WIDE_MAX);
    sla_hip_dec_walk_file keep[RES_WIDE_MAX];
    for (j = 0; j < nover; j++) { keep[j] = wt[over[j]]; keep[j].total = files[over[j]].f.total; }
    for (j = 0; j < nover; j++) { ot[j] = keep[j]; }
    BCHK(hipMemcpyAsync(d->d_src.ptr, ot, sizeof(*ot) * nover, hipMemcpyHostToDevice, d->stream));
    BRC(sla_hip_launch_dec_walk((const sla_hip_dec_walk_file*)d->d_src.ptr, nover, d->cfg.max_num_block_samples, d->cfg.enable_crc_check,
                                (sla_hip_dec_walk_result*)d->d_wres.ptr, NULL, NULL, NULL, d->stream));
    BCHK(hipMemcpyAsync(orr, d->d_wres.ptr, sizeof(*orr) * nover, hipMemcpyDeviceToHost, d->stream));
    BCHK(hipStreamSynchronize(d->stream));
    for (j = 0; j < nover; j++) { wr[over[j]] = orr[j]; }
  }
  for (i = 0; i < nf; i++) {
    files[i].first = (uint32_t)total; files[i].nb = wr[i].num_blocks;
    files[i].walk_err = (SLAApiResult)wr[i].stop; files[i].extent = wr[i].extent;
    total += wr[i].num_blocks;
  }
  if (total > 0xFFFFFFFFull || host_tables_reserve(d, (uint32_t)total) != 0) { return -1; }
  *nblocks = (uint32_t)total;
  return 0;
}

/* ---- the resident stage of a pass: what stands in for staging copies, upload and walk_chain when the sources are in
 * device memory; one for whole files (batch, WAV, salvage) and windows, up to the kind of walk. ----
 * Its tables lie in d->h_src (page-locked) and d->d_src: the gather table and behind it the walk table (sla_hip_dec_walk_file
 * or sla_hip_dec_window_file per file), over in one copy; behind them, on the host only, the write-mode walk's results
 * (sla_hip_dec_walk_result / _window_result), home after the pass's wait.  Only stage_tables knows where each lies. */
typedef struct {
  sla_hip_dec_gather* gt; void* wt; void* wr;                  /* host */
  const sla_hip_dec_gather* d_gt; const void* d_wt;            /* device */
  size_t up_bytes, wr_bytes;
} stage_t;

static int stage_tables(struct SLADecoder* d, uint32_t nf, size_t wt_size, size_t wr_size, stage_t* st)
{
  st->up_bytes = (sizeof(*st->gt) + wt_size) * (size_t)nf; st->wr_bytes = wr_size * (size_t)nf;
  if (hbuf_reserve(&d->h_src, st->up_bytes + st->wr_bytes) != 0 || dbuf_reserve(&d->d_src, st->up_bytes) != 0
      || dbuf_reserve(&d->d_wres, st->wr_bytes) != 0 || res_events(d) != 0) { return -1; }
  st->gt = (sla_hip_dec_gather*)d->h_src.ptr; st->wt = st->gt + nf; st->wr = (uint8_t*)st->wt + wt_size * (size_t)nf;
  st->d_gt = (const sla_hip_dec_gather*)d->d_src.ptr; st->d_wt = st->d_gt + nf;
  memset(st->gt, 0, st->up_bytes);
  return 0;
}

/* the first half of the stage: the tables over, the first ng gather entries (the longest max_bytes) into the pass image */
static int stage_gather(struct SLADecoder* d, const stage_t* st, uint32_t ng, uint32_t max_bytes, uint64_t img_bytes)
{
  BCHK(hipMemcpyAsync(d->d_src.ptr, st->gt, st->up_bytes, hipMemcpyHostToDevice, d->stream));
  BCHK(hipEventRecord(d->ev_src[0], d->stream));
  BRC(sla_hip_launch_dec_gather(st->d_gt, ng, max_bytes, (uint8_t*)d->d_image.ptr, img_bytes, d->stream));
  BCHK(hipEventRecord(d->ev_src[1], d->stream));
  return 0;
}

/* The stage of the pass files[0, nf), queued on the handle's stream and not waited for: stage_gather, then the walk in write
 * mode -- of windows, or of whole files with the wide walks of the long ones behind the lane launch -- into the block table
 * (d->d_blocks: nb rows, then nb ends) and d->d_crcf.  The walk's results (st->wr), the rows and the CRC fields
 * (d->h_blocks / d->h_crcf from the pass's first row) are on their way home, d->d_info is cleared. */
static int stage_queue(struct SLADecoder* d, const stage_t* st, const bfile_t* files, uint32_t nf, int windows, uint32_t ng,
                       uint32_t max_bytes, const pass_t* p)
{
  sla_hip_dec_block* db = (sla_hip_dec_block*)d->d_blocks.ptr;
  uint64_t* dend = (uint64_t*)(db + p->nb);
  uint32_t* dcrc = (uint32_t*)d->d_crcf.ptr;
  const uint32_t first = files[0].first;
  uint32_t i;
  if (stage_gather(d, st, ng, max_bytes, p->img_bytes) != 0) { return -1; }
  if (windows) {
    BRC(sla_hip_launch_dec_walk_window((const sla_hip_dec_window_file*)st->d_wt, nf, d->cfg.max_num_block_samples,
                                       (sla_hip_dec_window_result*)d->d_wres.ptr, db, dend, dcrc, d->stream));
  } else {
    BRC(sla_hip_launch_dec_walk((const sla_hip_dec_walk_file*)st->d_wt, nf, d->cfg.max_num_block_samples, d->cfg.enable_crc_check,
                                (sla_hip_dec_walk_result*)d->d_wres.ptr, db, dend, dcrc, d->stream));
    for (i = 0; i < nf; i++) {
      if (!files[i].wide) { continue; }
      sla_hip_dec_walk_file wf = ((const sla_hip_dec_walk_file*)st->wt)[i];      /* (a copy: the table is on its way to the device) */
      wf.total = files[i].f.total;
      if (res_wide_launch(d, &wf, i, db, dend, dcrc, NULL) != 0) { return -1; }
    }
  }
  BCHK(hipMemcpyAsync(st->wr, d->d_wres.ptr, st->wr_bytes, hipMemcpyDeviceToHost, d->stream));
  BCHK(hipMemcpyAsync(d->h_blocks + first, db, sizeof(*db) * (size_t)p->nb, hipMemcpyDeviceToHost, d->stream));
  BCHK(hipMemcpyAsync(d->h_crcf + first, dcrc, sizeof(uint32_t) * (size_t)p->nb, hipMemcpyDeviceToHost, d->stream));
  BCHK(hipEventRecord(d->ev_src[2], d->stream));
  BCHK(hipMemsetAsync(d->d_info.ptr, 0, sizeof(sla_hip_dec_info) * p->nb, d->stream));
  return 0;
}

/* after the pass's wait: the stage's times */
static void stage_times(struct SLADecoder* d, double* t_gather, double* t_walk)
{
  ev_add_ms(t_gather, d->ev_src[0], d->ev_src[1]); ev_add_ms(t_walk, d->ev_src[1], d->ev_src[2]);
}

/* The tables of a pass of whole resident files (source i is src[files[i].item]) and its stage queued; nothing when the pass
 * has no block. */
static int res_stage_pass(struct SLADecoder* d, const sla_hip_decode_item* items, const dev_out_t* dev, const bfile_t* files,
                          uint32_t nf, const pass_t* p, stage_t* st)
{
  sla_hip_dec_gather* gt;
  sla_hip_dec_walk_file* wt;
  const uint32_t first = files[0].first;
  uint32_t i, max_bytes = 0;
  if (p->nb == 0) { return 0; }
  if (stage_tables(d, nf, sizeof(*wt), sizeof(sla_hip_dec_walk_result), st) != 0) { return -1; }
  gt = st->gt; wt = (sla_hip_dec_walk_file*)st->wt;
  for (i = 0; i < nf; i++) {
    const sla_hip_decode_item* it = &items[files[i].item];
    gt[i].src = dev->items[files[i].item].data; gt[i].dst_off = files[i].img_off; gt[i].bytes = it->data_size; gt[i].reserved = 0;
    wt[i].src = gt[i].src; wt[i].img_off = files[i].img_off; wt[i].data_size = it->data_size; wt[i].total = files[i].f.total;
    wt[i].capacity = it->buffer_num_samples; wt[i].first = files[i].first - first; wt[i].max_rows = files[i].nb;
    wt[i].plane_off = (uint32_t)files[i].plane_off;
    if (it->data_size > max_bytes) { max_bytes = it->data_size; }
    if (files[i].wide) {
      if (res_wide_reserve(d, wt, &i, 1) != 0) { return -1; }
      wt[i].total = 0;
    }
  }
  return stage_queue(d, st, files, nf, 0, nf, max_bytes, p);
}

/* After the pass's wait: the stage's times, the rows brought back to positions in their own files (what examine_blocks
 * reads), and the write-mode walk checked against the count: a file whose chain changed in between fails the call. */
static int res_finish_pass(struct SLADecoder* d, const stage_t* st, const bfile_t* files, uint32_t nf, double* t_gather, double* t_walk)
{
  const sla_hip_dec_walk_result* wr = (const sla_hip_dec_walk_result*)st->wr;
  uint32_t i, b;
  stage_times(d, t_gather, t_walk);
  for (i = 0; i < nf; i++) {
    if (wr[i].num_blocks != files[i].nb || wr[i].stop != (uint32_t)files[i].walk_err || wr[i].extent != files[i].extent
        || wr[i].reserved != 0) { return -1; }                 /* reserved: a wide walk that overflowed since the count */
    for (b = 0; b < files[i].nb; b++) {
      d->h_blocks[files[i].first + b].byte_off -= files[i].img_off;
      d->h_blocks[files[i].first + b].smp_off -= (uint32_t)files[i].plane_off;
    }
  }
  return 0;
}

/* one emit table entry for item `it` (0 when there is nothing to write) */
static uint32_t emit_entry(sla_hip_dec_emit* e, const sla_hip_decode_device_item* it, uint32_t zero_fill, uint64_t plane_off,
                           uint32_t done, uint32_t C, uint32_t ms, uint32_t shift, uint32_t bps, uint32_t* max_lim)
{
  const uint32_t fill_end = zero_fill ? it->capacity : 0, lim = (fill_end > done) ? fill_end : done;
  if (lim == 0 || C == 0) { return 0; }
  e->plane_off = plane_off; e->channel_stride = it->channel_stride; e->sample_stride = it->sample_stride; e->dst = it->dst;
  e->done = done; e->fill_end = fill_end; e->num_channels = C; e->mid_side = ms; e->shift = shift; e->bits_per_sample = bps;
  if (lim > *max_lim) { *max_lim = lim; }
  return 1;
}

/* the emit table over in one copy and the emit kernel over it, on the handle's stream, waited for; its kernel time is
 * added to *kernel_ms */
static int emit_run(struct SLADecoder* d, const int32_t* planes, uint64_t stride, const sla_hip_dec_emit* et, uint32_t ne,
                    uint32_t max_lim, uint32_t format, float* kernel_ms)
{
  if (ne == 0) { return 0; }
  if (dbuf_reserve(&d->d_ftab, sizeof(*et) * ne) != 0) { return -1; }
  if (planes == NULL) {               /* a table of zero fills only: the kernel reads no plane, but takes a valid pointer */
    if (dbuf_reserve(&d->d_planes, 256) != 0) { return -1; }
    planes = (const int32_t*)d->d_planes.ptr;
  }
  BCHK(hipMemcpyAsync(d->d_ftab.ptr, et, sizeof(*et) * ne, hipMemcpyHostToDevice, d->stream));
  BCHK(hipEventRecord(d->ev[0], d->stream));
  BRC(sla_hip_launch_dec_emit_batch(planes, stride, (const sla_hip_dec_emit*)d->d_ftab.ptr, ne, max_lim, format, d->stream));
  BCHK(hipEventRecord(d->ev[1], d->stream));
  BCHK(hipStreamSynchronize(d->stream));
  ev_add_ms(kernel_ms, d->ev[0], d->ev[1]);
  return 0;
}

/* device destinations of items whose header gave a channel count but of which nothing was decoded (DEV_PENDING): the zero
 * fill, all of them in one launch of the emit kernel */
static int zero_fill_pending(struct SLADecoder* d, const call_mem_t* m, const sla_hip_decode_device_item* items, uint32_t num_items,
                             uint32_t format, float* kernel_ms, double* t_down)
{
  const double t = now_ms();
  uint32_t i, ne = 0, max_lim = 0;
  int rc;
  for (i = 0; i < num_items; i++) {
    if (m->state[i] == DEV_PENDING) { ne += emit_entry(m->fill + ne, &items[i], 1, 0, 0, m->chans[i], 0, 0, 32, &max_lim); }
  }
  rc = emit_run(d, NULL, 1, m->fill, ne, max_lim, format, kernel_ms);
  *t_down += now_ms() - t;
  return rc;
}

/* The last leg of the WAV calls for files[0, nf) that share C and bps (a pass, or one file decoded on its own): every file
 * that is to be delivered (wav_out_t) gets its header and its place in the emit table, one upload, one launch; host
 * destinations: one download of the staging image and the copies into the callers' buffers.  in_pass: the planes hold the
 * pass (regions at files[].plane_off, mid/side and shift still to do); otherwise decode_run's finished planes of one file. */
static int wav_emit_run(struct SLADecoder* d, const dev_out_t* dev, const sla_hip_decode_item* items, const bfile_t* files,
                        const uint32_t* done, uint32_t nf, int in_pass, const int32_t* planes, uint64_t stride, copy_list_t* cl,
                        float* kernel_ms)
{
  const wav_out_t* w = dev->wav;
  const dec_format_t* f = &files[0].f;
  const uint32_t B = f->bps / 8;
  sla_hip_wav_emit* et;
  uint64_t stage = 0;
  uint32_t i, ne = 0, max_n = 0;
  if (hbuf_reserve(&d->h_wav, sizeof(*et) * (size_t)nf) != 0 || dbuf_reserve(&d->d_wav, sizeof(*et) * (size_t)nf) != 0) { return -1; }
  et = (sla_hip_wav_emit*)d->h_wav.ptr;
  for (i = 0; i < nf; i++) {
    const uint32_t item = files[i].item;
    sla_hip_wav_info info;
    if ((in_pass && files[i].alone) || items[item].result != SLA_APIRESULT_OK || done[i] != files[i].f.total || w->hold[item] != 0) { continue; }
    memset(&et[ne], 0, sizeof(et[ne]));
    info.num_channels = f->C; info.bits_per_sample = f->bps; info.sampling_rate = w->rate[item];
    info.num_samples = done[i]; info.data_off = SLA_HIP_WAV_HEADER_BYTES; info.data_bytes = done[i] * f->C * B;
    (void)sla_hip_wav_header(&info, et[ne].header);
    et[ne].plane_off = in_pass ? files[i].plane_off : 0;
    et[ne].num_samples = done[i];
    et[ne].mid_side = in_pass ? f->ms : 0;
    et[ne].shift = in_pass ? 32u - f->bps + f->lshift : 0;
    et[ne].header_bytes = SLA_HIP_WAV_HEADER_BYTES;
    et[ne].dst = w->host ? (uint8_t*)(uintptr_t)stage : w->items[item].dst;      /* (host: the offset, until the image is there) */
    stage += (uint64_t)SLA_HIP_WAV_HEADER_BYTES + info.data_bytes;
    if (done[i] > max_n) { max_n = done[i]; }
    w->delivered[item] = 1;
    ne++;
  }
  if (ne == 0) { return 0; }
  if (w->host) {
    if (dbuf_reserve(&d->d_out, stage + 16) != 0 || hbuf_reserve(&d->h_out, stage + 16) != 0) { return -1; }
    for (i = 0; i < ne; i++) { et[i].dst = (uint8_t*)d->d_out.ptr + (uintptr_t)et[i].dst; }
  }
  BCHK(hipMemcpyAsync(d->d_wav.ptr, et, sizeof(*et) * ne, hipMemcpyHostToDevice, d->stream));
  BCHK(hipEventRecord(d->ev[0], d->stream));
  BRC(sla_hip_launch_wav_emit_batch(planes, stride, (const sla_hip_wav_emit*)d->d_wav.ptr, ne, max_n, f->C, B,
                                    (in_pass && f->ms && f->C == 2) ? 1u : 0u, d->stream));
  BCHK(hipEventRecord(d->ev[1], d->stream));
  if (w->host) { BCHK(hipMemcpyAsync(d->h_out.ptr, d->d_out.ptr, stage, hipMemcpyDeviceToHost, d->stream)); }
  BCHK(hipStreamSynchronize(d->stream));
  ev_add_ms(kernel_ms, d->ev[0], d->ev[1]);
  if (w->host) {
    uint32_t k = 0;
    for (i = 0; i < nf; i++) {
      const uint32_t item = files[i].item;
      if ((in_pass && files[i].alone) || !w->delivered[item]) { continue; }
      if (copy_add(cl, w->items[item].dst, (const uint8_t*)d->h_out.ptr + ((uintptr_t)et[k].dst - (uintptr_t)d->d_out.ptr),
                   (size_t)SLA_HIP_WAV_HEADER_BYTES + (size_t)et[k].num_samples * f->C * B) != 0) { return -1; }
      k++;
    }
    copy_run(cl);
  }
  return 0;
}

/* The decode kernels of a pass, once each over its nb blocks: the table (nb rows, then nb block ends) is in d->d_blocks,
 * the image in d->d_image, d->d_info is cleared.  The block infos come home to d->h_info[first ...]; waited for, the
 * kernels' time is added to *kernel_ms. */
static int pass_kernels_run(struct SLADecoder* d, const dec_format_t* f, uint32_t nb, uint32_t first, uint64_t img_bytes, uint64_t span,
                            float* kernel_ms, int queued);
static int pass_kernels(struct SLADecoder* d, const dec_format_t* f, uint32_t nb, uint32_t first, uint64_t img_bytes, uint64_t span,
                        float* kernel_ms)
{
  return pass_kernels_run(d, f, nb, first, img_bytes, span, kernel_ms, 0);
}
/* queued: the kernels only, on the handle's stream -- nothing comes home, nothing is waited for, no event is recorded */
static int pass_kernels_run(struct SLADecoder* d, const dec_format_t* f, uint32_t nb, uint32_t first, uint64_t img_bytes, uint64_t span,
                            float* kernel_ms, int queued)
{
  const sla_hip_dec_block* db = (const sla_hip_dec_block*)d->d_blocks.ptr;
  const sla_hip_dec_info* di = (const sla_hip_dec_info*)d->d_info.ptr;
  int32_t* planes = (int32_t*)d->d_planes.ptr;
  const uint32_t C = f->C;
  if (!queued) { BCHK(hipEventRecord(d->ev[0], d->stream)); }
  BRC(sla_hip_launch_dec_bits_x((const uint32_t*)d->d_image.ptr, img_bytes, db, nb, C, f->bps, f->lshift, f->ms, f->order, f->ntaps,
                                d->cfg.enable_crc_check == 1, planes, span, (sla_hip_dec_info*)d->d_info.ptr,
                                (sla_hip_dec_chan*)d->d_chan.ptr, (int32_t*)d->d_kint.ptr, d->stream,
                                (const uint64_t*)(db + nb)));
  if (!queued) { BCHK(hipMemcpyAsync(d->h_info + first, d->d_info.ptr, sizeof(sla_hip_dec_info) * nb, hipMemcpyDeviceToHost, d->stream)); }
  if (lms_order_ok(f->lms)) {
    BRC(sla_hip_launch_dec_lms(planes, span, db, di, nb, C, f->lms, d->stream));
    BRC(sla_hip_launch_dec_ltm(planes, span, db, di, (const sla_hip_dec_chan*)d->d_chan.ptr, nb, C, f->ntaps, d->cfg.max_num_block_samples, d->stream));
    BRC(sla_hip_launch_dec_lattice(planes, span, db, di, nb, C, (const int32_t*)d->d_kint.ptr, f->order, 1, d->stream));
  }
  if (queued) { return 0; }
  BCHK(hipEventRecord(d->ev[1], d->stream));
  BCHK(hipStreamSynchronize(d->stream));
  ev_add_ms(kernel_ms, d->ev[0], d->ev[1]);
  return 0;
}

/* One pass: files[0, nf), all with the same launch parameters, blocks d->h_blocks[files[0].first ...] contiguous.
 * dev != NULL: the samples go to the caller's device destinations through the emit kernel, nothing comes home.
 * Returns -1 on a device or allocation failure. */
static int batch_pass(struct SLADecoder* d, sla_hip_decode_item* items, bfile_t* files, uint32_t* done, uint32_t nf, copy_list_t* cl,
                      const dev_out_t* dev, double* t_up, double* t_walk, double* t_down, float* kernel_ms)
{
  const dec_format_t* f = &files[0].f;
  const uint32_t C = f->C, first = files[0].first;
  const int lms_ok = lms_order_ok(f->lms), res = (dev != NULL && dev->resident);
  uint64_t img_bytes, span, out_elems = 0;
  uint32_t nb, i, k, nfin = 0, max_done = 0;
  sla_hip_dec_block* tb;
  uint64_t* tend;
  sla_hip_dec_file* ft;
  pass_t p; stage_t st;
  double t;

  /* ---- images into staging (the bytes after each file up to its 4-byte boundary are zero) and over in one copy,
   *      the block table -- positions in the pass, then every block's end of stream -- likewise */
  t = now_ms();
  if (pass_begin(d, files, nf, &p) != 0) { return -1; }
  img_bytes = p.img_bytes; span = p.span; nb = p.nb;
  if ((!res && hbuf_reserve(&d->h_img, img_bytes + 16) != 0)
      || hbuf_reserve(&d->h_ptab, (sizeof(sla_hip_dec_block) + sizeof(uint64_t)) * (size_t)nb + sizeof(sla_hip_dec_emit) * nf) != 0
      || dbuf_reserve(&d->d_ftab, sizeof(sla_hip_dec_file) * nf) != 0) { return -1; }
  tb = (sla_hip_dec_block*)d->h_ptab.ptr;
  tend = (uint64_t*)(tb + nb);
  if (res) {
    /* resident sources: the gather and the walk in write mode do on the device what the rest of this stage does here */
    if (res_stage_pass(d, items, dev, files, nf, &p, &st) != 0) { return -1; }
  } else {
    for (i = 0; i < nf; i++) {
      const sla_hip_decode_item* it = &items[files[i].item];
      uint8_t* dst = (uint8_t*)d->h_img.ptr + files[i].img_off;
      const uint32_t pad = (uint32_t)(((uint64_t)it->data_size + 3) & ~(uint64_t)3) - it->data_size;
      if (pad != 0) { memset(dst + it->data_size, 0, pad); }
      if (copy_add(cl, dst, it->data, it->data_size) != 0) { return -1; }
    }
    copy_run(cl);
    for (i = 0, k = 0; i < nf; i++) {
      const uint64_t end = files[i].img_off + items[files[i].item].data_size;
      uint32_t b;
      for (b = 0; b < files[i].nb; b++, k++) {
        tb[k] = d->h_blocks[files[i].first + b];
        tb[k].byte_off += files[i].img_off;
        tb[k].smp_off += (uint32_t)files[i].plane_off;
        tend[k] = end;
      }
    }
    BCHK(hipMemcpyAsync(d->d_image.ptr, d->h_img.ptr, img_bytes, hipMemcpyHostToDevice, d->stream));
    BCHK(hipMemcpyAsync(d->d_blocks.ptr, tb, (sizeof(sla_hip_dec_block) + sizeof(uint64_t)) * (size_t)nb, hipMemcpyHostToDevice, d->stream));
    BCHK(hipMemsetAsync(d->d_info.ptr, 0, sizeof(sla_hip_dec_info) * nb, d->stream));
    BCHK(hipStreamSynchronize(d->stream));
    *t_up += now_ms() - t;
  }

  /* ---- the kernels, once each over all blocks of the pass */
  if (nb > 0) {
    if (pass_kernels(d, f, nb, first, img_bytes, span, kernel_ms) != 0) { return -1; }
    if (res && res_finish_pass(d, &st, files, nf, t_up, t_walk) != 0) { return -1; }
  }

  /* ---- every file examined on its own, in file order, with decode_run's code (done[]: zero on entry) */
  ft = (sla_hip_dec_file*)(tend + nb);
  for (i = 0; i < nf; i++) {
    sla_hip_decode_item* it = &items[files[i].item];
    uint32_t off = SLA_HEADER_SIZE, pos = 0;
    SLAApiResult result;
    if (examine_blocks(d, d->h_crcf + files[i].first, d->h_blocks + files[i].first, d->h_info + files[i].first, files[i].nb, lms_ok,
                       files[i].walk_err, NULL, &done[i], &off, &pos, &result)) {
      /* a block body that does not end where its size field says: the walk would resume where the reader stopped.
       * Rare (damaged or hand-made streams) -- the file is decoded again on its own, which is exact by construction. */
      files[i].alone = 1; done[i] = 0;
      continue;
    }
    it->result = result;
    if (done[i] > 0 && dev == NULL) {
      ft[nfin].plane_off = files[i].plane_off; ft[nfin].out_off = out_elems; ft[nfin].num_samples = done[i];
      ft[nfin].mid_side = f->ms; ft[nfin].shift = 32u - f->bps + f->lshift; ft[nfin].reserved = 0;
      out_elems += (uint64_t)done[i] * C;
      if (done[i] > max_done) { max_done = done[i]; }
      nfin++;
    }
  }

  /* ---- mid/side and left-justification of every file, packed, home in one copy, into the caller's planes; or, for
   *      device destinations, converted and stored there by the emit kernel, zero fill included */
  t = now_ms();
  if (dev != NULL && dev->wav != NULL) {
    if (wav_emit_run(d, dev, items, files, done, nf, 1, (const int32_t*)d->d_planes.ptr, span, cl, kernel_ms) != 0) { return -1; }
  } else if (dev != NULL) {
    sla_hip_dec_emit* et = (sla_hip_dec_emit*)(tend + nb);
    uint32_t ne = 0, max_lim = 0;
    for (i = 0; i < nf; i++) {
      if (files[i].alone) { continue; }
      ne += emit_entry(et + ne, &dev->items[files[i].item], dev->zero_fill, files[i].plane_off, done[i], C, f->ms,
                       32u - f->bps + f->lshift, f->bps, &max_lim);
    }
    if (emit_run(d, (const int32_t*)d->d_planes.ptr, span, et, ne, max_lim, dev->format, kernel_ms) != 0) { return -1; }
  } else if (nfin > 0) {
    uint64_t o = 0;
    if (dbuf_reserve(&d->d_out, sizeof(int32_t) * out_elems) != 0 || hbuf_reserve(&d->h_out, sizeof(int32_t) * out_elems) != 0) { return -1; }
    if (hipMemcpyAsync(d->d_ftab.ptr, ft, sizeof(sla_hip_dec_file) * nfin, hipMemcpyHostToDevice, d->stream) != hipSuccess
        || hipEventRecord(d->ev[0], d->stream) != hipSuccess
        || sla_hip_launch_dec_finish_batch((const int32_t*)d->d_planes.ptr, span, C, (const sla_hip_dec_file*)d->d_ftab.ptr, nfin,
                                           max_done, (int32_t*)d->d_out.ptr, d->stream) != 0
        || hipEventRecord(d->ev[1], d->stream) != hipSuccess
        || hipMemcpyAsync(d->h_out.ptr, d->d_out.ptr, sizeof(int32_t) * out_elems, hipMemcpyDeviceToHost, d->stream) != hipSuccess
        || hipStreamSynchronize(d->stream) != hipSuccess) { return -1; }
    ev_add_ms(kernel_ms, d->ev[0], d->ev[1]);
    for (i = 0; i < nf; i++) {
      sla_hip_decode_item* it = &items[files[i].item];
      uint32_t c;
      if (files[i].alone || done[i] == 0) { continue; }
      for (c = 0; c < C; c++) {
        if (copy_add(cl, it->buffer[c], (const int32_t*)d->h_out.ptr + o + (uint64_t)c * done[i], sizeof(int32_t) * (size_t)done[i]) != 0) { return -1; }
      }
      o += (uint64_t)done[i] * C;
    }
    copy_run(cl);
  }
  for (i = 0; i < nf; i++) { if (!files[i].alone) { items[files[i].item].output_num_samples = done[i]; } }
  *t_down += now_ms() - t;
  return 0;
}

/* The handle's format as the headers of a call left it, and the close of a call: the format is put back there (m != NULL:
 * decode_run on an `alone` file moves it out of item order) and timing[0..5] written (sla_hip_decoder_last_timing). */
typedef struct { struct SLAWaveFormat wf; struct SLAEncodeParameter ep; uint32_t flag; } fmt_mark_t;
static void fmt_mark(const struct SLADecoder* d, fmt_mark_t* m) { m->wf = d->wave_format; m->ep = d->encode_param; m->flag = d->status_flag; }
static void call_close(struct SLADecoder* d, const fmt_mark_t* m, double t0, double t_in, double t_walk, float kernel_ms, double t_out,
                       uint32_t passes)
{
  if (m != NULL) { d->wave_format = m->wf; d->encode_param = m->ep; d->status_flag = m->flag; }
  d->timing[0] = (float)t_in; d->timing[1] = (float)t_walk; d->timing[2] = kernel_ms; d->timing[3] = (float)t_out;
  d->timing[4] = (float)(now_ms() - t0); d->timing[5] = (float)passes;
}

/* num_items > 0; m: the call's arrays (files, done, fill; with dev also state and chans, as call_open left them) */
static int batch_run(struct SLADecoder* d, sla_hip_decode_item* items, uint32_t num_items, const dev_out_t* dev, call_mem_t* m)
{
  bfile_t* files = m->files;
  copy_list_t cl;
  fmt_mark_t after;
  uint32_t nf = 0, npass, nblocks = 0, passes = 0, i, p0;
  const int res = (dev != NULL && dev->resident);
  int rc = 0;
  float kernel_ms = 0.0f;
  double t0 = now_ms(), t_walk = 0.0, t_up = 0.0, t_down = 0.0, t;

  if (drain(d) != 0) { return SLA_APIRESULT_NG; }
  memset(d->timing, 0, sizeof(d->timing));
  if (res) { memset(d->walk_stats, 0, sizeof(d->walk_stats)); }
  memset(&cl, 0, sizeof(cl));

  /* ---- headers in item order: the handle's format moves exactly as under DecodeWhole of one item after the other */
  t = now_ms();
  for (i = 0; i < num_items; i++) {
    sla_hip_decode_item* it = &items[i];
    dec_format_t f;
    SLAApiResult ret;
    int verdict;
    uint32_t c;
    it->output_num_samples = 0;
    if (dev != NULL ? m->state[i] == DEV_REFUSED : (it->data == NULL || it->buffer == NULL)) { it->result = SLA_APIRESULT_INVALID_ARGUMENT; continue; }
    if ((ret = file_format(d, it->data, it->data_size, &f)) != SLA_APIRESULT_OK) { it->result = ret; continue; }
    if ((verdict = format_verdict(&f)) >= 0) { it->result = verdict; continue; }
    it->result = SLA_APIRESULT_OK;
    files[nf].item = i; files[nf].f = f; files[nf].bytes = it->data_size;
    if (dev != NULL) { m->state[i] = DEV_DECODED; }
    else { for (c = 0; c < f.C; c++) { if (it->buffer[c] == NULL) { files[nf].alone = 1; } } }     /* fails there as DecodeWhole does */
    nf++;
  }
  fmt_mark(d, &after);

  /* ---- files that share the launch parameters next to each other, each one's block chain walked */
  qsort(files, nf, sizeof(*files), slai_dec_file_cmp);
  for (npass = 0; npass < nf && !files[npass].alone; npass++) { }
  if (res) {
    /* on the device, all files in one launch (none is `alone` yet: that is decided for NULL planes, which device
     * destinations do not have) */
    if (res_count_walk(d, items, dev, files, nf, &nblocks) != 0) { rc = SLA_APIRESULT_NG; goto out; }
  }
  for (i = 0; i < nf && !res; i++) {
    const sla_hip_decode_item* it = &items[files[i].item];
    uint32_t b;
    if (files[i].alone) { continue; }
    files[i].first = nblocks;
    if (walk_chain(d, it->data, it->data_size, SLA_HEADER_SIZE, 0, files[i].f.total, it->buffer_num_samples, &nblocks, &files[i].walk_err) != 0) {
      rc = SLA_APIRESULT_NG; goto out;
    }
    files[i].nb = nblocks - files[i].first;
    for (b = files[i].first; b < nblocks; b++) {
      const sla_hip_dec_block* bl = &d->h_blocks[b];
      const uint32_t e = bl->smp_off + ((bl->flags & SLA_HIP_DEC_HEADER_ONLY) ? 0u : bl->num_samples);
      if (e > files[i].extent) { files[i].extent = e; }
    }
  }
  t_walk += now_ms() - t;

  /* ---- passes: runs of equal launch parameters, cut at SLA_HIP_DEC_BATCH_PASS sample-channels / DEC_BATCH_PASS_BYTES */
  for (p0 = 0; p0 < npass; ) {
    const uint32_t p1 = pass_cut(files, p0, npass);
    if (batch_pass(d, items, files + p0, m->done + p0, p1 - p0, &cl, dev, &t_up, &t_walk, &t_down, &kernel_ms) != 0) { rc = SLA_APIRESULT_NG; goto out; }
    passes++;
    p0 = p1;
  }

  /* ---- files decoded on their own; for device destinations decode_run leaves the finished planes in the handle's
   *      scratch and the emit kernel takes them from there */
  for (i = 0; i < nf; i++) {
    sla_hip_decode_item* it = &items[files[i].item];
    if (!files[i].alone) { continue; }
    if (res) {
      /* a resident file that needs a resync: its bytes come to host staging and decode_run reads them there */
      if (hbuf_reserve(&d->h_img, (size_t)it->data_size + 16) != 0
          || hipMemcpyAsync(d->h_img.ptr, dev->items[files[i].item].data, it->data_size, hipMemcpyDeviceToHost, d->stream) != hipSuccess
          || hipStreamSynchronize(d->stream) != hipSuccess) { rc = SLA_APIRESULT_NG; goto out; }
    }
    it->result = decode_run(d, res ? (const uint8_t*)d->h_img.ptr : it->data, it->data_size, NULL, NULL, 0, it->buffer, it->buffer_num_samples,
                            &it->output_num_samples, NULL);
    if (dev != NULL) {
      const int32_t* planes = (const int32_t*)d->d_planes.ptr;
      const uint64_t stride = run_plane_stride(files[i].f.total, it->buffer_num_samples);
      sla_hip_dec_emit e;
      uint32_t max_lim = 0, ne;
      t = now_ms();
      if (dev->wav != NULL) { rc = wav_emit_run(d, dev, items, &files[i], &it->output_num_samples, 1, 0, planes, stride, &cl, &kernel_ms); }
      else {
        ne = emit_entry(&e, &dev->items[files[i].item], dev->zero_fill, 0, it->output_num_samples, files[i].f.C, 0, 0, files[i].f.bps, &max_lim);
        rc = emit_run(d, planes, stride, &e, ne, max_lim, dev->format, &kernel_ms);
      }
      if (rc != 0) { rc = SLA_APIRESULT_NG; goto out; }
      t_down += now_ms() - t;
    }
  }

  /* ---- device destinations of items whose header gave a channel count but that were not decoded: the zero fill */
  if (dev != NULL && dev->zero_fill && zero_fill_pending(d, m, dev->items, num_items, dev->format, &kernel_ms, &t_down) != 0) { rc = SLA_APIRESULT_NG; }

out:
  call_close(d, &after, t0, t_up, t_walk, kernel_ms, t_down, passes);
  free(cl.v);
  return rc;
}

int sla_hip_decode_batch(struct SLADecoder* d, sla_hip_decode_item* items, uint32_t num_items)
{
  call_mem_t m;
  int rc;
  if (d == NULL || (items == NULL && num_items > 0)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_items == 0) { memset(d->timing, 0, sizeof(d->timing)); return 0; }
  if (call_mem_new(&m, num_items) != 0) { return SLA_APIRESULT_NG; }
  rc = batch_run(d, items, num_items, NULL, &m);
  free(m.base);
  return rc;
}

/* the channel count a file's header gives (its fields are delivered also when only the header CRC fails), 0 when none */
static uint32_t header_channels(const uint8_t* data, uint32_t data_size)
{
  struct SLAHeaderInfo h;
  SLAApiResult r;
  if (data == NULL) { return 0; }
  r = SLADecoder_DecodeHeader(data, data_size, &h);
  return (r == SLA_APIRESULT_OK || r == SLA_APIRESULT_DETECT_DATA_CORRUPTION) ? h.wave_format.num_channels : 0;
}

/* sla_internal.h: the region [0, C) x [0, n) of elements of esize bytes at p, element (c, i) at c * channel_stride +
 * i * sample_stride, may be accessed by a kernel.  A host pointer never passes: the runtime must report p as device memory
 * (of `device` when >= 0), and the region must lie inside p's allocation. */
int slai_device_region_ok(const void* p, uint32_t C, uint32_t n, uint64_t channel_stride, uint64_t sample_stride, uint64_t esize,
                          int device)
{
  hipPointerAttribute_t at;
  hipDeviceptr_t base = NULL;
  size_t size = 0;
  uint64_t bytes = 0, a, b, last, end;
  if ((uintptr_t)p % esize != 0) { return 0; }
  if (C > 0 && n > 0) {
    if (__builtin_mul_overflow((uint64_t)(C - 1), channel_stride, &a) || __builtin_mul_overflow((uint64_t)(n - 1), sample_stride, &b)
        || __builtin_add_overflow(a, b, &last) || __builtin_add_overflow(last, (uint64_t)1, &last) || __builtin_mul_overflow(last, esize, &bytes)
        || __builtin_add_overflow((uint64_t)(uintptr_t)p, bytes, &end)) { return 0; }
  }
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (at.type != hipMemoryTypeDevice || (device >= 0 && at.device != device)) { return 0; }
  if (bytes > 0) {
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if ((uintptr_t)p < (uintptr_t)base || end > (uint64_t)(uintptr_t)base + size) { return 0; }
  }
  return 1;
}

/* 1 when item `it` may be written: the argument checks of sla_hip_decode_batch_device, before any device work.  C is
 * the header's channel count; the region is [0, C) x [0, capacity) of elements of esize bytes. */
static int dst_region_ok(const sla_hip_decode_device_item* it, uint32_t C, uint64_t esize)
{
  if (it->data == NULL || it->dst == NULL || it->sample_stride == 0 || (C > 1 && it->channel_stride == 0)) { return 0; }
  return slai_device_region_ok(it->dst, C, it->capacity, it->channel_stride, it->sample_stride, esize, -1);
}

/* the handle's stream behind what the caller's stream holds at this moment */
static int order_behind(struct SLADecoder* d, sla_hip_stream_t stream)
{
  if (d->ev_order == NULL && hipEventCreateWithFlags(&d->ev_order, hipEventDisableTiming) != hipSuccess) { d->ev_order = NULL; return -1; }
  if (hipEventRecord(d->ev_order, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent(d->stream, d->ev_order, 0) != hipSuccess) { return -1; }
  return 0;
}

/* The opening of every device-destination call, on the arrays of m.  In: dv[i], the item as a device item, and ok[i], 0
 * where a check of the call's own has refused the item already.  In this order: resident sources are checked on the host
 * (ok[i]) before anything of an item is read; the handle's stream goes behind the caller's, so that nothing is read or
 * written before the caller's stream has reached the call; resident: the headers come home (*t_hdr: ms that took, else 0);
 * bi[i] becomes the item as batch_run reads it, its data the header brought home or the caller's host stream; esize != 0:
 * the destinations, elements of esize bytes, are checked with each header's channel count (chans[i]) before anything is
 * written.  state[i] is DEV_REFUSED where a check failed, else DEV_PENDING. */
static int call_open(struct SLADecoder* d, call_mem_t* m, uint32_t num_items, int resident, uint64_t esize, sla_hip_stream_t stream,
                     double* t_hdr)
{
  uint32_t i;
  *t_hdr = 0.0;
  if (drain(d) != 0) { return -1; }
  for (i = 0; i < num_items; i++) {
    m->src[i] = m->dv[i].data; m->size[i] = m->dv[i].data_size;
    if (resident && m->ok[i]) { m->ok[i] = (uint8_t)src_region_ok(m->dv[i].data, m->dv[i].data_size); }
  }
  if (order_behind(d, stream) != 0) { return -1; }
  if (resident) {
    const double t = now_ms();
    if (res_fetch_headers(d, m->src, m->size, m->ok, num_items) != 0) { return -1; }
    *t_hdr = now_ms() - t;
  }
  for (i = 0; i < num_items; i++) {
    const sla_hip_decode_device_item* it = &m->dv[i];
    m->bi[i].data = resident ? (const uint8_t*)d->h_hdr.ptr + (size_t)i * RES_HDR_SLOT : it->data;
    m->bi[i].data_size = it->data_size; m->bi[i].buffer_num_samples = it->capacity; m->bi[i].buffer = NULL;
    if (!m->ok[i]) { m->state[i] = DEV_REFUSED; continue; }
    if (esize == 0) { continue; }
    m->chans[i] = header_channels(m->bi[i].data, it->data_size);
    if (!dst_region_ok(it, m->chans[i], esize)) { m->state[i] = DEV_REFUSED; }
  }
  return 0;
}

static uint64_t pcm_esize(uint32_t sample_format) { return (sample_format == SLA_HIP_PCM_S16) ? 2u : 4u; }

/* sla_hip_decode_batch_device and sla_hip_decode_batch_resident */
static int decode_batch_dev(struct SLADecoder* d, sla_hip_decode_device_item* items, uint32_t num_items, uint32_t sample_format,
                            uint32_t flags, sla_hip_stream_t stream, int resident)
{
  call_mem_t m;
  dev_out_t dev;
  uint32_t i;
  int rc = SLA_APIRESULT_NG;
  double t_hdr;
  if (d == NULL || (items == NULL && num_items > 0) || sample_format > SLA_HIP_PCM_F32 || (flags & ~SLA_HIP_DEC_ZERO_FILL) != 0) {
    return SLA_APIRESULT_INVALID_ARGUMENT;
  }
  if (num_items == 0) { memset(d->timing, 0, sizeof(d->timing)); return 0; }
  if (call_mem_new(&m, num_items) != 0) { return SLA_APIRESULT_NG; }
  dev.items = items; dev.format = sample_format; dev.zero_fill = (flags & SLA_HIP_DEC_ZERO_FILL) ? 1u : 0u; dev.resident = resident; dev.wav = NULL;
  for (i = 0; i < num_items; i++) { m.dv[i] = items[i]; m.ok[i] = 1; }
  if (call_open(d, &m, num_items, resident, pcm_esize(sample_format), stream, &t_hdr) == 0) {
    rc = batch_run(d, m.bi, num_items, &dev, &m);
    d->timing[0] += (float)t_hdr;
    for (i = 0; i < num_items; i++) { items[i].result = m.bi[i].result; items[i].output_num_samples = m.bi[i].output_num_samples; }
  }
  free(m.base);
  return rc;
}

int sla_hip_decode_batch_device(struct SLADecoder* d, sla_hip_decode_device_item* items, uint32_t num_items, uint32_t sample_format,
                                uint32_t flags, sla_hip_stream_t stream)
{
  return decode_batch_dev(d, items, num_items, sample_format, flags, stream, 0);
}

int sla_hip_decode_batch_resident(struct SLADecoder* d, sla_hip_decode_device_item* items, uint32_t num_items,
                                  uint32_t sample_format, uint32_t flags, sla_hip_stream_t stream)
{
  return decode_batch_dev(d, items, num_items, sample_format, flags, stream, 1);
}

/* ---- sla_hip_salvage_resident (include/sla_hip.h): one resident stream decoded through damage ----
 * A resident call of one item (call_open on arrays of one) and one pass of one file (res_count_walk, pass_begin, the resident
 * stage, pass_kernels, emit_run), with three additions: the mode decision behind the count; the salvage scan in place of the
 * walk, behind the stage's gather half, when the chain is broken; and the silence (k_salvage_crc before the decode kernels,
 * k_dec_conceal before the emit).  The handle's format stays where the stream's header put it. */

/* one silent region: into the conceal list, the report and, while there is room, the caller's ranges */
static void salvage_note(sla_hip_salvage_report* rep, sla_hip_salvage_range* ranges, uint32_t range_capacity, sla_hip_dec_conceal* cl,
                         uint32_t* ncl, uint32_t* max_len, uint32_t start, uint32_t length, uint32_t reason)
{
  if (length == 0) { return; }
  cl[*ncl].smp_off = start; cl[*ncl].num_samples = length; (*ncl)++;
  if (length > *max_len) { *max_len = length; }
  if (rep->num_ranges < range_capacity) {
    ranges[rep->num_ranges].start = start; ranges[rep->num_ranges].length = length; ranges[rep->num_ranges].reason = reason;
  }
  rep->num_ranges++;
  rep->samples_lost += length;
}

/* the salvage scan of one stream queued on the handle's stream, its result on the way home to `home` (page-locked) */
static int salvage_scan_launch(struct SLADecoder* d, const sla_hip_dec_walk_file* wf, uint32_t C, uint32_t cap, uint32_t slot,
                               sla_hip_dec_block* db, uint64_t* dend, uint32_t* dcrc, sla_hip_salvage_scan* home)
{
  sla_hip_salvage_scan* dres = (sla_hip_salvage_scan*)d->d_wres.ptr + slot;
  BRC(sla_hip_launch_dec_salvage_scan(wf, C, d->cfg.max_num_block_samples, dres, db, dend, dcrc, cap, d->d_wide.ptr, d->stream));
  BCHK(hipMemcpyAsync(home, dres, sizeof(*home), hipMemcpyDeviceToHost, d->stream));
  return 0;
}

int sla_hip_salvage_resident(struct SLADecoder* d, const uint8_t* d_data, uint32_t data_size, void* dst, uint64_t channel_stride,
                             uint64_t sample_stride, uint32_t capacity, uint32_t sample_format, sla_hip_salvage_report* report,
                             sla_hip_salvage_range* ranges, uint32_t range_capacity, sla_hip_stream_t stream)
{
  sla_hip_decode_device_item di;
  sla_hip_decode_item bi;
  sla_hip_salvage_scan* scan;           /* [0] the count-mode scan, [1] the write-mode scan (page-locked) */
  sla_hip_dec_walk_file wf;
  sla_hip_dec_conceal* cl;
  sla_hip_dec_emit e;
  dev_out_t dev;
  call_mem_t m;
  bfile_t file;
  dec_format_t f;
  pass_t p; stage_t st;
  SLAApiResult ret;
  const uint8_t *src, *hdr;
  uint32_t* hbad;
  uint8_t ok = 1, state = DEV_PENDING;
  uint32_t C, N, nb = 0, nblocks = 0, mode, k, ncl = 0, max_len = 0, max_lim = 0, P = 0, scan_cap = 0, size, chans = 0;
  uint64_t span, img_bytes;
  int verdict;
  float kernel_ms = 0.0f;
  double t0 = now_ms(), t_up = 0.0, t_walk = 0.0, t_emit, t_hdr;

  if (d == NULL || d_data == NULL || dst == NULL || report == NULL || sample_format > SLA_HIP_PCM_F32
      || (ranges == NULL && range_capacity > 0)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  memset(report, 0, sizeof(*report));
  memset(d->timing, 0, sizeof(d->timing));
  memset(d->walk_stats, 0, sizeof(d->walk_stats));
  memset(&di, 0, sizeof(di));
  di.data = d_data; di.dst = dst; di.channel_stride = channel_stride; di.sample_stride = sample_stride;
  di.data_size = data_size; di.capacity = capacity;
  /* the opening of a resident call, on arrays of one item */
  memset(&m, 0, sizeof(m));
  m.dv = &di; m.bi = &bi; m.src = &src; m.size = &size; m.ok = &ok; m.state = &state; m.chans = &chans;
  if (call_open(d, &m, 1, 1, pcm_esize(sample_format), stream, &t_hdr) != 0) { return SLA_APIRESULT_NG; }
  if (state == DEV_REFUSED) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  hdr = (const uint8_t*)d->h_hdr.ptr;
  if ((ret = file_format(d, hdr, data_size, &f)) != SLA_APIRESULT_OK) { return ret; }
  if ((verdict = format_verdict(&f)) >= 0) { return verdict; }
  if (!lms_order_ok(f.lms)) { return SLA_APIRESULT_FAILED_TO_SYNTHESIZE; }
  C = f.C; N = f.total;
  if (capacity < N) { return SLA_APIRESULT_INSUFFICIENT_BUFFER_SIZE; }

  /* ---- the chain, counted with capacity N: intact when it accounts for exactly N samples */
  memset(&bi, 0, sizeof(bi)); memset(&dev, 0, sizeof(dev)); memset(&file, 0, sizeof(file));
  bi.data = hdr; bi.data_size = data_size; bi.buffer_num_samples = N;
  dev.items = &di; dev.format = sample_format; dev.resident = 1;
  file.f = f; file.bytes = data_size;
  if (res_count_walk(d, &bi, &dev, &file, 1, &nblocks) != 0) { return SLA_APIRESULT_NG; }
  mode = (file.walk_err == SLA_APIRESULT_OK && file.extent == N) ? 1u : 2u;
  report->mode = mode;
  if (hbuf_reserve(&d->h_wide, (sizeof(sla_hip_dec_wide_info) + sizeof(sla_hip_dec_walk_result)) * RES_WIDE_MAX + 2 * sizeof(*scan)) != 0) {
    return SLA_APIRESULT_NG;
  }
  scan = (sla_hip_salvage_scan*)((uint8_t*)d->h_wide.ptr + (sizeof(sla_hip_dec_wide_info) + sizeof(sla_hip_dec_walk_result)) * RES_WIDE_MAX);
  memset(&wf, 0, sizeof(wf));
  wf.src = d_data; wf.data_size = data_size; wf.total = N; wf.capacity = N;
  if (mode == 1u) {
    nb = file.nb;
  } else {
    /* the scan in count mode; nodes beyond the handle's capacity: once more with the exact count */
    uint32_t cap = slai_dec_wide_capacity(d->wide_nodes, data_size), attempt;
    for (attempt = 0; ; attempt++) {
      if (dbuf_reserve(&d->d_wide, (size_t)SLA_HIP_DEC_SALVAGE_SCRATCH_BYTES(data_size, cap)) != 0
          || dbuf_reserve(&d->d_wres, 2 * sizeof(*scan)) != 0) { return SLA_APIRESULT_NG; }
      if (salvage_scan_launch(d, &wf, C, cap, 0, NULL, NULL, NULL, &scan[0]) != 0
          || hipStreamSynchronize(d->stream) != hipSuccess) { return SLA_APIRESULT_NG; }
      d->walk_stats[0]++; d->walk_stats[2] += scan[0].nodes; d->walk_stats[3] += 2 * sla_hip_dec_wide_rounds(data_size, cap);
      if (!scan[0].overflow) { break; }
      d->walk_stats[1]++;
      if (attempt == 1 || scan[0].nodes == 0) { return SLA_APIRESULT_NG; }
      cap = scan[0].nodes;
    }
    P = scan[0].prefix_blocks;
    nb = P + scan[0].suffix_blocks;
    report->prefix_blocks = P; report->suffix_blocks = scan[0].suffix_blocks; report->suffix_byte = scan[0].suffix_byte;
    report->suffix_sample = (scan[0].suffix_byte != 0) ? N - scan[0].suffix_samples : 0;
    report->nodes = scan[0].nodes; report->sound_nodes = scan[0].sound_nodes;
    wf.max_rows = nb;
    scan_cap = cap;
  }
  t_walk = now_ms() - t0;

  /* ---- the pass: one file of nb rows and N samples, image at 0, planes at 0 */
  file.first = 0; file.nb = nb; file.extent = N;
  if (pass_begin(d, &file, 1, &p) != 0
      || hbuf_reserve(&d->h_ptab, sizeof(uint32_t) * (size_t)nb + sizeof(*cl) * ((size_t)nb + 1)) != 0
      || host_tables_reserve(d, nb) != 0) { return SLA_APIRESULT_NG; }
  span = p.span; img_bytes = p.img_bytes;
  hbad = (uint32_t*)d->h_ptab.ptr;
  cl = (sla_hip_dec_conceal*)(hbad + nb);
  if (nb > 0 && mode == 1u) {
    sla_hip_dec_block* db = (sla_hip_dec_block*)d->d_blocks.ptr;
    uint32_t* dbad = (uint32_t*)d->d_crcf.ptr + nb;
    if (res_stage_pass(d, &bi, &dev, &file, 1, &p, &st) != 0
        || sla_hip_launch_salvage_crc((const uint8_t*)d->d_image.ptr, db, (const uint32_t*)d->d_crcf.ptr, nb, dbad, d->stream) != 0
        || hipMemcpyAsync(hbad, dbad, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost, d->stream) != hipSuccess
        || pass_kernels(d, &f, nb, 0, img_bytes, span, &kernel_ms) != 0
        || res_finish_pass(d, &st, &file, 1, &t_up, &t_walk) != 0) { return SLA_APIRESULT_NG; }
  } else if (nb > 0) {
    sla_hip_dec_block* db = (sla_hip_dec_block*)d->d_blocks.ptr;
    if (stage_tables(d, 1, sizeof(sla_hip_dec_walk_file), sizeof(sla_hip_dec_walk_result), &st) != 0) { return SLA_APIRESULT_NG; }
    st.gt->src = d_data; st.gt->dst_off = 0; st.gt->bytes = data_size;
    if (stage_gather(d, &st, 1, data_size, img_bytes) != 0
        || salvage_scan_launch(d, &wf, C, scan_cap, 1, db, (uint64_t*)(db + nb), (uint32_t*)d->d_crcf.ptr, &scan[1]) != 0
        || hipMemcpyAsync(d->h_blocks, db, sizeof(*db) * (size_t)nb, hipMemcpyDeviceToHost, d->stream) != hipSuccess
        || hipMemsetAsync(d->d_info.ptr, 0, sizeof(sla_hip_dec_info) * nb, d->stream) != hipSuccess
        || pass_kernels(d, &f, nb, 0, img_bytes, span, &kernel_ms) != 0) { return SLA_APIRESULT_NG; }
    d->walk_stats[3] += 2 * sla_hip_dec_wide_rounds(data_size, scan_cap);
    /* a stream that changed between the two scans fails the call, as a walk that differs from its count does */
    if (memcmp(&scan[0], &scan[1], sizeof(scan[0])) != 0) { return SLA_APIRESULT_NG; }
    memset(hbad, 0, sizeof(uint32_t) * nb);
  }

  /* ---- every row examined with the whole-file decode's criteria; what fails becomes silence */
  for (k = 0; k < nb; k++) {
    const sla_hip_dec_block* b = &d->h_blocks[k];
    const sla_hip_dec_info* in = &d->h_info[k];
    uint32_t reason = 0;
    if (mode == 2u && k == P) { salvage_note(report, ranges, range_capacity, cl, &ncl, &max_len, scan[0].prefix_samples, N - scan[0].suffix_samples - scan[0].prefix_samples, SLA_HIP_SALVAGE_GAP); }
    if (hbad[k]) { reason = SLA_HIP_SALVAGE_CRC; }
    else if (in->type > 2 || in->overrun || in->used_bytes != b->byte_len) { reason = SLA_HIP_SALVAGE_UNDECODABLE; }
    if (reason == 0) { report->blocks_decoded++; continue; }
    report->blocks_concealed++;
    salvage_note(report, ranges, range_capacity, cl, &ncl, &max_len, b->smp_off, b->num_samples, reason);
  }
  if (mode == 2u && P == nb) { salvage_note(report, ranges, range_capacity, cl, &ncl, &max_len, scan[0].prefix_samples, N - scan[0].suffix_samples - scan[0].prefix_samples, SLA_HIP_SALVAGE_GAP); }

  /* ---- silence into the planes, then the emit of all N samples */
  t_emit = now_ms();
  if (ncl > 0) {
    if (dbuf_reserve(&d->d_src, sizeof(*cl) * ncl) != 0
        || hipMemcpyAsync(d->d_src.ptr, cl, sizeof(*cl) * ncl, hipMemcpyHostToDevice, d->stream) != hipSuccess
        || sla_hip_launch_dec_conceal((int32_t*)d->d_planes.ptr, span, C, (const sla_hip_dec_conceal*)d->d_src.ptr, ncl, max_len, d->stream) != 0) {
      return SLA_APIRESULT_NG;
    }
  }
  if (emit_entry(&e, &di, 0, 0, N, C, f.ms, 32u - f.bps + f.lshift, f.bps, &max_lim) != 0
      && emit_run(d, (const int32_t*)d->d_planes.ptr, span, &e, 1, max_lim, sample_format, &kernel_ms) != 0) { return SLA_APIRESULT_NG; }
  call_close(d, NULL, t0, t_up, t_walk, kernel_ms, now_ms() - t_emit, 1);
  return (report->blocks_concealed != 0 || report->samples_lost != 0) ? SLA_APIRESULT_DETECT_DATA_CORRUPTION : SLA_APIRESULT_OK;
}

/* sla_hip_decode_wav_batch / sla_hip_decode_wav_batch_resident (include/sla_hip.h): the items become device items whose
 * capacity is the header's num_samples and go through batch_run with the WAV emit as the last leg (wav_out_t). */
static int decode_wav_impl(struct SLADecoder* d, sla_hip_wav_item* items, uint32_t num_items, int resident, sla_hip_stream_t stream)
{
  call_mem_t m;
  sla_hip_decode_item* bi;
  sla_hip_decode_device_item* di;
  dev_out_t dev;
  wav_out_t w;
  uint32_t i;
  int rc = 0;
  double t_hdr = 0.0;
  if (d == NULL || (items == NULL && num_items > 0)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_items == 0) { memset(d->timing, 0, sizeof(d->timing)); return 0; }
  if (call_mem_new(&m, num_items) != 0) { return SLA_APIRESULT_NG; }
  bi = m.bi; di = m.dv;
  memset(&dev, 0, sizeof(dev)); memset(&w, 0, sizeof(w));
  dev.items = di; dev.resident = resident; dev.wav = &w;
  w.items = items; w.host = !resident; w.hold = m.hold; w.rate = m.rate; w.delivered = m.delivered;
  for (i = 0; i < num_items; i++) {
    const sla_hip_wav_item* it = &items[i];
    di[i].data = it->src; di[i].data_size = it->src_size; di[i].dst = it->dst; di[i].channel_stride = 1; di[i].sample_stride = 1;
    m.ok[i] = (it->src != NULL);
    items[i].output_size = 0; items[i].num_samples = 0;
  }
  /* the destinations are this call's to check: they hold what each header says */
  if (call_open(d, &m, num_items, resident, 0, stream, &t_hdr) != 0) { rc = SLA_APIRESULT_NG; goto out; }
  for (i = 0; i < num_items; i++) {
    const sla_hip_wav_item* it = &items[i];
    struct SLAHeaderInfo h;
    SLAApiResult r;
    uint64_t bytes;
    if (m.state[i] == DEV_REFUSED || it->dst == NULL) { m.state[i] = DEV_REFUSED; continue; }
    r = SLADecoder_DecodeHeader(bi[i].data, it->src_size, &h);
    if (r != SLA_APIRESULT_OK) { continue; }                    /* (batch_run gives the header's code) */
    bi[i].buffer_num_samples = di[i].capacity = h.num_samples;
    m.chans[i] = h.wave_format.num_channels; w.rate[i] = h.wave_format.sampling_rate;
    if (!(h.wave_format.bit_per_sample == 8 || h.wave_format.bit_per_sample == 16 || h.wave_format.bit_per_sample == 24
          || h.wave_format.bit_per_sample == 32)) { w.hold[i] = SLA_APIRESULT_INVALID_HEADER_FORMAT; continue; }
    bytes = (uint64_t)SLA_HIP_WAV_HEADER_BYTES + (uint64_t)h.num_samples * h.wave_format.num_channels * (h.wave_format.bit_per_sample / 8);
    if (bytes > 0xFFFFFFFFull || bytes > it->dst_capacity) { w.hold[i] = SLA_APIRESULT_INSUFFICIENT_BUFFER_SIZE; continue; }
    m.fbytes[i] = (uint32_t)bytes; m.wbits[i] = h.wave_format.bit_per_sample;
    if (resident && !slai_device_region_ok(it->dst, 1, 2, 0, bytes - 1, 1, -1)) { m.state[i] = DEV_REFUSED; }
  }
  rc = batch_run(d, bi, num_items, &dev, &m);
  d->timing[0] += (float)t_hdr;
  for (i = 0; i < num_items; i++) {
    items[i].result = (bi[i].result == SLA_APIRESULT_OK && w.hold[i] != 0) ? w.hold[i] : bi[i].result;
    if (rc == 0 && !w.delivered[i] && items[i].result == SLA_APIRESULT_OK && m.fbytes[i] == SLA_HIP_WAV_HEADER_BYTES) {
      /* a file of no samples joins no pass (format_verdict): its WAV is the header alone, written here */
      uint8_t hdr[SLA_HIP_WAV_HEADER_BYTES];
      sla_hip_wav_info info;
      memset(&info, 0, sizeof(info));
      info.num_channels = m.chans[i]; info.bits_per_sample = m.wbits[i]; info.sampling_rate = w.rate[i]; info.data_off = SLA_HIP_WAV_HEADER_BYTES;
      (void)sla_hip_wav_header(&info, hdr);
      if (!resident) { memcpy(items[i].dst, hdr, sizeof(hdr)); w.delivered[i] = 1; }
      else if (hipMemcpyAsync(items[i].dst, hdr, sizeof(hdr), hipMemcpyHostToDevice, d->stream) == hipSuccess
               && hipStreamSynchronize(d->stream) == hipSuccess) { w.delivered[i] = 1; }
      else { rc = SLA_APIRESULT_NG; }
    }
    if (rc == 0 && w.delivered[i]) {
      items[i].num_samples = bi[i].output_num_samples;
      items[i].output_size = m.fbytes[i];
    } else if (items[i].result == SLA_APIRESULT_OK) {
      items[i].result = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE;   /* (an OK decode that stopped short of the header's samples) */
    }
  }
out:
  free(m.base);
  return rc;
}

int sla_hip_decode_wav_batch(struct SLADecoder* d, sla_hip_wav_item* items, uint32_t num_items)
{
  return decode_wav_impl(d, items, num_items, 0, NULL);
}

int sla_hip_decode_wav_batch_resident(struct SLADecoder* d, sla_hip_wav_item* items, uint32_t num_items, sla_hip_stream_t stream)
{
  return decode_wav_impl(d, items, num_items, 1, stream);
}

int sla_hip_resident_headers(struct SLADecoder* d, const uint8_t* const* d_data, const uint32_t* data_size, uint32_t num,
                             struct SLAHeaderInfo* headers, int32_t* results, sla_hip_stream_t stream)
{
  uint8_t* ok;
  uint32_t i;
  int rc = 0;
  if (d == NULL || (num > 0 && (d_data == NULL || data_size == NULL || headers == NULL || results == NULL))) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num == 0) { return 0; }
  ok = (uint8_t*)calloc(num, 1);
  if (ok == NULL) { return SLA_APIRESULT_NG; }
  for (i = 0; i < num; i++) { ok[i] = (uint8_t)src_region_ok(d_data[i], data_size[i]); }
  if (drain(d) != 0 || order_behind(d, stream) != 0 || res_fetch_headers(d, d_data, data_size, ok, num) != 0) { rc = SLA_APIRESULT_NG; goto out; }
  for (i = 0; i < num; i++) {
    memset(&headers[i], 0, sizeof(headers[i]));
    results[i] = ok[i] ? (int32_t)SLADecoder_DecodeHeader((const uint8_t*)d->h_hdr.ptr + (size_t)i * RES_HDR_SLOT, data_size[i], &headers[i])
                       : (int32_t)SLA_APIRESULT_INVALID_ARGUMENT;
  }
out:
  free(ok);
  return rc;
}

/* ------------------------------------------------------------------------------------------------------------
 * sla_hip_decode_windows_resident (include/sla_hip.h): sla_hip_decode_batch_resident for a window of samples per item.
 * The opening (call_open), the grouping and the pass caps (pass_cut), the layout and reserve (pass_begin), the resident
 * stage, the kernels, the examination criteria, the emit and the zero fill are that call's code.  The window's own: the
 * walk (k_dec_walk_window: only the blocks the window overlaps get a row), so that a file's bytes in a pass are the byte
 * range of its kept blocks and not its whole stream; the refusal of bad hints and of a start behind the file; and the
 * all-or-nothing outcome: no samples before a failing block, no resync.
 * ------------------------------------------------------------------------------------------------------------ */
static void win_walk_entry(sla_hip_dec_window_file* w, const sla_hip_decode_window_item* it, uint32_t total)
{
  memset(w, 0, sizeof(*w));
  w->src = it->data; w->data_size = it->data_size; w->total = total; w->win_start = it->start; w->win_len = it->length;
  w->seek_byte = it->seek_byte; w->seek_sample = it->seek_sample;
}

/* The count-mode window walk of files[0, nf): one launch, one small copy home; wres[item] is each item's result, from
 * which every file's first / nb / walk_err / extent / bytes are set, and *nblocks; makes room for that many rows in the host tables. */
static int win_count_walk(struct SLADecoder* d, const sla_hip_decode_window_item* items, bfile_t* files, uint32_t nf,
                          sla_hip_dec_window_result* wres, uint32_t* nblocks)
{
  sla_hip_dec_window_file* wt;
  sla_hip_dec_window_result* wr;
  uint64_t total = 0;
  uint32_t i;
  if (nf == 0) { return 0; }
  if (hbuf_reserve(&d->h_src, (sizeof(*wt) + sizeof(*wr)) * (size_t)nf) != 0 || dbuf_reserve(&d->d_src, sizeof(*wt) * (size_t)nf) != 0
      || dbuf_reserve(&d->d_wres, sizeof(*wr) * (size_t)nf) != 0) { return -1; }
  wt = (sla_hip_dec_window_file*)d->h_src.ptr;
  wr = (sla_hip_dec_window_result*)(wt + nf);
  for (i = 0; i < nf; i++) { win_walk_entry(&wt[i], &items[files[i].item], files[i].f.total); }
  BCHK(hipMemcpyAsync(d->d_src.ptr, wt, sizeof(*wt) * nf, hipMemcpyHostToDevice, d->stream));
  BRC(sla_hip_launch_dec_walk_window((const sla_hip_dec_window_file*)d->d_src.ptr, nf, d->cfg.max_num_block_samples,
                                     (sla_hip_dec_window_result*)d->d_wres.ptr, NULL, NULL, NULL, d->stream));
  BCHK(hipMemcpyAsync(wr, d->d_wres.ptr, sizeof(*wr) * nf, hipMemcpyDeviceToHost, d->stream));
  BCHK(hipStreamSynchronize(d->stream));
  for (i = 0; i < nf; i++) {
    /* a walk that kept blocks ends behind where it began, in bytes and in samples: anything else is not this kernel's */
    if (wr[i].end_byte < wr[i].first_byte || wr[i].end_sample < wr[i].first_sample) { return -1; }
    wres[files[i].item] = wr[i];
    files[i].first = (uint32_t)total; files[i].nb = wr[i].num_blocks;
    files[i].walk_err = (SLAApiResult)wr[i].stop; files[i].extent = wr[i].end_sample - wr[i].first_sample;
    files[i].bytes = wr[i].end_byte - wr[i].first_byte;
    total += wr[i].num_blocks;
  }
  if (total > 0xFFFFFFFFull || host_tables_reserve(d, (uint32_t)total) != 0) { return -1; }
  *nblocks = (uint32_t)total;
  return 0;
}

/* The first failure among a file's kept blocks, in file order, by examine_blocks' criteria; a body that does not end
 * where its size field says, or a reader that ran off the end, is DETECT_DATA_CORRUPTION here: windows do no resync.
 * SLA_APIRESULT_NG, which neither the walk nor examine_blocks gives, marks "no failure" on the way. */
static SLAApiResult win_examine(const struct SLADecoder* d, const bfile_t* fl, int lms_ok)
{
  const uint32_t* cf = d->h_crcf + fl->first;
  const sla_hip_dec_block* bl = d->h_blocks + fl->first;
  const sla_hip_dec_info* in = d->h_info + fl->first;
  uint32_t j = 0, done = 0, off = 0, pos = 0;
  SLAApiResult r;
  while (j < fl->nb && !in[j].overrun) { j++; }
  if (examine_blocks(d, cf, bl, in, j, lms_ok, SLA_APIRESULT_NG, NULL, &done, &off, &pos, &r)) { return SLA_APIRESULT_DETECT_DATA_CORRUPTION; }
  if (r != SLA_APIRESULT_NG) { return r; }
  if (j < fl->nb) {
    /* block j's reader ran off the end: the criteria that come before the size comparison decide first */
    if (!examine_blocks(d, cf + j, bl + j, in + j, 1, lms_ok, SLA_APIRESULT_NG, NULL, &done, &off, &pos, &r) && r != SLA_APIRESULT_NG) { return r; }
    return SLA_APIRESULT_DETECT_DATA_CORRUPTION;
  }
  return fl->walk_err;
}

/* One pass of windows: files[0, nf) share the launch parameters, their rows are d->h_blocks[files[0].first ...].
 * dv[item] is the item as a device item of the resident call (capacity = length).  Returns -1 on a device or allocation
 * failure, or when the write-mode walk differs from the count. */
static int win_pass(struct SLADecoder* d, sla_hip_decode_window_item* items, const sla_hip_decode_device_item* dv, bfile_t* files,
                    uint32_t nf, const sla_hip_dec_window_result* wres, uint32_t format, uint32_t zero_fill, double* t_gather,
                    double* t_walk, double* t_down, float* kernel_ms)
{
  const dec_format_t* f = &files[0].f;
  const uint32_t C = f->C, first = files[0].first;
  const int lms_ok = lms_order_ok(f->lms);
  uint64_t img_bytes, span;
  uint32_t nb, i, ne = 0, max_lim = 0;
  sla_hip_dec_emit* et;
  pass_t p;
  double t;

  if (pass_begin(d, files, nf, &p) != 0 || hbuf_reserve(&d->h_ptab, sizeof(sla_hip_dec_emit) * (size_t)nf) != 0) { return -1; }
  img_bytes = p.img_bytes; span = p.span; nb = p.nb;
  for (i = 0; i < nf; i++) { d->win_stats[2] += files[i].bytes; }
  d->win_stats[3] += p.regions;

  if (nb > 0) {
    /* ---- the stage: the byte ranges gathered into the pass image, the walk in write mode; then the kernels */
    stage_t st;
    sla_hip_dec_gather* gt;
    sla_hip_dec_window_file* wt;
    const sla_hip_dec_window_result* wr;
    uint32_t ng = 0, max_bytes = 0;
    if (stage_tables(d, nf, sizeof(*wt), sizeof(*wr), &st) != 0) { return -1; }
    gt = st.gt;
    wt = (sla_hip_dec_window_file*)st.wt;
    wr = (const sla_hip_dec_window_result*)st.wr;
    for (i = 0; i < nf; i++) {
      const sla_hip_decode_window_item* it = &items[files[i].item];
      const sla_hip_dec_window_result* r = &wres[files[i].item];
      const uint32_t range = files[i].bytes;
      if (range > 0) {
        gt[ng].src = it->data + r->first_byte; gt[ng].dst_off = files[i].img_off; gt[ng].bytes = range; gt[ng].reserved = 0;
        ng++;
        if (range > max_bytes) { max_bytes = range; }
      }
      win_walk_entry(&wt[i], it, files[i].f.total);
      wt[i].img_off = files[i].img_off; wt[i].range_bytes = range; wt[i].base_byte = r->first_byte; wt[i].base_sample = r->first_sample;
      wt[i].plane_off = (uint32_t)files[i].plane_off; wt[i].first = files[i].first - first; wt[i].max_rows = files[i].nb;
    }
    if (stage_queue(d, &st, files, nf, 1, ng, max_bytes, &p) != 0 || pass_kernels(d, f, nb, first, img_bytes, span, kernel_ms) != 0) { return -1; }
    stage_times(d, t_gather, t_walk);
    /* a file whose chain changed since it was counted fails the call */
    for (i = 0; i < nf; i++) { if (memcmp(&wr[i], &wres[files[i].item], sizeof(wr[i])) != 0) { return -1; } }
  }

  /* ---- every window examined on its own; delivered whole from its first sample in the region, or not at all */
  t = now_ms();
  et = (sla_hip_dec_emit*)d->h_ptab.ptr;
  for (i = 0; i < nf; i++) {
    sla_hip_decode_window_item* it = &items[files[i].item];
    const uint32_t rest = files[i].f.total - it->start;
    uint32_t done = 0;
    it->result = win_examine(d, &files[i], lms_ok);
    if (it->result == SLA_APIRESULT_OK) { done = (it->length < rest) ? it->length : rest; }
    it->output_num_samples = done;
    ne += emit_entry(et + ne, &dv[files[i].item], zero_fill, files[i].plane_off + (it->start - wres[files[i].item].first_sample), done, C,
                     f->ms, 32u - f->bps + f->lshift, f->bps, &max_lim);
  }
  if (emit_run(d, (const int32_t*)d->d_planes.ptr, span, et, ne, max_lim, format, kernel_ms) != 0) { return -1; }
  *t_down += now_ms() - t;
  return 0;
}

int sla_hip_decode_windows_resident(struct SLADecoder* d, sla_hip_decode_window_item* items, uint32_t num_items,
                                    uint32_t sample_format, uint32_t flags, sla_hip_stream_t stream)
{
  const uint32_t zero_fill = (flags & SLA_HIP_DEC_ZERO_FILL) ? 1u : 0u;
  call_mem_t m;
  bfile_t* files;
  fmt_mark_t after;
  uint32_t nf = 0, nblocks = 0, passes = 0, i, p0;
  int rc = 0;
  float kernel_ms = 0.0f;
  double t0 = now_ms(), t_gather = 0.0, t_walk = 0.0, t_down = 0.0, t;
  if (d == NULL || (items == NULL && num_items > 0) || sample_format > SLA_HIP_PCM_F32 || (flags & ~SLA_HIP_DEC_ZERO_FILL) != 0) {
    return SLA_APIRESULT_INVALID_ARGUMENT;
  }
  memset(d->timing, 0, sizeof(d->timing));
  memset(d->win_stats, 0, sizeof(d->win_stats));
  if (num_items == 0) { return 0; }
  fmt_mark(d, &after);
  if (call_mem_new(&m, num_items) != 0) { rc = SLA_APIRESULT_NG; goto out; }
  files = m.files;
  /* the items as device items of the resident call (capacity = length); a bad hint refuses an item as a bad source does */
  for (i = 0; i < num_items; i++) {
    const sla_hip_decode_window_item* it = &items[i];
    sla_hip_decode_device_item* dv = &m.dv[i];
    dv->data = it->data; dv->dst = it->dst; dv->channel_stride = it->channel_stride; dv->sample_stride = it->sample_stride;
    dv->data_size = it->data_size; dv->capacity = it->length;
    m.ok[i] = (uint8_t)((it->seek_byte == 0 ? it->seek_sample == 0 : it->seek_byte >= SLA_HEADER_SIZE) && it->seek_sample <= it->start);
  }
  if (call_open(d, &m, num_items, 1, pcm_esize(sample_format), stream, &t_gather) != 0) { rc = SLA_APIRESULT_NG; goto out; }

  /* ---- headers in item order, as in batch_run */
  t = now_ms();
  for (i = 0; i < num_items; i++) {
    sla_hip_decode_window_item* it = &items[i];
    const uint8_t* hdr = m.bi[i].data;
    dec_format_t f;
    SLAApiResult ret;
    int verdict;
    it->output_num_samples = 0; it->first_block_byte = 0; it->first_block_sample = 0;
    it->result = SLA_APIRESULT_INVALID_ARGUMENT;
    if (m.state[i] == DEV_REFUSED) { continue; }
    if ((ret = file_format(d, hdr, it->data_size, &f)) != SLA_APIRESULT_OK) { it->result = ret; continue; }
    if (it->start > f.total) { m.state[i] = DEV_REFUSED; continue; }
    if ((verdict = format_verdict(&f)) >= 0) { it->result = verdict; continue; }
    it->result = SLA_APIRESULT_OK;
    if (it->start == f.total || it->length == 0) { continue; }       /* OK, no samples: nothing is decoded */
    files[nf].item = i; files[nf].f = f; m.state[i] = DEV_DECODED;
    nf++;
  }
  fmt_mark(d, &after);

  /* ---- windows that share the launch parameters next to each other, every chain walked up to its window's end */
  qsort(files, nf, sizeof(*files), slai_dec_file_cmp);
  if (win_count_walk(d, items, files, nf, m.wres, &nblocks) != 0) { rc = SLA_APIRESULT_NG; goto out; }
  for (i = 0; i < nf; i++) {
    const sla_hip_dec_window_result* r = &m.wres[files[i].item];
    items[files[i].item].first_block_byte = r->first_byte; items[files[i].item].first_block_sample = r->first_sample;
    d->win_stats[0] += r->skipped; d->win_stats[1] += r->num_blocks;
  }
  t_walk += now_ms() - t;

  /* ---- passes: batch_run's caps, an item costing its byte range and the samples of its kept blocks */
  for (p0 = 0; p0 < nf; ) {
    const uint32_t p1 = pass_cut(files, p0, nf);
    if (win_pass(d, items, m.dv, files + p0, p1 - p0, m.wres, sample_format, zero_fill, &t_gather, &t_walk, &t_down, &kernel_ms) != 0) {
      rc = SLA_APIRESULT_NG; goto out;
    }
    passes++;
    p0 = p1;
  }

  /* ---- destinations of items whose header gave a channel count but of which nothing was decoded: the zero fill */
  if (zero_fill && zero_fill_pending(d, &m, m.dv, num_items, sample_format, &kernel_ms, &t_down) != 0) { rc = SLA_APIRESULT_NG; }

out:
  call_close(d, &after, t0, t_gather, t_walk, kernel_ms, t_down, passes);
  free(m.base);
  return rc;
}

/* ------------------------------------------------------------------------------------------------------------
 * The block index from device bytes (include/sla_hip.h; the host builder and everything else of sla_hip_index is
 * sla_dec_index.c): the header gather, then the whole-file walk with capacity = the header's num_samples, no cap on the
 * block length and no CRC rows, in count and in write mode -- wide for a long stream, on a lane after an overflow.
 * ------------------------------------------------------------------------------------------------------------ */
#define IDX_MAX_BLOCK_SAMPLES 65535u     /* the format's: a 16-bit field */

/* one walk of wf (a host struct) queued on the handle's stream: wide, or on one lane; write: its wf->max_rows rows go to
 * d->d_blocks (rows, then ends) and d->d_crcf */
static int idx_walk_launch(struct SLADecoder* d, const sla_hip_dec_walk_file* wf, int wide, int write)
{
  sla_hip_dec_block* db = write ? (sla_hip_dec_block*)d->d_blocks.ptr : NULL;
  uint64_t* dend = write ? (uint64_t*)(db + wf->max_rows) : NULL;
  uint32_t* dcrc = write ? (uint32_t*)d->d_crcf.ptr : NULL;
  if (wide) {
    BRC(sla_hip_launch_dec_walk_wide(wf, IDX_MAX_BLOCK_SAMPLES, 0, (sla_hip_dec_walk_result*)d->d_wres.ptr, db, dend, dcrc,
                                     slai_dec_wide_capacity(d->wide_nodes, wf->data_size), d->d_wide.ptr, d->stream));
  } else {
    memcpy(d->h_src.ptr, wf, sizeof(*wf));
    BCHK(hipMemcpyAsync(d->d_src.ptr, d->h_src.ptr, sizeof(*wf), hipMemcpyHostToDevice, d->stream));
    BRC(sla_hip_launch_dec_walk((const sla_hip_dec_walk_file*)d->d_src.ptr, 1, IDX_MAX_BLOCK_SAMPLES, 0, (sla_hip_dec_walk_result*)d->d_wres.ptr,
                                db, dend, dcrc, d->stream));
  }
  return 0;
}

int sla_hip_index_build_resident(struct SLADecoder* d, const uint8_t* d_data, uint32_t data_size, sla_hip_stream_t stream,
                                 sla_hip_index** index)
{
  const uint32_t head_bytes = (data_size < SLA_HEADER_SIZE) ? data_size : SLA_HEADER_SIZE, zero = 0;
  uint8_t head[SLA_HEADER_SIZE], ok = 1;
  sla_hip_dec_walk_file wf;
  sla_hip_dec_walk_result count, *wr;
  sla_hip_index* x;
  uint32_t nb, b;
  int wide;
  if (d == NULL || d_data == NULL || index == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  *index = NULL;
  if (!src_region_ok(d_data, data_size)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (drain(d) != 0 || order_behind(d, stream) != 0 || res_fetch_headers(d, &d_data, &data_size, &ok, 1) != 0) { return SLA_APIRESULT_NG; }
  memcpy(head, d->h_hdr.ptr, head_bytes);
  if ((x = slai_index_new(head, head_bytes, data_size, 0)) == NULL) { return SLA_APIRESULT_NG; }
  if (!slai_index_has_header(x) || x->info.header.num_samples == 0) { *index = x; return 0; }

  memset(&wf, 0, sizeof(wf));
  wf.src = d_data; wf.data_size = data_size; wf.total = x->info.header.num_samples; wf.capacity = wf.total;
  free(x);
  wide = (d->wide_walk != 0 && data_size >= d->wide_walk);
  memset(d->walk_stats, 0, sizeof(d->walk_stats));
  if (hbuf_reserve(&d->h_src, sizeof(wf) + sizeof(*wr)) != 0 || dbuf_reserve(&d->d_src, sizeof(wf)) != 0
      || dbuf_reserve(&d->d_wres, sizeof(*wr)) != 0 || (wide && res_wide_reserve(d, &wf, &zero, 1) != 0)) { return SLA_APIRESULT_NG; }
  wr = (sla_hip_dec_walk_result*)((uint8_t*)d->h_src.ptr + sizeof(wf));
  /* ---- count mode; a wide walk whose nodes overflow goes to the lane */
  for (;;) {
    if (idx_walk_launch(d, &wf, wide, 0) != 0) { return SLA_APIRESULT_NG; }
    HIPCHK(hipMemcpyAsync(wr, d->d_wres.ptr, sizeof(*wr), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (!wide || wr->reserved != SLA_HIP_DEC_WIDE_OVERFLOW) { break; }
    wide = 0; d->walk_stats[1] = 1;
  }
  d->walk_stats[0] = (uint64_t)wide;                   /* sla_hip_decoder_last_walk: walked wide; overflowed and went to the lane */
  count = *wr;
  nb = count.num_blocks;
  /* ---- write mode, checked against the count */
  if (nb > 0) {
    if (dbuf_reserve(&d->d_blocks, (sizeof(sla_hip_dec_block) + sizeof(uint64_t)) * (size_t)nb + 16) != 0
        || dbuf_reserve(&d->d_crcf, sizeof(uint32_t) * (size_t)nb + 16) != 0 || host_tables_reserve(d, nb) != 0) { return SLA_APIRESULT_NG; }
    wf.first = 0; wf.max_rows = nb;
    if (idx_walk_launch(d, &wf, wide, 1) != 0) { return SLA_APIRESULT_NG; }
    HIPCHK(hipMemcpyAsync(wr, d->d_wres.ptr, sizeof(*wr), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipMemcpyAsync(d->h_blocks, d->d_blocks.ptr, sizeof(sla_hip_dec_block) * (size_t)nb, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (memcmp(wr, &count, sizeof(count)) != 0) { return SLA_APIRESULT_NG; }
  }
  if ((x = slai_index_new(head, head_bytes, data_size, nb)) == NULL) { return SLA_APIRESULT_NG; }
  for (b = 0; b < nb; b++) {
    x->rows[b].byte_off = (uint32_t)d->h_blocks[b].byte_off; x->rows[b].byte_len = d->h_blocks[b].byte_len;
    x->rows[b].smp_off = d->h_blocks[b].smp_off; x->rows[b].num_samples = d->h_blocks[b].num_samples;
  }
  x->info.stop = count.stop; x->info.extent = count.extent; x->info.num_blocks = nb;
  *index = x;
  return 0;
}

/* ------------------------------------------------------------------------------------------------------------
 * sla_hip_decode_windows_indexed (include/sla_hip.h): sla_hip_decode_windows_resident with the chain from the caller's
 * indexes and the examination on the device (k_dec_judge), so that nothing comes home and nothing is waited for.  The
 * per-item checks, the header pass, the grouping and the pass caps, layout and reserve, the gather, the decode kernels, the
 * emit entries and the emit launch are that call's code.  Its own: the rows laid out on the host (slai_index_window), a
 * pass's tables in one slot of the staging ring, the judge between decode and emit.
 * ------------------------------------------------------------------------------------------------------------ */
#define Q_NO_EMIT 0xFFFFFFFFu

/* The next slot of the ring with room for `bytes`: the oldest, waited for when its upload is still in flight -- one of the
 * two places this call may wait.  Idle slots grow along, so that a later call of the same shape allocates nothing. */
static void* q_claim(struct SLADecoder* d, size_t bytes)
{
  const uint32_t s = d->q_next % SLA_HIP_DEC_QUEUE_SLOTS;
  uint32_t k;
  for (k = 0; k < SLA_HIP_DEC_QUEUE_SLOTS; k++) {
    if (d->q_slot[k].ev == NULL && hipEventCreateWithFlags(&d->q_slot[k].ev, hipEventDisableTiming) != hipSuccess) { d->q_slot[k].ev = NULL; return NULL; }
    if (k == s && d->q_slot[k].busy) {
      if (hipEventSynchronize(d->q_slot[k].ev) != hipSuccess) { return NULL; }
      d->q_slot[k].busy = 0;
    }
    if (d->q_slot[k].busy && hipEventQuery(d->q_slot[k].ev) == hipSuccess) { d->q_slot[k].busy = 0; }
    if (!d->q_slot[k].busy && hbuf_reserve(&d->q_slot[k].h, bytes) != 0) { return NULL; }
  }
  d->q_next++;
  return d->q_slot[s].h.ptr;
}
/* the claimed slot's uploads are queued: its guard */
static int q_guard(struct SLADecoder* d)
{
  const uint32_t s = (d->q_next - 1) % SLA_HIP_DEC_QUEUE_SLOTS;
  BCHK(hipEventRecord(d->q_slot[s].ev, d->stream));
  d->q_slot[s].busy = 1;
  return 0;
}

/* One pass queued: files[0, nf) share the launch parameters (nf may be 0); loose[0, nloose) are items that reached no pass,
 * judged with no rows here (their result is the host's, m->hold[item]).  m->wres[item] is the item's plan: num_blocks kept,
 * stop, the byte and sample range, and -- in `skipped` and `reserved` -- the first row and the number of rows of its index. */
static int idx_pass(struct SLADecoder* d, const sla_hip_indexed_window_item* items, const call_mem_t* m, bfile_t* files, uint32_t nf,
                    const uint32_t* loose, uint32_t nloose, uint32_t format, uint32_t zero_fill, sla_hip_window_outcome* d_outcomes,
                    uint32_t num_items)
{
  const uint32_t nj = nf + nloose;
  dec_format_t f;
  sla_hip_dec_gather* gt;
  sla_hip_dec_block* tb;
  uint64_t* tend;
  sla_hip_dec_judge_item* jt;
  sla_hip_dec_emit* et;
  pass_t p;
  stage_t st;
  size_t bytes, o_rows, o_judge;
  uint8_t* slot;
  uint32_t i, k = 0, ng = 0, ne = 0, max_bytes = 0, max_lim = 0, nb;

  memset(&p, 0, sizeof(p)); memset(&f, 0, sizeof(f));
  p.span = 1;
  if (nf > 0) {
    f = files[0].f;
    if (pass_begin(d, files, nf, &p) != 0) { return -1; }
  } else if (dbuf_reserve(&d->d_planes, 256) != 0) { return -1; }
  nb = p.nb;
  o_rows = sizeof(*gt) * (size_t)nf;
  o_judge = o_rows + (sizeof(*tb) + sizeof(*tend)) * (size_t)nb;
  bytes = o_judge + (sizeof(*jt) + sizeof(*et)) * (size_t)nj;
  if (dbuf_reserve(&d->d_src, o_rows + 16) != 0 || dbuf_reserve(&d->d_qtab, (sizeof(*jt) + sizeof(*et)) * (size_t)nj) != 0 || res_events(d) != 0
      || (slot = (uint8_t*)q_claim(d, bytes + 16)) == NULL) { return -1; }
  gt = (sla_hip_dec_gather*)slot; tb = (sla_hip_dec_block*)(slot + o_rows); tend = (uint64_t*)(tb + nb);
  jt = (sla_hip_dec_judge_item*)(slot + o_judge); et = (sla_hip_dec_emit*)(jt + nj);
  memset(slot, 0, bytes);

  /* ---- the tables, straight from the indexes */
  for (i = 0; i < nf; i++) {
    const uint32_t item = files[i].item;
    const sla_hip_indexed_window_item* it = &items[item];
    const sla_hip_dec_window_result* r = &m->wres[item];
    const sla_hip_index_block* rows = it->index->rows + r->skipped;
    const uint32_t rest = files[i].f.total - it->start, whole = (it->length < rest) ? it->length : rest;
    const uint32_t done = (r->stop == SLA_APIRESULT_OK) ? whole : 0;
    uint32_t b;
    if (files[i].bytes > 0) {
      gt[ng].src = it->data + r->first_byte; gt[ng].dst_off = files[i].img_off; gt[ng].bytes = files[i].bytes;
      if (files[i].bytes > max_bytes) { max_bytes = files[i].bytes; }
      ng++;
    }
    jt[i].first = k; jt[i].nb = files[i].nb; jt[i].stop = r->stop; jt[i].ok_samples = whole; jt[i].outcome = item;
    jt[i].fill_end = zero_fill ? it->length : 0;
    for (b = 0; b < r->reserved; b++) {
      if (rows[b].num_samples == 0) { continue; }                   /* passed over, as the window walk does */
      /* every row lies whole inside the gathered range: an index guarantees it (rows ascend without overlap) */
      if (rows[b].byte_off < r->first_byte || (uint64_t)rows[b].byte_off + rows[b].byte_len > r->end_byte) { return -1; }
      tb[k].byte_off = files[i].img_off + (rows[b].byte_off - r->first_byte); tb[k].byte_len = rows[b].byte_len;
      tb[k].smp_off = (uint32_t)files[i].plane_off + (rows[b].smp_off - r->first_sample); tb[k].num_samples = rows[b].num_samples;
      tend[k] = files[i].img_off + files[i].bytes;
      k++;
    }
    if (k - jt[i].first != files[i].nb) { return -1; }
    jt[i].emit = emit_entry(et + ne, &m->dv[item], zero_fill, files[i].plane_off + (it->start - r->first_sample), done, f.C, f.ms,
                            32u - f.bps + f.lshift, f.bps, &max_lim) ? ne++ : Q_NO_EMIT;
  }
  for (i = 0; i < nloose; i++) {
    const uint32_t item = loose[i];
    sla_hip_dec_judge_item* j = &jt[nf + i];
    j->stop = (uint32_t)m->hold[item]; j->outcome = item; j->fill_end = zero_fill ? items[item].length : 0;
    j->emit = (zero_fill && m->state[item] == DEV_PENDING && emit_entry(et + ne, &m->dv[item], 1, 0, 0, m->chans[item], 0, 0, 32, &max_lim))
              ? ne++ : Q_NO_EMIT;
  }

  /* ---- queued: the tables over, the slot's guard, gather, decode kernels, judge, emit */
  st.gt = gt; st.up_bytes = sizeof(*gt) * (size_t)ng; st.d_gt = (const sla_hip_dec_gather*)d->d_src.ptr;
  if (nb > 0) {
    BCHK(hipMemcpyAsync(d->d_blocks.ptr, tb, (sizeof(*tb) + sizeof(*tend)) * (size_t)nb, hipMemcpyHostToDevice, d->stream));
    BCHK(hipMemsetAsync(d->d_info.ptr, 0, sizeof(sla_hip_dec_info) * nb, d->stream));
  }
  BCHK(hipMemcpyAsync(d->d_qtab.ptr, jt, (sizeof(*jt) + sizeof(*et)) * (size_t)nj, hipMemcpyHostToDevice, d->stream));
  if (ng > 0 && stage_gather(d, &st, ng, max_bytes, p.img_bytes) != 0) { return -1; }
  if (q_guard(d) != 0) { return -1; }
  if (nb > 0 && pass_kernels_run(d, &f, nb, 0, p.img_bytes, p.span, NULL, 1) != 0) { return -1; }
  BRC(sla_hip_launch_dec_judge((const uint8_t*)d->d_image.ptr, p.img_bytes, (const sla_hip_dec_block*)d->d_blocks.ptr,
                               (const sla_hip_dec_info*)d->d_info.ptr, nb, (const sla_hip_dec_judge_item*)d->d_qtab.ptr, nj,
                               d->cfg.enable_crc_check == 1, (uint32_t)lms_order_ok(f.lms),
                               (sla_hip_dec_emit*)((sla_hip_dec_judge_item*)d->d_qtab.ptr + nj), ne, d_outcomes, num_items, d->stream));
  BRC(sla_hip_launch_dec_emit_batch((const int32_t*)d->d_planes.ptr, p.span, (const sla_hip_dec_emit*)((sla_hip_dec_judge_item*)d->d_qtab.ptr + nj),
                                    ne, max_lim, format, d->stream));
  return 0;
}

int sla_hip_decode_windows_indexed(struct SLADecoder* d, const sla_hip_indexed_window_item* items, uint32_t num_items,
                                   uint32_t sample_format, uint32_t flags, sla_hip_window_outcome* d_outcomes, sla_hip_stream_t stream)
{
  const uint32_t zero_fill = (flags & SLA_HIP_DEC_ZERO_FILL) ? 1u : 0u;
  const uint64_t esize = pcm_esize(sample_format);
  const double t0 = now_ms();
  call_mem_t m;
  bfile_t* files;
  fmt_mark_t after;
  uint32_t *loose, nf = 0, nloose = 0, i, p0;
  int rc = 0;
  if (d == NULL || d_outcomes == NULL || (items == NULL && num_items > 0) || sample_format > SLA_HIP_PCM_F32
      || (flags & ~SLA_HIP_DEC_ZERO_FILL) != 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_items > 0 && !slai_device_region_ok(d_outcomes, 1, num_items, 0, 1, sizeof(*d_outcomes), -1)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  memset(d->timing, 0, sizeof(d->timing));
  if (num_items == 0) { return 0; }
  if (call_mem_new(&m, num_items) != 0) { return SLA_APIRESULT_NG; }
  files = m.files;
  loose = m.done;                                   /* (an array of the call that this route does not otherwise use) */

  /* ---- the per-item checks of the resident calls, on the host; the header is the index's */
  for (i = 0; i < num_items; i++) {
    const sla_hip_indexed_window_item* it = &items[i];
    sla_hip_decode_device_item* dv = &m.dv[i];
    dv->data = it->data; dv->dst = it->dst; dv->channel_stride = it->channel_stride; dv->sample_stride = it->sample_stride;
    dv->data_size = it->data_size; dv->capacity = it->length;
    m.state[i] = DEV_REFUSED;
    if (it->index == NULL || it->index->info.data_size != it->data_size || !src_region_ok(it->data, it->data_size)) { continue; }
    m.chans[i] = slai_index_has_header(it->index) ? it->index->info.header.wave_format.num_channels : 0;
    if (dst_region_ok(dv, m.chans[i], esize)) { m.state[i] = DEV_PENDING; }
  }
  if (order_behind(d, stream) != 0) { free(m.base); return SLA_APIRESULT_NG; }

  /* ---- headers in item order, as in sla_hip_decode_windows_resident; every window's rows planned from its index */
  for (i = 0; i < num_items; i++) {
    const sla_hip_indexed_window_item* it = &items[i];
    sla_hip_dec_window_result* r = &m.wres[i];
    dec_format_t f;
    SLAApiResult ret;
    int verdict;
    uint32_t row0, nrows, kept, stop;
    m.hold[i] = SLA_APIRESULT_INVALID_ARGUMENT;
    if (m.state[i] == DEV_REFUSED) { continue; }
    if ((ret = file_format(d, it->index->head, it->data_size, &f)) != SLA_APIRESULT_OK) { m.hold[i] = ret; continue; }
    if (it->start > f.total) { m.state[i] = DEV_REFUSED; continue; }
    if ((verdict = format_verdict(&f)) >= 0) { m.hold[i] = verdict; continue; }
    m.hold[i] = SLA_APIRESULT_OK;
    if (it->start == f.total || it->length == 0) { continue; }       /* OK, no samples: nothing is decoded */
    slai_index_window(it->index, f.total, it->start, it->length, d->cfg.max_num_block_samples, &row0, &nrows, &kept, &stop);
    r->num_blocks = kept; r->stop = stop; r->skipped = row0; r->reserved = nrows;
    if (kept > 0) {
      const sla_hip_index_block* a = &it->index->rows[row0];
      const sla_hip_index_block* z = &it->index->rows[row0 + nrows - 1];
      r->first_byte = a->byte_off; r->first_sample = a->smp_off;
      r->end_byte = z->byte_off + z->byte_len; r->end_sample = z->smp_off + z->num_samples;
    }
    files[nf].item = i; files[nf].f = f; files[nf].nb = kept; files[nf].walk_err = (SLAApiResult)stop;
    files[nf].extent = r->end_sample - r->first_sample; files[nf].bytes = r->end_byte - r->first_byte;
    m.state[i] = DEV_DECODED;
    nf++;
  }
  fmt_mark(d, &after);
  for (i = 0; i < num_items; i++) { if (m.state[i] != DEV_DECODED) { loose[nloose++] = i; } }

  /* ---- passes, by sla_hip_decode_windows_resident's grouping and caps; the first takes the loose items along */
  qsort(files, nf, sizeof(*files), slai_dec_file_cmp);
  for (p0 = 0; p0 < nf || nloose > 0; ) {
    const uint32_t p1 = (p0 < nf) ? pass_cut(files, p0, nf) : p0;
    d->queued = 1;
    if (idx_pass(d, items, &m, files + p0, p1 - p0, loose, nloose, sample_format, zero_fill, d_outcomes, num_items) != 0) { rc = SLA_APIRESULT_NG; break; }
    nloose = 0;
    p0 = p1;
  }

  /* ---- the caller's stream behind the handle's closing event */
  if (d->queued) {
    if ((d->ev_close == NULL && hipEventCreateWithFlags(&d->ev_close, hipEventDisableTiming) != hipSuccess)
        || hipEventRecord(d->ev_close, d->stream) != hipSuccess || hipStreamWaitEvent((hipStream_t)stream, d->ev_close, 0) != hipSuccess) { rc = SLA_APIRESULT_NG; }
  }
  d->wave_format = after.wf; d->encode_param = after.ep; d->status_flag = after.flag;
  d->timing[4] = (float)(now_ms() - t0);
  free(m.base);
  return rc;
}

/* ------------------------------------------------------------------------------------------------------------
 * sla_hip_splice_resident (include/sla_hip.h): new streams from parts of resident ones.  The layout is sla_splice.c's; here
 * the blocks it names are collected per item (sp_visit), the items sorted by launch parameters and cut into passes by the
 * edge blocks they decode, and per pass: gather + decode kernels + k_dec_judge on the edge blocks (each its own one-block
 * file of the pass layout), k_splice_check on every block, the one wait for the verdicts, placement, k_splice_edges and
 * k_splice_copy.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const uint8_t* src;           /* the block's sync code in its source */
  uint64_t out_off;             /* where it lies in its output */
  uint32_t byte_len, num_samples;      /* its row */
  uint32_t first, n, kind;      /* the kept samples of the row; SLAI_SPLICE_* */
  uint32_t ordinal;             /* its position in the output */
} sp_block_t;
typedef struct { sp_block_t* v; uint32_t n, cap, ordinal; int oom; const sla_hip_splice_item* it; } sp_list_t;

static void sp_visit(void* ctx, uint32_t seg, const sla_hip_index_block* row, uint32_t first, uint32_t n, uint32_t kind,
                     uint64_t out_off, uint32_t out_len)
{
  sp_list_t* l = (sp_list_t*)ctx;
  sp_block_t* b;
  (void)out_len;
  if (l->oom) { return; }
  if (l->n == l->cap) {
    const uint32_t cap = l->cap * 2 + 256;
    sp_block_t* v = (sp_block_t*)realloc(l->v, sizeof(*v) * (size_t)cap);
    if (v == NULL || cap < l->cap) { l->oom = 1; return; }
    l->v = v; l->cap = cap;
  }
  b = &l->v[l->n++];
  b->src = l->it->segments[seg].data + row->byte_off; b->out_off = out_off;
  b->byte_len = row->byte_len; b->num_samples = row->num_samples;
  b->first = first; b->n = n; b->kind = kind; b->ordinal = l->ordinal++;
}

#define SP_ALIGN(x) (((x) + 15u) & ~(size_t)15)

/* One pass: grp[0, ng) are accepted items of one set of launch parameters (grp[].first / .nb: their blocks in bl).  Returns
 * -1 on a device or allocation failure. */
static int splice_pass(struct SLADecoder* d, sla_hip_splice_item* items, const sla_hip_splice_layout* lay, const bfile_t* grp,
                       uint32_t ng, const sp_block_t* bl, uint8_t* d_arena, uint64_t arena_bytes, uint64_t* arena_used)
{
  const dec_format_t f = grp[0].f;
  const uint32_t width = f.bps - f.lshift;
  bfile_t* ef = NULL;
  sla_hip_dec_gather* gt; sla_hip_dec_block* tb; uint64_t* tend; sla_hip_dec_judge_item* jt; sla_hip_splice_check* ck; uint64_t* vw;
  sla_hip_splice_edge* et; sla_hip_splice_copy* ct; uint8_t* hd;
  uint8_t *hs, *ds;
  size_t o_tb, o_jt, o_ck, o_vw, o_oc, up_bytes, o_dl, o_ct, o_hd, dl_bytes;
  uint32_t ne = 0, nblk = 0, i, k, e, max_bytes = 0, nd = 0, nc = 0, net = 0, max_copy = 0;
  pass_t p;
  stage_t st;
  int rc = -1;

  for (i = 0; i < ng; i++) {
    nblk += grp[i].nb;
    for (k = 0; k < grp[i].nb; k++) { if (bl[grp[i].first + k].kind != SLAI_SPLICE_VERBATIM) { ne++; } }
  }
  memset(&p, 0, sizeof(p)); p.span = 1;
  if (ne > 0) {
    if ((ef = (bfile_t*)calloc(ne, sizeof(*ef))) == NULL) { return -1; }
    for (i = 0, e = 0; i < ng; i++) {
      for (k = 0; k < grp[i].nb; k++) {
        const sp_block_t* b = &bl[grp[i].first + k];
        if (b->kind == SLAI_SPLICE_VERBATIM) { continue; }
        ef[e].item = e; ef[e].f = f; ef[e].bytes = b->byte_len; ef[e].nb = 1; ef[e].extent = b->num_samples;
        e++;
      }
    }
    if (pass_begin(d, ef, ne, &p) != 0) { goto out; }
  } else if (dbuf_reserve(&d->d_planes, 256) != 0) { goto out; }

  /* ---- staging: gather table | rows, ends | judge items | check table | verdict words; on the device the first goes to
   *      d_src, the second to d_blocks, the rest to d_splice with the judge's outcomes behind them */
  o_tb = SP_ALIGN(sizeof(*gt) * (size_t)ne);
  o_jt = o_tb + SP_ALIGN((sizeof(*tb) + sizeof(*tend)) * (size_t)ne);
  o_ck = o_jt + SP_ALIGN(sizeof(*jt) * (size_t)ne);
  o_vw = o_ck + SP_ALIGN(sizeof(*ck) * (size_t)nblk);
  up_bytes = o_vw + SP_ALIGN(sizeof(*vw) * (size_t)ng);
  o_oc = up_bytes - o_jt;
  /* behind them, host only: the verdict words that come home; the delivery tables: edge entries | copy entries | headers */
  o_dl = SP_ALIGN(up_bytes + sizeof(*vw) * (size_t)ng);
  o_ct = SP_ALIGN(sizeof(*et) * (size_t)ne);
  o_hd = o_ct + SP_ALIGN(sizeof(*ct) * ((size_t)nblk + ng));
  dl_bytes = o_hd + 48u * (size_t)ng;
  if (hbuf_reserve(&d->h_splice, o_dl + dl_bytes) != 0 || dbuf_reserve(&d->d_src, o_tb + 16) != 0
      || dbuf_reserve(&d->d_splice, o_oc + sizeof(sla_hip_window_outcome) * (size_t)ne + 16) != 0 || res_events(d) != 0) { goto out; }
  hs = (uint8_t*)d->h_splice.ptr; ds = (uint8_t*)d->d_splice.ptr;
  memset(hs, 0, up_bytes);
  gt = (sla_hip_dec_gather*)hs; tb = (sla_hip_dec_block*)(hs + o_tb); tend = (uint64_t*)(tb + ne);
  jt = (sla_hip_dec_judge_item*)(hs + o_jt); ck = (sla_hip_splice_check*)(hs + o_ck); vw = (uint64_t*)(hs + o_vw);
  for (i = 0, e = 0, nblk = 0; i < ng; i++) {
    vw[i] = ~(uint64_t)0;
    for (k = 0; k < grp[i].nb; k++, nblk++) {
      const sp_block_t* b = &bl[grp[i].first + k];
      sla_hip_splice_check* c = &ck[nblk];
      c->src = b->src; c->byte_len = b->byte_len; c->num_samples = b->num_samples; c->verdict = i; c->ordinal = b->ordinal;
      c->edge = SLA_HIP_SPLICE_NO_EDGE;
      if (b->kind == SLAI_SPLICE_VERBATIM) { continue; }
      gt[e].src = b->src; gt[e].dst_off = ef[e].img_off; gt[e].bytes = b->byte_len;
      if (b->byte_len > max_bytes) { max_bytes = b->byte_len; }
      tb[e].byte_off = ef[e].img_off; tb[e].byte_len = b->byte_len; tb[e].smp_off = (uint32_t)ef[e].plane_off; tb[e].num_samples = b->num_samples;
      tend[e] = ef[e].img_off + b->byte_len;
      jt[e].first = e; jt[e].nb = 1; jt[e].outcome = e; jt[e].emit = Q_NO_EMIT;
      c->edge = e; c->plane_off = ef[e].plane_off + b->first; c->keep = b->n;
      e++;
    }
  }

  /* ---- queued: tables over, gather, decode kernels, judge, check; the verdicts home in the pass's one wait */
  if (ne > 0) {
    st.gt = gt; st.up_bytes = sizeof(*gt) * (size_t)ne; st.d_gt = (const sla_hip_dec_gather*)d->d_src.ptr;
    if (hipMemcpyAsync(d->d_blocks.ptr, tb, (sizeof(*tb) + sizeof(*tend)) * (size_t)ne, hipMemcpyHostToDevice, d->stream) != hipSuccess
        || hipMemsetAsync(d->d_info.ptr, 0, sizeof(sla_hip_dec_info) * ne, d->stream) != hipSuccess) { goto out; }
  }
  if (hipMemcpyAsync(ds, hs + o_jt, o_oc, hipMemcpyHostToDevice, d->stream) != hipSuccess) { goto out; }
  if (ne > 0) {
    if (stage_gather(d, &st, ne, max_bytes, p.img_bytes) != 0 || pass_kernels_run(d, &f, ne, 0, p.img_bytes, p.span, NULL, 1) != 0
        || sla_hip_launch_dec_judge((const uint8_t*)d->d_image.ptr, p.img_bytes, (const sla_hip_dec_block*)d->d_blocks.ptr,
                                    (const sla_hip_dec_info*)d->d_info.ptr, ne, (const sla_hip_dec_judge_item*)ds, ne,
                                    d->cfg.enable_crc_check == 1, (uint32_t)lms_order_ok(f.lms), NULL, 0,
                                    (sla_hip_window_outcome*)(ds + o_oc), ne, d->stream) != 0) { goto out; }
  }
  if (sla_hip_launch_splice_check((const sla_hip_splice_check*)(ds + (o_ck - o_jt)), nblk, d->cfg.enable_crc_check == 1,
                                  (const int32_t*)d->d_planes.ptr, p.span, f.C, width, f.ms,
                                  (const sla_hip_window_outcome*)(ds + o_oc), ne, (uint64_t*)(ds + (o_vw - o_jt)), ng, d->stream) != 0
      || hipMemcpyAsync(hs + up_bytes, ds + (o_vw - o_jt), sizeof(*vw) * (size_t)ng, hipMemcpyDeviceToHost, d->stream) != hipSuccess
      || hipStreamSynchronize(d->stream) != hipSuccess) { goto out; }
  vw = (uint64_t*)(hs + up_bytes);

  /* ---- verdicts, placement; the delivery tables of the clean items */
  for (i = 0; i < ng; i++) {
    sla_hip_splice_item* it = &items[grp[i].item];
    const uint32_t bytes = lay[grp[i].item].bytes;
    if (vw[i] != ~(uint64_t)0) { it->result = (int32_t)(vw[i] & 0xFFu); vw[i] = 0; continue; }
    if (d_arena != NULL) {
      if (bytes > arena_bytes - *arena_used) { it->result = SLA_APIRESULT_INSUFFICIENT_BUFFER_SIZE; vw[i] = 0; continue; }
      it->data = d_arena + *arena_used; *arena_used += bytes;
    }
    it->result = SLA_APIRESULT_OK; it->output_size = bytes;
    vw[i] = 1; nd++;
  }
  if (nd == 0) { rc = 0; goto out; }
  if (dbuf_reserve(&d->d_ftab, dl_bytes + 16) != 0) { goto out; }
  et = (sla_hip_splice_edge*)(hs + o_dl); ct = (sla_hip_splice_copy*)(hs + o_dl + o_ct); hd = hs + o_dl + o_hd;
  memset(et, 0, dl_bytes);
  for (i = 0, e = 0; i < ng; i++) {
    const sla_hip_splice_item* it = &items[grp[i].item];
    uint32_t run = 0;                    /* 1: ct[nc - 1] is a verbatim run that the next verbatim block may extend */
    if (vw[i] == 0) { for (k = 0; k < grp[i].nb; k++) { if (bl[grp[i].first + k].kind != SLAI_SPLICE_VERBATIM) { e++; } } continue; }
    memcpy(hd + 48u * (size_t)i, lay[grp[i].item].header, 48);
    ct[nc].src = (const uint8_t*)d->d_ftab.ptr + o_hd + 48u * (size_t)i; ct[nc].dst = it->data; ct[nc].bytes = SLA_HEADER_SIZE;
    if (max_copy < SLA_HEADER_SIZE) { max_copy = SLA_HEADER_SIZE; }
    nc++;
    for (k = 0; k < grp[i].nb; k++) {
      const sp_block_t* b = &bl[grp[i].first + k];
      if (b->kind != SLAI_SPLICE_VERBATIM) {
        et[net].dst = it->data + b->out_off; et[net].plane_off = ef[e].plane_off + b->first; et[net].num_samples = b->n;
        et[net].silent = (b->kind == SLAI_SPLICE_SILENT) ? 1u : 0u;
        net++; e++; run = 0;
        continue;
      }
      if (run && ct[nc - 1].src + ct[nc - 1].bytes == b->src && ct[nc - 1].bytes <= 0xFFFFFFFFu - b->byte_len) {
        ct[nc - 1].bytes += b->byte_len;
      } else {
        ct[nc].src = b->src; ct[nc].dst = it->data + b->out_off; ct[nc].bytes = b->byte_len;
        nc++; run = 1;
      }
      if (ct[nc - 1].bytes > max_copy) { max_copy = ct[nc - 1].bytes; }
    }
  }
  if (hipMemcpyAsync(d->d_ftab.ptr, et, dl_bytes, hipMemcpyHostToDevice, d->stream) != hipSuccess
      || hipEventRecord(d->ev_src[0], d->stream) != hipSuccess
      || (net > 0 && sla_hip_launch_splice_edges((const int32_t*)d->d_planes.ptr, p.span, (const sla_hip_splice_edge*)d->d_ftab.ptr, net,
                                                 f.C, width, f.ms, d->stream) != 0)
      || hipEventRecord(d->ev_src[1], d->stream) != hipSuccess
      || sla_hip_launch_splice_copy((const sla_hip_splice_copy*)((const uint8_t*)d->d_ftab.ptr + o_ct), nc, max_copy, d->stream) != 0
      || hipEventRecord(d->ev_src[2], d->stream) != hipSuccess
      || hipStreamSynchronize(d->stream) != hipSuccess) { goto out; }
  /* sla_hip_decoder_last_timing: [2] the span of k_splice_edges, [3] of k_splice_copy, summed over the passes */
  ev_add_ms(&d->timing[2], d->ev_src[0], d->ev_src[1]); ev_add_ms(&d->timing[3], d->ev_src[1], d->ev_src[2]);
  rc = 0;
out:
  free(ef);
  return rc;
}

int sla_hip_splice_resident(struct SLADecoder* d, sla_hip_splice_item* items, uint32_t num_items, uint8_t* d_arena, uint64_t arena_bytes,
                            sla_hip_stream_t stream)
{
  const double t0 = now_ms();
  sla_hip_splice_layout* lay;
  bfile_t* grp;
  sp_list_t list;
  uint64_t arena_used = 0;
  uint32_t i, s, k, ng = 0, p0;
  int rc = 0;
  if (d == NULL || (items == NULL && num_items > 0)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (d_arena != NULL && !((arena_bytes <= 1) ? slai_device_region_ok(d_arena, 1, (uint32_t)arena_bytes, 0, 1, 1, -1)
                                              : slai_device_region_ok(d_arena, 1, 2, 0, arena_bytes - 1, 1, -1))) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (drain(d) != 0) { return SLA_APIRESULT_NG; }
  memset(d->timing, 0, sizeof(d->timing));
  if (num_items == 0) { return 0; }
  lay = (sla_hip_splice_layout*)calloc(num_items, sizeof(*lay));
  grp = (bfile_t*)calloc(num_items, sizeof(*grp));
  memset(&list, 0, sizeof(list));
  if (lay == NULL || grp == NULL) { free(lay); free(grp); return SLA_APIRESULT_NG; }

  /* ---- per item, on the host: the layout, the source and destination checks, the handle's capacity, the pass caps */
  for (i = 0; i < num_items; i++) {
    sla_hip_splice_item* it = &items[i];
    const uint32_t b0 = list.n;
    uint64_t smp = 0, bytes = 0;
    dec_format_t f;
    SLAApiResult ret;
    it->output_size = 0;
    if (d_arena != NULL) { it->data = NULL; }
    list.it = it; list.ordinal = 0;
    if ((it->result = slai_splice_walk(it, &lay[i], sp_visit, &list)) != SLA_APIRESULT_OK) { list.n = b0; continue; }
    if (list.oom) { rc = SLA_APIRESULT_NG; goto out; }
    it->result = SLA_APIRESULT_INVALID_ARGUMENT;
    for (s = 0; s < it->num_segments; s++) { if (!src_region_ok(it->segments[s].data, it->segments[s].data_size)) { break; } }
    if (s < it->num_segments) { list.n = b0; continue; }
    if (d_arena == NULL && (it->data == NULL || !((it->data_size <= 1) ? slai_device_region_ok(it->data, 1, it->data_size, 0, 1, 1, -1)
                                                                        : slai_device_region_ok(it->data, 1, 2, 0, (uint64_t)it->data_size - 1, 1, -1)))) {
      list.n = b0; continue;
    }
    if ((ret = file_format(d, it->segments[0].index->head, it->segments[0].data_size, &f)) != SLA_APIRESULT_OK) { it->result = ret; list.n = b0; continue; }
    it->result = SLA_APIRESULT_OK;
    for (k = b0; k < list.n; k++) {
      const sp_block_t* b = &list.v[k];
      if (b->kind == SLAI_SPLICE_VERBATIM) { continue; }
      if (b->num_samples > d->cfg.max_num_block_samples) { it->result = SLA_APIRESULT_INSUFFICIENT_BUFFER_SIZE; break; }
      smp += ((uint64_t)b->num_samples + SLAI_DEC_BATCH_ALIGN) * f.C; bytes += (uint64_t)b->byte_len + 4;
    }
    if (it->result == SLA_APIRESULT_OK && (smp > SLA_HIP_DEC_BATCH_PASS || bytes > DEC_BATCH_PASS_BYTES)) { it->result = SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
    if (it->result == SLA_APIRESULT_OK && d_arena == NULL && lay[i].bytes > it->data_size) { it->result = SLA_APIRESULT_INSUFFICIENT_BUFFER_SIZE; }
    if (it->result != SLA_APIRESULT_OK) { list.n = b0; continue; }
    grp[ng].item = i; grp[ng].f = f; grp[ng].first = b0; grp[ng].nb = list.n - b0;
    grp[ng].extent = (uint32_t)(smp / f.C); grp[ng].bytes = (uint32_t)bytes;
    ng++;
  }
  if (order_behind(d, stream) != 0) { rc = SLA_APIRESULT_NG; goto out; }

  /* ---- passes: equal launch parameters, items ascending, cut where the edge blocks of one more item would exceed a cap */
  qsort(grp, ng, sizeof(*grp), slai_dec_file_cmp);
  for (p0 = 0; p0 < ng; ) {
    uint64_t smp = 0, bytes = 0;
    uint32_t p1 = p0;
    while (p1 < ng && slai_dec_same_launch(&grp[p1].f, &grp[p0].f)) {
      const uint64_t s1 = (uint64_t)grp[p1].extent * grp[p1].f.C, b1 = grp[p1].bytes;
      if (p1 > p0 && (smp + s1 > SLA_HIP_DEC_BATCH_PASS || bytes + b1 > DEC_BATCH_PASS_BYTES)) { break; }
      smp += s1; bytes += b1; p1++;
    }
    if (splice_pass(d, items, lay, grp + p0, p1 - p0, list.v, d_arena, arena_bytes, &arena_used) != 0) {
      /* a device failure: what this and the later passes would have delivered is not there */
      for (i = p0; i < ng; i++) { items[grp[i].item].result = SLA_APIRESULT_NG; items[grp[i].item].output_size = 0; if (d_arena != NULL) { items[grp[i].item].data = NULL; } }
      rc = SLA_APIRESULT_NG;
      break;
    }
    p0 = p1;
    d->timing[5] += 1.0f;
  }
out:
  d->timing[4] = (float)(now_ms() - t0);
  free(list.v); free(lay); free(grp);
  return rc;
}

int sla_hip_decoder_last_window_stats(const struct SLADecoder* decoder, uint64_t counters[4])
{
  if (decoder == NULL || counters == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  memcpy(counters, decoder->win_stats, sizeof(decoder->win_stats));
  return 0;
}

int sla_hip_decoder_set_option(struct SLADecoder* decoder, const char* name, double value)
{
  if (decoder == NULL || name == NULL || !(value >= 0.0) || value > 4294967295.0 || (double)(uint32_t)value != value) {
    return SLA_APIRESULT_INVALID_ARGUMENT;
  }
  if (strcmp(name, "wide_walk") == 0) { decoder->wide_walk = (uint32_t)value; }
  else if (strcmp(name, "wide_walk_nodes") == 0) { decoder->wide_nodes = (uint32_t)value; }
  else { return SLA_APIRESULT_INVALID_ARGUMENT; }
  return 0;
}

int sla_hip_decoder_last_walk(const struct SLADecoder* decoder, uint64_t counters[4])
{
  if (decoder == NULL || counters == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  memcpy(counters, decoder->walk_stats, sizeof(decoder->walk_stats));
  return 0;
}

int sla_hip_decoder_last_timing(const struct SLADecoder* decoder, float* timing_ms)
{
  if (decoder == NULL || timing_ms == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  memcpy(timing_ms, decoder->timing, sizeof(decoder->timing));
  return 0;
}

/* One block that starts at data[0]: its samples, its sample count and the bytes it occupied. */
static SLAApiResult decode_one_block(struct SLADecoder* d, const uint8_t* data, uint32_t data_size, int32_t** buffer,
                                     uint32_t buffer_num_samples, uint32_t* block_size, uint32_t* num_samples)
{
  return decode_run(d, data, data_size, NULL, NULL, 0, buffer, buffer_num_samples, num_samples, block_size);
}

/* ------------------------------------------------------------------------------------------------------------
 * Streaming decoder (reference src/SLADecoder.c:735-1123): the caller appends fragments of the stream and draws
 * ceil(1.05 * sampling_rate / decode_interval_hz) samples per call.  Same entry points, same packet bookkeeping
 * (up to 8 fragments referenced in place, copied into a block buffer of twice the largest possible block as room
 * allows, handed back through CollectDataFragment).  The unit of device work is a whole block: a block is decoded
 * (one SLADecoder block decode on the device) as soon as all its bytes are in the buffer, and calls are served
 * from its samples.  Where the reference would start on a block whose tail has not arrived yet, this decoder
 * returns the samples it has (possibly none) with SLA_APIRESULT_OK and continues once the rest has been appended.
 * ------------------------------------------------------------------------------------------------------------ */
#define STREAM_MAX_PACKETS 8              /* SLA_STREAMING_DECODE_MAX_NUM_PACKETS */
#define STREAM_MARGIN      1.05f          /* SLA_STREAMING_DECODE_NUM_SAMPLES_MARGIN */

typedef struct { const uint8_t* data; uint32_t size, used; } packet_t;

struct SLAStreamingDecoder {
  struct SLADecoder* core;
  float     decode_interval_hz;
  uint32_t  max_bit_per_sample;
  uint32_t  samples_per_decode;
  float     bytes_per_sample;                 /* estimate, refreshed by every block header */
  uint8_t*  data; uint32_t data_cap, data_size;
  packet_t  packets[STREAM_MAX_PACKETS];
  uint32_t  write_pos, read_pos, collect_pos, free_packets;
  int32_t*  cache[SLAI_MAX_CHANNELS];         /* samples of the current block */
  uint32_t  cache_cap, cache_n, cache_pos;
  uint32_t  cur_block_size;
};

struct SLAStreamingDecoder* SLAStreamingDecoder_Create(const struct SLAStreamingDecoderConfig* config)
{
  struct SLAStreamingDecoder* s;
  uint32_t ch;
  if (config == NULL || config->decode_interval_hz <= 0.0f) { return NULL; }
  s = (struct SLAStreamingDecoder*)calloc(1, sizeof(*s));
  if (s == NULL) { return NULL; }
  s->core = SLADecoder_Create(&config->core_config);
  if (s->core == NULL) { free(s); return NULL; }
  s->decode_interval_hz = config->decode_interval_hz;
  s->max_bit_per_sample = config->max_bit_per_sample;
  s->data_cap = 2u * SLA_CalculateSufficientBlockSize(config->core_config.max_num_channels, config->core_config.max_num_block_samples,
                                                      config->max_bit_per_sample);
  if (s->data_cap < 64) { s->data_cap = 64; }
  s->data = (uint8_t*)calloc(s->data_cap, 1);
  s->cache_cap = config->core_config.max_num_block_samples;
  for (ch = 0; ch < config->core_config.max_num_channels; ch++) { s->cache[ch] = (int32_t*)malloc(sizeof(int32_t) * (s->cache_cap + 1)); }
  s->bytes_per_sample = (float)((double)config->core_config.max_num_channels * (config->max_bit_per_sample / 8));
  s->free_packets = STREAM_MAX_PACKETS;
  if (s->data == NULL) { SLAStreamingDecoder_Destroy(s); return NULL; }
  for (ch = 0; ch < config->core_config.max_num_channels; ch++) { if (s->cache[ch] == NULL) { SLAStreamingDecoder_Destroy(s); return NULL; } }
  return s;
}

void SLAStreamingDecoder_Destroy(struct SLAStreamingDecoder* s)
{
  uint32_t ch;
  if (s == NULL) { return; }
  SLADecoder_Destroy(s->core);
  for (ch = 0; ch < SLAI_MAX_CHANNELS; ch++) { free(s->cache[ch]); }
  free(s->data);
  free(s);
}

SLAApiResult SLAStreamingDecoder_SetWaveFormat(struct SLAStreamingDecoder* s, const struct SLAWaveFormat* wave_format)
{
  SLAApiResult ret;
  if (s == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if ((ret = SLADecoder_SetWaveFormat(s->core, wave_format)) != SLA_APIRESULT_OK) { return ret; }
  if (wave_format->bit_per_sample > s->max_bit_per_sample) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  s->samples_per_decode = (uint32_t)ceil(STREAM_MARGIN * (float)wave_format->sampling_rate / s->decode_interval_hz);
  return SLA_APIRESULT_OK;
}

SLAApiResult SLAStreamingDecoder_SetEncodeParameter(struct SLAStreamingDecoder* s, const struct SLAEncodeParameter* encode_param)
{
  if (s == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  return SLADecoder_SetEncodeParameter(s->core, encode_param);
}

SLAApiResult SLAStreamingDecoder_EstimateMinimumNessesaryDataSize(struct SLAStreamingDecoder* s, uint32_t* estimate_data_size)
{
  uint32_t v;
  if (s == NULL || estimate_data_size == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  v = (uint32_t)ceil((double)s->bytes_per_sample * s->samples_per_decode);
  *estimate_data_size = (v > DEC_MIN_BLOCK_HEADER) ? v : DEC_MIN_BLOCK_HEADER;
  return SLA_APIRESULT_OK;
}

static uint32_t queue_remain(const struct SLAStreamingDecoder* s)
{
  uint32_t pos, size = 0;
  if (s->free_packets == STREAM_MAX_PACKETS) { return 0; }
  pos = s->read_pos;
  do {
    size += s->packets[pos].size - s->packets[pos].used;
    pos = (pos + 1) % STREAM_MAX_PACKETS;
  } while (pos != s->write_pos);
  return size;
}

SLAApiResult SLAStreamingDecoder_GetRemainDataSize(struct SLAStreamingDecoder* s, uint32_t* remain_data_size)
{
  uint32_t inside = 0;
  if (s == NULL || remain_data_size == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  /* the reference consumes a block's bytes as it hands its samples out; here the block is decoded at once, so the
   * share of its bytes that belongs to the samples still waiting is counted as remaining */
  if (s->cache_n > s->cache_pos && s->cache_n > 0) {
    inside = (uint32_t)(((uint64_t)s->cur_block_size * (s->cache_n - s->cache_pos)) / s->cache_n);
  }
  *remain_data_size = queue_remain(s) + s->data_size + inside;
  return SLA_APIRESULT_OK;
}

SLAApiResult SLAStreamingDecoder_EstimateDecodableNumSamples(struct SLAStreamingDecoder* s, uint32_t* estimate_num_samples)
{
  uint32_t remain;
  SLAApiResult ret;
  if (s == NULL || estimate_num_samples == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if ((ret = SLAStreamingDecoder_GetRemainDataSize(s, &remain)) != SLA_APIRESULT_OK) { return ret; }
  *estimate_num_samples = (uint32_t)floor((float)remain / s->bytes_per_sample);
  return SLA_APIRESULT_OK;
}

SLAApiResult SLAStreamingDecoder_GetOutputNumSamplesPerDecode(struct SLAStreamingDecoder* s, uint32_t* output_num_samples)
{
  if (s == NULL || output_num_samples == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  *output_num_samples = s->samples_per_decode;
  return SLA_APIRESULT_OK;
}

/* queued fragments -> block buffer, as far as there is room */
static void stream_pull(struct SLAStreamingDecoder* s)
{
  while (s->free_packets != STREAM_MAX_PACKETS && s->data_size < s->data_cap) {
    packet_t* p = &s->packets[s->read_pos];
    uint32_t take;
    if (s->read_pos == s->write_pos && p->size == p->used) { break; }
    take = p->size - p->used;
    if (take > s->data_cap - s->data_size) { take = s->data_cap - s->data_size; }
    memcpy(s->data + s->data_size, p->data + p->used, take);
    s->data_size += take; p->used += take;
    if (p->used == p->size) { s->read_pos = (s->read_pos + 1) % STREAM_MAX_PACKETS; }
    if (take == 0) { break; }
  }
}

SLAApiResult SLAStreamingDecoder_AppendDataFragment(struct SLAStreamingDecoder* s, const uint8_t* data, uint32_t data_size)
{
  if (s == NULL || data == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (s->free_packets == 0) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  if (data_size != 0) {
    packet_t* p = &s->packets[s->write_pos];
    p->data = data; p->size = data_size; p->used = 0;
    s->write_pos = (s->write_pos + 1) % STREAM_MAX_PACKETS;
    s->free_packets--;
  }
  stream_pull(s);
  return SLA_APIRESULT_OK;
}

SLAApiResult SLAStreamingDecoder_CollectDataFragment(struct SLAStreamingDecoder* s, const uint8_t** data_ptr, uint32_t* data_size)
{
  packet_t* p;
  if (s == NULL || data_ptr == NULL || data_size == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (s->free_packets == STREAM_MAX_PACKETS) { return SLA_APIRESULT_NO_DATA_FRAGMENTS; }
  p = &s->packets[s->collect_pos];
  if (p->used == 0) { return SLA_APIRESULT_NO_DATA_FRAGMENTS; }
  *data_ptr = p->data; *data_size = p->used;
  p->size -= p->used; p->data += p->used; p->used = 0;
  if (p->size == 0) { s->collect_pos = (s->collect_pos + 1) % STREAM_MAX_PACKETS; s->free_packets++; }
  return SLA_APIRESULT_OK;
}

SLAApiResult SLAStreamingDecoder_Decode(struct SLAStreamingDecoder* s, int32_t** buffer, uint32_t buffer_num_samples,
                                        uint32_t* num_output_samples)
{
  uint32_t goal, progress = 0, ch;
  const uint32_t C = (s != NULL) ? s->core->wave_format.num_channels : 0;
  if (s == NULL || buffer == NULL || num_output_samples == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (!(s->core->status_flag & STATUS_WAVE_FORMAT) || !(s->core->status_flag & STATUS_ENCODE_PARAM)) { return SLA_APIRESULT_PARAMETER_NOT_SET; }
  goal = (buffer_num_samples < s->samples_per_decode) ? buffer_num_samples : s->samples_per_decode;
  while (progress < goal) {
    uint32_t take;
    if (s->cache_pos >= s->cache_n) {
      /* next block: header fields first (src/SLADecoder.c:1031-1049), then the whole block once it is here */
      uint32_t bsize, nsmpl = 0, used = 0;
      SLAApiResult ret;
      stream_pull(s);
      if (s->data_size < DEC_MIN_BLOCK_HEADER) {
        if (progress > 0) { break; }
        return SLA_APIRESULT_INSUFFICIENT_DATA_SIZE;
      }
      if (rd_be16(s->data) != SLAI_SYNC_CODE) { return SLA_APIRESULT_FAILED_TO_FIND_SYNC_CODE; }
      bsize = rd_be32(s->data + 2) + 6u;
      if (bsize > s->data_size) { break; }                      /* the rest of the block has not been appended yet */
      ret = decode_one_block(s->core, s->data, s->data_size, s->cache, s->cache_cap, &used, &nsmpl);
      if (ret != SLA_APIRESULT_OK) { return ret; }
      if (used == 0 || used > s->data_size) { return SLA_APIRESULT_NG; }
      s->bytes_per_sample = (nsmpl > 0) ? (float)((double)bsize / nsmpl) : s->bytes_per_sample;
      s->cur_block_size = bsize;
      memmove(s->data, s->data + used, s->data_size - used);      /* src/SLADecoder.c:1086-1092 */
      s->data_size -= used;
      s->cache_n = nsmpl; s->cache_pos = 0;
      stream_pull(s);
      if (nsmpl == 0) { continue; }
    }
    take = s->cache_n - s->cache_pos;
    if (take > goal - progress) { take = goal - progress; }
    for (ch = 0; ch < C; ch++) { memcpy(buffer[ch] + progress, s->cache[ch] + s->cache_pos, sizeof(int32_t) * take); }
    s->cache_pos += take; progress += take;
  }
  *num_output_samples = progress;
  return SLA_APIRESULT_OK;
}
