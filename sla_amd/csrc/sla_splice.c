/* sla_splice.c -- the layout rule of sla_hip_splice_resident (include/sla_hip.h): which blocks an output stream is made of,
 * where each lies and what its 43 header bytes say.  Pure host arithmetic on block indexes, no device calls and no byte of
 * any stream: sla_hip_splice_plan for callers and tests, slai_splice_walk for the driver in sla_decoder.c. */
#include "sla_internal.h"

#include <string.h>

/* the header bytes every segment of one output shares: channels; rate, bits, offset_lshift, the three orders, the channel
 * process method; max_num_block_samples */
static int same_format(const uint8_t* a, const uint8_t* b)
{
  return a[14] == b[14] && memcmp(a + 19, b + 19, 10) == 0 && memcmp(a + 33, b + 33, 2) == 0;
}

static int splice_walk(const sla_hip_splice_item* item, sla_hip_splice_layout* lay, slai_splice_visit visit, void* ctx)
{
  const sla_hip_index* x0;
  struct SLAHeaderInfo h;
  uint64_t bytes = SLA_HEADER_SIZE, samples = 0, blocks = 0;
  uint32_t s, C, width, W, rate;
  if (item->segments == NULL || item->num_segments == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  for (s = 0; s < item->num_segments; s++) {
    const sla_hip_splice_segment* g = &item->segments[s];
    if (g->index == NULL || g->index->info.data_size != g->data_size || g->index->info.header_result != SLA_APIRESULT_OK
        || !same_format(g->index->head, item->segments[0].index->head)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  }
  x0 = item->segments[0].index;
  h = x0->info.header;
  C = h.wave_format.num_channels; rate = h.wave_format.sampling_rate;
  if (h.encode_param.ch_process_method == SLA_CHPROCESSMETHOD_STEREO_MS && C != 2) { return SLA_APIRESULT_INVAILD_CHPROCESSMETHOD; }
  if (C == 0 || C > SLAI_MAX_CHANNELS || h.wave_format.bit_per_sample == 0 || h.wave_format.bit_per_sample > 32
      || h.wave_format.offset_lshift >= h.wave_format.bit_per_sample) { return SLA_APIRESULT_INVALID_HEADER_FORMAT; }
  width = h.wave_format.bit_per_sample - h.wave_format.offset_lshift;
  W = C * width + ((h.encode_param.ch_process_method == SLA_CHPROCESSMETHOD_STEREO_MS) ? 1u : 0u);

  for (s = 0; s < item->num_segments; s++) {
    const sla_hip_splice_segment* g = &item->segments[s];
    const sla_hip_index_block* r = g->index->rows;
    const uint32_t nb = g->index->info.num_blocks;
    const uint64_t end = (uint64_t)g->start + g->length;
    uint32_t lo = 0, hi = nb, i;
    if (g->length == 0) { continue; }
    if (end > g->index->info.extent) {
      return (g->index->info.stop != SLA_APIRESULT_OK) ? (int)g->index->info.stop : SLA_APIRESULT_INSUFFICIENT_DATA_SIZE;
    }
    /* the first row that ends behind the segment's start (the rows' ends ascend) */
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if ((uint64_t)r[mid].smp_off + r[mid].num_samples <= g->start) { lo = mid + 1; } else { hi = mid; }
    }
    for (i = lo; i < nb && r[i].smp_off < end; i++) {
      const uint64_t row_end = (uint64_t)r[i].smp_off + r[i].num_samples;
      const uint32_t a = (r[i].smp_off > g->start) ? r[i].smp_off : g->start;
      const uint32_t b = (uint32_t)((row_end < end) ? row_end : end);
      const uint32_t n = b - a;
      uint32_t kind, len;
      if (r[i].num_samples == 0) { continue; }
      if (n == r[i].num_samples) { kind = SLAI_SPLICE_VERBATIM; len = r[i].byte_len; }
      else if (r[i].byte_len == SLAI_SPLICE_SILENT_BYTES) { kind = SLAI_SPLICE_SILENT; len = SLAI_SPLICE_SILENT_BYTES; }
      else { kind = SLAI_SPLICE_RAW; len = SLAI_SPLICE_SILENT_BYTES + (uint32_t)(((uint64_t)n * W + 7) / 8); }
      if (visit != NULL) { visit(ctx, s, &r[i], a - r[i].smp_off, n, kind, bytes, len); }
      if (kind == SLAI_SPLICE_VERBATIM) { lay->verbatim_bytes += len; } else { lay->edge_blocks++; }
      if (len > lay->max_block_size) { lay->max_block_size = len; }
      { const uint32_t bps = (uint32_t)(8u * len * rate) / n; if (bps > lay->max_bit_per_second) { lay->max_bit_per_second = bps; } }
      bytes += len; blocks++;
    }
    samples += g->length;
  }
  if (bytes > 0xFFFFFFFFull || samples > 0xFFFFFFFFull || blocks > 0xFFFFFFFFull) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  lay->bytes = (uint32_t)bytes; lay->num_samples = (uint32_t)samples; lay->num_blocks = (uint32_t)blocks;
  h.num_samples = lay->num_samples; h.num_blocks = lay->num_blocks;
  h.max_block_size = lay->max_block_size; h.max_bit_per_second = lay->max_bit_per_second;
  return slai_write_header(&h, lay->header, sizeof(lay->header));
}

/* on any refusal *lay is zero */
int slai_splice_walk(const sla_hip_splice_item* item, sla_hip_splice_layout* lay, slai_splice_visit visit, void* ctx)
{
  int rc;
  if (lay == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  memset(lay, 0, sizeof(*lay));
  if (item == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if ((rc = splice_walk(item, lay, visit, ctx)) != SLA_APIRESULT_OK) { memset(lay, 0, sizeof(*lay)); }
  return rc;
}

int sla_hip_splice_plan(const sla_hip_splice_item* item, sla_hip_splice_layout* layout)
{
  return slai_splice_walk(item, layout, NULL, NULL);
}
