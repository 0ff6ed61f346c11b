/* sla_dec_index.c -- the block index of a .sla stream (sla_hip_index, include/sla_hip.h): built from host bytes, read,
 * serialised and read back, and the rows a window needs of it.  Pure host code, no device calls: tests/test_index_model.py
 * holds it against tests/indexmodel.py.  The builder from device bytes is sla_hip_index_build_resident of sla_decoder.c. */
#include "sla_internal.h"
#include "SLADecoder.h"

#include <stdlib.h>
#include <string.h>

#define IDX_MIN_BLOCK_HEADER 11u         /* SLA_MINIMUM_BLOCK_HEADER_SIZE */
#define IDX_MAGIC            "SLAX"
#define IDX_VERSION          1u
#define IDX_FIXED            32u         /* magic, version, data_size, header_bytes, header_result, stop, extent, num_blocks */
#define IDX_ROWS_AT          (IDX_FIXED + SLAI_INDEX_HEAD)
#define IDX_CRC_BYTES        2u

static uint32_t rd_be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }
static uint32_t rd_be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
static uint32_t rd_le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static void wr_le32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

sla_hip_index* slai_index_new(const uint8_t* head, uint32_t head_bytes, uint32_t data_size, uint32_t num_blocks)
{
  sla_hip_index* x;
  if (head_bytes > SLA_HEADER_SIZE) { return NULL; }
  x = (sla_hip_index*)calloc(1, sizeof(*x) + sizeof(sla_hip_index_block) * (size_t)num_blocks);
  if (x == NULL) { return NULL; }
  x->rows = (sla_hip_index_block*)(x + 1);
  if (head_bytes > 0) { memcpy(x->head, head, head_bytes); }
  x->info.data_size = data_size; x->info.header_bytes = head_bytes;
  x->info.header_result = (int32_t)SLADecoder_DecodeHeader(x->head, data_size, &x->info.header);
  if (!slai_index_has_header(x)) { memset(&x->info.header, 0, sizeof(x->info.header)); }
  return x;
}

int slai_index_has_header(const sla_hip_index* x)
{
  return x->info.header_result == SLA_APIRESULT_OK || x->info.header_result == SLA_APIRESULT_DETECT_DATA_CORRUPTION;
}

/* The chain from byte 43 by walk_chain's rules (sla_decoder.c) with capacity = total, no cap on the block length and no
 * header-only rows; rows == NULL counts.  Returns the rows, *stop and *extent. */
static uint32_t index_walk(const uint8_t* data, uint32_t data_size, uint32_t total, sla_hip_index_block* rows, uint32_t* stop,
                           uint32_t* extent)
{
  uint32_t off = SLA_HEADER_SIZE, pos = 0, nb = 0;
  *stop = SLA_APIRESULT_OK;
  while (pos < total) {
    const uint8_t* p;
    uint32_t left, bsize, n;
    if (off > data_size) { *stop = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    left = data_size - off;
    if (left < IDX_MIN_BLOCK_HEADER) { *stop = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    p = data + off;
    if (rd_be16(p) != SLAI_SYNC_CODE) { *stop = SLA_APIRESULT_FAILED_TO_FIND_SYNC_CODE; break; }
    bsize = rd_be32(p + 2) + 6u;
    n = rd_be16(p + 8);
    if (bsize > left || bsize < SLAI_BLK_CRC_START) { *stop = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    if (n > total - pos) { *stop = SLA_APIRESULT_INSUFFICIENT_BUFFER_SIZE; break; }
    if (rows != NULL) { rows[nb].byte_off = off; rows[nb].byte_len = bsize; rows[nb].smp_off = pos; rows[nb].num_samples = n; }
    nb++;
    off += bsize; pos += n;
  }
  *extent = pos;
  return nb;
}

int sla_hip_index_build(const uint8_t* data, uint32_t data_size, sla_hip_index** index)
{
  const uint32_t head_bytes = (data_size < SLA_HEADER_SIZE) ? data_size : SLA_HEADER_SIZE;
  sla_hip_index* x;
  uint32_t nb = 0, stop, extent;
  if (data == NULL || index == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  *index = NULL;
  if ((x = slai_index_new(data, head_bytes, data_size, 0)) == NULL) { return SLA_APIRESULT_NG; }
  if (slai_index_has_header(x)) {
    const uint32_t total = x->info.header.num_samples;
    nb = index_walk(data, data_size, total, NULL, &stop, &extent);
    free(x);
    if ((x = slai_index_new(data, head_bytes, data_size, nb)) == NULL) { return SLA_APIRESULT_NG; }
    (void)index_walk(data, data_size, total, x->rows, &stop, &extent);
    x->info.stop = stop; x->info.extent = extent; x->info.num_blocks = nb;
  }
  *index = x;
  return 0;
}

int sla_hip_index_info(const sla_hip_index* index, sla_hip_index_summary* info)
{
  if (index == NULL || info == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  *info = index->info;
  return 0;
}

int sla_hip_index_blocks(const sla_hip_index* index, uint32_t first, uint32_t count, sla_hip_index_block* out)
{
  if (index == NULL || (out == NULL && count > 0) || first > index->info.num_blocks || count > index->info.num_blocks - first) {
    return SLA_APIRESULT_INVALID_ARGUMENT;
  }
  if (count > 0) { memcpy(out, index->rows + first, sizeof(*out) * (size_t)count); }
  return 0;
}

void sla_hip_index_destroy(sla_hip_index* index) { free(index); }

uint64_t sla_hip_index_serialized_bytes(const sla_hip_index* index)
{
  return (index == NULL) ? 0 : (uint64_t)IDX_ROWS_AT + 16u * (uint64_t)index->info.num_blocks + IDX_CRC_BYTES;
}

uint64_t sla_hip_index_serialize(const sla_hip_index* index, uint8_t* out, uint64_t capacity)
{
  const uint64_t bytes = sla_hip_index_serialized_bytes(index);
  uint32_t i, crc;
  uint8_t* p;
  if (index == NULL || out == NULL || capacity < bytes) { return 0; }
  memcpy(out, IDX_MAGIC, 4);
  wr_le32(out + 4, IDX_VERSION); wr_le32(out + 8, index->info.data_size); wr_le32(out + 12, index->info.header_bytes);
  wr_le32(out + 16, (uint32_t)index->info.header_result); wr_le32(out + 20, index->info.stop);
  wr_le32(out + 24, index->info.extent); wr_le32(out + 28, index->info.num_blocks);
  memcpy(out + IDX_FIXED, index->head, SLAI_INDEX_HEAD);
  p = out + IDX_ROWS_AT;
  for (i = 0; i < index->info.num_blocks; i++, p += 16) {
    wr_le32(p, index->rows[i].byte_off); wr_le32(p + 4, index->rows[i].byte_len);
    wr_le32(p + 8, index->rows[i].smp_off); wr_le32(p + 12, index->rows[i].num_samples);
  }
  crc = slai_crc16(out, (size_t)(bytes - IDX_CRC_BYTES));
  p[0] = (uint8_t)crc; p[1] = (uint8_t)(crc >> 8);
  return bytes;
}

int sla_hip_index_deserialize(const uint8_t* blob, uint64_t blob_bytes, sla_hip_index** index)
{
  sla_hip_index* x;
  uint32_t data_size, head_bytes, stop, extent, nb, i, k;
  uint64_t pos = 0, prev_end = 0;
  const uint8_t* p;
  if (blob == NULL || index == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  *index = NULL;
  if (blob_bytes < IDX_ROWS_AT + IDX_CRC_BYTES || memcmp(blob, IDX_MAGIC, 4) != 0 || rd_le32(blob + 4) != IDX_VERSION) {
    return SLA_APIRESULT_INVALID_ARGUMENT;
  }
  data_size = rd_le32(blob + 8); head_bytes = rd_le32(blob + 12);
  stop = rd_le32(blob + 20); extent = rd_le32(blob + 24); nb = rd_le32(blob + 28);
  if (blob_bytes != (uint64_t)IDX_ROWS_AT + 16u * (uint64_t)nb + IDX_CRC_BYTES) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  p = blob + blob_bytes - IDX_CRC_BYTES;
  if (slai_crc16(blob, (size_t)(blob_bytes - IDX_CRC_BYTES)) != ((uint32_t)p[0] | ((uint32_t)p[1] << 8))) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (head_bytes != ((data_size < SLA_HEADER_SIZE) ? data_size : SLA_HEADER_SIZE) || stop > SLA_APIRESULT_PARAMETER_NOT_SET) {
    return SLA_APIRESULT_INVALID_ARGUMENT;
  }
  for (k = head_bytes; k < SLAI_INDEX_HEAD; k++) { if (blob[IDX_FIXED + k] != 0) { return SLA_APIRESULT_INVALID_ARGUMENT; } }
  /* the rows, before anything is allocated */
  p = blob + IDX_ROWS_AT;
  for (i = 0; i < nb; i++, p += 16) {
    const uint32_t off = rd_le32(p), len = rd_le32(p + 4), smp = rd_le32(p + 8), n = rd_le32(p + 12);
    if (off < SLA_HEADER_SIZE || len < IDX_MIN_BLOCK_HEADER || (uint64_t)off + len > data_size || n > 65535u) { return SLA_APIRESULT_INVALID_ARGUMENT; }
    /* ascending without overlap: a window's gather range, first row's start to last row's end, then holds every row of it whole */
    if (off < prev_end || smp != pos) { return SLA_APIRESULT_INVALID_ARGUMENT; }
    prev_end = (uint64_t)off + len; pos += n;
  }
  if (extent != pos) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if ((x = slai_index_new(blob + IDX_FIXED, head_bytes, data_size, nb)) == NULL) { return SLA_APIRESULT_NG; }
  if ((uint32_t)x->info.header_result != rd_le32(blob + 16) || (!slai_index_has_header(x) && (nb != 0 || stop != 0))
      || (slai_index_has_header(x) && extent > x->info.header.num_samples)) {
    free(x);
    return SLA_APIRESULT_INVALID_ARGUMENT;
  }
  p = blob + IDX_ROWS_AT;
  for (i = 0; i < nb; i++, p += 16) {
    x->rows[i].byte_off = rd_le32(p); x->rows[i].byte_len = rd_le32(p + 4); x->rows[i].smp_off = rd_le32(p + 8); x->rows[i].num_samples = rd_le32(p + 12);
  }
  x->info.stop = stop; x->info.extent = extent; x->info.num_blocks = nb;
  *index = x;
  return 0;
}

void slai_index_window(const sla_hip_index* x, uint32_t total, uint32_t start, uint32_t length, uint32_t max_block_samples,
                       uint32_t* row0, uint32_t* nrows, uint32_t* kept, uint32_t* stop)
{
  const uint64_t win_end = ((uint64_t)start + length < total) ? (uint64_t)start + length : total;
  const sla_hip_index_block* r = x->rows;
  const uint32_t nb = x->info.num_blocks;
  uint32_t lo = 0, hi = nb, i, last = 0;
  *row0 = 0; *nrows = 0; *kept = 0; *stop = SLA_APIRESULT_OK;
  if (win_end == 0 || start >= win_end) { return; }
  /* the first row that ends behind the window's start (the rows' ends ascend) */
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((uint64_t)r[mid].smp_off + r[mid].num_samples <= start) { lo = mid + 1; } else { hi = mid; }
  }
  for (i = lo; ; i++) {
    const uint64_t pos = (i < nb) ? r[i].smp_off : x->info.extent;
    if (pos >= win_end) { break; }
    if (i == nb) { *stop = (x->info.stop != SLA_APIRESULT_OK) ? x->info.stop : (uint32_t)SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    if (r[i].num_samples == 0) { continue; }
    if (r[i].num_samples > max_block_samples) { *stop = SLA_APIRESULT_INSUFFICIENT_BUFFER_SIZE; break; }
    if (*kept == 0) { *row0 = i; }
    last = i; (*kept)++;
  }
  if (*kept > 0) { *nrows = last - *row0 + 1; }
}
