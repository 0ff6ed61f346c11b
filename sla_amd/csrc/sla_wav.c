/*
 * sla_wav.c -- the library's own RIFF/WAVE reader and writer (no device calls).
 *
 * Written from the RIFF/WAVE format: `RIFF` <size> `WAVE`, then chunks of { id[4], little-endian size, body, a pad byte
 * after a body of odd size }.  The reader finds `fmt ` and the `data` chunk behind it; the writer emits the canonical
 * 44-byte header.  The sample bytes themselves never pass through here: the kernels of kernels/wav.inc convert them.
 *
 * The reader is a scan over a WINDOW of the file, so that a file in device memory can be read from probes of a few
 * kilobytes (sla_hip_encode_wav_batch_resident): slai_wav_scan_step consumes whole chunk headers that lie inside the
 * window and either ends with a result code or asks for a window at scan->pos.  sla_hip_wav_parse is the scan with the
 * whole file as its window.  All offsets are 64-bit; no byte outside the window is read.
 */
#include <string.h>
#include "sla_internal.h"

static uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static void wr16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
static void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

void slai_wav_scan_init(slai_wav_scan* s)
{
  memset(s, 0, sizeof(*s));
}

/* [off, off + len) of the file: 0 = inside the window (*p its first byte), SLAI_WAV_NEED_MORE = inside the file but not
 * the window, INSUFFICIENT_DATA_SIZE = not inside the file */
static int scan_bytes(const uint8_t* win, uint64_t win_off, uint32_t win_len, uint64_t file_size, uint64_t off, uint32_t len,
                      const uint8_t** p)
{
  if (off > file_size || len > file_size - off) { return SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; }
  if (win == NULL || off < win_off || off - win_off > win_len || len > win_len - (off - win_off)) { return SLAI_WAV_NEED_MORE; }
  *p = win + (off - win_off);
  return 0;
}

int slai_wav_scan_step(slai_wav_scan* s, const uint8_t* win, uint64_t win_off, uint32_t win_len, uint64_t file_size)
{
  const uint8_t* p;
  int rc;
  if (s->pos == 0) {
    /* a file too short for the signature has none */
    if (file_size < 12) { return SLA_APIRESULT_INVALID_HEADER_FORMAT; }
    if ((rc = scan_bytes(win, win_off, win_len, file_size, 0, 12, &p)) != 0) { return rc; }
    if (memcmp(p, "RIFF", 4) != 0 || memcmp(p + 8, "WAVE", 4) != 0) { return SLA_APIRESULT_INVALID_HEADER_FORMAT; }
    s->pos = 12;
  }
  for (;;) {
    uint64_t body;
    uint32_t csize;
    uint8_t id[4];
    if ((rc = scan_bytes(win, win_off, win_len, file_size, s->pos, 8, &p)) != 0) { return rc; }
    memcpy(id, p, 4);
    csize = rd32(p + 4);
    body = s->pos + 8;
    if (memcmp(id, "fmt ", 4) == 0) {
      uint32_t tag, channels, rate, bits;
      if (csize < 16) { return SLA_APIRESULT_INVALID_HEADER_FORMAT; }
      if ((rc = scan_bytes(win, win_off, win_len, file_size, body, 16, &p)) != 0) { return rc; }
      tag = rd16(p); channels = rd16(p + 2); rate = rd32(p + 4); bits = rd16(p + 14);
      if (tag == 0xFFFEu) {
        /* extensible: cbSize, valid bits, channel mask, sub-format GUID whose first two bytes are the format tag */
        if (csize < 40) { return SLA_APIRESULT_INVALID_HEADER_FORMAT; }
        if ((rc = scan_bytes(win, win_off, win_len, file_size, body, 40, &p)) != 0) { return rc; }
        if (rd16(p + 16) < 22 || rd16(p + 24) != 1 || rd16(p + 18) != bits) { return SLA_APIRESULT_INVALID_HEADER_FORMAT; }
      } else if (tag != 1) {
        return SLA_APIRESULT_INVALID_HEADER_FORMAT;
      }
      if (!(bits == 8 || bits == 16 || bits == 24 || bits == 32) || channels == 0) { return SLA_APIRESULT_INVALID_HEADER_FORMAT; }
      s->info.num_channels = channels; s->info.bits_per_sample = bits; s->info.sampling_rate = rate;
      s->have_fmt = 1;
    } else if (memcmp(id, "data", 4) == 0) {
      uint32_t frame;
      if (!s->have_fmt) { return SLA_APIRESULT_INVALID_HEADER_FORMAT; }
      if (body > file_size || csize > file_size - body) { return SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; }
      if (body > 0xFFFFFFFFu) { return SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; }      /* (a position sla_hip_wav_info cannot hold) */
      frame = s->info.num_channels * (s->info.bits_per_sample / 8);
      s->info.num_samples = csize / frame;
      s->info.data_off = (uint32_t)body;
      s->info.data_bytes = s->info.num_samples * frame;
      return SLA_APIRESULT_OK;
    }
    s->pos = body + csize + (csize & 1u);
  }
}

int sla_hip_wav_parse(const uint8_t* data, uint32_t size, sla_hip_wav_info* info)
{
  slai_wav_scan s;
  int rc;
  if (data == NULL || info == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  memset(info, 0, sizeof(*info));
  slai_wav_scan_init(&s);
  rc = slai_wav_scan_step(&s, data, 0, size, size);
  if (rc == SLAI_WAV_NEED_MORE) { rc = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; }      /* (cannot happen: the window is the file) */
  if (rc == SLA_APIRESULT_OK) { *info = s.info; }
  return rc;
}

int sla_hip_wav_header(const sla_hip_wav_info* info, uint8_t out[SLA_HIP_WAV_HEADER_BYTES])
{
  uint32_t frame;
  if (info == NULL || out == NULL) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  frame = info->num_channels * (info->bits_per_sample / 8);
  memcpy(out, "RIFF", 4); wr32(out + 4, 36u + info->data_bytes);
  memcpy(out + 8, "WAVEfmt ", 8); wr32(out + 16, 16);
  wr16(out + 20, 1); wr16(out + 22, info->num_channels); wr32(out + 24, info->sampling_rate);
  wr32(out + 28, info->sampling_rate * frame); wr16(out + 32, frame); wr16(out + 34, info->bits_per_sample);
  memcpy(out + 36, "data", 4); wr32(out + 40, info->data_bytes);
  return SLA_APIRESULT_OK;
}
