/*
 * verify_tables_check.c -- stand-alone check of slai_verify_tables (sla_amd/csrc/sla_verify.c), the host routine that
 * turns the device pack's block table into the tables of the encoder's verification pass.  No device, no library: the
 * routine is compiled in as host code, so the program can run under the sanitizers:
 *
 *   cc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
 *      -I$ROCM/include -Iinclude -Isla_amd/csrc -o verify_tables_check tests/tools/verify_tables_check.c sla_amd/csrc/sla_verify.c
 *   ./verify_tables_check
 *
 * Every output array is allocated at exactly the size the routine may use (num_blocks entries, none for an empty
 * table), so a write past the end is an AddressSanitizer report.  The layouts are random batches: files with and without
 * blocks (leading, trailing, in a row), delivered or not, with the 43-byte headers or as one bare piece.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sla_internal.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 1664525u + 1013904223u; return (rng_state >> 8) % n; }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int one_layout(uint32_t nfiles, int bare, uint32_t channels)
{
  uint32_t* nblk = (uint32_t*)malloc(sizeof(uint32_t) * (nfiles ? nfiles : 1));
  slai_verify_seg* segs = (slai_verify_seg*)malloc(sizeof(slai_verify_seg) * (nfiles ? nfiles : 1));
  uint32_t f, b, nb = 0, k = 0, at = 0, want = 0, got, longest = 77, want_longest = 0;
  uint64_t cur = 0, pos = 0, compared = 77, want_compared = 0;
  sla_hip_pack_block* pb;
  sla_hip_dec_block* db; uint64_t* end; sla_hip_verify_expect* ex; uint32_t* so;
  for (f = 0; f < nfiles; f++) { nblk[f] = (rnd(3) == 0) ? 0 : rnd(5); if (bare && nfiles == 1) { nblk[f] += 1; } nb += nblk[f]; }
  /* exact sizes: malloc(0) may return NULL, which the routine must then never touch */
  pb = (sla_hip_pack_block*)malloc(sizeof(*pb) * nb);
  db = (sla_hip_dec_block*)malloc(sizeof(*db) * nb);
  end = (uint64_t*)malloc(sizeof(*end) * nb);
  ex = (sla_hip_verify_expect*)malloc(sizeof(*ex) * nb);
  so = (uint32_t*)malloc(sizeof(*so) * nb);
  for (f = 0; f < nfiles; f++) {
    uint64_t p = pos;
    segs[f].img_off = cur; segs[f].deliver = (rnd(4) != 0);
    if (!bare) { cur += 43; }
    for (b = 0; b < nblk[f]; b++, k++) {
      memset(&pb[k], 0, sizeof(pb[k]));
      pb[k].blk_off = p; pb[k].out_off = cur; pb[k].num_samples = 1 + rnd(4096); pb[k].type = rnd(3); pb[k].out_bytes = 11 + rnd(9000);
      cur += pb[k].out_bytes; p += pb[k].num_samples;
      if (segs[f].deliver) {
        want++; want_compared += (uint64_t)channels * pb[k].num_samples;
        if (pb[k].num_samples > want_longest) { want_longest = pb[k].num_samples; }
      }
    }
    segs[f].img_bytes = cur - segs[f].img_off;
    pos += (p - pos + 1023) / 1024 * 1024;
  }
  got = slai_verify_tables(pb, nb, segs, nfiles, channels, db, end, ex, so, &compared, &longest);
  CHECK(got == want); CHECK(compared == want_compared); CHECK(longest == want_longest);
  k = 0;
  for (f = 0; f < nfiles; f++) {
    for (b = 0; b < nblk[f]; b++, k++) {
      if (!segs[f].deliver) { continue; }
      CHECK(db[at].byte_off == pb[k].out_off); CHECK(db[at].byte_len == pb[k].out_bytes);
      CHECK(db[at].smp_off == (uint32_t)pb[k].blk_off); CHECK(db[at].num_samples == pb[k].num_samples); CHECK(db[at].flags == 0);
      CHECK(end[at] == segs[f].img_off + segs[f].img_bytes);
      CHECK(ex[at].type == pb[k].type); CHECK(ex[at].bytes == pb[k].out_bytes);
      CHECK(so[at] == f);
      at++;
    }
  }
  CHECK(at == got);
  free(nblk); free(segs); free(pb); free(db); free(end); free(ex); free(so);
  return 0;
}

int main(void)
{
  uint32_t i;
  /* no file at all, NULL everywhere */
  {
    uint64_t c = 5; uint32_t m = 5;
    if (slai_verify_tables(NULL, 0, NULL, 0, 2, NULL, NULL, NULL, NULL, &c, &m) != 0 || c != 0 || m != 0) { fprintf(stderr, "empty call\n"); return 1; }
    if (slai_verify_tables(NULL, 0, NULL, 0, 2, NULL, NULL, NULL, NULL, NULL, NULL) != 0) { fprintf(stderr, "empty call, no outputs\n"); return 1; }
  }
  for (i = 0; i < 4000; i++) {
    const uint32_t nfiles = (i < 40) ? i % 4 : rnd(12);
    if (one_layout(nfiles, 0, 1 + rnd(8)) != 0) { fprintf(stderr, "layout %u (%u files)\n", i, nfiles); return 1; }
  }
  for (i = 0; i < 400; i++) { if (one_layout(1, 1, 1 + rnd(8)) != 0) { fprintf(stderr, "bare piece %u\n", i); return 1; } }
  printf("verify_tables_check: ok\n");
  return 0;
}
