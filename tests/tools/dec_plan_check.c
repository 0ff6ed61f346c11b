/*
 * dec_plan_check.c -- stand-alone check of the batch decoder's pass arithmetic (slai_dec_file_cmp, slai_dec_cut,
 * slai_dec_layout, slai_dec_pick_wide, slai_dec_wide_capacity in sla_amd/csrc/sla_dec_plan.c): pure host arithmetic,
 * compiled in as host code, so the program can run under the sanitizers:
 *
 *   cc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
 *      -I$ROCM/include -Iinclude -Isla_amd/csrc -o dec_plan_check tests/tools/dec_plan_check.c sla_amd/csrc/sla_dec_plan.c
 *   ./dec_plan_check
 *
 * The 200 seeded batches of tests/decplanmodel.py (the same generator, draw for draw), every table and pick list allocated
 * at exactly its size: a read or write past either end is an AddressSanitizer report.  Checked on each: the order is the
 * comparison's; the cuts cover the files that are not alone exactly once and leave the alone ones out; no pass of several
 * files exceeds a cap, and a pass that ends inside a launch key could not have taken the next file; offsets are monotone,
 * image offsets multiples of 4, plane offsets multiples of 64, the totals the sums; the wide pick is sorted, complete and
 * at most SLAI_DEC_WIDE_MAX long.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sla_internal.h"

static uint32_t rng_state = 20261u;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 1664525u + 1013904223u; return (rng_state >> 8) % n; }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int one_batch(uint32_t* passes_seen)
{
  static const uint32_t ties[3] = { 1000, 2000, 5999 };
  slai_dec_format fm[3];
  const uint32_t nf = 1 + rnd(40);
  const uint64_t cap_s = 20000 + rnd(400000), cap_b = 2000 + rnd(40000);
  const uint32_t thr = (rnd(4) == 0) ? 0 : 1 + rnd(6000), nfmt = 1 + rnd(3);
  slai_dec_file* files = (slai_dec_file*)calloc(nf, sizeof(*files));
  uint32_t* pick;
  uint32_t i, k, n = 0, p0, npick, eligible = 0;
  CHECK(files != NULL);
  for (k = 0; k < nfmt; k++) {
    memset(&fm[k], 0, sizeof(fm[k]));
    fm[k].C = 1 + rnd(2); fm[k].bps = 16 + 8 * rnd(2); fm[k].ms = rnd(2); fm[k].order = 8u << rnd(2);
    fm[k].ntaps = rnd(2); fm[k].lms = 4u << rnd(2); fm[k].lshift = rnd(2);
  }
  for (i = 0; i < nf; i++) {
    files[i].item = i;
    files[i].f = fm[rnd(nfmt)];
    files[i].f.total = rnd(100000);
    files[i].extent = (rnd(8) == 0) ? 0 : rnd(20000);
    files[i].bytes = (rnd(8) == 0) ? 0 : ((rnd(5) == 0) ? ties[rnd(3)] : rnd(6000));
    files[i].nb = rnd(50);
    files[i].alone = (rnd(10) == 0);
  }
  qsort(files, nf, sizeof(*files), slai_dec_file_cmp);
  for (i = 1; i < nf; i++) { CHECK(slai_dec_file_cmp(&files[i - 1], &files[i]) < 0 && slai_dec_file_cmp(&files[i], &files[i - 1]) > 0); }
  while (n < nf && !files[n].alone) { n++; }
  for (i = n; i < nf; i++) { CHECK(files[i].alone); }

  for (p0 = 0; p0 < n; ) {
    const uint32_t p1 = slai_dec_cut(files, p0, n, cap_s, cap_b);
    /* the pass as a table of its own, exactly p1 - p0 entries */
    slai_dec_file* pass;
    uint64_t smp = 0, bytes = 0, img = 7, span = 7, want_img = 0, want_span = 0;
    uint32_t nb = 7, want_nb = 0;
    CHECK(p1 > p0 && p1 <= n);
    pass = (slai_dec_file*)malloc(sizeof(*pass) * (p1 - p0));
    CHECK(pass != NULL);
    memcpy(pass, files + p0, sizeof(*pass) * (p1 - p0));
    for (i = p0; i < p1; i++) {
      CHECK(slai_dec_same_launch(&files[i].f, &files[p0].f));
      smp += ((uint64_t)files[i].extent + SLAI_DEC_BATCH_ALIGN) * files[i].f.C; bytes += (uint64_t)files[i].bytes + 4;
    }
    CHECK(p1 - p0 == 1 || (smp <= cap_s && bytes <= cap_b));
    if (p1 < n && slai_dec_same_launch(&files[p1].f, &files[p0].f)) {
      CHECK(smp + ((uint64_t)files[p1].extent + SLAI_DEC_BATCH_ALIGN) * files[p1].f.C > cap_s || bytes + files[p1].bytes + 4 > cap_b);
    }
    slai_dec_layout(pass, p1 - p0, &img, &span, &nb);
    for (i = 0; i < p1 - p0; i++) {
      CHECK(pass[i].img_off == want_img && pass[i].plane_off == want_span);
      CHECK(pass[i].img_off % 4 == 0 && pass[i].plane_off % SLAI_DEC_BATCH_ALIGN == 0);
      want_img += pass[i].bytes; while (want_img % 4 != 0) { want_img++; }
      want_span += pass[i].extent; while (want_span % SLAI_DEC_BATCH_ALIGN != 0) { want_span++; }
      want_nb += pass[i].nb;
    }
    CHECK(img == want_img && span == want_span && nb == want_nb);
    free(pass);
    (*passes_seen)++;
    p0 = p1;
  }

  pick = (uint32_t*)malloc(sizeof(*pick) * SLAI_DEC_WIDE_MAX);
  CHECK(pick != NULL);
  npick = slai_dec_pick_wide(files, nf, thr, pick);
  for (i = 0; i < nf; i++) { eligible += (thr != 0 && files[i].bytes >= thr); }
  CHECK(npick == ((eligible < SLAI_DEC_WIDE_MAX) ? eligible : SLAI_DEC_WIDE_MAX));
  for (k = 0; k < npick; k++) {
    CHECK(pick[k] < nf && files[pick[k]].bytes >= thr);
    if (k > 0) {
      const slai_dec_file *a = &files[pick[k - 1]], *b = &files[pick[k]];
      CHECK(a->bytes > b->bytes || (a->bytes == b->bytes && a->item < b->item));
    }
  }
  for (i = 0; npick > 0 && i < nf; i++) {            /* nothing left out is longer than the last one picked, or equal and earlier */
    const slai_dec_file* last = &files[pick[npick - 1]];
    int picked = 0;
    for (k = 0; k < npick; k++) { picked |= (pick[k] == i); }
    if (!picked && files[i].bytes >= thr) { CHECK(files[i].bytes < last->bytes || (files[i].bytes == last->bytes && files[i].item > last->item)); }
  }
  free(pick); free(files);
  return 0;
}

int main(void)
{
  uint32_t b, passes = 0;
  for (b = 0; b < 200; b++) {
    if (one_batch(&passes) != 0) { fprintf(stderr, "batch %u failed\n", b); return 1; }
  }
  {
    slai_dec_file none;
    uint64_t img = 7, span = 7;
    uint32_t nb = 7, pick[SLAI_DEC_WIDE_MAX];
    memset(&none, 0, sizeof(none));
    slai_dec_layout(&none, 0, &img, &span, &nb);
    if (img != 0 || span != 0 || nb != 0 || slai_dec_pick_wide(&none, 0, 1, pick) != 0 || slai_dec_cut(&none, 0, 0, 1, 1) != 0) { return 1; }
    if (slai_dec_wide_capacity(0, 0) != (1u << 16) || slai_dec_wide_capacity(0, 0xFFFFFFFFu) != 0xFFFFFFu || slai_dec_wide_capacity(9, 1) != 9) { return 1; }
  }
  printf("dec_plan_check: OK (200 batches, %u passes)\n", passes);
  return 0;
}
