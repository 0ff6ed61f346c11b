/*
 * zero_runs_check.c -- stand-alone check of the run-list lookup of option "silence_runs" (slai_sort_runs,
 * slai_runs_zero_run, slai_silence_run in sla_amd/csrc/sla_plan.c): pure host arithmetic, compiled in as host code, so the
 * program can run under the sanitizers:
 *
 *   cc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
 *      -I$ROCM/include -Iinclude -Isla_amd/csrc -o zero_runs_check tests/tools/zero_runs_check.c sla_amd/csrc/sla_plan.c -lm
 *   ./zero_runs_check
 *
 * Seeded random files (zero runs of 1 .. 20000 samples around SLA's minimum block of 2048, zero tails, all-zero files), in
 * one segment or several on 1024-sample starts.  The run list is taken from the definition (include/sla_hip.h), shuffled
 * -- the device's order is unspecified -- and sorted by the helper; the lookup must answer every question as slai_zero_run
 * does on the mask rebuilt from the list, and every question the encoder can ask (a window that starts inside a file and
 * does not leave it, at least min(2048, what is left) long) as slai_zero_run does on the true mask.  The list and the masks
 * are allocated at exactly their sizes: a read past either end is an AddressSanitizer report.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sla_internal.h"

static uint32_t rng_state = 20261u;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 1664525u + 1013904223u; return (rng_state >> 8) % n; }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static const uint32_t k_lengths[] = { 1, 63, 64, 100, 1023, 2047, 2048, 2049, 3000, 5000, 20000 };

static uint64_t* pack(const uint8_t* bits, uint32_t span)
{
  const uint32_t nwords = (span + 63) / 64;
  uint64_t* m = (uint64_t*)calloc(nwords ? nwords : 1, 8);
  uint32_t s;
  for (s = 0; m != NULL && s < span; s++) { if (bits[s]) { m[s >> 6] |= 1ull << (s & 63); } }
  return m;
}

static int one_layout(uint32_t nfiles)
{
  uint32_t start[8], len[8], f, s, span = 0, nruns = 0, cap = 0, q;
  uint8_t *bits, *rebuilt;
  uint64_t *mask, *rmask;
  sla_hip_zero_run* runs = NULL;
  slai_silence by_runs, by_mask;
  for (f = 0; f < nfiles; f++) {
    start[f] = span;
    len[f] = (rnd(9) == 0) ? 0 : 1 + rnd(60000);
    span += (len[f] + 1023) / 1024 * 1024;
  }
  if (span == 0) { span = 1024; }
  bits = (uint8_t*)calloc(span, 1); rebuilt = (uint8_t*)malloc(span);
  CHECK(bits != NULL && rebuilt != NULL);
  for (f = 0; f < nfiles; f++) {
    const uint32_t kind = rnd(12);
    uint32_t k;
    if (len[f] == 0 || kind == 0) { continue; }                        /* empty, or all zero */
    memset(bits + start[f], 1, len[f]);
    for (k = rnd(7); k > 0; k--) {
      const uint32_t ln = k_lengths[rnd(sizeof(k_lengths) / sizeof(k_lengths[0]))], at = rnd(len[f]);
      memset(bits + start[f] + at, 0, (ln < len[f] - at) ? ln : len[f] - at);
    }
    if (kind <= 4) { const uint32_t t = 1 + rnd(4000); memset(bits + start[f] + len[f] - ((t < len[f]) ? t : len[f]), 0, (t < len[f]) ? t : len[f]); }
  }
  /* the list, from the definition: maximal zero runs inside a file, at least 2048 long or ending at the file's end */
  for (f = 0; f < nfiles; f++) {
    uint32_t a = 0;
    while (a < len[f]) {
      uint32_t b = a;
      if (bits[start[f] + a]) { a++; continue; }
      while (b < len[f] && !bits[start[f] + b]) { b++; }
      if (b - a >= SLA_HIP_ZERO_RUN_MIN || b == len[f]) {
        if (nruns == cap) { cap = cap ? 2 * cap : 4; runs = (sla_hip_zero_run*)realloc(runs, sizeof(*runs) * cap); CHECK(runs != NULL); }
        runs[nruns].start = start[f] + a; runs[nruns].length = b - a; nruns++;
      }
      a = b;
    }
  }
  {
    /* exactly nruns entries, shuffled */
    sla_hip_zero_run* exact = (sla_hip_zero_run*)malloc(sizeof(*runs) * (nruns ? nruns : 1));
    CHECK(exact != NULL);
    for (q = 0; q < nruns; q++) { exact[q] = runs[q]; }
    for (q = nruns; q > 1; q--) { const uint32_t j = rnd(q); const sla_hip_zero_run t = exact[q - 1]; exact[q - 1] = exact[j]; exact[j] = t; }
    free(runs); runs = exact;
  }
  slai_sort_runs(runs, nruns);
  for (q = 1; q < nruns; q++) { CHECK(runs[q - 1].start + runs[q - 1].length <= runs[q].start); }
  memset(rebuilt, 1, span);
  for (q = 0; q < nruns; q++) { memset(rebuilt + runs[q].start, 0, runs[q].length); }
  mask = pack(bits, span); rmask = pack(rebuilt, span);
  CHECK(mask != NULL && rmask != NULL);
  by_runs.nz = NULL; by_runs.runs = runs; by_runs.num_runs = nruns; by_runs.by_runs = 1;
  by_mask.nz = mask; by_mask.runs = NULL; by_mask.num_runs = 0; by_mask.by_runs = 0;
  /* any question inside the span: the rebuilt mask's answer */
  for (q = 0; q < 400; q++) {
    const uint32_t from = rnd(span), limit = 1 + rnd(span - from);
    CHECK(slai_runs_zero_run(runs, nruns, from, limit) == slai_zero_run(rmask, from, limit));
  }
  for (q = 0; q < nruns; q++) {
    const uint32_t a = runs[q].start, b = a + runs[q].length;
    CHECK(slai_runs_zero_run(runs, nruns, a, span - a) == slai_zero_run(rmask, a, span - a));
    CHECK(slai_runs_zero_run(runs, nruns, b - 1, 1) == 1);
    if (a > 0) { CHECK(slai_runs_zero_run(runs, nruns, a - 1, 5) == slai_zero_run(rmask, a - 1, 5)); }
    if (b < span) { CHECK(slai_runs_zero_run(runs, nruns, b, 1) == slai_zero_run(rmask, b, 1)); }
  }
  /* the encoder's questions: the true mask's decisions */
  for (f = 0; f < nfiles; f++) {
    for (s = 0; s < len[f]; s += 1 + rnd(700)) {
      const uint32_t pos = start[f] + s, remain = len[f] - s;
      const uint32_t min_blk = (SLAI_MIN_BLOCK < remain) ? SLAI_MIN_BLOCK : remain;
      uint32_t limit = min_blk + rnd(remain - min_blk + 1);
      const uint32_t got = slai_silence_run(&by_runs, pos, limit), want = slai_silence_run(&by_mask, pos, limit);
      CHECK((got >= min_blk) == (want >= min_blk));
      if (want >= min_blk) { CHECK(got == want); }
      CHECK(slai_silence_is_zero(&by_runs, pos, limit) == slai_silence_is_zero(&by_mask, pos, limit));
      limit = (16384u < remain) ? 16384u : remain;                     /* the hop's window */
      CHECK((slai_silence_run(&by_runs, pos, limit) >= min_blk) == (slai_silence_run(&by_mask, pos, limit) >= min_blk));
    }
  }
  CHECK(slai_silence_run(NULL, 0, 100) == 0);
  free(bits); free(rebuilt); free(mask); free(rmask); free(runs);
  return 0;
}

int main(void)
{
  uint32_t i;
  for (i = 0; i < 300; i++) {
    if (one_layout(1 + (i % 3 == 2 ? rnd(6) : 0)) != 0) { fprintf(stderr, "layout %u failed\n", i); return 1; }
  }
  {
    sla_hip_zero_run none;
    none.start = 0; none.length = 0;
    slai_sort_runs(&none, 0);
    if (slai_runs_zero_run(&none, 0, 3, 9) != 0) { return 1; }
  }
  printf("zero_runs_check: OK (300 layouts)\n");
  return 0;
}
