/* sla_dec_plan.c -- the pass arithmetic of the batch decoder (sla_decoder.c): which files share a pass, where a pass is
 * cut, where each file's bytes and samples lie in it, which resident files are walked wide.  Pure host arithmetic on
 * slai_dec_file tables, no device calls: tests/test_dec_pass_plan.py and tests/tools/dec_plan_check.c call it directly. */
#include "sla_internal.h"

/* the launch key: the kernels of a pass take these seven once for all its blocks */
int slai_dec_same_launch(const slai_dec_format* a, const slai_dec_format* b)
{
  return a->C == b->C && a->bps == b->bps && a->ms == b->ms && a->order == b->order && a->ntaps == b->ntaps
         && a->lms == b->lms && a->lshift == b->lshift;
}

/* qsort order of a call's files: the `alone` ones last, equal launch keys next to each other, item order within a key */
int slai_dec_file_cmp(const void* pa, const void* pb)
{
  const slai_dec_file* a = (const slai_dec_file*)pa;
  const slai_dec_file* b = (const slai_dec_file*)pb;
  const uint32_t ka[8] = { (uint32_t)a->alone, a->f.C, a->f.bps, a->f.ms, a->f.order, a->f.ntaps, a->f.lms, a->f.lshift };
  const uint32_t kb[8] = { (uint32_t)b->alone, b->f.C, b->f.bps, b->f.ms, b->f.order, b->f.ntaps, b->f.lms, b->f.lshift };
  int k;
  for (k = 0; k < 8; k++) { if (ka[k] != kb[k]) { return (ka[k] < kb[k]) ? -1 : 1; } }
  return (a->item < b->item) ? -1 : (a->item > b->item);
}

/* Where the pass that starts at files[p0] ends; files[0, n) are the sorted files that are not `alone`.  A file costs (extent +
 * SLAI_DEC_BATCH_ALIGN) * C sample-channels and bytes + 4 bytes; the first file is always admitted, the pass ends where the
 * launch key changes or where one more file would exceed a cap. */
uint32_t slai_dec_cut(const slai_dec_file* files, uint32_t p0, uint32_t n, uint64_t cap_samples, uint64_t cap_bytes)
{
  uint64_t smp = 0, bytes = 0;
  uint32_t p1 = p0;
  while (p1 < n && slai_dec_same_launch(&files[p1].f, &files[p0].f)) {
    const uint64_t s1 = ((uint64_t)files[p1].extent + SLAI_DEC_BATCH_ALIGN) * files[p1].f.C;
    const uint64_t b1 = (uint64_t)files[p1].bytes + 4;
    if (p1 > p0 && (smp + s1 > cap_samples || bytes + b1 > cap_bytes)) { break; }
    smp += s1; bytes += b1; p1++;
  }
  return p1;
}

/* The layout of the pass files[0, nf): every file's image at the next 4-byte offset, its plane region at the next multiple of
 * SLAI_DEC_BATCH_ALIGN samples.  Out: the image's bytes, the samples per plane (0 when no file has any), the blocks. */
void slai_dec_layout(slai_dec_file* files, uint32_t nf, uint64_t* img_bytes, uint64_t* span, uint32_t* nb)
{
  uint32_t i;
  *img_bytes = 0; *span = 0; *nb = 0;
  for (i = 0; i < nf; i++) {
    files[i].img_off = *img_bytes; *img_bytes += ((uint64_t)files[i].bytes + 3) & ~(uint64_t)3;
    files[i].plane_off = *span; *span += ((uint64_t)files[i].extent + SLAI_DEC_BATCH_ALIGN - 1) / SLAI_DEC_BATCH_ALIGN * SLAI_DEC_BATCH_ALIGN;
    *nb += files[i].nb;
  }
}

/* node capacity of a file's wide walk: the option, or one node per 256 stream bytes and at least 1 << 16 */
uint32_t slai_dec_wide_capacity(uint32_t option, uint32_t data_size)
{
  const uint32_t by_size = data_size / 256u;
  if (option != 0) { return option; }
  return (by_size < (1u << 16)) ? (1u << 16) : by_size;
}

/* the files of files[0, nf) of at least `threshold` bytes (0: none), the SLAI_DEC_WIDE_MAX longest of them, longest first,
 * equal sizes in item order -> pick[] (indices into files), their number */
uint32_t slai_dec_pick_wide(const slai_dec_file* files, uint32_t nf, uint32_t threshold, uint32_t pick[SLAI_DEC_WIDE_MAX])
{
  uint32_t n = 0, i, k;
  if (threshold == 0) { return 0; }
  for (i = 0; i < nf; i++) {
    const uint32_t size = files[i].bytes;
    if (size < threshold) { continue; }
    for (k = n; k > 0; k--) {
      const uint32_t ps = files[pick[k - 1]].bytes;
      if (ps > size || (ps == size && files[pick[k - 1]].item < files[i].item)) { break; }
      if (k < SLAI_DEC_WIDE_MAX) { pick[k] = pick[k - 1]; }
    }
    if (k < SLAI_DEC_WIDE_MAX) { pick[k] = i; if (n < SLAI_DEC_WIDE_MAX) { n++; } }
  }
  return n;
}
