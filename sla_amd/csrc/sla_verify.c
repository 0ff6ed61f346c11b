/*
 * sla_verify.c -- tables of the encoder's verification pass (option "verify"): pure host arithmetic, no device calls.
 *
 * The device pack leaves a table of sla_hip_pack_block on the host (where every block sits in the planes and in the
 * image).  The decoder's kernels want sla_hip_dec_block plus, per block, the byte end of its file in the image; the
 * compare kernel wants what the packer expects the parser to find and the file (segment) of every block.
 */
#include "sla_internal.h"

uint32_t slai_verify_tables(const sla_hip_pack_block* pb, uint32_t num_blocks, const slai_verify_seg* segs, uint32_t num_segs,
                            uint32_t num_channels, sla_hip_dec_block* blocks, uint64_t* block_end,
                            sla_hip_verify_expect* expect, uint32_t* seg_of_block, uint64_t* compared,
                            uint32_t* max_block_samples)
{
  uint32_t b, sg = 0, out = 0, longest = 0;
  uint64_t total = 0;
  for (b = 0; b < num_blocks && num_segs > 0; b++) {
    /* blocks and segments both ascend in the image; a segment without blocks (an empty file: its header only) is passed */
    while (sg + 1 < num_segs && pb[b].out_off >= segs[sg].img_off + segs[sg].img_bytes) { sg++; }
    if (pb[b].out_off < segs[sg].img_off || pb[b].out_off + pb[b].out_bytes > segs[sg].img_off + segs[sg].img_bytes) { continue; }
    if (!segs[sg].deliver) { continue; }
    blocks[out].byte_off = pb[b].out_off;
    blocks[out].byte_len = pb[b].out_bytes;
    blocks[out].smp_off = (uint32_t)pb[b].blk_off;
    blocks[out].num_samples = pb[b].num_samples;
    blocks[out].flags = 0;
    block_end[out] = segs[sg].img_off + segs[sg].img_bytes;
    expect[out].type = pb[b].type;
    expect[out].bytes = pb[b].out_bytes;
    seg_of_block[out] = sg;
    total += (uint64_t)num_channels * pb[b].num_samples;
    if (pb[b].num_samples > longest) { longest = pb[b].num_samples; }
    out++;
  }
  if (compared != NULL) { *compared = total; }
  if (max_block_samples != NULL) { *max_block_samples = longest; }
  return out;
}
