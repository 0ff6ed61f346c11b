// k_dec_judge: the verdict of sla_hip_decode_windows_indexed on the device -- what win_examine of sla_decoder.c does on the
// host for the synchronous window call, plus the check that the index the rows were laid out from still describes the bytes.
// One wave per item, four items per workgroup; the lanes stride the item's rows [first, first + nb) of the pass table, so
// that consecutive lanes load consecutive rows and infos.  A row's code, by the first rule that applies:
//   1. stale index: the ten chain-header bytes at the row's place in the pass image are not FF FF, size field + 6 ==
//      byte_len, sample count == num_samples (or do not lie inside the image)       -> DETECT_DATA_CORRUPTION
//   2. crc_check and info.crc != the big-endian field at byte 6                    -> DETECT_DATA_CORRUPTION
//   3. info.type > 2                                                               -> INVALID_HEADER_FORMAT
//   4. info.type == 0 and !lms_ok                                                  -> FAILED_TO_SYNTHESIZE
//   5. info.overrun or info.used_bytes != byte_len                                 -> DETECT_DATA_CORRUPTION
// The item's result is the code of its lowest failing row -- a wave-wide minimum of (row << 8) | code -- or, with none, the
// host's stop code.  Lane 0 stores {result, output_num_samples} and, for a failed item, patches the item's emit entry to
// "nothing decoded": done = 0, fill_end = the item's fill_end.  No atomics, no workgroup waits for another, every loop's
// trip count is known on entry.  Table positions outside the tables (rows, emit entry, outcome) are not touched: such an
// item is judged NG.
#define JUDGE_CORRUPT  11u    /* SLA_APIRESULT_DETECT_DATA_CORRUPTION */
#define JUDGE_HEADER   10u    /* SLA_APIRESULT_INVALID_HEADER_FORMAT */
#define JUDGE_SYNTH     8u    /* SLA_APIRESULT_FAILED_TO_SYNTHESIZE */
#define JUDGE_CLEAN    (~(uint64_t)0)

__device__ __forceinline__ uint32_t judge_row(const uint8_t* __restrict__ image, uint64_t image_bytes, const sla_hip_dec_block b,
                                              const sla_hip_dec_info in, uint32_t crc_check, uint32_t lms_ok)
{
  if (b.byte_off > image_bytes || image_bytes - b.byte_off < 10u) { return JUDGE_CORRUPT; }
  const uint8_t* p = image + b.byte_off;
  uint32_t h[10];
#pragma unroll
  for (int k = 0; k < 10; k++) { h[k] = p[k]; }
  const uint32_t size_field = (h[2] << 24) | (h[3] << 16) | (h[4] << 8) | h[5];
  if (h[0] != 0xFFu || h[1] != 0xFFu || size_field + 6u != b.byte_len || ((h[8] << 8) | h[9]) != b.num_samples) { return JUDGE_CORRUPT; }
  if (crc_check && in.crc != ((h[6] << 8) | h[7])) { return JUDGE_CORRUPT; }
  if (in.type > 2u) { return JUDGE_HEADER; }
  if (in.type == 0u && !lms_ok) { return JUDGE_SYNTH; }
  if (in.overrun != 0u || in.used_bytes != b.byte_len) { return JUDGE_CORRUPT; }
  return 0u;
}

__global__ __launch_bounds__(256)
void k_dec_judge(const uint8_t* __restrict__ image, uint64_t image_bytes, const sla_hip_dec_block* __restrict__ blocks,
                 const sla_hip_dec_info* __restrict__ info, uint32_t num_blocks, const sla_hip_dec_judge_item* __restrict__ items,
                 uint32_t num_items, uint32_t crc_check, uint32_t lms_ok, sla_hip_dec_emit* __restrict__ emit, uint32_t num_emit,
                 sla_hip_window_outcome* __restrict__ outcomes, uint32_t num_outcomes)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t item = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (item >= num_items) { return; }                            // wave-uniform
  const sla_hip_dec_judge_item it = items[item];
  const bool rows_ok = it.first <= num_blocks && it.nb <= num_blocks - it.first;
  const uint32_t nb = rows_ok ? it.nb : 0u;
  uint64_t key = JUDGE_CLEAN;
  for (uint32_t r = lane; r < nb; r += 64u) {                   // rows ascend per lane: the first failure is the lane's lowest
    if (key != JUDGE_CLEAN) { continue; }
    const uint32_t code = judge_row(image, image_bytes, blocks[it.first + r], info[it.first + r], crc_check, lms_ok);
    if (code != 0u) { key = ((uint64_t)r << 8) | code; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), off);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    key = (o < key) ? o : key;
  }
  if (lane != 0u) { return; }
  const uint32_t result = !rows_ok ? 1u /* SLA_APIRESULT_NG */ : (key != JUDGE_CLEAN) ? (uint32_t)(key & 0xFFu) : it.stop;
  if (it.outcome < num_outcomes) {
    sla_hip_window_outcome o;
    o.result = (int32_t)result; o.output_num_samples = (result == 0u) ? it.ok_samples : 0u;
    outcomes[it.outcome] = o;
  }
  if (result != 0u && it.emit < num_emit) {
    emit[it.emit].done = 0u;
    emit[it.emit].fill_end = it.fill_end;
  }
}
