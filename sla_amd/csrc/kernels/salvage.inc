// ---------------------------------------------------------------------------------------------
// The salvage scan (sla_hip_launch_dec_salvage_scan): the blocks of ONE resident stream whose chain is broken that can
// still be decoded, found by the whole device.  The rule is stated in include/sla_hip.h (sla_hip_salvage_resident) and,
// executable, in tests/salvagemodel.py.
//
// It stands on the wide walk (walk_wide.inc): k_wide_find / k_wide_scan / k_wide_index / k_wide_nodes give the nodes --
// every byte position at which a block could start -- numbered in ascending position, with {pos, bsize, n | crc field
// << 16} and the successor (the node at pos + bsize).  Behind them:
//   k_salvage_sound  one wave per node: n <= max_block_samples and bsize <= SLA_HIP_SALVAGE_MAX_BLOCK_BYTES first, then
//                    crc16_wave over [pos + 8, pos + bsize) against the stored field.  The cap bounds the CRC work a
//                    decoy's size field can cause.  Writes the sound flag, counts the sound nodes.
//   k_salvage_link   the sound successor of a node: its successor when both are sound, else none; jump = that, sum = n,
//                    last = the node itself, rank 0 for the start node and none for all others.  Start node of pass 0:
//                    the sound node at byte 43 (the prefix); of pass 1: the node q that k_salvage_pick chose (the suffix).
//   k_salvage_round  pointer doubling as k_wide_round, arrays ping-ponged, plus `last`: after R rounds (R as for the wide
//                    walk: 2^R is no less than the longest path) every node's jump is none, its sum the samples of its
//                    whole all-sound chain, its last the chain's final node; the path from the start node is ranked and
//                    has its sample positions.
//   k_salvage_cut    pass 0: atomicMin of the rank of the first path node with sample position + n > total (the prefix
//                    ends in front of it); both passes: the path's length, by its last node.
//   k_salvage_prefix the prefix rows in rank order; the prefix end {p0, s0} by the lane of its last block (lane 0 when it
//                    is empty); every node's chain end byte and chain sample sum kept for the pick.
//   k_salvage_pick   atomicMin of the index (= ascending position) of the sound nodes at or behind p0 whose chain ends at
//                    the stream's last byte with a sample sum <= total - s0.
//   k_salvage_rows   the suffix rows behind the prefix rows, at sample total - T + position on the path; the empty rows
//                    behind them; the result.
// Launch order on the stream is the only ordering: no kernel waits for another workgroup, every word an atomic touches
// was initialised by an earlier launch (k_salvage_init), and every loop runs a count known on entry.  The source is read
// by the wide walk's aligned loads and by byte loads inside [src, src + data_size).  After a node overflow every kernel
// sees zero nodes and the result says {overflow, the exact node count}.
// ---------------------------------------------------------------------------------------------
struct salvage_info {            // device words between the launches (64 bytes, behind the wide walk's part of the scratch)
  uint32_t sound;                // sound nodes
  uint32_t cut[2];               // pass 0: rank of the first path node that does not fit; WIDE_NONE: none
  uint32_t path_len[2];          // nodes on the ranked path of the pass
  uint32_t p0, s0;               // the prefix end
  uint32_t q;                    // node index of the suffix start, WIDE_NONE: none
  uint32_t reserved[8];
};

struct salvage_arrays {          // behind the wide walk's arrays in the scratch
  salvage_info* info;
  uint32_t* sound;               // [cap] 1: a sound block
  uint32_t* ssucc;               // [cap] the sound successor
  uint32_t* last[2];             // [cap] the last node reached along the chain
  uint32_t* cend;                // [cap] byte end of the node's all-sound chain
  uint64_t* csum;                // [cap] its samples
};

__global__ __launch_bounds__(64)
void k_salvage_init(salvage_info* __restrict__ info)
{
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    salvage_info i;
    i.sound = 0; i.cut[0] = i.cut[1] = WIDE_NONE; i.path_len[0] = i.path_len[1] = 0; i.p0 = SLA_HEADER_SIZE; i.s0 = 0; i.q = WIDE_NONE;
    for (int k = 0; k < 8; k++) { i.reserved[k] = 0; }
    *info = i;
  }
}

__global__ __launch_bounds__(256)
void k_salvage_sound(const uint8_t* __restrict__ src, uint32_t channels, uint32_t cap_n, uint32_t cap, wide_arrays A, salvage_arrays B)
{
  __shared__ uint16_t table[256];
  crc16_build_table(table);
  __syncthreads();
  const uint32_t count = wide_count(A.info, cap);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nw = gridDim.x * 4u;
  for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < count; i += nw) {
    const uint32_t n = A.ncrc[i] & 0xFFFFu, bsize = A.bsize[i], p = A.pos[i];
    uint32_t ok = 0;
    if (n <= cap_n && bsize <= SLA_HIP_SALVAGE_MAX_BLOCK_BYTES(channels, n)) {       // (uniform over the wave)
      ok = (crc16_wave(src, (uint64_t)p + DEC_WALK_CRC_START, (uint64_t)p + bsize, table, lane) == (A.ncrc[i] >> 16)) ? 1u : 0u;
    }
    if (lane == 0) {
      B.sound[i] = ok;
      if (ok) { atomicAdd(&B.info->sound, 1u); }
    }
  }
}

__global__ __launch_bounds__(256)
void k_salvage_link(uint32_t cap, wide_arrays A, salvage_arrays B, uint32_t pass)
{
  const uint32_t count = wide_count(A.info, cap);
  const uint32_t q = B.info->q;
  const uint32_t nt = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += nt) {
    const uint32_t s = A.succ[i];
    const bool ok = B.sound[i] != 0;
    const uint32_t ss = (ok && s != WIDE_NONE && B.sound[s] != 0) ? s : WIDE_NONE;
    const bool start = (pass == 0) ? (ok && A.pos[i] == SLA_HEADER_SIZE) : (i == q);
    B.ssucc[i] = ss; A.jump[0][i] = ss; A.sum[0][i] = A.ncrc[i] & 0xFFFFu; B.last[0][i] = i;
    A.rank[0][i] = start ? 0u : WIDE_NONE; A.rank[1][i] = WIDE_NONE; A.spos[0][i] = 0;
  }
}

__global__ __launch_bounds__(256)
void k_salvage_round(uint32_t cap, uint32_t step, wide_arrays A, salvage_arrays B, uint32_t from)
{
  const uint32_t count = wide_count(A.info, cap), to = from ^ 1u;
  const uint32_t nt = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += nt) {
    const uint32_t j = A.jump[from][i];
    const uint64_t s = A.sum[from][i];
    const uint32_t rk = A.rank[from][i];
    A.jump[to][i] = (j != WIDE_NONE) ? A.jump[from][j] : WIDE_NONE;
    A.sum[to][i] = (j != WIDE_NONE) ? s + A.sum[from][j] : s;
    B.last[to][i] = (j != WIDE_NONE) ? B.last[from][j] : B.last[from][i];
    if (rk != WIDE_NONE) {
      const uint64_t sp = A.spos[from][i];
      A.rank[to][i] = rk; A.spos[to][i] = sp;
      if (j != WIDE_NONE) { A.rank[to][j] = rk + step; A.spos[to][j] = sp + s; }
    }
  }
}

__global__ __launch_bounds__(256)
void k_salvage_cut(uint32_t total, uint32_t cap, wide_arrays A, salvage_arrays B, uint32_t fin, uint32_t pass)
{
  const uint32_t count = wide_count(A.info, cap);
  const uint32_t nt = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += nt) {
    const uint32_t rk = A.rank[fin][i];
    if (rk == WIDE_NONE) { continue; }
    if (pass == 0 && A.spos[fin][i] + (A.ncrc[i] & 0xFFFFu) > total) { atomicMin(&B.info->cut[0], rk); }
    if (B.ssucc[i] == WIDE_NONE) { B.info->path_len[pass] = rk + 1u; }
  }
}

__device__ __forceinline__ void salvage_row(const sla_hip_dec_walk_file& fi, uint32_t r, uint32_t pos, uint32_t bsize, uint32_t smp,
                                            uint32_t ncrc, sla_hip_dec_block* blocks, uint64_t* block_end, uint32_t* crc_field)
{
  sla_hip_dec_block b;
  b.byte_off = fi.img_off + pos; b.byte_len = bsize; b.smp_off = fi.plane_off + smp; b.num_samples = ncrc & 0xFFFFu; b.flags = 0;
  blocks[fi.first + r] = b;
  block_end[fi.first + r] = fi.img_off + fi.data_size;
  crc_field[fi.first + r] = ncrc >> 16;
}

// blocks of the prefix: the ranked path of pass 0 up to the cut
__device__ __forceinline__ uint32_t salvage_prefix_len(const salvage_info& si)
{
  return (si.cut[0] < si.path_len[0]) ? si.cut[0] : si.path_len[0];
}

__global__ __launch_bounds__(256)
void k_salvage_prefix(sla_hip_dec_walk_file fi, uint32_t cap, wide_arrays A, salvage_arrays B, uint32_t fin,
                      sla_hip_dec_block* __restrict__ blocks, uint64_t* __restrict__ block_end, uint32_t* __restrict__ crc_field)
{
  const uint32_t count = wide_count(A.info, cap);
  const salvage_info si = *B.info;
  const uint32_t P = salvage_prefix_len(si);
  const uint32_t rows = (blocks != nullptr) ? fi.max_rows : 0u;
  const uint32_t nt = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += nt) {
    const uint32_t l = B.last[fin][i];
    B.cend[i] = A.pos[l] + A.bsize[l];
    B.csum[i] = A.sum[fin][i];
    const uint32_t rk = A.rank[fin][i];
    if (rk == WIDE_NONE || rk >= P) { continue; }
    const uint64_t sp = A.spos[fin][i];
    if (rk < rows) { salvage_row(fi, rk, A.pos[i], A.bsize[i], (uint32_t)sp, A.ncrc[i], blocks, block_end, crc_field); }
    if (rk + 1u == P) { B.info->p0 = A.pos[i] + A.bsize[i]; B.info->s0 = (uint32_t)sp + (A.ncrc[i] & 0xFFFFu); }
  }
}

__global__ __launch_bounds__(256)
void k_salvage_pick(sla_hip_dec_walk_file fi, uint32_t cap, wide_arrays A, salvage_arrays B)
{
  const uint32_t count = wide_count(A.info, cap);
  const uint32_t p0 = B.info->p0, s0 = B.info->s0;
  const uint32_t nt = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += nt) {
    if (B.sound[i] != 0 && A.pos[i] >= p0 && B.cend[i] == fi.data_size && B.csum[i] <= (uint64_t)(fi.total - s0)) {
      atomicMin(&B.info->q, i);
    }
  }
}

__global__ __launch_bounds__(256)
void k_salvage_rows(sla_hip_dec_walk_file fi, uint32_t cap, wide_arrays A, salvage_arrays B, uint32_t fin,
                    sla_hip_salvage_scan* __restrict__ result, sla_hip_dec_block* __restrict__ blocks,
                    uint64_t* __restrict__ block_end, uint32_t* __restrict__ crc_field)
{
  const sla_hip_dec_wide_info wi = *A.info;
  const salvage_info si = *B.info;
  const bool over = wi.nodes > cap;
  const uint32_t count = over ? 0u : wi.nodes;
  const uint32_t P = over ? 0u : salvage_prefix_len(si);
  const bool have = !over && si.q != WIDE_NONE;
  const uint32_t K = have ? si.path_len[1] : 0u;
  const uint32_t T = have ? (uint32_t)B.csum[si.q] : 0u;
  const uint32_t rows = (blocks != nullptr) ? fi.max_rows : 0u;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
  for (uint32_t i = tid; have && i < count; i += nt) {
    const uint32_t rk = A.rank[fin][i];
    if (rk == WIDE_NONE || P + rk >= rows) { continue; }
    salvage_row(fi, P + rk, A.pos[i], A.bsize[i], fi.total - T + (uint32_t)A.spos[fin][i], A.ncrc[i], blocks, block_end, crc_field);
  }
  for (uint32_t r = tid; r < rows; r += nt) {
    if (r >= P + K) { wide_empty_row(fi, r, blocks, block_end, crc_field); }
  }
  if (tid == 0) {
    sla_hip_salvage_scan res;
    res.prefix_blocks = P; res.prefix_samples = over ? 0u : si.s0; res.prefix_end = over ? (uint32_t)SLA_HEADER_SIZE : si.p0;
    res.suffix_byte = have ? A.pos[si.q] : 0u; res.suffix_samples = T; res.suffix_blocks = K;
    res.nodes = wi.nodes; res.sound_nodes = over ? 0u : si.sound; res.overflow = over ? 1u : 0u;
    res.reserved[0] = res.reserved[1] = res.reserved[2] = 0;
    result[0] = res;
  }
}

// a stream too short for a block: the result and the empty rows, nothing else (scratch: the info words)
__global__ __launch_bounds__(256)
void k_salvage_none(sla_hip_dec_walk_file fi, sla_hip_dec_wide_info* __restrict__ info, sla_hip_salvage_scan* __restrict__ result,
                    sla_hip_dec_block* __restrict__ blocks, uint64_t* __restrict__ block_end, uint32_t* __restrict__ crc_field)
{
  const uint32_t rows = (blocks != nullptr) ? fi.max_rows : 0u;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
  if (tid == 0) {
    sla_hip_salvage_scan res;
    sla_hip_dec_wide_info i;
    res.prefix_blocks = 0; res.prefix_samples = 0; res.prefix_end = SLA_HEADER_SIZE; res.suffix_byte = 0; res.suffix_samples = 0;
    res.suffix_blocks = 0; res.nodes = 0; res.sound_nodes = 0; res.overflow = 0;
    res.reserved[0] = res.reserved[1] = res.reserved[2] = 0;
    result[0] = res;
    i.nodes = 0; i.path_len = 0; i.cut = WIDE_NONE; i.reserved = 0;
    *info = i;
  }
  for (uint32_t r = tid; r < rows; r += nt) { wide_empty_row(fi, r, blocks, block_end, crc_field); }
}

// ---------------------------------------------------------------------------------------------
// Mode 1 of sla_hip_salvage_resident: the chain is intact, rows whose stored CRC differs from the CRC of their bytes in
// the pass image are not to be entropy-decoded.  One wave per row: the row gets SLA_HIP_DEC_HEADER_ONLY and bad[row] = 1,
// else bad[row] = 0.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_salvage_crc(const uint8_t* __restrict__ image, sla_hip_dec_block* __restrict__ blocks, const uint32_t* __restrict__ crc_field,
                   uint32_t num_blocks, uint32_t* __restrict__ bad)
{
  __shared__ uint16_t table[256];
  crc16_build_table(table);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (j >= num_blocks) { return; }
  const sla_hip_dec_block b = blocks[j];
  const uint32_t crc = crc16_wave(image, b.byte_off + DEC_WALK_CRC_START, b.byte_off + b.byte_len, table, lane);
  if (lane == 0) {
    const uint32_t differs = (crc != crc_field[j]) ? 1u : 0u;
    bad[j] = differs;
    if (differs) { blocks[j].flags = b.flags | SLA_HIP_DEC_HEADER_ONLY; }
  }
}

// ---------------------------------------------------------------------------------------------
// k_dec_conceal: the plane regions [smp_off, smp_off + num_samples) of a device list, in all C planes, written zero --
// launched before the emit, so that a concealed block or a lost range leaves as silence: zero planes stay zero through
// mid/side and the left shift.  Entries are clipped to the plane stride.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_dec_conceal(int32_t* __restrict__ planes, uint64_t stride, uint32_t num_channels, const sla_hip_dec_conceal* __restrict__ list,
                   uint32_t count)
{
  for (uint32_t e = blockIdx.y; e < count; e += gridDim.y) {
    const sla_hip_dec_conceal c = list[e];
    const uint64_t lo = c.smp_off, hi = ((uint64_t)c.smp_off + c.num_samples < stride) ? (uint64_t)c.smp_off + c.num_samples : stride;
    for (uint64_t i = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (uint64_t)gridDim.x * blockDim.x) {
      for (uint32_t ch = 0; ch < num_channels; ch++) { planes[(uint64_t)ch * stride + i] = 0; }
    }
  }
}
