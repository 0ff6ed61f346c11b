// ---------------------------------------------------------------------------------------------
// The wide walk (sla_hip_launch_dec_walk_wide): the block table of ONE long resident stream, built by the whole device
// where k_dec_walk follows the chain on one lane.  Its result and rows are k_dec_walk's, byte for byte.
//
// A NODE is a byte position p at which the lane walk would keep a block if it ever got there: 43 <= p, p + 11 <=
// data_size, FF FF at p, 8 <= (size field + 6 mod 2^32) <= data_size - p -- its three chain checks, with its 32-bit
// wrap.  Nodes are found independently; each has at most one successor, the node at p + bsize, strictly ahead of it, so
// the nodes are a forest and the file's chain is the path from the node at byte 43 (node 0 when it exists, since no node
// lies below 43).  The path is ranked by pointer doubling.
//
// Positions are kept in the coordinate q = p + head, head = src & 15, so that the 32-byte WORDS of the find kernel are
// aligned 16-byte loads of the address space: word w covers q in [32w, 32w + 32) and is one uint32 of the bitmap.
//   k_wide_find   one lane per word, three aligned 16-byte loads (only those that overlap the stream, as k_dec_gather;
//                 the ten header bytes of a candidate reach at most 9 bytes into the third), 32 positions tested from
//                 registers; the word's bit mask is stored and the tile (256 words, one workgroup) counts its bits.
//   k_wide_scan   one workgroup: exclusive prefix of the tile counts in place, the exact node count (also beyond the
//                 capacity) and the starting values of the info words.
//   k_wide_index  per word the index of its first node: tile prefix + prefix of the words in the tile.
//   k_wide_nodes  per set bit the node {pos, bsize, n | crc field << 16}, its successor (index of the word of p + bsize
//                 + bits below it, or none), jump = successor, sum = n, rank = 0 for the node at byte 43 and none for
//                 all others in BOTH rank arrays.  Nodes at or above the capacity are dropped: the walk overflowed.
//   k_wide_round  round r, one launch, arrays ping-ponged: every node doubles its jump (2^r -> 2^(r+1) successors
//                 ahead) and its sample sum; a node whose rank is known (rank < 2^r) copies rank and sample position
//                 across and gives them, plus 2^r and its sum, to its 2^r-th successor.  Two nodes of a path have
//                 distinct 2^r-th successors and such a successor has rank >= 2^r, so it is not known yet and does not
//                 write its own slot: no two lanes write one word, and no lane reads an array this launch writes.
//                 The host launches ceil(log2(min(node_capacity, (data_size - 54) / 8 + 1))) rounds: blocks are at least
//                 8 bytes long and the last starts 11 bytes before the end, so that bounds the path, and after R
//                 rounds every rank below 2^R is known.
//   k_wide_cut    every ranked node tests where the lane walk would end: sample position >= total (OK) or a sample
//                 count above capacity - position or above max_block_samples (BUF); atomicMin of rank * 2 + (BUF) finds
//                 the first.  The ranked node without successor stores the path's length.
//   k_wide_rows   rows in rank order, the header-only row of a BUF stop with crc_check 1, the empty rows behind, and
//                 the result: by the lane of the cut node, or of the last path node when the path runs off the nodes
//                 (that lane applies the lane walk's checks at the byte behind its block for the stop code), or by lane
//                 0 when byte 43 is no node.  On overflow: {0, OK, 0, SLA_HIP_DEC_WIDE_OVERFLOW} and empty rows only.
// Sample positions are 64-bit sums; up to the cut they equal the lane walk's 32-bit pos, which never wraps because
// n <= capacity - pos is tested before it advances.  extent is the sample position at the cut.
// Launch order on the stream is the only ordering; the only atomics are the tile count in LDS and the atomicMin of the
// cut, whose word k_wide_scan initialised in an earlier launch.  Every loop runs a count known on entry.
// ---------------------------------------------------------------------------------------------
#define WIDE_NONE 0xFFFFFFFFu
#define WIDE_TILE 256u           // words per tile = lanes per workgroup of k_wide_find / k_wide_index

struct wide_arrays {             // the scratch carved by the launcher (see SLA_HIP_DEC_WIDE_SCRATCH_BYTES)
  sla_hip_dec_wide_info* info;
  uint32_t* mask;                // [words] one bit per position q
  uint32_t* word_first;          // [words] index of the word's first node
  uint32_t* tile;                // [tiles] count, then exclusive prefix
  uint64_t* sum[2];              // [cap] samples of the 2^r nodes from this one on
  uint64_t* spos[2];             // [cap] sample position of a ranked node
  uint32_t* jump[2];             // [cap] the 2^r-th successor
  uint32_t* rank[2];             // [cap]
  uint32_t* pos;                 // [cap] file position of the sync code
  uint32_t* bsize;               // [cap]
  uint32_t* ncrc;                // [cap] n | crc field << 16
  uint32_t* succ;                // [cap] the successor
};

// the little-endian 32 bits at byte k of the register image x (k static after unrolling)
#define WIDE_LE32(x, k) __builtin_amdgcn_alignbyte((x)[((k) >> 2) + 1], (x)[(k) >> 2], (uint32_t)((k) & 3))

__global__ __launch_bounds__(256)
void k_wide_find(const uint8_t* __restrict__ src, uint32_t data_size, uint32_t words, uint32_t* __restrict__ mask,
                 uint32_t* __restrict__ tile)
{
  __shared__ uint32_t count;
  const uint32_t w = blockIdx.x * WIDE_TILE + threadIdx.x;
  if (threadIdx.x == 0) { count = 0; }
  __syncthreads();
  if (w < words) {
    const uint32_t head = (uint32_t)((uintptr_t)src & 15u);
    const uint64_t qend = (uint64_t)head + data_size;                  // one behind the stream's last byte
    const uint64_t q0 = (uint64_t)w << 5;
    const gather_u4* a = (const gather_u4*)(src - head) + ((uint64_t)w << 1);
    const gather_u4 z = {0u, 0u, 0u, 0u};
    const gather_u4 v0 = a[0];                                           // q0 < qend for every w < words
    const gather_u4 v1 = (q0 + 16u < qend) ? a[1] : z;
    const gather_u4 v2 = (q0 + 32u < qend) ? a[2] : z;
    uint32_t x[12];
    x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w; x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
    x[8] = v2.x; x[9] = v2.y; x[10] = v2.z; x[11] = v2.w;
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 32; k++) {
      if ((WIDE_LE32(x, k) & 0xFFFFu) == 0xFFFFu) {
        const uint64_t q = q0 + (uint32_t)k;
        if (q >= (uint64_t)head + SLA_HEADER_SIZE && q + DEC_WALK_MIN_HEADER <= qend) {
          const uint32_t bsize = __builtin_bswap32(WIDE_LE32(x, k + 2)) + 6u;
          if (bsize >= DEC_WALK_CRC_START && bsize <= (uint32_t)(qend - q)) { m |= 1u << k; }
        }
      }
    }
    mask[w] = m;
    if (m != 0) { atomicAdd(&count, (uint32_t)__popc(m)); }
  }
  __syncthreads();
  if (threadIdx.x == 0) { tile[blockIdx.x] = count; }
}

// inclusive scan of one value per lane over a workgroup of N lanes (N a power of two); s: N words of LDS
template <uint32_t N>
__device__ __forceinline__ uint32_t wide_block_scan(uint32_t v, uint32_t* s)
{
  const uint32_t t = threadIdx.x;
  s[t] = v;
  __syncthreads();
#pragma unroll
  for (uint32_t d = 1; d < N; d <<= 1) {
    const uint32_t add = (t >= d) ? s[t - d] : 0u;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  return s[t];
}

__global__ __launch_bounds__(1024)
void k_wide_scan(uint32_t* __restrict__ tile, uint32_t tiles, sla_hip_dec_wide_info* __restrict__ info)
{
  __shared__ uint32_t s[1024];
  const uint32_t per = (tiles + 1023u) / 1024u;
  const uint32_t lo = threadIdx.x * per, hi = (lo + per < tiles) ? lo + per : tiles;
  uint32_t own = 0;
  for (uint32_t k = lo; k < hi; k++) { own += tile[k]; }
  const uint32_t incl = wide_block_scan<1024>(own, s);
  uint32_t run = incl - own;
  for (uint32_t k = lo; k < hi; k++) { const uint32_t c = tile[k]; tile[k] = run; run += c; }
  if (threadIdx.x == 1023u) {
    sla_hip_dec_wide_info i;
    i.nodes = incl; i.path_len = 0; i.cut = WIDE_NONE; i.reserved = 0;
    *info = i;
  }
}

__global__ __launch_bounds__(256)
void k_wide_index(const uint32_t* __restrict__ mask, uint32_t words, const uint32_t* __restrict__ tile,
                  uint32_t* __restrict__ word_first)
{
  __shared__ uint32_t s[WIDE_TILE];
  const uint32_t w = blockIdx.x * WIDE_TILE + threadIdx.x;
  const uint32_t c = (w < words) ? (uint32_t)__popc(mask[w]) : 0u;
  const uint32_t incl = wide_block_scan<WIDE_TILE>(c, s);
  if (w < words) { word_first[w] = tile[blockIdx.x] + incl - c; }
}

__global__ __launch_bounds__(256)
void k_wide_nodes(const uint8_t* __restrict__ src, uint32_t data_size, uint32_t words, uint32_t cap, wide_arrays A)
{
  const uint32_t w = blockIdx.x * WIDE_TILE + threadIdx.x;
  if (w >= words) { return; }
  uint32_t m = A.mask[w];
  if (m == 0) { return; }
  const uint32_t head = (uint32_t)((uintptr_t)src & 15u);
  uint32_t idx = A.word_first[w];
  const uint32_t cnt = (uint32_t)__popc(m);
  for (uint32_t c = 0; c < cnt; c++, idx++) {
    const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
    m &= m - 1u;
    if (idx >= cap) { continue; }
    const uint32_t p = (uint32_t)((((uint64_t)w << 5) + k) - head);
    const uint8_t* h = src + p;                                          // p + 11 <= data_size: the bit says so
    const uint32_t bsize = (((uint32_t)h[2] << 24) | ((uint32_t)h[3] << 16) | ((uint32_t)h[4] << 8) | h[5]) + 6u;
    const uint32_t n = ((uint32_t)h[8] << 8) | h[9];
    const uint64_t qt = (uint64_t)p + bsize + head;                      // p + bsize <= data_size
    const uint32_t wt = (uint32_t)(qt >> 5), bt = (uint32_t)(qt & 31u);
    uint32_t succ = WIDE_NONE;
    if (wt < words) {
      const uint32_t mt = A.mask[wt];
      if ((mt >> bt) & 1u) { succ = A.word_first[wt] + (uint32_t)__popc(mt & ((1u << bt) - 1u)); }
    }
    A.pos[idx] = p; A.bsize[idx] = bsize; A.ncrc[idx] = n | ((((uint32_t)h[6] << 8) | h[7]) << 16);
    A.succ[idx] = succ; A.jump[0][idx] = succ; A.sum[0][idx] = n;
    A.rank[0][idx] = (p == SLA_HEADER_SIZE) ? 0u : WIDE_NONE; A.rank[1][idx] = WIDE_NONE;
    A.spos[0][idx] = 0;
  }
}

// the nodes the later kernels work on: none after an overflow
__device__ __forceinline__ uint32_t wide_count(const sla_hip_dec_wide_info* info, uint32_t cap)
{
  const uint32_t n = info->nodes;
  return (n > cap) ? 0u : n;
}

__global__ __launch_bounds__(256)
void k_wide_round(uint32_t cap, uint32_t step, wide_arrays A, uint32_t from)
{
  const uint32_t count = wide_count(A.info, cap), to = from ^ 1u;
  const uint32_t nt = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += nt) {
    const uint32_t j = A.jump[from][i];
    const uint64_t s = A.sum[from][i];
    const uint32_t rk = A.rank[from][i];
    A.jump[to][i] = (j != WIDE_NONE) ? A.jump[from][j] : WIDE_NONE;
    A.sum[to][i] = (j != WIDE_NONE) ? s + A.sum[from][j] : s;
    if (rk != WIDE_NONE) {
      const uint64_t sp = A.spos[from][i];
      A.rank[to][i] = rk; A.spos[to][i] = sp;
      if (j != WIDE_NONE) { A.rank[to][j] = rk + step; A.spos[to][j] = sp + s; }
    }
  }
}

__global__ __launch_bounds__(256)
void k_wide_cut(sla_hip_dec_walk_file fi, uint32_t cap_n, uint32_t cap, wide_arrays A, uint32_t fin)
{
  const uint32_t count = wide_count(A.info, cap);
  const uint32_t nt = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += nt) {
    const uint32_t rk = A.rank[fin][i];
    if (rk == WIDE_NONE) { continue; }
    const uint64_t sp = A.spos[fin][i];
    const uint32_t n = A.ncrc[i] & 0xFFFFu;
    if (sp >= fi.total) { atomicMin(&A.info->cut, rk << 1); }
    else if (sp > fi.capacity || n > fi.capacity - sp || n > cap_n) { atomicMin(&A.info->cut, (rk << 1) | 1u); }
    if (A.succ[i] == WIDE_NONE) { A.info->path_len = rk + 1u; }
  }
}

// the stop code of the lane walk at byte `off`, where no node is (off <= data_size, or 43)
__device__ __forceinline__ uint32_t wide_stop_at(const uint8_t* src, uint32_t data_size, uint32_t off)
{
  if (off > data_size || data_size - off < DEC_WALK_MIN_HEADER) { return SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; }
  const uint8_t* p = src + off;
  if (p[0] != 0xFFu || p[1] != 0xFFu) { return SLA_APIRESULT_FAILED_TO_FIND_SYNC_CODE; }
  return SLA_APIRESULT_INSUFFICIENT_DATA_SIZE;                          // its size field: it would be a node otherwise
}

__device__ __forceinline__ void wide_empty_row(const sla_hip_dec_walk_file& fi, uint32_t r, sla_hip_dec_block* blocks,
                                               uint64_t* block_end, uint32_t* crc_field)
{
  sla_hip_dec_block b;
  b.byte_off = fi.img_off; b.byte_len = DEC_WALK_CRC_START; b.smp_off = fi.plane_off; b.num_samples = 0; b.flags = SLA_HIP_DEC_HEADER_ONLY;
  blocks[fi.first + r] = b;
  block_end[fi.first + r] = fi.img_off + fi.data_size;
  crc_field[fi.first + r] = 0;
}

__global__ __launch_bounds__(256)
void k_wide_rows(sla_hip_dec_walk_file fi, uint32_t crc_check, uint32_t cap, wide_arrays A, uint32_t fin,
                 sla_hip_dec_walk_result* __restrict__ result, sla_hip_dec_block* __restrict__ blocks,
                 uint64_t* __restrict__ block_end, uint32_t* __restrict__ crc_field)
{
  const sla_hip_dec_wide_info info = *A.info;
  const uint32_t rows = (blocks != nullptr) ? fi.max_rows : 0u;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
  const bool over = info.nodes > cap;
  const uint32_t count = over ? 0u : info.nodes;
  const uint32_t kc = info.cut >> 1;
  const bool cut = info.cut != WIDE_NONE, buf = cut && (info.cut & 1u) != 0;
  const uint32_t nb = over ? 0u : (cut ? kc + ((buf && crc_check == 1u) ? 1u : 0u) : info.path_len);
  for (uint32_t i = tid; i < count; i += nt) {
    const uint32_t rk = A.rank[fin][i];
    if (rk == WIDE_NONE) { continue; }
    const uint64_t sp = A.spos[fin][i];
    const uint32_t n = A.ncrc[i] & 0xFFFFu;
    if (rk < nb && rk < rows) {
      sla_hip_dec_block b;
      b.byte_off = fi.img_off + A.pos[i]; b.byte_len = A.bsize[i]; b.smp_off = fi.plane_off + (uint32_t)sp; b.num_samples = n;
      b.flags = (cut && rk == kc) ? SLA_HIP_DEC_HEADER_ONLY : 0u;
      blocks[fi.first + rk] = b;
      block_end[fi.first + rk] = fi.img_off + fi.data_size;
      crc_field[fi.first + rk] = A.ncrc[i] >> 16;
    }
    sla_hip_dec_walk_result res;
    res.reserved = 0;
    if (cut && rk == kc) {
      res.num_blocks = nb; res.stop = buf ? SLA_APIRESULT_INSUFFICIENT_BUFFER_SIZE : SLA_APIRESULT_OK; res.extent = (uint32_t)sp;
      result[0] = res;
    } else if (!cut && A.succ[i] == WIDE_NONE) {
      // the last node of the path and no cut on it: every node is kept, and the walk ends behind this one
      res.num_blocks = nb; res.extent = (uint32_t)(sp + n);
      res.stop = (sp + n >= fi.total) ? SLA_APIRESULT_OK : wide_stop_at(fi.src, fi.data_size, A.pos[i] + A.bsize[i]);
      result[0] = res;
    }
  }
  if (tid == 0 && (over || (!cut && info.path_len == 0))) {
    sla_hip_dec_walk_result res;
    res.num_blocks = 0; res.extent = 0; res.reserved = over ? SLA_HIP_DEC_WIDE_OVERFLOW : 0u;
    res.stop = (over || fi.total == 0) ? SLA_APIRESULT_OK : wide_stop_at(fi.src, fi.data_size, SLA_HEADER_SIZE);
    result[0] = res;
  }
  for (uint32_t r = tid; r < rows; r += nt) {
    if (r >= nb) { wide_empty_row(fi, r, blocks, block_end, crc_field); }
  }
}

// a file without samples or too short for a block: the result and the empty rows, nothing else (scratch: the info words)
__global__ __launch_bounds__(256)
void k_wide_none(sla_hip_dec_walk_file fi, sla_hip_dec_wide_info* __restrict__ info, sla_hip_dec_walk_result* __restrict__ result,
                 sla_hip_dec_block* __restrict__ blocks, uint64_t* __restrict__ block_end, uint32_t* __restrict__ crc_field)
{
  const uint32_t rows = (blocks != nullptr) ? fi.max_rows : 0u;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
  if (tid == 0) {
    sla_hip_dec_walk_result res;
    sla_hip_dec_wide_info i;
    res.num_blocks = 0; res.extent = 0; res.reserved = 0;
    res.stop = (fi.total == 0) ? SLA_APIRESULT_OK : SLA_APIRESULT_INSUFFICIENT_DATA_SIZE;   // off > data_size or < 11 bytes left
    result[0] = res;
    i.nodes = 0; i.path_len = 0; i.cut = WIDE_NONE; i.reserved = 0;
    *info = i;
  }
  for (uint32_t r = tid; r < rows; r += nt) { wide_empty_row(fi, r, blocks, block_end, crc_field); }
}
