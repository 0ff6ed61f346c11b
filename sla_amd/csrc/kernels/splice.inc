// kernels/splice.inc -- part of sla_decode.hip: the three kernels of sla_hip_splice_resident (include/sla_hip.h).
//
// k_splice_check   one wave per emitted block.  A verbatim block: rule 1 of k_dec_judge on the ten chain-header bytes where
//                  the row says the block lies in its SOURCE, the type the row's length implies (11 bytes <=> SILENT), and
//                  with crc_check the CRC16 over [8, byte_len).  An edge block: the code k_dec_judge gave its row, else the
//                  type rule, else every folded sample of the kept range must fit its channel's width.  A failing block
//                  lowers its item's verdict word to (ordinal << 8) | code (64-bit vector atomic minimum): the item's result
//                  is the code of its first failing block in output order.  Clean blocks touch nothing.
// k_splice_edges   one workgroup per edge block: the decoded, pre-finish planes (right-justified, mid/side folded) are a RAW
//                  block's coded values before the zig-zag fold.  Eight frames are exactly W bytes, so a lane that owns frames
//                  8k .. 8k+7 owns a byte-aligned chunk and needs no carry from its neighbour.  The block passes through LDS in
//                  tiles of whole chunks (the 11 header bytes ride in tile 0), laid out there at the destination's 16-byte
//                  phase: the bytes go out as 16-byte stores to aligned chunks that lie wholly inside the tile and as guarded
//                  byte stores elsewhere.  Wave 0 takes each tile's CRC16 from LDS (crc16_wave) and joins the tiles with
//                  crc16_mulmod; the CRC field is stored last.  No byte outside [dst, dst + len) is written.
// k_splice_copy    source pointer to destination pointer at any pair of alignments, k_enc_emit's scheme (kernels/emit.inc):
//                  aligned 16-byte chunks of the destination from two aligned 16-byte loads, heads and tails byte by byte.
#define SPLICE_CORRUPT   11u     /* SLA_APIRESULT_DETECT_DATA_CORRUPTION */
#define SPLICE_NG         1u
#define SPLICE_TILE_BYTES 32768u

typedef uint32_t splice_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t splice_fold(int32_t s) { const uint32_t u = (uint32_t)s << 1; return (s < 0) ? ~u : u; }

// x^(8 * bytes) mod P: what crc16_mulmod takes to move a CRC (normal bit order) over `bytes` more bytes
__device__ __forceinline__ uint32_t splice_crc_shift(uint64_t bytes)
{
  uint32_t g = 1, base = 2;
  for (uint64_t k = 8 * bytes; k != 0; k >>= 1) {
    if (k & 1) { g = crc16_mulmod(g, base); }
    base = crc16_mulmod(base, base);
  }
  return g;
}

__global__ __launch_bounds__(256)
void k_splice_check(const sla_hip_splice_check* __restrict__ table, uint32_t num_entries, uint32_t crc_check,
                    const int32_t* __restrict__ planes, uint64_t stride, uint32_t C, uint32_t width, uint32_t ms,
                    const sla_hip_window_outcome* __restrict__ outcomes, uint32_t num_outcomes,
                    unsigned long long* __restrict__ verdicts, uint32_t num_verdicts)
{
  __shared__ uint16_t crc_table[256];
  crc16_build_table(crc_table);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (e >= num_entries) { return; }                              // wave-uniform
  const sla_hip_splice_check g = table[e];
  uint32_t code = 0;
  if (g.src == nullptr || g.byte_len < 11u) { code = SPLICE_CORRUPT; }
  else if (g.edge != SLA_HIP_SPLICE_NO_EDGE) {
    if (g.edge >= num_outcomes || g.plane_off > stride || g.keep > stride - g.plane_off) { code = SPLICE_NG; }
    else { code = (uint32_t)outcomes[g.edge].result; }
  }
  if (code == 0u) {
    const uint8_t* p = g.src;
    uint32_t h[11];
#pragma unroll
    for (int k = 0; k < 11; k++) { h[k] = p[k]; }
    const uint32_t size_field = (h[2] << 24) | (h[3] << 16) | (h[4] << 8) | h[5];
    const uint32_t type = h[10] >> 6;
    if (h[0] != 0xFFu || h[1] != 0xFFu || size_field + 6u != g.byte_len || ((h[8] << 8) | h[9]) != g.num_samples
        || (type == 1u) != (g.byte_len == 11u)) { code = SPLICE_CORRUPT; }
    else if (g.edge == SLA_HIP_SPLICE_NO_EDGE) {
      if (crc_check && crc16_wave(p, 8u, g.byte_len, crc_table, lane) != ((h[6] << 8) | h[7])) { code = SPLICE_CORRUPT; }
    } else if (type != 1u) {
      bool bad = false;
      for (uint32_t c = 0; c < C; c++) {
        const uint32_t w = width + ((c == 1u && ms) ? 1u : 0u);
        if (w >= 32u) { continue; }
        const int32_t* row = planes + (uint64_t)c * stride + g.plane_off;
        for (uint32_t s = lane; s < g.keep; s += 64u) { bad = bad || ((splice_fold(row[s]) >> w) != 0u); }
      }
      if (__any(bad)) { code = SPLICE_CORRUPT; }
    }
  }
  if (lane == 0u && code != 0u && g.verdict < num_verdicts) {
    atomicMin(&verdicts[g.verdict], ((unsigned long long)g.ordinal << 8) | (code & 0xFFu));
  }
}

__global__ __launch_bounds__(256)
void k_splice_edges(const int32_t* __restrict__ planes, uint64_t stride, const sla_hip_splice_edge* __restrict__ table,
                    uint32_t num_entries, uint32_t C, uint32_t width, uint32_t ms)
{
  __shared__ uint16_t crc_table[256];
  __shared__ __attribute__((aligned(16))) uint8_t buf[SPLICE_TILE_BYTES + 32];
  crc16_build_table(crc_table);
  const uint32_t W = C * width + (ms ? 1u : 0u);                 // bits of a frame = bytes of eight
  const uint32_t T = (SPLICE_TILE_BYTES / W > 0u) ? SPLICE_TILE_BYTES / W : 1u;     // chunks of a tile
  for (uint32_t e = blockIdx.x; e < num_entries; e += gridDim.x) {
    __syncthreads();
    const sla_hip_splice_edge g = table[e];
    const uint32_t n = g.num_samples;
    if (g.dst == nullptr || n == 0u || n > 65535u || g.plane_off > stride || n > stride - g.plane_off) { continue; }   // uniform
    const uint32_t silent = (g.silent != 0u) ? 1u : 0u;
    const uint32_t len = 11u + (silent ? 0u : (uint32_t)(((uint64_t)n * W + 7u) >> 3));
    const uint32_t chunks = silent ? 0u : (n + 7u) >> 3;
    const uint32_t tiles = (chunks + T - 1u) / T > 0u ? (chunks + T - 1u) / T : 1u;
    uint8_t* dst = g.dst;
    uint32_t run = 0;                                            // wave 0: the CRC of [8, tile end), normal bit order
    for (uint32_t t = 0; t < tiles; t++) {
      const uint32_t lo = (t == 0u) ? 0u : 11u + t * T * W;
      const uint32_t end = 11u + (t + 1u) * T * W, hi = (end < len) ? end : len;
      const uint32_t head = (uint32_t)((uintptr_t)(dst + lo) & 15u);      // block byte lo + i lives in buf[head + i]
      uint8_t* tile = buf + head;
      if (t == 0u && threadIdx.x < 11u) {
        const uint32_t k = threadIdx.x, size_field = len - 6u;
        uint32_t v = 0xFFu;
        if (k >= 2u && k < 6u) { v = (size_field >> (8u * (5u - k))) & 0xFFu; }
        else if (k == 6u || k == 7u) { v = 0u; }
        else if (k == 8u) { v = n >> 8; }
        else if (k == 9u) { v = n & 0xFFu; }
        else if (k == 10u) { v = silent ? 0x40u : 0x80u; }
        tile[k] = (uint8_t)v;
      }
      const uint32_t k_end = ((t + 1u) * T < chunks) ? (t + 1u) * T : chunks;
      for (uint32_t k = t * T + threadIdx.x; k < k_end; k += blockDim.x) {
        uint8_t* out = tile + (11u + k * W - lo);
        const uint32_t s0 = k << 3, frames = (n - s0 < 8u) ? n - s0 : 8u;
        uint64_t acc = 0;
        uint32_t fill = 0, o = 0;
        for (uint32_t f = 0; f < frames; f++) {
          for (uint32_t c = 0; c < C; c++) {
            uint32_t w = width + ((c == 1u && ms) ? 1u : 0u);
            const uint32_t u = splice_fold(planes[(uint64_t)c * stride + g.plane_off + s0 + f]);
            if (w > 32u) {                                       // the 33-bit side field: a zero bit, then the 32 of the fold
              acc <<= (w - 32u); fill += w - 32u; w = 32u;
              if (fill >= 8u) { out[o++] = (uint8_t)(acc >> (fill - 8u)); fill -= 8u; }
            }
            acc = (acc << w) | (uint64_t)((w == 32u) ? u : (u & ((1u << w) - 1u)));
            fill += w;
            while (fill >= 8u) { out[o++] = (uint8_t)(acc >> (fill - 8u)); fill -= 8u; }
          }
        }
        if (fill != 0u) { out[o++] = (uint8_t)(acc << (8u - fill)); }      // the block's padding bits: zero
      }
      __syncthreads();
      if (threadIdx.x < 64u) {
        const uint32_t from = (lo < 8u) ? 8u : lo;
        const uint32_t crc = crc16_wave(tile, from - lo, hi - lo, crc_table, threadIdx.x);
        run = crc16_mulmod(run, splice_crc_shift(hi - from)) ^ crc16_rev(crc);
      }
      const uint32_t span = hi - lo, nchunks = (head + span + 15u) >> 4;
      for (uint32_t c = threadIdx.x; c < nchunks; c += blockDim.x) {
        const int32_t o0 = (int32_t)(c << 4) - (int32_t)head;   // the chunk's first byte, relative to lo
        if (o0 >= 0 && (uint32_t)o0 + 16u <= span && lo + (uint32_t)o0 >= 8u) {
          *(splice_u4*)(dst + lo + o0) = *(const splice_u4*)(buf + (c << 4));
        } else {
#pragma unroll
          for (int32_t k = 0; k < 16; k++) {
            const int32_t i = o0 + k;
            if (i >= 0 && (uint32_t)i < span && lo + (uint32_t)i != 6u && lo + (uint32_t)i != 7u) { dst[lo + i] = tile[i]; }
          }
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0u) {
      const uint32_t crc = crc16_rev(run);
      dst[6] = (uint8_t)(crc >> 8); dst[7] = (uint8_t)(crc & 0xFFu);
    }
  }
}

__global__ __launch_bounds__(256)
void k_splice_copy(const sla_hip_splice_copy* __restrict__ table, uint32_t num_entries)
{
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (uint64_t)gridDim.x * blockDim.x;
  for (uint32_t e = blockIdx.y; e < num_entries; e += gridDim.y) {
    const sla_hip_splice_copy* g = &table[e];
    const uint8_t* src = g->src;
    uint8_t* dst = g->dst;
    const uint32_t bytes = g->bytes;
    if (src == nullptr || dst == nullptr) { continue; }
    const uint32_t head = (uint32_t)((uintptr_t)dst & 15u);     // bytes of the first chunk before the destination
    const uint64_t chunks = ((uint64_t)head + bytes + 15u) >> 4;
    for (uint64_t c = tid; c < chunks; c += nt) {
      const int64_t o0 = (int64_t)(c << 4) - head;               // the chunk's first byte, relative to the destination
      if (o0 >= 0 && (uint64_t)o0 + 16u <= bytes) {
        const uint32_t o = (uint32_t)o0;
        const uintptr_t s = (uintptr_t)src + o;
        const uint32_t r = (uint32_t)(s & 15u);
        const splice_u4* a = (const splice_u4*)(s & ~(uintptr_t)15);
        const splice_u4 q0 = a[0];                               // holds byte o
        splice_u4 q1 = {0u, 0u, 0u, 0u};
        if (r != 0) { q1 = a[1]; }                               // holds byte o + 16 - r, which is before o + 16 <= bytes
        uint32_t w[5];
        switch (r >> 2) {
          case 0:  w[0] = q0.x; w[1] = q0.y; w[2] = q0.z; w[3] = q0.w; w[4] = q1.x; break;
          case 1:  w[0] = q0.y; w[1] = q0.z; w[2] = q0.w; w[3] = q1.x; w[4] = q1.y; break;
          case 2:  w[0] = q0.z; w[1] = q0.w; w[2] = q1.x; w[3] = q1.y; w[4] = q1.z; break;
          default: w[0] = q0.w; w[1] = q1.x; w[2] = q1.y; w[3] = q1.z; w[4] = q1.w; break;
        }
        splice_u4 q;
        q.x = __builtin_amdgcn_alignbyte(w[1], w[0], r & 3u);
        q.y = __builtin_amdgcn_alignbyte(w[2], w[1], r & 3u);
        q.z = __builtin_amdgcn_alignbyte(w[3], w[2], r & 3u);
        q.w = __builtin_amdgcn_alignbyte(w[4], w[3], r & 3u);
        *(splice_u4*)(dst + o) = q;
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
          const int64_t i = o0 + (int64_t)k;
          if (i >= 0 && (uint64_t)i < bytes) { dst[i] = src[i]; }
        }
      }
    }
  }
}
