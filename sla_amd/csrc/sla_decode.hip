// sla_decode.hip -- gfx950 (MI355X / CDNA4) kernels of the SLA decode path.
//
// The decoder is the encoder's mirror: every stage is a recurrence in time (the entropy decoder's adaptive
// parameters, the sign-log LMS, the long-term synthesis, the IIR lattice, the de-emphasis), so parallelism
// exists only ACROSS blocks and channels -- and, inside one (block, channel), across the taps / lattice
// stages, which is what the lanes of a wave are used for.  All arithmetic is int32 / uint64 and wraps
// exactly like the reference's C.
//
// Kernel                 replaces (reference file:line)
//   k_dec_crc            src/SLAUtility.c:321-339 (CRC16 of each block), check at src/SLADecoder.c:343-352
//   k_dec_bits           src/SLADecoder.c:355-412 (block header fields), :440-481 (silent / raw / compressed body),
//                        src/SLACoder.c:84-118 (Golomb), :140-163 (gamma), :272-318 (recursive Rice), :469-506
//                        (SLACoder_GetDataArray), :406-427 (initial parameters)
//   k_dec_lms            src/SLAPredictor.c:1334-1463 (SLALMSFilter_SynthesizeInt32)
//   k_dec_ltm            src/SLAPredictor.c:1034-1119 (SLALongTermSynthesizer_SynthesizeInt32)
//   k_dec_ltm_far        the same for blocks that do not fit LDS (up to the format's 65535 samples)
//   k_dec_lattice        src/SLAPredictor.c:610-740 (SLALPCSynthesizer_SynthesizeByParcorCoefInt32),
//                        :1768-1791 (SLAEmphasisFilter_DeEmphasisInt32)
//   k_dec_finish         src/SLAUtility.c:415-433 (mid/side -> left/right), src/SLADecoder.c:540-547 (left-justify)
//   k_dec_finish_batch   the same for every file of a batch pass, packed [file][ch][n] for one copy home
//   k_dec_emit_batch     the same, converted and stored to every file's own device destination
//   k_dec_walk           src/SLADecoder.c:696-722 (the block chain of whole files whose bytes are in device memory)
//   k_dec_walk_window    the same chain, for the blocks a window of samples overlaps (no counterpart in the reference)
//   k_wide_*             kernels/walk_wide.inc: the block table of one long file, found and ranked by the whole device
//   k_salvage_* / k_dec_conceal   kernels/salvage.inc: the decodable blocks of a damaged stream; silence in the planes
//   k_dec_gather         the staging copies of a batch pass, for files that are in device memory already
//   k_verify_blocks      (kernels/verify.inc) k_dec_finish fused with a compare against source planes, per block table
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sla_hip.h"
#include "sla_crc_dev.h"

namespace {

inline int hip_rc(hipError_t e) { return (e == hipSuccess) ? 0 : -(int)e; }

__device__ __forceinline__ int32_t unfold_i32(uint32_t u) { return (int32_t)(u >> 1) ^ -(int32_t)(u & 1u); }   // src/SLAUtility.h:39
__device__ __forceinline__ uint32_t ceil_log2_u32(uint32_t x) { return (x > 1) ? (32u - (uint32_t)__builtin_clz(x - 1u)) : 0u; }
// log2 of the Rice modulus of an adaptive parameter: 2^ceil(log2(round(p/2))), at least 1   src/SLACoder.c:30-31
__device__ __forceinline__ uint32_t rice_k(uint64_t p)
{
  uint32_t v = (uint32_t)(((p >> 1) + 128u) >> 8);
  v = v ? v : 1u;
  return ceil_log2_u32(v);
}
// 119/128 old + 9/128 code, the code term in 32-bit wrapping arithmetic                      src/SLACoder.c:26-28
__device__ __forceinline__ uint64_t rice_adapt(uint64_t p, uint32_t code)
{
  return (119u * p + (uint64_t)(uint32_t)(9u * (uint32_t)(code << 8)) + 64u) >> 7;
}
__device__ __forceinline__ uint32_t umax_wave(uint32_t v)
{
  for (int off = 32; off > 0; off >>= 1) { uint32_t o = __shfl_xor(v, off); v = (o > v) ? o : v; }
  return v;
}

// ---------------------------------------------------------------------------------------------
// MSB-first bit reader over the stream image (the file's bytes, viewed as 32-bit words).  Stateless apart
// from a bit position: a read is "the 32 bits at the position", assembled from two neighbouring words of
// the lane's row of an LDS window (one ds_read2 + a funnel shift), which the wave refills cooperatively
// (coalesced 256-byte loads, byte-swapped once) at every tile boundary.  No 64-bit shift register, no refill
// branches on the serial decode chain.  Words beyond the window (a tile that costs more than 64 bits per
// sample on average) come straight from memory.  Bytes past the end of the stream read as zero; a run of
// zeros that goes on past the end (only corrupt input does that) kills the reader: every later read returns 0.
// ---------------------------------------------------------------------------------------------
struct bit_reader {
  const uint32_t* img;
  const uint32_t* win;   // this lane's window row in LDS: words [base, base + win_words) of the image, MSB-first
  uint64_t words;        // words of the image that exist
  uint64_t base;         // word index of the window start
  uint64_t limit;        // give up beyond this absolute bit position
  uint32_t rp;           // bit offset of the first unread bit from the window start
  uint32_t win_words;
  bool dead;

  __device__ __forceinline__ uint64_t pos() const { return base * 32 + rp; }
  __device__ __forceinline__ uint32_t far_word(uint32_t idx) const
  {
    const uint64_t i = base + idx;
    return (i < words) ? __builtin_bswap32(img[i]) : 0u;
  }
  // the 32 bits at the read position
  __device__ __forceinline__ uint32_t peek() const
  {
    const uint32_t idx = rp >> 5, sh = rp & 31;
    uint32_t hi, lo;
    if (idx + 1 < win_words) { hi = win[idx]; lo = win[idx + 1]; }
    else { hi = far_word(idx); lo = far_word(idx + 1); }
    return sh ? ((hi << sh) | (lo >> (32 - sh))) : hi;
  }
  __device__ __forceinline__ void open(const uint32_t* image, uint64_t image_bytes, uint64_t byte_off, const uint32_t* window)
  {
    img = image; win = window; words = (image_bytes + 3) >> 2; limit = image_bytes * 8 + 64; dead = false;
    base = byte_off >> 2; rp = 8u * (uint32_t)(byte_off & 3); win_words = 0;
  }
  // n = 0..32 bits as an unsigned number
  __device__ __forceinline__ uint32_t get(uint32_t n)
  {
    if (n == 0 || dead) { return 0; }
    const uint32_t v = peek() >> (32 - n);
    rp += n;
    return v;
  }
  // any width: the low 32 bits of the number (reference reads up to 64 bits and the callers truncate); the bits above
  // them come first and are skipped
  __device__ __forceinline__ uint32_t get_wide(uint32_t n)
  {
    while (n > 32) {
      const uint32_t skip = (n - 32 < 32) ? (n - 32) : 32u;
      (void)get(skip);
      n -= skip;
    }
    return get(n);
  }
  // zeros before the next 1 bit; the 1 is consumed
  __device__ __forceinline__ uint32_t zero_run()
  {
    uint32_t run = 0;
    if (dead) { return 0; }
    for (;;) {
      const uint32_t v = peek();
      if (v != 0) {
        const uint32_t z = (uint32_t)__clz((int)v);
        rp += z + 1;
        return run + z;
      }
      run += 32; rp += 32;
      if (pos() > limit) { dead = true; return run; }
    }
  }
  __device__ __forceinline__ void align() { rp = (rp + 7u) & ~7u; }
};

// the wave moves every owner lane's window to its read position and loads the words from there on
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, uint32_t src)
{
  return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src) << 32) | (uint32_t)__shfl((int)(uint32_t)v, (int)src);
}
// BOUNDED: every lane's reader has an end of its own (blocks of several files in one image), so the words of an
// owner's window are bounded by that owner's end, not by the loading lane's
template <bool BOUNDED = false>
__device__ __forceinline__ void fill_windows(bit_reader& rd, uint32_t* s_win, uint32_t row_words, uint32_t win_words,
                                             uint32_t owners, uint32_t lane)
{
  __syncthreads();
  rd.base += rd.rp >> 5; rd.rp &= 31;
  for (uint32_t o = 0; o < owners; o++) {
    const uint64_t base = shfl_u64(rd.base, o);
    const uint64_t words = BOUNDED ? shfl_u64(rd.words, o) : rd.words;
    for (uint32_t k = lane; k < win_words; k += 64) {
      const uint64_t i = base + k;
      s_win[o * row_words + k] = (i < words) ? __builtin_bswap32(rd.img[i]) : 0u;
    }
  }
  rd.win_words = (lane < owners) ? win_words : 0u;
  __syncthreads();
}

__device__ __forceinline__ uint32_t gamma_get(bit_reader& rd)                  // src/SLACoder.c:140-163
{
  const uint32_t nd = rd.zero_run() + 1;
  if (nd == 1) { return 0; }
  const uint32_t top = (nd - 1 < 32) ? (1u << (nd - 1)) : 0u;
  return top + rd.get_wide(nd - 1) - 1u;
}

// ---------------------------------------------------------------------------------------------
// k_dec_crc: one wave per block, slice-parallel CRC16-IBM over [8, byte_len) (sla_crc_dev.h).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_dec_crc(const uint8_t* __restrict__ bytes, const sla_hip_dec_block* __restrict__ blocks, uint32_t num_blocks,
               sla_hip_dec_info* __restrict__ info)
{
  __shared__ uint16_t table[256];
  crc16_build_table(table);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= num_blocks) { return; }
  const sla_hip_dec_block b = blocks[j];
  const uint32_t crc = crc16_wave(bytes, b.byte_off + 8, b.byte_off + b.byte_len, table, lane);
  if (lane == 0) { info[j].crc = crc; }
}

// ---------------------------------------------------------------------------------------------
// k_dec_bits: one lane per block.  Parses the block header (per channel: shift, PARCOR codes, long-term
// flag / pitch / taps, initial Rice parameter) and then the body, whose codewords are interleaved
// (sample-major, channel-minor) and whose two Rice parameters per channel adapt with every sample: a
// strictly serial walk, parallel only across blocks.  `lanes` < 64 spreads the blocks over more waves
// (fewer lanes per wave = less divergence, more SIMDs and memory pipes in use); lanes * channels <= 64.
// Output: folded-back residuals (or raw samples / zeros) in the channel planes, right-justified.
// ---------------------------------------------------------------------------------------------
struct dec_bits_args {
  const uint32_t* image; uint64_t image_bytes;
  const uint64_t* block_end;   // BOUNDED: byte end of each block's file in the image (its reader's end of stream)
  const sla_hip_dec_block* blocks; uint32_t num_blocks;
  uint32_t bps, lshift, mid_side, order, ntaps, lanes;
  int32_t* planes; uint64_t stride;
  sla_hip_dec_info* info; sla_hip_dec_chan* chan; int32_t* kint;
};

#define DEC_TILE 64          // samples per channel a lane decodes between two flushes
#define DEC_ROW  (DEC_TILE + 1)
#define DEC_WIN  128         // words of stream per channel a lane finds in LDS per tile (64 bits per sample)

template <int C, bool BOUNDED>
__global__ __launch_bounds__(64)
void k_dec_bits(const dec_bits_args a)
{
  // [lanes * C] rows of DEC_TILE samples, one word of padding per row: a lane writes its rows sample by sample
  // (all lanes at the same column -> different banks), the flush reads them row-wise and stores 256 B at a time.
  // Direct 4-byte stores from the decode loop would sit in the same counter as the reader's prefetch and make
  // every refill wait for them.
  extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
  constexpr uint32_t WIN = DEC_WIN * C, WROW = WIN + 1;      // one word of padding: the lanes' rows start in different banks
  int32_t* s_tile = (int32_t*)s_dyn;                         // [lanes * C][DEC_ROW]
  uint32_t* s_win = s_dyn + a.lanes * C * DEC_ROW;           // [lanes][WROW]
  const uint32_t lane = threadIdx.x;
  const uint32_t j = blockIdx.x * a.lanes + lane;
  const bool mine = (lane < a.lanes) && (j < a.num_blocks);
  sla_hip_dec_block b;
  b.byte_off = 0; b.byte_len = 0; b.smp_off = 0; b.num_samples = 0; b.flags = 0;
  if (mine) { b = a.blocks[j]; }
  // the end of this block's stream: bytes past it read as zero and the give-up limit counts from it, exactly as
  // for the file decoded on its own
  const uint64_t end = (BOUNDED && mine) ? a.block_end[j] : a.image_bytes;
  bit_reader rd;
  rd.open(a.image, end, b.byte_off, s_win + (mine ? lane : 0u) * WROW);
  fill_windows<BOUNDED>(rd, s_win, WROW, WIN, a.lanes, lane);       // helper lanes have no row of their own: they only carry words
  (void)rd.get(16);                                        // sync code          src/SLADecoder.c:330-334
  (void)rd.get(32);                                        // size field         (the host walked these)
  (void)rd.get(16);                                        // CRC16
  (void)rd.get(16);                                        // samples per channel
  const uint32_t type = mine ? rd.get(2) : 1u;
  uint32_t init[C];
#pragma unroll
  for (uint32_t c = 0; c < (uint32_t)C; c++) { init[c] = 0; }
  if (mine && type == 0) {
#pragma unroll
    for (uint32_t c = 0; c < (uint32_t)C; c++) {
      const uint32_t rsh = rd.get(4);
      int32_t* kout = a.kint + ((uint64_t)j * C + c) * (a.order + 1);
      kout[0] = 0;
      for (uint32_t ord = 1; ord <= a.order; ord++) {
        const uint32_t q = (ord < 4) ? 16u : 8u;           // SLA_GET_PARCOR_QUANTIZE_BIT_WIDTH
        const int32_t code = unfold_i32(rd.get(q));
        kout[ord] = (int32_t)((uint32_t)code << (16u - q)) >> rsh;
      }
      sla_hip_dec_chan ci;
      ci.pitch = 0;
      for (int k = 0; k < 5; k++) { ci.ltm_coef[k] = 0; }
      if (rd.get(1) != 0) {
        ci.pitch = rd.get(10);                             // SLALONGTERM_PERIOD_NUM_BITS
        for (uint32_t k = 0; k < a.ntaps; k++) {
          const int32_t q16 = unfold_i32(rd.get(16));
          if (k < 5) { ci.ltm_coef[k] = (int32_t)((uint32_t)q16 << 16); }
        }
      }
      init[c] = rd.get_wide(a.bps);
      ci.rice_init = init[c];
      ci.reserved = 0;
      a.chan[(uint64_t)j * C + c] = ci;
    }
  }
  rd.align();

  const uint32_t n = (!mine || (b.flags & SLA_HIP_DEC_HEADER_ONLY)) ? 0u : b.num_samples;
  uint64_t p0[C], p1[C];
  uint32_t gm[C];
  uint64_t avg = 0;
#pragma unroll
  for (uint32_t c = 0; c < (uint32_t)C; c++) {
    p0[c] = p1[c] = (uint64_t)(uint32_t)(init[c] << 8);                        // SLACODER_PARAMETER_SET
    uint32_t g = (uint32_t)((p0[c] + 128u) >> 8);
    gm[c] = g ? g : 1u;
    avg += gm[c];
  }
  avg /= (uint32_t)C;
  const bool adaptive = (avg > 8);                                               // SLACODER_LOW_THRESHOULD_PARAMETER
  int32_t* row = s_tile + lane * C * DEC_ROW;
  const uint32_t nmax = umax_wave(n);

  for (uint32_t s0 = 0; s0 < nmax; s0 += DEC_TILE) {
    const uint32_t cnt = (s0 < n) ? ((n - s0 < DEC_TILE) ? (n - s0) : (uint32_t)DEC_TILE) : 0u;
    fill_windows<BOUNDED>(rd, s_win, WROW, WIN, a.lanes, lane);
    if (type == 1) {
      for (uint32_t u = 0; u < cnt; u++) {
#pragma unroll
        for (uint32_t c = 0; c < (uint32_t)C; c++) { row[c * DEC_ROW + u] = 0; }
      }
    } else if (type == 2) {
      for (uint32_t u = 0; u < cnt; u++) {
#pragma unroll
        for (uint32_t c = 0; c < (uint32_t)C; c++) {
          const uint32_t nb = a.bps - a.lshift + ((c == 1 && a.mid_side) ? 1u : 0u);
          row[c * DEC_ROW + u] = unfold_i32(rd.get_wide(nb));
        }
      }
    } else if (type == 0 && adaptive) {
      for (uint32_t u = 0; u < cnt; u++) {
#pragma unroll
        for (uint32_t c = 0; c < (uint32_t)C; c++) {
          const uint32_t k0 = rice_k(p0[c]), k1 = rice_k(p1[c]);
          const uint32_t m0 = 1u << k0;
          const uint32_t v = rd.peek();
          uint32_t q = (uint32_t)__clz((int)v);                      // 32 when v == 0
          const uint32_t k = q ? k1 : k0;
          uint32_t val;
          if (q < 16u && q + 1u + k <= 32u && !rd.dead) {
            // the whole codeword (unary part, stop bit, k remainder bits) lies inside the 32 bits just read
            const uint32_t rest = k ? ((v << (q + 1u)) >> (32u - k)) : 0u;
            rd.rp += q + 1u + k;
            val = q ? (m0 + ((q - 1u) << k1) + rest) : rest;
          } else {
            q = rd.zero_run();
            if (q == 0) { val = rd.get(k0); }
            else {
              if (q == 16) { q += gamma_get(rd); }
              val = m0 + ((q - 1u) << k1) + rd.get(k1);
            }
          }
          p0[c] = rice_adapt(p0[c], val);
          if (q != 0) { p1[c] = rice_adapt(p1[c], val - m0); }
          row[c * DEC_ROW + u] = unfold_i32(val);
        }
      }
    } else if (type == 0) {
      for (uint32_t u = 0; u < cnt; u++) {
#pragma unroll
        for (uint32_t c = 0; c < (uint32_t)C; c++) {
          const uint32_t m = gm[c];
          const uint32_t q = rd.zero_run();
          uint32_t val;
          if ((m & (m - 1u)) == 0) {
            val = q * m + rd.get(ceil_log2_u32(m));
          } else {
            const uint32_t bb = ceil_log2_u32(m), cut = (1u << bb) - m;
            uint32_t rest = rd.get(bb - 1);
            if (rest < cut) { val = q * m + rest; }
            else { rest = (rest << 1) + rd.get(1); val = q * m + rest - cut; }
          }
          row[c * DEC_ROW + u] = unfold_i32(val);
        }
      }
    }
    __syncthreads();
    // flush: row r = (owner lane, channel); the 64 lanes store its 64 samples side by side
    for (uint32_t r = 0; r < a.lanes * (uint32_t)C; r++) {
      const uint32_t owner = r / (uint32_t)C, c = r - owner * (uint32_t)C;
      const uint32_t on = (uint32_t)__shfl((int)n, (int)owner), ooff = (uint32_t)__shfl((int)b.smp_off, (int)owner);
      const uint32_t s = s0 + lane;
      if (s < on) { a.planes[(uint64_t)c * a.stride + ooff + s] = s_tile[r * DEC_ROW + lane]; }
    }
    __syncthreads();
  }
  rd.align();
  if (mine) {
    sla_hip_dec_info* io = a.info + j;
    io->type = type;
    io->used_bytes = (uint32_t)((rd.pos() >> 3) - b.byte_off);
    io->overrun = (rd.dead || (rd.pos() >> 3) > end) ? 1u : 0u;
  }
}

// ---------------------------------------------------------------------------------------------
// k_dec_lms: sign-log LMS synthesis.  Same lane layout as the encoder's k_tail: G = 2*ORDER lanes per
// (block, channel), lane t holds coefficient t and history t (t < ORDER: past OUTPUTS, else past predictions).
// The residual e is known in advance here, so its sign and step are off the serial chain; what is serial is
// coefficient -> prediction -> output -> history.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t sgn(int32_t v)
{
  int32_t r;
  asm("v_med3_i32 %0, %1, -1, 1" : "=v"(r) : "v"(v));
  return r;
}
__device__ __forceinline__ int32_t mad24(int32_t a, int32_t b, int32_t c)
{
  int32_t r;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t x)
{
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
template <int G>
__device__ __forceinline__ uint32_t group_sum(uint32_t x)
{
  x += dpp_u32<0xB1>(x);                       // quad_perm [1,0,3,2]
  x += dpp_u32<0x4E>(x);                       // quad_perm [2,3,0,1]
  x += dpp_u32<0x141>(x);                      // row_half_mirror
  if (G >= 16) { x += dpp_u32<0x140>(x); }     // row_mirror
  if (G >= 32) { x += (uint32_t)__shfl_xor((int)x, 16); }
  if (G >= 64) { x += (uint32_t)__shfl_xor((int)x, 32); }
  return x;
}

template <int ORDER, bool FIRST>
__device__ __forceinline__ int32_t lms_synth_block(int32_t e_mine, uint32_t grp_base, bool is_fir_head, bool is_iir_head,
                                                   uint32_t t, int32_t& coef, int32_t& h)
{
  constexpr int G = 2 * ORDER;
  int32_t v_mine = 0;
  int32_t es[G];
#pragma unroll
  for (int u = 0; u < G; u++) { es[u] = __shfl(e_mine, (int)(grp_base + u)); }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < G; u++) {
    const int32_t e = es[u];
    int32_t v, ph;
    if (FIRST && u < ORDER) {
      v = e; ph = e;                                                           // priming   src/SLAPredictor.c:1365-1387
    } else {
      const int32_t sh = sgn(h);
      const uint32_t sum = group_sum<G>((uint32_t)coef * (uint32_t)h) + (1u << 9);
      const int32_t p = (int32_t)sum >> 10;
      v = (int32_t)((uint32_t)e + (uint32_t)p);
      const int32_t ne = (int32_t)(0u - (uint32_t)e);
      const uint32_t mag = (uint32_t)max(e, ne);
      const int32_t lg = 32 - (int32_t)__clz((int)mag);
      const int32_t sign2 = __mul24(sgn(e), sh);
      coef = mad24(sign2, lg >> 1, coef);
      ph = p;
    }
    h = (int32_t)__builtin_amdgcn_update_dpp(h, h, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
    h = is_fir_head ? v : (is_iir_head ? ph : h);
    v_mine = (t == (uint32_t)u) ? v : v_mine;
  }
  return v_mine;
}

template <int ORDER>
__global__ __launch_bounds__(256)
void k_dec_lms(int32_t* __restrict__ planes, uint64_t stride, const sla_hip_dec_block* __restrict__ blocks,
               const sla_hip_dec_info* __restrict__ info, uint32_t num_blocks, uint32_t num_channels)
{
  constexpr int G = 2 * ORDER;
  constexpr int JPW = 64 / G;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t t = lane & (G - 1);
  const uint32_t grp_base = lane - t;
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t j = wave * JPW + (lane / G);
  const uint32_t num_jobs = num_blocks * num_channels;
  const bool have = (j < num_jobs);
  const uint32_t bi = have ? j / num_channels : 0, ch = have ? j - bi * num_channels : 0;
  const sla_hip_dec_block b = blocks[bi];
  const bool active = have && info[bi].type == 0 && !(b.flags & SLA_HIP_DEC_HEADER_ONLY);
  uint32_t n = active ? b.num_samples : 0;
  if (n < (uint32_t)ORDER) { n = 0; }                    // fewer samples than taps: everything passes through
  int32_t* io = planes + (uint64_t)ch * stride + b.smp_off;
  const bool is_fir_head = (t == 0), is_iir_head = (t == (uint32_t)ORDER);
  const uint32_t nmax = umax_wave(n);

  int32_t coef = 0, h = 0;
  int32_t e_next = (t < n) ? io[t] : 0;
  for (uint32_t s0 = 0; s0 < nmax; s0 += G) {
    const int32_t e_mine = e_next;
    const uint32_t sn = s0 + G + t;
    e_next = (sn < n) ? io[sn] : 0;
    const int32_t v = (s0 == 0) ? lms_synth_block<ORDER, true>(e_mine, grp_base, is_fir_head, is_iir_head, t, coef, h)
                                : lms_synth_block<ORDER, false>(e_mine, grp_base, is_fir_head, is_iir_head, t, coef, h);
    const uint32_t s = s0 + t;
    if (s < n) { io[s] = v; }
  }
}

// ---------------------------------------------------------------------------------------------
// k_dec_ltm: long-term synthesis, out[s] = in[s] + ((2^30 + sum_j coef[j] * out[s - delay + j]) >> 31) for
// s >= delay = pitch + taps/2.  The nearest tap lies d = pitch - (taps-1)/2 samples back, so d consecutive
// outputs are independent: one wave per (block, channel) walks the block (held in LDS) in steps of
// min(d, 64) samples.  d <= 0 never comes out of the encoder (pitch >= 3); such a stream is walked one
// sample at a time, taps that point at or past the current sample reading not-yet-synthesised input.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64)
void k_dec_ltm(int32_t* __restrict__ planes, uint64_t stride, const sla_hip_dec_block* __restrict__ blocks,
               const sla_hip_dec_info* __restrict__ info, const sla_hip_dec_chan* __restrict__ chan,
               uint32_t num_channels, uint32_t ntaps)
{
  extern __shared__ __attribute__((aligned(16))) int32_t s_blk[];
  const uint32_t j = blockIdx.x;
  const uint32_t bi = j / num_channels, ch = j - bi * num_channels;
  const sla_hip_dec_block b = blocks[bi];
  if (info[bi].type != 0 || (b.flags & SLA_HIP_DEC_HEADER_ONLY)) { return; }
  const sla_hip_dec_chan ci = chan[j];
  const uint32_t n = b.num_samples;
  const uint32_t delay = ci.pitch + (ntaps >> 1);
  if (ci.pitch == 0 || delay >= n) { return; }
  int32_t* io = planes + (uint64_t)ch * stride + b.smp_off;
  const uint32_t lane = threadIdx.x;
  for (uint32_t s = lane; s < n; s += 64) { s_blk[s] = io[s]; }
  __syncthreads();
  const int32_t d = (int32_t)ci.pitch - (int32_t)((ntaps - 1) >> 1);
  const uint32_t step = (d < 1) ? 1u : ((d > 64) ? 64u : (uint32_t)d);
  for (uint32_t s0 = delay; s0 < n; s0 += step) {
    const uint32_t s = s0 + lane;
    if (lane < step && s < n) {
      int64_t acc = (int64_t)1 << 30;
      for (uint32_t k = 0; k < ntaps; k++) {
        const uint32_t at = s - delay + k;
        acc += (int64_t)ci.ltm_coef[k] * (int64_t)((at < n) ? s_blk[at] : 0);
      }
      s_blk[s] = (int32_t)((uint32_t)s_blk[s] + (uint32_t)(int32_t)(acc >> 31));
    }
    __syncthreads();                                       // one wave: orders the LDS writes before the next step's reads
  }
  for (uint32_t s = delay + lane; s < n; s += 64) { io[s] = s_blk[s]; }
}

// ---------------------------------------------------------------------------------------------
// k_dec_ltm_far: the same synthesis for blocks that do not fit LDS.  The block passes through a ring of
// DEC_LTM_RING samples in chunks of DEC_LTM_CHUNK: sample s lives in slot s & (DEC_LTM_RING - 1).  While the chunk
// [c0, c1) is synthesised the ring holds the outputs back to c0 - DEC_LTM_HIST (delay = pitch + taps/2 <= 1023 + 2)
// and the raw input up to c1 + DEC_LTM_LOOK (a tap reaches at most s + 1: 5 taps at pitch 1), a span of at most
// HIST + CHUNK + LOOK <= RING samples, so no two live samples share a slot.  The steps inside a chunk are k_dec_ltm's:
// min(d, 64) independent outputs each, one sample per step for d < 1, whose taps at s and s + 1 find the ring's slots
// still holding input.  A step is cut at the chunk's end, which changes no value: every output is defined by the
// recurrence alone.
// Bounds: every LDS index is masked to the ring, so no num_samples, pitch or tap taken from the stream can leave it
// (the ring's size is fixed at compile time and does not depend on n or the handle).  Global memory is touched at
// io[s] with s < n for loads and delay <= s < n for stores only: the loops' own conditions, with `need`, c1 <= n.
// A tap position at >= n is never read (it counts as 0), at < 0 cannot occur (s >= delay).
// ---------------------------------------------------------------------------------------------
#define DEC_LTM_CHUNK 2048u
#define DEC_LTM_RING  4096u
#define DEC_LTM_HIST  1025u              // 10-bit pitch + taps / 2
#define DEC_LTM_LOOK  2u
static_assert((DEC_LTM_RING & (DEC_LTM_RING - 1u)) == 0 && DEC_LTM_HIST + DEC_LTM_CHUNK + DEC_LTM_LOOK <= DEC_LTM_RING,
              "live span of k_dec_ltm_far must fit its ring");

__global__ __launch_bounds__(64)
void k_dec_ltm_far(int32_t* __restrict__ planes, uint64_t stride, const sla_hip_dec_block* __restrict__ blocks,
                   const sla_hip_dec_info* __restrict__ info, const sla_hip_dec_chan* __restrict__ chan,
                   uint32_t num_channels, uint32_t ntaps)
{
  __shared__ __attribute__((aligned(16))) int32_t s_ring[DEC_LTM_RING];
  constexpr uint32_t M = DEC_LTM_RING - 1u;
  const uint32_t j = blockIdx.x;
  const uint32_t bi = j / num_channels, ch = j - bi * num_channels;
  const sla_hip_dec_block b = blocks[bi];
  if (info[bi].type != 0 || (b.flags & SLA_HIP_DEC_HEADER_ONLY)) { return; }
  const sla_hip_dec_chan ci = chan[j];
  const uint32_t n = b.num_samples;
  const uint32_t delay = ci.pitch + (ntaps >> 1);
  if (ci.pitch == 0 || delay >= n || delay > DEC_LTM_HIST) { return; }       // (a pitch is a 10-bit field: the last never holds)
  int32_t* io = planes + (uint64_t)ch * stride + b.smp_off;
  const uint32_t lane = threadIdx.x;
  const int32_t d = (int32_t)ci.pitch - (int32_t)((ntaps - 1) >> 1);
  const uint32_t step = (d < 1) ? 1u : ((d > 64) ? 64u : (uint32_t)d);
  uint32_t loaded = 0;                                       // [0, loaded) has been brought into the ring
  for (uint32_t c0 = 0; c0 < n; c0 += DEC_LTM_CHUNK) {
    const uint32_t c1 = (n - c0 > DEC_LTM_CHUNK) ? c0 + DEC_LTM_CHUNK : n;
    const uint32_t need = (n - c1 > DEC_LTM_LOOK) ? c1 + DEC_LTM_LOOK : n;
    for (uint32_t s = loaded + lane; s < need; s += 64) { s_ring[s & M] = io[s]; }
    loaded = need;
    __syncthreads();
    const uint32_t first = (c0 > delay) ? c0 : delay;
    for (uint32_t s0 = first; s0 < c1; s0 += step) {
      const uint32_t s = s0 + lane;
      if (lane < step && s < c1) {
        int64_t acc = (int64_t)1 << 30;
        for (uint32_t k = 0; k < ntaps; k++) {
          const uint32_t at = s - delay + k;
          acc += (int64_t)ci.ltm_coef[k] * (int64_t)((at < n) ? s_ring[at & M] : 0);
        }
        s_ring[s & M] = (int32_t)((uint32_t)s_ring[s & M] + (uint32_t)(int32_t)(acc >> 31));
      }
      __syncthreads();                                       // one wave: orders the LDS writes before the next step's reads
    }
    for (uint32_t s = first + lane; s < c1; s += 64) { io[s] = s_ring[s & M]; }
    __syncthreads();                                         // the next chunk's look-ahead lands in the slots of c0 and c0 + 1, read just above
  }
}

// ---------------------------------------------------------------------------------------------
// k_dec_lattice: PARCOR synthesis lattice + de-emphasis.  Per sample the reference walks the stages
// m = order..1:  f_{m-1} = f_m + R(k_m b_{m-1}[n-1]),  b_m[n] = b_{m-1}[n-1] - R(k_m f_{m-1}),  R(v) = (v + 2^14) >> 15.
// Every R(k_m b_{m-1}[n-1]) depends on the PREVIOUS sample only, so the lanes form them at once and the chain
// f_order -> f_0 becomes a prefix sum (wrapping adds are associative): position q = lane*R + r holds stage
// m = G*R - q, i.e. the first stage of the walk sits at the lowest position and the output f_0 appears on the
// last lane, which also carries the one-tap de-emphasis recurrence and stores the sample.  The new b values
// move one position up (b_m feeds stage m+1), the last position takes b_0 = f_0.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t lat_term(int32_t k, int32_t v) { return (int32_t)((uint32_t)k * (uint32_t)v + (1u << 14)) >> 15; }

template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_rows(uint32_t x)        // 0 where the source lane does not exist / row masked off
{
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xF, false);
}

template <int G>
__device__ __forceinline__ uint32_t group_prefix(uint32_t x)    // inclusive prefix sum over the G lanes of a group
{
  x += dpp_u32<0x111>(x);                      // row_shr:1
  x += dpp_u32<0x112>(x);                      // row_shr:2
  x += dpp_u32<0x114>(x);                      // row_shr:4
  x += dpp_u32<0x118>(x);                      // row_shr:8
  if (G >= 32) { x += dpp_rows<0x142, 0xA>(x); }   // row_bcast:15 into rows 1 and 3
  if (G >= 64) { x += dpp_rows<0x143, 0xC>(x); }   // row_bcast:31 into rows 2 and 3
  return x;
}

template <int G, int R>
__global__ __launch_bounds__(256)
void k_dec_lattice(int32_t* __restrict__ planes, uint64_t stride, const sla_hip_dec_block* __restrict__ blocks,
                   const sla_hip_dec_info* __restrict__ info, uint32_t num_blocks, uint32_t num_channels,
                   const int32_t* __restrict__ kint, uint32_t order, uint32_t deemphasis)
{
  constexpr int JPW = 64 / G;
  // the output lane parks its 16 samples here; the group then stores them side by side (a 4-byte store per
  // sample would share a counter with the prefetch of the next inputs and stall it)
  __shared__ int32_t s_out[(256 / G) * 16];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t t = lane & (G - 1);
  const uint32_t grp_base = lane - t;
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t j = wave * JPW + (lane / G);
  const uint32_t num_jobs = num_blocks * num_channels;
  const bool have = (j < num_jobs);
  const uint32_t bi = have ? j / num_channels : 0, ch = have ? j - bi * num_channels : 0;
  const sla_hip_dec_block b = blocks[bi];
  const bool active = have && info[bi].type == 0 && !(b.flags & SLA_HIP_DEC_HEADER_ONLY);
  const uint32_t n = active ? b.num_samples : 0;
  int32_t* io = planes + (uint64_t)ch * stride + b.smp_off;
  int32_t* park = s_out + (threadIdx.x / G) * 16;
  const bool is_last = (t == (uint32_t)(G - 1));
  const uint32_t nmax = umax_wave(n);

  int32_t k[R], bw[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t m = (uint32_t)(G * R) - (t * R + r);
    k[r] = (active && m <= order) ? kint[(uint64_t)j * (order + 1) + m] : 0;
    bw[r] = 0;
  }
  int32_t yprev = 0;
  int32_t e_next = (t < n) ? io[t] : 0;
  for (uint32_t s0 = 0; s0 < nmax; s0 += G) {
    const int32_t e_mine = e_next;
    const uint32_t sn = s0 + G + t;
    e_next = (sn < n) ? io[sn] : 0;
#pragma unroll 1
    for (int u0 = 0; u0 < G; u0 += 16) {
      int32_t es[16];
#pragma unroll
      for (int u = 0; u < 16; u++) { es[u] = __shfl(e_mine, (int)(grp_base + u0 + u)); }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 16; u++) {
        uint32_t c[R];
        uint32_t run = 0;
#pragma unroll
        for (int r = 0; r < R; r++) { run += (uint32_t)lat_term(k[r], bw[r]); c[r] = run; }
        const uint32_t excl = group_prefix<G>(run) - run + (uint32_t)es[u];
        int32_t f[R], nb[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
          f[r] = (int32_t)(excl + c[r]);
          nb[r] = (int32_t)((uint32_t)bw[r] - (uint32_t)lat_term(k[r], f[r]));
        }
        // b moves one position up; the group's last position takes the output
        int32_t from_next = (int32_t)__builtin_amdgcn_update_dpp(f[R - 1], nb[0], 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
        from_next = is_last ? f[R - 1] : from_next;
#pragma unroll
        for (int r = 0; r < R - 1; r++) { bw[r] = nb[r + 1]; }
        bw[R - 1] = from_next;
        // de-emphasis on the output lane: y[n] = x[n] + ((y[n-1] * 31) >> 5)     src/SLAPredictor.c:1781-1786
        const int32_t y = deemphasis ? (int32_t)((uint32_t)f[R - 1] + (uint32_t)((int32_t)((uint32_t)yprev * 31u) >> 5)) : f[R - 1];
        yprev = y;
        if (is_last) { park[u] = y; }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      {
        const uint32_t s = s0 + (uint32_t)u0 + (t & 15u);
        if (t < 16u && s < n) { io[s] = park[t & 15u]; }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_dec_finish: mid/side -> left/right and the final left-justification, elementwise over all samples.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_dec_finish(int32_t* __restrict__ planes, uint64_t stride, uint32_t num_channels, uint32_t num_samples,
                  uint32_t mid_side, uint32_t shift)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_samples) { return; }
  if (mid_side) {
    const int32_t side = planes[stride + i];
    const int32_t mid = (int32_t)(((uint32_t)planes[i] << 1) | ((uint32_t)side & 1u));
    const int32_t l = (int32_t)((uint32_t)mid + (uint32_t)side) >> 1, r = (int32_t)((uint32_t)mid - (uint32_t)side) >> 1;
    planes[i] = (int32_t)((uint32_t)l << shift);
    planes[stride + i] = (int32_t)((uint32_t)r << shift);
    for (uint32_t c = 2; c < num_channels; c++) { planes[(uint64_t)c * stride + i] = (int32_t)((uint32_t)planes[(uint64_t)c * stride + i] << shift); }
  } else {
    for (uint32_t c = 0; c < num_channels; c++) { planes[(uint64_t)c * stride + i] = (int32_t)((uint32_t)planes[(uint64_t)c * stride + i] << shift); }
  }
}

// k_dec_finish_batch: k_dec_finish for every file of a batch pass, out of place: the finished samples of file f go
// to out[files[f].out_off + c * n + i] (packed [file][ch][n], so that the pass comes home in one copy).  blockIdx.y
// walks the files, the x dimension their samples: loads and stores of consecutive lanes are consecutive words.
__global__ __launch_bounds__(256)
void k_dec_finish_batch(const int32_t* __restrict__ planes, uint64_t stride, uint32_t num_channels,
                        const sla_hip_dec_file* __restrict__ files, uint32_t num_files, int32_t* __restrict__ out)
{
  for (uint32_t f = blockIdx.y; f < num_files; f += gridDim.y) {
    const sla_hip_dec_file fi = files[f];
    const int32_t* src = planes + fi.plane_off;
    int32_t* dst = out + fi.out_off;
    const uint32_t n = fi.num_samples, shift = fi.shift;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      uint32_t c = 0;
      if (fi.mid_side && num_channels == 2) {
        const int32_t side = src[stride + i];
        const int32_t mid = (int32_t)(((uint32_t)src[i] << 1) | ((uint32_t)side & 1u));
        const int32_t l = (int32_t)((uint32_t)mid + (uint32_t)side) >> 1, r = (int32_t)((uint32_t)mid - (uint32_t)side) >> 1;
        dst[i] = (int32_t)((uint32_t)l << shift);
        dst[(uint64_t)n + i] = (int32_t)((uint32_t)r << shift);
        c = 2;
      }
      for (; c < num_channels; c++) { dst[(uint64_t)c * n + i] = (int32_t)((uint32_t)src[(uint64_t)c * stride + i] << shift); }
    }
  }
}

// k_dec_emit_batch: k_dec_finish_batch's mid/side and left-justification, then the conversion to the caller's sample
// format and the store to every file's own destination (sla_hip_decode_batch_device), with [done, fill_end) of every
// channel written zero in the same pass.  blockIdx.y walks the files, the x dimension their samples.  Three store
// shapes, chosen per file (wave-uniform): planar (sample_stride 1), a lane takes 4 consecutive samples of each channel,
// one 16-byte plane load and one 16-byte (int16: 8-byte) store; interleaved stereo (channel_stride 1, sample_stride 2),
// a lane takes one sample, its two elements in one store; any other strides one element per store.
template <uint32_t FMT> struct emit_type { typedef int32_t T; };
template <> struct emit_type<SLA_HIP_PCM_S16> { typedef int16_t T; };
template <> struct emit_type<SLA_HIP_PCM_F32> { typedef float T; };

template <uint32_t FMT>
__device__ __forceinline__ typename emit_type<FMT>::T emit_cvt(int32_t left, uint32_t bps)
{
  if constexpr (FMT == SLA_HIP_PCM_S32) { return left >> ((32u - bps) & 31u); }
  else if constexpr (FMT == SLA_HIP_PCM_S16) { return (int16_t)(left >> 16); }
  else if constexpr (FMT == SLA_HIP_PCM_F32) { return (float)left * 0x1p-31f; }     // exact scaling of the rounded int
  else { return left; }
}

// left / right of mid / side, left-justified (src/SLAUtility.c:415-433, as k_dec_finish)
__device__ __forceinline__ void emit_lr(int32_t m, int32_t side, uint32_t shift, int32_t& l, int32_t& r)
{
  const int32_t mid = (int32_t)(((uint32_t)m << 1) | ((uint32_t)side & 1u));
  l = (int32_t)((uint32_t)((int32_t)((uint32_t)mid + (uint32_t)side) >> 1) << shift);
  r = (int32_t)((uint32_t)((int32_t)((uint32_t)mid - (uint32_t)side) >> 1) << shift);
}

// 4 consecutive plane samples from g; those at or past `done` read as zero
__device__ __forceinline__ void emit_load4(const int32_t* p, uint64_t g, uint32_t done, bool vload, int32_t v[4])
{
  typedef int32_t i4 __attribute__((ext_vector_type(4)));
  if (vload && g + 4 <= done) {
    const i4 q = *(const i4*)(p + g);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = (g + k < done) ? p[g + k] : 0; }
  }
}

template <typename T>
__device__ __forceinline__ void emit_store4(T* p, uint64_t g, uint64_t lim, const T v[4])
{
  typedef T t4 __attribute__((ext_vector_type(4)));
  if (g + 4 <= lim) {
    t4 q; q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
    *(t4*)(p + g) = q;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) { if (g + k < lim) { p[g + k] = v[k]; } }
  }
}

template <uint32_t FMT>
__global__ __launch_bounds__(256)
void k_dec_emit_batch(const int32_t* __restrict__ planes, uint64_t stride, const sla_hip_dec_emit* __restrict__ files,
                      uint32_t num_files)
{
  typedef typename emit_type<FMT>::T T;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (uint64_t)gridDim.x * blockDim.x;
  for (uint32_t f = blockIdx.y; f < num_files; f += gridDim.y) {
    const sla_hip_dec_emit e = files[f];
    const int32_t* src = planes + e.plane_off;
    T* dst = (T*)e.dst;
    const uint32_t done = e.done, C = e.num_channels, shift = e.shift, bps = e.bits_per_sample;
    const uint64_t lim = (e.fill_end > done) ? e.fill_end : done, cs = e.channel_stride, ss = e.sample_stride;
    const bool ms = e.mid_side != 0 && C == 2;
    if (ss == 1 && (C == 1 || cs % 4 == 0) && ((uintptr_t)dst % (4 * sizeof(T))) == 0) {
      const bool vload = ((e.plane_off | stride) & 3u) == 0;
      for (uint64_t g = tid * 4; g < lim; g += nt * 4) {
        int32_t a[4], b[4];
        T o[4];
        if (ms) {
          emit_load4(src, g, done, vload, a);
          emit_load4(src + stride, g, done, vload, b);
#pragma unroll
          for (int k = 0; k < 4; k++) { int32_t l = 0, r = 0; if (g + k < done) { emit_lr(a[k], b[k], shift, l, r); } a[k] = l; b[k] = r; }
#pragma unroll
          for (int k = 0; k < 4; k++) { o[k] = emit_cvt<FMT>(a[k], bps); }
          emit_store4(dst, g, lim, o);
#pragma unroll
          for (int k = 0; k < 4; k++) { o[k] = emit_cvt<FMT>(b[k], bps); }
          emit_store4(dst + cs, g, lim, o);
        } else {
          for (uint32_t c = 0; c < C; c++) {
            emit_load4(src + (uint64_t)c * stride, g, done, vload, a);
#pragma unroll
            for (int k = 0; k < 4; k++) { o[k] = emit_cvt<FMT>((int32_t)((uint32_t)a[k] << shift), bps); }
            emit_store4(dst + (uint64_t)c * cs, g, lim, o);
          }
        }
      }
    } else if (C == 2 && cs == 1 && ss == 2 && ((uintptr_t)dst % (2 * sizeof(T))) == 0) {
      typedef T t2 __attribute__((ext_vector_type(2)));
      for (uint64_t i = tid; i < lim; i += nt) {
        int32_t l = 0, r = 0;
        if (i < done) {
          if (ms) { emit_lr(src[i], src[stride + i], shift, l, r); }
          else { l = (int32_t)((uint32_t)src[i] << shift); r = (int32_t)((uint32_t)src[stride + i] << shift); }
        }
        t2 q; q.x = emit_cvt<FMT>(l, bps); q.y = emit_cvt<FMT>(r, bps);
        *(t2*)(dst + 2 * i) = q;
      }
    } else {
      for (uint64_t i = tid; i < lim; i += nt) {
        if (ms && i < done) {
          int32_t l, r;
          emit_lr(src[i], src[stride + i], shift, l, r);
          dst[i * ss] = emit_cvt<FMT>(l, bps);
          dst[cs + i * ss] = emit_cvt<FMT>(r, bps);
        } else {
          for (uint32_t c = 0; c < C; c++) {
            const int32_t left = (i < done) ? (int32_t)((uint32_t)src[(uint64_t)c * stride + i] << shift) : 0;
            dst[(uint64_t)c * cs + i * ss] = emit_cvt<FMT>(left, bps);
          }
        }
      }
    }
  }
}

// De-emphasis as a pass of its own (per-call API): y[n] = x[n] + ((y[n-1] * (2^s - 1)) >> s), y[-1] = previous.
// A one-tap recurrence through a truncating shift: strictly serial, one lane.
__global__ __launch_bounds__(64)
void k_dec_deemphasis(int32_t* __restrict__ data, uint32_t n, int32_t previous, uint32_t shift)
{
  if (threadIdx.x != 0 || blockIdx.x != 0) { return; }
  const uint32_t numer = (1u << shift) - 1u;
  int32_t y = previous;
  for (uint32_t i = 0; i < n; i++) {
    y = (int32_t)((uint32_t)data[i] + (uint32_t)((int32_t)((uint32_t)y * numer) >> shift));
    data[i] = y;
  }
}

// ---------------------------------------------------------------------------------------------
// k_dec_walk: the host's walk_chain (sla_decoder.c; src/SLADecoder.c:696-722) for whole files whose bytes are in
// device memory, one file per lane: the chain is one dependent load per block, so blocks cannot go on lanes, but files
// are independent.  The checks, their order and the 32-bit arithmetic (`size field + 6` wraps) are the host's.  Ten
// byte loads per block, all inside [src + off, src + off + 11) with off + 11 <= data_size checked first: no byte
// outside the stream is read, whatever the alignment of src.  Count mode writes the per-file result only; write mode
// also the rows [first, first + max_rows) of the block table, of the block ends and of the stored CRC fields.
// A workgroup is one wave: a batch of a few hundred files spreads over as many CUs as it has waves, and a long file
// holds up only the 63 lanes next to it.
// ---------------------------------------------------------------------------------------------
#define DEC_WALK_SYNC       0xFFFFu     // SLAI_SYNC_CODE
#define DEC_WALK_MIN_HEADER 11u         // SLA_MINIMUM_BLOCK_HEADER_SIZE
#define DEC_WALK_CRC_START  8u          // SLAI_BLK_CRC_START

__global__ __launch_bounds__(64)
void k_dec_walk(const sla_hip_dec_walk_file* __restrict__ files, uint32_t num_files, uint32_t cap_n, uint32_t crc_check,
                sla_hip_dec_walk_result* __restrict__ results, sla_hip_dec_block* __restrict__ blocks,
                uint64_t* __restrict__ block_end, uint32_t* __restrict__ crc_field)
{
  const uint32_t f = blockIdx.x * 64u + threadIdx.x;
  if (f >= num_files) { return; }
  const sla_hip_dec_walk_file fi = files[f];
  const uint8_t* data = fi.src;
  const uint32_t data_size = fi.data_size, total = fi.total, rows = (blocks != nullptr) ? fi.max_rows : 0u;
  const uint64_t end = fi.img_off + data_size;
  uint32_t off = SLA_HEADER_SIZE, pos = 0, nb = 0, extent = 0, stop = SLA_APIRESULT_OK;
  while (pos < total) {
    if (off > data_size) { stop = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    const uint32_t left = data_size - off;
    if (left < DEC_WALK_MIN_HEADER) { stop = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    const uint8_t* p = data + off;
    uint32_t h[10];
#pragma unroll
    for (int k = 0; k < 10; k++) { h[k] = p[k]; }
    if (((h[0] << 8) | h[1]) != DEC_WALK_SYNC) { stop = SLA_APIRESULT_FAILED_TO_FIND_SYNC_CODE; break; }
    const uint32_t bsize = ((h[2] << 24) | (h[3] << 16) | (h[4] << 8) | h[5]) + 6u;
    const uint32_t n = (h[8] << 8) | h[9];
    if (bsize > left || bsize < DEC_WALK_CRC_START) { stop = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    uint32_t flags = 0;
    if (n > fi.capacity - pos || n > cap_n) {
      stop = SLA_APIRESULT_INSUFFICIENT_BUFFER_SIZE;
      if (crc_check != 1u) { break; }
      flags = SLA_HIP_DEC_HEADER_ONLY;
    }
    if (nb < rows) {
      sla_hip_dec_block b;
      b.byte_off = fi.img_off + off; b.byte_len = bsize; b.smp_off = fi.plane_off + pos; b.num_samples = n; b.flags = flags;
      blocks[fi.first + nb] = b;
      block_end[fi.first + nb] = end;
      crc_field[fi.first + nb] = (h[6] << 8) | h[7];
    }
    nb++;
    if (flags != 0) { break; }
    if (pos + n > extent) { extent = pos + n; }
    off += bsize; pos += n;
  }
  // rows the walk did not reach (the bytes changed since they were counted): empty, header-only, at the file's start
  for (uint32_t r = nb; r < rows; r++) {
    sla_hip_dec_block b;
    b.byte_off = fi.img_off; b.byte_len = DEC_WALK_CRC_START; b.smp_off = fi.plane_off; b.num_samples = 0; b.flags = SLA_HIP_DEC_HEADER_ONLY;
    blocks[fi.first + r] = b;
    block_end[fi.first + r] = end;
    crc_field[fi.first + r] = 0;
  }
  sla_hip_dec_walk_result res;
  res.num_blocks = nb; res.stop = stop; res.extent = extent; res.reserved = 0;
  results[f] = res;
}

// ---------------------------------------------------------------------------------------------
// k_dec_walk_window: k_dec_walk for a window of samples (sla_hip_decode_windows_resident).  The same shape -- one file
// per lane, a workgroup is one wave, ten byte loads per block inside [src + off, src + off + 11) with off + 11 <=
// data_size checked first -- and the same three chain checks in the same order and 32-bit arithmetic.  What differs:
// the walk may start at a hint, it ends at the window's end, blocks in front of the window are passed over without a
// row, and there is neither a capacity test nor a header-only row.  The sample position is carried in 64 bits: it only
// grows, so a chain (or a wrong hint) cannot bring it back below the window's end.  Every kept block has pos < win_end
// and num_samples <= cap_n, and the host sizes the plane region from the same walk in count mode.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64)
void k_dec_walk_window(const sla_hip_dec_window_file* __restrict__ files, uint32_t num_files, uint32_t cap_n,
                       sla_hip_dec_window_result* __restrict__ results, sla_hip_dec_block* __restrict__ blocks,
                       uint64_t* __restrict__ block_end, uint32_t* __restrict__ crc_field)
{
  const uint32_t f = blockIdx.x * 64u + threadIdx.x;
  if (f >= num_files) { return; }
  const sla_hip_dec_window_file fi = files[f];
  const uint8_t* data = fi.src;
  const uint32_t data_size = fi.data_size, rows = (blocks != nullptr) ? fi.max_rows : 0u;
  const uint64_t end = fi.img_off + fi.range_bytes;
  const uint64_t win_start = fi.win_start;
  uint64_t win_end = win_start + fi.win_len;
  if (win_end > fi.total) { win_end = fi.total; }
  uint32_t off = (fi.seek_byte != 0) ? fi.seek_byte : SLA_HEADER_SIZE;
  uint64_t pos = (fi.seek_byte != 0) ? fi.seek_sample : 0u;
  uint32_t nb = 0, skipped = 0, stop = SLA_APIRESULT_OK, first_byte = 0, first_sample = 0, end_byte = 0, end_sample = 0;
  while (pos < win_end) {
    if (off > data_size) { stop = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    const uint32_t left = data_size - off;
    if (left < DEC_WALK_MIN_HEADER) { stop = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    const uint8_t* p = data + off;
    uint32_t h[10];
#pragma unroll
    for (int k = 0; k < 10; k++) { h[k] = p[k]; }
    if (((h[0] << 8) | h[1]) != DEC_WALK_SYNC) { stop = SLA_APIRESULT_FAILED_TO_FIND_SYNC_CODE; break; }
    const uint32_t bsize = ((h[2] << 24) | (h[3] << 16) | (h[4] << 8) | h[5]) + 6u;
    const uint32_t n = (h[8] << 8) | h[9];
    if (bsize > left || bsize < DEC_WALK_CRC_START) { stop = SLA_APIRESULT_INSUFFICIENT_DATA_SIZE; break; }
    if (n == 0 || pos + n <= win_start) { skipped++; off += bsize; pos += n; continue; }       // in front of the window
    if (n > cap_n) { stop = SLA_APIRESULT_INSUFFICIENT_BUFFER_SIZE; break; }
    if (nb == 0) { first_byte = off; first_sample = (uint32_t)pos; }
    if (nb < rows) {
      sla_hip_dec_block b;
      b.byte_off = fi.img_off + (uint32_t)(off - fi.base_byte); b.byte_len = bsize;
      b.smp_off = fi.plane_off + (uint32_t)((uint32_t)pos - fi.base_sample); b.num_samples = n; b.flags = 0;
      blocks[fi.first + nb] = b;
      block_end[fi.first + nb] = end;
      crc_field[fi.first + nb] = (h[6] << 8) | h[7];
    }
    nb++;
    off += bsize; pos += n;
    end_byte = off; end_sample = (uint32_t)pos;
  }
  // rows the walk did not reach (the bytes changed since they were counted): empty, header-only, at the range's start
  for (uint32_t r = nb; r < rows; r++) {
    sla_hip_dec_block b;
    b.byte_off = fi.img_off; b.byte_len = DEC_WALK_CRC_START; b.smp_off = fi.plane_off; b.num_samples = 0; b.flags = SLA_HIP_DEC_HEADER_ONLY;
    blocks[fi.first + r] = b;
    block_end[fi.first + r] = end;
    crc_field[fi.first + r] = 0;
  }
  sla_hip_dec_window_result res;
  res.num_blocks = nb; res.stop = stop; res.skipped = skipped; res.first_byte = first_byte; res.first_sample = first_sample;
  res.end_byte = end_byte; res.end_sample = end_sample; res.reserved = 0;
  results[f] = res;
}

// ---------------------------------------------------------------------------------------------
// k_dec_gather: files at any byte address into the pass image at 4-byte-aligned offsets, zeros from each file's end to
// its 4-byte boundary.  blockIdx.y walks the table, the x dimension the aligned 16-byte chunks of the file's
// destination; a lane makes the four words of its chunk.  A chunk that lies wholly inside the padded destination range
// takes its 16 source bytes from the one or two ALIGNED 16-byte source words that hold them (two 16-byte loads, a word
// select by the source's word misalignment, v_alignbyte_b32 by its byte misalignment) and goes out in one 16-byte store;
// the chunks at a file's head and tail make their words one by one from aligned 4-byte loads, funnel-shifted the same
// way, and store those inside the range.  Bytes at or past `bytes` are masked to zero, which is the pad.
// Loads touch only aligned words that hold at least one byte of [src, src + bytes): such a word may reach up to 15 bytes
// before src or past the end, and is still inside the source's mapping, because device allocations start at least
// 16-byte aligned and are mapped in whole pages.
// ---------------------------------------------------------------------------------------------
typedef uint32_t gather_u4 __attribute__((ext_vector_type(4)));

// the word at byte offset o (a multiple of 4, o < bytes) of a source of `bytes` bytes, bytes past the end zero
__device__ __forceinline__ uint32_t gather_word(const uint8_t* src, uint32_t bytes, uint32_t o)
{
  const uintptr_t s = (uintptr_t)src + o;
  const uint32_t sh = (uint32_t)(s & 3u), valid = bytes - o;
  const uint32_t* a = (const uint32_t*)(s & ~(uintptr_t)3);
  const uint32_t lo = a[0];                                     // holds byte o
  const uint32_t hi = (sh != 0 && 4u - sh < valid) ? a[1] : 0u;  // holds byte o + 4 - sh
  const uint32_t w = __builtin_amdgcn_alignbyte(hi, lo, sh);
  return (valid >= 4u) ? w : (w & ((1u << (8u * valid)) - 1u));
}

__global__ __launch_bounds__(256)
void k_dec_gather(const sla_hip_dec_gather* __restrict__ table, uint32_t num_entries, uint8_t* __restrict__ image,
                  uint64_t image_bytes)
{
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (uint64_t)gridDim.x * blockDim.x;
  for (uint32_t e = blockIdx.y; e < num_entries; e += gridDim.y) {
    const sla_hip_dec_gather g = table[e];
    const uint32_t bytes = g.bytes;
    const uint64_t padded = ((uint64_t)bytes + 3u) & ~(uint64_t)3;
    if ((g.dst_off & 3u) != 0 || g.dst_off > image_bytes || padded > image_bytes - g.dst_off) { continue; }
    uint8_t* dst = image + g.dst_off;
    const uint32_t head = (uint32_t)((uintptr_t)dst & 15u);     // bytes of the first chunk before the destination
    const uint64_t chunks = (head + padded + 15u) >> 4;
    for (uint64_t c = tid; c < chunks; c += nt) {
      const int64_t o0 = (int64_t)(c << 4) - head;               // the chunk's first byte, relative to the destination
      if (o0 >= 0 && (uint64_t)o0 + 16u <= padded) {
        const uint32_t o = (uint32_t)o0;
        const uintptr_t s = (uintptr_t)g.src + o;
        const uint32_t r = (uint32_t)(s & 15u);
        const gather_u4* a = (const gather_u4*)(s & ~(uintptr_t)15);
        const gather_u4 q0 = a[0];                               // holds byte o (o < bytes)
        gather_u4 q1 = {0u, 0u, 0u, 0u};
        if (r != 0 && 16u - r < bytes - o) { q1 = a[1]; }        // holds byte o + 16 - r
        uint32_t w[5];
        switch (r >> 2) {
          case 0:  w[0] = q0.x; w[1] = q0.y; w[2] = q0.z; w[3] = q0.w; w[4] = q1.x; break;
          case 1:  w[0] = q0.y; w[1] = q0.z; w[2] = q0.w; w[3] = q1.x; w[4] = q1.y; break;
          case 2:  w[0] = q0.z; w[1] = q0.w; w[2] = q1.x; w[3] = q1.y; w[4] = q1.z; break;
          default: w[0] = q0.w; w[1] = q1.x; w[2] = q1.y; w[3] = q1.z; w[4] = q1.w; break;
        }
        uint32_t v[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
          const uint32_t valid = (bytes - o > 4u * k) ? (bytes - o - 4u * k) : 0u;
          const uint32_t x = __builtin_amdgcn_alignbyte(w[k + 1], w[k], r & 3u);
          v[k] = (valid >= 4u) ? x : (x & ((1u << (8u * valid)) - 1u));
        }
        gather_u4 q; q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        *(gather_u4*)(dst + o) = q;
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
          const int64_t ok = o0 + 4 * (int64_t)k;
          if (ok >= 0 && (uint64_t)ok < padded) { *(uint32_t*)(dst + ok) = gather_word(g.src, bytes, (uint32_t)ok); }
        }
      }
    }
  }
}

#include "kernels/walk_wide.inc"
#include "kernels/salvage.inc"
#include "kernels/verify.inc"
#include "kernels/judge.inc"
#include "kernels/splice.inc"

}  // namespace

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// blocks per wave of k_dec_bits: enough waves for every SIMD of the chip before a wave takes a second block
extern "C" uint32_t sla_hip_dec_bits_lanes(uint32_t num_blocks, uint32_t num_channels)
{
  uint32_t lanes = (num_blocks + 1023) / 1024;
  if (lanes < 1) { lanes = 1; }
  if (lanes > 64 / num_channels) { lanes = 64 / num_channels; }     // lanes * channels rows of LDS staging
  return lanes;
}

extern "C" int sla_hip_launch_dec_bits(const uint32_t* d_image, uint64_t image_bytes,
                                       const sla_hip_dec_block* d_blocks, uint32_t num_blocks,
                                       uint32_t num_channels, uint32_t bits_per_sample, uint32_t offset_lshift,
                                       uint32_t mid_side, uint32_t parcor_order, uint32_t longterm_order,
                                       uint32_t want_crc, int32_t* d_planes, uint64_t plane_stride,
                                       sla_hip_dec_info* d_info, sla_hip_dec_chan* d_chan, int32_t* d_kint,
                                       sla_hip_stream_t stream)
{
  return sla_hip_launch_dec_bits_x(d_image, image_bytes, d_blocks, num_blocks, num_channels, bits_per_sample, offset_lshift,
                                   mid_side, parcor_order, longterm_order, want_crc, d_planes, plane_stride, d_info, d_chan,
                                   d_kint, stream, nullptr);
}

extern "C" int sla_hip_launch_dec_bits_x(const uint32_t* d_image, uint64_t image_bytes,
                                         const sla_hip_dec_block* d_blocks, uint32_t num_blocks,
                                         uint32_t num_channels, uint32_t bits_per_sample, uint32_t offset_lshift,
                                         uint32_t mid_side, uint32_t parcor_order, uint32_t longterm_order,
                                         uint32_t want_crc, int32_t* d_planes, uint64_t plane_stride,
                                         sla_hip_dec_info* d_info, sla_hip_dec_chan* d_chan, int32_t* d_kint,
                                         sla_hip_stream_t stream, const uint64_t* d_block_end)
{
  if (d_image == nullptr || d_blocks == nullptr || d_planes == nullptr || d_info == nullptr || d_chan == nullptr || d_kint == nullptr) {
    return SLA_APIRESULT_INVALID_ARGUMENT;
  }
  if (num_channels == 0 || num_channels > 8 || bits_per_sample == 0 || bits_per_sample > 32 || offset_lshift >= bits_per_sample
      || parcor_order > 255 || longterm_order > 5 || (mid_side && num_channels != 2)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_blocks == 0) { return 0; }
  hipStream_t st = (hipStream_t)stream;
  if (want_crc) {
    hipLaunchKernelGGL(k_dec_crc, dim3((num_blocks + 3) / 4), dim3(256), 0, st, (const uint8_t*)d_image, d_blocks, num_blocks, d_info);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { return hip_rc(e); }
  }
  dec_bits_args a;
  a.image = d_image; a.image_bytes = image_bytes; a.block_end = d_block_end; a.blocks = d_blocks; a.num_blocks = num_blocks;
  a.bps = bits_per_sample; a.lshift = offset_lshift; a.mid_side = mid_side; a.order = parcor_order; a.ntaps = longterm_order;
  const uint32_t lanes = sla_hip_dec_bits_lanes(num_blocks, num_channels);
  a.lanes = lanes;
  a.planes = d_planes; a.stride = plane_stride; a.info = d_info; a.chan = d_chan; a.kint = d_kint;
  const dim3 grid((num_blocks + lanes - 1) / lanes), block(64);
  const size_t lds = sizeof(uint32_t) * ((size_t)lanes * num_channels * DEC_ROW + (size_t)lanes * (DEC_WIN * num_channels + 1));
#define SLA_DEC_BITS(B)                                                                \
  switch (num_channels) {                                                              \
    case 1: hipLaunchKernelGGL((k_dec_bits<1, B>), grid, block, lds, st, a); break;    \
    case 2: hipLaunchKernelGGL((k_dec_bits<2, B>), grid, block, lds, st, a); break;    \
    case 3: hipLaunchKernelGGL((k_dec_bits<3, B>), grid, block, lds, st, a); break;    \
    case 4: hipLaunchKernelGGL((k_dec_bits<4, B>), grid, block, lds, st, a); break;    \
    case 5: hipLaunchKernelGGL((k_dec_bits<5, B>), grid, block, lds, st, a); break;    \
    case 6: hipLaunchKernelGGL((k_dec_bits<6, B>), grid, block, lds, st, a); break;    \
    case 7: hipLaunchKernelGGL((k_dec_bits<7, B>), grid, block, lds, st, a); break;    \
    default: hipLaunchKernelGGL((k_dec_bits<8, B>), grid, block, lds, st, a); break;   \
  }
  if (d_block_end != nullptr) { SLA_DEC_BITS(true) } else { SLA_DEC_BITS(false) }
#undef SLA_DEC_BITS
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_dec_lms(int32_t* d_planes, uint64_t plane_stride, const sla_hip_dec_block* d_blocks,
                                      const sla_hip_dec_info* d_info, uint32_t num_blocks, uint32_t num_channels,
                                      uint32_t lms_order, sla_hip_stream_t stream)
{
  if (d_planes == nullptr || d_blocks == nullptr || d_info == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (lms_order != 4 && lms_order != 8 && lms_order != 16 && lms_order != 32) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_blocks == 0) { return 0; }
  hipStream_t st = (hipStream_t)stream;
  const uint32_t jobs = num_blocks * num_channels, jpw = 64 / (2 * lms_order);
  const dim3 grid(((jobs + jpw - 1) / jpw + 3) / 4), block(256);
  switch (lms_order) {
    case 4:  hipLaunchKernelGGL(k_dec_lms<4>,  grid, block, 0, st, d_planes, plane_stride, d_blocks, d_info, num_blocks, num_channels); break;
    case 8:  hipLaunchKernelGGL(k_dec_lms<8>,  grid, block, 0, st, d_planes, plane_stride, d_blocks, d_info, num_blocks, num_channels); break;
    case 16: hipLaunchKernelGGL(k_dec_lms<16>, grid, block, 0, st, d_planes, plane_stride, d_blocks, d_info, num_blocks, num_channels); break;
    default: hipLaunchKernelGGL(k_dec_lms<32>, grid, block, 0, st, d_planes, plane_stride, d_blocks, d_info, num_blocks, num_channels); break;
  }
  return hip_rc(hipGetLastError());
}

extern "C" uint32_t sla_hip_dec_ltm_window(void) { return DEC_LTM_CHUNK; }

extern "C" int sla_hip_launch_dec_ltm(int32_t* d_planes, uint64_t plane_stride, const sla_hip_dec_block* d_blocks,
                                      const sla_hip_dec_info* d_info, const sla_hip_dec_chan* d_chan,
                                      uint32_t num_blocks, uint32_t num_channels, uint32_t longterm_order,
                                      uint32_t max_block_samples, sla_hip_stream_t stream)
{
  if (d_planes == nullptr || d_blocks == nullptr || d_info == nullptr || d_chan == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8 || longterm_order > 5) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_blocks == 0 || longterm_order == 0) { return 0; }
  const size_t lds = (size_t)max_block_samples * sizeof(int32_t);
  if (lds > SLA_HIP_LDS_BUDGET) {                            // a block may not fit LDS: the ring kernel, whatever the blocks' lengths
    hipLaunchKernelGGL(k_dec_ltm_far, dim3(num_blocks * num_channels), dim3(64), 0, (hipStream_t)stream, d_planes, plane_stride,
                       d_blocks, d_info, d_chan, num_channels, longterm_order);
    return hip_rc(hipGetLastError());
  }
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_dec_ltm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { return hip_rc(e); }
  }
  hipLaunchKernelGGL(k_dec_ltm, dim3(num_blocks * num_channels), dim3(64), lds, (hipStream_t)stream, d_planes, plane_stride,
                     d_blocks, d_info, d_chan, num_channels, longterm_order);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_dec_lattice(int32_t* d_planes, uint64_t plane_stride, const sla_hip_dec_block* d_blocks,
                                          const sla_hip_dec_info* d_info, uint32_t num_blocks, uint32_t num_channels,
                                          const int32_t* d_kint, uint32_t parcor_order, uint32_t deemphasis, sla_hip_stream_t stream)
{
  if (d_planes == nullptr || d_blocks == nullptr || d_info == nullptr || d_kint == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8 || parcor_order > 255) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_blocks == 0) { return 0; }
  hipStream_t st = (hipStream_t)stream;
  const uint32_t jobs = num_blocks * num_channels;
#define SLA_DEC_LATTICE(G, R)                                                                                          \
  hipLaunchKernelGGL((k_dec_lattice<G, R>), dim3(((jobs + (64 / G) - 1) / (64 / G) + 3) / 4), dim3(256), 0, st, d_planes, \
                     plane_stride, d_blocks, d_info, num_blocks, num_channels, d_kint, parcor_order, deemphasis)
  if (parcor_order <= 16) { SLA_DEC_LATTICE(16, 1); }
  else if (parcor_order <= 32) { SLA_DEC_LATTICE(32, 1); }
  else if (parcor_order <= 64) { SLA_DEC_LATTICE(64, 1); }
  else if (parcor_order <= 128) { SLA_DEC_LATTICE(64, 2); }
  else { SLA_DEC_LATTICE(64, 4); }
#undef SLA_DEC_LATTICE
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_dec_finish(int32_t* d_planes, uint64_t plane_stride, uint32_t num_channels,
                                         uint32_t num_samples, uint32_t mid_side, uint32_t shift, sla_hip_stream_t stream)
{
  if (d_planes == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8 || shift > 31 || (mid_side && num_channels != 2) || plane_stride < num_samples) {
    return SLA_APIRESULT_INVALID_ARGUMENT;
  }
  if (num_samples == 0) { return 0; }
  hipLaunchKernelGGL(k_dec_finish, dim3((num_samples + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_planes, plane_stride,
                     num_channels, num_samples, mid_side, shift);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_dec_finish_batch(const int32_t* d_planes, uint64_t plane_stride, uint32_t num_channels,
                                               const sla_hip_dec_file* d_files, uint32_t num_files, uint32_t max_samples,
                                               int32_t* d_out, sla_hip_stream_t stream)
{
  if (d_planes == nullptr || d_files == nullptr || d_out == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_files == 0 || max_samples == 0) { return 0; }
  // enough workgroups to fill the chip for one long file; short files of a big pass get a workgroup row each
  uint32_t gx = (max_samples + 255) / 256;
  if (gx > 1024) { gx = 1024; }
  const uint32_t gy = (num_files < 65535u) ? num_files : 65535u;
  hipLaunchKernelGGL(k_dec_finish_batch, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, d_planes, plane_stride, num_channels,
                     d_files, num_files, d_out);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_dec_emit_batch(const int32_t* d_planes, uint64_t plane_stride, const sla_hip_dec_emit* d_files,
                                             uint32_t num_files, uint32_t max_samples, uint32_t sample_format, sla_hip_stream_t stream)
{
  if (d_planes == nullptr || d_files == nullptr || sample_format > SLA_HIP_PCM_F32) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_files == 0 || max_samples == 0) { return 0; }
  // a workgroup row covers 1024 samples of a planar file (256 lanes x 4); longer files and the other shapes grid-stride
  uint32_t gx = (max_samples + 1023) / 1024;
  if (gx > 1024) { gx = 1024; }
  const dim3 grid(gx, (num_files < 65535u) ? num_files : 65535u), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (sample_format) {
    case SLA_HIP_PCM_S32_LEFT: hipLaunchKernelGGL(k_dec_emit_batch<SLA_HIP_PCM_S32_LEFT>, grid, block, 0, st, d_planes, plane_stride, d_files, num_files); break;
    case SLA_HIP_PCM_S32:      hipLaunchKernelGGL(k_dec_emit_batch<SLA_HIP_PCM_S32>, grid, block, 0, st, d_planes, plane_stride, d_files, num_files); break;
    case SLA_HIP_PCM_S16:      hipLaunchKernelGGL(k_dec_emit_batch<SLA_HIP_PCM_S16>, grid, block, 0, st, d_planes, plane_stride, d_files, num_files); break;
    default:                   hipLaunchKernelGGL(k_dec_emit_batch<SLA_HIP_PCM_F32>, grid, block, 0, st, d_planes, plane_stride, d_files, num_files); break;
  }
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_dec_walk(const sla_hip_dec_walk_file* d_files, uint32_t num_files, uint32_t max_block_samples,
                                       uint32_t crc_check, sla_hip_dec_walk_result* d_results, sla_hip_dec_block* d_blocks,
                                       uint64_t* d_block_end, uint32_t* d_crc_field, sla_hip_stream_t stream)
{
  if (d_files == nullptr || d_results == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if ((d_blocks != nullptr || d_block_end != nullptr || d_crc_field != nullptr)
      && (d_blocks == nullptr || d_block_end == nullptr || d_crc_field == nullptr)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_files == 0) { return 0; }
  hipLaunchKernelGGL(k_dec_walk, dim3((num_files + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_files, num_files,
                     max_block_samples, crc_check, d_results, d_blocks, d_block_end, d_crc_field);
  return hip_rc(hipGetLastError());
}

extern "C" uint64_t sla_hip_dec_wide_scratch_bytes(uint32_t data_size, uint32_t node_capacity)
{
  return SLA_HIP_DEC_WIDE_SCRATCH_BYTES(data_size, node_capacity);
}

extern "C" uint32_t sla_hip_dec_wide_rounds(uint32_t data_size, uint32_t node_capacity)
{
  // blocks are at least 8 bytes long and the last starts 11 bytes before the end: a path has no more nodes than that,
  // and no more than the capacity
  uint64_t longest = (data_size < 54u) ? 0u : (uint64_t)(data_size - 54u) / 8u + 1u;
  uint32_t r = 0;
  if (longest > node_capacity) { longest = node_capacity; }
  while (((uint64_t)1 << r) < longest) { r++; }
  return r;
}

// the wide walk's scratch, carved as SLA_HIP_DEC_WIDE_SCRATCH_BYTES counts it (every part a multiple of 16 bytes); returns
// the byte behind it
static uint8_t* wide_carve(void* d_scratch, uint32_t data_size, uint32_t node_capacity, wide_arrays& A)
{
  const uint64_t max_tiles = SLA_HIP_DEC_WIDE_TILES(data_size), capa = ((uint64_t)node_capacity + 3u) & ~(uint64_t)3;
  uint8_t* s = (uint8_t*)d_scratch;
  A.info = (sla_hip_dec_wide_info*)s;                      s += 64;
  A.mask = (uint32_t*)s;                                   s += max_tiles * WIDE_TILE * 4u;
  A.word_first = (uint32_t*)s;                             s += max_tiles * WIDE_TILE * 4u;
  A.tile = (uint32_t*)s;                                   s += (max_tiles * 4u + 15u) & ~(uint64_t)15;
  for (int k = 0; k < 2; k++) { A.sum[k] = (uint64_t*)s;   s += capa * 8u; }
  for (int k = 0; k < 2; k++) { A.spos[k] = (uint64_t*)s;  s += capa * 8u; }
  for (int k = 0; k < 2; k++) { A.jump[k] = (uint32_t*)s;  s += capa * 4u; }
  for (int k = 0; k < 2; k++) { A.rank[k] = (uint32_t*)s;  s += capa * 4u; }
  A.pos = (uint32_t*)s;                                    s += capa * 4u;
  A.bsize = (uint32_t*)s;                                  s += capa * 4u;
  A.ncrc = (uint32_t*)s;                                   s += capa * 4u;
  A.succ = (uint32_t*)s;                                   s += capa * 4u;
  return s;
}

extern "C" int sla_hip_launch_dec_walk_wide(const sla_hip_dec_walk_file* file, uint32_t max_block_samples, uint32_t crc_check,
                                            sla_hip_dec_walk_result* d_result, sla_hip_dec_block* d_blocks,
                                            uint64_t* d_block_end, uint32_t* d_crc_field, uint32_t node_capacity,
                                            void* d_scratch, sla_hip_stream_t stream)
{
  if (file == nullptr || d_result == nullptr || d_scratch == nullptr || node_capacity == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if ((d_blocks != nullptr || d_block_end != nullptr || d_crc_field != nullptr)
      && (d_blocks == nullptr || d_block_end == nullptr || d_crc_field == nullptr)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (((uintptr_t)d_scratch & 15u) != 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  const sla_hip_dec_walk_file fi = *file;
  const hipStream_t st = (hipStream_t)stream;
  const uint32_t rows = (d_blocks != nullptr) ? fi.max_rows : 0u;
  if (fi.total == 0 || fi.data_size < SLA_HEADER_SIZE + DEC_WALK_MIN_HEADER) {
    const uint32_t g = (rows > 256u * 1024u) ? 1024u : (rows + 255u) / 256u;
    hipLaunchKernelGGL(k_wide_none, dim3(g ? g : 1u), dim3(256), 0, st, fi, (sla_hip_dec_wide_info*)d_scratch, d_result, d_blocks,
                       d_block_end, d_crc_field);
    return hip_rc(hipGetLastError());
  }
  if (fi.src == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  const uint32_t head = (uint32_t)((uintptr_t)fi.src & 15u);
  const uint32_t words = (uint32_t)(((uint64_t)head + fi.data_size + 31u) >> 5), tiles = (words + WIDE_TILE - 1u) / WIDE_TILE;
  wide_arrays A;
  (void)wide_carve(d_scratch, fi.data_size, node_capacity, A);
  const uint32_t rounds = sla_hip_dec_wide_rounds(fi.data_size, node_capacity);
  const uint32_t gn = (node_capacity > 256u * 1024u) ? 1024u : (node_capacity + 255u) / 256u;
  const uint32_t most = (rows > node_capacity) ? rows : node_capacity;
  const uint32_t gr = (most > 256u * 1024u) ? 1024u : (most + 255u) / 256u;
  hipLaunchKernelGGL(k_wide_find, dim3(tiles), dim3(WIDE_TILE), 0, st, fi.src, fi.data_size, words, A.mask, A.tile);
  hipLaunchKernelGGL(k_wide_scan, dim3(1), dim3(1024), 0, st, A.tile, tiles, A.info);
  hipLaunchKernelGGL(k_wide_index, dim3(tiles), dim3(WIDE_TILE), 0, st, A.mask, words, A.tile, A.word_first);
  hipLaunchKernelGGL(k_wide_nodes, dim3(tiles), dim3(WIDE_TILE), 0, st, fi.src, fi.data_size, words, node_capacity, A);
  for (uint32_t r = 0; r < rounds; r++) {
    hipLaunchKernelGGL(k_wide_round, dim3(gn), dim3(256), 0, st, node_capacity, 1u << r, A, r & 1u);
  }
  hipLaunchKernelGGL(k_wide_cut, dim3(gn), dim3(256), 0, st, fi, max_block_samples, node_capacity, A, rounds & 1u);
  hipLaunchKernelGGL(k_wide_rows, dim3(gr), dim3(256), 0, st, fi, crc_check, node_capacity, A, rounds & 1u, d_result, d_blocks,
                     d_block_end, d_crc_field);
  return hip_rc(hipGetLastError());
}

extern "C" uint64_t sla_hip_dec_salvage_scratch_bytes(uint32_t data_size, uint32_t node_capacity)
{
  return SLA_HIP_DEC_SALVAGE_SCRATCH_BYTES(data_size, node_capacity);
}

extern "C" int sla_hip_launch_dec_salvage_scan(const sla_hip_dec_walk_file* file, uint32_t num_channels, uint32_t max_block_samples,
                                               sla_hip_salvage_scan* d_result, sla_hip_dec_block* d_blocks, uint64_t* d_block_end,
                                               uint32_t* d_crc_field, uint32_t node_capacity, void* d_scratch, sla_hip_stream_t stream)
{
  if (file == nullptr || d_result == nullptr || d_scratch == nullptr || node_capacity == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if ((d_blocks != nullptr || d_block_end != nullptr || d_crc_field != nullptr)
      && (d_blocks == nullptr || d_block_end == nullptr || d_crc_field == nullptr)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (((uintptr_t)d_scratch & 15u) != 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  const sla_hip_dec_walk_file fi = *file;
  const hipStream_t st = (hipStream_t)stream;
  const uint32_t rows = (d_blocks != nullptr) ? fi.max_rows : 0u;
  if (fi.data_size < SLA_HEADER_SIZE + DEC_WALK_MIN_HEADER) {
    const uint32_t g = (rows > 256u * 1024u) ? 1024u : (rows + 255u) / 256u;
    hipLaunchKernelGGL(k_salvage_none, dim3(g ? g : 1u), dim3(256), 0, st, fi, (sla_hip_dec_wide_info*)d_scratch, d_result, d_blocks,
                       d_block_end, d_crc_field);
    return hip_rc(hipGetLastError());
  }
  if (fi.src == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  const uint32_t head = (uint32_t)((uintptr_t)fi.src & 15u);
  const uint32_t words = (uint32_t)(((uint64_t)head + fi.data_size + 31u) >> 5), tiles = (words + WIDE_TILE - 1u) / WIDE_TILE;
  const uint64_t capa = ((uint64_t)node_capacity + 3u) & ~(uint64_t)3;
  wide_arrays A;
  salvage_arrays B;
  // the salvage arrays behind the wide walk's, as SLA_HIP_DEC_SALVAGE_SCRATCH_BYTES counts them
  uint8_t* s = wide_carve(d_scratch, fi.data_size, node_capacity, A);
  B.info = (salvage_info*)s;                               s += 64;
  B.csum = (uint64_t*)s;                                   s += capa * 8u;
  for (int k = 0; k < 2; k++) { B.last[k] = (uint32_t*)s;  s += capa * 4u; }
  B.sound = (uint32_t*)s;                                  s += capa * 4u;
  B.ssucc = (uint32_t*)s;                                  s += capa * 4u;
  B.cend = (uint32_t*)s;
  const uint32_t rounds = sla_hip_dec_wide_rounds(fi.data_size, node_capacity), fin = rounds & 1u;
  const uint32_t gn = (node_capacity > 256u * 1024u) ? 1024u : (node_capacity + 255u) / 256u;
  const uint32_t gw = (node_capacity > 4u * 4096u) ? 4096u : (node_capacity + 3u) / 4u;      // one wave per node, four per workgroup
  const uint32_t most = (rows > node_capacity) ? rows : node_capacity;
  const uint32_t gr = (most > 256u * 1024u) ? 1024u : (most + 255u) / 256u;
  hipLaunchKernelGGL(k_salvage_init, dim3(1), dim3(64), 0, st, B.info);
  hipLaunchKernelGGL(k_wide_find, dim3(tiles), dim3(WIDE_TILE), 0, st, fi.src, fi.data_size, words, A.mask, A.tile);
  hipLaunchKernelGGL(k_wide_scan, dim3(1), dim3(1024), 0, st, A.tile, tiles, A.info);
  hipLaunchKernelGGL(k_wide_index, dim3(tiles), dim3(WIDE_TILE), 0, st, A.mask, words, A.tile, A.word_first);
  hipLaunchKernelGGL(k_wide_nodes, dim3(tiles), dim3(WIDE_TILE), 0, st, fi.src, fi.data_size, words, node_capacity, A);
  hipLaunchKernelGGL(k_salvage_sound, dim3(gw), dim3(256), 0, st, fi.src, num_channels, max_block_samples, node_capacity, A, B);
  for (uint32_t pass = 0; pass < 2; pass++) {
    hipLaunchKernelGGL(k_salvage_link, dim3(gn), dim3(256), 0, st, node_capacity, A, B, pass);
    for (uint32_t r = 0; r < rounds; r++) {
      hipLaunchKernelGGL(k_salvage_round, dim3(gn), dim3(256), 0, st, node_capacity, 1u << r, A, B, r & 1u);
    }
    hipLaunchKernelGGL(k_salvage_cut, dim3(gn), dim3(256), 0, st, fi.total, node_capacity, A, B, fin, pass);
    if (pass == 0) {
      hipLaunchKernelGGL(k_salvage_prefix, dim3(gn), dim3(256), 0, st, fi, node_capacity, A, B, fin, d_blocks, d_block_end, d_crc_field);
      hipLaunchKernelGGL(k_salvage_pick, dim3(gn), dim3(256), 0, st, fi, node_capacity, A, B);
    }
  }
  hipLaunchKernelGGL(k_salvage_rows, dim3(gr), dim3(256), 0, st, fi, node_capacity, A, B, fin, d_result, d_blocks, d_block_end, d_crc_field);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_salvage_crc(const uint8_t* d_image, sla_hip_dec_block* d_blocks, const uint32_t* d_crc_field,
                                          uint32_t num_blocks, uint32_t* d_bad, sla_hip_stream_t stream)
{
  if (d_image == nullptr || d_blocks == nullptr || d_crc_field == nullptr || d_bad == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_blocks == 0) { return 0; }
  hipLaunchKernelGGL(k_salvage_crc, dim3((num_blocks + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_image, d_blocks, d_crc_field,
                     num_blocks, d_bad);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_dec_conceal(int32_t* d_planes, uint64_t plane_stride, uint32_t num_channels,
                                          const sla_hip_dec_conceal* d_list, uint32_t count, uint32_t max_samples, sla_hip_stream_t stream)
{
  if (d_planes == nullptr || d_list == nullptr || num_channels == 0 || num_channels > 8) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (count == 0 || max_samples == 0) { return 0; }
  uint32_t gx = (max_samples + 255u) / 256u;
  if (gx > 1024u) { gx = 1024u; }
  hipLaunchKernelGGL(k_dec_conceal, dim3(gx, (count < 65535u) ? count : 65535u), dim3(256), 0, (hipStream_t)stream, d_planes, plane_stride,
                     num_channels, d_list, count);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_dec_walk_window(const sla_hip_dec_window_file* d_files, uint32_t num_files, uint32_t max_block_samples,
                                              sla_hip_dec_window_result* d_results, sla_hip_dec_block* d_blocks,
                                              uint64_t* d_block_end, uint32_t* d_crc_field, sla_hip_stream_t stream)
{
  if (d_files == nullptr || d_results == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if ((d_blocks != nullptr || d_block_end != nullptr || d_crc_field != nullptr)
      && (d_blocks == nullptr || d_block_end == nullptr || d_crc_field == nullptr)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_files == 0) { return 0; }
  hipLaunchKernelGGL(k_dec_walk_window, dim3((num_files + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_files, num_files,
                     max_block_samples, d_results, d_blocks, d_block_end, d_crc_field);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_dec_gather(const sla_hip_dec_gather* d_table, uint32_t num_entries, uint32_t max_bytes,
                                         uint8_t* d_image, uint64_t image_bytes, sla_hip_stream_t stream)
{
  if (d_table == nullptr || d_image == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_entries == 0 || max_bytes == 0) { return 0; }
  // a workgroup row covers 4096 bytes of a file (256 lanes x 16); longer files grid-stride
  uint64_t gx = ((uint64_t)max_bytes + 15 + 4095) / 4096;
  if (gx > 1024) { gx = 1024; }
  const dim3 grid((uint32_t)gx, (num_entries < 65535u) ? num_entries : 65535u), block(256);
  hipLaunchKernelGGL(k_dec_gather, grid, block, 0, (hipStream_t)stream, d_table, num_entries, d_image, image_bytes);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_dec_deemphasis(int32_t* d_data, uint32_t num_samples, int32_t previous, uint32_t coef_shift,
                                             sla_hip_stream_t stream)
{
  if (d_data == nullptr || coef_shift < 1 || coef_shift > 30) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_samples == 0) { return 0; }
  hipLaunchKernelGGL(k_dec_deemphasis, dim3(1), dim3(64), 0, (hipStream_t)stream, d_data, num_samples, previous, coef_shift);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_verify_blocks(const int32_t* d_planes, uint64_t plane_stride, const int32_t* d_source,
                                            uint64_t source_stride, const sla_hip_dec_block* d_blocks,
                                            const sla_hip_dec_info* d_info, const sla_hip_verify_expect* d_expect,
                                            const uint32_t* d_seg_of_block, uint32_t num_blocks, uint32_t num_channels,
                                            uint32_t mid_side, uint32_t shift, const uint32_t* d_image, uint64_t image_bytes,
                                            uint64_t* d_report, sla_hip_stream_t stream)
{
  if (d_planes == nullptr || d_source == nullptr || d_blocks == nullptr || d_info == nullptr || d_expect == nullptr
      || d_report == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8 || shift > 31 || (mid_side && num_channels != 2)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_blocks == 0) { return 0; }
  verify_args a;
  a.planes = d_planes; a.stride = plane_stride; a.source = d_source; a.sstride = source_stride;
  a.blocks = d_blocks; a.info = d_info; a.expect = d_expect; a.seg_of_block = d_seg_of_block;
  a.image = (const uint8_t*)d_image; a.image_bytes = image_bytes;
  a.report = (unsigned long long*)d_report;
  a.num_channels = num_channels; a.mid_side = mid_side; a.shift = shift;
  hipLaunchKernelGGL(k_verify_blocks, dim3(num_blocks), dim3(256), 0, (hipStream_t)stream, a);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_dec_judge(const uint8_t* d_image, uint64_t image_bytes, const sla_hip_dec_block* d_blocks,
                                        const sla_hip_dec_info* d_info, uint32_t num_blocks, const sla_hip_dec_judge_item* d_items,
                                        uint32_t num_items, uint32_t crc_check, uint32_t lms_ok, sla_hip_dec_emit* d_emit,
                                        uint32_t num_emit, sla_hip_window_outcome* d_outcomes, uint32_t num_outcomes,
                                        sla_hip_stream_t stream)
{
  if (d_items == nullptr || d_outcomes == nullptr || (num_emit > 0 && d_emit == nullptr)
      || (num_blocks > 0 && (d_image == nullptr || d_blocks == nullptr || d_info == nullptr))) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_items == 0) { return 0; }
  // one wave per item, four items per workgroup
  hipLaunchKernelGGL(k_dec_judge, dim3((num_items + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_image, image_bytes, d_blocks, d_info,
                     num_blocks, d_items, num_items, crc_check, lms_ok, d_emit, num_emit, d_outcomes, num_outcomes);
  return hip_rc(hipGetLastError());
}

static bool splice_format_ok(uint32_t num_channels, uint32_t width, uint32_t mid_side)
{
  return num_channels >= 1 && num_channels <= 8 && width >= 1 && width <= 32 && !(mid_side && num_channels != 2);
}

extern "C" int sla_hip_launch_splice_check(const sla_hip_splice_check* d_table, uint32_t num_entries, uint32_t crc_check,
                                           const int32_t* d_planes, uint64_t plane_stride, uint32_t num_channels, uint32_t width,
                                           uint32_t mid_side, const sla_hip_window_outcome* d_outcomes, uint32_t num_outcomes,
                                           uint64_t* d_verdicts, uint32_t num_verdicts, sla_hip_stream_t stream)
{
  if (d_table == nullptr || d_planes == nullptr || d_outcomes == nullptr || d_verdicts == nullptr
      || !splice_format_ok(num_channels, width, mid_side)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_entries == 0) { return 0; }
  // one wave per entry, four entries per workgroup
  hipLaunchKernelGGL(k_splice_check, dim3((num_entries + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_table, num_entries, crc_check,
                     d_planes, plane_stride, num_channels, width, mid_side ? 1u : 0u, d_outcomes, num_outcomes,
                     (unsigned long long*)d_verdicts, num_verdicts);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_splice_edges(const int32_t* d_planes, uint64_t plane_stride, const sla_hip_splice_edge* d_table,
                                           uint32_t num_entries, uint32_t num_channels, uint32_t width, uint32_t mid_side,
                                           sla_hip_stream_t stream)
{
  if (d_table == nullptr || d_planes == nullptr || !splice_format_ok(num_channels, width, mid_side)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_entries == 0) { return 0; }
  // one workgroup per block; longer tables grid-stride
  hipLaunchKernelGGL(k_splice_edges, dim3((num_entries < 65535u) ? num_entries : 65535u), dim3(256), 0, (hipStream_t)stream, d_planes,
                     plane_stride, d_table, num_entries, num_channels, width, mid_side ? 1u : 0u);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_splice_copy(const sla_hip_splice_copy* d_table, uint32_t num_entries, uint32_t max_bytes,
                                          sla_hip_stream_t stream)
{
  if (d_table == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_entries == 0 || max_bytes == 0) { return 0; }
  // a workgroup row covers 4096 bytes of an entry (256 lanes x 16); longer entries grid-stride
  uint64_t gx = ((uint64_t)max_bytes + 15 + 4095) / 4096;
  if (gx > 1024) { gx = 1024; }
  const dim3 grid((uint32_t)gx, (num_entries < 65535u) ? num_entries : 65535u), block(256);
  hipLaunchKernelGGL(k_splice_copy, grid, block, 0, (hipStream_t)stream, d_table, num_entries);
  return hip_rc(hipGetLastError());
}
