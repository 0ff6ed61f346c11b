// kernels/pack.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): device bit-pack: k_rice_k / k_rice_k2 / k_rice_bits / k_rice_write / k_block_crc, k_unpack16 / k_unpack24, their launchers
// ---------------------------------------------------------------------------------------------
// Bit-pack on the device (SURVEY 8(f) row 2): recursive-Rice / Golomb / gamma coding of the final
// residual (reference src/SLACoder.c:45-82, 120-138, 224-270, 429-467), block assembly and CRC16
// (src/SLAEncoder.c:682-798, src/SLAUtility.c:322-339).
//
//   k_rice_k     one lane per (block, channel): walks the residual with the two adaptive parameters
//                (8.8 fixed-point EMA, serial in time) and stores log2 of both Rice moduli per sample.
//                Blocks in fixed-Golomb mode need no state.
//   k_rice_bits  one wave per (block, channel): the channel's total bit count (code lengths are stateless)
//   k_rice_write one workgroup per block: header bytes, then tiles of 256 interleaved (sample, channel)
//                elements -- code length from (value, k0, k1), workgroup prefix sum -> bit offset, and
//                the <= 3 non-zero pieces of the codeword OR-ed into the zero-initialised image
//                (MSB-first, 32-bit atomics on byte-swapped words).  Unary zero runs cost nothing.
//   k_block_crc  one wave per block: slice-parallel CRC16-IBM over the block, size + CRC patched into the header.
//
// tests/test_gpu_pack.py drives these kernels alone through sla_hip_launch_rice_len / _rice_write against an independent
// writer (tests/slastream.py): initial parameters up to 2^32 - 1, residuals at the ends of int32, gamma escapes of 32 digits,
// tiles of more than 64 bits per sample, waves of jobs of 1 .. 1001 samples in both modes, every alignment of the planes and
// of the image, RAW fields of 4 .. 33 bits (the 33-bit side field of 32-bit mid/side input: its top bit is always clear, and
// the reference's own writer is undefined there -- the yardstick is the format).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fold_u32(int32_t s) { const uint32_t u = (uint32_t)s << 1; return (s < 0) ? ~u : u; }
__device__ __forceinline__ uint32_t ceil_log2_u32(uint32_t x) { return (x > 1) ? (32u - (uint32_t)__builtin_clz(x - 1u)) : 0u; }

// log2 of the Rice modulus of an adaptive parameter: 2^ceil(log2(round(p/2))), at least 1   src/SLACoder.c:30-31
__device__ __forceinline__ uint32_t rice_k(uint64_t p)
{
  uint32_t v = (uint32_t)(((p >> 1) + 128u) >> 8);
  v = v ? v : 1u;
  return ceil_log2_u32(v);
}
// 119/128 old + 9/128 code, the code term in 32-bit wrapping arithmetic                         src/SLACoder.c:26-28
__device__ __forceinline__ uint64_t rice_adapt(uint64_t p, uint32_t code)
{
  return (119u * p + (uint64_t)(uint32_t)(9u * (uint32_t)(code << 8)) + 64u) >> 7;
}
__device__ __forceinline__ uint32_t gamma_len(uint32_t g) { return (g == 0) ? 1u : (2u * ceil_log2_u32(g + 2u) - 1u); }

// length in bits of the recursive-Rice codeword of `v` under moduli 2^k0, 2^k1 (two parameters)
__device__ __forceinline__ uint32_t rrice_len(uint32_t v, uint32_t k0, uint32_t k1)
{
  if (v < (1u << k0)) { return 1u + k0; }
  v -= (1u << k0);
  const uint32_t q = 1u + (v >> k1);
  return (q < 16u) ? (q + 1u + k1) : (17u + gamma_len(q - 16u) + k1);
}
// length of the Golomb codeword of v with modulus m                                             src/SLACoder.c:45-82
__device__ __forceinline__ uint32_t golomb_len(uint32_t v, uint32_t m)
{
  const uint32_t q = v / m, r = v - q * m;
  if ((m & (m - 1u)) == 0) { return q + 1u + ceil_log2_u32(m); }
  const uint32_t b = ceil_log2_u32(m), cut = (1u << b) - m;
  return q + 1u + ((r < cut) ? (b - 1u) : b);
}

// The serial part only: the two adaptive parameters per sample (one lane per (block, channel)).  A lane issues its
// instructions one after the other, so every instruction that is not on the recurrence costs as much as one that is:
// the code lengths -- a function of (value, k0, k1), no state -- are left to k_rice_bits (a 10-second clip: 0.83 ->
// see DESIGN.md ms for the two kernels).
// One step of the walk in 32-bit arithmetic.  A parameter never leaves 32 bits (it starts as (uint32)(init << 8) and
// every step maps p to < 119/128 p + 2^25), but 119 p does: with p = 128 q + r and c = 128 cq + cr
//   (119 p + c + 64) >> 7  =  119 q + cq + ((119 r + cr + 64) >> 7),
// every term below 2^32.  c = (uint32)(9 (code << 8)) depends on the sample alone, so only the four operations of the
// second line sit on the serial chain.
__device__ __forceinline__ uint32_t rice_adapt32(uint32_t p, uint32_t code)
{
  // (measured: spelling 9 x and 119 q as opaque shift-adds instead of the multiplies the compiler picks is slower)
  const uint32_t c = 9u * (code << 8);
  const uint32_t q = p >> 7, r = p & 127u;
  return 119u * q + (c >> 7) + ((119u * r + (c & 127u) + 64u) >> 7);
}
__device__ __forceinline__ uint32_t rice_k32(uint32_t p)
{
  uint32_t v = ((p >> 1) + 128u) >> 8;
  v = v ? v : 1u;
  return ceil_log2_u32(v);
}

__global__ __launch_bounds__(64)
void k_rice_k(const int32_t* __restrict__ res, uint64_t stride, const sla_hip_rice_job* __restrict__ jobs,
              uint32_t num_jobs, uint16_t* __restrict__ kk)
{
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= num_jobs) { return; }
  const sla_hip_rice_job job = jobs[j];
  if (job.golomb_m != 0) { return; }                         // fixed-parameter mode: stateless
  const int32_t* in = res + (uint64_t)job.channel * stride + job.blk_off;
  uint16_t* ko = kk + (uint64_t)job.channel * stride + job.blk_off;
  const uint32_t n = job.blk_len;
  uint32_t p0 = (uint32_t)(job.rice_init << 8), p1 = p0;
  // one sample: both moduli as they stand, then the adaptation (the second parameter only when the first stage passes
  // the value on -- a select, the lanes of a wave walk different blocks)                          src/SLACoder.c:120-138
  auto step = [&](int32_t sample) -> uint32_t {
    const uint32_t v = fold_u32(sample);
    const uint32_t k0 = rice_k32(p0), k1 = rice_k32(p1);
    const uint32_t m0 = 1u << k0;
    const uint32_t n1 = rice_adapt32(p1, v - m0);
    p0 = rice_adapt32(p0, v);
    p1 = (v >= m0) ? n1 : p1;
    return k0 | (k1 << 8);
  };
  uint32_t s = 0;
  // up to the first sample whose residual and k addresses are both 16-byte aligned (block starts usually are)
  while (s < n && (((uintptr_t)(in + s) & 15u) != 0 || ((uintptr_t)(ko + s) & 15u) != 0) && s < 8) { ko[s] = (uint16_t)step(in[s]); s++; }
  if ((((uintptr_t)(in + s) & 15u) == 0) && (((uintptr_t)(ko + s) & 15u) == 0)) {
    for (; s + 8 <= n; s += 8) {
      const int4 a = *reinterpret_cast<const int4*>(in + s);          // a lane reads its own line: 16 bytes per access,
      const int4 b = *reinterpret_cast<const int4*>(in + s + 4);      // not 4, and one 16-byte store for 8 samples
      uint4 o;
      o.x = step(a.x); o.x |= step(a.y) << 16;
      o.y = step(a.z); o.y |= step(a.w) << 16;
      o.z = step(b.x); o.z |= step(b.y) << 16;
      o.w = step(b.z); o.w |= step(b.w) << 16;
      *reinterpret_cast<uint4*>(ko + s) = o;
    }
  }
  for (; s < n; s++) { ko[s] = (uint16_t)step(in[s]); }
}

// ---------------------------------------------------------------------------------------------
// k_rice_k2: the same walk as a two-lane pipeline, for files with few (block, channel) jobs -- where k_rice_k's duration
// is ONE job's serial walk (~105 ns per sample: a ten-second clip waits 0.43 ms for it with the chip empty).
// What is serial in the walk is only the two recurrences p0' = adapt(p0, v) and p1' = v >= 2^k0 ? adapt(p1, v - 2^k0) : p1;
// everything around them is a function of one sample: the code terms c = 9 (code << 8) split into c >> 7 and (c & 127) + 64,
// the exponents k = rice_k(p), the comparison.  So, per batch of 64 samples of a job:
//   P1  all lanes, lane = sample: fold the residual, the first recurrence's two code terms -> LDS
//   S   lane A walks p0 over batch t while lane B walks p1 over batch t - 1 -- the SAME instruction stream (B's update is
//       conditional, A's condition is always true): q = p >> 7, r = p & 127, p' = 119 q + hi + ((119 r + lo) >> 7);
//       both leave the parameter AS IT STOOD before each sample in LDS
//   P2  all lanes: k0 = rice_k(p0), the condition v >= 2^k0 and the second recurrence's code terms of v - 2^k0 -> LDS
//   P3  all lanes, batch t - 1: k1 = rice_k(p1), k0 | k1 << 8 -> global memory
// Eight jobs per wave (sixteen lanes in S).  Same values as k_rice_k, sample for sample (tests/test_gpu_pack.py on mixed
// waves, test_rice_walk_kernels_agree and every byte comparison of the suite: the pack stage chooses by the number of jobs).
// ---------------------------------------------------------------------------------------------
#define RK2_JOBS 8
// (Rows of 65 entries: in S sixteen lanes walk sixteen different rows in lock-step.  With rows of 64 every lane's operand sat on
// the same banks -- a 16-way conflict on each read, 8-way on each store: 6.0 conflict cycles per LDS instruction,
// profiles/r3_sq_counters_c2.csv.  Now row j of in_a starts at bank 2 j, of in_b at 16 + 2 j; of p0 at j, of p1 at 8 + j.)
struct rk2_lds {
  uint32_t in_a[RK2_JOBS][65][2];      // first recurrence: c >> 7, ((c & 127) + 64) | 1 << 8
  uint32_t in_b[RK2_JOBS][65][2];      // second recurrence: the same of v - 2^k0, bit 8 = the update happens
  uint32_t p0[RK2_JOBS][65], p1[RK2_JOBS][65];      // the parameters before each sample
  uint32_t v[RK2_JOBS][64];            // folded residual
  uint32_t k0[2][RK2_JOBS][64];        // first exponent, kept for one more step (the second one is a batch behind)
};

__global__ __launch_bounds__(256)
void k_rice_k2(const int32_t* __restrict__ res, uint64_t stride, const sla_hip_rice_job* __restrict__ jobs,
               uint32_t num_jobs, uint16_t* __restrict__ kk)
{
  __shared__ rk2_lds s_all[4];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  rk2_lds& L = s_all[wv];
  const uint32_t wave = blockIdx.x * 4 + wv;
  // lane l holds the fields of the wave's job l & 7; a phase that works on job j fetches them with a shuffle
  const uint32_t jb = wave * RK2_JOBS + (lane & 7u);
  const bool have = (jb < num_jobs);
  const sla_hip_rice_job job = jobs[have ? jb : 0];
  const uint32_t my_n = (have && job.golomb_m == 0) ? job.blk_len : 0u;          // fixed-parameter mode: stateless, nothing to walk
  const uint64_t my_off = (uint64_t)job.channel * stride + job.blk_off;
  const uint32_t nmax = umax_wave(my_n);
  const uint32_t nb = (nmax + 63u) / 64u;
  // the sixteen walking lanes: lane 2 j is A of job j, lane 2 j + 1 its B
  const uint32_t js = (lane >> 1) & 7u, role = lane & 1u;
  uint32_t p = (uint32_t)__shfl((int)(uint32_t)(job.rice_init << 8), (int)js);
  // the eight jobs' lengths and plane offsets as wave-uniform values (scalar registers), fetched once
  uint32_t n_of[RK2_JOBS]; uint64_t off_of[RK2_JOBS];
#pragma unroll
  for (int j = 0; j < RK2_JOBS; j++) {
    n_of[j] = (uint32_t)__builtin_amdgcn_readlane((int)my_n, j);
    off_of[j] = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(my_off >> 32), j) << 32)
              | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)my_off, j);
  }
  // residuals travel one batch ahead of their use: batch t + 1 is requested before the walk over batch t starts
  int32_t ahead[RK2_JOBS];
#pragma unroll
  for (int j = 0; j < RK2_JOBS; j++) { ahead[j] = (lane < n_of[j]) ? res[off_of[j] + lane] : 0; }
  for (uint32_t t = 0; t <= nb; t++) {
    if (t < nb) {
      // ---- P1: batch t of every job ----
#pragma unroll
      for (int j = 0; j < RK2_JOBS; j++) {
        const uint32_t v = fold_u32(ahead[j]);
        const uint32_t c = 9u * (v << 8);
        L.in_a[j][lane][0] = c >> 7; L.in_a[j][lane][1] = ((c & 127u) + 64u) | 256u;
        L.v[j][lane] = v;
      }
#pragma unroll
      for (int j = 0; j < RK2_JOBS; j++) {
        const uint32_t sidx = (t + 1u) * 64u + lane;
        ahead[j] = (sidx < n_of[j]) ? res[off_of[j] + sidx] : 0;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- S: A on batch t, B on batch t - 1 ----
    if (lane < 2 * RK2_JOBS && (role ? (t >= 1u) : (t < nb))) {
      const uint32_t (*in)[2] = role ? L.in_b[js] : L.in_a[js];
      uint32_t* pout = role ? L.p1[js] : L.p0[js];
#pragma unroll 1
      for (uint32_t i0 = 0; i0 < 64; i0 += 8) {
        uint32_t hi[8], lo[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { hi[u] = in[i0 + u][0]; lo[u] = in[i0 + u][1]; }      // eight steps' operands requested at once
#pragma unroll
        for (int u = 0; u < 8; u++) {
          pout[i0 + u] = p;
          const uint32_t q = p >> 7, r = p & 127u;
          const uint32_t np = 119u * q + hi[u] + ((119u * r + (lo[u] & 255u)) >> 7);
          p = (lo[u] & 256u) ? np : p;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (t < nb) {
      // ---- P2: batch t ----
#pragma unroll
      for (uint32_t j = 0; j < RK2_JOBS; j++) {
        const uint32_t k0 = rice_k32(L.p0[j][lane]);
        const uint32_t v = L.v[j][lane], m0 = 1u << k0;
        const uint32_t c = 9u * ((v - m0) << 8);
        L.in_b[j][lane][0] = c >> 7; L.in_b[j][lane][1] = ((c & 127u) + 64u) | ((v >= m0) ? 256u : 0u);
        L.k0[t & 1u][j][lane] = k0;
      }
    }
    if (t >= 1u) {
      // ---- P3: batch t - 1 ----
#pragma unroll
      for (int j = 0; j < RK2_JOBS; j++) {
        const uint32_t sidx = (t - 1u) * 64u + lane;
        const uint32_t k1 = rice_k32(L.p1[j][lane]);
        if (sidx < n_of[j]) { kk[off_of[j] + sidx] = (uint16_t)(L.k0[(t - 1u) & 1u][j][lane] | (k1 << 8)); }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// total body bits of every (block, channel): one wave per job, lanes stride over the samples
__global__ __launch_bounds__(256)
void k_rice_bits(const int32_t* __restrict__ res, uint64_t stride, const sla_hip_rice_job* __restrict__ jobs,
                 uint32_t num_jobs, const uint16_t* __restrict__ kk, uint64_t* __restrict__ chan_bits)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= num_jobs) { return; }
  const sla_hip_rice_job job = jobs[j];
  const int32_t* in = res + (uint64_t)job.channel * stride + job.blk_off;
  const uint16_t* ki = kk + (uint64_t)job.channel * stride + job.blk_off;
  uint64_t bits = 0;
  if (job.golomb_m != 0) {
    for (uint32_t s = lane; s < job.blk_len; s += 64) { bits += golomb_len(fold_u32(in[s]), job.golomb_m); }
  } else {
    for (uint32_t s = lane; s < job.blk_len; s += 64) {
      const uint32_t k = ki[s];
      bits += rrice_len(fold_u32(in[s]), k & 0xFF, k >> 8);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)bits, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(bits >> 32), off);
    bits += ((uint64_t)hi << 32) | lo;
  }
  if (lane == 0) { chan_bits[j] = bits; }
}

// OR `len` (1..33; 33 = the side field of a 32-bit mid/side RAW block, its top bit clear) bits of `val` into the image, the first bit landing at absolute bit `pos` (MSB-first)
__device__ __forceinline__ void put_piece(uint32_t* __restrict__ img, uint64_t pos, uint32_t val, uint32_t len)
{
  const uint64_t w = pos >> 5;
  const uint32_t sh = (uint32_t)(pos & 31);
  const uint64_t v64 = ((uint64_t)val << (64 - len)) >> sh;          // bit 63 = first bit of word w
  const uint32_t hi = (uint32_t)(v64 >> 32), lo = (uint32_t)v64;
  if (hi) { atomicOr(&img[w], __builtin_bswap32(hi)); }
  if (lo) { atomicOr(&img[w + 1], __builtin_bswap32(lo)); }
}

__global__ __launch_bounds__(256)
void k_rice_write(const int32_t* __restrict__ res, const int32_t* __restrict__ pcm, uint64_t stride,
                  const uint16_t* __restrict__ kk, const sla_hip_pack_block* __restrict__ blocks,
                  const uint8_t* __restrict__ headers, uint32_t num_channels, uint32_t raw_shift, uint32_t mid_side,
                  uint32_t* __restrict__ img)
{
  __shared__ uint32_t s_wave[4];
  __shared__ uint64_t s_base;
  const sla_hip_pack_block b = blocks[blockIdx.x];
  const uint32_t C = num_channels, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // header bytes (sync, size/crc placeholders, sample count, type, per-channel fields), packed by the host
  for (uint32_t t = threadIdx.x; t < b.header_bytes; t += blockDim.x) {
    const uint64_t at = b.out_off + t;
    atomicOr(&img[at >> 2], (uint32_t)headers[b.header_off + t] << (8 * (at & 3)));
  }
  if (b.type == 1) { return; }                                         // SILENT: header only
  if (threadIdx.x == 0) { s_base = (b.out_off + b.header_bytes) * 8ull; }
  __syncthreads();
  const uint32_t total = b.num_samples * C;
  for (uint32_t e0 = 0; e0 < total; e0 += 256) {
    const uint32_t e = e0 + threadIdx.x;
    uint32_t len = 0, v = 0, k0 = 0, k1 = 0, m = 0;
    if (e < total) {
      const uint32_t s = e / C, c = e - s * C;
      if (b.type == 2) {                                               // RAW: fixed width per channel
        int32_t x;
        if (!mid_side) { x = pcm[(uint64_t)c * stride + b.blk_off + s] >> raw_shift; }
        else {
          const int32_t l = pcm[b.blk_off + s] >> raw_shift, r = pcm[stride + b.blk_off + s] >> raw_shift;
          x = (c == 0) ? ((int32_t)((uint32_t)l + (uint32_t)r) >> 1) : (int32_t)((uint32_t)l - (uint32_t)r);
        }
        v = fold_u32(x);
        len = b.raw_bits + ((c == 1 && mid_side) ? 1u : 0u);
      } else {
        v = fold_u32(res[(uint64_t)c * stride + b.blk_off + s]);
        m = b.golomb_m[c];
        if (m != 0) { len = golomb_len(v, m); }
        else {
          const uint32_t k = kk[(uint64_t)c * stride + b.blk_off + s];
          k0 = k & 0xFF; k1 = k >> 8;
          len = rrice_len(v, k0, k1);
        }
      }
    }
    // exclusive prefix sum of `len` over the 256 elements of the tile
    uint32_t inc = len;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(inc, off); if (lane >= (uint32_t)off) { inc += o; } }
    if (lane == 63) { s_wave[wv] = inc; }
    __syncthreads();
    uint32_t wave_base = 0, tile_total = 0;
    for (uint32_t w = 0; w < 4; w++) { const uint32_t t = s_wave[w]; wave_base += (w < wv) ? t : 0u; tile_total += t; }
    const uint64_t pos = s_base + wave_base + (inc - len);
    if (e < total) {
      if (b.type == 2) {
        if (len > 0) { put_piece(img, pos, (len >= 32) ? v : (v & ((1u << len) - 1u)), len); }
      } else if (m != 0) {                                             // Golomb: zeros(q) 1 payload
        const uint32_t q = v / m, r = v - q * m;
        uint32_t nb, pay;
        if ((m & (m - 1u)) == 0) { nb = ceil_log2_u32(m); pay = r; }
        else { const uint32_t bb = ceil_log2_u32(m), cut = (1u << bb) - m; if (r < cut) { nb = bb - 1; pay = r; } else { nb = bb; pay = r + cut; } }
        put_piece(img, pos + q, (1u << nb) | pay, nb + 1);
      } else if (v < (1u << k0)) {                                     // stage 0: 1 rest
        put_piece(img, pos, (1u << k0) | v, k0 + 1);
      } else {
        const uint32_t vv = v - (1u << k0), q = 1u + (vv >> k1), rest = vv & ((1u << k1) - 1u);
        if (q < 16u) {
          put_piece(img, pos + q, (1u << k1) | rest, k1 + 1);
        } else {                                                       // zeros(16) 1 gamma(q-16) rest
          const uint32_t g = q - 16u;
          put_piece(img, pos + 16, 1u, 1);
          uint64_t at = pos + 17;
          if (g == 0) { put_piece(img, at, 1u, 1); at += 1; }
          else { const uint32_t nd = ceil_log2_u32(g + 2u); put_piece(img, at + nd - 1, g + 1u, nd); at += 2 * nd - 1; }
          if (k1 > 0) { put_piece(img, at, rest, k1); }
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) { s_base += tile_total; }
    __syncthreads();
  }
}

// one wave per block (4 blocks per workgroup): slice-parallel CRC16, see sla_crc_dev.h
__global__ __launch_bounds__(256)
void k_block_crc(const sla_hip_pack_block* __restrict__ blocks, uint32_t num_blocks, uint32_t* __restrict__ img)
{
  __shared__ uint16_t table[256];
  crc16_build_table(table);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= num_blocks) { return; }
  const sla_hip_pack_block b = blocks[j];
  const uint32_t crc = crc16_wave((const uint8_t*)img, b.out_off + 8, b.out_off + b.out_bytes, table, lane);
  if (lane != 0) { return; }
  // size field = bytes after sync + size (32 bit, big endian), then the CRC (16 bit)
  const uint32_t sz = b.out_bytes - 6;
  const uint8_t patch[6] = { (uint8_t)(sz >> 24), (uint8_t)(sz >> 16), (uint8_t)(sz >> 8), (uint8_t)sz,
                             (uint8_t)(crc >> 8), (uint8_t)crc };
  for (uint32_t t = 0; t < 6; t++) {
    const uint64_t at = b.out_off + 2 + t;
    atomicOr(&img[at >> 2], (uint32_t)patch[t] << (8 * (at & 3)));
  }
}

#define RICE_K2_MAX_JOBS 32768u
extern "C" int sla_hip_launch_rice_len(const int32_t* d_residual, uint64_t plane_stride, const sla_hip_rice_job* d_jobs,
                                       uint32_t num_jobs, uint16_t* d_kk, uint64_t* d_chan_bits, sla_hip_stream_t stream)
{
  if (d_residual == nullptr || d_jobs == nullptr || d_kk == nullptr || d_chan_bits == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_jobs == 0) { return 0; }
  /* few jobs: the two-lane pipeline (k_rice_k2), whose walk per sample is a third of k_rice_k's; many: one lane per job,
   * a quarter of the instructions per job and sample.  tuning().rice_lanes: 1 / 2 force one or the other */
  const uint32_t rl = tuning().rice_lanes;
  if (rl == 2 || (rl == 0 && num_jobs <= RICE_K2_MAX_JOBS)) {
    hipLaunchKernelGGL(k_rice_k2, dim3((num_jobs + 4 * RK2_JOBS - 1) / (4 * RK2_JOBS)), dim3(256), 0, (hipStream_t)stream, d_residual, plane_stride,
                       d_jobs, num_jobs, d_kk);
  } else {
    hipLaunchKernelGGL(k_rice_k, dim3((num_jobs + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_residual, plane_stride,
                       d_jobs, num_jobs, d_kk);
  }
  hipLaunchKernelGGL(k_rice_bits, dim3((num_jobs + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_residual, plane_stride,
                     d_jobs, num_jobs, d_kk, d_chan_bits);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_rice_write(const int32_t* d_residual, const int32_t* d_pcm, uint64_t plane_stride,
                                         const uint16_t* d_kk, const sla_hip_pack_block* d_blocks, uint32_t num_blocks,
                                         const uint8_t* d_headers, uint32_t num_channels, uint32_t raw_shift,
                                         uint32_t mid_side, uint32_t* d_image, sla_hip_stream_t stream)
{
  if (d_residual == nullptr || d_pcm == nullptr || d_kk == nullptr || d_blocks == nullptr || d_headers == nullptr || d_image == nullptr) {
    return SLA_APIRESULT_INVALID_ARGUMENT;
  }
  if (num_channels == 0 || num_channels > 8 || raw_shift > 31) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_blocks == 0) { return 0; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rice_write, dim3(num_blocks), dim3(256), 0, st, d_residual, d_pcm, plane_stride, d_kk, d_blocks,
                     d_headers, num_channels, raw_shift, mid_side, d_image);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { return hip_rc(e); }
  hipLaunchKernelGGL(k_block_crc, dim3((num_blocks + 3) / 4), dim3(256), 0, st, d_blocks, num_blocks, d_image);
  return hip_rc(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// k_unpack16: PCIe-side helper of SLAEncoder_EncodeWhole.  Input of <= 16 significant bits crosses the
// bus as int16 (the API's left-justified int32 has 16 zero low bits, checked on the host) and is
// re-expanded to the planar int32 layout every kernel reads.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_unpack16(const int16_t* __restrict__ in, int32_t* __restrict__ out, uint64_t count)
{
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 4 <= count) {
    const short4 v = *reinterpret_cast<const short4*>(in + i);
    int32_t* o = out + i;
    o[0] = (int32_t)v.x << 16; o[1] = (int32_t)v.y << 16; o[2] = (int32_t)v.z << 16; o[3] = (int32_t)v.w << 16;
  } else {
    for (uint64_t k = i; k < count; k++) { out[k] = (int32_t)in[k] << 16; }
  }
}

// k_unpack24: the same for input of <= 24 significant bits that crossed the bus as three bytes per sample (option
// "upload24"): four samples = three 32-bit words.
__global__ __launch_bounds__(256)
void k_unpack24(const uint32_t* __restrict__ in, int32_t* __restrict__ out, uint64_t count)
{
  const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;      // group of four samples
  const uint64_t i = q * 4;
  if (i + 4 <= count) {
    const uint32_t w0 = in[3 * q], w1 = in[3 * q + 1], w2 = in[3 * q + 2];
    int32_t* o = out + i;
    o[0] = (int32_t)(w0 << 8);
    o[1] = (int32_t)(((w0 >> 24) | (w1 << 8)) << 8);
    o[2] = (int32_t)(((w1 >> 16) | (w2 << 16)) << 8);
    o[3] = (int32_t)((w2 >> 8) << 8);
  } else if (i < count) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(in);
    for (uint64_t k = i; k < count; k++) { out[k] = (int32_t)(((uint32_t)b[3 * k] << 8) | ((uint32_t)b[3 * k + 1] << 16) | ((uint32_t)b[3 * k + 2] << 24)); }
  }
}

extern "C" int sla_hip_launch_unpack24(const uint8_t* d_in, int32_t* d_out, uint64_t count, sla_hip_stream_t stream)
{
  if (d_in == nullptr || d_out == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (count == 0) { return 0; }
  const uint64_t threads = (count + 3) / 4;
  hipLaunchKernelGGL(k_unpack24, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)d_in, d_out, count);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_unpack16(const int16_t* d_in, int32_t* d_out, uint64_t count, sla_hip_stream_t stream)
{
  if (d_in == nullptr || d_out == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (count == 0) { return 0; }
  const uint64_t threads = (count + 3) / 4;
  hipLaunchKernelGGL(k_unpack16, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_in, d_out, count);
  return hip_rc(hipGetLastError());
}
