// kernels/search.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): partition search: k_acf_tiles / k_acf_tiles_lds (tile sums), k_acf_blocks (chosen blocks, any order), k_search_finish, k_search_cert, k_plan
// ---------------------------------------------------------------------------------------------
// Exact partition search (see include/sla_hip.h): k_acf_tiles + k_search_finish.
//
// k_acf_tiles: one wave per (group, 1024-sample tile).  A lane owns 4 consecutive samples m[0..3]; the
// partner values x[m+lag] of lag block 4k..4k+3 are the 4-sample runs of lanes t+k and t+k+1, which
// arrive by a one-lane DPP shift per block -- 16 FMAs per 8 shifted dwords.  The last NB lanes
// of a pass only supply partners (their own multipliers are zero), so a pass advances (64-NB)*4
// samples; all passes' samples are requested before the first one is used.  Partners beyond the
// group's window are zero, partners beyond the tile are not: P[lag] holds every pair whose FIRST sample
// lies in the tile, X[lag] the ones among them whose second sample lies beyond it (a candidate ending
// with this tile has to give them back).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double shl1_f64(double v)       // lane t <- lane t+1, lane 63 <- 0
{
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130 /* wave_shl:1 */, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)        // all source lanes valid for the row permutations used
{
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// sum over the 64 lanes, valid in every lane (order of the additions is free: callers' sums are exact).
// In-row steps are DPP moves; the four row totals travel through SGPRs (ds_bpermute measured ~8x dearer).
__device__ __forceinline__ double wave_sum_f64(double v)
{
  v += dpp_f64<0xB1>(v);        // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);        // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);       // row_half_mirror
  v += dpp_f64<0x140>(v);       // row_mirror
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const double r0 = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
  const double r1 = __hiloint2double(__builtin_amdgcn_readlane(hi, 16), __builtin_amdgcn_readlane(lo, 16));
  const double r2 = __hiloint2double(__builtin_amdgcn_readlane(hi, 32), __builtin_amdgcn_readlane(lo, 32));
  const double r3 = __hiloint2double(__builtin_amdgcn_readlane(hi, 48), __builtin_amdgcn_readlane(lo, 48));
  return (r0 + r1) + (r2 + r3);
}

// Sums over the 64 lanes of M values per lane at once (M = 16, 32, 64; callers pad with zeros): a butterfly that halves
// the number of live values at every step -- a lane keeps the half selected by one of its lane-number bits and hands
// the other half to the partner that differs in that bit -- so the whole job costs M - 1 exchange-and-add operations
// instead of M separate 6-step wave sums.  The first (widest) steps use the cheap in-row DPP exchanges (xor 1, xor 2,
// xor 8 = rotate by 8 inside a row of 16), the narrow ones ds_swizzle / bpermute.  On return lane L holds the total of
// value `index` (every index < M exactly once among the lanes `writer` marks).  Callers' sums are exact or certified
// for any order of the additions.
__device__ __forceinline__ double swz_f64_xor4(double v)
{
  return __hiloint2double(__builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x101F), __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x101F));
}
__device__ __forceinline__ double swz_f64_xor16(double v)
{
  return __hiloint2double(__builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x401F), __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x401F));
}
__device__ __forceinline__ double shfl_f64_xor32(double v)
{
  return __hiloint2double(__shfl_xor(__double2hiint(v), 32), __shfl_xor(__double2loint(v), 32));
}
template <int STEP>
__device__ __forceinline__ double lane_exchange(double v)       // partner = lane ^ {1, 2, 8, 4, 16, 32}[STEP]
{
  if (STEP == 0) { return dpp_f64<0xB1>(v); }
  if (STEP == 1) { return dpp_f64<0x4E>(v); }
  if (STEP == 2) { return dpp_f64<0x128>(v); }                  // row_ror:8
  if (STEP == 3) { return swz_f64_xor4(v); }
  if (STEP == 4) { return swz_f64_xor16(v); }
  return shfl_f64_xor32(v);
}
template <int M, int STEP>
__device__ __forceinline__ void transpose_step(double (&v)[M], uint32_t lane)
{
  constexpr int K = M >> STEP;                                  // live values before this step
  constexpr uint32_t BIT = (STEP == 0) ? 1u : (STEP == 1) ? 2u : (STEP == 2) ? 8u : (STEP == 3) ? 4u : (STEP == 4) ? 16u : 32u;
  const bool up = (lane & BIT) != 0;
  if (K >= 2) {
#pragma unroll
    for (int j = 0; j < K / 2; j++) {
      const double lo = v[j], hi = v[j + K / 2];
      const double send = up ? lo : hi, keep = up ? hi : lo;
      v[j] = keep + lane_exchange<STEP>(send);
    }
  } else {
    v[0] += lane_exchange<STEP>(v[0]);                          // one value left: plain sum over the remaining lane bits
  }
}
template <int M>
__device__ __forceinline__ double wave_transpose_sum(double (&v)[M], uint32_t lane, uint32_t& index, bool& writer)
{
  transpose_step<M, 0>(v, lane); transpose_step<M, 1>(v, lane); transpose_step<M, 2>(v, lane);
  transpose_step<M, 3>(v, lane); transpose_step<M, 4>(v, lane); transpose_step<M, 5>(v, lane);
  const uint32_t b0 = lane & 1u, b1 = (lane >> 1) & 1u, b2 = (lane >> 2) & 1u, b3 = (lane >> 3) & 1u, b4 = (lane >> 4) & 1u, b5 = (lane >> 5) & 1u;
  // step k keeps the half selected by its bit: the bits spell the index from the top (M/2, M/4, ..)
  static_assert(M == 64 || M == 32 || M == 16 || M == 4 || M == 1, "wave_transpose_sum: 1, 4, 16, 32 or 64 values per lane");
  if (M == 1) { index = 0; writer = (lane == 0u); }       // nothing to hand over: six plain exchange-and-adds, lane 0's total is the one a piece of 4 gives its value 0
  else if (M == 64) { index = b0 * 32 + b1 * 16 + b3 * 8 + b2 * 4 + b4 * 2 + b5; writer = true; }
  else if (M == 32) { index = b0 * 16 + b1 * 8 + b3 * 4 + b2 * 2 + b4; writer = (b5 == 0); }
  else if (M == 16) { index = b0 * 8 + b1 * 4 + b3 * 2 + b2; writer = (b4 == 0 && b5 == 0); }
  else { index = b0 * 2 + b1; writer = (lane < 4u); }
  return v[0];
}

// The totals over the 64 lanes of LAGS = 4 NB accumulators per lane, stored to dst[lag] for lag < limit.  The butterfly takes
// a power of two of values and costs about one exchange-and-add per value: 36 lags padded to 64 paid for 63 of them (and the
// epilogue was a third of k_acf_tiles_lds' issue slots: it runs once per 1024-sample tile); cut into pieces of 32, 16 and 4
// values they pay 32 + 7 (36 lags: C3 tile sums 1.41 -> 1.35 ms) and 17 + 7 (20 lags); 52 lags as 32 + 17 + 7 measured SLOWER
// than the padded 63 (C5-240 s 1.36 -> 1.43 ms: three butterflies' worth of live registers in a kernel that already spills) and stay padded.
template <int M, int FIRST, int LAGS>
__device__ __forceinline__ void acf_reduce_piece(const double (&acc)[LAGS], uint32_t lane, double* __restrict__ dst, uint32_t limit)
{
  double tv[M];
#pragma unroll
  for (int i = 0; i < M; i++) { tv[i] = (FIRST + i < LAGS) ? acc[(FIRST + i < LAGS) ? FIRST + i : 0] : 0.0; }
  uint32_t index; bool writer;
  const double total = wave_transpose_sum<M>(tv, lane, index, writer);
  if (writer && FIRST + index < (uint32_t)LAGS && FIRST + index < limit) { dst[FIRST + index] = total; }
}
// TOP <= LAGS accumulators are live (see acf_tile_fma): TOP = LAGS - 3 leaves one value behind the first piece, which is summed on
// its own -- the same additions in the same order as its place in a piece of 4, so the total is the same double.
template <int LAGS, int TOP>
__device__ __forceinline__ void acf_reduce_store(const double (&acc)[TOP], uint32_t lane, double* __restrict__ dst, uint32_t limit)
{
  if constexpr (LAGS == 36 && TOP == 36) { acf_reduce_piece<32, 0>(acc, lane, dst, limit); acf_reduce_piece<4, 32>(acc, lane, dst, limit); }
  else if constexpr (LAGS == 36 && TOP == 33) { acf_reduce_piece<32, 0>(acc, lane, dst, limit); acf_reduce_piece<1, 32>(acc, lane, dst, limit); }
  else if constexpr (LAGS == 20 && TOP == 20) { acf_reduce_piece<16, 0>(acc, lane, dst, limit); acf_reduce_piece<4, 16>(acc, lane, dst, limit); }
  else if constexpr (LAGS == 20 && TOP == 17) { acf_reduce_piece<16, 0>(acc, lane, dst, limit); acf_reduce_piece<1, 16>(acc, lane, dst, limit); }
  else { acf_reduce_piece<(LAGS <= 16) ? 16 : (LAGS <= 32) ? 32 : 64, 0>(acc, lane, dst, limit); }
}

typedef int32_t i32x4_u __attribute__((ext_vector_type(4), aligned(4)));

// 4 consecutive raw samples of one plane, zero from `limit` on
__device__ __forceinline__ void load4_raw(const int32_t* __restrict__ plane, uint64_t base, uint32_t idx, uint32_t limit, int32_t (&v)[4])
{
  if (idx + 3 < limit) {
    const i32x4_u t = *(const i32x4_u*)(plane + base + idx);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++) { v[q] = (idx + q < limit) ? plane[base + idx + q] : 0; }
  }
}

// ---------------------------------------------------------------------------------------------
// The sliding dot products of a 256-sample tile, partners from LDS: lane t owns x[4t .. 4t+3] and pairs every one of them
// with the `lag` samples BEHIND it -- r[lag] = sum x[m] x[m - lag] -- so a tile only needs the samples in front of it, which
// the tile before has already staged, and the loads of the next tile can travel while this one is multiplied.  For the lag
// block 4k .. 4k+3 a lane needs x[4(t-k) - 3 .. 4(t-k) + 3].  The samples lie in LDS as 16-byte pairs, even pairs
// (x[4i], x[4i+1]) in E and odd pairs (x[4i+2], x[4i+3]) in O, slot HL + i for the tile's own pair i and slots [0, HL) for
// the HL = NB + 1 pairs in front of the tile: consecutive lanes read consecutive 16-byte slots (no bank conflicts), two
// ds_read_b128 per 16 FMAs.  (The first form of these kernels moved the partners from lane to lane by DPP: 16 moves per
// 16 FMAs, the last NB lanes of a pass only supplied partners, and nothing was in flight while a pass computed.)
// ---------------------------------------------------------------------------------------------
// TOP: the number of lags that have a reader (lag < TOP <= 4 NB; the BASELINE orders 16 / 32 / 48 need 17 / 33 / 49 of the 20 / 36 / 52).
// A lag at or above TOP is not computed, and a pair that only such lags touch is not read: with TOP = 4 NB - 3 the last block
// is 4 FMAs on pairs the block before it has already loaded.  The live lags' chains are the ones of the full form.
template <int NB, int TOP>
__device__ __forceinline__ void acf_tile_fma(const double (&own)[4], const double2* __restrict__ E, const double2* __restrict__ O,
                                             uint32_t lane, double (&acc)[TOP])
{
  static_assert(TOP > 4 * (NB - 1) && TOP <= 4 * NB, "acf_tile_fma: the last lag block holds the top lag");
  constexpr uint32_t HL = NB + 1;
  const double2* e = E + HL + lane;
  const double2* o = O + HL + lane;
  // block k works on P[i] = x[4(t-k) - 3 + i], i = 0 .. 6: (E[-k-1].y, O[-k-1].x, O[-k-1].y, E[-k].x, E[-k].y, O[-k].x, O[-k].y);
  // lag 4k + j reads P[3 - j ..]: the pair O[-k-1] from j = 1 on, E[-k-1] for j = 3 only
  double2 e0 = make_double2(own[0], own[1]), o0 = make_double2(own[2], own[3]);
  double2 e1 = e0, o1 = o0;
  if (TOP >= 4) { e1 = e[-1]; }
  if (TOP >= 2) { o1 = o[-1]; }
#pragma unroll
  for (int k = 0; k < NB; k++) {
    double2 e2 = e1, o2 = o1;
    if (4 * (k + 1) + 3 < TOP) { e2 = e[-k - 2]; }                          // the next block's new pairs travel under this block's FMAs
    if (4 * (k + 1) + 1 < TOP) { o2 = o[-k - 2]; }
    const double P[7] = {e1.y, o1.x, o1.y, e0.x, e0.y, o0.x, o0.y};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (4 * k + j < TOP) {
#pragma unroll
        for (int q = 0; q < 4; q++) { acc[4 * k + j] = __builtin_fma(own[q], P[q - j + 3], acc[4 * k + j]); }
      }
    }
    e0 = e1; o0 = o1; e1 = e2; o1 = o2;
  }
}

#define ACF_TILE 256u

// Small device words that have to be zero before the kernels BEHIND this one on the stream use them (counters, flags, the
// execution spans): cleared by the first workgroup of a kernel that is launched anyway instead of by a memset each -- a
// 4-byte hipMemsetAsync is a 4 us fill kernel plus a launch boundary, and a ten-minute mono file had five of them on its
// critical path (45 us of a 1.2 ms step).
struct clear_list { uint32_t* ptr[4]; uint32_t words[4]; };
__device__ __forceinline__ void clear_words(const clear_list& cl)
{
  if (blockIdx.x != 0) { return; }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    if (cl.ptr[r] != nullptr) { for (uint32_t i = threadIdx.x; i < cl.words[r]; i += blockDim.x) { cl.ptr[r][i] = 0u; } }
  }
}

// XT: the stride of tile_sums in tiles per group -- SLA_HIP_XTILES, or SLA_HIP_XTILES_FAR for windows of up to 64 tiles
// (sla_hip_launch_search_far).  A compile-time constant: nothing else of the kernel depends on it.
template <int NB, uint32_t XT = SLA_HIP_XTILES>
__global__ __launch_bounds__(256)
void k_acf_tiles(const int32_t* __restrict__ pcm, uint64_t stride, uint32_t ms,
                 const sla_hip_lpc_group* __restrict__ groups, uint32_t num_groups, uint32_t tiles_per_group,
                 double* __restrict__ tile_sums, clear_list cl, const uint32_t* early)
{
  constexpr uint32_t OL = 64 - NB;             // lanes of a pass that own samples
  constexpr uint32_t STEP = OL * 4, PASSES = (SLA_HIP_XTILE + STEP - 1) / STEP, LAGS = NB * 4;
  __shared__ double s_edge[4][2 * LAGS];       // x[t1-LAGS .. t1+LAGS) of each wave's tile end t1
  clear_words(cl);
  const bool stop = early_cancelled(early);    // (see k_acf_tiles_lds)
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t w = blockIdx.x * 4 + wv;
  const uint32_t gi = w / tiles_per_group, tile = w - gi * tiles_per_group;
  if (gi >= num_groups) { return; }
  const sla_hip_lpc_group g = groups[gi];
  const uint32_t N = g.num_samples, t0 = tile * SLA_HIP_XTILE;
  if (t0 >= N || stop) { return; }
  const uint32_t t1 = (t0 + SLA_HIP_XTILE < N) ? (t0 + SLA_HIP_XTILE) : N;
  const double scale = 4.656612873077392578125e-10;   // 2^-31, exact (same arithmetic as load_f64)

  int32_t ra[PASSES][4], rb[PASSES][4];
#pragma unroll
  for (uint32_t p = 0; p < PASSES; p++) {
    const uint32_t idx = t0 + p * STEP + 4 * lane;
    if (t0 + p * STEP < t1) {
      load4_raw(pcm + (ms ? 0 : (uint64_t)g.channel * stride), g.pcm_off, idx, N, ra[p]);
      if (ms) { load4_raw(pcm + stride, g.pcm_off, idx, N, rb[p]); }
    }
  }
  for (uint32_t i = lane; i < 2 * LAGS; i += 64) { s_edge[wv][i] = 0.0; }

  double acc[LAGS];
#pragma unroll
  for (int i = 0; i < (int)LAGS; i++) { acc[i] = 0.0; }
#pragma unroll
  for (uint32_t p = 0; p < PASSES; p++) {
    const uint32_t s0 = t0 + p * STEP;
    if (s0 < t1) {
      double cur[4], own[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t idx = s0 + 4 * lane + q;
        if (ms) {
          const double l = (double)ra[p][q] * scale, r = (double)rb[p][q] * scale;
          cur[q] = (g.channel == 0) ? ((l + r) / 2) : (l - r);
        } else {
          cur[q] = (double)ra[p][q] * scale;
        }
        own[q] = (lane < OL && idx < t1) ? cur[q] : 0.0;
        const int rel = (int)idx - ((int)t1 - (int)LAGS);
        if (rel >= 0 && rel < (int)(2 * LAGS)) { s_edge[wv][rel] = cur[q]; }
      }
#pragma unroll
      for (int k = 0; k < NB; k++) {
        double nxt[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { nxt[q] = shl1_f64(cur[q]); }
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const double partner = (q + j < 4) ? cur[q + j] : nxt[q + j - 4];
            acc[4 * k + j] = __builtin_fma(own[q], partner, acc[4 * k + j]);     // exact below the limit: fusing is free
          }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) { cur[q] = nxt[q]; }
      }
    }
  }
  double* dst = tile_sums + ((uint64_t)gi * XT + tile) * (2 * LAGS);
  {
    constexpr int M = (LAGS <= 16) ? 16 : (LAGS <= 32) ? 32 : 64;
    double tv[M];
#pragma unroll
    for (int i = 0; i < M; i++) { tv[i] = (i < (int)LAGS) ? acc[i] : 0.0; }
    uint32_t index; bool writer;
    const double total = wave_transpose_sum<M>(tv, lane, index, writer);
    if (writer && index < LAGS) { dst[index] = total; }
  }
  // pairs that straddle t1: lane = lag
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < LAGS) {
    double x = 0.0;
    const double* e = s_edge[wv];
#pragma unroll
    for (uint32_t j = 0; j + 1 < LAGS; j++) {                     // (as in k_acf_tiles_lds: all terms, the first `lane` kept)
      const double t = __builtin_fma(e[LAGS - lane + j], e[LAGS + j], x);
      x = (j < lane) ? t : x;
    }
    dst[LAGS + lane] = x;
  }
}

typedef double f64x2_u __attribute__((ext_vector_type(2), aligned(8)));

// A sample in the analysis' unit: raw * 2^-31; mid/side: l = a * 2^-31, r = b * 2^-31, mid = (l + r) / 2, side = l - r
// (src/SLAUtility.c:370-412).  Every step of that is exact in a double -- 32-bit integers, their 33-bit sum or difference, powers
// of two -- so the scale is applied once, to the sum: the same doubles from four operations instead of six.
__device__ __forceinline__ double mid_f64(int32_t a, int32_t b) { return ((double)a + (double)b) * 2.3283064365386962890625e-10; }       // 2^-32
__device__ __forceinline__ double side_f64(int32_t a, int32_t b) { return ((double)a - (double)b) * 4.656612873077392578125e-10; }      // 2^-31

// ---------------------------------------------------------------------------------------------
// k_acf_tiles_lds: the tile sums of k_acf_tiles with the partners from LDS (acf_tile_fma) instead of DPP moves -- for 52
// lags, where the moves are most of the instructions (C5: 489 -> see DESIGN us per launch; at 36 lags and below the DPP
// kernel is as fast or faster and stays).  acf_tile_fma pairs a sample with the ones BEHIND it; P_t[lag] needs the ones
// AHEAD (x[m] x[m + lag], m in the tile, m + lag anywhere in the window), so the tile is walked BACKWARDS: in reversed
// coordinates u = (t1 + 4 HL - 1) - m the partner m + lag is u - lag, the first 4 HL reversed samples -- the ones just
// above the tile's end -- are the front nobody owns, and the tile's own samples follow as up to four sub-tiles of 256.
// Samples below t0 count as zero (they are another tile's), samples from the window's end on are zero anyway.  X_t as
// in k_acf_tiles, from an edge buffer (filled from the values the wave stages anyway).  TOP: see acf_tile_fma.  (The first LDS port of round 3 kept the forward walk and re-defined P and X by
// the position of a pair's LATER sample; it was three times slower and was dropped.)
// ---------------------------------------------------------------------------------------------
template <int NB, int TOP, uint32_t XT = SLA_HIP_XTILES>      // XT: see k_acf_tiles
__global__ __launch_bounds__(256, (NB >= 13) ? 3 : 1)
void k_acf_tiles_lds(const int32_t* __restrict__ pcm, uint64_t stride, uint32_t ms,
                     const sla_hip_lpc_group* __restrict__ groups, uint32_t num_groups, uint32_t tiles_per_group,
                     double* __restrict__ tile_sums, clear_list cl, const uint32_t* early)
{
  constexpr uint32_t LAGS = NB * 4, HL = NB + 1;
  __shared__ double2 s_e[4][2][64 + HL], s_o[4][2][64 + HL];
  __shared__ double s_edge[4][2 * LAGS];       // x[t1-LAGS .. t1+LAGS) of each wave's tile end t1 (zero below t0)
  clear_words(cl);
  // started beside the prepass (sla_hip_launch_search_exact_early) and called off by it: every wave asks once, at its start --
  // the answer travels while the group's descriptor does and is looked at together with it, before any sample is loaded
  const bool stop = early_cancelled(early);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // the same in the wave's 64 lanes: the group, the tile and their bounds live in scalar registers
  const uint32_t w = blockIdx.x * 4 + wv;
  const uint32_t gi = w / tiles_per_group, tile = w - gi * tiles_per_group;
  if (gi >= num_groups) { return; }
  const sla_hip_lpc_group g = groups[gi];
  const uint32_t N = g.num_samples, t0 = tile * SLA_HIP_XTILE;
  if (t0 >= N || stop) { return; }
  const uint32_t t1 = (t0 + SLA_HIP_XTILE < N) ? (t0 + SLA_HIP_XTILE) : N;
  const double scale = 4.656612873077392578125e-10;   // 2^-31, exact (same arithmetic as load_f64)
  const int32_t* p0 = pcm + (ms ? 0 : (uint64_t)g.channel * stride) + g.pcm_off;
  const int32_t* p1 = pcm + stride + g.pcm_off;
  auto value = [&](int32_t a, int32_t b) -> double {
    if (ms) { return (g.channel == 0) ? mid_f64(a, b) : side_f64(a, b); }
    return (double)a * scale;
  };
  struct raw4 { int32_t a[4]; int32_t b[4]; };
  // a lane's four samples, reversed (the highest first).  Which of the three forms applies is the same for the whole wave:
  // one scalar branch per sub-tile, not both forms and a select per sample.
  auto values4 = [&](const raw4& c, double (&v)[4]) {
    if (!ms) {
#pragma unroll
      for (int q = 0; q < 4; q++) { v[q] = (double)c.a[3 - q] * scale; }
    } else if (g.channel == 0) {
#pragma unroll
      for (int q = 0; q < 4; q++) { v[q] = mid_f64(c.a[3 - q], c.b[3 - q]); }
    } else {
#pragma unroll
      for (int q = 0; q < 4; q++) { v[q] = side_f64(c.a[3 - q], c.b[3 - q]); }
    }
  };
  // four consecutive samples m0 .. m0+3 (m0 may be negative), zero outside [lo, N)
  auto fetch = [&](int64_t m0, uint32_t lo, raw4& r) {
#pragma unroll
    for (int q = 0; q < 4; q++) { r.a[q] = 0; r.b[q] = 0; }
    if (m0 >= (int64_t)lo && m0 + 3 < (int64_t)N) {
      const i32x4_u t = *(const i32x4_u*)(p0 + m0);
      r.a[0] = t.x; r.a[1] = t.y; r.a[2] = t.z; r.a[3] = t.w;
      if (ms) { const i32x4_u u = *(const i32x4_u*)(p1 + m0); r.b[0] = u.x; r.b[1] = u.y; r.b[2] = u.z; r.b[3] = u.w; }
    } else {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t m = m0 + q;
        if (m >= (int64_t)lo && m < (int64_t)N) { r.a[q] = p0[m]; if (ms) { r.b[q] = p1[m]; } }
      }
    }
  };
  // the same for a sub-tile that lies wholly inside [t0, t1): no guards (any alignment: i32x4_u is aligned(4))
  auto fetch_inside = [&](int64_t m0, raw4& r) {
    const i32x4_u t = *(const i32x4_u*)(p0 + m0);
    r.a[0] = t.x; r.a[1] = t.y; r.a[2] = t.z; r.a[3] = t.w;
#pragma unroll
    for (int q = 0; q < 4; q++) { r.b[q] = 0; }
    if (ms) { const i32x4_u u = *(const i32x4_u*)(p1 + m0); r.b[0] = u.x; r.b[1] = u.y; r.b[2] = u.z; r.b[3] = u.w; }
  };
  // sub-tile `sub` is [t1 - 256 (sub + 1), t1 - 256 sub): inside the tile when the tile has that many samples -- all four of a
  // whole tile, all but the lowest of a window's last one.  One scalar compare per sub-tile instead of 64-bit compares per lane.
  const uint32_t span = t1 - t0;
  auto fetch_sub = [&](uint32_t sub, raw4& r) {
    const int64_t m0 = (int64_t)t1 - (int64_t)ACF_TILE * (sub + 1) + 4 * (int64_t)(63 - lane);
    if ((sub + 1) * ACF_TILE <= span) { fetch_inside(m0, r); } else { fetch(m0, t0, r); }
  };
  // front: the 4 HL samples from t1 on, reversed; lane i < HL holds reversed positions 4 i .. 4 i + 3 = x[t1 + 4 HL - 1 - 4 i] downwards.
  // The edge buffer for X takes its upper half x[t1 .. t1 + LAGS) from them (lane 0's four lie beyond it) and its lower half from
  // the first sub-tile's own values below: nothing is loaded or converted a second time.
  if (lane < HL) {
    raw4 f;
    fetch((int64_t)t1 + 4 * (int64_t)HL - 4 - 4 * (int64_t)lane, t0, f);
    const double f0 = value(f.a[0], f.b[0]), f1 = value(f.a[1], f.b[1]), f2 = value(f.a[2], f.b[2]), f3 = value(f.a[3], f.b[3]);
    s_e[wv][0][lane] = make_double2(f3, f2);
    s_o[wv][0][lane] = make_double2(f1, f0);
    if (lane >= 1) {
      double* up = s_edge[wv] + LAGS + 4 * (HL - 1 - lane);
      up[0] = f0; up[1] = f1; up[2] = f2; up[3] = f3;
    }
  }
  double acc[TOP];
#pragma unroll
  for (int i = 0; i < TOP; i++) { acc[i] = 0.0; }
  const uint32_t nsub = (span + ACF_TILE - 1) / ACF_TILE;
  raw4 nxt;
  fetch_sub(0, nxt);
  double2* E = s_e[wv][0], * O = s_o[wv][0], * En = s_e[wv][1], * On = s_o[wv][1];      // this sub-tile's buffers and the next one's
  for (uint32_t sub = 0; sub < nsub; sub++) {
    const raw4 cur = nxt;
    if (sub + 1 < nsub) { fetch_sub(sub + 1, nxt); }
    double own[4];
    values4(cur, own);
    if (sub == 0 && lane < (uint32_t)NB) {     // x[t1 - LAGS .. t1): the top of the tile (zero below t0, as fetched)
      double* low = s_edge[wv] + LAGS - 4 - 4 * lane;
      low[0] = own[3]; low[1] = own[2]; low[2] = own[1]; low[3] = own[0];
    }
    E[HL + lane] = make_double2(own[0], own[1]);
    O[HL + lane] = make_double2(own[2], own[3]);
    if (lane >= 64 - HL) {                     // this sub-tile's last HL pairs are what the next one finds in front of it
      En[lane - (64 - HL)] = make_double2(own[0], own[1]);
      On[lane - (64 - HL)] = make_double2(own[2], own[3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    acf_tile_fma<NB, TOP>(own, E, O, lane, acc);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    { double2* t = E; E = En; En = t; t = O; O = On; On = t; }
  }
  // lag slots >= TOP of P and X are not written: k_search_finish and k_search_cert use lag <= order < TOP
  double* dst = tile_sums + ((uint64_t)gi * XT + tile) * (2 * LAGS);
  acf_reduce_store<(int)LAGS, TOP>(acc, lane, dst, TOP);
  // pairs that straddle t1: X[lag] = sum over j < lag of x[t1 - lag + j] x[t1 + j], a chain of dependent multiply-adds.
  if constexpr (TOP == 17 || TOP == 33) {
    // W = TOP - 1 lags (lag 0 has no such pair) times NP = 64 / W parts of the terms: all 64 lanes work, the chain is W / NP
    // long instead of W, and the parts meet in log2(NP) cross-lane additions.  Exact windows stay exact in any order; for
    // the others a sum takes at most W / NP + log2(NP) roundings instead of W (tests/acfmodel.py::roundings_tile).
    constexpr uint32_t W = TOP - 1, NP = 64 / W, CH = W / NP;
    const uint32_t lag = (lane & (W - 1)) + 1, part = lane / W;
    const double* e = s_edge[wv] + LAGS + part * CH;
    double x = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < CH; j++) {
      const double t = __builtin_fma(e[(int)j - (int)lag], e[j], x);      // (terms from `lag` on read on inside the buffer; not kept)
      x = (part * CH + j < lag) ? t : x;
    }
    if (NP == 4) { x += swz_f64_xor16(x); }
    x += shfl_f64_xor32(x);
    if (lane < W) { dst[LAGS + lag] = x; }
    if (lane == W) { dst[LAGS] = 0.0; }
  } else if (lane < (uint32_t)TOP) {
    // lane = lag.  Every lane runs all TOP - 1 terms and keeps the first `lane` of them (the same sums in the same order as a
    // loop to `lane`, whose trips -- two dependent LDS reads and a multiply-add each, ~130 cycles of latency, 35 of them --
    // held a wave's slot for as long as the tile's multiply-adds took to issue)
    double x = 0.0;
    const double* e = s_edge[wv];
    if constexpr (LAGS <= 36) {
#pragma unroll
      for (uint32_t j = 0; j + 1 < (uint32_t)TOP; j++) {
        const double t = __builtin_fma(e[LAGS - lane + j], e[LAGS + j], x);      // (j >= lane reads on inside the buffer; not kept)
        x = (j < lane) ? t : x;
      }
    } else {
      // (52 lags: the unrolled form measured slower, C5-240 s tile sums 1.36 -> 1.42 ms -- the kernel is short of registers as it is)
      for (uint32_t j = 0; j < lane; j++) { x = __builtin_fma(e[LAGS - lane + j], e[LAGS + j], x); }
    }
    dst[LAGS + lane] = x;
  }
}

// ---------------------------------------------------------------------------------------------
// k_acf_blocks: autocorrelation of the CHOSEN blocks' analysis windows in any summation order (the certified route of
// the block stage, see k_blocks_finish<.., true>).  One wave per (block, channel) walks the whole window in tiles of 256
// samples (acf_tile_fma); the accumulators live in registers across the tiles and are reduced over the lanes ONCE per
// block.  The samples are staged as the reference stages them -- x[s] = w[s]*in[s] - 0.96875 * w[s-1]*in[s-1]
// (src/SLAEncoder.c:505-515, 540-543, src/SLAPredictor.c:1803-1809): the previous windowed sample comes from the lane
// below (from the last lane of the tile before for lane 0).  Out: slot = { -, r[0..order] } and the quantiser's shift,
// exactly what k_lpc_blocks hands to k_blocks_finish -- but r[] is the exact sum only up to 4 ceil(N/256) + 6 roundings per
// lag, each worth 2^-53 * sum|x_i x_(i+lag)|: a lane's chain of four FMAs per tile and the six additions of the wave tree
// (tests/acfmodel.py::roundings_blocks; k_blocks_finish's delta budgets for them, tests/test_acf_error_model.py::
// test_block_budget_covers_both_sums; tests/test_gpu_acf_error.py holds the sums against exact ones through
// sla_hip_launch_acf_blocks).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double shr1_f64(double v, double first)       // lane t <- lane t-1, lane 0 <- first
{
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(first), __double2loint(v), 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(first), __double2hiint(v), 0x138, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

template <int NB, int TOP, bool MS>
__global__ __launch_bounds__(256, (NB >= 13) ? 3 : 1)      // 52 lags: 104 accumulator registers -- keep three waves per SIMD
void k_acf_blocks(const int32_t* __restrict__ pcm, uint64_t stride, uint32_t order,
                  const sla_hip_lpc_group* __restrict__ groups, uint32_t num_groups,
                  const double* __restrict__ window_pool, double* __restrict__ out, uint32_t* __restrict__ out_rshift,
                  unsigned long long* exec_span, uint32_t* __restrict__ zero_word, const uint32_t* __restrict__ dyn)
{
  constexpr uint32_t LAGS = NB * 4, HL = NB + 1;             // HL pairs in front of a tile: all that lags < 4 NB reach
  __shared__ double2 s_e[4][2][64 + HL], s_o[4][2][64 + HL];
  if (dyn != nullptr) { num_groups = (dyn[2] != 0u) ? 0u : (dyn[1] - dyn[3]); }      // (see k_blocks_finish)
  span_begin(exec_span);
  if (blockIdx.x == 0 && threadIdx.x == 0 && zero_word != nullptr) { *zero_word = 0u; }      // the fallback count k_blocks_finish appends to
  const uint32_t lane = threadIdx.x & 63;
  // the wave's number is the same in its 64 lanes: told so, the compiler keeps the group and its bounds in scalar registers and
  // branches on them.  Not at 52 lags, where every register move counts: C5-240 s block stage 0.70 ms without, 0.79 with
  // (0.78 before either; profiles/r7_acf_lags_ab.txt)
  const uint32_t wv = (NB < 13) ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : (threadIdx.x >> 6);
  const uint32_t gi = blockIdx.x * 4 + wv;
  if (gi >= num_groups) { span_end(exec_span); return; }
  const sla_hip_lpc_group g = groups[gi];
  const uint32_t N = g.num_samples;
  const double scale = 4.656612873077392578125e-10;   // 2^-31, exact
  const int32_t* p0 = pcm + (MS ? 0 : (uint64_t)g.channel * stride);
  const int32_t* p1 = pcm + stride;
  const double* win = window_pool + g.win_off;

  struct raw4 { int32_t a[4]; int32_t b[4]; double w[4]; };
  auto fetch = [&](uint32_t idx, raw4& r) {      // four consecutive raw samples (both channels for mid/side) and their window values; zero past the block
    load4_raw(p0, g.pcm_off, idx, N, r.a);
    if (MS) { load4_raw(p1, g.pcm_off, idx, N, r.b); }
#pragma unroll
    for (int q = 0; q < 4; q++) { r.w[q] = (idx + q < N) ? win[idx + q] : 0.0; }
  };
  // the same for a tile that lies wholly inside the block: no guards, the window as two 16-byte loads (any alignment:
  // i32x4_u is aligned(4), f64x2_u aligned(8))
  auto fetch_inside = [&](uint32_t idx, raw4& r) {
    const i32x4_u t = *(const i32x4_u*)(p0 + g.pcm_off + idx);
    r.a[0] = t.x; r.a[1] = t.y; r.a[2] = t.z; r.a[3] = t.w;
    if (MS) { const i32x4_u u = *(const i32x4_u*)(p1 + g.pcm_off + idx); r.b[0] = u.x; r.b[1] = u.y; r.b[2] = u.z; r.b[3] = u.w; }
    const f64x2_u w0 = *(const f64x2_u*)(win + idx), w1 = *(const f64x2_u*)(win + idx + 2);
    r.w[0] = w0.x; r.w[1] = w0.y; r.w[2] = w1.x; r.w[3] = w1.y;
  };

  double acc[TOP];
#pragma unroll
  for (int i = 0; i < TOP; i++) { acc[i] = 0.0; }
  uint32_t maxabs = 0;
  double carry = 0.0;                          // windowed sample right before the tile (0 before the block: src/SLAPredictor.c:1729-1738)
  if (lane < HL) { s_e[wv][0][lane] = make_double2(0.0, 0.0); s_o[wv][0][lane] = make_double2(0.0, 0.0); }      // nothing in front of the block
  raw4 nxt;
  if (ACF_TILE <= N) { fetch_inside(4 * lane, nxt); } else { fetch(4 * lane, nxt); }      // (one scalar compare per tile: N is the wave's)
  double2* E = s_e[wv][0], * O = s_o[wv][0], * En = s_e[wv][1], * On = s_o[wv][1];      // this tile's buffers and the next one's
  for (uint32_t s0 = 0; s0 < N; s0 += ACF_TILE) {
    const uint32_t idx = s0 + 4 * lane;
    const raw4 cur = nxt;
    if (s0 + 2 * ACF_TILE <= N) { fetch_inside(idx + ACF_TILE, nxt); }      // the next tile's samples travel while this one is multiplied
    else if (s0 + ACF_TILE < N) { fetch(idx + ACF_TILE, nxt); }
    double y[4], own[4];
    // (mid, side or plain: the same for the whole wave -- one scalar branch per tile, not both forms and a select per sample)
    auto staged = [&](int q, double v, int32_t iv) {
      y[q] = v * cur.w[q];
      const uint32_t a = (iv > 0) ? (uint32_t)iv : (0u - (uint32_t)iv);
      maxabs = (a > maxabs) ? a : maxabs;        // (samples past the block are zero)
    };
    if (!MS) {
#pragma unroll
      for (int q = 0; q < 4; q++) { staged(q, (double)cur.a[q] * scale, cur.a[q] >> g.int_shift); }
    } else if (g.channel == 0) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int32_t li = cur.a[q] >> g.int_shift, ri = cur.b[q] >> g.int_shift;
        staged(q, mid_f64(cur.a[q], cur.b[q]), (int32_t)((uint32_t)li + (uint32_t)ri) >> 1);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int32_t li = cur.a[q] >> g.int_shift, ri = cur.b[q] >> g.int_shift;
        staged(q, side_f64(cur.a[q], cur.b[q]), (int32_t)((uint32_t)li - (uint32_t)ri));
      }
    }
    const double below = shr1_f64(y[3], carry);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const double pv = (q == 0) ? below : y[q - 1];
      own[q] = y[q] - pv * 0.96875;
    }
    if (s0 + ACF_TILE > N) {                   // the block's last tile: nothing past its end
#pragma unroll
      for (int q = 0; q < 4; q++) { own[q] = (idx + q < N) ? own[q] : 0.0; }
    }
    carry = readlane_f64(y[3], 63);
    E[HL + lane] = make_double2(own[0], own[1]);
    O[HL + lane] = make_double2(own[2], own[3]);
    if (lane >= 64 - HL) {                     // this tile's last HL pairs are what the next tile finds in front of it
      En[lane - (64 - HL)] = make_double2(own[0], own[1]);
      On[lane - (64 - HL)] = make_double2(own[2], own[3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    acf_tile_fma<NB, TOP>(own, E, O, lane, acc);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    { double2* t = E; E = En; En = t; t = O; O = On; On = t; }
  }
  double* o = out + (uint64_t)g.slot_first * (order + 2);
  acf_reduce_store<(int)LAGS, TOP>(acc, lane, o + 1, order + 1);      // (order + 1 <= TOP: the launcher's choice)
  maxabs = umax_wave(maxabs);
  if (lane == 0) {
    const uint32_t l2c = (maxabs > 1) ? (32u - (uint32_t)__builtin_clz(maxabs - 1u)) : 0u;    // src/SLAUtility.c:677-696
    const uint32_t bitwidth = (maxabs > 0) ? (l2c + 1u) : 1u;
    out_rshift[g.slot_first] = (bitwidth > 16) ? (bitwidth - 16) : 0;
  }
  span_end(exec_span);
}

// k_search_finish: one wave per group.  r[lag] of candidate [start, end) = P of its tiles minus X of its
// last tile, then Levinson-Durbin per candidate exactly as in k_lpc.
//
// Windows over the exactness limit (loud material wider than 16 bits): the tile sums no longer equal the reference's
// serially rounded sums bit for bit -- but the search only has to deliver a PARTITION, and the reference's decision
// can be certified from sums that are merely close (cert > 0):
//   * the reference's r[lag] differs from the exact sum by at most n*2^-53 * sum|terms| <= n*2^-53 * r0 (recursive
//     summation of n exactly representable terms), ours by at most 64*2^-53 * (energy of the window).  The count, in
//     roundings a product passes through (tests/acfmodel.py::roundings_window): a tile's P takes 4 FMAs per 256-sample
//     sub-tile and the six additions of the wave tree, 22 (26 in k_acf_tiles<3>: five passes); the candidate's tiles are added
//     one after the other and the last tile's X subtracted, <= 16; X itself is a chain of up to `lag` <= 51 FMAs, but its
//     pairs straddle the candidate's end and their magnitudes add up to at most HALF the window's energy, <= 26: 64 in all
//     at 52 lags and 16 tiles (the 48 this comment used to state left X out: enough up to 33 live lags, not for 36 / 49 / 52;
//     tests/test_acf_error_model.py::test_search_budget_covers_the_tile_sums).  So the two Toeplitz matrices differ by a
//     symmetric Toeplitz matrix whose 2-norm is at most (2*order+1) * delta;
//   * the estimated code length of a candidate depends on its autocorrelation only through the final prediction
//     error e_p = r0 * prod(1 - k_j^2) = min over a, a_0 = 1, of a'Ra, which is monotone in the Loewner order:
//     R~ - d*I <= R_ref <= R~ + d*I  implies  e_p(R~ - d*I) <= e_p(R_ref) <= e_p(R~ + d*I);
//   * d = cert * (2*order+1) * delta with cert = 64: a factor 63 on top of the summation bounds for the rounding of the
//     Levinson recursion itself on either side (measured: the reference's estimate sits within 1e-4 of the bracket's
//     half width, tests/test_gpu_parity.py::test_search_certificate_brackets_the_reference).
// The candidate's slot then carries the tile-sum result plus, in parcor[0] (always 0 otherwise), the half width of
// log2(e_p); k_plan adds the widths up along the paths and only accepts a partition no width can change.  Anything
// else (not positive definite, not finite, cert <= 0) is flagged -- NaN in r[0], or an infinite width -- and redone
// as serial chains.
#define SEARCH_ACF_ROUNDINGS 64.0      // roundings per lag of the assembled tile sums, in units of 2^-53 * energy (see above)
#define XF_BATCH 64          // candidates one pass of the wave takes (at most)
#define XF_GROUPS 16         // groups one wave takes (at most)

// Final prediction error e_p of the Toeplitz system (r0, rc[1..order]) by the Schur recursion, both generator vectors
// in registers (static indices: the lower one moves down one slot per stage instead of the upper one moving up).
// Only used where nothing has to match the reference's Levinson recursion bit for bit (the certificate): fused
// multiply-adds, and NaN as soon as the recursion leaves the positive-definite range.
// FULL: order == P, known where the function is called -- every stage runs, nothing in the unrolled code is conditional and the
// compiler keeps both generators in registers without a single copy (with the stages conditional on m <= order every stage ended
// in a merge that pinned the vectors to fixed registers: one v_mov_b64 per pair of multiply-adds)
template <int P, bool FULL>
__device__ __forceinline__ double schur_error_impl(const double* __restrict__ rc, double r0, uint32_t order, double& growth)
{
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  double u[P + 1], v[P + 2];
#pragma unroll
  for (int i = 0; i <= P; i++) { const double x = ((uint32_t)i <= order && i >= 1) ? rc[i] : 0.0; u[i] = (i == 0) ? r0 : x; v[i] = x; }
  v[P + 1] = 0.0;
  bool bad = false;
  // stage m only has to renew the entries the later stages still read: u[0 .. P-m], v[0 .. P-m] (the result's cone of
  // dependence shrinks by one index per stage) -- half the multiply-adds of a square sweep; stages and indices are
  // unrolled, so both generator vectors stay in registers
#pragma unroll
  for (int m = 1; m <= P; m++) {
    if (FULL || (uint32_t)m <= order) {
      bad = bad || !(u[0] > 0.0);
      // k = -v[1] / u[0] by v_rcp_f64 and two Newton steps (~1e-16 relative) instead of the IEEE division's twenty-odd
      // instructions: this recursion only has to be ACCURATE -- its result is the end of a bracket whose width is at least
      // cert (2 order + 1) (n 2^-53) ~ 1e-9 of r0, and the caller widens the logarithms by 1e-11 on top -- not reproducible
      // bit for bit (nothing of it reaches the stream: DESIGN section 2a)
      double rc0 = __builtin_amdgcn_rcp(u[0]);
      rc0 = __builtin_fma(__builtin_fma(-u[0], rc0, 1.0), rc0, rc0);
      rc0 = __builtin_fma(__builtin_fma(-u[0], rc0, 1.0), rc0, rc0);
      const double k = -v[m] * rc0;
      bad = bad || !(fabs(k) < 1.0);
      growth *= 1.0 + fabs(k);                            // prod (1 + |k_j|) >= ||a||_1 of every predictor on the way
      // (entry i of the lower generator lives in v[i + m - 1] before stage m and in v[i + m] after it: the stage's "move down
      // by one" is a renaming, both updates are in place -- written as v[i] = f(v[i + 1]) every stage being conditional on
      // m <= order made the compiler materialise the move: 2271 v_mov_b64 beside 2489 multiply-adds in k_search_cert<48>)
#pragma unroll
      for (int i = 0; i <= P - m; i++) {
        const double t = v[i + m], ui = u[i];
        u[i] = __builtin_fma(k, t, ui);
        v[i + m] = __builtin_fma(k, ui, t);
      }
    }
  }
  return (!bad && u[0] > 0.0) ? u[0] : nan;
}

template <int P>
__device__ __forceinline__ double schur_error(const double* __restrict__ rc, double r0, uint32_t order, double& growth)
{
  if (order == (uint32_t)P) { return schur_error_impl<P, true>(rc, r0, order, growth); }      // (wave-uniform)
  return schur_error_impl<P, false>(rc, r0, order, growth);
}

// Levinson-Durbin of one candidate entirely in registers (the recursion of k_blocks_finish, src/SLAPredictor.c:253-328;
// stages and coefficient indices unrolled): o = { r0, parcor[0..order] }.  Same operations in the same order as
// levinson_out, which keeps its vectors in LDS.
template <int P>
__device__ __forceinline__ void levinson_regs(const double* __restrict__ rc, double* __restrict__ o, uint32_t order, uint32_t n)
{
  double r[P + 1], a[P + 1], par[P + 1];
#pragma unroll
  for (int i = 0; i <= P; i++) { r[i] = ((uint32_t)i <= order) ? rc[i] : 0.0; a[i] = 0.0; par[i] = 0.0; }
  if (!(n < order || fabs(r[0]) < (double)FLT_EPSILON)) {
    a[0] = 1.0;
    a[1] = -r[1] / r[0];
    par[1] = r[1] / r[0];
    double e = r[0] + r[1] * a[1];
#pragma unroll
    for (int d = 1; d < P; d++) {
      if ((uint32_t)d < order) {
        double gamma = 0.0;
#pragma unroll
        for (int i = 0; i <= d; i++) { gamma += a[i] * r[d + 1 - i]; }
        gamma /= (-e);
        e = (1.0 - gamma * gamma) * e;
        double nw[P + 1];
#pragma unroll
        for (int i = 1; i <= d; i++) { nw[i] = a[i] + gamma * a[d + 1 - i]; }
#pragma unroll
        for (int i = 1; i <= d; i++) { a[i] = nw[i]; }
        a[0] = 1.0 + gamma * 0.0;
        a[d + 1] = 0.0 + gamma * 1.0;
        par[d + 1] = -gamma;
      }
    }
  }
  o[0] = r[0];
#pragma unroll
  for (int j = 0; j <= P; j++) { if ((uint32_t)j <= order) { o[1 + j] = par[j]; } }
}

// One wave takes `gpw` groups at once when their candidates fit its lanes (a 4096-sample window has 10 candidates: six
// groups per wave instead of one wave with 10 busy lanes per group -- the kernel is bound by instruction issue); a
// group with more than 64 candidates (windows above 8192 samples) takes several passes of one wave.
// LDS: r[lanes][order+1] | a[lanes][order+2] | v[lanes][order+2] (work space of the exact windows' Levinson recursion)
template <int P, int mode>           // P >= order: 16, 32, 48, 64
__global__ __launch_bounds__(64)
void k_search_finish(uint32_t order, uint32_t lags, uint32_t gpw, uint32_t per,
                     const sla_hip_lpc_group* __restrict__ groups, uint32_t num_groups, const sla_hip_lpc_cand* __restrict__ cands,
                     const double* __restrict__ tile_sums, double* __restrict__ out, double exact_limit, double cert,
                     uint32_t* __restrict__ any_exact, const uint32_t* early)
{
  // early (may be NULL): the launch was queued before the host knew the file's offset_lshift -- exact_limit is the limit of
  // offset_lshift 0, the prepass has stored the shift meanwhile (the stream waited for it): a unit 2^lshift coarser, a
  // limit 4^lshift higher, exactly
  if (early != nullptr) {
    if (early_cancelled(early)) { return; }
    exact_limit = ldexp(exact_limit, 2 * (int)early[SLA_HIP_EARLY_LSHIFT]);
  }
  // any_exact (may be NULL): mode 1 sets the word when it meets a group below the limit, mode 2 returns at once while it is
  // still 0 -- loud material wider than 16 bits has no such group, and the mode-2 launch (70 KiB of LDS per workgroup) cost
  // 0.15 ms per C5-120 s launch just to find that out group by group
  if (mode == 2 && any_exact != nullptr && *any_exact == 0u) { return; }
  // mode 0: every group is known to be under the exactness limit (16-bit material): Levinson-Durbin in registers, LDS only
  // holds r; 1: only the groups over the limit (certificate; LDS only holds r: three times the waves per CU at order 48);
  // 2: only the groups below it, Levinson-Durbin with its vectors in LDS.  Material that may have both kinds is launched
  // as 1 + 2.
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ sla_hip_lpc_group s_g[XF_GROUPS];
  __shared__ double s_energy[XF_GROUPS];
  __shared__ uint32_t s_skip[XF_GROUPS];
  __shared__ uint32_t s_cmax;
  const uint32_t O1 = order + 1, O2 = order + 2;
  const uint32_t lane = threadIdx.x;
  const uint32_t g0 = blockIdx.x * gpw;
  const uint32_t ngr = (num_groups - g0 < gpw) ? (num_groups - g0) : gpw;
  const uint32_t slots = gpw * per;                  // lanes in use, <= 64
  if (lane == 0) { s_cmax = 0; }
  __syncthreads();
  if (lane < ngr) {
    const sla_hip_lpc_group g = groups[g0 + lane];
    const uint32_t ntiles = (g.num_samples + SLA_HIP_XTILE - 1) / SLA_HIP_XTILE;
    const double* ts = tile_sums + (uint64_t)(g0 + lane) * SLA_HIP_XTILES * 2 * lags;
    double energy = 0.0;
    for (uint32_t t = 0; t < ntiles; t++) { energy += ts[(uint64_t)t * 2 * lags]; }
    const bool skip = (mode == 1 && energy < exact_limit) || (mode == 2 && !(energy < exact_limit));
    if (mode == 1 && skip && any_exact != nullptr) { atomicOr(any_exact, 1u); }
    s_g[lane] = g; s_energy[lane] = energy; s_skip[lane] = skip ? 1u : 0u;
    if (!skip) { atomicMax(&s_cmax, g.cand_count); }
  }
  __syncthreads();
  const uint32_t cmax = s_cmax;
  double* r = lds;                                   // [slots][O1]
  double* av = lds + (size_t)slots * O1;             // [slots][O2]
  double* vv = av + (size_t)slots * O2;              // [slots][O2]
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  for (uint32_t c0 = 0; c0 < cmax; c0 += per) {
    const uint32_t total = ngr * per * O1;
    for (uint32_t q = lane; q < total; q += 64) {
      const uint32_t gl = q / (per * O1), rem = q - gl * per * O1;
      const uint32_t cl = rem / O1, lag = rem - cl * O1, ci = c0 + cl;
      if (ci < s_g[gl].cand_count && !s_skip[gl]) {
        const sla_hip_lpc_cand cd = cands[s_g[gl].cand_first + ci];
        const double* ts = tile_sums + (uint64_t)(g0 + gl) * SLA_HIP_XTILES * 2 * lags;
        const uint32_t end = cd.start + cd.len;
        double sum = 0.0;
        if (lag < cd.len) {
          const uint32_t tl = (end - 1) / SLA_HIP_XTILE;
          for (uint32_t t = cd.start / SLA_HIP_XTILE; t <= tl; t++) { sum += ts[(uint64_t)t * 2 * lags + lag]; }
          sum -= ts[(uint64_t)tl * 2 * lags + lags + lag];
        }
        r[(gl * per + cl) * O1 + lag] = sum;
      }
    }
    __syncthreads();
    const uint32_t gl = lane / per, cl = lane - gl * per, ci = c0 + cl;
    if (gl < ngr && ci < s_g[gl].cand_count && !s_skip[gl]) {
      const sla_hip_lpc_group g = s_g[gl];
      const double energy = s_energy[gl];
      const sla_hip_lpc_cand cd = cands[g.cand_first + ci];
      double* o = out + ((uint64_t)g.slot_first + ci) * O2;
      const double* rc = r + (size_t)lane * O1;
      if (energy < exact_limit) {
        if (mode == 0) { levinson_regs<P>(rc, o, order, cd.len); }
        else if (mode == 2) { levinson_regs<P>(rc, o, order, cd.len); }      // (registers, as mode 0: no work space in LDS)
      } else if (mode != 1 || !(cert > 0.0)) {
        o[0] = __longlong_as_double(0x7FF8000000000000ll);          // flagged: rerun as serial chains
      } else {
        // slot layout of a certified candidate: { r0, width, log2(e_p / r0), 0, .. }
        const double u = 1.1102230246251565e-16;                    // 2^-53
        const double r0 = rc[0];
        double w = inf, lg = 0.0;
        if (cd.len >= order && r0 > 2.0 * (double)FLT_EPSILON) {     // (the reference zeroes the coefficients below FLT_EPSILON, src/SLAPredictor.c:274)
          const double delta = ((double)cd.len * u) * r0 + (SEARCH_ACF_ROUNDINGS * u) * energy;
          const double d = cert * (double)(2 * order + 1) * delta;
          // one copy of the unrolled recursion, run for both ends of the bracket (inlined copies do not fit the instruction
          // cache).  The value handed to k_plan is the middle of the bracket in the logarithm, which is where the width applies:
          // log2(e_p) of the reference lies in [log2 e_lo, log2 e_hi] = mid +- w.  (A third recursion on the unshifted sums,
          // used as the middle until round 3, bought nothing but a third of this kernel's time.)
          double e2[2], g2[2] = {1.0, 1.0};
#pragma unroll 1
          for (int bk = 0; bk < 2; bk++) {
            const double rb = (bk == 0) ? (r0 + d) : (r0 - d);
            e2[bk] = (bk == 1 && !(r0 - d > (double)FLT_EPSILON)) ? __longlong_as_double(0x7FF8000000000000ll)
                                                                  : schur_error<P>(rc, rb, order, g2[bk]);
          }
          const double e_hi = e2[0], e_lo = e2[1];
          // The factor cert - 1 on top of the summation bounds is what is left for the rounding of the Levinson-Durbin
          // recursion itself (the reference's run): to first order it enters stage m through the sum num_m = sum a_i r_(m-i)
          // with at most (m + 2) 2^-53 ||a^(m-1)||_1 r0, i.e. like an autocorrelation error of that size -- covered by
          // d = cert (2 order + 1) delta as long as (order + 2) ||a||_1 2^-53 r0 <= (cert - 1) (2 order + 1) delta.
          // ||a||_1 <= prod (1 + |k_j|) of the more pessimistic bracket end; a candidate beyond that is not certified.
          const double gmax = fmax(g2[0], g2[1]);
          const bool rounding_covered = ((double)(order + 2) * gmax * u * r0 <= (cert - 1.0) * (double)(2 * order + 1) * delta);
          if (rounding_covered && e_lo > 0.0 && e_hi >= e_lo && e_hi < inf) {
            const double lh = log2(e_hi / r0), ll = log2(e_lo / r0);
            w = 0.5 * (lh - ll) * 1.000001 + 1e-11;               // (device log2: a few ulp)
            lg = 0.5 * (lh + ll);
          }
        }
        o[0] = r0;
        o[1] = (w == w) ? w : inf;
        o[2] = lg;
        for (uint32_t k = 2; k <= order; k++) { o[1 + k] = 0.0; }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// k_plan: the partition search's scalar tail on the device -- code-length estimate per candidate
// (src/SLAPredictor.c:416-468), adjacency matrix, Dijkstra (:1521-1581) -- so that the host does not have to
// fetch (order+2) doubles per candidate and evaluate 18 logarithms for each.  The reference's decisions hang
// on glibc's log(); the device's log() may differ from it in the last bits, so a result is only accepted
// when it provably does not depend on them: every comparison Dijkstra makes (minimum selection, relaxation)
// and every branch of the estimate must be decided by more than PLAN_MARGIN, which is > 1000x the largest
// possible discrepancy of a path cost (a few 1e-8 for 8 channels x 16384 samples x 16 edges).  Anything
// closer, non-finite or out of range is flagged and the host redoes that super-frame exactly as before.
// One wave per super-frame: lanes = candidates for the costs, lanes = nodes for the relaxation.
// ---------------------------------------------------------------------------------------------
#define PLAN_NODES 17            // 16384 / 1024 + 1
#define PLAN_MARGIN 1e-4
#define PLAN_BIG 16777216.0      // SLAOPTIMALENCODEESTIMATOR_DIJKSTRA_BIGWEIGHT

// `width`: half width of log2(e_p) the candidate carries (0: its sums are the reference's, bit for bit)
__device__ __forceinline__ double plan_code_length(double sumsq, uint32_t n, uint32_t bps, const double* __restrict__ parcor,
                                                   uint32_t order, double width, bool& sure)
{
  const double l2e = 1.4426950408889634;                        // src/SLAUtility.c:442-447
  double power = sumsq * ldexp(1.0, (int)(2 * (bps - 1)));
  if (fabs(power) <= (double)FLT_MIN) { if (width > 0.0) { sure = false; } return 0.0; }
  power = log(power) * l2e - log((double)n) * l2e;
  double gain = 0.0;
  if (width != 0.0) { gain = parcor[1]; }                        // certified candidate: log2(e_p / r0) itself (k_search_finish)
  else {
    // sum of log(1 - k^2), eight factors per logarithm: the value only has to agree with the host's sum of single
    // logarithms to within the margin every comparison must clear (1e-4 bytes; this differs by ~1e-11), and a product
    // of eight factors >= 2^-53 cannot underflow
    double prod = 1.0;
    for (uint32_t ord = 1; ord <= order; ord++) {
      const double f = 1.0 - parcor[ord] * parcor[ord];
      if (f < 0.0) { sure = false; }     // |k| > 1: the host's single logarithm is NaN; two such factors would cancel in the product
      prod *= f;
      if ((ord & 7u) == 0 || ord == order) { gain += log(prod) * l2e; prod = 1.0; }
    }
  }
  double len = 1.9426950408889634 + 0.5 * (power + gain);
  len /= 8;
  if (!(fabs(len) > 1e-9 + width / 16.0)) { sure = false; }     // too close to the clamp (or NaN)
  return (len <= 0) ? 0.125 : len;
}

__global__ __launch_bounds__(256)
void k_plan(const sla_hip_lpc_group* __restrict__ groups, uint32_t num_sf, uint32_t nch, uint32_t order, uint32_t bps,
            const sla_hip_lpc_cand* __restrict__ cands, double* __restrict__ lpc_out,
            uint32_t* __restrict__ parts, uint32_t* __restrict__ nparts, uint32_t* __restrict__ status, double margin,
            const uint32_t* early)
{
  __shared__ double s_adj[4][PLAN_NODES * PLAN_NODES];
  __shared__ uint32_t s_path[4][PLAN_NODES];
  if (early_cancelled(early)) { return; }
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t sf = blockIdx.x * 4 + wv;
  if (sf >= num_sf) { return; }
  const sla_hip_lpc_group g = groups[(uint64_t)sf * nch];       // channel 0 of the super-frame: all its candidates
  const uint32_t window = g.num_samples, O2 = order + 2;
  const uint32_t nodes = (window + SLA_HIP_XTILE - 1) / SLA_HIP_XTILE + 1;
  double* adj = s_adj[wv];
  bool sure = (nodes <= PLAN_NODES), inexact = false;
  double wmax = 0.0;
  if (!sure) { if (lane == 0) { status[sf] = 1; nparts[sf] = 0; } return; }
  for (uint32_t q = lane; q < nodes * nodes; q += 64) { adj[q] = PLAN_BIG; }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (uint32_t k = lane; k < g.cand_count; k += 64) {
    const sla_hip_lpc_cand cd = cands[g.cand_first + k];
    const uint32_t i = cd.start / SLA_HIP_XTILE, j = (uint32_t)(((uint64_t)cd.start + cd.len + SLA_HIP_XTILE - 1) / SLA_HIP_XTILE);
    double wedge = 0.0, est = 0.0;
    for (uint32_t ch = 0; ch < nch; ch++) {
      const double* o = lpc_out + ((uint64_t)g.slot_first + (uint64_t)ch * g.cand_count + k) * O2;
      const double width = o[1];                   // parcor[0]: 0, or the half width of log2(e_p) of a certified candidate
      est += cd.len * plan_code_length(o[0], cd.len, bps, o + 1, order, width, sure);
      wedge += cd.len * width / 16.0;              // bytes: length = n/8 * (const + log2(e_p * scale / n) / 2)
      if (width != 0.0) { inexact = true; }
    }
    if (!(wedge < PLAN_BIG / 2)) { sure = false; wedge = 0.0; }
    wmax = (wedge > wmax) ? wedge : wmax;
    est += 50.0;                                   // SLAOPTIMALENCODEESTIMATOR_ESTIMATE_BLOCK_SIZE
    est += 300.0;                                  // ..._LONGPATH_PENALTY
    if (!(fabs(est) < PLAN_BIG / 2)) { sure = false; }          // NaN (also the "rerun as serial chains" flag), inf, absurd
    // an edge of the lattice starts on the tile grid and ends on it or at the window's end; anything else is not the reference's edge
    const uint64_t end = (uint64_t)cd.start + cd.len;
    const bool on_grid = (cd.start % SLA_HIP_XTILE == 0) && end <= window && (end % SLA_HIP_XTILE == 0 || end == window);
    if (on_grid && i < nodes && j < nodes && j > i) { adj[i * nodes + j] = est; } else { sure = false; }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // a path has at most nodes-1 edges, each known to +-wmax: two path costs compare safely beyond 2*(nodes-1)*wmax
  for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(wmax, off); wmax = (o > wmax) ? o : wmax; }
  margin += 2.0 * (double)(nodes - 1) * wmax;
  inexact = (__ballot(inexact) != 0ull);
  // Dijkstra, lane = node: first-minimum selection, strict-improvement relaxation (as slai_shortest_path)
  double cost = (lane == 0) ? 0.0 : PLAN_BIG;
  bool done = false, reached = false;
  uint32_t pred = 0xFFFFFFFFu;
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  for (uint32_t round = 0; round <= nodes; round++) {
    const double v = (lane < nodes && !done && cost < PLAN_BIG) ? cost : inf;
    double best = v;
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(best, off); best = (o < best) ? o : best; }
    if (!(best < PLAN_BIG)) { break; }                         // the reference would not terminate: the host reports it
    const unsigned long long at = __ballot(v == best);
    const uint32_t cur = (uint32_t)__builtin_ctzll(at);
    double second = (lane == cur) ? inf : v;
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(second, off); second = (o < second) ? o : second; }
    if (second - best < margin) { sure = false; }
    if (cur == nodes - 1) { reached = true; break; }
    if (lane < nodes) {
      const double a = adj[cur * nodes + lane];
      if (a < PLAN_BIG) {                                      // BIG + x never improves a cost (all costs <= BIG)
        const double via = a + best;
        if (fabs(cost - via) < margin) { sure = false; }
        if (cost > via) { cost = via; pred = cur; }
      }
    }
    if (lane == cur) { done = true; }
  }
  if (lane < nodes) { s_path[wv][lane] = pred; }
  const bool all_sure = (__ballot(!sure) == 0ull);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane == 0) {
    uint32_t count = 0, node = nodes - 1;
    bool ok = reached && all_sure;
    while (ok && node != 0) {
      const uint32_t pr = s_path[wv][node];
      if (pr >= node) { ok = false; break; }
      count++; node = pr;
    }
    if (ok) {
      node = nodes - 1;
      for (uint32_t q = 0; q < count; q++) {
        const uint32_t pr = s_path[wv][node];
        const uint32_t off = pr * SLA_HIP_XTILE;
        uint32_t len = (node - pr) * SLA_HIP_XTILE;
        if (len > window - off) { len = window - off; }
        parts[(uint64_t)sf * PLAN_NODES + (count - q - 1)] = len;
        node = pr;
      }
    }
    nparts[sf] = ok ? count : 0;
    status[sf] = ok ? 0u : (inexact ? 2u : 1u);
    s_path[wv][0] = (ok || !inexact) ? 0u : 1u;
  }
  // a super-frame whose tile sums were only certified, not exact, and that did not certify: flag every candidate for
  // the serial-chain rerun (sla_hip_launch_lpc_rerun looks at r[0] of a group's first slot)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (s_path[wv][0] != 0u) {
    for (uint32_t q = lane; q < g.cand_count * nch; q += 64) {
      lpc_out[((uint64_t)g.slot_first + q) * O2] = __longlong_as_double(0x7FF8000000000000ll);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_search_cert: the certificate of the windows over the exactness limit (k_search_finish's mode 1) with its lanes full.
// A candidate needs TWO Schur recursions, one per end of the bracket; k_search_finish ran them one after the other in the
// candidate's lane, and an 8192-sample window has 36 candidates: 36 of 64 lanes busy, twice.  Here a lane is (candidate, end):
// a wave takes 32 consecutive candidate SLOTS of the launch -- the slots of the search groups are numbered consecutively,
// so a slot number is a flat candidate index and a wave's slots belong to at most two groups of equal size (it finds the
// group from the quotient and walks on where groups are shorter) -- lanes 0..31 run the end r0 + d, lanes 32..63 the end
// r0 - d of the same 32 candidates, the results meet through one cross-half exchange.  Same values as mode 1 (the same
// schur_error on the same operands); 14 KB of sums per wave become 12.5.
// ---------------------------------------------------------------------------------------------
#define XC_CANDS 32
#define XC_STAGE 1664u      /* doubles of tile sums a wave stages: 13 KB, twelve waves per CU */
template <int P>
__global__ __launch_bounds__(64)
void k_search_cert(uint32_t order, uint32_t lags, uint32_t per_max,
                   const sla_hip_lpc_group* __restrict__ groups, uint32_t num_groups, const sla_hip_lpc_cand* __restrict__ cands,
                   const double* __restrict__ tile_sums, double* __restrict__ out, double exact_limit, double cert,
                   uint32_t* __restrict__ any_exact, uint32_t stage_doubles, const uint32_t* early)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];          // the wave's tile sums, then r[XC_CANDS][order + 1] in their place
  if (early != nullptr) {                                                // (see k_search_finish)
    if (early_cancelled(early)) { return; }
    exact_limit = ldexp(exact_limit, 2 * (int)early[SLA_HIP_EARLY_LSHIFT]);
  }
  __shared__ uint32_t s_grp[XC_CANDS], s_start[XC_CANDS], s_len[XC_CANDS], s_live[XC_CANDS], s_nt[XC_CANDS];
  __shared__ double s_energy[XC_CANDS];
  const uint32_t O1 = order + 1, O2 = order + 2;
  const uint32_t lane = threadIdx.x, half = lane >> 5, cl = lane & 31u;
  const uint32_t slot0 = groups[0].slot_first;
  const uint32_t total = groups[num_groups - 1].slot_first + groups[num_groups - 1].cand_count - slot0;
  const uint32_t s = blockIdx.x * XC_CANDS + cl;                         // slot of this launch (both halves: the same candidate)
  if (blockIdx.x * XC_CANDS >= total) { return; }
  const uint32_t nvalid = (total - blockIdx.x * XC_CANDS < XC_CANDS) ? (total - blockIdx.x * XC_CANDS) : XC_CANDS;
  // ---- 1: whose candidate is this?  (Every global load of this prologue used to wait for the one before it -- the walk over
  // the groups, the energy tile by tile, every (candidate, lag) sum tile by tile: some eighty round trips to the L2 per wave
  // in front of a recursion that takes a few microseconds.  Now: four look-ahead loads at once, then the tile sums of the
  // wave's groups come into LDS in one sweep of independent loads, and everything else reads them there.)
  uint32_t g = 0, ci = 0, cand_first = 0, cand_count = 0, ntl = 0;
  if (half == 0 && s < total) {
    // no group has more than per_max candidates: group index >= s / per_max; walk on over shorter groups
    g = s / per_max;
    if (g >= num_groups) { g = num_groups - 1; }
    uint32_t ahead[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { const uint32_t j = (g + 1 + i < num_groups) ? g + 1 + i : num_groups - 1; ahead[i] = groups[j].slot_first - slot0; }
    uint32_t adv = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { if (g + 1 + i < num_groups && ahead[i] <= s) { adv = (uint32_t)i + 1; } }
    g += adv;
    if (g + 1 < num_groups && groups[g + 1].slot_first - slot0 <= s) {
      // many shorter groups in front (a batch of files, each ending in a short super-frame): bisect the rest
      uint32_t lo = g + 1, hi = num_groups - 1;
      while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (groups[mid].slot_first - slot0 <= s) { lo = mid; } else { hi = mid - 1; }
      }
      g = lo;
    }
    const sla_hip_lpc_group gr = groups[g];
    ci = s - (gr.slot_first - slot0);
    cand_first = gr.cand_first; cand_count = gr.cand_count;
    ntl = (gr.num_samples + SLA_HIP_XTILE - 1) / SLA_HIP_XTILE;
  }
  if (half == 0) { s_grp[cl] = g; s_nt[cl] = ntl; }
  __syncthreads();
  // ---- 2: the tile sums of the groups g_lo .. g_hi the wave's slots belong to (slots ascend with the groups)
  const uint32_t g_lo = s_grp[0], g_hi = s_grp[nvalid - 1];
  uint32_t max_nt = 1;
  for (uint32_t i = 0; i < nvalid; i++) { const uint32_t v = s_nt[i]; max_nt = (v > max_nt) ? v : max_nt; }
  const uint32_t S = max_nt * 2u * lags;                                 // doubles staged per group (whole tiles from tile 0)
  const uint32_t ng = g_hi - g_lo + 1u;
  const bool staged = (stage_doubles != 0u && (uint64_t)ng * S <= (uint64_t)stage_doubles);      // (0: the launcher chose the direct loads)
  if (staged) {
    for (uint32_t gg = 0; gg < ng; gg++) {
      const double* src = tile_sums + (uint64_t)(g_lo + gg) * SLA_HIP_XTILES * 2 * lags;
      double* dst = lds + (size_t)gg * S;
#pragma unroll 4
      for (uint32_t j = lane; j < S; j += 64) { dst[j] = src[j]; }
    }
  }
  __syncthreads();
  // ---- 3: energy, exact or not, the candidate's place.  (Tile sums of group gx, element idx: from the LDS copy, or -- a wave
  // whose groups do not fit -- from memory as before; two copies of the code, one address space each.)
  double* r = lds;
  constexpr int RPL = (XC_CANDS * (P + 1) + 63) / 64;
  double mine[RPL];
  auto gather = [&](auto staged_tag) {
  constexpr bool STG = decltype(staged_tag)::value;
  auto ts_at = [&](uint32_t gx, uint32_t idx) -> double {
    if constexpr (STG) { return lds[(size_t)(gx - g_lo) * S + idx]; }
    else { return tile_sums[(uint64_t)gx * SLA_HIP_XTILES * 2 * lags + idx]; }
  };
  if (half == 0) {
    uint32_t live = 0, start = 0, len = 0;
    double energy = 0.0;
    if (s < total && ci < cand_count) {
      for (uint32_t t = 0; t < ntl; t++) { energy += ts_at(g, t * 2 * lags); }
      if (energy < exact_limit) {
        if (any_exact != nullptr) { atomicOr(any_exact, 1u); }          // an exact window: the mode-2 launch behind this one takes it
      } else {
        const sla_hip_lpc_cand cd = cands[cand_first + ci];
        live = 1; start = cd.start; len = cd.len;
      }
    }
    s_start[cl] = start; s_len[cl] = len; s_live[cl] = live; s_energy[cl] = energy;
  }
  __syncthreads();
  // ---- 4: r[candidate][lag] = sum of P over its tiles - X of its last tile, gathered into registers first: r takes the place of
  // the staged sums
#pragma unroll
  for (int jj = 0; jj < RPL; jj++) {
    const uint32_t q = lane + 64u * (uint32_t)jj;
    double sum = 0.0;
    if (q < XC_CANDS * O1) {
      const uint32_t c2 = q / O1, lag = q - c2 * O1;
      if (s_live[c2]) {
        const uint32_t gx = s_grp[c2];
        const uint32_t st = s_start[c2], ln = s_len[c2], end = st + ln;
        if (lag < ln) {
          const uint32_t tl = (end - 1) / SLA_HIP_XTILE;
          for (uint32_t t = st / SLA_HIP_XTILE; t <= tl; t++) { sum += ts_at(gx, t * 2 * lags + lag); }
          sum -= ts_at(gx, tl * 2 * lags + lags + lag);
        }
      }
    }
    mine[jj] = sum;
  }
  };
  if (staged) { gather(std::true_type{}); } else { gather(std::false_type{}); }
  __syncthreads();
#pragma unroll
  for (int jj = 0; jj < RPL; jj++) {
    const uint32_t q = lane + 64u * (uint32_t)jj;
    if (q < XC_CANDS * O1 && s_live[q / O1]) { r[q] = mine[jj]; }
  }
  __syncthreads();
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const double u = 1.1102230246251565e-16;                              // 2^-53
  const bool live = (s_live[cl] != 0u);
  const double* rc = r + (size_t)cl * O1;
  const double r0 = live ? rc[0] : 1.0;
  const uint32_t len = s_len[cl];
  const bool valid = live && len >= order && r0 > 2.0 * (double)FLT_EPSILON;   // (the reference zeroes the coefficients below FLT_EPSILON, src/SLAPredictor.c:274)
  const double delta = ((double)len * u) * r0 + (SEARCH_ACF_ROUNDINGS * u) * s_energy[cl];
  const double d = cert * (double)(2 * order + 1) * delta;
  double e_mine = nan, g_mine = 1.0;
  if (valid) {
    const double rb = (half == 0) ? (r0 + d) : (r0 - d);
    if (half == 0 || r0 - d > (double)FLT_EPSILON) { e_mine = schur_error<P>(rc, rb, order, g_mine); }
  }
  // the other end of my candidate's bracket sits 32 lanes away
  const double e_other = __hiloint2double(__shfl_xor(__double2hiint(e_mine), 32), __shfl_xor(__double2loint(e_mine), 32));
  const double g_other = __hiloint2double(__shfl_xor(__double2hiint(g_mine), 32), __shfl_xor(__double2loint(g_mine), 32));
  if (live) {
    double* o = out + ((uint64_t)slot0 + s) * O2;
    if (half == 0) {
      // slot layout of a certified candidate: { r0, width, log2(e_p / r0), 0, .. }
      const double e_hi = e_mine, e_lo = e_other;
      double w = inf, lg = 0.0;
      if (valid) {
        // (the share of the bound left for the rounding of the reference's Levinson-Durbin run: see k_search_finish)
        const double gmax = fmax(g_mine, g_other);
        const bool rounding_covered = ((double)(order + 2) * gmax * u * r0 <= (cert - 1.0) * (double)(2 * order + 1) * delta);
        if (rounding_covered && e_lo > 0.0 && e_hi >= e_lo && e_hi < inf) {
          const double lh = log2(e_hi / r0), ll = log2(e_lo / r0);
          w = 0.5 * (lh - ll) * 1.000001 + 1e-11;                       // (device log2: a few ulp)
          lg = 0.5 * (lh + ll);
        }
      }
      o[0] = rc[0];
      o[1] = (w == w) ? w : inf;
      o[2] = lg;
    }
    // the rest of the slot is zero: the two lanes of the candidate share the stores
    for (uint32_t k = 2 + half; k <= order; k += 2) { o[1 + k] = 0.0; }
  }
}
