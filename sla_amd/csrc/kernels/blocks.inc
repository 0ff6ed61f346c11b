// kernels/blocks.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): k_lpc_blocks (exact chains of the chosen blocks, list mode), k_blocks_finish (Levinson-Durbin, quantiser, certificate, audit)
// ---------------------------------------------------------------------------------------------
// k_lpc_blocks: the chosen blocks (one candidate per group = the whole windowed block).
//
// A serial chain only has to be serial in its ADDITIONS: the terms c*(a+b) are independent.  So the work
// is split by role (512 threads).  Waves 2-7 ("producers") compute LB_K consecutive terms of every chain
// of the pack into an LDS tile, in the chain's own order (pairs i-major, then the leftover products; 0.0
// past the end, which leaves an accumulator untouched bit for bit); wave 0 owns one accumulator per
// (window, lag) and adds the previous tile -- half a ds_read_b128 and one v_add_f64 per step for up to 64
// chains at once; wave 1 does the same for the energy sums (two squares per step).  One barrier per tile,
// two tile buffers.  Measured on C2 (shader clock per workgroup of two 4096-sample windows): 265k ticks for
// the chains in k_lpc's one-lane-per-chain loop, 140k here; staging 62k -> 20k (straight-line batches);
// Levinson-Durbin + quantiser 60k -> 16k: it runs lane-parallel, one wave per window, lane j holds a[j]; the
// dot product is multiplied in parallel and summed in the reference's order through v_readlane; the
// reversed vector is a ds_bpermute.  The quantiser runs one lane per coefficient.
// LDS: x[pack][x_region] | terms[2][nch][LB_K+2] | sq[2][pack][2*LB_K] | r[pack][order+1]
// ---------------------------------------------------------------------------------------------
#define LB_K 24
#define LB_THREADS 512          // wave 0: lag accumulators, wave 1: energy accumulators, waves 2-7: term producers
#define LB_PRODUCERS (LB_THREADS - 128)
__device__ unsigned long long g_lpc_clk[8];   // SLA_HIP_LPC_CLK=1: shader-clock ticks per phase, summed over workgroups

__device__ __forceinline__ double readlane_f64(double v, int lane)      // lane must be wave-uniform
{
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// Stage one analysis window into LDS: x[s] = w[s]*in[s] - 0.96875 * w[s-1]*in[s-1] (src/SLAEncoder.c:505-515,
// 540-543, src/SLAPredictor.c:1803-1809) and return the wave's max |integer sample| (for the quantiser's
// shift).  MS is a template parameter so that the batch below is straight-line code: all its samples are
// requested before the first one is used (one memory latency per batch of 8, not per sample).
template <bool MS>
__device__ __forceinline__ uint32_t stage_window(const int32_t* __restrict__ pcm, uint64_t stride, const sla_hip_lpc_group& g,
                                                 const double* __restrict__ win, double* __restrict__ x, uint32_t tid)
{
  const double scale = 4.656612873077392578125e-10;   // 2^-31, exact
  const int32_t* p0 = pcm + (MS ? 0 : (uint64_t)g.channel * stride) + g.pcm_off;
  const int32_t* p1 = pcm + stride + g.pcm_off;        // right channel (MS only)
  uint32_t maxabs = 0;
  for (uint32_t base = 0; base < g.num_samples; base += LB_THREADS * 8) {
    int32_t l0[8], l1[8], r0[8], r1[8];
    double w0[8], w1[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const uint32_t s = base + u * LB_THREADS + tid;
      const bool in = (s < g.num_samples);
      const uint32_t sc = in ? s : 0, sp = (in && s > 0) ? (s - 1) : 0;
      l0[u] = p0[sc]; l1[u] = p0[sp];
      if (MS) { r0[u] = p1[sc]; r1[u] = p1[sp]; }
      w0[u] = win[sc]; w1[u] = win[sp];
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const uint32_t s = base + u * LB_THREADS + tid;
      if (s < g.num_samples) {
        double cur, prev;
        int32_t iv;
        if (MS) {
          // mid = (l+r)/2, side = l-r in double (src/SLAUtility.c:382-387); integers: (L+R)>>1, L-R on the shifted samples (:403-411)
          const double a = (double)l0[u] * scale, b = (double)r0[u] * scale, c = (double)l1[u] * scale, d = (double)r1[u] * scale;
          cur = (g.channel == 0) ? ((a + b) / 2) : (a - b);
          prev = (g.channel == 0) ? ((c + d) / 2) : (c - d);
          const int32_t li = l0[u] >> g.int_shift, ri = r0[u] >> g.int_shift;
          iv = (g.channel == 0) ? ((int32_t)((uint32_t)li + (uint32_t)ri) >> 1) : (int32_t)((uint32_t)li - (uint32_t)ri);
        } else {
          cur = (double)l0[u] * scale; prev = (double)l1[u] * scale;
          iv = l0[u] >> g.int_shift;
        }
        const double c = cur * w0[u];
        const double pv = (s > 0) ? (prev * w1[u]) : 0.0;
        x[s] = c - pv * 0.96875;
        const uint32_t a = (iv > 0) ? (uint32_t)iv : (0u - (uint32_t)iv);
        maxabs = (a > maxabs) ? a : maxabs;
      }
    }
  }
  return umax_wave(maxabs);
}

#define LB_ROW (LB_K + 2)     // terms of one chain and tile, padded: 16-byte aligned rows that spread over the banks

template <int S, int LBK>     // producer lanes per chain: 6 or 12; steps per tile: 24 or 48 (longer tiles pay for wide packs: fewer barriers, more operand reuse)
__device__ __forceinline__
void lpc_blocks_body(const int32_t* __restrict__ pcm, uint64_t stride, uint32_t ms, uint32_t order,
                  const sla_hip_lpc_group* __restrict__ groups, uint32_t num_groups, uint32_t pack,
                  const double* __restrict__ window_pool, double* __restrict__ out,
                  int32_t* __restrict__ out_code, int32_t* __restrict__ out_kint, uint32_t* __restrict__ out_rshift,
                  uint32_t x_region, uint32_t nch, uint32_t clk,
                  int32_t* __restrict__ lat_residual, uint32_t defer_levinson, uint32_t g0, const uint32_t* __restrict__ list)
{
  constexpr uint32_t Q = LBK / S;              // consecutive terms a producer lane makes per tile
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const unsigned long long t_start = clk ? clock64() : 0;
  __shared__ sla_hip_lpc_group s_g[LPC_MAX_PACK];
  __shared__ uint32_t s_maxabs[LPC_MAX_PACK];
  __shared__ uint32_t s_tiles;
  const uint32_t O1 = order + 1, O2 = order + 2;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t ng = (num_groups - g0 < pack) ? (num_groups - g0) : pack;
  if (tid < LPC_MAX_PACK) {
    if (tid < ng) { s_g[tid] = groups[(list != nullptr) ? list[g0 + tid] : (g0 + tid)]; }
    s_maxabs[tid] = 0;
  }
  if (tid == 0) { s_tiles = 0; }
  __syncthreads();
  double* terms = lds + (size_t)pack * x_region;            // [2][nch][(LBK + 2)]
  double* sq = terms + (size_t)2 * nch * (LBK + 2);            // [2][pack][2*LBK]
  double* r = sq + (size_t)2 * 2 * LBK * pack;             // [pack][O1]

  // ---- stage the windows: convert, mid/side, window, pre-emphasis (as k_lpc) -------------------------
  for (uint32_t k = 0; k < ng; k++) {
    const sla_hip_lpc_group g = s_g[k];
    const uint32_t maxabs = ms ? stage_window<true>(pcm, stride, g, window_pool + g.win_off, lds + (size_t)k * x_region, tid)
                               : stage_window<false>(pcm, stride, g, window_pool + g.win_off, lds + (size_t)k * x_region, tid);
    if (lane == 0) { atomicMax(&s_maxabs[k], maxabs); }
  }

  // ---- chain geometry: the consumer lane and the producer lanes of a chain derive the same numbers ------
  const uint32_t nchains = ng * order;
  const bool producer = (wv >= 2);
  const uint32_t pl = tid - 128;                            // producer lane number (valid when producer)
  const uint32_t ch = (wv == 0) ? lane : (producer ? (pl % nch) : 0xFFFFFFFFu);
  const uint32_t j = producer ? (pl / nch) : 0;             // which Q-term piece of the tile this producer lane makes
  const bool has_chain = (ch < nchains) && (!producer || j < (uint32_t)S);
  const uint32_t ck = has_chain ? (ch / order) : 0;
  const uint32_t lag = has_chain ? (1 + ch - ck * order) : 1;
  const uint32_t n = s_g[ck].num_samples;
  const uint32_t lag2 = lag << 1;
  const uint32_t grp = (has_chain && 3 * lag < n) ? (1 + (n - 3 * lag) / lag2) : 0;
  const uint32_t span = grp * lag2;
  const uint32_t npair = grp * lag;
  const uint32_t total = (has_chain && lag < n) ? (npair + (n - span - lag)) : 0;     // terms of this chain
  const double* xs = lds + (size_t)ck * x_region;
  {
    uint32_t need = (total + LBK - 1) / LBK;
    if (tid < ng) { const uint32_t e = (s_g[tid].num_samples + 2 * LBK - 1) / (2 * LBK); need = (e > need) ? e : need; }
    need = umax_wave(need);
    if (lane == 0) { atomicMax(&s_tiles, need); }
  }
  __syncthreads();
  const uint32_t ntiles = s_tiles;
  const unsigned long long t_staged = clk ? clock64() : 0;
  unsigned long long t_prod = 0, t_cons = 0;

  // producer position: term kk = tile*LBK + j*Q sits at (run pi, step pg) while it is a pair term
  uint32_t kk = j * Q;
  uint32_t pi = (grp != 0) ? (kk / grp) : 0, pg = (grp != 0) ? (kk - (kk / grp) * grp) : 0;
  uint32_t ppos = pi + pg * lag2;                           // sample index of a of that term
  // energy producer: lane e < 2*LBK*ng makes the square of sample tile*2*LBK + es of window ew
  const uint32_t nsq = 2 * LBK * ng;
  const uint32_t ew = pl / (2 * LBK), es = pl - ew * (2 * LBK);      // 2*LBK*LPC_MAX_PACK = 192 <= LB_PRODUCERS

  double acc = 0.0;
  for (uint32_t t = 0; t <= ntiles; t++) {
    const unsigned long long t_a = clk ? clock64() : 0;
    if (producer && t < ntiles) {
      // most tiles: every lane of this wave makes Q consecutive pair terms of one run -- no bookkeeping, and
      // b of one term is a of the next
      const bool plain = !has_chain || (kk + Q <= npair && pg + Q <= grp);
      if (__all(plain)) {
        if (has_chain) {
          double* dst = terms + ((size_t)(t & 1) * nch + ch) * (LBK + 2) + j * Q;
          const double* p = xs + ppos;
          double va[Q + 1], vc[Q];
#pragma unroll
          for (int q = 0; q < (int)Q; q++) { va[q] = p[q * lag2]; vc[q] = p[q * lag2 + lag]; }
          va[Q] = p[Q * lag2];
#pragma unroll
          for (int q = 0; q < (int)Q; q++) { dst[q] = vc[q] * (va[q] + va[q + 1]); }
        }
      } else if (has_chain) {
        double* dst = terms + ((size_t)(t & 1) * nch + ch) * (LBK + 2) + j * Q;
        uint32_t ii = pi, gg = pg, pos = ppos;
        uint32_t ia[Q]; bool pr[Q], vl[Q];
#pragma unroll
        for (int q = 0; q < (int)Q; q++) {
          const uint32_t kq = kk + q;
          pr[q] = (kq < npair); vl[q] = (kq < total);
          ia[q] = pr[q] ? pos : (vl[q] ? (span + (kq - npair)) : 0u);
          const bool wrap = (gg + 1 == grp);
          gg = wrap ? 0u : (gg + 1);
          ii += wrap ? 1u : 0u;
          pos = wrap ? ii : (pos + lag2);
        }
        double va[Q], vc[Q], vb[Q];
#pragma unroll
        for (int q = 0; q < (int)Q; q++) { va[q] = xs[ia[q]]; vc[q] = xs[ia[q] + lag]; vb[q] = xs[ia[q] + lag2]; }
#pragma unroll
        for (int q = 0; q < (int)Q; q++) {
          const double tv = vc[q] * (va[q] + (pr[q] ? vb[q] : 0.0));      // leftover products: c*a (a+0.0 == a up to the sign of zero, which a sum that starts at +0.0 cannot see)
          dst[q] = vl[q] ? tv : 0.0;
        }
      }
      if (has_chain) {
        kk += LBK;
        if (grp != 0) { pg += LBK; ppos += LBK * lag2; while (pg >= grp) { pg -= grp; pi++; ppos += 1 - span; } }
      }
      double* dq = sq + (size_t)(t & 1) * 2 * LBK * pack;
      if (pl < nsq) {
        const uint32_t idx = t * 2 * LBK + es;
        const double v = (idx < s_g[ew].num_samples) ? lds[(size_t)ew * x_region + idx] : 0.0;
        dq[ew * 2 * LBK + es] = v * v;
      }
    }
    const unsigned long long t_b = clk ? clock64() : 0;
    if (t >= 1) {
      if (wv == 0 && has_chain) {
        const double2* src = (const double2*)(terms + ((size_t)((t - 1) & 1) * nch + ch) * (LBK + 2));
        double2 v[LBK / 2];
#pragma unroll
        for (int q = 0; q < LBK / 2; q++) { v[q] = src[q]; }
        __builtin_amdgcn_sched_barrier(0);          // every load of the tile is in flight before the first add waits
#pragma unroll
        for (int q = 0; q < LBK / 2; q++) { acc += v[q].x; acc += v[q].y; }
      } else if (wv == 1 && lane < ng) {
        const double2* src = (const double2*)(sq + (size_t)((t - 1) & 1) * 2 * LBK * pack + lane * 2 * LBK);
        double2 v[LBK];
#pragma unroll
        for (int q = 0; q < LBK; q++) { v[q] = src[q]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < LBK; q++) { acc += v[q].x; acc += v[q].y; }
      }
    }
    if (clk) { const unsigned long long t_c = clock64(); t_prod += t_b - t_a; t_cons += t_c - t_b; }
    __syncthreads();
  }
  if (wv == 0 && has_chain) { r[ck * O1 + lag] = acc; }
  if (wv == 1 && lane < ng) { r[lane * O1] = acc; }
  __syncthreads();
  const unsigned long long t_chained = clk ? clock64() : 0;

  if (defer_levinson) {
    // the recursion and the quantiser run in k_blocks_finish (one LANE per window, everything in registers): this
    // workgroup only hands over r[0..order] (in the slot's parcor area) and the quantiser's shift
    if (wv < ng) {
      const sla_hip_lpc_group g = s_g[wv];
      double* o = out + (uint64_t)g.slot_first * O2;
      for (uint32_t i = lane; i <= order; i += 64) { o[1 + i] = r[wv * O1 + i]; }      // (order 64: r[64] has no lane of its own)
      if (lane == 0) {
        const uint32_t m = s_maxabs[wv];
        const uint32_t l2c = (m > 1) ? (32u - (uint32_t)__builtin_clz(m - 1u)) : 0u;    // src/SLAUtility.c:677-696
        const uint32_t bitwidth = (m > 0) ? (l2c + 1u) : 1u;
        out_rshift[g.slot_first] = (bitwidth > 16) ? (bitwidth - 16) : 0;
      }
    }
    return;
  }
  // ---- Levinson-Durbin, one wave per window, lane j = coefficient j   src/SLAPredictor.c:253-328 ------
  if (wv < ng) {
    const sla_hip_lpc_group g = s_g[wv];
    const uint64_t slot = g.slot_first;
    double* o = out + slot * O2;
    const double rc = (lane <= order) ? r[wv * O1 + lane] : 0.0;
    const double r0 = readlane_f64(rc, 0), r1 = readlane_f64(rc, 1);
    double par = 0.0;                               // lane j: parcor[j]
    if (!(g.num_samples < order || fabs(r0) < (double)FLT_EPSILON)) {
      const double a1 = -r1 / r0;
      double a = (lane == 0) ? 1.0 : ((lane == 1) ? a1 : 0.0);
      par = (lane == 1) ? (r1 / r0) : 0.0;
      double e = r0 + r1 * a1;
      for (uint32_t d = 1; d < order; d++) {
        const int src = (int)(d + 1) - (int)lane;                   // lanes 0..d read r[d+1-i] / a[d+1-i]
        const double rrev = __shfl(rc, src & 63);
        const double prod = a * rrev;
        double gamma = 0.0;
        for (uint32_t i = 0; i <= d; i++) { gamma += readlane_f64(prod, (int)i); }
        gamma /= (-e);
        e = (1.0 - gamma * gamma) * e;
        const double arev = __shfl(a, src & 63);
        const double v = (lane == 0) ? 0.0 : ((lane == d + 1) ? 1.0 : ((lane <= d) ? arev : 0.0));
        const double a_old = (lane == d + 1) ? 0.0 : a;
        a = a_old + gamma * v;
        par = (lane == d + 1) ? (-gamma) : par;
      }
    }
    if (lane <= order) { o[1 + lane] = par; }
    if (lane == 0) { o[0] = r0; }
    // coefficient quantiser, lane = coefficient                          src/SLAEncoder.c:567-589
    const uint32_t m = s_maxabs[wv];
    const uint32_t l2c = (m > 1) ? (32u - (uint32_t)__builtin_clz(m - 1u)) : 0u;    // src/SLAUtility.c:677-696
    const uint32_t bitwidth = (m > 0) ? (l2c + 1u) : 1u;
    const uint32_t rshift = (bitwidth > 16) ? (bitwidth - 16) : 0;
    if (lane == 0) { out_rshift[slot] = rshift; out_code[slot * O1] = 0; out_kint[slot * O1] = 0; }
    if (lane >= 1 && lane <= order) {
      const uint32_t qb = (lane < 4) ? 16 : 8;
      const int32_t lim = 1 << (qb - 1);
      const double kq = par * (double)lim;
      const double rk = (kq >= 0.0) ? floor(kq + 0.5) : -floor(-kq + 0.5);
      int32_t code = f64_to_i32_x86(rk);
      code = (code < -lim) ? -lim : code;
      code = (code > lim - 1) ? (lim - 1) : code;
      out_code[slot * O1 + lane] = code;
      out_kint[slot * O1 + lane] = (int32_t)((uint32_t)code << (16u - qb)) >> rshift;
    }
  }
  // ---- PARCOR lattice of the same blocks (k_lattice's wave-chunks), while their samples are still hot in L2 ----
  if (lat_residual != nullptr) {
    __threadfence();                                  // out_kint of this workgroup's slots: visible to its other waves
    __syncthreads();
    const uint32_t per = (SLA_WAVE - (order + LAT_T - 1) / LAT_T) * LAT_T;
    uint32_t first_chunk = 0;
    for (uint32_t k = 0; k < ng; k++) {
      const sla_hip_lpc_group g = s_g[k];
      const uint32_t nchunks = (g.num_samples + per - 1) / per;
      for (uint32_t cid = wv; cid < first_chunk + nchunks; cid += LB_THREADS / 64) {
        if (cid < first_chunk) { continue; }
        const uint32_t at = (cid - first_chunk) * per;
        lattice_chunk_wave(pcm, stride, ms, order, g.pcm_off, g.num_samples, at, (g.num_samples - at < per) ? (g.num_samples - at) : per,
                           g.channel, g.int_shift, out_kint + (uint64_t)g.slot_first * O1, lat_residual, lane);
      }
      first_chunk += nchunks;
    }
  }
  if (clk && lane == 0) {
    const unsigned long long t_end = clock64();
    if (wv == 0) {
      atomicAdd(&g_lpc_clk[0], t_staged - t_start); atomicAdd(&g_lpc_clk[1], t_chained - t_staged);
      atomicAdd(&g_lpc_clk[2], t_end - t_chained); atomicAdd(&g_lpc_clk[3], 1ull); atomicAdd(&g_lpc_clk[4], t_cons);
    }
    if (wv == 2) { atomicAdd(&g_lpc_clk[5], t_prod); }
    if (wv == 1) { atomicAdd(&g_lpc_clk[6], t_cons); }
  }
}

// list mode (list != NULL): the groups are list[0 .. *list_count) -- the blocks k_blocks_finish<.., true> could not
// certify -- and a fixed grid walks them (the count is only known on the device).
template <int S, int LBK>
__global__ __launch_bounds__(LB_THREADS)
void k_lpc_blocks(const int32_t* __restrict__ pcm, uint64_t stride, uint32_t ms, uint32_t order,
                  const sla_hip_lpc_group* __restrict__ groups, uint32_t num_groups, uint32_t pack,
                  const double* __restrict__ window_pool, double* __restrict__ out,
                  int32_t* __restrict__ out_code, int32_t* __restrict__ out_kint, uint32_t* __restrict__ out_rshift,
                  uint32_t x_region, uint32_t nch, uint32_t clk, unsigned long long* exec_span,
                  int32_t* __restrict__ lat_residual, uint32_t defer_levinson,
                  const uint32_t* __restrict__ list, const uint32_t* __restrict__ list_count)
{
  span_begin(exec_span);
  const uint32_t total = (list != nullptr) ? *list_count : num_groups;
  for (uint32_t g0 = blockIdx.x * pack; g0 < total; g0 += gridDim.x * pack) {
    lpc_blocks_body<S, LBK>(pcm, stride, ms, order, groups, total, pack, window_pool, out, out_code, out_kint, out_rshift,
                            x_region, nch, clk, lat_residual, defer_levinson, g0, list);
    __syncthreads();
  }
  span_end(exec_span);
}

// ---------------------------------------------------------------------------------------------
// k_blocks_finish: Levinson-Durbin (src/SLAPredictor.c:253-328) and the coefficient quantiser (src/SLAEncoder.c:567-589)
// of the chosen blocks, one LANE per (block, channel).  Inside k_lpc_blocks the recursion ran lane-parallel on one wave
// per window -- the sum gamma = sum a[i]*r[d+1-i] has to be added up in the reference's order, so it was (order^2)/2
// dependent v_readlane + v_add_f64 pairs while the other waves of the workgroup idled: 91 of 376 thousand cycles per
// C5 workgroup.  A lane that keeps a[] and r[] in registers does the same arithmetic, operation for operation, with no
// cross-lane traffic at all, and 64 windows share a wave; the loops are unrolled over the stage and the coefficient
// index so that every register index is static (the reversed vector v[i] = a[d+1-i] is just another register).
// In: slot = { -, r[0..order] } as k_lpc_blocks left it, rshift.  Out: slot = { r0, parcor[0..order] }, code, kint.
//
// CERT = true: r[] came from k_acf_blocks (any summation order), so the doubles are NOT the reference's bit for bit --
// but what reaches the bit stream are the quantised codes (16 bits for the first three coefficients, 8 bits for the
// rest, src/SLAEncoder.c:573-589) and the RAW decision (src/SLAEncoder.c:553-565).  Both are certified per block:
//   * |r_ref[j] - r[j]| <= delta = (n + max(64, 4 ceil(n/256) + 6)) * 2^-53 * r[0] (acf_blocks_budget).  Counted in roundings
//     a product passes through, each worth 2^-53 * sum|x_i x_(i+lag)| <= 2^-53 * r0 (tests/acfmodel.py derives the counts):
//     the reference's lag 0 is n squares added one after the other, n roundings; at a lag >= 1 it adds T terms c*(a+b) (two
//     roundings each) and leftover products, T + 1 <= n/2 + lag roundings.  k_acf_blocks keeps a lane's accumulators
//     across all tiles of the block, four FMAs per tile and lag, and runs the wave tree once: 4 ceil(n/256) + 6 (70 at
//     n = 4096, 262 at 16384; not the 48 this comment used to state).  Lag 0 is the tightest: n + 64 covers both sums only up to
//     n = 3584, hence the maximum.  tests/test_acf_error_model.py::test_block_budget_covers_both_sums checks the inequality for
//     every n <= 16384 and lag <= 51, tests/test_gpu_acf_error.py measures the kernel's sums against exact ones;
//   * to first order the reflection coefficient of stage m moves by
//        dk_m = -(B' dR A)/e + k_m (A' dR A)/e,   A = (1, a_1 .. a_(m-1), 0), B = A reversed, e = e_(m-1)
//     (the optimal predictors make the variation of A and B drop out: R A and R B vanish in the middle rows), hence
//        |dk_m| <= ||a^(m-1)||_1^2 * (1 + |k_m|) / e_(m-1) * max_j |dr_j|;
//   * the rounding of the recursion itself (the reference's run and this one) enters stage m through its sum
//     num_m = sum a_i r_(m-i), <= (m+2) 2^-53 ||a||_1 r0 per run: it is put through the same sensitivity;
//   * `safety` (16) multiplies the whole bound: tests/tools/cert_study.py and tests/test_gpu_cert.py measure the
//     largest |k - k_ref| at 0.6 % of the UNscaled bound over tones with noise floors down to -140 dB, music-like and
//     full-scale material at orders 16/32/48.
// A block is certified when every k_m * 2^(q-1) keeps its distance from the rounding boundaries (half-integers, and
// the two clip limits) and the estimated code length keeps its distance from the RAW threshold; everything else --
// non-finite values, |k| >= 1, r0 near FLT_EPSILON -- is flagged: its group index goes to fb_list and the exact kernels
// (k_lpc_blocks + k_blocks_finish<.., false> in list mode) redo it on the same stream.
// list mode (list != NULL): the groups to finish are list[0 .. *list_count).
// ---------------------------------------------------------------------------------------------
// roundings per lag the certificate allows the reference's sum and k_acf_blocks' together (see above; 256 = ACF_TILE)
__device__ __forceinline__ double acf_blocks_budget(uint32_t n)
{
  const uint32_t own = 4u * ((n + 255u) / 256u) + 6u;
  return (double)n + (double)((own > 64u) ? own : 64u);
}

template <int P, bool CERT>           // P >= order
__global__ __launch_bounds__(64, (P == 32 && CERT) ? 2 : 1)
void k_blocks_finish(const sla_hip_lpc_group* __restrict__ groups, uint32_t num_groups, uint32_t order,
                     double* __restrict__ out, int32_t* __restrict__ out_code, int32_t* __restrict__ out_kint,
                     const uint32_t* __restrict__ out_rshift,
                     const uint32_t* __restrict__ list, const uint32_t* __restrict__ list_count,
                     uint32_t* __restrict__ cert_flag, uint32_t* __restrict__ fb_list, uint32_t* __restrict__ fb_count,
                     double safety, uint32_t bps, const uint32_t* __restrict__ dyn = nullptr, uint32_t audit_every = 0u)
{
  // dyn: k_expand_scan's running numbers -- the launch was sized for the most groups the file can have, before the host
  // knew how many there are (see sla_hip_launch_lpc_blocks_cert)
  const uint32_t total = (list != nullptr) ? *list_count : ((dyn != nullptr) ? ((dyn[2] != 0u) ? 0u : (dyn[1] - dyn[3])) : num_groups);
  for (uint32_t li = blockIdx.x * 64 + threadIdx.x; li < total; li += gridDim.x * 64) {
  const uint32_t gi = (list != nullptr) ? list[li] : li;
  const uint32_t O1 = order + 1, O2 = order + 2;
  const sla_hip_lpc_group g = groups[gi];
  const uint64_t slot = g.slot_first;
  double* o = out + slot * O2;
  double r[P + 1], a[P + 1], par[P + 1];
#pragma unroll
  for (int i = 0; i <= P; i++) { r[i] = ((uint32_t)i <= order) ? o[1 + i] : 0.0; a[i] = 0.0; par[i] = 0.0; }
  const uint32_t rshift = out_rshift[slot];
  const double u = 1.1102230246251565e-16;      // 2^-53
  const double delta = CERT ? acf_blocks_budget(g.num_samples) * u * r[0] : 0.0;
  bool sure = true;
  double gain = 0.0, gain_w = 0.0;              // sum log2(1 - k^2) and its half width
  // margin test of one coefficient: does Round(k * 2^(q-1)) (half-integers away from zero, then clipped) keep its value
  // for every k within +-eps?  Only bounds below 1/64 of a code step count at all (ADVICE round 3: the UNscaled first-order
  // bound then stays below 1e-3 of a step, so that the factor `safety` in front of it provably dwarfs the higher-order
  // terms -- DESIGN section 2b; round 3 accepted up to 1/4).
#define SLA_CERT_COEF(m, kk, eps) do { \
    const double lim_ = ((m) < 4) ? 32768.0 : 128.0; \
    const double v_ = (kk) * lim_, w_ = (eps) * lim_ * 1.0000001 + 1e-12; \
    if (!(w_ < 0.015625) || !(fabs(v_) < lim_ + 2.0)) { sure = false; } \
    else if (v_ >= lim_ - 1.5) { if (!(v_ - w_ > lim_ - 1.5)) { sure = false; } } \
    else if (v_ <= -lim_ + 0.5) { if (!(v_ + w_ < -lim_ + 0.5)) { sure = false; } } \
    else { \
      const double f_ = fabs(v_) + 0.5, d_ = f_ - floor(f_); \
      if (!(d_ > w_ && 1.0 - d_ > w_)) { sure = false; } \
      if (!(v_ + w_ < lim_ - 1.5) && !(v_ - w_ > lim_ - 1.5)) { sure = false; } \
      if (!(v_ - w_ > -lim_ + 0.5) && !(v_ + w_ < -lim_ + 0.5)) { sure = false; } \
    } \
    { const double om_ = 1.0 - (kk) * (kk); \
      if (!(om_ > 0.0)) { sure = false; } \
      else { gain += log2(om_); gain_w += 2.0 * fabs(kk) * (eps) / om_ * 1.4426950408889634; } } \
  } while (0)
  if (CERT && g.num_samples >= order && !(fabs(r[0]) - (double)FLT_EPSILON > 2.0 * delta) && !((double)FLT_EPSILON - fabs(r[0]) > 2.0 * delta)) { sure = false; }
  if (!(g.num_samples < order || fabs(r[0]) < (double)FLT_EPSILON)) {
    a[0] = 1.0;
    a[1] = -r[1] / r[0];
    par[1] = r[1] / r[0];
    double e = r[0] + r[1] * a[1];
    if (CERT) {
      const double eps = safety * (1.0 + fabs(par[1])) / r[0] * (delta + 6.0 * u * r[0]);
      SLA_CERT_COEF(1, par[1], eps);
    }
#pragma unroll
    for (int d = 1; d < P; d++) {
      if ((uint32_t)d < order) {
        double gamma = 0.0;
#pragma unroll
        for (int i = 0; i <= d; i++) { gamma += a[i] * r[d + 1 - i]; }
        double n1 = 0.0;
        if (CERT) {
#pragma unroll
          for (int i = 0; i <= d; i++) { n1 += fabs(a[i]); }
        }
        const double e_prev = e;
        gamma /= (-e);
        e = (1.0 - gamma * gamma) * e;
        // a[i] <- a[i] + gamma * v[i],  v = (0, a[d], a[d-1], .., a[1], 1),  a[0] = 1, a[d+1] = 0 beforehand
        double nw[P + 1];
#pragma unroll
        for (int i = 1; i <= d; i++) { nw[i] = a[i] + gamma * a[d + 1 - i]; }
#pragma unroll
        for (int i = 1; i <= d; i++) { a[i] = nw[i]; }
        a[0] = 1.0 + gamma * 0.0;
        a[d + 1] = 0.0 + gamma * 1.0;
        par[d + 1] = -gamma;
        if (CERT) {
          if (!(e_prev > 0.0) || !(fabs(gamma) < 1.0)) { sure = false; }
          const double lev = 2.0 * (double)(d + 3) * u * n1 * r[0];
          const double eps = safety * n1 * n1 * (1.0 + fabs(gamma)) / e_prev * (delta + lev);
          SLA_CERT_COEF(d + 1, -gamma, eps);
        }
      }
    }
  }
#undef SLA_CERT_COEF
  o[0] = r[0];
  out_code[slot * O1] = 0; out_kint[slot * O1] = 0;
  bool codes_same = true;                       // (list mode on an audited pair: what the certified run stored against this run)
#pragma unroll
  for (int j = 0; j <= P; j++) {
    if ((uint32_t)j <= order) {
      o[1 + j] = par[j];
      if (j >= 1) {
        const uint32_t qb = (j < 4) ? 16 : 8;
        const int32_t lim = 1 << (qb - 1);
        const double kq = par[j] * (double)lim;
        const double rk = (kq >= 0.0) ? floor(kq + 0.5) : -floor(-kq + 0.5);
        int32_t code = f64_to_i32_x86(rk);
        code = (code < -lim) ? -lim : code;
        code = (code > lim - 1) ? (lim - 1) : code;
        const int32_t ki = (int32_t)((uint32_t)code << (16u - qb)) >> rshift;
        if (!CERT && cert_flag != nullptr && (out_code[slot * O1 + j] != code || out_kint[slot * O1 + j] != ki)) { codes_same = false; }
        out_code[slot * O1 + j] = code;
        out_kint[slot * O1 + j] = ki;
      }
    }
  }
  bool raw_side = false;
  if (CERT) {
    // RAW decision of the host (slai_code_length, src/SLAPredictor.c:416-468; threshold (double)0.95f on 8*bytes/bps):
    // bits = 1.94.. + (log2(r0 * 2^(2(bps-1)) / n) + sum log2(1 - k^2)) / 2, known here to +- half the widths
    const double power = r[0] * ldexp(1.0, (int)(2 * (bps - 1)));
    if (power > (double)FLT_MIN * 1.000001) {
      const double bits = 1.9426950408889634 + 0.5 * (log2(power) - log2((double)g.num_samples) + gain);
      const double half = 0.5 * (delta / r[0] * 1.4426950408889634 * 2.0 + gain_w) * 1.000001 + 1e-9;
      const double thr = (double)0.95f * (double)bps;
      if (!(fabs(bits - thr) > half)) { sure = false; }
      raw_side = (bits >= thr);
    } else if (!(power < (double)FLT_MIN * 0.999999)) { sure = false; }
    if (!(r[0] == r[0]) || !(fabs(r[0]) < 1e300)) { sure = false; }
    // audit (option cert_audit = N): every N-th CERTIFIED pair goes on the list as well, after its codes are stored; the exact
    // kernels then compare instead of overwrite (flag 3 | 8 * "the estimated length is on the RAW side of the threshold")
    const bool audit = sure && audit_every != 0u && (gi % audit_every) == audit_every - 1u;
    cert_flag[slot] = !sure ? 1u : !audit ? 0u : (3u | (raw_side ? 8u : 0u));
    if (!sure || audit) { fb_list[atomicAdd(fb_count, 1u)] = gi; }
  } else if (cert_flag != nullptr) {
    // exact: the reference's doubles bit for bit (2).  An audited pair (3): codes, lattice coefficients and the side of the RAW
    // threshold the certified run stored must be what this run computes -- 4 = they are, 5 = the certificate was WRONG
    // (the host fails the call).  The comparison of the estimated length ignores differences below 1e-6 bit (device log2
    // against itself on two sets of doubles that agree to ~1e-13: only a decision the certificate should never have taken
    // can differ by more).
    const uint32_t was = cert_flag[slot];
    if ((was & 7u) == 3u) {
      bool same = codes_same;
      if (bps != 0u) {
        double gain_e = 0.0;
        bool pd = true;
#pragma unroll
        for (int j = 1; j <= P; j++) { if ((uint32_t)j <= order) { const double om = 1.0 - par[j] * par[j]; if (om > 0.0) { gain_e += log2(om); } else { pd = false; } } }
        const double power = r[0] * ldexp(1.0, (int)(2 * (bps - 1)));
        if (pd && power > (double)FLT_MIN * 1.000001) {
          const double bits = 1.9426950408889634 + 0.5 * (log2(power) - log2((double)g.num_samples) + gain_e);
          const double thr = (double)0.95f * (double)bps;
          if (fabs(bits - thr) > 1e-6 && (bits >= thr) != ((was & 8u) != 0u)) { same = false; }
        } else if (!pd) { same = false; }
      }
      cert_flag[slot] = same ? 4u : 5u;
    } else {
      cert_flag[slot] = 2u;
    }
  }
  }
}
