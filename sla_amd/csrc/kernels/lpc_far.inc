// kernels/lpc_far.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): the far-window LPC stage: k_lpc's
// semantics for windows that do not fit the LDS (blocks and super-frames of up to 65 535 samples)
// ---------------------------------------------------------------------------------------------
// k_lpc_far_stage / _chains / _finish: autocorrelation chains over windows in GLOBAL memory
//
// The reference's autocorrelation walks the whole window once per lag (src/SLAPredictor.c:331-388: for i < lag: for l += 2 lag),
// so no sliding part of a long window can stand in for it: the window is staged once, as doubles, into a caller-provided
// scratch slot (65 535 doubles = 512 KiB: it stays in an XCD's 4 MiB L2), and chain_lag0 / chain_lag (lpc_chains.inc) run on
// it unchanged -- they take a plain pointer.  One thread owns one (candidate, lag) chain, as in k_lpc; unlike k_lpc the chains
// of one window spread over as many workgroups as they fill, because nothing ties them to one CU's LDS.
//   k_lpc_far_stage    one workgroup per group of a pass: convert, mid/side, window, pre-emphasis exactly as k_lpc stages them;
//                      block form: max |x| of the integer path -> the quantiser's shift, d_rshift[slot]
//   k_lpc_far_chains   256 chains per workgroup: first the lag >= 1 chains of the group's candidates (candidate-major), then
//                      their lag-0 chains, so that a wave runs one loop body; r[lag] -> d_out[slot][1 + lag]
//   k_lpc_far_finish   one lane per candidate: r[] from the slot into LDS, levinson_out, quantiser (block form)
// Groups beyond the scratch slots: passes of `slots` groups, group g in slot g % slots, stage and chains of a pass queued
// behind the chains of the pass before (stream order is what keeps a slot's reader ahead of its next writer).
// ---------------------------------------------------------------------------------------------
#define FAR_THREADS 256u
#define FAR_FINISH_LDS (60u * 1024u)      // r[], a[], v[] of the candidates one finish workgroup takes

// RERUN (sla_hip_launch_lpc_far_rerun, search form): only the groups that k_search_finish_far flagged -- NaN in r[0] of the group's
// first slot -- are analysed.  k_lpc_far_finish stores r0 into that very word while its other workgroups of the same group are
// still starting, so only the stage and chains kernels look at it: every one of them runs before the call's one finish launch,
// and no kernel in front of that writes r[0] of any slot.  The chains kernel hands the verdict on -- the lag-0 thread of every
// candidate of a flagged group stores the NaN into r[0] of ITS candidate's slot -- and a finish lane decides from its own slot.
__device__ __forceinline__ bool far_flagged(const double* __restrict__ out, const sla_hip_lpc_group& g, uint32_t order)
{
  const double r0 = out[(uint64_t)g.slot_first * (order + 2)];
  return r0 != r0;
}

template <bool RERUN>
__global__ __launch_bounds__(FAR_THREADS)
void k_lpc_far_stage(const int32_t* __restrict__ pcm, uint64_t stride, uint32_t ms,
                     const sla_hip_lpc_group* __restrict__ groups, uint32_t g_lo,
                     const double* __restrict__ window_pool, double* __restrict__ scratch, uint32_t slot_doubles,
                     uint32_t* __restrict__ out_rshift, unsigned long long* span,
                     const double* __restrict__ out, uint32_t order, uint32_t* __restrict__ rerun_counter)
{
  __shared__ uint32_t s_maxabs;
  span_begin(span);
  if (RERUN) {
    if (!far_flagged(out, groups[g_lo + blockIdx.x], order)) { return; }
    if (threadIdx.x == 0 && rerun_counter != nullptr) { atomicAdd(rerun_counter, 1u); }
  }
  if (threadIdx.x == 0) { s_maxabs = 0; }
  __syncthreads();
  const sla_hip_lpc_group g = groups[g_lo + blockIdx.x];
  double* x = scratch + (uint64_t)blockIdx.x * slot_doubles;
  const uint32_t n = (g.num_samples < slot_doubles) ? g.num_samples : slot_doubles;      // never past the slot
  const bool windowed = (g.win_off != SLA_HIP_NO_WINDOW) && (window_pool != nullptr);
  const double* win = window_pool + (windowed ? g.win_off : 0);
  uint32_t maxabs = 0;
  for (uint32_t s = threadIdx.x; s < n; s += FAR_THREADS) {
    double cur = load_f64(pcm, stride, ms, g.channel, g.pcm_off + s);
    if (windowed) {
      cur *= win[s];
      double prev = (s > 0) ? load_f64(pcm, stride, ms, g.channel, g.pcm_off + s - 1) * win[s - 1] : 0.0;
      cur -= prev * 0.96875;        // (2^5-1)*2^-5, src/SLAPredictor.c:1803-1809
    }
    x[s] = cur;
    if (out_rshift != nullptr) {
      int32_t v = load_int(pcm, stride, ms, g.channel, g.pcm_off + s, g.int_shift);
      uint32_t a = (v > 0) ? (uint32_t)v : (0u - (uint32_t)v);
      maxabs = (a > maxabs) ? a : maxabs;
    }
  }
  if (out_rshift != nullptr) {
    maxabs = umax_wave(maxabs);
    if ((threadIdx.x & 63) == 0) { atomicMax(&s_maxabs, maxabs); }
    __syncthreads();
    if (threadIdx.x == 0 && g.cand_count != 0) {
      const uint32_t m = s_maxabs;
      // bit width = ceil(log2(max|x|)) + 1, at least 1                  src/SLAUtility.c:677-696
      const uint32_t l2c = (m > 1) ? (32u - (uint32_t)__builtin_clz(m - 1u)) : 0u;
      const uint32_t bitwidth = (m > 0) ? (l2c + 1u) : 1u;
      out_rshift[g.slot_first] = (bitwidth > 16) ? (bitwidth - 16) : 0;
    }
  }
}

template <bool RERUN>
__global__ __launch_bounds__(FAR_THREADS)
void k_lpc_far_chains(const sla_hip_lpc_group* __restrict__ groups, uint32_t g_lo, const sla_hip_lpc_cand* __restrict__ cands,
                      uint32_t order, const double* __restrict__ scratch, uint32_t slot_doubles, uint32_t chunks,
                      double* __restrict__ out)
{
  const uint32_t gi = blockIdx.x / chunks, chunk = blockIdx.x - gi * chunks;
  const sla_hip_lpc_group g = groups[g_lo + gi];
  if (RERUN && !far_flagged(out, g, order)) { return; }
  const uint32_t nlag = g.cand_count * order;
  const uint32_t q = chunk * FAR_THREADS + threadIdx.x;
  if (q >= nlag + g.cand_count) { return; }
  const double* x = scratch + (uint64_t)gi * slot_doubles;
  const uint32_t wlen = (g.num_samples < slot_doubles) ? g.num_samples : slot_doubles;
  const uint32_t cidx = (q < nlag) ? (q / order) : (q - nlag);
  const uint32_t lag = (q < nlag) ? (1 + (q - cidx * order)) : 0;
  const sla_hip_lpc_cand cd = cands[g.cand_first + cidx];
  // (a candidate that leaves its window is the caller's error: it is analysed as empty instead of read out of the slot)
  const uint32_t n = (cd.start <= wlen && cd.len <= wlen - cd.start) ? cd.len : 0u;
  const double* xs = x + cd.start;
  double r;
  if (lag == 0) { r = chain_lag0(xs, n); } else { r = (lag < n) ? chain_lag(xs, n, lag) : 0.0; }
  out[((uint64_t)g.slot_first + cidx) * (order + 2) + 1 + lag] = r;
  // (slot 0 of a flagged group holds the NaN already: no thread of this launch changes what far_flagged reads)
  if (RERUN && lag == 0 && cidx != 0) { out[((uint64_t)g.slot_first + cidx) * (order + 2)] = __longlong_as_double(0x7FF8000000000000ll); }
}

template <bool RERUN>
__global__ __launch_bounds__(64)
void k_lpc_far_finish(const sla_hip_lpc_group* __restrict__ groups, const sla_hip_lpc_cand* __restrict__ cands,
                      uint32_t order, uint32_t per_wg, uint32_t chunks, uint32_t max_window, double* __restrict__ out,
                      int32_t* __restrict__ out_code, int32_t* __restrict__ out_kint, const uint32_t* __restrict__ out_rshift,
                      unsigned long long* span)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const uint32_t O1 = order + 1, O2 = order + 2;
  const uint32_t gi = blockIdx.x / chunks, chunk = blockIdx.x - gi * chunks;
  const sla_hip_lpc_group g = groups[gi];
  const uint32_t cidx = chunk * per_wg + threadIdx.x;
  if (threadIdx.x < per_wg && cidx < g.cand_count) {
    const sla_hip_lpc_cand cd = cands[g.cand_first + cidx];
    const uint32_t wlen = (g.num_samples < max_window) ? g.num_samples : max_window;
    const uint32_t n = (cd.start <= wlen && cd.len <= wlen - cd.start) ? cd.len : 0u;
    const uint64_t slot = (uint64_t)g.slot_first + cidx;
    double* rc = lds + (size_t)threadIdx.x * (O1 + 2 * O2);
    double* a = rc + O1;
    double* v = a + O2;
    double* o = out + slot * O2;
    if (!RERUN || o[0] != o[0]) {                                // (RERUN: this candidate's own word, see far_flagged)
      for (uint32_t i = 0; i < O1; i++) { rc[i] = o[1 + i]; }    // the chains left r[] where the coefficients go
      levinson_out(rc, a, v, o, order, n);
    }
    // coefficient quantiser (chosen blocks: one candidate per group), as in k_lpc; the thread reads its own stores
    if (out_code != nullptr) {
      const uint32_t rshift = out_rshift[slot];
      out_code[slot * O1] = 0; out_kint[slot * O1] = 0;
      for (uint32_t ord = 1; ord <= order; ord++) {
        const uint32_t qb = (ord < 4) ? 16 : 8;
        const int32_t lim = 1 << (qb - 1);
        double kq = o[1 + ord] * (double)lim;
        double rk = (kq >= 0.0) ? floor(kq + 0.5) : -floor(-kq + 0.5);
        int32_t code = f64_to_i32_x86(rk);
        code = (code < -lim) ? -lim : code;
        code = (code > lim - 1) ? (lim - 1) : code;
        out_code[slot * O1 + ord] = code;
        out_kint[slot * O1 + ord] = (int32_t)((uint32_t)code << (16u - qb)) >> rshift;
      }
    }
  }
  span_end(span);
}
