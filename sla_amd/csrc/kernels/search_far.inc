// kernels/search_far.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): the finish kernel of the
// tile-sum search for windows of up to 64 tiles (sla_hip_launch_search_far; the tile sums are k_acf_tiles / k_acf_tiles_lds
// of search.inc with a stride of SLA_HIP_XTILES_FAR tiles per group)
// ---------------------------------------------------------------------------------------------
// k_search_finish_far: k_search_finish's exact form (mode 0 / 2) for groups of up to 64 tiles and any number of candidates.
//
// A 65 535-sample window has 2015 candidates of up to 64 tiles each: walked as k_search_finish walks them -- one wave per
// group, 64 candidates per pass, every (candidate, lag) adding up its tiles from global memory -- that is 32 serial passes of
// up to 65 loads per sum.  Here a group's candidates spread over as many workgroups of 256 lanes as they fill (grid = groups x
// chunks, as k_lpc_far_finish), and every workgroup first stages, per lag, the RUNNING PREFIX of the group's P_t over the tiles
// and the X_t in LDS: r[lag] of candidate [first tile, last tile] is prefix[last + 1] - prefix[first] - X[last], three LDS
// reads.  Below the exactness limit every P_t, every X_t and every sum of some of them is an integer multiple of the squared
// unit below 2^53 of it (a partial sum of the window's pair products is bounded by the window's energy, whatever the number of
// tiles), so the prefixes and their differences are exact and equal k_search_finish's left-to-right sums bit for bit.
// LDS, lag-major so that the lanes of a wave -- candidates, i.e. different tiles at the same lag -- read consecutive doubles:
// prefix[order + 1][65] | X[order + 1][64], 53 KiB at order 51 (three workgroups = twelve waves per CU; the recursion's registers
// allow no more at the high orders anyway).
// The group's energy is the prefix of lag 0 over all its tiles, summed in tile order as k_search_finish sums it; a group at or
// over the limit gets NaN in r[0] of every candidate's slot and nothing else (sla_hip_launch_lpc_far_rerun redoes it).
// ---------------------------------------------------------------------------------------------
#define XFF_THREADS 256u
#define XFF_PSTRIDE (SLA_HIP_XTILES_FAR + 1u)

template <int P>           // P >= order: 16, 32, 48, 64
__global__ __launch_bounds__(XFF_THREADS)
void k_search_finish_far(uint32_t order, uint32_t lags, uint32_t chunks,
                         const sla_hip_lpc_group* __restrict__ groups, const sla_hip_lpc_cand* __restrict__ cands,
                         const double* __restrict__ tile_sums, double* __restrict__ out, double exact_limit,
                         unsigned long long* span)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  span_begin(span);
  const uint32_t O1 = order + 1, O2 = order + 2;
  const uint32_t gi = blockIdx.x / chunks, chunk = blockIdx.x - gi * chunks;
  const sla_hip_lpc_group g = groups[gi];
  uint32_t ntiles = (g.num_samples + SLA_HIP_XTILE - 1) / SLA_HIP_XTILE;
  if (ntiles > SLA_HIP_XTILES_FAR) { ntiles = SLA_HIP_XTILES_FAR; }      // (a window beyond max_window is the caller's error: never past the buffers)
  const uint32_t wlen = (g.num_samples < ntiles * SLA_HIP_XTILE) ? g.num_samples : ntiles * SLA_HIP_XTILE;
  const double* ts = tile_sums + (uint64_t)gi * SLA_HIP_XTILES_FAR * 2 * lags;
  double* pre = lds;                                      // [O1][XFF_PSTRIDE]: pre[lag][t] = P_0[lag] + .. + P_(t-1)[lag]
  double* xs = lds + (size_t)O1 * XFF_PSTRIDE;            // [O1][SLA_HIP_XTILES_FAR]
  for (uint32_t q = threadIdx.x; q < ntiles * O1; q += XFF_THREADS) {
    const uint32_t t = q / O1, lag = q - t * O1;
    pre[lag * XFF_PSTRIDE + t + 1] = ts[(uint64_t)t * 2 * lags + lag];
    xs[lag * SLA_HIP_XTILES_FAR + t] = ts[(uint64_t)t * 2 * lags + lags + lag];
  }
  __syncthreads();
  if (threadIdx.x < O1) {
    double* row = pre + threadIdx.x * XFF_PSTRIDE;
    double run = 0.0;
    row[0] = 0.0;
    for (uint32_t t = 0; t < ntiles; t++) { run += row[t + 1]; row[t + 1] = run; }      // tile order: lag 0's total is k_search_finish's energy
  }
  __syncthreads();
  const double energy = pre[ntiles];
  const uint32_t cidx = chunk * XFF_THREADS + threadIdx.x;
  if (cidx < g.cand_count) {
    const sla_hip_lpc_cand cd = cands[g.cand_first + cidx];
    double* o = out + ((uint64_t)g.slot_first + cidx) * O2;
    if (energy < exact_limit) {
      // (a candidate that leaves its window is the caller's error: analysed as empty, as k_lpc_far_chains has it)
      const uint32_t n = (cd.start <= wlen && cd.len <= wlen - cd.start) ? cd.len : 0u;
      const uint32_t first = cd.start / SLA_HIP_XTILE, last = (n != 0u) ? (cd.start + n - 1) / SLA_HIP_XTILE : first;
      const uint32_t lastc = (last < ntiles) ? last : 0u;      // (n == 0 at the window's end: nothing is kept of the reads)
      const uint32_t firstc = (first < ntiles) ? first : 0u;
      double rr[P + 1];
#pragma unroll
      for (int i = 0; i <= P; i++) {
        // exact below the limit: the difference of two exact prefixes minus the straddling pairs of the last tile
        rr[i] = 0.0;
        if ((uint32_t)i <= order) {                             // (the same for the whole launch)
          const double v = pre[i * XFF_PSTRIDE + lastc + 1] - pre[i * XFF_PSTRIDE + firstc] - xs[i * SLA_HIP_XTILES_FAR + lastc];
          rr[i] = ((uint32_t)i < n) ? v : 0.0;                  // r[lag] = 0 for lag >= len, as k_search_finish has it
        }
      }
      levinson_regs<P>(rr, o, order, n);
    } else {
      o[0] = __longlong_as_double(0x7FF8000000000000ll);          // flagged: rerun as serial chains
    }
  }
  span_end(span);
}
