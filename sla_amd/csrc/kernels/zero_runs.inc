// kernels/zero_runs.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): k_zero_run_tiles, k_zero_run_list (the run list of the silence mask)
// ---------------------------------------------------------------------------------------------
// The list of zero runs the host's super-frame hop and block test need instead of the whole mask (include/sla_hip.h,
// sla_hip_launch_zero_runs; DESIGN section 2e): every maximal run of zero bits inside a segment (a file) that is at least
// min_run samples long or ends at the segment's end.
//
// Everything is built on one quantity, "the last set bit before here": L(p) = 1 + the highest set bit position below p, 0 when
// there is none.  Bits between segments and behind the span are zero, so the zero run that ends at a set bit q of segment
// [s, e) starts at max(L(q), s), and the run that ends at e starts at max(L(e), s): segments only clip, they never take part
// in the scan, which therefore runs over the whole mask at once.
//
//   k_zero_run_tiles   a workgroup per tile of SLA_HIP_ZERO_RUN_TILE mask words, a wave per 128-word group of it (64 lanes x
//                      16 bytes, one load): L of the group's end, taken inside the group alone (0: the group is all zero),
//                      per group and -- their maximum -- per tile: ZR_GROUPS + 1 words per tile.
//   k_zero_run_list    the same grid: a wave finds L of its group's start from the tile words in front of its tile and the
//                      group words in front of it in its tile, scans its 128 words (shuffles, no LDS), and every word with a
//                      set bit tests the run that ends at its first one.  With min_run >= 64 no run that ends at a later bit
//                      of the word can qualify.  Further workgroups take the segments, a wave each: the run that ends at the
//                      segment's end.  Runs are appended with one atomic per wave and word slot, behind a ballot.
// No workgroup waits for another one: the two launches are the only ordering.  Every loop runs a count known on entry.
// ---------------------------------------------------------------------------------------------
#define ZR_GROUP_WORDS 128u                                        // mask words of one wave-wide 16-byte load
#define ZR_GROUPS (SLA_HIP_ZERO_RUN_TILE / ZR_GROUP_WORDS)         // groups (= waves) per tile
static_assert(ZR_GROUPS * ZR_GROUP_WORDS == SLA_HIP_ZERO_RUN_TILE && ZR_GROUPS >= 1 && ZR_GROUPS <= 16, "a tile is a workgroup of whole waves");

// the lane's two words of group `group` (words 2 lane, 2 lane + 1 of it); words at or behind nwords read as zero
__device__ __forceinline__ void zr_load(const uint64_t* __restrict__ nz, uint64_t nwords, uint64_t group, uint32_t lane, uint64_t& w0, uint64_t& w1)
{
  const uint64_t i = group * ZR_GROUP_WORDS + 2u * lane;
  w0 = 0; w1 = 0;
  if (i + 1 < nwords) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(nz + i);
    w0 = v.x; w1 = v.y;
  } else if (i < nwords) {
    w0 = nz[i];
  }
}

// 1 + position of the highest set bit of the pair that starts at sample `base` (0: none)
__device__ __forceinline__ uint32_t zr_last(uint64_t w0, uint64_t w1, uint32_t base)
{
  if (w1 != 0) { return base + 128u - (uint32_t)__clzll((long long)w1); }
  if (w0 != 0) { return base + 64u - (uint32_t)__clzll((long long)w0); }
  return 0u;
}

__global__ __launch_bounds__(64 * ZR_GROUPS)
void k_zero_run_tiles(const uint64_t* __restrict__ nz, uint32_t span, uint32_t* __restrict__ scratch, uint32_t* __restrict__ count)
{
  __shared__ uint32_t s_last[ZR_GROUPS];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t nwords = ((uint64_t)span + 63) / 64;
  const uint64_t group = (uint64_t)blockIdx.x * ZR_GROUPS + wave;
  uint64_t w0, w1;
  if (blockIdx.x == 0 && threadIdx.x == 0) { count[0] = 0; }        // (the list kernel appends behind this launch)
  zr_load(nz, nwords, group, lane, w0, w1);
  const uint32_t last = umax_wave(zr_last(w0, w1, (uint32_t)(group * ZR_GROUP_WORDS + 2u * lane) * 64u));
  if (lane == 0) { scratch[(size_t)blockIdx.x * (ZR_GROUPS + 1) + 1 + wave] = last; s_last[wave] = last; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t m = 0;
    for (uint32_t g = 0; g < ZR_GROUPS; g++) { m = (s_last[g] > m) ? s_last[g] : m; }
    scratch[(size_t)blockIdx.x * (ZR_GROUPS + 1)] = m;
  }
}

// L of the start of group `g` of tile `tile`, by the whole wave: tile words in front of the tile, group words in front of the
// group (values grow with the position wherever they are not 0, so the maximum is the nearest one)
__device__ __forceinline__ uint32_t zr_prefix(const uint32_t* __restrict__ scratch, uint32_t tile, uint32_t g, uint32_t lane)
{
  uint32_t m = 0;
  for (uint32_t t = lane; t < tile; t += 64) { const uint32_t v = scratch[(size_t)t * (ZR_GROUPS + 1)]; m = (v > m) ? v : m; }
  if (lane < g) { const uint32_t v = scratch[(size_t)tile * (ZR_GROUPS + 1) + 1 + lane]; m = (v > m) ? v : m; }
  return umax_wave(m);
}

// one entry per lane with `take` set, anywhere in the list; the count goes on past the capacity, the stores do not
__device__ __forceinline__ void zr_append(bool take, uint32_t start, uint32_t length, uint32_t lane, sla_hip_zero_run* __restrict__ runs,
                                          uint32_t capacity, uint32_t* __restrict__ count)
{
  const uint64_t votes = __ballot(take);
  if (votes == 0) { return; }                                       // (wave-uniform)
  uint32_t base = 0;
  if (lane == (uint32_t)__ffsll((long long)votes) - 1u) { base = atomicAdd(count, (uint32_t)__popcll(votes)); }
  base = (uint32_t)__shfl((int)base, __ffsll((long long)votes) - 1);
  if (take) {
    const uint32_t at = base + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
    if (at >= base && at < capacity) { runs[at].start = start; runs[at].length = length; }
  }
}

__global__ __launch_bounds__(64 * ZR_GROUPS)
void k_zero_run_list(const uint64_t* __restrict__ nz, uint32_t span, const uint32_t* __restrict__ seg_start,
                     const uint32_t* __restrict__ seg_len, uint32_t num_segs, uint32_t min_run, uint32_t ntiles,
                     const uint32_t* __restrict__ scratch, sla_hip_zero_run* __restrict__ runs, uint32_t capacity,
                     uint32_t* __restrict__ count)
{
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t nwords = ((uint64_t)span + 63) / 64;
  uint64_t w0, w1;
  if (blockIdx.x >= ntiles) {
    // ---- the run that ends at a segment's end: a wave per segment
    const uint32_t s = (blockIdx.x - ntiles) * ZR_GROUPS + wave;
    if (s >= num_segs) { return; }                                  // (wave-uniform)
    const uint32_t lo = (seg_start != nullptr) ? seg_start[s] : 0u;
    const uint32_t len = (seg_start != nullptr) ? seg_len[s] : span;
    if (len == 0 || lo >= span || len > span - lo) { return; }      // an empty segment has no run (one outside the mask: not read)
    const uint32_t end = lo + len;                                  // (<= span)
    const uint64_t group = (uint64_t)((end - 1u) >> 6) / ZR_GROUP_WORDS;
    const uint32_t tile = (uint32_t)(group / ZR_GROUPS), g = (uint32_t)(group % ZR_GROUPS);
    const uint32_t base = (uint32_t)(group * ZR_GROUP_WORDS + 2u * lane) * 64u;
    zr_load(nz, nwords, group, lane, w0, w1);
    // bits at or behind the segment's end do not count (they are zero anyway: the gap, or the end of the mask)
    if (end <= base) { w0 = 0; } else if (end - base < 64u) { w0 &= (1ull << (end - base)) - 1ull; }
    if (end <= base + 64u) { w1 = 0; } else if (end - base - 64u < 64u) { w1 &= (1ull << (end - base - 64u)) - 1ull; }
    uint32_t last = umax_wave(zr_last(w0, w1, base));
    if (last == 0) { last = zr_prefix(scratch, tile, g, lane); }
    if (last < lo) { last = lo; }
    zr_append(lane == 0 && last < end, last, end - last, lane, runs, capacity, count);
    return;
  }
  // ---- runs that end at a set bit: a wave per group
  const uint32_t tile = blockIdx.x;
  const uint64_t group = (uint64_t)tile * ZR_GROUPS + wave;
  const uint32_t base = (uint32_t)(group * ZR_GROUP_WORDS + 2u * lane) * 64u;
  zr_load(nz, nwords, group, lane, w0, w1);
  if (__ballot(w0 != 0 || w1 != 0) == 0) { return; }                // an all-zero group ends no run (wave-uniform)
  // L of this lane's first word: the group's prefix and the lanes below (inclusive max-scan, then one step down)
  uint32_t incl = zr_last(w0, w1, base);
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, off);
    if (lane >= (uint32_t)off && o > incl) { incl = o; }
  }
  uint32_t before = (uint32_t)__shfl_up((int)incl, 1);
  if (lane == 0) { before = 0; }
  const uint32_t prefix = zr_prefix(scratch, tile, wave, lane);
  if (prefix > before) { before = prefix; }
  for (int j = 0; j < 2; j++) {
    const uint64_t w = (j == 0) ? w0 : w1;
    const uint32_t wbase = base + 64u * (uint32_t)j;
    const uint32_t from = (j == 1 && w0 != 0) ? base + 64u - (uint32_t)__clzll((long long)w0) : before;
    bool take = false;
    uint32_t start = 0, length = 0;
    if (w != 0) {
      const uint32_t q = wbase + (uint32_t)__ffsll((long long)w) - 1u;      // the run [from, q) ends here
      if (q - from >= min_run) {
        // rare from here on: which segment is q in?  Its start clips the run.
        uint32_t lo = 0;
        bool inside = true;
        if (seg_start != nullptr) {
          uint32_t a = 0, b = num_segs;                             // the last segment that starts at or before q
          for (uint32_t it = 0; it < 32 && a < b; it++) {
            const uint32_t mid = a + (b - a) / 2;
            if (seg_start[mid] <= q) { a = mid + 1; } else { b = mid; }
          }
          inside = (a > 0) && (q - seg_start[a - 1] < seg_len[a - 1]);
          lo = inside ? seg_start[a - 1] : 0u;
        }
        start = (from > lo) ? from : lo;
        length = q - start;
        take = inside && length >= min_run;
      }
    }
    zr_append(take, start, length, lane, runs, capacity, count);
  }
}
