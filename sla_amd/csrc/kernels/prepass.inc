// kernels/prepass.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): k_prepass (OR word, silence mask, zero-word count), k_batch_scan (per-file summary of a batch)
// ---------------------------------------------------------------------------------------------
// k_prepass: one 64-bit "non-zero" word per 64 samples, OR of every raw word, count of all-zero words.
// A wave owns 16 consecutive mask words = 1024 samples and reads them fully coalesced, four words'
// worth of samples in flight at a time (the kernel is a pure HBM stream: 4 B per sample and channel).
// The count lets the host skip the copy of the mask when the file has no silence to find: a silent run
// long enough to become a block (>= 2048 samples) contains all-zero words.
// ---------------------------------------------------------------------------------------------
#define PREPASS_WORDS 16    // mask words per wave: enough waves in flight to cover the HBM latency
template <int NCH>      // 1, 2 or 0 = any
__global__ __launch_bounds__(256)
void k_prepass(const int32_t* __restrict__ pcm, uint64_t stride, uint32_t nch_rt, uint32_t n,
               uint32_t shift, uint32_t ms, uint32_t* __restrict__ or_mask, uint64_t* __restrict__ nz_mask,
               uint32_t* __restrict__ tile_or, uint32_t* __restrict__ cancel, uint32_t wave_stride)
{
  const uint32_t nch = (NCH != 0) ? (uint32_t)NCH : nch_rt;
  const uint32_t lane = threadIdx.x & 63;
  uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint64_t nwords = ((uint64_t)n + 63) / 64;
  uint32_t acc_all = 0, zero_all = 0;
  // wave_stride != 0 (sla_hip_launch_prepass_early with a limit on the workgroups): the grid is smaller than the file and every
  // wave walks on by that many waves -- a pass that runs BESIDE the search's tile sums, which read the same samples, is not to
  // take the memory system for itself: its result is not needed before they are done
  for (;;) {
  uint32_t acc = 0, zero_words = 0;
  // (one or two channels: 16 mask words = 4 KB requested before the first one is looked at -- the kernel is bound by how
  // many bytes the chip has in flight: C2 80 -> 68 us with 8 words)
  constexpr uint32_t WSTEP = (NCH == 1) ? 16u : (NCH == 2) ? 8u : 4u;
  for (uint32_t w0 = 0; w0 < PREPASS_WORDS; w0 += WSTEP) {
    const uint64_t word0 = wave * PREPASS_WORDS + w0;
    if (word0 >= nwords) { break; }
    if (NCH == 1 || NCH == 2) {
      int32_t a[WSTEP], b[WSTEP];
#pragma unroll
      for (int u = 0; u < (int)WSTEP; u++) {
        const uint64_t idx = (word0 + u) * 64 + lane;
        const bool in = (idx < n);
        a[u] = in ? pcm[idx] : 0;
        b[u] = (NCH == 2 && in) ? pcm[stride + idx] : 0;
      }
#pragma unroll
      for (int u = 0; u < (int)WSTEP; u++) {
        acc |= (uint32_t)a[u] | (uint32_t)b[u];
        bool nz;
        if (NCH == 2 && ms) {
          const int32_t l = a[u] >> shift, r = b[u] >> shift;
          nz = (((int32_t)((uint32_t)l + (uint32_t)r) >> 1) != 0) || ((uint32_t)l != (uint32_t)r);
        } else {
          nz = ((a[u] >> shift) != 0) || ((b[u] >> shift) != 0);
        }
        const uint64_t bits = __ballot(nz);
        if (word0 + u < nwords) {
          if (lane == 0) { nz_mask[word0 + u] = bits; }
          zero_words += (bits == 0) ? 1u : 0u;
        }
      }
    } else {
      for (uint32_t u = 0; u < 4; u++) {
        const uint64_t idx = (word0 + u) * 64 + lane;
        bool nz = false;
        if (idx < n) {
          for (uint32_t c = 0; c < nch; c++) { acc |= (uint32_t)pcm[(uint64_t)c * stride + idx]; }
          for (uint32_t c = 0; c < nch; c++) { nz = nz || (load_int(pcm, stride, ms, c, idx, shift) != 0); }
        }
        const uint64_t bits = __ballot(nz);
        if (word0 + u < nwords) {
          if (lane == 0) { nz_mask[word0 + u] = bits; }
          zero_words += (bits == 0) ? 1u : 0u;
        }
      }
    }
  }
  if (tile_or != nullptr) {       // OR of this wave's 1024 samples (batches: offset_lshift per file)
    for (int off = 32; off > 0; off >>= 1) { acc |= __shfl_xor(acc, off); }
    if (lane == 0) { tile_or[wave] = acc; }
  }
  // a search that was started beside this kernel (sla_hip_launch_prepass_early) is for nothing: tell it at once
  if (cancel != nullptr && lane == 0 && zero_words != 0) { __hip_atomic_store(cancel, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  acc_all |= acc; zero_all += zero_words;
  if (wave_stride == 0u) { break; }
  wave += wave_stride;
  if (wave * PREPASS_WORDS >= nwords) { break; }
  }
  for (int off = 32; off > 0; off >>= 1) { acc_all |= __shfl_xor(acc_all, off); }
  // thousands of waves, one word: only the few that still add a bit pay for the atomic (a stale read just costs one)
  if (lane == 0 && (acc_all & ~__atomic_load_n(or_mask, __ATOMIC_RELAXED)) != 0) { atomicOr(or_mask, acc_all); }
  if (lane == 0 && zero_all != 0) { atomicAdd(or_mask + 1, zero_all); }
}

// ---------------------------------------------------------------------------------------------
// k_prepass_done: one thread behind k_prepass on its stream (sla_hip_launch_prepass_early).  early[1] = offset_lshift of the
// file (src/SLAEncoder.c:425-455, as the host's lshift_of), early[0] is raised when the kernels that were started beside the
// prepass on the guess "no silence" must not go on: an all-zero mask word, an OR word of 0, samples wider than declared.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64)
void k_prepass_done(const uint32_t* or_mask, uint32_t bps, uint32_t* early)
{
  if (threadIdx.x != 0 || blockIdx.x != 0) { return; }
  const uint32_t orw = or_mask[0], zeros = or_mask[1];
  uint32_t lshift = 0;
  bool stop = (orw == 0u || zeros != 0u);
  if (orw != 0u) {
    const uint32_t ntz = (uint32_t)__builtin_ctz(orw);
    if (bps < 32u - ntz || bps - (32u - ntz) >= bps) { stop = true; } else { lshift = bps - (32u - ntz); }
  }
  early[SLA_HIP_EARLY_LSHIFT] = lshift;
  if (stop) { __hip_atomic_store(early + SLA_HIP_EARLY_CANCEL, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
}

// what a kernel of the early chain asks at its start: has the prepass called the start off?  (past the L1 / scalar caches:
// the word is raised while the kernel runs)
__device__ __forceinline__ bool early_cancelled(const uint32_t* early)
{
  return early != nullptr && __hip_atomic_load(early + SLA_HIP_EARLY_CANCEL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
}

// ---------------------------------------------------------------------------------------------
// k_batch_scan: what the host needs to know about every file of a batch (files back to back on 1024-sample boundaries,
// sla_hip_analyze_batch_device) from the prepass results, so that the silence mask itself stays on the device: the OR of the
// file's tile words (-> its offset_lshift), the number of all-zero 64-sample mask words inside it, and whether its last
// super-frame -- the one case in which a block can be SILENT without such a word: fewer than 127 samples left,
// src/SLAEncoder.c:392-408 with the minimum block length shrunk to what is left -- is all zero.  One workgroup per file.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_batch_scan(const uint64_t* __restrict__ nz, const uint32_t* __restrict__ tile_or, const uint32_t* __restrict__ file_start,
                  const uint32_t* __restrict__ file_len, uint32_t max_block, uint32_t* __restrict__ info)
{
  __shared__ uint32_t s_or[4], s_zero[4];
  const uint32_t f = blockIdx.x, start = file_start[f], len = file_len[f];
  const uint32_t w0 = start >> 6, nw = len >> 6;                                    // whole mask words of the file (it starts on a word)
  const uint32_t t0 = start / SLA_HIP_PREPASS_TILE, nt = (len + SLA_HIP_PREPASS_TILE - 1) / SLA_HIP_PREPASS_TILE;
  uint32_t orw = 0, zeros = 0;
  for (uint32_t i = threadIdx.x; i < nw; i += 256) { zeros += (nz[w0 + i] == 0ull) ? 1u : 0u; }
  for (uint32_t i = threadIdx.x; i < nt; i += 256) { orw |= tile_or[t0 + i]; }
  for (int off = 32; off > 0; off >>= 1) { orw |= (uint32_t)__shfl_xor((int)orw, off); zeros += (uint32_t)__shfl_xor((int)zeros, off); }
  if ((threadIdx.x & 63) == 0) { s_or[threadIdx.x >> 6] = orw; s_zero[threadIdx.x >> 6] = zeros; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t rem = (max_block != 0u) ? (len % max_block) : 0u;
    uint32_t tail = 0;
    if (rem >= 1u && rem < 127u) {
      tail = 1;
      for (uint32_t p = start + len - rem; p < start + len; p++) { if ((nz[p >> 6] >> (p & 63u)) & 1ull) { tail = 0; break; } }
    }
    info[3 * f] = s_or[0] | s_or[1] | s_or[2] | s_or[3];
    info[3 * f + 1] = s_zero[0] + s_zero[1] + s_zero[2] + s_zero[3];
    info[3 * f + 2] = tail;
  }
}
