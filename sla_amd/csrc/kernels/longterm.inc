// kernels/longterm.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): k_ltm_acf / k_ltm_acf2 (bit-exact NR FFT autocorrelation + pitch scan), k_ltm_solve (Toeplitz solve in x87 arithmetic)
// ---------------------------------------------------------------------------------------------
// k_ltm_acf: autocorrelation of the lattice residual by the reference's real FFT
// (src/SLAPredictor.c:827-853, src/SLAUtility.c:220-312): forward real FFT -> |.|^2 -> inverse.
// One workgroup per (block, channel); the F doubles live in LDS (F <= 16384) or, for the largest
// encoder capacity, in an L2-resident global scratch slot.  Bit-exactness: twiddles are NOT
// evaluated here -- the host generates them once with the reference's sin()-seeded recurrence --
// and every butterfly is the same mul/mul/sub, mul/mul/add, sub, sub, add, add sequence; the order
// of butterflies inside a stage is free because they touch disjoint elements.
// Twiddle buffer layout (doubles): [0,F/2) stage re fwd | [F/2,F) stage im fwd | [F,3F/2) re inv |
// [3F/2,2F) im inv | [2F,2F+F/4) real-pass re fwd | +F/4 im fwd | +F/4 re inv | +F/4 im inv.
// ---------------------------------------------------------------------------------------------
#define ACF_THREADS 512

// LDS layout: complex slot c (re, im = 16 B, always moved as one b128 access) lives at slot c ^ S(c), S a GF(2)-linear map
// of the bits 3.. of c onto the low nibble.  Every access pattern of a power-of-two FFT is "base + j * 2^s": without S all
// lanes of an access group hit the same 4 banks (measured in round 1: 13 bank-conflict cycles per LDS instruction).
// Round 3 folded the higher nibbles onto the low one, c ^ ((c >> 4 ^ c >> 8 ^ c >> 12) & 15): 2.0 - 2.2 conflict cycles
// per LDS instruction were left (profiles/r3_sq_counters_*), and tests/tools/fft_lds_conflicts.py -- a model of every pass
// of k_ltm_acf2 on gfx950's real access groups: a ds_read_b128 is served 16 lanes at a time, but the lanes are
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32), on 64 banks; a ds_write_b128 8 consecutive lanes at a time on 32 banks --
// reproduces those numbers (2.17 at 4096 points, 1.95 at 8192) and says where they come from: every WRITE of the first pass
// and of the inverse transform's first pass, every read at half-span 8, the bit-reversed scatter: all two-way.  The fold
// cannot separate what differs in bit 3 of c on a write (8 slots = 3 bits).  The rows below (bit j of the nibble = parity of
// (c >> 3) & ACF_SW_ROW<j>; hill-climbed in that script over the three transform sizes) leave 0.24 / 0.36 / 0.37 per
// instruction (2048 / 4096 / 8192 points), all of it in the middle pass's descending run.  The map costs about twice the
// instructions of the fold, and the kernel is bound by instruction issue, not by the LDS (the first build with these rows ran
// 7 % SLOWER: profiles/r4_fft_swizzle_ab.txt): it pays only together with the middle pass computing it four times per thread
// instead of four times per pair (acf2_middle).  S only reads bits >= 3 (bit 3 only into bits 0..2), so the map is a bijection, an index
// below 8 is its own image, and S(a + b) = S(a) ^ S(b) when a and b share no bit -- what the passes use.
#define ACF_SW_ROW0 718u
#define ACF_SW_ROW1 485u
#define ACF_SW_ROW2 129u
#define ACF_SW_ROW3 76u
static_assert((ACF_SW_ROW3 & 1u) == 0u, "bit 3 of the slot must not depend on itself");
__device__ __forceinline__ constexpr uint32_t acf_sw(uint32_t c)
{
  const uint32_t hi = c >> 3;
  return c ^ ((uint32_t)__builtin_popcount(hi & ACF_SW_ROW0) & 1u) ^ (((uint32_t)__builtin_popcount(hi & ACF_SW_ROW1) & 1u) << 1)
           ^ (((uint32_t)__builtin_popcount(hi & ACF_SW_ROW2) & 1u) << 2) ^ (((uint32_t)__builtin_popcount(hi & ACF_SW_ROW3) & 1u) << 3);
}

// One radix-2 butterfly of the reference's four1 loop (src/SLAUtility.c:220-260): same products, same order.
__device__ __forceinline__ void acf_bfly(double2& zi, double2& zq, double wr, double wi)
{
  const double tr = wr * zq.x - wi * zq.y;
  const double ti = wr * zq.y + wi * zq.x;
  zq = make_double2(zi.x - tr, zi.y - ti);
  zi = make_double2(zi.x + tr, zi.y + ti);
}

// The same butterfly for the certified route (k_ltm_acf_fast): products fused into the sums, 8 FP64 issues instead of 10.
// Not the reference's rounding: whoever uses it carries an error bound (acf_emit_cert, k_ltm_solve_cert).
__device__ __forceinline__ void acf_bfly_fma(double2& zi, double2& zq, double wr, double wi)
{
  const double tr = fma(wr, zq.x, -(wi * zq.y));
  const double ti = fma(wr, zq.y, wi * zq.x);
  zq = make_double2(zi.x - tr, zi.y - ti);
  zi = make_double2(zi.x + tr, zi.y + ti);
}
template <bool FAST>
__device__ __forceinline__ void acf_bfly_sel(double2& zi, double2& zq, double wr, double wi)
{
  if constexpr (FAST) { acf_bfly_fma(zi, zq, wr, wi); } else { acf_bfly(zi, zq, wr, wi); }
}

// R consecutive radix-2 stages (half-spans h, 2h, .., h<<(R-1)) on the 2^R points ci + m*h that only
// exchange data among themselves: one LDS round trip and one barrier instead of R, 2^R - 1 twiddles instead
// of R * 2^(R-1).  Every butterfly is the radix-2 one above on the same operands, so the results are the
// radix-2 results bit for bit (the order of butterflies inside a stage is free).
template <int R>
__device__ __forceinline__ void acf_pass(double2* z, uint32_t npts, uint32_t log2h, const double* __restrict__ twr,
                                         const double* __restrict__ twi)
{
  constexpr uint32_t P = 1u << R;
  const uint32_t h = 1u << log2h;
  for (uint32_t b = threadIdx.x; b < (npts >> R); b += ACF_THREADS) {
    const uint32_t low = b & (h - 1), ci = low + ((b >> log2h) << (log2h + R));
    double2 v[P];
#pragma unroll
    for (uint32_t m = 0; m < P; m++) { v[m] = z[acf_sw(ci + m * h)]; }
#pragma unroll
    for (int st = 0; st < R; st++) {
      const uint32_t hs = h << st;                      // half-span of this stage; its twiddles start at hs - 1
#pragma unroll
      for (uint32_t m = 0; m < P; m++) {
        if ((m >> st) & 1u) { continue; }
        const uint32_t k = low + (m & ((1u << st) - 1u)) * h;
        acf_bfly(v[m], v[m + (1u << st)], twr[hs - 1 + k], twi[hs - 1 + k]);
      }
    }
#pragma unroll
    for (uint32_t m = 0; m < P; m++) { z[acf_sw(ci + m * h)] = v[m]; }
  }
  __syncthreads();
}

__device__ __forceinline__ void acf_stages(double2* z, uint32_t log2npts, const double* __restrict__ twr,
                                           const double* __restrict__ twi)
{
  const uint32_t npts = 1u << log2npts;
  uint32_t log2h = 0;
  while (log2h < log2npts) {
    const uint32_t left = log2npts - log2h;
    if (left >= 3 && left != 4) { acf_pass<3>(z, npts, log2h, twr, twi); log2h += 3; }
    else if (left >= 2) { acf_pass<2>(z, npts, log2h, twr, twi); log2h += 2; }
    else { acf_pass<1>(z, npts, log2h, twr, twi); log2h += 1; }
  }
}

// the h1/h2 recombination pass shared by the forward and the inverse real transform; complex slot i-1
// holds the reference's (data[i1], data[i2]), slot npts-(i-1) its (data[i3], data[i4])
__device__ __forceinline__ void acf_real_pass(double2* z, uint32_t npts, double c2, const double* __restrict__ rtr,
                                              const double* __restrict__ rti)
{
  const double c1 = 0.5;
  for (uint32_t i = 2 + threadIdx.x; i <= (npts >> 1); i += ACF_THREADS) {
    const uint32_t ca = i - 1, cb = npts - (i - 1);
    const double wr = rtr[i - 2], wi = rti[i - 2];
    const double2 A = z[acf_sw(ca)], B = z[acf_sw(cb)];
    const double h1r = c1 * (A.x + B.x);
    const double h1i = c1 * (A.y - B.y);
    const double h2r = -c2 * (A.y + B.y);
    const double h2i = c2 * (A.x - B.x);
    z[acf_sw(ca)] = make_double2(h1r + wr * h2r - wi * h2i, h1i + wr * h2i + wi * h2r);
    z[acf_sw(cb)] = make_double2(h1r - wr * h2r + wi * h2i, -h1i + wr * h2i + wi * h2r);
  }
}

__device__ __forceinline__ double acf_at(const double2* z, uint32_t j)      // real element j of the array
{
  const double2 v = z[acf_sw(j >> 1)];
  return (j & 1u) ? v.y : v.x;
}

// Pitch candidate from the autocorrelation (reference src/SLAPredictor.c:866-924): segments run from an
// upward zero crossing to the next downward one (inclusive, capped at lag 256; a search that reaches 256
// inspects lags 256 and 257), each segment contributes its largest strict positive local maximum, and the
// earliest of the globally largest wins.  The three per-lag predicates are evaluated by 320 threads and
// ballotted into bit masks; one lane then hops from crossing to crossing with find-first-set and only
// touches the values of local maxima.
#define ACF_PICK_LAGS 320

__device__ __forceinline__ uint32_t first_set_from(const unsigned long long* m, uint32_t pos, uint32_t limit)
{
  while (pos < limit) {
    const unsigned long long w = m[pos >> 6] >> (pos & 63);
    if (w != 0) {
      const uint32_t hit = pos + (uint32_t)__builtin_ctzll(w);
      return (hit < limit) ? hit : limit;
    }
    pos = (pos | 63u) + 1u;
  }
  return limit;
}

__device__ __forceinline__ void acf_pick(const double* v, const unsigned long long* up, const unsigned long long* down,
                                         const unsigned long long* lm, uint32_t& chosen, uint32_t& ncand)
{
  double top = 0.0;
  uint32_t i = 1;
  chosen = 0; ncand = 0;
  while (i < 256) {
    uint32_t start = first_set_from(up, i, 256), end, arg = 0;
    double val = 0.0;
    end = (start < 256) ? first_set_from(down, start + 1, 256) : 257;
    for (uint32_t j = first_set_from(lm, start, end + 1); j <= end; j = first_set_from(lm, j + 1, end + 1)) {
      if (v[j] > val) { arg = j; val = v[j]; }
    }
    if (arg != 0) { ncand++; if (val > top) { top = val; chosen = arg; } }
    i = end + 1;
  }
}

// what a job leaves behind: the compact record {code, chosen lag, acf[0..4], acf[chosen-2..chosen+2]} (the Toeplitz
// solve follows in k_ltm_solve), or the first `head` autocorrelation values.
//
// The pitch scan (src/SLAPredictor.c:866-924; acf_pick above is its serial form) as ONE WAVE's work instead of one
// lane's -- a lane hopping from crossing to crossing through LDS-resident masks held the whole workgroup for 25 us per
// job, a third of the kernel.  The scan is a two-state machine over the lags 1 .. 255: OUT -> IN at an upward zero
// crossing, IN -> OUT behind a downward one (segment = [start, end], both inclusive; an unterminated segment also takes
// lag 256, and a scan that runs out of upward crossings while OUT inspects lags 256 and 257), and what it delivers is
// the first lag among the largest strict positive local maxima inside segments (per segment the first largest, over
// the segments the first largest: the smallest lag that attains the overall maximum) and whether there was any.
// Lane l owns lags 4l .. 4l+3: it folds its four transitions into one map {OUT, IN} -> {OUT, IN}, a 6-step wave scan
// composes the maps of the lanes below it, and an arg-max over (value, -lag) picks the candidate.
template <int THREADS>
__device__ __forceinline__ void acf_emit(const double2* z, uint32_t job, double* __restrict__ out, uint32_t head,
                                         double* s_acf, unsigned long long (*s_mask)[ACF_PICK_LAGS / 64])
{
  if (head == SLA_HIP_ACF_RECORD) {
    __syncthreads();
    if (threadIdx.x < ACF_PICK_LAGS) {
      const uint32_t j = threadIdx.x;
      const double vc = acf_at(z, j), vm = (j >= 1) ? acf_at(z, j - 1) : 0.0, vp = acf_at(z, j + 1);
      s_acf[j] = vc;
      const unsigned long long bu = __ballot(j >= 1 && j < 256 && vm < 0.0 && vc > 0.0);
      const unsigned long long bd = __ballot(j >= 1 && j < 256 && vc > 0.0 && vp < 0.0);
      const unsigned long long bl = __ballot(j >= 1 && j <= 257 && vc > vm && vc > vp && vc > 0.0);
      if ((j & 63) == 0) { s_mask[0][j >> 6] = bu; s_mask[1][j >> 6] = bd; s_mask[2][j >> 6] = bl; }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      const uint32_t lane = threadIdx.x;
      const uint32_t w = lane >> 4, sh = (lane & 15u) * 4;                      // lags 4*lane .. 4*lane+3 = bits sh .. sh+3 of word w
      const uint32_t up = (uint32_t)(s_mask[0][w] >> sh) & 15u, dn = (uint32_t)(s_mask[1][w] >> sh) & 15u;
      const uint32_t lm = (uint32_t)(s_mask[2][w] >> sh) & 15u;
      const uint32_t lm_hi = (uint32_t)s_mask[2][4] & 3u;                       // local maxima at lags 256, 257
      // this lane's map: state behind its four lags when the state in front of them is OUT (bit 0) / IN (bit 1)
      uint32_t f = 0;
#pragma unroll
      for (uint32_t s0 = 0; s0 < 2; s0++) {
        uint32_t st = s0;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) { st = st ? (((dn >> q) & 1u) ^ 1u) : ((up >> q) & 1u); }
        f |= st << s0;
      }
      // inclusive scan of the maps over the lanes (g = everything below, then f): h(s) = f(g(s))
      uint32_t g = f;
#pragma unroll
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t below = (uint32_t)__shfl_up((int)g, d);
        if (lane >= d) { g = ((g >> (below & 1u)) & 1u) | (((g >> ((below >> 1) & 1u)) & 1u) << 1); }
      }
      const uint32_t incl = g & 1u;                                            // state behind this lane's lags (the machine starts OUT)
      uint32_t st = (uint32_t)__shfl_up((int)incl, 1);
      if (lane == 0) { st = 0; }
      const uint32_t s255 = (uint32_t)__shfl((int)incl, 63);
      // s254 = state behind lag 254 = the state in front of lane 63's last lag
      double best = 0.0;
      uint32_t arg = 0;
      uint32_t s_before_last = 0;
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t lag = lane * 4 + q;
        const uint32_t prev = st;
        if (q == 3) { s_before_last = prev; }
        st = prev ? (((dn >> q) & 1u) ^ 1u) : ((up >> q) & 1u);
        if ((prev | st) && ((lm >> q) & 1u)) {                                   // inside a segment (both ends inclusive), a local maximum
          const double v = s_acf[lag];
          if (v > best) { best = v; arg = lag; }
        }
      }
      const uint32_t s254 = (uint32_t)__shfl((int)s_before_last, 63);
      if (lane < 2) {
        const uint32_t lag = 256 + lane;
        const bool open = (s255 != 0) && lane == 0;                            // unterminated segment: [start, 256]
        const bool pseudo = (s255 == 0 && s254 == 0);                          // OUT with no upward crossing left: lags 256, 257
        if ((open || pseudo) && ((lm_hi >> lane) & 1u)) {
          const double v = s_acf[lag];
          if (v > best) { best = v; arg = lag; }
        }
      }
      // arg-max over the lanes: larger value, then smaller lag (every candidate is > 0; 0.0 = none)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off);
        const uint32_t oa = (uint32_t)__shfl_xor((int)arg, off);
        if (ov > best || (ov == best && ov > 0.0 && oa < arg)) { best = ov; arg = oa; }
      }
      double* o = out + (uint64_t)job * SLA_HIP_ACF_RECORD;
      const bool live = fabs(s_acf[0]) > (double)FLT_MIN;
      const uint32_t chosen = live ? arg : 0u;
      if (lane == 0) { o[0] = !live ? 0.0 : ((best > 0.0) ? 1.0 : 2.0); o[1] = (double)chosen; }      // 0: silent block, 2: no pitch candidate
      if (lane < 5) { o[2 + lane] = s_acf[lane]; }
      if (lane >= 8 && lane < 13) { const uint32_t k = lane - 8; o[7 + k] = (chosen + k >= 2) ? s_acf[chosen + k - 2] : 0.0; }
    }
  } else {
    for (uint32_t t = threadIdx.x; t < head; t += THREADS) { out[(uint64_t)job * head + t] = acf_at(z, t); }
  }
}

template <bool IN_LDS>
__global__ __launch_bounds__(ACF_THREADS)
void k_ltm_acf(const int32_t* __restrict__ res, uint64_t stride, const sla_hip_acf_job* __restrict__ jobs,
               uint32_t njobs, uint32_t log2F, const double* __restrict__ tw, double* __restrict__ scratch,
               double* __restrict__ out, uint32_t head, unsigned long long* span,
               const uint32_t* __restrict__ list, const uint32_t* __restrict__ list_count)
{
  extern __shared__ double2 lds2[];
  span_begin(span);
  __shared__ double s_acf[ACF_PICK_LAGS];
  __shared__ unsigned long long s_mask[3][ACF_PICK_LAGS / 64];
  const uint32_t F = 1u << log2F, npts = F >> 1, log2npts = log2F - 1;
  double2* z = IN_LDS ? lds2 : reinterpret_cast<double2*>(scratch + (uint64_t)blockIdx.x * F);
  const double* twr_f = tw;            const double* twi_f = tw + (F >> 1);
  const double* twr_i = tw + F;        const double* twi_i = tw + F + (F >> 1);
  const double* rtr_f = tw + 2 * F;    const double* rti_f = rtr_f + (F >> 2);
  const double* rtr_i = rti_f + (F >> 2); const double* rti_i = rtr_i + (F >> 2);
  const double scale = 4.656612873077392578125e-10;   // 2^-31

  // list != nullptr: the jobs list[0 .. *list_count) instead of 0 .. njobs (the certified route's fallback; bit 31 = audited)
  if (list != nullptr) { njobs = *list_count; }
  for (uint32_t it = blockIdx.x; it < njobs; it += gridDim.x) {
    const uint32_t job = (list != nullptr) ? (list[it] & 0x7FFFFFFFu) : it;
    const sla_hip_acf_job jb = jobs[job];
    const int32_t* src = res + (uint64_t)jb.channel * stride + jb.blk_off;
    const uint32_t n = jb.blk_len;
    // load, zero-padded, straight into bit-reversed complex order
    for (uint32_t k = threadIdx.x; k < npts; k += ACF_THREADS) {
      const uint32_t j = __brev(k) >> (32 - log2npts);
      z[acf_sw(j)] = make_double2((2 * k < n) ? (double)src[2 * k] * scale : 0.0,
                                  (2 * k + 1 < n) ? (double)src[2 * k + 1] * scale : 0.0);
    }
    __syncthreads();
    acf_stages(z, log2npts, twr_f, twi_f);
    acf_real_pass(z, npts, -0.5, rtr_f, rti_f);
    __syncthreads();
    if (threadIdx.x == 0) {
      const double2 v = z[0];
      const double s0 = v.x + v.y, s1 = v.x - v.y;
      z[0] = make_double2(s0 * s0, s1 * s1);           // DC and Nyquist power
    }
    for (uint32_t i = 1 + threadIdx.x; i < npts; i += ACF_THREADS) {
      const double2 v = z[acf_sw(i)];
      z[acf_sw(i)] = make_double2(v.x * v.x + v.y * v.y, 0.0);
    }
    __syncthreads();
    acf_real_pass(z, npts, 0.5, rtr_i, rti_i);
    __syncthreads();
    if (threadIdx.x == 0) {
      const double2 v = z[0];
      z[0] = make_double2(0.5 * (v.x + v.y), 0.5 * (v.x - v.y));
    }
    __syncthreads();
    // in-place bit reversal, then the inverse stages
    for (uint32_t k = threadIdx.x; k < npts; k += ACF_THREADS) {
      const uint32_t j = __brev(k) >> (32 - log2npts);
      if (j > k) {
        const double2 a = z[acf_sw(k)], b = z[acf_sw(j)];
        z[acf_sw(k)] = b; z[acf_sw(j)] = a;
      }
    }
    __syncthreads();
    acf_stages(z, log2npts, twr_i, twi_i);
    acf_emit<ACF_THREADS>(z, job, out, head, s_acf, s_mask);
    __syncthreads();
  }
  span_end(span);
}

// ---------------------------------------------------------------------------------------------
// k_ltm_acf2: the same transform pair with fewer trips through the LDS (every butterfly is still the reference's
// radix-2 one on the same operands: bit for bit the results of k_ltm_acf).  Per job and 2^L complex points:
//   * the first three forward stages take their operands straight from the residual plane: the point at bit-reversed
//     position 8b + m is sample pair t + rev3(m) * 2^(L-3) when b = rev(t), so consecutive lanes read consecutive
//     samples, the zero padding costs no loads, and the scatter pass of k_ltm_acf is gone;
//   * forward recombination, power spectrum, inverse recombination and the inverse transform's bit reversal are ONE
//     pass: every step keeps the pair (i, N - i) to itself, so a thread carries its pairs through all of them in
//     registers, a barrier separates all reads from all (bit-reversed) writes -- four passes of k_ltm_acf;
//   * the record only needs autocorrelation lags 0 .. 259 (pitch <= 257, five taps): the last inverse passes only
//     compute the groups, and store the points, those lags depend on (`need` complex slots).
// LDS round trips per job at L = 13: 4 + 1 + ~3.9 instead of 15.
// ---------------------------------------------------------------------------------------------
typedef int32_t i32x2_u __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// one twiddle = one 16-byte buffer load from the table of (re, im) pairs: byte offset = per-lane part (VGPR) + a part that
// is the same for every lane (SGPR / literal) -- no address arithmetic per load (the split tables cost two 8-byte loads with
// 64-bit address arithmetic each: as many instructions as the butterfly they feed)
__device__ __forceinline__ double2 acf2_tw(__amdgpu_buffer_rsrc_t rsrc, uint32_t lane_bytes, uint32_t uniform_bytes)
{
  const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_bytes, uniform_bytes, 0);
  return make_double2(__hiloint2double((int)v.y, (int)v.x), __hiloint2double((int)v.w, (int)v.z));
}

#define ACF2_NEED 162u        // complex slots that hold lags 0 .. 323: what acf_emit reads for the compact record

template <int R, int L, int THREADS, bool FAST = false>
__device__ __forceinline__ void acf2_first_pass(double2* z, const int32_t* __restrict__ src, uint32_t n,
                                                const double* __restrict__ twr, const double* __restrict__ twi)
{
  constexpr uint32_t P = 1u << R, ngroups = 1u << (L - R);
  const double scale = 4.656612873077392578125e-10;   // 2^-31
  uint32_t tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
#pragma unroll 1
  for (uint32_t it = 0; it < (ngroups + THREADS - 1) / THREADS; it++) {
    const uint32_t t = tid + it * THREADS;
    if (t >= ngroups) { break; }
    const uint32_t b = __brev(t) >> (32 - (L - R));
    // Position P*b + m holds complex sample c = t + rev(m) * ngroups.  An odd m has rev(m) >= P/2, i.e. c >= npts/2: beyond any
    // block (blk_len <= capacity = npts), always zero padding.  The first stage pairs (m, m + 1) under the twiddle (1, 0): with
    // zq = +0 the reference's products and sums give tr = ti = +0 and both results equal zi bit for bit (an input is
    // (double)int * 2^-31, never -0): the stage is a copy, and the odd positions are neither loaded nor multiplied.
    double2 v[P];
#pragma unroll
    for (uint32_t m = 0; m < P; m += 2) {
      const uint32_t c = t + (__brev(m) >> (32 - R)) * ngroups;          // complex sample index of position P*b + m
      if (2 * c + 1 < n) {
        const i32x2_u w = *(const i32x2_u*)(src + 2 * c);
        v[m] = make_double2((double)w.x * scale, (double)w.y * scale);
      } else {
        v[m] = make_double2((2 * c < n) ? (double)src[2 * c] * scale : 0.0, 0.0);
      }
      v[m + 1] = v[m];
    }
    if (n > (1u << L)) {
      // (a caller of the launcher with blocks longer than half the transform: the odd positions hold samples; wave-uniform)
#pragma unroll
      for (uint32_t m = 1; m < P; m += 2) {
        const uint32_t c = t + (__brev(m) >> (32 - R)) * ngroups;
        v[m] = make_double2((2 * c < n) ? (double)src[2 * c] * scale : 0.0, (2 * c + 1 < n) ? (double)src[2 * c + 1] * scale : 0.0);
        acf_bfly_sel<FAST>(v[m - 1], v[m], twr[0], twi[0]);
      }
    }
#pragma unroll
    for (int st = 1; st < R; st++) {
      constexpr uint32_t one = 1u;
      const uint32_t hs = one << st;
#pragma unroll
      for (uint32_t m = 0; m < P; m++) {
        if ((m >> st) & 1u) { continue; }
        const uint32_t k = m & ((1u << st) - 1u);
        acf_bfly_sel<FAST>(v[m], v[m + (1u << st)], twr[hs - 1 + k], twi[hs - 1 + k]);      // the same twiddle in every lane: scalar loads
      }
    }
    const uint32_t a0 = acf_sw(P * b);                                    // (m < 8 is its own swizzle)
#pragma unroll
    for (uint32_t m = 0; m < P; m++) { z[a0 ^ m] = v[m]; }
  }
  __syncthreads();
}

// R radix-2 stages (half-spans h = 2^LOG2H, 2h, ..) in one trip through the LDS, every number the compiler can know a
// template parameter: the trip counts are 1 - 4, so whatever is computed per pass at run time (swizzle constants, twiddle
// offsets, loop bounds) is not amortised -- in the run-time form three of four issued instructions were such overhead.
//   * acf_sw is linear over GF(2) and the bits of m * h are clear in ci: acf_sw(ci + m * h) = acf_sw(ci) ^ acf_sw(m * h),
//     the second factor a literal;
//   * PRUNE (the compact record only needs the slots [0, ACF2_NEED) of the inverse transform): after this pass the
//     remaining stages only combine points whose positions agree modulo H = h << R, so only the positions p with
//     (p mod H) < need matter: groups beyond them are skipped, points beyond them not stored.
template <int R, int LOG2H, int L, int THREADS, bool INV, bool PRUNE, bool FAST = false>
__device__ __forceinline__ void acf2_pass(double2* z, __amdgpu_buffer_rsrc_t tw2)
{
  constexpr uint32_t P = 1u << R, h = 1u << LOG2H, H = h << R, npts = 1u << L, groups = npts >> R;
  constexpr uint32_t tw_base = INV ? npts : 0u;                             // first pair of this direction's stage table
  constexpr bool prune = PRUNE && (H > ACF2_NEED);
  constexpr uint32_t live_groups = (prune && h >= ACF2_NEED) ? (groups / h) * ACF2_NEED : groups;   // (only counts the work)
  (void)live_groups;
  // (an opaque copy of the thread number per pass: otherwise the addresses of EVERY pass are computed in front of the first
  // one -- the passes of a 4096-point job are straight-line code -- and held in registers, or spilled, until they are used)
  uint32_t tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
#pragma unroll 1
  for (uint32_t it = 0; it < (groups + THREADS - 1) / THREADS; it++) {
    // pruned passes with h >= need: renumber the groups so that the live ones (low < need) are dense over the threads
    uint32_t low, blk;
    if (prune && h >= ACF2_NEED) {
      constexpr uint32_t per = ACF2_NEED;                                   // live groups per block of h
      const uint32_t g = tid + it * THREADS;
      if (it * THREADS >= (groups / h) * per) { break; }
      if (g >= (groups / h) * per) { continue; }
      blk = g / per; low = g - blk * per;
    } else {
      const uint32_t b = tid + it * THREADS;
      if (groups % THREADS != 0 && b >= groups) { continue; }
      low = b & (h - 1); blk = b >> LOG2H;
    }
    const uint32_t ci = low + (blk << (LOG2H + R));
    const uint32_t a0 = acf_sw(ci);
    double2 v[P];
#pragma unroll
    for (uint32_t m = 0; m < P; m++) { v[m] = z[a0 ^ acf_sw(m << LOG2H)]; }
#pragma unroll
    for (int st = 0; st < R; st++) {
      const uint32_t hs = h << st;
#pragma unroll
      for (uint32_t m = 0; m < P; m++) {
        if ((m >> st) & 1u) { continue; }
        // twiddle hs - 1 + low + (m mod 2^st) * h of this direction's table
        const double2 w = acf2_tw(tw2, low << 4, (tw_base + hs - 1 + (m & ((1u << st) - 1u)) * h) << 4);
        acf_bfly_sel<FAST>(v[m], v[m + (1u << st)], w.x, w.y);
      }
    }
#pragma unroll
    for (uint32_t m = 0; m < P; m++) { if (!prune || low + m * h < ACF2_NEED) { z[a0 ^ acf_sw(m << LOG2H)] = v[m]; } }
  }
  __syncthreads();
}

// the stage schedule of one direction from half-span 2^LOG2H on: passes of three stages, the tail as 2 + 2 or 2
template <int LOG2H, int L, int THREADS, bool INV, bool PRUNE, bool FAST = false>
__device__ __forceinline__ void acf2_stages(double2* z, __amdgpu_buffer_rsrc_t tw2)
{
  constexpr int left = L - LOG2H;
  if constexpr (left >= 3 && left != 4) {
    acf2_pass<3, LOG2H, L, THREADS, INV, PRUNE, FAST>(z, tw2);
    acf2_stages<LOG2H + 3, L, THREADS, INV, PRUNE, FAST>(z, tw2);
  } else if constexpr (left >= 2) {
    acf2_pass<2, LOG2H, L, THREADS, INV, PRUNE, FAST>(z, tw2);
    acf2_stages<LOG2H + 2, L, THREADS, INV, PRUNE, FAST>(z, tw2);
  } else if constexpr (left == 1) {
    acf2_pass<1, LOG2H, L, THREADS, INV, PRUNE, FAST>(z, tw2);
  }
}

// the recombination of the reference's realft (src/SLAUtility.c:262-312) on the pair A = slot i-1, B = slot npts-(i-1):
// the expressions of acf_real_pass, operation for operation
__device__ __forceinline__ void acf2_recombine(double2& A, double2& B, double c2, double wr, double wi)
{
  const double c1 = 0.5;
  const double h1r = c1 * (A.x + B.x);
  const double h1i = c1 * (A.y - B.y);
  const double h2r = -c2 * (A.y + B.y);
  const double h2i = c2 * (A.x - B.x);
  A = make_double2(h1r + wr * h2r - wi * h2i, h1i + wr * h2i + wi * h2r);
  B = make_double2(h1r - wr * h2r + wi * h2i, -h1i + wr * h2i + wi * h2r);
}

// (the certified route's form: the same expressions with the products fused into the sums)
__device__ __forceinline__ void acf2_recombine_fma(double2& A, double2& B, double c2, double wr, double wi)
{
  const double h1r = 0.5 * (A.x + B.x);
  const double h1i = 0.5 * (A.y - B.y);
  const double h2r = -c2 * (A.y + B.y);
  const double h2i = c2 * (A.x - B.x);
  const double pr = fma(wr, h2r, -(wi * h2i)), pi = fma(wr, h2i, wi * h2r);
  A = make_double2(h1r + pr, h1i + pi);
  B = make_double2(h1r - pr, pi - h1i);
}

template <int L, int THREADS, bool FAST = false>
__device__ __forceinline__ void acf2_middle(double2* z, __amdgpu_buffer_rsrc_t tw2)
{
  // Thread tid takes the pairs (A = slot c, B = slot npts - c), c = tid + k THREADS in 1 .. npts/2 - 1 (c = 0: the DC / Nyquist
  // slot and the middle slot no pair touches, thread 0).  The swizzle is linear over GF(2) and tid, k THREADS share no bit:
  //   slot c            = tid ^ (k THREADS)                       -> S(tid) ^ literal
  //   slot npts - c     = u ^ ((Q - 1 - k) THREADS), u = THREADS - tid, Q = npts / THREADS   (tid = 0: (Q - k) THREADS, u = 0)
  // and the bit-reversed places of the scatter likewise (bit reversal is linear too): four swizzles per thread at run time
  // instead of four per pair (round 3 took c = tid + 1 + k THREADS, whose carry defeats this; its run also started one slot
  // off the 16-slot grid: two-way conflicts on every read of A).
  constexpr uint32_t npts = 1u << L, half = npts >> 1, K = half / THREADS, Q = npts / THREADS;
  static_assert(half % THREADS == 0 && K >= 1, "pairs per thread");
  double2 A[K], B[K];
  uint32_t tid = threadIdx.x;                                               // (opaque per phase, as in acf2_pass)
  asm volatile("" : "+v"(tid));
  const uint32_t u = (THREADS - tid) & (THREADS - 1u);
  const bool t0 = (tid == 0u);
  const uint32_t sa = acf_sw(tid), sb = acf_sw(u);
#pragma unroll
  for (uint32_t k = 0; k < K; k++) {
    if (k > 0 || !t0) {
      A[k] = z[sa ^ acf_sw(k * THREADS)];
      B[k] = z[sb ^ (t0 ? acf_sw((Q - k) * THREADS) : acf_sw((Q - 1u - k) * THREADS))];
    }
  }
  double2 dc = make_double2(0.0, 0.0), mid = make_double2(0.0, 0.0);
  if (threadIdx.x == 0) { dc = z[0]; mid = z[acf_sw(half)]; }
#pragma unroll
  for (uint32_t k = 0; k < K; k++) {
    if (k > 0 || !t0) {
      // recombination twiddles: pairs [2 npts, 2 npts + npts/2) forward, the next npts/2 inverse; entry c - 1 of either
      const double2 wf = acf2_tw(tw2, tid << 4, (2u * npts + k * THREADS - 1u) << 4);
      const double2 wi = acf2_tw(tw2, tid << 4, (2u * npts + half + k * THREADS - 1u) << 4);
      if constexpr (FAST) {
        acf2_recombine_fma(A[k], B[k], -0.5, wf.x, wf.y);
        A[k] = make_double2(fma(A[k].x, A[k].x, A[k].y * A[k].y), 0.0);
        B[k] = make_double2(fma(B[k].x, B[k].x, B[k].y * B[k].y), 0.0);
        acf2_recombine_fma(A[k], B[k], 0.5, wi.x, wi.y);
      } else {
        acf2_recombine(A[k], B[k], -0.5, wf.x, wf.y);
        A[k] = make_double2(A[k].x * A[k].x + A[k].y * A[k].y, 0.0);       // power spectrum  src/SLAPredictor.c:844-851
        B[k] = make_double2(B[k].x * B[k].x + B[k].y * B[k].y, 0.0);
        acf2_recombine(A[k], B[k], 0.5, wi.x, wi.y);
      }
    }
    __builtin_amdgcn_sched_barrier(0);          // one pair at a time: hoisting every pair's twiddles and temporaries costs spills
  }
  if (threadIdx.x == 0) {
    const double s0 = dc.x + dc.y, s1 = dc.x - dc.y;
    const double2 pw = make_double2(s0 * s0, s1 * s1);                   // DC and Nyquist power  :839-842
    dc = make_double2(0.5 * (pw.x + pw.y), 0.5 * (pw.x - pw.y));
    mid = make_double2(mid.x * mid.x + mid.y * mid.y, 0.0);              // the slot no pair touches
  }
  __syncthreads();                                                        // every read above is done: the slots may be overwritten
  asm volatile("" : "+v"(tid));
  // rev_L(tid ^ k THREADS) = rev_L(tid) ^ rev_L(k THREADS)
  const uint32_t ra = acf_sw(__brev(tid) >> (32 - L)), rb = acf_sw(__brev(u) >> (32 - L));
#pragma unroll
  for (uint32_t k = 0; k < K; k++) {
    if (k > 0 || !t0) {
      z[ra ^ acf_sw(__brev(k * THREADS) >> (32 - L))] = A[k];
      z[rb ^ (t0 ? acf_sw(__brev((Q - k) * THREADS) >> (32 - L)) : acf_sw(__brev((Q - 1u - k) * THREADS) >> (32 - L)))] = B[k];
    }
  }
  if (threadIdx.x == 0) { z[0] = dc; z[acf_sw(1)] = mid; }                // rev(0) = 0, rev(npts/2) = 1
  __syncthreads();
}

// <= 128 registers: four waves per SIMD (two workgroups of 512 threads on 64 KiB of LDS each, or one of 1024 on 128 KiB)
template <int L, int ACF2_THREADS, bool RECORD>
__global__ __launch_bounds__(ACF2_THREADS, 4)
void k_ltm_acf2(const int32_t* __restrict__ res, uint64_t stride, const sla_hip_acf_job* __restrict__ jobs,
                uint32_t njobs, const double* __restrict__ tw, double* __restrict__ out, uint32_t head, unsigned long long* span)
{
  extern __shared__ double2 lds2[];
  span_begin(span);
  __shared__ double s_acf[ACF_PICK_LAGS];
  __shared__ unsigned long long s_mask[3][ACF_PICK_LAGS / 64];
  constexpr uint32_t npts = 1u << L, F = npts << 1;
  double2* z = lds2;
  const double* twr_f = tw;            const double* twi_f = tw + (F >> 1);      // split tables: the first pass (same twiddles in every lane)
  // the table of (re, im) pairs behind the split ones: [0, npts) forward stages | [npts, 2 npts) inverse | recombination
  const __amdgpu_buffer_rsrc_t tw2 = __builtin_amdgcn_make_buffer_rsrc((void*)(tw + 3 * (size_t)F), 0, (int)(3u * F * sizeof(double)), 0x00020000);
  for (uint32_t job = blockIdx.x; job < njobs; job += gridDim.x) {
    const sla_hip_acf_job jb = jobs[job];
    const int32_t* src = res + (uint64_t)jb.channel * stride + jb.blk_off;
    acf2_first_pass<3, L, ACF2_THREADS>(z, src, jb.blk_len, twr_f, twi_f);
    acf2_stages<3, L, ACF2_THREADS, false, false>(z, tw2);
    acf2_middle<L, ACF2_THREADS>(z, tw2);
    acf2_stages<0, L, ACF2_THREADS, true, RECORD>(z, tw2);
    acf_emit<ACF2_THREADS>(z, job, out, head, s_acf, s_mask);
    __syncthreads();
  }
  span_end(span);
}

// k_ltm_acf2 over a device-resident list of jobs (the certified route's fallback and its audit): a fixed small grid walks
// list[0 .. *count); bit 31 of an entry marks an audited job (k_ltm_solve_list compares instead of replacing).
#define LTM_LIST_AUDIT 0x80000000u
template <int L, int ACF2_THREADS>
__global__ __launch_bounds__(ACF2_THREADS, 4)
void k_ltm_acf2_list(const int32_t* __restrict__ res, uint64_t stride, const sla_hip_acf_job* __restrict__ jobs,
                     const uint32_t* __restrict__ list, const uint32_t* __restrict__ count, const double* __restrict__ tw,
                     double* __restrict__ out, unsigned long long* span)
{
  extern __shared__ double2 lds2[];
  __shared__ double s_acf[ACF_PICK_LAGS];
  __shared__ unsigned long long s_mask[3][ACF_PICK_LAGS / 64];
  constexpr uint32_t npts = 1u << L, F = npts << 1;
  double2* z = lds2;
  const uint32_t n_list = *count;
  if (n_list == 0) { return; }                           // (the usual case: nothing recorded in the span either)
  const __amdgpu_buffer_rsrc_t tw2 = __builtin_amdgcn_make_buffer_rsrc((void*)(tw + 3 * (size_t)F), 0, (int)(3u * F * sizeof(double)), 0x00020000);
  for (uint32_t i = blockIdx.x; i < n_list; i += gridDim.x) {
    const uint32_t job = list[i] & ~LTM_LIST_AUDIT;
    const sla_hip_acf_job jb = jobs[job];
    const int32_t* src = res + (uint64_t)jb.channel * stride + jb.blk_off;
    acf2_first_pass<3, L, ACF2_THREADS>(z, src, jb.blk_len, tw, tw + (F >> 1));
    acf2_stages<3, L, ACF2_THREADS, false, false>(z, tw2);
    acf2_middle<L, ACF2_THREADS>(z, tw2);
    acf2_stages<0, L, ACF2_THREADS, true, true>(z, tw2);
    acf_emit<ACF2_THREADS>(z, job, out, SLA_HIP_ACF_RECORD, s_acf, s_mask);
    __syncthreads();
  }
  span_end(span);
}

// ---------------------------------------------------------------------------------------------
// k_ltm_acf_fast: the certified route's autocorrelation.  Nothing downstream reads the reference's bits: the record only
// feeds decisions (sign and neighbour comparisons of the pitch scan, an arg-max, a small Toeplitz solve, a 15-bit
// quantiser), so the transform may run in any order with fused multiply-adds as long as every decision is proven to come
// out as the reference's -- acf_emit_cert and k_ltm_solve_cert prove it under |r' - r_ref| <= eps, and what they cannot
// prove goes through k_ltm_acf2_list / k_ltm_solve_list.
//   * Transform size: H = 2^(l+1) >= blk_len real points instead of the reference's F = roundup2(2 * capacity).  The
//     circular autocorrelation of size H differs from the linear one by the wrap term
//         r[k] = c[k] - sum_{m < k - (H - n)} x[H - k + m] x[m]          (at most k terms, only when n > H - k)
//     which the workgroup adds up from the block's first and last ACF_WRAP_LAGS samples (four lags per thread).  A block shorter than
//     H - ACF_WRAP_LAGS has no wrap term at all (the smallest H is 2048, so every short last block).
//   * Twiddles: a table of its own per size (slai_fft_fast_export: cos / sin evaluated in double, the layout of the exact
//     table), the passes and the LDS swizzle of k_ltm_acf2 with FMA butterflies.
//   * The result is scaled to the reference's: its inverse transform is unnormalised, r_ref[k] = F/2 * sum x x.
// The workgroup picks l from blk_len: a workgroup-uniform branch over the instantiated sizes.
// ---------------------------------------------------------------------------------------------
#define ACF_WRAP_LAGS 264u          // lags the record can touch: pitch <= 257, + 2 taps, + the neighbour the scan compares with
#define ACF_FAST_LAGS 324u          // lags the pruned inverse leaves valid (ACF2_NEED slots)
#define ACF_FAST_TW_OFFSET(l, lmin) (12u * ((size_t)(1u << (l)) - (size_t)(1u << (lmin))))     // tables of the smaller sizes in front: 6 * 2^(q+1) doubles each

template <int L, int THREADS>
__device__ __forceinline__ void acf_fast_transform(double2* z, const int32_t* __restrict__ src, uint32_t n, const double* __restrict__ tw)
{
  constexpr uint32_t F = 2u << L;
  const __amdgpu_buffer_rsrc_t tw2 = __builtin_amdgcn_make_buffer_rsrc((void*)(tw + 3 * (size_t)F), 0, (int)(3u * F * sizeof(double)), 0x00020000);
  acf2_first_pass<3, L, THREADS, true>(z, src, n, tw, tw + (F >> 1));
  acf2_stages<3, L, THREADS, false, false, true>(z, tw2);
  acf2_middle<L, THREADS, true>(z, tw2);
  acf2_stages<0, L, THREADS, true, true, true>(z, tw2);
}

// acf_emit with the certificate: s_r holds r'[0 .. ACF_FAST_LAGS), eps = eps_rel * r'[0] bounds |r' - r_ref| at every lag.
// The record is certified (eps_out >= 0) only if every predicate the scan can evaluate is safe: |r'[j]| > eps for the
// lags 0 .. 258 (signs), |r'[j] - r'[j-1]| > 2 eps for 1 .. 258 (neighbour comparisons), the winning peak above every
// other candidate by more than 2 eps, r'[0] - eps > FLT_MIN.  An all-zero block is exact (r'[0] == 0: silent).
template <int THREADS>
__device__ __forceinline__ void acf_emit_cert(const double* s_r, uint32_t job, double* __restrict__ out, double* __restrict__ eps_out,
                                              double eps_rel, bool size_ok, unsigned long long (*s_mask)[ACF_PICK_LAGS / 64])
{
  const double eps = eps_rel * s_r[0];
  for (uint32_t j = threadIdx.x; j < ACF_PICK_LAGS; j += THREADS) {             // (whole waves: 320 = 5 x 64)
    const double vc = s_r[j], vm = (j >= 1) ? s_r[j - 1] : 0.0, vp = s_r[j + 1];
    const unsigned long long bu = __ballot(j >= 1 && j < 256 && vm < 0.0 && vc > 0.0);
    const unsigned long long bd = __ballot(j >= 1 && j < 256 && vc > 0.0 && vp < 0.0);
    const unsigned long long bl = __ballot(j >= 1 && j <= 257 && vc > vm && vc > vp && vc > 0.0);
    // (negated comparisons: a NaN or an infinity anywhere is unsafe)
    const unsigned long long bx = __ballot(j <= 258 && (!(fabs(vc) > eps) || (j >= 1 && !(fabs(vc - vm) > 2.0 * eps))));
    if ((j & 63) == 0) { s_mask[0][j >> 6] = bu; s_mask[1][j >> 6] = bd; s_mask[2][j >> 6] = bl; s_mask[3][j >> 6] = bx; }
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const uint32_t lane = threadIdx.x;
    const uint32_t w = lane >> 4, sh = (lane & 15u) * 4;
    const uint32_t up = (uint32_t)(s_mask[0][w] >> sh) & 15u, dn = (uint32_t)(s_mask[1][w] >> sh) & 15u;
    const uint32_t lm = (uint32_t)(s_mask[2][w] >> sh) & 15u;
    const uint32_t lm_hi = (uint32_t)s_mask[2][4] & 3u;
    bool unsafe = ((s_mask[3][0] | s_mask[3][1] | s_mask[3][2] | s_mask[3][3] | s_mask[3][4]) != 0ull) || !size_ok;
    uint32_t f = 0;
#pragma unroll
    for (uint32_t s0 = 0; s0 < 2; s0++) {
      uint32_t st = s0;
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) { st = st ? (((dn >> q) & 1u) ^ 1u) : ((up >> q) & 1u); }
      f |= st << s0;
    }
    uint32_t g = f;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t below = (uint32_t)__shfl_up((int)g, d);
      if (lane >= d) { g = ((g >> (below & 1u)) & 1u) | (((g >> ((below >> 1) & 1u)) & 1u) << 1); }
    }
    const uint32_t incl = g & 1u;
    uint32_t st = (uint32_t)__shfl_up((int)incl, 1);
    if (lane == 0) { st = 0; }
    const uint32_t s255 = (uint32_t)__shfl((int)incl, 63);
    double best = 0.0;
    uint32_t arg = 0, cand = 0, s_before_last = 0;      // cand: bits 0..3 this lane's lags, bit 4 lag 256 + lane
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      const uint32_t lag = lane * 4 + q;
      const uint32_t prev = st;
      if (q == 3) { s_before_last = prev; }
      st = prev ? (((dn >> q) & 1u) ^ 1u) : ((up >> q) & 1u);
      if ((prev | st) && ((lm >> q) & 1u)) {
        const double v = s_r[lag];
        cand |= 1u << q;
        if (v > best) { best = v; arg = lag; }
      }
    }
    const uint32_t s254 = (uint32_t)__shfl((int)s_before_last, 63);
    if (lane < 2) {
      const uint32_t lag = 256 + lane;
      const bool open = (s255 != 0) && lane == 0;
      const bool pseudo = (s255 == 0 && s254 == 0);
      if ((open || pseudo) && ((lm_hi >> lane) & 1u)) {
        const double v = s_r[lag];
        cand |= 16u;
        if (v > best) { best = v; arg = lag; }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(best, off);
      const uint32_t oa = (uint32_t)__shfl_xor((int)arg, off);
      if (ov > best || (ov == best && ov > 0.0 && oa < arg)) { best = ov; arg = oa; }
    }
    // the winner must stand clear of every other candidate: a tie, or anything within 2 eps of it, is not decided here
    bool close = false;
#pragma unroll
    for (uint32_t q = 0; q < 5; q++) {
      const uint32_t lag = (q < 4) ? lane * 4 + q : 256 + lane;
      if (((cand >> q) & 1u) && lag != arg && !(s_r[lag] < best - 2.0 * eps)) { close = true; }
    }
    if (__ballot(close) != 0ull) { unsafe = true; }
    const double r0 = s_r[0];
    const bool silent = (r0 == 0.0);                                         // exact: every sample of the block is zero
    const bool live = fabs(r0) > (double)FLT_MIN;
    if (!silent && !(r0 - eps > 2.0 * (double)FLT_MIN)) { unsafe = true; }
    const uint32_t chosen = live ? arg : 0u;
    double* o = out + (uint64_t)job * SLA_HIP_ACF_RECORD;
    if (lane == 0) {
      o[0] = !live ? 0.0 : ((best > 0.0) ? 1.0 : 2.0); o[1] = (double)chosen;
      eps_out[job] = (silent || !unsafe) ? eps : -1.0;
    }
    if (lane < 5) { o[2 + lane] = s_r[lane]; }
    if (lane >= 8 && lane < 13) { const uint32_t k = lane - 8; o[7 + k] = (chosen + k >= 2) ? s_r[chosen + k - 2] : 0.0; }
  }
}

template <int LTOP, int THREADS>
__global__ __launch_bounds__(THREADS, 4)
void k_ltm_acf_fast(const int32_t* __restrict__ res, uint64_t stride, const sla_hip_acf_job* __restrict__ jobs,
                    uint32_t njobs, const double* __restrict__ tw_fast, double* __restrict__ out, double* __restrict__ eps_out,
                    double eps_rel, unsigned long long* span)
{
  extern __shared__ double2 lds2[];
  span_begin(span);
  // THREADS = 2^(LTOP - 3): one radix-8 group per thread in the largest transform's passes (with more, half the workgroup
  // idles in every pass of a half-size transform and the kernel, bound by the latency of its passes, gains nothing)
  static_assert(THREADS == (1 << (LTOP - 3)), "threads per workgroup");
  constexpr int LMIN = (THREADS == 1024) ? 11 : 10;      // acf2_middle: at least one pair per thread; H >= 2048: a short last block has no wrap term
  static_assert(LTOP >= LMIN && LTOP <= LMIN + 2, "sizes instantiated below");
  __shared__ double s_r[ACF_FAST_LAGS + 4];
  __shared__ double s_head[ACF_WRAP_LAGS], s_tail[ACF_WRAP_LAGS + 8];
  __shared__ unsigned long long s_mask[4][ACF_PICK_LAGS / 64];
  double2* z = lds2;
  const double scale = 4.656612873077392578125e-10;   // 2^-31
  for (uint32_t job = blockIdx.x; job < njobs; job += gridDim.x) {
    const sla_hip_acf_job jb = jobs[job];
    const int32_t* src = res + (uint64_t)jb.channel * stride + jb.blk_off;
    const uint32_t n = jb.blk_len;
    uint32_t l = LMIN;
    while ((2u << l) < n && l < (uint32_t)LTOP) { l++; }
    const uint32_t H = 2u << l;
    const bool size_ok = (n <= H);                         // (a block beyond the capacity the kernel was built for: never certified)
    const double* tw = tw_fast + ACF_FAST_TW_OFFSET(l, LMIN);
    if (l == (uint32_t)LMIN) { acf_fast_transform<LMIN, THREADS>(z, src, n, tw); }
    else if constexpr (LTOP >= LMIN + 1) {
      if (l == (uint32_t)LMIN + 1) { acf_fast_transform<LMIN + 1, THREADS>(z, src, n, tw); }
      else if constexpr (LTOP >= LMIN + 2) { acf_fast_transform<LMIN + 2, THREADS>(z, src, n, tw); }
    }
    // wrap term of the lags 0 .. ACF_WRAP_LAGS - 1 and the scale of the reference: r_ref = F/2 sum, circular = H/2 sum
    const bool wrap = size_ok && (n + ACF_WRAP_LAGS > H);      // (then n >= H - 264 >= 1784: both runs lie inside the block)
    if (wrap) {
      for (uint32_t t = threadIdx.x; t < 2 * ACF_WRAP_LAGS + 8; t += THREADS) {
        if (t < ACF_WRAP_LAGS) { s_head[t] = (double)src[t] * scale; }
        else if (t < 2 * ACF_WRAP_LAGS) { s_tail[t - ACF_WRAP_LAGS] = (double)src[n - 2 * ACF_WRAP_LAGS + t] * scale; }
        else { s_tail[t - ACF_WRAP_LAGS] = 0.0; }                                // (the window below reads zeros beyond the block's end)
      }
    }
    const double ratio = (double)(1u << ((uint32_t)LTOP + 1u - l));             // F / H
    for (uint32_t t = threadIdx.x; t < ACF_FAST_LAGS + 4; t += THREADS) { s_r[t] = (t < ACF_FAST_LAGS) ? ratio * acf_at(z, t) : 0.0; }
    __syncthreads();
    if (wrap) {
      // wrap[k] = sum_{m < k - d} tail[264 - (k - d) + m] head[m], d = H - n, tail[i] = x[n - 264 + i] (zero from 264 on),
      // head[m] = x[m].  Thread (g, c), g = tid / 8, c = tid % 8: the four lags k0 .. k0 + 3, k0 = 4 + 4 g (4 .. 259), over the
      // terms m = 33 c .. 33 c + 32.  Lag k0 + q reads tail[base + m - q], base = 264 - k0 + d: a window of four values that
      // slides by one per term -- one tail and one head value loaded per four FMAs; a term beyond its lag's count reads zeros.
      const double fhalf = (double)(2u << (uint32_t)LTOP);                      // F / 2
      const uint32_t d = H - n;
      for (uint32_t it = threadIdx.x; it < 512u; it += THREADS) {
        const uint32_t g = it >> 3, c = it & 7u, k0 = 4u + 4u * g, m0 = 33u * c;
        const uint32_t base = ACF_WRAP_LAGS - k0 + d + m0;                      // >= 5
        double w0 = s_tail[min(base, ACF_WRAP_LAGS)], w1 = s_tail[min(base - 1u, ACF_WRAP_LAGS)];
        double w2 = s_tail[min(base - 2u, ACF_WRAP_LAGS)], w3 = s_tail[min(base - 3u, ACF_WRAP_LAGS)];
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
        for (uint32_t i = 0; i < 33u; i++) {
          const double hm = s_head[min(m0 + i, ACF_WRAP_LAGS - 1u)];
          a0 = fma(hm, w0, a0); a1 = fma(hm, w1, a1); a2 = fma(hm, w2, a2); a3 = fma(hm, w3, a3);
          w3 = w2; w2 = w1; w1 = w0; w0 = s_tail[min(base + i + 1u, ACF_WRAP_LAGS)];
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
          a0 += __shfl_xor(a0, off); a1 += __shfl_xor(a1, off); a2 += __shfl_xor(a2, off); a3 += __shfl_xor(a3, off);
        }
        if (c < 4u) {
          const double acc = (c == 0u) ? a0 : (c == 1u) ? a1 : (c == 2u) ? a2 : a3;
          s_r[k0 + c] = fma(-fhalf, acc, s_r[k0 + c]);
        }
      }
      if (threadIdx.x >= 1u && threadIdx.x < 4u) {                              // lags 1 .. 3: at most three terms
        const uint32_t k = threadIdx.x, cnt = (k > d) ? (k - d) : 0u;
        double acc = 0.0;
        for (uint32_t m = 0; m < cnt; m++) { acc = fma(s_tail[ACF_WRAP_LAGS - cnt + m], s_head[m], acc); }
        if (cnt != 0u) { s_r[k] = fma(-fhalf, acc, s_r[k]); }
      }
      __syncthreads();
    }
    acf_emit_cert<THREADS>(s_r, job, out, eps_out, eps_rel, size_ok, s_mask);
    __syncthreads();
  }
  span_end(span);
}

// ---------------------------------------------------------------------------------------------
// k_ltm_acf_int: the same stage without a transform.  The record reads the lags 0 .. 263 of an int32 block only, and with
// every sample split into balanced base-256 digits, x = sum_a d_a 2^(8a), d_a in [-128, 127], the direct sum becomes a
// handful of int8 matrix products (v_mfma_i32_16x16x64_i8), exact in i32:
//   sample m = 16 kappa + i;  A_a[i][kappa] = d_a(x[16 kappa + i]);  B_b,s[kappa][c] = d_b(x[16 (kappa + s) + c]), s = 0 .. 17
//   C[i][c] = sum_kappa A_a B_b,s adds 2^(8(a+b)) C[i][c] to the lag k = 16 s + c - i        (s = 0: c >= i only)
// Every (m, k) with 0 <= k <= 263 occurs once.  All digit pairs of one weight w = a + b share an accumulator.
//   * digit count D = 1 .. 5 (workgroup-uniform): the first D after which no sample leaves a remainder; digits beyond D are zero
//   * LDS: plane a, row i, byte kappa (row stride RS = 64 NT + 48 bytes, RS / 16 odd; zeros behind the block).  Lane
//     (r, h) = (lane & 15, lane >> 4) holds bytes kappa = 64 T + 16 h .. + 15 of row r as its A fragment and the same bytes
//     from kappa + s on as its B fragment of shift s: A and B pair the same kappa in the same (h, byte), so which k the
//     instruction gives a byte does not matter.  The B fragments of a wave's shifts come out of one window of dwords by
//     v_alignbyte_b32.
//   * the four waves deal the 18 shifts out 5 / 5 / 4 / 4 (rotated by the job, so that no SIMD always gets five)
//   * headroom: |cell| <= pairs (<= 5) * 1024 kappa * 2^14 < 2^27; a lag's sum of one weight <= 5 * 16384 * 2^14 < 2^31:
//     the diagonals are added up in i32 (LDS atomics after a DPP sum over the four rows a lane holds)
//   * sum_w 2^(8w) S_w[k] in 128 bits, rounded to double ONCE (exact below 2^53), times 2^-62 F/2: the scale of
//     k_ltm_acf_fast's samples (2^-31 each) and of the reference's unnormalised inverse
// RAW: no pick, the scaled sums of the lags 0 .. 263 go to `out` (sla_hip_launch_ltm_acf_int, tests).
// ---------------------------------------------------------------------------------------------
#define ACF_INT_LAGS 264u
#define ACF_INT_SHIFTS 18
#define ACF_INT_THREADS 256
#define ACF_INT_ROW(nt) (64u * (nt) + 48u)                         // bytes of a digit row for nt tiles of 64 kappa
#define ACF_INT_LDS(cap) (5u * 16u * ACF_INT_ROW(((cap) + 1023u) / 1024u))

typedef int acf_i32x4 __attribute__((ext_vector_type(4)));

template <int R>
__device__ __forceinline__ int acf_int_row_from(int v)            // lane c of a row of 16 receives lane (c + R) % 16
{
  if constexpr (R == 0) { return v; }
  else { return __builtin_amdgcn_update_dpp(0, v, 0x120 + (16 - R), 0xF, 0xF, false); }      // row_ror:(16 - R)
}

template <int D, int S0, int S>
__device__ __forceinline__ void acf_int_shifts(const unsigned char* planes, uint32_t rs, uint32_t nt, uint32_t lane, int (*s_sum)[ACF_INT_LAGS + 8])
{
  constexpr int W = 2 * D - 1;
  constexpr int WOFF = S0 & ~3, SH0 = S0 & 3;
  constexpr int NW = ((SH0 + S - 1) >> 2) + 5;                      // dwords of the B window
  const uint32_t r = lane & 15u, h = lane >> 4;
  const uint32_t ps = 16u * rs;
  acf_i32x4 acc[S][W];
#pragma unroll
  for (int s = 0; s < S; s++) {
#pragma unroll
    for (int w = 0; w < W; w++) { acc[s][w] = acf_i32x4{0, 0, 0, 0}; }
  }
  const unsigned char* row = planes + r * rs + 16u * h;
  for (uint32_t t = 0; t < nt; t++, row += 64) {
    acf_i32x4 a[D];
    uint32_t win[D][NW];
#pragma unroll
    for (int d = 0; d < D; d++) {
      a[d] = *(const acf_i32x4*)(row + d * ps);
      const uint32_t* wp = (const uint32_t*)(row + d * ps + WOFF);
#pragma unroll
      for (int q = 0; q < NW; q++) { win[d][q] = wp[q]; }
    }
#pragma unroll
    for (int s = 0; s < S; s++) {
      const int off = SH0 + s, dw = off >> 2, sh = off & 3;
#pragma unroll
      for (int b = 0; b < D; b++) {
        acf_i32x4 f;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          f[j] = (sh == 0) ? (int)win[b][dw + j] : (int)__builtin_amdgcn_alignbyte(win[b][dw + j + 1], win[b][dw + j], (uint32_t)sh);
        }
#pragma unroll
        for (int d = 0; d < D; d++) { acc[s][d + b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[d], f, acc[s][d + b], 0, 0, 0); }
      }
    }
  }
  // C[i][c]: c = lane & 15, i = 4 (lane >> 4) + reg, lag 16 s + c - i.  Lane c takes reg R of lane (c + R) % 16: all four on
  // the diagonal c - 4 h, or, where c + R wrapped, on c - 16 - 4 h -- which is the diagonal c - 4 h of the shift before,
  // so inside a wave's run of shifts the wrapped part joins the next lower shift's sum in the lane's own register.
  const int kbase = 16 * S0 + (int)r - 4 * (int)h;
#pragma unroll
  for (int w = 0; w < W; w++) {
    int carry = 0;
#pragma unroll
    for (int s = S - 1; s >= 0; s--) {
      const int v1 = acf_int_row_from<1>(acc[s][w][1]), v2 = acf_int_row_from<2>(acc[s][w][2]), v3 = acf_int_row_from<3>(acc[s][w][3]);
      const int yw = ((r >= 15u) ? v1 : 0) + ((r >= 14u) ? v2 : 0) + ((r >= 13u) ? v3 : 0);
      const int ym = acc[s][w][0] + v1 + v2 + v3 - yw + carry;
      carry = yw;
      if ((uint32_t)(kbase + 16 * s) < ACF_INT_LAGS && ym != 0) { atomicAdd(&s_sum[w][kbase + 16 * s], ym); }
    }
    if ((uint32_t)(kbase - 16) < ACF_INT_LAGS && carry != 0) { atomicAdd(&s_sum[w][kbase - 16], carry); }
  }
}

template <int D, int S0, int S>
__device__ __forceinline__ void acf_int_range(const unsigned char* planes, uint32_t rs, uint32_t nt, uint32_t lane, int (*s_sum)[ACF_INT_LAGS + 8])
{
  // (D >= 4: 7 or 9 weights per shift -- two shifts' accumulators at a time, the planes are read more than once)
  if constexpr (D >= 4 && S > 2) {
    acf_int_shifts<D, S0, 2>(planes, rs, nt, lane, s_sum);
    acf_int_range<D, S0 + 2, S - 2>(planes, rs, nt, lane, s_sum);
  } else {
    acf_int_shifts<D, S0, S>(planes, rs, nt, lane, s_sum);
  }
}

template <int D>
__device__ __forceinline__ void acf_int_products(const unsigned char* planes, uint32_t rs, uint32_t nt, uint32_t role, uint32_t lane, int (*s_sum)[ACF_INT_LAGS + 8])
{
  if (role == 0u) { acf_int_range<D, 0, 5>(planes, rs, nt, lane, s_sum); }
  else if (role == 1u) { acf_int_range<D, 5, 5>(planes, rs, nt, lane, s_sum); }
  else if (role == 2u) { acf_int_range<D, 10, 4>(planes, rs, nt, lane, s_sum); }
  else { acf_int_range<D, 14, 4>(planes, rs, nt, lane, s_sum); }
}

// sum_w 2^(8w) s_w, rounded to double once (round to nearest even; exact below 2^53)
__device__ __forceinline__ double acf_int_combine(const int (*s_sum)[ACF_INT_LAGS + 8], uint32_t k, uint32_t nw)
{
  // weights 0 .. 3 and 4 .. 8 in int64 each (|s_w| < 2^31; s_4 .. s_8 2^(8(w-4)) add up to less than 2^45)
  long long slo = 0, shi = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; w++) { if (w < nw) { slo += (long long)s_sum[w][k] * (1ll << (8u * w)); } }
#pragma unroll
  for (uint32_t w = 4; w < 9; w++) { if (w < nw) { shi += (long long)s_sum[w][k] * (1ll << (8u * (w - 4u))); } }
  if (shi > -(1ll << 29) && shi < (1ll << 29)) { return (double)(slo + shi * (1ll << 32)); }       // fits int64: one conversion
  const __int128 t = (__int128)shi * ((__int128)1 << 32) + (__int128)slo;
  const bool neg = t < 0;
  const unsigned __int128 mag = neg ? (unsigned __int128)(-t) : (unsigned __int128)t;
  const unsigned long long hi = (unsigned long long)(mag >> 64), lo = (unsigned long long)mag;
  double d;
  if (hi == 0ull) { d = (double)lo; }
  else {
    const uint32_t sh = 64u - (uint32_t)__clzll((long long)hi);                        // 1 .. 64 (here at most 32)
    unsigned long long top = (unsigned long long)(mag >> sh);
    if ((lo << (64u - sh)) != 0ull) { top |= 1ull; }                                     // sticky bit: 64 kept bits > 53 + 1
    d = ldexp((double)top, (int)sh);
  }
  return neg ? -d : d;
}

template <bool RAW>
__global__ __launch_bounds__(ACF_INT_THREADS, 3)
void k_ltm_acf_int(const int32_t* __restrict__ res, uint64_t stride, const sla_hip_acf_job* __restrict__ jobs,
                   uint32_t njobs, uint32_t log2F, double* __restrict__ out, double* __restrict__ eps_out,
                   double eps_rel, unsigned long long* span)
{
  extern __shared__ double2 lds2[];
  span_begin(span);
  __shared__ double s_r[ACF_FAST_LAGS + 4];
  __shared__ int s_sum[9][ACF_INT_LAGS + 8];
  __shared__ unsigned long long s_mask[4][ACF_PICK_LAGS / 64];
  __shared__ uint32_t s_nd;
  unsigned char* planes = (unsigned char*)lds2;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t cap = 1u << (log2F - 1u);
  const double scl = ldexp(1.0, (int)log2F - 1 - 62);                    // 2^-62 F/2
  for (uint32_t job = blockIdx.x; job < njobs; job += gridDim.x) {
    const sla_hip_acf_job jb = jobs[job];
    const int32_t* src = res + (uint64_t)jb.channel * stride + jb.blk_off;
    const bool size_ok = (jb.blk_len <= cap);                             // (a block beyond the capacity the LDS was sized for: never certified)
    const uint32_t n = size_ok ? jb.blk_len : 0u;
    const uint32_t nt = (n + 1023u) >> 10;
    const uint32_t rs = ACF_INT_ROW(nt);
    for (uint32_t t = tid; t < 9u * (ACF_INT_LAGS + 8u); t += ACF_INT_THREADS) { (&s_sum[0][0])[t] = 0; }
    if (tid == 0) { s_nd = 1u; }
    __syncthreads();
    // digit planes: thread (i, q) packs kappa = 4q .. 4q + 3 of row i into one dword per plane; zeros from n on.  Sixteen
    // quads of samples are fetched before the first is split (the loads of a job are one round trip, not one per quad).
    // The digits come four at a time: x1 = (x + 128) >> 8 is the remainder behind digit 0, and so on, hence
    // digit a = byte a of y = x + 0x80808080, less 128 -- the byte XOR 0x80 read as int8 -- and digit 4 = the carry out of
    // that sum, 1 from x = 2139062144 on.  D digits suffice when every higher one is zero: the table of DESIGN section 2c.
    const uint32_t nq = 16u * (rs >> 2), nlive = 16u * ((n + 63u) >> 6);
    uint32_t zor = 0;                                                     // OR of the samples' four low digits
    int top = 0;
    for (uint32_t base = tid; base < nlive; base += 4u * ACF_INT_THREADS) {
      int v[4][4];
#pragma unroll
      for (uint32_t it = 0; it < 4; it++) {
        const uint32_t idx = base + it * ACF_INT_THREADS, i = idx & 15u, q = idx >> 4;
        const int32_t* p = src + (64u * q + i);
        if (64u * q + 64u <= n) {
#pragma unroll
          for (uint32_t j = 0; j < 4; j++) { v[it][j] = p[16u * j]; }
        } else {
#pragma unroll
          for (uint32_t j = 0; j < 4; j++) { v[it][j] = (64u * q + 16u * j + i < n) ? p[16u * j] : 0; }
        }
      }
#pragma unroll
      for (uint32_t it = 0; it < 4; it++) {
        const uint32_t idx = base + it * ACF_INT_THREADS, i = idx & 15u, q = idx >> 4;
        if (idx < nlive) {
          uint32_t z[4];
#pragma unroll
          for (uint32_t j = 0; j < 4; j++) { z[j] = ((uint32_t)v[it][j] + 0x80808080u) ^ 0x80808080u; }
          zor |= z[0] | z[1] | z[2] | z[3];
          const int mx = max(max(v[it][0], v[it][1]), max(v[it][2], v[it][3]));
          top = max(top, mx);
          // 4 x 4 byte transpose: byte j of plane d's dword = digit d of sample j
          const uint32_t lo01 = (z[0] & 0x00FF00FFu) | ((z[1] & 0x00FF00FFu) << 8), hi01 = ((z[0] >> 8) & 0x00FF00FFu) | (z[1] & 0xFF00FF00u);
          const uint32_t lo23 = (z[2] & 0x00FF00FFu) | ((z[3] & 0x00FF00FFu) << 8), hi23 = ((z[2] >> 8) & 0x00FF00FFu) | (z[3] & 0xFF00FF00u);
          uint32_t pk[5];
          pk[0] = (lo01 & 0xFFFFu) | (lo23 << 16); pk[2] = (lo01 >> 16) | (lo23 & 0xFFFF0000u);
          pk[1] = (hi01 & 0xFFFFu) | (hi23 << 16); pk[3] = (hi01 >> 16) | (hi23 & 0xFFFF0000u);
          pk[4] = 0u;
          if (__ballot(mx >= 2139062144) != 0ull) {                       // (wave-uniform, rare: a fifth digit)
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) { pk[4] |= (v[it][j] >= 2139062144 ? 1u : 0u) << (8u * j); }
          }
          uint32_t* dst = (uint32_t*)(planes + i * rs) + q;
#pragma unroll
          for (uint32_t d = 0; d < 5; d++) { dst[d * 4u * rs] = pk[d]; }                    // (16 rs bytes per plane)
        }
      }
    }
    for (uint32_t idx = nlive + tid; idx < nq; idx += ACF_INT_THREADS) {                  // zeros behind the block
      uint32_t* dst = (uint32_t*)(planes + (idx & 15u) * rs) + (idx >> 4);
#pragma unroll
      for (uint32_t d = 0; d < 5; d++) { dst[d * 4u * rs] = 0u; }
    }
    {
      const uint32_t need = (__ballot(top >= 2139062144) != 0ull) ? 5u : (__ballot((zor >> 24) != 0u) != 0ull) ? 4u
                          : (__ballot((zor >> 16) != 0u) != 0ull) ? 3u : (__ballot((zor >> 8) != 0u) != 0ull) ? 2u : 1u;
      if (lane == 0 && need > 1u) { atomicMax(&s_nd, need); }
    }
    __syncthreads();
    const uint32_t nd = s_nd;
    const uint32_t role = (wave + job) & 3u;
    if (nt != 0u) {
      if (nd == 1u) { acf_int_products<1>(planes, rs, nt, role, lane, s_sum); }
      else if (nd == 2u) { acf_int_products<2>(planes, rs, nt, role, lane, s_sum); }
      else if (nd == 3u) { acf_int_products<3>(planes, rs, nt, role, lane, s_sum); }
      else if (nd == 4u) { acf_int_products<4>(planes, rs, nt, role, lane, s_sum); }
      else { acf_int_products<5>(planes, rs, nt, role, lane, s_sum); }
    }
    __syncthreads();
    for (uint32_t t = tid; t < ACF_FAST_LAGS + 4; t += ACF_INT_THREADS) {
      s_r[t] = (t < ACF_INT_LAGS) ? scl * acf_int_combine(s_sum, t, 2u * nd - 1u) : 0.0;
    }
    __syncthreads();
    if constexpr (RAW) {
      for (uint32_t t = tid; t < ACF_INT_LAGS; t += ACF_INT_THREADS) { out[(uint64_t)job * ACF_INT_LAGS + t] = s_r[t]; }
    } else {
      acf_emit_cert<ACF_INT_THREADS>(s_r, job, out, eps_out, eps_rel, size_ok, s_mask);
      if (!size_ok && tid == 0) { eps_out[job] = -1.0; }                 // (its sums were not formed: not the silent case)
    }
    __syncthreads();
  }
  span_end(span);
}

// ---------------------------------------------------------------------------------------------
// k_ltm_solve: pitch and taps of every (block, channel) from k_ltm_acf's compact record, written straight into the
// job table k_tail reads -- the long-term stage never leaves the device (src/SLAPredictor.c:855-863, 913-979;
// the 5x5 LU solve with two refinement passes is src/SLAUtility.c:487-674; the tap quantiser src/SLAEncoder.c:629-640).
// One lane per job.  The reference accumulates the refinement residual in x87 long double: ext80 below is that
// arithmetic in integers (64-bit significand, round to nearest even), so the result is the reference's bit for bit.
// ---------------------------------------------------------------------------------------------
struct ext80 { uint64_t m; int32_t e; uint32_t neg; };      // (-1)^neg * m * 2^e, bit 63 of m set (m == 0: zero)

__device__ __forceinline__ ext80 ext_from_double(double d)
{
  ext80 r; r.m = 0; r.e = 0; r.neg = 0;
  const uint64_t bits = (uint64_t)__double_as_longlong(d);
  const uint32_t be = (uint32_t)(bits >> 52) & 0x7FFu;
  uint64_t frac = bits & 0xFFFFFFFFFFFFFull;
  r.neg = (uint32_t)(bits >> 63);
  if (be == 0) {
    if (frac == 0) { return r; }
    const int lz = __clzll((long long)frac);
    r.m = frac << lz; r.e = -1074 - lz;
    return r;
  }
  r.m = (frac | (1ull << 52)) << 11;
  r.e = (int32_t)be - 1075 - 11;
  return r;
}

// a + b rounded to a 64-bit significand (FADD with the x87 precision control at its default, extended)
__device__ __forceinline__ ext80 ext_add(ext80 a, ext80 b)
{
  if (b.m == 0) { return a; }
  if (a.m == 0) { return b; }
  if (b.e > a.e || (b.e == a.e && b.m > a.m)) { const ext80 t = a; a = b; b = t; }      // |a| >= |b|
  const uint32_t shift = (uint32_t)(a.e - b.e);
  const unsigned __int128 A = (unsigned __int128)a.m << 63;                                 // value = A * 2^(a.e - 63)
  unsigned __int128 B = 0;
  bool sticky = false;
  if (shift < 128) {
    const unsigned __int128 full = (unsigned __int128)b.m << 63;
    B = full >> shift;
    sticky = ((B << shift) != full);
  } else {
    sticky = true;
  }
  unsigned __int128 S;
  if (a.neg == b.neg) { S = A + B; } else { S = A - B - (sticky ? 1u : 0u); }            // true value = S + (0, 1) when sticky
  ext80 r; r.neg = a.neg; r.m = 0; r.e = 0;
  if (S == 0 && !sticky) { r.neg = 0; return r; }
  const uint64_t hi0 = (uint64_t)(S >> 64), lo0 = (uint64_t)S;
  const int lz = hi0 ? __clzll((long long)hi0) : 64 + __clzll((long long)lo0);
  S <<= lz;
  uint64_t m = (uint64_t)(S >> 64);
  const uint64_t low = (uint64_t)S;
  int32_t ex = a.e - 63 - lz + 64;
  const uint64_t half = 1ull << 63;
  const bool up = (low > half) || (low == half && (sticky || (m & 1ull)));
  if (up) { m += 1; if (m == 0) { m = half; ex += 1; } }
  r.m = m; r.e = ex;
  return r;
}

// (double)x: round the 64-bit significand to 53 bits, nearest even
__device__ __forceinline__ double ext_to_double(ext80 x)
{
  if (x.m == 0) { return x.neg ? -0.0 : 0.0; }
  uint64_t m53 = x.m >> 11;
  const uint64_t rem = x.m & 0x7FFull;
  if (rem > 0x400ull || (rem == 0x400ull && (m53 & 1ull))) { m53 += 1; }
  const double v = ldexp((double)m53, x.e + 11);           // m53 <= 2^53: exact
  return x.neg ? -v : v;
}

#define LTM_NT 5

// The solve with the tap count as a template parameter: every loop is unrolled and every index static, so the 5 x 5 work
// arrays live in registers (with run-time dimensions and the pivot's row index they sat in scratch memory: 66 us per
// C5 launch for 45 000 tiny solves).  The pivot row and the permuted right-hand side are picked by compare-and-select
// over the (at most five) candidates; the arithmetic and its order are the host's (sla_ltm.c), operation for operation.
template <int D>
__device__ __forceinline__ int ltm_lu_factor_s(double (&A)[D][D], uint32_t (&perm)[D], double (&scale)[D], double* clear = nullptr)
{
  // clear != nullptr (k_ltm_solve_cert): *clear = the smallest (best - runner-up) / best over the pivot searches, i.e. by how
  // much every choice of a pivot row was decided
#pragma unroll
  for (int row = 0; row < D; row++) {
    double big = 0.0;
#pragma unroll
    for (int col = 0; col < D; col++) { if (fabs(A[row][col]) > big) { big = fabs(A[row][col]); } }
    if (fabs(big) <= (double)FLT_EPSILON) { return -1; }
    scale[row] = 1.0 / big;
  }
  int bad = 0;
#pragma unroll
  for (int col = 0; col < D; col++) {
#pragma unroll
    for (int row = 0; row < col; row++) {
      double sum = A[row][col];
#pragma unroll
      for (int k = 0; k < row; k++) { sum -= A[row][k] * A[k][col]; }
      A[row][col] = sum;
    }
    double big = 0.0, second = 0.0;
    uint32_t imax = (uint32_t)col;
#pragma unroll
    for (int row = col; row < D; row++) {
      double sum = A[row][col];
#pragma unroll
      for (int k = 0; k < col; k++) { sum -= A[row][k] * A[k][col]; }
      A[row][col] = sum;
      const double t = scale[row] * fabs(sum);
      if (t >= big) { second = big; big = t; imax = (uint32_t)row; } else if (t > second) { second = t; }
    }
    if (clear != nullptr && col != D - 1) { *clear = fmin(*clear, (big > 0.0) ? (big - second) / big : 0.0); }
#pragma unroll
    for (int r = col + 1; r < D; r++) {
      if (imax == (uint32_t)r) {
#pragma unroll
        for (int k = 0; k < D; k++) { const double t = A[r][k]; A[r][k] = A[col][k]; A[col][k] = t; }
        scale[r] = scale[col];
      }
    }
    perm[col] = imax;
    if (fabs(A[col][col]) <= (double)FLT_EPSILON) { bad = 1; }
    if (!bad && col != D - 1) {
      const double inv = 1.0 / A[col][col];
#pragma unroll
      for (int row = col + 1; row < D; row++) { A[row][col] *= inv; }
    }
  }
  return bad ? -1 : 0;
}

template <int D>
__device__ __forceinline__ void ltm_lu_substitute_s(const double (&A)[D][D], double (&b)[D], const uint32_t (&perm)[D])
{
  uint32_t first_nz = 0;
#pragma unroll
  for (int row = 0; row < D; row++) {
    const uint32_t pv = perm[row];
    double sum = b[row];
#pragma unroll
    for (int r = 0; r < D; r++) { if (pv == (uint32_t)r) { sum = b[r]; } }
    const double mine = b[row];
#pragma unroll
    for (int r = 0; r < D; r++) { if (pv == (uint32_t)r) { b[r] = mine; } }
    if (first_nz != 0) {
#pragma unroll
      for (int col = 0; col < row; col++) { if ((uint32_t)col >= first_nz) { sum -= A[row][col] * b[col]; } }
    } else if (sum != 0.0) {
      first_nz = (uint32_t)row;
    }
    b[row] = sum;
  }
#pragma unroll
  for (int row = D - 1; row >= 0; row--) {
    double sum = b[row];
#pragma unroll
    for (int col = row + 1; col < D; col++) { sum -= A[row][col] * b[col]; }
    b[row] = sum / A[row][row];
  }
}

template <int D>
__device__ __forceinline__ sla_hip_tail_job ltm_solve_one(const double* __restrict__ rec, const sla_hip_lpc_group g)
{
  double low[5], mid[5];
#pragma unroll
  for (int i = 0; i < 5; i++) { low[i] = rec[2 + i]; mid[i] = rec[7 + i]; }
  const uint32_t chosen = (uint32_t)rec[1];
  double vec[LTM_NT] = {0.0, 0.0, 0.0, 0.0, 0.0};
  uint32_t pitch = 0;
  int ret = 0;
  if (rec[0] == 0.0) {
    ret = 0;                                               // silent residual: no pitch, zero taps
  } else if (rec[0] != 1.0 || chosen < (uint32_t)(D / 2 + 1)) {
    ret = 4;
  } else {
    double R[D][D], A[D][D], x[D], err[D], scale[D], b[D];
    uint32_t perm[D];
#pragma unroll
    for (int r = 0; r < D; r++) {
#pragma unroll
      for (int c = 0; c < D; c++) { R[r][c] = low[(r >= c) ? (r - c) : (c - r)]; A[r][c] = R[r][c]; }
    }
#pragma unroll
    for (int r = 0; r < D; r++) { b[r] = mid[2 + r - D / 2]; x[r] = b[r]; }
    if (ltm_lu_factor_s<D>(A, perm, scale) != 0) {
      ret = 4;
    } else {
      ltm_lu_substitute_s<D>(A, x, perm);
#pragma unroll 1
      for (int it = 0; it < 2; it++) {
#pragma unroll
        for (int r = 0; r < D; r++) {
          ext80 acc = ext_from_double(-b[r]);
#pragma unroll
          for (int c = 0; c < D; c++) { acc = ext_add(acc, ext_from_double(R[r][c] * x[c])); }
          err[r] = ext_to_double(acc);
        }
        ltm_lu_substitute_s<D>(A, err, perm);
#pragma unroll
        for (int r = 0; r < D; r++) { x[r] -= err[r]; }
      }
      double mag = 0.0;
#pragma unroll
      for (int r = 0; r < D; r++) { mag += fabs(x[r]); }
      if (mag >= 1.0) {
#pragma unroll
        for (int r = 0; r < D; r++) { x[r] = 0.0; }
        x[D / 2] = mid[2] / low[0];
      }
      pitch = chosen;
#pragma unroll
      for (int r = 0; r < D; r++) { vec[r] = x[r]; }
    }
  }
  if (ret != 0 || pitch >= 256u) { pitch = 0; }            // src/SLAEncoder.c:629-632
  sla_hip_tail_job out;
  out.blk_off = g.pcm_off; out.blk_len = g.num_samples; out.channel = g.channel; out.pitch = pitch;
#pragma unroll
  for (int t = 0; t < LTM_NT; t++) {
    // Round(coef * 2^15) << 16 with the x86 conversion (out of range / NaN -> INT32_MIN)   src/SLAEncoder.c:635-640
    const double v = ((t < D) ? vec[t] : 0.0) * 32768.0;
    const double rv = (v >= 0.0) ? floor(v + 0.5) : -floor(-v + 0.5);
    const int32_t q = (!(rv > -2147483649.0 && rv < 2147483648.0)) ? INT32_MIN : (int32_t)rv;
    out.ltm_coef[t] = (int32_t)((uint32_t)q << 16);
  }
  out.pad_[0] = out.pad_[1] = 0;
  return out;
}

template <int D>
__global__ __launch_bounds__(64)
void k_ltm_solve(const double* __restrict__ acf, const sla_hip_lpc_group* __restrict__ groups, uint32_t num_jobs,
                 sla_hip_tail_job* __restrict__ jobs)
{
  const uint32_t j = blockIdx.x * 64 + threadIdx.x;
  if (j >= num_jobs) { return; }
  jobs[j] = ltm_solve_one<D>(acf + (uint64_t)j * SLA_HIP_ACF_RECORD, groups[j]);
}

// the exact solve over the list k_ltm_solve_cert left (records rewritten by k_ltm_acf2_list): a fixed grid strides over it.
// counters: [0] list entries, [1] uncertified jobs, [2] audited jobs whose certified pitch and taps equal the exact ones, [3] unequal
template <int D>
__global__ __launch_bounds__(64)
void k_ltm_solve_list(const double* __restrict__ acf, const sla_hip_lpc_group* __restrict__ groups,
                      const uint32_t* __restrict__ list, uint32_t* __restrict__ counters, sla_hip_tail_job* __restrict__ jobs)
{
  const uint32_t n_list = counters[0];
  for (uint32_t i = blockIdx.x * 64 + threadIdx.x; i < n_list; i += gridDim.x * 64) {
    const uint32_t entry = list[i], j = entry & ~LTM_LIST_AUDIT;
    const sla_hip_tail_job out = ltm_solve_one<D>(acf + (uint64_t)j * SLA_HIP_ACF_RECORD, groups[j]);
    if (entry & LTM_LIST_AUDIT) {
      const sla_hip_tail_job was = jobs[j];
      bool same = (was.pitch == out.pitch);
#pragma unroll
      for (int t = 0; t < LTM_NT; t++) { same = same && (was.ltm_coef[t] == out.ltm_coef[t]); }
      atomicAdd(&counters[same ? 2 : 3], 1u);
    }
    jobs[j] = out;
  }
}

// ---------------------------------------------------------------------------------------------
// k_ltm_solve_cert: pitch and taps from k_ltm_acf_fast's record when they provably equal what k_ltm_solve makes of the
// reference's record; otherwise the job goes onto the fallback list.  With |r' - r_ref| <= eps in every entry
// (dR: Toeplitz of entries <= eps, ||dR||_inf <= D eps; db: entries <= eps) the first-order perturbation of R x = b is
//     ||dx||_inf <= ||R^-1||_inf (eps + eps sum|x|)
// doubled here for the second-order terms (||R^-1|| D eps < 1e-3 is required) and widened by 128 u cond (1 + sum|x|) for
// the rounding of both solvers (LU with partial pivoting, refinement: a few u cond each).  ||R^-1||_inf comes from D unit
// solves with the factorisation at hand.  Certified means: the factorisation's failure tests (row maximum and pivots
// against FLT_EPSILON) are decided with margin, cond_inf <= 64, sum|x| is off 1 by more than D dx, and every tap * 2^15 is
// further from a rounding boundary of the quantiser than dx * 2^15 plus a few ulp of the value.
// ---------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(64)
void k_ltm_solve_cert(const double* __restrict__ acf, const double* __restrict__ eps_in, const sla_hip_lpc_group* __restrict__ groups,
                      uint32_t num_jobs, sla_hip_tail_job* __restrict__ jobs, uint32_t* __restrict__ list,
                      uint32_t* __restrict__ counters, uint32_t audit_every)
{
  const uint32_t j = blockIdx.x * 64 + threadIdx.x;
  if (j >= num_jobs) { return; }
  const double* rec = acf + (uint64_t)j * SLA_HIP_ACF_RECORD;
  const double u = 1.1102230246251565e-16;
  const double eps = eps_in[j];
  double low[5], mid[5];
#pragma unroll
  for (int i = 0; i < 5; i++) { low[i] = rec[2 + i]; mid[i] = rec[7 + i]; }
  const uint32_t chosen = (uint32_t)rec[1];
  bool ok = (eps >= 0.0) && (eps < 1.0e300);             // the pick is certified (acf_emit_cert), nothing non-finite
  double vec[LTM_NT] = {0.0, 0.0, 0.0, 0.0, 0.0};
  double delta = 0.0;
  uint32_t pitch = 0;
  int ret = 0;
  if (!ok || rec[0] == 0.0) {
    ret = 0;
  } else if (rec[0] != 1.0 || chosen < (uint32_t)(D / 2 + 1)) {
    ret = 4;
  } else {
    double R[D][D], A[D][D], x[D], err[D], scale[D], b[D];
    uint32_t perm[D];
    double rowmax = 0.0, normR = 0.0, clear = 1.0;
#pragma unroll
    for (int r = 0; r < D; r++) {
      double rs = 0.0;
#pragma unroll
      for (int c = 0; c < D; c++) { R[r][c] = low[(r >= c) ? (r - c) : (c - r)]; A[r][c] = R[r][c]; rs += fabs(R[r][c]); }
      normR = fmax(normR, rs);
    }
#pragma unroll
    for (int c = 0; c < D; c++) { rowmax = fmax(rowmax, fabs(low[c])); ok = ok && (fabs(low[c]) < 1.0e300) && (fabs(mid[c]) < 1.0e300); }
#pragma unroll
    for (int r = 0; r < D; r++) { b[r] = mid[2 + r - D / 2]; x[r] = b[r]; }
    if (rowmax + eps <= (double)FLT_EPSILON * (1.0 - 1.0e-9)) {
      ret = 4;                                             // row 0 (it holds r[0 .. D-1]) fails the reference's row test for certain
    } else if (!(low[0] - eps > (double)FLT_EPSILON * (1.0 + 1.0e-9))) {
      ok = false;                                          // (r[0] sits in every row: above the threshold, every row passes)
    } else if (ltm_lu_factor_s<D>(A, perm, scale, &clear) != 0) {
      ok = false;                                          // a pivot at FLT_EPSILON here: not decided for the reference
    } else {
      double pivmin = fabs(A[0][0]);
#pragma unroll
      for (int r = 1; r < D; r++) { pivmin = fmin(pivmin, fabs(A[r][r])); }
      ltm_lu_substitute_s<D>(A, x, perm);
#pragma unroll
      for (int r = 0; r < D; r++) {
        double acc = -b[r];
#pragma unroll
        for (int c = 0; c < D; c++) { acc = fma(R[r][c], x[c], acc); }
        err[r] = acc;
      }
      ltm_lu_substitute_s<D>(A, err, perm);
#pragma unroll
      for (int r = 0; r < D; r++) { x[r] -= err[r]; }
      double rows[D];
#pragma unroll
      for (int r = 0; r < D; r++) { rows[r] = 0.0; }
#pragma unroll
      for (int c = 0; c < D; c++) {
        double col[D];
#pragma unroll
        for (int r = 0; r < D; r++) { col[r] = (r == c) ? 1.0 : 0.0; }
        ltm_lu_substitute_s<D>(A, col, perm);
#pragma unroll
        for (int r = 0; r < D; r++) { rows[r] += fabs(col[r]); }
      }
      double ninv = 0.0, mag = 0.0;
#pragma unroll
      for (int r = 0; r < D; r++) { ninv = fmax(ninv, rows[r]); mag += fabs(x[r]); }
      const double kappa = ninv * normR;
      delta = 2.0 * ninv * eps * (1.0 + mag) + 128.0 * u * kappa * (1.0 + mag);
      // pivot = ratio of two leading minors of the row-permuted matrix; d det / det <= D ||R^-1|| D eps each: |d pivot| <=
      // 2 D^2 cond eps, doubled.  That compares like with like only if the reference exchanges the same rows: every pivot
      // search (scaled column entries, perturbed by at most ~2 D^2 cond^2 eps / r[0] ~ 1.5e-7 of the winner at cond = 64)
      // must have been decided by 1e-5 of the winner, or the job is not certified
      ok = ok && (clear > 1.0e-5) && (kappa <= 64.0) && (ninv * (double)D * eps < 1.0e-3)
              && (pivmin * (1.0 - 1.0e-9) - 4.0 * (double)(D * D) * kappa * eps > (double)FLT_EPSILON);
      if (mag - (double)D * delta - 1.0e-14 >= 1.0) {
#pragma unroll
        for (int r = 0; r < D; r++) { x[r] = 0.0; }
        x[D / 2] = mid[2] / low[0];
        delta = 2.0 * eps * (1.0 + fabs(x[D / 2])) / low[0] + 8.0 * u;       // the single tap r[p] / r[0]; the zero taps are exact
      } else if (!(mag + (double)D * delta + 1.0e-14 < 1.0)) {
        ok = false;
      }
      pitch = chosen;
#pragma unroll
      for (int r = 0; r < D; r++) { vec[r] = x[r]; }
    }
  }
  if (ret != 0 || pitch >= 256u) { pitch = 0; }
  const sla_hip_lpc_group g = groups[j];
  sla_hip_tail_job out;
  out.blk_off = g.pcm_off; out.blk_len = g.num_samples; out.channel = g.channel; out.pitch = pitch;
#pragma unroll
  for (int t = 0; t < LTM_NT; t++) {
    const double v = ((t < D) ? vec[t] : 0.0) * 32768.0;
    const double av = fabs(v);
    // floor(|v| + 0.5) steps where |v| + 0.5 is an integer, and the sum itself rounds: stay dx 2^15 and a few ulp away
    const double fr = (av + 0.5) - floor(av + 0.5);
    const double dist = fmin(fr, 1.0 - fr);
    if (t < D && !(dist > delta * 32768.0 + 16.0 * u * (av + 1.0) && av < 2.0e9)) { ok = false; }      // (a zero tap: dist = 0.5)
    const double rv = (v >= 0.0) ? floor(v + 0.5) : -floor(-v + 0.5);
    const int32_t q = (!(rv > -2147483649.0 && rv < 2147483648.0)) ? INT32_MIN : (int32_t)rv;
    out.ltm_coef[t] = (int32_t)((uint32_t)q << 16);
  }
  out.pad_[0] = out.pad_[1] = 0;
  jobs[j] = out;
  if (!ok) {
    list[atomicAdd(&counters[0], 1u)] = j;
    atomicAdd(&counters[1], 1u);
  } else if (audit_every != 0 && (j % audit_every) == 0) {
    list[atomicAdd(&counters[0], 1u)] = j | LTM_LIST_AUDIT;
  }
}
