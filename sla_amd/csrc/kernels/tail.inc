// kernels/tail.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): k_tailk: long-term filter, sign-log LMS cascade, folded sum, Rice initial parameter
// ---------------------------------------------------------------------------------------------
// Tail stage: long-term filter -> sign-log LMS -> folded sum (src/SLAPredictor.c:1031-1119, 1202-1331; src/SLACoder.c:361-385).
// The LMS is serial in time (every sample updates all 2 * ORDER coefficients from the error it just produced), so the
// parallelism inside one (block, channel) job exists only ACROSS THE TAPS: a few lanes own one job, each K taps of the input
// history and K of the prediction history; per sample the lanes' products meet in a DPP sum (wrapping int adds are
// associative, so the tree equals the reference's serial sum), the error and the step are computed redundantly by every
// lane of the job, and the histories move on by one DPP shift.  (Rounds 1 - 3 kept three earlier layouts -- 2 * ORDER
// lanes, ORDER lanes, ONE lane per job -- behind an option; k_tailk beat all of them at every job count, DESIGN section 4.)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t sgn(int32_t v)          // clamp to [-1, 1] = sign, one v_med3_i32
{
  int32_t r;
  asm("v_med3_i32 %0, %1, -1, 1" : "=v"(r) : "v"(v));
  return r;
}

__device__ __forceinline__ int32_t mad24(int32_t a, int32_t b, int32_t c)      // a, b within 24 bits; c + a*b wraps like int32
{
  int32_t r;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// all lanes of the permutation are valid, so old = 0 / bound_ctrl lets the add absorb the DPP read
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t x)
{
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}

// ---------------------------------------------------------------------------------------------
// k_tailk: the same stage with K taps of each history per lane (2 K coefficients), ORDER / K lanes per job -- for files
// with so many (block, channel) jobs that what counts is instructions per job and sample, not the length of one job's
// chain.  Measured (tests/tools/ubench_int.hip, one wave on a SIMD): an instruction that needs the result of a recent one
// issues 3.3 ns after it, an independent one 1.7 - 1.9 ns, a dependent DPP step with its wait states 6.8 ns -- and a
// 32-bit v_mul_lo costs what an add costs.  So a lone wave pays for every instruction of the per-sample loop (k_tail:
// 22 + 4 wait states = 105 ns per sample, which is the whole C2 launch), two or more waves per SIMD fill each other's
// stalls, and then the work per sample is what is left to cut: everything that is computed once per job and sample
// (the sum's last steps, error, logarithm, step, history shift: ~20 instructions) is shared by 64 / (ORDER / K) jobs
// of a wave instead of 4 (k_tail) or 8 (k_tail2), against 4 K instructions more for the lane's own products and
// updates.  ORDER 8: k_tail2 ~30 instructions per sample for 8 jobs, K = 2 ~37 for 16, K = 4 ~53 for 32.
//
// Layout.  The jobs of a DPP row (16 lanes) are interleaved: lane r of the row is lane r / JPR of job r % JPR (JPR = jobs
// per row), so a shift of the history to the job's next lane is row_shr:JPR for all jobs at once -- the first lane of
// every job has no source inside the row and keeps `old`, which is the new input / prediction: no select -- and the
// job's sum is log2(lanes) row rotations.  A lane keeps its K history values in place: at step u of the unrolled block
// the tap of age a sits in slot (a - u) mod K, the slot of the value that leaves for the next lane takes the one that
// arrives, and the signs are kept beside the values (one sign per arriving value instead of one per tap and sample).
// ---------------------------------------------------------------------------------------------
template <int LPJ>
__device__ __forceinline__ uint32_t job_sum(uint32_t x)          // over the lanes r, r + JPR, r + 2 JPR, .. of a row
{
  x += dpp_u32<0x128>(x);                                  // row_ror:8
  if (LPJ >= 4) { x += dpp_u32<0x124>(x); }                // row_ror:4
  if (LPJ >= 8) { x += dpp_u32<0x122>(x); }                // row_ror:2
  if (LPJ >= 16) { x += dpp_u32<0x121>(x); }               // row_ror:1
  return x;
}

// Samples cross global memory 32 at a time per job (TAILK_BLK): the job's lanes each move a run of 32 / lanes consecutive
// samples as 16-byte accesses, so a job touches each of its cache lines once.  (Per-sample accesses of 2 - 4 lanes per
// job made a wave's load touch 16 - 32 lines for 8 bytes each: the first version of this kernel was bound by those
// line fetches and lost to k_tail2 -- C3 60 min 4.6 against 3.6 ms with four taps per lane.)
#define TAILK_BLK 32
typedef int32_t tk_i32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef int32_t tk_i32x2 __attribute__((ext_vector_type(2), aligned(4)));

template <int N>
__device__ __forceinline__ void tk_load_run(const int32_t* __restrict__ p, int32_t (&v)[N])      // N consecutive words, 4-byte aligned
{
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int q = 0; q < N / 4; q++) {
      const tk_i32x4 x = *reinterpret_cast<const tk_i32x4*>(p + 4 * q);
      v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < N / 2; q++) {
      const tk_i32x2 x = *reinterpret_cast<const tk_i32x2*>(p + 2 * q);
      v[2 * q] = x.x; v[2 * q + 1] = x.y;
    }
  }
}
template <int N>
__device__ __forceinline__ void tk_store_run(int32_t* __restrict__ p, const int32_t (&v)[N])
{
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int q = 0; q < N / 4; q++) {
      tk_i32x4 x; x.x = v[4 * q]; x.y = v[4 * q + 1]; x.z = v[4 * q + 2]; x.w = v[4 * q + 3];
      *reinterpret_cast<tk_i32x4*>(p + 4 * q) = x;
    }
  } else {
#pragma unroll
    for (int q = 0; q < N / 2; q++) {
      tk_i32x2 x; x.x = v[2 * q]; x.y = v[2 * q + 1];
      *reinterpret_cast<tk_i32x2*>(p + 2 * q) = x;
    }
  }
}

// IIR24: every value in the prediction history is a prediction p = (int32)sum >> 10, i.e. |p| <= 2^21, and the coefficients are
// sums of at most blk_len steps of size <= 16 (src/SLAPredictor.c:123-144 with SLALMS_DELTA_WEIGHT_SHIFT 4), |c| <= 2^22 for
// blocks of at most 2^18 samples: their products are v_mad_i32_i24's (the low 32 bits of the 48-bit product are the wrapped
// product the reference computes) -- one instruction at ~1.9 add slots instead of v_mul_lo_u32 + v_add_u32 at ~3.3
// (tests/tools/ubench_lattice.hip).  Not while the history still holds the block's first ORDER samples (the priming copies
// them into BOTH histories, src/SLAPredictor.c:1233-1255, and a sample may be wider than 24 bits).
template <int ORDER, int K, bool FIRST, bool IIR24 = false>
__device__ __forceinline__ void tailk_block(const int32_t (&vm)[TAILK_BLK * K / ORDER], int32_t (&em)[TAILK_BLK * K / ORDER],
                                            const int (&addr)[ORDER / K], uint32_t L,
                                            int32_t (&ca)[K], int32_t (&cb)[K], int32_t (&ha)[K], int32_t (&hb)[K],
                                            int32_t (&sa)[K], int32_t (&sb)[K])
{
  constexpr int LPJ = ORDER / K, JPR = 16 / LPJ, SPL = TAILK_BLK / LPJ;
  constexpr int SHR = 0x110 + JPR;                         // row_shr:JPR
#pragma unroll
  for (int u0 = 0; u0 < TAILK_BLK; u0 += 8) {
    // sample u of the block was fetched by the job's lane u / SPL as its element u % SPL; eight at a time, all requested
    // before the first is used, so that no step of the chain waits for the LDS crossbar
    int32_t vs[8];
#pragma unroll
    for (int w = 0; w < 8; w++) { vs[w] = __builtin_amdgcn_ds_bpermute(addr[(u0 + w) / SPL], vm[(u0 + w) % SPL]); }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int w = 0; w < 8; w++) {
      const int u = u0 + w;
      const int32_t v = vs[w];
      int32_t e, ph;
      if (FIRST && u < ORDER) {
        e = v; ph = v;                                     // the first ORDER samples only prime both histories
      } else {
        uint32_t acc = 0;
#pragma unroll
        for (int a = 0; a < K; a++) {
          const int slot = ((a - u) % K + K) % K;
          acc += (uint32_t)ca[a] * (uint32_t)ha[slot];
          if (IIR24) { acc = (uint32_t)mad24(cb[a], hb[slot], (int32_t)acc); }
          else { acc += (uint32_t)cb[a] * (uint32_t)hb[slot]; }
        }
        const uint32_t sum = job_sum<LPJ>(acc) + (1u << 9);
        const int32_t p = (int32_t)sum >> 10;
        e = (int32_t)((uint32_t)v - (uint32_t)p);
        const int32_t ne = (int32_t)((uint32_t)p - (uint32_t)v);
        const uint32_t mag = (uint32_t)max(e, ne);
        // step = ceil(log2(|e| + 1)) >> 1 (step table src/SLAPredictor.c:123-144), times sign(e).  v_ffbh_u32 answers -1 for
        // zero, which would make the step 16 -- times sign(0) = 0: no special case (the portable __clz spelling cost five
        // instructions on this chain, this one three)
        // (round 4: sign(e) * m as the clamp of e to [-m, m] -- |e| >= 2^(bits - 1) >= bits / 2 = m for every e != 0, and e = 0 clamps
        // to 0 -- one v_med3_i32 instead of a sign and a 24-bit multiply, which the compiler had also wrapped in two extra shifts)
        uint32_t lead;
        asm("v_ffbh_u32 %0, %1" : "=v"(lead) : "v"(mag));
        const int32_t m = (int32_t)((32u - lead) >> 1);
        // (tried for K = 1, where the launch is one job's chain: -e as an instruction of its own beside e, and -m as
        // (lead - 31) >> 1 beside m -- two steps off the chain on paper, 0.352 -> 0.358 ms on C2: not kept)
        int32_t g;
        asm("v_med3_i32 %0, %1, %2, %3" : "=v"(g) : "v"(e), "v"(-m), "v"(m));
#pragma unroll
        for (int a = 0; a < K; a++) {
          const int slot = ((a - u) % K + K) % K;
          ca[a] = mad24(g, sa[slot], ca[a]);
          cb[a] = mad24(g, sb[slot], cb[a]);
        }
        ph = p;
      }
      const int put = (K - 1 - (u % K));                   // the slot of the lane's oldest value takes the arriving one
      ha[put] = (int32_t)__builtin_amdgcn_update_dpp(v, ha[put], SHR, 0xF, 0xF, false);
      hb[put] = (int32_t)__builtin_amdgcn_update_dpp(ph, hb[put], SHR, 0xF, 0xF, false);
      sa[put] = sgn(ha[put]);
      sb[put] = sgn(hb[put]);
      em[u % SPL] = (L == (uint32_t)(u / SPL)) ? e : em[u % SPL];
    }
  }
}

// The coder's initial Rice parameter of a job from its folded sum (src/SLACoder.c:371-384): the mean of the folded residual, at
// least 1, as the value that survives the coder's 32-bit 24.8 fixed-point word (src/SLACoder.c:14,19) -- init << 8 wraps at 2^24,
// and a word that comes back as 0 is sent as 1.  A job without samples divides nothing and gets 1.
__device__ __forceinline__ uint32_t rice_init_of(uint64_t fsum, uint32_t blk_len)
{
  if (blk_len == 0) { return 1u; }
  const uint64_t mean = fsum / blk_len;
  const uint32_t init = (uint32_t)(mean > 1 ? mean : 1);
  const uint32_t kept = (uint32_t)((((uint64_t)(uint32_t)(init << 8)) + 128u) >> 8);
  return kept ? kept : 1u;
}

template <int ORDER, int K>
__global__ __launch_bounds__(256)
void k_tailk(const int32_t* __restrict__ res_in, int32_t* __restrict__ res_out, uint64_t stride,
             const sla_hip_tail_job* __restrict__ jobs, uint32_t num_jobs, uint32_t ntaps,
             uint64_t* __restrict__ fold_sum, unsigned long long* span, uint32_t stage_flags, uint32_t* __restrict__ rice_init)
{
  span_begin(span);
  constexpr int LPJ = ORDER / K;               // lanes per job: 2 .. 16
  constexpr int JPR = 16 / LPJ;                // jobs per DPP row
  constexpr int JPW = 4 * JPR;                 // jobs per wave
  constexpr int SPL = TAILK_BLK / LPJ;         // consecutive samples a lane moves per block of 32: 2 .. 16
  static_assert(ORDER % K == 0 && LPJ >= 2 && LPJ <= 16 && (LPJ & (LPJ - 1)) == 0 && TAILK_BLK % ORDER == 0, "lanes per job");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t row = lane >> 4, r = lane & 15u;
  const uint32_t jr = r % JPR, L = r / JPR;
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t j = wave * JPW + row * JPR + jr;
  const bool have = (j < num_jobs);
  const sla_hip_tail_job job = jobs[have ? j : 0];
  const uint32_t n = have ? job.blk_len : 0;
  const int32_t* in = res_in + (uint64_t)job.channel * stride + job.blk_off;
  int32_t* out = res_out + (uint64_t)job.channel * stride + job.blk_off;
  const uint32_t delay = job.pitch + (ntaps >> 1);
  const bool use_ltm = (job.pitch >= 3);
  const bool pass = (n < (uint32_t)ORDER) || (stage_flags & 1u);      // fewer samples than taps, or no LMS stage wanted: everything passes through
  const uint32_t nmax = umax_wave(n);
  const bool iir24_ok = (nmax <= (1u << 18));        // |coefficient| <= 16 * blk_len stays a 24-bit value (see tailk_block)

  // the lane's run of block s0: samples [s0 + L SPL, + SPL), behind the long-term stage   src/SLAPredictor.c:1063-1099
  auto fetch_run = [&](uint32_t s0, int32_t (&v)[SPL]) {
    const uint32_t s = s0 + L * SPL;
    if (s + SPL <= n && (!use_ltm || s >= delay)) {
      tk_load_run<SPL>(in + s, v);
      if (use_ltm) {
        int32_t win[SPL + 4];                              // in[s - delay .. s - delay + SPL + ntaps - 2]
        const int32_t* w = in + (s - delay);
#pragma unroll
        for (int i = 0; i < SPL + 4; i++) { win[i] = ((uint32_t)i < SPL + ntaps - 1) ? w[i] : 0; }
#pragma unroll
        for (int i = 0; i < SPL; i++) {
          int64_t acc = (int64_t)1 << 30;
#pragma unroll
          for (int k = 0; k < 5; k++) { if ((uint32_t)k < ntaps) { acc += (int64_t)job.ltm_coef[k] * (int64_t)win[i + k]; } }
          v[i] = (int32_t)((uint32_t)v[i] - (uint32_t)(int32_t)(acc >> 31));
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < SPL; i++) {
        const uint32_t si = s + (uint32_t)i;
        int32_t x = 0;
        if (si < n) {
          x = in[si];
          if (use_ltm && si >= delay) {
            int64_t acc = (int64_t)1 << 30;
            for (uint32_t k = 0; k < ntaps; k++) { acc += (int64_t)job.ltm_coef[k] * (int64_t)in[si - delay + k]; }
            x = (int32_t)((uint32_t)x - (uint32_t)(int32_t)(acc >> 31));
          }
        }
        v[i] = x;
      }
    }
  };

  int addr[LPJ];                                     // ds_bpermute byte address of the job's lane l
#pragma unroll
  for (int l = 0; l < LPJ; l++) { addr[l] = (int)((row * 16 + (uint32_t)l * JPR + jr) * 4); }
  int32_t ca[K], cb[K], ha[K], hb[K], sa[K], sb[K];
#pragma unroll
  for (int a = 0; a < K; a++) { ca[a] = cb[a] = ha[a] = hb[a] = sa[a] = sb[a] = 0; }
  uint64_t fsum = 0;
  int32_t vm_next[SPL];
  fetch_run(0, vm_next);
  for (uint32_t s0 = 0; s0 < nmax; s0 += TAILK_BLK) {
    int32_t vm[SPL], em[SPL];
#pragma unroll
    for (int m = 0; m < SPL; m++) { vm[m] = vm_next[m]; em[m] = 0; }
    fetch_run(s0 + TAILK_BLK, vm_next);                // the next block travels while this one computes
    if (s0 == 0) { tailk_block<ORDER, K, true>(vm, em, addr, L, ca, cb, ha, hb, sa, sb); }
    else if (s0 < 2u * (uint32_t)ORDER || !iir24_ok) { tailk_block<ORDER, K, false>(vm, em, addr, L, ca, cb, ha, hb, sa, sb); }
    else { tailk_block<ORDER, K, false, true>(vm, em, addr, L, ca, cb, ha, hb, sa, sb); }
    const uint32_t s = s0 + L * SPL;
#pragma unroll
    for (int m = 0; m < SPL; m++) {
      em[m] = pass ? vm[m] : em[m];
      if (s + (uint32_t)m < n) { fsum += (em[m] < 0) ? ~((uint32_t)em[m] << 1) : ((uint32_t)em[m] << 1); }      // zig-zag fold, src/SLAUtility.h:37
    }
    if (s + SPL <= n) { tk_store_run<SPL>(out + s, em); }
    else {
#pragma unroll
      for (int m = 0; m < SPL; m++) { if (s + (uint32_t)m < n) { out[s + m] = em[m]; } }
    }
  }
#pragma unroll
  for (int off = JPR; off < 16; off <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)fsum, off);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(fsum >> 32), off);
    fsum += ((uint64_t)hi << 32) | lo;
  }
  if (have && L == 0) {
    fold_sum[j] = fsum;
    if (rice_init != nullptr) { rice_init[j] = rice_init_of(fsum, n); }      // one 64-bit divide per job, on one lane
  }
  span_end(span);
}
