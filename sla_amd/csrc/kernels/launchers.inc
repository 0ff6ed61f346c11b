// kernels/launchers.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): C-ABI launchers of the analysis kernels (include/sla_hip.h)
// ---------------------------------------------------------------------------------------------
// launchers (C-ABI, see include/sla_hip.h)
// ---------------------------------------------------------------------------------------------
// Optional extras of a launch travel in sla_hip_launch_extra (include/sla_hip.h): the two-word slot for its on-device execution
// span (see span_begin), a device-side group count, words to clear on the way.  (Rounds 2 - 3 passed them through thread-local
// one-shot requests that a later commit had to drop at every API entry; now they are arguments.)
static inline unsigned long long* span_of(const sla_hip_launch_extra* x) { return (x != nullptr) ? x->d_span : nullptr; }

// Tuning knobs of the launchers (include/sla_hip.h: sla_hip_tuning).  They belong to an encoder handle, which reads
// them ONCE (environment at SLAEncoder_Create, sla_hip_encoder_set_option afterwards) and names its copy to the
// launchers of its host thread; nothing on the launch path reads the environment.
// The thread keeps a COPY: a handle may be destroyed (or used on another thread) while this thread goes on calling
// launchers directly, and a stale pointer would then read freed memory.
static thread_local sla_hip_tuning t_tuning_val;
static thread_local bool t_tuning_set = false;
extern "C" void sla_hip_use_tuning(const sla_hip_tuning* tuning)
{
  if (tuning != nullptr) { t_tuning_val = *tuning; t_tuning_set = true; } else { t_tuning_set = false; }
}
static inline sla_hip_tuning tuning()
{
  sla_hip_tuning t;
  memset(&t, 0, sizeof(t));
  if (t_tuning_set) { t = t_tuning_val; }
  if (!(t.plan_margin >= PLAN_MARGIN)) { t.plan_margin = 0.0; }      // below the built-in margin: not a valid setting
  return t;
}

// hipFuncSetAttribute costs a driver call; the limit only ever has to grow (per kernel and device)
static hipError_t ensure_dynamic_lds(const void* fn, size_t bytes)
{
  static struct { const void* fn; int dev; size_t bytes; } seen[64];
  static int nseen = 0;
  static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
  int dev = 0;
  (void)hipGetDevice(&dev);
  pthread_mutex_lock(&mu);
  int slot = -1;
  for (int i = 0; i < nseen; i++) { if (seen[i].fn == fn && seen[i].dev == dev) { slot = i; break; } }
  if (slot >= 0 && seen[slot].bytes >= bytes) { pthread_mutex_unlock(&mu); return hipSuccess; }
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) {
    if (slot < 0 && nseen < 64) { slot = nseen++; seen[slot].fn = fn; seen[slot].dev = dev; seen[slot].bytes = 0; }
    if (slot >= 0) { seen[slot].bytes = bytes; }
  }
  pthread_mutex_unlock(&mu);
  return e;
}

static inline int hip_rc(hipError_t e) { return (e == hipSuccess) ? 0 : -(int)e; }

#define LIST_LPC_GRID 256u        // list mode of k_lpc_blocks: workgroups that walk the list of uncertified blocks
#define LIST_FINISH_GRID 64u      // list mode of k_blocks_finish

static int launch_prepass_impl(const int32_t* d_pcm, uint64_t plane_stride, uint32_t num_channels,
                               uint32_t num_samples, uint32_t bits_per_sample, uint32_t mid_side,
                               uint32_t* d_or_mask, uint64_t* d_nz_mask, uint32_t* d_tile_or, sla_hip_stream_t stream,
                               uint32_t* d_early = nullptr, uint32_t max_workgroups = 0)
{
  uint32_t* const cancel = (d_early != nullptr) ? d_early + SLA_HIP_EARLY_CANCEL : nullptr;
  if (d_pcm == nullptr || d_or_mask == nullptr || d_nz_mask == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8 || bits_per_sample == 0 || bits_per_sample > 32
      || plane_stride < num_samples || (mid_side && num_channels != 2)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(d_or_mask, 0, 2 * sizeof(uint32_t), st);
  if (e != hipSuccess) { return hip_rc(e); }
  if (num_samples == 0) {
    if (d_early != nullptr) { hipLaunchKernelGGL(k_prepass_done, dim3(1), dim3(64), 0, st, (const uint32_t*)d_or_mask, bits_per_sample, d_early); return hip_rc(hipGetLastError()); }
    return 0;
  }
  uint64_t nwords = ((uint64_t)num_samples + 63) / 64;
  uint32_t nblocks = (uint32_t)((nwords + 4 * PREPASS_WORDS - 1) / (4 * PREPASS_WORDS));
  const uint32_t shift = 32u - bits_per_sample;
  uint32_t wave_stride = 0;
  if (max_workgroups != 0 && max_workgroups < nblocks) { nblocks = max_workgroups; wave_stride = 4u * nblocks; }
  if (num_channels == 1) {
    hipLaunchKernelGGL(k_prepass<1>, dim3(nblocks), dim3(256), 0, st, d_pcm, plane_stride, num_channels, num_samples, shift, mid_side, d_or_mask, d_nz_mask, d_tile_or, cancel, wave_stride);
  } else if (num_channels == 2) {
    hipLaunchKernelGGL(k_prepass<2>, dim3(nblocks), dim3(256), 0, st, d_pcm, plane_stride, num_channels, num_samples, shift, mid_side, d_or_mask, d_nz_mask, d_tile_or, cancel, wave_stride);
  } else {
    hipLaunchKernelGGL(k_prepass<0>, dim3(nblocks), dim3(256), 0, st, d_pcm, plane_stride, num_channels, num_samples, shift, mid_side, d_or_mask, d_nz_mask, d_tile_or, cancel, wave_stride);
  }
  if (d_early != nullptr) {
    e = hipGetLastError();
    if (e != hipSuccess) { return hip_rc(e); }
    hipLaunchKernelGGL(k_prepass_done, dim3(1), dim3(64), 0, st, (const uint32_t*)d_or_mask, bits_per_sample, d_early);
  }
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_prepass_early(const int32_t* d_pcm, uint64_t plane_stride, uint32_t num_channels,
                                            uint32_t num_samples, uint32_t bits_per_sample, uint32_t mid_side,
                                            uint32_t* d_or_mask, uint64_t* d_nz_mask, uint32_t* d_early, uint32_t max_workgroups,
                                            sla_hip_stream_t stream)
{
  if (d_early == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  return launch_prepass_impl(d_pcm, plane_stride, num_channels, num_samples, bits_per_sample, mid_side, d_or_mask, d_nz_mask, nullptr, stream, d_early,
                             max_workgroups);
}

extern "C" int sla_hip_launch_prepass(const int32_t* d_pcm, uint64_t plane_stride, uint32_t num_channels,
                                      uint32_t num_samples, uint32_t bits_per_sample, uint32_t mid_side,
                                      uint32_t* d_or_mask, uint64_t* d_nz_mask, sla_hip_stream_t stream)
{
  return launch_prepass_impl(d_pcm, plane_stride, num_channels, num_samples, bits_per_sample, mid_side, d_or_mask, d_nz_mask, nullptr, stream);
}

extern "C" int sla_hip_launch_batch_scan(const uint64_t* d_nz_mask, const uint32_t* d_tile_or, const uint32_t* d_file_start,
                                         const uint32_t* d_file_len, uint32_t num_files, uint32_t max_block_samples,
                                         uint32_t* d_info, sla_hip_stream_t stream)
{
  if (d_nz_mask == nullptr || d_tile_or == nullptr || d_file_start == nullptr || d_file_len == nullptr || d_info == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_files == 0) { return 0; }
  hipLaunchKernelGGL(k_batch_scan, dim3(num_files), dim3(256), 0, (hipStream_t)stream, d_nz_mask, d_tile_or, d_file_start, d_file_len, max_block_samples, d_info);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_zero_runs(const uint64_t* d_nz_mask, uint32_t span,
                                        const uint32_t* d_seg_start, const uint32_t* d_seg_len, uint32_t num_segs,
                                        uint32_t min_run, sla_hip_zero_run* d_runs, uint32_t capacity,
                                        uint32_t* d_count, uint32_t* d_scratch, sla_hip_stream_t stream)
{
  if (d_nz_mask == nullptr || d_runs == nullptr || d_count == nullptr || d_scratch == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (((uintptr_t)d_nz_mask & 15u) != 0 || ((uintptr_t)d_scratch & 3u) != 0 || ((uintptr_t)d_count & 3u) != 0 || ((uintptr_t)d_runs & 3u) != 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (capacity == 0 || min_run < 64u || span > SLA_HIP_ZERO_RUN_MAX_SPAN) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (d_seg_start != nullptr && (d_seg_len == nullptr || num_segs == 0)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  hipStream_t st = (hipStream_t)stream;
  if (d_seg_start == nullptr) { d_seg_len = nullptr; num_segs = 1; }
  // (a span of no samples still runs: the first kernel zeroes the count, one workgroup over a mask of no words)
  const uint64_t nwords = ((uint64_t)span + 63) / 64;
  uint32_t ntiles = (uint32_t)((nwords + SLA_HIP_ZERO_RUN_TILE - 1) / SLA_HIP_ZERO_RUN_TILE);
  if (ntiles == 0) { ntiles = 1; }
  const uint32_t seg_blocks = (num_segs + ZR_GROUPS - 1) / ZR_GROUPS;
  hipLaunchKernelGGL(k_zero_run_tiles, dim3(ntiles), dim3(64 * ZR_GROUPS), 0, st, d_nz_mask, span, d_scratch, d_count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { return hip_rc(e); }
  hipLaunchKernelGGL(k_zero_run_list, dim3(ntiles + seg_blocks), dim3(64 * ZR_GROUPS), 0, st, d_nz_mask, span, d_seg_start, d_seg_len, num_segs,
                     min_run, ntiles, (const uint32_t*)d_scratch, d_runs, capacity, d_count);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_prepass_tiles(const int32_t* d_pcm, uint64_t plane_stride, uint32_t num_channels,
                                            uint32_t num_samples, uint32_t bits_per_sample, uint32_t mid_side,
                                            uint32_t* d_or_mask, uint64_t* d_nz_mask, uint32_t* d_tile_or, sla_hip_stream_t stream)
{
  if (d_tile_or == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  return launch_prepass_impl(d_pcm, plane_stride, num_channels, num_samples, bits_per_sample, mid_side, d_or_mask, d_nz_mask, d_tile_or, stream);
}

static int launch_lpc_impl(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                           const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                           uint32_t max_cands_per_group,
                           const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                           double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                           sla_hip_stream_t stream, uint32_t mode_flags, uint32_t* d_rerun_counter, int32_t* d_lat_residual,
                           const uint32_t* list = nullptr, const uint32_t* list_count = nullptr, uint32_t* d_cert_flag = nullptr,
                           uint32_t audit_bps = 0u, unsigned long long* span = nullptr);

extern "C" int sla_hip_launch_lpc_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                  const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                  uint32_t max_cands_per_group,
                                  const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                                  double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                                  sla_hip_stream_t stream, const sla_hip_launch_extra* extra)
{
  return launch_lpc_impl(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, max_cands_per_group, d_cands,
                         d_window_pool, d_out, d_code, d_kint, d_rshift, stream, 0u, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, span_of(extra));
}

extern "C" int sla_hip_launch_lpc(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                  const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                  uint32_t max_cands_per_group,
                                  const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                                  double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                                  sla_hip_stream_t stream)
{
  return sla_hip_launch_lpc_x(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, max_cands_per_group, d_cands, d_window_pool, d_out, d_code, d_kint, d_rshift, stream, nullptr);
}

extern "C" int sla_hip_launch_lpc_blocks_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                         const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                         const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                                         double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                                         int32_t* d_lattice_residual, sla_hip_stream_t stream, const sla_hip_launch_extra* extra)
{
  if (d_code == nullptr || d_lattice_residual == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  return launch_lpc_impl(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, 1, d_cands,
                         d_window_pool, d_out, d_code, d_kint, d_rshift, stream, 0u, nullptr, d_lattice_residual, nullptr, nullptr, nullptr, 0u, span_of(extra));
}

extern "C" int sla_hip_launch_lpc_blocks(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                         const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                         const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                                         double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                                         int32_t* d_lattice_residual, sla_hip_stream_t stream)
{
  return sla_hip_launch_lpc_blocks_x(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, d_cands, d_window_pool, d_out, d_code, d_kint, d_rshift, d_lattice_residual, stream, nullptr);
}

// k_acf_blocks in the instantiation that serves `order` (lags = sla_hip_search_exact_lags(order) != 0): the one place that
// chooses it, for the certified block stage and for sla_hip_launch_acf_blocks, which shows the sums to the tests.
// The lags that have a reader: order + 1.  The BASELINE orders 16 / 32 / 48 leave three lags of the last block of four without
// one and get kernels that do not compute them; every other order keeps the full blocks.
static void launch_acf_blocks(uint32_t lags, const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                              const sla_hip_lpc_group* d_groups, uint32_t num_groups, const double* d_window_pool,
                              double* d_out, uint32_t* d_rshift, hipStream_t st, unsigned long long* span,
                              uint32_t* zero_word, const uint32_t* dyn)
{
  const dim3 grid((num_groups + 3) / 4), block(256);
#define SLA_ACFB(NBB, TOPP) do { \
    if (mid_side) { hipLaunchKernelGGL((k_acf_blocks<NBB, TOPP, true>), grid, block, 0, st, d_pcm, plane_stride, order, d_groups, num_groups, d_window_pool, d_out, d_rshift, span, zero_word, dyn); } \
    else { hipLaunchKernelGGL((k_acf_blocks<NBB, TOPP, false>), grid, block, 0, st, d_pcm, plane_stride, order, d_groups, num_groups, d_window_pool, d_out, d_rshift, span, zero_word, dyn); } } while (0)
  switch (lags) {
    case 12: SLA_ACFB(3, 12); break;
    case 20: if (order == 16) { SLA_ACFB(5, 17); } else { SLA_ACFB(5, 20); } break;
    case 36: if (order == 32) { SLA_ACFB(9, 33); } else { SLA_ACFB(9, 36); } break;
    default: if (order == 48) { SLA_ACFB(13, 49); } else { SLA_ACFB(13, 52); } break;
  }
#undef SLA_ACFB
}

extern "C" int sla_hip_launch_acf_blocks(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                         const sla_hip_lpc_group* d_groups, uint32_t num_groups, const double* d_window_pool,
                                         double* d_out, uint32_t* d_rshift, sla_hip_stream_t stream)
{
  if (d_pcm == nullptr || d_groups == nullptr || d_window_pool == nullptr || d_out == nullptr || d_rshift == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (order < 1) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  const uint32_t lags = sla_hip_search_exact_lags(order);
  if (lags == 0) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }      // orders above 51 (more than 52 lags)
  if (num_groups == 0) { return 0; }
  launch_acf_blocks(lags, d_pcm, plane_stride, mid_side, order, d_groups, num_groups, d_window_pool, d_out, d_rshift, (hipStream_t)stream,
                    nullptr, nullptr, nullptr);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_lpc_blocks_cert_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                              const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                              const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                                              double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                                              uint32_t* d_cert_flag, uint32_t* d_fallback_list, uint32_t* d_fallback_count,
                                              double safety, uint32_t bits_per_sample, sla_hip_stream_t stream,
                                                const sla_hip_launch_extra* extra)
{
  if (d_pcm == nullptr || d_groups == nullptr || d_cands == nullptr || d_window_pool == nullptr || d_out == nullptr || d_code == nullptr
      || d_kint == nullptr || d_rshift == nullptr || d_cert_flag == nullptr || d_fallback_list == nullptr || d_fallback_count == nullptr) {
    return SLA_APIRESULT_INVALID_ARGUMENT;
  }
  if (order < 1 || max_window == 0 || bits_per_sample == 0 || bits_per_sample > 32 || !(safety >= 1.0)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  const uint32_t lags = sla_hip_search_exact_lags(order);
  if (lags == 0) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }      // orders above 51 (more than 52 lags): the exact kernels only
  if (num_groups == 0) { return 0; }
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  unsigned long long* span = span_of(extra);
  const uint32_t* dyn = (extra != nullptr) ? extra->d_group_count : nullptr;      // num_groups is then an upper bound, the kernels read the number
  launch_acf_blocks(lags, d_pcm, plane_stride, mid_side, order, d_groups, num_groups, d_window_pool, d_out, d_rshift, st, span, d_fallback_count, dyn);
  e = hipGetLastError();
  if (e != hipSuccess) { return hip_rc(e); }
  const dim3 fgrid((num_groups + 63) / 64), fblock(64);
  const uint32_t audit_every = tuning().cert_audit;
#define SLA_FINC(PP) hipLaunchKernelGGL((k_blocks_finish<PP, true>), fgrid, fblock, 0, st, d_groups, num_groups, order, d_out, d_code, d_kint, \
                                        d_rshift, (const uint32_t*)nullptr, (const uint32_t*)nullptr, d_cert_flag, d_fallback_list, d_fallback_count, safety, bits_per_sample, dyn, audit_every)
  if (order <= 16) { SLA_FINC(16); } else if (order <= 32) { SLA_FINC(32); } else if (order <= 48) { SLA_FINC(48); } else { SLA_FINC(64); }
#undef SLA_FINC
  e = hipGetLastError();
  if (e != hipSuccess) { return hip_rc(e); }
  // whatever could not be certified: the exact kernels over the list the finish kernel left (usually empty)
  return launch_lpc_impl(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, 1, d_cands,
                         d_window_pool, d_out, d_code, d_kint, d_rshift, stream, 0u, nullptr, nullptr,
                         d_fallback_list, d_fallback_count, d_cert_flag, bits_per_sample);
}

extern "C" int sla_hip_launch_lpc_blocks_cert(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                              const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                              const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                                              double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                                              uint32_t* d_cert_flag, uint32_t* d_fallback_list, uint32_t* d_fallback_count,
                                              double safety, uint32_t bits_per_sample, sla_hip_stream_t stream)
{
  return sla_hip_launch_lpc_blocks_cert_x(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, d_cands, d_window_pool, d_out, d_code,
                                          d_kint, d_rshift, d_cert_flag, d_fallback_list, d_fallback_count, safety, bits_per_sample, stream, nullptr);
}

extern "C" int sla_hip_launch_lpc_rerun(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                        const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                        uint32_t max_cands_per_group, const sla_hip_lpc_cand* d_cands,
                                        double* d_out, uint32_t* d_rerun_counter, sla_hip_stream_t stream)
{
  return launch_lpc_impl(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, max_cands_per_group, d_cands,
                         nullptr, d_out, nullptr, nullptr, nullptr, stream, 128u, d_rerun_counter, nullptr);
}

static int launch_lpc_impl(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                           const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                           uint32_t max_cands_per_group,
                           const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                           double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                           sla_hip_stream_t stream, uint32_t mode_flags, uint32_t* d_rerun_counter, int32_t* d_lat_residual,
                           const uint32_t* list, const uint32_t* list_count, uint32_t* d_cert_flag, uint32_t audit_bps,
                           unsigned long long* span)
{
  if (d_pcm == nullptr || d_groups == nullptr || d_cands == nullptr || d_out == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (order < 1 || order > 255 || max_window == 0 || max_cands_per_group == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if ((d_code != nullptr) != (d_kint != nullptr) || (d_code != nullptr) != (d_rshift != nullptr)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (d_code != nullptr && max_cands_per_group != 1) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_groups == 0) { return 0; }
  const sla_hip_tuning tune = tuning();
  if (list != nullptr && (d_code == nullptr || order > 64 || d_cert_flag == nullptr)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (d_code != nullptr && order <= 64 && (!tune.lpc_blocks_chains || list != nullptr)) {
    // chosen blocks: term tiles + lane-parallel Levinson (k_lpc_blocks)
    if (d_window_pool == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
    // the recursion inside k_lpc_blocks (the fused lattice needs it there) keeps coefficient j in lane j: orders up to 63
    if (d_lat_residual != nullptr && order > SLA_HIP_FUSED_LATTICE_MAX_ORDER) { return SLA_APIRESULT_INVALID_ARGUMENT; }
    uint32_t pmax = 64 / order;
    if (pmax > LPC_MAX_PACK) { pmax = LPC_MAX_PACK; }
    if (pmax > 2) { pmax = 2; }
    if (tune.lpc_pack >= 1 && tune.lpc_pack <= LPC_MAX_PACK && tune.lpc_pack * order <= 64) { pmax = tune.lpc_pack; }
    if (list != nullptr) { pmax = 1; }      // list mode (usually an empty list): the smallest LDS footprint, so that the launch does not wait for whole CUs
    for (uint32_t p = pmax; p >= 1; p--) {
      uint32_t nch = 16;
      while (nch < p * order) { nch <<= 1; }
      const size_t xr = ((size_t)max_window + 1) & ~(size_t)1;       // even: the term rows behind the windows are read as 16-byte pairs
      const uint32_t spl = (nch <= 32) ? 12 : 6;                    // producer lanes per chain: nch * spl <= LB_PRODUCERS
      // steps per tile: 48 for the wide packs (64 chains, 6 producer lanes each: C5-120 s 10.7 -> 10.3 ms per step, a
      // ten-minute order-16 file loses with them: 2.31 -> 2.46 ms) when the longer tiles still fit, else 24
      uint32_t lbk = (spl == 6 && 2u * 48u * p <= LB_PRODUCERS && tune.lpc_tile != 24u && list == nullptr) ? 48u : 24u;
      size_t bytes = sizeof(double) * ((size_t)p * xr + (size_t)2 * (lbk + 2) * nch + (size_t)2 * 2 * lbk * p + (size_t)p * (order + 1));
      if (bytes > SLA_HIP_LDS_BUDGET && lbk == 48u) {
        lbk = 24u;
        bytes = sizeof(double) * ((size_t)p * xr + (size_t)2 * (lbk + 2) * nch + (size_t)2 * 2 * lbk * p + (size_t)p * (order + 1));
      }
      if (bytes > SLA_HIP_LDS_BUDGET) { continue; }
      const void* fn = (spl == 12) ? (const void*)k_lpc_blocks<12, 24> : (lbk == 48u) ? (const void*)k_lpc_blocks<6, 48> : (const void*)k_lpc_blocks<6, 24>;
      hipError_t e = ensure_dynamic_lds(fn, bytes);
      if (e != hipSuccess) { return hip_rc(e); }
      // list mode: a fixed grid walks the list (two workgroups per CU hold what the device can run at once)
      const dim3 grid((list != nullptr) ? LIST_LPC_GRID : (num_groups + p - 1) / p), block(LB_THREADS);
#ifdef SLA_HIP_DEBUG
      const uint32_t clk = (uint32_t)(getenv("SLA_HIP_LPC_CLK") != nullptr);
#else
      const uint32_t clk = 0;
#endif
      // Levinson-Durbin + quantiser: in registers, one lane per window (k_blocks_finish), unless the lattice is fused in
      // (it needs the coefficients inside the workgroup)
      const uint32_t defer = (d_lat_residual == nullptr) ? 1u : 0u;
      if (spl == 12) {
        hipLaunchKernelGGL((k_lpc_blocks<12, 24>), grid, block, bytes, (hipStream_t)stream, d_pcm, plane_stride, mid_side, order,
                           d_groups, num_groups, p, d_window_pool, d_out, d_code, d_kint, d_rshift, (uint32_t)xr, nch, clk, span, d_lat_residual, defer, list, list_count);
      } else if (lbk == 48u) {
        hipLaunchKernelGGL((k_lpc_blocks<6, 48>), grid, block, bytes, (hipStream_t)stream, d_pcm, plane_stride, mid_side, order,
                           d_groups, num_groups, p, d_window_pool, d_out, d_code, d_kint, d_rshift, (uint32_t)xr, nch, clk, span, d_lat_residual, defer, list, list_count);
      } else {
        hipLaunchKernelGGL((k_lpc_blocks<6, 24>), grid, block, bytes, (hipStream_t)stream, d_pcm, plane_stride, mid_side, order,
                           d_groups, num_groups, p, d_window_pool, d_out, d_code, d_kint, d_rshift, (uint32_t)xr, nch, clk, span, d_lat_residual, defer, list, list_count);
      }
      if (defer) {
        const dim3 fgrid((list != nullptr) ? LIST_FINISH_GRID : (num_groups + 63) / 64), fblock(64);
#define SLA_FIN(PP) hipLaunchKernelGGL((k_blocks_finish<PP, false>), fgrid, fblock, 0, (hipStream_t)stream, d_groups, num_groups, order, d_out, d_code, d_kint, \
                                       d_rshift, list, list_count, d_cert_flag, (uint32_t*)nullptr, (uint32_t*)nullptr, 0.0, audit_bps)
        if (order <= 16) { SLA_FIN(16); } else if (order <= 32) { SLA_FIN(32); } else if (order <= 48) { SLA_FIN(48); } else { SLA_FIN(64); }
#undef SLA_FIN
      }
#ifdef SLA_HIP_DEBUG
      if (clk) {
        unsigned long long h[8] = {0}, z[8] = {0};
        (void)hipStreamSynchronize((hipStream_t)stream);
        (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_lpc_clk), sizeof(h));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_lpc_clk), z, sizeof(z));
        int occ = 0; (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, LB_THREADS, bytes);
        if (h[3] != 0) {
          fprintf(stderr, "[k_lpc_blocks] LDS %zu B, %d workgroups per CU; ", bytes, occ);
          fprintf(stderr, "[k_lpc_blocks] %llu workgroups (pack %u), ticks per workgroup: stage %llu, chains %llu (lag consumer busy %llu, producer busy %llu, energy consumer busy %llu), levinson+quantiser %llu\n",
                  h[3], p, h[0] / h[3], h[1] / h[3], h[4] / h[3], h[5] / h[3], h[6] / h[3], h[2] / h[3]);
        }
      }
#endif
      return hip_rc(hipGetLastError());
    }
    return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY;
  }
  if (d_lat_residual != nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }      /* only k_lpc_blocks carries the lattice */
  // windows per workgroup: as many as the LDS budget takes, at most what fills the three chain waves
  size_t x_region = (size_t)max_window;
  const size_t per_group_r = (size_t)max_cands_per_group * (order + 1);
  uint32_t pack = 1;
  for (uint32_t p = 2 /* measured on C2/C3: 2 beats 1 and 4 */; p >= 1; p--) {
    size_t xr = (size_t)max_window;
    if (xr * p < 2 * (size_t)p * max_cands_per_group * (order + 2)) { xr = 2 * (size_t)max_cands_per_group * (order + 2); }
    const size_t bytes = sizeof(double) * ((size_t)p * xr + (size_t)p * per_group_r);
    if (bytes <= SLA_HIP_LDS_BUDGET && ((size_t)(p - 1) * max_cands_per_group * order < 192 || p == 1)) { pack = p; x_region = xr; break; }
  }
  if (tune.lpc_pack >= 1 && tune.lpc_pack < pack) { pack = tune.lpc_pack; }
  if (x_region * pack < 2 * (size_t)pack * max_cands_per_group * (order + 2)) { x_region = 2 * (size_t)max_cands_per_group * (order + 2); }
  size_t lds = sizeof(double) * ((size_t)pack * x_region + (size_t)pack * per_group_r);
  if (lds > SLA_HIP_LDS_BUDGET) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  hipError_t e = ensure_dynamic_lds((const void*)k_lpc, lds);
  if (e != hipSuccess) { return hip_rc(e); }
  // a group with many chains (the partition search: candidates x lags) gets 7 chain waves instead of 3: the window
  // owns the LDS, so the workgroups per CU are few and more waves per workgroup are what hides the LDS gathers
  // (C5: 14.4 -> 13.3 ms of search per minute of audio)
  uint32_t lpc_threads = ((size_t)pack * max_cands_per_group * order >= 448) ? 512u : 256u;
  if (tune.lpc_threads == 256 || tune.lpc_threads == 512) { lpc_threads = tune.lpc_threads; }
  hipLaunchKernelGGL(k_lpc, dim3((num_groups + pack - 1) / pack), dim3(lpc_threads), lds, (hipStream_t)stream, d_pcm, plane_stride, mid_side, order,
                     d_groups, num_groups, pack, d_cands, d_window_pool, d_out, d_code, d_kint, d_rshift, (uint32_t)x_region,
                     mode_flags, d_rerun_counter);
  return hip_rc(hipGetLastError());
}

// The far-window LPC stage (kernels/lpc_far.inc): sla_hip_launch_lpc's semantics for windows of up to 65 535 samples.
// RERUN: only the groups flagged in d_out (sla_hip_launch_lpc_far_rerun; kernels/lpc_far.inc: far_flagged).  The passes of
// unflagged groups are launched all the same and return at their start, as the LDS kernel's rerun does.
template <bool RERUN>
static int launch_lpc_far_impl(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                               const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                               uint32_t max_cands_per_group,
                               const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                               double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                               double* d_scratch, uint32_t scratch_slots,
                               sla_hip_stream_t stream, const sla_hip_launch_extra* extra, uint32_t* d_rerun_counter)
{
  if (d_pcm == nullptr || d_groups == nullptr || d_cands == nullptr || d_out == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (order < 1 || order > 255 || max_window == 0 || max_window > SLA_HIP_LPC_FAR_MAX_WINDOW || max_cands_per_group == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if ((d_code != nullptr) != (d_kint != nullptr) || (d_code != nullptr) != (d_rshift != nullptr)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (d_code != nullptr && (max_cands_per_group != 1 || d_window_pool == nullptr)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (d_scratch == nullptr || scratch_slots == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_groups == 0) { return 0; }
  hipStream_t st = (hipStream_t)stream;
  const uint64_t chains = (uint64_t)max_cands_per_group * (order + 1);
  const uint64_t chunks = (chains + FAR_THREADS - 1) / FAR_THREADS;
  const size_t per_cand = sizeof(double) * (3 * (size_t)order + 5);      // r[order + 1], a[order + 2], v[order + 2]
  uint32_t per_wg = (uint32_t)(FAR_FINISH_LDS / per_cand);
  if (per_wg > 64) { per_wg = 64; }
  if (per_wg > max_cands_per_group) { per_wg = max_cands_per_group; }
  const uint64_t fchunks = ((uint64_t)max_cands_per_group + per_wg - 1) / per_wg;
  const uint32_t pass = (num_groups < scratch_slots) ? num_groups : scratch_slots;
  if (chunks * pass > 0x7FFFFFFFull || fchunks * num_groups > 0x7FFFFFFFull) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  for (uint32_t g_lo = 0; g_lo < num_groups; g_lo += pass) {
    const uint32_t ng = (num_groups - g_lo < pass) ? (num_groups - g_lo) : pass;
    hipLaunchKernelGGL(k_lpc_far_stage<RERUN>, dim3(ng), dim3(FAR_THREADS), 0, st, d_pcm, plane_stride, mid_side, d_groups, g_lo, d_window_pool,
                       d_scratch, max_window, d_rshift, (g_lo == 0) ? span_of(extra) : nullptr, (const double*)d_out, order, d_rerun_counter);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { return hip_rc(e); }
    hipLaunchKernelGGL(k_lpc_far_chains<RERUN>, dim3((uint32_t)(chunks * ng)), dim3(FAR_THREADS), 0, st, d_groups, g_lo, d_cands, order,
                       (const double*)d_scratch, max_window, (uint32_t)chunks, d_out);
    e = hipGetLastError();
    if (e != hipSuccess) { return hip_rc(e); }
  }
  hipLaunchKernelGGL(k_lpc_far_finish<RERUN>, dim3((uint32_t)(fchunks * num_groups)), dim3(64), per_wg * per_cand, st, d_groups, d_cands, order,
                     per_wg, (uint32_t)fchunks, max_window, d_out, d_code, d_kint, (const uint32_t*)d_rshift, span_of(extra));
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_lpc_far_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                        const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                        uint32_t max_cands_per_group,
                                        const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                                        double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                                        double* d_scratch, uint32_t scratch_slots,
                                        sla_hip_stream_t stream, const sla_hip_launch_extra* extra)
{
  return launch_lpc_far_impl<false>(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, max_cands_per_group, d_cands, d_window_pool,
                                    d_out, d_code, d_kint, d_rshift, d_scratch, scratch_slots, stream, extra, nullptr);
}

extern "C" int sla_hip_launch_lpc_far_rerun(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                            const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                            uint32_t max_cands_per_group, const sla_hip_lpc_cand* d_cands,
                                            double* d_out, double* d_scratch, uint32_t scratch_slots,
                                            uint32_t* d_rerun_counter, sla_hip_stream_t stream)
{
  return launch_lpc_far_impl<true>(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, max_cands_per_group, d_cands, nullptr,
                                   d_out, nullptr, nullptr, nullptr, d_scratch, scratch_slots, stream, nullptr, d_rerun_counter);
}

extern "C" int sla_hip_launch_lpc_far(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                      const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                      uint32_t max_cands_per_group,
                                      const sla_hip_lpc_cand* d_cands, const double* d_window_pool,
                                      double* d_out, int32_t* d_code, int32_t* d_kint, uint32_t* d_rshift,
                                      double* d_scratch, uint32_t scratch_slots, sla_hip_stream_t stream)
{
  return sla_hip_launch_lpc_far_x(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, max_cands_per_group, d_cands, d_window_pool,
                                  d_out, d_code, d_kint, d_rshift, d_scratch, scratch_slots, stream, nullptr);
}

extern "C" uint32_t sla_hip_search_exact_lags(uint32_t order)
{
  const uint32_t nb = (order + 1 + 3) / 4;
  if (order < 1) { return 0; }
  return (nb <= 3) ? 12 : (nb <= 5) ? 20 : (nb <= 9) ? 36 : (nb <= 13) ? 52 : 0;
}

static int launch_search_exact_impl(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                           const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                           uint32_t max_cands_per_group,
                                           const sla_hip_lpc_cand* d_cands, double* d_tile_sums, double* d_out,
                                           double exact_limit, double cert_safety, uint32_t* d_any_exact, sla_hip_stream_t stream, const sla_hip_launch_extra* extra,
                                           const uint32_t* d_early, void* prepass_done)
{
  if (d_pcm == nullptr || d_groups == nullptr || d_cands == nullptr || d_tile_sums == nullptr || d_out == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  const uint32_t lags = sla_hip_search_exact_lags(order);
  if (lags == 0 || max_window > SLA_HIP_XTILE * SLA_HIP_XTILES) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  if (max_window == 0 || max_cands_per_group == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_groups == 0) { return 0; }
  hipStream_t st = (hipStream_t)stream;
  clear_list cl = {{nullptr, nullptr, nullptr, nullptr}, {0, 0, 0, 0}};      // what the caller asked to have cleared on the way
  if (extra != nullptr) { for (int i = 0; i < 3; i++) { cl.ptr[i] = extra->clear_ptr[i]; cl.words[i] = extra->clear_words[i]; } }
  cl.ptr[3] = d_any_exact; cl.words[3] = (d_any_exact != nullptr) ? 1u : 0u;      // the flag k_search_finish raises
  const uint32_t tiles = (max_window + SLA_HIP_XTILE - 1) / SLA_HIP_XTILE;       // waves per group
  const uint32_t waves = num_groups * tiles;
  const dim3 grid((waves + 3) / 4), block(256);
  switch (lags) {
    case 12: hipLaunchKernelGGL(k_acf_tiles<3>, grid, block, 0, st, d_pcm, plane_stride, mid_side, d_groups, num_groups, tiles, d_tile_sums, cl, d_early); break;
    // (lag slots that no order <= `order` reads stay unwritten: orders 16 / 32 / 48 skip the top three of 20 / 36 / 52)
#define SLA_ACFT(NBB, TOPP) hipLaunchKernelGGL((k_acf_tiles_lds<NBB, TOPP>), grid, block, 0, st, d_pcm, plane_stride, mid_side, d_groups, num_groups, tiles, d_tile_sums, cl, d_early)
    case 20: if (order == 16) { SLA_ACFT(5, 17); } else { SLA_ACFT(5, 20); } break;
    case 36: if (order == 32) { SLA_ACFT(9, 33); } else { SLA_ACFT(9, 36); } break;
    default: if (order == 48) { SLA_ACFT(13, 49); } else { SLA_ACFT(13, 52); } break;
#undef SLA_ACFT
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { return hip_rc(e); }
  if (prepass_done != nullptr) {
    // the tile sums need nothing from the prepass and run beside it; what follows reads the offset_lshift it stores
    e = hipStreamWaitEvent(st, (hipEvent_t)prepass_done, 0);
    if (e != hipSuccess) { return hip_rc(e); }
  }
  // lanes = (group, candidate): `per` candidate slots per group and pass, `gpw` groups per wave
  const uint32_t per = (max_cands_per_group < XF_BATCH) ? max_cands_per_group : XF_BATCH;
  uint32_t gpw = XF_BATCH / per;
  if (gpw > XF_GROUPS) { gpw = XF_GROUPS; }
  if (gpw < 1) { gpw = 1; }
  const size_t lds_r = sizeof(double) * (size_t)gpw * per * (order + 1);
  // (the exact windows of mixed material run the recursion in registers as well: a launch that needs 70 KiB of LDS per
  // workgroup waits for CUs that the other streams' kernels have left that much of, even when -- loud material wider than
  // 16 bits -- it has nothing to do)
  // |x| < 2 in the search's unit (mid/side: side = l - r), so a window's energy stays below 4 x its length: when even
  // that is under the limit (16-bit material) every group takes the exact path and one launch does
  const bool all_exact = (exact_limit >= 4.0 * (double)max_window);
  const int pclass = (order <= 16) ? 16 : (order <= 32) ? 32 : (order <= 48) ? 48 : 64;      // (lags != 0: order <= 51)
#define SLA_FINISH(PP) do { \
    if (all_exact) { \
      e = ensure_dynamic_lds((const void*)k_search_finish<PP, 0>, lds_r); \
      if (e != hipSuccess) { return hip_rc(e); } \
      hipLaunchKernelGGL((k_search_finish<PP, 0>), dim3((num_groups + gpw - 1) / gpw), dim3(64), lds_r, st, order, lags, gpw, per, \
                         d_groups, num_groups, d_cands, d_tile_sums, d_out, exact_limit, cert_safety, d_any_exact, d_early); \
    } else { \
      e = ensure_dynamic_lds((const void*)k_search_finish<PP, 1>, lds_r); \
      if (e != hipSuccess) { return hip_rc(e); } \
      e = ensure_dynamic_lds((const void*)k_search_finish<PP, 2>, lds_r); \
      if (e != hipSuccess) { return hip_rc(e); } \
      if (cert_safety > 0.0) { \
        const uint64_t slots_bound = (uint64_t)num_groups * max_cands_per_group; \
        /* dynamic LDS: the tile sums of the groups a wave's 32 slots touch (XC_STAGE doubles: five groups of four 36-lag tiles, two of \
         * eight 52-lag tiles), then r[32][order + 1] in the same place */ \
        /* (staged where a window has six tiles or more -- 8192-sample frames: certificate 0.58 -> 0.36 ms per C5-240 s launch; with the \
         * four tiles of a 4096-sample window the sweep fetched more than the sums it replaced and cost a workgroup per CU: 0.29 -> 0.36) */ \
        const uint32_t win_tiles = (max_window + SLA_HIP_XTILE - 1) / SLA_HIP_XTILE, stage = (win_tiles >= 6u) ? XC_STAGE : 0u; \
        const uint32_t r_doubles = XC_CANDS * (order + 1), lds_doubles = (r_doubles > stage) ? r_doubles : stage; \
        hipLaunchKernelGGL((k_search_cert<PP>), dim3((uint32_t)((slots_bound + XC_CANDS - 1) / XC_CANDS)), dim3(64), sizeof(double) * lds_doubles, st, \
                           order, lags, max_cands_per_group, d_groups, num_groups, d_cands, d_tile_sums, d_out, exact_limit, cert_safety, d_any_exact, stage ? lds_doubles : 0u, d_early); \
      } else { \
      hipLaunchKernelGGL((k_search_finish<PP, 1>), dim3((num_groups + gpw - 1) / gpw), dim3(64), lds_r, st, order, lags, gpw, per, \
                         d_groups, num_groups, d_cands, d_tile_sums, d_out, exact_limit, cert_safety, d_any_exact, d_early); \
      } \
      hipLaunchKernelGGL((k_search_finish<PP, 2>), dim3((num_groups + gpw - 1) / gpw), dim3(64), lds_r, st, order, lags, gpw, per, \
                         d_groups, num_groups, d_cands, d_tile_sums, d_out, exact_limit, cert_safety, d_any_exact, d_early); \
    } } while (0)
  switch (pclass) {
    case 16: SLA_FINISH(16); break;
    case 32: SLA_FINISH(32); break;
    case 48: SLA_FINISH(48); break;
    default: SLA_FINISH(64); break;
  }
#undef SLA_FINISH
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_search_exact_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                           const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                           uint32_t max_cands_per_group,
                                           const sla_hip_lpc_cand* d_cands, double* d_tile_sums, double* d_out,
                                           double exact_limit, double cert_safety, uint32_t* d_any_exact, sla_hip_stream_t stream, const sla_hip_launch_extra* extra)
{
  return launch_search_exact_impl(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, max_cands_per_group, d_cands, d_tile_sums, d_out,
                                  exact_limit, cert_safety, d_any_exact, stream, extra, nullptr, nullptr);
}

extern "C" int sla_hip_launch_search_exact_early(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                           const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                           uint32_t max_cands_per_group,
                                           const sla_hip_lpc_cand* d_cands, double* d_tile_sums, double* d_out,
                                           double exact_limit, double cert_safety, uint32_t* d_any_exact, sla_hip_stream_t stream, const sla_hip_launch_extra* extra,
                                           const uint32_t* d_early, void* prepass_done)
{
  // (a launch of no groups would queue no wait: the kernels behind it on the stream would not be ordered behind the prepass)
  if (d_early == nullptr || prepass_done == nullptr || num_groups == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  return launch_search_exact_impl(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, max_cands_per_group, d_cands, d_tile_sums, d_out,
                                  exact_limit, cert_safety, d_any_exact, stream, extra, d_early, prepass_done);
}

extern "C" int sla_hip_launch_search_exact(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                           const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                           uint32_t max_cands_per_group,
                                           const sla_hip_lpc_cand* d_cands, double* d_tile_sums, double* d_out,
                                           double exact_limit, double cert_safety, uint32_t* d_any_exact, sla_hip_stream_t stream)
{
  return sla_hip_launch_search_exact_x(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, max_cands_per_group, d_cands, d_tile_sums, d_out, exact_limit, cert_safety, d_any_exact, stream, nullptr);
}

// The tile-sum search for windows of up to 64 tiles: the tile kernels of launch_search_exact_impl with the far stride, then
// k_search_finish_far (kernels/search_far.inc).  Exact form only: no certificate, no form beside the prepass.
extern "C" int sla_hip_launch_search_far_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                           const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                           uint32_t max_cands_per_group,
                                           const sla_hip_lpc_cand* d_cands, double* d_tile_sums, double* d_out,
                                           double exact_limit, sla_hip_stream_t stream, const sla_hip_launch_extra* extra)
{
  if (d_pcm == nullptr || d_groups == nullptr || d_cands == nullptr || d_tile_sums == nullptr || d_out == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  const uint32_t lags = sla_hip_search_exact_lags(order);
  if (lags == 0 || max_window > SLA_HIP_LPC_FAR_MAX_WINDOW) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  if (max_window == 0 || max_cands_per_group == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_groups == 0) { return 0; }
  hipStream_t st = (hipStream_t)stream;
  clear_list cl = {{nullptr, nullptr, nullptr, nullptr}, {0, 0, 0, 0}};
  if (extra != nullptr) { for (int i = 0; i < 3; i++) { cl.ptr[i] = extra->clear_ptr[i]; cl.words[i] = extra->clear_words[i]; } }
  const uint32_t tiles = (max_window + SLA_HIP_XTILE - 1) / SLA_HIP_XTILE;       // waves per group, <= SLA_HIP_XTILES_FAR
  const uint64_t waves = (uint64_t)num_groups * tiles;
  const uint64_t fchunks = ((uint64_t)max_cands_per_group + XFF_THREADS - 1) / XFF_THREADS;
  if (waves > 0x7FFFFFFFull || fchunks * num_groups > 0x7FFFFFFFull) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  const dim3 grid((uint32_t)((waves + 3) / 4)), block(256);
  const uint32_t* no_early = nullptr;
  switch (lags) {
    case 12: hipLaunchKernelGGL((k_acf_tiles<3, SLA_HIP_XTILES_FAR>), grid, block, 0, st, d_pcm, plane_stride, mid_side, d_groups, num_groups, tiles, d_tile_sums, cl, no_early); break;
#define SLA_ACFT(NBB, TOPP) hipLaunchKernelGGL((k_acf_tiles_lds<NBB, TOPP, SLA_HIP_XTILES_FAR>), grid, block, 0, st, d_pcm, plane_stride, mid_side, d_groups, num_groups, tiles, d_tile_sums, cl, no_early)
    case 20: if (order == 16) { SLA_ACFT(5, 17); } else { SLA_ACFT(5, 20); } break;
    case 36: if (order == 32) { SLA_ACFT(9, 33); } else { SLA_ACFT(9, 36); } break;
    default: if (order == 48) { SLA_ACFT(13, 49); } else { SLA_ACFT(13, 52); } break;
#undef SLA_ACFT
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { return hip_rc(e); }
  const size_t lds = sizeof(double) * (size_t)(order + 1) * (XFF_PSTRIDE + SLA_HIP_XTILES_FAR);      // 53 KiB at order 51
  const dim3 fgrid((uint32_t)(fchunks * num_groups)), fblock(XFF_THREADS);
#define SLA_FINISH_FAR(PP) do { \
    e = ensure_dynamic_lds((const void*)k_search_finish_far<PP>, lds); \
    if (e != hipSuccess) { return hip_rc(e); } \
    hipLaunchKernelGGL((k_search_finish_far<PP>), fgrid, fblock, lds, st, order, lags, (uint32_t)fchunks, d_groups, d_cands, \
                       (const double*)d_tile_sums, d_out, exact_limit, span_of(extra)); } while (0)
  if (order <= 16) { SLA_FINISH_FAR(16); } else if (order <= 32) { SLA_FINISH_FAR(32); } else if (order <= 48) { SLA_FINISH_FAR(48); } else { SLA_FINISH_FAR(64); }
#undef SLA_FINISH_FAR
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_search_far(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                         const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                         uint32_t max_cands_per_group,
                                         const sla_hip_lpc_cand* d_cands, double* d_tile_sums, double* d_out,
                                         double exact_limit, sla_hip_stream_t stream)
{
  return sla_hip_launch_search_far_x(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, max_cands_per_group, d_cands, d_tile_sums, d_out, exact_limit, stream, nullptr);
}

extern "C" int sla_hip_launch_plan_early(const sla_hip_lpc_group* d_groups, uint32_t num_superframes, uint32_t num_channels,
                                   uint32_t order, uint32_t bits_per_sample, const sla_hip_lpc_cand* d_cands,
                                   double* d_lpc_out, uint32_t* d_parts, uint32_t* d_num_parts, uint32_t* d_status,
                                   sla_hip_stream_t stream, const uint32_t* d_early)
{
  if (d_groups == nullptr || d_cands == nullptr || d_lpc_out == nullptr || d_parts == nullptr || d_num_parts == nullptr
      || d_status == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8 || order < 1 || bits_per_sample == 0 || bits_per_sample > 32) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_superframes == 0) { return 0; }
  hipLaunchKernelGGL(k_plan, dim3((num_superframes + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_groups, num_superframes, num_channels,
                     order, bits_per_sample, d_cands, d_lpc_out, d_parts, d_num_parts, d_status,
                     (tuning().plan_margin > 0.0) ? tuning().plan_margin : PLAN_MARGIN,   /* tests raise it to force the host path */
                     d_early);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_plan(const sla_hip_lpc_group* d_groups, uint32_t num_superframes, uint32_t num_channels,
                                   uint32_t order, uint32_t bits_per_sample, const sla_hip_lpc_cand* d_cands,
                                   double* d_lpc_out, uint32_t* d_parts, uint32_t* d_num_parts, uint32_t* d_status,
                                   sla_hip_stream_t stream)
{
  return sla_hip_launch_plan_early(d_groups, num_superframes, num_channels, order, bits_per_sample, d_cands, d_lpc_out, d_parts, d_num_parts, d_status,
                                   stream, nullptr);
}

extern "C" int sla_hip_launch_expand_masked(const sla_hip_superframe* d_superframes, uint32_t num_superframes,
                                     const uint32_t* d_parts, const uint32_t* d_num_parts, const uint32_t* d_status,
                                     uint32_t num_channels, uint32_t int_shift,
                                     const uint32_t* d_win_len, const uint32_t* d_win_off, uint32_t num_windows,
                                     uint32_t* d_run, uint32_t* d_prefix, sla_hip_lpc_group* d_groups, sla_hip_lpc_cand* d_cands,
                                     sla_hip_acf_job* d_acf_jobs, uint32_t group_capacity,
                                     uint32_t* counts, uint32_t sequence, const uint64_t* d_nonzero_mask, sla_hip_stream_t stream);

extern "C" int sla_hip_launch_expand(const sla_hip_superframe* d_superframes, uint32_t num_superframes,
                                     const uint32_t* d_parts, const uint32_t* d_num_parts, const uint32_t* d_status,
                                     uint32_t num_channels, uint32_t int_shift,
                                     const uint32_t* d_win_len, const uint32_t* d_win_off, uint32_t num_windows,
                                     uint32_t* d_run, uint32_t* d_prefix, sla_hip_lpc_group* d_groups, sla_hip_lpc_cand* d_cands,
                                     sla_hip_acf_job* d_acf_jobs, uint32_t group_capacity,
                                     uint32_t* counts, uint32_t sequence, sla_hip_stream_t stream)
{
  return sla_hip_launch_expand_masked(d_superframes, num_superframes, d_parts, d_num_parts, d_status, num_channels, int_shift, d_win_len,
                                      d_win_off, num_windows, d_run, d_prefix, d_groups, d_cands, d_acf_jobs, group_capacity, counts, sequence,
                                      nullptr, stream);
}

extern "C" int sla_hip_launch_expand_masked(const sla_hip_superframe* d_superframes, uint32_t num_superframes,
                                     const uint32_t* d_parts, const uint32_t* d_num_parts, const uint32_t* d_status,
                                     uint32_t num_channels, uint32_t int_shift,
                                     const uint32_t* d_win_len, const uint32_t* d_win_off, uint32_t num_windows,
                                     uint32_t* d_run, uint32_t* d_prefix, sla_hip_lpc_group* d_groups, sla_hip_lpc_cand* d_cands,
                                     sla_hip_acf_job* d_acf_jobs, uint32_t group_capacity,
                                     uint32_t* counts, uint32_t sequence, const uint64_t* d_nonzero_mask, sla_hip_stream_t stream)
{
  return sla_hip_launch_expand_early(d_superframes, num_superframes, d_parts, d_num_parts, d_status, num_channels, int_shift, d_win_len,
                                     d_win_off, num_windows, d_run, d_prefix, d_groups, d_cands, d_acf_jobs, group_capacity, counts, sequence,
                                     d_nonzero_mask, stream, nullptr);
}

extern "C" int sla_hip_launch_expand_early(const sla_hip_superframe* d_superframes, uint32_t num_superframes,
                                     const uint32_t* d_parts, const uint32_t* d_num_parts, const uint32_t* d_status,
                                     uint32_t num_channels, uint32_t int_shift,
                                     const uint32_t* d_win_len, const uint32_t* d_win_off, uint32_t num_windows,
                                     uint32_t* d_run, uint32_t* d_prefix, sla_hip_lpc_group* d_groups, sla_hip_lpc_cand* d_cands,
                                     sla_hip_acf_job* d_acf_jobs, uint32_t group_capacity,
                                     uint32_t* counts, uint32_t sequence, const uint64_t* d_nonzero_mask, sla_hip_stream_t stream,
                                     const uint32_t* d_early)
{
  if (d_superframes == nullptr || d_parts == nullptr || d_num_parts == nullptr || d_status == nullptr || d_run == nullptr
      || d_prefix == nullptr || d_groups == nullptr || d_cands == nullptr || d_acf_jobs == nullptr || counts == nullptr
      || (num_windows != 0 && (d_win_len == nullptr || d_win_off == nullptr))) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8 || int_shift > 31) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  hipLaunchKernelGGL(k_expand_scan, dim3(1), dim3(EXPAND_THREADS), 0, (hipStream_t)stream, d_superframes, num_superframes, d_parts,
                     d_num_parts, d_status, num_channels, d_win_len, num_windows, d_run, d_prefix, group_capacity,
                     (volatile uint32_t*)counts, sequence, d_nonzero_mask, d_early);
  if (num_superframes != 0) {
    hipLaunchKernelGGL(k_expand_write, dim3((num_superframes + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_superframes, num_superframes,
                       d_parts, d_num_parts, num_channels, int_shift, d_win_len, d_win_off, num_windows, d_run, d_prefix, d_groups, d_cands,
                       d_acf_jobs, d_nonzero_mask, d_early);
  }
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_lattice(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                      const sla_hip_lattice_chunk* d_chunks, uint32_t num_chunks,
                                      const int32_t* d_kint, int32_t* d_residual, sla_hip_stream_t stream)
{
  if (d_pcm == nullptr || d_chunks == nullptr || d_kint == nullptr || d_residual == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (order < 1 || order > 255 || (order + LAT_T - 1) / LAT_T >= 32) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_chunks == 0) { return 0; }
  hipLaunchKernelGGL(k_lattice, dim3((num_chunks + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_pcm, plane_stride,
                     mid_side, order, d_chunks, num_chunks, d_kint, d_residual, (unsigned long long*)nullptr, tuning().lattice_plain ? 2u : 0u);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_lattice_groups_x(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                             const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                             const int32_t* d_kint, int32_t* d_residual, sla_hip_stream_t stream, const sla_hip_launch_extra* extra)
{
  if (d_pcm == nullptr || d_groups == nullptr || d_kint == nullptr || d_residual == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (order < 1 || order > 255 || (order + LAT_T - 1) / LAT_T >= 32 || max_window == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_groups == 0) { return 0; }
  const uint32_t per = (SLA_WAVE - (order + LAT_T - 1) / LAT_T) * LAT_T;
  const uint32_t cpg = (max_window + per - 1) / per;
  const uint64_t waves = (uint64_t)num_groups * cpg;
  if (waves > 0x7FFFFFFFull) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  hipLaunchKernelGGL(k_lattice_groups, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_pcm, plane_stride,
                     mid_side, order, d_groups, num_groups, cpg, d_kint, d_residual, span_of(extra), tuning().lattice_plain ? 2u : 0u);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_lattice_groups(const int32_t* d_pcm, uint64_t plane_stride, uint32_t mid_side, uint32_t order,
                                             const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                             const int32_t* d_kint, int32_t* d_residual, sla_hip_stream_t stream)
{
  return sla_hip_launch_lattice_groups_x(d_pcm, plane_stride, mid_side, order, d_groups, num_groups, max_window, d_kint, d_residual, stream, nullptr);
}

extern "C" uint32_t sla_hip_lattice_chunk_samples(uint32_t order)
{
  return (SLA_WAVE - (order + LAT_T - 1) / LAT_T) * LAT_T;
}

extern "C" int sla_hip_launch_lattice_raw(const int32_t* d_samples, uint64_t plane_stride, uint32_t order,
                                          const sla_hip_lattice_chunk* d_chunks, uint32_t num_chunks,
                                          const int32_t* d_kint, int32_t* d_residual, sla_hip_stream_t stream)
{
  if (d_samples == nullptr || d_chunks == nullptr || d_kint == nullptr || d_residual == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (order < 1 || order > 255 || (order + LAT_T - 1) / LAT_T >= 32) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_chunks == 0) { return 0; }
  hipLaunchKernelGGL(k_lattice, dim3((num_chunks + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_samples, plane_stride,
                     0u, order, d_chunks, num_chunks, d_kint, d_residual, (unsigned long long*)nullptr, 1u | (tuning().lattice_plain ? 2u : 0u));
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_lpc_f64(const double* d_samples, uint32_t order,
                                      const sla_hip_lpc_group* d_groups, uint32_t num_groups, uint32_t max_window,
                                      uint32_t max_cands_per_group, const sla_hip_lpc_cand* d_cands,
                                      double* d_out, sla_hip_stream_t stream)
{
  return launch_lpc_impl(reinterpret_cast<const int32_t*>(d_samples), 0, 0, order, d_groups, num_groups, max_window, max_cands_per_group,
                         d_cands, nullptr, d_out, nullptr, nullptr, nullptr, stream, 512u, nullptr, nullptr);
}

extern "C" int sla_hip_launch_emphasis_i32(const int32_t* d_in, int32_t* d_out, uint32_t num_samples, int32_t previous,
                                           uint32_t coef_shift, sla_hip_stream_t stream)
{
  if (d_in == nullptr || d_out == nullptr || coef_shift == 0 || coef_shift > 30) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_samples == 0) { return 0; }
  hipLaunchKernelGGL(k_emphasis_i32, dim3((num_samples + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_in, d_out, num_samples, previous, coef_shift);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_emphasis_f64(const double* d_in, double* d_out, uint32_t num_samples, uint32_t coef_shift,
                                           sla_hip_stream_t stream)
{
  if (d_in == nullptr || d_out == nullptr || coef_shift == 0 || coef_shift > 30) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_samples == 0) { return 0; }
  hipLaunchKernelGGL(k_emphasis_f64, dim3((num_samples + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_in, d_out, num_samples, coef_shift);
  return hip_rc(hipGetLastError());
}

static int launch_tail_impl(const int32_t* d_res_in, int32_t* d_res_out, uint64_t plane_stride,
                            const sla_hip_tail_job* d_jobs, uint32_t num_jobs, uint32_t longterm_order,
                            uint32_t lms_order, uint64_t* d_fold_sum, sla_hip_stream_t stream, uint32_t stage_flags,
                            unsigned long long* span = nullptr, uint32_t* d_rice_init = nullptr);

extern "C" int sla_hip_launch_tail_x(const int32_t* d_res_in, int32_t* d_res_out, uint64_t plane_stride,
                                     const sla_hip_tail_job* d_jobs, uint32_t num_jobs, uint32_t longterm_order,
                                     uint32_t lms_order, uint64_t* d_fold_sum, sla_hip_stream_t stream, const sla_hip_launch_extra* extra)
{
  return launch_tail_impl(d_res_in, d_res_out, plane_stride, d_jobs, num_jobs, longterm_order, lms_order, d_fold_sum, stream, 0u, span_of(extra),
                          (extra != nullptr) ? extra->d_rice_init : nullptr);
}

extern "C" int sla_hip_launch_tail(const int32_t* d_res_in, int32_t* d_res_out, uint64_t plane_stride,
                                   const sla_hip_tail_job* d_jobs, uint32_t num_jobs, uint32_t longterm_order,
                                   uint32_t lms_order, uint64_t* d_fold_sum, sla_hip_stream_t stream)
{
  return launch_tail_impl(d_res_in, d_res_out, plane_stride, d_jobs, num_jobs, longterm_order, lms_order, d_fold_sum, stream, 0u);
}

extern "C" int sla_hip_launch_tail_stages(const int32_t* d_res_in, int32_t* d_res_out, uint64_t plane_stride,
                                          const sla_hip_tail_job* d_jobs, uint32_t num_jobs, uint32_t longterm_order,
                                          uint32_t lms_order, uint32_t skip_lms, uint64_t* d_fold_sum, sla_hip_stream_t stream)
{
  return launch_tail_impl(d_res_in, d_res_out, plane_stride, d_jobs, num_jobs, longterm_order, lms_order, d_fold_sum, stream,
                          skip_lms ? 1u : 0u);
}

/* one-tap-per-lane waves of k_tailk beyond which two taps per lane are chosen (1024 SIMDs) */
#define TAILK2_WAVES 2048u
static int launch_tail_impl(const int32_t* d_res_in, int32_t* d_res_out, uint64_t plane_stride,
                            const sla_hip_tail_job* d_jobs, uint32_t num_jobs, uint32_t longterm_order,
                            uint32_t lms_order, uint64_t* d_fold_sum, sla_hip_stream_t stream, uint32_t stage_flags,
                            unsigned long long* span, uint32_t* d_rice_init)
{
  if (d_res_in == nullptr || d_res_out == nullptr || d_jobs == nullptr || d_fold_sum == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (longterm_order > 5 || !(longterm_order & 1)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (!(lms_order == 4 || lms_order == 8 || lms_order == 16 || lms_order == 32)) { return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY; }
  if (num_jobs == 0) { return 0; }
  const uint32_t tw = tuning().tail_waves;
  hipStream_t st = (hipStream_t)stream;
  /* K taps of each history per lane (k_tailk).  Measured (tests/tools/chunk_sweep.py, LMS order 8, ms per launch; k_tail /
   * k_tail2 = the 2 * order- and order-lanes-per-job kernels of rounds 1 - 2, deleted in round 4):
   *   jobs     blocks          k_tail  k_tail2   K = 1   K = 2   K = 4
   *    3.5 k   4096 (C2 300 s)   0.42    0.49     0.35    0.43    0.62
   *    7 k     4096 (C2)         0.44    0.57     0.37    0.43    0.62
   *   14 k     4096 (C3 600 s)   0.99    0.78     0.50    0.49    0.68
   *   11 k     8192 (C5 120 s)   1.26    1.46     0.96    0.95    1.33
   *   90 k     4096 (C3)         4.33    3.60     1.95    1.46    1.55
   *  169 k     8192 (C5)        16.5    13.2      7.45    5.45    6.70
   * One tap per lane has the shortest chain per sample (0.35 ms per 4096 samples) and holds up to about two waves per SIMD;
   * beyond that two taps per lane halve the work per job.  Four never won: its 16-sample runs per lane cost more in the
   * long-term stage and registers than the shared per-sample work saves.  (One LANE per job -- histories in registers,
   * tiles transposed through LDS, round 3 -- lost to all of them: 16 half-rate 32-bit products per sample in one lane's
   * chain.) */
  uint32_t k = tuning().tail_taps;                                     /* 0 = by the number of jobs */
  const uint32_t k1_waves = (num_jobs * lms_order + 63u) / 64u;        /* waves of K = 1 */
  if (k != 1 && k != 2 && k != 4) { k = (lms_order > 16 || (k1_waves > TAILK2_WAVES && lms_order >= 4)) ? 2u : 1u; }
  if (k == 1 && lms_order > 16) { k = 2; }                /* at most sixteen lanes per job */
  if (k > lms_order / 2) { k = lms_order / 2; }          /* at least two */
  {
    /* four waves per workgroup: one workgroup fills a CU's four SIMDs with one wave each (one-wave workgroups landed two
     * on a SIMD while other CUs stood empty: C2 0.44 against 0.37 ms, C3 1.83 against 1.46) */
    const uint32_t twk = (tw >= 1 && tw <= 4) ? tw : 4u;
    const uint32_t jpw = 64 / (lms_order / k);
    const uint32_t jpb = twk * jpw;
    dim3 gridk((num_jobs + jpb - 1) / jpb), blockk(64 * twk);
#define LAUNCH_TAILK(O, KK) hipLaunchKernelGGL((k_tailk<O, KK>), gridk, blockk, 0, st, d_res_in, d_res_out, plane_stride, d_jobs, num_jobs, longterm_order, d_fold_sum, span, stage_flags, d_rice_init)
    switch (lms_order * 16 + k) {
      case 4 * 16 + 1:  LAUNCH_TAILK(4, 1); break;
      case 8 * 16 + 1:  LAUNCH_TAILK(8, 1); break;
      case 16 * 16 + 1: LAUNCH_TAILK(16, 1); break;
      case 4 * 16 + 2:  LAUNCH_TAILK(4, 2); break;
      case 8 * 16 + 2:  LAUNCH_TAILK(8, 2); break;
      case 8 * 16 + 4:  LAUNCH_TAILK(8, 4); break;
      case 16 * 16 + 2: LAUNCH_TAILK(16, 2); break;
      case 16 * 16 + 4: LAUNCH_TAILK(16, 4); break;
      case 32 * 16 + 2: LAUNCH_TAILK(32, 2); break;
      case 32 * 16 + 4: LAUNCH_TAILK(32, 4); break;
      default: return SLA_APIRESULT_EXCEED_HANDLE_CAPACITY;
    }
#undef LAUNCH_TAILK
  }
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_ltm_acf_x(const int32_t* d_residual, uint64_t plane_stride,
                                      const sla_hip_acf_job* d_jobs, uint32_t num_jobs, uint32_t fft_size,
                                      const double* d_twiddles, double* d_scratch, uint32_t scratch_slots,
                                      double* d_acf_head, uint32_t head, sla_hip_stream_t stream, const sla_hip_launch_extra* extra)
{
  if (d_residual == nullptr || d_jobs == nullptr || d_twiddles == nullptr || d_acf_head == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (fft_size < 1024 || fft_size > 65536 * 2 || (fft_size & (fft_size - 1)) || head == 0 || head > fft_size) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_jobs == 0) { return 0; }
  uint32_t log2F = 0;
  while ((1u << log2F) < fft_size) { log2F++; }
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = sizeof(double) * (size_t)fft_size;
  unsigned long long* span = span_of(extra);
  if (lds <= SLA_HIP_LDS_BUDGET && log2F >= 12 && log2F <= 14) {
    // the capacities the encoder is created with (2048 .. 8192 samples per block): fewer LDS passes, same bits
    hipError_t e = hipSuccess;
#define SLA_ACF2(LL, TT, REC) do { \
      e = ensure_dynamic_lds((const void*)k_ltm_acf2<LL, TT, REC>, lds); \
      if (e != hipSuccess) { return hip_rc(e); } \
      hipLaunchKernelGGL((k_ltm_acf2<LL, TT, REC>), dim3(num_jobs), dim3(TT), lds, st, d_residual, plane_stride, d_jobs, num_jobs, d_twiddles, d_acf_head, head, span); } while (0)
    const bool rec = (head == SLA_HIP_ACF_RECORD);
    // 64 KiB of LDS or less: 512 threads, two workgroups per CU; a 16384-point job owns the CU's LDS: 1024 threads (measured
    // on 11250 such jobs: 0.91 ms against 1.10 ms with 512 threads; k_ltm_acf: 1.85 ms) -- four waves per SIMD either way
    if (log2F == 12) { if (rec) { SLA_ACF2(11, 512, true); } else { SLA_ACF2(11, 512, false); } }
    else if (log2F == 13) { if (rec) { SLA_ACF2(12, 512, true); } else { SLA_ACF2(12, 512, false); } }
    else { if (rec) { SLA_ACF2(13, 1024, true); } else { SLA_ACF2(13, 1024, false); } }
#undef SLA_ACF2
  } else if (lds <= SLA_HIP_LDS_BUDGET) {
    hipError_t e = ensure_dynamic_lds((const void*)k_ltm_acf<true>, lds);
    if (e != hipSuccess) { return hip_rc(e); }
    hipLaunchKernelGGL(k_ltm_acf<true>, dim3(num_jobs), dim3(ACF_THREADS), lds, st, d_residual, plane_stride, d_jobs, num_jobs,
                       log2F, d_twiddles, (double*)nullptr, d_acf_head, head, span, (const uint32_t*)nullptr, (const uint32_t*)nullptr);
  } else {
    if (d_scratch == nullptr || scratch_slots == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
    uint32_t grid = (num_jobs < scratch_slots) ? num_jobs : scratch_slots;
    hipLaunchKernelGGL(k_ltm_acf<false>, dim3(grid), dim3(ACF_THREADS), 0, st, d_residual, plane_stride, d_jobs, num_jobs,
                       log2F, d_twiddles, d_scratch, d_acf_head, head, span, (const uint32_t*)nullptr, (const uint32_t*)nullptr);
  }
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_ltm_acf(const int32_t* d_residual, uint64_t plane_stride,
                                      const sla_hip_acf_job* d_jobs, uint32_t num_jobs, uint32_t fft_size,
                                      const double* d_twiddles, double* d_scratch, uint32_t scratch_slots,
                                      double* d_acf_head, uint32_t head, sla_hip_stream_t stream)
{
  return sla_hip_launch_ltm_acf_x(d_residual, plane_stride, d_jobs, num_jobs, fft_size, d_twiddles, d_scratch, scratch_slots, d_acf_head, head, stream, nullptr);
}

extern "C" int sla_hip_launch_ltm_solve(const double* d_acf_records, const sla_hip_lpc_group* d_groups, uint32_t num_jobs,
                                        uint32_t longterm_order, sla_hip_tail_job* d_jobs, sla_hip_stream_t stream)
{
  if (d_acf_records == nullptr || d_groups == nullptr || d_jobs == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (longterm_order == 0 || longterm_order > LTM_NT || (longterm_order & 1u) == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_jobs == 0) { return 0; }
  const dim3 grid((num_jobs + 63) / 64), block(64);
  if (longterm_order == 1) { hipLaunchKernelGGL(k_ltm_solve<1>, grid, block, 0, (hipStream_t)stream, d_acf_records, d_groups, num_jobs, d_jobs); }
  else if (longterm_order == 3) { hipLaunchKernelGGL(k_ltm_solve<3>, grid, block, 0, (hipStream_t)stream, d_acf_records, d_groups, num_jobs, d_jobs); }
  else { hipLaunchKernelGGL(k_ltm_solve<5>, grid, block, 0, (hipStream_t)stream, d_acf_records, d_groups, num_jobs, d_jobs); }
  return hip_rc(hipGetLastError());
}

// The certified long-term stage (k_ltm_acf_int or k_ltm_acf_fast -> k_ltm_solve_cert -> exact kernels over the fallback list), all on one
// stream.  The list kernels run on a fixed small grid and read the list's length on the device: an empty list costs two
// near-empty launches.  d_counters (4 words, zero before the call): list entries, uncertified jobs, audit ok, audit bad.
#define LIST_LTM_GRID 64u
extern "C" int sla_hip_ltm_cert_supported(uint32_t fft_size)
{
  return (fft_size == 4096 || fft_size == 8192 || fft_size == 16384 || fft_size == 32768) ? 1 : 0;
}

extern "C" int sla_hip_launch_ltm_acf_int(const int32_t* d_residual, uint64_t plane_stride, const sla_hip_acf_job* d_acf_jobs,
                                          uint32_t num_jobs, uint32_t fft_size, double* d_out, sla_hip_stream_t stream)
{
  if (d_residual == nullptr || d_acf_jobs == nullptr || d_out == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (!sla_hip_ltm_cert_supported(fft_size)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_jobs == 0) { return 0; }
  uint32_t log2F = 0;
  while ((1u << log2F) < fft_size) { log2F++; }
  const size_t lds = ACF_INT_LDS(fft_size / 2u);
  const hipError_t e = ensure_dynamic_lds((const void*)k_ltm_acf_int<true>, lds);
  if (e != hipSuccess) { return hip_rc(e); }
  hipLaunchKernelGGL((k_ltm_acf_int<true>), dim3(num_jobs), dim3(ACF_INT_THREADS), lds, (hipStream_t)stream, d_residual, plane_stride, d_acf_jobs,
                     num_jobs, log2F, d_out, (double*)nullptr, 0.0, (unsigned long long*)nullptr);
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_ltm_cert_x(const int32_t* d_residual, uint64_t plane_stride, const sla_hip_acf_job* d_acf_jobs,
                                       const sla_hip_lpc_group* d_groups, uint32_t num_jobs, uint32_t fft_size,
                                       const double* d_twiddles, const double* d_fast_twiddles, double* d_scratch, uint32_t scratch_slots,
                                       double* d_acf_records, double* d_eps, uint32_t longterm_order, double safety,
                                       sla_hip_tail_job* d_jobs, uint32_t* d_list, uint32_t* d_counters,
                                       sla_hip_stream_t stream, const sla_hip_launch_extra* extra)
{
  if (d_residual == nullptr || d_acf_jobs == nullptr || d_groups == nullptr || d_twiddles == nullptr || d_fast_twiddles == nullptr
      || d_acf_records == nullptr || d_eps == nullptr || d_jobs == nullptr || d_list == nullptr || d_counters == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (!sla_hip_ltm_cert_supported(fft_size)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (longterm_order == 0 || longterm_order > LTM_NT || (longterm_order & 1u) == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (!(safety >= SLA_HIP_LTM_CERT_SAFETY_MIN)) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_jobs == 0) { return 0; }
  uint32_t log2F = 0;
  while ((1u << log2F) < fft_size) { log2F++; }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* span = span_of(extra);
  const double eps_rel = sla_hip_ltm_cert_eps_rel(fft_size, safety);
  const uint32_t audit_every = tuning().cert_audit;
  hipError_t e = hipSuccess;
  // the transform is at most half the reference's: 16 bytes * 2^(log2F - 2) of LDS
#define SLA_ACFF(LTOP, TT) do { \
    const size_t lds = sizeof(double2) * ((size_t)1 << (LTOP)); \
    e = ensure_dynamic_lds((const void*)k_ltm_acf_fast<LTOP, TT>, lds); \
    if (e != hipSuccess) { return hip_rc(e); } \
    hipLaunchKernelGGL((k_ltm_acf_fast<LTOP, TT>), dim3(num_jobs), dim3(TT), lds, st, d_residual, plane_stride, d_acf_jobs, num_jobs, d_fast_twiddles, d_acf_records, d_eps, eps_rel, span); } while (0)
  if (tuning().ltm_int) {
    // the same record from exact integer sums on the int8 matrix pipe (k_ltm_acf_int): digit planes of a whole block in LDS
    const size_t lds = ACF_INT_LDS(fft_size / 2u);
    e = ensure_dynamic_lds((const void*)k_ltm_acf_int<false>, lds);
    if (e != hipSuccess) { return hip_rc(e); }
    hipLaunchKernelGGL((k_ltm_acf_int<false>), dim3(num_jobs), dim3(ACF_INT_THREADS), lds, st, d_residual, plane_stride, d_acf_jobs, num_jobs, log2F, d_acf_records, d_eps, eps_rel, span);
  }
  else if (log2F == 12) { SLA_ACFF(10, 128); }
  else if (log2F == 13) { SLA_ACFF(11, 256); }
  else if (log2F == 14) { SLA_ACFF(12, 512); }
  else { SLA_ACFF(13, 1024); }
#undef SLA_ACFF
  const dim3 grid((num_jobs + 63) / 64), block(64);
#define SLA_SOLVEC(D) hipLaunchKernelGGL(k_ltm_solve_cert<D>, grid, block, 0, st, d_acf_records, d_eps, d_groups, num_jobs, d_jobs, d_list, d_counters, audit_every)
  if (longterm_order == 1) { SLA_SOLVEC(1); } else if (longterm_order == 3) { SLA_SOLVEC(3); } else { SLA_SOLVEC(5); }
#undef SLA_SOLVEC
  // the exact route over whatever was not certified (and over the audited jobs)
  const size_t lds = sizeof(double) * (size_t)fft_size;
  if (lds <= SLA_HIP_LDS_BUDGET) {
#define SLA_ACF2L(LL, TT) do { \
      e = ensure_dynamic_lds((const void*)k_ltm_acf2_list<LL, TT>, lds); \
      if (e != hipSuccess) { return hip_rc(e); } \
      hipLaunchKernelGGL((k_ltm_acf2_list<LL, TT>), dim3(LIST_LTM_GRID), dim3(TT), lds, st, d_residual, plane_stride, d_acf_jobs, d_list, d_counters, d_twiddles, d_acf_records, span); } while (0)
    if (log2F == 12) { SLA_ACF2L(11, 512); } else if (log2F == 13) { SLA_ACF2L(12, 512); } else { SLA_ACF2L(13, 1024); }
#undef SLA_ACF2L
  } else {
    if (d_scratch == nullptr || scratch_slots == 0) { return SLA_APIRESULT_INVALID_ARGUMENT; }
    const uint32_t grid_l = (LIST_LTM_GRID < scratch_slots) ? LIST_LTM_GRID : scratch_slots;
    hipLaunchKernelGGL(k_ltm_acf<false>, dim3(grid_l), dim3(ACF_THREADS), 0, st, d_residual, plane_stride, d_acf_jobs, 0u,
                       log2F, d_twiddles, d_scratch, d_acf_records, SLA_HIP_ACF_RECORD, span, (const uint32_t*)d_list, (const uint32_t*)d_counters);
  }
  const dim3 grid_s(LIST_LTM_GRID);
#define SLA_SOLVEL(D) hipLaunchKernelGGL(k_ltm_solve_list<D>, grid_s, block, 0, st, d_acf_records, d_groups, d_list, d_counters, d_jobs)
  if (longterm_order == 1) { SLA_SOLVEL(1); } else if (longterm_order == 3) { SLA_SOLVEL(3); } else { SLA_SOLVEL(5); }
#undef SLA_SOLVEL
  return hip_rc(hipGetLastError());
}

extern "C" int sla_hip_launch_enc_emit_batch(const sla_hip_enc_emit* d_table, uint32_t num_entries, uint32_t max_bytes,
                                             const uint8_t* d_image, uint64_t image_bytes, sla_hip_stream_t stream)
{
  if (d_table == nullptr || d_image == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_entries == 0 || max_bytes == 0) { return 0; }
  // a workgroup row covers 4096 bytes of a file (256 lanes x 16); longer files grid-stride
  uint64_t gx = ((uint64_t)max_bytes + 15 + 4095) / 4096;
  if (gx > 1024) { gx = 1024; }
  const dim3 grid((uint32_t)gx, (num_entries < 65535u) ? num_entries : 65535u), block(256);
  hipLaunchKernelGGL(k_enc_emit, grid, block, 0, (hipStream_t)stream, d_table, num_entries, d_image, image_bytes);
  return hip_rc(hipGetLastError());
}
