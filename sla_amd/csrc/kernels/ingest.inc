// kernels/ingest.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): k_enc_ingest_batch, its launcher
// ---------------------------------------------------------------------------------------------
// k_enc_ingest_batch: the upload leg of sla_hip_encode_batch_device.  Every file's region of the caller's device memory is
// read once, converted to the left-justified int32 words of the handle's planes (the table of
// sla_hip_launch_enc_ingest_batch, include/sla_hip.h) and stored at the file's tile-aligned start; [num_samples, fill_end)
// of every plane is written zero in the same pass (the prepass tiles and the super-frame hop read that gap).  The mirror of
// k_dec_emit_batch: blockIdx.y walks the files, the x dimension their samples, three load shapes chosen per file
// (wave-uniform):
//   planar (sample_stride 1)                       a lane takes 4 consecutive samples of each channel: one 16-byte load
//                                                  (int16: 8-byte) and one 16-byte plane store per channel;
//   interleaved stereo (channel_stride 1, ss 2)    a lane takes 4 frames: one 16-byte load (int32 / float: two) and two
//                                                  16-byte plane stores;
//   any other strides                              one element at a time.
// A source that is not aligned to the load's width is read element by element by the same lane.  Refusals only the
// samples can show (SLA_HIP_PCM_S32 out of range: bit 0, SLA_HIP_PCM_F32 NaN: bit 1) are ORed within the wave, and the
// first lane that holds a flag ORs the wave's bits into the file's error word.
// ---------------------------------------------------------------------------------------------
template <uint32_t FMT> struct ingest_type { typedef int32_t T; };
template <> struct ingest_type<SLA_HIP_PCM_S16> { typedef int16_t T; };
template <> struct ingest_type<SLA_HIP_PCM_F32> { typedef float T; };

#define INGEST_ERR_RANGE 1u
#define INGEST_ERR_NAN   2u

// element -> left-justified word of a bps-bit file (the table of sla_hip_encode_batch_device in include/sla_hip.h)
template <uint32_t FMT>
__device__ __forceinline__ int32_t ingest_cvt(typename ingest_type<FMT>::T v, uint32_t bps, uint32_t& err)
{
  if constexpr (FMT == SLA_HIP_PCM_S32) {
    const int64_t hi = (bps != 0) ? ((int64_t)1 << (bps - 1)) - 1 : 0, lo = (bps != 0) ? -hi - 1 : 0;
    if ((int64_t)v < lo || (int64_t)v > hi) { err |= INGEST_ERR_RANGE; return 0; }
    return (bps != 0) ? (int32_t)((uint32_t)v << (32u - bps)) : 0;
  } else if constexpr (FMT == SLA_HIP_PCM_S16) {
    return (int32_t)((uint32_t)(int32_t)v << 16);
  } else if constexpr (FMT == SLA_HIP_PCM_F32) {
    if (v != v) { err |= INGEST_ERR_NAN; return 0; }
    if (bps == 0) { return 0; }
    // v * 2^(bps-1) is exact (a power-of-two scale; what overflows becomes +-inf and saturates); rintf rounds ties to even
    const float top = (float)((int64_t)1 << (bps - 1));
    const float q = rintf(v * top);
    int32_t r;
    if (q >= top) { r = (int32_t)(((int64_t)1 << (bps - 1)) - 1); }
    else if (q <= -top) { r = (int32_t)(-((int64_t)1 << (bps - 1))); }
    else { r = (int32_t)q; }
    return (int32_t)((uint32_t)r << (32u - bps));
  } else {
    return v;
  }
}

// 4 consecutive elements from g, those at or past n read as zero; vload: p + g is aligned to the 4-element width
template <typename T>
__device__ __forceinline__ void ingest_load4(const T* p, uint64_t g, uint64_t n, bool vload, T v[4])
{
  typedef T t4 __attribute__((ext_vector_type(4)));
  if (vload && g + 4 <= n) {
    const t4 q = *(const t4*)(p + g);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = (g + k < n) ? p[g + k] : (T)0; }
  }
}

// 4 plane words at g (those at or past lim are not stored): one 16-byte store when the plane position is aligned
__device__ __forceinline__ void ingest_store4(int32_t* p, uint64_t g, uint64_t lim, bool vstore, const int32_t w[4])
{
  typedef int32_t i4 __attribute__((ext_vector_type(4)));
  if (vstore && g + 4 <= lim) {
    i4 q; q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = w[3];
    *(i4*)(p + g) = q;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) { if (g + k < lim) { p[g + k] = w[k]; } }
  }
}

template <uint32_t FMT>
__global__ __launch_bounds__(256)
void k_enc_ingest_batch(const sla_hip_enc_ingest* __restrict__ files, uint32_t num_files, uint32_t C,
                        int32_t* __restrict__ planes, uint64_t stride, uint32_t* __restrict__ error)
{
  typedef typename ingest_type<FMT>::T T;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (uint64_t)gridDim.x * blockDim.x;
  for (uint32_t f = blockIdx.y; f < num_files; f += gridDim.y) {
    const sla_hip_enc_ingest e = files[f];
    const T* src = (const T*)e.src;
    int32_t* dst = planes + e.plane_off;
    const uint64_t n = e.num_samples, lim = (e.fill_end > e.num_samples) ? e.fill_end : e.num_samples;
    const uint64_t cs = e.channel_stride, ss = e.sample_stride;
    const uint32_t bps = e.bits_per_sample;
    const bool vstore = ((e.plane_off | stride) & 3u) == 0 && ((uintptr_t)planes % 16) == 0;
    uint32_t err = 0;
    if (ss == 1) {
      const bool vload = ((uintptr_t)src % (4 * sizeof(T))) == 0 && (C == 1 || cs % 4 == 0);
      for (uint64_t g = tid * 4; g < lim; g += nt * 4) {
        for (uint32_t c = 0; c < C; c++) {
          T v[4];
          int32_t w[4];
          ingest_load4(src + (uint64_t)c * cs, g, n, vload, v);
#pragma unroll
          for (int k = 0; k < 4; k++) { w[k] = (g + k < n) ? ingest_cvt<FMT>(v[k], bps, err) : 0; }
          ingest_store4(dst + (uint64_t)c * stride, g, lim, vstore, w);
        }
      }
    } else if (C == 2 && cs == 1 && ss == 2) {
      const bool vload = ((uintptr_t)src % 16) == 0;
      for (uint64_t g = tid * 4; g < lim; g += nt * 4) {
        T v[8];
        int32_t a[4], b[4];
        if (vload && g + 4 <= n) {
          if constexpr (sizeof(T) == 2) {
            typedef T t8 __attribute__((ext_vector_type(8)));
            const t8 q = *(const t8*)(src + 2 * g);
#pragma unroll
            for (int k = 0; k < 8; k++) { v[k] = q[k]; }
          } else {
            typedef T t4 __attribute__((ext_vector_type(4)));
            const t4 q0 = *(const t4*)(src + 2 * g), q1 = *(const t4*)(src + 2 * g + 4);
            v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
          }
        } else {
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const bool in = g + k < n;
            v[2 * k] = in ? src[2 * (g + k)] : (T)0;
            v[2 * k + 1] = in ? src[2 * (g + k) + 1] : (T)0;
          }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const bool in = g + k < n;
          a[k] = in ? ingest_cvt<FMT>(v[2 * k], bps, err) : 0;
          b[k] = in ? ingest_cvt<FMT>(v[2 * k + 1], bps, err) : 0;
        }
        ingest_store4(dst, g, lim, vstore, a);
        ingest_store4(dst + stride, g, lim, vstore, b);
      }
    } else {
      for (uint64_t i = tid; i < lim; i += nt) {
        for (uint32_t c = 0; c < C; c++) {
          dst[(uint64_t)c * stride + i] = (i < n) ? ingest_cvt<FMT>(src[(uint64_t)c * cs + i * ss], bps, err) : 0;
        }
      }
    }
    if constexpr (FMT == SLA_HIP_PCM_S32 || FMT == SLA_HIP_PCM_F32) {
      // the wave's flags first, then one atomic from the first lane that holds one
      const uint64_t any = __ballot(err != 0);
      if (any != 0) {
        const uint32_t wave_err = ((__ballot((err & INGEST_ERR_RANGE) != 0) != 0) ? INGEST_ERR_RANGE : 0u)
                                | ((__ballot((err & INGEST_ERR_NAN) != 0) != 0) ? INGEST_ERR_NAN : 0u);
        if ((threadIdx.x & 63) == (uint32_t)__builtin_ctzll(any)) { atomicOr(&error[f], wave_err); }
      }
    }
  }
}

extern "C" int sla_hip_launch_enc_ingest_batch(const sla_hip_enc_ingest* d_files, uint32_t num_files, uint32_t max_samples,
                                               uint32_t num_channels, uint32_t sample_format, int32_t* d_planes,
                                               uint64_t plane_stride, uint32_t* d_error, sla_hip_stream_t stream)
{
  if (d_files == nullptr || d_planes == nullptr || d_error == nullptr || sample_format > SLA_HIP_PCM_F32) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_files == 0 || max_samples == 0) { return 0; }
  // a workgroup row covers 1024 samples of a planar file (256 lanes x 4); longer files and the other shapes grid-stride
  uint32_t gx = (max_samples + 1023) / 1024;
  if (gx > 1024) { gx = 1024; }
  const dim3 grid(gx, (num_files < 65535u) ? num_files : 65535u), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (sample_format) {
    case SLA_HIP_PCM_S32_LEFT: hipLaunchKernelGGL(k_enc_ingest_batch<SLA_HIP_PCM_S32_LEFT>, grid, block, 0, st, d_files, num_files, num_channels, d_planes, plane_stride, d_error); break;
    case SLA_HIP_PCM_S32:      hipLaunchKernelGGL(k_enc_ingest_batch<SLA_HIP_PCM_S32>, grid, block, 0, st, d_files, num_files, num_channels, d_planes, plane_stride, d_error); break;
    case SLA_HIP_PCM_S16:      hipLaunchKernelGGL(k_enc_ingest_batch<SLA_HIP_PCM_S16>, grid, block, 0, st, d_files, num_files, num_channels, d_planes, plane_stride, d_error); break;
    default:                   hipLaunchKernelGGL(k_enc_ingest_batch<SLA_HIP_PCM_F32>, grid, block, 0, st, d_files, num_files, num_channels, d_planes, plane_stride, d_error); break;
  }
  return hip_rc(hipGetLastError());
}
