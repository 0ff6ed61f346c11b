// kernels/wav.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): k_wav_ingest, k_wav_ingest_any,
// k_wav_emit and their launchers
// ---------------------------------------------------------------------------------------------
// The byte work of the WAV layer (sla_wav.c reads and writes the headers; the data chunk is handled here).  A WAV data chunk
// is frames of C samples of B = 1 .. 4 little-endian bytes, at ANY byte address.  With L the left-justified plane word:
//     B = 1 (unsigned)  L = (u - 128) << 24      u = (L >> 24) + 128
//     B = 2             L = s << 16              s = L >> 16
//     B = 3             L = s << 8               s = L >> 8
//     B = 4             L = s                    s = L
//
// k_wav_ingest<C, B> (C = 1, 2): the mirror of k_enc_ingest_batch for packed frames.  blockIdx.y walks the files, the x
// dimension runs of 4 frames: a lane reads the 2 or 3 ALIGNED 16-byte words that hold its 4 * C * B bytes (only those that
// overlap the file's bytes: a data chunk may end at the last byte of an allocation), selects words by the source's word
// misalignment, realigns with v_alignbyte_b32 by its byte misalignment, cuts the samples out at compile-time positions and
// stores one 16-byte plane word group per channel.  [num_samples, fill_end) of every plane is written zero on the way.
// k_wav_ingest_any: every other channel count, one frame per lane, byte loads inside the file's bytes.
//
// k_wav_emit<C, B>: the mirror of k_enc_emit for WAV files.  Entry k writes exactly [dst, dst + header_bytes + n * C * B): the
// header bytes of the table, then the frames -- mid/side undone and left-justified as k_dec_emit_batch does it, converted as
// above.  blockIdx.y walks the table, the x dimension the aligned 16-byte chunks of the destination: a chunk wholly behind
// the header and inside the file is put together in registers from the 5 .. 16 samples that overlap it and goes out in one
// 16-byte store; the head (with the header) and the tail go out as guarded byte stores, because files packed back to back
// share 4- and 16-byte words with neighbours that other lanes write in the same launch.
// ---------------------------------------------------------------------------------------------
typedef uint32_t wav_u4 __attribute__((ext_vector_type(4)));

// the low B bytes of v (little-endian sample; the bits above them are ignored) -> left-justified word
template <uint32_t B>
__device__ __forceinline__ int32_t wav_to_left(uint32_t v)
{
  if constexpr (B == 1) { return (int32_t)(((v & 0xFFu) ^ 0x80u) << 24); }
  else if constexpr (B == 2) { return (int32_t)(v << 16); }
  else if constexpr (B == 3) { return (int32_t)(v << 8); }
  else { return (int32_t)v; }
}

// left-justified word -> the sample's B bytes in the low bits, zeros above
template <uint32_t B>
__device__ __forceinline__ uint32_t wav_from_left(int32_t left)
{
  if constexpr (B == 1) { return ((uint32_t)left >> 24) ^ 0x80u; }
  else if constexpr (B == 2) { return (uint32_t)left >> 16; }
  else if constexpr (B == 3) { return (uint32_t)left >> 8; }
  else { return (uint32_t)left; }
}

template <uint32_t C, uint32_t B>
__global__ __launch_bounds__(256)
void k_wav_ingest(const sla_hip_wav_ingest* __restrict__ files, uint32_t num_files, int32_t* __restrict__ planes, uint64_t stride)
{
  constexpr uint32_t F = C * B;                       // bytes of a frame = 32-bit words of 4 frames
  constexpr uint32_t NW = (4 * F + 15 + 15) / 16;     // aligned 16-byte words that 4 frames at any misalignment can touch
  static_assert(NW * 4 >= F + 4, "word select runs off the loaded words");
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (uint64_t)gridDim.x * blockDim.x;
  for (uint32_t f = blockIdx.y; f < num_files; f += gridDim.y) {
    const sla_hip_wav_ingest e = files[f];
    int32_t* dst = planes + e.plane_off;
    const uint64_t n = e.num_samples, lim = (e.fill_end > e.num_samples) ? e.fill_end : e.num_samples;
    const bool vstore = ((e.plane_off | stride) & 3u) == 0 && ((uintptr_t)planes % 16) == 0;
    for (uint64_t g = tid * 4; g < lim; g += nt * 4) {
      int32_t out[C][4];
#pragma unroll
      for (uint32_t c = 0; c < C; c++) { out[c][0] = 0; out[c][1] = 0; out[c][2] = 0; out[c][3] = 0; }
      if (g < n) {
        const uint32_t cnt = (n - g < 4) ? (uint32_t)(n - g) : 4u;
        const uintptr_t s = (uintptr_t)e.src + g * F, end = s + (uintptr_t)cnt * F;
        const uintptr_t base = s & ~(uintptr_t)15;
        const uint32_t r = (uint32_t)(s & 15u);
        uint32_t q[NW * 4], w[F + 1], a[F + 1];
#pragma unroll
        for (uint32_t k = 0; k < NW; k++) {
          wav_u4 v = {0u, 0u, 0u, 0u};
          if (base + 16u * k < end) { v = ((const wav_u4*)base)[k]; }      // (holds at least one of the lane's bytes)
          q[4 * k] = v.x; q[4 * k + 1] = v.y; q[4 * k + 2] = v.z; q[4 * k + 3] = v.w;
        }
        switch (r >> 2) {
          case 0:
#pragma unroll
            for (uint32_t k = 0; k <= F; k++) { w[k] = q[k]; }
            break;
          case 1:
#pragma unroll
            for (uint32_t k = 0; k <= F; k++) { w[k] = q[k + 1]; }
            break;
          case 2:
#pragma unroll
            for (uint32_t k = 0; k <= F; k++) { w[k] = q[k + 2]; }
            break;
          default:
#pragma unroll
            for (uint32_t k = 0; k <= F; k++) { w[k] = q[k + 3]; }
            break;
        }
#pragma unroll
        for (uint32_t k = 0; k < F; k++) { a[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], r & 3u); }
        a[F] = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4 * C; j++) {
          const uint32_t d = (j * B) / 4, sh = (j * B) % 4;
          const uint32_t v = (sh == 0) ? a[d] : (sh + B <= 4) ? (a[d] >> (8 * sh)) : __builtin_amdgcn_alignbyte(a[d + 1], a[d], sh);
          out[j % C][j / C] = (j / C < cnt) ? wav_to_left<B>(v) : 0;
        }
      }
#pragma unroll
      for (uint32_t c = 0; c < C; c++) { ingest_store4(dst + (uint64_t)c * stride, g, lim, vstore, out[c]); }
    }
  }
}

__global__ __launch_bounds__(256)
void k_wav_ingest_any(const sla_hip_wav_ingest* __restrict__ files, uint32_t num_files, uint32_t C, uint32_t B,
                      int32_t* __restrict__ planes, uint64_t stride)
{
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (uint64_t)gridDim.x * blockDim.x;
  for (uint32_t f = blockIdx.y; f < num_files; f += gridDim.y) {
    const sla_hip_wav_ingest e = files[f];
    int32_t* dst = planes + e.plane_off;
    const uint64_t n = e.num_samples, lim = (e.fill_end > e.num_samples) ? e.fill_end : e.num_samples;
    for (uint64_t i = tid; i < lim; i += nt) {
      for (uint32_t c = 0; c < C; c++) {
        int32_t left = 0;
        if (i < n) {
          const uint8_t* p = e.src + (i * C + c) * B;
          uint32_t v = 0;
          for (uint32_t b = 0; b < B; b++) { v |= (uint32_t)p[b] << (8 * b); }
          left = (B == 1) ? wav_to_left<1>(v) : (B == 2) ? wav_to_left<2>(v) : (B == 3) ? wav_to_left<3>(v) : wav_to_left<4>(v);
        }
        dst[(uint64_t)c * stride + i] = left;
      }
    }
  }
}

extern "C" int sla_hip_launch_wav_ingest_batch(const sla_hip_wav_ingest* d_files, uint32_t num_files, uint32_t max_samples,
                                               uint32_t num_channels, uint32_t bytes_per_sample, int32_t* d_planes,
                                               uint64_t plane_stride, sla_hip_stream_t stream)
{
  if (d_files == nullptr || d_planes == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8 || bytes_per_sample == 0 || bytes_per_sample > 4) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_files == 0 || max_samples == 0) { return 0; }
  // a workgroup row covers 1024 frames (256 lanes x 4); longer files grid-stride
  uint32_t gx = (uint32_t)(((uint64_t)max_samples + 1023) / 1024);
  if (gx > 1024) { gx = 1024; }
  const dim3 grid(gx, (num_files < 65535u) ? num_files : 65535u), block(256);
  hipStream_t st = (hipStream_t)stream;
#define WAV_INGEST(C_, B_) hipLaunchKernelGGL((k_wav_ingest<C_, B_>), grid, block, 0, st, d_files, num_files, d_planes, plane_stride)
  switch (num_channels * 8 + bytes_per_sample) {
    case 1 * 8 + 1: WAV_INGEST(1, 1); break;
    case 1 * 8 + 2: WAV_INGEST(1, 2); break;
    case 1 * 8 + 3: WAV_INGEST(1, 3); break;
    case 1 * 8 + 4: WAV_INGEST(1, 4); break;
    case 2 * 8 + 1: WAV_INGEST(2, 1); break;
    case 2 * 8 + 2: WAV_INGEST(2, 2); break;
    case 2 * 8 + 3: WAV_INGEST(2, 3); break;
    case 2 * 8 + 4: WAV_INGEST(2, 4); break;
    default:
      hipLaunchKernelGGL(k_wav_ingest_any, grid, block, 0, st, d_files, num_files, num_channels, bytes_per_sample, d_planes, plane_stride);
      break;
  }
#undef WAV_INGEST
  return hip_rc(hipGetLastError());
}

// the B bytes of interleaved sample s (frame s / C, channel s % C) of a file, finished as k_dec_emit_batch finishes it
template <uint32_t B>
__device__ __forceinline__ uint32_t wav_emit_sample(const int32_t* __restrict__ src, uint64_t stride, uint32_t C, bool ms,
                                                    uint32_t shift, uint64_t s)
{
  const uint64_t fr = s / C;
  const uint32_t c = (uint32_t)(s % C);
  if (ms) {
    // left / right of mid / side (src/SLAUtility.c:415-433, as k_dec_finish)
    const int32_t side = src[stride + fr];
    const int32_t mid = (int32_t)(((uint32_t)src[fr] << 1) | ((uint32_t)side & 1u));
    const uint32_t lr = (c == 0) ? (uint32_t)mid + (uint32_t)side : (uint32_t)mid - (uint32_t)side;
    return wav_from_left<B>((int32_t)((uint32_t)((int32_t)lr >> 1) << shift));
  }
  return wav_from_left<B>((int32_t)((uint32_t)src[(uint64_t)c * stride + fr] << shift));
}

// CT: the channel count at compile time, 0 = C_rt
template <uint32_t CT, uint32_t B>
__global__ __launch_bounds__(256)
void k_wav_emit(const int32_t* __restrict__ planes, uint64_t stride, const sla_hip_wav_emit* __restrict__ table,
                uint32_t num_entries, uint32_t C_rt, uint32_t use_ms)
{
  constexpr uint32_t NS = (16 + B - 1 + B - 1) / B;      // samples that 16 bytes starting inside a sample can overlap
  const uint32_t C = (CT != 0) ? CT : C_rt;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (uint64_t)gridDim.x * blockDim.x;
  for (uint32_t e = blockIdx.y; e < num_entries; e += gridDim.y) {
    const sla_hip_wav_emit* g = &table[e];
    const uint32_t hb = g->header_bytes, shift = g->shift & 31u;
    uint8_t* dst = g->dst;
    if ((hb != 0 && hb != SLA_HIP_WAV_HEADER_BYTES) || dst == nullptr) { continue; }
    const int32_t* src = planes + g->plane_off;
    const bool ms = use_ms != 0 && g->mid_side != 0 && C == 2;
    const uint64_t nsamp = (uint64_t)g->num_samples * C, bytes = hb + nsamp * B;
    const uint32_t head = (uint32_t)((uintptr_t)dst & 15u);      // bytes of the first chunk before the destination
    const uint64_t chunks = (head + bytes + 15u) >> 4;
    for (uint64_t c = tid; c < chunks; c += nt) {
      const int64_t o0 = (int64_t)(c << 4) - head;               // the chunk's first byte, relative to the destination
      if (o0 >= (int64_t)hb && (uint64_t)o0 + 16u <= bytes) {
        const uint64_t p0 = (uint64_t)o0 - hb, s0 = p0 / B;
        const uint32_t b0 = (uint32_t)(p0 % B);
        uint32_t t[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t i = 0; i < NS; i++) {
          const uint32_t d = (i * B) / 4, sh = ((i * B) % 4) * 8;
          const uint32_t v = (s0 + i < nsamp) ? wav_emit_sample<B>(src, stride, C, ms, shift, s0 + i) : 0u;
          t[d] |= v << sh;
          if (sh + 8 * B > 32) { t[d + 1] |= v >> (32 - sh); }
        }
        wav_u4 q;
        q.x = __builtin_amdgcn_alignbyte(t[1], t[0], b0);
        q.y = __builtin_amdgcn_alignbyte(t[2], t[1], b0);
        q.z = __builtin_amdgcn_alignbyte(t[3], t[2], b0);
        q.w = __builtin_amdgcn_alignbyte(t[4], t[3], b0);
        *(wav_u4*)(dst + o0) = q;
      } else {
#pragma unroll 1
        for (uint32_t k = 0; k < 16; k++) {
          const int64_t i = o0 + (int64_t)k;
          if (i < 0 || (uint64_t)i >= bytes) { continue; }
          if ((uint64_t)i < hb) { dst[i] = g->header[i]; continue; }
          const uint64_t p = (uint64_t)i - hb;
          dst[i] = (uint8_t)(wav_emit_sample<B>(src, stride, C, ms, shift, p / B) >> (8 * (uint32_t)(p % B)));
        }
      }
    }
  }
}

extern "C" int sla_hip_launch_wav_emit_batch(const int32_t* d_planes, uint64_t plane_stride, const sla_hip_wav_emit* d_table,
                                             uint32_t num_entries, uint32_t max_samples, uint32_t num_channels,
                                             uint32_t bytes_per_sample, uint32_t mid_side, sla_hip_stream_t stream)
{
  if (d_table == nullptr || d_planes == nullptr) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_channels == 0 || num_channels > 8 || bytes_per_sample == 0 || bytes_per_sample > 4) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (mid_side != 0 && num_channels != 2) { return SLA_APIRESULT_INVALID_ARGUMENT; }
  if (num_entries == 0) { return 0; }
  // a workgroup row covers 4096 bytes of a file (256 lanes x 16); longer files grid-stride
  const uint64_t max_bytes = (uint64_t)SLA_HIP_WAV_HEADER_BYTES + (uint64_t)max_samples * num_channels * bytes_per_sample + 15u;
  uint64_t gx = (max_bytes + 4095) / 4096;
  if (gx > 1024) { gx = 1024; }
  const dim3 grid((uint32_t)gx, (num_entries < 65535u) ? num_entries : 65535u), block(256);
  hipStream_t st = (hipStream_t)stream;
#define WAV_EMIT(C_, B_) hipLaunchKernelGGL((k_wav_emit<C_, B_>), grid, block, 0, st, d_planes, plane_stride, d_table, num_entries, num_channels, mid_side)
  const uint32_t ct = (num_channels <= 2) ? num_channels : 0u;
  switch (ct * 8 + bytes_per_sample) {
    case 0 * 8 + 1: WAV_EMIT(0, 1); break;
    case 0 * 8 + 2: WAV_EMIT(0, 2); break;
    case 0 * 8 + 3: WAV_EMIT(0, 3); break;
    case 0 * 8 + 4: WAV_EMIT(0, 4); break;
    case 1 * 8 + 1: WAV_EMIT(1, 1); break;
    case 1 * 8 + 2: WAV_EMIT(1, 2); break;
    case 1 * 8 + 3: WAV_EMIT(1, 3); break;
    case 1 * 8 + 4: WAV_EMIT(1, 4); break;
    case 2 * 8 + 1: WAV_EMIT(2, 1); break;
    case 2 * 8 + 2: WAV_EMIT(2, 2); break;
    case 2 * 8 + 3: WAV_EMIT(2, 3); break;
    default:        WAV_EMIT(2, 4); break;
  }
#undef WAV_EMIT
  return hip_rc(hipGetLastError());
}
