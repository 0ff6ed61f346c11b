// kernels/emit.inc -- part of sla_kernels.hip (one translation unit; included there, in this order): k_enc_emit (launcher: launchers.inc)
//
// k_enc_emit: the delivery leg of sla_hip_encode_batch_resident, the mirror of k_dec_gather (sla_decode.hip).  The pack image
// holds the files of a pass back to back at ANY byte offset, each with its 43 header bytes still zero; entry k of the table
// copies one file to a caller's device buffer at ANY byte address and puts the header the host built (it travels in the
// table) in front.  blockIdx.y walks the table, the x dimension the aligned 16-byte chunks of the destination.
//   * A chunk that lies wholly inside [dst + header_bytes, dst + bytes) takes its 16 bytes from the one or two ALIGNED 16-byte
//     words of the image that hold them (two 16-byte loads, a word select by the source's word misalignment, v_alignbyte_b32
//     by its byte misalignment) and goes out in one 16-byte store.  Both of those words hold at least one byte of the file.
//   * Every other chunk -- the file's head with the header, its tail -- goes out byte by byte, each byte guarded: files packed
//     back to back in an arena share 4-byte words and 16-byte chunks with their neighbours, which other lanes (of this entry's
//     neighbours) write in the same launch, so a store may not even rewrite a neighbour's byte with the value it read.
// No byte outside [dst, dst + bytes) is written and nothing outside [img_off, img_off + bytes) of the image is needed.  The
// 16-byte loads are aligned by address, so they may reach up to 15 bytes before a file's first byte or past its last: the
// image must be readable in whole aligned 16-byte words (include/sla_hip.h; pack_device_core pads d_image for it).
typedef uint32_t emit_u4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256)
void k_enc_emit(const sla_hip_enc_emit* __restrict__ table, uint32_t num_entries, const uint8_t* __restrict__ image,
                uint64_t image_bytes)
{
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (uint64_t)gridDim.x * blockDim.x;
  for (uint32_t e = blockIdx.y; e < num_entries; e += gridDim.y) {
    const sla_hip_enc_emit* g = &table[e];
    const uint64_t img_off = g->img_off;
    const uint32_t bytes = g->bytes, hb = g->header_bytes;
    uint8_t* dst = g->dst;
    if (img_off > image_bytes || bytes > image_bytes - img_off) { continue; }
    if ((hb != 0 && hb != 43u) || hb > bytes || dst == nullptr) { continue; }
    const uint8_t* src = image + img_off;
    const uint32_t head = (uint32_t)((uintptr_t)dst & 15u);     // bytes of the first chunk before the destination
    const uint64_t chunks = ((uint64_t)head + bytes + 15u) >> 4;
    for (uint64_t c = tid; c < chunks; c += nt) {
      const int64_t o0 = (int64_t)(c << 4) - head;               // the chunk's first byte, relative to the destination
      if (o0 >= (int64_t)hb && (uint64_t)o0 + 16u <= bytes) {
        const uint32_t o = (uint32_t)o0;
        const uintptr_t s = (uintptr_t)src + o;
        const uint32_t r = (uint32_t)(s & 15u);
        const emit_u4* a = (const emit_u4*)(s & ~(uintptr_t)15);
        const emit_u4 q0 = a[0];                                 // holds byte o
        emit_u4 q1 = {0u, 0u, 0u, 0u};
        if (r != 0) { q1 = a[1]; }                               // holds byte o + 16 - r, which is before o + 16 <= bytes
        uint32_t w[5];
        switch (r >> 2) {
          case 0:  w[0] = q0.x; w[1] = q0.y; w[2] = q0.z; w[3] = q0.w; w[4] = q1.x; break;
          case 1:  w[0] = q0.y; w[1] = q0.z; w[2] = q0.w; w[3] = q1.x; w[4] = q1.y; break;
          case 2:  w[0] = q0.z; w[1] = q0.w; w[2] = q1.x; w[3] = q1.y; w[4] = q1.z; break;
          default: w[0] = q0.w; w[1] = q1.x; w[2] = q1.y; w[3] = q1.z; w[4] = q1.w; break;
        }
        emit_u4 q;
        q.x = __builtin_amdgcn_alignbyte(w[1], w[0], r & 3u);
        q.y = __builtin_amdgcn_alignbyte(w[2], w[1], r & 3u);
        q.z = __builtin_amdgcn_alignbyte(w[3], w[2], r & 3u);
        q.w = __builtin_amdgcn_alignbyte(w[4], w[3], r & 3u);
        *(emit_u4*)(dst + o) = q;
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
          const int64_t i = o0 + (int64_t)k;
          if (i >= 0 && (uint64_t)i < bytes) { dst[i] = ((uint64_t)i < hb) ? g->header[i] : src[i]; }
        }
      }
    }
  }
}
