// verify.inc -- k_verify_blocks: k_dec_finish fused with a compare instead of a store (option "verify" of the encoder).
// Included from sla_decode.hip, inside its anonymous namespace.
//
// One workgroup per block of the table.  The decoded planes of the block -- right-justified, mid/side still folded -- are
// finished exactly as k_dec_finish_batch finishes them (src/SLAUtility.c:415-433, src/SLADecoder.c:540-547) and compared,
// all 32 bits, with the source plane words at the same positions.  Nothing outside [smp_off, smp_off + num_samples) of a
// block is read.  A lane takes the four samples of one 16-byte group of the planes (groups are cut at multiples of four
// plane positions, so a block that starts or ends inside a group gets a guarded group at that end): one 16-byte load per
// array and channel where that array's row is 16-byte aligned, four guarded 4-byte loads otherwise.
// Report: three 64-bit words per segment {differing sample-channels, smallest (position << 3 | channel) of one, bad
// blocks}.  A wave reduces first and touches the words only when it has something to report.

struct verify_args {
  const int32_t* planes; uint64_t stride;
  const int32_t* source; uint64_t sstride;
  const sla_hip_dec_block* blocks; const sla_hip_dec_info* info; const sla_hip_verify_expect* expect;
  const uint32_t* seg_of_block;
  const uint8_t* image; uint64_t image_bytes;
  unsigned long long* report;
  uint32_t num_channels, mid_side, shift;
};

// samples [g, g + 4) of a row; those outside [lo, hi) read as zero and are not touched
__device__ __forceinline__ void verify_load4(const int32_t* row, uint64_t g, uint64_t lo, uint64_t hi, bool vload, int32_t v[4])
{
  typedef int32_t i4 __attribute__((ext_vector_type(4)));
  if (vload && g >= lo && g + 4 <= hi) {
    const i4 q = *(const i4*)(row + g);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = (g + k >= lo && g + k < hi) ? row[g + k] : 0; }
  }
}

__device__ __forceinline__ bool verify_row_aligned(const int32_t* base, uint64_t row_off)
{
  return (((uintptr_t)base >> 2) + row_off) % 4 == 0 && ((uintptr_t)base & 3u) == 0;
}

// the block's structure: what the parser found against what the packer laid out
__device__ __forceinline__ bool verify_block_bad(const verify_args& a, uint32_t j, const sla_hip_dec_block& b)
{
  const sla_hip_dec_info in = a.info[j];
  const sla_hip_verify_expect ex = a.expect[j];
  bool bad = (in.type != ex.type) || (in.used_bytes != ex.bytes) || (in.overrun != 0);
  if (a.image != nullptr) {
    if (b.byte_off + 8 <= a.image_bytes) {
      const uint32_t field = ((uint32_t)a.image[b.byte_off + 6] << 8) | (uint32_t)a.image[b.byte_off + 7];
      bad = bad || (field != in.crc);
    } else {
      bad = true;
    }
  }
  return bad;
}

// lane `tid` of the block's 256: its groups of four positions, every channel; counts the differing sample-channels and
// keeps the smallest (position << 3 | channel) among them
__device__ __forceinline__ void verify_scan(const verify_args& a, const sla_hip_dec_block& b, uint32_t tid, uint32_t& ndiff,
                                            unsigned long long& first)
{
  const uint32_t C = a.num_channels, shift = a.shift;
  const uint64_t lo = b.smp_off, hi = (uint64_t)b.smp_off + b.num_samples;
  const bool ms = a.mid_side != 0 && C == 2;
  for (uint64_t g = (lo & ~3ull) + 4ull * tid; g < hi; g += 4ull * 256) {
    if (ms) {
      int32_t m[4], s[4], l[4], r[4];
      verify_load4(a.planes, g, lo, hi, verify_row_aligned(a.planes, 0), m);
      verify_load4(a.planes + a.stride, g, lo, hi, verify_row_aligned(a.planes, a.stride), s);
      verify_load4(a.source, g, lo, hi, verify_row_aligned(a.source, 0), l);
      verify_load4(a.source + a.sstride, g, lo, hi, verify_row_aligned(a.source, a.sstride), r);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (g + k < lo || g + k >= hi) { continue; }
        int32_t dl, dr;
        emit_lr(m[k], s[k], shift, dl, dr);
        if (dl != l[k]) { const unsigned long long key = (g + k) << 3; ndiff++; first = (key < first) ? key : first; }
        if (dr != r[k]) { const unsigned long long key = ((g + k) << 3) | 1ull; ndiff++; first = (key < first) ? key : first; }
      }
    } else {
      for (uint32_t c = 0; c < C; c++) {
        int32_t d[4], s[4];
        verify_load4(a.planes + (uint64_t)c * a.stride, g, lo, hi, verify_row_aligned(a.planes, (uint64_t)c * a.stride), d);
        verify_load4(a.source + (uint64_t)c * a.sstride, g, lo, hi, verify_row_aligned(a.source, (uint64_t)c * a.sstride), s);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (g + k < lo || g + k >= hi) { continue; }
          if ((int32_t)((uint32_t)d[k] << shift) != s[k]) {
            const unsigned long long key = ((g + k) << 3) | c;
            ndiff++;
            first = (key < first) ? key : first;
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(256)
void k_verify_blocks(const verify_args a)
{
  const uint32_t j = blockIdx.x;
  const sla_hip_dec_block b = a.blocks[j];
  if (b.flags & SLA_HIP_DEC_HEADER_ONLY) { return; }
  const uint32_t seg = (a.seg_of_block != nullptr) ? a.seg_of_block[j] : 0u;
  unsigned long long* rep = a.report + 3ull * seg;
  if (threadIdx.x == 0 && verify_block_bad(a, j, b)) { atomicAdd(rep + 2, 1ull); }

  uint32_t ndiff = 0;
  unsigned long long first = ~0ull;
  verify_scan(a, b, threadIdx.x, ndiff, first);
  // inside the wave first; one lane speaks, and only when there is something to say
  for (int off = 32; off > 0; off >>= 1) {
    ndiff += (uint32_t)__shfl_xor((int)ndiff, off);
    const unsigned long long o = shfl_u64(first, (threadIdx.x & 63u) ^ (uint32_t)off);
    first = (o < first) ? o : first;
  }
  if ((threadIdx.x & 63u) == 0 && ndiff != 0) {
    atomicAdd(rep, (unsigned long long)ndiff);
    atomicMin(rep + 1, first);
  }
}
