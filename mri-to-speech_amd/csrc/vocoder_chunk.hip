// Streaming vocoder: the kernels of the stateless chunk call (DESIGN.md "Streaming vocoder").
//
// m2s_vocoder_forward_chunk runs the generator on packed spans of mel rows, of which only rows context[b] ..
// len[b] - hold[b] - 1 of clip b are emitted.  The convolutions are the dense kernels of the whole-clip calls on the
// padded (B, T, ...) block; the two kernels here are what the chunk call adds around them:
//   crop_rows_kernel       the cone: between stages, keep only the rows of every clip that an emitted sample still
//                          depends on, (B, L, row) -> (B, L', row) in whatever storage the engine's activations have
//   chunk_wav_pack_kernel  padded wav (B, T * hop) -> the emitted rows, packed in clip order (the sibling of
//                          ragged_wav_pack_kernel, which emits every row)
#include "kernels.hpp"

namespace m2s {

namespace {

inline unsigned nblk(long n) { return (unsigned)((n + 255) / 256); }

// y[b][r] = x[b][drop + r], rows of row16 16-byte words: fp32, bf16 and the split [hi | lo] pair are all contiguous
// rows, so one kernel serves every storage.  Every word of y is written; x is read inside its own clip only
// (the launcher checks drop + rows_out <= rows_in).
__global__ void __launch_bounds__(256) crop_rows_kernel(const uint4* __restrict__ x, int B, long rows_in, long drop,
                                                        long rows_out, int row16, uint4* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long per = rows_out * row16;
  if (i >= B * per) return;
  const long clip = i / per, j = i - clip * per;
  y[i] = x[(clip * rows_in + drop) * row16 + j];
}

// V = float4 when hop % 4 == 0 (hop counted in V then).  Thread i owns element i of the padded block; it stores only
// if its row is one its clip emits, so the writes cover exactly the sum(n) * hop elements of dst.
template <typename V>
__global__ void __launch_bounds__(256) chunk_wav_pack_kernel(const V* __restrict__ src, const int* __restrict__ from,
                                                             const int* __restrict__ to, const int* __restrict__ n,
                                                             int B, int T, int hop, V* __restrict__ dst) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long per = (long)T * hop;
  if (i >= B * per) return;
  const int clip = (int)(i / per);
  const long j = i - clip * per - (long)from[clip] * hop;
  if (j >= 0 && j < (long)n[clip] * hop) dst[(long)to[clip] * hop + j] = src[i];
}

}  // namespace

void launch_crop_rows(const void* x, int B, long rows_in, long drop, long rows_out, size_t row_bytes, void* y,
                      hipStream_t s) {
  M2S_CHECK(row_bytes % 16 == 0 && B >= 1, "crop_rows: rows of whole 16-byte words");
  M2S_CHECK(drop >= 0 && rows_out >= 1 && drop + rows_out <= rows_in, "crop_rows: rows outside the block");
  const int row16 = (int)(row_bytes / 16);
  hipLaunchKernelGGL(crop_rows_kernel, dim3(nblk((long)B * rows_out * row16)), dim3(256), 0, s,
                     reinterpret_cast<const uint4*>(x), B, rows_in, drop, rows_out, row16, reinterpret_cast<uint4*>(y));
  M2S_HIP(hipGetLastError());
}

void launch_chunk_wav_pack(const float* wav_padded, const int* src, const int* dst, const int* n, int B, int T, int hop,
                           float* wav, hipStream_t s) {
  if (hop % 4 == 0)
    hipLaunchKernelGGL(chunk_wav_pack_kernel<float4>, dim3(nblk((long)B * T * (hop / 4))), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(wav_padded), src, dst, n, B, T, hop / 4,
                       reinterpret_cast<float4*>(wav));
  else
    hipLaunchKernelGGL(chunk_wav_pack_kernel<float>, dim3(nblk((long)B * T * hop)), dim3(256), 0, s, wav_padded, src,
                       dst, n, B, T, hop, wav);
  M2S_HIP(hipGetLastError());
}

}  // namespace m2s
