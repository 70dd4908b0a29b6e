// Ragged batches: clips of different lengths in one engine call (DESIGN.md "Ragged batches").
//
// The public surface is packed: clip b of `len[b]` steps owns rows off[b] .. off[b] + len[b] - 1 of an (N, ...)
// tensor, N = sum(len), off = exclusive prefix sum.  Inside the engine the batched kernels keep their dense
// (B, Tmax, ...) blocks; the kernels here move rows between the two forms and write the exact zeros the dense
// kernels must see past a short clip's end.  Every kernel finds its clip through the device table
// tab = [off: B ints | len: B ints] and walks the PADDED index space, so none needs a row -> clip search.
#include "kernels.hpp"

namespace m2s {

namespace {

inline unsigned nblk(long n) { return (unsigned)((n + 255) / 256); }

// Packed gate pre-activations (N, 8H) -> the padded (B, Tmax, 8H) block of the recurrence kernels, one pass of
// 16-byte accesses.  Rows (b, t >= len[b]) are exact zeros, bias included: h = c = 0 is then a fixed point of
// the cell, so the reverse direction of clip b reaches t = len[b] - 1 with the zero state it must start from.
__global__ void __launch_bounds__(256) ragged_pre_scatter_kernel(const float4* __restrict__ src,
                                                                 const int* __restrict__ tab, int B, int Tmax, int q,
                                                                 float4* __restrict__ dst) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Tmax * q) return;
  const long r = i / q;
  const int c = (int)(i - r * q), b = (int)(r / Tmax), t = (int)(r - (long)b * Tmax);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < tab[B + b]) v = src[((long)tab[b] + t) * q + c];
  dst[i] = v;
}

// mel_head_kernel (kernels.hip) on the valid rows of hs (2, B, Tmax, H): workgroup (t, b) reads row b Tmax + t
// and writes packed row off[b] + t of y (the sum merge, add2_kernel's a + b) and / or of the head output.  The K
// split, the FMA chains and the order of the partial sums are mel_head_kernel's, so a row rounds as it does there.
constexpr int HEAD_W = 16;  // = kernels.hip HEAD_W
__global__ void __launch_bounds__(64 * HEAD_W) ragged_head_gather_kernel(const float* __restrict__ hs,
                                                                        const int* __restrict__ tab, int B, int Tmax,
                                                                        int H, const float* __restrict__ wt,
                                                                        const float* __restrict__ b, int n_mels,
                                                                        float* __restrict__ y, float* __restrict__ out) {
  extern __shared__ float ys[];  // [H] + [HEAD_W][64] partial sums
  float* part = ys + H;
  const int t = blockIdx.x, clip = blockIdx.y;
  if (t >= tab[B + clip]) return;  // uniform over the workgroup
  const long src = (long)clip * Tmax + t, row = (long)tab[clip] + t;
  const long plane = (long)B * Tmax * H;
  for (int k = threadIdx.x; k < H; k += 64 * HEAD_W) {
    const float v = hs[src * H + k] + hs[plane + src * H + k];
    ys[k] = v;
    if (y) y[row * H + k] = v;
  }
  if (!out) return;
  __syncthreads();
  const int q = threadIdx.x >> 6;
  const int k0 = q * H / HEAD_W, k1 = (q + 1) * H / HEAD_W;
  for (int nb = 0; nb < n_mels; nb += 64) {
    const int n = nb + (threadIdx.x & 63);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < n_mels) {
      int k = k0;
      for (; k + 4 <= k1; k += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = fmaf(ys[k + j], wt[(long)(k + j) * n_mels + n], a[j]);
      }
      for (; k < k1; ++k) a[0] = fmaf(ys[k], wt[(long)k * n_mels + n], a[0]);
    }
    if (nb > 0) __syncthreads();  // the previous pass's partials were read
    part[threadIdx.x] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    const int l = threadIdx.x & 63;
    if (q == 0 && n < n_mels) {
      float p[HEAD_W];
#pragma unroll
      for (int w = 0; w < HEAD_W; ++w) p[w] = part[64 * w + l];
#pragma unroll
      for (int st = 1; st < HEAD_W; st *= 2)  // pairwise, fixed order
#pragma unroll
        for (int w = 0; w < HEAD_W; w += 2 * st) p[w] += p[w + st];
      out[row * n_mels + n] = p[0] + b[n];
    }
  }
}

// Packed mel (N, n_mels) -> the padded channel-last (B, Tmax, cs) ln-mel of the vocoder, exact zeros at
// t >= len[b] (conv_pre looks 6 frames past a clip's end and expects zeros there) and in the pad channels.
// GLUE: x is mel_norm and the value is mel_glue_kernel's (same operations, contraction off), with packed mel_db /
// mel_log outputs; otherwise x is the ln-mel itself (mel_to_nlc_kernel, layout 1).
template <typename T, bool GLUE>
__global__ void __launch_bounds__(256) ragged_glue_kernel(const float* __restrict__ x, const int* __restrict__ tab,
                                                          int B, int Tmax, int n_mels, const float* __restrict__ mean,
                                                          const float* __restrict__ sd, float* db, float* ln, T* ln_t,
                                                          int cs) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Tmax * cs) return;
  const long r = i / cs;
  const int n = (int)(i - r * cs), clip = (int)(r / Tmax), t = (int)(r - (long)clip * Tmax);
  if (n >= n_mels || t >= tab[B + clip]) {
    act_st<T>(ln_t, r, cs, n, 0.f);
    return;
  }
  const long o = ((long)tab[clip] + t) * n_mels + n;
  if constexpr (GLUE) {
#pragma clang fp contract(off)
    const float d = x[o] * sd[n] + mean[n];
    const float p = powf(10.0f, d / 10.0f);
    const float l = logf(fmaxf(p, 1e-5f));
    if (db) db[o] = d;
    if (ln) ln[o] = l;
    act_st<T>(ln_t, r, cs, n, l);
  } else {
    act_st<T>(ln_t, r, cs, n, x[o]);
  }
}

// Zeroes `halo` rows from row len[b] * scale of clip b in an activation buffer of `rows` = Tmax * scale rows per
// clip, each row `row16` 16-byte words: fp32 (cs x 4 bytes), bf16 (cs x 2) and the split pair ([hi cs | lo cs]
// bf16, both halves) are all contiguous rows of zero bits, so one kernel serves every storage.  Rows past the
// clip's own block are not touched (len[b] = Tmax writes nothing).
__global__ void __launch_bounds__(256) ragged_tail_mask_kernel(uint4* __restrict__ x, const int* __restrict__ tab,
                                                               int B, int rows, int scale, int halo, int row16) {
  const int clip = blockIdx.y;
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= (long)halo * row16) return;
  const long r = (long)tab[B + clip] * scale + j / row16;
  if (r >= rows) return;
  x[((long)clip * rows + r) * row16 + j % row16] = make_uint4(0u, 0u, 0u, 0u);
}

// Padded wav (B, Tmax * hop) -> packed (N * hop); V = float4 when hop % 4 == 0 (hop counted in V then).
template <typename V>
__global__ void __launch_bounds__(256) ragged_wav_pack_kernel(const V* __restrict__ src, const int* __restrict__ tab,
                                                              int B, int Tmax, int hop, V* __restrict__ dst) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long per = (long)Tmax * hop;
  if (i >= B * per) return;
  const int clip = (int)(i / per);
  const long j = i - clip * per;
  if (j < (long)tab[B + clip] * hop) dst[(long)tab[clip] * hop + j] = src[i];
}

}  // namespace

void launch_ragged_pre_scatter(const float* pre_packed, const int* tab, int B, int Tmax, int width, float* pre,
                               hipStream_t s) {
  M2S_CHECK(width % 4 == 0, "ragged_pre_scatter: row width % 4");
  hipLaunchKernelGGL(ragged_pre_scatter_kernel, dim3(nblk((long)B * Tmax * (width / 4))), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(pre_packed), tab, B, Tmax, width / 4,
                     reinterpret_cast<float4*>(pre));
  M2S_HIP(hipGetLastError());
}

void launch_ragged_head_gather(const float* hs, const int* tab, int B, int Tmax, int H, const float* wt, const float* b,
                               int n_mels, float* y, float* mel_norm, hipStream_t s) {
  M2S_CHECK(n_mels >= 1 && H >= 4 && B <= 65535, "ragged_head_gather: shape");
  hipLaunchKernelGGL(ragged_head_gather_kernel, dim3(Tmax, B), dim3(64 * HEAD_W), (H + HEAD_W * 64) * sizeof(float), s,
                     hs, tab, B, Tmax, H, wt, b, n_mels, y, mel_norm);
  M2S_HIP(hipGetLastError());
}

template <typename T>
void launch_ragged_glue(const float* x, const int* tab, int B, int Tmax, int n_mels, const float* mean,
                        const float* std_, float* db, float* ln, T* ln_t, int cs, hipStream_t s) {
  const dim3 grid(nblk((long)B * Tmax * cs));
  if (mean)
    hipLaunchKernelGGL((ragged_glue_kernel<T, true>), grid, dim3(256), 0, s, x, tab, B, Tmax, n_mels, mean, std_, db, ln,
                       ln_t, cs);
  else
    hipLaunchKernelGGL((ragged_glue_kernel<T, false>), grid, dim3(256), 0, s, x, tab, B, Tmax, n_mels, mean, std_, db,
                       ln, ln_t, cs);
  M2S_HIP(hipGetLastError());
}

void launch_ragged_tail_mask(void* x, const int* tab, int B, int rows, int scale, int halo, size_t row_bytes,
                             hipStream_t s) {
  M2S_CHECK(row_bytes % 16 == 0 && B <= 65535, "ragged_tail_mask: rows of whole 16-byte words");
  if (halo <= 0) return;
  const int row16 = (int)(row_bytes / 16);
  hipLaunchKernelGGL(ragged_tail_mask_kernel, dim3(nblk((long)halo * row16), B), dim3(256), 0, s,
                     reinterpret_cast<uint4*>(x), tab, B, rows, scale, halo, row16);
  M2S_HIP(hipGetLastError());
}

void launch_ragged_wav_pack(const float* wav_padded, const int* tab, int B, int Tmax, int hop, float* wav,
                            hipStream_t s) {
  if (hop % 4 == 0)
    hipLaunchKernelGGL(ragged_wav_pack_kernel<float4>, dim3(nblk((long)B * Tmax * (hop / 4))), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(wav_padded), tab, B, Tmax, hop / 4,
                       reinterpret_cast<float4*>(wav));
  else
    hipLaunchKernelGGL(ragged_wav_pack_kernel<float>, dim3(nblk((long)B * Tmax * hop)), dim3(256), 0, s, wav_padded, tab,
                       B, Tmax, hop, wav);
  M2S_HIP(hipGetLastError());
}

#define M2S_RAGGED_INST(T)                                                                                          \
  template void launch_ragged_glue<T>(const float*, const int*, int, int, int, const float*, const float*, float*, \
                                      float*, T*, int, hipStream_t);
M2S_RAGGED_INST(float)
M2S_RAGGED_INST(bf16_t)
M2S_RAGGED_INST(sp_t)

}  // namespace m2s
