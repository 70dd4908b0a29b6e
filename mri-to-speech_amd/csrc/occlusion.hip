// Occlusion sensitivity on the device (include/m2s.h "occlusion"): the mels of V = 1 + M variants of
// one clip (variant 0 unmasked, variant m + 1 under mask m) -> per-band scores and a coverage-weighted map, in two
// launches and without a host read.  A band is a 0 / 1 row over the mel bins (the Grad-CAM tool's bands); an "all
// bins" column is appended, nb = n_bands + 1.
//
// occlusion_score_kernel: one workgroup of four waves per masked variant.  A wave takes the frames t = wave, wave + 4,
// ...; lane l holds the bins l, l + 64, l + 128, l + 192 of |mel[m + 1][t] - mel[0][t]|, adds its own bins of a band in
// ascending order and the 64 lanes in a butterfly (xor 32 .. 1; float addition commutes, so every lane ends with
// the same bits).  per_frame = that sum / the band's bin count.  The sums of a wave's frames are added in ascending t
// in double, the four waves in ascending order in double, score = total / (T * bins), rounded once.  An empty band
// scores 0.
//
// occlusion_map_kernel: grid (band, pixel blocks).  c_m = max(1 - masks[m], 0); a thread owns its pixels and adds
// c_m and c_m * score[m][band] over ascending m; map = the quotient where the coverage exceeds 1e-6, else 0.  With
// `normalize` one workgroup walks the whole band, reduces min and max in a fixed tree and rewrites its own pixels as
// (v - min) / ((max - min) + 1e-6), the Grad-CAM heat maps' rule: a flat band gives exact zeros.
//
// No atomics and no order that depends on scheduling: repeated calls are bit-identical.
#include <algorithm>

#include "kernels.hpp"
#include "prof.hpp"

namespace m2s {
namespace {

constexpr int OC_ST = 256;    // threads of the score kernel
constexpr int OC_SW = OC_ST / 64;
constexpr int OC_MT = 1024;   // threads of the map kernel
constexpr int OC_MAXNB = 9;   // 8 bands + all bins
constexpr int OC_MAXMEL = 256;
constexpr int OC_Q = OC_MAXMEL / 64;  // bins per lane

__global__ void __launch_bounds__(OC_ST) occlusion_score_kernel(const float* __restrict__ mel, int T, int n_mels,
                                                                const float* __restrict__ band_mask, int n_bands,
                                                                float* __restrict__ score, float* __restrict__ per_frame) {
  __shared__ double part[OC_SW][OC_MAXNB];
  __shared__ int cnts[OC_MAXNB];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nb = n_bands + 1;
  const float* base = mel;
  const float* var = mel + (size_t)(m + 1) * T * n_mels;

  // bit b of bits[q]: bin lane + 64 q belongs to band b (bit n_bands: every real bin)
  unsigned bits[OC_Q];
  int cnt[OC_MAXNB];
#pragma unroll
  for (int q = 0; q < OC_Q; ++q) {
    const int j = lane + 64 * q;
    unsigned v = 0;
    if (j < n_mels) {
      v = 1u << n_bands;
      for (int b = 0; b < n_bands; ++b) v |= (band_mask[b * n_mels + j] != 0.f ? 1u : 0u) << b;
    }
    bits[q] = v;
  }
#pragma unroll
  for (int b = 0; b < OC_MAXNB; ++b) {
    int c = 0;
#pragma unroll
    for (int q = 0; q < OC_Q; ++q) c += (bits[q] >> b) & 1;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s);
    cnt[b] = c;
  }

  double acc[OC_MAXNB];
#pragma unroll
  for (int b = 0; b < OC_MAXNB; ++b) acc[b] = 0.0;
  for (int t = wave; t < T; t += OC_SW) {
    float d[OC_Q];
#pragma unroll
    for (int q = 0; q < OC_Q; ++q) {
      const int j = lane + 64 * q;
      d[q] = j < n_mels ? fabsf(var[(size_t)t * n_mels + j] - base[(size_t)t * n_mels + j]) : 0.f;
    }
#pragma unroll
    for (int b = 0; b < OC_MAXNB; ++b) {
      if (b < nb) {  // uniform
        float sum = 0.f;
#pragma unroll
        for (int q = 0; q < OC_Q; ++q) sum += ((bits[q] >> b) & 1) ? d[q] : 0.f;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s);
        if (per_frame && lane == 0) per_frame[((size_t)m * T + t) * nb + b] = cnt[b] > 0 ? sum / (float)cnt[b] : 0.f;
        acc[b] += (double)sum;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int b = 0; b < OC_MAXNB; ++b) part[wave][b] = acc[b];
    if (wave == 0) {
#pragma unroll
      for (int b = 0; b < OC_MAXNB; ++b) cnts[b] = cnt[b];
    }
  }
  __syncthreads();
  if (tid < nb) {
    double tot = 0.0;
    for (int v = 0; v < OC_SW; ++v) tot += part[v][tid];
    score[(size_t)m * nb + tid] = cnts[tid] > 0 ? (float)(tot / ((double)T * (double)cnts[tid])) : 0.f;
  }
}

__global__ void __launch_bounds__(OC_MT) occlusion_map_kernel(const float* __restrict__ score, int M, int nb,
                                                              const float* __restrict__ masks, int hw, int normalize,
                                                              float* __restrict__ map) {
  __shared__ float rmin[OC_MT / 64], rmax[OC_MT / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  float* o = map + (size_t)b * hw;
  float mn = INFINITY, mx = -INFINITY;
  for (int p = blockIdx.y * OC_MT + tid; p < hw; p += gridDim.y * OC_MT) {
    float den = 0.f, num = 0.f;
    for (int m = 0; m < M; ++m) {
      const float c = fmaxf(1.f - masks[(size_t)m * hw + p], 0.f);
      den += c;
      num += c * score[(size_t)m * nb + b];
    }
    const float v = den > 1e-6f ? num / den : 0.f;
    o[p] = v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  if (!normalize) return;  // uniform; below, gridDim.y == 1: this workgroup owns the band
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, s));
    mx = fmaxf(mx, __shfl_xor(mx, s));
  }
  if ((tid & 63) == 0) rmin[tid >> 6] = mn, rmax[tid >> 6] = mx;
  __syncthreads();
  mn = rmin[0], mx = rmax[0];
  for (int v = 1; v < OC_MT / 64; ++v) mn = fminf(mn, rmin[v]), mx = fmaxf(mx, rmax[v]);
  const float den = (mx - mn) + 1e-6f;
  for (int p = tid; p < hw; p += OC_MT) o[p] = (o[p] - mn) / den;  // a thread rereads its own stores
}

}  // namespace

void launch_occlusion_reduce(const float* mel, int V, int T, int n_mels, const float* band_mask, int n_bands,
                             const float* masks, int h, int w, int normalize, float* score, float* per_frame, float* map,
                             hipStream_t s) {
  M2S_CHECK(V >= 2, "occlusion_reduce: V < 2 (variant 0 is the baseline)");
  M2S_CHECK(T >= 1, "occlusion_reduce: T < 1");
  M2S_CHECK(n_mels >= 1 && n_mels <= OC_MAXMEL, "occlusion_reduce: n_mels outside 1..256");
  M2S_CHECK(n_bands >= 0 && n_bands <= OC_MAXNB - 1, "occlusion_reduce: n_bands outside 0..8");
  M2S_CHECK(band_mask || n_bands == 0, "occlusion_reduce: null band_mask");
  M2S_CHECK(mel && score, "occlusion_reduce: null argument");
  const int M = V - 1, nb = n_bands + 1;
  if (map) {
    M2S_CHECK(masks && h >= 1 && w >= 1 && (long)h * w <= 2147483647L / 2, "occlusion_reduce: a map needs masks (M, h, w)");
  }
  StageTag tag("occlusion");
  {
    const double elems = (double)V * T * n_mels;
    ProfScope ps("occlusion_score_kernel", 2.0 * elems * nb, 4.0 * (elems + (double)M * (T + 1) * nb), s);
    hipLaunchKernelGGL(occlusion_score_kernel, dim3(M), dim3(OC_ST), 0, s, mel, T, n_mels, band_mask, n_bands, score,
                       per_frame);
    M2S_HIP(hipGetLastError());
  }
  if (!map) return;
  const int hw = h * w;
  const int gy = normalize ? 1 : std::min((hw + OC_MT - 1) / OC_MT, 1024);  // the pixel loop strides by the grid
  ProfScope ps("occlusion_map_kernel", 3.0 * (double)nb * M * hw, 4.0 * (double)nb * hw * (M + 1.0), s);
  hipLaunchKernelGGL(occlusion_map_kernel, dim3(nb, gy), dim3(OC_MT), 0, s, score, M, nb, masks, hw, normalize ? 1 : 0, map);
  M2S_HIP(hipGetLastError());
}

}  // namespace m2s
