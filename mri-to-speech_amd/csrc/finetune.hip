// Fine-tuning glue (include/m2s.h "fine-tuning", DESIGN.md "Fine-tuning"): the gather of per-frame targets onto
// pairs, the criterion's denominators and gradient, the gradient norm, the clip factor and the AdamW update.
// The LOSS slots themselves come from metrics.hip's kernels on the gathered pairs; the gradient kernel below
// differentiates exactly that LOSS.  Fixed partitions, fixed orders, no atomics, vector stores only.
#include <cmath>

#include "finetune.hpp"
#include "prof.hpp"

namespace m2s {
namespace {

unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

__global__ void __launch_bounds__(256) ft_gather_kernel(const float* __restrict__ target, const float* __restrict__ mask,
                                                        const int* __restrict__ win, int P, int W, int M,
                                                        float* __restrict__ tgt, float* __restrict__ msk) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)P * W * M) return;
  const int m = (int)(i % M);
  const long ps = i / M;
  const int s = (int)(ps % W), p = (int)(ps / W);
  const long row = (long)win[p] + s;
  tgt[i] = target[row * M + m];
  if (m == 0) msk[ps] = mask ? mask[row] : 1.f;
}

// one workgroup: the four denominators as metrics.hip forms them (sum freq_w x a sum over rows, floored at 1e-6),
// in double, windows in a fixed partition (thread t: windows t, t + 256, ...) and a fixed tree
__global__ void __launch_bounds__(256) ft_denominators_kernel(const float* __restrict__ msk,
                                                              const FtHyper* __restrict__ hy, int P, int W, int M,
                                                              FtScalars* __restrict__ sc) {
  __shared__ double red[3][256];
  const int tid = threadIdx.x;
  double st = 0.0, sd = 0.0, sa = 0.0;
  for (int p = tid; p < P; p += 256) {
    const float* mk = msk + (long)p * W;
    for (int t = 0; t < W; ++t) {
      const double tw = hy->time_w[t], m1 = mk[t];
      st += tw * m1;
      if (t >= 1) {
        const double m0 = mk[t - 1];
        sd += tw * m1 * m0;
        if (t + 1 < W) sa += tw * (double)mk[t + 1] * m1 * m0;
      }
    }
  }
  red[0][tid] = st, red[1][tid] = sd, red[2][tid] = sa;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h)
      for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    double sfw = 0.0;
    for (int m = 0; m < M; ++m) sfw += (double)hy->freq_w[m];
    sc->k_mse = (float)(2.0 / fmax(sfw * red[0][0], 1e-6));
    sc->k_delta = W > 1 ? (float)(2.0 * (double)hy->coeff[0] / fmax(sfw * red[1][0], 1e-6)) : 0.f;
    sc->k_accel = W > 2 ? (float)(2.0 * (double)hy->coeff[1] / fmax(sfw * red[2][0], 1e-6)) : 0.f;
    sc->k_latest = (float)(2.0 * (double)hy->coeff[2] / fmax((double)P * sfw, 1e-6));
  }
}

// dLOSS / dpred of one (window, mel bin) column: the delta term spreads over 2 rows with the later row's time weight,
// the acceleration term over 3 with the middle row's; the MAE is not in LOSS
__global__ void __launch_bounds__(256) ft_criterion_grad_kernel(const float* __restrict__ pred,
                                                                const float* __restrict__ tgt,
                                                                const float* __restrict__ msk,
                                                                const FtHyper* __restrict__ hy,
                                                                const FtScalars* __restrict__ sc, int P, int W, int M,
                                                                float* __restrict__ dpred) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)P * M) return;
  const int p = (int)(i / M), m = (int)(i - (long)p * M);
  double d[FT_MAXW], mk[FT_MAXW], g[FT_MAXW];
  const long base = (long)p * W * M + m;
#pragma unroll
  for (int t = 0; t < FT_MAXW; ++t) {
    d[t] = mk[t] = g[t] = 0.0;
    if (t < W) {
      d[t] = (double)pred[base + (long)t * M] - (double)tgt[base + (long)t * M];
      mk[t] = msk[(long)p * W + t];
    }
  }
  const double km = sc->k_mse, kd = sc->k_delta, ka = sc->k_accel, kl = sc->k_latest;
#pragma unroll
  for (int t = 0; t < FT_MAXW; ++t) {
    if (t >= W) break;
    const double tw = hy->time_w[t];
    g[t] += km * tw * mk[t] * d[t];
    if (t >= 1) {
      const double w = kd * tw * mk[t] * mk[t - 1], dl = d[t] - d[t - 1];
      g[t] += w * dl;
      g[t - 1] -= w * dl;
      if (t + 1 < W) {
        const double wa = ka * tw * mk[t + 1] * mk[t] * mk[t - 1], ac = d[t + 1] - 2.0 * d[t] + d[t - 1];
        g[t + 1] += wa * ac;
        g[t] -= 2.0 * wa * ac;
        g[t - 1] += wa * ac;
      }
    }
    if (t == W - 1) g[t] += kl * d[t];
  }
  const double fw = hy->freq_w[m];
#pragma unroll
  for (int t = 0; t < FT_MAXW; ++t)
    if (t < W) dpred[base + (long)t * M] = (float)(fw * g[t]);
}

constexpr int NORM_CHUNK = 1024;
__global__ void __launch_bounds__(256) ft_sumsq_kernel(const float* __restrict__ g, long n, double* __restrict__ part) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const long i0 = (long)blockIdx.x * NORM_CHUNK;
  double s = 0.0;
  for (int q = 0; q < NORM_CHUNK / 256; ++q) {
    const long i = i0 + q * 256 + tid;
    if (i < n) s += (double)g[i] * (double)g[i];
  }
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(256) ft_norm_kernel(const double* __restrict__ part, int chunks,
                                                      const FtHyper* __restrict__ hy, const int64_t* __restrict__ step,
                                                      const float* __restrict__ mslots, FtScalars* __restrict__ sc,
                                                      float* __restrict__ slots, float* __restrict__ out_slots) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int q = tid; q < chunks; q += 256) s += part[q];
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid != 0) return;
  const double norm = sqrt(red[0]);
  const double mx = hy->max_norm;
  const double coef = mx > 0.0 ? fmin(1.0, mx / (norm + 1e-6)) : 1.0;
  const double t = (double)(*step + 1);
  sc->norm = (float)norm;
  sc->coef = (float)coef;
  sc->bc1 = (float)(1.0 - pow(0.9, t));
  sc->sqrt_bc2 = (float)sqrt(1.0 - pow(0.999, t));
  float v[M2S_FT_SLOTS];
  for (int q = 0; q < 6; ++q) v[q] = mslots[q];
  // LOSS from the device coefficients (the metrics launch carries the host's copy of them as kernel arguments)
  v[M2S_MET_LOSS] = (float)((double)v[M2S_MET_MSE] + (double)hy->coeff[0] * v[M2S_MET_DELTA] +
                            (double)hy->coeff[1] * v[M2S_MET_ACCEL] + (double)hy->coeff[2] * v[M2S_MET_LATEST]);
  v[6] = (float)norm;
  v[7] = (float)coef;
  for (int q = 0; q < M2S_FT_SLOTS; ++q) {
    slots[q] = v[q];
    if (out_slots) out_slots[q] = v[q];
  }
}

// torch.optim.AdamW (single-tensor form): p *= 1 - lr wd; m, v; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
__global__ void __launch_bounds__(256) ft_adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, long n,
                                                       const FtHyper* __restrict__ hy,
                                                       const FtScalars* __restrict__ sc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float lr = hy->lr, wd = hy->wd, coef = sc->coef;
  // 1 - beta as torch forms them: in double, then rounded (1.f - 0.999f is 2e-6 off 0.001)
  const float b2 = 0.999f, omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999), eps = 1e-8f;
  const float gi = g[i] * coef;
  float w = p[i];
  w *= 1.f - lr * wd;
  const float mi = m[i] + (gi - m[i]) * omb1;  // lerp, as torch's exp_avg.lerp_
  const float vi = b2 * v[i] + omb2 * gi * gi;
  const float denom = sqrtf(vi) / sc->sqrt_bc2 + eps;
  w -= (lr / sc->bc1) * (mi / denom);
  p[i] = w;
  m[i] = mi;
  v[i] = vi;
}

__global__ void ft_step_inc_kernel(int64_t* step) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *step = *step + 1;
}

}  // namespace

void launch_ft_gather(const float* target, const float* mask, const int* win, int P, int W, int M, float* tgt,
                      float* msk, hipStream_t s) {
  ProfScope ps("ft_gather_kernel", 0.0, 4.0 * 2.0 * P * W * (M + 1), s);
  hipLaunchKernelGGL(ft_gather_kernel, dim3(blocks_of((long)P * W * M)), dim3(256), 0, s, target, mask, win, P, W, M,
                     tgt, msk);
  M2S_HIP(hipGetLastError());
}

void launch_ft_denominators(const float* msk, const FtHyper* hy, int P, int W, int M, FtScalars* sc, hipStream_t s) {
  ProfScope ps("ft_denominators_kernel", 0.0, 4.0 * P * W, s);
  hipLaunchKernelGGL(ft_denominators_kernel, dim3(1), dim3(256), 0, s, msk, hy, P, W, M, sc);
  M2S_HIP(hipGetLastError());
}

void launch_ft_criterion_grad(const float* pred, const float* tgt, const float* msk, const FtHyper* hy,
                              const FtScalars* sc, int P, int W, int M, float* dpred, hipStream_t s) {
  ProfScope ps("ft_criterion_grad_kernel", 0.0, 4.0 * 3.0 * P * W * M, s);
  hipLaunchKernelGGL(ft_criterion_grad_kernel, dim3(blocks_of((long)P * M)), dim3(256), 0, s, pred, tgt, msk, hy, sc, P,
                     W, M, dpred);
  M2S_HIP(hipGetLastError());
}

int ft_norm_chunks(long n) { return (int)((n + NORM_CHUNK - 1) / NORM_CHUNK); }

void launch_ft_sumsq(const float* g, long n, double* part, hipStream_t s) {
  ProfScope ps("ft_sumsq_kernel", 2.0 * n, 4.0 * n, s);
  hipLaunchKernelGGL(ft_sumsq_kernel, dim3(ft_norm_chunks(n)), dim3(256), 0, s, g, n, part);
  M2S_HIP(hipGetLastError());
}

void launch_ft_norm(const double* part, int chunks, const FtHyper* hy, const int64_t* step, const float* mslots,
                    FtScalars* sc, float* slots, float* out_slots, hipStream_t s) {
  ProfScope ps("ft_norm_kernel", 0.0, 8.0 * chunks, s);
  hipLaunchKernelGGL(ft_norm_kernel, dim3(1), dim3(256), 0, s, part, chunks, hy, step, mslots, sc, slots, out_slots);
  M2S_HIP(hipGetLastError());
}

void launch_ft_adamw(float* p, const float* g, float* m, float* v, long n, const FtHyper* hy, const FtScalars* sc,
                     hipStream_t s) {
  ProfScope ps("ft_adamw_kernel", 12.0 * n, 4.0 * 7.0 * n, s);
  hipLaunchKernelGGL(ft_adamw_kernel, dim3(blocks_of(n)), dim3(256), 0, s, p, g, m, v, n, hy, sc);
  M2S_HIP(hipGetLastError());
}

void launch_ft_step_inc(int64_t* step, hipStream_t s) {
  ProfScope ps("ft_step_inc_kernel", 0.0, 16.0, s);
  hipLaunchKernelGGL(ft_step_inc_kernel, dim3(1), dim3(64), 0, s, step);
  M2S_HIP(hipGetLastError());
}

}  // namespace m2s
