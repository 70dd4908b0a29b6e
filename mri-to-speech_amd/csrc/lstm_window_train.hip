// Train-mode sliding-window BiLSTM and its backward through time (include/m2s.h "fine-tuning", DESIGN.md
// "Fine-tuning").  Like lstm_window.hip the recurrence of P independent windows of W <= 16 steps is a chain of
// throughput GEMMs, one launch per step, and step s + 1 follows step s by stream order alone: no flag, no spin loop,
// no cross-workgroup wait.  Every product runs on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) through one strided
// GEMM kernel; its K order is fixed by the tile geometry and split-K partials are added in ascending order, so a
// step is bit-reproducible.  There are no floating-point atomics.
//
// Saved activations: post-activation gates [dir][W][P][4 x 640] (torch's gate order i, f, g, o), cells and h
// [dir][W][P][640], indexed by the direction's LOCAL step (the reverse direction's local step s is frame W - 1 - s of
// the window).  With that layout the steps 1 .. W - 1 of dgates and the steps 0 .. W - 2 of h are each one contiguous
// (P (W - 1)) x N matrix: dW_hh is a single GEMM over K = P (W - 1).
// The gate activations are libm's expf and tanhf (not the rcp-based ones of the inference cell): the backward
// multiplies by 1 - tanh^2 and s (1 - s) of the SAVED values, and the gradient bars are set against float64.
#include <algorithm>

#include "finetune.hpp"
#include "prof.hpp"

namespace m2s {
namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int GT = 64;   // tile edge (M and N)
constexpr int GK = 16;   // K step
constexpr int GLD = 65;  // LDS row stride

struct GemmK {
  const float *A, *B;
  float* C;
  int M, N, K;
  long a_m, a_k, b_k, b_n, ldc, sA, sB, sC;
  const float *bias0, *bias1;
  long sBias;
  int splits, kchunk;
  float* part;
};

__global__ void __launch_bounds__(256) ft_gemm_kernel(const GemmK g) {
  __shared__ float As[GK][GLD];
  __shared__ float Bs[GK][GLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, l32 = lane & 31, wm = wave & 1, wn = wave >> 1;
  const int z = blockIdx.z / g.splits, sp = blockIdx.z - z * g.splits;
  const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
  const int kbeg = g.splits > 1 ? sp * g.kchunk : 0;
  const int kend = g.splits > 1 ? min(g.K, kbeg + g.kchunk) : g.K;
  const float* A = g.A + (long)z * g.sA;
  const float* B = g.B + (long)z * g.sB;
  const bool a_kfast = g.a_k == 1, b_kfast = g.b_k == 1;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int k0 = kbeg; k0 < kend; k0 += GK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i;
      {
        const int k = a_kfast ? e % GK : e / GT, m = a_kfast ? e / GK : e % GT;
        const int gm = m0 + m, gk = k0 + k;
        As[k][m] = gm < g.M && gk < kend ? A[(long)gm * g.a_m + (long)gk * g.a_k] : 0.f;
      }
      {
        const int k = b_kfast ? e % GK : e / GT, n = b_kfast ? e / GK : e % GT;
        const int gn = n0 + n, gk = k0 + k;
        Bs[k][n] = gn < g.N && gk < kend ? B[(long)gk * g.b_k + (long)gn * g.b_n] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < GK / 2; ++s)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * s + hh][32 * wm + l32], Bs[2 * s + hh][32 * wn + l32], acc, 0, 0,
                                                 0);
    __syncthreads();
  }
  // acc[i]: row 32 wm + 8 (i / 4) + 4 hh + i % 4, column 32 wn + l32
  const int col = n0 + 32 * wn + l32;
  if (col >= g.N) return;
  float bias = 0.f;
  if (g.bias0) bias = g.bias0[(long)z * g.sBias + col];
  if (g.bias1) bias += g.bias1[(long)z * g.sBias + col];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = m0 + 32 * wm + 8 * (i / 4) + 4 * hh + (i % 4);
    if (row >= g.M) continue;
    if (g.splits > 1)
      g.part[((long)blockIdx.z * g.M + row) * g.N + col] = acc[i];
    else
      g.C[(long)z * g.sC + (long)row * g.ldc + col] = acc[i] + bias;
  }
}

// the split-K partials of every batch, added in ascending split order
__global__ void __launch_bounds__(256) ft_gemm_reduce_kernel(const float* __restrict__ part, int M, int N, int splits,
                                                             long ldc, long sC, float* __restrict__ C) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)M * N) return;
  const int z = blockIdx.y;
  const int row = (int)(i / N), col = (int)(i - (long)row * N);
  float s = 0.f;
  for (int q = 0; q < splits; ++q) s += part[((long)z * splits + q) * M * N + i];
  C[(long)z * sC + (long)row * ldc + col] = s;
}

__device__ __forceinline__ float ft_sig(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ void __launch_bounds__(256) ft_cell_forward_kernel(const float* __restrict__ pre, const int* __restrict__ win,
                                                              int P, int W, int st, const float* __restrict__ rec,
                                                              float* __restrict__ gates, float* __restrict__ c,
                                                              float* __restrict__ h) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)P * FT_H) return;
  const int p = (int)(i / FT_H), u = (int)(i - (long)p * FT_H), dir = blockIdx.y;
  const long row = win[p] + (dir == 0 ? st : W - 1 - st);
  const float* pr = pre + row * 2 * FT_G + (long)dir * FT_G + u;
  float x[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) x[q] = pr[q * FT_H];
  if (st > 0) {
    const float* rr = rec + ((long)dir * P + p) * FT_G + u;
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] += rr[q * FT_H];
  }
  const float gi = ft_sig(x[0]), gf = ft_sig(x[1]), gg = tanhf(x[2]), go = ft_sig(x[3]);
  const long o = (((long)dir * W + st) * P + p) * FT_H + u;
  float cc = gi * gg;
  if (st > 0) cc += gf * c[o - (long)P * FT_H];
  float* gt = gates + (((long)dir * W + st) * P + p) * FT_G + u;
  gt[0] = gi, gt[FT_H] = gf, gt[2 * FT_H] = gg, gt[3 * FT_H] = go;
  c[o] = cc;
  h[o] = go * tanhf(cc);
}

// the dropout stream (DESIGN.md "Fine-tuning"): element e of (P, W, 640), seed, optimiser step t -> 32 bits
__device__ __forceinline__ uint32_t ft_mix(unsigned long long e, uint32_t seed, uint32_t t) {
  uint32_t x = (uint32_t)e * 0x9E3779B1u + (uint32_t)(e >> 32) * 0x27D4EB2Fu + seed * 0x85EBCA77u + t * 0xC2B2AE3Du;
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

__global__ void __launch_bounds__(256) ft_merge_dropout_kernel(const float* __restrict__ h,
                                                               const FtHyper* __restrict__ hy,
                                                               const int64_t* __restrict__ step, int P, int W, int train,
                                                               float* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)P * W * FT_H) return;
  const int u = (int)(i % FT_H);
  const long ps = i / FT_H;
  const int s = (int)(ps % W), p = (int)(ps / W);
  float v = h[((long)s * P + p) * FT_H + u] + h[(((long)W + (W - 1 - s)) * P + p) * FT_H + u];
  const uint32_t thr = train ? hy->drop_thr : 0u;
  if (thr != 0u) {  // p = 0: every element kept exactly, no multiply
    const uint32_t t = (uint32_t)(*step + 1);
    v = ft_mix((unsigned long long)i, hy->seed, t) >= thr ? v * hy->drop_scale : 0.f;
  }
  y[i] = v;
}

__global__ void __launch_bounds__(256) ft_cell_backward_kernel(const float* __restrict__ dy,
                                                               const FtHyper* __restrict__ hy,
                                                               const int64_t* __restrict__ step,
                                                               const float* __restrict__ dhrec,
                                                               const float* __restrict__ gates,
                                                               const float* __restrict__ c, int P, int W, int st,
                                                               float* __restrict__ dcn, float* __restrict__ dgates) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)P * FT_H) return;
  const int p = (int)(i / FT_H), u = (int)(i - (long)p * FT_H), dir = blockIdx.y;
  const int frame = dir == 0 ? st : W - 1 - st;
  const long e = ((long)p * W + frame) * FT_H + u;
  float dh = dy[e];
  const uint32_t thr = hy->drop_thr;
  if (thr != 0u) dh = ft_mix((unsigned long long)e, hy->seed, (uint32_t)(*step + 1)) >= thr ? dh * hy->drop_scale : 0.f;
  const long carry = ((long)dir * P + p) * FT_H + u;
  if (st < W - 1) dh += dhrec[carry];
  const long o = (((long)dir * W + st) * P + p) * FT_H + u;
  const float* gt = gates + (((long)dir * W + st) * P + p) * FT_G + u;
  const float gi = gt[0], gf = gt[FT_H], gg = gt[2 * FT_H], go = gt[3 * FT_H];
  const float tc = tanhf(c[o]);
  float dc = dh * go * (1.f - tc * tc);
  if (st < W - 1) dc += dcn[carry];
  const float cprev = st > 0 ? c[o - (long)P * FT_H] : 0.f;
  float* dg = dgates + (((long)dir * W + st) * P + p) * FT_G + u;
  dg[0] = dc * gg * gi * (1.f - gi);
  dg[FT_H] = st > 0 ? dc * cprev * gf * (1.f - gf) : 0.f;
  dg[2 * FT_H] = dc * gi * (1.f - gg * gg);
  dg[3 * FT_H] = dh * tc * go * (1.f - go);
  dcn[carry] = dc * gf;
}

// rowtab = [rowp: rows | lo: rows | hi: rows]: frame row r is local frame s of window rowp[r] - s where lo <= that < hi
__global__ void __launch_bounds__(256) ft_fold_kernel(const float* __restrict__ dgates, const int* __restrict__ rowtab,
                                                      int rows, int P, int W, float* __restrict__ dpre) {
  const int r = blockIdx.x, dir = blockIdx.y;
  const int rp = rowtab[r], lo = rowtab[rows + r], hi = rowtab[2 * rows + r];
  for (int n = threadIdx.x; n < FT_G; n += 256) {
    float acc = 0.f;
    for (int s = 0; s < W; ++s) {  // ascending s: a fixed order
      const int p = rp - s;
      if (p < lo || p >= hi) continue;
      const int ls = dir == 0 ? s : W - 1 - s;
      acc += dgates[(((long)dir * W + ls) * P + p) * FT_G + n];
    }
    dpre[(long)r * 2 * FT_G + (long)dir * FT_G + n] = acc;
  }
}

constexpr int CS_ROWS = 1024;
__global__ void __launch_bounds__(256) ft_colsum_kernel(const float* __restrict__ x, long R, int C,
                                                        double* __restrict__ part) {
  __shared__ double red[4][64];
  const int cl = threadIdx.x & 63, rq = threadIdx.x >> 6, col = blockIdx.x * 64 + cl;
  const long r0 = (long)blockIdx.y * CS_ROWS, r1 = min(R, r0 + CS_ROWS);
  double s = 0.0;
  if (col < C)
    for (long r = r0 + rq; r < r1; r += 4) s += (double)x[r * C + col];
  red[rq][cl] = s;
  __syncthreads();
  if (rq == 0 && col < C) part[(long)blockIdx.y * C + col] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}
__global__ void __launch_bounds__(256) ft_colsum_final_kernel(const double* __restrict__ part, int chunks, int C,
                                                              float* __restrict__ out0, float* __restrict__ out1) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= C) return;
  double s = 0.0;
  for (int q = 0; q < chunks; ++q) s += part[(long)q * C + col];
  out0[col] = (float)s;
  if (out1) out1[col] = (float)s;
}

unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void ft_split(int K, int* splits, int* kchunk) {
  const int s = std::max(1, std::min(16, (K + 63) / 64));
  const int kc = (((K + s - 1) / s) + GK - 1) / GK * GK;
  *splits = (K + kc - 1) / kc;
  *kchunk = kc;
}

void launch_ft_gemm(const FtGemm& f, const char* name, hipStream_t s) {
  M2S_CHECK(f.M >= 1 && f.N >= 1 && f.K >= 1 && f.batch >= 1 && f.splits >= 1, "ft_gemm: shape");
  M2S_CHECK(f.splits == 1 || (f.part && !f.bias0 && !f.bias1 && f.kchunk % GK == 0 &&
                              (long)f.kchunk * (f.splits - 1) < f.K && (long)f.kchunk * f.splits >= f.K),
            "ft_gemm: split-K partition");
  GemmK g{f.A, f.B, f.C, f.M, f.N, f.K, f.a_m, f.a_k, f.b_k, f.b_n, f.ldc, f.sA, f.sB, f.sC,
          f.bias0, f.bias1, f.sBias, f.splits, f.kchunk, f.part};
  const dim3 grid((f.N + GT - 1) / GT, (f.M + GT - 1) / GT, f.batch * f.splits);
  M2S_CHECK(grid.y <= 65535 && grid.z <= 65535, "ft_gemm: grid");
  {
    ProfScope ps(name, 2.0 * f.batch * f.M * f.N * f.K, 4.0 * f.batch * ((double)f.M * f.K + (double)f.K * f.N + (double)f.M * f.N), s);
    hipLaunchKernelGGL(ft_gemm_kernel, grid, dim3(256), 0, s, g);
    M2S_HIP(hipGetLastError());
  }
  if (f.splits > 1) {
    ProfScope ps("ft_gemm_reduce_kernel", (double)f.batch * f.splits * f.M * f.N, 4.0 * f.batch * (f.splits + 1.0) * f.M * f.N, s);
    hipLaunchKernelGGL(ft_gemm_reduce_kernel, dim3(blocks_of((long)f.M * f.N), f.batch), dim3(256), 0, s, f.part, f.M,
                       f.N, f.splits, f.ldc, f.sC, f.C);
    M2S_HIP(hipGetLastError());
  }
}

void launch_ft_cell_forward(const float* pre, const int* win, int P, int W, int st, const float* rec, float* gates,
                            float* c, float* h, hipStream_t s) {
  ProfScope ps("ft_cell_forward_kernel", 0.0, 4.0 * 2 * P * FT_H * 15.0, s);
  hipLaunchKernelGGL(ft_cell_forward_kernel, dim3(blocks_of((long)P * FT_H), 2), dim3(256), 0, s, pre, win, P, W, st, rec,
                     gates, c, h);
  M2S_HIP(hipGetLastError());
}

void launch_ft_cell_backward(const float* dy, const FtHyper* hy, const int64_t* step, const float* dhrec,
                             const float* gates, const float* c, int P, int W, int st, float* dcn, float* dgates,
                             hipStream_t s) {
  ProfScope ps("ft_cell_backward_kernel", 0.0, 4.0 * 2 * P * FT_H * 14.0, s);
  hipLaunchKernelGGL(ft_cell_backward_kernel, dim3(blocks_of((long)P * FT_H), 2), dim3(256), 0, s, dy, hy, step, dhrec,
                     gates, c, P, W, st, dcn, dgates);
  M2S_HIP(hipGetLastError());
}

void launch_ft_merge_dropout(const float* h, const FtHyper* hy, const int64_t* step, int P, int W, bool train, float* y,
                             hipStream_t s) {
  ProfScope ps("ft_merge_dropout_kernel", 0.0, 4.0 * 3.0 * P * W * FT_H, s);
  hipLaunchKernelGGL(ft_merge_dropout_kernel, dim3(blocks_of((long)P * W * FT_H)), dim3(256), 0, s, h, hy, step, P, W,
                     train ? 1 : 0, y);
  M2S_HIP(hipGetLastError());
}

void launch_ft_fold(const float* dgates, const int* rowtab, int rows, int P, int W, float* dpre, hipStream_t s) {
  ProfScope ps("ft_fold_kernel", 0.0, 4.0 * 2 * FT_G * ((double)P * W + rows), s);
  hipLaunchKernelGGL(ft_fold_kernel, dim3(rows, 2), dim3(256), 0, s, dgates, rowtab, rows, P, W, dpre);
  M2S_HIP(hipGetLastError());
}

int ft_colsum_chunks(long R) { return (int)((R + CS_ROWS - 1) / CS_ROWS); }

void launch_ft_colsum(const float* x, long R, int C, double* part, float* out0, float* out1, hipStream_t s) {
  const int chunks = ft_colsum_chunks(R);
  M2S_CHECK(R >= 1 && C >= 1 && chunks <= 65535, "ft_colsum: shape");
  {
    ProfScope ps("ft_colsum_kernel", (double)R * C, 4.0 * R * C, s);
    hipLaunchKernelGGL(ft_colsum_kernel, dim3((C + 63) / 64, chunks), dim3(256), 0, s, x, R, C, part);
    M2S_HIP(hipGetLastError());
  }
  ProfScope ps("ft_colsum_final_kernel", (double)chunks * C, 8.0 * chunks * C, s);
  hipLaunchKernelGGL(ft_colsum_final_kernel, dim3((C + 255) / 256), dim3(256), 0, s, part, chunks, C, out0, out1);
  M2S_HIP(hipGetLastError());
}

}  // namespace m2s
