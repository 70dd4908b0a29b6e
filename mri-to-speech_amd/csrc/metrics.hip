// Fused validation metrics (include/m2s.h "fused mel metrics"): the weighted MaskedMSEMAE criterion
// and band MAEs of the reference trainer's validate(), eval_mel.py's masked MSE / MAE and its MCD-like, for one
// batch of (B, T, M) predictions in two launches.
//
// mel_metrics_seq_kernel: one workgroup of 256 threads per sequence.  Sweep 1: lane i takes the elements
// e = i, i + 256, ... of the sequence's T x M block (e = t M + m) and keeps one fp32 accumulator per sum, so a lane
// holds ceil(T M / 256) terms; the 256 lanes are then added in a binary tree of depth 8 in LDS, in a fixed order.
// The differences are formed in double from the fp32 inputs (exact) and rounded once, so the first and second time
// differences carry one rounding each whatever cancels; a term is fmaf(value^2, weight, acc).  The denominators
// factor into sum(freq_w) x a sum over rows, which the same sweep collects.  Sweep 1 also finds the two maxima of the
// MCD-like's top_db floor; sweep 2 (cache hits) runs the DCT of x'_pred - x'_tgt row by row against a table of
// cos(pi j / 2M), j < 4M, built once per workgroup from double.  The sequence's MET_PART partials go to the
// workspace: nothing is shared between workgroups, so a sequence's numbers do not depend on the batch.
//
// mel_metrics_group_kernel: one workgroup.  32 lanes per group add the group's partials in ascending sequence order in
// double; lane 0 of the group forms the quotients and adds them to its running totals; the eight group lanes are
// added in ascending order at the end.  out = this call, acc += this call.  No atomics, no waits.
#include <cmath>

#include "../../include/m2s.h"
#include "kernels.hpp"
#include "prof.hpp"

namespace m2s {
namespace {

constexpr int MT = 256;        // threads of either kernel
constexpr int MET_NV = 20;     // tree-reduced sums of sweep 1
constexpr int MET_MAXM = 256;  // mel bins
constexpr int MET_MAXK = 64;   // MCD-like coefficients
constexpr int MET_ROWS = 4;    // rows per DCT pass (MET_ROWS * MET_MAXK work items = one per thread)

// partial-sum slots of one sequence (MET_PART floats)
enum {
  P_MSE = 0, P_MAE, P_DELTA, P_ACCEL, P_LATEST, P_ESQ, P_EABS,  // numerators
  P_SFW, P_ST, P_SD, P_SA, P_SM,                                  // sum freq_w; row sums of the four denominators
  P_BAND = 12,                                                    // 8 band |diff| sums
  P_MCD = 20,                                                     // the sequence's MCD-like, NaN where skipped
};

struct SeqArgs {
  const float *pred, *target, *mask;
  int T, M;
  const float *freq_w, *time_w;
  int bands[16], n_bands;
  const float *mean, *sd;
  int n_mfcc;
  float *per_seq, *part;
};

__global__ void __launch_bounds__(MT) mel_metrics_seq_kernel(const SeqArgs a) {
  __shared__ float red[MET_NV][MT];
  __shared__ float mx[2][MT];
  __shared__ float costab[4 * MET_MAXM];
  __shared__ float dlt[MET_ROWS][MET_MAXM];
  __shared__ float csq[MET_ROWS][MET_MAXK];
  __shared__ float rowacc[MET_ROWS];
  __shared__ int nrows_s;
  const int b = blockIdx.x, tid = threadIdx.x, T = a.T, M = a.M;
  const float* pr = a.pred + (long)b * T * M;
  const float* tg = a.target + (long)b * T * M;
  const float* mk = a.mask ? a.mask + (long)b * T : nullptr;
  const bool mcd = a.mean != nullptr;

  float acc[MET_NV];
#pragma unroll
  for (int v = 0; v < MET_NV; ++v) acc[v] = 0.f;
  float maxp = -INFINITY, maxt = -INFINITY;
  int nrows = 0;
  for (long e = tid; e < (long)T * M; e += MT) {
    const int t = (int)(e / M), m = (int)(e - (long)t * M);
    const double d1 = (double)pr[e] - (double)tg[e];
    const float d = (float)d1, fw = a.freq_w[m], tw = a.time_w[t];
    const float m1 = mk ? mk[t] : 1.f;
    const float rw = tw * m1;
    const float w = fw * rw;
    acc[P_MSE] = fmaf(d * d, w, acc[P_MSE]);
    acc[P_MAE] = fmaf(fabsf(d), w, acc[P_MAE]);
    const float ev = d * m1;
    acc[P_ESQ] = fmaf(ev, ev, acc[P_ESQ]);
    acc[P_EABS] += fabsf(ev);
    if (t == 0) acc[P_SFW] += fw;
    if (m == 0) {
      acc[P_ST] += rw;
      acc[P_SM] += m1;
      nrows += m1 != 0.f ? 1 : 0;
    }
    if (t >= 1) {
      const double d0 = (double)pr[e - M] - (double)tg[e - M];
      const float m0 = mk ? mk[t - 1] : 1.f;
      const float dl = (float)(d1 - d0);
      const float rwd = (float)((double)tw * m1 * m0);  // the later row's time weight
      acc[P_DELTA] = fmaf(dl * dl, fw * rwd, acc[P_DELTA]);
      if (m == 0) acc[P_SD] += rwd;
      if (t + 1 < T) {
        const double d2 = (double)pr[e + M] - (double)tg[e + M];
        const float m2 = mk ? mk[t + 1] : 1.f;
        const float ac = (float)(d2 - 2.0 * d1 + d0);
        const float rwa = (float)((double)tw * m2 * m1 * m0);  // the middle row's time weight
        acc[P_ACCEL] = fmaf(ac * ac, fw * rwa, acc[P_ACCEL]);
        if (m == 0) acc[P_SA] += rwa;
      }
    }
    if (t == T - 1) acc[P_LATEST] = fmaf(d * d, fw, acc[P_LATEST]);  // unmasked, no time weight
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < a.n_bands && m >= a.bands[2 * k] && m < a.bands[2 * k + 1]) acc[P_BAND + k] += fabsf(d);  // unmasked
    if (mcd && m1 != 0.f) {
      maxp = fmaxf(maxp, fmaxf(fmaf(pr[e], a.sd[m], a.mean[m]), -100.f));
      maxt = fmaxf(maxt, fmaxf(fmaf(tg[e], a.sd[m], a.mean[m]), -100.f));
    }
  }
  // ---- the 256 lanes of every sum: binary tree, depth 8, fixed order ----------------------------------------
#pragma unroll
  for (int v = 0; v < MET_NV; ++v) red[v][tid] = acc[v];
  mx[0][tid] = maxp;
  mx[1][tid] = maxt;
  if (tid == 0) nrows_s = 0;
  if (tid < MET_ROWS) rowacc[tid] = 0.f;
  if (mcd)
    for (int j = tid; j < 4 * M; j += MT) costab[j] = (float)cos(M_PI * (double)j / (double)(2 * M));
  __syncthreads();
  for (int st = MT / 2; st > 0; st >>= 1) {
    if (tid < st) {
#pragma unroll
      for (int v = 0; v < MET_NV; ++v) red[v][tid] += red[v][tid + st];
      mx[0][tid] = fmaxf(mx[0][tid], mx[0][tid + st]);
      mx[1][tid] = fmaxf(mx[1][tid], mx[1][tid + st]);
    }
    __syncthreads();
  }
  if (nrows) atomicAdd(&nrows_s, nrows);  // an integer count in LDS: exact in any order
  float* part = a.part + (long)b * MET_PART;
  if (tid < MET_NV) part[tid] = red[tid][0];
  if (tid > MET_NV && tid < MET_PART) part[tid] = 0.f;
  __syncthreads();

  // ---- MCD-like: the rows with mask != 0, MET_ROWS at a time --------------------------------------------------
  float value = NAN;
  if (mcd && nrows_s > 0) {
    const float florp = mx[0][0] - 80.f, flort = mx[1][0] - 80.f;  // top_db, separately for pred and target
    const int K = a.n_mfcc;
    const float s0 = (float)sqrt(1.0 / M), sk = (float)sqrt(2.0 / M);
    float mine = 0.f;  // thread r < MET_ROWS: the norms of rows r, r + MET_ROWS, ...
    for (int t0 = 0; t0 < T; t0 += MET_ROWS) {
      for (int i = tid; i < MET_ROWS * M; i += MT) {
        const int r = i / M, m = i - r * M, t = t0 + r;
        float v = 0.f;
        if (t < T && (mk ? mk[t] : 1.f) != 0.f) {
          const float xp = fmaxf(fmaxf(fmaf(pr[(long)t * M + m], a.sd[m], a.mean[m]), -100.f), florp);
          const float xt = fmaxf(fmaxf(fmaf(tg[(long)t * M + m], a.sd[m], a.mean[m]), -100.f), flort);
          v = xp - xt;
        }
        dlt[r][m] = v;
      }
      __syncthreads();
      {
        const int r = tid / MET_MAXK, k = tid - r * MET_MAXK;
        if (k < K) {
          float c = 0.f;
          int j = k;  // k (2m + 1) mod 4M
          for (int m = 0; m < M; ++m) {
            c = fmaf(dlt[r][m], costab[j], c);
            j += 2 * k;
            if (j >= 4 * M) j -= 4 * M;
          }
          c *= k == 0 ? s0 : sk;
          csq[r][k] = c * c;
        }
      }
      __syncthreads();
      if (tid < MET_ROWS && t0 + tid < T && (mk ? mk[t0 + tid] : 1.f) != 0.f) {
        float q = 0.f;
        for (int k = 0; k < K; ++k) q += csq[tid][k];
        mine += sqrtf(q);
      }
      // dlt and csq are rewritten only after the next pass's first barrier / this loop's barriers
      __syncthreads();
    }
    if (tid < MET_ROWS) rowacc[tid] = mine;
    __syncthreads();
    const float sum = (rowacc[0] + rowacc[1]) + (rowacc[2] + rowacc[3]);
    const float v = (float)(10.0 / M_LN10 * M_SQRT2) * (sum / (float)nrows_s);
    if (isfinite(v)) value = v;
  }
  if (tid == 0) {
    part[P_MCD] = value;
    if (a.per_seq) {
      a.per_seq[(long)b * 3 + 0] = red[P_ESQ][0];
      a.per_seq[(long)b * 3 + 1] = red[P_EABS][0];
      a.per_seq[(long)b * 3 + 2] = value;
    }
  }
}

struct GroupArgs {
  const float* part;
  int B, T, M, group;
  float coeff[3];
  int bands[16], n_bands;
  double* acc;
  float* out;
};

__global__ void __launch_bounds__(MT) mel_metrics_group_kernel(const GroupArgs a) {
  constexpr int GL = MT / MET_PART;  // groups per pass (8)
  __shared__ double sums[GL][MET_PART];
  __shared__ double tot[GL][M2S_METRICS_SLOTS];
  const int tid = threadIdx.x, gl = tid / MET_PART, v = tid % MET_PART;
  const int ngroups = (a.B + a.group - 1) / a.group;
  double mine[M2S_METRICS_SLOTS];
#pragma unroll
  for (int i = 0; i < M2S_METRICS_SLOTS; ++i) mine[i] = 0.0;
  for (int g0 = 0; g0 < ngroups; g0 += GL) {
    const int g = g0 + gl;
    const int b0 = g * a.group, b1 = min(a.B, b0 + a.group);
    double s = 0.0;
    if (g < ngroups) {
      if (v == P_MCD) {  // the finite values' sum
        for (int b = b0; b < b1; ++b) {
          const float x = a.part[(long)b * MET_PART + P_MCD];
          if (x == x) s += (double)x;
        }
      } else if (v == P_MCD + 1) {  // ... and their count
        for (int b = b0; b < b1; ++b) {
          const float x = a.part[(long)b * MET_PART + P_MCD];
          if (x == x) s += 1.0;
        }
      } else if (v == P_SFW) {  // the same for every sequence
        s = (double)a.part[(long)b0 * MET_PART + P_SFW];
      } else {
        for (int b = b0; b < b1; ++b) s += (double)a.part[(long)b * MET_PART + v];  // ascending sequence order
      }
    }
    sums[gl][v] = s;
    __syncthreads();
    if (v == 0 && g < ngroups) {
      const double* S = sums[gl];
      const double n = (double)(b1 - b0), sfw = S[P_SFW];
      const double den = fmax(sfw * S[P_ST], 1e-6);
      const double mse = S[P_MSE] / den, mae = S[P_MAE] / den;
      const double delta = a.T > 1 ? S[P_DELTA] / fmax(sfw * S[P_SD], 1e-6) : 0.0;
      const double accel = a.T > 2 ? S[P_ACCEL] / fmax(sfw * S[P_SA], 1e-6) : 0.0;
      const double latest = S[P_LATEST] / fmax(n * sfw, 1e-6);
      mine[M2S_MET_LOSS] += mse + (double)a.coeff[0] * delta + (double)a.coeff[1] * accel + (double)a.coeff[2] * latest;
      mine[M2S_MET_MSE] += mse;
      mine[M2S_MET_MAE] += mae;
      mine[M2S_MET_DELTA] += delta;
      mine[M2S_MET_ACCEL] += accel;
      mine[M2S_MET_LATEST] += latest;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int width = k < a.n_bands ? min(a.bands[2 * k + 1], a.M) - a.bands[2 * k] : 0;
        if (width > 0) mine[M2S_MET_BAND0 + k] += S[P_BAND + k] / (n * a.T * width);
      }
      const double eden = fmax(S[P_SM], 1.0);
      const double emse = S[P_ESQ] / eden, emae = S[P_EABS] / eden;
      mine[M2S_MET_EVAL_LOSS] += 0.8 * emse + 0.2 * emae;
      mine[M2S_MET_EVAL_MSE] += emse;
      mine[M2S_MET_EVAL_MAE] += emae;
      mine[M2S_MET_GROUPS] += 1.0;
      mine[M2S_MET_MCD_SUM] += S[P_MCD];
      mine[M2S_MET_MCD_COUNT] += S[P_MCD + 1];
    }
    __syncthreads();
  }
  if (v == 0) {
#pragma unroll
    for (int i = 0; i < M2S_METRICS_SLOTS; ++i) tot[gl][i] = mine[i];
  }
  __syncthreads();
  if (tid < M2S_METRICS_SLOTS) {
    double s = 0.0;
    for (int q = 0; q < GL; ++q) s += tot[q][tid];
    if (a.out) a.out[tid] = (float)s;
    if (a.acc) a.acc[tid] += s;
  }
}

}  // namespace

void launch_mel_metrics(const MelMetricsArgs& m, hipStream_t s) {
  M2S_CHECK(m.B >= 1 && m.T >= 1 && m.M >= 1 && m.M <= MET_MAXM && (double)m.T * m.M <= 2147483647.0,
            "mel_metrics: shape");
  M2S_CHECK(m.n_bands >= 0 && m.n_bands <= 8 && m.n_mfcc <= MET_MAXK, "mel_metrics: bands / n_mfcc");
  static_assert(MET_PART == 32 && P_MCD + 2 <= MET_PART && MT / MET_MAXK == MET_ROWS, "metrics geometry");
  SeqArgs a{};
  a.pred = m.pred, a.target = m.target, a.mask = m.mask;
  a.T = m.T, a.M = m.M;
  a.freq_w = m.freq_w, a.time_w = m.time_w;
  a.n_bands = m.n_bands;
  a.mean = m.mean, a.sd = m.sd, a.n_mfcc = m.n_mfcc;
  a.per_seq = m.per_seq, a.part = m.part;
  GroupArgs g{};
  g.part = m.part;
  g.B = m.B, g.T = m.T, g.M = m.M;
  g.group = m.group <= 0 || m.group >= m.B ? m.B : m.group;
  g.n_bands = m.n_bands;
  for (int i = 0; i < 16; ++i) a.bands[i] = g.bands[i] = i < 2 * m.n_bands ? m.bands[i] : 0;
  for (int i = 0; i < 3; ++i) g.coeff[i] = m.coeff[i];
  g.acc = m.acc, g.out = m.out;
  StageTag tag("metrics");
  const double elems = (double)m.B * m.T * m.M;
  {
    // two inputs read once (the neighbouring rows and the DCT sweep hit the cache), ~30 flops an element plus the DCT
    ProfScope ps("mel_metrics_seq_kernel", elems * (30.0 + (m.mean ? 2.0 * m.n_mfcc : 0.0)),
                 4.0 * (2.0 * elems + (double)m.B * (m.T + MET_PART + 3)), s);
    hipLaunchKernelGGL(mel_metrics_seq_kernel, dim3(m.B), dim3(MT), 0, s, a);
    M2S_HIP(hipGetLastError());
  }
  ProfScope ps("mel_metrics_group_kernel", (double)m.B * MET_PART, 4.0 * m.B * MET_PART + 12.0 * M2S_METRICS_SLOTS, s);
  hipLaunchKernelGGL(mel_metrics_group_kernel, dim3(1), dim3(MT), 0, s, g);
  M2S_HIP(hipGetLastError());
}

}  // namespace m2s
