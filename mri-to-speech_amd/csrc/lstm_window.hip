// Sliding-window BiLSTM: thousands of independent sequences of at most W <= 16 steps (DESIGN.md "Windowed
// acoustic inference").  The opposite regime of lstm_persistent.hip: the recurrence is a chain of W - 1 throughput
// GEMMs, M = S windows, N = 4 x 640 gate columns, K = 640, one launch per step.  Step s + 1 follows step s by
// stream order alone: no flag, no tag, no spin loop, no co-residency requirement, nothing that can time out.
//
// Windows.  win[w] = {row0, k | delay << 8}: window w covers the packed projected rows row0 .. row0 + k - 1 and is
// active at the global steps j = delay .. delay + k - 1 (local step s = j - delay).  The forward direction reads row
// row0 + s, the reverse one row0 + k - 1 - s.  `latest` aligns every window at its END (delay = W - k), so the h of
// the window's last frame is what step W - 1 writes; a window still in its warm-up (s < 0) keeps h = c = 0 by
// predicate, and the zero state makes its first active GEMM step the step-0 cell exactly.  `mean` starts every
// window at step 0 (delay = 0) and keeps every step's h for the merge.
//
// Step 0 is elementwise (h = o tanh(i g), c = i g on one projected row).  Steps 1 .. W - 1: workgroup (ug, dir)
// holds the 64 W_hh rows of 16 hidden units x 4 gates (rows permuted at pack time: [dir][ug][gate x 16 + unit][640])
// as resident MFMA A fragments and walks 32-window tiles; its 8 waves split K (80 each), the partials are summed in
// LDS in a fixed order, and 512 threads run the cell update for (unit, window) pairs with the GATHERED projected
// row, fp32 c, the rcp-based sigmoid and tanh(x) = 2 sigmoid(2x) - 1 of the other recurrence kernels.  The next
// step's h is stored in the operand layout: fp32 [S][640] (exact-f32 v_mfma_f32_32x32x2_f32 products, the fp32
// engine) or split [S][hi 640 | lo 640] bf16 (W_hi h_lo + W_lo h_hi + W_hi h_hi, v_mfma_f32_32x32x16_bf16, fp32
// accumulation: lstm_x3_kernel's arithmetic; the bf16x3 / bf16 / fp8 engines).
// An output element is one dot product over its own window's h in a K order fixed by the tile geometry, so a row's
// bits do not depend on S, on the window's place in its tile or on what else is in the batch.
#include <algorithm>

#include "kernels.hpp"
#include "lstm_cell.hpp"

namespace m2s {
namespace {

constexpr int LW_H = LSTM_H;         // hidden size these kernels are built for
constexpr int LW_U = 16;             // units per workgroup (64 gate rows = two MFMA M tiles)
constexpr int LW_S = 32;             // windows per tile (one MFMA N tile)
constexpr int LW_W = 8;              // waves
constexpr int LW_KW = LW_H / LW_W;   // K slice per wave (80)
constexpr int LW_KS = LW_KW / 16;    // split: k-steps of 16 per wave (5)
constexpr int LW_KH = LW_KW / 2;     // fp32: floats per lane (k half = lane / 32)
constexpr int LW_G = LW_H / LW_U;    // unit groups per direction (40)

// clip table (host-staged): [off | len | ctx | wbase | obase], B ints each
__global__ void __launch_bounds__(256) lstm_window_table_kernel(const int* __restrict__ tab, int B, int W, int mean,
                                                                int2* __restrict__ win) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int off = tab[b], len = tab[B + b], ctx = tab[2 * B + b], wbase = tab[3 * B + b];
  if (mean) {
    const int k = min(len, W);
    if (i >= len - k + 1) return;
    win[wbase + i] = make_int2(off + i, k);
  } else {
    if (i >= len - ctx) return;
    const int t = ctx + i, k = min(W, t + 1);
    win[wbase + i] = make_int2(off + t - k + 1, k | ((W - k) << 8));
  }
}

// Step 0 of every window, both directions.  hop: the step-1 operand [dirs][S][..]; c: [dirs][S][640]; hf0 / hf1:
// fp32 h of the forward / reverse direction of this step (either may be null).  latest: the reverse direction is
// only this step, on the window's last frame, and goes to hf1 alone.
template <bool SPLIT>
__global__ void __launch_bounds__(256) lstm_window_step0_kernel(const float* __restrict__ pre,
                                                                const int2* __restrict__ win, int S, int latest,
                                                                void* hop, float* c, float* hf0, float* hf1) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)S * LW_H) return;
  const int w = (int)(i / LW_H), u = (int)(i - (long)w * LW_H), dir = blockIdx.y;
  const int2 e = win[w];
  const int k = e.y & 255, delay = e.y >> 8;
  const bool active = dir == 1 || delay == 0;
  float h = 0.f, cc = 0.f;
  if (active) {
    const float* pr = pre + (long)(dir == 0 ? e.x : e.x + k - 1) * 8 * LW_H + (long)dir * 4 * LW_H + u;
    const float gi = lstm_sig(pr[0]), gg = lstm_tanh(pr[2 * LW_H]), go = lstm_sig(pr[3 * LW_H]);
    cc = gi * gg;
    h = go * lstm_tanh(cc);
  }
  float* hf = dir == 0 ? hf0 : hf1;
  if (hf) hf[i] = h;
  if (dir == 1 && latest) return;
  if (!hop) return;  // W = 1: no recurrent step follows
  c[(long)dir * S * LW_H + i] = cc;
  if constexpr (SPLIT) {
    bf16_t* o = static_cast<bf16_t*>(hop) + ((long)dir * S + w) * 2 * LW_H + u;
    bf16_t hi, lo;
    lstm_split_h(h, hi, lo);
    o[0] = hi;
    o[LW_H] = lo;
  } else {
    static_cast<float*>(hop)[(long)dir * S * LW_H + i] = h;
  }
}

// One recurrent step j >= 1 of every window.  grid (tile walkers, 40 unit groups, dirs).
template <bool SPLIT>
__global__ void __launch_bounds__(64 * LW_W, 1) lstm_window_step_kernel(const float* __restrict__ pre,
                                                                         const float* __restrict__ wperm,
                                                                         const int2* __restrict__ win, int S, int j,
                                                                         const void* __restrict__ hin, void* hout,
                                                                         float* c, float* hf, long hf_dir_stride) {
  __shared__ float red[LW_W][2 * 32][LW_S + 1];
  const int dir = blockIdx.z, ug = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, l32 = lane & 31;
  const int kw = wave * LW_KW;
  const float* wg = wperm + ((size_t)dir * LW_G + ug) * 64 * LW_H;

  // ---- the workgroup's 64 W_hh rows -> resident A fragments (tile m, lane row 32 m + l32) -------------------
  bf16x8 whi[SPLIT ? 2 : 1][SPLIT ? LW_KS : 1], wlo[SPLIT ? 2 : 1][SPLIT ? LW_KS : 1];
  float wa[SPLIT ? 1 : 2][SPLIT ? 1 : LW_KH];
  if constexpr (SPLIT) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
      lstm_wfrag_split(wg + (size_t)(32 * m + l32) * LW_H + kw + 8 * hh, whi[m], wlo[m]);  // k = kw + 16 s + 8 hh + 0..7
  } else {
#pragma unroll
    for (int m = 0; m < 2; ++m)
      lstm_wfrag_f32(wg + (size_t)(32 * m + l32) * LW_H + kw + LW_KH * hh, wa[m]);  // k = kw + 40 hh + s
  }

  const int cu = tid % LW_U, cb = tid / LW_U;  // cell-update pair (unit, window of the tile) of this thread
  const int unit = ug * LW_U + cu;
  const int ntiles = (S + LW_S - 1) / LW_S;
  for (int mt = blockIdx.x; mt < ntiles; mt += gridDim.x) {
    // ---- this thread's window, its gathered gate pre-activations and cell state (latency under the MFMAs) -------
    const int wc = mt * LW_S + cb;
    bool live = wc < S, active = false;
    float prf[4] = {0.f, 0.f, 0.f, 0.f}, cprev = 0.f;
    if (live) {
      const int2 e = win[wc];
      const int k = e.y & 255, s = j - (e.y >> 8);
      active = s >= 0 && s < k;
      if (active) {
        const float* pr = pre + (long)(dir == 0 ? e.x + s : e.x + k - 1 - s) * 8 * LW_H + (long)dir * 4 * LW_H + unit;
#pragma unroll
        for (int q = 0; q < 4; ++q) prf[q] = pr[q * LW_H];
        cprev = c[((long)dir * S + wc) * LW_H + unit];
      }
    }
    // ---- B fragments of h_{j-1}: window mt 32 + l32 (zeros past S), this wave's K slice -------------------------
    f32x16 acc[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
    const int wl = mt * LW_S + l32;
    if constexpr (SPLIT) {
      uint4 bh[LW_KS], bl[LW_KS];
      const bf16_t* hr = static_cast<const bf16_t*>(hin) + ((long)dir * S + wl) * 2 * LW_H + kw + 8 * hh;
#pragma unroll
      for (int s = 0; s < LW_KS; ++s) {
        bh[s] = wl < S ? *reinterpret_cast<const uint4*>(hr + 16 * s) : make_uint4(0u, 0u, 0u, 0u);
        bl[s] = wl < S ? *reinterpret_cast<const uint4*>(hr + 16 * s + LW_H) : make_uint4(0u, 0u, 0u, 0u);
      }
      lstm_mfma_x3(whi, wlo, bh, bl, acc);
    } else {
      float hb[LW_KH];
      const float* hr = static_cast<const float*>(hin) + ((long)dir * S + wl) * LW_H + kw + LW_KH * hh;
#pragma unroll
      for (int s = 0; s < LW_KH; s += 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (wl < S) v = *reinterpret_cast<const float4*>(hr + s);
        hb[s] = v.x;
        hb[s + 1] = v.y;
        hb[s + 2] = v.z;
        hb[s + 3] = v.w;
      }
#pragma unroll
      for (int s = 0; s < LW_KH; ++s)
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[m][s], hb[s], acc[m], 0, 0, 0);
    }
    // ---- K-slice partials -> LDS: acc[m][i] holds row 32 m + 8 (i / 4) + 4 hh + i % 4, window l32 ---------------
#pragma unroll
    for (int m = 0; m < 2; ++m) lstm_store_partial(red[wave] + 32 * m, acc[m], hh, l32);
    __syncthreads();
    // ---- cell update: thread -> (unit cu, window cb), partials summed in a fixed order --------------------------
    if (live) {
      float h = 0.f, cc = 0.f;
      if (active) {
        float gs[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int r = g * LW_U + cu;
          gs[g] = lstm_sum8(red, r, cb);
        }
        cc = cprev;
        h = lstm_cell(prf, gs, true, cc);
      }
      const long o = ((long)dir * S + wc) * LW_H + unit;
      c[o] = cc;
      if (hf) hf[(long)dir * hf_dir_stride + (long)wc * LW_H + unit] = h;
      if (hout) {
        if constexpr (SPLIT) {
          bf16_t* ho = static_cast<bf16_t*>(hout) + ((long)dir * S + wc) * 2 * LW_H + unit;
          bf16_t hi, lo;
          lstm_split_h(h, hi, lo);
          ho[0] = hi;
          ho[LW_H] = lo;
        } else {
          static_cast<float*>(hout)[o] = h;
        }
      }
    }
    __syncthreads();  // red free for the next tile
  }
}

// `mean` merge: output row (clip b, frame t) = the fixed-order (ascending window) average over the windows that
// contain t of the forward h at local step t - w and of the reverse h at local step k - 1 - (t - w).  hf
// [dir][step][S][640]; hm [2][N][640] (forward | reverse means: the head's sum merge adds the two).
__global__ void __launch_bounds__(160) lstm_window_mean_kernel(const float4* __restrict__ hf,
                                                               const int* __restrict__ tab, int B, int W, int S, long N,
                                                               float4* __restrict__ hm) {
  const int b = blockIdx.y, t = blockIdx.x, len = tab[B + b];
  if (t >= len) return;
  const int k = min(len, W), nwin = len - k + 1, wbase = tab[3 * B + b];
  const int w0 = max(0, t - k + 1), w1 = min(t, nwin - 1);
  const int q = LW_H / 4, u = threadIdx.x;
  const long plane = (long)S * q;  // one step of one direction
  float4 f = make_float4(0.f, 0.f, 0.f, 0.f), r = f;
  for (int w = w0; w <= w1; ++w) {
    const int s = t - w;
    const float4 a = hf[(long)s * plane + (long)(wbase + w) * q + u];
    const float4 d = hf[((long)W + (k - 1 - s)) * plane + (long)(wbase + w) * q + u];
    f.x += a.x, f.y += a.y, f.z += a.z, f.w += a.w;
    r.x += d.x, r.y += d.y, r.z += d.z, r.w += d.w;
  }
  const float n = (float)(w1 - w0 + 1);
  const long row = (long)tab[b] + t;
  hm[row * q + u] = make_float4(f.x / n, f.y / n, f.z / n, f.w / n);
  hm[(N + row) * q + u] = make_float4(r.x / n, r.y / n, r.z / n, r.w / n);
}

// Pair rows: output row (pair p, local step s) = the forward h of window p at step s + its reverse h at step
// W - 1 - s (the reverse direction reaches frame s of the window at that step): the sum merge of M(x[p .. p + W - 1])[s].
// hf [dir][step][S][640], every window full (k = W); y (S, W, 640), y2 the same rows again (may be null).  One
// workgroup per output row, 160 float4 lanes: coalesced reads and writes, nothing shared between workgroups.
__global__ void __launch_bounds__(160) lstm_window_pairs_kernel(const float4* __restrict__ hf, int W, int S,
                                                                float4* __restrict__ y, float4* __restrict__ y2) {
  const int p = blockIdx.x, s = blockIdx.y;
  const int q = LW_H / 4, u = threadIdx.x;
  const long plane = (long)S * q;
  const float4 a = hf[(long)s * plane + (long)p * q + u];
  const float4 d = hf[((long)W + (W - 1 - s)) * plane + (long)p * q + u];
  const float4 o = make_float4(a.x + d.x, a.y + d.y, a.z + d.z, a.w + d.w);
  const long row = (long)p * W + s;
  y[row * q + u] = o;
  if (y2) y2[row * q + u] = o;
}

}  // namespace

bool lstm_window_supported(int H) { return H == LW_H; }

void pack_lstm_window_whh(const float* const whh[2], int H, float* out) {
  M2S_CHECK(H == LW_H, "lstm_window: rnn_hidden must be 640");
  for (int dir = 0; dir < 2; ++dir)
    for (int ug = 0; ug < LW_G; ++ug)
      for (int r = 0; r < 64; ++r) {
        const int g = r / LW_U, u = ug * LW_U + r % LW_U;
        const float* src = whh[dir] + ((size_t)g * H + u) * H;
        float* dst = out + (((size_t)dir * LW_G + ug) * 64 + r) * H;
        for (int k = 0; k < H; ++k) dst[k] = src[k];
      }
}

void launch_lstm_window_table(const int* tab, int B, int W, bool mean, int max_windows, int2* win, hipStream_t s) {
  M2S_CHECK(B >= 1 && B <= 65535 && max_windows >= 1, "lstm_window_table: shape");
  hipLaunchKernelGGL(lstm_window_table_kernel, dim3((max_windows + 255) / 256, B), dim3(256), 0, s, tab, B, W,
                     mean ? 1 : 0, win);
  M2S_HIP(hipGetLastError());
}

void launch_lstm_window_step0(const float* pre, const int2* win, int S, bool latest, bool split, void* hop, float* c,
                              float* hf0, float* hf1, hipStream_t s) {
  const dim3 grid((unsigned)(((long)S * LW_H + 255) / 256), 2);
  if (split)
    hipLaunchKernelGGL(lstm_window_step0_kernel<true>, grid, dim3(256), 0, s, pre, win, S, latest ? 1 : 0, hop, c, hf0,
                       hf1);
  else
    hipLaunchKernelGGL(lstm_window_step0_kernel<false>, grid, dim3(256), 0, s, pre, win, S, latest ? 1 : 0, hop, c,
                       hf0, hf1);
  M2S_HIP(hipGetLastError());
}

void launch_lstm_window_step(const float* pre, const float* wperm, const int2* win, int S, int j, int dirs, bool split,
                             const void* hin, void* hout, float* c, float* hf, long hf_dir_stride, hipStream_t s) {
  M2S_CHECK(S >= 1 && j >= 1 && (dirs == 1 || dirs == 2), "lstm_window_step: shape");
  // tile walkers per unit group: enough workgroups to fill the device twice over, each keeping its W_hh rows for
  // several tiles (the walk only decides who computes a tile, never how)
  const int ntiles = (S + LW_S - 1) / LW_S;
  const int walkers = std::min(ntiles, std::max(1, 512 / (LW_G * dirs)));
  const dim3 grid(walkers, LW_G, dirs);
  if (split)
    hipLaunchKernelGGL(lstm_window_step_kernel<true>, grid, dim3(64 * LW_W), 0, s, pre, wperm, win, S, j, hin, hout, c,
                       hf, hf_dir_stride);
  else
    hipLaunchKernelGGL(lstm_window_step_kernel<false>, grid, dim3(64 * LW_W), 0, s, pre, wperm, win, S, j, hin, hout, c,
                       hf, hf_dir_stride);
  M2S_HIP(hipGetLastError());
}

void launch_lstm_window_mean(const float* hf, const int* tab, int B, int W, int S, long N, int max_len, float* hm,
                             hipStream_t s) {
  M2S_CHECK(B >= 1 && B <= 65535 && max_len >= 1, "lstm_window_mean: shape");
  hipLaunchKernelGGL(lstm_window_mean_kernel, dim3(max_len, B), dim3(160), 0, s, reinterpret_cast<const float4*>(hf),
                     tab, B, W, S, N, reinterpret_cast<float4*>(hm));
  M2S_HIP(hipGetLastError());
}

void launch_lstm_window_pairs(const float* hf, int W, int S, float* y, float* y2, hipStream_t s) {
  M2S_CHECK(S >= 1 && W >= 1 && W <= 16, "lstm_window_pairs: shape");
  hipLaunchKernelGGL(lstm_window_pairs_kernel, dim3(S, W), dim3(160), 0, s, reinterpret_cast<const float4*>(hf), W, S,
                     reinterpret_cast<float4*>(y), reinterpret_cast<float4*>(y2));
  M2S_HIP(hipGetLastError());
}

}  // namespace m2s
