// Kernels of the Grad-CAM engine (cam.hpp): the band-power cotangents, the backward
// through time of many cotangents over one saved forward, and the heat maps.  Exact fp32; every
// reduction runs in a fixed order that depends on the model's sizes only, so a cotangent's result does
// not depend on how many others share its launch.
#include <algorithm>
#include <cstdint>

#include "cam.hpp"
#include "prof.hpp"

namespace m2s {

namespace {

// ---------------------------------------------------------------------------------------------
// (a) d target_k / d pred_norm.  target = (mean | sum) over frames of sum_{m in band} 10^(dB[t,m]/10) with
// dB = pred * std + mean (mri_gradcam_formant.py:230-247), or that band power at one frame (:254-266).
__global__ void __launch_bounds__(256) gradcam_cotangent_kernel(const float* __restrict__ pred,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ sd,
                                                                const float* __restrict__ mask,
                                                                const int* __restrict__ fidx, int F, int T, int nm,
                                                                int k0, long total, int sum, float* __restrict__ dpred) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int m = (int)(i % nm);
  const long r = i / nm;
  const int t = (int)(r % T), k = k0 + (int)(r / T);
  const int band = k / (1 + F), j = k - band * (1 + F);
  float s;
  if (j == 0) s = sum ? 1.f : 1.f / (float)T;
  else s = fidx[j - 1] == t ? 1.f : 0.f;
  const float mk = mask[(long)band * nm + m];
  float v = 0.f;
  if (s != 0.f && mk != 0.f) {
    const float db = __fadd_rn(__fmul_rn(pred[(long)t * nm + m], sd[m]), mean[m]);
    const float pw = powf(10.0f, db / 10.0f);
    v = s * pw * 2.302585092994046f / 10.0f * sd[m] * mk;
  }
  dpred[i] = v;
}

// ---------------------------------------------------------------------------------------------
// (b) one step of the backward through time for up to 16 cotangents and both directions.
// Workgroup = 16 hidden units of one direction, 8 waves.  dh[u][k] = dy[k][t][u] + sum_n W_hh^T[u][n] dG[k][tn][n]
// is a (16 units x 4H) x (4H x 16 cotangents) product on v_mfma_f32_16x16x4_f32 with the cotangents as the
// N dimension: every lane loads 16 bytes of its W_hh^T row and 16 bytes of its cotangent's previous gate
// gradient per four MFMAs, so a weight is read once per launch whatever the number of cotangents.  Wave w
// takes the 16-wide slices w, w + 8, ... of the 4H reduction; the eight partial tiles are added in wave
// order.  Columns past `kc` are zero and are never stored; columns never mix, so a cotangent's bits do not
// depend on its neighbours.  The step's gates and cells are staged once and shared by all cotangents.
constexpr int BM_WAVES = 8;
__global__ void __launch_bounds__(BM_WAVES * 64) lstm_bptt_multi_step_kernel(
    const float* __restrict__ whh_t, const float* __restrict__ dy, const float* __restrict__ gates,
    const float* __restrict__ cells, float* __restrict__ dc, float* __restrict__ dg, int kc, int T, int H, int step) {
  __shared__ float red[BM_WAVES][16][17];  // [wave][unit][cotangent]
  __shared__ float sg[6][16];              // i, f, g, o, c, c_prev of the 16 units
  const int G = 4 * H;
  const int dir = blockIdx.y, u0 = blockIdx.x * 16, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q = lane >> 4;
  const int t = dir == 0 ? T - 1 - step : step;
  const int tn = dir == 0 ? t + 1 : t - 1;  // processed before this step: its gate gradients feed dh
  const int tp = dir == 0 ? t - 1 : t + 1;  // the step whose cell this step consumed
  const long row = (long)dir * T + t;       // saved activations of one sequence: (2, 1, T, .)
  if (tid < 96) {
    const int which = tid >> 4, u = u0 + (tid & 15);
    float v;
    if (which < 4) v = gates[row * G + (long)which * H + u];
    else if (which == 4) v = cells[row * H + u];
    else v = step == T - 1 ? 0.f : cells[((long)dir * T + tp) * H + u];  // the last step is the direction's first cell
    sg[which][tid & 15] = v;
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (step > 0) {
    const bool live = r16 < kc;
    const float* wrow = whh_t + ((long)dir * H + u0 + r16) * G + 4 * q + 16 * wave;
    // a padding column reads cotangent 0's row (always there) and is zeroed after the load: no divergent load
    const float* brow = dg + (((long)dir * kc + (live ? r16 : 0)) * T + tn) * G + 4 * q + 16 * wave;
    const int nit = (G / 16 - wave + BM_WAVES - 1) / BM_WAVES;  // slices wave, wave + 8, ...
    auto load_b = [&](int i) {
      float4 b = *reinterpret_cast<const float4*>(brow + 16 * BM_WAVES * i);
      b.x = live ? b.x : 0.f;
      b.y = live ? b.y : 0.f;
      b.z = live ? b.z : 0.f;
      b.w = live ? b.w : 0.f;
      return b;
    };
    auto mma = [&](const float4& a, const float4& b) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    };
    int i = 0;
    for (; i + 1 < nit; i += 2) {  // two slices' loads in flight; the slices are still added in order
      const float4 a0 = *reinterpret_cast<const float4*>(wrow + 16 * BM_WAVES * i);
      const float4 a1 = *reinterpret_cast<const float4*>(wrow + 16 * BM_WAVES * (i + 1));
      const float4 b0 = load_b(i), b1 = load_b(i + 1);
      mma(a0, b0);
      mma(a1, b1);
    }
    if (i < nit) mma(*reinterpret_cast<const float4*>(wrow + 16 * BM_WAVES * i), load_b(i));
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave][4 * q + r][r16] = acc[r];  // D[m = 4 (lane / 16) + r][n = lane % 16]
  __syncthreads();
  if (tid < 256) {
    const int ul = tid & 15, k = tid >> 4;  // units fastest: 64-byte runs in dG
    if (k < kc) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < BM_WAVES; ++w) s += red[w][ul][k];
      const int u = u0 + ul;
      const float gi = sg[0][ul], gf = sg[1][ul], gg = sg[2][ul], go = sg[3][ul], c = sg[4][ul], cp = sg[5][ul];
      const float dh = dy[((long)k * T + t) * H + u] + s;
      const float tc = tanhf(c);
      float* dcp = dc + ((long)dir * kc + k) * H + u;
      const float dcv = (step > 0 ? *dcp : 0.f) + dh * go * (1.f - tc * tc);
      float* o = dg + (((long)dir * kc + k) * T + t) * G;
      o[u] = dcv * gg * gi * (1.f - gi);
      o[H + u] = dcv * cp * gf * (1.f - gf);
      o[2 * H + u] = dcv * gi * (1.f - gg * gg);
      o[3 * H + u] = dh * tc * go * (1.f - go);
      *dcp = dcv * gf;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// (c) heat maps (mri_gradcam_formant.py:169-200): cam = relu(sum_c w[c] feats[frame][c]) on the h x w map,
// bilinear resize to H x W (torch align_corners=False), (v - min) / ((max - min) + 1e-6) over the resized map.
// One workgroup per map: scaled weights, the source map and the row / column sample tables in LDS, one pass
// for the extremes, one pass that writes.  The interpolation is the lerp form a + l (b - a): a constant map
// resizes to exactly that constant, so its normalised map is exactly zero.
// mode 0: map m takes weights row m, frame tab ? tab[m] : m, output map m.
// mode 1: map m is cotangent k0 + m of a chunk laid out (kc, T, C); whole-clip cotangents (j = 0) leave;
//         a frame cotangent takes row m * T + tab[j - 1], frame tab[j - 1], output map band * F + j - 1.
struct HeatArgs {
  const float* feats;
  const float* weights;
  const int* tab;
  float* out;
  float wscale;
  int N, C, h, w, H, W, mode, k0, F, T, vec;
};

__device__ __forceinline__ float heat_sample(const float* cam, const int* xi, const float* xl, const int* yi,
                                             const float* yl, int w, int h, int W, int i) {
  const int y = i / W, x = i - y * W;
  const int y0 = yi[y], x0 = xi[x];
  const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
  const float lx = xl[x], ly = yl[y];
  const float a = cam[y0 * w + x0], b = cam[y0 * w + x1], c = cam[y1 * w + x0], d = cam[y1 * w + x1];
  const float top = a + lx * (b - a), bot = c + lx * (d - c);
  return top + ly * (bot - top);
}

__global__ void __launch_bounds__(256) cam_heatmap_kernel(const HeatArgs a) {
  extern __shared__ float sm[];
  const int P = a.h * a.w, tid = threadIdx.x;
  float* sw = sm;             // [C] weights * wscale
  float* cam = sw + a.C;      // [P]
  float* xl = cam + P;        // [W]
  float* yl = xl + a.W;       // [H]
  int* xi = reinterpret_cast<int*>(yl + a.H);  // [W]
  int* yi = xi + a.W;                          // [H]
  __shared__ float rmin[4], rmax[4];
  int m = blockIdx.x, fr;
  long wrow, omap;
  if (a.mode == 0) {
    fr = a.tab ? a.tab[m] : m;
    wrow = m;
    omap = m;
  } else {
    const int k = a.k0 + m, band = k / (1 + a.F), j = k - band * (1 + a.F);
    if (j == 0) return;
    fr = a.tab[j - 1];
    wrow = (long)m * a.T + fr;
    omap = (long)band * a.F + (j - 1);
  }
  const bool valid = fr >= 0 && fr < a.N;  // a frame outside the clip gives an all-zero map
  for (int c = tid; c < a.C; c += 256) sw[c] = valid ? a.weights[wrow * a.C + c] * a.wscale : 0.f;
  const float sx = (float)a.w / (float)a.W, sy = (float)a.h / (float)a.H;
  for (int x = tid; x < a.W; x += 256) {
    const float src = fmaxf(sx * ((float)x + 0.5f) - 0.5f, 0.f);
    const int i0 = min((int)src, a.w - 1);
    xi[x] = i0;
    xl[x] = src - (float)i0;
  }
  for (int y = tid; y < a.H; y += 256) {
    const float src = fmaxf(sy * ((float)y + 0.5f) - 0.5f, 0.f);
    const int i0 = min((int)src, a.h - 1);
    yi[y] = i0;
    yl[y] = src - (float)i0;
  }
  __syncthreads();
  for (int p = tid; p < P; p += 256) {
    float s = 0.f;
    if (valid) {
      const float* f = a.feats + (long)fr * a.C * P + p;
      for (int c = 0; c < a.C; ++c) s = fmaf(sw[c], f[(long)c * P], s);
    }
    cam[p] = fmaxf(s, 0.f);
  }
  __syncthreads();
  const int total = a.H * a.W;
  float mn = 3.402823466e38f, mx = -3.402823466e38f;
  for (int i = tid; i < total; i += 256) {
    const float v = heat_sample(cam, xi, xl, yi, yl, a.w, a.h, a.W, i);
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o));
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
  if ((tid & 63) == 0) {
    rmin[tid >> 6] = mn;
    rmax[tid >> 6] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(rmin[0], rmin[1]), fminf(rmin[2], rmin[3]));
  mx = fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3]));
  const float den = (mx - mn) + 1e-6f;
  float* o = a.out + omap * (long)total;
  if (a.vec) {  // H * W % 4 == 0 and a 16-byte aligned output: 16-byte stores along W
    for (int i = tid * 4; i < total; i += 1024) {
      float4 v;
      v.x = (heat_sample(cam, xi, xl, yi, yl, a.w, a.h, a.W, i) - mn) / den;
      v.y = (heat_sample(cam, xi, xl, yi, yl, a.w, a.h, a.W, i + 1) - mn) / den;
      v.z = (heat_sample(cam, xi, xl, yi, yl, a.w, a.h, a.W, i + 2) - mn) / den;
      v.w = (heat_sample(cam, xi, xl, yi, yl, a.w, a.h, a.W, i + 3) - mn) / den;
      *reinterpret_cast<float4*>(o + i) = v;
    }
  } else {
    for (int i = tid; i < total; i += 256) o[i] = (heat_sample(cam, xi, xl, yi, yl, a.w, a.h, a.W, i) - mn) / den;
  }
}

}  // namespace

void launch_gradcam_cotangents(const float* pred, const float* mean, const float* sd, const float* mask,
                               const int* fidx, int F, int T, int nm, int k0, int kc, bool sum, float* dpred,
                               hipStream_t s) {
  const long total = (long)kc * T * nm;
  if (total <= 0) return;
  M2S_CHECK((total + 255) / 256 <= 2147483647L, "gradcam cotangents: too many elements");
  ProfScope ps("gradcam_cotangents", 8.0 * total, 4.0 * total, s);
  hipLaunchKernelGGL(gradcam_cotangent_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pred, mean, sd,
                     mask, fidx, F, T, nm, k0, total, sum ? 1 : 0, dpred);
  M2S_HIP(hipGetLastError());
}

void launch_lstm_bptt_multi_step(const float* whh_t, const float* dy, const float* gates, const float* cells, float* dc,
                                 float* dg, int kc, int T, int H, int step, hipStream_t s) {
  M2S_CHECK(H > 0 && H % 16 == 0, "lstm_bptt_multi: hidden size must be a multiple of 16");
  M2S_CHECK(kc >= 1 && kc <= kGradcamKC && T >= 1 && step >= 0 && step < T, "lstm_bptt_multi: chunk / step");
  const double G = 4.0 * H;
  ProfScope ps("lstm_bptt_multi_step", 2.0 * 2 * kc * G * H, 4.0 * (2 * G * H + 2.0 * kc * (2 * G + H) + 2 * 6.0 * H), s);
  hipLaunchKernelGGL(lstm_bptt_multi_step_kernel, dim3(H / 16, 2), dim3(BM_WAVES * 64), 0, s, whh_t, dy, gates, cells,
                     dc, dg, kc, T, H, step);
  M2S_HIP(hipGetLastError());
}

static size_t heat_lds_bytes(int C, int h, int w, int H, int W) {
  return sizeof(float) * ((size_t)C + (size_t)h * w + 2 * ((size_t)H + W));
}

bool cam_heatmap_shape_ok(int C, int h, int w, int H, int W) {
  return C >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && (long)h * w <= 16384 && (long)H * W <= 2147483647L - 1024 &&
         H <= 16384 && W <= 16384 && heat_lds_bytes(C, h, w, H, W) <= 64 * 1024 - 64;
}

void launch_cam_heatmap(const float* feats, int N, int C, int h, int w, const float* weights, float wscale,
                        const int* tab, int mode, int k0, int F, int T, int M, int H, int W, float* out,
                        hipStream_t s) {
  M2S_CHECK(cam_heatmap_shape_ok(C, h, w, H, W), "cam_heatmap: map sizes (the source map, the weights and the "
                                                 "sample tables must fit 64 KB of LDS)");
  M2S_CHECK(N >= 1 && M >= 0 && (mode == 0 || tab), "cam_heatmap: bad argument");
  if (M == 0) return;
  HeatArgs a;
  a.feats = feats;
  a.weights = weights;
  a.tab = tab;
  a.out = out;
  a.wscale = wscale;
  a.N = N; a.C = C; a.h = h; a.w = w; a.H = H; a.W = W;
  a.mode = mode; a.k0 = k0; a.F = F; a.T = T;
  a.vec = ((long)H * W % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0) ? 1 : 0;
  const double px = (double)M * H * W;
  ProfScope ps("cam_heatmap", 2.0 * M * C * h * w + 20.0 * px, 4.0 * (px + (double)M * C * (h * w + 1)), s);
  hipLaunchKernelGGL(cam_heatmap_kernel, dim3(M), dim3(256), heat_lds_bytes(C, h, w, H, W), s, a);
  M2S_HIP(hipGetLastError());
}

}  // namespace m2s
