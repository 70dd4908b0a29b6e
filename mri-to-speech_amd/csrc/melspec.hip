// Waveform -> mel spectrogram, exact fp32 (m2s_melspec_* in m2s.h; DESIGN.md "Mel-spectrogram front end").
//
// The STFT is a GEMM on the f32 MFMA: frames (T x n_fft) . [w cos | -w sin] (n_fft x 2 bins), the window folded
// into tables built on the host in float64.  One workgroup owns (clip, tile of FT frames, group of four bin
// waves): it stages the tile's span of the waveform, (FT - 1) hop + n_fft floats, into LDS once, with the
// pre-emphasis and the reflect padding applied on the way in, and its A fragments are overlapping windows read
// from there at f hop + k.  One wave owns TPW tiles of 16 bins: it accumulates re and im over K, forms the
// magnitude or power in registers, transposes that 16 x 16 tile through LDS and multiplies it into its
// mel (FT x n_mels) accumulators, so the spectrum never leaves the CU.  Every wave writes its partial mel sums to
// the workspace; melspec_finish_kernel adds the P partials of an element in index order and applies the output
// map.  FT, TPW and P follow from the config alone, so a frame's summation order never depends on B, L or the
// frame's place in the batch.  No atomics, no flags, no waiting between workgroups.
#include <cmath>
#include <vector>

#include "melspec.hpp"
#include "prof.hpp"

namespace m2s {

namespace {

constexpr int SPAN_MAX = 15360;  // floats of LDS for the staged waveform (60 KB: two workgroups per CU)
constexpr int TR_LD = 17;        // row stride of the 16 x 16 transpose tile (odd: conflict-free both ways)

struct MelArgs {
  const float* wav;
  const float* dft;
  const float* basis;
  float* part;
  long L;
  int B, T, pad, hop, span, ft, k0, kb, nt, tpw, parts, power, n_mels;
  float preemph;
};

template <int MT, int NMT>
__global__ __launch_bounds__(256) void melspec_kernel(const MelArgs p) {
  extern __shared__ float smem[];
  float* xs = smem;                   // span + 16 floats: the tile's waveform, zeros behind the clip's end
  float* tr = smem + p.span + 16;     // 4 waves x MT x 16 x TR_LD
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, r = lane & 15;
  const int b = blockIdx.z, f0 = blockIdx.x * p.ft;
  const float* x = p.wav + (size_t)b * p.L;
  const long q0 = (long)f0 * p.hop, Lp = p.L + 2 * p.pad;
  for (int i = tid; i < p.span + 16; i += 256) {
    const long q = q0 + i;
    float v = 0.f;
    if (i < p.span && q < Lp) {
      long j = q - p.pad;
      if (j < 0) j = -j;
      if (j >= p.L) j = 2 * (p.L - 1) - j;
      v = x[j];
      if (p.preemph != 0.f && j > 0) v -= p.preemph * x[j - 1];
    }
    xs[i] = v;
  }
  __syncthreads();

  const int pidx = blockIdx.y * 4 + wave;
  float* trw = tr + wave * (MT * 16 * TR_LD);
  int rowoff[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) rowoff[mt] = min(mt * 16 + r, p.ft - 1) * p.hop + g;
  f32x4 acc[NMT][MT];
#pragma unroll
  for (int t = 0; t < NMT; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int it = 0; it < p.tpw; ++it) {
    const int j = pidx * p.tpw + it;
    const bool live = pidx < p.parts && j < p.nt;  // wave-uniform
    if (live) {
      f32x4 re[MT], im[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) re[mt] = im[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float4* tb = reinterpret_cast<const float4*>(p.dft) + (size_t)j * p.kb * 128 + lane;
      const float* xa = xs + p.k0;
      for (int kb = 0; kb < p.kb; ++kb) {
        const float4 br4 = tb[(size_t)kb * 128], bi4 = tb[(size_t)kb * 128 + 64];
        const float br[4] = {br4.x, br4.y, br4.z, br4.w}, bi[4] = {bi4.x, bi4.y, bi4.z, bi4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const float a = xa[rowoff[mt] + kb * 16 + 4 * i];
            re[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, br[i], re[mt], 0, 0, 0);
            im[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bi[i], im[mt], 0, 0, 0);
          }
      }
      // D layout: lane holds rows 4 g + i, column r
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float v = re[mt][i] * re[mt][i] + im[mt][i] * im[mt][i];
          if (p.power == 1) v = sqrtf(v + 1e-9f);
          trw[mt * (16 * TR_LD) + (4 * g + i) * TR_LD + r] = v;
        }
    }
    __syncthreads();
    if (live) {
      const float* bb = p.basis + (size_t)j * 4 * NMT * 64 + lane;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float a[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = trw[mt * (16 * TR_LD) + r * TR_LD + 4 * q + g];
#pragma unroll
        for (int t = 0; t < NMT; ++t) {
          const float w = bb[(q * NMT + t) * 64];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], w, acc[t][mt], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  if (pidx >= p.parts) return;
  float* out = p.part + ((size_t)pidx * p.B + b) * p.T * p.n_mels;
#pragma unroll
  for (int t = 0; t < NMT; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int fl = mt * 16 + 4 * g + i, mel = t * 16 + r;
        if (fl < p.ft && f0 + fl < p.T && mel < p.n_mels) out[(size_t)(f0 + fl) * p.n_mels + mel] = acc[t][mt][i];
      }
}

// mel[b][f][m] = map(sum over the partials in index order); n = B T n_mels
__global__ __launch_bounds__(256) void melspec_finish_kernel(const float* part, int parts, size_t n, int T, int n_mels,
                                                             int out_map, int layout, float* mel) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  float s = part[idx];
  for (int q = 1; q < parts; ++q) s += part[(size_t)q * n + idx];
  // comparisons, not fmaxf: a NaN stays a NaN, as with torch.clamp
  if (out_map == 0) s = logf(s < 1e-5f ? 1e-5f : s);
  else if (out_map == 1) s = 10.f * log10f(s < 1e-10f ? 1e-10f : s);
  if (layout == 1) {
    mel[idx] = s;
  } else {
    const int m = (int)(idx % n_mels);
    const size_t bf = idx / n_mels;
    const int f = (int)(bf % T);
    mel[((bf / T) * n_mels + m) * T + f] = s;
  }
}

template <int MT, int NMT>
void launch(const MelArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  allow_lds(reinterpret_cast<const void*>(&melspec_kernel<MT, NMT>));
  hipLaunchKernelGGL((melspec_kernel<MT, NMT>), grid, dim3(256), lds, s, a);
}

template <int MT>
void launch_nmt(int nmt, const MelArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  switch (nmt) {
    case 1: return launch<MT, 1>(a, grid, lds, s);
    case 2: return launch<MT, 2>(a, grid, lds, s);
    case 4: return launch<MT, 4>(a, grid, lds, s);
    default: return launch<MT, 8>(a, grid, lds, s);
  }
}

}  // namespace

MelSpec::MelSpec(const m2s_melspec_cfg& c, const float* mel_basis_host, int device) : c_(c), device_(device) {
  M2S_CHECK(c.n_fft >= 16 && c.n_fft <= 4096 && c.n_fft % 2 == 0, "melspec: n_fft must be even, 16..4096");
  M2S_CHECK(c.hop >= 1, "melspec: hop must be >= 1");
  M2S_CHECK(c.win >= 1 && c.win <= c.n_fft, "melspec: win must be 1..n_fft");
  M2S_CHECK(c.n_mels >= 1 && c.n_mels <= 128, "melspec: n_mels must be 1..128");
  M2S_CHECK(c.pad == 0 || c.pad == 1, "melspec: pad must be 0 or 1");
  M2S_CHECK(c.pad == 0 || c.hop <= c.n_fft, "melspec: the reflect pad needs hop <= n_fft");
  M2S_CHECK(c.power == 1 || c.power == 2, "melspec: power must be 1 or 2");
  M2S_CHECK(c.out >= 0 && c.out <= 2, "melspec: out must be 0, 1 or 2");
  M2S_CHECK(std::isfinite(c.preemph), "melspec: preemph must be finite");
  M2S_CHECK(mel_basis_host, "melspec: null mel basis");
  pad_ = c.pad ? (c.n_fft - c.hop) / 2 : 0;
  bins_ = c.n_fft / 2 + 1;
  nt_ = ceil_div(bins_, 16);
  const int left = (c.n_fft - c.win) / 2;  // torch.stft centres a short window in the frame
  k0_ = left / 16 * 16;
  kb_ = (std::min(round_up(left + c.win, 16), round_up(c.n_fft, 16)) - k0_) / 16;
  ft_ = 32;
  while (ft_ > 1 && (long)(ft_ - 1) * c.hop + c.n_fft + 16 > SPAN_MAX) ft_ /= 2;
  mt_ = ft_ > 16 ? 2 : 1;
  span_ = (int)((long)(ft_ - 1) * c.hop + c.n_fft);
  tpw_ = nt_ >= 32 ? 2 : 1;
  parts_ = ceil_div(nt_, tpw_);
  nmt_ = c.n_mels <= 16 ? 1 : c.n_mels <= 32 ? 2 : c.n_mels <= 64 ? 4 : 8;

  // float64 tables, rounded once to fp32; the angle is reduced exactly: (k n) mod n_fft
  const int N = c.n_fft;
  const double two_pi = 6.283185307179586476925286766559;
  std::vector<double> ct(N), st(N), w(N, 0.0);
  for (int i = 0; i < N; ++i) ct[i] = std::cos(two_pi * i / N), st[i] = std::sin(two_pi * i / N);
  for (int i = 0; i < c.win; ++i) w[left + i] = 0.5 - 0.5 * std::cos(two_pi * i / c.win);  // periodic Hann
  std::vector<float> dft((size_t)nt_ * kb_ * 512, 0.f);
  for (int j = 0; j < nt_; ++j)
    for (int kb = 0; kb < kb_; ++kb)
      for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 4; ++i) {
          const int k = k0_ + 16 * kb + 4 * i + (lane >> 4), bin = 16 * j + (lane & 15);
          if (k >= N || bin >= bins_) continue;
          const int a = (int)(((long)k * bin) % N);
          const size_t o = (((size_t)j * kb_ + kb) * 2 * 64 + lane) * 4 + i;
          dft[o] = (float)(w[k] * ct[a]);
          dft[o + 256] = (float)(-w[k] * st[a]);
        }
  std::vector<float> basis((size_t)nt_ * 4 * nmt_ * 64, 0.f);
  for (int j = 0; j < nt_; ++j)
    for (int q = 0; q < 4; ++q)
      for (int t = 0; t < nmt_; ++t)
        for (int lane = 0; lane < 64; ++lane) {
          const int bin = 16 * j + 4 * q + (lane >> 4), mel = 16 * t + (lane & 15);
          if (bin < bins_ && mel < c.n_mels)
            basis[(((size_t)j * 4 + q) * nmt_ + t) * 64 + lane] = mel_basis_host[(size_t)mel * bins_ + bin];
        }
  M2S_HIP(hipMalloc(&dft_, dft.size() * sizeof(float)));
  if (hipMalloc(&basis_, basis.size() * sizeof(float)) != hipSuccess) {
    (void)hipFree(dft_);
    throw Error(M2S_E_HIP, "melspec: hipMalloc failed");
  }
  hipError_t e = hipMemcpy(dft_, dft.data(), dft.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(basis_, basis.data(), basis.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dft_);
    (void)hipFree(basis_);
    throw Error(M2S_E_HIP, std::string("melspec: table upload: ") + hipGetErrorString(e));
  }
}

MelSpec::~MelSpec() {
  (void)hipFree(dft_);
  (void)hipFree(basis_);
}

int MelSpec::frames(long L) const {
  if (L < 1 || L > 0x7fffffffL - 2 * (long)pad_) return 0;
  if (pad_ >= L) return 0;  // a reflect pad mirrors each side once
  const long Lp = L + 2 * (long)pad_;
  if (Lp < c_.n_fft) return 0;
  return (int)(1 + (Lp - c_.n_fft) / c_.hop);
}

size_t MelSpec::workspace_bytes(int B, long L) const {
  const int T = frames(L);
  if (B < 1 || B > 65535 || T == 0) return 0;
  return ((size_t)parts_ * B * T * c_.n_mels * sizeof(float) + 255) & ~size_t(255);
}

void MelSpec::forward(const float* wav, int B, long L, float* mel, int layout, void* ws, size_t ws_bytes,
                      hipStream_t s) const {
  M2S_CHECK(B >= 1 && B <= 65535, "melspec: B must be 1..65535");
  const int T = frames(L);
  M2S_CHECK(T > 0, "melspec: clip too short for one frame (or for the reflect pad)");
  M2S_CHECK(layout == 0 || layout == 1, "melspec: layout must be 0 or 1");
  M2S_CHECK(ws_bytes >= workspace_bytes(B, L), "workspace too small");
  const size_t n = (size_t)B * T * c_.n_mels;
  MelArgs a;
  a.wav = wav, a.dft = dft_, a.basis = basis_, a.part = static_cast<float*>(ws);
  a.L = L, a.B = B, a.T = T, a.pad = pad_, a.hop = c_.hop, a.span = span_, a.ft = ft_, a.k0 = k0_, a.kb = kb_;
  a.nt = nt_, a.tpw = tpw_, a.parts = parts_, a.power = c_.power, a.n_mels = c_.n_mels, a.preemph = c_.preemph;
  const dim3 grid(ceil_div(T, ft_), ceil_div(parts_, 4), B);
  const size_t lds = ((size_t)span_ + 16 + 4 * mt_ * 16 * TR_LD) * sizeof(float);
  StageTag tag("melspec");
  {
    const double rows = (double)B * T;
    const double flops = rows * (4.0 * c_.win * bins_ + 3.0 * bins_ + 2.0 * bins_ * c_.n_mels);
    const double bytes = 4.0 * ((double)B * L + (double)n + (double)nt_ * kb_ * 512 + (double)bins_ * c_.n_mels);
    ProfScope ps("melspec<f32,mt" + std::to_string(mt_) + ",nm" + std::to_string(nmt_) + ">", flops, bytes, s,
                 4.0 * (double)parts_ * n);
    if (mt_ == 2) launch_nmt<2>(nmt_, a, grid, lds, s);
    else launch_nmt<1>(nmt_, a, grid, lds, s);
    M2S_HIP(hipGetLastError());
  }
  {
    ProfScope ps("melspec_finish", (double)parts_ * n, 0.0, s);
    hipLaunchKernelGGL(melspec_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.part, parts_, n, T,
                       c_.n_mels, c_.out, layout, mel);
    M2S_HIP(hipGetLastError());
  }
}

}  // namespace m2s
