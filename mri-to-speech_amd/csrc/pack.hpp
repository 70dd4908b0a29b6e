// Host-side packing helpers shared by the packers (pack_acoustic.cpp, pack_vocoder.cpp), the model plans
// (acoustic_cnn.cpp, acoustic_rnn.cpp, vocoder.cpp) and the Grad-CAM path (cam.cpp):
//   * state-dict lookup, host bf16 / split / e4m3 conversions, per-channel e4m3 scales (channel_scales);
//   * the MFMA operand fragment writers, the one definition of each lane order: frag_bf16 (plain K),
//     frag_bf16_pwl (er_fused.hip's permuted K) and frag_e4m3, with the emit policy Plane (bf16 / hi / lo);
//   * dense-conv packing into the conv kernels' [phase][n_pad][kp] rows, ConvArgs set-up;
//   * TF-SAME padding, the tf_efficientnetv2_b2 stage table and its one walk (for_each_backbone_block /
//     for_each_backbone_map).
// DESIGN.md "Weight packing" says how to add a layout.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "model.hpp"

namespace m2s {

inline const HostTensor& need(const StateDict& sd, const std::string& k, std::vector<int64_t> shape) {
  auto it = sd.find(k);
  if (it == sd.end()) throw Error(M2S_E_ARG, "missing state-dict key: " + k);
  if (it->second.shape != shape) {
    std::string got, want;
    for (auto d : it->second.shape) got += std::to_string(d) + ",";
    for (auto d : shape) want += std::to_string(d) + ",";
    throw Error(M2S_E_ARG, "shape mismatch for " + k + ": got (" + got + ") want (" + want + ")");
  }
  return it->second;
}

inline uint16_t f2bf_host(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // quiet NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf2f_host(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
inline void split_host(float f, uint16_t* hi, uint16_t* lo) {
  *hi = f2bf_host(f);
  *lo = f2bf_host(f - bf2f_host(*hi));
}

// Event-profiler record names = the kernels' demangled symbols as rocprofv3 prints them, so the
// two profiles can be joined on the name.
template <typename T>
inline std::string tname(const char* base, const char* extra = "") {
  return std::string(base) + (std::is_same<T, bf16_t>::value ? "<unsigned short" : std::is_same<T, sp_t>::value ? "<m2s::sp_t" : "<float") +
         extra + ">";
}

inline int kc_of(int dtype) { return dtype == M2S_DT_F32 ? Elem<float>::KC : Elem<bf16_t>::KC; }
// bytes per activation element of a dtype's storage (split fp32: hi + lo; e4m3 operands keep bf16)
inline size_t act_bytes(int dtype) { return dtype == M2S_DT_BF16 || dtype == M2S_DT_FP8 ? 2 : 4; }

constexpr float kE4M3Max = 448.f;  // largest finite e4m3
// OCP e4m3fn rounding of a float (round to nearest even; 3 mantissa bits, exponents -6..8 with
// subnormals down to 2^-9, largest finite 448): the grid gfx950's v_cvt_pk_fp8_f32 rounds onto.
inline float e4m3_host(float x) {
  if (!(x == x) || x == 0.f) return 0.f;
  const float a = std::fabs(x);
  if (a >= kE4M3Max) return std::copysign(kE4M3Max, x);
  int e;
  std::frexp(a, &e);                       // a = m * 2^e, m in [0.5, 1): leading bit 2^(e-1)
  const float step = std::ldexp(1.f, std::max(e - 1, -6) - 3);
  return std::copysign(std::nearbyint(a / step) * step, x);
}


// OCP e4m3fn bit pattern of a value on the e4m3 grid (e4m3_host output; -0 -> +0)
inline uint8_t e4m3_bits_host(float v) {
  if (v == 0.f) return 0;
  const uint8_t sgn = v < 0.f ? 0x80 : 0;
  const float a = std::fabs(v);
  int e;
  std::frexp(a, &e);
  const int E = e - 1;  // a = 1.m x 2^E
  if (E < -6) return sgn | (uint8_t)std::nearbyint(a / std::ldexp(1.f, -9));  // subnormal: m x 2^-9
  return sgn | (uint8_t)((E + 7) << 3) | (uint8_t)std::nearbyint((a / std::ldexp(1.f, E) - 1.f) * 8.f);
}

// Per-output-channel e4m3 scales: s[n] = max_k |get(n, k)| / 448 (the largest finite e4m3), 1 for an all-zero row
// and for the pad rows rows .. n_pad - 1.
template <class Get>
inline std::vector<float> channel_scales(int rows, int cols, Get get, int n_pad = 0) {
  std::vector<float> sc(std::max(rows, n_pad), 1.f);
  for (int n = 0; n < rows; ++n) {
    float amax = 0.f;
    for (int k = 0; k < cols; ++k) amax = std::max(amax, std::fabs(get(n, k)));
    if (amax > 0.f) sc[n] = amax / kE4M3Max;
  }
  return sc;
}
// the e4m3 byte of w / scale
inline uint8_t emit_e4m3(float w, float scale) { return e4m3_bits_host(e4m3_host(w / scale)); }

// What a 16-bit fragment element holds of a weight: its bf16 rounding, or the hi / lo plane of its split.
enum class Plane { bf16, hi, lo };
inline uint16_t emit16(Plane p, float w) {
  if (p == Plane::bf16) return f2bf_host(w);
  uint16_t hi, lo;
  split_host(w, &hi, &lo);
  return p == Plane::hi ? hi : lo;
}

// ---- MFMA operand fragments.  A packer names the tile and gives w(n, k), which returns 0 outside the real
// weights; the lane order is written here and nowhere else.
// One 16 x 32 operand tile of v_mfma_f32_16x16x32_bf16 as [lane][8]: lane (row r = lane & 15, k group g = lane >> 4)
// holds w(16 n16 + r, 32 ks + 8 g + e), e = 0..7.  512 elements.
template <class W>
inline void frag_bf16(uint16_t* dst, Plane p, int n16, int ks, W w) {
  for (int ln = 0; ln < 64; ++ln)
    for (int e = 0; e < 8; ++e) dst[ln * 8 + e] = emit16(p, w(16 * n16 + (ln & 15), 32 * ks + 8 * (ln >> 4) + e));
}
// The same tile in the permuted K order of the fused EdgeResidual kernels' conv_pwl (er_fused.hip header, "k-slot
// permutation": the expanded tile leaves conv_exp's accumulators with lane group g owning channels 4 g .. 4 g + 3
// of each 16, so a lane's 8 elements are channels 4 g + 0..3 and 16 + 4 g + 0..3 of the k-step's 32).
template <class W>
inline void frag_bf16_pwl(uint16_t* dst, Plane p, int n16, int ks, W w) {
  for (int ln = 0; ln < 64; ++ln)
    for (int e = 0; e < 8; ++e) {
      const int g4 = 4 * (ln >> 4);
      dst[ln * 8 + e] = emit16(p, w(16 * n16 + (ln & 15), 32 * ks + (e < 4 ? g4 + e : 16 + g4 + e - 4)));
    }
}
// One half (16 bytes a lane) of an e4m3 operand tile of the K = 128 MFMA as [lane][16] (er8_fused.hip, er8w_fused.hip):
// byte j of lane (r, g) is w(n, g, 16 half + j) / scale[n] for n = 16 n16 + r < rows, zero past them.  1024 bytes.
template <class W>
inline void frag_e4m3(uint8_t* dst, int n16, int half, const std::vector<float>& scale, int rows, W w) {
  for (int ln = 0; ln < 64; ++ln)
    for (int j = 0; j < 16; ++j) {
      const int n = 16 * n16 + (ln & 15);
      dst[ln * 16 + j] = n < rows ? emit_e4m3(w(n, ln >> 4, 16 * half + j), scale[n]) : 0;
    }
}
// the mid channel behind byte b of lane group g in those kernels' conv_pwl operand (16 channels a 4-byte column)
inline int e4m3_pwl_channel(int g, int b) { return 16 * (b >> 2) + 4 * g + (b & 3); }

// A 1x1 conv as e4m3 bytes for the K = 128 block-scaled MFMA (gemm128.hip): rows [n_pad][kp], kp = cin
// rounded up to 128, w[n][c] / s[n] on the e4m3 grid with s = channel_scales; scales and bias [n_pad].
template <class Get, class Bias>
inline void pack_gemm_f8(Arena& ar, int cin, int cout, int n_pad, int kp, Get get, Bias bias, size_t* w_off,
                         size_t* s_off, size_t* b_off) {
  std::vector<uint8_t> w((size_t)n_pad * kp, 0);
  const std::vector<float> sc = channel_scales(cout, cin, get, n_pad);
  std::vector<float> b(n_pad, 0.f);
  for (int n = 0; n < cout; ++n) {
    for (int c = 0; c < cin; ++c) w[(size_t)n * kp + c] = emit_e4m3(get(n, c), sc[n]);
    b[n] = bias(n);
  }
  *w_off = ar.add_vec(w);
  *s_off = ar.add_vec(sc);
  *b_off = ar.add_vec(b);
}

inline PConv make_pconv(int kind, int cin, int cout, int ntaps, int dtype) {
  PConv p;
  p.kind = kind;
  p.cin = cin;
  p.cout = cout;
  p.cs_in = chan_stride(cin);
  p.cs_out = chan_stride(cout);
  p.ntaps = ntaps;
  const int kc = kc_of(dtype);
  p.tpc = conv_tpc(p.cs_in, kc);
  p.kp = conv_kp(ntaps, p.cs_in, kc);
  p.n_pad = round_up(p.cs_out, 64);
  return p;
}

// get(phase, n, tap, c) for n < cout, tap < ntaps, c < cin; bias(n)
template <class Get, class Bias>
inline void pack_conv(Arena& ar, int dtype, PConv& p, Get get, Bias bias) {
  std::vector<float> w((size_t)p.phases * p.n_pad * p.kp, 0.f);
  for (int ph = 0; ph < p.phases; ++ph)
    for (int n = 0; n < p.cout; ++n)
      for (int t = 0; t < p.ntaps; ++t)
        for (int c = 0; c < p.cin; ++c)
          w[((size_t)ph * p.n_pad + n) * p.kp + (size_t)t * p.cs_in + c] = get(ph, n, t, c);
  if (dtype == M2S_DT_FP8) {  // per output channel (over its phases): w / s on the e4m3 grid (exact in bf16)
    const std::vector<float> sc = channel_scales(
        p.n_pad, p.phases * p.kp, [&](int n, int k) { return w[((size_t)(k / p.kp) * p.n_pad + n) * p.kp + k % p.kp]; });
    std::vector<uint16_t> h(w.size());
    for (size_t i = 0; i < w.size(); ++i) h[i] = f2bf_host(e4m3_host(w[i] / sc[(i / p.kp) % p.n_pad]));
    p.w_off = ar.add_vec(h);
    p.ws_off = ar.add_vec(sc);
    p.fp8 = true;
  } else if (dtype == M2S_DT_BF16) {
    std::vector<uint16_t> h(w.size());
    for (size_t i = 0; i < w.size(); ++i) h[i] = f2bf_host(w[i]);
    p.w_off = ar.add_vec(h);
  } else if (dtype == M2S_DT_BF16X3) {  // rows [hi kp | lo kp]
    std::vector<uint16_t> h(2 * w.size());
    const size_t rows = w.size() / p.kp;
    for (size_t r = 0; r < rows; ++r)
      for (int k = 0; k < p.kp; ++k) split_host(w[r * p.kp + k], &h[2 * r * p.kp + k], &h[(2 * r + 1) * p.kp + k]);
    p.w_off = ar.add_vec(h);
  } else {
    p.w_off = ar.add_vec(w);
  }
  std::vector<float> b(p.n_pad, 0.f);
  for (int n = 0; n < p.cout; ++n) b[n] = bias(n);
  p.b_off = ar.add_vec(b);
}

inline ConvArgs conv_args(const PConv& p) {
  ConvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.w = p.w;
  a.bias = p.b;
  a.kind = p.kind;
  a.cs_in = p.cs_in;
  a.cs_out = p.cs_out;
  a.n_pad = p.n_pad;
  a.kp = p.kp;
  a.ntaps = p.ntaps;
  a.tpc = p.tpc;
  a.ks = p.ks;
  a.stride = p.stride;
  a.dil = p.dil;
  a.pad_left = p.pad_left;
  a.ct_u = p.ct_u;
  a.ct_pad = p.ct_pad;
  a.ct_k = p.ct_k;
  a.OH = 1;
  a.accum_div = 1.f;
  a.wscale = p.wscale;
  return a;
}

// algorithmic work of one conv launch (profiler records): flops, and compulsory traffic = input
// once, output once (+ residual / accumulator read), weights once
template <typename T>
inline void conv_cost(const ConvArgs& a, const PConv& p, double* flops_out, double* bytes_out) {
  const double rows = (double)a.M;
  const double flops = 2.0 * p.macs_per_row * rows;
  const double es = sizeof(T) * Elem<T>::R;
  // compulsory traffic: input once, output once (+ residual/accum read), weights once
  double in_rows = p.kind == KIND_CONV2D ? (double)a.IH * a.IW * (a.M / ((double)a.OH * a.OW))
                                         : (p.kind == KIND_GEMM ? rows : 0.0);
  if (p.kind == KIND_CONV1D || p.kind == KIND_CONVT) in_rows = (double)a.L_in * (a.M / (double)(p.kind == KIND_CONV1D ? a.L_out : a.L_in));
  const double out_rows = rows * (p.kind == KIND_CONVT ? p.ct_u : 1);
  const double bytes = es * (in_rows * p.cin + out_rows * p.cout * (1 + (a.res ? 1 : 0) + (a.accum ? 1 : 0)) +
                             (double)p.phases * p.cout * p.ntaps * p.cin);
  *flops_out = flops;
  *bytes_out = bytes;
}

template <typename T>
inline void run_conv(const ConvArgs& a, const PConv& p, const ConvTune& tune, hipStream_t s) {
  double flops, bytes;
  conv_cost<T>(a, p, &flops, &bytes);
  launch_conv<T>(a, tune, s, flops, bytes);
}

// TF "SAME": out = ceil(in / s), total pad = max((out - 1) * s + k - in, 0), top/left = total / 2
inline void same_pad(int in, int k, int s, int* out, int* pad) {
  *out = (in + s - 1) / s;
  if (s == 1) {
    *pad = (k - 1) / 2;  // timm static padding for odd k, stride 1
  } else {
    int total = std::max((*out - 1) * s + k - in, 0);
    *pad = total / 2;
  }
}

constexpr int EFF_STEM = 32, EFF_OUT = 208;
constexpr int SE_RD_MAX = 64;  // SE reduce width of tf_efficientnetv2_b2 is <= 52 (chan_stride <= 64)
struct StageDef {
  int type, reps, k, stride, exp, cout;
  float se;
};
constexpr StageDef kStages[6] = {{0, 2, 3, 1, 1, 16, 0.f},   {1, 3, 3, 2, 4, 32, 0.f},
                                    {1, 3, 3, 2, 4, 56, 0.f},   {2, 4, 3, 2, 4, 104, 0.25f},
                                    {2, 6, 3, 1, 6, 120, 0.25f}, {2, 10, 3, 2, 6, 208, 0.25f}};
inline int make_divisible(double v, int d = 8) { return std::max(d, (int)(v + d / 2.0) / d * d); }

// The one walk over the backbone's 28 blocks (timm's builder rules; BlockDef: model.hpp): only a stage's first
// block strides; mid = the expanded width (0 for ConvBnAct), rd = the SE reduce width (IR only).
template <class F>
inline void for_each_backbone_block(F&& f) {
  int cin = EFF_STEM, index = 0;
  for (int s = 0; s < 6; ++s) {
    const StageDef& sd = kStages[s];
    for (int r = 0; r < sd.reps; ++r) {
      const int stride = r == 0 ? sd.stride : 1, mid = sd.type == 0 ? 0 : make_divisible(cin * (double)sd.exp);
      const int rd = sd.type == 2 ? (int)std::lround(mid * (sd.se / sd.exp)) : 0;
      f(BlockDef{index++, s, r, sd.type, sd.k, stride, cin, sd.cout, mid, rd, stride == 1 && cin == sd.cout});
      cin = sd.cout;
    }
  }
}
// ... with the TF-SAME map sizes of an H x W frame carried along: the block reads (ih, iw) and writes (oh, ow);
// block 0 reads the stem's output.
struct BlockMap {
  int ih, iw, oh, ow;
};
template <class F>
inline void for_each_backbone_map(int H, int W, F&& f) {
  BlockMap m;
  int pad;
  same_pad(H, 3, 2, &m.oh, &pad);
  same_pad(W, 3, 2, &m.ow, &pad);
  for_each_backbone_block([&](const BlockDef& d) {
    m.ih = m.oh;
    m.iw = m.ow;
    same_pad(m.ih, d.k, d.stride, &m.oh, &pad);
    same_pad(m.iw, d.k, d.stride, &m.ow, &pad);
    f(d, m);
  });
}

}  // namespace m2s
