// Weight packing of the HiFi-GAN generator: host code only, no device call.  Weight norm w = g * v / ||v||
// (models.py:94-108; run_mri_video_inference.py:99-115) is folded; the transposed convs are packed per output
// phase; every resblock conv is packed for conv_gemm and, where a fused kernel takes it, in that kernel's
// fragment order (pack_rb1_frag, pack_conv1d_halo) or as e4m3 rows (pack_gemm_f8).  The order of the Arena::add
// calls is the arena layout (tests/test_pack_cpu.py pins the bytes).
#include <algorithm>
#include <cmath>

#include "pack.hpp"

namespace m2s {

namespace {

std::vector<float> fold_wn(const StateDict& sd, const std::string& p, std::vector<int64_t> shape) {
  auto it = sd.find(p + ".weight");
  if (it != sd.end()) {
    const HostTensor& t = need(sd, p + ".weight", shape);
    return std::vector<float>(t.data, t.data + t.numel());
  }
  std::vector<int64_t> gs(shape.size(), 1);
  gs[0] = shape[0];
  const HostTensor& g = need(sd, p + ".weight_g", gs);
  const HostTensor& v = need(sd, p + ".weight_v", shape);
  const size_t inner = v.numel() / shape[0];
  std::vector<float> w(v.numel());
  for (int64_t i = 0; i < shape[0]; ++i) {
    double acc = 0.0;
    for (size_t j = 0; j < inner; ++j) acc += (double)v.data[i * inner + j] * v.data[i * inner + j];
    const float sc = g.data[i] / (float)std::sqrt(acc);
    for (size_t j = 0; j < inner; ++j) w[i * inner + j] = v.data[i * inner + j] * sc;
  }
  return w;
}

constexpr size_t kFrag = 64 * 8;  // elements of one bf16 fragment

// One resblock conv (C, C, k), weight norm folded, and its bias
struct RbWeights {
  std::vector<float> wv;
  const float* bias;
  int C, k;
  auto tap(int t) const {  // (n, c) of tap t as the fragment writers ask for it, zero past the last tap
    return [this, t](int n, int c) { return t < k ? wv[((size_t)n * C + c) * k + t] : 0.f; };
  }
};

// mrf_fused.hip: [tap][hi/lo if split][n16][k32][lane][8], taps padded to the kernel's tap group with zeros
size_t pack_rb1_frag(Arena& ar, const RbWeights& w, bool split) {
  const int taps = rb1_frag_taps(w.C, w.k, split), nt16 = w.C / 16, k32 = w.C / 32, planes = split ? 2 : 1;
  std::vector<uint16_t> f((size_t)taps * planes * nt16 * k32 * kFrag);
  size_t o = 0;
  for (int t = 0; t < taps; ++t)
    for (int pl = 0; pl < planes; ++pl)
      for (int nt = 0; nt < nt16; ++nt)
        for (int kc = 0; kc < k32; ++kc, o += kFrag)
          frag_bf16(&f[o], !split ? Plane::bf16 : pl == 0 ? Plane::hi : Plane::lo, nt, kc, w.tap(t));
  return ar.add_vec(f);
}

// conv1d_halo.hip (split only): [tap][k32][hi/lo][n16][lane][8]
size_t pack_conv1d_halo(Arena& ar, const RbWeights& w) {
  std::vector<uint16_t> f(conv1d_halo_frag_elems(w.C, w.k));
  size_t o = 0;
  for (int t = 0; t < w.k; ++t)
    for (int kc = 0; kc < w.C / 32; ++kc)
      for (int pl = 0; pl < 2; ++pl)
        for (int nt = 0; nt < w.C / 16; ++nt, o += kFrag) frag_bf16(&f[o], pl == 0 ? Plane::hi : Plane::lo, nt, kc, w.tap(t));
  return ar.add_vec(f);
}

// Reach (m2s.config.generator_reach is the same rule): the interval of input positions that output frame 0, the
// samples 0 .. hop - 1, depends on, carried from the waveform back to the mel.  conv_post and conv_pre read 6
// positions ahead; a causal MRF stage reads sum((k - 1) d [+ (k - 1) for ResBlock1's second conv]) positions
// back, the largest over its kernel sizes; a transposed conv of rate u, kernel k, padding p reads inputs
// ceil((n + p - k + 1) / u) .. floor((n + p) / u) for output n.  Level l is the input of upsampler l.
void generator_reach(const m2s_hifigan_h& h, VocoderPlan& p) {
  auto fdiv = [](long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
  long lo = 0, hi = p.hop - 1 + 6, scale = p.hop;
  for (int i = h.n_up - 1; i >= 0; --i) {
    long mrf = 0;
    for (int j = 0; j < h.n_kernels; ++j) {
      long r = 0;
      for (int d = 0; d < h.n_dilations[j]; ++d)
        r += (long)(h.resblock_kernel_sizes[j] - 1) * (h.resblock_dilation_sizes[j][d] + (h.resblock == 1 ? 1 : 0));
      mrf = std::max(mrf, r);
    }
    const long u = h.upsample_rates[i], k = h.upsample_kernel_sizes[i], pad = (k - u) / 2;
    lo = -fdiv(-(lo - mrf + pad - k + 1), u);
    hi = fdiv(hi + pad, u);
    scale /= u;
    p.lvl_back[i] = (int)-fdiv(lo, scale);
    p.lvl_ahead[i] = (int)fdiv(hi, scale);
  }
  p.back = (int)-lo;
  p.ahead = (int)hi + 6;
}

}  // namespace

void pack_vocoder(const StateDict& sd, const m2s_hifigan_h& h, int dtype, const VocPackWants& wants, Arena& ar,
                  VocoderPlan& p) {
  check_generator_config(h, dtype);
  M2S_CHECK(wants.rbs.size() == (size_t)h.n_up * h.n_kernels, "pack_vocoder: one RbWants per resblock");
  // fp8 engines: e4m3 resblock (MRF) convs at C = 64 / 128 / 256; conv_pre, the upsamplers and the fused
  // C = 32 ResBlock1 kernel stay bf16
  const int io_dt = dtype == M2S_DT_FP8 ? M2S_DT_BF16 : dtype;
  const int c0 = h.upsample_initial_channel;
  {  // conv_pre: Conv1d(num_mels, c0, 7), no weight norm (models.py:94)
    const HostTensor& w = need(sd, "conv_pre.weight", {c0, h.num_mels, 7});
    const HostTensor& b = need(sd, "conv_pre.bias", {c0});
    p.pre = make_pconv(KIND_CONV1D, h.num_mels, c0, 7, io_dt);
    p.pre.ks = 7;
    p.pre.pad_left = 0;  // F.pad(x, (0, 6)): look-ahead of 6 frames, zeros past the end
    p.pre.macs_per_row = (double)c0 * h.num_mels * 7;
    const int ci = h.num_mels;
    pack_conv(ar, io_dt, p.pre, [&](int, int n, int t, int c) { return w.data[((size_t)n * ci + c) * 7 + t]; },
              [&](int n) { return b.data[n]; });
  }
  p.hop = 1;
  for (int i = 0; i < h.n_up; ++i) {
    const int u = h.upsample_rates[i], k = h.upsample_kernel_sizes[i];
    const int ci = c0 >> i, co = c0 >> (i + 1);
    M2S_CHECK(co >= 4, "generator too narrow");
    // ConvTranspose1d(k, u, padding (k-u)/2) (models.py:98-101) gives L*u outputs only when k - u is
    // even and non-negative; the polyphase packing and conv_post's look-ahead assume exactly L*u
    M2S_CHECK(u >= 1 && k >= u && (k - u) % 2 == 0,
              "upsample kernel " + std::to_string(k) + " / rate " + std::to_string(u) +
                  ": k - u must be even and >= 0 (output length L*u)");
    p.hop *= u;
    const std::string up = "ups." + std::to_string(i);
    std::vector<float> w = fold_wn(sd, up, {ci, co, k});  // ConvTranspose1d weight (in, out, k)
    const HostTensor& b = need(sd, up + ".bias", {co});
    PConv pc = make_pconv(KIND_CONVT, ci, co, (k + u - 1) / u, io_dt);
    pc.phases = u;
    pc.ct_u = u;
    pc.ct_pad = (k - u) / 2;
    pc.ct_k = k;
    pc.macs_per_row = (double)ci * co * k / u;  // per output position, averaged over phases
    const int pad = pc.ct_pad;
    pack_conv(ar, io_dt, pc,
              [&](int ph, int n, int t, int c) {
                const int j = (ph + pad) % u + t * u;  // tap t of phase ph uses kernel index j
                return j < k ? w[((size_t)c * co + n) * k + j] : 0.f;
              },
              [&](int n) { return b.data[n]; });
    p.ups.push_back(pc);
    for (int j = 0; j < h.n_kernels; ++j) {
      RB rb;
      rb.k = h.resblock_kernel_sizes[j];
      const int kk = rb.k;
      for (int d = 0; d < h.n_dilations[j]; ++d) rb.dil.push_back(h.resblock_dilation_sizes[j][d]);
      const std::string q = "resblocks." + std::to_string(i * h.n_kernels + j);
      const bool fsplit = dtype == M2S_DT_BF16X3;
      // which extra copies the resblock's convs get (voc_route.hpp voc_pack_wants)
      const RbWants& want = wants.rbs[(size_t)i * h.n_kernels + j];
      auto load = [&](const std::string& name) {
        return RbWeights{fold_wn(sd, name, {co, co, kk}), need(sd, name + ".bias", {co}).data, co, kk};
      };
      auto dense = [&](const RbWeights& w, int dil) {  // the conv_gemm packing
        PConv c = make_pconv(KIND_CONV1D, co, co, kk, dtype);
        c.ks = kk;
        c.dil = dil;
        c.pad_left = (kk - 1) * dil;  // get_padding(k, d) = k*d - d, then truncation: causal (utils.py:33-34)
        c.macs_per_row = (double)co * co * kk;
        pack_conv(ar, dtype, c, [&](int, int n, int t, int cc) { return w.wv[((size_t)n * co + cc) * kk + t]; },
                  [&](int n) { return w.bias[n]; });
        return c;
      };
      auto e4m3 = [&](const RbWeights& w) {
        RB::F8 f;
        pack_gemm_f8(
            ar, kk * co, co, co, round_up(kk * co, 128),
            [&](int n, int kx) { return w.wv[((size_t)n * co + kx % co) * kk + kx / co]; },  // K = tap-major t C + c
            [&](int n) { return w.bias[n]; }, &f.w, &f.s, &f.b);
        return f;
      };
      for (size_t d = 0; d < rb.dil.size(); ++d) {
        if (h.resblock == 2) {
          rb.c1.push_back(dense(load(q + ".convs." + std::to_string(d)), rb.dil[d]));
          continue;
        }
        const RbWeights w1 = load(q + ".convs1." + std::to_string(d));
        rb.c1.push_back(dense(w1, rb.dil[d]));
        const RbWeights w2 = load(q + ".convs2." + std::to_string(d));
        rb.c2.push_back(dense(w2, 1));
        if (want.frag) {
          rb.f1_off.push_back(pack_rb1_frag(ar, w1, fsplit));
          rb.f2_off.push_back(pack_rb1_frag(ar, w2, fsplit));
        }
        if (want.halo) {
          rb.h1_off.push_back(pack_conv1d_halo(ar, w1));
          rb.h2_off.push_back(pack_conv1d_halo(ar, w2));
        }
        if (want.q8) {
          rb.q1.push_back(e4m3(w1));
          rb.q2.push_back(e4m3(w2));
        }
      }
      p.rbs.push_back(rb);
    }
  }
  p.post_c = c0 >> h.n_up;
  {
    std::vector<float> w = fold_wn(sd, "conv_post", {1, p.post_c, 7});
    const HostTensor& b = need(sd, "conv_post.bias", {1});
    std::vector<float> wt((size_t)7 * p.post_c);
    for (int c = 0; c < p.post_c; ++c)
      for (int t = 0; t < 7; ++t) wt[(size_t)t * p.post_c + c] = w[(size_t)c * 7 + t];
    p.post_w = ar.add_vec(wt);
    p.post_b = b.data[0];
  }
  generator_reach(h, p);
}

}  // namespace m2s
