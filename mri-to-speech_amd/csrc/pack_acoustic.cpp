// Weight packing of the acoustic model (CNN + BiLSTM + head): host code only, no device call.  It mirrors what
// the reference does at load time and folds what is constant at inference:
//   * BatchNorm (eps 1e-3, torch's alpha = w / sqrt(var + eps), beta = b - mean * alpha) into
//     the preceding conv (timm BatchNormAct2d);
//   * the grey -> RGB repeat (mri_acoustic_model.py:43-44) into conv_stem (sum over in-channels);
//   * LSTM b_ih + b_hh.
// Every fused EdgeResidual kernel has its packer here (pack_er_*): it keeps the kernel's stage / piece order and
// writes each operand tile through pack.hpp's fragment writers.  The order of the Arena::add calls is the arena
// layout (tests/test_pack_cpu.py pins the bytes).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pack.hpp"

namespace m2s {

StateDict make_state_dict(const m2s_tensor* t, int n) {
  StateDict sd;
  for (int i = 0; i < n; ++i) {
    M2S_CHECK(t[i].name != nullptr, "state dict entry without a name");
    if (t[i].elem != M2S_ELEM_F32) continue;  // num_batches_tracked etc.
    M2S_CHECK(t[i].ndim >= 0 && t[i].ndim <= 4, std::string("bad ndim for ") + t[i].name);
    HostTensor h;
    h.data = static_cast<const float*>(t[i].data);
    for (int d = 0; d < t[i].ndim; ++d) h.shape.push_back(t[i].shape[d]);
    sd[t[i].name] = h;
  }
  return sd;
}

size_t Arena::add(const void* p, size_t bytes) {
  size_t off = (host_.size() + 255) & ~size_t(255);
  host_.resize(off + bytes);
  if (bytes) std::memcpy(host_.data() + off, p, bytes);
  bytes_ = host_.size();
  return off;
}

namespace {

struct BN {
  std::vector<float> a, b;
};
BN fold_bn(const StateDict& sd, const std::string& p, int c) {
  const float* w = need(sd, p + ".weight", {c}).data;
  const float* bb = need(sd, p + ".bias", {c}).data;
  const float* m = need(sd, p + ".running_mean", {c}).data;
  const float* v = need(sd, p + ".running_var", {c}).data;
  BN r;
  r.a.resize(c);
  r.b.resize(c);
  for (int i = 0; i < c; ++i) {
    const float invstd = 1.0f / std::sqrt(v[i] + 1e-3f);
    r.a[i] = invstd * w[i];
    r.b[i] = bb[i] - m[i] * r.a[i];
  }
  return r;
}

// One EdgeResidual block's BatchNorm-folded weights as the fused kernels index them; zero outside the real
// channels and taps, so a packer never restates a bound.
struct ErWeights {
  const float *we, *wq;  // conv_exp (mid, cin, 3, 3), conv_pwl (cout, mid)
  const BN *e1, *e2;
  int cin, cs_in, mid, cout, cs_out;
  float exp_at(int n, int c, int t) const {
    return n < mid && c < cin && t < 9 ? we[((size_t)n * cin + c) * 9 + t] * e1->a[n] : 0.f;
  }
  // conv_exp in the kernels' K order, k = tap * cs_in + channel
  float exp(int n, int k) const { return exp_at(n, k % cs_in, k / cs_in); }
  float pwl(int n, int c) const { return n < cout && c < mid ? wq[(size_t)n * mid + c] * e2->a[n] : 0.f; }
};
constexpr size_t kFrag = 64 * 8;  // elements of one bf16 fragment

// er_fused.hip (32 -> 128 -> 32): conv_exp [tap][n16][lane][8]; conv_pwl [n16][k-step][lane][8], permuted K
void pack_er_fused(Arena& ar, const ErWeights& w, Block& b) {
  std::vector<uint16_t> fe(9 * 8 * kFrag), fp(2 * 4 * kFrag);
  auto exp = [&](int n, int k) { return w.exp(n, k); };
  auto pwl = [&](int n, int c) { return w.pwl(n, c); };
  for (int t = 0; t < 9; ++t)
    for (int nt = 0; nt < 8; ++nt) frag_bf16(&fe[(t * 8 + nt) * kFrag], Plane::bf16, nt, t, exp);
  for (int on = 0; on < 2; ++on)
    for (int ks = 0; ks < 4; ++ks) frag_bf16_pwl(&fp[(on * 4 + ks) * kFrag], Plane::bf16, on, ks, pwl);
  b.er_wexp = ar.add_vec(fe);
  b.er_wpwl = ar.add_vec(fp);
  b.er_frag = true;
}

// er8_fused.hip (the same block on e4m3): conv_exp [q][n16][half][lane][16 B], lane group g of K step q = tap
// 4 q + g (zero past tap 8), byte b = input channel b; conv_pwl [n16][half][lane][16 B] in e4m3_pwl_channel order
void pack_er8(Arena& ar, const ErWeights& w, Block& b) {
  const std::vector<float> s1 = channel_scales(128, 9 * w.cs_in, [&](int n, int k) { return w.exp(n, k); });
  const std::vector<float> s2 = channel_scales(32, 128, [&](int n, int c) { return w.pwl(n, c); });
  std::vector<uint8_t> f8e((size_t)3 * 8 * 2 * 1024, 0), f8p((size_t)2 * 2 * 1024, 0);
  for (int q = 0; q < 3; ++q)
    for (int nt = 0; nt < 8; ++nt)
      for (int h = 0; h < 2; ++h)
        frag_e4m3(&f8e[(size_t)((q * 8 + nt) * 2 + h) * 1024], nt, h, s1, 128,
                  [&](int n, int g, int bb) { return w.exp_at(n, bb, 4 * q + g); });
  for (int on = 0; on < 2; ++on)
    for (int h = 0; h < 2; ++h)
      frag_e4m3(&f8p[(size_t)(on * 2 + h) * 1024], on, h, s2, 32,
                [&](int n, int g, int bb) { return w.pwl(n, e4m3_pwl_channel(g, bb)); });
  b.er8_wexp = ar.add_vec(f8e);
  b.er8_sexp = ar.add_vec(s1);
  b.er8_wpwl = ar.add_vec(f8p);
  b.er8_spwl = ar.add_vec(s2);
  b.er8 = true;
}

// er2_fused.hip (56 -> 224 -> 56) stage stream [20][16 pieces][lane][8]: stages 0..17 = conv_exp k-step s (tap
// s / 2, input channels 32 (s % 2) ..), piece = n16; stages 18 / 19 = conv_pwl k-steps 0..3 / 4..6, piece =
// local k-step * 4 + n16, permuted K
void pack_er2_fused(Arena& ar, const ErWeights& w, Block& b) {
  std::vector<uint16_t> st((size_t)er2_stage_elems(), 0);
  for (int sg = 0; sg < 20; ++sg)
    for (int pc = 0; pc < 16; ++pc) {
      uint16_t* dst = &st[((size_t)sg * 16 + pc) * kFrag];
      if (sg < 18)
        frag_bf16(dst, Plane::bf16, pc, sg, [&](int n, int k) { return w.exp(n, k); });
      else
        frag_bf16_pwl(dst, Plane::bf16, pc & 3, (sg == 18 ? 0 : 4) + (pc >> 2), [&](int n, int c) { return w.pwl(n, c); });
    }
  b.er_wexp = ar.add_vec(st);
  b.er_frag = true;
}

// er8w_fused.hip (the same block on e4m3) stage stream: conv_exp K step q = [n16 0..15][half][lane][16 B], lane
// group g = tap 2 q + (g >> 1), byte b = input channel 32 (g & 1) + b (zero past tap 8, channel 55, mid channel
// 223); then conv_pwl [n16][kq][half][lane][16 B], byte b = mid channel 128 kq + e4m3_pwl_channel(g, b)
void pack_er8w(Arena& ar, const ErWeights& w, Block& b) {
  const std::vector<float> s1 = channel_scales(w.mid, 9 * w.cs_in, [&](int n, int k) { return w.exp(n, k); });
  const std::vector<float> s2 = channel_scales(w.cout, w.mid, [&](int n, int c) { return w.pwl(n, c); }, 64);
  std::vector<uint8_t> w8(er8w_stream_bytes(), 0);
  for (int q = 0; q < 5; ++q)
    for (int nt = 0; nt < 16; ++nt)
      for (int h = 0; h < 2; ++h)
        frag_e4m3(&w8[(size_t)((q * 16 + nt) * 2 + h) * 1024], nt, h, s1, w.mid,
                  [&](int n, int g, int bb) { return w.exp_at(n, 32 * (g & 1) + bb, 2 * q + (g >> 1)); });
  const size_t pw0 = (size_t)5 * 32 * 1024;
  for (int on = 0; on < 4; ++on)
    for (int kq = 0; kq < 2; ++kq)
      for (int h = 0; h < 2; ++h)
        frag_e4m3(&w8[pw0 + (size_t)((on * 2 + kq) * 2 + h) * 1024], on, h, s2, w.cout,
                  [&](int n, int g, int bb) { return w.pwl(n, 128 * kq + e4m3_pwl_channel(g, bb)); });
  b.er8w_w = ar.add_vec(w8);
  b.er8w_sexp = ar.add_vec(s1);
  b.er8w_spwl = ar.add_vec(s2);
  b.er8w = true;
}

// ers2_fused.hip (stride 2): conv_exp [k-step][n16][lane][8] in K order (cs_in 16: two taps a k-step), conv_pwl
// [n16][k-step][lane][8], permuted K.  The split kernel (ers2_sp_kernel) reads the same orders as [hi | lo] planes.
void pack_ers2_fused(Arena& ar, const ErWeights& w, bool split, Block& b) {
  const int ks_n = (9 * w.cs_in + 31) / 32, ntn = w.mid / 16, onn = w.cs_out / 16, pkn = w.mid / 32;
  const size_t fe_n = (size_t)ks_n * ntn * kFrag, fp_n = (size_t)onn * pkn * kFrag;
  const int planes = split ? 2 : 1;
  std::vector<uint16_t> fe(planes * fe_n, 0), fp(planes * fp_n, 0);
  for (int pl = 0; pl < planes; ++pl) {
    const Plane plane = !split ? Plane::bf16 : pl == 0 ? Plane::hi : Plane::lo;
    for (int ks = 0; ks < ks_n; ++ks)
      for (int nt = 0; nt < ntn; ++nt)
        frag_bf16(&fe[pl * fe_n + ((size_t)ks * ntn + nt) * kFrag], plane, nt, ks, [&](int n, int k) { return w.exp(n, k); });
    for (int on = 0; on < onn; ++on)
      for (int ks = 0; ks < pkn; ++ks)
        frag_bf16_pwl(&fp[pl * fp_n + ((size_t)on * pkn + ks) * kFrag], plane, on, ks, [&](int n, int c) { return w.pwl(n, c); });
  }
  b.er_wexp = ar.add_vec(fe);
  b.er_wpwl = ar.add_vec(fp);
  (split ? b.ers_sp : b.er_frag) = true;
}

// er_sp_fused.hip stage stream: per conv_exp k-step (tap, 32 input channels) a W_hi and a W_lo stage of nt
// fragments [n16][lane][8]; then conv_pwl's W_hi stages and W_lo stages, piece j = (k-step j / ON, n16 j % ON),
// permuted K
void pack_er_sp(Arena& ar, const ErWeights& w, Block& b) {
  int nt = 0;
  const int nst = er_sp_nt_stages(w.cs_in, w.mid, w.cs_out, &nt);
  const int nce = 9 * (w.cs_in / 32) * 2, on_n = w.cs_out / 16, pn = on_n * (w.mid / 32), nps = (pn + nt - 1) / nt;
  std::vector<uint16_t> st((size_t)nst * nt * kFrag, 0);
  for (int sg = 0; sg < nst; ++sg)
    for (int pc = 0; pc < nt; ++pc) {
      uint16_t* dst = &st[((size_t)sg * nt + pc) * kFrag];
      if (sg < nce) {
        frag_bf16(dst, sg & 1 ? Plane::lo : Plane::hi, pc, sg >> 1, [&](int n, int k) { return w.exp(n, k); });
      } else {
        const int j = ((sg - nce) % nps) * nt + pc;
        if (j < pn)
          frag_bf16_pwl(dst, (sg - nce) / nps ? Plane::lo : Plane::hi, j % on_n, j / on_n,
                        [&](int n, int c) { return w.pwl(n, c); });
      }
    }
  b.er_sp_w = ar.add_vec(st);
  b.er_sp = true;
}

}  // namespace

void pack_acoustic(const StateDict& sd, int n_mels, int hidden, int dtype, Arena& ar, AcousticPlan& p) {
  M2S_CHECK(dtype == M2S_DT_F32 || dtype == M2S_DT_BF16 || dtype == M2S_DT_BF16X3 || dtype == M2S_DT_FP8, "bad dtype");
  M2S_CHECK(n_mels > 0 && hidden > 0 && hidden % 8 == 0, "bad n_mels / rnn_hidden");
  const std::string P = "cnn.backbone.";
  {  // stem: fold repeat(1,3,1,1) by summing the 3 input channels; then BN
    const float* w = need(sd, P + "conv_stem.weight", {EFF_STEM, 3, 3, 3}).data;
    BN bn = fold_bn(sd, P + "bn1", EFF_STEM);
    std::vector<float> w9(EFF_STEM * 9);
    for (int o = 0; o < EFF_STEM; ++o)
      for (int t = 0; t < 9; ++t)
        w9[o * 9 + t] = (w[(o * 3 + 0) * 9 + t] + w[(o * 3 + 1) * 9 + t] + w[(o * 3 + 2) * 9 + t]) * bn.a[o];
    p.stem_w = ar.add_vec(w9);
    p.stem_b = ar.add_vec(bn.b);
  }
  // fp8 engines run the bf16 kernels (and bf16 packings) except the stride-1 IR blocks' SE-gated conv_pwl,
  // which gets an e4m3 copy for the block-scaled MFMA (gemm128.hip) below
  const int pdt = dtype == M2S_DT_FP8 ? M2S_DT_BF16 : dtype;
  for_each_backbone_block([&](const BlockDef& d) {
    Block b{d};
    const std::string q = d.key();
    const int k = d.k, cin = d.cin;
    // a dense conv with its BatchNorm folded: weight (co, ci, k, k) or (co, ci, 1, 1)
    auto conv2d_kxk = [&](PConv& pc, const float* w, int ci, int co, const BN& bn) {
      pc = make_pconv(KIND_CONV2D, ci, co, k * k, pdt);
      pc.ks = k;
      pc.stride = b.stride;
      pc.macs_per_row = (double)co * ci * k * k;
      pack_conv(ar, pdt, pc, [&](int, int n, int t, int c) { return w[((size_t)n * ci + c) * k * k + t] * bn.a[n]; },
                [&](int n) { return bn.b[n]; });
    };
    auto conv1x1 = [&](PConv& pc, const float* w, int ci, int co, const BN& bn) {
      pc = make_pconv(KIND_GEMM, ci, co, 1, pdt);
      pc.macs_per_row = (double)co * ci;
      pack_conv(ar, pdt, pc, [&](int, int n, int, int c) { return w[(size_t)n * ci + c] * bn.a[n]; },
                [&](int n) { return bn.b[n]; });
    };
    if (b.type == 0) {
      const BN bn1 = fold_bn(sd, q + "bn1", b.cout);
      conv2d_kxk(b.c1, need(sd, q + "conv.weight", {b.cout, cin, k, k}).data, cin, b.cout, bn1);
    } else if (b.type == 1) {
      const BN e1 = fold_bn(sd, q + "bn1", b.mid);
      const float* we = need(sd, q + "conv_exp.weight", {b.mid, cin, k, k}).data;
      conv2d_kxk(b.c1, we, cin, b.mid, e1);
      const BN e2 = fold_bn(sd, q + "bn2", b.cout);
      const float* wq = need(sd, q + "conv_pwl.weight", {b.cout, b.mid, 1, 1}).data;
      conv1x1(b.c2, wq, b.mid, b.cout, e2);
      // the fused kernels' copies: the first kernel that supports the block at its benched map size
      const int csi = b.c1.cs_in, cso = chan_stride(b.cout);
      const ErWeights w{we, wq, &e1, &e2, cin, csi, b.mid, b.cout, cso};
      const bool s1 = b.stride == 1 && b.skip && k == 3, s2 = b.stride == 2 && k == 3;
      if (dtype == M2S_DT_BF16X3 && s1 && er_sp_supported(32, 32, csi, b.mid, cso)) {
        pack_er_sp(ar, w, b);
      } else if (dtype == M2S_DT_BF16X3 && s2 && ers2_sp_supported(8, 16, csi, b.mid, cso)) {
        pack_ers2_fused(ar, w, true, b);
      } else if (pdt == M2S_DT_BF16 && s1 && er_fused_supported(64, 64, cin, b.mid, b.cout, b.c1.kp, b.c2.kp)) {
        pack_er_fused(ar, w, b);
        if (dtype == M2S_DT_FP8) pack_er8(ar, w, b);
      } else if (pdt == M2S_DT_BF16 && s1 && er2_fused_supported(32, 32, csi, b.mid, b.cout, b.c1.kp, b.c2.kp)) {
        pack_er2_fused(ar, w, b);
        if (dtype == M2S_DT_FP8 && er8w_fused_supported(32, 32, csi, b.mid, b.cout)) pack_er8w(ar, w, b);
      } else if (pdt == M2S_DT_BF16 && s2 && ers2_fused_supported(8, 16, csi, b.mid, cso, b.c1.kp, b.c2.kp)) {
        pack_ers2_fused(ar, w, false, b);
      }
    } else {
      const int m = b.mid, cs = chan_stride(m), rd = b.rd;
      p.max_mid_cs = std::max(p.max_mid_cs, cs);
      const BN bn1 = fold_bn(sd, q + "bn1", m);
      const float* wp = need(sd, q + "conv_pw.weight", {m, cin, 1, 1}).data;
      conv1x1(b.c1, wp, cin, m, bn1);
      // the e4m3 expand (ir_pwdw / ir_pwdw_s2 x8; the stride-2 blocks' copy is used where ir_pwdw_s2 runs, blocks.5.0)
      if (dtype == M2S_DT_FP8 && chan_stride(cin) <= 256) {
        size_t boff = 0;
        b.f8x_kp = round_up(chan_stride(cin), 128);
        pack_gemm_f8(ar, cin, m, round_up(cs, 32), b.f8x_kp, [&](int n, int c) { return wp[(size_t)n * cin + c] * bn1.a[n]; },
                     [&](int n) { return bn1.b[n]; }, &b.f8x_w, &b.f8x_s, &boff);
        b.f8_pw = true;
      }
      const float* wd = need(sd, q + "conv_dw.weight", {m, 1, k, k}).data;
      const BN bn2 = fold_bn(sd, q + "bn2", m);
      std::vector<float> w9((size_t)cs * 9, 0.f), bd(cs, 0.f);
      for (int c = 0; c < m; ++c) {
        for (int t = 0; t < 9; ++t) w9[(size_t)t * cs + c] = wd[(size_t)c * 9 + t] * bn2.a[c];  // tap-major
        bd[c] = bn2.b[c];
      }
      b.dw_w = ar.add_vec(w9);
      b.dw_b = ar.add_vec(bd);
      if (pdt == M2S_DT_BF16) {  // fused kernel: bf16 weight in the half matching the channel
        std::vector<uint32_t> w2(w9.size());  // (v_dot2 against a (c, c+1) activation dword)
        for (size_t i = 0; i < w9.size(); ++i) {
          const uint32_t h = f2bf_host(w9[i]);
          w2[i] = (i % cs) % 2 == 0 ? h : h << 16;
        }
        b.dw_w2 = ar.add_vec(w2);
      }
      const float* w1 = need(sd, q + "se.conv_reduce.weight", {rd, m, 1, 1}).data;
      const float* b1 = need(sd, q + "se.conv_reduce.bias", {rd}).data;
      const float* w2 = need(sd, q + "se.conv_expand.weight", {m, rd, 1, 1}).data;
      const float* b2 = need(sd, q + "se.conv_expand.bias", {m}).data;
      // SE excitation as two GEMMs over all images: (N x mid) . W1^T -> SiLU -> . W2^T -> sigmoid
      // (fp8 engines keep the SE excitation in bf16: a gate error scales the whole block output)
      const int se_dt = dtype == M2S_DT_FP8 ? M2S_DT_BF16 : dtype;
      b.se1 = make_pconv(KIND_GEMM, m, rd, 1, se_dt);
      b.se1.macs_per_row = (double)m * rd;
      pack_conv(ar, se_dt, b.se1, [&](int, int n, int, int c) { return w1[(size_t)n * m + c]; },
                [&](int n) { return b1[n]; });
      b.se2 = make_pconv(KIND_GEMM, rd, m, 1, se_dt);
      b.se2.macs_per_row = (double)m * rd;
      pack_conv(ar, se_dt, b.se2, [&](int, int n, int, int c) { return w2[(size_t)n * rd + c]; },
                [&](int n) { return b2[n]; });
      const BN bn3 = fold_bn(sd, q + "bn3", b.cout);
      const float* wl = need(sd, q + "conv_pwl.weight", {b.cout, m, 1, 1}).data;
      conv1x1(b.c2, wl, m, b.cout, bn3);
      if (dtype == M2S_DT_FP8 && chan_stride(b.cout) <= 224) {  // (stride 2: used with ir_pwdw_s2's e4m3 output)
        b.f8_kp = round_up(cs, 128);
        b.f8_npad = std::max(round_up(chan_stride(b.cout), 64), chan_stride(b.cout) > 128 ? 224 : 128);
        pack_gemm_f8(ar, m, b.cout, b.f8_npad, b.f8_kp, [&](int n, int c) { return wl[(size_t)n * m + c] * bn3.a[n]; },
                     [&](int n) { return bn3.b[n]; }, &b.f8_w, &b.f8_s, &b.f8_b);
        b.f8_pwl = true;
      }
    }
    p.blocks.push_back(b);
  });
  // BiLSTM: input projection of both directions as one fp32 GEMM (rows [fwd 4H | bwd 4H]).
  const int H = hidden;
  const float* wih[2] = {need(sd, "rnn.lstm.weight_ih_l0", {4 * H, EFF_OUT}).data,
                         need(sd, "rnn.lstm.weight_ih_l0_reverse", {4 * H, EFF_OUT}).data};
  const float* bih[2] = {need(sd, "rnn.lstm.bias_ih_l0", {4 * H}).data, need(sd, "rnn.lstm.bias_ih_l0_reverse", {4 * H}).data};
  const float* bhh[2] = {need(sd, "rnn.lstm.bias_hh_l0", {4 * H}).data, need(sd, "rnn.lstm.bias_hh_l0_reverse", {4 * H}).data};
  const float* whh[2] = {need(sd, "rnn.lstm.weight_hh_l0", {4 * H, H}).data,
                         need(sd, "rnn.lstm.weight_hh_l0_reverse", {4 * H, H}).data};
  p.lstm_ih = make_pconv(KIND_GEMM, EFF_OUT, 8 * H, 1, M2S_DT_F32);
  p.lstm_ih.cs_in = EFF_OUT;  // 208 = 13 x 16: valid fp32 K chunking without padding
  p.lstm_ih.tpc = 1;
  p.lstm_ih.kp = EFF_OUT;
  p.lstm_ih.cs_out = 8 * H;
  p.lstm_ih.n_pad = round_up(8 * H, 64);
  p.lstm_ih.macs_per_row = 8.0 * H * EFF_OUT;
  pack_conv(ar, M2S_DT_F32, p.lstm_ih,
            [&](int, int n, int, int c) { return wih[n / (4 * H)][(size_t)(n % (4 * H)) * EFF_OUT + c]; },
            [&](int n) { return bih[n / (4 * H)][n % (4 * H)] + bhh[n / (4 * H)][n % (4 * H)]; });
  std::vector<float> wh((size_t)2 * 4 * H * H);
  std::memcpy(wh.data(), whh[0], sizeof(float) * 4 * H * H);
  std::memcpy(wh.data() + (size_t)4 * H * H, whh[1], sizeof(float) * 4 * H * H);
  p.whh = ar.add_vec(wh);
  if (lstm_window_supported(H)) {  // the windowed path's copy: rows permuted so a workgroup's tile holds all four gates
    pack_lstm_window_whh(whh, H, wh.data());
    p.whh_win = ar.add_vec(wh);
  }
  const float* hw = need(sd, "head.weight", {n_mels, H}).data;
  const float* hb = need(sd, "head.bias", {n_mels}).data;
  std::vector<float> wt((size_t)H * n_mels);
  for (int n = 0; n < n_mels; ++n)
    for (int k = 0; k < H; ++k) wt[(size_t)k * n_mels + n] = hw[(size_t)n * H + k];
  p.head_wt = ar.add_vec(wt);
  p.head_b = ar.add(hb, sizeof(float) * n_mels);
}

}  // namespace m2s
