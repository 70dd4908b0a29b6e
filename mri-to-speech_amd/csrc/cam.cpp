// Grad-CAM path host code (cam.hpp): the train-mode backbone plan and the BiLSTM / Linear autograd
// entry points.
//
// Reference behaviour (scripts/mri_gradcam_formant.py): compute_gradcam puts the model in train()
// (:223), so the backbone's BatchNorms normalise with the statistics of the B*T frames of the call and
// update their running statistics (timm BatchNormAct2d = torch BatchNorm2d, momentum 0.1, eps 1e-3);
// the last feature map is made a gradient leaf (:155-160), pooled, run through rnn and head
// (:162-165), and the band power's gradient is read back at feats.grad (:247-248).  Nothing needs the
// backbone's own backward, so the backbone here is a forward with batch statistics only.
#include "cam.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "pack.hpp"
#include "prof.hpp"

namespace m2s {

namespace {

const int kTaps[5] = {2, 5, 8, 18, 28};  // timm features_only taps: blocks run (mri_gradcam_formant.py:155-158)

}  // namespace

CamBackbone::CamBackbone(const StateDict& sd, int device) : device_(device) {
  const std::string P = "cnn.backbone.";
  auto add_bn = [&](const std::string& p, int c) {
    BNp b;
    b.C = c;
    b.g = arena_.add(need(sd, p + ".weight", {c}).data, sizeof(float) * c);
    b.b = arena_.add(need(sd, p + ".bias", {c}).data, sizeof(float) * c);
    bn_.push_back(b);
    return (int)bn_.size() - 1;
  };
  {  // grey repeated to RGB: the three input-channel taps of conv_stem summed
    const float* w = need(sd, P + "conv_stem.weight", {EFF_STEM, 3, 3, 3}).data;
    std::vector<float> w9(EFF_STEM * 9);
    for (int o = 0; o < EFF_STEM; ++o)
      for (int t = 0; t < 9; ++t) w9[o * 9 + t] = w[(o * 3 + 0) * 9 + t] + w[(o * 3 + 1) * 9 + t] + w[(o * 3 + 2) * 9 + t];
    stem_w_ = arena_.add_vec(w9);
    stem_bn_ = add_bn(P + "bn1", EFF_STEM);
  }
  auto zero = [](int) { return 0.f; };
  for_each_backbone_block([&](const BlockDef& d) {
    Blk b{d};
    const std::string q = d.key();
    const int cin = d.cin;
    auto conv3 = [&](PConv& pc, const std::string& wk, int ci, int co) {
      const float* w = need(sd, wk, {co, ci, 3, 3}).data;
      pc = make_pconv(KIND_CONV2D, ci, co, 9, M2S_DT_F32);
      pc.ks = 3;
      pc.stride = b.stride;
      pc.macs_per_row = 9.0 * co * ci;
      pack_conv(arena_, M2S_DT_F32, pc, [&](int, int n, int t, int c) { return w[((size_t)n * ci + c) * 9 + t]; }, zero);
    };
    auto conv1 = [&](PConv& pc, const std::string& wk, int ci, int co) {
      const float* w = need(sd, wk, {co, ci, 1, 1}).data;
      pc = make_pconv(KIND_GEMM, ci, co, 1, M2S_DT_F32);
      pc.macs_per_row = (double)co * ci;
      pack_conv(arena_, M2S_DT_F32, pc, [&](int, int n, int, int c) { return w[(size_t)n * ci + c]; }, zero);
    };
    if (b.type == 0) {
      conv3(b.c1, q + "conv.weight", cin, b.cout);
      b.bn[0] = add_bn(q + "bn1", b.cout);
    } else if (b.type == 1) {
      conv3(b.c1, q + "conv_exp.weight", cin, b.mid);
      b.bn[0] = add_bn(q + "bn1", b.mid);
      conv1(b.c2, q + "conv_pwl.weight", b.mid, b.cout);
      b.bn[1] = add_bn(q + "bn2", b.cout);
    } else {
      const int m = b.mid, cs = chan_stride(m), rd = b.rd;
      conv1(b.c1, q + "conv_pw.weight", cin, m);
      b.bn[0] = add_bn(q + "bn1", m);
      const float* wd = need(sd, q + "conv_dw.weight", {m, 1, 3, 3}).data;
      std::vector<float> w9((size_t)cs * 9, 0.f);
      for (int c = 0; c < m; ++c)
        for (int t = 0; t < 9; ++t) w9[(size_t)t * cs + c] = wd[(size_t)c * 9 + t];
      b.dw = arena_.add_vec(w9);
      b.bn[1] = add_bn(q + "bn2", m);
      const float* w1 = need(sd, q + "se.conv_reduce.weight", {rd, m, 1, 1}).data;
      const float* b1 = need(sd, q + "se.conv_reduce.bias", {rd}).data;
      const float* w2 = need(sd, q + "se.conv_expand.weight", {m, rd, 1, 1}).data;
      const float* b2 = need(sd, q + "se.conv_expand.bias", {m}).data;
      b.se1 = make_pconv(KIND_GEMM, m, rd, 1, M2S_DT_F32);
      b.se1.macs_per_row = (double)m * rd;
      pack_conv(arena_, M2S_DT_F32, b.se1, [&](int, int n, int, int c) { return w1[(size_t)n * m + c]; },
                [&](int n) { return b1[n]; });
      b.se2 = make_pconv(KIND_GEMM, rd, m, 1, M2S_DT_F32);
      b.se2.macs_per_row = (double)m * rd;
      pack_conv(arena_, M2S_DT_F32, b.se2, [&](int, int n, int, int c) { return w2[(size_t)n * rd + c]; },
                [&](int n) { return b2[n]; });
      conv1(b.c2, q + "conv_pwl.weight", m, b.cout);
      b.bn[2] = add_bn(q + "bn3", b.cout);
    }
    blocks_.push_back(b);
  });
  arena_.upload(device);
  for (auto& b : blocks_) {
    b.c1.resolve(arena_);
    if (b.type != 0) b.c2.resolve(arena_);
    if (b.type == 2) {
      b.se1.resolve(arena_);
      b.se2.resolve(arena_);
    }
  }
}

int CamBackbone::bn_stats_floats() const {
  int n = 0;
  for (const BNp& b : bn_) n += 2 * b.C;
  return n;
}

namespace {
struct CamDims {
  size_t io = 0, mid = 0;  // per-frame floats of the block outputs / expanded maps
  int cs_mid = 0;
};
struct CamBufs {  // ping-pong block outputs, expanded maps, SE means / hidden / gates, BatchNorm partial sums
  float *A, *B, *M, *M2, *sem, *hid, *gate, *scr;
};
}  // namespace

static CamDims cam_dims(int H, int W) {
  CamDims d;
  for_each_backbone_map(H, W, [&](const BlockDef& b, const BlockMap& m) {
    if (b.type != 0) {
      const int cs = chan_stride(b.mid);
      d.mid = std::max(d.mid, (size_t)(b.type == 2 ? m.ih * m.iw : m.oh * m.ow) * cs);
      d.cs_mid = std::max(d.cs_mid, cs);
    }
    // every map a block reads or writes (block 0 reads the stem's output)
    d.io = std::max({d.io, (size_t)m.ih * m.iw * chan_stride(b.cin), (size_t)m.oh * m.ow * chan_stride(b.cout)});
  });
  return d;
}

// the backbone's scratch: the size query and the call both run this
static CamBufs cam_bufs(Workspace& w, int N, const CamDims& d) {
  CamBufs b;
  b.A = w.take<float>((size_t)N * d.io);
  b.B = w.take<float>((size_t)N * d.io);
  b.M = w.take<float>((size_t)N * d.mid);
  b.M2 = w.take<float>((size_t)N * d.mid);
  b.sem = w.take<float>((size_t)N * d.cs_mid);
  b.hid = w.take<float>((size_t)N * SE_RD_MAX);
  b.gate = w.take<float>((size_t)N * d.cs_mid);
  b.scr = w.take<float>(bn_train_scratch_floats(0, std::max(d.cs_mid, 256)));
  return b;
}

size_t CamBackbone::workspace_bytes(int N, int H, int W) const {
  return Workspace::bytes([&](Workspace& w) { cam_bufs(w, N, cam_dims(H, W)); });
}

void CamBackbone::forward(const float* frames, int N, int H, int W, float* const taps[5], float* bn_stats, void* ws,
                          size_t wsb, hipStream_t s) {
  M2S_CHECK(N > 0 && H >= 32 && W >= 32, "cam backbone: bad input size");
  const CamDims d = cam_dims(H, W);
  Workspace w(ws, wsb);
  const CamBufs cb = cam_bufs(w, N, d);
  float *const A = cb.A, *const Bf = cb.B, *const M = cb.M, *const M2 = cb.M2;
  float *const sem = cb.sem, *const hid = cb.hid, *const gate = cb.gate, *const scr = cb.scr;
  // the conv kernels index their inputs with 32-bit offsets: run them over frame chunks
  const int fc = (int)std::max<size_t>(1, std::min<size_t>(N, 2147483647ull / std::max(d.io, d.mid)));
  std::vector<size_t> st_off(bn_.size());
  {
    size_t o = 0;
    for (size_t i = 0; i < bn_.size(); ++i) {
      st_off[i] = o;
      o += 2 * (size_t)bn_[i].C;
    }
  }
  auto bn = [&](float* x, long rows, int layer, int cs, int act, const float* res) {
    const BNp& p = bn_[layer];
    launch_bn_train(x, rows, p.C, cs, static_cast<const float*>(arena_.ptr(p.g)),
                    static_cast<const float*>(arena_.ptr(p.b)), 1e-3f, act, res, bn_stats + st_off[layer], scr, s);
  };
  int oh, ow, pt, pl;
  same_pad(H, 3, 2, &oh, &pt);
  same_pad(W, 3, 2, &ow, &pl);
  launch_stem_raw(frames, N, H, W, oh, ow, pt, pl, static_cast<const float*>(arena_.ptr(stem_w_)), A, s);
  bn(A, (long)N * oh * ow, stem_bn_, chan_stride(EFF_STEM), 1, nullptr);
  float* cur = A;
  float* nxt = Bf;
  int ti = 0;
  for (size_t k = 0; k < blocks_.size(); ++k) {
    const Blk& b = blocks_[k];
    int nh, nw, qt, ql;
    same_pad(oh, 3, b.stride, &nh, &qt);
    same_pad(ow, 3, b.stride, &nw, &ql);
    const int cso = chan_stride(b.cout), csm = b.mid ? chan_stride(b.mid) : 0;
    // one conv over all frames, chunked; in / out per-frame strides in floats
    auto conv = [&](const PConv& pc, const float* x, size_t xs, float* y, size_t ys, int IH, int IW, int OH, int OW,
                    const float* scale) {
      for (int n0 = 0; n0 < N; n0 += fc) {
        const int nc = std::min(fc, N - n0);
        ConvArgs a = conv_args(pc);
        a.x = x + (size_t)n0 * xs;
        a.y = y + (size_t)n0 * ys;
        a.M = nc * OH * OW;
        if (pc.kind == KIND_CONV2D) {
          a.IH = IH;
          a.IW = IW;
          a.OH = OH;
          a.OW = OW;
          a.pad_t = qt;
          a.pad_l = ql;
        } else {
          a.OH = OH * OW;  // rows per image (the SE gate table is per image)
        }
        if (scale) {
          a.in_xform = IN_SE_SCALE;
          a.in_scale = scale + (size_t)n0 * pc.cs_in;
        }
        run_conv<float>(a, pc, ConvTune{}, s);
      }
    };
    const size_t pin = (size_t)oh * ow, pout = (size_t)nh * nw;
    if (b.type == 0) {
      conv(b.c1, cur, pin * b.c1.cs_in, nxt, pout * cso, oh, ow, nh, nw, nullptr);
      bn(nxt, (long)N * pout, b.bn[0], cso, 1, b.skip ? cur : nullptr);
    } else if (b.type == 1) {
      conv(b.c1, cur, pin * b.c1.cs_in, M, pout * csm, oh, ow, nh, nw, nullptr);
      bn(M, (long)N * pout, b.bn[0], csm, 1, nullptr);
      conv(b.c2, M, pout * csm, nxt, pout * cso, nh, nw, nh, nw, nullptr);
      bn(nxt, (long)N * pout, b.bn[1], cso, 0, b.skip ? cur : nullptr);
    } else {
      conv(b.c1, cur, pin * b.c1.cs_in, M, pin * csm, oh, ow, oh, ow, nullptr);
      bn(M, (long)N * pin, b.bn[0], csm, 1, nullptr);
      launch_dw_raw(M, N, oh, ow, nh, nw, b.stride, qt, ql, csm, static_cast<const float*>(arena_.ptr(b.dw)), M2, s);
      bn(M2, (long)N * pout, b.bn[1], csm, 1, nullptr);
      launch_gap<float>(M2, N, (int)pout, csm, csm, sem, s);  // SE squeeze, (N, cs_mid)
      ConvArgs r1 = conv_args(b.se1);                        // conv_reduce + SiLU
      r1.x = sem;
      r1.y = hid;
      r1.M = N;
      r1.act = ACT_SILU;
      run_conv<float>(r1, b.se1, ConvTune{}, s);
      ConvArgs r2 = conv_args(b.se2);  // conv_expand + sigmoid -> gates
      r2.x = hid;
      r2.y = gate;
      r2.M = N;
      r2.act = ACT_SIGMOID;
      run_conv<float>(r2, b.se2, ConvTune{}, s);
      conv(b.c2, M2, pout * csm, nxt, pout * cso, nh, nw, nh, nw, gate);
      bn(nxt, (long)N * pout, b.bn[2], cso, 0, b.skip ? cur : nullptr);
    }
    std::swap(cur, nxt);
    oh = nh;
    ow = nw;
    if (ti < 5 && (int)k + 1 == kTaps[ti]) {
      if (taps && taps[ti]) launch_to_nchw(cur, N, oh * ow, b.cout, cso, taps[ti], s);
      ++ti;
    }
  }
}

// ---- BiLSTM / Linear autograd entry points -------------------------------------------------------
namespace {
struct LstmTrainBufs {  // one layout for the forward (pre, whh) and the backward (dg, wt, hp, dc)
  float* pre_dg;  // fwd: gate pre-activations (BT, 8H); bwd: dG (2, BT, 4H)
  float* whh_wt;  // fwd: W_hh of both directions; bwd: W_hh^T
  float *hp, *dc;  // bwd: h_prev (2, BT, H), the carried cell gradient (2, B, H)
};
}  // namespace

static LstmTrainBufs lstm_train_bufs(Workspace& w, int B, int T, int H) {
  const size_t BT = (size_t)B * T;
  LstmTrainBufs b;
  b.pre_dg = w.take<float>(std::max(BT * 8 * H, (size_t)2 * BT * 4 * H));
  b.whh_wt = w.take<float>((size_t)2 * 4 * H * H);
  b.hp = w.take<float>(std::max((size_t)2 * B * H, (size_t)2 * BT * H));
  b.dc = w.take<float>((size_t)2 * B * H);
  return b;
}

size_t bilstm_train_workspace_bytes(int B, int T, int, int H) {
  return Workspace::bytes([&](Workspace& w) { lstm_train_bufs(w, B, T, H); });
}

void bilstm_train_forward(const float* x, int B, int T, int C, int H, const float* const w_ih[2],
                          const float* const w_hh[2], const float* const b_ih[2], const float* const b_hh[2], float* y,
                          float* gates, float* cells, float* hid, void* ws, size_t wsb, hipStream_t s) {
  M2S_CHECK(B > 0 && T > 0 && C > 0 && H > 0 && H % 8 == 0, "bilstm_train: shape");
  const long BT = (long)B * T;
  Workspace w(ws, wsb);
  const LstmTrainBufs b = lstm_train_bufs(w, B, T, H);
  float *const pre = b.pre_dg, *const whh = b.whh_wt;
  for (int d = 0; d < 2; ++d) {
    // pre[bt][d*4H + n] = sum_c x[bt][c] W_ih[n][c] + b_ih[n] + b_hh[n]
    launch_gemm_f32((int)BT, 4 * H, C, x, C, 1, w_ih[d], 1, C, pre + (size_t)d * 4 * H, 8L * H, b_ih[d], b_hh[d], false, s);
    M2S_HIP(hipMemcpyAsync(whh + (size_t)d * 4 * H * H, w_hh[d], sizeof(float) * 4 * H * H, hipMemcpyDeviceToDevice, s));
  }
  for (int st = 0; st < T; ++st) launch_lstm_train_step(pre, whh, gates, cells, hid, B, T, H, st, s);
  launch_add2(hid, hid + BT * H, y, BT * H, s);
}

void bilstm_train_backward(const float* x, const float* dy, int B, int T, int C, int H, const float* const w_ih[2],
                           const float* const w_hh[2], const float* gates, const float* cells, const float* hid,
                           float* dx, float* const dw_ih[2], float* const dw_hh[2], float* const db[2], void* ws,
                           size_t wsb, hipStream_t s) {
  M2S_CHECK(B > 0 && T > 0 && C > 0 && H > 0 && H % 8 == 0, "bilstm_train: shape");
  const long BT = (long)B * T;
  const int G = 4 * H;
  Workspace w(ws, wsb);
  const LstmTrainBufs b = lstm_train_bufs(w, B, T, H);
  float *const dg = b.pre_dg, *const wt = b.whh_wt, *const hp = b.hp, *const dc = b.dc;
  for (int d = 0; d < 2; ++d) launch_transpose(w_hh[d], 1, G, H, wt + (size_t)d * G * H, s);
  for (int st = 0; st < T; ++st) launch_lstm_bptt_step(wt, dy, gates, cells, dc, dg, B, T, H, st, s);
  launch_lstm_hprev(hid, hp, B, T, H, s);
  for (int d = 0; d < 2; ++d) {
    const float* g = dg + (size_t)d * BT * G;
    if (dx)  // dx[bt][c] (+)= sum_n dG[bt][n] W_ih[n][c]
      launch_gemm_f32((int)BT, C, G, g, G, 1, w_ih[d], C, 1, dx, C, nullptr, nullptr, d == 1, s);
    if (dw_ih && dw_ih[d])  // dW_ih[n][c] = sum_bt dG[bt][n] x[bt][c]
      launch_gemm_f32(G, C, (int)BT, g, 1, G, x, C, 1, dw_ih[d], C, nullptr, nullptr, false, s);
    if (dw_hh && dw_hh[d])  // dW_hh[n][k] = sum_bt dG[bt][n] h_prev[bt][k]
      launch_gemm_f32(G, H, (int)BT, g, 1, G, hp + (size_t)d * BT * H, H, 1, dw_hh[d], H, nullptr, nullptr, false, s);
    if (db && db[d]) launch_colsum(g, (int)BT, G, G, db[d], false, s);
  }
}

// ---- many cotangents through one saved sequence ----------------------------------------------------
namespace {
struct BpttMultiBufs {
  float* dg;  // (2, kc, T, 4H) gate gradients of one chunk
  float* wt;  // W_hh^T of both directions (2, H, 4H)
  float* dc;  // (2, kc, H) carried cell gradient
};
}  // namespace

static void bptt_multi_check(int K, int T, int C, int H) {
  M2S_CHECK(K > 0 && T > 0 && C > 0 && H > 0 && H % 16 == 0, "bilstm_train_backward_multi: shape (H % 16 == 0)");
  M2S_CHECK((long)std::min(K, kGradcamKC) * T <= 4000000L, "bilstm_train_backward_multi: sequence too long");
}

static BpttMultiBufs bptt_multi_bufs(Workspace& w, int K, int T, int H) {
  const size_t kc = (size_t)std::min(K, kGradcamKC);
  BpttMultiBufs b;
  b.dg = w.take<float>(2 * kc * T * 4 * H);
  b.wt = w.take<float>((size_t)2 * 4 * H * H);
  b.dc = w.take<float>(2 * kc * H);
  return b;
}

// one chunk: dy (kc,T,H) -> dx (kc,T,C); b.wt already holds W_hh^T
static void bptt_multi_chunk(const BpttMultiBufs& b, const float* dy, int kc, int T, int C, int H,
                             const float* const w_ih[2], const float* gates, const float* cells, float* dx,
                             hipStream_t s) {
  const int G = 4 * H;
  for (int st = 0; st < T; ++st) launch_lstm_bptt_multi_step(b.wt, dy, gates, cells, b.dc, b.dg, kc, T, H, st, s);
  for (int d = 0; d < 2; ++d)  // dx[kt][c] (+)= sum_n dG[d][kt][n] W_ih[d][n][c]
    launch_gemm_f32(kc * T, C, G, b.dg + (size_t)d * kc * T * G, G, 1, w_ih[d], C, 1, dx, C, nullptr, nullptr, d == 1, s);
}

size_t bilstm_train_backward_multi_workspace_bytes(int K, int T, int C, int H) {
  bptt_multi_check(K, T, C, H);
  return Workspace::bytes([&](Workspace& w) { bptt_multi_bufs(w, K, T, H); });
}

void bilstm_train_backward_multi(const float* dy, int K, int T, int C, int H, const float* const w_ih[2],
                                 const float* const w_hh[2], const float* gates, const float* cells, float* dx,
                                 void* ws, size_t wsb, hipStream_t s) {
  bptt_multi_check(K, T, C, H);
  Workspace w(ws, wsb);
  const BpttMultiBufs b = bptt_multi_bufs(w, K, T, H);
  for (int d = 0; d < 2; ++d) launch_transpose(w_hh[d], 1, 4 * H, H, b.wt + (size_t)d * 4 * H * H, s);
  for (int k0 = 0; k0 < K; k0 += kGradcamKC) {
    const int kc = std::min(kGradcamKC, K - k0);
    bptt_multi_chunk(b, dy + (size_t)k0 * T * H, kc, T, C, H, w_ih, gates, cells, dx + (size_t)k0 * T * C, s);
  }
}

// ---- the Grad-CAM engine ---------------------------------------------------------------------------
GradCam::GradCam(const StateDict& sd, int device) : bb_(sd, device) {
  auto hw = sd.find("head.weight");
  M2S_CHECK(hw != sd.end() && hw->second.shape.size() == 2, "missing state-dict key: head.weight (n_mels, hidden)");
  nm_ = (int)hw->second.shape[0];
  hid_ = (int)hw->second.shape[1];
  M2S_CHECK(nm_ >= 1 && hid_ >= 16 && hid_ % 16 == 0, "gradcam: head.weight shape");
  const int C = kStages[5].cout;
  for (int d = 0; d < 2; ++d) {
    const std::string sfx = d ? "_l0_reverse" : "_l0";
    w_ih_[d] = arena_.add(need(sd, "rnn.lstm.weight_ih" + sfx, {4 * hid_, C}).data, sizeof(float) * 4 * hid_ * C);
    w_hh_[d] = arena_.add(need(sd, "rnn.lstm.weight_hh" + sfx, {4 * hid_, hid_}).data, sizeof(float) * 4 * hid_ * hid_);
    b_ih_[d] = arena_.add(need(sd, "rnn.lstm.bias_ih" + sfx, {4 * hid_}).data, sizeof(float) * 4 * hid_);
    b_hh_[d] = arena_.add(need(sd, "rnn.lstm.bias_hh" + sfx, {4 * hid_}).data, sizeof(float) * 4 * hid_);
  }
  head_w_ = arena_.add(hw->second.data, sizeof(float) * nm_ * hid_);
  head_b_ = arena_.add(need(sd, "head.bias", {nm_}).data, sizeof(float) * nm_);
  arena_.upload(device);
}

namespace {
struct GradCamDims {
  int T, C, h, w, P, K, kc, nm, hid;
  size_t bb_bytes, lstm_bytes;
};
struct GradCamBufs {
  float *feats, *bn, *pooled, *y, *gates, *cells, *hid, *pred, *dpred, *dy, *dx, *mask;
  int* fidx;
  void *bbws, *lstmws;
  BpttMultiBufs bp;
};
}  // namespace

static size_t gradcam_fpad(int n_frames) { return ((size_t)std::max(n_frames, 1) + 3) & ~size_t(3); }

// the engine's scratch: the size query and the call both run this.  The optional outputs (pred_norm, dpooled,
// bn_stats) always have their stand-ins here, so the size does not depend on which of them the caller wants.  Only the frame-index table (n_frames ints)
// grows with the number of targets past kGradcamKC.
static GradCamBufs gradcam_bufs(Workspace& w, const GradCamDims& d, int n_bands, int n_frames, size_t bn_floats) {
  GradCamBufs b;
  const size_t T = (size_t)d.T, fpad = gradcam_fpad(n_frames);
  b.fidx = w.take<int>(fpad + (size_t)n_bands * d.nm);  // [frame_idx, padded | band_mask]: one staged copy
  b.mask = b.fidx ? reinterpret_cast<float*>(b.fidx + fpad) : nullptr;
  b.feats = w.take<float>(T * d.C * d.P);
  b.bn = w.take<float>(bn_floats);
  b.bbws = w.take<char>(d.bb_bytes);
  b.pooled = w.take<float>(T * d.C);
  b.y = w.take<float>(T * d.hid);
  b.gates = w.take<float>(2 * T * 4 * d.hid);
  b.cells = w.take<float>(2 * T * d.hid);
  b.hid = w.take<float>(2 * T * d.hid);
  b.lstmws = w.take<char>(d.lstm_bytes);
  b.pred = w.take<float>(T * d.nm);
  b.dpred = w.take<float>((size_t)d.kc * T * d.nm);
  b.dy = w.take<float>((size_t)d.kc * T * d.hid);
  b.dx = w.take<float>((size_t)d.kc * T * d.C);
  b.bp = bptt_multi_bufs(w, d.K, d.T, d.hid);
  return b;
}

static GradCamDims gradcam_dims(const CamBackbone& bb, int nm, int hid, int T, int H, int W, int n_bands, int n_frames) {
  M2S_CHECK(T >= 1 && H >= 32 && W >= 32, "gradcam: bad clip size");
  M2S_CHECK(n_bands >= 1 && n_bands <= 4096, "gradcam: n_bands must be at least 1");
  M2S_CHECK(n_frames >= 0, "gradcam: negative n_frames");
  const long K = (long)n_bands * (1 + (long)n_frames);
  M2S_CHECK(K <= 2147483647L / 4, "gradcam: too many targets");
  GradCamDims d;
  d.T = T;
  d.C = kStages[5].cout;
  d.h = H;
  d.w = W;
  for (int i = 0; i < 5; ++i) d.h = (d.h + 1) / 2, d.w = (d.w + 1) / 2;
  d.P = d.h * d.w;
  M2S_CHECK(cam_heatmap_shape_ok(d.C, d.h, d.w, H, W), "gradcam: frame size too large for the heat-map kernel");
  d.K = (int)K;
  d.kc = (int)std::min<long>(K, kGradcamKC);
  d.nm = nm;
  d.hid = hid;
  bptt_multi_check(d.K, T, d.C, hid);
  d.bb_bytes = bb.workspace_bytes(T, H, W);
  d.lstm_bytes = bilstm_train_workspace_bytes(1, T, d.C, hid);
  return d;
}

size_t GradCam::workspace_bytes(int T, int H, int W, int n_bands, int n_frames) const {
  const GradCamDims d = gradcam_dims(bb_, nm_, hid_, T, H, W, n_bands, n_frames);
  return Workspace::bytes([&](Workspace& w) { gradcam_bufs(w, d, n_bands, n_frames, (size_t)bb_.bn_stats_floats()); });
}

void GradCam::forward(const float* frames, int T, int H, int W, const float* mean, const float* sd,
                      const float* band_mask, int n_bands, const int* frame_idx, int n_frames, int reduction,
                      float* heat_seq, float* heat_frame, float* pred_norm, float* dpooled, float* bn_stats, void* ws,
                      size_t wsb, hipStream_t s) {
  const GradCamDims d = gradcam_dims(bb_, nm_, hid_, T, H, W, n_bands, n_frames);
  M2S_CHECK(reduction == 0 || reduction == 1, "gradcam: reduction must be 0 (mean) or 1 (sum)");
  M2S_CHECK(n_frames == 0 || (frame_idx && heat_frame), "gradcam: null frame_idx / heat_frame");
  for (int j = 0; j < n_frames; ++j)
    M2S_CHECK(frame_idx[j] >= 0 && frame_idx[j] < T, "gradcam: target frame index outside [0, T)");
  for (int b = 0; b < n_bands; ++b) {
    bool any = false;
    for (int m = 0; m < nm_; ++m) {
      const float v = band_mask[(size_t)b * nm_ + m];
      M2S_CHECK(v == 0.f || v == 1.f, "gradcam: band_mask entries must be 0 or 1");
      any = any || v != 0.f;
    }
    M2S_CHECK(any, "gradcam: a band selects no mel bin");
  }
  Workspace w(ws, wsb);
  const GradCamBufs b = gradcam_bufs(w, d, n_bands, n_frames, (size_t)bb_.bn_stats_floats());
  const int F = n_frames, C = d.C, Hd = hid_;
  {
    const size_t fpad = gradcam_fpad(F);
    std::vector<int> tab(fpad + (size_t)n_bands * nm_, 0);
    for (int j = 0; j < F; ++j) tab[j] = frame_idx[j];
    std::memcpy(tab.data() + fpad, band_mask, sizeof(float) * (size_t)n_bands * nm_);
    tab_.upload_ints(tab.data(), tab.size(), b.fidx, s);  // M2S_E_STATE on a capturing stream
  }
  auto A = [&](size_t off) { return static_cast<const float*>(arena_.ptr(off)); };
  const float* wih[2] = {A(w_ih_[0]), A(w_ih_[1])};
  const float* whh[2] = {A(w_hh_[0]), A(w_hh_[1])};
  const float* bih[2] = {A(b_ih_[0]), A(b_ih_[1])};
  const float* bhh[2] = {A(b_hh_[0]), A(b_hh_[1])};
  float* pred = pred_norm ? pred_norm : b.pred;
  {
    StageTag tag("gradcam_fwd");
    float* taps[5] = {nullptr, nullptr, nullptr, nullptr, b.feats};
    bb_.forward(frames, T, H, W, taps, bn_stats ? bn_stats : b.bn, b.bbws, d.bb_bytes, s);
    launch_gap_nchw(b.feats, (long)T * C, d.P, b.pooled, s);
    bilstm_train_forward(b.pooled, 1, T, C, Hd, wih, whh, bih, bhh, b.y, b.gates, b.cells, b.hid, b.lstmws,
                         d.lstm_bytes, s);
    linear_forward(b.y, T, Hd, nm_, A(head_w_), A(head_b_), pred, s);
  }
  StageTag tag("gradcam_bwd");
  for (int dd = 0; dd < 2; ++dd) launch_transpose(whh[dd], 1, 4 * Hd, Hd, b.bp.wt + (size_t)dd * 4 * Hd * Hd, s);
  const float inv_p = 1.f / (float)d.P;
  const size_t map = (size_t)H * W;
  for (int k0 = 0; k0 < d.K; k0 += kGradcamKC) {
    const int kc = std::min(kGradcamKC, d.K - k0);
    launch_gradcam_cotangents(pred, mean, sd, b.mask, b.fidx, F, T, nm_, k0, kc, reduction == 1, b.dpred, s);
    // the head's backward: dy (kc T, hidden) = dpred (kc T, n_mels) W_head
    launch_gemm_f32(kc * T, Hd, nm_, b.dpred, nm_, 1, A(head_w_), Hd, 1, b.dy, Hd, nullptr, nullptr, false, s);
    float* dx = dpooled ? dpooled + (size_t)k0 * T * C : b.dx;
    bptt_multi_chunk(b.bp, b.dy, kc, T, C, Hd, wih, b.gates, b.cells, dx, s);
    // the map of target k at its own frame(s), under its own cotangent; grads.mean((2,3)) = dpooled / P
    bool frame_targets = false;
    for (int kl = 0; kl < kc; ++kl) {
      const int k = k0 + kl, band = k / (1 + F), j = k % (1 + F);
      if (j != 0) {
        frame_targets = true;
        continue;
      }
      launch_cam_heatmap(b.feats, T, C, d.h, d.w, dx + (size_t)kl * T * C, inv_p, nullptr, 0, 0, 0, T, T, H, W,
                         heat_seq + (size_t)band * T * map, s);
    }
    if (frame_targets)
      launch_cam_heatmap(b.feats, T, C, d.h, d.w, dx, inv_p, b.fidx, 1, k0, F, T, kc, H, W, heat_frame, s);
  }
}

void linear_forward(const float* x, int rows, int in, int out, const float* w, const float* b, float* y, hipStream_t s) {
  launch_gemm_f32(rows, out, in, x, in, 1, w, 1, in, y, out, b, nullptr, false, s);
}

void linear_backward(const float* dy, const float* x, int rows, int in, int out, const float* w, float* dx, float* dw,
                     float* db, hipStream_t s) {
  if (dx) launch_gemm_f32(rows, in, out, dy, out, 1, w, in, 1, dx, in, nullptr, nullptr, false, s);
  if (dw) launch_gemm_f32(out, in, rows, dy, 1, out, x, in, 1, dw, in, nullptr, nullptr, false, s);
  if (db) launch_colsum(dy, rows, out, out, db, false, s);
}

}  // namespace m2s
