// Grad-CAM path of the acoustic model (the reference's scripts/mri_gradcam_formant.py:128-279):
// a train-mode backbone forward (BatchNorm on batch statistics, timm / torch semantics) and the
// autograd kernels behind the feature-map gradient: BiLSTM forward with saved activations and its
// backward through time, the head Linear, GAP.  Exact fp32 throughout (the reference runs fp32).
#pragma once

#include <vector>

#include "conv_igemm.hpp"
#include "model.hpp"

namespace m2s {

// ---- kernels (cam.hip) ------------------------------------------------------------------------
// C[m][n] (accumulate ? += : =) sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn] (+ bias1[n] + bias2[n]);
// C row-major with leading dimension ldc.  fp32 FMA, k ascending per output.
void launch_gemm_f32(int M, int N, int K, const float* A, long sam, long sak, const float* B, long sbk, long sbn,
                     float* C, long ldc, const float* bias1, const float* bias2, bool accumulate, hipStream_t s);
// out[c] (+)= sum over rows of x[r*ld + c], c < cols (rows ascending)
void launch_colsum(const float* x, int rows, int cols, long ld, float* out, bool accumulate, hipStream_t s);
// conv_stem without bias / activation: frames (N,H,W) -> z (N,OH,OW,32) with w9 [32][9] (RGB repeat folded)
void launch_stem_raw(const float* frames, int N, int H, int W, int OH, int OW, int pad_t, int pad_l, const float* w9,
                     float* z, hipStream_t s);
// depthwise 3x3 without bias / activation: x (N,IH,IW,cs) -> z (N,OH,OW,cs), w tap-major [9][cs]
void launch_dw_raw(const float* x, int N, int IH, int IW, int OH, int OW, int stride, int pad_t, int pad_l, int cs,
                   const float* w, float* z, hipStream_t s);
// BatchNorm with batch statistics over rows x (M, cs), C real channels:
//   stats[0:C] = mean, stats[C:2C] = biased variance (two passes, partial sums reduced in double);
//   x <- act((x - mean) * gamma / sqrt(var + eps) + beta) (+ res), pad channels zero.
size_t bn_train_scratch_floats(long M, int cs);
void launch_bn_train(float* x, long M, int C, int cs, const float* gamma, const float* beta, float eps, int act,
                     const float* res, float* stats, float* scratch, hipStream_t s);
// (N,P,cs) channel-last -> (N,C,P) dense
void launch_to_nchw(const float* x, int N, int P, int C, int cs, float* y, hipStream_t s);
// GAP of NCHW maps and its backward: y (N*C) = mean over P; dx (N*C*P) = dy / P
void launch_gap_nchw(const float* x, long NC, int P, float* y, hipStream_t s);
void launch_gap_nchw_bwd(const float* dy, long NC, int P, float* dx, hipStream_t s);
// BiLSTM with saved activations, both directions, one launch per time step (grid: H/8 unit groups x 2).
//   pre (B,T,8H) = x W_ih^T + b_ih + b_hh for [fwd 4H | bwd 4H]; whh (2,4H,H);
//   gates (2,B,T,4H) post-activation i,f,g,o; cells, hid (2,B,T,H)
void launch_lstm_train_step(const float* pre, const float* whh, float* gates, float* cells, float* hid, int B, int T,
                            int H, int step, hipStream_t s);
// backward step (reverse of the forward order per direction): whh_t (2,H,4H) = W_hh^T, dy (B,T,H) (the
// sum merge sends the same dy to both directions), dc (2,B,H) carried cell gradient, dg (2,B,T,4H) out
void launch_lstm_bptt_step(const float* whh_t, const float* dy, const float* gates, const float* cells, float* dc,
                           float* dg, int B, int T, int H, int step, hipStream_t s);
// hp (2,B,T,H): the hidden state each step consumed (fwd: h[t-1], bwd: h[t+1], zero at the ends)
void launch_lstm_hprev(const float* hid, float* hp, int B, int T, int H, hipStream_t s);
// (rows, cols) -> (cols, rows), for `planes` consecutive matrices
void launch_transpose(const float* x, int planes, int rows, int cols, float* y, hipStream_t s);

// ---- kernels of the Grad-CAM engine (gradcam.hip) ----------------------------------------------------
// cotangents per backward-through-time pass: the N tile of v_mfma_f32_16x16x4_f32
constexpr int kGradcamKC = 16;
// dpred (kc,T,nm) = d target_k / d pred_norm for cotangents k0 .. k0 + kc - 1, k = band * (1 + F) + j: j = 0 the
// whole-clip target (mean: 1/T per frame, sum: 1), j >= 1 the band power of frame fidx[j-1].
// dpred[k,t,m] = s_k(t) * ln10/10 * std[m] * 10^((pred std + mean)[t,m] / 10) * mask[band,m]
void launch_gradcam_cotangents(const float* pred, const float* mean, const float* sd, const float* mask,
                               const int* fidx, int F, int T, int nm, int k0, int kc, bool sum, float* dpred,
                               hipStream_t s);
// one step of the backward through time for kc <= kGradcamKC cotangents over one saved sequence, both
// directions (grid: H/16 unit groups x 2): whh_t (2,H,4H), dy (kc,T,H), gates (2,1,T,4H), cells (2,1,T,H),
// dc (2,kc,H) carried cell gradient, dg (2,kc,T,4H) out.  H % 16 == 0.
void launch_lstm_bptt_multi_step(const float* whh_t, const float* dy, const float* gates, const float* cells, float* dc,
                                 float* dg, int kc, int T, int H, int step, hipStream_t s);
// heat maps out (.,H,W) from feats (N,C,h,w) NCHW and channel weights (scaled by wscale); see gradcam.hip for
// the two addressing modes (0: M plain maps with frame table `tab` or frame = map index; 1: the frame
// cotangents of a (kc,T,C) chunk starting at cotangent k0, M = kc)
bool cam_heatmap_shape_ok(int C, int h, int w, int H, int W);
void launch_cam_heatmap(const float* feats, int N, int C, int h, int w, const float* weights, float wscale,
                        const int* tab, int mode, int k0, int F, int T, int M, int H, int W, float* out,
                        hipStream_t s);

// ---- BiLSTM (nn.LSTM 1 layer, bidirectional, batch_first, sum merge) and Linear with autograd ------
// x (B,T,C); weights in nn.LSTM layout per direction d (0 fwd, 1 reverse): w_ih (4H,C), w_hh (4H,H),
// b_ih / b_hh (4H).  forward: y (B,T,H) = h_fwd + h_bwd, saved gates (2,B,T,4H), cells / hid (2,B,T,H).
// backward: dy (B,T,H) -> dx (B,T,C), dw_ih / dw_hh / db (= d b_ih = d b_hh) per direction; any output
// pointer may be null.
size_t bilstm_train_workspace_bytes(int B, int T, int C, int H);
void bilstm_train_forward(const float* x, int B, int T, int C, int H, const float* const w_ih[2],
                          const float* const w_hh[2], const float* const b_ih[2], const float* const b_hh[2], float* y,
                          float* gates, float* cells, float* hid, void* ws, size_t wsb, hipStream_t s);
void bilstm_train_backward(const float* x, const float* dy, int B, int T, int C, int H, const float* const w_ih[2],
                           const float* const w_hh[2], const float* gates, const float* cells, const float* hid,
                           float* dx, float* const dw_ih[2], float* const dw_hh[2], float* const db[2], void* ws,
                           size_t wsb, hipStream_t s);
// K cotangents dy (K,T,H) through the backward of ONE saved sequence (gates (2,1,T,4H), cells (2,1,T,H) of
// bilstm_train_forward with B = 1) -> dx (K,T,C); no weight gradient.  Chunks of kGradcamKC cotangents, T launches
// per chunk; the workspace holds one chunk, so it stops growing at K = kGradcamKC.  A cotangent's dx is
// bit-identical whatever K and its position.
size_t bilstm_train_backward_multi_workspace_bytes(int K, int T, int C, int H);
void bilstm_train_backward_multi(const float* dy, int K, int T, int C, int H, const float* const w_ih[2],
                                 const float* const w_hh[2], const float* gates, const float* cells, float* dx,
                                 void* ws, size_t wsb, hipStream_t s);
// y (rows,out) = x (rows,in) W^T + b ; backward dx = dy W, dw = dy^T x, db = column sums of dy
void linear_forward(const float* x, int rows, int in, int out, const float* w, const float* b, float* y, hipStream_t s);
void linear_backward(const float* dy, const float* x, int rows, int in, int out, const float* w, float* dx, float* dw,
                     float* db, hipStream_t s);

// ---- the train-mode backbone ---------------------------------------------------------------------
class CamBackbone {
 public:
  CamBackbone(const StateDict& sd, int device);
  int device() const { return device_; }
  // BatchNorm layers in state-dict order (conv_stem's bn1, then per block bn1 / bn2 / bn3); stats layout
  // per layer [mean C | var C]
  int bn_layers() const { return (int)bn_.size(); }
  int bn_channels(int i) const { return bn_[i].C; }
  int bn_stats_floats() const;
  size_t workspace_bytes(int N, int H, int W) const;
  // frames (N,H,W) -> the five timm feature maps (taps[i]: (N,C,OH,OW) fp32 dense, shapes as
  // effnet_features), bn_stats: batch mean / biased var of every BN layer
  void forward(const float* frames, int N, int H, int W, float* const taps[5], float* bn_stats, void* ws, size_t wsb,
               hipStream_t s);

 private:
  struct BNp {
    int C = 0;
    size_t g = 0, b = 0;  // gamma, beta (arena offsets)
  };
  struct Blk : BlockDef {
    PConv c1, c2, se1, se2;
    size_t dw = 0;
    int bn[3] = {-1, -1, -1};
  };
  int device_;
  Arena arena_;
  size_t stem_w_ = 0;
  int stem_bn_ = 0;
  std::vector<BNp> bn_;
  std::vector<Blk> blocks_;
};

// ---- the Grad-CAM engine ------------------------------------------------------------
// compute_gradcam for every band and target frame of one clip in one pass: one train-mode backbone forward,
// GAP, BiLSTM with saved activations, head, then all K = n_bands * (1 + n_frames) cotangents through the
// backward together and the heat maps on the device.
class GradCam {
 public:
  GradCam(const StateDict& sd, int device);
  int device() const { return bb_.device(); }
  int n_mels() const { return nm_; }
  int hidden() const { return hid_; }
  int bn_stats_floats() const { return bb_.bn_stats_floats(); }
  // throws M2S_E_ARG for a shape forward would refuse
  size_t workspace_bytes(int T, int H, int W, int n_bands, int n_frames) const;
  // frames (T,H,W), mean / std (n_mels) device; band_mask (n_bands,n_mels) 0/1 and frame_idx (n_frames) HOST.
  // heat_seq (n_bands,T,H,W), heat_frame (n_bands,n_frames,H,W); optional pred_norm (T,n_mels), dpooled (K,T,C),
  // bn_stats.  Arguments are checked before any launch.
  void forward(const float* frames, int T, int H, int W, const float* mean, const float* sd, const float* band_mask,
               int n_bands, const int* frame_idx, int n_frames, int reduction, float* heat_seq, float* heat_frame,
               float* pred_norm, float* dpooled, float* bn_stats, void* ws, size_t wsb, hipStream_t s);

 private:
  CamBackbone bb_;
  Arena arena_;
  int nm_ = 0, hid_ = 0;
  size_t w_ih_[2] = {0, 0}, w_hh_[2] = {0, 0}, b_ih_[2] = {0, 0}, b_hh_[2] = {0, 0}, head_w_ = 0, head_b_ = 0;
  RaggedTable tab_;  // frame_idx and band_mask on their way to the device
};

}  // namespace m2s
