// Launchers for the non-GEMM kernels of the hot path.
#pragma once

#include "lstm_route.hpp"
#include "m2s_common.hpp"

namespace m2s {

// Asynchronous failure report of the persistent kernels' bounded waits (LDS flag rings, grid hand-offs): the
// engine's host-mapped error word takes one of these codes; m2s_acoustic_status turns it into an error.
enum AsyncCode : unsigned { M2S_ASYNC_LSTM = 1u, M2S_ASYNC_WS = 2u };
struct AsyncReport {
  unsigned spin_max = 1u << 20;  // polls per LDS flag wait (each ~1 s_sleep) before it counts as timed out
  unsigned* err = nullptr;       // host-mapped error word, or null (no report)
};
// one lane of the wave stores `code` to the host-mapped word (system scope: the host reads it after a sync)
__device__ __forceinline__ void report_async(unsigned* err, unsigned code, int lane) {
  if (err && lane == 0) __hip_atomic_store(err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// conv_stem (3x3 s2 TF-SAME, grey repeat folded: w[o][9]) + bn1 + SiLU.  frames fp32 (N,H,W)
// -> y (N,OH,OW,cs_out) T.  timm conv_stem/bn1, mri_acoustic_model.py:41-46.
template <typename T>
void launch_stem(const float* frames, int N, int H, int W, int OH, int OW, int pad_t, int pad_l,
                 const float* w9, const float* bias, int cout, int cs_out, T* y, hipStream_t s);

// conv_dw (3x3 depthwise, stride 1/2, TF-SAME) + bn2 + SiLU, plus per-(image, pixel block, channel)
// partial sums of the output (SE squeeze).  x (N,IH,IW,cs) -> y (N,OH,OW,cs),
// sums (N, dw_pixel_blocks(OH, OW), cs) fp32.  (dwse.hip)
int dw_pixel_blocks(int OH, int OW);
template <typename T>
void launch_dwconv(const T* x, int N, int IH, int IW, int OH, int OW, int stride, int pad_t, int pad_l,
                   int C, int cs, const float* w9, const float* bias, T* y, float* sums, hipStream_t s);

// SE squeeze: mean (N, cs) in the compute dtype from the depthwise partial sums (N, npb, cs).
// (The excitation conv_reduce -> SiLU -> conv_expand -> sigmoid then runs as two MFMA GEMMs.)
template <typename T>
void launch_se_mean(const float* psum, int N, int npb, int cs, float inv_count, T* mean, hipStream_t s);

// Fused conv_pw + bn1 + SiLU + conv_dw (stride 1) + bn2 + SiLU + SE squeeze for maps whose
// haloed tile fits a workgroup ((OH+2)(OW+2) <= 400 bf16 / 324 split, OH*OW <= 256): x (N,P,cs_in) ->
// y (N,P,cs_mid), se_mean (N,cs_mid).  wpw packed [>=ceil64(cs_mid)][kp], bpw likewise padded.
// bf16: x/y/se_mean bf16, wdw = tap-major [9][cs_mid] bf16 weights in the dword half of their channel
// (uint32).  split (bf16x3): x/y/se_mean sp_t, wpw rows [hi kp | lo kp], wdw = fp32 [9][cs_mid].
// (ir_fused.hip)
bool ir_fused_supported(int OH, int OW, int cs_in, int cs_mid, bool split);
void launch_ir_pwdw(const void* x, int N, int cs_in, int kp, const void* wpw, const float* bpw, const void* wdw,
                    const float* bdw, int OH, int OW, int cs_mid, void* y, void* se_mean, bool split, double flops,
                    double bytes, hipStream_t s, bool f8_out = false, const void* x8 = nullptr,
                    const void* w8 = nullptr, const float* wsc = nullptr, int kp8 = 0);
// f8_out (bf16 inputs and weights): the depthwise output y is stored as OCP e4m3 bytes [N][P][cs_mid]
// (saturated to +-448), the operand of launch_se_gemm_f8; the SE means stay bf16 (exact sums).
// x8 (with f8_out): the expand runs on e4m3 too: x8 = the block input as e4m3 rows of kp8 bytes (kp8 = cs_in
// rounded up to 128, zero past cs_in; launch_se_*_f8 y8 / launch_rows_e4m3), w8 = e4m3 [rows][kp8] with
// per-channel scales wsc (pack_gemm_f8), one block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 per 128 k.
// bf16 (N*P, cs) rows -> e4m3 rows of ld8 bytes (zeros past cs): an e4m3 expand operand for a block input
// no e4m3 producer wrote.
void launch_rows_e4m3(const void* x, long rows, int cs, void* y8, int ld8, hipStream_t s);

// fp8 engines: the SE-gated conv_pwl (+ bn3 + skip) of a stride-1 IR block on v_mfma_scale_f32_16x16x128_f8f6f4:
// y (M, cs_out) bf16 = wscale[n] * sum_k w8[n][k] e4m3(gate[m / P][k] x8[m][k]) + bias[n] (+ res (M, cs_out) bf16).
// x8: e4m3 (M, cs_in) (launch_ir_pwdw f8_out); w8: e4m3 [n_pad][kp], kp = cs_in rounded up to 128, zero
// padded (pack_gemm_f8); gate: bf16 (M / P, cs_in).  P % 64 == 0, cs_out <= 224.  (gemm128.hip)
// y8 (optional): an e4m3 copy of y, rows of ld8 bytes (the next IR block's expand operand).
bool se_gemm_f8_supported(int P, int cs_in, int cs_out);
void launch_se_gemm_f8(const void* x8, int M, int P, int cs_in, const void* w8, int kp, int n_pad, const float* wscale,
                       const float* bias, const void* gate, const void* res, void* y, int cs_out, hipStream_t s,
                       double flops, double bytes, void* y8 = nullptr, int ld8 = 0);

// bf16x3 engines: the same SE-gated conv_pwl (+ bn3 + skip) in split fp32 on gemm128.hip: x interleaved split
// (M, cs_in / 32, [hi 32 | lo 32]) (il_st8), w split rows [hi cs_in | lo cs_in] (conv_gemm packing, n_pad rows),
// gate split (M / P, [hi cs_in | lo cs_in]), res / y split (M, [hi cs_out | lo cs_out]).  P % 64 == 0.
bool se_gemm_sp_supported(int P, int cs_in, int cs_out);
void launch_se_gemm_sp(const void* x, int M, int P, int cs_in, const void* w, int n_pad, const float* bias,
                       const void* gate, const void* res, void* y, int cs_out, hipStream_t s, double flops, double bytes,
                       int waves);  // waves: 8 (two a SIMD) or 4 a workgroup (Switches::se_sp_waves)

// The same split SE-gated conv_pwl as a persistent warp-specialised GEMM: loader waves fill a 3-slot LDS
// ring by LDS-DMA and consumer waves compute, synchronised by per-slot FULL / FREE counters in LDS (no
// per-K-step barrier; the ring runs across tiles).  Same operands as launch_se_gemm_sp; P % 256 == 0 with
// cs_out <= 128 (16x16 maps) or P == 64 with 128 < cs_out <= 224 (8x8 maps).  (se_ws.hip)
bool se_ws_supported(int P, int cs_in, int cs_out);
// Every FULL / FREE wait is bounded by rep.spin_max polls; a timeout is reported through rep.err and the
// consumer's tiles from then on are stored as NaN.
// x_f32: x holds plain fp32 rows [M][cs_in] (ir_ws's fm32 output) instead of the interleaved split layout.
// rev: the workgroups walk their tiles from the last row tile down (the rows a forward-walking producer wrote last
// are read first); every tile's result is independent of the order.
// half: a short last round runs as half tiles (Switches::sews_half); cfg: tile / ring variant, 0 = the default
// (Switches::se_ws_cfg; A/B only).
void launch_se_ws(const void* x, int M, int P, int cs_in, const void* w, int n_pad, const float* bias, const void* gate,
                  const void* res, void* y, int cs_out, hipStream_t s, double flops, double bytes, AsyncReport rep,
                  bool x_f32, bool rev, bool half, int cfg);

// fp8 engines: launch_se_gemm_f8's operation (e4m3 x8 / w8, bf16 gate / res / y) on the same warp-specialised
// flag ring.  (se_ws.hip)
bool se_ws_f8_supported(int P, int cs_in, int cs_out);
// y8 (optional): an e4m3 copy of y, rows of ld8 bytes (the next IR block's e4m3 expand operand, launch_ir_pwdw x8)
void launch_se_ws_f8(const void* x8, int M, int P, int cs_in, const void* w8, int kp, int n_pad, const float* wscale,
                     const float* bias, const void* gate, const void* res, void* y, int cs_out, hipStream_t s, double flops,
                     double bytes, void* y8 = nullptr, int ld8 = 0, AsyncReport rep = {}, bool half = false);

// The same for a stride-2 depthwise (TF-SAME, top / left pads pad_t / pad_l) on an IH x IW <= 256-pixel
// conv_pw map: y (N, OH*OW, cs_mid), se_mean over the OH x OW output.  (ir_fused.hip)
// Split-fp32 IR front half (conv_pw + bn1 + SiLU + conv_dw + bn2 + SiLU + SE squeeze) on W = 8 / 16 maps as
// one persistent warp-specialised workgroup per CU; same outputs as launch_ir_pwdw(split = true) (stride 1) and
// launch_ir_pwdw_s2(split = true) (stride 2: 16x16 -> 8x8, TF-SAME pads pad_t / pad_l; y is the OH x OW map).
// wdw: fp32 tap-major [9][cs_mid].  (ir_ws.hip)
bool ir_ws_supported(int H, int W, int cs_in, int kp, int cs_mid);
bool ir_ws_s2_supported(int H, int W, int cs_in, int kp, int cs_mid, int OH, int OW, int pad_t, int pad_l);
// The hand-off waits are bounded by rep.spin_max polls; a timeout is reported through rep.err and the images of
// that workgroup get NaN SE means (their block output is NaN).
void launch_ir_ws(const void* x, int N, int H, int W, int cs_in, int kp, int cs_mid, const void* wpw, const float* bpw,
                  const float* wdw, const float* bdw, void* y, void* se_mean, double flops, double bytes,
                  hipStream_t s, AsyncReport rep = {}, int stride = 1, int OH = 0, int OW = 0, int pad_t = 0,
                  int pad_l = 0, double spill = 0.0, bool fm32 = false, int parts = 0, bool handoff = false);
// fm32: y is stored as plain fp32 rows [N * OH * OW][cs_mid] (for launch_se_ws(x_f32 = true)) instead of the
// interleaved split layout: one 16-byte store per 4 channels, no split in the consumers.
// parts > 0: that many slice ranges for the tail images instead of the launcher's rule (Switches::irws_parts).
// 16-wide stride-1 maps of at most 16 rows and 8 x 8 stride-1 maps run the per-wave form (ir_ws_wave.hpp: the
// depthwise on the expand's MFMA accumulators, no hand-offs, so no waits and nothing to report through rep); handoff
// (Switches::irws_handoff): the handed-off form there too, recorded as ir_ws_kernel<16, 4, 1, 1> / <8, 4, 1, 1> /
// <8, 7, 1, 1>.  8-wide maps of any other height run the handed-off form under the plain name in both settings.
// Stride-2 IR front half on bands of 4 output rows (blocks.3.0: 32x32 -> 16x16), split fp32 or bf16: y =
// the SE GEMM's operand (N, OH*OW, cs_mid; split: interleaved hi/lo), psum = squeeze partial sums
// (N, OH / 4, cs_mid) for launch_se_mean.  wdw: fp32 tap-major [9][cs_mid].  (ir_s2band.hip)
int ir_s2band_bands(int OH);
bool ir_s2band_supported(int IH, int IW, int OH, int OW, int cs_in, int kp, int cs_mid);
void launch_ir_s2band(const void* x, int N, int IH, int IW, int cs_in, int kp, const void* wpw, const float* bpw,
                      const float* wdw, const float* bdw, int OH, int OW, int pad_t, int pad_l, int cs_mid, void* y,
                      float* psum, bool split, double flops, double bytes, hipStream_t s, bool f8_out = false);
bool ir_fused_s2_supported(int IH, int IW, int cs_in, int cs_mid, bool split);
void launch_ir_pwdw_s2(const void* x, int N, int cs_in, int kp, const void* wpw, const float* bpw, const void* wdw,
                       const float* bdw, int IH, int IW, int OH, int OW, int pad_t, int pad_l, int cs_mid, void* y,
                       void* se_mean, bool split, double flops, double bytes, hipStream_t s, bool f8_out = false,
                       const void* x8 = nullptr, const void* w8 = nullptr, const float* wsc = nullptr, int kp8 = 0);

// Fused HiFi-GAN ResBlock1 (all (c1, c2) pairs of one resblock + the MRF running sum), bf16 for C in
// {32, 64} or split fp32 (split: x, S as [hi C | lo C] per position) for C = 32:
// x (B, L, C) -> S (B, L, C) with S = x' (accum 0), S += x' (1), S = (S + x') / div (2).  (mrf_fused.hip)
// Split-fp32 causal dilated Conv1d with the tile's input rows staged once in LDS (conv1d_halo.hip), for the
// C = 64 MRF convs; a[i].w in fragment order [tap][C/32][hi/lo][C/16][64 lanes][8] bf16
// (conv1d_halo_frag_elems), n batched convs of one shape (grid.z).
bool conv1d_halo_sp_supported(int C, int cs, int k, int dil);
size_t conv1d_halo_frag_elems(int C, int k);
void launch_conv1d_halo_sp(const struct ConvArgs* a, int n, hipStream_t s, double flops, double bytes);
// One ResBlock1 pair x' = x + c2(lrelu(c1(lrelu(x)))) per launch with the tensor between the two convs kept in
// LDS (conv1d_halo_pair_kernel): x holds lrelu(x), the residual is recovered from it as the c2 launches do.
// chain = false: n independent pairs (grid.z), y = the pair's output (act: stored as lrelu(x'), the next pair's
// operand; accum as ConvArgs::accum, the MRF sum read from and written to y).  chain = true: the n pairs of one
// tile run in order in one workgroup, pair j accumulating as its accum says into a running sum in registers
// (rounded to hi + lo between pairs as the stored sum is), and only the last pair's y is written.
struct HaloPair {
  const void* x;
  const void* w1;  // c1 (k taps, dilation dil) and c2 (k taps, dilation 1) in conv1d_halo fragment order
  const void* w2;
  const float* b1;
  const float* b2;
  void* y;
  int k, dil;
  int accum;
  int act;  // LeakyReLU 0.1 on the value stored
};
bool conv1d_halo_pair_supported(int C, int cs, int k, int dil);
bool conv1d_halo_pair_fills(int C, int B, int L);  // clips x tiles fill the device's resident workgroup slots
void launch_conv1d_halo_pair(const HaloPair* p, int n, int C, int B, int L, bool chain, float div, hipStream_t s,
                             double flops, double bytes);
// w1/w2 are in fragment order: [rb1_frag_taps(C, k, split)][hi/lo if split][C/16][C/32][64 lanes][8] bf16,
// element (tap t, n16, k32, lane, e) = W[n16*16 + lane%16][k32*32 + 8*(lane/16) + e][t] (zero taps past k).
bool rb1_fused_supported(int C, int cs, int k, const int* dil, int np, int kp, bool split);
int rb1_frag_taps(int C, int k, bool split);
void launch_rb1_fused(const bf16_t* x, bf16_t* s, int B, int L, int C, int k, int np, const int* dil,
                      const bf16_t* const* w1, const float* const* b1, const bf16_t* const* w2,
                      const float* const* b2, int kp, int accum, float div, bool split, double flops, double bytes,
                      hipStream_t st);

// conv_stem + bn1 + SiLU + blocks.0.0 (3x3 32->16 + SiLU) + blocks.0.1 (3x3 16->16 + SiLU + skip) in
// one kernel: frames (N,H,W) fp32 -> y (N,OH,OW,16).  w0/w1: packed conv rows (kp 288 / 160); bf16, or
// split fp32 (`split`: [hi | lo] weight rows, y in sp_t layout).  (stem_b0.hip)
void launch_stem_b0(const float* frames, int N, int H, int W, int OH, int OW, int pad_t, int pad_l, const float* w9,
                    const float* b9, const void* w0, const float* b0, int kp0, const void* w1, const float* b1,
                    int kp1, void* y, bool split, double flops, double bytes, hipStream_t s, int parts);
// parts > 0: that many tile-row ranges a strip (clamped to the tile rows) instead of the launcher's fill rule
// (Switches::stem_parts)

// SqueezeExcite excitation (bf16, or split fp32 with split = true): gate (N, cs_mid) =
// sigmoid(W2 · SiLU(W1 · mean + b1) + b2), mean (N, cs_mid) from the squeeze; w1 packed [>= rd][kp1],
// w2 packed [>= mid][kp2] (split: rows [hi kp | lo kp]).  (se_excite.hip)
bool se_excite_supported(int rd, int kp2, int cs_mid);
void launch_se_excite(const void* mean, int N, int mid, int cs_mid, const void* w1, int kp1, const float* b1,
                      int rd, const void* w2, int kp2, const float* b2, void* gate, bool split, hipStream_t s);

// bf16 EdgeResidual (stride 1, skip) 32 -> 128 -> 32: conv_exp 3x3 + SiLU, conv_pwl 1x1, + x in one
// persistent kernel; x, y (N,H,W,32); wexp / wpwl in the kernel's fragment orders.  (er_fused.hip)
bool er_fused_supported(int H, int W, int cin, int mid, int cout, int kp_exp, int kp_pwl);
void launch_er_fused(const bf16_t* x, int N, int H, int W, const bf16_t* wexp, const float* bexp, const bf16_t* wpwl,
                     const float* bpwl, bf16_t* y, double flops, double bytes, hipStream_t s);

// fp8 engines: er_fused's block on e4m3 operands (v_mfma_scale_f32_16x16x128_f8f6f4): wexp e4m3 [3][8][2][64][16]
// (tap groups of four, per-channel scales sexp), wpwl e4m3 [2][2][64][16] (permuted K, scales spwl); x, y bf16
// (N,H,W,32); x8 (optional): the input as e4m3 bytes (N,H,W,32) from the producer (ers2_fused / er8_fused y8),
// y8 (optional, needs x8): e4m3 bytes of y for the next er8 block.  (er8_fused.hip)
bool er8_fused_supported(int H, int W, int cin, int mid, int cout);
void launch_er8_fused(const bf16_t* x, int N, int H, int W, const uint8_t* wexp, const float* sexp, const float* bexp,
                      const uint8_t* wpwl, const float* spwl, const float* bpwl, bf16_t* y, double flops, double bytes,
                      hipStream_t s, const uint8_t* x8 = nullptr, uint8_t* y8 = nullptr);

// bf16 EdgeResidual (stride 1, skip) 56 -> 224 -> 56 (channel strides 64 / 224 / 64): same fusion with the
// weights streamed through an LDS ring; wst = er2_stage_elems() bf16 in the kernel's stage order.
// (er2_fused.hip)
bool er2_fused_supported(int H, int W, int cs_in, int mid, int cout, int kp_exp, int kp_pwl);
int er2_stage_elems();
// fp8 engines: the same block (56 -> 224 -> 56, 32x32, skip) on e4m3 operands (er8w_fused.hip): x8 = the input as
// e4m3 bytes (N, H, W, 64) written by the producer block, wst = the e4m3 stage stream (er8w_stream_bytes(); conv_exp
// 5 K steps of [16 n16][2][64][16 B], then conv_pwl [4][2][2][64][16 B] with the permuted K), per-channel scales
// sexp [224] / spwl [64]; y8 (optional) = e4m3 of y for the next such block.
bool er8w_fused_supported(int H, int W, int cs_in, int mid, int cout);
size_t er8w_stream_bytes();
void launch_er8w_fused(const bf16_t* x, const uint8_t* x8, int N, int H, int W, const uint8_t* wst, const float* sexp,
                       const float* bexp, const float* spwl, const float* bpwl, bf16_t* y, uint8_t* y8, double flops,
                       double bytes, hipStream_t s);
void launch_er2_fused(const bf16_t* x, int N, int H, int W, const bf16_t* wst, const float* bexp, const float* bpwl,
                      bf16_t* y, double flops, double bytes, hipStream_t s);

// Split-fp32 EdgeResidual (stride 1, skip), (cs_in, mid, cs_out) in {(32, 128, 32), (64, 224, 64)}: conv_exp
// 3x3 + SiLU -> conv_pwl + x with the three-term products, weights streamed in W_hi / W_lo stages of
// `nt` = mid / 16 fragments; x, y in sp_t layout; wst = er_sp_nt_stages() stages of nt x [64][8] bf16.
// (er_sp_fused.hip)
bool er_sp_supported(int H, int W, int cs_in, int mid, int cs_out);
int er_sp_nt_stages(int cs_in, int mid, int cs_out, int* nt);
// merged: blocks.1's W_hi and W_lo stages share one ring slot (half the barriers, same MFMA order).
void launch_er_sp(const void* x, int N, int H, int W, int cs_in, int mid, int cs_out, const void* wst, const float* bexp,
                  const float* bpwl, void* y, double flops, double bytes, hipStream_t s, bool merged = true);

// bf16 stride-2 EdgeResidual (no skip), (cs_in, mid, cs_out) in {(16, 64, 32), (32, 128, 64)}: conv_exp
// 3x3/s2 TF-SAME + SiLU -> conv_pwl; x (N,H,W,cs_in) -> y (N,OH,OW,cs_out); wexp ers2_exp_elems() bf16 in
// the kernel's fragment order, wpwl [cs_out/16][mid/32][64][8] with er_fused.hip's K permutation.
// (ers2_fused.hip)
bool ers2_fused_supported(int OH, int OW, int cs_in, int mid, int cs_out, int kp_exp, int kp_pwl);
int ers2_exp_elems(int cs_in, int mid);
// split fp32 blocks.1.0 (16 -> 64 -> 32): wexp [hi/lo][k-step][n16][lane][8], wpwl [hi/lo][n16][k-step][lane][8]
bool ers2_sp_supported(int OH, int OW, int cs_in, int mid, int cs_out);
void launch_ers2_sp(const void* x, int N, int H, int W, int OH, int OW, int pad_t, int pad_l, int cs_in, int mid,
                    int cs_out, const void* wexp, const float* bexp, const void* wpwl, const float* bpwl, void* y,
                    double flops, double bytes, hipStream_t s);
void launch_ers2_fused(const bf16_t* x, int N, int H, int W, int OH, int OW, int pad_t, int pad_l, int cs_in, int mid,
                       int cs_out, const bf16_t* wexp, const float* bexp, const bf16_t* wpwl, const float* bpwl,
                       bf16_t* y, double flops, double bytes, hipStream_t s, uint8_t* y8 = nullptr);

// Decoded frames -> model input: uint8 (N,H,W) grey or (N,H,W,3) BGR -> fp32 (N,H,W) in [0, 1]
// (_preprocess_frame, run_mri_video_inference.py:34-54, on frames already at the model's size).  (preprocess.hip)
void launch_preprocess(const uint8_t* frames, int N, int H, int W, int channels, float* out, hipStream_t s);

// The same with the resize on the device: uint8 (N,h,w) grey or (N,h,w,3) BGR at the scanner's size -> fp32
// (N,out_h,out_w).  interp 0 = cv2.INTER_LINEAR, 1 = cv2.INTER_AREA (OpenCV's 8-bit two-tap path; no axis may
// shrink); norm 0 = per-frame z-score + min-max (_preprocess_frame), 1 = / 255 (preprocess_rtmri_data.py:99-113).
// At most 65536 pixels a frame on either side.  One workgroup per frame, no workspace.  (frames.hip)
void launch_frames(const uint8_t* frames, int N, int h, int w, int channels, int out_h, int out_w, int interp, int norm,
                   float* out, hipStream_t s);
// n_masks masked variants of every frame: masks (n_masks,h,w) fp32, every byte of every channel becomes
// (uint8)clip((float)byte * mask[y][x], 0, 255) before BGR -> grey; out (n_masks,N,out_h,out_w).  Grid (N, n_masks),
// the masks read from global memory while the frame is staged.  (frames.hip)
void launch_frames_masked(const uint8_t* frames, int N, int h, int w, int channels, const float* masks, int n_masks,
                          int out_h, int out_w, int interp, int norm, float* out, hipStream_t s);

// Occlusion scores and map of one clip: mel (V,T,n_mels), variant 0 the baseline; band_mask (n_bands,n_mels) 0 / 1;
// score (V-1,nb), per_frame (V-1,T,nb) or null, map (nb,h,w) or null from masks (V-1,h,w); nb = n_bands + 1 (the
// last column is all bins).  Two launches, fixed summation order.  (occlusion.hip)
void launch_occlusion_reduce(const float* mel, int V, int T, int n_mels, const float* band_mask, int n_bands,
                             const float* masks, int h, int w, int normalize, float* score, float* per_frame, float* map,
                             hipStream_t s);

// Global average pool: x (N,P,cs) T -> feats (N,C) fp32 (dense, row stride C).
template <typename T>
void launch_gap(const T* x, int N, int P, int C, int cs, float* feats, hipStream_t s);

// One BiLSTM time step for both directions (step s: fwd t = s, bwd t = T-1-s).
// pre (B,T,8H) fp32 = x W_ih^T + b_ih + b_hh for [fwd | bwd]; whh (2,4H,H); hs (2,B,T,H); cst (2,B,H).
void launch_lstm_step(const float* pre, const float* whh, float* hs, float* cst, int B, int T, int H,
                      int step, hipStream_t s);

// The same recurrence for all T steps in ONE launch (lstm_persistent.hip; H = 640 only): W_hh resident in VGPRs
// across co-resident workgroups that hand h_t to each other every step.  Five kernels, chosen by lstm_plan
// (lstm_route.hpp): lstm_small (B <= 4 or 8: data-tagged fp32 granules, VALU dot products), lstm_x3g (split engines,
// B <= 16: three bf16 MFMA terms over hi / lo operands, split granules), lstm_x3 (split engines above that: h
// published split by write-through stores behind per-workgroup flags), lstm_mid (fp32, B <= 16: granules in chunks
// whose sweep overlaps the previous chunk's dot products) and lstm_persistent (exact-f32 MFMA, counter barrier).
// `sync`: lstm_sync_bytes(p.engine_sync) of device memory: the engine's own buffer where the plan says so (its
// granule tags continue across calls from *epoch, no memset; a null epoch zeroes it every call), else the call's
// workspace (reset by the launcher).  `spin_max` bounds each hand-off wait (polls with s_sleep 1); on a timeout the
// kernel stores 1 to `err_host` (pinned, host-mapped) and writes NaN to the rest of the outputs.
constexpr unsigned LSTM_SPIN_MAX = 1u << 24;
size_t lstm_sync_bytes(bool engine);
void launch_lstm(const LstmPlan& p, const float* pre, const float* whh, float* hs, int B, int T, int H, void* sync,
                 unsigned* epoch, unsigned spin_max, unsigned* err_host, hipStream_t s);

// Sliding-window BiLSTM (lstm_window.hip): S independent windows of at most W <= 16 steps, one launch per step,
// no cross-workgroup communication.  H = 640 only.
bool lstm_window_supported(int H);
// W_hh (4H, H) of the two directions -> [dir][unit group of 16][gate x 16 + unit][H] fp32 (2 x 4H x H floats): one
// workgroup's 64 rows hold all four gates of its hidden units
void pack_lstm_window_whh(const float* const whh[2], int H, float* out);
// clip table tab = [off | len | ctx | wbase | obase] (B ints each) -> win[w] = {first projected row, k | delay << 8}.
// latest: one window per output frame t >= ctx, k = min(W, t + 1), delay = W - k; mean: the len - min(len, W) + 1
// full windows of a clip (one of k = len steps where len <= W), delay = 0.  max_windows: the largest count per clip
void launch_lstm_window_table(const int* tab, int B, int W, bool mean, int max_windows, int2* win, hipStream_t s);
// step 0 (elementwise): hop = the next step's operand [dirs][S] (fp32 rows of H, or split [hi H | lo H] bf16; null
// if no step follows), c [dirs][S][H]; hf0 / hf1: fp32 h of the forward / reverse direction (may be null).  latest:
// the reverse direction is this step alone, on the window's last frame, and is written to hf1 only
void launch_lstm_window_step0(const float* pre, const int2* win, int S, bool latest, bool split, void* hop, float* c,
                              float* hf0, float* hf1, hipStream_t s);
// recurrent step j >= 1 of `dirs` directions: hin -> hout (operand layout; hout may be null on the last step), c
// in place, hf (may be null) fp32 h at hf + dir * hf_dir_stride + window * H
void launch_lstm_window_step(const float* pre, const float* wperm, const int2* win, int S, int j, int dirs, bool split,
                             const void* hin, void* hout, float* c, float* hf, long hf_dir_stride, hipStream_t s);
// mean merge: hf [2][W][S][H] -> hm [2][N][H] (forward | reverse averages per packed output row, fixed order)
void launch_lstm_window_mean(const float* hf, const int* tab, int B, int W, int S, long N, int max_len, float* hm,
                             hipStream_t s);

// pair rows: hf [2][W][S][H] of S full windows -> y (S, W, H), y[p][s] = hf[fwd][s][p] + hf[rev][W - 1 - s][p];
// y2 (may be null) receives the same rows
void launch_lstm_window_pairs(const float* hf, int W, int S, float* y, float* y2, hipStream_t s);

// validation metrics (metrics.hip; m2s.h "fused mel metrics"): MET_PART floats of partial sums per sequence, then the
// per-group reduction
constexpr int MET_PART = 32;
struct MelMetricsArgs {
  const float *pred, *target, *mask;
  int B, T, M, group;
  const float *freq_w, *time_w;
  float coeff[3];  // delta, accel, latest
  int bands[16], n_bands;
  const float *mean, *sd;
  int n_mfcc;
  double* acc;
  float *out, *per_seq, *part;
};
void launch_mel_metrics(const MelMetricsArgs& a, hipStream_t s);

// head: y = hs[0] + hs[1] (sum merge); out = y W^T + b.  wt (H, n_mels) transposed weight.
// merged: hs is one plane of rows that are already sum-merged (the pair rows)
void launch_mel_head(const float* hs, int rows, int H, const float* wt, const float* b, int n_mels,
                     float* out, hipStream_t s, bool merged = false);

// mel glue: db = x*std + mean; ln = log(clamp(10^(db/10), 1e-5)).  Any output may be null.
// ln_t (rows, cs) T channel-last copy feeds the vocoder.
template <typename T>
void launch_mel_glue(const float* x, int rows, int n_mels, const float* mean, const float* std_,
                     float* db, float* ln, T* ln_t, int cs, hipStream_t s);

// mel (B,C,T) fp32 [layout 0] or (B,T,C) fp32 [layout 1] -> (B,T,cs) T.
template <typename T>
void launch_mel_to_nlc(const float* mel, int B, int C, int Tn, int layout, T* y, int cs, hipStream_t s);

// conv_post: leaky_relu(0.01) -> right pad 6 -> Conv1d(C,1,7) -> tanh.  x (B,L,cs) T -> wav (B,L) fp32.
template <typename T>
void launch_conv_post(const T* x, int B, int L, int C, int cs, const float* w /*[7][C]*/, float bias,
                      float* wav, hipStream_t s);

// y = a + b (fp32, n elements)
void launch_add2(const float* a, const float* b, float* y, long n, hipStream_t s);
// fp8 engines: y (n bytes, e4m3) = lrelu(x) for bf16 x, n % 8 == 0  (kernels.hip)
void launch_lrelu_e4m3(const bf16_t* x, uint8_t* y, long n, float slope, hipStream_t s);
// fp8 engines, HiFi-GAN MRF conv at C in {128, 256} (models.py:11-49, causal left pad (k - 1) dil): x8 e4m3
// (B, L, C) already LeakyReLU'd; w8 e4m3 [C][k C] tap-major (pack_gemm_f8), per-channel scales; v = conv + bias
// (+ res bf16); y bf16 = v, or with accum 1 / 2 the MRF running sum y + v / (y + v) / accum_div; y8 (e4m3) =
// lrelu(v, slope8).  Either output may be null.  (gemm128.hip)
bool conv1d_f8_supported(int C, int k);
void launch_conv1d_f8(const void* x8, int B, int L, int C, int k, int dil, const void* w8, const float* wscale,
                      const float* bias, const void* res, void* y, void* y8, float slope8, int accum, float accum_div,
                      hipStream_t s, double flops, double bytes);

// Ragged batches (ragged.hip): clip b of len[b] steps owns packed rows off[b] .. off[b] + len[b] - 1; the dense
// kernels run on (B, Tmax, ...) blocks.  tab = device table [off: B ints | len: B ints].
// packed gate pre-activations (N, width) -> padded (B, Tmax, width), exact zero rows at t >= len[b]
void launch_ragged_pre_scatter(const float* pre_packed, const int* tab, int B, int Tmax, int width, float* pre,
                               hipStream_t s);
// launch_mel_head (and the sum merge y = hs[0] + hs[1]) on the valid rows of hs (2, B, Tmax, H) -> packed
// y (N, H) / mel_norm (N, n_mels); either may be null.  Rounds as mel_head_kernel / add2_kernel do.
void launch_ragged_head_gather(const float* hs, const int* tab, int B, int Tmax, int H, const float* wt, const float* b,
                               int n_mels, float* y, float* mel_norm, hipStream_t s);
// packed x (N, n_mels) -> padded channel-last ln_t (B, Tmax, cs) with exact zeros at t >= len[b].  mean != null:
// x is mel_norm, launch_mel_glue's arithmetic, packed db / ln (N, n_mels) outputs (may be null); mean == null: x
// is the ln-mel itself (launch_mel_to_nlc, layout 1).
template <typename T>
void launch_ragged_glue(const float* x, const int* tab, int B, int Tmax, int n_mels, const float* mean,
                        const float* std_, float* db, float* ln, T* ln_t, int cs, hipStream_t s);
// zeroes `halo` rows from row len[b] * scale of clip b in a buffer of `rows` = Tmax * scale rows per clip, a row =
// row_bytes contiguous bytes (fp32, bf16 or the split hi / lo pair); nothing past the clip's own rows
void launch_ragged_tail_mask(void* x, const int* tab, int B, int rows, int scale, int halo, size_t row_bytes,
                             hipStream_t s);
// padded wav (B, Tmax * hop) -> packed (N * hop)
void launch_ragged_wav_pack(const float* wav_padded, const int* tab, int B, int Tmax, int hop, float* wav,
                            hipStream_t s);

// Streaming vocoder (vocoder_chunk.hip): the chunk call's glue between the dense generator kernels.
// x (B, rows_in, row_bytes) -> y (B, rows_out, row_bytes), y[b][r] = x[b][drop + r]; a row = row_bytes contiguous
// bytes in any activation storage (a multiple of 16, as in launch_ragged_tail_mask); drop + rows_out <= rows_in
void launch_crop_rows(const void* x, int B, long rows_in, long drop, long rows_out, size_t row_bytes, void* y,
                      hipStream_t s);
// padded wav (B, T * hop) -> the packed emitted rows: clip b's rows src[b] .. src[b] + n[b] - 1 go to packed rows
// dst[b] ..., hop samples a row; src / dst / n = device arrays of B ints
void launch_chunk_wav_pack(const float* wav_padded, const int* src, const int* dst, const int* n, int B, int T, int hop,
                           float* wav, hipStream_t s);

// (rows, cs) T -> (rows, C) fp32 dense (debug taps)
template <typename T>
void launch_unpad(const T* x, long rows, int C, int cs, float* y, hipStream_t s);

}  // namespace m2s
