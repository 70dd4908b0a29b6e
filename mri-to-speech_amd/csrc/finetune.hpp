// Fine-tuning engine of the BiLSTM and the mel head (include/m2s.h "fine-tuning", DESIGN.md "Fine-tuning"): the
// kernels' launchers (lstm_window_train.hip, finetune.hip) and the engine that chains them (finetune.cpp).
#pragma once

#include <cstdint>
#include <map>
#include <vector>

#include "../../include/m2s.h"
#include "m2s_common.hpp"

namespace m2s {

constexpr int FT_H = 640;     // rnn_hidden
constexpr int FT_G = 4 * 640; // gate columns of one direction
constexpr int FT_IN = 208;    // encoder features
constexpr int FT_MAXM = 256;  // mel bins
constexpr int FT_MAXW = 16;   // window

// the device hyper-parameter block (m2s_finetune_set_hyper writes it, kernels read it)
struct FtHyper {
  float lr, wd, max_norm, drop_scale;  // drop_scale = 1 / (1 - p)
  uint32_t drop_thr, seed;             // keep iff mix >= drop_thr = floor(p 2^32)
  float coeff[3];                      // delta, accel, latest
  float freq_w[FT_MAXM];
  float time_w[FT_MAXW];
};
// what the reductions leave for later kernels of the step
struct FtScalars {
  float k_mse, k_delta, k_accel, k_latest;  // 2 coeff / denominator of the four LOSS terms
  float norm, coef;                         // gradient norm before clipping, the clip factor
  float bc1, sqrt_bc2;                      // AdamW's bias corrections at the step being taken
};

// ---- lstm_window_train.hip -----------------------------------------------------------------------------------
// C[z] (M x N, row stride ldc) = A[z] (M x K) B[z] (K x N) (+ bias0[z] + bias1[z] per column) on the exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32), any element strides: A[m][k] at a_m m + a_k k, B[k][n] at b_k k + b_n n.  64 x 64 tiles,
// K in ascending steps of 16.  splits > 1: split z' of every batch covers k in [z' kchunk, (z' + 1) kchunk) and goes
// to part[z][z'] (M x N dense); launch_ft_gemm then adds the partials in ascending order into C (no bias).
struct FtGemm {
  const float *A = nullptr, *B = nullptr;
  float* C = nullptr;
  int M = 0, N = 0, K = 0, batch = 1;
  long a_m = 0, a_k = 0, b_k = 0, b_n = 0, ldc = 0;
  long sA = 0, sB = 0, sC = 0;
  const float *bias0 = nullptr, *bias1 = nullptr;
  long sBias = 0;
  int splits = 1, kchunk = 0;
  float* part = nullptr;
};
// the fixed split-K partition of a reduction length K (a function of K alone): up to 16 parts of a multiple of 16
void ft_split(int K, int* splits, int* kchunk);
void launch_ft_gemm(const FtGemm& g, const char* name, hipStream_t s);

// train-mode cell of local step st of both directions: gate pre-activations = the gathered projected row (+ rec
// [dir][P][2560], the recurrent GEMM, when st > 0) -> post-activation gates [dir][W][P][2560], c and h [dir][W][P][640]
void launch_ft_cell_forward(const float* pre, const int* win, int P, int W, int st, const float* rec, float* gates,
                            float* c, float* h, hipStream_t s);
// backward cell of local step st: dh = dhrec [dir][P][640] (st < W - 1) + dropout(dy)[p][frame]; writes dgates
// [dir][W][P][2560] at st and carries dc f in dcn [dir][P][640]
void launch_ft_cell_backward(const float* dy, const FtHyper* hy, const int64_t* step, const float* dhrec,
                             const float* gates, const float* c, int P, int W, int st, float* dcn, float* dgates,
                             hipStream_t s);
// y (P, W, 640) = (h[fwd][s][p] + h[rev][W - 1 - s][p]) mask / (1 - p); train = false: no mask
void launch_ft_merge_dropout(const float* h, const FtHyper* hy, const int64_t* step, int P, int W, bool train, float* y,
                             hipStream_t s);
// dpre (rows, 5120): row r receives dgates of the windows r - s, s ascending
void launch_ft_fold(const float* dgates, const int* rowtab, int rows, int P, int W, float* dpre, hipStream_t s);
// out0[c] (and out1[c], may be null) = sum over R rows of x (R, C) by a fixed partition: chunks of 1024 rows summed
// in double into part (ceil(R / 1024), C) doubles, then the chunks in ascending order
int ft_colsum_chunks(long R);
void launch_ft_colsum(const float* x, long R, int C, double* part, float* out0, float* out1, hipStream_t s);

// ---- finetune.hip --------------------------------------------------------------------------------------------
void launch_ft_gather(const float* target, const float* mask, const int* win, int P, int W, int M, float* tgt,
                      float* msk, hipStream_t s);
void launch_ft_denominators(const float* msk, const FtHyper* hy, int P, int W, int M, FtScalars* sc, hipStream_t s);
void launch_ft_criterion_grad(const float* pred, const float* tgt, const float* msk, const FtHyper* hy,
                              const FtScalars* sc, int P, int W, int M, float* dpred, hipStream_t s);
int ft_norm_chunks(long n);
void launch_ft_sumsq(const float* g, long n, double* part, hipStream_t s);
// norm, coef, the bias corrections of step *step + 1 -> sc; the 8 slots -> slots / out_slots (may be null)
void launch_ft_norm(const double* part, int chunks, const FtHyper* hy, const int64_t* step, const float* mslots,
                    FtScalars* sc, float* slots, float* out_slots, hipStream_t s);
void launch_ft_adamw(float* p, const float* g, float* m, float* v, long n, const FtHyper* hy, const FtScalars* sc,
                     hipStream_t s);
void launch_ft_step_inc(int64_t* step, hipStream_t s);

// ---- finetune.cpp ----------------------------------------------------------------------------------------------
class FineTune {
 public:
  FineTune(const m2s_tensor* sd, int n, int n_mels, int device);
  ~FineTune();
  FineTune(const FineTune&) = delete;
  FineTune& operator=(const FineTune&) = delete;
  int device() const { return device_; }
  int n_mels() const { return M_; }
  void set_hyper(const m2s_finetune_hyper& h, const float* freq_w, const float* time_w, int window, hipStream_t s);
  size_t workspace_bytes(const int* lengths, int B, int window) const;
  void step(const float* feats, const float* target, const float* mask, const int* lengths, int B, long rows, int window,
            float* out_slots, void* ws, size_t ws_bytes, hipStream_t s);
  void forward(const float* feats, const int* lengths, int B, long rows, int window, bool train, float* mel_norm,
               void* ws, size_t ws_bytes, hipStream_t s);
  void grads(float* const* g10, hipStream_t s);
  void export_state(float* const* p10, float* const* m10, float* const* v10, int64_t* step, hipStream_t s);
  void import_moments(const float* const* m10, const float* const* v10, const int64_t* step, hipStream_t s);

 private:
  struct Plan {
    int B = 0, W = 0, P = 0;
    long rows = 0;
  };
  struct Bufs;
  Plan plan(const int* lengths, int B, long rows, int window) const;
  Bufs layout(class Workspace& ws, const Plan& p) const;
  void stage_table(const int* lengths, const Plan& p, hipStream_t s);
  void run_forward(const float* feats, const Plan& p, const Bufs& b, bool train, float* pred, hipStream_t s);
  size_t count(int i) const { return off_[i + 1] - off_[i]; }

  int device_ = 0, M_ = 0, hyper_window_ = 0;
  size_t off_[M2S_FT_TENSORS + 1] = {};
  float *params_ = nullptr, *grads_ = nullptr, *m_ = nullptr, *v_ = nullptr;
  int64_t* step_ = nullptr;
  FtHyper* hyper_ = nullptr;
  FtScalars* scal_ = nullptr;
  float* slots_ = nullptr;  // the last step's 8 slots
  float host_coeff_[3] = {0.f, 0.f, 0.f};
  // the staged window tables, keyed by [window, lengths...]: [win row0: P | rowp: rows | lo: rows | hi: rows].  An
  // entry keeps its device address for the engine's lifetime (a captured step holds it); tab_ = the current call's
  struct Table {
    int* dev = nullptr;
    std::vector<int> host;
  };
  std::map<std::vector<int>, Table> tables_;
  int* tab_ = nullptr;
};

}  // namespace m2s
