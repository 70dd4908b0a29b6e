// The fine-tuning engine (include/m2s.h "fine-tuning", DESIGN.md "Fine-tuning"): fp32 masters of the BiLSTM and
// mel head, their gradients and AdamW moments, the device step count and hyper-parameter block, and the launch
// sequence of one optimisation step.  Nothing in a step reads device memory back to the host.
#include "finetune.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "model.hpp"
#include "prof.hpp"

namespace m2s {

namespace {

const char* const kNames[M2S_FT_TENSORS] = {
    "rnn.lstm.weight_ih_l0",         "rnn.lstm.weight_hh_l0",         "rnn.lstm.bias_ih_l0",
    "rnn.lstm.bias_hh_l0",           "rnn.lstm.weight_ih_l0_reverse", "rnn.lstm.weight_hh_l0_reverse",
    "rnn.lstm.bias_ih_l0_reverse",   "rnn.lstm.bias_hh_l0_reverse",   "head.weight",
    "head.bias"};

bool capturing(hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  M2S_HIP(hipStreamIsCapturing(s, &cap));
  return cap != hipStreamCaptureStatusNone;
}

template <class T>
T* dev_alloc(size_t n) {
  void* p = nullptr;
  M2S_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
  return static_cast<T*>(p);
}

}  // namespace

struct FineTune::Bufs {
  float *pre, *rec, *gates, *c, *h, *y, *pred;                  // forward
  float *tgt, *msk, *part, *mslots;                             // criterion
  float *dpred, *dy, *dhrec, *dcn, *dgates, *dpre, *gpart;      // backward
  double *cpart, *npart;                                        // column-sum and norm partials
};

FineTune::FineTune(const m2s_tensor* sd, int n, int n_mels, int device) : device_(device), M_(n_mels) {
  M2S_CHECK(n_mels >= 1 && n_mels <= FT_MAXM, "finetune: n_mels outside 1..256");
  const StateDict d = make_state_dict(sd, n);
  const size_t sizes[M2S_FT_TENSORS] = {(size_t)FT_G * FT_IN, (size_t)FT_G * FT_H, FT_G, FT_G,
                                        (size_t)FT_G * FT_IN, (size_t)FT_G * FT_H, FT_G, FT_G,
                                        (size_t)n_mels * FT_H, (size_t)n_mels};
  off_[0] = 0;
  for (int i = 0; i < M2S_FT_TENSORS; ++i) off_[i + 1] = off_[i] + sizes[i];
  std::vector<float> host(off_[M2S_FT_TENSORS]);
  for (int i = 0; i < M2S_FT_TENSORS; ++i) {
    auto it = d.find(kNames[i]);
    M2S_CHECK(it != d.end(), std::string("missing state-dict key: ") + kNames[i]);
    M2S_CHECK(it->second.numel() == sizes[i],
              std::string("state-dict key ") + kNames[i] + " has the wrong shape (rnn_hidden must be 640)");
    std::memcpy(host.data() + off_[i], it->second.data, sizes[i] * sizeof(float));
  }
  const size_t total = off_[M2S_FT_TENSORS];
  params_ = dev_alloc<float>(total);
  grads_ = dev_alloc<float>(total);
  m_ = dev_alloc<float>(total);
  v_ = dev_alloc<float>(total);
  step_ = dev_alloc<int64_t>(1);
  hyper_ = dev_alloc<FtHyper>(1);
  scal_ = dev_alloc<FtScalars>(1);
  slots_ = dev_alloc<float>(M2S_FT_SLOTS);
  M2S_HIP(hipMemcpy(params_, host.data(), total * sizeof(float), hipMemcpyHostToDevice));
  M2S_HIP(hipMemset(grads_, 0, total * sizeof(float)));
  M2S_HIP(hipMemset(m_, 0, total * sizeof(float)));
  M2S_HIP(hipMemset(v_, 0, total * sizeof(float)));
  M2S_HIP(hipMemset(step_, 0, sizeof(int64_t)));
  M2S_HIP(hipMemset(hyper_, 0, sizeof(FtHyper)));
  M2S_HIP(hipMemset(scal_, 0, sizeof(FtScalars)));
  M2S_HIP(hipMemset(slots_, 0, M2S_FT_SLOTS * sizeof(float)));
  M2S_HIP(hipDeviceSynchronize());
}

FineTune::~FineTune() {
  for (void* p : {(void*)params_, (void*)grads_, (void*)m_, (void*)v_, (void*)step_, (void*)hyper_, (void*)scal_,
                  (void*)slots_})
    if (p) (void)hipFree(p);
  for (auto& kv : tables_)
    if (kv.second.dev) (void)hipFree(kv.second.dev);
}

void FineTune::set_hyper(const m2s_finetune_hyper& h, const float* freq_w, const float* time_w, int window,
                         hipStream_t s) {
  M2S_CHECK(freq_w && time_w, "finetune_set_hyper: null freq_w or time_w");
  if (capturing(s))  // the copy's host source and the host-side window / coefficients are not stream-ordered
    throw Error(M2S_E_STATE, "finetune_set_hyper: cannot be captured into a graph; set the hyper-parameters before");
  M2S_CHECK(window >= 1 && window <= FT_MAXW, "finetune_set_hyper: window outside 1..16");
  M2S_CHECK(h.dropout >= 0.f && h.dropout < 1.f, "finetune_set_hyper: dropout outside [0, 1)");
  M2S_CHECK(std::isfinite(h.lr) && std::isfinite(h.weight_decay) && std::isfinite(h.max_norm),
            "finetune_set_hyper: non-finite hyper-parameter");
  FtHyper d{};
  d.lr = h.lr, d.wd = h.weight_decay, d.max_norm = h.max_norm;
  d.drop_scale = 1.0f / (1.0f - h.dropout);
  d.drop_thr = (uint32_t)std::floor((double)h.dropout * 4294967296.0);
  d.seed = h.seed;
  d.coeff[0] = h.delta_coeff, d.coeff[1] = h.accel_coeff, d.coeff[2] = h.latest_coeff;
  for (int i = 0; i < M_; ++i) d.freq_w[i] = freq_w[i];
  for (int i = 0; i < window; ++i) d.time_w[i] = time_w[i];
  // a pageable source: the runtime stages it before the call returns, the copy itself is stream-ordered
  M2S_HIP(hipMemcpyAsync(hyper_, &d, sizeof(FtHyper), hipMemcpyHostToDevice, s));
  for (int i = 0; i < 3; ++i) host_coeff_[i] = d.coeff[i];
  hyper_window_ = window;
}

FineTune::Plan FineTune::plan(const int* lengths, int B, long rows, int window) const {
  M2S_CHECK(lengths, "finetune: null lengths");
  M2S_CHECK(window >= 1 && window <= FT_MAXW, "finetune: window = " + std::to_string(window) + " outside 1..16");
  M2S_CHECK(B >= 1, "finetune: B < 1");
  long n = 0, P = 0;
  for (int b = 0; b < B; ++b) {
    M2S_CHECK(lengths[b] >= 1, "finetune: lengths[" + std::to_string(b) + "] < 1");
    M2S_CHECK(lengths[b] >= window, "finetune: lengths[" + std::to_string(b) + "] = " + std::to_string(lengths[b]) +
                                        " is shorter than the window of " + std::to_string(window));
    n += lengths[b];
    P += lengths[b] - window + 1;
  }
  M2S_CHECK(rows < 0 || n == rows, "finetune: sum(lengths) = " + std::to_string(n) + " != rows = " + std::to_string(rows));
  // the GEMMs' row tiles (64 rows) go on a 65535-wide grid axis
  M2S_CHECK((double)P * window <= 4000000.0 && n <= 4000000, "finetune: more than 4000000 pair rows or frame rows");
  Plan p;
  p.B = B, p.W = window, p.P = (int)P, p.rows = n;
  return p;
}

FineTune::Bufs FineTune::layout(Workspace& ws, const Plan& p) const {
  const size_t P = (size_t)p.P, W = (size_t)p.W, R = (size_t)p.rows, M = (size_t)M_;
  Bufs b{};
  b.pre = ws.take<float>(R * 2 * FT_G);
  b.rec = ws.take<float>(2 * P * FT_G);
  b.gates = ws.take<float>(2 * W * P * FT_G);
  b.c = ws.take<float>(2 * W * P * FT_H);
  b.h = ws.take<float>(2 * W * P * FT_H);
  b.y = ws.take<float>(P * W * FT_H);
  b.pred = ws.take<float>(P * W * M);
  b.tgt = ws.take<float>(P * W * M);
  b.msk = ws.take<float>(P * W);
  b.part = ws.take<float>(P * MET_PART);
  b.mslots = ws.take<float>(M2S_METRICS_SLOTS);
  b.dpred = ws.take<float>(P * W * M);
  b.dy = ws.take<float>(P * W * FT_H);
  b.dhrec = ws.take<float>(2 * P * FT_H);
  b.dcn = ws.take<float>(2 * P * FT_H);
  b.dgates = ws.take<float>(2 * W * P * FT_G);
  b.dpre = ws.take<float>(R * 2 * FT_G);
  int sh, sw = 1, si, kc;
  ft_split((int)(P * W), &sh, &kc);
  if (W > 1) ft_split((int)(P * (W - 1)), &sw, &kc);
  ft_split((int)R, &si, &kc);
  const size_t gp = std::max({(size_t)sh * M * FT_H, W > 1 ? (size_t)2 * sw * FT_G * FT_H : 0, (size_t)2 * si * FT_G * FT_IN});
  b.gpart = ws.take<float>(gp);
  b.cpart = ws.take<double>((size_t)ft_colsum_chunks((long)(P * W)) * std::max<size_t>(M, FT_G));
  b.npart = ws.take<double>((size_t)ft_norm_chunks((long)off_[M2S_FT_TENSORS]));
  return b;
}

size_t FineTune::workspace_bytes(const int* lengths, int B, int window) const {
  const Plan p = plan(lengths, B, -1, window);
  return Workspace::bytes([&](Workspace& ws) { layout(ws, p); });
}

// [win row0: P | rowp: rows | lo: rows | hi: rows], staged once per (lengths, window)
// A staged table lives, at its own address, until the engine is destroyed: a captured step holds that address, and
// calls with other lengths in between (a validation batch) stage their own table beside it.
void FineTune::stage_table(const int* lengths, const Plan& p, hipStream_t s) {
  std::vector<int> key;
  key.reserve((size_t)p.B + 1);
  key.push_back(p.W);
  key.insert(key.end(), lengths, lengths + p.B);
  auto it = tables_.find(key);
  if (it != tables_.end()) {
    tab_ = it->second.dev;
    return;
  }
  if (capturing(s))
    throw Error(M2S_E_STATE, "finetune: the window table of these lengths is not staged; run one eager call with "
                             "them before capturing");
  const size_t n = (size_t)p.P + 3 * (size_t)p.rows;
  Table t;
  t.host.assign(n, 0);
  int* win = t.host.data();
  int *rowp = win + p.P, *lo = rowp + p.rows, *hi = lo + p.rows;
  int off = 0, wbase = 0;
  for (int b = 0; b < p.B; ++b) {
    const int len = lengths[b], nwin = len - p.W + 1;
    for (int i = 0; i < nwin; ++i) win[wbase + i] = off + i;
    for (int t = 0; t < len; ++t) rowp[off + t] = wbase + t, lo[off + t] = wbase, hi[off + t] = wbase + nwin;
    off += len, wbase += nwin;
  }
  t.dev = dev_alloc<int>(n);
  const hipError_t e = hipMemcpyAsync(t.dev, t.host.data(), n * sizeof(int), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) (void)hipStreamSynchronize(s);  // once per new (lengths, window): the host copy ends here
  if (e != hipSuccess) {
    (void)hipFree(t.dev);
    M2S_HIP(e);
  }
  t.host.clear();
  t.host.shrink_to_fit();
  tab_ = t.dev;
  tables_.emplace(std::move(key), std::move(t));
}

void FineTune::run_forward(const float* feats, const Plan& p, const Bufs& b, bool train, float* pred, hipStream_t s) {
  const int P = p.P, W = p.W;
  const long dirstride = (long)(off_[4] - off_[0]);
  StageTag tag("finetune");
  {
    FtGemm g;  // the projection, once per frame row, both directions
    g.A = feats, g.a_m = FT_IN, g.a_k = 1, g.sA = 0;
    g.B = params_ + off_[0], g.b_k = 1, g.b_n = FT_IN, g.sB = dirstride;
    g.C = b.pre, g.ldc = 2 * FT_G, g.sC = FT_G;
    g.bias0 = params_ + off_[2], g.bias1 = params_ + off_[3], g.sBias = dirstride;
    g.M = (int)p.rows, g.N = FT_G, g.K = FT_IN, g.batch = 2;
    launch_ft_gemm(g, "ft_gemm_kernel<project>", s);
  }
  for (int st = 0; st < W; ++st) {
    if (st > 0) {
      FtGemm g;  // h_{st-1} W_hh^T: M = P windows, N = 2560, K = 640
      g.A = b.h + (size_t)(st - 1) * P * FT_H, g.a_m = FT_H, g.a_k = 1, g.sA = (long)W * P * FT_H;
      g.B = params_ + off_[1], g.b_k = 1, g.b_n = FT_H, g.sB = dirstride;
      g.C = b.rec, g.ldc = FT_G, g.sC = (long)P * FT_G;
      g.M = P, g.N = FT_G, g.K = FT_H, g.batch = 2;
      launch_ft_gemm(g, "ft_gemm_kernel<recurrent>", s);
    }
    launch_ft_cell_forward(b.pre, tab_, P, W, st, b.rec, b.gates, b.c, b.h, s);
  }
  launch_ft_merge_dropout(b.h, hyper_, step_, P, W, train, b.y, s);
  {
    FtGemm g;  // the head
    g.A = b.y, g.a_m = FT_H, g.a_k = 1;
    g.B = params_ + off_[8], g.b_k = 1, g.b_n = FT_H;
    g.C = pred, g.ldc = M_;
    g.bias0 = params_ + off_[9];
    g.M = P * W, g.N = M_, g.K = FT_H;
    launch_ft_gemm(g, "ft_gemm_kernel<head>", s);
  }
}

void FineTune::forward(const float* feats, const int* lengths, int B, long rows, int window, bool train, float* mel_norm,
                       void* ws, size_t ws_bytes, hipStream_t s) {
  const Plan p = plan(lengths, B, rows, window);
  M2S_CHECK(!train || window == hyper_window_, "finetune_forward: window differs from the last set_hyper");
  Workspace w(ws, ws_bytes);
  const Bufs b = layout(w, p);
  stage_table(lengths, p, s);
  run_forward(feats, p, b, train, mel_norm, s);
}

void FineTune::step(const float* feats, const float* target, const float* mask, const int* lengths, int B, long rows,
                    int window, float* out_slots, void* ws, size_t ws_bytes, hipStream_t s) {
  const Plan p = plan(lengths, B, rows, window);
  M2S_CHECK(window == hyper_window_, "finetune_step: window " + std::to_string(window) +
                                         " differs from the last set_hyper's " + std::to_string(hyper_window_));
  Workspace w(ws, ws_bytes);
  const Bufs b = layout(w, p);
  stage_table(lengths, p, s);
  const int P = p.P, W = p.W, M = M_, R = (int)p.rows;
  const long dirstride = (long)(off_[4] - off_[0]);
  const int* rowtab = tab_ + P;
  run_forward(feats, p, b, true, b.pred, s);
  StageTag tag("finetune");
  // ---- criterion: the slots from metrics.hip on the gathered pairs as one group, then dLOSS / dpred ----------
  launch_ft_gather(target, mask, tab_, P, W, M, b.tgt, b.msk, s);
  {
    MelMetricsArgs a{};
    a.pred = b.pred, a.target = b.tgt, a.mask = b.msk;
    a.B = P, a.T = W, a.M = M, a.group = P;
    a.freq_w = hyper_->freq_w, a.time_w = hyper_->time_w;
    for (int i = 0; i < 3; ++i) a.coeff[i] = host_coeff_[i];
    a.out = b.mslots, a.part = b.part;
    launch_mel_metrics(a, s);
  }
  launch_ft_denominators(b.msk, hyper_, P, W, M, scal_, s);
  launch_ft_criterion_grad(b.pred, b.tgt, b.msk, hyper_, scal_, P, W, M, b.dpred, s);
  // ---- head backward ------------------------------------------------------------------------------------------
  {
    FtGemm g;  // dW = dpred^T drop(y), K = P W
    g.A = b.dpred, g.a_m = 1, g.a_k = M;
    g.B = b.y, g.b_k = FT_H, g.b_n = 1;
    g.C = grads_ + off_[8], g.ldc = FT_H;
    g.M = M, g.N = FT_H, g.K = P * W;
    ft_split(g.K, &g.splits, &g.kchunk);
    g.part = b.gpart;
    launch_ft_gemm(g, "ft_gemm_kernel<head_dw>", s);
  }
  launch_ft_colsum(b.dpred, (long)P * W, M, b.cpart, grads_ + off_[9], nullptr, s);
  {
    FtGemm g;  // dy = dpred W
    g.A = b.dpred, g.a_m = M, g.a_k = 1;
    g.B = params_ + off_[8], g.b_k = FT_H, g.b_n = 1;
    g.C = b.dy, g.ldc = FT_H;
    g.M = P * W, g.N = FT_H, g.K = M;
    launch_ft_gemm(g, "ft_gemm_kernel<head_dy>", s);
  }
  // ---- backward through time ---------------------------------------------------------------------------------
  for (int st = W - 1; st >= 0; --st) {
    if (st < W - 1) {
      FtGemm g;  // dgates_{st+1} W_hh: M = P, N = 640, K = 2560
      g.A = b.dgates + (size_t)(st + 1) * P * FT_G, g.a_m = FT_G, g.a_k = 1, g.sA = (long)W * P * FT_G;
      g.B = params_ + off_[1], g.b_k = FT_H, g.b_n = 1, g.sB = dirstride;
      g.C = b.dhrec, g.ldc = FT_H, g.sC = (long)P * FT_H;
      g.M = P, g.N = FT_H, g.K = FT_G, g.batch = 2;
      launch_ft_gemm(g, "ft_gemm_kernel<bptt>", s);
    }
    launch_ft_cell_backward(b.dy, hyper_, step_, b.dhrec, b.gates, b.c, P, W, st, b.dcn, b.dgates, s);
  }
  // ---- weight gradients ---------------------------------------------------------------------------------------
  if (W > 1) {
    FtGemm g;  // dW_hh = sum_{s >= 1} dgates_s^T h_{s-1}: one GEMM over K = P (W - 1)
    g.A = b.dgates + (size_t)P * FT_G, g.a_m = 1, g.a_k = FT_G, g.sA = (long)W * P * FT_G;
    g.B = b.h, g.b_k = FT_H, g.b_n = 1, g.sB = (long)W * P * FT_H;
    g.C = grads_ + off_[1], g.ldc = FT_H, g.sC = dirstride;
    g.M = FT_G, g.N = FT_H, g.K = P * (W - 1), g.batch = 2;
    ft_split(g.K, &g.splits, &g.kchunk);
    g.part = b.gpart;
    launch_ft_gemm(g, "ft_gemm_kernel<dwhh>", s);
  } else {
    ProfScope ps("ft_zero_dwhh", 0.0, 2.0 * FT_G * FT_H * sizeof(float), s);  // window 1: no recurrent step
    for (int dir = 0; dir < 2; ++dir)
      M2S_HIP(hipMemsetAsync(grads_ + off_[1 + 4 * dir], 0, (size_t)FT_G * FT_H * sizeof(float), s));
  }
  for (int dir = 0; dir < 2; ++dir)
    launch_ft_colsum(b.dgates + (size_t)dir * W * P * FT_G, (long)W * P, FT_G, b.cpart, grads_ + off_[2 + 4 * dir],
                     grads_ + off_[3 + 4 * dir], s);
  launch_ft_fold(b.dgates, rowtab, R, P, W, b.dpre, s);
  {
    FtGemm g;  // dW_ih = dpre_rows^T feats, K = rows
    g.A = b.dpre, g.a_m = 1, g.a_k = 2 * FT_G, g.sA = FT_G;
    g.B = feats, g.b_k = FT_IN, g.b_n = 1, g.sB = 0;
    g.C = grads_ + off_[0], g.ldc = FT_IN, g.sC = dirstride;
    g.M = FT_G, g.N = FT_IN, g.K = R, g.batch = 2;
    ft_split(g.K, &g.splits, &g.kchunk);
    g.part = b.gpart;
    launch_ft_gemm(g, "ft_gemm_kernel<dwih>", s);
  }
  // ---- norm, clip, AdamW, step count ---------------------------------------------------------------------------
  const long total = (long)off_[M2S_FT_TENSORS];
  launch_ft_sumsq(grads_, total, b.npart, s);
  launch_ft_norm(b.npart, ft_norm_chunks(total), hyper_, step_, b.mslots, scal_, slots_, out_slots, s);
  launch_ft_adamw(params_, grads_, m_, v_, total, hyper_, scal_, s);
  launch_ft_step_inc(step_, s);
}

void FineTune::grads(float* const* g10, hipStream_t s) {
  M2S_CHECK(g10, "finetune_grads: null argument");
  for (int i = 0; i < M2S_FT_TENSORS; ++i)
    if (g10[i]) M2S_HIP(hipMemcpyAsync(g10[i], grads_ + off_[i], count(i) * sizeof(float), hipMemcpyDeviceToDevice, s));
}

void FineTune::export_state(float* const* p10, float* const* m10, float* const* v10, int64_t* step, hipStream_t s) {
  const float* src[3] = {params_, m_, v_};
  float* const* dst[3] = {p10, m10, v10};
  for (int q = 0; q < 3; ++q)
    for (int i = 0; dst[q] && i < M2S_FT_TENSORS; ++i)
      if (dst[q][i])
        M2S_HIP(hipMemcpyAsync(dst[q][i], src[q] + off_[i], count(i) * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (step) M2S_HIP(hipMemcpyAsync(step, step_, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
}

void FineTune::import_moments(const float* const* m10, const float* const* v10, const int64_t* step, hipStream_t s) {
  M2S_CHECK(m10 && v10 && step, "finetune_import_moments: null argument");
  for (int i = 0; i < M2S_FT_TENSORS; ++i) M2S_CHECK(m10[i] && v10[i], "finetune_import_moments: null tensor");
  for (int i = 0; i < M2S_FT_TENSORS; ++i) {
    M2S_HIP(hipMemcpyAsync(m_ + off_[i], m10[i], count(i) * sizeof(float), hipMemcpyDeviceToDevice, s));
    M2S_HIP(hipMemcpyAsync(v_ + off_[i], v10[i], count(i) * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  M2S_HIP(hipMemcpyAsync(step_, step, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
}

}  // namespace m2s
