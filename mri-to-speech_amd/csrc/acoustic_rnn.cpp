// Execution plan of the acoustic model's BiLSTM and mel head, in its four call forms: dense (B, T), ragged
// (packed clips on a zero-padded block), windowed (sliding windows, lstm_window.hip) and pairs (every row of every
// training window), each with its scratch layout, size query and the forward* entry behind the CNN.
#include <algorithm>

#include "plan_util.hpp"
#include "prof.hpp"

namespace m2s {

size_t Acoustic::workspace_bytes(int B, int T, int H, int W) const {
  return Workspace::bytes([&](Workspace& ws) {
    feats_buf(ws, (size_t)B * T);
    effnet_ws(ws, B * T, H, W);
    lstm_bufs(ws, B, T);
  });
}

void Acoustic::project(const float* feats, float* pre, long rows, int kwave, hipStream_t s) {
  ConvArgs a = pw_args(p_.lstm_ih, feats, pre, (int)rows, 1);
  a.kwave = kwave;
  run_conv<float>(a, p_.lstm_ih, sw_.conv, s);
}

void Acoustic::head(const float* h, long rows, bool merged, float* mel_norm, hipStream_t s) {
  const int H = hidden_;
  StageTag tag("head");
  ProfScope ps("mel_head_kernel", 2.0 * rows * H * n_mels_, 4.0 * rows * ((merged ? 1 : 2) * H + n_mels_), s);
  launch_mel_head(h, (int)rows, H, arena_.at<float>(p_.head_wt), arena_.at<float>(p_.head_b), n_mels_, mel_norm, s,
                  merged);
}

void Acoustic::lstm_recurrence(const float* pre, float* hs, float* cst, void* sync, int B, int T, double seq_steps,
                               double rows, hipStream_t s) {
  const int H = hidden_;
  const float* whh = arena_.at<float>(p_.whh);
  const LstmPlan p = lstm_plan(
      {sw_.lstm_persistent, sw_.lstm_mid, sw_.lstm_x3, sw_.lstm_x3g, sw_.lstm_small_b, sw_.lstm_mid_ch}, dtype_, B, H);
  if (p.route == LstmRoute::Step) {
    for (int st = 0; st < T; ++st) {
      ProfScope ps(p.name, 2.0 * 2 * (rows / T) * 4.0 * H * H, 4.0 * 2 * 4 * H * H, s);
      launch_lstm_step(pre, whh, hs, cst, B, T, H, st, s);
    }
    return;
  }
  // algorithmic bytes: W_hh of both directions once, gate pre-activations in, h out
  ProfScope ps(p.name, p.terms * 2 * 4.0 * H * H * seq_steps, 4.0 * 2 * 4 * H * H + 4.0 * rows * (8.0 * H + 2.0 * H), s);
  launch_lstm(p, pre, whh, hs, B, T, H, p.engine_sync ? gsync_ : sync, p.engine_sync ? &gsync_epoch_ : nullptr,
              lstm_spin_max_, err_dev_, s);
}

Acoustic::LstmBufs Acoustic::lstm_bufs(Workspace& ws, int B, int T) const {
  const size_t BT = (size_t)B * T, H = (size_t)hidden_;
  LstmBufs b{};
  b.pre = ws.take<float>(BT * 8 * H);
  b.hs = ws.take<float>(2 * BT * H);
  b.cst = ws.take<float>((size_t)2 * B * H);
  b.sync = ws.take<char>(lstm_sync_bytes(false));
  return b;
}

void Acoustic::bilstm(const float* feats, int B, int T, float* y, float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(B > 0 && T > 0, "bilstm: empty input");
  const int H = hidden_;
  const size_t BT = (size_t)B * T;
  const LstmBufs b = lstm_bufs(ws, B, T);
  float* const hs = b.hs;
  StageTag tag("bilstm");
  // small passes (<= 64 frames): the four waves of a row tile split K (one 30-frame clip: 20 -> 12 us); larger passes
  // keep four row groups a workgroup sharing the weight tile (K split there: the 1920-frame step's projection
  // 0.13 ms slower).  The K summation order therefore differs between the two size classes (fp32 rounding only).
  // (keyed on the projection's row count M: a ragged call of N packed rows switches where a dense one of N does)
  project(feats, b.pre, (long)BT, BT <= 64 ? 1 : 0, s);
  lstm_recurrence(b.pre, hs, b.cst, b.sync, B, T, (double)B * (T - 1), (double)BT, s);
  if (mel_norm) head(hs, (long)BT, false, mel_norm, s);
  if (y) launch_add2(hs, hs + BT * H, y, (long)(BT * H), s);
}

void Acoustic::forward(const float* frames, int B, int T, int H, int W, float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(B > 0 && T > 0, "acoustic: empty input");
  bilstm(cnn_feats(frames, (long)B * T, H, W, ws, s), B, T, nullptr, mel_norm, ws, s);
}

// ------------------------------------------------------------------------------------------
// Ragged batches (ragged.hip, DESIGN.md "Ragged batches")
size_t Acoustic::ragged_workspace_bytes(const int* lengths, int B, int H, int W) const {
  const RaggedDims d = ragged_dims(lengths, B, sum_lengths(lengths, B));
  return Workspace::bytes([&](Workspace& ws) {
    feats_buf(ws, (size_t)d.N);
    effnet_ws(ws, (int)d.N, H, W);
    ragged_lstm_bufs(ws, d);
  });
}

Acoustic::RaggedLstmBufs Acoustic::ragged_lstm_bufs(Workspace& ws, const RaggedDims& d) const {
  RaggedLstmBufs b{};
  b.tab = ws.take<int>((size_t)2 * d.B);
  b.pre_packed = ws.take<float>((size_t)d.N * 8 * hidden_);
  b.d = lstm_bufs(ws, d.B, d.Tmax);
  return b;
}

void Acoustic::bilstm_ragged(const float* feats, const int* lengths, int B, long N, float* y, float* mel_norm,
                             Workspace& ws, hipStream_t s) {
  const RaggedDims d = ragged_dims(lengths, B, N);
  const int H = hidden_, T = d.Tmax;
  const RaggedLstmBufs rb = ragged_lstm_bufs(ws, d);
  int* const tab = rb.tab;
  float *const pre_packed = rb.pre_packed, *const pre = rb.d.pre, *const hs = rb.d.hs;
  rtab_.upload(lengths, B, tab, s);
  StageTag tag("bilstm");
  project(feats, pre_packed, N, N <= 64 ? 1 : 0, s);  // kwave as bilstm: by the projection's row count
  {
    ProfScope ps("ragged_pre_scatter_kernel", 0.0, 2.0 * 4.0 * N * 8.0 * H, s);
    launch_ragged_pre_scatter(pre_packed, tab, B, T, 8 * H, pre, s);
  }
  // the dense kernels, Tmax steps for every clip: zero pre-activation rows keep the reverse direction's state at
  // exactly zero until the clip's last frame, and the forward direction's padded steps are never read
  lstm_recurrence(pre, hs, rb.d.cst, rb.d.sync, B, T, (double)(N - B), (double)N, s);
  StageTag head("head");
  ProfScope ps("ragged_head_gather_kernel", mel_norm ? 2.0 * N * H * n_mels_ : 0.0,
               4.0 * N * (2 * H + (mel_norm ? n_mels_ : 0) + (y ? H : 0)), s);
  launch_ragged_head_gather(hs, tab, B, T, H, arena_.at<float>(p_.head_wt), arena_.at<float>(p_.head_b), n_mels_, y,
                            mel_norm, s);
}

void Acoustic::forward_ragged(const float* frames, const int* lengths, int B, long N, int H, int W, float* mel_norm,
                              Workspace& ws, hipStream_t s) {
  ragged_dims(lengths, B, N);  // before the CNN launches
  ragged_check_stream(s);
  bilstm_ragged(cnn_feats(frames, N, H, W, ws, s), lengths, B, N, nullptr, mel_norm, ws, s);
}

// ------------------------------------------------------------------------------------------
// Windowed inference (lstm_window.hip, DESIGN.md "Windowed acoustic inference")
WindowPlan window_plan(const int* lengths, const int* context, int B, long rows, int window, int merge) {
  M2S_CHECK(window >= 1 && window <= 16, "windowed: window = " + std::to_string(window) + " outside 1..16");
  M2S_CHECK(merge == M2S_WINDOW_LATEST || merge == M2S_WINDOW_MEAN, "windowed: unknown merge " + std::to_string(merge));
  M2S_CHECK(!(context && merge == M2S_WINDOW_MEAN), "windowed: a context needs the latest merge");
  const RaggedDims d = ragged_dims(lengths, B, rows);
  WindowPlan p;
  p.B = B;
  p.W = window;
  p.mean = merge == M2S_WINDOW_MEAN;
  p.N = d.N;
  p.max_len = d.Tmax;
  p.tab.resize((size_t)5 * B);
  long off = 0;
  for (int b = 0; b < B; ++b) {
    const int len = lengths[b], ctx = context ? context[b] : 0;
    M2S_CHECK(ctx >= 0 && ctx <= window - 1 && ctx < len,
              "windowed: context[" + std::to_string(b) + "] = " + std::to_string(ctx) + " outside 0..min(window - 1, " +
                  "length - 1)");
    const int k = std::min(len, window);
    const int nwin = p.mean ? len - k + 1 : len - ctx;
    p.tab[b] = (int)off;
    p.tab[B + b] = len;
    p.tab[2 * B + b] = ctx;
    p.tab[3 * B + b] = (int)p.S;
    p.tab[4 * B + b] = (int)p.R;
    for (int j = 0; j < window; ++j)
      p.active[j] += p.mean ? (k > j ? 2.0 * nwin : 0.0) : (double)std::max(0, len - std::max(ctx, window - 1 - j));
    p.max_windows = std::max(p.max_windows, nwin);
    off += len;
    p.S += nwin;
    p.R += len - ctx;
  }
  return p;
}

Acoustic::WindowBufs Acoustic::window_bufs(Workspace& ws, const WindowPlan& p) const {
  const size_t H = (size_t)hidden_, S = (size_t)p.S, dirs = p.mean ? 2 : 1;
  WindowBufs b;
  b.tab = ws.take<int>((size_t)5 * p.B);
  b.win = ws.take<int2>(S);
  b.pre = ws.take<float>((size_t)p.N * 8 * H);
  if (p.W > 1) {  // the step operands (fp32 rows or split pairs: 4 bytes an element either way) and the cell state
    b.hop[0] = ws.take<float>(dirs * S * H);
    if (p.W > 2) b.hop[1] = ws.take<float>(dirs * S * H);
    b.c = ws.take<float>(dirs * S * H);
  }
  b.hm = ws.take<float>((size_t)(p.pairs ? 1 : 2) * p.R * H);  // pairs: the merged rows, one plane
  if (p.mean) b.hf = ws.take<float>((size_t)2 * p.W * S * H);
  return b;
}

size_t Acoustic::window_query(const WindowPlan& p, int H, int W) const {
  return Workspace::bytes([&](Workspace& ws) {
    if (H != 0 || W != 0) {
      feats_buf(ws, (size_t)p.N);
      effnet_ws(ws, (int)p.N, H, W);
    }
    window_bufs(ws, p);
  });
}

size_t Acoustic::windowed_workspace_bytes(const int* lengths, const int* context, int B, int H, int W, int window,
                                          int merge) const {
  M2S_CHECK(lstm_window_supported(hidden_), "windowed: rnn_hidden must be 640");
  return window_query(window_plan(lengths, context, B, sum_lengths(lengths, B), window, merge), H, W);
}

// the clip table, the projection and the W step launches of a plan: what latest, mean and the pair outputs share
void Acoustic::window_steps(const float* feats, const WindowPlan& p, const WindowBufs& b, hipStream_t s) {
  const int H = hidden_, W = p.W, S = (int)p.S, dirs = p.mean ? 2 : 1, B = p.B;
  const bool split = dtype_ != M2S_DT_F32;
  rtab_.upload_ints(p.tab.data(), p.tab.size(), b.tab, s);
  // the projection, once per FRAME row; one K order for every row count (kwave stays 0: a row's bits must not
  // depend on how many rows the call holds, or a stream's chunking would show)
  project(feats, b.pre, p.N, 0, s);
  {
    ProfScope ps("lstm_window_table_kernel", 0.0, 4.0 * (5.0 * B + 2.0 * S), s);
    launch_lstm_window_table(b.tab, B, W, p.mean, p.max_windows, b.win, s);
  }
  const size_t plane = (size_t)S * H;
  {
    // step 0: three gates of one projected row per (window, unit); latest adds the reverse step of every window
    const double cells = p.active[0] + (p.mean ? 0.0 : (double)S);
    ProfScope ps("lstm_window_step0_kernel", 0.0, 4.0 * cells * H * (3.0 + 2.0), s);
    launch_lstm_window_step0(b.pre, b.win, S, !p.mean, split, b.hop[0], b.c, p.mean ? b.hf : (W == 1 ? b.hm : nullptr),
                             p.mean ? b.hf + (size_t)W * plane : b.hm + (size_t)p.R * H, s);
  }
  const float* wperm = arena_.at<float>(p_.whh_win);
  for (int j = 1; j < W; ++j) {
    const void* hin = b.hop[(j - 1) & 1];
    void* hout = j + 1 < W ? b.hop[j & 1] : nullptr;
    float* hf = p.mean ? b.hf + (size_t)j * plane : (j == W - 1 ? b.hm : nullptr);
    // algorithmic work of the VALID window steps: W_hh of the launched directions once, and per cell update the
    // four gathered gates, h in and out, c in and out
    ProfScope ps(split ? "lstm_window_step_kernel<split>" : "lstm_window_step_kernel<f32>",
                 (split ? 3.0 : 2.0) * 4.0 * H * H * p.active[j], 4.0 * dirs * 4 * H * H + 4.0 * p.active[j] * H * 8.0, s);
    launch_lstm_window_step(b.pre, wperm, b.win, S, j, dirs, split, hin, hout, b.c, hf, (long)((size_t)W * plane), s);
  }
}

void Acoustic::bilstm_windowed(const float* feats, const int* lengths, const int* context, int B, long N, int window,
                               int merge, float* y, float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(lstm_window_supported(hidden_), "windowed: rnn_hidden must be 640");
  const WindowPlan p = window_plan(lengths, context, B, N, window, merge);
  ragged_check_stream(s);
  const int H = hidden_, W = p.W, S = (int)p.S;
  const WindowBufs b = window_bufs(ws, p);
  StageTag tag("bilstm");
  window_steps(feats, p, b, s);
  if (p.mean) {
    double contrib = 0.0;  // (window, step, direction) rows read: every valid one once
    for (int j = 0; j < W; ++j) contrib += p.active[j];
    ProfScope ps("lstm_window_mean_kernel", contrib * H, 4.0 * H * (contrib + 2.0 * p.N), s);
    launch_lstm_window_mean(b.hf, b.tab, B, W, S, p.N, p.max_len, b.hm, s);
  }
  if (mel_norm) head(b.hm, p.R, false, mel_norm, s);
  if (y) launch_add2(b.hm, b.hm + (size_t)p.R * H, y, (long)((size_t)p.R * H), s);
}

void Acoustic::forward_windowed(const float* frames, const int* lengths, const int* context, int B, long N, int H,
                                int W, int window, int merge, float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(lstm_window_supported(hidden_), "windowed: rnn_hidden must be 640");
  window_plan(lengths, context, B, N, window, merge);  // before the CNN launches
  ragged_check_stream(s);
  bilstm_windowed(cnn_feats(frames, N, H, W, ws, s), lengths, context, B, N, window, merge, nullptr, mel_norm, ws, s);
}

// ------------------------------------------------------------------------------------------
// Pair outputs: every row of every training window (m2s.h "pair outputs")
WindowPlan pairs_plan(const int* lengths, int B, long rows, int window) {
  WindowPlan p = window_plan(lengths, nullptr, B, rows, window, M2S_WINDOW_MEAN);
  for (int b = 0; b < B; ++b)
    M2S_CHECK(lengths[b] >= window, "pairs: lengths[" + std::to_string(b) + "] = " + std::to_string(lengths[b]) +
                                        " is shorter than the window of " + std::to_string(window) +
                                        " (the reference skips such clips: leave them out)");
  M2S_CHECK((double)p.S * window <= 2147483647.0, "pairs: P x window out of range");
  p.pairs = true;
  p.R = p.S * window;
  return p;
}

size_t Acoustic::pairs_workspace_bytes(const int* lengths, int B, int H, int W, int window) const {
  M2S_CHECK(lstm_window_supported(hidden_), "pairs: rnn_hidden must be 640");
  return window_query(pairs_plan(lengths, B, sum_lengths(lengths, B), window), H, W);
}

void Acoustic::bilstm_pairs(const float* feats, const int* lengths, int B, long N, int window, float* y,
                            float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(lstm_window_supported(hidden_), "pairs: rnn_hidden must be 640");
  const WindowPlan p = pairs_plan(lengths, B, N, window);
  ragged_check_stream(s);
  const int H = hidden_, W = p.W, S = (int)p.S;
  const WindowBufs b = window_bufs(ws, p);
  StageTag tag("bilstm");
  window_steps(feats, p, b, s);
  {
    // every (window, step, direction) row read once, every merged row written once (twice with y)
    ProfScope ps("lstm_window_pairs_kernel", (double)p.R * H, 4.0 * H * p.R * (y ? 4.0 : 3.0), s);
    launch_lstm_window_pairs(b.hf, W, S, b.hm, y, s);
  }
  if (mel_norm) head(b.hm, p.R, true, mel_norm, s);
}

void Acoustic::forward_pairs(const float* frames, const int* lengths, int B, long N, int H, int W, int window,
                             float* mel_norm, Workspace& ws, hipStream_t s) {
  M2S_CHECK(lstm_window_supported(hidden_), "pairs: rnn_hidden must be 640");
  pairs_plan(lengths, B, N, window);  // before the CNN launches
  ragged_check_stream(s);
  bilstm_pairs(cnn_feats(frames, N, H, W, ws, s), lengths, B, N, window, nullptr, mel_norm, ws, s);
}

}  // namespace m2s
