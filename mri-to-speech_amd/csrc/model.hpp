// Packed models and their execution plans (host side of libm2s).
#pragma once

#include <map>
#include <string>
#include <vector>

#include "../../include/m2s.h"
#include "cnn_route.hpp"
#include "conv_igemm.hpp"
#include "kernels.hpp"
#include "voc_route.hpp"

namespace m2s {

struct HostTensor {
  const float* data = nullptr;
  std::vector<int64_t> shape;
  size_t numel() const {
    size_t n = 1;
    for (auto d : shape) n *= (size_t)d;
    return n;
  }
};
using StateDict = std::map<std::string, HostTensor>;
StateDict make_state_dict(const m2s_tensor* t, int n);

// Host staging of every packed array; one device allocation per model.  The packers (pack_acoustic.cpp,
// pack_vocoder.cpp) fill it with add(); upload() moves it to the device and frees the host copy.
class Arena {
 public:
  size_t add(const void* p, size_t bytes);
  template <class V>
  size_t add_vec(const std::vector<V>& v) {
    return add(v.data(), v.size() * sizeof(V));
  }
  void upload(int device);
  void* ptr(size_t off) const { return static_cast<char*>(dev_) + off; }
  template <class T>
  const T* at(size_t off) const {  // ptr(off) as the packed array's element type
    return static_cast<const T*>(ptr(off));
  }
  size_t bytes() const { return bytes_; }                  // staged so far (kept across upload)
  const uint8_t* host() const { return host_.data(); }     // the staged bytes, until upload()
  ~Arena();

 private:
  std::vector<uint8_t> host_;
  size_t bytes_ = 0;
  void* dev_ = nullptr;
};

// One packed dense conv layer (rows = output channels [x phases], k = tap * cs_in + c).
struct PConv {
  int kind = KIND_GEMM;
  int cin = 0, cout = 0, cs_in = 0, cs_out = 0;
  int ntaps = 1, ks = 1, stride = 1, kp = 0, n_pad = 0, tpc = 1, phases = 1;
  int dil = 1, pad_left = 0;
  int ct_u = 1, ct_pad = 0, ct_k = 1;
  double macs_per_row = 0;  // algorithmic MACs per output position (all phases)
  size_t w_off = 0, b_off = 0, ws_off = 0;
  bool fp8 = false;                // M2S_DT_FP8: e4m3-grid weights (bf16 storage) + per-channel scales
  const void* w = nullptr;
  const float* b = nullptr;
  const float* wscale = nullptr;   // [n_pad] when fp8
  void resolve(const Arena& a) {
    w = a.ptr(w_off);
    b = a.at<float>(b_off);
    wscale = fp8 ? a.at<float>(ws_off) : nullptr;
  }
};

class Workspace {  // bump allocator over a caller-provided device buffer
 public:
  Workspace(void* base, size_t bytes) : base_(static_cast<char*>(base)), cap_(bytes) {}
  template <class T>
  T* take(size_t n) {
    size_t off = (used_ + 255) & ~size_t(255);
    used_ = off + n * sizeof(T);
    if (base_ && used_ > cap_) throw Error(M2S_E_ARG, "workspace too small");
    return base_ ? reinterpret_cast<T*>(base_ + off) : nullptr;
  }
  size_t used() const { return (used_ + 255) & ~size_t(255); }
  // what a layout function takes: the answer of a size query (the pointers it returns are null)
  template <class F>
  static size_t bytes(F&& layout) {
    Workspace ws(nullptr, 0);
    layout(ws);
    return ws.used();
  }

 private:
  char* base_;
  size_t cap_;
  size_t used_ = 0;
};

// Scratch layouts: each entry point's scratch is laid out by one `*_bufs(Workspace&, shape)` function that only takes
// and returns typed pointers; the call runs it on the caller's buffer, the size query through Workspace::bytes.

// f(ActTag<T>{}) with the activation storage type of an engine dtype: bf16_t (bf16, fp8), sp_t (bf16x3) or float
template <typename T>
struct ActTag {
  using type = T;
};
template <class F>
auto dispatch_act(int dtype, F&& f) {
  if (dtype == M2S_DT_BF16 || dtype == M2S_DT_FP8) return f(ActTag<bf16_t>{});
  if (dtype == M2S_DT_BF16X3) return f(ActTag<sp_t>{});
  return f(ActTag<float>{});
}

// Ragged batches (ragged.hip): `lengths[B]` host integers >= 1, N = sum(lengths) packed rows, Tmax = max.
struct RaggedDims {
  int B = 0, Tmax = 0, Tmin = 0;
  long N = 0;
};
// M2S_E_ARG unless B >= 1, every length >= 1, sum(lengths) == rows and B x Tmax rows fit the dense kernels' int
// row counts; no launch happens before it
RaggedDims ragged_dims(const int* lengths, int B, long rows);
// M2S_E_STATE if `s` is capturing: a ragged call stages its clip table per call and cannot be replayed
void ragged_check_stream(hipStream_t s);

// The clip table of a ragged call, [off: B ints | len: B ints], on its way to the device: filled in an engine-owned
// pinned buffer and copied stream-ordered.  The buffer is rewritten only after the previous call's copy has
// completed (an event recorded behind it), so calls on different streams never race on it.  Stream capture of a
// ragged call is not supported: M2S_E_STATE if `s` is capturing.
class RaggedTable {
 public:
  RaggedTable() = default;
  RaggedTable(const RaggedTable&) = delete;
  RaggedTable& operator=(const RaggedTable&) = delete;
  ~RaggedTable();
  void upload(const int* lengths, int B, int* dev, hipStream_t s);  // [off | len] through upload_ints
  // any table of n ints through the staging buffer (the windowed calls' five-column clip table)
  void upload_ints(const int* src, size_t n, int* dev, hipStream_t s);

 private:
  int* host_ = nullptr;
  size_t cap_ = 0;
  hipEvent_t done_ = nullptr;
};

// Windowed calls (lstm_window.hip, DESIGN.md "Windowed acoustic inference"): the validated shape of one call.
// N packed input rows, S windows, R output rows (= N - sum(context)); tab = [off | len | ctx | wbase | obase];
// active[j]: window-directions that run a cell update at global step j (the algorithmic work of that launch).
struct WindowPlan {
  int B = 0, W = 0, max_windows = 0, max_len = 0;
  bool mean = false, pairs = false;  // pairs: the mean route, every row of every window kept unmerged
  long N = 0, S = 0, R = 0;
  std::vector<int> tab;
  double active[16] = {};
};
// M2S_E_ARG, before any launch: window outside 1..16, an unknown merge, a context with mean, a context entry outside
// 0..min(W - 1, len - 1), and the ragged calls' own argument errors
WindowPlan window_plan(const int* lengths, const int* context, int B, long rows, int window, int merge);
// the mean plan of clips that are all at least `window` long (M2S_E_ARG otherwise): S = P pairs, R = P * window rows
WindowPlan pairs_plan(const int* lengths, int B, long rows, int window);

// ---- packed plans: what the packers produce beside the arena bytes (offsets until the engine resolves them) ----
// One block of the tf_efficientnetv2_b2 backbone as pack.hpp's for_each_backbone_block yields it: block `index`
// is rep `rep` of `stage`.
struct BlockDef {
  int index = 0, stage = 0, rep = 0;
  int type = 0;  // 0 cn, 1 er, 2 ir
  int k = 3, stride = 1, cin = 0, cout = 0, mid = 0, rd = 0;
  bool skip = false;
  std::string key() const {  // state-dict prefix
    return "cnn.backbone.blocks." + std::to_string(stage) + "." + std::to_string(rep) + ".";
  }
};
// ... packed for the inference engine
struct Block : BlockDef {
  PConv c1, c2;              // cn: c1 ; er: conv_exp, conv_pwl ; ir: conv_pw, conv_pwl
  size_t dw_w = 0, dw_b = 0;  // ir depthwise, tap-major (9 x cs_mid) and (cs_mid), fp32
  size_t dw_w2 = 0;           // bf16 engines: the same taps as bf16 in the channel's dword half
  PConv se1, se2;             // ir SE: conv_reduce (mid -> rd, SiLU), conv_expand (rd -> mid, sigmoid)
  size_t er_wexp = 0, er_wpwl = 0;  // bf16 er 32 -> 128 -> 32 stride 1: fused-kernel fragment orders
  bool er_frag = false;
  // fp8 engines, er 32 -> 128 -> 32 stride 1 on e4m3 (er8_fused.hip): fragments, per-channel scales
  size_t er8_wexp = 0, er8_sexp = 0, er8_wpwl = 0, er8_spwl = 0;
  bool er8 = false;
  // fp8 engines, er 56 -> 224 -> 56 stride 1 on e4m3 (er8w_fused.hip): stage stream, per-channel scales
  size_t er8w_w = 0, er8w_sexp = 0, er8w_spwl = 0;
  bool er8w = false;
  size_t er_sp_w = 0;  // split fp32 er stride 1: er_sp_fused.hip stage stream
  bool er_sp = false;
  bool ers_sp = false;  // split fp32 er stride 2 (blocks.1.0): er_wexp / er_wpwl in [hi/lo] fragment order
  // fp8 engines, ir conv_pwl: e4m3 bytes [f8_npad][f8_kp] of W / scale, per-channel scales, bias
  size_t f8_w = 0, f8_s = 0, f8_b = 0;
  int f8_kp = 0, f8_npad = 0;
  bool f8_pwl = false;
  // fp8 engines, ir conv_pw (stride 1): e4m3 bytes [round_up(cs_mid, 32)][f8x_kp] of W / scale, scales
  size_t f8x_w = 0, f8x_s = 0;
  int f8x_kp = 0;
  bool f8_pw = false;
};

struct AcousticPlan {
  size_t stem_w = 0, stem_b = 0;
  std::vector<Block> blocks;
  PConv lstm_ih;
  size_t whh = 0, head_wt = 0, head_b = 0;
  size_t whh_win = 0;  // W_hh in lstm_window.hip's row order (pack_lstm_window_whh)
  int max_mid_cs = 0;
};
// pack_acoustic.cpp: BatchNorm folded, every weight array of a `dtype` engine staged in `ar`.  Host code only.
void pack_acoustic(const StateDict& sd, int n_mels, int hidden, int dtype, Arena& ar, AcousticPlan& p);

// One resblock of the HiFi-GAN generator.
struct RB {
  int k = 3;
  std::vector<int> dil;
  std::vector<PConv> c1, c2;  // resblock "1": c1 (dilated) + c2 ; "2": c1 only
  // bf16 resblock "1" at C in {32, 64}: the same weights in the fused kernel's fragment order
  std::vector<size_t> f1_off, f2_off;
  std::vector<const bf16_t*> f1, f2;
  // split resblock "1" at C in {64, 128}: conv1d_halo.hip fragment order
  std::vector<size_t> h1_off, h2_off;
  std::vector<const bf16_t*> h1, h2;
  // fp8 resblock "1" at C in {128, 256}: e4m3 [C][k C] weights, scales, biases (conv1d_f8)
  struct F8 {
    size_t w = 0, s = 0, b = 0;
    const void* wp = nullptr;
    const float* sp = nullptr;
    const float* bp = nullptr;
  };
  std::vector<F8> q1, q2;
  void resolve(const Arena& a) {
    for (auto* cv : {&c1, &c2})
      for (PConv& c : *cv) c.resolve(a);
    auto frags = [&](const std::vector<size_t>& off, std::vector<const bf16_t*>& v) {
      for (size_t o : off) v.push_back(a.at<bf16_t>(o));
    };
    frags(f1_off, f1);
    frags(f2_off, f2);
    frags(h1_off, h1);
    frags(h2_off, h2);
    for (auto* qv : {&q1, &q2})
      for (F8& f : *qv) {
        f.wp = a.ptr(f.w);
        f.sp = a.at<float>(f.s);
        f.bp = a.at<float>(f.b);
      }
  }
};

struct VocoderPlan {
  PConv pre;
  std::vector<PConv> ups;
  std::vector<RB> rbs;
  size_t post_w = 0;
  float post_b = 0.f;
  int post_c = 0, hop = 1;
  // reach in mel rows (interval propagation over the config): of the whole generator, and of what follows level l
  int back = 0, ahead = 0, lvl_back[8] = {}, lvl_ahead[8] = {};
};
// pack_vocoder.cpp: weight norm folded, every weight array staged in `ar`, and the reach.  wants =
// voc_pack_wants(h, dtype, switches) (voc_route.hpp): the extra copies each resblock's convs get.  Host code only.
void pack_vocoder(const StateDict& sd, const m2s_hifigan_h& h, int dtype, const VocPackWants& wants, Arena& ar,
                  VocoderPlan& p);

class Acoustic {
 public:
  Acoustic(const StateDict& sd, int n_mels, int hidden, int dtype, int device);
  ~Acoustic();
  Acoustic(const Acoustic&) = delete;
  Acoustic& operator=(const Acoustic&) = delete;
  // M2S_E_INTERNAL (and clears the flag) if a BiLSTM barrier of an earlier launch timed out
  unsigned take_async_error();
  unsigned lstm_spin_max_ = LSTM_SPIN_MAX;  // fault injection: m2s_acoustic_set_lstm_spin_limit
  unsigned ws_spin_max_ = 1u << 20;        // LDS flag-ring waits of ir_ws / se_ws; m2s_acoustic_set_ws_spin_limit
  AsyncReport ws_report() const {
    AsyncReport r;
    r.spin_max = ws_spin_max_;
    r.err = err_dev_;
    return r;
  }
  int device() const { return device_; }
  int n_mels() const { return n_mels_; }
  int chunk = 1920;  // = m2s.config.CNN_CHUNK (the benched pass size)

  size_t workspace_bytes(int B, int T, int H, int W) const;
  void forward(const float* frames, int B, int T, int H, int W, float* mel_norm, Workspace& ws, hipStream_t s);
  void effnet(const float* frames, int N, int H, int W, float* feats, int stop_after, float* probe, int* probe_dims,
              Workspace& ws, hipStream_t s);
  void bilstm(const float* feats, int B, int T, float* y, float* mel_norm, Workspace& ws, hipStream_t s);
  // Ragged batches: packed feats (N, 208) / frames (N, H, W) of B clips, lengths[B] on the host; packed outputs
  // y (N, hidden), mel_norm (N, n_mels).  The recurrence runs the dense kernels on a zero-padded (B, Tmax) block.
  size_t ragged_workspace_bytes(const int* lengths, int B, int H, int W) const;
  void bilstm_ragged(const float* feats, const int* lengths, int B, long N, float* y, float* mel_norm, Workspace& ws,
                     hipStream_t s);
  void forward_ragged(const float* frames, const int* lengths, int B, long N, int H, int W, float* mel_norm,
                      Workspace& ws, hipStream_t s);
  // Sliding windows of `window` frames over packed clips (m2s.h "windowed inference"): packed feats (N, 208) /
  // frames (N, H, W) -> y (R, hidden), mel_norm (R, n_mels), R = N - sum(context).  H = W = 0 in the query: the
  // BiLSTM part alone (bilstm_windowed's exact size).
  size_t windowed_workspace_bytes(const int* lengths, const int* context, int B, int H, int W, int window,
                                  int merge) const;
  void bilstm_windowed(const float* feats, const int* lengths, const int* context, int B, long N, int window, int merge,
                       float* y, float* mel_norm, Workspace& ws, hipStream_t s);
  void forward_windowed(const float* frames, const int* lengths, const int* context, int B, long N, int H, int W,
                        int window, int merge, float* mel_norm, Workspace& ws, hipStream_t s);
  // Pair outputs (m2s.h "pair outputs"): every row of every full window, y (P, window, hidden) / mel_norm
  // (P, window, n_mels), on the mean route's window table and step launches.
  size_t pairs_workspace_bytes(const int* lengths, int B, int H, int W, int window) const;
  void bilstm_pairs(const float* feats, const int* lengths, int B, long N, int window, float* y, float* mel_norm,
                    Workspace& ws, hipStream_t s);
  void forward_pairs(const float* frames, const int* lengths, int B, long N, int H, int W, int window, float* mel_norm,
                     Workspace& ws, hipStream_t s);

 private:
  struct WindowBufs {
    int* tab = nullptr;
    int2* win = nullptr;
    float *pre = nullptr, *c = nullptr, *hm = nullptr, *hf = nullptr;
    void* hop[2] = {nullptr, nullptr};
  };
  WindowBufs window_bufs(Workspace& ws, const WindowPlan& p) const;
  // the size query of a windowed or pairs plan: with the CNN's scratch in front unless H = W = 0
  size_t window_query(const WindowPlan& p, int H, int W) const;
  void window_steps(const float* feats, const WindowPlan& p, const WindowBufs& b, hipStream_t s);
  template <typename T>
  struct EffBufs {  // one CNN pass of pass_frames(N) frames
    T *A, *B, *M, *M2, *se_mean, *se_hid, *scale;  // ... SE means, hidden (rd <= 64), gates
    float* sums;
    // fp8: e4m3 copies of IR block inputs (the e4m3 expand's operand), written by the previous block's SE GEMM
    // (y8) or converted (the expand reads no byte past cs_in of a row)
    uint8_t* X8[2];
  };
  template <typename T>
  EffBufs<T> effnet_bufs(Workspace& ws, int N, int H, int W) const;
  void effnet_ws(Workspace& ws, int N, int H, int W) const;  // effnet_bufs of the engine's dtype
  float* feats_buf(Workspace& ws, size_t rows) const;         // precedes the CNN in the forward* calls
  // the forward* calls' CNN leg: feats_buf, then the GAP features of N frames in it
  float* cnn_feats(const float* frames, long N, int H, int W, Workspace& ws, hipStream_t s);
  // the BiLSTM input projection (lstm_ih GEMM) of `rows` feature rows; kwave: ConvArgs::kwave, the caller's choice
  void project(const float* feats, float* pre, long rows, int kwave, hipStream_t s);
  // the mel head on `rows` rows of h under stage "head": [fwd | bwd] planes, or merged rows (one plane)
  void head(const float* h, long rows, bool merged, float* mel_norm, hipStream_t s);
  struct LstmBufs {
    float *pre, *hs, *cst;
    void* sync;
  };
  LstmBufs lstm_bufs(Workspace& ws, int B, int T) const;
  struct RaggedLstmBufs {
    int* tab;
    float* pre_packed;
    LstmBufs d;  // the dense set at (B, Tmax)
  };
  RaggedLstmBufs ragged_lstm_bufs(Workspace& ws, const RaggedDims& d) const;
  // One CNN pass at one block: frames n0 .. n0 + nc and the block's record of the pass's route table (cnn_route.hpp:
  // geometry, kernels, e4m3 hand-offs).  A block function reads cur (fp8: and cur8, its e4m3 copy in X8[0] / X8[1],
  // where the record says the block reads one), writes nxt and, where the record says so, an e4m3 copy into next8;
  // the loop then advances them.
  template <typename T>
  struct EffPass {
    EffBufs<T> b;
    hipStream_t s;
    int nc, n0;
    const BlockRoute* r;
    T *cur, *nxt;
    uint8_t *cur8, *next8;
    uint8_t* other8() const { return cur8 == b.X8[0] ? b.X8[1] : b.X8[0]; }  // the X8 buffer cur8 does not hold
  };
  // the recurrence for (B, T), shared by bilstm and bilstm_ragged: the kernel lstm_plan (lstm_route.hpp) chooses,
  // one record, one launch (or a launch per step).  seq_steps / rows: the recurrent steps and (b, t) rows that count
  // as algorithmic work (a ragged call: the valid ones)
  void lstm_recurrence(const float* pre, float* hs, float* cst, void* sync, int B, int T, double seq_steps, double rows,
                       hipStream_t s);
  RaggedTable rtab_;
  template <typename T>
  void effnet_t(const float* frames, int N, int H, int W, float* feats, int stop_after, float* probe, int* probe_dims,
                Workspace& ws, hipStream_t s);
  // block k of a pass, executing p.r: ConvBnAct, EdgeResidual, and InvertedResidual as front half (expand +
  // depthwise + SE mean), SE gates and the gated conv_pwl
  template <typename T>
  void effnet_cn(EffPass<T>& p, size_t k);
  template <typename T>
  void effnet_er(EffPass<T>& p, size_t k);
  template <typename T>
  void effnet_ir_front(EffPass<T>& p, size_t k);
  template <typename T>
  void effnet_ir_se(EffPass<T>& p, size_t k);
  template <typename T>
  void effnet_ir_pwl(EffPass<T>& p, size_t k);
  int pass_frames(int N) const;
  size_t effnet_x8(int H, int W) const;  // fp8 engines: bytes per image of an e4m3 expand-operand buffer
  void effnet_dims(int H, int W, size_t* io_elems, size_t* mid_elems, size_t* se_elems) const;

  int dtype_, device_, n_mels_, hidden_;
  const Switches sw_;  // the M2S_* switches as the environment held them when the engine was created (switches.hpp)
  Arena arena_;
  AcousticPlan p_;
  unsigned* err_host_ = nullptr;  // pinned, host-mapped: set by a one-launch BiLSTM kernel whose hand-off wait timed out
  unsigned* err_dev_ = nullptr;
  // the hand-off buffer of the plans with engine_sync (lstm_route.hpp: lstm_small, lstm_x3g), lstm_sync_bytes(true),
  // and its epoch count: zeroed at creation, on first use, at the tag wrap guard and by every replay of a captured
  // launch, else tags continue from the last call; a capture never lowers the count (lstm_route.hpp lstm_epoch_rule)
  void* gsync_ = nullptr;
  unsigned gsync_epoch_ = 0;
};

class Vocoder {
 public:
  Vocoder(const StateDict& sd, const m2s_hifigan_h& h, int dtype, int device);
  int device() const { return device_; }
  int hop() const { return p_.hop; }
  int num_mels() const { return h_.num_mels; }
  size_t workspace_bytes(int B, int T) const;
  void forward(const float* mel, int layout, int B, int T, float* wav, Workspace& ws, hipStream_t s);
  // The stage tap (m2s_vocoder_probe): the dense call up to tap 0 (conv_pre's output), 2i + 1 (stage i's upsampler
  // output, X) or 2i + 2 (stage i's MRF output, S), then that tensor as stored -> out fp32 (B, L, C) channel-last.
  // *act: the buffer holds lrelu(x) (the route's hand-off flag of its producer); nothing is inverted
  void probe(const float* mel, int layout, int B, int T, int tap, float* out, int* L, int* C, int* act, Workspace& ws,
             hipStream_t s);
  // L, C and that flag of a tap on T-row clips, from the config and the route table alone (M2S_E_ARG for a tap out of range)
  bool tap_info(int tap, int T, int* L, int* C) const;
  // pipeline entry: mel glue (dB, ln-power; run_mri_video_inference.py:227-233) fused with the
  // cast to the channel-last vocoder input (ln_buf: rows x cs(num_mels) x 4 bytes), then the generator.
  void forward_from_norm(const float* mel_norm, const float* mean, const float* std_, int B, int T, float* mel_db,
                         float* mel_log, void* ln_buf, float* wav, Workspace& ws, hipStream_t s);
  // Ragged batches: packed layout-1 mel (N, num_mels) -> packed wav (N * hop); the generator runs on the padded
  // (B, Tmax) block with zeros written where a short clip's consumers look past its end (run_t)
  size_t ragged_workspace_bytes(const int* lengths, int B) const;
  void forward_ragged(const float* mel, const int* lengths, int B, long N, float* wav, Workspace& ws, hipStream_t s);
  // ... from packed mel_norm through the glue (packed mel_db / mel_log, may be null)
  void forward_from_norm_ragged(const float* mel_norm, const float* mean, const float* std_, const int* lengths, int B,
                                long N, float* mel_db, float* mel_log, float* wav, Workspace& ws, hipStream_t s);
  // Streaming (vocoder_chunk.hip, DESIGN.md "Streaming vocoder"): the generator over packed spans of B clips, of
  // which clip b's rows context[b] .. lengths[b] - hold[b] - 1 are emitted: packed wav (out_rows * hop).  Stateless;
  // the rows equal the whole clip's where context >= back or the span starts the clip, and hold >= ahead or it ends it.
  void reach(int* back, int* ahead) const {
    *back = p_.back;
    *ahead = p_.ahead;
  }
  size_t chunk_workspace_bytes(const int* lengths, const int* context, const int* hold, int B) const;
  void forward_chunk(const float* mel, const int* lengths, const int* context, const int* hold, int B, long N,
                     float* wav, Workspace& ws, hipStream_t s);
  // the cone: between stages the chunk call drops the rows no emitted sample depends on
  // (m2s_vocoder_set_chunk_cone, for tests and timing); off: every stage runs on the full spans.  Same contract
  bool chunk_cone_ = true;
  size_t act_elems(int B, int T) const;

 private:
  // tab (ragged calls, with a clip shorter than Tn): the device clip table; the input S of every upsampler and of
  // conv_post then gets the rows its consumer reads past a clip's end zeroed (launch_ragged_tail_mask)
  // cone (chunk calls): after conv_pre (level 0) and after the MRF of stage l - 1 (level l < n_up) the block keeps
  // rows drop[l] .. drop[l] + keep[l] - 1 of every clip (crop_rows_kernel), and the tail masks of that block read
  // the clip lengths at mask[l] + B (null: no clip of the block ends early)
  struct Cone {
    int drop[8], keep[8];
    const int* mask[8];
  };
  struct Probe {  // a probe call's tap and destination; run_t fills in what it copied
    int tap;
    float* out;
    int L, C;
    bool act;
  };
  template <typename T>
  void run_t(const void* mel_nlc, int B, int Tn, float* wav, Workspace& ws, hipStream_t s, const int* tab = nullptr,
             const Cone* cone = nullptr, Probe* probe = nullptr);
  template <typename T>
  struct GenBufs {  // the generator's activation buffers, act_elems(B, T) each
    T *X, *Hb[2], *T1, *S;
    T* E8;                 // fp8: e4m3 outputs of the C = 128 / 256 MRF pairs
    T* Bt[CONV_BATCH][3];  // split: per resblock, c1 output and the pair outputs (ping-pong)
  };
  template <typename T>
  GenBufs<T> gen_bufs(Workspace& ws, int B, int T_) const;
  void gen_ws(Workspace& ws, int B, int T) const;  // gen_bufs of the engine's dtype
  // the channel-last generator input, rows x cs(num_mels) activation elements
  void* mel_in(Workspace& ws, int B, int T) const;
  struct RaggedBufs {  // a ragged or chunk call's prefix: clip table, padded ln-mel, padded wav; then gen_bufs at (B, Tmax)
    int* tab;
    void* ln_buf;
    float* wav_pad;
  };
  // tab_cols: ints per clip of the table (ragged: off, len; chunk: 5 + n_up columns, chunk_plan)
  RaggedBufs ragged_bufs(Workspace& ws, int B, int Tmax, int tab_cols = 2) const;
  // A chunk call, validated (M2S_E_ARG before any launch): the padded block, the rows each level keeps, and the
  // device table [off | len | src | dst | n | len at level 0 | ... | len at level n_up - 1], B ints a column:
  // clip b's emitted rows are rows src[b] .. src[b] + n[b] - 1 of the final block and packed rows dst[b] ...
  struct ChunkPlan {
    RaggedDims d;
    long out_rows = 0;
    bool crop = false, mask = false;  // any level drops rows; a clip ends before its block does
    int drop[8] = {}, keep[8] = {};
    int t_final = 0;  // rows per clip of the block conv_post runs on
    std::vector<int> tab;
  };
  ChunkPlan chunk_plan(const int* lengths, const int* context, const int* hold, int B, long rows) const;
  void ragged_run(const float* x, const float* mean, const float* std_, const int* lengths, int B, long N,
                  float* mel_db, float* mel_log, float* wav, Workspace& ws, hipStream_t s);
  // the MRF of stage i on its route (route_.stages[i], voc_route.hpp): X -> S, L rows a clip
  template <typename T>
  void mrf_stage_batched(int i, const GenBufs<T>& g, int B, int L, hipStream_t s);
  template <typename T>
  void mrf_stage_f8(int i, const GenBufs<T>& g, int B, int L, hipStream_t s);
  template <typename T>
  void mrf_stage_resblocks(int i, const GenBufs<T>& g, int B, int L, hipStream_t s);
  m2s_hifigan_h h_;
  int dtype_, device_;
  const Switches sw_;  // as Acoustic::sw_
  const VocPackWants wants_;  // what pack_vocoder staged beside the conv_gemm rows
  const VocRoute route_;      // every stage's MRF route and hand-offs, planned once (voc_route.hpp)
  Arena arena_;
  VocoderPlan p_;
  RaggedTable rtab_;
};

// The pipeline calls' scratch: mel_norm (rows, n_mels), the dense call's channel-last vocoder input (4 bytes an
// element in every dtype), then `rest` (the larger of the two engines' queries): the acoustic model's, then the vocoder's
struct PipelineBufs {
  float* mn;
  void* ln_t;
  char* rest;
  size_t rest_bytes;
};
PipelineBufs pipeline_bufs(Workspace& ws, const Acoustic& a, const Vocoder& v, int B, int T, int H, int W);
PipelineBufs pipeline_ragged_bufs(Workspace& ws, const Acoustic& a, const Vocoder& v, const int* lengths, int B, int H,
                                  int W);

}  // namespace m2s
