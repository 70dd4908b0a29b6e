// extern "C" surface of libm2s (include/m2s.h): argument checks, device guards, and the
// exception -> status-code boundary.  No CPU fallback exists behind any of these entry points.
#include <cstring>
#include <string>

#include "../../include/m2s.h"
#include "cam.hpp"
#include "finetune.hpp"
#include "melspec.hpp"
#include "model.hpp"

struct m2s_acoustic {
  m2s::Acoustic impl;
};
struct m2s_vocoder {
  m2s::Vocoder impl;
};
struct m2s_cam {
  m2s::CamBackbone impl;
};
struct m2s_gradcam {
  m2s::GradCam impl;
  m2s_gradcam(const m2s::StateDict& sd, int device) : impl(sd, device) {}
};
struct m2s_finetune {
  m2s::FineTune impl;
  m2s_finetune(const m2s_tensor* sd, int n, int n_mels, int device) : impl(sd, n, n_mels, device) {}
};
struct m2s_melspec {
  m2s::MelSpec impl;
  m2s_melspec(const m2s_melspec_cfg& c, const float* basis, int device) : impl(c, basis, device) {}
};

extern "C" int m2s_prof_enable_impl(int on);
extern "C" int m2s_prof_collect_impl(m2s_prof_stat* out, int max, int* n_out);
extern "C" int m2s_prof_launches_impl(m2s_prof_launch* out, int max, int* n_out);

namespace {

thread_local std::string g_err;

class DeviceGuard {
 public:
  explicit DeviceGuard(int dev) {
    M2S_HIP(hipGetDevice(&prev_));
    if (prev_ != dev) M2S_HIP(hipSetDevice(dev));
    dev_ = dev;
  }
  ~DeviceGuard() {
    if (prev_ != dev_) (void)hipSetDevice(prev_);
  }

 private:
  int prev_ = 0, dev_ = 0;
};

template <class F>
int guarded(F f) {
  try {
    f();
    return M2S_OK;
  } catch (const m2s::Error& e) {
    g_err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_err = e.what();
    return M2S_E_INTERNAL;
  } catch (...) {
    g_err = "unknown error";
    return M2S_E_INTERNAL;
  }
}

void check_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw m2s::Error(M2S_E_NODEV, "no HIP device visible");
  if (device < 0 || device >= n) throw m2s::Error(M2S_E_NODEV, "device index out of range");
  hipDeviceProp_t p;
  M2S_HIP(hipGetDeviceProperties(&p, device));
  if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
    throw m2s::Error(M2S_E_NODEV, std::string("libm2s is built for gfx950, device is ") + p.gcnArchName);
}

hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }

// a size query: 0 for a null handle, and for arguments the call would reject (m2s_last_error says why)
template <class F>
size_t size_query(bool handles, F f) {
  size_t r = 0;
  if (handles) guarded([&] { r = f(); });
  return r;
}

// an earlier launch of this engine hit a BiLSTM barrier timeout (its outputs hold NaN): fail loudly
void no_pending_error(m2s::Acoustic& a) {
  const unsigned e = a.take_async_error();
  if (e == m2s::M2S_ASYNC_WS)
    throw m2s::Error(M2S_E_INTERNAL, "a previous CNN launch timed out at an LDS flag-ring wait (ir_ws / se_ws "
                                     "producer-consumer hand-off); the affected outputs were poisoned with NaN");
  if (e != 0)
    throw m2s::Error(M2S_E_INTERNAL, "a previous BiLSTM launch timed out at its grid barrier (workgroups not "
                                     "co-resident?); its outputs were poisoned with NaN");
}

}  // namespace

extern "C" {

int m2s_abi_version(void) { return M2S_ABI_VERSION; }
const char* m2s_last_error(void) { return g_err.c_str(); }

int m2s_device_check(int device) {
  return guarded([&] { check_device(device); });
}

int m2s_acoustic_create(const m2s_tensor* sd, int n, int n_mels, int rnn_hidden, int dtype, int device,
                        m2s_acoustic** out) {
  return guarded([&] {
    M2S_CHECK(out && (sd || n == 0), "null argument");
    check_device(device);
    DeviceGuard g(device);
    *out = new m2s_acoustic{m2s::Acoustic(m2s::make_state_dict(sd, n), n_mels, rnn_hidden, dtype, device)};
  });
}

void m2s_acoustic_destroy(m2s_acoustic* m) { delete m; }

int m2s_acoustic_set_chunk(m2s_acoustic* m, int frames) {
  return guarded([&] {
    M2S_CHECK(m && frames > 0, "bad argument");
    m->impl.chunk = frames;
  });
}

int m2s_acoustic_status(m2s_acoustic* m) {
  return guarded([&] {
    M2S_CHECK(m, "null argument");
    no_pending_error(m->impl);
  });
}

int m2s_acoustic_set_lstm_spin_limit(m2s_acoustic* m, unsigned polls) {
  return guarded([&] {
    M2S_CHECK(m, "bad argument");
    m->impl.lstm_spin_max_ = polls;
  });
}

int m2s_acoustic_set_ws_spin_limit(m2s_acoustic* m, unsigned polls) {
  return guarded([&] {
    M2S_CHECK(m, "bad argument");
    m->impl.ws_spin_max_ = polls;
  });
}

size_t m2s_acoustic_workspace_bytes(const m2s_acoustic* m, int B, int T, int H, int W) {
  return size_query(m, [&] { return m->impl.workspace_bytes(B, T, H, W); });
}

int m2s_acoustic_forward(m2s_acoustic* m, const float* frames, int B, int T, int H, int W, float* mel_norm, void* ws,
                         size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && frames && mel_norm && ws, "null argument");
    no_pending_error(m->impl);
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    m->impl.forward(frames, B, T, H, W, mel_norm, w, S(stream));
  });
}

int m2s_effnet_forward(m2s_acoustic* m, const float* frames, int N, int H, int W, float* feats, void* ws,
                       size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && frames && feats && ws, "null argument");
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    m->impl.effnet(frames, N, H, W, feats, -1, nullptr, nullptr, w, S(stream));
  });
}

int m2s_effnet_probe(m2s_acoustic* m, const float* frames, int N, int H, int W, int n_blocks, float* out, int* oh,
                     int* ow, int* oc, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && frames && ws, "null argument");
    M2S_CHECK(n_blocks >= 0 && n_blocks <= 28, "n_blocks out of range");
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    int dims[3] = {0, 0, 0};
    m->impl.effnet(frames, N, H, W, nullptr, n_blocks, out, dims, w, S(stream));
    if (oh) *oh = dims[0];
    if (ow) *ow = dims[1];
    if (oc) *oc = dims[2];
  });
}

int m2s_bilstm_summerge(m2s_acoustic* m, const float* feats, int B, int T, float* y, float* mel_norm, void* ws,
                        size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && feats && ws, "null argument");
    no_pending_error(m->impl);
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    m->impl.bilstm(feats, B, T, y, mel_norm, w, S(stream));
  });
}

int m2s_mel_glue(const float* mel_norm, int rows, int n_mels, const float* mean, const float* std, float* mel_db,
                 float* mel_log, void* stream) {
  return guarded([&] {
    M2S_CHECK(mel_norm && mean && std && rows >= 0 && n_mels > 0, "bad argument");
    if (rows == 0) return;
    m2s::launch_mel_glue<float>(mel_norm, rows, n_mels, mean, std, mel_db, mel_log, nullptr, n_mels, S(stream));
  });
}

int m2s_preprocess_frames(const uint8_t* frames, int n, int h, int w, int channels, float* out, void* stream) {
  return guarded([&] {
    M2S_CHECK(frames && out && n >= 0 && h > 0 && w > 0 && (channels == 1 || channels == 3), "bad argument");
    m2s::launch_preprocess(frames, n, h, w, channels, out, S(stream));
  });
}

int m2s_preprocess_frames_resize(const uint8_t* frames, int n, int h, int w, int channels, int out_h, int out_w,
                                 int interp, int norm, float* out, void* stream) {
  return guarded([&] {
    M2S_CHECK(n >= 0 && (n == 0 || (frames && out)), "bad argument");
    m2s::launch_frames(frames, n, h, w, channels, out_h, out_w, interp, norm, out, S(stream));  // checks the limits
  });
}

int m2s_preprocess_frames_masked(const uint8_t* frames, int n, int h, int w, int channels, const float* masks, int n_masks,
                                 int out_h, int out_w, int interp, int norm, float* out, void* stream) {
  return guarded([&] {
    M2S_CHECK(n >= 0 && n_masks >= 1 && (n == 0 || (frames && masks && out)), "bad argument");
    m2s::launch_frames_masked(frames, n, h, w, channels, masks, n_masks, out_h, out_w, interp, norm, out, S(stream));
  });
}

int m2s_occlusion_reduce(const float* mel, int V, int T, int n_mels, const float* band_mask, int n_bands,
                         const float* masks, int h, int w, int normalize, float* score, float* per_frame, float* map,
                         void* stream) {
  return guarded([&] {
    m2s::launch_occlusion_reduce(mel, V, T, n_mels, band_mask, n_bands, masks, h, w, normalize, score, per_frame, map,
                                 S(stream));  // checks the limits
  });
}

int m2s_vocoder_create(const m2s_tensor* sd, int n, const m2s_hifigan_h* h, int dtype, int device, m2s_vocoder** out) {
  return guarded([&] {
    M2S_CHECK(out && h && (sd || n == 0), "null argument");
    check_device(device);
    DeviceGuard g(device);
    *out = new m2s_vocoder{m2s::Vocoder(m2s::make_state_dict(sd, n), *h, dtype, device)};
  });
}

void m2s_vocoder_destroy(m2s_vocoder* v) { delete v; }

size_t m2s_vocoder_workspace_bytes(const m2s_vocoder* v, int B, int T) {
  return size_query(v, [&] { return v->impl.workspace_bytes(B, T); });
}

int m2s_vocoder_forward(m2s_vocoder* v, const float* mel, int mel_layout, int B, int T, float* wav, void* ws,
                        size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(v && mel && wav && ws, "null argument");
    M2S_CHECK(mel_layout == 0 || mel_layout == 1, "mel_layout must be 0 or 1");
    DeviceGuard g(v->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    v->impl.forward(mel, mel_layout, B, T, wav, w, S(stream));
  });
}

int m2s_vocoder_probe(m2s_vocoder* v, const float* mel, int mel_layout, int B, int T, int tap, float* out, int* L, int* C,
                      int* lrelu, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(v && mel && out && ws, "null argument");
    M2S_CHECK(mel_layout == 0 || mel_layout == 1, "mel_layout must be 0 or 1");
    DeviceGuard g(v->impl.device());
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    M2S_HIP(hipStreamIsCapturing(S(stream), &cap));
    if (cap != hipStreamCaptureStatusNone)
      throw m2s::Error(M2S_E_STATE, "the vocoder probe is a test tap: it cannot be captured into a graph");
    m2s::Workspace w(ws, ws_bytes);
    v->impl.probe(mel, mel_layout, B, T, tap, out, L, C, lrelu, w, S(stream));
  });
}

int m2s_vocoder_tap_info(const m2s_vocoder* v, int tap, int T, int* L, int* C, int* lrelu) {
  return guarded([&] {
    M2S_CHECK(v && T > 0, "bad argument");
    int l = 0, c = 0;
    const bool act = v->impl.tap_info(tap, T, &l, &c);
    if (L) *L = l;
    if (C) *C = c;
    if (lrelu) *lrelu = act ? 1 : 0;
  });
}

size_t m2s_pipeline_workspace_bytes(const m2s_acoustic* m, const m2s_vocoder* v, int B, int T, int H, int W) {
  return size_query(m && v, [&] {
    return m2s::Workspace::bytes([&](m2s::Workspace& w) { m2s::pipeline_bufs(w, m->impl, v->impl, B, T, H, W); });
  });
}

int m2s_pipeline_forward(m2s_acoustic* m, m2s_vocoder* v, const float* frames, int B, int T, int H, int W,
                         const float* mean, const float* std, float* mel_norm, float* mel_db, float* mel_log,
                         float* wav, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && v && frames && mean && std && wav && ws, "null argument");
    M2S_CHECK(m->impl.device() == v->impl.device(), "acoustic model and vocoder on different devices");
    M2S_CHECK(m->impl.n_mels() == v->impl.num_mels(), "n_mels mismatch between acoustic model and vocoder");
    no_pending_error(m->impl);
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    const m2s::PipelineBufs b = m2s::pipeline_bufs(w, m->impl, v->impl, B, T, H, W);
    // acoustic scratch is dead once mel_norm is written; the vocoder reuses it
    m2s::Workspace aw(b.rest, b.rest_bytes), vw(b.rest, b.rest_bytes);
    m->impl.forward(frames, B, T, H, W, b.mn, aw, S(stream));
    if (mel_norm)
      M2S_HIP(hipMemcpyAsync(mel_norm, b.mn, (size_t)B * T * m->impl.n_mels() * sizeof(float), hipMemcpyDeviceToDevice,
                             S(stream)));
    v->impl.forward_from_norm(b.mn, mean, std, B, T, mel_db, mel_log, b.ln_t, wav, vw, S(stream));
  });
}

size_t m2s_acoustic_ragged_workspace_bytes(const m2s_acoustic* m, const int* lengths, int B, int H, int W) {
  return size_query(m, [&] { return m->impl.ragged_workspace_bytes(lengths, B, H, W); });
}

int m2s_bilstm_summerge_ragged(m2s_acoustic* m, const float* feats, const int* lengths, int B, int rows, float* y,
                               float* mel_norm, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && feats && ws, "null argument");
    no_pending_error(m->impl);
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    m->impl.bilstm_ragged(feats, lengths, B, rows, y, mel_norm, w, S(stream));
  });
}

int m2s_acoustic_forward_ragged(m2s_acoustic* m, const float* frames, const int* lengths, int B, int rows, int H,
                                int W, float* mel_norm, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && frames && mel_norm && ws, "null argument");
    no_pending_error(m->impl);
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    m->impl.forward_ragged(frames, lengths, B, rows, H, W, mel_norm, w, S(stream));
  });
}

size_t m2s_acoustic_windowed_workspace_bytes(const m2s_acoustic* m, const int* lengths, const int* context, int B,
                                             int H, int W, int window, int merge) {
  return size_query(m, [&] { return m->impl.windowed_workspace_bytes(lengths, context, B, H, W, window, merge); });
}

int m2s_bilstm_windowed(m2s_acoustic* m, const float* feats, const int* lengths, const int* context, int B, int rows,
                        int window, int merge, float* y, float* mel_norm, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && feats && ws, "null argument");
    no_pending_error(m->impl);
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    m->impl.bilstm_windowed(feats, lengths, context, B, rows, window, merge, y, mel_norm, w, S(stream));
  });
}

int m2s_acoustic_forward_windowed(m2s_acoustic* m, const float* frames, const int* lengths, const int* context, int B,
                                  int rows, int H, int W, int window, int merge, float* mel_norm, void* ws,
                                  size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && frames && mel_norm && ws, "null argument");
    no_pending_error(m->impl);
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    m->impl.forward_windowed(frames, lengths, context, B, rows, H, W, window, merge, mel_norm, w, S(stream));
  });
}

size_t m2s_acoustic_pairs_workspace_bytes(const m2s_acoustic* m, const int* lengths, int B, int H, int W, int window) {
  return size_query(m, [&] { return m->impl.pairs_workspace_bytes(lengths, B, H, W, window); });
}

int m2s_bilstm_pairs(m2s_acoustic* m, const float* feats, const int* lengths, int B, int rows, int window, float* y,
                     float* mel_norm, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && feats && ws, "null argument");
    no_pending_error(m->impl);
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    m->impl.bilstm_pairs(feats, lengths, B, rows, window, y, mel_norm, w, S(stream));
  });
}

int m2s_acoustic_forward_pairs(m2s_acoustic* m, const float* frames, const int* lengths, int B, int rows, int H, int W,
                               int window, float* mel_norm, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && frames && mel_norm && ws, "null argument");
    no_pending_error(m->impl);
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    m->impl.forward_pairs(frames, lengths, B, rows, H, W, window, mel_norm, w, S(stream));
  });
}

size_t m2s_mel_metrics_workspace_bytes(int B) {
  if (B < 1) return 0;
  return m2s::Workspace::bytes([&](m2s::Workspace& w) { w.take<float>((size_t)B * m2s::MET_PART); });
}

int m2s_mel_metrics(const float* pred, const float* target, const float* mask, int B, int T, int M, int group,
                    const float* freq_w, const float* time_w, float delta_coeff, float accel_coeff, float latest_coeff,
                    const int* bands, int n_bands, const float* mean, const float* std_, int n_mfcc, double* acc,
                    float* out, float* per_seq, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(pred && target && freq_w && time_w && ws, "null argument");
    M2S_CHECK(B >= 1 && T >= 1 && M >= 1 && M <= 256, "mel_metrics: B, T >= 1 and 1 <= M <= 256");
    M2S_CHECK(group >= 0, "mel_metrics: group must be >= 0");
    M2S_CHECK(n_bands >= 0 && n_bands <= 8 && (bands || n_bands == 0), "mel_metrics: n_bands outside 0..8 or null bands");
    M2S_CHECK((mean == nullptr) == (std_ == nullptr), "mel_metrics: mean and std go together");
    if (mean) M2S_CHECK(n_mfcc >= 1 && n_mfcc <= M && n_mfcc <= 64, "mel_metrics: n_mfcc outside 1..min(M, 64)");
    m2s::Workspace w(ws, ws_bytes);
    m2s::MelMetricsArgs a{};
    a.part = w.take<float>((size_t)B * m2s::MET_PART);
    a.pred = pred, a.target = target, a.mask = mask;
    a.B = B, a.T = T, a.M = M, a.group = group;
    a.freq_w = freq_w, a.time_w = time_w;
    a.coeff[0] = delta_coeff, a.coeff[1] = accel_coeff, a.coeff[2] = latest_coeff;
    a.n_bands = n_bands;
    for (int i = 0; i < 2 * n_bands; ++i) a.bands[i] = bands[i];
    a.mean = mean, a.sd = std_, a.n_mfcc = mean ? n_mfcc : 0;
    a.acc = acc, a.out = out, a.per_seq = per_seq;
    m2s::launch_mel_metrics(a, S(stream));
  });
}

size_t m2s_vocoder_ragged_workspace_bytes(const m2s_vocoder* v, const int* lengths, int B) {
  return size_query(v, [&] { return v->impl.ragged_workspace_bytes(lengths, B); });
}

int m2s_vocoder_forward_ragged(m2s_vocoder* v, const float* mel, const int* lengths, int B, int rows, float* wav,
                               void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(v && mel && wav && ws, "null argument");
    DeviceGuard g(v->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    v->impl.forward_ragged(mel, lengths, B, rows, wav, w, S(stream));
  });
}

int m2s_vocoder_reach(const m2s_vocoder* v, int* back, int* ahead) {
  return guarded([&] {
    M2S_CHECK(v && back && ahead, "null argument");
    v->impl.reach(back, ahead);
  });
}

int m2s_vocoder_set_chunk_cone(m2s_vocoder* v, int on) {
  return guarded([&] {
    M2S_CHECK(v, "null argument");
    v->impl.chunk_cone_ = on != 0;
  });
}

size_t m2s_vocoder_chunk_workspace_bytes(const m2s_vocoder* v, const int* lengths, const int* context, const int* hold,
                                         int B) {
  return size_query(v, [&] { return v->impl.chunk_workspace_bytes(lengths, context, hold, B); });
}

int m2s_vocoder_forward_chunk(m2s_vocoder* v, const float* mel, const int* lengths, const int* context, const int* hold,
                              int B, int rows, float* wav, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(v && mel && wav && ws, "null argument");
    DeviceGuard g(v->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    v->impl.forward_chunk(mel, lengths, context, hold, B, rows, wav, w, S(stream));
  });
}

size_t m2s_pipeline_ragged_workspace_bytes(const m2s_acoustic* m, const m2s_vocoder* v, const int* lengths, int B,
                                           int H, int W) {
  return size_query(m && v, [&] {
    return m2s::Workspace::bytes(
        [&](m2s::Workspace& w) { m2s::pipeline_ragged_bufs(w, m->impl, v->impl, lengths, B, H, W); });
  });
}

int m2s_pipeline_forward_ragged(m2s_acoustic* m, m2s_vocoder* v, const float* frames, const int* lengths, int B,
                                int rows, int H, int W, const float* mean, const float* std, float* mel_norm,
                                float* mel_db, float* mel_log, float* wav, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && v && frames && mean && std && wav && ws, "null argument");
    M2S_CHECK(m->impl.device() == v->impl.device(), "acoustic model and vocoder on different devices");
    M2S_CHECK(m->impl.n_mels() == v->impl.num_mels(), "n_mels mismatch between acoustic model and vocoder");
    no_pending_error(m->impl);
    m2s::ragged_dims(lengths, B, rows);
    DeviceGuard g(m->impl.device());
    m2s::Workspace w(ws, ws_bytes);
    const m2s::PipelineBufs b = m2s::pipeline_ragged_bufs(w, m->impl, v->impl, lengths, B, H, W);
    // the head writes the caller's mel_norm directly where there is one (packed rows: no internal layout)
    float* mn = mel_norm ? mel_norm : b.mn;
    // acoustic scratch is dead once mel_norm is written; the vocoder reuses it
    m2s::Workspace aw(b.rest, b.rest_bytes), vw(b.rest, b.rest_bytes);
    m->impl.forward_ragged(frames, lengths, B, rows, H, W, mn, aw, S(stream));
    v->impl.forward_from_norm_ragged(mn, mean, std, lengths, B, rows, mel_db, mel_log, wav, vw, S(stream));
  });
}

int m2s_cam_create(const m2s_tensor* sd, int n, int device, m2s_cam** out) {
  return guarded([&] {
    M2S_CHECK(out && (sd || n == 0), "null argument");
    check_device(device);
    DeviceGuard g(device);
    *out = new m2s_cam{m2s::CamBackbone(m2s::make_state_dict(sd, n), device)};
  });
}

void m2s_cam_destroy(m2s_cam* c) { delete c; }

int m2s_cam_bn_layers(const m2s_cam* c) { return c ? c->impl.bn_layers() : 0; }

int m2s_cam_bn_channels(const m2s_cam* c, int layer) {
  return c && layer >= 0 && layer < c->impl.bn_layers() ? c->impl.bn_channels(layer) : 0;
}

size_t m2s_cam_workspace_bytes(const m2s_cam* c, int N, int H, int W) {
  return size_query(c, [&] { return c->impl.workspace_bytes(N, H, W); });
}

int m2s_cam_backbone(m2s_cam* c, const float* frames, int N, int H, int W, float* const* taps, float* bn_stats,
                     void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(c && frames && taps && bn_stats && ws, "null argument");
    DeviceGuard g(c->impl.device());
    c->impl.forward(frames, N, H, W, taps, bn_stats, ws, ws_bytes, S(stream));
  });
}

size_t m2s_bilstm_train_workspace_bytes(int B, int T, int C, int H) {
  return size_query(true, [&] { return m2s::bilstm_train_workspace_bytes(B, T, C, H); });
}

int m2s_bilstm_train_forward(const float* x, int B, int T, int C, int H, const float* const* w, float* y,
                             float* gates, float* cells, float* hid, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(x && w && y && gates && cells && hid && ws, "null argument");
    for (int i = 0; i < 8; ++i) M2S_CHECK(w[i], "null LSTM weight");
    const float* wih[2] = {w[0], w[4]};
    const float* whh[2] = {w[1], w[5]};
    const float* bih[2] = {w[2], w[6]};
    const float* bhh[2] = {w[3], w[7]};
    m2s::bilstm_train_forward(x, B, T, C, H, wih, whh, bih, bhh, y, gates, cells, hid, ws, ws_bytes, S(stream));
  });
}

int m2s_bilstm_train_backward(const float* x, const float* dy, int B, int T, int C, int H, const float* const* w,
                              const float* gates, const float* cells, const float* hid, float* dx, float* const* grads,
                              void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(x && dy && w && gates && cells && hid && ws, "null argument");
    const float* wih[2] = {w[0], w[4]};
    const float* whh[2] = {w[1], w[5]};
    M2S_CHECK(wih[0] && wih[1] && whh[0] && whh[1], "null LSTM weight");
    float* dwih[2] = {grads ? grads[0] : nullptr, grads ? grads[3] : nullptr};
    float* dwhh[2] = {grads ? grads[1] : nullptr, grads ? grads[4] : nullptr};
    float* db[2] = {grads ? grads[2] : nullptr, grads ? grads[5] : nullptr};
    m2s::bilstm_train_backward(x, dy, B, T, C, H, wih, whh, gates, cells, hid, dx, dwih, dwhh, db, ws, ws_bytes,
                               S(stream));
  });
}

int m2s_gradcam_create(const m2s_tensor* sd, int n, int device, m2s_gradcam** out) {
  return guarded([&] {
    M2S_CHECK(out && (sd || n == 0), "null argument");
    check_device(device);
    DeviceGuard g(device);
    *out = new m2s_gradcam(m2s::make_state_dict(sd, n), device);
  });
}

void m2s_gradcam_destroy(m2s_gradcam* g) {
  if (!g) return;
  guarded([&] {
    DeviceGuard dg(g->impl.device());
    delete g;
  });
}

int m2s_gradcam_n_mels(const m2s_gradcam* g) { return g ? g->impl.n_mels() : 0; }

int m2s_gradcam_bn_stats_floats(const m2s_gradcam* g) { return g ? g->impl.bn_stats_floats() : 0; }

int m2s_gradcam_chunk(void) { return m2s::kGradcamKC; }

size_t m2s_gradcam_workspace_bytes(const m2s_gradcam* g, int T, int H, int W, int n_bands, int n_frames) {
  return size_query(g, [&] { return g->impl.workspace_bytes(T, H, W, n_bands, n_frames); });
}

int m2s_gradcam_forward(m2s_gradcam* g, const float* frames, int T, int H, int W, const float* mean, const float* std_,
                        const float* band_mask, int n_bands, const int* frame_idx, int n_frames, int reduction,
                        float* heat_seq, float* heat_frame, float* pred_norm, float* dpooled, float* bn_stats,
                        void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(g && frames && mean && std_ && band_mask && heat_seq && ws, "null argument");
    DeviceGuard dg(g->impl.device());
    g->impl.forward(frames, T, H, W, mean, std_, band_mask, n_bands, frame_idx, n_frames, reduction, heat_seq,
                    heat_frame, pred_norm, dpooled, bn_stats, ws, ws_bytes, S(stream));
  });
}

int m2s_gradcam_cotangents(const float* pred_norm, int T, int n_mels, const float* mean, const float* std_,
                           const float* band_mask, int n_bands, const int* frame_idx, int n_frames, int reduction,
                           float* dpred, void* stream) {
  return guarded([&] {
    M2S_CHECK(pred_norm && mean && std_ && band_mask && dpred && (frame_idx || n_frames == 0), "null argument");
    M2S_CHECK(T >= 1 && n_mels >= 1 && n_bands >= 1 && n_frames >= 0 && (reduction == 0 || reduction == 1),
              "gradcam_cotangents: bad argument");
    const long K = (long)n_bands * (1 + (long)n_frames);
    M2S_CHECK(K <= 2147483647L / 4, "gradcam_cotangents: too many targets");
    m2s::launch_gradcam_cotangents(pred_norm, mean, std_, band_mask, frame_idx, n_frames, T, n_mels, 0, (int)K,
                                   reduction == 1, dpred, S(stream));
  });
}

size_t m2s_bilstm_train_backward_multi_workspace_bytes(int K, int T, int C, int H) {
  return size_query(true, [&] { return m2s::bilstm_train_backward_multi_workspace_bytes(K, T, C, H); });
}

int m2s_bilstm_train_backward_multi(const float* dy, int K, int T, int C, int H, const float* const* w,
                                    const float* gates, const float* cells, float* dx, void* ws, size_t ws_bytes,
                                    void* stream) {
  return guarded([&] {
    M2S_CHECK(dy && w && gates && cells && dx && ws, "null argument");
    const float* wih[2] = {w[0], w[4]};
    const float* whh[2] = {w[1], w[5]};
    M2S_CHECK(wih[0] && wih[1] && whh[0] && whh[1], "null LSTM weight");
    m2s::bilstm_train_backward_multi(dy, K, T, C, H, wih, whh, gates, cells, dx, ws, ws_bytes, S(stream));
  });
}

int m2s_cam_heatmap(const float* feats, int N, int C, int h, int w, const float* weights, const int* frame, int M,
                    int H, int W, float* out, void* stream) {
  return guarded([&] {
    M2S_CHECK(feats && weights && frame && out && N >= 1 && M >= 0, "bad argument");
    m2s::launch_cam_heatmap(feats, N, C, h, w, weights, 1.f, frame, 0, 0, 0, 0, M, H, W, out, S(stream));
  });
}

int m2s_linear_forward(const float* x, int rows, int in, int out, const float* w, const float* b, float* y,
                       void* stream) {
  return guarded([&] {
    M2S_CHECK(x && w && y && rows >= 0 && in > 0 && out > 0, "bad argument");
    m2s::linear_forward(x, rows, in, out, w, b, y, S(stream));
  });
}

int m2s_linear_backward(const float* dy, const float* x, int rows, int in, int out, const float* w, float* dx,
                        float* dw, float* db, void* stream) {
  return guarded([&] {
    M2S_CHECK(dy && x && w && rows >= 0 && in > 0 && out > 0, "bad argument");
    m2s::linear_backward(dy, x, rows, in, out, w, dx, dw, db, S(stream));
  });
}

int m2s_gap_forward(const float* x, int64_t nc, int p, float* y, void* stream) {
  return guarded([&] {
    M2S_CHECK(x && y && nc >= 0 && p > 0, "bad argument");
    m2s::launch_gap_nchw(x, nc, p, y, S(stream));
  });
}

int m2s_gap_backward(const float* dy, int64_t nc, int p, float* dx, void* stream) {
  return guarded([&] {
    M2S_CHECK(dy && dx && nc >= 0 && p > 0, "bad argument");
    m2s::launch_gap_nchw_bwd(dy, nc, p, dx, S(stream));
  });
}

int m2s_melspec_create(const m2s_melspec_cfg* cfg, const float* mel_basis_host, int device, m2s_melspec** out) {
  return guarded([&] {
    M2S_CHECK(cfg && mel_basis_host && out, "null argument");
    check_device(device);
    DeviceGuard g(device);
    *out = new m2s_melspec(*cfg, mel_basis_host, device);
  });
}

void m2s_melspec_destroy(m2s_melspec* m) {
  if (!m) return;
  guarded([&] {
    DeviceGuard g(m->impl.device());
    delete m;
  });
}

int m2s_melspec_n_mels(const m2s_melspec* m) { return m ? m->impl.n_mels() : 0; }

int m2s_melspec_frames(const m2s_melspec* m, int L) { return m ? m->impl.frames(L) : 0; }

size_t m2s_melspec_workspace_bytes(const m2s_melspec* m, int B, int L) { return m ? m->impl.workspace_bytes(B, L) : 0; }

int m2s_melspec_forward(m2s_melspec* m, const float* wav, int B, int L, float* mel, int layout, void* ws,
                        size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(m && wav && mel && ws, "null argument");
    DeviceGuard g(m->impl.device());
    m->impl.forward(wav, B, L, mel, layout, ws, ws_bytes, S(stream));
  });
}

int m2s_finetune_create(const m2s_tensor* sd, int n, int n_mels, int device, m2s_finetune** out) {
  return guarded([&] {
    M2S_CHECK(out && (sd || n == 0), "null argument");
    check_device(device);
    DeviceGuard g(device);
    *out = new m2s_finetune(sd, n, n_mels, device);
  });
}

void m2s_finetune_destroy(m2s_finetune* ft) {
  if (!ft) return;
  guarded([&] {
    DeviceGuard g(ft->impl.device());
    delete ft;
  });
}

int m2s_finetune_n_mels(const m2s_finetune* ft) { return ft ? ft->impl.n_mels() : 0; }

int m2s_finetune_set_hyper(m2s_finetune* ft, const m2s_finetune_hyper* h, const float* freq_w, const float* time_w,
                           int window, void* stream) {
  return guarded([&] {
    M2S_CHECK(ft && h, "null argument");
    DeviceGuard g(ft->impl.device());
    ft->impl.set_hyper(*h, freq_w, time_w, window, S(stream));
  });
}

size_t m2s_finetune_workspace_bytes(const m2s_finetune* ft, const int* lengths, int B, int window) {
  return size_query(ft, [&] { return ft->impl.workspace_bytes(lengths, B, window); });
}

int m2s_finetune_step(m2s_finetune* ft, const float* feats, const float* target, const float* mask, const int* lengths,
                      int B, int rows, int window, float* out_slots, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(ft && feats && target && lengths && ws, "null argument");
    DeviceGuard g(ft->impl.device());
    ft->impl.step(feats, target, mask, lengths, B, rows, window, out_slots, ws, ws_bytes, S(stream));
  });
}

int m2s_finetune_forward(m2s_finetune* ft, const float* feats, const int* lengths, int B, int rows, int window,
                         int train, float* mel_norm, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    M2S_CHECK(ft && feats && lengths && mel_norm && ws, "null argument");
    DeviceGuard g(ft->impl.device());
    ft->impl.forward(feats, lengths, B, rows, window, train != 0, mel_norm, ws, ws_bytes, S(stream));
  });
}

int m2s_finetune_grads(m2s_finetune* ft, float* const* grads10, void* stream) {
  return guarded([&] {
    M2S_CHECK(ft, "null argument");
    DeviceGuard g(ft->impl.device());
    ft->impl.grads(grads10, S(stream));
  });
}

int m2s_finetune_export(m2s_finetune* ft, float* const* params10, float* const* m10, float* const* v10, int64_t* step,
                        void* stream) {
  return guarded([&] {
    M2S_CHECK(ft, "null argument");
    DeviceGuard g(ft->impl.device());
    ft->impl.export_state(params10, m10, v10, step, S(stream));
  });
}

int m2s_finetune_import_moments(m2s_finetune* ft, const float* const* m10, const float* const* v10,
                                const int64_t* step, void* stream) {
  return guarded([&] {
    M2S_CHECK(ft, "null argument");
    DeviceGuard g(ft->impl.device());
    ft->impl.import_moments(m10, v10, step, S(stream));
  });
}

int m2s_prof_enable(int on) { return m2s_prof_enable_impl(on); }

int m2s_prof_collect(m2s_prof_stat* out, int max, int* n_out) {
  return guarded([&] { m2s_prof_collect_impl(out, max, n_out); });
}

}  // extern "C"

int m2s_prof_launches(m2s_prof_launch* out, int max, int* n_out) {
  return guarded([&] { m2s_prof_launches_impl(out, max, n_out); });
}
