// PyTorch-ROCm custom ops over the libm2s C ABI (include/m2s.h): torch.ops.m2s.*.
//
// The ops take the packed model as an opaque int handle (an m2s_acoustic* / m2s_vocoder* created
// through the C ABI and owned by the Python engine object), allocate their outputs and workspace
// through the torch caching allocator on the CURRENT HIP stream (so concurrent streams get separate,
// stream-ordered workspaces) and launch there.  Fake (meta) kernels for torch.compile / FakeTensor
// tracing live in m2s/ops.py.  Errors: TORCH_CHECK -> RuntimeError with m2s_last_error().
//
// Reference interfaces (mri2speech_code/mri_acoustic_model.py, models.py, scripts/run_mri_video_inference.py):
//   acoustic_forward   OTNLikeCNNBiLSTM.forward (eval)                 mri_acoustic_model.py:116-136
//   effnet_forward     EffNetV2B2Backbone.forward + GlobalAvgPool      mri_acoustic_model.py:15-18,39-48
//   effnet_features    the timm feature maps (Grad-CAM tap)           mri_gradcam_formant.py:155-158
//   bilstm_summerge    BiLSTMSumMerge.forward + head Linear            mri_acoustic_model.py:67-72,135
//   mel_glue           denormalize_mel + dB -> ln-power                run_mri_video_inference.py:160-163,227-233
//   hifigan_forward    Generator.forward                               models.py:113-131
//   pipeline_forward   the no_grad section of main()                   run_mri_video_inference.py:222-242
//   preprocess_frames  _preprocess_frame after the host decode         run_mri_video_inference.py:34-54
//   preprocess_frames_resize  the same with cv2.resize on the device, and the training convention
//                      (INTER_AREA, / 255)                            mri2speech_code/preprocess_rtmri_data.py:99-113
//   preprocess_frames_masked  build_mask's application ahead of the front end, every variant   scripts/mask_rtmri_video.py:96-98
//   occlusion_reduce   the masking experiment's comparison, as scores and a map   docs/rtmri_pipeline_notes.md step 5
//   *_pairs            the model on every training pair of a clip   mri2speech_code/preprocess_rtmri_data.py:198-259,
//                      train_mri_acoustic_model.py:349-384
//   mel_metrics        MaskedMSEMAE, band MAEs, eval_mel's losses and MCD-like   train_mri_acoustic_model.py:57-167,
//                      263-277, mri2speech_code/eval_mel.py:19-82,104-155
//   *_ragged           the same forward passes over clips of different lengths, packed (include/m2s.h)
//   hifigan_forward_chunk  Generator.forward on spans of a stream, emitting the rows that are final (include/m2s.h)
//   cam_backbone       backbone(x) in train() (batch-statistics BN)    mri_gradcam_formant.py:153-160,221-225
//   bilstm_train_*     model.rnn(seq) forward / autograd backward      mri_gradcam_formant.py:162-164,247-248
//   linear_*           model.head(...) forward / autograd backward     mri_gradcam_formant.py:165
//   gradcam            compute_gradcam, all bands and target frames    mri_gradcam_formant.py:128-279,407-426
//   gradcam_cotangents the targets' gradients w.r.t. pred_norm         mri_gradcam_formant.py:230-247,254-266
//   bilstm_train_backward_multi  the LSTM backward of all targets      mri_gradcam_formant.py:247-248,262-266
//   cam_heatmap        _compute_cam_from_grads                         mri_gradcam_formant.py:169-200
//   gap_*              feats.mean(dim=(2,3)) forward / backward        mri_gradcam_formant.py:162
//   mel_spectrogram    mel_spectrogram / compute_mel_db up to the dB map   meldataset.py:57-93,
//                      mri2speech_code/preprocess_rtmri_data.py:121-147
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <tuple>
#include <vector>

#include "../../include/m2s.h"

namespace {

void ok(int rc, const char* what) { TORCH_CHECK(rc == M2S_OK, "libm2s ", what, " failed (", rc, "): ", m2s_last_error()); }

// PyTorch-ROCm exposes HIP devices as DeviceType::CUDA ("masquerading"); torch.cuda.current_stream()
// is this stream
void* S() { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }
using Guard = c10::hip::HIPGuardMasqueradingAsCUDA;

at::Tensor f32_on_device(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a HIP (cuda) tensor; libm2s has no CPU path");
  return t.to(at::kFloat).contiguous();
}

at::Tensor workspace(size_t bytes, const at::Tensor& like) {
  return at::empty({(int64_t)std::max<size_t>(bytes, 256)}, like.options().dtype(at::kByte));
}

m2s_acoustic* A(int64_t h) {
  TORCH_CHECK(h != 0, "null acoustic handle");
  return reinterpret_cast<m2s_acoustic*>(h);
}
m2s_vocoder* V(int64_t h) {
  TORCH_CHECK(h != 0, "null vocoder handle");
  return reinterpret_cast<m2s_vocoder*>(h);
}

// frames (B,T,H,W) -> mel_norm (B,T,n_mels)
at::Tensor acoustic_forward(int64_t h, const at::Tensor& frames, int64_t n_mels) {
  TORCH_CHECK(frames.dim() == 4, "acoustic_forward: frames must be (B,T,H,W)");
  const Guard g(frames.device());
  const at::Tensor x = f32_on_device(frames, "frames");
  const int B = x.size(0), T = x.size(1), H = x.size(2), W = x.size(3);
  at::Tensor out = at::empty({B, T, n_mels}, x.options());
  if (B * T == 0) return out;
  at::Tensor ws = workspace(m2s_acoustic_workspace_bytes(A(h), B, T, H, W), x);
  ok(m2s_acoustic_forward(A(h), x.data_ptr<float>(), B, T, H, W, out.data_ptr<float>(), ws.data_ptr(), ws.numel(), S()),
     "acoustic_forward");
  return out;
}

// frames (N,H,W) -> feats (N,208)
at::Tensor effnet_forward(int64_t h, const at::Tensor& frames) {
  TORCH_CHECK(frames.dim() == 3, "effnet_forward: frames must be (N,H,W)");
  const Guard g(frames.device());
  const at::Tensor x = f32_on_device(frames, "frames");
  const int N = x.size(0), H = x.size(1), W = x.size(2);
  at::Tensor out = at::empty({N, 208}, x.options());
  if (N == 0) return out;
  at::Tensor ws = workspace(m2s_acoustic_workspace_bytes(A(h), N, 1, H, W), x);
  ok(m2s_effnet_forward(A(h), x.data_ptr<float>(), N, H, W, out.data_ptr<float>(), ws.data_ptr(), ws.numel(), S()),
     "effnet_forward");
  return out;
}

// frames (N,H,W) -> feature map after `n_blocks` timm blocks (0 = stem), (N,C,OH,OW)
at::Tensor effnet_features(int64_t h, const at::Tensor& frames, int64_t n_blocks) {
  TORCH_CHECK(frames.dim() == 3, "effnet_features: frames must be (N,H,W)");
  const Guard g(frames.device());
  const at::Tensor x = f32_on_device(frames, "frames");
  const int N = x.size(0), H = x.size(1), W = x.size(2);
  // the stem output (32 channels at H/2 x W/2) is the largest map of the network
  at::Tensor buf = at::empty({(int64_t)N * ((H + 1) / 2) * ((W + 1) / 2) * 32}, x.options());
  at::Tensor ws = workspace(m2s_acoustic_workspace_bytes(A(h), N, 1, H, W), x);
  int oh = 0, ow = 0, oc = 0;
  ok(m2s_effnet_probe(A(h), x.data_ptr<float>(), N, H, W, (int)n_blocks, buf.data_ptr<float>(), &oh, &ow, &oc,
                      ws.data_ptr(), ws.numel(), S()),
     "effnet_features");
  return buf.narrow(0, 0, (int64_t)N * oh * ow * oc).view({N, oh, ow, oc}).permute({0, 3, 1, 2}).contiguous();
}

// feats (B,T,208) -> (y (B,T,hidden) sum-merged BiLSTM output, mel_norm (B,T,n_mels) head output)
std::tuple<at::Tensor, at::Tensor> bilstm_summerge(int64_t h, const at::Tensor& feats, int64_t hidden, int64_t n_mels) {
  TORCH_CHECK(feats.dim() == 3 && feats.size(2) == 208, "bilstm_summerge: feats must be (B,T,208)");
  const Guard g(feats.device());
  const at::Tensor x = f32_on_device(feats, "feats");
  const int B = x.size(0), T = x.size(1);
  at::Tensor y = at::empty({B, T, hidden}, x.options());
  at::Tensor m = at::empty({B, T, n_mels}, x.options());
  if (B * T == 0) return {y, m};
  at::Tensor ws = workspace(m2s_acoustic_workspace_bytes(A(h), B, T, 64, 64), x);
  ok(m2s_bilstm_summerge(A(h), x.data_ptr<float>(), B, T, y.data_ptr<float>(), m.data_ptr<float>(), ws.data_ptr(),
                         ws.numel(), S()),
     "bilstm_summerge");
  return {y, m};
}

// mel_norm (..., n_mels), mean/std (n_mels) -> (mel_db, mel_log), same shape
std::tuple<at::Tensor, at::Tensor> mel_glue(const at::Tensor& mel_norm, const at::Tensor& mean, const at::Tensor& std_) {
  const Guard g(mel_norm.device());
  const at::Tensor x = f32_on_device(mel_norm, "mel_norm");
  const int nm = x.size(-1);
  TORCH_CHECK(mean.numel() == nm && std_.numel() == nm, "mel_glue: mean/std must have n_mels entries");
  const at::Tensor mu = mean.to(x.device(), at::kFloat).contiguous(), sd = std_.to(x.device(), at::kFloat).contiguous();
  at::Tensor db = at::empty_like(x), ln = at::empty_like(x);
  ok(m2s_mel_glue(x.data_ptr<float>(), (int)(x.numel() / nm), nm, mu.data_ptr<float>(), sd.data_ptr<float>(),
                  db.data_ptr<float>(), ln.data_ptr<float>(), S()),
     "mel_glue");
  return {db, ln};
}

// mel (B,num_mels,T) [layout 0] or (B,T,num_mels) [layout 1] -> wav (B,1,T*hop)
at::Tensor hifigan_forward(int64_t v, const at::Tensor& mel, int64_t layout, int64_t hop) {
  TORCH_CHECK(mel.dim() == 3 && (layout == 0 || layout == 1), "hifigan_forward: mel must be 3-D, layout 0 or 1");
  const Guard g(mel.device());
  const at::Tensor x = f32_on_device(mel, "mel");
  const int B = x.size(0), T = layout == 0 ? x.size(2) : x.size(1);
  at::Tensor wav = at::empty({B, 1, (int64_t)T * hop}, x.options());
  if (B * T == 0) return wav;
  at::Tensor ws = workspace(m2s_vocoder_workspace_bytes(V(v), B, T), x);
  ok(m2s_vocoder_forward(V(v), x.data_ptr<float>(), (int)layout, B, T, wav.data_ptr<float>(), ws.data_ptr(), ws.numel(),
                         S()),
     "hifigan_forward");
  return wav;
}

// mel as hifigan_forward -> the tensor stored at `tap` (include/m2s.h m2s_vocoder_probe), (B, channels, T*scale);
// channels and scale are the caller's arithmetic on the config (the fake kernel's shape), checked against the engine's
at::Tensor hifigan_features(int64_t v, const at::Tensor& mel, int64_t layout, int64_t tap, int64_t channels, int64_t scale) {
  TORCH_CHECK(mel.dim() == 3 && (layout == 0 || layout == 1), "hifigan_features: mel must be 3-D, layout 0 or 1");
  const Guard g(mel.device());
  const at::Tensor x = f32_on_device(mel, "mel");
  const int B = x.size(0), T = layout == 0 ? x.size(2) : x.size(1);
  at::Tensor buf = at::empty({B, (int64_t)T * scale, channels}, x.options());
  at::Tensor ws = workspace(m2s_vocoder_workspace_bytes(V(v), B, T), x);
  int L = 0, C = 0;
  // the sizes are the caller's: ask the engine for the tap's before anything is written
  ok(m2s_vocoder_tap_info(V(v), (int)tap, T, &L, &C, nullptr), "hifigan_features");
  TORCH_CHECK(L == (int64_t)T * scale && C == channels, "hifigan_features: tap ", tap, " is (B, ", C, ", ", L,
              "), not (B, ", channels, ", ", (int64_t)T * scale, ")");
  ok(m2s_vocoder_probe(V(v), x.data_ptr<float>(), (int)layout, B, T, (int)tap, buf.data_ptr<float>(), nullptr, nullptr,
                       nullptr, ws.data_ptr(), ws.numel(), S()),
     "hifigan_features");
  return buf.permute({0, 2, 1}).contiguous();
}

// frames (B,T,H,W) -> (mel_norm, mel_db, mel_log (B,T,n_mels), wav (B,T*hop))
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> pipeline_forward(int64_t h, int64_t v, const at::Tensor& frames,
                                                                            const at::Tensor& mean, const at::Tensor& std_,
                                                                            int64_t n_mels, int64_t hop) {
  TORCH_CHECK(frames.dim() == 4, "pipeline_forward: frames must be (B,T,H,W)");
  const Guard g(frames.device());
  const at::Tensor x = f32_on_device(frames, "frames");
  const int B = x.size(0), T = x.size(1), H = x.size(2), W = x.size(3);
  const at::Tensor mu = mean.to(x.device(), at::kFloat).contiguous(), sd = std_.to(x.device(), at::kFloat).contiguous();
  TORCH_CHECK(mu.numel() == n_mels && sd.numel() == n_mels, "pipeline_forward: mean/std must have n_mels entries");
  at::Tensor mn = at::empty({B, T, n_mels}, x.options()), db = at::empty_like(mn), ln = at::empty_like(mn);
  at::Tensor wav = at::empty({B, (int64_t)T * hop}, x.options());
  if (B * T == 0) return {mn, db, ln, wav};
  at::Tensor ws = workspace(m2s_pipeline_workspace_bytes(A(h), V(v), B, T, H, W), x);
  ok(m2s_pipeline_forward(A(h), V(v), x.data_ptr<float>(), B, T, H, W, mu.data_ptr<float>(), sd.data_ptr<float>(),
                          mn.data_ptr<float>(), db.data_ptr<float>(), ln.data_ptr<float>(), wav.data_ptr<float>(),
                          ws.data_ptr(), ws.numel(), S()),
     "pipeline_forward");
  return {mn, db, ln, wav};
}

// Ragged batches (include/m2s.h): packed tensors of N = sum(lengths) rows, clip b at rows off_b .. off_b + len_b - 1.
// The C ABI validates lengths against the row count before any launch.
std::vector<int> host_lengths(at::IntArrayRef lengths, const char* what) {
  std::vector<int> l;
  for (int64_t v : lengths) {
    TORCH_CHECK(v >= INT32_MIN && v <= INT32_MAX, what, ": length out of range");
    l.push_back((int)v);
  }
  return l;
}

// feats (N,208) -> (y (N,hidden), mel_norm (N,n_mels))
std::tuple<at::Tensor, at::Tensor> bilstm_summerge_ragged(int64_t h, const at::Tensor& feats, at::IntArrayRef lengths,
                                                          int64_t hidden, int64_t n_mels) {
  TORCH_CHECK(feats.dim() == 2 && feats.size(1) == 208, "bilstm_summerge_ragged: feats must be packed (N,208)");
  const Guard g(feats.device());
  const at::Tensor x = f32_on_device(feats, "feats");
  const std::vector<int> l = host_lengths(lengths, "bilstm_summerge_ragged");
  const int N = x.size(0), B = (int)l.size();
  at::Tensor y = at::empty({N, hidden}, x.options());
  at::Tensor m = at::empty({N, n_mels}, x.options());
  at::Tensor ws = workspace(m2s_acoustic_ragged_workspace_bytes(A(h), l.data(), B, 64, 64), x);
  ok(m2s_bilstm_summerge_ragged(A(h), x.data_ptr<float>(), l.data(), B, N, y.data_ptr<float>(), m.data_ptr<float>(),
                                ws.data_ptr(), ws.numel(), S()),
     "bilstm_summerge_ragged");
  return {y, m};
}

// frames (N,H,W) -> mel_norm (N,n_mels)
at::Tensor acoustic_forward_ragged(int64_t h, const at::Tensor& frames, at::IntArrayRef lengths, int64_t n_mels) {
  TORCH_CHECK(frames.dim() == 3, "acoustic_forward_ragged: frames must be packed (N,H,W)");
  const Guard g(frames.device());
  const at::Tensor x = f32_on_device(frames, "frames");
  const std::vector<int> l = host_lengths(lengths, "acoustic_forward_ragged");
  const int N = x.size(0), H = x.size(1), W = x.size(2), B = (int)l.size();
  at::Tensor out = at::empty({N, n_mels}, x.options());
  at::Tensor ws = workspace(m2s_acoustic_ragged_workspace_bytes(A(h), l.data(), B, H, W), x);
  ok(m2s_acoustic_forward_ragged(A(h), x.data_ptr<float>(), l.data(), B, N, H, W, out.data_ptr<float>(), ws.data_ptr(),
                                 ws.numel(), S()),
     "acoustic_forward_ragged");
  return out;
}

// Windowed inference (include/m2s.h): sliding windows of `window` frames, merge 0 = latest, 1 = mean; `context`
// empty = none.  Output rows = N - sum(context).
int64_t windowed_out_rows(int64_t N, const std::vector<int>& c) {
  int64_t r = N;
  for (int v : c) r -= v;
  return r < 0 ? 0 : r;
}

// feats (N,208) -> (y (R,hidden), mel_norm (R,n_mels))
std::tuple<at::Tensor, at::Tensor> bilstm_windowed(int64_t h, const at::Tensor& feats, at::IntArrayRef lengths,
                                                   at::IntArrayRef context, int64_t window, int64_t merge,
                                                   int64_t hidden, int64_t n_mels) {
  TORCH_CHECK(feats.dim() == 2 && feats.size(1) == 208, "bilstm_windowed: feats must be packed (N,208)");
  TORCH_CHECK(context.empty() || context.size() == lengths.size(), "bilstm_windowed: one context entry per clip");
  const Guard g(feats.device());
  const at::Tensor x = f32_on_device(feats, "feats");
  const std::vector<int> l = host_lengths(lengths, "bilstm_windowed"), c = host_lengths(context, "bilstm_windowed");
  const int N = x.size(0), B = (int)l.size();
  const int* cp = c.empty() ? nullptr : c.data();
  const int64_t R = windowed_out_rows(N, c);
  at::Tensor y = at::empty({R, hidden}, x.options());
  at::Tensor m = at::empty({R, n_mels}, x.options());
  at::Tensor ws = workspace(m2s_acoustic_windowed_workspace_bytes(A(h), l.data(), cp, B, 0, 0, (int)window, (int)merge), x);
  ok(m2s_bilstm_windowed(A(h), x.data_ptr<float>(), l.data(), cp, B, N, (int)window, (int)merge, y.data_ptr<float>(),
                         m.data_ptr<float>(), ws.data_ptr(), ws.numel(), S()),
     "bilstm_windowed");
  return {y, m};
}

// frames (N,H,W) -> mel_norm (R,n_mels)
at::Tensor acoustic_forward_windowed(int64_t h, const at::Tensor& frames, at::IntArrayRef lengths,
                                     at::IntArrayRef context, int64_t window, int64_t merge, int64_t n_mels) {
  TORCH_CHECK(frames.dim() == 3, "acoustic_forward_windowed: frames must be packed (N,H,W)");
  TORCH_CHECK(context.empty() || context.size() == lengths.size(), "acoustic_forward_windowed: one context entry per clip");
  const Guard g(frames.device());
  const at::Tensor x = f32_on_device(frames, "frames");
  const std::vector<int> l = host_lengths(lengths, "acoustic_forward_windowed"),
                         c = host_lengths(context, "acoustic_forward_windowed");
  const int N = x.size(0), H = x.size(1), W = x.size(2), B = (int)l.size();
  const int* cp = c.empty() ? nullptr : c.data();
  at::Tensor out = at::empty({windowed_out_rows(N, c), n_mels}, x.options());
  at::Tensor ws = workspace(m2s_acoustic_windowed_workspace_bytes(A(h), l.data(), cp, B, H, W, (int)window, (int)merge), x);
  ok(m2s_acoustic_forward_windowed(A(h), x.data_ptr<float>(), l.data(), cp, B, N, H, W, (int)window, (int)merge,
                                   out.data_ptr<float>(), ws.data_ptr(), ws.numel(), S()),
     "acoustic_forward_windowed");
  return out;
}

// Pair outputs (include/m2s.h): every row of every window of `window` frames, P = sum(lengths[b] - window + 1) pairs
int64_t pair_count(const std::vector<int>& l, int64_t window) {
  int64_t p = 0;
  for (int v : l) p += std::max<int64_t>(0, (int64_t)v - window + 1);
  return p;
}

// feats (N,208) -> (y (P,window,hidden), mel_norm (P,window,n_mels))
std::tuple<at::Tensor, at::Tensor> bilstm_pairs(int64_t h, const at::Tensor& feats, at::IntArrayRef lengths,
                                                int64_t window, int64_t hidden, int64_t n_mels) {
  TORCH_CHECK(feats.dim() == 2 && feats.size(1) == 208, "bilstm_pairs: feats must be packed (N,208)");
  const Guard g(feats.device());
  const at::Tensor x = f32_on_device(feats, "feats");
  const std::vector<int> l = host_lengths(lengths, "bilstm_pairs");
  const int N = x.size(0), B = (int)l.size();
  const int64_t P = pair_count(l, window), Wd = std::max<int64_t>(window, 0);
  at::Tensor y = at::empty({P, Wd, hidden}, x.options());
  at::Tensor m = at::empty({P, Wd, n_mels}, x.options());
  at::Tensor ws = workspace(m2s_acoustic_pairs_workspace_bytes(A(h), l.data(), B, 0, 0, (int)window), x);
  ok(m2s_bilstm_pairs(A(h), x.data_ptr<float>(), l.data(), B, N, (int)window, y.data_ptr<float>(), m.data_ptr<float>(),
                      ws.data_ptr(), ws.numel(), S()),
     "bilstm_pairs");
  return {y, m};
}

// frames (N,H,W) -> mel_norm (P,window,n_mels)
at::Tensor acoustic_forward_pairs(int64_t h, const at::Tensor& frames, at::IntArrayRef lengths, int64_t window,
                                  int64_t n_mels) {
  TORCH_CHECK(frames.dim() == 3, "acoustic_forward_pairs: frames must be packed (N,H,W)");
  const Guard g(frames.device());
  const at::Tensor x = f32_on_device(frames, "frames");
  const std::vector<int> l = host_lengths(lengths, "acoustic_forward_pairs");
  const int N = x.size(0), H = x.size(1), W = x.size(2), B = (int)l.size();
  at::Tensor out = at::empty({pair_count(l, window), std::max<int64_t>(window, 0), n_mels}, x.options());
  at::Tensor ws = workspace(m2s_acoustic_pairs_workspace_bytes(A(h), l.data(), B, H, W, (int)window), x);
  ok(m2s_acoustic_forward_pairs(A(h), x.data_ptr<float>(), l.data(), B, N, H, W, (int)window, out.data_ptr<float>(),
                                ws.data_ptr(), ws.numel(), S()),
     "acoustic_forward_pairs");
  return out;
}

// Fused validation metrics (include/m2s.h): pred / target (B,T,M), mask (B,T) or None -> (out (M2S_METRICS_SLOTS)
// fp32 of this call, per_seq (B,3)); acc (M2S_METRICS_SLOTS) float64 is added to in place.  coeffs = delta, accel,
// latest; bands = flat {start, end} pairs; mean / std None: no MCD-like.
std::tuple<at::Tensor, at::Tensor> mel_metrics(const at::Tensor& pred, const at::Tensor& target,
                                               const c10::optional<at::Tensor>& mask, int64_t group,
                                               const at::Tensor& freq_w, const at::Tensor& time_w,
                                               at::ArrayRef<double> coeffs, at::IntArrayRef bands,
                                               const c10::optional<at::Tensor>& mean,
                                               const c10::optional<at::Tensor>& std_, int64_t n_mfcc, at::Tensor acc) {
  TORCH_CHECK(pred.dim() == 3 && pred.sizes() == target.sizes(), "mel_metrics: pred and target must be equal (B,T,M)");
  TORCH_CHECK(coeffs.size() == 3 && bands.size() % 2 == 0, "mel_metrics: three coefficients, {start,end} band pairs");
  TORCH_CHECK(mean.has_value() == std_.has_value(), "mel_metrics: mean and std go together");
  const Guard g(pred.device());
  const at::Tensor p = f32_on_device(pred, "pred"), t = f32_on_device(target, "target");
  const at::Tensor fw = f32_on_device(freq_w, "freq_w"), tw = f32_on_device(time_w, "time_w");
  const int B = p.size(0), T = p.size(1), M = p.size(2);
  TORCH_CHECK(fw.numel() == M && tw.numel() == T, "mel_metrics: freq_w must have M entries and time_w T");
  at::Tensor mk, mu, sd;
  if (mask.has_value()) {
    mk = f32_on_device(*mask, "mask");
    TORCH_CHECK(mk.dim() == 2 && mk.size(0) == B && mk.size(1) == T, "mel_metrics: mask must be (B,T)");
  }
  if (mean.has_value()) {
    mu = f32_on_device(*mean, "mean"), sd = f32_on_device(*std_, "std");
    TORCH_CHECK(mu.numel() == M && sd.numel() == M, "mel_metrics: mean and std must have M entries");
  }
  TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == at::kDouble && acc.is_contiguous() && acc.numel() == M2S_METRICS_SLOTS,
              "mel_metrics: acc must be a contiguous float64 device tensor of ", (int)M2S_METRICS_SLOTS, " entries");
  at::Tensor out = at::empty({M2S_METRICS_SLOTS}, p.options());
  at::Tensor per_seq = at::empty({B, 3}, p.options());
  std::vector<int> bd(bands.begin(), bands.end());
  at::Tensor ws = workspace(m2s_mel_metrics_workspace_bytes(B), p);
  ok(m2s_mel_metrics(p.data_ptr<float>(), t.data_ptr<float>(), mk.defined() ? mk.data_ptr<float>() : nullptr, B, T, M,
                     (int)group, fw.data_ptr<float>(), tw.data_ptr<float>(), (float)coeffs[0], (float)coeffs[1],
                     (float)coeffs[2], bd.data(), (int)(bd.size() / 2), mu.defined() ? mu.data_ptr<float>() : nullptr,
                     sd.defined() ? sd.data_ptr<float>() : nullptr, (int)n_mfcc, acc.data_ptr<double>(),
                     out.data_ptr<float>(), per_seq.data_ptr<float>(), ws.data_ptr(), ws.numel(), S()),
     "mel_metrics");
  return {out, per_seq};
}

// mel (N,num_mels) packed layout 1 -> wav (N*hop)
at::Tensor hifigan_forward_ragged(int64_t v, const at::Tensor& mel, at::IntArrayRef lengths, int64_t hop) {
  TORCH_CHECK(mel.dim() == 2, "hifigan_forward_ragged: mel must be packed (N,num_mels)");
  const Guard g(mel.device());
  const at::Tensor x = f32_on_device(mel, "mel");
  const std::vector<int> l = host_lengths(lengths, "hifigan_forward_ragged");
  const int N = x.size(0), B = (int)l.size();
  at::Tensor wav = at::empty({(int64_t)N * hop}, x.options());
  at::Tensor ws = workspace(m2s_vocoder_ragged_workspace_bytes(V(v), l.data(), B), x);
  ok(m2s_vocoder_forward_ragged(V(v), x.data_ptr<float>(), l.data(), B, N, wav.data_ptr<float>(), ws.data_ptr(),
                                ws.numel(), S()),
     "hifigan_forward_ragged");
  return wav;
}

// Streaming vocoder (include/m2s.h): mel (N,num_mels) packed spans -> wav (R*hop), R = N - sum(context) - sum(hold):
// of clip b, the rows context[b] .. lengths[b] - hold[b] - 1
at::Tensor hifigan_forward_chunk(int64_t v, const at::Tensor& mel, at::IntArrayRef lengths, at::IntArrayRef context,
                                 at::IntArrayRef hold, int64_t hop) {
  TORCH_CHECK(mel.dim() == 2, "hifigan_forward_chunk: mel must be packed (N,num_mels)");
  TORCH_CHECK(context.size() == lengths.size() && hold.size() == lengths.size(),
              "hifigan_forward_chunk: one context and one hold entry per clip");
  const Guard g(mel.device());
  const at::Tensor x = f32_on_device(mel, "mel");
  const std::vector<int> l = host_lengths(lengths, "hifigan_forward_chunk"),
                         c = host_lengths(context, "hifigan_forward_chunk"),
                         hd = host_lengths(hold, "hifigan_forward_chunk");
  const int N = x.size(0), B = (int)l.size();
  at::Tensor wav = at::empty({windowed_out_rows(windowed_out_rows(N, c), hd) * hop}, x.options());
  at::Tensor ws = workspace(m2s_vocoder_chunk_workspace_bytes(V(v), l.data(), c.data(), hd.data(), B), x);
  ok(m2s_vocoder_forward_chunk(V(v), x.data_ptr<float>(), l.data(), c.data(), hd.data(), B, N, wav.data_ptr<float>(),
                               ws.data_ptr(), ws.numel(), S()),
     "hifigan_forward_chunk");
  return wav;
}

// frames (N,H,W) -> (mel_norm, mel_db, mel_log (N,n_mels), wav (N*hop))
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> pipeline_forward_ragged(
    int64_t h, int64_t v, const at::Tensor& frames, at::IntArrayRef lengths, const at::Tensor& mean,
    const at::Tensor& std_, int64_t n_mels, int64_t hop) {
  TORCH_CHECK(frames.dim() == 3, "pipeline_forward_ragged: frames must be packed (N,H,W)");
  const Guard g(frames.device());
  const at::Tensor x = f32_on_device(frames, "frames");
  const std::vector<int> l = host_lengths(lengths, "pipeline_forward_ragged");
  const int N = x.size(0), H = x.size(1), W = x.size(2), B = (int)l.size();
  const at::Tensor mu = mean.to(x.device(), at::kFloat).contiguous(), sd = std_.to(x.device(), at::kFloat).contiguous();
  TORCH_CHECK(mu.numel() == n_mels && sd.numel() == n_mels, "pipeline_forward_ragged: mean/std must have n_mels entries");
  at::Tensor mn = at::empty({N, n_mels}, x.options()), db = at::empty_like(mn), ln = at::empty_like(mn);
  at::Tensor wav = at::empty({(int64_t)N * hop}, x.options());
  at::Tensor ws = workspace(m2s_pipeline_ragged_workspace_bytes(A(h), V(v), l.data(), B, H, W), x);
  ok(m2s_pipeline_forward_ragged(A(h), V(v), x.data_ptr<float>(), l.data(), B, N, H, W, mu.data_ptr<float>(),
                                 sd.data_ptr<float>(), mn.data_ptr<float>(), db.data_ptr<float>(), ln.data_ptr<float>(),
                                 wav.data_ptr<float>(), ws.data_ptr(), ws.numel(), S()),
     "pipeline_forward_ragged");
  return {mn, db, ln, wav};
}

// decoded frames uint8 (T,H,W) grey or (T,H,W,3) BGR -> (T,H,W) fp32 in [0,1]
at::Tensor preprocess_frames(const at::Tensor& frames) {
  TORCH_CHECK(frames.is_cuda() && frames.scalar_type() == at::kByte, "preprocess_frames: uint8 HIP tensor expected");
  TORCH_CHECK(frames.dim() == 3 || (frames.dim() == 4 && frames.size(3) == 3), "preprocess_frames: (T,H,W[,3])");
  const Guard g(frames.device());
  const at::Tensor x = frames.contiguous();
  const int n = x.size(0), hh = x.size(1), ww = x.size(2), ch = x.dim() == 4 ? 3 : 1;
  at::Tensor out = at::empty({n, hh, ww}, x.options().dtype(at::kFloat));
  ok(m2s_preprocess_frames(x.data_ptr<uint8_t>(), n, hh, ww, ch, out.data_ptr<float>(), S()), "preprocess_frames");
  return out;
}

// decoded frames uint8 (T,h,w) grey or (T,h,w,3) BGR at the scanner's size -> (T,out_h,out_w) fp32, resized and
// normalised on the device (interp: m2s_frame_interp, norm: m2s_frame_norm)
at::Tensor preprocess_frames_resize(const at::Tensor& frames, int64_t out_h, int64_t out_w, int64_t interp, int64_t norm) {
  TORCH_CHECK(frames.is_cuda() && frames.scalar_type() == at::kByte, "preprocess_frames_resize: uint8 HIP tensor expected");
  TORCH_CHECK(frames.dim() == 3 || (frames.dim() == 4 && frames.size(3) == 3), "preprocess_frames_resize: (T,h,w[,3])");
  TORCH_CHECK(out_h > 0 && out_w > 0 && out_h <= 65536 && out_w <= 65536, "preprocess_frames_resize: bad output size");
  const Guard g(frames.device());
  const at::Tensor x = frames.contiguous();
  const int n = x.size(0), hh = x.size(1), ww = x.size(2), ch = x.dim() == 4 ? 3 : 1;
  at::Tensor out = at::empty({n, out_h, out_w}, x.options().dtype(at::kFloat));
  ok(m2s_preprocess_frames_resize(x.data_ptr<uint8_t>(), n, hh, ww, ch, (int)out_h, (int)out_w, (int)interp, (int)norm,
                                  out.data_ptr<float>(), S()),
     "preprocess_frames_resize");
  return out;
}

// the same for M masked variants of every frame: masks (M,h,w) fp32 -> (M,T,out_h,out_w); every byte is multiplied
// by its pixel's mask, clipped and truncated before BGR -> grey (scripts/mask_rtmri_video.py:96-98)
at::Tensor preprocess_frames_masked(const at::Tensor& frames, const at::Tensor& masks, int64_t out_h, int64_t out_w,
                                    int64_t interp, int64_t norm) {
  TORCH_CHECK(frames.is_cuda() && frames.scalar_type() == at::kByte, "preprocess_frames_masked: uint8 HIP tensor expected");
  TORCH_CHECK(frames.dim() == 3 || (frames.dim() == 4 && frames.size(3) == 3), "preprocess_frames_masked: (T,h,w[,3])");
  TORCH_CHECK(out_h > 0 && out_w > 0 && out_h <= 65536 && out_w <= 65536, "preprocess_frames_masked: bad output size");
  TORCH_CHECK(masks.is_cuda() && masks.scalar_type() == at::kFloat && masks.dim() == 3 && masks.size(0) >= 1 &&
                  masks.size(1) == frames.size(1) && masks.size(2) == frames.size(2),
              "preprocess_frames_masked: masks must be a fp32 HIP tensor (M,h,w) of the frames' size, M >= 1");
  const Guard g(frames.device());
  const at::Tensor x = frames.contiguous(), mk = masks.contiguous();
  const int n = x.size(0), hh = x.size(1), ww = x.size(2), ch = x.dim() == 4 ? 3 : 1;
  at::Tensor out = at::empty({mk.size(0), n, out_h, out_w}, x.options().dtype(at::kFloat));
  ok(m2s_preprocess_frames_masked(x.data_ptr<uint8_t>(), n, hh, ww, ch, mk.data_ptr<float>(), (int)mk.size(0), (int)out_h,
                                  (int)out_w, (int)interp, (int)norm, out.data_ptr<float>(), S()),
     "preprocess_frames_masked");
  return out;
}

// mel (V,T,n_mels) of one clip's variants (0 = baseline), band_mask (n_bands,n_mels), masks (V-1,h,w) or None ->
// score (V-1,nb), per_frame (V-1,T,nb) [(0,T,nb) unless wanted], map (nb,h,w) [(nb,0,0) without masks]
std::tuple<at::Tensor, at::Tensor, at::Tensor> occlusion_reduce(const at::Tensor& mel_, const at::Tensor& band_mask_,
                                                                const c10::optional<at::Tensor>& masks_, bool normalize,
                                                                bool want_per_frame) {
  TORCH_CHECK(mel_.dim() == 3, "occlusion_reduce: mel must be (V,T,n_mels)");
  TORCH_CHECK(band_mask_.dim() == 2 && band_mask_.size(1) == mel_.size(2), "occlusion_reduce: band_mask must be (n_bands,n_mels)");
  const Guard g(mel_.device());
  const at::Tensor mel = f32_on_device(mel_, "mel"), bm = f32_on_device(band_mask_, "band_mask");
  const int V = mel.size(0), T = mel.size(1), nm = mel.size(2), n_bands = bm.size(0), nb = n_bands + 1;
  const int M = V > 0 ? V - 1 : 0;
  at::Tensor masks;
  int h = 0, w = 0;
  if (masks_.has_value()) {
    masks = f32_on_device(*masks_, "masks");
    TORCH_CHECK(masks.dim() == 3 && masks.size(0) == M, "occlusion_reduce: masks must be (V-1,h,w)");
    h = masks.size(1), w = masks.size(2);
  }
  at::Tensor score = at::empty({M, nb}, mel.options());
  at::Tensor pf = at::empty({want_per_frame ? M : 0, T, nb}, mel.options());
  at::Tensor map = at::empty({nb, h, w}, mel.options());
  ok(m2s_occlusion_reduce(mel.data_ptr<float>(), V, T, nm, n_bands ? bm.data_ptr<float>() : nullptr, n_bands,
                          masks.defined() ? masks.data_ptr<float>() : nullptr, h, w, normalize ? 1 : 0,
                          score.data_ptr<float>(), want_per_frame ? pf.data_ptr<float>() : nullptr,
                          masks.defined() ? map.data_ptr<float>() : nullptr, S()),
     "occlusion_reduce");
  return {score, pf, map};
}

m2s_cam* Cm(int64_t h) {
  TORCH_CHECK(h != 0, "null cam handle");
  return reinterpret_cast<m2s_cam*>(h);
}

std::vector<const float*> f32_ptrs(const std::vector<at::Tensor>& ts, size_t n, const char* what) {
  TORCH_CHECK(ts.size() == n, what, ": expected ", n, " tensors");
  std::vector<const float*> p;
  for (const auto& t : ts) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), what, ": contiguous fp32 HIP tensors");
    p.push_back(t.data_ptr<float>());
  }
  return p;
}

// frames (N,H,W) -> five train-mode feature maps (N,C,OH,OW) + BN batch statistics (flat)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> cam_backbone(int64_t h,
                                                                                                const at::Tensor& frames) {
  TORCH_CHECK(frames.dim() == 3, "cam_backbone: frames must be (N,H,W)");
  const Guard g(frames.device());
  const at::Tensor x = f32_on_device(frames, "frames");
  const int N = x.size(0), H = x.size(1), W = x.size(2);
  TORCH_CHECK(N > 0, "cam_backbone: empty batch");
  static const int ch[5] = {16, 32, 56, 120, 208}, red[5] = {2, 4, 8, 16, 32};
  std::vector<at::Tensor> taps;
  std::vector<float*> tp;
  for (int i = 0; i < 5; ++i) {
    int oh = H, ow = W;
    for (int r = 1; r < red[i]; r *= 2) oh = (oh + 1) / 2, ow = (ow + 1) / 2;
    taps.push_back(at::empty({N, ch[i], oh, ow}, x.options()));
    tp.push_back(taps.back().data_ptr<float>());
  }
  int64_t nst = 0;
  for (int l = 0; l < m2s_cam_bn_layers(Cm(h)); ++l) nst += 2 * m2s_cam_bn_channels(Cm(h), l);
  at::Tensor stats = at::empty({nst}, x.options());
  at::Tensor ws = workspace(m2s_cam_workspace_bytes(Cm(h), N, H, W), x);
  ok(m2s_cam_backbone(Cm(h), x.data_ptr<float>(), N, H, W, tp.data(), stats.data_ptr<float>(), ws.data_ptr(),
                      ws.numel(), S()),
     "cam_backbone");
  return {taps[0], taps[1], taps[2], taps[3], taps[4], stats};
}

// x (B,T,C), w = [w_ih, w_hh, b_ih, b_hh] x (fwd, reverse) -> y (B,T,H), gates (2,B,T,4H), cells, hid (2,B,T,H)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> bilstm_train_forward(const at::Tensor& x_,
                                                                                const std::vector<at::Tensor>& w) {
  TORCH_CHECK(x_.dim() == 3, "bilstm_train_forward: x must be (B,T,C)");
  const Guard g(x_.device());
  const at::Tensor x = f32_on_device(x_, "x");
  std::vector<at::Tensor> wc;
  for (const auto& t : w) wc.push_back(f32_on_device(t, "lstm weight"));
  const auto p = f32_ptrs(wc, 8, "bilstm_train_forward");
  const int B = x.size(0), T = x.size(1), C = x.size(2), Hd = wc[1].size(1);
  TORCH_CHECK(wc[0].size(0) == 4 * Hd && wc[0].size(1) == C && wc[1].size(0) == 4 * Hd, "bilstm_train_forward: weight shapes");
  at::Tensor y = at::empty({B, T, Hd}, x.options());
  at::Tensor gates = at::empty({2, B, T, 4 * Hd}, x.options());
  at::Tensor cells = at::empty({2, B, T, Hd}, x.options()), hid = at::empty({2, B, T, Hd}, x.options());
  if (B * T == 0) return {y, gates, cells, hid};
  at::Tensor ws = workspace(m2s_bilstm_train_workspace_bytes(B, T, C, Hd), x);
  ok(m2s_bilstm_train_forward(x.data_ptr<float>(), B, T, C, Hd, p.data(), y.data_ptr<float>(), gates.data_ptr<float>(),
                              cells.data_ptr<float>(), hid.data_ptr<float>(), ws.data_ptr(), ws.numel(), S()),
     "bilstm_train_forward");
  return {y, gates, cells, hid};
}

// -> dx (B,T,C), [d w_ih, d w_hh, d bias] x (fwd, reverse)
std::tuple<at::Tensor, std::vector<at::Tensor>> bilstm_train_backward(const at::Tensor& dy_, const at::Tensor& x_,
                                                                      const std::vector<at::Tensor>& w,
                                                                      const at::Tensor& gates, const at::Tensor& cells,
                                                                      const at::Tensor& hid) {
  const Guard g(x_.device());
  const at::Tensor x = f32_on_device(x_, "x"), dy = f32_on_device(dy_, "dy");
  std::vector<at::Tensor> wc;
  for (const auto& t : w) wc.push_back(f32_on_device(t, "lstm weight"));
  const auto p = f32_ptrs(wc, 8, "bilstm_train_backward");
  const int B = x.size(0), T = x.size(1), C = x.size(2), Hd = wc[1].size(1);
  TORCH_CHECK(dy.sizes() == at::IntArrayRef({B, T, Hd}), "bilstm_train_backward: dy shape");
  const at::Tensor gs = f32_on_device(gates, "gates"), cs = f32_on_device(cells, "cells"), hs = f32_on_device(hid, "hid");
  at::Tensor dx = at::zeros_like(x);
  std::vector<at::Tensor> grads;
  for (int d = 0; d < 2; ++d) {
    grads.push_back(at::zeros_like(wc[4 * d]));
    grads.push_back(at::zeros_like(wc[4 * d + 1]));
    grads.push_back(at::zeros_like(wc[4 * d + 2]));
  }
  if (B * T == 0) return {dx, grads};
  std::vector<float*> gp;
  for (auto& t : grads) gp.push_back(t.data_ptr<float>());
  at::Tensor ws = workspace(m2s_bilstm_train_workspace_bytes(B, T, C, Hd), x);
  ok(m2s_bilstm_train_backward(x.data_ptr<float>(), dy.data_ptr<float>(), B, T, C, Hd, p.data(), gs.data_ptr<float>(),
                               cs.data_ptr<float>(), hs.data_ptr<float>(), dx.data_ptr<float>(), gp.data(),
                               ws.data_ptr(), ws.numel(), S()),
     "bilstm_train_backward");
  return {dx, grads};
}

// ---- Grad-CAM engine (include/m2s.h "Grad-CAM engine") ---------------------------------------------------
m2s_gradcam* Gc(int64_t h) {
  TORCH_CHECK(h != 0, "null gradcam handle");
  return reinterpret_cast<m2s_gradcam*>(h);
}

at::Tensor frame_table(at::IntArrayRef idx, const at::Tensor& like) {
  const std::vector<int> v = host_lengths(idx, "frame index");
  return at::tensor(v, at::TensorOptions().dtype(at::kInt)).to(like.device());
}

// frames (T,H,W), mean / std (n_mels), band_mask (n_bands,n_mels) 0/1, frame_idx host list, reduction 0 mean / 1 sum
// -> heat_seq (n_bands,T,H,W), heat_frame (n_bands,F,H,W), pred_norm (T,n_mels), dpooled (K,T,208) or (0,T,208),
//    bn_stats (flat)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> gradcam(int64_t h, const at::Tensor& frames,
                                                                               const at::Tensor& mean,
                                                                               const at::Tensor& std_,
                                                                               const at::Tensor& band_mask,
                                                                               at::IntArrayRef frame_idx,
                                                                               int64_t reduction, bool want_dpooled) {
  TORCH_CHECK(frames.dim() == 3, "gradcam: frames must be (T,H,W)");
  TORCH_CHECK(band_mask.dim() == 2, "gradcam: band_mask must be (n_bands,n_mels)");
  const Guard g(frames.device());
  const at::Tensor x = f32_on_device(frames, "frames");
  const at::Tensor mu = f32_on_device(mean, "mean"), sd = f32_on_device(std_, "std");
  const at::Tensor mask = band_mask.to(at::kCPU, at::kFloat).contiguous();  // validated on the host before any launch
  const int T = x.size(0), H = x.size(1), W = x.size(2), nb = mask.size(0), nm = m2s_gradcam_n_mels(Gc(h));
  TORCH_CHECK(T > 0, "gradcam: empty clip");
  TORCH_CHECK(mask.size(1) == nm && mu.numel() == nm && sd.numel() == nm, "gradcam: mean / std / band_mask must have ",
              nm, " mel bins");
  const std::vector<int> fi = host_lengths(frame_idx, "gradcam frame index");
  const int F = (int)fi.size();
  for (int v : fi) TORCH_CHECK_INDEX(v >= 0 && v < T, "gradcam: target frame ", v, " outside [0, ", T, ")");
  const int64_t K = (int64_t)nb * (1 + F);
  at::Tensor heat_seq = at::empty({nb, T, H, W}, x.options()), heat_frame = at::empty({nb, F, H, W}, x.options());
  at::Tensor pred = at::empty({T, nm}, x.options());
  at::Tensor dpooled = at::empty({want_dpooled ? K : 0, T, 208}, x.options());
  at::Tensor stats = at::empty({(int64_t)m2s_gradcam_bn_stats_floats(Gc(h))}, x.options());
  const size_t wsb = m2s_gradcam_workspace_bytes(Gc(h), T, H, W, nb, F);
  TORCH_CHECK(wsb > 0, "libm2s gradcam: ", m2s_last_error());
  at::Tensor ws = workspace(wsb, x);
  ok(m2s_gradcam_forward(Gc(h), x.data_ptr<float>(), T, H, W, mu.data_ptr<float>(), sd.data_ptr<float>(),
                         mask.data_ptr<float>(), nb, fi.data(), F, (int)reduction, heat_seq.data_ptr<float>(),
                         F ? heat_frame.data_ptr<float>() : nullptr, pred.data_ptr<float>(),
                         want_dpooled ? dpooled.data_ptr<float>() : nullptr, stats.data_ptr<float>(), ws.data_ptr(),
                         ws.numel(), S()),
     "gradcam");
  return {heat_seq, heat_frame, pred, dpooled, stats};
}

// pred_norm (T,n_mels), band_mask (n_bands,n_mels) -> dpred (K,T,n_mels)
at::Tensor gradcam_cotangents(const at::Tensor& pred_, const at::Tensor& mean, const at::Tensor& std_,
                              const at::Tensor& band_mask, at::IntArrayRef frame_idx, int64_t reduction) {
  TORCH_CHECK(pred_.dim() == 2 && band_mask.dim() == 2, "gradcam_cotangents: pred_norm (T,n_mels), band_mask (n_bands,n_mels)");
  const Guard g(pred_.device());
  const at::Tensor pred = f32_on_device(pred_, "pred_norm"), mu = f32_on_device(mean, "mean");
  const at::Tensor sd = f32_on_device(std_, "std"), mask = f32_on_device(band_mask, "band_mask");
  const int T = pred.size(0), nm = pred.size(1), nb = mask.size(0), F = (int)frame_idx.size();
  TORCH_CHECK(mask.size(1) == nm && mu.numel() == nm && sd.numel() == nm, "gradcam_cotangents: mel bin counts differ");
  TORCH_CHECK(T > 0 && nb > 0, "gradcam_cotangents: empty input");
  const at::Tensor fi = frame_table(frame_idx, pred);
  at::Tensor out = at::empty({(int64_t)nb * (1 + F), T, nm}, pred.options());
  ok(m2s_gradcam_cotangents(pred.data_ptr<float>(), T, nm, mu.data_ptr<float>(), sd.data_ptr<float>(),
                            mask.data_ptr<float>(), nb, F ? fi.data_ptr<int>() : nullptr, F, (int)reduction,
                            out.data_ptr<float>(), S()),
     "gradcam_cotangents");
  return out;
}

// dy (K,T,H), weights as bilstm_train_forward, gates (2,1,T,4H), cells (2,1,T,H) -> dx (K,T,C)
at::Tensor bilstm_train_backward_multi(const at::Tensor& dy_, const std::vector<at::Tensor>& w, const at::Tensor& gates,
                                       const at::Tensor& cells) {
  TORCH_CHECK(dy_.dim() == 3, "bilstm_train_backward_multi: dy must be (K,T,H)");
  const Guard g(dy_.device());
  const at::Tensor dy = f32_on_device(dy_, "dy");
  std::vector<at::Tensor> wc;
  for (const auto& t : w) wc.push_back(f32_on_device(t, "lstm weight"));
  const auto p = f32_ptrs(wc, 8, "bilstm_train_backward_multi");
  const int K = dy.size(0), T = dy.size(1), Hd = wc[1].size(1), C = wc[0].size(1);
  TORCH_CHECK(dy.size(2) == Hd && wc[0].size(0) == 4 * Hd && wc[1].size(0) == 4 * Hd, "bilstm_train_backward_multi: weight shapes");
  const at::Tensor gs = f32_on_device(gates, "gates"), cs = f32_on_device(cells, "cells");
  TORCH_CHECK(gs.sizes() == at::IntArrayRef({2, 1, T, 4 * Hd}) && cs.sizes() == at::IntArrayRef({2, 1, T, Hd}),
              "bilstm_train_backward_multi: gates (2,1,T,4H) and cells (2,1,T,H) of one sequence");
  at::Tensor dx = at::empty({K, T, C}, dy.options());
  if ((int64_t)K * T == 0) return dx;
  const size_t wsb = m2s_bilstm_train_backward_multi_workspace_bytes(K, T, C, Hd);
  TORCH_CHECK(wsb > 0, "libm2s bilstm_train_backward_multi: ", m2s_last_error());
  at::Tensor ws = workspace(wsb, dy);
  ok(m2s_bilstm_train_backward_multi(dy.data_ptr<float>(), K, T, C, Hd, p.data(), gs.data_ptr<float>(),
                                     cs.data_ptr<float>(), dx.data_ptr<float>(), ws.data_ptr(), ws.numel(), S()),
     "bilstm_train_backward_multi");
  return dx;
}

// feats (N,C,h,w), weights (M,C), frame host list (M) -> heat maps (M,H,W)
at::Tensor cam_heatmap(const at::Tensor& feats_, const at::Tensor& weights_, at::IntArrayRef frame, int64_t H, int64_t W) {
  TORCH_CHECK(feats_.dim() == 4 && weights_.dim() == 2, "cam_heatmap: feats (N,C,h,w), weights (M,C)");
  const Guard g(feats_.device());
  const at::Tensor feats = f32_on_device(feats_, "feats"), wt = f32_on_device(weights_, "weights");
  const int N = feats.size(0), C = feats.size(1), h = feats.size(2), w = feats.size(3), M = wt.size(0);
  TORCH_CHECK(wt.size(1) == C && (int64_t)frame.size() == M, "cam_heatmap: one weight row and one frame index per map");
  TORCH_CHECK(N > 0 && H > 0 && W > 0 && H <= INT32_MAX && W <= INT32_MAX, "cam_heatmap: empty input");
  for (int64_t v : frame) TORCH_CHECK_INDEX(v >= 0 && v < N, "cam_heatmap: frame ", v, " outside [0, ", N, ")");
  at::Tensor out = at::empty({M, H, W}, feats.options());
  if (M == 0) return out;
  const at::Tensor fi = frame_table(frame, feats);
  ok(m2s_cam_heatmap(feats.data_ptr<float>(), N, C, h, w, wt.data_ptr<float>(), fi.data_ptr<int>(), M, (int)H, (int)W,
                     out.data_ptr<float>(), S()),
     "cam_heatmap");
  return out;
}

// x (..., in), w (out, in), b (out) -> y (..., out)
at::Tensor linear_forward(const at::Tensor& x_, const at::Tensor& w_, const c10::optional<at::Tensor>& b_) {
  const Guard g(x_.device());
  const at::Tensor x = f32_on_device(x_, "x"), w = f32_on_device(w_, "weight");
  TORCH_CHECK(w.dim() == 2 && x.size(-1) == w.size(1), "linear_forward: shapes");
  at::Tensor b;
  if (b_.has_value()) b = f32_on_device(*b_, "bias");
  const int in = w.size(1), out = w.size(0), rows = x.numel() / in;
  auto shape = x.sizes().vec();
  shape.back() = out;
  at::Tensor y = at::empty(shape, x.options());
  if (rows == 0) return y;
  ok(m2s_linear_forward(x.data_ptr<float>(), rows, in, out, w.data_ptr<float>(), b.defined() ? b.data_ptr<float>() : nullptr,
                        y.data_ptr<float>(), S()),
     "linear_forward");
  return y;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> linear_backward(const at::Tensor& dy_, const at::Tensor& x_,
                                                               const at::Tensor& w_) {
  const Guard g(x_.device());
  const at::Tensor x = f32_on_device(x_, "x"), w = f32_on_device(w_, "weight"), dy = f32_on_device(dy_, "dy");
  const int in = w.size(1), out = w.size(0), rows = x.numel() / in;
  TORCH_CHECK(dy.numel() == (int64_t)rows * out, "linear_backward: dy shape");
  at::Tensor dx = at::empty_like(x), dw = at::zeros_like(w), db = at::zeros({out}, w.options());
  if (rows == 0) return {dx, dw, db};
  ok(m2s_linear_backward(dy.data_ptr<float>(), x.data_ptr<float>(), rows, in, out, w.data_ptr<float>(),
                         dx.data_ptr<float>(), dw.data_ptr<float>(), db.data_ptr<float>(), S()),
     "linear_backward");
  return {dx, dw, db};
}

// (N,C,H,W) -> (N,C) mean over H,W ; backward (N,C) -> (N,C,H,W)
at::Tensor gap_forward(const at::Tensor& x_) {
  TORCH_CHECK(x_.dim() == 4, "gap_forward: (N,C,H,W)");
  const Guard g(x_.device());
  const at::Tensor x = f32_on_device(x_, "x");
  at::Tensor y = at::empty({x.size(0), x.size(1)}, x.options());
  ok(m2s_gap_forward(x.data_ptr<float>(), x.size(0) * x.size(1), (int)(x.size(2) * x.size(3)), y.data_ptr<float>(), S()),
     "gap_forward");
  return y;
}

at::Tensor gap_backward(const at::Tensor& dy_, int64_t h, int64_t w) {
  TORCH_CHECK(dy_.dim() == 2, "gap_backward: dy (N,C)");
  const Guard g(dy_.device());
  const at::Tensor dy = f32_on_device(dy_, "dy");
  at::Tensor dx = at::empty({dy.size(0), dy.size(1), h, w}, dy.options());
  ok(m2s_gap_backward(dy.data_ptr<float>(), dy.numel(), (int)(h * w), dx.data_ptr<float>(), S()), "gap_backward");
  return dx;
}

// wav (B,L) -> mel (B,n_mels,T) [layout 0] or (B,T,n_mels) [layout 1]; handle = an m2s_melspec*, whose n_mels
// and frame count are asked of the engine itself
at::Tensor mel_spectrogram(int64_t h, const at::Tensor& wav, int64_t layout) {
  TORCH_CHECK(h != 0, "null melspec handle");
  TORCH_CHECK(wav.dim() == 2 && (layout == 0 || layout == 1), "mel_spectrogram: wav must be (B,L), layout 0 or 1");
  m2s_melspec* m = reinterpret_cast<m2s_melspec*>(h);
  const Guard g(wav.device());
  const at::Tensor x = f32_on_device(wav, "wav");
  TORCH_CHECK(x.size(1) <= INT32_MAX && x.size(0) <= INT32_MAX, "mel_spectrogram: wav too large");
  const int B = x.size(0), L = x.size(1);
  const int T = m2s_melspec_frames(m, L), nm = m2s_melspec_n_mels(m);
  TORCH_CHECK(B >= 1 && T >= 1, "mel_spectrogram: B = ", B, ", L = ", L, ": no frame (clip shorter than n_fft, or than the reflect pad)");
  at::Tensor out = layout == 0 ? at::empty({B, nm, T}, x.options()) : at::empty({B, T, nm}, x.options());
  at::Tensor ws = workspace(m2s_melspec_workspace_bytes(m, B, L), x);
  ok(m2s_melspec_forward(m, x.data_ptr<float>(), B, L, out.data_ptr<float>(), (int)layout, ws.data_ptr(), ws.numel(), S()),
     "mel_spectrogram");
  return out;
}

// ---- fine-tuning engine (m2s/finetune.py; handle = HeadTuner.handle) ---------------------------------------------
m2s_finetune* Ft(int64_t h) {
  TORCH_CHECK(h != 0, "null finetune handle");
  return reinterpret_cast<m2s_finetune*>(h);
}

const int64_t kFtRows[M2S_FT_TENSORS] = {2560, 2560, 2560, 2560, 2560, 2560, 2560, 2560, 0, 0};
const int64_t kFtCols[M2S_FT_TENSORS] = {208, 640, 0, 0, 208, 640, 0, 0, 640, 0};
std::vector<at::Tensor> ft_tensors(int64_t h, const at::TensorOptions& opt) {
  const int64_t nm = m2s_finetune_n_mels(Ft(h));
  std::vector<at::Tensor> out;
  for (int i = 0; i < M2S_FT_TENSORS; ++i) {
    const int64_t r = kFtRows[i] ? kFtRows[i] : nm;
    out.push_back(kFtCols[i] ? at::empty({r, kFtCols[i]}, opt) : at::empty({r}, opt));
  }
  return out;
}
std::vector<float*> ft_ptrs(std::vector<at::Tensor>& v) {
  std::vector<float*> p;
  for (auto& t : v) p.push_back(t.data_ptr<float>());
  return p;
}

// feats (rows,208), target (rows,n_mels), mask (rows) or None -> the step's 8 slots (device); no host sync
at::Tensor finetune_step(int64_t h, const at::Tensor& feats, const at::Tensor& target,
                         const c10::optional<at::Tensor>& mask, at::IntArrayRef lengths, int64_t window) {
  TORCH_CHECK(feats.dim() == 2 && feats.size(1) == 208, "finetune_step: feats must be (rows,208)");
  const Guard g(feats.device());
  const at::Tensor x = f32_on_device(feats, "feats"), t = f32_on_device(target, "target");
  const int nm = m2s_finetune_n_mels(Ft(h));
  TORCH_CHECK(t.dim() == 2 && t.size(0) == x.size(0) && t.size(1) == nm, "finetune_step: target must be (rows,n_mels)");
  at::Tensor mk;
  if (mask.has_value() && mask->defined()) {
    mk = f32_on_device(*mask, "mask");
    TORCH_CHECK(mk.dim() == 1 && mk.size(0) == x.size(0), "finetune_step: mask must be (rows)");
  }
  const std::vector<int> len = host_lengths(lengths, "finetune_step lengths");
  const size_t wsb = m2s_finetune_workspace_bytes(Ft(h), len.data(), (int)len.size(), (int)window);
  TORCH_CHECK(wsb > 0, "libm2s finetune_step: ", m2s_last_error());
  at::Tensor ws = workspace(wsb, x);
  at::Tensor slots = at::empty({(int64_t)M2S_FT_SLOTS}, x.options());
  ok(m2s_finetune_step(Ft(h), x.data_ptr<float>(), t.data_ptr<float>(), mk.defined() ? mk.data_ptr<float>() : nullptr,
                       len.data(), (int)len.size(), (int)x.size(0), (int)window, slots.data_ptr<float>(), ws.data_ptr(),
                       ws.numel(), S()),
     "finetune_step");
  return slots;
}

// feats (rows,208) -> predictions (P,window,n_mels), dropout on (train) or off; no update
at::Tensor finetune_forward(int64_t h, const at::Tensor& feats, at::IntArrayRef lengths, int64_t window, bool train) {
  TORCH_CHECK(feats.dim() == 2 && feats.size(1) == 208, "finetune_forward: feats must be (rows,208)");
  const Guard g(feats.device());
  const at::Tensor x = f32_on_device(feats, "feats");
  const std::vector<int> len = host_lengths(lengths, "finetune_forward lengths");
  const size_t wsb = m2s_finetune_workspace_bytes(Ft(h), len.data(), (int)len.size(), (int)window);
  TORCH_CHECK(wsb > 0, "libm2s finetune_forward: ", m2s_last_error());
  int64_t P = 0;
  for (int v : len) P += v - window + 1;
  at::Tensor ws = workspace(wsb, x);
  at::Tensor out = at::empty({P, window, (int64_t)m2s_finetune_n_mels(Ft(h))}, x.options());
  ok(m2s_finetune_forward(Ft(h), x.data_ptr<float>(), len.data(), (int)len.size(), (int)x.size(0), (int)window,
                          train ? 1 : 0, out.data_ptr<float>(), ws.data_ptr(), ws.numel(), S()),
     "finetune_forward");
  return out;
}

// the last step's gradients before clipping, in the order of m2s.h; `like` names the device
std::vector<at::Tensor> finetune_grads(int64_t h, const at::Tensor& like) {
  TORCH_CHECK(like.is_cuda(), "finetune_grads: `like` must be a HIP (cuda) tensor");
  const Guard g(like.device());
  std::vector<at::Tensor> out = ft_tensors(h, like.options().dtype(at::kFloat));
  const std::vector<float*> p = ft_ptrs(out);
  ok(m2s_finetune_grads(Ft(h), p.data(), S()), "finetune_grads");
  return out;
}

// (params[10], m[10], v[10], step (1,) int64 on the device)
std::tuple<std::vector<at::Tensor>, std::vector<at::Tensor>, std::vector<at::Tensor>, at::Tensor> finetune_export(
    int64_t h, const at::Tensor& like) {
  TORCH_CHECK(like.is_cuda(), "finetune_export: `like` must be a HIP (cuda) tensor");
  const Guard g(like.device());
  const at::TensorOptions opt = like.options().dtype(at::kFloat);
  std::vector<at::Tensor> pp = ft_tensors(h, opt), mm = ft_tensors(h, opt), vv = ft_tensors(h, opt);
  at::Tensor step = at::empty({1}, like.options().dtype(at::kLong));
  const std::vector<float*> a = ft_ptrs(pp), b = ft_ptrs(mm), c = ft_ptrs(vv);
  ok(m2s_finetune_export(Ft(h), a.data(), b.data(), c.data(), step.data_ptr<int64_t>(), S()), "finetune_export");
  return {pp, mm, vv, step};
}

// the inverse of finetune_export's m, v and step
void finetune_import(int64_t h, at::TensorList m, at::TensorList v, const at::Tensor& step) {
  TORCH_CHECK(m.size() == M2S_FT_TENSORS && v.size() == M2S_FT_TENSORS, "finetune_import: 10 tensors each");
  TORCH_CHECK(step.is_cuda() && step.scalar_type() == at::kLong && step.numel() == 1 && step.is_contiguous(),
              "finetune_import: step must be a device int64 tensor of one element");
  const Guard g(step.device());
  std::vector<at::Tensor> ref = ft_tensors(h, step.options().dtype(at::kFloat)), keep;
  std::vector<const float*> mp, vp;
  for (int i = 0; i < M2S_FT_TENSORS; ++i) {
    TORCH_CHECK(m[i].numel() == ref[i].numel() && v[i].numel() == ref[i].numel(), "finetune_import: tensor ", i,
                " has the wrong size");
    keep.push_back(f32_on_device(m[i], "m"));
    mp.push_back(keep.back().data_ptr<float>());
    keep.push_back(f32_on_device(v[i], "v"));
    vp.push_back(keep.back().data_ptr<float>());
  }
  ok(m2s_finetune_import_moments(Ft(h), mp.data(), vp.data(), step.data_ptr<int64_t>(), S()), "finetune_import");
}

}  // namespace

TORCH_LIBRARY(m2s, m) {
  m.def("mel_spectrogram(int handle, Tensor wav, int layout) -> Tensor");
  m.def("acoustic_forward(int handle, Tensor frames, int n_mels) -> Tensor");
  m.def("effnet_forward(int handle, Tensor frames) -> Tensor");
  m.def("effnet_features(int handle, Tensor frames, int n_blocks) -> Tensor");
  m.def("bilstm_summerge(int handle, Tensor feats, int hidden, int n_mels) -> (Tensor, Tensor)");
  m.def("mel_glue(Tensor mel_norm, Tensor mean, Tensor std) -> (Tensor, Tensor)");
  m.def("hifigan_forward(int handle, Tensor mel, int layout, int hop) -> Tensor");
  m.def("hifigan_features(int handle, Tensor mel, int layout, int tap, int channels, int scale) -> Tensor");
  m.def("pipeline_forward(int acoustic, int vocoder, Tensor frames, Tensor mean, Tensor std, int n_mels, int hop)"
        " -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("bilstm_summerge_ragged(int handle, Tensor feats, int[] lengths, int hidden, int n_mels) -> (Tensor, Tensor)");
  m.def("acoustic_forward_ragged(int handle, Tensor frames, int[] lengths, int n_mels) -> Tensor");
  m.def("hifigan_forward_ragged(int handle, Tensor mel, int[] lengths, int hop) -> Tensor");
  m.def("pipeline_forward_ragged(int acoustic, int vocoder, Tensor frames, int[] lengths, Tensor mean, Tensor std,"
        " int n_mels, int hop) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("bilstm_windowed(int handle, Tensor feats, int[] lengths, int[] context, int window, int merge, int hidden,"
        " int n_mels) -> (Tensor, Tensor)");
  m.def("acoustic_forward_windowed(int handle, Tensor frames, int[] lengths, int[] context, int window, int merge,"
        " int n_mels) -> Tensor");
  m.def("bilstm_pairs(int handle, Tensor feats, int[] lengths, int window, int hidden, int n_mels) -> (Tensor, Tensor)");
  m.def("acoustic_forward_pairs(int handle, Tensor frames, int[] lengths, int window, int n_mels) -> Tensor");
  m.def("mel_metrics(Tensor pred, Tensor target, Tensor? mask, int group, Tensor freq_w, Tensor time_w, float[] coeffs,"
        " int[] bands, Tensor? mean, Tensor? std, int n_mfcc, Tensor(a!) acc) -> (Tensor, Tensor)");
  m.def("hifigan_forward_chunk(int handle, Tensor mel, int[] lengths, int[] context, int[] hold, int hop) -> Tensor");
  m.def("preprocess_frames(Tensor frames) -> Tensor");
  m.def("preprocess_frames_resize(Tensor frames, int out_h, int out_w, int interp, int norm) -> Tensor");
  m.def("preprocess_frames_masked(Tensor frames, Tensor masks, int out_h, int out_w, int interp, int norm) -> Tensor");
  m.def("occlusion_reduce(Tensor mel, Tensor band_mask, Tensor? masks, bool normalize, bool want_per_frame)"
        " -> (Tensor, Tensor, Tensor)");
  m.def("cam_backbone(int handle, Tensor frames) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("bilstm_train_forward(Tensor x, Tensor[] weights) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("bilstm_train_backward(Tensor dy, Tensor x, Tensor[] weights, Tensor gates, Tensor cells, Tensor hid)"
        " -> (Tensor, Tensor[])");
  m.def("gradcam(int handle, Tensor frames, Tensor mean, Tensor std, Tensor band_mask, int[] frame_idx, int reduction,"
        " bool want_dpooled) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("gradcam_cotangents(Tensor pred_norm, Tensor mean, Tensor std, Tensor band_mask, int[] frame_idx, int reduction)"
        " -> Tensor");
  m.def("bilstm_train_backward_multi(Tensor dy, Tensor[] weights, Tensor gates, Tensor cells) -> Tensor");
  m.def("cam_heatmap(Tensor feats, Tensor weights, int[] frame, int H, int W) -> Tensor");
  m.def("linear_forward(Tensor x, Tensor weight, Tensor? bias) -> Tensor");
  m.def("linear_backward(Tensor dy, Tensor x, Tensor weight) -> (Tensor, Tensor, Tensor)");
  m.def("gap_forward(Tensor x) -> Tensor");
  m.def("gap_backward(Tensor dy, int h, int w) -> Tensor");
  m.def("finetune_step(int handle, Tensor feats, Tensor target, Tensor? mask, int[] lengths, int window) -> Tensor");
  m.def("finetune_forward(int handle, Tensor feats, int[] lengths, int window, bool train) -> Tensor");
  m.def("finetune_grads(int handle, Tensor like) -> Tensor[]");
  m.def("finetune_export(int handle, Tensor like) -> (Tensor[], Tensor[], Tensor[], Tensor)");
  m.def("finetune_import(int handle, Tensor[] m, Tensor[] v, Tensor step) -> ()");
}

TORCH_LIBRARY_IMPL(m2s, CUDA, m) {  // CUDA = the HIP device key of PyTorch-ROCm
  m.impl("acoustic_forward", &acoustic_forward);
  m.impl("effnet_forward", &effnet_forward);
  m.impl("effnet_features", &effnet_features);
  m.impl("bilstm_summerge", &bilstm_summerge);
  m.impl("mel_glue", &mel_glue);
  m.impl("hifigan_forward", &hifigan_forward);
  m.impl("hifigan_features", &hifigan_features);
  m.impl("pipeline_forward", &pipeline_forward);
  m.impl("bilstm_summerge_ragged", &bilstm_summerge_ragged);
  m.impl("acoustic_forward_ragged", &acoustic_forward_ragged);
  m.impl("hifigan_forward_ragged", &hifigan_forward_ragged);
  m.impl("pipeline_forward_ragged", &pipeline_forward_ragged);
  m.impl("bilstm_windowed", &bilstm_windowed);
  m.impl("acoustic_forward_windowed", &acoustic_forward_windowed);
  m.impl("bilstm_pairs", &bilstm_pairs);
  m.impl("acoustic_forward_pairs", &acoustic_forward_pairs);
  m.impl("mel_metrics", &mel_metrics);
  m.impl("hifigan_forward_chunk", &hifigan_forward_chunk);
  m.impl("preprocess_frames", &preprocess_frames);
  m.impl("preprocess_frames_resize", &preprocess_frames_resize);
  m.impl("preprocess_frames_masked", &preprocess_frames_masked);
  m.impl("occlusion_reduce", &occlusion_reduce);
  m.impl("cam_backbone", &cam_backbone);
  m.impl("bilstm_train_forward", &bilstm_train_forward);
  m.impl("bilstm_train_backward", &bilstm_train_backward);
  m.impl("gradcam", &gradcam);
  m.impl("gradcam_cotangents", &gradcam_cotangents);
  m.impl("bilstm_train_backward_multi", &bilstm_train_backward_multi);
  m.impl("cam_heatmap", &cam_heatmap);
  m.impl("linear_forward", &linear_forward);
  m.impl("linear_backward", &linear_backward);
  m.impl("gap_forward", &gap_forward);
  m.impl("gap_backward", &gap_backward);
  m.impl("mel_spectrogram", &mel_spectrogram);
  m.impl("finetune_step", &finetune_step);
  m.impl("finetune_forward", &finetune_forward);
  m.impl("finetune_grads", &finetune_grads);
  m.impl("finetune_export", &finetune_export);
  m.impl("finetune_import", &finetune_import);
}
