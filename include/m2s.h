/*
 * m2s.h - C ABI of libm2s, the MI355X (gfx950) implementation of the rtMRI video -> mel ->
 * waveform inference hot path of YamaneKoyo/mri-to-speech.
 *
 * Plain pointers and sizes only.  Every device pointer is a HIP device allocation on the
 * object's device; `stream` is a hipStream_t (NULL = default stream).  Every call is
 * asynchronous on `stream` unless stated otherwise.  Functions return M2S_OK or an error
 * code; m2s_last_error() gives a thread-local message.  Nothing here falls back to the CPU:
 * without a gfx950 device the create calls fail with M2S_E_NODEV.
 *
 * Reference interfaces replaced (paths inside the reference repository):
 *   m2s_acoustic_*      OTNLikeCNNBiLSTM built by build_acoustic_model(**kw) and loaded with
 *                       load_state_dict(strict=False)   mri2speech_code/mri_acoustic_model.py:74-156,
 *                       scripts/run_mri_video_inference.py:119-148
 *   m2s_acoustic_forward   OTNLikeCNNBiLSTM.forward (eval)   mri_acoustic_model.py:116-136
 *   m2s_effnet_forward     EffNetV2B2Backbone.forward + GlobalAvgPool   mri_acoustic_model.py:15-18,39-48
 *   m2s_bilstm_summerge    BiLSTMSumMerge.forward + head Linear   mri_acoustic_model.py:67-72,135
 *   m2s_mel_glue           denormalize_mel + dB -> ln-power   run_mri_video_inference.py:160-163,227-233
 *   m2s_vocoder_*          Generator(h) + load_state_dict(ckpt['generator']) + weight-norm removal
 *                          models.py:88-109, run_mri_video_inference.py:89-116
 *   m2s_vocoder_forward    Generator.forward   models.py:113-131
 *   m2s_pipeline_forward   the no_grad section of main()   run_mri_video_inference.py:222-242
 *   m2s_cam_*              the train-mode backbone forward of compute_gradcam (model.train(): BatchNorm
 *                          on batch statistics)   scripts/mri_gradcam_formant.py:153-160,221-225
 *   m2s_bilstm_train_*     BiLSTMSumMerge forward + autograd backward   mri_acoustic_model.py:50-72,
 *                          scripts/mri_gradcam_formant.py:162-164,247-248
 *   m2s_linear_*           nn.Linear head forward + backward   mri_acoustic_model.py:103,135,
 *                          scripts/mri_gradcam_formant.py:165
 *   m2s_gap_*              GlobalAvgPool / feats.mean((2,3)) forward + backward
 *                          mri_acoustic_model.py:15-18, scripts/mri_gradcam_formant.py:162
 *   m2s_gradcam_*          compute_gradcam for all bands and target frames of a clip, heat maps included
 *                          scripts/mri_gradcam_formant.py:128-279,407-426
 *   m2s_bilstm_train_backward_multi   the LSTM part of the backward() calls, all targets at once   :247-248,262-266
 *   m2s_cam_heatmap        _compute_cam_from_grads   scripts/mri_gradcam_formant.py:169-200
 *   m2s_melspec_*          mel_spectrogram (reflect pad, periodic-Hann STFT, magnitude, mel, ln)
 *                          meldataset.py:57-93, as inference.py:25-26 and train.py:228-252 call it; and
 *                          pre_emphasis + compute_mel_db up to the dB map (the caller supplies the mel basis)
 *                          mri2speech_code/preprocess_rtmri_data.py:37-43,121-147
 *   m2s_*_pairs         the model on every training pair of a clip: the windows pass3_save_pairs cuts
 *                          mri2speech_code/preprocess_rtmri_data.py:198-259, as OTNLikeTrainer.validate() feeds them
 *                          to the model   mri2speech_code/train_mri_acoustic_model.py:349-384
 *   m2s_mel_metrics     the weighted MaskedMSEMAE criterion and the band MAEs of validate()
 *                          train_mri_acoustic_model.py:57-167,263-277; eval_mel.py's MaskedMSEMAE, mcd_like and
 *                          evaluation loop   mri2speech_code/eval_mel.py:19-32,39-82,104-155
 */
#ifndef M2S_H_
#define M2S_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M2S_ABI_VERSION 6

enum m2s_status { M2S_OK = 0, M2S_E_ARG = 1, M2S_E_HIP = 2, M2S_E_STATE = 3, M2S_E_NODEV = 4, M2S_E_INTERNAL = 5 };
/* compute dtype of the convolution stacks.  The BiLSTM input projection, head and glue run in fp32 in every
 * dtype; the BiLSTM recurrence runs exact-f32 products in M2S_DT_F32 and for B <= 4 (lstm_small_kernel), and
 * split three-term bf16x3 products (W_hh and h_t as hi + lo bf16 pairs, fp32 cell state and gates;
 * lstm_x3_kernel) for B > 4 in the BF16, BF16X3 and FP8 engines:
 *   M2S_DT_F32    exact f32 MFMA products (v_mfma_f32_16x16x4_f32), fp32 storage
 *   M2S_DT_BF16   bf16 storage and operands, fp32 accumulation
 *   M2S_DT_BF16X3 split fp32: every activation / weight is a bf16 pair hi + lo (17 significant
 *                 bits), products are the three bf16 MFMA terms hi*hi + hi*lo + lo*hi with fp32
 *                 accumulation; meets the fp32 tolerances of the parity tests
 *   M2S_DT_FP8    configs[4]: OCP e4m3 storage and block-scaled e4m3 MFMA
 *                 (v_mfma_scale_f32_16x16x128_f8f6f4, unit E8M0 block scales, per-output-channel
 *                 fp32 weight scales applied in the epilogue) for: the IR blocks' conv_pw expand
 *                 (stride 1 and blocks.5.0), expanded maps and SE-gated conv_pwl GEMMs (every IR
 *                 block, blocks.3.0 / 5.0 included); the EdgeResidual blocks.1.1/.2 and blocks.2.1/.2
 *                 (conv_exp + conv_pwl); the C = 128 / 256 MRF convs (C = 64 / 32 on request:
 *                 M2S_F8_MRF64 / M2S_F8_MRF32, slower than the fused bf16 ResBlock1).  The stem, the
 *                 stride-2 EdgeResidual blocks.1.0 / 2.0, the blocks.3.0 expand, the IR depthwise convs
 *                 (f16 or fp32 accumulation of a 16-bit tile), the C = 32 / 64 MRF convs and the
 *                 upsamplers run the bf16 path */
enum m2s_dtype { M2S_DT_F32 = 0, M2S_DT_BF16 = 1, M2S_DT_BF16X3 = 2, M2S_DT_FP8 = 3 };
/* host tensor element types */
enum m2s_elem { M2S_ELEM_F32 = 0, M2S_ELEM_I64 = 1 };

int m2s_abi_version(void);
const char* m2s_last_error(void);
/* M2S_OK if HIP device `device` exists and is gfx950 (synchronous). */
int m2s_device_check(int device);

/* One state-dict entry, reference key name, contiguous row-major HOST memory. */
typedef struct m2s_tensor {
  const char* name;
  const void* data;
  int elem; /* m2s_elem */
  int ndim;
  int64_t shape[4];
} m2s_tensor;

/* ------------------------------------------------------------------ acoustic model ---- */
typedef struct m2s_acoustic m2s_acoustic;

/* Packs a reference-format state dict (keys of OTNLikeCNNBiLSTM.state_dict(): cnn.backbone.*,
 * rnn.lstm.*, head.*) for `device`: BatchNorm folded, grey->RGB repeat folded into conv_stem,
 * layouts converted.  Unknown keys are ignored (strict=False); a missing required key is
 * M2S_E_ARG naming the key.  Synchronous. */
int m2s_acoustic_create(const m2s_tensor* sd, int n, int n_mels, int rnn_hidden, int dtype, int device,
                        m2s_acoustic** out);
void m2s_acoustic_destroy(m2s_acoustic* m);
/* frames per CNN pass (bounds the CNN workspace); default 1920 (= m2s.config.CNN_CHUNK, the size bench.py times).
 * A pass may hold up to chunk + chunk / 16 frames where one pass fewer then covers N (no short tail pass), so
 * the workspace and the kernels' size checks see up to ~6 % more frames than `frames`. */
int m2s_acoustic_set_chunk(m2s_acoustic* m, int frames);
/* Asynchronous failure report.  The persistent BiLSTM waits at a grid barrier once per time step, and
 * the persistent CNN kernels (ir_ws, se_ws) at LDS flags between their producer and consumer waves;
 * a wait that exceeds its poll limit poisons the affected outputs with NaN and raises a host-visible flag.  This call returns M2S_E_INTERNAL (and clears the flag) when such a
 * launch has happened: call it after synchronising the stream.  The next forward / bilstm /
 * pipeline call on the engine fails the same way.  Synchronous, host only. */
int m2s_acoustic_status(m2s_acoustic* m);
/* Fault injection for tests: polls per BiLSTM barrier wait before it times out (default 2^24); 0 makes
 * the first wait time out unconditionally. */
int m2s_acoustic_set_lstm_spin_limit(m2s_acoustic* m, unsigned polls);
/* Fault injection for tests: polls per LDS flag-ring wait of the persistent CNN kernels (ir_ws producers'
 * weight-slot wait, se_ws FULL / FREE waits; default 2^20) before it times out; 0 makes every such wait time out.
 * A timeout poisons the affected outputs with NaN and is reported by m2s_acoustic_status. */
int m2s_acoustic_set_ws_spin_limit(m2s_acoustic* m, unsigned polls);
/* Workspace contract, for every `ws` / `ws_bytes` pair and every *_workspace_bytes query of this header
 * (tests/test_gpu_workspace.py holds each entry point to it):
 *   - `ws` is caller-owned device memory, 256-byte aligned.  Its contents on entry are arbitrary: no call reads a
 *     workspace byte it has not written itself during that call, so NaN bit patterns, random bytes or the leftovers
 *     of any earlier call give bit-identical outputs.
 *   - Nothing in the workspace persists between calls: it may be reused, overwritten or freed once the stream has
 *     passed the call.  What an engine keeps across calls (the BiLSTM hand-off tags) it owns itself.
 *   - The size a query reports is sufficient, and it is exact to its 256-byte granule for the call the query is named
 *     after (m2s_acoustic_forward, m2s_vocoder_forward, m2s_pipeline_forward, their *_ragged forms,
 *     m2s_cam_backbone, m2s_bilstm_train_backward, m2s_gradcam_forward, m2s_bilstm_train_backward_multi,
 *     m2s_acoustic_forward_pairs, m2s_bilstm_pairs with H = W = 0, m2s_mel_metrics): 256 bytes less is refused with M2S_E_ARG, nothing outside the
 *     caller's buffers is written, and the engine stays usable.  The calls without a query of their own take the
 *     enclosing call's and use a part of it: m2s_effnet_forward / m2s_effnet_probe on N frames that of
 *     m2s_acoustic_workspace_bytes(m, N, 1, H, W); m2s_bilstm_summerge that of (m, B, T, H, W) for any valid frame
 *     size, e.g. 64 x 64; m2s_bilstm_summerge_ragged that of m2s_acoustic_ragged_workspace_bytes likewise;
 *     m2s_bilstm_train_forward that of m2s_bilstm_train_workspace_bytes.
 *   - Every size query returns 0 for a null handle.
 *   - Every output is written completely, each element from this call's inputs alone, and no byte outside the
 *     outputs and the workspace is written: outputs have exactly their documented size, with no slack. */
size_t m2s_acoustic_workspace_bytes(const m2s_acoustic* m, int B, int T, int H, int W);
/* frames (B,T,H,W) fp32 in [0,1] -> mel_norm (B,T,n_mels) fp32. */
int m2s_acoustic_forward(m2s_acoustic* m, const float* frames, int B, int T, int H, int W, float* mel_norm,
                         void* ws, size_t ws_bytes, void* stream);
/* frames (N,H,W) -> feats (N,208) fp32 (GAP of the last timm feature map). */
int m2s_effnet_forward(m2s_acoustic* m, const float* frames, int N, int H, int W, float* feats, void* ws,
                       size_t ws_bytes, void* stream);
/* Debug tap: feature map after `n_blocks` timm blocks (0 = after conv_stem/bn1), written as
 * (N,OH,OW,C) fp32 dense to `out`; returns OH, OW, C through the pointers. */
int m2s_effnet_probe(m2s_acoustic* m, const float* frames, int N, int H, int W, int n_blocks, float* out,
                     int* oh, int* ow, int* oc, void* ws, size_t ws_bytes, void* stream);
/* feats (B,T,208) -> y (B,T,rnn_hidden) sum-merged BiLSTM output (may be NULL) and
 * mel_norm (B,T,n_mels) head output (may be NULL). */
int m2s_bilstm_summerge(m2s_acoustic* m, const float* feats, int B, int T, float* y, float* mel_norm, void* ws,
                        size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------- mel glue ---- */
/* mel_db = x*std + mean; mel_log = ln(clamp(10^(mel_db/10), 1e-5)); x (rows,n_mels).
 * mean/std are DEVICE fp32 arrays of n_mels; either output may be NULL. */
int m2s_mel_glue(const float* mel_norm, int rows, int n_mels, const float* mean, const float* std, float* mel_db,
                 float* mel_log, void* stream);

/* ----------------------------------------------------------------------- vocoder ---- */
typedef struct m2s_hifigan_h {
  int resblock; /* 1 or 2 (h.resblock "1"/"2") */
  int num_mels;
  int upsample_initial_channel;
  int n_up;
  int upsample_rates[8];
  int upsample_kernel_sizes[8];
  int n_kernels;
  int resblock_kernel_sizes[8];
  int n_dilations[8];
  int resblock_dilation_sizes[8][8];
} m2s_hifigan_h;

typedef struct m2s_vocoder m2s_vocoder;

/* Frame preprocessing after the host decode (replaces _preprocess_frame,
 * run_mri_video_inference.py:34-54, on frames that already have the model's size): frames uint8 (n,h,w) grey
 * (channels = 1) or (n,h,w,3) BGR (channels = 3) -> out (n,h,w) fp32, per frame z-score then
 * min-max to [0, 1]; a constant frame gives zeros.  Device pointers, stream-ordered. */
int m2s_preprocess_frames(const uint8_t* frames, int n, int h, int w, int channels, float* out, void* stream);

/* The whole frame front end on the device, resize included: frames uint8 (n,h,w) grey (channels = 1) or
 * (n,h,w,3) BGR (channels = 3) at the scanner's size -> out (n,out_h,out_w) fp32.  BGR -> grey first (the
 * reference resizes the grey frame), then the resize, then the normalisation, in one kernel with no workspace.
 * Serves both frame conventions of the reference:
 *   inference   scripts/run_mri_video_inference.py:34-54 (_preprocess_frame): cv2.INTER_LINEAR, per-frame
 *               z-score, min-max to [0, 1]            -> M2S_FRAME_LINEAR, M2S_FRAME_ZSCORE_MINMAX
 *   training    mri2speech_code/preprocess_rtmri_data.py:99-113: cv2.INTER_AREA, / 255
 *                                                     -> M2S_FRAME_AREA, M2S_FRAME_UNIT
 * The resize is OpenCV's 8-bit two-tap fixed-point path (11-bit weights), which INTER_AREA also takes where no
 * axis shrinks.  Limits, each M2S_E_ARG before anything is launched: channels is 1 or 3; h <= out_h and
 * w <= out_w (shrinking takes other OpenCV paths: true area averaging, the exact-2x case); h*w <= 65536 and
 * out_h*out_w <= 65536; interp and norm are values of the enums below.  n = 0 is a no-op.  Equal sizes give
 * m2s_preprocess_frames' output bit for bit with LINEAR + ZSCORE_MINMAX.  Stateless: nothing is staged from the
 * host, so the call can be captured into a graph.  Device pointers, stream-ordered. */
enum m2s_frame_interp { M2S_FRAME_LINEAR = 0, M2S_FRAME_AREA = 1 };
enum m2s_frame_norm { M2S_FRAME_ZSCORE_MINMAX = 0, M2S_FRAME_UNIT = 1 };
int m2s_preprocess_frames_resize(const uint8_t* frames, int n, int h, int w, int channels, int out_h, int out_w,
                                 int interp, int norm, float* out, void* stream);

/* ------------------------------------------------------------------- occlusion ----
 * The masking experiment (scripts/mask_rtmri_video.py, docs/rtmri_pipeline_notes.md step 5) on the device.
 *
 * m2s_preprocess_frames_masked: the frame front end above for n_masks masked variants of every frame in one
 * launch.  masks is device fp32 (n_masks,h,w); out is (n_masks,n,out_h,out_w).  Variant m of frame i is the
 * reference's application, every byte of every channel -> (uint8)clip((float)byte * masks[m][y][x], 0, 255)
 * (one IEEE multiply, truncation toward zero: numpy's bits), followed by m2s_preprocess_frames_resize: BGR ->
 * grey, resize, normalisation.  Mask values outside [0, 1] are legal (the clip handles them); masks must be
 * finite.  M2S_E_ARG before anything is launched: every refusal of m2s_preprocess_frames_resize, n_masks outside
 * 1..65535, a null masks with n > 0.  n = 0 is a no-op.  Stateless, no workspace, writes out completely and
 * nothing else; can be captured into a graph.  Device pointers, stream-ordered. */
int m2s_preprocess_frames_masked(const uint8_t* frames, int n, int h, int w, int channels, const float* masks, int n_masks,
                                 int out_h, int out_w, int interp, int norm, float* out, void* stream);

/* m2s_occlusion_reduce: the variants' mels of ONE clip -> scores and an occlusion-sensitivity map, without a host
 * read.  mel is device fp32 (V,T,n_mels), variant 0 the unmasked baseline, variant m + 1 the clip under mask m,
 * M = V - 1.  band_mask is device fp32 (n_bands,n_mels) of 0 / 1 (the Grad-CAM bands); an "all bins" column is
 * always appended: nb = n_bands + 1.  Outputs, device fp32:
 *   score     (M,nb)    mean over t and over the band's bins of |mel[m + 1] - mel[0]| (dB where mel is mel_db);
 *                       a band without bins scores 0
 *   per_frame (M,T,nb)  the same per frame; may be NULL
 *   map       (nb,h,w)  sum_m c_m score[m][b] / sum_m c_m with c_m = max(1 - masks[m], 0), masks device fp32
 *                       (M,h,w), finite; 0 where sum_m c_m > 1e-6 does not hold.  With normalize != 0 every band
 *                       becomes (v - min) / ((max - min) + 1e-6) over its pixels, the Grad-CAM heat maps' rule: a
 *                       flat band gives zeros.  May be NULL, and masks with it.
 * At most two launches, no atomics, a fixed summation order: repeated calls are bit-identical.  M2S_E_ARG before
 * anything is launched: V < 2, T < 1, n_mels outside 1..256, n_bands outside 0..8, a null band_mask with
 * n_bands > 0, a null mel or score, a map without masks or with h or w < 1.  No workspace; can be captured into
 * a graph.  Stream-ordered. */
int m2s_occlusion_reduce(const float* mel, int V, int T, int n_mels, const float* band_mask, int n_bands,
                         const float* masks, int h, int w, int normalize, float* score, float* per_frame, float* map,
                         void* stream);

/* Packs a Generator state dict (weight_g/weight_v or plain weight after remove_weight_norm).
 * Strict like load_state_dict(ckpt['generator']): a missing key is M2S_E_ARG.  Synchronous. */
int m2s_vocoder_create(const m2s_tensor* sd, int n, const m2s_hifigan_h* h, int dtype, int device, m2s_vocoder** out);
void m2s_vocoder_destroy(m2s_vocoder* v);
size_t m2s_vocoder_workspace_bytes(const m2s_vocoder* v, int B, int T);
/* mel fp32, layout 0 = (B,num_mels,T) as Generator.forward takes it, 1 = (B,T,num_mels);
 * wav (B, T*prod(upsample_rates)) fp32. */
int m2s_vocoder_forward(m2s_vocoder* v, const float* mel, int mel_layout, int B, int T, float* wav, void* ws,
                        size_t ws_bytes, void* stream);
/* Debug tap (as m2s_effnet_probe for the CNN): the dense call m2s_vocoder_forward up to one stored tensor, which is
 * then copied to `out` as fp32 (B, L, C), channel-last and dense; L (rows per clip) and C come back through the
 * pointers (any of them may be NULL).  Taps: 0 = conv_pre's output (L = T, C = upsample_initial_channel);
 * 2i + 1 = stage i's upsampler output; 2i + 2 = stage i's MRF output (the resblocks' mean), i = 0 .. n_up - 1
 * (L = T * the rates up to stage i, C = upsample_initial_channel >> (i + 1)).
 *   - The values are returned exactly as stored: in a bf16 / fp8 engine every float is a bf16 value, in a bf16x3
 *     engine the sum of the two stored bf16 planes.
 *   - Where the engine hands the tensor on as LeakyReLU(x) (slope 0.1; the split engine's batched stages and the
 *     producers in front of them), the buffer is returned as it is and *lrelu is set to 1, else 0.  Nothing is
 *     inverted.  m2s_vocoder_tap_info gives L, C and the flag without a launch.
 *   - `ws` is that of m2s_vocoder_workspace_bytes(v, B, T); the launches are those of m2s_vocoder_forward up to the
 *     tap plus one copy, and m2s_vocoder_forward itself is unchanged by the tap's existence.
 *   - M2S_E_ARG before any launch: a null v, mel, out or ws, mel_layout other than 0 / 1, B or T < 1, tap outside
 *     0 .. 2 n_up.  M2S_E_STATE if `stream` is capturing.  Dense calls only. */
int m2s_vocoder_probe(m2s_vocoder* v, const float* mel, int mel_layout, int B, int T, int tap, float* out, int* L,
                      int* C, int* lrelu, void* ws, size_t ws_bytes, void* stream);
int m2s_vocoder_tap_info(const m2s_vocoder* v, int tap, int T, int* L, int* C, int* lrelu);

/* ------------------------------------------------------------------- end to end ---- */
size_t m2s_pipeline_workspace_bytes(const m2s_acoustic* m, const m2s_vocoder* v, int B, int T, int H, int W);
/* frames (B,T,H,W) -> mel_norm, mel_db, mel_log (B,T,n_mels) and wav (B,T*hop).  mel_* may be NULL. */
int m2s_pipeline_forward(m2s_acoustic* m, m2s_vocoder* v, const float* frames, int B, int T, int H, int W,
                         const float* mean, const float* std, float* mel_norm, float* mel_db, float* mel_log,
                         float* wav, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- graph capture ---- */
/* The DENSE entry points may be called on a stream that is being captured into a HIP graph (hipStreamBeginCapture,
 * torch.cuda.graph) and the graph replayed any number of times: m2s_acoustic_forward, m2s_effnet_forward,
 * m2s_effnet_probe, m2s_bilstm_summerge, m2s_mel_glue, m2s_vocoder_forward, m2s_pipeline_forward, and the stateless
 * calls that say so (m2s_preprocess_frames_resize, m2s_preprocess_frames_masked, m2s_occlusion_reduce,
 * m2s_mel_metrics).  A replay computes, bit for bit, what the same engine's eager call computes on the buffers'
 * contents at replay time (tests/test_gpu_graph.py).  The calls that stage a host table per call refuse a capturing
 * stream with M2S_E_STATE before anything is launched: the ragged, windowed, pairs and chunk calls and
 * m2s_gradcam_forward.  Profiling (m2s_prof_enable) records events around every launch: leave it off while capturing.
 * What the caller owes:
 *   - Inputs, outputs and the workspace are baked into the graph as addresses: all of them stay allocated, at those
 *     addresses, for the graph's life, and no other work may use the workspace while a replay runs.
 *   - One stream at a time per engine.  An acoustic engine owns the BiLSTM hand-off buffer and its error word (below),
 *     so eager calls and replays on one engine must not overlap: order them on one stream or with events.
 *   - Split K: small launches of the convolution GEMMs spread K over several workgroups through a scratch buffer the
 *     library keeps per (device, stream) and grows on demand.  A capturing stream cannot allocate: it borrows the
 *     device's largest such buffer, and where none is large enough the launch is recorded unsplit (correct, slower,
 *     and rounded as the unsplit kernel rounds).  So run one eager call of the same shape on the device before the
 *     capture if split K is to stay on, which the usual warm-up does.  The graph keeps the borrowed address: the
 *     stream that owns the buffer must not run a larger call (which frees and regrows it) while the graph is alive,
 *     nor split-K launches of its own while the graph replays on another stream.
 *   - m2s_acoustic_status after synchronising, as for eager calls: a replay's hand-off timeout is reported the same way.
 * The BiLSTM hand-off tags (lstm_small_kernel, lstm_x3g_kernel): eager calls continue one epoch count per engine and
 * never clear the buffer.  A captured call records the zeroing of the buffer (a kernel node) and runs at epoch 0, so
 * every replay RESTARTS the buffer's tags; the capture itself leaves the buffer alone and never lowers the engine's
 * count (it raises it to T + 1 at least), so eager calls before, between and after captures and replays, in any
 * order, never meet a tag they could take for their own (csrc/lstm_route.hpp lstm_epoch_rule).  The other
 * recurrence kernels zero their sync words in the workspace per launch, under capture by a kernel node too. */

/* ---------------------------------------------------------------- ragged batches ---- */
/* Clips of different lengths in one call.  The data is PACKED: `lengths` is a HOST array of B integers, each
 * >= 1; N = sum(lengths); clip b owns rows off_b .. off_b + lengths[b] - 1 of every (N, ...) tensor, off = the
 * exclusive prefix sum.  Frames are (N,H,W), feats (N,208), mels (N,n_mels), wav (N*hop).  Padding to
 * Tmax = max(lengths) exists only inside the workspace: the batched kernels run on (B,Tmax) blocks, with exact
 * zeros written where a short clip's reverse LSTM direction and the generator's look-ahead (conv_pre, every
 * ConvTranspose1d, conv_post) must see them, so each clip's result is the per-clip one (DESIGN.md "Ragged
 * batches").  With all lengths equal every output is bit-identical to the dense entry point's on (B,T).
 * M2S_E_ARG, before any launch, if B < 1, a length is < 1, or sum(lengths) != `rows`.  The clip table travels
 * through an engine-owned pinned buffer per call, so these calls cannot be captured into a graph: M2S_E_STATE if
 * `stream` is capturing.  The *_workspace_bytes queries return 0 for arguments the calls would reject. */
size_t m2s_acoustic_ragged_workspace_bytes(const m2s_acoustic* m, const int* lengths, int B, int H, int W);
/* feats (rows,208) -> y (rows,rnn_hidden) (may be NULL) and mel_norm (rows,n_mels) (may be NULL), packed. */
int m2s_bilstm_summerge_ragged(m2s_acoustic* m, const float* feats, const int* lengths, int B, int rows, float* y,
                               float* mel_norm, void* ws, size_t ws_bytes, void* stream);
/* frames (rows,H,W) fp32 in [0,1] -> mel_norm (rows,n_mels), packed. */
int m2s_acoustic_forward_ragged(m2s_acoustic* m, const float* frames, const int* lengths, int B, int rows, int H,
                                int W, float* mel_norm, void* ws, size_t ws_bytes, void* stream);
size_t m2s_vocoder_ragged_workspace_bytes(const m2s_vocoder* v, const int* lengths, int B);
/* mel (rows,num_mels) fp32, packed layout 1 -> wav (rows*hop) fp32, packed. */
int m2s_vocoder_forward_ragged(m2s_vocoder* v, const float* mel, const int* lengths, int B, int rows, float* wav,
                               void* ws, size_t ws_bytes, void* stream);
size_t m2s_pipeline_ragged_workspace_bytes(const m2s_acoustic* m, const m2s_vocoder* v, const int* lengths, int B,
                                           int H, int W);
/* frames (rows,H,W) -> mel_norm, mel_db, mel_log (rows,n_mels) and wav (rows*hop), packed.  mel_* may be NULL. */
int m2s_pipeline_forward_ragged(m2s_acoustic* m, m2s_vocoder* v, const float* frames, const int* lengths, int B,
                                int rows, int H, int W, const float* mean, const float* std, float* mel_norm,
                                float* mel_db, float* mel_log, float* wav, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------ windowed inference ---- */
/* The acoustic checkpoint is trained on overlapping windows of ref_frames (default 4) frames, stride 1, with the
 * BiLSTM starting from zero state in both directions on every window; the reference's own inference (and every
 * entry point above) runs the recurrence over the whole clip.  These ADDITIVE calls run it over sliding windows
 * instead (DESIGN.md "Windowed acoustic inference").  M(x) = the per-clip forward on k rows (projection, BiLSTM
 * from zero state, sum merge, head), W = `window` (1..16), inputs packed as in the ragged calls:
 *   M2S_WINDOW_LATEST  out[t] = M(x[max(0, t - W + 1) .. t])[last]: causal, the window ENDING at t; the first W - 1
 *                      frames of a clip use the truncated window that starts at the clip's first row
 *   M2S_WINDOW_MEAN    len <= W: out = M(x); otherwise out[t] = the mean, over the full windows w = 0 .. len - W that
 *                      contain t, of M(x[w .. w + W - 1])[t - w] (a fixed-order average of the merged hidden rows,
 *                      then the head)
 * `context` (LATEST only, may be NULL) is a HOST array of B integers, 0 <= context[b] <= min(W - 1, lengths[b] - 1):
 * the first context[b] rows of clip b are history that windows reach into but that get no output row, so the outputs
 * hold rows = sum(lengths[b] - context[b]) packed rows in clip order.  That is the whole streaming state: keep the
 * last W - 1 FEATURE rows of a stream, prepend them to the next chunk, and the rows are bit-identical to one call
 * over the concatenation.  No hidden state crosses a call, and a row's bits do not depend on what else is in the
 * batch.  The recurrence is a launch per step (lstm_window.hip): no cross-workgroup waits, nothing that can time
 * out, and the asynchronous error word is not involved.
 * M2S_E_ARG, before any launch: window outside 1..16, an unknown merge, a context with MEAN, a context entry out of
 * range, rnn_hidden != 640, and the ragged calls' argument errors.  M2S_E_STATE if `stream` is capturing (the clip
 * table is staged per call, as in the ragged calls).  The workspace contract above applies as written. */
enum m2s_window_merge { M2S_WINDOW_LATEST = 0, M2S_WINDOW_MEAN = 1 };
/* Exact size for m2s_acoustic_forward_windowed on (H, W) frames; with H = W = 0 the exact size for
 * m2s_bilstm_windowed alone.  0 for arguments the calls would reject. */
size_t m2s_acoustic_windowed_workspace_bytes(const m2s_acoustic* m, const int* lengths, const int* context, int B,
                                             int H, int W, int window, int merge);
/* feats (rows,208) -> y (out_rows,rnn_hidden) merged hidden rows (may be NULL) and mel_norm (out_rows,n_mels) (may
 * be NULL), out_rows = rows - sum(context). */
int m2s_bilstm_windowed(m2s_acoustic* m, const float* feats, const int* lengths, const int* context, int B, int rows,
                        int window, int merge, float* y, float* mel_norm, void* ws, size_t ws_bytes, void* stream);
/* frames (rows,H,W) fp32 in [0,1] -> mel_norm (out_rows,n_mels).  The CNN runs once per frame row. */
int m2s_acoustic_forward_windowed(m2s_acoustic* m, const float* frames, const int* lengths, const int* context, int B,
                                  int rows, int H, int W, int window, int merge, float* mel_norm, void* ws,
                                  size_t ws_bytes, void* stream);

/* -------------------------------------------------------- validation: pair outputs ---- */
/* The training pairs of the reference (preprocess_rtmri_data.py:198-259) are every window of `window` consecutive
 * frames of a clip, stride 1.  These ADDITIVE calls give the model's output on every row of every pair, which a
 * loss over pairs needs (LATEST keeps one row per window, MEAN averages them), with the CNN run once per frame row.
 * Inputs are packed exactly as in the *_windowed calls.  P = sum(lengths[b] - window + 1); pair p = pbase_b + i is
 * the window on rows i .. i + window - 1 of clip b, pairs in clip order, windows ascending within a clip (the order
 * pass3_save_pairs writes them); row s of pair p is M(x_b[i .. i + window - 1])[s], M as defined above.  The route is
 * MEAN's (same window table, same step launches, every step's h kept); lstm_window_pairs_kernel then writes the
 * sum-merged rows and the head runs on P * window rows.  Row window - 1 of a pair is bit-identical to LATEST's row
 * of the same frame.
 * M2S_E_ARG, before any launch: window outside 1..16, a lengths[b] < window (the reference skips such clips, so the
 * caller must too), rnn_hidden != 640, and the ragged calls' argument errors.  M2S_E_STATE if `stream` is capturing.
 * The workspace contract above applies as written. */
/* Exact size for m2s_acoustic_forward_pairs on (H, W) frames; with H = W = 0 the exact size for m2s_bilstm_pairs
 * alone.  0 for arguments the calls would reject. */
size_t m2s_acoustic_pairs_workspace_bytes(const m2s_acoustic* m, const int* lengths, int B, int H, int W, int window);
/* feats (rows,208) -> y (P,window,rnn_hidden) (may be NULL) and mel_norm (P,window,n_mels) (may be NULL). */
int m2s_bilstm_pairs(m2s_acoustic* m, const float* feats, const int* lengths, int B, int rows, int window, float* y,
                     float* mel_norm, void* ws, size_t ws_bytes, void* stream);
/* frames (rows,H,W) fp32 in [0,1] -> mel_norm (P,window,n_mels). */
int m2s_acoustic_forward_pairs(m2s_acoustic* m, const float* frames, const int* lengths, int B, int rows, int H, int W,
                               int window, float* mel_norm, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------- validation: fused mel metrics ---- */
/* The reference's validation numbers of one batch of (B,T,M) predictions in two launches and no host sync
 * (DESIGN.md §24): the weighted MaskedMSEMAE criterion and band MAEs of OTNLikeTrainer.validate(), eval_mel.py's
 * masked MSE / MAE and its MCD-like.  pred / target (B,T,M) standardised dB mels, mask (B,T) floats or NULL = ones;
 * every array argument is device memory except `bands`.
 * Groups: sequences fall into consecutive groups of `group` sequences (0 or >= B: one group; the last may be
 * short).  A group is one batch of the reference: every loss is computed per group and summed over the groups, and
 * GROUPS counts them, so the reference's tot / cnt is a division on the host.
 * With diff = pred - target, w[b,t,m] = freq_w[m] time_w[t] mask[b,t], sums over one group:
 *   MSE     sum diff^2 w / max(sum w, 1e-6);  MAE likewise with |diff|
 *   DELTA   d = diff[t] - diff[t-1], t >= 1, weight freq_w[m] time_w[t] mask[t] mask[t-1] (the LATER row's time
 *           weight): sum d^2 w / max(sum w, 1e-6); 0 when T = 1
 *   ACCEL   a = diff[t+1] - 2 diff[t] + diff[t-1], weight freq_w[m] time_w[t] mask[t+1] mask[t] mask[t-1] (the MIDDLE
 *           row's time weight); 0 when T <= 2
 *   LATEST  row T - 1, NOT masked, not time-weighted: sum diff^2 freq_w / max(group size * sum freq_w, 1e-6)
 *   LOSS    MSE + delta_coeff DELTA + accel_coeff ACCEL + latest_coeff LATEST
 *   BANDk   the plain (unmasked) mean of |diff| over all b, t and bands[2k] <= m < min(bands[2k+1], M); a band
 *           that is empty after clipping adds nothing
 *   EVAL_*  eval_mel.py:24-32: e = diff mask; EVAL_MSE = sum e^2 / max(sum mask, 1) (frames, not frames x M; the
 *           mask is squared with the difference), EVAL_MAE = sum |e| / the same, EVAL_LOSS = 0.8 MSE + 0.2 MAE
 *   MCD     per sequence over its rows with mask != 0 (mean and std non-NULL): db = x std + mean;
 *           x' = max(max(db, -100), max over the sequence's masked rows and all mels of that - 80), the maximum
 *           taken separately for pred and target (power_to_db(db_to_power(.)), ref 1, amin 1e-10, top_db 80);
 *           c_k = s_k sum_m x'_m cos(pi k (2m + 1) / 2M), k < n_mfcc, s_0 = sqrt(1/M), s_k = sqrt(2/M);
 *           value = (10 / ln 10) sqrt(2) mean over rows of |c_pred - c_tgt|_2.  A sequence without a masked row or
 *           with a non-finite value is skipped.  MCD_SUM / MCD_COUNT: the values' sum and count.
 * `acc` (M2S_METRICS_SLOTS doubles) is ADDED to; `out` (M2S_METRICS_SLOTS floats) holds this call alone; `per_seq`
 * (B,3) holds a sequence's masked squared-difference sum, absolute sum and MCD-like (NaN where skipped).  Each may
 * be NULL.  One workgroup per sequence writes its partial sums to the workspace (fp32 lanes, fixed-order tree); one
 * workgroup reduces them per group in ascending sequence order in double.  No atomics, no waits: a call is
 * bit-reproducible and a sequence's per_seq row does not depend on what else is in the batch.
 * M2S_E_ARG, before any launch: B, T or M < 1, M > 256, n_bands outside 0..8, a null bands with n_bands > 0, only one
 * of mean / std, n_mfcc < 1 or > M with MCD on, n_mfcc > 64, an undersized workspace.  Stateless: can be captured. */
enum m2s_metrics_slot {
  M2S_MET_LOSS = 0, M2S_MET_MSE, M2S_MET_MAE, M2S_MET_DELTA, M2S_MET_ACCEL, M2S_MET_LATEST,
  M2S_MET_BAND0, M2S_MET_BAND1, M2S_MET_BAND2, M2S_MET_BAND3, M2S_MET_BAND4, M2S_MET_BAND5, M2S_MET_BAND6,
  M2S_MET_BAND7, M2S_MET_EVAL_LOSS, M2S_MET_EVAL_MSE, M2S_MET_EVAL_MAE, M2S_MET_GROUPS, M2S_MET_MCD_SUM,
  M2S_MET_MCD_COUNT, M2S_METRICS_SLOTS
};
size_t m2s_mel_metrics_workspace_bytes(int B);
int m2s_mel_metrics(const float* pred, const float* target, const float* mask, int B, int T, int M, int group,
                    const float* freq_w, const float* time_w, float delta_coeff, float accel_coeff, float latest_coeff,
                    const int* bands, int n_bands, const float* mean, const float* std_, int n_mfcc, double* acc,
                    float* out, float* per_seq, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------ streaming vocoder ---- */
/* The generator of this reference has causal resblocks; it looks ahead only through conv_pre's and conv_post's right
 * pad of 6 and through the transposed convs.  So output frame o (hop samples) depends on mel rows o - back ..
 * o + ahead only: the generator's REACH, a property of the config alone (interval propagation over rates, kernels
 * and dilations; m2s.config.generator_reach is the same rule).  The shipped config has reach (16, 7), resblock "2"
 * with dilations [1, 3] has (6, 7).  `ahead` rows is the algorithmic latency of streaming this model: 7 rows of 420
 * samples at 11413 Hz = 258 ms for the shipped config, whatever the hardware. */
int m2s_vocoder_reach(const m2s_vocoder* v, int* back, int* ahead);
/* One stateless chunk call, ADDITIVE (DESIGN.md "Streaming vocoder").  mel (rows, num_mels) ln-mel, packed as in the
 * ragged calls; `lengths`, `context`, `hold` are HOST arrays of B ints.  With G(x_b) = the generator on clip b's
 * lengths[b] rows as a whole clip (what m2s_vocoder_forward_ragged computes: both ends of the span are clip ends),
 * the call writes, packed in clip order,
 *     G(x_b)[context[b] * hop : (lengths[b] - hold[b]) * hop]
 * so wav has out_rows * hop samples, out_rows = sum(lengths[b] - context[b] - hold[b]).  Rows in context and hold
 * are read but get no output.  No state crosses a call.  The emitted rows are the rows of the WHOLE clip the span
 * was cut from if (context[b] >= back or the span starts at the clip's first row) and (hold[b] >= ahead or the span
 * ends at the clip's last row): keep the last back + ahead mel rows of a stream and every chunking of a clip gives
 * the whole clip's waveform (to rounding: a kernel's summation plan may depend on the row count).
 * Between stages the call drops the rows no emitted sample depends on (the cone; whole mel rows of every clip, on
 * the left only if every clip has context >= back, on the right only if every clip has hold >= ahead).  That
 * changes the work, never the contract; m2s_vocoder_set_chunk_cone(v, 0) turns it off, for tests and timing.
 * M2S_E_ARG, before any launch: B < 1, a length < 1, context[b] < 0, hold[b] < 0, context[b] + hold[b] >=
 * lengths[b], sum(lengths) != rows, null context or hold.  M2S_E_STATE if `stream` is capturing (the clip table is
 * staged per call, as in the ragged calls).  The workspace contract above applies as written; the query is exact to
 * the granule, and returns 0 for arguments the call would reject. */
int m2s_vocoder_set_chunk_cone(m2s_vocoder* v, int on);
size_t m2s_vocoder_chunk_workspace_bytes(const m2s_vocoder* v, const int* lengths, const int* context, const int* hold,
                                         int B);
int m2s_vocoder_forward_chunk(m2s_vocoder* v, const float* mel, const int* lengths, const int* context, const int* hold,
                              int B, int rows, float* wav, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------- Grad-CAM (autograd) path ---- */
/* compute_gradcam (scripts/mri_gradcam_formant.py:203-279) runs the model in train() and back-
 * propagates a mel-band power to the last feature map.  These entry points are that path, exact
 * fp32; every pointer is a device pointer on the current HIP device unless stated otherwise. */
typedef struct m2s_cam m2s_cam;
/* Packs the backbone part of an acoustic state dict (cnn.backbone.*) with unfolded BatchNorms:
 * raw conv weights, BN gamma / beta.  Synchronous. */
int m2s_cam_create(const m2s_tensor* sd, int n, int device, m2s_cam** out);
void m2s_cam_destroy(m2s_cam* c);
/* BatchNorm layers in state-dict order (conv_stem's bn1, then bn1 / bn2 / bn3 of every block) and
 * their channel counts: m2s_cam_backbone writes [mean C | biased var C] per layer, in that order. */
int m2s_cam_bn_layers(const m2s_cam* c);
int m2s_cam_bn_channels(const m2s_cam* c, int layer);
size_t m2s_cam_workspace_bytes(const m2s_cam* c, int N, int H, int W);
/* frames (N,H,W) fp32 -> the five timm feature maps with train-mode BatchNorm (statistics of the N
 * frames), taps[i] (N,C_i,OH_i,OW_i) fp32 (C = 16, 32, 56, 120, 208 at strides 2..32; a NULL entry
 * is skipped), and every BN layer's batch statistics into bn_stats. */
int m2s_cam_backbone(m2s_cam* c, const float* frames, int N, int H, int W, float* const* taps, float* bn_stats,
                     void* ws, size_t ws_bytes, void* stream);
/* nn.LSTM(C, H, bidirectional, batch_first) + sum merge with saved activations.  w[8] = w_ih, w_hh,
 * b_ih, b_hh of the forward direction, then of the reverse one (nn.LSTM layouts).  x (B,T,C) ->
 * y (B,T,H); gates (2,B,T,4H) post-activation i,f,g,o, cells / hid (2,B,T,H) kept for the backward. */
size_t m2s_bilstm_train_workspace_bytes(int B, int T, int C, int H);
int m2s_bilstm_train_forward(const float* x, int B, int T, int C, int H, const float* const* w, float* y,
                             float* gates, float* cells, float* hid, void* ws, size_t ws_bytes, void* stream);
/* Backward through time: dy (B,T,H) -> dx (B,T,C) and grads[6] = d w_ih, d w_hh, d bias (= d b_ih =
 * d b_hh) of the forward direction, then of the reverse one; any output may be NULL. */
int m2s_bilstm_train_backward(const float* x, const float* dy, int B, int T, int C, int H, const float* const* w,
                              const float* gates, const float* cells, const float* hid, float* dx, float* const* grads,
                              void* ws, size_t ws_bytes, void* stream);
/* y (rows,out) = x (rows,in) w^T + b (b may be NULL); backward dx = dy w, dw = dy^T x, db = sum dy. */
int m2s_linear_forward(const float* x, int rows, int in, int out, const float* w, const float* b, float* y,
                       void* stream);
int m2s_linear_backward(const float* dy, const float* x, int rows, int in, int out, const float* w, float* dx,
                        float* dw, float* db, void* stream);
/* mean over the last P elements of nc rows (NCHW maps: nc = N*C, P = H*W) and its backward. */
int m2s_gap_forward(const float* x, int64_t nc, int p, float* y, void* stream);
int m2s_gap_backward(const float* dy, int64_t nc, int p, float* dx, void* stream);

/* ------------------------------------------------------------- Grad-CAM engine ---- */
/* compute_gradcam for every formant band and every target frame of one clip in one call:
 * what main() of scripts/mri_gradcam_formant.py does per band (:407-426), compute_gradcam (:203-279) with
 * _forward_with_features (:128-166) and _compute_cam_from_grads (:169-200).  Exact fp32.  The K = n_bands *
 * (1 + n_frames) targets share one train-mode forward; target k = band * (1 + n_frames) + j is the whole-clip
 * band power for j = 0 and the band power of frame frame_idx[j - 1] for j >= 1.  Their cotangents go through
 * the backward together, m2s_gradcam_chunk() at a time.  One clip per call, as the reference's helper. */
typedef struct m2s_gradcam m2s_gradcam;
/* Packs cnn.backbone.* like m2s_cam_create and keeps rnn.lstm.* and head.* as fp32.  Synchronous. */
int m2s_gradcam_create(const m2s_tensor* sd, int n, int device, m2s_gradcam** out);
void m2s_gradcam_destroy(m2s_gradcam* g);
/* rows of head.weight */
int m2s_gradcam_n_mels(const m2s_gradcam* g);
/* floats of bn_stats: [mean C | biased var C] per BatchNorm layer, the layers of m2s_cam_bn_layers */
int m2s_gradcam_bn_stats_floats(const m2s_gradcam* g);
/* cotangents per backward pass (a compile-time constant): a call runs T * ceil(K / chunk) step launches */
int m2s_gradcam_chunk(void);
/* 0 for arguments the call would reject.  Proportional to min(K, chunk) * T: past K = chunk only the staged
 * frame-index table (n_frames ints) grows. */
size_t m2s_gradcam_workspace_bytes(const m2s_gradcam* g, int T, int H, int W, int n_bands, int n_frames);
/* frames (T,H,W) fp32 in [0,1], mean / std (n_mels) the scaler, all device memory.  band_mask (n_bands,n_mels)
 * of 0 / 1 and frame_idx (n_frames; may repeat, any order) are HOST arrays.  reduction 0 = mean, 1 = sum (:243-247).
 * Outputs: heat_seq (n_bands,T,H,W): frame t under the whole-clip target; heat_frame (n_bands,n_frames,H,W):
 * frame frame_idx[j] under its own target (NULL allowed when n_frames = 0); optional (NULL to skip) pred_norm
 * (T,n_mels), dpooled (K,T,C = 208) = d target_k / d pooled features (feats.grad = dpooled / (h w), constant
 * over a channel's positions), bn_stats as m2s_cam_backbone writes them.
 * M2S_E_ARG, before any launch: T < 1, a frame smaller than 32 x 32, n_bands < 1, an index outside [0, T), a mask
 * entry other than 0 / 1, a band with no bin set, an undersized workspace.  M2S_E_STATE on a capturing stream
 * (the tables are staged per call). */
int m2s_gradcam_forward(m2s_gradcam* g, const float* frames, int T, int H, int W, const float* mean, const float* std_,
                        const float* band_mask, int n_bands, const int* frame_idx, int n_frames, int reduction,
                        float* heat_seq, float* heat_frame, float* pred_norm, float* dpooled, float* bn_stats,
                        void* ws, size_t ws_bytes, void* stream);
/* Stage: the targets' gradients with respect to pred_norm (:230-247, :254-266 differentiated), every pointer
 * device memory (band_mask, frame_idx too): dpred (K,T,n_mels),
 *   dpred[k,t,m] = s_k(t) ln10/10 std[m] 10^((pred std + mean)[t,m] / 10) mask[band,m],
 * s_k(t) = 1/T (mean) or 1 (sum) for j = 0, [t == frame_idx[j-1]] for j >= 1. */
int m2s_gradcam_cotangents(const float* pred_norm, int T, int n_mels, const float* mean, const float* std_,
                           const float* band_mask, int n_bands, const int* frame_idx, int n_frames, int reduction,
                           float* dpred, void* stream);
/* Stage: K cotangents dy (K,T,H) through the backward of one saved sequence (gates (2,1,T,4H), cells (2,1,T,H)
 * from m2s_bilstm_train_forward with B = 1; w[8] as there) -> dx (K,T,C); what K loss.backward() calls leave
 * in the LSTM input's .grad (:247-248, :262-266), without the weight gradients.  H % 16 == 0.  dx[k] is
 * bit-identical whatever K and k's position; an all-zero cotangent gives exactly zero.  The query returns 0 for
 * arguments the call would reject and stops growing at K = m2s_gradcam_chunk(). */
size_t m2s_bilstm_train_backward_multi_workspace_bytes(int K, int T, int C, int H);
int m2s_bilstm_train_backward_multi(const float* dy, int K, int T, int C, int H, const float* const* w,
                                    const float* gates, const float* cells, float* dx, void* ws, size_t ws_bytes,
                                    void* stream);
/* Stage: _compute_cam_from_grads (:169-200) for M maps.  feats (N,C,h,w), weights (M,C) (the spatial mean of the
 * gradient), frame (M) device ints into N -> out (M,H,W): relu(sum_c weights[m,c] feats[frame[m],c]), bilinear
 * resize (align_corners=False), (v - min) / ((max - min) + 1e-6) over the resized map.  Any h, w, H, W whose
 * source map, weights and sample tables fit 64 KB of LDS; a frame outside [0, N) gives an all-zero map. */
int m2s_cam_heatmap(const float* feats, int N, int C, int h, int w, const float* weights, const int* frame, int M,
                    int H, int W, float* out, void* stream);

/* ------------------------------------------------ analysis: waveform -> mel ---- */
/* The opposite direction of the vocoder: wav (B,L) -> mel, exact fp32 (an f32-MFMA DFT with float64-built
 * tables, the spectrum kept on chip; DESIGN.md "Mel-spectrogram front end").  The mel basis is the caller's: the
 * engine does not know what a mel scale is. */
typedef struct m2s_melspec_cfg {
  int n_fft;     /* even, 16..4096 */
  int hop;       /* >= 1 (<= n_fft with pad = 1) */
  int win;       /* 1..n_fft, periodic Hann centred in the frame */
  int n_mels;    /* 1..128 */
  int pad;       /* 0 none: T = 1 + (L - n_fft)/hop;  1 reflect by (n_fft - hop)/2 (integer division) each side */
  int power;     /* 1: sqrt(re^2 + im^2 + 1e-9);  2: re^2 + im^2 */
  int out;       /* 0 ln(max(m,1e-5));  1 10*log10(max(m,1e-10));  2 linear */
  float preemph; /* 0 off; y[0] = x[0], y[n] = x[n] - c*x[n-1], applied before padding */
} m2s_melspec_cfg;
typedef struct m2s_melspec m2s_melspec;
/* mel_basis_host (n_mels, n_fft/2+1) fp32 row-major HOST memory, copied.  M2S_E_ARG for a config outside the
 * ranges above.  Synchronous. */
int m2s_melspec_create(const m2s_melspec_cfg* cfg, const float* mel_basis_host, int device, m2s_melspec** out);
void m2s_melspec_destroy(m2s_melspec* m);
/* the config's n_mels (what a caller holding only the handle needs to size `mel`) */
int m2s_melspec_n_mels(const m2s_melspec* m);
/* T for clips of L samples (trailing samples that do not fill a frame are ignored), or 0 where forward refuses L:
 * L < n_fft with pad = 0; a reflect pad >= L or a padded length < n_fft with pad = 1. */
int m2s_melspec_frames(const m2s_melspec* m, int L);
/* 0 for arguments forward would reject.  The workspace holds the partial mel sums over the bins; how many there
 * are per frame, and so the order in which a frame is summed, follows from the config alone, never from B or L. */
size_t m2s_melspec_workspace_bytes(const m2s_melspec* m, int B, int L);
/* wav (B,L) fp32 -> mel fp32, layout 0 = (B,n_mels,T), 1 = (B,T,n_mels).  M2S_E_ARG, before any launch, if
 * B < 1 or m2s_melspec_frames(m, L) is 0.  A clip's result does not depend on B or on its place in the batch. */
int m2s_melspec_forward(m2s_melspec* m, const float* wav, int B, int L, float* mel, int layout, void* ws,
                        size_t ws_bytes, void* stream);

/* ---------------------------------------------- fine-tuning: BiLSTM and mel head ---- */
/* One optimisation step of OTNLikeTrainer.train_epoch (train_mri_acoustic_model.py) for one batch and one
 * micro-batch, restricted to rnn.lstm.* and head.* with cnn.* frozen in eval mode (DESIGN.md "Fine-tuning"): the
 * caller passes cached encoder features.  fp32 throughout (no autocast, no GradScaler), rnn_hidden = 640.
 * Inputs are packed as in the pair calls: feats (rows,208) of B clips, lengths[B] on the HOST, target (rows,n_mels)
 * standardised dB mels and mask (rows) floats (NULL = ones) PER FRAME ROW; pair p, row s is window i, frame i + s
 * of its clip, P = sum(lengths[b] - window + 1) pairs in pass3_save_pairs order.  The calls gather targets and masks.
 * Forward: nn.LSTM(208, 640, bidirectional) from zero state on every window, sum merge, Dropout(p) with scale
 * 1 / (1 - p), Linear(640, n_mels).  Criterion: LOSS of m2s_mel_metrics on (P,window,n_mels) as ONE group, with the
 * freq_w / time_w / coefficients of the last m2s_finetune_set_hyper.  Backward: exact gradients of the 10 tensors,
 * in this order everywhere below: weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, the same four with the
 * _reverse suffix, head.weight, head.bias (bias_ih and bias_hh get equal gradients and separate moments).
 * clip_grad_norm_: coef = min(1, max_norm / (norm + 1e-6)) over the 10 tensors, skipped when max_norm <= 0.
 * torch.optim.AdamW(lr, (0.9, 0.999), 1e-8, weight_decay) on all 10: p *= 1 - lr wd, moments, bias-corrected
 * update, step count from 1.
 * Dropout mask: element e of (P,window,640) at optimiser step t (the step this update is, counted from 1) is kept
 * iff mix(e, seed, t) >= floor(p 2^32), mix = the 32-bit integer hash of DESIGN.md "Fine-tuning"; the backward
 * regenerates it.  p = 0 keeps every element and multiplies nothing.
 * A step reads nothing back to the host.  Every reduction has a fixed partition and order and there are no
 * floating-point atomics, waits or flags: equal inputs and state give equal bits.
 * Capture: the window table of (lengths, window) is staged by the first call that sees them; after one eager
 * m2s_finetune_step / m2s_finetune_forward, calls with the same lengths and window can be captured (one linear
 * chain of launches) and a replay advances the device step count and the dropout stream as an eager step does.  A
 * staged table keeps its device address until m2s_finetune_destroy, so eager calls with other lengths between two
 * replays (each staging a table of its own, P + 3 rows ints) leave a captured step valid.  A capturing call with a
 * table that is not staged returns M2S_E_STATE, and so does m2s_finetune_set_hyper on a capturing stream.
 * M2S_E_ARG, before any launch: a null handle, feats, target, lengths or ws; the pair calls' argument errors (window
 * outside 1..16, a lengths[b] < window, B < 1, sum(lengths) != rows); a window other than the last set_hyper's (or
 * no set_hyper yet); an undersized workspace.  The workspace contract above applies as written. */
typedef struct m2s_finetune m2s_finetune;
typedef struct m2s_finetune_hyper {
  float lr, weight_decay, max_norm, dropout; /* dropout in [0, 1) */
  unsigned seed;
  float delta_coeff, accel_coeff, latest_coeff;
} m2s_finetune_hyper;
enum { M2S_FT_TENSORS = 10, M2S_FT_SLOTS = 8 };
/* Takes rnn.lstm.* and head.* from a full or partial state dict (a missing one: M2S_E_ARG naming it); 1 <= n_mels
 * <= 256.  Moments and step count start at zero.  Synchronous. */
int m2s_finetune_create(const m2s_tensor* sd, int n, int n_mels, int device, m2s_finetune** out);
void m2s_finetune_destroy(m2s_finetune* ft);
int m2s_finetune_n_mels(const m2s_finetune* ft);
/* Host values -> the device hyper-parameter block, stream-ordered: freq_w[n_mels], time_w[window] host arrays. */
int m2s_finetune_set_hyper(m2s_finetune* ft, const m2s_finetune_hyper* h, const float* freq_w, const float* time_w,
                           int window, void* stream);
/* Exact size for m2s_finetune_step AND for m2s_finetune_forward: the forward call takes the step's layout, so either
 * call refuses a workspace 256 bytes smaller.  0 for arguments the calls reject. */
size_t m2s_finetune_workspace_bytes(const m2s_finetune* ft, const int* lengths, int B, int window);
/* out_slots (device, M2S_FT_SLOTS floats, may be NULL): LOSS, MSE, MAE, DELTA, ACCEL, LATEST of the batch BEFORE the
 * update (train-mode predictions), the gradient norm before clipping, coef. */
int m2s_finetune_step(m2s_finetune* ft, const float* feats, const float* target, const float* mask, const int* lengths,
                      int B, int rows, int window, float* out_slots, void* ws, size_t ws_bytes, void* stream);
/* Predictions mel_norm (P,window,n_mels) with dropout on (train != 0: the mask of the next step) or off; no update. */
int m2s_finetune_forward(m2s_finetune* ft, const float* feats, const int* lengths, int B, int rows, int window,
                         int train, float* mel_norm, void* ws, size_t ws_bytes, void* stream);
/* The last step's gradients before clipping -> grads10[i] (device, the tensor's shape; an entry may be NULL). */
int m2s_finetune_grads(m2s_finetune* ft, float* const* grads10, void* stream);
/* Parameters, first and second moments (device arrays of the tensors' shapes) and the step count (device int64);
 * any pointer, and any entry of an array, may be NULL. */
int m2s_finetune_export(m2s_finetune* ft, float* const* params10, float* const* m10, float* const* v10, int64_t* step,
                        void* stream);
/* The inverse of the export's m, v and step (device pointers), for resuming; m10 and v10 non-NULL with 10 entries. */
int m2s_finetune_import_moments(m2s_finetune* ft, const float* const* m10, const float* const* v10,
                                const int64_t* step, void* stream);

/* -------------------------------------------------------------------- profiling ---- */
/* While enabled, every kernel launch is bracketed by HIP events on its own stream. */
typedef struct m2s_prof_stat {
  char name[96];     /* kernel symbol family, e.g. "conv_igemm<bf16,conv2d,2x4>" */
  int64_t launches;
  double ms;         /* summed event time */
  double flops;      /* summed algorithmic FLOPs */
  double bytes;      /* summed algorithmic HBM bytes (compulsory in + out + weights) */
} m2s_prof_stat;
int m2s_prof_enable(int on);
/* Synchronises on the recorded events, writes up to `max` stats, clears the record. */
int m2s_prof_collect(m2s_prof_stat* out, int max, int* n_out);
/* One recorded launch, in launch order: its kernel name, the stage of the path it belongs to
 * ("cnn", "bilstm", "head", "glue", "voc_pre", "ups_c<C>", "mrf_c<C>", "voc_post", "melspec"; bench.py's
 * roofline.stages), event time, algorithmic FLOPs and bytes (compulsory in + out + weights of the
 * operation the kernel implements), and spill_bytes: an intermediate map the kernel writes only for a
 * later kernel of the same operation to read back (ir_ws: the IR block's expanded depthwise map, which
 * the SE-gated conv_pwl reads; ABI 6), counted once, not part of `bytes`. */
typedef struct m2s_prof_launch {
  char name[96];
  char stage[24];
  double ms;
  double flops;
  double bytes;
  double spill_bytes;
} m2s_prof_launch;
/* Synchronises on the recorded events, writes up to `max` launches in launch order (*n_out = all of
 * them), clears the record.  out == NULL: *n_out = the number recorded, the record stays. */
int m2s_prof_launches(m2s_prof_launch* out, int max, int* n_out);

#ifdef __cplusplus
}
#endif

#endif /* M2S_H_ */
