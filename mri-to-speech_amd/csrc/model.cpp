// What the engines share on the host: the weight arena, the validated shape and the clip table of a ragged call,
// and the pipeline calls' scratch.  The execution plans themselves are in acoustic_cnn.cpp (CNN), acoustic_rnn.cpp
// (BiLSTM + head, all call forms) and vocoder.cpp (HiFi-GAN generator).
#include "model.hpp"

#include <algorithm>
#include <cstring>

#include "plan_util.hpp"

namespace m2s {

void Arena::upload(int device) {
  M2S_HIP(hipSetDevice(device));
  M2S_HIP(hipMalloc(&dev_, host_.size() + 256));
  M2S_HIP(hipMemcpy(dev_, host_.data(), host_.size(), hipMemcpyHostToDevice));
  std::vector<uint8_t>().swap(host_);
}

Arena::~Arena() {
  if (dev_) (void)hipFree(dev_);
}

// ------------------------------------------------------------------------------------------
// Ragged batches (ragged.hip, DESIGN.md "Ragged batches")
RaggedDims ragged_dims(const int* lengths, int B, long rows) {
  M2S_CHECK(lengths && B >= 1, "ragged: at least one clip (lengths must not be empty)");
  RaggedDims d;
  d.B = B;
  d.Tmin = lengths[0];
  for (int b = 0; b < B; ++b) {
    M2S_CHECK(lengths[b] >= 1, "ragged: clip " + std::to_string(b) + " has length " + std::to_string(lengths[b]) +
                                   "; every length must be >= 1");
    d.N += lengths[b];
    d.Tmax = std::max(d.Tmax, lengths[b]);
    d.Tmin = std::min(d.Tmin, lengths[b]);
  }
  M2S_CHECK(d.N == rows, "ragged: sum(lengths) = " + std::to_string(d.N) + " but the packed input has " +
                             std::to_string(rows) + " rows");
  // the dense path counts its B x T rows in an int (the projection's M, the kernels' row indices)
  M2S_CHECK((double)B * d.Tmax <= 2147483647.0 && B <= 65535, "ragged: B x Tmax out of range");
  return d;
}

RaggedTable::~RaggedTable() {
  if (done_) (void)hipEventDestroy(done_);
  if (host_) (void)hipHostFree(host_);
}

void ragged_check_stream(hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  M2S_HIP(hipStreamIsCapturing(s, &cap));
  if (cap != hipStreamCaptureStatusNone)
    throw Error(M2S_E_STATE, "ragged calls cannot be captured into a graph (the clip table is staged per call)");
}

void RaggedTable::upload(const int* lengths, int B, int* dev, hipStream_t s) {
  std::vector<int> tab((size_t)2 * B);
  int off = 0;
  for (int b = 0; b < B; ++b) {
    tab[b] = off;
    tab[B + b] = lengths[b];
    off += lengths[b];
  }
  upload_ints(tab.data(), tab.size(), dev, s);
}

void RaggedTable::upload_ints(const int* src, size_t n, int* dev, hipStream_t s) {
  ragged_check_stream(s);
  if (!done_) M2S_HIP(hipEventCreateWithFlags(&done_, hipEventDisableTiming));
  M2S_HIP(hipEventSynchronize(done_));  // the previous call's copy has read the staging buffer
  if (cap_ < n) {
    if (host_) M2S_HIP(hipHostFree(host_));
    host_ = nullptr;
    cap_ = 0;
    M2S_HIP(hipHostMalloc(reinterpret_cast<void**>(&host_), n * sizeof(int), hipHostMallocDefault));
    cap_ = n;
  }
  std::memcpy(host_, src, n * sizeof(int));
  M2S_HIP(hipMemcpyAsync(dev, host_, n * sizeof(int), hipMemcpyHostToDevice, s));
  M2S_HIP(hipEventRecord(done_, s));
}

// ------------------------------------------------------------------------------------------
// Pipeline scratch (capi.cpp: the size queries and m2s_pipeline_forward(_ragged))
PipelineBufs pipeline_bufs(Workspace& ws, const Acoustic& a, const Vocoder& v, int B, int T, int H, int W) {
  const size_t rows = (size_t)B * T;
  PipelineBufs b{};
  b.mn = ws.take<float>(rows * a.n_mels());
  b.ln_t = ws.take<char>(rows * chan_stride(a.n_mels()) * 4);
  b.rest_bytes = std::max(a.workspace_bytes(B, T, H, W), v.workspace_bytes(B, T));
  b.rest = ws.take<char>(b.rest_bytes);
  return b;
}

PipelineBufs pipeline_ragged_bufs(Workspace& ws, const Acoustic& a, const Vocoder& v, const int* lengths, int B, int H,
                                  int W) {
  PipelineBufs b{};
  b.rest_bytes = std::max(a.ragged_workspace_bytes(lengths, B, H, W), v.ragged_workspace_bytes(lengths, B));
  b.mn = ws.take<float>((size_t)sum_lengths(lengths, B) * a.n_mels());
  b.rest = ws.take<char>(b.rest_bytes);
  return b;
}

}  // namespace m2s
