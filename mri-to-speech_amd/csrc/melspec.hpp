// Waveform -> mel spectrogram on the device (melspec.hip; m2s_melspec_* in m2s.h).
#pragma once

#include <cstddef>

#include "../../include/m2s.h"
#include "m2s_common.hpp"

namespace m2s {

// Everything the kernels need that follows from the config alone.  The frame tile FT, the bin tiles a wave
// owns and so the number of partial mel sums P are fixed here, never by B or L: the summation order of a frame
// depends on the config only.
class MelSpec {
 public:
  MelSpec(const m2s_melspec_cfg& cfg, const float* mel_basis_host, int device);
  ~MelSpec();
  MelSpec(const MelSpec&) = delete;
  MelSpec& operator=(const MelSpec&) = delete;

  int device() const { return device_; }
  int n_mels() const { return c_.n_mels; }
  // frames of an L-sample clip, 0 where forward refuses L
  int frames(long L) const;
  size_t workspace_bytes(int B, long L) const;
  void forward(const float* wav, int B, long L, float* mel, int layout, void* ws, size_t ws_bytes, hipStream_t s) const;

 private:
  m2s_melspec_cfg c_;
  int device_ = 0;
  int pad_ = 0;      // reflect samples per side
  int bins_ = 0;     // n_fft / 2 + 1
  int nt_ = 0;       // 16-bin tiles
  int k0_ = 0;       // first K row kept (multiple of 16): rows where the window is zero are skipped
  int kb_ = 0;       // 16-row K blocks kept
  int ft_ = 0;       // frames per workgroup
  int mt_ = 0;       // 16-frame MFMA row tiles per workgroup
  int tpw_ = 0;      // bin tiles per wave
  int parts_ = 0;    // partial mel sums per frame = waves over the bins
  int nmt_ = 0;      // 16-mel column tiles (1, 2, 4 or 8)
  int span_ = 0;     // floats of waveform one workgroup stages
  float* dft_ = nullptr;    // [nt][kb][re | im][64 lanes][4 K steps]
  float* basis_ = nullptr;  // [nt][4 K steps][nmt][64 lanes]
};

}  // namespace m2s
