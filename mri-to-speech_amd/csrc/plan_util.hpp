// Small helpers shared by the execution-plan files (acoustic_cnn.cpp, acoustic_rnn.cpp, vocoder.cpp, model.cpp):
// the per-instantiation engine traits and the ConvArgs builders.  (The M2S_* switches: switches.hpp.)  Internal:
// model.hpp stays the header everything else includes.
#pragma once

#include <type_traits>

#include "pack.hpp"

namespace m2s {

// Which engine a plan template runs for, from its activation type T alone.  dispatch_act (model.hpp) instantiates
// bf16_t only for the bf16 and fp8 engines, sp_t only for bf16x3 and float only for fp32, so no plan needs a dtype_
// test beside these: the bf16 / split-only fused kernels are open to exactly the engines that are kNotF32.
template <class T>
constexpr bool kSplit = std::is_same<T, sp_t>::value;
template <class T>
constexpr bool kNotF32 = !std::is_same<T, float>::value;
// bytes an activation element takes in memory (split fp32: hi + lo planes)
template <class T>
constexpr size_t kStoreBytes = sizeof(T) * Elem<T>::R;

// packed rows of a ragged call's clips (lengths may be null in a size query: ragged_dims then raises)
inline long sum_lengths(const int* lengths, int B) {
  long n = 0;
  for (int b = 0; lengths && b < B; ++b) n += lengths[b];
  return n;
}

// a 1x1 conv as a GEMM over `rows` rows, P of them an image (the SE convs: one row an image)
inline ConvArgs pw_args(const PConv& pc, const void* x, void* y, int rows, int P) {
  ConvArgs a = conv_args(pc);
  a.x = x;
  a.y = y;
  a.M = rows;
  a.OH = P;
  return a;
}

}  // namespace m2s
