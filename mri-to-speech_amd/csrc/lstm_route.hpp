// Which recurrence kernel a BiLSTM call (B sequences, hidden size H) runs: the batch limits of the one-launch
// kernels (lstm_persistent.hip) and the ladder that chooses between them, in one place.  Host code only (no HIP
// header): a plain C++ program can include it (tests/lstm_route_dump.cpp).  The .hip files size their LDS and
// hand-off buffers from these limits; Acoustic::lstm_recurrence launches what lstm_plan() returns.
#pragma once

#include "../../include/m2s.h"

namespace m2s {

constexpr int LSTM_H = 640;         // the hidden size every one-launch kernel (and lstm_window.hip) is built for
constexpr int LSTM_SMALL_B = 4;     // lstm_small's default batch limit and its narrow instantiation
constexpr int LSTM_SMALL_CAP = 8;   // its wide instantiation (Switches::lstm_small_b = 8 routes B <= 8 to it)
constexpr int LSTM_GRANULE_B = 16;  // lstm_x3g and lstm_mid end here: a granule sweep grows with B (lstm_plan)
constexpr int LSTM_LAUNCH_B = 64;   // sequences per launch of lstm_x3 / lstm_persistent (c in LDS); more: several

enum class LstmRoute { Step, Small, X3g, X3, Mid, Persistent };

// The epoch-tagged granule kernels hand h over in a buffer the engine owns and zeroes once (lstm_persistent.hip
// lstm_epoch); the others in the call's workspace, zeroed per launch.
constexpr bool lstm_engine_sync(LstmRoute r) { return r == LstmRoute::Small || r == LstmRoute::X3g; }

// The epoch rule of that buffer (lstm_persistent.hip lstm_epoch queries the stream and issues the zeroing; the
// decision is here, host arithmetic only, and tests/test_lstm_epoch_cpu.py enumerates it).  A launch with epoch ep
// and length T publishes tag ep + s + 1 at step s < T - 1 into parity slot s & 1, accepts at step s >= 1 a granule of
// slot (s - 1) & 1 whose tag EQUALS ep + s, and marks a timeout with ep + 1; steps 1 and 2 read slots the launch has
// not rewritten yet.  So a launch that does not zero the buffer itself needs every tag and mark that an earlier eager
// launch, or a replay of any graph captured so far, can have left to be below ep + 1:
//  * eager: ep = count, count += T + 1 (an eager launch leaves tags <= ep + T - 1 and the mark ep + 1);
//  * under capture the zeroing is only RECORDED: the launch is recorded with ep = 0 behind it, and every replay
//    leaves tags <= T - 1 and the mark 1, whenever it runs.  The count is raised to at least T + 1 and never
//    lowered, so later eager epochs stay above all of them (the buffer itself is untouched at capture time: a
//    restart of the count there would let the next eager launch meet the tags of the eager launches before it);
//  * first use (count 0; the constructor zeroes the buffer too): zero, ep = 0, count = T + 1;
//  * at the wrap guard (count > LSTM_EPOCH_WRAP - T) the count cannot restart either, for a graph captured earlier
//    may be replayed later: the launch zeroes the buffer, runs at ep = 0 and leaves the count where it is (its tags,
//    <= T - 1, are below it).  From there on the long calls of an engine pay a memset node each (~4.6 us); the
//    count gets there after 4.0e9 recurrence steps.
constexpr unsigned LSTM_EPOCH_WRAP = 0xF0000000u;

struct LstmEpoch {
  unsigned ep;     // the launch's epoch
  unsigned count;  // the engine's count after it
  bool zero;       // zero the buffer (ahead of the launch, on its stream) first
};

inline LstmEpoch lstm_epoch_rule(unsigned count, int T, bool capturing) {
  const unsigned span = (unsigned)T + 1u;
  if (capturing) return {0u, count > span ? count : span, true};
  if (count == 0) return {0u, span, true};
  if (count > LSTM_EPOCH_WRAP - (unsigned)T) return {0u, count, true};
  return {count, count + span, false};
}

// Switches' six lstm_* members (switches.hpp), as the engine read them
struct LstmSwitches {
  bool persistent, mid, x3, x3g;
  int small_b, mid_ch;
};

struct LstmPlan {
  LstmRoute route;
  int inst;          // Small: the 4- or 8-sequence instantiation; Mid: sequences per chunk, 4 / 8 / 16; else 0
  const char* name;  // the launch record
  int terms;         // the record's flops per weight and step: 2, or 3 for the three-term split products
  bool engine_sync;  // lstm_engine_sync(route)
};

inline LstmPlan lstm_plan_of(LstmRoute r, int inst = 0) {
  const char* const names[] = {"lstm_step_kernel", "lstm_small_kernel", "lstm_x3g_kernel",
                               "lstm_x3_kernel",   "lstm_mid_kernel",   "lstm_persistent_kernel"};
  const bool x3 = r == LstmRoute::X3g || r == LstmRoute::X3;
  return {r, inst, names[(int)r], x3 ? 3 : 2, lstm_engine_sync(r)};
}

// First match wins.  "split": every engine but the fp32 one (three bf16 MFMA terms over hi / lo operands).
inline LstmPlan lstm_plan(const LstmSwitches& w, int dtype, int B, int H) {
  const bool split = dtype != M2S_DT_F32;
  if (H != LSTM_H || !w.persistent) return lstm_plan_of(LstmRoute::Step);  // one launch per step (kernels.hip)
  if (B >= 1 && B <= w.small_b) return lstm_plan_of(LstmRoute::Small, B > LSTM_SMALL_B ? LSTM_SMALL_CAP : LSTM_SMALL_B);
  // 5..16 sequences (configs[4]'s 8 clips a GPU): the granule hand-off (lstm_persistent.hip lstm_x3g_kernel)
  if (split && w.x3 && w.x3g && B >= 1 && B <= LSTM_GRANULE_B) return lstm_plan_of(LstmRoute::X3g);
  // split engines above the small-batch kernel: 4.1 / 5.2 / 9.9 us per step at B = 8 / 16 / 64 against
  // lstm_mid's 7.2 / 11.9 and the f32 counter-barrier kernel's 24
  if (split && w.x3) return lstm_plan_of(LstmRoute::X3);
  // above 16 sequences every workgroup's sweep of B x 640 granules per step (sc1 loads, the exchange volume grows
  // with B) costs more than the counter barrier's plain loads of h (tools/lstm_bench.py,
  // profiles/r03f_lstm_ab.txt: B = 32 20.2 vs 18.3 us, B = 64 40.9 vs 24.7 us per step)
  if (w.mid && B > w.small_b && B <= LSTM_GRANULE_B) {
    // sequences per chunk: 4 up to B = 8 (two chunks at B = 8: the second one's sweep overlaps the first's dot
    // products; 6.5 us per step vs 8.6 at one chunk of 8), 8 above; mid_ch = 4 / 8 / 16 forces one for A/B runs
    const bool forced = w.mid_ch == 4 || w.mid_ch == 8 || w.mid_ch == 16;
    return lstm_plan_of(LstmRoute::Mid, forced ? w.mid_ch : (B <= 8 ? 4 : 8));
  }
  return lstm_plan_of(LstmRoute::Persistent);
}

}  // namespace m2s
