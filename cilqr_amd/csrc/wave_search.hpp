// Private to cilqr_amd/csrc: the joint search of one wavefront over the samples of a trajectory, shared by
// kernels_scene_window.hip and kernels_scene_predict.hip.  The rule's halving is a chain of log2 T dependent loads; here the
// wave's 64 lanes probe 64 evenly spaced samples of the remaining interval per round -- the last sample of each 1/64th --,
// one __ballot finds the first lane whose predicate holds and the interval becomes that lane's piece: three rounds for 10^5
// samples, two for 1501.  Every probed index lies in [0, T).
#pragma once
#include "dev_model.hpp"

namespace cilqr {

constexpr int kSwWave = 64;

// the first k of [0, T) with pred(k), T if there is none, for a predicate that is monotone in k; all 64 lanes call it with
// the same T (the ballots are the wave's)
template <class Pred>
CILQR_DEV int sw_wave_first(int T, int lane, Pred pred) {
  int a = 0, b = T;   // the answer lies in [a, b]; nothing in [0, a) holds
  while (b - a > kSwWave) {
    const int step = ((b - a - 1) >> 6) + 1;   // ceil((b - a) / 64): lane l probes the last sample of piece l
    const long long p = (long long)a + (long long)(lane + 1) * step - 1;
    const bool valid = p < b;
    const bool hit = valid && pred((int)p);
    const unsigned long long hits = __ballot(hit);
    if (hits != 0ull) {
      const int j = __ffsll(hits) - 1;   // the probes of the lanes below j are valid and do not hold
      b = a + (j + 1) * step - 1;
      a = a + j * step;
    } else {
      a = a + __popcll(__ballot(valid)) * step;   // past the last probe; <= b
    }
  }
  const int p = a + lane;
  const unsigned long long hits = __ballot(p < b && pred(p));
  return hits != 0ull ? a + (__ffsll(hits) - 1) : b;
}

}  // namespace cilqr
