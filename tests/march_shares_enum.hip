// Host program of tests/test_march_shares_cpu.py: every piece that MarchShares (csrc/march_common.h) hands to every wave, for
// the note march's and the onset march's cuts, as lines `cuts n_windows total_waves wave ws T0 T1`.  No HIP call.
#include <cstdio>

#include "march_common.h"

template <int kCut1, int kCut2, int kCut3>
static void enumerate(int cuts, int n_windows, int total_waves) {
  constexpr int kStrips = 3;
  for (int gw = 0; gw < total_waves; ++gw) {
    bp::MarchShares<kStrips, kCut1, kCut2, kCut3> shares(gw, total_waves, n_windows * kStrips);
    int ws, T0, T1;
    while (shares.next(ws, T0, T1)) std::printf("%d %d %d %d %d %d %d\n", cuts, n_windows, total_waves, gw, ws, T0, T1);
  }
}

int main() {
  const int windows[] = {1, 2, 3, 5, 256};
  for (int n : windows) {
    const int waves[] = {4, 8, 12, 64, 8 * n, 2048};
    for (int i = 0; i < 6; ++i) {
      const int tw = waves[i];
      if ((i == 4 && (tw == 4 || tw == 8 || tw == 12 || tw == 64)) || (i == 5 && tw == waves[4])) continue;  // listed twice
      enumerate<68, 133, 151>(0, n, tw);  // note_march16.hip
      enumerate<64, 129, 150>(1, n, tw);  // onset_march16.hip
    }
  }
  return 0;
}
