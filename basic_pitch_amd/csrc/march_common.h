// What the wave-private marches (note_march16.hip, onset_march16.hip, conv_contour_march.hip, the 32x32x16 forms kept for
// A/B runs) share beside their arithmetic and their LDS layouts: the fence around a wave's LDS image, the order in which
// workgroups take their work, the cut of the frames into shares, the launchers' grid.  The block order and the cut are
// TEXT that a kernel expands in place: as functions (forced inline or not; the cut as `bool next()`, as `done()` +
// `take()`, as a loop calling the body back) they moved the compiler's block layout and register allocation of the march
// around them, and a march's device code does not move for a helper's sake (tools/kernel_digest.py).
#pragma once
#include "bp_common.h"

namespace bp {

// A wave's LDS image (ring of rows, row image) is written lane-private and read across lanes: this fence orders the two.
// It waits for the writes it orders, so where it stands decides its cost: right behind a commit it exposes the LDS write
// latency once per row.  The marches put it in front of the first read of the committed row, with matrix work between —
// onset: three k-steps (the row committed at the end of step r is first read by k-step 4 of step r + 1); note: at the
// start of the next step (k-step 1 reads the row committed in the middle of the last); contour: at the END of a row step,
// a row of matrix work behind the commit into the other buffer — and once before a new piece's prologue overwrites the image.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The workgroup's logical block in the XCD-aware order: workgroups go to the 8 XCDs round-robin (blockIdx % 8) and each
// XCD has its own L2; consecutive pieces of work — the strips (and chunks) of ONE window, which read overlapping parts of
// the same zp rows — are given to workgroups of the same XCD, so a row is fetched from HBM by one L2 instead of by up to
// eight.  Inside each half of the grid: a CU hosts workgroups p and p + gridDim.x / 2, and when the pieces per wave are no
// whole number the first half of the LOGICAL blocks carries the extra piece — the pair of a CU stays (first, second half).
#define BP_XCD_LOGICAL_BLOCK()                                                                                     \
  ({                                                                                                               \
    const int half_n = (int)gridDim.x / 2, pq = (int)blockIdx.x % (half_n > 0 ? half_n : 1);                       \
    (gridDim.x % 16 == 0) ? ((int)blockIdx.x / half_n) * half_n + (pq % 8) * (half_n / 8) + pq / 8 : (int)blockIdx.x; \
  })

// The pieces (ws, T0, T1) — frames [T0, T1) of (window, strip) pair ws — of wave gw of total_waves over n_ws pairs of
// kFrames frames, 3 strips per window: every wave takes an equal share of the frames as at most two marches.
//  * exactly 8 waves per window (full batches: 2048 waves, 256 windows; 3 strips x 172 frames = 8 x 64.5): waves 0-2 of
//    a window march frames 0 .. kCut1 of strips 0, 1, 2, waves 3-5 frames kCut1 .. kCut2, wave 6 the rest of strip 0 and
//    kCut2 .. kCut3 of strip 1, wave 7 the rest of strips 1 and 2 — 1.25 pieces per wave, and the three strips of a frame
//    range, which read the SAME input rows, are marched at the same time by neighbouring waves of one workgroup;
//  * any other wave count: the pairs laid end to end, wave g of G takes the g-th G-th (a share may span several pairs).
// _STATE declares the wave's state; _TAKE, inside `for (int pi = 0;; ++pi) { int ws, T0, T1;`, sets the piece or LEAVEs.
#define BP_MARCH_SHARES_STATE(gw, total_waves, n_ws, kStrips)                                                      \
  const bool aligned = (total_waves) == 8 * ((n_ws) / (kStrips)); /* wave-uniform */                               \
  const int b8 = (gw) >> 3, j8 = (gw) & 7;                                                                         \
  const int64_t total = (int64_t)(n_ws) * kFrames;                                                                 \
  int64_t F0 = total * (gw) / (total_waves); /* the end-to-end order's share */                                    \
  const int64_t F1 = total * ((gw) + 1) / (total_waves)
#define BP_MARCH_SHARES_TAKE(kStrips, kCut1, kCut2, kCut3, LEAVE)                                                  \
  if (aligned) {                                                                                                   \
    if (pi >= (j8 < 6 ? 1 : 2)) LEAVE;                                                                             \
    if (j8 < 6) {                                                                                                  \
      ws = (kStrips) * b8 + (j8 < 3 ? j8 : j8 - 3), T0 = j8 < 3 ? 0 : (kCut1), T1 = j8 < 3 ? (kCut1) : (kCut2);    \
    } else if (pi == 0) {                                                                                          \
      ws = (kStrips) * b8 + (j8 - 6), T0 = j8 == 6 ? (kCut2) : (kCut3), T1 = kFrames;                              \
    } else {                                                                                                       \
      ws = (kStrips) * b8 + (j8 - 5), T0 = (kCut2), T1 = j8 == 6 ? (kCut3) : kFrames;                              \
    }                                                                                                              \
  } else {                                                                                                         \
    if (F0 >= F1) LEAVE;                                                                                           \
    ws = (int)(F0 / kFrames);                                                                                      \
    T0 = (int)(F0 - (int64_t)ws * kFrames);                                                                        \
    T1 = F1 - (int64_t)ws * kFrames < kFrames ? (int)(F1 - (int64_t)ws * kFrames) : kFrames;                       \
    F0 = (int64_t)(ws + 1) * kFrames;                                                                              \
  }

// The same text for the host (tests/test_march_shares_cpu.py): next() yields a wave's pieces in its march's order.
template <int kStrips, int kCut1, int kCut2, int kCut3>
struct MarchShares {
  int gw, total_waves, n_ws, pi = 0;
  int64_t taken = 0;  // frames of the end-to-end share that earlier pieces took
  __host__ __device__ MarchShares(int gw_, int total_waves_, int n_ws_) : gw(gw_), total_waves(total_waves_), n_ws(n_ws_) {}
  __host__ __device__ bool next(int& ws, int& T0, int& T1) {
    BP_MARCH_SHARES_STATE(gw, total_waves, n_ws, kStrips);
    F0 += taken;
    BP_MARCH_SHARES_TAKE(kStrips, kCut1, kCut2, kCut3, return false)
    taken = F0 - total * gw / total_waves;
    ++pi;
    return true;
  }
};

// Grid of a persistent march over n_ws pairs: `occ` workgroups per CU; small batches: waves of at least min_frames frames.
inline int march_grid(int n_ws, int min_frames, int waves_per_wg, int occ, int n_cu) {
  const int64_t waves = ((int64_t)n_ws * kFrames + min_frames - 1) / min_frames;
  const int grid = (int)((waves + waves_per_wg - 1) / waves_per_wg);
  return grid > occ * n_cu ? occ * n_cu : grid;
}

}  // namespace bp
