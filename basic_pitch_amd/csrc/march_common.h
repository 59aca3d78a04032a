// What the wave-private marches (note_march16.hip, onset_march16.hip, conv_contour_march.hip, the 32x32x16 forms kept for
// A/B runs) share beside their arithmetic and their LDS layouts: the fence around a wave's LDS image, the order in which
// workgroups take their work, the cut of the frames into shares, the launchers' grid, the hand-over of the issue priority
// between the two waves of a SIMD, the tool builds' stamps.  The block order, the cut and the priority rule are
// TEXT that a kernel expands in place: as functions (forced inline or not; the cut as `bool next()`, as `done()` +
// `take()`, as a loop calling the body back) they moved the compiler's block layout and register allocation of the march
// around them, and a march's device code does not move for a helper's sake (tools/kernel_digest.py).
#pragma once
#include <cstring>

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

// Sharing the issue priority.  With both halves of the grid resident (gridDim.x == 2 n_cu) every SIMD holds one wave of
// the first half and one of the second, dispatched later.  At equal priority the older wave wins the vector-issue
// arbitration on every row, runs ahead and retires first; the younger one finishes alone, at the one-wave rate, and the
// launch waits for it (profiles/march_priority.md).  The rule `prio` (wave-uniform, from the launcher: march_prio) hands
// the arbitration over ONCE — no flip per row or k-step, which slows both waves:
//    0         no wave changes priority;
//    1 .. 99   a second-half wave raises its priority when it has marched that percentage of the rows of its own share,
//              counted over all its pieces, halo rows included;
//    -1        the same at half of EACH piece, back to 0 at the piece's end (A/B);
//    100, 101  the first / the second half runs at priority 1 from its first row (A/B).
// First-half waves never flip; a wave without rows never reaches _ROW.  The countdown lives in one scalar register.
// _ROWS (between _SHARES_STATE and the piece loop) counts the rows of the wave's share: `halo` rows per piece beside its
// frames; _STATE declares the countdown; _PIECE stands at the head of a piece, _ROW at the head of a row.
#define BP_MARCH_PRIO_SECOND_HALF() ((int)blockIdx.x >= (int)gridDim.x / 2)
#define BP_MARCH_PRIO_ROWS(prio, kStrips, kCut1, kCut2, kCut3, halo, rows)                                         \
  int rows = 0;                                                                                                    \
  if ((prio) > 0 && (prio) < 100 && BP_MARCH_PRIO_SECOND_HALF()) {                                                 \
    const int64_t F0_first = F0;                                                                                   \
    for (int pi = 0;; ++pi) {                                                                                      \
      int ws, T0, T1;                                                                                              \
      BP_MARCH_SHARES_TAKE(kStrips, kCut1, kCut2, kCut3, break)                                                    \
      (void)ws;                                                                                                    \
      rows += T1 - T0 + (halo);                                                                                    \
    }                                                                                                              \
    F0 = F0_first;                                                                                                 \
  }
#define BP_MARCH_PRIO_STATE(prio, rows)                                                                            \
  int prio_left = ((prio) > 0 && (prio) < 100 && BP_MARCH_PRIO_SECOND_HALF()) ? 1 + (rows) * (prio) / 100 : 0;     \
  if ((prio) >= 100 && ((prio) == 101) == BP_MARCH_PRIO_SECOND_HALF()) __builtin_amdgcn_s_setprio(1)
#define BP_MARCH_PRIO_PIECE(prio, piece_rows)                                                                      \
  if ((prio) < 0 && BP_MARCH_PRIO_SECOND_HALF()) {                                                                 \
    __builtin_amdgcn_s_setprio(0);                                                                                 \
    prio_left = 1 + (piece_rows) / 2;                                                                              \
  }
#define BP_MARCH_PRIO_ROW() \
  if (--prio_left == 0) __builtin_amdgcn_s_setprio(1)

// The rule of a launch: `adopted` (the kernel's measured choice) when both halves of the grid are resident, none otherwise.
// A/B library only: BP_MARCH_PRIO = off | 1 .. 99 | piece | first | second replaces every kernel's choice.
inline int march_prio(int adopted, int grid, int n_cu) {
  static const int forced = [] {
    const char* e = ab_env("BP_MARCH_PRIO");
    if (!e) return -2;
    if (strcmp(e, "off") == 0) return 0;
    if (strcmp(e, "piece") == 0) return -1;
    if (strcmp(e, "first") == 0) return 100;
    if (strcmp(e, "second") == 0) return 101;
    const int v = atoi(e);
    return v >= 1 && v <= 99 ? v : -2;
  }();
  return grid == 2 * n_cu ? (forced != -2 ? forced : adopted) : 0;
}

#ifdef BP_MARCH_PROF
// Tool builds only (tools/experiments/march_prof.py): 100 MHz stamps of EVERY wave of a launch of at most 512 workgroups,
// written by lane 0 as they are taken into a buffer of their own that no kernel reads: per wave [0] entry, [1] set-up
// done, [2 .. 5] end of piece 0 .. 3, [6] exit, [7] rows | pieces << 16 | XCC_ID << 20 | HW_ID << 32.  The wave's slot is
// its PHYSICAL place, 4 blockIdx.x + wave.  _READ defines the C function the tool fetches the last launch's stamps with.
#define BP_MARCH_PROF_BUF(name)                                                                                    \
  __device__ unsigned long long name[2048 * 8];                                                                    \
  extern "C" int name##_read(unsigned long long* dst) {                                                            \
    if (hipDeviceSynchronize() != hipSuccess) return -1;                                                           \
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(name), sizeof(name)) == hipSuccess ? 0 : -1;                        \
  }
#define BP_MARCH_PROF_ENTRY(name, wave)                                                                            \
  unsigned long long* const prof_rec = name + ((int)blockIdx.x * 4 + (wave)) * 8;                                  \
  const bool prof_on = (threadIdx.x & 63) == 0 && gridDim.x <= 512;                                                \
  int prof_rows = 0, prof_pieces = 0;                                                                              \
  if (prof_on) {                                                                                                   \
    prof_rec[0] = __builtin_amdgcn_s_memrealtime();                                                                \
    prof_rec[2] = prof_rec[3] = prof_rec[4] = prof_rec[5] = 0;                                                     \
  }
#define BP_MARCH_PROF_SETUP()                                                                                      \
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                      \
  if (prof_on) prof_rec[1] = __builtin_amdgcn_s_memrealtime()
#define BP_MARCH_PROF_ROW() ++prof_rows
#define BP_MARCH_PROF_PIECE_END()                                                                                  \
  if (prof_on && prof_pieces < 4) prof_rec[2 + prof_pieces] = __builtin_amdgcn_s_memrealtime();                    \
  ++prof_pieces
#define BP_MARCH_PROF_EXIT()                                                                                       \
  if (prof_on) {                                                                                                   \
    prof_rec[6] = __builtin_amdgcn_s_memrealtime();                                                                \
    prof_rec[7] = (unsigned long long)(unsigned)(prof_rows & 0xffff) | (unsigned long long)(prof_pieces & 15) << 16 | \
                  (unsigned long long)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 15) << 20 |                     \
                  (unsigned long long)(unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11)) << 32;                   \
  }
#else
#define BP_MARCH_PROF_BUF(name)
#define BP_MARCH_PROF_ENTRY(name, wave)
#define BP_MARCH_PROF_SETUP()
#define BP_MARCH_PROF_ROW()
#define BP_MARCH_PROF_PIECE_END()
#define BP_MARCH_PROF_EXIT()
#endif

// Grid of a persistent march over n_ws pairs: `occ` workgroups per CU; small batches: waves of at least min_frames frames.
inline int march_grid(int n_ws, int min_frames, int waves_per_wg, int occ, int n_cu) {
  const int64_t waves = ((int64_t)n_ws * kFrames + min_frames - 1) / min_frames;
  const int grid = (int)((waves + waves_per_wg - 1) / waves_per_wg);
  return grid > occ * n_cu ? occ * n_cu : grid;
}

}  // namespace bp
