// The launch decisions of the dense path in one place: what each launcher of the default (split-precision) path derives
// from n_windows and the device's CU count — which kernel, which grid, how many chunks, slabs, items per workgroup — as
// inline host functions, with the constants they read.  The launchers call these functions; bp_launch_plan (bp_api.hip, the
// handle-free test hook of include/basic_pitch_amd.h) fills its struct from the same functions, so that
// tests/test_launch_plan_cpu.py can enumerate every regime of every batch size without a device and
// tests/test_gpu_launch_regimes.py can run the sizes on either side of every change.  march_grid and march_prio
// (march_common.h) are the note and the onset march's part of it.  Host code only — nothing here reaches a kernel's text
// except as the constants the kernels read before (tools/kernel_digest.py) — but for the layout of the fused contour
// march's partial sums (kCf*, cf_*), which its writer, its readers and the plan share as __host__ __device__ functions.
#pragma once
#include "march_common.h"

namespace bp {

// ---- cqt_planes_pyramid.hip
constexpr int kPlDecimateWaves = 4;  // waves (tiles in flight) per workgroup of pl_decimate_kernel
inline int pl_resident_waves(int n_cu) { return n_cu * 16; }
// With at least half a window per CU the whole pyramid is ONE launch, a workgroup per window (the 22.05 kHz kernel from
// a third: a 3-minute track is 110 windows, and the four wide launches it took below half the CUs cost 55 us where
// 110 workgroups of the per-window kernel take 40).
inline bool pyramid_one_launch(int n_windows, int n_cu, bool ext) {
  return ext ? n_windows >= n_cu / 2 : 3 * n_windows >= n_cu;
}
// Grid of one wide decimator launch over `tiles` tiles per window: four items per workgroup, within the resident waves.
inline int pyramid_decimate_grid(int tiles, int n_windows, int n_cu) {
  const int items = tiles * n_windows;
  int grid = (items + kPlDecimateWaves - 1) / kPlDecimateWaves;
  if (grid > pl_resident_waves(n_cu) / kPlDecimateWaves) grid = pl_resident_waves(n_cu) / kPlDecimateWaves;
  return grid;
}

// ---- cqt_planes_filterbank.hip
constexpr int kPlFbThreads = 1024;  // threads of a filterbank workgroup: 16 waves, a task each
// One window per workgroup pays from half a window per CU on.  (A file job's 110-window tracks on three lanes, round 5:
// with the fused form from 32 windows on, 1,258 files/s against 1,460 — a third of the CUs for 60 us is worse than all
// of them for 29 + 15 us even when other lanes' kernels could fill the rest.)
inline bool filterbank_fused(bool has_zp, int n_windows, int n_cu) { return has_zp && 2 * n_windows >= n_cu; }
// fused: workgroup g owns windows g, g + grid, ...; strided: `tasks` (window, level, tile) over the waves of the grid
inline int filterbank_grid(bool fused, int n_windows, int tasks, int n_cu) {
  int grid;
  if (fused) {
    grid = n_windows < n_cu ? n_windows : n_cu;
  } else {
    grid = (tasks + kPlFbThreads / 64 - 1) / (kPlFbThreads / 64);
    if (grid > n_cu) grid = n_cu;
  }
  return grid;
}

// ---- conv_contour_march.hip
constexpr int kCmWaves = 4;          // independent waves per workgroup
constexpr int kCmStrips = 7;         // 32-bin strips: bins 20 .. 243
#ifndef BP_CM_CHUNKS
#define BP_CM_CHUNKS 4
#endif
constexpr int kCmChunks = BP_CM_CHUNKS;  // frame chunks per window (4: 0.211 ms at B = 256; 8: 0.225 — twice the warm-up rows; 1: 0.227 —
                                         // 7 of a CU's 8 wave slots busy; same-box sweep at the end of round 4: 2 / 3 / 4 / 5 / 6
                                         // chunks = 0.225 / 0.227 / 0.201 / 0.210 / 0.215 ms)
constexpr int kCmMaxChunks = 32;     // what a small batch is cut into at the most
constexpr int kCmPrio = 0;           // march_common.h: no wave changes priority (profiles/march_priority.md)
// small batches: more, shorter chunks until there is a task per resident wave (a task is a serial march of rows: at
// one window, 4 chunks leave 28 waves marching 45 rows each while 2020 wave slots idle)
inline int contour_march_chunks(int n_windows, int n_cu) {
  int chunks = kCmChunks;
  while (chunks < kCmMaxChunks && (int64_t)n_windows * chunks * kCmStrips < (int64_t)2 * n_cu * kCmWaves) chunks *= 2;
  return chunks;
}
// two workgroups of four waves per CU (registers), persistent
inline int contour_march_grid(int n_tasks, int n_cu) {
  int grid = (n_tasks + kCmWaves - 1) / kCmWaves;
  if (grid > 2 * n_cu) grid = 2 * n_cu;
  return grid;
}

// ---- conv_contour_march.hip with conv2 in its epilogue, conv_contour2.hip contour_conv2_finish_kernel: what the fused
// march hands on instead of c1 (these functions are the kernels' text too: __host__ __device__).
// A position's c1 pixel pair is projected on (frame tap dt) x (output bin offset ob = -2 .. 3 relative to bin 2 p); the
// three offsets that meet in output bin 2 q + e — ob = e + 2 from position q - 1, e from q, e - 2 from q + 1 — are the
// classes 2, 1, 0.  A class sums its five frame taps in the order dt = 0 .. 4; an output column is then
// (class 2 of q - 1 + class 1 of q) + class 0 of q + 1.  Per (window, strip) and output row the march stores kCfCols columns:
// 32 of its own bins, then the two bins in front of the strip (class 0 of its first position) and the two behind it
// (class 2 of its last).  Where a chunk of frames begins at T0 > 0, the output rows T0 - 2 .. T0 + 1 have terms on both sides
// of the cut: the chunk in front stores what it has summed (kCfPrefRows prefixes), the chunk behind stores its terms one by
// one (kCfTermRows, cf_term_index), per class, and the finisher adds prefix + term + term in the same order — whatever the
// number of chunks, every output is the same sequence of additions.
constexpr int kCfCols = 36;
constexpr int kCfClassRow = 3 * 32;   // a seam row: [class][position n][e]
constexpr int kCfPrefRows = 4;        // output rows T0 - 2 .. T0 + 1
constexpr int kCfTermRows = 10;       // 1 + 2 + 3 + 4 terms of those rows
constexpr int kCfSeam = (kCfPrefRows + kCfTermRows) * kCfClassRow;            // floats per (seam, strip)
constexpr int kCfMain = kCmStrips * kFrames * kCfCols;                        // floats per window: [strip][row][col]
constexpr int kCfWin = kCfMain + (kCmMaxChunks - 1) * kCmStrips * kCfSeam;    // + [seam][strip] records
static_assert(kCfWin <= 8 * kPlaneC, "the partial sums of a window fit the exact-f32 path's c1 plane, which the default path leaves idle");
__host__ __device__ constexpr int cf_chunk_t0(int ci, int chunks) { return (ci * kFrames) / chunks; }
// the chunk that holds frame x
__host__ __device__ constexpr int cf_chunk_of(int x, int chunks) { return ((x + 1) * chunks - 1) / kFrames; }
// output row t lies on a seam (rows T0 - 2 .. T0 + 1 of a chunk ci >= 1): the chunk, and the row's index r = t - (T0 - 2)
__host__ __device__ inline bool cf_seam_of_row(int t, int chunks, int& ci, int& r) {
  const int x = t + 2 < kFrames - 1 ? t + 2 : kFrames - 1;
  ci = cf_chunk_of(x, chunks);
  const int T0 = cf_chunk_t0(ci, chunks);
  r = t - (T0 - 2);
  return ci >= 1 && T0 >= t - 1;
}
// seam row r holds the terms dt = 4 - r .. 4 of the chunk behind the cut
__host__ __device__ constexpr int cf_term_index(int r, int dt) { return r * (r + 1) / 2 + dt - (4 - r); }
__host__ __device__ constexpr int64_t cf_seam_offset(int ci, int strip) {
  return (int64_t)kCfMain + (int64_t)((ci - 1) * kCmStrips + strip) * kCfSeam;
}
// The projection's row 16 block + 4 gq + r is C register r of lane group gq = e + 2 s; slot = 4 block + r:
//   s = 0: slots 0 .. 4 = class 0 (ob = e - 2), dt = slot;  slots 5 .. 7 = class 1 (ob = e), dt = slot - 5
//   s = 1: slots 0 .. 4 = class 2 (ob = e + 2), dt = slot;  slots 5, 6 = class 1, dt = slot - 2;  slot 7 unused
__host__ __device__ inline bool cf_slot(int gq, int slot, int& dt, int& ob) {
  const int e = gq & 1, s = gq >> 1;
  if (slot < 5) {
    dt = slot, ob = s ? e + 2 : e - 2;
    return true;
  }
  dt = s ? slot - 2 : slot - 5, ob = e;
  return !(s && slot == 7);
}
// The finisher: a wave per (window, slab of frames), within the resident waves.  Two waves per SIMD (184 VGPRs: three rows
// of c1 AND of partial sums in flight per wave; at three waves per SIMD with the partial sums one row ahead the launch took
// 53.7 us in the trace against 44 - 45)
constexpr int kCfOcc = 2;
constexpr int kCfMaxSlabs = 16;
struct Conv2FinishLaunch {
  int n_slabs, slab_rows, grid;
};
inline Conv2FinishLaunch conv2_finish_launch(int n_windows, int n_cu) {
  Conv2FinishLaunch l;
  int n_slabs = (int)(((int64_t)n_cu * 4 * kCfOcc) / n_windows);
  n_slabs = n_slabs < 1 ? 1 : (n_slabs > kCfMaxSlabs ? kCfMaxSlabs : n_slabs);
  l.slab_rows = (kFrames + n_slabs - 1) / n_slabs;
  l.n_slabs = (kFrames + l.slab_rows - 1) / l.slab_rows;
  l.grid = (int)(((int64_t)n_windows * l.n_slabs + 3) / 4);
  return l;
}

// ---- conv_contour_rim_march.hip
constexpr int kRmTileFrames = 16;
constexpr int kRmTiles = (kFrames + kRmTileFrames - 1) / kRmTileFrames;  // 11
#ifndef BP_RM_DEPTH
#define BP_RM_DEPTH 4
#endif
constexpr int kRmDepth = BP_RM_DEPTH;        // items whose zp words are in flight (LDS-DMA)
constexpr int kRmRing = kRmDepth + 1;        // raw buffers
// one workgroup of ten waves per CU (168 VGPRs: three waves per SIMD), half of them per side; few windows: a workgroup
// per item and side
inline int rim_march_per_side(int n_items, int n_cu) {
  int per_side = n_cu / 2 > 0 ? n_cu / 2 : 1;
  if (per_side > n_items) per_side = n_items;
  return per_side;
}
// items of workgroup `wg` of a side (the kernel's n_my): wg, wg + per_side, ...
inline int rim_march_items_of(int wg, int n_items, int per_side) {
  return wg < n_items ? (n_items - wg + per_side - 1) / per_side : 0;
}

// ---- conv_contour2.hip
constexpr int kP2Group = 16;                         // windows per flat index group
constexpr int kP2Cols = kP2Group * kC1Row;           // 4288 flat columns per group
constexpr int kP2Strip = 64, kP2Stride = 60;         // columns a wave reads / stores per row
constexpr int kP2Strips = (kP2Cols + kP2Stride - 1) / kP2Stride;  // 72
#ifndef P2_OCC
#define P2_OCC 4
#endif
constexpr int kP2Occ = P2_OCC;  // resident waves per SIMD the launch is cut for (and the register budget allows)
constexpr int kP2PerLaunch = 256;   // windows per launch
constexpr int kP2MaxSlabs = 16;
struct Conv2ProjLaunch {
  int n;          // windows of this launch
  int n_groups;   // groups of kP2Group windows, the last one ragged when n is no multiple
  int n_slabs;    // frame slabs per window
  int slab_rows;  // frames per slab
  int grid;       // workgroups of four waves
};
inline int64_t conv2_proj_slots(int n_cu) { return (int64_t)n_cu * 4 * kP2Occ; }
// sub-batches of 256 windows, each cut into as many frame slabs as keep one launch within the resident waves:
// the launch that starts at window w0
inline Conv2ProjLaunch conv2_proj_launch(int n_windows, int w0, int n_cu) {
  Conv2ProjLaunch l;
  l.n = n_windows - w0 < kP2PerLaunch ? n_windows - w0 : kP2PerLaunch;
  l.n_groups = (l.n + kP2Group - 1) / kP2Group;
  int n_slabs = (int)(conv2_proj_slots(n_cu) / ((int64_t)l.n_groups * kP2Strips));
  n_slabs = n_slabs < 1 ? 1 : (n_slabs > kP2MaxSlabs ? kP2MaxSlabs : n_slabs);
#ifdef P2_SLABS  // tools only
  n_slabs = P2_SLABS;
#endif
  l.slab_rows = (kFrames + n_slabs - 1) / n_slabs;
  l.n_slabs = (kFrames + l.slab_rows - 1) / l.slab_rows;
  const int64_t waves = (int64_t)l.n_groups * l.n_slabs * kP2Strips;
  l.grid = (int)((waves + 3) / 4);
  return l;
}

// ---- note_march16.hip, onset_march16.hip: march_grid, march_prio (march_common.h) with
constexpr int kN16Waves = 4;    // independent waves per workgroup
constexpr int kN16Strips = 3;   // 32-pixel strips of a row, 30 inner pixels each
#ifndef N16_OCC
#define N16_OCC 2
#endif
constexpr int kN16Occ = N16_OCC;  // resident workgroups per CU (x 4 waves: waves per SIMD)
constexpr int kN16Prio = 45;      // march_common.h: a second-half wave takes the issue priority at 45 % of its rows
constexpr int kN16MinFrames = 12; // small batches: fewer waves, at least this many frames each
constexpr int kO16Waves = 4;      // independent waves per workgroup
constexpr int kO16Strips = 3;     // 32-pixel strips of a row, 30 inner pixels each
constexpr int kO16Occ = 2;        // resident workgroups per CU (LDS)
constexpr int kO16Prio = 45;      // march_common.h: a second-half wave takes the issue priority at 45 % of its rows
constexpr int kO16MinFrames = 6;
// What BP_MARCH_SHARES_STATE (march_common.h) decides on the device from the same two numbers, restated for the plan: the
// eight-waves-per-window cut, and whether an end-to-end share is longer than one (window, strip) pair.
inline bool march_aligned(int total_waves, int n_ws, int strips) { return total_waves == 8 * (n_ws / strips); }
inline bool march_share_spans_pairs(int total_waves, int n_ws, int strips) {
  return !march_aligned(total_waves, n_ws, strips) && n_ws > total_waves;
}

}  // namespace bp
