// The sequential half of note decoding on the device, for a job of many clips (bp_infer_clips_events /
// bp_note_events_from_maps, include/basic_pitch_amd_events.h): the tracker from the onset peaks, the melodia trick, the
// amplitude means and the bends per event — decode_core's candidate branch (csrc/note_decode.cpp), operation for operation.
//
// For one long track the tracker is a serial chain and a workgroup is slower than a host core.  For a job of clips the chains
// are independent: ONE WORKGROUP PER CLIP, hundreds of them on 256 compute units.  Inside a workgroup every decision is
// workgroup-uniform (every wave evaluates it on the same values), and only the wide parts are shared out: a wave scans 64
// frames of a pitch per ballot, the zeroing, the wipes and the argmax go over all 256 threads, amplitudes one event per lane.
//
// `energy`, the working copy of the clip's note rows that found notes are zeroed in, lies in LDS where the clip fits
// (kNoteTrackLdsRows rows) and in a scratch buffer of the handle where it does not.  Both forms run one body (nt_track), in the
// style of note_device.hip's kRing / linear templates.
//
// The LDS budget.  A compute unit has 160 KiB and runs floor(163840 / bytes per workgroup) workgroups.  A launch's dynamic LDS
// is the state of its longest clip plus the pairwise sum's stacks at the depth that length needs (nt_stack_depth), beside 32
// static bytes: a job of one-window clips (142 rows) takes 51,120 + 512 + 32 bytes, THREE workgroups per compute unit.  (With
// the stacks static at the depth of the longest clip the library takes, 5,120 bytes, the same job took 56,272 bytes: two.)
//
// The order contract.  Onset phase: frames T-2 ... 1, bins 87 ... 0, every set bit of the onset-peak bitmap in exactly that
// order, each seeing the zeroes of the notes before it.  Melodia phase: the argmax of `energy` over the clip, ties to the
// lowest flat index t * 88 + f, until the maximum is not above the frame threshold.  Events leave in the order found.
//
// Bit-exactness of the amplitudes.  np.mean in float32 is numpy's pairwise sum; here it is the same additions in the same
// order: a leaf of at most 128 values with eight accumulators, leaves joined left + right by an explicit stack in LDS (no
// device recursion, no indexed register array: the product library's kernels use no scratch).  Only float32 additions and one
// IEEE division are involved; `#pragma clang fp contract(off) reassociate(off)` below keeps the compiler from fusing or
// reordering any of them, whatever flags the library is built with, and HIP's float division is correctly rounded by default.
#include <algorithm>
#include <vector>

#include "bp_kernels.h"

#pragma clang fp contract(off)
#pragma clang fp reassociate(off)

namespace bp {

constexpr int kNtF = 88, kNtMidi = 21;
// words of working state per row: 88 cells of energy, the row's maximum, the lowest bin that holds it
constexpr int kNtRowWords = kNtF + 2;
constexpr int kNtStack = 10;  // bound of the pairwise sum's stack depth: 7 suffices for kNoteTrackMaxRows (m_d <= n / 2^d + 15)
static_assert(kNoteTrackLdsRows * kNtRowWords * 4 + 2 * kNtStack * 64 * 4 + 256 <= 160 * 1024, "LDS budget per workgroup");
static_assert((kNoteTrackMaxRows >> 7) + 15 <= 128, "depth 7 reaches a leaf");

// The deepest the stack of nt_mean gets over any n <= rows values (a note may span any part of a clip): a sum of n > 128 values
// is one level above the deeper of its two halves.  Not monotonic in n — 255 values split into 120 + 135 and need two levels,
// 256 into 128 + 128 and need one — so the answer is the running maximum.  At least 1: the stacks are never empty arrays.
static int nt_stack_depth(int64_t rows) {
  static const std::vector<uint8_t> upto = [] {
    std::vector<uint8_t> need(kNoteTrackMaxRows + 1, 0), most(kNoteTrackMaxRows + 1, 1);
    for (int n = 129; n <= kNoteTrackMaxRows; ++n) {
      const int n2 = n / 2 - (n / 2) % 8;
      need[n] = (uint8_t)(1 + std::max(need[n2], need[n - n2]));
      most[n] = std::max(most[n - 1], need[n]);
    }
    return most;
  }();
  return upto[(size_t)(rows < 0 ? 0 : (rows < kNoteTrackMaxRows ? rows : kNoteTrackMaxRows))];
}

struct NtEvent {
  int start, end, pitch;
  float amp;
};

// ---- the scan both phases share: steps j = 0 ... n - 1 visit row from + dir * j of bin f; k counts consecutive cells below
// the frame threshold.  The host loop `while (more && k < tol) { below ? ++k : k = 0; ++i; }` as (steps taken, final k): a wave
// takes 64 steps per ballot and walks the runs of the mask with scalar bit operations.  Every wave computes the same answer.
__device__ __forceinline__ void nt_scan(const float* energy, int f, int from, int dir, int n, int tol, double thresh, int lane,
                                        int& steps, int& k_out) {
  int k = 0;
  steps = tol > 0 ? n : 0;
  for (int base = 0; tol > 0 && base < n; base += 64) {
    const int j = base + lane;
    bool below = false;
    if (j < n) below = (double)energy[(from + dir * j) * kNtF + f] < thresh;
    const unsigned long long m = __ballot(below);
    const int cnt = n - base < 64 ? n - base : 64;
    int pos = 0;
    bool found = false;
    while (pos < cnt) {
      const unsigned long long x = ~(m >> pos);  // lanes at and behind cnt are not below: a run ends inside the chunk
      int ones = x ? __builtin_ctzll(x) : 64;
      if (ones > cnt - pos) ones = cnt - pos;
      if (k + ones >= tol) {
        steps = base + pos + (tol - k);
        k = tol;
        found = true;
        break;
      }
      k += ones;
      pos += ones;
      if (pos >= cnt) break;
      const unsigned long long y = m >> pos;  // bit 0 clear: a cell at or above the threshold
      int zeros = y ? __builtin_ctzll(y) : 64;
      if (zeros > cnt - pos) zeros = cnt - pos;
      pos += zeros;
      k = 0;
    }
    if (found) break;
  }
  k_out = k;
}

// maximum of a row and the lowest bin that holds it (the clip has no NaN)
__device__ __forceinline__ void nt_row_max(const float* energy, int t, float* rm) {
  const float* e = energy + t * kNtF;
  float m = e[0];
  int a = 0;
#pragma unroll 8  // not all 87: every compare of an unrolled chain holds a scalar register pair until its select
  for (int f = 1; f < kNtF; ++f) {
    const float v = e[f];
    if (v > m) m = v, a = f;
  }
  rm[2 * t] = m;
  rm[2 * t + 1] = __int_as_float(a);
}

// numpy's pairwise sum of n <= 128 float32 values with stride 88 (note_decode.cpp pairwise_sum_f32, its first two branches)
__device__ __forceinline__ float nt_leaf_sum(const float* __restrict__ a, int n) {
  if (n < 8) {
    float res = 0.0f;
    for (int i = 0; i < n; ++i) res += a[i * kNtF];
    return res;
  }
  float r0 = a[0], r1 = a[kNtF], r2 = a[2 * kNtF], r3 = a[3 * kNtF], r4 = a[4 * kNtF], r5 = a[5 * kNtF], r6 = a[6 * kNtF],
        r7 = a[7 * kNtF];
  int i;
  for (i = 8; i < n - (n % 8); i += 8) {
    const float* p = a + i * kNtF;
    r0 += p[0], r1 += p[kNtF], r2 += p[2 * kNtF], r3 += p[3 * kNtF];
    r4 += p[4 * kNtF], r5 += p[5 * kNtF], r6 += p[6 * kNtF], r7 += p[7 * kNtF];
  }
  float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += a[i * kNtF];
  return res;
}

// np.mean of n >= 1 values of one bin (mean_f32): the recursion `sum(a, n2) + sum(a + n2, n - n2)`, n2 = n / 2 - (n / 2) % 8, as a
// walk with the lane's own stack in LDS.  An entry is a right half still to do (len > 0: its offset) or a finished left sum
// (len 0: its bits).
__device__ __forceinline__ float nt_mean(const float* __restrict__ a, int n, int (*s_off)[64], int (*s_len)[64], int lane) {
  int sp = 0, off = 0, len = n;
  float v;
  for (;;) {
    while (len > 128) {
      int n2 = len / 2;
      n2 -= n2 % 8;
      s_off[sp][lane] = off + n2;
      s_len[sp][lane] = len - n2;
      ++sp;
      len = n2;
    }
    v = nt_leaf_sum(a + (int64_t)off * kNtF, len);
    bool right = false;
    while (sp > 0) {
      const int l = s_len[sp - 1][lane];
      if (l > 0) {
        off = s_off[sp - 1][lane];
        len = l;
        s_len[sp - 1][lane] = 0;
        s_off[sp - 1][lane] = __float_as_int(v);
        right = true;
        break;
      }
      v = __int_as_float(s_off[sp - 1][lane]) + v;
      --sp;
    }
    if (!right) break;
  }
  const float s = 0.0f + v;
  return s / (float)n;
}

struct NtArgs {
  const float* note;        // [rows][88] frequency-constrained note rows of all clips
  const uint32_t* bits;     // [rows][3] onset-peak bitmap
  const int8_t* bend_map;   // [rows][88], or null: no bends wanted
  const int64_t* offs;      // [n_clips + 1] rows before each clip (a sweep: before each decode, which is where it writes)
  const int64_t* ev_first;  // [n_clips + 1] event records before each clip's region of the pool
  const int4* stats;        // per clip the record of note_device.hip (NdStats): .y != 0 is "a NaN in the note or onset rows"
  float* scratch;           // kNtRowWords words per row of all clips: the working state of clips over kNoteTrackLdsRows rows
  NtEvent* ev_pool;
  int8_t* bd_pool;          // clip c's bends at 88 * offs[c]: its region is the size of its bend map
  int4* counts;             // per clip: events, bends, status, 0
  double frame_thresh;
  int energy_tol, min_note_len, melodia;
};

// One clip.  energy: the working state of T rows (LDS or scratch), the cells and behind them per row the maximum and the bits of
// its bin; stack: 2 x depth x 64 words of LDS for nt_mean, depth >= nt_stack_depth(T); first: the clip's first row of a.note,
// a.bits and a.bend_map (the clips of a job: a.offs[c]; a decode of a sweep: its segment's, which other decodes share); its
// regions of the pools and its counts go by c.  Everything else as in NtArgs.
__device__ __forceinline__ void nt_track(const NtArgs& a, int64_t c, int64_t first, int T, float* energy, int* stack, int depth) {
  int(*s_off)[64] = reinterpret_cast<int(*)[64]>(stack), (*s_len)[64] = reinterpret_cast<int(*)[64]>(stack + depth * 64);
  __shared__ float s_best_v[4];
  __shared__ int s_best_i[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* note = a.note + first * kNtF;
  const uint32_t* bits = a.bits + first * 3;
  const int8_t* bend_map = a.bend_map ? a.bend_map + first * kNtF : nullptr;
  NtEvent* ev = a.ev_pool + a.ev_first[c];
  int8_t* bd = a.bd_pool + a.offs[c] * kNtF;
  const int cap_e = (int)(a.ev_first[c + 1] - a.ev_first[c]);
  const int tol = a.energy_tol, mnl = a.min_note_len;
  const double thresh = a.frame_thresh;
  int ne = 0, nb = 0;
  bool full = false;

  for (int i = tid; i < T * kNtF; i += 256) energy[i] = note[i];
  __syncthreads();

  // an event leaves: its record without the amplitude, its bends.  False: the region is full (nothing is written past it)
  auto emit = [&](int start, int end, int f) -> bool {
    const int len = end - start;
    if (ne >= cap_e || (bend_map && nb + len > T * kNtF)) return false;
    if (tid == 0) ev[ne] = NtEvent{start, end, f + kNtMidi, 0.0f};
    if (bend_map) {
      for (int t = start + tid; t < end; t += 256) bd[nb + (t - start)] = bend_map[t * kNtF + f];
      nb += len;
    }
    ++ne;
    return true;
  };
  // a note from the onset peak (start, f): follow the energy forward (decode_core track_from)
  auto track_from = [&](int start, int f) -> bool {
    if (start >= T - 1) return true;
    int steps, k;
    nt_scan(energy, f, start + 1, 1, T - 2 - start, tol, thresh, lane, steps, k);
    const int i = start + 1 + steps - k;
    if (i - start <= mnl) return true;
    __syncthreads();  // every wave has scanned before the cells change
    for (int r = start + tid; r < i; r += 256) {
      energy[r * kNtF + f] = 0.0f;
      if (f < kNtF - 1) energy[r * kNtF + f + 1] = 0.0f;
      if (f > 0) energy[r * kNtF + f - 1] = 0.0f;
    }
    __syncthreads();
    return emit(start, i, f);
  };

  // ---- onset phase: 64 rows per load, the rows that hold a peak by ballot, their bits from the highest down
  for (int tb = T - 2; tb >= 1 && !full; tb -= 64) {
    const int t = tb - lane;
    uint32_t w0 = 0, w1 = 0, w2 = 0;
    if (t >= 1) w0 = bits[t * 3], w1 = bits[t * 3 + 1], w2 = bits[t * 3 + 2] & 0xffffffu;
    unsigned long long rows = __ballot((w0 | w1 | w2) != 0);
    while (rows && !full) {
      const int l = __builtin_ctzll(rows);
      rows &= rows - 1;
      uint32_t hi = __shfl(w2, l), mid = __shfl(w1, l), lo = __shfl(w0, l);
      while ((hi | mid | lo) && !full) {  // one call site: the highest bin left
        uint32_t& w = hi ? hi : (mid ? mid : lo);
        const int base = hi ? 64 : (mid ? 32 : 0), b = 31 - __builtin_clz(w);
        w &= ~(1u << b);
        full = !track_from(tb - l, base + b);
      }
    }
  }

  // ---- melodia phase: per-row maxima, refreshed for the rows a walk wipes; the argmax over the rows by the workgroup
  if (a.melodia && !full) {
    float* rm = energy + T * kNtF;
    for (int t = tid; t < T; t += 256) nt_row_max(energy, t, rm);
    __syncthreads();
    for (;;) {
      float bv = -__int_as_float(0x7f800000);
      int bi = 0x7fffffff;
      for (int t = tid; t < T; t += 256)
        if (rm[2 * t] > bv) bv = rm[2 * t], bi = t * kNtF + __float_as_int(rm[2 * t + 1]);  // ascending rows: the first stays
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
      }
      if (lane == 0) s_best_v[wave] = bv, s_best_i[wave] = bi;
      __syncthreads();
      bv = s_best_v[0], bi = s_best_i[0];
#pragma unroll
      for (int w = 1; w < 4; ++w)
        if (s_best_v[w] > bv || (s_best_v[w] == bv && s_best_i[w] < bi)) bv = s_best_v[w], bi = s_best_i[w];
      if (!((double)bv > thresh)) break;
      const int i_mid = bi / kNtF, f = bi % kNtF;
      // forward over rows i_mid + 1 ... T - 2, backward over i_mid - 1 ... 1: a walk reads a row before it wipes it and never
      // reads it again, so both scans see the cells as they are now
      int sf = 0, kf = 0, sb = 0, kb = 0;
#pragma unroll 1
      for (int dir = 1; dir >= -1; dir -= 2) {  // one copy of the scan
        const int n = dir > 0 ? T - 2 - i_mid : i_mid - 1;
        int steps, k;
        nt_scan(energy, f, i_mid + dir, dir, n > 0 ? n : 0, tol, thresh, lane, steps, k);
        if (dir > 0) sf = steps, kf = k; else sb = steps, kb = k;
      }
      const int i_end = i_mid + sf - kf, i_start = i_mid - sb + kb;
      __syncthreads();  // every wave has its maximum and its scans before the cells and s_best change
      for (int r = i_mid - sb + tid; r <= i_mid + sf; r += 256) {
        energy[r * kNtF + f] = 0.0f;
        if (r != i_mid) {  // the maximum's own row loses that cell alone
          if (f < kNtF - 1) energy[r * kNtF + f + 1] = 0.0f;
          if (f > 0) energy[r * kNtF + f - 1] = 0.0f;
        }
        const int at = __float_as_int(rm[2 * r + 1]);
        if (at >= f - 1 && at <= f + 1) nt_row_max(energy, r, rm);  // this thread alone touches row r
      }
      __syncthreads();
      if (i_end - i_start <= mnl) continue;
      if (!emit(i_start, i_end, f)) {
        full = true;
        break;
      }
    }
  }

  // ---- amplitudes: np.mean over the ORIGINAL note rows, an event per lane of the first wave
  __syncthreads();
  if (full) ne = nb = 0;
  if (wave == 0)
    for (int e = lane; e < ne; e += 64) {
      const NtEvent v = ev[e];
      ev[e].amp = nt_mean(note + (int64_t)v.start * kNtF + (v.pitch - kNtMidi), v.end - v.start, s_off, s_len, lane);
    }
  if (tid == 0) a.counts[c] = make_int4(ne, nb, full ? 2 : 0, 0);
}

// where the stacks lie in a launch's dynamic LDS: behind the working state of lds_rows rows (kLds), or alone
template <bool kLds>
__device__ __forceinline__ int* nt_stack(float* s_state, int lds_rows) {
  return reinterpret_cast<int*>(s_state + (kLds ? lds_rows * kNtRowWords : 0));
}

// kLds: the clips of at most lds_rows rows, their working state in dynamic LDS (lds_rows * kNtRowWords words, the stacks behind
// it); otherwise the longer ones, theirs in the scratch buffer (dynamic LDS: the stacks alone).  A clip of the other kind is
// the other launch's.  depth: of the stacks the launch has room for.
template <bool kLds>
__global__ __launch_bounds__(256) void nt_track_kernel(NtArgs a, int lds_rows, int depth) {
  extern __shared__ float s_state[];
  const int64_t c = blockIdx.x;
  const int64_t rows = a.offs[c + 1] - a.offs[c];
  if ((rows <= lds_rows) != kLds) return;
  // no rows: nothing to decode; a NaN: the host's rules decide (status 1); more rows than a region is ever given: status 2
  if (rows == 0 || a.stats[c].y != 0 || rows > kNoteTrackMaxRows) {
    if (threadIdx.x == 0) a.counts[c] = make_int4(0, 0, rows == 0 ? 0 : (a.stats[c].y != 0 ? 1 : 2), 0);
    return;
  }
  const int T = (int)rows;
  float* state = kLds ? s_state : a.scratch + a.offs[c] * kNtRowWords;
  nt_track(a, c, a.offs[c], T, state, nt_stack<kLds>(s_state, lds_rows), depth);
}

// The same two forms for segments that carry their own parameters (bp_streams_events: a segment is a stream's slice): segment
// c decodes with seg[c], read beside its row offsets; a segment marked `skip` (an onset threshold <= 0) is the host's, status 1.
template <bool kLds>
__global__ __launch_bounds__(256) void nt_track_segs_kernel(NtArgs a, const NoteTrackSeg* __restrict__ seg, int lds_rows, int depth) {
  extern __shared__ float s_state[];
  const int64_t c = blockIdx.x;
  const int64_t rows = a.offs[c + 1] - a.offs[c];
  if ((rows <= lds_rows) != kLds) return;
  const NoteTrackSeg p = seg[c];
  const bool host = p.skip != 0 || a.stats[c].y != 0;
  if (rows == 0 || host || rows > kNoteTrackMaxRows) {
    if (threadIdx.x == 0) a.counts[c] = make_int4(0, 0, rows == 0 ? 0 : (host ? 1 : 2), 0);
    return;
  }
  a.frame_thresh = p.frame_thresh;
  a.energy_tol = p.energy_tol, a.min_note_len = p.min_note_len, a.melodia = p.melodia;
  if (!p.bends) a.bend_map = nullptr;
  float* state = kLds ? s_state : a.scratch + a.offs[c] * kNtRowWords;
  nt_track(a, c, a.offs[c], (int)rows, state, nt_stack<kLds>(s_state, lds_rows), depth);
}

// The same two forms over the decode table of a sweep (bp_note_events_sweep): workgroup c is decode c, tab[c] says which rows
// of which note copy, bitmap and stats block it reads and with which parameters.  Decodes share rows, so what a decode WRITES
// is its own: a.offs holds the rows of the decodes before it — its region of the bend pool and of the scratch state —, and
// a.ev_first its region of the event pool, as for the clips of a job.  a.bend_map is the one bend map of the shared rows.
template <bool kLds>
__global__ __launch_bounds__(256) void nt_track_sweep_kernel(NtArgs a, const NoteSweepDecode* __restrict__ tab, int lds_rows,
                                                             int depth) {
  extern __shared__ float s_state[];
  const int64_t c = blockIdx.x;
  const NoteSweepDecode d = tab[c];
  if ((d.rows <= lds_rows) != kLds) return;
  // (a set with an onset threshold <= 0 has no dense half: its stats pointer is null and never read)
  const bool host = d.rows > 0 && (d.seg.skip != 0 || static_cast<const int4*>(d.stats)->y != 0);
  if (d.rows == 0 || host || d.rows > kNoteTrackMaxRows) {
    if (threadIdx.x == 0) a.counts[c] = make_int4(0, 0, d.rows == 0 ? 0 : (host ? 1 : 2), 0);
    return;
  }
  a.note = d.note, a.bits = reinterpret_cast<const uint32_t*>(d.bits);
  a.frame_thresh = d.seg.frame_thresh;
  a.energy_tol = d.seg.energy_tol, a.min_note_len = d.seg.min_note_len, a.melodia = d.seg.melodia;
  if (!d.seg.bends) a.bend_map = nullptr;
  float* state = kLds ? s_state : a.scratch + a.offs[c] * kNtRowWords;
  nt_track(a, c, d.first, (int)d.rows, state, nt_stack<kLds>(s_state, lds_rows), depth);
}

// ---- the second step: events and bends contiguous in clip order.  meta: [n + 1] events before each clip, [n + 1] bends before
// each clip, [n] status.
__global__ __launch_bounds__(256) void nt_offsets_kernel(const int4* __restrict__ counts, int64_t n, int64_t* __restrict__ meta) {
  __shared__ int64_t s_e[256], s_b[256];
  const int tid = threadIdx.x;
  const int64_t per = (n + 255) / 256, lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  int64_t se = 0, sb = 0;
  for (int64_t c = lo; c < hi; ++c) se += counts[c].x, sb += counts[c].y;
  s_e[tid] = se, s_b[tid] = sb;
  __syncthreads();
  if (tid == 0) {
    int64_t re = 0, rb = 0;
    for (int i = 0; i < 256; ++i) {
      const int64_t e = s_e[i], b = s_b[i];
      s_e[i] = re, s_b[i] = rb;
      re += e, rb += b;
    }
    meta[n] = re, meta[2 * n + 1] = rb;
  }
  __syncthreads();
  se = s_e[tid], sb = s_b[tid];
  for (int64_t c = lo; c < hi; ++c) {
    meta[c] = se, meta[n + 1 + c] = sb, meta[2 * n + 2 + c] = counts[c].z;
    se += counts[c].x, sb += counts[c].y;
  }
}

__global__ __launch_bounds__(256) void nt_pack_kernel(const int4* __restrict__ counts, const int64_t* __restrict__ offs,
                                                      const int64_t* __restrict__ ev_first, const int64_t* __restrict__ meta,
                                                      int64_t n, const int4* __restrict__ ev_pool, const int8_t* __restrict__ bd_pool,
                                                      int4* __restrict__ ev_out, int8_t* __restrict__ bd_out) {
  const int64_t c = blockIdx.x;
  const int ne = counts[c].x, nb = counts[c].y;
  const int4* ev = ev_pool + ev_first[c];
  const int8_t* bd = bd_pool + offs[c] * kNtF;
  int4* eo = ev_out + meta[c];
  int8_t* bo = bd_out + meta[n + 1 + c];
  for (int i = threadIdx.x; i < ne; i += 256) eo[i] = ev[i];
  for (int i = threadIdx.x; i < nb; i += 256) bo[i] = bd[i];
}

int64_t note_track_capacity(int64_t rows, int min_note_len) {
  if (rows <= 0 || rows > kNoteTrackMaxRows) return 0;
  const int64_t shortest = (int64_t)(min_note_len > 0 ? min_note_len : 0) + 1;
  return kNtF * ((rows + shortest - 1) / shortest);
}

int64_t note_track_scratch_floats(int64_t total_rows) { return total_rows * kNtRowWords; }

// The tracker's launches for either kind of segment: the LDS form sized by the longest segment that takes it (a job of
// one-window clips runs three workgroups per compute unit), the scratch form where a segment is longer (lds_limit 0: for every
// segment), each with the stacks its longest segment needs; then the second step (meta null: none).  extra: what a kernel takes between the
// arguments and lds_rows.
template <class Kernel, class... Extra>
static hipError_t nt_launch(Kernel lds, Kernel scratch, const NtArgs& a, int64_t n, int64_t max_rows, int lds_limit, int64_t* meta,
                            void* ev_out, int8_t* bd_out, hipStream_t s, Extra... extra) {
  const int lds_rows = (int)(max_rows < lds_limit ? max_rows : lds_limit);
  const int depth = nt_stack_depth(lds_rows), deep = nt_stack_depth(max_rows);
  const size_t lds_bytes = ((size_t)lds_rows * kNtRowWords + 2 * depth * 64) * 4;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lds, dim3((unsigned)n), dim3(256), lds_bytes, s, a, extra..., lds_rows, depth);
  if (max_rows > lds_limit)
    hipLaunchKernelGGL(scratch, dim3((unsigned)n), dim3(256), (size_t)2 * deep * 64 * 4, s, a, extra..., lds_rows, deep);
  if (!meta) return hipGetLastError();  // the events stay in the pool (launch_note_track_sweep for launch_note_score)
  hipLaunchKernelGGL(nt_offsets_kernel, dim3(1), dim3(256), 0, s, a.counts, n, meta);
  hipLaunchKernelGGL(nt_pack_kernel, dim3((unsigned)n), dim3(256), 0, s, a.counts, a.offs, a.ev_first, meta, n,
                     reinterpret_cast<const int4*>(a.ev_pool), a.bd_pool, static_cast<int4*>(ev_out), bd_out);
  return hipGetLastError();
}

hipError_t launch_note_track_segs(const float* note, const uint8_t* bits, const int8_t* bend_map, const int64_t* offs,
                                  const int64_t* ev_first, const void* stats, const NoteTrackSeg* seg, int64_t n_segs,
                                  int64_t max_rows, int form, float* scratch, void* ev_pool, int8_t* bd_pool, void* counts,
                                  int64_t* meta, void* ev_out, int8_t* bd_out, hipStream_t s) {
  if (n_segs <= 0) return hipSuccess;
  const NtArgs a{note, reinterpret_cast<const uint32_t*>(bits), bend_map, offs, ev_first, static_cast<const int4*>(stats), scratch,
                 static_cast<NtEvent*>(ev_pool), bd_pool, static_cast<int4*>(counts), 0.0, 0, 0, 0};
  return nt_launch(&nt_track_segs_kernel<true>, &nt_track_segs_kernel<false>, a, n_segs, max_rows,
                   form == kNoteTrackFormScratch ? 0 : kNoteTrackLdsRows, meta, ev_out, bd_out, s, seg);
}

hipError_t launch_note_track_sweep(const NoteSweepDecode* tab, int64_t n_decodes, int64_t max_rows, const int8_t* bend_map,
                                   const int64_t* pool_rows, const int64_t* ev_first, float* scratch, void* ev_pool, int8_t* bd_pool,
                                   void* counts, int64_t* meta, void* ev_out, int8_t* bd_out, hipStream_t s) {
  if (n_decodes <= 0) return hipSuccess;
  const NtArgs a{nullptr, nullptr, bend_map, pool_rows, ev_first, nullptr, scratch, static_cast<NtEvent*>(ev_pool), bd_pool,
                 static_cast<int4*>(counts), 0.0, 0, 0, 0};
  return nt_launch(&nt_track_sweep_kernel<true>, &nt_track_sweep_kernel<false>, a, n_decodes, max_rows, kNoteTrackLdsRows, meta,
                   ev_out, bd_out, s, tab);
}

hipError_t launch_note_track(const float* note, const uint8_t* bits, const int8_t* bend_map, const int64_t* offs,
                             const int64_t* ev_first, const void* stats, int64_t n_clips, int64_t max_rows, double frame_thresh,
                             int energy_tol, int min_note_len, int melodia, float* scratch, void* ev_pool, int8_t* bd_pool,
                             void* counts, int64_t* meta, void* ev_out, int8_t* bd_out, hipStream_t s) {
  if (n_clips <= 0) return hipSuccess;
  const NtArgs a{note, reinterpret_cast<const uint32_t*>(bits), bend_map, offs, ev_first, static_cast<const int4*>(stats), scratch,
                 static_cast<NtEvent*>(ev_pool), bd_pool, static_cast<int4*>(counts), frame_thresh, energy_tol, min_note_len, melodia};
  return nt_launch(&nt_track_kernel<true>, &nt_track_kernel<false>, a, n_clips, max_rows, kNoteTrackLdsRows, meta, ev_out, bd_out, s);
}

}  // namespace bp
