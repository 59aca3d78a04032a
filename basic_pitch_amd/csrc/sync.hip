// Two recordings against each other on the device (include/basic_pitch_amd_sync.h): the note rows of the
// segments that a pair names become one feature of 16 bytes a unit, and every pair of segments a path by the header's
// recurrence.  Every number is the header's integer, so sums may be taken in any order.  Two kernels, stream-ordered.
//
// FEATURES (sync_feature_kernel).  Unit-parallel over all segments: sixteen lanes a unit, a lane a class (lanes 12 ... 15
// idle).  The lane reads the pitches of ITS class of every frame of the unit, all octaves whatever the band — the twelve
// classes are all 88 pitches, so the NaN flag of the segment comes from the same loads —, quantises them and sums what lies
// in the band above the threshold.  The squares meet by four shuffles inside the sixteen lanes; the ceiling root is the
// float64 root put right by comparisons (s < 2^42: the float64 root is within one of it); four lanes' bytes make a word.
//
// RECURRENCE AND BACKTRACE (sync_path_kernel<kL, kC, kNA>).  A WORKGROUP TAKES A PAIR.  Lane l owns columns l kC ... l kC +
// kC - 1 of b and works at step s on row i = s - l.  D is int32 in registers, "unreachable" is -2^30 and a reachable D is never
// negative, so a candidate is reachable exactly when it is >= 0 and an unreachable one loses every strict comparison against a
// reachable one: the tie order needs no case for it.  The lane below's last-column D of the row it just finished is this
// lane's (i, j-1) source for its first column, and what came one step earlier is the (i-1, j-1) source: a data-parallel shift
// by one lane within the wave, and for lane 0 of a wave the value lane 63 of the wave below left in LDS, double-buffered: ONE
// barrier per step, taken by every lane on every step, idle or not.  xa lies in LDS as three planes of words (consecutive
// lanes read consecutive words, descending), the lane's columns of xb are 3 kC registers, a gain is three v_dot4_u32_u8.  The
// predecessors are two bits a cell, 2 kC bits a lane and step, stored as [step][lane]: a wave's store is one run.
// Backtrace: tiles of kSyncTraceTile steps x kSyncTraceTile lanes of those records come to LDS (where xa was) by all lanes —
// a move to a lower lane costs at least one step, so the walk cannot leave the tile's lanes before it leaves its steps —,
// lane 0 walks the tile and stores the cells it visits, packed, from the end of the path backwards; when (0, 0) is reached all
// lanes turn them round into the pair's region and fill the tail.  No loop waits on memory another workgroup writes; no
// indexed register array, no recursion, no inline assembly: no scratch.
#include "bp_kernels.h"

#pragma clang fp contract(off)
#pragma clang fp reassociate(off)

namespace bp {

namespace {

constexpr int kPitches = 88, kClasses = 12, kLanesPerUnit = 16;
constexpr int kNeg = -(1 << 30);  // unreachable; a candidate from it stays below 0 (a gain is at most 65,025, doubled)

__device__ __forceinline__ int quantise(float x) { return (int)floorf(fminf(fmaxf(x, 0.0f), 1.0f) * 1024.0f + 0.5f); }

// the segment of unit `at`: the last one whose unit_first is <= at (unit_first ascends, every segment has units)
__device__ __forceinline__ int64_t segment_of(const SyncSeg* __restrict__ segs, int64_t n, int64_t at) {
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (segs[mid].unit_first <= at) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void sync_feature_kernel(const float* __restrict__ note, SyncParams prm, const SyncSeg* __restrict__ segs,
                                                           int64_t n_segs, int64_t n_units, uint32_t* __restrict__ feat,
                                                           uint32_t* __restrict__ nan_flags) {
  const int tid = threadIdx.x, k = tid & (kLanesPerUnit - 1);
  const int64_t g = (int64_t)blockIdx.x * (256 / kLanesPerUnit) + (tid >> 4);
  if (g >= n_units) return;  // (the sixteen lanes of a unit leave together)
  const int64_t c = segment_of(segs, n_segs, g);
  const SyncSeg seg = segs[c];
  const int64_t t0 = (g - seg.unit_first) * prm.hop, t1 = t0 + prm.hop < seg.rows ? t0 + prm.hop : seg.rows;
  int cu = 0, nan = 0;  // cu <= 64 * 2^13
  if (k < kClasses)
    for (int64_t t = t0; t < t1; ++t) {
      const float* __restrict__ row = note + (seg.row_first + t) * kPitches;
      for (int p = (k + 3) % 12; p < kPitches; p += 12) {  // class (p + 9) % 12 == k
        const float x = row[p];
        nan |= x != x;
        const int above = quantise(x) - prm.threshold_q;
        if (p >= prm.min_pitch && p <= prm.max_pitch && above > 0) cu += above;
      }
    }
  long long s = (long long)cu * cu;  // < 2^38, the sum of twelve < 2^42
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o), nan |= __shfl_xor(nan, o);
  long long r = (long long)sqrt((double)s);
#pragma unroll
  for (int fix = 0; fix < 2; ++fix) r += r * r < s ? 1 : 0;
#pragma unroll
  for (int fix = 0; fix < 2; ++fix) r -= r > 0 && (r - 1) * (r - 1) >= s ? 1 : 0;  // the smallest r with r * r >= s
  const uint32_t x = (uint32_t)(255 * cu) / (uint32_t)(r > 0 ? r : 1);             // <= 255: cu <= r; a silent unit is 0 / 1
  const uint32_t word = x | (__shfl_down(x, 1) << 8) | (__shfl_down(x, 2) << 16) | (__shfl_down(x, 3) << 24);
  if ((k & 3) == 0) feat[g * 4 + (k >> 2)] = word;  // (lanes 12 ... 15 hold 0: the four zero bytes)
  if (nan && k == 0) atomicOr(&nan_flags[c], 1u);
}

// lane l takes the value of lane l - 1 of its wave (wave_shr:1); lane 0 keeps its own
__device__ __forceinline__ int from_lane_below(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

template <int kC>
struct PredOf {
  using type = uint8_t;
};
template <>
struct PredOf<8> {
  using type = uint16_t;
};

// kL lanes, kC columns a lane, room for kNA units of a in LDS
template <int kL, int kC, int kNA>
__global__ __launch_bounds__(kL) void sync_path_kernel(const uint4* __restrict__ feat, const SyncSeg* __restrict__ segs,
                                                       const SyncPair* __restrict__ pairs, const uint32_t* __restrict__ nan_flags, int band,
                                                       uint8_t* __restrict__ pred_pool, uint32_t* __restrict__ walk_pool,
                                                       int2* __restrict__ path_pool, SyncSummary* __restrict__ summaries) {
  using Pred = typename PredOf<kC>::type;
  constexpr int kW = kL / 64, kT = kSyncTraceTile;
  static_assert(sizeof(Pred) * 8 >= 2 * kC && kT * kT * sizeof(Pred) <= 3 * kNA * sizeof(uint32_t), "a record holds a lane's bits; a tile fits where xa was");
  __shared__ uint32_t s_xa[3 * kNA];
  __shared__ int s_edge[2][kW];
  __shared__ int s_at[4];  // the walk between tiles: its step, its lane, the cells stored, whether (0, 0) is reached
  __shared__ int s_total;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SyncPair pr = pairs[blockIdx.x];
  const int N = pr.a >= 0 ? (int)segs[pr.a].n_units : 0, M = pr.b >= 0 ? (int)segs[pr.b].n_units : 0;
  const int cap = N > 0 && M > 0 ? N + M - 1 : 0;
  int2* __restrict__ path = path_pool + pr.path_first;
  const auto refuse = [&](int why) {
    for (int k = tid; k < cap; k += kL) path[k] = make_int2(-1, -1);
    if (tid == 0) summaries[blockIdx.x] = SyncSummary{why, N, M, 0, pr.path_first, 0};
  };
  if ((pr.a >= 0 && nan_flags[pr.a] != 0) || (pr.b >= 0 && nan_flags[pr.b] != 0)) return refuse(1);  // (uniform)
  if (cap == 0 || N > kNA || M > kL * kC) return refuse(2);  // (the launch chooses kNA, kL and kC so that only "no rows" is met)

  const uint4* __restrict__ fa = feat + segs[pr.a].unit_first;
  const uint4* __restrict__ fb = feat + segs[pr.b].unit_first;
  for (int i = tid; i < N; i += kL) {
    const uint4 v = fa[i];
    s_xa[i] = v.x, s_xa[kNA + i] = v.y, s_xa[2 * kNA + i] = v.z;
  }
  const int used = (M + kC - 1) / kC, steps = N + used - 1;
  const int j0 = tid * kC;
  uint32_t xb[kC][3];
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    const uint4 v = fb[j0 + c < M ? j0 + c : M - 1];  // (a column past the end: the last one again, never admissible)
    xb[c][0] = v.x, xb[c][1] = v.y, xb[c][2] = v.z;
  }
  Pred* __restrict__ pred = reinterpret_cast<Pred*>(pred_pool + pr.pred_first);
  const int wide = N > M ? N - 1 : M - 1, limit = band * wide;  // < 2^26
  int D[kC];
#pragma unroll
  for (int c = 0; c < kC; ++c) D[c] = kNeg;
  int last = kNeg, left_before = kNeg;
  __syncthreads();

  // ---- forward
  for (int s = 0; s < steps; ++s) {
    int left_in = from_lane_below(last);
    if (lane == 0) left_in = wave > 0 && s > 0 ? s_edge[(s - 1) & 1][wave - 1] : kNeg;
    int diag = left_before, left = left_in;
    left_before = left_in;
    const int i = s - tid;
    const bool active = tid < used && i >= 0 && i < N;
    const int row = i < 0 ? 0 : (i < N ? i : N - 1);  // (an idle lane reads a row of a and uses nothing of it)
    const uint32_t a0 = s_xa[row], a1 = s_xa[kNA + row], a2 = s_xa[2 * kNA + row];
    uint32_t bits = 0;
#pragma unroll
    for (int c = 0; c < kC; ++c) {
      const int g = (int)__builtin_amdgcn_udot4(a0, xb[c][0], __builtin_amdgcn_udot4(a1, xb[c][1], __builtin_amdgcn_udot4(a2, xb[c][2], 0u, false), false), false);
      const int j = j0 + c, up = D[c];
      int best = diag + 2 * g;
      uint32_t code = 0;
      if (up + g > best) best = up + g, code = 1;
      if (left + g > best) best = left + g, code = 2;
      if (s == 0 && j == 0) best = 2 * g, code = 0;  // D[0][0]
      const int off = i * (M - 1) - j * (N - 1);
      const bool admissible = j < M && (band == 0 || (off < 0 ? -off : off) <= limit);
      if (!admissible || best < 0) best = kNeg;
      bits |= code << (2 * c);
      diag = up, left = best;
      D[c] = active ? best : up;
    }
    last = active ? left : kNeg;
    if (active) pred[(size_t)s * used + tid] = (Pred)bits;
    if (lane == 63) s_edge[s & 1][wave] = last;
    __syncthreads();
  }

  // ---- the end of the path
  const int l_end = (M - 1) / kC;
  if (tid == l_end) {
#pragma unroll
    for (int c = 0; c < kC; ++c)
      if (c == (M - 1) % kC) s_total = D[c];
  }
  if (tid == 0) s_at[0] = steps - 1, s_at[1] = l_end, s_at[2] = 0, s_at[3] = 0;
  __threadfence();  // the records are in memory for the lanes that fetch them
  __syncthreads();
  const int total = s_total;
  if (total < 0) return refuse(2);  // (uniform; the header's staircase says that no band does this)

  // ---- backtrace, a tile at a time from the end
  Pred* tile = reinterpret_cast<Pred*>(s_xa);
  uint32_t* __restrict__ walk = walk_pool + pr.path_first;
  int wi = N - 1, wj = M - 1;  // lane 0's
  const int n_tiles = (steps + kT - 1) / kT + 1;
  for (int it = 0; it < n_tiles; ++it) {
    if (s_at[3]) break;  // (uniform: written before the last barrier)
    const int s_cur = s_at[0], l_cur = s_at[1];
    const int s_lo = s_cur - kT + 1 > 0 ? s_cur - kT + 1 : 0, l_lo = l_cur - kT + 1 > 0 ? l_cur - kT + 1 : 0;
    for (int e = tid; e < kT * kT; e += kL) {
      const int sr = s_lo + e / kT, l = l_lo + e % kT;
      // (inside the pair's steps x used records.  Where lane l had no row at step sr nothing was stored and the byte is what
      // the pool held before: the walk only visits cells that a lane computed, so it never reads such a record.)
      if (sr <= s_cur && l <= l_cur) tile[e] = pred[(size_t)sr * used + l];
    }
    __syncthreads();
    if (tid == 0) {
      int k = s_at[2], done = 0;
      while (k < cap) {  // (a path has at most cap cells: nothing is stored beyond the pair's region)
        const int l = wj / kC, s = wi + l;
        if (s < s_lo || l < l_lo) break;
        walk[k++] = ((uint32_t)wi << 16) | (uint32_t)wj;
        if (wi == 0 && wj == 0) {
          done = 1;
          break;
        }
        const uint32_t code = ((uint32_t)tile[(s - s_lo) * kT + (l - l_lo)] >> (2 * (wj % kC))) & 3u;
        if (code != 2 && wi > 0) --wi;
        if (code != 1 && wj > 0) --wj;
      }
      s_at[0] = wi + wj / kC, s_at[1] = wj / kC, s_at[2] = k, s_at[3] = done || k >= cap;
      __threadfence();
    }
    __syncthreads();
  }
  const int n = s_at[2];
  for (int k = tid; k < cap; k += kL) {
    int2 cell = make_int2(-1, -1);
    if (k < n) {
      const uint32_t w = walk[n - 1 - k];
      cell = make_int2((int)(w >> 16), (int)(w & 0xffffu));
    }
    path[k] = cell;
  }
  if (tid == 0) summaries[blockIdx.x] = SyncSummary{0, N, M, n, pr.path_first, total};
}

template <int kL, int kC>
void launch_path(int max_n, unsigned n_pairs, hipStream_t s, const uint4* feat, const SyncSeg* segs, const SyncPair* pairs,
                 const uint32_t* nan_flags, int band, uint8_t* pred, uint32_t* walk, int2* path, SyncSummary* summaries) {
  if (max_n <= kSyncSmallRows)
    hipLaunchKernelGGL((sync_path_kernel<kL, kC, kSyncSmallRows>), dim3(n_pairs), dim3(kL), 0, s, feat, segs, pairs, nan_flags, band, pred, walk,
                       path, summaries);
  else
    hipLaunchKernelGGL((sync_path_kernel<kL, kC, kSyncMaxUnits>), dim3(n_pairs), dim3(kL), 0, s, feat, segs, pairs, nan_flags, band, pred, walk,
                       path, summaries);
}

}  // namespace

hipError_t launch_sync(const float* note, const SyncParams& params, const SyncSeg* segs, int64_t n_segs, int64_t n_units,
                       const SyncPair* pairs, int64_t n_pairs, int max_n, int max_m, uint32_t* nan_flags, void* feat, uint8_t* pred,
                       uint32_t* walk, int32_t* path, SyncSummary* summaries, hipStream_t s) {
  if (n_pairs <= 0) return hipSuccess;
  constexpr int kUnits = 256 / kLanesPerUnit;
  if (n_segs < 1 || n_units < 1 || (n_units + kUnits - 1) / kUnits > 0x7fffffffll || n_pairs > 0x7fffffffll || max_n < 0 ||
      max_n > kSyncMaxUnits || max_m < 0 || max_m > kSyncMaxUnits)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(nan_flags, 0, (size_t)n_segs * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sync_feature_kernel, dim3((unsigned)((n_units + kUnits - 1) / kUnits)), dim3(256), 0, s, note, params, segs, n_segs, n_units,
                     static_cast<uint32_t*>(feat), nan_flags);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const SyncPlan plan = sync_plan(max_m);
  const uint4* f = static_cast<const uint4*>(feat);
  int2* out = reinterpret_cast<int2*>(path);
  const unsigned n = (unsigned)n_pairs;
  if (plan.lanes == kSyncSmallLanes && plan.cols == 1)
    launch_path<kSyncSmallLanes, 1>(max_n, n, s, f, segs, pairs, nan_flags, params.band, pred, walk, out, summaries);
  else if (plan.lanes == kSyncSmallLanes && plan.cols == 2)
    launch_path<kSyncSmallLanes, 2>(max_n, n, s, f, segs, pairs, nan_flags, params.band, pred, walk, out, summaries);
  else if (plan.lanes == kSyncSmallLanes && plan.cols == 4)
    launch_path<kSyncSmallLanes, 4>(max_n, n, s, f, segs, pairs, nan_flags, params.band, pred, walk, out, summaries);
  else if (plan.lanes == kSyncSmallLanes)
    launch_path<kSyncSmallLanes, 8>(max_n, n, s, f, segs, pairs, nan_flags, params.band, pred, walk, out, summaries);
  else if (plan.cols == 4)
    launch_path<kSyncLanes, 4>(max_n, n, s, f, segs, pairs, nan_flags, params.band, pred, walk, out, summaries);
  else
    launch_path<kSyncLanes, 8>(max_n, n, s, f, segs, pairs, nan_flags, params.band, pred, walk, out, summaries);
  return hipGetLastError();
}

}  // namespace bp
