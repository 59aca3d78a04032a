// Tempo and beats on the device (include/basic_pitch_amd_beat.h): the onset rows of a segment become a strength
// per row, the strengths a period by autocorrelation under the prior, and the period a beat path by the header's recurrence.
// Every number is the header's integer, so sums may be taken in any order.  Three kernels, stream-ordered.
//
// STRENGTH (beat_strength_kernel).  Row-parallel over all segments: a block takes kBeatStrengthRows rows of ONE segment, eight
// lanes a row, a 16-byte load a lane and step (a row is 22 of them).  The NaN flag comes from the same loads and covers all 88
// pitches whatever the band.  sum o and sum o^2 are reduced in the block and added by one integer atomic each per block.
//
// TEMPO (beat_tempo_kernel).  A block takes a tile of kBeatTempoRows rows x kBeatTempoLags lags of one segment: the strengths
// of the tile and of the lags behind it come to LDS once, zero beyond the segment's end, so the loop has no bounds test; a lane
// takes a lag and a quarter of the rows (o[t] is a broadcast, o[t + L] 64 consecutive words), the quarters are added through
// LDS, and one integer atomic per lag and block goes into A[segment][lag].  One long track is many tiles.
//
// PATH (beat_path_kernel).  A WORKGROUP TAKES A SEGMENT.  It picks the period (every wave for itself: no broadcast), then runs
// the recurrence A BLOCK OF dmin FRAMES AT A TIME: a beat's predecessor lies at least dmin back, so the frames of a block depend
// on earlier blocks alone, A WAVE TAKES A FRAME, and the workgroup meets once per block.  Inside a wave the lanes take the
// candidates d = dmin + lane + 64 k (at most 7 a lane), read C[t - d] from an LDS ring of int64, subtract pen[d] — in registers,
// a lane's d are the same for every frame — and pack (value + 2^44, 1023 - d) into one 64-bit key, whose maximum over the wave
// (DPP row scans and broadcasts, no trip through LDS) is the largest value at the smallest d; the start candidate is the
// initial key, so ties go to it.  The kernel is paced by its instruction count (16 waves on four SIMDs), so the ring holds
// C << 10 and a candidate's key is one 64-bit addition of a constant of the lane.  The strengths come to LDS two chunks of kBeatRing rows ahead.  The predecessor is one uint16 a
// row in the pool.  Ending: the first maximum of C over the last P frames, from the ring.  Backtrace: tiles of 4096
// predecessors come back to LDS by all lanes (the strengths' buffer is free by then), lane 0 walks the tile and stores the
// beats, last beat first — the caller turns them round.  No indexed register array, no recursion, no inline assembly: no scratch.
#include <cstring>

#include "bp_kernels.h"

#pragma clang fp contract(off)
#pragma clang fp reassociate(off)

namespace bp {

namespace {

constexpr int kPitches = 88, kRowVecs = kPitches / 4;
constexpr int kPredTile = 4 * kBeatRing;  // uint16 entries in the bytes of 2 * kBeatRing ints
constexpr long long kBias = 1ll << 44;
constexpr unsigned long long kStartKey = ((unsigned long long)kBias << 10) | 1023ull;  // value 0, d 0

__device__ __forceinline__ int quantise(float x) { return (int)floorf(fminf(fmaxf(x, 0.0f), 1.0f) * 1024.0f + 0.5f); }

// the segment of block / tile `at`: the last one whose first is <= at (the firsts ascend; a segment's are one run)
template <int64_t BeatSeg::*kFirst>
__device__ __forceinline__ int64_t segment_of(const BeatSeg* __restrict__ segs, int64_t n, int64_t at) {
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (segs[mid].*kFirst <= at) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void add64(int64_t* at, long long v) { atomicAdd(reinterpret_cast<unsigned long long*>(at), (unsigned long long)v); }

__global__ __launch_bounds__(256) void beat_strength_kernel(const float* __restrict__ onset, const BeatParams* __restrict__ params,
                                                            const BeatSeg* __restrict__ segs, int64_t n_segs,
                                                            int32_t* __restrict__ strength, int64_t* __restrict__ acc) {
  __shared__ int s_row[kBeatStrengthRows];
  const int tid = threadIdx.x, part = tid & 7, r = tid >> 3;
  const int64_t b = blockIdx.x;
  const int64_t c = segment_of<&BeatSeg::blk_first>(segs, n_segs, b);
  const BeatSeg seg = segs[c];
  const int thr = params->threshold_q, lo = params->min_pitch, hi = params->max_pitch;
  const int64_t t = (b - seg.blk_first) * kBeatStrengthRows + r;
  int sum = 0, nan = 0;
  if (t < seg.rows) {
    const float4* __restrict__ row = reinterpret_cast<const float4*>(onset + (seg.row_first + t) * kPitches);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int j = part + 8 * k;
      if (j < kRowVecs) {
        const float4 v = row[j];
        const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          nan |= x[e] != x[e];
          const int pitch = 4 * j + e, above = quantise(x[e]) - thr;
          if (pitch >= lo && pitch <= hi && above > 0) sum += above;
        }
      }
    }
  }
  sum += __shfl_xor(sum, 1);
  sum += __shfl_xor(sum, 2);
  sum += __shfl_xor(sum, 4);
  if (part == 0) {
    s_row[r] = sum;  // (0 beyond the segment's last row)
    if (t < seg.rows) strength[seg.row_first + t] = sum;
  }
  const int any_nan = __syncthreads_or(nan);
  if (tid < 64) {
    long long v = tid < kBeatStrengthRows ? s_row[tid] : 0, sq = v * v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o), sq += __shfl_xor(sq, o);
    if (tid == 0) {
      int64_t* a = acc + c * kBeatAccStride;
      if (v) add64(a, v), add64(a + 1, sq);
      if (any_nan) atomicOr(reinterpret_cast<unsigned long long*>(a + 2), 1ull);
    }
  }
}

constexpr int kTempoStage = kBeatTempoRows + kBeatMaxLag + kBeatTempoLags;  // 576: the tile's rows and the widest lag behind them

__global__ __launch_bounds__(256) void beat_tempo_kernel(const BeatParams* __restrict__ params, const BeatSeg* __restrict__ segs,
                                                         int64_t n_segs, const int32_t* __restrict__ strength, int64_t* __restrict__ acc) {
  __shared__ int s_o[kTempoStage];
  __shared__ long long s_part[4][kBeatTempoLags];
  static_assert(kBeatTempoLags == 64 && kBeatTempoRows == 256, "a lane a lag, a wave a quarter of the rows");
  const int tid = threadIdx.x, lq = tid & 63, rq = tid >> 6;
  const int64_t tile = blockIdx.x;
  const int64_t c = segment_of<&BeatSeg::tile_first>(segs, n_segs, tile);
  const BeatSeg seg = segs[c];
  const int64_t last_lag = params->lag_max < seg.rows - 1 ? params->lag_max : seg.rows - 1;
  const int64_t local = tile - seg.tile_first;
  const int64_t t0 = local / seg.lag_tiles * kBeatTempoRows;
  const int L = params->lag_min + (int)(local % seg.lag_tiles) * kBeatTempoLags + lq;  // <= last_lag + 63 <= 319
  for (int i = tid; i < kTempoStage; i += 256) s_o[i] = t0 + i < seg.rows ? strength[seg.row_first + t0 + i] : 0;
  __syncthreads();
  long long a = 0;
#pragma unroll 8
  for (int j = 0; j < 64; ++j) {
    const int t = rq * 64 + j;  // t + L <= 255 + 319 < kTempoStage
    a += (long long)s_o[t] * s_o[t + L];
  }
  s_part[rq][lq] = a;
  __syncthreads();
  if (tid < 64) {
    a = (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]);
    if (L <= last_lag && a) add64(acc + c * kBeatAccStride + kBeatAccLags + L, a);
  }
}

// kWaves: the frames of a block computed at once (1: frame by frame, the form the block-parallel one is measured against).
// kStaged: the backtrace walks tiles of predecessors in LDS; false: lane 0 walks the pool in global memory (measured against).
template <int kWaves, bool kStaged>
__global__ __launch_bounds__(kWaves * 64) void beat_path_kernel(const BeatParams* __restrict__ params, const BeatSeg* __restrict__ segs,
                                                                const int32_t* __restrict__ strength, int64_t* __restrict__ acc,
                                                                uint16_t* __restrict__ pred_pool, int32_t* __restrict__ beats,
                                                                BeatSummary* __restrict__ summaries) {
  constexpr int kThreads = kWaves * 64, kFill = kBeatRing / kThreads;
  static_assert(kBeatRing >= 2 * kBeatMaxLag + kBeatMaxLag / 2 && (kBeatRing & (kBeatRing - 1)) == 0, "the ring holds dmax + one block of dmin");
  static_assert(kBeatRing % kThreads == 0, "a refill is whole rounds of the workgroup");
  __shared__ long long s_C[kBeatRing];
  __shared__ int s_o[2 * kBeatRing];
  __shared__ long long s_pen[2 * kBeatMaxLag + 1];
  __shared__ long long s_S[kBeatMaxLag + 2];
  __shared__ int s_walk[2];  // where the walk stands (-1: at a start), the beats so far
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const BeatSeg seg = segs[c];
  int64_t* a = acc + c * kBeatAccStride;
  const int64_t rows = seg.rows;
  const int lag_min = params->lag_min;
  const int last_lag = (int)(params->lag_max < rows - 1 ? params->lag_max : rows - 1);
  if (tid == 0) a[kBeatAccClocks] = (int64_t)wall_clock64();
  const int early = a[2] ? 1 : (rows - 1 < lag_min ? 2 : 0);
  if (early) {  // (uniform)
    if (tid == 0) summaries[c] = BeatSummary{early, 0, 0, 0, 0.0};
    return;
  }
  // the period: S[L] = A[L] * prior[L], its first maximum
  for (int L = lag_min + tid; L <= last_lag + 1; L += kThreads) s_S[L] = L <= last_lag ? a[kBeatAccLags + L] * params->prior[L] : 0;
  __syncthreads();
  long long best = -1;
  int P = lag_min;
  for (int L = lag_min + lane; L <= last_lag; L += 64) {
    const long long v = s_S[L];
    if (v > best) best = v, P = L;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(P, o);
    if (ov > best || (ov == best && oi < P)) best = ov, P = oi;
  }
  if (best == 0) {  // (uniform) no pulse
    if (tid == 0) summaries[c] = BeatSummary{2, 0, 0, 0, 0.0};
    return;
  }
  // the scale and the penalties (a product of two strengths is above 0: so is their sum)
  const long long m = a[1] / a[0];
  const int dmin = P / 2 > 1 ? P / 2 : 1, dmax = 2 * P;
  for (int d = dmin + tid; d <= dmax; d += kThreads) s_pen[d] = (long long)params->tightness * m * (d - P) * (d - P) / ((long long)P * P);
  for (int i = tid; i < 2 * kBeatRing; i += kThreads) s_o[i] = i < rows ? strength[seg.row_first + i] : 0;
  __syncthreads();
  const int nk = (dmax - dmin + 64) / 64;  // candidates a lane, at most 7
  // A lane's candidates are the same gaps for every frame: what a gap adds to a ring entry is a constant of the lane.  The
  // ring holds C << 10, so a candidate's key (C - pen + 2^44) << 10 | 1023 - d is ONE 64-bit addition, ring entry + gap_key.  A
  // lane beyond dmax takes dmax again: the same key twice changes no maximum, and no lane needs a predicate.
  int gap[7];
  long long gap_key[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    gap[k] = dmin + lane + 64 * k < dmax ? dmin + lane + 64 * k : dmax;
    gap_key[k] = (long long)(((unsigned long long)(kBias - s_pen[gap[k]]) << 10) | (unsigned long long)(1023 - gap[k]));
  }
  if (tid == 0) a[kBeatAccClocks + 1] = (int64_t)wall_clock64();
  uint16_t* __restrict__ pred = pred_pool + seg.row_first;
  // the recurrence, a block of dmin frames between two barriers
  int64_t refill = kBeatRing;  // when a block starts at or behind this row, rows [refill + ring, refill + 2 ring) replace [refill - ring, refill)
  for (int64_t tb = 0; tb < rows; tb += dmin) {
    const int64_t te = tb + dmin < rows ? tb + dmin : rows;
    const bool fill = tb >= refill;  // (uniform; a block is at most 128 frames, so it ends inside the chunk that is there)
    int held[kFill];
    if (fill) {
#pragma unroll
      for (int i = 0; i < kFill; ++i) {
        const int64_t r = refill + kBeatRing + tid + (int64_t)i * kThreads;
        held[i] = r < rows ? strength[seg.row_first + r] : 0;
      }
    }
    const bool whole = tb >= dmax;  // (uniform) every gap of every frame of the block reaches a frame: no test of d <= t
    for (int t = (int)tb + wave; t < (int)te; t += kWaves) {
      unsigned long long key = kStartKey;
      const long long own = (long long)s_o[t & (2 * kBeatRing - 1)] << 10;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        if (k < nk) {  // (uniform)
          const unsigned long long cand = (unsigned long long)s_C[(t - gap[k]) & (kBeatRing - 1)] + (unsigned long long)gap_key[k];  // (read whatever is there)
          if ((whole || gap[k] <= t) && cand > key) key = cand;
        }
      }
      key = wave_max64(key);
      if (lane == 0) {
        s_C[t & (kBeatRing - 1)] = own + (long long)((key & ~1023ull) - ((unsigned long long)kBias << 10));
        pred[t] = (uint16_t)(1023 - (int)(key & 1023));
      }
    }
    if (fill) {
#pragma unroll
      for (int i = 0; i < kFill; ++i) s_o[(refill + kBeatRing + tid + (int64_t)i * kThreads) & (2 * kBeatRing - 1)] = held[i];
      refill += kBeatRing;
    }
    lds_barrier();  // (LDS alone is handed on: the predecessor stores stay in flight, a __syncthreads() here waited for each)
  }
  __syncthreads();  // the predecessors are in memory for whoever walks them
  if (tid == 0) a[kBeatAccClocks + 2] = (int64_t)wall_clock64();
  // the ending: the first maximum of C over the last P frames (every wave for itself)
  const int64_t from = rows - P > 0 ? rows - P : 0;
  unsigned long long ek = 0;
  for (int64_t t = from + lane; t < rows; t += 64) {
    const unsigned long long cand = (unsigned long long)s_C[t & (kBeatRing - 1)] | (unsigned long long)(1023 - (t - from));  // (the ring holds C << 10)
    if (cand > ek) ek = cand;
  }
  ek = wave_max64(ek);
  const int64_t end = from + 1023 - (int64_t)(ek & 1023);
  // the backtrace: last beat first
  int32_t* __restrict__ out = beats + seg.beat_first;
  int64_t n = 0;
  if (kStaged) {
    uint16_t* s_tile = reinterpret_cast<uint16_t*>(s_o);
    int64_t cur = end;
    for (;;) {
      const int64_t lo = cur - (kPredTile - 1) > 0 ? cur - (kPredTile - 1) : 0;
      for (int64_t i = tid; i <= cur - lo; i += kThreads) s_tile[i] = pred[lo + i];
      __syncthreads();
      if (tid == 0) {
        int64_t t = cur;
        for (;;) {
          if (n < seg.beat_cap) out[n] = (int32_t)t;
          ++n;
          const int d = s_tile[t - lo];
          t = d ? t - d : -1;
          if (t < lo) break;
        }
        s_walk[0] = (int)t, s_walk[1] = (int)n;
      }
      __syncthreads();
      cur = s_walk[0];
      if (cur < 0) break;  // (uniform)
    }
  } else if (tid == 0) {
    for (int64_t t = end; t >= 0;) {
      if (n < seg.beat_cap) out[n] = (int32_t)t;
      ++n;
      const int d = pred[t];
      t = d ? t - d : -1;
    }
  }
  if (tid == 0) {
    double refined = (double)P;
    if (lag_min < P && P < last_lag) {
      const double l = (double)s_S[P - 1], mid = (double)s_S[P], r = (double)s_S[P + 1];
      if (mid > l && mid > r) {
        const double num = 0.5 * (l - r), twice = 2.0 * mid, den = (l - twice) + r;
        refined = (double)P + num / den;
      }
    }
    summaries[c] = BeatSummary{0, P, n, best, refined};
    a[kBeatAccClocks + 3] = (int64_t)wall_clock64();
  }
}

// which form of the path kernel: the product library has one; the A/B library measures the other two (BP_BEAT_PATH=serial:
// frame by frame in one wave; =walk: the backtrace in global memory)
int path_form() {
  static const int form = [] {
    const char* e = ab_env("BP_BEAT_PATH");
    return e && std::strcmp(e, "serial") == 0 ? 1 : (e && std::strcmp(e, "walk") == 0 ? 2 : 0);
  }();
  return form;
}

}  // namespace

hipError_t launch_beats(const float* onset, const BeatParams* params, const BeatSeg* segs, int64_t n_segs, int64_t n_blocks,
                        int64_t n_tiles, int32_t* strength, int64_t* acc, uint16_t* pred, int32_t* beats, BeatSummary* summaries,
                        hipStream_t s) {
  if (n_segs <= 0) return hipSuccess;
  if (n_blocks < 1 || n_blocks > 0x7fffffffll || n_tiles < 0 || n_tiles > 0x7fffffffll || n_segs > 0x7fffffffll) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(acc, 0, (size_t)n_segs * kBeatAccStride * sizeof(int64_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(beat_strength_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, onset, params, segs, n_segs, strength, acc);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (n_tiles > 0) {
    hipLaunchKernelGGL(beat_tempo_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, params, segs, n_segs, strength, acc);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const int form = path_form();
  if (form == 1)
    hipLaunchKernelGGL((beat_path_kernel<1, true>), dim3((unsigned)n_segs), dim3(64), 0, s, params, segs, strength, acc, pred, beats, summaries);
  else if (form == 2)
    hipLaunchKernelGGL((beat_path_kernel<kBeatPathWaves, false>), dim3((unsigned)n_segs), dim3(kBeatPathWaves * 64), 0, s, params, segs, strength,
                       acc, pred, beats, summaries);
  else
    hipLaunchKernelGGL((beat_path_kernel<kBeatPathWaves, true>), dim3((unsigned)n_segs), dim3(kBeatPathWaves * 64), 0, s, params, segs, strength,
                       acc, pred, beats, summaries);
  return hipGetLastError();
}

}  // namespace bp
