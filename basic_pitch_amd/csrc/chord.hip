// Chords and key on the device (include/basic_pitch_amd_chord.h): the note rows of a segment become a chroma per
// row, the chroma of a segment with boundaries sums per unit, and the units a path over the states by the header's Potts
// recurrence.  Every number is the header's integer, so sums may be taken in any order.  Four kernels, stream-ordered.
//
// CHROMA (chord_chroma_kernel).  Row-parallel over all segments: a block takes kChordChromaRows rows of ONE segment, which are
// one run of 16-byte words (a row is 22 of them), quantises them into LDS — the NaN flag comes from the same loads and covers
// all 88 pitches whatever the band — and folds them, sixteen lanes a row and a lane a class, to one 32-byte row of uint16[16].
// sum c, sum c^2 and Ctot[12] are reduced in the block and added by one integer atomic per value per block.
//
// POOL (chord_pool_kernel).  Only the units of segments with boundaries: sixteen lanes a unit, a lane a class, 32 bytes a step;
// lane 12 carries the unit's length.  Nothing of it waits for the recurrence.
//
// PATH (chord_path_kernel).  A WAVE TAKES A SEGMENT and a lane a state; the waves of a workgroup share nothing, so NO BARRIER
// sits on the chain.  The lane's 12 weights and bias * m are registers.  The unit's sums are the same for every lane: the wave
// fetches the NEXT chunk of kChordChunk units while it walks this one (a lane a unit, held in registers, stored to the other
// half of the wave's LDS at the chunk's end) and reads a unit's sums from LDS one unit ahead of its use.  A step is: the
// emission (off the chain), the packed key (D + 2^48) << 6 | 63 - s, its maximum over the wave by DPP (wave_max64), the strict
// comparison, whose ballot IS the record's predecessor mask, and one select.  Lanes beyond n_states hold D = -2^48: key below
// every state's, never updated.  D starts at 0, so unit 0 needs no case of its own (nothing exceeds 0 - pen).  The key is
// picked in the same kernel by the same reduction.  Backtrace: tiles of kChordTraceTile records come to the wave's LDS by all
// lanes (the chunks' buffer is free by then), the walk reads them there, the tile's labels leave by all lanes.
//
// LABEL (chord_label_kernel).  A byte a row: the row's unit (with boundaries: by bisection) and that unit's label, 0 under a
// status.  No indexed register array, no recursion, no inline assembly: no scratch.
#include "bp_kernels.h"

#pragma clang fp contract(off)
#pragma clang fp reassociate(off)

namespace bp {

namespace {

constexpr int kPitches = 88, kRowVecs = kPitches / 4, kTileVecs = kChordChromaRows * kRowVecs;
constexpr int kLanesPerRow = 16;  // a chroma row: 12 classes and 4 zeros (pool: the length at 12)
constexpr long long kBias = 1ll << 48;
static_assert(kChordClasses == 12 && kChordMaxStates == 64, "a lane a state, a row of 16 entries");
static_assert(kChordTraceTile * 16 == 2 * kChordChunk * 64, "the backtrace's tile is the two chunk buffers of a wave");

__device__ __forceinline__ int quantise(float x) { return (int)floorf(fminf(fmaxf(x, 0.0f), 1.0f) * 1024.0f + 0.5f); }

// the segment of block / unit / row `at`: the last one whose first is <= at (the firsts ascend; a segment without any shares
// its first with the next one that has some)
template <int64_t ChordSeg::*kFirst>
__device__ __forceinline__ int64_t segment_of(const ChordSeg* __restrict__ segs, int64_t n, int64_t at) {
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (segs[mid].*kFirst <= at) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void add64(int64_t* at, long long v) { atomicAdd(reinterpret_cast<unsigned long long*>(at), (unsigned long long)v); }

__global__ __launch_bounds__(256) void chord_chroma_kernel(const float* __restrict__ note, const ChordParams* __restrict__ params,
                                                           const ChordSeg* __restrict__ segs, int64_t n_segs,
                                                           uint16_t* __restrict__ chroma, int64_t* __restrict__ acc) {
  __shared__ uint2 s_q[kTileVecs];  // the tile quantised, above the threshold and inside the band: four uint16 a word
  __shared__ int s_cls[4][kLanesPerRow];
  __shared__ long long s_sq[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int64_t c = segment_of<&ChordSeg::blk_first>(segs, n_segs, b);
  const ChordSeg seg = segs[c];
  const int thr = params->threshold_q, lo = params->min_pitch, hi = params->max_pitch;
  const int64_t t0 = (b - seg.blk_first) * kChordChromaRows;
  const int n_rows = (int)(seg.rows - t0 < kChordChromaRows ? seg.rows - t0 : kChordChromaRows);
  const float4* __restrict__ tile = reinterpret_cast<const float4*>(note + (seg.row_first + t0) * kPitches);
  int nan = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = tid + 256 * k;
    if (i < n_rows * kRowVecs) {  // (<= kTileVecs: inside the segment's rows and inside s_q)
      const float4 v = tile[i];
      const float x[4] = {v.x, v.y, v.z, v.w};
      uint32_t q[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        nan |= x[e] != x[e];
        const int pitch = 4 * (i % kRowVecs) + e, above = quantise(x[e]) - thr;
        q[e] = pitch >= lo && pitch <= hi && above > 0 ? (uint32_t)above : 0u;
      }
      s_q[i] = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
    }
  }
  const int any_nan = __syncthreads_or(nan);
  const uint16_t* s_q16 = reinterpret_cast<const uint16_t*>(s_q);
  const int k = tid & (kLanesPerRow - 1);
  int cls = 0;
  long long sq = 0;
#pragma unroll
  for (int pass = 0; pass < kChordChromaRows / 16; ++pass) {
    const int r = (tid >> 4) + 16 * pass;
    if (r < n_rows) {
      int v = 0;
      if (k < kChordClasses)
        for (int p = (k + 3) % 12; p < kPitches; p += 12) v += s_q16[r * kPitches + p];  // class (p + 9) % 12 == k
      chroma[(seg.row_first + t0 + r) * kLanesPerRow + k] = (uint16_t)v;  // (<= 8 * 1024)
      cls += v, sq += (long long)v * v;
    }
  }
  cls += __shfl_xor(cls, 16);
  cls += __shfl_xor(cls, 32);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
  if (lane < kLanesPerRow) s_cls[wave][lane] = cls;
  if (lane == 0) s_sq[wave] = sq;
  __syncthreads();
  if (tid < 64) {
    const int total = tid < kLanesPerRow ? (s_cls[0][tid] + s_cls[1][tid]) + (s_cls[2][tid] + s_cls[3][tid]) : 0;
    int all = total;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) all += __shfl_xor(all, o);
    int64_t* a = acc + c * kChordAccStride;
    if (tid < kChordClasses && total) add64(a + kChordAccClasses + tid, total);
    if (tid == 0) {
      if (all) add64(a, all), add64(a + 1, (s_sq[0] + s_sq[1]) + (s_sq[2] + s_sq[3]));
      if (any_nan) atomicOr(reinterpret_cast<unsigned long long*>(a + 2), 1ull);
    }
  }
}

__global__ __launch_bounds__(256) void chord_pool_kernel(const ChordSeg* __restrict__ segs, int64_t n_segs, int64_t n_pool_units,
                                                         const int32_t* __restrict__ bounds, const uint16_t* __restrict__ chroma,
                                                         uint32_t* __restrict__ pool) {
  const int tid = threadIdx.x, k = tid & (kLanesPerRow - 1);
  const int64_t g = (int64_t)blockIdx.x * (256 / kLanesPerRow) + (tid >> 4);
  if (g >= n_pool_units) return;
  const ChordSeg seg = segs[segment_of<&ChordSeg::pool_first>(segs, n_segs, g)];
  const int64_t u = g - seg.pool_first;  // < seg.n_units, and the segment has n_units - 1 boundaries
  const int32_t* __restrict__ B = bounds + seg.bound_first;
  const int64_t first = u ? B[u - 1] : 0, end = u < seg.n_units - 1 ? B[u] : seg.rows;
  const uint16_t* __restrict__ rows = chroma + seg.row_first * kLanesPerRow + k;
  uint32_t sum = 0;
  for (int64_t t = first; t < end; ++t) sum += rows[t * kLanesPerRow];
  pool[g * kLanesPerRow + k] = k == kChordClasses ? (uint32_t)(end - first) : sum;
}

typedef short short2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ short2v as_short2(uint32_t v) { return __builtin_bit_cast(short2v, v); }

// what a wave's LDS hands from some lanes to others: its own operations are in order, the compiler must keep them so
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The recurrence over the units of one segment by one wave.  kPooled: a unit is 16 uint32 of `pool` (12 sums, the length),
// otherwise 16 uint16 of `chroma` and one frame long.  D: 0 in the lanes of states, -2^48 beyond; comes back as D[last].
template <bool kPooled>
__device__ __forceinline__ void chord_chain(const uint4* __restrict__ src, int64_t n_units, uint4* in, int lane, bool valid,
                                            const int (&w)[kChordClasses], const short2v (&w2)[kChordClasses / 2], long long bias_m, long long sp_m, uint4* __restrict__ rec,
                                            long long& D) {
  constexpr int kVecs = kPooled ? 4 : 2;  // 16-byte words a unit
  uint32_t held[4 * kVecs];  // (words, not uint4: an array of vectors copied under a condition stays in memory)
  if (lane < n_units) {
#pragma unroll
    for (int j = 0; j < kVecs; ++j) in[lane * kVecs + j] = src[lane * kVecs + j];
  }
  for (int64_t first = 0; first < n_units; first += kChordChunk) {
    const int buf = (int)(first / kChordChunk) & 1;
    const int64_t ahead = first + kChordChunk + lane;  // the unit this lane fetches for the next chunk
    const int64_t fetched = ahead < n_units ? ahead : n_units - 1;  // (beyond the end: the last unit again, not stored)
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
      const uint4 v = src[fetched * kVecs + j];
      held[4 * j] = v.x, held[4 * j + 1] = v.y, held[4 * j + 2] = v.z, held[4 * j + 3] = v.w;
    }
    wave_lds_fence();
    const uint4* chunk = in + buf * kChordChunk * kVecs;
    const int here = (int)(n_units - first < kChordChunk ? n_units - first : kChordChunk);
    uint4 next[kVecs];
#pragma unroll
    for (int j = 0; j < kVecs; ++j) next[j] = chunk[j];
    for (int i = 0; i < here; ++i) {
      uint4 cur[kVecs];
#pragma unroll
      for (int j = 0; j < kVecs; ++j) cur[j] = next[j];
      const int after = i + 1 < kChordChunk ? i + 1 : i;  // (inside the chunk's buffer; beyond `here` it is read and not used)
#pragma unroll
      for (int j = 0; j < kVecs; ++j) next[j] = chunk[after * kVecs + j];
      long long e, pen;
      if (kPooled) {
        const uint32_t cu[kChordClasses] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y,
                                            cur[1].z, cur[1].w, cur[2].x, cur[2].y, cur[2].z, cur[2].w};
        const long long len = cur[3].x;
        e = len * bias_m;
#pragma unroll
        for (int k = 0; k < kChordClasses; ++k) e += (long long)w[k] * (long long)cu[k];
        pen = len * sp_m;
      } else {
        const uint32_t pair[6] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y};
        int dot = 0;  // |dot| <= 12 * 2^10 * 2^13 < 2^31; weights and sums both fit int16: six v_dot2_i32_i16
#pragma unroll
        for (int k = 0; k < kChordClasses / 2; ++k) dot = __builtin_amdgcn_sdot2(w2[k], as_short2(pair[k]), dot, false);
        e = bias_m + dot;
        pen = sp_m;
      }
      const unsigned long long key = ((unsigned long long)(D + kBias) << 6) | (unsigned long long)(63 - lane);
      const unsigned long long top = wave_max64(key);
      const long long over = (long long)(top >> 6) - kBias - pen;
      const bool move = valid && over > D;
      const unsigned long long mask = __ballot(move);
      if (lane == 0) rec[first + i] = make_uint4((uint32_t)mask, (uint32_t)(mask >> 32), 63u - (uint32_t)(top & 63), 0u);
      if (valid) D = e + (move ? over : D);
    }
    wave_lds_fence();
    if (ahead < n_units) {
#pragma unroll
      for (int j = 0; j < kVecs; ++j)
        in[((buf ^ 1) * kChordChunk + lane) * kVecs + j] = make_uint4(held[4 * j], held[4 * j + 1], held[4 * j + 2], held[4 * j + 3]);
    }
  }
}

__global__ __launch_bounds__(kChordPathWaves * 64) void chord_path_kernel(const ChordParams* __restrict__ params,
                                                                          const ChordSeg* __restrict__ segs, int64_t n_segs,
                                                                          const uint16_t* __restrict__ chroma,
                                                                          const uint32_t* __restrict__ pool, int64_t* __restrict__ acc,
                                                                          uint4* __restrict__ records, uint8_t* __restrict__ unit_labels,
                                                                          ChordSummary* __restrict__ summaries) {
  __shared__ uint4 s_in[kChordPathWaves][2 * kChordChunk * 4];  // a wave's two chunks of units; then its tile of records
  __shared__ uint8_t s_lab[kChordPathWaves][kChordTraceTile];
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int64_t c = (int64_t)blockIdx.x * kChordPathWaves + wave;
  if (c >= n_segs) return;  // (no barrier below: a wave is on its own)
  const ChordSeg seg = segs[c];
  int64_t* a = acc + c * kChordAccStride;
  if (lane == 0) a[kChordAccClocks] = (int64_t)wall_clock64();
  const long long sum = a[0];
  const int early = a[2] ? 1 : (sum == 0 ? 2 : 0);
  if (early) {  // (uniform)
    if (lane == 0) summaries[c] = ChordSummary{early, -1, 0, 0, 0, 0};
    return;
  }
  const long long m = a[1] / sum;
  // the key: lane j < 24 has K[j]; the first maximum by the packed key
  long long K = 0;
  if (lane < 24) {
    const int mode = lane / 12, tonic = lane % 12;
#pragma unroll
    for (int k = 0; k < kChordClasses; ++k) K += (long long)params->key_profile[mode][(k - tonic + 12) % 12] * a[kChordAccClasses + k];
  }
  const unsigned long long key_top = wave_max64(lane < 24 ? ((unsigned long long)(K + kBias) << 6) | (unsigned long long)(63 - lane) : 0ull);
  const int n = params->n_states;
  const bool valid = lane < n;
  int w[kChordClasses];
#pragma unroll
  for (int k = 0; k < kChordClasses; ++k) w[k] = params->weights[lane][k];
  short2v w2[kChordClasses / 2];  // the same in pairs of int16 (|w| <= 1024) for the frame units' dot products
#pragma unroll
  for (int k = 0; k < kChordClasses / 2; ++k) w2[k] = short2v{(short)w[2 * k], (short)w[2 * k + 1]};
  const long long bias_m = (long long)params->bias[lane] * m, sp_m = (long long)params->switch_penalty * m;
  if (lane == 0) a[kChordAccClocks + 1] = (int64_t)wall_clock64();
  uint4* in = s_in[wave];
  uint4* __restrict__ rec = records + seg.unit_first;
  const int64_t n_units = seg.n_units;
  long long D = valid ? 0 : -kBias;
  if (seg.pooled)  // (uniform)
    chord_chain<true>(reinterpret_cast<const uint4*>(pool + seg.pool_first * kLanesPerRow), n_units, in, lane, valid, w, w2, bias_m, sp_m, rec, D);
  else
    chord_chain<false>(reinterpret_cast<const uint4*>(chroma + seg.row_first * kLanesPerRow), n_units, in, lane, valid, w, w2, bias_m, sp_m, rec, D);
  const unsigned long long end_top = wave_max64(((unsigned long long)(D + kBias) << 6) | (unsigned long long)(63 - lane));
  __threadfence();  // the records are in memory for the lanes that fetch them
  if (lane == 0) a[kChordAccClocks + 2] = (int64_t)wall_clock64();
  // the backtrace: the last tile first
  int cur = 63 - (int)(end_top & 63), changes = 0;
  uint8_t* lab = s_lab[wave];
  for (int64_t hi = n_units - 1; hi >= 0;) {
    const int64_t lo = hi - (kChordTraceTile - 1) > 0 ? hi - (kChordTraceTile - 1) : 0;
    const int count = (int)(hi - lo + 1);  // <= kChordTraceTile
    for (int i = lane; i < count; i += 64) in[i] = rec[lo + i];
    wave_lds_fence();
    for (int i = count - 1; i >= 0; --i) {
      const uint4 r = in[i];
      if (lane == 0) lab[i] = (uint8_t)cur;
      const unsigned long long mask = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
      if ((mask >> cur) & 1) ++changes, cur = __builtin_amdgcn_readfirstlane((int)r.z);  // (unit 0's mask is 0)
    }
    wave_lds_fence();
    for (int i = lane; i < count; i += 64) unit_labels[seg.unit_first + lo + i] = lab[i];
    wave_lds_fence();
    hi = lo - 1;
  }
  if (lane == 0) {
    summaries[c] = ChordSummary{0, 63 - (int)(key_top & 63), (int32_t)n_units, changes, (long long)(end_top >> 6) - kBias,
                                (long long)(key_top >> 6) - kBias};
    a[kChordAccClocks + 3] = (int64_t)wall_clock64();
  }
}

__global__ __launch_bounds__(256) void chord_label_kernel(const ChordSeg* __restrict__ segs, int64_t n_segs, int64_t n_rows,
                                                          const int32_t* __restrict__ bounds, const uint8_t* __restrict__ unit_labels,
                                                          const ChordSummary* __restrict__ summaries, uint8_t* __restrict__ labels) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n_rows) return;
  const int64_t c = segment_of<&ChordSeg::row_first>(segs, n_segs, g);
  const ChordSeg seg = segs[c];
  const int64_t t = g - seg.row_first;
  int64_t u = t;
  if (seg.pooled) {  // the boundaries at or before t: that many units lie before its own
    const int32_t* __restrict__ B = bounds + seg.bound_first;
    int64_t lo = 0, hi = seg.n_units - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (B[mid] <= t) lo = mid + 1; else hi = mid;
    }
    u = lo;
  }
  labels[g] = summaries[c].status ? (uint8_t)0 : unit_labels[seg.unit_first + u];
}

}  // namespace

hipError_t launch_chords(const float* note, const ChordParams* params, const ChordSeg* segs, int64_t n_segs, int64_t n_blocks,
                         int64_t n_rows, int64_t n_pool_units, const int32_t* bounds, uint16_t* chroma, uint32_t* pool, int64_t* acc,
                         void* records, uint8_t* unit_labels, uint8_t* labels, ChordSummary* summaries, hipStream_t s) {
  if (n_segs <= 0) return hipSuccess;
  if (n_blocks < 1 || n_blocks > 0x7fffffffll || n_rows < 1 || n_pool_units < 0 || n_pool_units > 0x7fffffffll || n_segs > 0x7fffffffll)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(acc, 0, (size_t)n_segs * kChordAccStride * sizeof(int64_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(chord_chroma_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, note, params, segs, n_segs, chroma, acc);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (n_pool_units > 0) {
    constexpr int kUnits = 256 / kLanesPerRow;
    hipLaunchKernelGGL(chord_pool_kernel, dim3((unsigned)((n_pool_units + kUnits - 1) / kUnits)), dim3(256), 0, s, segs, n_segs, n_pool_units,
                       bounds, chroma, pool);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(chord_path_kernel, dim3((unsigned)((n_segs + kChordPathWaves - 1) / kChordPathWaves)), dim3(kChordPathWaves * 64), 0, s,
                     params, segs, n_segs, chroma, pool, acc, static_cast<uint4*>(records), unit_labels, summaries);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(chord_label_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, s, segs, n_segs, n_rows, bounds, unit_labels,
                     summaries, labels);
  return hipGetLastError();
}

}  // namespace bp
