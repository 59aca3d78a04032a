// Forced alignment on the device (include/basic_pitch_amd_align.h): the states of a score against the note and
// onset rows of a segment by the header's monotone recurrence.  Two kernels, stream-ordered.
//
// EMISSIONS (align_emit_kernel).  g[t][j] and b[t][j] are [rows x 88] . [88 x S] twice, note / active and onset / begins, and
// run on the f16 matrix cores (v_mfma_f32_32x32x16_f16), a wave per tile of 32 rows x 32 states, K = 88 padded to 96 with
// zeros: six instructions per map.  THE PRODUCT IS EXACT.  The A operand is q(x), an integer 0 ... 1024, and every integer up
// to 2048 is an f16; the B operand is 0 or 1.  Every product is therefore an integer of at most 1024, every partial sum of the
// 96 an integer of at most 88 x 1024 = 90,112 < 2^24, and fp32 adds integers below 2^24 without rounding: the accumulators
// hold the exact sums whatever order the instruction adds in, and (int) of them is the header's integer.  That is why the
// definition quantises to 1024.  The maps are quantised as they are loaded (two 16-byte loads a lane and step, a row is 352
// bytes), the NaN flag comes from the same loads — every tile reads all 88 pitches of its rows, and every row is in a tile —
// and is complete when the kernel ends, before the next one writes anything.  A lane builds its B fragments from the bit
// masks of ITS state (column lane & 31) once, eight bits a step, before the loop.  What leaves is 8 bytes a cell: g and g + b.
//
// RECURRENCE AND BACKTRACE (align_path_kernel).  A WORKGROUP TAKES A SEGMENT; lane `tid` holds states tid, tid + lanes, ...
// (up to four), so that the loads of a wave are 64 consecutive cells.  D is int64 in registers; "unreachable" is -2^62, and a
// reachable D is at most rows x 88 x 1024 x 17 < 2^44 in magnitude, so the two never meet.  The neighbour's D[t-1][j-1] is
// the lane below: a data-parallel shift by one lane within the wave, and for lane 0 of a wave the value lane 63 of the wave
// below left in LDS (for wave 0, of the last wave at the lane's previous state), double-buffered: ONE barrier per frame.
// The gains do not depend on the chain and are read kDepth frames ahead by unconditional loads into named registers.  The
// predecessor is ONE BIT per cell: the ballot of "entered", a 64-bit word per wave and state index, stored by lane 0.
// Backtrace: tiles of kAlignTileRows rows of those words come back to LDS by all lanes, lane 0 walks the tile and stores
// first_frame where the path enters a state — stores, no chain of dependent global loads — and everyone leaves when state 0
// is reached.  No indexed register array, no recursion, no inline assembly: no scratch.
#include "bp_kernels.h"

namespace bp {

namespace {

constexpr int kPitches = 88, kTile = kAlignTileRows;
constexpr int64_t kUnreachable = -(1ll << 62), kHalf = -(1ll << 61);  // reachable: above kHalf

__device__ __forceinline__ _Float16 quantise(float x) {
  return (_Float16)floorf(fminf(fmaxf(x, 0.0f), 1.0f) * 1024.0f + 0.5f);  // 0 ... 1024: exact in f16
}

// the segment of tile `tile`: the last one whose tile_first is <= tile (tile_first ascends; the tiles of a segment are one run)
__device__ __forceinline__ int64_t segment_of(const AlignSeg* __restrict__ segs, int64_t n, int64_t tile) {
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (segs[mid].tile_first <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void align_emit_kernel(const float* __restrict__ note, const float* __restrict__ onset,
                                                         const AlignState* __restrict__ states, const AlignSeg* __restrict__ segs,
                                                         int64_t n_segs, int64_t n_tiles, int threshold_q, int onset_weight,
                                                         int2* __restrict__ gains, uint32_t* __restrict__ nan_flags) {
  const int lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // a wave a tile
  if (tile >= n_tiles) return;                                         // (wave-uniform)
  const int64_t c = segment_of(segs, n_segs, tile);
  const AlignSeg seg = segs[c];
  const int S = seg.n_states, blocks = (S + 31) / 32;
  const int64_t local = tile - seg.tile_first;
  const int64_t t0 = local / blocks * 32;
  const int j0 = (int)(local % blocks) * 32;
  const int r = lane & 31, h = lane >> 5;
  const int64_t t_own = t0 + r < seg.rows ? t0 + r : seg.rows - 1;  // (a row past the end: the last row again, not stored)
  const float* nrow = note + (seg.row_first + t_own) * kPitches;
  const float* orow = onset + (seg.row_first + t_own) * kPitches;
  const int j = j0 + r;
  uint64_t act[2] = {0, 0}, beg[2] = {0, 0};
  if (j < S) {
    const AlignState st = states[seg.state_first + j];
    act[0] = st.active[0], act[1] = st.active[1], beg[0] = st.begins[0], beg[1] = st.begins[1];
  }
  const int n_act = __popcll(act[0]) + __popcll(act[1]);
  f32x16 acc_n, acc_o;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc_n[i] = 0.0f, acc_o[i] = 0.0f;
  bool bad = false;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const int k0 = 16 * s + 8 * h;  // this lane's eight pitches of the step
    f16x8 a_n, a_o, b_n, b_o;
    if (k0 < kPitches) {
      const float4 n0 = *reinterpret_cast<const float4*>(nrow + k0), n1 = *reinterpret_cast<const float4*>(nrow + k0 + 4);
      const float4 o0 = *reinterpret_cast<const float4*>(orow + k0), o1 = *reinterpret_cast<const float4*>(orow + k0 + 4);
      const float vn[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
      const float vo[8] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        bad = bad || vn[i] != vn[i] || vo[i] != vo[i];
        a_n[i] = quantise(vn[i]), a_o[i] = quantise(vo[i]);
      }
    } else {  // pitches 88 ... 95: the padding
#pragma unroll
      for (int i = 0; i < 8; ++i) a_n[i] = (_Float16)0.0f, a_o[i] = (_Float16)0.0f;
    }
    const unsigned bits_n = (unsigned)(act[k0 >> 6] >> (k0 & 63)) & 0xffu, bits_o = (unsigned)(beg[k0 >> 6] >> (k0 & 63)) & 0xffu;
#pragma unroll
    for (int i = 0; i < 8; ++i) b_n[i] = (_Float16)(float)((bits_n >> i) & 1u), b_o[i] = (_Float16)(float)((bits_o >> i) & 1u);
    acc_n = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_n, b_n, acc_n, 0, 0, 0);
    acc_o = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_o, b_o, acc_o, 0, 0, 0);
  }
  if (__any(bad) && lane == 0) atomicOr(&nan_flags[c], 1u);
  if (j >= S) return;
  // C: the column (state) is lane & 31, register i holds row (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
  int2* out = gains + seg.cell_first + j;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t t = t0 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (t < seg.rows) {
      const int g = (int)acc_n[i] - threshold_q * n_act;
      out[t * S] = make_int2(g, g + onset_weight * (int)acc_o[i]);
    }
  }
}

// lane l takes the value of lane l - 1 of its wave (wave_shr:1); lane 0 keeps its own
__device__ __forceinline__ int64_t from_lane_below(int64_t v) {
  const int lo = (int)(uint32_t)(uint64_t)v, hi = (int)(uint32_t)((uint64_t)v >> 32);
  const uint32_t l = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
  const uint32_t u = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
  return (int64_t)(((uint64_t)u << 32) | l);
}

// kL lanes, kK states a lane (state k * kL + tid), kD frames of gains ahead
template <int kL, int kK, int kD>
__global__ __launch_bounds__(kL) void align_path_kernel(const int2* __restrict__ gains, const AlignState* __restrict__ states,
                                                        const AlignSeg* __restrict__ segs, const uint32_t* __restrict__ nan_flags,
                                                        uint64_t* __restrict__ pred_pool, int32_t* __restrict__ first_frame,
                                                        int64_t* __restrict__ total, int32_t* __restrict__ status) {
  constexpr int kW = kL / 64, kMaxWords = kL * kK / 64;
  __shared__ int64_t s_edge[2][kK * kW];
  __shared__ uint64_t s_tile[kTile * kMaxWords];
  __shared__ int64_t s_final;
  __shared__ int s_state;
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const AlignSeg seg = segs[c];
  const int S = seg.n_states, words = (S + 63) / 64;
  const int64_t rows = seg.rows;
  int32_t* ff = first_frame + seg.state_first;
  const auto refuse = [&](int why) {
    for (int j = tid; j < S; j += kL) ff[j] = -1;
    if (tid == 0) total[c] = 0, status[c] = why;
  };
  if (nan_flags[c] != 0) return refuse(1);
  if (S > rows) return refuse(2);  // (no path, and nothing to walk)
  uint64_t* pred = pred_pool + seg.pred_first;

  int32_t earliest[kK], latest[kK];
  const int2* cells = gains + seg.cell_first;  // (a segment's cells are below 2^28: 32-bit indices from here)
  uint32_t jc[kK];
  int64_t D[kK];
#pragma unroll
  for (int k = 0; k < kK; ++k) {
    const int j = k * kL + tid;
    earliest[k] = INT32_MAX, latest[k] = INT32_MAX;  // a lane without a state never enters
    if (j < S) {
      const AlignState st = states[seg.state_first + j];
      earliest[k] = st.earliest, latest[k] = st.latest;
    }
    jc[k] = (uint32_t)(j < S ? j : S - 1);  // (such a lane reads the last state's cells and uses nothing of them)
    D[k] = kUnreachable;
  }

  // ---- forward
  // Every load is unconditional (a row past the end is the last row again): a load under a branch is waited for where the
  // branch joins, which puts the latency of HBM on every frame.
  int2 e[kD][kK];
#pragma unroll
  for (int d = 0; d < kD; ++d)
#pragma unroll
    for (int k = 0; k < kK; ++k) e[d][k] = cells[(uint32_t)((d < rows ? d : rows - 1) * S) + jc[k]];
  const auto frame = [&](int64_t t, const int2 (&cell)[kK]) {
    const int par = (int)(t & 1), q = par ^ 1;
#pragma unroll
    for (int k = 0; k < kK; ++k) {
      // D[t-1][j-1]: the D[k] of the lane below, taken before this lane's own is written (the states of one k alone meet here)
      int64_t up = from_lane_below(D[k]);
      if (lane == 0) {
        const int edge = k * kW + wave;
        up = edge > 0 && t > 0 ? s_edge[q][edge - 1] : kUnreachable;
      }
      const int64_t g = cell[k].x, eg = cell[k].y;
      int64_t stay = D[k] > kHalf ? D[k] + g : kUnreachable;
      int64_t enter = up > kHalf && earliest[k] <= t && t <= latest[k] ? up + eg : kUnreachable;
      if (t == 0) stay = kUnreachable, enter = k == 0 && tid == 0 && earliest[0] <= 0 ? eg : kUnreachable;
      const bool take = enter > stay;
      D[k] = take ? enter : stay;
      const unsigned long long entered = __ballot(take && t > 0);
      if (lane == 0 && k * kL + wave * 64 < S) pred[t * words + k * kW + wave] = entered;
      if (lane == 63) s_edge[par][k * kW + wave] = D[k];
    }
    __syncthreads();
  };
  int64_t base = 0;
  for (; base + kD <= rows; base += kD) {
#pragma unroll
    for (int d = 0; d < kD; ++d) {
      const int64_t t = base + d, ahead = t + kD < rows ? t + kD : rows - 1;
      int2 cell[kK];
#pragma unroll
      for (int k = 0; k < kK; ++k) cell[k] = e[d][k], e[d][k] = cells[(uint32_t)(ahead * S) + jc[k]];
      frame(t, cell);
    }
  }
#pragma unroll
  for (int d = 0; d < kD; ++d)  // the last rows, fewer than the depth: they are in the registers
    if (base + d < rows) frame(base + d, e[d]);

  // ---- the end of the path
#pragma unroll
  for (int k = 0; k < kK; ++k)
    if (k * kL + tid == S - 1) s_final = D[k];
  if (tid == 0) s_state = S - 1;
  __syncthreads();
  const int64_t end = s_final;
  if (!(end > kHalf)) return refuse(2);

  // ---- backtrace, a tile at a time from the end
  int j = S - 1;  // lane 0's
  for (int64_t t0 = (rows - 1) / kTile * kTile; t0 >= 0; t0 -= kTile) {
    if (s_state == 0) break;  // (uniform: written before the last barrier)
    const int len = (int)(rows - t0 < kTile ? rows - t0 : kTile);
    const uint64_t* src = pred + t0 * words;
    for (int i = tid; i < len * words; i += kL) s_tile[i] = src[i];
    __syncthreads();  // (and the frames' stores of this workgroup are visible to its loads)
    if (tid == 0) {
      for (int r = len - 1; r >= 0 && j > 0; --r) {
        const int64_t t = t0 + r;
        if (t > 0 && ((s_tile[r * words + (j >> 6)] >> (j & 63)) & 1ull)) ff[j--] = (int32_t)t;
      }
      s_state = j;
    }
    __syncthreads();
  }
  if (tid == 0) ff[0] = 0, total[c] = end, status[c] = 0;
}

template <int kL, int kK, int kD>
void launch_path(const int2* gains, const AlignState* states, const AlignSeg* segs, int64_t n_segs, const uint32_t* nan_flags,
                 uint64_t* pred, int32_t* first_frame, int64_t* total, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL((align_path_kernel<kL, kK, kD>), dim3((unsigned)n_segs), dim3(kL), 0, s, gains, states, segs, nan_flags, pred,
                     first_frame, total, status);
}

}  // namespace

hipError_t launch_align(const float* note, const float* onset, const AlignState* states, const AlignSeg* segs, int64_t n_segs,
                        int64_t n_tiles, int max_states, int threshold_q, int onset_weight, void* gains, uint64_t* pred,
                        uint32_t* nan_flags, int32_t* first_frame, int64_t* total, int32_t* status, hipStream_t s) {
  if (n_segs <= 0) return hipSuccess;
  if (max_states < 1 || max_states > kAlignMaxStates || n_tiles < 1 || (n_tiles + 3) / 4 > 0x7fffffffll || n_segs > 0x7fffffffll)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(nan_flags, 0, (size_t)n_segs * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  int2* g = static_cast<int2*>(gains);
  hipLaunchKernelGGL(align_emit_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, s, note, onset, states, segs, n_segs, n_tiles,
                     threshold_q, onset_weight, g, nan_flags);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (max_states <= kAlignSmallLanes)
    launch_path<kAlignSmallLanes, 1, kAlignReadAhead>(g, states, segs, n_segs, nan_flags, pred, first_frame, total, status, s);
  else if (max_states <= kAlignLanes)
    launch_path<kAlignLanes, 1, kAlignReadAhead>(g, states, segs, n_segs, nan_flags, pred, first_frame, total, status, s);
  else if (max_states <= 2 * kAlignLanes)
    launch_path<kAlignLanes, 2, kAlignReadAhead>(g, states, segs, n_segs, nan_flags, pred, first_frame, total, status, s);
  else
    launch_path<kAlignLanes, 4, kAlignReadAheadWide>(g, states, segs, n_segs, nan_flags, pred, first_frame, total, status, s);
  return hipGetLastError();
}

}  // namespace bp
