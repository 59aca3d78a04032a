// The melody of contour rows on the device (include/basic_pitch_amd_melody.h): one f0 track per decode by the
// header's Viterbi recurrence, its records written or — a scored sweep — counted against a reference track where they are.
//
// A WORKGROUP TAKES A DECODE, A LANE A STATE: lanes 0 ... 263 the bins, lane 264 the bookkeeping of the unvoiced state U; 320
// lanes, five waves.  The recurrence is serial over frames, so everything is arranged to make a frame short:
//
//   forward   What a frame leaves in LDS is P[t][b] = D[t][b] - D[t][U], double-buffered, with a halo of kMelodyMaxJump cells
//             of -inf on each side and -inf in the bins outside the band: the window of a voiced target is loads on either
//             side without a bounds test, unrolled so that they are issued together, and a candidate from outside the band
//             never wins (every candidate inside it is finite).  The unvoiced target needs the first maximum of P[b'] -
//             voicing_penalty over the band: each wave reduces its 64 lanes (wave_max, the first lane that holds it by ballot) and leaves a partial;
//             at the next frame EVERY lane combines the five partials, in wave order with a strict comparison, into D[t][U]
//             itself — that is the broadcast the normalisation needs, and it is why ONE barrier per frame is enough: a lane
//             writes P[t][b] and its wave's partial, the workgroup meets, and the next frame reads both.
//   emissions do not depend on the recurrence: a lane holds kMelodyReadAhead rows of its bin in registers (the frame loop
//             is unrolled by that depth, so the registers are named, not indexed) and asks for row t + depth when it takes
//             row t; the loads of a wave are 64 consecutive floats.  The not-finite / magnitude flag comes from these loads.
//   backtrace The predecessors (a byte per bin: the source's offset in the window, 255 for U; U's own source in 16 bits
//             behind them) went to the pool as the frames passed.  From the end, tiles of kMelodyTileRows rows come back to
//             LDS by 16-byte loads of all lanes, lane 0 walks the tile in LDS and leaves the bins, and a lane per row reads
//             its three cells, refines in float64 as multipitch.hip does, and stores 16 bytes — or counts.
//
// `#pragma clang fp contract(off) reassociate(off)` keeps every operation as the header writes it, so the records equal the
// host checker's bit for bit (tests/test_gpu_melody.py).  No indexed register array, no recursion: no scratch.
#include "bp_kernels.h"

#pragma clang fp contract(off)
#pragma clang fp reassociate(off)

namespace bp {

namespace {

constexpr int kLanes = 320, kWaves = kLanes / 64;
constexpr int kHalo = kMelodyMaxJump, kDepth = kMelodyReadAhead, kTile = kMelodyTileRows, kStride = kMelodyPredStride;
constexpr int kPRow = kMpBins + 2 * kHalo;  // 296
constexpr int kU = kMpBins;                 // the unvoiced state
constexpr int kFromU = 255;                 // a voiced target's predecessor byte: U
static_assert(kStride % 16 == 0 && kStride >= kMpBins + 2, "a row of predecessors is whole 16-byte words");
static_assert(kTile <= kLanes, "a lane per row of a tile");

// The maximum of a wave in every lane, by data-parallel primitives: within the rows of 16 lanes a lane takes the maximum
// with the lane 1, 2, 4 and 8 below it (a lane without one keeps its own value), lane 15 of a row then goes to the row above
// and lane 31 to the upper half, and lane 63 holds the wave's.  Six VALU operations instead of six trips through the LDS
// crossbar: the reduction is on the serial chain of every frame.
template <int kCtrl>
__device__ __forceinline__ float dpp_max(float v) {
  const int own = __float_as_int(v);
  return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(own, own, kCtrl, 0xf, 0xf, false)));
}
__device__ __forceinline__ float wave_max(float v) {
  v = dpp_max<0x111>(v);  // row_shr:1
  v = dpp_max<0x112>(v);  // row_shr:2
  v = dpp_max<0x114>(v);  // row_shr:4
  v = dpp_max<0x118>(v);  // row_shr:8
  v = dpp_max<0x142>(v);  // row_bcast:15
  v = dpp_max<0x143>(v);  // row_bcast:31
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
  return v;
}
__device__ __forceinline__ bool within(double d, const MpScoreParams& sp) {
  return sp.strict ? d < sp.pitch_tolerance_cents : d <= sp.pitch_tolerance_cents;
}
// the first maximum of the five wave partials, in wave order
__device__ __forceinline__ void first_max(const float* __restrict__ v, const int* __restrict__ i, float* best, int* arg) {
  float bv = v[0];
  int bi = i[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const float c = v[w];
    if (c > bv) bv = c, bi = i[w];
  }
  *best = bv, *arg = bi;
}

// kJ: the widest window the launch reads, max_jump of its sets rounded up to 4 or kMelodyMaxJump.  The window loop is
// unrolled to that width so that its LDS loads are issued together — as a loop of max_jump trips every load was waited for
// by itself, nine round trips to LDS a frame at the default.  The penalties pen[d] come from a table in LDS with +inf beyond
// the decode's own max_jump, so such a candidate is -inf (or NaN in the halo) and never taken; read from LDS once, they live
// in vector registers — as uniform values the compiler kept them and their predicates in scalar registers, and the wide
// form spilled 25 of those.
template <int kJ>
__global__ __launch_bounds__(kLanes) void melody_kernel(const float* __restrict__ contour, const MelodyParams* __restrict__ sets,
                                                        const MelodyDecode* __restrict__ dec, uint8_t* __restrict__ pred_pool,
                                                        uint4* __restrict__ points, const double* __restrict__ ref_pitch,
                                                        MpScoreParams sp, int64_t* __restrict__ scores, int32_t* __restrict__ status) {
  __shared__ float s_P[2][kPRow];
  __shared__ float s_part_v[2][kWaves];
  __shared__ int s_part_i[2][kWaves];
  __shared__ uint4 s_pred[kTile * kStride / 16];
  __shared__ int16_t s_bin[kTile];
  __shared__ unsigned long long s_cnt[kWaves][5];
  __shared__ float s_pen[kMelodyMaxJump + 1];
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MelodyDecode d = dec[c];
  const MelodyParams p = sets[d.set];
  const int64_t rows = d.rows;
  if (rows <= 0) {
    if (tid == 0) status[c] = 0;
    if (tid < 6 && scores) scores[6 * c + tid] = 0;
    return;
  }
  const float kNegInf = -__builtin_inff();
  const int b = tid;
  const bool bin_lane = b < kMpBins, in_band = bin_lane && b >= p.min_bin && b <= p.max_bin;
  const int J = p.max_jump;
  const float thr = p.threshold, jp = p.jump_penalty, vp = p.voicing_penalty;
  if (tid < kHalo) {
    s_P[0][tid] = kNegInf, s_P[1][tid] = kNegInf;
    s_P[0][kHalo + kMpBins + tid] = kNegInf, s_P[1][kHalo + kMpBins + tid] = kNegInf;
  }
  if (tid <= kMelodyMaxJump) s_pen[tid] = tid <= J ? jp * (float)tid : __builtin_inff();
  __syncthreads();
  float pen[kJ + 1];
#pragma unroll
  for (int i = 0; i <= kJ; ++i) pen[i] = s_pen[i];
  const float* col = contour + d.first * kMpBins + (bin_lane ? b : 0);  // (the lanes beyond the bins read bin 0 and use nothing of it)
  uint8_t* pred = pred_pool + d.pred_first * kStride;

  // ---- forward
  // Every load is unconditional (a row past the end is the last row again): a load under a branch is waited for where the
  // branch joins, which puts the latency of HBM on every frame.
  float e[kDepth];
#pragma unroll
  for (int k = 0; k < kDepth; ++k) e[k] = col[(k < rows ? k : rows - 1) * kMpBins];
  bool bad = false;
  float d_own = kNegInf, d_u = thr;  // D[t][b] of the lane's bin (-inf outside the band), D[t][U]
  const auto frame = [&](int64_t t, float cell) {
    bad = bad || !(fabsf(cell) <= 65536.0f);
    const int par = (int)(t & 1), q = par ^ 1;
    float best = 0.0f;
    if (t == 0) {
      d_u = thr;
    } else {
      float u_best;
      int u_from;
      first_max(s_part_v[q], s_part_i[q], &u_best, &u_from);
      if (0.0f > u_best) u_best = 0.0f, u_from = kU;  // P[U], exactly 0, last
      d_u = thr + u_best;
      if (tid == kU) *reinterpret_cast<uint16_t*>(pred + t * kStride + kU) = (uint16_t)u_from;
      if (in_band) {
        const float* w = &s_P[q][kHalo + b];
        best = kNegInf;
        int arg = 0;
#pragma unroll
        for (int dd = -kJ; dd <= kJ; ++dd) {
          const int far = dd < 0 ? -dd : dd;
          const float cand = w[dd] - pen[far];
          if (cand > best) best = cand, arg = dd + J;
        }
        const float from_u = 0.0f - vp;  // P[U] - voicing_penalty
        if (from_u > best) best = from_u, arg = kFromU;
        pred[t * kStride + b] = (uint8_t)arg;
      }
    }
    d_own = in_band ? cell + best : kNegInf;
    const float P = in_band ? d_own - d_u : kNegInf;
    const float to_u = in_band ? P - vp : kNegInf;
    if (bin_lane) s_P[par][kHalo + b] = P;
    const float m = wave_max(to_u);
    const unsigned long long holds = __ballot(to_u == m);
    if (lane == 0) s_part_v[par][wave] = m, s_part_i[par][wave] = 64 * wave + (holds ? __builtin_ctzll(holds) : 0);
    __syncthreads();
  };
  int64_t base = 0;
  for (; base + kDepth <= rows; base += kDepth) {
#pragma unroll
    for (int k = 0; k < kDepth; ++k) {
      const int64_t t = base + k, ahead = t + kDepth < rows ? t + kDepth : rows - 1;
      const float cell = e[k];
      e[k] = col[ahead * kMpBins];
      frame(t, cell);
    }
  }
#pragma unroll
  for (int k = 0; k < kDepth; ++k)  // the last rows, fewer than the depth: they are in the registers
    if (base + k < rows) frame(base + k, e[k]);
  // the last state: the first maximum of D[rows - 1] in state order (the partials of the frame before are read by now)
  {
    const int q = (int)(rows & 1);
    const float m = wave_max(d_own);
    const unsigned long long holds = __ballot(d_own == m);
    if (lane == 0) s_part_v[q][wave] = m, s_part_i[q][wave] = 64 * wave + (holds ? __builtin_ctzll(holds) : 0);
  }
  const bool any_bad = __syncthreads_or(bad) != 0;
  if (any_bad) {
    if (points)
      for (int64_t r = tid; r < rows; r += kLanes) points[d.first + r] = make_uint4(0xffffffffu, 0u, 0u, 0u);  // {-1, 0.0f, 0.0}
    if (tid == 0) status[c] = 1;
    if (tid < 6 && scores) scores[6 * c + tid] = tid == 0 ? rows : 0;
    return;
  }
  int state = kU;
  if (tid == 0) {
    float best;
    first_max(s_part_v[rows & 1], s_part_i[rows & 1], &best, &state);
    if (d_u > best) state = kU;
  }

  // ---- backtrace, a tile at a time from the end
  unsigned n_ref = 0, n_est = 0, n_both = 0, n_pitch = 0, n_chroma = 0;
  for (int64_t t0 = (rows - 1) / kTile * kTile; t0 >= 0; t0 -= kTile) {
    const int len = (int)(rows - t0 < kTile ? rows - t0 : kTile);
    const uint4* src = reinterpret_cast<const uint4*>(pred + t0 * kStride);  // (the pool and a row's stride are 16-byte aligned)
    for (int i = tid; i < len * (kStride / 16); i += kLanes) s_pred[i] = src[i];
    __syncthreads();  // (and the frames' stores of this workgroup are visible to its loads)
    if (tid == 0) {
      const uint8_t* tile = reinterpret_cast<const uint8_t*>(s_pred);
      for (int r = len - 1; r >= 0; --r) {
        s_bin[r] = (int16_t)(state == kU ? -1 : state);
        if (t0 + r > 0) {
          const uint8_t* row = tile + r * kStride;
          if (state == kU) {
            state = *reinterpret_cast<const uint16_t*>(row + kU);
          } else {
            const int a = row[state];
            state = a == kFromU ? kU : state + a - J;
          }
          state = state < 0 ? 0 : state > kU ? kU : state;  // (a state is 0 ... 264 by construction)
        }
      }
    }
    __syncthreads();
    if (tid < len) {
      const int64_t r = d.first + t0 + tid;
      const int bin = s_bin[tid];
      float cell = 0.0f;
      double pitch = 0.0;
      if (bin >= 0) {
        const float* row = contour + r * kMpBins;
        cell = row[bin];
        double delta = 0.0;
        if (bin >= 1 && bin <= kMpBins - 2) {
          const float lf = row[bin - 1], rf = row[bin + 1];
          if (cell > lf && cell > rf) {
            const double l = (double)lf, m = (double)cell, rr = (double)rf;
            delta = 0.5 * (l - rr) / ((l - 2.0 * m) + rr);
          }
        }
        pitch = 21.0 + ((double)bin + delta) / 3.0;
      }
      if (points) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(pitch);
        points[r] = make_uint4((unsigned)bin, __float_as_uint(cell), (unsigned)bits, (unsigned)(bits >> 32));
      } else {
        const double ref = ref_pitch[r];
        const bool rv = ref != 0.0, ev = bin >= 0;
        n_ref += rv, n_est += ev;
        if (rv && ev) {
          const double dc = 100.0 * (ref - pitch);
          n_both += 1;
          n_pitch += within(fabs(dc), sp);
          n_chroma += within(fabs(dc - 1200.0 * floor(dc / 1200.0 + 0.5)), sp);
        }
      }
    }
  }
  if (points) {
    if (tid == 0) status[c] = 0;
    return;
  }
  n_ref = wave_sum(n_ref), n_est = wave_sum(n_est), n_both = wave_sum(n_both), n_pitch = wave_sum(n_pitch), n_chroma = wave_sum(n_chroma);
  if (lane == 0) s_cnt[wave][0] = n_ref, s_cnt[wave][1] = n_est, s_cnt[wave][2] = n_both, s_cnt[wave][3] = n_pitch, s_cnt[wave][4] = n_chroma;
  __syncthreads();
  if (tid < 5) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v += s_cnt[w][tid];
    scores[6 * c + 1 + tid] = (int64_t)v;
  }
  if (tid == 0) scores[6 * c] = rows, status[c] = 0;
}

}  // namespace

hipError_t launch_melody(const float* contour, const MelodyParams* sets, const MelodyDecode* dec, int64_t n_decodes, int max_jump,
                         uint8_t* pred, void* points, const double* ref_pitch, MpScoreParams sp, int64_t* scores, int32_t* status,
                         hipStream_t s) {
  if (n_decodes <= 0) return hipSuccess;
  if (max_jump < 0 || max_jump > kMelodyMaxJump) return hipErrorInvalidValue;
  if (max_jump <= kMelodyNarrowJump)
    hipLaunchKernelGGL(melody_kernel<kMelodyNarrowJump>, dim3((unsigned)n_decodes), dim3(kLanes), 0, s, contour, sets, dec, pred,
                       static_cast<uint4*>(points), ref_pitch, sp, scores, status);
  else
    hipLaunchKernelGGL(melody_kernel<kMelodyMaxJump>, dim3((unsigned)n_decodes), dim3(kLanes), 0, s, contour, sets, dec, pred,
                       static_cast<uint4*>(points), ref_pitch, sp, scores, status);
  return hipGetLastError();
}

}  // namespace bp
