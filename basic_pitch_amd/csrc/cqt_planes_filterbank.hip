// CQT front end on pre-split f16 planes, stage 2 (BP_STAGE_FILTERBANK): the filterbank over the pyramid's planes with the
// magnitude / log epilogue in registers and, fused, the window's normalise + BatchNorm + split.  Design and arithmetic:
// cqt_planes.h.
//   basic_pitch/layers/nnaudio.py:216-256, 640-661   get_cqt_complex per level, * sqrt(lengths), magnitude
//   basic_pitch/layers/signal.py:171-178             power, 10*log10(power + 1e-10), per-example min / max
#include <cmath>
#include <type_traits>

#include "cqt_planes.h"
#include "launch_plan.h"

namespace bp {

// value of lane + 4 of the same 16-lane row (DPP row_shl:4; lanes 12..15 of a row read 0)
__device__ __forceinline__ float pl_from_lane_plus4(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x104, 0xf, 0xf, true));
}

// ================================================================================================
// filterbank: one wave per (window, level, 16-frame tile), all 72 filter columns, epilogue in registers
//   column groups (16 columns each): 0 = re of filters 0..15, 1 = im 0..15 (taps 16..239: k-steps 0..6),
//   2 = re 16..31, 3 = im 16..31, 4 = {re 32..35 | im 32..35 | 8 zero columns} (taps 48..207: k-steps 1..5)
constexpr int kPlFbFrags = 7 + 7 + 5 + 5 + 5;  // step-fragments, hi and lo each
__host__ __device__ constexpr int pl_fb_frag0(int g) { return g == 0 ? 0 : g == 1 ? 7 : g == 2 ? 14 : g == 3 ? 19 : 24; }
__host__ __device__ constexpr int pl_fb_step0(int g) { return g < 2 ? 0 : 1; }
__host__ __device__ constexpr int pl_fb_steps(int g) { return g < 2 ? 7 : 5; }
// the 29 (k-step, group) products of a task in issue order: k-step major, so an A fragment is finished with after its step
struct PlFbItem {
  int s, q, f;  // k-step, column group, index of the group's step-fragment in LDS
};
__host__ __device__ constexpr PlFbItem pl_fb_item(int i) {
  int n = 0;
  for (int s = 0; s < 7; ++s)
    for (int q = 0; q < 5; ++q) {
      if (s < pl_fb_step0(q) || s >= pl_fb_step0(q) + pl_fb_steps(q)) continue;
      if (n == i) return PlFbItem{s, q, pl_fb_frag0(q) + s - pl_fb_step0(q)};
      ++n;
    }
  return PlFbItem{-1, -1, -1};
}
static_assert(pl_fb_item(kPlFbFrags - 1).s == 6 && pl_fb_item(kPlFbFrags).s == -1, "29 products per task");

// Normalise + BatchNorm + split of four consecutive bins into `zp` words (signal.py:177-183, models.py:187-189):
// z = (lp - min) * (bn_a / range) + bn_b, hi = rn_f16(z), lo = rn_f16((z - hi) 2^11), word = hi | lo << 16.
__device__ __forceinline__ uint4 pl_zp_pack4(const float (&x)[4], float mn, float nk, float bn_b) {
  uint32_t u[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float z = norm_bn_k(x[e], mn, nk, bn_b);
    const _Float16 hi = (_Float16)z;
    const _Float16 lo = (_Float16)((z - (float)hi) * kLoScale);
    u[e] = (uint32_t)__builtin_bit_cast(unsigned short, hi) | ((uint32_t)__builtin_bit_cast(unsigned short, lo) << 16);
  }
  return uint4{u[0], u[1], u[2], u[3]};
}

// THREADS / APF: 1024 threads = 4 waves per SIMD (128 VGPRs each) keep three k-steps of A fragments ahead; 768 / 704
// threads = 3 waves per SIMD with up to 168 VGPRs hold the whole next task's fragments in flight.
// FUSED: a workgroup owns whole windows (its waves draw the window's 99 tasks), keeps the tiles' extrema in LDS and, when
// the window's last task is done, normalises its log-power map itself and writes the pre-split, BatchNorm-ed `zp` words
// (signal.py:177-183, models.py:187-189: what zpack_kernel does in a launch of its own) — the map was written by this
// CU a few microseconds ago and comes back from L2, the extrema never leave the CU.  !FUSED: tasks strided over all
// workgroups, extrema partials to `mmp` (launches with fewer windows than CUs, and the per-stage test hook).
//
// Round 5 (the kernel was paced by its instruction count: 9 vector instructions per matrix instruction, of which the
// normalise phase issued 45 %):
//  * every A fragment is `uniform base (SGPR pair) + one 32-bit lane offset`: no 64-bit vector address arithmetic.  The
//    two level-0 tiles that touch the ends of the signal read the 32 edge rows (above), whose row pitch makes the lane
//    offset the same as into the audio;
//  * the epilogue works on the accumulators as they are: with s = sqrt(len_b) 2^-12 (nnaudio.py:649-650 and the taps'
//    scale) the reference's 10 log10((s re)^2 + (s im)^2 + eps) is kln2 [log2(re^2 + im^2 + eps / s^2) + log2(s^2)]; the
//    two per-bin constants come from an LDS table (built at the kernel's start): 7 instead of 13 operations per value
//    and no sqrt (the reference takes the root for the magnitude and squares it again, nnaudio.py:661, signal.py:174);
//  * FUSED: a lane keeps running extrema over all its tasks of a window; one DPP reduction per wave and window;
//  * the normalise phase runs over three index spaces (bins that come back from L2, bins in LDS, the one mixed group
//    of four) with compile-time divisors, the affine map folded to (lp - min) * (bn_a / range) + bn_b.
template <int THREADS, int APF, bool FUSED, bool EXT>
__global__ __launch_bounds__(THREADS) void cqt_filterbank_planes_kernel(
    const uint16_t* __restrict__ pl, const float* __restrict__ audio, int64_t audio_stride,
    const uint4* __restrict__ bfrag, const float* __restrict__ bin_eps, float* __restrict__ lp, float2* __restrict__ mmp,
    uint32_t* __restrict__ zp, int n_windows, LogConsts kc, PlGeo g, unsigned per_window_magic) {
  constexpr int NB = EXT ? kBinsExt : kBins;
  constexpr int NL = EXT ? kOctavesExt : kOctaves;
  constexpr int HOP0 = EXT ? 512 : 256;
  constexpr int kLog2Hop0 = EXT ? 9 : 8;
  constexpr int kPerWindow = NL * kPlTilesPerLevel;
  constexpr int kWaves = THREADS / 64;
  static_assert(kPlTilesPerLevel == 11, "the multiply-shift below divides by 11");
  __shared__ __attribute__((aligned(16))) uint4 bfr[kPlFbFrags * 2 * 64];
  // the per-bin constants and the level offsets from LDS, not from global / constant memory: a wave's memory counters are
  // in order, so a global load in the epilogue would wait for every A fragment prefetched for the next task before it
  __shared__ float2 s_bin[NB];
  __shared__ int s_off[10];
  __shared__ int s_next;
  __shared__ float2 s_mm[FUSED ? kWaves : 1];
  // FUSED: the log-power values of the four top levels (144 bins x 172 frames = 97 KB: what is left of the CU's LDS) wait
  // for the normalise phase here instead of making the round trip through L2 / HBM
  constexpr int kLdsBins = 4 * kBpo;
  constexpr int kLdsBin0 = NB - kLdsBins;  // bins from here on wait in LDS
  __shared__ float s_lp[FUSED ? kFrames * kLdsBins : 1];
  PL_STAMP(1, 0);
  PL_STAMP_RT(1, 14);
  // log2 -> 10 log10 (uniform: kept in a scalar register)
  const float kln2 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(0.69314718055994531f * kc.s0 * kc.s1)));
  if (threadIdx.x == 0) s_next = 0;
  for (int i = threadIdx.x; i < kPlFbFrags * 2 * 64; i += THREADS) bfr[i] = bfrag[i];
  {
    // The per-bin pair {eps_b = eps / s^2, c_b = kln2 log2(s^2)}.  c_b is derived HERE, with the very instructions the
    // epilogue uses, as c_b = rn(v0 - log2(eps_b) kln2), v0 = the log-power of a silent bin (10 log10(eps), the value
    // every bin had before round 5): a bin whose power vanishes beside eps_b (digital silence) then evaluates to
    // rn(log2(eps_b) kln2 + c_b) = v0 EXACTLY, whatever its bin (|c_b| < 64 rounds to 2^-19, half an ulp of v0 ~ -100 is
    // 2^-18) — the window's range is exactly 0 and divide_no_nan yields the reference's constant map (signal.py:179-183).
    // With a table rounded on the host the silent window's extrema differed in the last bit and the normalisation blew
    // that up to a full-scale pattern.
    const float v0 = __fmul_rn(__builtin_amdgcn_logf(kc.eps), kln2);
    for (int i = threadIdx.x; i < NB; i += THREADS) {
      const float e = bin_eps[i];
      s_bin[i] = make_float2(e, __fmaf_rn(-__builtin_amdgcn_logf(e), kln2, v0));
    }
  }
  if (threadIdx.x < 10) s_off[threadIdx.x] = g.off[threadIdx.x];
  __syncthreads();
  PL_STAMP(1, 1);
  int lane = threadIdx.x & 63;
  const int n_tasks = n_windows * kPerWindow;
  const float kInf = __int_as_float(0x7f800000);
  // D row (frame of the tile) = 4 kg + r, column (filter of the group) = t.  Every per-lane offset below is re-derived
  // from the (opaque) lane index inside the task loop — a handful of operations per task — instead of living in a dozen
  // registers through it: at 128 registers per lane the kernel would spill them.
  int t = lane & 15, kg = lane >> 4;
  // Tasks of this workgroup: blockIdx.x + gridDim.x * j, j = 0, 1, ...; its waves DRAW j from a counter in LDS instead of
  // owning a fixed share: the SIMD's issue arbitration favours the older waves of a workgroup (phase clocks: wave 0
  // finishes a task in 7.5 k cycles, wave 10 in 19.5 k), so with fixed shares the old waves ran out of work at 40 % of
  // the kernel's duration and the young ones finished it alone.
  struct Pos {
    int b, rem;
  };
  int win = blockIdx.x;  // FUSED: the window this workgroup is working on
  auto grab = [&]() -> int {
    int j = 0;
    if ((threadIdx.x & 63) == 0) j = atomicAdd(&s_next, 1);
    j = __builtin_amdgcn_readfirstlane(j);
    if constexpr (FUSED) return j < kPerWindow ? win * kPerWindow + j : -1;
    const int task_ = blockIdx.x + gridDim.x * j;
    return task_ < n_tasks ? task_ : -1;
  };
  auto pos_of = [&](int task_) {  // task / per_window by multiply-shift (exact below 2^32 / 95 for 99, 2^32 / 4 for 110)
    if constexpr (FUSED) return Pos{win, task_ - win * kPerWindow};
    const int b_ = (int)__umulhi((unsigned)task_, per_window_magic);
    return Pos{b_, task_ - b_ * kPerWindow};
  };
  // Where a task's A fragments come from: two uniform bases (first / second 16-byte half of a k-step's fragment) + this
  // lane's byte offset + step * s.  Planes: 16 bytes of the hi plane per k-step (32 elements apart), the lo plane g.stride
  // elements behind it.  Level 0: the fp32 audio itself — 8 samples = two 16-byte loads per k-step, split to hi / lo in
  // registers when the k-step is consumed (every level-0 sample feeds at most one frame: hop >= window, so nothing is
  // split twice) — or, for the two tiles at the ends of the signal, the edge rows.
  struct Src {
    const char* p0;
    const char* p1;
    uint32_t voff;
    int step;  // bytes between k-steps
    int raw;   // fp32 samples: split at consumption (an int: a bool's padding bytes made the struct copies go through scratch)
  };
  auto src_of = [&](Pos p) -> Src {
    const int level_ = (p.rem * 745) >> 13;  // rem / 11 for rem < 2700
    const int tile_ = p.rem - level_ * kPlTilesPerLevel;
    const uint16_t* wpl = pl + (int64_t)p.b * 2 * g.stride;
    if (level_ == 0) {  // wave-uniform
      const float* a = (tile_ == 0 || tile_ == kPlTilesPerLevel - 1)
                           ? reinterpret_cast<const float*>(wpl + __builtin_amdgcn_readfirstlane(s_off[0])) + (tile_ ? 16 * HOP0 : 0)
                           : audio + (int64_t)p.b * audio_stride + (16 * tile_ * HOP0 - kPlPad);
      const char* c = reinterpret_cast<const char*>(a);
      return Src{c, c + 16, (uint32_t)(t * HOP0 + 16 + 8 * kg) * 4u, 128, 1};  // fp32 samples, frame pitch = hop0
    }
    const int sh = kLog2Hop0 - level_;  // log2(hop of the level)
    const char* c = reinterpret_cast<const char*>(wpl + __builtin_amdgcn_readfirstlane(s_off[level_]) + ((16 * tile_) << sh));
    return Src{c, c + 2 * g.stride, (((uint32_t)t << sh) << 1) + 32u + 16u * (uint32_t)kg, 64, 0};  // f16 elements
  };
  auto load16 = [](const char* base, uint32_t off) {
    uint4 v;
    __builtin_memcpy(&v, __builtin_assume_aligned(base + off, 2), 16);  // 2-byte alignment at the hop-1 level; dword at least elsewhere
    return v;
  };
  for (; win < (FUSED ? n_windows : blockIdx.x + 1); win += gridDim.x) {
  float rmin = kInf, rmax = -kInf;  // FUSED: this lane's extrema over its tasks of the window
  int task = grab();
  int ntask = task >= 0 ? grab() : -1;
  if (task >= 0) {
  Pos pos = pos_of(task);
  // A fragments: a ring of 7 k-steps.  When a task starts, its first APF steps are in the ring (fetched during the task
  // before); step s + APF is fetched when step s has been consumed — for s + APF >= 7 that is step s + APF - 7 of the NEXT
  // task.  APF = 7: every load has a whole task's matrix work to land (a level-0 / level-1 task streams from HBM).
  uint4 ah[7], al[7];
  Src src = src_of(pos);
  {
#pragma unroll
    for (int s = 0; s < APF; ++s) {
      ah[s] = load16(src.p0, src.voff + src.step * s);
      al[s] = load16(src.p1, src.voff + src.step * s);
    }
  }
  for (;;) {
    // keep the filter fragments in LDS: without an opaque offset the compiler hoists all 58 loop-invariant reads
    asm volatile("" : "+v"(lane));
    t = lane & 15, kg = lane >> 4;
    const int nntask = ntask >= 0 ? grab() : -1;  // drawn a task ahead: its LDS round trip is nobody's critical path
    const int b = pos.b, rem = pos.rem;
    const int level = (rem * 745) >> 13, tile = rem - level * kPlTilesPerLevel;
    const uint4* bl = bfr + lane;
    const bool more = ntask >= 0;
    const Pos npos = more ? pos_of(ntask) : pos;
    const Src nsrc = more ? src_of(npos) : src;

    f32x4 hh[5], xx[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) hh[q] = xx[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // filter fragments two products ahead of the matrix instructions that use them: issued right behind a product's
    // instructions, an LDS read's ~100 cycles would be exposed 29 times per task (they were: the compiler's own order)
    constexpr int kBPf = 2;
    uint4 bh[kPlFbFrags], bw[kPlFbFrags];
#pragma unroll
    for (int i = 0; i < kBPf; ++i) {
      bh[i] = bl[(2 * pl_fb_item(i).f) * 64];
      bw[i] = bl[(2 * pl_fb_item(i).f + 1) * 64];
    }
#pragma unroll
    for (int i = 0; i < kPlFbFrags; ++i) {
      constexpr auto item = [](int j) { return pl_fb_item(j); };
      const int s = item(i).s, q = item(i).q;
      if (i + kBPf < kPlFbFrags) {
        bh[i + kBPf] = bl[(2 * item(i + kBPf).f) * 64];
        bw[i + kBPf] = bl[(2 * item(i + kBPf).f + 1) * 64];
      }
      if (src.raw && (i == 0 || item(i - 1).s != s)) {  // first product of k-step s of a level-0 task (wave-uniform): the
        const float4 a = __builtin_bit_cast(float4, ah[s]), c = __builtin_bit_cast(float4, al[s]);  // slot holds 8 samples
        pl_split8(a, c, ah[s], al[s]);
      }
      __builtin_amdgcn_sched_barrier(0);
#ifdef PL_FB_PAIRED
      // tools (A/B): the second correction product of item i - 1 behind the first two of item i, so that the two updates of
      // an xx accumulator are three matrix instructions apart instead of back to back (same order per accumulator: same bits)
      hh[q] = BP_PL_MFMA16(ah[s], bh[i], hh[q]);
      xx[q] = BP_PL_MFMA16(al[s], bh[i], xx[q]);
      if (i > 0) xx[item(i - 1).q] = BP_PL_MFMA16(ah[item(i - 1).s], bw[i - 1], xx[item(i - 1).q]);
      if (i + 1 == kPlFbFrags) xx[q] = BP_PL_MFMA16(ah[s], bw[i], xx[q]);
#else
      hh[q] = BP_PL_MFMA16(ah[s], bh[i], hh[q]);
      xx[q] = BP_PL_MFMA16(al[s], bh[i], xx[q]);
      xx[q] = BP_PL_MFMA16(ah[s], bw[i], xx[q]);
#endif
      if (i + 1 == kPlFbFrags || item(i + 1).s != s) {  // last product of k-step s: its ring slot takes step s + APF
        const int sn = s + APF;
        if (sn < 7) {
          ah[sn] = load16(src.p0, src.voff + src.step * sn);
          al[sn] = load16(src.p1, src.voff + src.step * sn);
        } else {
          ah[sn - 7] = load16(nsrc.p0, nsrc.voff + nsrc.step * (sn - 7));
          al[sn - 7] = load16(nsrc.p1, nsrc.voff + nsrc.step * (sn - 7));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }

    // epilogue: D row (frame) = 4 kg + r, column (filter of the group) = lane & 15
    const int bin0 = (NL - 1 - level) * kBpo - 15;  // nnaudio.py:640-642
    char* lp_t = reinterpret_cast<char*>(lp + ((int64_t)b * kFrames + 16 * tile) * NB + bin0);
    const int fr0 = 16 * tile + 4 * kg;
    const uint32_t so_kg = __umul24((unsigned)kg, 16u * NB);             // lp stores: + (r NB + 16 group) floats
    const uint32_t so_hbm = so_kg + 4u * (unsigned)t, so_hbm4 = so_kg + 4u * (32u + ((unsigned)t & 3u));
    const int so_lds = 4 * kg * kLdsBins + t, so_lds4 = 4 * kg * kLdsBins + 32 + (t & 3);
    float vmin = FUSED ? rmin : kInf, vmax = FUSED ? rmax : -kInf;
    // `masked` (wave-uniform): the tile has padding frames (the 11th tile) or the level has bins below the CQT's first
    // (the deepest level): 8 of 10 tasks have neither, and then only group 4's unused columns need a predicate
    const bool masked = tile == kPlTilesPerLevel - 1 || bin0 < 0;
    const bool to_lds = FUSED && level < 4;  // wave-uniform
    float* lds_t = s_lp + 16 * tile * kLdsBins + (3 - level) * kBpo;
    auto finish = [&](auto masked_c, auto lds_c, const f32x4& hr, const f32x4& xr, const f32x4& hi_, const f32x4& xi, int k,
                      int grp, bool col_ok) {
      constexpr bool kMasked = decltype(masked_c)::value, kLds = decltype(lds_c)::value;
      const bool bin_ok = col_ok && (!kMasked || bin0 + k >= 0);
      const float2 bc = s_bin[kMasked ? (bin0 + k >= 0 ? bin0 + k : 0) : bin0 + k];
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float re = __fmaf_rn(xr[r], kLoUnscale, hr[r]);
        const float im = __fmaf_rn(xi[r], kLoUnscale, hi_[r]);
        const float pw = __fmaf_rn(im, im, __fmul_rn(re, re));
        // nnaudio.py:649-661 and signal.py:174-175 in accumulator units (see the header), hardware 1-ulp log2
        v[r] = __fmaf_rn(__builtin_amdgcn_logf(__fadd_rn(pw, bc.x)), kln2, bc.y);
      }
      auto put = [&](int r) {
        if constexpr (kLds)
          lds_t[(grp == 2 ? so_lds4 : so_lds + 16 * grp) + r * kLdsBins] = v[r];
        else
          *reinterpret_cast<float*>(lp_t + (grp == 2 ? so_hbm4 : so_hbm) + (grp == 2 ? 0 : 64 * grp) + r * NB * 4) = v[r];
      };
      if constexpr (kMasked) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (bin_ok && fr0 + r < kFrames) {
            put(r);
            vmin = fminf(vmin, v[r]);
            vmax = fmaxf(vmax, v[r]);
          }
      } else if (bin_ok) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          put(r);
          vmin = fminf(vmin, v[r]);
          vmax = fmaxf(vmax, v[r]);
        }
      }
    };
    // group 4: re of filter 32 + c in column c, im in column 4 + c: bring the im values over (row_shl:4)
    // (one call per element: written as a loop over r, hipcc 7.2 emits the DPP move for r = 0 only and reuses it)
    const f32x4 hi4 = {pl_from_lane_plus4(hh[4][0]), pl_from_lane_plus4(hh[4][1]), pl_from_lane_plus4(hh[4][2]),
                       pl_from_lane_plus4(hh[4][3])};
    const f32x4 xi4 = {pl_from_lane_plus4(xx[4][0]), pl_from_lane_plus4(xx[4][1]), pl_from_lane_plus4(xx[4][2]),
                       pl_from_lane_plus4(xx[4][3])};
    auto finish_all = [&](auto mc, auto lc) {
      finish(mc, lc, hh[0], xx[0], hh[1], xx[1], t, 0, true);
      finish(mc, lc, hh[2], xx[2], hh[3], xx[3], 16 + t, 1, true);
      finish(mc, lc, hh[4], xx[4], hi4, xi4, 32 + (t & 3), 2, t < 4);
    };
    if (to_lds) {
      if (masked)
        finish_all(std::true_type{}, std::true_type{});
      else
        finish_all(std::false_type{}, std::true_type{});
    } else {
      if (masked)
        finish_all(std::true_type{}, std::false_type{});
      else
        finish_all(std::false_type{}, std::false_type{});
    }
    if constexpr (FUSED) {
      rmin = vmin, rmax = vmax;
    } else {
      vmin = wave_min_lane63(vmin);
      vmax = wave_max_lane63(vmax);
      if ((threadIdx.x & 63) == 63) mmp[(int64_t)b * kPerWindow + rem] = make_float2(vmin, vmax);
    }
    if (!more) break;
    pos = npos, src = nsrc, task = ntask, ntask = nntask;
  }
  }  // if (task >= 0)
  if constexpr (!FUSED) break;
  if constexpr (FUSED) {
    // ---- the window is complete: normalise + BatchNorm + split, as zpack_kernel (conv_branch.hip) ----
    PL_STAMP(1, 2);
    rmin = wave_min_lane63(rmin);
    rmax = wave_max_lane63(rmax);
    if ((threadIdx.x & 63) == 63) s_mm[threadIdx.x >> 6] = make_float2(rmin, rmax);
    __syncthreads();  // every tile's log-power values (global stores of this workgroup / LDS) and the waves' extrema are visible
    PL_STAMP(1, 3);
    float vmin = kInf, vmax = -kInf;
    if ((threadIdx.x & 63) < kWaves) {
      const float2 e = s_mm[threadIdx.x & 63];
      vmin = e.x, vmax = e.y;
    }
    const float mn = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wave_min_lane63(vmin)), 63));
    const float mx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wave_max_lane63(vmax)), 63));
    const float nk = norm_scale(mn, mx, kc);
    const float* lpb = lp + (int64_t)win * kFrames * NB;
    // only the words that carry bins: `zp`'s pad frames / pad words are zero since bp_create and nobody writes them
    uint32_t* zb = zp + (int64_t)win * kZWin + kZRow + kZPadL;  // frame 0, bin 0 (kZPadL is a multiple of 4)
    constexpr int kJ = (NB + 3) / 4;     // groups of four bins per frame
    constexpr int kJH = kLdsBin0 / 4;    // groups whose four bins all come back from L2
    static_assert(kLdsBin0 % 4 == 1 && NB % 4 == 1, "group kJH is {1 bin from L2, 3 from LDS}; the last group holds one bin");
    constexpr int kJL = kJ - kJH - 1;    // groups whose bins all wait in LDS: columns 4 j' + 3 .. 4 j' + 6
    // (the thread index through an opaque copy: the index arithmetic below does not depend on the window, and hoisted out
    // of the window loop it would sit in ~40 registers through the task loop — the compiler spilled them to scratch)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const char* lpc = reinterpret_cast<const char*>(lpb);
    char* zc = reinterpret_cast<char*>(zb);
    // i / d and i % d for the three small index spaces on the full-rate 24-bit multiplier (the generic 32-bit forms are
    // quarter rate): q = (i M) >> 20 with M = ceil(2^20 / d), exact while i (M d - 2^20) < 2^20
    auto divmod = [](int i, auto d_c, auto n_c) {
      constexpr unsigned d = decltype(d_c)::value, n = decltype(n_c)::value, M = ((1u << 20) + d - 1) / d;
      static_assert((unsigned long long)n * (M * d - (1u << 20)) < (1u << 20) && (unsigned long long)n * M < (1ull << 32), "exact");
      const unsigned q = __umul24((unsigned)i, M) >> 20;
      return uint2{q, (unsigned)i - __umul24(q, d)};
    };
    // (A) from L2: all loads of a thread in flight at once (issued one by one, every item would pay the round trip; the
    // memory clobber keeps the compiler from sinking each load into the block that uses it)
    {
      constexpr int nA = kFrames * kJH;
      constexpr int kZb = (nA + THREADS - 1) / THREADS;
      float4 v[kZb];
#pragma unroll
      for (int k = 0; k < kZb; ++k) {
        const int i = tid + k * THREADS;
        const uint2 tj = divmod(i < nA ? i : nA - 1, std::integral_constant<unsigned, kJH>{}, std::integral_constant<unsigned, nA>{});
        v[k] = *reinterpret_cast<const float4*>(lpc + (__umul24(tj.x, NB * 4u) + 16u * tj.y));  // dword alignment is enough
      }
      asm volatile("" ::: "memory");
#pragma unroll
      for (int k = 0; k < kZb; ++k) {
        const int i = tid + k * THREADS;
        if (i < nA) {
          const uint2 tj = divmod(i, std::integral_constant<unsigned, kJH>{}, std::integral_constant<unsigned, nA>{});
          const float x4[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
          pl_store16(zc + (__umul24(tj.x, kZRow * 4u) + 16u * tj.y), pl_zp_pack4(x4, mn, nk, kc.bn_b));
        }
      }
    }
    PL_STAMP(1, 4);
    // (B) from LDS
    {
      constexpr int nB = kFrames * kJL;
      for (int i = tid; i < nB; i += THREADS) {
        const uint2 tj = divmod(i, std::integral_constant<unsigned, kJL>{}, std::integral_constant<unsigned, nB>{});
        const float* row = s_lp + __umul24(tj.x, (unsigned)kLdsBins) + 4u * tj.y + 3u;
        const bool last = tj.y == kJL - 1;  // bins NB - 1 .. NB + 2: one bin, three pad words
        const float x4[4] = {row[0], last ? 0.f : row[1], last ? 0.f : row[2], last ? 0.f : row[3]};
        uint4 w = pl_zp_pack4(x4, mn, nk, kc.bn_b);
        if (last) w.y = w.z = w.w = 0u;
        pl_store16(zc + (__umul24(tj.x, kZRow * 4u) + 16u * (tj.y + kJH + 1)), w);
      }
    }
    // (C) the mixed group: bin 4 kJH from L2, the next three from LDS
    if (tid < kFrames) {
      const float x4[4] = {lpb[tid * NB + 4 * kJH], s_lp[tid * kLdsBins], s_lp[tid * kLdsBins + 1], s_lp[tid * kLdsBins + 2]};
      pl_store16(zc + (__umul24((unsigned)tid, kZRow * 4u) + 16u * kJH), pl_zp_pack4(x4, mn, nk, kc.bn_b));
    }
    PL_STAMP(1, 5);
    __syncthreads();  // s_lp, s_mm and the task counter are free for the next window
    PL_STAMP(1, 6);
    PL_STAMP_RT(1, 15);
    if (threadIdx.x == 0) s_next = 0;
    __syncthreads();
  }
  }  // windows
}

// ================================================================================================
// host side
int filterbank_planes_partials(bool ext) { return make_pl_geo(ext).n_levels * kPlTilesPerLevel; }

// The per-bin constant of the filterbank's epilogue (see the kernel's header): eps / s^2 with s = sqrt(len_b) 2^-12,
// evaluated in float64 and rounded once.  (Its partner kln2 log2(s^2) is derived on the device: see the kernel.)
void filterbank_planes_bin_consts(const float* sqrt_len, int n_bins, LogConsts kc, float* out) {
  for (int b = 0; b < n_bins; ++b) {
    const double s = (double)sqrt_len[b] * (double)kPlFmTapUnscale;
    out[b] = (float)((double)kc.eps / (s * s));
  }
}

// zp != null and enough windows to give every CU its own: the fused kernel (filterbank + normalise / BatchNorm / split of
// whole windows per workgroup) — returns true, `zp` is complete; otherwise tasks strided over the chip, extrema partials in
// `scratch` (fold them with launch_zpack_partials or launch_mm_reduce) — returns false.
// `audio`: the fp32 signal (level 0 has no planes: the interior tiles of level 0 read it directly, the two tiles at the
// ends of the signal read the edge rows the pyramid kernel / launch_planes_edge_rows left where level 0's planes were).
bool launch_filterbank_planes(const uint16_t* pl, const float* audio, int64_t audio_stride, const void* bfrag,
                              const float* bin_consts, float* lp, float* scratch, uint32_t* zp, int n_windows, LogConsts kc,
                              int n_cu, bool ext, hipStream_t stream) {
  const PlGeo g = make_pl_geo(ext);
  const int tasks = n_windows * g.n_levels * kPlTilesPerLevel;
  const uint4* bf = static_cast<const uint4*>(bfrag);
  const float* bk = bin_consts;
  float2* mm = reinterpret_cast<float2*>(scratch);
  const unsigned per_window = (unsigned)(g.n_levels * kPlTilesPerLevel);
  const unsigned magic = (unsigned)((0x100000000ull + per_window - 1) / per_window);
  // one window per workgroup pays from half a window per CU on (launch_plan.h)
  const bool fused = filterbank_fused(zp != nullptr, n_windows, n_cu);
  // (768 threads with 7 / 5 k-steps of A fragments ahead, 158 VGPRs: 0.070 - 0.074 / 0.069 ms against 0.069 - 0.070, round 5)
  constexpr int kThreads = kPlFbThreads, kApf = 3;
  const int grid = filterbank_grid(fused, n_windows, tasks, n_cu);
#define BP_PL_FB_LAUNCH(F, E)                                                                                           \
  hipLaunchKernelGGL((cqt_filterbank_planes_kernel<kThreads, kApf, F, E>), dim3(grid), dim3(kThreads), 0, stream, pl,   \
                     audio, audio_stride, bf, bk, lp, mm, zp, n_windows, kc, g, magic)
  if (fused) {
    if (ext) BP_PL_FB_LAUNCH(true, true); else BP_PL_FB_LAUNCH(true, false);
  } else {
    if (ext) BP_PL_FB_LAUNCH(false, true); else BP_PL_FB_LAUNCH(false, false);
  }
#undef BP_PL_FB_LAUNCH
  return fused;
}

#ifdef PL_PROF
extern "C" int bp_debug_pl_prof(unsigned long long* out) {
  const int rc = pl_prof_pyramid(out);
  return rc ? rc : (int)hipMemcpyFromSymbol(out + 2 * 16 * 16, HIP_SYMBOL(g_pl_prof), sizeof(g_pl_prof));
}
#endif

}  // namespace bp
