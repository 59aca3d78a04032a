// CQT front end on PRE-SPLIT, REFLECT-PADDED f16 planes (round 3): what its two stages share — the plane geometry, the
// constants, the load / split / store helpers and the tools' phase stamps.  cqt_planes_pyramid.hip holds the decimators
// (BP_STAGE_PYRAMID), cqt_planes_filterbank.hip the filterbank with its fused normalise phase (BP_STAGE_FILTERBANK).
//
// The pyramid lives in HBM as pre-split, reflect-padded f16 planes and the matrix operands of both
// stages come straight from those planes — no LDS staging, no workgroup barriers, every wave an independent
// worker.  Same operators and reference lines as cqt_mfma.hip (which this path superseded as the default):
//   basic_pitch/layers/nnaudio.py:259-284, 636-638   downsampling_by_n: zero-pad 127, 256-tap FIR, stride 2
//   basic_pitch/layers/nnaudio.py:216-256, 640-661   get_cqt_complex per level, * sqrt(lengths), magnitude
//   basic_pitch/layers/nnaudio.py:300-301            ReflectionPad1D(128)
//   basic_pitch/layers/signal.py:171-178             power, 10*log10(power + 1e-10), per-example min / max
//
// Why.  The staged kernels were paced by their instruction count: per (window, level, 16-frame tile) the
// four role waves of a workgroup spent ~1570 wave-instructions around 84 matrix instructions — every sample split into
// f16 hi + lo again in front of every use (2.3 times on average: once for the decimator, ~1.25 times for the
// filterbank's overlapping tiles), an exchange of the re / im planes through LDS, three workgroup barriers.  Here
//   * a sample is split ONCE, where it is produced (level 0: pl_split_kernel; level k >= 1: the decimator's epilogue),
//     and stored as two f16 planes (hi, lo * 2^11) — the same 4 bytes per sample as fp32;
//   * a level's region carries its own reflect padding (128 samples either side, nnaudio.py:300-301), written by the
//     tile that computes the mirrored samples, so a filterbank A fragment — 8 consecutive samples of a frame's 256-tap
//     window — is ONE aligned 16-byte global load per lane (L1 / L2 absorb the Hankel overlap), for every frame;
//   * one wave owns a whole (window, level, tile): all five 16-column groups of the 72 filter columns, re and im of a
//     filter in the SAME lane, so the magnitude / log epilogue runs in registers: no exchange, no barrier.  The filter
//     fragments (58 KB) are the only LDS tenants (read-only, one copy per CU);
//   * the decimator runs transposed (filter = A operand, signal = B operand): a lane ends up with 4 CONSECUTIVE
//     outputs, i.e. one 8-byte store per plane.  The reference zero-pads where the filterbank reflects: the two edge
//     tiles of a level mask their fragments, all others run unmasked.
//
// Arithmetic is unchanged: x = hi + lo 2^-11 (rn), products hi*hi + (lo*hi + hi*lo) 2^-11 on v_mfma_f32_16x16x32_f16,
// fp32 accumulation, taps pre-scaled by 2^10 (decimator) / 2^12 (CQT kernels) — see cqt_mfma.hip's header.
#pragma once
#include "bp_kernels.h"

namespace bp {

constexpr float kPlDmTapUnscale = 1.0f / 1024.0f;
constexpr float kPlFmTapUnscale = 1.0f / 4096.0f;
constexpr int kPlPad = 128;        // reflect padding in front of a level's samples (a multiple of 8: units stay aligned)
constexpr int kPlTileOut = 256;    // decimator outputs per tile (16 row-blocks x 16)
constexpr int kPlDmSteps = 9;
constexpr int kPlTilesPerLevel = (kFrames + 15) / 16;  // 11 filterbank tiles of 16 frames

// Geometry of a window's planes.  Element = one f16; a window owns 2 * stride elements: hi plane, then lo plane.  Level
// k's samples live at [off[k] + kPlPad, off[k] + kPlPad + len[k]); regions are multiples of 64 elements (128 bytes).
struct PlGeo {
  int n_levels, hop0, n_bins;
  int len[10];
  int off[10];
  int rlen[10];
  int64_t stride;
};

inline PlGeo make_pl_geo(bool ext) {
  PlGeo g{};
  g.n_levels = ext ? kOctavesExt : kOctaves;
  g.hop0 = ext ? 512 : 256;
  g.n_bins = ext ? kBinsExt : kBins;
  int64_t off = 0;
  for (int k = 0; k < g.n_levels; ++k) {
    g.len[k] = ext ? (k == 0 ? kAudioNExt : level_len(k - 1)) : level_len(k);
    // readers: the next level's decimator up to len + 767 past the region start + pad; the filterbank's padding frames
    // (172..175 of the 11th tile) up to 176 hop + 256
    const int hop = g.hop0 >> k;
    int need = kPlPad + g.len[k] + 776;
    if (need < 176 * hop + 256) need = 176 * hop + 256;
    g.rlen[k] = (need + 63) & ~63;
    g.off[k] = (int)off;
    off += g.rlen[k];
  }
  g.stride = off;
  return g;
}

// tools only (tools/build_all_variant.sh prof -DPL_PROF; tools/experiments/cqt_prof.py): phase stamps of two workgroups of
// the per-window kernels, [workgroup slot][wave][stamp].  Each stage file stamps a copy of its own (a __device__ variable
// belongs to one file); bp_debug_pl_prof (cqt_planes_filterbank.hip) hands out both: [0 = pyramid, 1 = filterbank][...]
#ifdef PL_PROF
static __device__ unsigned long long g_pl_prof[2][16][16];
int pl_prof_pyramid(unsigned long long* out);  // cqt_planes_pyramid.hip: its copy, 2 x 16 x 16 values
#define PL_STAMP(kern, i)                                                                                   \
  do {                                                                                                      \
    if ((blockIdx.x == 0 || blockIdx.x == 131) && (threadIdx.x & 63) == 0)                                  \
      g_pl_prof[blockIdx.x ? 1 : 0][threadIdx.x >> 6][i] = __builtin_amdgcn_s_memtime();                   \
  } while (0)
#define PL_STAMP_RT(kern, i)                                                                                \
  do {                                                                                                      \
    if ((blockIdx.x == 0 || blockIdx.x == 131) && (threadIdx.x & 63) == 0)                                  \
      g_pl_prof[blockIdx.x ? 1 : 0][threadIdx.x >> 6][i] = wall_clock64();                                 \
  } while (0)
#else
#define PL_STAMP(kern, i) ((void)0)
#define PL_STAMP_RT(kern, i) ((void)0)
#endif

#define BP_PL_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0)

__device__ __forceinline__ uint4 pl_load16(const uint16_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);  // alignment as the pointer has it (2 bytes for the hop-1 level): the compiler picks
  return v;
}

__device__ __forceinline__ void pl_split8(const float4& a, const float4& c, uint4& h, uint4& l) {
  split_f16x2_rn(f32x2{a.x, a.y}, h.x, l.x);
  split_f16x2_rn(f32x2{a.z, a.w}, h.y, l.y);
  split_f16x2_rn(f32x2{c.x, c.y}, h.z, l.z);
  split_f16x2_rn(f32x2{c.z, c.w}, h.w, l.w);
}

// 8 / 16 bytes to global memory that only a LATER launch reads (planes, zp).  -DPL_STORE_SC1 (tools: A/B): write-through
// stores that do not leave the line in the XCD's L2 (MI355X_MICROARCH.md, "stores of each flavour").
__device__ __forceinline__ void pl_store8(void* p, uint2 v) {
#ifdef PL_STORE_SC1
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v.x | ((unsigned long long)v.y << 32),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *reinterpret_cast<uint2*>(p) = v;
#endif
}
__device__ __forceinline__ void pl_store16(void* p, uint4 v) {
#ifdef PL_STORE_SC1
  const u32x4 d = {v.x, v.y, v.z, v.w};
  asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(d) : "memory");
#else
  *reinterpret_cast<uint4*>(p) = v;
#endif
}

}  // namespace bp
