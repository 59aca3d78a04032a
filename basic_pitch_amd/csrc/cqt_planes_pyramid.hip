// CQT front end on pre-split f16 planes, stage 1 (BP_STAGE_PYRAMID): the decimators that build the pyramid's planes, and the
// split / unsplit / edge-row kernels around them.  Design and arithmetic: cqt_planes.h.
//   basic_pitch/layers/nnaudio.py:259-284, 636-638   downsampling_by_n: zero-pad 127, 256-tap FIR, stride 2
//   basic_pitch/layers/nnaudio.py:300-301            ReflectionPad1D(128)
#include <cstdlib>
#include <cstring>

#include "cqt_planes.h"
#include "launch_plan.h"

namespace bp {

int64_t planes_elements_per_window(bool ext) { return 2 * make_pl_geo(ext).stride; }

// Level 0's "edge rows" (fp32, where the level-0 planes used to be: element 0 of the window's hi plane).  Frame f's
// 256-sample window reads samples f hop - 128 .. f hop + 127 with reflection at both ends (nnaudio.py:229, 300-301).  The
// filterbank takes the frames of its interior tiles (frames 16 .. 159) straight from the audio; the two tiles that touch
// the ends of the signal — tile 0 (frame 0 is mirrored at the front) and tile 10 (frames 171 .. 175 run past the end; the
// 11th tile's padding frames included: finite values nobody's result depends on) — read these 32 rows instead: rows
// 0 .. 15 = the windows of frames 0 .. 15, rows 16 .. 31 = those of frames 160 .. 175, reflection applied, row pitch =
// hop0 floats (so that a lane's byte offset into a row block equals its offset into the audio: round 5 — every A fragment
// of a task is then `uniform base + one per-lane 32-bit offset`, the addressing form that costs no vector arithmetic).

__device__ __forceinline__ float4 pl_edge_row_load(const float* __restrict__ x, int L, int f, int hop0, int lane) {
  const int i0 = f * hop0 - kPlPad + 4 * lane;  // this lane's four samples of frame f's window
  if (i0 >= 0 && i0 + 3 < L) return *reinterpret_cast<const float4*>(x + i0);  // dword alignment is enough for global vector loads
  float e[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int i = i0 + k;
    i = i < 0 ? -i : i;                     // reflection without repeating the edge sample
    i = i >= L ? 2 * (L - 1) - i : i;
    const bool ok = i >= 0 && i < L;        // beyond one reflection: the padding frames' slack
    e[k] = ok ? x[ok ? i : 0] : 0.0f;
  }
  return float4{e[0], e[1], e[2], e[3]};
}

// rows r and 16 + r (r = 0 .. 15) by one wave: both loads in flight, then both stores.  (A wave that wrote all 16 rows of
// a block one after the other chained 16 memory round trips in front of its own tiles: measured + 4 us on the pyramid.)
__device__ __forceinline__ void pl_write_edge_row_pair(const float* __restrict__ x, int L, float* __restrict__ rows, int hop0,
                                                       int r, int lane) {
  const float4 a = pl_edge_row_load(x, L, r, hop0, lane);
  const float4 b = pl_edge_row_load(x, L, (kPlTilesPerLevel - 1) * 16 + r, hop0, lane);
  *reinterpret_cast<float4*>(rows + r * hop0 + 4 * lane) = a;
  *reinterpret_cast<float4*>(rows + (16 + r) * hop0 + 4 * lane) = b;
}

// one block of 16 rows (head: frames 0 .. 15, else frames 160 .. 175), four rows in flight at a time
__device__ __forceinline__ void pl_write_edge_rows(const float* __restrict__ x, int L, float* __restrict__ rows, int hop0,
                                                   bool head, int lane) {
  const int r0 = head ? 0 : 16, f0 = head ? 0 : (kPlTilesPerLevel - 1) * 16;
#pragma unroll 1
  for (int r = 0; r < 16; r += 4) {
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = pl_edge_row_load(x, L, f0 + r + k, hop0, lane);
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(rows + (r0 + r + k) * hop0 + 4 * lane) = v[k];
  }
}

// the same as a launch of its own (the per-stage test hook, whose planes come from pl_split_kernel)
__global__ __launch_bounds__(64) void pl_edge_rows_kernel(const float* __restrict__ audio, int64_t audio_stride, int L,
                                                          uint16_t* __restrict__ pl, int64_t stride, int off0, int hop0) {
  const float* x = audio + (int64_t)blockIdx.x * audio_stride;
  float* rows = reinterpret_cast<float*>(pl + (int64_t)blockIdx.x * 2 * stride + off0);
  pl_write_edge_rows(x, L, rows, hop0, true, threadIdx.x);
  pl_write_edge_rows(x, L, rows, hop0, false, threadIdx.x);
}

// ================================================================================================
// fp32 signal -> planes of one level (level 0 in production; any level for the per-stage test hook)
__global__ __launch_bounds__(256) void pl_split_kernel(const float* __restrict__ src, int64_t src_stride, int L,
                                                       uint16_t* __restrict__ pl, int64_t stride, int off, int rlen) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (8 * q >= rlen) return;
  const float* x = src + (int64_t)blockIdx.y * src_stride;
  uint16_t* hi = pl + (int64_t)blockIdx.y * 2 * stride + off + 8 * q;
  const int g0 = 8 * q - kPlPad;
  float v[8];
  if (g0 >= 0 && g0 + 8 <= L) {
    const float4 a = *reinterpret_cast<const float4*>(x + g0);  // dword alignment is enough for global vector loads
    const float4 c = *reinterpret_cast<const float4*>(x + g0 + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = c.x, v[5] = c.y, v[6] = c.z, v[7] = c.w;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int g = g0 + e;
      g = g < 0 ? -g : g;                    // nnaudio.py:300-301: reflection without repeating the edge sample
      g = g >= L ? 2 * (L - 1) - g : g;
      const bool ok = g >= 0 && g < L;       // beyond one reflection: slack nobody's result depends on
      v[e] = ok ? x[ok ? g : 0] : 0.0f;
    }
  }
  uint4 h, l;
  split_f16x2_rn(f32x2{v[0], v[1]}, h.x, l.x);
  split_f16x2_rn(f32x2{v[2], v[3]}, h.y, l.y);
  split_f16x2_rn(f32x2{v[4], v[5]}, h.z, l.z);
  split_f16x2_rn(f32x2{v[6], v[7]}, h.w, l.w);
  *reinterpret_cast<uint4*>(hi) = h;
  *reinterpret_cast<uint4*>(hi + stride) = l;
}

// planes -> fp32 (test hook: the pyramid stage's levels as the oracle lays them out)
__global__ __launch_bounds__(256) void pl_unsplit_kernel(const uint16_t* __restrict__ pl, int64_t stride, int off, int L,
                                                         float* __restrict__ dst, int64_t dst_stride) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= L) return;
  const uint16_t* hi = pl + (int64_t)blockIdx.y * 2 * stride + off + kPlPad + i;
  const float h = (float)__builtin_bit_cast(_Float16, hi[0]);
  const float l = (float)__builtin_bit_cast(_Float16, hi[stride]);
  dst[(int64_t)blockIdx.y * dst_stride + i] = h + l * kLoUnscale;
}

// ================================================================================================
// decimate by 2: one wave per tile of 256 outputs
//   D[u][m] = sum_i T[u][i] X[i][m],  T[u][i] = h[i - 2u - 1] (A operand, packed on the host),  X[i][m] = element
//   2 o0 + 32 m + i of the input region (B operand): output n = o0 + 16 m + u reads samples 2n + j - 127, i.e. region
//   elements kPlPad + 2n + j - 127 = 2 o0 + 32 m + (2u + j + 1).
// Row rho of a tile = the 32 elements from 2 o0 + 32 rho; the fragment of lane (m, kg) at k-step s is row m + s, unit kg:
// 24 rows serve all 9 steps.  Re-loading the fragment every step would pull the tile through the texture path 9 times
// (18 KB per tile, and a chain of dependent latencies); instead the 24 rows are fetched ONCE — lane (m, kg) row m, lanes
// m >= 8 also row m + 8 —, parked in a wave-private LDS image, and the fragments are ds_read_b128 from there.
// LDS images whose 16-byte units are read as B fragments — the row images here, the resident planes of the per-window
// kernel — are XOR-swizzled: unit u of an image (4 units = one row of 32 elements) sits at u ^ 2 when bit 4 of u is set,
// i.e. the unit pairs (0, 2) and (1, 3) of rows 4 .. 7 (mod 8) are swapped.  ds_read_b128 is served in four groups of 16
// lanes ({0-3, 12-15, 20-27}, ...: MI355X_MICROARCH.md): at the natural 64-byte row pitch rows rho and rho + 4 (+ 12) of
// a group share banks — 8 LDS cycles per read instead of 4, with a padded pitch of 5 units (rounds 3 - 4: "4 + 1 of
// skew") just the same, with 6 none but no LDS left for it; enumerated (round 5) for every k-step, tile offset and 16-byte
// aligned base: 8 -> 4.  The decimator tiles' 18 signal-fragment reads were what the LDS pipe of a CU spent its time on
// (a round of 16 tiles: 2,880 LDS cycles against 1,400 matrix-pipe cycles per SIMD).  A lane's unit at k-step s is row
// m + s, unit kg: it reads unit kg ^ 2 p(s), p(s) = ((m + s) >> 2) & 1 — one select per k-step between two lane bases.
constexpr int kPlRowU = 4;                      // 16-byte units per row in LDS
constexpr int kPlRowsU = 2 * 24 * kPlRowU;      // hi rows, then lo rows: 192 units = 3072 bytes per wave
__device__ __forceinline__ int pl_swz_elems(int e) { return e ^ ((e >> 3) & 16); }    // f16 elements (8 per unit)

__device__ __forceinline__ uint4 pl_zero_outside(uint4 v, int idx, int L_in) {
  // keep elements whose sample index idx + e - kPlPad lies in [0, L_in): the reference zero-pads the decimator's input
  int nv = kPlPad + L_in - idx;  // elements [0, nv) of this unit are real samples ...
  nv = idx < kPlPad ? 0 : nv;    // ... unless the whole unit lies in front of the signal (kPlPad is a multiple of 8)
  v.x &= (nv > 0 ? 0xffffu : 0u) | (nv > 1 ? 0xffff0000u : 0u);
  v.y &= (nv > 2 ? 0xffffu : 0u) | (nv > 3 ? 0xffff0000u : 0u);
  v.z &= (nv > 4 ? 0xffffu : 0u) | (nv > 5 ? 0xffff0000u : 0u);
  v.w &= (nv > 6 ? 0xffffu : 0u) | (nv > 7 ? 0xffff0000u : 0u);
  return v;
}

__device__ __forceinline__ bool pl_tile_is_edge(int tile, int L_in) {
  return tile == 0 || 2 * kPlTileOut * tile + 32 * 23 + 32 > kPlPad + L_in;  // some fragment reaches outside the signal
}

// What a lane fetches for a tile: its row m, and (lanes m >= 8) row m + 8.  F32IN: 8 fp32 samples per row (the level-0
// signal itself, zero outside [0, L): nnaudio.py:269-279); else 8 f16 hi + 8 f16 lo from the input level's planes.
template <bool F32IN>
struct PlRaw;
template <>
struct PlRaw<true> {
  float4 a0, a1, b0, b1;
};
template <>
struct PlRaw<false> {
  uint4 ah, al, bh, bl;
};

template <bool F32IN>
__device__ __forceinline__ PlRaw<F32IN> pl_fetch_rows(const float* __restrict__ x, const uint16_t* __restrict__ in_hi,
                                                       int64_t stride, int L_in, int tile, int lane) {
  const int m = lane & 15, kg = lane >> 4;
  const int base = 2 * kPlTileOut * tile + 32 * m + 8 * kg;
  PlRaw<F32IN> r;
  if constexpr (F32IN) {
    // zero outside [0, L_in) (nnaudio.py:269-279).  A row's two halves start at multiples of 4 and both window lengths are
    // multiples of 4: a half is either all signal or all padding, so the edge tiles need two predicated 16-byte loads
    // per row, not eight predicated samples.
    static_assert(kAudioN % 4 == 0 && kAudioNExt % 4 == 0 && kPlPad % 4 == 0, "no half straddles an end of the signal");
    auto row = [&](int g0, float4& lo4, float4& hi4) {
      if (!pl_tile_is_edge(tile, L_in)) {
        lo4 = *reinterpret_cast<const float4*>(x + g0);  // dword alignment is enough for global vector loads
        hi4 = *reinterpret_cast<const float4*>(x + g0 + 4);
      } else {
        lo4 = hi4 = float4{0.f, 0.f, 0.f, 0.f};
        if (g0 >= 0 && g0 + 3 < L_in) lo4 = *reinterpret_cast<const float4*>(x + g0);
        if (g0 + 4 >= 0 && g0 + 7 < L_in) hi4 = *reinterpret_cast<const float4*>(x + g0 + 4);
      }
    };
    row(base - kPlPad, r.a0, r.a1);
    r.b0 = r.b1 = float4{0.f, 0.f, 0.f, 0.f};
    if (m >= 8) row(base - kPlPad + 256, r.b0, r.b1);
  } else {
    r.ah = *reinterpret_cast<const uint4*>(in_hi + base);
    r.al = *reinterpret_cast<const uint4*>(in_hi + stride + base);
    r.bh = r.bl = uint4{0u, 0u, 0u, 0u};
    if (m >= 8) {
      r.bh = *reinterpret_cast<const uint4*>(in_hi + base + 256);
      r.bl = *reinterpret_cast<const uint4*>(in_hi + stride + base + 256);
    }
  }
  return r;
}

// The four consecutive outputs a lane holds after a tile's matrix work (D: column m = lane & 15, rows u = 4 kg + r):
// tap scale off, split, one 8-byte store per plane into the output level's planes (HBM, for the filterbank), optionally a
// second copy into an LDS image of the level (`mir_hi` = its sample 0, lo plane `mir_stride` elements behind; no padding
// there; null = none), and — the tiles that hold samples 1..128 and L-129..L-2 — the level's reflect padding
// (nnaudio.py:300-301).  Shared by every decimator kernel: a level's bits do not depend on which kernel made it.
// TAIL = false: the level's reflect padding is written by somebody else (pl_reflect_pad_from_lds); the level's last,
// partial group of four is stored here either way.
// SWZ: the LDS image is a swizzled resident region (per-window kernel): `mir_hi` = the REGION's element 0 (sample 0 sits
// kPlPad elements behind it), elements at pl_swz_elems(region index).
template <bool TAIL = true, bool SWZ = false>
__device__ __forceinline__ void pl_tile_store(const f32x4& hh, const f32x4& xx, uint16_t* __restrict__ out_hi, int64_t stride,
                                              int L_out, int tile, int lane, uint16_t* mir_hi, int mir_stride) {
  const int m = lane & 15, kg = lane >> 4;
  const int o0 = kPlTileOut * tile;
  const int n0 = o0 + 16 * m + 4 * kg;
  float v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = (hh[r] + xx[r] * kLoUnscale) * kPlDmTapUnscale;
  uint2 h2, l2;
  split_f16x2_rn(f32x2{v[0], v[1]}, h2.x, l2.x);
  split_f16x2_rn(f32x2{v[2], v[3]}, h2.y, l2.y);
  uint16_t* oh = out_hi + kPlPad + n0;
  if (n0 + 3 < L_out) {
    pl_store8(oh, h2);
    pl_store8(oh + stride, l2);
  }
  if (mir_hi != nullptr) {  // wave-uniform
    uint16_t* mh = SWZ ? mir_hi + pl_swz_elems(kPlPad + n0) : mir_hi + n0;  // four elements: inside one half-row either way
    if (n0 + 3 < L_out) {
      *reinterpret_cast<uint2*>(mh) = h2;
      *reinterpret_cast<uint2*>(mh + mir_stride) = l2;
    } else if (n0 < L_out) {  // the level's last, partial group of four: zeros behind the last sample (images are sized in fours)
      const int nv = L_out - n0;  // 1 .. 3 valid
      const uint32_t m0 = nv > 1 ? 0xffffffffu : 0xffffu, m1 = nv > 2 ? 0xffffu : 0u;
      *reinterpret_cast<uint2*>(mh) = uint2{h2.x & m0, h2.y & m1};
      *reinterpret_cast<uint2*>(mh + mir_stride) = uint2{l2.x & m0, l2.y & m1};
    }
  }
  // the level's last (partial) group of four, and the reflect padding: the tiles that hold samples 1..128 and
  // L-129..L-2 write their mirror images (nnaudio.py:300-301).  Wave-uniform conditions, 16-bit stores.
  const bool tail = TAIL ? (o0 + kPlTileOut > L_out - 130 || tile == 0) : o0 + kPlTileOut > L_out;
  if (tail) {
    const uint16_t eh[4] = {(uint16_t)(h2.x & 0xffffu), (uint16_t)(h2.x >> 16), (uint16_t)(h2.y & 0xffffu), (uint16_t)(h2.y >> 16)};
    const uint16_t el[4] = {(uint16_t)(l2.x & 0xffffu), (uint16_t)(l2.x >> 16), (uint16_t)(l2.y & 0xffffu), (uint16_t)(l2.y >> 16)};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + r;
      if (n >= L_out) continue;
      if (n0 + 3 >= L_out) {
        oh[r] = eh[r];
        oh[stride + r] = el[r];
      }
      if constexpr (TAIL) {
        if (n >= 1 && n <= kPlPad) {
          out_hi[kPlPad - n] = eh[r];
          out_hi[stride + kPlPad - n] = el[r];
        }
        if (n <= L_out - 2 && n >= L_out - 1 - kPlPad) {
          const int q = kPlPad + 2 * (L_out - 1) - n;
          out_hi[q] = eh[r];
          out_hi[stride + q] = el[r];
        }
      }
    }
  }
}

// A level's reflect padding in its HBM planes (nnaudio.py:300-301: 128 mirrored samples in front and behind, the edge
// sample not repeated) from the level's LDS image (`img` = its sample 0, lo plane `img_stride` elements behind), by ONE
// wave: out[kPlPad - n] = s[n], n = 1 .. 128, and out[kPlPad + L + j] = s[L - 2 - j], j = 0 .. 127 — two elements per
// lane, end and plane.  The bits pl_tile_store<true> writes; off the tiles' critical path (below level 4 every tile of a
// level holds padding samples, and the scattered 16-bit stores were a third of a one-tile level's time).
// `region` = the swizzled resident region of the level (sample n at pl_swz_elems(kPlPad + n)).
__device__ __forceinline__ void pl_reflect_pad_from_lds(const uint16_t* region, int img_stride, int L, uint16_t* __restrict__ out_hi,
                                                        int64_t stride, int lane) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int n = 2 * lane + 1 + e;  // 1 .. 128
    const int a = pl_swz_elems(kPlPad + n);
    out_hi[kPlPad - n] = region[a];
    out_hi[stride + kPlPad - n] = region[img_stride + a];
    const int j = 2 * lane + e;      // 0 .. 127
    const int b = pl_swz_elems(kPlPad + L - 2 - j);
    out_hi[kPlPad + L + j] = region[b];
    out_hi[stride + kPlPad + L + j] = region[img_stride + b];
  }
}

// One tile through a wave-private row image in LDS (the input comes from global memory: the fp32 signal or a level's planes).
// F32IN = false: the input level is a plane region (`raw` holds the lane's units of its hi / lo planes).
// F32IN = true:  the input is the fp32 signal (level 0): rows are split in registers.  (Level 0 has no planes: what the
//                filterbank cannot read from the audio — the windows mirrored at the ends of the signal — are the edge
//                rows, written by the kernels around this routine.)
// MIRROR: see pl_tile_store.
// PF:     k-steps of LDS fragment reads kept ahead of the matrix instructions (0 = the compiler's own order, which reads
//         each fragment right in front of its use and waits: fine where four waves per SIMD and a prefetched next item
//         cover it, 1.5 k cycles per tile where a tile's latency is the critical path — the per-window kernel).
// SWZ_MIR: the mirror image is a swizzled resident region (see pl_tile_store).
template <bool F32IN, bool MIRROR = false, int PF = 0, bool SWZ_MIR = false>
__device__ __forceinline__ void pl_dec_tile(const PlRaw<F32IN>& raw, int64_t stride, int L_in, uint16_t* __restrict__ out_hi,
                                            int L_out, int tile, const uint4 (&th)[kPlDmSteps], const uint4* __restrict__ tlo,
                                            uint4* __restrict__ rows, int lane, uint16_t* mir_hi = nullptr, int mir_stride = 0) {
  // keep the lo fragments in LDS: without an opaque offset the compiler hoists the 9 item-invariant reads into registers
  asm volatile("" : "+v"(lane));
  const int m = lane & 15, kg = lane >> 4;
  const int base = 2 * kPlTileOut * tile + 32 * m + 8 * kg;  // region element of this lane's own row
  uint4 ah, al, bh, bl;
  if constexpr (F32IN) {
    pl_split8(raw.a0, raw.a1, ah, al);
    pl_split8(raw.b0, raw.b1, bh, bl);
  } else {
    ah = raw.ah, al = raw.al, bh = raw.bh, bl = raw.bl;
    if (pl_tile_is_edge(tile, L_in)) {  // the planes carry reflect padding where the decimator wants zeros
      ah = pl_zero_outside(ah, base, L_in);
      al = pl_zero_outside(al, base, L_in);
      bh = pl_zero_outside(bh, base + 256, L_in);
      bl = pl_zero_outside(bl, base + 256, L_in);
    }
  }
  // the swizzled row image: row rho's unit kg at 4 rho + (kg ^ 2 p), p = (rho >> 2) & 1
  uint4* r0 = rows + m * kPlRowU + kg;
  uint4* r1 = rows + m * kPlRowU + (kg ^ 2);
  {
    uint4* wr = (m & 4) ? r1 : r0;  // rows m and m + 8 have the same p
    wr[0] = ah;
    wr[24 * kPlRowU] = al;
    if (m >= 8) {
      wr[8 * kPlRowU] = bh;
      wr[(24 + 8) * kPlRowU] = bl;
    }
  }
  auto row_at = [&](int s) { return ((m + s) & 4) ? r1 : r0; };  // the lane's unit of row m + s
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // three independent accumulator chains (hi hi, lo hi, hi lo: nine dependent matrix instructions each) — round 5: with
  // the two correction products on ONE accumulator the 18-deep dependent chain was the latency of a deep level's tile
  f32x4 hh = {0.f, 0.f, 0.f, 0.f}, xa = hh, xb = hh;
  const uint4* tl = tlo + lane;
  if constexpr (PF == 0) {
#pragma unroll
    for (int s = 0; s < kPlDmSteps; ++s) {
      const uint4* rs = row_at(s);
      const uint4 xh = rs[s * kPlRowU], xl = rs[(24 + s) * kPlRowU];
      const uint4 tls = tl[s * 64];
      hh = BP_PL_MFMA16(th[s], xh, hh);
      xa = BP_PL_MFMA16(tls, xh, xa);
      xb = BP_PL_MFMA16(th[s], xl, xb);
    }
  } else {
    uint4 xh[PF + 1], xl[PF + 1], tls[PF + 1];
    auto rd = [&](int s) {
      const uint4* rs = row_at(s);
      xh[s % (PF + 1)] = rs[s * kPlRowU];
      xl[s % (PF + 1)] = rs[(24 + s) * kPlRowU];
      tls[s % (PF + 1)] = tl[s * 64];
    };
#pragma unroll
    for (int s = 0; s < PF; ++s) rd(s);
#pragma unroll
    for (int s = 0; s < kPlDmSteps; ++s) {
      if (s + PF < kPlDmSteps) rd(s + PF);
      __builtin_amdgcn_sched_barrier(0);
      hh = BP_PL_MFMA16(th[s], xh[s % (PF + 1)], hh);
      xa = BP_PL_MFMA16(tls[s % (PF + 1)], xh[s % (PF + 1)], xa);
      xb = BP_PL_MFMA16(th[s], xl[s % (PF + 1)], xb);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // the rows are read: the next tile of this wave may overwrite them
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  pl_tile_store<true, SWZ_MIR>(hh, xa + xb, out_hi, stride, L_out, tile, lane, MIRROR ? mir_hi : nullptr, mir_stride);
}

// One tile whose input level is resident in LDS as contiguous hi / lo planes (round 5): the B fragment of lane (m, kg) at
// k-step s — the 8 elements from 2 o0 + 32 (m + s) + 8 kg of the region that starts kPlPad elements in front of the level's
// sample 0 — is ONE ds_read_b128 straight from the plane: no row image, no copy, no wavefront fence (the level was complete
// at the last workgroup barrier).  `in_hi` = LDS address of that region's element 0, lo plane `in_stride` elements behind.
// The region is ZERO beside the samples — kPlPad elements in front, kPwTail behind (the reference zero-pads the decimator's
// input, nnaudio.py:269-279) — so no tile masks anything: with the masks in registers (18 fragments x ~26 operations in
// an edge tile, and below level 4 every tile is one) a one-tile level took 2.2 us, half of it the masks.
// At the natural 64-byte row pitch lanes m and m + 4 share banks (2-way: 8 instead of 4 LDS cycles per read, ~70 cycles a
// tile).  The same matrix instructions in the same order on the same operands as pl_dec_tile: the same bits.
// `in_tile`: the tile's index inside the region `in_hi` starts (>= 0: a region that holds only part of the level — the
// chunks of level 0 — starts at a multiple of 16 tiles).
template <int PF, bool TAIL>
__device__ __forceinline__ void pl_dec_tile_lds(const uint16_t* in_hi, int in_stride, uint16_t* __restrict__ out_hi,
                                                int64_t stride, int L_out, int tile, const uint4 (&th)[kPlDmSteps],
                                                const uint4* __restrict__ tlo, int lane, uint16_t* mir_hi, int mir_stride,
                                                int in_tile = -1) {
  asm volatile("" : "+v"(lane));  // keep the filter's lo fragments in LDS (see pl_dec_tile)
  const int m = lane & 15, kg = lane >> 4;
  // the region is swizzled (see kPlRowU): the lane's unit of row 16 tile + m + s is kg ^ 2 p(s), p(s) = ((m + s) >> 2) & 1
  const int base = 2 * kPlTileOut * (in_tile >= 0 ? in_tile : tile) + 32 * m;
  const uint4* p0 = reinterpret_cast<const uint4*>(in_hi + base + 8 * kg);
  const uint4* p1 = reinterpret_cast<const uint4*>(in_hi + base + 8 * (kg ^ 2));
  static_assert((2 * kPlTileOut) % 256 == 0, "a tile starts on a swizzle period");
  const uint4* tl = tlo + lane;
  f32x4 hh = {0.f, 0.f, 0.f, 0.f}, xa = hh, xb = hh;
  uint4 xh[PF + 1], xl[PF + 1], tls[PF + 1];
  auto rd = [&](int s) {
    const uint4* ps = ((m + s) & 4) ? p1 : p0;
    xh[s % (PF + 1)] = ps[4 * s];
    xl[s % (PF + 1)] = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(ps + 4 * s) + in_stride);
    tls[s % (PF + 1)] = tl[s * 64];
  };
#pragma unroll
  for (int s = 0; s < PF; ++s) rd(s);
#pragma unroll
  for (int s = 0; s < kPlDmSteps; ++s) {
    if (s + PF < kPlDmSteps) rd(s + PF);
    __builtin_amdgcn_sched_barrier(0);
    hh = BP_PL_MFMA16(th[s], xh[s % (PF + 1)], hh);
    xa = BP_PL_MFMA16(tls[s % (PF + 1)], xh[s % (PF + 1)], xa);
    xb = BP_PL_MFMA16(th[s], xl[s % (PF + 1)], xb);
    __builtin_amdgcn_sched_barrier(0);
  }
  pl_tile_store<TAIL, true>(hh, xa + xb, out_hi, stride, L_out, tile, lane, mir_hi, mir_stride);
}

// The filter's hi fragments live in registers (36 VGPRs), its lo fragments in LDS (9 KB, one ds_read_b128 per k-step):
// with all 18 in registers the kernels would hold 3 waves per SIMD instead of 4.
__device__ __forceinline__ void pl_load_tfrag(const uint4* __restrict__ tfrag, uint4 (&th)[kPlDmSteps], uint4* tlo) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int s = 0; s < kPlDmSteps; ++s) th[s] = tfrag[s * 64 + lane];
  for (int i = threadIdx.x; i < kPlDmSteps * 64; i += blockDim.x) tlo[i] = tfrag[kPlDmSteps * 64 + i];
  __syncthreads();
}

// One level of every window.  F32IN: level 0 -> 1 from the fp32 audio (the tiles at the ends of a window also leave level
// 0's edge rows); else planes -> planes.  Waves walk (window, tile) items, the rows of the next item are fetched before the
// matrix work of the current one; no workgroup barrier after the fragments are in.  (Launches with fewer windows than half
// the CUs: the per-window kernels below would leave most of the chip idle.)
template <bool F32IN>
__global__ __launch_bounds__(256, 4) void pl_decimate_kernel(const float* __restrict__ audio, int64_t audio_stride,
                                                             uint16_t* __restrict__ pl, int64_t stride, int off_in, int L_in,
                                                             int off_out, int L_out, int tiles,
                                                             const uint4* __restrict__ tfrag, int n_windows,
                                                             int hop0) {
  __shared__ __attribute__((aligned(16))) uint4 tlo[kPlDmSteps * 64];
  __shared__ __attribute__((aligned(16))) uint4 rows_all[4 * kPlRowsU];
  uint4 th[kPlDmSteps];
  pl_load_tfrag(tfrag, th, tlo);
  const int lane = threadIdx.x & 63;
  uint4* rows = rows_all + wave_id() * kPlRowsU;
  const int n_items = n_windows * tiles;
  // items of this workgroup: blockIdx.x + gridDim.x * j, drawn from a counter in LDS (the older waves of a workgroup win
  // the issue arbitration and would otherwise run out of work long before the younger ones: see the filterbank below)
  __shared__ int s_next;
  if (threadIdx.x == 0) s_next = 0;
  __syncthreads();
  auto grab = [&]() -> int {
    int j = 0;
    if ((threadIdx.x & 63) == 0) j = atomicAdd(&s_next, 1);
    const int it = blockIdx.x + gridDim.x * __builtin_amdgcn_readfirstlane(j);
    return it < n_items ? it : -1;
  };
  // rows of TWO items ahead in flight (round 4: with one, a wave had ~3 KB outstanding and the launch sat at the
  // latency-bandwidth product of 16 waves per CU, not at the HBM rate — dropping the level-0 plane writes did not move it)
  auto fetch = [&](int it) {
    const int fb = it / tiles, ft = it - fb * tiles;
    return pl_fetch_rows<F32IN>(audio + (int64_t)fb * audio_stride, pl + (int64_t)fb * 2 * stride + off_in, stride, L_in, ft,
                                lane);
  };
  int item = grab();
  if (item < 0) return;
  int item1 = grab();
  int item2 = item1 >= 0 ? grab() : -1;
  PlRaw<F32IN> raw = fetch(item);
  PlRaw<F32IN> raw1 = fetch(item1 >= 0 ? item1 : item);
  for (;;) {
    const int item3 = item2 >= 0 ? grab() : -1;
    const PlRaw<F32IN> raw2 = fetch(item2 >= 0 ? item2 : item);
    const int b = item / tiles, tile = item - b * tiles;
    uint16_t* w = pl + (int64_t)b * 2 * stride;
    if constexpr (F32IN) {
      if (tile == 0 || tile == tiles - 1)  // wave-uniform
        pl_write_edge_rows(audio + (int64_t)b * audio_stride, L_in, reinterpret_cast<float*>(w + off_in), hop0, tile == 0, lane);
    }
    pl_dec_tile<F32IN>(raw, stride, L_in, w + off_out, L_out, tile, th, tlo, rows, lane);
    if (item1 < 0) break;
    raw = raw1, raw1 = raw2, item = item1, item1 = item2, item2 = item3;
  }
}

// The deeper levels of one window, one workgroup of 16 waves: a level is a few dozen tiles at most and depends on the one
// above it, so as separate launches each would pay a launch boundary and a ramp for a few microseconds of work.  The
// levels this workgroup reads again stay in LDS (hi and lo plane of levels `lds_first` .. last - 1, samples only: the
// decimator zero-pads, the two edge tiles of a level mask whatever lies beside the samples), so the seven dependent
// steps pay an LDS round trip and a barrier each, not a store-acknowledge + L2 read (28 us for 3 us of matrix work);
// every level is also written to its planes in HBM for the filterbank.
// (Since round 5 the 22.05 kHz pyramid of a launch with at least half a window per CU runs in pl_pyramid_window_kernel
// below; this one serves the extended 44.1 kHz pyramid, whose level 1 does not fit the CU's LDS, and the deep levels of
// small launches.)
struct PlTail {
  int first, last, lds_first;
};
constexpr int kPlTailThreads = 1024;
constexpr int kPlTailGuard = kPlPad;     // elements in front of the first resident level: tile 0 reads (and masks) them
constexpr int kPlTailLdsElems = 21760;   // per plane: guard + levels 2..7 of the 22.05 kHz pyramid (each rounded up to 8)

__host__ __device__ inline int pl_tail_lds_need(const PlGeo& g, int lds_first, int last) {
  int n = kPlTailGuard;
  for (int k = lds_first; k < last; ++k) n += (g.len[k] + 7) & ~7;
  return n;
}

__global__ __launch_bounds__(kPlTailThreads) void pl_decimate_tail_kernel(const float* __restrict__ audio, int64_t audio_stride,
                                                                       uint16_t* __restrict__ pl, PlGeo g, PlTail t,
                                                                       const uint4* __restrict__ tfrag) {
  __shared__ __attribute__((aligned(16))) uint4 tlo[kPlDmSteps * 64];
  __shared__ __attribute__((aligned(16))) uint4 rows_all[(kPlTailThreads / 64) * kPlRowsU];
  __shared__ __attribute__((aligned(16))) uint16_t s_pl[2 * kPlTailLdsElems];  // hi plane, lo plane
  const int lane = threadIdx.x & 63;
  const int wave = wave_id();
  uint16_t* w = pl + (int64_t)blockIdx.x * 2 * g.stride;
  // level 0's 32 edge rows, two per wave, before anything else is live in registers
  if (t.first == 1)
    pl_write_edge_row_pair(audio + (int64_t)blockIdx.x * audio_stride, g.len[0], reinterpret_cast<float*>(w + g.off[0]), g.hop0,
                           wave, lane);
  uint4 th[kPlDmSteps];
  pl_load_tfrag(tfrag, th, tlo);
  uint4* rows = rows_all + wave * kPlRowsU;
  int loff_in = 0, loff_out = kPlTailGuard;  // LDS element of sample 0 of the input / output level (when resident)
  for (int k = t.first; k <= t.last; ++k) {
    const int tiles = (g.len[k] + kPlTileOut - 1) / kPlTileOut;
    const bool in_lds = k - 1 >= t.lds_first, out_lds = k >= t.lds_first && k < t.last;  // workgroup-uniform
    uint16_t* mir = out_lds ? s_pl + loff_out : nullptr;
    if (k == 1) {
      // level 0 -> 1 straight from the fp32 audio (round 4: the wide launch that did this spent 18 of its 35 us on per-item
      // bookkeeping — queue draws, 64-bit addresses, edge predicates — with nothing to do: ablation in DESIGN_LOG.md).  Here a
      // wave walks tiles wave, wave + 16, ... of its workgroup's window, the next tile's rows in flight during the current
      // one's matrix work; level 1 goes to its planes in HBM (level 2 reads it back through L2 after the barrier below).
      const float* x = audio + (int64_t)blockIdx.x * audio_stride;
      int tile = wave;
      if (tile < tiles) {
        PlRaw<true> raw = pl_fetch_rows<true>(x, nullptr, 0, g.len[0], tile, lane);
        for (;;) {
          const int ntile = tile + kPlTailThreads / 64;
          const PlRaw<true> nraw = pl_fetch_rows<true>(x, nullptr, 0, g.len[0], ntile < tiles ? ntile : tile, lane);
          pl_dec_tile<true, false, 1>(raw, g.stride, g.len[0], w + g.off[1], g.len[1], tile, th, tlo, rows, lane);
          if (ntile >= tiles) break;
          raw = nraw, tile = ntile;
        }
      }
    } else
    for (int tile = wave; tile < tiles; tile += kPlTailThreads / 64) {
      PlRaw<false> raw;
      if (in_lds)
        raw = pl_fetch_rows<false>(nullptr, s_pl + loff_in - kPlPad, kPlTailLdsElems, g.len[k - 1], tile, lane);
      else
        raw = pl_fetch_rows<false>(nullptr, w + g.off[k - 1], g.stride, g.len[k - 1], tile, lane);
      pl_dec_tile<false, true, 3>(raw, g.stride, g.len[k - 1], w + g.off[k], g.len[k], tile, th, tlo, rows, lane, mir,
                                  kPlTailLdsElems);
    }
    __syncthreads();  // level k is complete: in LDS for this workgroup (and in L2: same CU, same L1, workgroup scope)
    if (out_lds) {
      loff_in = loff_out;
      loff_out += (g.len[k] + 7) & ~7;
    }
  }
}

// The whole 22.05 kHz pyramid of one window, one workgroup of 16 waves, every level a wave reads again resident in LDS
// (round 5).  What the round-4 kernel above spent per tile — ~350 instructions around 27 matrix instructions, for level
// 1 as for the last, and a round of 16 tiles is paced by instruction issue (four waves per SIMD in lockstep behind the
// level's barrier) — was mostly staging: every input row fetched, parked in a wave-private row image, fenced and read
// back.  Here
//   * level 0 -> 1 still goes through the row images (the input is the fp32 signal in HBM: fetched a tile ahead, split in
//     registers), but level 1 ALSO stays in LDS (region A, 88 KB: hi and lo plane, samples only);
//   * levels 2 .. 8 read their B fragments straight from the resident planes (pl_dec_tile_lds: 27 ds_read_b128 of the
//     signal + 9 of the filter's lo fragments, 27 matrix instructions, the store): ~125 instructions a tile;
//   * the LDS is time-shared: the 16 row images (60 KB, region B) are dead once level 1 is complete and take level 2;
//     level 1's region is dead once level 2 is complete and takes levels 3 .. 7 back to back;
//   * the barrier between levels waits for LDS traffic only (lds_barrier): the plane stores to HBM, which only the
//     filterbank launch reads, stay in flight.
// Every level is written to its planes in HBM as before; the bits are those of the kernels above (same matrix
// instructions in the same order, same split, same masks).
constexpr int kPwThreads = 1024;
constexpr int kPwGuard = kPlPad;   // zeros in front of a resident level (the decimator's zero padding; tile 0 reads them)
constexpr int kPwTail = 768;       // zeros behind it (the last tile's fragments reach at most 767 elements past the samples)
// (whole swizzle periods of 256 elements: a region's swizzle is then that of its plane, whatever its offset in it)
__host__ __device__ constexpr int pw_level_elems(int k) { return (kPwGuard + ((level_len(k) + 7) & ~7) + kPwTail + 255) & ~255; }
constexpr int kPwPlaneA = pw_level_elems(1);  // 22824 elements per plane: level 1; later levels 3 .. 7 back to back
constexpr int kPwPlaneB = pw_level_elems(2);  // 11864: level 2, in the space of the row images
static_assert(2 * kPwPlaneB * 2 <= (kPwThreads / 64) * kPlRowsU * 16, "level 2 fits the row images' space");
static_assert(pw_level_elems(3) + pw_level_elems(4) + pw_level_elems(5) + pw_level_elems(6) + pw_level_elems(7) <= kPwPlaneA,
              "levels 3..7 fit level 1's space");
static_assert(kPlDmSteps * 64 * 16 + (kPwThreads / 64) * kPlRowsU * 16 + 2 * kPwPlaneA * 2 <= 160 * 1024, "LDS budget");

// zero elements [from, to) of both planes of a resident region (from, to multiples of 4), all threads of the workgroup
__device__ __forceinline__ void pw_zero(uint16_t* hi, int stride, int from, int to) {
  for (int i = from + 4 * (int)threadIdx.x; i < to; i += 4 * kPwThreads) {
    const int a = pl_swz_elems(i);  // region element i (a group of four stays inside its half-row)
    *reinterpret_cast<uint2*>(hi + a) = uint2{0u, 0u};
    *reinterpret_cast<uint2*>(hi + stride + a) = uint2{0u, 0u};
  }
}

// levels 2 .. 8 with compile-time geometry (the kernel serves the 22.05 kHz pyramid only): no scalar loads of the level's
// lengths and offsets between the barriers of a 1-microsecond level
template <int K>
struct PwLevel {
  static constexpr int kLen = level_len(K), kLenIn = level_len(K - 1);
  static constexpr int kTiles = (kLen + kPlTileOut - 1) / kPlTileOut;
  static constexpr bool kKeep = K < kOctaves - 1;  // somebody reads this level again: it gets an LDS image
  // element offset of the level's region (its zero guard) inside its LDS plane: level 1 and 3 open region A, 2 opens B
  static constexpr int region_off() {
    int off = 0;
    for (int j = 3; j < K; ++j) off += pw_level_elems(j);
    return K <= 3 ? 0 : off;
  }
};

template <int K>
__device__ __forceinline__ void pw_level(uint16_t* reg_a, uint16_t* b16, uint16_t* w, const int (&off)[10], int64_t stride,
                                         const uint4 (&th)[kPlDmSteps], const uint4* tlo, int wave, int lane) {
  using G = PwLevel<K>;
  using GI = PwLevel<K - 1>;
  constexpr int kWaves = kPwThreads / 64;
  // input: level K - 1 (region A for K = 2 and K >= 4, region B for K = 3); output image: B for K = 2, A otherwise
  const uint16_t* in_hi = (K == 3 ? b16 : reg_a) + GI::region_off();
  constexpr int in_stride = K == 3 ? kPwPlaneB : kPwPlaneA;
  uint16_t* img = (K == 2 ? b16 : reg_a) + G::region_off();  // level K's (swizzled) region: sample 0 kPwGuard elements in
  constexpr int img_stride = K == 2 ? kPwPlaneB : kPwPlaneA;
  if constexpr (K == 2) {  // level 2's zero surroundings in region B (the row images' space)
    pw_zero(b16, kPwPlaneB, 0, kPwGuard);
    pw_zero(b16, kPwPlaneB, kPwGuard + ((G::kLen + 3) & ~3), kPwPlaneB);
  }
  if constexpr (K == 3) {  // those of levels 3 .. 7 in region A (level 1 is dead): one contiguous stretch behind each level
    pw_zero(reg_a, kPwPlaneA, 0, kPwGuard);
    pw_zero(reg_a, kPwPlaneA, PwLevel<3>::region_off() + kPwGuard + ((level_len(3) + 3) & ~3), PwLevel<4>::region_off() + kPwGuard);
    pw_zero(reg_a, kPwPlaneA, PwLevel<4>::region_off() + kPwGuard + ((level_len(4) + 3) & ~3), PwLevel<5>::region_off() + kPwGuard);
    pw_zero(reg_a, kPwPlaneA, PwLevel<5>::region_off() + kPwGuard + ((level_len(5) + 3) & ~3), PwLevel<6>::region_off() + kPwGuard);
    pw_zero(reg_a, kPwPlaneA, PwLevel<6>::region_off() + kPwGuard + ((level_len(6) + 3) & ~3), PwLevel<7>::region_off() + kPwGuard);
    pw_zero(reg_a, kPwPlaneA, PwLevel<7>::region_off() + kPwGuard + ((level_len(7) + 3) & ~3), PwLevel<7>::region_off() + pw_level_elems(7));
  }
  // the reflect padding of level K - 1's planes, from its image, by the youngest wave (it has the fewest tiles): levels
  // 2 .. 7; level 1 and level 8 (no image) write theirs from the tiles
  if constexpr (K >= 3)
    if (wave == kWaves - 1)
      pl_reflect_pad_from_lds(in_hi, in_stride, GI::kLen, w + off[K - 1], stride, lane);
  for (int tile = wave; tile < G::kTiles; tile += kWaves)
    pl_dec_tile_lds<3, !G::kKeep>(in_hi, in_stride, w + off[K], stride, G::kLen, tile, th, tlo, lane, G::kKeep ? img : nullptr,
                                  img_stride);
  lds_barrier();  // level K is complete
  PL_STAMP(0, 3 + K);
}

__global__ __launch_bounds__(kPwThreads) void pl_pyramid_window_kernel(const float* __restrict__ audio, int64_t audio_stride,
                                                                      uint16_t* __restrict__ pl, PlGeo g,
                                                                      const uint4* __restrict__ tfrag) {
  __shared__ __attribute__((aligned(16))) uint4 tlo[kPlDmSteps * 64];
  __shared__ __attribute__((aligned(16))) uint4 reg_b[(kPwThreads / 64) * kPlRowsU];
  __shared__ __attribute__((aligned(16))) uint16_t reg_a[2 * kPwPlaneA];
  const int lane = threadIdx.x & 63;
  const int wave = wave_id();
  constexpr int kWaves = kPwThreads / 64;
  static_assert(kWaves == 16, "two of level 0's 32 edge rows per wave");
  uint16_t* w = pl + (int64_t)blockIdx.x * 2 * g.stride;
  uint16_t* const b16 = reinterpret_cast<uint16_t*>(reg_b);
  const float* x = audio + (int64_t)blockIdx.x * audio_stride;
  constexpr int kL0 = kAudioN, kL1 = level_len(1);
  constexpr int tiles1 = (kL1 + kPlTileOut - 1) / kPlTileOut;
  PL_STAMP(0, 0);
  PL_STAMP_RT(0, 14);
  // The kernel's first memory round trips ALL AT ONCE (issued one behind the other they were 5.6 us of a 36 us kernel):
  // the first chunk of the signal, the filter fragments (hi: registers, lo: one 16-byte piece per thread for LDS), the
  // samples of this wave's two edge rows.
  //
  // Level 0 -> 1 through resident CHUNKS (round 5, second half): 16 tiles' worth of the fp32 signal (8,192 samples + the
  // 768 the last tile's fragments reach past them, zeros outside [0, L): nnaudio.py:269-279) are split to f16 hi + lo ONCE
  // per sample by the whole workgroup — coalesced float4 loads, the next chunk's in flight during this chunk's tiles — and
  // parked as swizzled planes in region B; the tiles then read their fragments straight from the planes like levels 2 .. 8
  // do (~150 instructions a tile).  The wave-private row images before it fetched, split and parked every sample 1.5 times
  // in per-lane code: ~350 instructions a tile, and instruction issue is what paces a round of 16 tiles.
  constexpr int kChunkTiles = 16;
  constexpr int kChunkSamples = 2 * kPlTileOut * kChunkTiles;        // 8192
  constexpr int kChunkElems = kChunkSamples + kPwTail;               // 8960 region elements per plane
  constexpr int kChunkGroups = kChunkElems / 4;                      // float4 groups: 2240
  constexpr int kChunkPer = (kChunkGroups + kPwThreads - 1) / kPwThreads;
  constexpr int kChunks = (tiles1 + kChunkTiles - 1) / kChunkTiles;
  static_assert(kChunkElems % 256 == 0 && 2 * kChunkElems * 2 <= (kPwThreads / 64) * kPlRowsU * 16, "a chunk fits region B");
  static_assert(kL0 % 4 == 0 && kPwGuard % 4 == 0, "a group of four samples lies inside the signal or outside it");
  float4 cv[kChunkPer];
  auto chunk_load = [&](int c) {
#pragma unroll
    for (int k = 0; k < kChunkPer; ++k) {
      const int gq = (int)threadIdx.x + k * kPwThreads;
      const int n = kChunkSamples * c + 4 * gq - kPwGuard;  // sample index of the group's first element
      cv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gq < kChunkGroups && n >= 0 && n < kL0) cv[k] = *reinterpret_cast<const float4*>(x + n);
    }
  };
  auto chunk_store = [&]() {
#pragma unroll
    for (int k = 0; k < kChunkPer; ++k) {
      const int gq = (int)threadIdx.x + k * kPwThreads;
      if (gq < kChunkGroups) {
        uint2 h2, l2;
        split_f16x2_rn(f32x2{cv[k].x, cv[k].y}, h2.x, l2.x);
        split_f16x2_rn(f32x2{cv[k].z, cv[k].w}, h2.y, l2.y);
        const int a = pl_swz_elems(4 * gq);
        *reinterpret_cast<uint2*>(b16 + a) = h2;
        *reinterpret_cast<uint2*>(b16 + kChunkElems + a) = l2;
      }
    }
  };
  chunk_load(0);
  uint4 th[kPlDmSteps];
#pragma unroll
  for (int s = 0; s < kPlDmSteps; ++s) th[s] = tfrag[s * 64 + lane];
  static_assert(kPlDmSteps * 64 <= kPwThreads, "one lo-fragment piece per thread");
  uint4 tlo_piece = uint4{0u, 0u, 0u, 0u};
  if (threadIdx.x < kPlDmSteps * 64) tlo_piece = tfrag[kPlDmSteps * 64 + threadIdx.x];
  float* edge_rows = reinterpret_cast<float*>(w + g.off[0]);
  const float4 er_a = pl_edge_row_load(x, kL0, wave, g.hop0, lane);
  const float4 er_b = pl_edge_row_load(x, kL0, (kPlTilesPerLevel - 1) * 16 + wave, g.hop0, lane);
  // (nothing above waits) level 1's zero surroundings in region A — its samples come from the tiles below
  pw_zero(reg_a, kPwPlaneA, 0, kPwGuard);
  pw_zero(reg_a, kPwPlaneA, kPwGuard + ((kL1 + 3) & ~3), kPwPlaneA);
  if (threadIdx.x < kPlDmSteps * 64) tlo[threadIdx.x] = tlo_piece;
  *reinterpret_cast<float4*>(edge_rows + wave * g.hop0 + 4 * lane) = er_a;
  *reinterpret_cast<float4*>(edge_rows + (16 + wave) * g.hop0 + 4 * lane) = er_b;
  PL_STAMP(0, 1);
  int off[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) off[k] = g.off[k];
#pragma unroll 1
  for (int c = 0; c < kChunks; ++c) {
    chunk_store();                      // chunk c: split, into region B
    if (c + 1 < kChunks) chunk_load(c + 1);
    lds_barrier();                      // the chunk (and, the first time, the lo fragments) are in LDS
    if (c == 0) PL_STAMP(0, 2);
    const int tile = kChunkTiles * c + wave;
    if (tile < tiles1)
      pl_dec_tile_lds<3, true>(b16, kChunkElems, w + off[1], g.stride, kL1, tile, th, tlo, lane, reg_a, kPwPlaneA, wave);
    lds_barrier();                      // every wave has read the chunk
  }
  PL_STAMP(0, 3);
  PL_STAMP(0, 4);  // (level 1 is complete in region A, the chunk buffer is dead: the loop's last barrier)
  pw_level<2>(reg_a, b16, w, off, g.stride, th, tlo, wave, lane);
  pw_level<3>(reg_a, b16, w, off, g.stride, th, tlo, wave, lane);
  pw_level<4>(reg_a, b16, w, off, g.stride, th, tlo, wave, lane);
  pw_level<5>(reg_a, b16, w, off, g.stride, th, tlo, wave, lane);
  pw_level<6>(reg_a, b16, w, off, g.stride, th, tlo, wave, lane);
  pw_level<7>(reg_a, b16, w, off, g.stride, th, tlo, wave, lane);
  pw_level<8>(reg_a, b16, w, off, g.stride, th, tlo, wave, lane);
  PL_STAMP_RT(0, 15);
}

// ================================================================================================
// host side
void launch_planes_split(const float* src, int64_t src_stride, int level, uint16_t* pl, int n_windows, bool ext,
                         hipStream_t stream) {
  const PlGeo g = make_pl_geo(ext);
  const int units = g.rlen[level] / 8;
  hipLaunchKernelGGL(pl_split_kernel, dim3((units + 255) / 256, n_windows), dim3(256), 0, stream, src, src_stride,
                     g.len[level], pl, g.stride, g.off[level], g.rlen[level]);
}

void launch_planes_edge_rows(const float* audio, int64_t audio_stride, uint16_t* pl, int n_windows, bool ext,
                             hipStream_t stream) {
  const PlGeo g = make_pl_geo(ext);
  hipLaunchKernelGGL(pl_edge_rows_kernel, dim3(n_windows), dim3(64), 0, stream, audio, audio_stride, g.len[0], pl, g.stride,
                     g.off[0], g.hop0);
}

void launch_planes_unsplit(const uint16_t* pl, int level, float* dst, int64_t dst_stride, int n_windows, bool ext,
                           hipStream_t stream) {
  const PlGeo g = make_pl_geo(ext);
  hipLaunchKernelGGL(pl_unsplit_kernel, dim3((g.len[level] + 255) / 256, n_windows), dim3(256), 0, stream, pl, g.stride,
                     g.off[level], g.len[level], dst, dst_stride);
}

// levels 1 .. n-1 (planes) and level 0's edge rows from the fp32 audio
void launch_pyramid_planes(const float* audio, int64_t audio_stride, uint16_t* pl, const void* tfrag, int n_windows, int n_cu,
                           bool ext, hipStream_t stream) {
  const PlGeo g = make_pl_geo(ext);
  const uint4* tf = static_cast<const uint4*>(tfrag);
  // with at least half a window per CU (the 22.05 kHz kernel: a third) the whole pyramid is ONE launch (launch_plan.h)
  const bool one_launch = pyramid_one_launch(n_windows, n_cu, ext);
  if (one_launch && !ext) {
    hipLaunchKernelGGL(pl_pyramid_window_kernel, dim3(n_windows), dim3(kPwThreads), 0, stream, audio, audio_stride, pl, g, tf);
    return;
  }
  if (!one_launch) {
    const int tiles = (g.len[1] + kPlTileOut - 1) / kPlTileOut;
    const int grid = pyramid_decimate_grid(tiles, n_windows, n_cu);
    hipLaunchKernelGGL(pl_decimate_kernel<true>, dim3(grid), dim3(256), 0, stream, audio, audio_stride, pl, g.stride, g.off[0],
                       g.len[0], g.off[1], g.len[1], tiles, tf, n_windows, g.hop0);
  }
  // with fewer windows than CUs the per-window kernel would leave most of the chip idle on the long levels: those run wide
  int first_tail = one_launch ? 1 : 2;
  if (!one_launch)
    for (; first_tail < g.n_levels && g.len[first_tail] > 16 * kPlTileOut; ++first_tail) {
      const int k = first_tail;
      const int tiles = (g.len[k] + kPlTileOut - 1) / kPlTileOut;
      const int grid = pyramid_decimate_grid(tiles, n_windows, n_cu);
      hipLaunchKernelGGL(pl_decimate_kernel<false>, dim3(grid), dim3(256), 0, stream, (const float*)nullptr, (int64_t)0, pl,
                         g.stride, g.off[k - 1], g.len[k - 1], g.off[k], g.len[k], tiles, tf, n_windows, 0);
    }
  if (first_tail < g.n_levels) {
    // levels kept in LDS: as many of the deepest ones as fit (22.05 kHz: all from level 2; extended pyramid: from level 3)
    int lds_first = first_tail < 2 ? 2 : first_tail;
    while (pl_tail_lds_need(g, lds_first, g.n_levels - 1) > kPlTailLdsElems) ++lds_first;
    hipLaunchKernelGGL(pl_decimate_tail_kernel, dim3(n_windows), dim3(kPlTailThreads), 0, stream, audio, audio_stride, pl, g,
                       PlTail{first_tail, g.n_levels - 1, lds_first}, tf);
  }
}

#ifdef PL_PROF
int pl_prof_pyramid(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pl_prof), sizeof(g_pl_prof)); }
#endif

}  // namespace bp
