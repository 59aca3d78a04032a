// A/B kernel of the contour conv1 — compiled only into builds with -DBP_AB_KERNELS (basic_pitch_amd/build.py
// build_library(ab=True): the comparison tests and tools); the product library does not carry it.  The default path is
// conv_contour_march.hip (interior) + conv_contour_rim_march.hip / conv_contour_rim.hip (rim) + conv_contour2.hip (conv2).
// Here: the round-2 folded conv1 of the interior bins (BP_CONV1=rounds), the kernel the march is tested against.
//
//   contour_conv1_folded_kernel   Conv2D 8->8, (3 frames x 39 bins), "same", folded BN, ReLU on the harmonic stack
//                                 (basic_pitch/models.py:241-250, nn.py:69-88), groups 5..60     zp -> c1
//
// Why not one fused kernel (conv_contour.hip): 65 % of the whole path's FLOPs are conv1, and the fused
// kernel's matrix pipe idles two thirds of the time — the register-resident weights force a K split over 4
// waves, so every 32-position tile pays a cross-wave reduction, two barriers and a serial conv2 epilogue
// (measured: 2.2 k cycles of MFMA phase + 4.5 k cycles of latency-bound epilogue per tile; neither more
// prefetch nor software pipelining across tiles nor de-phasing the two resident workgroups moved it, see
// DESIGN.md §7).  Here conv1 is a pure matrix kernel and the tiny conv2 runs at the HBM rate behind it.
//
// conv1 mapping (v_mfma_f32_32x32x16_f16, split-precision operands, bp_common.h):
//   C[(bin offset j, out channel o) (32 rows)][position (32 cols)] = Wt[(j,o)][k] x S[k][position]
//   * position = (frame, group of 4 adjacent bins); rows carry a 4-bin Toeplitz expansion of the kernel.
//   * NO K split: every wave owns complete sums of its positions — no reduction, no barrier per tile — and stores c1
//     straight from the accumulator layout after bias and ReLU (a lane holds 4 consecutive channels of a pixel = one
//     16-byte store).
//   * a round (256 positions = 3.9 image rows) ends with the only barrier; the image rows of the NEXT round
//     are gathered from zp (8 harmonic shifts, no masks: zp carries its own zero padding) and written to the
//     ring between the MFMAs of the current round.
//
// Roofline: f16 MFMA issue — 577 MFLOP per window algorithmic (56 of conv1's 66 groups), 3 f16 MFMAs per product (hi*hi,
// lo*hi, hi*lo); 312 KB (zp) read, 1.25 MB (c1) written per window.
#include "bp_kernels.h"

namespace bp {

constexpr int kD1EdgeGroups = 5;                   // groups 0..4 and 61..65 see the crop of the stack (bins < 20, >= 244)

struct Conv1Params {
  const uint32_t* zp;   // [n][kZRowsP][kZRow] padded pre-split z (zpack_kernel)
  const uint4* wlds;    // [3][12][hi|lo][64] x (8 x f16) A fragments
  const float* bias;    // [8]
  float* c1;            // [n][172][kC1Row][8] relu(conv1), 2 zero bins of padding either side of a row
  int n_windows;
  int chunks;           // row chunks per window (work items = n_windows * chunks)
};

// bias + ReLU and the c1 store: register r of a lane is (bin offset j = r >> 2, channel o = 4 kh + (r & 3))
__device__ __forceinline__ void d1_store(float* __restrict__ dst, const f32x16& hh, const f32x16& xx,
                                         const float (&bias4)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float4 v;
    v.x = fmaxf((hh[4 * j + 0] + xx[4 * j + 0] * kLoUnscale) + bias4[0], 0.0f);
    v.y = fmaxf((hh[4 * j + 1] + xx[4 * j + 1] * kLoUnscale) + bias4[1], 0.0f);
    v.z = fmaxf((hh[4 * j + 2] + xx[4 * j + 2] * kLoUnscale) + bias4[2], 0.0f);
    v.w = fmaxf((hh[4 * j + 3] + xx[4 * j + 3] * kLoUnscale) + bias4[3], 0.0f);
    *reinterpret_cast<float4*>(dst + j * 8) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------
// Folded conv1 for the interior of the stack (groups 5..60 = bins 20..243).
//
// The 8 stack channels are shifted copies of ONE image (z at bin f + s_c, s = -36, 0, 36, 57, 72, 84, 93, 101:
// nn.py:51-54,73-85), so away from the crop the 8 x 39-tap kernels of an output channel collapse into a single
// kernel over z:   K[o][dt][g] = sum_c W1[o][c][dt][g - s_c + 19],   g in [-55, 120]   (176 taps: the eight 39-tap
// intervals overlap or abut).  K = 3 x 176 = 528 instead of 3 x 312 = 936 products per output: 36 k-steps of 16
// taps (179 with the 4-bin Toeplitz expansion, 192 padded) instead of the 8-channel form's 63.  The MFMA mapping is the one above:
//   C[(j, o)][position] = Kt[(j, o)][tap'] x Z[tap'][position],   Z[tap'][m] = z[4 m + tap' - 56]
//   * B: 8 consecutive taps = 8 consecutive z bins = 16 bytes of the f16 image row; the lane stride is 4 bins = 8
//     bytes, so each row is kept twice (the second copy shifted by 4 bins) and odd groups read the shifted copy:
//     every read is an aligned ds_read_b128;
//   * A: Toeplitz-expanded fragments straight from LDS ([dt][k-step][hi|lo][lane], 73.7 KB), packed on the host.
// At the rim (bins < 20 or >= 244) "crop to 264 bins, then zero-pad" removes a different set of taps for every
// output bin: those 2 x 5 groups per frame are the rim kernels' (conv_contour_rim_march.hip, conv_contour_rim.hip).
constexpr int kF1Threads = 512;
constexpr int kF1Steps = 36;                       // 3 frames x 12 k-steps of 16 taps
constexpr int kF1Groups = 56;                      // groups 5..60
// LDS layout of a z row: hi copy 0, hi copy 1 (shifted 4 bins), lo copy 0, lo copy 1, kF1Copy 16-byte units each.
// A ds_read_b128 is serviced in four groups of 16 lanes — {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same
// + 32 (MI355X_MICROARCH.md, LDS) — and a group is conflict-free when its 16 units fall into 16 distinct 16-byte bank
// columns (unit index mod 16).  A wave's 32 lanes are consecutive (frame, group) positions, even groups reading copy 0
// at unit m / 2 and odd groups copy 1 at kF1Copy + (m - 1) / 2, wrapping to the next frame (+ row stride - 28 units)
// after group 60.  Enumerating every tile start: copies 73 units apart and a row stride of 4 x 73 = 292 give ZERO
// conflicts (the first layout, 72 / 288, cost 4.3 extra LDS cycles per group: SQ_LDS_BANK_CONFLICT 3.2e7 per launch);
// the ring is 16 rows so that its own wrap (16 strides) keeps the columns too.
constexpr int kF1Ring = 16;                        // z rows resident
constexpr int kF1Copy = 73;                        // uint4 per row copy (464 f16 used)
constexpr int kF1RowU4 = 4 * kF1Copy;
constexpr int kF1Round = 256;
constexpr int kF1Pf = 3;
static_assert(kF1Ring * kF1RowU4 * 16 + 3 * 12 * 2 * 64 * 16 <= 160 * 1024, "LDS budget");

template <bool WLO>
__global__ __launch_bounds__(kF1Threads, 2) void contour_conv1_folded_kernel(Conv1Params p) {
  __shared__ __attribute__((aligned(16))) uint4 zimg[kF1Ring * kF1RowU4];
  __shared__ __attribute__((aligned(16))) uint4 afr[kF1Steps * 2 * 64];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = wave_id();
  const int kh = lane >> 5, li = lane & 31;

  for (int i = tid; i < kF1Steps * 2 * 64; i += kF1Threads) afr[i] = p.wlds[i];
  for (int i = tid; i < kF1Ring * kF1RowU4; i += kF1Threads) zimg[i] = uint4{0u, 0u, 0u, 0u};
  float bias4[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) bias4[q] = p.bias[4 * kh + q];

  // one staging task = 4 consecutive zp words (bins 4 u - 56 .. 4 u - 53) of one image row -> 8 B of hi and of lo,
  // written to copy 0 at element 4 u and to copy 1 (shifted by 4 bins) at element 4 u - 4
  constexpr int kTasksRow = kZRow / 4;  // 112
  auto stage_row_task = [&](const uint32_t* __restrict__ zwin, int row, int u) {
    const uint4 wv = *reinterpret_cast<const uint4*>(zwin + (int64_t)(row + 1) * kZRow + 4 * u);
    uint2 h2, l2;
    h2.x = (wv.x & 0xffffu) | (wv.y << 16);
    h2.y = (wv.z & 0xffffu) | (wv.w << 16);
    l2.x = (wv.x >> 16) | (wv.y & 0xffff0000u);
    l2.y = (wv.z >> 16) | (wv.w & 0xffff0000u);
    uint2* rowp = reinterpret_cast<uint2*>(zimg + ((row + kF1Ring) % kF1Ring) * kF1RowU4);
    rowp[u] = h2;                                   // hi copy 0
    rowp[2 * 2 * kF1Copy + u] = l2;                 // lo copy 0
    if (u > 0) {
      rowp[2 * kF1Copy + u - 1] = h2;               // hi copy 1
      rowp[2 * 3 * kF1Copy + u - 1] = l2;           // lo copy 1
    }
  };

  const int rows_per = (kFrames + p.chunks - 1) / p.chunks;
  const int n_items = p.n_windows * p.chunks;
  for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int b = item / p.chunks;
    const int t0 = (item - b * p.chunks) * rows_per;
    const int t1 = t0 + rows_per < kFrames ? t0 + rows_per : kFrames;
    const int npos = (t1 - t0) * kF1Groups;
    const int nrounds = (npos + kF1Round - 1) / kF1Round;
    const uint32_t* zwin = p.zp + (int64_t)b * kZWin;  // padded window: frame -1 is row 0, bin -56 is word 0
    float* c1b = p.c1 + (int64_t)b * kC1Win;

    lds_barrier();
    int staged_hi = t0 + (kF1Round - 1) / kF1Groups + 1;
    staged_hi = staged_hi < t1 ? staged_hi : t1;
    for (int e = tid; e < (staged_hi - t0 + 2) * kTasksRow; e += kF1Threads) {
      const int ri = e / kTasksRow;
      stage_row_task(zwin, t0 - 1 + ri, e - ri * kTasksRow);
    }
    lds_barrier();

    for (int k = 0; k < nrounds; ++k) {
      int need_hi = t0 + (kF1Round * (k + 1) + kF1Round - 1) / kF1Groups + 1;
      need_hi = need_hi < t1 ? need_hi : t1;
      const int n_new = (k + 1 < nrounds) ? need_hi - staged_hi : 0;
      const int first_new = staged_hi + 1;

      const int pos = kF1Round * k + 32 * w + li;
      const bool pvalid = pos < npos;
      const int posc = pvalid ? pos : npos - 1;
      const int prr = posc / kF1Groups;
      const int pgrp = kD1EdgeGroups + posc - prr * kF1Groups;  // group 5..60
      const int prow = t0 + prr;
      // B operand: z elements 4 m + 16 s + 8 kh .. + 7 of copy (m & 1); uint4 index (m - copy) / 2 + kh + 2 s
      const int cpy = pgrp & 1;
      const int boff = cpy * kF1Copy + ((pgrp - cpy) >> 1) + kh;
      int rowb[3];
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) rowb[dt] = ((prow - 1 + dt + kF1Ring) % kF1Ring) * kF1RowU4 + boff;

      f32x16 hh, xx;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        hh[r] = 0.0f;
        xx[r] = 0.0f;
      }
      f16x8 ah[kF1Steps], al[kF1Steps], bh[kF1Steps], bl[kF1Steps];
      auto issue = [&](int s) {
        const int dt = s / 12, e = s - 12 * dt;
        if (WLO) al[s] = __builtin_bit_cast(f16x8, afr[(2 * s + 1) * 64 + lane]);
        bh[s] = __builtin_bit_cast(f16x8, zimg[rowb[dt] + 2 * e]);
        ah[s] = __builtin_bit_cast(f16x8, afr[(2 * s) * 64 + lane]);
        bl[s] = __builtin_bit_cast(f16x8, zimg[rowb[dt] + 2 * e + 2 * kF1Copy]);
      };
#pragma unroll
      for (int s = 0; s < kF1Pf; ++s) issue(s);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < kF1Steps; ++s) {
        if (s + kF1Pf < kF1Steps) issue(s + kF1Pf);
        // the z rows of the next round: at most 6 rows x 112 tasks, two per thread, early in the round
        if (s == 2 || s == 14) {
          const int e = (s == 2 ? 0 : kF1Threads) + tid;
          if (e < n_new * kTasksRow) {
            const int ri = e / kTasksRow;
            stage_row_task(zwin, first_new + ri, e - ri * kTasksRow);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (WLO) xx = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[s], bh[s], xx, 0, 0, 0);
        hh = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], bh[s], hh, 0, 0, 0);
        xx = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], bl[s], xx, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      staged_hi += n_new;
      if (pvalid) d1_store(c1b + ((int64_t)prow * kC1Row + kC1Pad + 4 * pgrp) * 8 + 4 * kh, hh, xx, bias4);
      lds_barrier();
    }
  }
}

static int conv1_chunks(int n_windows, int n_cu) {
  // one workgroup per CU; split windows into row chunks when there are fewer windows than CUs
  int chunks = 1;
  while (chunks < 4 && n_windows * chunks < n_cu) chunks *= 2;
  return chunks;
}

// folded kernel: the interior groups
void launch_contour_conv1_folded(const uint32_t* zp, const void* wfold, const float* bias, float* c1, int n_windows,
                                 int n_cu, bool weights_have_lo, hipStream_t stream) {
  Conv1Params p{zp, static_cast<const uint4*>(wfold), bias, c1, n_windows, conv1_chunks(n_windows, n_cu)};
  const int items = p.n_windows * p.chunks;
  const int grid = items < n_cu ? items : n_cu;
  if (weights_have_lo)
    hipLaunchKernelGGL(contour_conv1_folded_kernel<true>, dim3(grid), dim3(kF1Threads), 0, stream, p);
  else
    hipLaunchKernelGGL(contour_conv1_folded_kernel<false>, dim3(grid), dim3(kF1Threads), 0, stream, p);
}

}  // namespace bp
