// The f0 peaks of contour rows on the device (include/basic_pitch_amd_multipitch.h): picked, refined and
// compacted for the segments of a job (count -> scan -> write), and the decodes of a threshold / band sweep scored frame by
// frame where the peaks are (one workgroup per decode).
//
// A WAVE TAKES A ROW.  A row is 264 cells, four wave-widths and eight cells: lane l reads the cells l, 64 + l, ..., 256 + l
// (coalesced; the fifth load only in lanes 0 ... 7) and, where its bin may be a peak (1 ... 262, so b - 1 and b + 1 stay in the
// row and no read crosses a row, let alone a segment), the two neighbours by shifted loads of lines the wave has just
// fetched.  The peak predicate is the header's in float32; __ballot makes the five 64-bit words of the row's peak mask,
// their popcount is the row's count and the popcount below a lane's bit its peak's rank in the row: the order by bin is
// structural.  A cell that is not finite flags the row's segment (an atomic OR; the flag only ever becomes 1).
//
// The order by frame over millions of rows is an exclusive scan of the row counts, and it cannot be folded into the count
// pass: a flagged segment has NO points, and which segments are flagged is known only when every row has been seen.  So
// the scan is a launch of its own, ONE workgroup of kMpScanTile lanes that takes kMpScanTile rows a pass with the rows of
// flagged segments counted as empty and carries the sum from pass to pass in a register; a second small launch reads the
// points before each segment's first row as the point offsets.  At 8 bytes read and 8 written per row it is a fraction of the
// count pass's 1,056.  The write pass is only launched once the host has seen that the total fits the caller's room: it
// recomputes the mask and stores each peak, refined, at its row's first slot plus its rank.
//
// The refinement is the header's in float64 — `#pragma clang fp contract(off) reassociate(off)` keeps it as written; the
// division is the IEEE one — so the points equal the host checker's bit for bit (tests/test_gpu_multipitch.py).
//
// No indexed register array (the five words are unrolled by a template parameter), no recursion: no scratch.
#include "bp_kernels.h"

#pragma clang fp contract(off)
#pragma clang fp reassociate(off)

namespace bp {

namespace {

constexpr int kWidth = 256, kWaves = kWidth / 64;
constexpr int kRowsPerBlock = 64;  // of the count and write passes: 16 rows a wave
constexpr int kMaxPeaks = 132;     // a row's peaks (at most 131), rounded up to an even count

struct MpPoint {  // bp_f0_point
  int32_t frame;
  float salience;
  double pitch_midi;
};
static_assert(sizeof(MpPoint) == 16, "bp_f0_point");

struct MpCell {
  float l, c, r;
  bool peak;
};

__device__ __forceinline__ bool mp_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// word K of the row's peak mask; the lane's cell of it with its neighbours; *bad: the lane saw a cell that is not finite
template <int K>
__device__ __forceinline__ unsigned long long mp_mask(const float* __restrict__ row, int lane, const MpParams& p, MpCell* cell, bool* bad) {
  const int b = 64 * K + lane;
  MpCell v{0.0f, 0.0f, 0.0f, false};
  if (b < kMpBins) {
    v.c = row[b];
    *bad = *bad || !mp_finite(v.c);
    if (b >= 1 && b <= kMpBins - 2 && b >= p.min_bin && b <= p.max_bin) {
      v.l = row[b - 1], v.r = row[b + 1];
      v.peak = v.c >= p.threshold && v.c > v.l && v.c > v.r;
    }
  }
  *cell = v;
  return __ballot(v.peak);
}

__device__ __forceinline__ double mp_pitch(int b, const MpCell& v) {
  const double l = (double)v.l, c = (double)v.c, r = (double)v.r;
  const double delta = 0.5 * (l - r) / ((l - 2.0 * c) + r);
  return 21.0 + ((double)b + delta) / 3.0;
}

__device__ __forceinline__ int mp_rank(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// the segment of row r: the last i of 0 ... n_segs - 1 with offs[i] <= r (segments without rows are passed over)
__device__ __forceinline__ int mp_segment(const int64_t* __restrict__ offs, int64_t n_segs, int64_t r) {
  int64_t lo = 0, hi = n_segs;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (offs[mid] <= r) lo = mid;
    else hi = mid;
  }
  return (int)lo;
}

__global__ __launch_bounds__(kWidth) void mp_count_kernel(const float* __restrict__ contour, const int64_t* __restrict__ offs, int64_t n_segs,
                                                          int64_t T, MpParams p, int2* __restrict__ row_info, int32_t* __restrict__ seg_bad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = 0; i < kRowsPerBlock / kWaves; ++i) {
    const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + i * kWaves + wave;
    if (r >= T) break;
    const float* row = contour + r * kMpBins;
    MpCell cell;
    bool bad = false;
    int n = __popcll(mp_mask<0>(row, lane, p, &cell, &bad));
    n += __popcll(mp_mask<1>(row, lane, p, &cell, &bad));
    n += __popcll(mp_mask<2>(row, lane, p, &cell, &bad));
    n += __popcll(mp_mask<3>(row, lane, p, &cell, &bad));
    n += __popcll(mp_mask<4>(row, lane, p, &cell, &bad));
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0) {
      const int seg = mp_segment(offs, n_segs, r);
      row_info[r] = make_int2(n, seg);
      if (any_bad) atomicOr(&seg_bad[seg], 1);
    }
  }
}

// one workgroup: row_first[r] = the points before row r, row_first[T] = all
__global__ __launch_bounds__(kMpScanTile) void mp_scan_kernel(const int2* __restrict__ row_info, const int32_t* __restrict__ seg_bad, int64_t T,
                                                              int64_t* __restrict__ row_first) {
  __shared__ int s_wave[kMpScanTile / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t carry = 0;
  for (int64_t base = 0; base < T; base += kMpScanTile) {
    const int64_t r = base + tid;
    int v = 0;
    if (r < T) {
      const int2 info = row_info[r];
      v = seg_bad[info.y] ? 0 : info.x;
    }
    int incl = v;  // (a tile holds at most 1,024 x 131 points: 32 bits)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kMpScanTile / 64; ++w) {
      const int s = s_wave[w];
      before += w < wave ? s : 0;
      total += s;
    }
    if (r < T) row_first[r] = carry + before + (incl - v);
    carry += total;
    __syncthreads();  // s_wave is read: the next pass may write it
  }
  if (tid == 0) row_first[T] = carry;
}

// meta: point_offsets [n_segs + 1], then as 32-bit words the statuses [n_segs]
__global__ __launch_bounds__(kWidth) void mp_offsets_kernel(const int64_t* __restrict__ offs, const int64_t* __restrict__ row_first,
                                                            const int32_t* __restrict__ seg_bad, int64_t n_segs, int64_t* __restrict__ meta) {
  const int64_t i = (int64_t)blockIdx.x * kWidth + threadIdx.x;
  if (i > n_segs) return;
  meta[i] = row_first[offs[i]];
  if (i < n_segs) reinterpret_cast<int32_t*>(meta + n_segs + 1)[i] = seg_bad[i] ? 1 : 0;
}

template <int K>
__device__ __forceinline__ int mp_store(const float* __restrict__ row, int lane, const MpParams& p, int32_t frame, MpPoint* __restrict__ out, int before) {
  MpCell cell;
  bool bad = false;
  const unsigned long long m = mp_mask<K>(row, lane, p, &cell, &bad);
  if (cell.peak) out[before + mp_rank(m, lane)] = MpPoint{frame, cell.c, mp_pitch(64 * K + lane, cell)};
  return before + __popcll(m);
}

__global__ __launch_bounds__(kWidth) void mp_write_kernel(const float* __restrict__ contour, int64_t T, MpParams p, const int2* __restrict__ row_info,
                                                          const int32_t* __restrict__ seg_bad, const int64_t* __restrict__ offs,
                                                          const int64_t* __restrict__ row_first, MpPoint* __restrict__ points) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = 0; i < kRowsPerBlock / kWaves; ++i) {
    const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + i * kWaves + wave;
    if (r >= T) break;
    const int2 info = row_info[r];
    if (info.x == 0 || seg_bad[info.y]) continue;
    const float* row = contour + r * kMpBins;
    MpPoint* out = points + row_first[r];
    const int32_t frame = (int32_t)(r - offs[info.y]);
    int n = mp_store<0>(row, lane, p, frame, out, 0);
    n = mp_store<1>(row, lane, p, frame, out, n);
    n = mp_store<2>(row, lane, p, frame, out, n);
    n = mp_store<3>(row, lane, p, frame, out, n);
    (void)mp_store<4>(row, lane, p, frame, out, n);
  }
}

// ---- a sweep scored where the peaks are: ONE WORKGROUP PER DECODE, a wave takes a frame.  The peak mask as above; the
// refined pitches go, in bin order, into the wave's own kMaxPeaks doubles of LDS (written and read by that wave alone: its LDS
// instructions complete in order, no barrier); then the refs of the segment, IN ASCENDING PITCH with the frames they sound on
// (the host's table), are tested 64 at a time, and each that sounds takes the lowest free estimate it hits — the greedy the
// header allows: `next` passes the estimates that are taken or too low for this ref and every later one.  The walk is the same
// in every lane.  The sums are 64-bit and per wave; one LDS step joins the waves.
//
// Width.  Four waves for the jobs of short segments — a one-window decode is 142 frames, 36 a wave, and a compute unit holds
// eight such workgroups —, sixteen where the job's longest decode has more than kMpSweepLongRows rows: the decodes of a whole
// track are few and long, the frames are independent, and a workgroup is all that works on one (measured on one 110-window
// track under 64 sets, four waves: 29.6 ms, profiles/multipitch.md).  The counts do not depend on the width: every frame is
// matched by one wave alone and the sums are integers.
template <int K>
__device__ __forceinline__ int mp_pitches(const float* __restrict__ row, int lane, const MpParams& p, double* __restrict__ est, int before, bool* bad) {
  MpCell cell;
  const unsigned long long m = mp_mask<K>(row, lane, p, &cell, bad);
  if (cell.peak) est[before + mp_rank(m, lane)] = mp_pitch(64 * K + lane, cell);
  return before + __popcll(m);
}

__device__ __forceinline__ bool mp_hits(double ref, double est, const MpScoreParams& sp) {
  const double d = 100.0 * fabs(ref - est);
  return sp.strict ? d < sp.pitch_tolerance_cents : d <= sp.pitch_tolerance_cents;
}

template <int kSweepWaves>
__global__ __launch_bounds__(64 * kSweepWaves) void mp_sweep_kernel(const float* __restrict__ contour, const MpParams* __restrict__ sets,
                                                                    const MpDecode* __restrict__ dec, const MpRef* __restrict__ all_refs,
                                                                    MpScoreParams sp, int64_t n, int64_t* __restrict__ out) {
  __shared__ double s_est[kSweepWaves][kMaxPeaks];
  __shared__ unsigned long long s_part[kSweepWaves][5];
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MpDecode d = dec[c];
  const MpParams p = sets[d.set];
  int64_t* score = out + 5 * c;
  int32_t* status_out = reinterpret_cast<int32_t*>(out + 5 * n) + c;
  if (d.n_ref > kNoteScoreMaxNotes) {
    if (tid == 0) score[0] = d.rows, score[1] = 0, score[2] = 0, score[3] = 0, score[4] = 0, *status_out = 3;
    return;
  }
  const MpRef* refs = all_refs + d.ref_first;
  const int nr = d.n_ref;
  double* est = s_est[wave];
  unsigned long long sum_ref = 0, sum_est = 0, sum_tp = 0, sum_sub = 0, any_bad = 0;
  for (int64_t fr = wave; fr < d.rows; fr += kSweepWaves) {
    const float* row = contour + (d.first + fr) * kMpBins;
    bool bad = false;
    int n_est = mp_pitches<0>(row, lane, p, est, 0, &bad);
    n_est = mp_pitches<1>(row, lane, p, est, n_est, &bad);
    n_est = mp_pitches<2>(row, lane, p, est, n_est, &bad);
    n_est = mp_pitches<3>(row, lane, p, est, n_est, &bad);
    n_est = mp_pitches<4>(row, lane, p, est, n_est, &bad);
    any_bad |= __ballot(bad);
    __builtin_amdgcn_wave_barrier();  // (the compiler keeps the reads of est below behind the writes above)
    const int frame = (int)fr;        // (rows fit 32 bits: BP_SWEEP_MAX_ROWS)
    int n_ref = 0, tp = 0, next = 0;
    for (int base = 0; base < nr; base += 64) {
      const int j = base + lane;
      bool sounds = false;
      if (j < nr) {
        const MpRef r = refs[j];
        sounds = r.f0 <= frame && frame < r.f1;
      }
      unsigned long long m = __ballot(sounds);
      n_ref += __popcll(m);
      while (m != 0 && next < n_est) {
        const double ref_pitch = refs[base + __builtin_ctzll(m)].pitch;
        m &= m - 1;
        while (next < n_est && est[next] < ref_pitch && !mp_hits(ref_pitch, est[next], sp)) ++next;
        if (next < n_est && mp_hits(ref_pitch, est[next], sp)) ++tp, ++next;
      }
    }
    __builtin_amdgcn_wave_barrier();  // est is read: the next frame may write it
    sum_ref += (unsigned)n_ref, sum_est += (unsigned)n_est, sum_tp += (unsigned)tp;
    sum_sub += (unsigned)((n_ref < n_est ? n_ref : n_est) - tp);
  }
  if (lane == 0)
    s_part[wave][0] = sum_ref, s_part[wave][1] = sum_est, s_part[wave][2] = sum_tp, s_part[wave][3] = sum_sub, s_part[wave][4] = any_bad;
  __syncthreads();
  if (tid != 0) return;
  unsigned long long v[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int w = 0; w < kSweepWaves; ++w)
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] += s_part[w][k];
  const bool ok = v[4] == 0;
  score[0] = d.rows, score[1] = ok ? (int64_t)v[0] : 0, score[2] = ok ? (int64_t)v[1] : 0, score[3] = ok ? (int64_t)v[2] : 0;
  score[4] = ok ? (int64_t)v[3] : 0, *status_out = ok ? 0 : 1;
}

}  // namespace

hipError_t launch_mp_count(const float* contour, const int64_t* offs, int64_t n_segs, int64_t T, MpParams p, int2* row_info,
                           int32_t* seg_bad, hipStream_t s) {
  if (T <= 0 || n_segs <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)((T + kRowsPerBlock - 1) / kRowsPerBlock);
  hipLaunchKernelGGL(mp_count_kernel, dim3(blocks), dim3(kWidth), 0, s, contour, offs, n_segs, T, p, row_info, seg_bad);
  return hipGetLastError();
}

hipError_t launch_mp_scan(const int2* row_info, const int32_t* seg_bad, const int64_t* offs, int64_t n_segs, int64_t T,
                          int64_t* row_first, int64_t* meta, hipStream_t s) {
  if (T <= 0 || n_segs <= 0) return hipSuccess;
  hipLaunchKernelGGL(mp_scan_kernel, dim3(1), dim3(kMpScanTile), 0, s, row_info, seg_bad, T, row_first);
  hipLaunchKernelGGL(mp_offsets_kernel, dim3((unsigned)((n_segs + 1 + kWidth - 1) / kWidth)), dim3(kWidth), 0, s, offs, row_first, seg_bad,
                     n_segs, meta);
  return hipGetLastError();
}

hipError_t launch_mp_write(const float* contour, int64_t T, MpParams p, const int2* row_info, const int32_t* seg_bad,
                           const int64_t* offs, const int64_t* row_first, void* points, hipStream_t s) {
  if (T <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)((T + kRowsPerBlock - 1) / kRowsPerBlock);
  hipLaunchKernelGGL(mp_write_kernel, dim3(blocks), dim3(kWidth), 0, s, contour, T, p, row_info, seg_bad, offs, row_first,
                     static_cast<MpPoint*>(points));
  return hipGetLastError();
}

hipError_t launch_mp_sweep_frames(const float* contour, const MpParams* sets, const MpDecode* dec, const MpRef* refs,
                                  MpScoreParams sp, int64_t n_decodes, int64_t max_rows, int64_t* out, hipStream_t s) {
  if (n_decodes <= 0) return hipSuccess;
  if (max_rows > kMpSweepLongRows)
    hipLaunchKernelGGL(mp_sweep_kernel<16>, dim3((unsigned)n_decodes), dim3(1024), 0, s, contour, sets, dec, refs, sp, n_decodes, out);
  else
    hipLaunchKernelGGL(mp_sweep_kernel<4>, dim3((unsigned)n_decodes), dim3(256), 0, s, contour, sets, dec, refs, sp, n_decodes, out);
  return hipGetLastError();
}

}  // namespace bp
