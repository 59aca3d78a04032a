// The dense half of note decoding on the device (round 5; SURVEY.md §8f rank 1: "HIP for the dense parts: onset inference,
// peak picking, thresholding").  The posteriorgrams of a track are already in HBM when the CNN is done; what the host's
// note tracker (csrc/note_decode.cpp, the sequential half) needs of them is
//   * the note map (T x 88 float32) — it follows energies along a pitch and averages amplitudes,
//   * WHERE the onset peaks are: a bitmap (T x 12 bytes: 88 bits per frame), not the onset map,
//   * the pitch bend of bin f at frame t: T x 88 int8, not the 264-bin contour map,
// 7.0 MB per 3-minute track instead of 27.6 MB over PCIe — written into page-locked host memory by the kernels
// themselves when the caller's buffers are (no copy engine: the engine is busy bringing the next file in) —, and the
// three dense scans leave the host cores.
//
// Reference lines (spotify/basic-pitch v0.4.0, basic_pitch/note_creation.py):
//   constrain_frequency   314-343   bins outside [min, max] zeroed in the note and onset maps
//   get_infered_onsets    289-311   onsets = max(onsets, max(onsets) * fd / max(fd)), fd = max(0, min_n (frames[t] - frames[t - n])), n = 1, 2
//   output_to_notes_polyphonic 394-402   scipy.signal.argrelmax along time (strictly above both neighbours), >= onset_thresh
//   get_pitch_bends       182-219   argmax over the 51-bin Gaussian-weighted window of the contour row, minus the centre
// The arithmetic is the host decoder's, operation for operation (float64 differences and quotient, IEEE division; float64
// products for the bend's argmax with the host's Gaussian table): the same bits, the same events —
// tests/test_gpu_parity.py::test_device_note_candidates_give_the_host_decoders_events.
#include "bp_kernels.h"

namespace bp {

constexpr int kNdF = 88, kNdFC = 264;
constexpr int kNdBitsRow = 12;  // bytes per frame of the onset-peak bitmap: 88 bits + 8 zero bits (rows of whole dwords)

struct NdStats {
  int max_on_ord;                  // f2ord(max onset)
  int nan;                         // a NaN in the note or onset map: the host decides (numpy's propagation rules)
  unsigned long long max_fd_bits;  // bits of max fd (a non-negative double: its bits order like the value)
};

__global__ __launch_bounds__(256) void nd_constrain_kernel(float* __restrict__ note, float* __restrict__ onset, int64_t n_cells,
                                                           int lo, int hi) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_cells) return;
  const int f = (int)(i % kNdF);
  if (f < lo || f >= hi) note[i] = onset[i] = 0.0f;
}

// the same into copies (a sweep's sets share the source rows); a null destination is skipped
__global__ __launch_bounds__(256) void nd_constrain_copy_kernel(const float* __restrict__ note, const float* __restrict__ onset,
                                                                float* __restrict__ note_dst, float* __restrict__ onset_dst,
                                                                int64_t n_cells, int lo, int hi) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_cells) return;
  const int f = (int)(i % kNdF);
  const bool keep = f >= lo && f < hi;
  if (note_dst) note_dst[i] = keep ? note[i] : 0.0f;
  if (onset_dst) onset_dst[i] = keep ? onset[i] : 0.0f;
}

// the initial values of a record: maxima that any row exceeds or equals, no NaN seen
__device__ __forceinline__ void nd_stats_reset(NdStats* st) {
  st->max_on_ord = f2ord(-__int_as_float(0x7f800000));
  st->nan = 0;
  st->max_fd_bits = 0ull;
}

__global__ __launch_bounds__(64) void nd_stats_init_kernel(NdStats* st) {
  if (threadIdx.x == 0) nd_stats_reset(st);
}

// The extrema of one row join the lane's (lanes take bins lane and lane + 64).  with_fd: the row has two predecessors in its
// track, rows t - 1 and t - 2 of the same maps.  kRing: the maps are a ring of `cap` rows, absolute row t at slot t % cap
// (a stream's retained rows, below); linear: row t at t, cap unused.  One body: the arithmetic of the forms cannot drift apart.
template <bool kRing>
__device__ __forceinline__ void nd_row(const float* __restrict__ note, const float* __restrict__ onset, int64_t t, int64_t cap,
                                       bool with_fd, int lane, float& mo, double& mfd, int& nan) {
  const int64_t s0 = kRing ? t % cap : t;
  const int64_t s1 = !kRing || s0 >= 1 ? s0 - 1 : s0 - 1 + cap, s2 = !kRing || s0 >= 2 ? s0 - 2 : s0 - 2 + cap;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int f = lane + 64 * h;
    if (f >= kNdF) break;
    const float o = onset[s0 * kNdF + f], n0 = note[s0 * kNdF + f];
    nan |= (o != o) | (n0 != n0);
    mo = o > mo ? o : mo;
    if (with_fd) {
      const double d1 = (double)n0 - (double)note[s1 * kNdF + f], d2 = (double)n0 - (double)note[s2 * kNdF + f];
      const double d = d1 < d2 ? d1 : d2;
      mfd = d > mfd ? d : mfd;
    }
  }
}

// the workgroup's extrema in thread 0: wave shuffles, then the four waves through LDS
__device__ __forceinline__ void nd_reduce(float& mo, double& mfd, int& nan) {
  __shared__ float s_mo[4];
  __shared__ double s_fd[4];
  __shared__ int s_nan[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float a = __shfl_xor(mo, o);
    mo = a > mo ? a : mo;
    const double b = __shfl_xor(mfd, o);
    mfd = b > mfd ? b : mfd;
    nan |= __shfl_xor(nan, o);
  }
  if (lane == 0) s_mo[wave] = mo, s_fd[wave] = mfd, s_nan[wave] = nan;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w) {
      mo = s_mo[w] > mo ? s_mo[w] : mo;
      mfd = s_fd[w] > mfd ? s_fd[w] : mfd;
      nan |= s_nan[w];
    }
}

// thread 0's extrema join a record that other workgroups join too: ONE atomic per quantity and workgroup (as first written,
// every frame's wave published its own: 15 k serialised atomics per 3-minute track on three addresses, 0.36 ms — more than
// the CQT of the track)
__device__ __forceinline__ void nd_publish(NdStats* __restrict__ st, float mo, double mfd, int nan) {
  atomicMax(&st->max_on_ord, f2ord(mo));
  if (mfd > 0.0) atomicMax(&st->max_fd_bits, (unsigned long long)__double_as_longlong(mfd));
  if (nan) atomicOr(&st->nan, 1);
}

// Extrema of the two maps: a wave walks frames, a workgroup folds its four waves and publishes.
// The range form: frames [t0, T) JOIN the record (maxima and the NaN flag only ever grow), the differences of a frame reach
// back to frames t - 1 and t - 2 of the same maps whether or not those lie in the range — a record that has seen [0, a) and
// then [a, b) equals one that has seen [0, b), which is what lets a stream carry it over its final rows.
__global__ __launch_bounds__(256) void nd_stats_kernel(const float* __restrict__ note, const float* __restrict__ onset, int64_t t0,
                                                       int64_t T, int infer, NdStats* __restrict__ st) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float mo = -__int_as_float(0x7f800000);
  double mfd = 0.0;
  int nan = 0;
  for (int64_t t = t0 + (int64_t)blockIdx.x * 4 + wave; t < T; t += (int64_t)gridDim.x * 4)
    nd_row<false>(note, onset, t, 0, infer && t >= 2, lane, mo, mfd, nan);
  nd_reduce(mo, mfd, nan);
  if (threadIdx.x == 0) nd_publish(st, mo, mfd, nan);
}

// np.maximum: NaN if either operand is NaN
__device__ __forceinline__ double nd_np_maximum(double a, double b) {
  if (a != a || b != b) return __longlong_as_double(0x7ff8000000000000ll);
  return a > b ? a : b;
}

// The bitmap words of frame t of a track of n frames, decoded AS A WHOLE TRACK: the `t < 2` and `1 <= t <= n - 2` cases count
// from the track's first frame.  s0: the row of frame t in the maps.  kRing (a stream's rolling horizon, stream_api.hip): the
// maps are a ring of `cap` rows and s0 = (a + t) % cap for the slice that starts at absolute row a, whatever rows a - 1 and
// a - 2 still hold in the ring.  Linear: s0 = t of maps whose row 0 is the track's first frame — a whole buffer, or ONE clip
// of a buffer of many (the segmented form below); cap unused.  One body: the arithmetic of the three forms cannot drift apart.
template <bool kRing>
__device__ __forceinline__ void nd_candidates_row(const float* __restrict__ note, const float* __restrict__ onset, int64_t t,
                                                  int64_t n, int64_t s0, int64_t cap, int infer, double onset_thresh,
                                                  const NdStats* __restrict__ st, uint32_t* __restrict__ bits, int lane) {
  const double max_on_d = (double)ord2f(st->max_on_ord);
  const double max_fd = __longlong_as_double((long long)st->max_fd_bits);
  // the row of frame t + k in the maps (k = -3 ... 1; cap > 3)
  auto row = [&](int k) -> int64_t {
    const int64_t r = s0 + k;
    if (!kRing) return r;
    return r < 0 ? r + cap : (r >= cap ? r - cap : r);
  };
  auto fd_at = [&](int k, int f) -> double {
    if (t + k < 2) return 0.0;
    const double n0 = (double)note[row(k) * kNdF + f];
    const double d1 = n0 - (double)note[row(k - 1) * kNdF + f], d2 = n0 - (double)note[row(k - 2) * kNdF + f];
    const double d = d1 < d2 ? d1 : d2;
    return d < 0 ? 0.0 : d;
  };
  auto on_at = [&](int k, int f) -> double {
    const double o = (double)onset[row(k) * kNdF + f];
    if (!infer) return o;
    const double scaled = (max_on_d * fd_at(k, f)) / max_fd;  // 0 / 0 -> NaN when nothing rises, like numpy
    return nd_np_maximum(o, scaled);
  };
  bool c[2] = {false, false};
  if (t >= 1 && t <= n - 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int f = lane + 64 * h;
      if (f >= kNdF) break;
      const double v = on_at(0, f);
      c[h] = v > on_at(-1, f) && v > on_at(1, f) && v >= onset_thresh;
    }
  }
  const unsigned long long b0 = __ballot(c[0]), b1 = __ballot(c[1]);
  if (lane < 3) bits[t * 3 + lane] = lane == 0 ? (uint32_t)b0 : (lane == 1 ? (uint32_t)(b0 >> 32) : (uint32_t)b1);
}

// A wave per frame.  kRing: the bitmap is that of rows [a, T) of the ring; linear: a = 0, cap unused.  Only the linear form is
// launched (a track): the rows of rings go through nd_streams_candidates_kernel.
template <bool kRing>
__global__ __launch_bounds__(256) void nd_candidates_kernel(const float* __restrict__ note, const float* __restrict__ onset,
                                                            int64_t a, int64_t T, int64_t cap, int infer, double onset_thresh,
                                                            const NdStats* __restrict__ st, uint32_t* __restrict__ bits) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n = T - a;  // t: the frame of the slice
  if (t >= n) return;
  nd_candidates_row<kRing>(note, onset, t, n, kRing ? (a + t) % cap : t, cap, infer, onset_thresh, st, bits, threadIdx.x & 63);
}

// ---- many clips in one buffer (bp_infer_clips_candidates, clips_api.hip) -------------------------------------------------------
// The maps of n_clips clips lie one after the other: clip c owns rows [offs[c], offs[c + 1]) and is decoded as its own whole
// track.  The table offs[0 ... n_clips] is in device memory; a row finds its clip by binary search.  Every clip has one stats
// record, table[c].  Frequency limits and bends are row-local and run over all rows with the kernels of a single track.

// the clip that owns row r < offs[n]: the last c with offs[c] <= r (clips without rows own none)
__device__ __forceinline__ int64_t nd_clip_of_row(const int64_t* __restrict__ offs, int64_t n, int64_t r) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (offs[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void nd_clips_stats_init_kernel(NdStats* __restrict__ table, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  nd_stats_reset(table + c);
}

// Extrema per clip.  A workgroup takes kNdClipRows consecutive rows and, for every clip that owns some of them, folds those
// rows (a wave per row, nd_row with the difference term only from the clip's third row on: rows 0 and 1 of a clip never read
// the rows before them, which are another clip's) and publishes: one atomic per quantity, workgroup and clip touched.
constexpr int kNdClipRows = 64;
__global__ __launch_bounds__(256) void nd_clips_stats_kernel(const float* __restrict__ note, const float* __restrict__ onset,
                                                             const int64_t* __restrict__ offs, int64_t n_clips, int infer,
                                                             NdStats* __restrict__ table) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t total = offs[n_clips], r0 = (int64_t)blockIdx.x * kNdClipRows;
  const int64_t r1 = r0 + kNdClipRows < total ? r0 + kNdClipRows : total;
  for (int64_t c = nd_clip_of_row(offs, n_clips, r0); c < n_clips && offs[c] < r1; ++c) {  // block-uniform
    const int64_t first = offs[c], lo = first > r0 ? first : r0, hi = offs[c + 1] < r1 ? offs[c + 1] : r1;
    if (hi <= lo) continue;
    float mo = -__int_as_float(0x7f800000);
    double mfd = 0.0;
    int nan = 0;
    for (int64_t t = lo + wave; t < hi; t += 4) nd_row<false>(note, onset, t, 0, infer && t - first >= 2, lane, mo, mfd, nan);
    nd_reduce(mo, mfd, nan);
    if (threadIdx.x == 0) nd_publish(table + c, mo, mfd, nan);
    __syncthreads();  // thread 0 has read the waves' words before the next clip's are written
  }
}

// The bitmap: a wave per row of the buffer, the frame counted from its clip's first row, the clip's own length and record.  A
// clip whose record has the NaN flag gets a zero bitmap (the caller decodes its maps on the host: status 1).
__global__ __launch_bounds__(256) void nd_clips_candidates_kernel(const float* __restrict__ note, const float* __restrict__ onset,
                                                                  const int64_t* __restrict__ offs, int64_t n_clips, int infer,
                                                                  double onset_thresh, const NdStats* __restrict__ table,
                                                                  uint32_t* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= offs[n_clips]) return;
  const int64_t c = nd_clip_of_row(offs, n_clips, r), first = offs[c], t = r - first;
  if (table[c].nan) {  // wave-uniform
    if (lane < 3) bits[r * 3 + lane] = 0u;
    return;
  }
  nd_candidates_row<false>(note + first * kNdF, onset + first * kNdF, t, offs[c + 1] - first, t, 0, infer, onset_thresh, table + c,
                           bits + first * 3, lane);
}

// Pitch bends.  A workgroup takes kNdBendFrames consecutive frames: their contour rows go to LDS as float64 once (264
// conversions per frame instead of 88 x 51), each between two margins of -inf, so that every bin's window is the full 51
// taps — a tap outside the row yields -inf x gauss = -inf, which never exceeds the running maximum and never comes
// first (the running index starts at the first tap inside the row, where the host's loop starts).  An item is (frame,
// bin): 16 x 88 = 1408 items over 256 threads, consecutive lanes consecutive bins (3 doubles apart: conflict-free
// ds_read_b64), the Gaussian in registers, four vector operations per tap (multiply, compare, maximum, select) where the
// wave-per-frame form with table-driven loop bounds issued twelve at 69 % lane use: 72 -> ~20 us per 3-minute track.
// The products and comparisons are the host loop's float64 operations in the host loop's order: the same argmax.  A NaN
// anywhere in the block's rows (np.argmax: the first NaN wins) sends the block through the comparison that handles it.
constexpr int kNdBendFrames = 16, kNdBendPad = 26, kNdBendPitch = kNdFC + 2 * kNdBendPad;  // rows 16-byte aligned
static_assert(kNdBendPad >= 25 && (kNdBendPad * 8) % 16 == 0 && (kNdBendPitch * 8) % 16 == 0, "aligned rows");

__device__ __forceinline__ int nd_bend_argmax(const double* __restrict__ win, const double (&g)[26], int first) {
  int best = first;
  double bestv = -__longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
  for (int j = 0; j < 51; ++j) {
    const double v = win[j] * g[j <= 25 ? j : 50 - j];
    best = v > bestv ? j : best;
    bestv = __builtin_fmax(bestv, v);
  }
  return best;
}

// np.argmax over the taps [first, 50] with a NaN somewhere in the block: the first maximum, the first NaN wins (the margins
// behind the row are -inf and never win).  A rolled loop with the Gaussian from LDS: this path is for broken inputs.
__device__ __forceinline__ int nd_bend_argmax_nan(const double* __restrict__ win, const double* __restrict__ g, int first) {
  int best = first;
  double bestv = win[first] * g[first];
#pragma unroll 1
  for (int j = first + 1; j < 51; ++j) {
    const double v = win[j] * g[j];
    const bool take = (v > bestv) | ((v != v) & (bestv == bestv));
    bestv = take ? v : bestv;
    best = take ? j : best;
  }
  return best;
}

// kRing: row t of the T rows is absolute row first + t of a ring of `cap` contour rows (slot r % cap); the bends are written
// linear, row t at bend + t * 88, as in the linear form (first = 0, cap unused).
// `block`: which kNdBendFrames rows of the T the workgroup takes.  A device function: the kernel of a track (linear) and the
// kernel of the streams' rings (nd_streams_bend_kernel, below) run this one body.
template <bool kRing>
__device__ __forceinline__ void nd_bend_block(const float* __restrict__ contour, int64_t first, int64_t T, int64_t cap,
                                              const int4* __restrict__ tab, const double* __restrict__ gauss,
                                              int8_t* __restrict__ bend, int64_t block) {
  __shared__ __attribute__((aligned(16))) double s_row[kNdBendFrames * kNdBendPitch];
  __shared__ int s_start[kNdF], s_first[kNdF];
  __shared__ double s_g[51];
  __shared__ int s_nan;
  const int tid = threadIdx.x;
  const int64_t t0 = block * kNdBendFrames;
  const double ninf = -__longlong_as_double(0x7ff0000000000000ll);
  if (tid == 0) s_nan = 0;
  if (tid >= 128 && tid < 128 + 51) s_g[tid - 128] = gauss[tid - 128];
  if (tid < kNdF) {
    const int4 w = tab[tid];  // f0, n, g0, shift: tap j of the 51 reads row bin f0 - g0 + j; the first inside the row is g0
    s_start[tid] = kNdBendPad + w.x - w.z;
    s_first[tid] = w.z;
  }
  for (int i = tid; i < kNdBendFrames * 2 * kNdBendPad; i += 256) {
    const int r = i / (2 * kNdBendPad), c = i - r * (2 * kNdBendPad);
    s_row[r * kNdBendPitch + (c < kNdBendPad ? c : kNdFC + c)] = ninf;
  }
  // the Gaussian exp(-(j - 25)^2 / 50) is symmetric bit for bit (the host squares j - 25): 26 values, in vector registers
  // (left to itself the compiler keeps the words in scalar registers it does not have)
  double g[26];
#pragma unroll
  for (int j = 0; j < 26; ++j) {
    g[j] = gauss[j];
    asm volatile("" : "+v"(g[j]));
  }
  __syncthreads();
  // the block's rows are contiguous in memory: 16 x 264 floats as float4s (264 = 4 x 66: no float4 straddles two rows)
  int nan = 0;
  const int64_t n_rows = T - t0 < kNdBendFrames ? T - t0 : kNdBendFrames;
  const float4* src = reinterpret_cast<const float4*>(contour + (kRing ? 0 : t0 * kNdFC));
  for (int e = tid; e < kNdBendFrames * (kNdFC / 4); e += 256) {
    const int r = e / (kNdFC / 4), c4 = e - r * (kNdFC / 4);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r < n_rows) v = kRing ? src[((first + t0 + r) % cap) * (kNdFC / 4) + c4] : src[e];
    nan |= (v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w);
    double* d = &s_row[r * kNdBendPitch + kNdBendPad + 4 * c4];
    *reinterpret_cast<double2*>(d) = double2{(double)v.x, (double)v.y};
    *reinterpret_cast<double2*>(d + 2) = double2{(double)v.z, (double)v.w};
  }
  if (nan) s_nan = 1;
  __syncthreads();
  if (s_nan == 0) {  // block-uniform
#pragma unroll 1
    for (int item = tid; item < kNdBendFrames * kNdF; item += 256) {
      const int r = item / kNdF, b = item - r * kNdF;
      if (r >= n_rows) break;
      const int best = nd_bend_argmax(&s_row[r * kNdBendPitch + s_start[b]], g, s_first[b]);
      bend[t0 * kNdF + item] = (int8_t)(best - 25);  // = (best - g0) - shift, shift = 25 - g0
    }
  } else {
#pragma unroll 1
    for (int item = tid; item < kNdBendFrames * kNdF; item += 256) {
      const int r = item / kNdF, b = item - r * kNdF;
      if (r >= n_rows) break;
      const int best = nd_bend_argmax_nan(&s_row[r * kNdBendPitch + s_start[b]], s_g, s_first[b]);
      bend[t0 * kNdF + item] = (int8_t)(best - 25);
    }
  }
}

template <bool kRing>
__global__ __launch_bounds__(256, 3) void nd_bend_kernel(const float* __restrict__ contour, int64_t first, int64_t T, int64_t cap,
                                                      const int4* __restrict__ tab, const double* __restrict__ gauss,
                                                      int8_t* __restrict__ bend) {
  nd_bend_block<kRing>(contour, first, T, cap, tab, gauss, bend, (int64_t)blockIdx.x);
}

// device -> page-locked host memory, by the compute queue: the note map, the bitmap and the bend map of a track in one
// launch (4-byte words, a wave writes 256 contiguous bytes; the copy engine stays free for the next file's samples), the
// stats record with them — and the device record back to its initial values for the next track (one launch and one
// 16-byte copy fewer per track).  n_st records: one for a track, one per clip of a buffer of many.
__global__ __launch_bounds__(256) void nd_export_kernel(const uint32_t* __restrict__ s0, uint32_t* __restrict__ d0, int64_t n0,
                                                        const uint32_t* __restrict__ s1, uint32_t* __restrict__ d1, int64_t n1,
                                                        const uint32_t* __restrict__ s2, uint32_t* __restrict__ d2, int64_t n2,
                                                        NdStats* __restrict__ st, NdStats* __restrict__ st_dst, int64_t n_st) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n0; i += step) d0[i] = s0[i];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n1; i += step) d1[i] = s1[i];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += step) d2[i] = s2[i];
  if (blockIdx.x == 0)
    for (int64_t c = threadIdx.x; c < n_st; c += 256) {
      st_dst[c] = st[c];
      st[c].max_on_ord = f2ord(-__int_as_float(0x7f800000));
      st[c].nan = 0;
      st[c].max_fd_bits = 0ull;
    }
}

// Frames [t0, t1) of the device maps note / onset join the stats record.  Frames t0 - 1 and t0 - 2 are read when t0 > 0.
void launch_note_fold(const float* note, const float* onset, int64_t t0, int64_t t1, int infer, void* stats, hipStream_t s) {
  if (t1 <= t0) return;
  const unsigned frames4 = (unsigned)((t1 - t0 + 3) / 4);
  hipLaunchKernelGGL(nd_stats_kernel, dim3(frames4 < 512u ? frames4 : 512u), dim3(256), 0, s, note, onset, t0, t1, infer,
                     static_cast<NdStats*>(stats));
}

// note / onset / contour: device maps of T frames.  constrain_frequency on them (`lo`, `hi`: the bins it keeps; 0, 88: none to
// zero), their extrema into `stats` (which must hold its initial values: launch_note_stats_init), the onset-peak bitmap of
// all T frames ([T][12] bytes) and, when `bend` != null, the bend map ([T][88] bytes; a row's bends depend on that row alone).
// All three results stay on the device.
void launch_note_candidates(float* note, float* onset, const float* contour, int64_t T, int lo, int hi, int infer,
                            double onset_thresh, const void* tab, const double* gauss, void* stats, uint8_t* bits,
                            int8_t* bend, hipStream_t s) {
  if (T <= 0) return;
  if (lo > 0 || hi < kNdF)
    hipLaunchKernelGGL(nd_constrain_kernel, dim3((unsigned)((T * kNdF + 255) / 256)), dim3(256), 0, s, note, onset, T * kNdF, lo, hi);
  launch_note_fold(note, onset, 0, T, infer, stats, s);
  hipLaunchKernelGGL(nd_candidates_kernel<false>, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, note, onset, (int64_t)0, T,
                     (int64_t)0, infer, onset_thresh, static_cast<const NdStats*>(stats), reinterpret_cast<uint32_t*>(bits));
  if (bend)
    hipLaunchKernelGGL(nd_bend_kernel<false>, dim3((unsigned)((T + kNdBendFrames - 1) / kNdBendFrames)), dim3(256), 0, s, contour,
                       (int64_t)0, T, (int64_t)0, static_cast<const int4*>(tab), gauss, bend);
}

void launch_note_stats_init(void* stats, hipStream_t s) {
  hipLaunchKernelGGL(nd_stats_init_kernel, dim3(1), dim3(64), 0, s, static_cast<NdStats*>(stats));
}

// the three results to device-visible host pointers (sizes in bytes, multiples of 4; a null destination is skipped), and
// the n_stats records at `stats`, which are left holding their initial values
void launch_note_export(const void* note, void* note_dst, int64_t note_bytes, const void* bits, void* bits_dst,
                        int64_t bits_bytes, const void* bend, void* bend_dst, int64_t bend_bytes, void* stats,
                        void* stats_dst, int64_t n_stats, hipStream_t s) {
  hipLaunchKernelGGL(nd_export_kernel, dim3(64), dim3(256), 0, s, static_cast<const uint32_t*>(note),
                     static_cast<uint32_t*>(note_dst), note_dst ? note_bytes / 4 : 0, static_cast<const uint32_t*>(bits),
                     static_cast<uint32_t*>(bits_dst), bits_dst ? bits_bytes / 4 : 0, static_cast<const uint32_t*>(bend),
                     static_cast<uint32_t*>(bend_dst), bend_dst ? bend_bytes / 4 : 0, static_cast<NdStats*>(stats),
                     static_cast<NdStats*>(stats_dst), n_stats);
}

void launch_constrain_copy(const float* note, const float* onset, float* note_dst, float* onset_dst, int64_t n_rows, int lo,
                           int hi, hipStream_t s) {
  if (n_rows <= 0 || (!note_dst && !onset_dst)) return;
  hipLaunchKernelGGL(nd_constrain_copy_kernel, dim3((unsigned)((n_rows * kNdF + 255) / 256)), dim3(256), 0, s, note, onset, note_dst,
                     onset_dst, n_rows * kNdF, lo, hi);
}

void launch_clips_stats_init(void* table, int64_t n_clips, hipStream_t s) {
  if (n_clips <= 0) return;
  hipLaunchKernelGGL(nd_clips_stats_init_kernel, dim3((unsigned)((n_clips + 255) / 256)), dim3(256), 0, s,
                     static_cast<NdStats*>(table), n_clips);
}

// note / onset / contour: the device maps of n_clips clips, total_rows > 0 rows in all, clip c at rows [offs[c], offs[c + 1]) (offs:
// device memory).  What launch_note_candidates does for one track, for every clip as its own track: `table` (n_clips records
// holding their initial values) receives the clips' extrema.
void launch_clips_candidates(float* note, float* onset, const float* contour, const int64_t* offs, int64_t n_clips,
                             int64_t total_rows, int lo, int hi, int infer, double onset_thresh, const void* tab,
                             const double* gauss, void* table, uint8_t* bits, int8_t* bend, hipStream_t s) {
  if (total_rows <= 0 || n_clips <= 0) return;
  if (lo > 0 || hi < kNdF)
    hipLaunchKernelGGL(nd_constrain_kernel, dim3((unsigned)((total_rows * kNdF + 255) / 256)), dim3(256), 0, s, note, onset,
                       total_rows * kNdF, lo, hi);
  hipLaunchKernelGGL(nd_clips_stats_kernel, dim3((unsigned)((total_rows + kNdClipRows - 1) / kNdClipRows)), dim3(256), 0, s, note,
                     onset, offs, n_clips, infer, static_cast<NdStats*>(table));
  hipLaunchKernelGGL(nd_clips_candidates_kernel, dim3((unsigned)((total_rows + 3) / 4)), dim3(256), 0, s, note, onset, offs, n_clips,
                     infer, onset_thresh, static_cast<const NdStats*>(table), reinterpret_cast<uint32_t*>(bits));
  // a row's bends depend on that row alone (a NaN elsewhere in a block of 16 rows only chooses between two loops that give a
  // row without NaN the same first maximum): the kernel of a single track, its blocks free to straddle clips
  if (bend)
    hipLaunchKernelGGL(nd_bend_kernel<false>, dim3((unsigned)((total_rows + kNdBendFrames - 1) / kNdBendFrames)), dim3(256), 0, s,
                       contour, (int64_t)0, total_rows, (int64_t)0, static_cast<const int4*>(tab), gauss, bend);
}

// ---- the rows a stream retains (stream_api.hip, bp_stream_keep / bp_stream_keep_rolling) ------------------------------------
// The retained maps are a ring of `cap` rows ([cap] note, [cap] onset, [cap] contour; absolute row r at slot r % cap),
// frequency-constrained as they are put, and a transcript decodes rows [a, T) as a whole track ("the updates of streams",
// below).  This part is how rows enter the store and how the extrema of the final rows are carried.  A stream that keeps
// every row reserves a ring that never wraps: a = 0, slot r is row r, and the extrema of its rows are carried in ONE record,
// which the final rows join with launch_note_fold on the ring as the linear maps it then is.
//
// A rolling horizon cannot carry the two maxima of its slice in one record: a record only grows, and a row that leaves the
// horizon cannot be taken out of it.  So its final rows fill a TABLE of records, one
// per block of kNdRingBlock absolute rows (block b at table slot b % n_tab; fd from the real predecessors), and an update
// joins the blocks that lie wholly in [a + 2, R) (R: the final rows) and scans the rest — the partial first block with rows a
// and a + 1, whose fd is zero by the decoder's t >= 2 rule, the partial last block and the tail — directly.  Maxima and an
// OR are exact: the joined record is nd_stats_kernel's on the linear slice whatever the order.
constexpr int kNdRingBlock = 64;

// Rows [t0, t0 + n) of linear maps (row 0 of src_* is absolute row t0) go to their slots, constrain_frequency applied on the
// way (bins outside [lo, hi) of note and onset become 0).  An item is one float, float c of row r of the source; n <= cap, so no
// slot is written twice.  Scalar loads: the source may be a caller's device buffer, of which only float alignment is known.
// A device function: the kernel of a step's final rows and the kernel of the tails of an update run this one body.
constexpr int kNdPutRow = 2 * kNdF + kNdFC;
__device__ __forceinline__ void nd_ring_put_item(const float* __restrict__ src_note, const float* __restrict__ src_onset,
                                                 const float* __restrict__ src_contour, float* __restrict__ note,
                                                 float* __restrict__ onset, float* __restrict__ contour, int64_t t0, int64_t cap,
                                                 int lo, int hi, int64_t r, int c) {
  const int64_t slot = (t0 + r) % cap;
  if (c < kNdF)
    note[slot * kNdF + c] = c < lo || c >= hi ? 0.0f : src_note[r * kNdF + c];
  else if (c < 2 * kNdF)
    onset[slot * kNdF + c - kNdF] = c - kNdF < lo || c - kNdF >= hi ? 0.0f : src_onset[r * kNdF + c - kNdF];
  else
    contour[slot * kNdFC + c - 2 * kNdF] = src_contour[r * kNdFC + c - 2 * kNdF];
}

__global__ __launch_bounds__(256) void nd_ring_put_kernel(const float* __restrict__ src_note, const float* __restrict__ src_onset,
                                                          const float* __restrict__ src_contour, float* __restrict__ note,
                                                          float* __restrict__ onset, float* __restrict__ contour, int64_t t0,
                                                          int64_t n, int64_t cap, int lo, int hi) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * kNdPutRow; i += step) {
    const int64_t r = i / kNdPutRow;
    nd_ring_put_item(src_note, src_onset, src_contour, note, onset, contour, t0, cap, lo, hi, r, (int)(i - r * kNdPutRow));
  }
}

// Final rows [t0, t1) join the table: workgroup i takes block t0 / kNdRingBlock + i, a wave walks its rows.  A block that
// starts at or after `fresh_from` begins anew (its table slot held a block that left the ring); the block t0 lies inside
// joins what earlier steps left.  One workgroup per block and launches of one queue: plain stores, no atomics.
__global__ __launch_bounds__(256) void nd_ring_fold_kernel(const float* __restrict__ note, const float* __restrict__ onset, int64_t t0,
                                                           int64_t t1, int64_t cap, int infer, int64_t fresh_from,
                                                           NdStats* __restrict__ table, int64_t n_tab) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = t0 / kNdRingBlock + blockIdx.x, b0 = b * kNdRingBlock;
  const int64_t lo = b0 > t0 ? b0 : t0, hi = b0 + kNdRingBlock < t1 ? b0 + kNdRingBlock : t1;
  float mo = -__int_as_float(0x7f800000);
  double mfd = 0.0;
  int nan = 0;
  for (int64_t t = lo + wave; t < hi; t += 4) nd_row<true>(note, onset, t, cap, infer && t >= 2, lane, mo, mfd, nan);
  nd_reduce(mo, mfd, nan);
  if (threadIdx.x == 0) {
    NdStats* rec = table + b % n_tab;
    int ord = f2ord(mo);
    unsigned long long fd_bits = (unsigned long long)__double_as_longlong(mfd);  // mfd >= 0: its bits order like the value
    if (b0 < fresh_from) {
      ord = rec->max_on_ord > ord ? rec->max_on_ord : ord;
      fd_bits = rec->max_fd_bits > fd_bits ? rec->max_fd_bits : fd_bits;
      nan |= rec->nan;
    }
    rec->max_on_ord = ord, rec->nan = nan, rec->max_fd_bits = fd_bits;
  }
}

// The record of the slice [a, T) (st holds the initial values): the table's blocks [e0, e1) / kNdRingBlock, which lie wholly in
// [a + 2, R), joined by workgroup 0, and the rows [a, e0) and [e1, T) scanned, a wave per row, fd only from frame 2 of the
// slice on.  Without a whole block e0 == e1 and the two ranges are the slice.  The two halves of nd_streams_stats_kernel, below.

// edge rows j0, j0 + step, ... < j1 of the n_edge = (e0 - a) + (T - e1) join the wave's extrema
__device__ __forceinline__ void nd_edge_rows(const float* __restrict__ note, const float* __restrict__ onset, int64_t a, int64_t e0,
                                             int64_t e1, int64_t cap, int infer, int64_t j0, int64_t j1, int64_t step, int lane,
                                             float& mo, double& mfd, int& nan) {
  const int64_t n_head = e0 - a;
  for (int64_t j = j0; j < j1; j += step) {
    const int64_t t = j < n_head ? a + j : e1 + (j - n_head);
    nd_row<true>(note, onset, t, cap, infer && t - a >= 2, lane, mo, mfd, nan);
  }
}

// the records of the table's blocks [e0, e1) / kNdRingBlock join the thread's extrema, a thread per block
__device__ __forceinline__ void nd_join_blocks(const NdStats* __restrict__ table, int64_t n_tab, int64_t e0, int64_t e1, float& mo,
                                               double& mfd, int& nan) {
  for (int64_t b = e0 / kNdRingBlock + threadIdx.x; b < e1 / kNdRingBlock; b += 256) {
    const NdStats rec = table[b % n_tab];
    const float o = ord2f(rec.max_on_ord);
    const double d = __longlong_as_double((long long)rec.max_fd_bits);
    mo = o > mo ? o : mo;
    mfd = d > mfd ? d : mfd;
    nan |= rec.nan;
  }
}

int64_t note_ring_records(int64_t cap) { return (cap + kNdRingBlock - 1) / kNdRingBlock + 2 + 1; }

void note_ring_edges(int64_t a, int64_t R, int64_t T, int64_t* e0, int64_t* e1) {
  *e0 = (a + 2 + kNdRingBlock - 1) / kNdRingBlock * kNdRingBlock, *e1 = R / kNdRingBlock * kNdRingBlock;
  if (*e0 >= *e1) *e0 = *e1 = T;
}

static NdStats* ring_table(void* records) { return static_cast<NdStats*>(records); }
static int64_t ring_n_tab(int64_t cap) { return note_ring_records(cap) - 1; }
static unsigned ring_grid(int64_t items) { return (unsigned)(items < 2048 * 256 ? (items + 255) / 256 : 2048); }

void launch_ring_put(const float* src_note, const float* src_onset, const float* src_contour, float* ring, int64_t cap,
                     int64_t t0, int64_t n, int lo, int hi, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(nd_ring_put_kernel, dim3(ring_grid(n * (2 * kNdF + kNdFC))), dim3(256), 0, s, src_note, src_onset,
                     src_contour, ring, ring + cap * kNdF, ring + cap * 2 * kNdF, t0, n, cap, lo, hi);
}

void launch_ring_fold(const float* ring, int64_t cap, int64_t t0, int64_t t1, int64_t fresh_from, int infer, void* records,
                      hipStream_t s) {
  if (t1 <= t0) return;
  const int64_t n_blocks = (t1 - 1) / kNdRingBlock - t0 / kNdRingBlock + 1;  // <= n_tab for t1 - t0 <= cap: no slot twice
  hipLaunchKernelGGL(nd_ring_fold_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, ring, ring + cap * kNdF, t0, t1, cap, infer,
                     fresh_from, ring_table(records), ring_n_tab(cap));
}

// ---- the updates of streams (bp_stream_candidates[_rolling], bp_streams_candidates, bp_streams_events; stream_api.hip) ---------
// An update decodes rows [a, T) of every stream's store as a whole track, for n stores at once (a single update is n = 1): the
// segmented form the clips call introduced, a segment being a stream.  Stream c is u[c]; the work items of each launch are
// counted over all streams and an item finds its stream by nd_clip_of_row in a prefix array (pre + k * (n + 1), k = one of
// the kNdPre* below).  The bodies are the device functions above, in their ring forms: nd_ring_put_item, nd_edge_rows /
// nd_join_blocks / nd_reduce / nd_publish, nd_candidates_row<true>, nd_bend_block<true>.  The update records are a table of the
// handle's, record c for stream c.
enum { kNdPreTail, kNdPreChunk, kNdPreBits, kNdPreBend, kNdPreNote, kNdPreArrays };
static_assert(kNdPreArrays == kStreamUpdatePrefixes, "the host's table has one array per launch");
constexpr int kNdEdgeChunk = 64;  // edge rows a workgroup of the stats launch scans

// the rows of all tails to their slots: a workgroup walks rows, its threads the 440 floats of one
__global__ __launch_bounds__(256) void nd_streams_put_kernel(const StreamUpdate* __restrict__ u, const int64_t* __restrict__ offs,
                                                             int64_t n) {
  const int64_t total = offs[n];
  for (int64_t r = blockIdx.x; r < total; r += gridDim.x) {  // block-uniform
    const int64_t c = nd_clip_of_row(offs, n, r), local = r - offs[c];
    const StreamUpdate& d = u[c];
    for (int col = threadIdx.x; col < kNdPutRow; col += 256)
      nd_ring_put_item(d.tail_note, d.tail_onset, d.tail_contour, d.ring, d.ring + d.cap * kNdF, d.ring + d.cap * 2 * kNdF, d.R, d.cap,
                       d.lo, d.hi, local, col);
  }
}

// record c: the initial values for a rolling stream, a copy of the record its final rows have joined for a keeping stream
__global__ __launch_bounds__(256) void nd_streams_stats_init_kernel(const StreamUpdate* __restrict__ u, int64_t n,
                                                                    NdStats* __restrict__ st) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  if (u[c].n_tab == 0 && u[c].records)
    st[c] = *static_cast<const NdStats*>(u[c].records);
  else
    nd_stats_reset(st + c);
}

// A workgroup per stream and chunk of kNdEdgeChunk edge rows; the first of a rolling stream also joins the whole blocks of
// its table.  A keeping stream's edge rows are its tail (e0 = a, e1 = R).  Maxima and an OR: the record is that of the
// slice whatever the partition.
__global__ __launch_bounds__(256) void nd_streams_stats_kernel(const StreamUpdate* __restrict__ u, const int64_t* __restrict__ offs,
                                                               int64_t n, NdStats* __restrict__ st) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c = nd_clip_of_row(offs, n, blockIdx.x), chunk = blockIdx.x - offs[c];
  const StreamUpdate& d = u[c];
  float mo = -__int_as_float(0x7f800000);
  double mfd = 0.0;
  int nan = 0;
  const int64_t n_edge = (d.e0 - d.a) + (d.T - d.e1), j0 = chunk * kNdEdgeChunk;
  nd_edge_rows(d.ring, d.ring + d.cap * kNdF, d.a, d.e0, d.e1, d.cap, d.infer, j0 + wave,
               j0 + kNdEdgeChunk < n_edge ? j0 + kNdEdgeChunk : n_edge, 4, lane, mo, mfd, nan);
  if (chunk == 0 && d.n_tab) nd_join_blocks(static_cast<const NdStats*>(d.records), d.n_tab, d.e0, d.e1, mo, mfd, nan);
  nd_reduce(mo, mfd, nan);
  if (threadIdx.x == 0) nd_publish(st + c, mo, mfd, nan);
}

// the bitmaps of all slices, packed: a wave per row, the frame counted from its stream's row a
__global__ __launch_bounds__(256) void nd_streams_candidates_kernel(const StreamUpdate* __restrict__ u,
                                                                    const int64_t* __restrict__ offs, int64_t n,
                                                                    const NdStats* __restrict__ st, uint32_t* __restrict__ bits) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= offs[n]) return;
  const int64_t c = nd_clip_of_row(offs, n, r), t = r - offs[c];
  const StreamUpdate& d = u[c];
  nd_candidates_row<true>(d.ring, d.ring + d.cap * kNdF, t, d.T - d.a, (d.a + t) % d.cap, d.cap, d.infer, d.onset_thresh, st + c,
                          bits + d.bits_offset * 3, threadIdx.x & 63);
}

// A workgroup takes kNdBendFrames rows of ONE stream, counted from its row n0: a block's NaN switch sees the same rows
// whichever streams share the step.
__global__ __launch_bounds__(256, 3) void nd_streams_bend_kernel(const StreamUpdate* __restrict__ u, const int64_t* __restrict__ offs,
                                                                 int64_t n, const int4* __restrict__ tab,
                                                                 const double* __restrict__ gauss, int8_t* __restrict__ bend) {
  const int64_t c = nd_clip_of_row(offs, n, blockIdx.x);
  const StreamUpdate& d = u[c];
  nd_bend_block<true>(d.ring + d.cap * 2 * kNdF, d.n0, d.T - d.n0, d.cap, tab, gauss, bend + d.note_offset * kNdF,
                      (int64_t)blockIdx.x - offs[c]);
}

// note rows [n0, T) of every stream from their slots to the packed buffer: 32 threads a row, 22 of them a float4 each (a row is
// 352 bytes and both bases come from the allocator: every float4 is aligned)
static_assert(kNdF % 4 == 0, "whole float4s");
__global__ __launch_bounds__(256) void nd_streams_gather_kernel(const StreamUpdate* __restrict__ u, const int64_t* __restrict__ offs,
                                                                int64_t n, float4* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int q = threadIdx.x & 31;
  if (r >= offs[n] || q >= kNdF / 4) return;
  const int64_t c = nd_clip_of_row(offs, n, r);
  const StreamUpdate& d = u[c];
  const int64_t slot = (d.n0 + (r - offs[c])) % d.cap;
  out[r * (kNdF / 4) + q] = reinterpret_cast<const float4*>(d.ring + slot * kNdF)[q];
}

void launch_streams_put(const StreamUpdate* u, const int64_t* pre, int64_t n, int64_t tail_rows, hipStream_t s) {
  if (tail_rows <= 0) return;
  hipLaunchKernelGGL(nd_streams_put_kernel, dim3((unsigned)(tail_rows < 4096 ? tail_rows : 4096)), dim3(256), 0, s, u,
                     pre + kNdPreTail * (n + 1), n);
}

int64_t streams_stats_chunks(int64_t n_edge) { return (n_edge + kNdEdgeChunk - 1) / kNdEdgeChunk; }
int64_t streams_bend_blocks(int64_t n_rows) { return (n_rows + kNdBendFrames - 1) / kNdBendFrames; }

void launch_streams_candidates(const StreamUpdate* u, const int64_t* pre, int64_t n, int64_t chunks, int64_t bits_rows,
                               int64_t bend_blocks, int64_t note_rows, const void* tab, const double* gauss, void* stats,
                               uint8_t* bits, int8_t* bend, float* note, hipStream_t s) {
  const int64_t m = n + 1;
  NdStats* st = static_cast<NdStats*>(stats);
  hipLaunchKernelGGL(nd_streams_stats_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, u, n, st);
  if (chunks > 0)
    hipLaunchKernelGGL(nd_streams_stats_kernel, dim3((unsigned)chunks), dim3(256), 0, s, u, pre + kNdPreChunk * m, n, st);
  if (bits_rows > 0)
    hipLaunchKernelGGL(nd_streams_candidates_kernel, dim3((unsigned)((bits_rows + 3) / 4)), dim3(256), 0, s, u, pre + kNdPreBits * m, n,
                       st, reinterpret_cast<uint32_t*>(bits));
  if (bend_blocks > 0)
    hipLaunchKernelGGL(nd_streams_bend_kernel, dim3((unsigned)bend_blocks), dim3(256), 0, s, u, pre + kNdPreBend * m, n,
                       static_cast<const int4*>(tab), gauss, bend);
  if (note_rows > 0)
    hipLaunchKernelGGL(nd_streams_gather_kernel, dim3((unsigned)((note_rows + 7) / 8)), dim3(256), 0, s, u, pre + kNdPreNote * m, n,
                       reinterpret_cast<float4*>(note));
}

}  // namespace bp
