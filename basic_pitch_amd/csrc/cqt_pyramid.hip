// CQT pyramid: 8 x decimate-by-2 with the 256-tap half-band FIR, plus the windowing / un-overlapping copies of the track
// calls and of the streaming steps: one gather and one scatter over window segments (bp_common.h WindowSeg).
//
// Reference behaviour (spotify/basic-pitch v0.4.0):
//   basic_pitch/layers/nnaudio.py:259-284 downsampling_by_n(match_torch_exactly=True):
//       zero-pad 127 samples each side, conv1d with the firwin2 kernel, stride 2, VALID
//   basic_pitch/layers/nnaudio.py:636-638     applied 8 times, level k+1 from level k
//   basic_pitch/inference.py:194-244          window_audio_file / get_audio_input
//   basic_pitch/inference.py:247-279          unwrap_output
//
// Roofline: 11.18 M MAC / window on the f32 VALU (2 % of the path's FLOPs); the signal tile is
// staged once in LDS and every thread produces two adjacent outputs from 65 ds_read_b128, so the
// kernel is VALU-issue bound, not LDS- or HBM-bound.  Algorithmic bytes per window: 175,376 B read
// (level 0) + 174,764 B of pyramid written.
#include "bp_kernels.h"

namespace bp {

constexpr int kDecThreads = 256;
constexpr int kDecOutPerBlock = 2 * kDecThreads;        // 512 outputs
constexpr int kDecTileIn = 2 * kDecOutPerBlock + 256;   // 1280 staged inputs (1278 used)

// y[n] = sum_{j=0}^{255} h[j] * xz[2n + j - 127],  xz = x zero-extended     (nnaudio.py:269-279)
__global__ __launch_bounds__(kDecThreads) void decimate2_kernel(const float* __restrict__ src,
                                                                int64_t src_stride, int len_in,
                                                                float* __restrict__ dst,
                                                                int64_t dst_stride, int len_out,
                                                                const float* __restrict__ h) {
  __shared__ __attribute__((aligned(16))) float s[kDecTileIn];
  const int b = blockIdx.y;
  const int o0 = blockIdx.x * kDecOutPerBlock;
  const float* x = src + (int64_t)b * src_stride;
  const int in0 = 2 * o0 - 127;
  for (int i = threadIdx.x; i < kDecTileIn; i += kDecThreads) {
    const int g = in0 + i;
    s[i] = (g >= 0 && g < len_in) ? x[g] : 0.0f;
  }
  __syncthreads();

  // outputs n = o0 + 2*tid (A) and n+1 (B).  A reads s[4*tid + j], B reads s[4*tid + 2 + j].
  // Tap quad k (taps 4k..4k+3) multiplies s[4tid+4k .. +3] for A and s[4tid+4k+2 .. +5] for B, so
  // both outputs consume the same four (wave-uniform, scalar-loaded) coefficients per step.
  const float4* s4 = reinterpret_cast<const float4*>(s + 4 * threadIdx.x);
  float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;  // two partial sums per output (even / odd quads)
  float4 cur = s4[0];
#pragma unroll 4
  for (int k = 0; k < 64; k += 2) {
    const float4 mid = s4[k + 1];
    const float4 nxt = s4[k + 2];
    const float h0 = h[4 * k + 0], h1 = h[4 * k + 1], h2 = h[4 * k + 2], h3 = h[4 * k + 3];
    const float h4 = h[4 * k + 4], h5 = h[4 * k + 5], h6 = h[4 * k + 6], h7 = h[4 * k + 7];
    a0 = fmaf(h0, cur.x, a0);
    a0 = fmaf(h1, cur.y, a0);
    a0 = fmaf(h2, cur.z, a0);
    a0 = fmaf(h3, cur.w, a0);
    b0 = fmaf(h0, cur.z, b0);
    b0 = fmaf(h1, cur.w, b0);
    b0 = fmaf(h2, mid.x, b0);
    b0 = fmaf(h3, mid.y, b0);
    a1 = fmaf(h4, mid.x, a1);
    a1 = fmaf(h5, mid.y, a1);
    a1 = fmaf(h6, mid.z, a1);
    a1 = fmaf(h7, mid.w, a1);
    b1 = fmaf(h4, mid.z, b1);
    b1 = fmaf(h5, mid.w, b1);
    b1 = fmaf(h6, nxt.x, b1);
    b1 = fmaf(h7, nxt.y, b1);
    cur = nxt;
  }
  const int n = o0 + 2 * threadIdx.x;
  float* y = dst + (int64_t)b * dst_stride;
  if (n + 1 < len_out) {
    *reinterpret_cast<float2*>(y + n) = make_float2(a0 + a1, b0 + b1);
  } else if (n < len_out) {
    y[n] = a0 + a1;
  }
}

void launch_pyramid(const float* audio, float* pyr, const float* lowpass, int n_windows,
                    hipStream_t stream) {
  for (int k = 1; k < kOctaves; ++k) {
    const float* src = (k == 1) ? audio : pyr + pyr_off(k - 1);
    const int64_t sstride = (k == 1) ? kAudioN : kPyrStride;
    const int lin = level_len(k - 1), lout = level_len(k);
    dim3 grid((lout + kDecOutPerBlock - 1) / kDecOutPerBlock, n_windows);
    hipLaunchKernelGGL(decimate2_kernel, grid, dim3(kDecThreads), 0, stream, src, sstride, lin,
                       pyr + pyr_off(k), (int64_t)kPyrStride, lout, lowpass);
  }
}

// ---- windowing (inference.py:242 zero lead-in of 3840, 207-213 hop 36164 + tail pad) and unwrap_output (inference.py:
// 267-279: keep frames 15..156 of every window, trim to T rows), over the segments of a chunk (bp_common.h WindowSeg).
// win_len / hop: 43844 / 36164 samples at 22.05 kHz, doubled for the extended 44.1 kHz geometry.  blockIdx.y = window
// slot of the chunk, blockIdx.z = map; everything about a slot is block-uniform.

// the segment that holds `slot`: the last one whose first slot is <= slot (the table is in slot order)
__device__ __forceinline__ const WindowSeg& seg_of_slot(const WindowSeg* __restrict__ seg, int n, int slot) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg[mid].at <= slot) lo = mid; else hi = mid;
  }
  return seg[lo];
}

// window `slot`: sample start + i of the source, or 0 outside [0, n_valid)
__device__ __forceinline__ void gather_window(const WindowSeg& g, int slot, float* __restrict__ audio, int win_len, int hop) {
  const int64_t start = g.start + (int64_t)(slot - g.at) * hop;
  int64_t off = start;  // sample start + i lies at src[off + i], in a ring at src[off + i - ring_cap] from i = wrap on
  int wrap = win_len;
  if (g.ring_cap > 0) {
    off = ((start % g.ring_cap) + g.ring_cap) % g.ring_cap;
    wrap = g.ring_cap - (int)off;  // win_len <= ring_cap: one wrap at most
  }
  float* dst = audio + (int64_t)slot * win_len;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < win_len; i += gridDim.x * 256) {
    const int64_t x = start + i;
    dst[i] = (x >= 0 && x < g.n_valid) ? g.src[off + (i < wrap ? i : i - g.ring_cap)] : 0.0f;
  }
}

// kept frames 15..156 of window `slot` of one map -> rows out_row + 142 i onwards of out[map], below total_rows
__device__ __forceinline__ void scatter_window(const WindowSeg& g, int slot, int map, const float* __restrict__ note,
                                               const float* __restrict__ onset, const float* __restrict__ contour) {
  const int64_t row0 = g.out_row + (int64_t)(slot - g.at) * 142;
  const int64_t left = g.total_rows - row0;
  if (row0 < 0 || left <= 0) return;
  const int n_freq = map == 2 ? kFreqC : kFreqN;
  const float* win_out = map == 0 ? note : (map == 1 ? onset : contour);
  const float* src = win_out + ((int64_t)slot * kFrames + 15) * n_freq;
  float* dst = g.out[map] + row0 * n_freq;
  const int n = (int)(left < 142 ? left : 142) * n_freq;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) dst[i] = src[i];
}

// The wrappers differ only in where the segment table lives: the kernel arguments (track calls) or device memory
// (streaming steps).
__global__ __launch_bounds__(256) void window_tracks_kernel(WindowSegs ts, float* __restrict__ audio, int win_len, int hop) {
  gather_window(seg_of_slot(ts.seg, ts.n, blockIdx.y), blockIdx.y, audio, win_len, hop);
}

__global__ __launch_bounds__(256) void window_streams_kernel(const WindowSeg* __restrict__ segs, int n_segs,
                                                             float* __restrict__ audio, int win_len, int hop) {
  gather_window(seg_of_slot(segs, n_segs, blockIdx.y), blockIdx.y, audio, win_len, hop);
}

__global__ __launch_bounds__(256) void unwrap_tracks_kernel(WindowSegs ts, const float* __restrict__ note,
                                                            const float* __restrict__ onset,
                                                            const float* __restrict__ contour) {
  scatter_window(seg_of_slot(ts.seg, ts.n, blockIdx.y), blockIdx.y, blockIdx.z, note, onset, contour);
}

__global__ __launch_bounds__(256) void unwrap_streams_kernel(const WindowSeg* __restrict__ segs, int n_segs,
                                                             const float* __restrict__ note,
                                                             const float* __restrict__ onset,
                                                             const float* __restrict__ contour) {
  scatter_window(seg_of_slot(segs, n_segs, blockIdx.y), blockIdx.y, blockIdx.z, note, onset, contour);
}

void launch_window_tracks(const WindowSegs& ts, int n_slots, float* audio, int win_len, int hop, hipStream_t stream) {
  hipLaunchKernelGGL(window_tracks_kernel, dim3(43, n_slots), dim3(256), 0, stream, ts, audio, win_len, hop);
}

void launch_unwrap_tracks(const WindowSegs& ts, int n_slots, const float* note, const float* onset, const float* contour,
                          hipStream_t stream) {
  hipLaunchKernelGGL(unwrap_tracks_kernel, dim3(16, n_slots, 3), dim3(256), 0, stream, ts, note, onset, contour);
}

void launch_window_streams(const WindowSeg* segs, int n_segs, int n_slots, float* audio, int win_len, int hop,
                           hipStream_t stream) {
  hipLaunchKernelGGL(window_streams_kernel, dim3(43, n_slots), dim3(256), 0, stream, segs, n_segs, audio, win_len, hop);
}

void launch_unwrap_streams(const WindowSeg* segs, int n_segs, int n_slots, const float* note, const float* onset,
                           const float* contour, hipStream_t stream) {
  hipLaunchKernelGGL(unwrap_streams_kernel, dim3(16, n_slots, 3), dim3(256), 0, stream, segs, n_segs, note, onset, contour);
}

}  // namespace bp
