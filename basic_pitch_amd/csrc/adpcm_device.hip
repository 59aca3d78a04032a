// IMA ADPCM on the device (include/basic_pitch_amd_adpcm.h): the blocks of one or many files, as the files store them, to
// interleaved int16 in one launch.  The BP_PCM_S16 ingest (audio_ingest.hip) follows, as it follows flac_device.hip for FLAC.
//
// A CHAIN is one channel of one block: its samples depend on each other (predictor and step index), chains do not.  One lane
// walks one chain; a launch has as many lanes as the job has chains.  The launch takes a table of SEGMENTS (AdpcmSeg,
// bp_kernels.h) — the blocks of one file each; a single file is the one-segment case — and a lane finds its segment by a
// binary search over the segments' first chains.  The two block layouts (RIFF/WAVE tag 0x11, CAF ima4) are one kernel body
// with the layout as a template parameter; the step is adpcm_host.h's, restated for the device.
//
// Bounds: no byte pattern of a file can take a lane out of its buffers.  A chain reads only where [pos, pos + len) lies inside
// its segment's data_bytes (the host has checked byte_off + data_bytes against the buffer), writes frame f only where f <
// frame_cap (the host has sized the output for out_off + frame_cap * channels), and clamps the step index to 0 ... 88 before
// every table read.  The step table lives in LDS (a copy of the constant table per workgroup): no indexed register array,
// no scratch.
//
// The mapping is the plain one: the lanes of a wave read and write block_bytes apart (4 bytes a read, 2 a store).  Staging the
// blocks and the decoded runs through LDS would coalesce both; profiles/adpcm.md has what the plain form costs.  What a chain
// is bound by is latency, not bandwidth — a file of one window has a few dozen chains of thousands of codes — so a chain
// asks for the bytes of kAhead groups at once and reads the table eight entries at a time (ima_step8).
#include <hip/hip_runtime.h>

#include "../../include/basic_pitch_amd_adpcm.h"
#include "bp_kernels.h"

namespace bp {

namespace {

constexpr int kAdpcmThreads = 256;
constexpr int kSteps = 89;

__constant__ int16_t kStepTable[kSteps] = {
    7,     8,     9,     10,    11,    12,    13,    14,    16,    17,    19,    21,    23,    25,    28,    31,    34,    37,
    41,    45,    50,    55,    60,    66,    73,    80,    88,    97,    107,   118,   130,   143,   157,   173,   190,   209,
    230,   253,   279,   307,   337,   371,   408,   449,   494,   544,   598,   658,   724,   796,   876,   963,   1060,  1166,
    1282,  1411,  1552,  1707,  1878,  2066,  2272,  2499,  2749,  3024,  3327,  3660,  4026,  4428,  4871,  5358,  5894,  6484,
    7132,  7845,  8630,  9493,  10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

__device__ __forceinline__ int clamp_index(int index) { return index < 0 ? 0 : index > kSteps - 1 ? kSteps - 1 : index; }

// Eight codes of one chain, low nibble first (adpcm_host.h ima_step, eight times): frames [f, f + 8) below frame_cap are stored.
// The index chain does not depend on the table (index += {-1, -1, -1, -1, 2, 4, 6, 8}[code & 7], clamped), so it runs first,
// the eight table reads are in flight together, and the predictor chain is adds and clamps alone: a lone wave — a file of a
// few blocks — pays the LDS latency once per eight codes, not once per code.  index is inside 0 ... 88 on entry and on return.
__device__ __forceinline__ void ima_step8(const int* step, uint32_t w, int& pred, int& index, int16_t* out, int64_t f, int64_t frame_cap,
                                          int C) {
  int s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int code = (int)((w >> (4 * j)) & 15u);
    s[j] = step[clamp_index(index)];
    index = clamp_index(index + ((code & 4) ? 2 * (code & 3) + 2 : -1));
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int code = (int)((w >> (4 * j)) & 15u);
    int d = s[j] >> 3;
    if (code & 4) d += s[j];
    if (code & 2) d += s[j] >> 1;
    if (code & 1) d += s[j] >> 2;
    pred = (code & 8) ? pred - d : pred + d;
    pred = pred < -32768 ? -32768 : pred > 32767 ? 32767 : pred;
    if (f + j < frame_cap) out[(f + j) * C] = (int16_t)pred;
  }
}

// four bytes at data[at ...] as a little-endian word (a file's blocks start at any byte)
__device__ __forceinline__ uint32_t word_at(const uint8_t* data, int64_t at) {
  return (uint32_t)data[at] | ((uint32_t)data[at + 1] << 8) | ((uint32_t)data[at + 2] << 16) | ((uint32_t)data[at + 3] << 24);
}

constexpr int kAhead = 4;  // groups of a chain whose bytes are asked for together: one memory round trip per 32 codes

template <int CODEC>
__global__ __launch_bounds__(kAdpcmThreads) void adpcm_decode_kernel(const uint8_t* __restrict__ bytes, const AdpcmSeg* __restrict__ segs,
                                                                     int n_segs, int64_t n_chains, int16_t* __restrict__ pcm) {
  __shared__ int step[kSteps];
  if (threadIdx.x < kSteps) step[threadIdx.x] = kStepTable[threadIdx.x];
  __syncthreads();
  const int64_t chain = (int64_t)blockIdx.x * kAdpcmThreads + threadIdx.x;
  if (chain >= n_chains) return;
  // the last segment whose first chain is not behind this one
  int lo = 0, hi = n_segs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].first_chain <= chain) lo = mid;
    else hi = mid - 1;
  }
  const AdpcmSeg sg = segs[lo];
  const int C = sg.channels;
  const int64_t k = chain - sg.first_chain;
  const int64_t b = k / C;
  const int c = (int)(k - b * C);
  if (b >= sg.n_blocks) return;
  const uint8_t* const data = bytes + sg.byte_off;
  int16_t* const out = pcm + sg.out_off + c;  // this channel's sample of frame 0
  const int64_t blk = b * sg.block_bytes;     // the block's first byte in the segment
  if (CODEC == BP_ADPCM_IMA_WAV) {
    const int64_t hdr = blk + 4 * c;
    if (hdr + 4 > sg.data_bytes) return;
    int pred = (int16_t)(uint16_t)(data[hdr] | (data[hdr + 1] << 8));
    int index = clamp_index(data[hdr + 2]);
    const int64_t f0 = b * sg.block_frames;
    if (f0 < sg.frame_cap) out[f0 * C] = (int16_t)pred;
    const int groups = (sg.block_bytes - 4 * C) / (4 * C);
    for (int g0 = 0; g0 < groups; g0 += kAhead) {
      uint32_t w[kAhead];
      bool have[kAhead];
#pragma unroll
      for (int q = 0; q < kAhead; ++q) {
        const int64_t at = blk + (int64_t)4 * C * (1 + g0 + q) + 4 * c;
        have[q] = g0 + q < groups && at + 4 <= sg.data_bytes && f0 + 1 + 8 * (int64_t)(g0 + q) < sg.frame_cap;
        w[q] = have[q] ? word_at(data, at) : 0u;
      }
#pragma unroll
      for (int q = 0; q < kAhead; ++q) {
        if (!have[q]) return;
        ima_step8(step, w[q], pred, index, out, f0 + 1 + 8 * (int64_t)(g0 + q), sg.frame_cap, C);
      }
    }
  } else {
    const int64_t hdr = blk + 34 * c;
    if (hdr + 34 > sg.data_bytes) return;
    const int h = (data[hdr] << 8) | data[hdr + 1];
    int pred = (int16_t)(uint16_t)(h & 0xff80);
    int index = clamp_index(h & 0x7f);
    const int64_t f0 = b * 64;
    uint32_t w[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) w[g] = word_at(data, hdr + 2 + 4 * g);  // inside the 34 bytes checked above
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      if (f0 + 8 * g >= sg.frame_cap) return;
      ima_step8(step, w[g], pred, index, out, f0 + 8 * g, sg.frame_cap, C);
    }
  }
}

}  // namespace

void launch_adpcm_decode(int codec, const uint8_t* bytes, const AdpcmSeg* segs, int n_segs, int64_t n_chains, int16_t* pcm,
                         hipStream_t stream) {
  if (n_segs < 1 || n_chains < 1) return;
  const dim3 grid((unsigned)((n_chains + kAdpcmThreads - 1) / kAdpcmThreads)), block(kAdpcmThreads);
  if (codec == BP_ADPCM_IMA_WAV) adpcm_decode_kernel<BP_ADPCM_IMA_WAV><<<grid, block, 0, stream>>>(bytes, segs, n_segs, n_chains, pcm);
  else adpcm_decode_kernel<BP_ADPCM_IMA4><<<grid, block, 0, stream>>>(bytes, segs, n_segs, n_chains, pcm);
}

}  // namespace bp
