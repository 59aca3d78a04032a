// FLAC decode on the device (round 6; SURVEY.md 8(f) rank 2: "WAV/FLAC decode").  The container half of
// `librosa.load(path, sr=22050, mono=True)` (basic_pitch/inference.py:239; README.md:182-189 lists .flac) for the file job:
// the host decoder (flac_decode.cpp) sustains ~80 M samples per second and core — five three-minute stereo files per second
// and core against the ~1,400 a GPU transcribes — and FLAC halves the bytes a file costs on the storage device, in host
// DRAM and on PCIe, which are what an 8-GPU file job runs out of first.
//
// The format (RFC 9639) is serial inside a frame — a Rice code's position is the sum of the lengths of all codes before
// it, a subframe starts where the previous one ends, linear prediction is a recurrence — and independent from frame to
// frame, each frame beginning on a byte boundary with a sync code and a CRC-8-protected header that carries its own
// position in the stream.  So the FILE's bytes go to the device as they are, and three launches decode them:
//   1. flac_scan_kernel     every byte position that looks like a frame header (sync code, no reserved value, sample size
//                           and channel count of STREAMINFO, CRC-8 right) becomes a candidate (offset, coded number,
//                           block size), kept in file order (a workgroup owns 64 KB of the file and a slice of the list);
//   2. flac_chain_kernel    one workgroup compacts the candidates in file order and keeps those that continue their
//                           predecessor or are continued by their successor (coded number + 1 / sample number + block
//                           size): a sync pattern inside compressed data passes the CRC-8 once in ~10^7 bytes and the number
//                           check practically never — and if it did, the chain as a whole or the frame's CRC-16 fails and
//                           the call reports the file as not decodable here;
//   3. flac_decode_kernel   A LANE TRIO PER FRAME (three waves per 64 frames): the parser — subframe headers, Rice / escaped
//                           residuals from a 32-bit funnel-shift window over a ring of the lane's stream in LDS (the lanes
//                           of a wave load TOGETHER, at a service every 16 codes: see FdBits) —, the restorer — prediction
//                           (constant, verbatim, fixed order 0..4, LPC order 1..12 as exact float64 FMAs on a register
//                           history, 13..32 with 64-bit sums on an LDS ring), wasted bits, the channels as coded to scratch
//                           rows —, fed through a mailbox in LDS, and the checker — the frame's CRC-16 (eight bytes per
//                           step, tables in LDS);
//   4. flac_finalize_kernel the parallel tail, a thread per sample: stereo decorrelation and the interleaved 16- or 32-bit
//                           PCM the ingest kernels read (audio_ingest.hip downmix_raw_kernel) — bit for bit what the host
//                           decoder produces.  A three-minute stereo file is ~1,940 frames = 31 waves; the serial decode of
//                           a frame sets the latency of the call (~1 - 2 ms), not the throughput of the job, whose lanes
//                           keep several files in flight.
// Not decoded here (status BP_FLACDEV_UNSUPPORTED, the caller uses the host decoder): streams without a sample count or
// block sizes in STREAMINFO, more than 24 bits per sample, more than 8 channels.  The MD5 of STREAMINFO is not checked on
// the device (one serial pass over the whole stream); every frame's CRC-16 and the stream's sample count are.
#include "flac_kernels.h"

namespace bp {

// The four launches of one file: each kernel is its stage's body (flac_kernels.h) on the one stream of the call.
__global__ __launch_bounds__(256) void flac_scan_kernel(const uint8_t* __restrict__ file, FdStream st, FdCand* __restrict__ cands,
                                                        uint32_t* __restrict__ counts, int* __restrict__ status) {
  fd_scan_chunk(file, st, blockIdx.x, cands + (size_t)blockIdx.x * kFdChunkCands, counts + blockIdx.x, status);
}

__global__ __launch_bounds__(kFdChainThreads) void flac_chain_kernel(const FdCand* __restrict__ cands, const uint32_t* __restrict__ counts,
                                                                     int n_chunks, FdStream st, FdCand* __restrict__ packed,
                                                                     uint32_t* __restrict__ offs, FdFrame* __restrict__ frames,
                                                                     int max_frames, int* __restrict__ n_frames,
                                                                     int* __restrict__ status) {
  fd_chain_stream(cands, counts, n_chunks, st, packed, offs, frames, max_frames, n_frames, status);
}

__global__ __launch_bounds__(3 * kFdLanes) void flac_decode_kernel(FdDecodeParams p) {
  fd_decode_frame(p, blockIdx.x * kFdLanes + (threadIdx.x & (kFdLanes - 1)));
}

__global__ __launch_bounds__(256) void flac_finalize_kernel(FdDecodeParams p) {
  fd_finalize_sample(p, blockIdx.y, blockIdx.x * 256 + threadIdx.x);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// The CRC-16 tables of the checker ([8][256], eight bytes per step), made once per handle.
int flac_device_crc_table(FlacDeviceBuffers& b) {
  if (b.crc_tab) return 0;
  uint16_t tab[8][256];
  for (int i = 0; i < 256; ++i) {
    uint16_t c = (uint16_t)(i << 8);
    for (int k = 0; k < 8; ++k) c = (uint16_t)((c & 0x8000) ? (c << 1) ^ 0x8005 : c << 1);
    tab[0][i] = c;
  }
  for (int k = 1; k < 8; ++k)
    for (int i = 0; i < 256; ++i) tab[k][i] = (uint16_t)((tab[k - 1][i] << 8) ^ tab[0][tab[k - 1][i] >> 8]);
  return b.crc_tab.upload(&tab[0][0], 8 * 256) == hipSuccess ? 0 : -1;
}

// Decode the FLAC stream at `d_file` (already on the device, padded with >= 64 zero bytes) into interleaved PCM at `d_pcm`
// (int16 when bits <= 16, else int32 left-justified).  Asynchronous on `stream`; *status (device) receives the error bits.
int flac_device_decode(FlacDeviceBuffers& b, const FdStream& st, void* d_pcm, hipStream_t stream) {
  const int n_chunks = (int)((st.nbytes - st.audio_start + kFdChunk - 1) / kFdChunk);
  const int64_t max_frames = (st.total + st.min_block - 1) / st.min_block + 1;
  if (!fd_reserve(b.cands, (size_t)n_chunks * kFdChunkCands, sizeof(FdCand)) || !fd_reserve(b.counts, (size_t)n_chunks) ||
      !fd_reserve(b.packed, (size_t)n_chunks * kFdChunkCands, sizeof(FdCand)) || !fd_reserve(b.offs, (size_t)n_chunks) ||
      !fd_reserve(b.frames, (size_t)max_frames, sizeof(FdFrame)) ||
      !fd_reserve(b.scratch, (size_t)max_frames * st.max_block * st.channels))
    return -1;
  if (!b.meta && b.meta.reserve(2) != hipSuccess) return -1;
  if (flac_device_crc_table(b) != 0) return -1;
  if (hipMemsetAsync(b.meta, 0, 2 * sizeof(int), stream) != hipSuccess) return -1;
  hipLaunchKernelGGL(flac_scan_kernel, dim3(n_chunks), dim3(256), 0, stream, b.file, st, b.cands.as<FdCand>(), b.counts, b.meta);
  hipLaunchKernelGGL(flac_chain_kernel, dim3(1), dim3(kFdChainThreads), 0, stream, b.cands.as<const FdCand>(), b.counts, n_chunks,
                     st, b.packed.as<FdCand>(), b.offs, b.frames.as<FdFrame>(), (int)max_frames, b.meta + 1, b.meta);
  FdDecodeParams p{b.file, b.frames.as<const FdFrame>(), b.meta + 1, st, b.scratch, d_pcm, st.bits <= 16 ? 16 - st.bits : 32 - st.bits,
                   st.bits <= 16 ? 0 : 1, b.meta, b.crc_tab};
  hipLaunchKernelGGL(flac_decode_kernel, dim3((unsigned)((max_frames + kFdLanes - 1) / kFdLanes)), dim3(3 * kFdLanes), 0, stream, p);
  hipLaunchKernelGGL(flac_finalize_kernel, dim3((unsigned)((st.max_block + 255) / 256), (unsigned)max_frames), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace bp
