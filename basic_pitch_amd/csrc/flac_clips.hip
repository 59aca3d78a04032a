// FLAC decode on the device for a JOB of many streams (bp_infer_flac_clips_candidates, clips_api.hip).  A short
// clip is a few dozen frames: decoded alone (flac_device.hip) it fills less than one wave of the decode kernel and pays four
// launches, an upload and a wait for ~40 us of device work.  Here the four stages run ONCE for all clips of a job:
//   * every clip's bytes lie in one buffer, each clip 16-byte aligned and followed by >= 64 zero bytes (the padding the scan's
//     pieces, the header parse and the parser's blocks may read into), and a table (FdClip, bp_kernels.h) says where: the
//     clip's own FdStream — audio_start and nbytes count from the clip's first byte —, its first scan workgroup (= its first
//     slice of the candidate lists), its first frame slot, its rows of scratch, its PCM;
//   * scan      a workgroup finds its clip by binary search over the first workgroups (as clip_of_block, audio_ingest.hip) and
//               scans that clip's chunk up to that clip's nbytes: a sync pattern in a clip's last bytes is a candidate of that
//               clip or of none;
//   * chain     a workgroup per clip, on that clip's slices, into that clip's frame slots, status word and frame count;
//   * decode    a lane trio per frame SLOT; a lane finds its clip by binary search over the first slots, so the frames of one
//               wave may be of different streams (bits, channels, block sizes): everything the body reads of the stream is
//               per lane.  Slots a clip's chain did not fill (it has max_frames of them) end at once;
//   * finalize  a workgroup per slot (grid.x), looping over the frame's samples.
// The bodies are those of the single-file kernels (flac_kernels.h): a clip's samples are bit for bit what flac_device_decode
// gives for it alone, whatever its neighbours.  Error bits go to the clip's own word: meta[2 c] status, meta[2 c + 1] frames.
#include "flac_kernels.h"

namespace bp {

// the last clip whose first workgroup / slot is <= idx (the table is sorted by both; every clip owns >= 1 of each)
template <uint32_t FdClip::*kFirst>
__device__ __forceinline__ int64_t fd_clip_of(const FdClip* __restrict__ clips, int64_t n, uint32_t idx) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (clips[mid].*kFirst <= idx) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ FdDecodeParams fd_clip_params(const FdClip& k, int64_t c, const uint8_t* job, const FdFrame* frames,
                                                         int32_t* scratch, uint8_t* pcm, int* meta, const uint16_t* crc_tab) {
  return FdDecodeParams{job + k.base, frames + k.first_slot, meta + 2 * c + 1, k.st, scratch + k.scratch_off, pcm + k.pcm_off,
                        k.out_shift, k.out_wide, meta + 2 * c, crc_tab};
}

__global__ __launch_bounds__(256) void flac_clips_scan_kernel(const uint8_t* __restrict__ job, const FdClip* __restrict__ clips,
                                                              int64_t n_clips, FdCand* __restrict__ cands,
                                                              uint32_t* __restrict__ counts, int* __restrict__ meta) {
  const int64_t c = fd_clip_of<&FdClip::first_wg>(clips, n_clips, blockIdx.x);
  const FdClip k = clips[c];
  fd_scan_chunk(job + k.base, k.st, blockIdx.x - k.first_wg, cands + (size_t)blockIdx.x * kFdChunkCands, counts + blockIdx.x,
                meta + 2 * c);
}

__global__ __launch_bounds__(kFdChainThreads) void flac_clips_chain_kernel(const FdClip* __restrict__ clips,
                                                                           const FdCand* __restrict__ cands,
                                                                           const uint32_t* __restrict__ counts,
                                                                           FdCand* __restrict__ packed, uint32_t* __restrict__ offs,
                                                                           FdFrame* __restrict__ frames, int* __restrict__ meta) {
  const int64_t c = blockIdx.x;
  const FdClip k = clips[c];
  fd_chain_stream(cands + (size_t)k.first_wg * kFdChunkCands, counts + k.first_wg, k.n_chunks, k.st,
                  packed + (size_t)k.first_wg * kFdChunkCands, offs + k.first_wg, frames + k.first_slot, k.max_frames,
                  meta + 2 * c + 1, meta + 2 * c);
}

__global__ __launch_bounds__(3 * kFdLanes) void flac_clips_decode_kernel(const uint8_t* __restrict__ job,
                                                                         const FdClip* __restrict__ clips, int64_t n_clips,
                                                                         const FdFrame* __restrict__ frames, int32_t* scratch,
                                                                         uint8_t* pcm, int* meta, const uint16_t* crc_tab) {
  // a slot behind the last clip's (the grid is whole waves) lands in the last clip with f >= its max_frames >= its frame count
  const uint32_t slot = blockIdx.x * kFdLanes + (threadIdx.x & (kFdLanes - 1));
  const int64_t c = fd_clip_of<&FdClip::first_slot>(clips, n_clips, slot);
  const FdClip k = clips[c];
  fd_decode_frame(fd_clip_params(k, c, job, frames, scratch, pcm, meta, crc_tab), (int)(slot - k.first_slot));
}

__global__ __launch_bounds__(256) void flac_clips_finalize_kernel(const FdClip* __restrict__ clips, int64_t n_clips,
                                                                  const FdFrame* __restrict__ frames, int32_t* scratch, uint8_t* pcm,
                                                                  int* meta) {
  const int64_t c = fd_clip_of<&FdClip::first_slot>(clips, n_clips, blockIdx.x);
  const FdClip k = clips[c];
  const FdDecodeParams p = fd_clip_params(k, c, nullptr, frames, scratch, pcm, meta, nullptr);
  const int f = (int)(blockIdx.x - k.first_slot);
  for (int i = threadIdx.x; i < k.st.max_block; i += 256) fd_finalize_sample(p, f, i);
}

// Decode the n_clips > 0 streams of `tab` (host; read by an asynchronous copy: alive until the stream has been waited for), whose
// bytes are in b.file, into d_pcm (pcm_bytes, zeroed first: a clip that fails leaves no uninitialised memory).  b.meta receives
// [n_clips][2]: error bits, frame count.  wgs / slots / scratch: the totals over the table.
int flac_clips_decode(FlacDeviceBuffers& b, const FdClip* tab, int64_t n_clips, int64_t wgs, int64_t slots, int64_t scratch,
                      void* d_pcm, size_t pcm_bytes, hipStream_t stream) {
  if (!fd_reserve(b.cands, (size_t)wgs * kFdChunkCands, sizeof(FdCand)) || !fd_reserve(b.counts, (size_t)wgs) ||
      !fd_reserve(b.packed, (size_t)wgs * kFdChunkCands, sizeof(FdCand)) || !fd_reserve(b.offs, (size_t)wgs) ||
      !fd_reserve(b.frames, (size_t)slots, sizeof(FdFrame)) || !fd_reserve(b.scratch, (size_t)scratch) ||
      !fd_reserve(b.clips, (size_t)n_clips, sizeof(FdClip)) || !fd_reserve(b.meta, (size_t)(2 * n_clips)))
    return -1;
  if (flac_device_crc_table(b) != 0) return -1;
  if (hipMemcpyAsync(b.clips, tab, (size_t)n_clips * sizeof(FdClip), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemsetAsync(b.meta, 0, (size_t)(2 * n_clips) * sizeof(int), stream) != hipSuccess ||
      (pcm_bytes && hipMemsetAsync(d_pcm, 0, pcm_bytes, stream) != hipSuccess))
    return -1;
  const FdClip* d_tab = b.clips.as<const FdClip>();
  hipLaunchKernelGGL(flac_clips_scan_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, b.file, d_tab, n_clips, b.cands.as<FdCand>(),
                     b.counts, b.meta);
  hipLaunchKernelGGL(flac_clips_chain_kernel, dim3((unsigned)n_clips), dim3(kFdChainThreads), 0, stream, d_tab,
                     b.cands.as<const FdCand>(), b.counts, b.packed.as<FdCand>(), b.offs, b.frames.as<FdFrame>(), b.meta);
  hipLaunchKernelGGL(flac_clips_decode_kernel, dim3((unsigned)((slots + kFdLanes - 1) / kFdLanes)), dim3(3 * kFdLanes), 0, stream,
                     b.file, d_tab, n_clips, b.frames.as<const FdFrame>(), b.scratch, static_cast<uint8_t*>(d_pcm), b.meta, b.crc_tab);
  hipLaunchKernelGGL(flac_clips_finalize_kernel, dim3((unsigned)slots), dim3(256), 0, stream, d_tab, n_clips,
                     b.frames.as<const FdFrame>(), b.scratch, static_cast<uint8_t*>(d_pcm), b.meta);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace bp
