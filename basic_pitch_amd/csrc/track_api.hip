// C ABI of the track family (include/basic_pitch_amd.h): whole signals -> un-overlapped posteriorgrams on the device — from
// host or device samples, raw PCM (downmix + resampling), or a FLAC or IMA ADPCM file's bytes decoded on the device — and the
// device-side note candidates of those maps.
//
// Every entry point is a source, the track and a sink on one driver (run_track):
//   validate everything -> queue the source -> tracks_core -> queue the sink -> wait -> the FLAC decoder's verdict.
// Nothing is queued before every argument has been checked, and a call that fails after queuing work returns only once the
// handle's stream has drained (finish): the caller may reuse its buffers as soon as any call returns.
//
// The staging buffers of these calls are the handle's typed, grow-only buffers (device_buffer.h): a call reserves what it
// needs before it queues work on them, and nothing here frees by hand.
#include <algorithm>

#include "../../include/basic_pitch_amd_adpcm.h"
#include "bp_context.h"

using namespace bp;

extern "C" void bp_internal_bend_tables(int32_t* tab, double* gauss);
extern "C" void bp_internal_freq_limits(const bp_note_params* prm, int* lo, int* hi);
extern "C" int bp_internal_flac_device_supported(const bp_flac_stream_layout* lay, size_t nbytes);

namespace {

// ---- geometry: windows and frames of a 22.05 kHz signal for a hop / lead-in (the reference's 36164 / 3840, or a handle's:
// doubled for the extended range), the length of a signal resampled to `rate`
int64_t n_windows_of(int64_t n_samples, int hop, int lead) { return n_samples <= 0 ? 0 : (n_samples + lead + hop - 1) / hop; }

int64_t n_frames_of(int64_t n_samples, int hop, int lead) {
  if (n_samples <= 0) return 0;
  // int(n_samples / hop_size * 142) evaluated like the reference: float64 division, then product
  const double n_expected_windows = (double)n_samples / (double)hop;
  const int64_t rows = (int64_t)(n_expected_windows * (double)BP_FRAMES_PER_WINDOW);
  const int64_t avail = n_windows_of(n_samples, hop, lead) * BP_FRAMES_PER_WINDOW;
  return rows < avail ? rows : avail;
}

int64_t h_windows(bp_handle h, int64_t n) { return n_windows_of(n, h->hop, h->lead); }

}  // namespace

// ---- what the clip jobs (clips_api.hip) and the streaming sessions (stream_api.hip) share with this file (declared in
// bp_context.h): the end of a call, the argument domain of raw PCM, the resampling filter's builder, the copies of the three
// maps, the geometry of a handle, track_out, the tracks and the way home of the note candidates
namespace bp {

// The end of a call that has queued work: the wait, or on the first error the drained stream (its own status ignored), so
// that no copy from or into a caller's buffer is still in flight when the call returns.
int finish(bp_handle h, int rc) {
  if (rc == BP_OK) rc = wait_stream(h);
  if (rc != BP_OK) (void)hipStreamSynchronize(h->stream);
  return rc;
}

int pcm_width(int format) {
  // BP_PCM_F32, S16, S24, S32, U8, F64; S16_BE, S24_BE, S32_BE, F32_BE, F64_BE, S8, ULAW, ALAW
  static const int width[] = {4, 2, 3, 4, 1, 8, 2, 3, 4, 4, 8, 1, 1, 1};
  return format >= BP_PCM_F32 && format <= BP_PCM_ALAW ? width[format] : 0;
}

// pcm_given: false for a null pcm pointer (the FLAC path's device buffer counts as given)
int check_ingest(bp_handle h, bool pcm_given, int format, int64_t n_frames, int channels, int sample_rate, int mem_kind) {
  if (n_frames < 0 || channels < 1 || channels > 64 || sample_rate < 1000 || sample_rate > 768000 || pcm_width(format) == 0 ||
      (mem_kind != BP_MEM_HOST && mem_kind != BP_MEM_DEVICE) || (n_frames > 0 && !pcm_given)) {
    h->err = "audio ingest: bad argument (n_frames, channels, sample_rate, format, mem_kind or null pcm)";
    return BP_ERR_INVALID_ARG;
  }
  return BP_OK;
}

int upload_filter(bp_handle h, int sample_rate, bool tabulated_only, ResamplePlan* plan, DeviceBuffer<double>* dev) {
  std::vector<double> taps;
  ResamplePlan pl = make_resample_plan(sample_rate, h->rate, taps);
  pl.rev_off = 0;
  *plan = pl;
  if (pl.direct && tabulated_only) return BP_ERR_UNSUPPORTED;
  if (!pl.direct && pl.up == 1 && pl.down == 2) {
    // the 2 : 1 kernel walks the taps backwards, a block of 32 per scalar load: a reversed copy behind the table, padded
    // with zeros to whole blocks (a zero tap adds x * 0 = 0 to a float64 sum)
    const size_t M = taps.size(), base = (M + 31) / 32 * 32;
    taps.resize(2 * base, 0.0);
    for (size_t i = 0; i < M; ++i) taps[base + i] = taps[M - 1 - i];
    plan->rev_off = (int64_t)base;
  }
  BP_HIP(dev->upload(taps.data(), taps.size()));
  return BP_OK;
}

int copy_maps(bp_handle h, const Maps& dst, const Maps& src, int64_t T, hipMemcpyKind kind) {
  BP_HIP(hipMemcpyAsync(dst.note, src.note, (size_t)T * kFreqN * 4, kind, h->stream));
  BP_HIP(hipMemcpyAsync(dst.onset, src.onset, (size_t)T * kFreqN * 4, kind, h->stream));
  BP_HIP(hipMemcpyAsync(dst.contour, src.contour, (size_t)T * kFreqC * 4, kind, h->stream));
  return BP_OK;
}

int64_t resampled_length(int64_t n_frames, int sample_rate, int rate) {
  return n_frames <= 0 || sample_rate <= 0 ? 0 : (n_frames * (int64_t)rate + sample_rate - 1) / sample_rate;
}

int64_t h_frames(bp_handle h, int64_t n) { return n_frames_of(n, h->hop, h->lead); }

// The only way to h->track_out: grown for `rows` rows of maps.  Whatever a *_candidates call left there for bp_track_maps
// is gone from then on.
int take_track_out(bp_handle h, int64_t rows, Maps* m) {
  h->maps_rows = 0;
  BP_HIP(h->track_out.reserve((size_t)(rows * kMapsRow)));
  *m = maps_at(h->track_out, rows);
  return BP_OK;
}

// A private copy of maps the caller gives (T rows, host or device memory after mem_kind) in track_out: the frequency limits
// are applied in place.  *m: the copy.
int take_given_maps(bp_handle h, const float* note, const float* onset, const float* contour, int64_t T, int mem_kind, Maps* m) {
  if (int rc = take_track_out(h, T, m)) return rc;
  if (T == 0) return BP_OK;
  const Maps given{const_cast<float*>(note), const_cast<float*>(onset), const_cast<float*>(contour)};  // only read
  return copy_maps(h, *m, given, T, mem_kind == BP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice);
}

int flac_format(const bp_flac_stream_layout& lay) { return lay.bits_per_sample > 16 ? BP_PCM_S32 : BP_PCM_S16; }

// n samples as the device decoders leave them — left-justified in 16 bits, or in 32 (wide) — to int32; src may be out
void flac_pcm_to_int32(const void* src, bool wide, int shift, int64_t n, int32_t* out) {
  const int32_t* s32 = static_cast<const int32_t*>(src);
  const int16_t* s16 = static_cast<const int16_t*>(src);
  for (int64_t i = 0; i < n; ++i) out[i] = (wide ? s32[i] : (int32_t)s16[i]) >> shift;
}

// ---- the tracks: windows of device-resident model-rate signals -> their un-overlapped maps (device memory).  The windows of
// consecutive tracks are packed into full chunks; the pieces of a chunk — one WindowSeg each; a single track: one per
// chunk — are windowed by ONE launch and un-overlapped by one launch (more than kMaxTrackSegs pieces per chunk: several)
int tracks_core(bp_handle h, int64_t n_tracks, const float* const* d_in, const int64_t* n_samples, const Maps* d_out) {
  hipStream_t s = h->stream;
  std::vector<WindowSeg> segs;
  int cur = 0;
  auto for_groups = [&](auto&& fn) {
    for (size_t g0 = 0; g0 < segs.size(); g0 += kMaxTrackSegs) {
      WindowSegs ts{};
      ts.n = (int)std::min<size_t>(kMaxTrackSegs, segs.size() - g0);
      for (int k = 0; k < ts.n; ++k) ts.seg[k] = segs[g0 + k];
      const int first = ts.seg[0].at, slots = ts.seg[ts.n - 1].at + ts.seg[ts.n - 1].n_windows - first;
      for (int k = 0; k < ts.n; ++k) ts.seg[k].at -= first;  // slots relative to the group's first window
      fn(ts, first, slots);
    }
  };
  auto flush = [&]() -> int {
    if (cur == 0) return BP_OK;
    for_groups([&](const WindowSegs& ts, int first, int slots) {
      launch_window_tracks(ts, slots, h->audio + (int64_t)first * h->win_len, h->win_len, h->hop, s);
    });
    if (int rc = run_chunk(h, h->audio, cur, h->note, h->onset, h->contour)) return rc;
    for_groups([&](const WindowSegs& ts, int first, int slots) {
      launch_unwrap_tracks(ts, slots, h->note + (int64_t)first * kPlaneN, h->onset + (int64_t)first * kPlaneN,
                           h->contour + (int64_t)first * kPlaneC, s);
    });
    segs.clear();
    cur = 0;
    return BP_OK;
  };
  for (int64_t t = 0; t < n_tracks; ++t) {
    const int64_t n_win = h_windows(h, n_samples[t]);
    const int64_t T = h_frames(h, n_samples[t]);
    for (int64_t w0 = 0; w0 < n_win;) {
      const int64_t room = h->cap - cur;
      const int n = (int)((n_win - w0) < room ? (n_win - w0) : room);
      segs.push_back(WindowSeg{d_in[t], {d_out[t].note, d_out[t].onset, d_out[t].contour}, n_samples[t], w0 * h->hop - h->lead,
                               w0 * BP_FRAMES_PER_WINDOW, T, 0, n, cur});
      cur += n;
      w0 += n;
      if (cur == h->cap)
        if (int rc = flush()) return rc;
    }
  }
  if (int rc = flush()) return rc;
  BP_HIP(hipGetLastError());
  return BP_OK;
}

// The results of T rows go home: the note map, the bitmap and the bends (null: not wanted), and the n_stats records at d_stats
// into stats_host (stats_host_dev: the same page-locked block as the device sees it).
// Into page-locked buffers (bp_host_alloc) a kernel of this stream writes them over PCIe itself:
// the copy engine serialises the copies of all lanes in both directions (measured: a lane's 27 MB of posteriorgrams
// going out kept the next file's samples from coming in), and it is busy with the inbound samples.  Pageable
// destinations take ordinary copies.
// (the attributes describe the START of a buffer only — a pointer into a page-locked block that ends before
// `bytes` would send the kernel's writes past the registration.  The whole extent must lie inside the allocation the
// pointer belongs to: hipMemGetAddressRange gives its base and size for the device view of a page-locked block; where that
// cannot be established the copies take over.)
int send_candidates(bp_handle h, const float* d_note, int64_t T, const uint8_t* d_bits, const int8_t* d_bend, float* note_out,
                    uint8_t* cand_out, int8_t* bend_out, void* d_stats, int* stats_host, void* stats_host_dev, int64_t n_stats,
                    bool* exported_by_kernel) {
  hipStream_t s = h->stream;
  const int64_t bits_bytes = T * BP_NOTE_CAND_ROW_BYTES, bend_bytes = T * 88;  // multiples of 4
  const bool want_bends = d_bend != nullptr;
  auto device_view = [](void* p, size_t bytes) -> void* {
    hipPointerAttribute_t at;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (!p) return nullptr;
    if (hipPointerGetAttributes(&at, p) != hipSuccess || (at.type == hipMemoryTypeHost && at.devicePointer &&
                                                          hipMemGetAddressRange(&base, &size, at.devicePointer) != hipSuccess)) {
      (void)hipGetLastError();
      return nullptr;
    }
    if (at.type != hipMemoryTypeHost || !at.devicePointer) return nullptr;
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(base), q = reinterpret_cast<uintptr_t>(at.devicePointer);
    return (q >= b0 && q + bytes <= b0 + size) ? at.devicePointer : nullptr;
  };
  void *v_note = device_view(note_out, (size_t)T * 88 * 4), *v_bits = device_view(cand_out, (size_t)bits_bytes),
       *v_bend = want_bends ? device_view(bend_out, (size_t)bend_bytes) : nullptr;
  const bool aligned = !((reinterpret_cast<uintptr_t>(v_note) | reinterpret_cast<uintptr_t>(v_bits) | reinterpret_cast<uintptr_t>(v_bend)) & 3);
  if (v_note && v_bits && (v_bend || !want_bends) && aligned) {
    // ... the stats records with them; the same kernel leaves the device records initialised for the next call
    launch_note_export(d_note, v_note, T * 88 * 4, d_bits, v_bits, bits_bytes, d_bend, v_bend, bend_bytes, d_stats,
                       stats_host_dev, n_stats, s);
    BP_HIP(hipGetLastError());
    *exported_by_kernel = true;
  } else {
    BP_HIP(hipMemcpyAsync(stats_host, d_stats, (size_t)n_stats * kStatsBytes, hipMemcpyDeviceToHost, s));
    BP_HIP(hipMemcpyAsync(note_out, d_note, (size_t)T * 88 * 4, hipMemcpyDeviceToHost, s));
    BP_HIP(hipMemcpyAsync(cand_out, d_bits, (size_t)bits_bytes, hipMemcpyDeviceToHost, s));
    if (want_bends) BP_HIP(hipMemcpyAsync(bend_out, d_bend, (size_t)bend_bytes, hipMemcpyDeviceToHost, s));
  }
  return BP_OK;
}

// room for the bitmap and the bends of T rows in h->nd_buf
int reserve_candidates(bp_handle h, int64_t T, uint8_t** d_bits, int8_t** d_bend) {
  const int64_t bits_room = (T * BP_NOTE_CAND_ROW_BYTES + 15) & ~(int64_t)15;
  BP_HIP(h->nd_buf.reserve((size_t)(bits_room + T * 88)));
  *d_bits = h->nd_buf;
  *d_bend = h->nd_buf.as<int8_t>() + bits_room;
  return BP_OK;
}

}  // namespace bp

namespace {

// host samples of n_tracks tracks (`total` in all) into h->track, one after the other; d_in[t]: track t's device view
int stage_samples(bp_handle h, int64_t n_tracks, const float* const* samples, const int64_t* n_samples, int64_t total,
                  const float** d_in) {
  BP_HIP(h->track.reserve((size_t)total));
  for (int64_t t = 0, so = 0; t < n_tracks; so += n_samples[t++]) {
    if (n_samples[t] > 0)
      BP_HIP(hipMemcpyAsync(h->track + so, samples[t], (size_t)n_samples[t] * 4, hipMemcpyHostToDevice, h->stream));
    d_in[t] = h->track + so;
  }
  return BP_OK;
}

// ---- audio ingest: downmix + resample into h->res_dev (or straight through when already mono 22.05 kHz on the device)
// n_frames > 0, the arguments checked; *out = device pointer of the 22.05 kHz signal (bp_handle_resampled_length samples)
int queue_ingest(bp_handle h, const void* pcm, int format, int64_t n_frames, int channels, int sample_rate, int mem_kind,
                 const float** out) {
  hipStream_t s = h->stream;
  const int64_t n_out = bp_handle_resampled_length(h, n_frames, sample_rate);
  const void* d_pcm = pcm;
  if (mem_kind == BP_MEM_HOST) {
    const int64_t bytes = n_frames * channels * pcm_width(format);
    BP_HIP(h->pcm_dev.reserve((size_t)bytes));
    BP_HIP(hipMemcpyAsync(h->pcm_dev, pcm, (size_t)bytes, hipMemcpyHostToDevice, s));
    d_pcm = h->pcm_dev;
  }
  const float* d_mono = static_cast<const float*>(d_pcm);
  if (channels > 1 || format != BP_PCM_F32) {
    BP_HIP(h->mono_dev.reserve((size_t)n_frames));
    launch_downmix_raw(d_pcm, format, n_frames, channels, h->mono_dev, s);
    d_mono = h->mono_dev;
  }
  if (sample_rate == h->rate) {
    *out = d_mono;
    return BP_OK;
  }
  if (h->taps_rate != sample_rate) {  // one cached filter: replaced when the rate changes
    h->taps_rate = 0;
    BP_HIP(h->taps_dev.reset());
    if (int rc = upload_filter(h, sample_rate, false, &h->plan, &h->taps_dev)) return rc;
    h->taps_rate = sample_rate;
  }
  BP_HIP(h->res_dev.reserve((size_t)n_out));
  launch_resample(d_mono, n_frames, h->taps_dev, h->plan, h->res_dev, n_out, h->resample_mode, s);
  BP_HIP(hipGetLastError());
  *out = h->res_dev;
  return BP_OK;
}

// ---- FLAC decoded on the device (flac_device.hip) -----------------------------------------------------------------------
int check_flac(bp_handle h, const void* file, size_t nbytes, bp_flac_stream_layout* lay) {
  if (!file || nbytes < 42) {
    h->err = "FLAC on the device: null or too short";
    return BP_ERR_INVALID_ARG;
  }
  if (bp_flac_layout(file, nbytes, lay) != BP_OK) {
    h->err = std::string("FLAC on the device: ") + bp_audio_last_error();
    return BP_ERR_BAD_AUDIO;
  }
  if (!bp_internal_flac_device_supported(lay, nbytes)) {
    h->err = "FLAC on the device: a stream the device decoder leaves to the host (no sample count / block sizes in STREAMINFO, "
             "more than 24 bits or 8 channels, or 2 GB and more)";
    return BP_ERR_UNSUPPORTED;
  }
  return BP_OK;
}

// The file's bytes to the device, the three decode launches queued on the handle's stream, the error bits on their way to a
// page-locked word; the PCM (flac_format) is being written to h->pcm_dev.
int queue_flac(bp_handle h, const void* file, size_t nbytes, const bp_flac_stream_layout& lay) {
  hipStream_t s = h->stream;
  BP_HIP(h->fd_status_host.alloc(2));
  if (nbytes + 64 > h->fd.file.capacity()) BP_HIP(h->fd.file.reserve(nbytes + nbytes / 4 + 4096));
  BP_HIP(hipMemcpyAsync(h->fd.file, file, nbytes, hipMemcpyHostToDevice, s));
  BP_HIP(hipMemsetAsync(h->fd.file + nbytes, 0, 64, s));
  const int64_t bytes = lay.n_frames * lay.channels * (flac_format(lay) == BP_PCM_S32 ? 4 : 2);
  BP_HIP(h->pcm_dev.reserve((size_t)bytes));
  FdStream st{lay.channels, lay.bits_per_sample, lay.min_block, lay.max_block, lay.n_frames, (uint32_t)lay.audio_start,
              (uint32_t)nbytes};
  if (flac_device_decode(h->fd, st, h->pcm_dev, s) != 0) {
    h->err = "FLAC on the device: allocation or launch failed";
    (void)hipGetLastError();
    return BP_ERR_HIP;
  }
  BP_HIP(hipMemcpyAsync(h->fd_status_host, h->fd.meta, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
  return BP_OK;
}

// after the stream has been waited for: what the decode kernels reported
int flac_device_verdict(bp_handle h) {
  const int st = h->fd_status_host ? h->fd_status_host[0] : 0;
  if (st == 0) return BP_OK;
  h->err = std::string("FLAC on the device: the stream could not be decoded (") + ((st & 2) ? "frame chain " : "") +
           ((st & 4) ? "CRC-16 " : "") + ((st & 8) ? "reserved value / overrun " : "") + ((st & 16) ? "candidate overflow " : "") +
           "); the host decoder (bp_flac_decode) reports the cause";
  return BP_ERR_BAD_AUDIO;
}

// ---- IMA ADPCM decoded on the device (adpcm_device.hip) ------------------------------------------------------------------------
int check_adpcm(bp_handle h, const void* file, size_t nbytes, bp_adpcm_layout* lay) {
  if (!file) {
    h->err = "IMA ADPCM on the device: null file";
    return BP_ERR_INVALID_ARG;
  }
  if (bp_adpcm_layout_of(file, nbytes, lay) != BP_OK) {
    h->err = std::string("IMA ADPCM on the device: ") + bp_files_last_error();
    return BP_ERR_BAD_AUDIO;
  }
  return BP_OK;
}

}  // namespace

// What the track calls and the clip jobs share (bp_context.h): the blocks of n files at files[i] + lay[i].data_start to the
// device, one after the other, and ONE launch that expands them all; file i's samples (BP_PCM_S16, interleaved) lie at
// h->ad.pcm + pcm_off[i].  All files have lay[0]'s codec.  segs: the caller's, alive until the stream has been waited for.
int bp::queue_adpcm(bp_handle h, int64_t n, const void* const* files, const bp_adpcm_layout* lay, std::vector<AdpcmSeg>& segs,
                    int64_t* pcm_off) {
  hipStream_t s = h->stream;
  segs.clear();
  int64_t bytes = 0, samples = 0, chains = 0;
  for (int64_t i = 0; i < n; ++i) {
    const bp_adpcm_layout& l = lay[i];
    const int64_t blocks = (l.n_frames + l.block_frames - 1) / l.block_frames;  // (those that hold a frame to write)
    samples = (samples + 7) / 8 * 8;  // every file's samples from a 16-byte boundary
    pcm_off[i] = samples;
    if (blocks > 0) segs.push_back(AdpcmSeg{bytes, blocks * l.block_bytes, samples, l.n_frames, chains, (int32_t)blocks, l.block_bytes, l.block_frames, l.channels});
    bytes += blocks * l.block_bytes, samples += l.n_frames * l.channels, chains += blocks * l.channels;
  }
  if (segs.empty()) return BP_OK;
  if ((size_t)bytes > h->ad.file.capacity()) BP_HIP(h->ad.file.reserve((size_t)(bytes + bytes / 4 + 4096)));
  if ((size_t)samples > h->ad.pcm.capacity()) BP_HIP(h->ad.pcm.reserve((size_t)(samples + samples / 4 + 4096)));
  if (segs.size() > h->ad.segs.capacity()) BP_HIP(h->ad.segs.reserve(segs.size() + segs.size() / 4 + 16));
  for (int64_t i = 0, k = 0; i < n; ++i) {
    if (lay[i].n_frames <= 0) continue;
    const AdpcmSeg& sg = segs[(size_t)k++];
    BP_HIP(hipMemcpyAsync(h->ad.file + sg.byte_off, static_cast<const uint8_t*>(files[i]) + lay[i].data_start, (size_t)sg.data_bytes,
                          hipMemcpyHostToDevice, s));
  }
  BP_HIP(hipMemcpyAsync(h->ad.segs, segs.data(), segs.size() * sizeof(AdpcmSeg), hipMemcpyHostToDevice, s));
  launch_adpcm_decode(lay[0].codec, h->ad.file, h->ad.segs, (int)segs.size(), chains, h->ad.pcm, s);
  BP_HIP(hipGetLastError());
  return BP_OK;
}

namespace {

// ---- device-side note candidates (note_device.hip): what note decoding needs of a track's maps
// m: device maps of T > 0 frames (note / onset are modified when the parameters set a frequency range, like
// constrain_frequency does).  Outputs: host buffers, complete once the stream has been waited for.
int queue_candidates(bp_handle h, const Maps& m, int64_t T, const bp_note_params* prm, float* note_out, uint8_t* cand_out,
                     int8_t* bend_out, bool* exported_by_kernel) {
  hipStream_t s = h->stream;
  const void* tab = nullptr;
  const double* gauss = nullptr;
  if (int rc = note_tables(h, &tab, &gauss)) return rc;
  uint8_t* d_bits = nullptr;
  int8_t* d_bend = nullptr;
  if (int rc = reserve_candidates(h, T, &d_bits, &d_bend)) return rc;
  void* d_stats = h->nd_tables + kTabBytes + kGaussBytes;
  int lo = 0, hi = 88;
  bp_internal_freq_limits(prm, &lo, &hi);
  const bool want_bends = prm->include_pitch_bends != 0 && bend_out != nullptr;
  if (!h->nd_stats_ready) launch_note_stats_init(d_stats, s);
  h->nd_stats_ready = false;
  launch_note_candidates(m.note, m.onset, m.contour, T, lo, hi, prm->infer_onsets != 0, prm->onset_threshold, tab, gauss,
                         d_stats, d_bits, want_bends ? d_bend : nullptr, s);
  BP_HIP(hipGetLastError());
  return send_candidates(h, m.note, T, d_bits, want_bends ? d_bend : nullptr, note_out, cand_out, bend_out, d_stats,
                         h->nd_stats_host, h->nd_stats_host_dev, 1, exported_by_kernel);
}

// ---- the driver ------------------------------------------------------------------------------------------------------------
// Where the 22.05 kHz signal comes from.  kSamples: `count` samples; kPcm: `count` frames of PCM (downmix + resampling);
// kFlac: a FLAC file of `count` bytes in host memory, decoded on the device, then as kPcm; kFlacPcm: the same decode, the PCM
// left in h->pcm_dev (bp_flac_decode_device); kAdpcm / kAdpcmPcm: the same for an IMA ADPCM file, the PCM in h->ad.pcm;
// kMaps: no signal but `count` rows of maps already made (data: the note map).
enum SourceKind { kSamples, kPcm, kFlac, kFlacPcm, kAdpcm, kAdpcmPcm, kMaps };
struct Source {
  SourceKind kind;
  const void* data;
  int64_t count;
  int mem_kind;                       // where `data` lies
  int format, channels, sample_rate;  // kPcm
  const float *onset, *contour;       // kMaps
  int64_t n;                          // set by check_args: the signal's length (kMaps: rows)
  bp_flac_stream_layout lay;          // set by check_args: kFlac / kFlacPcm
  bp_adpcm_layout ad;                 // set by check_args: kAdpcm / kAdpcmPcm
  std::vector<AdpcmSeg> ad_segs;      // the decode launch's table (read by an asynchronous copy: alive until the wait)
};

// Where the results go.  kSignal: the signal to `signal` (host or device memory after mem_kind; NULL: it stays on the
// device); kHostMaps / kDeviceMaps: the caller's maps; kCandidates: the note candidates (host buffers), the maps stay in
// track_out for bp_track_maps.
enum SinkKind { kSignal, kHostMaps, kDeviceMaps, kCandidates };
struct Sink {
  SinkKind kind;
  Maps maps;
  float* signal;
  int mem_kind;
  const bp_note_params* params;
  float* note_out;
  uint8_t* cand_bits;
  int8_t* bend_map;
  int* status;
};

Sink maps_sink(float* note, float* onset, float* contour, int mem_kind) {
  return Sink{mem_kind == BP_MEM_HOST ? kHostMaps : kDeviceMaps, {note, onset, contour}};
}

// every argument, before anything is queued; src.n, src.lay and *T (rows of the maps) are known afterwards.  Outputs are
// needed only when there are rows to write.
int check_args(bp_handle h, const char* what, Source& src, const Sink& k, int64_t* T) {
  auto invalid = [&](const char* why) {
    h->err = std::string(what) + ": " + why;
    return BP_ERR_INVALID_ARG;
  };
  int rc = BP_OK;
  if (k.kind == kCandidates && (!k.params || !k.status)) return invalid("null params / status");
  if (src.kind == kSamples || src.kind == kMaps) {
    if (src.count < 0 || (src.mem_kind != BP_MEM_HOST && src.mem_kind != BP_MEM_DEVICE))
      return invalid("negative length or unknown mem_kind");
    if (src.count > 0 && (!src.data || (src.kind == kMaps && (!src.onset || !src.contour)))) return invalid("null input pointer");
    src.n = src.count;
  } else if (src.kind == kPcm) {
    if ((rc = check_ingest(h, src.data != nullptr, src.format, src.count, src.channels, src.sample_rate, src.mem_kind))) return rc;
    src.n = resampled_length(src.count, src.sample_rate, h->rate);
  } else if (src.kind == kAdpcm || src.kind == kAdpcmPcm) {
    if ((rc = check_adpcm(h, src.data, (size_t)src.count, &src.ad))) return rc;
    const bp_adpcm_layout& l = src.ad;
    if ((rc = check_ingest(h, true, BP_PCM_S16, l.n_frames, l.channels, l.sample_rate, BP_MEM_DEVICE))) return rc;
    if (src.kind == kAdpcm) src.n = resampled_length(l.n_frames, l.sample_rate, h->rate);
  } else {
    if ((rc = check_flac(h, src.data, (size_t)src.count, &src.lay))) return rc;
    const bp_flac_stream_layout& l = src.lay;
    if (src.kind == kFlac) {
      if ((rc = check_ingest(h, true, flac_format(l), l.n_frames, l.channels, l.sample_rate, BP_MEM_DEVICE))) return rc;
      src.n = resampled_length(l.n_frames, l.sample_rate, h->rate);
    }
  }
  *T = src.kind == kMaps ? src.n : h_frames(h, src.n);
  const bool missing = k.kind == kSignal      ? src.kind == kPcm && src.n > 0 && !k.signal
                       : k.kind == kCandidates ? *T > 0 && (!k.note_out || !k.cand_bits)
                                               : *T > 0 && (!k.maps.note || !k.maps.onset || !k.maps.contour);
  return missing ? invalid("null output pointer") : BP_OK;
}

// the source, the track, the sink: everything a call queues.  kMaps: a private copy of the given maps goes to track_out (the
// frequency limits are applied in place).
int queue_all(bp_handle h, Source& src, const Sink& k, int64_t T, bool* exported_by_kernel) {
  const float* d = static_cast<const float*>(src.data);  // the signal on the device (kFlacPcm: none, the PCM in h->pcm_dev)
  Maps m = k.maps;
  int rc = BP_OK;
  if (src.kind == kSamples && src.mem_kind == BP_MEM_HOST) {
    const float* host = d;
    rc = stage_samples(h, 1, &host, &src.count, src.count, &d);
  } else if (src.kind == kPcm && src.count > 0) {
    rc = queue_ingest(h, src.data, src.format, src.count, src.channels, src.sample_rate, src.mem_kind, &d);
  } else if ((src.kind == kFlac || src.kind == kFlacPcm) && !(rc = queue_flac(h, src.data, (size_t)src.count, src.lay)) &&
             src.kind == kFlac) {
    rc = queue_ingest(h, h->pcm_dev, flac_format(src.lay), src.lay.n_frames, src.lay.channels, src.lay.sample_rate,
                      BP_MEM_DEVICE, &d);
  } else if (src.kind == kAdpcm || src.kind == kAdpcmPcm) {
    int64_t pcm_off = 0;
    if (!(rc = queue_adpcm(h, 1, &src.data, &src.ad, src.ad_segs, &pcm_off)) && src.kind == kAdpcm && src.ad.n_frames > 0)
      rc = queue_ingest(h, h->ad.pcm, BP_PCM_S16, src.ad.n_frames, src.ad.channels, src.ad.sample_rate, BP_MEM_DEVICE, &d);
  } else if (src.kind == kMaps) {
    rc = take_given_maps(h, d, src.onset, src.contour, T, src.mem_kind, &m);
  }
  if (rc) return rc;
  switch (k.kind) {
    case kSignal:
      if (k.signal && src.n > 0)
        BP_HIP(hipMemcpyAsync(k.signal, d, (size_t)src.n * 4,
                              k.mem_kind == BP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
      return BP_OK;
    case kHostMaps:
    case kDeviceMaps:
      if (h_windows(h, src.n) == 0) return BP_OK;
      if (k.kind == kHostMaps && (rc = take_track_out(h, T, &m))) return rc;
      if ((rc = tracks_core(h, 1, &d, &src.n, &m))) return rc;
      return k.kind == kHostMaps && T > 0 ? copy_maps(h, k.maps, m, T, hipMemcpyDeviceToHost) : BP_OK;
    case kCandidates:
      if (T == 0) return BP_OK;
      if (src.kind != kMaps && ((rc = take_track_out(h, T, &m)) || (rc = tracks_core(h, 1, &d, &src.n, &m)))) return rc;
      return queue_candidates(h, m, T, k.params, k.note_out, k.cand_bits, k.bend_map, exported_by_kernel);
  }
  return BP_OK;
}

int run_track(bp_handle h, const char* what, Source src, const Sink& k, bp_flac_stream_layout* lay = nullptr,
              bp_adpcm_layout* ad = nullptr) {
  if (!h) return BP_ERR_INVALID_ARG;
  int64_t T = 0;
  int rc = check_args(h, what, src, k, &T);
  if (rc) return rc;
  const bool flac = src.kind == kFlac || src.kind == kFlacPcm;
  if (lay) *lay = src.lay;
  if (ad) *ad = src.ad;
  if (k.kind == kCandidates) *k.status = 0;
  // nothing to queue and nothing to wait for (a candidates call waits for the stream whatever the length)
  if (!flac && src.n == 0 && k.kind != kCandidates && !(src.kind == kAdpcmPcm && src.ad.n_frames > 0)) return BP_OK;
  BP_HIP(hipSetDevice(h->device));
  bool exported_by_kernel = false;
  if ((rc = finish(h, queue_all(h, src, k, T, &exported_by_kernel)))) return rc;
  if (k.kind == kCandidates && T > 0) {
    if (exported_by_kernel) h->nd_stats_ready = true;  // only now: the export kernel, which re-initialises the record, has run
    // numpy's rules for NaN cells, and an onset threshold <= 0 (every cell that is not a peak qualifies), need the maps
    // themselves: the host decoder takes over (bp_track_maps + bp_notes_decode)
    const int nan_flag = h->nd_stats_host[1];
    if (nan_flag || !(k.params->onset_threshold > 0.0)) *k.status = 1;
    if (src.kind != kMaps) h->maps_rows = T;  // the track's maps stay in track_out for bp_track_maps
  }
  return flac ? flac_device_verdict(h) : BP_OK;
}

// bp_infer_tracks: host tracks are staged one after the other, their maps come back from one block
int queue_tracks(bp_handle h, int64_t n_tracks, const float* const* samples, const int64_t* n_samples, float* const* note,
                 float* const* onset, float* const* contour, int mem_kind, int64_t total_samples, int64_t total_rows) {
  // device views of every track's input and outputs
  std::vector<const float*> d_in(samples, samples + n_tracks);
  std::vector<Maps> d_out(n_tracks);
  Maps all;
  int rc = BP_OK;
  if (mem_kind == BP_MEM_HOST &&
      ((rc = take_track_out(h, total_rows, &all)) || (rc = stage_samples(h, n_tracks, samples, n_samples, total_samples, d_in.data()))))
    return rc;
  for (int64_t t = 0, ro = 0; t < n_tracks; ro += h_frames(h, n_samples[t++]))
    d_out[t] = mem_kind == BP_MEM_HOST ? maps_at(all.note + ro * kMapsRow, h_frames(h, n_samples[t])) : Maps{note[t], onset[t], contour[t]};
  if ((rc = tracks_core(h, n_tracks, d_in.data(), n_samples, d_out.data()))) return rc;
  for (int64_t t = 0; t < n_tracks && mem_kind == BP_MEM_HOST; ++t) {
    const int64_t T = h_frames(h, n_samples[t]);
    if (T > 0 && (rc = copy_maps(h, {note[t], onset[t], contour[t]}, d_out[t], T, hipMemcpyDeviceToHost))) return rc;
  }
  return BP_OK;
}

}  // namespace

int bp::note_tables(bp_handle h, const void** tab, const double** gauss) {
  if (!h->nd_tables) {
    std::vector<uint8_t> raw(kTabBytes + kGaussBytes + kStatsBytes, 0);
    bp_internal_bend_tables(reinterpret_cast<int32_t*>(raw.data()), reinterpret_cast<double*>(raw.data() + kTabBytes));
    BP_HIP(h->nd_stats_host.alloc(kStatsBytes / sizeof(int)));
    BP_HIP(hipHostGetDevicePointer(&h->nd_stats_host_dev, h->nd_stats_host, 0));
    BP_HIP(h->nd_tables.upload(raw.data(), raw.size()));
    h->workspace_bytes += raw.size();  // the one table bp_get_info reports that bp_create does not make
  }
  if (tab) *tab = h->nd_tables;
  if (gauss) *gauss = reinterpret_cast<const double*>(h->nd_tables + kTabBytes);
  return BP_OK;
}

extern "C" {

int64_t bp_handle_track_n_windows(bp_handle h, int64_t n_samples) { return h ? h_windows(h, n_samples) : 0; }
int64_t bp_handle_track_n_frames(bp_handle h, int64_t n_samples) { return h ? h_frames(h, n_samples) : 0; }
int64_t bp_handle_window_samples(bp_handle h) { return h ? h->win_len : 0; }
int bp_handle_sample_rate(bp_handle h) { return h ? h->rate : 0; }
int64_t bp_handle_resampled_length(bp_handle h, int64_t n_frames, int sample_rate) { return h ? resampled_length(n_frames, sample_rate, h->rate) : 0; }

int64_t bp_track_n_windows(int64_t n_samples) { return n_windows_of(n_samples, BP_HOP_SIZE, BP_OVERLAP_LEN / 2); }
int64_t bp_track_n_frames(int64_t n_samples) { return n_frames_of(n_samples, BP_HOP_SIZE, BP_OVERLAP_LEN / 2); }
int64_t bp_resampled_length(int64_t n_frames, int sample_rate) { return resampled_length(n_frames, sample_rate, BP_AUDIO_SAMPLE_RATE); }

int bp_infer_track(bp_handle h, const float* samples, int64_t n_samples, float* note, float* onset,
                   float* contour, int mem_kind) {
  return run_track(h, "bp_infer_track", Source{kSamples, samples, n_samples, mem_kind}, maps_sink(note, onset, contour, mem_kind));
}

int bp_infer_tracks(bp_handle h, int64_t n_tracks, const float* const* samples, const int64_t* n_samples,
                    float* const* note, float* const* onset, float* const* contour, int mem_kind) {
  if (!h) return BP_ERR_INVALID_ARG;
  if (n_tracks < 0 || (mem_kind != BP_MEM_HOST && mem_kind != BP_MEM_DEVICE) ||
      (n_tracks > 0 && (!samples || !n_samples || !note || !onset || !contour))) {
    h->err = "bp_infer_tracks: bad argument";
    return BP_ERR_INVALID_ARG;
  }
  int64_t total_samples = 0, total_rows = 0;
  for (int64_t t = 0; t < n_tracks; ++t) {
    const int64_t T = h_frames(h, n_samples[t]);
    if (n_samples[t] < 0 || (n_samples[t] > 0 && !samples[t]) || (T > 0 && (!note[t] || !onset[t] || !contour[t]))) {
      h->err = "bp_infer_tracks: negative length, null samples or null output pointer";
      return BP_ERR_INVALID_ARG;
    }
    total_samples += n_samples[t];
    total_rows += T;
  }
  if (total_samples == 0) return BP_OK;
  BP_HIP(hipSetDevice(h->device));
  return finish(h, queue_tracks(h, n_tracks, samples, n_samples, note, onset, contour, mem_kind, total_samples, total_rows));
}

int bp_resample(bp_handle h, const float* pcm, int64_t n_frames, int channels, int sample_rate, float* out22k,
                int mem_kind) {
  return run_track(h, "bp_resample", Source{kPcm, pcm, n_frames, mem_kind, BP_PCM_F32, channels, sample_rate},
                   Sink{kSignal, {}, out22k, mem_kind});
}

int bp_infer_pcm_raw(bp_handle h, const void* pcm, int format, int64_t n_frames, int channels, int sample_rate, float* note,
                     float* onset, float* contour, int mem_kind) {
  return run_track(h, "bp_infer_pcm", Source{kPcm, pcm, n_frames, mem_kind, format, channels, sample_rate},
                   maps_sink(note, onset, contour, mem_kind));
}

int bp_infer_pcm(bp_handle h, const float* pcm, int64_t n_frames, int channels, int sample_rate, float* note,
                 float* onset, float* contour, int mem_kind) {
  return bp_infer_pcm_raw(h, pcm, BP_PCM_F32, n_frames, channels, sample_rate, note, onset, contour, mem_kind);
}

int bp_note_candidates(bp_handle h, const float* note, const float* onset, const float* contour, int64_t n_frames,
                       const bp_note_params* params, int mem_kind, float* note_out, uint8_t* cand_bits, int8_t* bend_map,
                       int* status) {
  return run_track(h, "bp_note_candidates", Source{kMaps, note, n_frames, mem_kind, 0, 0, 0, onset, contour},
                   Sink{kCandidates, {}, nullptr, 0, params, note_out, cand_bits, bend_map, status});
}

int bp_infer_pcm_raw_candidates(bp_handle h, const void* pcm, int format, int64_t n_frames, int channels, int sample_rate,
                                const bp_note_params* params, float* note_out, uint8_t* cand_bits, int8_t* bend_map,
                                int* status) {
  return run_track(h, "bp_infer_pcm_raw_candidates", Source{kPcm, pcm, n_frames, BP_MEM_HOST, format, channels, sample_rate},
                   Sink{kCandidates, {}, nullptr, 0, params, note_out, cand_bits, bend_map, status});
}

int bp_track_maps(bp_handle h, int64_t n_frames, float* note, float* onset, float* contour, int mem_kind) {
  if (!h) return BP_ERR_INVALID_ARG;
  if (n_frames <= 0 || n_frames != h->maps_rows || !note || !onset || !contour ||
      (mem_kind != BP_MEM_HOST && mem_kind != BP_MEM_DEVICE)) {
    h->err = "bp_track_maps: no maps of that many rows are left on the device (call it right after a *_candidates call of "
             "this handle, with that call's row count) or a null / unknown destination";
    return BP_ERR_INVALID_ARG;
  }
  BP_HIP(hipSetDevice(h->device));
  const Maps m = maps_at(h->track_out, n_frames);
  return finish(h, copy_maps(h, {note, onset, contour}, m, n_frames,
                             mem_kind == BP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
}

int bp_flac_decode_device(bp_handle h, const void* file, size_t nbytes, int32_t* pcm, int64_t capacity_frames, int64_t* n_frames) {
  if (!h || !n_frames) return BP_ERR_INVALID_ARG;
  bp_flac_stream_layout lay;
  if (int rc = run_track(h, "bp_flac_decode_device", Source{kFlacPcm, file, (int64_t)nbytes}, Sink{kSignal}, &lay)) return rc;
  *n_frames = lay.n_frames;
  if (!pcm) return BP_OK;
  if (capacity_frames < lay.n_frames) {
    h->err = "bp_flac_decode_device: the output buffer is too small";
    return BP_ERR_INVALID_ARG;
  }
  const int64_t n = lay.n_frames * lay.channels;
  const bool wide = flac_format(lay) == BP_PCM_S32;
  std::vector<int16_t> tmp(wide ? 0 : (size_t)n);
  void* home = wide ? (void*)pcm : tmp.data();
  BP_HIP(hipMemcpy(home, h->pcm_dev, (size_t)n * (wide ? 4 : 2), hipMemcpyDeviceToHost));
  flac_pcm_to_int32(home, wide, (wide ? 32 : 16) - lay.bits_per_sample, n, pcm);
  return BP_OK;
}

int bp_infer_flac(bp_handle h, const void* file, size_t nbytes, float* note, float* onset, float* contour, int mem_kind) {
  return run_track(h, "bp_infer_flac", Source{kFlac, file, (int64_t)nbytes}, maps_sink(note, onset, contour, mem_kind));
}

int bp_infer_flac_candidates(bp_handle h, const void* file, size_t nbytes, const bp_note_params* params, float* note_out,
                             uint8_t* cand_bits, int8_t* bend_map, int* status) {
  return run_track(h, "bp_infer_flac_candidates", Source{kFlac, file, (int64_t)nbytes},
                   Sink{kCandidates, {}, nullptr, 0, params, note_out, cand_bits, bend_map, status});
}

// ---- IMA ADPCM files (include/basic_pitch_amd_adpcm.h) -------------------------------------------------------------------------
int bp_adpcm_decode_device(bp_handle h, const void* file, size_t nbytes, int16_t* pcm, int64_t max_frames, int64_t* n_frames) {
  if (!h || !n_frames) return BP_ERR_INVALID_ARG;
  const char* what = "bp_adpcm_decode_device";
  // (the layout twice: the room is an argument, and every argument is checked before anything is queued)
  bp_adpcm_layout lay;
  if (int rc = check_adpcm(h, file, nbytes, &lay)) return rc;
  *n_frames = lay.n_frames;
  if (pcm && max_frames < lay.n_frames) {
    h->err = std::string(what) + ": the output buffer is too small";
    return BP_ERR_INVALID_ARG;
  }
  if (int rc = run_track(h, what, Source{kAdpcmPcm, file, (int64_t)nbytes}, Sink{kSignal}, nullptr, &lay)) return rc;
  if (!pcm || lay.n_frames == 0) return BP_OK;
  BP_HIP(hipMemcpy(pcm, h->ad.pcm, (size_t)(lay.n_frames * lay.channels) * sizeof(int16_t), hipMemcpyDeviceToHost));
  return BP_OK;
}

int bp_infer_adpcm(bp_handle h, const void* file, size_t nbytes, float* note, float* onset, float* contour, int mem_kind) {
  return run_track(h, "bp_infer_adpcm", Source{kAdpcm, file, (int64_t)nbytes}, maps_sink(note, onset, contour, mem_kind));
}

int bp_infer_adpcm_candidates(bp_handle h, const void* file, size_t nbytes, const bp_note_params* params, float* note_out,
                              uint8_t* cand_bits, int8_t* bend_map, int* status) {
  return run_track(h, "bp_infer_adpcm_candidates", Source{kAdpcm, file, (int64_t)nbytes},
                   Sink{kCandidates, {}, nullptr, 0, params, note_out, cand_bits, bend_map, status});
}

}  // extern "C"
