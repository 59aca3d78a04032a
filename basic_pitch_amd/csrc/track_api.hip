// C ABI of the track family (include/basic_pitch_amd.h): whole signals -> un-overlapped posteriorgrams on the device — from
// host or device samples, raw PCM (downmix + resampling), or a FLAC file's bytes decoded on the device — and the device-side
// note candidates of those maps.
//
// Every entry point is a source, the track and a sink on one driver (run_track):
//   validate everything -> queue the source -> tracks_core -> queue the sink -> wait -> the FLAC decoder's verdict.
// Nothing is queued before every argument has been checked, and a call that fails after queuing work returns only once the
// handle's stream has drained (finish): the caller may reuse its buffers as soon as any call returns.
//
// The staging buffers of these calls are the handle's typed, grow-only buffers (device_buffer.h): a call reserves what it
// needs before it queues work on them, and nothing here frees by hand.
#include <algorithm>
#include <cstring>

#include "../../include/basic_pitch_amd_flac_clips.h"
#include "bp_context.h"

using namespace bp;

extern "C" void bp_internal_bend_tables(int32_t* tab, double* gauss);
extern "C" void bp_internal_freq_limits(const bp_note_params* prm, int* lo, int* hi);
extern "C" double bp_internal_frame_time(int64_t frame);
extern "C" int bp_internal_flac_device_supported(const bp_flac_stream_layout* lay, size_t nbytes);

// ---- what the streaming sessions (stream_api.hip) share with this file (declared in bp_context.h): the end of a call, the
// argument domain of raw PCM, the resampling filter's builder, the copies of the three maps
namespace bp {

// The end of a call that has queued work: the wait, or on the first error the drained stream (its own status ignored), so
// that no copy from or into a caller's buffer is still in flight when the call returns.
int finish(bp_handle h, int rc) {
  if (rc == BP_OK) rc = wait_stream(h);
  if (rc != BP_OK) (void)hipStreamSynchronize(h->stream);
  return rc;
}

int pcm_width(int format) {
  static const int width[] = {4, 2, 3, 4, 1, 8};  // BP_PCM_F32, S16, S24, S32, U8, F64
  return format >= BP_PCM_F32 && format <= BP_PCM_F64 ? width[format] : 0;
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

// ---- the tracker behind any dense half (declared in bp_context.h): the clips calls here, bp_streams_events in stream_api.hip
static bool seg_bends(const EventsJob& job, int64_t c) {
  return job.seg ? job.seg[c].bends != 0 : job.prm->include_pitch_bends != 0;
}

int events_reserve(bp_handle h, const EventsJob& job, EventsPlan* plan) {
  const int64_t n = job.n, T = job.offs[n];
  plan->ev_first.assign((size_t)n + 1, 0);
  plan->max_rows = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t rows = job.offs[i + 1] - job.offs[i];
    plan->ev_first[(size_t)i + 1] =
        plan->ev_first[(size_t)i] + note_track_capacity(rows, job.seg ? job.seg[i].min_note_len : job.prm->min_note_len);
    plan->max_rows = std::max(plan->max_rows, rows);
  }
  const int64_t pool_events = plan->ev_first[(size_t)n], n_meta = 3 * n + 2;
  const bool scratch = plan->max_rows > kNoteTrackLdsRows || job.form == kNoteTrackFormScratch;
  BP_HIP(h->ev_first.reserve((size_t)n + 1));
  BP_HIP(h->ev_meta.reserve((size_t)n_meta));
  BP_HIP(h->ev_counts.reserve((size_t)n * 16));
  BP_HIP(h->ev_pool.reserve((size_t)pool_events * 16));
  BP_HIP(h->ev_out.reserve((size_t)pool_events * 16));
  BP_HIP(h->bd_pool.reserve((size_t)T * 88));
  BP_HIP(h->bd_out.reserve((size_t)T * 88));
  if (scratch) BP_HIP(h->ev_scratch.reserve((size_t)note_track_scratch_floats(T)));
  if (job.seg) BP_HIP(h->ev_seg.reserve((size_t)n * sizeof(NoteTrackSeg)));
  BP_HIP(h->ev_home.reserve((size_t)n_meta));  // page-locked: the offsets and status come home first
  return BP_OK;
}

int events_queue(bp_handle h, const EventsJob& job, const EventsPlan& plan, const TrackInputs& in) {
  hipStream_t s = h->stream;
  const int64_t n = job.n;
  BP_HIP(hipMemcpyAsync(h->ev_first, plan.ev_first.data(), (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  if (job.seg) {
    BP_HIP(hipMemcpyAsync(h->ev_seg, job.seg, (size_t)n * sizeof(NoteTrackSeg), hipMemcpyHostToDevice, s));
    BP_HIP(launch_note_track_segs(in.note, in.bits, in.bend, in.offs, h->ev_first, in.stats, h->ev_seg.as<NoteTrackSeg>(), n,
                                  plan.max_rows, job.form, h->ev_scratch, h->ev_pool, h->bd_pool, h->ev_counts, h->ev_meta, h->ev_out,
                                  h->bd_out, s));
  } else {
    const bp_note_params* prm = job.prm;
    BP_HIP(launch_note_track(in.note, in.bits, in.bend, in.offs, h->ev_first, in.stats, n, plan.max_rows, prm->frame_threshold,
                             prm->energy_tol, prm->min_note_len, prm->melodia_trick != 0, h->ev_scratch, h->ev_pool, h->bd_pool,
                             h->ev_counts, h->ev_meta, h->ev_out, h->bd_out, s));
  }
  BP_HIP(hipMemcpyAsync(h->ev_home, h->ev_meta, (size_t)(3 * n + 2) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  return BP_OK;
}

int events_home(bp_handle h, const EventsJob& job, const EventsSink& out, bool* device_error) {
  hipStream_t s = h->stream;
  const int64_t n = job.n, n_meta = 3 * n + 2;
  const int64_t* meta = h->ev_home;
  const int64_t n_events = meta[n], n_bends = meta[2 * n + 1];
  for (int64_t i = 0; i <= n; ++i) out.event_offsets[i] = meta[i];
  for (int64_t i = 0; i < n; ++i) out.status[i] = (int)meta[2 * n + 2 + i];
  if (n_events > out.max_events || n_bends > out.max_bends) {
    h->err = std::string(job.what) + ": output buffers too small: " + std::to_string(n_events) + " events and " +
             std::to_string(n_bends) + " bends are needed (event_offsets[" + job.count_name + "] holds the events)";
    return BP_ERR_INVALID_ARG;
  }
  if (n_events == 0) return BP_OK;
  struct Raw {
    int32_t start, end, pitch;
    float amp;
  };
  Raw* raw = nullptr;
  int8_t* raw_bends = nullptr;
  auto home = [&]() -> int {
    // the stream has drained and the offsets are out of the block: it may grow for the events and, behind them, the bends
    BP_HIP(h->ev_home.reserve((size_t)std::max(n_meta, 2 * n_events + (n_bends + 7) / 8)));
    raw = reinterpret_cast<Raw*>(static_cast<int64_t*>(h->ev_home));
    raw_bends = reinterpret_cast<int8_t*>(raw + n_events);
    BP_HIP(hipMemcpyAsync(raw, h->ev_out, (size_t)n_events * sizeof(Raw), hipMemcpyDeviceToHost, s));
    if (n_bends) BP_HIP(hipMemcpyAsync(raw_bends, h->bd_out, (size_t)n_bends, hipMemcpyDeviceToHost, s));
    return BP_OK;
  };
  if (int rc = finish(h, home())) {
    if (device_error) *device_error = true;
    return rc;
  }
  for (int64_t i = 0; i < n_bends; ++i) out.bends[i] = (int32_t)raw_bends[i];
  int64_t bo = 0;
  for (int64_t c = 0; c < n; ++c) {
    const int64_t first = job.first_frame ? job.first_frame[c] : 0;
    const bool want_bends = seg_bends(job, c);
    for (int64_t e = out.event_offsets[c]; e < out.event_offsets[c + 1]; ++e) {
      const Raw& r = raw[e];
      bp_note_event& ev = out.events[e];
      std::memset(&ev, 0, sizeof ev);  // reserved fields and padding
      ev.start_frame = (int32_t)(first + r.start), ev.end_frame = (int32_t)(first + r.end);
      ev.start_s = bp_internal_frame_time(first + r.start), ev.end_s = bp_internal_frame_time(first + r.end);
      ev.pitch_midi = r.pitch;
      ev.amplitude = r.amp;
      ev.bend_offset = bo;
      ev.n_bends = want_bends ? r.end - r.start : 0;
      bo += ev.n_bends;
    }
  }
  return BP_OK;
}

}  // namespace bp

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

int64_t resampled_length(int64_t n_frames, int sample_rate, int rate) {
  return n_frames <= 0 || sample_rate <= 0 ? 0 : (n_frames * (int64_t)rate + sample_rate - 1) / sample_rate;
}

int64_t h_windows(bp_handle h, int64_t n) { return n_windows_of(n, h->hop, h->lead); }
int64_t h_frames(bp_handle h, int64_t n) { return n_frames_of(n, h->hop, h->lead); }

// The only way to h->track_out: grown for `rows` rows of maps.  Whatever a *_candidates call left there for bp_track_maps
// is gone from then on.
int take_track_out(bp_handle h, int64_t rows, Maps* m) {
  h->maps_rows = 0;
  BP_HIP(h->track_out.reserve((size_t)(rows * kMapsRow)));
  *m = maps_at(h->track_out, rows);
  return BP_OK;
}

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

int flac_format(const bp_flac_stream_layout& lay) { return lay.bits_per_sample > 16 ? BP_PCM_S32 : BP_PCM_S16; }

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

// ---- device-side note candidates (note_device.hip): what note decoding needs of a track's maps
constexpr size_t kTabBytes = 88 * 16, kGaussBytes = 51 * 8, kStatsBytes = 16;

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

// The candidates of the maps of n_clips clips that lie one after the other in m, clip c at rows [offs[c], offs[c + 1]) of
// offs[n_clips] = T > 0 rows, each clip decoded as its own whole track.  offs (host) must stay as it is until the stream has
// been waited for.  The device half: *d_bits / *d_bend (null without want_bends) are where the bitmap and the bends of all
// rows lie, the clips' records are in h->clip_stats and their row offsets in h->clip_rows; nothing goes home.
int queue_clips_dense(bp_handle h, const Maps& m, int64_t n_clips, const int64_t* offs, const bp_note_params* prm, bool want_bends,
                      uint8_t** d_bits_out, int8_t** d_bend_out) {
  hipStream_t s = h->stream;
  const int64_t T = offs[n_clips];
  const void* tab = nullptr;
  const double* gauss = nullptr;
  if (int rc = note_tables(h, &tab, &gauss)) return rc;
  uint8_t* d_bits = nullptr;
  int8_t* d_bend = nullptr;
  if (int rc = reserve_candidates(h, T, &d_bits, &d_bend)) return rc;
  if ((size_t)n_clips * kStatsBytes > h->clip_stats.capacity()) h->clip_stats_ready = 0;  // a new block: nothing initialised
  BP_HIP(h->clip_stats.reserve((size_t)n_clips * kStatsBytes));
  BP_HIP(h->clip_rows.reserve((size_t)n_clips + 1));
  BP_HIP(hipMemcpyAsync(h->clip_rows, offs, (size_t)(n_clips + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  int lo = 0, hi = 88;
  bp_internal_freq_limits(prm, &lo, &hi);
  if (h->clip_stats_ready < n_clips) launch_clips_stats_init(h->clip_stats, n_clips, s);
  h->clip_stats_ready = 0;
  launch_clips_candidates(m.note, m.onset, m.contour, h->clip_rows, n_clips, T, lo, hi, prm->infer_onsets != 0,
                          prm->onset_threshold, tab, gauss, h->clip_stats, d_bits, want_bends ? d_bend : nullptr, s);
  BP_HIP(hipGetLastError());
  *d_bits_out = d_bits;
  *d_bend_out = want_bends ? d_bend : nullptr;
  return BP_OK;
}

// ... and home: the note rows, the bitmap and the bends to host buffers, clip c's record as h->clip_stats_host[4 c ...]
int queue_clips_candidates(bp_handle h, const Maps& m, int64_t n_clips, const int64_t* offs, const bp_note_params* prm,
                           float* note_out, uint8_t* cand_out, int8_t* bend_out, bool* exported_by_kernel) {
  uint8_t* d_bits = nullptr;
  int8_t* d_bend = nullptr;
  // the page-locked copy of the records, before anything is queued
  BP_HIP(h->clip_stats_host.reserve((size_t)n_clips * (kStatsBytes / sizeof(int))));
  void* stats_host_dev = nullptr;
  BP_HIP(hipHostGetDevicePointer(&stats_host_dev, h->clip_stats_host, 0));
  if (int rc = queue_clips_dense(h, m, n_clips, offs, prm, prm->include_pitch_bends != 0 && bend_out != nullptr, &d_bits, &d_bend))
    return rc;
  return send_candidates(h, m.note, offs[n_clips], d_bits, d_bend, note_out, cand_out, bend_out, h->clip_stats, h->clip_stats_host,
                         stats_host_dev, n_clips, exported_by_kernel);
}

// ---- the driver ------------------------------------------------------------------------------------------------------------
// Where the 22.05 kHz signal comes from.  kSamples: `count` samples; kPcm: `count` frames of PCM (downmix + resampling);
// kFlac: a FLAC file of `count` bytes in host memory, decoded on the device, then as kPcm; kFlacPcm: the same decode, the PCM
// left in h->pcm_dev (bp_flac_decode_device); kMaps: no signal but `count` rows of maps already made (data: the note map).
enum SourceKind { kSamples, kPcm, kFlac, kFlacPcm, kMaps };
struct Source {
  SourceKind kind;
  const void* data;
  int64_t count;
  int mem_kind;                       // where `data` lies
  int format, channels, sample_rate;  // kPcm
  const float *onset, *contour;       // kMaps
  int64_t n;                          // set by check_args: the signal's length (kMaps: rows)
  bp_flac_stream_layout lay;          // set by check_args: kFlac / kFlacPcm
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
int queue_all(bp_handle h, const Source& src, const Sink& k, int64_t T, bool* exported_by_kernel) {
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
  } else if (src.kind == kMaps && !(rc = take_track_out(h, T, &m)) && T > 0) {
    const Maps given{const_cast<float*>(d), const_cast<float*>(src.onset), const_cast<float*>(src.contour)};  // only read
    rc = copy_maps(h, m, given, T, src.mem_kind == BP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice);
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

int run_track(bp_handle h, const char* what, Source src, const Sink& k, bp_flac_stream_layout* lay = nullptr) {
  if (!h) return BP_ERR_INVALID_ARG;
  int64_t T = 0;
  int rc = check_args(h, what, src, k, &T);
  if (rc) return rc;
  const bool flac = src.kind == kFlac || src.kind == kFlacPcm;
  if (lay) *lay = src.lay;
  if (k.kind == kCandidates) *k.status = 0;
  // nothing to queue and nothing to wait for (a candidates call waits for the stream whatever the length)
  if (!flac && src.n == 0 && k.kind != kCandidates) return BP_OK;
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

// ---- many clips in one call (include/basic_pitch_amd_clips.h) -------------------------------------------------------------
// Every argument of every clip (check_ingest; with_pcm: the samples are needed too), before anything is queued: n_model[i] =
// clip i's samples at the handle's rate, offsets[i] = the rows of the clips before it, offsets[n_clips] = all rows.
int check_clips(bp_handle h, const char* what, int64_t n_clips, const bp_clip* clips, int sample_rate, int mem_kind, bool with_pcm,
                int64_t* n_model, int64_t* offsets) {
  if (n_clips < 0 || (n_clips > 0 && !clips) || !offsets) {
    h->err = std::string(what) + ": negative n_clips, null clips or null offsets";
    return BP_ERR_INVALID_ARG;
  }
  offsets[0] = 0;
  for (int64_t i = 0; i < n_clips; ++i) {
    const bp_clip& c = clips[i];
    if (int rc = check_ingest(h, !with_pcm || c.pcm != nullptr, c.format, c.n_frames, c.channels, sample_rate, mem_kind)) {
      h->err = std::string(what) + ": clip " + std::to_string(i) + ": " + h->err;
      return rc;
    }
    const int64_t n = resampled_length(c.n_frames, sample_rate, h->rate);
    if (n_model) n_model[i] = n;
    offsets[i + 1] = offsets[i] + h_frames(h, n);
  }
  return BP_OK;
}

// The handle's cached filter becomes that of sample_rate (queue_ingest's cache); a ratio whose taps the one-shot path
// evaluates in the kernel is refused and leaves the cache as it was.  Nothing is queued: the table goes up with a plain copy.
int clips_filter(bp_handle h, const char* what, int sample_rate) {
  if (h->taps_rate != sample_rate) {
    ResamplePlan pl{};
    DeviceBuffer<double> dev;
    const int rc = upload_filter(h, sample_rate, true, &pl, &dev);
    if (rc != BP_OK && rc != BP_ERR_UNSUPPORTED) return rc;
    if (rc == BP_OK) {
      h->taps_rate = 0;
      h->taps_dev = std::move(dev);
      h->plan = pl;
      h->taps_rate = sample_rate;
      return BP_OK;
    }
  } else if (!h->plan.direct) {
    return BP_OK;
  }
  h->err = std::string(what) + ": " + std::to_string(sample_rate) + " Hz -> " + std::to_string(h->rate) +
           " Hz needs a filter whose taps the one-shot calls evaluate in the kernel; such ratios are not taken in batches";
  return BP_ERR_UNSUPPORTED;
}

// Batched ingest: the clips' PCM to the device (host clips one after the other in h->pcm_dev), ONE downmix launch and ONE
// resampling launch for all of them; d_in[i] = clip i's signal at the handle's rate (n_model[i] samples).  `tab` (n_clips
// records, filled here) must stay as it is until the stream has been waited for.
int queue_clips_ingest(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int mem_kind, const int64_t* n_model,
                       ClipDesc* tab, const float** d_in) {
  hipStream_t s = h->stream;
  auto up = [](int64_t v, int64_t a) { return (v + a - 1) / a * a; };
  // offsets of every clip in the three staging buffers (bytes of PCM 16-byte aligned; floats 4-float aligned)
  int64_t pcm_bytes = 0, mono_floats = 0, out_floats = 0, mono_blocks = 0, out_blocks = 0;
  std::vector<int64_t> pcm_off(n_clips), mono_off(n_clips, -1), out_off(n_clips, -1);
  for (int64_t i = 0; i < n_clips; ++i) {
    const bp_clip& c = clips[i];
    if (c.n_frames == 0) continue;
    pcm_off[i] = pcm_bytes;
    if (mem_kind == BP_MEM_HOST) pcm_bytes += up(c.n_frames * c.channels * pcm_width(c.format), 16);
    if (c.channels > 1 || c.format != BP_PCM_F32) mono_off[i] = mono_floats, mono_floats += up(c.n_frames, 4);
    if (sample_rate != h->rate) out_off[i] = out_floats, out_floats += up(n_model[i], 4);
  }
  if (pcm_bytes) BP_HIP(h->pcm_dev.reserve((size_t)pcm_bytes));
  if (mono_floats) BP_HIP(h->mono_dev.reserve((size_t)mono_floats));
  if (out_floats) BP_HIP(h->res_dev.reserve((size_t)out_floats));
  BP_HIP(h->clip_tab.reserve((size_t)n_clips));
  for (int64_t i = 0; i < n_clips; ++i) {
    const bp_clip& c = clips[i];
    ClipDesc& d = tab[i];
    d = ClipDesc{nullptr, nullptr, nullptr, c.n_frames, n_model[i], mono_blocks, out_blocks, c.format, c.channels};
    d_in[i] = nullptr;
    if (c.n_frames == 0) continue;
    d.src = c.pcm;
    if (mem_kind == BP_MEM_HOST) {
      d.src = h->pcm_dev + pcm_off[i];
      BP_HIP(hipMemcpyAsync(h->pcm_dev + pcm_off[i], c.pcm, (size_t)(c.n_frames * c.channels * pcm_width(c.format)),
                            hipMemcpyHostToDevice, s));
    }
    d.mono = static_cast<const float*>(d.src);
    if (mono_off[i] >= 0) d.mono = h->mono_dev + mono_off[i], mono_blocks += (c.n_frames + 1023) / 1024;
    d.out = const_cast<float*>(d.mono);  // already at the handle's rate: windowed where it lies, never written
    if (out_off[i] >= 0) d.out = h->res_dev + out_off[i], out_blocks += (n_model[i] + 255) / 256;
    d_in[i] = d.out;
  }
  if (mono_blocks + out_blocks == 0) return BP_OK;
  BP_HIP(hipMemcpyAsync(h->clip_tab, tab, (size_t)n_clips * sizeof(ClipDesc), hipMemcpyHostToDevice, s));
  launch_clips_downmix(h->clip_tab, n_clips, mono_blocks, s);
  launch_clips_resample(h->clip_tab, n_clips, out_blocks, h->taps_dev, h->plan, s);
  BP_HIP(hipGetLastError());
  return BP_OK;
}

// everything bp_infer_clips_candidates queues: the ingest, the model on the clips' windows packed into full chunks (the maps
// to h->track_out, concatenated by offs), the candidates of every clip.  offs[n_clips] > 0.
int queue_clips_maps(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int mem_kind, const int64_t* n_model,
                     const int64_t* offs, std::vector<ClipDesc>& tab, Maps* all_out) {
  std::vector<const float*> d_in(n_clips);
  std::vector<Maps> d_out(n_clips);
  Maps all;
  int rc = BP_OK;
  if ((rc = take_track_out(h, offs[n_clips], &all)) ||
      (rc = queue_clips_ingest(h, n_clips, clips, sample_rate, mem_kind, n_model, tab.data(), d_in.data())))
    return rc;
  for (int64_t i = 0; i < n_clips; ++i)
    d_out[i] = Maps{all.note + offs[i] * kFreqN, all.onset + offs[i] * kFreqN, all.contour + offs[i] * kFreqC};
  *all_out = all;
  return tracks_core(h, n_clips, d_in.data(), n_model, d_out.data());
}

int queue_clips(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int mem_kind, const int64_t* n_model,
                const int64_t* offs, const bp_note_params* prm, float* note_out, uint8_t* cand_bits, int8_t* bend_map,
                std::vector<ClipDesc>& tab, bool* exported_by_kernel) {
  Maps all;
  if (int rc = queue_clips_maps(h, n_clips, clips, sample_rate, mem_kind, n_model, offs, tab, &all)) return rc;
  return queue_clips_candidates(h, all, n_clips, offs, prm, note_out, cand_bits, bend_map, exported_by_kernel);
}

// after the stream has been waited for: what the clips' records say (a clip without rows: 0)
void clips_status(bp_handle h, int64_t n_clips, const int64_t* offs, const bp_note_params* prm, bool exported_by_kernel, int* status) {
  if (exported_by_kernel) h->clip_stats_ready = n_clips;  // only now: the export kernel, which re-initialises the records, has run
  for (int64_t i = 0; i < n_clips; ++i)
    status[i] = offs[i + 1] > offs[i] && (h->clip_stats_host[4 * i + 1] || !(prm->onset_threshold > 0.0)) ? 1 : 0;
}

// ---- note events of many clips (include/basic_pitch_amd_events.h)
// every argument that is not a clip's, before anything is queued
int check_events(bp_handle h, const char* what, int64_t n_clips, const bp_note_params* prm, const EventsSink& out) {
  auto invalid = [&](const char* why) {
    h->err = std::string(what) + ": " + why;
    return BP_ERR_INVALID_ARG;
  };
  if (n_clips < 0 || !prm || !out.event_offsets || (n_clips > 0 && !out.status)) return invalid("negative n_clips, null params, event_offsets or status");
  if (out.max_events < 0 || out.max_bends < 0 || (out.max_events > 0 && !out.events) || (out.max_bends > 0 && !out.bends))
    return invalid("negative max_events / max_bends, or room without a buffer");
  if (prm->melodia_trick && prm->frame_threshold < 0.0)
    return invalid("a negative frame threshold with the melodia trick never terminates (note_creation.py:452)");
  if (prm->min_note_len < 0) return invalid("negative min_note_len");
  return BP_OK;
}

// The jobs that need no device work: no rows at all, or an onset threshold <= 0 (status 1 for every clip that has rows, as
// bp_infer_clips_candidates reports it).  True: the outputs are complete.
bool events_without_device(int64_t n_clips, const int64_t* offs, const bp_note_params* prm, const EventsSink& out) {
  if (offs[n_clips] > 0 && prm->onset_threshold > 0.0) return false;
  for (int64_t i = 0; i < n_clips; ++i) out.status[i] = offs[i + 1] > offs[i] ? 1 : 0;
  for (int64_t i = 0; i <= n_clips; ++i) out.event_offsets[i] = 0;
  return true;
}

// Behind the maps of the clips (m, in h->track_out; rc: what queuing them returned): the dense half, the tracker, the pack, the
// wait; then the events and bends home (events_home).
int run_events(bp_handle h, const char* what, int rc, const Maps& m, int64_t n, const int64_t* offs, const bp_note_params* prm,
               const EventsSink& out) {
  const EventsJob job{what, "n_clips", n, offs, prm, nullptr, nullptr, kNoteTrackFormAuto};
  EventsPlan plan;
  auto queue = [&]() -> int {
    uint8_t* d_bits = nullptr;
    int8_t* d_bend = nullptr;
    if (int qrc = events_reserve(h, job, &plan)) return qrc;
    if (int qrc = queue_clips_dense(h, m, n, offs, prm, prm->include_pitch_bends != 0, &d_bits, &d_bend)) return qrc;
    return events_queue(h, job, plan, TrackInputs{m.note, d_bits, d_bend, h->clip_rows, h->clip_stats});
  };
  if ((rc = finish(h, rc ? rc : queue()))) return rc;
  return events_home(h, job, out, nullptr);
}

// ---- a job of FLAC clips decoded on the device (include/basic_pitch_amd_flac_clips.h; flac_clips.hip) -------------
// What the host knows of a job before anything is queued: every clip's layout, which clips are left to the host, the rows, and
// where each device clip lies in the job's buffers (the table flac_clips_decode uploads).
struct FlacJob {
  std::vector<bp_flac_stream_layout> lay;
  std::vector<int64_t> dev;            // clip -> its record of `tab`; -1: left to the host
  std::vector<int64_t> n_model, offs;  // samples at the handle's rate; rows before each clip
  std::vector<FdClip> tab;
  int64_t file_bytes = 0, wgs = 0, slots = 0, scratch = 0, pcm_bytes = 0;
};

// sample_rate 0: no rate to agree with and no rows (bp_flac_clips_decode_device)
int plan_flac_clips(bp_handle h, const char* what, int64_t n, const bp_flac_clip* clips, int sample_rate, FlacJob* job) {
  if (n < 0 || (n > 0 && !clips)) {
    h->err = std::string(what) + ": negative n_clips or null clips";
    return BP_ERR_INVALID_ARG;
  }
  auto up16 = [](int64_t v) { return (v + 15) / 16 * 16; };
  job->lay.assign((size_t)n, bp_flac_stream_layout{});
  job->dev.assign((size_t)n, -1);
  job->n_model.assign((size_t)n, 0);
  job->offs.assign((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    const bp_flac_clip& c = clips[i];
    bp_flac_stream_layout& l = job->lay[(size_t)i];
    job->offs[(size_t)i + 1] = job->offs[(size_t)i];
    if (!c.file && c.nbytes) {
      h->err = std::string(what) + ": clip " + std::to_string(i) + ": null file";
      return BP_ERR_INVALID_ARG;
    }
    if (c.nbytes < 42 || bp_flac_layout(c.file, c.nbytes, &l) != BP_OK) continue;
    if (sample_rate && l.sample_rate != sample_rate) {
      h->err = std::string(what) + ": clip " + std::to_string(i) + ": its STREAMINFO says " + std::to_string(l.sample_rate) +
               " Hz, the call " + std::to_string(sample_rate) + " Hz (one rate per call)";
      return BP_ERR_INVALID_ARG;
    }
    if (!bp_internal_flac_device_supported(&l, c.nbytes) || (size_t)l.audio_start >= c.nbytes) continue;
    // scratch is bounded before anything is allocated: a row of max_block samples per frame SLOT, min_block samples a slot
    const int64_t max_frames = (l.n_frames + l.min_block - 1) / l.min_block + 1;
    if (max_frames * l.max_block > 8 * l.n_frames + 2 * (int64_t)l.max_block) continue;
    if (sample_rate) {
      if (int rc = check_ingest(h, true, flac_format(l), l.n_frames, l.channels, sample_rate, BP_MEM_DEVICE)) {
        h->err = std::string(what) + ": clip " + std::to_string(i) + ": " + h->err;
        return rc;
      }
      job->n_model[(size_t)i] = resampled_length(l.n_frames, sample_rate, h->rate);
      job->offs[(size_t)i + 1] += h_frames(h, job->n_model[(size_t)i]);
    }
    const bool wide = flac_format(l) == BP_PCM_S32;
    FdClip k{};
    k.st = FdStream{l.channels, l.bits_per_sample, l.min_block, l.max_block, l.n_frames, (uint32_t)l.audio_start, (uint32_t)c.nbytes};
    k.base = (uint64_t)job->file_bytes, k.first_wg = (uint32_t)job->wgs, k.first_slot = (uint32_t)job->slots;
    k.n_chunks = (int32_t)((c.nbytes - (size_t)l.audio_start + kFdChunkBytes - 1) / kFdChunkBytes), k.max_frames = (int32_t)max_frames;
    k.scratch_off = (uint64_t)job->scratch, k.pcm_off = (uint64_t)job->pcm_bytes;
    k.out_shift = (wide ? 32 : 16) - l.bits_per_sample, k.out_wide = wide ? 1 : 0;
    job->file_bytes += up16((int64_t)c.nbytes + 64);
    job->wgs += k.n_chunks, job->slots += max_frames, job->scratch += max_frames * l.max_block * l.channels;
    job->pcm_bytes += up16(l.n_frames * l.channels * (wide ? 4 : 2));
    if (job->wgs >= ((int64_t)1 << 31) || job->slots >= ((int64_t)1 << 31)) {
      h->err = std::string(what) + ": the job is too large for one call (2^31 scan chunks or frame slots)";
      return BP_ERR_INVALID_ARG;
    }
    job->dev[(size_t)i] = (int64_t)job->tab.size();
    job->tab.push_back(k);
  }
  return BP_OK;
}

// The job's bytes to the device (zeros between and behind the clips), the four decode launches, every clip's error bits and
// frame count on their way to h->fd_status_host; the PCM is being written to h->pcm_dev.  job.tab is not empty.
int queue_flac_clips(bp_handle h, const bp_flac_clip* clips, const FlacJob& job) {
  hipStream_t s = h->stream;
  const int64_t n_dev = (int64_t)job.tab.size();
  BP_HIP(h->fd_status_host.reserve((size_t)(2 * n_dev)));
  BP_HIP(h->fd.file.reserve((size_t)job.file_bytes));
  BP_HIP(h->pcm_dev.reserve((size_t)job.pcm_bytes));
  BP_HIP(hipMemsetAsync(h->fd.file, 0, (size_t)job.file_bytes, s));
  for (size_t i = 0; i < job.dev.size(); ++i)
    if (job.dev[i] >= 0)
      BP_HIP(hipMemcpyAsync(h->fd.file + job.tab[(size_t)job.dev[i]].base, clips[i].file, clips[i].nbytes, hipMemcpyHostToDevice, s));
  if (flac_clips_decode(h->fd, job.tab.data(), n_dev, job.wgs, job.slots, job.scratch, h->pcm_dev, (size_t)job.pcm_bytes, s) != 0) {
    h->err = "FLAC clips on the device: allocation or launch failed";
    (void)hipGetLastError();
    return BP_ERR_HIP;
  }
  BP_HIP(hipMemcpyAsync(h->fd_status_host, h->fd.meta, (size_t)(2 * n_dev) * sizeof(int), hipMemcpyDeviceToHost, s));
  return BP_OK;
}

// the decoded clips as the PCM clips calls take them: device memory, a clip left to the host without frames
std::vector<bp_clip> flac_pcm_clips(bp_handle h, const FlacJob& job) {
  std::vector<bp_clip> out(job.dev.size(), bp_clip{nullptr, 0, BP_PCM_S16, 1});
  for (size_t i = 0; i < job.dev.size(); ++i)
    if (job.dev[i] >= 0)
      out[i] = bp_clip{h->pcm_dev + job.tab[(size_t)job.dev[i]].pcm_off, job.lay[i].n_frames, flac_format(job.lay[i]), job.lay[i].channels};
  return out;
}

// the host-side statuses; with `decoded` (the stream has been waited for) the decoder's verdict on every device clip too
void flac_clips_status(bp_handle h, const FlacJob& job, bool decoded, int* status) {
  for (size_t i = 0; i < job.dev.size(); ++i) {
    if (job.dev[i] < 0) status[i] = BP_CLIP_FLAC_HOST;
    else if (decoded && h->fd_status_host[2 * job.dev[i]] != 0) status[i] = BP_CLIP_FLAC_FAILED;
  }
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

int bp_clips_row_offsets(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int64_t* offsets) {
  if (!h) return BP_ERR_INVALID_ARG;
  return check_clips(h, "bp_clips_row_offsets", n_clips, clips, sample_rate, BP_MEM_HOST, false, nullptr, offsets);
}

int bp_infer_clips_candidates(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                              const bp_note_params* params, float* note_out, uint8_t* cand_bits, int8_t* bend_map, int* status) {
  if (!h) return BP_ERR_INVALID_ARG;
  const char* what = "bp_infer_clips_candidates";
  if (!params || (n_clips > 0 && !status)) {
    h->err = std::string(what) + ": null params / status";
    return BP_ERR_INVALID_ARG;
  }
  std::vector<int64_t> n_model((size_t)(n_clips > 0 ? n_clips : 0)), offs((size_t)(n_clips > 0 ? n_clips : 0) + 1);
  if (int rc = check_clips(h, what, n_clips, clips, sample_rate, pcm_mem_kind, true, n_model.data(), offs.data())) return rc;
  const int64_t total = offs[(size_t)n_clips];
  if (total > 0 && (!note_out || !cand_bits)) {
    h->err = std::string(what) + ": null output pointer";
    return BP_ERR_INVALID_ARG;
  }
  for (int64_t i = 0; i < n_clips; ++i) status[i] = 0;
  if (total == 0) return BP_OK;  // no clip has a row: nothing to queue
  BP_HIP(hipSetDevice(h->device));
  if (sample_rate != h->rate)
    if (int rc = clips_filter(h, what, sample_rate)) return rc;
  std::vector<ClipDesc> tab((size_t)n_clips);
  bool exported_by_kernel = false;
  if (int rc = finish(h, queue_clips(h, n_clips, clips, sample_rate, pcm_mem_kind, n_model.data(), offs.data(), params, note_out,
                                     cand_bits, bend_map, tab, &exported_by_kernel)))
    return rc;
  clips_status(h, n_clips, offs.data(), params, exported_by_kernel, status);
  return BP_OK;
}

// ---- note events of many clips from the device (include/basic_pitch_amd_events.h) --------------------------------------------
int64_t bp_events_capacity(int64_t rows, int min_note_len) { return note_track_capacity(rows, min_note_len); }

int bp_infer_clips_events(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                          const bp_note_params* params, bp_note_event* events, int64_t max_events, int32_t* bends,
                          int64_t max_bends, int64_t* event_offsets, int* status) {
  if (!h) return BP_ERR_INVALID_ARG;
  const char* what = "bp_infer_clips_events";
  const EventsSink out{events, max_events, bends, max_bends, event_offsets, status};
  if (int rc = check_events(h, what, n_clips, params, out)) return rc;
  std::vector<int64_t> n_model((size_t)n_clips), offs((size_t)n_clips + 1);
  if (int rc = check_clips(h, what, n_clips, clips, sample_rate, pcm_mem_kind, true, n_model.data(), offs.data())) return rc;
  if (events_without_device(n_clips, offs.data(), params, out)) return BP_OK;
  BP_HIP(hipSetDevice(h->device));
  if (sample_rate != h->rate)
    if (int rc = clips_filter(h, what, sample_rate)) return rc;
  std::vector<ClipDesc> tab((size_t)n_clips);
  Maps all;
  return run_events(h, what, queue_clips_maps(h, n_clips, clips, sample_rate, pcm_mem_kind, n_model.data(), offs.data(), tab, &all),
                    all, n_clips, offs.data(), params, out);
}

int bp_note_events_from_maps(bp_handle h, int64_t n_clips, const int64_t* row_offsets, const float* note, const float* onset,
                             const float* contour, int mem_kind, const bp_note_params* params, bp_note_event* events,
                             int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets, int* status) {
  if (!h) return BP_ERR_INVALID_ARG;
  const char* what = "bp_note_events_from_maps";
  const EventsSink out{events, max_events, bends, max_bends, event_offsets, status};
  if (int rc = check_events(h, what, n_clips, params, out)) return rc;
  bool ordered = row_offsets && row_offsets[0] == 0;
  for (int64_t i = 0; ordered && i < n_clips; ++i) ordered = row_offsets[i + 1] >= row_offsets[i];
  if (!ordered || (mem_kind != BP_MEM_HOST && mem_kind != BP_MEM_DEVICE)) {
    h->err = std::string(what) + ": row_offsets must start at 0 and never decrease; mem_kind must be BP_MEM_HOST or BP_MEM_DEVICE";
    return BP_ERR_INVALID_ARG;
  }
  const int64_t T = row_offsets[n_clips];
  if (T > 0 && (!note || !onset || !contour)) {
    h->err = std::string(what) + ": null input pointer";
    return BP_ERR_INVALID_ARG;
  }
  if (events_without_device(n_clips, row_offsets, params, out)) return BP_OK;
  BP_HIP(hipSetDevice(h->device));
  // a private copy of the maps: the frequency limits are applied in place
  Maps m;
  int rc = take_track_out(h, T, &m);
  if (!rc) {
    const Maps given{const_cast<float*>(note), const_cast<float*>(onset), const_cast<float*>(contour)};  // only read
    rc = copy_maps(h, m, given, T, mem_kind == BP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice);
  }
  return run_events(h, what, rc, m, n_clips, row_offsets, params, out);
}

#ifdef BP_AB_KERNELS
// The A/B library's test hook for the segmented note candidates (declared nowhere: the tests name it): the clips' maps are
// given, not made — host maps of offsets[n_clips] rows, clip c at rows [offsets[c], offsets[c + 1]) — and go through what
// bp_infer_clips_candidates runs behind the model.  The product library has no such call.
int bp_ab_clips_candidates_from_maps(bp_handle h, int64_t n_clips, const int64_t* offsets, const float* note, const float* onset,
                                     const float* contour, const bp_note_params* params, float* note_out, uint8_t* cand_bits,
                                     int8_t* bend_map, int* status) {
  if (!h || n_clips < 1 || !offsets || !note || !onset || !contour || !params || !note_out || !cand_bits || !status ||
      offsets[0] != 0 || offsets[n_clips] < 1)
    return BP_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n_clips; ++i)
    if (offsets[i + 1] < offsets[i]) return BP_ERR_INVALID_ARG;
  BP_HIP(hipSetDevice(h->device));
  const int64_t T = offsets[n_clips];
  bool exported_by_kernel = false;
  Maps m;
  int rc = take_track_out(h, T, &m);
  if (!rc) {
    const Maps given{const_cast<float*>(note), const_cast<float*>(onset), const_cast<float*>(contour)};  // only read
    if (!(rc = copy_maps(h, m, given, T, hipMemcpyHostToDevice)))
      rc = queue_clips_candidates(h, m, n_clips, offsets, params, note_out, cand_bits, bend_map, &exported_by_kernel);
    rc = finish(h, rc);
  }
  if (rc) return rc;
  clips_status(h, n_clips, offsets, params, exported_by_kernel, status);
  return BP_OK;
}

// The A/B library's test hook for the tracker with per-segment parameters (declared nowhere: the tests name it):
// bp_note_events_from_maps on host maps with one bp_note_params per segment and the tracker form (0: as the product chooses,
// 2: every segment's working state in the scratch buffer).  The dense half — frequency limits, inferred onsets, the onset
// threshold — takes params[0], and makes the bend map where any segment wants bends; the tracker takes segment c's frame
// threshold, tolerance, minimum length, melodia and bends.
int bp_ab_note_events_from_maps_forms(bp_handle h, int64_t n, const int64_t* row_offsets, const float* note, const float* onset,
                                      const float* contour, const bp_note_params* params, int form, bp_note_event* events,
                                      int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets, int* status) {
  if (!h || n < 1 || !row_offsets || !note || !onset || !contour || !params || !event_offsets || !status || row_offsets[0] != 0 ||
      row_offsets[n] < 1 || (form != kNoteTrackFormAuto && form != kNoteTrackFormScratch) || !(params[0].onset_threshold > 0.0))
    return BP_ERR_INVALID_ARG;
  const char* what = "bp_ab_note_events_from_maps_forms";
  const EventsSink out{events, max_events, bends, max_bends, event_offsets, status};
  std::vector<NoteTrackSeg> seg((size_t)n);
  bool any_bends = false;
  for (int64_t i = 0; i < n; ++i) {
    any_bends = any_bends || params[i].include_pitch_bends != 0;
    if (row_offsets[i + 1] < row_offsets[i]) return BP_ERR_INVALID_ARG;
    if (int rc = check_events(h, what, n, params + i, out)) return rc;
    const bp_note_params& p = params[i];
    seg[(size_t)i] = NoteTrackSeg{p.frame_threshold, p.energy_tol, p.min_note_len, p.melodia_trick != 0,
                                  p.include_pitch_bends != 0, 0, 0};
  }
  BP_HIP(hipSetDevice(h->device));
  const int64_t T = row_offsets[n];
  const EventsJob job{what, "n", n, row_offsets, nullptr, seg.data(), nullptr, form};
  EventsPlan plan;
  auto queue = [&]() -> int {
    Maps m;
    uint8_t* d_bits = nullptr;
    int8_t* d_bend = nullptr;
    const Maps given{const_cast<float*>(note), const_cast<float*>(onset), const_cast<float*>(contour)};  // only read
    if (int rc = events_reserve(h, job, &plan)) return rc;
    if (int rc = take_track_out(h, T, &m)) return rc;
    if (int rc = copy_maps(h, m, given, T, hipMemcpyHostToDevice)) return rc;
    if (int rc = queue_clips_dense(h, m, n, row_offsets, params, any_bends, &d_bits, &d_bend)) return rc;
    return events_queue(h, job, plan, TrackInputs{m.note, d_bits, d_bend, h->clip_rows, h->clip_stats});
  };
  if (int rc = finish(h, queue())) return rc;
  return events_home(h, job, out, nullptr);
}
#endif

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
  BP_HIP(hipMemcpy(wide ? (void*)pcm : tmp.data(), h->pcm_dev, (size_t)n * (wide ? 4 : 2), hipMemcpyDeviceToHost));
  const int sh = (wide ? 32 : 16) - lay.bits_per_sample;  // left-justified on the device
  for (int64_t i = 0; i < n; ++i) pcm[i] = (wide ? pcm[i] : (int32_t)tmp[(size_t)i]) >> sh;
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

// ---- a job of FLAC clips (include/basic_pitch_amd_flac_clips.h) ------------------------------------------------------------------
int bp_flac_clips_row_offsets(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int sample_rate, int64_t* offsets, int* status) {
  if (!h) return BP_ERR_INVALID_ARG;
  const char* what = "bp_flac_clips_row_offsets";
  if (!offsets || (n_clips > 0 && !status) || sample_rate < 1) {
    h->err = std::string(what) + ": null offsets / status or no sample rate";
    return BP_ERR_INVALID_ARG;
  }
  FlacJob job;
  if (int rc = plan_flac_clips(h, what, n_clips, clips, sample_rate, &job)) return rc;
  for (int64_t i = 0; i <= n_clips; ++i) offsets[i] = job.offs[(size_t)i];
  for (int64_t i = 0; i < n_clips; ++i) status[i] = 0;
  flac_clips_status(h, job, false, status);
  return BP_OK;
}

int bp_flac_clips_decode_device(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int32_t* pcm, const int64_t* pcm_offsets,
                                int* status) {
  if (!h) return BP_ERR_INVALID_ARG;
  const char* what = "bp_flac_clips_decode_device";
  if (!pcm_offsets || (n_clips > 0 && !status)) {
    h->err = std::string(what) + ": null pcm_offsets / status";
    return BP_ERR_INVALID_ARG;
  }
  FlacJob job;
  if (int rc = plan_flac_clips(h, what, n_clips, clips, 0, &job)) return rc;
  for (int64_t i = 0; i < n_clips; ++i)
    if (job.dev[(size_t)i] >= 0 && (!pcm || pcm_offsets[i] < 0 ||
                                    pcm_offsets[i + 1] - pcm_offsets[i] < job.lay[(size_t)i].n_frames * job.lay[(size_t)i].channels)) {
      h->err = std::string(what) + ": clip " + std::to_string(i) + ": null pcm or too little room between its offsets";
      return BP_ERR_INVALID_ARG;
    }
  for (int64_t i = 0; i < n_clips; ++i) status[i] = 0;
  flac_clips_status(h, job, false, status);
  if (job.tab.empty()) return BP_OK;
  BP_HIP(hipSetDevice(h->device));
  h->maps_rows = 0;  // (the PCM staging is shared with the track calls; their maps are not, but a decode is no *_candidates call)
  if (int rc = finish(h, queue_flac_clips(h, clips, job))) return rc;
  std::vector<uint8_t> home((size_t)job.pcm_bytes);
  BP_HIP(hipMemcpy(home.data(), h->pcm_dev, home.size(), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n_clips; ++i) {
    if (job.dev[(size_t)i] < 0) continue;
    const FdClip& k = job.tab[(size_t)job.dev[(size_t)i]];
    const int64_t n = k.st.total * k.st.channels;
    int32_t* out = pcm + pcm_offsets[i];
    const int sh = k.out_shift;  // left-justified on the device
    if (k.out_wide) {
      const int32_t* src = reinterpret_cast<const int32_t*>(home.data() + k.pcm_off);
      for (int64_t j = 0; j < n; ++j) out[j] = src[j] >> sh;
    } else {
      const int16_t* src = reinterpret_cast<const int16_t*>(home.data() + k.pcm_off);
      for (int64_t j = 0; j < n; ++j) out[j] = (int32_t)src[j] >> sh;
    }
  }
  flac_clips_status(h, job, true, status);
  return BP_OK;
}

int bp_infer_flac_clips_candidates(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int sample_rate,
                                   const bp_note_params* params, float* note_out, uint8_t* cand_bits, int8_t* bend_map, int* status) {
  if (!h) return BP_ERR_INVALID_ARG;
  const char* what = "bp_infer_flac_clips_candidates";
  if (!params || (n_clips > 0 && !status) || sample_rate < 1) {
    h->err = std::string(what) + ": null params / status or no sample rate";
    return BP_ERR_INVALID_ARG;
  }
  FlacJob job;
  if (int rc = plan_flac_clips(h, what, n_clips, clips, sample_rate, &job)) return rc;
  const int64_t total = job.offs[(size_t)n_clips];
  if (total > 0 && (!note_out || !cand_bits)) {
    h->err = std::string(what) + ": null output pointer";
    return BP_ERR_INVALID_ARG;
  }
  for (int64_t i = 0; i < n_clips; ++i) status[i] = 0;
  flac_clips_status(h, job, false, status);
  if (total == 0) return BP_OK;  // no clip has a row: nothing to queue
  BP_HIP(hipSetDevice(h->device));
  if (sample_rate != h->rate)
    if (int rc = clips_filter(h, what, sample_rate)) return rc;
  std::vector<ClipDesc> tab((size_t)n_clips);
  std::vector<bp_clip> decoded;
  bool exported_by_kernel = false;
  auto queue = [&]() -> int {
    if (int rc = queue_flac_clips(h, clips, job)) return rc;
    decoded = flac_pcm_clips(h, job);
    return queue_clips(h, n_clips, decoded.data(), sample_rate, BP_MEM_DEVICE, job.n_model.data(), job.offs.data(), params, note_out,
                       cand_bits, bend_map, tab, &exported_by_kernel);
  };
  if (int rc = finish(h, queue())) return rc;
  clips_status(h, n_clips, job.offs.data(), params, exported_by_kernel, status);
  flac_clips_status(h, job, true, status);
  return BP_OK;
}

int bp_infer_flac_clips_events(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int sample_rate, const bp_note_params* params,
                               bp_note_event* events, int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets,
                               int* status) {
  if (!h) return BP_ERR_INVALID_ARG;
  const char* what = "bp_infer_flac_clips_events";
  const EventsSink out{events, max_events, bends, max_bends, event_offsets, status};
  if (int rc = check_events(h, what, n_clips, params, out)) return rc;
  if (sample_rate < 1) {
    h->err = std::string(what) + ": no sample rate";
    return BP_ERR_INVALID_ARG;
  }
  FlacJob job;
  if (int rc = plan_flac_clips(h, what, n_clips, clips, sample_rate, &job)) return rc;
  if (events_without_device(n_clips, job.offs.data(), params, out)) {
    flac_clips_status(h, job, false, status);
    return BP_OK;
  }
  BP_HIP(hipSetDevice(h->device));
  if (sample_rate != h->rate)
    if (int rc = clips_filter(h, what, sample_rate)) return rc;
  std::vector<ClipDesc> tab((size_t)n_clips);
  std::vector<bp_clip> decoded;
  Maps all{};
  int rc = queue_flac_clips(h, clips, job);
  if (rc == BP_OK) {
    decoded = flac_pcm_clips(h, job);
    rc = queue_clips_maps(h, n_clips, decoded.data(), sample_rate, BP_MEM_DEVICE, job.n_model.data(), job.offs.data(), tab, &all);
  }
  if ((rc = run_events(h, what, rc, all, n_clips, job.offs.data(), params, out))) {
    flac_clips_status(h, job, false, status);  // (buffers too small: status and event_offsets are complete but for the verdicts)
    return rc;
  }
  // a clip the decoder failed on has no events: the others' move up, their bends with them
  int64_t w = 0, bw = 0;
  for (int64_t c = 0; c < n_clips; ++c) {
    const bool drop = job.dev[(size_t)c] >= 0 && h->fd_status_host[2 * job.dev[(size_t)c]] != 0;
    const int64_t e0 = event_offsets[c], e1 = event_offsets[c + 1];
    event_offsets[c] = w;
    for (int64_t e = e0; e < e1 && !drop; ++e) {
      bp_note_event ev = events[e];
      if (ev.n_bends && bw != ev.bend_offset) std::memmove(bends + bw, bends + ev.bend_offset, (size_t)ev.n_bends * sizeof(int32_t));
      ev.bend_offset = bw, bw += ev.n_bends;
      events[w++] = ev;
    }
    if (c + 1 == n_clips) event_offsets[n_clips] = w;
  }
  flac_clips_status(h, job, true, status);
  return BP_OK;
}

}  // extern "C"
