// C ABI of the jobs of many clips (include/basic_pitch_amd_clips.h, _events.h, _flac_clips.h, _sweep.h): many short clips through the
// model in one call — raw PCM, FLAC or IMA ADPCM files' bytes decoded on the device, or maps the caller already holds — and home either
// the note candidates of every clip or, the tracker run on the device too, the note events alone: under one parameter set, or
// (a sweep) every segment under many; or, of the contour rows alone, the f0 peaks of every segment and the frame-level counts of
// threshold sweeps over them (include/basic_pitch_amd_multipitch.h); or the melody of every segment, one f0 track by a Viterbi
// recurrence, and the melody measures of parameter sweeps over it (include/basic_pitch_amd_melody.h); or, of the note and onset
// rows, the alignment of every segment's reference score by a monotone recurrence (include/basic_pitch_amd_align.h); or, of the
// onset rows alone, the tempo and the beats of every segment (include/basic_pitch_amd_beat.h).
//
// Every entry point is a source and a sink on one driver (run_clips), the job family's run_track (track_api.hip):
//   the sink's fixed arguments -> the source's plan (rows of every clip) -> the outputs against the rows -> statuses and the
//   exits without device work -> the filter -> queue the source, the dense half, the sink -> wait -> statuses / events home ->
//   the FLAC decoder's verdicts.
// Nothing is queued before every argument has been checked, a call that fails after queuing work returns only once the
// handle's stream has drained (finish), and every host buffer an asynchronous copy reads is a member of the driver's ClipsJob,
// which outlives the wait.  The tracker's host half (events_reserve / events_queue / events_home) lives here too:
// bp_streams_events (stream_api.hip) puts it behind its own dense half.
#include <algorithm>
#include <cstring>
#include <map>
#include <tuple>

#include "../../include/basic_pitch_amd_adpcm.h"
#include "../../include/basic_pitch_amd_flac_clips.h"
#include "../../include/basic_pitch_amd_score.h"
#include "../../include/basic_pitch_amd_frame_score.h"
#include "../../include/basic_pitch_amd_multipitch.h"
#include "../../include/basic_pitch_amd_melody.h"
#include "../../include/basic_pitch_amd_align.h"
#include "../../include/basic_pitch_amd_beat.h"
#include "../../include/basic_pitch_amd_sweep.h"
#include "bp_context.h"

using namespace bp;

extern "C" void bp_internal_freq_limits(const bp_note_params* prm, int* lo, int* hi);
extern "C" double bp_internal_frame_time(int64_t frame);
extern "C" const char* bp_internal_score_bad_params(const bp_score_params* p);
extern "C" int64_t bp_internal_score_bad_ref(const bp_ref_note* refs, int64_t n);
extern "C" double bp_internal_score_offset_tol(const bp_ref_note* r, const bp_score_params* p);
extern "C" void bp_internal_frame_interval(double start_s, double end_s, int64_t n_frames, int64_t* f0, int64_t* f1);
extern "C" void bp_internal_frame_pitch_range(const bp_ref_note* r, const bp_score_params* p, int32_t* lo, int32_t* hi);
extern "C" const char* bp_internal_mp_bad_params(const bp_mp_params* p);
extern "C" const char* bp_internal_melody_bad_params(const bp_melody_params* p);  // melody_host.cpp
extern "C" int64_t bp_internal_melody_bad_ref(const double* ref_pitch, int64_t n);
extern "C" const char* bp_internal_align_bad_params(const bp_align_params* p);  // align_host.cpp
extern "C" const char* bp_internal_align_bad_states(const bp_align_state* states, int64_t n, int64_t* index);
extern "C" const char* bp_internal_beat_bad_params(const bp_beat_params* p);  // beat_host.cpp
extern "C" int bp_internal_flac_device_supported(const bp_flac_stream_layout* lay, size_t nbytes);

namespace bp {

// ---- the tracker behind any dense half (declared in bp_context.h): the clips calls here, bp_streams_events in stream_api.hip
static bool seg_bends(const EventsJob& job, int64_t c) {
  return job.seg ? job.seg[c].bends != 0 : job.prm->include_pitch_bends != 0;
}

int events_reserve(bp_handle h, const EventsJob& job, EventsPlan* plan, bool home) {
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
  BP_HIP(h->ev_counts.reserve((size_t)n * 16));
  BP_HIP(h->ev_pool.reserve((size_t)pool_events * 16));
  if (scratch) BP_HIP(h->ev_scratch.reserve((size_t)note_track_scratch_floats(T)));
  if (job.seg) BP_HIP(h->ev_seg.reserve((size_t)n * sizeof(NoteTrackSeg)));
  if (!home) return BP_OK;
  BP_HIP(h->ev_meta.reserve((size_t)n_meta));
  BP_HIP(h->ev_out.reserve((size_t)pool_events * 16));
  BP_HIP(h->bd_pool.reserve((size_t)T * 88));
  BP_HIP(h->bd_out.reserve((size_t)T * 88));
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

int invalid(bp_handle h, const char* what, const std::string& why) {
  h->err = std::string(what) + ": " + why;
  return BP_ERR_INVALID_ARG;
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

// ---- many clips in one call (include/basic_pitch_amd_clips.h) -------------------------------------------------------------
// Every argument of every clip (check_ingest; with_pcm: the samples are needed too), before anything is queued: n_model[i] =
// clip i's samples at the handle's rate, offsets[i] = the rows of the clips before it, offsets[n_clips] = all rows.
int check_clips(bp_handle h, const char* what, int64_t n_clips, const bp_clip* clips, int sample_rate, int mem_kind, bool with_pcm,
                int64_t* n_model, int64_t* offsets) {
  if (n_clips < 0 || (n_clips > 0 && !clips) || !offsets) return invalid(h, what, "negative n_clips, null clips or null offsets");
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

// The ingest and the model on the clips' windows packed into full chunks: the maps to h->track_out (*all_out), concatenated by
// offs.  offs[n_clips] > 0.
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

// ---- note events of many clips (include/basic_pitch_amd_events.h)
// every argument that is not a clip's, before anything is queued
// why the tracker refuses a parameter set (null: it takes it), and why a call's room for events and bends is refused
const char* bad_params(const bp_note_params& prm) {
  if (prm.melodia_trick && prm.frame_threshold < 0.0)
    return "a negative frame threshold with the melodia trick never terminates (note_creation.py:452)";
  return prm.min_note_len < 0 ? "negative min_note_len" : nullptr;
}
const char* bad_room(const EventsSink& out) {
  const bool bad = out.max_events < 0 || out.max_bends < 0 || (out.max_events > 0 && !out.events) || (out.max_bends > 0 && !out.bends);
  return bad ? "negative max_events / max_bends, or room without a buffer" : nullptr;
}

int check_events(bp_handle h, const char* what, int64_t n_clips, const bp_note_params* prm, const EventsSink& out) {
  auto invalid = [&](const char* why) { return ::invalid(h, what, why); };
  if (n_clips < 0 || !prm || !out.event_offsets || (n_clips > 0 && !out.status)) return invalid("negative n_clips, null params, event_offsets or status");
  if (const char* why = bad_room(out)) return invalid(why);
  if (const char* why = bad_params(*prm)) return invalid(why);
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
  if (n < 0 || (n > 0 && !clips)) return invalid(h, what, "negative n_clips or null clips");
  auto up16 = [](int64_t v) { return (v + 15) / 16 * 16; };
  job->lay.assign((size_t)n, bp_flac_stream_layout{});
  job->dev.assign((size_t)n, -1);
  job->n_model.assign((size_t)n, 0);
  job->offs.assign((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    const bp_flac_clip& c = clips[i];
    bp_flac_stream_layout& l = job->lay[(size_t)i];
    job->offs[(size_t)i + 1] = job->offs[(size_t)i];
    if (!c.file && c.nbytes) return invalid(h, what, "clip " + std::to_string(i) + ": null file");
    if (c.nbytes < 42 || bp_flac_layout(c.file, c.nbytes, &l) != BP_OK) continue;
    if (sample_rate && l.sample_rate != sample_rate)
      return invalid(h, what, "clip " + std::to_string(i) + ": its STREAMINFO says " + std::to_string(l.sample_rate) + " Hz, the call " +
                                  std::to_string(sample_rate) + " Hz (one rate per call)");
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
    if (job->wgs >= ((int64_t)1 << 31) || job->slots >= ((int64_t)1 << 31))
      return invalid(h, what, "the job is too large for one call (2^31 scan chunks or frame slots)");
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

// the host-side statuses; with `decoded` (the stream has been waited for) the decoder's verdict on every device clip too
void flac_clips_status(bp_handle h, const FlacJob& job, bool decoded, int* status) {
  for (size_t i = 0; i < job.dev.size(); ++i) {
    if (job.dev[i] < 0) status[i] = BP_CLIP_FLAC_HOST;
    else if (decoded && h->fd_status_host[2 * job.dev[i]] != 0) status[i] = BP_CLIP_FLAC_FAILED;
  }
}

// A clip the decoder failed on has no events: the others' move up, their bends with them.
void drop_failed_clips(bp_handle h, const FlacJob& job, const EventsSink& out) {
  const int64_t n = (int64_t)job.dev.size();
  int64_t w = 0, bw = 0;
  for (int64_t c = 0; c < n; ++c) {
    const bool drop = job.dev[(size_t)c] >= 0 && h->fd_status_host[2 * job.dev[(size_t)c]] != 0;
    const int64_t e0 = out.event_offsets[c], e1 = out.event_offsets[c + 1];
    out.event_offsets[c] = w;
    for (int64_t e = e0; e < e1 && !drop; ++e) {
      bp_note_event ev = out.events[e];
      if (ev.n_bends && bw != ev.bend_offset)
        std::memmove(out.bends + bw, out.bends + ev.bend_offset, (size_t)ev.n_bends * sizeof(int32_t));
      ev.bend_offset = bw, bw += ev.n_bends;
      out.events[w++] = ev;
    }
    if (c + 1 == n) out.event_offsets[n] = w;
  }
}

// ---- a job of IMA ADPCM clips decoded on the device (include/basic_pitch_amd_adpcm.h; adpcm_device.hip) --------------------------
// What the host knows of a job before anything is queued: every clip's layout (all of one codec, rate and channel count), and
// what queue_adpcm's asynchronous copies read.
struct AdpcmJob {
  std::vector<bp_adpcm_layout> lay;
  std::vector<const void*> files;
  std::vector<AdpcmSeg> segs;
  std::vector<int64_t> pcm_off;
};

// every clip's headers and ingest arguments; *sample_rate: the clips' (no clips: the handle's); n_model / offs as check_clips
int plan_adpcm_clips(bp_handle h, const char* what, int64_t n, const bp_adpcm_clip* clips, AdpcmJob* job, int* sample_rate,
                     std::vector<int64_t>* n_model, std::vector<int64_t>* offs) {
  if (n < 0 || (n > 0 && !clips)) return invalid(h, what, "negative n_clips or null clips");
  job->lay.assign((size_t)n, bp_adpcm_layout{});
  job->files.assign((size_t)n, nullptr);
  job->pcm_off.assign((size_t)n, 0);
  n_model->assign((size_t)n, 0);
  offs->assign((size_t)n + 1, 0);
  *sample_rate = h->rate;
  for (int64_t i = 0; i < n; ++i) {
    const std::string clip = "clip " + std::to_string(i) + ": ";
    bp_adpcm_layout& l = job->lay[(size_t)i];
    if (!clips[i].file) return invalid(h, what, clip + "null file");
    if (bp_adpcm_layout_of(clips[i].file, clips[i].nbytes, &l) != BP_OK) {
      h->err = std::string(what) + ": " + clip + bp_files_last_error();
      return BP_ERR_BAD_AUDIO;
    }
    const bp_adpcm_layout& first = job->lay[0];
    if (l.codec != first.codec || l.sample_rate != first.sample_rate || l.channels != first.channels)
      return invalid(h, what, clip + "codec " + std::to_string(l.codec) + ", " + std::to_string(l.sample_rate) + " Hz, " +
                                  std::to_string(l.channels) + " channels; clip 0 has codec " + std::to_string(first.codec) + ", " +
                                  std::to_string(first.sample_rate) + " Hz, " + std::to_string(first.channels) +
                                  " channels (one codec, rate and channel count per call)");
    if (int rc = check_ingest(h, true, BP_PCM_S16, l.n_frames, l.channels, l.sample_rate, BP_MEM_DEVICE)) {
      h->err = std::string(what) + ": " + clip + h->err;
      return rc;
    }
    *sample_rate = l.sample_rate;
    job->files[(size_t)i] = clips[i].file;
    (*n_model)[(size_t)i] = resampled_length(l.n_frames, l.sample_rate, h->rate);
    (*offs)[(size_t)i + 1] = (*offs)[(size_t)i] + h_frames(h, (*n_model)[(size_t)i]);
  }
  return BP_OK;
}

// ---- the driver ------------------------------------------------------------------------------------------------------------
// Where the maps of the n segments come from.  kPcmClips: `clips` (PCM in host or device memory after mem_kind) at sample_rate;
// kFlacClips: `flac` (bytes in host memory, STREAMINFO rate sample_rate), decoded on the device, then as kPcmClips in device
// memory; kAdpcmClips: `adpcm` (IMA ADPCM files' bytes in host memory; the rate is the files'), decoded on the device by one
// launch, then as kPcmClips in device memory; kGivenMaps: no signal but maps already made (mem_kind), segment c at rows
// [row_offsets[c], row_offsets[c + 1]).
enum JobSourceKind { kPcmClips, kFlacClips, kGivenMaps, kAdpcmClips };
struct JobSource {
  JobSourceKind kind;
  int64_t n;
  int mem_kind, sample_rate;
  const bp_clip* clips;
  const bp_flac_clip* flac;
  const int64_t* row_offsets;
  const float *note, *onset, *contour;
  const bp_adpcm_clip* adpcm;
};

// Where the results go.  kCandidatesHome: the note candidates of all rows (host buffers) and out.status, the maps stay in
// track_out; kEventsHome: the events (out).  params: of the dense half, and of the tracker unless seg_params gives every
// segment its own (with the tracker's form and the call's name for n: the A/B hook).  kSweepHome: the events (out) of n_decodes
// decodes, decode j segment decodes[j].segment under sets[decodes[j].params] (decodes null: the cross product, set-major);
// params is null, every set has its own dense half.  kScoreHome: the same sweep, but what goes home is `scores` and out.status
// alone — every decode's events scored on the device against the refs of its segment (include/basic_pitch_amd_score.h).
// with_frames: the calls of include/basic_pitch_amd_frame_score.h — `frames` goes home too, and `scores` may be null.
enum JobSinkKind { kCandidatesHome, kEventsHome, kSweepHome, kScoreHome, kMultiPitchHome, kMultiPitchScoreHome, kMelodyHome, kMelodyScoreHome, kAlignHome, kBeatHome };
struct JobSink {
  JobSinkKind kind;
  const bp_note_params* params;
  EventsSink out;
  float* note_out;
  uint8_t* cand_bits;
  int8_t* bend_map;
  const bp_note_params* seg_params;
  int form;
  const char* count_name;
  int64_t n_sets, n_decodes;
  const bp_note_params* sets;
  const bp_sweep_decode* decodes;
  const int64_t* ref_offsets;  // kScoreHome: [n segments + 1], the refs of each segment
  const bp_ref_note* refs;
  const bp_score_params* score_params;
  bp_note_score* scores;
  bool with_frames;
  bp_frame_score* frames;
  // kMultiPitchHome: the points (include/basic_pitch_amd_multipitch.h) of the n segments under mp_params[0], out.status per
  // segment.  kMultiPitchScoreHome: n_decodes decodes of the segments under mp_params[0 ... n_sets), scored against the refs:
  // `frames` and out.status alone go home.
  const bp_mp_params* mp_params;
  bp_f0_point* points;
  int64_t max_points;
  int64_t* point_offsets;
  // kMelodyHome: the records (include/basic_pitch_amd_melody.h) of the n segments under mel_params[0], a record per row, room
  // for max_points of them, out.status per segment.  kMelodyScoreHome: n_decodes decodes of the segments under mel_params[0 ...
  // n_sets), scored against ref_pitch (parallel to the rows of the segments): mel_scores and out.status alone go home.
  const bp_melody_params* mel_params;
  bp_melody_point* mel_points;
  const double* ref_pitch;
  bp_melody_score* mel_scores;
  // kAlignHome: the alignment (include/basic_pitch_amd_align.h) of the n segments, segment i against al_states[state_offsets[i]
  // ... state_offsets[i + 1]) under al_params: first_frame parallel to the states (room for max_states), al_total and out.status
  // per segment.
  const bp_align_params* al_params;
  const int64_t* state_offsets;
  const bp_align_state* al_states;
  int32_t* first_frame;
  int64_t max_states;
  int64_t* al_total;
  // kBeatHome: tempo and beats (include/basic_pitch_amd_beat.h) of the n segments under bt_params: a summary per segment, the
  // beats as one compact array (room for max_beats) with bt_offsets [n + 1].
  const bp_beat_params* bt_params;
  bp_beat_summary* bt_summaries;
  int32_t* bt_beats;
  int64_t max_beats;
  int64_t* bt_offsets;
};

JobSink candidates_sink(const bp_note_params* params, float* note_out, uint8_t* cand_bits, int8_t* bend_map, int* status) {
  return JobSink{kCandidatesHome, params, EventsSink{nullptr, 0, nullptr, 0, nullptr, status}, note_out, cand_bits, bend_map};
}

JobSink events_sink(const bp_note_params* params, bp_note_event* events, int64_t max_events, int32_t* bends, int64_t max_bends,
                    int64_t* event_offsets, int* status) {
  return JobSink{kEventsHome, params, EventsSink{events, max_events, bends, max_bends, event_offsets, status},
                 nullptr, nullptr, nullptr, nullptr, kNoteTrackFormAuto, "n_clips"};
}

JobSink sweep_sink(int64_t n_sets, const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes, bp_note_event* events,
                   int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets, int* status) {
  JobSink k = events_sink(nullptr, events, max_events, bends, max_bends, event_offsets, status);
  k.kind = kSweepHome, k.count_name = "n_decodes";
  k.n_sets = n_sets, k.n_decodes = n_decodes, k.sets = sets, k.decodes = decodes;
  return k;
}

JobSink score_sink(int64_t n_sets, const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes, const int64_t* ref_offsets,
                   const bp_ref_note* refs, const bp_score_params* score_params, bp_note_score* scores, int* status) {
  JobSink k = sweep_sink(n_sets, sets, n_decodes, decodes, nullptr, 0, nullptr, 0, nullptr, status);
  k.kind = kScoreHome;
  k.ref_offsets = ref_offsets, k.refs = refs, k.score_params = score_params, k.scores = scores;
  return k;
}

JobSink frame_score_sink(int64_t n_sets, const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                         const int64_t* ref_offsets, const bp_ref_note* refs, const bp_score_params* score_params, bp_note_score* scores,
                         bp_frame_score* frames, int* status) {
  JobSink k = score_sink(n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, status);
  k.with_frames = true, k.frames = frames;
  return k;
}

JobSink multipitch_sink(const bp_mp_params* p, bp_f0_point* points, int64_t max_points, int64_t* point_offsets, int* status) {
  JobSink k{};
  k.kind = kMultiPitchHome, k.out.status = status;
  k.mp_params = p, k.points = points, k.max_points = max_points, k.point_offsets = point_offsets;
  return k;
}

JobSink multipitch_score_sink(int64_t n_sets, const bp_mp_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                              const int64_t* ref_offsets, const bp_ref_note* refs, const bp_score_params* score_params,
                              bp_frame_score* frames, int* status) {
  JobSink k{};
  k.kind = kMultiPitchScoreHome, k.out.status = status;
  k.mp_params = sets, k.n_sets = n_sets, k.n_decodes = n_decodes, k.decodes = decodes;
  k.ref_offsets = ref_offsets, k.refs = refs, k.score_params = score_params, k.with_frames = true, k.frames = frames;
  return k;
}

JobSink melody_sink(const bp_melody_params* p, bp_melody_point* points, int64_t max_points, int* status) {
  JobSink k{};
  k.kind = kMelodyHome, k.out.status = status;
  k.mel_params = p, k.mel_points = points, k.max_points = max_points;
  return k;
}

JobSink melody_score_sink(int64_t n_sets, const bp_melody_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                          const double* ref_pitch, const bp_score_params* score_params, bp_melody_score* scores, int* status) {
  JobSink k{};
  k.kind = kMelodyScoreHome, k.out.status = status;
  k.mel_params = sets, k.n_sets = n_sets, k.n_decodes = n_decodes, k.decodes = decodes;
  k.ref_pitch = ref_pitch, k.score_params = score_params, k.mel_scores = scores;
  return k;
}

JobSink align_sink(const int64_t* state_offsets, const bp_align_state* states, const bp_align_params* p, int32_t* first_frame,
                   int64_t max_states, int64_t* total, int* status) {
  JobSink k{};
  k.kind = kAlignHome, k.out.status = status;
  k.al_params = p, k.state_offsets = state_offsets, k.al_states = states, k.first_frame = first_frame, k.max_states = max_states;
  k.al_total = total;
  return k;
}

JobSink beat_sink(const bp_beat_params* p, bp_beat_summary* summaries, int32_t* beats, int64_t max_beats, int64_t* beat_offsets) {
  JobSink k{};
  k.kind = kBeatHome;
  k.bt_params = p, k.bt_summaries = summaries, k.bt_beats = beats, k.max_beats = max_beats, k.bt_offsets = beat_offsets;
  return k;
}

// ---- a sweep: the segments of a job under many parameter sets (include/basic_pitch_amd_sweep.h) -----------------
// A dense key: what the dense half of note decoding depends on.  Sets of one key share its bitmap and its block of stats
// records; keys of one band [lo, hi) share the constrained copy of the note rows.
struct SweepKey {
  int lo, hi, infer;
  double onset_thresh;
  int band;  // its band's slot of h->sw_note; -1: all 88 bins, the maps themselves
};
// What the host knows of a sweep before anything is queued, and what its asynchronous copies read.
struct SweepJob {
  std::vector<int64_t> segment;     // per decode: its segment, its set (the cross product spelled out)
  std::vector<int32_t> params;
  std::vector<NoteTrackSeg> seg;    // per decode: the tracker's parameters
  std::vector<int64_t> pool_rows;   // [n_decodes + 1] rows of the decodes before each: its regions of the pools
  std::vector<int> set_key;         // set -> its key; -1: no decode with rows names it, or its onset threshold is <= 0
  std::vector<SweepKey> keys;       // ordered by band
  int64_t n_bands = 0;              // constrained copies of the note rows
  bool bends = false;               // a decode that reaches the tracker wants bends
  std::vector<uint8_t> block;       // the decode table (NoteSweepDecode) with pool_rows and the event regions behind it
  // kScoreHome: the refs as the device reads them, per decode which are its segment's, the room the launch's LDS needs
  std::vector<NoteScoreRef> refs;
  std::vector<NoteScoreDecode> ref_of;
  int max_refs = 0, max_depth = 0;
  std::vector<NoteFrameRef> frame_refs;  // with_frames: per segment its refs in ascending pitch, as note_frames.hip reads them
};

// what a scored sweep takes beside a sweep's arguments, before anything is queued
int check_score(bp_handle h, const char* what, int64_t n_segs, const JobSink& k) {
  auto invalid = [&](const std::string& why) { return ::invalid(h, what, why); };
  if (k.with_frames) {
    if (!k.ref_offsets || (k.n_decodes > 0 && !k.frames)) return invalid("null ref_offsets or frames");
  } else if (!k.ref_offsets || (k.n_decodes > 0 && !k.scores)) {
    return invalid("null ref_offsets or scores");
  }
  if (const char* why = bp_internal_score_bad_params(k.score_params)) return invalid(why);
  if (k.ref_offsets[0] != 0) return invalid("ref_offsets must start at 0");
  for (int64_t i = 0; i < n_segs; ++i)
    if (k.ref_offsets[i + 1] < k.ref_offsets[i])
      return invalid("segment " + std::to_string(i) + ": ref_offsets decrease (" + std::to_string(k.ref_offsets[i]) + " to " +
                     std::to_string(k.ref_offsets[i + 1]) + ")");
  if (k.ref_offsets[n_segs] > 0 && !k.refs) return invalid("null refs");
  const int64_t bad = bp_internal_score_bad_ref(k.refs, k.ref_offsets[n_segs]);
  if (bad >= 0) return invalid("ref " + std::to_string(bad) + ": a field is not finite, or end_s < start_s");
  return BP_OK;
}

// decode j of a scored sweep without events: {n_ref, 0, 0, 0} and {rows, 0, 0, 0, 0} (its segment: seg)
void score_nothing(const JobSink& k, int64_t j, int64_t seg, int64_t rows) {
  const int64_t n_ref = k.ref_offsets[seg + 1] - k.ref_offsets[seg];
  if (k.scores) k.scores[j] = bp_note_score{(int32_t)std::min<int64_t>(n_ref, INT32_MAX), 0, 0, 0};
  if (k.frames) k.frames[j] = bp_frame_score{rows, 0, 0, 0, 0};
}

// the decode table of a sweep against its segments and sets; decodes null: the cross product
int check_decode_table(bp_handle h, const char* what, int64_t n_segs, int64_t n_sets, int64_t n_decodes, const bp_sweep_decode* decodes) {
  auto invalid = [&](const std::string& why) { return ::invalid(h, what, why); };
  if (!decodes) {
    const bool product = n_segs == 0 || n_sets == 0 ? n_decodes == 0 : n_decodes % n_segs == 0 && n_decodes / n_segs == n_sets;
    if (!product) return invalid("decodes is NULL (the cross product) and n_decodes is not n_sets * n_segments");
    return BP_OK;
  }
  for (int64_t j = 0; j < n_decodes; ++j) {
    const bp_sweep_decode& d = decodes[j];
    if (d.reserved != 0) return invalid("decode " + std::to_string(j) + ": reserved must be 0");
    if (d.params < 0 || d.params >= n_sets)
      return invalid("decode " + std::to_string(j) + ": params " + std::to_string(d.params) + " is not one of the " + std::to_string(n_sets) + " sets");
    if (d.segment < 0 || d.segment >= n_segs)
      return invalid("decode " + std::to_string(j) + ": segment " + std::to_string(d.segment) + " is not one of the " + std::to_string(n_segs) + " segments");
  }
  return BP_OK;
}

// every argument of a sweep that is not a segment's, before anything is queued
int check_sweep(bp_handle h, const char* what, int64_t n_segs, const JobSink& k) {
  auto invalid = [&](const std::string& why) { return ::invalid(h, what, why); };
  const bool score = k.kind == kScoreHome;  // no events go home: no offsets, no room
  if (n_segs < 0 || k.n_sets < 0 || k.n_decodes < 0 || (k.n_sets > 0 && !k.sets) || (!score && !k.out.event_offsets) ||
      (k.n_decodes > 0 && !k.out.status))
    return invalid("negative n_segments / n_clips, n_sets or n_decodes, null sets, event_offsets or status");
  if (const char* why = score ? nullptr : bad_room(k.out)) return invalid(why);
  if (k.n_decodes > BP_SWEEP_MAX_DECODES)
    return invalid(std::to_string(k.n_decodes) + " decodes, more than BP_SWEEP_MAX_DECODES (" + std::to_string(BP_SWEEP_MAX_DECODES) +
                   "): split the job");
  for (int64_t p = 0; p < k.n_sets; ++p)
    if (const char* why = bad_params(k.sets[p])) return invalid("set " + std::to_string(p) + ": " + why);
  return check_decode_table(h, what, n_segs, k.n_sets, k.n_decodes, k.decodes);
}

// The decodes against the rows (offs: of the n_segs segments): every decode's tracker parameters and regions, the dense keys of
// the sets that reach the tracker.  *queued false: no decode needs the device — no rows, or an onset threshold <= 0 (status 1,
// as events_without_device says it) — and the outputs are complete.
int plan_sweep(bp_handle h, const char* what, int64_t n_segs, const int64_t* offs, const JobSink& k, SweepJob* w, bool* queued) {
  const int64_t n = k.n_decodes;
  const bool score = k.kind == kScoreHome;
  w->segment.resize((size_t)n), w->params.resize((size_t)n), w->seg.resize((size_t)n);
  w->pool_rows.assign((size_t)n + 1, 0);
  w->set_key.assign((size_t)k.n_sets, -1);
  std::map<std::tuple<int, int, int, double>, int> keys;  // (a threshold > 0 is no NaN: the order is total)
  *queued = false;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t i = k.decodes ? k.decodes[j].segment : j % n_segs;
    const int32_t p = k.decodes ? k.decodes[j].params : (int32_t)(j / n_segs);
    const bp_note_params& prm = k.sets[p];
    const int64_t rows = offs[i + 1] - offs[i];
    const bool skip = !(prm.onset_threshold > 0.0);
    w->segment[(size_t)j] = i, w->params[(size_t)j] = p;
    w->seg[(size_t)j] = NoteTrackSeg{prm.frame_threshold, prm.energy_tol, prm.min_note_len, prm.melodia_trick != 0,
                                     prm.include_pitch_bends != 0, skip, 0};
    w->pool_rows[(size_t)j + 1] = w->pool_rows[(size_t)j] + rows;
    if (rows == 0 || skip) continue;
    *queued = true;
    w->bends = w->bends || (prm.include_pitch_bends != 0 && !score);  // (a scored sweep counts the bends and makes none)
    if (w->set_key[(size_t)p] >= 0) continue;
    int lo = 0, hi = 88;
    bp_internal_freq_limits(&prm, &lo, &hi);
    w->set_key[(size_t)p] = keys.emplace(std::make_tuple(lo, hi, prm.infer_onsets != 0, prm.onset_threshold), (int)keys.size()).first->second;
  }
  if (w->pool_rows[(size_t)n] > BP_SWEEP_MAX_ROWS)
    return invalid(h, what, "the decodes have " + std::to_string(w->pool_rows[(size_t)n]) + " rows in all, more than BP_SWEEP_MAX_ROWS (" +
                                std::to_string(BP_SWEEP_MAX_ROWS) + "): split the job");
  if (!*queued) {
    for (int64_t j = 0; j < n; ++j) k.out.status[j] = w->pool_rows[(size_t)j + 1] > w->pool_rows[(size_t)j] ? 1 : 0;
    for (int64_t j = 0; j <= n && !score; ++j) k.out.event_offsets[j] = 0;
    for (int64_t j = 0; j < n && score; ++j)
      score_nothing(k, j, w->segment[(size_t)j], w->pool_rows[(size_t)j + 1] - w->pool_rows[(size_t)j]);
    return BP_OK;
  }
  if (score) {  // the refs as the device reads them; which are whose
    const int64_t n_refs = k.ref_offsets[n_segs];
    w->refs.resize(k.scores ? (size_t)n_refs : 0);
    for (int64_t i = 0; i < n_refs && k.scores; ++i) {
      const bp_ref_note& r = k.refs[i];
      w->refs[(size_t)i] = NoteScoreRef{r.start_s, r.end_s, r.pitch_midi, bp_internal_score_offset_tol(&r, k.score_params)};
    }
    w->ref_of.resize((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
      const int64_t seg = w->segment[(size_t)j], first = k.ref_offsets[seg];
      const int64_t rows = w->pool_rows[(size_t)j + 1] - w->pool_rows[(size_t)j];
      w->ref_of[(size_t)j] = NoteScoreDecode{first, (int32_t)std::min<int64_t>(k.ref_offsets[seg + 1] - first, kNoteScoreMaxNotes + 1),
                                             w->seg[(size_t)j].bends && rows <= kNoteTrackMaxRows ? (int32_t)(88 * rows) : -1};
    }
  }
  if (score && k.with_frames) {  // what depends on a ref and its segment alone, by the checker's own functions; a segment's in pitch order
    w->frame_refs.resize((size_t)k.ref_offsets[n_segs]);
    std::vector<int64_t> order;
    for (int64_t i = 0; i < n_segs; ++i) {
      const int64_t first = k.ref_offsets[i], rows = offs[i + 1] - offs[i];
      order.resize((size_t)(k.ref_offsets[i + 1] - first));
      for (size_t r = 0; r < order.size(); ++r) order[r] = first + (int64_t)r;
      std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return k.refs[a].pitch_midi < k.refs[b].pitch_midi; });
      for (size_t r = 0; r < order.size(); ++r) {
        const bp_ref_note& ref = k.refs[order[r]];
        int64_t f0 = 0, f1 = 0;
        NoteFrameRef& out = w->frame_refs[(size_t)first + r];
        bp_internal_frame_interval(ref.start_s, ref.end_s, rows, &f0, &f1);
        out.f0 = (int32_t)f0, out.f1 = (int32_t)f1;  // (rows <= BP_SWEEP_MAX_ROWS)
        bp_internal_frame_pitch_range(&ref, k.score_params, &out.lo, &out.hi);
      }
    }
  }
  // the keys in the map's order, which keeps a band's keys together; a set's key by that order
  std::vector<int> order(keys.size());
  for (const auto& kv : keys) {
    const auto& [lo, hi, infer, thresh] = kv.first;
    const bool full = lo <= 0 && hi >= 88;
    if (!full && (w->keys.empty() || w->keys.back().lo != lo || w->keys.back().hi != hi)) ++w->n_bands;
    order[(size_t)kv.second] = (int)w->keys.size();
    w->keys.push_back(SweepKey{lo, hi, infer, thresh, full ? -1 : (int)w->n_bands - 1});
  }
  for (int& key : w->set_key)
    if (key >= 0) key = order[(size_t)key];
  return BP_OK;
}

// What a job knows of itself, and every host buffer its asynchronous copies read: the driver holds it until the wait is over.
struct ClipsJob {
  FlacJob flac;                                // n_model and offs of the clips (kPcmClips too); the rest: kFlacClips
  const int64_t* offs = nullptr;               // rows before each segment (kGivenMaps: the caller's)
  std::vector<bp_clip> decoded;                // kFlacClips, kAdpcmClips: the clips' PCM on the device
  AdpcmJob adpcm;                              // kAdpcmClips
  std::vector<ClipDesc> tab;
  std::vector<NoteTrackSeg> seg;
  bool dense_bends = false;                    // kEventsHome: the dense half makes the bend map
  SweepJob sweep;                              // kSweepHome, kScoreHome
  const bp_score_params* score_params = nullptr;  // kScoreHome
  bool want_scores = true, want_frames = false;   // kScoreHome: the note-matching launch, the frame launch
  EventsJob ev{};
  EventsPlan plan;
  bool exported_by_kernel = false;
  // kMultiPitchHome, kMultiPitchScoreHome: where the contour rows lie on the device (the write pass runs after the first
  // wait); the decode table and the refs in pitch order as multipitch.hip reads them
  const float* mp_contour = nullptr;
  std::vector<MpDecode> mp_dec;
  std::vector<MpRef> mp_refs;
  std::vector<MelodyDecode> mel_dec;  // kMelodyHome: a decode per segment; kMelodyScoreHome: the decode table
  std::vector<AlignSeg> al_segs;      // kAlignHome: the segments with rows and states, and what they take of the pools
  int64_t al_cells = 0, al_words = 0, al_tiles = 0;
  int al_max_states = 0;
  std::vector<BeatSeg> bt_segs;       // kBeatHome: the segments with rows, and what they take of the launches and of the beat pool
  int64_t bt_blocks = 0, bt_tiles = 0, bt_cap = 0;
};

// A sweep behind the maps of its n_segs segments (offs: their rows, T > 0 in all): the dense half once per key — the note rows
// constrained into the band's copy where the band is new, the onset rows into the one working copy (the launches are serial:
// it is reused from band to band), then the stats and the bitmap of every segment as the clips calls make them, into the key's
// own blocks — and the bend map once; the tracker over the decode table; the offsets on their way home.  The maps
// themselves are only read.  The records are in h->sw_stats, not the clips calls' h->clip_stats, whose state stays as it was.
// score: no bend map, the tracker without its offsets and pack launches, then the scoring launch over the events where they
// lie (note_score.hip) and the scores with the statuses on their way home.
int queue_sweep(bp_handle h, const Maps& all, int64_t n_segs, const int64_t* offs, ClipsJob& job, bool score) {
  hipStream_t s = h->stream;
  SweepJob& w = job.sweep;
  const int64_t T = offs[n_segs], n = job.ev.n, n_keys = (int64_t)w.keys.size();
  const int64_t plane = T * kFreqN, bits_plane = T * BP_NOTE_CAND_ROW_BYTES, stats_block = n_segs * (int64_t)kStatsBytes;
  const void* tab = nullptr;
  const double* gauss = nullptr;
  if (int rc = note_tables(h, &tab, &gauss)) return rc;
  uint8_t* unused = nullptr;
  int8_t* d_bend = nullptr;
  if (w.bends)
    if (int rc = reserve_candidates(h, T, &unused, &d_bend)) return rc;
  if (w.n_bands) {
    BP_HIP(h->sw_note.reserve((size_t)(w.n_bands * plane)));
    BP_HIP(h->sw_onset.reserve((size_t)plane));
  }
  BP_HIP(h->sw_bits.reserve((size_t)(n_keys * bits_plane)));
  BP_HIP(h->sw_stats.reserve((size_t)(n_keys * stats_block)));
  BP_HIP(h->clip_rows.reserve((size_t)n_segs + 1));
  // The decode table and, behind it, the two arrays the tracker's launches read by decode — the rows and the event records
  // before each — as ONE block and one copy, queued with the row offsets before the first launch: a copy from pageable memory
  // waits for the stream's earlier work.
  const size_t tab_bytes = (size_t)n * sizeof(NoteSweepDecode), pre_bytes = (size_t)(n + 1) * sizeof(int64_t);
  static_assert(sizeof(NoteSweepDecode) % sizeof(int64_t) == 0, "the arrays behind the table are aligned");
  w.block.assign(tab_bytes + 2 * pre_bytes, 0);
  BP_HIP(h->sw_tab.reserve(w.block.size()));
  NoteSweepDecode* recs = reinterpret_cast<NoteSweepDecode*>(w.block.data());
  for (int64_t j = 0; j < n; ++j) {
    NoteSweepDecode& d = recs[j];
    const int64_t seg = w.segment[(size_t)j];
    const int key = w.set_key[(size_t)w.params[(size_t)j]];
    d.first = offs[seg], d.rows = offs[seg + 1] - offs[seg], d.seg = w.seg[(size_t)j];
    if (d.rows == 0 || d.seg.skip) continue;  // (never reaches the tracker's body: nothing of a key is read)
    const int band = w.keys[(size_t)key].band;
    d.note = band >= 0 ? h->sw_note + band * plane : all.note;
    d.bits = h->sw_bits + key * bits_plane;
    d.stats = h->sw_stats + key * stats_block + seg * (int64_t)kStatsBytes;
  }
  std::memcpy(w.block.data() + tab_bytes, w.pool_rows.data(), pre_bytes);
  std::memcpy(w.block.data() + tab_bytes + pre_bytes, job.plan.ev_first.data(), pre_bytes);
  const int64_t* d_rows = reinterpret_cast<const int64_t*>(h->sw_tab + tab_bytes);
  BP_HIP(hipMemcpyAsync(h->clip_rows, offs, (size_t)(n_segs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  BP_HIP(hipMemcpyAsync(h->sw_tab, w.block.data(), w.block.size(), hipMemcpyHostToDevice, s));
  if (score && job.want_scores) {
    // The LDS of the scoring launch: the most refs a decode it scores can have, the deepest its path can get — min(events,
    // refs + 1), the events bounded by what the decode's region of the pool holds.  Its tables go with the tracker's.
    for (int64_t j = 0; j < n; ++j) {
      const int n_ref = w.ref_of[(size_t)j].n_ref;
      if (n_ref > kNoteScoreMaxNotes) continue;  // status 3: never searched
      const int64_t room = job.plan.ev_first[(size_t)j + 1] - job.plan.ev_first[(size_t)j];
      w.max_refs = std::max(w.max_refs, n_ref);
      w.max_depth = std::max(w.max_depth, (int)std::min<int64_t>({room, (int64_t)n_ref + 1, (int64_t)kNoteScoreMaxNotes}));
    }
    BP_HIP(h->sc_refs.reserve(w.refs.size()));
    BP_HIP(h->sc_out.reserve((size_t)(5 * n)));
    BP_HIP(h->sc_home.reserve((size_t)(5 * n)));
    if (!w.refs.empty())
      BP_HIP(hipMemcpyAsync(h->sc_refs, w.refs.data(), w.refs.size() * sizeof(NoteScoreRef), hipMemcpyHostToDevice, s));
  }
  if (score) {  // which refs are whose: both scoring launches read it
    BP_HIP(h->sc_dec.reserve((size_t)n));
    BP_HIP(hipMemcpyAsync(h->sc_dec, w.ref_of.data(), (size_t)n * sizeof(NoteScoreDecode), hipMemcpyHostToDevice, s));
  }
  if (score && job.want_frames) {  // the frame launch's table, its counts [decodes][5] with the statuses (32-bit) behind them
    BP_HIP(h->fs_refs.reserve(w.frame_refs.size()));
    BP_HIP(h->fs_out.reserve((size_t)(5 * n + (n + 1) / 2)));
    BP_HIP(h->fs_home.reserve((size_t)(5 * n + (n + 1) / 2)));
    if (!w.frame_refs.empty())
      BP_HIP(hipMemcpyAsync(h->fs_refs, w.frame_refs.data(), w.frame_refs.size() * sizeof(NoteFrameRef), hipMemcpyHostToDevice, s));
  }
  launch_clips_stats_init(h->sw_stats, n_keys * n_segs, s);
  int made = 0;  // bands whose copies exist; sw_onset holds the last one's
  for (int64_t i = 0; i < n_keys; ++i) {
    const SweepKey& key = w.keys[(size_t)i];
    float *note = all.note, *onset = all.onset;
    if (key.band >= 0) {
      note = h->sw_note + key.band * plane, onset = h->sw_onset;
      if (key.band == made) launch_constrain_copy(all.note, all.onset, note, onset, T, key.lo, key.hi, s), ++made;
    }
    launch_clips_candidates(note, onset, all.contour, h->clip_rows, n_segs, T, 0, kFreqN, key.infer, key.onset_thresh, tab, gauss,
                            h->sw_stats + i * stats_block, h->sw_bits + i * bits_plane, i == 0 ? d_bend : nullptr, s);
  }
  BP_HIP(hipGetLastError());
  if (score) {  // the events stay where the tracker leaves them: one more launch, and 20 bytes per decode go home
    BP_HIP(launch_note_track_sweep(h->sw_tab.as<NoteSweepDecode>(), n, job.plan.max_rows, nullptr, d_rows, d_rows + n + 1, h->ev_scratch,
                                   h->ev_pool, nullptr, h->ev_counts, nullptr, nullptr, nullptr, s));
    const bp_score_params& p = *job.score_params;
    if (job.want_scores) {
      BP_HIP(launch_note_score(h->ev_counts, d_rows + n + 1, h->ev_pool, h->sc_dec, h->sc_refs,
                               NoteScoreParams{p.onset_tolerance_s, p.pitch_tolerance_cents, p.strict != 0}, n, w.max_refs, w.max_depth,
                               h->sc_out, s));
      BP_HIP(hipMemcpyAsync(h->sc_home, h->sc_out, (size_t)(5 * n) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    if (job.want_frames) {  // 40 bytes more per decode; the statuses too where the note-matching launch was skipped
      BP_HIP(launch_note_frames(h->ev_counts, d_rows, d_rows + n + 1, h->ev_pool, h->sc_dec, h->fs_refs, n, job.plan.max_rows, h->fs_out, s));
      const size_t bytes = (size_t)(5 * n) * sizeof(int64_t) + (job.want_scores ? 0 : (size_t)n * sizeof(int32_t));
      BP_HIP(hipMemcpyAsync(h->fs_home, h->fs_out, bytes, hipMemcpyDeviceToHost, s));
    }
    return BP_OK;
  }
  BP_HIP(launch_note_track_sweep(h->sw_tab.as<NoteSweepDecode>(), n, job.plan.max_rows, d_bend, d_rows, d_rows + n + 1, h->ev_scratch,
                                 h->ev_pool, h->bd_pool, h->ev_counts, h->ev_meta, h->ev_out, h->bd_out, s));
  BP_HIP(hipMemcpyAsync(h->ev_home, h->ev_meta, (size_t)(3 * n + 2) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  return BP_OK;
}

// ---- multi-pitch estimates: the f0 peaks of the contour rows (include/basic_pitch_amd_multipitch.h) ---------------
MpParams mp_device_params(const bp_mp_params& p) { return MpParams{p.threshold, p.min_bin, p.max_bin, 0}; }

// the sink's fixed arguments, before anything is queued
int check_multipitch(bp_handle h, const char* what, int64_t n_segs, const JobSink& k) {
  auto invalid = [&](const std::string& why) { return ::invalid(h, what, why); };
  if (k.kind == kMultiPitchHome) {
    if (n_segs < 0 || !k.point_offsets || (n_segs > 0 && !k.out.status))
      return invalid("negative n_segments / n_clips, null point_offsets or status");
    if (k.max_points < 0 || (k.max_points > 0 && !k.points)) return invalid("negative max_points, or room without a buffer");
    if (const char* why = bp_internal_mp_bad_params(k.mp_params)) return invalid(std::string("params: ") + why);
    return BP_OK;
  }
  if (n_segs < 0 || k.n_sets < 0 || k.n_decodes < 0 || (k.n_sets > 0 && !k.mp_params) || (k.n_decodes > 0 && !k.out.status))
    return invalid("negative n_segments / n_clips, n_sets or n_decodes, null sets or status");
  if (k.n_decodes > BP_SWEEP_MAX_DECODES)
    return invalid(std::to_string(k.n_decodes) + " decodes, more than BP_SWEEP_MAX_DECODES (" + std::to_string(BP_SWEEP_MAX_DECODES) +
                   "): split the job");
  for (int64_t p = 0; p < k.n_sets; ++p)
    if (const char* why = bp_internal_mp_bad_params(k.mp_params + p)) return invalid("set " + std::to_string(p) + ": " + why);
  if (int rc = check_decode_table(h, what, n_segs, k.n_sets, k.n_decodes, k.decodes)) return rc;
  return check_score(h, what, n_segs, k);
}

// The outputs against the rows (offs: of the n segments).  *queued false: nothing needs the device and the outputs are
// complete.  A scored sweep: the decode table, and per segment its refs in ascending pitch with the frames they sound on, by the
// checker's own function.
int plan_multipitch(bp_handle h, const char* what, int64_t n, const int64_t* offs, const JobSink& k, ClipsJob& job, bool* queued) {
  const auto too_many = [&](int64_t rows) {
    return invalid(h, what, std::to_string(rows) + " rows in all, more than BP_SWEEP_MAX_ROWS (" + std::to_string(BP_SWEEP_MAX_ROWS) +
                                "): split the job");
  };
  if (k.kind == kMultiPitchHome) {
    if (offs[n] > BP_SWEEP_MAX_ROWS) return too_many(offs[n]);
    *queued = offs[n] > 0;
    for (int64_t i = 0; i <= n && !*queued; ++i) k.point_offsets[i] = 0;
    for (int64_t i = 0; i < n && !*queued; ++i) k.out.status[i] = 0;
    return BP_OK;
  }
  job.mp_dec.resize((size_t)k.n_decodes);
  int64_t rows_in_all = 0;
  for (int64_t j = 0; j < k.n_decodes; ++j) {
    const int64_t i = k.decodes ? k.decodes[j].segment : j % n;
    const int32_t p = k.decodes ? k.decodes[j].params : (int32_t)(j / n);
    const int64_t first = k.ref_offsets[i];
    job.mp_dec[(size_t)j] = MpDecode{offs[i], offs[i + 1] - offs[i], first,
                                     (int32_t)std::min<int64_t>(k.ref_offsets[i + 1] - first, kNoteScoreMaxNotes + 1), p};
    rows_in_all += offs[i + 1] - offs[i];
  }
  if (rows_in_all > BP_SWEEP_MAX_ROWS) return too_many(rows_in_all);
  *queued = rows_in_all > 0;
  if (!*queued) {  // (every decode is of a segment without rows)
    for (int64_t j = 0; j < k.n_decodes; ++j) {
      k.frames[j] = bp_frame_score{0, 0, 0, 0, 0};
      k.out.status[j] = job.mp_dec[(size_t)j].n_ref > kNoteScoreMaxNotes ? 3 : 0;
    }
    return BP_OK;
  }
  job.mp_refs.resize((size_t)k.ref_offsets[n]);
  std::vector<int64_t> order;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t first = k.ref_offsets[i], rows = offs[i + 1] - offs[i];
    order.resize((size_t)(k.ref_offsets[i + 1] - first));
    for (size_t r = 0; r < order.size(); ++r) order[r] = first + (int64_t)r;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return k.refs[a].pitch_midi < k.refs[b].pitch_midi; });
    for (size_t r = 0; r < order.size(); ++r) {
      const bp_ref_note& ref = k.refs[order[r]];
      int64_t f0 = 0, f1 = 0;
      bp_internal_frame_interval(ref.start_s, ref.end_s, rows, &f0, &f1);
      job.mp_refs[(size_t)first + r] = MpRef{(int32_t)f0, (int32_t)f1, ref.pitch_midi};  // (rows <= BP_SWEEP_MAX_ROWS)
    }
  }
  return BP_OK;
}

// Behind the contour rows of the n segments (on the device, T > 0 in all).  The points: the count pass, the scan, and the
// offsets and statuses on their way home — the write pass waits for the host's look at the total (multipitch_home).  A scored
// sweep: its tables, its one launch, the counts with the statuses on their way home.
int queue_multipitch(bp_handle h, const float* contour, int64_t n, const int64_t* offs, const JobSink& k, ClipsJob& job) {
  hipStream_t s = h->stream;
  const int64_t T = offs[n];
  job.mp_contour = contour;
  if (k.kind == kMultiPitchHome) {
    const size_t n_meta = (size_t)(n + 1 + (n + 1) / 2);
    BP_HIP(h->clip_rows.reserve((size_t)n + 1));
    BP_HIP(h->mp_rows.reserve((size_t)T));
    BP_HIP(h->mp_first.reserve((size_t)T + 1));
    BP_HIP(h->mp_bad.reserve((size_t)n));
    BP_HIP(h->mp_meta.reserve(n_meta));
    BP_HIP(h->mp_home.reserve(n_meta));
    BP_HIP(hipMemcpyAsync(h->clip_rows, offs, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    BP_HIP(hipMemsetAsync(h->mp_bad, 0, (size_t)n * sizeof(int32_t), s));
    BP_HIP(launch_mp_count(contour, h->clip_rows, n, T, mp_device_params(*k.mp_params), h->mp_rows, h->mp_bad, s));
    BP_HIP(launch_mp_scan(h->mp_rows, h->mp_bad, h->clip_rows, n, T, h->mp_first, h->mp_meta, s));
    BP_HIP(hipMemcpyAsync(h->mp_home, h->mp_meta, n_meta * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return BP_OK;
  }
  const int64_t nd = k.n_decodes;
  const size_t n_out = (size_t)(5 * nd + (nd + 1) / 2);
  int64_t max_rows = 0;
  for (const MpDecode& d : job.mp_dec) max_rows = std::max(max_rows, d.rows);
  static_assert(sizeof(MpParams) == sizeof(bp_mp_params), "the sets go to the device as they are");
  BP_HIP(h->mp_sets.reserve((size_t)k.n_sets));
  BP_HIP(h->mp_dec.reserve((size_t)nd));
  BP_HIP(h->mp_refs.reserve(job.mp_refs.size()));
  BP_HIP(h->mp_out.reserve(n_out));
  BP_HIP(h->mp_home.reserve(n_out));
  BP_HIP(hipMemcpyAsync(h->mp_sets, k.mp_params, (size_t)k.n_sets * sizeof(MpParams), hipMemcpyHostToDevice, s));
  BP_HIP(hipMemcpyAsync(h->mp_dec, job.mp_dec.data(), (size_t)nd * sizeof(MpDecode), hipMemcpyHostToDevice, s));
  if (!job.mp_refs.empty())
    BP_HIP(hipMemcpyAsync(h->mp_refs, job.mp_refs.data(), job.mp_refs.size() * sizeof(MpRef), hipMemcpyHostToDevice, s));
  BP_HIP(launch_mp_sweep_frames(contour, h->mp_sets, h->mp_dec, h->mp_refs,
                                MpScoreParams{k.score_params->pitch_tolerance_cents, k.score_params->strict != 0}, nd, max_rows, h->mp_out, s));
  BP_HIP(hipMemcpyAsync(h->mp_home, h->mp_out, n_out * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  return BP_OK;
}

// The stream has drained.  The points: the offsets and statuses are in the page-locked block; when the total fits the
// caller's room, the write pass and the points home, and the wait for them.  A scored sweep: the counts and statuses.
int multipitch_home(bp_handle h, const char* what, int64_t n, const int64_t* offs, const JobSink& k, const ClipsJob& job) {
  if (k.kind == kMultiPitchScoreHome) {
    std::memcpy(k.frames, h->mp_home, (size_t)k.n_decodes * sizeof(bp_frame_score));
    const int32_t* st = reinterpret_cast<const int32_t*>(h->mp_home + 5 * k.n_decodes);
    for (int64_t j = 0; j < k.n_decodes; ++j) k.out.status[j] = st[j];
    return BP_OK;
  }
  const int64_t* meta = h->mp_home;
  const int32_t* st = reinterpret_cast<const int32_t*>(meta + n + 1);
  const int64_t total = meta[n];
  for (int64_t i = 0; i <= n; ++i) k.point_offsets[i] = meta[i];
  for (int64_t i = 0; i < n; ++i) k.out.status[i] = st[i];
  if (total > k.max_points) {
    h->err = std::string(what) + ": output buffer too small: " + std::to_string(total) +
             " points are needed (point_offsets[n] holds them; nothing has been written to points)";
    return BP_ERR_INVALID_ARG;
  }
  if (total == 0) return BP_OK;
  auto write = [&]() -> int {
    BP_HIP(h->mp_points.reserve((size_t)total * sizeof(bp_f0_point)));
    BP_HIP(launch_mp_write(job.mp_contour, offs[n], mp_device_params(*k.mp_params), h->mp_rows, h->mp_bad, h->clip_rows, h->mp_first,
                           h->mp_points, h->stream));
    BP_HIP(hipMemcpyAsync(k.points, h->mp_points, (size_t)total * sizeof(bp_f0_point), hipMemcpyDeviceToHost, h->stream));
    return BP_OK;
  };
  return finish(h, write());
}

// ---- the melody: one f0 track per segment by a Viterbi recurrence (include/basic_pitch_amd_melody.h) ---------------
// the sink's fixed arguments, before anything is queued
int check_melody(bp_handle h, const char* what, int64_t n_segs, const JobSink& k) {
  auto invalid = [&](const std::string& why) { return ::invalid(h, what, why); };
  if (k.kind == kMelodyHome) {
    if (n_segs < 0 || (n_segs > 0 && !k.out.status)) return invalid("negative n_segments / n_clips, or null status");
    if (k.max_points < 0 || (k.max_points > 0 && !k.mel_points)) return invalid("negative max_points, or room without a buffer");
    if (const char* why = bp_internal_melody_bad_params(k.mel_params)) return invalid(std::string("params: ") + why);
    return BP_OK;
  }
  if (n_segs < 0 || k.n_sets < 0 || k.n_decodes < 0 || (k.n_sets > 0 && !k.mel_params) || (k.n_decodes > 0 && (!k.out.status || !k.mel_scores)))
    return invalid("negative n_segments / n_clips, n_sets or n_decodes, null sets, scores or status");
  if (k.n_decodes > BP_SWEEP_MAX_DECODES)
    return invalid(std::to_string(k.n_decodes) + " decodes, more than BP_SWEEP_MAX_DECODES (" + std::to_string(BP_SWEEP_MAX_DECODES) +
                   "): split the job");
  for (int64_t p = 0; p < k.n_sets; ++p)
    if (const char* why = bp_internal_melody_bad_params(k.mel_params + p)) return invalid("set " + std::to_string(p) + ": " + why);
  if (int rc = check_decode_table(h, what, n_segs, k.n_sets, k.n_decodes, k.decodes)) return rc;
  if (const char* why = bp_internal_score_bad_params(k.score_params)) return invalid(why);
  return BP_OK;
}

// The outputs against the rows (offs: of the n segments): the room, the reference track, the bound, the decode table with
// every decode's region of the predecessor pool.  *queued false: nothing needs the device and the outputs are complete.
int plan_melody(bp_handle h, const char* what, int64_t n, const int64_t* offs, const JobSink& k, ClipsJob& job, bool* queued) {
  auto invalid = [&](const std::string& why) { return ::invalid(h, what, why); };
  const auto too_many = [&](int64_t rows) {
    return invalid(std::to_string(rows) + " rows in all, more than BP_SWEEP_MAX_ROWS (" + std::to_string(BP_SWEEP_MAX_ROWS) + "): split the job");
  };
  if (k.kind == kMelodyHome) {
    if (offs[n] > BP_SWEEP_MAX_ROWS) return too_many(offs[n]);
    if (k.max_points < offs[n])
      return invalid("room for " + std::to_string(k.max_points) + " records, but the segments have " + std::to_string(offs[n]) +
                     " rows and a row is a record (nothing has been written)");
    *queued = offs[n] > 0;
    for (int64_t i = 0; i < n; ++i) k.out.status[i] = 0;
    for (int64_t i = 0; i < n && *queued; ++i)
      if (offs[i + 1] > offs[i]) job.mel_dec.push_back(MelodyDecode{offs[i], offs[i + 1] - offs[i], offs[i], 0, (int32_t)i});
    return BP_OK;
  }
  if (offs[n] > 0 && !k.ref_pitch) return invalid("null ref_pitch");
  const int64_t bad = bp_internal_melody_bad_ref(k.ref_pitch, offs[n]);
  if (bad >= 0) return invalid("ref_pitch " + std::to_string(bad) + ": negative or not finite");
  job.mel_dec.resize((size_t)k.n_decodes);
  int64_t rows_in_all = 0;
  for (int64_t j = 0; j < k.n_decodes; ++j) {
    const int64_t i = k.decodes ? k.decodes[j].segment : j % n;
    const int32_t p = k.decodes ? k.decodes[j].params : (int32_t)(j / n);
    job.mel_dec[(size_t)j] = MelodyDecode{offs[i], offs[i + 1] - offs[i], rows_in_all, p, 0};
    rows_in_all += offs[i + 1] - offs[i];
    if (rows_in_all > BP_SWEEP_MAX_ROWS) return too_many(rows_in_all);
  }
  *queued = rows_in_all > 0;
  for (int64_t j = 0; j < k.n_decodes && !*queued; ++j) k.mel_scores[j] = bp_melody_score{0, 0, 0, 0, 0, 0}, k.out.status[j] = 0;
  return BP_OK;
}

// Behind the contour rows of the n segments (on the device, T > 0 in all): the tables, the one launch, and the records or
// the counts with the statuses on their way home.  kMelodyHome: the `reserved` word of a decode is its segment (the kernel
// does not read it), and the statuses come home per decode.
int queue_melody(bp_handle h, const float* contour, int64_t n, const int64_t* offs, const JobSink& k, ClipsJob& job) {
  hipStream_t s = h->stream;
  const bool scored = k.kind == kMelodyScoreHome;
  const int64_t nd = (int64_t)job.mel_dec.size(), n_sets = scored ? k.n_sets : 1;
  int64_t pred_rows = 0;
  int max_jump = 0;  // of the sets a decode names
  for (const MelodyDecode& d : job.mel_dec) pred_rows += d.rows, max_jump = std::max(max_jump, (int)k.mel_params[d.set].max_jump);
  static_assert(sizeof(MelodyParams) == sizeof(bp_melody_params), "the sets go to the device as they are");
  const size_t n_out = (size_t)((scored ? 6 * nd : 0) + (nd + 1) / 2);
  BP_HIP(h->mel_sets.reserve((size_t)n_sets));
  BP_HIP(h->mel_dec.reserve((size_t)nd));
  BP_HIP(h->mel_pred.reserve((size_t)pred_rows * kMelodyPredStride));
  BP_HIP(h->mel_out.reserve(n_out));
  BP_HIP(h->mel_home.reserve(n_out));
  BP_HIP(hipMemcpyAsync(h->mel_sets, k.mel_params, (size_t)n_sets * sizeof(MelodyParams), hipMemcpyHostToDevice, s));
  BP_HIP(hipMemcpyAsync(h->mel_dec, job.mel_dec.data(), (size_t)nd * sizeof(MelodyDecode), hipMemcpyHostToDevice, s));
  int64_t* out = h->mel_out;
  if (scored) {
    BP_HIP(h->mel_ref.reserve((size_t)offs[n]));
    BP_HIP(hipMemcpyAsync(h->mel_ref, k.ref_pitch, (size_t)offs[n] * sizeof(double), hipMemcpyHostToDevice, s));
    BP_HIP(launch_melody(contour, h->mel_sets, h->mel_dec, nd, max_jump, h->mel_pred, nullptr, h->mel_ref,
                         MpScoreParams{k.score_params->pitch_tolerance_cents, k.score_params->strict != 0}, out,
                         reinterpret_cast<int32_t*>(out + 6 * nd), s));
  } else {
    BP_HIP(h->mel_points.reserve((size_t)offs[n] * sizeof(bp_melody_point)));
    BP_HIP(launch_melody(contour, h->mel_sets, h->mel_dec, nd, max_jump, h->mel_pred, h->mel_points, nullptr, MpScoreParams{0.0, false}, nullptr,
                         reinterpret_cast<int32_t*>(out), s));
    BP_HIP(hipMemcpyAsync(k.mel_points, h->mel_points, (size_t)offs[n] * sizeof(bp_melody_point), hipMemcpyDeviceToHost, s));
  }
  BP_HIP(hipMemcpyAsync(h->mel_home, out, n_out * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  return BP_OK;
}

// the stream has drained: the statuses, and a scored sweep's counts, are in the page-locked block
void melody_home(bp_handle h, const JobSink& k, const ClipsJob& job) {
  const int64_t nd = (int64_t)job.mel_dec.size();
  if (k.kind == kMelodyScoreHome) {
    std::memcpy(k.mel_scores, h->mel_home, (size_t)nd * sizeof(bp_melody_score));
    const int32_t* st = reinterpret_cast<const int32_t*>(h->mel_home + 6 * nd);
    for (int64_t j = 0; j < nd; ++j) k.out.status[j] = st[j];
    return;
  }
  const int32_t* st = reinterpret_cast<const int32_t*>(static_cast<int64_t*>(h->mel_home));
  for (int64_t j = 0; j < nd; ++j) k.out.status[job.mel_dec[(size_t)j].reserved] = st[j];
}

// ---- forced alignment: the states of a score against the note and onset rows (include/basic_pitch_amd_align.h) ---
// the sink's fixed arguments, before anything is queued
int check_align(bp_handle h, const char* what, int64_t n_segs, const JobSink& k) {
  auto invalid = [&](const std::string& why) { return ::invalid(h, what, why); };
  if (n_segs < 0 || (n_segs > 0 && (!k.out.status || !k.al_total))) return invalid("negative n_segments / n_clips, or null total or status");
  if (const char* why = bp_internal_align_bad_params(k.al_params)) return invalid(std::string("params: ") + why);
  if (n_segs == 0) return BP_OK;
  bool ordered = k.state_offsets && k.state_offsets[0] == 0;
  for (int64_t i = 0; ordered && i < n_segs; ++i) ordered = k.state_offsets[i + 1] >= k.state_offsets[i];
  if (!ordered) return invalid("state_offsets must start at 0 and never decrease");
  const int64_t n_states = k.state_offsets[n_segs];
  if (n_states > 0 && !k.al_states) return invalid("null states");
  if (k.max_states < 0 || (k.max_states > 0 && !k.first_frame)) return invalid("negative max_states, or room without a buffer");
  if (k.max_states < n_states)
    return invalid("room for " + std::to_string(k.max_states) + " first frames, but the segments have " + std::to_string(n_states) +
                   " states (nothing has been written)");
  for (int64_t i = 0; i < n_segs; ++i)
    if (k.state_offsets[i + 1] - k.state_offsets[i] > BP_ALIGN_MAX_STATES)
      return invalid("segment " + std::to_string(i) + ": " + std::to_string(k.state_offsets[i + 1] - k.state_offsets[i]) +
                     " states, more than BP_ALIGN_MAX_STATES (" + std::to_string(BP_ALIGN_MAX_STATES) + ")");
  int64_t bad = -1;
  if (const char* why = bp_internal_align_bad_states(k.al_states, n_states, &bad)) return invalid("state " + std::to_string(bad) + ": " + why);
  return BP_OK;
}

// The outputs against the rows (offs: of the n segments): the bounds, the results of the segments that need no device, and
// for the others their regions of the pools.  *queued false: nothing needs the device and the outputs are complete.
int plan_align(bp_handle h, const char* what, int64_t n, const int64_t* offs, const JobSink& k, ClipsJob& job, bool* queued) {
  auto invalid = [&](const std::string& why) { return ::invalid(h, what, why); };
  if (offs[n] > BP_SWEEP_MAX_ROWS)
    return invalid(std::to_string(offs[n]) + " rows in all, more than BP_SWEEP_MAX_ROWS (" + std::to_string(BP_SWEEP_MAX_ROWS) + "): split the job");
  int64_t cells = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t rows = offs[i + 1] - offs[i], S = k.state_offsets[i + 1] - k.state_offsets[i];
    if (rows > 0 && S == 0) return invalid("segment " + std::to_string(i) + ": rows but no state (a path needs a state)");
    cells += rows * S;  // (at most 2^23 x 2^12 a segment: no overflow before the test)
    if (cells > BP_ALIGN_MAX_CELLS)
      return invalid(std::to_string(cells) + " cells (rows x states) up to segment " + std::to_string(i) + ", more than BP_ALIGN_MAX_CELLS (" +
                     std::to_string(BP_ALIGN_MAX_CELLS) + "): split the job");
  }
  for (int64_t i = 0; i < n; ++i) {
    const int64_t rows = offs[i + 1] - offs[i], S = k.state_offsets[i + 1] - k.state_offsets[i];
    k.al_total[i] = 0, k.out.status[i] = rows == 0 && S > 0 ? 2 : 0;  // (states without a row: infeasible)
    for (int64_t j = 0; j < S; ++j) k.first_frame[k.state_offsets[i] + j] = -1;
    if (rows == 0 || S == 0) continue;
    job.al_segs.push_back(AlignSeg{offs[i], rows, k.state_offsets[i], job.al_cells, job.al_words, job.al_tiles, (int32_t)S, (int32_t)i});
    job.al_cells += rows * S, job.al_words += rows * ((S + 63) / 64);
    job.al_tiles += ((rows + kAlignEmitRows - 1) / kAlignEmitRows) * ((S + kAlignEmitRows - 1) / kAlignEmitRows);
    job.al_max_states = std::max(job.al_max_states, (int)S);
  }
  *queued = !job.al_segs.empty();
  return BP_OK;
}

// Behind the note and onset rows of the n segments (on the device, 16-byte aligned): the tables, the launches, and the first
// frames, totals and statuses on their way home.
int queue_align(bp_handle h, const float* note, const float* onset, int64_t n, const JobSink& k, ClipsJob& job) {
  hipStream_t s = h->stream;
  const int64_t nd = (int64_t)job.al_segs.size(), n_states = k.state_offsets[n];
  static_assert(sizeof(AlignState) == sizeof(bp_align_state) && sizeof(bp_align_state) == 40, "the states go to the device as they are");
  const size_t n_out = (size_t)(nd + (nd + 1) / 2);
  BP_HIP(h->al_states.reserve((size_t)n_states));
  BP_HIP(h->al_segs.reserve((size_t)nd));
  BP_HIP(h->al_gains.reserve((size_t)job.al_cells * 8));
  BP_HIP(h->al_pred.reserve((size_t)job.al_words));
  BP_HIP(h->al_nan.reserve((size_t)nd));
  BP_HIP(h->al_first.reserve((size_t)n_states));
  BP_HIP(h->al_out.reserve(n_out));
  BP_HIP(h->al_home.reserve(n_out));
  BP_HIP(hipMemcpyAsync(h->al_states, k.al_states, (size_t)n_states * sizeof(AlignState), hipMemcpyHostToDevice, s));
  BP_HIP(hipMemcpyAsync(h->al_segs, job.al_segs.data(), (size_t)nd * sizeof(AlignSeg), hipMemcpyHostToDevice, s));
  // (the first frames of the segments that are not queued are -1 already, on the host and here)
  BP_HIP(hipMemsetAsync(h->al_first, 0xff, (size_t)n_states * sizeof(int32_t), s));
  int64_t* out = h->al_out;
  BP_HIP(launch_align(note, onset, h->al_states, h->al_segs, nd, job.al_tiles, job.al_max_states, k.al_params->threshold_q,
                      k.al_params->onset_weight, static_cast<uint8_t*>(h->al_gains), h->al_pred, h->al_nan, h->al_first, out,
                      reinterpret_cast<int32_t*>(out + nd), s));
  BP_HIP(hipMemcpyAsync(k.first_frame, h->al_first, (size_t)n_states * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  BP_HIP(hipMemcpyAsync(h->al_home, out, n_out * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  return BP_OK;
}

// the stream has drained: the totals and the statuses are in the page-locked block
void align_home(bp_handle h, const JobSink& k, const ClipsJob& job) {
  const int64_t nd = (int64_t)job.al_segs.size();
  const int32_t* st = reinterpret_cast<const int32_t*>(h->al_home + nd);
  for (int64_t c = 0; c < nd; ++c) {
    const int32_t i = job.al_segs[(size_t)c].segment;
    k.al_total[i] = h->al_home[c], k.out.status[i] = st[c];
  }
}

// ---- tempo and beats: the onset rows alone (include/basic_pitch_amd_beat.h) -----------------------------------------
// the sink's fixed arguments, before anything is queued
int check_beat(bp_handle h, const char* what, int64_t n_segs, const JobSink& k) {
  auto invalid = [&](const std::string& why) { return ::invalid(h, what, why); };
  if (n_segs < 0 || (n_segs > 0 && (!k.bt_summaries || !k.bt_offsets))) return invalid("negative n_segments / n_clips, or null summaries or beat_offsets");
  if (const char* why = bp_internal_beat_bad_params(k.bt_params)) return invalid(std::string("params: ") + why);
  if (k.max_beats < 0 || (k.max_beats > 0 && !k.bt_beats)) return invalid("negative max_beats, or room without a buffer");
  return BP_OK;
}

// The outputs against the rows (offs: of the n segments): the bounds, the room, the results of the segments without rows, and
// for the others their blocks, tiles and regions of the beat pool.  *queued false: nothing needs the device and the outputs
// are complete.
int plan_beat(bp_handle h, const char* what, int64_t n, const int64_t* offs, const JobSink& k, ClipsJob& job, bool* queued) {
  auto invalid = [&](const std::string& why) { return ::invalid(h, what, why); };
  if (offs[n] > BP_SWEEP_MAX_ROWS)
    return invalid(std::to_string(offs[n]) + " rows in all, more than BP_SWEEP_MAX_ROWS (" + std::to_string(BP_SWEEP_MAX_ROWS) + "): split the job");
  const bp_beat_params& p = *k.bt_params;
  int64_t cap = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t rows = offs[i + 1] - offs[i];
    if (rows > BP_BEAT_MAX_ROWS)
      return invalid("segment " + std::to_string(i) + ": " + std::to_string(rows) + " rows, more than BP_BEAT_MAX_ROWS (" +
                     std::to_string(BP_BEAT_MAX_ROWS) + ")");
    cap += bp_beats_capacity(rows, p.lag_min);
  }
  if (k.max_beats < cap)
    return invalid("room for " + std::to_string(k.max_beats) + " beats, but the segments can have " + std::to_string(cap) +
                   " (the sum of bp_beats_capacity; nothing has been written)");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t rows = offs[i + 1] - offs[i];
    k.bt_summaries[i] = bp_beat_summary{rows == 0 ? 2 : 0, 0, 0, 0, 0.0};  // (no row: no pulse)
    if (rows == 0) continue;
    const int64_t last_lag = std::min<int64_t>(p.lag_max, rows - 1), room = bp_beats_capacity(rows, p.lag_min);
    const int32_t lag_tiles = last_lag < p.lag_min ? 0 : (int32_t)((last_lag - p.lag_min + kBeatTempoLags) / kBeatTempoLags);
    job.bt_segs.push_back(BeatSeg{offs[i], rows, job.bt_blocks, job.bt_tiles, job.bt_cap, room, lag_tiles, (int32_t)i});
    job.bt_blocks += (rows + kBeatStrengthRows - 1) / kBeatStrengthRows;
    job.bt_tiles += (rows + kBeatTempoRows - 1) / kBeatTempoRows * lag_tiles;
    job.bt_cap += room;
  }
  *queued = !job.bt_segs.empty();
  for (int64_t i = 0; i <= n && !*queued && k.bt_offsets; ++i) k.bt_offsets[i] = 0;  // (null: a call of zero segments may pass none)
  return BP_OK;
}

// Behind the onset rows of the n segments (on the device, 16-byte aligned): the tables, the three launches, and the summaries
// and the beat pool on their way home (one page-locked block: the summaries, then the pool).
int queue_beat(bp_handle h, const float* onset, int64_t n, const JobSink& k, ClipsJob& job) {
  hipStream_t s = h->stream;
  const int64_t nd = (int64_t)job.bt_segs.size(), rows = job.offs[n];
  static_assert(sizeof(BeatParams) == sizeof(bp_beat_params) && sizeof(bp_beat_params) == 1064, "the parameters go to the device as they are");
  static_assert(sizeof(BeatSummary) == sizeof(bp_beat_summary) && sizeof(bp_beat_summary) == 32, "the summaries come home as they are");
  const size_t n_home = (size_t)(4 * nd + (job.bt_cap + 1) / 2);  // in int64: 32 bytes a summary, 4 a beat
  BP_HIP(h->bt_params.reserve(1));
  BP_HIP(h->bt_segs.reserve((size_t)nd));
  BP_HIP(h->bt_strength.reserve((size_t)rows));
  BP_HIP(h->bt_acc.reserve((size_t)nd * kBeatAccStride));
  BP_HIP(h->bt_pred.reserve((size_t)rows));
  BP_HIP(h->bt_out.reserve(n_home));
  BP_HIP(h->bt_home.reserve(n_home));
  BP_HIP(hipMemcpyAsync(h->bt_params, k.bt_params, sizeof(BeatParams), hipMemcpyHostToDevice, s));
  BP_HIP(hipMemcpyAsync(h->bt_segs, job.bt_segs.data(), (size_t)nd * sizeof(BeatSeg), hipMemcpyHostToDevice, s));
  int64_t* out = h->bt_out;
  BP_HIP(launch_beats(onset, h->bt_params, h->bt_segs, nd, job.bt_blocks, job.bt_tiles, h->bt_strength, h->bt_acc, h->bt_pred,
                      reinterpret_cast<int32_t*>(out + 4 * nd), reinterpret_cast<BeatSummary*>(out), s));
  BP_HIP(hipMemcpyAsync(h->bt_home, out, n_home * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  return BP_OK;
}

// the stream has drained: the summaries and the pool are in the page-locked block; the beats leave it compact and ascending
// (a segment's lie in its region of the pool last beat first)
void beat_home(bp_handle h, int64_t n, const JobSink& k, const ClipsJob& job) {
  const int64_t nd = (int64_t)job.bt_segs.size();
  const int64_t* home = h->bt_home;
  const int32_t* pool = reinterpret_cast<const int32_t*>(home + 4 * nd);
  for (int64_t c = 0; c < nd; ++c) std::memcpy(&k.bt_summaries[job.bt_segs[(size_t)c].segment], home + 4 * c, sizeof(bp_beat_summary));
  int64_t at = 0, c = 0;
  for (int64_t i = 0; i < n; ++i) {
    k.bt_offsets[i] = at;
    if (c < nd && job.bt_segs[(size_t)c].segment == i) {
      const BeatSeg& seg = job.bt_segs[(size_t)c++];
      const int64_t nb = std::min(k.bt_summaries[i].n_beats, seg.beat_cap);  // (n_beats is within the room by the header's bound)
      for (int64_t j = 0; j < nb; ++j) k.bt_beats[at + j] = pool[seg.beat_first + nb - 1 - j];
      at += nb;
    }
  }
  k.bt_offsets[n] = at;
}

// everything a job queues: the source (the maps of all segments to track_out, concatenated by job.offs), the dense half of
// note decoding for every segment as its own track, the sink
int queue_job(bp_handle h, const JobSource& s, const JobSink& k, ClipsJob& job) {
  Maps all{};
  int rc = BP_OK;
  const bool multipitch = k.kind == kMultiPitchHome || k.kind == kMultiPitchScoreHome;
  const bool melody = k.kind == kMelodyHome || k.kind == kMelodyScoreHome;
  if (s.kind == kGivenMaps && (k.kind == kAlignHome || k.kind == kBeatHome)) {
    // the note and onset rows alone (the beats: the onset rows), read where they lie unless they are in host memory or not
    // 16-byte aligned
    const size_t cells = (size_t)job.offs[s.n] * kFreqN;
    const auto where = [&](const float* given, DeviceBuffer<float>& copy, float** at) -> int {
      *at = const_cast<float*>(given);
      if (s.mem_kind == BP_MEM_DEVICE && reinterpret_cast<uintptr_t>(given) % 16 == 0) return BP_OK;
      BP_HIP(copy.reserve(cells));
      BP_HIP(hipMemcpyAsync(copy, given, cells * sizeof(float), s.mem_kind == BP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->stream));
      *at = copy;
      return BP_OK;
    };
    if (k.kind == kBeatHome) {
      if ((rc = where(s.onset, h->bt_onset, &all.onset))) return rc;
    } else if ((rc = where(s.note, h->al_note, &all.note)) || (rc = where(s.onset, h->al_onset, &all.onset))) {
      return rc;
    }
  } else if (s.kind == kGivenMaps && (multipitch || melody)) {
    // the contour rows alone, read where they lie: a map in host memory gets a device copy, one in device memory is not copied
    all.contour = const_cast<float*>(s.contour);
    if (s.mem_kind == BP_MEM_HOST) {
      auto& copy = melody ? h->mel_contour : h->mp_contour;
      const size_t cells = (size_t)job.offs[s.n] * kFreqC;
      BP_HIP(copy.reserve(cells));
      BP_HIP(hipMemcpyAsync(copy, s.contour, cells * sizeof(float), hipMemcpyHostToDevice, h->stream));
      all.contour = copy;
    }
  } else if (s.kind == kGivenMaps) {
    rc = take_given_maps(h, s.note, s.onset, s.contour, job.offs[s.n], s.mem_kind, &all);
  } else {
    const bp_clip* clips = s.clips;
    if (s.kind == kFlacClips) {
      // the decoded clips as the PCM clips calls take them: device memory, a clip left to the host without frames
      const FlacJob& f = job.flac;
      if ((rc = queue_flac_clips(h, s.flac, f))) return rc;
      job.decoded.assign(f.dev.size(), bp_clip{nullptr, 0, BP_PCM_S16, 1});
      for (size_t i = 0; i < f.dev.size(); ++i)
        if (f.dev[i] >= 0)
          job.decoded[i] = bp_clip{h->pcm_dev + f.tab[(size_t)f.dev[i]].pcm_off, f.lay[i].n_frames, flac_format(f.lay[i]), f.lay[i].channels};
      clips = job.decoded.data();
    } else if (s.kind == kAdpcmClips) {
      AdpcmJob& a = job.adpcm;
      if ((rc = queue_adpcm(h, s.n, a.files.data(), a.lay.data(), a.segs, a.pcm_off.data()))) return rc;
      job.decoded.assign((size_t)s.n, bp_clip{nullptr, 0, BP_PCM_S16, 1});
      for (size_t i = 0; i < a.lay.size(); ++i)
        if (a.lay[i].n_frames > 0) job.decoded[i] = bp_clip{h->ad.pcm + a.pcm_off[i], a.lay[i].n_frames, BP_PCM_S16, a.lay[i].channels};
      clips = job.decoded.data();
    }
    job.tab.resize((size_t)s.n);
    rc = queue_clips_maps(h, s.n, clips, s.sample_rate, s.kind != kPcmClips ? BP_MEM_DEVICE : s.mem_kind, job.flac.n_model.data(),
                          job.offs, job.tab, &all);
  }
  if (rc) return rc;
  if (multipitch) return queue_multipitch(h, all.contour, s.n, job.offs, k, job);
  if (melody) return queue_melody(h, all.contour, s.n, job.offs, k, job);
  if (k.kind == kAlignHome) return queue_align(h, all.note, all.onset, s.n, k, job);
  if (k.kind == kBeatHome) return queue_beat(h, all.onset, s.n, k, job);
  if (k.kind == kCandidatesHome)
    return queue_clips_candidates(h, all, s.n, job.offs, k.params, k.note_out, k.cand_bits, k.bend_map, &job.exported_by_kernel);
  uint8_t* d_bits = nullptr;
  int8_t* d_bend = nullptr;
  const bool score = k.kind == kScoreHome;
  if ((rc = events_reserve(h, job.ev, &job.plan, !score))) return rc;
  if (k.kind == kSweepHome || score) return queue_sweep(h, all, s.n, job.offs, job, score);
  if ((rc = queue_clips_dense(h, all, s.n, job.offs, k.params, job.dense_bends, &d_bits, &d_bend))) return rc;
  return events_queue(h, job.ev, job.plan, TrackInputs{all.note, d_bits, d_bend, h->clip_rows, h->clip_stats});
}

int run_clips(bp_handle h, const char* what, JobSource src, const JobSink& k) {
  if (!h) return BP_ERR_INVALID_ARG;
  auto invalid = [&](const char* why) { return ::invalid(h, what, why); };
  const int64_t n = src.n;
  const bool flac = src.kind == kFlacClips, score = k.kind == kScoreHome, sweep = k.kind == kSweepHome || score;
  const bool events = k.kind == kEventsHome || sweep;
  const bool multipitch = k.kind == kMultiPitchHome || k.kind == kMultiPitchScoreHome;
  const bool melody = k.kind == kMelodyHome || k.kind == kMelodyScoreHome;
  const bool align = k.kind == kAlignHome, beat = k.kind == kBeatHome;
  int rc = BP_OK;
  // the sink's fixed arguments
  if (beat) {
    if ((rc = check_beat(h, what, n, k))) return rc;
  } else if (align) {
    if ((rc = check_align(h, what, n, k))) return rc;
  } else if (multipitch) {
    if ((rc = check_multipitch(h, what, n, k))) return rc;
  } else if (melody) {
    if ((rc = check_melody(h, what, n, k))) return rc;
  } else if (events) {
    if ((rc = sweep ? check_sweep(h, what, n, k) : check_events(h, what, n, k.params, k.out))) return rc;
    if (score && (rc = check_score(h, what, n, k))) return rc;
    if (flac && src.sample_rate < 1) return invalid("no sample rate");
  } else if (!k.params || (n > 0 && !k.out.status) || (flac && src.sample_rate < 1)) {
    return invalid(flac ? "null params / status or no sample rate" : "null params / status");
  }
  // the source's plan (every argument of every segment, its rows), the outputs against the rows
  ClipsJob job;
  job.score_params = k.score_params;
  job.want_scores = !k.with_frames || k.scores != nullptr, job.want_frames = k.with_frames;
  if (src.kind == kGivenMaps) {
    bool ordered = n >= 0 && src.row_offsets && src.row_offsets[0] == 0;
    for (int64_t i = 0; ordered && i < n; ++i) ordered = src.row_offsets[i + 1] >= src.row_offsets[i];
    if (!ordered || (src.mem_kind != BP_MEM_HOST && src.mem_kind != BP_MEM_DEVICE))
      return invalid("row_offsets must start at 0 and never decrease; mem_kind must be BP_MEM_HOST or BP_MEM_DEVICE");
    if (src.row_offsets[n] > 0 && (beat ? !src.onset : (!align && !src.contour) || (!multipitch && !melody && (!src.note || !src.onset))))
      return invalid("null input pointer");
    job.offs = src.row_offsets;
  } else {
    if (flac) {
      rc = plan_flac_clips(h, what, n, src.flac, src.sample_rate, &job.flac);
    } else if (src.kind == kAdpcmClips) {  // (the rate is the files' own)
      rc = plan_adpcm_clips(h, what, n, src.adpcm, &job.adpcm, &src.sample_rate, &job.flac.n_model, &job.flac.offs);
    } else {
      job.flac.n_model.resize((size_t)std::max<int64_t>(n, 0)), job.flac.offs.resize(job.flac.n_model.size() + 1);
      rc = check_clips(h, what, n, src.clips, src.sample_rate, src.mem_kind, true, job.flac.n_model.data(), job.flac.offs.data());
    }
    if (rc) return rc;
    job.offs = job.flac.offs.data();
  }
  const int64_t total = job.offs[n];
  if (multipitch) {  // the points or the counts of the contour rows: no note decoding, and a wait before the points are written
    bool queued = false;
    if ((rc = plan_multipitch(h, what, n, job.offs, k, job, &queued)) || !queued) return rc;
    BP_HIP(hipSetDevice(h->device));
    if (src.kind != kGivenMaps && src.sample_rate != h->rate)
      if ((rc = clips_filter(h, what, src.sample_rate))) return rc;
    if ((rc = finish(h, queue_job(h, src, k, job)))) return rc;
    return multipitch_home(h, what, n, job.offs, k, job);
  }
  if (melody) {  // the records or the counts of the contour rows: no note decoding, one launch
    bool queued = false;
    if ((rc = plan_melody(h, what, n, job.offs, k, job, &queued)) || !queued) return rc;
    BP_HIP(hipSetDevice(h->device));
    if (src.kind != kGivenMaps && src.sample_rate != h->rate)
      if ((rc = clips_filter(h, what, src.sample_rate))) return rc;
    if ((rc = finish(h, queue_job(h, src, k, job)))) return rc;
    melody_home(h, k, job);
    return BP_OK;
  }
  if (align) {  // the first frames of every segment's states: no note decoding, the emissions and one workgroup per segment
    bool queued = false;
    if ((rc = plan_align(h, what, n, job.offs, k, job, &queued)) || !queued) return rc;
    BP_HIP(hipSetDevice(h->device));
    if (src.kind != kGivenMaps && src.sample_rate != h->rate)
      if ((rc = clips_filter(h, what, src.sample_rate))) return rc;
    if ((rc = finish(h, queue_job(h, src, k, job)))) return rc;
    align_home(h, k, job);
    return BP_OK;
  }
  if (beat) {  // the summaries and the beats of the onset rows: no note decoding, three launches
    bool queued = false;
    if ((rc = plan_beat(h, what, n, job.offs, k, job, &queued)) || !queued) return rc;
    BP_HIP(hipSetDevice(h->device));
    if (src.kind != kGivenMaps && src.sample_rate != h->rate)
      if ((rc = clips_filter(h, what, src.sample_rate))) return rc;
    if ((rc = finish(h, queue_job(h, src, k, job)))) return rc;
    beat_home(h, n, k, job);
    return BP_OK;
  }
  if (!events && total > 0 && (!k.note_out || !k.cand_bits)) return invalid("null output pointer");
  // the statuses the host knows, and the jobs that need no device work
  if (!events)
    for (int64_t i = 0; i < n; ++i) k.out.status[i] = 0;
  bool done = total == 0;  // (no clip has a row)
  if (sweep) {
    bool queued = false;
    if ((rc = plan_sweep(h, what, n, job.offs, k, &job.sweep, &queued))) return rc;
    done = !queued;
  } else if (events) {
    done = events_without_device(n, job.offs, k.params, k.out);
  }
  if (flac && (done || !events)) flac_clips_status(h, job.flac, false, k.out.status);
  if (done) return BP_OK;
  BP_HIP(hipSetDevice(h->device));
  if (src.kind != kGivenMaps && src.sample_rate != h->rate)
    if ((rc = clips_filter(h, what, src.sample_rate))) return rc;
  if (sweep) {  // the tracker's job is over the decodes: its "row offsets" are the decodes' regions of the pools
    job.ev = EventsJob{what, k.count_name, k.n_decodes, job.sweep.pool_rows.data(), nullptr, job.sweep.seg.data(), nullptr, k.form};
  } else if (events) {
    job.dense_bends = !k.seg_params && k.params->include_pitch_bends != 0;
    for (int64_t i = 0; k.seg_params && i < n; ++i) {
      const bp_note_params& p = k.seg_params[i];
      job.dense_bends = job.dense_bends || p.include_pitch_bends != 0;
      job.seg.push_back(NoteTrackSeg{p.frame_threshold, p.energy_tol, p.min_note_len, p.melodia_trick != 0, p.include_pitch_bends != 0, 0, 0});
    }
    job.ev = EventsJob{what, k.count_name, n, job.offs, k.seg_params ? nullptr : k.params, k.seg_params ? job.seg.data() : nullptr,
                       nullptr, k.form};
  }
  rc = finish(h, queue_job(h, src, k, job));
  if (!events) {  // what the clips' records say (a clip without rows: 0)
    if (rc) return rc;
    if (job.exported_by_kernel) h->clip_stats_ready = n;  // only now: the export kernel, which re-initialises the records, has run
    for (int64_t i = 0; i < n; ++i)
      k.out.status[i] = job.offs[i + 1] > job.offs[i] && (h->clip_stats_host[4 * i + 1] || !(k.params->onset_threshold > 0.0)) ? 1 : 0;
  } else if (score) {  // the stream has drained: the scores and the statuses are in the page-locked block
    if (rc) return rc;
    if (job.want_scores) std::memcpy(k.scores, h->sc_home, (size_t)k.n_decodes * sizeof(bp_note_score));
    if (job.want_frames) std::memcpy(k.frames, h->fs_home, (size_t)k.n_decodes * sizeof(bp_frame_score));
    const int32_t* st = job.want_scores ? h->sc_home + 4 * k.n_decodes : reinterpret_cast<const int32_t*>(h->fs_home + 5 * k.n_decodes);
    for (int64_t j = 0; j < k.n_decodes; ++j) k.out.status[j] = st[j];
  } else if (rc || (rc = events_home(h, job.ev, k.out, nullptr))) {
    // (buffers too small: status and event_offsets are complete but for the decoder's verdicts)
    if (flac) flac_clips_status(h, job.flac, false, k.out.status);
    return rc;
  } else if (flac) {
    drop_failed_clips(h, job.flac, k.out);
  }
  if (flac) flac_clips_status(h, job.flac, true, k.out.status);
  return BP_OK;
}

}  // namespace

extern "C" {

int bp_clips_row_offsets(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int64_t* offsets) {
  if (!h) return BP_ERR_INVALID_ARG;
  return check_clips(h, "bp_clips_row_offsets", n_clips, clips, sample_rate, BP_MEM_HOST, false, nullptr, offsets);
}

int bp_infer_clips_candidates(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                              const bp_note_params* params, float* note_out, uint8_t* cand_bits, int8_t* bend_map, int* status) {
  return run_clips(h, "bp_infer_clips_candidates", JobSource{kPcmClips, n_clips, pcm_mem_kind, sample_rate, clips},
                   candidates_sink(params, note_out, cand_bits, bend_map, status));
}

int64_t bp_events_capacity(int64_t rows, int min_note_len) { return note_track_capacity(rows, min_note_len); }

int bp_infer_clips_events(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                          const bp_note_params* params, bp_note_event* events, int64_t max_events, int32_t* bends,
                          int64_t max_bends, int64_t* event_offsets, int* status) {
  return run_clips(h, "bp_infer_clips_events", JobSource{kPcmClips, n_clips, pcm_mem_kind, sample_rate, clips},
                   events_sink(params, events, max_events, bends, max_bends, event_offsets, status));
}

int bp_note_events_from_maps(bp_handle h, int64_t n_clips, const int64_t* row_offsets, const float* note, const float* onset,
                             const float* contour, int mem_kind, const bp_note_params* params, bp_note_event* events,
                             int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets, int* status) {
  return run_clips(h, "bp_note_events_from_maps", JobSource{kGivenMaps, n_clips, mem_kind, 0, nullptr, nullptr, row_offsets, note, onset, contour},
                   events_sink(params, events, max_events, bends, max_bends, event_offsets, status));
}

// ---- a sweep (include/basic_pitch_amd_sweep.h) -------------------------------------------------------------------------------------
int bp_note_events_sweep(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, const float* onset,
                         const float* contour, int mem_kind, int64_t n_sets, const bp_note_params* sets, int64_t n_decodes,
                         const bp_sweep_decode* decodes, bp_note_event* events, int64_t max_events, int32_t* bends, int64_t max_bends,
                         int64_t* event_offsets, int* status) {
  return run_clips(h, "bp_note_events_sweep", JobSource{kGivenMaps, n_segments, mem_kind, 0, nullptr, nullptr, row_offsets, note, onset, contour},
                   sweep_sink(n_sets, sets, n_decodes, decodes, events, max_events, bends, max_bends, event_offsets, status));
}

int bp_infer_clips_events_sweep(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind, int64_t n_sets,
                                const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes, bp_note_event* events,
                                int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets, int* status) {
  return run_clips(h, "bp_infer_clips_events_sweep", JobSource{kPcmClips, n_clips, pcm_mem_kind, sample_rate, clips},
                   sweep_sink(n_sets, sets, n_decodes, decodes, events, max_events, bends, max_bends, event_offsets, status));
}

// ---- a scored sweep (include/basic_pitch_amd_score.h) -----------------------------------------------------------------------------
int bp_note_events_sweep_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, const float* onset,
                               const float* contour, int mem_kind, int64_t n_sets, const bp_note_params* sets, int64_t n_decodes,
                               const bp_sweep_decode* decodes, const int64_t* ref_offsets, const bp_ref_note* refs,
                               const bp_score_params* score_params, bp_note_score* scores, int* status) {
  return run_clips(h, "bp_note_events_sweep_score", JobSource{kGivenMaps, n_segments, mem_kind, 0, nullptr, nullptr, row_offsets, note, onset, contour},
                   score_sink(n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, status));
}

int bp_infer_clips_events_sweep_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                      int64_t n_sets, const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                                      const int64_t* ref_offsets, const bp_ref_note* refs, const bp_score_params* score_params,
                                      bp_note_score* scores, int* status) {
  return run_clips(h, "bp_infer_clips_events_sweep_score", JobSource{kPcmClips, n_clips, pcm_mem_kind, sample_rate, clips},
                   score_sink(n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, status));
}

// ---- a sweep scored at the note and the frame level (include/basic_pitch_amd_frame_score.h) ----------------------------------------
int bp_note_events_sweep_frame_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note,
                                     const float* onset, const float* contour, int mem_kind, int64_t n_sets,
                                     const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                                     const int64_t* ref_offsets, const bp_ref_note* refs, const bp_score_params* score_params,
                                     bp_note_score* scores, bp_frame_score* frames, int* status) {
  return run_clips(h, "bp_note_events_sweep_frame_score", JobSource{kGivenMaps, n_segments, mem_kind, 0, nullptr, nullptr, row_offsets, note, onset, contour},
                   frame_score_sink(n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, frames, status));
}

int bp_infer_clips_events_sweep_frame_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                            int64_t n_sets, const bp_note_params* sets, int64_t n_decodes,
                                            const bp_sweep_decode* decodes, const int64_t* ref_offsets, const bp_ref_note* refs,
                                            const bp_score_params* score_params, bp_note_score* scores, bp_frame_score* frames,
                                            int* status) {
  return run_clips(h, "bp_infer_clips_events_sweep_frame_score", JobSource{kPcmClips, n_clips, pcm_mem_kind, sample_rate, clips},
                   frame_score_sink(n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, frames, status));
}

// ---- multi-pitch estimates (include/basic_pitch_amd_multipitch.h) -------------------------------------------------------------------
int bp_multipitch_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour, int mem_kind,
                            const bp_mp_params* p, bp_f0_point* points, int64_t max_points, int64_t* point_offsets, int* status) {
  return run_clips(h, "bp_multipitch_from_maps", JobSource{kGivenMaps, n_segments, mem_kind, 0, nullptr, nullptr, row_offsets, nullptr, nullptr, contour},
                   multipitch_sink(p, points, max_points, point_offsets, status));
}

int bp_infer_clips_multipitch(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                              const bp_mp_params* p, bp_f0_point* points, int64_t max_points, int64_t* point_offsets, int* status) {
  return run_clips(h, "bp_infer_clips_multipitch", JobSource{kPcmClips, n_clips, pcm_mem_kind, sample_rate, clips},
                   multipitch_sink(p, points, max_points, point_offsets, status));
}

int bp_multipitch_sweep_frame_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour, int mem_kind,
                                    int64_t n_sets, const bp_mp_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                                    const int64_t* ref_offsets, const bp_ref_note* refs, const bp_score_params* score_params,
                                    bp_frame_score* frames, int* status) {
  return run_clips(h, "bp_multipitch_sweep_frame_score",
                   JobSource{kGivenMaps, n_segments, mem_kind, 0, nullptr, nullptr, row_offsets, nullptr, nullptr, contour},
                   multipitch_score_sink(n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, frames, status));
}

int bp_infer_clips_multipitch_sweep_frame_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                                int64_t n_sets, const bp_mp_params* sets, int64_t n_decodes,
                                                const bp_sweep_decode* decodes, const int64_t* ref_offsets, const bp_ref_note* refs,
                                                const bp_score_params* score_params, bp_frame_score* frames, int* status) {
  return run_clips(h, "bp_infer_clips_multipitch_sweep_frame_score", JobSource{kPcmClips, n_clips, pcm_mem_kind, sample_rate, clips},
                   multipitch_score_sink(n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, frames, status));
}

// ---- the melody (include/basic_pitch_amd_melody.h) -------------------------------------------------------------------------------
int bp_melody_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour, int mem_kind,
                        const bp_melody_params* p, bp_melody_point* points, int64_t max_points, int* status) {
  return run_clips(h, "bp_melody_from_maps", JobSource{kGivenMaps, n_segments, mem_kind, 0, nullptr, nullptr, row_offsets, nullptr, nullptr, contour},
                   melody_sink(p, points, max_points, status));
}

int bp_infer_clips_melody(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                          const bp_melody_params* p, bp_melody_point* points, int64_t max_points, int* status) {
  return run_clips(h, "bp_infer_clips_melody", JobSource{kPcmClips, n_clips, pcm_mem_kind, sample_rate, clips},
                   melody_sink(p, points, max_points, status));
}

int bp_melody_sweep_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour, int mem_kind,
                          int64_t n_sets, const bp_melody_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                          const double* ref_pitch, const bp_score_params* score_params, bp_melody_score* scores, int* status) {
  return run_clips(h, "bp_melody_sweep_score", JobSource{kGivenMaps, n_segments, mem_kind, 0, nullptr, nullptr, row_offsets, nullptr, nullptr, contour},
                   melody_score_sink(n_sets, sets, n_decodes, decodes, ref_pitch, score_params, scores, status));
}

int bp_infer_clips_melody_sweep_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                      int64_t n_sets, const bp_melody_params* sets, int64_t n_decodes,
                                      const bp_sweep_decode* decodes, const double* ref_pitch,
                                      const bp_score_params* score_params, bp_melody_score* scores, int* status) {
  return run_clips(h, "bp_infer_clips_melody_sweep_score", JobSource{kPcmClips, n_clips, pcm_mem_kind, sample_rate, clips},
                   melody_score_sink(n_sets, sets, n_decodes, decodes, ref_pitch, score_params, scores, status));
}

// ---- tempo and beats (include/basic_pitch_amd_beat.h) ----------------------------------------------------------------------------
int bp_beats_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* onset, int mem_kind,
                       const bp_beat_params* p, bp_beat_summary* summaries, int32_t* beats, int64_t max_beats, int64_t* beat_offsets) {
  return run_clips(h, "bp_beats_from_maps", JobSource{kGivenMaps, n_segments, mem_kind, 0, nullptr, nullptr, row_offsets, nullptr, onset, nullptr},
                   beat_sink(p, summaries, beats, max_beats, beat_offsets));
}

int bp_infer_clips_beats(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind, const bp_beat_params* p,
                         bp_beat_summary* summaries, int32_t* beats, int64_t max_beats, int64_t* beat_offsets) {
  return run_clips(h, "bp_infer_clips_beats", JobSource{kPcmClips, n_clips, pcm_mem_kind, sample_rate, clips},
                   beat_sink(p, summaries, beats, max_beats, beat_offsets));
}

// the clock readings of the path kernel for segment c of the handle's last beat call with rows (100 MHz ticks: start, period
// picked, recurrence done, backtrace done): tools/bench_beat.py
int bp_internal_beat_clocks(bp_handle h, int64_t c, int64_t* clocks) {
  if (!h || !clocks || c < 0 || (size_t)(c + 1) * kBeatAccStride > h->bt_acc.capacity()) return BP_ERR_INVALID_ARG;
  BP_HIP(hipSetDevice(h->device));
  BP_HIP(hipMemcpy(clocks, h->bt_acc + c * kBeatAccStride + kBeatAccClocks, 4 * sizeof(int64_t), hipMemcpyDeviceToHost));
  return BP_OK;
}

// ---- forced alignment (include/basic_pitch_amd_align.h) --------------------------------------------------------------------------
int bp_align_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, const float* onset,
                       int mem_kind, const int64_t* state_offsets, const bp_align_state* states, const bp_align_params* p,
                       int32_t* first_frame, int64_t max_states, int64_t* total, int* status) {
  return run_clips(h, "bp_align_from_maps", JobSource{kGivenMaps, n_segments, mem_kind, 0, nullptr, nullptr, row_offsets, note, onset, nullptr},
                   align_sink(state_offsets, states, p, first_frame, max_states, total, status));
}

int bp_infer_clips_align(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                         const int64_t* state_offsets, const bp_align_state* states, const bp_align_params* p, int32_t* first_frame,
                         int64_t max_states, int64_t* total, int* status) {
  return run_clips(h, "bp_infer_clips_align", JobSource{kPcmClips, n_clips, pcm_mem_kind, sample_rate, clips},
                   align_sink(state_offsets, states, p, first_frame, max_states, total, status));
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
  return run_clips(h, "bp_ab_clips_candidates_from_maps",
                   JobSource{kGivenMaps, n_clips, BP_MEM_HOST, 0, nullptr, nullptr, offsets, note, onset, contour},
                   candidates_sink(params, note_out, cand_bits, bend_map, status));
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
  JobSink k = events_sink(params, events, max_events, bends, max_bends, event_offsets, status);
  k.seg_params = params, k.form = form, k.count_name = "n";
  for (int64_t i = 0; i < n; ++i) {
    if (row_offsets[i + 1] < row_offsets[i]) return BP_ERR_INVALID_ARG;
    if (int rc = check_events(h, what, n, params + i, k.out)) return rc;
  }
  return run_clips(h, what, JobSource{kGivenMaps, n, BP_MEM_HOST, 0, nullptr, nullptr, row_offsets, note, onset, contour}, k);
}
#endif

// ---- a job of FLAC clips (include/basic_pitch_amd_flac_clips.h) ------------------------------------------------------------------
int bp_flac_clips_row_offsets(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int sample_rate, int64_t* offsets, int* status) {
  if (!h) return BP_ERR_INVALID_ARG;
  const char* what = "bp_flac_clips_row_offsets";
  if (!offsets || (n_clips > 0 && !status) || sample_rate < 1) return invalid(h, what, "null offsets / status or no sample rate");
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
  if (!pcm_offsets || (n_clips > 0 && !status)) return invalid(h, what, "null pcm_offsets / status");
  FlacJob job;
  if (int rc = plan_flac_clips(h, what, n_clips, clips, 0, &job)) return rc;
  for (int64_t i = 0; i < n_clips; ++i)
    if (job.dev[(size_t)i] >= 0 && (!pcm || pcm_offsets[i] < 0 ||
                                    pcm_offsets[i + 1] - pcm_offsets[i] < job.lay[(size_t)i].n_frames * job.lay[(size_t)i].channels))
      return invalid(h, what, "clip " + std::to_string(i) + ": null pcm or too little room between its offsets");
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
    flac_pcm_to_int32(home.data() + k.pcm_off, k.out_wide != 0, k.out_shift, k.st.total * k.st.channels, pcm + pcm_offsets[i]);
  }
  flac_clips_status(h, job, true, status);
  return BP_OK;
}

int bp_infer_flac_clips_candidates(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int sample_rate,
                                   const bp_note_params* params, float* note_out, uint8_t* cand_bits, int8_t* bend_map, int* status) {
  return run_clips(h, "bp_infer_flac_clips_candidates", JobSource{kFlacClips, n_clips, BP_MEM_HOST, sample_rate, nullptr, clips},
                   candidates_sink(params, note_out, cand_bits, bend_map, status));
}

int bp_infer_flac_clips_events(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int sample_rate, const bp_note_params* params,
                               bp_note_event* events, int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets,
                               int* status) {
  return run_clips(h, "bp_infer_flac_clips_events", JobSource{kFlacClips, n_clips, BP_MEM_HOST, sample_rate, nullptr, clips},
                   events_sink(params, events, max_events, bends, max_bends, event_offsets, status));
}

// ---- a job of IMA ADPCM clips (include/basic_pitch_amd_adpcm.h) -------------------------------------------------------------------
int bp_infer_adpcm_clips_events(bp_handle h, int64_t n_clips, const bp_adpcm_clip* clips, const bp_note_params* params,
                                bp_note_event* events, int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets,
                                int* status) {
  JobSource src{kAdpcmClips, n_clips, BP_MEM_HOST, 0};
  src.adpcm = clips;
  return run_clips(h, "bp_infer_adpcm_clips_events", src, events_sink(params, events, max_events, bends, max_bends, event_offsets, status));
}

}  // extern "C"
