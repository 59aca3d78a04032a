// The driver of the jobs of many clips or segments and its sources (include/basic_pitch_amd_clips.h, _events.h, _flac_clips.h,
// _adpcm.h): many short clips through the model in one call — raw PCM, FLAC or IMA ADPCM files' bytes decoded on the device, or
// maps the caller already holds — and home either the note candidates of every clip or, the tracker run on the device too, the
// note events alone.  What else a job can end in has a file of its own: clips_sweep.hip (every segment under many parameter
// sets, its events home or scored), clips_multipitch.hip, clips_melody.hip, clips_align.hip, clips_beat.hip.
//
// Every entry point is a source and a sink on one driver (run_clips), the job family's run_track (track_api.hip); the sink
// protocol, the order of a call and the lifetime rule are in clips_job.h, with the helpers the sinks share (defined here).
// Nothing is queued before every argument has been checked, and a call that fails after queuing work returns only once the
// handle's stream has drained (finish).  The tracker's host half (events_reserve / events_queue / events_home) lives here too:
// bp_streams_events (stream_api.hip) puts it behind its own dense half.
#include <algorithm>
#include <cstring>

#include "../../include/basic_pitch_amd_adpcm.h"
#include "clips_job.h"

using namespace bp;

extern "C" void bp_internal_freq_limits(const bp_note_params* prm, int* lo, int* hi);
extern "C" double bp_internal_frame_time(int64_t frame);
extern "C" const char* bp_internal_score_bad_params(const bp_score_params* p);
extern "C" int64_t bp_internal_score_bad_ref(const bp_ref_note* refs, int64_t n);
extern "C" void bp_internal_frame_interval(double start_s, double end_s, int64_t n_frames, int64_t* f0, int64_t* f1);
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

// ---- what the sinks share (declared in clips_job.h) --------------------------------------------------------------------------
int invalid(bp_handle h, const char* what, const std::string& why) {
  h->err = std::string(what) + ": " + why;
  return BP_ERR_INVALID_ARG;
}

int64_t ascending_from_zero(const int64_t* offsets, int64_t n) {
  if (!offsets || offsets[0] != 0) return 0;
  for (int64_t i = 1; i <= n; ++i)
    if (offsets[i] < offsets[i - 1]) return i;
  return -1;
}

const char* bad_params(const bp_note_params& prm) {
  if (prm.melodia_trick && prm.frame_threshold < 0.0)
    return "a negative frame threshold with the melodia trick never terminates (note_creation.py:452)";
  return prm.min_note_len < 0 ? "negative min_note_len" : nullptr;
}
const char* bad_room(const EventsSink& out) {
  const bool fine = check_room(out.max_events, out.events) && check_room(out.max_bends, out.bends);
  return fine ? nullptr : "negative max_events / max_bends, or room without a buffer";
}

// the decode table of a sweep against its segments and sets; decodes null: the cross product
static int check_decode_table(bp_handle h, const char* what, int64_t n_segs, int64_t n_sets, int64_t n_decodes, const bp_sweep_decode* decodes) {
  auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
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

int check_sets_and_decodes(bp_handle h, const char* what, int64_t n_segs, int64_t n_sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                           bool nulls, const char* counts, const char* also, const std::function<const char*(int64_t)>& bad_set) {
  if (n_segs < 0 || n_sets < 0 || n_decodes < 0 || nulls) return invalid(h, what, counts);
  if (also) return invalid(h, what, also);
  if (n_decodes > BP_SWEEP_MAX_DECODES)
    return invalid(h, what, std::to_string(n_decodes) + " decodes, more than BP_SWEEP_MAX_DECODES (" + std::to_string(BP_SWEEP_MAX_DECODES) +
                                "): split the job");
  for (int64_t p = 0; p < n_sets; ++p)
    if (const char* why = bad_set(p)) return invalid(h, what, "set " + std::to_string(p) + ": " + why);
  return check_decode_table(h, what, n_segs, n_sets, n_decodes, decodes);
}

int check_rows_in_all(bp_handle h, const char* what, int64_t rows, const char* lead) {
  if (rows <= BP_SWEEP_MAX_ROWS) return BP_OK;
  return invalid(h, what, lead + std::to_string(rows) + " rows in all, more than BP_SWEEP_MAX_ROWS (" + std::to_string(BP_SWEEP_MAX_ROWS) +
                              "): split the job");
}

int check_score(bp_handle h, const char* what, int64_t n_segs, int64_t n_decodes, const int64_t* ref_offsets, const bp_ref_note* refs,
                const bp_score_params* score_params, const void* out, const char* out_name) {
  auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
  if (!ref_offsets || (n_decodes > 0 && !out)) return invalid(std::string("null ref_offsets or ") + out_name);
  if (const char* why = bp_internal_score_bad_params(score_params)) return invalid(why);
  const int64_t at = ascending_from_zero(ref_offsets, n_segs);
  if (at == 0) return invalid("ref_offsets must start at 0");
  if (at > 0)
    return invalid("segment " + std::to_string(at - 1) + ": ref_offsets decrease (" + std::to_string(ref_offsets[at - 1]) + " to " +
                   std::to_string(ref_offsets[at]) + ")");
  if (ref_offsets[n_segs] > 0 && !refs) return invalid("null refs");
  const int64_t bad = bp_internal_score_bad_ref(refs, ref_offsets[n_segs]);
  if (bad >= 0) return invalid("ref " + std::to_string(bad) + ": a field is not finite, or end_s < start_s");
  return BP_OK;
}

void refs_in_pitch_order(int64_t n_segs, const int64_t* offs, const int64_t* ref_offsets, const bp_ref_note* refs,
                         const std::function<void(size_t, const bp_ref_note&, int32_t, int32_t)>& put) {
  std::vector<int64_t> order;
  for (int64_t i = 0; i < n_segs; ++i) {
    const int64_t first = ref_offsets[i], rows = offs[i + 1] - offs[i];
    order.resize((size_t)(ref_offsets[i + 1] - first));
    for (size_t r = 0; r < order.size(); ++r) order[r] = first + (int64_t)r;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return refs[a].pitch_midi < refs[b].pitch_midi; });
    for (size_t r = 0; r < order.size(); ++r) {
      const bp_ref_note& ref = refs[order[r]];
      int64_t f0 = 0, f1 = 0;
      bp_internal_frame_interval(ref.start_s, ref.end_s, rows, &f0, &f1);
      put((size_t)first + r, ref, (int32_t)f0, (int32_t)f1);  // (rows <= BP_SWEEP_MAX_ROWS)
    }
  }
}

}  // namespace bp

namespace {

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
int check_events(bp_handle h, const char* what, int64_t n_clips, const bp_note_params* prm, const EventsSink& out) {
  auto invalid = [&](const char* why) { return bp::invalid(h, what, why); };
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

// ---- the candidates sink: the note candidates of all rows (host buffers) and a status per clip; the maps stay in track_out -----
struct CandidatesSink final : JobSink {
  const bp_note_params* params;
  float* note_out;
  uint8_t* cand_bits;
  int8_t* bend_map;
  int* status;
  bool exported_by_kernel = false;
  CandidatesSink(const bp_note_params* p, float* note, uint8_t* bits, int8_t* bend, int* st)
      : params(p), note_out(note), cand_bits(bits), bend_map(bend), status(st) {}

  MapsUse use(bp_handle) const override { return MapsUse{true, true, true, false, true}; }
  int check(bp_handle h, const char* what, int64_t n) override {
    return !params || (n > 0 && !status) ? invalid(h, what, "null params / status") : BP_OK;
  }
  int plan(bp_handle h, const char* what, int64_t n, const int64_t* offs, bool* queued) override {
    if (offs[n] > 0 && (!note_out || !cand_bits)) return invalid(h, what, "null output pointer");
    for (int64_t i = 0; i < n; ++i) status[i] = 0;
    *queued = offs[n] > 0;  // (else no clip has a row)
    return BP_OK;
  }
  int queue(bp_handle h, const Maps& all, int64_t n, const int64_t* offs) override {
    return queue_clips_candidates(h, all, n, offs, params, note_out, cand_bits, bend_map, &exported_by_kernel);
  }
  // what the clips' records say (a clip without rows: 0)
  int home(bp_handle h, const char*, int64_t n, const int64_t* offs) override {
    if (exported_by_kernel) h->clip_stats_ready = n;  // only now: the export kernel, which re-initialises the records, has run
    for (int64_t i = 0; i < n; ++i)
      status[i] = offs[i + 1] > offs[i] && (h->clip_stats_host[4 * i + 1] || !(params->onset_threshold > 0.0)) ? 1 : 0;
    return BP_OK;
  }
  EventsSink clip_results() const override { return EventsSink{nullptr, 0, nullptr, 0, nullptr, status}; }
};

// ---- the events sink: the tracker on the device too, the note events alone go home (out).  params: of the dense half, and of
// the tracker unless seg_params gives every segment its own (with the tracker's form and the call's name for n: the A/B hook).
struct NoteEventsSink final : JobSink {
  const bp_note_params* params;
  EventsSink out;
  const bp_note_params* seg_params = nullptr;
  int form = kNoteTrackFormAuto;
  const char* count_name = "n_clips";
  std::vector<NoteTrackSeg> seg;
  bool dense_bends = false;  // the dense half makes the bend map
  EventsJob ev{};
  EventsPlan ev_plan;
  NoteEventsSink(const bp_note_params* p, const EventsSink& o) : params(p), out(o) {}

  MapsUse use(bp_handle) const override { return MapsUse{true, true, true, false, true}; }
  int check(bp_handle h, const char* what, int64_t n) override { return check_events(h, what, n, params, out); }
  int plan(bp_handle, const char* what, int64_t n, const int64_t* offs, bool* queued) override {
    *queued = !events_without_device(n, offs, params, out);
    if (!*queued) return BP_OK;
    dense_bends = !seg_params && params->include_pitch_bends != 0;
    for (int64_t i = 0; seg_params && i < n; ++i) {
      const bp_note_params& p = seg_params[i];
      dense_bends = dense_bends || p.include_pitch_bends != 0;
      seg.push_back(NoteTrackSeg{p.frame_threshold, p.energy_tol, p.min_note_len, p.melodia_trick != 0, p.include_pitch_bends != 0, 0, 0});
    }
    ev = EventsJob{what, count_name, n, offs, seg_params ? nullptr : params, seg_params ? seg.data() : nullptr, nullptr, form};
    return BP_OK;
  }
  // the dense half of note decoding for every segment as its own track, the tracker behind it
  int queue(bp_handle h, const Maps& all, int64_t n, const int64_t* offs) override {
    uint8_t* d_bits = nullptr;
    int8_t* d_bend = nullptr;
    int rc = BP_OK;
    if ((rc = events_reserve(h, ev, &ev_plan)) || (rc = queue_clips_dense(h, all, n, offs, params, dense_bends, &d_bits, &d_bend))) return rc;
    return events_queue(h, ev, ev_plan, TrackInputs{all.note, d_bits, d_bend, h->clip_rows, h->clip_stats});
  }
  int home(bp_handle h, const char*, int64_t, const int64_t*) override { return events_home(h, ev, out, nullptr); }
  EventsSink clip_results() const override { return out; }
};

// ---- the driver ------------------------------------------------------------------------------------------------------------
// What the source knows of a job, and every host buffer its asynchronous copies read: the driver holds it until the wait is over.
struct ClipsJob {
  FlacJob flac;                   // n_model and offs of the clips (kPcmClips too); the rest: kFlacClips
  const int64_t* offs = nullptr;  // rows before each segment (kGivenMaps: the caller's)
  std::vector<bp_clip> decoded;   // kFlacClips, kAdpcmClips: the clips' PCM on the device
  AdpcmJob adpcm;                 // kAdpcmClips
  std::vector<ClipDesc> tab;
};

// One plane of given maps (cells floats) where a sink may read it: where it lies, unless it is in host memory or, with
// aligned16, off a 16-byte boundary — then its copy in `copy`, the sink's own buffer.
int given_plane(bp_handle h, const float* given, size_t cells, int mem_kind, bool aligned16, DeviceBuffer<float>& copy, float** at) {
  *at = const_cast<float*>(given);
  if (mem_kind == BP_MEM_DEVICE && (!aligned16 || reinterpret_cast<uintptr_t>(given) % 16 == 0)) return BP_OK;
  BP_HIP(copy.reserve(cells));
  BP_HIP(hipMemcpyAsync(copy, given, cells * sizeof(float), mem_kind == BP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->stream));
  *at = copy;
  return BP_OK;
}

// everything a job queues: the source (the maps of all segments, concatenated by job.offs: made into track_out, or given and
// taken as the sink uses them), then the sink
int queue_job(bp_handle h, const JobSource& s, JobSink& sink, ClipsJob& job) {
  Maps all{};
  int rc = BP_OK;
  const MapsUse use = sink.use(h);
  const int64_t T = job.offs[s.n];
  if (s.kind == kGivenMaps && use.private_copy) {
    rc = take_given_maps(h, s.note, s.onset, s.contour, T, s.mem_kind, &all);
  } else if (s.kind == kGivenMaps) {
    if (use.note) rc = given_plane(h, s.note, (size_t)T * kFreqN, s.mem_kind, use.aligned16, *use.note_copy, &all.note);
    if (!rc && use.onset) rc = given_plane(h, s.onset, (size_t)T * kFreqN, s.mem_kind, use.aligned16, *use.onset_copy, &all.onset);
    if (!rc && use.contour) rc = given_plane(h, s.contour, (size_t)T * kFreqC, s.mem_kind, use.aligned16, *use.contour_copy, &all.contour);
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
  return rc ? rc : sink.queue(h, all, s.n, job.offs);
}

}  // namespace

namespace bp {

int run_clips(bp_handle h, const char* what, JobSource src, JobSink& sink) {
  if (!h) return BP_ERR_INVALID_ARG;
  const int64_t n = src.n;
  const bool flac = src.kind == kFlacClips, given = src.kind == kGivenMaps;
  int rc = BP_OK;
  // the sink's fixed arguments
  if ((rc = sink.check(h, what, n))) return rc;
  if (flac && src.sample_rate < 1) return invalid(h, what, "no sample rate");
  // the source's plan (every argument of every segment, its rows), the outputs against the rows
  ClipsJob job;
  if (given) {
    if (n < 0 || ascending_from_zero(src.row_offsets, n) >= 0 || (src.mem_kind != BP_MEM_HOST && src.mem_kind != BP_MEM_DEVICE))
      return invalid(h, what, "row_offsets must start at 0 and never decrease; mem_kind must be BP_MEM_HOST or BP_MEM_DEVICE");
    const MapsUse use = sink.use(h);
    if (src.row_offsets[n] > 0 && ((use.note && !src.note) || (use.onset && !src.onset) || (use.contour && !src.contour)))
      return invalid(h, what, "null input pointer");
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
  bool queued = false;
  if ((rc = sink.plan(h, what, n, job.offs, &queued))) return rc;
  // the statuses the host knows of FLAC clips, and the jobs that need no device work
  const EventsSink out = flac ? sink.clip_results() : EventsSink{};
  if (flac && (!queued || !out.event_offsets)) flac_clips_status(h, job.flac, false, out.status);
  if (!queued) return BP_OK;
  BP_HIP(hipSetDevice(h->device));
  if (!given && src.sample_rate != h->rate)
    if ((rc = clips_filter(h, what, src.sample_rate))) return rc;
  if ((rc = finish(h, queue_job(h, src, sink, job))) == BP_OK) rc = sink.home(h, what, n, job.offs);
  if (!flac) return rc;
  if (rc) {  // (buffers too small: status and event_offsets are complete but for the decoder's verdicts)
    if (out.event_offsets) flac_clips_status(h, job.flac, false, out.status);
    return rc;
  }
  if (out.event_offsets) drop_failed_clips(h, job.flac, out);
  flac_clips_status(h, job.flac, true, out.status);
  return BP_OK;
}

}  // namespace bp

extern "C" {

int bp_clips_row_offsets(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int64_t* offsets) {
  if (!h) return BP_ERR_INVALID_ARG;
  return check_clips(h, "bp_clips_row_offsets", n_clips, clips, sample_rate, BP_MEM_HOST, false, nullptr, offsets);
}

int bp_infer_clips_candidates(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                              const bp_note_params* params, float* note_out, uint8_t* cand_bits, int8_t* bend_map, int* status) {
  CandidatesSink sink(params, note_out, cand_bits, bend_map, status);
  return run_clips(h, "bp_infer_clips_candidates", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

int64_t bp_events_capacity(int64_t rows, int min_note_len) { return note_track_capacity(rows, min_note_len); }

int bp_infer_clips_events(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                          const bp_note_params* params, bp_note_event* events, int64_t max_events, int32_t* bends,
                          int64_t max_bends, int64_t* event_offsets, int* status) {
  NoteEventsSink sink(params, EventsSink{events, max_events, bends, max_bends, event_offsets, status});
  return run_clips(h, "bp_infer_clips_events", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

int bp_note_events_from_maps(bp_handle h, int64_t n_clips, const int64_t* row_offsets, const float* note, const float* onset,
                             const float* contour, int mem_kind, const bp_note_params* params, bp_note_event* events,
                             int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets, int* status) {
  NoteEventsSink sink(params, EventsSink{events, max_events, bends, max_bends, event_offsets, status});
  return run_clips(h, "bp_note_events_from_maps", given_maps(n_clips, row_offsets, note, onset, contour, mem_kind), sink);
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
  CandidatesSink sink(params, note_out, cand_bits, bend_map, status);
  return run_clips(h, "bp_ab_clips_candidates_from_maps", given_maps(n_clips, offsets, note, onset, contour, BP_MEM_HOST), sink);
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
  NoteEventsSink k(params, EventsSink{events, max_events, bends, max_bends, event_offsets, status});
  k.seg_params = params, k.form = form, k.count_name = "n";
  for (int64_t i = 0; i < n; ++i) {
    if (row_offsets[i + 1] < row_offsets[i]) return BP_ERR_INVALID_ARG;
    if (int rc = check_events(h, what, n, params + i, k.out)) return rc;
  }
  return run_clips(h, what, given_maps(n, row_offsets, note, onset, contour, BP_MEM_HOST), k);
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
  CandidatesSink sink(params, note_out, cand_bits, bend_map, status);
  return run_clips(h, "bp_infer_flac_clips_candidates", JobSource{kFlacClips, n_clips, BP_MEM_HOST, sample_rate, nullptr, clips}, sink);
}

int bp_infer_flac_clips_events(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int sample_rate, const bp_note_params* params,
                               bp_note_event* events, int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets,
                               int* status) {
  NoteEventsSink sink(params, EventsSink{events, max_events, bends, max_bends, event_offsets, status});
  return run_clips(h, "bp_infer_flac_clips_events", JobSource{kFlacClips, n_clips, BP_MEM_HOST, sample_rate, nullptr, clips}, sink);
}

// ---- a job of IMA ADPCM clips (include/basic_pitch_amd_adpcm.h) -------------------------------------------------------------------
int bp_infer_adpcm_clips_events(bp_handle h, int64_t n_clips, const bp_adpcm_clip* clips, const bp_note_params* params,
                                bp_note_event* events, int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets,
                                int* status) {
  JobSource src{kAdpcmClips, n_clips, BP_MEM_HOST, 0};
  src.adpcm = clips;
  NoteEventsSink sink(params, EventsSink{events, max_events, bends, max_bends, event_offsets, status});
  return run_clips(h, "bp_infer_adpcm_clips_events", src, sink);
}

}  // extern "C"
