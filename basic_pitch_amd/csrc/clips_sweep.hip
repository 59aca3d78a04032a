// A sweep: the segments of a job under many parameter sets (include/basic_pitch_amd_sweep.h), its events home or
// scored on the device against reference notes at the note level (include/basic_pitch_amd_score.h) and the frame level
// (include/basic_pitch_amd_frame_score.h): the sink behind run_clips (clips_job.h) and its entry points.  Host code only.
#include <algorithm>
#include <cstring>
#include <map>
#include <tuple>

#include "../../include/basic_pitch_amd_frame_score.h"
#include "clips_job.h"

using namespace bp;

extern "C" void bp_internal_freq_limits(const bp_note_params* prm, int* lo, int* hi);
extern "C" double bp_internal_score_offset_tol(const bp_ref_note* r, const bp_score_params* p);
extern "C" void bp_internal_frame_pitch_range(const bp_ref_note* r, const bp_score_params* p, int32_t* lo, int32_t* hi);

namespace {

// A dense key: what the dense half of note decoding depends on.  Sets of one key share its bitmap and its block of stats
// records; keys of one band [lo, hi) share the constrained copy of the note rows.
struct SweepKey {
  int lo, hi, infer;
  double onset_thresh;
  int band;  // its band's slot of h->sw_note; -1: all 88 bins, the maps themselves
};

// The events (out) of n_decodes decodes, decode j segment decodes[j].segment under sets[decodes[j].params] (decodes null: the
// cross product, set-major); every set has its own dense half.  score: the same sweep, but what goes home is `scores` and
// out.status alone — every decode's events scored on the device against the refs of its segment.  with_frames: `frames` goes
// home too, and `scores` may be null.
struct SweepSink final : JobSink {
  struct Args {
    bool score, with_frames;
    int64_t n_sets;
    const bp_note_params* sets;
    int64_t n_decodes;
    const bp_sweep_decode* decodes;
    EventsSink out;
    const int64_t* ref_offsets;  // score: [n segments + 1], the refs of each segment
    const bp_ref_note* refs;
    const bp_score_params* score_params;
    bp_note_score* scores;
    bp_frame_score* frames;
  } a;
  // What the host knows of a sweep before anything is queued, and what its asynchronous copies read.
  std::vector<int64_t> segment;     // per decode: its segment, its set (the cross product spelled out)
  std::vector<int32_t> params;
  std::vector<NoteTrackSeg> seg;    // per decode: the tracker's parameters
  std::vector<int64_t> pool_rows;   // [n_decodes + 1] rows of the decodes before each: its regions of the pools
  std::vector<int> set_key;         // set -> its key; -1: no decode with rows names it, or its onset threshold is <= 0
  std::vector<SweepKey> keys;       // ordered by band
  int64_t n_bands = 0;              // constrained copies of the note rows
  bool bends = false;               // a decode that reaches the tracker wants bends
  std::vector<uint8_t> block;       // the decode table (NoteSweepDecode) with pool_rows and the event regions behind it
  // score: the refs as the device reads them, per decode which are its segment's, the room the launch's LDS needs
  std::vector<NoteScoreRef> score_refs;
  std::vector<NoteScoreDecode> ref_of;
  int max_refs = 0, max_depth = 0;
  std::vector<NoteFrameRef> frame_refs;  // with_frames: per segment its refs in ascending pitch, as note_frames.hip reads them
  const bool want_scores;                // the note-matching launch (the frame launch: with_frames)
  EventsJob ev{};  // the tracker's job is over the decodes: its "row offsets" are the decodes' regions of the pools
  EventsPlan ev_plan;
  explicit SweepSink(const Args& args) : a(args), want_scores(!args.with_frames || args.scores != nullptr) {}

  MapsUse use(bp_handle) const override { return MapsUse{true, true, true, false, true}; }

  int check(bp_handle h, const char* what, int64_t n_segs) override {
    // (a scored sweep sends no events home: no offsets, no room)
    if (int rc = check_sets_and_decodes(h, what, n_segs, a.n_sets, a.n_decodes, a.decodes,
                                        (a.n_sets > 0 && !a.sets) || (!a.score && !a.out.event_offsets) || (a.n_decodes > 0 && !a.out.status),
                                        "negative n_segments / n_clips, n_sets or n_decodes, null sets, event_offsets or status",
                                        a.score ? nullptr : bad_room(a.out), [&](int64_t p) { return bad_params(a.sets[p]); }))
      return rc;
    if (!a.score) return BP_OK;
    return check_score(h, what, n_segs, a.n_decodes, a.ref_offsets, a.refs, a.score_params, a.with_frames ? (const void*)a.frames : a.scores,
                       a.with_frames ? "frames" : "scores");
  }

  // decode j of a scored sweep without events: {n_ref, 0, 0, 0} and {rows, 0, 0, 0, 0}
  void score_nothing(int64_t j, int64_t rows) {
    const int64_t n_ref = a.ref_offsets[segment[(size_t)j] + 1] - a.ref_offsets[segment[(size_t)j]];
    if (a.scores) a.scores[j] = bp_note_score{(int32_t)std::min<int64_t>(n_ref, INT32_MAX), 0, 0, 0};
    if (a.frames) a.frames[j] = bp_frame_score{rows, 0, 0, 0, 0};
  }

  // The decodes against the rows: every decode's tracker parameters and regions, the dense keys of the sets that reach the
  // tracker.  *queued false: no decode needs the device — no rows, or an onset threshold <= 0 (status 1, as the events sink
  // says it).
  int plan(bp_handle h, const char* what, int64_t n_segs, const int64_t* offs, bool* queued) override {
    const int64_t n = a.n_decodes;
    segment.resize((size_t)n), params.resize((size_t)n), seg.resize((size_t)n);
    pool_rows.assign((size_t)n + 1, 0);
    set_key.assign((size_t)a.n_sets, -1);
    std::map<std::tuple<int, int, int, double>, int> found;  // (a threshold > 0 is no NaN: the order is total)
    *queued = false;
    for (int64_t j = 0; j < n; ++j) {
      const DecodePair d = decode_pair(a.decodes, j, n_segs);
      const bp_note_params& prm = a.sets[d.set];
      const int64_t rows = offs[d.segment + 1] - offs[d.segment];
      const bool skip = !(prm.onset_threshold > 0.0);
      segment[(size_t)j] = d.segment, params[(size_t)j] = d.set;
      seg[(size_t)j] = NoteTrackSeg{prm.frame_threshold, prm.energy_tol, prm.min_note_len, prm.melodia_trick != 0,
                                    prm.include_pitch_bends != 0, skip, 0};
      pool_rows[(size_t)j + 1] = pool_rows[(size_t)j] + rows;
      if (rows == 0 || skip) continue;
      *queued = true;
      bends = bends || (prm.include_pitch_bends != 0 && !a.score);  // (a scored sweep counts the bends and makes none)
      if (set_key[(size_t)d.set] >= 0) continue;
      int lo = 0, hi = 88;
      bp_internal_freq_limits(&prm, &lo, &hi);
      set_key[(size_t)d.set] = found.emplace(std::make_tuple(lo, hi, prm.infer_onsets != 0, prm.onset_threshold), (int)found.size()).first->second;
    }
    if (int rc = check_rows_in_all(h, what, pool_rows[(size_t)n], "the decodes have ")) return rc;
    if (!*queued) {
      for (int64_t j = 0; j < n; ++j) a.out.status[j] = pool_rows[(size_t)j + 1] > pool_rows[(size_t)j] ? 1 : 0;
      for (int64_t j = 0; j <= n && !a.score; ++j) a.out.event_offsets[j] = 0;
      for (int64_t j = 0; j < n && a.score; ++j) score_nothing(j, pool_rows[(size_t)j + 1] - pool_rows[(size_t)j]);
      return BP_OK;
    }
    if (a.score) {  // the refs as the device reads them; which are whose
      const int64_t n_refs = a.ref_offsets[n_segs];
      score_refs.resize(a.scores ? (size_t)n_refs : 0);
      for (int64_t i = 0; i < n_refs && a.scores; ++i) {
        const bp_ref_note& r = a.refs[i];
        score_refs[(size_t)i] = NoteScoreRef{r.start_s, r.end_s, r.pitch_midi, bp_internal_score_offset_tol(&r, a.score_params)};
      }
      ref_of.resize((size_t)n);
      for (int64_t j = 0; j < n; ++j) {
        const int64_t first = a.ref_offsets[segment[(size_t)j]], rows = pool_rows[(size_t)j + 1] - pool_rows[(size_t)j];
        ref_of[(size_t)j] = NoteScoreDecode{first, (int32_t)std::min<int64_t>(a.ref_offsets[segment[(size_t)j] + 1] - first, kNoteScoreMaxNotes + 1),
                                            seg[(size_t)j].bends && rows <= kNoteTrackMaxRows ? (int32_t)(88 * rows) : -1};
      }
    }
    if (a.score && a.with_frames) {  // what depends on a ref and its segment alone, by the checker's own functions
      frame_refs.resize((size_t)a.ref_offsets[n_segs]);
      refs_in_pitch_order(n_segs, offs, a.ref_offsets, a.refs, [&](size_t slot, const bp_ref_note& ref, int32_t f0, int32_t f1) {
        frame_refs[slot].f0 = f0, frame_refs[slot].f1 = f1;
        bp_internal_frame_pitch_range(&ref, a.score_params, &frame_refs[slot].lo, &frame_refs[slot].hi);
      });
    }
    // the keys in the map's order, which keeps a band's keys together; a set's key by that order
    std::vector<int> order(found.size());
    for (const auto& kv : found) {
      const auto& [lo, hi, infer, thresh] = kv.first;
      const bool full = lo <= 0 && hi >= 88;
      if (!full && (keys.empty() || keys.back().lo != lo || keys.back().hi != hi)) ++n_bands;
      order[(size_t)kv.second] = (int)keys.size();
      keys.push_back(SweepKey{lo, hi, infer, thresh, full ? -1 : (int)n_bands - 1});
    }
    for (int& key : set_key)
      if (key >= 0) key = order[(size_t)key];
    ev = EventsJob{what, "n_decodes", n, pool_rows.data(), nullptr, seg.data(), nullptr, kNoteTrackFormAuto};
    return BP_OK;
  }

  // Behind the maps of the n_segs segments (T > 0 rows in all): the dense half once per key — the note rows constrained into
  // the band's copy where the band is new, the onset rows into the one working copy (the launches are serial: it is reused
  // from band to band), then the stats and the bitmap of every segment as the clips calls make them, into the key's own
  // blocks — and the bend map once; the tracker over the decode table; the offsets on their way home.  The maps themselves
  // are only read.  The records are in h->sw_stats, not the clips calls' h->clip_stats, whose state stays as it was.
  // score: no bend map, the tracker without its offsets and pack launches, then the scoring launch over the events where they
  // lie (note_score.hip) and the scores with the statuses on their way home.
  int queue(bp_handle h, const Maps& all, int64_t n_segs, const int64_t* offs) override {
    if (int rc = events_reserve(h, ev, &ev_plan, !a.score)) return rc;
    hipStream_t s = h->stream;
    const int64_t T = offs[n_segs], n = a.n_decodes, n_keys = (int64_t)keys.size();
    const int64_t plane = T * kFreqN, bits_plane = T * BP_NOTE_CAND_ROW_BYTES, stats_block = n_segs * (int64_t)kStatsBytes;
    const void* tab = nullptr;
    const double* gauss = nullptr;
    if (int rc = note_tables(h, &tab, &gauss)) return rc;
    uint8_t* unused = nullptr;
    int8_t* d_bend = nullptr;
    if (bends)
      if (int rc = reserve_candidates(h, T, &unused, &d_bend)) return rc;
    if (n_bands) {
      BP_HIP(h->sw_note.reserve((size_t)(n_bands * plane)));
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
    block.assign(tab_bytes + 2 * pre_bytes, 0);
    BP_HIP(h->sw_tab.reserve(block.size()));
    NoteSweepDecode* recs = reinterpret_cast<NoteSweepDecode*>(block.data());
    for (int64_t j = 0; j < n; ++j) {
      NoteSweepDecode& d = recs[j];
      const int64_t i = segment[(size_t)j];
      const int key = set_key[(size_t)params[(size_t)j]];
      d.first = offs[i], d.rows = offs[i + 1] - offs[i], d.seg = seg[(size_t)j];
      if (d.rows == 0 || d.seg.skip) continue;  // (never reaches the tracker's body: nothing of a key is read)
      const int band = keys[(size_t)key].band;
      d.note = band >= 0 ? h->sw_note + band * plane : all.note;
      d.bits = h->sw_bits + key * bits_plane;
      d.stats = h->sw_stats + key * stats_block + i * (int64_t)kStatsBytes;
    }
    std::memcpy(block.data() + tab_bytes, pool_rows.data(), pre_bytes);
    std::memcpy(block.data() + tab_bytes + pre_bytes, ev_plan.ev_first.data(), pre_bytes);
    const int64_t* d_rows = reinterpret_cast<const int64_t*>(h->sw_tab + tab_bytes);
    BP_HIP(hipMemcpyAsync(h->clip_rows, offs, (size_t)(n_segs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    BP_HIP(hipMemcpyAsync(h->sw_tab, block.data(), block.size(), hipMemcpyHostToDevice, s));
    if (a.score && want_scores) {
      // The LDS of the scoring launch: the most refs a decode it scores can have, the deepest its path can get — min(events,
      // refs + 1), the events bounded by what the decode's region of the pool holds.  Its tables go with the tracker's.
      for (int64_t j = 0; j < n; ++j) {
        const int n_ref = ref_of[(size_t)j].n_ref;
        if (n_ref > kNoteScoreMaxNotes) continue;  // status 3: never searched
        const int64_t room = ev_plan.ev_first[(size_t)j + 1] - ev_plan.ev_first[(size_t)j];
        max_refs = std::max(max_refs, n_ref);
        max_depth = std::max(max_depth, (int)std::min<int64_t>({room, (int64_t)n_ref + 1, (int64_t)kNoteScoreMaxNotes}));
      }
      BP_HIP(h->sc_refs.reserve(score_refs.size()));
      BP_HIP(h->sc_out.reserve((size_t)(5 * n)));
      BP_HIP(h->sc_home.reserve((size_t)(5 * n)));
      if (!score_refs.empty())
        BP_HIP(hipMemcpyAsync(h->sc_refs, score_refs.data(), score_refs.size() * sizeof(NoteScoreRef), hipMemcpyHostToDevice, s));
    }
    if (a.score) {  // which refs are whose: both scoring launches read it
      BP_HIP(h->sc_dec.reserve((size_t)n));
      BP_HIP(hipMemcpyAsync(h->sc_dec, ref_of.data(), (size_t)n * sizeof(NoteScoreDecode), hipMemcpyHostToDevice, s));
    }
    if (a.score && a.with_frames) {  // the frame launch's table, its counts [decodes][5] with the statuses (32-bit) behind them
      BP_HIP(h->fs_refs.reserve(frame_refs.size()));
      BP_HIP(h->fs_out.reserve((size_t)(5 * n + (n + 1) / 2)));
      BP_HIP(h->fs_home.reserve((size_t)(5 * n + (n + 1) / 2)));
      if (!frame_refs.empty())
        BP_HIP(hipMemcpyAsync(h->fs_refs, frame_refs.data(), frame_refs.size() * sizeof(NoteFrameRef), hipMemcpyHostToDevice, s));
    }
    launch_clips_stats_init(h->sw_stats, n_keys * n_segs, s);
    int made = 0;  // bands whose copies exist; sw_onset holds the last one's
    for (int64_t i = 0; i < n_keys; ++i) {
      const SweepKey& key = keys[(size_t)i];
      float *note = all.note, *onset = all.onset;
      if (key.band >= 0) {
        note = h->sw_note + key.band * plane, onset = h->sw_onset;
        if (key.band == made) launch_constrain_copy(all.note, all.onset, note, onset, T, key.lo, key.hi, s), ++made;
      }
      launch_clips_candidates(note, onset, all.contour, h->clip_rows, n_segs, T, 0, kFreqN, key.infer, key.onset_thresh, tab, gauss,
                              h->sw_stats + i * stats_block, h->sw_bits + i * bits_plane, i == 0 ? d_bend : nullptr, s);
    }
    BP_HIP(hipGetLastError());
    if (a.score) {  // the events stay where the tracker leaves them: one more launch, and 20 bytes per decode go home
      BP_HIP(launch_note_track_sweep(h->sw_tab.as<NoteSweepDecode>(), n, ev_plan.max_rows, nullptr, d_rows, d_rows + n + 1, h->ev_scratch,
                                     h->ev_pool, nullptr, h->ev_counts, nullptr, nullptr, nullptr, s));
      const bp_score_params& p = *a.score_params;
      if (want_scores) {
        BP_HIP(launch_note_score(h->ev_counts, d_rows + n + 1, h->ev_pool, h->sc_dec, h->sc_refs,
                                 NoteScoreParams{p.onset_tolerance_s, p.pitch_tolerance_cents, p.strict != 0}, n, max_refs, max_depth,
                                 h->sc_out, s));
        BP_HIP(hipMemcpyAsync(h->sc_home, h->sc_out, (size_t)(5 * n) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      }
      if (a.with_frames) {  // 40 bytes more per decode; the statuses too where the note-matching launch was skipped
        BP_HIP(launch_note_frames(h->ev_counts, d_rows, d_rows + n + 1, h->ev_pool, h->sc_dec, h->fs_refs, n, ev_plan.max_rows, h->fs_out, s));
        const size_t bytes = (size_t)(5 * n) * sizeof(int64_t) + (want_scores ? 0 : (size_t)n * sizeof(int32_t));
        BP_HIP(hipMemcpyAsync(h->fs_home, h->fs_out, bytes, hipMemcpyDeviceToHost, s));
      }
      return BP_OK;
    }
    BP_HIP(launch_note_track_sweep(h->sw_tab.as<NoteSweepDecode>(), n, ev_plan.max_rows, d_bend, d_rows, d_rows + n + 1, h->ev_scratch,
                                   h->ev_pool, h->bd_pool, h->ev_counts, h->ev_meta, h->ev_out, h->bd_out, s));
    BP_HIP(hipMemcpyAsync(h->ev_home, h->ev_meta, (size_t)(3 * n + 2) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return BP_OK;
  }

  // the events home; a scored sweep: the scores and the statuses are in the page-locked blocks
  int home(bp_handle h, const char*, int64_t, const int64_t*) override {
    if (!a.score) return events_home(h, ev, a.out, nullptr);
    const int64_t n = a.n_decodes;
    if (want_scores) std::memcpy(a.scores, h->sc_home, (size_t)n * sizeof(bp_note_score));
    if (a.with_frames) std::memcpy(a.frames, h->fs_home, (size_t)n * sizeof(bp_frame_score));
    const int32_t* st = want_scores ? h->sc_home + 4 * n : statuses_behind(h->fs_home, 5 * n);
    for (int64_t j = 0; j < n; ++j) a.out.status[j] = st[j];
    return BP_OK;
  }
};

SweepSink::Args events_of(int64_t n_sets, const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes, bp_note_event* events,
                          int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets, int* status) {
  return {false, false, n_sets, sets, n_decodes, decodes, EventsSink{events, max_events, bends, max_bends, event_offsets, status}};
}
// frames null: the note level alone (include/basic_pitch_amd_score.h)
SweepSink::Args scored(bool with_frames, int64_t n_sets, const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                       const int64_t* ref_offsets, const bp_ref_note* refs, const bp_score_params* score_params, bp_note_score* scores,
                       bp_frame_score* frames, int* status) {
  return {true, with_frames, n_sets, sets, n_decodes, decodes, EventsSink{nullptr, 0, nullptr, 0, nullptr, status},
          ref_offsets, refs, score_params, scores, frames};
}

}  // namespace

extern "C" {

int bp_note_events_sweep(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, const float* onset,
                         const float* contour, int mem_kind, int64_t n_sets, const bp_note_params* sets, int64_t n_decodes,
                         const bp_sweep_decode* decodes, bp_note_event* events, int64_t max_events, int32_t* bends, int64_t max_bends,
                         int64_t* event_offsets, int* status) {
  SweepSink sink(events_of(n_sets, sets, n_decodes, decodes, events, max_events, bends, max_bends, event_offsets, status));
  return run_clips(h, "bp_note_events_sweep", given_maps(n_segments, row_offsets, note, onset, contour, mem_kind), sink);
}

int bp_infer_clips_events_sweep(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind, int64_t n_sets,
                                const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes, bp_note_event* events,
                                int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets, int* status) {
  SweepSink sink(events_of(n_sets, sets, n_decodes, decodes, events, max_events, bends, max_bends, event_offsets, status));
  return run_clips(h, "bp_infer_clips_events_sweep", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

// ---- a scored sweep (include/basic_pitch_amd_score.h) -----------------------------------------------------------------------------
int bp_note_events_sweep_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, const float* onset,
                               const float* contour, int mem_kind, int64_t n_sets, const bp_note_params* sets, int64_t n_decodes,
                               const bp_sweep_decode* decodes, const int64_t* ref_offsets, const bp_ref_note* refs,
                               const bp_score_params* score_params, bp_note_score* scores, int* status) {
  SweepSink sink(scored(false, n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, nullptr, status));
  return run_clips(h, "bp_note_events_sweep_score", given_maps(n_segments, row_offsets, note, onset, contour, mem_kind), sink);
}

int bp_infer_clips_events_sweep_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                      int64_t n_sets, const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                                      const int64_t* ref_offsets, const bp_ref_note* refs, const bp_score_params* score_params,
                                      bp_note_score* scores, int* status) {
  SweepSink sink(scored(false, n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, nullptr, status));
  return run_clips(h, "bp_infer_clips_events_sweep_score", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

// ---- a sweep scored at the note and the frame level (include/basic_pitch_amd_frame_score.h) ----------------------------------------
int bp_note_events_sweep_frame_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note,
                                     const float* onset, const float* contour, int mem_kind, int64_t n_sets,
                                     const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                                     const int64_t* ref_offsets, const bp_ref_note* refs, const bp_score_params* score_params,
                                     bp_note_score* scores, bp_frame_score* frames, int* status) {
  SweepSink sink(scored(true, n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, frames, status));
  return run_clips(h, "bp_note_events_sweep_frame_score", given_maps(n_segments, row_offsets, note, onset, contour, mem_kind), sink);
}

int bp_infer_clips_events_sweep_frame_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                            int64_t n_sets, const bp_note_params* sets, int64_t n_decodes,
                                            const bp_sweep_decode* decodes, const int64_t* ref_offsets, const bp_ref_note* refs,
                                            const bp_score_params* score_params, bp_note_score* scores, bp_frame_score* frames,
                                            int* status) {
  SweepSink sink(scored(true, n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, frames, status));
  return run_clips(h, "bp_infer_clips_events_sweep_frame_score", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

}  // extern "C"
