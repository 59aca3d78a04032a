// C ABI of the streaming sessions (include/basic_pitch_amd.h, include/basic_pitch_amd_live.h, include/basic_pitch_amd_rolling.h,
// include/basic_pitch_amd_update.h, include/basic_pitch_amd_stream_events.h): audio that arrives over time -> the rows of the un-overlapped
// posteriorgrams as they become final, for one stream or for many streams of one handle per step.
//
// A stream keeps on the device a ring of the model-rate signal that reaches back to the first sample of its oldest
// incomplete window and, when it resamples, the last ceil(n_taps / up) mono input frames; its counters are absolute int64
// on the host.  A step (step()) is: validate everything -> plan -> queue -> wait.  The plan is made on the host from the
// counters alone: rounds of (per stream: as much of the chunk as the ring has room for, resampled at absolute output
// indices) + (the windows that are now complete, of all streams, packed into one chunk of the handle's workspace: one
// WindowSeg per stream, the track calls' descriptor with a source that wraps).  A round queues one windowing launch, the
// model and one un-overlapping launch, however many streams take part; the segments of all rounds travel to the device in
// one copy.
//
// Why the rows equal the one-shot call's, bit for bit: the downmix, the resampling sum, the window gather and the row
// scatter are the one-shot calls' own device functions (audio_ingest.hip mono_frame / resample_sum, cqt_pyramid.hip
// gather_window / scatter_window); a resampled sample is one float64 sum over the same frames with the same taps in the
// same order wherever the chunk boundaries fall, a window's samples depend on its index alone, and a window's result does
// not depend on its batch or its slot.
//
// A step has three modes.  A push and a finish commit: the plan's copies of the counters become the stream's.  A PEEK is the
// finish plan made on the same copies and never written back: "the rows a finish would emit now".  Its only trace on the
// device is the tail of the model-rate signal (samples n_res up to the resampled length, their sums clipped at the last
// frame) in the ring's free room beyond n_res:
//   * the room always suffices — every step runs all complete windows, so the ring holds less than one window of samples
//     afterwards and more than kRingHops hops are free, while the tail is at most centre / down + 2 samples (the samples whose
//     filter reaches past the last frame); tail_fits() checks it before anything is queued;
//   * a later push ingests from the stream's own n_res, which the peek left alone: it rewrites those ring positions with the
//     complete sums before its windows are planned, and a window is gathered only up to the plan's n_res — no clipped,
//     provisional sum can reach a final row.
// The history buffers and cur_hist belong to the downmix of a chunk, and a peek has no chunk.
//
// bp_stream_keep and bp_stream_keep_rolling give a stream ONE store of retained rows (bp_stream_state::KeptRows): the three
// maps of its rows (1,760 bytes per row), frequency-constrained, in a ring of `cap` rows, absolute row r at slot r % cap, that
// holds the last `horizon` rows and the room of a tail (note_device.hip, "the rows a stream retains").  Final rows enter it
// as they are emitted (launch_ring_put), the rows of a tail at every update.  An update decodes rows [a, T),
// a = max(0, T - horizon), as a whole track — their stats record, the bitmap (12 bytes a row: it depends on both maxima and on
// the row count) and the bends, all counted from a — and sends home the bitmap and the note and bend rows the caller does not
// hold yet: not the maps.
//   * bp_stream_keep reserves cap = horizon = max_rows + a tail's room: the ring never wraps, a stays 0, the caller's linear
//     arrays are host rings that never wrap either, and a step past max_rows is refused.  The extrema of the final rows are
//     carried in one record, which they join as they are emitted; an update joins the tail to a copy of it in the handle's
//     table of update records.
//   * bp_stream_keep_rolling reserves horizon_rows + a tail's room.  Rows leave the slice, which one record cannot follow, so
//     the final rows fill a table of records, one per block of 64 absolute rows, and an update joins the record of the slice
//     from the table's whole blocks and a scan of the edge rows.  Nothing such a stream owns, sends home or computes per
//     update grows with its age.
//
// Every update is one step of n streams of either mode (queue_updates): one peek step for all tails, one table of streams
// (StreamUpdate, note_device.hip "the updates of streams"), the segmented launches, and the results packed and linear in the
// handle's buffers.  What becomes of them is the entry point's (UpdateResults):
//   * bp_streams_candidates has the packed rows and the records copied home as they lie;
//   * bp_stream_candidates and bp_stream_candidates_rolling are the step of ONE stream — their own argument checks and
//     messages, then a table of one — and copy the rows from the packed buffers into the caller's host rings, split where a
//     ring wraps (copy_to_host_ring);
//   * bp_streams_events sends nothing home (every stream's whole slice stays packed) and runs the tracker of the clips calls
//     behind it (note_track.hip, a segment per stream with the stream's own parameters; clips_api.hip events_reserve /
//     events_queue / events_home): the events and their bends are all that crosses PCIe.
//
// A stream's ring, history and kept maps are buffers that free themselves (device_buffer.h): bp_stream_close sets the
// handle's device and deletes the state, and an open or keep that fails leaves nothing behind.
#include <algorithm>
#include <cstring>
#include <memory>

#include "bp_context.h"
#include "../../include/basic_pitch_amd_stream_events.h"

using namespace bp;

extern "C" void bp_internal_freq_limits(const bp_note_params* prm, int* lo, int* hi);  // note_decode.cpp

struct bp_stream_state {
  bp_handle h = nullptr;
  int format = 0, channels = 0, sample_rate = 0;
  bool resamples = false;  // false: the input is at the handle's rate and is only converted and downmixed
  ResamplePlan plan{};
  const double* taps = nullptr;  // the handle's table for this rate
  int n_hist = 0;                // ceil(n_taps / up) frames; 0 without resampling
  int ring_cap = 0;
  DeviceBuffer<float> ring;
  DeviceBuffer<float> hist;  // both halves in one block: half i at hist + i * n_hist
  int cur_hist = 0;
  int64_t n_in = 0;      // input frames taken
  int64_t n_res = 0;     // samples of the model-rate signal made
  int64_t w_next = 0;    // first window that has not run
  int64_t rows_out = 0;  // rows emitted
  bool finished = false, broken = false;
  // bp_stream_keep / bp_stream_keep_rolling: the maps of the last `horizon` rows and a tail's room ([cap] note, onset, contour;
  // absolute row r at slot r % cap), frequency-constrained for `prm`, and the stats records of note_device.hip that carry
  // their extrema: the record the final rows join (table: the block table of a rolling horizon).  The last record of `rec` is
  // reserved and unused (an update's record lies in the handle's table, h->up_stats); it stays in the documented
  // bp_stream_state_bytes.
  struct KeptRows {
    int64_t cap = 0, horizon = 0;  // cap == 0: the stream retains nothing
    int64_t limit = INT64_MAX;     // final rows a step may reach: bp_stream_keep reserves no more
    bool table = false;
    DeviceBuffer<float> rows, rec;
  } kept;
  bp_note_params prm{};
  int lo = 0, hi = 88;
#ifdef BP_AB_KERNELS
  // bp_ab_stream_poison (the A/B library only): the cell of the kept copy that becomes a NaN when its row is written
  int64_t ab_nan_row = -1;
  int ab_nan_map = 0, ab_nan_bin = 0;
#endif
};

namespace {

// windows a ring holds beyond the incomplete one: a push of more audio than that runs in several rounds
constexpr int kRingHops = 4;

int64_t complete_windows(int64_t n, int win_len, int hop, int lead) {
  const int64_t first = (int64_t)win_len - lead;  // window w is complete at w * hop - lead + win_len samples
  return n < first ? 0 : (n - first) / hop + 1;
}

// samples of the model-rate signal whose whole sum has arrived with `n_in` input frames: k down + centre <= n_in up - 1
int64_t ready_samples(const bp_stream_state* s, int64_t n_in) {
  if (!s->resamples) return n_in;
  const int64_t t = n_in * s->plan.up - 1 - s->plan.centre;
  return t < 0 ? 0 : t / s->plan.down + 1;
}

// rows a push of n_frames (finish: the end of the signal) adds to those already emitted
int64_t rows_of_step(const bp_stream_state* s, int64_t n_frames, bool finish) {
  bp_handle h = s->h;
  int64_t rows;
  if (finish)
    rows = bp_handle_track_n_frames(h, bp_handle_resampled_length(h, s->n_in, s->sample_rate));
  else
    rows = complete_windows(std::max(s->n_res, ready_samples(s, s->n_in + n_frames)), h->win_len, h->hop, h->lead) *
           BP_FRAMES_PER_WINDOW;
  return std::max<int64_t>(0, rows - s->rows_out);
}

int stream_taps(bp_handle h, bp_stream_state* s) {
  for (const auto& t : h->st_taps)
    if (t.rate == s->sample_rate) {
      s->plan = t.plan;
      s->taps = t.dev;
      return BP_OK;
    }
  ResamplePlan pl{};
  DeviceBuffer<double> dev;
  if (int rc = upload_filter(h, s->sample_rate, true, &pl, &dev)) {
    if (rc == BP_ERR_UNSUPPORTED)
      h->err = "bp_stream_open: " + std::to_string(s->sample_rate) + " Hz -> " + std::to_string(h->rate) +
               " Hz needs a filter of " + std::to_string(pl.n_taps) +
               " taps, which the one-shot calls evaluate in the kernel; such ratios are not streamed";
    return rc;
  }
  s->plan = pl;
  s->taps = dev;
  h->st_taps.push_back({s->sample_rate, std::move(dev), pl});
  return BP_OK;
}

// rows a peek can have: the windows that have not run when every complete one has are at most two (window > hop)
constexpr int64_t kTailRows = 2 * BP_FRAMES_PER_WINDOW;
constexpr int64_t kStatsFloats = 4;  // a stats record of note_device.hip: 16 bytes

Maps rows_from(const Maps& m, int64_t r) { return {m.note + r * kFreqN, m.onset + r * kFreqN, m.contour + r * kFreqC}; }
int64_t n_records(const bp_stream_state::KeptRows& k) { return k.table ? note_ring_records(k.cap) : 2; }
int64_t kept_bytes(const bp_stream_state* s) {
  return s->kept.cap ? (s->kept.cap * kMapsRow + n_records(s->kept) * kStatsFloats) * 4 : 0;
}

// Rows [r0, r1) of the linear device maps `src` (its row 0 is row r0; r1 - r0 <= cap) go to their slots of the store,
// frequency-constrained on the way; they have not joined a stats record yet.  In the A/B library the cell that
// bp_ab_stream_poison names, if it lies in them, then becomes a quiet NaN — after the constraint, so a poisoned cell outside
// [lo, hi) stays a NaN in either mode.  The product library has no such hook.
int poison_rows(bp_handle h, const bp_stream_state* s, int64_t r0, int64_t r1) {
#ifdef BP_AB_KERNELS
  const auto& k = s->kept;
  if (s->ab_nan_row >= r0 && s->ab_nan_row < r1) {
    const Maps kept = maps_at(k.rows, k.cap);
    float* cell = (s->ab_nan_map ? kept.onset : kept.note) + (s->ab_nan_row % k.cap) * kFreqN + s->ab_nan_bin;
    BP_HIP(hipMemsetD32Async(cell, 0x7fc00000, 1, h->stream));
  }
#endif
  return BP_OK;
}

int put_rows(bp_handle h, const bp_stream_state* s, const Maps& src, int64_t r0, int64_t r1) {
  const auto& k = s->kept;
  launch_ring_put(src.note, src.onset, src.contour, k.rows, k.cap, r0, r1 - r0, s->lo, s->hi, h->stream);
  BP_HIP(hipGetLastError());
  return poison_rows(h, s, r0, r1);
}

// the tail of the signal a peek makes (samples n_res ... resampled length) fits the ring's free room: see the file header
bool tail_fits(const bp_stream_state* s) {
  bp_handle h = s->h;
  const int64_t keep = std::max<int64_t>(0, s->w_next * h->hop - h->lead);
  return bp_handle_resampled_length(h, s->n_in, s->sample_rate) - s->n_res <= s->ring_cap - (s->n_res - keep);
}

// ---- one step of n streams ------------------------------------------------------------------------------------------------
enum Mode { kPush, kFinish, kPeek };

struct Entry {
  bp_stream_state* s;
  const uint8_t* pcm;  // the chunk where the kernels read it (device)
  int64_t n_frames;
  bool finish;         // planned as the end of the signal (a finish, a peek)
  bool peek;           // ... on copies of the counters that are not written back
  Maps out;            // the rows of this call where the kernels write them (device)
  Maps user;
  int64_t rows;
  const float* mono;   // the chunk's mono form (resampling streams)
  // the plan's copy of the counters
  int64_t n_res, w_next, n_total;
};

// a stream's entry of a step: the plan's copies start as the stream's counters
Entry plan_entry(bp_stream_state* s, Mode mode, int64_t n_frames, int64_t rows, const Maps& user) {
  Entry e{};
  e.s = s;
  e.finish = mode != kPush;
  e.peek = mode == kPeek;
  e.n_frames = n_frames;
  e.rows = rows;
  e.user = user;
  e.n_res = s->n_res;
  e.w_next = s->w_next;
  e.n_total = e.finish ? bp_handle_resampled_length(s->h, s->n_in, s->sample_rate) : -1;
  return e;
}

struct Ingest {
  int e;
  int64_t k0, n_k;
};
struct Round {
  std::vector<Ingest> ingests;
  int seg0 = 0, n_segs = 0, n_slots = 0;  // its segments in the step's table, its windows
};

int queue_step(bp_handle h, std::vector<Entry>& es, const void* const* pcm, int pcm_mem_kind, int out_mem_kind,
               std::vector<WindowSeg>& segs) {
  hipStream_t q = h->stream;
  // scratch of the step, grown before anything is queued: the chunks (host PCM; each at a multiple of 16 bytes), their mono
  // form, the rows (host outputs)
  int64_t pcm_bytes = 0, mono_floats = 0, out_floats = 0;
  for (auto& e : es) {
    const int64_t bytes = e.n_frames * e.s->channels * pcm_width(e.s->format);
    if (pcm_mem_kind == BP_MEM_HOST) pcm_bytes += (bytes + 15) / 16 * 16;
    if (e.s->resamples) mono_floats += (e.n_frames + 3) / 4 * 4;
    if (out_mem_kind == BP_MEM_HOST) out_floats += e.rows * kMapsRow;
  }
  int rc;
  BP_HIP(h->st_pcm.reserve((size_t)pcm_bytes));
  BP_HIP(h->st_mono.reserve((size_t)mono_floats));
  BP_HIP(h->st_out.reserve((size_t)out_floats));
  int64_t pcm_at = 0, mono_at = 0, out_at = 0;
  for (size_t i = 0; i < es.size(); ++i) {
    Entry& e = es[i];
    const int64_t bytes = e.n_frames * e.s->channels * pcm_width(e.s->format);
    e.pcm = static_cast<const uint8_t*>(pcm ? pcm[i] : nullptr);
    if (pcm_mem_kind == BP_MEM_HOST) {
      e.pcm = h->st_pcm + pcm_at;
      pcm_at += (bytes + 15) / 16 * 16;
    }
    e.mono = h->st_mono + mono_at;
    if (e.s->resamples) mono_at += (e.n_frames + 3) / 4 * 4;
    e.out = e.user;
    if (out_mem_kind == BP_MEM_HOST) {
      e.out = maps_at(h->st_out + out_at, e.rows);
      out_at += e.rows * kMapsRow;
    }
  }

  // ---- the plan: rounds of ingest + complete windows, from the counters alone
  std::vector<Round> rounds;
  segs.clear();
  for (;;) {
    Round r;
    r.seg0 = (int)segs.size();
    for (size_t i = 0; i < es.size(); ++i) {
      Entry& e = es[i];
      const bp_stream_state* s = e.s;
      const int64_t keep = std::max<int64_t>(0, e.w_next * h->hop - h->lead);  // oldest sample a window still needs
      const int64_t room = s->ring_cap - (e.n_res - keep);
      const int64_t have = e.finish ? e.n_total : ready_samples(s, s->n_in + e.n_frames);
      const int64_t n_k = std::min(room, have - e.n_res);
      if (n_k > 0) {
        r.ingests.push_back({(int)i, e.n_res, n_k});
        e.n_res += n_k;
      }
    }
    for (size_t i = 0; i < es.size() && r.n_slots < h->cap; ++i) {
      Entry& e = es[i];
      const bp_stream_state* s = e.s;
      const int64_t n_win = e.finish && e.n_res == e.n_total ? bp_handle_track_n_windows(h, e.n_total)
                                                             : complete_windows(e.n_res, h->win_len, h->hop, h->lead);
      const int n = (int)std::min<int64_t>(n_win - e.w_next, h->cap - r.n_slots);
      if (n <= 0) continue;
      // the stream's windows of this round: a track's piece whose source wraps, its rows counted from this call's first
      // (a window's rows are emitted by the step that runs it; finish: e.rows ends at T)
      segs.push_back(WindowSeg{s->ring, {e.out.note, e.out.onset, e.out.contour}, e.n_res, e.w_next * h->hop - h->lead,
                               e.w_next * BP_FRAMES_PER_WINDOW - s->rows_out, e.rows, s->ring_cap, n, r.n_slots});
      e.w_next += n;
      r.n_slots += n;
    }
    r.n_segs = (int)segs.size() - r.seg0;
    if (r.ingests.empty() && r.n_slots == 0) break;
    rounds.push_back(std::move(r));
  }

  // ---- queue: the chunks, their mono form and the next history; the segment table; the rounds; the rows
  for (size_t i = 0; i < es.size(); ++i) {
    Entry& e = es[i];
    bp_stream_state* s = e.s;
    if (e.n_frames == 0) continue;
    if (pcm_mem_kind == BP_MEM_HOST)
      BP_HIP(hipMemcpyAsync(const_cast<uint8_t*>(e.pcm), pcm[i], (size_t)(e.n_frames * s->channels * pcm_width(s->format)),
                            hipMemcpyHostToDevice, q));
    if (s->resamples)
      launch_stream_downmix(e.pcm, s->format, e.n_frames, s->channels, const_cast<float*>(e.mono), 0, 0, s->hist + s->cur_hist * s->n_hist,
                            s->hist + (s->cur_hist ^ 1) * s->n_hist, s->n_hist, q);
  }
  if (!segs.empty()) {
    BP_HIP(h->st_segs.reserve(segs.size()));
    BP_HIP(hipMemcpyAsync(h->st_segs, segs.data(), segs.size() * sizeof(WindowSeg), hipMemcpyHostToDevice, q));
  }
  const WindowSeg* d_segs = h->st_segs;
  for (const Round& r : rounds) {
    for (const Ingest& g : r.ingests) {
      const Entry& e = es[g.e];
      bp_stream_state* s = e.s;
      const int pos = (int)(g.k0 % s->ring_cap);
      if (s->resamples)
        launch_stream_resample(s->hist + s->cur_hist * s->n_hist, s->n_hist, e.mono, s->n_in, s->n_in + e.n_frames, s->taps, s->plan, g.k0,
                               g.n_k, s->ring, pos, s->ring_cap, q);
      else  // frames [k0, k0 + n_k) of the signal are frames k0 - n_in onwards of the chunk
        launch_stream_downmix(e.pcm + (g.k0 - s->n_in) * s->channels * pcm_width(s->format), s->format, g.n_k, s->channels,
                              s->ring, pos, s->ring_cap, nullptr, nullptr, 0, q);
    }
    if (r.n_slots == 0) continue;
    launch_window_streams(d_segs + r.seg0, r.n_segs, r.n_slots, h->audio, h->win_len, h->hop, q);
    if ((rc = run_chunk(h, h->audio, r.n_slots, h->note, h->onset, h->contour))) return rc;
    launch_unwrap_streams(d_segs + r.seg0, r.n_segs, r.n_slots, h->note, h->onset, h->contour, q);
  }
  BP_HIP(hipGetLastError());
  // streams that retain their maps: the final rows of this step go to their slots and join the record or the table — the
  // last `cap` of them at most: a row further back has left every later slice, and so has the block it starts
  for (const Entry& e : es) {
    const bp_stream_state* s = e.s;
    const auto& k = s->kept;
    if (!k.cap || e.peek || e.rows == 0) continue;
    const int64_t r1 = s->rows_out + e.rows, r0 = std::max(s->rows_out, r1 - k.cap);
    if ((rc = put_rows(h, s, rows_from(e.out, r0 - s->rows_out), r0, r1))) return rc;
    if (k.table)
      launch_ring_fold(k.rows, k.cap, r0, r1, r0 > s->rows_out ? 0 : r0, s->prm.infer_onsets != 0, k.rec, q);
    else  // the ring never wraps: linear maps
      launch_note_fold(k.rows, k.rows + k.cap * kFreqN, r0, r1, s->prm.infer_onsets != 0, k.rec, q);
    BP_HIP(hipGetLastError());
  }
  for (const Entry& e : es)
    if (out_mem_kind == BP_MEM_HOST && e.rows > 0 && (rc = copy_maps(h, e.user, e.out, e.rows, hipMemcpyDeviceToHost))) return rc;
  return BP_OK;
}

// The tail of a stream that retains its maps: the peek's rows through the step's scratch into the slots behind the final
// rows (nothing committed; the next final rows overwrite them).
int queue_tail(bp_handle h, bp_stream_state* s, int64_t tail_rows, std::vector<WindowSeg>& segs) {
  if (tail_rows <= 0) return BP_OK;
  BP_HIP(h->st_out.reserve((size_t)(tail_rows * kMapsRow)));
  std::vector<Entry> es{plan_entry(s, kPeek, 0, tail_rows, maps_at(h->st_out, tail_rows))};
  if (int rc = queue_step(h, es, nullptr, BP_MEM_HOST, BP_MEM_DEVICE, segs)) return rc;
  return put_rows(h, s, es[0].user, s->rows_out, s->rows_out + tail_rows);
}

// Rows [r0, r1), linear on the device with row r0 first, to a host ring of ring_rows rows (row r at r % ring_rows): one copy,
// and one more wherever the ring wraps.
int copy_to_host_ring(bp_handle h, void* ring, int64_t ring_rows, const void* src, int64_t row_bytes, int64_t r0, int64_t r1) {
  for (int64_t r = r0; r < r1;) {
    const int64_t at = r % ring_rows, n = std::min(r1 - r, ring_rows - at);
    BP_HIP(hipMemcpyAsync(static_cast<uint8_t*>(ring) + at * row_bytes, static_cast<const uint8_t*>(src) + (r - r0) * row_bytes,
                          (size_t)(n * row_bytes), hipMemcpyDeviceToHost, h->stream));
    r += n;
  }
  return BP_OK;
}

// What becomes of the results of an update step, which queue_updates leaves packed and linear on the device: the bitmaps of
// all slices in h->up_bits, the note rows and bends of [new_row, n_rows) in h->up_note / up_bend, the n records in h->up_stats,
// the prefix arrays behind the table in h->up_tab.
struct UpdateResults {
  bool bends;         // the streams whose parameters include bends get them
  bool records_home;  // the n records go to h->up_stats_host, where [i * 4 + 1] is stream i's NaN flag: the caller's status
  float* note;        // the packed rows go home into these three as they lie; bits == null: they stay on the device
  int8_t* bend;
  uint8_t* bits;
  // bp_streams_candidates: everything home, packed; bends if the caller gave room for them
  static UpdateResults packed_home(float* note, int8_t* bend, uint8_t* bits) { return {bend != nullptr, true, note, bend, bits}; }
  // bp_stream_candidates[_rolling]: the caller copies the rows into host rings; bends if it has a bend ring
  static UpdateResults for_host_rings(bool bend_ring) { return {bend_ring, true, nullptr, nullptr, nullptr}; }
  // bp_streams_events: the tracker reads rows and records where they lie
  static UpdateResults for_tracker() { return {true, false, nullptr, nullptr, nullptr}; }
};

// An update of n streams that retain their maps (u: the out fields filled, plan_updates; tail[i]: the rows of stream i's peek):
// the tails of all streams through one peek step into the scratch, the table of streams in one copy, the segmented launches
// of note_device.hip — the tails into the stores, per stream the record of its slice [a, T), the bitmap, the bends and the
// note rows from new_row on.  `tab`: the table's host form, alive until the wait.
int queue_updates(bp_handle h, int64_t n, const bp_stream_update* u, const std::vector<int64_t>& tail, int64_t note_rows,
                  int64_t bits_rows, std::vector<WindowSeg>& segs, std::vector<uint8_t>& tab, const UpdateResults& out) {
  hipStream_t q = h->stream;
  const void* bend_tab = nullptr;
  const double* gauss = nullptr;
  int rc = note_tables(h, &bend_tab, &gauss);
  if (rc) return rc;
  const size_t m = (size_t)n + 1;
  tab.assign((size_t)n * sizeof(StreamUpdate) + kStreamUpdatePrefixes * m * sizeof(int64_t), 0);
  StreamUpdate* d = reinterpret_cast<StreamUpdate*>(tab.data());
  int64_t* pre = reinterpret_cast<int64_t*>(tab.data() + (size_t)n * sizeof(StreamUpdate));
  int64_t *pre_tail = pre, *pre_chunk = pre + m, *pre_bits = pre + 2 * m, *pre_bend = pre + 3 * m, *pre_note = pre + 4 * m;
  // everything the step needs, before anything is queued
  int64_t tail_rows = 0;
  for (int64_t t : tail) tail_rows += t;
  bool bends = false;
  for (int64_t i = 0; i < n; ++i) bends = bends || (out.bends && u[i].stream->prm.include_pitch_bends != 0 && u[i].n_rows > u[i].new_row);
  BP_HIP(h->st_out.reserve((size_t)(tail_rows * kMapsRow)));
  BP_HIP(h->up_tab.reserve(tab.size()));
  BP_HIP(h->up_note.reserve((size_t)(note_rows * kFreqN)));
  BP_HIP(h->up_bend.reserve(bends ? (size_t)(note_rows * kFreqN) : 0));
  BP_HIP(h->up_bits.reserve((size_t)(bits_rows * BP_NOTE_CAND_ROW_BYTES)));
  BP_HIP(h->up_stats.reserve((size_t)(n * kStatsFloats * 4)));
  BP_HIP(h->up_stats_host.reserve((size_t)(n * kStatsFloats)));

  std::vector<Entry> es;
  int64_t at = 0;
  for (int64_t i = 0; i < n; ++i) {
    bp_stream_state* s = u[i].stream;
    const auto& k = s->kept;
    const int64_t t = tail[(size_t)i], T = u[i].n_rows, a = u[i].first_row, n0 = u[i].new_row, R = s->rows_out;
    const Maps rows = maps_at(h->st_out + at * kMapsRow, t);
    if (t > 0) es.push_back(plan_entry(s, kPeek, 0, t, rows));
    at += t;
    StreamUpdate& e = d[i];
    e.ring = k.rows;
    e.tail_note = rows.note, e.tail_onset = rows.onset, e.tail_contour = rows.contour;
    e.records = k.rec;
    e.cap = k.cap, e.a = a, e.R = R, e.T = T, e.n0 = n0;
    e.e0 = a, e.e1 = R;  // a keeping stream: the tail joins a copy of the carried record
    if (k.table && T > a) note_ring_edges(a, R, T, &e.e0, &e.e1);
    e.n_tab = k.table ? n_records(k) - 1 : 0;
    e.note_offset = u[i].note_offset, e.bits_offset = u[i].bits_offset;
    e.onset_thresh = s->prm.onset_threshold;
    e.lo = s->lo, e.hi = s->hi, e.infer = s->prm.infer_onsets != 0;
    e.bends = out.bends && s->prm.include_pitch_bends != 0;
    pre_tail[i + 1] = pre_tail[i] + t;
    pre_chunk[i + 1] = pre_chunk[i] + streams_stats_chunks((e.e0 - a) + (T - e.e1));
    pre_bits[i + 1] = pre_bits[i] + (T - a);
    pre_bend[i + 1] = pre_bend[i] + (e.bends ? streams_bend_blocks(T - n0) : 0);
    pre_note[i + 1] = pre_note[i] + (T - n0);
  }
  if (!es.empty() && (rc = queue_step(h, es, nullptr, BP_MEM_HOST, BP_MEM_DEVICE, segs))) return rc;
  BP_HIP(hipMemcpyAsync(h->up_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, q));
  const StreamUpdate* d_tab = h->up_tab.as<StreamUpdate>();
  const int64_t* d_pre = reinterpret_cast<const int64_t*>(h->up_tab + (size_t)n * sizeof(StreamUpdate));
  launch_streams_put(d_tab, d_pre, n, tail_rows, q);
  BP_HIP(hipGetLastError());
  for (int64_t i = 0; i < n; ++i)  // the A/B library's hook, as put_rows applies it
    if ((rc = poison_rows(h, u[i].stream, d[i].R, d[i].T))) return rc;
  launch_streams_candidates(d_tab, d_pre, n, pre_chunk[n], bits_rows, pre_bend[n], note_rows, bend_tab, gauss, h->up_stats, h->up_bits,
                            h->up_bend, h->up_note, q);
  BP_HIP(hipGetLastError());
  if (out.records_home) BP_HIP(hipMemcpyAsync(h->up_stats_host, h->up_stats, (size_t)(n * kStatsFloats * 4), hipMemcpyDeviceToHost, q));
  if (!out.bits) return BP_OK;
  BP_HIP(hipMemcpyAsync(out.bits, h->up_bits, (size_t)(bits_rows * BP_NOTE_CAND_ROW_BYTES), hipMemcpyDeviceToHost, q));
  if (note_rows > 0) BP_HIP(hipMemcpyAsync(out.note, h->up_note, (size_t)(note_rows * kFreqN * 4), hipMemcpyDeviceToHost, q));
  if (bends) BP_HIP(hipMemcpyAsync(out.bend, h->up_bend, (size_t)(note_rows * kFreqN), hipMemcpyDeviceToHost, q));
  return BP_OK;
}

// the slice [a, T) of the store, linear, to the caller's host maps: one copy per map, two where the slots wrap
int queue_rolling_maps(bp_handle h, bp_stream_state* s, int64_t tail_rows, const Maps& out, std::vector<WindowSeg>& segs) {
  int rc;
  if ((rc = queue_tail(h, s, tail_rows, segs))) return rc;
  const auto& k = s->kept;
  const int64_t T = s->rows_out + tail_rows, a = bp_stream_horizon_first_row(T, k.horizon);
  const Maps ring = maps_at(k.rows, k.cap);
  for (int64_t r = a; r < T;) {
    const int64_t at = r % k.cap, n = std::min(T - r, k.cap - at);
    if ((rc = copy_maps(h, rows_from(out, r - a), rows_from(ring, at), n, hipMemcpyDeviceToHost))) return rc;
    r += n;
  }
  return BP_OK;
}

// validate everything -> queue -> wait -> the streams' counters (a peek leaves them).  pcm / n_frames: NULL for finish / peek.
int step(bp_handle h, const char* what, int64_t n, const bp_stream* streams, const void* const* pcm, const int64_t* n_frames,
         int pcm_mem_kind, float* const* note, float* const* onset, float* const* contour, const int64_t* capacity_rows,
         int out_mem_kind, int64_t* rows, Mode mode) {
  const bool finish_streams = mode != kPush;
  auto invalid = [&](const std::string& why) {
    h->err = std::string(what) + ": " + why;
    return BP_ERR_INVALID_ARG;
  };
  if (n < 0 || (out_mem_kind != BP_MEM_HOST && out_mem_kind != BP_MEM_DEVICE) ||
      (pcm_mem_kind != BP_MEM_HOST && pcm_mem_kind != BP_MEM_DEVICE))
    return invalid("negative count or unknown mem_kind");
  if (n > 0 && (!streams || !rows || !capacity_rows || !note || !onset || !contour || (!finish_streams && (!pcm || !n_frames))))
    return invalid("null argument array");
  std::vector<Entry> es((size_t)n);
  bool work = false;
  for (int64_t i = 0; i < n; ++i) {
    bp_stream_state* s = streams[i];
    if (!s) return invalid("null stream");
    if (s->h != h) return invalid("a stream of another handle");
    if (s->broken) return invalid("a stream whose earlier call failed on the device: only bp_stream_close is valid");
    if (s->finished) return invalid("a finished stream: only bp_stream_close is valid");
    for (int64_t j = 0; j < i; ++j)
      if (streams[j] == s) return invalid("the same stream twice in one step");
    const int64_t n_in = finish_streams ? 0 : n_frames[i];
    if (n_in < 0 || (n_in > 0 && !pcm[i])) return invalid("negative n_frames or null pcm");
    const int64_t n_rows = rows_of_step(s, n_in, finish_streams);
    if (capacity_rows[i] < n_rows)
      return invalid("capacity_rows " + std::to_string(capacity_rows[i]) + " is too small for the " + std::to_string(n_rows) +
                     " rows of this step (bp_stream_rows_bound); nothing was taken from the stream");
    if (n_rows > 0 && (!note[i] || !onset[i] || !contour[i])) return invalid("null output pointer");
    if (mode == kPeek && !tail_fits(s)) {
      h->err = std::string(what) + ": the end of the resampled signal does not fit the stream's ring";
      return BP_ERR_UNSUPPORTED;
    }
    if (mode != kPeek && s->rows_out + n_rows > s->kept.limit) {
      h->err = std::string(what) + ": the " + std::to_string(n_rows) + " rows of this step would exceed the " +
               std::to_string(s->kept.limit) + " rows bp_stream_keep reserved; nothing was taken from the stream";
      return BP_ERR_OUT_OF_MEMORY;
    }
    es[(size_t)i] = plan_entry(s, mode, n_in, n_rows, {note[i], onset[i], contour[i]});
    work = work || n_in > 0 || mode == kFinish || n_rows > 0;
  }
  if (work) {
    BP_HIP(hipSetDevice(h->device));
    std::vector<WindowSeg> segs;  // read by an asynchronous copy: alive until the wait
    if (int rc = finish(h, queue_step(h, es, pcm, pcm_mem_kind, out_mem_kind, segs))) {
      for (auto& e : es) e.s->broken = true;
      return rc;
    }
  }
  for (int64_t i = 0; i < n; ++i) {
    const Entry& e = es[(size_t)i];
    bp_stream_state* s = e.s;
    rows[i] = e.rows;
    if (mode == kPeek) continue;
    if (s->resamples && e.n_frames > 0) s->cur_hist ^= 1;
    s->n_in += e.n_frames;
    s->n_res = e.n_res;
    s->w_next = e.w_next;
    s->rows_out += e.rows;
    s->finished = finish_streams;
  }
  return BP_OK;
}

}  // namespace

extern "C" {

int64_t bp_stream_rows_after(int64_t n_samples_22k, int finished) {
  if (finished) return bp_track_n_frames(n_samples_22k);
  return complete_windows(n_samples_22k, BP_AUDIO_N_SAMPLES, BP_HOP_SIZE, BP_OVERLAP_LEN / 2) * BP_FRAMES_PER_WINDOW;
}

int bp_stream_open(bp_handle h, int format, int channels, int sample_rate, bp_stream* out) {
  if (!h) return BP_ERR_INVALID_ARG;
  if (!out) {
    h->err = "bp_stream_open: null output";
    return BP_ERR_INVALID_ARG;
  }
  *out = nullptr;
  if (int rc = check_ingest(h, false, format, 0, channels, sample_rate, BP_MEM_HOST)) return rc;
  BP_HIP(hipSetDevice(h->device));
  std::unique_ptr<bp_stream_state> s(new bp_stream_state);
  s->h = h;
  s->format = format, s->channels = channels, s->sample_rate = sample_rate;
  s->resamples = sample_rate != h->rate;
  if (s->resamples) {
    if (int rc = stream_taps(h, s.get())) return rc;
    s->n_hist = (int)((s->plan.n_taps + s->plan.up - 1) / s->plan.up);
  }
  s->ring_cap = h->win_len + kRingHops * h->hop;
  BP_HIP(s->ring.reserve((size_t)s->ring_cap));
  if (s->n_hist > 0) {
    // both halves of the history in one block; zeros stand for the frames in front of the signal (never read: the sums are
    // clipped at frame 0)
    BP_HIP(s->hist.reserve((size_t)s->n_hist * 2));
    BP_HIP(hipMemset(s->hist, 0, (size_t)s->n_hist * 2 * sizeof(float)));
  }
  *out = s.release();
  return BP_OK;
}

void bp_stream_close(bp_stream s) {
  if (!s) return;
  // no call returns with work of the stream still queued (finish), so its buffers are idle
  (void)hipSetDevice(s->h->device);
  delete s;
}

int64_t bp_stream_state_bytes(bp_stream s) { return s ? ((int64_t)s->ring_cap + 2 * (int64_t)s->n_hist) * 4 + kept_bytes(s) : 0; }

int64_t bp_stream_rows_bound(bp_stream s, int64_t n_frames) {
  if (!s || s->finished || n_frames < 0) return 0;
  return std::max(rows_of_step(s, n_frames, false), rows_of_step(s, 0, true));
}

int bp_stream_push(bp_stream s, const void* pcm, int64_t n_frames, int pcm_mem_kind, float* note, float* onset, float* contour,
                   int64_t capacity_rows, int out_mem_kind, int64_t* rows) {
  if (!s) return BP_ERR_INVALID_ARG;
  return step(s->h, "bp_stream_push", 1, &s, &pcm, &n_frames, pcm_mem_kind, &note, &onset, &contour, &capacity_rows, out_mem_kind,
              rows, kPush);
}

int bp_stream_finish(bp_stream s, float* note, float* onset, float* contour, int64_t capacity_rows, int out_mem_kind,
                     int64_t* rows) {
  if (!s) return BP_ERR_INVALID_ARG;
  return step(s->h, "bp_stream_finish", 1, &s, nullptr, nullptr, BP_MEM_HOST, &note, &onset, &contour, &capacity_rows,
              out_mem_kind, rows, kFinish);
}

int bp_stream_peek(bp_stream s, float* note, float* onset, float* contour, int64_t capacity_rows, int out_mem_kind, int64_t* rows) {
  if (!s) return BP_ERR_INVALID_ARG;
  return step(s->h, "bp_stream_peek", 1, &s, nullptr, nullptr, BP_MEM_HOST, &note, &onset, &contour, &capacity_rows, out_mem_kind,
              rows, kPeek);
}

int bp_streams_peek(bp_handle h, int64_t n, const bp_stream* streams, float* const* note, float* const* onset,
                    float* const* contour, const int64_t* capacity_rows, int out_mem_kind, int64_t* rows) {
  if (!h) return BP_ERR_INVALID_ARG;
  return step(h, "bp_streams_peek", n, streams, nullptr, nullptr, BP_MEM_HOST, note, onset, contour, capacity_rows, out_mem_kind,
              rows, kPeek);
}

int bp_streams_push(bp_handle h, int64_t n, const bp_stream* streams, const void* const* pcm, const int64_t* n_frames,
                    int pcm_mem_kind, float* const* note, float* const* onset, float* const* contour,
                    const int64_t* capacity_rows, int out_mem_kind, int64_t* rows) {
  if (!h) return BP_ERR_INVALID_ARG;
  return step(h, "bp_streams_push", n, streams, pcm, n_frames, pcm_mem_kind, note, onset, contour, capacity_rows, out_mem_kind,
              rows, kPush);
}

// bp_stream_keep and bp_stream_keep_rolling after the checks of their own argument: from now on the stream retains its maps
// in a ring of `rows` rows and a tail's room.  table: `rows` is a rolling horizon.  No table: they are all the final rows the
// stream may emit, and the horizon is the whole ring — the first row of a slice stays 0.
static int keep_rows(bp_stream s, const char* what, const bp_note_params* params, int64_t rows, bool table) {
  bp_handle h = s->h;
  auto invalid = [&](const char* why) {
    h->err = std::string(what) + ": " + why;
    return BP_ERR_INVALID_ARG;
  };
  auto& k = s->kept;
  if (s->broken || s->finished) return invalid("a finished or broken stream");
  if (k.cap && !k.table)
    return invalid(table ? "the stream keeps all its maps already (bp_stream_keep): one or the other"
                         : "the stream keeps its maps already (the decoding parameters are fixed by the first call)");
  if (k.cap)
    return invalid(table ? "the stream keeps a rolling horizon already (the parameters are fixed by the first call)"
                         : "the stream keeps a rolling horizon already (bp_stream_keep_rolling): one or the other");
  if (s->rows_out > 0) return invalid("rows have left the stream already: call it before the first window completes");
  BP_HIP(hipSetDevice(h->device));
  if (int rc = note_tables(h, nullptr, nullptr)) return rc;
  const int64_t cap = rows + kTailRows;
  if (!table && cap > (int64_t)1 << 40) return invalid("max_rows is out of range");
  // The record that final rows join starts with the initial values; a block table starts empty: a block is written anew by
  // the step that emits its first row.  A setup that fails frees what it reserved.
  DeviceBuffer<float> maps, rec;
  BP_HIP(maps.reserve((size_t)(cap * kMapsRow)));
  BP_HIP(rec.reserve((size_t)((table ? note_ring_records(cap) : 2) * kStatsFloats)));
  if (!table) {
    launch_note_stats_init(rec, h->stream);
    if (int rc = finish(h, hipGetLastError() == hipSuccess ? BP_OK : BP_ERR_HIP)) return rc;
  }
  k.rows = std::move(maps), k.rec = std::move(rec);
  k.cap = cap, k.horizon = table ? rows : cap, k.table = table;
  if (!table) k.limit = rows;
  s->prm = *params;
  bp_internal_freq_limits(params, &s->lo, &s->hi);
  return BP_OK;
}

int bp_stream_keep(bp_stream s, const bp_note_params* params, int64_t max_rows) {
  if (!s) return BP_ERR_INVALID_ARG;
  if (!params || max_rows <= 0) {
    s->h->err = "bp_stream_keep: null params or a max_rows that is not positive";
    return BP_ERR_INVALID_ARG;
  }
  return keep_rows(s, "bp_stream_keep", params, max_rows, false);
}

// the arguments of the calls that read a stream's retained rows (table: those of a rolling horizon), before anything is
// queued; *tail_rows: the rows of the peek.  A finished stream has no tail: its final rows are the whole track.  Whether the
// tail fits is tail_refused's verdict, which each call applies where it always has among its own checks.
static int check_kept(bp_stream s, const char* what, bool table, int with_tail, int64_t* tail_rows) {
  bp_handle h = s->h;
  auto invalid = [&](const char* why) {
    h->err = std::string(what) + ": " + why;
    return BP_ERR_INVALID_ARG;
  };
  if (!s->kept.cap || s->kept.table != table)
    return invalid(table ? "the stream keeps no rolling horizon (bp_stream_keep_rolling)" : "the stream does not keep its maps (bp_stream_keep)");
  if (s->broken) return invalid("a stream whose earlier call failed on the device: only bp_stream_close is valid");
  *tail_rows = with_tail && !s->finished ? rows_of_step(s, 0, true) : 0;
  return BP_OK;
}

static int tail_refused(bp_stream s, const char* what, bool table, int64_t tail_rows) {
  if (tail_rows <= kTailRows && (tail_rows == 0 || tail_fits(s))) return BP_OK;
  s->h->err = std::string(what) + ": the end of the signal does not fit the stream's ring or the room behind the " +
              (table ? "final" : "kept") + " rows";
  return BP_ERR_UNSUPPORTED;
}

// bp_stream_candidates and bp_stream_candidates_rolling: an update into host rings of ring_rows rows of which the caller
// holds the rows before `held`, an argument the caller knows as `held_name`
static int candidates(bp_stream s, const char* what, bool table, int with_tail, float* note_ring, uint8_t* bits_ring,
                      int8_t* bend_ring, int64_t ring_rows, int64_t held, const char* held_name, int64_t* first_row,
                      int64_t* n_rows, int* status) {
  bp_handle h = s->h;
  auto invalid = [&](const std::string& why) {
    h->err = std::string(what) + ": " + why;
    return BP_ERR_INVALID_ARG;
  };
  // every argument, before anything is queued
  int64_t tail_rows = 0;
  if (int rc = check_kept(s, what, table, with_tail, &tail_rows)) return rc;
  if (int rc = table ? tail_refused(s, what, table, tail_rows) : BP_OK) return rc;
  const int64_t T = s->rows_out + tail_rows;
  if (table && ring_rows < s->kept.cap)
    return invalid("ring_rows " + std::to_string(ring_rows) + " is less than the " + std::to_string(s->kept.cap) +
                   " rows of the stream's ring (horizon_rows + 284)");
  if (held < 0 || held > s->rows_out)
    return invalid(std::string(held_name) + " " + std::to_string(held) + " is not in 0 ... " + std::to_string(s->rows_out) +
                   ", the final rows");
  if (!table && ring_rows < T)
    return invalid("capacity_rows " + std::to_string(ring_rows) + " is too small for the " + std::to_string(T) + " rows");
  if (T > 0 && (!note_ring || !bits_ring)) return invalid("null output pointer");
  if (int rc = table ? BP_OK : tail_refused(s, what, table, tail_rows)) return rc;
  const int64_t a = bp_stream_horizon_first_row(T, s->kept.horizon);
  *first_row = a;
  *n_rows = T;
  *status = s->prm.onset_threshold > 0.0 ? 0 : 1;
  if (T == 0) return BP_OK;
  BP_HIP(hipSetDevice(h->device));
  // the step of one stream, then from its packed results into the rings: the bitmap of the whole slice, the note rows the
  // caller does not hold yet, their bends
  bp_stream_update u{};
  u.stream = s, u.held_rows = held;
  u.first_row = a, u.n_rows = T, u.new_row = std::max(held, a);
  const std::vector<int64_t> tail{tail_rows};
  std::vector<WindowSeg> segs;  // both read by asynchronous copies: alive until the wait
  std::vector<uint8_t> tab;
  const bool want_bends = s->prm.include_pitch_bends != 0 && bend_ring != nullptr;
  auto queue = [&]() -> int {
    if (int rc = queue_updates(h, 1, &u, tail, T - u.new_row, T - a, segs, tab, UpdateResults::for_host_rings(bend_ring != nullptr)))
      return rc;
    if (int rc = copy_to_host_ring(h, bits_ring, ring_rows, h->up_bits, BP_NOTE_CAND_ROW_BYTES, a, T)) return rc;
    if (int rc = copy_to_host_ring(h, note_ring, ring_rows, h->up_note, kFreqN * 4, u.new_row, T)) return rc;
    return want_bends ? copy_to_host_ring(h, bend_ring, ring_rows, h->up_bend, kFreqN, u.new_row, T) : BP_OK;
  };
  if (int rc = finish(h, queue())) {
    s->broken = true;
    return rc;
  }
  if (h->up_stats_host[1]) *status = 1;  // a NaN in the slice: the host decodes the maps themselves
  return BP_OK;
}

// the caller's linear arrays of capacity_rows rows are host rings that never wrap: the slice starts at row 0
int bp_stream_candidates(bp_stream s, int with_tail, float* note_out, uint8_t* cand_bits, int8_t* bend_map, int64_t first_row,
                         int64_t capacity_rows, int64_t* n_rows, int* status) {
  if (!s) return BP_ERR_INVALID_ARG;
  if (!n_rows || !status) {
    s->h->err = "bp_stream_candidates: null n_rows / status";
    return BP_ERR_INVALID_ARG;
  }
  int64_t a = 0;
  return candidates(s, "bp_stream_candidates", false, with_tail, note_out, cand_bits, bend_map, capacity_rows, first_row, "first_row",
                    &a, n_rows, status);
}

int64_t bp_stream_horizon_first_row(int64_t n_rows, int64_t horizon_rows) {
  return n_rows > horizon_rows ? n_rows - horizon_rows : 0;
}

int bp_stream_keep_rolling(bp_stream s, const bp_note_params* params, int64_t horizon_rows) {
  if (!s) return BP_ERR_INVALID_ARG;
  const char* why = !params ? "null params"
                    : horizon_rows < 3 || horizon_rows > (int64_t)1 << 40
                        ? "horizon_rows is out of range (at least 3: a peak needs a row on either side)"
                        : nullptr;
  if (why) {
    s->h->err = std::string("bp_stream_keep_rolling: ") + why;
    return BP_ERR_INVALID_ARG;
  }
  return keep_rows(s, "bp_stream_keep_rolling", params, horizon_rows, true);
}

int bp_stream_candidates_rolling(bp_stream s, int with_tail, float* note_ring, uint8_t* bits_ring, int8_t* bend_ring,
                                 int64_t ring_rows, int64_t held_rows, int64_t* first_row, int64_t* n_rows, int* status) {
  if (!s) return BP_ERR_INVALID_ARG;
  if (!first_row || !n_rows || !status) {
    s->h->err = "bp_stream_candidates_rolling: null first_row / n_rows / status";
    return BP_ERR_INVALID_ARG;
  }
  return candidates(s, "bp_stream_candidates_rolling", true, with_tail, note_ring, bits_ring, bend_ring, ring_rows, held_rows,
                    "held_rows", first_row, n_rows, status);
}

int bp_stream_rolling_maps(bp_stream s, int with_tail, float* note, float* onset, float* contour, int64_t capacity_rows,
                           int64_t* first_row, int64_t* n_rows) {
  if (!s) return BP_ERR_INVALID_ARG;
  bp_handle h = s->h;
  auto invalid = [&](const std::string& why) {
    h->err = "bp_stream_rolling_maps: " + why;
    return BP_ERR_INVALID_ARG;
  };
  if (!first_row || !n_rows) return invalid("null first_row / n_rows");
  int64_t tail_rows = 0;
  if (int rc = check_kept(s, "bp_stream_rolling_maps", true, with_tail, &tail_rows)) return rc;
  if (int rc = tail_refused(s, "bp_stream_rolling_maps", true, tail_rows)) return rc;
  const int64_t T = s->rows_out + tail_rows, a = bp_stream_horizon_first_row(T, s->kept.horizon);
  if (capacity_rows < T - a)
    return invalid("capacity_rows " + std::to_string(capacity_rows) + " is too small for the " + std::to_string(T - a) + " rows");
  if (T > a && (!note || !onset || !contour)) return invalid("null output pointer");
  *first_row = a;
  *n_rows = T;
  if (T == 0) return BP_OK;
  BP_HIP(hipSetDevice(h->device));
  std::vector<WindowSeg> segs;  // read by an asynchronous copy: alive until the wait
  if (int rc = finish(h, queue_rolling_maps(h, s, tail_rows, Maps{note, onset, contour}, segs))) {
    s->broken = true;
    return rc;
  }
  return BP_OK;
}

// ---- the updates of n streams in one step (include/basic_pitch_amd_update.h) -------------------------------------------------
// every per-stream argument, in index order, and the out fields but status; tail[i]: the rows of stream i's peek.  for_events:
// the host decoder's rules for the stream's kept parameters and its absolute frames as well (bp_streams_events).
static int plan_updates(bp_handle h, const char* what, int64_t n, bp_stream_update* u, int with_tail, std::vector<int64_t>& tail,
                        int64_t* note_rows, int64_t* bits_rows, bool for_events = false) {
  auto invalid = [&](const std::string& why) {
    h->err = std::string(what) + ": " + why;
    return BP_ERR_INVALID_ARG;
  };
  if (n < 0 || (n > 0 && !u)) return invalid("negative count or null array of updates");
  tail.assign((size_t)n, 0);
  *note_rows = *bits_rows = 0;
  for (int64_t i = 0; i < n; ++i) {
    bp_stream_state* s = u[i].stream;
    const std::string at = "stream " + std::to_string(i) + ": ";
    if (!s) return invalid(at + "null stream");
    if (s->h != h) return invalid(at + "a stream of another handle");
    for (int64_t j = 0; j < i; ++j)
      if (u[j].stream == s) return invalid(at + "the same stream twice in one step (also stream " + std::to_string(j) + ")");
    if (!s->kept.cap) return invalid(at + "the stream retains nothing (bp_stream_keep or bp_stream_keep_rolling)");
    if (s->broken) return invalid(at + "a stream whose earlier call failed on the device: only bp_stream_close is valid");
    if (u[i].held_rows < 0 || u[i].held_rows > s->rows_out)
      return invalid(at + "held_rows " + std::to_string(u[i].held_rows) + " is not in 0 ... " + std::to_string(s->rows_out) +
                     ", the final rows");
    tail[(size_t)i] = with_tail && !s->finished ? rows_of_step(s, 0, true) : 0;
    const std::string who = std::string(what) + ": stream " + std::to_string(i);
    if (int rc = tail_refused(s, who.c_str(), s->kept.table, tail[(size_t)i])) return rc;
    if (!for_events) continue;
    if (s->prm.melodia_trick && s->prm.frame_threshold < 0.0)
      return invalid(at + "a negative frame threshold with the melodia trick never terminates (note_creation.py:452)");
    if (s->prm.min_note_len < 0) return invalid(at + "negative min_note_len");
    if (s->rows_out + tail[(size_t)i] > INT32_MAX) return invalid(at + "the absolute frames pass INT32_MAX");
  }
  for (int64_t i = 0; i < n; ++i) {
    const bp_stream_state* s = u[i].stream;
    const int64_t T = s->rows_out + tail[(size_t)i], a = bp_stream_horizon_first_row(T, s->kept.horizon);
    u[i].first_row = a, u[i].n_rows = T, u[i].new_row = std::max(u[i].held_rows, a);
    u[i].note_offset = *note_rows, u[i].bits_offset = *bits_rows;
    *note_rows += T - u[i].new_row, *bits_rows += T - a;
  }
  return BP_OK;
}

int bp_streams_update_layout(bp_handle h, int64_t n, bp_stream_update* u, int with_tail, int64_t* note_rows, int64_t* bits_rows) {
  if (!h) return BP_ERR_INVALID_ARG;
  if (!note_rows || !bits_rows) {
    h->err = "bp_streams_update_layout: null note_rows / bits_rows";
    return BP_ERR_INVALID_ARG;
  }
  std::vector<int64_t> tail;
  return plan_updates(h, "bp_streams_update_layout", n, u, with_tail, tail, note_rows, bits_rows);
}

int bp_streams_candidates(bp_handle h, int64_t n, bp_stream_update* u, int with_tail, float* note_out, int8_t* bend_out,
                          uint8_t* bits_out, int64_t note_capacity_rows, int64_t bits_capacity_rows) {
  if (!h) return BP_ERR_INVALID_ARG;
  const char* what = "bp_streams_candidates";
  auto invalid = [&](const std::string& why) {
    h->err = std::string(what) + ": " + why;
    return BP_ERR_INVALID_ARG;
  };
  std::vector<int64_t> tail;
  int64_t note_rows = 0, bits_rows = 0;
  if (int rc = plan_updates(h, what, n, u, with_tail, tail, &note_rows, &bits_rows)) return rc;
  if (note_capacity_rows < note_rows || bits_capacity_rows < bits_rows)
    return invalid("note_capacity_rows " + std::to_string(note_capacity_rows) + " / bits_capacity_rows " +
                   std::to_string(bits_capacity_rows) + " are too small for the " + std::to_string(note_rows) + " / " +
                   std::to_string(bits_rows) + " rows of this update (bp_streams_update_layout)");
  if ((note_rows > 0 && !note_out) || (bits_rows > 0 && !bits_out)) return invalid("null output pointer");
  for (int64_t i = 0; i < n; ++i) u[i].status = u[i].stream->prm.onset_threshold > 0.0 ? 0 : 1;
  if (bits_rows == 0) return BP_OK;  // no stream has a row yet
  BP_HIP(hipSetDevice(h->device));
  std::vector<WindowSeg> segs;  // both read by asynchronous copies: alive until the wait
  std::vector<uint8_t> tab;
  if (int rc = finish(h, queue_updates(h, n, u, tail, note_rows, bits_rows, segs, tab, UpdateResults::packed_home(note_out, bend_out, bits_out)))) {
    for (int64_t i = 0; i < n; ++i) u[i].stream->broken = true;
    return rc;
  }
  for (int64_t i = 0; i < n; ++i)
    if (h->up_stats_host[i * kStatsFloats + 1]) u[i].status = 1;  // a NaN in the slice: the host decodes the maps themselves
  return BP_OK;
}

// ---- the note events of n streams from the device (include/basic_pitch_amd_stream_events.h) ---------------------------------
// plan_updates with held_rows = 0 for every stream (new_row = first_row: the whole slice is gathered), the out fields but status,
// the tracker's segment of every stream and the capacities of the regions
static int plan_events(bp_handle h, const char* what, int64_t n, bp_stream_events* u, int with_tail, std::vector<bp_stream_update>& up,
                       std::vector<int64_t>& tail, std::vector<NoteTrackSeg>& seg, int64_t* rows, int64_t* events_capacity,
                       int64_t* bends_capacity) {
  if (n < 0 || (n > 0 && !u)) {
    h->err = std::string(what) + ": negative count or null array of streams";
    return BP_ERR_INVALID_ARG;
  }
  up.assign((size_t)n, bp_stream_update{});
  for (int64_t i = 0; i < n; ++i) up[(size_t)i].stream = u[i].stream;
  int64_t note_rows = 0;
  if (int rc = plan_updates(h, what, n, up.data(), with_tail, tail, &note_rows, rows, true)) return rc;
  seg.assign((size_t)n, NoteTrackSeg{});
  *events_capacity = *bends_capacity = 0;
  for (int64_t i = 0; i < n; ++i) {
    const bp_note_params& p = u[i].stream->prm;
    const int64_t slice = up[(size_t)i].n_rows - up[(size_t)i].first_row;
    u[i].first_row = up[(size_t)i].first_row, u[i].n_rows = up[(size_t)i].n_rows;
    seg[(size_t)i] = NoteTrackSeg{p.frame_threshold, p.energy_tol, p.min_note_len, p.melodia_trick != 0, p.include_pitch_bends != 0,
                                  !(p.onset_threshold > 0.0), 0};
    *events_capacity += note_track_capacity(slice, p.min_note_len);
    if (p.include_pitch_bends && slice <= kNoteTrackMaxRows) *bends_capacity += slice * kFreqN;
  }
  return BP_OK;
}

int bp_streams_events_layout(bp_handle h, int64_t n, bp_stream_events* u, int with_tail, int64_t* events_capacity,
                             int64_t* bends_capacity) {
  if (!h) return BP_ERR_INVALID_ARG;
  if (!events_capacity || !bends_capacity) {
    h->err = "bp_streams_events_layout: null events_capacity / bends_capacity";
    return BP_ERR_INVALID_ARG;
  }
  std::vector<bp_stream_update> up;
  std::vector<int64_t> tail;
  std::vector<NoteTrackSeg> seg;
  int64_t rows = 0;
  return plan_events(h, "bp_streams_events_layout", n, u, with_tail, up, tail, seg, &rows, events_capacity, bends_capacity);
}

int bp_streams_events(bp_handle h, int64_t n, bp_stream_events* u, int with_tail, bp_note_event* events, int64_t max_events,
                      int32_t* bends, int64_t max_bends, int64_t* event_offsets) {
  if (!h) return BP_ERR_INVALID_ARG;
  const char* what = "bp_streams_events";
  const EventsSink out{events, max_events, bends, max_bends, event_offsets, nullptr};
  auto invalid = [&](const char* why) {
    h->err = std::string(what) + ": " + why;
    return BP_ERR_INVALID_ARG;
  };
  std::vector<bp_stream_update> up;
  std::vector<int64_t> tail;
  std::vector<NoteTrackSeg> seg;
  int64_t rows = 0, cap_e = 0, cap_b = 0;
  if (int rc = plan_events(h, what, n, u, with_tail, up, tail, seg, &rows, &cap_e, &cap_b)) return rc;
  if (!out.event_offsets) return invalid("null event_offsets");
  if (out.max_events < 0 || out.max_bends < 0 || (out.max_events > 0 && !out.events) || (out.max_bends > 0 && !out.bends))
    return invalid("negative max_events / max_bends, or room without a buffer");
  bool work = false;
  std::vector<int64_t> offs((size_t)n + 1, 0), first((size_t)n, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t slice = u[i].n_rows - u[i].first_row;
    u[i].status = seg[(size_t)i].skip ? 1 : 0;
    offs[(size_t)i + 1] = offs[(size_t)i] + slice;
    first[(size_t)i] = u[i].first_row;
    work = work || (slice > 0 && !seg[(size_t)i].skip);
  }
  for (int64_t i = 0; i <= n; ++i) out.event_offsets[i] = 0;
  if (!work) return BP_OK;  // no stream has a row yet, or none that the device decodes
  BP_HIP(hipSetDevice(h->device));
  const EventsJob job{what, "n", n, offs.data(), nullptr, seg.data(), first.data(), kNoteTrackFormAuto};
  EventsPlan plan;
  std::vector<WindowSeg> segs;  // both read by asynchronous copies: alive until the wait
  std::vector<uint8_t> tab;
  auto broken = [&](int rc) {
    for (int64_t i = 0; i < n; ++i) u[i].stream->broken = true;
    return rc;
  };
  auto queue = [&]() -> int {
    if (int rc = events_reserve(h, job, &plan)) return rc;
    if (int rc = queue_updates(h, n, up.data(), tail, rows, rows, segs, tab, UpdateResults::for_tracker())) return rc;
    // the rows before each stream's slice: the table's prefix array of the note rows (new_row = first_row)
    const int64_t* d_pre = reinterpret_cast<const int64_t*>(h->up_tab + (size_t)n * sizeof(StreamUpdate));
    return events_queue(h, job, plan,
                        TrackInputs{h->up_note, h->up_bits, h->up_bend, d_pre + (kStreamUpdatePrefixes - 1) * (n + 1), h->up_stats});
  };
  if (int rc = finish(h, queue())) return broken(rc);
  std::vector<int> status((size_t)n, 0);
  bool device_error = false;
  const EventsSink sink{out.events, out.max_events, out.bends, out.max_bends, out.event_offsets, status.data()};
  const int rc = events_home(h, job, sink, &device_error);
  for (int64_t i = 0; i < n; ++i) u[i].status = seg[(size_t)i].skip ? 1 : status[(size_t)i];
  return device_error ? broken(rc) : rc;
}

#ifdef BP_AB_KERNELS
// The A/B library's test hook for the NaN path of a stream that retains its maps (declared nowhere: the tests name it).  From
// now on the cell (map: 0 note, 1 onset; absolute row; bin) of the RETAINED copy is a NaN whenever its row is written there
// (put_rows) — as a row of a tail at an update, as a final row at the step that emits it.  The rows handed to the caller are
// not touched.
int bp_ab_stream_poison(bp_stream s, int map, int64_t row, int bin) {
  if (!s || !s->kept.cap || map < 0 || map > 1 || row < 0 || bin < 0 || bin >= kFreqN) return BP_ERR_INVALID_ARG;
  s->ab_nan_map = map, s->ab_nan_row = row, s->ab_nan_bin = bin;
  return BP_OK;
}
#endif

}  // extern "C"
