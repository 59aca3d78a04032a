// C ABI of the streaming sessions (include/basic_pitch_amd.h): audio that arrives over time -> the rows of the un-overlapped
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
#include <algorithm>
#include <cstring>

#include "bp_context.h"

using namespace bp;

struct bp_stream_state {
  bp_handle h = nullptr;
  int format = 0, channels = 0, sample_rate = 0;
  bool resamples = false;  // false: the input is at the handle's rate and is only converted and downmixed
  ResamplePlan plan{};
  const double* taps = nullptr;  // the handle's table for this rate
  int n_hist = 0;                // ceil(n_taps / up) frames; 0 without resampling
  int ring_cap = 0;
  float* ring = nullptr;
  float* hist[2] = {nullptr, nullptr};
  int cur_hist = 0;
  int64_t n_in = 0;      // input frames taken
  int64_t n_res = 0;     // samples of the model-rate signal made
  int64_t w_next = 0;    // first window that has not run
  int64_t rows_out = 0;  // rows emitted
  bool finished = false, broken = false;
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
  double* dev = nullptr;
  if (int rc = upload_filter(h, s->sample_rate, true, &pl, &dev)) {
    if (rc == BP_ERR_UNSUPPORTED)
      h->err = "bp_stream_open: " + std::to_string(s->sample_rate) + " Hz -> " + std::to_string(h->rate) +
               " Hz needs a filter of " + std::to_string(pl.n_taps) +
               " taps, which the one-shot calls evaluate in the kernel; such ratios are not streamed";
    return rc;
  }
  h->st_taps.push_back({s->sample_rate, dev, pl});
  s->plan = pl;
  s->taps = dev;
  return BP_OK;
}

void free_stream(bp_stream_state* s) {
  if (s->ring) (void)hipFree(s->ring);
  if (s->hist[0]) (void)hipFree(s->hist[0]);
  delete s;
}

// ---- one step of n streams ------------------------------------------------------------------------------------------------
struct Entry {
  bp_stream_state* s;
  const uint8_t* pcm;  // the chunk where the kernels read it (device)
  int64_t n_frames;
  bool finish;
  Maps out;            // the rows of this call where the kernels write them (device)
  Maps user;
  int64_t rows;
  const float* mono;   // the chunk's mono form (resampling streams)
  // the plan's copy of the counters
  int64_t n_res, w_next, n_total;
};

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
  // scratch of the step, grown before anything is queued: the chunks (host PCM), their mono form, the rows (host outputs)
  int64_t pcm_floats = 0, mono_floats = 0, out_floats = 0;
  for (auto& e : es) {
    const int64_t bytes = e.n_frames * e.s->channels * pcm_width(e.s->format);
    if (pcm_mem_kind == BP_MEM_HOST) pcm_floats += (bytes + 15) / 16 * 4;
    if (e.s->resamples) mono_floats += (e.n_frames + 3) / 4 * 4;
    if (out_mem_kind == BP_MEM_HOST) out_floats += e.rows * kMapsRow;
  }
  int rc;
  if ((rc = grow(h, &h->st_pcm, &h->st_pcm_cap, pcm_floats)) || (rc = grow(h, &h->st_mono, &h->st_mono_cap, mono_floats)) ||
      (rc = grow(h, &h->st_out, &h->st_out_cap, out_floats)))
    return rc;
  int64_t pcm_at = 0, mono_at = 0, out_at = 0;
  for (size_t i = 0; i < es.size(); ++i) {
    Entry& e = es[i];
    const int64_t bytes = e.n_frames * e.s->channels * pcm_width(e.s->format);
    e.pcm = static_cast<const uint8_t*>(pcm ? pcm[i] : nullptr);
    if (pcm_mem_kind == BP_MEM_HOST) {
      e.pcm = reinterpret_cast<const uint8_t*>(h->st_pcm + pcm_at);
      pcm_at += (bytes + 15) / 16 * 4;
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
      launch_stream_downmix(e.pcm, s->format, e.n_frames, s->channels, const_cast<float*>(e.mono), 0, 0, s->hist[s->cur_hist],
                            s->hist[s->cur_hist ^ 1], s->n_hist, q);
  }
  if (!segs.empty()) {
    const int64_t floats = (int64_t)(segs.size() * sizeof(WindowSeg) + 3) / 4;
    if ((rc = grow(h, &h->st_segs, &h->st_segs_cap, floats))) return rc;
    BP_HIP(hipMemcpyAsync(h->st_segs, segs.data(), segs.size() * sizeof(WindowSeg), hipMemcpyHostToDevice, q));
  }
  const WindowSeg* d_segs = reinterpret_cast<const WindowSeg*>(h->st_segs);
  for (const Round& r : rounds) {
    for (const Ingest& g : r.ingests) {
      const Entry& e = es[g.e];
      bp_stream_state* s = e.s;
      const int pos = (int)(g.k0 % s->ring_cap);
      if (s->resamples)
        launch_stream_resample(s->hist[s->cur_hist], s->n_hist, e.mono, s->n_in, s->n_in + e.n_frames, s->taps, s->plan, g.k0,
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
  for (const Entry& e : es)
    if (out_mem_kind == BP_MEM_HOST && e.rows > 0 && (rc = copy_maps(h, e.user, e.out, e.rows, hipMemcpyDeviceToHost))) return rc;
  return BP_OK;
}

// validate everything -> queue -> wait -> the streams' counters.  pcm / n_frames: NULL for finish.
int step(bp_handle h, const char* what, int64_t n, const bp_stream* streams, const void* const* pcm, const int64_t* n_frames,
         int pcm_mem_kind, float* const* note, float* const* onset, float* const* contour, const int64_t* capacity_rows,
         int out_mem_kind, int64_t* rows, bool finish_streams) {
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
    Entry& e = es[(size_t)i];
    e = Entry{};
    e.s = s;
    e.finish = finish_streams;
    e.n_frames = finish_streams ? 0 : n_frames[i];
    if (e.n_frames < 0 || (e.n_frames > 0 && !pcm[i])) return invalid("negative n_frames or null pcm");
    e.rows = rows_of_step(s, e.n_frames, finish_streams);
    if (capacity_rows[i] < e.rows)
      return invalid("capacity_rows " + std::to_string(capacity_rows[i]) + " is too small for the " + std::to_string(e.rows) +
                     " rows of this step (bp_stream_rows_bound); nothing was taken from the stream");
    if (e.rows > 0 && (!note[i] || !onset[i] || !contour[i])) return invalid("null output pointer");
    e.user = {note[i], onset[i], contour[i]};
    e.n_res = s->n_res;
    e.w_next = s->w_next;
    e.n_total = finish_streams ? bp_handle_resampled_length(h, s->n_in, s->sample_rate) : -1;
    work = work || e.n_frames > 0 || finish_streams;
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
    if (s->resamples && e.n_frames > 0) s->cur_hist ^= 1;
    s->n_in += e.n_frames;
    s->n_res = e.n_res;
    s->w_next = e.w_next;
    s->rows_out += e.rows;
    s->finished = finish_streams;
    rows[i] = e.rows;
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
  bp_stream_state* s = new bp_stream_state;
  s->h = h;
  s->format = format, s->channels = channels, s->sample_rate = sample_rate;
  s->resamples = sample_rate != h->rate;
  if (s->resamples) {
    if (int rc = stream_taps(h, s)) {
      delete s;
      return rc;
    }
    s->n_hist = (int)((s->plan.n_taps + s->plan.up - 1) / s->plan.up);
  }
  s->ring_cap = h->win_len + kRingHops * h->hop;
  hipError_t e = hipMalloc(&s->ring, (size_t)s->ring_cap * 4);
  if (e == hipSuccess && s->n_hist > 0) {
    // both halves of the history in one block; zeros stand for the frames in front of the signal (never read: the sums are
    // clipped at frame 0)
    e = hipMalloc(&s->hist[0], (size_t)s->n_hist * 2 * 4);
    if (e == hipSuccess) e = hipMemset(s->hist[0], 0, (size_t)s->n_hist * 2 * 4);
    s->hist[1] = s->hist[0] ? s->hist[0] + s->n_hist : nullptr;
  }
  if (e != hipSuccess) {
    free_stream(s);
    BP_HIP(e);
  }
  *out = s;
  return BP_OK;
}

void bp_stream_close(bp_stream s) {
  if (!s) return;
  // no call returns with work of the stream still queued (finish), so its buffers are idle
  (void)hipSetDevice(s->h->device);
  free_stream(s);
}

int64_t bp_stream_state_bytes(bp_stream s) { return s ? ((int64_t)s->ring_cap + 2 * (int64_t)s->n_hist) * 4 : 0; }

int64_t bp_stream_rows_bound(bp_stream s, int64_t n_frames) {
  if (!s || s->finished || n_frames < 0) return 0;
  return std::max(rows_of_step(s, n_frames, false), rows_of_step(s, 0, true));
}

int bp_stream_push(bp_stream s, const void* pcm, int64_t n_frames, int pcm_mem_kind, float* note, float* onset, float* contour,
                   int64_t capacity_rows, int out_mem_kind, int64_t* rows) {
  if (!s) return BP_ERR_INVALID_ARG;
  return step(s->h, "bp_stream_push", 1, &s, &pcm, &n_frames, pcm_mem_kind, &note, &onset, &contour, &capacity_rows, out_mem_kind,
              rows, false);
}

int bp_stream_finish(bp_stream s, float* note, float* onset, float* contour, int64_t capacity_rows, int out_mem_kind,
                     int64_t* rows) {
  if (!s) return BP_ERR_INVALID_ARG;
  return step(s->h, "bp_stream_finish", 1, &s, nullptr, nullptr, BP_MEM_HOST, &note, &onset, &contour, &capacity_rows,
              out_mem_kind, rows, true);
}

int bp_streams_push(bp_handle h, int64_t n, const bp_stream* streams, const void* const* pcm, const int64_t* n_frames,
                    int pcm_mem_kind, float* const* note, float* const* onset, float* const* contour,
                    const int64_t* capacity_rows, int out_mem_kind, int64_t* rows) {
  if (!h) return BP_ERR_INVALID_ARG;
  return step(h, "bp_streams_push", n, streams, pcm, n_frames, pcm_mem_kind, note, onset, contour, capacity_rows, out_mem_kind,
              rows, false);
}

}  // extern "C"
