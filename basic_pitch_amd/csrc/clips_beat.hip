// Tempo and beats of every segment of a job, of the onset rows alone (include/basic_pitch_amd_beat.h, beat.hip):
// the sink behind run_clips (clips_job.h) and its entry points.  Host code only.
#include <algorithm>
#include <cstring>

#include "../../include/basic_pitch_amd_beat.h"
#include "clips_job.h"

using namespace bp;

extern "C" const char* bp_internal_beat_bad_params(const bp_beat_params* p);  // beat_host.cpp

namespace {

// A summary per segment under `params`, the beats as one compact array (room for max_beats) with beat_offsets [n + 1].
struct BeatSink final : JobSink {
  struct Args {
    const bp_beat_params* params;
    bp_beat_summary* summaries;
    int32_t* beats;
    int64_t max_beats;
    int64_t* beat_offsets;
  } a;
  std::vector<BeatSeg> segs;  // the segments with rows, and what they take of the launches and of the beat pool
  int64_t blocks = 0, tiles = 0, cap = 0;
  explicit BeatSink(const Args& args) : a(args) {}

  // the onset rows alone, read where they lie unless they are in host memory or not 16-byte aligned
  MapsUse use(bp_handle h) const override { return MapsUse{false, true, false, true, false, nullptr, &h->bt_onset, nullptr}; }

  int check(bp_handle h, const char* what, int64_t n_segs) override {
    auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
    if (n_segs < 0 || (n_segs > 0 && (!a.summaries || !a.beat_offsets))) return invalid("negative n_segments / n_clips, or null summaries or beat_offsets");
    if (const char* why = bp_internal_beat_bad_params(a.params)) return invalid(std::string("params: ") + why);
    if (!check_room(a.max_beats, a.beats)) return invalid("negative max_beats, or room without a buffer");
    return BP_OK;
  }

  // the bounds, the room, the results of the segments without rows, and for the others their blocks, tiles and regions of
  // the beat pool
  int plan(bp_handle h, const char* what, int64_t n, const int64_t* offs, bool* queued) override {
    auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
    if (int rc = check_rows_in_all(h, what, offs[n])) return rc;
    const bp_beat_params& p = *a.params;
    int64_t room_needed = 0;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t rows = offs[i + 1] - offs[i];
      if (rows > BP_BEAT_MAX_ROWS)
        return invalid("segment " + std::to_string(i) + ": " + std::to_string(rows) + " rows, more than BP_BEAT_MAX_ROWS (" +
                       std::to_string(BP_BEAT_MAX_ROWS) + ")");
      room_needed += bp_beats_capacity(rows, p.lag_min);
    }
    if (a.max_beats < room_needed)
      return invalid("room for " + std::to_string(a.max_beats) + " beats, but the segments can have " + std::to_string(room_needed) +
                     " (the sum of bp_beats_capacity; nothing has been written)");
    for (int64_t i = 0; i < n; ++i) {
      const int64_t rows = offs[i + 1] - offs[i];
      a.summaries[i] = bp_beat_summary{rows == 0 ? 2 : 0, 0, 0, 0, 0.0};  // (no row: no pulse)
      if (rows == 0) continue;
      const int64_t last_lag = std::min<int64_t>(p.lag_max, rows - 1), room = bp_beats_capacity(rows, p.lag_min);
      const int32_t lag_tiles = last_lag < p.lag_min ? 0 : (int32_t)((last_lag - p.lag_min + kBeatTempoLags) / kBeatTempoLags);
      segs.push_back(BeatSeg{offs[i], rows, blocks, tiles, cap, room, lag_tiles, (int32_t)i});
      blocks += (rows + kBeatStrengthRows - 1) / kBeatStrengthRows;
      tiles += (rows + kBeatTempoRows - 1) / kBeatTempoRows * lag_tiles;
      cap += room;
    }
    *queued = !segs.empty();
    for (int64_t i = 0; i <= n && !*queued && a.beat_offsets; ++i) a.beat_offsets[i] = 0;  // (null: a call of zero segments may pass none)
    return BP_OK;
  }

  // the tables, the three launches, and the summaries and the beat pool on their way home (one page-locked block: the
  // summaries, then the pool)
  int queue(bp_handle h, const Maps& all, int64_t n, const int64_t* offs) override {
    hipStream_t s = h->stream;
    const int64_t nd = (int64_t)segs.size(), rows = offs[n];
    static_assert(sizeof(BeatParams) == sizeof(bp_beat_params) && sizeof(bp_beat_params) == 1064, "the parameters go to the device as they are");
    static_assert(sizeof(BeatSummary) == sizeof(bp_beat_summary) && sizeof(bp_beat_summary) == 32, "the summaries come home as they are");
    const size_t n_home = (size_t)(4 * nd + (cap + 1) / 2);  // in int64: 32 bytes a summary, 4 a beat
    BP_HIP(h->bt_params.reserve(1));
    BP_HIP(h->bt_segs.reserve((size_t)nd));
    BP_HIP(h->bt_strength.reserve((size_t)rows));
    BP_HIP(h->bt_acc.reserve((size_t)nd * kBeatAccStride));
    BP_HIP(h->bt_pred.reserve((size_t)rows));
    BP_HIP(h->bt_out.reserve(n_home));
    BP_HIP(h->bt_home.reserve(n_home));
    BP_HIP(hipMemcpyAsync(h->bt_params, a.params, sizeof(BeatParams), hipMemcpyHostToDevice, s));
    BP_HIP(hipMemcpyAsync(h->bt_segs, segs.data(), (size_t)nd * sizeof(BeatSeg), hipMemcpyHostToDevice, s));
    int64_t* out = h->bt_out;
    BP_HIP(launch_beats(all.onset, h->bt_params, h->bt_segs, nd, blocks, tiles, h->bt_strength, h->bt_acc, h->bt_pred,
                        reinterpret_cast<int32_t*>(out + 4 * nd), reinterpret_cast<BeatSummary*>(out), s));
    BP_HIP(hipMemcpyAsync(h->bt_home, out, n_home * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return BP_OK;
  }

  // the summaries and the pool are in the page-locked block; the beats leave it compact and ascending (a segment's lie in its
  // region of the pool last beat first)
  int home(bp_handle h, const char*, int64_t n, const int64_t*) override {
    const int64_t nd = (int64_t)segs.size();
    const int64_t* block = h->bt_home;
    const int32_t* pool = reinterpret_cast<const int32_t*>(block + 4 * nd);
    for (int64_t c = 0; c < nd; ++c) std::memcpy(&a.summaries[segs[(size_t)c].segment], block + 4 * c, sizeof(bp_beat_summary));
    int64_t at = 0, c = 0;
    for (int64_t i = 0; i < n; ++i) {
      a.beat_offsets[i] = at;
      if (c < nd && segs[(size_t)c].segment == i) {
        const BeatSeg& seg = segs[(size_t)c++];
        const int64_t nb = std::min(a.summaries[i].n_beats, seg.beat_cap);  // (n_beats is within the room by the header's bound)
        for (int64_t j = 0; j < nb; ++j) a.beats[at + j] = pool[seg.beat_first + nb - 1 - j];
        at += nb;
      }
    }
    a.beat_offsets[n] = at;
    return BP_OK;
  }
};

}  // namespace

extern "C" {

int bp_beats_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* onset, int mem_kind,
                       const bp_beat_params* p, bp_beat_summary* summaries, int32_t* beats, int64_t max_beats, int64_t* beat_offsets) {
  BeatSink sink({p, summaries, beats, max_beats, beat_offsets});
  return run_clips(h, "bp_beats_from_maps", given_maps(n_segments, row_offsets, nullptr, onset, nullptr, mem_kind), sink);
}

int bp_infer_clips_beats(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind, const bp_beat_params* p,
                         bp_beat_summary* summaries, int32_t* beats, int64_t max_beats, int64_t* beat_offsets) {
  BeatSink sink({p, summaries, beats, max_beats, beat_offsets});
  return run_clips(h, "bp_infer_clips_beats", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

// the clock readings of the path kernel for segment c of the handle's last beat call with rows (100 MHz ticks: start, period
// picked, recurrence done, backtrace done): tools/bench_beat.py
int bp_internal_beat_clocks(bp_handle h, int64_t c, int64_t* clocks) {
  if (!h || !clocks || c < 0 || (size_t)(c + 1) * kBeatAccStride > h->bt_acc.capacity()) return BP_ERR_INVALID_ARG;
  BP_HIP(hipSetDevice(h->device));
  BP_HIP(hipMemcpy(clocks, h->bt_acc + c * kBeatAccStride + kBeatAccClocks, 4 * sizeof(int64_t), hipMemcpyDeviceToHost));
  return BP_OK;
}

}  // extern "C"
