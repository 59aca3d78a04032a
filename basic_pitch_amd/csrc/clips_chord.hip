// Chords and key of every segment of a job, of the note rows alone (include/basic_pitch_amd_chord.h, chord.hip):
// the sink behind run_clips (clips_job.h) and its entry points.  Host code only.
#include <algorithm>
#include <cstring>

#include "../../include/basic_pitch_amd_chord.h"
#include "clips_job.h"

using namespace bp;

extern "C" const char* bp_internal_chord_bad_params(const bp_chord_params* p);                         // chord_host.cpp
extern "C" int bp_internal_chord_bounds_ok(const int32_t* bounds, int64_t n, int64_t rows);  // chord_host.cpp

namespace {

// A summary per segment under `params` and a label per row (room for max_labels), the units of segment i between
// bounds[bound_offsets[i] ... bound_offsets[i + 1]) (both null: frames everywhere).
struct ChordSink final : JobSink {
  struct Args {
    const bp_chord_params* params;
    const int64_t* bound_offsets;
    const int32_t* bounds;
    bp_chord_summary* summaries;
    uint8_t* labels;
    int64_t max_labels;
  } a;
  std::vector<ChordSeg> segs;  // the segments with rows, and what they take of the launches and of the pools
  int64_t blocks = 0, units = 0, pool_units = 0;
  explicit ChordSink(const Args& args) : a(args) {}

  // the note rows alone, read where they lie unless they are in host memory or not 16-byte aligned
  MapsUse use(bp_handle h) const override { return MapsUse{true, false, false, true, false, &h->ch_note, nullptr, nullptr}; }

  int check(bp_handle h, const char* what, int64_t n_segs) override {
    auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
    if (n_segs < 0 || (n_segs > 0 && !a.summaries)) return invalid("negative n_segments / n_clips, or null summaries");
    if (const char* why = bp_internal_chord_bad_params(a.params)) return invalid(std::string("params: ") + why);
    if (!check_room(a.max_labels, a.labels)) return invalid("negative max_labels, or room without a buffer");
    if (!a.bound_offsets != !a.bounds) return invalid("bounds and bound_offsets go together: one of them is null");
    if (a.bound_offsets) {
      const int64_t at = ascending_from_zero(a.bound_offsets, n_segs);
      if (at >= 0) return invalid("bound_offsets do not start at 0 or decrease at entry " + std::to_string(at));
    }
    return BP_OK;
  }

  // the bounds, the room, the boundaries of every segment, the results of the segments without rows, and for the others
  // their blocks and their regions of the unit pools
  int plan(bp_handle h, const char* what, int64_t n, const int64_t* offs, bool* queued) override {
    auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
    if (int rc = check_rows_in_all(h, what, offs[n])) return rc;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t rows = offs[i + 1] - offs[i];
      if (rows > BP_CHORD_MAX_ROWS)
        return invalid("segment " + std::to_string(i) + ": " + std::to_string(rows) + " rows, more than BP_CHORD_MAX_ROWS (" +
                       std::to_string(BP_CHORD_MAX_ROWS) + ")");
      if (a.bounds && !bp_internal_chord_bounds_ok(a.bounds + a.bound_offsets[i], a.bound_offsets[i + 1] - a.bound_offsets[i], rows))
        return invalid("segment " + std::to_string(i) + ": its boundaries are not strictly ascending inside 0 < B < " + std::to_string(rows));
    }
    if (a.max_labels < offs[n])
      return invalid("room for " + std::to_string(a.max_labels) + " labels, but the segments have " + std::to_string(offs[n]) +
                     " rows (nothing has been written)");
    for (int64_t i = 0; i < n; ++i) {
      const int64_t rows = offs[i + 1] - offs[i];
      a.summaries[i] = bp_chord_summary{rows == 0 ? 2 : 0, -1, 0, 0, 0, 0};  // (no row: nothing sounds)
      if (rows == 0) continue;
      const int64_t bound_first = a.bounds ? a.bound_offsets[i] : 0, n_bounds = a.bounds ? a.bound_offsets[i + 1] - bound_first : 0;
      const int64_t n_units = n_bounds ? n_bounds + 1 : rows;
      segs.push_back(ChordSeg{offs[i], rows, blocks, units, n_units, pool_units, bound_first, n_bounds ? 1 : 0, (int32_t)i});
      blocks += (rows + kChordChromaRows - 1) / kChordChromaRows;
      units += n_units;
      if (n_bounds) pool_units += n_units;
    }
    *queued = !segs.empty();
    return BP_OK;
  }

  // the tables, the launches, and the summaries and the labels on their way home (one page-locked block: the summaries,
  // then the labels)
  int queue(bp_handle h, const Maps& all, int64_t n, const int64_t* offs) override {
    hipStream_t s = h->stream;
    const int64_t nd = (int64_t)segs.size(), rows = offs[n], n_bounds = a.bounds ? a.bound_offsets[n] : 0;
    static_assert(sizeof(ChordParams) == sizeof(bp_chord_params) && sizeof(bp_chord_params) == 3456, "the parameters go to the device as they are");
    static_assert(sizeof(ChordSummary) == sizeof(bp_chord_summary) && sizeof(bp_chord_summary) == 32, "the summaries come home as they are");
    const size_t n_home = (size_t)(4 * nd + (rows + 7) / 8);  // in int64: 32 bytes a summary, 1 a label
    BP_HIP(h->ch_params.reserve(1));
    BP_HIP(h->ch_segs.reserve((size_t)nd));
    BP_HIP(h->ch_bounds.reserve((size_t)std::max<int64_t>(1, n_bounds)));
    BP_HIP(h->ch_chroma.reserve((size_t)rows * 16));
    BP_HIP(h->ch_pool.reserve((size_t)std::max<int64_t>(1, pool_units) * 16));
    BP_HIP(h->ch_acc.reserve((size_t)nd * kChordAccStride));
    BP_HIP(h->ch_records.reserve((size_t)units));
    BP_HIP(h->ch_unit_labels.reserve((size_t)units));
    BP_HIP(h->ch_out.reserve(n_home));
    BP_HIP(h->ch_home.reserve(n_home));
    BP_HIP(hipMemcpyAsync(h->ch_params, a.params, sizeof(ChordParams), hipMemcpyHostToDevice, s));
    BP_HIP(hipMemcpyAsync(h->ch_segs, segs.data(), (size_t)nd * sizeof(ChordSeg), hipMemcpyHostToDevice, s));
    if (n_bounds) {
      BP_HIP(hipMemcpyAsync(h->ch_bounds, a.bounds, (size_t)n_bounds * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    int64_t* out = h->ch_out;
    BP_HIP(launch_chords(all.note, h->ch_params, h->ch_segs, nd, blocks, rows, pool_units, h->ch_bounds, h->ch_chroma, h->ch_pool, h->ch_acc,
                         h->ch_records, h->ch_unit_labels, reinterpret_cast<uint8_t*>(out + 4 * nd), reinterpret_cast<ChordSummary*>(out), s));
    BP_HIP(hipMemcpyAsync(h->ch_home, out, n_home * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return BP_OK;
  }

  // the summaries and the labels are in the page-locked block; the segments with rows tile the rows, so the labels leave as
  // one run
  int home(bp_handle h, const char*, int64_t n, const int64_t* offs) override {
    const int64_t nd = (int64_t)segs.size();
    const int64_t* block = h->ch_home;
    for (int64_t c = 0; c < nd; ++c) std::memcpy(&a.summaries[segs[(size_t)c].segment], block + 4 * c, sizeof(bp_chord_summary));
    if (offs[n]) std::memcpy(a.labels, block + 4 * nd, (size_t)offs[n]);
    return BP_OK;
  }
};

}  // namespace

extern "C" {

int bp_chords_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, int mem_kind,
                        const bp_chord_params* p, const int64_t* bound_offsets, const int32_t* bounds, bp_chord_summary* summaries,
                        uint8_t* labels, int64_t max_labels) {
  ChordSink sink({p, bound_offsets, bounds, summaries, labels, max_labels});
  return run_clips(h, "bp_chords_from_maps", given_maps(n_segments, row_offsets, note, nullptr, nullptr, mem_kind), sink);
}

int bp_infer_clips_chords(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind, const bp_chord_params* p,
                          const int64_t* bound_offsets, const int32_t* bounds, bp_chord_summary* summaries, uint8_t* labels,
                          int64_t max_labels) {
  ChordSink sink({p, bound_offsets, bounds, summaries, labels, max_labels});
  return run_clips(h, "bp_infer_clips_chords", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

// the clock readings of the path kernel for segment c of the handle's last chord call with rows (100 MHz ticks: start, key
// picked, recurrence done, backtrace done): tools/bench_chord.py
int bp_internal_chord_clocks(bp_handle h, int64_t c, int64_t* clocks) {
  if (!h || !clocks || c < 0 || (size_t)(c + 1) * kChordAccStride > h->ch_acc.capacity()) return BP_ERR_INVALID_ARG;
  BP_HIP(hipSetDevice(h->device));
  BP_HIP(hipMemcpy(clocks, h->ch_acc + c * kChordAccStride + kChordAccClocks, 4 * sizeof(int64_t), hipMemcpyDeviceToHost));
  return BP_OK;
}

}  // extern "C"
