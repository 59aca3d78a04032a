// Forced alignment of every segment of a job: the states of a score against the note and onset rows
// (include/basic_pitch_amd_align.h, align.hip): the sink behind run_clips (clips_job.h) and its entry points.
// Host code only.
#include <algorithm>

#include "../../include/basic_pitch_amd_align.h"
#include "clips_job.h"

using namespace bp;

extern "C" const char* bp_internal_align_bad_params(const bp_align_params* p);  // align_host.cpp
extern "C" const char* bp_internal_align_bad_states(const bp_align_state* states, int64_t n, int64_t* index);

namespace {

// Segment i against states[state_offsets[i] ... state_offsets[i + 1]) under `params`: first_frame parallel to the states (room
// for max_states), total and status per segment.
struct AlignSink final : JobSink {
  struct Args {
    const int64_t* state_offsets;
    const bp_align_state* states;
    const bp_align_params* params;
    int32_t* first_frame;
    int64_t max_states;
    int64_t* total;
    int* status;
  } a;
  std::vector<AlignSeg> segs;  // the segments with rows and states, and what they take of the pools
  int64_t cells = 0, words = 0, tiles = 0;
  int most_states = 0;
  explicit AlignSink(const Args& args) : a(args) {}

  // the note and onset rows alone, read where they lie unless they are in host memory or not 16-byte aligned
  MapsUse use(bp_handle h) const override { return MapsUse{true, true, false, true, false, &h->al_note, &h->al_onset, nullptr}; }

  int check(bp_handle h, const char* what, int64_t n_segs) override {
    auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
    if (n_segs < 0 || (n_segs > 0 && (!a.status || !a.total))) return invalid("negative n_segments / n_clips, or null total or status");
    if (const char* why = bp_internal_align_bad_params(a.params)) return invalid(std::string("params: ") + why);
    if (n_segs == 0) return BP_OK;
    if (ascending_from_zero(a.state_offsets, n_segs) >= 0) return invalid("state_offsets must start at 0 and never decrease");
    const int64_t n_states = a.state_offsets[n_segs];
    if (n_states > 0 && !a.states) return invalid("null states");
    if (!check_room(a.max_states, a.first_frame)) return invalid("negative max_states, or room without a buffer");
    if (a.max_states < n_states)
      return invalid("room for " + std::to_string(a.max_states) + " first frames, but the segments have " + std::to_string(n_states) +
                     " states (nothing has been written)");
    for (int64_t i = 0; i < n_segs; ++i)
      if (a.state_offsets[i + 1] - a.state_offsets[i] > BP_ALIGN_MAX_STATES)
        return invalid("segment " + std::to_string(i) + ": " + std::to_string(a.state_offsets[i + 1] - a.state_offsets[i]) +
                       " states, more than BP_ALIGN_MAX_STATES (" + std::to_string(BP_ALIGN_MAX_STATES) + ")");
    int64_t bad = -1;
    if (const char* why = bp_internal_align_bad_states(a.states, n_states, &bad)) return invalid("state " + std::to_string(bad) + ": " + why);
    return BP_OK;
  }

  // the bounds, the results of the segments that need no device, and for the others their regions of the pools
  int plan(bp_handle h, const char* what, int64_t n, const int64_t* offs, bool* queued) override {
    auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
    if (int rc = check_rows_in_all(h, what, offs[n])) return rc;
    int64_t cells_so_far = 0;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t rows = offs[i + 1] - offs[i], S = a.state_offsets[i + 1] - a.state_offsets[i];
      if (rows > 0 && S == 0) return invalid("segment " + std::to_string(i) + ": rows but no state (a path needs a state)");
      cells_so_far += rows * S;  // (at most 2^23 x 2^12 a segment: no overflow before the test)
      if (cells_so_far > BP_ALIGN_MAX_CELLS)
        return invalid(std::to_string(cells_so_far) + " cells (rows x states) up to segment " + std::to_string(i) +
                       ", more than BP_ALIGN_MAX_CELLS (" + std::to_string(BP_ALIGN_MAX_CELLS) + "): split the job");
    }
    for (int64_t i = 0; i < n; ++i) {
      const int64_t rows = offs[i + 1] - offs[i], S = a.state_offsets[i + 1] - a.state_offsets[i];
      a.total[i] = 0, a.status[i] = rows == 0 && S > 0 ? 2 : 0;  // (states without a row: infeasible)
      for (int64_t j = 0; j < S; ++j) a.first_frame[a.state_offsets[i] + j] = -1;
      if (rows == 0 || S == 0) continue;
      segs.push_back(AlignSeg{offs[i], rows, a.state_offsets[i], cells, words, tiles, (int32_t)S, (int32_t)i});
      cells += rows * S, words += rows * ((S + 63) / 64);
      tiles += ((rows + kAlignEmitRows - 1) / kAlignEmitRows) * ((S + kAlignEmitRows - 1) / kAlignEmitRows);
      most_states = std::max(most_states, (int)S);
    }
    *queued = !segs.empty();
    return BP_OK;
  }

  // the tables, the launches, and the first frames, totals and statuses on their way home
  int queue(bp_handle h, const Maps& all, int64_t n, const int64_t*) override {
    hipStream_t s = h->stream;
    const int64_t nd = (int64_t)segs.size(), n_states = a.state_offsets[n];
    static_assert(sizeof(AlignState) == sizeof(bp_align_state) && sizeof(bp_align_state) == 40, "the states go to the device as they are");
    const size_t n_out = (size_t)(nd + (nd + 1) / 2);
    BP_HIP(h->al_states.reserve((size_t)n_states));
    BP_HIP(h->al_segs.reserve((size_t)nd));
    BP_HIP(h->al_gains.reserve((size_t)cells * 8));
    BP_HIP(h->al_pred.reserve((size_t)words));
    BP_HIP(h->al_nan.reserve((size_t)nd));
    BP_HIP(h->al_first.reserve((size_t)n_states));
    BP_HIP(h->al_out.reserve(n_out));
    BP_HIP(h->al_home.reserve(n_out));
    BP_HIP(hipMemcpyAsync(h->al_states, a.states, (size_t)n_states * sizeof(AlignState), hipMemcpyHostToDevice, s));
    BP_HIP(hipMemcpyAsync(h->al_segs, segs.data(), (size_t)nd * sizeof(AlignSeg), hipMemcpyHostToDevice, s));
    // (the first frames of the segments that are not queued are -1 already, on the host and here)
    BP_HIP(hipMemsetAsync(h->al_first, 0xff, (size_t)n_states * sizeof(int32_t), s));
    int64_t* out = h->al_out;
    BP_HIP(launch_align(all.note, all.onset, h->al_states, h->al_segs, nd, tiles, most_states, a.params->threshold_q, a.params->onset_weight,
                        static_cast<uint8_t*>(h->al_gains), h->al_pred, h->al_nan, h->al_first, out, reinterpret_cast<int32_t*>(out + nd), s));
    BP_HIP(hipMemcpyAsync(a.first_frame, h->al_first, (size_t)n_states * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    BP_HIP(hipMemcpyAsync(h->al_home, out, n_out * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return BP_OK;
  }

  // the totals and the statuses are in the page-locked block
  int home(bp_handle h, const char*, int64_t, const int64_t*) override {
    const int64_t nd = (int64_t)segs.size();
    const int32_t* st = statuses_behind(h->al_home, nd);
    for (int64_t c = 0; c < nd; ++c) {
      const int32_t i = segs[(size_t)c].segment;
      a.total[i] = h->al_home[c], a.status[i] = st[c];
    }
    return BP_OK;
  }
};

}  // namespace

extern "C" {

int bp_align_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, const float* onset,
                       int mem_kind, const int64_t* state_offsets, const bp_align_state* states, const bp_align_params* p,
                       int32_t* first_frame, int64_t max_states, int64_t* total, int* status) {
  AlignSink sink({state_offsets, states, p, first_frame, max_states, total, status});
  return run_clips(h, "bp_align_from_maps", given_maps(n_segments, row_offsets, note, onset, nullptr, mem_kind), sink);
}

int bp_infer_clips_align(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                         const int64_t* state_offsets, const bp_align_state* states, const bp_align_params* p, int32_t* first_frame,
                         int64_t max_states, int64_t* total, int* status) {
  AlignSink sink({state_offsets, states, p, first_frame, max_states, total, status});
  return run_clips(h, "bp_infer_clips_align", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

}  // extern "C"
