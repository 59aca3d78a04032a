// Multi-pitch estimates of every segment of a job: the f0 peaks of the contour rows, and the frame-level counts of threshold
// sweeps over them (include/basic_pitch_amd_multipitch.h, multipitch.hip): the sink behind run_clips
// (clips_job.h) and its entry points.  Host code only.
#include <algorithm>
#include <cstring>

#include "../../include/basic_pitch_amd_multipitch.h"
#include "clips_job.h"

using namespace bp;

extern "C" const char* bp_internal_mp_bad_params(const bp_mp_params* p);  // multipitch_host.cpp

namespace {

MpParams mp_device_params(const bp_mp_params& p) { return MpParams{p.threshold, p.min_bin, p.max_bin, 0}; }

// The points: of the n segments under sets[0], room for max_points, point_offsets [n + 1] and status per segment.  scored:
// n_decodes decodes of the segments under sets[0 ... n_sets), scored against the refs: `frames` and status per decode alone go
// home.
struct MultiPitchSink final : JobSink {
  struct Args {
    bool scored;
    int64_t n_sets;
    const bp_mp_params* sets;
    int64_t n_decodes;
    const bp_sweep_decode* decodes;
    bp_f0_point* points;
    int64_t max_points;
    int64_t* point_offsets;
    const int64_t* ref_offsets;
    const bp_ref_note* refs;
    const bp_score_params* score_params;
    bp_frame_score* frames;
    int* status;
  } a;
  const float* contour = nullptr;  // where the contour rows lie on the device (the write pass runs after the first wait)
  std::vector<MpDecode> dec;       // scored: the decode table and the refs in pitch order as multipitch.hip reads them
  std::vector<MpRef> refs;
  explicit MultiPitchSink(const Args& args) : a(args) {}

  // the contour rows alone, read where they lie: a map in host memory gets a device copy, one in device memory is not copied
  MapsUse use(bp_handle h) const override { return MapsUse{false, false, true, false, false, nullptr, nullptr, &h->mp_contour}; }

  int check(bp_handle h, const char* what, int64_t n_segs) override {
    auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
    if (!a.scored) {
      if (n_segs < 0 || !a.point_offsets || (n_segs > 0 && !a.status)) return invalid("negative n_segments / n_clips, null point_offsets or status");
      if (!check_room(a.max_points, a.points)) return invalid("negative max_points, or room without a buffer");
      if (const char* why = bp_internal_mp_bad_params(a.sets)) return invalid(std::string("params: ") + why);
      return BP_OK;
    }
    if (int rc = check_sets_and_decodes(h, what, n_segs, a.n_sets, a.n_decodes, a.decodes, (a.n_sets > 0 && !a.sets) || (a.n_decodes > 0 && !a.status),
                                        "negative n_segments / n_clips, n_sets or n_decodes, null sets or status", nullptr,
                                        [&](int64_t p) { return bp_internal_mp_bad_params(a.sets + p); }))
      return rc;
    return check_score(h, what, n_segs, a.n_decodes, a.ref_offsets, a.refs, a.score_params, a.frames, "frames");
  }

  // A scored sweep: the decode table, and per segment its refs in ascending pitch with the frames they sound on.
  int plan(bp_handle h, const char* what, int64_t n, const int64_t* offs, bool* queued) override {
    if (!a.scored) {
      if (int rc = check_rows_in_all(h, what, offs[n])) return rc;
      *queued = offs[n] > 0;
      for (int64_t i = 0; i <= n && !*queued; ++i) a.point_offsets[i] = 0;
      for (int64_t i = 0; i < n && !*queued; ++i) a.status[i] = 0;
      return BP_OK;
    }
    dec.resize((size_t)a.n_decodes);
    int64_t rows_in_all = 0;
    for (int64_t j = 0; j < a.n_decodes; ++j) {
      const DecodePair d = decode_pair(a.decodes, j, n);
      const int64_t i = d.segment, first = a.ref_offsets[i];
      dec[(size_t)j] = MpDecode{offs[i], offs[i + 1] - offs[i], first, (int32_t)std::min<int64_t>(a.ref_offsets[i + 1] - first, kNoteScoreMaxNotes + 1), d.set};
      rows_in_all += offs[i + 1] - offs[i];
    }
    if (int rc = check_rows_in_all(h, what, rows_in_all)) return rc;
    *queued = rows_in_all > 0;
    if (!*queued) {  // (every decode is of a segment without rows)
      for (int64_t j = 0; j < a.n_decodes; ++j) {
        a.frames[j] = bp_frame_score{0, 0, 0, 0, 0};
        a.status[j] = dec[(size_t)j].n_ref > kNoteScoreMaxNotes ? 3 : 0;
      }
      return BP_OK;
    }
    refs.resize((size_t)a.ref_offsets[n]);
    refs_in_pitch_order(n, offs, a.ref_offsets, a.refs, [&](size_t slot, const bp_ref_note& ref, int32_t f0, int32_t f1) {
      refs[slot] = MpRef{f0, f1, ref.pitch_midi};
    });
    return BP_OK;
  }

  // The points: the count pass, the scan, and the offsets and statuses on their way home — the write pass waits for the
  // host's look at the total (home).  A scored sweep: its tables, its one launch, the counts with the statuses on their way home.
  int queue(bp_handle h, const Maps& all, int64_t n, const int64_t* offs) override {
    hipStream_t s = h->stream;
    const int64_t T = offs[n];
    contour = all.contour;
    if (!a.scored) {
      const size_t n_meta = (size_t)(n + 1 + (n + 1) / 2);
      BP_HIP(h->clip_rows.reserve((size_t)n + 1));
      BP_HIP(h->mp_rows.reserve((size_t)T));
      BP_HIP(h->mp_first.reserve((size_t)T + 1));
      BP_HIP(h->mp_bad.reserve((size_t)n));
      BP_HIP(h->mp_meta.reserve(n_meta));
      BP_HIP(h->mp_home.reserve(n_meta));
      BP_HIP(hipMemcpyAsync(h->clip_rows, offs, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
      BP_HIP(hipMemsetAsync(h->mp_bad, 0, (size_t)n * sizeof(int32_t), s));
      BP_HIP(launch_mp_count(contour, h->clip_rows, n, T, mp_device_params(*a.sets), h->mp_rows, h->mp_bad, s));
      BP_HIP(launch_mp_scan(h->mp_rows, h->mp_bad, h->clip_rows, n, T, h->mp_first, h->mp_meta, s));
      BP_HIP(hipMemcpyAsync(h->mp_home, h->mp_meta, n_meta * sizeof(int64_t), hipMemcpyDeviceToHost, s));
      return BP_OK;
    }
    const int64_t nd = a.n_decodes;
    const size_t n_out = (size_t)(5 * nd + (nd + 1) / 2);
    int64_t max_rows = 0;
    for (const MpDecode& d : dec) max_rows = std::max(max_rows, d.rows);
    static_assert(sizeof(MpParams) == sizeof(bp_mp_params), "the sets go to the device as they are");
    BP_HIP(h->mp_sets.reserve((size_t)a.n_sets));
    BP_HIP(h->mp_dec.reserve((size_t)nd));
    BP_HIP(h->mp_refs.reserve(refs.size()));
    BP_HIP(h->mp_out.reserve(n_out));
    BP_HIP(h->mp_home.reserve(n_out));
    BP_HIP(hipMemcpyAsync(h->mp_sets, a.sets, (size_t)a.n_sets * sizeof(MpParams), hipMemcpyHostToDevice, s));
    BP_HIP(hipMemcpyAsync(h->mp_dec, dec.data(), (size_t)nd * sizeof(MpDecode), hipMemcpyHostToDevice, s));
    if (!refs.empty()) BP_HIP(hipMemcpyAsync(h->mp_refs, refs.data(), refs.size() * sizeof(MpRef), hipMemcpyHostToDevice, s));
    BP_HIP(launch_mp_sweep_frames(contour, h->mp_sets, h->mp_dec, h->mp_refs,
                                  MpScoreParams{a.score_params->pitch_tolerance_cents, a.score_params->strict != 0}, nd, max_rows, h->mp_out, s));
    BP_HIP(hipMemcpyAsync(h->mp_home, h->mp_out, n_out * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return BP_OK;
  }

  // The points: the offsets and statuses are in the page-locked block; when the total fits the caller's room, the write pass
  // and the points home, and the wait for them.  A scored sweep: the counts and statuses.
  int home(bp_handle h, const char* what, int64_t n, const int64_t* offs) override {
    if (a.scored) {
      std::memcpy(a.frames, h->mp_home, (size_t)a.n_decodes * sizeof(bp_frame_score));
      const int32_t* st = statuses_behind(h->mp_home, 5 * a.n_decodes);
      for (int64_t j = 0; j < a.n_decodes; ++j) a.status[j] = st[j];
      return BP_OK;
    }
    const int64_t* meta = h->mp_home;
    const int32_t* st = statuses_behind(meta, n + 1);
    const int64_t total = meta[n];
    for (int64_t i = 0; i <= n; ++i) a.point_offsets[i] = meta[i];
    for (int64_t i = 0; i < n; ++i) a.status[i] = st[i];
    if (total > a.max_points) {
      h->err = std::string(what) + ": output buffer too small: " + std::to_string(total) +
               " points are needed (point_offsets[n] holds them; nothing has been written to points)";
      return BP_ERR_INVALID_ARG;
    }
    if (total == 0) return BP_OK;
    auto write = [&]() -> int {
      BP_HIP(h->mp_points.reserve((size_t)total * sizeof(bp_f0_point)));
      BP_HIP(launch_mp_write(contour, offs[n], mp_device_params(*a.sets), h->mp_rows, h->mp_bad, h->clip_rows, h->mp_first, h->mp_points,
                             h->stream));
      BP_HIP(hipMemcpyAsync(a.points, h->mp_points, (size_t)total * sizeof(bp_f0_point), hipMemcpyDeviceToHost, h->stream));
      return BP_OK;
    };
    return finish(h, write());
  }
};

MultiPitchSink::Args points_of(const bp_mp_params* p, bp_f0_point* points, int64_t max_points, int64_t* point_offsets, int* status) {
  return {false, 1, p, 0, nullptr, points, max_points, point_offsets, nullptr, nullptr, nullptr, nullptr, status};
}
MultiPitchSink::Args scored(int64_t n_sets, const bp_mp_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes, const int64_t* ref_offsets,
                            const bp_ref_note* refs, const bp_score_params* score_params, bp_frame_score* frames, int* status) {
  return {true, n_sets, sets, n_decodes, decodes, nullptr, 0, nullptr, ref_offsets, refs, score_params, frames, status};
}

}  // namespace

extern "C" {

int bp_multipitch_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour, int mem_kind,
                            const bp_mp_params* p, bp_f0_point* points, int64_t max_points, int64_t* point_offsets, int* status) {
  MultiPitchSink sink(points_of(p, points, max_points, point_offsets, status));
  return run_clips(h, "bp_multipitch_from_maps", given_maps(n_segments, row_offsets, nullptr, nullptr, contour, mem_kind), sink);
}

int bp_infer_clips_multipitch(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                              const bp_mp_params* p, bp_f0_point* points, int64_t max_points, int64_t* point_offsets, int* status) {
  MultiPitchSink sink(points_of(p, points, max_points, point_offsets, status));
  return run_clips(h, "bp_infer_clips_multipitch", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

int bp_multipitch_sweep_frame_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour, int mem_kind,
                                    int64_t n_sets, const bp_mp_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                                    const int64_t* ref_offsets, const bp_ref_note* refs, const bp_score_params* score_params,
                                    bp_frame_score* frames, int* status) {
  MultiPitchSink sink(scored(n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, frames, status));
  return run_clips(h, "bp_multipitch_sweep_frame_score", given_maps(n_segments, row_offsets, nullptr, nullptr, contour, mem_kind), sink);
}

int bp_infer_clips_multipitch_sweep_frame_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                                int64_t n_sets, const bp_mp_params* sets, int64_t n_decodes,
                                                const bp_sweep_decode* decodes, const int64_t* ref_offsets, const bp_ref_note* refs,
                                                const bp_score_params* score_params, bp_frame_score* frames, int* status) {
  MultiPitchSink sink(scored(n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, frames, status));
  return run_clips(h, "bp_infer_clips_multipitch_sweep_frame_score", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

}  // extern "C"
