// The melody of every segment of a job: one f0 track by a Viterbi recurrence over the contour rows, and the melody measures of
// parameter sweeps over it (include/basic_pitch_amd_melody.h, melody.hip): the sink behind run_clips
// (clips_job.h) and its entry points.  Host code only.
#include <algorithm>
#include <cstring>

#include "../../include/basic_pitch_amd_melody.h"
#include "clips_job.h"

using namespace bp;

extern "C" const char* bp_internal_melody_bad_params(const bp_melody_params* p);  // melody_host.cpp
extern "C" int64_t bp_internal_melody_bad_ref(const double* ref_pitch, int64_t n);
extern "C" const char* bp_internal_score_bad_params(const bp_score_params* p);

namespace {

// The records: of the n segments under sets[0], a record per row, room for max_points of them, status per segment.  scored:
// n_decodes decodes of the segments under sets[0 ... n_sets), scored against ref_pitch (parallel to the rows of the segments):
// scores and status per decode alone go home.
struct MelodySink final : JobSink {
  struct Args {
    bool scored;
    int64_t n_sets;
    const bp_melody_params* sets;
    int64_t n_decodes;
    const bp_sweep_decode* decodes;
    bp_melody_point* points;  // the records, room for max_points
    int64_t max_points;
    const double* ref_pitch;  // scored
    const bp_score_params* score_params;
    bp_melody_score* scores;
    int* status;
  } a;
  std::vector<MelodyDecode> dec;  // the records: a decode per segment with rows; scored: the decode table
  explicit MelodySink(const Args& args) : a(args) {}

  // the contour rows alone, read where they lie: a map in host memory gets a device copy, one in device memory is not copied
  MapsUse use(bp_handle h) const override { return MapsUse{false, false, true, false, false, nullptr, nullptr, &h->mel_contour}; }

  int check(bp_handle h, const char* what, int64_t n_segs) override {
    auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
    if (!a.scored) {
      if (n_segs < 0 || (n_segs > 0 && !a.status)) return invalid("negative n_segments / n_clips, or null status");
      if (!check_room(a.max_points, a.points)) return invalid("negative max_points, or room without a buffer");
      if (const char* why = bp_internal_melody_bad_params(a.sets)) return invalid(std::string("params: ") + why);
      return BP_OK;
    }
    if (int rc = check_sets_and_decodes(h, what, n_segs, a.n_sets, a.n_decodes, a.decodes,
                                        (a.n_sets > 0 && !a.sets) || (a.n_decodes > 0 && (!a.status || !a.scores)),
                                        "negative n_segments / n_clips, n_sets or n_decodes, null sets, scores or status", nullptr,
                                        [&](int64_t p) { return bp_internal_melody_bad_params(a.sets + p); }))
      return rc;
    if (const char* why = bp_internal_score_bad_params(a.score_params)) return invalid(why);
    return BP_OK;
  }

  // the room, the reference track, the bound, the decode table with every decode's region of the predecessor pool
  int plan(bp_handle h, const char* what, int64_t n, const int64_t* offs, bool* queued) override {
    auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
    if (!a.scored) {
      if (int rc = check_rows_in_all(h, what, offs[n])) return rc;
      if (a.max_points < offs[n])
        return invalid("room for " + std::to_string(a.max_points) + " records, but the segments have " + std::to_string(offs[n]) +
                       " rows and a row is a record (nothing has been written)");
      *queued = offs[n] > 0;
      for (int64_t i = 0; i < n; ++i) a.status[i] = 0;
      for (int64_t i = 0; i < n && *queued; ++i)
        if (offs[i + 1] > offs[i]) dec.push_back(MelodyDecode{offs[i], offs[i + 1] - offs[i], offs[i], 0, (int32_t)i});
      return BP_OK;
    }
    if (offs[n] > 0 && !a.ref_pitch) return invalid("null ref_pitch");
    const int64_t bad = bp_internal_melody_bad_ref(a.ref_pitch, offs[n]);
    if (bad >= 0) return invalid("ref_pitch " + std::to_string(bad) + ": negative or not finite");
    dec.resize((size_t)a.n_decodes);
    int64_t rows_in_all = 0;
    for (int64_t j = 0; j < a.n_decodes; ++j) {
      const DecodePair d = decode_pair(a.decodes, j, n);
      dec[(size_t)j] = MelodyDecode{offs[d.segment], offs[d.segment + 1] - offs[d.segment], rows_in_all, d.set, 0};
      rows_in_all += offs[d.segment + 1] - offs[d.segment];
      if (int rc = check_rows_in_all(h, what, rows_in_all)) return rc;
    }
    *queued = rows_in_all > 0;
    for (int64_t j = 0; j < a.n_decodes && !*queued; ++j) a.scores[j] = bp_melody_score{0, 0, 0, 0, 0, 0}, a.status[j] = 0;
    return BP_OK;
  }

  // The tables, the one launch, and the records or the counts with the statuses on their way home.  The records: the
  // `reserved` word of a decode is its segment (the kernel does not read it), and the statuses come home per decode.
  int queue(bp_handle h, const Maps& all, int64_t n, const int64_t* offs) override {
    hipStream_t s = h->stream;
    const int64_t nd = (int64_t)dec.size(), n_sets = a.scored ? a.n_sets : 1;
    int64_t pred_rows = 0;
    int max_jump = 0;  // of the sets a decode names
    for (const MelodyDecode& d : dec) pred_rows += d.rows, max_jump = std::max(max_jump, (int)a.sets[d.set].max_jump);
    static_assert(sizeof(MelodyParams) == sizeof(bp_melody_params), "the sets go to the device as they are");
    const size_t n_out = (size_t)((a.scored ? 6 * nd : 0) + (nd + 1) / 2);
    BP_HIP(h->mel_sets.reserve((size_t)n_sets));
    BP_HIP(h->mel_dec.reserve((size_t)nd));
    BP_HIP(h->mel_pred.reserve((size_t)pred_rows * kMelodyPredStride));
    BP_HIP(h->mel_out.reserve(n_out));
    BP_HIP(h->mel_home.reserve(n_out));
    BP_HIP(hipMemcpyAsync(h->mel_sets, a.sets, (size_t)n_sets * sizeof(MelodyParams), hipMemcpyHostToDevice, s));
    BP_HIP(hipMemcpyAsync(h->mel_dec, dec.data(), (size_t)nd * sizeof(MelodyDecode), hipMemcpyHostToDevice, s));
    int64_t* out = h->mel_out;
    if (a.scored) {
      BP_HIP(h->mel_ref.reserve((size_t)offs[n]));
      BP_HIP(hipMemcpyAsync(h->mel_ref, a.ref_pitch, (size_t)offs[n] * sizeof(double), hipMemcpyHostToDevice, s));
      BP_HIP(launch_melody(all.contour, h->mel_sets, h->mel_dec, nd, max_jump, h->mel_pred, nullptr, h->mel_ref,
                           MpScoreParams{a.score_params->pitch_tolerance_cents, a.score_params->strict != 0}, out,
                           reinterpret_cast<int32_t*>(out + 6 * nd), s));
    } else {
      BP_HIP(h->mel_points.reserve((size_t)offs[n] * sizeof(bp_melody_point)));
      BP_HIP(launch_melody(all.contour, h->mel_sets, h->mel_dec, nd, max_jump, h->mel_pred, h->mel_points, nullptr, MpScoreParams{0.0, false},
                           nullptr, reinterpret_cast<int32_t*>(out), s));
      BP_HIP(hipMemcpyAsync(a.points, h->mel_points, (size_t)offs[n] * sizeof(bp_melody_point), hipMemcpyDeviceToHost, s));
    }
    BP_HIP(hipMemcpyAsync(h->mel_home, out, n_out * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return BP_OK;
  }

  // the statuses, and a scored sweep's counts in front of them, are in the page-locked block
  int home(bp_handle h, const char*, int64_t, const int64_t*) override {
    const int64_t nd = (int64_t)dec.size();
    const int32_t* st = statuses_behind(h->mel_home, a.scored ? 6 * nd : 0);
    if (a.scored) std::memcpy(a.scores, h->mel_home, (size_t)nd * sizeof(bp_melody_score));
    for (int64_t j = 0; j < nd; ++j) a.status[a.scored ? j : dec[(size_t)j].reserved] = st[j];
    return BP_OK;
  }
};

MelodySink::Args records(const bp_melody_params* p, bp_melody_point* points, int64_t max_points, int* status) {
  return {false, 1, p, 0, nullptr, points, max_points, nullptr, nullptr, nullptr, status};
}
MelodySink::Args scored(int64_t n_sets, const bp_melody_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                        const double* ref_pitch, const bp_score_params* score_params, bp_melody_score* scores, int* status) {
  return {true, n_sets, sets, n_decodes, decodes, nullptr, 0, ref_pitch, score_params, scores, status};
}

}  // namespace

extern "C" {

int bp_melody_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour, int mem_kind,
                        const bp_melody_params* p, bp_melody_point* points, int64_t max_points, int* status) {
  MelodySink sink(records(p, points, max_points, status));
  return run_clips(h, "bp_melody_from_maps", given_maps(n_segments, row_offsets, nullptr, nullptr, contour, mem_kind), sink);
}

int bp_infer_clips_melody(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                          const bp_melody_params* p, bp_melody_point* points, int64_t max_points, int* status) {
  MelodySink sink(records(p, points, max_points, status));
  return run_clips(h, "bp_infer_clips_melody", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

int bp_melody_sweep_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour, int mem_kind,
                          int64_t n_sets, const bp_melody_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                          const double* ref_pitch, const bp_score_params* score_params, bp_melody_score* scores, int* status) {
  MelodySink sink(scored(n_sets, sets, n_decodes, decodes, ref_pitch, score_params, scores, status));
  return run_clips(h, "bp_melody_sweep_score", given_maps(n_segments, row_offsets, nullptr, nullptr, contour, mem_kind), sink);
}

int bp_infer_clips_melody_sweep_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                      int64_t n_sets, const bp_melody_params* sets, int64_t n_decodes,
                                      const bp_sweep_decode* decodes, const double* ref_pitch,
                                      const bp_score_params* score_params, bp_melody_score* scores, int* status) {
  MelodySink sink(scored(n_sets, sets, n_decodes, decodes, ref_pitch, score_params, scores, status));
  return run_clips(h, "bp_infer_clips_melody_sweep_score", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

}  // extern "C"
