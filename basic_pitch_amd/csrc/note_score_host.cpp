// Note-level scoring on the host (include/basic_pitch_amd_score.h): bp_score_note_events, the checker the device kernel
// (note_score.hip) is held to and the route for the decodes a device call leaves, and the argument rules both share.
//
// The three predicates are the header's, in float64 and as written; the matching is Kuhn's augmenting paths over adjacency
// lists built once per graph.  The device searches differently (no lists, a scan per step); a maximum matching's size is
// unique, so the counts agree.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/basic_pitch_amd_score.h"

#pragma clang fp contract(off)
#pragma clang fp reassociate(off)

extern "C" {

void bp_score_params_default(bp_score_params* p) {
  if (!p) return;
  p->onset_tolerance_s = 0.05;       // mir_eval.transcription.precision_recall_f1_overlap's defaults
  p->offset_ratio = 0.2;
  p->offset_min_tolerance_s = 0.05;
  p->pitch_tolerance_cents = 50.0;
  p->strict = 0;
  p->reserved = 0;
}

// why a call refuses the score parameters (null: it takes them)
const char* bp_internal_score_bad_params(const bp_score_params* p) {
  if (!p) return "null score_params";
  const double v[4] = {p->onset_tolerance_s, p->offset_ratio, p->offset_min_tolerance_s, p->pitch_tolerance_cents};
  for (double x : v)
    if (!std::isfinite(x) || x < 0.0) return "score_params: a tolerance or the offset ratio is negative or not finite";
  return p->reserved != 0 ? "score_params: reserved must be 0" : nullptr;
}

// the first of n refs a call refuses — a field that is not finite, or an end before its start —, or -1
int64_t bp_internal_score_bad_ref(const bp_ref_note* refs, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    const bp_ref_note& r = refs[i];
    if (!std::isfinite(r.start_s) || !std::isfinite(r.end_s) || !std::isfinite(r.pitch_midi) || r.end_s < r.start_s) return i;
  }
  return -1;
}

// the offset tolerance a ref sets, the one expression of it: the checker below and the table the device reads (clips_sweep.hip)
double bp_internal_score_offset_tol(const bp_ref_note* r, const bp_score_params* p) {
  return std::fmax(p->offset_ratio * (r->end_s - r->start_s), p->offset_min_tolerance_s);
}

}  // extern "C"

namespace {

inline bool within(double d, double tol, bool strict) { return strict ? d < tol : d <= tol; }
inline double round6(double x) { return std::rint(x * 1e6) / 1e6; }

// the size of a maximum matching of events (left) to refs (right), adj[e] the refs event e hits
int64_t max_matching(const std::vector<std::vector<int32_t>>& adj, int64_t n_ref) {
  std::vector<int32_t> of_ref((size_t)n_ref, -1), path_e, path_r;
  std::vector<size_t> next(adj.size());
  std::vector<uint8_t> seen((size_t)n_ref);
  int64_t size = 0;
  for (size_t root = 0; root < adj.size(); ++root) {
    if (adj[root].empty()) continue;
    std::fill(seen.begin(), seen.end(), 0);
    path_e.assign(1, (int32_t)root), path_r.clear();
    next[root] = 0;
    while (!path_e.empty()) {
      const int32_t e = path_e.back();
      int32_t r = -1;
      while (next[(size_t)e] < adj[(size_t)e].size() && r < 0) {
        const int32_t c = adj[(size_t)e][next[(size_t)e]++];
        if (!seen[(size_t)c]) r = c;
      }
      if (r < 0) {  // a dead end: back to the event before, which goes on behind the ref it took
        path_e.pop_back();
        if (!path_r.empty()) path_r.pop_back();
        continue;
      }
      seen[(size_t)r] = 1;
      path_r.push_back(r);
      const int32_t held_by = of_ref[(size_t)r];
      if (held_by < 0) {  // a free ref: every event of the path takes the ref it chose
        for (size_t i = 0; i < path_e.size(); ++i) of_ref[(size_t)path_r[i]] = path_e[i];
        ++size;
        break;
      }
      path_e.push_back(held_by);
      next[(size_t)held_by] = 0;
    }
  }
  return size;
}

}  // namespace

extern "C" int bp_score_note_events(const bp_note_event* est, int64_t n_est, const bp_ref_note* ref, int64_t n_ref,
                                    const bp_score_params* p, bp_note_score* out) {
  if (!out || n_est < 0 || n_ref < 0 || (n_est > 0 && !est) || (n_ref > 0 && !ref) || n_est > INT32_MAX || n_ref > INT32_MAX)
    return BP_ERR_INVALID_ARG;
  if (bp_internal_score_bad_params(p) || bp_internal_score_bad_ref(ref, n_ref) >= 0) return BP_ERR_INVALID_ARG;
  const bool strict = p->strict != 0;
  std::vector<std::vector<int32_t>> onset((size_t)n_est), offset((size_t)n_est);
  for (int64_t e = 0; e < n_est; ++e)
    for (int64_t r = 0; r < n_ref; ++r) {
      const double d_on = round6(std::fabs(ref[r].start_s - est[e].start_s));
      const double cents = 100.0 * std::fabs(ref[r].pitch_midi - (double)est[e].pitch_midi);
      if (!within(d_on, p->onset_tolerance_s, strict) || !within(cents, p->pitch_tolerance_cents, strict)) continue;
      onset[(size_t)e].push_back((int32_t)r);
      const double d_off = round6(std::fabs(ref[r].end_s - est[e].end_s));
      if (within(d_off, bp_internal_score_offset_tol(&ref[r], p), strict)) offset[(size_t)e].push_back((int32_t)r);
    }
  out->n_ref = (int32_t)n_ref, out->n_est = (int32_t)n_est;
  out->matched_onset = (int32_t)max_matching(onset, n_ref);
  out->matched_offset = (int32_t)max_matching(offset, n_ref);
  return BP_OK;
}
