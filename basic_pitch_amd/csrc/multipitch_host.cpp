// Multi-pitch estimates on the host (include/basic_pitch_amd_multipitch.h): bp_multipitch_rows, the checker the device kernels
// (multipitch.hip) are held to, and bp_score_f0_frames, the frame-level counts with the peaks' pitches as the estimate side —
// the checker of the scored sweep and the route for the decodes it leaves.  Device-free: links with plain g++ beside
// note_frames_host.cpp, note_score_host.cpp and note_decode.cpp, whose functions for the frame time, the frames a ref sounds on
// and the validation of refs and tolerances it uses; it has no copy of them.
//
// The predicates and the refinement are the header's, as written: float32 comparisons, float64 arithmetic, nothing fused or
// reassociated.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/basic_pitch_amd_multipitch.h"

#pragma clang fp contract(off)
#pragma clang fp reassociate(off)

extern "C" const char* bp_internal_score_bad_params(const bp_score_params* p);  // note_score_host.cpp
extern "C" int64_t bp_internal_score_bad_ref(const bp_ref_note* refs, int64_t n);
extern "C" void bp_internal_frame_interval(double start_s, double end_s, int64_t n_frames, int64_t* f0, int64_t* f1);  // note_frames_host.cpp

namespace {

inline bool finite32(float v) { return std::fabs(v) <= 3.402823466e+38f; }
inline bool is_peak(const float* row, int b, const bp_mp_params& p) {
  return row[b] >= p.threshold && row[b] > row[b - 1] && row[b] > row[b + 1];
}
inline bool within(double d, double tol, bool strict) { return strict ? d < tol : d <= tol; }
inline bool hits(double ref_pitch, double est_pitch, const bp_score_params* p) {
  return within(100.0 * std::fabs(ref_pitch - est_pitch), p->pitch_tolerance_cents, p->strict != 0);
}

struct Span {
  int64_t f0, f1;  // sounds on f0 ... f1 - 1
  double pitch;
};

}  // namespace

extern "C" {

void bp_mp_params_default(bp_mp_params* p) {
  if (p) *p = bp_mp_params{0.3f, 1, BP_MP_BINS - 2, 0};
}

// why a parameter set is refused; null: it is taken
const char* bp_internal_mp_bad_params(const bp_mp_params* p) {
  if (!p) return "null params";
  if (!finite32(p->threshold)) return "the threshold is not finite";
  if (p->min_bin < 1) return "min_bin is below 1";
  if (p->max_bin > BP_MP_BINS - 2) return "max_bin is above 262";
  if (p->min_bin > p->max_bin) return "min_bin is above max_bin";
  return p->reserved != 0 ? "reserved must be 0" : nullptr;
}

int bp_multipitch_rows(const float* contour, int64_t rows, const bp_mp_params* p, bp_f0_point* points, int64_t max_points,
                       int64_t* n_points, int* status) {
  if (rows < 0 || (rows > 0 && !contour) || max_points < 0 || (max_points > 0 && !points) || !n_points || !status ||
      rows > INT32_MAX || bp_internal_mp_bad_params(p))
    return BP_ERR_INVALID_ARG;
  *n_points = 0, *status = 0;
  for (int64_t i = 0; i < rows * BP_MP_BINS; ++i)
    if (!finite32(contour[i])) {
      *status = 1;
      return BP_OK;
    }
  int64_t n = 0;
  for (int64_t t = 0; t < rows; ++t)
    for (int b = p->min_bin; b <= p->max_bin; ++b) n += is_peak(contour + t * BP_MP_BINS, b, *p);
  *n_points = n;
  if (n > max_points) return BP_ERR_INVALID_ARG;
  bp_f0_point* out = points;
  for (int64_t t = 0; t < rows; ++t) {
    const float* row = contour + t * BP_MP_BINS;
    for (int b = p->min_bin; b <= p->max_bin; ++b) {
      if (!is_peak(row, b, *p)) continue;
      const double l = (double)row[b - 1], c = (double)row[b], r = (double)row[b + 1];
      const double delta = 0.5 * (l - r) / ((l - 2.0 * c) + r);
      *out++ = bp_f0_point{(int32_t)t, row[b], 21.0 + ((double)b + delta) / 3.0};
    }
  }
  return BP_OK;
}

int bp_score_f0_frames(const bp_f0_point* est, int64_t n_est, const bp_ref_note* ref, int64_t n_ref, int64_t n_frames,
                       const bp_score_params* p, bp_frame_score* out) {
  if (!out || n_est < 0 || n_ref < 0 || n_frames < 0 || (n_est > 0 && !est) || (n_ref > 0 && !ref) || n_ref > INT32_MAX)
    return BP_ERR_INVALID_ARG;
  if (bp_internal_score_bad_params(p) || bp_internal_score_bad_ref(ref, n_ref) >= 0) return BP_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n_est; ++i)
    if (!std::isfinite(est[i].pitch_midi)) return BP_ERR_INVALID_ARG;
  // the refs in ascending pitch with the frames they sound on; the points by frame, then pitch
  std::vector<Span> refs;
  for (int64_t i = 0; i < n_ref; ++i) {
    Span s{0, 0, ref[i].pitch_midi};
    bp_internal_frame_interval(ref[i].start_s, ref[i].end_s, n_frames, &s.f0, &s.f1);
    if (s.f0 < s.f1) refs.push_back(s);
  }
  std::stable_sort(refs.begin(), refs.end(), [](const Span& a, const Span& b) { return a.pitch < b.pitch; });
  std::vector<std::pair<int64_t, double>> pts;
  for (int64_t i = 0; i < n_est; ++i)
    if (est[i].frame >= 0 && est[i].frame < n_frames) pts.emplace_back(est[i].frame, est[i].pitch_midi);
  std::sort(pts.begin(), pts.end());
  pts.erase(std::unique(pts.begin(), pts.end()), pts.end());

  bp_frame_score sum{n_frames, 0, 0, 0, 0};
  // the ref side of every frame: no point on a frame leaves min(n_ref, 0) - 0 = 0 substitutions there
  for (const Span& r : refs) sum.ref_frames += r.f1 - r.f0;
  sum.est_frames = (int64_t)pts.size();
  for (size_t a = 0; a < pts.size();) {
    const int64_t fr = pts[a].first;
    size_t b = a;
    while (b < pts.size() && pts[b].first == fr) ++b;
    int64_t n_r = 0, tp = 0;
    size_t next = a;  // the estimates below are taken, or too low for this ref and every later one
    for (const Span& r : refs) {
      if (!(r.f0 <= fr && fr < r.f1)) continue;
      ++n_r;
      while (next < b && pts[next].second < r.pitch && !hits(r.pitch, pts[next].second, p)) ++next;
      if (next < b && hits(r.pitch, pts[next].second, p)) ++tp, ++next;
    }
    sum.true_pos += tp, sum.e_sub += std::min<int64_t>(n_r, (int64_t)(b - a)) - tp;
    a = b;
  }
  *out = sum;
  return BP_OK;
}

}  // extern "C"
