// The melody of a contour map on the host (include/basic_pitch_amd_melody.h): bp_melody_rows, the checker the device kernel
// (melody.hip) is held to, bp_score_melody_frames, the checker of the scored sweep, and the validation of parameter sets and
// reference tracks that the device entry points (clips_melody.hip) use instead of a copy.  Device-free: links with plain g++
// beside note_frames_host.cpp and note_score_host.cpp, whose validation of the tolerances it uses.
//
// The recurrence and the refinement are the header's, as written: float32 operations one at a time, the parabola in float64,
// nothing fused or reassociated.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/basic_pitch_amd_melody.h"

#pragma clang fp contract(off)
#pragma clang fp reassociate(off)
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif

extern "C" const char* bp_internal_score_bad_params(const bp_score_params* p);  // note_score_host.cpp

namespace {

constexpr int kBins = BP_MP_BINS;
constexpr float kMaxMagnitude = 65536.0f;

inline bool in_range(float v) { return std::fabs(v) <= kMaxMagnitude; }  // false for NaN
inline bool within(double d, double tol, bool strict) { return strict ? d < tol : d <= tol; }

}  // namespace

extern "C" {

void bp_melody_params_default(bp_melody_params* p) {
  if (p) *p = bp_melody_params{0.3f, 0.05f, 0.5f, 4, 0, kBins - 1, {0, 0}};
}

// why a parameter set is refused; null: it is taken
const char* bp_internal_melody_bad_params(const bp_melody_params* p) {
  if (!p) return "null params";
  if (!in_range(p->threshold)) return "the threshold is not finite or beyond +-65536";
  if (!(p->jump_penalty >= 0.0f && p->jump_penalty <= kMaxMagnitude)) return "jump_penalty is not in 0 ... 65536";
  if (!(p->voicing_penalty >= 0.0f && p->voicing_penalty <= kMaxMagnitude)) return "voicing_penalty is not in 0 ... 65536";
  if (p->max_jump < 0 || p->max_jump > BP_MELODY_MAX_JUMP) return "max_jump is not in 0 ... 16";
  if (p->min_bin < 0) return "min_bin is below 0";
  if (p->max_bin > kBins - 1) return "max_bin is above 263";
  if (p->min_bin > p->max_bin) return "min_bin is above max_bin";
  return p->reserved[0] != 0 || p->reserved[1] != 0 ? "reserved must be 0" : nullptr;
}

// the first entry of a reference track that is negative or not finite; -1: none
int64_t bp_internal_melody_bad_ref(const double* ref_pitch, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!(ref_pitch[i] >= 0.0) || !std::isfinite(ref_pitch[i])) return i;
  return -1;
}

int bp_melody_rows(const float* contour, int64_t rows, const bp_melody_params* p, bp_melody_point* points, int64_t max_points,
                   int* status) {
  if (rows < 0 || max_points < rows || (rows > 0 && (!contour || !points)) || !status || rows > INT32_MAX ||
      bp_internal_melody_bad_params(p))
    return BP_ERR_INVALID_ARG;
  *status = 0;
  for (int64_t t = 0; t < rows; ++t) points[t] = bp_melody_point{-1, 0.0f, 0.0};
  for (int64_t i = 0; i < rows * kBins; ++i)
    if (!in_range(contour[i])) {
      *status = 1;
      return BP_OK;
    }
  if (rows == 0) return BP_OK;
  const int lo = p->min_bin, hi = p->max_bin, J = p->max_jump, U = kBins;
  float pen[BP_MELODY_MAX_JUMP + 1];
  for (int d = 0; d <= J; ++d) pen[d] = p->jump_penalty * (float)d;
  // pred[t][b]: the source bin, or U; pred[t][U] likewise
  std::vector<int16_t> pred((size_t)rows * (kBins + 1));
  float prev[kBins + 1], cur[kBins + 1], P[kBins + 1];
  for (int b = lo; b <= hi; ++b) prev[b] = contour[b];
  prev[U] = p->threshold;
  for (int64_t t = 1; t < rows; ++t) {
    const float* row = contour + t * kBins;
    int16_t* from = pred.data() + (size_t)t * (kBins + 1);
    const float u = prev[U];
    for (int b = lo; b <= hi; ++b) P[b] = prev[b] - u;
    P[U] = prev[U] - u;
    for (int b = lo; b <= hi; ++b) {
      const int first = b - J < lo ? lo : b - J, last = b + J > hi ? hi : b + J;
      float best = P[first] - pen[b - first];
      int arg = first;
      for (int s = first + 1; s <= last; ++s) {
        const float cand = P[s] - pen[s < b ? b - s : s - b];
        if (cand > best) best = cand, arg = s;
      }
      const float cand = P[U] - p->voicing_penalty;
      if (cand > best) best = cand, arg = U;
      cur[b] = row[b] + best;
      from[b] = (int16_t)arg;
    }
    float best = P[lo] - p->voicing_penalty;
    int arg = lo;
    for (int s = lo + 1; s <= hi; ++s) {
      const float cand = P[s] - p->voicing_penalty;
      if (cand > best) best = cand, arg = s;
    }
    if (P[U] > best) best = P[U], arg = U;
    cur[U] = p->threshold + best;
    from[U] = (int16_t)arg;
    for (int b = lo; b <= hi; ++b) prev[b] = cur[b];
    prev[U] = cur[U];
  }
  int state = lo;
  for (int s = lo + 1; s <= hi; ++s)
    if (prev[s] > prev[state]) state = s;
  if (prev[U] > prev[state]) state = U;
  for (int64_t t = rows - 1; t >= 0; --t) {
    if (state != U) {
      const float* row = contour + t * kBins;
      const int b = state;
      double delta = 0.0;
      if (b >= 1 && b <= kBins - 2 && row[b] > row[b - 1] && row[b] > row[b + 1]) {
        const double l = (double)row[b - 1], c = (double)row[b], r = (double)row[b + 1];
        delta = 0.5 * (l - r) / ((l - 2.0 * c) + r);
      }
      points[t] = bp_melody_point{b, row[b], 21.0 + ((double)b + delta) / 3.0};
    }
    if (t > 0) state = pred[(size_t)t * (kBins + 1) + (size_t)state];
  }
  return BP_OK;
}

int bp_score_melody_frames(const bp_melody_point* est, const double* ref_pitch, int64_t n_frames, const bp_score_params* p,
                           bp_melody_score* out) {
  if (!out || n_frames < 0 || (n_frames > 0 && (!est || !ref_pitch)) || bp_internal_score_bad_params(p)) return BP_ERR_INVALID_ARG;
  if (bp_internal_melody_bad_ref(ref_pitch, n_frames) >= 0) return BP_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n_frames; ++i)
    if (est[i].bin >= 0 && !std::isfinite(est[i].pitch_midi)) return BP_ERR_INVALID_ARG;
  bp_melody_score s{n_frames, 0, 0, 0, 0, 0};
  const double tol = p->pitch_tolerance_cents;
  const bool strict = p->strict != 0;
  for (int64_t i = 0; i < n_frames; ++i) {
    const bool rv = ref_pitch[i] != 0.0, ev = est[i].bin >= 0;
    s.ref_voiced += rv, s.est_voiced += ev;
    if (!rv || !ev) continue;
    ++s.both_voiced;
    const double d = 100.0 * (ref_pitch[i] - est[i].pitch_midi);
    s.pitch_ok += within(std::fabs(d), tol, strict);
    s.chroma_ok += within(std::fabs(d - 1200.0 * std::floor(d / 1200.0 + 0.5)), tol, strict);
  }
  *out = s;
  return BP_OK;
}

}  // extern "C"
