// Tempo and beats on the host (include/basic_pitch_amd_beat.h): bp_beat_rows, the checker the device kernels (beat.hip) are
// held to, the prior table and the room for beats, and the validation of the parameters that the device entry points
// (clips_beat.hip) use instead of a copy.  Device-free: links with plain g++.
//
// Everything is the header's integers; the one float64 expression, the refined period, is written operation by operation.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/basic_pitch_amd_beat.h"

namespace {

constexpr int kPitches = BP_BEAT_PITCHES;

inline int quantise(float x) { return (int)floorf(fminf(fmaxf(x, 0.0f), 1.0f) * 1024.0f + 0.5f); }

}  // namespace

extern "C" {

int bp_beat_prior(double start_bpm, double sd_octaves, int32_t* prior) {
  if (!prior || !(start_bpm > 0.0) || !(sd_octaves > 0.0) || !std::isfinite(start_bpm) || !std::isfinite(sd_octaves)) return BP_ERR_INVALID_ARG;
  const double L0 = 60.0 * 22050.0 / 256.0 / start_bpm;
  prior[0] = 0;
  for (int L = 1; L <= BP_BEAT_MAX_LAG; ++L) {
    const double z = std::log2((double)L / L0) / sd_octaves;
    prior[L] = (int32_t)std::lrint(1024.0 * std::exp(-0.5 * z * z));
  }
  return BP_OK;
}

void bp_beat_params_default(bp_beat_params* p) {
  if (!p) return;
  *p = bp_beat_params{};
  p->threshold_q = 307, p->min_pitch = 0, p->max_pitch = kPitches - 1, p->lag_min = 21, p->lag_max = 172, p->tightness = 4;
  bp_beat_prior(120.0, 1.0, p->prior);
}

// why a parameter set is refused; null: it is taken
const char* bp_internal_beat_bad_params(const bp_beat_params* p) {
  if (!p) return "null params";
  if (p->threshold_q < 0 || p->threshold_q > BP_BEAT_Q_ONE) return "threshold_q is not in 0 ... 1024";
  if (p->min_pitch < 0 || p->min_pitch > p->max_pitch || p->max_pitch >= kPitches) return "min_pitch / max_pitch are not 0 <= min_pitch <= max_pitch <= 87";
  if (p->lag_min < 2 || p->lag_min > p->lag_max || p->lag_max > BP_BEAT_MAX_LAG) return "lag_min / lag_max are not 2 <= lag_min <= lag_max <= 256";
  if (p->tightness < 0 || p->tightness > BP_BEAT_MAX_TIGHTNESS) return "tightness is not in 0 ... 1024";
  for (int L = 0; L <= BP_BEAT_MAX_LAG; ++L)
    if (p->prior[L] < 0 || p->prior[L] > BP_BEAT_Q_ONE) return "a prior entry is not in 0 ... 1024";
  return p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved_tail != 0 ? "reserved must be 0" : nullptr;
}

int64_t bp_beats_capacity(int64_t rows, int32_t lag_min) {
  if (rows < 0 || lag_min < 2 || lag_min > BP_BEAT_MAX_LAG) return -1;
  const int64_t gap = lag_min / 2 > 1 ? lag_min / 2 : 1;
  return rows <= lag_min ? 0 : (rows - 1) / gap + 1;
}

int bp_beat_rows(const float* onset, int64_t rows, const bp_beat_params* p, int32_t* beats, int64_t max_beats,
                 bp_beat_summary* summary) {
  if (rows < 0 || rows > BP_BEAT_MAX_ROWS || (rows > 0 && !onset) || !summary || bp_internal_beat_bad_params(p) || max_beats < 0 ||
      (max_beats > 0 && !beats) || max_beats < bp_beats_capacity(rows, p->lag_min))
    return BP_ERR_INVALID_ARG;
  *summary = bp_beat_summary{0, 0, 0, 0, 0.0};
  for (int64_t i = 0; i < rows * kPitches; ++i)
    if (std::isnan(onset[i])) {
      summary->status = 1;
      return BP_OK;
    }
  summary->status = 2;  // until a pulse is found
  if (rows - 1 < p->lag_min) return BP_OK;
  // strength
  std::vector<int32_t> o((size_t)rows);
  int64_t sum = 0, sum_sq = 0;
  for (int64_t t = 0; t < rows; ++t) {
    int32_t v = 0;
    for (int q = p->min_pitch; q <= p->max_pitch; ++q) {
      const int above = quantise(onset[t * kPitches + q]) - p->threshold_q;
      v += above > 0 ? above : 0;
    }
    o[(size_t)t] = v, sum += v, sum_sq += (int64_t)v * v;
  }
  // tempo
  const int64_t last_lag = p->lag_max < rows - 1 ? p->lag_max : rows - 1;
  std::vector<int64_t> S((size_t)last_lag + 2, 0);
  int64_t P = p->lag_min;
  for (int64_t L = p->lag_min; L <= last_lag; ++L) {
    int64_t a = 0;
    for (int64_t t = 0; t + L < rows; ++t) a += (int64_t)o[(size_t)t] * o[(size_t)(t + L)];
    S[(size_t)L] = a * p->prior[L];
    if (S[(size_t)L] > S[(size_t)P]) P = L;
  }
  if (S[(size_t)P] == 0) return BP_OK;
  // scale and penalty (sum > 0: a product of two strengths is)
  const int64_t m = sum_sq / sum, dmin = P / 2 > 1 ? P / 2 : 1, dmax = 2 * P;
  std::vector<int64_t> pen((size_t)dmax + 1, 0);
  for (int64_t d = dmin; d <= dmax; ++d) pen[(size_t)d] = (int64_t)p->tightness * m * (d - P) * (d - P) / (P * P);
  // recurrence
  std::vector<int64_t> Cst((size_t)rows);
  std::vector<uint16_t> pred((size_t)rows);  // the gap to the previous beat; 0: a start
  for (int64_t t = 0; t < rows; ++t) {
    int64_t best = 0, from = 0;
    for (int64_t d = dmin; d <= dmax && d <= t; ++d) {
      const int64_t c = Cst[(size_t)(t - d)] - pen[(size_t)d];
      if (c > best) best = c, from = d;
    }
    Cst[(size_t)t] = o[(size_t)t] + best, pred[(size_t)t] = (uint16_t)from;
  }
  // path
  int64_t end = rows - P > 0 ? rows - P : 0;
  for (int64_t t = end + 1; t < rows; ++t)
    if (Cst[(size_t)t] > Cst[(size_t)end]) end = t;
  int64_t n = 1;
  for (int64_t t = end; pred[(size_t)t]; t -= pred[(size_t)t]) ++n;
  int64_t k = n;
  for (int64_t t = end;; t -= pred[(size_t)t]) {
    beats[--k] = (int32_t)t;
    if (!pred[(size_t)t]) break;
  }
  double refined = (double)P;
  if (p->lag_min < P && P < last_lag) {
    const double l = (double)S[(size_t)P - 1], c = (double)S[(size_t)P], r = (double)S[(size_t)P + 1];
    if (c > l && c > r) {  // (so the denominator is below 0 whatever the rounding)
      const double num = 0.5 * (l - r), twice = 2.0 * c, den = (l - twice) + r;
      refined = (double)P + num / den;
    }
  }
  *summary = bp_beat_summary{0, (int32_t)P, n, S[(size_t)P], refined};
  return BP_OK;
}

}  // extern "C"
