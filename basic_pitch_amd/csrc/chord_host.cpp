// Chords and key on the host (include/basic_pitch_amd_chord.h): bp_chord_rows, the checker the device kernels (chord.hip) are
// held to, the default tables, and the validation of the parameters and of a segment's boundaries that the device entry
// points (clips_chord.hip) use instead of a copy.  Device-free: links with plain g++.
//
// Everything is the header's integers; the one float64 computation, the key profiles, makes a table that is an input.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/basic_pitch_amd_chord.h"

namespace {

constexpr int kPitches = BP_CHORD_PITCHES, kClasses = BP_CHORD_CLASSES;

inline int quantise(float x) { return (int)floorf(fminf(fmaxf(x, 0.0f), 1.0f) * 1024.0f + 0.5f); }

// the qualities in the order of the vocabularies: tones above the root, -1 ends a chord
constexpr int kTones[7][5] = {{0, 4, 7, -1, -1}, {0, 3, 7, -1, -1}, {0, 3, 6, -1, -1}, {0, 4, 8, -1, -1},
                              {0, 4, 7, 10, -1}, {0, 4, 7, 11, -1}, {0, 3, 7, 10, -1}};
constexpr int kMajMin[] = {0, 1}, kTriads[] = {0, 1, 2, 3}, kSevenths[] = {0, 1, 4, 5, 6};

constexpr double kProfiles[2][kClasses] = {{6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88},
                                           {6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17}};

}  // namespace

extern "C" {

int bp_chord_templates(int vocabulary, bp_chord_params* p) {
  if (!p || vocabulary < BP_CHORD_VOCAB_MAJMIN || vocabulary > BP_CHORD_VOCAB_SEVENTHS) return BP_ERR_INVALID_ARG;
  const int* qualities = vocabulary == BP_CHORD_VOCAB_MAJMIN ? kMajMin : (vocabulary == BP_CHORD_VOCAB_TRIADS ? kTriads : kSevenths);
  const int n_qualities = vocabulary == BP_CHORD_VOCAB_MAJMIN ? 2 : (vocabulary == BP_CHORD_VOCAB_TRIADS ? 4 : 5);
  for (int s = 0; s < BP_CHORD_MAX_STATES; ++s) {
    p->bias[s] = 0;
    for (int k = 0; k < kClasses; ++k) p->weights[s][k] = 0;
  }
  p->bias[0] = 12;  // N
  p->n_states = 1 + 12 * n_qualities;
  for (int i = 0; i < n_qualities; ++i)
    for (int root = 0; root < 12; ++root) {
      const int* tones = kTones[qualities[i]];
      int n = 0;
      while (n < 5 && tones[n] >= 0) ++n;
      int32_t* w = p->weights[1 + 12 * i + root];
      for (int k = 0; k < kClasses; ++k) w[k] = -n;
      for (int j = 0; j < n; ++j) w[(root + tones[j]) % 12] = 12 - n;
    }
  return BP_OK;
}

int bp_chord_key_profiles(bp_chord_params* p) {
  if (!p) return BP_ERR_INVALID_ARG;
  for (int mode = 0; mode < 2; ++mode) {
    double mean = 0.0, norm = 0.0;
    for (int k = 0; k < kClasses; ++k) mean += kProfiles[mode][k];
    mean /= kClasses;
    for (int k = 0; k < kClasses; ++k) norm += (kProfiles[mode][k] - mean) * (kProfiles[mode][k] - mean);
    norm = std::sqrt(norm);
    for (int k = 0; k < kClasses; ++k) p->key_profile[mode][k] = (int32_t)std::lrint(1024.0 * (kProfiles[mode][k] - mean) / norm);
  }
  return BP_OK;
}

void bp_chord_params_default(bp_chord_params* p) {
  if (!p) return;
  *p = bp_chord_params{};
  p->threshold_q = 307, p->min_pitch = 0, p->max_pitch = kPitches - 1, p->switch_penalty = 128;
  bp_chord_templates(BP_CHORD_VOCAB_MAJMIN, p);
  bp_chord_key_profiles(p);
}

// why a parameter set is refused; null: it is taken
const char* bp_internal_chord_bad_params(const bp_chord_params* p) {
  if (!p) return "null params";
  if (p->threshold_q < 0 || p->threshold_q > BP_CHORD_Q_ONE) return "threshold_q is not in 0 ... 1024";
  if (p->min_pitch < 0 || p->min_pitch > p->max_pitch || p->max_pitch >= kPitches) return "min_pitch / max_pitch are not 0 <= min_pitch <= max_pitch <= 87";
  if (p->n_states < 1 || p->n_states > BP_CHORD_MAX_STATES) return "n_states is not in 1 ... 64";
  if (p->switch_penalty < 0 || p->switch_penalty > BP_CHORD_MAX_PENALTY) return "switch_penalty is not in 0 ... 1024";
  auto outside = [](int32_t v) { return v < -BP_CHORD_MAX_WEIGHT || v > BP_CHORD_MAX_WEIGHT; };
  for (int s = 0; s < BP_CHORD_MAX_STATES; ++s) {
    if (outside(p->bias[s])) return "a bias entry is not in -1024 ... 1024";
    for (int k = 0; k < kClasses; ++k)
      if (outside(p->weights[s][k])) return "a weights entry is not in -1024 ... 1024";
  }
  for (int k = 0; k < 2 * kClasses; ++k)
    if (outside(p->key_profile[k / kClasses][k % kClasses])) return "a key_profile entry is not in -1024 ... 1024";
  return p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0 ? "reserved must be 0" : nullptr;
}

// whether n boundaries are strictly ascending inside 0 < B < rows
int bp_internal_chord_bounds_ok(const int32_t* bounds, int64_t n, int64_t rows) {
  for (int64_t i = 0; i < n; ++i)
    if (bounds[i] <= (i ? bounds[i - 1] : 0) || bounds[i] >= rows) return 0;
  return 1;
}

int bp_chord_rows(const float* note, int64_t rows, const bp_chord_params* p, const int32_t* bounds, int64_t n_bounds, uint8_t* labels,
                  int64_t max_labels, bp_chord_summary* summary) {
  if (rows < 0 || rows > BP_CHORD_MAX_ROWS || (rows > 0 && !note) || !summary || bp_internal_chord_bad_params(p) || n_bounds < 0 ||
      (n_bounds > 0 && !bounds) || !bp_internal_chord_bounds_ok(bounds, n_bounds, rows) || max_labels < rows || (max_labels > 0 && !labels))
    return BP_ERR_INVALID_ARG;
  *summary = bp_chord_summary{0, -1, 0, 0, 0, 0};
  for (int64_t t = 0; t < rows; ++t) labels[t] = 0;
  for (int64_t i = 0; i < rows * kPitches; ++i)
    if (std::isnan(note[i])) {
      summary->status = 1;
      return BP_OK;
    }
  summary->status = 2;  // until something sounds
  // chroma, the scale's sums and the totals of the classes
  std::vector<int32_t> c((size_t)rows * kClasses, 0);
  int64_t sum = 0, sum_sq = 0, total[kClasses] = {};
  for (int64_t t = 0; t < rows; ++t) {
    int32_t* row = &c[(size_t)t * kClasses];
    for (int q = p->min_pitch; q <= p->max_pitch; ++q) {
      const int above = quantise(note[t * kPitches + q]) - p->threshold_q;
      if (above > 0) row[(q + 9) % 12] += above;
    }
    for (int k = 0; k < kClasses; ++k) sum += row[k], sum_sq += (int64_t)row[k] * row[k], total[k] += row[k];
  }
  if (sum == 0) return BP_OK;
  const int64_t m = sum_sq / sum;
  // key
  int key = 0;
  int64_t key_score = 0;
  for (int j = 0; j < 24; ++j) {
    int64_t K = 0;
    for (int k = 0; k < kClasses; ++k) K += (int64_t)p->key_profile[j / 12][(k - j % 12 + 12) % 12] * total[k];
    if (j == 0 || K > key_score) key = j, key_score = K;
  }
  // recurrence over the units
  const int n = p->n_states;
  const int64_t n_units = n_bounds ? n_bounds + 1 : rows;
  auto unit_first = [&](int64_t u) { return n_bounds ? (u ? (int64_t)bounds[u - 1] : 0) : u; };
  auto unit_end = [&](int64_t u) { return n_bounds ? (u < n_bounds ? (int64_t)bounds[u] : rows) : u + 1; };
  std::vector<uint64_t> moved((size_t)n_units, 0);  // bit s: the predecessor of state s at the unit is `from`, not s
  std::vector<uint8_t> from((size_t)n_units, 0);
  int64_t D[BP_CHORD_MAX_STATES] = {};
  for (int64_t u = 0; u < n_units; ++u) {
    const int64_t len = unit_end(u) - unit_first(u);
    int64_t cu[kClasses] = {};
    for (int64_t t = unit_first(u); t < unit_end(u); ++t)
      for (int k = 0; k < kClasses; ++k) cu[k] += c[(size_t)t * kClasses + k];
    int a = 0;
    for (int s = 1; s < n; ++s)
      if (D[s] > D[a]) a = s;
    const int64_t over = D[a] - len * p->switch_penalty * m;
    from[(size_t)u] = (uint8_t)a;
    for (int s = 0; s < n; ++s) {
      int64_t e = len * p->bias[s] * m;
      for (int k = 0; k < kClasses; ++k) e += (int64_t)p->weights[s][k] * cu[k];
      const bool move = u > 0 && over > D[s];  // (D[a] itself is never below `over`: a stays)
      if (move) moved[(size_t)u] |= 1ull << s;
      D[s] = e + (u == 0 ? 0 : (move ? over : D[s]));
    }
  }
  // path
  int cur = 0;
  for (int s = 1; s < n; ++s)
    if (D[s] > D[cur]) cur = s;
  const int64_t score = D[cur];
  int32_t changes = 0;
  for (int64_t u = n_units - 1; u >= 0; --u) {
    for (int64_t t = unit_first(u); t < unit_end(u); ++t) labels[t] = (uint8_t)cur;
    if (u > 0 && ((moved[(size_t)u] >> cur) & 1)) changes += from[(size_t)u] != cur, cur = from[(size_t)u];
  }
  *summary = bp_chord_summary{0, key, (int32_t)n_units, changes, score, key_score};
  return BP_OK;
}

}  // extern "C"
