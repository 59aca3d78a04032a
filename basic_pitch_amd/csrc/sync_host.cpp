// Two recordings against each other on the host (include/basic_pitch_amd_sync.h): bp_sync_rows, the checker the device kernels
// (sync.hip) are held to, and the validation of the parameters that the device entry points (clips_sync.hip) use instead of a
// copy.  Device-free: links with plain g++.  Everything is the header's integers.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/basic_pitch_amd_sync.h"

namespace {

constexpr int kPitches = BP_SYNC_PITCHES, kClasses = BP_SYNC_CLASSES;
constexpr int32_t kUnreachable = -1;  // a reachable D is a sum of gains: never negative

inline int quantise(float x) { return (int)floorf(fminf(fmaxf(x, 0.0f), 1.0f) * 1024.0f + 0.5f); }

inline int64_t units_of(int64_t rows, int64_t hop) { return (rows + hop - 1) / hop; }

// the smallest r with r * r >= s, 0 <= s < 2^42: by bisection over 0 ... 2^21
int64_t ceil_root(int64_t s) {
  int64_t lo = 0, hi = 1ll << 21;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (mid * mid >= s) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the features of a segment, 12 bytes a unit; false: a NaN somewhere in its rows
bool features(const float* note, int64_t rows, const bp_sync_params* p, std::vector<uint8_t>& x) {
  for (int64_t i = 0; i < rows * kPitches; ++i)
    if (std::isnan(note[i])) return false;
  const int64_t U = units_of(rows, p->hop);
  x.assign((size_t)U * kClasses, 0);
  for (int64_t u = 0; u < U; ++u) {
    int64_t cu[kClasses] = {};
    for (int64_t t = u * p->hop; t < (u + 1) * p->hop && t < rows; ++t)
      for (int q = p->min_pitch; q <= p->max_pitch; ++q) {
        const int above = quantise(note[t * kPitches + q]) - p->threshold_q;
        if (above > 0) cu[(q + 9) % 12] += above;
      }
    int64_t s = 0;
    for (int k = 0; k < kClasses; ++k) s += cu[k] * cu[k];
    if (s == 0) continue;
    const int64_t r = ceil_root(s);
    for (int k = 0; k < kClasses; ++k) x[(size_t)u * kClasses + k] = (uint8_t)(255 * cu[k] / r);
  }
  return true;
}

}  // namespace

extern "C" {

void bp_sync_params_default(bp_sync_params* p) {
  if (!p) return;
  *p = bp_sync_params{};
  p->threshold_q = 307, p->min_pitch = 0, p->max_pitch = kPitches - 1, p->hop = 4, p->band = 0;
}

// why a parameter set is refused; null: it is taken
const char* bp_internal_sync_bad_params(const bp_sync_params* p) {
  if (!p) return "null params";
  if (p->threshold_q < 0 || p->threshold_q > BP_CHORD_Q_ONE) return "threshold_q is not in 0 ... 1024";
  if (p->min_pitch < 0 || p->min_pitch > p->max_pitch || p->max_pitch >= kPitches) return "min_pitch / max_pitch are not 0 <= min_pitch <= max_pitch <= 87";
  if (p->hop < 1 || p->hop > BP_SYNC_MAX_HOP) return "hop is not in 1 ... 64";
  if (p->band < 0 || p->band > BP_SYNC_MAX_UNITS) return "band is not in 0 ... 8192";
  return p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0 ? "reserved must be 0" : nullptr;
}

int bp_sync_rows(const float* note_a, int64_t rows_a, const float* note_b, int64_t rows_b, const bp_sync_params* p, int32_t* path,
                 int64_t max_path, bp_sync_summary* summary) {
  if (rows_a < 0 || rows_b < 0 || (rows_a > 0 && !note_a) || (rows_b > 0 && !note_b) || !summary || bp_internal_sync_bad_params(p)) return BP_ERR_INVALID_ARG;
  const int64_t N = units_of(rows_a, p->hop), M = units_of(rows_b, p->hop);
  if (N > BP_SYNC_MAX_UNITS || M > BP_SYNC_MAX_UNITS) return BP_ERR_INVALID_ARG;
  const int64_t room = N > 0 && M > 0 ? N + M - 1 : 0;
  if (max_path < room || (max_path > 0 && !path)) return BP_ERR_INVALID_ARG;
  *summary = bp_sync_summary{0, (int32_t)N, (int32_t)M, 0, 0, 0};
  for (int64_t e = 0; e < 2 * room; ++e) path[e] = -1;
  std::vector<uint8_t> xa, xb;
  if (!features(note_a, rows_a, p, xa) || !features(note_b, rows_b, p, xb)) {
    summary->status = 1;
    return BP_OK;
  }
  if (room == 0) {
    summary->status = 2;
    return BP_OK;
  }
  const int64_t widest = (N > M ? N : M) - 1;
  auto admissible = [&](int64_t i, int64_t j) {
    if (p->band == 0) return true;
    const int64_t off = i * (M - 1) - j * (N - 1);
    return (off < 0 ? -off : off) <= (int64_t)p->band * widest;
  };
  // the recurrence: two rows of D, and of every cell where it came from (0 diagonal, 1 (i-1, j), 2 (i, j-1))
  std::vector<int32_t> above((size_t)M, kUnreachable), row((size_t)M, kUnreachable);
  std::vector<uint8_t> from((size_t)(N * M), 0);
  for (int64_t i = 0; i < N; ++i) {
    for (int64_t j = 0; j < M; ++j) {
      int32_t g = 0;
      for (int k = 0; k < kClasses; ++k) g += (int32_t)xa[(size_t)i * kClasses + k] * (int32_t)xb[(size_t)j * kClasses + k];
      int32_t best = kUnreachable;
      uint8_t came = 0;
      if (i == 0 && j == 0) {
        best = 2 * g;
      } else if (admissible(i, j)) {
        if (i > 0 && j > 0 && above[(size_t)j - 1] >= 0) best = above[(size_t)j - 1] + 2 * g, came = 0;
        if (i > 0 && above[(size_t)j] >= 0 && above[(size_t)j] + g > best) best = above[(size_t)j] + g, came = 1;
        if (j > 0 && row[(size_t)j - 1] >= 0 && row[(size_t)j - 1] + g > best) best = row[(size_t)j - 1] + g, came = 2;
      }
      row[(size_t)j] = best, from[(size_t)(i * M + j)] = came;
    }
    above.swap(row);
  }
  const int32_t total = above[(size_t)M - 1];
  if (total < 0) {  // (no band does this: the header's staircase)
    summary->status = 2;
    return BP_OK;
  }
  // the path, walked back into the end of the region and moved to its front
  int64_t i = N - 1, j = M - 1, at = room;
  for (;;) {
    --at;
    path[2 * at] = (int32_t)i, path[2 * at + 1] = (int32_t)j;
    if (i == 0 && j == 0) break;
    const uint8_t came = from[(size_t)(i * M + j)];
    if (came != 2) --i;
    if (came != 1) --j;
  }
  const int64_t n_path = room - at;
  for (int64_t e = 0; e < 2 * n_path; ++e) path[e] = path[2 * at + e];
  for (int64_t e = 2 * n_path; e < 2 * room; ++e) path[e] = -1;
  summary->n_path = (int32_t)n_path, summary->total = total;
  return BP_OK;
}

}  // extern "C"
