// Forced alignment on the host (include/basic_pitch_amd_align.h): bp_align_rows, the checker the device kernels (align.hip)
// are held to, and the validation of parameters and states that the device entry points (clips_align.hip) use instead of a
// copy.  Device-free: links with plain g++.
//
// The recurrence is the header's in int64, with "unreachable" a flag beside the number, not a sentinel inside it.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/basic_pitch_amd_align.h"

namespace {

constexpr int kPitches = BP_ALIGN_PITCHES;

inline int quantise(float x) { return (int)floorf(fminf(fmaxf(x, 0.0f), 1.0f) * 1024.0f + 0.5f); }
inline bool has(const uint64_t* m, int p) { return (m[p >> 6] >> (p & 63)) & 1; }

}  // namespace

extern "C" {

void bp_align_params_default(bp_align_params* p) {
  if (p) *p = bp_align_params{307, 2, {0, 0}};
}

// why a parameter set is refused; null: it is taken
const char* bp_internal_align_bad_params(const bp_align_params* p) {
  if (!p) return "null params";
  if (p->threshold_q < 0 || p->threshold_q > BP_ALIGN_Q_ONE) return "threshold_q is not in 0 ... 1024";
  if (p->onset_weight < 0 || p->onset_weight > BP_ALIGN_MAX_ONSET_WEIGHT) return "onset_weight is not in 0 ... 16";
  return p->reserved[0] != 0 || p->reserved[1] != 0 ? "reserved must be 0" : nullptr;
}

// why the first malformed state of states[0 ... n) is refused, *index its index; null: all are taken
const char* bp_internal_align_bad_states(const bp_align_state* states, int64_t n, int64_t* index) {
  for (int64_t j = 0; j < n; ++j) {
    const bp_align_state& s = states[j];
    const char* why = nullptr;
    if (s.active[1] >> (kPitches - 64) || s.begins[1] >> (kPitches - 64))
      why = "a bit at or above 88 is set";
    else if ((s.begins[0] & ~s.active[0]) || (s.begins[1] & ~s.active[1]))
      why = "begins is not a subset of active";
    else if (s.earliest < 0)
      why = "earliest is negative";
    else if (s.earliest > s.latest)
      why = "earliest is above latest";
    if (why) {
      if (index) *index = j;
      return why;
    }
  }
  return nullptr;
}

int bp_align_rows(const float* note, const float* onset, int64_t rows, const bp_align_state* states, int64_t n_states,
                  const bp_align_params* p, int32_t* first_frame, int64_t max_states, int64_t* total, int* status) {
  if (rows < 0 || n_states < 0 || max_states < n_states || rows > INT32_MAX || n_states > BP_ALIGN_MAX_STATES ||
      (rows > 0 && (!note || !onset || n_states == 0)) || (n_states > 0 && (!states || !first_frame)) || !total || !status ||
      bp_internal_align_bad_params(p) || bp_internal_align_bad_states(states, n_states, nullptr))
    return BP_ERR_INVALID_ARG;
  const int64_t S = n_states;
  *total = 0, *status = 0;
  for (int64_t j = 0; j < S; ++j) first_frame[j] = -1;
  for (int64_t i = 0; i < rows * kPitches; ++i)
    if (std::isnan(note[i]) || std::isnan(onset[i])) {
      *status = 1;
      return BP_OK;
    }
  if (S == 0) return BP_OK;
  if (S > rows) {  // (rows == 0 among them)
    *status = 2;
    return BP_OK;
  }
  // the pitches of every state, and what the threshold takes from it
  std::vector<uint8_t> act((size_t)S * kPitches), beg((size_t)S * kPitches);
  std::vector<int32_t> n_act((size_t)S), n_beg((size_t)S), off((size_t)S);
  for (int64_t j = 0; j < S; ++j) {
    for (int q = 0; q < kPitches; ++q) {
      if (has(states[j].active, q)) act[(size_t)j * kPitches + n_act[(size_t)j]++] = (uint8_t)q;
      if (has(states[j].begins, q)) beg[(size_t)j * kPitches + n_beg[(size_t)j]++] = (uint8_t)q;
    }
    off[(size_t)j] = p->threshold_q * n_act[(size_t)j];
  }
  const size_t words = (size_t)(S + 63) / 64;
  std::vector<uint64_t> entered((size_t)rows * words, 0);  // one bit per cell: the state was entered at this frame
  std::vector<int64_t> D((size_t)S, 0), next((size_t)S, 0);
  std::vector<uint8_t> ok((size_t)S, 0), next_ok((size_t)S, 0);
  int32_t qn[kPitches], qo[kPitches];
  for (int64_t t = 0; t < rows; ++t) {
    for (int q = 0; q < kPitches; ++q) qn[q] = quantise(note[t * kPitches + q]), qo[q] = quantise(onset[t * kPitches + q]);
    // (a state beyond frame t cannot be reached, one more than rows - 1 - t before the end cannot reach it: both are decided
    // by the recurrence itself, nothing is cut here)
    const int64_t last = t < S - 1 ? t : S - 1;
    for (int64_t j = 0; j <= last; ++j) {
      int32_t g = -off[(size_t)j], b = 0;
      const uint8_t* a = &act[(size_t)j * kPitches];
      for (int k = 0; k < n_act[(size_t)j]; ++k) g += qn[a[k]];
      const uint8_t* e = &beg[(size_t)j * kPitches];
      for (int k = 0; k < n_beg[(size_t)j]; ++k) b += qo[e[k]];
      b *= p->onset_weight;
      if (t == 0) {
        next_ok[0] = states[0].earliest <= 0;
        next[0] = (int64_t)g + b;
        continue;
      }
      const bool can_stay = ok[(size_t)j] != 0;
      const bool can_enter = j >= 1 && ok[(size_t)j - 1] && states[j].earliest <= t && t <= states[j].latest;
      const int64_t stay = D[(size_t)j] + g, enter = j >= 1 ? D[(size_t)j - 1] + g + b : 0;
      const bool take = can_enter && (!can_stay || enter > stay);
      next_ok[(size_t)j] = can_stay || can_enter;
      next[(size_t)j] = take ? enter : stay;
      if (take) entered[(size_t)t * words + (size_t)(j >> 6)] |= 1ull << (j & 63);
    }
    for (int64_t j = last + 1; j < S && j <= t + 1; ++j) next_ok[(size_t)j] = 0;
    D.swap(next), ok.swap(next_ok);
  }
  if (!ok[(size_t)S - 1]) {
    *status = 2;
    return BP_OK;
  }
  *total = D[(size_t)S - 1];
  int64_t j = S - 1;
  for (int64_t t = rows - 1; t > 0 && j > 0; --t)
    if ((entered[(size_t)t * words + (size_t)(j >> 6)] >> (j & 63)) & 1) first_frame[j--] = (int32_t)t;
  first_frame[0] = 0;  // (a reachable end has walked back to state 0: every entered state was entered from a reachable one)
  return BP_OK;
}

}  // extern "C"
