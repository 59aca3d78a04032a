// The chord and key checker (csrc/chord_host.cpp: no device) over seeded random maps, tables, boundaries and malformed inputs
// as a program of its own: tests/test_chord_cpu.py builds it plain and with the host sanitizers (address, undefined) and asks
// both for the same line.  Every buffer is a heap block of exactly the size the call may touch.  Usage: chord_host [cases]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/basic_pitch_amd_chord.h"

namespace {
uint64_t state = 0x9e3779b97f4a7c15ull;
uint32_t draw(uint32_t n) {  // 0 ... n - 1
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33) % n;
}
int32_t signed_entry() { return (int32_t)draw(2 * BP_CHORD_MAX_WEIGHT + 1) - BP_CHORD_MAX_WEIGHT; }
}  // namespace

int main(int argc, char** argv) {
  const int cases = argc > 1 ? std::atoi(argv[1]) : 200;
  const int64_t rows_of[8] = {0, 1, 2, 31, 65, 130, 300, 1100};
  const int states_of[6] = {1, 2, 25, 49, 61, 64};
  long long decoded = 0, flagged = 0, silent = 0, refused = 0, changes = 0, units = 0;
  uint64_t labels_sum = 0;
  int64_t scores = 0, keys = 0;
  for (int c = 0; c < cases; ++c) {
    const int64_t rows = rows_of[draw(8)];
    std::vector<float> note((size_t)(rows * BP_CHORD_PITCHES));
    const int kind = (int)draw(4);  // a thousand levels, eighths on stretches, runs of triads, silence
    for (size_t i = 0; i < note.size(); ++i) {
      const size_t t = i / BP_CHORD_PITCHES, q = i % BP_CHORD_PITCHES;
      if (kind == 0) note[i] = ((float)draw(1101) - 50.0f) / 1000.0f;
      if (kind == 1) note[i] = (float)((t / 7 + q % 12) % 9) / 8.0f;
      if (kind == 2) note[i] = (q + 9) % 12 == (t / 10) % 12 || (q + 9) % 12 == (t / 10 + 4) % 12 || (q + 9) % 12 == (t / 10 + 7) % 12 ? 0.9f : 0.0f;
      if (kind == 3) note[i] = 0.0f;
    }
    if (rows > 0 && draw(10) == 0) {
      const float odd[3] = {std::numeric_limits<float>::quiet_NaN(), -std::numeric_limits<float>::infinity(),
                            std::numeric_limits<float>::infinity()};
      note[draw((uint32_t)note.size())] = odd[draw(3)];
    }
    bp_chord_params p;
    bp_chord_params_default(&p);
    p.threshold_q = (int32_t)draw(4) * 128, p.switch_penalty = (int32_t)(draw(3) == 0 ? draw(BP_CHORD_MAX_PENALTY + 1) : draw(200));
    p.min_pitch = (int32_t)draw(40), p.max_pitch = p.min_pitch + (int32_t)draw((uint32_t)(BP_CHORD_PITCHES - p.min_pitch));
    const int table = (int)draw(5);
    if (table < 3 && bp_chord_templates(table, &p) != BP_OK) return 1;
    if (table >= 3) {  // a random signed table
      p.n_states = states_of[draw(6)];
      for (int s = 0; s < p.n_states; ++s) {
        p.bias[s] = signed_entry();
        for (int k = 0; k < BP_CHORD_CLASSES; ++k) p.weights[s][k] = signed_entry();
      }
      for (int k = 0; k < 2 * BP_CHORD_CLASSES; ++k) p.key_profile[k / BP_CHORD_CLASSES][k % BP_CHORD_CLASSES] = signed_entry();
    }
    // boundaries: none, every frame, or irregular
    std::vector<int32_t> bounds;
    const int how = (int)draw(3);
    for (int64_t b = 1; b < rows; ++b)
      if (how == 1 || (how == 2 && draw(6) == 0)) bounds.push_back((int32_t)b);
    std::vector<uint8_t> labels((size_t)rows, 200);  // exactly the rows
    bp_chord_summary s{-7, -7, -7, -7, -7, -7};
    // the refusals first: each leaves the outputs alone
    {
      bp_chord_params q = p;
      const int which = (int)draw(8);
      if (which == 0) q.threshold_q = BP_CHORD_Q_ONE + 1;
      if (which == 1) q.n_states = 0;
      if (which == 2) q.n_states = BP_CHORD_MAX_STATES + 1;
      if (which == 3) q.switch_penalty = -1;
      if (which == 4) q.weights[draw(BP_CHORD_MAX_STATES)][draw(BP_CHORD_CLASSES)] = 1025;
      if (which == 5) q.reserved[draw(3)] = 1;
      if (which == 6) q.max_pitch = BP_CHORD_PITCHES;
      if (which == 7) q.key_profile[draw(2)][draw(BP_CHORD_CLASSES)] = -1025;
      if (bp_chord_rows(note.data(), rows, &q, bounds.data(), (int64_t)bounds.size(), labels.data(), rows, &s) != BP_ERR_INVALID_ARG) return 2;
      ++refused;
      if (rows > 0) {
        if (bp_chord_rows(note.data(), rows, &p, bounds.data(), (int64_t)bounds.size(), labels.data(), rows - 1, &s) != BP_ERR_INVALID_ARG) return 4;
        ++refused;
        std::vector<int32_t> bad(bounds);
        bad.push_back(draw(2) ? (int32_t)rows : (bad.empty() ? 0 : bad.back()));  // at the end of the rows, or not ascending
        if (bp_chord_rows(note.data(), rows, &p, bad.data(), (int64_t)bad.size(), labels.data(), rows, &s) != BP_ERR_INVALID_ARG) return 5;
        ++refused;
      }
      if (s.status != -7 || s.score != -7) return 3;
      for (uint8_t l : labels)
        if (l != 200) return 3;
    }
    if (bp_chord_rows(rows ? note.data() : nullptr, rows, &p, bounds.empty() ? nullptr : bounds.data(), (int64_t)bounds.size(),
                      rows ? labels.data() : nullptr, rows, &s) != BP_OK)
      return 6;
    if (s.status == 0) {
      ++decoded;
      const int64_t n_units = bounds.empty() ? rows : (int64_t)bounds.size() + 1;
      if (s.key < 0 || s.key > 23 || s.n_units != n_units || s.n_changes < 0 || s.n_changes >= n_units) return 8;
      int64_t seen = 0;
      for (int64_t t = 0; t < rows; ++t) {
        if (labels[(size_t)t] >= p.n_states) return 9;
        if (t && labels[(size_t)t] != labels[(size_t)t - 1]) ++seen;
        labels_sum += (uint64_t)labels[(size_t)t] * (uint64_t)(t + 1);
      }
      if (seen != s.n_changes) return 10;  // (the labels change where the units' states do)
      changes += s.n_changes, units += s.n_units, scores += s.score % 1000003, keys += s.key;
    } else {
      flagged += s.status == 1, silent += s.status == 2;
      if (s.key != -1 || s.n_units != 0 || s.n_changes != 0 || s.score != 0 || s.key_score != 0) return 13;
      for (uint8_t l : labels)
        if (l != 0) return 14;
    }
  }
  std::printf("chord %d cases: decoded %lld flagged %lld silent %lld refused %lld units %lld changes %lld keys %lld labels %llu scores %lld\n",
              cases, decoded, flagged, silent, refused, units, changes, (long long)keys, (unsigned long long)labels_sum, (long long)scores);
  return 0;
}
