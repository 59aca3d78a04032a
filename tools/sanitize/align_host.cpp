// The alignment checker (csrc/align_host.cpp: no device) over seeded random maps, state lists and malformed inputs as a program
// of its own: tests/test_align_cpu.py builds it plain and with the host sanitizers (address, undefined) and asks both for the
// same line.  Usage: align_host [cases]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/basic_pitch_amd_align.h"

namespace {
uint64_t state = 0x9e3779b97f4a7c15ull;
uint32_t draw(uint32_t n) {  // 0 ... n - 1
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33) % n;
}
void set_bit(uint64_t* m, uint32_t p) { m[p >> 6] |= 1ull << (p & 63); }
}  // namespace

int main(int argc, char** argv) {
  const int cases = argc > 1 ? std::atoi(argv[1]) : 200;
  const int64_t rows_of[7] = {0, 1, 2, 9, 65, 173, 300};
  long long aligned = 0, flagged = 0, infeasible = 0, refused = 0, n_states = 0;
  uint64_t frames = 0;
  int64_t totals = 0;
  for (int c = 0; c < cases; ++c) {
    const int64_t rows = rows_of[draw(7)];
    std::vector<float> note((size_t)(rows * BP_ALIGN_PITCHES)), onset(note.size());
    const bool eighths = draw(2) != 0;  // (ties everywhere) or a thousand levels, some beyond 0 ... 1
    for (std::vector<float>* m : {&note, &onset})
      for (float& v : *m) v = eighths ? (float)draw(9) / 8.0f : ((float)draw(1101) - 50.0f) / 1000.0f;
    if (rows > 0 && draw(10) == 0) {
      const float odd[3] = {std::numeric_limits<float>::quiet_NaN(), -std::numeric_limits<float>::infinity(),
                            std::numeric_limits<float>::infinity()};
      (draw(2) ? note : onset)[draw((uint32_t)note.size())] = odd[draw(3)];
    }
    // mostly fewer states than rows, sometimes more (infeasible), sometimes none
    const int64_t S = rows == 0 ? draw(3) : draw(8) == 0 ? rows + 1 + draw(3) : 1 + draw((uint32_t)(rows < 80 ? rows : 80));
    std::vector<bp_align_state> st((size_t)S);
    for (int64_t j = 0; j < S; ++j) {
      st[(size_t)j] = bp_align_state{{0, 0}, {0, 0}, 0, INT32_MAX};
      for (uint32_t k = draw(5); k > 0; --k) {
        const uint32_t p = draw(BP_ALIGN_PITCHES);
        set_bit(st[(size_t)j].active, p);
        if (draw(2)) set_bit(st[(size_t)j].begins, p);
      }
      if (j > 0 && rows >= S && draw(4) == 0) {  // a window around an even spread, now and then too tight to be met
        const int32_t mid = (int32_t)(j * rows / S);
        st[(size_t)j].earliest = mid > 3 ? mid - (int32_t)draw(4) : 0;
        st[(size_t)j].latest = mid + (int32_t)draw(4);
      }
    }
    bp_align_params p;
    bp_align_params_default(&p);
    p.threshold_q = (int32_t)draw(9) * 128, p.onset_weight = (int32_t)draw(BP_ALIGN_MAX_ONSET_WEIGHT + 1);
    std::vector<int32_t> ff((size_t)S + 1, 12345);
    int64_t total = -1;
    int status = -1;
    // the refusals first: each leaves the outputs alone
    {
      bp_align_params q = p;
      const int which = (int)draw(4);
      if (which == 0) q.threshold_q = BP_ALIGN_Q_ONE + 1;
      if (which == 1) q.onset_weight = -1;
      if (which == 2) q.reserved[1] = 1;
      bool bad_state = false;
      std::vector<bp_align_state> broken = st;
      if (which == 3 && S > 0) {
        bp_align_state& b = broken[draw((uint32_t)S)];
        const int how = (int)draw(4);
        if (how == 0) b.active[1] |= 1ull << (24 + draw(40));
        if (how == 1) b.begins[0] = ~b.active[0];
        if (how == 2) b.earliest = -1 - (int32_t)draw(5);
        if (how == 3) b.earliest = 7, b.latest = 6;
        bad_state = !(how == 1 && b.begins[0] == 0);
      }
      if (which < 3 || bad_state) {
        if (bp_align_rows(note.data(), onset.data(), rows, broken.data(), S, &q, ff.data(), S, &total, &status) != BP_ERR_INVALID_ARG) return 2;
        if (total != -1 || status != -1 || ff[0] != 12345) return 3;
        ++refused;
      }
      if (S > 0 && bp_align_rows(note.data(), onset.data(), rows, st.data(), S, &p, ff.data(), S - 1, &total, &status) != BP_ERR_INVALID_ARG) return 4;
      ++refused;
    }
    if (rows > 0 && S == 0) {
      if (bp_align_rows(note.data(), onset.data(), rows, st.data(), S, &p, ff.data(), S, &total, &status) != BP_ERR_INVALID_ARG) return 5;
      ++refused;
      continue;
    }
    if (bp_align_rows(note.data(), onset.data(), rows, st.data(), S, &p, ff.data(), S, &total, &status) != BP_OK) return 6;
    if (ff[(size_t)S] != 12345) return 7;  // nothing beyond the states is written
    n_states += S;
    if (status == 0) {
      if (S > 0) ++aligned;
      totals += total;
      for (int64_t j = 0; j < S; ++j) {
        if (ff[(size_t)j] < (j ? ff[(size_t)j - 1] + 1 : 0) || ff[(size_t)j] >= rows) return 8;  // a monotone path inside the rows
        frames += (uint64_t)ff[(size_t)j] * (uint64_t)(j + 1);
      }
    } else {
      flagged += status == 1, infeasible += status == 2;
      for (int64_t j = 0; j < S; ++j)
        if (ff[(size_t)j] != -1) return 9;
      if (total != 0) return 10;
    }
  }
  std::printf("align %d cases: aligned %lld flagged %lld infeasible %lld refused %lld states %lld frames %llu totals %lld\n", cases, aligned,
              flagged, infeasible, refused, n_states, (unsigned long long)frames, (long long)totals);
  return 0;
}
