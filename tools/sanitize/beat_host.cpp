// The tempo and beat checker (csrc/beat_host.cpp: no device) over seeded random maps, parameter sets and malformed inputs as a
// program of its own: tests/test_beat_cpu.py builds it plain and with the host sanitizers (address, undefined) and asks both
// for the same line.  Usage: beat_host [cases]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/basic_pitch_amd_beat.h"

namespace {
uint64_t state = 0x9e3779b97f4a7c15ull;
uint32_t draw(uint32_t n) {  // 0 ... n - 1
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33) % n;
}
}  // namespace

int main(int argc, char** argv) {
  const int cases = argc > 1 ? std::atoi(argv[1]) : 200;
  const int64_t rows_of[8] = {0, 1, 22, 65, 130, 173, 300, 1100};
  long long decoded = 0, flagged = 0, no_pulse = 0, refused = 0, n_beats = 0;
  uint64_t frames = 0;
  int64_t scores = 0, periods = 0;
  for (int c = 0; c < cases; ++c) {
    const int64_t rows = rows_of[draw(8)];
    std::vector<float> onset((size_t)(rows * BP_BEAT_PITCHES));
    const int kind = (int)draw(4);  // a thousand levels, eighths on few pitches, a pulse train, silence
    const uint32_t period = 20 + draw(60);
    for (size_t i = 0; i < onset.size(); ++i) {
      const size_t t = i / BP_BEAT_PITCHES, q = i % BP_BEAT_PITCHES;
      if (kind == 0) onset[i] = ((float)draw(1101) - 50.0f) / 1000.0f;
      if (kind == 1) onset[i] = q % 11 == 0 && draw(3) == 0 ? (float)draw(9) / 8.0f : 0.0f;
      if (kind == 2) onset[i] = t % period == 0 && q % 5 == 0 ? 0.9f : (float)draw(200) / 1000.0f;
      if (kind == 3) onset[i] = 0.0f;
    }
    if (rows > 0 && draw(10) == 0) {
      const float odd[3] = {std::numeric_limits<float>::quiet_NaN(), -std::numeric_limits<float>::infinity(),
                            std::numeric_limits<float>::infinity()};
      onset[draw((uint32_t)onset.size())] = odd[draw(3)];
    }
    bp_beat_params p;
    bp_beat_params_default(&p);
    p.threshold_q = (int32_t)draw(4) * 128,p.tightness = (int32_t)(draw(3) == 0 ? draw(BP_BEAT_MAX_TIGHTNESS + 1) : draw(9));
    p.lag_min = 2 + (int32_t)draw(40), p.lag_max = p.lag_min + (int32_t)draw((uint32_t)(BP_BEAT_MAX_LAG - p.lag_min + 1));
    p.min_pitch = (int32_t)draw(40), p.max_pitch = p.min_pitch + (int32_t)draw((uint32_t)(BP_BEAT_PITCHES - p.min_pitch));
    if (draw(4) == 0 && bp_beat_prior(40.0 + draw(200), 0.25 + draw(8) / 4.0, p.prior) != BP_OK) return 1;
    const int64_t cap = bp_beats_capacity(rows, p.lag_min);
    if (cap < 0) return 1;
    std::vector<int32_t> beats((size_t)cap + 1, 12345);
    bp_beat_summary s{-1, -1, -1, -1, -1.0};
    // the refusals first: each leaves the outputs alone
    {
      bp_beat_params q = p;
      const int which = (int)draw(7);
      if (which == 0) q.threshold_q = BP_BEAT_Q_ONE + 1;
      if (which == 1) q.lag_min = 1;
      if (which == 2) q.lag_max = BP_BEAT_MAX_LAG + 1;
      if (which == 3) q.tightness = -1;
      if (which == 4) q.prior[draw(BP_BEAT_MAX_LAG + 1)] = 1025;
      if (which == 5) q.reserved_tail = 1;
      if (which == 6) q.max_pitch = BP_BEAT_PITCHES;
      if (bp_beat_rows(onset.data(), rows, &q, beats.data(), cap, &s) != BP_ERR_INVALID_ARG) return 2;
      if (s.status != -1 || s.n_beats != -1 || beats[0] != 12345) return 3;
      ++refused;
      if (cap > 0) {
        if (bp_beat_rows(onset.data(), rows, &p, beats.data(), cap - 1, &s) != BP_ERR_INVALID_ARG) return 4;
        ++refused;
      }
    }
    if (bp_beat_rows(rows ? onset.data() : nullptr, rows, &p, beats.data(), cap, &s) != BP_OK) return 6;
    if (beats[(size_t)cap] != 12345) return 7;  // nothing beyond the room is written
    if (s.status == 0) {
      ++decoded;
      const int64_t last_lag = p.lag_max < rows - 1 ? p.lag_max : rows - 1;
      if (s.period < p.lag_min || s.period > last_lag || s.n_beats < 1 || s.n_beats > cap || s.score <= 0) return 8;
      if (!(s.period_refined > s.period - 1.0 && s.period_refined < s.period + 1.0)) return 9;
      const int64_t dmin = s.period / 2 > 1 ? s.period / 2 : 1, dmax = 2 * (int64_t)s.period;
      for (int64_t j = 0; j < s.n_beats; ++j) {
        if (beats[(size_t)j] < 0 || beats[(size_t)j] >= rows) return 10;
        if (j && (beats[(size_t)j] - beats[(size_t)j - 1] < dmin || beats[(size_t)j] - beats[(size_t)j - 1] > dmax)) return 11;
        frames += (uint64_t)beats[(size_t)j] * (uint64_t)(j + 1);
      }
      if (beats[(size_t)s.n_beats - 1] < rows - s.period) return 12;  // the last beat lies in the last P rows
      n_beats += s.n_beats, scores += s.score % 1000003, periods += s.period;
    } else {
      flagged += s.status == 1, no_pulse += s.status == 2;
      if (s.period != 0 || s.n_beats != 0 || s.score != 0 || s.period_refined != 0.0 || beats[0] != 12345) return 13;
    }
  }
  std::printf("beat %d cases: decoded %lld flagged %lld silent %lld refused %lld beats %lld periods %lld frames %llu scores %lld\n", cases,
              decoded, flagged, no_pulse, refused, n_beats, (long long)periods, (unsigned long long)frames, (long long)scores);
  return 0;
}
