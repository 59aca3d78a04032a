// The melody checkers (csrc/melody_host.cpp, with note_score_host.cpp and note_decode.cpp: no device) over seeded random maps
// as a program of its own: tests/test_melody_cpu.py builds it plain and with the host sanitizers (address, undefined) and asks
// both for the same line.  Usage: melody_host [cases]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/basic_pitch_amd_melody.h"

namespace {
uint64_t state = 0x9e3779b97f4a7c15ull;
uint32_t draw(uint32_t n) {  // 0 ... n - 1
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33) % n;
}
}  // namespace

int main(int argc, char** argv) {
  const int cases = argc > 1 ? std::atoi(argv[1]) : 200;
  const int64_t rows_of[6] = {0, 1, 2, 9, 65, 173};
  const double tolerances[4] = {0.0, 30.0, 50.0, 100.0};
  long long voiced = 0, unvoiced = 0, flagged = 0, refused = 0, jumps = 0;
  uint64_t pitch_bits = 0;
  bp_melody_score sum{0, 0, 0, 0, 0, 0};
  for (int c = 0; c < cases; ++c) {
    const int64_t rows = rows_of[draw(6)];
    std::vector<float> map((size_t)(rows * BP_MP_BINS));
    const bool eighths = draw(2) != 0;  // (ties everywhere) or a thousand levels
    for (float& v : map) v = eighths ? (float)draw(9) / 8.0f : (float)draw(1000) / 1000.0f;
    if (rows > 0 && draw(10) == 0) {
      const float bad[3] = {std::numeric_limits<float>::quiet_NaN(), -std::numeric_limits<float>::infinity(), 65537.0f};
      map[draw((uint32_t)map.size())] = bad[draw(3)];
    }
    bp_melody_params p;
    bp_melody_params_default(&p);
    p.threshold = (float)draw(11) / 8.0f, p.jump_penalty = (float)draw(4) / 8.0f, p.voicing_penalty = (float)draw(5) / 8.0f;
    p.max_jump = (int32_t)draw(BP_MELODY_MAX_JUMP + 1);
    p.min_bin = (int32_t)draw(264), p.max_bin = p.min_bin + (int32_t)draw((uint32_t)(264 - p.min_bin));
    // exactly the room asked for, a canary behind it
    std::vector<bp_melody_point> points((size_t)rows + 1);
    std::memset(&points[(size_t)rows], 0x5a, sizeof(bp_melody_point));
    int status = -1;
    if (bp_melody_rows(map.data(), rows, &p, points.data(), rows, &status) != BP_OK || status < 0 || status > 1) return 1;
    const unsigned char* canary = reinterpret_cast<const unsigned char*>(&points[(size_t)rows]);
    for (size_t i = 0; i < sizeof(bp_melody_point); ++i)
      if (canary[i] != 0x5a) return 2;
    flagged += status;
    for (int64_t t = 0; t < rows; ++t) {
      const bp_melody_point& q = points[(size_t)t];
      if (q.bin < 0) {
        ++unvoiced;
        continue;
      }
      if (status != 0 || q.bin < p.min_bin || q.bin > p.max_bin || q.salience != map[(size_t)(t * BP_MP_BINS + q.bin)]) return 3;
      ++voiced;
      if (t > 0 && points[(size_t)t - 1].bin >= 0) {
        const int32_t j = q.bin - points[(size_t)t - 1].bin;
        if (j > p.max_jump || -j > p.max_jump) return 4;
        jumps += j != 0;
      }
      uint64_t bits;
      std::memcpy(&bits, &q.pitch_midi, 8);
      pitch_bits ^= bits + (uint64_t)t;
    }
    // the counts against a reference that follows the track, an octave off now and then
    std::vector<double> ref((size_t)rows);
    for (int64_t t = 0; t < rows; ++t) {
      const bp_melody_point& q = points[(size_t)t];
      const uint32_t kind = draw(8);
      ref[(size_t)t] = q.bin < 0 ? (kind == 0 ? 60.0 : 0.0) : kind == 1 ? 0.0 : q.pitch_midi + (kind == 2 ? 12.0 : kind == 3 ? 0.5 : 0.0);
    }
    bp_score_params sp;
    bp_score_params_default(&sp);
    sp.pitch_tolerance_cents = tolerances[draw(4)], sp.strict = (int32_t)draw(2);
    bp_melody_score out{};
    if (bp_score_melody_frames(points.data(), ref.data(), rows, &sp, &out) != BP_OK) return 5;
    sum.n_frames += out.n_frames, sum.ref_voiced += out.ref_voiced, sum.est_voiced += out.est_voiced;
    sum.both_voiced += out.both_voiced, sum.pitch_ok += out.pitch_ok, sum.chroma_ok += out.chroma_ok;
    // ... and what is refused: too little room, a malformed set, a negative reference pitch
    if (rows > 0) refused += bp_melody_rows(map.data(), rows, &p, points.data(), rows - 1, &status) == BP_ERR_INVALID_ARG;
    p.max_jump = BP_MELODY_MAX_JUMP + 1;
    refused += bp_melody_rows(map.data(), rows, &p, points.data(), rows, &status) == BP_ERR_INVALID_ARG;
    if (rows > 0) {
      ref[draw((uint32_t)rows)] = -1.0;
      refused += bp_score_melody_frames(points.data(), ref.data(), rows, &sp, &out) == BP_ERR_INVALID_ARG;
    }
  }
  std::printf("melody %d cases: voiced %lld unvoiced %lld jumps %lld pitch_bits %016llx flagged %lld refused %lld n_frames %lld ref_voiced %lld "
              "est_voiced %lld both_voiced %lld pitch_ok %lld chroma_ok %lld\n",
              cases, voiced, unvoiced, jumps, (unsigned long long)pitch_bits, flagged, refused, (long long)sum.n_frames, (long long)sum.ref_voiced,
              (long long)sum.est_voiced, (long long)sum.both_voiced, (long long)sum.pitch_ok, (long long)sum.chroma_ok);
  return 0;
}
