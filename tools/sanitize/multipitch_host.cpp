// The multi-pitch checkers (csrc/multipitch_host.cpp, with note_frames_host.cpp, note_score_host.cpp and note_decode.cpp: no
// device) over seeded random maps as a program of its own: tests/test_multipitch_cpu.py builds it plain and with the host
// sanitizers (address, undefined) and asks both for the same line.  Usage: multipitch_host [cases]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/basic_pitch_amd_multipitch.h"

extern "C" double bp_internal_frame_time(int64_t frame);

namespace {
uint64_t state = 0x9e3779b97f4a7c15ull;
uint32_t draw(uint32_t n) {  // 0 ... n - 1
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33) % n;
}
}  // namespace

int main(int argc, char** argv) {
  const int cases = argc > 1 ? std::atoi(argv[1]) : 200;
  const int64_t rows_of[6] = {0, 1, 2, 65, 172, 173};
  const double tolerances[4] = {0.0, 30.0, 50.0, 100.0};
  long long n_points = 0, flagged = 0, refused = 0, repeated = 0;
  uint64_t pitch_bits = 0;
  bp_frame_score sum{0, 0, 0, 0, 0};
  for (int c = 0; c < cases; ++c) {
    const int64_t rows = rows_of[draw(6)];
    std::vector<float> map((size_t)(rows * BP_MP_BINS));
    const bool sparse = draw(2) != 0;
    for (float& v : map) v = sparse && draw(8) ? 0.0f : (float)draw(1000) / 1000.0f;  // (plateaus of zeros; equal cells now and then)
    if (rows > 0 && draw(10) == 0) map[draw((uint32_t)map.size())] = draw(2) ? std::numeric_limits<float>::quiet_NaN() : std::numeric_limits<float>::infinity();
    bp_mp_params p;
    bp_mp_params_default(&p);
    p.threshold = (float)draw(100) / 100.0f - 0.1f;
    p.min_bin = 1 + (int32_t)draw(262), p.max_bin = p.min_bin + (int32_t)draw((uint32_t)(263 - p.min_bin));
    // the capacity protocol: without room first, then with exactly the room asked for, a canary behind it
    int64_t need = -1, got = -1;
    int status = -1, again = -1;
    const int rc0 = bp_multipitch_rows(map.data(), rows, &p, nullptr, 0, &need, &status);
    if (rc0 != BP_OK && need <= 0) return 1;
    refused += rc0 != BP_OK;
    std::vector<bp_f0_point> points((size_t)need + 1);
    std::memset(&points[(size_t)need], 0x5a, sizeof(bp_f0_point));
    if (bp_multipitch_rows(map.data(), rows, &p, points.data(), need, &got, &again) != BP_OK || got != need || again != status) return 2;
    const unsigned char* canary = reinterpret_cast<const unsigned char*>(&points[(size_t)need]);
    for (size_t i = 0; i < sizeof(bp_f0_point); ++i)
      if (canary[i] != 0x5a) return 3;
    repeated += rc0 != BP_OK;
    flagged += status;
    n_points += need;
    for (int64_t i = 0; i < need; ++i) {
      uint64_t bits;
      std::memcpy(&bits, &points[(size_t)i].pitch_midi, 8);
      pitch_bits ^= bits + (uint64_t)i;
    }
    // the frame-level counts of the points against refs some of which sit on a peak
    std::vector<bp_ref_note> ref(draw(8));
    for (bp_ref_note& r : ref) {
      const int64_t start = (int64_t)draw(200) - 10;
      r.start_s = bp_internal_frame_time(start), r.end_s = bp_internal_frame_time(start + draw(60));
      r.pitch_midi = need > 0 && draw(2) ? points[draw((uint32_t)need)].pitch_midi + (draw(2) ? 0.0 : 0.5) : 30.0 + draw(70);
    }
    bp_score_params sp;
    bp_score_params_default(&sp);
    sp.pitch_tolerance_cents = tolerances[draw(4)], sp.strict = (int32_t)draw(2);
    bp_frame_score out{};
    if (bp_score_f0_frames(points.data(), need, ref.data(), (int64_t)ref.size(), rows, &sp, &out) != BP_OK) return 4;
    sum.n_frames += out.n_frames, sum.ref_frames += out.ref_frames, sum.est_frames += out.est_frames;
    sum.true_pos += out.true_pos, sum.e_sub += out.e_sub;
    // ... and what is refused: a malformed set, a negative n_frames
    p.max_bin = 263;
    refused += bp_multipitch_rows(map.data(), rows, &p, points.data(), need, &got, &again) == BP_ERR_INVALID_ARG;
    refused += bp_score_f0_frames(points.data(), need, ref.data(), (int64_t)ref.size(), -1, &sp, &out) == BP_ERR_INVALID_ARG;
  }
  std::printf("multipitch %d cases: points %lld pitch_bits %016llx flagged %lld repeated %lld refused %lld n_frames %lld ref_frames %lld "
              "est_frames %lld true_pos %lld e_sub %lld\n",
              cases, n_points, (unsigned long long)pitch_bits, flagged, repeated, refused, (long long)sum.n_frames, (long long)sum.ref_frames,
              (long long)sum.est_frames, (long long)sum.true_pos, (long long)sum.e_sub);
  return 0;
}
