// The frame-level checker (csrc/note_frames_host.cpp, with note_score_host.cpp and note_decode.cpp: no device) over seeded
// random cases as a program of its own: tests/test_frame_score_cpu.py builds it plain and with the host sanitizers (address,
// undefined) and asks both for the same line.  Usage: frame_score_host [cases]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/basic_pitch_amd_frame_score.h"

extern "C" double bp_internal_frame_time(int64_t frame);

namespace {
uint64_t state = 0x9e3779b97f4a7c15ull;
uint32_t draw(uint32_t n) {  // 0 ... n - 1
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33) % n;
}
}  // namespace

int main(int argc, char** argv) {
  const int cases = argc > 1 ? std::atoi(argv[1]) : 300;
  const int64_t frames_of[6] = {150, 172, 173, 344, 345, 360};
  const double tolerances[5] = {0.0, 30.0, 50.0, 100.0, 120.0}, moved[5] = {0.0, 0.3, -0.3, 0.5, -0.5};
  bp_frame_score sum{0, 0, 0, 0, 0};
  int refused = 0;
  for (int c = 0; c < cases; ++c) {
    std::vector<bp_note_event> est(draw(12));  // (an empty side among them)
    std::vector<bp_ref_note> ref(draw(12));
    for (bp_note_event& e : est) {
      const int64_t start = 1 + draw(300);
      e = bp_note_event{};
      e.start_s = bp_internal_frame_time(start), e.end_s = bp_internal_frame_time(start + 3 + draw(58));
      e.pitch_midi = 58 + (int32_t)draw(6);
    }
    for (bp_ref_note& r : ref) {
      const int64_t start = (int64_t)draw(320) - 10;  // some before frame 0
      r.start_s = bp_internal_frame_time(start), r.end_s = bp_internal_frame_time(start + draw(61));  // (some of no length)
      r.pitch_midi = 58.0 + draw(6) + moved[draw(5)];
    }
    bp_score_params p;
    bp_score_params_default(&p);
    p.pitch_tolerance_cents = tolerances[draw(5)], p.strict = (int32_t)draw(2);
    bp_frame_score out{};
    const int rc = bp_score_note_frames(est.data(), (int64_t)est.size(), ref.data(), (int64_t)ref.size(), frames_of[draw(6)], &p, &out);
    if (rc != BP_OK) return 1;
    sum.n_frames += out.n_frames, sum.ref_frames += out.ref_frames, sum.est_frames += out.est_frames;
    sum.true_pos += out.true_pos, sum.e_sub += out.e_sub;
    // ... and what it refuses: a negative n_frames, a ref that ends before it starts
    refused += bp_score_note_frames(est.data(), (int64_t)est.size(), ref.data(), (int64_t)ref.size(), -1, &p, &out) == BP_ERR_INVALID_ARG;
    if (!ref.empty()) {
      ref[0].end_s = ref[0].start_s - 1.0;
      refused += bp_score_note_frames(est.data(), (int64_t)est.size(), ref.data(), (int64_t)ref.size(), 100, &p, &out) == BP_ERR_INVALID_ARG;
    }
  }
  std::printf("frame scores %d cases: n_frames %lld ref_frames %lld est_frames %lld true_pos %lld e_sub %lld refused %d\n", cases,
              (long long)sum.n_frames, (long long)sum.ref_frames, (long long)sum.est_frames, (long long)sum.true_pos, (long long)sum.e_sub,
              refused);
  return 0;
}
