// Frame-level scoring on the host (include/basic_pitch_amd_frame_score.h): bp_score_note_frames, the checker the device kernel
// (note_frames.hip) is held to and the route for the decodes a device call leaves, and the two functions of a ref and its
// segment alone that both share — the frames a note sounds on and the estimated pitches a ref hits — which the device reads
// from a table the host makes with them (clips_sweep.hip), so that the kernel compares integers alone.
//
// The predicates are the header's, in float64 and as written.  The frame time is strictly increasing, so the frames a note
// sounds on are one interval, found from a guess by steps with the very comparison of the definition.  Between two frames
// at which some note starts or ends the two sides of a frame do not change: the checker matches once per such stretch and
// multiplies by its length.  The matching is the greedy the header allows (refs in ascending pitch, each the lowest free estimated pitch
// it hits); the device does the same on a bit mask.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/basic_pitch_amd_frame_score.h"

#pragma clang fp contract(off)
#pragma clang fp reassociate(off)

extern "C" double bp_internal_frame_time(int64_t frame);  // note_decode.cpp
extern "C" const char* bp_internal_score_bad_params(const bp_score_params* p);  // note_score_host.cpp
extern "C" int64_t bp_internal_score_bad_ref(const bp_ref_note* refs, int64_t n);

namespace {

inline bool within(double d, double tol, bool strict) { return strict ? d < tol : d <= tol; }
inline bool hits(double ref_pitch, double est_pitch, const bp_score_params* p) {
  return within(100.0 * std::fabs(ref_pitch - est_pitch), p->pitch_tolerance_cents, p->strict != 0);
}

// the first frame of 0 ... n_frames - 1 whose time is >= t; n_frames: none.  time(fr) = fr * hop - offset * floor(fr / 172)
// lies less than one window offset (0.9 frames) above fr * (hop - offset / 172): a guess from that, then steps to the frame
// the definition's own comparison singles out — the time is strictly increasing, so there is one.
int64_t first_frame_at(double t, int64_t n_frames) {
  if (t != t) return n_frames;  // (an event's time may be anything: no frame's time is >= a NaN)
  const double hop = 256.0 / 22050.0, offset = hop * (172.0 - (43844.0 / 256.0)) + 0.0018;
  const double guess = t / (hop - offset / 172.0);
  int64_t fr = guess <= 0.0 ? 0 : (guess >= (double)n_frames ? n_frames : (int64_t)guess);
  while (fr > 0 && bp_internal_frame_time(fr - 1) >= t) --fr;
  while (fr < n_frames && bp_internal_frame_time(fr) < t) ++fr;
  return fr;
}

struct Span {
  int64_t f0, f1;  // sounds on f0 ... f1 - 1
  double pitch;
};

}  // namespace

extern "C" {

// the frames of 0 ... n_frames - 1 on which a note of [start_s, end_s) sounds: *f0 ... *f1 - 1 (none: *f0 == *f1)
void bp_internal_frame_interval(double start_s, double end_s, int64_t n_frames, int64_t* f0, int64_t* f1) {
  *f0 = first_frame_at(start_s, n_frames);
  *f1 = std::max(*f0, first_frame_at(end_s, n_frames));
}

// the estimated pitches of 21 ... 108 a ref hits, as note bins (pitch - 21): *lo ... *hi, one run around the bin nearest the
// ref because the distance, and with it the predicate's left side, never falls on the way out; none: *lo > *hi
void bp_internal_frame_pitch_range(const bp_ref_note* r, const bp_score_params* p, int32_t* lo, int32_t* hi) {
  *lo = 88, *hi = -1;
  const double nearest = std::rint(r->pitch_midi) - 21.0;
  const int32_t b = nearest <= 0.0 ? 0 : (nearest >= 87.0 ? 87 : (int32_t)nearest);
  if (!hits(r->pitch_midi, (double)(21 + b), p)) return;
  *lo = *hi = b;
  while (*lo > 0 && hits(r->pitch_midi, (double)(21 + *lo - 1), p)) --*lo;
  while (*hi < 87 && hits(r->pitch_midi, (double)(21 + *hi + 1), p)) ++*hi;
}

int bp_score_note_frames(const bp_note_event* est, int64_t n_est, const bp_ref_note* ref, int64_t n_ref, int64_t n_frames,
                         const bp_score_params* p, bp_frame_score* out) {
  if (!out || n_est < 0 || n_ref < 0 || n_frames < 0 || (n_est > 0 && !est) || (n_ref > 0 && !ref) || n_est > INT32_MAX ||
      n_ref > INT32_MAX)
    return BP_ERR_INVALID_ARG;
  if (bp_internal_score_bad_params(p) || bp_internal_score_bad_ref(ref, n_ref) >= 0) return BP_ERR_INVALID_ARG;
  // both sides by pitch, with the frames they sound on; the frames at which a side changes
  std::vector<Span> refs, ests;
  std::vector<int64_t> cuts{0, n_frames};
  auto add = [&](std::vector<Span>& side, double start_s, double end_s, double pitch) {
    Span s{0, 0, pitch};
    bp_internal_frame_interval(start_s, end_s, n_frames, &s.f0, &s.f1);
    if (s.f0 == s.f1) return;
    side.push_back(s);
    cuts.push_back(s.f0), cuts.push_back(s.f1);
  };
  for (int64_t i = 0; i < n_ref; ++i) add(refs, ref[i].start_s, ref[i].end_s, ref[i].pitch_midi);
  for (int64_t i = 0; i < n_est; ++i) add(ests, est[i].start_s, est[i].end_s, (double)est[i].pitch_midi);
  auto by_pitch = [](const Span& a, const Span& b) { return a.pitch < b.pitch; };
  std::stable_sort(refs.begin(), refs.end(), by_pitch);
  std::stable_sort(ests.begin(), ests.end(), by_pitch);
  std::sort(cuts.begin(), cuts.end());
  cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());

  bp_frame_score sum{n_frames, 0, 0, 0, 0};
  std::vector<double> sounding;  // the estimate side of a frame: distinct pitches, ascending
  for (size_t c = 0; c + 1 < cuts.size(); ++c) {
    const int64_t fr = cuts[c], len = cuts[c + 1] - fr;
    sounding.clear();
    for (const Span& e : ests)
      if (e.f0 <= fr && fr < e.f1 && (sounding.empty() || sounding.back() != e.pitch)) sounding.push_back(e.pitch);
    int64_t n_r = 0, tp = 0;
    size_t next = 0;  // the estimated pitches below are taken, or too low for this ref and every later one
    for (const Span& r : refs) {
      if (!(r.f0 <= fr && fr < r.f1)) continue;
      ++n_r;
      while (next < sounding.size() && sounding[next] < r.pitch && !hits(r.pitch, sounding[next], p)) ++next;
      if (next < sounding.size() && hits(r.pitch, sounding[next], p)) ++tp, ++next;
    }
    const int64_t n_e = (int64_t)sounding.size();
    sum.ref_frames += n_r * len, sum.est_frames += n_e * len, sum.true_pos += tp * len, sum.e_sub += (std::min(n_r, n_e) - tp) * len;
  }
  *out = sum;
  return BP_OK;
}

}  // extern "C"
