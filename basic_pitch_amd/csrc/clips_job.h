// Private to csrc: the driver of the jobs of many clips or segments (run_clips, clips_api.hip) and the protocol of its sinks
// (clips_api.hip: candidates, events; clips_sweep.hip, clips_multipitch.hip, clips_melody.hip, clips_align.hip,
// clips_beat.hip).  An entry point is a source, a sink on its own stack, and one call of run_clips:
//   handle -> sink.check -> the source's plan -> given maps against sink.use() -> sink.plan -> (nothing queued: done) ->
//   the device, the filter -> finish(the source's maps; sink.queue) -> sink.home -> the FLAC decoder's verdicts.
// Lifetime: the sink and the driver's own job state both outlive finish — run_clips returns only after it — so a host buffer
// that an asynchronous copy reads is a member of the sink (or of the driver's job) and needs no other owner.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "../../include/basic_pitch_amd_flac_clips.h"
#include "../../include/basic_pitch_amd_score.h"
#include "bp_context.h"

// (none of this is the libraries' ABI: the symbols stay out of their dynamic tables)
#pragma GCC visibility push(hidden)
namespace bp {

// Where the maps of the n segments come from.  kPcmClips: `clips` (PCM in host or device memory after mem_kind) at sample_rate;
// kFlacClips: `flac` (bytes in host memory, STREAMINFO rate sample_rate), decoded on the device, then as kPcmClips in device
// memory; kAdpcmClips: `adpcm` (IMA ADPCM files' bytes in host memory; the rate is the files'), decoded on the device by one
// launch, then as kPcmClips in device memory; kGivenMaps: no signal but maps already made (mem_kind), segment c at rows
// [row_offsets[c], row_offsets[c + 1]).
enum JobSourceKind { kPcmClips, kFlacClips, kGivenMaps, kAdpcmClips };
struct JobSource {
  JobSourceKind kind;
  int64_t n;
  int mem_kind, sample_rate;
  const bp_clip* clips;
  const bp_flac_clip* flac;
  const int64_t* row_offsets;
  const float *note, *onset, *contour;
  const bp_adpcm_clip* adpcm;
};
inline JobSource pcm_clips(int64_t n, const bp_clip* clips, int sample_rate, int mem_kind) {
  return JobSource{kPcmClips, n, mem_kind, sample_rate, clips};
}
inline JobSource given_maps(int64_t n, const int64_t* row_offsets, const float* note, const float* onset, const float* contour, int mem_kind) {
  return JobSource{kGivenMaps, n, mem_kind, 0, nullptr, nullptr, row_offsets, note, onset, contour};
}

// What a sink reads of given maps.  note / onset / contour: the plane must be given and is read.  private_copy: the sink takes
// all three as take_given_maps' copy in track_out.  Otherwise a plane is read where it lies, unless it is in host memory — or,
// with aligned16, in device memory off a 16-byte boundary — and is then copied into the sink's own buffer (*_copy).
struct MapsUse {
  bool note, onset, contour, aligned16, private_copy;
  DeviceBuffer<float>*note_copy = nullptr, *onset_copy = nullptr, *contour_copy = nullptr;
};

// Where the results go: four phases, called in this order by run_clips.  n: the segments; offs: their rows, [n + 1].
struct JobSink {
  virtual MapsUse use(bp_handle h) const = 0;
  // the fixed arguments: everything that does not depend on a segment's rows.  Nothing is written.
  virtual int check(bp_handle h, const char* what, int64_t n) = 0;
  // the outputs against the rows, the host tables, the results that need no device.  *queued false: the outputs are complete.
  virtual int plan(bp_handle h, const char* what, int64_t n, const int64_t* offs, bool* queued) = 0;
  // behind the maps of all segments, which the source has queued (on the device; `all` holds the planes use() names)
  virtual int queue(bp_handle h, const Maps& all, int64_t n, const int64_t* offs) = 0;
  // the stream has drained.  A second pass is queued here and waited for with finish.
  virtual int home(bp_handle h, const char* what, int64_t n, const int64_t* offs) = 0;
  // What the FLAC source's own steps need of a sink that takes FLAC clips: where the clips' statuses go, and, where note
  // events go home, the events (event_offsets null: none do).
  virtual EventsSink clip_results() const { return EventsSink{}; }

 protected:
  ~JobSink() = default;
};

int run_clips(bp_handle h, const char* what, JobSource src, JobSink& sink);

// ---- what the sinks share (clips_api.hip) --------------------------------------------------------------------------------------
int invalid(bp_handle h, const char* what, const std::string& why);
// -1: offsets (n + 1 of them) start at 0 and never decrease; 0: null, or no 0 at the start; i > 0: offsets[i] < offsets[i - 1]
int64_t ascending_from_zero(const int64_t* offsets, int64_t n);
// room for `max` records in `buffer`: not negative, and none without a buffer
inline bool check_room(int64_t max, const void* buffer) { return max >= 0 && (max == 0 || buffer); }
// why the tracker refuses a parameter set (null: it takes it), and why a call's room for events and bends is refused
const char* bad_params(const bp_note_params& prm);
const char* bad_room(const EventsSink& out);
// A swept call's counts (`nulls`: one of the call's own pointers is missing; both under the message `counts`), then `also`
// (null: nothing more), the bound on the decodes, every set by bad_set (null: it is taken), and the decode table against the
// segments and sets (decodes null: the cross product).
int check_sets_and_decodes(bp_handle h, const char* what, int64_t n_segs, int64_t n_sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                           bool nulls, const char* counts, const char* also, const std::function<const char*(int64_t)>& bad_set);
// decode j of a swept call: its segment and its set (decodes null: the cross product, set-major)
struct DecodePair {
  int64_t segment;
  int32_t set;
};
inline DecodePair decode_pair(const bp_sweep_decode* decodes, int64_t j, int64_t n_segs) {
  return decodes ? DecodePair{decodes[j].segment, decodes[j].params} : DecodePair{j % n_segs, (int32_t)(j / n_segs)};
}
// BP_OK, or the refusal of `rows` rows in all above BP_SWEEP_MAX_ROWS (lead: what has them, in front of the count)
int check_rows_in_all(bp_handle h, const char* what, int64_t rows, const char* lead = "");
// what a scored call takes of refs: ref_offsets and `out` (named out_name in the message; needed where there are decodes),
// the scoring parameters, the refs themselves
int check_score(bp_handle h, const char* what, int64_t n_segs, int64_t n_decodes, const int64_t* ref_offsets, const bp_ref_note* refs,
                const bp_score_params* score_params, const void* out, const char* out_name);
// every segment's refs in ascending pitch (stable), each with the frames it sounds on among the segment's rows, by the
// checker's own function: put(slot, ref, f0, f1), slot = ref_offsets[segment] + its place in that order
void refs_in_pitch_order(int64_t n_segs, const int64_t* offs, const int64_t* ref_offsets, const bp_ref_note* refs,
                         const std::function<void(size_t, const bp_ref_note&, int32_t, int32_t)>& put);
// a block that came home as n_words int64 words with 32-bit statuses behind them: the statuses
inline const int32_t* statuses_behind(const int64_t* block, int64_t n_words) { return reinterpret_cast<const int32_t*>(block + n_words); }

}  // namespace bp
#pragma GCC visibility pop
