/* basic_pitch_amd_frame_score.h: frame-level precision / recall / accuracy and error-rate counts of decoded events against
 * reference notes — on the host for one list of events, and on the device for every decode of a sweep, beside the note-level
 * counts of basic_pitch_amd_score.h: one more launch behind the tracker, 40 more bytes per decode on their way home, no event
 * across PCIe.  Same library and handle type as basic_pitch_amd.h, same rules: every argument is checked before anything is
 * queued, errors through bp_last_error(h). */
#ifndef BASIC_PITCH_AMD_FRAME_SCORE_H
#define BASIC_PITCH_AMD_FRAME_SCORE_H

#include "basic_pitch_amd_score.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- the definition ----
 * A restatement of mir_eval.multipitch.evaluate (mir_eval 0.7) for the case where reference and estimate are sampled on the
 * same time base, the segment's own frames: the frame-level score ("Acc") transcription papers report beside the note-level
 * F-measures.  It is UNPINNED against mir_eval itself (mir_eval is not among this project's dependencies; README,
 * "Unpinned"): the tests hold it to an independent restatement of the same rules, not to that package.
 *
 *   frames     A segment of n_frames rows has the frames 0 ... n_frames - 1; frame fr has the time time(fr) =
 *              model_frames_to_time()[fr], the expression every event's start_s / end_s come from.  That expression steps
 *              DOWN a little at every multiple of 172 (the window offset) but is strictly increasing: a frame is later than
 *              the frame before it by at least 1.2 ms.
 *   sounding   A note, reference or estimated alike, sounds on frame fr when start_s <= time(fr) < end_s, in float64,
 *              evaluated as written.  For a decoded event this is exactly start_frame <= fr < end_frame.  A ref with
 *              end_s == start_s sounds nowhere; refs may start before 0 or end after the segment.
 *   sides      The estimate side of a frame is the SET of distinct pitch_midi of the events sounding there (the tracker
 *              never emits two events of one pitch on one frame; the host checker, which takes arbitrary events, dedupes).
 *              The reference side is the MULTISET of the refs sounding there, as given.  Pitches may be fractional and
 *              outside 21 ... 108.
 *   hit        100 * |ref.pitch_midi - est.pitch_midi|  cmp  pitch_tolerance_cents, cmp being <=, or < when `strict`: the
 *              note level's pitch predicate, without a logarithm.  Of bp_score_params only pitch_tolerance_cents and strict
 *              are read; the other fields are validated as they are for the note level.
 *   per frame  n_ref(fr), n_est(fr) the sizes of the two sides; tp(fr) the size of a MAXIMUM matching of the frame's hit
 *              graph.  The size is unique, so the host and the device may search differently.  Every ref hits an interval
 *              of pitches of one width, so a greedy is ALLOWED, not required: refs in ascending pitch, each taking the
 *              lowest estimated pitch it hits that is still free (earliest-deadline matching of equal windows) finds a
 *              maximum matching.  (mir_eval counts a frame's true positives with util.match_events, a maximum bipartite
 *              matching within a window of half a semitone; the tolerance is a parameter here.)
 *
 * The counts are sums over the frames of a segment:
 *
 *   n_frames    the frames of the segment
 *   ref_frames  sum of n_ref(fr)          est_frames  sum of n_est(fr)
 *   true_pos    sum of tp(fr)             e_sub       sum of min(n_ref(fr), n_est(fr)) - tp(fr)
 *
 * Misses and false alarms follow exactly.  Per frame, e_miss(fr) = max(0, n_ref - n_est) and e_fa(fr) = max(0, n_est - n_ref),
 * and max(0, a - b) = a - min(a, b), so  n_ref(fr) = tp(fr) + e_sub(fr) + e_miss(fr)  and  n_est(fr) = tp(fr) + e_sub(fr) +
 * e_fa(fr)  on every frame, hence over their sums:
 *
 *   e_miss = ref_frames - true_pos - e_sub        e_fa = est_frames - true_pos - e_sub
 *
 * The caller forms every rate, and every rate is 0 when its denominator is 0: precision = true_pos / est_frames, recall =
 * true_pos / ref_frames, accuracy = true_pos / (ref_frames + est_frames - true_pos), and the four error rates e_sub, e_miss,
 * e_fa and e_tot = e_sub + e_miss + e_fa, each over ref_frames.
 *
 * The chroma variants of mir_eval.multipitch are NOT offered: matching on the pitch circle is not a problem of equal
 * intervals on a line and would need a search of its own.
 *
 * All fields are int64: BP_SWEEP_MAX_ROWS rows times BP_SCORE_MAX_NOTES refs does not fit 32 bits.
 */
typedef struct bp_frame_score {
  int64_t n_frames, ref_frames, est_frames, true_pos, e_sub;
} bp_frame_score; /* 40 bytes */

/*
 * ---- on the host: the checker, and the route for the decodes a device call leaves (status != 0) ----
 * No handle and no device.  Events are read for start_s, end_s and pitch_midi alone.  BP_ERR_INVALID_ARG for what
 * bp_score_note_events refuses (a null pointer with a count above 0, a negative count, null p or out, a ref with a
 * non-finite field or end_s < start_s, a negative or non-finite tolerance or ratio, a non-zero `reserved`) and for a negative
 * n_frames.
 */
int bp_score_note_frames(const bp_note_event* est, int64_t n_est, const bp_ref_note* ref, int64_t n_ref, int64_t n_frames,
                         const bp_score_params* p, bp_frame_score* out);

/*
 * ---- on the device: every decode of a sweep scored at both levels where its events lie ----
 * The two calls take the arguments of bp_note_events_sweep_score and bp_infer_clips_events_sweep_score up to score_params and
 * run the same job up to and including its one tracker launch.  Then the note-matching launch of those calls, unless scores is
 * NULL, and one more launch, a workgroup per decode, that rolls the decode's events into a bit mask per frame and matches the
 * refs sounding on each frame against it.
 *
 * The contract.  For every decode j with status[j] == 0, frames[j] is what bp_score_note_frames returns for the events
 * bp_note_events_sweep (bp_infer_clips_events_sweep) returns for decode j, with the refs of its segment, n_frames = the rows
 * of its segment, and score_params; scores[j], when asked for, is what bp_note_events_sweep_score gives.
 *
 *   status[j]   in every case the status bp_note_events_sweep_score gives that decode — 0, 1, 2, or 3 for more than
 *               BP_SCORE_MAX_NOTES events or refs —, whether scores is NULL or not.  A non-zero status leaves frames[j] =
 *               {n_frames, 0, 0, 0, 0} and scores[j] = {n_ref, 0, 0, 0} and touches no other decode; the caller scores such a
 *               decode through the other routes, bp_score_note_events and bp_score_note_frames.
 *   scores      NULL: the note-matching launch is skipped, and 44 bytes per decode come home instead of 60.
 *   refused     (BP_ERR_INVALID_ARG, the message names the index) what the scoring calls refuse, but for a null scores; and
 *               a null frames.
 *   nothing to do, afterwards   as the scoring calls; the decodes of a call without device work have {n_frames, 0, 0, 0, 0},
 *               {n_ref, 0, 0, 0} and their status.  The events, sweep and scoring calls on the same handle are undisturbed,
 *               before and after.
 *
 * Memory.  What basic_pitch_amd_score.h says, and 16 bytes more per ref on the device (its frames and the pitches it hits,
 * worked out on the host by the checker's own functions: the kernel compares integers alone).  A workgroup keeps 12 bytes of
 * LDS per frame of the chunk it works on; a launch takes that for its longest decode, at most 2,048 frames (24 KiB).
 */
int bp_note_events_sweep_frame_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note,
                                     const float* onset, const float* contour, int mem_kind, int64_t n_sets,
                                     const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                                     const int64_t* ref_offsets /*[n_segments+1]*/, const bp_ref_note* refs,
                                     const bp_score_params* score_params, bp_note_score* scores /*[n_decodes] or NULL*/,
                                     bp_frame_score* frames /*[n_decodes]*/, int* status /*[n_decodes]*/);
int bp_infer_clips_events_sweep_frame_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                            int64_t n_sets, const bp_note_params* sets, int64_t n_decodes,
                                            const bp_sweep_decode* decodes, const int64_t* ref_offsets /*[n_clips+1]*/,
                                            const bp_ref_note* refs, const bp_score_params* score_params,
                                            bp_note_score* scores /*[n_decodes] or NULL*/, bp_frame_score* frames /*[n_decodes]*/,
                                            int* status /*[n_decodes]*/);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_FRAME_SCORE_H */
