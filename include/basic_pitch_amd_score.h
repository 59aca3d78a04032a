/* basic_pitch_amd_score.h: note-level precision / recall / F-measure counts of decoded events against reference notes — on the
 * host for one list of events, and on the device for every decode of a sweep, where a decode becomes 16 bytes of counts and
 * no event crosses PCIe.  Same library and handle type as basic_pitch_amd.h, same rules: every argument is checked before
 * anything is queued, errors through bp_last_error(h). */
#ifndef BASIC_PITCH_AMD_SCORE_H
#define BASIC_PITCH_AMD_SCORE_H

#include "basic_pitch_amd_sweep.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- the definition ----
 * A restatement of mir_eval.transcription.match_notes / precision_recall_f1_overlap (mir_eval 0.7), the note-level score
 * transcription papers report.  It is UNPINNED against mir_eval itself (mir_eval is not among this project's dependencies;
 * README, "Unpinned"): the tests hold it to an independent restatement of the same rules, not to that package.
 *
 * An estimated note is a decoded event: its pitch is pitch_midi, its times are the frame times of start_frame and end_frame,
 * the start_s / end_s every events call returns.  A reference note is a bp_ref_note, in seconds from the start of its
 * segment (clip).  All arithmetic is float64, evaluated as written, nothing fused.  With cmp being <=, or < when `strict`:
 *
 *   onset hit   rint(|ref.start_s - est.start_s| * 1e6) / 1e6  cmp  onset_tolerance_s                  (np.round(., 6))
 *   pitch hit   100 * |ref.pitch_midi - est.pitch_midi|  cmp  pitch_tolerance_cents
 *   offset hit  rint(|ref.end_s - est.end_s| * 1e6) / 1e6  cmp  max(offset_ratio * (ref.end_s - ref.start_s), offset_min_tolerance_s)
 *
 * mir_eval states the pitch distance as 1200 * |log2(f_est / f_ref)| of frequencies in Hz; with f = 440 * 2^((m - 69) / 12)
 * that is the same quantity, 100 * |m_est - m_ref|.  It is stated here in MIDI numbers, without a logarithm, so that the host
 * and the device evaluate the same operations and agree bit for bit.
 *
 *   matched_onset   the size of a MAXIMUM matching of the bipartite graph "onset hit and pitch hit" between refs and events
 *   matched_offset  the same for "onset hit, pitch hit and offset hit"
 *
 * The size of a maximum matching is unique: the counts depend neither on the algorithm nor on the order of the notes, so the
 * host and the device may search differently and must still agree exactly.  The second graph is a subgraph of the first, but
 * matched_offset is a maximum matching of its own, not the first one filtered.  mir_eval's average overlap ratio is NOT
 * offered: it is a mean over the pairs of the matching found, and depends on which maximum matching that is.
 *
 * Precision = matched / n_est, recall = matched / n_ref, F = 2 P R / (P + R), all 0 when either side is empty (as mir_eval);
 * the caller forms them from the counts.
 */
typedef struct bp_ref_note {
  double start_s, end_s; /* seconds from the start of its segment / clip */
  double pitch_midi;     /* may be fractional */
} bp_ref_note;           /* 24 bytes */

typedef struct bp_score_params {
  double onset_tolerance_s;      /* 0.05 */
  double offset_ratio;           /* 0.2  */
  double offset_min_tolerance_s; /* 0.05 */
  double pitch_tolerance_cents;  /* 50   */
  int32_t strict;                /* 0: <=, 1: < */
  int32_t reserved;              /* 0 */
} bp_score_params;               /* 40 bytes */

void bp_score_params_default(bp_score_params* p);

typedef struct bp_note_score {
  int32_t n_ref, n_est, matched_onset, matched_offset;
} bp_note_score; /* 16 bytes */

/*
 * ---- on the host: the checker, and the route for the decodes a device call leaves (status != 0) ----
 * No handle and no device.  Events are read for start_s, end_s and pitch_midi alone.  BP_ERR_INVALID_ARG for a null pointer
 * with a count above 0, a negative count, null p or out, and everything the device calls refuse in refs and p (below).
 */
int bp_score_note_events(const bp_note_event* est, int64_t n_est, const bp_ref_note* ref, int64_t n_ref, const bp_score_params* p,
                         bp_note_score* out);

/*
 * ---- on the device: every decode of a sweep scored where its events lie ----
 * bp_note_events_sweep_score takes its segments, sets and decode table as bp_note_events_sweep does,
 * bp_infer_clips_events_sweep_score its clips as bp_infer_clips_events_sweep does (decodes == NULL: the cross product,
 * set-major), and both run that sweep up to and including its one tracker launch.  Then one more launch, a workgroup per
 * decode, scores the decode's events in the tracker's pool against the refs of its segment: refs[ref_offsets[i]] ...
 * refs[ref_offsets[i + 1] - 1] are segment (clip) i's, ref_offsets[0] = 0.  scores [n_decodes] and status [n_decodes] come
 * home, 20 bytes per decode; events and bends are neither packed nor copied.
 *
 * The contract.  For every decode j with status[j] == 0, scores[j] is what bp_score_note_events returns for the events
 * bp_note_events_sweep (bp_infer_clips_events_sweep) returns for decode j, with the refs of its segment and score_params.
 *
 *   status[j]   0, 1, 2  as basic_pitch_amd_events.h defines them.
 *               3        the decode has more than BP_SCORE_MAX_NOTES events, or its segment more than that many refs.
 *               For a non-zero status scores[j] is {n_ref, 0, 0, 0} and no other decode is affected; the caller scores such a
 *               decode through the other routes and bp_score_note_events.
 *   sets        include_pitch_bends changes no score: these calls make no bend map and need no bend pool.  The bends a set asks
 *               for are still COUNTED against the capacity of the decode's region (status 2), so that a decode's status is
 *               the one the sweep calls give it.  The frequency limits of a set do not filter the refs; a caller who sweeps
 *               a band passes the refs of that band.
 *   refused     (BP_ERR_INVALID_ARG, the message names the index) what the sweep calls refuse; null scores, status or
 *               ref_offsets; ref_offsets that do not start at 0 or that decrease (the segment is named); a ref with a
 *               non-finite field or end_s < start_s (the ref is named); a non-finite or negative tolerance or ratio; a
 *               non-zero `reserved`.
 *   nothing to do, afterwards   as the sweep calls; the decodes of a call without device work have {n_ref, 0, 0, 0} and their
 *               status.  The events calls on the same handle are undisturbed, before and after.
 *
 * BP_SCORE_MAX_NOTES.  A workgroup keeps the state of its search in LDS: per ref the event it is matched to (a 16-bit index)
 * and one bit of the visited map, per level of the alternating path the event and the ref taken there (two 16-bit indices),
 * the path being at most as deep as the smaller side.  That is 2 + 4 bytes and 1 bit per note, 6.125 bytes:
 *     16,384 notes x 6.125 bytes = 100,352 bytes of the 163,840 a compute unit has; 32,768 notes would need 200,704.
 * A launch takes what its largest decode can need (the refs of its segment, the events its region of the pool holds), not
 * the bound: a job of one-window segments with some tens of refs each takes under 1 KiB per workgroup.
 *
 * Memory.  BP_SWEEP_MAX_DECODES and BP_SWEEP_MAX_ROWS apply as they stand.  Of the per-decode-row figures in
 * basic_pitch_amd_sweep.h the two bend terms (2 x 88 bytes) and the packed copy of the event records fall away: 16 x 88 /
 * (min_note_len + 1) bytes of event records per decode row (117 at the default 11, 1408 at 0) and, when a segment has more
 * than 432 rows, 360 bytes of working state.  At the cap that is 4.0 GB with the default minimum length and 14.8 GB at the
 * worst (6.5 and 28 for the sweep calls).  The refs take 24 bytes each on the device.
 */
#define BP_SCORE_MAX_NOTES 16384

int bp_note_events_sweep_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, const float* onset,
                               const float* contour, int mem_kind, int64_t n_sets, const bp_note_params* sets, int64_t n_decodes,
                               const bp_sweep_decode* decodes, const int64_t* ref_offsets /*[n_segments+1]*/, const bp_ref_note* refs,
                               const bp_score_params* score_params, bp_note_score* scores /*[n_decodes]*/, int* status /*[n_decodes]*/);
int bp_infer_clips_events_sweep_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                      int64_t n_sets, const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                                      const int64_t* ref_offsets /*[n_clips+1]*/, const bp_ref_note* refs,
                                      const bp_score_params* score_params, bp_note_score* scores /*[n_decodes]*/,
                                      int* status /*[n_decodes]*/);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_SCORE_H */
