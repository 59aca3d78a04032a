/* basic_pitch_amd_events.h: note events straight from the device for a job of many clips.  Same library and handle type as
 * basic_pitch_amd.h, same rules: every argument is checked before anything is queued, errors through bp_last_error(h). */
#ifndef BASIC_PITCH_AMD_EVENTS_H
#define BASIC_PITCH_AMD_EVENTS_H

#include "basic_pitch_amd_clips.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- a job of clips: "what would bp_infer_clips_candidates + bp_notes_decode_candidates give for each of them?" ----
 * bp_infer_clips_candidates brings home 450 bytes per row (the note map, the onset-peak bitmap, the bend map) for a host
 * thread to run the sequential half of note decoding on.  These calls run that half on the device too, one workgroup per
 * clip, and bring home the events and their bends alone.
 *
 * The contract.  For every clip i with status[i] = 0 the events event_offsets[i] ... event_offsets[i + 1] - 1 are, field by
 * field and in order, the events bp_notes_decode_candidates returns for clip i's rows of bp_infer_clips_candidates (or of
 * bp_note_candidates on clip i's maps alone) with the same parameters: frames, pitch, the float32 amplitude, the times
 * (the host fills them with the expression bp_notes_decode uses), the bends.  bend_offset indexes `bends`, which holds the
 * bends of all clips in event order; reserved fields are zero.
 *
 * The order of a clip's events: the notes from the onset peaks first — frames T-2 ... 1, bins 87 ... 0, every peak in that
 * order, each seeing the cells the notes before it zeroed —, then the notes of the melodia trick in the order its argmax
 * (ties to the lowest t * 88 + f) finds them.
 *
 *   status[i]  0  decoded.
 *              1  a NaN in the clip's note or onset rows, or params->onset_threshold <= 0 (as bp_infer_clips_candidates).
 *              2  the clip's events or bends passed the capacity of its region, or it has more than BP_EVENTS_MAX_ROWS rows.
 *              For 1 and 2 the clip has no events here (event_offsets[i + 1] == event_offsets[i]) and no other clip is affected;
 *              the caller decodes it by the other routes (bp_infer_pcm_raw + bp_notes_decode, bp_infer_pcm_raw_candidates).
 *
 * Capacity.  A clip of `rows` rows decodes into a region of the handle's pool that holds bp_events_capacity(rows,
 * min_note_len) events and 88 * rows bends:
 *     bp_events_capacity = 88 * ceil(rows / (max(min_note_len, 0) + 1))        (0 for rows > BP_EVENTS_MAX_ROWS)
 * Why that is enough for ordinary parameters (frame_threshold > 0): a note spans more than min_note_len frames and zeroes its
 * own cells, and it ends where energy_tol cells below the threshold follow it (or at the clip's end).  A later scan or melodia
 * walk at that pitch that reaches the note from either side meets its zeroed cells and those cells behind them, at least
 * energy_tol cells below the threshold in a row, and ends before them; a melodia walk zeroes every cell it visits.  The notes
 * of one pitch are therefore disjoint spans of at least min_note_len + 1 of the clip's rows: at most rows / (min_note_len + 1)
 * events and rows bends per pitch, times 88 pitches.  (One exception, a walk that starts on the clip's last row, which no
 * scan counts, is far inside the slack of 88 pitches.)  With a frame threshold of 0, zeroed cells no longer end a scan, notes
 * of one pitch overlap and a dense clip can pass the bound: status 2.
 *
 *   params        params->melodia_trick with a negative frame_threshold is refused as bp_notes_decode refuses it; a negative
 *                 min_note_len is refused.
 *   max_events,   the room at `events` / `bends` (which may be NULL when the room is 0).  When the job needs more the call
 *   max_bends     fails with BP_ERR_INVALID_ARG, event_offsets[n_clips] and the message hold the totals needed (the message
 *                 both), status and event_offsets are complete, and the call can be repeated with larger buffers.
 *   afterwards    as after bp_infer_clips_candidates; a call that fails after queuing returns once the stream has drained.
 *
 * bp_infer_clips_events: bp_infer_clips_candidates followed by the tracker; the clips' arguments are that call's.
 * bp_note_events_from_maps: the same for posteriorgram segments the caller already holds (mem_kind: host or device), clip i
 * at rows [row_offsets[i], row_offsets[i + 1]) of note / onset [rows][88] and contour [rows][264]; row_offsets[0] = 0.  The
 * caller's maps are left untouched (frequency limits are applied to a copy), as by bp_note_candidates.  n_clips = 1 is a
 * single set of maps.
 */
#define BP_EVENTS_MAX_ROWS 8192

int64_t bp_events_capacity(int64_t rows, int min_note_len);

int bp_infer_clips_events(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                          const bp_note_params* params, bp_note_event* events, int64_t max_events, int32_t* bends,
                          int64_t max_bends, int64_t* event_offsets /*[n_clips+1]*/, int* status);
int bp_note_events_from_maps(bp_handle h, int64_t n_clips, const int64_t* row_offsets, const float* note, const float* onset,
                             const float* contour, int mem_kind, const bp_note_params* params, bp_note_event* events,
                             int64_t max_events, int32_t* bends, int64_t max_bends, int64_t* event_offsets, int* status);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_EVENTS_H */
