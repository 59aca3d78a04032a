/* basic_pitch_amd_stream_events.h: the note events of many live streams straight from the device.  Same library, handle and
 * stream types and rules as basic_pitch_amd_update.h and basic_pitch_amd_events.h: every argument is checked before anything is
 * queued, errors through bp_last_error(h). */
#ifndef BASIC_PITCH_AMD_STREAM_EVENTS_H
#define BASIC_PITCH_AMD_STREAM_EVENTS_H

#include "basic_pitch_amd_update.h"
#include "basic_pitch_amd_events.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- the events of n streams: "what would the single update + bp_notes_decode_candidates_at give for each of them?" ----
 * bp_streams_candidates refreshes the candidates of n streams in one device step, and then a host thread per stream runs the
 * sequential half of note decoding over the whole slice, and the bitmap of the slice and the new note and bend rows travel home
 * at every update.  This call runs that half on the device too (the tracker of bp_infer_clips_events, one workgroup per
 * stream, each with the stream's own parameters) and brings home the events and their bends alone.
 *
 * The contract.  For every stream i with status 0, first_row, n_rows and the events event_offsets[i] ... event_offsets[i + 1] - 1
 * with their bends are, field by field and in order, what this route returns: the single update of that stream with
 * held_rows = 0 (bp_stream_candidates for a keeping stream, bp_stream_candidates_rolling for a rolling one), followed by
 * bp_notes_decode_candidates_at(..., first_frame = first_row, the parameters the stream was given when it began to keep rows).
 * Frames are absolute (shifted by first_row), the times are those of the absolute frames; pitch, the float32 amplitude,
 * bend_offset / n_bends (into `bends`, the bends of all streams in event order) as there; reserved fields are zero.  This holds
 * for any set, order and mixture of streams in the call: keeping and rolling, each with its own parameters, rate and format,
 * of any age, finished or not, with or without a tail.
 *
 *   status  0  decoded.
 *           1  a NaN in the slice, or onset_threshold <= 0, as bp_streams_candidates reports it.
 *           2  the slice has more than BP_EVENTS_MAX_ROWS rows, or its events or bends passed its region:
 *              bp_events_capacity(n_rows - first_row, min_note_len) events and 88 * (n_rows - first_row) bends.
 *           A stream with status 1 or 2 has no events here (event_offsets[i + 1] == event_offsets[i]) and affects no other
 *           stream; the caller takes the existing routes for it (the single updates, bp_stream_rolling_maps).
 *
 * Like bp_streams_candidates the call commits nothing: later pushes, peeks, updates of either kind and the finish return the
 * bytes they would have returned without it.  n = 0, or no stream with a row yet, is BP_OK with zero offsets, nothing queued.
 *
 * Refused before anything is queued, the streams as they were, the message naming the index of the first offender: what
 * bp_streams_candidates refuses (a null stream, a stream of another handle, the same stream twice, a stream that retains
 * nothing, a broken stream: BP_ERR_INVALID_ARG; a tail that does not fit: BP_ERR_UNSUPPORTED), a stream whose kept parameters
 * have the melodia trick with a negative frame threshold or a negative min_note_len, and one whose absolute frames pass
 * INT32_MAX (both as the host decoder refuses them).
 *
 *   max_events,  the room at `events` / `bends` (which may be NULL when the room is 0).  When the call needs more it fails with
 *   max_bends    BP_ERR_INVALID_ARG, event_offsets[n] and the message hold the totals needed (the message both), status and
 *                event_offsets are complete, the streams are as they were, and the call can be repeated with larger buffers.
 *   afterwards   an error after the first enqueue drains the queue and leaves every stream of the call broken, as a failed
 *                push does.
 *
 * Device memory.  The whole slice [first_row, n_rows) of every stream is gathered and decoded on the device at every call
 * (nothing of it goes home), in grow-only buffers of the handle sized by the largest call.  Per slice row: 352 B note rows,
 * 88 B bend map, 12 B bitmap, 2 x 88 B bends (the regions and their packed copy) and 32 * 88 / (min_note_len + 1) B of event
 * records — about 900 B for min_note_len = 11 — and 360 B more for the tracker's working state when any slice of the call has
 * more than 432 rows.  The bend map of the whole slice is computed at every call.
 *
 * bp_streams_events_layout fills first_row and n_rows of every element from the streams' counters alone (no GPU work, nothing
 * changed) and returns the sums of the regions' capacities: with max_events >= *events_capacity and max_bends >=
 * *bends_capacity the call cannot fail for room.
 */
typedef struct bp_stream_events {
  bp_stream stream;   /* in  */
  int64_t first_row;  /* out: a, the first row of the slice */
  int64_t n_rows;     /* out: T, the final rows and the tail */
  int status;         /* out: 0, 1 or 2 */
} bp_stream_events;

int bp_streams_events_layout(bp_handle h, int64_t n, bp_stream_events* u, int with_tail, int64_t* events_capacity,
                             int64_t* bends_capacity);

int bp_streams_events(bp_handle h, int64_t n, bp_stream_events* u, int with_tail, bp_note_event* events, int64_t max_events,
                      int32_t* bends, int64_t max_bends, int64_t* event_offsets /*[n+1]*/);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_STREAM_EVENTS_H */
