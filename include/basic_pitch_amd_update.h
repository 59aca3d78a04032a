/* basic_pitch_amd_update.h: the live transcripts of many streams in one step.  Same library, handle and stream types and rules
 * as basic_pitch_amd_live.h and basic_pitch_amd_rolling.h: every argument is checked before anything is queued, errors through
 * bp_last_error(h). */
#ifndef BASIC_PITCH_AMD_UPDATE_H
#define BASIC_PITCH_AMD_UPDATE_H

#include "basic_pitch_amd_rolling.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- an update of n streams: "what would bp_stream_candidates / bp_stream_candidates_rolling write for each of them?" ----
 * An update of one stream is about twenty launches and copies and a wait for a few microseconds of device work.  This call
 * takes n streams of one handle at once — of either retention mode (bp_stream_keep, bp_stream_keep_rolling), mixed, with their
 * own note parameters, horizons, rates and formats, of any age, finished or not: the tails' windows of all of them run in shared
 * batches (as bp_streams_peek runs them), and a constant number of launches and copies, whatever n, makes every stream's
 * record, bitmap, bends and new note rows.
 *
 * The outputs are PACKED and LINEAR in host memory, stream i's rows behind stream i - 1's in argument order; the caller
 * scatters them into whatever arrays or rings it keeps:
 *   note_out [note_rows][88] float32 and bend_out [note_rows][88] int8 (may be NULL)
 *                     stream i's rows [new_row, n_rows) at row note_offset.  new_row = n0 = max(held_rows, first_row).
 *                     Bend rows are written only for streams whose parameters include pitch bends.
 *   bits_out [bits_rows][12]   stream i's rows [first_row, n_rows) at row bits_offset.
 * bp_streams_update_layout fills first_row, n_rows, new_row, note_offset and bits_offset of every element and the two totals
 * from the streams' counters alone: no GPU work, nothing changed.  bp_streams_candidates fills them again, and status.
 *
 * The contract.  For every stream i with status 0: first_row and n_rows, rows [n0, T) of note (and of bend, where the stream
 * has bends and bend_out is not NULL) and rows [a, T) of the bitmap are bit for bit what the single call — bp_stream_candidates
 * for a keeping stream, bp_stream_candidates_rolling for a rolling one, alone on the same handle with the same held_rows —
 * writes for that stream, for any set, order and mixture of streams in the call.  For a stream with status 1 (a NaN in its
 * slice, or onset_threshold <= 0) only status, first_row, n_rows and the note rows are contractual; the caller falls back to
 * the maps as with the single calls.  A NaN in one stream changes no other stream's status or bytes.
 *
 * The call is an update: it commits nothing to any stream's counters.  Later pushes, peeks, single updates and the finish
 * return the bytes they would have returned without it.  with_tail as in the single calls.  n = 0 is BP_OK, nothing queued.
 *
 * Refused before anything is queued, the streams as they were, the message naming the index of the first offender: a null
 * stream, a stream of another handle, the same stream twice, a stream that retains nothing, a broken stream, held_rows outside
 * 0 ... rows emitted (BP_ERR_INVALID_ARG); a tail that does not fit the stream's ring (BP_ERR_UNSUPPORTED); then capacities
 * below the layout's totals and a null output with rows to write (BP_ERR_INVALID_ARG).  An error after the first enqueue
 * drains the queue and leaves every stream of the call broken, as a failed push does.
 */
typedef struct bp_stream_update {
  bp_stream stream;     /* in  */
  int64_t held_rows;    /* in : final rows of note / bend the caller already holds (the single calls' first_row / held_rows) */
  int64_t first_row;    /* out: a, the first row of the slice */
  int64_t n_rows;       /* out: T, the final rows and the tail */
  int64_t new_row;      /* out: n0 = max(held_rows, a), the first note / bend row sent */
  int64_t note_offset;  /* out: row of note_out / bend_out where this stream's rows [n0, T) start */
  int64_t bits_offset;  /* out: row of bits_out where this stream's rows [a, T) start */
  int status;           /* out: 0, or 1 (a NaN in the slice, onset_threshold <= 0) */
} bp_stream_update;

int bp_streams_update_layout(bp_handle h, int64_t n, bp_stream_update* u, int with_tail, int64_t* note_rows, int64_t* bits_rows);

int bp_streams_candidates(bp_handle h, int64_t n, bp_stream_update* u, int with_tail, float* note_out, int8_t* bend_out,
                          uint8_t* bits_out, int64_t note_capacity_rows, int64_t bits_capacity_rows);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_UPDATE_H */
