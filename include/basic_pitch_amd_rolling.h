/* basic_pitch_amd_rolling.h: rolling live transcripts — a stream that stays open for hours in bounded device memory.  Same
 * library, handle and stream types and rules as basic_pitch_amd_live.h: every argument is checked before anything is queued,
 * errors through bp_last_error(h). */
#ifndef BASIC_PITCH_AMD_ROLLING_H
#define BASIC_PITCH_AMD_ROLLING_H

#include "basic_pitch_amd_live.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- the rolling horizon: "what would the one-shot call return for the last H rows, had the track started there?" ----
 * bp_stream_keep reserves a row of device memory for every row the session will ever have.  A rolling stream keeps the last
 * H = horizon_rows rows of its maps in a ring, and a transcript is the exact decode of those rows: device memory, the bytes
 * sent home and the work of an update depend on H and never on the age of the stream.
 *
 * The contract.  X: all audio pushed so far; M = bp_infer_pcm_raw(X), T rows; a = max(0, T - H).  A rolling transcript is bit
 * for bit what bp_notes_decode returns for the maps M[a:T] as if they were a whole track — the inferred-onset differences of
 * rows a and a + 1 are zero (the decoder's t >= 2 case starts at a), rows a and T - 1 cannot be onset peaks, the two maxima
 * and the NaN flag are taken over the slice only — with every start_frame / end_frame shifted by a and the times evaluated
 * at the ABSOLUTE frames (model_frames_to_time, note_creation.py:346-357: the time of a frame depends on its window number,
 * so it is not "slice time plus a constant").  While T <= H that is the transcript of bp_stream_candidates.
 *
 *   bp_stream_keep_rolling   opt-in, before the first row leaves the stream, instead of bp_stream_keep (either one after the
 *                     other is BP_ERR_INVALID_ARG; horizon_rows < 3 is refused).  The stream then owns cap = horizon_rows +
 *                     2 * 142 rows of 1,760 bytes (the slice and the two windows of a tail; absolute row r lives at slot
 *                     r mod cap) and (cap + 63) / 64 + 3 records of 16 bytes: the two maxima and the NaN flag of every block
 *                     of 64 absolute rows, filled as the rows become final, and one record that is reserved.  That is all:
 *                     bp_stream_state_bytes grows by cap * 1760 + 16 * ((cap + 63) / 64 + 3) and reads the same after 3
 *                     windows and after 300.  No push is ever refused for the age of the stream.  The decoding parameters
 *                     are fixed here and constrain_frequency is applied to the kept copy, as with bp_stream_keep; the rows
 *                     handed out by push, peek and finish are untouched.
 *   bp_stream_horizon_first_row   a = max(0, n_rows - horizon_rows): pure geometry, no GPU.
 *   bp_stream_candidates_rolling  what bp_notes_decode_candidates_at needs for the slice [a, T): *first_row = a, *n_rows = T =
 *                     the final rows plus, with with_tail != 0, the rows of a peek (written to the slots behind the final
 *                     rows, never counted, overwritten by the next final rows).  The caller's arrays are RINGS of
 *                     ring_rows >= cap rows indexed by absolute row mod ring_rows: note_ring [ring_rows][88] float32,
 *                     bits_ring [ring_rows][12], bend_ring [ring_rows][88] int8 (may be null without pitch bends).  Note
 *                     and bend rows are written only for absolute rows >= max(held_rows, a): held_rows (0 ... rows emitted)
 *                     is the count of final rows the caller holds from earlier updates; the rows of a tail are sent every
 *                     time.  The bitmap is written for all rows of [a, T): it depends on the maxima, on a and on T.  Over
 *                     PCIe per update: the new rows and 12 * min(T, H) bytes.  *status as bp_stream_candidates: 1 = a NaN
 *                     in the slice or onset_threshold <= 0, decode the maps of bp_stream_rolling_maps with
 *                     bp_notes_decode.  A NaN leaves with its row: once the row is out of the horizon the status is 0
 *                     again.  ring_rows < cap and held_rows outside 0 ... rows emitted are BP_ERR_INVALID_ARG with nothing
 *                     changed.  Valid after bp_stream_finish (no tail then).
 *   bp_stream_rolling_maps   the kept maps of the slice, linear: note / onset [n][88], contour [n][264] for the n = T - a
 *                     rows (capacity_rows >= n; *first_row = a and *n_rows = T as above), for the status 1 fallback.  The
 *                     rows are frequency-constrained already; the constraint is idempotent, so decoding them with the
 *                     same parameters applies it again without effect.
 *   bp_notes_decode_candidates_at   bp_notes_decode_candidates on a linear slice whose frame 0 is absolute row first_frame:
 *                     start_frame / end_frame are shifted by first_frame and the times are those of the absolute frames;
 *                     everything else, and the whole result for first_frame = 0, is bp_notes_decode_candidates bit for bit.
 *                     Host code, no GPU.  first_frame < 0 or first_frame + n_frames > INT32_MAX is BP_ERR_INVALID_ARG.
 * The A/B library's bp_ab_stream_poison addresses an absolute row of a rolling stream as well and poisons the row's slot
 * whenever that row is written.
 */
int bp_stream_keep_rolling(bp_stream s, const bp_note_params* params, int64_t horizon_rows);
int64_t bp_stream_horizon_first_row(int64_t n_rows, int64_t horizon_rows);
int bp_stream_candidates_rolling(bp_stream s, int with_tail, float* note_ring, uint8_t* bits_ring, int8_t* bend_ring,
                                 int64_t ring_rows, int64_t held_rows, int64_t* first_row, int64_t* n_rows, int* status);
int bp_stream_rolling_maps(bp_stream s, int with_tail, float* note, float* onset, float* contour, int64_t capacity_rows,
                           int64_t* first_row, int64_t* n_rows);
int bp_notes_decode_candidates_at(const float* note, const uint8_t* cand_bits, const int8_t* bend_map, int64_t n_frames,
                                  int64_t first_frame, const bp_note_params* params, bp_note_event* events, int64_t max_events,
                                  int32_t* bends, int64_t max_bends, int64_t* n_events, int64_t* n_bends);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_ROLLING_H */
