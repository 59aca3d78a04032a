/* basic_pitch_amd_live.h: live transcripts of the streaming sessions of basic_pitch_amd.h (same library, same handle and
 * stream types, same rules: every argument is checked before anything is queued, errors through bp_last_error(h)). */
#ifndef BASIC_PITCH_AMD_LIVE_H
#define BASIC_PITCH_AMD_LIVE_H

#include "basic_pitch_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- live transcripts: "what would the one-shot call return if the audio ended now?" ----
 * Final rows trail the audio by 0.4 to 2 seconds (a row leaves once its window is complete), and note events exist only for a
 * whole track: get_infered_onsets (note_creation.py:289-311) scales by two maxima over all frames and the melodia pass walks
 * the whole posteriorgram, so an early event can change when later audio arrives.  What IS exact at any moment is the
 * answer for the audio so far, and these calls give it without ending the stream.
 *
 *   bp_stream_peek    the rows bp_stream_finish would emit now, with nothing committed.  After a stream has taken input X, the
 *                     rows it has emitted followed by the rows of a peek are bit for bit bp_infer_pcm_raw(X); the stream is
 *                     left exactly as it was, and every later push or finish returns the bytes it would have returned
 *                     without the peek.  bp_stream_rows_bound(s, 0) bounds the rows; a stream that has taken no frames
 *                     gives 0 rows; a finished or broken stream is refused.
 *   bp_streams_peek   the same for n DIFFERENT streams of handle h: the tail windows of all of them packed into full batches,
 *                     one windowing launch, the model and one un-overlapping launch per batch, like bp_streams_push.
 *   bp_stream_keep    opt-in, before the first row leaves the stream: from now on the three maps of every row the stream
 *                     emits also stay in device memory, 1,760 bytes per row (about 10.6 MB per minute of audio), reserved
 *                     here for max_rows rows (and the two windows of a tail) and counted by bp_stream_state_bytes.  A push or
 *                     finish that would exceed max_rows fails with BP_ERR_OUT_OF_MEMORY before anything is queued; the stream
 *                     stays valid (bp_stream_peek, bp_stream_candidates, bp_stream_close).  The decoding parameters are
 *                     fixed here: constrain_frequency (note_creation.py:314-343) is applied to the kept copy.  The rows handed
 *                     to the caller by push, peek and finish stay unconstrained and unchanged.
 *   bp_stream_candidates  what bp_notes_decode_candidates needs for *n_rows = T rows, in the layouts of bp_note_candidates:
 *                     T = the kept rows plus, with with_tail != 0, the rows of a peek — written behind the kept rows and never
 *                     counted as kept.  note_out [T][88] and bend_map [T][88] are written only from row first_row on: pass
 *                     the count of final rows already held from earlier updates (0 ... rows emitted; final rows never change,
 *                     the rows of a tail are sent every time).  cand_bits [T][12] is written whole on every update: it
 *                     depends on the two maxima and on T.  The maxima are carried in a per-stream record that final rows
 *                     join as they are emitted; an update joins the tail to a copy of it.  Work per update therefore does
 *                     not grow with the session beyond the 12 bytes per row of the bitmap.  *status as bp_note_candidates:
 *                     1 = a NaN in the maps or onset_threshold <= 0, decode the maps themselves (the rows of push + peek)
 *                     with bp_notes_decode.  capacity_rows < T is BP_ERR_INVALID_ARG with nothing changed.  Valid after
 *                     bp_stream_finish too (no tail then: the kept rows are the track).
 * Testing the NaN path: the A/B library (build_library(ab=True)) exports bp_ab_stream_poison(s, map, row, bin), which makes
 * one cell of the kept copy a NaN whenever its row is written; the product library has no such call.
 * Same events as bp_notes_decode on bp_infer_pcm_raw of the audio so far, bit for bit (tests/test_gpu_stream_peek.py).
 */
int bp_stream_peek(bp_stream s, float* note, float* onset, float* contour, int64_t capacity_rows, int out_mem_kind,
                   int64_t* rows);
int bp_streams_peek(bp_handle h, int64_t n, const bp_stream* streams, float* const* note, float* const* onset,
                    float* const* contour, const int64_t* capacity_rows, int out_mem_kind, int64_t* rows);
int bp_stream_keep(bp_stream s, const bp_note_params* params, int64_t max_rows);
int bp_stream_candidates(bp_stream s, int with_tail, float* note_out, uint8_t* cand_bits, int8_t* bend_map, int64_t first_row,
                         int64_t capacity_rows, int64_t* n_rows, int* status);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_LIVE_H */
