/* basic_pitch_amd_melody.h: the melody of the contour posteriorgram — ONE f0 track with voiced / unvoiced decisions, decoded
 * by a Viterbi recurrence over the frames of a segment, on the device for the segments of a job or for clips through the
 * model, and sweeps of its parameters scored by the melody measures where the track is, with nothing but counts on their way
 * home.  Same library and handle type as basic_pitch_amd.h, same rules as basic_pitch_amd_multipitch.h: every argument is
 * checked before anything is queued, errors through bp_last_error(h), a refusal names the index, a call that fails after
 * queuing returns once the handle's stream has drained. */
#ifndef BASIC_PITCH_AMD_MELODY_H
#define BASIC_PITCH_AMD_MELODY_H

#include "basic_pitch_amd_multipitch.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- the definition ----
 * What the melody of a segment is, said once: the host checker, the kernel and the tests' restatement are all held to it.
 * It is UNPINNED against any third-party tracker (README, "Unpinned"): it is this project's own statement of salience
 * tracking by dynamic programming.
 *
 * A segment is `rows` rows of contour[rows][264] (float32, three bins per semitone), c[t][b] its cells.
 *
 *   states      The bins min_bin ... max_bin in ascending order, then the unvoiced state U, last in the order.
 *   emissions   e[t][b] = c[t][b],   e[t][U] = threshold.
 *   recurrence  Every operation is a single float32 operation, evaluated as written, nothing fused or reassociated.
 *                   pen[d]  = jump_penalty * (float)d            d = 0 ... max_jump, one rounded product each
 *                   D[0][s] = e[0][s]
 *               and for t >= 1, first normalised against U so that the magnitudes stay bounded however long the segment:
 *                   P[s]    = D[t-1][s] - D[t-1][U]              (P[U] is exactly 0)
 *               The candidates of a voiced target b, IN THIS ORDER: the sources b' in the band with |b - b'| <= max_jump,
 *               ascending, each P[b'] - pen[|b - b'|]; then U, P[U] - voicing_penalty.  The candidates of target U: every
 *               band bin ascending, P[b'] - voicing_penalty; then U, P[U].  The predecessor is the first candidate that is
 *               strictly greater than all before it: TIES GO TO THE LOWEST BIN, AND TO U LAST.
 *                   D[t][s] = e[t][s] + best
 *   path        The last state is the first maximum of D[rows-1] in state order; the rest follow the predecessors.
 *   record      One bp_melody_point per row: RECORD r OF A SEGMENT IS ROW r.  Unvoiced: {-1, 0.0f, 0.0}.  Voiced: the bin,
 *               the cell itself, and
 *                   pitch_midi = 21.0 + ((double)bin + delta) / 3.0
 *               where delta is the parabola of basic_pitch_amd_multipitch.h in float64,
 *                   delta      = 0.5 * (l - r) / ((l - 2.0 * c) + r)
 *               used only when 1 <= bin <= 262 and the cell strictly exceeds both neighbours (of the row, whatever the
 *               band); otherwise delta = 0.0 — a path may sit on a shoulder, and there the parabola has no bound.  Hz are
 *               NOT produced by the library; the Python layer forms them.
 *   status      Per segment (and per decode of a sweep).  0: decoded.  1: a cell anywhere in the segment's rows, whatever
 *               the band, is NaN or has a magnitude above 65536 in float32; every record of such a segment is the unvoiced
 *               record, and no other segment is affected.
 *
 * The defaults are a prototype's, tried on one clip; they are not tuned.
 */
#define BP_MELODY_MAX_JUMP 16
typedef struct bp_melody_params {
  float threshold;       /* emission of the unvoiced state; finite, |threshold| <= 65536  (default 0.3)  */
  float jump_penalty;    /* per bin of movement; 0 ... 65536                              (default 0.05) */
  float voicing_penalty; /* for switching between voiced and unvoiced; 0 ... 65536        (default 0.5)  */
  int32_t max_jump;      /* largest movement in bins, 0 ... BP_MELODY_MAX_JUMP            (default 4)    */
  int32_t min_bin;       /* 0 <= min_bin <= max_bin <= 263                                (default 0)    */
  int32_t max_bin;       /*                                                               (default 263)  */
  int32_t reserved[2];   /* 0 */
} bp_melody_params;      /* 32 bytes */
void bp_melody_params_default(bp_melody_params* p);

typedef struct bp_melody_point {
  int32_t bin;    /* -1: unvoiced */
  float salience; /* c[t][bin], the float32 cell itself; 0.0f unvoiced */
  double pitch_midi;
} bp_melody_point; /* 16 bytes */

/*
 * ---- the melody measures ----
 * The rules of mir_eval.melody restated for a single time base, with no pitch on unvoiced estimate frames; mir_eval is not
 * installed where this project is tested, so the restatement is UNPINNED against it (README, "Unpinned").
 *
 * The reference is ref_pitch[n_frames], doubles on the segment's own frames: 0.0 is unvoiced, anything else a MIDI pitch.
 * A frame is voiced on the estimate side when its record's bin is >= 0.  On the frames voiced on both sides, with
 *     d = 100.0 * (ref - est)                                    in float64
 * pitch_ok counts |d| cmp tol and chroma_ok counts |d - 1200.0 * floor(d / 1200.0 + 0.5)| cmp tol, where tol and cmp are
 * pitch_tolerance_cents and strict (0: <=, 1: <) of bp_score_params.  The Python layer forms the ratios: voicing recall
 * both_voiced / ref_voiced, voicing false alarm (est_voiced - both_voiced) / (n_frames - ref_voiced), raw pitch pitch_ok /
 * ref_voiced, raw chroma chroma_ok / ref_voiced, overall (pitch_ok + n_frames - ref_voiced - est_voiced + both_voiced) /
 * n_frames; a zero denominator gives 0.0.
 */
typedef struct bp_melody_score {
  int64_t n_frames, ref_voiced, est_voiced, both_voiced, pitch_ok, chroma_ok;
} bp_melody_score; /* 48 bytes */

/* rows of emissions a lane of the kernel holds in registers ahead of the recurrence; rows of predecessors a tile of the
 * backtrace stages in LDS; bytes of predecessors per row in device memory (264 bins a byte each, the unvoiced state's in 16
 * bits behind them, rounded up to whole 16-byte words) */
#define BP_MELODY_READ_AHEAD 8
#define BP_MELODY_TILE_ROWS 128
#define BP_MELODY_PRED_STRIDE 272

/*
 * ---- on the host: the checkers, no handle and no device ----
 * The records of one segment into points[0 ... rows), *status the segment's.  BP_ERR_INVALID_ARG for max_points < rows (a
 * row is a record: there is no capacity protocol), a null contour or points with rows > 0, negative rows, a null status, and
 * a malformed p: a threshold that is not finite or beyond +-65536, a penalty that is not finite, negative or above 65536,
 * max_jump outside 0 ... BP_MELODY_MAX_JUMP, min_bin < 0, max_bin > 263, min_bin > max_bin, a non-zero reserved.
 */
int bp_melody_rows(const float* contour, int64_t rows, const bp_melody_params* p, bp_melody_point* points, int64_t max_points,
                   int* status);

/*
 * The counts above of est[0 ... n_frames) against ref_pitch[0 ... n_frames).  Refused: a null out, negative n_frames, null
 * est or ref_pitch with frames, a ref_pitch entry that is negative or not finite (the calls that take a handle name its index
 * in their message), a voiced record whose pitch_midi is not finite, and p as the other score calls refuse it.
 */
int bp_score_melody_frames(const bp_melody_point* est, const double* ref_pitch, int64_t n_frames, const bp_score_params* p,
                           bp_melody_score* out);

/*
 * ---- on the device: segments the caller holds ----
 * Segment i is rows [row_offsets[i], row_offsets[i + 1]) of contour, which lies in host or device memory after mem_kind and is
 * left untouched.  points[row_offsets[i] ... row_offsets[i + 1]) are the records of segment i, byte for byte those of
 * bp_melody_rows on its rows.
 *
 *   room        max_points >= row_offsets[n_segments], else refused with nothing written.
 *   nothing     Zero segments or zero rows: BP_OK (statuses 0) and no device work.
 *   bound       row_offsets[n_segments] <= BP_SWEEP_MAX_ROWS.  There is no bound per segment: a three-minute track is one.
 *   refused     negative n_segments, row_offsets that do not start at 0 or decrease, a bad mem_kind, a null contour with
 *               rows, a null status with segments, negative max_points or too little room or room without a buffer, a
 *               malformed p.
 *
 * How.  One launch, A WORKGROUP PER DECODE and a lane per state (264 bins and U: 320 lanes).  Forward: P is double-buffered
 * in LDS with a halo of BP_MELODY_MAX_JUMP cells of -inf on each side, so the window needs no bounds test (its loads are
 * unrolled, 4 bins on either side when no set of the call has a larger max_jump and 16 otherwise); the unvoiced
 * target's first maximum over the band is reduced within waves and the wave partials are combined through LDS by every
 * lane, which is also the broadcast of D[t][U]; ONE workgroup barrier per frame.  The emissions are read
 * BP_MELODY_READ_AHEAD rows ahead into registers by coalesced 4-byte loads, and the not-finite / magnitude flag comes from
 * the same loads, complete before anything is written.  Predecessors: one byte per state per row, BP_MELODY_PRED_STRIDE
 * bytes a row, in a grow-only pool on the handle — at BP_SWEEP_MAX_ROWS that is 2.3 GB.  Backtrace: tiles of
 * BP_MELODY_TILE_ROWS rows of predecessors are staged in LDS by all lanes, one lane walks the tile and leaves the bins in
 * LDS, then a lane per row writes the record (three cells, the float64 parabola, one 16-byte store).
 * LDS per workgroup: 2 x 296 x 4 bytes of P + 2 x 5 x 8 bytes of wave partials + 128 x 272 bytes of predecessors + 128 x 2
 * bytes of bins + 5 x 5 x 8 bytes of partial counts + 17 x 4 bytes of jump penalties = 37,788 bytes (38,072 as the compiler
 * lays them out).
 * The serial chain over frames is the known weak point: one long track is one workgroup.
 */
int bp_melody_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour, int mem_kind,
                        const bp_melody_params* p, bp_melody_point* points, int64_t max_points, int* status);

/*
 * ---- clips through the model ----
 * The clips as bp_infer_clips_events takes them, through the same driver; a segment is a clip, its rows those of
 * bp_clips_row_offsets.  Outputs, room and bound as above.
 */
int bp_infer_clips_melody(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                          const bp_melody_params* p, bp_melody_point* points, int64_t max_points, int* status);

/*
 * ---- parameter sweeps, scored where the track is ----
 * Decode j is segment decodes[j].segment under sets[decodes[j].params]; decodes == NULL is the cross product, set-major
 * (n_decodes == n_sets * n_segments).  The decode table, BP_SWEEP_MAX_DECODES and the refusals that name an index are those of
 * basic_pitch_amd_sweep.h; a malformed set is refused by its index.  The rows of all DECODES together are bounded by
 * BP_SWEEP_MAX_ROWS (the predecessors of every decode have a region of their own).  ref_pitch runs parallel to the rows of
 * the segments: ref_pitch[row_offsets[i] + r] belongs to row r of segment i; an entry that is negative or not finite is
 * refused, and the message names its index.
 *
 * The contract.  For every decode j with status[j] == 0, scores[j] is what bp_score_melody_frames gives on the records
 * bp_melody_from_maps returns for that segment under that set, with the segment's stretch of ref_pitch and score_params.
 *
 *   status[j]   0; 1: as above.  A non-zero status leaves scores[j] = {n_frames, 0, 0, 0, 0, 0} and touches no other decode.
 *   home        No record is materialised: 52 bytes per decode cross PCIe.
 *
 * How.  The same kernel: the lanes that would write a tile's records add to the counts instead (int64, reduced once per
 * decode).  Device memory beside the predecessors: 8 bytes per row of ref_pitch, 32 per set, 32 per decode, 52 per decode
 * of results.
 */
int bp_melody_sweep_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour, int mem_kind,
                          int64_t n_sets, const bp_melody_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                          const double* ref_pitch, const bp_score_params* score_params, bp_melody_score* scores /*[n_decodes]*/,
                          int* status /*[n_decodes]*/);
int bp_infer_clips_melody_sweep_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                      int64_t n_sets, const bp_melody_params* sets, int64_t n_decodes,
                                      const bp_sweep_decode* decodes, const double* ref_pitch,
                                      const bp_score_params* score_params, bp_melody_score* scores /*[n_decodes]*/,
                                      int* status /*[n_decodes]*/);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_MELODY_H */
