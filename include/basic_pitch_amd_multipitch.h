/* basic_pitch_amd_multipitch.h: multi-pitch estimates from the contour posteriorgram — the f0 peaks of every row, picked,
 * refined and compacted on the device for the segments of a job or for clips through the model, and threshold / band sweeps
 * scored at the frame level where the peaks are, with nothing but counts on their way home.  Same library and handle type as
 * basic_pitch_amd.h, same rules: every argument is checked before anything is queued, errors through bp_last_error(h), a call
 * that fails after queuing returns once the handle's stream has drained. */
#ifndef BASIC_PITCH_AMD_MULTIPITCH_H
#define BASIC_PITCH_AMD_MULTIPITCH_H

#include "basic_pitch_amd_frame_score.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- the definition ----
 * What a multi-pitch estimate is, said once: the host checker, the kernels and the tests' restatement are all held to it.  It
 * is UNPINNED against any third-party peak picker (README, "Unpinned"): it is this project's statement of "threshold + local
 * maxima along frequency + parabolic refinement", the decode the salience literature uses.
 *
 * A segment is `rows` rows of contour[rows][264] (float32, three bins per semitone), c[t][b] its cells.
 *
 *   peak        Bin b of row t is a peak when, compared in float32,
 *                   min_bin <= b <= max_bin,   c[t][b] >= threshold,   c[t][b] > c[t][b-1],   c[t][b] > c[t][b+1]
 *               — the rule of scipy.signal.argrelmax(..., axis=1), the one the project restates for onset peaks.  Bins 0 and
 *               263 are never peaks and a plateau has none, so two peaks are at least two bins apart and a row has AT MOST
 *               131 PEAKS (bins 1, 3, ..., 261).
 *   refinement  In float64, evaluated as written, nothing fused or reassociated.  With l, c, r the cells b-1, b, b+1 widened
 *               to double:
 *                   delta      = 0.5 * (l - r) / ((l - 2.0 * c) + r)
 *                   pitch_midi = 21.0 + ((double)b + delta) / 3.0
 *               Bin 3k is MIDI 21 + k, the mapping of the bend code of note_creation.py.  |delta| <= 0.5, so the peaks of a
 *               row are strictly ascending in pitch_midi.  Hz are NOT produced by the library: 440 * 2^((m - 69) / 12) needs
 *               an exponential that host and device do not share; the Python layer forms it.
 *   point       One bp_f0_point per peak.  A segment's points are ordered by frame, then by bin, both ascending: THE ORDER
 *               IS PART OF THE CONTRACT.
 *   status      Per segment (and per decode of a sweep).  0: picked.  1: a NaN or an infinity anywhere in the segment's
 *               contour rows, whatever the bin range; the segment then has no points and no other segment is affected.
 */
typedef struct bp_mp_params {
  float threshold;  /* finite */
  int32_t min_bin;  /* 1 ... 262, lowest bin that may be a peak  (default 1)   */
  int32_t max_bin;  /* min_bin ... 262, highest                  (default 262) */
  int32_t reserved; /* 0 */
} bp_mp_params;     /* 16 bytes */
void bp_mp_params_default(bp_mp_params* p); /* threshold 0.3, 1, 262, 0 */

typedef struct bp_f0_point {
  int32_t frame;  /* row within its segment */
  float salience; /* c[t][b], the float32 cell itself */
  double pitch_midi;
} bp_f0_point; /* 16 bytes */

#define BP_MP_BINS 264
#define BP_MP_MAX_PEAKS_PER_ROW 131
/* rows the scan of the device call takes in one pass (below); a job with more carries a sum from pass to pass */
#define BP_MP_SCAN_TILE_ROWS 1024

/*
 * ---- on the host: the checker, no handle and no device ----
 * The points of one segment into points[0 ... max_points), *n_points their number, *status the segment's.  When max_points is
 * too small the call returns BP_ERR_INVALID_ARG with *n_points holding the number needed (and *status set); nothing is written
 * to points.  BP_ERR_INVALID_ARG too for a null contour with rows > 0, negative rows or max_points, room without a buffer,
 * null n_points or status, and a malformed p: a non-finite threshold, min_bin < 1, max_bin > 262, min_bin > max_bin, a
 * non-zero reserved.
 */
int bp_multipitch_rows(const float* contour, int64_t rows, const bp_mp_params* p, bp_f0_point* points, int64_t max_points,
                       int64_t* n_points, int* status);

/*
 * The frame-level counts of basic_pitch_amd_frame_score.h with ONE substitution: the estimate side of frame fr is the set of
 * pitch_midi of the points on that frame (distinct values; a point whose frame is outside 0 ... n_frames - 1 counts nowhere).
 * Taken as they stand from that header: the reference side (the refs sounding at time(fr), a multiset), the hit predicate
 * 100 * |ref - est| cmp tolerance in float64, tp as the size of a maximum matching, the five int64 fields.  The greedy that
 * header allows is still a maximum matching for fractional estimates, since every ref still hits an interval of one width:
 * refs in ascending pitch, each the lowest free estimate it hits.  Refused as bp_score_note_frames refuses, and for a point
 * with a non-finite pitch_midi.
 */
int bp_score_f0_frames(const bp_f0_point* est, int64_t n_est, const bp_ref_note* ref, int64_t n_ref, int64_t n_frames,
                       const bp_score_params* p, bp_frame_score* out);

/*
 * ---- on the device: segments the caller holds ----
 * Segment i is rows [row_offsets[i], row_offsets[i + 1]) of contour, which lies in host or device memory after mem_kind and is
 * left untouched.  point_offsets[i] ... point_offsets[i + 1] are the points of segment i, byte for byte those of
 * bp_multipitch_rows on its rows.
 *
 *   capacity    The protocol of basic_pitch_amd_events.h.  When the job needs more than max_points the call fails with
 *               BP_ERR_INVALID_ARG; point_offsets[n_segments] and the message hold the total, status and point_offsets are
 *               complete, nothing has been written to points, and the call can be repeated.
 *   nothing     Zero segments or zero rows: BP_OK with zeroed offsets (statuses 0) and no device work.
 *   bound       row_offsets[n_segments] <= BP_SWEEP_MAX_ROWS.  There is no bound per segment: a three-minute track is one.
 *   refused     negative n_segments, row_offsets that do not start at 0 or decrease, a bad mem_kind, a null contour with
 *               rows, null point_offsets or status, negative max_points or room without a buffer, a malformed p.
 *
 * How.  Three launches and one wait between them: a wave takes a row (coalesced loads, the peak mask by ballot, its popcount
 * the row's count) and flags its segment when a cell is not finite; one workgroup scans the row counts, BP_MP_SCAN_TILE_ROWS
 * a pass, into every row's first slot with the rows of flagged segments counted as empty; the offsets and statuses come home,
 * and only when the total fits the caller's room is the write pass launched, which recomputes the mask and puts each peak at
 * its row's first slot plus its rank within the mask.  Device memory beside the points: 16 bytes a row.
 */
int bp_multipitch_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour, int mem_kind,
                            const bp_mp_params* p, bp_f0_point* points, int64_t max_points,
                            int64_t* point_offsets /*[n_segments+1]*/, int* status);

/*
 * ---- clips through the model ----
 * The clips as bp_infer_clips_events takes them, through the same driver; a segment is a clip, its rows those of
 * bp_clips_row_offsets.  Outputs, capacity protocol and bound as above.
 */
int bp_infer_clips_multipitch(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                              const bp_mp_params* p, bp_f0_point* points, int64_t max_points,
                              int64_t* point_offsets /*[n_clips+1]*/, int* status);

/*
 * ---- threshold and band sweeps, scored where the peaks are ----
 * Decode j is segment decodes[j].segment under sets[decodes[j].params]; decodes == NULL is the cross product, set-major
 * (n_decodes == n_sets * n_segments).  The decode table, BP_SWEEP_MAX_DECODES and the refusals that name an index are those of
 * basic_pitch_amd_sweep.h, the ref validation that of basic_pitch_amd_score.h; a malformed set is refused by its index.  The
 * rows of all DECODES together are bounded by BP_SWEEP_MAX_ROWS.
 *
 * The contract.  For every decode j with status[j] == 0, frames[j] is what bp_score_f0_frames gives on the points
 * bp_multipitch_from_maps returns for that segment under that set, with the refs of the segment, n_frames = its rows, and
 * score_params.
 *
 *   status[j]   0; 1: a NaN or an infinity in the segment's rows; 3: the segment has more than BP_SCORE_MAX_NOTES refs (looked
 *               at first: such a decode's rows are not read).  A non-zero status leaves frames[j] = {n_frames, 0, 0, 0, 0} and
 *               touches no other decode; the caller scores a decode of status 3 with the two host calls above.
 *   home        No point is materialised: 44 bytes per decode cross PCIe.
 *
 * How.  One launch, a workgroup of four waves per decode.  A wave takes a frame: the peak mask from the contour row as
 * above — the map is read, never copied per set —, the refined pitches into the wave's 132 doubles of LDS, then the refs of
 * the segment, which the host has put in ascending pitch with the frames they sound on (the checker's own functions), are
 * tested 64 at a time and those that sound take the lowest free estimate they hit.  Counts are int64.
 * LDS per workgroup: 4 waves x 132 x 8 bytes of pitches + 4 x 5 x 8 bytes of partial sums = 4,384 bytes.  A job whose
 * longest decode has more than 2,048 rows (whole tracks: few decodes, long ones) gets workgroups of 16 waves instead, 16 x
 * 132 x 8 + 16 x 5 x 8 = 17,536 bytes; the counts do not depend on the width.
 * Device memory: 16 bytes per ref, 16 per set, 32 per decode, 48 per decode of results.
 */
int bp_multipitch_sweep_frame_score(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* contour,
                                    int mem_kind, int64_t n_sets, const bp_mp_params* sets, int64_t n_decodes,
                                    const bp_sweep_decode* decodes, const int64_t* ref_offsets /*[n_segments+1]*/,
                                    const bp_ref_note* refs, const bp_score_params* score_params,
                                    bp_frame_score* frames /*[n_decodes]*/, int* status /*[n_decodes]*/);
int bp_infer_clips_multipitch_sweep_frame_score(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate,
                                                int pcm_mem_kind, int64_t n_sets, const bp_mp_params* sets, int64_t n_decodes,
                                                const bp_sweep_decode* decodes, const int64_t* ref_offsets /*[n_clips+1]*/,
                                                const bp_ref_note* refs, const bp_score_params* score_params,
                                                bp_frame_score* frames /*[n_decodes]*/, int* status /*[n_decodes]*/);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_MULTIPITCH_H */
