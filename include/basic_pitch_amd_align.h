/* basic_pitch_amd_align.h: forced alignment — reference notes that are NOT on the audio's time base (a MIDI score, the
 * annotations of another take, labels that sit off or drift) are aligned to the note and onset posteriorgrams of a segment
 * by a monotone dynamic programme, on the device for the segments of a job or for clips through the model.  The aligned notes
 * are bp_ref_notes again and go into the score calls of basic_pitch_amd_score.h.  Same library and handle type as
 * basic_pitch_amd.h, same rules: every argument is checked before anything is queued, errors through bp_last_error(h), a
 * refusal names the index of the segment or state, a call that fails after queuing returns once the handle's stream has
 * drained. */
#ifndef BASIC_PITCH_AMD_ALIGN_H
#define BASIC_PITCH_AMD_ALIGN_H

#include "basic_pitch_amd_score.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- the definition ----
 * What the alignment of a segment is, said once: the host checker, the kernels and the tests' restatement are all held to
 * it.  It is UNPINNED against any third-party aligner (README, "Unpinned"): it is this project's own statement of
 * score-to-audio alignment by dynamic programming.
 *
 * A segment is `rows` rows of note[rows][88] and onset[rows][88] (float32).  Its score is S >= 1 states IN ORDER; a state
 * says which pitches sound while it lasts (`active`), which of them start with it (`begins`), and in which window of frames
 * its first frame must lie.  Every frame is in exactly one state, and the state index rises by 0 or 1 per frame.
 *
 *   quantise    q(x) = (int)floorf(min(max(x, 0.0f), 1.0f) * 1024.0f + 0.5f), 0 ... 1024; qn[t][p] = q(note[t][p]),
 *               qo[t][p] = q(onset[t][p]).
 *   gains       int32, exact:
 *                   g[t][j] = sum over p in active_j of qn[t][p]  -  threshold_q * |active_j|
 *                   b[t][j] = onset_weight * sum over p in begins_j of qo[t][p]
 *               g is, up to a constant of the frame, minus the L1 distance between the quantised row and the state's
 *               piano-roll when threshold_q is 512: a sounding pitch gains what it has above the threshold and a silent one
 *               gains nothing, so a state is paid for the energy it explains.  b pays for entering where the onsets are.
 *   recurrence  int64.  With "unreachable" below every number:
 *                   D[0][0] = g[0][0] + b[0][0]   if earliest_0 <= 0;  every other D[0][j] is unreachable
 *               and for t >= 1
 *                   stay    = D[t-1][j] + g[t][j]
 *                   enter   = D[t-1][j-1] + g[t][j] + b[t][j]       (j >= 1, admissible only when earliest_j <= t <= latest_j)
 *                   D[t][j] = max(stay, enter)
 *               An unreachable source gives an unreachable candidate: unreachable stays unreachable.  ENTER ONLY WHEN
 *               STRICTLY GREATER: ties stay.  The result is defined by these integers, not by an order of operations: any
 *               exact arithmetic gives it.
 *   path        ends in (rows - 1, S - 1) and follows the decisions back.  first_frame[j] is the frame at which state j was
 *               entered, first_frame[0] = 0.  Because ties stay, among all optimal paths this is the one with the smallest
 *               first_frame[S - 1], then the smallest first_frame[S - 2], and so on.
 *   status      Per segment.  0: aligned; total = D[rows - 1][S - 1].  1: a cell anywhere in the segment's note or onset
 *               rows, in whatever pitch, is NaN.  2: infeasible — (rows - 1, S - 1) is unreachable: more states than rows,
 *               or windows that cannot be met.  With a non-zero status every first_frame of the segment is -1 and total is 0,
 *               and no other segment is affected.  Status 1 is decided before status 2.
 *
 * The defaults are a prototype's, tried on one clip; they are not tuned.
 */
typedef struct bp_align_state {
  uint64_t active[2];       /* bit p: pitch 21 + p sounds; bits >= 88 must be 0 */
  uint64_t begins[2];       /* the pitches that start at this state; a subset of active */
  int32_t earliest, latest; /* the state's first frame lies in earliest ... latest; 0 <= earliest <= latest, INT32_MAX: free */
} bp_align_state;           /* 40 bytes */

typedef struct bp_align_params {
  int32_t threshold_q;  /* 0 ... 1024, in units of 1/1024   (default 307) */
  int32_t onset_weight; /* 0 ... 16                          (default 2)   */
  int32_t reserved[2];  /* 0 */
} bp_align_params;      /* 16 bytes */
void bp_align_params_default(bp_align_params* p);

#define BP_ALIGN_PITCHES 88
#define BP_ALIGN_Q_ONE 1024
#define BP_ALIGN_MAX_ONSET_WEIGHT 16

/*
 * ---- bounds ----
 * BP_ALIGN_MAX_STATES, per segment.  The recurrence is one workgroup of BP_ALIGN_LANES = 1024 lanes (16 waves, 4 per SIMD) per
 * segment, and a lane holds the int64 D of its states in registers.  16 waves on a compute unit leave a lane 512 / 4 = 128
 * vector registers.  Per state a lane keeps 2 registers of D, 2 x BP_ALIGN_READ_AHEAD_WIDE = 8 of gains read ahead, 2 of the
 * window, 1 index and about 7 temporaries while it is computed: 20, beside some 36 that do not depend on the count; four states
 * are 116 of the 128 by the compiler's report, eight would be near 200 and spill.
 *     BP_ALIGN_MAX_STATES = 1024 lanes x 4 states = 4096
 * LDS at that size, of the 163,840 bytes a compute unit has: a backtrace tile of BP_ALIGN_TILE_ROWS = 128 rows x 4096 / 8
 * bytes of predecessor bits = 65,536 bytes, the wave edges 2 x 4 x 16 x 8 = 1,024 bytes, 16 bytes of flags: 66,576.
 *
 * Rows.  The rows of all segments together are at most BP_SWEEP_MAX_ROWS.
 *
 * BP_ALIGN_MAX_CELLS bounds sum over segments of rows_i * S_i: the gains are materialised (DESIGN.md 22 says why), 8 bytes a
 * cell (g and g + b, int32 each), and the predecessor is one bit a cell in rows of whole 64-bit words.
 *     268,435,456 cells x 8 bytes = 2,147,483,648 bytes of gains, and 33,554,432 bytes of predecessor bits at the least
 * A three-minute piece of 15,500 rows against 4096 states is 63,488,000 cells, 508 MB.
 */
#define BP_ALIGN_LANES 1024
#define BP_ALIGN_SMALL_LANES 256 /* a job whose largest score has no more states runs workgroups of this size */
#define BP_ALIGN_STATES_PER_LANE 4
#define BP_ALIGN_MAX_STATES (BP_ALIGN_LANES * BP_ALIGN_STATES_PER_LANE)
#define BP_ALIGN_MAX_CELLS 268435456
#define BP_ALIGN_READ_AHEAD 8      /* frames of gains a lane holds ahead of the recurrence, up to two states a lane */
#define BP_ALIGN_READ_AHEAD_WIDE 4 /* with four states a lane */
#define BP_ALIGN_TILE_ROWS 128     /* rows of predecessor bits a tile of the backtrace stages in LDS */
#define BP_ALIGN_EMIT_ROWS 32      /* rows and states of one matrix-core tile of the emissions */

/*
 * ---- on the host: the checker, no handle and no device ----
 * The alignment of one segment: first_frame[0 ... n_states), *total, *status.  BP_ERR_INVALID_ARG for max_states < n_states,
 * negative rows or n_states, rows > 0 with n_states == 0 (a path needs a state), n_states > BP_ALIGN_MAX_STATES, null note or
 * onset with rows, null states or first_frame with states, a null total or status, a malformed p (threshold_q outside
 * 0 ... 1024, onset_weight outside 0 ... 16, a non-zero reserved) and a malformed state (a bit >= 88, begins outside active,
 * earliest < 0, earliest > latest).  rows == 0: status 0 without states, status 2 with.
 */
int bp_align_rows(const float* note, const float* onset, int64_t rows, const bp_align_state* states, int64_t n_states,
                  const bp_align_params* p, int32_t* first_frame, int64_t max_states, int64_t* total, int* status);

/*
 * ---- on the device: segments the caller holds ----
 * Segment i is rows [row_offsets[i], row_offsets[i + 1]) of note and onset, which lie in host or device memory after mem_kind
 * and are left untouched, and states [state_offsets[i], state_offsets[i + 1]) of states (host memory).  first_frame runs
 * parallel to states; first_frame, total[i] and status[i] are byte for byte those of bp_align_rows on the segment.
 *
 *   room        max_states >= state_offsets[n_segments], else refused with nothing written.
 *   nothing     Zero segments, and segments without rows or without states, do no device work.
 *   refused     negative n_segments, row_offsets or state_offsets that do not start at 0 or decrease, a bad mem_kind, null
 *               note or onset with rows, null states with states, null total or status with segments, too little room or
 *               room without a buffer, a malformed p; a segment with rows and no state, with more than BP_ALIGN_MAX_STATES
 *               states (the segment is named), a malformed state (the state is named); more than BP_SWEEP_MAX_ROWS rows or
 *               BP_ALIGN_MAX_CELLS cells in all.
 *
 * How (csrc/align.hip).  Three launches.  EMISSIONS: [rows x 88] . [88 x S] twice (note / active, onset /
 * begins) on the f16 matrix cores, tiles of 32 rows x 32 states a wave; the maps are quantised as they are loaded and the NaN
 * flag comes from the same loads; the operands 0 ... 1024 and 0 / 1 are exact in f16 and every partial sum is an integer of
 * at most 88 x 1024 < 2^24, so the fp32 accumulators hold exact integers whatever the order of summation.  RECURRENCE: a
 * workgroup per segment, a state per lane and up to four above 1024, D in registers, the neighbour's D[t-1][j-1] by a
 * data-parallel shift within a wave and through LDS across waves, ONE barrier per frame, the gains read ahead, the
 * predecessor ONE BIT per cell by a ballot.  BACKTRACE, in the same workgroup: tiles of BP_ALIGN_TILE_ROWS rows of bits
 * through LDS, one lane walks.  The serial chain over frames is the known weak point: one long piece is one workgroup.
 */
int bp_align_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, const float* onset,
                       int mem_kind, const int64_t* state_offsets /*[n_segments+1]*/, const bp_align_state* states,
                       const bp_align_params* p, int32_t* first_frame, int64_t max_states, int64_t* total /*[n_segments]*/,
                       int* status /*[n_segments]*/);

/*
 * ---- clips through the model ----
 * The clips as bp_infer_clips_events takes them, through the same driver; a segment is a clip, its rows those of
 * bp_clips_row_offsets.  Outputs, room and bounds as above.
 */
int bp_infer_clips_align(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                         const int64_t* state_offsets /*[n_clips+1]*/, const bp_align_state* states, const bp_align_params* p,
                         int32_t* first_frame, int64_t max_states, int64_t* total /*[n_clips]*/, int* status /*[n_clips]*/);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_ALIGN_H */
