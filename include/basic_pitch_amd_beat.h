/* basic_pitch_amd_beat.h: tempo and beats — where the pulse of a segment lies and how fast it is, from the onset posteriorgram
 * alone: one global period by autocorrelation under a tempo prior, then the beat frames by a dynamic programme over frames, on
 * the device for the segments of a job or for clips through the model.  Same library and handle type as basic_pitch_amd.h, same
 * rules: every argument is checked before anything is queued, errors through bp_last_error(h), a refusal names the index of
 * the segment, a call that fails after queuing returns once the handle's stream has drained. */
#ifndef BASIC_PITCH_AMD_BEAT_H
#define BASIC_PITCH_AMD_BEAT_H

#include "basic_pitch_amd_align.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- the definition ----
 * What the tempo and the beats of a segment are, said once: the host checker, the kernels and the tests' restatement are all
 * held to it.  It is this project's own statement of tempo estimation by autocorrelation and of beat tracking by dynamic
 * programming, after Ellis 2007 ("Beat tracking by dynamic programming"); it is UNPINNED against librosa and mir_eval
 * (README, "Unpinned").  EVERYTHING BELOW IS EXACT INTEGER ARITHMETIC: the result is a property of the integers and not of an
 * order of summation, so the device may add in any order and still equals the host byte for byte.
 *
 * A segment is `rows` rows of onset[rows][88] (float32).
 *
 *   strength    q(x) is the quantiser of basic_pitch_amd_align.h: 0 ... 1024, clamped, an infinity is a value, only a NaN is a
 *               status.
 *                   o[t] = sum over p in min_pitch ... max_pitch of max(q(onset[t][p]) - threshold_q, 0)
 *               an int32 of at most 88 x 1024 = 90,112.
 *   tempo       The lags are L = lag_min ... min(lag_max, rows - 1).
 *                   A[L] = sum over t = 0 ... rows-1-L of o[t] * o[t+L]        (int64)
 *                   S[L] = A[L] * prior[L]                                      (int64)
 *               The period P is the first maximum of S in ascending L: ties go to the smallest lag.  prior[0 ...
 *               BP_BEAT_MAX_LAG] are int32 values 0 ... 1024 and part of the parameters, that is, DATA: because the table is an
 *               input, libm differences between machines cannot break the byte equality of checker and device.
 *               bp_beat_prior(start_bpm, sd_octaves, prior) fills the log-normal table: entry L is
 *               lrint(1024 * exp(-0.5 * (log2(L / L0) / sd)^2)) with L0 = 60 * 22050 / 256 / start_bpm, and entry 0 is 0.
 *   scale       m = floor(sum of o[t]^2 / sum of o[t]), the contraharmonic mean: for a sparse pulse train it is about the height
 *               of a pulse, so `tightness` means the same on quiet and on loud material.
 *   penalty     dmin = max(1, P / 2) and dmax = 2 * P (integer division);
 *                   pen[d] = floor(tightness * m * (d - P)^2 / (P * P))        for d = dmin ... dmax, int64
 *   recurrence  C[t] = o[t] + best, int64.  The candidates for `best` come in this order: first "start", with value 0 and no
 *               predecessor, then C[t-d] - pen[d] for d = dmin ... dmax with t - d >= 0, in ascending d.  The predecessor is the
 *               first candidate that is STRICTLY GREATER than all before it: ties go to the start, and otherwise to the
 *               smallest d.
 *   path        The last beat is the first maximum of C[t] over t in [max(0, rows - P), rows).  The rest of the path follows
 *               the predecessors back to a start.  Beats come out as ascending int32 frame indices.
 *   refined     period_refined = P + 0.5 * (l - r) / ((l - 2c) + r), where l, c, r are S[P-1], S[P], S[P+1] converted to
 *               float64 and every operation is one IEEE float64 operation as written.  The formula is used only when
 *               lag_min < P < the last admissible lag and S[P] strictly exceeds both neighbours (compared as the float64 values
 *               c > l and c > r, so the denominator is never 0); otherwise period_refined is (double)P.  Beats per minute are not produced by the library: 60 * 22050 / 256 / period_refined.
 *   status      Per segment.  0: decoded.  1: a NaN anywhere in the segment's onset rows, in whatever pitch; this is decided
 *               first.  2: no pulse — rows - 1 < lag_min, or every S[L] is 0, as with silence or with everything under the
 *               threshold.  A non-zero status gives period 0, no beats, score 0 and refined 0.0, and touches no other segment.
 *
 * Known limits, as they are.  The defaults are a prototype's and are not tuned.  The estimate is ONE GLOBAL TEMPO per segment;
 * tempo changes are followed only as far as pen allows.  Leading and trailing beats are not trimmed: an isolated onset before
 * the first beat or after the last one can add a beat.  Octave errors follow the prior: a pulse at lag 29 reads as period 58
 * under the default prior.
 */
#define BP_BEAT_MAX_LAG 256
#define BP_BEAT_PITCHES 88
#define BP_BEAT_Q_ONE 1024
#define BP_BEAT_MAX_TIGHTNESS 1024
#define BP_BEAT_MAX_ROWS 524288 /* 2^19 rows of one segment, about 100 minutes */

typedef struct bp_beat_params {
  int32_t threshold_q;                /* 0 ... 1024, in units of 1/1024             (default 307) */
  int32_t min_pitch, max_pitch;       /* 0 <= min_pitch <= max_pitch <= 87         (default 0, 87) */
  int32_t lag_min, lag_max;           /* 2 <= lag_min <= lag_max <= BP_BEAT_MAX_LAG (default 21, 172: about 246 to 30 beats a minute) */
  int32_t tightness;                  /* 0 ... 1024                                 (default 4) */
  int32_t reserved[2];                /* 0 */
  int32_t prior[BP_BEAT_MAX_LAG + 1]; /* 0 ... 1024 each; entry L weighs lag L     (default bp_beat_prior(120, 1.0)) */
  int32_t reserved_tail;              /* 0 */
} bp_beat_params;                     /* 1064 bytes */

typedef struct bp_beat_summary {
  int32_t status;        /* 0, 1 (a NaN) or 2 (no pulse) */
  int32_t period;        /* P in frames; 0 with a non-zero status */
  int64_t n_beats;
  int64_t score;         /* S[P] */
  double period_refined; /* frames; 0.0 with a non-zero status */
} bp_beat_summary;       /* 32 bytes */

/* the defaults above, the table filled by bp_beat_prior(120.0, 1.0, p->prior) */
void bp_beat_params_default(bp_beat_params* p);
/* prior[0 ... BP_BEAT_MAX_LAG] of a log-normal tempo prior around start_bpm, sd_octaves wide.  BP_ERR_INVALID_ARG for a null
 * table, a start_bpm or an sd_octaves that is not finite and above 0. */
int bp_beat_prior(double start_bpm, double sd_octaves, int32_t* prior);

/*
 * ---- bounds ----
 * BP_BEAT_MAX_LAG = 256: 5.8 beats a minute at the slow end, far below music; it fixes the table, the widest candidate set
 * (dmin = 128 ... dmax = 512: 385 candidates, at most 7 a lane of a wave) and the LDS ring of the path kernel.
 * Rows of one segment: at most BP_BEAT_MAX_ROWS = 2^19.  The rows of all segments together: at most BP_SWEEP_MAX_ROWS.
 * Overflow, with o <= 90,112 < 2^17 and rows <= 2^19:
 *     A[L] * 1024 < 90,112^2 * 2^19 * 2^10 < 2^62                           S fits int64
 *     sum of o[t]^2 < 2^34 * 2^19 = 2^53                                    m <= 90,112
 *     tightness * m * (d - P)^2 <= 2^10 * 2^17 * 2^16 = 2^43 < 2^44         the numerator of pen; pen < 2^44
 *     0 <= C[t] <= (t + 1) * 90,112 < 2^19 * 2^17 = 2^36 < 2^40             C; a candidate C - pen lies in (-2^44, 2^40)
 * The path kernel packs (candidate + 2^44, 1023 - d) into one 64-bit key of 46 + 10 bits; the predecessor is one uint16 a row.
 *
 * Room for beats.  Two beats are at least dmin = max(1, P / 2) >= max(1, lag_min / 2) frames apart and a segment of rows <=
 * lag_min has none, so a segment has at most
 *     bp_beats_capacity(rows, lag_min) = rows <= lag_min ? 0 : (rows - 1) / max(1, lag_min / 2) + 1
 * beats: it follows from the rows and lag_min alone.  -1 for negative rows or a lag_min outside 2 ... BP_BEAT_MAX_LAG.
 */
int64_t bp_beats_capacity(int64_t rows, int32_t lag_min);

#define BP_BEAT_RING 1024      /* int64 entries of C the path kernel keeps in LDS: >= dmax + one block of dmin frames = 640 */
#define BP_BEAT_TEMPO_ROWS 256 /* rows of one tile of the tempo kernel */
#define BP_BEAT_TEMPO_LAGS 64  /* lags of one tile of the tempo kernel */
#define BP_BEAT_PATH_WAVES 16  /* waves of the path kernel's workgroup: frames of a block computed at once */

/*
 * ---- on the host: the checker, no handle and no device ----
 * Tempo and beats of one segment: *summary, and beats[0 ... summary->n_beats).  BP_ERR_INVALID_ARG for negative rows, rows >
 * BP_BEAT_MAX_ROWS, null onset with rows, a null summary, a malformed p (threshold_q outside 0 ... 1024, pitches outside
 * 0 <= min_pitch <= max_pitch <= 87, lags outside 2 <= lag_min <= lag_max <= 256, tightness outside 0 ... 1024, a prior entry
 * outside 0 ... 1024, a non-zero reserved word), max_beats < bp_beats_capacity(rows, p->lag_min) or room without a buffer.
 * rows == 0: status 2.
 */
int bp_beat_rows(const float* onset, int64_t rows, const bp_beat_params* p, int32_t* beats, int64_t max_beats,
                 bp_beat_summary* summary);

/*
 * ---- on the device: segments the caller holds ----
 * Segment i is rows [row_offsets[i], row_offsets[i + 1]) of onset, which lies in host or device memory after mem_kind and is
 * left untouched.  Beats are ONE COMPACT int32 array: segment i's beats are beats[beat_offsets[i] ... beat_offsets[i + 1]),
 * beat_offsets an output of n_segments + 1 entries; summaries[i], the offsets and the beats are byte for byte those of
 * bp_beat_rows on the segment.
 *
 *   room        max_beats >= sum over segments of bp_beats_capacity(rows_i, p->lag_min), checked before anything is queued;
 *               with too little room the call is refused and nothing is written.
 *   nothing     Zero segments, and segments without rows (status 2), do no device work: they are settled on the host.
 *   refused     negative n_segments, row_offsets that do not start at 0 or decrease, a bad mem_kind, null onset with rows, null
 *               summaries or beat_offsets with segments, too little room or room without a buffer, a malformed p; a segment of
 *               more than BP_BEAT_MAX_ROWS rows (the segment is named); more than BP_SWEEP_MAX_ROWS rows in all.
 *
 * How (csrc/beat.hip).  Three launches.  STRENGTH: row-parallel over all segments, 16-byte loads, eight lanes a
 * row; the NaN flag comes from the same loads, sum o and sum o^2 are reduced in the block and added by ONE integer atomic per
 * block.  TEMPO: tiles of BP_BEAT_TEMPO_ROWS rows x BP_BEAT_TEMPO_LAGS lags, int64 products reduced per block, integer atomics
 * into A[segment][lag], so that one long track spreads over the chip.  PATH: a workgroup per segment picks the period and
 * refines it, then runs the recurrence A BLOCK OF dmin FRAMES AT A TIME — frames t ... t + dmin - 1 depend only on frames at
 * most t - dmin back, so a wave takes a frame and the workgroup meets ONCE PER BLOCK, not once per frame —, the candidates of a
 * frame over the lanes of its wave, C in an LDS ring, pen in registers, the best (value, smallest d) by data-parallel
 * primitives; the ending and the backtrace run in the same kernel.
 */
int bp_beats_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* onset, int mem_kind,
                       const bp_beat_params* p, bp_beat_summary* summaries /*[n_segments]*/, int32_t* beats, int64_t max_beats,
                       int64_t* beat_offsets /*[n_segments+1]*/);

/*
 * ---- clips through the model ----
 * The clips as bp_infer_clips_events takes them, through the same driver; a segment is a clip, its rows those of
 * bp_clips_row_offsets.  Outputs, room and bounds as above.
 */
int bp_infer_clips_beats(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                         const bp_beat_params* p, bp_beat_summary* summaries /*[n_clips]*/, int32_t* beats, int64_t max_beats,
                         int64_t* beat_offsets /*[n_clips+1]*/);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_BEAT_H */
