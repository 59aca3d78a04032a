/* basic_pitch_amd_chord.h: chords and key — which chord sounds in every row of a segment and what key the segment is in, from
 * the note posteriorgram alone: a chroma per row, pooled over units (frames, or the stretches between given boundaries such as
 * beats), a Viterbi path over a table of chord templates with one switching penalty (a Potts model), and a key by profile
 * correlation, on the device for the segments of a job or for clips through the model.  Same library and handle type as
 * basic_pitch_amd.h, same rules: every argument is checked before anything is queued, errors through bp_last_error(h), a
 * refusal names the index of the segment, a call that fails after queuing returns once the handle's stream has drained. */
#ifndef BASIC_PITCH_AMD_CHORD_H
#define BASIC_PITCH_AMD_CHORD_H

#include "basic_pitch_amd_beat.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- the definition ----
 * What the chords and the key of a segment are, said once: the host checker, the kernels and the tests' restatement are all
 * held to it.  It is this project's own statement of template chord recognition with a switching penalty and of profile key
 * finding; it is UNPINNED against any third-party chord or key estimator (README, "Unpinned").  EVERYTHING BELOW IS EXACT
 * INTEGER ARITHMETIC, int64 wherever a bound below exceeds 31 bits: the result is a property of the integers and not of an
 * order of summation, so the device may add in any order and still equals the host byte for byte.
 *
 * A segment is `rows` rows of note[rows][88] (float32).  Pitch p is MIDI 21 + p; its pitch class is (p + 9) % 12, C = 0.
 *
 *   chroma      q(x) is the quantiser of basic_pitch_amd_align.h: 0 ... 1024, clamped, an infinity is a value, only a NaN is a
 *               status.
 *                   c[t][k] = sum over p in min_pitch ... max_pitch with class k of max(q(note[t][p]) - threshold_q, 0)
 *               at most 8 x 1024 = 2^13 (a class has at most 8 pitches).
 *   units       Without boundaries unit u is frame u.  With boundaries B_0 < B_1 < ... < B_{n-1}, all strictly inside
 *               0 < B < rows, the units are [0, B_0), [B_0, B_1), ..., [B_{n-1}, rows): n + 1 of them.  len(u) is the unit's
 *               number of frames and
 *                   cu[u][k] = sum of c[t][k] over the unit's frames
 *               which is below 2^32.
 *   scale       m = floor(sum of c^2 / sum of c) over all frames and classes of the segment, the contraharmonic mean as in
 *               basic_pitch_amd_beat.h: about the height of what sounds, so bias and switch_penalty mean the same on quiet and
 *               on loud material.  m <= 2^13.
 *   states      n_states is 1 ... BP_CHORD_MAX_STATES.  State s has weights[s][12] and bias[s], each in -1024 ... 1024.  They
 *               are DATA, part of the parameters like the beat prior: the library knows no chord names.  By convention state 0
 *               of a table is "no chord".
 *   emission        e[u][s] = len(u) * bias[s] * m + sum over k of weights[s][k] * cu[u][k]
 *               in magnitude below len(u) * 2^28.
 *   recurrence  (Potts)  pen[u] = len(u) * switch_penalty * m, switch_penalty in 0 ... 1024.  D[0][s] = e[0][s].  For u >= 1 let
 *               a be the first maximum of D[u-1][.] in ascending state order.  State s STAYS, with predecessor s, unless
 *               D[u-1][a] - pen[u] is STRICTLY GREATER than D[u-1][s]; then the predecessor is a.  Ties stay.
 *                   D[u][s] = e[u][s] + best                                   |D| < 2^19 * 2^28 = 2^47
 *   path        The last state is the first maximum of D[last][.] in state order; the predecessors are followed back from
 *               there.  Every ROW gets its unit's state as a uint8: one label per row, so a row is a record and there is no
 *               capacity protocol (max_labels >= the rows, checked before anything is queued).  n_changes counts the units
 *               u >= 1 whose state differs from that of unit u - 1.
 *   key             Ctot[k] = sum over t of c[t][k]
 *                   K[j] = sum over k of key_profile[j / 12][(k - j % 12 + 12) % 12] * Ctot[k]       j = 0 ... 23
 *               (the major tonics C ... B, then the minor tonics).  Profile entries are in -1024 ... 1024 and are data.  The key
 *               is the first maximum of K in ascending j.
 *   status      Per segment.  0: decoded.  1: a NaN anywhere in the segment's note rows, in whatever pitch; this is decided
 *               first.  2: nothing sounds — no rows, or sum of c = 0, as with silence or with everything under the threshold.
 *               A non-zero status gives every label 0, key -1, n_units 0, n_changes 0 and scores 0, and touches no other
 *               segment.
 *
 * Known limits, as they are.  The defaults are a prototype's and are not tuned.  There is ONE KEY per segment: modulations
 * are not followed.  There is no bass and no inversion: C:maj and its inversions are one state.  Templates see
 * octave-folded energy only, so a chord and the same pitch classes spread over five octaves are one chroma.
 * Planted triads (tests/test_chord_cpu.py): clean triads of the majmin table in runs of frame units, every sounding pitch at
 * one level, with silence between some, come back exactly under the default parameters, silence as state 0, when every run
 * has AT LEAST 22 FRAMES (a quarter of a second), and not with 21.  The figure follows from the defaults: a switch costs 128 m
 * a frame, silence earns N 12 m a frame over a chord and a triad earns 12 m a frame over one that shares two of its tones, so
 * a chord - silence - the same chord, or C:maj - A:min - C:maj, pays two switches (256 m) only from 22 frames on (264 m).
 */
#define BP_CHORD_MAX_STATES 64
#define BP_CHORD_CLASSES 12
#define BP_CHORD_PITCHES 88
#define BP_CHORD_Q_ONE 1024
#define BP_CHORD_MAX_WEIGHT 1024  /* the magnitude of a weight, a bias and a profile entry */
#define BP_CHORD_MAX_PENALTY 1024 /* the largest switch_penalty */
#define BP_CHORD_MAX_ROWS 524288  /* 2^19 rows of one segment, about 100 minutes */

typedef struct bp_chord_params {
  int32_t threshold_q;                                        /* 0 ... 1024, in units of 1/1024 (default 307) */
  int32_t min_pitch, max_pitch;                               /* 0 <= min_pitch <= max_pitch <= 87 (default 0, 87) */
  int32_t n_states;                                           /* 1 ... BP_CHORD_MAX_STATES (default 25: majmin) */
  int32_t switch_penalty;                                     /* 0 ... 1024 (default 128) */
  int32_t reserved[3];                                        /* 0 */
  int32_t bias[BP_CHORD_MAX_STATES];                          /* -1024 ... 1024; entries from n_states on are not used */
  int32_t weights[BP_CHORD_MAX_STATES][BP_CHORD_CLASSES];     /* -1024 ... 1024; rows from n_states on are not used */
  int32_t key_profile[2][BP_CHORD_CLASSES];                   /* -1024 ... 1024: major, minor (default Krumhansl-Kessler) */
} bp_chord_params;                                            /* 3456 bytes */

typedef struct bp_chord_summary {
  int32_t status;    /* 0, 1 (a NaN) or 2 (nothing sounds) */
  int32_t key;       /* 0 ... 11 C ... B major, 12 ... 23 C ... B minor; -1 with a non-zero status */
  int32_t n_units;   /* 0 with a non-zero status */
  int32_t n_changes;
  int64_t score;     /* the final D */
  int64_t key_score; /* K[key] */
} bp_chord_summary;  /* 32 bytes */

/* the vocabularies of bp_chord_templates */
#define BP_CHORD_VOCAB_MAJMIN 0   /* N, 12 maj, 12 min: 25 states */
#define BP_CHORD_VOCAB_TRIADS 1   /* N, maj, min, dim, aug: 49 states */
#define BP_CHORD_VOCAB_SEVENTHS 2 /* N, maj, min, 7, maj7, min7: 61 states */

/* threshold 307, pitches 0 ... 87, switch_penalty 128, the majmin table and the Krumhansl-Kessler profiles */
void bp_chord_params_default(bp_chord_params* p);
/* n_states, bias and weights of one vocabulary (the other fields are left; entries beyond n_states become 0).  State 0 is N:
 * weights 0 and bias 12.  The others come quality-major, root ascending from C, with bias 0: a chord of n tones has weight
 * 12 - n on its tones and -n elsewhere, so every row sums to 0.  Tones above the root: maj 0 4 7, min 0 3 7, dim 0 3 6, aug
 * 0 4 8, 7 0 4 7 10, maj7 0 4 7 11, min7 0 3 7 10.  BP_ERR_INVALID_ARG for a null p or an unknown vocabulary. */
int bp_chord_templates(int vocabulary, bp_chord_params* p);
/* key_profile of the Krumhansl-Kessler profiles
 *     major 6.35 2.23 3.48 2.33 4.38 4.09 2.52 5.19 2.39 3.66 2.29 2.88
 *     minor 6.33 2.68 3.52 5.38 2.60 3.53 2.54 4.75 3.98 2.69 3.34 3.17
 * each with its mean removed, scaled to unit norm x 1024 and rounded by lrint.  The table is an input and not part of the byte
 * equality, so libm differences between machines cannot break it.  BP_ERR_INVALID_ARG for a null p. */
int bp_chord_key_profiles(bp_chord_params* p);

/*
 * ---- bounds ----
 * Rows of one segment: at most BP_CHORD_MAX_ROWS = 2^19.  The rows of all segments together: at most BP_SWEEP_MAX_ROWS.
 * Overflow, with c <= 2^13, rows <= 2^19 and every table entry <= 2^10 in magnitude:
 *     cu <= 2^13 * (2^19 - 1) < 2^32                                        a unit of a segment with boundaries is shorter than it
 *     sum of c^2 <= 12 * 2^26 * 2^19 < 2^49                                 m <= 2^13
 *     |len * bias * m| <= len * 2^23,  |sum of weights * cu| <= 12 * 2^10 * len * 2^13 < len * 2^27       |e| < len * 2^28
 *     |D| < 2^19 * 2^28 = 2^47,  pen <= 2^19 * 2^10 * 2^13 = 2^42            D - pen fits int64 with room
 *     |K| <= 12 * 2^10 * 2^13 * 2^19 < 2^46
 * The path kernel packs (D + 2^48, 63 - s) into one 64-bit key of 49 + 6 bits, and (K + 2^48, 63 - j) likewise.
 */
#define BP_CHORD_CHROMA_ROWS 32 /* rows of one block of the chroma kernel */
#define BP_CHORD_TRACE_TILE 512 /* records of one tile of the backtrace */
#define BP_CHORD_PATH_WAVES 4   /* waves of the path kernel's workgroup: segments decoded side by side */

/*
 * ---- on the host: the checker, no handle and no device ----
 * Chords and key of one segment: *summary, and labels[0 ... rows).  bounds: n_bounds boundaries, or null with n_bounds 0 for
 * frame units.  BP_ERR_INVALID_ARG, with nothing written, for negative rows, rows > BP_CHORD_MAX_ROWS, null note with rows, a
 * null summary, a malformed p (threshold_q outside 0 ... 1024, pitches outside 0 <= min_pitch <= max_pitch <= 87, n_states
 * outside 1 ... 64, switch_penalty outside 0 ... 1024, a bias, weight or profile entry outside -1024 ... 1024, a
 * non-zero reserved word), negative n_bounds or boundaries without an array, boundaries that are not strictly ascending
 * inside 0 < B < rows, max_labels < rows or room without a buffer.  rows == 0: status 2.
 */
int bp_chord_rows(const float* note, int64_t rows, const bp_chord_params* p, const int32_t* bounds, int64_t n_bounds,
                  uint8_t* labels, int64_t max_labels, bp_chord_summary* summary);

/*
 * ---- on the device: segments the caller holds ----
 * Segment i is rows [row_offsets[i], row_offsets[i + 1]) of note, which lies in host or device memory after mem_kind and is
 * left untouched.  Its boundaries are bounds[bound_offsets[i] ... bound_offsets[i + 1]), the layout of beats / beat_offsets of
 * bp_beats_from_maps, so that call's output goes in as it is (but for a beat at frame 0, which is no boundary).  bounds and
 * bound_offsets may BOTH be null: frame units everywhere; a segment without boundaries has frame units.  labels[r] is the
 * label of row r of note, parallel to its rows; summaries[i] and the labels are byte for byte those of bp_chord_rows on
 * the segment.
 *
 *   room        max_labels >= row_offsets[n_segments], checked before anything is queued; with too little room the call is
 *               refused and nothing is written.
 *   nothing     Zero segments, and segments without rows (status 2), do no device work: they are settled on the host.
 *   refused     negative n_segments, row_offsets that do not start at 0 or decrease, a bad mem_kind, null note with rows, null
 *               summaries with segments, too little room or room without a buffer, a malformed p; one of bounds and
 *               bound_offsets without the other, bound_offsets that do not start at 0 or decrease; a segment whose boundaries
 *               are not strictly ascending inside 0 < B < rows, or of more than BP_CHORD_MAX_ROWS rows (the segment is named);
 *               more than BP_SWEEP_MAX_ROWS rows in all.
 *
 * How (csrc/chord.hip).  CHROMA: row-parallel over all segments, a block takes BP_CHORD_CHROMA_ROWS rows by
 * 16-byte loads, quantises and folds them to one 32-byte row of uint16[16]; the NaN flag comes from the same loads; sum c,
 * sum c^2 and Ctot[12] are reduced in the block and added by ONE integer atomic per value per block.  POOL: only where a
 * segment has boundaries, unit-parallel sums: they do not depend on the recurrence and do not sit on its chain.  PATH: ONE WAVE
 * PER SEGMENT, one lane per state, BP_CHORD_PATH_WAVES waves a workgroup each with a segment of its own: NO BARRIER sits on the
 * chain.  A lane holds its 12 weights and its bias in registers; the unit's sums are wave-uniform and fetched a chunk ahead;
 * the first maximum is one cross-lane reduction of the packed key; the ballot of the strict comparison IS the unit's
 * predecessor mask and goes out with a as one 16-byte record; the key is picked in the same kernel; the backtrace walks
 * tiles of BP_CHORD_TRACE_TILE records staged in LDS.  LABEL: one byte a row.
 */
int bp_chords_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, int mem_kind,
                        const bp_chord_params* p, const int64_t* bound_offsets /*[n_segments+1] or null*/, const int32_t* bounds,
                        bp_chord_summary* summaries /*[n_segments]*/, uint8_t* labels, int64_t max_labels);

/*
 * ---- clips through the model ----
 * The clips as bp_infer_clips_events takes them, through the same driver; a segment is a clip, its rows those of
 * bp_clips_row_offsets, and the boundaries are frames of the clip's rows.  Outputs, room and bounds as above.
 */
int bp_infer_clips_chords(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                          const bp_chord_params* p, const int64_t* bound_offsets /*[n_clips+1] or null*/, const int32_t* bounds,
                          bp_chord_summary* summaries /*[n_clips]*/, uint8_t* labels, int64_t max_labels);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_CHORD_H */
