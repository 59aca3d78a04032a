/* basic_pitch_amd_sync.h: two recordings against each other — which stretch of one segment sounds with which stretch of
 * another, from the note posteriorgrams alone: a chroma per row pooled over units of `hop` frames, one feature byte a class, a
 * gain a pair of units, and the best monotone path from the first units of both to their last (a dynamic time warp), on the
 * device for a table of pairs of the segments of a job or of clips through the model.  Two takes of a piece, a performance
 * against a rendition of its score, an annotated recording whose labels should move onto another.  Same library and handle
 * type as basic_pitch_amd.h, same rules: every argument is checked before anything is queued, errors through
 * bp_last_error(h), a refusal names the index of the pair or of the segment, a call that fails after queuing returns once the
 * handle's stream has drained. */
#ifndef BASIC_PITCH_AMD_SYNC_H
#define BASIC_PITCH_AMD_SYNC_H

#include "basic_pitch_amd_chord.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- the definition ----
 * What the synchronisation of two segments is, said once: the host checker, the kernels and the tests' restatement are all
 * held to it.  It is this project's own statement of chroma dynamic time warping; it is UNPINNED against any third-party
 * alignment or time-warping implementation (README, "Unpinned").  EVERYTHING BELOW IS EXACT INTEGER ARITHMETIC: the result is
 * a property of the integers and not of an order of summation, so the device may add in any order and still equals the host
 * byte for byte.
 *
 * A job is n segments (rows of note[rows][88], float32) and a table of n_pairs pairs (a, b) of segment indices.  A segment
 * may appear in many pairs, and a == b is allowed.
 *
 *   chroma      c[t][k] exactly as basic_pitch_amd_chord.h defines it: the quantiser q, threshold_q, min_pitch ... max_pitch,
 *               class (p + 9) % 12.  A chroma entry is at most 2^13.
 *   units       Unit u is the frames [u * hop, min((u + 1) * hop, rows)), hop in 1 ... BP_SYNC_MAX_HOP.
 *                   U = ceil(rows / hop)
 *                   cu[u][k] = sum of c[t][k] over the unit's frames                        at most 64 * 2^13 = 2^19
 *   feature     One byte a class.  With s = sum over k of cu[u][k]^2 (int64, below 12 * 2^38 < 2^42) and s > 0, r is THE
 *               SMALLEST INTEGER WITH r * r >= s, the ceiling root, and
 *                   x[u][k] = floor(255 * cu[u][k] / r)
 *               With s = 0 the unit is all zero.  The ceiling root, not the floor root, is what gives
 *                   sum over k of x[u][k]^2 <= 255^2
 *               (x <= 255 cu / r, so the sum is at most 255^2 s / r^2 <= 255^2); with the floor root two classes of 1 each,
 *               s = 2 and r = 1, become (255, 255).  With the ceiling root they are (127, 127).
 *   gain            g(i, j) = sum over k of xa[i][k] * xb[j][k]
 *               and by Cauchy-Schwarz 0 <= g <= 255^2 = 65,025.
 *   admissible  Every cell when band == 0.  Otherwise the cells with
 *                   |i * (M - 1) - j * (N - 1)| <= band * max(N - 1, M - 1)
 *               in int64 (every term is below 2^26 under the bounds below).  N and M are the units of a and of b; band is
 *               0 ... BP_SYNC_MAX_UNITS.
 *   recurrence      D[0][0] = 2 * g(0, 0)
 *                   D[i][j] = max(D[i-1][j-1] + 2 * g(i, j), D[i-1][j] + g(i, j), D[i][j-1] + g(i, j))
 *               over the sources that exist, are admissible and are reachable.  An inadmissible cell is unreachable.  The
 *               weights 2 / 1 / 1 give every path the same total weight N + M, so nothing favours long or short paths and no
 *               constant need be subtracted.  A cell (i, j) lies at weight i + j + 2 of its paths, so
 *                   D <= (N + M) * 65,025 <= 16,384 x 65,025 = 1,065,369,600 < 2^31
 *               with N, M <= BP_SYNC_MAX_UNITS = 8192: D is int32.
 *   ties        Diagonal before (i-1, j) before (i, j-1): a later candidate wins only when STRICTLY GREATER.
 *   path        From (N-1, M-1) back to (0, 0) along the recorded predecessors, reported in ascending order as int32 pairs
 *               (i, j).  Its length is max(N, M) <= n_path <= N + M - 1.
 *   status      Per pair.  0: total = D[N-1][M-1].  1: a NaN anywhere in the note rows of either segment, in whatever pitch;
 *               this is decided first.  2: no path, because a segment has no rows.  With a non-zero status n_path and total
 *               are 0.  units_a and units_b are U of the two segments whatever the status.  A silent unit is not a status: it
 *               earns 0 everywhere and the tie rule decides the path through it.
 *               A BAND NEVER CUTS THE END OFF: with band >= 1 and N >= M the cells (i, round(i (M-1) / (N-1))) are within
 *               half a column of the line, so admissible, and from one row to the next the rounded column grows by 0 or 1
 *               (the line grows by at most 1): a staircase of admissible diagonal and (i-1, j) steps from (0, 0) to
 *               (N-1, M-1); N < M likewise in columns; N or M of 1 makes both sides 0.  So status 2 has no second cause.
 *   room        There is no capacity protocol.  Pair p owns N_p + M_p - 1 entries of path (0 when either segment has no rows),
 *               one pair after the other; summary.path_first says where its region starts; entries of the region past n_path
 *               are (-1, -1).  max_path is checked against the sum before anything is queued.
 *
 * Known limits, as they are.  Both ends are fixed: there is no subsequence search.  ONE WORKGROUP A PAIR: a single long pair
 * does not fill the chip.  Octave-folded energy only.  The defaults are a prototype's and are not tuned.
 * A segment against ITSELF gives the pure diagonal when every unit has the same self-gain g(u, u): then D[i][i] = 2 (i + 1) g
 * meets the weight bound above, and the diagonal candidate, first in the tie order, is taken all the way.  It is not a theorem
 * of the definition: the floors make g(u, u) differ by a few parts in a thousand between units, and a path may then dwell on
 * the louder one.  One-hot units (one sounding pitch class) all have g(u, u) = 65,025: planted warps of such units, b = a[w]
 * for a non-decreasing w with steps of 0 or 1 and neighbouring classes that differ, come back as the path {(w[j], j)} with
 * total (N + M) * 65,025 (tests/test_sync_cpu.py).
 */
#define BP_SYNC_MAX_UNITS 8192 /* units of a segment: 1024 lanes x 8 columns a lane of the recurrence's largest workgroup; at
                                  eight columns the kernel holds 24 feature and 16 D registers a lane and the compiler reports
                                  no scratch and no spills, and D stays int32 by the bound above */
#define BP_SYNC_MAX_HOP 64
#define BP_SYNC_MAX_GAIN 65025       /* 255^2 */
#define BP_SYNC_MAX_CELLS 268435456  /* 2^28: the sum of N x M over the pairs of a job */
#define BP_SYNC_MAX_PRED_BYTES 268435456 /* 2^28: the device's store of predecessors over the pairs of a job (below) */
#define BP_SYNC_CLASSES 12
#define BP_SYNC_PITCHES 88
#define BP_SYNC_TRACE_TILE 64 /* steps and lanes of one tile of the backtrace */

typedef struct bp_sync_params {
  int32_t threshold_q;          /* 0 ... 1024, in units of 1/1024 (default 307) */
  int32_t min_pitch, max_pitch; /* 0 <= min_pitch <= max_pitch <= 87 (default 0, 87) */
  int32_t hop;                  /* 1 ... BP_SYNC_MAX_HOP frames a unit (default 4) */
  int32_t band;                 /* 0: every cell; 1 ... BP_SYNC_MAX_UNITS: the band's half width in units (default 0) */
  int32_t reserved[3];          /* 0 */
} bp_sync_params;               /* 32 bytes */

typedef struct bp_sync_pair {
  int32_t a, b; /* indices of segments */
} bp_sync_pair; /* 8 bytes */

typedef struct bp_sync_summary {
  int32_t status;     /* 0, 1 (a NaN) or 2 (a segment without rows) */
  int32_t units_a, units_b;
  int32_t n_path;     /* 0 with a non-zero status */
  int64_t path_first; /* where the pair's region of path starts, in entries of two int32 */
  int64_t total;      /* D[N-1][M-1]; 0 with a non-zero status */
} bp_sync_summary;    /* 32 bytes */

/* threshold 307, pitches 0 ... 87, hop 4, band 0 */
void bp_sync_params_default(bp_sync_params* p);

/*
 * ---- on the host: the checker, no handle and no device ----
 * One pair: *summary (path_first 0) and path[0 ... N + M - 1) as pairs of int32, the tail past n_path (-1, -1).
 * BP_ERR_INVALID_ARG, with nothing written, for negative rows, a segment of more than BP_SYNC_MAX_UNITS units, null note with
 * rows, a null summary, a malformed p (threshold_q outside 0 ... 1024, pitches outside 0 <= min_pitch <= max_pitch <= 87, hop
 * outside 1 ... 64, band outside 0 ... 8192, a non-zero reserved word), max_path below N + M - 1 (0 when either segment has no
 * rows), or room without a buffer.  rows_a == 0 or rows_b == 0: status 2.
 */
int bp_sync_rows(const float* note_a, int64_t rows_a, const float* note_b, int64_t rows_b, const bp_sync_params* p, int32_t* path,
                 int64_t max_path, bp_sync_summary* summary);

/*
 * ---- on the device: segments the caller holds ----
 * Segment i is rows [row_offsets[i], row_offsets[i + 1]) of note, which lies in host or device memory after mem_kind and is
 * left untouched.  summaries[p] and the pair's region of path are byte for byte those of bp_sync_rows on segments pairs[p].a
 * and pairs[p].b, but for path_first.
 *
 *   room        max_path >= the sum over the pairs of N_p + M_p - 1, checked before anything is queued; with too little room
 *               the call is refused and nothing is written.
 *   nothing     Zero pairs is a call that does nothing.  A pair of TWO segments without rows (status 2) is settled on the
 *               host.  A pair with rows on one side alone goes to the device, because a NaN in those rows decides first
 *               (status 1, else 2): its workgroup reads the segment's flag and leaves.  A segment that no pair names costs
 *               no device work beyond the source's own.
 *   refused     negative n_segments or n_pairs, row_offsets that do not start at 0 or decrease, a bad mem_kind, null note with
 *               rows, null pairs or summaries with pairs, a malformed p; a pair outside 0 ... n_segments - 1 (the pair is
 *               named); a segment of a pair of more than BP_SYNC_MAX_UNITS units (the pair and the segment are named); more
 *               than BP_SYNC_MAX_CELLS cells or BP_SYNC_MAX_PRED_BYTES bytes of predecessors over the pairs (the pair at
 *               which the sum passes the bound is named); more than BP_SWEEP_MAX_ROWS rows in all; too little room or room
 *               without a buffer.
 *
 * How (csrc/sync.hip).  FEATURES: unit-parallel over the segments that a pair names, sixteen lanes a unit and a
 * lane a class: quantise, fold, pool over hop, the ceiling root and the division; 16 bytes a unit, 12 feature bytes and 4 zero
 * bytes; the NaN flag of a segment comes from the same loads; computed once a segment however many pairs name it.  RECURRENCE:
 * ONE WORKGROUP A PAIR.  Lane l owns C consecutive columns of b and works at step s on row i = s - l; the one value it needs
 * of the lane below, that lane's last-column D of the row it just finished, comes by a data-parallel shift inside a wave and
 * through LDS at the waves' edges, and the value received one step earlier is this step's diagonal source: one barrier a
 * step, N + lanes in use - 1 steps.  xa is staged in LDS, the lane's columns of xb are registers, a gain is three
 * v_dot4_u32_u8 where it is used; no gain reaches memory.  The predecessors are two bits a cell in the skewed order
 * [step][lane], so a step's stores are one run: (N + lanes - 1) x lanes x C cells and not N x M, which is what
 * BP_SYNC_MAX_PRED_BYTES bounds (a byte a lane and step up to four columns, two at eight).  C and the workgroup come from the
 * job's longest b.  BACKTRACE, same workgroup: tiles of BP_SYNC_TRACE_TILE steps x lanes of predecessors through LDS, one lane
 * walks, all lanes store the path and the (-1, -1) tail.
 */
int bp_sync_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, int mem_kind, int64_t n_pairs,
                      const bp_sync_pair* pairs, const bp_sync_params* p, bp_sync_summary* summaries /*[n_pairs]*/, int32_t* path,
                      int64_t max_path);

/*
 * ---- clips through the model ----
 * The clips as bp_infer_clips_events takes them, through the same driver; a segment is a clip, its rows those of
 * bp_clips_row_offsets.  Pairs, outputs, room and bounds as above.
 */
int bp_infer_clips_sync(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind, int64_t n_pairs,
                        const bp_sync_pair* pairs, const bp_sync_params* p, bp_sync_summary* summaries /*[n_pairs]*/, int32_t* path,
                        int64_t max_path);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_SYNC_H */
