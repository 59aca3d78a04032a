/* basic_pitch_amd_sweep.h: the same posteriorgrams decoded under many parameter sets in one device call.  Same library and
 * handle type as basic_pitch_amd.h, same rules: every argument is checked before anything is queued, errors through
 * bp_last_error(h). */
#ifndef BASIC_PITCH_AMD_SWEEP_H
#define BASIC_PITCH_AMD_SWEEP_H

#include "basic_pitch_amd_events.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- a sweep: "what would bp_note_events_from_maps give for this segment under each of these parameter sets?" ----
 * Tuning the thresholds on a validation set, trying a frequency band, sweeping the minimum note length: the model's output
 * does not change between those decodes, only the note decoding does.  A sweep takes n_segments segments (as
 * bp_note_events_from_maps takes them) or n_clips clips (as bp_infer_clips_events), n_sets parameter sets and a table of
 * decodes, and runs every decode in one call: the maps go to the device (or through the model) once, the dense half of note
 * decoding runs once per distinct (lowest bin, highest bin, infer_onsets, onset_threshold) among the sets, the bend map once,
 * and the tracker is ONE launch with a workgroup per decode.
 *
 * The decode table.  Decode j is segment decodes[j].segment under sets[decodes[j].params]; `reserved` must be 0.  The same
 * pair may appear more than once.  decodes == NULL is the cross product, set-major: n_decodes must equal n_sets * n_segments,
 * and decode p * n_segments + i is segment i under set p.  Every set is validated, whether a decode names it or not.
 *
 * The contract.  For every decode j, status[j] and the events event_offsets[j] ... event_offsets[j + 1] - 1 with their bends
 * are what bp_note_events_from_maps (bp_infer_clips_events) returns for that segment (clip) alone with that set: field by
 * field and in the same order, statuses 0, 1 and 2 as basic_pitch_amd_events.h defines them.  bend_offset runs through the
 * bends of all decodes in event order; a decode whose set has include_pitch_bends == 0 contributes none.  The caller's maps
 * are left untouched.  A decode's capacity is bp_events_capacity(its rows, its set's min_note_len) events and 88 * rows bends.
 *
 *   max_events,   as in basic_pitch_amd_events.h: when the job needs more the call fails with BP_ERR_INVALID_ARG,
 *   max_bends     event_offsets[n_decodes] and the message hold the totals ("N events and M bends are needed"), status and
 *                 event_offsets are complete, and the call can be repeated with larger buffers.
 *   refused       a set that bp_note_events_from_maps refuses (the message names the set's index), a decode out of range or
 *                 with a non-zero `reserved` (the message names j), more than BP_SWEEP_MAX_DECODES decodes, more than
 *                 BP_SWEEP_MAX_ROWS rows over all decodes (split the job).
 *   nothing to do n_sets == 0, n_decodes == 0 or no rows at all: BP_OK, event_offsets zeroed, no device work.
 *   afterwards    as after bp_infer_clips_events; a call that fails after queuing returns once the stream has drained.
 *
 * BP_SWEEP_MAX_ROWS bounds the handle's pools, which grow with the rows of all DECODES (a decode writes its bends and, over
 * 432 rows, its working state into regions of its own) while the maps, bitmaps and note copies grow with the rows of the
 * segments alone.  Per decode row: 2 x 88 bytes of bends (the pool and the packed output), 2 x 16 x 88 / (min_note_len + 1)
 * bytes of event records (235 at the default 11, 2816 at 0), and 360 bytes of working state when any segment of the job has
 * more than 432 rows.  At the cap that is 6.5 GB with the default minimum length and 28 GB at the worst, of the 288 GB of an
 * MI355X; 64 sets over 512 one-window clips are 4.7 M rows.
 */
typedef struct bp_sweep_decode {
  int64_t segment; /* which segment (clip) */
  int32_t params;  /* which of the sets */
  int32_t reserved;
} bp_sweep_decode; /* 16 bytes */

#define BP_SWEEP_MAX_DECODES 65536
#define BP_SWEEP_MAX_ROWS 8388608

int bp_note_events_sweep(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, const float* onset,
                         const float* contour, int mem_kind, int64_t n_sets, const bp_note_params* sets, int64_t n_decodes,
                         const bp_sweep_decode* decodes, bp_note_event* events, int64_t max_events, int32_t* bends,
                         int64_t max_bends, int64_t* event_offsets /*[n_decodes+1]*/, int* status /*[n_decodes]*/);
int bp_infer_clips_events_sweep(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                                int64_t n_sets, const bp_note_params* sets, int64_t n_decodes, const bp_sweep_decode* decodes,
                                bp_note_event* events, int64_t max_events, int32_t* bends, int64_t max_bends,
                                int64_t* event_offsets /*[n_decodes+1]*/, int* status /*[n_decodes]*/);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_SWEEP_H */
