/* basic_pitch_amd_clips.h: many short clips in one call — raw PCM in, what note decoding needs out.  Same library and handle
 * type as basic_pitch_amd.h, same rules: every argument is checked before anything is queued, errors through
 * bp_last_error(h). */
#ifndef BASIC_PITCH_AMD_CLIPS_H
#define BASIC_PITCH_AMD_CLIPS_H

#include "basic_pitch_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- a job of clips: "what would bp_infer_pcm_raw_candidates return for each of them?" ----
 * A clip of 1 to 15 windows is under 40 us of device work behind about ten launches and a wait.  These calls take n_clips
 * clips at once: one downmix launch and one resampling launch for all of them, their windows packed into full batches across
 * clip boundaries (as bp_infer_tracks packs tracks), and the dense half of note decoding for every clip as its own whole track
 * — a constant number of launches per batch of windows, whatever the number of clips.
 *
 * The contract.  For every clip i, the rows [offsets[i], offsets[i + 1]) of note_out ([rows][88] float32), cand_bits
 * ([rows][12] bytes) and bend_map ([rows][88] int8; may be NULL, and is written only with params->include_pitch_bends) and
 * status[i] are bit for bit what bp_infer_pcm_raw_candidates(h, clip i alone, ...) writes, for any grouping and order of the
 * clips — except cand_bits of a clip with status 1 and a NaN, which are zero here.  status[i] = 1: a NaN in that clip's note or
 * onset rows, or params->onset_threshold <= 0; the caller decodes that clip's maps itself (bp_infer_pcm_raw + bp_notes_decode).
 * A NaN in one clip changes no other clip's status or bytes.  A clip of n_frames = 0 has no rows and status 0.
 *
 *   format, channels   per clip (format: any of the 14 BP_PCM_* codes); one sample_rate per call.  A ratio sample_rate : the handle's rate
 *                      whose filter the one-shot calls evaluate in the kernel is refused with BP_ERR_UNSUPPORTED, as
 *                      bp_stream_open refuses it.  Clips that are mono float32 at the handle's rate are windowed where they lie.
 *   pcm_mem_kind       BP_MEM_HOST or BP_MEM_DEVICE: where every clip's pcm lies.  The outputs are host buffers.
 *   errors             the argument domain of bp_infer_pcm_raw per clip; the message names the first offending clip's index.
 *   afterwards         the maps of the clips do not stay on the handle: bp_track_maps is refused until the next *_candidates
 *                      call of a single track.  The handle's cached resampling filter is that of sample_rate.
 *
 * bp_clips_row_offsets: offsets[i] = rows of the clips before clip i, offsets[n_clips] = all rows; the rows of a clip are
 * bp_handle_track_n_frames(h, bp_handle_resampled_length(h, n_frames, sample_rate)).  Touches neither the GPU nor the handle's
 * state; pcm is not looked at.
 */
typedef struct { const void* pcm; int64_t n_frames; int format; int channels; } bp_clip;

int bp_clips_row_offsets(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int64_t* offsets);

int bp_infer_clips_candidates(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind,
                              const bp_note_params* params, float* note_out, uint8_t* cand_bits, int8_t* bend_map, int* status);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_CLIPS_H */
