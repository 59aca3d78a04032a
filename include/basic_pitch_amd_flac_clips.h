/* basic_pitch_amd_flac_clips.h: a job of many FLAC files' bytes in one call, decoded on the device.  Same library and handle
 * type as basic_pitch_amd.h, same rules: every argument is checked before anything is queued, errors through
 * bp_last_error(h). */
#ifndef BASIC_PITCH_AMD_FLAC_CLIPS_H
#define BASIC_PITCH_AMD_FLAC_CLIPS_H

#include "basic_pitch_amd_events.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- datasets of short excerpts are stored as FLAC ----
 * bp_infer_flac_candidates decodes one file per call: four launches, an upload and a wait for a few dozen frames.  These calls
 * take the bytes of n_clips files, decode them all with four launches (csrc/flac_clips.hip: the same device code, every
 * stage on a table of streams), and hand the samples to what bp_infer_clips_candidates / bp_infer_clips_events run behind
 * their ingest: one downmix and one resampling launch, the clips' windows packed into full batches, the note candidates (and
 * the tracker) of every clip as its own track.
 *
 * The contract, per clip.  status[i] is
 *   0, 1, 2              as bp_infer_clips_candidates / bp_infer_clips_events define them.  For 0 the clip's rows (events) are
 *                        bit for bit those of bp_infer_flac_candidates on clip i alone (followed by
 *                        bp_notes_decode_candidates), for any grouping and order of the clips — and so those of the PCM
 *                        clips calls on the host decoder's samples.
 *   BP_CLIP_FLAC_HOST    the device decoder leaves the clip to the host, known before anything is queued: bp_flac_layout
 *                        fails, the stream is one bp_infer_flac refuses with BP_ERR_UNSUPPORTED (no sample count or block
 *                        sizes in STREAMINFO, more than 24 bits or 8 channels), no frame follows the metadata, the clip has
 *                        fewer than 42 bytes, or its scratch rows would exceed 8 * n_frames + 2 * max_block samples per channel
 *                        (streams whose smallest and largest block sizes are far apart; a fixed block size never does).
 *                        The clip has NO rows (offsets[i + 1] == offsets[i]), no events, and no device work.
 *   BP_CLIP_FLAC_FAILED  the device decoder could not follow the stream (lost frame chain, CRC-16 mismatch, reserved value or
 *                        overrun, candidate overflow).  The rows exist (they were laid out from STREAMINFO), their contents
 *                        are unspecified; in the events call the clip has no events.
 * For both, no other clip's status or bytes change; the caller takes the clip through bp_flac_decode — which also names a
 * corrupt file's fault — and the PCM calls.
 *
 *   sample_rate   one per call.  A clip whose STREAMINFO says another rate fails the whole call with BP_ERR_INVALID_ARG (the
 *                 message names the first such clip); a ratio whose filter is not tabulated is BP_ERR_UNSUPPORTED, as in
 *                 bp_infer_clips_candidates.
 *   clips         file may be NULL only with nbytes == 0.
 *   outputs       sized by bp_flac_clips_row_offsets, which touches neither the GPU nor the handle's state and gives the
 *                 offsets and the host-side statuses (0 or BP_CLIP_FLAC_HOST) the infer calls will use.  A job without
 *                 any row queues nothing.
 *   afterwards    as after bp_infer_clips_candidates: bp_track_maps is refused, the cached filter is that of sample_rate.  A
 *                 call that fails after queuing returns once the stream has drained.
 *
 * bp_flac_clips_decode_device: the decode alone, for tests and tools.  Clip i's interleaved samples, sign-extended int32 as
 * bp_flac_decode_device returns them, go to pcm + pcm_offsets[i]; pcm_offsets[i + 1] - pcm_offsets[i] must hold the clip's
 * n_frames * channels of bp_flac_layout (a BP_CLIP_FLAC_HOST clip needs no room and gets no samples).
 */
#define BP_CLIP_FLAC_HOST 3
#define BP_CLIP_FLAC_FAILED 4

typedef struct { const void* file; size_t nbytes; } bp_flac_clip;

int bp_flac_clips_row_offsets(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int sample_rate,
                              int64_t* offsets /*[n_clips+1]*/, int* status /*[n_clips]*/);
int bp_flac_clips_decode_device(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int32_t* pcm,
                                const int64_t* pcm_offsets /*[n_clips+1], in samples*/, int* status);
int bp_infer_flac_clips_candidates(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int sample_rate,
                                   const bp_note_params* params, float* note_out, uint8_t* cand_bits, int8_t* bend_map,
                                   int* status);
int bp_infer_flac_clips_events(bp_handle h, int64_t n_clips, const bp_flac_clip* clips, int sample_rate,
                               const bp_note_params* params, bp_note_event* events, int64_t max_events, int32_t* bends,
                               int64_t max_bends, int64_t* event_offsets, int* status);

#ifdef __cplusplus
}
#endif
#endif /* BASIC_PITCH_AMD_FLAC_CLIPS_H */
