/*
 * basic_pitch_amd: IMA ADPCM files — RIFF/WAVE format tag 0x11 (IMA / DVI ADPCM, 4 bits a sample; plain, inside
 * WAVE_FORMAT_EXTENSIBLE, RF64 / BW64) and CAF format id `ima4` (IMA 4:1).
 *
 * Replaces: the decode step of librosa.load for these files (inference.py:239 hands WAV to libsndfile, which reads tag 0x11;
 * `ima4` in CAF goes beyond it).  The samples are not addressable one by one, so no bp_pcm_format stands for them: the file's
 * bytes go to the device as they are, a quarter of the PCM, one launch expands them to interleaved int16 in a buffer of the
 * handle (csrc/adpcm_device.hip), and the BP_PCM_S16 ingest follows.
 *
 * The step, for both layouts, with s = step[index] (the 89-entry IMA table):
 *   d = s>>3, + s if code & 4, + s>>1 if code & 2, + s>>2 if code & 1; predictor -= d if code & 8, else += d; clamped to
 *   int16; index += {-1, -1, -1, -1, 2, 4, 6, 8}[code & 7], clamped to 0 ... 88.  A decoded sample v is v / 32768 as a float.
 * WAV (B = block align, C = channels): a block starts with C headers of 4 bytes (int16 LE predictor, uint8 step index,
 *   a reserved byte); the predictor is the block's first frame; then (B - 4C) bytes in groups of 4 bytes per channel in
 *   channel rotation, 8 codes a group, low nibble first: (B - 4C) * 2 / C + 1 frames a block.  (B - 4C) must be a positive
 *   multiple of 4C.  Frames: whole blocks only, capped by the `fact` chunk's count where it is present and smaller.
 * CAF: 64 frames and 34 * C bytes a packet, C sub-packets of 34 bytes in channel order: a big-endian word h (predictor =
 *   (int16)(h & 0xff80), index = h & 0x7f), then 32 bytes of codes, low nibble first; all 64 frames come from the codes.
 *   Frames: packets x 64, capped by the `pakt` chunk's valid frames where it is present; priming frames must be 0.
 * A step index above 88 in a header is read as 88, on the host and on the device.  Not read: 3- and 5-bit IMA, MS ADPCM
 * (tag 2), `ima4` in AIFF-C: BP_ERR_BAD_AUDIO, naming what was found.
 *
 *   bp_adpcm_layout_of       the facts of a file from its headers: host code, no handle, thread-safe; `file` = the whole file
 *                            in memory or a prefix that holds the headers (the counts are then those of the prefix).
 *   bp_adpcm_decode          interleaved int16 [n_frames][channels] on the host: the checker of the device decoder.
 *   bp_adpcm_decode_device   the same samples from the device decoder (pcm NULL: decode, count, copy nothing).
 *   bp_infer_adpcm           the file's posteriorgrams: bp_infer_pcm_raw(BP_PCM_S16) of those samples, bit for bit.
 *   bp_infer_adpcm_candidates  as bp_infer_flac_candidates; bp_track_maps fetches the maps afterwards.
 *   bp_infer_adpcm_clips_events  many short files in one call: one copy, ONE decode launch for all of them, then what
 *                            bp_infer_clips_events does on their samples in device memory.  All clips share codec, sample rate
 *                            and channel count (BP_ERR_INVALID_ARG names the first that differs); a clip without frames has
 *                            no rows.  Contract and status codes: include/basic_pitch_amd_events.h.
 * bp_wav_info / bp_wav_decode take tag 0x11 too (floats of the same int16).
 * Errors of the host calls: BP_ERR_BAD_AUDIO (not such a file, a fault in the headers), BP_ERR_INVALID_ARG (null pointer,
 * buffer too small; *n_frames says what is needed); message from bp_files_last_error.  The handle calls: bp_last_error;
 * they take the channel counts and rates of every ingest call (1 - 64 channels, 1,000 - 768,000 Hz), check every argument
 * before anything is queued, and return only once the handle's stream has drained.
 */
#ifndef BASIC_PITCH_AMD_ADPCM_H
#define BASIC_PITCH_AMD_ADPCM_H

#include "basic_pitch_amd_containers.h"
#include "basic_pitch_amd_events.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { BP_ADPCM_IMA_WAV = 1, BP_ADPCM_IMA4 = 2 };

typedef struct bp_adpcm_layout {
  int32_t container;    /* BP_CONTAINER_WAV | BP_CONTAINER_CAF */
  int32_t codec;        /* BP_ADPCM_* */
  int32_t channels;
  int32_t sample_rate;
  int32_t block_bytes;  /* WAV: the block align; CAF: 34 * channels */
  int32_t block_frames; /* frames a block decodes to */
  int64_t n_frames;
  int64_t data_start;   /* byte offset of the first block */
  int64_t data_bytes;   /* bytes of blocks held (a trailing partial block included) */
} bp_adpcm_layout;

typedef struct bp_adpcm_clip {
  const void* file; /* the file's bytes, host memory */
  size_t nbytes;
} bp_adpcm_clip;

int bp_adpcm_layout_of(const void* file, size_t nbytes, bp_adpcm_layout* out);
int bp_adpcm_decode(const void* file, size_t nbytes, int16_t* pcm, int64_t max_frames, int64_t* n_frames);

int bp_adpcm_decode_device(bp_handle h, const void* file, size_t nbytes, int16_t* pcm, int64_t max_frames, int64_t* n_frames);
int bp_infer_adpcm(bp_handle h, const void* file, size_t nbytes, float* note, float* onset, float* contour, int mem_kind);
int bp_infer_adpcm_candidates(bp_handle h, const void* file, size_t nbytes, const bp_note_params* params, float* note_out,
                              uint8_t* cand_bits, int8_t* bend_map, int* status);
int bp_infer_adpcm_clips_events(bp_handle h, int64_t n_clips, const bp_adpcm_clip* clips, const bp_note_params* params,
                                bp_note_event* events, int64_t max_events, int32_t* bends, int64_t max_bends,
                                int64_t* event_offsets, int* status);

#ifdef __cplusplus
}
#endif

#endif /* BASIC_PITCH_AMD_ADPCM_H */
