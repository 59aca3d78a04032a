/*
 * basic_pitch_amd: AIFF / AIFF-C, CAF, AU and RF64 / BW64 files — headers around uncompressed samples.
 *
 * Replaces: the decode step of librosa.load for these containers (inference.py:239 hands them to libsndfile).  The host
 * reads the headers alone; the samples go to the device in the file's own sample format (bp_pcm_format codes 0 to 13 of
 * basic_pitch_amd.h) and become float there, so every call that takes a `format` takes such a file's samples as they lie
 * in the file: bp_infer_pcm_raw, bp_infer_pcm_raw_candidates, bp_infer_clips_candidates / _events, bp_stream_open.
 * bp_transcribe_files and bp_files_batch_probe read these files beside RIFF/WAVE and FLAC.
 *
 *   AIFF / AIFF-C   FORM ... AIFF | AIFC; chunks in any order, padded to even size.  COMM: channels, frames, sample size
 *                   (a sample is ceil(bits / 8) bytes, left-justified as stored; 8-bit is signed), 80-bit extended rate
 *                   (nearest integer); AIFF-C adds a compression type: NONE, twos, in24, in32 (big-endian integers), sowt
 *                   (little-endian integers), fl32 / FL32, fl64 / FL64 (big-endian floats), ulaw / ULAW, alaw / ALAW,
 *                   `raw ` (unsigned 8-bit).  SSND: offset, block size, then the samples at 8 + offset.
 *   CAF             caff version 1; `desc`: float64 rate, format id lpcm / ulaw / alaw, flags bit 0 float, bit 1
 *                   little-endian; bytes per packet = channels x width, one frame per packet; lpcm of 8 (signed) / 16 /
 *                   24 / 32-bit integers and 32 / 64-bit floats in either byte order.  `data`: a 4-byte edit count, then
 *                   the samples; a size of -1 means to the end of the file.
 *   AU              .snd, big-endian; encodings 1 mu-law, 2 / 3 / 4 / 5 signed 8 / 16 / 24 / 32-bit, 6 / 7 float 32 / 64,
 *                   27 A-law; a data size of 0xffffffff means to the end of the file.
 *   RF64 / BW64     a RIFF/WAVE file whose 64-bit sizes lie in its ds64 chunk: BP_CONTAINER_WAV; bp_wav_info and
 *                   bp_wav_decode take it too.
 *   RIFF/WAVE       beside integer and float PCM: G.711, format tag 7 (mu-law) or 6 (A-law) with 8 bits, plain, inside
 *                   WAVE_FORMAT_EXTENSIBLE or in RF64 / BW64: BP_PCM_ULAW / BP_PCM_ALAW, the samples of the AU or AIFF-C
 *                   file of the same bytes.
 * A file that ends before its header's count holds the frames that are there.  IMA ADPCM (RIFF/WAVE tag 0x11, CAF `ima4`)
 * is not samples but blocks: include/basic_pitch_amd_adpcm.h reads it, these two calls answer BP_ERR_BAD_AUDIO.  Not read:
 * the little-endian AU variant (`dns.`), Sony Wave64, MS ADPCM (tag 2), 3- and 5-bit IMA and every compressed AIFF-C type
 * (ima4, MAC3, ...): BP_ERR_BAD_AUDIO, naming what was found.
 *
 *   bp_pcm_file_layout_of   the facts of a file from its headers: host code, no handle, thread-safe; `file` = the whole
 *                           file in memory, or a prefix of it that holds the headers (the frame count is then that of
 *                           the prefix).
 *   bp_pcm_file_decode      interleaved float32 [n_frames][channels], the values the device makes of the samples: the
 *                           host checker of the device conversion (what bp_wav_decode is for RIFF/WAVE).
 * Errors: BP_ERR_BAD_AUDIO (not one of the four containers, a fault in the headers, contents that are not read),
 * BP_ERR_INVALID_ARG (null pointer, buffer too small; *n_frames says what is needed); message from bp_files_last_error.
 */
#ifndef BASIC_PITCH_AMD_CONTAINERS_H
#define BASIC_PITCH_AMD_CONTAINERS_H

#include "basic_pitch_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { BP_CONTAINER_WAV = 1, BP_CONTAINER_AIFF = 2, BP_CONTAINER_CAF = 3, BP_CONTAINER_AU = 4 }; /* RF64: WAV */

typedef struct bp_pcm_file_layout {
  int32_t container;       /* BP_CONTAINER_* */
  int32_t format;          /* BP_PCM_* of the samples as the file stores them */
  int32_t channels;
  int32_t sample_rate;
  int32_t bits_per_sample; /* as the header says: 12 for a 12-bit AIFF in 16-bit words, 8 for G.711 */
  int32_t reserved;
  int64_t n_frames;
  int64_t data_start;      /* byte offset of the first sample */
} bp_pcm_file_layout;

int bp_pcm_file_layout_of(const void* file, size_t nbytes, bp_pcm_file_layout* out);
int bp_pcm_file_decode(const void* file, size_t nbytes, float* pcm, int64_t max_frames, int64_t* n_frames);

#ifdef __cplusplus
}
#endif

#endif /* BASIC_PITCH_AMD_CONTAINERS_H */
