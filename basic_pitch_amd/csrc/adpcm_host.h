// IMA ADPCM on the host, shared by wav_file.cpp (bp_wav_decode of format tag 0x11) and adpcm_file.cpp (the layouts, bp_adpcm_decode):
// the step and the two block layouts include/basic_pitch_amd_adpcm.h describes.  Everything here is inline, so that a program
// which links wav_file.cpp alone still links.  adpcm_device.hip is the same arithmetic on the device; bp_adpcm_decode checks it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace bp_file {

constexpr int kImaSteps = 89;
constexpr int16_t kImaStep[kImaSteps] = {
    7,     8,     9,     10,    11,    12,    13,    14,    16,    17,    19,    21,    23,    25,    28,    31,    34,    37,
    41,    45,    50,    55,    60,    66,    73,    80,    88,    97,    107,   118,   130,   143,   157,   173,   190,   209,
    230,   253,   279,   307,   337,   371,   408,   449,   494,   544,   598,   658,   724,   796,   876,   963,   1060,  1166,
    1282,  1411,  1552,  1707,  1878,  2066,  2272,  2499,  2749,  3024,  3327,  3660,  4026,  4428,  4871,  5358,  5894,  6484,
    7132,  7845,  8630,  9493,  10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

// one code: the shift form (s>>3, + s, + s>>1, + s>>2), not ((2 code + 1) s) >> 3, which rounds differently
inline void ima_step(int code, int& pred, int& index) {
  const int s = kImaStep[index];
  int d = s >> 3;
  if (code & 4) d += s;
  if (code & 2) d += s >> 1;
  if (code & 1) d += s >> 2;
  pred = (code & 8) ? pred - d : pred + d;
  pred = pred < -32768 ? -32768 : pred > 32767 ? 32767 : pred;
  index += (code & 4) ? 2 * (code & 3) + 2 : -1;  // {-1, -1, -1, -1, 2, 4, 6, 8}[code & 7]
  index = index < 0 ? 0 : index > 88 ? 88 : index;
}

// RIFF/WAVE tag 0x11.  A block of `block_bytes`: per channel int16 LE predictor (the block's first frame), step index (above 88:
// 88), a reserved byte; then groups of 4 bytes per channel in channel rotation, 8 codes a group, low nibble first.  Writes
// frames [0, n_frames) of the blocks at `data` (data_bytes of them are there: blocks that do not lie inside are not read).
inline void ima_wav_decode(const uint8_t* data, size_t data_bytes, int channels, int block_bytes, int64_t n_frames, int16_t* out) {
  const int64_t block_frames = (int64_t)(block_bytes - 4 * channels) * 2 / channels + 1;
  const int groups = (block_bytes - 4 * channels) / (4 * channels);
  for (int64_t b = 0; b * block_frames < n_frames && (size_t)(b + 1) * (size_t)block_bytes <= data_bytes; ++b) {
    const uint8_t* blk = data + (size_t)b * (size_t)block_bytes;
    const int64_t f0 = b * block_frames;
    for (int c = 0; c < channels; ++c) {
      int pred = (int16_t)(uint16_t)(blk[4 * c] | (blk[4 * c + 1] << 8));
      int index = blk[4 * c + 2] > 88 ? 88 : blk[4 * c + 2];
      out[f0 * channels + c] = (int16_t)pred;
      for (int g = 0; g < groups; ++g) {
        const uint8_t* p = blk + 4 * channels * (1 + g) + 4 * c;
        for (int k = 0; k < 8; ++k) {
          const int64_t f = f0 + 1 + 8 * g + k;
          if (f >= n_frames) break;
          ima_step((p[k >> 1] >> (4 * (k & 1))) & 15, pred, index);
          out[f * channels + c] = (int16_t)pred;
        }
      }
    }
  }
}

// CAF `ima4`.  A packet of 34 bytes per channel in channel order: a big-endian word h (predictor = (int16)(h & 0xff80), index =
// min(h & 0x7f, 88)), then 32 bytes of codes, low nibble first: 64 frames, all from the codes.
inline void ima4_decode(const uint8_t* data, size_t data_bytes, int channels, int64_t n_frames, int16_t* out) {
  const size_t packet = (size_t)34 * (size_t)channels;
  for (int64_t b = 0; b * 64 < n_frames && (size_t)(b + 1) * packet <= data_bytes; ++b) {
    for (int c = 0; c < channels; ++c) {
      const uint8_t* p = data + (size_t)b * packet + (size_t)34 * (size_t)c;
      const int h = (p[0] << 8) | p[1];
      int pred = (int16_t)(uint16_t)(h & 0xff80);
      int index = (h & 0x7f) > 88 ? 88 : (h & 0x7f);
      for (int k = 0; k < 64; ++k) {
        const int64_t f = b * 64 + k;
        if (f >= n_frames) break;
        ima_step((p[2 + (k >> 1)] >> (4 * (k & 1))) & 15, pred, index);
        out[f * channels + c] = (int16_t)pred;
      }
    }
  }
}

}  // namespace bp_file
