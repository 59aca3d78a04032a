// IMA ADPCM files on the host alone (include/basic_pitch_amd_adpcm.h): RIFF/WAVE format tag 0x11 — the chunk walk is
// wav_walk's — and CAF `ima4`, whose desc / pakt / data chunks are walked here; the facts of a file from its headers
// (adpcm_walk, bp_adpcm_layout_of) and the host decoder (bp_adpcm_decode), the checker of adpcm_device.hip.  The step and the
// two block layouts are adpcm_host.h's.  No handle, no state but the thread's error string: thread-safe like flac_decode.cpp.
// Nothing here calls the device library.
//   IMA:  IMA Digital Audio Focus and Technical Working Groups, Recommended Practices for Enhancing Digital Audio
//         Compatibility in Multimedia Systems 3.00 (1992), the DVI ADPCM algorithm; the step is Python's audioop.adpcm2lin
//   WAV:  Microsoft Multimedia Standards Update, New Multimedia Data Types and Data Techniques 3.0 (1994), WAVE_FORMAT_DVI_ADPCM
//   CAF:  Apple Core Audio Format Specification 1.0 (desc, pakt, data); `ima4`: Apple TN 1081 (QuickTime IMA 4:1)
#include <cmath>
#include <cstring>

#include "adpcm_host.h"
#include "file_host.h"

namespace bp_file {

namespace {

uint16_t be16(const uint8_t* p) { return (uint16_t)((p[0] << 8) | p[1]); }
uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
uint64_t be64(const uint8_t* p) { return ((uint64_t)be32(p) << 32) | be32(p + 4); }
bool is(const uint8_t* p, const char* id) { return std::memcmp(p, id, 4) == 0; }

int fail(const std::string& why) {
  g_file_error = why;
  return -1;
}

// caff with a desc of format id `ima4`: the 8-byte head, every chunk's 12-byte head, the 32 bytes of desc and 24 of pakt
int caf_ima4_walk(const ByteSource& src, bp_adpcm_layout& lay) {
  const size_t n = src.size;
  uint8_t head[12] = {0}, desc[32], pakt[24];
  if (n < 8 || !src.at(0, 8, head) || !is(head, "caff")) return 0;
  if (be16(head + 4) != 1) return 0;  // (caf_walk names the version)
  bool have_desc = false, have_data = false, have_pakt = false;
  uint64_t data_bytes = 0;
  int64_t data_start = 0;
  size_t pos = 8;
  while (pos + 12 <= n) {
    if (!src.at(pos, 12, head)) return -1;
    const int64_t size = (int64_t)be64(head + 4);
    const size_t rest = n - (pos + 12);
    const bool to_end = size < 0 || (uint64_t)size >= rest;  // -1 (data alone may say so): to the end of the file
    const size_t avail = to_end ? rest : (size_t)size;
    if (is(head, "desc")) {
      if (avail < 32) return 0;  // (caf_walk reports it)
      if (!src.at(pos + 12, 32, desc)) return -1;
      if (!is(desc + 8, "ima4")) return 0;
      have_desc = true;
    } else if (is(head, "pakt") && avail >= 24) {
      if (!src.at(pos + 12, 24, pakt)) return -1;
      have_pakt = true;
    } else if (is(head, "data")) {
      data_bytes = avail > 4 ? avail - 4 : 0;  // behind the edit count
      data_start = (int64_t)(pos + 12 + (avail < 4 ? avail : 4));
      have_data = true;
    } else if (size < 0) {
      return have_desc ? fail("negative size of a CAF chunk") : 0;
    }
    if (to_end) break;
    pos += 12 + (size_t)size;
  }
  if (!have_desc) return 0;
  if (!have_data) return fail("missing desc or data chunk");
  double rate;
  const uint64_t rate_bits = be64(desc);
  std::memcpy(&rate, &rate_bits, 8);
  const uint32_t packet_bytes = be32(desc + 16), packet_frames = be32(desc + 20), channels = be32(desc + 24);
  if (channels < 1) return fail("zero channels");
  if (channels > 65535) return fail("bad channel count " + std::to_string(channels));
  if (packet_frames != 64 || packet_bytes != 34 * channels)
    return fail("unsupported CAF ima4 packet layout: " + std::to_string(packet_frames) + " frames in " + std::to_string(packet_bytes) +
                " bytes a packet (read: 64 frames in " + std::to_string(34 * channels) + " bytes)");
  if (!(rate >= 0.5 && rate < 2147483647.0)) return fail("bad sample rate in the header");
  lay = bp_adpcm_layout{};
  lay.container = BP_CONTAINER_CAF, lay.codec = BP_ADPCM_IMA4, lay.channels = (int32_t)channels;
  lay.sample_rate = (int32_t)std::llround(rate);
  lay.block_bytes = (int32_t)(34 * channels), lay.block_frames = 64;
  lay.data_start = data_start, lay.data_bytes = (int64_t)data_bytes;
  lay.n_frames = (int64_t)(data_bytes / (uint64_t)lay.block_bytes) * 64;
  if (have_pakt) {  // packets, valid frames, priming frames, remainder frames
    const int64_t valid = (int64_t)be64(pakt + 8);
    const int32_t priming = (int32_t)be32(pakt + 16);
    if (priming != 0) return fail("unsupported CAF pakt chunk: " + std::to_string(priming) + " priming frames (read: 0)");
    if (valid >= 0 && valid < lay.n_frames) lay.n_frames = valid;
  }
  return BP_ADPCM_IMA4;
}

}  // namespace

int adpcm_walk(const ByteSource& src, bp_adpcm_layout& lay) {
  uint8_t magic[12] = {0};
  if (src.size && !src.at(0, src.size < 12 ? src.size : 12, magic)) return -1;
  switch (pcm_container_of(magic, src.size)) {
    case BP_CONTAINER_WAV: {
      WavInfo w;
      size_t data_pos = 0;
      if (!wav_walk(src, w, data_pos)) return w.tag == kWavTagIma ? -1 : 0;
      if (w.tag != kWavTagIma) return 0;
      lay = bp_adpcm_layout{};
      lay.container = BP_CONTAINER_WAV, lay.codec = BP_ADPCM_IMA_WAV, lay.channels = w.channels, lay.sample_rate = w.sample_rate;
      lay.block_bytes = w.block_align, lay.block_frames = (w.block_align - 4 * w.channels) * 2 / w.channels + 1;
      lay.n_frames = w.n_frames, lay.data_start = (int64_t)data_pos, lay.data_bytes = (int64_t)w.pcm_bytes;
      return BP_ADPCM_IMA_WAV;
    }
    case BP_CONTAINER_CAF: return caf_ima4_walk(src, lay);
    default: return 0;
  }
}

}  // namespace bp_file

using namespace bp_file;

namespace {
// the layout of the bytes at `file`, or the status to return
int layout_of(const char* what, const void* file, size_t nbytes, bp_adpcm_layout& lay) {
  ByteSource src;
  src.mem = static_cast<const uint8_t*>(file), src.size = nbytes;
  const int kind = adpcm_walk(src, lay);
  if (kind == 0) g_file_error = std::string(what) + ": not an IMA ADPCM file (RIFF/WAVE format tag 0x11 or CAF ima4)";
  return kind > 0 ? BP_OK : BP_ERR_BAD_AUDIO;
}
}  // namespace

extern "C" {

int bp_adpcm_layout_of(const void* file, size_t nbytes, bp_adpcm_layout* out) {
  if (!file || !out) {
    g_file_error = "bp_adpcm_layout_of: null pointer";
    return BP_ERR_INVALID_ARG;
  }
  return layout_of("bp_adpcm_layout_of", file, nbytes, *out);
}

int bp_adpcm_decode(const void* file, size_t nbytes, int16_t* pcm, int64_t max_frames, int64_t* n_frames) {
  if (!file || !pcm) {
    g_file_error = "bp_adpcm_decode: null pointer";
    return BP_ERR_INVALID_ARG;
  }
  bp_adpcm_layout lay;
  if (int rc = layout_of("bp_adpcm_decode", file, nbytes, lay)) return rc;
  if (n_frames) *n_frames = lay.n_frames;
  if (lay.n_frames > max_frames) {
    g_file_error = "bp_adpcm_decode: buffer too small";
    return BP_ERR_INVALID_ARG;
  }
  const uint8_t* data = static_cast<const uint8_t*>(file) + lay.data_start;
  if (lay.codec == BP_ADPCM_IMA_WAV) ima_wav_decode(data, (size_t)lay.data_bytes, lay.channels, lay.block_bytes, lay.n_frames, pcm);
  else ima4_decode(data, (size_t)lay.data_bytes, lay.channels, lay.n_frames, pcm);
  return BP_OK;
}

}  // extern "C"
