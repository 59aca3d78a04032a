// RIFF / WAVE, on the host alone (basic_pitch_amd/audio.py read_wav: PCM 8 / 16 / 24 / 32, IEEE float 32 / 64, G.711 (tags 7
// and 6) and IMA ADPCM (tag 0x11, adpcm_host.h); WAVE_FORMAT_EXTENSIBLE; RF64 / BW64, whose 64-bit data size lies in a ds64
// chunk: EBU Tech 3306): the chunk walk, the
// sample conversion, bp_wav_info and bp_wav_decode.  Nothing here calls the device library; the file job (file_pipeline.cpp) parses its WAV files with wav_walk / wav_parse and sends the samples as stored.
#include <cerrno>
#include <cstring>
#include <unistd.h>

#include "adpcm_host.h"
#include "file_host.h"

namespace bp_file {

namespace {
uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }
}  // namespace

bool ByteSource::at(size_t pos, size_t len, uint8_t* out) const {
  if (mem) {
    std::memcpy(out, mem + pos, len);
    return true;
  }
  size_t done = 0;
  while (done < len) {
    const ssize_t got = pread(fd, out + done, len - done, (off_t)(pos + done));
    if (got < 0 && errno == EINTR) continue;
    if (got <= 0) {
      g_file_error = got < 0 ? std::string("read failed: ") + std::strerror(errno) : "the file is shorter than its size";
      return false;
    }
    done += (size_t)got;
  }
  return true;
}

// the chunk walk of a RIFF/WAVE file: the format and where the samples lie (data_pos; w.pcm is the caller's to set).  Reads
// the 12-byte head, every chunk's 8-byte head, up to 26 bytes of a fmt chunk, 24 of a ds64 chunk and 4 of a fact chunk, nothing
// else.
bool wav_walk(const ByteSource& src, WavInfo& w, size_t& data_pos) {
  const size_t n = src.size;
  uint8_t head[12] = {0}, body[26];
  if (n >= 12) (void)src.at(0, 12, head);
  // RF64 / BW64: the sizes that do not fit 32 bits are 0xffffffff in place and stand in the ds64 chunk
  const bool rf64 = std::memcmp(head, "RF64", 4) == 0 || std::memcmp(head, "BW64", 4) == 0;
  if (n < 12 || !(rf64 || std::memcmp(head, "RIFF", 4) == 0) || std::memcmp(head + 8, "WAVE", 4) != 0) {
    g_file_error = "not a RIFF/WAVE file";
    return false;
  }
  size_t pos = 12;
  bool have_fmt = false, have_data = false, have_ds64 = false;
  uint64_t ds64_data = 0;
  while (pos + 8 <= n) {
    if (!src.at(pos, 8, head)) return false;
    uint64_t size = rd32(head + 4);
    if (rf64 && have_ds64 && size == 0xffffffffu && std::memcmp(head, "data", 4) == 0) size = ds64_data;
    const size_t avail = n - (pos + 8) < size ? n - (pos + 8) : (size_t)size;  // a truncated last chunk: what is there
    if (rf64 && std::memcmp(head, "ds64", 4) == 0 && avail >= 24) {  // RIFF size, data size, sample count
      if (!src.at(pos + 8, 24, body)) return false;
      ds64_data = rd64(body + 8), have_ds64 = true;
    }
    if (std::memcmp(head, "fmt ", 4) == 0 && avail >= 16) {
      if (!src.at(pos + 8, avail < 26 ? avail : 26, body)) return false;
      w.tag = rd16(body), w.channels = rd16(body + 2), w.sample_rate = (int)rd32(body + 4), w.bits = rd16(body + 14);
      w.block_align = rd16(body + 12);
      if (w.tag == 0xFFFE && avail >= 26) w.tag = rd16(body + 24);  // the real tag sits in the GUID
      have_fmt = true;
    } else if (std::memcmp(head, "data", 4) == 0) {
      data_pos = pos + 8, w.pcm_bytes = avail;
      have_data = true;
    } else if (std::memcmp(head, "fact", 4) == 0 && avail >= 4) {  // the sample count of a compressed format
      if (!src.at(pos + 8, 4, body)) return false;
      if (rd32(body) != 0xffffffffu) w.fact_frames = (int64_t)rd32(body);  // (RF64: the count is ds64's; the blocks decide)
    }
    if (size >= n - (pos + 8)) break;  // the file ends in this chunk
    pos += 8 + (size_t)size + (size & 1);
  }
  if (!have_fmt || !have_data) {
    g_file_error = "missing fmt or data chunk";
    return false;
  }
  int width = 0;
  if (w.tag == 1 && (w.bits == 8 || w.bits == 16 || w.bits == 24 || w.bits == 32)) width = w.bits / 8;
  if (w.tag == 3 && (w.bits == 32 || w.bits == 64)) width = w.bits / 8;
  if ((w.tag == 7 || w.tag == 6) && w.bits == 8) width = 1;  // G.711 mu-law, A-law
  if (w.tag == kWavTagIma) {
    // blocks of block_align bytes: 4 header bytes a channel, then groups of 4 bytes a channel (adpcm_host.h)
    if (w.bits != 4) {
      g_file_error = "unsupported IMA ADPCM sample size " + std::to_string(w.bits) + " (4 bits a sample are read)";
      return false;
    }
    if (w.channels < 1) {
      g_file_error = "zero channels";
      return false;
    }
    const int payload = w.block_align - 4 * w.channels;
    if (payload <= 0 || payload % (4 * w.channels) != 0) {
      g_file_error = "unsupported IMA ADPCM block align " + std::to_string(w.block_align) + " for " + std::to_string(w.channels) +
                     " channels (4 header bytes and whole groups of 4 bytes a channel are read)";
      return false;
    }
    w.n_frames = (int64_t)(w.pcm_bytes / (size_t)w.block_align) * ((int64_t)payload * 2 / w.channels + 1);  // whole blocks only
    if (w.fact_frames >= 0 && w.fact_frames < w.n_frames) w.n_frames = w.fact_frames;
    return true;
  }
  if (!width) {
    g_file_error = w.tag == 1 ? "unsupported PCM bit depth " + std::to_string(w.bits)
                              : "unsupported WAV format tag " + std::to_string(w.tag);
    return false;
  }
  if (w.channels < 1) {
    g_file_error = "zero channels";
    return false;
  }
  w.n_frames = (int64_t)(w.pcm_bytes / (size_t)width) / w.channels;
  return true;
}

bool wav_parse(const uint8_t* d, size_t n, WavInfo& w) {
  ByteSource src;
  src.mem = d, src.size = n;
  size_t data_pos = 0;
  if (!wav_walk(src, w, data_pos)) return false;
  w.pcm = d + data_pos;
  return true;
}

// samples -> float32 exactly as read_wav does (power-of-two scales: multiplying by the reciprocal is exact)
void wav_to_float(const WavInfo& w, float* out) {
  const int64_t n = w.n_frames * w.channels;
  const uint8_t* p = w.pcm;
  if (w.tag == 1 && w.bits == 16) {
    for (int64_t i = 0; i < n; ++i) out[i] = (float)(int16_t)rd16(p + 2 * i) * (1.0f / 32768.0f);
  } else if (w.tag == 1 && w.bits == 8) {
    for (int64_t i = 0; i < n; ++i) out[i] = ((float)p[i] - 128.0f) * (1.0f / 128.0f);
  } else if (w.tag == 1 && w.bits == 24) {
    for (int64_t i = 0; i < n; ++i) {
      int32_t v = (int32_t)p[3 * i] | ((int32_t)p[3 * i + 1] << 8) | ((int32_t)p[3 * i + 2] << 16);
      if (v >= 1 << 23) v -= 1 << 24;
      out[i] = (float)v / 8388608.0f;
    }
  } else if (w.tag == 1 && w.bits == 32) {
    for (int64_t i = 0; i < n; ++i) out[i] = (float)((double)(int32_t)rd32(p + 4 * i) / 2147483648.0);
  } else if (w.tag == 7) {
    for (int64_t i = 0; i < n; ++i) out[i] = (float)ulaw_expand(p[i]) * (1.0f / 32768.0f);
  } else if (w.tag == 6) {
    for (int64_t i = 0; i < n; ++i) out[i] = (float)alaw_expand(p[i]) * (1.0f / 32768.0f);
  } else if (w.tag == kWavTagIma) {
    std::vector<int16_t> pcm((size_t)n);
    ima_wav_decode(p, w.pcm_bytes, w.channels, w.block_align, w.n_frames, pcm.data());
    for (int64_t i = 0; i < n; ++i) out[i] = (float)pcm[(size_t)i] * (1.0f / 32768.0f);
  } else if (w.bits == 32) {
    std::memcpy(out, p, (size_t)n * 4);
  } else {
    for (int64_t i = 0; i < n; ++i) {
      double v;
      std::memcpy(&v, p + 8 * i, 8);
      out[i] = (float)v;
    }
  }
}

int wav_pcm_format(const WavInfo& w) {
  if (w.tag == 1) return w.bits == 8 ? BP_PCM_U8 : w.bits == 16 ? BP_PCM_S16 : w.bits == 24 ? BP_PCM_S24 : BP_PCM_S32;
  if (w.tag == 7 || w.tag == 6) return w.tag == 7 ? BP_PCM_ULAW : BP_PCM_ALAW;
  if (w.tag == kWavTagIma) return -1;
  return w.bits == 32 ? BP_PCM_F32 : BP_PCM_F64;
}

}  // namespace bp_file

using namespace bp_file;

extern "C" {

int bp_wav_info(const void* file, size_t nbytes, int* channels, int* sample_rate, int* bits_per_sample, int64_t* n_frames) {
  WavInfo w;
  if (!file || !wav_parse(static_cast<const uint8_t*>(file), nbytes, w)) {
    if (!file) g_file_error = "bp_wav_info: null pointer";
    return file ? BP_ERR_BAD_AUDIO : BP_ERR_INVALID_ARG;
  }
  if (channels) *channels = w.channels;
  if (sample_rate) *sample_rate = w.sample_rate;
  if (bits_per_sample) *bits_per_sample = w.bits;
  if (n_frames) *n_frames = w.n_frames;
  return BP_OK;
}

int bp_wav_decode(const void* file, size_t nbytes, float* pcm, int64_t max_frames, int64_t* n_frames) {
  WavInfo w;
  if (!file || !pcm) {
    g_file_error = "bp_wav_decode: null pointer";
    return BP_ERR_INVALID_ARG;
  }
  if (!wav_parse(static_cast<const uint8_t*>(file), nbytes, w)) return BP_ERR_BAD_AUDIO;
  if (n_frames) *n_frames = w.n_frames;
  if (w.n_frames > max_frames) {
    g_file_error = "bp_wav_decode: buffer too small";
    return BP_ERR_INVALID_ARG;
  }
  wav_to_float(w, pcm);
  return BP_OK;
}

}  // extern "C"
