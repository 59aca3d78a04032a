// AIFF / AIFF-C, CAF and AU, on the host alone: headers around uncompressed samples (include/basic_pitch_amd_containers.h
// names what is read of each).  Like wav_walk, a parser reads the headers from an open file and says what the samples are
// and where they lie; the samples themselves go to the device as the file stores them (audio_ingest.hip pcm_sample<FMT>).
// pcm_to_float is that conversion on the host, the checker behind bp_pcm_file_decode.  RF64 / BW64 is wav_walk's.
// Nothing here calls the device library.  Not read: the little-endian AU variant (`dns.`), Sony Wave64, MS ADPCM; IMA ADPCM
// (WAV tag 0x11, CAF ima4) is adpcm_file.cpp's.
//   AIFF:   Audio Interchange File Format 1.3 (Apple, 1989); AIFF-C draft 08/26/91; `sowt`, `fl32`, `in24`: Apple TN 2053
//   CAF:    Apple Core Audio Format Specification 1.0
//   AU:     the Sun / NeXT audio file header (audio_filehdr)
//   G.711:  ITU-T G.711, the expansion in arithmetic
#include <cmath>
#include <cstring>

#include "file_host.h"

namespace bp_file {

namespace {

uint16_t be16(const uint8_t* p) { return (uint16_t)((p[0] << 8) | p[1]); }
uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
uint64_t be64(const uint8_t* p) { return ((uint64_t)be32(p) << 32) | be32(p + 4); }
bool is(const uint8_t* p, const char* id) { return std::memcmp(p, id, 4) == 0; }

// a four-character code as text, unprintable bytes as '?'
std::string fourcc(const uint8_t* p) {
  std::string s(4, '?');
  for (int i = 0; i < 4; ++i)
    if (p[i] >= 0x20 && p[i] < 0x7f) s[i] = (char)p[i];
  return s;
}

bool fail(const std::string& why) {
  g_file_error = why;
  return false;
}

// a header's sample rate as the nearest integer the ingest can be asked for
bool take_rate(double rate, bp_pcm_file_layout& lay) {
  if (!(rate >= 0.5 && rate < 2147483647.0)) return fail("bad sample rate in the header");
  lay.sample_rate = (int32_t)std::llround(rate);
  return true;
}

int width_of(int format) {
  static const int width[] = {4, 2, 3, 4, 1, 8, 2, 3, 4, 4, 8, 1, 1, 1};  // track_api.hip pcm_width
  return width[format];
}

// integer PCM of `bytes` bytes a sample: big-endian, little-endian (one byte has no order: signed either way)
int int_format(int bytes, bool little) {
  switch (bytes) {
    case 1: return BP_PCM_S8;
    case 2: return little ? BP_PCM_S16 : BP_PCM_S16_BE;
    case 3: return little ? BP_PCM_S24 : BP_PCM_S24_BE;
    default: return little ? BP_PCM_S32 : BP_PCM_S32_BE;
  }
}

// frames: the smaller of the header's count and what the file holds (a truncated file: what is there)
void take_frames(uint64_t header_frames, uint64_t data_bytes, bp_pcm_file_layout& lay) {
  const uint64_t held = data_bytes / ((uint64_t)width_of(lay.format) * (uint64_t)lay.channels);
  lay.n_frames = (int64_t)(held < header_frames ? held : header_frames);
}

}  // namespace

int pcm_container_of(const uint8_t* head, size_t size) {
  if (size >= 12 && (is(head, "RIFF") || is(head, "RF64") || is(head, "BW64")) && is(head + 8, "WAVE")) return BP_CONTAINER_WAV;
  if (size >= 12 && is(head, "FORM") && (is(head + 8, "AIFF") || is(head + 8, "AIFC"))) return BP_CONTAINER_AIFF;
  if (size >= 4 && is(head, "caff")) return BP_CONTAINER_CAF;
  if (size >= 4 && is(head, ".snd")) return BP_CONTAINER_AU;
  return 0;
}

// FORM AIFF | AIFC: the 12-byte head, every chunk's 8-byte head, 22 bytes of COMM and 8 of SSND
bool aiff_walk(const ByteSource& src, bp_pcm_file_layout& lay) {
  const size_t n = src.size;
  uint8_t head[12] = {0}, body[22];
  if (n < 12 || !src.at(0, 12, head) || pcm_container_of(head, n) != BP_CONTAINER_AIFF) return fail("not an AIFF file");
  const bool aifc = is(head + 8, "AIFC");
  lay = bp_pcm_file_layout{};
  lay.container = BP_CONTAINER_AIFF;
  bool have_comm = false, have_ssnd = false;
  uint64_t comm_frames = 0, data_bytes = 0;
  uint8_t type[4] = {'N', 'O', 'N', 'E'};
  double rate = 0.0;
  size_t pos = 12;
  while (pos + 8 <= n) {
    if (!src.at(pos, 8, head)) return false;
    const uint32_t size = be32(head + 4);
    const size_t avail = n - (pos + 8) < size ? n - (pos + 8) : size;
    if (is(head, "COMM")) {
      const size_t need = aifc ? 22 : 18;
      if (avail < need) return fail("truncated COMM chunk: " + std::to_string(avail) + " of " + std::to_string(need) + " bytes");
      if (!src.at(pos + 8, need, body)) return false;
      lay.channels = be16(body), comm_frames = be32(body + 2), lay.bits_per_sample = be16(body + 6);
      // 80-bit extended: sign and 15-bit exponent (bias 16383), 64-bit mantissa with an explicit integer bit
      const int exponent = be16(body + 8) & 0x7fff;
      rate = std::ldexp((double)be64(body + 10), exponent - 16383 - 63);
      if (body[8] & 0x80) rate = -rate;
      if (aifc) std::memcpy(type, body + 18, 4);  // (the Pascal string that names the type follows: not read)
      have_comm = true;
    } else if (is(head, "SSND")) {
      if (avail < 8) return fail("truncated SSND chunk");
      if (!src.at(pos + 8, 8, body)) return false;
      const uint64_t offset = be32(body);  // (then the block size: alignment advice)
      data_bytes = avail - 8 > offset ? avail - 8 - offset : 0;
      lay.data_start = (int64_t)(pos + 16 + (data_bytes ? offset : avail - 8));
      have_ssnd = true;
    }
    if (size >= n - (pos + 8)) break;  // the file ends in this chunk
    pos += 8 + (size_t)size + (size & 1);
  }
  if (!have_comm) return fail("missing COMM chunk");
  if (!have_ssnd && comm_frames != 0) return fail("missing SSND chunk");  // (a file without frames may leave it out)
  if (!have_ssnd) lay.data_start = (int64_t)n;
  if (lay.channels < 1) return fail("zero channels");
  const int bits = lay.bits_per_sample, bytes = (bits + 7) / 8;
  const bool ints = bits >= 1 && bits <= 32;
  if (is(type, "NONE") || is(type, "twos") || is(type, "in24") || is(type, "in32") || is(type, "sowt")) {
    if (!ints) return fail("unsupported AIFF sample size " + std::to_string(bits));
    lay.format = int_format(bytes, is(type, "sowt"));
  } else if ((is(type, "fl32") || is(type, "FL32")) && bits == 32) {
    lay.format = BP_PCM_F32_BE;
  } else if ((is(type, "fl64") || is(type, "FL64")) && bits == 64) {
    lay.format = BP_PCM_F64_BE;
  } else if (is(type, "ulaw") || is(type, "ULAW")) {
    lay.format = BP_PCM_ULAW, lay.bits_per_sample = 8;  // (COMM says 16 here: the size of the expanded sample)
  } else if (is(type, "alaw") || is(type, "ALAW")) {
    lay.format = BP_PCM_ALAW, lay.bits_per_sample = 8;
  } else if (is(type, "raw ") && bits >= 1 && bits <= 8) {
    lay.format = BP_PCM_U8;
  } else if (is(type, "fl32") || is(type, "FL32") || is(type, "fl64") || is(type, "FL64") || is(type, "raw ")) {
    return fail("unsupported sample size " + std::to_string(bits) + " for AIFF-C compression type '" + fourcc(type) + "'");
  } else {
    return fail("unsupported AIFF-C compression type '" + fourcc(type) + "'");
  }
  if (!take_rate(rate, lay)) return false;
  take_frames(comm_frames, data_bytes, lay);
  return true;
}

// caff: the 8-byte head, every chunk's 12-byte head and the 32 bytes of desc
bool caf_walk(const ByteSource& src, bp_pcm_file_layout& lay) {
  const size_t n = src.size;
  uint8_t head[12] = {0}, body[32];
  if (n < 8 || !src.at(0, 8, head) || !is(head, "caff")) return fail("not a CAF file");
  if (be16(head + 4) != 1) return fail("unsupported CAF version " + std::to_string(be16(head + 4)));
  lay = bp_pcm_file_layout{};
  lay.container = BP_CONTAINER_CAF;
  bool have_desc = false, have_data = false;
  uint64_t data_bytes = 0;
  size_t pos = 8;
  while (pos + 12 <= n) {
    if (!src.at(pos, 12, head)) return false;
    const int64_t size = (int64_t)be64(head + 4);
    const size_t rest = n - (pos + 12);
    const bool to_end = size < 0 || (uint64_t)size >= rest;  // -1 (data alone may say so): to the end of the file
    const size_t avail = to_end ? rest : (size_t)size;
    if (is(head, "desc")) {
      if (avail < 32) return fail("truncated desc chunk");
      if (!src.at(pos + 12, 32, body)) return false;
      have_desc = true;
    } else if (is(head, "data")) {
      data_bytes = avail > 4 ? avail - 4 : 0;  // behind the edit count
      lay.data_start = (int64_t)(pos + 12 + (avail < 4 ? avail : 4));
      have_data = true;
    } else if (size < 0) {
      return fail("negative size of CAF chunk '" + fourcc(head) + "'");
    }
    if (to_end) break;
    pos += 12 + (size_t)size;
  }
  if (!have_desc || !have_data) return fail("missing desc or data chunk");
  double rate;
  const uint64_t rate_bits = be64(body);
  std::memcpy(&rate, &rate_bits, 8);
  const uint8_t* id = body + 8;
  const uint32_t flags = be32(body + 12), packet_bytes = be32(body + 16), packet_frames = be32(body + 20);
  const uint32_t channels = be32(body + 24), bits = be32(body + 28);
  if (channels < 1) return fail("zero channels");
  if (channels > 65535) return fail("bad channel count " + std::to_string(channels));
  lay.channels = (int32_t)channels, lay.bits_per_sample = (int32_t)(bits > 64 ? 0 : bits);
  if (is(id, "lpcm")) {
    const bool is_float = flags & 1, little = flags & 2;
    if (is_float && (bits == 32 || bits == 64))
      lay.format = bits == 32 ? (little ? BP_PCM_F32 : BP_PCM_F32_BE) : (little ? BP_PCM_F64 : BP_PCM_F64_BE);
    else if (!is_float && (bits == 8 || bits == 16 || bits == 24 || bits == 32))
      lay.format = int_format((int)bits / 8, little);
    else
      return fail(std::string("unsupported CAF lpcm of ") + std::to_string(bits) + (is_float ? "-bit floats" : "-bit integers"));
  } else if (is(id, "ulaw") || is(id, "alaw")) {
    lay.format = is(id, "ulaw") ? BP_PCM_ULAW : BP_PCM_ALAW, lay.bits_per_sample = 8;
  } else {
    return fail("unsupported CAF format '" + fourcc(id) + "'");
  }
  if (packet_frames != 1 || packet_bytes != channels * (uint32_t)width_of(lay.format))
    return fail("unsupported CAF packet layout: " + std::to_string(packet_frames) + " frames in " + std::to_string(packet_bytes) +
                " bytes a packet (read: 1 frame of " + std::to_string(channels * (uint32_t)width_of(lay.format)) + " bytes)");
  if (!take_rate(rate, lay)) return false;
  take_frames(~(uint64_t)0, data_bytes, lay);
  return true;
}

// .snd: six big-endian words; an annotation may follow them
bool au_walk(const ByteSource& src, bp_pcm_file_layout& lay) {
  const size_t n = src.size;
  uint8_t head[24] = {0};
  if (n < 4 || !src.at(0, 4, head) || !is(head, ".snd")) return fail("not an AU file");
  if (n < 24 || !src.at(0, 24, head)) return fail("truncated AU header");
  lay = bp_pcm_file_layout{};
  lay.container = BP_CONTAINER_AU;
  const uint32_t header_bytes = be32(head + 4), data_size = be32(head + 8), encoding = be32(head + 12);
  const uint32_t channels = be32(head + 20);
  if (header_bytes < 24) return fail("bad AU header size " + std::to_string(header_bytes));
  switch (encoding) {
    case 1: lay.format = BP_PCM_ULAW, lay.bits_per_sample = 8; break;
    case 2: lay.format = BP_PCM_S8, lay.bits_per_sample = 8; break;
    case 3: lay.format = BP_PCM_S16_BE, lay.bits_per_sample = 16; break;
    case 4: lay.format = BP_PCM_S24_BE, lay.bits_per_sample = 24; break;
    case 5: lay.format = BP_PCM_S32_BE, lay.bits_per_sample = 32; break;
    case 6: lay.format = BP_PCM_F32_BE, lay.bits_per_sample = 32; break;
    case 7: lay.format = BP_PCM_F64_BE, lay.bits_per_sample = 64; break;
    case 27: lay.format = BP_PCM_ALAW, lay.bits_per_sample = 8; break;
    default: return fail("unsupported AU encoding " + std::to_string(encoding));
  }
  if (channels < 1) return fail("zero channels");
  if (channels > 65535) return fail("bad channel count " + std::to_string(channels));
  lay.channels = (int32_t)channels;
  if (!take_rate((double)be32(head + 16), lay)) return false;
  const size_t start = header_bytes < n ? header_bytes : n;
  lay.data_start = (int64_t)start;
  uint64_t data_bytes = n - start;
  if (data_size != 0xffffffffu && data_size < data_bytes) data_bytes = data_size;  // 0xffffffff: to the end of the file
  take_frames(~(uint64_t)0, data_bytes, lay);
  return true;
}

bool pcm_file_walk(const ByteSource& src, bp_pcm_file_layout& lay) {
  uint8_t magic[12] = {0};
  if (src.size && !src.at(0, src.size < 12 ? src.size : 12, magic)) return false;
  switch (pcm_container_of(magic, src.size)) {
    case BP_CONTAINER_WAV: {
      WavInfo w;
      size_t data_pos = 0;
      if (!wav_walk(src, w, data_pos)) return false;
      if (w.tag == kWavTagIma) return fail("IMA ADPCM samples are blocks, not PCM of a bp_pcm_format (bp_adpcm_layout_of reads the file)");
      lay = bp_pcm_file_layout{};
      lay.container = BP_CONTAINER_WAV, lay.format = wav_pcm_format(w), lay.channels = w.channels, lay.sample_rate = w.sample_rate;
      lay.bits_per_sample = w.bits, lay.n_frames = w.n_frames, lay.data_start = (int64_t)data_pos;
      return true;
    }
    case BP_CONTAINER_AIFF: return aiff_walk(src, lay);
    case BP_CONTAINER_CAF: return caf_walk(src, lay);
    case BP_CONTAINER_AU: return au_walk(src, lay);
    default: return fail("not a WAV, AIFF, CAF or AU file");
  }
}

// sample i of every format as pcm_sample<FMT> makes it on the device (power-of-two scales: exact)
void pcm_to_float(int format, const uint8_t* p, int64_t n, float* out) {
  auto word = [&](int64_t i, int bytes, bool big) {  // the unsigned word of sample i
    uint64_t v = 0;
    for (int b = 0; b < bytes; ++b) v |= (uint64_t)p[(int64_t)bytes * i + b] << 8 * (big ? bytes - 1 - b : b);
    return v;
  };
  auto s24 = [](uint64_t v) { return (float)((int32_t)v - (v >= 1u << 23 ? 1 << 24 : 0)) * (1.0f / 8388608.0f); };
  auto f32 = [](uint64_t v) {
    const uint32_t w = (uint32_t)v;
    float f;
    std::memcpy(&f, &w, 4);
    return f;
  };
  auto f64 = [](uint64_t v) {
    double d;
    std::memcpy(&d, &v, 8);
    return (float)d;
  };
  for (int64_t i = 0; i < n; ++i) {
    switch (format) {
      case BP_PCM_S16: out[i] = (float)(int16_t)word(i, 2, false) * (1.0f / 32768.0f); break;
      case BP_PCM_S16_BE: out[i] = (float)(int16_t)word(i, 2, true) * (1.0f / 32768.0f); break;
      case BP_PCM_S24: out[i] = s24(word(i, 3, false)); break;
      case BP_PCM_S24_BE: out[i] = s24(word(i, 3, true)); break;
      case BP_PCM_S32: out[i] = (float)((double)(int32_t)word(i, 4, false) * (1.0 / 2147483648.0)); break;
      case BP_PCM_S32_BE: out[i] = (float)((double)(int32_t)word(i, 4, true) * (1.0 / 2147483648.0)); break;
      case BP_PCM_U8: out[i] = ((float)p[i] - 128.0f) * (1.0f / 128.0f); break;
      case BP_PCM_S8: out[i] = (float)(int8_t)p[i] * (1.0f / 128.0f); break;
      case BP_PCM_ULAW: out[i] = (float)ulaw_expand(p[i]) * (1.0f / 32768.0f); break;
      case BP_PCM_ALAW: out[i] = (float)alaw_expand(p[i]) * (1.0f / 32768.0f); break;
      case BP_PCM_F64: out[i] = f64(word(i, 8, false)); break;
      case BP_PCM_F64_BE: out[i] = f64(word(i, 8, true)); break;
      case BP_PCM_F32_BE: out[i] = f32(word(i, 4, true)); break;
      default: out[i] = f32(word(i, 4, false)); break;
    }
  }
}

}  // namespace bp_file

using namespace bp_file;

extern "C" {

int bp_pcm_file_layout_of(const void* file, size_t nbytes, bp_pcm_file_layout* out) {
  if (!file || !out) {
    g_file_error = "bp_pcm_file_layout_of: null pointer";
    return BP_ERR_INVALID_ARG;
  }
  ByteSource src;
  src.mem = static_cast<const uint8_t*>(file), src.size = nbytes;
  return pcm_file_walk(src, *out) ? BP_OK : BP_ERR_BAD_AUDIO;
}

int bp_pcm_file_decode(const void* file, size_t nbytes, float* pcm, int64_t max_frames, int64_t* n_frames) {
  if (!file || !pcm) {
    g_file_error = "bp_pcm_file_decode: null pointer";
    return BP_ERR_INVALID_ARG;
  }
  bp_pcm_file_layout lay;
  ByteSource src;
  src.mem = static_cast<const uint8_t*>(file), src.size = nbytes;
  if (!pcm_file_walk(src, lay)) return BP_ERR_BAD_AUDIO;
  if (n_frames) *n_frames = lay.n_frames;
  if (lay.n_frames > max_frames) {
    g_file_error = "bp_pcm_file_decode: buffer too small";
    return BP_ERR_INVALID_ARG;
  }
  pcm_to_float(lay.format, src.mem + lay.data_start, lay.n_frames * lay.channels, pcm);
  return BP_OK;
}

}  // extern "C"
