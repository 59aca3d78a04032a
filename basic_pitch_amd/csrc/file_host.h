// What the host side of the file job shares across its sources: wav_file.cpp (RIFF/WAVE, RF64), pcm_file.cpp (AIFF, CAF,
// AU), adpcm_file.cpp (IMA ADPCM in WAV and CAF), note_writers.cpp (.csv and .mid bytes), file_io.cpp (reading and writing
// files, the thread's error string) and file_pipeline.cpp (the job itself, the only one of the six that calls the device
// library).  Internal: nothing here is
// part of the library's interface.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/basic_pitch_amd_adpcm.h"

namespace bp_file __attribute__((visibility("hidden"))) {

// what bp_files_last_error returns: the last failure of this thread in any of the four sources
extern thread_local std::string g_file_error;

// ---- wav_file.cpp
struct WavInfo {
  int tag = 0, channels = 0, sample_rate = 0, bits = 0;
  int block_align = 0;       // tag 0x11 (IMA ADPCM): the bytes of a block
  int64_t fact_frames = -1;  // the fact chunk's sample count; -1: no such chunk
  const uint8_t* pcm = nullptr;
  size_t pcm_bytes = 0;
  int64_t n_frames = 0;
};
constexpr int kWavTagIma = 0x11;  // IMA / DVI ADPCM: blocks, not samples (adpcm_host.h); wav_pcm_format has no code for it

// The bytes of a file by position: the whole file in memory, or an open file of which only the bytes asked for are read
// (bp_files_batch_probe and the batching workers decide a file's route from its headers alone).
struct ByteSource {
  const uint8_t* mem = nullptr;
  int fd = -1;
  size_t size = 0;
  bool at(size_t pos, size_t len, uint8_t* out) const;  // [pos, pos + len) lies inside the file
};

bool wav_walk(const ByteSource& src, WavInfo& w, size_t& data_pos);
bool wav_parse(const uint8_t* d, size_t n, WavInfo& w);
int wav_pcm_format(const WavInfo& w);  // the BP_PCM_* of the samples as the file stores them; tag 0x11: -1
void wav_to_float(const WavInfo& w, float* out);

// ITU-T G.711 in arithmetic: a code byte -> the value left-justified in 16 bits (RIFF/WAVE tags 7 / 6, AIFF-C, CAF, AU)
inline int ulaw_expand(uint32_t b) {
  const uint32_t u = ~b & 0xffu;
  const int t = (int)((((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u));
  return (u & 0x80u) ? 0x84 - t : t - 0x84;
}
inline int alaw_expand(uint32_t b) {
  const uint32_t a = (b ^ 0x55u) & 0xffu, s = (a >> 4) & 7u;
  int t = (int)((a & 15u) << 4);
  t = s == 0 ? t + 8 : s == 1 ? t + 0x108 : (t + 0x108) << (s - 1);
  return (a & 0x80u) ? t : -t;
}

// ---- pcm_file.cpp: the other containers of uncompressed samples, read like wav_walk from the headers alone.  Each fills
// every field of `lay` (format = the BP_PCM_* of the samples as the file stores them) or sets g_file_error.  Uses
// wav_file.cpp and file_io.cpp; nothing of wav_file.cpp, note_writers.cpp, file_io.cpp or the decoders uses it.
int pcm_container_of(const uint8_t* head, size_t size);  // BP_CONTAINER_* by a file's first 12 bytes (fewer: `size`), or 0
bool aiff_walk(const ByteSource& src, bp_pcm_file_layout& lay);
bool caf_walk(const ByteSource& src, bp_pcm_file_layout& lay);
bool au_walk(const ByteSource& src, bp_pcm_file_layout& lay);
bool pcm_file_walk(const ByteSource& src, bp_pcm_file_layout& lay);  // whichever of the four the file is (WAV: wav_walk)
void pcm_to_float(int format, const uint8_t* p, int64_t n_samples, float* out);  // the device's conversion, on the host

// ---- adpcm_file.cpp: IMA ADPCM in RIFF/WAVE (tag 0x11) and CAF (`ima4`), read like wav_walk from the headers alone
// (include/basic_pitch_amd_adpcm.h).  adpcm_kind: BP_ADPCM_* when the headers say the file is one of the two, 0 when it is
// something else (nothing set), -1 when it is one with a fault (g_file_error set).  Uses wav_file.cpp and file_io.cpp.
int adpcm_walk(const ByteSource& src, bp_adpcm_layout& lay);

// ---- note_writers.cpp
void notes_csv(const bp_note_event* ev, int64_t n, const int32_t* bends, std::string& out);
bool notes_midi(const bp_note_event* ev, int64_t n, const int32_t* bends, bool multiple_pitch_bends, double tempo,
                std::vector<uint8_t>& out);

// ---- file_io.cpp
// ensure(bytes) -> page-aligned buffer of at least that many bytes, or null (g_file_error set)
bool read_file_into(const std::string& path, const std::function<void*(size_t)>& ensure, size_t& n, bool direct,
                    bool* was_direct = nullptr);
bool write_new_file(const std::string& path, const void* data, size_t n);
std::string stem_of(const std::string& path);
std::string two_path_message(const std::string& t0, const std::string& p0, const std::string& t1, const std::string& p1,
                             const std::string& t2);

}  // namespace bp_file
