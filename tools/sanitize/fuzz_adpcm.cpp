#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <cstdint>
#include "../../include/basic_pitch_amd_adpcm.h"
// G.711 and IMA ADPCM files through the host parsers and decoders (csrc/adpcm_file.cpp, wav_file.cpp, pcm_file.cpp): every
// prefix of every seed file, then the seed with every header field — each aligned 16-, 32- and 64-bit word of its first 128
// bytes — set to its extremes (all zeros, all ones, the sign bit alone, all but the sign bit, in either byte order).  Links
// against the device-free sources alone, no stub for any library function: build it with the host sanitizers and it must
// print what the plain build prints.  usage: fuzz_adpcm SEED_FILE...
// Every input lies in a malloc'd block of exactly its size, so a read past the file's end is a finding.
static long ok = 0, bad = 0;
static uint64_t sum = 0;

static int one(const std::vector<uint8_t>& d, const char* what, long at) {
  uint8_t* h = (uint8_t*)malloc(d.size() ? d.size() : 1);
  if (!d.empty()) memcpy(h, d.data(), d.size());
  int any = 0;
  bp_adpcm_layout lay;
  int rc = bp_adpcm_layout_of(h, d.size(), &lay);
  if (rc == 0) {
    any = 1;
    if (lay.n_frames < 0 || lay.channels < 1 || lay.block_bytes < 1 || lay.block_frames < 1 || lay.data_start < 0 || lay.data_bytes < 0 ||
        (uint64_t)(lay.data_start + lay.data_bytes) > d.size() || lay.n_frames > lay.data_bytes / lay.block_bytes * lay.block_frames) {
      fprintf(stderr, "bad layout: %s %ld\n", what, at);
      return 1;
    }
    sum += (uint64_t)lay.n_frames * 31 + (uint64_t)lay.codec * 7 + (uint64_t)lay.data_start;
    if (lay.n_frames * lay.channels < 5000000) {
      std::vector<int16_t> out((size_t)(lay.n_frames * lay.channels) + 1, 12345);
      int64_t got = 0;
      rc = bp_adpcm_decode(h, d.size(), out.data(), lay.n_frames, &got);
      if (rc != 0 || got != lay.n_frames || out.back() != 12345) { fprintf(stderr, "decode disagrees with the layout: %s %ld\n", what, at); return 1; }
      for (size_t i = 0; i + 1 < out.size(); i += 13) sum += (uint16_t)out[i];
    }
  } else if (!bp_files_last_error()[0]) { fprintf(stderr, "a refusal without a message: %s %ld\n", what, at); return 1; }
  int c = 0, r = 0, b = 0; int64_t nf = 0;
  rc = bp_wav_info(h, d.size(), &c, &r, &b, &nf);
  if (rc == 0) {
    any = 1;
    if (nf < 0 || c < 1) { fprintf(stderr, "bad bp_wav_info: %s %ld\n", what, at); return 1; }
    if (nf * c < 5000000) {
      std::vector<float> out((size_t)(nf * c) + 1, 7.0f);
      int64_t got = 0;
      if (bp_wav_decode(h, d.size(), out.data(), nf, &got) != 0 || got != nf || out.back() != 7.0f) { fprintf(stderr, "bp_wav_decode disagrees: %s %ld\n", what, at); return 1; }
      uint32_t bits;
      for (size_t i = 0; i + 1 < out.size(); i += 17) { memcpy(&bits, &out[i], 4); sum += bits; }
    }
  }
  bp_pcm_file_layout play;
  if (bp_pcm_file_layout_of(h, d.size(), &play) == 0) {
    any = 1;
    if (play.n_frames * play.channels < 5000000) {
      std::vector<float> out((size_t)(play.n_frames * play.channels) + 1);
      int64_t got = 0;
      if (bp_pcm_file_decode(h, d.size(), out.data(), play.n_frames, &got) != 0 || got != play.n_frames) { fprintf(stderr, "bp_pcm_file_decode disagrees: %s %ld\n", what, at); return 1; }
    }
  }
  free(h);
  (any ? ok : bad)++;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s SEED_FILE...\n", argv[0]); return 2; }
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> seed(1 << 16);
    seed.resize(fread(seed.data(), 1, seed.size(), f));
    fclose(f);
    if (seed.empty()) { fprintf(stderr, "%s is empty\n", argv[a]); return 2; }
    for (size_t n = 0; n <= seed.size(); ++n)  // every prefix
      if (one(std::vector<uint8_t>(seed.begin(), seed.begin() + (long)n), argv[a], (long)n)) return 1;
    const size_t head = seed.size() < 128 ? seed.size() : 128;
    for (int width = 2; width <= 8; width *= 2)
      for (size_t p = 0; p + width <= head; p += 2)
        for (int v = 0; v < 6; ++v) {
          std::vector<uint8_t> d = seed;
          for (int k = 0; k < width; ++k) {
            const bool top_le = k == width - 1, top_be = k == 0;
            uint8_t byte = v == 0 ? 0x00 : v == 1 ? 0xff : 0;
            if (v == 2) byte = top_le ? 0x80 : 0x00;  // the sign bit alone, little-endian
            if (v == 3) byte = top_le ? 0x7f : 0xff;  // all but the sign bit, little-endian
            if (v == 4) byte = top_be ? 0x80 : 0x00;  // ... big-endian
            if (v == 5) byte = top_be ? 0x7f : 0xff;
            d[p + k] = byte;
          }
          if (one(d, argv[a], -(long)(p * 100 + width * 10 + v))) return 1;
        }
  }
  printf("adpcm ok %ld bad %ld checksum %llu\n", ok, bad, (unsigned long long)sum);
  return 0;
}
