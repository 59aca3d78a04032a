#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <cstdint>
#include "../../include/basic_pitch_amd_containers.h"
// Mutated AIFF / AIFF-C, CAF, AU and RF64 headers through the parsers and the host decoder (csrc/pcm_file.cpp, wav_file.cpp).
// Links against the device-free sources alone, no stub for any library function: build it with the host sanitizers and it
// must print what the plain build prints.  usage: fuzz_containers ITERATIONS SEED_FILE...
// Every mutant lies in a malloc'd block of exactly its size, so a read past the file's end is a finding.
static uint64_t s = 88172645463325252ull;
static uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); }
int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s ITERATIONS SEED_FILE...\n", argv[0]); return 2; }
  const int n_it = atoi(argv[1]);
  std::vector<std::vector<uint8_t>> seeds;
  for (int a = 2; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> d(1 << 16);
    d.resize(fread(d.data(), 1, d.size(), f));
    fclose(f);
    if (d.empty()) { fprintf(stderr, "%s is empty\n", argv[a]); return 2; }
    seeds.push_back(d);
  }
  long ok = 0, bad = 0;
  uint64_t sum = 0;
  for (int it = 0; it < n_it; ++it) {
    std::vector<uint8_t> d = seeds[(size_t)it % seeds.size()];
    const size_t head = d.size() < 96 ? d.size() : 96;
    switch ((it / (int)seeds.size()) % 6) {
      case 0: break;  // the seed itself
      case 1: for (int k = 0; k < 1 + (int)(rnd() % 4); ++k) d[rnd() % head] = (uint8_t)rnd(); break;
      case 2: d.resize(rnd() % (d.size() + 1)); break;
      case 3: for (int k = 0; k < 1 + (int)(rnd() % 6); ++k) d[rnd() % head] ^= (uint8_t)(1u << (rnd() % 8)); break;
      case 4: { size_t p = rnd() % head; const uint8_t v = (rnd() & 1) ? 0xff : 0x00;  // sizes of all ones / zeros
                for (int k = 0; k < 4 + (int)(rnd() % 5) && p + k < d.size(); ++k) d[p + k] = v; break; }
      default: { size_t p = rnd() % head; for (int k = 0; k < 1 + (int)(rnd() % 31) && p + k < d.size(); ++k) d[p + k] = (uint8_t)rnd();
                 d.resize(head + rnd() % (d.size() - head + 1)); break; }
    }
    uint8_t* h = (uint8_t*)malloc(d.size() ? d.size() : 1);
    memcpy(h, d.data(), d.size());
    bp_pcm_file_layout lay;
    int rc = bp_pcm_file_layout_of(h, d.size(), &lay);
    if (rc == 0) {
      if (lay.n_frames < 0 || lay.channels < 1 || lay.data_start < 0 || (uint64_t)lay.data_start > d.size()) { fprintf(stderr, "bad layout at %d\n", it); return 1; }
      sum += (uint64_t)lay.n_frames * 31 + (uint64_t)lay.format * 7 + (uint64_t)lay.data_start;
      if (lay.n_frames * lay.channels < 5000000) {
        std::vector<float> out((size_t)(lay.n_frames * lay.channels) + 1);
        int64_t got = 0;
        rc = bp_pcm_file_decode(h, d.size(), out.data(), lay.n_frames, &got);
        if (rc != 0 || got != lay.n_frames) { fprintf(stderr, "decode disagrees with the layout at %d\n", it); return 1; }
        uint32_t bits;
        for (size_t i = 0; i < out.size() - 1; i += 17) { memcpy(&bits, &out[i], 4); sum += bits; }
      }
      if (lay.container == BP_CONTAINER_WAV) {  // RF64 through the WAV calls
        int c, r, b; int64_t nf;
        if (bp_wav_info(h, d.size(), &c, &r, &b, &nf) != 0 || nf != lay.n_frames) { fprintf(stderr, "bp_wav_info disagrees at %d\n", it); return 1; }
      }
    } else if (!bp_files_last_error()[0]) { fprintf(stderr, "a refusal without a message at %d\n", it); return 1; }
    free(h);
    (rc == 0 ? ok : bad)++;
  }
  printf("containers ok %ld bad %ld checksum %llu\n", ok, bad, (unsigned long long)sum);
  return 0;
}
