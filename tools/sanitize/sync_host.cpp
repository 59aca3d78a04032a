// The synchronisation checker (csrc/sync_host.cpp: no device) over seeded random maps, parameters, degenerate segments and
// malformed inputs as a program of its own: tests/test_sync_cpu.py builds it plain and with the host sanitizers (address,
// undefined) and asks both for the same line.  Every buffer is a heap block of exactly the size the call may touch.
// Usage: sync_host [cases]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/basic_pitch_amd_sync.h"

namespace {
uint64_t state = 0x9e3779b97f4a7c15ull;
uint32_t draw(uint32_t n) {  // 0 ... n - 1
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(state >> 33) % n;
}

std::vector<float> a_map(int64_t rows) {
  std::vector<float> note((size_t)(rows * BP_SYNC_PITCHES));
  const int kind = (int)draw(4);  // a thousand levels, eighths on stretches, one sounding pitch a stretch, silence
  for (size_t i = 0; i < note.size(); ++i) {
    const size_t t = i / BP_SYNC_PITCHES, q = i % BP_SYNC_PITCHES;
    if (kind == 0) note[i] = ((float)draw(1101) - 50.0f) / 1000.0f;
    if (kind == 1) note[i] = (float)((t / 7 + q % 12) % 9) / 8.0f;
    if (kind == 2) note[i] = q == 30 + (t / 5) % 12 ? 1.0f : 0.0f;
    if (kind == 3) note[i] = 0.0f;
  }
  if (rows > 0 && draw(12) == 0) {
    const float odd[3] = {std::numeric_limits<float>::quiet_NaN(), -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::infinity()};
    note[draw((uint32_t)note.size())] = odd[draw(3)];
  }
  return note;
}
}  // namespace

int main(int argc, char** argv) {
  const int cases = argc > 1 ? std::atoi(argv[1]) : 200;
  const int64_t rows_of[8] = {0, 1, 2, 7, 33, 64, 130, 301};
  const int32_t hops[5] = {1, 3, 4, 17, BP_SYNC_MAX_HOP}, bands[5] = {0, 0, 1, 3, 20};
  long long paths = 0, flagged = 0, empty = 0, refused = 0, cells = 0, steps = 0;
  int64_t totals = 0;
  uint64_t path_sum = 0;
  for (int c = 0; c < cases; ++c) {
    const int64_t rows_a = rows_of[draw(8)], rows_b = rows_of[draw(8)];
    const std::vector<float> a = a_map(rows_a), b = a_map(rows_b);
    bp_sync_params p;
    bp_sync_params_default(&p);
    p.threshold_q = (int32_t)draw(4) * 128, p.hop = hops[draw(5)], p.band = bands[draw(5)];
    p.min_pitch = (int32_t)draw(40), p.max_pitch = p.min_pitch + (int32_t)draw((uint32_t)(BP_SYNC_PITCHES - p.min_pitch));
    const int64_t N = (rows_a + p.hop - 1) / p.hop, M = (rows_b + p.hop - 1) / p.hop, room = N > 0 && M > 0 ? N + M - 1 : 0;
    std::vector<int32_t> path((size_t)(2 * room), 200);  // exactly the region
    bp_sync_summary s{-7, -7, -7, -7, -7, -7};
    // the refusals first: each leaves the outputs alone
    {
      bp_sync_params q = p;
      const int which = (int)draw(7);
      if (which == 0) q.threshold_q = BP_CHORD_Q_ONE + 1;
      if (which == 1) q.hop = 0;
      if (which == 2) q.hop = BP_SYNC_MAX_HOP + 1;
      if (which == 3) q.band = -1;
      if (which == 4) q.band = BP_SYNC_MAX_UNITS + 1;
      if (which == 5) q.reserved[draw(3)] = 1;
      if (which == 6) q.max_pitch = BP_SYNC_PITCHES;
      if (bp_sync_rows(a.data(), rows_a, b.data(), rows_b, &q, path.data(), room, &s) != BP_ERR_INVALID_ARG) return 2;
      ++refused;
      if (room > 0) {
        if (bp_sync_rows(a.data(), rows_a, b.data(), rows_b, &p, path.data(), room - 1, &s) != BP_ERR_INVALID_ARG) return 4;
        if (bp_sync_rows(a.data(), rows_a, b.data(), rows_b, &p, nullptr, room, &s) != BP_ERR_INVALID_ARG) return 4;
        if (bp_sync_rows(nullptr, rows_a, b.data(), rows_b, &p, path.data(), room, &s) != BP_ERR_INVALID_ARG) return 4;
        refused += 3;
      }
      if (bp_sync_rows(a.data(), -1, b.data(), rows_b, &p, path.data(), room, &s) != BP_ERR_INVALID_ARG) return 5;
      if (bp_sync_rows(a.data(), rows_a, b.data(), rows_b, &p, path.data(), room, nullptr) != BP_ERR_INVALID_ARG) return 5;
      refused += 2;
      if (s.status != -7 || s.total != -7) return 3;
      for (int32_t e : path)
        if (e != 200) return 3;
    }
    if (bp_sync_rows(rows_a ? a.data() : nullptr, rows_a, rows_b ? b.data() : nullptr, rows_b, &p, room ? path.data() : nullptr, room, &s) != BP_OK)
      return 6;
    if (s.units_a != N || s.units_b != M || s.path_first != 0) return 7;
    if (s.status == 0) {
      ++paths;
      if (s.n_path < (N > M ? N : M) || s.n_path > room || s.total < 0 || s.total > (N + M) * (int64_t)BP_SYNC_MAX_GAIN) return 8;
      if (path[0] != 0 || path[1] != 0 || path[(size_t)(2 * s.n_path - 2)] != N - 1 || path[(size_t)(2 * s.n_path - 1)] != M - 1) return 9;
      const int64_t widest = (N > M ? N : M) - 1;
      for (int64_t k = 0; k < s.n_path; ++k) {
        const int64_t i = path[(size_t)(2 * k)], j = path[(size_t)(2 * k + 1)];
        if (k > 0) {
          const int64_t di = i - path[(size_t)(2 * k - 2)], dj = j - path[(size_t)(2 * k - 1)];
          if (di < 0 || di > 1 || dj < 0 || dj > 1 || di + dj == 0) return 10;  // monotone, by the three steps
        }
        const int64_t off = i * (M - 1) - j * (N - 1);
        if (p.band > 0 && (off < 0 ? -off : off) > p.band * widest) return 11;  // inside the band
        path_sum += (uint64_t)(i * 3 + j) * (uint64_t)(k + 1);
      }
      for (int64_t e = 2 * s.n_path; e < 2 * room; ++e)
        if (path[(size_t)e] != -1) return 12;
      cells += N * M, steps += s.n_path, totals += s.total % 1000003;
    } else {
      flagged += s.status == 1, empty += s.status == 2;
      if (s.n_path != 0 || s.total != 0) return 13;
      for (int32_t e : path)
        if (e != -1) return 14;
    }
  }
  std::printf("sync %d cases: paths %lld flagged %lld empty %lld refused %lld cells %lld steps %lld path %llu totals %lld\n", cases, paths,
              flagged, empty, refused, cells, steps, (unsigned long long)path_sum, (long long)totals);
  return 0;
}
