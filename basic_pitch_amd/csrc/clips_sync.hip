// Pairs of the segments of a job against each other, of the note rows alone (include/basic_pitch_amd_sync.h, sync.hip,
// DESIGN.md 25): the sink behind run_clips (clips_job.h) and its entry points.  Host code only.
#include <algorithm>
#include <cstring>

#include "../../include/basic_pitch_amd_sync.h"
#include "clips_job.h"

using namespace bp;

extern "C" const char* bp_internal_sync_bad_params(const bp_sync_params* p);  // sync_host.cpp

namespace {

// A summary per pair under `params`, and the pairs' regions of path one after the other (room for max_path entries).
struct SyncSink final : JobSink {
  struct Args {
    int64_t n_pairs;
    const bp_sync_pair* pairs;
    const bp_sync_params* params;
    bp_sync_summary* summaries;
    int32_t* path;
    int64_t max_path;
  } a;
  std::vector<SyncSeg> segs;    // the segments with rows that a pair names
  std::vector<SyncPair> pairs;  // the pairs with rows on at least one side (a side without rows: -1)
  std::vector<int64_t> pair_of;  // their indices in the caller's table
  int64_t units = 0, entries = 0, pred_bytes = 0;
  int max_n = 0, max_m = 0;
  explicit SyncSink(const Args& args) : a(args) {}

  // the note rows alone, read where they lie unless they are in host memory (the loads are a float's: no alignment is asked)
  MapsUse use(bp_handle h) const override { return MapsUse{true, false, false, false, false, &h->sy_note, nullptr, nullptr}; }

  int check(bp_handle h, const char* what, int64_t n_segs) override {
    auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
    if (n_segs < 0 || a.n_pairs < 0) return invalid("negative n_segments / n_clips or n_pairs");
    if (a.n_pairs > 0 && (!a.pairs || !a.summaries)) return invalid("null pairs or summaries");
    if (const char* why = bp_internal_sync_bad_params(a.params)) return invalid(std::string("params: ") + why);
    if (!check_room(a.max_path, a.path)) return invalid("negative max_path, or room without a buffer");
    for (int64_t p = 0; p < a.n_pairs; ++p)
      if (a.pairs[p].a < 0 || a.pairs[p].a >= n_segs || a.pairs[p].b < 0 || a.pairs[p].b >= n_segs)
        return invalid("pair " + std::to_string(p) + ": (" + std::to_string(a.pairs[p].a) + ", " + std::to_string(a.pairs[p].b) +
                       ") names a segment outside 0 ... " + std::to_string(n_segs - 1));
    return BP_OK;
  }

  // the bounds, the room, the results of the pairs without any rows, and for the others their segments' units and their
  // regions of the pools
  int plan(bp_handle h, const char* what, int64_t n, const int64_t* offs, bool* queued) override {
    auto invalid = [&](const std::string& why) { return bp::invalid(h, what, why); };
    if (int rc = check_rows_in_all(h, what, offs[n])) return rc;
    const int64_t hop = a.params->hop;
    auto units_of = [&](int64_t i) { return (offs[i + 1] - offs[i] + hop - 1) / hop; };
    int64_t cells = 0, room = 0;
    for (int64_t p = 0; p < a.n_pairs; ++p) {
      const int64_t side[2] = {a.pairs[p].a, a.pairs[p].b}, N = units_of(side[0]), M = units_of(side[1]);
      for (int64_t i : side)
        if (units_of(i) > BP_SYNC_MAX_UNITS)
          return invalid("pair " + std::to_string(p) + ": segment " + std::to_string(i) + " has " + std::to_string(units_of(i)) +
                         " units, more than BP_SYNC_MAX_UNITS (" + std::to_string(BP_SYNC_MAX_UNITS) + ")");
      cells += N * M, room += N > 0 && M > 0 ? N + M - 1 : 0;
      if (cells > BP_SYNC_MAX_CELLS)
        return invalid("pair " + std::to_string(p) + ": with it the pairs have more than BP_SYNC_MAX_CELLS (" + std::to_string(BP_SYNC_MAX_CELLS) + ") cells");
      if (N > 0 && M > 0) max_n = std::max<int>(max_n, (int)N), max_m = std::max<int>(max_m, (int)M);
    }
    const SyncPlan variant = sync_plan(max_m);
    for (int64_t p = 0; p < a.n_pairs; ++p) {
      const int64_t N = units_of(a.pairs[p].a), M = units_of(a.pairs[p].b);
      if (N > 0 && M > 0) pred_bytes += sync_pred_bytes(variant, N, M);
      if (pred_bytes > kSyncMaxPredBytes)
        return invalid("pair " + std::to_string(p) + ": with it the pairs' predecessors take more than BP_SYNC_MAX_PRED_BYTES (" +
                       std::to_string(BP_SYNC_MAX_PRED_BYTES) + ") bytes");
    }
    if (a.max_path < room)
      return invalid("room for " + std::to_string(a.max_path) + " path entries, but the pairs need " + std::to_string(room) +
                     " (nothing has been written)");
    // from here on nothing is refused
    std::vector<int32_t> seg_of((size_t)n, -1);
    auto device_seg = [&](int64_t i) -> int32_t {
      if (offs[i + 1] == offs[i]) return -1;
      if (seg_of[(size_t)i] < 0) {
        seg_of[(size_t)i] = (int32_t)segs.size();
        segs.push_back(SyncSeg{offs[i], offs[i + 1] - offs[i], units, units_of(i)});
        units += units_of(i);
      }
      return seg_of[(size_t)i];
    };
    int64_t pred_first = 0;
    for (int64_t p = 0; p < a.n_pairs; ++p) {
      const int64_t N = units_of(a.pairs[p].a), M = units_of(a.pairs[p].b);
      a.summaries[p] = bp_sync_summary{2, (int32_t)N, (int32_t)M, 0, entries, 0};  // (no rows on either side: no path)
      if (N == 0 && M == 0) continue;
      pairs.push_back(SyncPair{device_seg(a.pairs[p].a), device_seg(a.pairs[p].b), pred_first, entries});
      pair_of.push_back(p);
      if (N > 0 && M > 0) pred_first += sync_pred_bytes(variant, N, M), entries += N + M - 1;
    }
    *queued = !pairs.empty();
    return BP_OK;
  }

  // the tables, the launches, and the summaries and the path on their way home (one page-locked block: the summaries, then
  // the path)
  int queue(bp_handle h, const Maps& all, int64_t, const int64_t*) override {
    hipStream_t s = h->stream;
    const int64_t nd = (int64_t)pairs.size(), ns = (int64_t)segs.size();
    static_assert(sizeof(SyncParams) == sizeof(bp_sync_params) && sizeof(bp_sync_params) == 32, "the parameters go to the device as they are");
    static_assert(sizeof(SyncSummary) == sizeof(bp_sync_summary) && sizeof(bp_sync_summary) == 32, "the summaries come home as they are");
    const size_t n_home = (size_t)(4 * nd + entries);  // in int64: 32 bytes a summary, 8 a path entry
    BP_HIP(h->sy_segs.reserve((size_t)ns));
    BP_HIP(h->sy_pairs.reserve((size_t)nd));
    BP_HIP(h->sy_nan.reserve((size_t)ns));
    BP_HIP(h->sy_feat.reserve((size_t)units));
    BP_HIP(h->sy_pred.reserve((size_t)std::max<int64_t>(16, pred_bytes)));
    BP_HIP(h->sy_walk.reserve((size_t)std::max<int64_t>(1, entries)));
    BP_HIP(h->sy_out.reserve(n_home));
    BP_HIP(h->sy_home.reserve(n_home));
    BP_HIP(hipMemcpyAsync(h->sy_segs, segs.data(), (size_t)ns * sizeof(SyncSeg), hipMemcpyHostToDevice, s));
    BP_HIP(hipMemcpyAsync(h->sy_pairs, pairs.data(), (size_t)nd * sizeof(SyncPair), hipMemcpyHostToDevice, s));
    SyncParams prm;
    std::memcpy(&prm, a.params, sizeof(prm));
    int64_t* out = h->sy_out;
    BP_HIP(launch_sync(all.note, prm, h->sy_segs, ns, units, h->sy_pairs, nd, max_n, max_m, h->sy_nan, static_cast<uint4*>(h->sy_feat),
                       h->sy_pred, h->sy_walk, reinterpret_cast<int32_t*>(out + 4 * nd), reinterpret_cast<SyncSummary*>(out), s));
    BP_HIP(hipMemcpyAsync(h->sy_home, out, n_home * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return BP_OK;
  }

  // the summaries and the path are in the page-locked block; the regions of the pairs with a path tile the entries, so the
  // path leaves as one run
  int home(bp_handle h, const char*, int64_t, const int64_t*) override {
    const int64_t nd = (int64_t)pairs.size();
    const int64_t* block = h->sy_home;
    for (int64_t c = 0; c < nd; ++c) std::memcpy(&a.summaries[pair_of[(size_t)c]], block + 4 * c, sizeof(bp_sync_summary));
    if (entries) std::memcpy(a.path, block + 4 * nd, (size_t)entries * 8);
    return BP_OK;
  }
};

}  // namespace

extern "C" {

int bp_sync_from_maps(bp_handle h, int64_t n_segments, const int64_t* row_offsets, const float* note, int mem_kind, int64_t n_pairs,
                      const bp_sync_pair* pairs, const bp_sync_params* p, bp_sync_summary* summaries, int32_t* path, int64_t max_path) {
  SyncSink sink({n_pairs, pairs, p, summaries, path, max_path});
  return run_clips(h, "bp_sync_from_maps", given_maps(n_segments, row_offsets, note, nullptr, nullptr, mem_kind), sink);
}

int bp_infer_clips_sync(bp_handle h, int64_t n_clips, const bp_clip* clips, int sample_rate, int pcm_mem_kind, int64_t n_pairs,
                        const bp_sync_pair* pairs, const bp_sync_params* p, bp_sync_summary* summaries, int32_t* path, int64_t max_path) {
  SyncSink sink({n_pairs, pairs, p, summaries, path, max_path});
  return run_clips(h, "bp_infer_clips_sync", pcm_clips(n_clips, clips, sample_rate, pcm_mem_kind), sink);
}

}  // extern "C"
