// The decodes of a sweep scored against reference notes where their events lie (bp_note_events_sweep_score,
// include/basic_pitch_amd_score.h): the launch behind the tracker's (note_track.hip) in place of its offsets and
// pack launches.  ONE WORKGROUP OF ONE WAVE PER DECODE: it reads the decode's count and NtEvent records from its region of the
// pool and the refs of its segment, and leaves 16 bytes of counts and a status.
//
// The counts are the sizes of two maximum bipartite matchings (events x refs; "onset and pitch hit", then "onset, pitch and
// offset hit"), found by augmenting paths (Kuhn): from every event in turn, a depth-first search for a free ref over
// alternating paths, each ref visited once per search.  Every decision is wave-uniform; the wide part is the scan — for the
// event at the head of the path the 64 lanes test 64 refs per ballot, the hit predicate evaluated on the fly (no adjacency in
// memory), and the ballot selects the first hit not yet visited.  A search that returns to an event goes on behind the ref
// it took there.  The host checker (note_score_host.cpp) searches over adjacency lists; a maximum matching's size is unique.
//
// State in dynamic LDS, sized per launch from the job's largest decode: per ref the event that holds it (16 bits, kNone:
// free), the visited bitmap, and the explicit path — per level the event and the ref it took (16 bits each).  The event ->
// ref direction is not kept: a search starts from each event once, while it is unmatched, and never asks for an event's
// partner.  No device recursion, no indexed register array: no scratch.
//
// Bit-equality with the host.  The estimated times are bp_internal_frame_time's expression (note_decode.cpp) on the event's
// frames, the predicates the header's, all in float64; `#pragma clang fp contract(off) reassociate(off)` keeps the compiler
// from fusing or reordering (the frame time's `a - b * c` would otherwise become one fma), float64 division is correctly
// rounded, rint and floor are exact.  A ref's offset tolerance, which depends on the ref alone, comes with the table.
#include "bp_kernels.h"

#pragma clang fp contract(off)
#pragma clang fp reassociate(off)

namespace bp {

namespace {

constexpr uint32_t kNone = 0xffffu;
static_assert(kNoteScoreMaxNotes < (int)kNone, "an index fits 16 bits beside the free mark");
// 2 bytes of_ref + 1 bit seen per ref, 2 + 2 bytes per level of the path (include/basic_pitch_amd_score.h: BP_SCORE_MAX_NOTES)
static_assert(kNoteScoreMaxNotes * 2 + kNoteScoreMaxNotes / 8 + (kNoteScoreMaxNotes + 1) * 4 + 64 <= 160 * 1024, "LDS budget per workgroup");

struct NsEvent {  // note_track.hip NtEvent
  int start, end, pitch;
  float amp;
};

// model_frames_to_time()[fr]: note_decode.cpp bp_internal_frame_time, the same operations in the same order
__device__ __forceinline__ double ns_frame_time(int64_t fr) {
  const double window_offset = (256.0 / 22050.0) * (172.0 - (43844.0 / 256.0)) + 0.0018;
  const double original = (double)(fr * 256) / 22050.0;
  const double window_number = floor((double)fr / 172.0);
  return original - (window_offset * window_number);
}

__device__ __forceinline__ bool ns_within(double d, double tol, int strict) { return strict ? d < tol : d <= tol; }
__device__ __forceinline__ double ns_round6(double x) { return rint(x * 1e6) / 1e6; }

// the first ref j >= from, not yet seen, that the event (start, end, pitch) hits; -1: none.  Wave-uniform.
__device__ __forceinline__ int ns_scan(const NoteScoreRef* __restrict__ refs, int nr, const uint32_t* seen, int from, double start,
                                       double end, double pitch, const NoteScoreParams& p, bool with_offset, int lane) {
  for (int base = from & ~63; base < nr; base += 64) {
    const int j = base + lane;
    bool hit = false;
    if (j >= from && j < nr && !((seen[j >> 5] >> (j & 31)) & 1u)) {
      const NoteScoreRef r = refs[j];
      hit = ns_within(ns_round6(fabs(r.start_s - start)), p.onset_tol, p.strict) &&
            ns_within(100.0 * fabs(r.pitch_midi - pitch), p.pitch_tol, p.strict);
      if (hit && with_offset) hit = ns_within(ns_round6(fabs(r.end_s - end)), r.offset_tol, p.strict);
    }
    const unsigned long long m = __ballot(hit);
    if (m) return base + __builtin_ctzll(m);
  }
  return -1;
}

// max_refs, max_depth: what the launch's LDS has room for — every decode it scores has at most max_refs refs, and
// min(events, refs + 1) <= max_depth
__global__ __launch_bounds__(64) void ns_score_kernel(const int4* __restrict__ counts, const int64_t* __restrict__ ev_first,
                                                      const NsEvent* __restrict__ ev_pool, const NoteScoreDecode* __restrict__ dec,
                                                      const NoteScoreRef* __restrict__ all_refs, NoteScoreParams p, int64_t n,
                                                      int max_refs, int max_depth, int32_t* __restrict__ out) {
  extern __shared__ uint32_t s_score[];
  const int64_t c = blockIdx.x;
  const int lane = threadIdx.x;
  const NoteScoreDecode d = dec[c];
  const int4 cnt = counts[c];
  const int ne = cnt.x, nr = d.n_ref;
  int status = cnt.z;
  const NsEvent* ev = ev_pool + ev_first[c];
  if (status == 0 && d.bend_room >= 0) {  // the frames the decode's bends would take, against the room the sweep calls give them
    long long frames = 0;
    for (int i = lane; i < ne; i += 64) frames += ev[i].end - ev[i].start;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) frames += __shfl_xor(frames, o);
    if (frames > d.bend_room) status = 2;
  }
  if (status == 0 && (ne > kNoteScoreMaxNotes || nr > kNoteScoreMaxNotes || nr > max_refs || (ne < nr + 1 ? ne : nr + 1) > max_depth))
    status = 3;  // (the last two never hold for a launch sized as launch_note_score is told to: nothing is written past LDS)
  int4* score = reinterpret_cast<int4*>(out) + c;
  int32_t* status_out = out + 4 * n + c;
  if (status != 0) {
    if (lane == 0) *score = make_int4(nr, 0, 0, 0), *status_out = status;
    return;
  }
  // LDS: the bitmap (words), the refs' holders (16 bits each), the path's events and refs
  const int words = (max_refs + 31) >> 5;
  uint32_t* seen = s_score;
  uint16_t* of_ref = reinterpret_cast<uint16_t*>(seen + words);
  uint16_t* path_e = of_ref + ((max_refs + 1) & ~1);
  uint16_t* path_r = path_e + ((max_depth + 1) & ~1);
  const NoteScoreRef* refs = all_refs + d.ref_first;
  const int nr_words = (nr + 31) >> 5;

  int matched_onset = 0, matched_offset = 0;
#pragma unroll 1  // one copy of the search
  for (int pass = 0; pass < 2; ++pass) {
    const bool with_offset = pass == 1;
    int size = 0;
    for (int j = lane; j < nr; j += 64) of_ref[j] = (uint16_t)kNone;
    for (int root = 0; root < ne && nr > 0; ++root) {
      __syncthreads();  // the holders of the search before (or the initial ones) are written, its bitmap no longer read
      for (int w = lane; w < nr_words; w += 64) seen[w] = 0;
      __syncthreads();
      int sp = 0, cur = root, from = 0;
      for (;;) {
        const NsEvent e = ev[cur];
        const int r = ns_scan(refs, nr, seen, from, ns_frame_time(e.start), ns_frame_time(e.end), (double)e.pitch, p, with_offset, lane);
        if (r < 0) {  // a dead end: back to the event before, which goes on behind the ref it took
          if (sp == 0) break;
          --sp;
          cur = __builtin_amdgcn_readfirstlane((int)path_e[sp]);
          from = __builtin_amdgcn_readfirstlane((int)path_r[sp]) + 1;
          continue;
        }
        if (lane == 0) {
          seen[r >> 5] |= 1u << (r & 31);
          path_e[sp] = (uint16_t)cur, path_r[sp] = (uint16_t)r;
        }
        __syncthreads();
        const uint32_t held_by = __builtin_amdgcn_readfirstlane((uint32_t)of_ref[r]);
        if (held_by == kNone) {  // a free ref: every event of the path takes the ref it chose (distinct refs: no two lanes collide)
          for (int i = lane; i <= sp; i += 64) of_ref[path_r[i]] = path_e[i];
          ++size;
          break;
        }
        ++sp, cur = (int)held_by, from = 0;
      }
    }
    if (with_offset) matched_offset = size; else matched_onset = size;
    __syncthreads();
  }
  if (lane == 0) *score = make_int4(nr, ne, matched_onset, matched_offset), *status_out = 0;
}

}  // namespace

size_t note_score_lds_bytes(int max_refs, int max_depth) {
  return (size_t)((max_refs + 31) >> 5) * 4 + (size_t)((max_refs + 1) & ~1) * 2 + (size_t)((max_depth + 1) & ~1) * 4;
}

hipError_t launch_note_score(const void* counts, const int64_t* ev_first, const void* ev_pool, const NoteScoreDecode* dec,
                             const NoteScoreRef* refs, const NoteScoreParams& prm, int64_t n_decodes, int max_refs, int max_depth,
                             int32_t* out, hipStream_t s) {
  if (n_decodes <= 0) return hipSuccess;
  const size_t lds = note_score_lds_bytes(max_refs, max_depth);
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ns_score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ns_score_kernel, dim3((unsigned)n_decodes), dim3(64), lds, s, static_cast<const int4*>(counts), ev_first,
                     static_cast<const NsEvent*>(ev_pool), dec, refs, prm, n_decodes, max_refs, max_depth, out);
  return hipGetLastError();
}

}  // namespace bp
