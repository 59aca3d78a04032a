// The decodes of a sweep scored frame by frame where their events lie (bp_note_events_sweep_frame_score,
// include/basic_pitch_amd_frame_score.h): one launch behind the tracker's (note_track.hip), beside the
// note-matching launch (note_score.hip) or in its place.  ONE WORKGROUP PER DECODE: it reads the decode's count and NtEvent
// records from its region of the pool, the rows of its segment and the refs of its segment, and leaves 40 bytes of counts and
// a status.
//
// Frames are taken in chunks of at most kNoteFramesChunk.  Step 1 rolls the events into LDS, a mask of 88 bits (3 words) per
// frame: a wave takes an event, its lanes the event's frames, each an LDS atomic OR — two events of different pitch share a
// frame's words.  Step 2: a lane takes a frame, its mask in registers, and walks the refs of the segment, which the host has
// put IN ASCENDING PITCH and reduced to integers (the frames a ref sounds on, the note bins it hits: note_frames_host.cpp):
// a ref that sounds takes the lowest set bit at or above max(lo, the bit after the one taken last) if that is <= hi.  The
// bins a ref hits being one run whose ends both rise with the pitch, the bits taken rise too, so "free" is "above the last
// one taken" and no bit needs clearing; this is the greedy the header allows, a maximum matching.  The ref walked is the
// same for all lanes: scalar loads.  A ref that sounds on no frame of the chunk is skipped for the whole wave.  Step 3: the
// lanes' 64-bit sums of n_ref, n_est (popcount), tp and min(n_ref, n_est) - tp go through wave shuffles and one LDS step.
//
// Nothing here is floating point: bit-equality with the host checker is structural.  No indexed register array (the mask is
// three named words; the search for a bit at or above a bound is two shifts and two count-trailing-zeros), no recursion: no
// scratch.
//
// Width: 256 lanes.  Unlike the note matcher's serial search (one wave) the frames are independent and the
// ref walk per frame is the long, serial part, so lanes should cover frames: a one-window decode has 172 frames, which three
// of the four waves take in ONE pass (64 lanes would walk the refs three times over, 128 twice), and in step 1 its few tens
// of events are 4 waves x a handful of rounds.  512 would leave five waves of eight idle on such a decode and halve the
// workgroups a compute unit holds.  LDS per launch is 12 bytes x the frames of the job's longest decode, at most one chunk
// (24 KiB): 2 KiB for one-window jobs, so a compute unit is limited by its wave slots (8 workgroups), not by LDS.
#include "bp_kernels.h"

namespace bp {

namespace {

constexpr int kWidth = 256, kWaves = kWidth / 64;

struct NfEvent {  // note_track.hip NtEvent
  int start, end, pitch;
  float amp;
};

// the lowest set bit of the 88-bit mask (lo64: bins 0 ... 63, hi32: bins 64 ... 87) at or above b (0 ... 88); none: 1000
__device__ __forceinline__ int nf_lowest_from(unsigned long long lo64, uint32_t hi32, int b) {
  if (b < 64) {
    const unsigned long long x = lo64 & (~0ull << b);
    if (x) return __builtin_ctzll(x);
    b = 64;
  }
  const uint32_t y = hi32 & (~0u << (b - 64));  // (b - 64 <= 24)
  return y ? 64 + __builtin_ctz(y) : 1000;
}

// the workgroup's sums of four values, in every lane
__device__ __forceinline__ void nf_block_sum(unsigned long long (&v)[4], unsigned long long (*part)[4], int tid) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
  __syncthreads();  // part is no longer read
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) part[tid >> 6][k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = part[0][k];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v[k] += part[w][k];
  }
}

// chunk: the frames the launch's LDS has room for (3 words each)
__global__ __launch_bounds__(kWidth) void nf_frames_kernel(const int4* __restrict__ counts, const int64_t* __restrict__ rows,
                                                           const int64_t* __restrict__ ev_first, const NfEvent* __restrict__ ev_pool,
                                                           const NoteScoreDecode* __restrict__ dec, const NoteFrameRef* __restrict__ all_refs,
                                                           int64_t n, int chunk, int64_t* __restrict__ out) {
  extern __shared__ uint32_t s_roll[];
  __shared__ unsigned long long s_part[kWaves][4];
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const NoteScoreDecode d = dec[c];
  const int4 cnt = counts[c];
  const int ne = cnt.x, nr = d.n_ref;
  const int64_t T = rows[c + 1] - rows[c];
  int status = cnt.z;
  const NfEvent* ev = ev_pool + ev_first[c];
  // the status is launch_note_score's (note_score.hip): the frames the decode's bends would take against their room, the bound
  if (status == 0 && d.bend_room >= 0) {
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int i = tid; i < ne; i += kWidth) v[0] += (unsigned long long)(ev[i].end - ev[i].start);
    nf_block_sum(v, s_part, tid);
    if ((long long)v[0] > d.bend_room) status = 2;
  }
  if (status == 0 && (ne > kNoteScoreMaxNotes || nr > kNoteScoreMaxNotes)) status = 3;
  int64_t* score = out + 5 * c;
  int32_t* status_out = reinterpret_cast<int32_t*>(out + 5 * n) + c;
  if (status != 0) {
    if (tid == 0) score[0] = T, score[1] = 0, score[2] = 0, score[3] = 0, score[4] = 0, *status_out = status;
    return;
  }
  const NoteFrameRef* refs = all_refs + d.ref_first;
  unsigned long long sum[4] = {0, 0, 0, 0};  // n_ref, n_est, tp, min(n_ref, n_est) - tp
  for (int64_t base = 0; base < T; base += chunk) {
    const int len = (int)(T - base < chunk ? T - base : chunk);
    for (int w = tid; w < 3 * len; w += kWidth) s_roll[w] = 0;
    __syncthreads();
    for (int i = wave; i < ne; i += kWaves) {
      const NfEvent e = ev[i];
      const int bin = e.pitch - 21;
      if (bin < 0 || bin > 87) continue;  // (the tracker's pitches are 21 + a note bin)
      const int a = (int)((e.start > base ? e.start : base) - base);
      const int b = (int)((e.end < base + len ? e.end : base + len) - base);
      for (int f = a + lane; f < b; f += 64) atomicOr(&s_roll[3 * f + (bin >> 5)], 1u << (bin & 31));
    }
    __syncthreads();
    const int first = (int)base;  // (rows fit 32 bits: BP_SWEEP_MAX_ROWS)
    for (int f = tid; f < len; f += kWidth) {
      const int fr = first + f;
      const uint32_t m0 = s_roll[3 * f], m1 = s_roll[3 * f + 1], m2 = s_roll[3 * f + 2];
      const unsigned long long lo64 = (unsigned long long)m0 | ((unsigned long long)m1 << 32);
      const int n_est = __popc(m0) + __popc(m1) + __popc(m2);
      int n_ref = 0, tp = 0, bound = 0;
      for (int j = 0; j < nr; ++j) {
        const NoteFrameRef r = refs[j];
        if (r.f1 <= first || r.f0 >= first + len) continue;  // sounds nowhere in the chunk: the same for every lane
        if (fr < r.f0 || fr >= r.f1) continue;
        ++n_ref;
        const int pick = nf_lowest_from(lo64, m2, bound > r.lo ? bound : r.lo);
        if (pick <= r.hi) ++tp, bound = pick + 1;
      }
      sum[0] += (unsigned)n_ref, sum[1] += (unsigned)n_est, sum[2] += (unsigned)tp;
      sum[3] += (unsigned)((n_ref < n_est ? n_ref : n_est) - tp);
    }
    __syncthreads();  // the roll is read: the next chunk may zero it
  }
  nf_block_sum(sum, s_part, tid);
  if (tid == 0)
    score[0] = T, score[1] = (int64_t)sum[0], score[2] = (int64_t)sum[1], score[3] = (int64_t)sum[2], score[4] = (int64_t)sum[3],
    *status_out = 0;
}

}  // namespace

size_t note_frames_lds_bytes(int64_t max_rows) {
  const int64_t frames = max_rows < 1 ? 1 : (max_rows < kNoteFramesChunk ? max_rows : kNoteFramesChunk);
  return (size_t)frames * 3 * sizeof(uint32_t);
}

hipError_t launch_note_frames(const void* counts, const int64_t* rows, const int64_t* ev_first, const void* ev_pool,
                              const NoteScoreDecode* dec, const NoteFrameRef* refs, int64_t n_decodes, int64_t max_rows, int64_t* out,
                              hipStream_t s) {
  if (n_decodes <= 0) return hipSuccess;
  const size_t lds = note_frames_lds_bytes(max_rows);
  hipLaunchKernelGGL(nf_frames_kernel, dim3((unsigned)n_decodes), dim3(kWidth), lds, s, static_cast<const int4*>(counts), rows, ev_first,
                     static_cast<const NfEvent*>(ev_pool), dec, refs, n_decodes, (int)(lds / (3 * sizeof(uint32_t))), out);
  return hipGetLastError();
}

}  // namespace bp
