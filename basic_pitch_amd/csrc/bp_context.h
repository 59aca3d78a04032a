// Private to csrc: the handle (struct bp_context) and what bp_api.hip, track_api.hip, the clip jobs (clips_api.hip and the sinks'
// clips_*.hip, which share clips_job.h beside this header), stream_api.hip and
// weight_pack.hip share of it — the HIP error macro, the chunk / wait helpers (defined in bp_api.hip), the maps, filter,
// argument and candidates helpers of the track calls, the clip jobs and the streaming sessions (defined in track_api.hip), and
// the tracker's host half (defined in clips_api.hip).  The handle's memory is owned by the buffers of device_buffer.h:
// deleting the handle frees it.
#pragma once
#include "../../include/basic_pitch_amd.h"
#include "../../include/basic_pitch_amd_adpcm.h"

#include <cstdio>
#include <string>
#include <vector>

#include "bp_kernels.h"

struct bp_context {
  int device = 0;
  unsigned flags = 0;
  int n_cu = 256;
  char arch[32] = {0};
  hipStream_t own_stream = nullptr, stream = nullptr;
  hipEvent_t done = nullptr;  // BP_FLAG_BLOCKING_WAIT: the event a waiting host thread sleeps on
  int64_t cap = 0;
  int64_t workspace_bytes = 0;
  std::string err;

  // window geometry: the reference's 22.05 kHz model, or the extended 44.1 kHz range (BP_FLAG_EXT_CQT_44K)
  bool ext = false;
  int win_len = bp::kAudioN, hop = BP_HOP_SIZE, lead = BP_OVERLAP_LEN / 2, n_bins = bp::kBins, rate = BP_AUDIO_SAMPLE_RATE;
  int64_t pyr_stride = bp::kPyrStride;

  bp::LogConsts kc{};
  float b_contour2 = 0, b_note2 = 0, b_onset2 = 0;
  // Every allocation of the handle is a buffer that frees itself (device_buffer.h).  The operand tables weight_pack.hip
  // packs are raw bytes (PackedWeights::tables names them by member pointer): f16 fragments go to the launchers as they
  // are, fp32 tables through as<float>().
  using Table = bp::DeviceBuffer<uint8_t>;
  template <class T>
  using Buffer = bp::DeviceBuffer<T>;
  // device constants
  Table d_lowpass, d_sqrt_len, d_fb_bfrag;
  Table d_pl_bin_k;  // cqt_planes_filterbank.hip: per-bin eps / s^2, s = sqrt(len) 2^-12
  // fused branches (conv_branch.hip): f16 hi/lo A fragments + {bias1[32], extra[9], bias2}
  Table d_note_wfrag, d_note_w16, d_note_wf32, d_onset_wfrag, d_onset_wf32, d_onset_w16;
  Buffer<uint32_t> zp;  // [cap][kZRowsP][kZRow] pre-split z, zero padded (bp_common.h)
  // contour branch: conv1 A fragments (interior march, round-2 folded, rim GEMM, rim march), bias[8], conv2 taps [5][5][8]
  Table d_d1_wfold, d_d1_wmarch, d_d1_wrim, d_d1_wrimm, d_d1_bias, d_d2_w, d_d2_wproj;
  int resample_mode = 0;  // BP_RESAMPLE=plain|tiled: 1 | 2 (A/B runs of the resampling kernels)
  Buffer<float> c1s;  // [cap][172][kC1Row][8] relu(conv1); pad bins zeroed once at allocation
  // cqt_planes.h: decimator / filterbank fragments (f16 hi / lo), the planes of a chunk [cap][2][stride] f16
  Table d_pl_tfrag, d_pl_bfrag;
  Buffer<uint16_t> planes;
  Table d_c1_bfrag, d_c1_bias, d_o1_bfrag, d_o1_bias;
  Table d_n1_bfrag, d_n1_bias, d_w_contour2, d_w_note2, d_w_onset2;
  // workspace (per chunk of `cap` windows)
  Buffer<float> audio, pyr, lp, c1, contour, n1, note, o1, onset;
  Buffer<int> mm;
  Buffer<float> fb_scratch;  // filterbank partial extrema (grow-only; >= cap windows)
  // track path staging (grow-only)
  Buffer<float> track;
  // audio ingest (audio_ingest.hip): staging for PCM (bytes) / mono / 22.05 kHz signal (grow-only), cached filter
  Buffer<uint8_t> pcm_dev;
  Buffer<float> mono_dev, res_dev;
  Buffer<double> taps_dev;
  int taps_rate = 0;
  bp::ResamplePlan plan{};
  Buffer<float> track_out;  // [T, 88+88+264] staging when outputs are host pointers
  int64_t maps_rows = 0;    // rows of the maps a *_candidates call left in track_out (bp_track_maps); 0: none
  // device-side note candidates (note_device.hip): bitmap [T][11] + bend map [T][88], the bend tables with the stats record
  Buffer<uint8_t> nd_buf;
  Table nd_tables;                     // [88] int4 windows, [51] double Gaussian, then the stats record
  bp::FlacDeviceBuffers fd;            // flac_device.hip: the file's bytes, the frame lists, the scratch rows
  bp::PinnedBuffer<int> fd_status_host;  // the device decoder's error bits of the last call
  bp::AdpcmDeviceBuffers ad;           // adpcm_device.hip: the files' bytes, their int16 samples, the segment table (grow-only)
  bp::PinnedBuffer<int> nd_stats_host;   // copy of the stats record (4 words; [1]: a NaN was seen)
  void* nd_stats_host_dev = nullptr;  // the same buffer as the device sees it
  bool nd_stats_ready = false;     // the device record holds its initial values (the export kernel leaves it so)
  // many clips in one call (bp_infer_clips_candidates, clips_api.hip), all grow-only: the table of clips, the clips' row
  // offsets, one stats record of 16 bytes per clip and the page-locked copy of the records (4 words per clip)
  Buffer<bp::ClipDesc> clip_tab;
  Buffer<int64_t> clip_rows;
  Table clip_stats;
  bp::PinnedBuffer<int> clip_stats_host;
  int64_t clip_stats_ready = 0;  // the first so many device records hold their initial values (the export kernel leaves them so)
  // note events of many clips (bp_infer_clips_events, note_track.hip), all grow-only and scratch of one call: the first event
  // record of each clip's region, the pool of regions (16-byte event records; bends, a byte each), the working state of the
  // clips too long for LDS, per clip its counts and status, the packed events and bends with the offsets that go home first
  // (ev_meta), and the page-locked block both copies land in
  Buffer<int64_t> ev_first, ev_meta;
  Table ev_pool, ev_counts, ev_out;
  Buffer<int8_t> bd_pool, bd_out;
  Buffer<float> ev_scratch;
  Table ev_seg;  // bp_streams_events: the table of the segments' own parameters (NoteTrackSeg)
  bp::PinnedBuffer<int64_t> ev_home;
  // a sweep (bp_note_events_sweep, clips_sweep.hip SweepSink::queue), all grow-only, scratch of one call and grown by sweeps alone: the
  // note rows constrained per band [bands][T][88], the working copy of the onset rows [T][88], per dense key the bitmap
  // [keys][T][12] and the stats records [keys][segments], the decode table (NoteSweepDecode) with the rows and the event
  // records before each decode behind it
  Buffer<float> sw_note, sw_onset;
  Buffer<uint8_t> sw_bits;
  Table sw_stats, sw_tab;
  // a scored sweep (bp_note_events_sweep_score, clips_sweep.hip SweepSink::queue), all grow-only, scratch of one call and grown by the
  // score calls alone: the refs of all segments, per decode which of them are its segment's, the scores [decodes][4] with the
  // statuses [decodes] behind them, and the page-locked block they come home in
  Buffer<bp::NoteScoreRef> sc_refs;
  Buffer<bp::NoteScoreDecode> sc_dec;
  Buffer<int32_t> sc_out;
  bp::PinnedBuffer<int32_t> sc_home;
  // the frame level of a scored sweep (bp_note_events_sweep_frame_score, clips_sweep.hip SweepSink::queue), all grow-only, scratch of
  // one call and grown by the frame-score calls alone: per segment its refs in pitch order as frames and note bins, the counts
  // [decodes][5] with the statuses [decodes] (32-bit) behind them, and the page-locked block they come home in
  Buffer<bp::NoteFrameRef> fs_refs;
  Buffer<int64_t> fs_out;
  bp::PinnedBuffer<int64_t> fs_home;
  // multi-pitch estimates (bp_multipitch_from_maps and its kin, clips_multipitch.hip), all grow-only, scratch of one call and grown
  // by those calls alone: the device copy of a contour map given in host memory, per row its peak count and segment, the
  // points before each row, per segment the not-finite flag, the point offsets with the statuses behind them, the points; of a
  // scored sweep the sets, the decode table, the refs in pitch order and the counts [decodes][5] with the statuses (32-bit)
  // behind them; and the page-locked block offsets or counts come home in
  Buffer<float> mp_contour;
  Buffer<int2> mp_rows;
  Buffer<int64_t> mp_first, mp_meta, mp_out;
  Buffer<int32_t> mp_bad;
  Table mp_points;
  Buffer<bp::MpParams> mp_sets;
  Buffer<bp::MpDecode> mp_dec;
  Buffer<bp::MpRef> mp_refs;
  bp::PinnedBuffer<int64_t> mp_home;
  // the melody (bp_melody_from_maps and its kin, clips_melody.hip), all grow-only, scratch of one call and grown by those calls
  // alone: the device copy of a contour map given in host memory, the sets, the decode table, the predecessors (one byte per
  // state per row of every decode, bp::kMelodyPredStride bytes a row: the one large pool, 2.3 GB at BP_SWEEP_MAX_ROWS), the
  // records, a scored sweep's reference track, the counts [decodes][6] with the statuses (32-bit) behind them, and the
  // page-locked block they come home in
  Buffer<float> mel_contour;
  Buffer<bp::MelodyParams> mel_sets;
  Buffer<bp::MelodyDecode> mel_dec;
  Table mel_pred, mel_points;
  Buffer<double> mel_ref;
  Buffer<int64_t> mel_out;
  bp::PinnedBuffer<int64_t> mel_home;
  // forced alignment (bp_align_from_maps, bp_infer_clips_align, clips_align.hip), all grow-only, scratch of one call and grown by
  // those calls alone: the device copies of note and onset maps given in host memory (or not 16-byte aligned), the states, the
  // segment table, the gains (8 bytes a cell: the one large pool, 2 GiB at BP_ALIGN_MAX_CELLS), the predecessor bits (a bit a
  // cell in whole 64-bit words a row), the NaN flags, the first frames, the totals [segments] with the statuses (32-bit) behind
  // them, and the page-locked block those come home in
  Buffer<float> al_note, al_onset;
  Buffer<bp::AlignState> al_states;
  Buffer<bp::AlignSeg> al_segs;
  Table al_gains;
  Buffer<uint64_t> al_pred;
  Buffer<uint32_t> al_nan;
  Buffer<int32_t> al_first;
  Buffer<int64_t> al_out;
  bp::PinnedBuffer<int64_t> al_home;
  // tempo and beats (bp_beats_from_maps, bp_infer_clips_beats, clips_beat.hip), all grow-only, scratch of one call and grown by
  // those calls alone: the device copy of an onset map given in host memory (or not 16-byte aligned), the parameters with their
  // prior table, the segment table, the strength of every row, per segment bp::kBeatAccStride sums (sum o, sum o^2, the NaN
  // flag, the autocorrelation per lag, the path kernel's clock readings), the predecessors (one uint16 a row: 16 MiB at
  // BP_SWEEP_MAX_ROWS), the summaries [segments] with the beat pool (32-bit) behind them, and the page-locked block those come
  // home in
  Buffer<float> bt_onset;
  Buffer<bp::BeatParams> bt_params;
  Buffer<bp::BeatSeg> bt_segs;
  Buffer<int32_t> bt_strength;
  Buffer<int64_t> bt_acc;
  Buffer<uint16_t> bt_pred;
  Buffer<int64_t> bt_out;
  bp::PinnedBuffer<int64_t> bt_home;
  // chords and key (bp_chords_from_maps, bp_infer_clips_chords, clips_chord.hip), all grow-only, scratch of one call and grown
  // by those calls alone: the device copy of a note map given in host memory (or not 16-byte aligned), the parameters with
  // their tables, the segment table, the boundaries of all segments, the chroma (32 bytes a row), the pooled sums (64 bytes
  // a unit of a segment with boundaries), per segment bp::kChordAccStride sums, the records (16 bytes a unit: 128 MiB at
  // BP_SWEEP_MAX_ROWS), a label a unit, the summaries [segments] with the labels (a byte a row) behind them, and the
  // page-locked block those come home in
  Buffer<float> ch_note;
  Buffer<bp::ChordParams> ch_params;
  Buffer<bp::ChordSeg> ch_segs;
  Buffer<int32_t> ch_bounds;
  Buffer<uint16_t> ch_chroma;
  Buffer<uint32_t> ch_pool;
  Buffer<int64_t> ch_acc;
  Buffer<uint4> ch_records;
  Buffer<uint8_t> ch_unit_labels;
  Buffer<int64_t> ch_out;
  bp::PinnedBuffer<int64_t> ch_home;
  // two recordings against each other (bp_sync_from_maps, bp_infer_clips_sync, clips_sync.hip), all grow-only, scratch of one
  // call and grown by those calls alone: the device copy of a note map given in host memory, the tables of the segments that
  // a pair names and of the pairs, a NaN flag a segment, the features (16 bytes a unit), the predecessors in the skewed order
  // of the recurrence (at most bp::kSyncMaxPredBytes), the walked path (4 bytes an entry), the summaries [pairs] with the
  // path (8 bytes an entry) behind them, and the page-locked block those come home in
  Buffer<float> sy_note;
  Buffer<bp::SyncSeg> sy_segs;
  Buffer<bp::SyncPair> sy_pairs;
  Buffer<uint32_t> sy_nan;
  Buffer<uint4> sy_feat;
  Buffer<uint8_t> sy_pred;
  Buffer<uint32_t> sy_walk;
  Buffer<int64_t> sy_out;
  bp::PinnedBuffer<int64_t> sy_home;
  // streaming sessions (stream_api.hip).  Scratch of one step (grow-only; nothing of a stream survives a call in them):
  // the PCM of the step's chunks, their mono form, the rows on their way to host buffers, the step's window segments.  The
  // streams' own state is theirs.  The filters are kept per input rate: streams of one rate share a table.
  Buffer<uint8_t> st_pcm;
  Buffer<float> st_mono, st_out;
  Buffer<bp::WindowSeg> st_segs;
  struct StreamTaps {
    int rate;
    Buffer<double> dev;
    bp::ResamplePlan plan;
  };
  std::vector<StreamTaps> st_taps;
  // the updates of many streams in one step (bp_streams_candidates), all grow-only and scratch of one call: the table of
  // streams with its prefix arrays, the packed note rows, bends and bitmaps on their way home, one stats record of 16 bytes per
  // stream and the page-locked copy of the records (4 words per stream)
  Table up_tab;
  Buffer<float> up_note;
  Buffer<int8_t> up_bend;
  Buffer<uint8_t> up_bits;
  Table up_stats;
  bp::PinnedBuffer<int> up_stats_host;

  // stage timing: a ring of event sets, one per chunk, averaged by bp_get_stage_ms
  static constexpr int kTimedRing = 128;
  static constexpr int kDomEvery = 4;
  static constexpr int kMaxMarks = 32;  // intervals per chunk (bp_get_stage_ms sums those of a stage)
  hipEvent_t ev[kTimedRing][kMaxMarks + 1] = {};
  // per ring slot (the mark sequence depends on the chunk: zpack only below half a window per CU):
  // stage id of the interval between ev[c][i] and ev[c][i+1]; -1: not a stage (skipped)
  int seq[kTimedRing][kMaxMarks] = {};
  int n_seq[kTimedRing] = {};
  int64_t timed_chunks = 0;  // chunks recorded since the last bp_get_stage_ms
  int64_t dom_chunks = 0;    // chunks seen in BP_FLAG_TIME_DOMINANT mode (every kDomEvery-th is recorded)

  // what is not memory; the buffers free themselves after it.  The handle's device is current (bp_destroy, bp_create).
  ~bp_context() {
    for (auto& row : ev)
      for (auto& e : row)
        if (e) (void)hipEventDestroy(e);
    if (done) (void)hipEventDestroy(done);
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
};

#define BP_HIP(call)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                \
      char buf_[512];                                                                      \
      std::snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                    __FILE__, __LINE__);                                                   \
      h->err = buf_;                                                                       \
      return (e_ == hipErrorOutOfMemory) ? BP_ERR_OUT_OF_MEMORY : BP_ERR_HIP;              \
    }                                                                                      \
  } while (0)

namespace bp {
int run_chunk(bp_handle h, const float* audio_dev, int n, float* note_dev, float* onset_dev, float* contour_dev);
int wait_stream(bp_handle h);
// track_api.hip: the end of a call that has queued work, and the argument domain of raw PCM
int finish(bp_handle h, int rc);
int pcm_width(int format);
int check_ingest(bp_handle h, bool pcm_given, int format, int64_t n_frames, int channels, int sample_rate, int mem_kind);
// the resampling filter sample_rate -> the handle's rate on the device: the plan, the table (with the 2 : 1 kernel's reversed
// copy behind it) in *dev, which owns it.  tabulated_only: a plan whose taps are evaluated in the kernel is returned
// in *plan with BP_ERR_UNSUPPORTED, nothing allocated and no message set.
int upload_filter(bp_handle h, int sample_rate, bool tabulated_only, ResamplePlan* plan, DeviceBuffer<double>* dev);
// the three maps of T rows: [T][88] note, [T][88] onset, [T][264] contour — one after the other when they share a block
struct Maps { float *note, *onset, *contour; };
constexpr int64_t kMapsRow = 2 * kFreqN + kFreqC;  // floats of one row of all three
inline Maps maps_at(float* base, int64_t T) { return {base, base + T * kFreqN, base + T * 2 * kFreqN}; }
int copy_maps(bp_handle h, const Maps& dst, const Maps& src, int64_t T, hipMemcpyKind kind);
// the handle's tables of the device-side note candidates (note_device.hip), made on first use: the bend windows and the
// Gaussian on the device, the page-locked copy of the stats record
int note_tables(bp_handle h, const void** tab, const double** gauss);
constexpr size_t kTabBytes = 88 * 16, kGaussBytes = 51 * 8, kStatsBytes = 16;  // of nd_tables; a stats record
// track_api.hip, for the jobs of many clips (clips_api.hip and the sinks' files).  The geometry of a handle: the length of a signal resampled to
// `rate`, the rows of the maps of n samples at the handle's rate
int64_t resampled_length(int64_t n_frames, int sample_rate, int rate);
int64_t h_frames(bp_handle h, int64_t n);
// the only way to h->track_out, grown for `rows` rows of maps (h->maps_rows = 0); the same with a private copy of given maps
int take_track_out(bp_handle h, int64_t rows, Maps* m);
int take_given_maps(bp_handle h, const float* note, const float* onset, const float* contour, int64_t T, int mem_kind, Maps* m);
// IMA ADPCM (adpcm_device.hip): the blocks of n files (lay[i] of files[i]; all of lay[0]'s codec) to the device and one decode
// launch for all; file i's interleaved int16 samples at h->ad.pcm + pcm_off[i].  segs stays alive until the wait.
int queue_adpcm(bp_handle h, int64_t n, const void* const* files, const bp_adpcm_layout* lay, std::vector<AdpcmSeg>& segs,
                int64_t* pcm_off);
// the PCM format the device FLAC decoders write (left-justified), and n such samples as int32 (src may be out)
int flac_format(const bp_flac_stream_layout& lay);
void flac_pcm_to_int32(const void* src, bool wide, int shift, int64_t n, int32_t* out);
// windows of device-resident signals at the handle's rate -> their un-overlapped maps, packed into full chunks
int tracks_core(bp_handle h, int64_t n_tracks, const float* const* d_in, const int64_t* n_samples, const Maps* d_out);
// room for the bitmap and the bends of T rows in h->nd_buf; the candidates of T rows and n_stats records on their way home
int reserve_candidates(bp_handle h, int64_t T, uint8_t** d_bits, int8_t** d_bend);
int send_candidates(bp_handle h, const float* d_note, int64_t T, const uint8_t* d_bits, const int8_t* d_bend, float* note_out,
                    uint8_t* cand_out, int8_t* bend_out, void* d_stats, int* stats_host, void* stats_host_dev, int64_t n_stats,
                    bool* exported_by_kernel);

// ---- the tracker (note_track.hip) behind any dense half, its host half in clips_api.hip: the clips calls there and in clips_sweep.hip,
// bp_streams_events (stream_api.hip).
// Where a call's results go:
struct EventsSink {
  bp_note_event* events;
  int64_t max_events;
  int32_t* bends;
  int64_t max_bends;
  int64_t* event_offsets;
  int* status;
};
// A job of n segments, segment c at rows [offs[c], offs[c + 1]) of the dense half's outputs.  prm: the parameters of all
// segments (the clips calls' launch), or seg: one record per segment.  first_frame (null: zeros) is added to a segment's frames.
struct EventsJob {
  const char *what, *count_name;  // for messages: the call, and its name for n
  int64_t n;
  const int64_t* offs;
  const bp_note_params* prm;
  const NoteTrackSeg* seg;
  const int64_t* first_frame;
  int form;
};
struct EventsPlan {
  std::vector<int64_t> ev_first;  // read by an asynchronous copy: alive until the wait
  int64_t max_rows = 0;
};
// what the dense half left on the device: note rows, bitmap, bend map (null: none), the row offsets, a record per segment
struct TrackInputs {
  const float* note;
  const uint8_t* bits;
  const int8_t* bend;
  const int64_t* offs;
  const void* stats;
};
// The handle's buffers grown to the job (nothing queued); the tracker, the pack and the offsets on their way home; and, after
// the wait, the offsets and status, the events and bends home in one copy each and the frame-to-time arithmetic.
// *device_error (may be null) is set where events_home fails after queuing; buffers too small is not such a failure.
// home false: the events stay in the pool (a scored sweep) — no bends, no packed copies, no offsets.
int events_reserve(bp_handle h, const EventsJob& job, EventsPlan* plan, bool home = true);
int events_queue(bp_handle h, const EventsJob& job, const EventsPlan& plan, const TrackInputs& in);
int events_home(bp_handle h, const EventsJob& job, const EventsSink& out, bool* device_error);
}  // namespace bp
