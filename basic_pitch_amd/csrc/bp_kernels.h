// Private to csrc: the host functions each kernel file exports to the rest of the library, and the FLAC decoder's host
// structs.  Every file that defines one of these includes this header, so the compiler checks each definition against
// its declaration.  Declarations under BP_AB_KERNELS exist only in the A/B library (build.py AB_SOURCES).
#pragma once
#include <vector>

#include "bp_common.h"
#include "device_buffer.h"

namespace bp {

// cqt_pyramid.hip
void launch_pyramid(const float* audio, float* pyr, const float* lowpass, int n_windows, hipStream_t s);
// windowing / un-overlapping over the segments of a chunk: the table in the kernel arguments (track calls) or in device
// memory (streaming steps)
void launch_window_tracks(const WindowSegs& ts, int n_slots, float* audio, int win_len, int hop, hipStream_t stream);
void launch_unwrap_tracks(const WindowSegs& ts, int n_slots, const float* note, const float* onset, const float* contour,
                          hipStream_t stream);
void launch_window_streams(const WindowSeg* segs, int n_segs, int n_slots, float* audio, int win_len, int hop,
                           hipStream_t stream);
void launch_unwrap_streams(const WindowSeg* segs, int n_segs, int n_slots, const float* note, const float* onset,
                           const float* contour, hipStream_t stream);

// cqt_filterbank.hip: the exact-f32 filterbank (BP_FLAG_F32_MFMA)
size_t filterbank_scratch_floats(int n_windows);
void launch_filterbank(const float* audio, const float* pyr, const float* bfrag, const float* sqrt_len,
                       float* lp, int* mm, float* scratch, int n_windows, LogConsts kc, int n_cu,
                       hipStream_t s);
void launch_mm_reduce(const float* scratch, int* mm, int n_windows, int n_partials, hipStream_t stream);

// The pyramid as pre-split, reflect-padded f16 planes; operands straight from HBM / L2 (cqt_planes.h).
// cqt_planes_pyramid.hip: the planes of every level from the fp32 audio
int64_t planes_elements_per_window(bool ext);
void launch_planes_split(const float* src, int64_t src_stride, int level, uint16_t* pl, int n_windows, bool ext,
                         hipStream_t stream);
void launch_planes_unsplit(const uint16_t* pl, int level, float* dst, int64_t dst_stride, int n_windows, bool ext,
                           hipStream_t stream);
void launch_planes_edge_rows(const float* audio, int64_t audio_stride, uint16_t* pl, int n_windows, bool ext,
                             hipStream_t stream);
void launch_pyramid_planes(const float* audio, int64_t audio_stride, uint16_t* pl, const void* tfrag, int n_windows,
                           int n_cu, bool ext, hipStream_t stream);
// cqt_planes_filterbank.hip: the filterbank over the planes, normalise / BatchNorm / split fused for whole windows
int filterbank_planes_partials(bool ext);
bool launch_filterbank_planes(const uint16_t* pl, const float* audio, int64_t audio_stride, const void* bfrag,
                              const float* bin_consts, float* lp, float* scratch,
                              uint32_t* zp, int n_windows, LogConsts kc, int n_cu, bool ext, hipStream_t stream);
void filterbank_planes_bin_consts(const float* sqrt_len, int n_bins, LogConsts kc, float* out);

// conv_contour1.hip, conv_stride3.hip, conv_heads.hip: the exact-f32 layers (BP_FLAG_F32_MFMA)
void launch_contour1(const float* lp, const int* mm, const float* bfrag, const float* bias, float* c1,
                     int n_windows, LogConsts kc, int n_cu, hipStream_t s);
void launch_onset1(const float* lp, const int* mm, const float* bfrag, const float* bias, float* o1,
                   int n_windows, LogConsts kc, int n_cu, hipStream_t s);
void launch_note1(const float* contour, const float* bfrag, const float* bias, float* n1, int n_windows,
                  int n_cu, hipStream_t s);
void launch_contour2(const float* c1, const float* wgt, float bias, float* contour, int n_windows,
                     hipStream_t s);
void launch_note2(const float* n1, const float* wgt, float bias, float* note, int n_windows,
                  hipStream_t s);
void launch_onset2(const float* note, const float* o1, const float* wgt, float bias, float* onset,
                   int n_windows, hipStream_t s);

// conv_branch.hip: z pack
void launch_zpack(const float* lp, const int* mm, uint32_t* zp, int n_windows, LogConsts kc, int n_bins,
                  hipStream_t s);
void launch_zpack_partials(const float* lp, const float* scratch, int n_partials, uint32_t* zp, int n_windows,
                           LogConsts kc, int n_bins, hipStream_t stream);

// contour conv1: conv_contour_march.hip (interior), conv_contour_rim_march.hip and conv_contour_rim.hip (rim)
bool contour_conv1_use_march();
// (w2 = conv2's taps [5][5][8]: conv2 in the march's epilogue, c1 = the partial sums of launch_plan.h; nullptr: relu(conv1))
void launch_contour_conv1_march(const uint32_t* zp, const void* wfrag, const float* bias, float* c1, const float* w2,
                                int n_windows, int n_cu, bool weights_have_lo, hipStream_t stream);
void launch_contour_conv1_rim(const uint32_t* zp, const void* afrag, const float* bias, float* c1, int n_windows, int n_cu,
                              bool weights_have_lo, bool ext, hipStream_t stream);
void launch_contour_conv1_rim_march(const uint32_t* zp, const void* afrag, const float* bias, float* c1, int n_windows, int n_cu,
                                    bool weights_have_lo, hipStream_t stream);
// conv_contour2.hip
void launch_contour_conv2_proj(const float* c1, const void* wfrag, float bias, float* contour, int n_windows, int n_cu,
                               bool weights_have_lo, hipStream_t stream);
// behind the fused march: partial sums + the rim's c1 (c1s) -> contour
void launch_contour_conv2_finish(const float* c1s, float* part, const void* wfrag, float bias, float* contour,
                                 int n_windows, int n_cu, bool weights_have_lo, hipStream_t stream);
// note_march16.hip, onset_march16.hip
void launch_note_march16(const float* contour, const void* wfrag, const float* wf32, float* note, int n_windows, int n_cu,
                         bool weights_have_lo, hipStream_t stream);
void launch_onset_march16(const uint32_t* zp, const float* note, const void* wfrag, const float* wf32, float* onset,
                          int n_windows, int n_cu, bool weights_have_lo, hipStream_t stream);

#ifdef BP_AB_KERNELS
// conv_contour_direct.hip: the round-2 folded conv1 (BP_CONV1=rounds)
void launch_contour_conv1_folded(const uint32_t* zp, const void* wfold, const float* bias, float* c1, int n_windows,
                                 int n_cu, bool weights_have_lo, hipStream_t stream);
// conv_contour2.hip: the round-2 vector kernel (BP_CONV2=valu)
void launch_contour_conv2(const float* c1, const float* w2, float bias, float* contour, int n_windows, int n_cu,
                          hipStream_t stream);
// note_march.hip, onset_march.hip: the 32x32x16 forms of the marches (BP_NOTE=march32, BP_ONSET=march32)
void launch_note_march(const float* contour, const void* wfrag, const float* wf32, float* note, int n_windows,
                       bool weights_have_lo, hipStream_t stream);
void launch_onset_march(const uint32_t* zp, const float* note, const void* wfrag, const float* wf32, float* onset,
                        int n_windows, int n_cu, bool weights_have_lo, hipStream_t stream);
// conv_branch.hip: the workgroup onset kernel (BP_ONSET=ring)
void launch_onset_branch(const uint32_t* zp, const float* note, const void* wfrag, const float* wf32, float* onset,
                         int n_windows, int n_cu, bool weights_have_lo, hipStream_t stream);
#endif

// audio_ingest.hip
ResamplePlan make_resample_plan(int source_rate, int target_rate, std::vector<double>& taps);
// channel mean of interleaved PCM of any bp_pcm_format (float PCM: BP_PCM_F32)
void launch_downmix_raw(const void* raw, int format, int64_t n_frames, int channels, float* mono, hipStream_t stream);
void launch_resample(const float* x, int64_t n_in, const double* taps, const ResamplePlan& pl, float* y,
                     int64_t n_out, int mode, hipStream_t stream);
// streaming ingest (stream_api.hip): frames -> mono at dst[(dst_pos + i) % dst_cap] (dst_cap 0: a plain buffer) and, with
// n_hist > 0, the last n_hist mono frames of (hist_old | these frames) -> hist_new; outputs [k0, k0 + n_k) of the signal
// whose frames before `chunk_start` are the n_hist of `hist` and from there on `chunk` -> ring[(ring_pos + i) % ring_cap]
void launch_stream_downmix(const void* raw, int format, int64_t n_frames, int channels, float* dst, int dst_pos, int dst_cap,
                           const float* hist_old, float* hist_new, int n_hist, hipStream_t stream);
void launch_stream_resample(const float* hist, int n_hist, const float* chunk, int64_t chunk_start, int64_t n_in,
                            const double* taps, const ResamplePlan& pl, int64_t k0, int64_t n_k, float* ring, int ring_pos,
                            int ring_cap, hipStream_t stream);

// batched ingest (bp_infer_clips_candidates): one clip of the table a call uploads.  The downmix launch gives clip c the
// workgroups [mono_block, next clip's mono_block), the resampling launch [out_block, next clip's out_block); a clip that
// needs no downmix (mono float32) or no resampling (already at the handle's rate) takes none and is read where it lies.
struct ClipDesc {
  const void* src;     // the clip's interleaved PCM (device)
  const float* mono;   // its mono float32 form: src itself, or where the downmix writes it
  float* out;          // its signal at the handle's rate, where the resampling writes it
  int64_t n_frames;    // frames of PCM
  int64_t n_out;       // samples at the handle's rate
  int64_t mono_block;  // first workgroup of the downmix launch (1024 frames each)
  int64_t out_block;   // first workgroup of the resampling launch (256 outputs each)
  int format, channels;
};
// clips: the table in device memory, n_blocks: the workgroups of all clips together
void launch_clips_downmix(const ClipDesc* clips, int64_t n_clips, int64_t n_blocks, hipStream_t stream);
void launch_clips_resample(const ClipDesc* clips, int64_t n_clips, int64_t n_blocks, const double* taps, const ResamplePlan& pl,
                           hipStream_t stream);

// flac_device.hip
struct FdStream {
  int channels, bits, min_block, max_block;
  int64_t total;       // samples per channel
  uint32_t audio_start, nbytes;
};
struct FlacDeviceBuffers {
  DeviceBuffer<uint8_t> file;                   // the file's bytes + 64 zero bytes
  DeviceBuffer<uint8_t> cands, packed, frames;  // FdCand [chunks][kFdChunkCands]; FdCand, in file order; FdFrame
  DeviceBuffer<uint32_t> counts, offs;
  DeviceBuffer<int32_t> scratch;
  DeviceBuffer<int> meta;                       // [0] status, [1] n_frames (a job of clips: that pair per clip)
  DeviceBuffer<uint16_t> crc_tab;
  DeviceBuffer<uint8_t> clips;                  // flac_clips.hip: the job's table (FdClip)
};
int flac_device_decode(FlacDeviceBuffers& b, const FdStream& st, void* d_pcm, hipStream_t stream);
int flac_device_crc_table(FlacDeviceBuffers& b);  // b.crc_tab, made on first use; 0 or -1

// adpcm_device.hip: IMA ADPCM blocks -> interleaved int16.  One segment = the blocks of one file (a job of clips: n segments in
// one launch; a single file: one).  Offsets count from the start of the buffers the launch is given.
struct AdpcmSeg {
  int64_t byte_off;     // the segment's first block in the bytes buffer
  int64_t data_bytes;   // bytes of blocks that may be read from there
  int64_t out_off;      // its first sample (int16) in the output buffer
  int64_t frame_cap;    // frames of it that may be written: [0, frame_cap)
  int64_t first_chain;  // chains (one channel of one block) of the segments before it
  int32_t n_blocks, block_bytes, block_frames, channels;
};
struct AdpcmDeviceBuffers {
  DeviceBuffer<uint8_t> file;   // the bytes of the call's files, one after the other
  DeviceBuffer<int16_t> pcm;    // the decoded samples
  DeviceBuffer<AdpcmSeg> segs;  // the launch's segment table
};
// codec: BP_ADPCM_IMA_WAV | BP_ADPCM_IMA4.  segs: n_segs records in device memory, first_chain ascending; n_chains: of all.
// Every read lies inside [byte_off, byte_off + data_bytes) of its segment, every write inside its frame_cap.
void launch_adpcm_decode(int codec, const uint8_t* bytes, const AdpcmSeg* segs, int n_segs, int64_t n_chains, int16_t* pcm,
                         hipStream_t stream);

constexpr int kFdChunkBytes = 65536;  // bytes of a stream a scan workgroup owns (flac_kernels.h kFdChunk)
// flac_clips.hip: one stream of a job of many (bp_infer_flac_clips_candidates).  The job's bytes lie in FlacDeviceBuffers::file,
// clip by clip; st.audio_start and st.nbytes count from the clip's first byte.  The table is sorted by first_wg and first_slot.
struct FdClip {
  FdStream st;
  uint64_t base;         // the clip's first byte in the job's buffer: 16-byte aligned, >= 64 zero bytes behind the clip
  uint32_t first_wg;     // its first workgroup of the scan launch = its first slice of the candidate lists (n_chunks >= 1 of them)
  uint32_t first_slot;   // its first frame slot (max_frames >= 1 of them)
  int32_t n_chunks, max_frames;
  uint64_t scratch_off;  // its rows of scratch ([max_frames][channels][max_block] int32), in int32s
  uint64_t pcm_off;      // its interleaved PCM in the job's PCM buffer, in bytes (16-byte aligned)
  int32_t out_shift, out_wide;  // sample << out_shift fills an int16 (0) or int32 (1) word: BP_PCM_S16 / BP_PCM_S32
};
int flac_clips_decode(FlacDeviceBuffers& b, const FdClip* tab, int64_t n_clips, int64_t wgs, int64_t slots, int64_t scratch,
                      void* d_pcm, size_t pcm_bytes, hipStream_t stream);

// note_device.hip
void launch_note_candidates(float* note, float* onset, const float* contour, int64_t T, int lo, int hi, int infer,
                            double onset_thresh, const void* tab, const double* gauss, void* stats, uint8_t* bits,
                            int8_t* bend, hipStream_t s);
void launch_note_export(const void* note, void* note_dst, int64_t note_bytes, const void* bits, void* bits_dst,
                        int64_t bits_bytes, const void* bend, void* bend_dst, int64_t bend_bytes, void* stats,
                        void* stats_dst, int64_t n_stats, hipStream_t s);
// many clips in one buffer, clip c at rows [offs[c], offs[c + 1]) (offs: device memory), each decoded as its own whole track:
// n_clips stats records of 16 bytes to their initial values; launch_note_candidates for every clip (its record: table[c])
void launch_clips_stats_init(void* table, int64_t n_clips, hipStream_t s);
void launch_clips_candidates(float* note, float* onset, const float* contour, const int64_t* offs, int64_t n_clips,
                             int64_t total_rows, int lo, int hi, int infer, double onset_thresh, const void* tab,
                             const double* gauss, void* table, uint8_t* bits, int8_t* bend, hipStream_t s);
void launch_note_stats_init(void* stats, hipStream_t s);
// constrain_frequency into copies: the bins outside [lo, hi) of n_rows rows of note -> note_dst and onset -> onset_dst are 0, the
// others the source's; a null destination is skipped.  The sources are only read (a sweep's maps are shared by its sets).
void launch_constrain_copy(const float* note, const float* onset, float* note_dst, float* onset_dst, int64_t n_rows, int lo,
                           int hi, hipStream_t s);

// note_track.hip: the sequential half of note decoding for many clips, one workgroup per clip (bp_infer_clips_events).
// A clip of at most kNoteTrackLdsRows rows keeps its working copy of the note rows in LDS, a longer one in `scratch`
// (note_track_scratch_floats of all rows); one of more than kNoteTrackMaxRows rows is not decoded (status 2).
constexpr int kNoteTrackLdsRows = 432, kNoteTrackMaxRows = 8192;
// event records a clip's region of the pool holds (BP_EVENTS_CAPACITY of include/basic_pitch_amd_events.h)
int64_t note_track_capacity(int64_t rows, int min_note_len);
int64_t note_track_scratch_floats(int64_t total_rows);
// note / bits / bend_map (null: no bends) / offs / stats: what launch_clips_candidates left on the device for n_clips > 0 clips.
// ev_first [n_clips + 1]: the event records before each clip's region of ev_pool (16 bytes each); clip c's bends go to
// bd_pool + 88 * offs[c].  counts: n_clips records of 16 bytes.  Then the second step: meta = [n_clips + 1] events before each
// clip, [n_clips + 1] bends before each clip, [n_clips] status; ev_out / bd_out the events and bends contiguous in clip order.
hipError_t launch_note_track(const float* note, const uint8_t* bits, const int8_t* bend_map, const int64_t* offs,
                             const int64_t* ev_first, const void* stats, int64_t n_clips, int64_t max_rows, double frame_thresh,
                             int energy_tol, int min_note_len, int melodia, float* scratch, void* ev_pool, int8_t* bd_pool,
                             void* counts, int64_t* meta, void* ev_out, int8_t* bd_out, hipStream_t s);
// The same for segments that carry their own parameters (bp_streams_events: a segment is a stream's slice).  seg: a device table
// of n_segs records; bend_map is read only for segments with `bends`; a segment with `skip` gets status 1 and no events.
// form: kNoteTrackFormAuto — the LDS form up to kNoteTrackLdsRows rows, the scratch form beyond —, or kNoteTrackFormScratch to
// keep every segment's working state in `scratch` (the A/B library's tests).
struct NoteTrackSeg {
  double frame_thresh;
  int energy_tol, min_note_len, melodia, bends, skip, reserved;
};
constexpr int kNoteTrackFormAuto = 0, kNoteTrackFormScratch = 2;  // 1 was the bit-plane form (measured, not kept)
hipError_t launch_note_track_segs(const float* note, const uint8_t* bits, const int8_t* bend_map, const int64_t* offs,
                                  const int64_t* ev_first, const void* stats, const NoteTrackSeg* seg, int64_t n_segs,
                                  int64_t max_rows, int form, float* scratch, void* ev_pool, int8_t* bd_pool, void* counts,
                                  int64_t* meta, void* ev_out, int8_t* bd_out, hipStream_t s);
// The same over the decode table of a sweep (bp_note_events_sweep, include/basic_pitch_amd_sweep.h): decode j is one
// workgroup, a segment of the shared maps under one parameter set.  Many decodes read the same rows; what a decode writes is
// its own: with pool_rows[j] the rows of the decodes before it, its bends go to bd_pool + 88 * pool_rows[j], its working state
// (a segment of more than kNoteTrackLdsRows rows) to scratch + note_track_scratch_floats(pool_rows[j]), its events to its region
// ev_first[j] of ev_pool.  pool_rows and ev_first ([n_decodes + 1], device memory) are the two arrays the offsets and pack
// launches read for the clips of a job; meta, ev_out and bd_out are theirs, over decodes.
struct NoteSweepDecode {
  const float* note;    // the note rows its set decodes: the copy constrained to the set's band (all segments' rows)
  const uint8_t* bits;  // the onset-peak bitmap of its set's dense key (all segments' rows)
  const void* stats;    // its segment's record in that key's block (null: seg.skip)
  int64_t first, rows;  // its segment's rows in `note`, `bits` and the bend map
  NoteTrackSeg seg;     // the tracker's parameters; skip: an onset threshold <= 0, the host's (status 1)
};
hipError_t launch_note_track_sweep(const NoteSweepDecode* tab, int64_t n_decodes, int64_t max_rows, const int8_t* bend_map,
                                   const int64_t* pool_rows, const int64_t* ev_first, float* scratch, void* ev_pool, int8_t* bd_pool,
                                   void* counts, int64_t* meta, void* ev_out, int8_t* bd_out, hipStream_t s);
// meta null: the tracker alone — no offsets, no pack, ev_out and bd_out unused; the events stay in the decodes' regions of
// ev_pool with their counts and statuses in `counts` (16 bytes per decode: events, bends, status, 0) for launch_note_score.

// note_score.hip: the decodes of a sweep scored against reference notes in place (bp_note_events_sweep_score,
// include/basic_pitch_amd_score.h), one workgroup per decode behind launch_note_track_sweep(meta = null).  refs: the table of
// all segments' refs with the offset tolerance each ref sets; dec[j]: the refs of decode j's segment.  prm: the tolerances the
// predicates compare against.  max_refs / max_depth size the launch's LDS (note_score_lds_bytes): every decode has at most
// max_refs refs or more than kNoteScoreMaxNotes (status 3), and min(events its region holds, refs + 1) <= max_depth.
// out: [n_decodes] {n_ref, n_est, matched_onset, matched_offset}, then [n_decodes] status.
constexpr int kNoteScoreMaxNotes = 16384;  // BP_SCORE_MAX_NOTES
struct NoteScoreRef {
  double start_s, end_s, pitch_midi;
  double offset_tol;  // max(offset_ratio * (end_s - start_s), offset_min_tolerance_s)
};
struct NoteScoreDecode {
  int64_t ref_first;
  int32_t n_ref;      // at most kNoteScoreMaxNotes + 1 (more: the same status)
  int32_t bend_room;  // 88 * rows where the decode's set asks for bends, else -1.  No bends are made, but a decode whose
                      // events span more frames than its bend region would hold is the sweep calls' status 2: the tracker
                      // stops at the event that passes the room, and the lengths being positive, that is when the sum does
};
struct NoteScoreParams {
  double onset_tol, pitch_tol;
  int strict;
};
size_t note_score_lds_bytes(int max_refs, int max_depth);
hipError_t launch_note_score(const void* counts, const int64_t* ev_first, const void* ev_pool, const NoteScoreDecode* dec,
                             const NoteScoreRef* refs, const NoteScoreParams& prm, int64_t n_decodes, int max_refs, int max_depth,
                             int32_t* out, hipStream_t s);
// The same decodes scored frame by frame (note_frames.hip; bp_note_events_sweep_frame_score,
// include/basic_pitch_amd_frame_score.h), one workgroup per decode, beside or in place of launch_note_score.  rows: [n_decodes
// + 1] the rows of the decodes before each (the tracker's row offsets).  dec: launch_note_score's table, read for the refs of
// the decode's segment and the status; refs: per segment its refs IN ASCENDING PITCH, each as the frames it sounds on and the
// note bins it hits (made on the host by the checker's functions, note_frames_host.cpp).  max_rows: the longest decode, which
// sizes the launch's LDS (note_frames_lds_bytes).  out: [n_decodes] {n_frames, ref_frames, est_frames, true_pos, e_sub},
// then, as 32-bit words, [n_decodes] status — the status launch_note_score leaves.
constexpr int kNoteFramesChunk = 2048;  // frames a workgroup rolls into LDS at a time
struct NoteFrameRef {
  int32_t f0, f1;  // sounds on frames f0 ... f1 - 1 of its segment
  int32_t lo, hi;  // hits the note bins lo ... hi (lo > hi: none)
};
size_t note_frames_lds_bytes(int64_t max_rows);
hipError_t launch_note_frames(const void* counts, const int64_t* rows, const int64_t* ev_first, const void* ev_pool,
                              const NoteScoreDecode* dec, const NoteFrameRef* refs, int64_t n_decodes, int64_t max_rows, int64_t* out,
                              hipStream_t s);
// multipitch.hip: the f0 peaks of contour rows (include/basic_pitch_amd_multipitch.h).  T rows in n_segs
// segments, segment i at rows [offs[i], offs[i + 1]) (offs on the device).
// count: row_info[r] = {the peaks of row r, its segment}, seg_bad[i] != 0 where a cell of segment i is not finite (zeroed by
// the caller).  scan: row_first[r] = the points before row r with the rows of flagged segments empty, row_first[T] the total;
// meta = point_offsets [n_segs + 1], then as 32-bit words the statuses [n_segs].  write: the points (16-byte bp_f0_point
// records) of every row at row_first[r]; the caller has made sure that row_first[T] of them fit.
constexpr int kMpBins = 264, kMpScanTile = 1024;  // BP_MP_BINS, BP_MP_SCAN_TILE_ROWS
struct MpParams {  // bp_mp_params
  float threshold;
  int32_t min_bin, max_bin, reserved;
};
hipError_t launch_mp_count(const float* contour, const int64_t* offs, int64_t n_segs, int64_t T, MpParams p, int2* row_info,
                           int32_t* seg_bad, hipStream_t s);
hipError_t launch_mp_scan(const int2* row_info, const int32_t* seg_bad, const int64_t* offs, int64_t n_segs, int64_t T,
                          int64_t* row_first, int64_t* meta, hipStream_t s);
hipError_t launch_mp_write(const float* contour, int64_t T, MpParams p, const int2* row_info, const int32_t* seg_bad,
                           const int64_t* offs, const int64_t* row_first, void* points, hipStream_t s);
// The decodes of a multi-pitch sweep scored frame by frame, one workgroup per decode: decode j is rows [first, first + rows)
// of contour under sets[set] against refs[ref_first ... ref_first + n_ref), its segment's IN ASCENDING PITCH with the frames
// they sound on.  out: [n_decodes] {n_frames, ref_frames, est_frames, true_pos, e_sub}, then as 32-bit words [n_decodes]
// status (1: a cell is not finite; 3: n_ref > kNoteScoreMaxNotes).
struct MpRef {
  int32_t f0, f1;  // sounds on frames f0 ... f1 - 1 of its segment
  double pitch;
};
struct MpDecode {
  int64_t first, rows, ref_first;
  int32_t n_ref, set;  // n_ref at most kNoteScoreMaxNotes + 1 (more: the same status)
};
struct MpScoreParams {
  double pitch_tolerance_cents;
  bool strict;
};
constexpr int64_t kMpSweepLongRows = 2048;  // a job whose longest decode has more rows gets workgroups of 16 waves, not 4
hipError_t launch_mp_sweep_frames(const float* contour, const MpParams* sets, const MpDecode* dec, const MpRef* refs,
                                  MpScoreParams sp, int64_t n_decodes, int64_t max_rows, int64_t* out, hipStream_t s);
// melody.hip: one f0 track per decode by a Viterbi recurrence over its rows (include/basic_pitch_amd_melody.h),
// a workgroup per decode.  Decode j is rows [first, first + rows) of contour under sets[set]; its predecessors go to rows
// [pred_first, pred_first + rows) of pred (kMelodyPredStride bytes a row, regions of distinct decodes disjoint).  points given:
// record r of decode j at points[first + r] (16-byte bp_melody_point records).  points null: the records are scored against
// ref_pitch[first + r] instead and scores[j] = {n_frames, ref_voiced, est_voiced, both_voiced, pitch_ok, chroma_ok}.  status[j]:
// 0, or 1 where a cell of the rows is NaN or above 65536 in magnitude (unvoiced records, or {n_frames, 0, 0, 0, 0, 0}).
// max_jump: the largest max_jump of the sets the decodes name; a launch whose sets all stay within kMelodyNarrowJump reads
// windows of that width, any other the full kMelodyMaxJump on either side.
constexpr int kMelodyMaxJump = 16, kMelodyReadAhead = 8, kMelodyTileRows = 128, kMelodyPredStride = 272;  // BP_MELODY_*
constexpr int kMelodyNarrowJump = 4;
struct MelodyParams {  // bp_melody_params
  float threshold, jump_penalty, voicing_penalty;
  int32_t max_jump, min_bin, max_bin, reserved[2];
};
struct MelodyDecode {
  int64_t first, rows, pred_first;
  int32_t set, reserved;
};
hipError_t launch_melody(const float* contour, const MelodyParams* sets, const MelodyDecode* dec, int64_t n_decodes, int max_jump,
                         uint8_t* pred, void* points, const double* ref_pitch, MpScoreParams sp, int64_t* scores, int32_t* status,
                         hipStream_t s);
// align.hip: forced alignment (include/basic_pitch_amd_align.h).  Segment c of segs is rows [row_first, row_first
// + rows) of note / onset against states [state_first, state_first + n_states) of states, rows > 0 and 1 <= n_states <=
// kAlignMaxStates; its gains go to cells [cell_first, cell_first + rows * n_states) of gains (8 bytes a cell), its predecessor
// bits to words [pred_first, pred_first + rows * ceil(n_states / 64)) of pred, and the tiles of 32 rows x 32 states of its
// emissions are tiles [tile_first, tile_first + ceil(rows / 32) * ceil(n_states / 32)) of the n_tiles of the launch (the
// regions of distinct segments disjoint, tile_first ascending).  first_frame[state_first + j], total[c], status[c]: the
// header's, -1 / 0 with a status of 1 (a NaN; nan_flags [n_segs] is scratch) or 2 (infeasible).  max_states: the largest
// n_states, which chooses the workgroup of the recurrence.  note and onset must be 16-byte aligned.
constexpr int kAlignLanes = 1024, kAlignSmallLanes = 256, kAlignMaxStates = 4096, kAlignReadAhead = 8, kAlignReadAheadWide = 4;  // BP_ALIGN_*
constexpr int kAlignTileRows = 128, kAlignEmitRows = 32;
struct AlignState {  // bp_align_state
  uint64_t active[2], begins[2];
  int32_t earliest, latest;
};
struct AlignSeg {
  int64_t row_first, rows, state_first, cell_first, pred_first, tile_first;
  int32_t n_states, segment;  // segment: the caller's index (the kernels do not read it)
};
hipError_t launch_align(const float* note, const float* onset, const AlignState* states, const AlignSeg* segs, int64_t n_segs,
                        int64_t n_tiles, int max_states, int threshold_q, int onset_weight, void* gains, uint64_t* pred,
                        uint32_t* nan_flags, int32_t* first_frame, int64_t* total, int32_t* status, hipStream_t s);
// beat.hip: tempo and beats (include/basic_pitch_amd_beat.h).  Segment c of segs is rows [row_first, row_first +
// rows) of onset, rows > 0; it is blocks [blk_first, blk_first + ceil(rows / kBeatStrengthRows)) of the n_blocks of the strength
// launch and tiles [tile_first, tile_first + ceil(rows / kBeatTempoRows) * lag_tiles) of the n_tiles of the tempo launch
// (lag_tiles: ceil(admissible lags / kBeatTempoLags), 0 where rows <= lag_min; both firsts ascending, the regions of distinct
// segments disjoint).  strength [all rows] is o[t], parallel to the rows of onset; acc is kBeatAccStride int64 a segment: sum o,
// sum o^2, the NaN flag, A[0 ... 256], and four clock readings of the path kernel (100 MHz: start, period picked, recurrence
// done, backtrace done) for tools/bench_beat.py; pred one uint16 a row, parallel to the rows of onset.  summaries[c]: the
// header's record.  The beats of segment c go to beats[beat_first ...) IN DESCENDING ORDER, summaries[c].n_beats of them (at most
// bp_beats_capacity of the segment: the caller's region).  onset must be 16-byte aligned.
constexpr int kBeatMaxLag = 256, kBeatRing = 1024, kBeatTempoRows = 256, kBeatTempoLags = 64, kBeatPathWaves = 16;  // BP_BEAT_*
constexpr int kBeatStrengthRows = 32, kBeatAccStride = 264, kBeatAccLags = 3, kBeatAccClocks = 260;
struct BeatParams {  // bp_beat_params
  int32_t threshold_q, min_pitch, max_pitch, lag_min, lag_max, tightness, reserved[2], prior[kBeatMaxLag + 1], reserved_tail;
};
struct BeatSummary {  // bp_beat_summary
  int32_t status, period;
  int64_t n_beats, score;
  double period_refined;
};
struct BeatSeg {
  int64_t row_first, rows, blk_first, tile_first, beat_first, beat_cap;  // beat_cap: the room at beat_first; nothing is stored beyond it
  int32_t lag_tiles, segment;  // segment: the caller's index (the kernels do not read it)
};
hipError_t launch_beats(const float* onset, const BeatParams* params, const BeatSeg* segs, int64_t n_segs, int64_t n_blocks,
                        int64_t n_tiles, int32_t* strength, int64_t* acc, uint16_t* pred, int32_t* beats, BeatSummary* summaries,
                        hipStream_t s);
// chord.hip: chords and key (include/basic_pitch_amd_chord.h).  Segment c of segs is rows [row_first, row_first +
// rows) of note, rows > 0, the segments' rows one run from 0 to n_rows; it is blocks [blk_first, blk_first + ceil(rows /
// kChordChromaRows)) of the n_blocks of the chroma launch and units [unit_first, unit_first + n_units) of records and
// unit_labels.  pooled 0: unit u is row u.  pooled 1: the units lie between bounds[bound_first ... bound_first + n_units - 1)
// (strictly ascending inside 0 < B < rows) and are units [pool_first, pool_first + n_units) of the n_pool_units of the pool
// launch (pool_first ascending).  chroma is one row of 16 uint16 a row of note (classes 0 ... 11, then zeros), pool one row
// of 16 uint32 a pooled unit (the classes' sums, the unit's length, zeros); acc is kChordAccStride int64 a segment: sum c, sum
// c^2, the NaN flag, Ctot[12], and at kChordAccClocks four clock readings of the path kernel (100 MHz: start, key picked,
// recurrence done, backtrace done) for tools/bench_chord.py; records 16 bytes a unit (the predecessor mask and the best
// state); unit_labels a byte a unit; labels a byte a row of note; summaries[c]: the header's record.  note must be 16-byte
// aligned.
constexpr int kChordMaxStates = 64, kChordClasses = 12, kChordChromaRows = 32, kChordTraceTile = 512, kChordPathWaves = 4;  // BP_CHORD_*
constexpr int kChordChunk = 64, kChordAccStride = 24, kChordAccClasses = 3, kChordAccClocks = 16;
struct ChordParams {  // bp_chord_params
  int32_t threshold_q, min_pitch, max_pitch, n_states, switch_penalty, reserved[3], bias[kChordMaxStates];
  int32_t weights[kChordMaxStates][kChordClasses], key_profile[2][kChordClasses];
};
struct ChordSummary {  // bp_chord_summary
  int32_t status, key, n_units, n_changes;
  int64_t score, key_score;
};
struct ChordSeg {
  int64_t row_first, rows, blk_first, unit_first, n_units, pool_first, bound_first;
  int32_t pooled, segment;  // segment: the caller's index (the kernels do not read it)
};
hipError_t launch_chords(const float* note, const ChordParams* params, const ChordSeg* segs, int64_t n_segs, int64_t n_blocks,
                         int64_t n_rows, int64_t n_pool_units, const int32_t* bounds, uint16_t* chroma, uint32_t* pool, int64_t* acc,
                         void* records, uint8_t* unit_labels, uint8_t* labels, ChordSummary* summaries, hipStream_t s);
// sync.hip: two recordings against each other (include/basic_pitch_amd_sync.h).  Segment c of segs is rows
// [row_first, row_first + rows) of note, rows > 0, and units [unit_first, unit_first + n_units) of the n_units of feat, 16
// bytes a unit (unit_first ascending).  Pair p of pairs is segments a and b of segs, pred_bytes bytes of pred from pred_first
// (16-byte aligned) and n_a + n_b - 1 entries of walk and of path from path_first; summaries[p]: the header's record.  max_n,
// max_m: the most units of an a and of a b; they choose the launch variant (sync_plan), which the host needs for the pairs'
// pred_bytes.  note is read by 4-byte loads: it needs no alignment beyond a float's.
constexpr int kSyncMaxUnits = 8192, kSyncMaxHop = 64, kSyncTraceTile = 64;  // BP_SYNC_*
constexpr int kSyncSmallLanes = 256, kSyncLanes = 1024, kSyncSmallRows = 2048;
constexpr int64_t kSyncMaxPredBytes = 1ll << 28;  // BP_SYNC_MAX_PRED_BYTES
struct SyncParams {  // bp_sync_params
  int32_t threshold_q, min_pitch, max_pitch, hop, band, reserved[3];
};
struct SyncSummary {  // bp_sync_summary
  int32_t status, units_a, units_b, n_path;
  int64_t path_first, total;
};
struct SyncSeg {
  int64_t row_first, rows, unit_first, n_units;
};
struct SyncPair {
  int32_t a, b;
  int64_t pred_first, path_first;
};
// the variant for a job whose longest b has max_m units: lanes of the workgroup, columns a lane, bytes of predecessors a lane
// and step
struct SyncPlan {
  int lanes, cols, pred_bytes;
};
inline SyncPlan sync_plan(int max_m) {
  if (max_m <= kSyncSmallLanes) return SyncPlan{kSyncSmallLanes, 1, 1};
  if (max_m <= 2 * kSyncSmallLanes) return SyncPlan{kSyncSmallLanes, 2, 1};
  if (max_m <= 4 * kSyncSmallLanes) return SyncPlan{kSyncSmallLanes, 4, 1};
  if (max_m <= 8 * kSyncSmallLanes) return SyncPlan{kSyncSmallLanes, 8, 2};
  if (max_m <= 4 * kSyncLanes) return SyncPlan{kSyncLanes, 4, 1};
  return SyncPlan{kSyncLanes, 8, 2};
}
// the bytes of predecessors of a pair of n x m units under a plan: (n + lanes in use - 1) steps of lanes in use
inline int64_t sync_pred_bytes(const SyncPlan& plan, int64_t n, int64_t m) {
  const int64_t used = (m + plan.cols - 1) / plan.cols;
  return ((n + used - 1) * used * plan.pred_bytes + 15) / 16 * 16;
}
hipError_t launch_sync(const float* note, const SyncParams& params, const SyncSeg* segs, int64_t n_segs, int64_t n_units,
                       const SyncPair* pairs, int64_t n_pairs, int max_n, int max_m, uint32_t* nan_flags, void* feat, uint8_t* pred,
                       uint32_t* walk, int32_t* path, SyncSummary* summaries, hipStream_t s);
// frames [t0, t1) of linear device maps join a stats record (launch_note_candidates' second step on its own)
void launch_note_fold(const float* note, const float* onset, int64_t t0, int64_t t1, int infer, void* stats, hipStream_t s);
// The rows a stream retains (stream_api.hip): `ring` is [cap] note, [cap] onset, [cap] contour with absolute row r at slot
// r % cap.  A rolling horizon has beside it `records`, note_ring_records(cap) stats records of 16 bytes: the table of
// per-block extrema of the final rows and, last, one record that is reserved and unused.
int64_t note_ring_records(int64_t cap);
// rows [t0, t0 + n), n <= cap, of linear maps into their slots, frequency-constrained to the bins [lo, hi)
void launch_ring_put(const float* src_note, const float* src_onset, const float* src_contour, float* ring, int64_t cap,
                     int64_t t0, int64_t n, int lo, int hi, hipStream_t s);
// final rows [t0, t1), t1 - t0 <= cap, join the table; blocks that start at or after fresh_from begin anew
void launch_ring_fold(const float* ring, int64_t cap, int64_t t0, int64_t t1, int64_t fresh_from, int infer, void* records,
                      hipStream_t s);
// the rows of [a, T) (R <= T: the final rows) that an update of a rolling horizon scans are [a, *e0) and [*e1, T); the table's
// blocks [*e0, *e1) / 64 join whole
void note_ring_edges(int64_t a, int64_t R, int64_t T, int64_t* e0, int64_t* e1);

// The updates of streams, one or many in a step (stream_api.hip queue_updates): one stream of the table a call uploads.  Behind the table
// lie kStreamUpdatePrefixes arrays of n + 1 int64, the running totals over the streams of: tail rows, workgroups of the stats
// launch (streams_stats_chunks of the edge rows), bitmap rows T - a, workgroups of the bend launch (streams_bend_blocks of
// T - n0, 0 without bends), note rows T - n0.
struct StreamUpdate {
  float* ring;                                         // the store: [cap] note, [cap] onset, [cap] contour
  const float *tail_note, *tail_onset, *tail_contour;  // the tail's rows, linear, row 0 = absolute row R (the step's scratch)
  const void* records;   // the stream's records: the block table (n_tab > 0), or the one record its final rows have joined
  int64_t cap, a, R, T, n0;
  int64_t e0, e1;        // the stats launch scans rows [a, e0) and [e1, T) (note_ring_edges; a keeping stream: a and R)
  int64_t n_tab;         // records of the block table; 0: one carried record
  int64_t note_offset, bits_offset;  // its first row of the packed note / bend rows, of the packed bitmap
  double onset_thresh;
  int lo, hi, infer, bends;
};
constexpr int kStreamUpdatePrefixes = 5;
int64_t streams_stats_chunks(int64_t n_edge);
int64_t streams_bend_blocks(int64_t n_rows);
// the tails' rows to their slots, frequency-constrained per stream (what launch_ring_put does for a stream's final rows)
void launch_streams_put(const StreamUpdate* u, const int64_t* pre, int64_t n, int64_t tail_rows, hipStream_t s);
// per stream: its update record (`stats`: n records of 16 bytes) from its table or carried record and its edge rows, then, packed
// and linear in argument order, the bitmap of [a, T), the bends and the note rows of [n0, T); the last four arguments before the
// queue are device buffers
void launch_streams_candidates(const StreamUpdate* u, const int64_t* pre, int64_t n, int64_t chunks, int64_t bits_rows,
                               int64_t bend_blocks, int64_t note_rows, const void* tab, const double* gauss, void* stats,
                               uint8_t* bits, int8_t* bend, float* note, hipStream_t s);

}  // namespace bp
