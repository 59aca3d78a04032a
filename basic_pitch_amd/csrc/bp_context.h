// Private to csrc: the handle (struct bp_context) and what bp_api.hip and track_api.hip share of it — the kernel launches
// both call, the HIP error macro and the workspace / chunk / wait helpers (defined in bp_api.hip).
#pragma once
#include "../../include/basic_pitch_amd.h"

#include <cstdio>
#include <string>
#include <vector>

#include "bp_common.h"

namespace bp {
// kernels the track entry points launch (one translation unit each)
void launch_window_track(const float* samples, int64_t n_samples, int64_t first_window, int n_windows,
                         float* audio, int win_len, int hop, int lead, hipStream_t stream);
void launch_window_tracks(const TrackSegs& ts, int n_slots, float* audio, int win_len, int hop, int lead,
                          hipStream_t stream);
void launch_unwrap_tracks(const TrackSegs& ts, int n_slots, const float* note, const float* onset, const float* contour,
                          hipStream_t stream);
void launch_unwrap3(const float* note, const float* onset, const float* contour, int64_t first_window, int n_windows,
                    int64_t total_rows, float* o_note, float* o_onset, float* o_contour, hipStream_t stream);
ResamplePlan make_resample_plan(int source_rate, int target_rate, std::vector<double>& taps);
void launch_downmix(const float* pcm, int64_t n_frames, int channels, float* mono, hipStream_t stream);
void launch_downmix_raw(const void* raw, int format, int64_t n_frames, int channels, float* mono, hipStream_t stream);
void launch_resample(const float* x, int64_t n_in, const double* taps, const ResamplePlan& pl, float* y,
                     int64_t n_out, int mode, hipStream_t stream);
// flac_device.hip
struct FdStream {
  int channels, bits, min_block, max_block;
  int64_t total;
  uint32_t audio_start, nbytes;
};
struct FlacDeviceBuffers {
  uint8_t* file = nullptr;
  size_t file_cap = 0;
  void* cands = nullptr;
  uint32_t* counts = nullptr;
  size_t cands_cap = 0, counts_cap = 0;
  void* packed = nullptr;
  uint32_t* offs = nullptr;
  size_t packed_cap = 0, offs_cap = 0;
  void* frames = nullptr;
  int32_t* scratch = nullptr;
  size_t frames_cap = 0, scratch_cap = 0;
  int* meta = nullptr;
  uint16_t* crc_tab = nullptr;
};
int flac_device_decode(FlacDeviceBuffers& b, const FdStream& st, void* d_pcm, hipStream_t stream);
void flac_device_free(FlacDeviceBuffers& b);
// note_device.hip
void launch_note_candidates(float* note, float* onset, const float* contour, int64_t T, int lo, int hi, int infer,
                            double onset_thresh, const void* tab, const double* gauss, void* stats, uint8_t* bits,
                            int8_t* bend, hipStream_t s);
void launch_note_export(const void* note, void* note_dst, int64_t note_bytes, const void* bits, void* bits_dst,
                        int64_t bits_bytes, const void* bend, void* bend_dst, int64_t bend_bytes, void* stats,
                        void* stats_dst, hipStream_t s);
void launch_note_stats_init(void* stats, hipStream_t s);
}  // namespace bp

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
  // device constants
  float *d_lowpass = nullptr, *d_sqrt_len = nullptr, *d_fb_bfrag = nullptr;
  float* d_pl_bin_k = nullptr;  // cqt_planes.hip filterbank: per-bin eps / s^2, s = sqrt(len) 2^-12
  // fused branches (conv_branch.hip): f16 hi/lo A fragments (raw bytes) + {bias1[32], extra[9], bias2}
  float *d_note_wfrag = nullptr, *d_note_w16 = nullptr, *d_note_wf32 = nullptr, *d_onset_wfrag = nullptr, *d_onset_wf32 = nullptr,
        *d_onset_wmx = nullptr, *d_onset_w16 = nullptr;
  float* zp = nullptr;  // uint32 [cap][kZRowsP][kZRow] pre-split z, zero padded (bp_common.h)
  // contour branch, two-kernel form (conv_contour_direct.hip): LDS weight image, bias[8], conv2 taps [5][5][8]
  float *d_d1_wlds = nullptr, *d_d1_wfold = nullptr, *d_d1_wmarch = nullptr, *d_d1_wrim = nullptr, *d_d1_wrimm = nullptr, *d_d1_bias = nullptr,
        *d_d2_w = nullptr, *d_d2_wproj = nullptr;
  bool rim_exact = false, fold_mx = false;
  int resample_mode = 0;  // BP_RESAMPLE=plain|tiled: 1 | 2 (A/B runs of the resampling kernels)
  int contour_parts = 0;  // BP_CONTOUR_PARTS (0: automatic)
  float* d_d1_wfold_mx = nullptr;
  float* c1s = nullptr;  // [cap][172][kC1Row][8] relu(conv1); pad bins zeroed once at allocation
  // cqt_planes.hip: decimator / filterbank fragments (raw bytes of f16 hi / lo), the planes of a chunk [cap][2][stride] f16
  float *d_pl_tfrag = nullptr, *d_pl_bfrag = nullptr, *planes = nullptr;
  float *d_c1_bfrag = nullptr, *d_c1_bias = nullptr, *d_o1_bfrag = nullptr, *d_o1_bias = nullptr;
  float *d_n1_bfrag = nullptr, *d_n1_bias = nullptr, *d_w_contour2 = nullptr, *d_w_note2 = nullptr,
        *d_w_onset2 = nullptr;
  // workspace (per chunk of `cap` windows)
  float *audio = nullptr, *pyr = nullptr, *lp = nullptr, *c1 = nullptr, *contour = nullptr, *n1 = nullptr,
        *note = nullptr, *o1 = nullptr, *onset = nullptr;
  int* mm = nullptr;
  float* fb_scratch = nullptr;  // filterbank partial extrema (grow-only; >= cap windows)
  int64_t fb_scratch_windows = 0;
  // track path staging (grow-only)
  float* track = nullptr;
  int64_t track_cap = 0;
  // audio ingest (audio_ingest.hip): staging for PCM / mono / 22.05 kHz signal (grow-only), cached filter
  float *pcm_dev = nullptr, *mono_dev = nullptr, *res_dev = nullptr;
  int64_t pcm_cap = 0, mono_cap = 0, res_cap = 0;
  double* taps_dev = nullptr;
  int taps_rate = 0;
  bp::ResamplePlan plan{};
  float* track_out = nullptr;  // [T, 88+88+264] staging when outputs are host pointers
  int64_t track_out_cap = 0;
  int64_t maps_rows = 0;       // rows of the maps a *_candidates call left in track_out (bp_track_maps); 0: none
  // device-side note candidates (note_device.hip): bitmap [T][11] + bend map [T][88] (bytes), stats, the bend tables
  float* nd_buf = nullptr;
  int64_t nd_cap = 0;          // floats
  float* nd_tables = nullptr;  // [88] int4 windows, [51] double Gaussian, then the stats record
  bp::FlacDeviceBuffers fd;            // flac_device.hip: the file's bytes, the frame lists, the scratch rows
  int* fd_status_host = nullptr;   // page-locked: the device decoder's error bits of the last call
  float* nd_stats_host = nullptr;  // page-locked copy of the stats record
  void* nd_stats_host_dev = nullptr;  // the same buffer as the device sees it
  bool nd_stats_ready = false;     // the device record holds its initial values (the export kernel leaves it so)

  // stage timing: a ring of event sets, one per chunk, averaged by bp_get_stage_ms
  static constexpr int kTimedRing = 128;
  static constexpr int kDomEvery = 4;
  static constexpr int kMaxMarks = 32;  // a stage may be launched in parts (the contour branch): its intervals are summed
  hipEvent_t ev[kTimedRing][kMaxMarks + 1] = {};
  // per ring slot (the mark sequence depends on the chunk: zpack only below half a window per CU, contour parts):
  // stage id of the interval between ev[c][i] and ev[c][i+1]; -1: not a stage (skipped)
  int seq[kTimedRing][kMaxMarks] = {};
  int n_seq[kTimedRing] = {};
  bool ev_valid = false;
  int64_t timed_chunks = 0;  // chunks recorded since the last bp_get_stage_ms
  int64_t dom_chunks = 0;    // chunks seen in BP_FLAG_TIME_DOMINANT mode (every kDomEvery-th is recorded)
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
int upload(bp_handle h, const std::vector<float>& host, float** dev);
int alloc(bp_handle h, float** p, int64_t floats);
int grow(bp_handle h, float** buf, int64_t* cap, int64_t need);
int run_chunk(bp_handle h, const float* audio_dev, int n, float* note_dev, float* onset_dev, float* contour_dev);
int wait_stream(bp_handle h);
}  // namespace bp
