// C ABI of libbasicpitch_amd.so (include/basic_pitch_amd.h): the handle's lifecycle (bp_create uploads what
// weight_pack.hip packs, then allocates the HBM workspace: init_device; the handle's buffers own that memory, so bp_destroy
// is a delete), the stage orchestration of a chunk (run_chunk), bp_infer*, the per-stage test hook and stage timing.
//
// Replaces, for the hot path only, what the reference delegates to TensorFlow / onnxruntime /
// TFLite / CoreML behind basic_pitch/inference.py:71-182 (Model) and the window loop of
// run_inference (inference.py:282-315).
#include <cmath>
#include <cstring>
#include <ctime>

#include "bp_context.h"
#include "cqt_planes.h"
#include "launch_plan.h"
#include "weight_pack.h"

namespace bp {
// the onset branch: the wave-private march on 16x16x32.  A/B builds only: BP_ONSET=march32 selects the 32x32x16 form of
// the march, BP_ONSET=ring the workgroup kernel.
static void launch_onset(const uint32_t* zp, const float* note, const void* wfrag, const float* wf32, const void* w16,
                         float* onset, int n_windows, int n_cu, bool weights_have_lo, hipStream_t stream) {
#ifdef BP_AB_KERNELS
  static const int kind = [] {
    const char* e = ab_env("BP_ONSET");
    return e && std::strcmp(e, "ring") == 0 ? 2 : (e && std::strcmp(e, "march32") == 0 ? 1 : 0);
  }();
  if (kind == 1) {
    launch_onset_march(zp, note, wfrag, wf32, onset, n_windows, n_cu, weights_have_lo, stream);
    return;
  }
  if (kind == 2) {
    launch_onset_branch(zp, note, wfrag, wf32, onset, n_windows, n_cu, weights_have_lo, stream);
    return;
  }
#endif
  (void)wfrag;
  launch_onset_march16(zp, note, w16, wf32, onset, n_windows, n_cu, weights_have_lo, stream);
}
// contour conv2: the tap projection on the matrix cores (round 6).  A/B builds only: BP_CONV2=valu selects the round-2 kernel.
static void launch_conv2(const float* c1, const float* w2, const void* wproj, float bias, float* contour, int n_windows,
                         int n_cu, bool weights_have_lo, hipStream_t stream) {
#ifdef BP_AB_KERNELS
  static const bool valu = [] {
    const char* e = ab_env("BP_CONV2");
    return e && std::strcmp(e, "valu") == 0;
  }();
  if (valu) {
    launch_contour_conv2(c1, w2, bias, contour, n_windows, n_cu, stream);
    return;
  }
#endif
  (void)w2;
  launch_contour_conv2_proj(c1, wproj, bias, contour, n_windows, n_cu, weights_have_lo, stream);
}
// the note branch: the wave-private march on 16x16x32 (round 6).  A/B builds only: BP_NOTE=march32 selects the 32x32x16 form.
static void launch_note(const float* contour, const void* wfrag, const void* w16, const float* wf32, float* note, int n_windows,
                        int n_cu, bool weights_have_lo, hipStream_t stream) {
#ifdef BP_AB_KERNELS
  static const bool march32 = [] {
    const char* e = ab_env("BP_NOTE");
    return e && std::strcmp(e, "march32") == 0;
  }();
  if (march32) {
    launch_note_march(contour, wfrag, wf32, note, n_windows, weights_have_lo, stream);
    return;
  }
#endif
  (void)wfrag;
  launch_note_march16(contour, w16, wf32, note, n_windows, n_cu, weights_have_lo, stream);
}
}  // namespace bp

using namespace bp;

std::atomic<int64_t> bp::g_live_device_bytes{0};

namespace {

thread_local std::string g_create_error;

// Everything bp_create puts on the device: the stream, the operand tables, the workspace of `cap` windows.
// workspace_bytes is the sum of the tables and of what `ws` allocates.
int init_device(bp_handle h, const PackedWeights& pw) {
  BP_HIP(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
  h->stream = h->own_stream;
  for (auto& [field, bytes] : pw.tables) {
    BP_HIP((h->*field).upload(bytes.data(), bytes.size()));
    h->workspace_bytes += bytes.size();
  }
  auto ws = [h](auto& buf, int64_t n) {
    h->workspace_bytes += n * sizeof(*buf);
    return buf.reserve((size_t)n);
  };
  const int64_t cap = h->cap;
  BP_HIP(ws(h->audio, cap * (int64_t)h->win_len));
  BP_HIP(ws(h->pyr, cap * h->pyr_stride));
  BP_HIP(ws(h->lp, cap * kFrames * (int64_t)h->n_bins + 4));
  BP_HIP(ws(h->c1, cap * 8 * kPlaneC));
  BP_HIP(ws(h->contour, cap * kPlaneC));
  BP_HIP(ws(h->n1, cap * 32 * kPlaneN));
  BP_HIP(ws(h->note, cap * kPlaneN));
  BP_HIP(ws(h->o1, cap * 32 * kPlaneN));
  BP_HIP(ws(h->onset, cap * kPlaneN));
  BP_HIP(ws(h->zp, cap * (int64_t)kZWin));
  BP_HIP(ws(h->c1s, cap * (int64_t)kC1Win));
  // pad frames / pad words of zp are zero for good: the fused filterbank writes only the words that carry bins
  BP_HIP(hipMemset(h->zp, 0, (size_t)cap * kZWin * sizeof(uint32_t)));
  BP_HIP(hipMemset(h->c1s, 0, (size_t)cap * kC1Win * sizeof(float)));  // pad bins stay zero
  if (!(h->flags & BP_FLAG_F32_MFMA)) {
    // f16 planes of a chunk (an even count); zeroed once: the slack behind a level's reflect padding is read (and
    // discarded or masked) but never written, and has to stay finite
    const int64_t pl_n = (cap * planes_elements_per_window(h->ext) + 1) / 2 * 2;
    BP_HIP(ws(h->planes, pl_n));
    BP_HIP(hipMemset(h->planes, 0, (size_t)pl_n * sizeof(uint16_t)));
  }
  BP_HIP(h->mm.reserve((size_t)cap * 2));
  BP_HIP(h->fb_scratch.reserve(filterbank_scratch_floats((int)cap)));
  if (h->flags & (BP_FLAG_STAGE_TIMING | BP_FLAG_TIME_DOMINANT))
    for (auto& row : h->ev)
      for (auto& e : row) BP_HIP(hipEventCreate(&e));
  if (h->flags & BP_FLAG_BLOCKING_WAIT) BP_HIP(hipEventCreateWithFlags(&h->done, hipEventBlockingSync | hipEventDisableTiming));
  return BP_OK;
}

// The rim of contour conv1: the register-resident march (309-bin CQT), the round-3 GEMM for the extended 44.1 kHz mode
// (its 160 z bins per side would need 120 VGPRs of weights) and, in the A/B library, on BP_RIM=gemm.
static void launch_rim(bp_handle h, const uint32_t* zp, float* c1, int n, bool wlo, hipStream_t s) {
  static const bool gemm = [] {
    const char* e = ab_env("BP_RIM");
    return e && std::strcmp(e, "gemm") == 0;
  }();
  if (h->ext || gemm || !h->d_d1_wrimm)
    launch_contour_conv1_rim(zp, h->d_d1_wrim, h->d_d1_bias.as<float>(), c1, n, h->n_cu, wlo, h->ext, s);
  else
    launch_contour_conv1_rim_march(zp, h->d_d1_wrimm, h->d_d1_bias.as<float>(), c1, n, h->n_cu, wlo, s);
}

// conv2 inside the interior march (the default of the 309-bin path): the march leaves partial sums of conv2 instead of c1,
// in the exact-f32 path's c1 plane (idle here; launch_plan.h kCfWin), and contour_conv2_finish_kernel takes the place of the
// projection kernel.  The extended mode keeps the unfused pair; A/B library only: BP_CONV2=unfused (and valu, and
// BP_CONV1=rounds, whose kernels need c1) select it for the default mode.
static bool contour_fused(bp_handle h) {
  static const bool unfused = [] {
    const char* e = ab_env("BP_CONV2");
    return e && (std::strcmp(e, "unfused") == 0 || std::strcmp(e, "valu") == 0);
  }();
  return !h->ext && !unfused && contour_conv1_use_march();
}

// The interior of contour conv1: the vertical march.  A/B library only: the round-2 folded kernel on BP_CONV1=rounds.
static void launch_conv1_interior(bp_handle h, const uint32_t* zp, float* c1, int n, bool wlo, hipStream_t s) {
#ifdef BP_AB_KERNELS
  if (!contour_conv1_use_march()) {
    launch_contour_conv1_folded(zp, h->d_d1_wfold, h->d_d1_bias.as<float>(), c1, n, h->n_cu, wlo, s);
    return;
  }
#endif
  if (contour_fused(h))
    launch_contour_conv1_march(zp, h->d_d1_wmarch, h->d_d1_bias.as<float>(), h->c1, h->d_d2_w.as<float>(), n, h->n_cu, wlo, s);
  else
    launch_contour_conv1_march(zp, h->d_d1_wmarch, h->d_d1_bias.as<float>(), c1, nullptr, n, h->n_cu, wlo, s);
}

// contour conv2 of a handle: the finisher behind the fused march, or launch_conv2 on c1
static void launch_conv2_of(bp_handle h, float* contour, int n, bool wlo, hipStream_t s) {
  if (contour_fused(h))
    launch_contour_conv2_finish(h->c1s, h->c1, h->d_d2_wproj, h->b_contour2, contour, n, h->n_cu, wlo, s);
  else
    launch_conv2(h->c1s, h->d_d2_w.as<float>(), h->d_d2_wproj, h->b_contour2, contour, n, h->n_cu, wlo, s);
}

// Offset of pyramid level k >= 1 in a window's fp32 pyramid row (the extended mode's level 1 is the 22.05 kHz signal itself).
static int64_t pyr_level_off(bp_handle h, int k) {
  return h->ext ? ((k == 1) ? 0 : kAudioN + pyr_off(k - 1)) : pyr_off(k);
}

}  // namespace

namespace bp {

// One chunk (n <= cap) of windows already resident at `audio_dev`; outputs to device pointers.
int run_chunk(bp_handle h, const float* audio_dev, int n, float* note_dev, float* onset_dev,
              float* contour_dev) {
  hipStream_t s = h->stream;
  const bool timing = (h->flags & BP_FLAG_STAGE_TIMING) != 0;
  // BP_FLAG_TIME_DOMINANT: events only around the dominant kernel, on every fourth chunk (an event record between two
  // kernels keeps the second from starting under the first's tail: a pair per chunk cost 0.75 against 0.71 ms per step
  // at B = 256, round 5; sampled, the launches that are measured are the same and the rest run undisturbed)
  const bool dom = !timing && (h->flags & BP_FLAG_TIME_DOMINANT) && !(h->flags & BP_FLAG_F32_MFMA) &&
                   (h->dom_chunks++ % bp_context::kDomEvery) == 0;
  const bool wlo = !(h->flags & BP_FLAG_BF16_WEIGHTS);  // conv weights carry an f16 lo part
  int e = dom ? -1 : 0;  // index of the last event recorded
  const int ring_slot = (int)(h->timed_chunks % bp_context::kTimedRing);
  hipEvent_t* ev = h->ev[ring_slot];
  int* seq = h->seq[ring_slot];
  if (timing) BP_HIP(hipEventRecord(ev[0], s));
  // dominant-kernel timing: one (begin, end) pair per launch of the kernel; the interval between two pairs is no stage
#define BP_DOM_BEGIN()                                \
  do {                                                \
    if (dom) {                                        \
      if (e >= 0) seq[e] = -1;                        \
      BP_HIP(hipEventRecord(ev[e + 1], s));           \
      ++e;                                            \
    }                                                 \
  } while (0)
#define BP_DOM_END(id)                                \
  do {                                                \
    if (dom) {                                        \
      seq[e] = (id);                                  \
      BP_HIP(hipEventRecord(ev[e + 1], s));           \
      ++e;                                            \
    }                                                 \
  } while (0)
  // closes the interval of stage `id` (the kernels launched since the previous mark)
#define BP_MARK(id)                                \
  do {                                             \
    if (timing) {                                  \
      seq[e] = (id);                               \
      BP_HIP(hipEventRecord(ev[++e], s));          \
    }                                              \
  } while (0)
  bool zp_done = false;
  if (h->flags & BP_FLAG_F32_MFMA) {
    launch_pyramid(audio_dev, h->pyr, h->d_lowpass.as<float>(), n, s);
    BP_MARK(BP_STAGE_PYRAMID);
    launch_filterbank(audio_dev, h->pyr, h->d_fb_bfrag.as<float>(), h->d_sqrt_len.as<float>(), h->lp, h->mm, h->fb_scratch, n,
                      h->kc, h->n_cu, s);
    BP_MARK(BP_STAGE_FILTERBANK);
  } else {
    launch_pyramid_planes(audio_dev, h->win_len, h->planes, h->d_pl_tfrag, n, h->n_cu, h->ext, s);
    BP_MARK(BP_STAGE_PYRAMID);
    // with at least half a window per CU the kernel also normalises / BatchNorms / splits its windows (`zp` complete)
    zp_done = launch_filterbank_planes(h->planes, audio_dev, h->win_len, h->d_pl_bfrag, h->d_pl_bin_k.as<float>(), h->lp,
                                       h->fb_scratch, h->zp, n, h->kc, h->n_cu, h->ext, s);
    BP_MARK(BP_STAGE_FILTERBANK);
  }
  if (h->flags & BP_FLAG_F32_MFMA) {
    launch_contour1(h->lp, h->mm, h->d_c1_bfrag.as<float>(), h->d_c1_bias.as<float>(), h->c1, n, h->kc, h->n_cu, s);
    BP_MARK(BP_STAGE_CONTOUR1);
    launch_contour2(h->c1, h->d_w_contour2.as<float>(), h->b_contour2, contour_dev, n, s);
    BP_MARK(BP_STAGE_CONTOUR2);
    launch_note1(contour_dev, h->d_n1_bfrag.as<float>(), h->d_n1_bias.as<float>(), h->n1, n, h->n_cu, s);
    BP_MARK(BP_STAGE_NOTE1);
    launch_note2(h->n1, h->d_w_note2.as<float>(), h->b_note2, note_dev, n, s);
    BP_MARK(BP_STAGE_NOTE2);
    launch_onset1(h->lp, h->mm, h->d_o1_bfrag.as<float>(), h->d_o1_bias.as<float>(), h->o1, n, h->kc, h->n_cu, s);
    BP_MARK(BP_STAGE_ONSET1);
    launch_onset2(note_dev, h->o1, h->d_w_onset2.as<float>(), h->b_onset2, onset_dev, n, s);
    BP_MARK(BP_STAGE_ONSET2);
  } else {
    if (!zp_done) {
      // fewer windows than CUs: the filterbank left per-tile extrema, folded here by every workgroup for itself
      launch_zpack_partials(h->lp, h->fb_scratch, filterbank_planes_partials(h->ext), h->zp, n, h->kc, h->n_bins, s);
      BP_MARK(BP_STAGE_ZPACK);
    }
    const uint32_t* zp = h->zp;
    launch_rim(h, zp, h->c1s, n, wlo, s);
    BP_MARK(BP_STAGE_CONTOUR_CONV1_EDGE);
    BP_DOM_BEGIN();
    launch_conv1_interior(h, zp, h->c1s, n, wlo, s);
    BP_DOM_END(BP_STAGE_CONTOUR_CONV1);
    BP_MARK(BP_STAGE_CONTOUR_CONV1);
    launch_conv2_of(h, contour_dev, n, wlo, s);
    BP_MARK(BP_STAGE_CONTOUR_CONV2);
    launch_note(contour_dev, h->d_note_wfrag, h->d_note_w16, h->d_note_wf32.as<float>(), note_dev, n, h->n_cu, wlo, s);
    BP_MARK(BP_STAGE_NOTE);
    launch_onset(zp, note_dev, h->d_onset_wfrag, h->d_onset_wf32.as<float>(), h->d_onset_w16, onset_dev, n, h->n_cu, wlo, s);
    BP_MARK(BP_STAGE_ONSET);
  }
#undef BP_MARK
#undef BP_DOM_BEGIN
#undef BP_DOM_END
  if (timing || dom) {
    h->n_seq[ring_slot] = e < 0 ? 0 : e;
    h->timed_chunks++;
  }
  BP_HIP(hipGetLastError());
  return BP_OK;
}


// end of a host-blocking call: spin on the stream (lowest latency) or, with BP_FLAG_BLOCKING_WAIT, give the core to another
// worker thread while the device works.  hipEventSynchronize on a hipEventBlockingSync event does not do that here: measured
// on the MI355X box its user time equals its wall time (tools/experiments/host_cpu.py — the runtime polls the signal), so
// the wait is a query after 20, 40, then every 80 us with the thread asleep in between (a call of a few ms ends ~0.1 ms late).
int wait_stream(bp_handle h) {
  if (h->done) {
    BP_HIP(hipEventRecord(h->done, h->stream));
    for (long ns = 20000;;) {
      const hipError_t e = hipEventQuery(h->done);
      if (e == hipSuccess) break;
      if (e != hipErrorNotReady) BP_HIP(e);
      const timespec ts{0, ns};
      nanosleep(&ts, nullptr);
      if (ns < 80000) ns *= 2;
    }
  } else {
    BP_HIP(hipStreamSynchronize(h->stream));
  }
  return BP_OK;
}

}  // namespace bp

extern "C" {

const char* bp_version(void) { return "basic_pitch_amd 0.1.0 (gfx950)"; }

// Number of HIP devices this process sees (0 without a GPU or a HIP runtime).
int bp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

const char* bp_last_error(bp_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int bp_create(const void* weights, size_t nbytes, int device_ordinal, unsigned flags,
              int64_t max_windows_hint, bp_handle* out) {
  if (!out) {
    g_create_error = "bp_create: out is NULL";
    return BP_ERR_INVALID_ARG;
  }
  *out = nullptr;
  // windows per chunk: the per-window kernels put the window index in gridDim.y (<= 65535) and several launch helpers
  // count items in 32-bit; 16384 windows (3 GB of workspace) is far beyond where a larger chunk still helps
  if (max_windows_hint > BP_MAX_WINDOWS_PER_CHUNK) {
    g_create_error = "bp_create: max_windows_hint exceeds BP_MAX_WINDOWS_PER_CHUNK (16384); larger batches are chunked "
                     "inside bp_infer, pass 0 for the default of 256";
    return BP_ERR_INVALID_ARG;
  }
  PackedWeights pw;
  if (int rc = pack_weights(weights, nbytes, flags, pw, g_create_error)) return rc;

  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    g_create_error = "bp_create: no HIP device visible (this library has no CPU path)";
    return BP_ERR_NO_DEVICE;
  }
  if (device_ordinal < 0 || device_ordinal >= n_dev) {
    g_create_error = "bp_create: device_ordinal out of range";
    return BP_ERR_INVALID_ARG;
  }
  hipDeviceProp_t prop;
  if (hipSetDevice(device_ordinal) != hipSuccess || hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) {
    g_create_error = "bp_create: hipSetDevice / hipGetDeviceProperties failed";
    return BP_ERR_NO_DEVICE;
  }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_create_error = std::string("bp_create: device is ") + prop.gcnArchName +
                     ", this library only carries gfx950 (MI355X) code objects";
    return BP_ERR_NO_DEVICE;
  }

  bp_handle h = new bp_context();
  h->device = device_ordinal;
  h->flags = (flags & BP_FLAG_F32_MFMA) ? (flags & ~BP_FLAG_BF16_WEIGHTS) : flags;
  h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  std::snprintf(h->arch, sizeof h->arch, "%s", prop.gcnArchName);
  h->cap = max_windows_hint > 0 ? max_windows_hint : 256;
  if (flags & BP_FLAG_EXT_CQT_44K) {
    if (flags & BP_FLAG_F32_MFMA) {
      g_create_error = "bp_create: BP_FLAG_EXT_CQT_44K is not available on the exact-f32 path (BP_FLAG_F32_MFMA)";
      delete h;
      return BP_ERR_UNSUPPORTED;
    }
    h->ext = true;
    h->win_len = kAudioNExt;
    h->hop = 2 * BP_HOP_SIZE;
    h->lead = BP_OVERLAP_LEN;
    h->n_bins = kBinsExt;
    h->rate = 2 * BP_AUDIO_SAMPLE_RATE;
    h->pyr_stride = kPyrStrideExt;
  }
  h->kc = pw.kc;
  h->b_contour2 = pw.b_contour2;
  h->b_note2 = pw.b_note2;
  h->b_onset2 = pw.b_onset2;
  if (const char* es = ab_env("BP_RESAMPLE"))  // A/B runs: the resampler's simpler kernels (bit-identical results)
    h->resample_mode = std::strcmp(es, "plain") == 0 ? 1 : std::strcmp(es, "tiled") == 0 ? 2 : 0;

  if (int rc = init_device(h, pw)) {
    g_create_error = h->err;
    delete h;
    return rc;
  }
  *out = h;
  return BP_OK;
}

void bp_destroy(bp_handle h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  delete h;
}

int bp_set_stream(bp_handle h, void* hip_stream) {
  if (!h) return BP_ERR_INVALID_ARG;
  hipStream_t next = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->own_stream;
  if (next == h->stream) return BP_OK;
  // One workspace per handle (pyr, lp, zp, c1s, staging buffers): work still queued on the previous stream must
  // finish before work on the new stream may touch it.  Order the two streams with an event instead of a host sync.
  BP_HIP(hipSetDevice(h->device));
  hipEvent_t ev;
  BP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, h->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(next, ev, 0);
  (void)hipEventDestroy(ev);  // released once the recorded work completes
  BP_HIP(e);
  h->stream = next;
  return BP_OK;
}

int bp_synchronize(bp_handle h) {
  if (!h) return BP_ERR_INVALID_ARG;
  BP_HIP(hipSetDevice(h->device));
  BP_HIP(hipStreamSynchronize(h->stream));
  return BP_OK;
}

int bp_get_info(bp_handle h, bp_info* out) {
  if (!h || !out) return BP_ERR_INVALID_ARG;
  out->device_ordinal = h->device;
  out->compute_units = h->n_cu;
  out->max_windows = h->cap;
  out->workspace_bytes = h->workspace_bytes;
  std::memset(out->arch, 0, sizeof out->arch);
  std::snprintf(out->arch, sizeof out->arch, "%s", h->arch);
  return BP_OK;
}

int bp_infer_async(bp_handle h, const float* audio_dev, int64_t n_windows, float* note_dev,
                   float* onset_dev, float* contour_dev) {
  if (!h) return BP_ERR_INVALID_ARG;
  if (n_windows < 0 || (n_windows > 0 && (!audio_dev || !note_dev || !onset_dev || !contour_dev))) {
    h->err = "bp_infer: null pointer or negative window count";
    return BP_ERR_INVALID_ARG;
  }
  BP_HIP(hipSetDevice(h->device));
  for (int64_t w0 = 0; w0 < n_windows; w0 += h->cap) {
    const int n = (int)((n_windows - w0) < h->cap ? (n_windows - w0) : h->cap);
    int rc = run_chunk(h, audio_dev + w0 * h->win_len, n, note_dev + w0 * kPlaneN, onset_dev + w0 * kPlaneN,
                       contour_dev + w0 * kPlaneC);
    if (rc) return rc;
  }
  return BP_OK;
}

int bp_infer(bp_handle h, const float* audio, int64_t n_windows, float* note, float* onset,
             float* contour, int mem_kind) {
  if (!h) return BP_ERR_INVALID_ARG;
  if (mem_kind == BP_MEM_DEVICE) {
    int rc = bp_infer_async(h, audio, n_windows, note, onset, contour);
    if (rc) return rc;
    BP_HIP(hipStreamSynchronize(h->stream));
    return BP_OK;
  }
  if (mem_kind != BP_MEM_HOST) {
    h->err = "bp_infer: unknown mem_kind";
    return BP_ERR_INVALID_ARG;
  }
  if (n_windows < 0 || (n_windows > 0 && (!audio || !note || !onset || !contour))) {
    h->err = "bp_infer: null pointer or negative window count";
    return BP_ERR_INVALID_ARG;
  }
  BP_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  for (int64_t w0 = 0; w0 < n_windows; w0 += h->cap) {
    const int n = (int)((n_windows - w0) < h->cap ? (n_windows - w0) : h->cap);
    BP_HIP(hipMemcpyAsync(h->audio, audio + w0 * h->win_len, (size_t)n * h->win_len * 4, hipMemcpyHostToDevice, s));
    int rc = run_chunk(h, h->audio, n, h->note, h->onset, h->contour);
    if (rc) return rc;
    BP_HIP(hipMemcpyAsync(note + w0 * kPlaneN, h->note, (size_t)n * kPlaneN * 4, hipMemcpyDeviceToHost, s));
    BP_HIP(hipMemcpyAsync(onset + w0 * kPlaneN, h->onset, (size_t)n * kPlaneN * 4, hipMemcpyDeviceToHost, s));
    BP_HIP(hipMemcpyAsync(contour + w0 * kPlaneC, h->contour, (size_t)n * kPlaneC * 4, hipMemcpyDeviceToHost, s));
    BP_HIP(hipStreamSynchronize(s));
  }
  return BP_OK;
}


void* bp_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

void bp_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int bp_get_stage_ms(bp_handle h, float* ms, int n) {
  if (!h || !ms || n < BP_N_STAGES) return BP_ERR_INVALID_ARG;
  if (!(h->flags & (BP_FLAG_STAGE_TIMING | BP_FLAG_TIME_DOMINANT)) || h->timed_chunks == 0) {
    h->err = "bp_get_stage_ms: handle was not created with BP_FLAG_STAGE_TIMING / BP_FLAG_TIME_DOMINANT or nothing ran yet";
    return BP_ERR_UNSUPPORTED;
  }
  BP_HIP(hipStreamSynchronize(h->stream));
  const int64_t cnt = h->timed_chunks < bp_context::kTimedRing ? h->timed_chunks : bp_context::kTimedRing;
  double acc[BP_N_STAGES] = {0};
  for (int64_t c = 0; c < cnt; ++c) {
    for (int i = 0; i < h->n_seq[c]; ++i) {
      float t = 0.f;
      if (h->seq[c][i] < 0) continue;
      BP_HIP(hipEventElapsedTime(&t, h->ev[c][i], h->ev[c][i + 1]));
      acc[h->seq[c][i]] += t;
    }
  }
  for (int i = 0; i < BP_N_STAGES; ++i) ms[i] = (float)(acc[i] / (double)cnt);
  h->timed_chunks = 0;
  h->dom_chunks = 0;  // the first chunk after a read-out is a sampled one
  return BP_OK;
}

int bp_pyramid_layout(int level, int64_t* offset, int64_t* length) {
  if (level < 1 || level > 8 || !offset || !length) return BP_ERR_INVALID_ARG;
  *offset = pyr_off(level);
  *length = level_len(level);
  return BP_OK;
}

int bp_run_stage(bp_handle h, int stage, const bp_stage_buffers* bf, int64_t n_windows) {
  if (!h || !bf || n_windows <= 0 || n_windows > (1 << 20)) return BP_ERR_INVALID_ARG;
  BP_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int n = (int)n_windows;
  auto need = [&](const void* p) { return p != nullptr; };
  const bool wlo = !(h->flags & BP_FLAG_BF16_WEIGHTS);
  bool ok = true;
  switch (stage) {
    case BP_STAGE_PYRAMID:
      if ((ok = need(bf->audio) && need(bf->pyr))) {
        if (h->flags & BP_FLAG_F32_MFMA) {
          launch_pyramid(bf->audio, bf->pyr, h->d_lowpass.as<float>(), n, s);
        } else {  // the planes pyramid, its levels converted to the fp32 rows the test compares
          if (n > h->cap) {
            h->err = "bp_run_stage: pyramid needs n_windows <= max_windows (internal planes buffer)";
            return BP_ERR_INVALID_ARG;
          }
          uint16_t* pl = h->planes;
          launch_pyramid_planes(bf->audio, h->win_len, pl, h->d_pl_tfrag, n, h->n_cu, h->ext, s);
          const int n_lev = h->ext ? kOctavesExt : kOctaves;
          for (int k = 1; k < n_lev; ++k) {
            launch_planes_unsplit(pl, k, bf->pyr + pyr_level_off(h, k), h->pyr_stride, n, h->ext, s);
          }
        }
      }
      break;
    case BP_STAGE_FILTERBANK:
      if ((ok = need(bf->audio) && need(bf->pyr) && need(bf->lp) && need(bf->mm))) {
        BP_HIP(h->fb_scratch.reserve(filterbank_scratch_floats(n)));
        if (h->flags & BP_FLAG_F32_MFMA)
          launch_filterbank(bf->audio, bf->pyr, h->d_fb_bfrag.as<float>(), h->d_sqrt_len.as<float>(), bf->lp, bf->mm,
                            h->fb_scratch, n, h->kc, h->n_cu, s);
        else {  // the given fp32 levels split into planes (test hook), then the planes filterbank
          if (n > h->cap) {
            h->err = "bp_run_stage: filterbank needs n_windows <= max_windows (internal planes buffer)";
            return BP_ERR_INVALID_ARG;
          }
          uint16_t* pl = h->planes;
          launch_planes_edge_rows(bf->audio, h->win_len, pl, n, h->ext, s);  // level 0: fp32, straight from the audio
          const int n_lev = h->ext ? kOctavesExt : kOctaves;
          for (int k = 1; k < n_lev; ++k) {
            launch_planes_split(bf->pyr + pyr_level_off(h, k), h->pyr_stride, k, pl, n, h->ext, s);
          }
          (void)launch_filterbank_planes(pl, bf->audio, h->win_len, h->d_pl_bfrag, h->d_pl_bin_k.as<float>(), bf->lp, h->fb_scratch, nullptr, n, h->kc, h->n_cu,
                                         h->ext, s);
          launch_mm_reduce(h->fb_scratch, bf->mm, n, filterbank_planes_partials(h->ext), s);
        }
      }
      break;
    case BP_STAGE_CONTOUR1:
      if ((ok = need(bf->lp) && need(bf->mm) && need(bf->c1)))
        launch_contour1(bf->lp, bf->mm, h->d_c1_bfrag.as<float>(), h->d_c1_bias.as<float>(), bf->c1, n, h->kc, h->n_cu, s);
      break;
    case BP_STAGE_CONTOUR2:
      if ((ok = need(bf->c1) && need(bf->contour)))
        launch_contour2(bf->c1, h->d_w_contour2.as<float>(), h->b_contour2, bf->contour, n, s);
      break;
    case BP_STAGE_NOTE1:
      if ((ok = need(bf->contour) && need(bf->n1)))
        launch_note1(bf->contour, h->d_n1_bfrag.as<float>(), h->d_n1_bias.as<float>(), bf->n1, n, h->n_cu, s);
      break;
    case BP_STAGE_NOTE2:
      if ((ok = need(bf->n1) && need(bf->note))) launch_note2(bf->n1, h->d_w_note2.as<float>(), h->b_note2, bf->note, n, s);
      break;
    case BP_STAGE_ONSET1:
      if ((ok = need(bf->lp) && need(bf->mm) && need(bf->o1)))
        launch_onset1(bf->lp, bf->mm, h->d_o1_bfrag.as<float>(), h->d_o1_bias.as<float>(), bf->o1, n, h->kc, h->n_cu, s);
      break;
    case BP_STAGE_ONSET2:
      if ((ok = need(bf->note) && need(bf->o1) && need(bf->onset)))
        launch_onset2(bf->note, bf->o1, h->d_w_onset2.as<float>(), h->b_onset2, bf->onset, n, s);
      break;
    case BP_STAGE_ZPACK:
      if ((ok = need(bf->lp) && need(bf->mm) && need(bf->zp))) launch_zpack(bf->lp, bf->mm, bf->zp, n, h->kc, h->n_bins, s);
      break;
    case BP_STAGE_CONTOUR:
      if ((ok = need(bf->zp) && need(bf->contour))) {
        if (n > h->cap) {
          h->err = "bp_run_stage: contour needs n_windows <= max_windows (internal c1 buffer)";
          return BP_ERR_INVALID_ARG;
        } else {
          launch_rim(h, bf->zp, h->c1s, n, wlo, s);
          launch_conv1_interior(h, bf->zp, h->c1s, n, wlo, s);
          launch_conv2_of(h, bf->contour, n, wlo, s);
        }
      }
      break;
    case BP_STAGE_NOTE:
      if ((ok = need(bf->contour) && need(bf->note)))
        launch_note(bf->contour, h->d_note_wfrag, h->d_note_w16, h->d_note_wf32.as<float>(), bf->note, n, h->n_cu, wlo, s);
      break;
    case BP_STAGE_ONSET:
      if ((ok = need(bf->zp) && need(bf->note) && need(bf->onset)))
        launch_onset(bf->zp, bf->note, h->d_onset_wfrag, h->d_onset_wf32.as<float>(), h->d_onset_w16, bf->onset, n, h->n_cu, wlo, s);
      break;
    default:
      h->err = "bp_run_stage: unknown stage";
      return BP_ERR_INVALID_ARG;
  }
  if (!ok) {
    h->err = "bp_run_stage: a buffer this stage needs is NULL";
    return BP_ERR_INVALID_ARG;
  }
  BP_HIP(hipGetLastError());
  BP_HIP(hipStreamSynchronize(s));
  return BP_OK;
}

// What the launchers of the default path decide for a chunk of n_windows windows on a device of n_cu compute units, from
// the functions they call themselves (launch_plan.h).  No handle, no device.
int bp_launch_plan(int64_t n_windows, int n_cu, unsigned flags, bp_launch_plan_out* out) {
  if (!out || n_windows <= 0 || n_windows > BP_MAX_WINDOWS_PER_CHUNK || n_cu <= 0 || n_cu > 4096) return BP_ERR_INVALID_ARG;
  if (flags & BP_FLAG_F32_MFMA) return BP_ERR_UNSUPPORTED;  // the exact-f32 path has launchers of its own
  const int n = (int)n_windows;
  const bool ext = (flags & BP_FLAG_EXT_CQT_44K) != 0;
  const PlGeo g = make_pl_geo(ext);
  std::memset(out, 0, sizeof *out);
  // pyramid
  out->pyramid_one_launch = pyramid_one_launch(n, n_cu, ext);
  out->pyramid_decimate_grid = out->pyramid_one_launch ? 0 : pyramid_decimate_grid((g.len[1] + kPlTileOut - 1) / kPlTileOut, n, n_cu);
  out->pyramid_decimate_grid_cap = pl_resident_waves(n_cu) / kPlDecimateWaves;
  // filterbank of run_chunk (zp given)
  out->filterbank_fused = filterbank_fused(true, n, n_cu);
  out->filterbank_grid = filterbank_grid(out->filterbank_fused != 0, n, n * g.n_levels * kPlTilesPerLevel, n_cu);
  // contour conv1: interior march, rim (the extended mode's rim is the GEMM, a workgroup per item: no decision)
  out->conv1_chunks = contour_march_chunks(n, n_cu);
  out->conv1_grid = contour_march_grid(n * out->conv1_chunks * kCmStrips, n_cu);
  out->conv1_prio = march_prio(kCmPrio, out->conv1_grid, n_cu);
  out->rim_march = !ext;
  if (!ext) {
    out->rim_items = n * kRmTiles;
    out->rim_per_side = rim_march_per_side(out->rim_items, n_cu);
    out->rim_items_max = rim_march_items_of(0, out->rim_items, out->rim_per_side);
    out->rim_items_min = rim_march_items_of(out->rim_per_side - 1, out->rim_items, out->rim_per_side);
    out->rim_ring = kRmRing;
  }
  // contour conv2
  out->conv2_slots = (int32_t)conv2_proj_slots(n_cu);
  for (int w0 = 0; w0 < n; w0 += kP2PerLaunch) {
    const Conv2ProjLaunch l = conv2_proj_launch(n, w0, n_cu);
    int32_t* dst = w0 == 0 ? &out->conv2_first_windows : &out->conv2_last_windows;
    dst[0] = l.n, dst[1] = l.n_groups, dst[2] = l.n_slabs, dst[3] = l.slab_rows, dst[4] = l.grid;
    if (w0 == 0) std::memcpy(&out->conv2_last_windows, dst, 5 * sizeof(int32_t));
    out->conv2_launches += 1;
    out->conv2_windows += l.n;
  }
  // conv2 in the march's epilogue (the 309-bin path's default) and its finisher
  out->conv2_fused = !ext;
  if (!ext) {
    const Conv2FinishLaunch l = conv2_finish_launch(n, n_cu);
    out->fused_cols = kCfCols, out->fused_seam_rows = kCfPrefRows, out->fused_term_rows = kCfTermRows;
    out->fused_window_floats = kCfWin;
    out->finish_slabs = l.n_slabs, out->finish_slab_rows = l.slab_rows, out->finish_grid = l.grid;
  }
  // note and onset marches
  out->note_grid = march_grid(n * kN16Strips, kN16MinFrames, kN16Waves, kN16Occ, n_cu);
  out->note_grid_cap = kN16Occ * n_cu;
  out->note_prio = march_prio(kN16Prio, out->note_grid, n_cu);
  out->note_aligned = march_aligned(out->note_grid * kN16Waves, n * kN16Strips, kN16Strips);
  out->note_share_spans_pairs = march_share_spans_pairs(out->note_grid * kN16Waves, n * kN16Strips, kN16Strips);
  out->onset_grid = march_grid(n * kO16Strips, kO16MinFrames, kO16Waves, kO16Occ, n_cu);
  out->onset_grid_cap = kO16Occ * n_cu;
  out->onset_prio = march_prio(kO16Prio, out->onset_grid, n_cu);
  out->onset_aligned = march_aligned(out->onset_grid * kO16Waves, n * kO16Strips, kO16Strips);
  out->onset_share_spans_pairs = march_share_spans_pairs(out->onset_grid * kO16Waves, n * kO16Strips, kO16Strips);
  return BP_OK;
}

#ifdef BP_AB_KERNELS
// The A/B library's test hook for leaks (declared nowhere: the tests name it): bytes of device memory the buffers of this
// process hold.  A counter of the library's own, because what the device reports as free moves with other processes' work.
int64_t bp_ab_live_device_bytes(void) { return g_live_device_bytes.load(); }
#endif

}  // extern "C"
