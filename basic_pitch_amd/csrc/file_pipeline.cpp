// Whole files, natively (round 4): decode -> device (downmix, resampling, CQT + CNN) -> note events -> .mid / .csv on C++
// worker threads, no Python in the loop.  The batch job of the reference is a Python loop over files
//   basic_pitch/inference.py:509-604 predict_and_save: predict() per file, then pretty_midi write (586) / csv writer (409-428)
//   basic_pitch/note_creation.py:52-116 model_output_to_notes
// and this package's Python pipeline (predict_and_save_many) was bound by the interpreter: 78 three-minute files per
// second against 2,600 per second of device capacity.  Here a worker thread owns a file from its bytes to
// its outputs; the GPU is a shared resource the workers queue for (one lane per handle), everything else runs in parallel.
//
// This file is the job alone: what it does on the host without a device lies in wav_file.cpp (RIFF/WAVE, RF64), pcm_file.cpp
// (AIFF, CAF, AU), adpcm_file.cpp (IMA ADPCM in WAV and CAF), note_writers.cpp (.csv / .mid bytes) and file_io.cpp (reading and
// writing files), declared in file_host.h.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/basic_pitch_amd_adpcm.h"
#include "../../include/basic_pitch_amd_flac_clips.h"
#include "adpcm_host.h"
#include "file_host.h"

extern "C" int bp_internal_flac_device_supported(const bp_flac_stream_layout* lay, size_t nbytes);  // flac_decode.cpp

namespace {

using namespace bp_file;

// ---------------------------------------------------------------------------------------------------------------------
// page-locked, grow-only: what a worker hands to / receives from the device goes by DMA without the runtime's staging copy.
// Page-locking tens of megabytes costs milliseconds, so a worker's buffers go back to a process-wide pool when it ends and
// the next bp_transcribe_files call starts from them (at most kPoolMax buffers are kept; the rest are released).
struct PinnedPool {
  static constexpr size_t kPoolMax = 192;              // buffers
  static constexpr size_t kPoolBytes = (size_t)2 << 30;  // and bytes kept between calls (16 workers of 3-minute files: ~1 GB)
  std::mutex mu;
  std::vector<std::pair<void*, size_t>> free_list;
  size_t pooled_bytes = 0;
  // the smallest pooled buffer of at least n bytes, else a new one
  std::pair<void*, size_t> take(size_t n) {
    {
      std::lock_guard<std::mutex> lk(mu);
      size_t best = free_list.size();
      for (size_t i = 0; i < free_list.size(); ++i)
        if (free_list[i].second >= n && (best == free_list.size() || free_list[i].second < free_list[best].second)) best = i;
      if (best != free_list.size()) {
        const auto b = free_list[best];
        free_list.erase(free_list.begin() + (long)best);
        pooled_bytes -= b.second;
        return b;
      }
    }
    const size_t want = n + n / 8 + 4096;
    return {bp_host_alloc(want), want};
  }
  void give(void* p, size_t cap) {
    if (!p) return;
    {
      std::lock_guard<std::mutex> lk(mu);
      if (free_list.size() < kPoolMax && pooled_bytes + cap <= kPoolBytes) {
        free_list.emplace_back(p, cap);
        pooled_bytes += cap;
        return;
      }
    }
    bp_host_free(p);
  }
};
PinnedPool g_pinned;

struct Pinned {
  void* p = nullptr;
  size_t cap = 0;
  bool ensure(size_t n) {
    if (n <= cap) return true;
    g_pinned.give(p, cap);
    p = nullptr, cap = 0;
    const auto b = g_pinned.take(n);
    if (!b.first) {
      g_file_error = "page-locked host allocation of " + std::to_string(b.second) + " bytes failed";
      return false;
    }
    p = b.first, cap = b.second;
    return true;
  }
  ~Pinned() { g_pinned.give(p, cap); }
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
};

// ---------------------------------------------------------------------------------------------------------------------
// What a file is and who decodes it: asked by the per-file route with the file's bytes and by clip_route with its headers.
// Pcm: AIFF / AIFF-C, CAF or AU (pcm_file.cpp), like Wav a header around samples the device converts as they are stored.
enum class Container { Neither, Wav, Flac, Pcm };

// from a file's first bytes (up to 12 of them; `size` is the file's)
Container sniff(const uint8_t* head, size_t size) {
  switch (pcm_container_of(head, size)) {
    case 0: break;
    case BP_CONTAINER_WAV: return Container::Wav;  // RIFF, RF64 or BW64
    default: return Container::Pcm;
  }
  if (size >= 4 && (std::memcmp(head, "fLaC", 4) == 0 || std::memcmp(head, "ID3", 3) == 0)) return Container::Flac;
  return Container::Neither;
}

// What a Wav or Pcm file holds, from its headers: samples the device converts as they are stored (format: their BP_PCM_*), or
// IMA ADPCM blocks (adpcm: BP_ADPCM_*, `ad` filled; RIFF/WAVE tag 0x11, CAF ima4), which the device expands itself
// (adpcm_device.hip).  The one walk behind clip_route and the per-file route.  False: g_file_error says why.
struct Samples {
  int channels = 0, sample_rate = 0, format = BP_PCM_F32, adpcm = 0;
  int64_t n_frames = 0;
  size_t data_pos = 0;
  bp_adpcm_layout ad{};
};

bool walk_samples(const ByteSource& src, Container kind, Samples& s) {
  s = Samples{};
  if (kind == Container::Wav) {
    WavInfo w;
    if (!wav_walk(src, w, s.data_pos)) return false;
    s.channels = w.channels, s.sample_rate = w.sample_rate, s.n_frames = w.n_frames, s.format = wav_pcm_format(w);
    if (w.tag != kWavTagIma) return true;
  } else {
    bp_pcm_file_layout lay;
    if (pcm_file_walk(src, lay)) {
      s.channels = lay.channels, s.sample_rate = lay.sample_rate, s.n_frames = lay.n_frames, s.format = lay.format;
      s.data_pos = (size_t)lay.data_start;
      return true;
    }
  }
  // blocks, not samples: the headers once more as adpcm_file.cpp reads them (a file that is no such file keeps its message)
  const std::string why = g_file_error;
  const int codec = adpcm_walk(src, s.ad);
  if (codec == 0) g_file_error = why;
  if (codec <= 0) return false;
  s.channels = s.ad.channels, s.sample_rate = s.ad.sample_rate, s.n_frames = s.ad.n_frames, s.format = BP_PCM_S16;
  s.data_pos = (size_t)s.ad.data_start, s.adpcm = codec;
  return true;
}

// FLAC: the file's BYTES go to the device and are decoded there (flac_device.hip) — no core-time per sample here, half
// the PCIe bytes of the PCM — unless the stream is one the device decoder leaves to the host (flac_decode.cpp
// bp_internal_flac_device_supported) or params.host_flac asks for the host decoder.  `bytes`: the file, or a prefix of it
// that holds the metadata.  Device and Host have `lay` filled, unless host_flac decided; Unparsed: bp_audio_last_error
// says why (a prefix may simply be too short).
enum class FlacDecoder { Device, Host, Unparsed };

FlacDecoder flac_decoder(bool host_flac, const uint8_t* bytes, size_t n, size_t file_size, bp_flac_stream_layout& lay) {
  if (host_flac) return FlacDecoder::Host;
  if (bp_flac_layout(bytes, n, &lay) != BP_OK) return FlacDecoder::Unparsed;
  return bp_internal_flac_device_supported(&lay, file_size) ? FlacDecoder::Device : FlacDecoder::Host;
}

// ---------------------------------------------------------------------------------------------------------------------
// Batches of short files (params.clip_batch > 0).  A worker claims a run of files, decides every file's
// route from its headers, and takes the short ones through one clips-events call per container and sample rate; every
// other file, and every file a call could not finish, goes the per-file route below, unchanged.
//
// What a worker holds is bounded whatever the caller asks for: a run has at most kClipBatchMax files, and the files of
// one lane acquisition have at most kClipBatchBytes of file bytes (the worker's page-locked batch buffer) and
// kClipBatchWindows windows (the lane's maps on the device: 142 rows of 440 floats a window); a run that passes either is
// taken in several parts.
constexpr int64_t kClipBatchMax = 1024;
constexpr size_t kClipBatchBytes = (size_t)64 << 20;
constexpr int64_t kClipBatchWindows = 1024;
constexpr size_t kClipAlign = 4096;  // a file's bytes start at a 4 KiB boundary of the batch buffer (O_DIRECT reads land there)
size_t slot_bytes(size_t size) { return (size + kClipAlign - 1) / kClipAlign * kClipAlign + kClipAlign; }

std::atomic<int64_t> g_batched{0};  // files whose outputs came from a batched call since the library was loaded

struct ClipFile {
  int route = 0;  // 0: the per-file route; 1: a batched PCM call; 2: a batched FLAC call; negative: a bp_status
  int channels = 0, sample_rate = 0, format = BP_PCM_F32;
  int adpcm = 0;  // route 1: BP_ADPCM_* of a file of IMA ADPCM blocks, which takes the batched ADPCM call; else 0
  int64_t n_frames = 0, windows = 0;
  size_t data_pos = 0;  // WAV, AIFF, CAF, AU: where the samples lie in the file
  // the calls of a part, one per key: the route, for IMA ADPCM with the codec and the channel count (one of each per call)
  int group() const { return adpcm ? 0x100 | adpcm | (channels << 16) : route; }
};

// the windows of n_frames frames at sample_rate at the lanes' geometry (no handle: that of the default mode)
int64_t clip_windows(bp_handle h, int64_t n_frames, int sample_rate) {
  return h ? bp_handle_track_n_windows(h, bp_handle_resampled_length(h, n_frames, sample_rate))
           : bp_track_n_windows(bp_resampled_length(n_frames, sample_rate));
}

// the jobs whose maps the host decodes (host_decode, or an onset threshold <= 0, with which every clip of a clips call has
// status 1): nothing of them is batched
bool host_decodes(const bp_transcribe_params& prm) { return prm.host_decode || !(prm.notes.onset_threshold > 0.0); }

// The one place that decides whether a batch takes a file, from its headers: the probe asks with an open file, a worker
// once with the open file (before it reads anything else) and once more with the bytes it then read.  What the file is and
// who decodes a FLAC stream are sniff's and flac_decoder's to say, as on the per-file route; here is what only a batch asks.
// A file whose channels or rate the clips calls would refuse (check_ingest: 1 - 64 channels, 1,000 - 768,000 Hz) keeps the
// per-file route, which reports it.  An error is set without the path.
int clip_route(const ByteSource& src, bp_handle h, const bp_transcribe_params& prm, ClipFile& c) {
  c = ClipFile{};
  uint8_t magic[12] = {0};
  if (src.size && !src.at(0, src.size < 12 ? src.size : 12, magic)) return c.route = BP_ERR_BAD_AUDIO;
  auto in_domain = [&]() { return c.channels >= 1 && c.channels <= 64 && c.sample_rate >= 1000 && c.sample_rate <= 768000; };
  const Container kind = sniff(magic, src.size);
  switch (kind) {
    case Container::Wav:
    case Container::Pcm: {  // samples, or IMA ADPCM blocks: short files of either are batched
      Samples sm;
      if (!walk_samples(src, kind, sm)) return c.route = BP_ERR_BAD_AUDIO;
      c.channels = sm.channels, c.sample_rate = sm.sample_rate, c.n_frames = sm.n_frames, c.format = sm.format;
      c.data_pos = sm.data_pos, c.adpcm = sm.adpcm;
      if (host_decodes(prm) || !in_domain() || src.size > kClipBatchBytes) return c.route = 0;
      c.windows = clip_windows(h, c.n_frames, c.sample_rate);  // a file without frames: a clip without rows
      return c.route = c.windows <= BP_FILES_CLIP_MAX_WINDOWS ? 1 : 0;
    }
    case Container::Flac: {
      if (host_decodes(prm) || prm.host_flac) return c.route = 0;  // before anything more of the file is read
      const bool host_flac = false;  // (returned above: flac_decoder never answers Host with `lay` unfilled here)
      // STREAMINFO lies in the metadata in front of the first frame: from memory as it is, from a file a prefix that grows
      // until the metadata fits in it (a parse that succeeds has read nothing behind the metadata)
      bp_flac_stream_layout lay;
      FlacDecoder dec = FlacDecoder::Unparsed;
      if (src.mem) {
        dec = flac_decoder(host_flac, src.mem, src.size, src.size, lay);
      } else {
        std::vector<uint8_t> head;
        for (size_t want = (size_t)64 << 10; dec == FlacDecoder::Unparsed; want *= 4) {
          const size_t n = want < src.size ? want : src.size;
          head.resize(n);
          if (!src.at(0, n, head.data())) return c.route = BP_ERR_BAD_AUDIO;
          dec = flac_decoder(host_flac, head.data(), n, src.size, lay);
          if (n == src.size) break;
        }
      }
      if (dec == FlacDecoder::Unparsed) {
        g_file_error = bp_audio_last_error();
        return c.route = BP_ERR_BAD_AUDIO;
      }
      c.channels = lay.channels, c.sample_rate = lay.sample_rate, c.n_frames = lay.n_frames, c.format = BP_PCM_S16;
      // the streams the device decoders leave to the host (bp_infer_flac; the clips call's scratch bound)
      if (dec != FlacDecoder::Device || (size_t)lay.audio_start >= src.size || src.size < 42) return c.route = 0;
      if (((lay.n_frames + lay.min_block - 1) / lay.min_block + 1) * lay.max_block > 8 * lay.n_frames + 2 * (int64_t)lay.max_block) return c.route = 0;
      if (!in_domain() || src.size > kClipBatchBytes) return c.route = 0;
      c.windows = clip_windows(h, c.n_frames, c.sample_rate);
      return c.route = c.windows >= 1 && c.windows <= BP_FILES_CLIP_MAX_WINDOWS ? 2 : 0;
    }
    case Container::Neither: break;
  }
  g_file_error = "not a WAV or FLAC file (the native pipeline reads RIFF/WAVE and FLAC)";
  return c.route = BP_ERR_BAD_AUDIO;
}

// the route of the file at `path`, read from its headers alone
int clip_route_of_path(const std::string& path, bp_handle h, const bp_transcribe_params& prm, ClipFile& c, size_t* size) {
  c = ClipFile{};
  const int fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
  struct stat st;
  if (fd < 0 || fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
    if (fd >= 0) close(fd);
    g_file_error = path + " is not a file path.";
    return c.route = BP_ERR_BAD_AUDIO;
  }
  ByteSource src;
  src.fd = fd, src.size = (size_t)st.st_size;
  if (size) *size = src.size;
  const int route = clip_route(src, h, prm, c);
  close(fd);
  return route;
}

// a clips-events call refused with "output buffers too small: N events and M bends" (the only place the interface gives the
// bend total): the capacities to ask with once more.  False: it refused for another reason, or the room was there.
bool grow_to_needed(const char* msg, int64_t& cap_ev, int64_t& cap_b) {
  long long need_ev = 0, need_b = 0;
  const char* p = msg ? std::strstr(msg, "output buffers too small: ") : nullptr;
  if (!p || std::sscanf(p, "output buffers too small: %lld events and %lld bends", &need_ev, &need_b) != 2) return false;
  if (need_ev <= cap_ev && need_b <= cap_b) return false;
  cap_ev = std::max<int64_t>(cap_ev, need_ev), cap_b = std::max<int64_t>(cap_b, need_b);
  return true;
}

// one worker per core this process may really use: a cgroup CPU quota (containers: 16 of a host's 256 hardware threads)
// counts, not the host's thread count — oversubscribed workers measured 25 % slower (the quota throttles every thread of
// the group, the ones feeding the GPU included)
int default_threads() {
  int n = (int)std::thread::hardware_concurrency();
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char quota[32];
    long period = 0;
    if (std::fscanf(f, "%31s %ld", quota, &period) == 2 && std::strcmp(quota, "max") != 0 && period > 0) {
      const long q = std::atol(quota) / period;
      if (q >= 1 && q < n) n = (int)q;
    }
    std::fclose(f);
  }
  return n < 1 ? 1 : n;
}

void set_report(bp_file_report* r, int status, const std::string& msg) {
  r->status = status;
  std::snprintf(r->message, sizeof r->message, "%s", msg.c_str());
}

void clear_report(bp_file_report* r) {  // everything but the status and the message
  r->n_note_events = 0, r->n_frames = 0;
  r->ms_read = r->ms_lane_wait = r->ms_device = r->ms_notes = r->ms_write = 0.0f;
}

struct Lap {  // lap(): milliseconds since the previous lap
  std::chrono::steady_clock::time_point clock = std::chrono::steady_clock::now();
  float operator()() {
    const auto t = std::chrono::steady_clock::now();
    const float ms = std::chrono::duration<float, std::milli>(t - clock).count();
    clock = t;
    return ms;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// One bp_transcribe_files call: what is constant for it or shared by its workers.
struct Job {
  bp_handle* handles;
  const char* const* paths;
  int64_t n_files;
  std::string out_dir;
  bp_transcribe_params prm;
  bp_file_report* reports;
  std::vector<char> dup;  // files whose stem an earlier file has: reported, never run
  // GPU lanes: a worker takes any free handle for the duration of its device calls
  std::mutex lane_mu;
  std::condition_variable lane_cv;
  std::vector<int> free_lanes;
  std::atomic<int64_t> next{0};  // the first file no worker has claimed

  std::string out_base(int64_t i) const { return out_dir + "/" + stem_of(paths[i]) + "_basic_pitch."; }
  // refuse before doing the work, like build_output_path
  bool outputs_exist(const std::string& base) const {
    struct stat st;
    return (prm.save_midi && stat((base + "mid").c_str(), &st) == 0) || (prm.save_notes && stat((base + "csv").c_str(), &st) == 0);
  }
  // rows of the maps of a file (every lane is of handles[0]'s mode)
  int64_t rows_of(int64_t n_frames, int sample_rate) const {
    return bp_handle_track_n_frames(handles[0], bp_handle_resampled_length(handles[0], n_frames, sample_rate));
  }
};

class Lane {  // a lane from its construction to release() or the end of the scope
 public:
  explicit Lane(Job& j) : job(j) {
    std::unique_lock<std::mutex> lk(job.lane_mu);
    job.lane_cv.wait(lk, [&] { return !job.free_lanes.empty(); });
    lane = job.free_lanes.back();
    job.free_lanes.pop_back();
  }
  ~Lane() { release(); }
  Lane(const Lane&) = delete;
  Lane& operator=(const Lane&) = delete;
  bp_handle handle() const { return job.handles[lane]; }
  void release() {
    if (lane < 0) return;
    {
      std::lock_guard<std::mutex> lk(job.lane_mu);
      job.free_lanes.push_back(lane);
    }
    job.lane_cv.notify_one();
    lane = -1;
  }

 private:
  Job& job;
  int lane = -1;
};

// One thread of the job and the buffers it owns.
class Worker {
 public:
  explicit Worker(Job& j) : job(j), prm(j.prm) {}
  void run();  // claim files until none is left

 private:
  struct Audio {  // what the device gets of one file
    const uint8_t* bytes = nullptr;  // the file
    size_t n_bytes = 0;
    bool flac_on_device = false;  // the device decodes `bytes`; else it gets `pcm`
    bool adpcm_on_device = false;  // IMA ADPCM: the device expands `bytes`
    const void* pcm = nullptr;
    int channels = 0, sample_rate = 0, format = BP_PCM_F32;
    int64_t n_frames = 0;
  };
  struct Maps {  // views of `maps` for a file of T rows
    float *note, *onset, *contour;
    // device-side candidates (the default): the same page-locked buffer holds the note map, the onset-peak bitmap
    // (T x 12 bytes) and, from a 16-byte boundary, the pitch-bend map (T x 88 bytes) instead of the onset / contour maps
    uint8_t* cand_bits;
    int8_t* bend_map;
    Maps(void* p, int64_t T)
        : note(static_cast<float*>(p)), onset(note + T * 88), contour(onset + T * 88), cand_bits(reinterpret_cast<uint8_t*>(onset)),
          bend_map(reinterpret_cast<int8_t*>(cand_bits + ((T * BP_NOTE_CAND_ROW_BYTES + 15) & ~(int64_t)15))) {}
  };
  struct Member {  // a file of a part
    int64_t index;
    ClipFile c;
    size_t size, offset, n_bytes;  // the file's size by its headers; where its bytes lie in `batch`; the bytes read
    int64_t rows;
  };
  struct Group {  // the files of one clips-events call: one container, one sample rate
    std::vector<size_t> members;
    std::vector<bp_note_event> events;
    std::vector<int32_t> bends;
    std::vector<int64_t> offsets;
    std::vector<int> status;
    int rc = BP_OK;
    float ms_device = 0.0f;
  };
  using Groups = std::map<std::pair<int, int>, Group>;  // by (ClipFile::group(), sample rate)

  // the per-file route: one file from its bytes to its outputs
  void one_file(int64_t i);
  bool host_flac_decode(const std::string& path, bp_file_report* rep, Audio& a);
  bool read_audio(const std::string& path, bp_file_report* rep, Audio& a);
  bool infer(const std::string& path, bp_file_report* rep, Audio& a, const Maps& m, int64_t T, bool& use_cand, Lap& lap);
  bool decode_notes(const std::string& path, bp_file_report* rep, const Maps& m, int64_t T, bool use_cand, int64_t& n_ev);
  bool write_outputs(const std::string& base, const bp_note_event* ev, int64_t n_ev, const int32_t* ev_bends);
  // the batch route: files join a part; one part is read, inferred in one lane acquisition and written
  void claim(int64_t i);
  void flush();
  void read_part(Groups& groups);
  void infer_group(bp_handle h, int key, int sample_rate, Group& g);
  void write_group(const Group& g, float ms_read, float ms_wait, Lap& lap);

  Job& job;
  const bp_transcribe_params& prm;
  Pinned file, decoded, maps;  // the file's bytes; PCM of a file decoded on the host; the three posteriorgrams
  std::vector<bp_note_event> events;
  std::vector<int32_t> bends;
  std::vector<uint8_t> midi;
  std::string csv;
  Pinned batch;  // the bytes of a part's short files, each in its slot
  std::vector<Member> part;
  std::vector<int64_t> later;  // files of the part that take the per-file route after all
  size_t part_bytes = 0;
  int64_t part_windows = 0;
};

// the host decoder (flac_decode.cpp): float32 samples in `decoded`
bool Worker::host_flac_decode(const std::string& path, bp_file_report* rep, Audio& a) {
  int bits = 0;
  if (bp_flac_info(a.bytes, a.n_bytes, &a.channels, &a.sample_rate, &bits, &a.n_frames) != BP_OK) {
    set_report(rep, BP_ERR_BAD_AUDIO, path + ": " + bp_audio_last_error());
    return false;
  }
  if (!decoded.ensure((size_t)(a.n_frames * a.channels) * sizeof(float) + 4)) {
    set_report(rep, BP_ERR_OUT_OF_MEMORY, path + ": " + g_file_error);
    return false;
  }
  int64_t got = 0;
  if (bp_flac_decode(a.bytes, a.n_bytes, static_cast<float*>(decoded.p), a.n_frames, &got) != BP_OK || got != a.n_frames) {
    set_report(rep, BP_ERR_BAD_AUDIO, path + ": " + bp_audio_last_error());
    return false;
  }
  a.pcm = decoded.p, a.format = BP_PCM_F32, a.flac_on_device = false;
  return true;
}

// the file's bytes in `file`, and what they hold
bool Worker::read_audio(const std::string& path, bp_file_report* rep, Audio& a) {
  if (!read_file_into(path, [&](size_t bytes) -> void* { return file.ensure(bytes) ? file.p : nullptr; }, a.n_bytes, prm.direct_io != 0)) {
    set_report(rep, BP_ERR_BAD_AUDIO, g_file_error);
    return false;
  }
  a.bytes = static_cast<const uint8_t*>(file.p);
  const Container kind = sniff(a.bytes, a.n_bytes);
  switch (kind) {
    case Container::Wav:
    case Container::Pcm: {
      ByteSource src;
      src.mem = a.bytes, src.size = a.n_bytes;
      Samples sm;
      if (!walk_samples(src, kind, sm)) {
        set_report(rep, BP_ERR_BAD_AUDIO, path + ": " + g_file_error);
        return false;
      }
      // the samples go to the device as the file stores them (bp_infer_pcm_raw converts there); IMA ADPCM blocks too
      // (bp_infer_adpcm expands them there), unless the job decodes on the host: then their int16 samples go
      a.channels = sm.channels, a.sample_rate = sm.sample_rate, a.n_frames = sm.n_frames, a.pcm = a.bytes + sm.data_pos;
      a.format = sm.format;
      if (!sm.adpcm) return true;
      if (!prm.host_decode) {
        a.adpcm_on_device = true;
        return true;
      }
      if (!decoded.ensure((size_t)(a.n_frames * a.channels) * sizeof(int16_t) + 4)) {
        set_report(rep, BP_ERR_OUT_OF_MEMORY, path + ": " + g_file_error);
        return false;
      }
      int16_t* pcm = static_cast<int16_t*>(decoded.p);
      if (sm.adpcm == BP_ADPCM_IMA_WAV) ima_wav_decode(a.bytes + sm.data_pos, (size_t)sm.ad.data_bytes, a.channels, sm.ad.block_bytes, a.n_frames, pcm);
      else ima4_decode(a.bytes + sm.data_pos, (size_t)sm.ad.data_bytes, a.channels, a.n_frames, pcm);
      a.pcm = pcm;
      return true;
    }
    case Container::Flac: {
      bp_flac_stream_layout lay;
      if (flac_decoder(prm.host_flac != 0, a.bytes, a.n_bytes, a.n_bytes, lay) != FlacDecoder::Device) return host_flac_decode(path, rep, a);
      a.flac_on_device = true;
      a.channels = lay.channels, a.sample_rate = lay.sample_rate, a.n_frames = lay.n_frames;
      return true;
    }
    case Container::Neither: break;
  }
  set_report(rep, BP_ERR_BAD_AUDIO, path + ": not a WAV or FLAC file (the native pipeline reads RIFF/WAVE and FLAC)");
  return false;
}

// the maps (or the candidates) of the file on a lane.  A FLAC stream the device decoder could not follow goes to the host
// decoder, which either decodes it or names the fault, and then once more to a lane as PCM.
bool Worker::infer(const std::string& path, bp_file_report* rep, Audio& a, const Maps& m, int64_t T, bool& use_cand, Lap& lap) {
  int8_t* bend_map = prm.notes.include_pitch_bends ? m.bend_map : nullptr;
  int rc = BP_OK;
  std::string err;
  for (int attempt = 0; attempt < 2; ++attempt) {
    Lane lane(job);
    rep->ms_lane_wait += lap();
    bp_handle h = lane.handle();
    rc = BP_OK;
    if (T > 0) {
      if (use_cand) {
        int status = 0;
        rc = a.flac_on_device    ? bp_infer_flac_candidates(h, a.bytes, a.n_bytes, &prm.notes, m.note, m.cand_bits, bend_map, &status)
             : a.adpcm_on_device ? bp_infer_adpcm_candidates(h, a.bytes, a.n_bytes, &prm.notes, m.note, m.cand_bits, bend_map, &status)
                                 : bp_infer_pcm_raw_candidates(h, a.pcm, a.format, a.n_frames, a.channels, a.sample_rate, &prm.notes,
                                                               m.note, m.cand_bits, bend_map, &status);
        if (rc == BP_OK && status != 0) {  // a NaN in the maps: numpy's rules need the maps themselves — they are
          use_cand = false;                // still on the device, the lane is still ours
          rc = bp_track_maps(h, T, m.note, m.onset, m.contour, BP_MEM_HOST);
        }
      } else {
        rc = a.flac_on_device    ? bp_infer_flac(h, a.bytes, a.n_bytes, m.note, m.onset, m.contour, BP_MEM_HOST)
             : a.adpcm_on_device ? bp_infer_adpcm(h, a.bytes, a.n_bytes, m.note, m.onset, m.contour, BP_MEM_HOST)
                                 : bp_infer_pcm_raw(h, a.pcm, a.format, a.n_frames, a.channels, a.sample_rate, m.note, m.onset, m.contour,
                                                    BP_MEM_HOST);
      }
      if (rc != BP_OK) err = bp_last_error(h);
    }
    lane.release();
    rep->ms_device += lap();
    if (!(a.flac_on_device && (rc == BP_ERR_BAD_AUDIO || rc == BP_ERR_UNSUPPORTED))) break;
    if (!host_flac_decode(path, rep, a)) return false;
    rep->ms_read += lap();
  }
  if (rc != BP_OK) set_report(rep, rc, path + ": " + err);
  return rc == BP_OK;
}

// the maps' note events in `events` / `bends`, once more with the room the decoder asks for
bool Worker::decode_notes(const std::string& path, bp_file_report* rep, const Maps& m, int64_t T, bool use_cand, int64_t& n_ev) {
  int64_t n_b = 0;
  int rc = BP_OK;
  size_t cap_ev = (size_t)std::max<int64_t>(256, T / 4), cap_b = (size_t)std::max<int64_t>(4096, 4 * T);
  for (int attempt = 0; attempt < 2; ++attempt) {
    events.resize(cap_ev), bends.resize(cap_b);
    rc = T <= 0 ? BP_OK
         : use_cand ? bp_notes_decode_candidates(m.note, m.cand_bits, prm.notes.include_pitch_bends ? m.bend_map : nullptr, T,
                                                 &prm.notes, events.data(), (int64_t)cap_ev, bends.data(), (int64_t)cap_b, &n_ev, &n_b)
                    : bp_notes_decode(m.note, m.onset, m.contour, T, &prm.notes, events.data(), (int64_t)cap_ev, bends.data(),
                                      (int64_t)cap_b, &n_ev, &n_b);
    if (rc == BP_OK || !((size_t)n_ev > cap_ev || (size_t)n_b > cap_b)) break;
    cap_ev = std::max(cap_ev, (size_t)n_ev), cap_b = std::max(cap_b, (size_t)n_b);
  }
  if (rc != BP_OK) set_report(rep, rc, path + ": " + bp_notes_last_error());
  return rc == BP_OK;
}

// base + "mid" / "csv" as the job asks for them; false: g_file_error says why
bool Worker::write_outputs(const std::string& base, const bp_note_event* ev, int64_t n_ev, const int32_t* ev_bends) {
  const int32_t* bp = prm.notes.include_pitch_bends ? ev_bends : nullptr;
  if (prm.save_midi && !(notes_midi(ev, n_ev, bp, prm.multiple_pitch_bends != 0, prm.midi_tempo, midi) &&
                         write_new_file(base + "mid", midi.data(), midi.size())))
    return false;
  if (!prm.save_notes) return true;
  csv.clear();
  notes_csv(ev, n_ev, bp, csv);
  return write_new_file(base + "csv", csv.data(), csv.size());
}

// The order of the checks: outputs exist, read, parse, device, decode, write.
void Worker::one_file(const int64_t i) {
  bp_file_report* rep = &job.reports[i];
  clear_report(rep);
  Lap lap;
  const std::string path = job.paths[i];
  const std::string base = job.out_base(i);
  if (job.outputs_exist(base)) {
    set_report(rep, BP_ERR_INVALID_ARG,
               two_path_message("", base + "*", " already exists and would be overwritten. Skipping output files for ", path, "."));
    return;
  }
  Audio a;
  if (!read_audio(path, rep, a)) return;
  const int64_t T = job.rows_of(a.n_frames, a.sample_rate);
  if (T > 0 && !maps.ensure((size_t)T * (88 + 88 + 264) * sizeof(float))) {
    set_report(rep, BP_ERR_OUT_OF_MEMORY, path + ": " + g_file_error);
    return;
  }
  const Maps m(maps.p, T);
  bool use_cand = !host_decodes(prm);
  rep->ms_read = lap();
  if (!infer(path, rep, a, m, T, use_cand, lap)) return;
  rep->n_frames = T;
  int64_t n_ev = 0;
  if (!decode_notes(path, rep, m, T, use_cand, n_ev)) return;
  rep->n_note_events = (int32_t)n_ev;
  rep->ms_notes = lap();
  if (!write_outputs(base, events.data(), n_ev, bends.data())) {
    set_report(rep, BP_ERR_INVALID_ARG, g_file_error);
    return;
  }
  rep->ms_write = lap();
  set_report(rep, BP_OK, "");
}

// ---- params.clip_batch > 0: runs of files, the short ones in batched calls ---------------------------------------------------

// the part's bytes into `batch`, and the files whose bytes confirm the route their headers gave into their groups
void Worker::read_part(Groups& groups) {
  if (!batch.ensure(part_bytes)) return;
  uint8_t* base = static_cast<uint8_t*>(batch.p);
  size_t at = 0;
  for (size_t k = 0; k < part.size(); ++k) {
    Member& m = part[k];
    m.offset = at;
    uint8_t* slot = base + at;
    const size_t room = slot_bytes(m.size);
    at += room;
    // (a file that grew since its headers were read does not fit its slot: the per-file route takes it)
    const bool ok = read_file_into(job.paths[m.index], [slot, room](size_t bytes) -> void* { return bytes <= room ? slot : nullptr; },
                                   m.n_bytes, prm.direct_io != 0);
    ByteSource src;
    src.mem = slot, src.size = m.n_bytes;
    const int route = m.c.route;
    if (!ok || clip_route(src, job.handles[0], prm, m.c) != route) continue;  // the bytes read decide, as the headers did
    m.rows = job.rows_of(m.c.n_frames, m.c.sample_rate);
    groups[{m.c.group(), m.c.sample_rate}].members.push_back(k);
  }
}

// one clips-events call over a group's files, once more if it asks for more room
void Worker::infer_group(bp_handle h, int key, int sample_rate, Group& g) {
  const bool flac = key == 2, adpcm = (key & 0x100) != 0;
  const uint8_t* base = static_cast<const uint8_t*>(batch.p);
  const int64_t n = (int64_t)g.members.size();
  std::vector<bp_clip> pcm_clips;
  std::vector<bp_flac_clip> flac_clips;
  std::vector<bp_adpcm_clip> adpcm_clips;
  int64_t rows = 0;
  for (size_t k : g.members) {
    const Member& m = part[k];
    rows += m.rows;
    if (flac) flac_clips.push_back(bp_flac_clip{base + m.offset, m.n_bytes});
    else if (adpcm) adpcm_clips.push_back(bp_adpcm_clip{base + m.offset, m.n_bytes});
    else pcm_clips.push_back(bp_clip{base + m.offset + m.c.data_pos, m.c.n_frames, m.c.format, m.c.channels});
  }
  g.offsets.assign((size_t)n + 1, 0), g.status.assign((size_t)n, 0);
  int64_t cap_ev = std::max<int64_t>(256, rows / 2), cap_b = std::max<int64_t>(4096, 8 * rows);
  for (int attempt = 0; attempt < 2; ++attempt) {
    g.events.resize((size_t)cap_ev), g.bends.resize((size_t)cap_b);
    g.rc = flac ? bp_infer_flac_clips_events(h, n, flac_clips.data(), sample_rate, &prm.notes, g.events.data(), cap_ev, g.bends.data(),
                                             cap_b, g.offsets.data(), g.status.data())
           : adpcm ? bp_infer_adpcm_clips_events(h, n, adpcm_clips.data(), &prm.notes, g.events.data(), cap_ev, g.bends.data(), cap_b,
                                                 g.offsets.data(), g.status.data())
                : bp_infer_clips_events(h, n, pcm_clips.data(), sample_rate, BP_MEM_HOST, &prm.notes, g.events.data(), cap_ev,
                                        g.bends.data(), cap_b, g.offsets.data(), g.status.data());
    if (g.rc != BP_ERR_INVALID_ARG || !grow_to_needed(bp_last_error(h), cap_ev, cap_b)) break;
  }
}

// The outputs of a group: nothing of a file is written before its events are final.  A call that failed as a whole and
// every clip whose status is not 0 are left to the per-file route, whose outputs and report are today's by construction.
void Worker::write_group(const Group& g, float ms_read, float ms_wait, Lap& lap) {
  std::vector<size_t> written;
  for (size_t q = 0; q < g.members.size(); ++q) {
    const Member& m = part[g.members[q]];
    if (g.rc != BP_OK || g.status[q] != 0) {
      later.push_back(m.index);
      continue;
    }
    bp_file_report* rep = &job.reports[m.index];
    clear_report(rep);
    const int64_t n_ev = g.offsets[q + 1] - g.offsets[q];
    rep->n_frames = m.rows, rep->n_note_events = (int32_t)n_ev;
    rep->ms_read = ms_read, rep->ms_lane_wait = ms_wait, rep->ms_device = g.ms_device;
    if (!write_outputs(job.out_base(m.index), g.events.data() + g.offsets[q], n_ev, g.bends.data())) {
      set_report(rep, BP_ERR_INVALID_ARG, g_file_error);
      continue;
    }
    set_report(rep, BP_OK, "");
    written.push_back(q);
  }
  const float ms_write = written.empty() ? 0.0f : lap() / (float)written.size();
  for (size_t q : written) job.reports[part[g.members[q]].index].ms_write = ms_write;
  g_batched.fetch_add((int64_t)written.size(), std::memory_order_relaxed);
}

// one part: its files' bytes, one lane acquisition, one call per group, the outputs; then the files left to the per-file route
void Worker::flush() {
  if (part.empty()) return;
  later.clear();
  Lap lap;
  Groups groups;
  read_part(groups);
  std::vector<char> in_group(part.size(), 0);
  for (const auto& kv : groups)
    for (size_t k : kv.second.members) in_group[k] = 1;
  for (size_t k = 0; k < part.size(); ++k)
    if (!in_group[k]) later.push_back(part[k].index);
  const size_t n_grouped = part.size() - later.size();
  const float ms_read = n_grouped ? lap() / (float)n_grouped : 0.0f;
  float ms_wait = 0.0f;
  if (n_grouped) {
    Lane lane(job);
    ms_wait = lap() / (float)n_grouped;
    for (auto& kv : groups) {
      infer_group(lane.handle(), kv.first.first, kv.first.second, kv.second);
      kv.second.ms_device = lap() / (float)kv.second.members.size();
    }
  }  // the lane goes back before anything is written
  for (const auto& kv : groups) write_group(kv.second, ms_read, ms_wait, lap);
  part.clear(), part_bytes = 0, part_windows = 0;
  std::sort(later.begin(), later.end());
  for (int64_t i : later) one_file(i);
}

// file i of a claimed run: into the part if its headers send it to a batch, else down the per-file route at once
void Worker::claim(const int64_t i) {
  Member m{i, ClipFile{}, 0, 0, 0, 0};
  // an output that exists is the per-file route's to report; so is every file the headers do not send to a batch
  if (job.outputs_exist(job.out_base(i)) || host_decodes(prm) || clip_route_of_path(job.paths[i], job.handles[0], prm, m.c, &m.size) <= 0) {
    one_file(i);
    return;
  }
  if (!part.empty() && (part_bytes + slot_bytes(m.size) > kClipBatchBytes + 2 * kClipAlign || part_windows + m.c.windows > kClipBatchWindows))
    flush();
  part_bytes += slot_bytes(m.size), part_windows += m.c.windows;
  part.push_back(m);
}

void Worker::run() {
  if (prm.clip_batch <= 0) {  // none of the batching code runs
    for (;;) {
      const int64_t i = job.next.fetch_add(1);
      if (i >= job.n_files) break;
      if (!job.dup[(size_t)i]) one_file(i);
    }
    return;
  }
  const int64_t step = std::min<int64_t>(prm.clip_batch, kClipBatchMax);
  for (;;) {
    const int64_t lo = job.next.fetch_add(step);
    if (lo >= job.n_files) break;
    const int64_t hi = std::min(job.n_files, lo + step);
    for (int64_t i = lo; i < hi; ++i)
      if (!job.dup[(size_t)i]) claim(i);
    flush();
  }
}

}  // namespace

extern "C" {

int64_t bp_files_batched(void) { return g_batched.load(std::memory_order_relaxed); }

// The route every file would take in a job with params->clip_batch > 0, from its headers alone: the function the workers ask.
int bp_files_batch_probe(bp_handle* handles, int n_handles, const char* const* paths, int64_t n_files,
                         const bp_transcribe_params* params, int32_t* route) {
  if (n_handles < 0 || (n_handles > 0 && (!handles || !handles[0])) || n_files < 0 || (n_files && (!paths || !route)) || !params) {
    g_file_error = "bp_files_batch_probe: null pointer or bad count";
    return BP_ERR_INVALID_ARG;
  }
  if (params->clip_batch < 0) {
    g_file_error = "bp_files_batch_probe: negative clip_batch";
    return BP_ERR_INVALID_ARG;
  }
  for (int64_t i = 0; i < n_files; ++i) {
    ClipFile c;
    if (!paths[i]) {
      g_file_error = "bp_files_batch_probe: null path";
      return BP_ERR_INVALID_ARG;
    }
    // (a job whose maps the host decodes opens no file here: the per-file route reads and reports every one of them)
    route[i] = host_decodes(*params) ? 0 : clip_route_of_path(paths[i], n_handles > 0 ? handles[0] : nullptr, *params, c, nullptr);
  }
  return BP_OK;
}

void bp_files_release_buffers(void) {
  std::vector<std::pair<void*, size_t>> all;
  {
    std::lock_guard<std::mutex> lk(g_pinned.mu);
    all.swap(g_pinned.free_list);
    g_pinned.pooled_bytes = 0;
  }
  for (auto& b : all) bp_host_free(b.first);
}

void bp_transcribe_params_default(bp_transcribe_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  bp_note_params_default(&p->notes);
  p->midi_tempo = 120.0;
  p->save_midi = 1;
  p->save_notes = 1;
}

int bp_transcribe_files(bp_handle* handles, int n_handles, const char* const* paths, int64_t n_files, const char* out_dir,
                        const bp_transcribe_params* params, bp_file_report* reports) {
  if (!handles || n_handles < 1 || n_files < 0 || (n_files && !paths) || !out_dir || !params || (n_files && !reports)) {
    g_file_error = "bp_transcribe_files: null pointer or bad count";
    return BP_ERR_INVALID_ARG;
  }
  if (params->clip_batch < 0) {
    g_file_error = "bp_transcribe_files: negative clip_batch";
    return BP_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_handles; ++i)
    if (!handles[i]) {
      g_file_error = "bp_transcribe_files: null handle";
      return BP_ERR_INVALID_ARG;
    }
  // every lane must be of the same mode: a file's output buffers are sized from handles[0] and the device call runs on
  // whichever lane is free (a default and an EXT_CQT_44K handle would disagree on rate and frame count)
  for (int i = 1; i < n_handles; ++i) {
    const int64_t probe = 1 << 20;
    if (bp_handle_sample_rate(handles[i]) != bp_handle_sample_rate(handles[0]) ||
        bp_handle_track_n_frames(handles[i], probe) != bp_handle_track_n_frames(handles[0], probe) ||
        bp_handle_resampled_length(handles[i], probe, 44100) != bp_handle_resampled_length(handles[0], probe, 44100)) {
      g_file_error = "bp_transcribe_files: the handles are of different modes (sample rate / frame geometry)";
      return BP_ERR_INVALID_ARG;
    }
  }
  struct stat st;
  if (stat(out_dir, &st) != 0 || !S_ISDIR(st.st_mode)) {
    g_file_error = std::string(out_dir) + " is not a directory.";
    return BP_ERR_INVALID_ARG;
  }
  Job job;
  job.handles = handles, job.paths = paths, job.n_files = n_files, job.out_dir = out_dir, job.prm = *params, job.reports = reports;
  for (int i = 0; i < n_handles; ++i) job.free_lanes.push_back(i);
  // two inputs with the same stem would write the same files: the first in input order wins (inference.py:401-404)
  job.dup.assign((size_t)n_files, 0);
  std::map<std::string, int64_t> seen;
  for (int64_t i = 0; i < n_files; ++i) {
    const auto first = seen.emplace(stem_of(paths[i]), i);
    if (first.second) continue;
    job.dup[(size_t)i] = 1;
    clear_report(&reports[i]);
    set_report(&reports[i], BP_ERR_INVALID_ARG,
               two_path_message("the outputs of ", paths[i], " would overwrite those of ", paths[first.first->second], " (same file stem)"));
  }
  int n_threads = job.prm.threads > 0 ? job.prm.threads : default_threads();
  n_threads = n_threads < 1 ? 1 : (n_threads > 64 ? 64 : n_threads);
  if (n_threads > n_files) n_threads = (int)(n_files > 0 ? n_files : 1);
  std::vector<std::thread> pool;
  for (int t = 1; t < n_threads; ++t) pool.emplace_back([&job] { Worker(job).run(); });
  Worker(job).run();
  for (auto& t : pool) t.join();
  return BP_OK;
}

}  // extern "C"
