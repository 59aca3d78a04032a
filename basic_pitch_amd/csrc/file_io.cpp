// Files on the host alone: a file's bytes into a caller's buffer (O_DIRECT where the file system takes it), a new file that
// never overwrites, the stem of a path, messages that name two paths, and the thread's last error (bp_files_last_error) that
// wav_file.cpp, note_writers.cpp and the file job (file_pipeline.cpp) set.  Nothing here calls the device library.
#include <atomic>
#include <cerrno>
#include <cstdlib>
#include <cstring>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "file_host.h"

namespace bp_file {

thread_local std::string g_file_error;

namespace {
std::atomic<int64_t> g_direct_reads{0};  // files whose bytes came in by O_DIRECT since the library was loaded
}  // namespace

// A file's bytes into a page-locked buffer.  `direct`: O_DIRECT — the storage device's DMA writes straight into the
// page-locked buffer the GPU's copy engine reads from; the page cache is bypassed, so a file crosses host DRAM twice (device
// write, PCIe read) instead of four times (page-cache fill, the copy out of it: read + write, PCIe read) and no core copies
// it (host DRAM bandwidth is the first resource an 8-GPU file job runs out of).  O_DIRECT wants the buffer, the
// offset and the length aligned to the logical block size: the pooled buffers are page-aligned, the length is rounded up
// to 4 KiB (the read stops at the end of the file).  A file system that refuses O_DIRECT (tmpfs, some overlays: EINVAL at
// open or at the first read) is read through the page cache as before.
bool read_file_into(const std::string& path, const std::function<void*(size_t)>& ensure, size_t& n, bool direct, bool* was_direct) {
  n = 0;
  int fd = -1;
#ifdef O_DIRECT
  if (direct) fd = open(path.c_str(), O_RDONLY | O_CLOEXEC | O_DIRECT);
#endif
  bool is_direct = fd >= 0;
  if (fd < 0) fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd < 0) {
    g_file_error = path + " is not a file path.";
    return false;
  }
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
    g_file_error = path + " is not a file path.";
    close(fd);
    return false;
  }
  const size_t size = (size_t)st.st_size;
  constexpr size_t kBlock = 4096;
  const size_t want = is_direct ? ((size + kBlock - 1) / kBlock) * kBlock : size;
  uint8_t* dst = static_cast<uint8_t*>(ensure(want ? want : 1));
  if (!dst) {
    close(fd);
    return false;
  }
  while (n < size) {
    // direct: n stays a multiple of the block size until the file's end (a short read ends the loop or the file)
    const ssize_t got = read(fd, dst + n, want - n);
    if (got < 0 && errno == EINTR) continue;
    if (got < 0 && is_direct && errno == EINVAL && n == 0) {  // the file system takes the flag at open and refuses the read
      close(fd);
      fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
      is_direct = false;
      if (fd < 0) {
        g_file_error = path + " is not a file path.";
        return false;
      }
      continue;
    }
    if (got < 0) {
      g_file_error = path + ": " + std::strerror(errno);
      close(fd);
      return false;
    }
    if (got == 0) break;  // shorter than fstat said: what is there
    n += (size_t)got;
    if (is_direct && (n % kBlock) != 0) break;  // the file's tail
  }
  if (n > size) n = size;
  close(fd);
  if (is_direct) g_direct_reads.fetch_add(1, std::memory_order_relaxed);
  if (was_direct) *was_direct = is_direct;
  return true;
}

// inference.py:401-404: never overwrite.  O_EXCL makes the existence check and the creation one step (two processes
// writing into the same directory cannot both win), and a short or failed write removes the partial file, so that a retry
// does not find a corpse and report "already exists".
bool write_new_file(const std::string& path, const void* data, size_t n) {
  const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0666);
  if (fd < 0) {
    g_file_error = errno == EEXIST ? path + " already exists and would be overwritten." : "cannot write " + path + ": " + std::strerror(errno);
    return false;
  }
  const uint8_t* p = static_cast<const uint8_t*>(data);
  size_t done = 0;
  while (done < n) {
    const ssize_t w = write(fd, p + done, n - done);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) {
      g_file_error = "cannot write " + path + ": " + std::strerror(errno);
      close(fd);
      unlink(path.c_str());
      return false;
    }
    done += (size_t)w;
  }
  if (close(fd) != 0) {
    g_file_error = "cannot write " + path + ": " + std::strerror(errno);
    unlink(path.c_str());
    return false;
  }
  return true;
}

std::string stem_of(const std::string& path) {
  const size_t slash = path.find_last_of('/');
  std::string base = slash == std::string::npos ? path : path.substr(slash + 1);
  const size_t dot = base.find_last_of('.');
  if (dot != std::string::npos && dot != 0) base.erase(dot);  // os.path.splitext
  return base;
}

// A report's message field holds 239 characters.  A message that names two paths keeps its wording whatever their
// length: a path that does not fit is shortened to "..." + its last characters (the file name stays), so that the reason
// ("same file stem", "already exists") is never cut off.
namespace {
constexpr size_t kMessageChars = sizeof(bp_file_report::message) - 1;

std::string path_tail(const std::string& p, size_t n) {
  if (p.size() <= n) return p;
  return n <= 3 ? p.substr(p.size() - n) : "..." + p.substr(p.size() - (n - 3));
}
}  // namespace

std::string two_path_message(const std::string& t0, const std::string& p0, const std::string& t1, const std::string& p1,
                             const std::string& t2) {
  const size_t fixed = t0.size() + t1.size() + t2.size();
  if (fixed + p0.size() + p1.size() <= kMessageChars) return t0 + p0 + t1 + p1 + t2;
  const size_t room = kMessageChars > fixed ? kMessageChars - fixed : 0;
  size_t n0 = room / 2, n1 = room - n0;  // a path shorter than its half leaves the rest to the other
  if (p0.size() < n0) {
    n1 += n0 - p0.size();
    n0 = p0.size();
  } else if (p1.size() < n1) {
    n0 += n1 - p1.size();
    n1 = p1.size();
  }
  return t0 + path_tail(p0, n0) + t1 + path_tail(p1, n1) + t2;
}

}  // namespace bp_file

using namespace bp_file;

extern "C" {

const char* bp_files_last_error(void) { return g_file_error.c_str(); }

int64_t bp_files_direct_reads(void) { return g_direct_reads.load(std::memory_order_relaxed); }

// The pipeline's file reader on its own, into ordinary page-aligned host memory (no device needed): the file's length, a
// 64-bit FNV-1a of its bytes and whether O_DIRECT was really used — what the CPU tests compare with Python's read.
int64_t bp_files_read_probe(const char* path, int direct_io, uint64_t* fnv1a, int* used_direct) {
  if (!path) {
    g_file_error = "bp_files_read_probe: null path";
    return BP_ERR_INVALID_ARG;
  }
  void* mem = nullptr;
  size_t n = 0;
  bool was = false;
  const bool ok = read_file_into(std::string(path), [&](size_t bytes) -> void* {
    if (posix_memalign(&mem, 4096, bytes) != 0) {
      mem = nullptr;
      g_file_error = "bp_files_read_probe: out of memory";
    }
    return mem;
  }, n, direct_io != 0, &was);
  if (!ok) {
    std::free(mem);
    return BP_ERR_BAD_AUDIO;
  }
  uint64_t h = 1469598103934665603ull;
  const uint8_t* p = static_cast<const uint8_t*>(mem);
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
  std::free(mem);
  if (fnv1a) *fnv1a = h;
  if (used_direct) *used_direct = was ? 1 : 0;
  return (int64_t)n;
}

}  // extern "C"
