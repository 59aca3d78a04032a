// Note events -> the bytes of a .csv and of a Standard MIDI File, on the host alone: bp_notes_to_csv, bp_notes_to_midi and the
// writers of the file job (file_pipeline.cpp).
//
// The writers restate, byte for byte, what the Python side of this package writes (basic_pitch_amd/midi.py — itself
// pinned to pretty_midi + mido's layout by tests/golden/midi — and inference.save_note_events): tests/test_file_pipeline.py
// compares them on the reference-generated note fixtures without a GPU.
//   basic_pitch/inference.py:409-428 the csv writer, 586 the pretty_midi write
//   basic_pitch/note_creation.py:222-267 note_events_to_midi, 270-286 drop_overlapping_pitch_bends
#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstring>
#include <map>

#include "file_host.h"

namespace bp_file {

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// repr(float) of CPython (float_repr_style "short"): the shortest digit string that round-trips, fixed notation while
// -4 < decimal point position <= 16, else d.ddde+XX with at least two exponent digits; ".0" behind integral values
void py_float_repr(double v, std::string& out) {
  if (std::isnan(v)) {
    out += "nan";
    return;
  }
  if (std::isinf(v)) {
    out += v < 0 ? "-inf" : "inf";
    return;
  }
  char buf[40];
  auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific);  // shortest round-trip digits
  std::string s(buf, r.ptr);
  const bool neg = s[0] == '-';
  if (neg) s.erase(0, 1);
  const size_t epos = s.find('e');
  std::string digits = s.substr(0, epos);
  const int exp10 = std::stoi(s.substr(epos + 1));
  digits.erase(std::remove(digits.begin(), digits.end(), '.'), digits.end());
  const int decpt = exp10 + 1;  // value = 0.DIGITS x 10^decpt
  if (neg) out += '-';
  const int nd = (int)digits.size();
  if (decpt > -4 && decpt <= 16) {
    if (decpt <= 0) {
      out += "0.";
      out.append((size_t)-decpt, '0');
      out += digits;
    } else if (decpt >= nd) {
      out += digits;
      out.append((size_t)(decpt - nd), '0');
      out += ".0";
    } else {
      out.append(digits, 0, (size_t)decpt);
      out += '.';
      out.append(digits, (size_t)decpt, std::string::npos);
    }
  } else {
    out += digits[0];
    if (nd > 1) {
      out += '.';
      out.append(digits, 1, std::string::npos);
    }
    const int e = decpt - 1;
    out += 'e';
    out += e < 0 ? '-' : '+';
    const int ae = e < 0 ? -e : e;
    if (ae < 10) out += '0';
    out += std::to_string(ae);
  }
}

// velocity = int(np.round(127 * amplitude)) with amplitude a float32 scalar: float32 product, round half to even
int velocity_of(float amplitude) { return (int)std::nearbyintf(127.0f * amplitude); }

}  // namespace

// inference.save_note_events: csv.writer rows start, end, pitch, velocity, *bends with "\r\n" line ends
void notes_csv(const bp_note_event* ev, int64_t n, const int32_t* bends, std::string& out) {
  out += "start_time_s,end_time_s,pitch_midi,velocity,pitch_bend\r\n";
  for (int64_t i = 0; i < n; ++i) {
    py_float_repr(ev[i].start_s, out);
    out += ',';
    py_float_repr(ev[i].end_s, out);
    out += ',';
    out += std::to_string(ev[i].pitch_midi);
    out += ',';
    out += std::to_string(velocity_of(ev[i].amplitude));
    for (int32_t k = 0; bends && k < ev[i].n_bends; ++k) {  // bends may be NULL (no pitch bends), as in notes_midi
      out += ',';
      out += std::to_string(bends[ev[i].bend_offset + k]);
    }
    out += "\r\n";
  }
}

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// note events -> Standard MIDI File bytes: note_creation.note_events_to_midi + midi.PrettyMIDI.to_bytes
void put_vlq(std::vector<uint8_t>& d, int64_t v) {
  uint8_t tmp[5];
  int k = 0;
  tmp[k++] = (uint8_t)(v & 0x7F);
  v >>= 7;
  while (v) {
    tmp[k++] = (uint8_t)((v & 0x7F) | 0x80);
    v >>= 7;
  }
  while (k) d.push_back(tmp[--k]);
}
void put_chunk(std::vector<uint8_t>& out, const char* tag, const std::vector<uint8_t>& data) {
  out.insert(out.end(), tag, tag + 4);
  const uint32_t n = (uint32_t)data.size();
  out.push_back((uint8_t)(n >> 24)), out.push_back((uint8_t)(n >> 16)), out.push_back((uint8_t)(n >> 8)), out.push_back((uint8_t)n);
  out.insert(out.end(), data.begin(), data.end());
}

struct MidiNote {
  double start, end;
  int pitch, vel;
  int64_t first_bend, n_bends;  // into the flat tick / time arrays
};

}  // namespace

bool notes_midi(const bp_note_event* ev, int64_t n, const int32_t* bends, bool multiple_pitch_bends, double tempo,
                std::vector<uint8_t>& out) {
  const int resolution = 220;
  const double tick_scale = 60.0 / (tempo * resolution);
  auto ticks_of = [&](double t) -> int64_t { return t > 0 ? (int64_t)std::nearbyint(t / tick_scale) : 0; };

  // drop_overlapping_pitch_bends: sorted(events) (tuple order: start, end, pitch, amplitude), bends dropped from any two
  // notes that overlap in time
  std::vector<int64_t> order((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
  std::vector<char> keep_bends((size_t)n, 1);
  if (!multiple_pitch_bends) {
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
      if (ev[a].start_s != ev[b].start_s) return ev[a].start_s < ev[b].start_s;
      if (ev[a].end_s != ev[b].end_s) return ev[a].end_s < ev[b].end_s;
      if (ev[a].pitch_midi != ev[b].pitch_midi) return ev[a].pitch_midi < ev[b].pitch_midi;
      return ev[a].amplitude < ev[b].amplitude;
    });
    for (int64_t i = 0; i + 1 < n; ++i)
      for (int64_t j = i + 1; j < n; ++j) {
        if (ev[order[(size_t)j]].start_s >= ev[order[(size_t)i]].end_s) break;
        keep_bends[(size_t)order[(size_t)i]] = keep_bends[(size_t)order[(size_t)j]] = 0;
      }
  }
  // pitch bends of all notes: ticks = round(b * 4096 / 3) clipped to [-8192, 8191], times = linspace(start, end, n)
  std::vector<int64_t> bend_tick;
  std::vector<double> bend_time;
  std::vector<MidiNote> notes((size_t)n);
  for (int64_t q = 0; q < n; ++q) {
    const bp_note_event& e = ev[order[(size_t)q]];
    MidiNote& m = notes[(size_t)q];
    m.start = e.start_s, m.end = e.end_s, m.pitch = e.pitch_midi, m.vel = velocity_of(e.amplitude);
    m.first_bend = (int64_t)bend_tick.size();
    m.n_bends = (bends && keep_bends[(size_t)order[(size_t)q]]) ? e.n_bends : 0;
    const double step = m.n_bends > 1 ? (e.end_s - e.start_s) / (double)(m.n_bends - 1) : 0.0;
    for (int64_t k = 0; k < m.n_bends; ++k) {
      int64_t t = (int64_t)std::nearbyint((double)((int64_t)bends[e.bend_offset + k] * 4096) / 3.0);
      t = t > 8191 ? 8191 : (t < -8192 ? -8192 : t);
      bend_tick.push_back(t);
      bend_time.push_back((m.n_bends > 1 && k == m.n_bends - 1) ? e.end_s : (double)k * step + e.start_s);
    }
  }
  // instruments: one, or (multiple_pitch_bends) one per note number in order of first appearance
  std::vector<std::vector<int64_t>> members;
  if (n > 0) {
    if (multiple_pitch_bends) {
      std::map<int, size_t> slot;
      for (int64_t q = 0; q < n; ++q) {
        auto it = slot.find(notes[(size_t)q].pitch);
        if (it == slot.end()) {
          slot[notes[(size_t)q].pitch] = members.size();
          members.emplace_back();
          it = slot.find(notes[(size_t)q].pitch);
        }
        members[it->second].push_back(q);
      }
    } else {
      members.emplace_back();
      for (int64_t q = 0; q < n; ++q) members[0].push_back(q);
    }
  }

  std::vector<std::vector<uint8_t>> tracks;
  {  // timing track: set_tempo, time_signature 4/4 at tick 0, end_of_track one tick later
    const int tempo_us = (int)(6e7 / (60.0 / (tick_scale * resolution)));
    std::vector<uint8_t> t = {0x00, 0xFF, 0x51, 0x03, (uint8_t)(tempo_us >> 16), (uint8_t)(tempo_us >> 8), (uint8_t)tempo_us,
                              0x00, 0xFF, 0x58, 0x04, 0x04, 0x02, 0x18, 0x08, 0x01, 0xFF, 0x2F, 0x00};
    tracks.push_back(std::move(t));
  }
  struct Ev {
    int64_t tick, key;
    int note, velo;  // -1: not a note event
    uint8_t status, d1;
    int d2;          // -1: one data byte
  };
  for (size_t inst = 0; inst < members.size(); ++inst) {
    static const int channels[15] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15};
    const int ch = channels[inst % 15];
    std::vector<Ev> e;
    e.push_back(Ev{0, (int64_t)6 << 16, -1, -1, (uint8_t)(0xC0 | ch), 4 /* Electric Piano 1 */, -1});
    for (int64_t q : members[inst]) {
      const MidiNote& m = notes[(size_t)q];
      e.push_back(Ev{ticks_of(m.start), ((int64_t)10 << 16) + m.pitch * 256 + m.vel, m.pitch, m.vel, (uint8_t)(0x90 | ch),
                     (uint8_t)m.pitch, m.vel});
      e.push_back(Ev{ticks_of(m.end), ((int64_t)10 << 16) + m.pitch * 256, m.pitch, 0, (uint8_t)(0x90 | ch), (uint8_t)m.pitch, 0});
    }
    for (int64_t q : members[inst]) {
      const MidiNote& m = notes[(size_t)q];
      for (int64_t k = 0; k < m.n_bends; ++k) {
        const int64_t b = bend_tick[(size_t)(m.first_bend + k)], v14 = b + 8192;
        e.push_back(Ev{ticks_of(bend_time[(size_t)(m.first_bend + k)]), ((int64_t)7 << 16) + b, -1, -1, (uint8_t)(0xE0 | ch),
                       (uint8_t)(v14 & 0x7F), (int)(v14 >> 7)});
      }
    }
    std::stable_sort(e.begin(), e.end(), [](const Ev& a, const Ev& b) { return a.tick != b.tick ? a.tick < b.tick : a.key < b.key; });
    // pretty_midi's fix-up: a note-on directly followed by the same pitch's note-off at the same tick is swapped (decided
    // on the sorted order as it was; the swaps cannot overlap)
    std::vector<size_t> sw;
    for (size_t k = 0; k + 1 < e.size(); ++k)
      if (e[k].tick == e[k + 1].tick && e[k].note >= 0 && e[k].note == e[k + 1].note && e[k].velo != 0 && e[k + 1].velo == 0)
        sw.push_back(k);
    for (size_t k : sw) std::swap(e[k], e[k + 1]);
    std::vector<uint8_t> d;
    d.reserve(e.size() * 4 + 8);
    int64_t last = 0;
    int running = -1;
    for (const Ev& x : e) {
      if (x.tick - last < 0 || x.tick - last >= ((int64_t)1 << 28)) {
        g_file_error = "MIDI delta time out of range";
        return false;
      }
      put_vlq(d, x.tick - last);
      last = x.tick;
      if (x.status != running) d.push_back(x.status);
      running = x.status;
      d.push_back(x.d1);
      if (x.d2 >= 0) d.push_back((uint8_t)x.d2);
    }
    d.push_back(0x01), d.push_back(0xFF), d.push_back(0x2F), d.push_back(0x00);  // end of track, one tick later
    tracks.push_back(std::move(d));
  }
  out.clear();
  std::vector<uint8_t> hd = {0x00, 0x01, (uint8_t)(tracks.size() >> 8), (uint8_t)tracks.size(), (uint8_t)(resolution >> 8),
                             (uint8_t)resolution};
  put_chunk(out, "MThd", hd);
  for (const auto& t : tracks) put_chunk(out, "MTrk", t);
  return true;
}

}  // namespace bp_file

using namespace bp_file;

extern "C" {

int64_t bp_notes_to_midi(const bp_note_event* events, int64_t n_events, const int32_t* bends, int multiple_pitch_bends,
                         double midi_tempo, uint8_t* out, int64_t capacity) {
  if (n_events < 0 || (n_events && !events) || !(midi_tempo > 0)) {
    g_file_error = "bp_notes_to_midi: bad arguments";
    return BP_ERR_INVALID_ARG;
  }
  std::vector<uint8_t> bytes;
  if (!notes_midi(events, n_events, bends, multiple_pitch_bends != 0, midi_tempo, bytes)) return BP_ERR_INVALID_ARG;
  if (out && (int64_t)bytes.size() <= capacity) std::memcpy(out, bytes.data(), bytes.size());
  return (int64_t)bytes.size();
}

int64_t bp_notes_to_csv(const bp_note_event* events, int64_t n_events, const int32_t* bends, char* out, int64_t capacity) {
  if (n_events < 0 || (n_events && !events)) {
    g_file_error = "bp_notes_to_csv: bad arguments";
    return BP_ERR_INVALID_ARG;
  }
  std::string s;
  notes_csv(events, n_events, bends, s);
  if (out && (int64_t)s.size() <= capacity) std::memcpy(out, s.data(), s.size());
  return (int64_t)s.size();
}

}  // extern "C"
