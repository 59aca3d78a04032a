// The weights blob -> the operand tables of a handle: blob parsing, the f16 conversions and the packing of every
// kernel's operands, all on the host.  pack_weights is the one entry point (weight_pack.h); bp_create uploads what it
// returns.  A .hip file because the packers use bp_common.h's __host__ __device__ tap helpers.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "weight_pack.h"

using namespace bp;

namespace {

struct Tensor {
  const float* data = nullptr;
  uint32_t ndim = 0, dims[4] = {1, 1, 1, 1}, count = 0;
};

struct Blob {
  std::vector<std::pair<std::string, Tensor>> t;
  const Tensor* find(const char* name) const {
    for (auto& kv : t)
      if (kv.first == name) return &kv.second;
    return nullptr;
  }
};

bool parse_blob(const void* weights, size_t nbytes, Blob& out, std::string& err) {
  const uint8_t* p = static_cast<const uint8_t*>(weights);
  if (!p || nbytes < 16 || std::memcmp(p, "BPAMDW01", 8) != 0) {
    err = "weights blob: bad magic (expected BPAMDW01)";
    return false;
  }
  uint32_t version, n;
  std::memcpy(&version, p + 8, 4);
  std::memcpy(&n, p + 12, 4);
  if (version != 1 || n > 1024 || nbytes < 16 + (size_t)52 * n) {
    err = "weights blob: bad version or truncated directory";
    return false;
  }
  const size_t data0 = 16 + (size_t)52 * n;
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t* e = p + 16 + (size_t)52 * i;
    char name[25] = {0};
    std::memcpy(name, e, 24);
    Tensor t;
    std::memcpy(&t.ndim, e + 24, 4);
    std::memcpy(t.dims, e + 28, 16);
    uint32_t off;
    std::memcpy(&off, e + 44, 4);
    std::memcpy(&t.count, e + 48, 4);
    if (t.ndim > 4 || data0 + 4 * ((size_t)off + t.count) > nbytes) {
      err = std::string("weights blob: tensor out of bounds: ") + name;
      return false;
    }
    t.data = reinterpret_cast<const float*>(p + data0 + 4 * (size_t)off);
    out.t.emplace_back(name, t);
  }
  return true;
}

bool expect(const Blob& b, const char* name, std::initializer_list<uint32_t> shape, const Tensor*& t,
            std::string& err) {
  t = b.find(name);
  if (!t) {
    err = std::string("weights blob: missing tensor ") + name;
    return false;
  }
  uint32_t cnt = 1;
  uint32_t i = 0;
  for (uint32_t d : shape) {
    if (i >= t->ndim || t->dims[i] != d) {
      err = std::string("weights blob: wrong shape for ") + name;
      return false;
    }
    cnt *= d;
    ++i;
  }
  if (i != t->ndim || cnt != t->count) {
    err = std::string("weights blob: wrong rank/count for ") + name;
    return false;
  }
  return true;
}

// ---- operand packing -----------------------------------------------------------------------
// Filterbank B fragments [4 roles][55 steps][64 lanes] (cqt_filterbank.hip roles; 16x16x4: lane ->
// B[k = lane >> 4][n = lane & 15]).
bool pack_filterbank(const Tensor* re, const Tensor* im, std::vector<float>& out, std::string& err) {
  // verify the clipped K ranges cover every non-zero tap
  for (int f = 0; f < 36; ++f) {
    const int lo = f < 16 ? 20 : f < 32 ? 48 : 68, hi = f < 16 ? 236 : f < 32 ? 208 : 188;
    for (int i = 0; i < 256; ++i) {
      if ((i < lo || i >= hi) && (re->data[f * 256 + i] != 0.f || im->data[f * 256 + i] != 0.f)) {
        err = "CQT kernel support exceeds the tap ranges this build is specialised for";
        return false;
      }
    }
  }
  out.assign(4 * 55 * 64, 0.f);
  for (int role = 0; role < 4; ++role) {
    for (int j = 0; j < 55; ++j) {
      for (int lane = 0; lane < 64; ++lane) {
        const int kk = lane >> 4, n = lane & 15;
        float v = 0.f;
        if (role < 2) {
          if (j < 54) {
            const int tap = 4 * (5 + j) + kk;
            v = (role == 0 ? re : im)->data[n * 256 + tap];
          }
        } else {
          const Tensor* main = (role == 2) ? re : im;
          if (j < 40) {
            const int tap = 4 * (12 + j) + kk;
            v = main->data[(16 + n) * 256 + tap];
          } else {
            const int s = (role == 2 ? 17 : 32) + (j - 40);
            const int tap = 4 * s + kk;
            if (n < 4)
              v = re->data[(32 + n) * 256 + tap];
            else if (n < 8)
              v = im->data[(32 + n - 4) * 256 + tap];
          }
        }
        out[((size_t)role * 55 + j) * 64 + lane] = v;
      }
    }
  }
  return true;
}

// IEEE binary16 <-> binary32 on the host (round to nearest even; overflow gives an infinity, which put_split reports)
uint16_t f32_to_f16(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  const int32_t exp = (int32_t)((x >> 23) & 0xff) - 127 + 15;
  uint32_t man = x & 0x7fffffu;
  if (((x >> 23) & 0xff) == 0xff) return (uint16_t)(sign | 0x7c00u | (man ? 0x200u : 0));
  if (exp >= 31) return (uint16_t)(sign | 0x7c00u);
  if (exp <= 0) {
    if (exp < -10) return (uint16_t)sign;
    man |= 0x800000u;
    const int shift = 14 - exp;  // 14..24
    uint32_t half = man >> shift;
    const uint32_t rem = man & ((1u << shift) - 1), mid = 1u << (shift - 1);
    if (rem > mid || (rem == mid && (half & 1))) ++half;
    return (uint16_t)(sign | half);
  }
  uint32_t half = ((uint32_t)exp << 10) | (man >> 13);
  const uint32_t rem = man & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (half & 1))) ++half;  // may carry into the exponent: correct
  return (uint16_t)(sign | half);
}

float f16_to_f32(uint16_t hv) {
  const uint32_t sign = (uint32_t)(hv & 0x8000u) << 16;
  uint32_t exp = (hv >> 10) & 0x1f, man = hv & 0x3ffu, x;
  if (exp == 0) {
    if (man == 0) {
      x = sign;
    } else {
      int e = -1;
      do {
        ++e;
        man <<= 1;
      } while (!(man & 0x400u));
      x = sign | ((uint32_t)(127 - 15 - e) << 23) | ((man & 0x3ffu) << 13);
    }
  } else if (exp == 31) {
    x = sign | 0x7f800000u | (man << 13);
  } else {
    x = sign | ((exp - 15 + 127) << 23) | (man << 13);
  }
  float f;
  std::memcpy(&f, &x, 4);
  return f;
}

// x = hi + lo / lo_scale: lo_scale > 1 keeps the residual inside f16's normal range (cqt_mfma.hip).  Returns false if
// the hi part is not a finite f16 (|v| >= 65520, or v not finite): the caller refuses the weights.
bool put_split(std::vector<uint16_t>& out, size_t hi_base, size_t lo_base, size_t idx, float v,
               float lo_scale = 1.0f) {
  const uint16_t hi = f32_to_f16(v);
  out[hi_base + idx] = hi;
  out[lo_base + idx] = f32_to_f16((v - f16_to_f32(hi)) * lo_scale);
  return (hi & 0x7c00u) != 0x7c00u;
}

// The folded kernel (pack_contour_folded) for the vertical march (conv_contour_march.hip): M = 16 rows = (2-bin offset j,
// out channel o), a position is a pair of bins, K = 6 k-steps of 32 taps per frame tap.  A fragments [3 dt][6 k-steps]
// [hi|lo][64 lanes] x (8 x f16): lane (row i = 8 j + o = lane & 15, gq = lane >> 4), element el -> tap' = 32 s + 8 gq + el,
// g = tap' - j - 56.
bool pack_contour_march(const Tensor* w1, std::vector<uint16_t>& out) {
  bool ok = true;
  static const int shifts[8] = {-36, 0, 36, 57, 72, 84, 93, 101};  // nn.py:51-54 (bp_common.h harm_shift)
  std::vector<double> keff((size_t)8 * 3 * 176, 0.0);               // [o][dt][g + 55]
  for (int o = 0; o < 8; ++o)
    for (int c = 0; c < 8; ++c)
      for (int dt = 0; dt < 3; ++dt)
        for (int df = 0; df < 39; ++df)
          keff[((size_t)o * 3 + dt) * 176 + (df - 19 + shifts[c] + 55)] += (double)w1->data[((o * 8 + c) * 3 + dt) * 39 + df];
  out.assign((size_t)18 * 2 * 64 * 8, 0);
  for (int dt = 0; dt < 3; ++dt)
    for (int s = 0; s < 6; ++s)
      for (int lane = 0; lane < 64; ++lane) {
        const int gq = lane >> 4, i = lane & 15, j = i >> 3, o = i & 7;
        const size_t base_hi = (((size_t)(dt * 6 + s) * 2 + 0) * 64 + lane) * 8;
        const size_t base_lo = (((size_t)(dt * 6 + s) * 2 + 1) * 64 + lane) * 8;
        for (int el = 0; el < 8; ++el) {
          const int g = 32 * s + 8 * gq + el - j - 56;
          const float v = (g >= -55 && g <= 120) ? (float)keff[((size_t)o * 3 + dt) * 176 + g + 55] : 0.0f;
          ok &= put_split(out, base_hi, base_lo, el, v, 2048.0f);
        }
      }
  return ok;
}

// Rim of the contour conv1 as a dense GEMM (conv_contour_rim.hip): per side (low rim f in [0, 20), high rim
// f in [244, 264)) the position-dependent folded kernel K[(f, o)][dt][j] over the z bins j0 + [0, 144):
//   K = sum over (c, df) with stack bin f + df - 19 inside [0, 264) (nn.py:87 crops the stack to 264 bins, the
//   convolution zero-pads THAT) and z bin f + df - 19 + shift_c == j0 + j of W1[o][c][dt][df].
// A fragments [side][M block 5][k-step 27 = dt * 9 + e][hi|lo][64 lanes][8]: lane (i = lane & 31 = 8 (f % 4) + o,
// kh = lane >> 5), element el: j = 16 e + 8 kh + el.
// `n_bins`: bins of the CQT (309; 345 for the extended 44.1 kHz mode, whose bins 309..344 reach the high rim); `kJ`: z bins a
// side's window holds (144; 160 for the extended mode: the kernel's RimGeo<160>).
bool pack_contour_rim(const Tensor* w1, std::vector<uint16_t>& out, int n_bins = 309, int kJ = 144) {
  static const int shifts[8] = {-36, 0, 36, 57, 72, 84, 93, 101};
  bool ok = true;
  const int kStepsDt = kJ / 16;
  out.assign((size_t)2 * 5 * 3 * kStepsDt * 2 * 64 * 8, 0);
  for (int side = 0; side < 2; ++side) {
    const int f0 = side ? 244 : 0, j0 = side ? (kJ == 144 ? 184 : 188) : 0;  // conv_contour_rim.hip RimGeo::j0
    std::vector<double> k((size_t)20 * 8 * 3 * kJ, 0.0);  // [f_local][o][dt][j]
    for (int fl = 0; fl < 20; ++fl)
      for (int o = 0; o < 8; ++o)
        for (int c = 0; c < 8; ++c)
          for (int dt = 0; dt < 3; ++dt)
            for (int df = 0; df < 39; ++df) {
              const int sb = f0 + fl + df - 19;  // stack bin this tap reads
              if (sb < 0 || sb >= 264) continue;
              const int j = sb + shifts[c] - j0;  // z bin (zero outside [0, 309): nothing to add there)
              const int zb = sb + shifts[c];
              if (zb < 0 || zb >= n_bins) continue;
              if (j < 0 || j >= kJ) {  // cannot happen with the windows above
                std::fprintf(stderr, "pack_contour_rim: z bin %d outside the side's window\n", zb);
                std::abort();
              }
              k[(((size_t)fl * 8 + o) * 3 + dt) * kJ + j] += (double)w1->data[((o * 8 + c) * 3 + dt) * 39 + df];
            }
    for (int mb = 0; mb < 5; ++mb)
      for (int dt = 0; dt < 3; ++dt)
        for (int e = 0; e < kStepsDt; ++e)
          for (int lane = 0; lane < 64; ++lane) {
            const int kh = lane >> 5, i = lane & 31, fl = 4 * mb + (i >> 3), o = i & 7;
            const size_t step = ((size_t)(side * 5 + mb) * 3 * kStepsDt + dt * kStepsDt + e);
            const size_t base_hi = ((step * 2 + 0) * 64 + lane) * 8, base_lo = ((step * 2 + 1) * 64 + lane) * 8;
            for (int el = 0; el < 8; ++el) {
              const int j = 16 * e + 8 * kh + el;
              ok &= put_split(out, base_hi, base_lo, el, (float)k[(((size_t)fl * 8 + o) * 3 + dt) * kJ + j], 2048.0f);
            }
          }
  }
  return ok;
}

// The same dense per-side matrix for the register-resident rim kernel (conv_contour_rim_march.hip, 309-bin CQT): M blocks of
// 16 rows = (2 bins x 8 channels), K = (dt, j) flattened = 432 -> 14 k-steps of 32 (zeros behind 432).  A fragments
// [side][block 10][k-step 14][hi|lo][64 lanes][8]: lane (row i = lane & 15 = 8 (f % 2) + o, g = lane >> 4), element el:
// k = 32 s + 8 g + el.
bool pack_contour_rim_march(const Tensor* w1, std::vector<uint16_t>& out) {
  static const int shifts[8] = {-36, 0, 36, 57, 72, 84, 93, 101};
  bool ok = true;
  constexpr int kJ = 144, kSteps = (3 * kJ + 31) / 32, n_bins = 309;
  out.assign((size_t)2 * 10 * kSteps * 2 * 64 * 8, 0);
  for (int side = 0; side < 2; ++side) {
    const int f0 = side ? 244 : 0, j0 = side ? 184 : 0;
    std::vector<double> k((size_t)20 * 8 * 3 * kJ, 0.0);  // [f_local][o][dt][j], as pack_contour_rim
    for (int fl = 0; fl < 20; ++fl)
      for (int o = 0; o < 8; ++o)
        for (int c = 0; c < 8; ++c)
          for (int dt = 0; dt < 3; ++dt)
            for (int df = 0; df < 39; ++df) {
              const int sb = f0 + fl + df - 19;
              if (sb < 0 || sb >= 264) continue;
              const int zb = sb + shifts[c], j = zb - j0;
              if (zb < 0 || zb >= n_bins) continue;
              if (j < 0 || j >= kJ) {
                std::fprintf(stderr, "pack_contour_rim_march: z bin %d outside the side's window\n", zb);
                std::abort();
              }
              k[(((size_t)fl * 8 + o) * 3 + dt) * kJ + j] += (double)w1->data[((o * 8 + c) * 3 + dt) * 39 + df];
            }
    for (int mb = 0; mb < 10; ++mb)
      for (int s = 0; s < kSteps; ++s)
        for (int lane = 0; lane < 64; ++lane) {
          const int g = lane >> 4, i = lane & 15, fl = 2 * mb + (i >> 3), o = i & 7;
          const size_t step = (size_t)(side * 10 + mb) * kSteps + s;
          const size_t base_hi = ((step * 2 + 0) * 64 + lane) * 8, base_lo = ((step * 2 + 1) * 64 + lane) * 8;
          for (int el = 0; el < 8; ++el) {
            const int kk = 32 * s + 8 * g + el;
            const float v = kk < 3 * kJ ? (float)k[(((size_t)fl * 8 + o) * 3 + kk / kJ) * kJ + kk % kJ] : 0.0f;
            ok &= put_split(out, base_hi, base_lo, el, v, 2048.0f);
          }
        }
  }
  return ok;
}

// contour conv1 Toeplitz B fragments [4 waves][126][64] (conv_contour1.hip).
void pack_contour1(const Tensor* w, std::vector<float>& out) {
  static const int chan[4][2] = {{0, 1}, {2, 4}, {5, 3}, {6, 7}};
  out.assign(4 * 126 * 64, 0.f);
  for (int wave = 0; wave < 4; ++wave)
    for (int slot = 0; slot < 2; ++slot)
      for (int dt = 0; dt < 3; ++dt)
        for (int ep = 0; ep < 21; ++ep)
          for (int lane = 0; lane < 64; ++lane) {
            const int kodd = lane >> 5, n = lane & 31, o = n >> 2, jj = n & 3;
            const int c = chan[wave][slot];
            const int df = 2 * ep + kodd - jj;
            float v = 0.f;
            if (df >= 0 && df < 39) v = w->data[((o * 8 + c) * 3 + dt) * 39 + df];
            out[((size_t)wave * 126 + slot * 63 + dt * 21 + ep) * 64 + lane] = v;
          }
}

void pack_onset1(const Tensor* w, std::vector<float>& out) {
  out.assign(100 * 64, 0.f);
  for (int cp = 0; cp < 4; ++cp)
    for (int dt = 0; dt < 5; ++dt)
      for (int dw = 0; dw < 5; ++dw)
        for (int lane = 0; lane < 64; ++lane) {
          const int c = 2 * cp + (lane >> 5), o = lane & 31;
          out[((size_t)(cp * 5 + dt) * 5 + dw) * 64 + lane] = w->data[((o * 8 + c) * 5 + dt) * 5 + dw];
        }
}

void pack_note1(const Tensor* w, std::vector<float>& out) {
  out.assign(25 * 64, 0.f);
  for (int s = 0; s < 25; ++s)
    for (int lane = 0; lane < 64; ++lane) {
      const int k = 2 * s + (lane >> 5), o = lane & 31;
      out[(size_t)s * 64 + lane] = (k < 49) ? w->data[o * 49 + k] : 0.f;
    }
}

// onset_march16.hip: conv1 (8 -> 32, 5 x 5, models.py:295-304) and the 3 x 3 head's feature channels (305-318) as
// v_mfma_f32_16x16x32_f16 A fragments: [A1 hi: (2 s + mb) x 64 lanes][A1 lo: 14 + ...][A2 hi][A2 lo] x 8 f16.
// A1: lane (m = lane & 15, g = lane >> 4), element e: out channel 16 mb + m, stack channel e, tap onset16_{dt,dw}(s, g).
// A2: row rho = lane & 15 = 4 dt + dw (dt, dw < 3), K index 8 g + e <-> conv1 channel 4 g + e (e < 4) or 16 + 4 g + e - 4:
// the order in which conv1's C layout leaves a pixel's channels in a lane.
// Returns 0, or bit 0 / bit 1 set if a weight of w1 / w2 has no finite f16 hi part.
int pack_onset16(const Tensor* w1, const Tensor* w2, std::vector<uint16_t>& out) {
  const size_t frag = 64 * 8, a1h = 0, a1l = 2 * kOnset16KSteps * frag, a2h = 2 * a1l, a2l = a2h + frag;
  out.assign(a2l + frag, 0);
  int bad = 0;
  for (int s = 0; s < kOnset16KSteps; ++s)
    for (int mb = 0; mb < 2; ++mb)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int m = lane & 15, g = lane >> 4;
          const int q = onset16_dt(s, g) * 5 + onset16_dw(s, g);
          const float v = onset16_live(s, g) ? w1->data[((16 * mb + m) * 8 + e) * 25 + q] : 0.f;
          if (!put_split(out, a1h, a1l, ((size_t)(2 * s + mb) * 64 + lane) * 8 + e, v, 2048.0f)) bad |= 1;
        }
  for (int lane = 0; lane < 64; ++lane)
    for (int e = 0; e < 8; ++e) {
      const int rho = lane & 15, g = lane >> 4;
      const int dt = rho >> 2, dw = rho & 3;
      const int ch = e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4);
      const float v = (dt < 3 && dw < 3) ? w2->data[((1 + ch) * 3 + dt) * 3 + dw] : 0.f;  // channel 0 of the concat is the note map
      if (!put_split(out, a2h, a2l, (size_t)lane * 8 + e, v, 2048.0f)) bad |= 2;
    }
  return bad;
}

// conv_contour2.hip contour_conv2_proj_kernel: Conv2D 8 -> 1, 5 x 5 (models.py:254-263; w2 is OIHW (1, 8, 5, 5)) as the A operand
// of v_mfma_f32_32x32x16_f16 with the three split-precision products packed along K: two fragments x 64 lanes x (8 x f16),
// A1 = [hi 2^11 | hi], A2 = [lo 2^11 | 0] against the B operand [hi(c1) | lo(c1) 2^11] of four channels.  Lane (m = lane & 31,
// hk = lane >> 5), elements j < 4 / j >= 4: channel 4 hk + (j & 3); row m <-> C register r = (m & 3) + 4 (m >> 3) of lane half
// (m >> 2) & 1; half 0 holds frame taps dt = 0, 1, 2 (r = 5 dt + df, r = 15 unused), half 1 dt = 3, 4 (r = 5 (dt - 3) + df,
// r >= 10 unused).
bool pack_conv2_proj(const Tensor* w2, std::vector<uint16_t>& out) {
  const size_t frag = 64 * 8;
  out.assign(2 * frag, 0);
  bool ok = true;
  for (int lane = 0; lane < 64; ++lane)
    for (int j = 0; j < 4; ++j) {
      const int m = lane & 31, hk = lane >> 5;
      const int r = (m & 3) + 4 * (m >> 3), half = (m >> 2) & 1;
      const int dt = (half ? 3 : 0) + r / 5, df = r % 5, ch = 4 * hk + j;
      const bool used = half ? r < 10 : r < 15;
      const float v = used ? w2->data[(ch * 5 + dt) * 5 + df] : 0.f;
      const uint16_t hi = f32_to_f16(v);
      const float hif = f16_to_f32(hi);
      if (!(std::fabs(hif) * 2048.0f < 65504.0f)) ok = false;
      const size_t idx = (size_t)lane * 8 + j;
      out[idx] = f32_to_f16(hif * 2048.0f);                 // x hi(c1)
      out[idx + 4] = hi;                                    // x lo(c1) 2^11
      out[frag + idx] = f32_to_f16((v - hif) * 2048.0f);    // x hi(c1); elements 4..7 stay zero
    }
  return ok;
}

// note_march16.hip: conv1 (1 -> 32, 7 x 7, stride (1, 3), models.py:270-278) and the (7, 3) head (282-289) as
// v_mfma_f32_16x16x32_f16 A fragments, 18 x 64 lanes x (8 x f16): conv1 [kind][k-step s][block mb] at (4 kind + 2 s + mb),
// conv2 [kind][block mb] at 12 + 2 kind + mb; kind 0 = hi 2^11, 1 = hi, 2 = lo 2^11 (the kernel adds all three products
// into one accumulator at scale 2^11).  conv1: lane (m = lane & 15, g = lane >> 4), element e: out channel 16 mb + m, frame
// tap dt = 4 s + g (7: zero), bin offset e (7: zero).  conv2: row rho = lane & 15 = 4 dw + i <-> tap (dt = 4 mb + i, dw)
// (dw = 3, dt = 7: zero rows); K index 8 g + e <-> conv1 channel 4 g + e (e < 4) or 16 + 4 g + e - 4 — the order in which
// conv1's C layout leaves a pixel's channels in a lane.  Returns false if a weight's hi part does not survive the 2^11.
bool pack_note16(const Tensor* w1, const Tensor* w2, std::vector<uint16_t>& out) {
  const size_t frag = 64 * 8;
  out.assign(18 * frag, 0);
  bool ok = true;
  auto put3 = [&](size_t f_hi_scaled, size_t f_hi, size_t f_lo, size_t idx, float v) {
    const uint16_t hi = f32_to_f16(v);
    const float hif = f16_to_f32(hi);
    if (!(std::fabs(hif) * 2048.0f < 65504.0f)) ok = false;
    out[f_hi_scaled * frag + idx] = f32_to_f16(hif * 2048.0f);
    out[f_hi * frag + idx] = hi;
    out[f_lo * frag + idx] = f32_to_f16((v - hif) * 2048.0f);
  };
  for (int s = 0; s < 2; ++s)
    for (int mb = 0; mb < 2; ++mb)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int m = lane & 15, g = lane >> 4, dt = 4 * s + g;
          const float v = (dt < 7 && e < 7) ? w1->data[((16 * mb + m) * 7 + dt) * 7 + e] : 0.f;
          put3(0 + 2 * s + mb, 4 + 2 * s + mb, 8 + 2 * s + mb, (size_t)lane * 8 + e, v);
        }
  for (int mb = 0; mb < 2; ++mb)
    for (int lane = 0; lane < 64; ++lane)
      for (int e = 0; e < 8; ++e) {
        const int rho = lane & 15, g = lane >> 4;
        const int dw = rho >> 2, dt = 4 * mb + (rho & 3);
        const int ch = e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4);
        const float v = (dw < 3 && dt < 7) ? w2->data[(ch * 7 + dt) * 3 + dw] : 0.f;
        put3(12 + mb, 14 + mb, 16 + mb, (size_t)lane * 8 + e, v);
      }
  return ok;
}

// cqt_planes_pyramid.hip decimator (transposed: the filter is the A operand): T[u][i] = h[i - 2u - 1] — the input window starts one
// sample before the reference's (an 8-sample aligned element of the padded plane) — as [hi: 9 steps][lo: 9 steps] x 64
// lanes x 8 f16; lane (u = lane & 15, kg = lane >> 4), element e: i = 32 s + 8 kg + e.
void pack_decimator_f16(const Tensor* lowp, std::vector<uint16_t>& out, int shift = 1) {
  const size_t lo_base = (size_t)9 * 64 * 8;
  out.assign(2 * lo_base, 0);
  for (int s = 0; s < 9; ++s)
    for (int lane = 0; lane < 64; ++lane)
      for (int e = 0; e < 8; ++e) {
        const int u = lane & 15, kg = lane >> 4;
        const int j = 32 * s + 8 * kg + e - 2 * u - shift;
        // taps pre-scaled by 2^10, residuals by a further 2^11 (kDmTapScale / kLoScale in cqt_mfma.hip)
        put_split(out, 0, lo_base, ((size_t)s * 64 + lane) * 8 + e,
                  (j >= 0 && j < 256) ? lowp->data[j] * 1024.0f : 0.f, 2048.0f);
      }
}

// cqt_planes_filterbank.hip: [29 step-fragments][hi|lo][64 lanes][8] f16.  Column groups of 16: 0 = re of filters 0..15,
// 1 = im 0..15 (7 steps from tap 16), 2 = re 16..31, 3 = im 16..31, 4 = {re 32..35, im 32..35, 8 zero columns} (5 steps
// from tap 48); lane (n = lane & 15, kg), element e: tap = 16 + 32 s + 8 kg + e of k-step s.
void pack_filterbank_planes(const Tensor* re, const Tensor* im, std::vector<uint16_t>& out) {
  out.assign((size_t)29 * 2 * 64 * 8, 0);
  static const int frag0[5] = {0, 7, 14, 19, 24}, step0[5] = {0, 0, 1, 1, 1}, steps[5] = {7, 7, 5, 5, 5};
  for (int g = 0; g < 5; ++g)
    for (int s = 0; s < steps[g]; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int n = lane & 15, kg = lane >> 4;
          const int tap = 16 + 32 * (step0[g] + s) + 8 * kg + e;
          float v = 0.f;
          if (g < 4) {
            v = ((g & 1) ? im : re)->data[((g >> 1) * 16 + n) * 256 + tap];
          } else if (n < 8) {
            v = (n < 4 ? re : im)->data[(32 + (n & 3)) * 256 + tap];
          }
          const size_t base = ((size_t)(frag0[g] + s) * 2) * 64 * 8;
          put_split(out, base, base + 64 * 8, (size_t)lane * 8 + e, v * 4096.0f, 2048.0f);
        }
}

#ifdef BP_AB_KERNELS  // operands of the A/B library's kernels
// Folded contour conv1 (conv_contour_direct.hip, interior groups): the 8 stack channels are shifted copies of one
// image, so K[o][dt][g] = sum_c W1[o][c][dt][g - s_c + 19], g in [-55, 120].  A fragments [3 dt][12 k-steps][hi|lo]
// [64 lanes] x (8 x f16): lane (row i = 8 j + o, half kh), element el -> tap' = 16 e + 8 kh + el, g = tap' - j - 56.
void pack_contour_folded(const Tensor* w1, std::vector<uint16_t>& out) {
  static const int shifts[8] = {-36, 0, 36, 57, 72, 84, 93, 101};  // nn.py:51-54 (bp_common.h harm_shift)
  std::vector<double> keff((size_t)8 * 3 * 176, 0.0);               // [o][dt][g + 55]
  for (int o = 0; o < 8; ++o)
    for (int c = 0; c < 8; ++c)
      for (int dt = 0; dt < 3; ++dt)
        for (int df = 0; df < 39; ++df)
          keff[((size_t)o * 3 + dt) * 176 + (df - 19 + shifts[c] + 55)] += (double)w1->data[((o * 8 + c) * 3 + dt) * 39 + df];
  out.assign((size_t)36 * 2 * 64 * 8, 0);
  for (int dt = 0; dt < 3; ++dt)
    for (int e = 0; e < 12; ++e)
      for (int lane = 0; lane < 64; ++lane) {
        const int kh = lane >> 5, i = lane & 31, j = i >> 3, o = i & 7;
        const size_t base_hi = (((size_t)(dt * 12 + e) * 2 + 0) * 64 + lane) * 8;
        const size_t base_lo = (((size_t)(dt * 12 + e) * 2 + 1) * 64 + lane) * 8;
        for (int el = 0; el < 8; ++el) {
          const int g = 16 * e + 8 * kh + el - j - 56;
          const float v = (g >= -55 && g <= 120) ? (float)keff[((size_t)o * 3 + dt) * 176 + g + 55] : 0.0f;
          put_split(out, base_hi, base_lo, el, v, 2048.0f);
        }
      }
}

// Fused branch A fragments (conv_branch.hip): [A1 hi: KS1*64][A1 lo: KS1*64][A2 hi: 2*64][A2 lo: 2*64] x 8 f16.
// A1 lane (i = out channel = lane & 31, h = lane >> 5), element e: conv1 weight of k = 8h + e of step s.
// A2 lane (i = projection row, h), element e of step s2: conv2 weight of the channel that C-register
// 8*s2 + e of half h holds: (e & 3) + 16*s2 + 8*(e >> 2) + 4h.
void pack_branch(int ks1, const Tensor* w1, const Tensor* w2, bool onset, std::vector<uint16_t>& out) {
  const size_t a1h = 0, a1l = (size_t)ks1 * 64 * 8, a2h = 2 * a1l, a2l = a2h + 2 * 64 * 8;
  out.assign(a2l + 2 * 64 * 8, 0);
  const int kh2 = onset ? 3 : 7;
  for (int s = 0; s < ks1; ++s)
    for (int lane = 0; lane < 64; ++lane)
      for (int e = 0; e < 8; ++e) {
        const int i = lane & 31, hh = lane >> 5;
        float v = 0.f;
        if (onset) {  // k-step = tap pair of the 5x5 window x 8 stack channels (models.py:295-304)
          const int q = 2 * s + hh;
          if (q < 25) v = w1->data[((i * 8 + e) * 5 + q / 5) * 5 + q % 5];
        } else {  // k-step = frame-tap pair x 8 adjacent bins, 7 used (models.py:270-278)
          const int dt = 2 * s + hh;
          if (dt < 7 && e < 7) v = w1->data[(i * 7 + dt) * 7 + e];
        }
        put_split(out, a1h, a1l, ((size_t)s * 64 + lane) * 8 + e, v, 2048.0f);
      }
  // A2 row rho is C row rho of the projection: register r = (rho & 3) + 4 (rho >> 3) of lane half (rho >> 2) & 1.
  // Half 0 takes frame taps 0 .. DT0-1, half 1 the rest, three dw taps in consecutive registers: the kernel's
  // horizontal sum is then two lane shifts (conv_branch.hip, NoteBr::DT0 / OnsetBr::DT0).
  const int dt0 = onset ? 2 : 4;
  for (int s2 = 0; s2 < 2; ++s2)
    for (int lane = 0; lane < 64; ++lane)
      for (int e = 0; e < 8; ++e) {
        const int rho = lane & 31, hh = lane >> 5;
        const int ch = (e & 3) + 16 * s2 + 8 * (e >> 2) + 4 * hh;
        const int r = (rho & 3) + 4 * (rho >> 3), half = (rho >> 2) & 1;
        const int dt = dt0 * half + r / 3, dw = r % 3;
        float v = 0.f;
        if (r < 3 * dt0 && dt < kh2) {
          v = onset ? w2->data[((1 + ch) * 3 + dt) * 3 + dw]   // channel 0 of the concat is the note map
                    : w2->data[(ch * 7 + dt) * 3 + dw];
        }
        put_split(out, a2h, a2l, ((size_t)s2 * 64 + lane) * 8 + e, v, 2048.0f);
      }
}
#endif  // BP_AB_KERNELS

}  // namespace

namespace bp {

namespace {

// a device table of the handle: `field` receives the bytes of `parts`, one after the other
template <class... V>
void add(PackedWeights& pw, bp_context::Table bp_context::*field, const V&... parts) {
  std::vector<uint8_t> bytes;
  (bytes.insert(bytes.end(), reinterpret_cast<const uint8_t*>(parts.data()),
                reinterpret_cast<const uint8_t*>(parts.data() + parts.size())),
   ...);
  pw.tables.emplace_back(field, std::move(bytes));
}

std::vector<float> vec(const Tensor* t) { return std::vector<float>(t->data, t->data + t->count); }

}  // namespace

int pack_weights(const void* weights, size_t nbytes, unsigned flags, PackedWeights& out, std::string& err) {
  Blob blob;
  if (!parse_blob(weights, nbytes, blob, err)) return BP_ERR_BAD_WEIGHTS;
  const Tensor *re, *im, *lowp, *sq, *eps, *lsc, *bn, *c1w, *c1b, *c2w, *c2b, *n1w, *n1b, *n2w, *n2b, *o1w,
      *o1b, *o2w, *o2b;
  if (!expect(blob, "cqt_kernel_re", {36, 256}, re, err) || !expect(blob, "cqt_kernel_im", {36, 256}, im, err) ||
      !expect(blob, "cqt_lowpass", {256}, lowp, err) || !expect(blob, "cqt_sqrt_len", {309}, sq, err) ||
      !expect(blob, "log_eps", {1}, eps, err) || !expect(blob, "log_scale", {2}, lsc, err) ||
      !expect(blob, "bn_affine", {2}, bn, err) || !expect(blob, "contour1_w", {8, 8, 3, 39}, c1w, err) ||
      !expect(blob, "contour1_b", {8}, c1b, err) || !expect(blob, "contour2_w", {1, 8, 5, 5}, c2w, err) ||
      !expect(blob, "contour2_b", {1}, c2b, err) || !expect(blob, "note1_w", {32, 1, 7, 7}, n1w, err) ||
      !expect(blob, "note1_b", {32}, n1b, err) || !expect(blob, "note2_w", {1, 32, 7, 3}, n2w, err) ||
      !expect(blob, "note2_b", {1}, n2b, err) || !expect(blob, "onset1_w", {32, 8, 5, 5}, o1w, err) ||
      !expect(blob, "onset1_b", {32}, o1b, err) || !expect(blob, "onset2_w", {1, 33, 3, 3}, o2w, err) ||
      !expect(blob, "onset2_b", {1}, o2b, err))
    return BP_ERR_BAD_WEIGHTS;
  // BP_FLAG_BF16_WEIGHTS: the six Conv2D weight tensors rounded to bf16 (round to nearest even); everything
  // downstream (packing, the exact same kernels) sees ordinary fp32 numbers with 8 significant bits
  std::vector<std::vector<float>> rounded;
  std::vector<Tensor> rounded_t;
  rounded.reserve(6);
  rounded_t.reserve(6);
  if ((flags & BP_FLAG_BF16_WEIGHTS) && !(flags & BP_FLAG_F32_MFMA)) {
    auto to_bf16 = [&](const Tensor*& t) {
      rounded.emplace_back(t->data, t->data + t->count);
      for (float& v : rounded.back()) {
        uint32_t u;
        std::memcpy(&u, &v, 4);
        u = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
        std::memcpy(&v, &u, 4);
      }
      Tensor c = *t;
      c.data = rounded.back().data();
      rounded_t.push_back(c);
      t = &rounded_t.back();
    };
    to_bf16(c1w), to_bf16(c2w), to_bf16(n1w), to_bf16(n2w), to_bf16(o1w), to_bf16(o2w);
  }
  // a model is any set of finite numbers: a NaN or an infinity would reach every output of a branch unannounced (after the
  // bf16 rounding: a finite value next to FLT_MAX rounds to an infinity)
  for (const auto& nt : {std::make_pair("bn_affine", bn), std::make_pair("contour1_w", c1w), std::make_pair("contour1_b", c1b),
                         std::make_pair("contour2_w", c2w), std::make_pair("contour2_b", c2b), std::make_pair("note1_w", n1w),
                         std::make_pair("note1_b", n1b), std::make_pair("note2_w", n2w), std::make_pair("note2_b", n2b),
                         std::make_pair("onset1_w", o1w), std::make_pair("onset1_b", o1b), std::make_pair("onset2_w", o2w),
                         std::make_pair("onset2_b", o2b)})
    for (uint32_t i = 0; i < nt.second->count; ++i)
      if (!std::isfinite(nt.second->data[i])) {
        err = std::string("bp_create: ") + nt.first + " holds a NaN or an infinity";
        return BP_ERR_BAD_WEIGHTS;
      }
  std::vector<float> fb;
  if (!pack_filterbank(re, im, fb, err)) return BP_ERR_UNSUPPORTED;
  const bool ext = (flags & BP_FLAG_EXT_CQT_44K) != 0;
  out.kc.eps = eps->data[0];
  out.kc.s0 = lsc->data[0];
  out.kc.s1 = lsc->data[1];
  out.kc.bn_a = bn->data[0];
  out.kc.bn_b = bn->data[1];
  out.b_contour2 = c2b->data[0];
  out.b_note2 = n2b->data[0];
  out.b_onset2 = o2b->data[0];

  // split-precision path: f16 hi | scaled-lo operand fragments + fp32 side tables
  std::vector<uint16_t> frag;
  pack_decimator_f16(lowp, frag);
  add(out, &bp_context::d_pl_tfrag, frag);
  pack_filterbank_planes(re, im, frag);
  add(out, &bp_context::d_pl_bfrag, frag);
  std::vector<float> w2t(200);
  for (int dt = 0; dt < 5; ++dt)
    for (int dw = 0; dw < 5; ++dw)
      for (int c = 0; c < 8; ++c) w2t[(dt * 5 + dw) * 8 + c] = c2w->data[(c * 5 + dt) * 5 + dw];
  add(out, &bp_context::d_d1_bias, vec(c1b));
  add(out, &bp_context::d_d2_w, w2t);
  if (!pack_conv2_proj(c2w, frag)) {
    err = "bp_create: a contour conv2 weight is too large for the scaled f16 operand (|w| >= 31.98)";
    return BP_ERR_BAD_WEIGHTS;
  }
  add(out, &bp_context::d_d2_wproj, frag);
#ifdef BP_AB_KERNELS  // the round-2 folded conv1 (conv_contour_direct.hip)
  pack_contour_folded(c1w, frag);
  add(out, &bp_context::d_d1_wfold, frag);
#endif
  // contour1_w reaches the kernels summed over the harmonic shifts that meet in one z bin (up to 8 taps)
  bool c1_ok = pack_contour_march(c1w, frag);
  add(out, &bp_context::d_d1_wmarch, frag);
  // ext: the 345-bin CQT, 160 z bins per rim side (conv_contour_rim.hip RimGeo<160>)
  c1_ok &= ext ? pack_contour_rim(c1w, frag, kBinsExt, 160) : pack_contour_rim(c1w, frag);
  add(out, &bp_context::d_d1_wrim, frag);
  if (!ext) {  // the register-resident rim kernel serves the 309-bin CQT
    c1_ok &= pack_contour_rim_march(c1w, frag);
    add(out, &bp_context::d_d1_wrimm, frag);
  }
  if (!c1_ok) {
    err = "bp_create: contour1_w, folded over the harmonic shifts, is too large for the f16 operand (|w| >= 65520)";
    return BP_ERR_BAD_WEIGHTS;
  }
  // the reduced-precision fp8-corrections mode was retired in round 6 (not faster than the default any more, narrower
  // than the config's fp32); BP_FLAG_F16_CORRECTIONS, the name of today's only arithmetic, wins when both are set
  if ((flags & BP_FLAG_FP8_CORRECTIONS) && !(flags & BP_FLAG_F16_CORRECTIONS)) {
    err = "bp_create: BP_FLAG_FP8_CORRECTIONS was retired in round 6; every split-precision product is computed on f16";
    return BP_ERR_INVALID_ARG;
  }
  for (int br = 0; br < 2; ++br) {
    std::vector<float> f32(42, 0.f);
    const Tensor* b1 = br ? o1b : n1b;
    for (int i = 0; i < 32; ++i) f32[i] = b1->data[i];
    if (br)
      for (int i = 0; i < 9; ++i) f32[32 + i] = o2w->data[i];  // onset2 taps of concat channel 0 (the note map)
    f32[41] = br ? o2b->data[0] : n2b->data[0];
#ifdef BP_AB_KERNELS  // the 32x32x16 kernels' fragments (note_march.hip, onset_march.hip, conv_branch.hip)
    pack_branch(br ? 13 : 4, br ? o1w : n1w, br ? o2w : n2w, br == 1, frag);
    add(out, br ? &bp_context::d_onset_wfrag : &bp_context::d_note_wfrag, frag);
#endif
    add(out, br ? &bp_context::d_onset_wf32 : &bp_context::d_note_wf32, f32);
  }
  // the note march on 16x16x32 (the default): its own fragment order, the hi parts also at scale 2^11
  if (!pack_note16(n1w, n2w, frag)) {
    err = "bp_create: a note-branch weight is too large for the scaled f16 operand (|w| >= 31.98)";
    return BP_ERR_BAD_WEIGHTS;
  }
  add(out, &bp_context::d_note_w16, frag);
  // the onset march on 16x16x32 (the default): its own fragment order
  // (onset2_w's taps of concat channel 0, the note map, are an fp32 table: no f16 limit there)
  if (const int bad = pack_onset16(o1w, o2w, frag)) {
    err = std::string("bp_create: ") + ((bad & 1) ? "onset1_w" : "onset2_w") +
          " holds a weight too large for the f16 operand (|w| >= 65520)";
    return BP_ERR_BAD_WEIGHTS;
  }
  add(out, &bp_context::d_onset_w16, frag);

  std::vector<float> c1f, o1f, n1f;
  pack_contour1(c1w, c1f);
  pack_onset1(o1w, o1f);
  pack_note1(n1w, n1f);
  std::vector<float> sqrt_len = vec(sq);
  if (ext) {
    // lengths = ceil(Q * sr / f_b), f_b = 27.5 * 2^(b / 36), Q = 1 / (2^(1/36) - 1) at sr = 44100 (nnaudio.py:532,
    // 590-593); bin b + 36 of this table must reproduce bin b of the 22.05 kHz artifact
    const double Q = 1.0 / (std::pow(2.0, 1.0 / 36.0) - 1.0);
    std::vector<float> ext_len(kBinsExt);
    for (int bn = 0; bn < kBinsExt; ++bn)
      ext_len[bn] = (float)std::sqrt(std::ceil(Q * 44100.0 / (27.5 * std::pow(2.0, bn / 36.0))));
    for (int bn = 0; bn < kBins; ++bn)
      if (std::fabs(ext_len[bn + 36] - sqrt_len[bn]) > 1e-6f * sqrt_len[bn]) {
        err = "bp_create: the extended sqrt(lengths) table does not continue the model's table";
        return BP_ERR_BAD_WEIGHTS;
      }
    sqrt_len = ext_len;
  }
  std::vector<float> bin_k(sqrt_len.size());
  filterbank_planes_bin_consts(sqrt_len.data(), (int)sqrt_len.size(), out.kc, bin_k.data());
  add(out, &bp_context::d_pl_bin_k, bin_k);
  add(out, &bp_context::d_lowpass, vec(lowp));
  add(out, &bp_context::d_sqrt_len, sqrt_len);
  add(out, &bp_context::d_fb_bfrag, fb);
  add(out, &bp_context::d_c1_bfrag, c1f);
  add(out, &bp_context::d_c1_bias, vec(c1b));
  add(out, &bp_context::d_o1_bfrag, o1f);
  add(out, &bp_context::d_o1_bias, vec(o1b));
  add(out, &bp_context::d_n1_bfrag, n1f);
  add(out, &bp_context::d_n1_bias, vec(n1b));
  add(out, &bp_context::d_w_contour2, vec(c2w));
  add(out, &bp_context::d_w_note2, vec(n2w));
  add(out, &bp_context::d_w_onset2, vec(o2w));
  return BP_OK;
}

}  // namespace bp
