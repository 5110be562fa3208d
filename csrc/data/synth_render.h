// Synthetic generator v3: the per-sample plan record and the per-pixel render, shared by the host
// generator (csrc/data/synthetic_gen.cpp) and the device render (csrc/kernels/datagen.hip).
//
// A sample is two warped templates (its class's stroke and a weaker stroke of another class), a gain
// and speckle noise.  Everything transcendental (rotations, the templates' Gaussians) is done once on
// the host when the plan is made; the render is adds, multiplies, min / max, integer hashing and
// float <-> int conversions only, evaluated in one fixed order with contraction off, so the host and
// the device give the same bytes.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SYNTH_HD __host__ __device__ inline
#else
#define SYNTH_HD inline
#endif

namespace synth {

constexpr int IMG = 28;                         // output image side
constexpr int PAD = 3;                          // the warp runs on (IMG + 2 PAD)^2, a crop shifts by +/-PAD
constexpr int CANVAS = IMG + 2 * PAD;           // 34: the side of a template's drawn area
constexpr int BORDER = 15;                      // zero border around it: warped look-ups need no bounds test
constexpr int TS = CANVAS + 2 * BORDER;         // 64: template side as stored
constexpr int CLASSES = 10;
constexpr int STYLES = 6;
constexpr int TEMPLATE_FLOATS = CLASSES * STYLES * TS * TS;   // 983,040 B

// One sample of the plan.  m / o map an output pixel (col c, row r) to stored-template coordinates:
// x = m[0] c + m[1] r + m[2], y = m[3] c + m[4] r + m[5] (crop shift and border folded in).
struct Sample {
  float m[6];          // the class's stroke
  float o[6];          // the other class's stroke
  float ostr;          // its strength
  float gain;
  float nthr, namp;    // speckle: namp * u where u > nthr
  uint32_t key0, key1; // noise key
  int32_t tmain;       // template index (class * STYLES + style) of the class's stroke
  int32_t tother;      // ... of the other class's stroke
  int32_t label;       // the class the image was drawn from (before label noise)
  int32_t reserved[3];
};
static_assert(sizeof(Sample) == 96, "plan record is 96 bytes");

SYNTH_HD uint32_t mix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// uniform [0, 1) with 24 bits, a pure function of (key, pixel)
SYNTH_HD float pixel_uniform(uint32_t key0, uint32_t key1, uint32_t pixel) {
  const uint32_t h = mix32(mix32(key0 ^ (pixel * 0x9E3779B9u)) + key1);
  return (float)(h >> 8) * (1.0f / 16777216.0f);
}

// bilinear look-up in one stored template (zero border: coordinates are clamped into it)
SYNTH_HD float sample_template(const float* t, float x, float y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  x = x < 0.0f ? 0.0f : x;
  y = y < 0.0f ? 0.0f : y;
  x = x > (float)(TS - 2) ? (float)(TS - 2) : x;
  y = y > (float)(TS - 2) ? (float)(TS - 2) : y;
  const int x0 = (int)x, y0 = (int)y;
  const float wx = x - (float)x0, wy = y - (float)y0;
  const float* p = t + y0 * TS + x0;
  const float top = (1.0f - wx) * p[0] + wx * p[1];
  const float bot = (1.0f - wx) * p[TS] + wx * p[TS + 1];
  return (1.0f - wy) * top + wy * bot;
}

// pixel (0 .. IMG*IMG-1, row-major) of sample s
SYNTH_HD uint8_t render_pixel(const Sample& s, const float* templates, int pixel) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float r = (float)(pixel / IMG), c = (float)(pixel % IMG);
  const float mx = (s.m[0] * c + s.m[1] * r) + s.m[2], my = (s.m[3] * c + s.m[4] * r) + s.m[5];
  const float ox = (s.o[0] * c + s.o[1] * r) + s.o[2], oy = (s.o[3] * c + s.o[4] * r) + s.o[5];
  const float a = sample_template(templates + (int64_t)s.tmain * (TS * TS), mx, my);
  const float b = sample_template(templates + (int64_t)s.tother * (TS * TS), ox, oy);
  const float u = pixel_uniform(s.key0, s.key1, (uint32_t)pixel);
  float v = (a + s.ostr * b) * s.gain;
  if (u > s.nthr) v = v + s.namp * u;
  v = v < 0.0f ? 0.0f : v;
  v = v > 1.0f ? 1.0f : v;
  return (uint8_t)(int)(v * 255.0f + 0.5f);
}

}  // namespace synth
