// screen_core.h -- the 8-bit scoring and interval code shared by screen_kernel (screen8.hip) and the second stage of the
// 4-bit tier (screen4.hip): one text, so both give a row the same score8 and the same enclosure e (head of screen8.hip).
#pragma once
#include "scan_core.h"

#define BCX_SCREEN_WAVES (BCX_SCAN_THREADS / 64)

struct Q16 { float4 a, b, c, d; };   // the 16 fp32 query values matching one 16-byte piece of codes

__device__ __forceinline__ float dot16(const uint4& x, const Q16& q, float acc) {
  // (float)(byte k of a word): v_cvt_f32_ubyte0..3, one instruction per element, exact
  acc = fmaf((float)(x.x & 0xffu), q.a.x, acc); acc = fmaf((float)((x.x >> 8) & 0xffu), q.a.y, acc);
  acc = fmaf((float)((x.x >> 16) & 0xffu), q.a.z, acc); acc = fmaf((float)(x.x >> 24), q.a.w, acc);
  acc = fmaf((float)(x.y & 0xffu), q.b.x, acc); acc = fmaf((float)((x.y >> 8) & 0xffu), q.b.y, acc);
  acc = fmaf((float)((x.y >> 16) & 0xffu), q.b.z, acc); acc = fmaf((float)(x.y >> 24), q.b.w, acc);
  acc = fmaf((float)(x.z & 0xffu), q.c.x, acc); acc = fmaf((float)((x.z >> 8) & 0xffu), q.c.y, acc);
  acc = fmaf((float)((x.z >> 16) & 0xffu), q.c.z, acc); acc = fmaf((float)(x.z >> 24), q.c.w, acc);
  acc = fmaf((float)(x.w & 0xffu), q.d.x, acc); acc = fmaf((float)((x.w >> 8) & 0xffu), q.d.y, acc);
  acc = fmaf((float)((x.w >> 16) & 0xffu), q.d.z, acc); acc = fmaf((float)(x.w >> 24), q.d.w, acc);
  return acc;
}

// the 16 query values of piece v (columns 16 v .. 16 v + 15; beyond d: zero), and their sum
__device__ __forceinline__ Q16 load_q16(const float* q, int v, int d, bool ok, float& sum) {
  float t[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int j = 16 * v + k;
    const bool in = ok && j < d;
    const float val = q[in ? j : 0];
    t[k] = in ? val : 0.0f;
    sum += t[k];
  }
  Q16 r;
  r.a = make_float4(t[0], t[1], t[2], t[3]); r.b = make_float4(t[4], t[5], t[6], t[7]);
  r.c = make_float4(t[8], t[9], t[10], t[11]); r.d = make_float4(t[12], t[13], t[14], t[15]);
  return r;
}

// The single-query interval of one row: score8 = scale * acc, e as derived at the head of screen8.hip.
__device__ __forceinline__ void screen_interval(float s0, float scale, float bound, float kacc, float err_coef, float qscale,
                                                float& U, float& L) {
  const float e = (fmaf(scale, kacc, bound) * 1.000002f + err_coef) * qscale;
  const float ee = e + fabsf(s0) * 2e-7f;
  U = s0 + ee; L = s0 - ee;
}

// lanes per row and pieces per lane for rows of nvec 16-byte pieces, and the accumulation term kacc of that shape
static inline int screen_group(int nvec) {
  int g = 1;
  while (g < 64 && g < nvec) g <<= 1;
  return g;
}
static inline int screen_chunks(int nvec, int G) {
  int CH = (nvec + G - 1) / G, chp = 1;
  while (chp < CH) chp <<= 1;
  return chp;
}
static inline float screen_kacc(int G, int CH, int d) {
  int lg = 0;
  while ((1 << lg) < G) ++lg;
  const double u = 5.9604644775390625e-08;
  return (float)(1.3 * u * (511.0 * (16.0 * CH + 1.0) + 127.0 * lg) * sqrt((double)d));
}
