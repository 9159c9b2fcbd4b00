/* Host check of libm_ref.hpp's ref_tanhf (glibc 2.35 sysdeps/ieee754/flt-32/s_tanhf.c on s_expm1f.c, float arithmetic
 * without contraction) against the host's tanhf: every float of [-22.5, 22.5] (beyond 22 the result is the constant
 * 1 - tiny), every 1009th float above that, +-inf and a nan.  Build without contraction, as the library is:
 *   cc -O2 -ffp-contract=off -fopenmp tools/check_libm_ref_tanhf.c -lm
 * With an argument: that stride over [-22.5, 22.5] instead of 1. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static inline uint32_t asu32(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static inline float asf(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

static float my_expm1f(float x)
{
  const float o_threshold = 8.8721679688e+01f, ln2_hi = 6.9313812256e-01f, ln2_lo = 9.0580006145e-06f,
              invln2 = 1.4426950216e+00f, Q1 = -3.3333335072e-02f, Q2 = 1.5873016091e-03f, Q3 = -7.9365076090e-05f,
              Q4 = 4.0082177293e-06f, Q5 = -2.0109921195e-07f;
  float y, hi, lo, c = 0.0f, t, e, hxs, hfx, r1;
  int32_t k;
  uint32_t hx = asu32(x);
  const uint32_t xsb = hx & 0x80000000u;
  hx &= 0x7fffffffu;
  if (hx >= 0x4195b844u) { /* |x| >= 27 ln2 */
    if (hx >= 0x42b17218u) {
      if (hx > 0x7f800000u) return x + x;
      if (hx == 0x7f800000u) return xsb == 0 ? x : -1.0f;
      if (x > o_threshold) return INFINITY;
    }
    if (xsb != 0) return -1.0f;
  }
  if (hx > 0x3eb17218u) { /* |x| > 0.5 ln2 */
    if (hx < 0x3F851592u) { /* |x| < 1.5 ln2 */
      if (xsb == 0) { hi = x - ln2_hi; lo = ln2_lo; k = 1; }
      else { hi = x + ln2_hi; lo = -ln2_lo; k = -1; }
    } else {
      k = (int32_t)(invln2 * x + (xsb == 0 ? 0.5f : -0.5f));
      t = (float)k;
      hi = x - t * ln2_hi;
      lo = t * ln2_lo;
    }
    x = hi - lo;
    c = (hi - x) - lo;
  } else if (hx < 0x33000000u) { /* |x| < 2^-25 */
    return x;
  } else
    k = 0;
  hfx = 0.5f * x;
  hxs = x * hfx;
  r1 = 1.0f + hxs * (Q1 + hxs * (Q2 + hxs * (Q3 + hxs * (Q4 + hxs * Q5))));
  t = 3.0f - r1 * hfx;
  e = hxs * ((r1 - t) / (6.0f - x * t));
  if (k == 0) return x - (x * e - hxs);
  e = (x * (e - c) - c);
  e -= hxs;
  if (k == -1) return 0.5f * (x - e) - 0.5f;
  if (k == 1) {
    if (x < -0.25f) return -2.0f * (e - (x + 0.5f));
    return 1.0f + 2.0f * (x - e);
  }
  if (k <= -2 || k > 56) {
    y = 1.0f - (e - x);
    y = asf(asu32(y) + ((uint32_t)k << 23));
    return y - 1.0f;
  }
  if (k < 23) {
    t = asf(0x3f800000u - (0x1000000u >> k)); /* 1 - 2^-k */
    y = t - (e - x);
    y = asf(asu32(y) + ((uint32_t)k << 23));
  } else {
    t = asf((uint32_t)(0x7f - k) << 23); /* 2^-k */
    y = x - (e + t);
    y += 1.0f;
    y = asf(asu32(y) + ((uint32_t)k << 23));
  }
  return y;
}

static float my_tanhf(float x)
{
  const uint32_t jx = asu32(x), ix = jx & 0x7fffffffu;
  float t, z;
  if (ix >= 0x7f800000u) return (jx >> 31) ? 1.0f / x - 1.0f : 1.0f / x + 1.0f;
  if (ix < 0x41b00000u) { /* |x| < 22 */
    if (ix == 0) return x;
    if (ix < 0x24000000u) return x * (1.0f + x); /* |x| < 2^-55 */
    if (ix >= 0x3f800000u) {
      t = my_expm1f(2.0f * fabsf(x));
      z = 1.0f - 2.0f / (t + 2.0f);
    } else {
      t = my_expm1f(-2.0f * fabsf(x));
      z = -t / (t + 2.0f);
    }
  } else
    z = 1.0f - 1.0e-30f;
  return (jx >> 31) ? -z : z;
}

int main(int argc, char **argv)
{
  const uint32_t stride = argc > 1 ? (uint32_t)atoi(argv[1]) : 1u, top = asu32(22.5f);
  long n = 0, bad = 0;
  uint32_t first = 0;
#pragma omp parallel for reduction(+ : n, bad) schedule(static)
  for (int64_t u = 0; u <= (int64_t)0x7f800000u; u++) {
    if (u <= top ? u % stride : (u % 1009 && u != 0x7f800000u)) continue;
    for (int sgn = 0; sgn < 2; sgn++) {
      const float x = asf((uint32_t)u | (sgn ? 0x80000000u : 0u));
      n++;
      if (asu32(tanhf(x)) != asu32(my_tanhf(x))) {
        bad++;
#pragma omp critical
        if (!first) first = asu32(x);
      }
    }
  }
  const float nn = my_tanhf(NAN);
  printf("tanhf: n=%ld mismatches=%ld first=%a nan->%s\n", n, bad, (double)asf(first), nn != nn ? "nan" : "NOT nan");
  return bad != 0 || nn == nn;
}
