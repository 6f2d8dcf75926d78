// quantize_host.cpp -- the layer-0 input quantiser on the host: out[i] = q8(x[i] * s), q8 = round half
// to even then clamp to [-128, 127] (rnnt_device.hpp q8, oracle_q8), for callers that send int8 features
// to the engine (rnnt_quantize_features_host, include/rnnt_mi355x.h).  Host code only.
//
// Bit-identical to the device kernel: one fp32 multiply (no contraction: -ffp-contract=off), rounding
// to nearest even in the default rounding mode, and a clamp in which NaN takes the device's way --
// fminf(fmaxf(NaN, -128), 127) = -128 there.
//
// Two bodies, picked at run time (roundps / AVX2 are not in the x86-64 baseline):
//  * AVX2, 32 features per iteration: vmulps; the clamp first, in fp32 -- vminps(127, v) keeps a NaN
//    (the instruction returns its second operand when either is NaN), vmaxps(v, -128) then turns it into
//    -128, and +-inf / 1e30 land on the bounds; vcvtps2dq rounds to nearest even (clamping before the
//    rounding gives the same integers: the bounds are integers and rounding is monotonic); vpackssdw +
//    vpacksswb narrow (their saturation never acts on [-128, 127]); one vpermd undoes the packs'
//    128-bit lane interleave.  Unaligned loads and stores; the last n % 32 features go the plain way.
//  * plain C++ (rintf per element where the target has no rounding instruction): the tail and the
//    fallback.
#include "quantize_host.hpp"

#include <math.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace rnnt {

namespace {

void quantize_plain(const float* x, int64_t n, float s, int8_t* out) {
  for (int64_t i = 0; i < n; ++i) {
    float r = rintf(x[i] * s);
    r = r > -128.0f ? r : -128.0f;  // false for NaN as well: -128
    r = r < 127.0f ? r : 127.0f;
    out[i] = (int8_t)(int32_t)r;
  }
}

#if defined(__x86_64__)
// eight features -> eight int32 in [-128, 127]
__attribute__((target("avx2"))) inline __m256i q8x8(const float* p, __m256 vs) {
  const __m256 v = _mm256_mul_ps(_mm256_loadu_ps(p), vs);
  return _mm256_cvtps_epi32(_mm256_max_ps(_mm256_min_ps(_mm256_set1_ps(127.0f), v), _mm256_set1_ps(-128.0f)));
}

__attribute__((target("avx2"))) void quantize_avx2(const float* x, int64_t n, float s, int8_t* out) {
  const __m256 vs = _mm256_set1_ps(s);
  const __m256i order = _mm256_setr_epi32(0, 4, 1, 5, 2, 6, 3, 7);
  int64_t i = 0;
  for (; i + 32 <= n; i += 32) {
    const __m256i ab = _mm256_packs_epi32(q8x8(x + i, vs), q8x8(x + i + 8, vs));        // per 128-bit lane: a | b
    const __m256i cd = _mm256_packs_epi32(q8x8(x + i + 16, vs), q8x8(x + i + 24, vs));  //                   c | d
    const __m256i b8 = _mm256_packs_epi16(ab, cd);  // dwords: a0 b0 c0 d0 | a1 b1 c1 d1
    _mm256_storeu_si256((__m256i*)(out + i), _mm256_permutevar8x32_epi32(b8, order));
  }
  quantize_plain(x + i, n - i, s, out + i);
}
#endif

}  // namespace

void quantize_features_host(const float* x, int64_t n, float s, int8_t* out) {
#if defined(__x86_64__)
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (avx2) return quantize_avx2(x, n, s, out);
#endif
  quantize_plain(x, n, s, out);
}

}  // namespace rnnt
