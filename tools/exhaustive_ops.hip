// exhaustive_ops.hip -- checks the shortened correctly-rounded sequences and the libm restatements that the solvers and
// MLPs use against IEEE / glibc results on EVERY float of their domains, on the GPU itself (v_rcp_f32 / v_sqrt_f32 are
// hardware approximations that a host cannot emulate bit for bit).  Test tool, not product code.
//
// The "shipped:" variants call the product's own functions through its headers (csrc/libm_ref.hpp, rte_device.hpp,
// x2_device.hpp; the packed forms on both lanes, lane y holding the operand at the mirrored index of the run), so a
// change to a header is what gets checked.  The local copies below remain only as the alternative candidates.
//
//   rcp    : 1/b, b in [2^-60, 2^60]       rcp_rn_normal, x2::rcp2 and candidates
//   sqrt   : sqrtf(x), x in [2^-20, 2^20]  sqrt_rn_normal, x2::sqrt2 and candidates
//   soft   : x/(|x|+1), every finite x     div_softsign and candidates
//   divlw  : (1-T)/t, T = ref_expf_neg(-t), every t in (sqrt(FLT_EPSILON), 2^126]: solver_div, x2::div2
//   divlw> : the same for every t in (2^126, inf]: outside solver_div's stated domain, reported for the record
//   divsw  : a/dd, every dd in [eps, 1] and [-4, -eps], a in {0, 2^-100, 1e-20, 1e-3, 0.37, 1, 50, 100}: solver_div, div2
//   exp    : ref_expf_neg and ref_expf_neg_batch<4> (LDS table) on every float of [-105, -0], every 1009th float below
//            that, and -inf, against the host's expf evaluated in this program
//   log    : ref_logf_nb (and ref_logf) on every positive finite float against the host's logf
//   cos    : ref_cosf on every float of [0, pi] against the host's cosf
//   tanh   : ref_tanhf (the MLPs' tanh activation) on every float of [-10, 10] against the host's tanhf
//
// reference of the divisions and roots: the compiler's IEEE sequences (default flags: correctly rounded f32 division
// and sqrt), cross-checked with double-precision evaluations rounded once (innocuous double rounding for / and sqrt).
// Output: one line per (op, variant): mismatches against the reference and the first mismatching input.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "libm_ref.hpp"
#include "x2_device.hpp"

using rrtmgpnn::x2::f2;

__device__ __forceinline__ float rcp_cur(float b)
{
  float r = __builtin_amdgcn_rcpf(b);
  r = fmaf(fmaf(-b, r, 1.0f), r, r);
  float q = r;
  q = fmaf(fmaf(-b, q, 1.0f), r, q);
  return fmaf(fmaf(-b, q, 1.0f), r, q);
}
// Newton step, one correction
__device__ __forceinline__ float rcp_a(float b)
{
  float r = __builtin_amdgcn_rcpf(b);
  r = fmaf(fmaf(-b, r, 1.0f), r, r);
  return fmaf(fmaf(-b, r, 1.0f), r, r);
}
// no Newton step, two corrections
__device__ __forceinline__ float rcp_b(float b)
{
  const float r = __builtin_amdgcn_rcpf(b);
  float q = fmaf(fmaf(-b, r, 1.0f), r, r);
  return fmaf(fmaf(-b, q, 1.0f), r, q);
}
__device__ __forceinline__ float sqrt_cur(float x)
{
  const float s = __builtin_amdgcn_sqrtf(x);
  const float sm = __uint_as_float(__float_as_uint(s) - 1u), sp = __uint_as_float(__float_as_uint(s) + 1u);
  const float em = fmaf(-sm, s, x), ep = fmaf(-sp, s, x);
  float r = (em <= 0.0f) ? sm : s;
  return (ep > 0.0f) ? sp : r;
}
// the hardware estimate alone, and with only one of the two one-ulp corrections
__device__ __forceinline__ float sqrt_raw(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float sqrt_up(float x)
{
  const float s = __builtin_amdgcn_sqrtf(x);
  const float sp = __uint_as_float(__float_as_uint(s) + 1u);
  return (fmaf(-sp, s, x) > 0.0f) ? sp : s;
}
__device__ __forceinline__ float sqrt_dn(float x)
{
  const float s = __builtin_amdgcn_sqrtf(x);
  const float sm = __uint_as_float(__float_as_uint(s) - 1u);
  return (fmaf(-sm, s, x) <= 0.0f) ? sm : s;
}
__device__ __forceinline__ float sqrt_d(float x) { return (float)__builtin_amdgcn_sqrt((double)x); }
__device__ __forceinline__ float div_cur(float a, float b)
{
  float r = __builtin_amdgcn_rcpf(b);
  r = fmaf(fmaf(-b, r, 1.0f), r, r);
  float q = a * r;
  q = fmaf(fmaf(-b, q, a), r, q);
  return fmaf(fmaf(-b, q, a), r, q);
}
__device__ __forceinline__ float div_a(float a, float b)
{
  const float r = __builtin_amdgcn_rcpf(b);
  float q = a * r;
  q = fmaf(fmaf(-b, q, a), r, q);
  return fmaf(fmaf(-b, q, a), r, q);
}

// no Newton step, two corrections on the negated residual (b*q - a): the same arithmetic for nonzero residuals, and
// a -0 quotient keeps its sign
__device__ __forceinline__ float div_b(float a, float b)
{
  const float r = __builtin_amdgcn_rcpf(b);
  float q = a * r;
  q = fmaf(-fmaf(b, q, -a), r, q);
  return fmaf(-fmaf(b, q, -a), r, q);
}

constexpr int kVar = 10;
enum Op { RCP = 0, SQRT, SOFT, DIVLW, DIVSW, EXP, LOG, COS, TANH };

struct Acc {
  unsigned long long c[kVar] = {};
  uint32_t f[kVar] = {};
  __device__ __forceinline__ void cmp(int j, float v, float ref, uint32_t u)
  {
    if (__float_as_uint(v) != __float_as_uint(ref)) {
      if (!c[j]) f[j] = u;
      c[j]++;
    }
  }
};

// Element k of a run is the float with bits lo + k*stride.  One thread per `per` consecutive elements of the chunk
// [k0, k0 + nchunk) of a run of n; per-thread mismatch counts and first bad input, stored with vector stores.  ref:
// the host's results for the chunk (EXP, LOG, COS, TANH); num: the numerator (DIVSW).
template <int OP>
__global__ void check(uint32_t lo, uint32_t stride, uint64_t n, uint64_t k0, uint64_t nchunk, uint32_t per,
                      const float *__restrict__ ref, float num, unsigned long long *cnt, uint32_t *first)
{
  using namespace rrtmgpnn;
  __shared__ uint64_t etab[32];
  load_exp_table(etab);
  __syncthreads();
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  Acc acc;
  auto bits = [&](uint64_t k) { return lo + (uint32_t)(k * stride); };
  for (uint32_t i = 0; i < per; i += 4) {
    const uint64_t kb = k0 + t * per + i;
    if (kb >= k0 + nchunk) break;
    if constexpr (OP == EXP) {
      float x[4], yb[4];
      for (int m = 0; m < 4; m++) x[m] = __uint_as_float(bits(kb + m < k0 + nchunk ? kb + m : k0 + nchunk - 1));
      ref_expf_neg_batch<4>(x, yb, etab);
      for (int m = 0; m < 4; m++) {
        if (kb + m >= k0 + nchunk) break;
        const float r = ref[kb + m - k0];
        acc.cmp(0, ref_expf_neg(x[m], etab), r, __float_as_uint(x[m]));
        acc.cmp(1, yb[m], r, __float_as_uint(x[m]));
      }
      continue;
    }
    for (int m = 0; m < 4; m++) {
      const uint64_t k = kb + m;
      if (k >= k0 + nchunk) break;
      const uint32_t u = bits(k), up = bits(n - 1 - k);  // up: the operand lane y of the packed forms holds
      const float x = __uint_as_float(u), xp = __uint_as_float(up);
      if constexpr (OP == RCP) {
        const float r = 1.0f / x;
        acc.cmp(kVar - 1, r, (float)(1.0 / (double)x), u);
        acc.cmp(0, rcp_cur(x), r, u); acc.cmp(1, rcp_a(x), r, u); acc.cmp(2, rcp_b(x), r, u);
        acc.cmp(3, rcp_rn_normal(x), r, u);
        const f2 p = x2::rcp2((f2){x, xp});
        acc.cmp(4, p.x, r, u); acc.cmp(5, p.y, 1.0f / xp, up);
      } else if constexpr (OP == SQRT) {
        const float r = sqrtf(x);
        acc.cmp(kVar - 1, r, (float)sqrt((double)x), u);
        acc.cmp(0, sqrt_cur(x), r, u); acc.cmp(1, sqrt_d(x), r, u); acc.cmp(2, sqrt_raw(x), r, u);
        acc.cmp(3, sqrt_up(x), r, u); acc.cmp(4, sqrt_dn(x), r, u);
        acc.cmp(5, sqrt_rn_normal(x), r, u);
        const f2 p = x2::sqrt2((f2){x, xp});
        acc.cmp(6, p.x, r, u); acc.cmp(7, p.y, sqrtf(xp), up);
      } else if constexpr (OP == SOFT) {
        if (!(fabsf(x) < 3.0e38f)) continue;  // finite x; |x| + 1 below inf
        const float b = fabsf(x) + 1.0f, r = x / b;
        acc.cmp(kVar - 1, r, (float)((double)x / (double)b), u);
        acc.cmp(0, div_cur(x, b), r, u); acc.cmp(1, div_a(x, b), r, u); acc.cmp(2, div_b(x, b), r, u);
        acc.cmp(3, div_softsign(x, b), r, u);
      } else if constexpr (OP == DIVLW || OP == DIVSW) {
        // LW: (1 - T) / t as lw_noscat_kernel forms it; SW: (w0 * RT) / dd of sw_two_stream, numerator given
        const float a = OP == DIVLW ? 1.0f - ref_expf_neg(-x, etab) : num;
        const float ap = OP == DIVLW ? 1.0f - ref_expf_neg(-xp, etab) : num;
        const float r = a / x;
        acc.cmp(kVar - 1, r, (float)((double)a / (double)x), u);
        acc.cmp(0, solver_div(a, x), r, u);
        const f2 p = x2::div2((f2){a, ap}, (f2){x, xp});
        acc.cmp(1, p.x, r, u); acc.cmp(2, p.y, ap / xp, up);
        acc.cmp(3, x2::div2(a, x), r, u);  // the one-g-point-per-lane overload
      } else if constexpr (OP == LOG) {
        acc.cmp(0, ref_logf_nb(x), ref[k - k0], u); acc.cmp(1, ref_logf(x), ref[k - k0], u);
      } else if constexpr (OP == COS) {
        acc.cmp(0, ref_cosf(x), ref[k - k0], u);
      } else if constexpr (OP == TANH) {
        acc.cmp(0, ref_tanhf(x), ref[k - k0], u);
      }
    }
  }
  for (int j = 0; j < kVar; j++) {
    cnt[t * kVar + j] = acc.c[j];
    first[t * kVar + j] = acc.f[j];
  }
}

constexpr uint64_t kChunk = 1ull << 26;  // elements per launch
constexpr uint32_t kPer = 256;           // elements per thread
constexpr int kThreads = 256, kHostThreads = 16;

#define HIP_OK(e)                                                               \
  do {                                                                          \
    if ((e) != hipSuccess) { printf("%s failed\n", #e); exit(1); }              \
  } while (0)

static unsigned long long *d_cnt;
static uint32_t *d_first;
static float *d_ref;
static std::vector<float> h_ref;

// the host's libm on the chunk's inputs, split over at most kHostThreads threads
static void host_reference(float (*fn)(float), uint32_t lo, uint32_t stride, uint64_t k0, uint64_t nchunk)
{
  std::vector<std::thread> th;
  const uint64_t each = (nchunk + kHostThreads - 1) / kHostThreads;
  for (int w = 0; w < kHostThreads; w++) {
    const uint64_t b = w * each, e = std::min(nchunk, b + each);
    if (b >= e) break;
    th.emplace_back([=] {
      for (uint64_t i = b; i < e; i++) {
        const uint32_t u = lo + (uint32_t)((k0 + i) * stride);
        float x;
        memcpy(&x, &u, 4);
        h_ref[i] = fn(x);
      }
    });
  }
  for (auto &t : th) t.join();
}

template <int OP>
static void run(const char *name, uint32_t lo, uint32_t hi, const char *const *vnames, uint32_t stride = 1,
                float (*host_fn)(float) = nullptr, float num = 0.0f)
{
  const uint64_t n = ((uint64_t)hi - lo) / stride + 1;
  const uint64_t max_thr = kChunk / kPer;
  std::vector<unsigned long long> hc(max_thr * kVar), tot(kVar, 0);
  std::vector<uint32_t> hf(max_thr * kVar), f(kVar, 0);
  for (uint64_t k0 = 0; k0 < n; k0 += kChunk) {
    const uint64_t nchunk = std::min(kChunk, n - k0);
    const uint64_t nthr = (nchunk + kPer - 1) / kPer, blocks = (nthr + kThreads - 1) / kThreads;
    if (host_fn) {
      host_reference(host_fn, lo, stride, k0, nchunk);
      HIP_OK(hipMemcpy(d_ref, h_ref.data(), sizeof(float) * nchunk, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(check<OP>, dim3((unsigned)blocks), dim3(kThreads), 0, 0, lo, stride, n, k0, nchunk, kPer, d_ref,
                       num, d_cnt, d_first);
    if (hipDeviceSynchronize() != hipSuccess) { printf("%s: kernel failed\n", name); exit(1); }
    HIP_OK(hipMemcpy(hc.data(), d_cnt, sizeof(unsigned long long) * blocks * kThreads * kVar, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hf.data(), d_first, sizeof(uint32_t) * blocks * kThreads * kVar, hipMemcpyDeviceToHost));
    for (uint64_t t = 0; t < blocks * kThreads; t++)
      for (int j = 0; j < kVar; j++) {
        if (hc[t * kVar + j] && !tot[j]) f[j] = hf[t * kVar + j];
        tot[j] += hc[t * kVar + j];
      }
  }
  for (int j = 0; j < kVar; j++) {
    if (!vnames[j]) continue;
    float fx;
    memcpy(&fx, &f[j], 4);
    printf("%-7s %-32s inputs %llu mismatches %llu first %a\n", name, vnames[j], (unsigned long long)n, tot[j],
           tot[j] ? (double)fx : 0.0);
  }
  fflush(stdout);
}

static uint32_t fbits(float x)
{
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}

int main()
{
  const uint64_t max_thr = (kChunk / kPer + kThreads - 1) / kThreads * kThreads;
  HIP_OK(hipMalloc(&d_cnt, sizeof(unsigned long long) * max_thr * kVar));
  HIP_OK(hipMalloc(&d_first, sizeof(uint32_t) * max_thr * kVar));
  HIP_OK(hipMalloc(&d_ref, sizeof(float) * kChunk));
  h_ref.resize(kChunk);

  const char *rv[kVar] = {"current(newton+2corr)", "newton+1corr", "2corr", "shipped:rcp_rn_normal", "shipped:rcp2.x",
                          "shipped:rcp2.y", nullptr, nullptr, nullptr, "ref-vs-double"};
  run<RCP>("rcp", 0x21800000u /* 2^-60 */, 0x5d800000u /* 2^60 */, rv);
  const char *sv[kVar] = {"current", "f64-sqrt", "raw", "up-only", "down-only", "shipped:sqrt_rn_normal",
                          "shipped:sqrt2.x", "shipped:sqrt2.y", nullptr, "ref-vs-double"};
  run<SQRT>("sqrt", 0x35800000u /* 2^-20 */, 0x49800000u /* 2^20 */, sv);
  run<SQRT>("sqrt<", 0x38d1b717u /* 1e-4 */, 0x40800000u /* 4 */, sv);
  const char *dv[kVar] = {"current(newton+2corr)", "2corr", "2corr-negres", "shipped:div_softsign", nullptr, nullptr,
                          nullptr, nullptr, nullptr, "ref-vs-double"};
  run<SOFT>("soft+", 0x00000000u, 0x7f7fffffu, dv);
  run<SOFT>("soft-", 0x80000000u, 0xff7fffffu, dv);
  // below 2^126 in magnitude (the documented domain)
  run<SOFT>("soft+<", 0x00000000u, 0x7e7fffffu, dv);
  run<SOFT>("soft-<", 0x80000000u, 0xfe7fffffu, dv);

  // the solvers' divisions in their two uses
  const char *lv[kVar] = {"shipped:solver_div", "shipped:div2.x", "shipped:div2.y", "shipped:div2(scalar)", nullptr,
                          nullptr, nullptr, nullptr, nullptr, "ref-vs-double"};
  run<DIVLW>("divlw", fbits(sqrtf(FLT_EPSILON)) + 1, 0x7e800000u /* 2^126 */, lv);
  // past the stated domain, for the record (v_rcp_f32 returns 0 where 1/t is subnormal, so every quotient is 0 there,
  // and a nan at t = inf): reported, not required to match
  const char *lv2[kVar] = {"solver_div(out-of-domain)"};
  run<DIVLW>("divlw>", 0x7e800001u, 0x7f800000u /* inf */, lv2);
  const char *wv[kVar] = {"shipped:solver_div", "shipped:div2.x", "shipped:div2.y", "shipped:div2(scalar)", nullptr,
                          nullptr, nullptr, nullptr, nullptr, "ref-vs-double"};
  const float nums[8] = {0.0f, 0x1p-100f, 1e-20f, 1e-3f, 0.37f, 1.0f, 50.0f, 100.0f};
  for (int i = 0; i < 8; i++) {
    char nm[16];
    snprintf(nm, sizeof nm, "divsw+%d", i);
    run<DIVSW>(nm, fbits(FLT_EPSILON), 0x3f800000u /* 1 */, wv, 1, nullptr, nums[i]);
    snprintf(nm, sizeof nm, "divsw-%d", i);
    run<DIVSW>(nm, fbits(-FLT_EPSILON), 0xc0800000u /* -4 */, wv, 1, nullptr, nums[i]);
  }

  // the libm restatements against the host's libm
  const char *ev[kVar] = {"shipped:ref_expf_neg", "shipped:ref_expf_neg_batch4"};
  run<EXP>("exp", 0x80000000u /* -0 */, 0xc2d20000u /* -105 */, ev, 1, expf);
  run<EXP>("exp<", 0xc2d20001u, 0xff7fffffu /* -FLT_MAX */, ev, 1009, expf);
  run<EXP>("exp-inf", 0xff800000u, 0xff800000u, ev, 1, expf);
  const char *gv[kVar] = {"shipped:ref_logf_nb", "shipped:ref_logf"};
  run<LOG>("log", 0x00000001u, 0x7f7fffffu, gv, 1, logf);
  const char *cv[kVar] = {"shipped:ref_cosf"};
  run<COS>("cos", 0x00000000u, 0x40490fdbu /* pi */, cv, 1, cosf);
  const char *tv[kVar] = {"shipped:ref_tanhf"};
  run<TANH>("tanh+", 0x00000000u, 0x41200000u /* 10 */, tv, 1, tanhf);
  run<TANH>("tanh-", 0x80000000u, 0xc1200000u /* -10 */, tv, 1, tanhf);
  return 0;
}
