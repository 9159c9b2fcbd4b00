// rte_device.hpp -- device-side pieces shared by the RTE solver kernels (kernels_rte.hip,
// kernels_lw_scat.hip): constants, band lookup, the ordered broadband reduction and column-local
// buffer addressing.
#pragma once
#include "internal.hpp"
#include "libm_ref.hpp"

#include <cfloat>
#include <cmath>

namespace rrtmgpnn {

static constexpr float kPi = 3.14159265358979323846f;


__device__ __forceinline__ int band_of(const BandArgs &b, int g)
{
  for (int i = 0; i < b.nbnd; i++)
    if (g >= b.lims[2 * i] - 1 && g < b.lims[2 * i + 1]) return i;
  return 0;
}

static constexpr int kExpTabOff = 0, kExpTabFloats = 64;  // exp table (32 x u64) at the front of LDS

// The solvers' divisions whose operands stay in the normal range use div_rn_normal, and their exps of non-positive
// arguments ref_expf_neg (libm_ref.hpp): the bits of a / b and of glibc's expf, in fewer instructions.
// Two uses: sw_two_stream's (w0 * RT) / dd, bitwise against the reference at every operand edge tried, numerators
// below div_rn_normal's stated 2^-100 included; and the LW source's (1 - T) / t, t = tau * D, bitwise up to
// t = 2^126 and wrong beyond (0 for finite t, nan for t = inf): the LW entry points state tau * D <= 2^126
// (include/rrtmgpnn.h; tests/test_gpu_solver_edges.py).
__device__ __forceinline__ float solver_div(float a, float b) { return div_rn_normal(a, b); }
// RRTMGPNN_FAST_LIBM (opt-in tolerance build, librrtmgpnn_fastlibm.so; never the default): the solvers' exps of
// non-positive arguments use the hardware exponential (v_exp_f32, a few ulp) instead of glibc's algorithm
// evaluated in double.  Fluxes then differ from the reference's in the last bits; tests/test_gpu_tolerance.py holds
// them to the north star's 1e-3 W/m2 RMS.
#ifndef RRTMGPNN_FAST_LIBM
#define RRTMGPNN_FAST_LIBM 0
#endif
// The direct-beam transmittance exp(-tau/mu0) multiplies down every layer of a column, so its rounding errors compound:
// it keeps glibc's algorithm in the tolerance build too (with the hardware exp there, C3 SW down-flux errors reached
// 1.0e-3 W/m2 RMS, the north star's bar itself).
__device__ __forceinline__ float solver_exp_beam(float x, const uint64_t *tab) { return ref_expf_neg(x, tab); }
__device__ __forceinline__ float solver_exp_neg(float x, const uint64_t *tab)
{
#if RRTMGPNN_FAST_LIBM
  // 2^(x log2 e) on the hardware exp2 (v_exp_f32, ~1 ulp), with the product x*log2(e) carried in two parts (hi by
  // the rounded product, lo by fma residual + x*(log2(e) - hi constant)) so its rounding does not scale with |x|;
  // the lo part enters as the first-order factor (1 + lo*ln2).
  (void)tab;
  const float L = 1.44269502162933349609375f, L_lo = 1.925963033500011079E-8f, LN2 = 0.693147180559945f;
  const float t = x * L;
  float e = fmaf(x, L, -t);
  e = fmaf(x, L_lo, e);
  const float r = __builtin_amdgcn_exp2f(t);
  return (x < -0x1.9fe368p6f) ? 0.0f : fmaf(r, e * LN2, r);
#else
  return ref_expf_neg(x, tab);
#endif
}


// interpolate1D of compute_Planck_source_nn (rrtmgp/kernels/mo_gas_optics_kernels.F90:1024-1043)
__device__ __forceinline__ float interp1d(float val, float offset, float delta, int ntemp, const float *__restrict__ t)
{
  float val0 = (val - offset) / delta;
  int iv = (int)val0;  // Fortran int(): truncation
  float frac = val0 - (float)iv;
  int index = min(ntemp - 1, max(1, iv + 1));
  float lo = t[index - 1], hi = t[index];
  return lo + frac * (hi - lo);
}

// fused Planck table size in floats, padded so the ring that follows stays 16-byte aligned; jac: with the row
// B_b(tsfc + 1) of the Jacobian instances
__host__ __device__ constexpr size_t lw_btab_floats(int nbnd, int nlay, bool jac = false)
{
  return ((size_t)nbnd * (2 * nlay + 2 + (jac ? 1 : 0)) + 3) & ~(size_t)3;
}

// The fused Planck table of column icol, built by the whole block into btab (lw_btab_floats(nbnd, nlay, kJac) floats of
// LDS): band Planck values B_b(tlay(l)) at [b][l], B_b(tlev(l)) at [b][nlay+l], B_b(tsfc) at [nbnd*brow + b], with
// brow = 2*nlay + 1; interpolate1D of compute_Planck_source_nn.  The caller's barrier comes before the first read.
template <bool kJac>
__device__ __forceinline__ void lw_planck_table(float *btab, const LwPlanck &pl, int nbnd, int nlay, int icol)
{
  const int nlev = nlay + 1, brow = 2 * nlay + 1;
  const float *tl = pl.tlay + (size_t)nlay * icol, *tv = pl.tlev + (size_t)nlev * icol;
  // kBtabU entries per thread per round, their loads issued together: the temperatures, then the table pairs (a
  // loop of one entry per round waits out two dependent load latencies per entry, ~16 per block at C3)
  constexpr int kBtabU = 8;
  // kJac: one more row, B_b(tsfc + 1), at [nbnd*(brow+1) + b]
  const int ntab = nbnd * (brow + (kJac ? 2 : 1)), nrow = nbnd * brow;
  for (int i0 = threadIdx.x; i0 < ntab; i0 += kBtabU * (int)blockDim.x) {
    float T[kBtabU];
    int bb[kBtabU];
#pragma unroll
    for (int u = 0; u < kBtabU; u++) {
      const int i = min(i0 + u * (int)blockDim.x, ntab - 1);  // clamped: past-the-end entries are not stored
      int b = i < nrow ? i / brow : i - nrow;
      const int k = i < nrow ? i - b * brow : -1;
      bool plus1 = false;
      if constexpr (kJac) {
        plus1 = b >= nbnd;
        if (plus1) b -= nbnd;
      }
      bb[u] = b;
      const float *p = k < 0 ? pl.tsfc + icol : (k < nlay ? tl + k : tv + (k - nlay));  // one load, no branch
      T[u] = *p;
      if constexpr (kJac)
        if (plus1) T[u] = T[u] + 1.0f;
    }
    float v[kBtabU];
#pragma unroll
    for (int u = 0; u < kBtabU; u++)
      v[u] = interp1d(T[u], pl.tmin, pl.tdelta, pl.ntemp, pl.totplnk + (size_t)pl.ntemp * bb[u]);
#pragma unroll
    for (int u = 0; u < kBtabU; u++) {
      const int i = i0 + u * (int)blockDim.x;
      if (i < ntab) btab[i] = v[u];
    }
  }
}

// inc_2stream_by_2stream_bybnd (rte/kernels/mo_optical_props_kernels.F90:430-463) for one g-point: the
// same expressions as increment_bybnd_kernel, so the incremented properties are bit-identical.
__device__ __forceinline__ void inc_2str(float &t1, float &w1, float &g1, float t2, float w2, float g2)
{
  const float eps = 3.0f * FLT_MIN;
  const float tau12 = t1 + t2;
  const float tauscat12 = t1 * w1 + t2 * w2;
  g1 = (t1 * w1 * g1 + t2 * w2 * g2) / fmaxf(eps, tauscat12);
  w1 = tauscat12 / fmaxf(eps, tau12);
  t1 = tau12;
}

// Gauss-Jacobi quadrature of the LW no-scattering solvers (secants and weights, nmus <= 4)
struct LwAngles {
  float D[4], w[4];
  int nmus;
  const float *Dg;  // rte_lw's lw_Ds: per-(g-point, column) secants D(igpt, icol), one angle (nullptr: Gauss D)
  int rad;          // kMulti with one angle (g-point outputs): store radiances, reduce with fac as lw_solver_noscat
};

// ------------------------------------------------------------------------------------------
// By-band fluxes (ty_fluxes_byband, extensions/mo_fluxes_byband.F90; sum_byband,
// extensions/mo_fluxes_byband_kernels.F90:31-50): a band's flux starts from the band's first g-point value and adds
// the others one by one in increasing g.  The solvers' by-band instances (template flag kBand) form these sums from the
// LDS ring rows that the ordered broadband flush walks, inside that flush's barrier window, and store them to
// (nbnd, nlev, ncol) arrays; a null array is not wanted.
// ------------------------------------------------------------------------------------------
struct BandOut {
  float *up, *dn, *dir;
  BandArgs b;
};

inline BandOut band_out(const SolverExtras &ex) { return BandOut{ex.bnd_up, ex.bnd_dn, ex.bnd_dir, ex.bnd}; }

// sum_byband over g-points [lo, hi) of one row; add2: the value is r[i] + r2[i], rounded once per g-point (the SW
// total down flux from the diffuse and direct rows)
__device__ __forceinline__ float band_walk(const float *r, const float *r2, bool add2, int lo, int hi)
{
  float s = add2 ? r[lo] + r2[lo] : r[lo];
  if (add2) for (int i = lo + 1; i < hi; i++) s = s + (r[i] + r2[i]);
  else      for (int i = lo + 1; i < hi; i++) s = s + r[i];
  return s;
}

// The band sums of `n` staged levels of a ring [ncb][nq][rows][rs] (column stride cs, quantity stride qs floats; the
// levels in rows slot0 .. slot0 + n - 1, row c holding level lev0 + c*dl).  One lane per (column, quantity, level, band),
// band fastest, so a wave's stores are contiguous; the items are dealt out starting at lane t0, the first lane that the
// broadband flush leaves idle (rounded up to a wave by the caller where whole waves are idle), and wrap around the
// block.  o[q] is quantity q's output (null: skipped); dn_q: the quantity whose value is its own row plus quantity 2's
// (-1: none).  Columns at or past ncol store nothing.  Call between the flush's two barriers.
__device__ __forceinline__ void band_flush(const float *ring, int rs, int qs, int cs, int ncb, int nq, int n,
                                           int slot0, int lev0, int dl, int nlev, int icol0, int ncol, int dn_q,
                                           float *o0, float *o1, float *o2, const BandArgs &b, int t0)
{
  const int nb = b.nbnd, items = ncb * nq * n * nb, nt = (int)blockDim.x;
  int first = (int)threadIdx.x - t0;
  if (first < 0) first += nt;
  for (int it = first; it < items; it += nt) {
    const int row = it / nb, ib = it - row * nb;
    const int cq = row / n, s = row - cq * n;
    const int c = cq / nq, q = cq - c * nq;
    float *o = q == 0 ? o0 : (q == 1 ? o1 : o2);
    const int icol = icol0 + c;
    if (!o || icol >= ncol) continue;
    const float *rc = ring + (size_t)c * cs;
    const float *r = rc + (size_t)q * qs + (size_t)(slot0 + s) * rs;
    const float *r2 = rc + (size_t)2 * qs + (size_t)(slot0 + s) * rs;
    const int lo = b.lims[2 * ib] - 1, hi = b.lims[2 * ib + 1];
    o[ib + (size_t)nb * ((size_t)(lev0 + s * dl) + (size_t)nlev * icol)] = band_walk(r, r2, q == dn_q, lo, hi);
  }
}

// ------------------------------------------------------------------------------------------
// Ordered broadband reduction.  The reference sums g-points into 4 interleaved partial sums,
// partial j accumulating g = j, j+4, j+8, ... in increasing g, then ((p0+p1)+p2)+p3
// (rte/kernels/mo_rte_solver_kernels.F90:296-318 LW, :643-686 SW).  A float32 tree reduction
// differs from that by several ulp of the broadband flux (~1e-3 W/m2 at SW magnitudes), so the
// kernels reproduce the reference's order exactly: each level's per-g values are staged in an
// LDS ring of R levels; when it fills, one thread per (quantity, level) walks them sequentially.
// ------------------------------------------------------------------------------------------
// Flush `n` staged levels.  ring: [nq][R][ngpt], slot c holds level lev0 + c*dl; part: [nq][nlev][4].
// One thread per (quantity, level) walks the level's g-points with 16-byte LDS reads: element k of
// the float4 at m is g = 4m + k, so the 4 interleaved partials advance together, each in g order.
// dn_mode (SW): quantity 1 is accumulated as (s + ring1) + ring2, i.e. sums_dn + radn_dn + radn_dir.
// ngpt % 4 != 0, or seq: the reference uses sum(radn, 1) instead (one sequential sum, kept in partial 0).
// slot0: the first staged slot (the levels sit in slots slot0 .. slot0 + n - 1)
// kBand: also the by-band sums of column icol (band_flush; o0 / o1 / o2 are quantities 0 / 1 / 2's outputs)
template <int R, bool kBand = false>
__device__ __forceinline__ void ring_flush(const float *ring, float *part, int nq, int n, int lev0, int dl, int ngpt,
                                           int nlev, bool dn_mode, bool seq = false, int slot0 = 0,
                                           const BandArgs *b = nullptr, float *o0 = nullptr, float *o1 = nullptr,
                                           float *o2 = nullptr, int icol = 0)
{
  __syncthreads();
  const int t = threadIdx.x;
  if (t < nq * n) {
    const int q = t / n, c = t - q * n;
    const float *r = ring + ((size_t)q * R + slot0 + c) * ngpt;
    const float *r2 = ring + ((size_t)2 * R + slot0 + c) * ngpt;
    const bool dn = dn_mode && q == 1;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if ((ngpt & 3) == 0 && !seq) {
      const float4 *r4 = (const float4 *)r, *q4 = (const float4 *)r2;
      const int n4 = ngpt >> 2;
      if (dn) {
#pragma unroll 4
        for (int m = 0; m < n4; m++) {
          const float4 a = r4[m], b = q4[m];
          s0 = (s0 + a.x) + b.x; s1 = (s1 + a.y) + b.y; s2 = (s2 + a.z) + b.z; s3 = (s3 + a.w) + b.w;
        }
      } else {
#pragma unroll 4
        for (int m = 0; m < n4; m++) {
          const float4 a = r4[m];
          s0 = s0 + a.x; s1 = s1 + a.y; s2 = s2 + a.z; s3 = s3 + a.w;
        }
      }
    } else {
      if (dn) for (int i = 0; i < ngpt; i++) s0 = s0 + (r[i] + r2[i]);  // radn_dn = radn_dn + radn_dir; sum
      else    for (int i = 0; i < ngpt; i++) s0 = s0 + r[i];
    }
    float4 *p = (float4 *)(part + ((size_t)q * nlev + lev0 + c * dl) * 4);
    *p = make_float4(s0, s1, s2, s3);
  }
  if constexpr (kBand)
    band_flush(ring, ngpt, R * ngpt, 0, 1, nq, n, slot0, lev0, dl, nlev, icol, icol + 1, dn_mode ? 1 : -1, o0, o1, o2,
               *b, (nq * n + 63) & ~63);
  __syncthreads();
}

// ring_flush of one quantity (nq = 1, no dn_mode) for ngpt % 4 == 0 with one lane per partial: lane (s, j) walks
// partial j of slot s (ring rows `stride` floats apart) and stores it to part[lev][j] -- the same partial sums as
// ring_flush's float4 walk, in the same order, with a quarter of its instructions on the flushing wave.  With rows
// padded to stride = ngpt + 4 the lanes' rows start in different LDS banks.
// slot0: the first staged slot (the levels sit in slots slot0 .. slot0 + n - 1)
// kBand: also the by-band sums of column icol into bnd (band_flush; null: not wanted)
template <bool kBand = false>
__device__ __forceinline__ void ring_flush_lanes(const float *ring, int stride, float *part, int n, int lev0, int dl,
                                                 int ngpt, int slot0 = 0, const BandArgs *b = nullptr,
                                                 float *bnd = nullptr, int nlev = 0, int icol = 0)
{
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 4 * n) {
    const int sl = t >> 2, j = t & 3;
    const float *r = ring + (size_t)(slot0 + sl) * stride + j;
    const int n4 = ngpt >> 2;
    float sum = 0.0f;
#pragma unroll 8
    for (int m = 0; m < n4; m++) sum = sum + r[4 * m];
    part[(size_t)(lev0 + sl * dl) * 4 + j] = sum;
  }
  if constexpr (kBand)
    band_flush(ring, stride, 0, 0, 1, 1, n, slot0, lev0, dl, nlev, icol, icol + 1, -1, bnd, nullptr, nullptr, *b, 64);
  __syncthreads();
}

// ring_flush_lanes for two quantities staged in rows [2][R][stride] (the dual LW instance: all-sky, clear): lane
// (q, s, j) walks partial j of quantity q's slot s and stores it to part[q][lev][j] (part [2][nlev][4]) -- the same
// partial sums in the same order, 8 lanes per level within one wave (8 * R <= 64)
template <int R>
__device__ __forceinline__ void ring_flush_lanes2(const float *ring, int stride, float *part, int nlev, int n, int lev0,
                                                  int dl, int ngpt)
{
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 8 * n) {
    const int q = t >= 4 * n ? 1 : 0, u = t - 4 * n * q, sl = u >> 2, j = u & 3;
    const float *r = ring + (size_t)(q * R + sl) * stride + j;
    const int n4 = ngpt >> 2;
    float sum = 0.0f;
#pragma unroll 8
    for (int m = 0; m < n4; m++) sum = sum + r[4 * m];
    part[((size_t)q * nlev + lev0 + sl * dl) * 4 + j] = sum;
  }
  __syncthreads();
}

__device__ __forceinline__ float combine4(const float *p) { return ((p[0] + p[1]) + p[2]) + p[3]; }

// The SW solvers' flush for blocks that hold `ncb` columns: ring [ncb][3][R][ngpt] (up, dif, dir of column c at
// ring + c*3*R*ngpt).  Each (column, quantity, level) thread forms the level's complete ordered sum -- the same
// partials and the same ((p0 + p1) + p2) + p3 as ring_flush + combine4 -- and stores it straight to the flux
// array: up, dn (= dif + dir, dn_mode) and dir.  Columns at or past ncol (the grid's last block) store nothing.
// kTotal: the down slot already holds the total (diffuse + direct) g-point flux, as sw_solver_2stream forms it when it
// saves g-point fluxes (:660-670): the down sum is s + total instead of (s + diffuse) + direct
// stride: floats per ring row (ngpt, or ngpt padded so that the rows the flush threads walk together fall in different
// LDS banks)
// kBand: also the by-band sums (band_flush), the down value formed as dif + dir per g-point unless kTotal
// kSkies (the dual clear + all-sky instances, ncb = 2): the two "columns" of the ring are the two skies of column icol0
// -- ring column 0 stores to o_up / o_dn / o_dir, ring column 1 to c_up / c_dn / c_dir, both at column icol0
// kSfc (rrtmgpnn_solver_request_sfc_byband): the by-band sums of the one level in slot sfc_slot (the surface; < 0: not
// among this flush's levels) into bo's (nbnd, ncol) arrays -- band_flush of that slot alone, with n = 1 and nlev = 1
template <int R, bool kTotal = false, bool kBand = false, bool kSkies = false, bool kSfc = false>
__device__ __forceinline__ void ring_flush_sw(const float *ring, int ncb, int n, int lev0, int dl, int ngpt, int nlev,
                                              int icol0, int ncol, float *o_up, float *o_dn, float *o_dir,
                                              int stride = 0, int slot0 = 0, const BandOut *bo = nullptr,
                                              float *c_up = nullptr, float *c_dn = nullptr, float *c_dir = nullptr,
                                              int sfc_slot = -1)
{
  __syncthreads();
  const int t = threadIdx.x;
  const int rs = stride ? stride : ngpt;
  if (t < 3 * ncb * n) {
    const int c = t / (3 * n), rem = t - c * 3 * n, q = rem / n, s = rem - q * n;
    const float *rc = ring + (size_t)c * 3 * R * rs;
    const float *r = rc + ((size_t)q * R + slot0 + s) * rs;
    const float *r2 = rc + ((size_t)2 * R + slot0 + s) * rs;
    const bool dn = q == 1;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if ((ngpt & 3) == 0) {
      const float4 *r4 = (const float4 *)r, *q4 = (const float4 *)r2;
      const int n4 = ngpt >> 2;
      if (dn && !kTotal) {
#pragma unroll 4
        for (int m = 0; m < n4; m++) {
          const float4 a = r4[m], b = q4[m];
          s0 = (s0 + a.x) + b.x; s1 = (s1 + a.y) + b.y; s2 = (s2 + a.z) + b.z; s3 = (s3 + a.w) + b.w;
        }
      } else {
#pragma unroll 4
        for (int m = 0; m < n4; m++) {
          const float4 a = r4[m];
          s0 = s0 + a.x; s1 = s1 + a.y; s2 = s2 + a.z; s3 = s3 + a.w;
        }
      }
    } else {
      if (dn && !kTotal) for (int i = 0; i < ngpt; i++) s0 = s0 + (r[i] + r2[i]);
      else    for (int i = 0; i < ngpt; i++) s0 = s0 + r[i];
    }
    const int icol = kSkies ? icol0 : icol0 + c;
    if (icol < ncol) {
      float *o = q == 0 ? o_up : (q == 1 ? o_dn : o_dir);
      if constexpr (kSkies) o = c == 0 ? o : (q == 0 ? c_up : (q == 1 ? c_dn : c_dir));
      o[lev0 + s * dl + (size_t)nlev * icol] = ((s0 + s1) + s2) + s3;
    }
  }
  if constexpr (kBand)
    band_flush(ring, rs, R * rs, 3 * R * rs, ncb, 3, n, slot0, lev0, dl, nlev, icol0, ncol, kTotal ? -1 : 1, bo->up,
               bo->dn, bo->dir, bo->b, (3 * ncb * n + 63) & ~63);
  if constexpr (kSfc)
    if (sfc_slot >= 0)
      band_flush(ring, rs, R * rs, 3 * R * rs, ncb, 3, 1, sfc_slot, 0, 0, 1, icol0, ncol, 1, bo->up, bo->dn, bo->dir,
                 bo->b, (3 * ncb * n + 63) & ~63);
  __syncthreads();
}

// The same sums with one lane per partial (ngpt % 4 == 0): lane (q, c, s, j) walks partial j of quantity q, column c,
// ring slot slot0 + s -- 4 words per step instead of a float4 per (q, c, s) -- and the four partials of a row are then
// combined ((p0 + p1) + p2) + p3 by the row's lane j = 0 (partials fetched from lanes j = 1..3 of its quad).  Lanes
// are ordered quantity-major, so with 64 lanes per (quantity) group a wave walks one quantity only: the down sums (two
// adds per step) and the others do not share a wave's instruction stream.  Same partials, same additions, same order,
// same bits as ring_flush_sw; about a quarter of its instructions on the critical wave.
// ring_flush_sw_lanes maps a lane's row to its column with three comparisons: at most this many columns per block
// (the SW launchers refuse more before launching)
constexpr int kFlushLanesMaxCols = 4;

// kSkies, kSfc: as ring_flush_sw's
template <int R, bool kTotal = false, bool kBand = false, bool kSkies = false, bool kSfc = false>
__device__ __forceinline__ void ring_flush_sw_lanes(const float *ring, int ncb, int n, int lev0, int dl, int ngpt,
                                                    int nlev, int icol0, int ncol, float *o_up, float *o_dn,
                                                    float *o_dir, int stride, int slot0 = 0,
                                                    const BandOut *bo = nullptr, float *c_up = nullptr,
                                                    float *c_dn = nullptr, float *c_dir = nullptr, int sfc_slot = -1)
{
  __syncthreads();
  const int t = threadIdx.x;
  const int per_q = ncb * n * 4;  // lanes per quantity
  if (t < 3 * per_q) {  // idle lanes of the last wave walk nothing (the branch is per lane only in that wave)
    // the lane's (quantity, column, slot, partial) by comparisons and 24-bit products: integer division by the
    // runtime per_q and n took ~40 dependent VALU ops (quarter-rate multiplies among them) before every flush
    const int q = (t >= per_q) + (t >= 2 * per_q);  // three quantities
    const int rem = t - (int)__umul24((unsigned)q, (unsigned)per_q), row = rem >> 2, j = rem & 3;
    const int c = (ncb > 1 && row >= n) + (ncb > 2 && row >= 2 * n) + (ncb > 3 && row >= 3 * n);  // ncb <= kFlushLanesMaxCols
    const int sl = row - (int)__umul24((unsigned)c, (unsigned)n);
    // LDS offsets (well under 2^24 floats)
    const int rc = (int)__umul24((unsigned)c, (unsigned)(3 * R * stride)) + j;
    const float *r = ring + rc + (int)__umul24((unsigned)(q * R + slot0 + sl), (unsigned)stride);
    const float *r2 = ring + rc + (int)__umul24((unsigned)(2 * R + slot0 + sl), (unsigned)stride);
    const int n4 = ngpt >> 2;
    float sum = 0.0f;
    if (q == 1 && !kTotal) {
#pragma unroll 8
      for (int m = 0; m < n4; m++) sum = (sum + r[4 * m]) + r2[4 * m];
    } else {
#pragma unroll 8
      for (int m = 0; m < n4; m++) sum = sum + r[4 * m];
    }
    // the quad's partials p0..p3 sit in lanes j = 0..3 of consecutive threads (per_q is a multiple of 4)
    const float p1 = __shfl_down(sum, 1, 4), p2 = __shfl_down(sum, 2, 4), p3 = __shfl_down(sum, 3, 4);
    const int icol = kSkies ? icol0 : icol0 + c;
    if (j == 0 && icol < ncol) {
      float *o = q == 0 ? o_up : (q == 1 ? o_dn : o_dir);
      if constexpr (kSkies) o = c == 0 ? o : (q == 0 ? c_up : (q == 1 ? c_dn : c_dir));
      o[lev0 + (dl > 0 ? sl : -sl) + (size_t)nlev * icol] = ((sum + p1) + p2) + p3;  // dl = +-1
    }
  }
  if constexpr (kBand)
    band_flush(ring, stride, R * stride, 3 * R * stride, ncb, 3, n, slot0, lev0, dl, nlev, icol0, ncol,
               kTotal ? -1 : 1, bo->up, bo->dn, bo->dir, bo->b, (3 * per_q + 63) & ~63);
  if constexpr (kSfc)
    if (sfc_slot >= 0)
      band_flush(ring, stride, R * stride, 3 * R * stride, ncb, 3, 1, sfc_slot, 0, 0, 1, icol0, ncol, 1, bo->up, bo->dn,
                 bo->dir, bo->b, (3 * per_q + 63) & ~63);
  __syncthreads();
}

// Columns per block for a solver whose column occupies `lanes` lanes: the count (1, 2 or 4, at most 512 lanes)
// that leaves the fewest idle lanes in the block's last wave -- the two-per-lane SW kernel's 112 lanes per column
// (224 g-points): 4 columns = 448 lanes = 7 full waves instead of 2 waves with 16 idle lanes each (C4 -5 %).
inline int columns_per_block(int lanes)
{
  int best = 1;
  double best_waste = 1e30;
  for (int k = 1; k <= 4; k *= 2) {
    if (k * lanes > 512) break;
    const double waste = (double)((k * lanes + 63) / 64 * 64) / (k * lanes);
    if (waste < best_waste - 1e-9) { best = k; best_waste = waste; }
  }
  return best;
}

// ------------------------------------------------------------------------------------------
// Column-local addressing.  Every solver array is (ngpt, n, ncol) with the column block uniform per
// workgroup, so each array gets a per-column buffer descriptor built from wave-uniform values: a
// load is `buffer_load v, voff=g*4, s_rsrc, soff=layer*ngpt*4` -- no per-lane 64-bit address math,
// the layer offset lives in an SGPR.
// ------------------------------------------------------------------------------------------
// A buffer offset past every solver array's range: raw buffer stores there are dropped, loads return 0 (the
// range check covers the VGPR offset; the SGPR layer offset is added past it), so idle lanes and padding steps
// can issue the same stores as the others without a branch.
static constexpr uint32_t kBufOOB = 0x7ffff000u;

// The cache policy of one global stream: the raw buffer builtins' last (immediate) argument, so a template argument of
// every load and store helper.  kNT marks lines that nothing reads again (the `nt` modifier on gfx950); the scope bits
// (sc0 = 1, sc1 = 16) change coherence and stay 0 everywhere.  The out-of-range offsets above do not depend on it.
// Which stream carries which policy: the kCp* constants beside each kernel's tuning constants (DESIGN.md section 3,
// "Cache policies per stream").
enum class CachePolicy : int { kDefault = 0, kNT = 2 };

struct ColArr {
  __amdgpu_buffer_rsrc_t r;
  __device__ __forceinline__ ColArr() = default;
  __device__ __forceinline__ ColArr(const float *base, size_t col_off, uint32_t bytes)
      : r(__builtin_amdgcn_make_buffer_rsrc((void *)(base + col_off), 0, (int)bytes, 0x00020000)) {}
  template <CachePolicy CP = CachePolicy::kDefault>
  __device__ __forceinline__ float ld(uint32_t voff, uint32_t soff) const
  {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, (int)CP));
  }
  template <CachePolicy CP = CachePolicy::kDefault>
  __device__ __forceinline__ void st(float v, uint32_t voff, uint32_t soff) const
  {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, voff, soff, (int)CP);
  }
};

}  // namespace rrtmgpnn
