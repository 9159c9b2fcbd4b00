// kernels_mcica.hip -- McICA cloud sampling for gfx950 (extensions/cloud_optics/mo_cloud_sampling.F90).
//
//  * sampled_mask_kernel : sampled_mask_max_ran (:125-192) and sampled_mask_exp_ran (:200-285): the T/F cloud mask of
//                          every (g-point, layer, column) from the caller's random numbers, as a byte mask for the class
//                          layer and / or a packed mask (one bit per g-point) for the solvers' fused increment
//  * draw_samples_kernel : apply_cloud_mask (:291-307): the band value where the mask is set, else 0
//  * the seeded route (no reference counterpart): sampled_mask_kernel<kExp, true> draws its random numbers itself, and
//    mcica_randoms_kernel writes the same stream out as an array (the generator is described below)
//  * the compact masks (no reference counterpart): sampled_mask_kernel<kExp, kSeeded, true> samples the packed mask of
//    a block compacted to its daylit columns (rrtmgpnn_daylit_plan), dense row j from source column idx[j]
//
// The extension predates this fork's layout (as mo_heating_rates does); here randoms and both masks are
// (ngpt, nlay, ncol), cloud_frac (nlay, ncol) and overlap_param (nlay-1, ncol), first index fastest.
//
// Mask kernel: one block per column, lane = g-point (striding by the block when ngpt exceeds it).  The layers are
// walked in array order as the reference walks them, the carried random deviate in a register; the only array
// streamed is randoms, kMaskPf layers of it in flight per lane (the seeded instances stream none).  The reference's
// first / last cloudy layer bounds need no search: a layer outside them is a clear layer, and a clear layer's mask is
// false either way.  That is also
// where this kernel departs from the reference's exp_ran, which never assigns the mask of a clear layer lying between
// cloudy ones (its `if` has no `else`, :261-279): here those elements are false, the evident meaning and what max_ran
// does.  The file is compiled with -ffp-contract=off: the comparison is the reference's strict
// local_rand > (1 - cloud_frac) in float32, and exp_ran's correlated deviate is formed left to right without fused
// multiply-adds.
#include "internal.hpp"

#include <cmath>
#include <type_traits>

namespace rrtmgpnn {

static constexpr int kMaskPf = 4;      // layers of randoms in flight per lane
static constexpr int kMaskMaxT = 256;  // lanes per column block

// The seeded route's generator: Philox4x32-10 (Salmon et al., SC'11), a counter-based generator, so a number depends on
// its counter and key alone and neither on the launch nor on which other numbers were drawn.  One call gives the four
// words of kMaskPf = 4 consecutive layers of one g-point of one column:
//   counter (g, l >> 2, (col0 + icol) mod 2^32, stream), key (seed low, seed high); layer l takes word l & 3.
// Each round is two 32 x 32 -> 64 bit products, written as 64-bit products so that both halves come from one
// v_mad_u64_u32 (DESIGN.md §3 has what the compiler chose), and three exclusive-ors per pair.
static_assert(kMaskPf == 4, "one Philox4x32 call per group of kMaskPf layers");

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&w)[4])
{
#pragma unroll
  for (int r = 0; r < 10; r++) {
    if (r > 0) {  // the key is bumped before rounds 2..10
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  w[0] = c0;
  w[1] = c1;
  w[2] = c2;
  w[3] = c3;
}

// 24 random bits -> [0, 1 - 2^-24]: both the conversion and the product are exact in float32
__device__ __forceinline__ float philox_unit(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

// kSeeded: `src` is rng, the four device words {seed low, seed high, stream, col0}, instead of randoms; the kMaskPf
// layers of prefetched randoms become one Philox call per lane per group of kMaskPf layers, skipped by the whole block
// where none of the group's layers is cloudy (cloud_frac is uniform over the block and a deviate is consumed only at a
// cloudy layer, so the skip is exact).  Everything after the deviate is the same statements.
// kCompact (the _active entries: the mask of a block compacted to its daylit columns, rrtmgpnn_daylit_plan): block j
// samples source column idx[j] -- its cloud_frac, overlap_param, randoms and, seeded, its counter word col0 + idx[j],
// so a column has the same clouds compacted or not -- and writes row j of the dense packed mask; blocks at or past
// min(max(*nact, 0), ncol) return at once (ncol is the grid).  The plan takes the byte mask's argument slot (the
// compact entries write packed words only), so the other instances keep their arguments.
struct MaskPlan {
  const int *idx, *nact;
};
using MaskBytes = unsigned char *__restrict__;
template <bool kExp, bool kSeeded = false, bool kCompact = false>
__global__ void __launch_bounds__(kMaskMaxT)
    sampled_mask_kernel(int ngpt, int nlay, const std::conditional_t<kSeeded, uint32_t, float> *__restrict__ src,
                        const float *__restrict__ cloud_frac, const float *__restrict__ overlap,
                        std::conditional_t<kCompact, MaskPlan, MaskBytes> mask, uint32_t *__restrict__ bits)
{
  int icol = blockIdx.x;
  const int nw = (ngpt + 31) / 32;
  if constexpr (kCompact) {
    if ((int)blockIdx.x >= min(max(*mask.nact, 0), (int)gridDim.x)) return;
    icol = mask.idx[blockIdx.x];
  }
  const float *cf = cloud_frac + (size_t)nlay * icol;
  const float *ov = kExp ? overlap + (size_t)(nlay - 1) * icol : nullptr;
  const size_t col = (size_t)nlay * icol;  // this column's first (layer, column) row
  const size_t ocol = kCompact ? (size_t)nlay * blockIdx.x : col;  // ... and that of its output
  uint32_t k0 = 0, k1 = 0, stream = 0, gcol = 0;  // seeded: rng, read once per block (block-uniform loads)
  if constexpr (kSeeded) {
    k0 = src[0];
    k1 = src[1];
    stream = src[2];
    gcol = src[3] + (uint32_t)icol;  // the global column, modulo 2^32
  }
  for (int g0 = 0; g0 < ngpt; g0 += blockDim.x) {
    const int g = g0 + (int)threadIdx.x;
    // a wave wholly past the last g-point has nothing to do (wave-uniform: the ballot below sees whole waves)
    if ((g & ~63) >= ngpt) continue;
    const bool on = g < ngpt;
    const int gc = on ? g : ngpt - 1;  // clamped g-point for unconditional loads
    const float *rc = nullptr;
    float pr[kMaskPf];
    if constexpr (!kSeeded) {
      rc = src + (size_t)ngpt * col + gc;
#pragma unroll
      for (int p = 0; p < kMaskPf; p++) pr[p] = rc[(size_t)ngpt * min(p, nlay - 1)];
    }
    float local = 0.0f;  // local_rands(igpt)
    bool prev = false;   // cloud_mask_layer(ilay-1)
    for (int l0 = 0; l0 < nlay; l0 += kMaskPf) {
      if constexpr (kSeeded) {
        bool any = false;  // block-uniform
#pragma unroll
        for (int p = 0; p < kMaskPf; p++) any = any || cf[min(l0 + p, nlay - 1)] > 0.0f;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (any) philox4x32_10((uint32_t)g, (uint32_t)(l0 >> 2), gcol, stream, k0, k1, w);
#pragma unroll
        for (int p = 0; p < kMaskPf; p++) pr[p] = philox_unit(w[p]);
      }
#pragma unroll
      for (int p = 0; p < kMaskPf; p++) {
        const int l = l0 + p;
        const float r = pr[p];
        if constexpr (!kSeeded) pr[p] = rc[(size_t)ngpt * min(l + kMaskPf, nlay - 1)];
        // the last chunk's steps past nlay only issued their (clamped) load
        if (l < nlay) {
          const float frac = cf[l];
          const bool cloudy = frac > 0.0f;
          if (kExp && prev) {
            // correlated deviates under an adjacent cloudy layer (:272-274); rho and the root are per (layer, column);
            // prev is false at l = 0, so l - 1 >= 0 (and nlay = 1 never reads the then empty overlap_param)
            const float rho = ov[l - 1];
            const float sq = sqrtf(1.0f - rho * rho);  // correctly rounded on all of [0, 1], zero included
            const float corr = rho * (local - 0.5f) + sq * (r - 0.5f) + 0.5f;
            local = cloudy ? corr : local;
          } else if (!prev) {
            local = cloudy ? r : local;  // new deviates if the adjacent layer isn't cloudy; max_ran keeps them if it is
          }
          const bool m = on && cloudy && local > (1.0f - frac);
          prev = cloudy;
          if constexpr (!kCompact)
            if (mask && on) mask[g + (size_t)ngpt * (col + l)] = m ? 1 : 0;
          if (kCompact || bits) {
            // bit g % 32 of word g / 32: the wave's ballot holds two words, stored by its first lane
            const unsigned long long b = __ballot(m);
            if ((threadIdx.x & 63) == 0) {
              const int w = g >> 5;
              uint32_t *o = bits + (size_t)nw * (ocol + l);
              o[w] = (uint32_t)b;
              if (w + 1 < nw) o[w + 1] = (uint32_t)(b >> 32);
            }
          }
        }
      }
    }
  }
}

int launch_sampled_mask(rrtmgpnn_context *ctx, bool exp_ran, int ngpt, int nlay, int ncol, const float *randoms,
                        const float *cloud_frac, const float *overlap, unsigned char *mask, uint32_t *bits)
{
  if (ncol == 0) return RRTMGPNN_OK;
  const int threads = std::min((ngpt + 63) / 64 * 64, kMaskMaxT);
  if (exp_ran)
    hipLaunchKernelGGL(sampled_mask_kernel<true>, dim3(ncol), dim3(threads), 0, ctx->stream, ngpt, nlay, randoms,
                       cloud_frac, overlap, mask, bits);
  else
    hipLaunchKernelGGL(sampled_mask_kernel<false>, dim3(ncol), dim3(threads), 0, ctx->stream, ngpt, nlay, randoms,
                       cloud_frac, overlap, mask, bits);
  RRTMGPNN_LAUNCH_CHECK("sampled_mask_kernel");
  return RRTMGPNN_OK;
}

int launch_sampled_mask_seeded(rrtmgpnn_context *ctx, bool exp_ran, int ngpt, int nlay, int ncol, const uint32_t *rng,
                               const float *cloud_frac, const float *overlap, unsigned char *mask, uint32_t *bits)
{
  if (ncol == 0) return RRTMGPNN_OK;
  const int threads = std::min((ngpt + 63) / 64 * 64, kMaskMaxT);
  if (exp_ran)
    hipLaunchKernelGGL((sampled_mask_kernel<true, true>), dim3(ncol), dim3(threads), 0, ctx->stream, ngpt, nlay, rng,
                       cloud_frac, overlap, mask, bits);
  else
    hipLaunchKernelGGL((sampled_mask_kernel<false, true>), dim3(ncol), dim3(threads), 0, ctx->stream, ngpt, nlay, rng,
                       cloud_frac, overlap, mask, bits);
  RRTMGPNN_LAUNCH_CHECK("sampled_mask_kernel (seeded)");
  return RRTMGPNN_OK;
}

// the compact masks (kCompact): src is randoms or rng; the grid is the launch-time ncol, the count a device word
int launch_sampled_mask_active(rrtmgpnn_context *ctx, bool exp_ran, bool seeded, int ngpt, int nlay, int ncol,
                               const void *src, const float *cloud_frac, const float *overlap, const int *idx,
                               const int *nact, uint32_t *bits)
{
  if (ncol == 0) return RRTMGPNN_OK;
  const int threads = std::min((ngpt + 63) / 64 * 64, kMaskMaxT);
  const MaskPlan plan{idx, nact};
  auto go = [&](auto kern, auto *s) {
    hipLaunchKernelGGL(kern, dim3(ncol), dim3(threads), 0, ctx->stream, ngpt, nlay, s, cloud_frac, overlap, plan, bits);
  };
  if (seeded && exp_ran) go(sampled_mask_kernel<true, true, true>, (const uint32_t *)src);
  else if (seeded) go(sampled_mask_kernel<false, true, true>, (const uint32_t *)src);
  else if (exp_ran) go(sampled_mask_kernel<true, false, true>, (const float *)src);
  else go(sampled_mask_kernel<false, false, true>, (const float *)src);
  RRTMGPNN_LAUNCH_CHECK("sampled_mask_kernel (compact)");
  return RRTMGPNN_OK;
}

// The seeded route's numbers as an array (ngpt, nlay, ncol): blocks stride over (layer group, column) pairs, lane =
// g-point (striding by the block above kMaskMaxT g-points), one Philox call per lane and group, each of its up to
// kMaskPf rows a contiguous store of ngpt values.
__global__ void __launch_bounds__(kMaskMaxT)
    mcica_randoms_kernel(int ngpt, int nlay, long long nblk, const uint32_t *__restrict__ rng,
                         float *__restrict__ randoms)
{
  const int ngrp = (nlay + kMaskPf - 1) / kMaskPf;
  const uint32_t k0 = rng[0], k1 = rng[1], stream = rng[2], col0 = rng[3];
  for (long long b = blockIdx.x; b < nblk; b += gridDim.x) {
    const long long icol = b / ngrp;
    const int l0 = (int)(b - icol * ngrp) * kMaskPf;
    float *out = randoms + (size_t)ngpt * ((size_t)nlay * icol + l0);
    for (int g = threadIdx.x; g < ngpt; g += blockDim.x) {
      uint32_t w[4];
      philox4x32_10((uint32_t)g, (uint32_t)(l0 >> 2), col0 + (uint32_t)icol, stream, k0, k1, w);
#pragma unroll
      for (int p = 0; p < kMaskPf; p++)
        if (l0 + p < nlay) out[(size_t)ngpt * p + g] = philox_unit(w[p]);
    }
  }
}

int launch_mcica_randoms(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const uint32_t *rng, float *randoms)
{
  const long long nblk = (long long)((nlay + kMaskPf - 1) / kMaskPf) * ncol;
  if (nblk == 0) return RRTMGPNN_OK;
  const int threads = std::min((ngpt + 63) / 64 * 64, kMaskMaxT);
  const long long cap = (long long)ctx->num_cus * (2048 / threads);
  hipLaunchKernelGGL(mcica_randoms_kernel, dim3((unsigned)(nblk < cap ? nblk : cap)), dim3(threads), 0, ctx->stream,
                     ngpt, nlay, nblk, rng, randoms);
  RRTMGPNN_LAUNCH_CHECK("mcica_randoms_kernel");
  return RRTMGPNN_OK;
}

// One thread per g-point, blocks striding over (lay, col) rows, as increment_bybnd_kernel: the g-point's band is looked
// up once per thread and every row is a contiguous store of ngpt values.  N: 1 (tau) or 3 (tau, ssa, g).
template <int N>
__global__ void draw_samples_kernel(long long nrow, int ngpt, BandArgs bands, const unsigned char *__restrict__ mask,
                                    const float *__restrict__ tau_bnd, const float *__restrict__ ssa_bnd,
                                    const float *__restrict__ g_bnd, float *__restrict__ tau, float *__restrict__ ssa,
                                    float *__restrict__ g)
{
  const int igpt = threadIdx.x;
  if (igpt >= ngpt) return;
  int b = -1;  // lims 1-based; the API refuses band limits that leave a g-point out
  for (int k = 0; k < bands.nbnd && b < 0; k++)
    if (igpt >= bands.lims[2 * k] - 1 && igpt < bands.lims[2 * k + 1]) b = k;
  if (b < 0) return;
  for (long long r = blockIdx.x; r < nrow; r += gridDim.x) {
    const long long i = igpt + (long long)ngpt * r, ib = b + (long long)bands.nbnd * r;
    const bool m = mask[i] != 0;
    tau[i] = m ? tau_bnd[ib] : 0.0f;
    if constexpr (N == 3) {
      ssa[i] = m ? ssa_bnd[ib] : 0.0f;
      g[i] = m ? g_bnd[ib] : 0.0f;
    }
  }
}

int launch_draw_samples(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const BandArgs &bands,
                        const unsigned char *mask, const float *tau_bnd, const float *ssa_bnd, const float *g_bnd,
                        float *tau, float *ssa, float *g)
{
  const long long nrow = (long long)nlay * ncol;
  if (nrow == 0) return RRTMGPNN_OK;
  if (ngpt > 1024) return fail(RRTMGPNN_ERR_UNSUPPORTED, "draw_samples: more than 1024 g-points");
  const int threads = (ngpt + 63) / 64 * 64;
  const long long cap = (long long)ctx->num_cus * (2048 / threads);
  const dim3 grid((unsigned)(nrow < cap ? nrow : cap)), block(threads);
  if (ssa)
    hipLaunchKernelGGL(draw_samples_kernel<3>, grid, block, 0, ctx->stream, nrow, ngpt, bands, mask, tau_bnd, ssa_bnd,
                       g_bnd, tau, ssa, g);
  else
    hipLaunchKernelGGL(draw_samples_kernel<1>, grid, block, 0, ctx->stream, nrow, ngpt, bands, mask, tau_bnd, ssa_bnd,
                       g_bnd, tau, ssa, g);
  RRTMGPNN_LAUNCH_CHECK("draw_samples_kernel");
  return RRTMGPNN_OK;
}

}  // namespace rrtmgpnn
