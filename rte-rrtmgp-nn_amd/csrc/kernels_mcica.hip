// kernels_mcica.hip -- McICA cloud sampling for gfx950 (extensions/cloud_optics/mo_cloud_sampling.F90).
//
//  * sampled_mask_kernel : sampled_mask_max_ran (:125-192) and sampled_mask_exp_ran (:200-285): the T/F cloud mask of
//                          every (g-point, layer, column) from the caller's random numbers, as a byte mask for the class
//                          layer and / or a packed mask (one bit per g-point) for the solvers' fused increment
//  * draw_samples_kernel : apply_cloud_mask (:291-307): the band value where the mask is set, else 0
//
// The extension predates this fork's layout (as mo_heating_rates does); here randoms and both masks are
// (ngpt, nlay, ncol), cloud_frac (nlay, ncol) and overlap_param (nlay-1, ncol), first index fastest.
//
// Mask kernel: one block per column, lane = g-point (striding by the block when ngpt exceeds it).  The layers are
// walked in array order as the reference walks them, the carried random deviate in a register; the only array
// streamed is randoms, kMaskPf layers of it in flight per lane.  The reference's first / last cloudy layer bounds
// need no search: a layer outside them is a clear layer, and a clear layer's mask is false either way.  That is also
// where this kernel departs from the reference's exp_ran, which never assigns the mask of a clear layer lying between
// cloudy ones (its `if` has no `else`, :261-279): here those elements are false, the evident meaning and what max_ran
// does.  The file is compiled with -ffp-contract=off: the comparison is the reference's strict
// local_rand > (1 - cloud_frac) in float32, and exp_ran's correlated deviate is formed left to right without fused
// multiply-adds.
#include "internal.hpp"

#include <cmath>

namespace rrtmgpnn {

static constexpr int kMaskPf = 4;      // layers of randoms in flight per lane
static constexpr int kMaskMaxT = 256;  // lanes per column block

template <bool kExp>
__global__ void __launch_bounds__(kMaskMaxT)
    sampled_mask_kernel(int ngpt, int nlay, const float *__restrict__ randoms, const float *__restrict__ cloud_frac,
                        const float *__restrict__ overlap, unsigned char *__restrict__ mask,
                        uint32_t *__restrict__ bits)
{
  const int icol = blockIdx.x, nw = (ngpt + 31) / 32;
  const float *cf = cloud_frac + (size_t)nlay * icol;
  const float *ov = kExp ? overlap + (size_t)(nlay - 1) * icol : nullptr;
  const size_t col = (size_t)nlay * icol;  // this column's first (layer, column) row
  for (int g0 = 0; g0 < ngpt; g0 += blockDim.x) {
    const int g = g0 + (int)threadIdx.x;
    // a wave wholly past the last g-point has nothing to do (wave-uniform: the ballot below sees whole waves)
    if ((g & ~63) >= ngpt) continue;
    const bool on = g < ngpt;
    const int gc = on ? g : ngpt - 1;  // clamped g-point for unconditional loads
    const float *rc = randoms + (size_t)ngpt * col + gc;
    float pr[kMaskPf];
#pragma unroll
    for (int p = 0; p < kMaskPf; p++) pr[p] = rc[(size_t)ngpt * min(p, nlay - 1)];
    float local = 0.0f;  // local_rands(igpt)
    bool prev = false;   // cloud_mask_layer(ilay-1)
    for (int l0 = 0; l0 < nlay; l0 += kMaskPf) {
#pragma unroll
      for (int p = 0; p < kMaskPf; p++) {
        const int l = l0 + p;
        const float r = pr[p];
        pr[p] = rc[(size_t)ngpt * min(l + kMaskPf, nlay - 1)];
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
          if (mask && on) mask[g + (size_t)ngpt * (col + l)] = m ? 1 : 0;
          if (bits) {
            // bit g % 32 of word g / 32: the wave's ballot holds two words, stored by its first lane
            const unsigned long long b = __ballot(m);
            if ((threadIdx.x & 63) == 0) {
              const int w = g >> 5;
              uint32_t *o = bits + (size_t)nw * (col + l);
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
