// kernels_bc.hip -- upper boundary condition from one isothermal layer (extensions/mo_compute_bc.F90) for gfx950.
//
// compute_bc puts one thin layer between the gas optics' minimum pressure and the model's top, runs gas optics and
// rte_lw / rte_sw on it and returns the spectrally resolved downward flux at its bottom, (ngpt, ncol): the inc_flux of
// the solver entries.  Two small kernels around the existing gas-optics launch at nlay = 1:
//
//  * bc_inputs_kernel   : the one-layer problem (mo_compute_bc.F90:108-140), gathered from the model's arrays
//  * bc_flux_kernel<SW> : the one-layer solve at the bottom level only -- LW: compute_Planck_source_nn's products with
//                         tlev = tsfc = tlay, lw_source_noscat's source_dn and lw_transport_noscat_dn from a zero
//                         incident radiance, per angle; SW: sw_solver_2stream's direct beam.  No source array, no
//                         (ngpt, 2, ncol) flux array, no LDS.
#include "rte_device.hpp"

#include <cfloat>

namespace rrtmgpnn {

constexpr int kBcThreads = 256;

// One lane per column.  out: play1 (ncol), tlay1 (ncol), plev1 (2, ncol), then one (ncol) array per 2-D gas array of
// src.p, in order.  top = top_lay - 1 (0-based); the layer's lower edge is plev(top_lay + 1) in both orientations
// (quirk B-15: with top_at_1 that is the model's second level, so the layer overlaps the model's top layer).
// The pointer loop is unrolled over constant indices so every pointer stays a kernel-argument SGPR.
__global__ void __launch_bounds__(kBcThreads) bc_inputs_kernel(int ncol, int nlay, int top, float press_min,
                                                               const float *__restrict__ plev,
                                                               const float *__restrict__ tlay, BcGather src,
                                                               float *__restrict__ out)
{
  const int icol = blockIdx.x * kBcThreads + threadIdx.x;
  if (icol >= ncol) return;
  float *play1 = out, *tlay1 = out + ncol, *plev1 = out + 2 * (size_t)ncol, *gas1 = out + 4 * (size_t)ncol;
  const float p1 = press_min, p2 = plev[(size_t)(top + 1) + (size_t)(nlay + 1) * icol];
  plev1[2 * (size_t)icol] = p1;
  plev1[2 * (size_t)icol + 1] = p2;
  play1[icol] = 0.5f * (p1 + p2);
  const size_t s = (size_t)top + (size_t)nlay * icol;
  tlay1[icol] = tlay[s];
#pragma unroll
  for (int k = 0; k < kBcMaxGather; k++)
    if (k < src.n) gas1[(size_t)k * ncol + icol] = src.p[k][s];
}

int launch_bc_inputs(rrtmgpnn_context *ctx, int ncol, int nlay, int top_lay, float press_min, const float *plev,
                     const float *tlay, const BcGather &src, float *out)
{
  if (ncol == 0) return RRTMGPNN_OK;
  hipLaunchKernelGGL(bc_inputs_kernel, dim3((ncol + kBcThreads - 1) / kBcThreads), dim3(kBcThreads), 0, ctx->stream,
                     ncol, nlay, top_lay - 1, press_min, plev, tlay, src, out);
  RRTMGPNN_LAUNCH_CHECK("bc_inputs_kernel");
  return RRTMGPNN_OK;
}

// One lane per (g-point, column), g-points innermost: tau, pfrac and flux_bc are (ngpt, ncol), read and written
// coalesced.  The exps read glibc's 32-entry table from constant memory (the solvers keep it in LDS; here each lane
// takes one to four exps in all).
//
// LW (kSW false): lay_source = pfrac * B_b(tlay) and lev_source = pfrac * B_b(tlev) with tlev = tlay, so both are the
// same product (rrtmgpnn_compute_planck_source_nn at nlay = 1).  Per angle t = tau * D, T = exp(-t), source_dn as
// lw_source_noscat (rte/kernels/mo_rte_solver_kernels.F90:742-776), radn_dn = T * 0 + source_dn (:982-1009, from the
// zero incident radiance 0 / (2 pi w)).  One angle: the bare radiance (quirk B-5, :286-291), times fac = 2 pi w when
// as_flux; several: fac * radn of the first angle plus the later angles' in order (:368-407).  tau * D <= 2^126 as for
// every no-scattering LW entry (solver_div).
//
// SW (kSW true): the direct beam of sw_solver_2stream (:541-692) at the layer's bottom: (solar_source * mu0) at the top
// times exp(-tau * (1 / mu0)).
template <bool kSW>
__global__ void __launch_bounds__(kBcThreads) bc_flux_kernel(int ngpt, int ncol, const float *__restrict__ tau,
                                                             const float *__restrict__ pfrac,
                                                             const float *__restrict__ tlay1, LwPlanck pl,
                                                             BandArgs bands, LwAngles ang, int as_flux,
                                                             const float *__restrict__ solar_source,
                                                             const float *__restrict__ mu0p,
                                                             float *__restrict__ flux_bc)
{
  const long long i = (long long)blockIdx.x * kBcThreads + threadIdx.x;
  if (i >= (long long)ngpt * ncol) return;
  const int icol = (int)(i / ngpt), g = (int)(i - (long long)icol * ngpt);
  const float t0 = tau[i];
  if constexpr (kSW) {
    const float mu0 = mu0p[icol], mu0_inv = 1.0f / mu0;
    const float Ftop = solar_source[g] * mu0;
    flux_bc[i] = solver_exp_beam(-t0 * mu0_inv, kExpTab) * Ftop;
  } else {
    const float *tab = pl.totplnk + (size_t)pl.ntemp * band_of(bands, g);
    const float pf = pfrac[i], T1 = tlay1[icol];
    const float ly = pf * interp1d(T1, pl.tmin, pl.tdelta, pl.ntemp, tab);    // lay_source
    const float lvdn = pf * interp1d(T1, pl.tmin, pl.tdelta, pl.ntemp, tab);  // lev_source, tlev = tlay
    const float tau_thresh = sqrtf(FLT_EPSILON);
    float out = 0.0f;
    for (int imu = 0; imu < ang.nmus; imu++) {
      const float fac = 2.0f * kPi * ang.w[imu];
      const float t = t0 * ang.D[imu];
      const float T = solver_exp_neg(-t, kExpTab);
      const float fact = (t > tau_thresh) ? solver_div(1.0f - T, t) - T : t * (0.5f - 1.0f / 3.0f * t);
      const float S = (1.0f - T) * lvdn + 2.0f * fact * (ly - lvdn);
      const float I = T * 0.0f + S;
      if (ang.nmus == 1) out = as_flux ? fac * I : I;
      else out = imu == 0 ? fac * I : out + fac * I;
    }
    flux_bc[i] = out;
  }
}

int launch_bc_flux_lw(rrtmgpnn_context *ctx, int ngpt, int ncol, const float *tau, const float *pfrac,
                      const float *tlay1, const LwPlanck &pl, const BandArgs &bands, int nmus, const float *Ds,
                      const float *wts, int as_flux, float *flux_bc)
{
  if (ncol == 0) return RRTMGPNN_OK;
  LwAngles ang{};
  ang.nmus = nmus;
  for (int k = 0; k < nmus; k++) { ang.D[k] = Ds[k]; ang.w[k] = wts[k]; }
  const long long n = (long long)ngpt * ncol;
  hipLaunchKernelGGL(bc_flux_kernel<false>, dim3((unsigned)((n + kBcThreads - 1) / kBcThreads)), dim3(kBcThreads), 0,
                     ctx->stream, ngpt, ncol, tau, pfrac, tlay1, pl, bands, ang, as_flux, nullptr, nullptr, flux_bc);
  RRTMGPNN_LAUNCH_CHECK("bc_flux_kernel<lw>");
  return RRTMGPNN_OK;
}

int launch_bc_flux_sw(rrtmgpnn_context *ctx, int ngpt, int ncol, const float *tau, const float *solar_source,
                      const float *mu0, float *flux_bc)
{
  if (ncol == 0) return RRTMGPNN_OK;
  const long long n = (long long)ngpt * ncol;
  hipLaunchKernelGGL(bc_flux_kernel<true>, dim3((unsigned)((n + kBcThreads - 1) / kBcThreads)), dim3(kBcThreads), 0,
                     ctx->stream, ngpt, ncol, tau, nullptr, nullptr, LwPlanck{}, BandArgs{}, LwAngles{}, 0,
                     solar_source, mu0, flux_bc);
  RRTMGPNN_LAUNCH_CHECK("bc_flux_kernel<sw>");
  return RRTMGPNN_OK;
}

}  // namespace rrtmgpnn
