// kernels_lw_scat.hip -- longwave solvers with scattering for gfx950.
//
//  * lw_rescl_kernel   : lw_solver_noscat[_GaussQuad] with do_rescaling -- what rte_lw runs for two-stream
//                        optical properties unless use_2stream is set (rte/mo_rte_lw.F90:372-387): scattering
//                        folded into a scaled optical depth (rte/kernels/mo_rte_solver_kernels.F90:209-233),
//                        a no-scattering pass down, then lw_transport_1rescl (:1729-1795): up and down again
//                        with the adjustment terms
//  * lw_2stream_kernel : lw_solver_2stream (:426-486) with lw_two_stream (:1018-1069, Fu et al. coefficients),
//                        lw_source_2str (:1112-1162) and adding (:1526-1637); sum_broadband_nocol sums
//  * lw_rescl_planck_inc_kernel : lw_rescl_kernel's transport on a 1scl gas atmosphere incremented in-kernel by
//                        band-resolved two-stream clouds (McICA-maskable), the Planck sources formed in-kernel: two
//                        g-point arrays read instead of five, one workspace plane instead of two (row f-9)
//
// Same layout and launch shape as the no-scattering solver: one block per column, one lane per g-point,
// the vertical recurrences in registers, level values that a later pass needs parked in a per-column
// workspace, broadband sums in the reference's order (rte_device.hpp).  Every layer quantity is recomputed
// from the inputs in each pass with the same expressions, so it has the same bits each time.
#include "rte_device.hpp"

namespace rrtmgpnn {

constexpr int kScatRing = 8;  // levels staged per ordered flush

// rescaled layer optics (:209-233) and lw_source_noscat (:742-776; lev_source(l) / lev_source(l+1) in array
// order for every orientation, quirk B-1)
struct RsLayer {
  float trans, An, Cn, sdn, sup;
};

__device__ __forceinline__ RsLayer rs_layer(float tau, float ssal, float g, float D, float lay, float lev_l,
                                            float lev_lp1, const uint64_t *etab)
{
  const float tau_thresh = sqrtf(FLT_EPSILON);
  RsLayer r;
  const float wb = ssal * (1.0f - g) * 0.5f;
  const float scaleTau = (1.0f - ssal + wb);
  r.Cn = 0.4f * wb / scaleTau;
  const float t = tau * D * scaleTau;
  r.trans = solver_exp_neg(-t, etab);
  r.An = (1.0f - r.trans * r.trans);
  const float T = r.trans;
  const float fact = (t > tau_thresh) ? (1.0f - T) / t - T : t * (0.5f - 1.0f / 3.0f * t);
  r.sdn = (1.0f - T) * lev_lp1 + 2.0f * fact * (lay - lev_lp1);
  r.sup = (1.0f - T) * lev_l + 2.0f * fact * (lay - lev_l);
  return r;
}

// kBand: also the by-band fluxes bo.up / bo.dn (ty_fluxes_byband, (nbnd, nlay+1, ncol)): with one angle summed from the
// ring rows in the flush's barrier window (the terms the broadband sum adds: fac * radiance, the bare radiance when
// ngpt % 4 != 0), with several angles from the per-g accumulators
//
// kJac (without kBand and g-point outputs; rrtmgpnn_solver_request_jacobian): also flux_jac (nlay+1, ncol), the Jacobian of
// the upward flux with respect to the surface temperature: J = e * sfc_jac at the surface, J = trans * J with the
// rescaled transmittance in pass 2 (:1761, 1782), staged in a second ring beside the up values (or, several angles,
// a third accumulator plane) and summed as flux_up is.  No downward Jacobian (:1743-1745).
//
// O: the instance's options, an OR of the kResclOpt* bits (internal.hpp), named again in the first lines
template <uint32_t O>
__global__ void __launch_bounds__(256) lw_rescl_kernel(int ngpt, int nlay, int ncol, int top_at_1, LwAngles ang,
                                                       const float *__restrict__ inc_flux,
                                                       const float *__restrict__ tau, const float *__restrict__ ssa,
                                                       const float *__restrict__ gg, const float *__restrict__ lay,
                                                       const float *__restrict__ lev, const float *__restrict__ emis,
                                                       const float *__restrict__ sfc, float *__restrict__ ws,
                                                       float *__restrict__ flux_up, float *__restrict__ flux_dn,
                                                       float *__restrict__ gpt_up, float *__restrict__ gpt_dn,
                                                       BandOut bo, const float *__restrict__ sfc_jac,
                                                       float *__restrict__ flux_jac)
{
  constexpr bool kBand = (O & kResclOptBand) != 0, kJac = (O & kResclOptJac) != 0;
  static_assert(!kJac || !kBand, "the Jacobian instance has no by-band outputs");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int icol = blockIdx.x, g = threadIdx.x;
  const bool on = g < ngpt;
  const int gc = on ? g : ngpt - 1;
  const int nlev = nlay + 1;
  // ty_fluxes_flexible g-point outputs (ngpt, nlev, ncol): with one angle the radiances (quirk B-5), with several they
  // are the angle accumulators
  const bool gpt = gpt_up != nullptr;
  float *gdn = gpt ? gpt_dn + (size_t)ngpt * nlev * icol : nullptr, *gup = gpt ? gpt_up + (size_t)ngpt * nlev * icol : nullptr;
  uint64_t *etab = (uint64_t *)(smem + kExpTabOff);
  float *ring = smem + kExpTabFloats;                 // [kScatRing][ngpt]; kJac: [2][kScatRing][ngpt]
  float *part = ring + (size_t)(kJac ? 2 : 1) * kScatRing * ngpt;  // [2][nlev][4]: 0 = dn, 1 = up; kJac: 2 = Jacobian
  load_exp_table(etab);
  __syncthreads();
  const bool multi = ang.nmus > 1;
  // workspace per column: first-pass radn_dn and the radn_up of the up pass (nlev each), and with nmus > 1
  // the per-g flux accumulators (dn, up; kJac: and the Jacobian's)
  float *wcol = ws + (size_t)(multi ? (kJac ? 5 : 4) : 2) * nlev * ngpt * icol;
  float *WD = wcol, *WU = wcol + (size_t)nlev * ngpt, *acc_base = wcol + (size_t)2 * nlev * ngpt;
  const size_t cl = (size_t)ngpt * nlay * icol, cv = (size_t)ngpt * nlev * icol;
  auto X = [&](int l) { return (size_t)gc + (size_t)ngpt * l; };
  const float *tc = tau + cl, *wc = ssa + cl, *gcol = gg + cl, *yc = lay + cl, *vc = lev + cv;
  const float e = emis[gc + (size_t)ngpt * icol], ss = sfc[gc + (size_t)ngpt * icol];
  const float sj = kJac ? sfc_jac[gc + (size_t)ngpt * icol] : 0.0f;
  const float inc = inc_flux ? inc_flux[gc + (size_t)ngpt * icol] : 0.0f;
  auto layer = [&](int l, float D) {
    return rs_layer(tc[X(l)], wc[X(l)], gcol[X(l)], D, yc[X(l)], vc[X(l)], vc[X(l + 1)], etab);
  };
  const int top = top_at_1 ? 0 : nlay, sfcl = top_at_1 ? nlay : 0, dl_dn = top_at_1 ? 1 : -1;
  float *pdn = part, *pup = part + (size_t)nlev * 4;

  for (int imu = 0; imu < ang.nmus; imu++) {
    const float D = ang.D[imu];
    const float fac = (multi || (ngpt & 3) == 0) ? 2.0f * kPi * ang.w[imu] : 1.0f;  // quirk B-5 as noscat
    const bool acc = imu > 0;
    // v = fac * radiance; rad = the radiance
    auto put = [&](float v, float rad, int r, int q, int level) {
      if (!on) return;
      if (multi) {
        float *w = (gpt ? (q == 0 ? gdn : gup) + (size_t)level * ngpt : acc_base + ((size_t)q * nlev + level) * ngpt) + g;
        *w = acc ? *w + v : v;
      } else {
        ring[(size_t)r * ngpt + g] = v;
        if (gpt) (q == 0 ? gdn : gup)[(size_t)level * ngpt + g] = rad;
      }
    };
    // kJac: v = fac * J of an up-pass level
    auto put_jac = [&](float v, int r, int level) {
      if (!on) return;
      if (multi) {
        float *w = acc_base + ((size_t)2 * nlev + level) * ngpt + g;
        *w = acc ? *w + v : v;
      } else {
        ring[((size_t)kScatRing + r) * ngpt + g] = v;
      }
    };
    auto flush = [&](float *pq, int n, int lev0, int dl) {
      if (multi) return;
      if constexpr (kJac) {
        // the up pass flushes both rings: flux_up's partials to pup, the Jacobian's to the plane after it
        if (pq == pup) ring_flush<kScatRing>(ring, pq, 2, n, lev0, dl, ngpt, nlev, false);
        else           ring_flush<kScatRing>(ring, pq, 1, n, lev0, dl, ngpt, nlev, false);
      } else if constexpr (kBand)
        ring_flush<kScatRing, true>(ring, pq, 1, n, lev0, dl, ngpt, nlev, false, false, 0, &bo.b,
                                    pq == pdn ? bo.dn : bo.up, nullptr, nullptr, icol);
      else
        ring_flush<kScatRing>(ring, pq, 1, n, lev0, dl, ngpt, nlev, false);
    };
    // 1: no-scattering transport down with the rescaled optics (lw_transport_noscat_dn)
    const float I0 = inc / (2.0f * kPi * ang.w[imu]);
    float I = I0;
    if (on) WD[X(top)] = I;
    for (int j = 0; j < nlay; j++) {
      const int l = top_at_1 ? j : nlay - 1 - j;
      const RsLayer r = layer(l, D);
      I = r.trans * I + r.sdn;
      if (on) WD[X(top_at_1 ? l + 1 : l)] = I;
    }
    // surface reflection and emission
    float U = I * (1.0f - e) + e * ss;
    float J = e * sj;  // kJac (:270)
    if (on) WU[X(sfcl)] = U;
    put(fac * U, U, 0, 1, sfcl);
    if constexpr (kJac) put_jac(fac * J, 0, sfcl);
    flush(pup, 1, sfcl, 1);
    // 2: up with the adjustment from the first-pass radiance at the layer top (lw_transport_1rescl)
    for (int j0 = 0; j0 < nlay; j0 += kScatRing) {
      for (int s = 0; s < kScatRing; s++) {
        const int j = j0 + s;
        if (j < nlay) {
          const int l = top_at_1 ? nlay - 1 - j : j;
          const int ltop = top_at_1 ? l : l + 1;
          const RsLayer r = layer(l, D);
          const float adj = r.Cn * (r.An * WD[X(ltop)] - r.trans * r.sdn - r.sup);
          U = r.trans * U + r.sup + adj;
          if (on) WU[X(ltop)] = U;
          put(fac * U, U, s, 1, ltop);
          if constexpr (kJac) {
            J = r.trans * J;
            put_jac(fac * J, s, ltop);
          }
        }
      }
      flush(pup, min(kScatRing, nlay - j0), sfcl - dl_dn * (j0 + 1), -dl_dn);
    }
    // 3: down again with the adjustment from radn_up(l) in array order: the layer top when top_at_1, the
    //    layer bottom otherwise (:1761-1767 vs :1783-1789, reproduced)
    I = I0;
    put(fac * I, I, 0, 0, top);
    flush(pdn, 1, top, 1);
    for (int j0 = 0; j0 < nlay; j0 += kScatRing) {
      for (int s = 0; s < kScatRing; s++) {
        const int j = j0 + s;
        if (j < nlay) {
          const int l = top_at_1 ? j : nlay - 1 - j;
          const RsLayer r = layer(l, D);
          const float adj = r.Cn * (r.An * WU[X(l)] - r.trans * r.sup - r.sdn);
          I = r.trans * I + r.sdn + adj;
          put(fac * I, I, s, 0, top_at_1 ? l + 1 : l);
        }
      }
      flush(pdn, min(kScatRing, nlay - j0), top + dl_dn * (j0 + 1), dl_dn);
    }
  }
  if (multi) {
    __syncthreads();
    if constexpr (kBand) {
      // sum_byband of the angle-summed g-point fluxes: one lane per (quantity, level, band), band fastest
      const int nb = bo.b.nbnd;
      for (int t = g; t < 2 * nlev * nb; t += blockDim.x) {
        const int r = t / nb, ib = t - r * nb;
        float *o = r < nlev ? bo.dn : bo.up;
        if (!o) continue;
        const float *w = acc_base + (size_t)r * ngpt;
        o[ib + (size_t)nb * ((r % nlev) + (size_t)nlev * icol)] =
            band_walk(w, w, false, bo.b.lims[2 * ib] - 1, bo.b.lims[2 * ib + 1]);
      }
    }
    for (int t = g; t < 2 * nlev; t += blockDim.x) {
      const float *w = gpt ? (t < nlev ? gdn : gup) + (size_t)(t % nlev) * ngpt : acc_base + (size_t)t * ngpt;
      float s = 0.0f;
      for (int i = 0; i < ngpt; i++) s = s + w[i];  // sum_broadband: sequential over g
      const int l = t % nlev;
      (t < nlev ? flux_dn : flux_up)[l + (size_t)nlev * icol] = s;
    }
    if constexpr (kJac) {
      for (int l = g; l < nlev; l += blockDim.x) {
        const float *w = acc_base + ((size_t)2 * nlev + l) * ngpt;
        float s = 0.0f;
        for (int i = 0; i < ngpt; i++) s = s + w[i];  // sum_broadband
        flux_jac[l + (size_t)nlev * icol] = s;
      }
    }
    return;
  }
  for (int l = g; l < nlev; l += blockDim.x) {
    flux_dn[l + (size_t)nlev * icol] = combine4(pdn + 4 * l);
    flux_up[l + (size_t)nlev * icol] = combine4(pup + 4 * l);
    if constexpr (kJac) flux_jac[l + (size_t)nlev * icol] = combine4(pup + 4 * (nlev + l));
  }
}

// ------------------------------------------------------------------------------------------
// lw_rescl_planck_inc_kernel (rrtmgpnn_lw_solver_1rescl_planck_inc): the rescaled solver on a 1scl gas atmosphere
// incremented by band-resolved two-stream clouds, with the Planck sources formed in-kernel.  What
// compute_Planck_source_nn, zeroed gas ssa / g, [draw_samples,] increment and lw_rescl_kernel give, bit for bit, from
// two g-point arrays (tau, pfrac) and three band arrays instead of five g-point arrays:
//  * optics: inc_2str(tau, 0, 0, tau_bnd(b), ssa_bnd(b), g_bnd(b)) -- the gas operands are the literal zeros the host
//    would have stored, kept in the expressions (the sign of a zero g depends on them);
//  * kMask: where the g-point's bit of cmask (nw, nlay, ncol) is clear the three band operands are 0, which is what
//    draw_samples leaves there for increment to add;
//  * sources: lay = pfrac(l) * B_b(tlay(l)), lev(li) = pfrac(min(li, nlay-1)) * B_b(tlev(li)), sfc = pfrac(sfc_lay) *
//    B_b(tsfc), the band Planck values interpolated once per column into LDS by lw_planck_table (rte_device.hpp), which
//    lw_noscat_kernel's kFused instances call too;
//  * transport: rs_layer and the three passes of lw_rescl_kernel, the same ring and ordered flush.
// A layer's inputs -- tau, pfrac, the neighbouring pfrac of lev(l+1), three band values (one address per band: the
// loads broadcast), kMask: one mask word -- are loaded kPF layers ahead of the recurrence in every pass, and so is the
// workspace value that passes 2 and 3 read.
// Workspace: ONE plane (nlev, ngpt) per column.  Pass 1 parks radn_dn there; pass 2 reads level ltop's value and then
// writes its radn_up to the same element (read first, by the same lane), never reading the surface element, which the
// surface step overwrote; pass 3 reads only radn_up.  With several angles two accumulator planes follow.
// LDS: etab | B [nbnd][2*nlay+1], Bsfc [nbnd] | ring [kScatRing][ngpt] | part [2][nlev][4]
// ------------------------------------------------------------------------------------------
#ifndef RRTMGPNN_LW_SCAT_PF
#define RRTMGPNN_LW_SCAT_PF 1
#endif
constexpr int kScatPf = RRTMGPNN_LW_SCAT_PF;  // layers of inputs in flight per lane
static_assert(kScatPf >= 1 && kScatRing % kScatPf == 0, "prefetch depth must divide the ring");

struct RsIn {
  float t, y, yn, tb, wb, gb;
  uint32_t m;
  float ta;  // kAer
};

// the no-scattering layer of the clear radiance (kDual): lw_noscat_kernel's step, expression for expression, so the
// clear fluxes carry the bits of rrtmgpnn_lw_solver_noscat_planck[_inc] (rs_layer with ssa = g = 0 gives the same
// values wherever tau * D <= 2^126; this one also shares that kernel's division)
struct NsLayer {
  float trans, sdn, sup;
};

__device__ __forceinline__ NsLayer ns_layer(float tau, float D, float lay, float lev_l, float lev_lp1,
                                            const uint64_t *etab)
{
  const float tau_thresh = sqrtf(FLT_EPSILON);
  NsLayer r;
  const float t = tau * D;
  const float T = solver_exp_neg(-t, etab);
  const float fact = (t > tau_thresh) ? solver_div(1.0f - T, t) - T : t * (0.5f - 1.0f / 3.0f * t);
  r.trans = T;
  r.sdn = (1.0f - T) * lev_lp1 + 2.0f * fact * (lay - lev_lp1);
  r.sup = (1.0f - T) * lev_l + 2.0f * fact * (lay - lev_l);
  return r;
}

// the arguments of the kAer / kDual instances only: the others' argument list is the one they had
template <bool kOn>
struct ScatDualArgs {};
template <>
struct ScatDualArgs<true> {
  const float *tau_aer;              // kAer: (nbnd, nlay, ncol)
  float *flux_up_clr, *flux_dn_clr;  // kDual: (nlay+1, ncol)
};

// kAer (rrtmgpnn_lw_solver_1rescl_planck_clr_all with an aerosol request): a second, unmasked band increment tau_aer
// (nbnd, nlay, ncol) in front of the cloud's -- inc_2stream_by_1scalar_bybnd, which leaves ssa = g = +0 and
// tau + tau_aer(band), then inc_2str with the cloud: two separately rounded adds, (tau + tau_aer) + tau_cld.  One more
// band value per prefetched layer, read as tau_bnd is (same band offset, its own column base).  The mask never
// switches it.
//
// kDual (one angle; the same entry in mode 1): clear-sky fluxes (gases [+ aerosols], no scattering) beside the all-sky
// ones from one read of tau, pfrac, the band rows and the mask word and one Planck table (rte_lw of
// extensions/mo_rrtmgp_clr_all_sky.F90:146-172).  Each lane carries the clear radiance of t_clr = tau [+ tau_aer]
// through ns_layer: down in pass 1, up in pass 2; pass 3 has nothing to add for it.  The clear values are staged in a
// second ring ([2][kScatRing][ngpt]: 0 = all-sky, 1 = clear) and reduced to part planes 2 (up) and 3 (dn): clear down
// by pass 1's own flushes (the all-sky radiance stages nothing there), clear up beside all-sky up by pass 2's.  The
// three passes are written once: what the clear radiance adds stands under `if constexpr (kDual)` at the points of the
// loop where it acts, so the prefetch, the workspace reads and the flush windows are the single instances' own.
//
// O: the instance's options, an OR of the kScatOpt* bits (internal.hpp), named again in the first lines
template <uint32_t O>
__global__ void __launch_bounds__(256) lw_rescl_planck_inc_kernel(
    int ngpt, int nlay, int ncol, int top_at_1, LwAngles ang, const float *__restrict__ inc_flux,
    const float *__restrict__ tau, const float *__restrict__ pfrac, const float *__restrict__ tau_bnd,
    const float *__restrict__ ssa_bnd, const float *__restrict__ g_bnd, const float *__restrict__ emis, LwPlanck pl,
    BandArgs bands, const uint32_t *__restrict__ cmask, float *__restrict__ ws, float *__restrict__ flux_up,
    float *__restrict__ flux_dn, ScatDualArgs<(O & (kScatOptAer | kScatOptDual)) != 0> da)
{
  constexpr bool kMask = (O & kScatOptMask) != 0, kAer = (O & kScatOptAer) != 0, kDual = (O & kScatOptDual) != 0;
  constexpr int kPF = kScatPf;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int icol = blockIdx.x, g = threadIdx.x;
  const bool on = g < ngpt;
  const int gc = on ? g : ngpt - 1;  // clamped g-point for unconditional loads
  const int nlev = nlay + 1, nbnd = bands.nbnd, brow = 2 * nlay + 1;
  uint64_t *etab = (uint64_t *)(smem + kExpTabOff);
  float *btab = smem + kExpTabFloats;
  float *ring = btab + lw_btab_floats(nbnd, nlay);  // [kScatRing][ngpt]; kDual: [2][kScatRing][ngpt]
  // [2][nlev][4]: 0 = dn, 1 = up; kDual: [4][nlev][4]: and 2 = clear up, 3 = clear dn
  float *part = ring + (size_t)(kDual ? 2 : 1) * kScatRing * ngpt;
  load_exp_table(etab);
  const bool multi = !kDual && ang.nmus > 1;
  float *W = ws + (size_t)(multi ? 3 : 1) * nlev * ngpt * icol, *acc_base = W + (size_t)nlev * ngpt;
  auto X = [&](int l) { return (size_t)gc + (size_t)ngpt * l; };
  // column-local descriptors (rte_device.hpp): the layer offset is an SGPR, the lane's offset a VGPR
  const int b = band_of(bands, gc);
  const uint32_t vg = 4u * (uint32_t)gc, row = 4u * (uint32_t)ngpt, vb = 4u * (uint32_t)b, irow = 4u * (uint32_t)nbnd;
  const uint32_t nw = (uint32_t)((ngpt + 31) / 32), vm = 4u * (uint32_t)(gc >> 5), mrow = 4u * nw;
  const uint32_t mbit = 1u << (gc & 31);
  const ColArr Ttau(tau, (size_t)ngpt * nlay * icol, row * nlay), Tpf(pfrac, (size_t)ngpt * nlay * icol, row * nlay);
  const size_t cb = (size_t)nbnd * nlay * icol;
  const ColArr Ttb(tau_bnd, cb, irow * nlay), Twb(ssa_bnd, cb, irow * nlay), Tgb(g_bnd, cb, irow * nlay);
  const ColArr Tmsk(kMask ? (const float *)cmask : tau, kMask ? (size_t)nw * nlay * icol : 0, mrow * nlay);
  const float *aer_base = tau;
  if constexpr (kAer) aer_base = da.tau_aer;
  const ColArr Taer(aer_base, kAer ? cb : 0, irow * nlay);
  auto load = [&](int l) {
    RsIn d;
    d.t = Ttau.ld(vg, row * (uint32_t)l);
    d.y = Tpf.ld(vg, row * (uint32_t)l);
    d.yn = Tpf.ld(vg, row * (uint32_t)min(l + 1, nlay - 1));
    d.tb = Ttb.ld(vb, irow * (uint32_t)l);
    d.wb = Twb.ld(vb, irow * (uint32_t)l);
    d.gb = Tgb.ld(vb, irow * (uint32_t)l);
    d.m = kMask ? __float_as_uint(Tmsk.ld(vm, mrow * (uint32_t)l)) : 0u;
    d.ta = kAer ? Taer.ld(vb, irow * (uint32_t)l) : 0.0f;
    return d;
  };
  const float ysfc = Tpf.ld(vg, row * (uint32_t)(pl.sfc_lay - 1));
  const float e = pl.emis_by_band ? emis[b + (size_t)nbnd * icol] : emis[gc + (size_t)ngpt * icol];
  const float inc = inc_flux ? inc_flux[gc + (size_t)ngpt * icol] : 0.0f;
  lw_planck_table<false>(btab, pl, nbnd, nlay, icol);  // band Planck values of this column (rte_device.hpp)
  const float *bl = btab + (size_t)b * brow;  // this lane's band row
  __syncthreads();
  const float ss = ysfc * btab[(size_t)nbnd * brow + b];
  auto layer = [&](const RsIn &d, int l, float D) {
    const bool cld = !kMask || (d.m & mbit) != 0;
    float t = d.t, w = 0.0f, gq = 0.0f;
    if constexpr (kAer) t = d.t + d.ta;
    inc_2str(t, w, gq, cld ? d.tb : 0.0f, cld ? d.wb : 0.0f, cld ? d.gb : 0.0f);
    return rs_layer(t, w, gq, D, d.y * bl[l], d.y * bl[nlay + l], d.yn * bl[nlay + l + 1], etab);
  };
  // kDual: the clear layer, from the same operands
  auto layer_clr = [&](const RsIn &d, int l, float D) {
    float t = d.t;
    if constexpr (kAer) t = d.t + d.ta;
    return ns_layer(t, D, d.y * bl[l], d.y * bl[nlay + l], d.yn * bl[nlay + l + 1], etab);
  };
  const int top = top_at_1 ? 0 : nlay, sfcl = top_at_1 ? nlay : 0, dl_dn = top_at_1 ? 1 : -1;
  auto lay_dn = [&](int j) { return top_at_1 ? j : nlay - 1 - j; };  // j-th layer from the top
  auto lay_up = [&](int j) { return top_at_1 ? nlay - 1 - j : j; };  // j-th layer from the surface
  float *pdn = part, *pup = part + (size_t)nlev * 4;

  // kDual: the clear ring and its part planes (null in the single instances, whose LDS holds neither)
  [[maybe_unused]] float *const ring_clr = kDual ? ring + (size_t)kScatRing * ngpt : nullptr;
  [[maybe_unused]] float *const pup_clr = kDual ? part + (size_t)2 * nlev * 4 : nullptr;
  [[maybe_unused]] float *const pdn_clr = kDual ? part + (size_t)3 * nlev * 4 : nullptr;

  const int nang = kDual ? 1 : ang.nmus;
  for (int imu = 0; imu < nang; imu++) {
    const float D = ang.D[imu];
    const float fac = (multi || (ngpt & 3) == 0) ? 2.0f * kPi * ang.w[imu] : 1.0f;  // quirk B-5 as noscat
    const bool acc = imu > 0;
    // v = fac * radiance of plane q (0 = dn, 1 = up)
    auto put = [&](float v, int r, int q, int level) {
      if (!on) return;
      if (multi) {
        float *w = acc_base + ((size_t)q * nlev + level) * ngpt + g;
        *w = acc ? *w + v : v;
      } else {
        ring[(size_t)r * ngpt + g] = v;
      }
    };
    // kDual: v = fac * the clear radiance, into the second ring
    auto put_clr = [&](float v, int r) {
      if (on) ring_clr[(size_t)r * ngpt + g] = v;
    };
    // nq rings from rg on into nq part planes from pq on.  kDual: the clear ring alone (pass 1, to plane 3), both rings
    // (pass 2, to planes 1 and 2), the all-sky ring alone (pass 3)
    auto flush = [&](const float *rg, float *pq, int nq, int n, int lev0, int dl) {
      if (!multi) ring_flush<kScatRing>(rg, pq, nq, n, lev0, dl, ngpt, nlev, false);
    };
    RsIn pf[kPF];
    float pw[kPF];
    // 1: no-scattering transport down with the rescaled optics (lw_transport_noscat_dn), radn_dn into W; kDual: the
    //    clear radiance beside it, staged in its ring and flushed here
    const float I0 = inc / (2.0f * kPi * ang.w[imu]);
    float I = I0;
    [[maybe_unused]] float Ic = I0;  // kDual
    if (on) W[X(top)] = I;
#pragma unroll
    for (int p = 0; p < kPF; p++) pf[p] = load(lay_dn(min(p, nlay - 1)));
    if constexpr (kDual) {
      put_clr(fac * Ic, 0);
      flush(ring_clr, pdn_clr, 1, 1, top, 1);
    }
    for (int j0 = 0; j0 < nlay; j0 += kScatRing) {
#pragma unroll
      for (int s = 0; s < kScatRing; s++) {
        const int j = j0 + s, p = s % kPF, l = lay_dn(min(j, nlay - 1));
        const RsIn d = pf[p];
        pf[p] = load(lay_dn(min(j + kPF, nlay - 1)));
        if (j < nlay) {
          const RsLayer r = layer(d, l, D);
          I = r.trans * I + r.sdn;
          if (on) W[X(top_at_1 ? l + 1 : l)] = I;
          if constexpr (kDual) {
            const NsLayer c = layer_clr(d, l, D);
            Ic = c.trans * Ic + c.sdn;
            put_clr(fac * Ic, s);
          }
        }
      }
      if constexpr (kDual) flush(ring_clr, pdn_clr, 1, min(kScatRing, nlay - j0), top + dl_dn * (j0 + 1), dl_dn);
    }
    // surface reflection and emission
    float U = I * (1.0f - e) + e * ss;
    [[maybe_unused]] float Uc = Ic * (1.0f - e) + e * ss;  // kDual
    if (on) W[X(sfcl)] = U;
    put(fac * U, 0, 1, sfcl);
    if constexpr (kDual) put_clr(fac * Uc, 0);
    flush(ring, pup, kDual ? 2 : 1, 1, sfcl, 1);
    // 2: up with the adjustment from the first-pass radiance at the layer top (lw_transport_1rescl); the layer top's
    //    element of W is read (radn_dn), then written (radn_up); kDual: the clear radiance up beside it, one flush of
    //    both rings
    auto ltop_of = [&](int l) { return top_at_1 ? l : l + 1; };
#pragma unroll
    for (int p = 0; p < kPF; p++) {
      const int l = lay_up(min(p, nlay - 1));
      pf[p] = load(l);
      pw[p] = W[X(ltop_of(l))];
    }
    for (int j0 = 0; j0 < nlay; j0 += kScatRing) {
#pragma unroll
      for (int s = 0; s < kScatRing; s++) {
        const int j = j0 + s, p = s % kPF, l = lay_up(min(j, nlay - 1)), ltop = ltop_of(l);
        const RsIn d = pf[p];
        const float wd = pw[p];
        {
          const int ln = lay_up(min(j + kPF, nlay - 1));
          pf[p] = load(ln);
          pw[p] = W[X(ltop_of(ln))];
        }
        if (j < nlay) {
          const RsLayer r = layer(d, l, D);
          const float adj = r.Cn * (r.An * wd - r.trans * r.sdn - r.sup);
          U = r.trans * U + r.sup + adj;
          if (on) W[X(ltop)] = U;
          put(fac * U, s, 1, ltop);
          if constexpr (kDual) {
            const NsLayer c = layer_clr(d, l, D);
            Uc = c.trans * Uc + c.sup;
            put_clr(fac * Uc, s);
          }
        }
      }
      flush(ring, pup, kDual ? 2 : 1, min(kScatRing, nlay - j0), sfcl - dl_dn * (j0 + 1), -dl_dn);
    }
    // 3: down again with the adjustment from radn_up(l) in array order: the layer top when top_at_1, the
    //    layer bottom otherwise (:1761-1767 vs :1783-1789, reproduced); the clear radiance has nothing to add
    I = I0;
    put(fac * I, 0, 0, top);
#pragma unroll
    for (int p = 0; p < kPF; p++) {
      const int l = lay_dn(min(p, nlay - 1));
      pf[p] = load(l);
      pw[p] = W[X(l)];
    }
    flush(ring, pdn, 1, 1, top, 1);
    for (int j0 = 0; j0 < nlay; j0 += kScatRing) {
#pragma unroll
      for (int s = 0; s < kScatRing; s++) {
        const int j = j0 + s, p = s % kPF, l = lay_dn(min(j, nlay - 1));
        const RsIn d = pf[p];
        const float wu = pw[p];
        {
          const int ln = lay_dn(min(j + kPF, nlay - 1));
          pf[p] = load(ln);
          pw[p] = W[X(ln)];
        }
        if (j < nlay) {
          const RsLayer r = layer(d, l, D);
          const float adj = r.Cn * (r.An * wu - r.trans * r.sup - r.sdn);
          I = r.trans * I + r.sdn + adj;
          put(fac * I, s, 0, top_at_1 ? l + 1 : l);
        }
      }
      flush(ring, pdn, 1, min(kScatRing, nlay - j0), top + dl_dn * (j0 + 1), dl_dn);
    }
  }
  if (multi) {
    __syncthreads();
    for (int t = g; t < 2 * nlev; t += blockDim.x) {
      const float *w = acc_base + (size_t)t * ngpt;
      float s = 0.0f;
      for (int i = 0; i < ngpt; i++) s = s + w[i];  // sum_broadband: sequential over g
      (t < nlev ? flux_dn : flux_up)[(t % nlev) + (size_t)nlev * icol] = s;
    }
    return;
  }
  for (int l = g; l < nlev; l += blockDim.x) {
    flux_dn[l + (size_t)nlev * icol] = combine4(pdn + 4 * l);
    flux_up[l + (size_t)nlev * icol] = combine4(pup + 4 * l);
    if constexpr (kDual) {
      da.flux_dn_clr[l + (size_t)nlev * icol] = combine4(pdn_clr + 4 * l);
      da.flux_up_clr[l + (size_t)nlev * icol] = combine4(pup_clr + 4 * l);
    }
  }
}

// lw_two_stream (:1018-1069) and lw_source_2str (:1112-1162) for one layer
struct L2Layer {
  float Rdif, Tdif, sdn, sup;
};

__device__ __forceinline__ L2Layer l2_layer(float tau, float w0, float g, float lev_top, float lev_bot,
                                            const uint64_t *etab)
{
  const float k_min = 1.e-4f, LW_diff_sec = 1.66f;
  L2Layer r;
  const float gamma1 = LW_diff_sec * (1.0f - 0.5f * w0 * (1.0f + g));
  const float gamma2 = LW_diff_sec * 0.5f * w0 * (1.0f - g);
  const float k = sqrtf(fmaxf((gamma1 - gamma2) * (gamma1 + gamma2), k_min));
  const float emk = solver_exp_neg(-tau * k, etab);
  const float em2k = emk * emk;
  const float RT = 1.0f / (k * (1.0f + em2k) + gamma1 * (1.0f - em2k));
  r.Rdif = RT * gamma2 * (1.0f - em2k);
  r.Tdif = RT * 2.0f * k * emk;
  if (tau > 1.0e-8f) {
    const float Z = (lev_bot - lev_top) / (tau * (gamma1 + gamma2));
    const float Zup_top = Z + lev_top, Zup_bottom = Z + lev_bot;
    const float Zdn_top = -Z + lev_top, Zdn_bottom = -Z + lev_bot;
    r.sup = kPi * (Zup_top - r.Rdif * Zdn_top - r.Tdif * Zup_bottom);
    r.sdn = kPi * (Zdn_bottom - r.Rdif * Zup_bottom - r.Tdif * Zdn_top);
  } else {
    r.sup = 0.0f;
    r.sdn = 0.0f;
  }
  return r;
}

// kBand: also the by-band fluxes bo.up / bo.dn, summed from the ring rows in the flush's barrier window
template <bool kBand = false>
__global__ void __launch_bounds__(256) lw_2stream_kernel(int ngpt, int nlay, int ncol, int top_at_1,
                                                         const float *__restrict__ inc_flux,
                                                         const float *__restrict__ tau, const float *__restrict__ ssa,
                                                         const float *__restrict__ gg, const float *__restrict__ lev,
                                                         const float *__restrict__ emis,
                                                         const float *__restrict__ sfc, float *__restrict__ ws,
                                                         float *__restrict__ flux_up, float *__restrict__ flux_dn,
                                                         float *__restrict__ gpt_up, float *__restrict__ gpt_dn,
                                                         BandOut bo)
{
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int icol = blockIdx.x, g = threadIdx.x;
  const bool on = g < ngpt;
  const int gc = on ? g : ngpt - 1;
  const int nlev = nlay + 1;
  uint64_t *etab = (uint64_t *)(smem + kExpTabOff);
  float *ring = smem + kExpTabFloats;                 // [2][kScatRing][ngpt]: up, dn
  float *part = ring + (size_t)2 * kScatRing * ngpt;  // [2][nlev][4]
  load_exp_table(etab);
  __syncthreads();
  // workspace per column: albedo and source of upward radiation at each level (adding, Eqs 9 and 11)
  float *WA = ws + (size_t)2 * nlev * ngpt * icol, *WS = WA + (size_t)nlev * ngpt;
  const size_t cl = (size_t)ngpt * nlay * icol, cv = (size_t)ngpt * nlev * icol;
  auto X = [&](int l) { return (size_t)gc + (size_t)ngpt * l; };
  const float *tc = tau + cl, *wc = ssa + cl, *gcol = gg + cl, *vc = lev + cv;
  auto layer = [&](int l) {
    const int lt = top_at_1 ? l : l + 1, lb = top_at_1 ? l + 1 : l;
    return l2_layer(tc[X(l)], wc[X(l)], gcol[X(l)], vc[X(lt)], vc[X(lb)], etab);
  };
  const float e = emis[gc + (size_t)ngpt * icol], ss = sfc[gc + (size_t)ngpt * icol];
  const int top = top_at_1 ? 0 : nlay, sfcl = top_at_1 ? nlay : 0, dl_dn = top_at_1 ? 1 : -1;
  // bottom to top: albedo and source (adding :1555-1574 / :1595-1614)
  float alb_b = 1.0f - e, src_b = kPi * e * ss;
  if (on) {
    WA[X(sfcl)] = alb_b;
    WS[X(sfcl)] = src_b;
  }
  for (int j = 0; j < nlay; j++) {
    const int l = top_at_1 ? nlay - 1 - j : j;
    const L2Layer r = layer(l);
    const float denom = 1.0f / (1.0f - r.Rdif * alb_b);
    const float alb = r.Rdif + r.Tdif * r.Tdif * alb_b * denom;
    const float src = r.sup + r.Tdif * denom * (src_b + alb_b * r.sdn);
    if (on) {
      WA[X(top_at_1 ? l : l + 1)] = alb;
      WS[X(top_at_1 ? l : l + 1)] = src;
    }
    alb_b = alb;
    src_b = src;
  }
  // top to bottom: fluxes (Eqs 12-13), sum_broadband_nocol = sum(flux, 1): sequential over g
  // level `lev` of the g-point outputs (flux_up_gpt / flux_dn_gpt, :481-483), when asked for
  float *gu = gpt_up ? gpt_up + (size_t)ngpt * nlev * icol : nullptr, *gd = gpt_dn ? gpt_dn + (size_t)ngpt * nlev * icol : nullptr;
  auto put = [&](float up, float dn, int s, int lev) {
    if (on) {
      ring[(size_t)s * ngpt + g] = up;
      ring[((size_t)kScatRing + s) * ngpt + g] = dn;
      if (gu) {
        gu[(size_t)lev * ngpt + g] = up;
        gd[(size_t)lev * ngpt + g] = dn;
      }
    }
  };
  auto flush = [&](int n, int lev0, int dl) {
    if constexpr (kBand)
      ring_flush<kScatRing, true>(ring, part, 2, n, lev0, dl, ngpt, nlev, false, true, 0, &bo.b, bo.up, bo.dn, nullptr,
                                  icol);
    else
      ring_flush<kScatRing>(ring, part, 2, n, lev0, dl, ngpt, nlev, false, true);
  };
  float Fdn = (on && inc_flux) ? inc_flux[g + (size_t)ngpt * icol] : 0.0f;
  put(Fdn * alb_b + src_b, Fdn, 0, top);
  flush(1, top, 1);
  for (int j0 = 0; j0 < nlay; j0 += kScatRing) {
    for (int s = 0; s < kScatRing; s++) {
      const int j = j0 + s;
      if (j < nlay) {
        const int l = top_at_1 ? j : nlay - 1 - j, lbelow = top_at_1 ? l + 1 : l;
        const L2Layer r = layer(l);
        const float alb = WA[X(lbelow)], src = WS[X(lbelow)];
        const float denom = 1.0f / (1.0f - r.Rdif * alb);
        Fdn = (r.Tdif * Fdn + r.Rdif * src + r.sdn) * denom;
        put(Fdn * alb + src, Fdn, s, lbelow);
      }
    }
    flush(min(kScatRing, nlay - j0), top + dl_dn * (j0 + 1), dl_dn);
  }
  for (int l = g; l < nlev; l += blockDim.x) {
    flux_up[l + (size_t)nlev * icol] = combine4(part + 4 * l);
    flux_dn[l + (size_t)nlev * icol] = combine4(part + (size_t)nlev * 4 + 4 * l);
  }
}

// The instances lw_rescl_kernel is compiled for
using LwResclInstances = SolverInstances<0u, kResclOptBand, kResclOptJac>;

int launch_lw_rescl(rrtmgpnn_context *ctx, const SolverExtras &ex, const LwNoscat &p, const float *ssa, const float *g,
                    const float *lay_source, const float *lev_source, const float *sfc_source)
{
  const int ngpt = p.ngpt, nlay = p.nlay, ncol = p.ncol, nmus = p.nmus;
  if (ncol == 0) return RRTMGPNN_OK;
  if (nmus < 1 || nmus > 4) return fail(RRTMGPNN_ERR_ARGUMENT, "lw solver: nmus must be 1..4");
  if (ngpt > 256) return fail(RRTMGPNN_ERR_UNSUPPORTED, "lw rescaled solver: more than 256 g-points");
  LwAngles a{};
  a.nmus = nmus;
  for (int i = 0; i < nmus; i++) { a.D[i] = p.Ds[i]; a.w[i] = p.wts[i]; }
  const int threads = (ngpt + 63) / 64 * 64;
  const bool jac = ex.jac_up != nullptr;
  if (jac && (ex.gpt_up || ex.gpt_dn || ex.byband()))
    return fail(RRTMGPNN_ERR_UNSUPPORTED, "lw rescaled solver: the flux Jacobian comes without g-point or by-band outputs");
  if (jac && !ex.sfc_jac) return fail(RRTMGPNN_ERR_ARGUMENT, "lw rescaled solver: the flux Jacobian needs sfc_source_Jac");
  const size_t lds = sizeof(float) * (kExpTabFloats + (size_t)(jac ? 2 : 1) * kScatRing * ngpt +
                                      (size_t)(jac ? 3 : 2) * (nlay + 1) * 4);
  if (lds > 64 * 1024) return fail(RRTMGPNN_ERR_UNSUPPORTED, "lw rescaled solver: too many layers for LDS partials");
  void *ws = nullptr;
  const int planes = nmus > 1 ? (jac ? 5 : 4) : 2;
  if (int rc = ctx->workspace(sizeof(float) * planes * (size_t)ngpt * (nlay + 1) * ncol, &ws)) return rc;
  if ((ex.gpt_up == nullptr) != (ex.gpt_dn == nullptr))
    return fail(RRTMGPNN_ERR_ARGUMENT, "lw solver: g-point outputs need both gpt_flux_up and gpt_flux_dn");
  if (ex.byband() && ex.bnd_dir) return fail(RRTMGPNN_ERR_ARGUMENT, "lw solver: bnd_flux_dn_dir is not a longwave output");
  if (ex.byband() && ex.gpt_up)
    return fail(RRTMGPNN_ERR_UNSUPPORTED, "lw solver: by-band and g-point outputs in one call (rrtmgpnn_sum_byband "
                                          "reduces g-point fluxes)");
  // by band, or the Jacobian (never both, and the Jacobian without g-point outputs: refused above)
  const bool bb = ex.byband();
  const uint32_t options = jac ? kResclOptJac : (bb ? kResclOptBand : 0u);
  return launch_listed(ctx, kSolverLwRescl, LwResclInstances{}, options, [&](auto oc) -> int {
    hipLaunchKernelGGL(lw_rescl_kernel<decltype(oc)::value>, dim3(ncol), dim3(threads), lds, ctx->stream, ngpt, nlay,
                       ncol, p.top_at_1, a, p.inc_flux, p.tau, ssa, g, lay_source, lev_source, p.sfc_emis, sfc_source,
                       (float *)ws, p.flux_up, p.flux_dn, ex.gpt_up, ex.gpt_dn, bb ? band_out(ex) : BandOut{},
                       ex.sfc_jac, ex.jac_up);
    RRTMGPNN_LAUNCH_CHECK("lw_rescl_kernel");
    return RRTMGPNN_OK;
  });
}

// lw_rescl_planck_inc_kernel's LDS in bytes; dual: two rings, four part planes
static size_t lw_rescl_planck_lds(int nbnd, int nlay, int ngpt, bool dual)
{
  return sizeof(float) * (kExpTabFloats + lw_btab_floats(nbnd, nlay) + (size_t)(dual ? 2 : 1) * kScatRing * ngpt +
                          (size_t)(dual ? 4 : 2) * (nlay + 1) * 4);
}

// The instances lw_rescl_planck_inc_kernel is compiled for: {mask} x {aerosol} x {dual}
using LwResclIncInstances =
    SolverInstances<0u, kScatOptMask, kScatOptAer, kScatOptAer | kScatOptMask, kScatOptDual, kScatOptDual | kScatOptMask,
                    kScatOptDual | kScatOptAer, kScatOptDual | kScatOptAer | kScatOptMask>;

// What a launch of lw_rescl_planck_inc_kernel is refused for, in this order, and the workspace it is given: the one set
// of limits of launch_lw_rescl_planck_inc and, ahead of its clear launch, launch_lw_rescl_planck_clr_all.  flux_up_clr
// set: the dual instance.  *lds: the launch's LDS in bytes.
static int lw_rescl_planck_limits(rrtmgpnn_context *ctx, const SolverExtras &ex, const LwNoscat &p, int nbnd,
                                  const float *flux_up_clr, const float *flux_dn_clr, size_t *lds, void **ws)
{
  if (p.nmus < 1 || p.nmus > 4) return fail(RRTMGPNN_ERR_ARGUMENT, "lw solver: nmus must be 1..4");
  if (p.ngpt > 256) return fail(RRTMGPNN_ERR_UNSUPPORTED, "lw rescaled solver: more than 256 g-points");
  if (ex.byband() || ex.gpt_up || ex.gpt_dn || ex.jac_up || ex.lw_Ds)
    return fail(RRTMGPNN_ERR_UNSUPPORTED, "lw rescaled solver (fused Planck, band increment): broadband fluxes only");
  const bool dual = flux_up_clr != nullptr;
  if (dual && (!flux_dn_clr || p.nmus != 1))
    return fail(RRTMGPNN_ERR_UNSUPPORTED, "lw rescaled solver (fused Planck, band increment): the dual instance runs one "
                                          "angle and writes both clear-sky arrays");
  *lds = lw_rescl_planck_lds(nbnd, p.nlay, p.ngpt, dual);
  if (*lds > 64 * 1024) return fail(RRTMGPNN_ERR_UNSUPPORTED, "lw rescaled solver: too many layers for LDS partials");
  // the shared radn_dn / radn_up plane, and the two angle accumulators (as many as the no-scattering clear launch of
  // launch_lw_rescl_planck_clr_all accumulates in)
  const int planes = p.nmus > 1 ? 3 : 1;
  return ctx->workspace(sizeof(float) * planes * (size_t)p.ngpt * (p.nlay + 1) * p.ncol, ws);
}

// in.tau_bnd, ssa_bnd, g_bnd: the band-resolved two-stream increment; ex.mask_bits, or null: the McICA mask that
// switches it; ex.aer_tau, or null: the 1scl aerosol in front of it (from the _clr_all entry only: _1rescl_planck_inc
// refuses the request).  flux_up_clr / flux_dn_clr set (both; one angle): the dual instance.  No other extras have an
// instance (the entries refuse them).
int launch_lw_rescl_planck_inc(rrtmgpnn_context *ctx, const SolverExtras &ex, const LwNoscat &p, const LwPlanckIn &in,
                               const float *ssa_bnd, const float *g_bnd, float *flux_up_clr, float *flux_dn_clr)
{
  const int ngpt = p.ngpt, nlay = p.nlay, ncol = p.ncol, nmus = p.nmus;
  if (ncol == 0) return RRTMGPNN_OK;
  size_t lds = 0;
  void *ws = nullptr;
  if (int rc = lw_rescl_planck_limits(ctx, ex, p, in.bands.nbnd, flux_up_clr, flux_dn_clr, &lds, &ws)) return rc;
  const bool dual = flux_up_clr != nullptr;
  LwAngles a{};
  a.nmus = nmus;
  for (int i = 0; i < nmus; i++) { a.D[i] = p.Ds[i]; a.w[i] = p.wts[i]; }
  const int threads = (ngpt + 63) / 64 * 64;
  const uint32_t options = (ex.mask_bits ? kScatOptMask : 0u) | (ex.aer_tau ? kScatOptAer : 0u) | (dual ? kScatOptDual : 0u);
  return launch_listed(ctx, kSolverLwResclInc, LwResclIncInstances{}, options, [&](auto oc) -> int {
    constexpr uint32_t O = decltype(oc)::value;
    // the kAer / kDual instances have their own arguments behind the others' list
    ScatDualArgs<(O & (kScatOptAer | kScatOptDual)) != 0> da{};
    if constexpr ((O & (kScatOptAer | kScatOptDual)) != 0) da = {ex.aer_tau, flux_up_clr, flux_dn_clr};
    hipLaunchKernelGGL(lw_rescl_planck_inc_kernel<O>, dim3(ncol), dim3(threads), lds, ctx->stream, ngpt, nlay, ncol,
                       p.top_at_1, a, p.inc_flux, p.tau, in.pfrac, in.tau_bnd, ssa_bnd, g_bnd, p.sfc_emis, in.pl,
                       in.bands, ex.mask_bits, (float *)ws, p.flux_up, p.flux_dn, da);
    RRTMGPNN_LAUNCH_CHECK("lw_rescl_planck_inc_kernel");
    return RRTMGPNN_OK;
  });
}

// rte_lw of extensions/mo_rrtmgp_clr_all_sky.F90:146-172 for scattering clouds (rte/mo_rte_lw.F90:372-387): clear-sky
// fluxes of tau [+ ex.aer_tau] without scattering, all-sky fluxes of that incremented by the (masked) two-stream cloud
// through the rescaled solver.  dual (one angle only, and where the dual instance's LDS fits: it holds one more ring and
// two more part planes than the single one, so at large nlay x nbnd the two launches still serve): one launch of the
// dual instance; otherwise the no-scattering launcher (the aerosol as its increment) and the non-dual instance back to
// back on the context's stream.  Identical bits either way.  The mask belongs to the all-sky launch only.  The all-sky
// launcher's limits and workspace are checked before the clear launch is issued, so a refused call writes nothing.
int launch_lw_rescl_planck_clr_all(rrtmgpnn_context *ctx, const SolverExtras &ex, bool dual, const LwNoscat &p,
                                   const LwPlanckIn &in, const float *ssa_bnd, const float *g_bnd, float *flux_up_clr,
                                   float *flux_dn_clr)
{
  if (p.ncol == 0) return RRTMGPNN_OK;
  if (dual && p.nmus == 1 && lw_rescl_planck_lds(in.bands.nbnd, p.nlay, p.ngpt, true) <= 64 * 1024)
    return launch_lw_rescl_planck_inc(ctx, ex, p, in, ssa_bnd, g_bnd, flux_up_clr, flux_dn_clr);
  {
    // the non-dual all-sky launch's limits and workspace, ahead of the clear launch
    size_t lds = 0;
    void *ws = nullptr;
    if (int rc = lw_rescl_planck_limits(ctx, ex, p, in.bands.nbnd, nullptr, nullptr, &lds, &ws)) return rc;
  }
  SolverExtras clear_ex = ex;
  clear_ex.mask_bits = nullptr;
  clear_ex.aer_tau = nullptr;
  LwNoscat clear = p;
  clear.flux_up = flux_up_clr;
  clear.flux_dn = flux_dn_clr;
  LwPlanckIn clear_in = in;
  clear_in.tau_bnd = ex.aer_tau;
  if (int rc = launch_lw_noscat_planck(ctx, clear_ex, clear, clear_in)) return rc;
  return ctx->second_solver_launch(launch_lw_rescl_planck_inc(ctx, ex, p, in, ssa_bnd, g_bnd, nullptr, nullptr));
}

int launch_lw_2stream(rrtmgpnn_context *ctx, const SolverExtras &ex, int ngpt, int nlay, int ncol, int top_at_1,
                      const float *inc_flux, const float *tau, const float *ssa, const float *g,
                      const float *lev_source, const float *sfc_emis, const float *sfc_source, float *flux_up,
                      float *flux_dn)
{
  if (ncol == 0) return RRTMGPNN_OK;
  if (ngpt > 256) return fail(RRTMGPNN_ERR_UNSUPPORTED, "lw two-stream solver: more than 256 g-points");
  const int threads = (ngpt + 63) / 64 * 64;
  const size_t lds = sizeof(float) * (kExpTabFloats + (size_t)2 * kScatRing * ngpt + (size_t)2 * (nlay + 1) * 4);
  if (lds > 64 * 1024) return fail(RRTMGPNN_ERR_UNSUPPORTED, "lw two-stream solver: too many layers for LDS partials");
  void *ws = nullptr;
  if (int rc = ctx->workspace(sizeof(float) * 2 * (size_t)ngpt * (nlay + 1) * ncol, &ws)) return rc;
  if ((ex.gpt_up == nullptr) != (ex.gpt_dn == nullptr))
    return fail(RRTMGPNN_ERR_ARGUMENT, "lw solver: g-point outputs need both gpt_flux_up and gpt_flux_dn");
  if (ex.byband() && ex.bnd_dir) return fail(RRTMGPNN_ERR_ARGUMENT, "lw solver: bnd_flux_dn_dir is not a longwave output");
  if (ex.byband() && ex.gpt_up)
    return fail(RRTMGPNN_ERR_UNSUPPORTED, "lw solver: by-band and g-point outputs in one call (rrtmgpnn_sum_byband "
                                          "reduces g-point fluxes)");
  if (ex.byband())
    hipLaunchKernelGGL(lw_2stream_kernel<true>, dim3(ncol), dim3(threads), lds, ctx->stream, ngpt, nlay, ncol, top_at_1,
                       inc_flux, tau, ssa, g, lev_source, sfc_emis, sfc_source, (float *)ws, flux_up, flux_dn,
                       ex.gpt_up, ex.gpt_dn, band_out(ex));
  else
    hipLaunchKernelGGL(lw_2stream_kernel<false>, dim3(ncol), dim3(threads), lds, ctx->stream, ngpt, nlay, ncol,
                       top_at_1, inc_flux, tau, ssa, g, lev_source, sfc_emis, sfc_source, (float *)ws, flux_up, flux_dn,
                       ex.gpt_up, ex.gpt_dn, BandOut{});
  RRTMGPNN_LAUNCH_CHECK("lw_2stream_kernel");
  return RRTMGPNN_OK;
}

}  // namespace rrtmgpnn
