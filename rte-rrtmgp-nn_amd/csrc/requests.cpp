// requests.cpp -- which solver entry honours which request (the table), and the one function that applies a row.
#include "requests.hpp"

namespace rrtmgpnn {

// the refusals that name other entries, whole or after the refusing entry's name
static constexpr char kNoMaskMsg[] = "solver_request_cloud_mask: this solver entry takes no cloud mask (the _planck_inc, "
                                     "_2stream_inc, _2stream_rfmip, _2stream_clr_all and _2stream_rfmip_clr_all entries do)";
static constexpr char kMaskIsArgumentMsg[] = "lw_solver_noscat_planck_clr_all_mcica: the cloud mask is this entry's "
                                             "mask_bits argument, not a solver_request_cloud_mask request";
static constexpr char kNoActiveMsg[] = "solver_request_active_columns: this solver entry takes no active-column count (the "
                                       "sw_solver_2stream, sw_solver_2stream_inc and sw_solver_2stream_rfmip entries do)";
static constexpr char kNoSfcBybandMsg[] = "solver_request_sfc_byband: this solver entry takes no surface by-band request "
                                          "(the sw_solver_2stream_inc and sw_solver_2stream_rfmip entries do)";
static constexpr char kNoJacobianTail[] = ": no flux Jacobian from this entry (the lw_solver_noscat, _noscat_planck, "
                                          "_noscat_planck_inc and _1rescl entries have it)";
static constexpr char kNoJacobian2streamMsg[] = "rte_lw: can't provide Jacobian of fluxes w.r.t surface temperature with "
                                                "2-stream";
static constexpr char kNoAerosolTail[] = ": this solver entry takes no aerosol request (the lw_solver_noscat_planck_inc, "
                                         "_planck_clr_all, _planck_clr_all_mcica, sw_solver_2stream_inc, "
                                         "sw_solver_2stream_rfmip, sw_solver_2stream_clr_all and "
                                         "sw_solver_2stream_rfmip_clr_all entries do)";
static constexpr char kNoBybandPlanck[] = ": by-band outputs are not available from this entry (the _planck and "
                                          "_planck_inc entries have them)";
static constexpr char kNoByband1rescl[] = ": by-band outputs are not available from this entry (the lw_solver_1rescl entry "
                                          "has them, without a mask)";
static constexpr char kNoBybandSw[] = ": by-band outputs are not available from this entry (the sw_solver_2stream_inc and "
                                      "sw_solver_2stream_rfmip entries have them)";

// The table: the only statement of which entry honours which request.  A row reads entry; by-band; cloud mask; flux
// Jacobian and its refusal; aerosol; active-column count; (aerosol ahead of by-band; surface by-band outputs).
using J = TakeJacobian;
using A = TakeAerosol;
using N = TakeActive;
constexpr RequestPolicy kRequestPolicies[kNumPolicyRows] = {
    // lw_solver_noscat_GaussQuad (rte/kernels/mo_rte_solver_kernels.F90:332-415)
    {"lw_solver_noscat", kTake, kNoMaskMsg, J::kSources, nullptr, A::kRefuse, N::kRefuse},
    // ... behind compute_Planck_source_nn (rrtmgp/kernels/mo_gas_optics_kernels.F90:615-683)
    {"lw_solver_noscat_planck", kTake, kNoMaskMsg, J::kFused, nullptr, A::kRefuse, N::kRefuse},
    // ... and inc_1scalar_by_1scalar_bybnd (rte/kernels/mo_optical_props_kernels.F90:426-484)
    {"lw_solver_noscat_planck_inc", kTake, kTake, J::kFused, nullptr, A::k1scl, N::kRefuse},
    // rte_lw twice, clear and all sky (extensions/mo_rrtmgp_clr_all_sky.F90:146-172)
    {"lw_solver_noscat_planck_clr_all", kNoBybandPlanck, kNoMaskMsg, J::kRefuse, nullptr, A::k1scl, N::kRefuse, true},
    // ... the all sky under a McICA mask (extensions/cloud_optics/mo_cloud_sampling.F90), the entry's own argument
    {"lw_solver_noscat_planck_clr_all_mcica", kNoBybandPlanck, kMaskIsArgumentMsg, J::kRefuse, nullptr, A::k1scl,
     N::kRefuse, true},
    // rte_lw on two-stream properties, the rescaled solver (rte/mo_rte_lw.F90:372-387)
    {"lw_solver_1rescl", kTake, kNoMaskMsg, J::kSources, nullptr, A::kRefuse, N::kRefuse},
    // ... behind compute_Planck_source_nn and inc_2stream_by_2stream_bybnd (mo_optical_props_kernels.F90:430-463)
    {"lw_solver_1rescl_planck_inc", kNoByband1rescl, kTake, J::kRefuse, nullptr, A::kRefuse, N::kRefuse},
    // ... twice, clear and all sky (extensions/mo_rrtmgp_clr_all_sky.F90:146-172)
    {"lw_solver_1rescl_planck_clr_all", kNoByband1rescl, kTake, J::kRefuse, nullptr, A::k1scl, N::kRefuse},
    // lw_solver_2stream (rte/kernels/mo_rte_solver_kernels.F90:426-486)
    {"lw_solver_2stream", kTake, kNoMaskMsg, J::kRefuse, kNoJacobian2streamMsg, A::kRefuse, N::kRefuse},
    // sw_solver_2stream (rte/kernels/mo_rte_solver_kernels.F90:541-692)
    {"sw_solver_2stream", kTake, kNoMaskMsg, J::kRefuse, nullptr, A::kRefuse, N::kAlone},
    // sw_solver_noscat (rte/kernels/mo_rte_solver_kernels.F90:496-532)
    {"sw_solver_noscat", kTake, kNoMaskMsg, J::kRefuse, nullptr, A::kRefuse, N::kRefuse},
    // sw_solver_2stream behind inc_2stream_by_2stream_bybnd (rte/kernels/mo_optical_props_kernels.F90:430-463)
    {"sw_solver_2stream_inc", kTake, kTake, J::kRefuse, nullptr, A::k2str, N::kBesideSky, false, true},
    // rte_sw twice, clear and all sky (extensions/mo_rrtmgp_clr_all_sky.F90:283-304)
    {"sw_solver_2stream_clr_all", kNoBybandSw, kTake, J::kRefuse, nullptr, A::k2str, N::kRefuse},
    // sw_solver_2stream_inc behind the RFMIP driver's boundary conditions (rrtmgp_rfmip_sw.F90:403-441)
    {"sw_solver_2stream_rfmip", kTake, kTake, J::kRefuse, nullptr, A::k2str, N::kBesideSky, false, true},
    // ... twice, clear and all sky (extensions/mo_rrtmgp_clr_all_sky.F90:283-304)
    {"sw_solver_2stream_rfmip_clr_all", kNoBybandSw, kTake, J::kRefuse, nullptr, A::k2str, N::kRefuse},
};

int band_args(int nbnd, const int *lims, int ngpt, BandArgs &b)
{
  if (nbnd < 1 || nbnd > kMaxBands || !lims) return fail(RRTMGPNN_ERR_ARGUMENT, "band limits: need 1..64 bands");
  b.nbnd = nbnd;
  for (int i = 0; i < nbnd; i++) {
    b.lims[2 * i] = lims[2 * i];
    b.lims[2 * i + 1] = lims[2 * i + 1];
    if (lims[2 * i] < 1 || lims[2 * i + 1] > ngpt || lims[2 * i] > lims[2 * i + 1])
      return fail(RRTMGPNN_ERR_ARGUMENT, "band limits out of range [1, ngpt]");
  }
  return RRTMGPNN_OK;
}

namespace {

// every armed path ends here or in success: the only place a message is built
int refuse(int code, const RequestPolicy &p, const char *tail) { return fail(code, std::string(p.entry) + tail); }

int apply_active(const RequestPolicy &p, const ArmedRequests &rq, const CallDims &d, SolverExtras &ex)
{
  if (!rq.active.armed) return RRTMGPNN_OK;
  if (p.active == TakeActive::kRefuse) return fail(RRTMGPNN_ERR_ARGUMENT, kNoActiveMsg);
  if (p.active == TakeActive::kBesideSky && (rq.byband.armed || rq.jacobian.armed))
    return refuse(RRTMGPNN_ERR_UNSUPPORTED, p, ": an active-column count together with a by-band (alone or paired with a "
                                               "cloud mask) or Jacobian request");
  if (p.active == TakeActive::kAlone &&
      (rq.byband.armed || rq.cloud_mask.armed || rq.aerosol.armed || rq.jacobian.armed))
    return refuse(RRTMGPNN_ERR_UNSUPPORTED, p, ": an active-column count together with a by-band, cloud-mask, aerosol or "
                                               "Jacobian request");
  if (rq.active.ncol != d.ncol)
    return refuse(RRTMGPNN_ERR_ARGUMENT, p, ": the requested active-column count's ncol is not this call's");
  ex.nact = rq.active.nact;
  return RRTMGPNN_OK;
}

int apply_byband(const RequestPolicy &p, const ArmedRequests &rq, const CallDims &d, SolverExtras &ex)
{
  if (!rq.byband.armed) return RRTMGPNN_OK;
  if (p.byband_refusal) return refuse(RRTMGPNN_ERR_ARGUMENT, p, p.byband_refusal);
  if (int rc = band_args(rq.byband.nbnd, rq.byband.lims, d.ngpt, ex.bnd)) return rc;
  ex.bnd_up = rq.byband.up;
  ex.bnd_dn = rq.byband.dn;
  ex.bnd_dir = rq.byband.dir;
  return RRTMGPNN_OK;
}

// a set of the entry's kind (LW: 1scl, SW: 2str) on the call's own bands and extents; by-band outputs and an honoured
// flux Jacobian do not go with it (the class layers then use the materialising increment)
int apply_aerosol(const RequestPolicy &p, const ArmedRequests &rq, const CallDims &d, SolverExtras &ex)
{
  const AerosolRequest &a = rq.aerosol;
  if (!a.armed) return RRTMGPNN_OK;
  if (p.aerosol == TakeAerosol::kRefuse) return refuse(RRTMGPNN_ERR_ARGUMENT, p, kNoAerosolTail);
  if (rq.byband.armed) return refuse(RRTMGPNN_ERR_UNSUPPORTED, p, ": an aerosol increment together with by-band outputs");
  if (rq.jacobian.armed && p.jacobian != TakeJacobian::kRefuse)
    return refuse(RRTMGPNN_ERR_UNSUPPORTED, p, ": an aerosol increment together with the flux Jacobian");
  if (p.aerosol == TakeAerosol::k1scl && (a.ssa || a.g))
    return refuse(RRTMGPNN_ERR_ARGUMENT, p, ": a longwave entry takes a 1scl aerosol (ssa_aer and g_aer null)");
  if (p.aerosol == TakeAerosol::k2str && (!a.ssa || !a.g))
    return refuse(RRTMGPNN_ERR_ARGUMENT, p, ": a shortwave entry takes a 2str aerosol (ssa_aer and g_aer set)");
  if (a.nbnd != d.nbnd || a.nlay != d.nlay || a.ncol != d.ncol)
    return refuse(RRTMGPNN_ERR_ARGUMENT, p, ": the requested aerosol's extents (nbnd, nlay, ncol) are not this call's");
  ex.aer_tau = a.tau;
  ex.aer_ssa = a.ssa;
  ex.aer_g = a.g;
  return RRTMGPNN_OK;
}

// the LW entries that read source arrays need the request's sfc_source_Jac, the fused-Planck ones form it in-kernel
// and take none; by-band outputs do not go with it
int apply_jacobian(const RequestPolicy &p, const ArmedRequests &rq, const CallDims &d, SolverExtras &ex)
{
  const JacobianRequest &j = rq.jacobian;
  if (!j.armed) return RRTMGPNN_OK;
  if (p.jacobian == TakeJacobian::kRefuse)
    return p.jacobian_refusal ? fail(RRTMGPNN_ERR_ARGUMENT, p.jacobian_refusal)
                              : refuse(RRTMGPNN_ERR_ARGUMENT, p, kNoJacobianTail);
  if (rq.byband.armed) return refuse(RRTMGPNN_ERR_UNSUPPORTED, p, ": a flux Jacobian together with by-band outputs");
  if (j.ngpt != d.ngpt || j.nlay != d.nlay || j.ncol != d.ncol)
    return refuse(RRTMGPNN_ERR_ARGUMENT, p, ": the requested flux Jacobian's extents (ngpt, nlay, ncol) are not this call's");
  if (p.jacobian == TakeJacobian::kSources && !j.sfc_jac)
    return refuse(RRTMGPNN_ERR_ARGUMENT, p, ": the flux Jacobian needs sfc_source_Jac beside this entry's source arrays");
  if (p.jacobian == TakeJacobian::kFused && j.sfc_jac)
    return refuse(RRTMGPNN_ERR_ARGUMENT, p, ": sfc_source_Jac must be null, this entry forms it from the Planck fraction");
  ex.sfc_jac = j.sfc_jac;
  ex.jac_up = j.flux_up;
  return RRTMGPNN_OK;
}

int apply_mask(const RequestPolicy &p, const ArmedRequests &rq, const CallDims &d, SolverExtras &ex)
{
  const CloudMaskRequest &m = rq.cloud_mask;
  if (!m.armed) return RRTMGPNN_OK;
  if (p.mask_refusal) return fail(RRTMGPNN_ERR_ARGUMENT, p.mask_refusal);
  // both armed: only as the pair rrtmgpnn_solver_request_byband_mcica states (a by-band request left over from an
  // earlier arming beside a fresh mask is not one)
  if (rq.byband.armed && !m.paired)
    return refuse(RRTMGPNN_ERR_UNSUPPORTED, p, ": a cloud mask together with by-band outputs, requested separately "
                                               "(solver_request_byband_mcica requests the pair)");
  if (m.ngpt != d.ngpt || m.nlay != d.nlay || m.ncol != d.ncol)
    return refuse(RRTMGPNN_ERR_ARGUMENT, p, ": the requested cloud mask's extents (ngpt, nlay, ncol) are not this call's");
  ex.mask_bits = m.bits;
  return RRTMGPNN_OK;
}

// the surface level's by-band sums: beside a taken cloud mask and / or aerosol, never beside the full by-band outputs
// (whose surface level they equal) or a flux Jacobian; on the call's own bands and columns
int apply_sfc_byband(const RequestPolicy &p, const ArmedRequests &rq, const CallDims &d, SolverExtras &ex)
{
  const SfcBybandRequest &s = rq.sfc_byband;
  if (!s.armed) return RRTMGPNN_OK;
  if (!p.sfc_byband) return fail(RRTMGPNN_ERR_ARGUMENT, kNoSfcBybandMsg);
  if (rq.byband.armed)
    return refuse(RRTMGPNN_ERR_UNSUPPORTED, p, ": surface by-band outputs together with a by-band request (alone or paired "
                                               "with a cloud mask), whose surface level they are");
  if (rq.jacobian.armed)
    return refuse(RRTMGPNN_ERR_UNSUPPORTED, p, ": surface by-band outputs together with a Jacobian request");
  if (!ex.mask_bits && !ex.aer_tau)
    return refuse(RRTMGPNN_ERR_UNSUPPORTED, p, ": surface by-band outputs need a cloud mask or an aerosol request beside "
                                               "them (rrtmgpnn_solver_request_byband has the surface level in its outputs)");
  if (s.ncol != d.ncol)
    return refuse(RRTMGPNN_ERR_ARGUMENT, p, ": the requested surface by-band outputs' ncol is not this call's");
  if (s.nbnd != d.nbnd)
    return refuse(RRTMGPNN_ERR_ARGUMENT, p, ": the requested surface by-band outputs' bands are not this call's increment "
                                            "bands");
  if (int rc = band_args(s.nbnd, s.lims, d.ngpt, ex.sfc_bnd)) return rc;
  ex.sfc_bnd_up = s.up;
  ex.sfc_bnd_dn = s.dn;
  ex.sfc_bnd_dir = s.dir;
  return RRTMGPNN_OK;
}

}  // namespace

// The order of the checks, the same for every entry: active-column count, by-band, aerosol, cloud mask, flux Jacobian,
// then the g-point outputs beside what was taken, then the surface by-band outputs.  Each request is first refused where the row refuses it, then checked
// against the other armed requests, then against the call's extents, then taken into `ex`.  (Of the orders that keep
// every answer one the ladders this replaced gave for the same requests or a part of them, this one changes the fewest;
// DESIGN.md, "Solver dispatch".  The one departure, RequestPolicy::aerosol_ahead_of_byband, swaps the second and third
// step for two rows.)
int apply_requests(const RequestPolicy &p, const ArmedRequests &rq, const CallDims &d, SolverExtras &ex)
{
  if (!rq.any()) return RRTMGPNN_OK;
  if (int rc = apply_active(p, rq, d, ex)) return rc;
  if (p.aerosol_ahead_of_byband)
    if (int rc = apply_aerosol(p, rq, d, ex)) return rc;
  if (int rc = apply_byband(p, rq, d, ex)) return rc;
  if (!p.aerosol_ahead_of_byband)
    if (int rc = apply_aerosol(p, rq, d, ex)) return rc;
  if (int rc = apply_mask(p, rq, d, ex)) return rc;
  if (int rc = apply_jacobian(p, rq, d, ex)) return rc;
  if (ex.jac_up && d.gpt_outputs)
    return refuse(RRTMGPNN_ERR_UNSUPPORTED, p, ": a flux Jacobian together with g-point outputs");
  if (ex.nact && d.gpt_outputs)
    return refuse(RRTMGPNN_ERR_UNSUPPORTED, p, ": an active-column count together with g-point outputs");
  return apply_sfc_byband(p, rq, d, ex);
}

}  // namespace rrtmgpnn
