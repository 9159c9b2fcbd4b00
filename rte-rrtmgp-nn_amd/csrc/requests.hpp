// requests.hpp -- the per-call requests of the solver entries: what a context holds armed, what one call's options are,
// and the policy by which each entry answers each request.  No HIP here: the unit builds and runs on a host alone
// (tests/test_request_policy_host.py).
#pragma once
#include <cstdint>
#include <string>

#include "../../include/rrtmgpnn.h"

namespace rrtmgpnn {

int fail(int code, const std::string &msg);

constexpr int kMaxBands = 64;

// band limits as a kernel argument: 1-based inclusive (first, last) g-point per band
struct BandArgs {
  int lims[2 * kMaxBands];
  int nbnd;
};
int band_args(int nbnd, const int *lims, int ngpt, BandArgs &b);

// A solver call's options, beyond the problem itself.  The entry (api.cpp) builds one on its stack -- the requested
// part from the context's armed requests (apply_requests), the rest from its own arguments -- and hands it to the
// launchers, which read it and nothing else: a launcher's signature says that it honours options, its body which.
// Which entry honours which request: kRequestPolicies (requests.cpp), the one statement of it.
struct SolverExtras {
  // rte_lw's lw_Ds and ty_fluxes_flexible's g-point outputs, (ngpt, nlay+1, ncol) each (the *_gpt entries)
  const float *lw_Ds = nullptr;
  float *gpt_up = nullptr, *gpt_dn = nullptr, *gpt_dir = nullptr;
  // ty_fluxes_byband's by-band outputs, (nbnd, nlay+1, ncol) each, and their band limits
  // (rrtmgpnn_solver_request_byband); every solver launch has by-band instances
  float *bnd_up = nullptr, *bnd_dn = nullptr, *bnd_dir = nullptr;
  BandArgs bnd{};
  bool byband() const { return bnd_up || bnd_dn || bnd_dir; }
  // McICA: the packed cloud mask (nw, nlay, ncol), nw = ceil(ngpt / 32), of the fused band increment
  // (rrtmgpnn_solver_request_cloud_mask / _byband_mcica, or the _clr_all_mcica entry's argument)
  const uint32_t *mask_bits = nullptr;
  // rte_lw's flux_up_Jac (rrtmgpnn_solver_request_jacobian): d flux_up / d T_sfc, (nlay+1, ncol), carried beside the
  // up pass from sfc_jac (ngpt, ncol) -- null on the fused-Planck path, which forms it in-kernel.  Only the LW
  // no-scattering and rescaled launchers have Jacobian instances, without by-band or g-point outputs
  const float *sfc_jac = nullptr;
  float *jac_up = nullptr;
  // rrtmgpnn_solver_request_aerosol: a second, unmasked band increment (nbnd, nlay, ncol) on the call's own bands, applied
  // in front of the call's fused band increment (which a mask may switch; this one never).  aer_ssa / aer_g are both
  // null for a 1scl (LW) aerosol and both set for a 2str (SW) one.  Only the fused-Planck incremented LW launchers and
  // the checkpointed SW launcher (band-pair increment) have aerosol instances, without by-band, g-point or Jacobian
  // outputs and without lw_Ds
  const float *aer_tau = nullptr, *aer_ssa = nullptr, *aer_g = nullptr;
  // the sw_solver_2stream_clr_all entries' clear-sky outputs, (nlay+1, ncol) each: set (all three), the checkpointed SW
  // launcher runs its dual instance, which solves the clear sky (the gases and the aerosol, never the fused band
  // increment) beside the all-sky problem; broadband outputs only
  float *clr_up = nullptr, *clr_dn = nullptr, *clr_dir = nullptr;
  // rrtmgpnn_solver_request_active_columns: one device word, the number of columns (the first *nact of the call's ncol)
  // the kernel solves; only the checkpointed SW launcher has such instances, for g == NULL: kSolverSwCkActive without
  // any of the above, kSolverSwCkActiveSky beside mask_bits and / or a 2str aerosol (rows of the call's ncol both)
  const int *nact = nullptr;
  // rrtmgpnn_solver_request_sfc_byband: the by-band sums of the surface level alone, (nbnd, ncol) each, on the call's own
  // increment bands; only the checkpointed SW launcher has such instances (kSolverSwCkSfcBand), for g == NULL, the
  // band-pair layout and a cloud mask and / or a 2str aerosol, with nact or without
  float *sfc_bnd_up = nullptr, *sfc_bnd_dn = nullptr, *sfc_bnd_dir = nullptr;
  BandArgs sfc_bnd{};
  bool sfc_byband() const { return sfc_bnd_up || sfc_bnd_dn || sfc_bnd_dir; }
};

// The requests: each is armed on a context for its next solver call, which takes and clears all of them whatever it
// then returns.
// rrtmgpnn_solver_request_byband
struct BybandRequest {
  bool armed = false;
  float *up = nullptr, *dn = nullptr, *dir = nullptr;
  int nbnd = 0;
  int lims[2 * kMaxBands] = {0};
};
// rrtmgpnn_solver_request_cloud_mask
struct CloudMaskRequest {
  bool armed = false;
  // armed together with the by-band request by rrtmgpnn_solver_request_byband_mcica: the pair is meant.  A later
  // separate request of either half drops it
  bool paired = false;
  int ngpt = 0, nlay = 0, ncol = 0;
  const uint32_t *bits = nullptr;
};
// rrtmgpnn_solver_request_jacobian
struct JacobianRequest {
  bool armed = false;
  int ngpt = 0, nlay = 0, ncol = 0;
  const float *sfc_jac = nullptr;
  float *flux_up = nullptr;
};
// rrtmgpnn_solver_request_aerosol
struct AerosolRequest {
  bool armed = false;
  int nbnd = 0, nlay = 0, ncol = 0;
  const float *tau = nullptr, *ssa = nullptr, *g = nullptr;
};
// rrtmgpnn_solver_request_active_columns
struct ActiveRequest {
  bool armed = false;
  int ncol = 0;
  const int *nact = nullptr;
};
// rrtmgpnn_solver_request_sfc_byband
struct SfcBybandRequest {
  bool armed = false;
  float *up = nullptr, *dn = nullptr, *dir = nullptr;
  int nbnd = 0, ncol = 0;
  int lims[2 * kMaxBands] = {0};
};
struct ArmedRequests {
  BybandRequest byband;
  CloudMaskRequest cloud_mask;
  JacobianRequest jacobian;
  AerosolRequest aerosol;
  ActiveRequest active;
  SfcBybandRequest sfc_byband;
  bool any() const
  {
    return byband.armed || cloud_mask.armed || jacobian.armed || aerosol.armed || active.armed || sfc_byband.armed;
  }
};

// What one solver entry does with each kind of request: one row of kRequestPolicies per entry (a *_gpt twin shares its
// entry's row), applied by apply_requests.
constexpr const char *kTake = nullptr;  // in place of a refusal's text: the entry takes the request
enum class TakeJacobian { kRefuse, kSources, kFused };  // kSources needs the request's sfc_source_Jac, kFused none
enum class TakeAerosol { kRefuse, k1scl, k2str };
enum class TakeActive { kRefuse, kAlone, kBesideSky };  // kBesideSky: also beside a cloud mask and / or an aerosol
struct RequestPolicy {
  const char *entry;
  const char *byband_refusal;  // after the entry's name, or kTake
  const char *mask_refusal;  // whole, or kTake: alone, or beside a taken by-band request as the _byband_mcica pair
  TakeJacobian jacobian;
  const char *jacobian_refusal;  // kRefuse: whole, or null: the entry's name and the default text
  TakeAerosol aerosol;
  TakeActive active;
  // the aerosol is looked at ahead of the by-band request (the two lw_solver_noscat_planck_clr_all rows)
  bool aerosol_ahead_of_byband = false;
  // the entry takes rrtmgpnn_solver_request_sfc_byband (beside a taken cloud mask and / or aerosol)
  bool sfc_byband = false;
};

// the call's extents, and whether it has g-point outputs (a *_gpt entry given at least one): neither a flux Jacobian
// nor an active-column count goes with those
struct CallDims {
  int ngpt, nbnd, nlay, ncol;
  bool gpt_outputs;
};

// The entry's answer to what was armed: RRTMGPNN_OK with the requested part of `ex` filled, or the refusal.  Allocates
// nothing when nothing is armed.
int apply_requests(const RequestPolicy &policy, const ArmedRequests &taken, const CallDims &dims, SolverExtras &ex);

// the table's rows, one per entry
enum PolicyRow {
  kRowLwNoscat, kRowLwNoscatPlanck, kRowLwNoscatPlanckInc, kRowLwNoscatPlanckClrAll, kRowLwNoscatPlanckClrAllMcica,
  kRowLw1rescl, kRowLw1resclPlanckInc, kRowLw1resclPlanckClrAll, kRowLw2stream, kRowSw2stream, kRowSwNoscat,
  kRowSw2streamInc, kRowSw2streamClrAll, kRowSw2streamRfmip, kRowSw2streamRfmipClrAll, kNumPolicyRows
};
extern const RequestPolicy kRequestPolicies[kNumPolicyRows];

}  // namespace rrtmgpnn
