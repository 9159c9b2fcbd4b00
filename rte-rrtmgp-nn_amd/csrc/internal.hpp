// internal.hpp -- shared declarations of the rrtmgpnn runtime (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/rrtmgpnn.h"
#include "requests.hpp"

namespace rrtmgpnn {

void set_error(const std::string &msg);
int fail(int code, const std::string &msg);

#define RRTMGPNN_HIP(call)                                                                           \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      return ::rrtmgpnn::fail(RRTMGPNN_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Launch-error check after a kernel launch.
#define RRTMGPNN_LAUNCH_CHECK(name)                                                                  \
  do {                                                                                               \
    hipError_t e_ = hipGetLastError();                                                               \
    if (e_ != hipSuccess)                                                                            \
      return ::rrtmgpnn::fail(RRTMGPNN_ERR_DEVICE, std::string(name) + " launch: " + hipGetErrorString(e_)); \
  } while (0)

constexpr int kMaxLayers = 7;   // network layers (excluding input)
constexpr int kMaxInputs = 32;  // NN input features
extern int g_sw_kernel_default;  // rrtmgpnn_context_set_sw_kernel(NULL, mode)
extern int g_mlp_kernel_default;  // rrtmgpnn_context_set_mlp_kernel(NULL, mode)
extern int g_lw_clr_all_default;  // rrtmgpnn_context_set_lw_clr_all(NULL, mode)
extern int g_sw_clr_all_default;  // rrtmgpnn_context_set_sw_clr_all(NULL, mode)
extern int g_lw_scat_clr_all_default;  // rrtmgpnn_context_set_lw_scat_clr_all(NULL, mode)
// Raise a kernel's dynamic-LDS limit to 160 KiB on the current device, once per (kernel, device): a function
// attribute is per device, so a second GPU of the same process gets its own call.  Thread-safe; after the first
// call for a (kernel, device) pair it makes no HIP call (hipGraph captures stay attribute-free).
int raise_lds_limit(const void *kernel);

// BandArgs, SolverExtras and the armed requests: requests.hpp

// Planck inputs of the LW solvers that form the sources in-kernel from the Planck fraction (a kernel argument)
struct LwPlanck {
  const float *tlay, *tlev, *tsfc, *totplnk;
  int ntemp, sfc_lay;
  int emis_by_band;  // sfc_emis is (nbnd, ncol) and expanded in-kernel (rte_lw's expand)
  float tmin, tdelta;
};

// The launchers' problem descriptions: plain aggregates, brace-initialised by the entries.
// LW without scattering; sfc_emis is per g-point, or per band on the fused-Planck path with pl.emis_by_band
struct LwNoscat {
  int ngpt, nlay, ncol, top_at_1, nmus;
  const float *Ds, *wts, *inc_flux, *tau, *sfc_emis;
  float *flux_up, *flux_dn;
};
// ... its sources on the fused-Planck path; tau_bnd (nbnd, nlay, ncol), or null: the band increment of tau
struct LwPlanckIn {
  LwPlanck pl;
  const float *pfrac;
  BandArgs bands;
  const float *tau_bnd;
};
// SW two-stream; bands != nullptr: the atmosphere is incremented by the band-resolved 2str set (tau, ssa, g)_bnd
// in-kernel
struct Sw2Stream {
  int ngpt, nlay, ncol, top_at_1;
  const float *inc_flux, *inc_flux_dif, *tau, *ssa, *g, *mu0, *alb_dir, *alb_dif;
  const BandArgs *bands;
  const float *tau_bnd, *ssa_bnd, *g_bnd;
  float *flux_up, *flux_dn, *flux_dir;
};

}  // namespace rrtmgpnn

// Device workspace owned by a context: grown on demand, never shrunk, so steady-state calls
// (and hipGraph capture of them) perform no allocation.  A call made while the context's stream is being
// captured pins the buffer (ws_pinned): the graph holds its address, so a later call that would grow it fails
// with RRTMGPNN_ERR_ARGUMENT instead of freeing memory the graph still writes (rrtmgpnn_context_unpin_workspace
// once the graph is destroyed; or give the graph a context of its own).
struct rrtmgpnn_context {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int num_cus = 256;
  int sw_kernel = -1;  // SW two-stream kernel: 0 by ngpt, 1 / 2 g-points per lane, -1 the library default
  int mlp_max_cus = 0;  // rrtmgpnn_context_set_mlp_max_cus: CUs' worth of network blocks, 0 = all
  int mlp_kernel = -1;  // LW network tiling: 0 32x32x2 where instantiated, 1 16x16x4, -1 the library default
  int lw_clr_all = -1;  // clear + all-sky LW entry: 0 default, 1 the dual kernel, 2 two launches, -1 the library default
  int sw_clr_all = -1;  // clear + all-sky SW entries: the same modes
  int lw_scat_clr_all = -1;  // clear + all-sky LW entry for scattering clouds: the same modes
  // rrtmgpnn_context_get_mlp_path: the kernel of this context's last network launch (kind, A's and B's (K1S, H1T, H2T),
  // flags), written by the launchers
  int mlp_path[8] = {0};
  void set_mlp_path(int kind, int ak = 0, int ah1 = 0, int ah2 = 0, int bk = 0, int bh1 = 0, int bh2 = 0, int flags = 0)
  {
    const int p[8] = {kind, ak, ah1, ah2, bk, bh1, bh2, flags};
    for (int i = 0; i < 8; i++) mlp_path[i] = p[i];
  }
  // rrtmgpnn_context_get_solver_path: the kernel of this context's last solver launch (family, options value, launches
  // of the call, instances in the family's list), written by the launchers (launch_listed below)
  int solver_path[4] = {0};
  void set_solver_path(int family, uint32_t options, int listed)
  {
    const int p[4] = {family, (int)options, 1, listed};
    for (int i = 0; i < 4; i++) solver_path[i] = p[i];
  }
  // the two-launch fallbacks of the clear + all-sky calls: the status of the second launch, counted when it went out
  int second_solver_launch(int rc)
  {
    if (rc == RRTMGPNN_OK) solver_path[2] = 2;
    return rc;
  }
  // the requests armed for the next solver call on this context, which takes and clears them (requests.hpp)
  rrtmgpnn::ArmedRequests armed;
  void *ws = nullptr;
  size_t ws_bytes = 0;
  bool ws_pinned = false;
  int workspace(size_t bytes, void **out);
  // device data environment (present.cpp): a caching pool of device buffers and the host -> device map
  struct Present {
    void *dev = nullptr;
    size_t bytes = 0;
    int state = 0;  // 0 host newer, 1 both current, 2 device newer
    uint64_t gen = 0;  // the host array's process-wide generation this copy was made at (present.cpp)
  };
  std::multimap<size_t, void *> pool_free;      // capacity -> buffer
  std::unordered_map<void *, size_t> pool_live;  // buffer -> capacity
  std::unordered_map<const void *, Present> present;
  int pool_get(size_t bytes, void **out);
  void pool_put(void *p);
  void pool_clear();
  // pinned staging ring for host <-> device copies of pageable host arrays: the host side is one memcpy into the
  // ring, the DMA runs asynchronously on the stream; the ring is reused after sync(), which also completes the
  // device-to-host copies queued in pending_d2h
  void *pin = nullptr;
  size_t pin_cap = 0, pin_head = 0;
  struct PendingD2H {
    void *dst;
    const void *src;
    size_t bytes;
  };
  std::vector<PendingD2H> pending_d2h;
  int h2d(void *dst, const void *host, size_t bytes);
  int d2h(void *host, const void *dev, size_t bytes);
  int sync();
};

// A network: host copy of the model + device images.
//   d_raw    : plain weights (n_in, n_out) per layer + biases (generic forward path)
//   d_packed : MFMA operand image for the fused 3-layer kernel (see kernels_nn.hip)
struct rrtmgpnn_network {
  int device = 0;
  int nlayers = 0;
  int dims[rrtmgpnn::kMaxLayers + 1] = {0};
  int act[rrtmgpnn::kMaxLayers] = {0};
  std::vector<std::vector<float>> w, b;
  std::vector<float> in_min, in_max, out_mean, out_std;
  std::vector<std::string> input_names;
  float *d_raw = nullptr;
  size_t raw_w_off[rrtmgpnn::kMaxLayers] = {0}, raw_b_off[rrtmgpnn::kMaxLayers] = {0};
  // packed MFMA image (3-layer networks only)
  float *d_packed = nullptr;
  int packed_floats = 0;
  int k1s = 0, h1t = 0, h2t = 0, ngt = 0;
  int off_l1 = 0, off_l2 = 0, off_l3 = 0, off_b1 = 0, off_b2 = 0, off_b3 = 0, off_std = 0, off_mean = 0;
  // packed image of the 32x32x2 kernel (kernels_nn32.hip; 3-layer networks with hidden widths <= 64):
  // s32 = KS, HT1, N2, HT2, N3, NGT
  float *d_packed32 = nullptr;
  int packed32_floats = 0;
  int s32[6] = {0};
  bool has_out_scaling() const { return !out_mean.empty(); }
};

// Cloud optics (extensions/cloud_optics/mo_cloud_optics.F90 ty_cloud_optics): one device buffer holding
// the LUT or Pade tables in the file's Fortran layout; off[] are float offsets into it
//   LUT : ext/ssa/asy liquid (nsize_liq, nband) [0..2], ice (nsize_ice, nband, nrghice) [3..5]
//   Pade: ext/ssa/asy liquid (nband, nsizereg, ncoef) [0..2], ice (..., nrghice) [3..5], size-regime
//         bounds [6..11]
struct rrtmgpnn_cloud_optics {
  int device = 0;
  int lut_mode = 1;
  int nband = 0, nsize_liq = 0, nsize_ice = 0, nrghice = 0, nsizereg = 0, ncoef_ext = 0, ncoef_ssa = 0;
  int icergh = 1;
  float radliq_lwr = 0, radliq_upr = 0, radice_lwr = 0, radice_upr = 0, liq_step = 0, ice_step = 0;
  std::vector<float> band_lims_wvn;
  float *d_tab = nullptr;
  size_t off[12] = {0};
};

namespace rrtmgpnn {
// The solver kernels' compile-time options.  Each kernel family takes one options value, an OR of its bits below, and
// turns it back into its named constexpr flags in its first lines.  A launcher has three parts: a select_* function
// that maps the call (its extras and argument struct) to the options value or to a refusal, one list of the options
// values the family compiles (SolverInstances), and launch_listed, which walks that list and hands the matching
// instance to the launcher's generic lambda.  rrtmgpnn_context_get_solver_path reports (family, options) of the last
// launch; include/rrtmgpnn.h documents these values, tests/test_gpu_solver_dispatch.py holds them to the table.
enum SolverFamily {
  kSolverNone = 0,
  kSolverLwNoscat = 1,     // lw_noscat_kernel (kernels_rte.hip)
  kSolverSwCk = 2,         // sw_2stream_ck_kernel (kernels_sw_ck.hip)
  kSolverLwResclInc = 3,   // lw_rescl_planck_inc_kernel (kernels_lw_scat.hip)
  kSolverLwRescl = 4,      // lw_rescl_kernel (kernels_lw_scat.hip)
  kSolverSw2Stream = 5,    // sw_2stream_kernel (kernels_rte.hip)
  kSolverSwX2 = 6,         // sw_2stream_x2_kernel (kernels_sw_x2.hip)
  kSolverSwCkActive = 7,   // sw_2stream_ck_kernel, the active-count instances (rrtmgpnn_solver_request_active_columns)
  kSolverSwCkActiveSky = 8,  // ... those beside a cloud mask and / or an aerosol (a McICA step on daylit columns)
  kSolverSwCkSfcBand = 9  // sw_2stream_ck_kernel, the surface by-band instances (rrtmgpnn_solver_request_sfc_byband)
};
// lw_noscat_kernel
constexpr uint32_t kLwOptFused = 1, kLwOptInc = 2, kLwOptMulti = 4, kLwOptBand = 8, kLwOptDual = 16, kLwOptMask = 32,
                   kLwOptMaskS = 64, kLwOptJac = 128, kLwOptAer = 256;
// sw_2stream_ck_kernel; kSwCkSmall: the small-grid set of chunk length, ring, wave floor, lane type and prefetch
// (kCk*Small, VSmall), else the default set
constexpr uint32_t kSwCkHasG = 1, kSwCkInc = 2, kSwCkGpt = 4, kSwCkTn = 8, kSwCkEmk = 16, kSwCkBandPair = 32,
                   kSwCkBand = 64, kSwCkMask = 128, kSwCkAer = 256, kSwCkDual = 512, kSwCkSmall = 1024,
                   kSwCkActive = 2048,  // the active-column count comes from a device word (families kSolverSwCkActive,
                                        // kSolverSwCkActiveSky)
                   kSwCkSfcBand = 4096;  // by-band sums of the surface level alone (family kSolverSwCkSfcBand)
// lw_rescl_planck_inc_kernel
constexpr uint32_t kScatOptMask = 1, kScatOptAer = 2, kScatOptDual = 4;
// lw_rescl_kernel
constexpr uint32_t kResclOptBand = 1, kResclOptJac = 2;
// sw_2stream_kernel and sw_2stream_x2_kernel (the latter has no g-point instances)
constexpr uint32_t kSwOptHasG = 1, kSwOptInc = 2, kSwOptGpt = 4, kSwOptBand = 8;

// the options values a family compiles, and no others
template <uint32_t... Os>
struct SolverInstances {};
// go(std::integral_constant<uint32_t, O>) launches the family's instance O and returns its status; an options value
// that is not listed has no instance.  The launch that went out is recorded in the context
template <uint32_t... Os, class Go>
int launch_listed(rrtmgpnn_context *ctx, SolverFamily family, SolverInstances<Os...>, uint32_t o, Go &&go)
{
  int rc = RRTMGPNN_OK;
  const bool listed = ((o == Os && ((rc = go(std::integral_constant<uint32_t, Os>{})), true)) || ...);
  if (!listed) return fail(RRTMGPNN_ERR_UNSUPPORTED, "solver: no instance is compiled for the options of this call");
  if (rc == RRTMGPNN_OK) ctx->set_solver_path(family, o, (int)sizeof...(Os));
  return rc;
}

// kernels_clouds.hip
struct BandArgs;
int launch_cloud_optics(rrtmgpnn_context *ctx, const rrtmgpnn_cloud_optics *co, int ncol, int nlay, const float *clwp,
                        const float *ciwp, const float *reliq, const float *reice, float *tau, float *ssa, float *g);
int launch_increment_bybnd(rrtmgpnn_context *ctx, int ncol, int nlay, int ngpt, const BandArgs *bands, float *tau1,
                           float *ssa1, float *g1, const float *tau2, const float *ssa2, const float *g2);
int launch_heating_rate(rrtmgpnn_context *ctx, int ncol, int nlay, int k_day, float c0, float c1, const float *up,
                        const float *dn, const float *plev, float *hr);
int launch_sw_boundary(rrtmgpnn_context *ctx, int ngpt, int ncol, const float *solar_source, const float *tsi,
                       const float *sfc_alb, const float *sza, float *toa, float *alb, float *mu0);
// the RFMIP driver's SW boundary conditions as inputs of a solver launch (rrtmgpnn_sw_solver_2stream_rfmip): the
// checkpointed solver forms them in its prologue; the other solver kernels get them from launch_sw_boundary, into
// toa / alb / mu0 (scratch)
struct SwBc {
  const float *solar_source, *tsi, *sfc_alb, *sza;
  float *toa, *alb, *mu0;
};
// the device-side part: the inputs and the driver's two constants (deg_to_rad, the usecol bound)
struct SwBcDev {
  const float *solar_source, *tsi, *sfc_alb, *sza;
  float deg_to_rad, sza_max;
};
SwBcDev sw_boundary_device(const SwBc *bc);
constexpr int kSwBoundaryMaxG = 1024;
int launch_delta_scale(rrtmgpnn_context *ctx, long long n, float *tau, float *ssa, float *g, const float *fwd);
// kernels_mcica.hip: sampled_mask_max_ran / _exp_ran (mask: bytes, bits: packed words; either may be null) and
// apply_cloud_mask
int launch_sampled_mask(rrtmgpnn_context *ctx, bool exp_ran, int ngpt, int nlay, int ncol, const float *randoms,
                        const float *cloud_frac, const float *overlap, unsigned char *mask, uint32_t *bits);
// the seeded route: rng is the four device words {seed low, seed high, stream, col0} (rrtmgpnn_mcica_rng_set)
int launch_sampled_mask_seeded(rrtmgpnn_context *ctx, bool exp_ran, int ngpt, int nlay, int ncol, const uint32_t *rng,
                               const float *cloud_frac, const float *overlap, unsigned char *mask, uint32_t *bits);
// the mask of a block compacted to its daylit columns (rrtmgpnn_daylit_plan's idx and count): src is randoms, or rng
// when seeded; packed words only, row j of bits from source column idx[j], rows at or past the count untouched
int launch_sampled_mask_active(rrtmgpnn_context *ctx, bool exp_ran, bool seeded, int ngpt, int nlay, int ncol,
                               const void *src, const float *cloud_frac, const float *overlap, const int *idx,
                               const int *nact, uint32_t *bits);
int launch_mcica_randoms(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const uint32_t *rng, float *randoms);
int launch_draw_samples(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const BandArgs &bands,
                        const unsigned char *mask, const float *tau_bnd, const float *ssa_bnd, const float *g_bnd,
                        float *tau, float *ssa, float *g);
// kernels_nn.hip
struct GasArgs {
  const float *p[kMaxInputs];
  int nd[kMaxInputs];
};
int launch_nn_inputs(rrtmgpnn_context *ctx, int ncol, int nlay, int nx, const float *play, const float *tlay,
                     const GasArgs &gas, const float *in_min_max /*host 2*nx*/, float *out);
int launch_col_dry(rrtmgpnn_context *ctx, int ncol, int nlay, const float *h2o, const float *plev, float *col_dry);
int launch_tlev(rrtmgpnn_context *ctx, int ncol, int nlay, const float *play, const float *plev, const float *tlay,
                float *tlev);
enum MlpMode { MLP_PLAIN = 0, MLP_LW_PAIR = 1, MLP_SW_PAIR = 2, MLP_SW_ABS = 3, MLP_LW_BOTH = 4 };
// state the MLP kernel forms its inputs from (fused gas optics): compute_nn_inputs + get_col_dry in-kernel
struct MlpInputs {
  const float *play, *tlay, *plev, *h2o;
  int nlay;
  GasArgs gas;
  float mn[kMaxInputs], mx[kMaxInputs];
};
int launch_mlp(rrtmgpnn_context *ctx, MlpMode mode, const rrtmgpnn_network *A, const rrtmgpnn_network *B,
               long long nbatch, int ngpt, const float *x, const float *col_dry, float *out0, float *out1,
               float *out2, const MlpInputs *in = nullptr);
int launch_mlp_generic(rrtmgpnn_context *ctx, const rrtmgpnn_network *net, long long nbatch, const float *x,
                       float *out);
// launch_mlp(MLP_PLAIN) has a 16x16x4 instance for the network: a packed image of a compiled shape within 160 KiB of LDS
bool mlp_plain_instance(const rrtmgpnn_network *net);
int pack_network(rrtmgpnn_network *net);
// kernels_nn32.hip: the LW pair, LW both and SW pair modes on v_mfma_f32_32x32x2_f32; RRTMGPNN_ERR_UNSUPPORTED (no error set) when no instance
// exists for the networks (launch_mlp then runs the 16x16x4 kernel)
int pack_network32(rrtmgpnn_network *net);
int launch_mlp32(rrtmgpnn_context *ctx, MlpMode mode, const rrtmgpnn_network *A, const rrtmgpnn_network *B,
                 long long nbatch, int ngpt, const float *x, const float *col_dry, float *out0, float *out1,
                 float *out2, const MlpInputs *in, const int *nact = nullptr);
// kernels_rte.hip
int launch_planck_source(rrtmgpnn_context *ctx, int ncol, int nlay, int ngpt, int ntemp, const float *tlay,
                         const float *tlev, const float *tsfc, int sfc_lay, const BandArgs &bands,
                         float temp_ref_min, float totplnk_delta, const float *totplnk, float *sfc_source,
                         float *sfc_source_Jac, float *pfrac, float *lev_source);
int launch_lw_noscat(rrtmgpnn_context *ctx, const SolverExtras &ex, const LwNoscat &p, const float *lay_source,
                     const float *lev_source, const float *sfc_source);
int launch_lw_noscat_planck(rrtmgpnn_context *ctx, const SolverExtras &ex, const LwNoscat &p, const LwPlanckIn &in);
// clear-sky fluxes (tau) and all-sky fluxes (tau + tau_bnd) of the same columns; dual: one launch of the dual instance
// where it exists (one angle), else the two instances back to back.  ex.mask_bits, or null: the all-sky set's
// increment is switched per g-point by a McICA mask (the masked dual instance, or the masked single one)
int launch_lw_noscat_planck_clr_all(rrtmgpnn_context *ctx, const SolverExtras &ex, bool dual, const LwNoscat &p,
                                    const LwPlanckIn &in, float *flux_up_clr, float *flux_dn_clr);
// bc: the RFMIP boundary conditions, which overwrite p's inc_flux, mu0 and albedos
int launch_sw_2stream(rrtmgpnn_context *ctx, const SolverExtras &ex, Sw2Stream p, const SwBc *bc = nullptr);
// kernels_sw_x2.hip (called by launch_sw_2stream for even ngpt; ws sized by it)
size_t sw_2stream_x2_layer_planes(bool inc);
int launch_sw_2stream_x2(rrtmgpnn_context *ctx, const SolverExtras &ex, const Sw2Stream &p, void *ws);
int launch_sw_noscat(rrtmgpnn_context *ctx, const SolverExtras &ex, int ngpt, int nlay, int ncol, int top_at_1,
                     const float *inc_flux, const float *tau, const float *mu0, float *flux_dir);
// kernels_sw_ck.hip (checkpointed passes; called by launch_sw_2stream for even ngpt in mode 3)
// the checkpointed SW kernel's small-grid instance applies (clear sky, g = 0, no g-point outputs, the grid in one round)
bool sw_ck_small(const rrtmgpnn_context *ctx, int ngpt, int ncol, bool has_g, bool inc, bool gpt);
// planes: the large-grid instances' workspace planes (kCkTnNN, kCkTnInc, ...); false after that allocation failed
// dual: the clear + all-sky instances (ex.clr_up set): two skies' checkpoints and (planes) their transmittance plane
size_t sw_2stream_ck_ws_floats(int ngpt, int nlay, int ncol, bool small, bool inc, bool nn, bool planes = true,
                               bool dual = false);
// the checkpointed kernel is what launch_sw_2stream runs for this context and ngpt (without g-point outputs)
bool sw_ck_selected(const rrtmgpnn_context *ctx, int ngpt);
int launch_sw_2stream_ck(rrtmgpnn_context *ctx, const SolverExtras &ex, const Sw2Stream &p, void *ws,
                         bool planes = true, const SwBcDev *bc = nullptr);
// kernels_lw_scat.hip
int launch_lw_rescl(rrtmgpnn_context *ctx, const SolverExtras &ex, const LwNoscat &p, const float *ssa, const float *g,
                    const float *lay_source, const float *lev_source, const float *sfc_source);
// the rescaled solver on the fused-Planck path, tau incremented in-kernel by the band-resolved 2str set
// (in.tau_bnd, ssa_bnd, g_bnd), which ex.mask_bits (or null) switches per g-point; broadband fluxes only
int launch_lw_rescl_planck_inc(rrtmgpnn_context *ctx, const SolverExtras &ex, const LwNoscat &p, const LwPlanckIn &in,
                               const float *ssa_bnd, const float *g_bnd, float *flux_up_clr = nullptr,
                               float *flux_dn_clr = nullptr);
int launch_lw_rescl_planck_clr_all(rrtmgpnn_context *ctx, const SolverExtras &ex, bool dual, const LwNoscat &p,
                                   const LwPlanckIn &in, const float *ssa_bnd, const float *g_bnd, float *flux_up_clr,
                                   float *flux_dn_clr);
int launch_lw_2stream(rrtmgpnn_context *ctx, const SolverExtras &ex, int ngpt, int nlay, int ncol, int top_at_1,
                      const float *inc_flux, const float *tau, const float *ssa, const float *g,
                      const float *lev_source, const float *sfc_emis, const float *sfc_source, float *flux_up,
                      float *flux_dn);
int launch_expand(rrtmgpnn_context *ctx, int nband, int ngpt, int ncol, const BandArgs &bands, const float *in,
                  float *out);
// kernels_bc.hip (rrtmgpnn_compute_bc_lw / _sw): the one-layer problem of extensions/mo_compute_bc.F90 and its solve
// the 2-D (nlay, ncol) arrays whose top-layer values the gather copies: the gases and the h2o vmr of get_col_dry
constexpr int kBcMaxGather = kMaxInputs + 1;
struct BcGather {
  const float *p[kBcMaxGather];
  int n;
};
// out: play1 (ncol), tlay1 (ncol), plev1 (2, ncol), then src.n arrays of (ncol); top_lay 1-based
constexpr size_t bc_inputs_floats(int ncol, int ngather) { return (size_t)ncol * (4 + ngather); }
int launch_bc_inputs(rrtmgpnn_context *ctx, int ncol, int nlay, int top_lay, float press_min, const float *plev,
                     const float *tlay, const BcGather &src, float *out);
int launch_bc_flux_lw(rrtmgpnn_context *ctx, int ngpt, int ncol, const float *tau, const float *pfrac,
                      const float *tlay1, const LwPlanck &pl, const BandArgs &bands, int nmus, const float *Ds,
                      const float *wts, int as_flux, float *flux_bc);
int launch_bc_flux_sw(rrtmgpnn_context *ctx, int ngpt, int ncol, const float *tau, const float *solar_source,
                      const float *mu0, float *flux_bc);
// kernels_daylit.hip (rrtmgpnn_daylit_plan / _gather_columns / _scatter_columns): the daylit columns of a block, their
// rows gathered into dense arrays, and the dense fluxes scattered back with zeros at night
constexpr int kDaylitMaxGather = 16, kDaylitMaxScatter = 6;
// n arrays of row[a] floats per column; gather: row idx[j] of src to row j of dst; scatter: row slot[i] of src to row i
struct ColumnTable {
  const float *src[kDaylitMaxGather];
  float *dst[kDaylitMaxGather];
  int row[kDaylitMaxGather];
  int n;
};
int launch_daylit_plan(rrtmgpnn_context *ctx, int ncol, const float *v, int kind, float bound, int *idx, int *slot,
                       int *nday);
int launch_gather_columns(rrtmgpnn_context *ctx, int ncol, const ColumnTable &t, const int *idx, const int *nday);
int launch_scatter_columns(rrtmgpnn_context *ctx, int ncol, const ColumnTable &t, const int *slot);
// kernels_fluxes.hip: sum_byband of a g-point array (ngpt, nlev, ncol) into (nbnd, nlev, ncol)
int launch_sum_byband(rrtmgpnn_context *ctx, int ngpt, long long nrow, const BandArgs &bands, const float *gpt_flux,
                      float *bnd_flux);
}  // namespace rrtmgpnn
