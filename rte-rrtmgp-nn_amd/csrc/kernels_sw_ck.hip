// kernels_sw_ck.hip -- the SW two-stream solver with checkpointed passes (two g-points per lane, packed fp32).
//
// Same arithmetic as sw_2stream_x2_kernel (kernels_sw_x2.hip) and so the same bits as the reference's
// sw_solver_2stream + sw_two_stream_source + adding (rte/kernels/mo_rte_solver_kernels.F90:541-692, 1366-1480,
// 1526-1637), but the three per-level workspace planes (direct beam, adding albedo, adding source: 3 x 98 MB written
// and read back at C3) are replaced by checkpoints every K levels:
//
//   pass 1 (top -> bottom) : direct beam; stores the beam at the top of every chunk of K layers (1/K of a plane).
//   pass 2 (bottom -> top) : per chunk, from the chunk's beam checkpoint: the beam forward through the chunk (its
//                            transmittances exp(-tau/mu0) are the ones sw_two_stream needs anyway, passed in), then the
//                            adding albedo / source backward through it; stores them at the top of every chunk.
//   pass 3 (top -> bottom) : per chunk: sw_two_stream of its K layers (the beam carried from the top as in pass 1),
//                            albedo / source walked up from the checkpoint at the chunk's bottom (pass 2's recurrence,
//                            same expressions, same bits), then the fluxes walked down (Eqs 12-13), into the ordered
//                            broadband reduction's LDS ring.
//
// Per launch this reads tau three times and ssa twice (as before) but moves 3/K planes of checkpoints instead of 6
// planes of workspace.  The VALU work per element is pass 2's and 3's sw_two_stream plus one more adding step in pass
// 3; the K layers of a chunk are independent until the recurrences, which gives the scheduler K-wide ILP.
// Workspace: (ngpt, 3 nck + 2, ncol) checkpoints, per column nck beam rows, then nck+1 albedo and nck+1 source rows,
// nck = ceil(nlay / K); row c of each holds level c*K counted from the top, albedo / source row nck the surface.
#include "x2_device.hpp"

#include <algorithm>
#include <type_traits>

namespace rrtmgpnn {
using namespace x2;

namespace {

// V: one lane's g-points, f2 (two per lane, packed fp32) or float (one per lane)
template <class V>
struct Coef2 {
  V Rdif, Tdif, Sup, Sdn;
};

// max-by-magnitude guard of sw_two_stream's 1 - (k mu0)^2 denominator, element by element
__device__ __forceinline__ float ck_eps_guard(float v, float eps) { return (fabsf(v) >= eps) ? v : eps; }
__device__ __forceinline__ f2 ck_eps_guard(f2 v, float eps) { return (f2){ck_eps_guard(v.x, eps), ck_eps_guard(v.y, eps)}; }

// sw_two_stream (kernels_rte.hip) term by term for the K layers of a chunk, with the direct-beam transmittances
// Tnoscat = exp(-tau/mu0) given, stage by stage so that the K layers' exps share one batch of table reads
// kEmk: 0 forms exp(-tau k); 1 forms it and hands it out in emk_io; 2 takes it from emk_io (the value mode 1 handed
// out for the same layer, same bits)
template <bool kG0, int K, class V, int kEmk = 0>
__device__ __forceinline__ void ck_two_stream_k(const V (&tau)[K], const V (&w0)[K], const V (&g)[K], float mu0,
                                                const V (&Tnoscat)[K], const V (&dir_inc)[K], Coef2<V> (&c)[K],
                                                const uint64_t *etab, V (&emk_io)[K])
{
  const float eps = FLT_EPSILON, k_min = 1.e-4f;
  V gamma1[K], gamma2[K], k[K], arg[K], emk[K];
#pragma unroll
  for (int p = 0; p < K; p++) {
    if constexpr (kG0) {
      // g = 0: one rounding of the value the reference rounds at 4x and scales back exactly -- the same bits for
      // every |ssa| < 6.8e37 (tools/check_sw_identities.py walks all of those floats), two operations fewer
      gamma1[p] = 2.0f - w0[p] * 1.25f;
      gamma2[p] = w0[p] * .75f;
    } else {
      gamma1[p] = (8.0f - w0[p] * (5.0f + 3.0f * g[p])) * .25f;
      gamma2[p] = 3.0f * (w0[p] * (1.0f - g[p])) * .25f;
    }
    k[p] = sqrt2(vmax((gamma1[p] - gamma2[p]) * (gamma1[p] + gamma2[p]), (V)k_min));
    arg[p] = -tau[p] * k[p];
  }
  if constexpr (kEmk == 2) {
#pragma unroll
    for (int p = 0; p < K; p++) emk[p] = emk_io[p];
  } else {
    exp_neg_batch(arg, emk, etab);
    if constexpr (kEmk == 1) {
#pragma unroll
      for (int p = 0; p < K; p++) emk_io[p] = emk[p];
    }
  }
#pragma unroll
  for (int p = 0; p < K; p++) {
    const V em2k = emk[p] * emk[p];
    const V RTd = rcp2(k[p] * (1.0f + em2k) + gamma1[p] * (1.0f - em2k));
    c[p].Rdif = RTd * gamma2[p] * (1.0f - em2k);
    c[p].Tdif = RTd * 2.0f * k[p] * emk[p];
    const V gamma3 = kG0 ? (V)0.5f : (2.0f - 3.0f * mu0 * g[p]) * .25f;
    const V gamma4 = 1.0f - gamma3;
    // g = 0 (gamma3 = gamma4 = 1/2): alpha1 = alpha2 = (gamma1 + gamma2) / 2, the sum k's radicand already formed
    // (same bits, tools/check_sw_identities.py)
    const V alpha1 = kG0 ? (gamma1[p] + gamma2[p]) * .5f : gamma1[p] * gamma4 + gamma2[p] * gamma3;
    const V alpha2 = kG0 ? alpha1 : gamma1[p] * gamma3 + gamma2[p] * gamma4;
    const V k2e = 2.0f * k[p] * emk[p];
    const V k_mu = k[p] * mu0, k_mu2 = k_mu * k_mu, k_g3 = k[p] * gamma3, k_g4 = k[p] * gamma4;
    const V dd = ck_eps_guard(1.0f - k_mu2, eps);
    const V RT = div2(w0[p] * RTd, dd);
    const V Tn = Tnoscat[p];
    V Rdir = RT * ((1.0f - k_mu) * (alpha2 + k_g3) - (1.0f + k_mu) * (alpha2 - k_g3) * em2k -
                   k2e * (gamma3 - alpha2 * mu0) * Tn);
    V Tdir = RT * (k2e * (gamma4 + alpha1 * mu0) -
                   Tn * ((1.0f + k_mu) * (alpha1 + k_g4) - (1.0f - k_mu) * (alpha1 - k_g4) * em2k));
    Rdir = vmax((V)0.0f, vmin(Rdir, (1.0f - Tn)));
    Tdir = vmax((V)0.0f, vmin(Tdir, (1.0f - Tn - Rdir)));
    c[p].Sup = Rdir * dir_inc[p];
    c[p].Sdn = Tdir * dir_inc[p];
  }
}

// inc_2stream_by_2stream_bybnd (rte/kernels/mo_optical_props_kernels.F90:430-463) for a lane's g-points, as inc_2str2
template <class V>
__device__ __forceinline__ void ck_inc(V &t1, V &w1, V &g1, V t2, V w2, V g2)
{
  const float eps = 3.0f * FLT_MIN;
  const V tau12 = t1 + t2;
  const V tauscat12 = t1 * w1 + t2 * w2;
  g1 = (t1 * w1 * g1 + t2 * w2 * g2) / vmax((V)eps, tauscat12);
  w1 = tauscat12 / vmax((V)eps, tau12);
  t1 = tau12;
}

// the flush walks the ordered sums one lane per partial (ring_flush_sw_lanes) when the block has the lanes for it
// (C3 flush 18 us from 31 us with one lane per column); flux-ring rows are padded by 4 floats, so the lanes of one
// partial read different banks
constexpr bool kCkFlushLanes = true;
__host__ __device__ constexpr int ck_ring_stride(int ngpt) { return ngpt + 4; }

// a lane's load of one layer: its V, or (kOne: the dual instances, whose lane owns one g-point) one float
template <bool kOne, CachePolicy CP, class V>
__device__ __forceinline__ auto ck_ld(const ColArrV<V> &a, uint32_t voff, uint32_t soff)
{
  if constexpr (kOne) return a.template ld1<CP>(voff, soff);
  else return a.template ldv<CP>(voff, soff);
}

}  // namespace

// K: layers per chunk (checkpoint spacing); kCkRing: levels staged for the ordered broadband sums (a multiple of K).
// K = 3 layers per chunk under a 3-waves-per-SIMD register budget (132 VGPRs, no spill; at 4 waves K = 3 spilled and
// K = 2 fit): C3 step -3 %, C4 -1 % against K = 2 or the two-per-lane workspace kernel; K = 4 (148 VGPRs) was best
// alone at C3 but 13 % slower at C4, K = 6 spilled (tools/gpu_ab.sh, round 2).  Round 4 (the SW solver alone,
// alternating, bitwise; tools/kernel_ab.py): a ring of 9 levels (7 flushes per 60-layer column instead of 10) C4 -2.7 %;
// a 2-wave floor (no VGPR spill) +7 % with K = 3, +5 % with K = 4 / ring 8.
constexpr int kCkK = 3, kCkRing = 9, kCkWaves = 3;
// pass 1 loads kCkP1 chunks of optical depths per step (and the next step's while it computes)
constexpr int kCkP1 = 2;
// Waves per SIMD of the large-grid clear-sky NN instance (g = NULL, no increment; C5).  Round 2 chose 4 (128 VGPRs)
// when it also ran C3; since the small-grid instance took C3 over, the register floor spilled 19-21 VGPRs for no
// residency gain: at 3 (no spill) the C5 shard's SW solver runs 10 % faster alone, 12 % with the ring of 9 (round 4).
constexpr int kCkWavesNN = 3;
// Workspace planes of the large-grid instances (as the small-grid instance's kCkTnSmall / kCkEmkSmall): the clear-sky
// NN instance (C5) and the all-sky ones (C4).  Round 5 (tools/kernel_ab.py alone, tools/gpu_ab.sh whole steps;
// bitwise): the C5 shard's SW solver 32.68 -> 31.64 ms with both planes (the transmittances alone 32.24, exp(-k tau)
// alone 33.23: with both, pass 3 reads no tau), whole steps 66.63 -> 64.77 ms (2 alternating pairs); the large grid is
// then at HBM (199 GB per launch at 6.3 TB/s) where it was at its VALU floor (valu_busy 0.99, 3.35 TB/s).  C4 all sky:
// the transmittance plane 1.480 -> 1.458 ms alone (1.50 -> 1.435 in steps), steps within noise (-0.5 %); exp(-k tau)
// +1.3 %.  A/B knobs: tools/ablations.py swck_nnplanes / swck_incplanes.  The planes cost workspace (C5 shard: 15.7 ->
// 46.4 GB): when that allocation fails, launch_sw_2stream retries without them and these instances run without planes
// (the round-4 forms; same bits).
constexpr bool kCkTnNN = true, kCkEmkNN = true;
constexpr bool kCkTnInc = true, kCkEmkInc = false;
// ... and of the dual (clear + all-sky) instances, a pair per g-point each.  Without planes a lane evaluates ten exps
// per layer (two skies x (pass 1's beam, passes 2 and 3's beam and exp(-k tau))) against five in the two single-sky
// launches, which have planes, and spills (168 VGPRs, 14-66 spilled).  The SW solver alone at C4, alternating builds
// and routes on one box, two rounds (tools/sw_clr_all_ab.py, profiles/sw_clr_all_planes_c4.txt), the dual launch against
// the two launches' 2.46-2.47 ms (spread 0.03-0.05): no plane 2.709 / 2.708 (+10 %), the transmittance plane 2.424 /
// 2.443 (-1.5 %), exp(-k tau) alone 2.538 / 2.550, both 2.478 / 2.476; with a mask and aerosols 3.904, 2.871 (-10.6 %
// against 3.21), 3.007, 2.936.  So the transmittance plane alone, as in the all-sky instances (kCkTnInc).
// (The variants were builds with these two constants changed.)  When the workspace with the plane does not fit, the plane-free
// instances run (launch_sw_2stream's fallback; the same bits).
constexpr bool kCkTnDual = true, kCkEmkDual = false;

// kGpt: also store the g-point fluxes (ty_fluxes_flexible: up, total down, direct; (ngpt, nlay+1, ncol)) and sum the
// broadband down flux from the total as sw_solver_2stream does when it saves them (:572-588, :660-684)
// Small grids (the clear-sky instance when the grid fits in one round of resident waves, e.g. C3): 2 waves per SIMD
// as the register floor (more independent layers per wave where there are too few waves to hide the exps' latency);
// chunk length and ring below.  Whole-step A/B at C3 (one box, alternating): +1.3 %, SW solver -2.4 %; a ring of 4 was
// 3 % slower, K = 2 at 4 waves +0.5 %.  With many columns (C4, C5) K = 3 at 3-4 waves stays (K = 4 was 13 % slower).
// The small-grid instance also keeps pass 1's beam transmittances exp(-tau/mu0) in a workspace plane that passes 2 and
// 3 read instead of evaluating the exp again, and pass 2's exp(-tau k) in a second plane that pass 3 reads (C3: SW
// solver -3.7 %, step -3.7 %, alternating A/B on one box).  One g-point per lane (twice the waves to hide latency with;
// packed fp32 issues at the same cost per element as scalar fp32 on gfx950, tools/valu_rates.hip) measured slower than
// two.  (The transmittance plane in the all-sky instances measured slower in round 3; on the round-4 kernels it was
// faster at C4 and is on there since round 5: kCkTnInc above.)
// Round 4 (alone, alternating, bitwise; with the fence-free walk): K = 3 with a ring of 9 levels (three chunks per
// flush, 7 flushes per column instead of 8) -2.3 % against K = 4 / ring 8; K = 3 / ring 6 +3 %, K = 2 / ring 6 +5 %,
// K = 5 / ring 10 equal; a 3-wave floor equal.  A ring of 12 levels would not leave room for three blocks per CU.
constexpr int kCkKSmall = 3, kCkRingSmall = 9, kCkWavesSmall = 2;
constexpr bool kCkTnSmall = true, kCkEmkSmall = true;
using VSmall = f2;
// pass-1 chunks per load step of the small-grid instance (its pass 1 is latency-bound at C3: 10 dependent load steps
// of 6 layers per 60-layer column with the default)
constexpr int kCkP1Small = 2;
// passes 2 and 3 of the small-grid instance prefetch this many chunks ahead (three register buffers for 2): at C3
// each pass streams at 4.8-5.2 TB/s where the same 8-byte loads reach 6.3 TB/s at 3 waves per SIMD with 4 per lane in
// flight (tools/bw_width.hip), i.e. a chunk's loads are not always back when its body starts
constexpr int kCkAheadSmall = 1;

// Cache policies (CachePolicy, rte_device.hpp) of the kernel's global streams, one set per instance family: the
// small-grid clear-sky instance (C3), the large clear-sky NN instance (C5: _NN) and the all-sky instances (C4: _INC);
// every other instance keeps the default.  Each can be set from the command line (-DRRTMGPNN_CP_SW_P3_LD=2).
//   p1_ld   : pass 1's tau loads (pass 2 reads them again: a control);
//   p1_st   : pass 1's transmittance plane and beam checkpoints (read by pass 2: a control);
//   p2_last : pass 2's last-use loads: the beam checkpoint, and tau where pass 3 reads exp(-k tau) from its plane
//             instead (kEmk; without that plane tau stays default in pass 2 whatever this says);
//   p2_st   : pass 2's exp(-k tau) plane and albedo / source checkpoints (read by pass 3: a control);
//   p3_ld   : all of pass 3's loads (ssa, g, both planes, the checkpoints, and tau without the exp(-k tau) plane).
// Shipped in all three families: p2_last and p3_ld (kNT).  Alone, alternating (profiles/cache_policy_ab.txt): p3_ld C3
// -1.3 %, C4 -1.8 %; p2_last within the spread by itself; both C3 -1.6 %, C4 -1.9 %, C5 shard -2.5 %.  Whole steps with
// both (profiles/cache_policy_bench_ab.txt): C3 -2.2 %, C4 -1.45 %, C5 shard -1.25 %; without p2_last C3 -1.6 %, C5
// -0.8 %.  The controls stay default: p1_ld +2.5 % alone at C3 (+0.3 % C4), p1_st +3.3 % (+0.6 %), p2_st equal.
struct SwCkCp {
  CachePolicy p1_ld, p1_st, p2_last, p2_st, p3_ld;
};
#define RRTMGPNN_CP_(x) ((CachePolicy)(x))
#ifndef RRTMGPNN_CP_SW_P1_LD
#define RRTMGPNN_CP_SW_P1_LD 0
#endif
#ifndef RRTMGPNN_CP_SW_P1_ST
#define RRTMGPNN_CP_SW_P1_ST 0
#endif
#ifndef RRTMGPNN_CP_SW_P2_LAST
#define RRTMGPNN_CP_SW_P2_LAST 2
#endif
#ifndef RRTMGPNN_CP_SW_P2_ST
#define RRTMGPNN_CP_SW_P2_ST 0
#endif
#ifndef RRTMGPNN_CP_SW_P3_LD
#define RRTMGPNN_CP_SW_P3_LD 2
#endif
#ifndef RRTMGPNN_CP_SW_P1_LD_NN
#define RRTMGPNN_CP_SW_P1_LD_NN 0
#endif
#ifndef RRTMGPNN_CP_SW_P1_ST_NN
#define RRTMGPNN_CP_SW_P1_ST_NN 0
#endif
#ifndef RRTMGPNN_CP_SW_P2_LAST_NN
#define RRTMGPNN_CP_SW_P2_LAST_NN 2
#endif
#ifndef RRTMGPNN_CP_SW_P2_ST_NN
#define RRTMGPNN_CP_SW_P2_ST_NN 0
#endif
#ifndef RRTMGPNN_CP_SW_P3_LD_NN
#define RRTMGPNN_CP_SW_P3_LD_NN 2
#endif
#ifndef RRTMGPNN_CP_SW_P1_LD_INC
#define RRTMGPNN_CP_SW_P1_LD_INC 0
#endif
#ifndef RRTMGPNN_CP_SW_P1_ST_INC
#define RRTMGPNN_CP_SW_P1_ST_INC 0
#endif
#ifndef RRTMGPNN_CP_SW_P2_LAST_INC
#define RRTMGPNN_CP_SW_P2_LAST_INC 2
#endif
#ifndef RRTMGPNN_CP_SW_P2_ST_INC
#define RRTMGPNN_CP_SW_P2_ST_INC 0
#endif
#ifndef RRTMGPNN_CP_SW_P3_LD_INC
#define RRTMGPNN_CP_SW_P3_LD_INC 2
#endif
constexpr SwCkCp kCpSwSmall = {RRTMGPNN_CP_(RRTMGPNN_CP_SW_P1_LD), RRTMGPNN_CP_(RRTMGPNN_CP_SW_P1_ST),
                               RRTMGPNN_CP_(RRTMGPNN_CP_SW_P2_LAST), RRTMGPNN_CP_(RRTMGPNN_CP_SW_P2_ST),
                               RRTMGPNN_CP_(RRTMGPNN_CP_SW_P3_LD)};
constexpr SwCkCp kCpSwNN = {RRTMGPNN_CP_(RRTMGPNN_CP_SW_P1_LD_NN), RRTMGPNN_CP_(RRTMGPNN_CP_SW_P1_ST_NN),
                            RRTMGPNN_CP_(RRTMGPNN_CP_SW_P2_LAST_NN), RRTMGPNN_CP_(RRTMGPNN_CP_SW_P2_ST_NN),
                            RRTMGPNN_CP_(RRTMGPNN_CP_SW_P3_LD_NN)};
constexpr SwCkCp kCpSwInc = {RRTMGPNN_CP_(RRTMGPNN_CP_SW_P1_LD_INC), RRTMGPNN_CP_(RRTMGPNN_CP_SW_P1_ST_INC),
                             RRTMGPNN_CP_(RRTMGPNN_CP_SW_P2_LAST_INC), RRTMGPNN_CP_(RRTMGPNN_CP_SW_P2_ST_INC),
                             RRTMGPNN_CP_(RRTMGPNN_CP_SW_P3_LD_INC)};
constexpr SwCkCp kCpSwOther = {};
#undef RRTMGPNN_CP_

// V: f2 (two g-points per lane) or float (one per lane).  kBandPair (fused increment, two g-points per lane): every
// band starts at an even g-point, so both g-points of a lane lie in one band and its band values are one load each
// (the RRTMGP g-point sets: 16 per band).  Round 4, C4: SW solver -1.7 % alone, steps -0.8 % (3 alternating pairs)
// kMask (with kInc, two g-points per lane): the band increment is a McICA-sampled cloud
// (rrtmgpnn_solver_request_cloud_mask): bit g % 32 of word g / 32 of cmask (nw, nlay, ncol) switches (tau, ssa, g)_bnd
// on or off for g-point g -- a clear bit makes all three 0, draw_samples
// (extensions/cloud_optics/mo_cloud_sampling.F90:291-307) -- and ck_inc then increments by them as it does by any
// other values (a zero increment still rounds tau * ssa / max(eps, tau)).  Both g-points of a lane are selected
// separately (g is even, so they share the word), also in the band-pair form; the word is loaded with the layer's
// band values.  With kBand (rrtmgpnn_solver_request_byband_mcica) the flush's band sums are those of the sampled
// columns; the by-band limits are the request's, not the increment's.
// kAer (with kInc and kBandPair, two g-points per lane, no by-band or g-point outputs; rrtmgpnn_solver_request_aerosol):
// a second, unmasked band increment (tau, ssa, g)_aer on the same bands in front of the maskable one -- aerosols, then
// clouds, as rte_sw of extensions/mo_rrtmgp_clr_all_sky.F90 orders them (:288-290, :297-299): ck_inc by the aerosol,
// then ck_inc by the (selected) cloud, inc_2stream_by_2stream_bybnd twice, unchanged.  Three more band values per chunk
// layer, loaded as ld_bnd loads the cloud's; pass 1, which needs the optical depth only, takes (tau + tau_aer) +
// sel(tau_cld).  With gg == NULL the gas g going into the first increment is the literal 0, so gas optics never writes
// a g array.  The mask never touches the aerosol.
// kDual (with kInc, V = f2, no by-band or g-point outputs; rrtmgpnn_sw_solver_2stream_clr_all): clear-sky
// beside all-sky fluxes of the same columns, rte_sw twice in extensions/mo_rrtmgp_clr_all_sky.F90:283-304.  One column
// per block, lane t owns g-point t alone, and the two components of V are that g-point's two skies: .x all sky, .y
// clear.  tau, ssa, the gas g, the band values and the mask word are one scalar load per layer each; props() forms
// .y from the gas properties as loaded (with kAer: one ck_inc by the aerosol) and .x from .y's values by ck_inc with the
// (mask-selected) cloud -- the clear component is never incremented by zeros, which would still round.  With gg == NULL
// .y runs the general gamma / alpha expressions at g = 0, the bits of the kG0 short forms
// (tools/check_sw_identities.py).  The recurrences, the checkpoints ((2 ngpt, 3 nck + 2, ncol), a lane's pair at
// 8 g bytes), the planes ((2 ngpt, nlay, ncol) each) and the ring ([2 skies][3][R][rs], the footprint of two columns)
// are per sky; one flush window reduces both (ring_flush_sw*'s kSkies) and stores sky 1 to clr_up / clr_dn / clr_dir.
// kBandPair is not used: one g-point has one band whatever the limits are.
// The workspace planes (kSwCkTn | kSwCkEmk) of each instance family, from the constants above
constexpr uint32_t sw_ck_planes(bool tn, bool emk) { return (tn ? kSwCkTn : 0u) | (emk ? kSwCkEmk : 0u); }
constexpr uint32_t kSwCkPlanesNN = sw_ck_planes(kCkTnNN, kCkEmkNN), kSwCkPlanesInc = sw_ck_planes(kCkTnInc, kCkEmkInc),
                   kSwCkPlanesDual = sw_ck_planes(kCkTnDual, kCkEmkDual),
                   kSwCkPlanesSmall = sw_ck_planes(kCkTnSmall, kCkEmkSmall);
// waves per SIMD of instance O: the small-grid floor, the large-grid clear-sky NN instance's, or the others'
constexpr int sw_ck_waves(uint32_t O)
{
  return (O & kSwCkSmall) ? kCkWavesSmall : ((O & (kSwCkHasG | kSwCkInc | kSwCkGpt)) == 0 ? kCkWavesNN : kCkWaves);
}

// O: the instance's options, an OR of the kSwCk* bits (internal.hpp), named again in the first lines
template <uint32_t O>
__global__ void __launch_bounds__(512, sw_ck_waves(O))
    sw_2stream_ck_kernel(int ngpt, int nlay, int ncol, int top_at_1, int ncb, const float *__restrict__ inc_flux,
                         const float *__restrict__ inc_dif, const float *__restrict__ tau,
                         const float *__restrict__ ssa, const float *__restrict__ gg, const float *__restrict__ mu0p,
                         const float *__restrict__ alb_dir, const float *__restrict__ alb_dif, BandArgs bands,
                         const float *__restrict__ tau_bnd, const float *__restrict__ ssa_bnd,
                         const float *__restrict__ g_bnd, float *__restrict__ ws, float *__restrict__ flux_up,
                         float *__restrict__ flux_dn, float *__restrict__ flux_dir, float *__restrict__ gpt_up,
                         float *__restrict__ gpt_dn, float *__restrict__ gpt_dir, SwBcDev bc, BandOut bo,
                         const uint32_t *__restrict__ cmask, const float *__restrict__ tau_aer,
                         const float *__restrict__ ssa_aer, const float *__restrict__ g_aer,
                         float *__restrict__ clr_up, float *__restrict__ clr_dn, float *__restrict__ clr_dir)
{
  constexpr bool kHasG = (O & kSwCkHasG) != 0, kInc = (O & kSwCkInc) != 0, kGpt = (O & kSwCkGpt) != 0;
  constexpr bool kTn = (O & kSwCkTn) != 0, kEmk = (O & kSwCkEmk) != 0, kBandPair = (O & kSwCkBandPair) != 0;
  constexpr bool kBand = (O & kSwCkBand) != 0, kMask = (O & kSwCkMask) != 0, kAer = (O & kSwCkAer) != 0;
  constexpr bool kDual = (O & kSwCkDual) != 0, kSmall = (O & kSwCkSmall) != 0, kActive = (O & kSwCkActive) != 0;
  constexpr bool kSfcBand = (O & kSwCkSfcBand) != 0;
  static_assert(!kActive || (!kDual && !kGpt && !kBand && !kHasG),
                "the active-count instances: clear sky or the fused increment (masked, behind an aerosol), broadband "
                "outputs");
  // kActive (rrtmgpnn_solver_request_active_columns): the block solves columns below *nact, a device word read here,
  // before any barrier -- the word arrives in cmask's place or, in the instances that have a mask or an aerosol
  // (family kSolverSwCkActiveSky), in clr_up's, which only the dual instances use; so every other instance keeps its
  // arguments.  ncol stays the launch's in everything that lays out memory (the checkpoints pW, the planes, the mask's
  // and the aerosol's rows); nca bounds the columns a block works on and the flush stores
  int nca = ncol;
  if constexpr (kActive) {
    const int *const nactp = (kMask || kAer) ? (const int *)clr_up : (const int *)cmask;
    nca = min(max(*nactp, 0), ncol);  // never past the allocation
    if ((int)blockIdx.x * ncb >= nca) return;
  }
  // chunk length, ring levels, wave floor, pass-1 chunks per step and prefetch distance: the small-grid set or the default
  constexpr int K = kSmall ? kCkKSmall : kCkK, R = kSmall ? kCkRingSmall : kCkRing, WAVES = sw_ck_waves(O);
  constexpr int P1C = kSmall ? kCkP1Small : kCkP1, AHEAD = kSmall ? kCkAheadSmall : 1;
  using V = std::conditional_t<kSmall, VSmall, f2>;
  static_assert(R % K == 0, "the flux ring must hold whole chunks");
  static_assert(!kDual || (kInc && sizeof(V) == 8 && !kGpt && !kBand && !kBandPair),
                "the dual instances: two skies of one g-point per lane, broadband outputs");
  static_assert(!kAer || (kInc && (kBandPair || kDual) && sizeof(V) == 8 && !kGpt && !kBand),
                "the aerosol increment goes in front of the fused band-pair increment");
  static_assert(!kMask || (kInc && sizeof(V) == 8 && !kGpt), "the cloud mask switches the fused band increment");
  static_assert(!kSfcBand || (kInc && kBandPair && (kMask || kAer) && sizeof(V) == 8 && !kDual && !kGpt && !kBand &&
                              !kHasG && !kSmall),
                "the surface by-band instances: the masked cloud and / or the aerosol on the band-pair increment");
  constexpr bool kG0 = !kHasG && !kInc;  // g is the literal 0 (the NN path)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // `ncb` columns per block: lane t works on column c = t / (ngpt/NPL), g-points g .. g + NPL - 1
  constexpr int NPL = kDual ? 1 : sizeof(V) / sizeof(float);
  using CA_ = ColArrV<V>;
  using L = std::conditional_t<kDual, float, V>;  // what a lane loads of a layer's properties
  const int ncr = kDual ? 2 : ncb;  // rings in the block's LDS (kDual: ncb = 1, a ring per sky)
  const int nlev = nlay + 1, lanes = ngpt / NPL, nck = (nlay + K - 1) / K;
  const int icol0 = blockIdx.x * ncb, nc = min(ncb, nca - icol0);
  const int craw = (int)threadIdx.x / lanes;
  const bool on = craw < nc;
  const int c = on ? craw : nc - 1;
  const int g = NPL * ((int)threadIdx.x - craw * lanes);
  const int gc = on ? g : ngpt - NPL;
  const int icol = icol0 + c;
  // this column's ring [3][R][rs]: rows padded by 4 floats, so the flush threads' rows start in different LDS banks
  const int rs = ck_ring_stride(ngpt);
  float *ring = smem + kExpTabFloats + (size_t)c * 3 * R * rs;
  uint64_t *etab = (uint64_t *)(smem + kExpTabOff);
  load_exp_table(etab);
  // bc.tsi != NULL: the RFMIP driver's boundary conditions formed here (sw_boundary_kernel's expressions, same bits):
  // the solar source is staged in the ring's LDS, which pass 3 first writes after a barrier below
  const bool bcf = bc.tsi != nullptr;
  float *const bsrc = smem + kExpTabFloats;
  if (bcf)
    for (int i = threadIdx.x; i < ngpt; i += blockDim.x) bsrc[i] = bc.solar_source[i];
  // small-grid instance: the barrier comes after pass 1's first loads (kEarly below)
  constexpr bool kEarly = !kInc && WAVES == kCkWavesSmall;
  // the instance family's cache policies: small-grid clear sky, all sky, large-grid clear-sky NN, or none
  constexpr SwCkCp kCp = kEarly ? kCpSwSmall : (kInc ? kCpSwInc : ((kG0 && !kGpt) ? kCpSwNN : kCpSwOther));
  if constexpr (!kEarly) __syncthreads();
  const int dl_dn = top_at_1 ? 1 : -1;
  const uint32_t row = 4u * (uint32_t)ngpt;
  const uint32_t vL = 4u * (uint32_t)gc + (uint32_t)c * row * nlay;
  const size_t cl = (size_t)ngpt * nlay * icol0;
  const uint32_t bL = (uint32_t)nc * row * nlay;
  const CA_ Ttau(tau, cl, bL), Tssa(ssa, cl, bL), Tg(kHasG ? gg : tau, cl, bL);
  // checkpoints, column by column: (ngpt, 3 nck + 2, ncol) -- rows [0, nck) the beam, [nck, 2 nck + 1) the albedo,
  // [2 nck + 1, 3 nck + 2) the source; one buffer descriptor for the three (the layer offset in the SGPR offset)
  const int nrw = 3 * nck + 2;
  const size_t pW = (size_t)(kDual ? 2 : 1) * ngpt * nrw * ncol;
  // (kDual: rows of 2 ngpt, the lane's two skies side by side)
  const uint32_t rowW = kDual ? 2u * row : row;
  const uint32_t vW = (kDual ? 8u : 4u) * (uint32_t)gc + (uint32_t)c * rowW * nrw;
  const CA_ CW(ws, (size_t)(kDual ? 2 : 1) * ngpt * nrw * icol0, (uint32_t)nc * rowW * nrw);
  const uint32_t sA0 = rowW * (uint32_t)nck, sS0 = rowW * (uint32_t)(2 * nck + 1);
  // kTn: the beam transmittances (ngpt, nlay, ncol), addressed as tau.  kEmk: pass 2's exp(-tau k) in the plane after
  // it, which pass 3 reads instead of evaluating the exp again.  (Keeping all four coefficients R_dif, T_dif, S_up, S_dn
  // instead, so that pass 3 forms none, was 23 % slower at C3: four planes written and read cost more than they save.)
  // (kDual: planes of (2 ngpt, nlay, ncol), addressed as the checkpoints' rows: vLp, rowW)
  constexpr int kSk = kDual ? 2 : 1;
  const size_t plane = (size_t)kSk * ngpt * nlay * ncol;
  const uint32_t vLp = kDual ? 8u * (uint32_t)gc + (uint32_t)c * rowW * nlay : vL;
  const CA_ CT(kTn ? ws + pW : ws, kTn ? kSk * cl : 0, kTn ? kSk * bL : 0u);
  const CA_ CE(kEmk ? ws + pW + (kTn ? plane : 0) : ws, kEmk ? kSk * cl : 0, kEmk ? kSk * bL : 0u);
  const uint32_t vWs = on ? vW : kBufOOB;
  // band-resolved increments: one band offset per g-point of the lane
  const size_t cb = (size_t)bands.nbnd * nlay * icol0;
  const uint32_t brow = 4u * (uint32_t)bands.nbnd, vbc = (uint32_t)c * brow * nlay;
  const uint32_t vb0 = kInc ? 4u * (uint32_t)band_of(bands, gc) + vbc : 0u,
                 vb1 = kInc ? 4u * (uint32_t)band_of(bands, gc + NPL - 1) + vbc : 0u;
  const uint32_t bB = kInc ? (uint32_t)nc * brow * nlay : 0u;
  const CA_ Bt(kInc ? tau_bnd : tau, kInc ? cb : 0, bB), Bw(kInc ? ssa_bnd : tau, kInc ? cb : 0, bB),
      Bg(kInc ? g_bnd : tau, kInc ? cb : 0, bB);
  // kAer: the aerosol's arrays, on the same bands (same offsets, their own column base)
  const CA_ At(kAer ? tau_aer : tau, kAer ? cb : 0, kAer ? bB : 0u), Aw(kAer ? ssa_aer : tau, kAer ? cb : 0, kAer ? bB : 0u),
      Ag(kAer ? g_aer : tau, kAer ? cb : 0, kAer ? bB : 0u);
  auto ld_bnd = [&](const CA_ &a, int l) -> L {
    if constexpr (!kInc) return (L)0.0f;
    else if constexpr (kDual) return a.ld1(vb0, brow * (uint32_t)l);
    else if constexpr (NPL == 2 && kBandPair) {
      const float v = a.ld1(vb0, brow * (uint32_t)l);
      return (f2){v, v};
    } else if constexpr (NPL == 2) return (f2){a.ld1(vb0, brow * (uint32_t)l), a.ld1(vb1, brow * (uint32_t)l)};
    else return a.ld1(vb0, brow * (uint32_t)l);
  };
  // kMask: the lane's mask word of layer l (its column's plane of (nw, nlay, ncol)) and the selection of a band value
  // by the bits of its two g-points
  const int nw = (ngpt + 31) / 32;
  const uint32_t mrow = kMask ? 4u * (uint32_t)nw : 0u;
  const uint32_t vm = 4u * (uint32_t)(gc >> 5) + (uint32_t)c * mrow * nlay, msh = (uint32_t)(gc & 31);
  const ColArr2 Mk(kMask ? (const float *)cmask : tau, kMask ? (size_t)nw * nlay * icol0 : 0,
                   kMask ? (uint32_t)nc * mrow * nlay : 0u);
  auto ld_msk = [&](int l) -> uint32_t {
    if constexpr (kMask) return __float_as_uint(Mk.ld1(vm, mrow * (uint32_t)l));
    else return 0u;
  };
  auto sel = [&](L v, uint32_t m) -> L {
    if constexpr (kMask && kDual) return ((m >> msh) & 1u) ? v : 0.0f;
    else if constexpr (kMask && NPL == 2) {
      const uint32_t b = m >> msh;
      return (f2){(b & 1u) ? v[0] : 0.0f, (b & 2u) ? v[1] : 0.0f};
    } else return v;
  };
  // mu0 = merge(cos(sza * deg_to_rad), 1, usecol) (rrtmgp_rfmip_sw.F90:236-238, 421-427) or the caller's
  const float sza = bcf ? bc.sza[icol] : 0.0f;
  const float mu0 = bcf ? (sza < bc.sza_max ? ref_cosf(sza * bc.deg_to_rad) : 1.0f) : mu0p[icol];
  const float mu0_inv = 1.0f / mu0;
  // j counts layers from the top (clamped to the last layer); the result is the array layer
  auto lay = [&](int j) { return top_at_1 ? min(j, nlay - 1) : nlay - 1 - min(j, nlay - 1); };
  auto ld_col = [&](const float *p) -> V {
    if constexpr (kDual) return on ? (V)p[gc + (size_t)ngpt * icol] : (V)0.0f;
    else return on ? *(const V *)(p + gc + (size_t)ngpt * icol) : (V)0.0f;
  };
  const int top = top_at_1 ? 0 : nlay;
  // the surface albedo, spectrally constant (rrtmgp_rfmip_sw.F90:428-433), or the caller's per g-point
  const V alb_bc = on && bcf ? (V)bc.sfc_alb[icol] : (V)0.0f;
  // Pass 1 reads P1 = kCkP1 * K layers per step (little arithmetic per layer: it needs many loads in flight).  In the
  // small-grid instance (one round of blocks: every block's prologue is on the kernel's path) its first step's loads go
  // out here, ahead of the prologue's barrier, which would hold them back until the exp table and the solar source are
  // in LDS.  Round 6, C3: the solver alone -1.3 %; in the large clear-sky instance C5 steps +0.3 % (2 pairs), so not
  // there (profiles/r06/swearly_*.txt)
  constexpr int P1 = P1C * K;
  // (kDual: t is the clear sky's optical depth and q the cloud's, selected; the all-sky depth is their sum)
  struct Buf1 {
    L t[P1];
    L q[kDual ? P1 : 1];
  } A1, B1;
  auto load1 = [&](Buf1 &b, int c1) {
#pragma unroll
    for (int p = 0; p < P1; p++) {
      const int l = lay(c1 * P1 + p);
      b.t[p] = ck_ld<kDual, kCp.p1_ld>(Ttau, vL, row * (uint32_t)l);
      if constexpr (kAer) b.t[p] += ld_bnd(At, l);
      if constexpr (kDual) b.q[p] = sel(ld_bnd(Bt, l), ld_msk(l));
      else if constexpr (kMask) b.t[p] += sel(ld_bnd(Bt, l), ld_msk(l));
      else if constexpr (kInc) b.t[p] += ld_bnd(Bt, l);
    }
  };
  if constexpr (kEarly) {
    load1(A1, 0);
    __syncthreads();
  }
  // the incident flux toa = toa_src * tsi / def_tsi (rrtmgp_rfmip_sw.F90:403-418), def_tsi the source summed in g order
  // by every lane (broadcast LDS reads; no barrier); or the caller's
  auto bc_toa = [&]() -> V {
    float s = 0.0f;
    int i = 0;
    for (; i + 8 <= ngpt; i += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = bsrc[i + j];
#pragma unroll
      for (int j = 0; j < 8; j++) s = s + v[j];
    }
    for (; i < ngpt; i++) s = s + bsrc[i];
    const float t = bc.tsi[icol];
    if constexpr (NPL == 2) return on ? (V){bsrc[gc] * t / s, bsrc[gc + 1] * t / s} : (V)0.0f;
    else return on ? (V)(bsrc[gc] * t / s) : (V)0.0f;
  };
  const V Ftop = (bcf ? bc_toa() : ld_col(inc_flux)) * mu0;

  // one chunk's optical properties (the band increment is formed as they are used, as inc_2str2 does), with the
  // checkpoints the pass reads for it: fb the beam at the chunk's top (pass 2), ae / se the albedo and source at its
  // bottom (pass 3)
  struct Chunk {
    L t[K], w[K], g[K], qt[K], qw[K], qg[K];
    V tn[K], em[K], fb, ae, se;
    uint32_t qm[kMask ? K : 1];
    L at[kAer ? K : 1], aw[kAer ? K : 1], ag[kAer ? K : 1];
  };
  // pass: 2 or 3 (a constant: it selects the streams' cache policies).  Pass 3's loads are all last uses; pass 2's are
  // the beam checkpoint's and, when pass 3 reads exp(-k tau) from its plane and so no tau, tau's
  auto load_chunk = [&](Chunk &ch, int ck, auto pass_c) {
    constexpr int pass = decltype(pass_c)::value;
    constexpr CachePolicy cpT = pass == 3 ? kCp.p3_ld : (kEmk ? kCp.p2_last : CachePolicy::kDefault);
    constexpr CachePolicy cp3 = pass == 3 ? kCp.p3_ld : CachePolicy::kDefault;
#pragma unroll
    for (int p = 0; p < K; p++) {
      const int l = lay(ck * K + p);
      const uint32_t s = row * (uint32_t)l;
      ch.t[p] = ck_ld<kDual, cpT>(Ttau, vL, s);
      ch.tn[p] = kTn ? CT.template ldv<cp3>(vLp, rowW * (uint32_t)l) : (V)0.0f;
      ch.em[p] = (kEmk && pass == 3) ? CE.template ldv<cp3>(vLp, rowW * (uint32_t)l) : (V)0.0f;
      ch.w[p] = ck_ld<kDual, cp3>(Tssa, vL, s);
      ch.g[p] = kHasG ? ck_ld<kDual, cp3>(Tg, vL, s) : (L)0.0f;
      if constexpr (kInc) {
        ch.qt[p] = ld_bnd(Bt, l);
        ch.qw[p] = ld_bnd(Bw, l);
        ch.qg[p] = ld_bnd(Bg, l);
        if constexpr (kMask) ch.qm[p] = ld_msk(l);
        if constexpr (kAer) {
          ch.at[p] = ld_bnd(At, l);
          ch.aw[p] = ld_bnd(Aw, l);
          ch.ag[p] = ld_bnd(Ag, l);
        }
      } else {
        ch.qt[p] = ch.qw[p] = ch.qg[p] = (L)0.0f;
      }
    }
    if constexpr (pass == 2) {
      ch.fb = CW.template ldv<kCp.p2_last>(vW, rowW * (uint32_t)ck);
    } else {
      const uint32_t sE = rowW * (uint32_t)min(ck + 1, nck);
      ch.ae = CW.template ldv<cp3>(vW, sA0 + sE);
      ch.se = CW.template ldv<cp3>(vW, sS0 + sE);
    }
  };
  // the (incremented) properties of layer p of a chunk
  auto props = [&](const Chunk &ch, int p, V &t, V &w, V &g0) {
    if constexpr (kDual) {
      // .y: the gases (and the aerosol) alone; .x: those values, then the (selected) cloud
      float ty = ch.t[p], wy = ch.w[p], gy = kHasG ? ch.g[p] : 0.0f;
      if constexpr (kAer) ck_inc(ty, wy, gy, ch.at[p], ch.aw[p], ch.ag[p]);
      float tx = ty, wx = wy, gx = gy;
      ck_inc(tx, wx, gx, sel(ch.qt[p], ch.qm[kMask ? p : 0]), sel(ch.qw[p], ch.qm[kMask ? p : 0]),
             sel(ch.qg[p], ch.qm[kMask ? p : 0]));
      t = (V){tx, ty};
      w = (V){wx, wy};
      g0 = (V){gx, gy};
    } else {
      t = ch.t[p];
      w = ch.w[p];
      g0 = kHasG ? ch.g[p] : (V)0.0f;
      if constexpr (kAer) ck_inc(t, w, g0, ch.at[p], ch.aw[p], ch.ag[p]);
      if constexpr (kMask) ck_inc(t, w, g0, sel(ch.qt[p], ch.qm[p]), sel(ch.qw[p], ch.qm[p]), sel(ch.qg[p], ch.qm[p]));
      else if constexpr (kInc) ck_inc(t, w, g0, ch.qt[p], ch.qw[p], ch.qg[p]);
    }
  };
  // Each pass walks its chunks two at a time through two register buffers: the loads of the next chunk go to the other
  // buffer while this one is computed, so no copy waits for them at the end of the step.  body(buf, ck, valid)
  // computes chunk ck; idx(i) is the pass's i-th chunk.  With an odd count the last step's second body runs on the
  // last chunk again with valid = false (no state change, no stores), so that no branch separates a prefetch from its
  // use (the compiler sinks loads past such a branch).  No scheduling fences between the loads and the bodies: the
  // scheduler may then start a chunk's independent coefficient algebra under the previous chunk's recurrence (round
  // 4: C3 SW solver -0.6 to -2.5 %, C4 -1.1 %, tools/kernel_ab.py).
  auto walk = [&](auto &&load, auto &&body, int count, auto &&idx, auto &A, auto &B, bool preloaded = false) {
    if (!preloaded) load(A, idx(0));
    for (int i = 0; i < count; i += 2) {
      load(B, idx(min(i + 1, count - 1)));
      body(A, idx(i), true);
      load(A, idx(min(i + 2, count - 1)));
      body(B, idx(min(i + 1, count - 1)), i + 1 < count);
    }
  };
  // the same walk two chunks ahead through three buffers (same bodies in the same order: same bits)
  auto walk3 = [&](auto &&load, auto &&body, int count, auto &&idx, auto &A, auto &B, auto &C) {
    load(A, idx(0));
    load(B, idx(min(1, count - 1)));
    for (int i = 0; i < count; i += 3) {
      load(C, idx(min(i + 2, count - 1)));
      body(A, idx(i), true);
      load(A, idx(min(i + 3, count - 1)));
      body(B, idx(min(i + 1, count - 1)), i + 1 < count);
      load(B, idx(min(i + 4, count - 1)));
      body(C, idx(min(i + 2, count - 1)), i + 2 < count);
    }
  };

  // ---- pass 1: direct beam, checkpoint at every chunk top (steps of P1 layers, A1 / B1 / load1 above) ----
  V Fd = Ftop;
  {
    const int np1 = (nlay + P1 - 1) / P1;
    auto body1 = [&](Buf1 &b, int c1, bool valid) {
      const int n = valid ? min(P1, nlay - c1 * P1) : 0;
      V arg[P1], Tn[P1];
#pragma unroll
      for (int p = 0; p < P1; p++) {
        if constexpr (kDual) arg[p] = -(V){b.t[p] + b.q[p], b.t[p]} * mu0_inv;
        else arg[p] = -b.t[p] * mu0_inv;
      }
      exp_beam_batch(arg, Tn, etab);
      if constexpr (kTn) {
#pragma unroll
        for (int p = 0; p < P1; p++)
          CT.template stv<kCp.p1_st>(Tn[p], (on && p < n) ? vLp : kBufOOB, rowW * (uint32_t)lay(c1 * P1 + p));
      }
#pragma unroll
      for (int p = 0; p < P1; p++) {
        if (p % K == 0) CW.template stv<kCp.p1_st>(Fd, (p < n) ? vWs : kBufOOB, rowW * (uint32_t)(c1 * P1C + p / K));
        Fd = (p < n) ? Tn[p] * Fd : Fd;
      }
    };
    walk(load1, body1, np1, [](int i) { return i; }, A1, B1, kEarly);
  }
  // ---- pass 2: bottom -> top adding; albedo / source checkpoint at every chunk top and at the surface ----
  V alb_b = bcf ? alb_bc : ld_col(alb_dif);
  V src_b = Fd * (bcf ? alb_bc : ld_col(alb_dir));
  CW.template stv<kCp.p2_st>(alb_b, vWs, sA0 + rowW * (uint32_t)nck);
  CW.template stv<kCp.p2_st>(src_b, vWs, sS0 + rowW * (uint32_t)nck);
  {
    Chunk A, B;
    auto load2 = [&](Chunk &ch, int ck) { load_chunk(ch, ck, std::integral_constant<int, 2>{}); };
    auto body2 = [&](Chunk &cur, int ck, bool valid) {
      const int n = valid ? min(K, nlay - ck * K) : 0;
      V t[K], w[K], g0[K], Tn[K], Fin[K];
      V Fb = cur.fb;
#pragma unroll
      for (int p = 0; p < K; p++) props(cur, p, t[p], w[p], g0[p]);
      if constexpr (kTn) {
#pragma unroll
        for (int p = 0; p < K; p++) Tn[p] = cur.tn[p];  // pass 1's transmittances
      } else {
        V arg[K];
#pragma unroll
        for (int p = 0; p < K; p++) arg[p] = -t[p] * mu0_inv;
        exp_beam_batch(arg, Tn, etab);  // pass 1's expressions, same bits
      }
#pragma unroll
      for (int p = 0; p < K; p++) {
        Fin[p] = Fb;  // the beam at the layer's top
        Fb = Tn[p] * Fb;
      }
      // the chunk's coefficients (layers past nlay in the last chunk see the clamped last layer and are not used),
      // then the adding recurrence
      Coef2<V> cf[K];
      V em[K];
      ck_two_stream_k<kG0, K, V, kEmk ? 1 : 0>(t, w, g0, mu0, Tn, Fin, cf, etab, em);
      if constexpr (kEmk) {
#pragma unroll
        for (int p = 0; p < K; p++)
          CE.template stv<kCp.p2_st>(em[p], (on && p < n) ? vLp : kBufOOB, rowW * (uint32_t)lay(ck * K + p));
      }
#pragma unroll
      for (int p = K - 1; p >= 0; p--) {
        const V denom = rcp2(1.0f - cf[p].Rdif * alb_b);
        const V alb = cf[p].Rdif + cf[p].Tdif * cf[p].Tdif * alb_b * denom;
        const V src = cf[p].Sup + cf[p].Tdif * denom * (src_b + alb_b * cf[p].Sdn);
        alb_b = (p < n) ? alb : alb_b;
        src_b = (p < n) ? src : src_b;
      }
      CW.template stv<kCp.p2_st>(alb_b, valid && ck > 0 ? vWs : kBufOOB, sA0 + rowW * (uint32_t)ck);
      CW.template stv<kCp.p2_st>(src_b, valid && ck > 0 ? vWs : kBufOOB, sS0 + rowW * (uint32_t)ck);
    };
    if constexpr (AHEAD == 2) {
      Chunk C;
      walk3(load2, body2, nck, [&](int i) { return nck - 1 - i; }, A, B, C);
    } else {
      walk(load2, body2, nck, [&](int i) { return nck - 1 - i; }, A, B);
    }
  }
  // ---- pass 3: top -> bottom fluxes + ordered broadband sums ----
  // idle lanes (past the block's columns) store their ring values to one spare slot instead of branching around the
  // stores; slots past the last level (the last chunk's padding layers) are written and never read
  float *const spare = smem + kExpTabFloats + (size_t)ncr * 3 * R * rs;
  // level `lev` (array index) of the g-point outputs
  auto put = [&](V up, V dif, V dir, int r, int lev, bool valid) {
    const V dn = kGpt ? dif + dir : dif;  // kGpt: the total, rounded once ("flux_dn is total", :665-666)
    if constexpr (kDual) {
      // sky s of g-point g in ring s (idle lanes: the spare slot's two floats)
      const size_t o2 = on ? (size_t)3 * R * rs : 1;
      float *const pu = on ? &ring[(size_t)r * rs + g] : spare;
      float *const pd = on ? &ring[((size_t)R + r) * rs + g] : spare;
      float *const pr = on ? &ring[((size_t)2 * R + r) * rs + g] : spare;
      pu[0] = up.x, pu[o2] = up.y;
      pd[0] = dn.x, pd[o2] = dn.y;
      pr[0] = dir.x, pr[o2] = dir.y;
    } else {
      *(V *)(on ? &ring[(size_t)r * rs + g] : spare) = up;
      *(V *)(on ? &ring[((size_t)R + r) * rs + g] : spare) = dn;
      *(V *)(on ? &ring[((size_t)2 * R + r) * rs + g] : spare) = dir;
    }
    if constexpr (kGpt) {
      if (on && valid) {
        const size_t o = (size_t)g + (size_t)ngpt * ((size_t)lev + (size_t)nlev * icol);
        *(V *)&gpt_up[o] = up;
        *(V *)&gpt_dn[o] = dn;
        *(V *)&gpt_dir[o] = dir;
      }
    }
  };
  auto flush = [&](int n, int lev0, int dl, int slot0 = 0, bool sfc = false) {
    // kBand: the by-band sums bo.up / bo.dn / bo.dir in the same barrier window; the ring keeps diffuse and direct
    // apart (the broadband bits do not move) and the band walk forms dif + dir itself (band_flush)
    // kSfcBand (rrtmgpnn_solver_request_sfc_byband): the same walk over the surface level alone, the last of the
    // levels of pass 3's last flush (sfc), into bo's (nbnd, ncol) arrays
    const BandOut *pb = (kBand || kSfcBand) ? &bo : nullptr;
    const int sfc_slot = (kSfcBand && sfc) ? slot0 + n - 1 : -1;
    if (kCkFlushLanes && (ngpt & 3) == 0 && 3 * ncr * n * 4 <= (int)blockDim.x)
      ring_flush_sw_lanes<R, kGpt, kBand, kDual, kSfcBand>(smem + kExpTabFloats, ncr, n, lev0, dl, ngpt, nlev, icol0,
                                                           nca, flux_up, flux_dn, flux_dir, rs, slot0, pb, clr_up,
                                                           clr_dn, clr_dir, sfc_slot);
    else
      ring_flush_sw<R, kGpt, kBand, kDual, kSfcBand>(smem + kExpTabFloats, ncr, n, lev0, dl, ngpt, nlev, icol0, nca,
                                                     flux_up, flux_dn, flux_dir, rs, slot0, pb, clr_up, clr_dn, clr_dir,
                                                     sfc_slot);
  };
  // the ring holds M = R / K chunks; the block flushes it when it is full (a barrier, the ordered sums, a barrier).
  // (Staggering the blocks' flush phases, so that blocks sharing a CU flush at different chunks, measured equal, round
  // 4: the flush's cost is its own latency inside each block, not the whole chip flushing at once.)
  constexpr int M = R / K;
  V Fdn = inc_dif ? ld_col(inc_dif) : (V)0.0f;
  if (bcf) __syncthreads();  // every lane has read the staged solar source before the ring is written
  put(Fdn * alb_b + src_b, Fdn, Ftop, 0, top, true);
  flush(1, top, 1);
  {
    Chunk A, B;
    V Fd3 = Ftop;
    auto load3 = [&](Chunk &ch, int ck) { load_chunk(ch, ck, std::integral_constant<int, 3>{}); };
    auto body3 = [&](Chunk &cur, int ck, bool valid) {
      const int n = valid ? min(K, nlay - ck * K) : 0;
      // the chunk's coefficients, top down, the beam carried as pass 1 carries it
      V t[K], w[K], g0[K], Tn[K], Fin[K], Fdir[K];
#pragma unroll
      for (int p = 0; p < K; p++) props(cur, p, t[p], w[p], g0[p]);
      if constexpr (kTn) {
#pragma unroll
        for (int p = 0; p < K; p++) Tn[p] = cur.tn[p];
      } else {
        V arg[K];
#pragma unroll
        for (int p = 0; p < K; p++) arg[p] = -t[p] * mu0_inv;
        exp_beam_batch(arg, Tn, etab);
      }
#pragma unroll
      for (int p = 0; p < K; p++) {
        Fin[p] = Fd3;
        Fd3 = (p < n) ? Tn[p] * Fd3 : Fd3;
        Fdir[p] = Fd3;  // the beam at the layer's bottom
      }
      Coef2<V> cf[K];
      ck_two_stream_k<kG0, K, V, kEmk ? 2 : 0>(t, w, g0, mu0, Tn, Fin, cf, etab, cur.em);
      // albedo / source at levels ck*K + p + 1 (A[p], S[p]), walked up from the checkpoint with pass 2's expressions;
      // D[p] = 1 / (1 - R_dif(p) * A[p]) is the adding denominator both walks use
      V Al[K], S[K], D[K];
      {
        V a = cur.ae, s = cur.se;
#pragma unroll
        for (int p = K - 1; p >= 0; p--) {
          Al[p] = a;
          S[p] = s;
          const V denom = rcp2(1.0f - cf[p].Rdif * a);
          D[p] = denom;
          if (p > 0) {
            const V an = cf[p].Rdif + cf[p].Tdif * cf[p].Tdif * a * denom;
            const V sn = cf[p].Sup + cf[p].Tdif * denom * (s + a * cf[p].Sdn);
            a = (p < n) ? an : a;
            s = (p < n) ? sn : s;
          }
        }
      }
      // fluxes down the chunk (adding :1583-1591, Eqs 12-13)
      const int rbase = (ck % M) * K;
#pragma unroll
      for (int p = 0; p < K; p++) {
        const V fdn = (cf[p].Tdif * Fdn + cf[p].Rdif * S[p] + cf[p].Sdn) * D[p];
        Fdn = (p < n) ? fdn : Fdn;
        put(fdn * Al[p] + S[p], fdn, Fdir[p], rbase + p, top + dl_dn * (ck * K + p + 1), p < n);
      }
      if (valid && (rbase + K == R || ck == nck - 1)) {
        const int j0 = ck * K - rbase;  // first layer of this ring's levels
        flush(min(R, nlay - j0), top + dl_dn * (j0 + 1), dl_dn, 0, ck == nck - 1);  // pass 3 ends at the surface
      }
    };
    if constexpr (AHEAD == 2) {
      Chunk C;
      walk3(load3, body3, nck, [](int i) { return i; }, A, B, C);
    } else {
      walk(load3, body3, nck, [](int i) { return i; }, A, B);
    }
  }
}

bool sw_ck_small(const rrtmgpnn_context *ctx, int ngpt, int ncol, bool has_g, bool inc, bool gpt)
{
  // 2 g-points per lane; one round of 16 waves of 64 lanes per CU
  return !has_g && !inc && !gpt && (long long)ncol * (ngpt / 2) <= 64LL * 16 * ctx->num_cus;
}

// workspace floats of the checkpointed kernel (sized for the smaller of the chunk lengths, so it holds either
// instance) plus the planes of the instance that runs: small-grid clear sky, large-grid clear sky (NN: g = NULL, no
// increment, no g-point outputs) or all sky (inc)
// dual: the clear + all-sky instances' checkpoints and planes, a pair per g-point each
size_t sw_2stream_ck_ws_floats(int ngpt, int nlay, int ncol, bool small, bool inc, bool nn, bool planes, bool dual)
{
  if (dual)
    return 2 * sw_2stream_ck_ws_floats(ngpt, nlay, ncol, false, true, false, false, false) +
           (planes ? (size_t)2 * ((int)kCkTnDual + (int)kCkEmkDual) * ngpt * nlay * ncol : 0);
  const int np = small  ? (int)kCkTnSmall + (int)kCkEmkSmall
                 : !planes ? 0
                 : nn     ? (int)kCkTnNN + (int)kCkEmkNN
                 : inc    ? (int)kCkTnInc + (int)kCkEmkInc
                          : 0;
  const size_t tn = (size_t)np * ngpt * nlay * ncol;
  const int k = std::min(kCkK, kCkKSmall);
  const size_t nck = (size_t)(nlay + k - 1) / k;
  return (size_t)ngpt * ncol * (nck + 2 * (nck + 1)) + tn;
}

// The instances sw_2stream_ck_kernel is compiled for, family by family (select_sw_ck below names the calls they serve)
using SwCkInstances = SolverInstances<
    // clear + all sky from one launch: {gas g} x {mask} x {aerosol}, with the dual family's planes and without
    kSwCkDual | kSwCkInc | kSwCkPlanesDual, kSwCkDual | kSwCkInc | kSwCkPlanesDual | kSwCkHasG,
    kSwCkDual | kSwCkInc | kSwCkPlanesDual | kSwCkMask, kSwCkDual | kSwCkInc | kSwCkPlanesDual | kSwCkMask | kSwCkHasG,
    kSwCkDual | kSwCkInc | kSwCkPlanesDual | kSwCkAer, kSwCkDual | kSwCkInc | kSwCkPlanesDual | kSwCkAer | kSwCkHasG,
    kSwCkDual | kSwCkInc | kSwCkPlanesDual | kSwCkMask | kSwCkAer,
    kSwCkDual | kSwCkInc | kSwCkPlanesDual | kSwCkMask | kSwCkAer | kSwCkHasG,
    kSwCkDual | kSwCkInc, kSwCkDual | kSwCkInc | kSwCkHasG, kSwCkDual | kSwCkInc | kSwCkMask,
    kSwCkDual | kSwCkInc | kSwCkMask | kSwCkHasG, kSwCkDual | kSwCkInc | kSwCkAer,
    kSwCkDual | kSwCkInc | kSwCkAer | kSwCkHasG, kSwCkDual | kSwCkInc | kSwCkMask | kSwCkAer,
    kSwCkDual | kSwCkInc | kSwCkMask | kSwCkAer | kSwCkHasG,
    // aerosol + (masked) cloud, band pair: {gas g} x {mask}, with the all-sky planes and without
    kSwCkAer | kSwCkInc | kSwCkBandPair | kSwCkPlanesInc, kSwCkAer | kSwCkInc | kSwCkBandPair | kSwCkPlanesInc | kSwCkHasG,
    kSwCkAer | kSwCkInc | kSwCkBandPair | kSwCkPlanesInc | kSwCkMask,
    kSwCkAer | kSwCkInc | kSwCkBandPair | kSwCkPlanesInc | kSwCkMask | kSwCkHasG,
    kSwCkAer | kSwCkInc | kSwCkBandPair, kSwCkAer | kSwCkInc | kSwCkBandPair | kSwCkHasG,
    kSwCkAer | kSwCkInc | kSwCkBandPair | kSwCkMask, kSwCkAer | kSwCkInc | kSwCkBandPair | kSwCkMask | kSwCkHasG,
    // masked cloud: {gas g} x {band pair}, by band (no planes), with the all-sky planes and without
    kSwCkMask | kSwCkInc | kSwCkBand, kSwCkMask | kSwCkInc | kSwCkBand | kSwCkHasG,
    kSwCkMask | kSwCkInc | kSwCkBand | kSwCkBandPair, kSwCkMask | kSwCkInc | kSwCkBand | kSwCkBandPair | kSwCkHasG,
    kSwCkMask | kSwCkInc | kSwCkPlanesInc, kSwCkMask | kSwCkInc | kSwCkPlanesInc | kSwCkHasG,
    kSwCkMask | kSwCkInc | kSwCkPlanesInc | kSwCkBandPair, kSwCkMask | kSwCkInc | kSwCkPlanesInc | kSwCkBandPair | kSwCkHasG,
    kSwCkMask | kSwCkInc, kSwCkMask | kSwCkInc | kSwCkHasG, kSwCkMask | kSwCkInc | kSwCkBandPair,
    kSwCkMask | kSwCkInc | kSwCkBandPair | kSwCkHasG,
    // g-point outputs
    kSwCkGpt, kSwCkGpt | kSwCkHasG,
    // by band: the small-grid instance, the increment ({gas g} x {band pair}) and the clear sky, all without planes
    kSwCkBand | kSwCkSmall | kSwCkPlanesSmall, kSwCkBand | kSwCkInc, kSwCkBand | kSwCkInc | kSwCkHasG,
    kSwCkBand | kSwCkInc | kSwCkBandPair, kSwCkBand | kSwCkInc | kSwCkBandPair | kSwCkHasG, kSwCkBand,
    kSwCkBand | kSwCkHasG,
    // the increment: {gas g} x {band pair}, with the all-sky planes and without
    kSwCkInc | kSwCkPlanesInc, kSwCkInc | kSwCkPlanesInc | kSwCkHasG, kSwCkInc | kSwCkPlanesInc | kSwCkBandPair,
    kSwCkInc | kSwCkPlanesInc | kSwCkBandPair | kSwCkHasG, kSwCkInc, kSwCkInc | kSwCkHasG, kSwCkInc | kSwCkBandPair,
    kSwCkInc | kSwCkBandPair | kSwCkHasG,
    // clear sky: with a gas g; the small-grid instance; the large-grid NN instance with its planes and without
    kSwCkHasG, kSwCkSmall | kSwCkPlanesSmall, kSwCkPlanesNN, 0u>;

// ... and with the active-column count read from a device word (rrtmgpnn_solver_request_active_columns), a family of
// its own (kSolverSwCkActive): what a step on compacted daylit columns selects and no more -- the small-grid clear-sky
// instance, the large-grid NN instance with its planes and without, and the fused increment ({band pair} x {the all-sky
// plane}); no gas g
using SwCkActiveInstances = SolverInstances<
    kSwCkActive | kSwCkSmall | kSwCkPlanesSmall, kSwCkActive | kSwCkPlanesNN, kSwCkActive,
    kSwCkActive | kSwCkInc | kSwCkBandPair | kSwCkPlanesInc, kSwCkActive | kSwCkInc | kSwCkBandPair,
    kSwCkActive | kSwCkInc | kSwCkPlanesInc, kSwCkActive | kSwCkInc>;

// ... and the count beside a cloud mask and / or an aerosol (kSolverSwCkActiveSky): what a McICA step on compacted daylit
// columns selects -- the masked cloud ({band pair} x {the all-sky plane}), the aerosol in front of it and the aerosol in
// front of an unmasked cloud (band pair, with the plane and without); no gas g.  The mask's and the aerosol's rows are
// those of the dense columns (extents of the launch-time ncol)
using SwCkActiveSkyInstances = SolverInstances<
    kSwCkActive | kSwCkInc | kSwCkMask | kSwCkBandPair | kSwCkPlanesInc, kSwCkActive | kSwCkInc | kSwCkMask | kSwCkBandPair,
    kSwCkActive | kSwCkInc | kSwCkMask | kSwCkPlanesInc, kSwCkActive | kSwCkInc | kSwCkMask,
    kSwCkActive | kSwCkInc | kSwCkMask | kSwCkAer | kSwCkBandPair | kSwCkPlanesInc,
    kSwCkActive | kSwCkInc | kSwCkMask | kSwCkAer | kSwCkBandPair,
    kSwCkActive | kSwCkInc | kSwCkAer | kSwCkBandPair | kSwCkPlanesInc, kSwCkActive | kSwCkInc | kSwCkAer | kSwCkBandPair>;

// ... and the by-band sums of the surface level (rrtmgpnn_solver_request_sfc_byband, kSolverSwCkSfcBand): each instance
// is its twin of the first family (aerosol / masked cloud, band pair, no gas g) or of kSolverSwCkActiveSky plus the bit,
// {the count} x {mask, mask + aerosol, aerosol} x {the all-sky plane}
using SwCkSfcBandInstances = SolverInstances<
    kSwCkSfcBand | kSwCkInc | kSwCkMask | kSwCkBandPair | kSwCkPlanesInc, kSwCkSfcBand | kSwCkInc | kSwCkMask | kSwCkBandPair,
    kSwCkSfcBand | kSwCkInc | kSwCkMask | kSwCkAer | kSwCkBandPair | kSwCkPlanesInc,
    kSwCkSfcBand | kSwCkInc | kSwCkMask | kSwCkAer | kSwCkBandPair,
    kSwCkSfcBand | kSwCkInc | kSwCkAer | kSwCkBandPair | kSwCkPlanesInc, kSwCkSfcBand | kSwCkInc | kSwCkAer | kSwCkBandPair,
    kSwCkSfcBand | kSwCkActive | kSwCkInc | kSwCkMask | kSwCkBandPair | kSwCkPlanesInc,
    kSwCkSfcBand | kSwCkActive | kSwCkInc | kSwCkMask | kSwCkBandPair,
    kSwCkSfcBand | kSwCkActive | kSwCkInc | kSwCkMask | kSwCkAer | kSwCkBandPair | kSwCkPlanesInc,
    kSwCkSfcBand | kSwCkActive | kSwCkInc | kSwCkMask | kSwCkAer | kSwCkBandPair,
    kSwCkSfcBand | kSwCkActive | kSwCkInc | kSwCkAer | kSwCkBandPair | kSwCkPlanesInc,
    kSwCkSfcBand | kSwCkActive | kSwCkInc | kSwCkAer | kSwCkBandPair>;

// The instance a call runs (its options value), or the refusal.  planes: the workspace with the instance family's
// planes was allocated (launch_sw_2stream's fallback runs the plane-free twins: the same bits); small: sw_ck_small()
static int select_sw_ck(const SolverExtras &ex, const Sw2Stream &p, bool planes, bool small, uint32_t *options)
{
  const BandArgs *const bands = p.bands;
  const bool bb = ex.byband(), gpt = ex.gpt_up || ex.gpt_dn || ex.gpt_dir;
  // kBandPair: every band of the increment starts at an even (0-based) g-point
  bool pair = bands != nullptr;
  for (int i = 0; bands && i < bands->nbnd; i++) pair = pair && ((bands->lims[2 * i] - 1) % 2 == 0);
  uint32_t o = (p.g ? kSwCkHasG : 0u) | (bands ? kSwCkInc : 0u) | (ex.mask_bits ? kSwCkMask : 0u);
  if (ex.sfc_byband()) {
    // the surface level's by-band sums: the twin's rules (the branches below) hold, and on top of them no gas g, the
    // band-pair layout (also for a masked cloud alone) and the request's bands the increment's own
    if (ex.clr_up || bb || gpt)
      return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: surface by-band outputs with clear-sky twins, by-band or g-point "
                                            "outputs");
    if (!ex.mask_bits && !ex.aer_tau)
      return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: surface by-band outputs need a cloud mask or an aerosol increment");
    if (p.g) return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: surface by-band outputs with a gas g array (g == NULL: the NN path)");
    if (!bands) return fail(RRTMGPNN_ERR_ARGUMENT, "sw solver: surface by-band outputs need the fused band increment");
    if (!pair)
      return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: surface by-band outputs need every band to start at an odd "
                                            "(1-based) g-point, the band-pair layout");
    bool same = ex.sfc_bnd.nbnd == bands->nbnd;
    for (int i = 0; same && i < 2 * bands->nbnd; i++) same = ex.sfc_bnd.lims[i] == bands->lims[i];
    if (!same)
      return fail(RRTMGPNN_ERR_ARGUMENT, "sw solver: the requested surface by-band outputs' bands are not this call's "
                                         "increment bands");
    o |= kSwCkSfcBand;
  }
  if (ex.nact) {
    // the daylit columns of a compacted block: the instance the same call would run without the count (chosen from the
    // launch-time ncol: the host never sees the count), from the family's own list
    if (ex.clr_up || bb || gpt)
      return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: an active-column count with clear-sky twins, by-band or g-point "
                                            "outputs");
    if (p.g)
      return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: an active-column count with a gas g array (g == NULL: the NN path)");
    if (ex.aer_tau) {
      // kSolverSwCkActiveSky: the rules of the aerosol branch below, then those of the mask branch
      if (!bands) return fail(RRTMGPNN_ERR_ARGUMENT, "sw solver: an aerosol increment needs the fused band increment behind it");
      if (!ex.aer_ssa || !ex.aer_g)
        return fail(RRTMGPNN_ERR_ARGUMENT, "sw solver: a shortwave entry takes a 2str aerosol (ssa_aer and g_aer set)");
      if (!pair)
        return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: an aerosol increment needs every band to start at an odd "
                                              "(1-based) g-point, the band-pair layout");
      o |= kSwCkActive | kSwCkAer | kSwCkBandPair | (planes ? kSwCkPlanesInc : 0u);
    } else if (ex.mask_bits) {
      if (!bands) return fail(RRTMGPNN_ERR_ARGUMENT, "sw solver: a cloud mask needs the fused band increment");
      o |= kSwCkActive | (pair ? kSwCkBandPair : 0u) | (planes ? kSwCkPlanesInc : 0u);
    } else {
      o |= kSwCkActive | (bands ? (pair ? kSwCkBandPair : 0u) | (planes ? kSwCkPlanesInc : 0u)
                                : (small ? kSwCkSmall | kSwCkPlanesSmall : (planes ? kSwCkPlanesNN : 0u)));
    }
  } else if (ex.clr_up) {
    // clear-sky beside all-sky fluxes (rrtmgpnn_sw_solver_2stream_clr_all): the dual instances, one column per block,
    // one g-point per lane, two rings; {gas g} x {mask} x {aerosol}, with the planes of kCkTnDual / kCkEmkDual or, when
    // that workspace did not fit, without
    if (!bands || !ex.clr_dn || !ex.clr_dir)
      return fail(RRTMGPNN_ERR_ARGUMENT, "sw solver: the clear + all-sky instances need the fused band increment and "
                                         "all three clear-sky outputs");
    if (bb || gpt)
      return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: clear + all-sky fluxes with by-band or g-point outputs");
    if (ex.aer_tau && (!ex.aer_ssa || !ex.aer_g))
      return fail(RRTMGPNN_ERR_ARGUMENT, "sw solver: a shortwave entry takes a 2str aerosol (ssa_aer and g_aer set)");
    o |= kSwCkDual | (ex.aer_tau ? kSwCkAer : 0u) | (planes ? kSwCkPlanesDual : 0u);
  } else if (ex.aer_tau) {
    // aerosols in front of the (masked) cloud increment (rrtmgpnn_solver_request_aerosol): the band-pair layout only,
    // with the all-sky instances' transmittance plane or, when that workspace did not fit, without it (the same bits)
    if (!bands) return fail(RRTMGPNN_ERR_ARGUMENT, "sw solver: an aerosol increment needs the fused band increment behind it");
    if (!ex.aer_ssa || !ex.aer_g)
      return fail(RRTMGPNN_ERR_ARGUMENT, "sw solver: a shortwave entry takes a 2str aerosol (ssa_aer and g_aer set)");
    // (as in launch_lw_impl: not reachable through the C ABI as it stands -- the two entries have no g-point arguments
    // and refuse a by-band request beside the aerosol themselves, and launch_sw_2stream checks both again)
    if (bb || gpt)
      return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: an aerosol increment with by-band or g-point outputs");
    if (!pair)
      return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: an aerosol increment needs every band to start at an odd "
                                            "(1-based) g-point, the band-pair layout");
    o |= kSwCkAer | kSwCkBandPair | (planes ? kSwCkPlanesInc : 0u);
  } else if (ex.mask_bits) {
    // McICA: the masked twins of the fused increment (rrtmgpnn_solver_request_cloud_mask); by band
    // (rrtmgpnn_solver_request_byband_mcica) without workspace planes, as the unmasked by-band instances
    if (!bands) return fail(RRTMGPNN_ERR_ARGUMENT, "sw solver: a cloud mask needs the fused band increment");
    if (gpt) return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: a cloud mask with g-point outputs");
    o |= (pair ? kSwCkBandPair : 0u) | (bb ? kSwCkBand : (planes ? kSwCkPlanesInc : 0u));
  } else if (gpt) {  // ty_fluxes_flexible g-point outputs: all three (launch_sw_2stream)
    if (bands) return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: g-point outputs with a fused increment");
    o |= kSwCkGpt;
  } else if (bb) {
    // by-band instances: the small-grid clear-sky instance where it applies (as without the request), else the
    // large-grid forms without workspace planes (the same bits as the others)
    o |= kSwCkBand | (small ? kSwCkSmall | kSwCkPlanesSmall : 0u) | (pair ? kSwCkBandPair : 0u);
  } else if (bands) {
    o |= (pair ? kSwCkBandPair : 0u) | (planes ? kSwCkPlanesInc : 0u);
  } else if (!p.g) {
    // the small-grid instance when the clear-sky grid fits in one round of resident waves, else the NN instance
    o |= small ? kSwCkSmall | kSwCkPlanesSmall : (planes ? kSwCkPlanesNN : 0u);
  }
  *options = o;
  return RRTMGPNN_OK;
}

// ngpt even and <= 256
int launch_sw_2stream_ck(rrtmgpnn_context *ctx, const SolverExtras &ex, const Sw2Stream &p, void *ws, bool planes,
                         const SwBcDev *bc)
{
  const int ngpt = p.ngpt, nlay = p.nlay, ncol = p.ncol;
  const BandArgs nob{};
  const BandArgs &b = p.bands ? *p.bands : nob;
  const SwBcDev nobc{};  // tsi == NULL: the caller's inc_flux, mu0 and albedos
  const SwBcDev &bcd = bc ? *bc : nobc;
  const bool gpt = ex.gpt_up || ex.gpt_dn || ex.gpt_dir;
  const BandOut bo = ex.byband()       ? band_out(ex)
                     : ex.sfc_byband() ? BandOut{ex.sfc_bnd_up, ex.sfc_bnd_dn, ex.sfc_bnd_dir, ex.sfc_bnd}
                                       : BandOut{};
  uint32_t options = 0;
  if (int rc = select_sw_ck(ex, p, planes, sw_ck_small(ctx, ngpt, ncol, p.g != nullptr, p.bands != nullptr, gpt), &options))
    return rc;
  auto go = [&](auto oc) -> int {
    constexpr uint32_t O = decltype(oc)::value;
    constexpr bool kDual = (O & kSwCkDual) != 0, kInc = (O & kSwCkInc) != 0;
    constexpr int ring = (O & kSwCkSmall) ? kCkRingSmall : kCkRing;
    // npl g-points per lane, ncb columns per block (two where 512 lanes hold them); the dual instances: one g-point
    // per lane, one column per block, a ring per sky
    constexpr int npl = kDual ? 1 : ((O & kSwCkSmall) ? (int)(sizeof(VSmall) / sizeof(float)) : 2);
    const int ncb = kDual ? 1 : (npl == 2 ? (2 * (ngpt / 2) <= 512 ? 2 : 1) : columns_per_block(ngpt));
    if (ncb > kFlushLanesMaxCols)  // the flush's lane -> column map (ring_flush_sw_lanes) covers at most 4 columns
      return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: more columns per block than the ordered flush maps");
    const int threads = (ncb * (ngpt / npl) + 63) / 64 * 64;
    const dim3 grid((ncol + ncb - 1) / ncb), block(threads);
    const size_t lds =
        sizeof(float) * (kExpTabFloats + (size_t)(kDual ? 2 : ncb) * 3 * ring * ck_ring_stride(ngpt) + 4);  // + spare
    if (lds > 160 * 1024) return fail(RRTMGPNN_ERR_UNSUPPORTED, "sw solver: LDS ring exceeds 160 KiB");
    const auto kern = sw_2stream_ck_kernel<O>;
    if (lds > 64 * 1024)
      if (int rc = raise_lds_limit((const void *)kern)) return rc;
    // the count word in the mask's place or, beside a mask or an aerosol, in the first clear-sky output's
    constexpr bool kCount = (O & kSwCkActive) != 0, kSky = kCount && (O & (kSwCkMask | kSwCkAer)) != 0;
    hipLaunchKernelGGL(kern, grid, block, lds, ctx->stream, ngpt, nlay, ncol, p.top_at_1, ncb, p.inc_flux,
                       p.inc_flux_dif, p.tau, p.ssa, p.g, p.mu0, p.alb_dir, p.alb_dif, b, kInc ? p.tau_bnd : nullptr,
                       kInc ? p.ssa_bnd : nullptr, kInc ? p.g_bnd : nullptr, (float *)ws, p.flux_up, p.flux_dn,
                       p.flux_dir, ex.gpt_up, ex.gpt_dn, ex.gpt_dir, bcd, bo,
                       (kCount && !kSky) ? (const uint32_t *)ex.nact : ex.mask_bits, ex.aer_tau, ex.aer_ssa, ex.aer_g,
                       kSky ? (float *)ex.nact : ex.clr_up, ex.clr_dn, ex.clr_dir);
    RRTMGPNN_LAUNCH_CHECK(kDual ? "sw_2stream_ck_kernel (clear + all sky)" : "sw_2stream_ck_kernel");
    return RRTMGPNN_OK;
  };
  if (ex.sfc_byband()) return launch_listed(ctx, kSolverSwCkSfcBand, SwCkSfcBandInstances{}, options, go);
  if (ex.nact && (ex.mask_bits || ex.aer_tau))
    return launch_listed(ctx, kSolverSwCkActiveSky, SwCkActiveSkyInstances{}, options, go);
  if (ex.nact) return launch_listed(ctx, kSolverSwCkActive, SwCkActiveInstances{}, options, go);
  return launch_listed(ctx, kSolverSwCk, SwCkInstances{}, options, go);
}

}  // namespace rrtmgpnn
