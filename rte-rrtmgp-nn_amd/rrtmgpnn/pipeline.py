"""Device-resident clear-sky LW+SW step: the hot path of BASELINE.json's metric.

One `ClearSkyStep` owns every input and output of one column block in HBM and replays
    gas_optics_int (NN)  ->  rte_lw (no-scattering)      [LW, g256]
    gas_optics_ext (NN)  ->  rte_sw (two-stream)         [SW, g224]
with the same kernels as the class-level API (api.py), but with all ctypes arguments prepared once
so the host cost per step is just the launches (or one hipGraph replay).

fused=True (default) keeps intermediates that the flux computation does not need out of HBM: the
Planck sources are formed inside the LW solver from the Planck fraction
(rrtmgpnn_lw_solver_noscat_planck: same products, same bits, compute_Planck_source_nn's arrays never
stored), and the SW asymmetry parameter -- identically zero in the NN path -- is passed as NULL
instead of being written and re-read.  fused=False issues exactly the class layer's call sequence.

What one step computes is exactly the drivers' per-block work
(examples/rfmip-clear-sky/rrtmgp_rfmip_lw.F90:399-441, rrtmgp_rfmip_sw.F90:374-451):
compute_nn_inputs, get_col_dry, both NN models per stream with post-processing, the Planck sources,
the band->g emissivity expansion, the SW boundary conditions (gas_optics_ext's incident flux
renormalised to each column's TSI, the per-g-point surface albedo and mu0 = cos(sza), formed from the
block's TSI, albedo and zenith angle, rrtmgp_rfmip_sw.F90:403-434: in the fused step inside the SW
solver, rrtmgpnn_sw_solver_2stream_rfmip; unfused rrtmgpnn_sw_boundary_rfmip), both solvers and the
broadband reductions.  The step's inputs are the driver's per-column state; the only
data prepared once are the model's (network weights, the Planck table, solar_source after set_tsi).
The unfused step computes col_dry once and shares it between LW and SW (same h2o and plev).

clouds=(lwp, iwp, rel, rei) makes it the all-sky step of examples/all-sky/rrtmgp_allsky.F90:366-446
(config C4) with NN gas optics: cloud optics by band (LUT by default, ice roughness 2 as in the example,
:219), added to the LW absorption optical depth by band (1scl increment), and for SW delta-scaled and
added as a two-stream increment; the SW solver then sees a non-zero asymmetry parameter.

mcica={...} (with clouds) samples the band clouds per g-point with McICA (extensions/cloud_optics/mo_cloud_sampling.F90)
from a cloud fraction per layer and the caller's random numbers.  Fused, each chain runs the mask kernel into a packed
mask and arms it (rrtmgpnn_solver_request_cloud_mask) for the fused solver call, which switches the band increment per
g-point; unfused, the class layer's mask -> draw_samples -> increment sequence.  With "seed" in place of the
"randoms_*" arrays the mask kernels draw the numbers themselves (Philox4x32-10, include/rrtmgpnn.h): the step then holds
no randoms arrays, only two 4-word device buffers {seed low, seed high, stream, col0} (set_mcica_seed), and a column's
clouds depend on (seed, stream, col0 + its index) alone, however the columns are split over steps.

clrsky=True (with clouds) also produces the clear-sky fluxes of the same columns, as rte_lw / rte_sw of
extensions/mo_rrtmgp_clr_all_sky.F90 do: gas optics once, a clear solve, clouds%increment, the all-sky solve.  Fused,
the LW pair comes from one call (rrtmgpnn_lw_solver_noscat_planck_clr_all) and the SW chain gets one more solver
launch on the unincremented properties; unfused, the clear solvers run before the increment_* calls.

mcica={..., "clrsky": True} is the two together: McICA all-sky fluxes and the clear-sky fluxes of the same columns
(cloud radiative effect).  Fused, the LW pair comes from rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica, which takes the
packed mask as an argument (one launch of the masked dual kernel with one angle), and the SW chain is the McICA one
plus the clear solver launch; unfused, the clear solve, then mask -> draw_samples -> increment, then the all-sky solve.

mcica={..., "byband": True}: the by-band fluxes of a byband=True step under the sampled clouds (byband_fluxes()).  Fused,
the paired request rrtmgpnn_solver_request_byband_mcica takes the place of each chain's cloud-mask request, so the
masked by-band solver instances run; unfused, rrtmgpnn_solver_request_byband ahead of each plain solver call of the
McICA sequence.  Not with "clrsky": the clear + all-sky kernel has no by-band form.

jacobian=True: the step also owns lw_up_jac (ncol, nlay+1), rte_lw's flux_up_Jac -- d flux_up / d T_sfc at every level,
for a host model that updates its LW fluxes between radiation calls -- and arms rrtmgpnn_solver_request_jacobian right
before the LW solver call, which then carries the Jacobian beside its upward radiance: fused, sfc_source_Jac is formed
in-kernel; unfused, it is the array compute_planck_source_nn already writes.  Clear-sky, overcast or McICA clouds; not
with by-band or clear-sky outputs, which have no Jacobian instances.

aerosols={"lw_tau": (ncol, nlay, nband_lw), "sw_tau": ..., "sw_ssa": ..., "sw_g": (ncol, nlay, nband_sw)}: aerosol
optical properties by band (the host's, delta-scaled by the host), which mo_rrtmgp_clr_all_sky.F90 adds to the gas
properties ahead of the clear solve (:155-157, :288-290): the clear sky is gases plus aerosols.  The step owns device
buffers of them, which set_aerosols refills between steps or replays.  Fused without clouds, the aerosol is the solver
call's own band increment (_planck_inc, _rfmip with nbnd > 0); with clouds each chain arms
rrtmgpnn_solver_request_aerosol right before its solver, which then adds the aerosol and the (sampled) cloud as it reads
the gas properties, and the clear SW launch takes the aerosol as its increment.  Unfused, rrtmgpnn_increment_bybnd by the
aerosol follows gas optics, the reference's sequence.  Not with byband, jacobian or mcica["byband"], for which the
solvers have no aerosol instances.

lw_scattering=True (with clouds, fused): the LW clouds scatter.  LW cloud optics run with three outputs (cld_tau_lw,
cld_ssa_lw, cld_g_lw by band) and the chain's all-sky solver call is rrtmgpnn_lw_solver_1rescl_planck_inc: rte_lw's
rescaled solver on the gas optical depth incremented in-kernel by the two-stream band cloud, the Planck sources formed
in-kernel.  mcica= arms the cloud mask for it as for the absorbing clouds; clrsky=True (or mcica's "clrsky") adds a
rrtmgpnn_lw_solver_noscat_planck launch for the clear set ahead of it (the rescaled solver without scattering is the
no-scattering one, bit for bit).  Not with fused=False, byband, mcica["byband"], jacobian or aerosols, for which the
entry has no instances.  Off (the default), nothing of the step changes.

upper_bc=True: the step owns lw_inc_flux (ncol, ngpt_lw), the downward LW flux at the model's top from one thin
isothermal layer between the gas optics' minimum pressure and that top (extensions/mo_compute_bc.F90), formed every
step by rrtmgpnn_compute_bc_lw (flux units, the step's nmus) at the head of the LW chain and passed as inc_flux to
whichever LW solver entry the other options select, fused or not.  The reference's pressure check runs on the host
arrays at construction and in inputs_for (ValueError with the reference's message): the unmodified RFMIP columns, whose
top level is the minimum pressure itself, are refused.  Every option set takes it; the SW chain is untouched (the _rfmip
solver forms its own incident flux).  Off (the default), nothing of the step changes.

lw_dual=True (with lw_scattering=True and clear-sky outputs): the LW chain's solver call is
rrtmgpnn_lw_solver_1rescl_planck_clr_all, which gives both flux sets, and no lw_solver_clr is issued;
rrtmgpnn_context_set_lw_scat_clr_all decides one dual launch or two.  aerosols= is then accepted beside lw_scattering:
lw_aerosol is armed right before the solver (clear sky = gases + aerosols), and set_aerosols works between replays.  Not
without lw_scattering or clear-sky outputs, nor with fused=False, byband, jacobian or mcica["byband"].

daylit=True (fused, clear sky or overcast clouds=): the SW chain runs on the block's daylit columns only, as a host model
does, in place of the RFMIP driver's mu0 = 1 solve of the night columns (rrtmgp_rfmip_sw.F90:433) -- and sw_up, sw_dn
and sw_dir of the night columns are 0, the driver's zeroing (:456-463) applied to flux_dir as well.  The chain becomes
rrtmgpnn_daylit_plan on sza; one rrtmgpnn_gather_columns of play, tlay, plev, the SW gases, sza, tsi, sfc_alb (and the
cloud fields) into step-owned dense twins of full extent; rrtmgpnn_gas_optics_sw_nn_active; cloud optics and delta
scaling on the dense cloud fields at full extent (rows past the count are stale and never read);
rrtmgpnn_solver_request_active_columns and the _rfmip solver; rrtmgpnn_scatter_columns into sw_up / sw_dn / sw_dir.  The
count of daylit columns is a device word that the network and the solver read, so a captured step follows the sun:
set_sza() between replays, no recapture.  The LW chain is untouched.  Not with mcica, aerosols, clrsky, byband, sw_dual,
fused=False, sw=False, capture_chains or run_blocks.  Off (the default), nothing of the step changes.

mcica={..., "daylit": True} (fused): the daylit-column SW chain under McICA-sampled clouds, with aerosols= and the "clrsky"
key where given -- the configuration of a weather or climate host.  The chain is the daylit=True one with four
differences.  The aerosol's three SW band arrays are gathered too, in a rrtmgpnn_gather_columns call of their own (their
rows are long: the call runs the long-row gather kernel), and the other arrays take a second call where they exceed 16.  The packed mask is sampled for the compacted columns directly, by the _active twin of the step's
mask entry: dense column j reads cloud_frac, overlap_param and the random numbers of column idx[j] in place -- none of
them is gathered -- and, seeded, draws with the counter word col0 + idx[j], so a column has the clouds it has in the
step without "daylit".  The solver call has the cloud-mask, the aerosol (where given) and the active-column requests
armed together (solver family 8).  With "clrsky", the active-column request is armed again (sw_active_clr) for the clear
launch, which takes the aerosol as its own increment or none (family 7), and one rrtmgpnn_scatter_columns writes all six
SW flux arrays, zeros at night in each.  The LW chain is untouched: full extent, its own mask and stream.  set_sza,
set_aerosols, set_mcica_seed and set_mcica_randoms work between graph replays without recapture.  Not with
mcica["byband"], sw_dual, fused=False, capture_chains or run_blocks; daylit=True beside it is refused as above.

sfc_byband=True (fused, clouds= with mcica= and / or aerosols=): the step also owns the SW fluxes at the surface by band,
sw_sfc_bnd_up / sw_sfc_bnd_dn / sw_sfc_bnd_dir, (ncol, nband) each (sfc_byband_fluxes()) -- what a host hands to its land,
ocean and sea-ice models.  rrtmgpnn_solver_request_sfc_byband (sw_sfc_byband, host-only) is armed right before the
all-sky SW launch, beside its mask and aerosol requests, and that launch forms the band sums of its surface level
(solver family 9); the clear launch is as it was.  With mcica["daylit"] the solver writes dense rows and a
rrtmgpnn_scatter_columns call of their own (daylit_scatter_sfc, rows of nband floats) puts them back, zeros at night.
The values are the surface level of the by-band fluxes of the same step.  Not with byband, mcica["byband"], sw_dual,
fused=False, sw=False, daylit=True, nor without clouds= and one of mcica= and aerosols=.  Off (the default), nothing of
the step changes.
"""

from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, data, shard
from ._lib import check, float_array, int_array, ptr_array
from .api import GAUSS_DS, GAUSS_WTS, Context


# calls of the SW chain (issued on the second stream when overlapping)
SW_CHAIN = {"sw_boundary", "nn_inputs_sw", "predict_nn_sw", "cloud_optics_sw", "delta_scale_sw", "increment_sw",
            "sw_byband", "sw_solver", "sw_solver_clr", "mcica_mask_sw", "draw_samples_sw", "sw_mask",
            "mcica_randoms_sw", "sw_mask_byband", "sw_aerosol", "increment_aer_sw",
            "daylit_plan", "daylit_gather", "sw_active", "daylit_scatter",
            "daylit_gather2", "daylit_gather3", "sw_active_clr", "sw_sfc_byband", "daylit_scatter_sfc"}


# issue order of the fused step (stable sort; names not listed keep their place at the end)
# (lw_byband / sw_byband: a byband step's by-band requests, host-only calls issued right before their solver;
# mcica_mask_*: a McICA step's mask kernels, which depend on no network; lw_mask / sw_mask: its cloud-mask requests,
# host-only like the by-band ones; lw_mask_byband / sw_mask_byband: the two as one paired request, mcica={"byband": True};
# lw_jacobian: a jacobian=True step's request, host-only too; lw_aerosol / sw_aerosol: an aerosols= step's requests
# beside clouds, host-only)
# (lw_solver_clr: an lw_scattering step's clear launch, ahead of the mask request its all-sky launch consumes)
# (lw_upper_bc: an upper_bc=True step's boundary flux, at the head of the LW chain)
# (daylit_plan / daylit_gather: a daylit=True step's compaction at the head of the SW chain; sw_active: its active-column
# request, host-only, right before the solver; daylit_scatter: the fluxes back to their columns, behind it)
# (daylit_gather2 / daylit_gather3: a mcica["daylit"] step's further gather calls, for what the first call's 16 arrays leave
# and for the aerosol's long rows, which get a call of their own; sw_active_clr:
# its active-column request for the clear launch sw_solver_clr, which in every other step is the chain's last call)
# (sw_sfc_byband: a sfc_byband=True step's request, host-only, right before the all-sky solver; daylit_scatter_sfc: its
# dense rows back to their columns in a mcica["daylit"] step)
FUSED_ORDER = ["sw_boundary", "get_col_dry", "expand_emis", "lw_upper_bc", "nn_inputs_lw", "cloud_optics_lw", "mcica_mask_lw",
               "predict_nn_lw", "lw_solver_clr", "lw_byband", "lw_mask", "lw_mask_byband", "lw_jacobian", "lw_aerosol", "lw_solver", "daylit_plan", "daylit_gather", "daylit_gather2", "daylit_gather3", "nn_inputs_sw", "cloud_optics_sw",
               "delta_scale_sw", "mcica_mask_sw", "predict_nn_sw", "sw_byband", "sw_mask", "sw_mask_byband", "sw_aerosol", "sw_active", "sw_sfc_byband", "sw_solver", "sw_active_clr", "sw_solver_clr", "daylit_scatter",
               "daylit_scatter_sfc"]


def issue_order(calls, fused, lw_after=""):
    """The step's issue order of `calls` ((name, fn, args) tuples): fused steps sort by FUSED_ORDER (stable; names
    not listed keep their place at the end); lw_after (an SW-chain call) moves the SW-chain calls up to and including
    it ahead of the rest, so the LW chain can be gated on it.  Each chain keeps its own relative order (a chain is
    issued on one stream, in this order)."""
    calls = list(calls)
    if fused:
        order = {n: i for i, n in enumerate(FUSED_ORDER)}
        calls.sort(key=lambda c: order.get(c[0], len(order)))
    if lw_after:
        names = [n for n, _, _ in calls]
        if lw_after not in names or lw_after not in SW_CHAIN or "get_col_dry" in names:
            raise ValueError("lw_after: %r is not a call of this fused step's SW chain" % lw_after)
        cut = names.index(lw_after)
        head = [c for i, c in enumerate(calls) if c[0] in SW_CHAIN and i <= cut]
        # an upper_bc=True step's boundary flux depends on no network: issued on the LW stream ahead of the gate it runs
        # beside the SW chain's head, and the LW network stays the first call behind the gate (at C3 the option added
        # 0.099 ms to the step so, 0.125 ms with the call behind the gate: DESIGN.md section 3)
        pre = [c for c in calls if c[0] == "lw_upper_bc"]
        calls = pre + head + [c for c in calls if c not in head and c not in pre]
    return calls


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


class ClearSkyStep:
    """One column block's step (module docstring).  `calls`, its launch list of (name, fn, args), is built chain by
    chain: _lw_chain() and _sw_chain() write each chain's calls down in the order the unfused step issues them, from
    one record per chain (_chain_record) and one method per sequence the two chains share (_cloud_optics_call,
    _clouds_in, _request); _finish() applies the schedule.  tests/golden/step_plan.json pins the list, the buffers and
    the schedule of every option set (tests/step_plan.py).

    sw=False: the LW half alone (config C2, rrtmgp_rfmip_lw.F90): gas optics LW + Planck + rte_lw.
    byband: the step also owns by-band fluxes (ty_fluxes_byband; lw_bnd_up / lw_bnd_dn, sw_bnd_up / sw_bnd_dn /
    sw_bnd_dir, (ncol, nlay+1, nband)) and arms rrtmgpnn_solver_request_byband before each solver call, so the
    solvers' by-band instances run and a captured graph carries the arrays.
    clrsky (all-sky steps): the step also owns clear-sky fluxes of the same columns (lw_up_clr, lw_dn_clr, sw_up_clr,
    sw_dn_clr, sw_dir_clr; clrsky_fluxes()).  By-band clear-sky fluxes are out of scope: clrsky with byband is refused.
    lw_after: the SW-chain call the LW chain starts after on two streams (None: the default gate in _finish; "": the
    chains start together).  (`overlap` is the stream-overlap flag.)
    mcica (all-sky steps): McICA-sampled clouds (extensions/cloud_optics/mo_cloud_sampling.F90) in place of overcast
    ones: {"cloud_frac": (ncol, nlay), "randoms_lw": (ncol, nlay, ngpt_lw), "randoms_sw": (ncol, nlay, ngpt_sw),
    "overlap_param": None (maximum-random overlap) or (ncol, nlay-1) (exponential-random)}.  The randoms are step-owned
    device buffers (mcica_randoms()) the caller refills between steps or replays (set_mcica_randoms).  With "seed": int
    (and optionally "stream_lw": 0, "stream_sw": 1, "col0": 0) in place of "randoms_lw" / "randoms_sw" the numbers are
    drawn in the mask kernels (the _seeded entries) from two step-owned 4-word device buffers, which set_mcica_seed
    rewrites between steps or replays; fused=False then fills scratch arrays with rrtmgpnn_mcica_randoms ahead of the
    class layer's sequence.  "clrsky": True / "byband": True: also the clear-sky fluxes of the same columns / the by-band
    fluxes of a byband=True step under the sampled clouds, not the two together; the clrsky= and byband= arguments
    themselves are refused with mcica.
    sw_dual (fused steps with clear-sky outputs): the SW chain's two solver launches are one call of
    rrtmgpnn_sw_solver_2stream_rfmip_clr_all (sw_solver; no sw_solver_clr), which the context's
    rrtmgpnn_context_set_sw_clr_all mode runs as the dual kernel or as the two launches; the same ten flux arrays, bit
    for bit.  Refused without clear-sky outputs, with sw=False, fused=False or byband.
    jacobian: the step also owns lw_up_jac (ncol, nlay+1), the Jacobian of lw_up with respect to the surface
    temperature (rte_lw's flux_up_Jac), requested from the LW solver call; refused with byband, clrsky and their mcica
    keys.
    aerosols: aerosol optical properties by band, {"lw_tau": (ncol, nlay, nband_lw), "sw_tau", "sw_ssa", "sw_g": (ncol,
    nlay, nband_sw)} (the SW keys only with sw=True), in step-owned device buffers (aer_tau_lw, aer_tau_sw, aer_ssa_sw,
    aer_g_sw) that set_aerosols refills between steps or replays: added to the gas properties ahead of the clear solve,
    so the clear-sky fluxes are those of gases plus aerosols; refused with byband, jacobian and mcica["byband"].
    sfc_byband: the step also owns the SW fluxes at the surface by band (sw_sfc_bnd_up / sw_sfc_bnd_dn / sw_sfc_bnd_dir,
    (ncol, nband); sfc_byband_fluxes()), formed by the all-sky SW launch of a fused step with clouds= and mcica= and / or
    aerosols= (module docstring); refused with byband, mcica["byband"], sw_dual, fused=False, sw=False and daylit=True."""

    def __init__(self, prob, device=0, nmus=1, ctx=None, lw_models=("lw_abs", "lw_pfrac"),
                 sw_models=("sw_abs", "sw_ray"), fused=True, clouds=None, icergh=2, cloud_lut=True, overlap=True,
                 sw=True, lw_after=None, sw_after=None, sw_priority=0, lw_net_cus=None, sw_net_cus=0, byband=False,
                 clrsky=False, mcica=None, jacobian=False, aerosols=None, lw_scattering=False, sw_dual=False,
                 lw_dual=False, upper_bc=False, spectral=None, daylit=False, sfc_byband=False):
        lw_models, sw_models = self._resolve_spectral(spectral, lw_models, sw_models)
        self.sfc_byband = bool(sfc_byband)
        if self.sfc_byband:
            # (ahead of the other option checks, so that the refusal names this option)
            bad = [w for w, on in (("byband", bool(byband)),
                                   ("mcica['byband']", mcica is not None and bool(mcica.get("byband"))),
                                   ("sw_dual", bool(sw_dual)), ("fused=False", not fused), ("sw=False", not sw),
                                   ("daylit=True", bool(daylit)), ("no clouds", clouds is None),
                                   ("neither mcica nor aerosols", mcica is None and aerosols is None)) if on]
            if bad:
                raise ValueError("sfc_byband=True with %s is not supported: the surface by-band fluxes come from the fused "
                                 "all-sky SW launch under a McICA mask and / or behind an aerosol request (the by-band "
                                 "outputs of byband=True hold the surface level)" % ", ".join(bad))
        self.daylit = bool(daylit)
        if self.daylit:
            # (ahead of the other option checks, so that the refusal names this option)
            bad = [w for w, on in (("mcica", mcica is not None), ("aerosols", aerosols is not None),
                                   ("clrsky", bool(clrsky)), ("byband", bool(byband)), ("sw_dual", bool(sw_dual)),
                                   ("fused=False", not fused), ("sw=False", not sw)) if on]
            if bad:
                raise ValueError("daylit=True with %s is not supported: the daylit-column SW chain is the fused clear-sky "
                                 "or overcast one, broadband only (the active-count network and solver instances)"
                                 % ", ".join(bad))
        self.mcica_daylit = mcica is not None and bool(mcica.get("daylit"))
        if self.mcica_daylit:
            # (before any device object exists; daylit=True beside it was refused above)
            bad = [w for w, on in (("mcica['byband']", bool(mcica.get("byband"))), ("sw_dual", bool(sw_dual)),
                                   ("fused=False", not fused)) if on]
            if bad:
                raise ValueError("mcica['daylit'] with %s is not supported: the daylit-column McICA SW chain is the fused "
                                 "one with one solver launch per sky, broadband only (the active-count masked and aerosol "
                                 "solver instances)" % ", ".join(bad))
        self.lw_dual = bool(lw_dual)
        self.upper_bc = bool(upper_bc)
        if self.lw_dual:
            # (ahead of the other option checks, so that the refusal names this option)
            bad = [w for w, on in (("lw_scattering=False", not lw_scattering),
                                   ("no clear-sky outputs (clrsky=True or mcica's 'clrsky')",
                                    not (clrsky or (mcica is not None and mcica.get("clrsky")))),
                                   ("fused=False", not fused), ("byband", bool(byband)), ("jacobian", bool(jacobian)),
                                   ("mcica['byband']", mcica is not None and bool(mcica.get("byband")))) if on]
            if bad:
                raise ValueError("lw_dual=True with %s is not supported: the clear + all-sky LW entry for scattering "
                                 "clouds serves the fused LW chain of an lw_scattering step with clear-sky outputs, "
                                 "broadband only" % ", ".join(bad))
        self._resolve_options(fused, clouds, sw, sw_priority, byband, clrsky, mcica, aerosols, jacobian)
        self.sw_dual = bool(sw_dual)
        if self.sw_dual:
            bad = [w for w, on in (("no clear-sky outputs (clrsky=True or mcica's 'clrsky')", not self.clrsky),
                                   ("sw=False", not sw), ("fused=False", not fused), ("byband", self.byband)) if on]
            if bad:
                raise ValueError("sw_dual=True with %s is not supported: the clear + all-sky SW entry serves the fused "
                                 "SW chain of a step with clear-sky outputs, broadband only" % ", ".join(bad))
        self.jacobian = bool(jacobian)
        self.lw_scattering = bool(lw_scattering)
        if self.lw_scattering:
            bad = [w for w, on in (("fused=False", not fused), ("byband", self.byband), ("jacobian", self.jacobian),
                                   ("aerosols", self.aerosols and not self.lw_dual), ("no clouds", clouds is None)) if on]
            if bad:
                raise ValueError("lw_scattering=True with %s is not supported: the fused rescaled LW solve takes band "
                                 "clouds (clouds=) and gives broadband fluxes only" % ", ".join(bad))
        if self.jacobian and (self.byband or self.clrsky):
            raise ValueError("jacobian=True with by-band or clear-sky outputs (byband, clrsky or the mcica keys) is not "
                             "supported: the solvers' by-band and clear + all-sky instances carry no Jacobian")
        self._open_device(device, ctx, lw_models, sw_models, icergh, cloud_lut)
        self._allocate(prob, clouds, mcica)
        if self.aerosols:
            self._allocate_aerosols(aerosols)
        self._prepare_arguments(nmus)
        # unfused, the SW boundary conditions follow get_col_dry, the call the SW stream forks after
        self.calls = self._col_dry() + self._sw_boundary() + self._lw_chain() + (self._sw_chain() if sw else [])
        if sw:
            self._finish(overlap, lw_after, sw_after, lw_net_cus, sw_net_cus)
        else:
            self._finish(False)

    def _resolve_spectral(self, spectral, lw_models, sw_models):
        """spectral=: the step's spectral configuration.  None: the shipped g256 / g224 tables and the models named by
        lw_models / sw_models.  A dict selects the k-distribution tables by ngpt and loads the models from paths:
        "ngpt_lw", "ngpt_sw" (data.load_kdist's ngpt; absent or None: the shipped tables), "lw_models" (absorption,
        Planck fraction) or (single model,), "sw_models" (absorption, Rayleigh) -- model files, netCDF or RBIN."""
        self._ngpt_lw = self._ngpt_sw = None
        if spectral is None:
            return lw_models, sw_models
        unknown = set(spectral) - {"lw_models", "sw_models", "ngpt_lw", "ngpt_sw"}
        if unknown:
            raise ValueError("spectral: unknown keys %s" % sorted(unknown))
        self._ngpt_lw, self._ngpt_sw = spectral.get("ngpt_lw"), spectral.get("ngpt_sw")
        lw_models, sw_models = tuple(spectral.get("lw_models", lw_models)), tuple(spectral.get("sw_models", sw_models))
        if len(lw_models) not in (1, 2) or len(sw_models) != 2:
            raise ValueError("spectral: lw_models is (absorption, planck_frac) or (both,), sw_models (absorption, "
                             "rayleigh)")
        return lw_models, sw_models

    def _resolve_options(self, fused, clouds, sw, sw_priority, byband, clrsky, mcica, aerosols=None, jacobian=False):
        """Every option check, and the flags derived from the options, before any device object exists."""
        self.aerosols = aerosols is not None
        if self.aerosols:
            if byband or jacobian or (mcica is not None and mcica.get("byband")):
                raise ValueError("aerosols with byband=True, jacobian=True or mcica['byband'] is not supported: the "
                                 "solvers' aerosol instances have no by-band or Jacobian outputs")
            want = {"lw_tau"} | ({"sw_tau", "sw_ssa", "sw_g"} if sw else set())
            if set(aerosols) != want:
                raise ValueError("aerosols: expected the keys %s, got %s" % (sorted(want), sorted(aerosols)))
        self.mcica = mcica is not None
        if self.mcica and clouds is None:
            raise ValueError("mcica: sampled clouds need clouds=(lwp, iwp, rel, rei)")
        if self.mcica and (clrsky or byband):
            raise ValueError("mcica with clrsky=True or byband=True is not supported (clear-sky fluxes beside the "
                             "sampled ones: the key mcica={..., 'clrsky': True})")
        if self.mcica and not sw:
            raise ValueError("mcica with sw=False is not supported")
        self.clrsky = bool(clrsky) or bool(self.mcica and mcica.get("clrsky"))
        if self.clrsky and clouds is None:
            raise ValueError("clrsky=True: clear-sky fluxes beside the all-sky ones need clouds=(lwp, iwp, rel, rei)")
        if self.clrsky and byband:
            raise ValueError("clrsky=True with byband=True: by-band clear-sky fluxes are not supported")
        mcica_byband = bool(self.mcica and mcica.get("byband"))
        if mcica_byband and self.clrsky:
            raise ValueError("mcica: 'byband' with 'clrsky': the clear + all-sky kernel has no by-band form")
        self.seeded = bool(self.mcica and mcica.get("seed") is not None)
        if self.seeded:
            if mcica.get("randoms_lw") is not None or mcica.get("randoms_sw") is not None:
                raise ValueError("mcica: seed together with randoms_lw / randoms_sw")
            self._seed = {"seed": int(mcica["seed"]), "stream_lw": int(mcica.get("stream_lw", 0)),
                          "stream_sw": int(mcica.get("stream_sw", 1)), "col0": int(mcica.get("col0", 0))}
        self.allsky = clouds is not None
        self.fused, self.sw, self.sw_priority = fused, sw, sw_priority
        self.byband = bool(byband) or mcica_byband
        # fused McICA by-band: each chain's mask and by-band requests are one paired request
        self._paired = mcica_byband and fused

    def _open_device(self, device, ctx, lw_models, sw_models, icergh, cloud_lut):
        """The step's streams and context, and the model data: networks, k-distributions, cloud optics."""
        self.dev = torch.device("cuda", device)
        self._own_ctx = ctx is None  # a caller's context keeps its settings (the LW network's CU cap in _finish)
        # Streams: non-blocking HIP streams this step alone holds for its lifetime (_lib.stream_acquire), released by
        # close() after its graph and contexts -- never torch's pooled streams, which torch hands out round-robin to
        # every caller, nor the legacy null stream.  Captures run on these same streams and replays launch on the LW
        # one (the round-5 host segfault).
        self._streams, self._closed, self.graph, self.ctx2 = [], False, None, None
        self.ctx = ctx or Context(device, self._new_stream())
        L = self.L = _lib.lib()
        self.kd_lw, self.kd_sw = data.load_kdist("lw", self._ngpt_lw), data.load_kdist("sw", self._ngpt_sw)

        def net(name):
            h = _lib.c_vp()
            check(L.rrtmgpnn_network_load(self.ctx.h, data.path(name).encode(), h), "network_load " + name)
            return h

        self.lw_nets = [net(n) for n in lw_models]
        self.sw_nets = [net(n) for n in sw_models]
        self.lw_names = data.rbin.unchars(data.load_model(lw_models[0])["input_names"])
        self.sw_names = data.rbin.unchars(data.load_model(sw_models[0])["input_names"])
        self.nx_lw, self.nx_sw = len(self.lw_names), len(self.sw_names)
        self.ng_lw, self.ng_sw = self.kd_lw["ngpt"], self.kd_sw["ngpt"]
        self.nb_lw = self.kd_lw["nband"]
        for w, models, ng in (("lw", lw_models, self.ng_lw), ("sw", sw_models, self.ng_sw)):
            for k, name in enumerate(models):  # a single LW model predicts tau and the Planck fraction: 2 ngpt outputs
                ny = int(data.load_model(name)["dims"][-1])
                if ny != (2 * ng if w == "lw" and len(models) == 1 else ng):
                    raise ValueError("%s model %r has %d outputs, the %s k-distribution %d g-points"
                                     % (w, name, ny, w, ng))
        if self.allsky:
            self.nb_sw = self.kd_sw["nband"]
            self.cloud_lw, self.cloud_sw = (self._cloud_optics(w, cloud_lut, icergh) for w in ("lw", "sw"))

    def _allocate(self, prob, clouds, mcica):
        """The step's HBM-resident tensors: inputs, intermediates, outputs, and what clrsky / byband / mcica add."""
        self.ncol, self.nlay = ncol, nlay = prob["ncol"], prob["nlay"]
        self.top_at_1 = int(bool(prob["top_at_1"]))
        dev, sw, fused = self.dev, self.sw, self.fused

        # ---- inputs ----
        self._gas_names = list(prob["gases"])
        ins = self._inputs(prob, clouds)
        self.play, self.plev, self.tlay, self.tlev, self.tsfc = ins[:5]
        self.gases = dict(zip(self._gas_names, ins[5:5 + len(self._gas_names)]))
        self.sfc_emis, self.sza, self.tsi, self.sfc_alb = ins[5 + len(self._gas_names):9 + len(self._gas_names)]
        self.totplnk = _t(self.kd_lw["totplnk"], dev)
        # gas_optics_ext's toa_src per g-point: solar_source after set_tsi(1361) (rrtmgp_rfmip_sw.F90:317)
        self.solar_source = _t(data.set_tsi(self.kd_sw["solar_source"], 1361.0), dev)
        self.sfc_lay = 1 if prob["play"][0, 0] > prob["play"][0, nlay - 1] else nlay

        # ---- intermediates / outputs ----
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        self.col_dry = f(ncol, nlay)
        self.x_lw, self.x_sw = f(ncol, nlay, self.nx_lw), f(ncol, nlay, self.nx_sw)
        self.tau_lw, self.lay_src = f(ncol, nlay, self.ng_lw), f(ncol, nlay, self.ng_lw)
        self.emis_gpt = f(ncol, self.ng_lw)
        if sw:
            self.tau_sw, self.ssa_sw = f(ncol, nlay, self.ng_sw), f(ncol, nlay, self.ng_sw)
            # the SW boundary conditions, formed every step (unfused: rrtmgpnn_sw_boundary_rfmip; fused: in the SW
            # solver, which uses these only as scratch when its kernel does not form them itself)
            self.toa, self.alb, self.mu0 = f(ncol, self.ng_sw), f(ncol, self.ng_sw), f(ncol)
        if not fused:  # arrays the fused step never materialises
            self.lev_src = f(ncol, nlay + 1, self.ng_lw)
            self.sfc_src, self.sfc_jac = f(ncol, self.ng_lw), f(ncol, self.ng_lw)
        if not fused and sw:
            self.g_sw = f(ncol, nlay, self.ng_sw)
        if self.allsky:
            self.lwp, self.iwp, self.rel, self.rei = ins[-4:]
            self.cld_tau_lw = f(ncol, nlay, self.nb_lw)
            if self.lw_scattering:
                self.cld_ssa_lw, self.cld_g_lw = f(ncol, nlay, self.nb_lw), f(ncol, nlay, self.nb_lw)
            self.cld_tau_sw, self.cld_ssa_sw, self.cld_g_sw = (f(ncol, nlay, self.nb_sw) for _ in range(3))
        if self.mcica:
            self._allocate_mcica(mcica, f)
        f_sw = f if sw else (lambda *s: f(*s).zero_())  # an LW-only step's SW fluxes are zero
        self.lw_up, self.lw_dn = f(ncol, nlay + 1), f(ncol, nlay + 1)
        self.sw_up, self.sw_dn, self.sw_dir = (f_sw(ncol, nlay + 1) for _ in range(3))
        if self.upper_bc:
            self._upper_bc_check(prob)
            self.lw_inc_flux = f(ncol, self.ng_lw)
        if self.jacobian:
            self.lw_up_jac = f(ncol, nlay + 1)
        if self.clrsky:
            self.lw_up_clr, self.lw_dn_clr = f(ncol, nlay + 1), f(ncol, nlay + 1)
            self.sw_up_clr, self.sw_dn_clr, self.sw_dir_clr = (f_sw(ncol, nlay + 1) for _ in range(3))
        if self.byband:
            self.lw_bnd_up, self.lw_bnd_dn = f(ncol, nlay + 1, self.nb_lw), f(ncol, nlay + 1, self.nb_lw)
            if sw:
                self.sw_bnd_up, self.sw_bnd_dn, self.sw_bnd_dir = (
                    f(ncol, nlay + 1, self.kd_sw["nband"]) for _ in range(3))
        if self.sfc_byband:
            self.sw_sfc_bnd_up, self.sw_sfc_bnd_dn, self.sw_sfc_bnd_dir = (
                f(ncol, self.kd_sw["nband"]).zero_() for _ in range(3))
        if self.daylit or self.mcica_daylit:
            self._allocate_daylit()

    def _allocate_daylit(self):
        """A daylit=True step's plan (idx, slot, the count word) and the dense twins of what its SW chain reads and
        writes, all of full extent so that an all-day replay fits.  The twins start as copies: rows at or past the
        count, which the full-extent cloud kernels still walk, always hold some column's values."""
        ncol, dev = self.ncol, self.dev
        self.day_idx, self.day_slot = (torch.zeros(ncol, dtype=torch.int32, device=dev) for _ in range(2))
        self.nday = torch.zeros(1, dtype=torch.int32, device=dev)
        names = ["play", "tlay", "plev"]
        # the SW network's gases (inputs 3 on; every gas of the step is an (ncol, nlay) array) and get_col_dry's h2o
        self._day_gases = [n for n in dict.fromkeys(["h2o"] + list(self.sw_names[2:])) if n in self.gases]
        names += ["sza", "tsi", "sfc_alb"] + (["lwp", "iwp", "rel", "rei"] if self.allsky else [])
        self._day_pairs = [(getattr(self, n), n) for n in names] + [(self.gases[n], "gas_" + n) for n in self._day_gases]
        for t, n in self._day_pairs:
            setattr(self, "d_" + n, t.clone())
        self.d_sw_up, self.d_sw_dn, self.d_sw_dir = (torch.zeros_like(self.sw_up) for _ in range(3))
        self._day_pairs_aer = []
        if self.mcica_daylit and self.clrsky:
            self.d_sw_up_clr, self.d_sw_dn_clr, self.d_sw_dir_clr = (torch.zeros_like(self.sw_up) for _ in range(3))
        if self.sfc_byband:
            self.d_sw_sfc_bnd_up, self.d_sw_sfc_bnd_dn, self.d_sw_sfc_bnd_dir = (
                torch.zeros_like(self.sw_sfc_bnd_up) for _ in range(3))
        # (a mcica["daylit"] step gathers in as many calls as its list needs: its aerosol arrays join in _allocate_aerosols)
        if len(self._day_pairs) > 16 and not self.mcica_daylit:
            raise ValueError("daylit=True: more than 16 arrays to gather")

    def set_sza(self, sza):
        """Overwrite the step's solar zenith angles (degrees, (ncol)) between steps or graph replays; complete on
        return.  A daylit=True step plans its daylit columns from them on the device every step: no recapture."""
        torch.cuda.synchronize(self.dev)  # nothing in flight reads the angles
        src = sza if isinstance(sza, torch.Tensor) else _t(sza, self.dev)
        if tuple(src.shape) != tuple(self.sza.shape):
            raise ValueError("set_sza: sza has shape %s, expected %s" % (tuple(src.shape), tuple(self.sza.shape)))
        self.sza.copy_(src)
        torch.cuda.synchronize(self.dev)

    def _upper_bc_check(self, prob):
        """compute_bc's pressure check (extensions/mo_compute_bc.F90:110-114) on a host problem's plev(:, top_lay)."""
        from .compute_bc import pressure_check
        top = 0 if prob["top_at_1"] else prob["nlay"] - 1
        e = pressure_check(np.asarray(prob["plev"])[:, top], self.kd_lw["press_ref_min"][0])
        if e:
            raise ValueError(e)

    def _allocate_aerosols(self, aerosols):
        """An aerosols= step's band properties, step-owned: the solver calls hold their addresses."""
        ncol, nlay = self.ncol, self.nlay
        self.nb_sw = self.kd_sw["nband"]
        want = {"lw_tau": (ncol, nlay, self.nb_lw)}
        if self.sw:
            want.update({k: (ncol, nlay, self.nb_sw) for k in ("sw_tau", "sw_ssa", "sw_g")})
        for k, shape in want.items():
            if tuple(np.shape(aerosols[k])) != shape:
                raise ValueError("aerosols: %s has shape %s, expected %s" % (k, tuple(np.shape(aerosols[k])), shape))
            w, q = k.split("_")
            setattr(self, "aer_%s_%s" % (q, w), torch.empty(shape, dtype=torch.float32, device=self.dev))
        self.set_aerosols(**aerosols)
        if self.mcica_daylit:  # the SW aerosol of the daylit columns: dense twins, gathered every step
            for n in ("aer_tau_sw", "aer_ssa_sw", "aer_g_sw"):
                setattr(self, "d_" + n, getattr(self, n).clone())
                self._day_pairs_aer.append((getattr(self, n), n))

    def set_aerosols(self, lw_tau=None, sw_tau=None, sw_ssa=None, sw_g=None):
        """Copy new aerosol properties into the step's buffers (None keeps an array) between steps or graph replays;
        complete on return."""
        if not self.aerosols:
            raise ValueError("set_aerosols: the step was built without aerosols=")
        torch.cuda.synchronize(self.dev)  # nothing in flight reads the buffers
        for name, src in (("aer_tau_lw", lw_tau), ("aer_tau_sw", sw_tau), ("aer_ssa_sw", sw_ssa), ("aer_g_sw", sw_g)):
            if src is None:
                continue
            dst = getattr(self, name, None)
            if dst is None:
                raise ValueError("set_aerosols: an LW-only step holds no SW aerosols")
            src = src if isinstance(src, torch.Tensor) else _t(src, self.dev)
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError("set_aerosols: %s has shape %s, expected %s" % (name, tuple(src.shape), tuple(dst.shape)))
            dst.copy_(src)
        torch.cuda.synchronize(self.dev)

    def _allocate_mcica(self, mcica, f):
        """A McICA step's cloud fraction, overlap parameter, random numbers (or seed words) and masks."""
        ncol, nlay, dev = self.ncol, self.nlay, self.dev
        self.cloud_frac = _t(mcica["cloud_frac"], dev)
        ov = mcica.get("overlap_param")
        self.overlap_param = None if ov is None else _t(ov, dev)
        if self.seeded:
            self.rng_lw, self.rng_sw = (torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(2))
            self.set_mcica_seed()
            # unfused: scratch arrays rrtmgpnn_mcica_randoms fills every step
            self.randoms_lw = None if self.fused else f(ncol, nlay, self.ng_lw)
            self.randoms_sw = None if self.fused else f(ncol, nlay, self.ng_sw)
        else:
            self.randoms_lw, self.randoms_sw = _t(mcica["randoms_lw"], dev), _t(mcica["randoms_sw"], dev)
        want = {"cloud_frac": (ncol, nlay), "randoms_lw": (ncol, nlay, self.ng_lw),
                "randoms_sw": (ncol, nlay, self.ng_sw), "overlap_param": (ncol, nlay - 1)}
        for k, t in (("cloud_frac", self.cloud_frac), ("randoms_lw", self.randoms_lw),
                     ("randoms_sw", self.randoms_sw), ("overlap_param", self.overlap_param)):
            if t is not None and tuple(t.shape) != want[k]:
                raise ValueError("mcica: %s has shape %s, expected %s" % (k, tuple(t.shape), want[k]))
        if self.fused:  # the packed masks the solvers take
            self.mask_bits_lw = torch.zeros((ncol, nlay, (self.ng_lw + 31) // 32), dtype=torch.int32, device=dev)
            self.mask_bits_sw = torch.zeros((ncol, nlay, (self.ng_sw + 31) // 32), dtype=torch.int32, device=dev)
        else:  # the class layer's logical masks and g-point cloud properties
            self.mask_lw = torch.zeros((ncol, nlay, self.ng_lw), dtype=torch.uint8, device=dev)
            self.mask_sw = torch.zeros((ncol, nlay, self.ng_sw), dtype=torch.uint8, device=dev)
            self.smp_tau_lw = f(ncol, nlay, self.ng_lw)
            self.smp_tau_sw, self.smp_ssa_sw, self.smp_g_sw = (f(ncol, nlay, self.ng_sw) for _ in range(3))

    def _p(self, *names):
        """The device addresses of the step's tensors of these names (None where this mode holds no such tensor)."""
        return tuple(None if t is None else t.data_ptr() for t in (getattr(self, n, None) for n in names))

    def _prepare_arguments(self, nmus):
        """The ctypes arrays the calls share, and the two chains' records."""
        def gas_args(names):
            ptrs, nds = [], []
            for k, n in enumerate(names):
                t = self.gases.get(n) if k >= 2 else None
                ptrs.append(t.data_ptr() if t is not None else None)
                nds.append(2)
            return ptr_array(ptrs), int_array(nds)

        self._g_lw, self._nd_lw = gas_args(self.lw_names)
        self._g_sw, self._nd_sw = gas_args(self.sw_names)
        self._nets_lw = ptr_array([h.value for h in self.lw_nets])
        self._nets_sw = ptr_array([h.value for h in self.sw_nets])
        self._lims_lw = int_array(self.kd_lw["band_lims_gpt"].ravel())
        self._lims_sw = int_array(self.kd_sw["band_lims_gpt"].ravel())
        self._Ds, self._W = float_array(GAUSS_DS[nmus]), float_array(GAUSS_WTS[nmus])
        self.nmus = nmus
        self._chain_lw = self._chain_record("lw", self.kd_lw, self._lims_lw)
        self._chain_sw = self._chain_record("sw", self.kd_sw, self._lims_sw)

    def _chain_record(self, w, kd, lims):
        """What the cloud handling of the two chains differs in: the sizes and band limits, and the addresses (or None)
        of the optical properties, the clouds by band, the sampled clouds, the masks, the random numbers and the
        by-band outputs.  The LW chain carries tau alone, so the ssa and g slots of its triples are NULL (but for an
        lw_scattering step's band clouds, cld_ssa_lw and cld_g_lw); the SW
        asymmetry parameter is NULL in the fused step (quirk B-6: identically zero in the NN path, which the SW kernels
        take as a literal 0 instead of writing and re-reading a zero array; same fluxes, bit for bit)."""
        p = self._p
        triple = (lambda stem: p(stem + "tau_lw") + (p(stem + "ssa_lw", stem + "g_lw") if stem == "cld_" else (None, None))) \
            if w == "lw" else \
            (lambda stem: p(stem + "tau_sw", stem + "ssa_sw", stem + "g_sw"))
        mask, bits, randoms, rng = p("mask_" + w, "mask_bits_" + w, "randoms_" + w, "rng_" + w)
        return SimpleNamespace(sfx=w, ngpt=kd["ngpt"], nband=kd["nband"], lims=lims, props=triple(""),
                               cld=triple("cld_"), smp=triple("smp_"), aer=triple("aer_"), mask=mask, bits=bits, randoms=randoms, rng=rng,
                               bnd=p(w + "_bnd_up", w + "_bnd_dn") + (p("sw_bnd_dir") if w == "sw" else (None,)))

    # ---- the sequences both chains issue, from a chain's record ----
    def _cloud_optics_call(self, ch):
        """Cloud optics by band (rrtmgp_allsky.F90:383, :420); none on a clear-sky step."""
        if not self.allsky:
            return []
        return [("cloud_optics_" + ch.sfx, self.L.rrtmgpnn_cloud_optics_compute,
                 (self.ctx.h, getattr(self, "cloud_" + ch.sfx), self.ncol, self.nlay)
                 + self._p("lwp", "iwp", "rel", "rei") + ch.cld)]

    def _clouds_in(self, ch):
        """clouds%increment(atmos) of a chain (rrtmgp_allsky.F90:383-395, :420-433).  Fused, the solver adds the band
        clouds itself, so only a McICA step issues something here: the mask kernel, into packed bits.  Unfused: the
        increment by band, or the class layer's McICA sequence at g-point resolution, (randoms ->) mask -> draw_samples
        -> increment."""
        L, c, ncol, nlay = self.L, self.ctx.h, self.ncol, self.nlay
        if not self.allsky:
            return []
        if self.fused:
            return [self._mask_call(ch, None, ch.bits)] if self.mcica else []
        if not self.mcica:
            return [("increment_" + ch.sfx, L.rrtmgpnn_increment_bybnd,
                     (c, ncol, nlay, ch.ngpt, ch.nband, ch.lims) + ch.props + ch.cld)]
        return self._randoms_call(ch) + [
            self._mask_call(ch, ch.mask, None),
            ("draw_samples_" + ch.sfx, L.rrtmgpnn_draw_samples,
             (c, ch.ngpt, nlay, ncol, ch.nband, ch.lims, ch.mask) + ch.cld + ch.smp),
            ("increment_" + ch.sfx, L.rrtmgpnn_increment, (c, ncol, nlay, ch.ngpt) + ch.props + ch.smp),
        ]

    def _request(self, ch, mask=True):
        """The host-only request armed right before the solver call that consumes it: the fused McICA step's cloud mask
        (mask=False: that solver entry takes the mask as an argument), the by-band outputs, or the two as one paired
        request."""
        L, c = self.L, self.ctx.h
        if self._paired:
            return [(ch.sfx + "_mask_byband", L.rrtmgpnn_solver_request_byband_mcica,
                     (c, ch.nband, ch.lims) + ch.bnd + (ch.ngpt, self.nlay, self.ncol, ch.bits))]
        if self.mcica and self.fused:
            return [(ch.sfx + "_mask", L.rrtmgpnn_solver_request_cloud_mask,
                     (c, ch.ngpt, self.nlay, self.ncol, ch.bits))] if mask else []
        if self.byband:
            return [(ch.sfx + "_byband", L.rrtmgpnn_solver_request_byband, (c, ch.nband, ch.lims) + ch.bnd)]
        return []

    def _aerosol_request(self, ch):
        """A fused aerosols= step's request beside clouds, armed right before the chain's all-sky solver call, which adds
        the aerosol in front of its own (cloud) increment."""
        if not (self.aerosols and self.fused and self.allsky):
            return []
        return [(ch.sfx + "_aerosol", self.L.rrtmgpnn_solver_request_aerosol,
                 (self.ctx.h, ch.nband, self.nlay, self.ncol) + ch.aer)]

    def _aerosols_in(self, ch):
        """An unfused aerosols= step's aer_props%increment(optical_props), right after gas optics."""
        if not self.aerosols or self.fused:
            return []
        return [("increment_aer_" + ch.sfx, self.L.rrtmgpnn_increment_bybnd,
                 (self.ctx.h, self.ncol, self.nlay, ch.ngpt, ch.nband, ch.lims) + ch.props + ch.aer)]

    def _sfc_byband_request(self, ch, dense=False):
        """A sfc_byband=True step's request, armed right before the all-sky SW solver call beside its mask and aerosol
        requests: the surface level's band sums into sw_sfc_bnd_* (dense: a mcica["daylit"] step's dense twins)."""
        if not self.sfc_byband:
            return []
        out = ["%ssw_sfc_bnd_%s" % ("d_" if dense else "", k) for k in ("up", "dn", "dir")]
        return [("sw_sfc_byband", self.L.rrtmgpnn_solver_request_sfc_byband,
                 (self.ctx.h, ch.nband, ch.lims, self.ncol) + self._p(*out))]

    def _jacobian_request(self):
        """A jacobian=True step's request, armed right before the LW solver call (after the chain's other request, which
        it may stand beside): flux_up_Jac into lw_up_jac.  Fused, the solver forms sfc_source_Jac itself and takes none;
        unfused, the array planck_source wrote."""
        if not self.jacobian:
            return []
        return [("lw_jacobian", self.L.rrtmgpnn_solver_request_jacobian,
                 (self.ctx.h, self.ng_lw, self.nlay, self.ncol)
                 + ((None,) if self.fused else self._p("sfc_jac")) + self._p("lw_up_jac"))]

    def _mask_call(self, ch, mask, bits):
        """The chain's call of sampled_mask_max_ran, or _exp_ran when the step has an overlap parameter, into a logical
        mask or packed bits; a seeded fused step, which holds no random numbers, calls the _seeded entry on its 4-word
        buffer."""
        src, sfx = (ch.rng, "_seeded") if ch.randoms is None else (ch.randoms, "")
        head = (self.ctx.h, ch.ngpt, self.nlay, self.ncol, src) + self._p("cloud_frac")
        if self.overlap_param is None:
            return ("mcica_mask_" + ch.sfx, getattr(self.L, "rrtmgpnn_sampled_mask_max_ran" + sfx), head + (mask, bits))
        return ("mcica_mask_" + ch.sfx, getattr(self.L, "rrtmgpnn_sampled_mask_exp_ran" + sfx),
                head + self._p("overlap_param") + (mask, bits))

    def _randoms_call(self, ch):
        """A seeded unfused step's fill of its scratch randoms ([] on the array route)."""
        if not self.seeded:
            return []
        return [("mcica_randoms_" + ch.sfx, self.L.rrtmgpnn_mcica_randoms,
                 (self.ctx.h, ch.ngpt, self.nlay, self.ncol, ch.rng, ch.randoms))]

    # ---- the call list ----
    def _col_dry(self):
        """Unfused: col_dry, computed once for both chains (the fused network kernels form it themselves)."""
        if self.fused:
            return []
        return [("get_col_dry", self.L.rrtmgpnn_get_col_dry,
                 (self.ctx.h, self.ncol, self.nlay, self.gases["h2o"].data_ptr()) + self._p("plev", "col_dry"))]

    def _sw_boundary(self):
        """The driver's SW boundary conditions.  Fused: formed in the SW solver's prologue
        (rrtmgpnn_sw_solver_2stream_rfmip).  Round 6 before that: a kernel at the head of the SW chain (7.7 us at C3);
        on the LW stream beside the SW network, with the SW solver waiting for it, the C3 step measured 0.497 ms against
        0.43 (the extra edge into the SW solver let the LW network take the CUs first; profiles/r06/README.md).
        Unfused (the class layer's calls): a kernel of its own."""
        if self.fused or not self.sw:
            return []
        return [("sw_boundary", self.L.rrtmgpnn_sw_boundary_rfmip,
                 (self.ctx.h, self.ng_sw, self.ncol)
                 + self._p("solar_source", "tsi", "sfc_alb", "sza", "toa", "alb", "mu0"))]

    def _lw_chain(self):
        """The LW chain's calls in issue order (unfused: after get_col_dry)."""
        L, c, ncol, nlay, p, ch = self.L, self.ctx.h, self.ncol, self.nlay, self._p, self._chain_lw
        h2o = (self.gases["h2o"].data_ptr(),)
        if self.fused:
            # compute_nn_inputs + get_col_dry + predict_nn_lw in one kernel (rrtmgpnn_gas_optics_lw_nn): the network
            # inputs and column amounts are formed in-kernel and never stored (same bits as the three calls)
            return [
                *self._upper_bc_call(),
                ("predict_nn_lw", L.rrtmgpnn_gas_optics_lw_nn,
                 (c, ncol, nlay, self.ng_lw, self.nx_lw) + p("play", "tlay", "plev") + h2o
                 + (self._g_lw, self._nd_lw, self._nets_lw, len(self.lw_nets)) + p("tau_lw", "lay_src")),
                *self._cloud_optics_call(ch),
                *self._clouds_in(ch),
                *self._lw_clear_scattering(),
                # (the clear + all-sky McICA entry takes the mask as an argument)
                *self._request(ch, mask=not self.clrsky or self.lw_scattering),
                *self._jacobian_request(),
                *self._aerosol_request(ch),
                self._lw_solver_fused(),
            ]
        planck = (self.nb_lw, self.ng_lw, self.kd_lw["nPlanckTemp"]) + p("tlay", "tlev", "tsfc") + (
            self.sfc_lay, self._lims_lw, float(self.kd_lw["temp_ref_min"][0]), float(self.kd_lw["totplnk_delta"]))
        solver = lambda name, up, dn: (  # noqa: E731
            name, L.rrtmgpnn_lw_solver_noscat,
            (c, self.ng_lw, nlay, ncol, self.top_at_1, self.nmus, self._Ds, self._W) + p("lw_inc_flux")
            + p("tau_lw", "lay_src", "lev_src", "emis_gpt", "sfc_src", up, dn))
        clouds = self._clouds_in(ch)
        return [
            *self._upper_bc_call(),
            ("nn_inputs_lw", L.rrtmgpnn_compute_nn_inputs,
             (c, ncol, nlay, self.nx_lw) + p("play", "tlay") + (self._g_lw, self._nd_lw, self.lw_nets[0]) + p("x_lw")),
            ("predict_nn_lw", L.rrtmgpnn_predict_nn_lw,
             (c, ncol, nlay, self.ng_lw, self.nx_lw) + p("x_lw", "col_dry") + (self._nets_lw, len(self.lw_nets))
             + p("tau_lw", "lay_src")),
            *self._aerosols_in(ch),
            *self._cloud_optics_call(ch),
            # clouds%increment(atmos) before rte_lw (rrtmgp_allsky.F90:383-395) ...
            *([] if self.clrsky else clouds),
            ("planck_source", L.rrtmgpnn_compute_planck_source_nn,
             (c, ncol, nlay) + planck + p("totplnk", "sfc_src", "sfc_jac", "lay_src", "lev_src")),
            ("expand_emis", L.rrtmgpnn_expand_band_to_gpt,
             (c, self.nb_lw, self.ng_lw, ncol, self._lims_lw) + p("sfc_emis", "emis_gpt")),
            # ... or, with clear-sky fluxes, after the clear solve (mo_rrtmgp_clr_all_sky.F90:161-172)
            *([solver("lw_solver_clr", "lw_up_clr", "lw_dn_clr")] + clouds if self.clrsky else []),
            *self._request(ch),
            *self._jacobian_request(),
            solver("lw_solver", "lw_up", "lw_dn"),
        ]

    def _upper_bc_call(self):
        """An upper_bc=True step's boundary flux into lw_inc_flux, the inc_flux of the chain's solver calls: in flux
        units (as_flux = 1) at the step's angles."""
        if not self.upper_bc:
            return []
        kd = self.kd_lw
        return [("lw_upper_bc", self.L.rrtmgpnn_compute_bc_lw,
                 (self.ctx.h, self.ncol, self.nlay, self.ng_lw, self.nx_lw, self.top_at_1, float(kd["press_ref_min"][0]))
                 + self._p("play", "plev", "tlay") + (self.gases["h2o"].data_ptr(),)
                 + (self._g_lw, self._nd_lw, self._nets_lw, len(self.lw_nets), self.nb_lw, kd["nPlanckTemp"],
                    self._lims_lw, float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]))
                 + self._p("totplnk") + (self.nmus, self._Ds, self._W, 1) + self._p("lw_inc_flux"))]

    def _lw_planck_args(self, inc, up, dn):
        """The arguments of a fused-Planck LW entry: `inc` the names of its band increment's arrays."""
        p = self._p
        return (self.ctx.h, self.ng_lw, self.nlay, self.ncol, self.top_at_1, self.nmus, self._Ds, self._W) \
            + p("lw_inc_flux", "tau_lw", *inc, "lay_src") \
            + (self.nb_lw, self.kd_lw["nPlanckTemp"]) + p("tlay", "tlev", "tsfc") \
            + (self.sfc_lay, self._lims_lw, float(self.kd_lw["temp_ref_min"][0]), float(self.kd_lw["totplnk_delta"])) \
            + p("totplnk") + (1,) + p("sfc_emis", up, dn)

    def _lw_clear_scattering(self):
        """An lw_scattering step's clear launch (clrsky): the no-scattering fused-Planck entry on the gas optical depth,
        issued ahead of the cloud-mask request, which belongs to the all-sky launch."""
        if not (self.lw_scattering and self.clrsky) or self.lw_dual:  # (lw_dual: both sets from the one solver call)
            return []
        return [("lw_solver_clr", self.L.rrtmgpnn_lw_solver_noscat_planck,
                 self._lw_planck_args((), "lw_up_clr", "lw_dn_clr"))]

    def _lw_solver_fused(self):
        """The fused step's LW solver call: compute_Planck_source_nn fused into the solver (sources formed in-kernel
        from pfrac; the surface emissivity goes in by band, as rte_lw takes it, and is expanded in-kernel).  All-sky,
        the cloud increment by band is added as tau is read (_planck_inc); with clear-sky fluxes both flux sets come
        from one call of the dual entry (_clr_all), whose McICA twin takes the packed mask as its last argument instead
        of a request."""
        L, p = self.L, self._p
        if self.lw_dual:
            # scattering clouds with clear-sky outputs from one entry: the mask request (all-sky set only) and the
            # aerosol request (both sets) stand right before it; rrtmgpnn_context_set_lw_scat_clr_all decides one
            # launch or two
            return ("lw_solver", L.rrtmgpnn_lw_solver_1rescl_planck_clr_all,
                    self._lw_planck_args(("cld_tau_lw", "cld_ssa_lw", "cld_g_lw"), "lw_up", "lw_dn")
                    + p("lw_up_clr", "lw_dn_clr"))
        if self.lw_scattering:
            # scattering clouds: the rescaled solver with the two-stream band increment (a McICA step's mask is armed
            # by request, with or without clear-sky fluxes)
            return ("lw_solver", L.rrtmgpnn_lw_solver_1rescl_planck_inc,
                    self._lw_planck_args(("cld_tau_lw", "cld_ssa_lw", "cld_g_lw"), "lw_up", "lw_dn"))
        args = (self.ctx.h, self.ng_lw, self.nlay, self.ncol, self.top_at_1, self.nmus, self._Ds, self._W) \
            + p("lw_inc_flux", "tau_lw") + (p("cld_tau_lw") if self.allsky else p("aer_tau_lw") if self.aerosols else ()) \
            + p("lay_src") \
            + (self.nb_lw, self.kd_lw["nPlanckTemp"]) + p("tlay", "tlev", "tsfc") \
            + (self.sfc_lay, self._lims_lw, float(self.kd_lw["temp_ref_min"][0]), float(self.kd_lw["totplnk_delta"])) \
            + p("totplnk") + (1,) + p("sfc_emis", "lw_up", "lw_dn")
        if self.clrsky and self.mcica:
            return ("lw_solver", L.rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica,
                    args + p("lw_up_clr", "lw_dn_clr", "mask_bits_lw"))
        if self.clrsky:
            return ("lw_solver", L.rrtmgpnn_lw_solver_noscat_planck_clr_all, args + p("lw_up_clr", "lw_dn_clr"))
        # (clear sky with aerosols: the aerosol is the entry's own increment)
        inc = self.allsky or self.aerosols
        entry = L.rrtmgpnn_lw_solver_noscat_planck_inc if inc else L.rrtmgpnn_lw_solver_noscat_planck
        return ("lw_solver", entry, args)

    def _sw_chain(self):
        """The SW chain's calls in issue order (unfused: after sw_boundary)."""
        L, c, ncol, nlay, p, ch = self.L, self.ctx.h, self.ncol, self.nlay, self._p, self._chain_sw
        h2o = (self.gases["h2o"].data_ptr(),)
        delta_scale = [("delta_scale_sw", L.rrtmgpnn_delta_scale_2str,
                        (c, ncol * nlay * self.nb_sw) + ch.cld + (None,))] if self.allsky else []
        if self.daylit or self.mcica_daylit:
            return self._sw_chain_daylit()
        if self.fused:
            # the boundary conditions and (all sky) clouds%increment(atmos) fused into the solver
            # (rrtmgpnn_sw_solver_2stream_rfmip; same bits as sw_boundary_rfmip + sw_solver_2stream[_inc])
            no_inc = (0, None, None, None, None)
            # aerosols: the clear launch's own increment, and with clouds a request ahead of the all-sky launch
            aer_inc = (self.nb_sw, self._lims_sw) + ch.aer if self.aerosols else no_inc
            band_inc = (self.nb_sw, self._lims_sw) + ch.cld if self.allsky else aer_inc
            solver = lambda name, inc, *out: (  # noqa: E731
                name, L.rrtmgpnn_sw_solver_2stream_rfmip,
                (c, self.ng_sw, nlay, ncol, self.top_at_1) + p("solar_source", "tsi", "sfc_alb", "sza")
                + p("tau_sw", "ssa_sw") + (None,) + inc + p("toa", "alb", "mu0", *out))
            head = [
                ("predict_nn_sw", L.rrtmgpnn_gas_optics_sw_nn,
                 (c, ncol, nlay, self.ng_sw, self.nx_sw) + p("play", "tlay", "plev") + h2o
                 + (self._g_sw, self._nd_sw, self._nets_sw) + ch.props),
                *self._cloud_optics_call(ch),
                *delta_scale,
                *self._clouds_in(ch),
                *self._request(ch),
                *self._aerosol_request(ch),
                *self._sfc_byband_request(ch),
            ]
            if self.sw_dual:
                # both flux sets from one call (rrtmgpnn_sw_solver_2stream_rfmip_clr_all): the same requests ahead of
                # it, the clear outputs behind the all-sky ones
                return head + [(
                    "sw_solver", L.rrtmgpnn_sw_solver_2stream_rfmip_clr_all,
                    (c, self.ng_sw, nlay, ncol, self.top_at_1) + p("solar_source", "tsi", "sfc_alb", "sza")
                    + p("tau_sw", "ssa_sw") + (None,) + band_inc
                    + p("toa", "alb", "mu0", "sw_up", "sw_dn", "sw_dir", "sw_up_clr", "sw_dn_clr", "sw_dir_clr"))]
            return head + [
                solver("sw_solver", band_inc, "sw_up", "sw_dn", "sw_dir"),
                # clear-sky fluxes: one more solver launch on the SW chain, on the gas optics' own properties (the fused
                # solver leaves tau / ssa as they were).  Through the same entry without an increment: the
                # checkpointed kernel forms the boundary conditions in its prologue and never stores them, so there is
                # nothing in toa / alb / mu0 for a plain solver call to read
                *([solver("sw_solver_clr", aer_inc, "sw_up_clr", "sw_dn_clr", "sw_dir_clr")]
                  if self.clrsky else []),
            ]
        solver = lambda name, *out: (  # noqa: E731
            name, L.rrtmgpnn_sw_solver_2stream,
            (c, self.ng_sw, nlay, ncol, self.top_at_1) + p("toa") + (None,) + ch.props + p("mu0", "alb", "alb", *out))
        return [
            ("nn_inputs_sw", L.rrtmgpnn_compute_nn_inputs,
             (c, ncol, nlay, self.nx_sw) + p("play", "tlay") + (self._g_sw, self._nd_sw, self.sw_nets[0]) + p("x_sw")),
            ("predict_nn_sw", L.rrtmgpnn_predict_nn_sw,
             (c, ncol, nlay, self.ng_sw, self.nx_sw) + p("x_sw", "col_dry") + (self._nets_sw,) + ch.props),
            *self._aerosols_in(ch),
            # clouds%delta_scale(); clouds%increment(atmos) before rte_sw (rrtmgp_allsky.F90:420-433), and with clear-sky
            # fluxes the clear solve before the increment (mo_rrtmgp_clr_all_sky.F90:246-259)
            *self._cloud_optics_call(ch),
            *delta_scale,
            *([solver("sw_solver_clr", "sw_up_clr", "sw_dn_clr", "sw_dir_clr")] if self.clrsky else []),
            *self._clouds_in(ch),
            *self._request(ch),
            solver("sw_solver", "sw_up", "sw_dn", "sw_dir"),
        ]

    def _sw_chain_daylit(self):
        """A daylit=True step's SW chain (module docstring): the fused chain on dense twins of its inputs, between the
        plan + gather at its head and the scatter at its end.  usecol = sza < 90 - 2 spacing(90)
        (rrtmgp_rfmip_sw.F90:285-287), the bound the solver's own mu0 merge uses."""
        L, c, ncol, nlay, p, ch = self.L, self.ctx.h, self.ncol, self.nlay, self._p, self._chain_sw
        bound = float(np.float32(90.0) - np.float32(2.0) * data.spacing(90.0))
        pairs = self._day_pairs
        if self.mcica_daylit:
            return self._sw_chain_mcica_daylit(bound)
        rows = [int(t[0].numel()) if t.dim() > 1 else 1 for t, _ in pairs]
        # (ctypes arrays the captured calls point at: kept on the step)
        self._day_src = ptr_array([t.data_ptr() for t, _ in pairs])
        self._day_dst = ptr_array([getattr(self, "d_" + n).data_ptr() for _, n in pairs])
        self._day_rows = int_array(rows)
        self._day_dense = ptr_array(list(p("d_sw_up", "d_sw_dn", "d_sw_dir")))
        self._day_out = ptr_array(list(p("sw_up", "sw_dn", "sw_dir")))
        self._day_out_rows = int_array([nlay + 1] * 3)
        dense_gas = {n: getattr(self, "d_gas_" + n) for n in self._day_gases}
        g = [dense_gas.get(n) if k >= 2 else None for k, n in enumerate(self.sw_names)]
        self._g_sw_day = ptr_array([t.data_ptr() if t is not None else None for t in g])
        cld_in = p("d_lwp", "d_iwp", "d_rel", "d_rei")
        band_inc = (self.nb_sw, self._lims_sw) + ch.cld if self.allsky else (0, None, None, None, None)
        return [
            ("daylit_plan", L.rrtmgpnn_daylit_plan, (c, ncol) + p("sza") + (0, bound) + p("day_idx", "day_slot", "nday")),
            ("daylit_gather", L.rrtmgpnn_gather_columns,
             (c, ncol, len(pairs), self._day_src, self._day_dst, self._day_rows) + p("day_idx", "nday")),
            ("predict_nn_sw", L.rrtmgpnn_gas_optics_sw_nn_active,
             (c, ncol, nlay, self.ng_sw, self.nx_sw) + p("d_play", "d_tlay", "d_plev", "d_gas_h2o")
             + (self._g_sw_day, self._nd_sw, self._nets_sw) + ch.props + p("nday")),
            *([("cloud_optics_sw", L.rrtmgpnn_cloud_optics_compute, (c, self.cloud_sw, ncol, nlay) + cld_in + ch.cld),
               ("delta_scale_sw", L.rrtmgpnn_delta_scale_2str, (c, ncol * nlay * self.nb_sw) + ch.cld + (None,))]
              if self.allsky else []),
            ("sw_active", L.rrtmgpnn_solver_request_active_columns, (c, ncol) + p("nday")),
            ("sw_solver", L.rrtmgpnn_sw_solver_2stream_rfmip,
             (c, self.ng_sw, nlay, ncol, self.top_at_1) + p("solar_source", "d_tsi", "d_sfc_alb", "d_sza")
             + p("tau_sw", "ssa_sw") + (None,) + band_inc + p("toa", "alb", "mu0", "d_sw_up", "d_sw_dn", "d_sw_dir")),
            ("daylit_scatter", L.rrtmgpnn_scatter_columns,
             (c, ncol, 3, self._day_dense, self._day_out, self._day_out_rows) + p("day_slot")),
        ]

    def _sw_chain_mcica_daylit(self, bound):
        """A mcica["daylit"] step's SW chain (module docstring): the daylit=True chain with the aerosol gathered too, the
        mask sampled for the compacted columns, the three requests ahead of the all-sky launch and, with clear-sky
        outputs, the clear launch on the active columns behind it; one scatter of three or six flux arrays."""
        L, c, ncol, nlay, p, ch = self.L, self.ctx.h, self.ncol, self.nlay, self._p, self._chain_sw
        pairs = self._day_pairs
        # (ctypes arrays the captured calls point at: kept on the step) -- 16 arrays per gather call; the aerosol's band
        # arrays (rows of nband * nlay floats) in a call of their own, which then runs the long-row gather kernel
        self._day_tables = []
        for part in [pairs[k:k + 16] for k in range(0, len(pairs), 16)] + ([self._day_pairs_aer] if self.aerosols else []):
            self._day_tables.append((len(part), ptr_array([t.data_ptr() for t, _ in part]),
                                     ptr_array([getattr(self, "d_" + n).data_ptr() for _, n in part]),
                                     int_array([int(t[0].numel()) if t.dim() > 1 else 1 for t, _ in part])))
        if len(self._day_tables) > 3:
            raise ValueError("mcica['daylit']: more than three gather calls")
        sky = ("", "_clr") if self.clrsky else ("",)
        dense = ["d_sw_%s%s" % (k, s) for s in sky for k in ("up", "dn", "dir")]
        self._day_dense = ptr_array(list(p(*dense)))
        self._day_out = ptr_array(list(p(*[n[2:] for n in dense])))
        self._day_out_rows = int_array([nlay + 1] * len(dense))
        dense_gas = {n: getattr(self, "d_gas_" + n) for n in self._day_gases}
        g = [dense_gas.get(n) if k >= 2 else None for k, n in enumerate(self.sw_names)]
        self._g_sw_day = ptr_array([t.data_ptr() if t is not None else None for t in g])
        no_inc = (0, None, None, None, None)
        aer = p("d_aer_tau_sw", "d_aer_ssa_sw", "d_aer_g_sw")
        aer_inc = (self.nb_sw, self._lims_sw) + aer if self.aerosols else no_inc
        solver = lambda name, inc, *out: (  # noqa: E731
            name, L.rrtmgpnn_sw_solver_2stream_rfmip,
            (c, self.ng_sw, nlay, ncol, self.top_at_1) + p("solar_source", "d_tsi", "d_sfc_alb", "d_sza")
            + p("tau_sw", "ssa_sw") + (None,) + inc + p("toa", "alb", "mu0", *out))
        # the _active twin of the step's mask entry: the plan's idx and count in place of the byte mask
        src, sfx = (ch.rng, "_seeded") if ch.randoms is None else (ch.randoms, "")
        exp_ran = self.overlap_param is not None
        mask = ("mcica_mask_sw",
                getattr(L, "rrtmgpnn_sampled_mask_%s%s_active" % ("exp_ran" if exp_ran else "max_ran", sfx)),
                (c, ch.ngpt, nlay, ncol, src) + p("cloud_frac") + (p("overlap_param") if exp_ran else ())
                + p("day_idx", "nday") + (ch.bits,))
        active = lambda name: (name, L.rrtmgpnn_solver_request_active_columns, (c, ncol) + p("nday"))  # noqa: E731
        sfc_scatter = []
        if self.sfc_byband:
            # the surface rows (nband floats) back to their columns, zeros at night: a scatter call of their own
            sfc = ["sw_sfc_bnd_%s" % k for k in ("up", "dn", "dir")]
            self._day_sfc_dense = ptr_array(list(p(*["d_" + n for n in sfc])))
            self._day_sfc_out = ptr_array(list(p(*sfc)))
            self._day_sfc_rows = int_array([self.nb_sw] * 3)
            sfc_scatter = [("daylit_scatter_sfc", L.rrtmgpnn_scatter_columns,
                            (c, ncol, 3, self._day_sfc_dense, self._day_sfc_out, self._day_sfc_rows) + p("day_slot"))]
        return [
            ("daylit_plan", L.rrtmgpnn_daylit_plan, (c, ncol) + p("sza") + (0, bound) + p("day_idx", "day_slot", "nday")),
            *[("daylit_gather" + ("", "2", "3")[k], L.rrtmgpnn_gather_columns, (c, ncol) + t + p("day_idx", "nday"))
              for k, t in enumerate(self._day_tables)],
            ("predict_nn_sw", L.rrtmgpnn_gas_optics_sw_nn_active,
             (c, ncol, nlay, self.ng_sw, self.nx_sw) + p("d_play", "d_tlay", "d_plev", "d_gas_h2o")
             + (self._g_sw_day, self._nd_sw, self._nets_sw) + ch.props + p("nday")),
            ("cloud_optics_sw", L.rrtmgpnn_cloud_optics_compute,
             (c, self.cloud_sw, ncol, nlay) + p("d_lwp", "d_iwp", "d_rel", "d_rei") + ch.cld),
            ("delta_scale_sw", L.rrtmgpnn_delta_scale_2str, (c, ncol * nlay * self.nb_sw) + ch.cld + (None,)),
            mask,
            *self._request(ch),
            *([("sw_aerosol", L.rrtmgpnn_solver_request_aerosol, (c, ch.nband, nlay, ncol) + aer)]
              if self.aerosols else []),
            active("sw_active"),
            *self._sfc_byband_request(ch, dense=True),
            solver("sw_solver", (self.nb_sw, self._lims_sw) + ch.cld, "d_sw_up", "d_sw_dn", "d_sw_dir"),
            *([active("sw_active_clr"), solver("sw_solver_clr", aer_inc, "d_sw_up_clr", "d_sw_dn_clr", "d_sw_dir_clr")]
              if self.clrsky else []),
            ("daylit_scatter", L.rrtmgpnn_scatter_columns,
             (c, ncol, len(dense), self._day_dense, self._day_out, self._day_out_rows) + p("day_slot")),
            *sfc_scatter,
        ]

    def _finish(self, overlap, lw_after=None, sw_after=None, lw_net_cus=None, sw_net_cus=0):
        # fused: the small kernels that do not depend on a network's output go first in their chain, ahead of the big
        # ones: issued after the LW network (class-layer order), expand_emis waited ~75 us at C3 for CUs the SW solver
        # held while the LW solver, which needs it, could not start
        self.calls = issue_order(self.calls, self.fused)
        # overlap: the SW chain runs on a second context/stream, forked after col_dry (which both streams read; the
        # fused step, whose chains form col_dry each in their network kernel, forks at its start)
        # and joined at the end of the step -- the VALU-bound SW solver shares the CUs with the MFMA-bound LW
        # network and the LW solver instead of running after them
        self.overlap = overlap
        # The LW chain may start once a call of the SW chain has finished (issued first, the SW network then has the
        # chip to itself), and the SW solver may wait for a call of the LW chain (sw_after).  Default: the LW chain
        # after the SW network -- the SW chain is the critical path at every size.  Round 4, alternating whole steps on
        # one box: C3 0.435-0.439 ms, against 0.470-0.473 for both networks first and then the two solvers side by
        # side (the SW solver waiting for both networks) and 0.469-0.476 for the chains started together; C4 2.613-2.618
        # against 2.649-2.670 started together (3 pairs), C5 shard 62.96-63.03 against 63.64-63.65 (2 pairs).  Started
        # together at C4, the SW network ran beside the LW network and solver for 775 us (239 alone) and the SW solver
        # started 1.1 ms into the step.
        names = [n for n, _, _ in self.calls]
        gate = ""
        if overlap and self.fused and "predict_nn_sw" in names and "predict_nn_lw" in names:
            gate = "predict_nn_sw"
        if sw_after is None:
            sw_after = ""
        self.lw_after = (gate if lw_after is None else lw_after) if overlap else ""
        if self.lw_after:
            self.calls = issue_order(self.calls, self.fused, self.lw_after)
            self._gate = torch.cuda.Event()
        # lw_net_cus: the LW network's blocks on at most that many CUs (rrtmgpnn_context_set_mlp_max_cus; 0: all).
        # Default with the LW chain gated on the SW network and an SW solver grid that fits in one round of resident
        # waves (ncol * ngpt_sw / 128 waves of 64 lanes, 2 g-points per lane, against 16 per CU; C3): 3/8 of the CUs.
        # Each LW network block holds most of a CU's LDS (108 KB), so on the full chip it kept the SW solver, launched
        # beside it, off every CU for its first 75 us at C3; confined, it leaves the SW solver the other CUs from the
        # start.  Round 4, C3 whole steps (3 alternating rounds, one box): 0.4350-0.4368 ms on 160 CUs, 0.4374-0.4379
        # on 192, 0.4417-0.4434 on 224, 0.4456-0.4462 on all 256.  Round 6, on the kernels with their prologue loads in
        # flight (4 alternating rounds, profiles/r06/lwcap*_c3.txt): 96 CUs 1.1 % faster than 160 (every round), 128
        # 0.6-1.1 %, 64 and 144 equal.  With more columns (C4) the cap costs 2 % (the SW solver is throughput-bound
        # there; 2.705-2.726 on 192 against 2.651-2.664 ms); C5 equal.
        # A caller's context is left as it is unless lw_net_cus is given.  The caps are overlap measures: without a
        # second stream both networks run on self.ctx, so a cap would confine the SW network too -- refused.
        explicit = lw_net_cus is not None
        if not overlap and (lw_net_cus or sw_net_cus):
            raise ValueError("lw_net_cus / sw_net_cus cap the networks of overlapped chains; overlap is off")
        if lw_net_cus is None:
            lw_net_cus = 0
            cus = torch.cuda.get_device_properties(self.dev).multi_processor_count
            if self._own_ctx and self.overlap and self.lw_after and self.ncol * self.ng_sw <= 2048 * cus:
                lw_net_cus = 3 * cus // 8
        if self._own_ctx or explicit:
            self.ctx.set_mlp_max_cus(int(lw_net_cus))
        # the cap in force on the LW context (a caller's context may carry its own), which bench.py's serialised stage
        # timings lift and restore
        self.lw_net_cus = self.ctx.mlp_max_cus()
        # sw_after: an LW-chain call the SW solver waits for (the two networks first, then the two solvers side by side)
        self.sw_after = sw_after if overlap else ""
        if self.sw_after:
            names = [n for n, _, _ in self.calls]  # (as reordered for lw_after)
            if self.sw_after not in names or self.sw_after in SW_CHAIN or "sw_solver" not in names:
                raise ValueError("sw_after: %r is not a call of this fused step's LW chain" % self.sw_after)
            if names.index(self.sw_after) > names.index("sw_solver"):
                raise ValueError("sw_after: %r is issued after the SW solver" % self.sw_after)
            # the event is recorded on the LW stream right after that call is issued, and the SW stream waits for it
            # right before the SW solver -- the SW network, issued in between, does not wait
            self._gate2 = torch.cuda.Event()
        self.ctx2 = None
        if overlap:
            self.ctx2 = Context(self.dev.index, self._sw_stream())
            # sw_net_cus: the SW network's blocks on at most that many CUs (0: all; an A/B knob, not a default)
            self.sw_net_cus = int(sw_net_cus or 0)
            if self.sw_net_cus:
                check(self.L.rrtmgpnn_context_set_mlp_max_cus(self.ctx2.h, self.sw_net_cus), "context_set_mlp_max_cus")
            self.calls = [(n, f, ((self.ctx2.h,) + tuple(a[1:])) if n in SW_CHAIN else a) for n, f, a in self.calls]
            self._fork, self._join = torch.cuda.Event(), torch.cuda.Event()
        self.graph = None

    def set_mcica_seed(self, seed=None, stream_lw=None, stream_sw=None, col0=None):
        """Rewrite a seeded step's two 4-word buffers (None keeps a value) between steps or graph replays; complete on
        return."""
        if not (self.mcica and self.seeded):
            raise ValueError("set_mcica_seed: the step was built without mcica={'seed': ...}")
        for k, v in (("seed", seed), ("stream_lw", stream_lw), ("stream_sw", stream_sw), ("col0", col0)):
            if v is not None:
                self._seed[k] = int(v)
        torch.cuda.synchronize(self.dev)  # nothing in flight reads the words
        sd = self._seed
        for buf, stream in ((self.rng_lw, sd["stream_lw"]), (self.rng_sw, sd["stream_sw"])):
            check(self.L.rrtmgpnn_mcica_rng_set(self.ctx.h, sd["seed"] & 0xFFFFFFFFFFFFFFFF, stream & 0xFFFFFFFF,
                                                sd["col0"] & 0xFFFFFFFF, buf.data_ptr()), "mcica_rng_set")

    def mcica_randoms(self):
        """The step-owned device buffers of a McICA step's random numbers, (randoms_lw, randoms_sw), (ncol, nlay, ngpt)
        each: refill them (in place) between steps or graph replays."""
        if not self.mcica:
            raise ValueError("mcica_randoms: the step was built without mcica=")
        if self.seeded:
            raise ValueError("mcica_randoms: a seeded step holds no caller-filled random numbers (set_mcica_seed)")
        return self.randoms_lw, self.randoms_sw

    def set_mcica_randoms(self, randoms_lw=None, randoms_sw=None):
        """Copy new random numbers into the step's buffers; complete on return."""
        lw, sw = self.mcica_randoms()
        for dst, src in ((lw, randoms_lw), (sw, randoms_sw)):
            if src is not None:
                dst.copy_(_t(src, self.dev) if not isinstance(src, torch.Tensor) else src)
        torch.cuda.synchronize(self.dev)

    def _new_stream(self, priority=0):
        """A stream held by this step alone until close() (_lib.stream_acquire)."""
        h = _lib.stream_acquire(self.dev.index, priority)
        self._streams.append((h, priority))
        return torch.cuda.ExternalStream(h, device=self.dev)

    def _sw_stream(self):
        # default priority: a high-priority SW stream (critical path) was measured 25 % slower at C3 -- it takes every
        # CU first and the chains stop overlapping (tools/ab_prio.sh)
        # sw_priority < 0: a higher-priority stream (the two-solvers-side-by-side schedule, so the SW solver's blocks are
        # dispatched ahead of the LW solver's when both are ready)
        return self._new_stream(self.sw_priority)

    def stream_for(self, name):
        """The torch stream a call of `self.calls` is issued on."""
        return self.ctx2.stream if (self.overlap and name in SW_CHAIN) else self.ctx.stream

    def _cloud_optics(self, which, lut, icergh):
        h = _lib.c_vp()
        check(self.L.rrtmgpnn_cloud_optics_load(self.ctx.h, data.cloud_optics_path(which).encode(), int(bool(lut)), h),
              "cloud_optics_load " + which)
        check(self.L.rrtmgpnn_cloud_optics_set_ice_roughness(h, int(icergh)), "set_ice_roughness")
        return h

    def close(self):
        """Release the step's device state in dependency order: finish its work, destroy its hipGraph, then its
        contexts (workspaces, buffer pools) and cloud-optics objects, then hand its streams back.  Left to garbage collection the
        order is the attribute dict's (the contexts before the graph whose nodes address their workspaces).  Idempotent;
        the step is unusable afterwards."""
        if getattr(self, "_closed", True):
            return
        self._closed = True
        torch.cuda.synchronize(self.dev)
        g, self.graph = getattr(self, "graph", None), None
        for x in (g,) + tuple(getattr(self, "chain_graphs", ())):
            if x is not None:
                x.reset()
        self.chain_graphs = ()
        for k in ("cloud_lw", "cloud_sw"):
            h = getattr(self, k, None)
            if h:
                self.L.rrtmgpnn_cloud_optics_destroy(h)
                setattr(self, k, None)
        if getattr(self, "ctx2", None) is not None:
            self.ctx2.close()
        if self._own_ctx:
            self.ctx.close()
        streams, self._streams = self._streams, []
        for h, prio in streams:
            _lib.stream_release(h, self.dev.index, prio)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _enter(self):
        """Order the step after the caller's current stream (the step runs on its own streams); returns the caller's
        stream when it differs from the step's, for _leave."""
        cur = torch.cuda.current_stream(self.dev)
        if cur.cuda_stream == self.ctx.stream.cuda_stream:
            return None
        self.ctx.stream.wait_stream(cur)
        return cur

    def _leave(self, cur):
        if cur is not None:
            cur.wait_stream(self.ctx.stream)

    def step(self, timing=None):
        """Issue one step, ordered after the caller's current stream's work and before its later work.  timing: a dict
        name -> list; each launch is then bracketed by timing events recorded on the stream it runs on (the step's own
        concurrency is unchanged) and (start, end) is appended."""
        cur = self._enter()
        self._issue(timing)
        self._leave(cur)

    def _issue(self, timing=None):
        fork_after = "get_col_dry" if any(n == "get_col_dry" for n, _, _ in self.calls) else None
        if self.overlap and fork_after is None:  # fused step: the chains share no kernel; fork at the start
            self._fork.record(self.ctx.stream)
            self.ctx2.stream.wait_event(self._fork)
        for name, fn, args in self.calls:
            if self.sw_after and name == "sw_solver":
                self.ctx2.stream.wait_event(self._gate2)
            if timing is not None:
                s = self.stream_for(name)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
            rc = fn(*args)
            if rc:
                check(rc, name)
            if timing is not None:
                e1.record(s)
                timing.setdefault(name, []).append((e0, e1))
            if self.overlap and name == fork_after:
                self._fork.record(self.ctx.stream)
                self.ctx2.stream.wait_event(self._fork)
            if self.overlap and name == self.lw_after:
                self._gate.record(self.ctx2.stream)
                self.ctx.stream.wait_event(self._gate)
            if self.sw_after and name == self.sw_after:
                self._gate2.record(self.ctx.stream)
        if self.overlap:
            self._join.record(self.ctx2.stream)
            self.ctx.stream.wait_event(self._join)

    def capture(self):
        """Capture one step into a hipGraph (torch.cuda.CUDAGraph); replay with `replay()`.  The capture runs on the
        step's own streams (a caller's context, which may sit on the legacy null stream, is moved to a capture stream
        the step owns for the duration), with events of its own: no stream or event of the graph is shared with
        another graph or with eager steps."""
        self.step()  # warm-up: kernel attributes + workspace allocation happen outside capture
        torch.cuda.synchronize(self.dev)
        if self.graph is not None:
            self.graph.reset()
            self.graph = None
        self._fork, self._join = torch.cuda.Event(), torch.cuda.Event()
        if self.lw_after:
            self._gate = torch.cuda.Event()
        if self.sw_after:
            self._gate2 = torch.cuda.Event()
        g = torch.cuda.CUDAGraph()
        old = None
        if not self._own_ctx:
            if getattr(self, "_cap_stream", None) is None:
                self._cap_stream = self._new_stream()
            old = self.ctx.stream
            self.ctx.use_stream(self._cap_stream)
        s = self.ctx.stream
        try:
            with torch.cuda.graph(g, stream=s):
                self._issue()
        finally:
            if old is not None:
                self.ctx.use_stream(old)
        self.graph = g
        return g

    def capture_chains(self):
        """A stream of blocks (run_blocks): the SW chain (network, solver with the boundary conditions) and the LW chain
        (network, solver) captured as two hipGraphs, each on its own context's stream and alone -- no gate or join
        between them."""
        if not (self.overlap and self.sw):
            raise ValueError("capture_chains: a step with its LW and SW chains on two streams")
        self._refuse_blocks()
        if self.daylit:
            raise ValueError("daylit=True with capture_chains / run_blocks is not supported: a stream of blocks re-runs "
                             "one block, whose daylit columns do not change")
        self.step()  # warm-up outside capture
        torch.cuda.synchronize(self.dev)
        graphs = []
        for chain, ctx in ((lambda n: n in SW_CHAIN, self.ctx2), (lambda n: n not in SW_CHAIN, self.ctx)):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=ctx.stream):
                for name, fn, args in self.calls:
                    if chain(name):
                        rc = fn(*args)
                        if rc:
                            check(rc, name)
            graphs.append(g)
        self.chain_graphs = tuple(graphs)

    def _refuse_blocks(self):
        if self.mcica_daylit:
            raise ValueError("mcica['daylit'] with capture_chains / run_blocks is not supported: a stream of blocks "
                             "re-runs one block, whose daylit columns do not change")

    def run_blocks(self, k):
        """k blocks streamed through the step: each chain replays k times in its own stream's order, and block b+1's
        SW chain starts as soon as block b's SW solver is done -- beside block b's LW chain -- instead of after
        block b's join.  (A stream of distinct blocks needs each block's inputs and outputs in storage of its own;
        this one re-runs the step's block, whose results are the same every time.)  Ordered after the caller's
        current stream's work and before its later work."""
        self._refuse_blocks()
        if self.daylit:
            raise ValueError("daylit=True with capture_chains / run_blocks is not supported: a stream of blocks re-runs "
                             "one block, whose daylit columns do not change")
        g_sw, g_lw = self.chain_graphs
        cur = torch.cuda.current_stream(self.dev)
        for s in (self.ctx2.stream, self.ctx.stream):
            if s.cuda_stream != cur.cuda_stream:
                s.wait_stream(cur)
        for _ in range(k):
            with torch.cuda.stream(self.ctx2.stream):
                g_sw.replay()
            with torch.cuda.stream(self.ctx.stream):
                g_lw.replay()
        for s in (self.ctx2.stream, self.ctx.stream):
            if s.cuda_stream != cur.cuda_stream:
                cur.wait_stream(s)

    def replay(self):
        """Launch the captured step on the step's stream, ordered after the caller's current stream's work and before
        its later work."""
        cur = self._enter()
        with torch.cuda.stream(self.ctx.stream):
            self.graph.replay()
        self._leave(cur)

    def _inputs(self, prob, clouds=None):
        """Device input tensors of a host problem, in io_tensors() order: the state, the gases, the surface emissivity
        by band, and the driver's per-column SW state -- solar zenith angle, TSI, surface albedo (rrtmgp_rfmip_sw.F90:
        244-259) -- (+ the cloud fields)."""
        dev = self.dev
        ins = [_t(prob[k], dev) for k in ("play", "plev", "tlay", "tlev", "tsfc")]
        ins += [_t(prob["gases"][k], dev) for k in self._gas_names]
        ins += [_t(np.repeat(prob["sfc_emis"][:, None], self.nb_lw, axis=1), dev),  # (ncol, nband)
                _t(prob["sza"], dev), _t(prob["tsi"], dev), _t(prob["sfc_alb"], dev)]
        if clouds is not None:
            ins += [_t(a, dev) for a in clouds]
        return ins

    def inputs_for(self, prob, clouds=None):
        """io_tensors()-ordered device inputs of another block of the same shape (bench.py's chunked shard: copied
        into this step's inputs before each replay)."""
        if prob["ncol"] != self.ncol or prob["nlay"] != self.nlay or list(prob["gases"]) != self._gas_names:
            raise ValueError("inputs_for: block shape differs from the step's")
        if self.upper_bc:
            self._upper_bc_check(prob)
        return self._inputs(prob, clouds if self.allsky else None)

    def io_tensors(self):
        """(inputs, outputs): the device tensors a host-resident caller would upload / download per step."""
        ins = [self.play, self.plev, self.tlay, self.tlev, self.tsfc, *self.gases.values(), self.sfc_emis, self.sza,
               self.tsi, self.sfc_alb]
        if self.allsky:
            ins += [self.lwp, self.iwp, self.rel, self.rei]
        return ins, [self.lw_up, self.lw_dn, self.sw_up, self.sw_dn, self.sw_dir]

    def sfc_byband_fluxes(self):
        """Host copies of a sfc_byband step's SW fluxes at the surface by band, (ncol, nband) each."""
        if not self.sfc_byband:
            raise ValueError("sfc_byband_fluxes: the step was built without sfc_byband=True")
        return {k: getattr(self, k).cpu().numpy() for k in ("sw_sfc_bnd_up", "sw_sfc_bnd_dn", "sw_sfc_bnd_dir")}

    def byband_fluxes(self):
        """Host copies of a byband step's by-band fluxes, (ncol, nlay+1, nband) each."""
        names = ("lw_bnd_up", "lw_bnd_dn") + (("sw_bnd_up", "sw_bnd_dn", "sw_bnd_dir") if self.sw else ())
        return {k: getattr(self, k).cpu().numpy() for k in names}

    def clrsky_fluxes(self):
        """Host copies of a clrsky step's clear-sky broadband fluxes, keyed like fluxes() with a _clr suffix."""
        if not self.clrsky:
            raise ValueError("clrsky_fluxes: the step was built without clrsky=True")
        return {k: getattr(self, k).cpu().numpy()
                for k in ("lw_up_clr", "lw_dn_clr", "sw_up_clr", "sw_dn_clr", "sw_dir_clr")}

    def jacobian_flux(self):
        """Host copy of a jacobian=True step's lw_up_jac, (ncol, nlay+1)."""
        if not self.jacobian:
            raise ValueError("jacobian_flux: the step was built without jacobian=True")
        return self.lw_up_jac.cpu().numpy()

    def fluxes(self):
        """Host copies of the broadband fluxes, with SW zeroed where sza >= 90 is applied by the caller."""
        return {k: getattr(self, k).cpu().numpy() for k in ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")}


class ChunkedRank:
    """A rank's column range [lo, hi) streamed through one step in chunks (bench.py --global: a C5 rank holds more
    columns than one step's block).  Every chunk's inputs stay resident in HBM; `run()` copies each chunk's inputs
    into the step's input tensors (device to device, on the step's stream), replays the step (its hipGraph when
    captured) and copies its fluxes into the rank's flux slab `flux` (lw_up, lw_dn, sw_up, sw_dn, sw_dir; (hi - lo,
    nlay + 1) each).  A short last chunk runs through a second step of its own shape.

    problem(c0, c1) -> (prob, clouds): columns [c0, c1) of the global problem.  make_step(prob, clouds) -> a
    ClearSkyStep of that block's shape."""

    def __init__(self, lo, hi, chunk, problem, make_step, use_graph=True):
        self.lo, self.hi = lo, hi
        self.chunks = shard.chunk_ranges(lo, hi, chunk)
        self.steps, self._run_of, self.chunk_ins, self._step_of = [], [], [], []
        for k, (c0, c1) in enumerate(self.chunks):
            prob, clouds = problem(c0, c1)
            if k == 0:
                self.first = (prob, clouds)  # the first chunk's host problem (bench.py's CPU baseline samples it)
            st = next((s for s in self.steps if s.ncol == c1 - c0), None)
            if st is None:
                st = make_step(prob, clouds)
                self.steps.append(st)
                ins, _ = st.io_tensors()
                self.chunk_ins.append([t.clone() for t in ins] if len(self.chunks) > 1 else None)
                if use_graph:
                    st.capture()
            else:
                self.chunk_ins.append(st.inputs_for(prob, clouds))
            self._step_of.append(st)
        self.step = self.steps[0]
        dev = self.step.dev
        outs = self.step.io_tensors()[1]
        self.single = len(self.chunks) == 1
        self.flux = list(outs) if self.single else [
            torch.empty((hi - lo,) + tuple(o.shape[1:]), dtype=o.dtype, device=dev) for o in outs]
        self.use_graph = use_graph

    def run(self):
        """One pass over the rank's columns, ordered after the caller's current stream's work and before its later
        work (the chunks run on their steps' own streams; no ordering is needed between the two steps' chunks: their
        buffers and slab rows are disjoint)."""
        if self.single:
            st = self.step
            st.replay() if self.use_graph else st.step()
            return
        cur = torch.cuda.current_stream(self.step.dev)
        used = []
        for (c0, c1), st, src in zip(self.chunks, self._step_of, self.chunk_ins):
            ins, outs = st.io_tensors()
            s = st.ctx.stream
            if st not in used:
                used.append(st)
                if s.cuda_stream != cur.cuda_stream:
                    s.wait_stream(cur)
            with torch.cuda.stream(s):
                for d, x in zip(ins, src):
                    d.copy_(x, non_blocking=True)
                st.replay() if self.use_graph else st.step()
                for r, o in zip(self.flux, outs):
                    r[c0 - self.lo:c1 - self.lo].copy_(o, non_blocking=True)
        for st in used:
            if st.ctx.stream.cuda_stream != cur.cuda_stream:
                cur.wait_stream(st.ctx.stream)

    def close(self):
        """Release every step (ClearSkyStep.close: graph, contexts, streams, in that order)."""
        for st in self.steps:
            st.close()
