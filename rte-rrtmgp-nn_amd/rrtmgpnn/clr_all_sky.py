"""Clear-sky and all-sky fluxes from one call: extensions/mo_rrtmgp_clr_all_sky.F90's rte_lw and rte_sw over the class
layer of api.py.

Both follow the reference's sequence (:146-172 LW, :274-308 SW): gas optics once, the optional
aer_props%increment(optical_props), the clear solve into clrsky_fluxes, cloud_props%increment(optical_props), the
all-sky solve into allsky_fluxes.  k_dist is a GasOpticsRRTMGP (the reference takes the abstract ty_gas_optics), and
the networks go in as neural_nets, as GasOpticsRRTMGP.gas_optics takes them.  Error messages are the reference's,
typos included ('rrtmpg_lw: ...').

rte_lw takes the library's dual entry (rrtmgpnn_lw_solver_noscat_planck_clr_all: tau, the Planck fraction and the
band cloud optical depth read once, both flux sets from one kernel with one angle) when the cloud properties are
1scl and defined by band on k_dist's bands and both flux objects want broadband up / down fluxes only; gas optics then
leaves the Planck sources unformed and the kernel forms them.  With 2str clouds (LW scattering: the rescaled solver) in
the same situation, without aerosols or with aerosols of the fused kind (aerosol_by_request: 1scl, by band, same
extents), it takes the fused scattering route: gas optics into a 1scl object (no ssa / g arrays) and one call of
rrtmgpnn_lw_solver_1rescl_planck_clr_all, the cloud mask armed when mask_bits is given and the aerosols armed as its
aerosol request: clear sky = gases [+ aerosols] without scattering (the rescaled solver with ssa = g = 0 is the
no-scattering one, bit for bit), all sky = that + the clouds, the same bits as the sequence; the context's
rrtmgpnn_context_set_lw_scat_clr_all mode decides one dual launch or two.  LW_SCAT_FUSED = False keeps the sequence
below (the comparison route).  Every other case -- 2str clouds with other aerosols, clouds on g-points, g-point or
by-band outputs -- runs the two solves with api.rte_lw.

mask_bits= / cloud_mask= (both functions; not in the reference's interface) make the all-sky solve a McICA one: the band
cloud is sampled per g-point by a mask from cloud_sampling.sampled_mask_*.  Where rte_lw would take the dual entry it
takes its masked twin (rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica) on the packed mask, and rte_sw's all-sky solve is
the library's masked fused solve; the cases that fall back run draw_samples on the byte mask ahead of the reference's
sequence.

aer_props: where rte_lw takes a dual entry, or rte_sw the masked fused solve, and the aerosols are of the fused kind
(aerosol_by_request), they are not added to the g-point arrays by aer_props.increment but armed as the solver's
aerosol request (rrtmgpnn_solver_request_aerosol): the solver adds them, then the clouds, as it reads the gas
properties -- the same two increments in the same order, the same bits.  The SW clear solve is then the fused solve with
the aerosol as its band increment; both solves get g = NULL for the gas properties, so the g array gas optics wrote
(zeros) is not read.  Every other case keeps the reference's sequence.  AEROSOL_REQUEST = False keeps it everywhere (the
comparison route).  As for the masked fused SW solve itself, the SW route needs the checkpointed SW kernel
(rrtmgpnn_context_set_sw_kernel mode 0 or 3, the default): the class layer does not know a context's mode, and the call
raises under modes 1 and 2.
"""
import torch

from . import _lib, api, cloud_sampling
from ._lib import check, float_array, int_array
from .api import (GAUSS_DS, GAUSS_WTS, FluxesByBand, OpticalProps1scl, OpticalProps2str, SourceFuncLW, _f32dev, _p,
                  context)


# the aerosol request route may be taken (False: always aer_props.increment, the reference's sequence)
AEROSOL_REQUEST = True
# the fused LW scattering route may be taken (False: always gas optics into 2str properties, [draw_samples,] increment
# and the rescaled solver)
LW_SCAT_FUSED = True
# rte_sw may take both SW flux sets from one call of rrtmgpnn_sw_solver_2stream_clr_all (False: always the two solves)
SW_CLR_ALL_FUSED = True


def aerosol_by_request(aer_props, optical_props, kind, extents=None):
    """Are these aerosols of the fused kind for a solve on optical_props -- `kind` (OpticalProps1scl for the LW,
    OpticalProps2str for the SW), defined by band (ngpt == nband) on optical_props' bands, the same (ncol, nlay)?
    extents: (ncol, nlay) of an optical_props that is initialised but holds no arrays yet."""
    return (aer_props is not None and isinstance(aer_props, kind) and isinstance(optical_props, kind)
            and aer_props.bands_are_equal(optical_props) and aer_props.get_ngpt() == optical_props.get_nband()
            and not aer_props.gpoints_are_equal(optical_props)
            and (aer_props.get_ncol(), aer_props.get_nlay())
            == (extents or (optical_props.get_ncol(), optical_props.get_nlay())))


def _shape(a):
    return None if a is None else tuple(a.shape)


def _aer_check(aer_props, ncol, nlay, ngpt, nband, msg):
    """The reference's aerosol extent checks (:93-99, :225-231), as written there: the second one can only fire when
    ngpt == nband."""
    e = ""
    if aer_props is not None:
        if (aer_props.get_ncol(), aer_props.get_nlay()) != (ncol, nlay):
            e = msg
        if not (aer_props.get_ngpt() != ngpt or aer_props.get_ngpt() != nband):
            e = msg
    return e


def _init_like(cloud_props, k_dist, which, kind=None):
    """optical_props of cloud_props' class (or of `kind`) on k_dist's spectral grid, initialised but holding no arrays
    yet (:117-126)."""
    if kind is None:
        if isinstance(cloud_props, OpticalProps2str):
            kind = OpticalProps2str
        elif isinstance(cloud_props, OpticalProps1scl):
            kind = OpticalProps1scl
        else:
            return None, which + "_solver(...ty_optical_props_nstr...) not yet implemented"
    op = kind()
    return op, op.init(k_dist.get_band_lims_wavenumber(), k_dist.get_band_lims_gpoint())


def _alloc(op, ncol, nlay, device):
    """The arrays of an initialised optical_props (:128-137)."""
    return (op.alloc_2str if isinstance(op, OpticalProps2str) else op.alloc_1scl)(ncol, nlay, device=device)


def _alloc_like(cloud_props, k_dist, ncol, nlay, device, which):
    """optical_props of cloud_props' class on k_dist's spectral grid (:117-137)."""
    op, e = _init_like(cloud_props, k_dist, which)
    return op, e or _alloc(op, ncol, nlay, device)


def _broadband_only(fluxes):
    """Does this flux object want exactly the broadband up and down fluxes (what the dual entry writes)?"""
    if fluxes.flux_up is None or fluxes.flux_dn is None or fluxes.flux_net is not None:
        return False
    if fluxes.are_desired_gpt() or (isinstance(fluxes, FluxesByBand) and fluxes.are_desired_byband()):
        return False
    return True


def _mask_check(who, mask_bits, cloud_mask, ncol, nlay, ngpt):
    """Extents of the McICA masks rte_lw / rte_sw take, in the style of cloud_sampling._mask_args."""
    if mask_bits is not None and (_shape(mask_bits) != (ncol, nlay, (ngpt + 31) // 32)
                                  or mask_bits.element_size() != 4):
        return "%s: mask_bits is not (ncol, nlay, ceil(ngpt/32)) 32-bit words" % who
    if cloud_mask is not None and (_shape(cloud_mask) != (ncol, nlay, ngpt) or cloud_mask.element_size() != 1):
        return "%s: cloud_mask is not (ncol, nlay, ngpt) bytes" % who
    if not all(m is None or m.is_contiguous() for m in (mask_bits, cloud_mask)):
        return "%s: arrays must be contiguous" % who
    return ""


def _sampled(who, cloud_mask, cloud_props, optical_props, k_dist):
    """cloud_props (by band) sampled onto optical_props' g-points with the byte mask (draw_samples): (clouds, message)."""
    if cloud_mask is None:
        return None, ("%s: this case runs the sampled sequence (draw_samples, increment), which needs cloud_mask "
                      "(ncol, nlay, ngpt); mask_bits alone serves the fused solver entries" % who)
    smp = OpticalProps2str() if isinstance(cloud_props, OpticalProps2str) else OpticalProps1scl()
    e = smp.init(k_dist.get_band_lims_wavenumber(), k_dist.get_band_lims_gpoint())
    e = e or (smp.alloc_2str if isinstance(smp, OpticalProps2str) else smp.alloc_1scl)(
        optical_props.get_ncol(), optical_props.get_nlay(), device=optical_props.tau.device)
    e = e or cloud_sampling.draw_samples(cloud_mask, cloud_props, smp)
    return smp, e


def rte_lw(k_dist, gas_concs, p_lay, t_lay, p_lev, t_sfc, sfc_emis, cloud_props, allsky_fluxes, clrsky_fluxes,
           aer_props=None, col_dry=None, t_lev=None, inc_flux=None, n_gauss_angles=None, neural_nets=None,
           mask_bits=None, cloud_mask=None):
    """rte_lw (extensions/mo_rrtmgp_clr_all_sky.F90:46-175).  Tensors in this project's layout: p_lay, t_lay (ncol,
    nlay); p_lev, t_lev (ncol, nlay+1); t_sfc (ncol); sfc_emis (ncol, nband); inc_flux (ncol, ngpt).

    mask_bits / cloud_mask (an extension of the reference's interface, which has no sampling here): the all-sky solve
    sees cloud_props (by band) sampled per g-point with a McICA mask (cloud_sampling.sampled_mask_*), the clear solve
    is unchanged.  mask_bits, int32 (ncol, nlay, ceil(ngpt/32)), serves the library's masked dual entry
    (rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica) in the case the unmasked dual entry serves; every other case runs
    the reference's sequence with the cloud sampled first (draw_samples), which needs the byte mask cloud_mask, uint8
    (ncol, nlay, ngpt).  Given both, they must describe the same mask."""
    ncol, nlay = tuple(p_lay.shape)
    ngpt, nband = k_dist.get_ngpt(), k_dist.get_nband()
    e = _aer_check(aer_props, ncol, nlay, ngpt, nband, "rrtmpg_lw: aerosol properties inconsistently sized")
    if t_lev is not None and _shape(t_lev) != (ncol, nlay + 1):
        e = "rrtmpg_lw: t_lev inconsistently sized"
    if inc_flux is not None and _shape(inc_flux) != (ncol, ngpt):
        e = "rrtmpg_lw: incident flux inconsistently sized"
    e = e or _mask_check("rte_lw", mask_bits, cloud_mask, ncol, nlay, ngpt)
    if e:
        return e
    masked = mask_bits is not None or cloud_mask is not None
    top_at_1 = bool(p_lay[0, 0] < p_lay[0, nlay - 1])
    dev = p_lay.device
    # the route is decided on an initialised object that holds no arrays yet, so that each route allocates only the
    # arrays it uses
    optical_props, e = _init_like(cloud_props, k_dist, "lw")
    if e:
        return e
    sources = SourceFuncLW()
    e = sources.alloc(ncol, nlay, spec=k_dist, device=dev)
    if e:
        return e
    nmu = 1 if n_gauss_angles is None else int(n_gauss_angles)
    fusable = (cloud_props.bands_are_equal(optical_props)
               and not cloud_props.gpoints_are_equal(optical_props) and cloud_props.get_ngpt() == nband
               and (cloud_props.get_ncol(), cloud_props.get_nlay()) == (ncol, nlay)
               and _broadband_only(allsky_fluxes) and _broadband_only(clrsky_fluxes) and 1 <= nmu <= 4
               and _shape(sfc_emis) == (ncol, nband) and (not masked or mask_bits is not None))
    dual = fusable and isinstance(optical_props, OpticalProps1scl)
    scat = fusable and LW_SCAT_FUSED and isinstance(optical_props, OpticalProps2str)
    aer_scat = False
    if scat:
        # the gas atmosphere stays 1scl: its ssa and g are the solver's literal zeros, never arrays
        gas_1scl, e = _init_like(cloud_props, k_dist, "lw", OpticalProps1scl)
        if e:
            return e
        # aerosols of the fused kind ride the clear + all-sky entry as its aerosol request; any other kind keeps the
        # materialising sequence
        aer_scat = AEROSOL_REQUEST and aerosol_by_request(aer_props, gas_1scl, OpticalProps1scl, (ncol, nlay))
        scat = aer_props is None or aer_scat
        if scat:
            optical_props = gas_1scl
    e = _alloc(optical_props, ncol, nlay, dev)
    if e:
        return e
    e = k_dist.gas_optics(p_lay, p_lev, t_lay, t_sfc, gas_concs, optical_props, sources, col_dry=col_dry, tlev=t_lev,
                          neural_nets=neural_nets, defer_planck=dual or scat)
    if e:
        return e
    dual = dual and sources.planck_deferred is not None
    if scat and sources.planck_deferred is None:
        # (gas optics defers whenever it is asked to; the 1scl gas properties leave no sequence to fall back to)
        return "rte_lw: gas optics left the Planck sources formed; the fused scattering solve forms them itself"
    if scat:
        tlay_d, tlev_d, tsfc_d, sfc_lay = sources.planck_deferred
        ctx = context(dev.index)
        emis = _f32dev(sfc_emis, dev)
        head = (ctx.h, ngpt, nlay, ncol, int(top_at_1), nmu, float_array(GAUSS_DS[nmu]), float_array(GAUSS_WTS[nmu]),
                _p(inc_flux), _p(optical_props.tau))
        tail = (_p(sources.lay_source), nband, k_dist.get_nPlanckTemp(), _p(tlay_d), _p(tlev_d), _p(tsfc_d), sfc_lay,
                int_array(k_dist.band_lims_gpt.ravel()), k_dist.temp_ref_min, k_dist.totplnk_delta, _p(k_dist.totplnk),
                1, _p(emis))
        # clear sky = gases [+ aerosols], all sky = that + the (sampled) clouds, from one entry; the context's
        # rrtmgpnn_context_set_lw_scat_clr_all mode decides one launch or two
        if masked:
            cloud_sampling.arm_cloud_mask(ctx, ngpt, mask_bits)
        if aer_scat:
            cloud_sampling.arm_aerosol(ctx, aer_props)
        check(_lib.lib().rrtmgpnn_lw_solver_1rescl_planck_clr_all(
            *head, _p(cloud_props.tau), _p(cloud_props.ssa), _p(cloud_props.g), *tail, _p(allsky_fluxes.flux_up),
            _p(allsky_fluxes.flux_dn), _p(clrsky_fluxes.flux_up), _p(clrsky_fluxes.flux_dn)),
            "lw_solver_1rescl_planck_clr_all")
        return ""
    aer_req = dual and AEROSOL_REQUEST and aerosol_by_request(aer_props, optical_props, OpticalProps1scl)
    if aer_props is not None and not aer_req:
        e = aer_props.increment(optical_props)
        if e:
            return e
    if dual:
        tlay_d, tlev_d, tsfc_d, sfc_lay = sources.planck_deferred
        ctx = context(dev.index)
        if aer_req:
            cloud_sampling.arm_aerosol(ctx, aer_props)
        emis = _f32dev(sfc_emis, dev)
        args = (ctx.h, ngpt, nlay, ncol, int(top_at_1), nmu, float_array(GAUSS_DS[nmu]), float_array(GAUSS_WTS[nmu]),
                _p(inc_flux), _p(optical_props.tau), _p(cloud_props.tau), _p(sources.lay_source), nband,
                k_dist.get_nPlanckTemp(), _p(tlay_d), _p(tlev_d), _p(tsfc_d), sfc_lay,
                int_array(k_dist.band_lims_gpt.ravel()), k_dist.temp_ref_min, k_dist.totplnk_delta, _p(k_dist.totplnk),
                1, _p(emis), _p(allsky_fluxes.flux_up), _p(allsky_fluxes.flux_dn), _p(clrsky_fluxes.flux_up),
                _p(clrsky_fluxes.flux_dn))
        if masked:
            check(_lib.lib().rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica(*args, _p(mask_bits)),
                  "lw_solver_noscat_planck_clr_all_mcica")
        else:
            check(_lib.lib().rrtmgpnn_lw_solver_noscat_planck_clr_all(*args), "lw_solver_noscat_planck_clr_all")
        return ""
    if masked:  # the reference's sequence on the sampled cloud
        cloud_props, e = _sampled("rte_lw", cloud_mask, cloud_props, optical_props, k_dist)
        if e:
            return e
    e = api.rte_lw(optical_props, top_at_1, sources, sfc_emis, clrsky_fluxes, inc_flux=inc_flux,
                   n_gauss_angles=n_gauss_angles)
    if e:
        return e
    e = cloud_props.increment(optical_props)
    if e:
        return e
    return api.rte_lw(optical_props, top_at_1, sources, sfc_emis, allsky_fluxes, inc_flux=inc_flux,
                      n_gauss_angles=n_gauss_angles)


def rte_sw(k_dist, gas_concs, p_lay, t_lay, p_lev, mu0, sfc_alb_dir, sfc_alb_dif, cloud_props, allsky_fluxes,
           clrsky_fluxes, aer_props=None, col_dry=None, inc_flux=None, tsi_scaling=None, neural_nets=None,
           mask_bits=None, cloud_mask=None):
    """rte_sw (extensions/mo_rrtmgp_clr_all_sky.F90:177-310).  sfc_alb_dir / sfc_alb_dif: (ncol, nband) as there
    (expanded to g-points), or (ncol, ngpt) as api.rte_sw takes them; inc_flux (ncol, ngpt); tsi_scaling: the
    reference's single multiply of the incident flux.

    mask_bits / cloud_mask (an extension of the reference's interface, as in rte_lw): the clear solve as without them,
    then the all-sky solve on cloud_props (by band) sampled per g-point.  With mask_bits, 2str clouds on k_dist's
    bands, even ngpt and broadband-only all-sky fluxes that is the library's masked fused solve
    (rrtmgpnn_solver_request_cloud_mask + rrtmgpnn_sw_solver_2stream_inc: the increment switched per g-point as the
    properties are read); every other case runs draw_samples and increment first, which needs cloud_mask.

    One call (SW_CLR_ALL_FUSED): with 2str clouds by band on k_dist's bands and extents, ngpt even and at most 256, both
    flux objects broadband-only and desired and the albedos per g-point, both solves are one call of
    rrtmgpnn_sw_solver_2stream_clr_all -- masked (mask_bits) or not, aer_props by request where they qualify and
    incremented first otherwise: the same flux objects, bit for bit.  Every other case keeps the sequence above."""
    ncol, nlay = tuple(p_lay.shape)
    ngpt, nband = k_dist.get_ngpt(), k_dist.get_nband()
    e = ""
    if inc_flux is not None and tsi_scaling is not None:
        e = "rrtmpg_sw: only one of inc_flux, tsi_scaling may be supplied."
    e = _aer_check(aer_props, ncol, nlay, ngpt, nband, "rrtmpg_sw: aerosol properties inconsistently sized") or e
    if tsi_scaling is not None and tsi_scaling <= 0:
        e = "rrtmpg_sw: tsi_scaling is < 0"
    if inc_flux is not None and _shape(inc_flux) != (ncol, ngpt):
        e = "rrtmpg_sw: incident flux inconsistently sized"
    e = e or _mask_check("rte_sw", mask_bits, cloud_mask, ncol, nlay, ngpt)
    if e:
        return e
    masked = mask_bits is not None or cloud_mask is not None
    top_at_1 = bool(p_lay[0, 0] < p_lay[0, nlay - 1])
    dev = p_lay.device
    optical_props, e = _alloc_like(cloud_props, k_dist, ncol, nlay, dev, "sw")
    if e:
        return e
    toa_flux = torch.empty((ncol, ngpt), dtype=torch.float32, device=dev)
    e = k_dist.gas_optics(p_lay, p_lev, t_lay, gas_concs, optical_props, toa_flux, col_dry=col_dry,
                          neural_nets=neural_nets)
    if e:
        return e
    if inc_flux is not None:
        toa_flux.copy_(_f32dev(inc_flux, dev))
    if tsi_scaling is not None:
        toa_flux.mul_(float(tsi_scaling))
    ctx = context(dev.index)
    albs = []
    for a in (sfc_alb_dir, sfc_alb_dif):
        a = _f32dev(a, dev)
        if tuple(a.shape) == (ncol, nband) and nband != ngpt:
            g = torch.empty((ncol, ngpt), dtype=torch.float32, device=dev)
            check(_lib.lib().rrtmgpnn_expand_band_to_gpt(ctx.h, nband, ngpt, ncol,
                                                         int_array(k_dist.band_lims_gpt.ravel()), _p(a), _p(g)),
                  "expand")
            a = g
        albs.append(a)
    mu0 = _f32dev(mu0, dev)
    fused = False
    if masked:
        fused = (mask_bits is not None and isinstance(optical_props, OpticalProps2str) and ngpt % 2 == 0
                 and cloud_props.bands_are_equal(optical_props) and not cloud_props.gpoints_are_equal(optical_props)
                 and cloud_props.get_ngpt() == nband
                 and (cloud_props.get_ncol(), cloud_props.get_nlay()) == (ncol, nlay)
                 and not allsky_fluxes.are_desired_gpt()
                 and not (isinstance(allsky_fluxes, FluxesByBand) and allsky_fluxes.are_desired_byband())
                 and allsky_fluxes.are_desired()
                 and all(_shape(a) == (ncol, ngpt) for a in albs))
    f = lambda t: t if t is not None else torch.empty((ncol, nlay + 1), dtype=torch.float32, device=dev)  # noqa: E731
    lims = int_array(k_dist.band_lims_gpt.ravel())
    broadband = lambda fl: (fl.are_desired() and not fl.are_desired_gpt()  # noqa: E731
                            and not (isinstance(fl, FluxesByBand) and fl.are_desired_byband()))
    one_call = (SW_CLR_ALL_FUSED and (not masked or mask_bits is not None)
                and isinstance(optical_props, OpticalProps2str) and isinstance(cloud_props, OpticalProps2str)
                and ngpt % 2 == 0 and ngpt <= 256
                and cloud_props.bands_are_equal(optical_props) and not cloud_props.gpoints_are_equal(optical_props)
                and cloud_props.get_ngpt() == nband
                and (cloud_props.get_ncol(), cloud_props.get_nlay()) == (ncol, nlay)
                and broadband(allsky_fluxes) and broadband(clrsky_fluxes)
                and all(_shape(a) == (ncol, ngpt) for a in albs))
    if one_call:
        # aerosols by request where the solver's aerosol instances take them (band-pair layout: mode 2 of
        # rrtmgpnn_context_set_sw_clr_all runs the single-sky aerosol instance), incremented into the gas properties
        # otherwise; the gas g is read only in that second case
        by_req = (AEROSOL_REQUEST and aerosol_by_request(aer_props, optical_props, OpticalProps2str)
                  and all((int(lo) - 1) % 2 == 0 for lo in k_dist.band_lims_gpt[:, 0]))
        if aer_props is not None and not by_req:
            e = aer_props.increment(optical_props)
            if e:
                return e
        up, dn, dr = f(allsky_fluxes.flux_up), f(allsky_fluxes.flux_dn), f(allsky_fluxes.flux_dn_dir)
        upc, dnc, drc = f(clrsky_fluxes.flux_up), f(clrsky_fluxes.flux_dn), f(clrsky_fluxes.flux_dn_dir)
        if by_req:
            cloud_sampling.arm_aerosol(ctx, aer_props)
        if mask_bits is not None:
            cloud_sampling.arm_cloud_mask(ctx, ngpt, mask_bits)
        check(_lib.lib().rrtmgpnn_sw_solver_2stream_clr_all(
            ctx.h, ngpt, nlay, ncol, int(top_at_1), _p(toa_flux), None, _p(optical_props.tau), _p(optical_props.ssa),
            None if (by_req or aer_props is None) else _p(optical_props.g), nband, lims, _p(cloud_props.tau),
            _p(cloud_props.ssa), _p(cloud_props.g), _p(mu0), _p(albs[0]), _p(albs[1]), _p(up), _p(dn), _p(dr), _p(upc),
            _p(dnc), _p(drc)), "sw_solver_2stream_clr_all")
        if allsky_fluxes.flux_net is not None:
            torch.sub(dn, up, out=allsky_fluxes.flux_net)
        if clrsky_fluxes.flux_net is not None:
            torch.sub(dnc, upc, out=clrsky_fluxes.flux_net)
        return ""
    # aerosols by request: the masked fused solve is taken and the clear fluxes are broadband ones as well
    # (band-pair layout: the solver's aerosol instances need every band to start at an odd 1-based g-point)
    aer_req = (fused and AEROSOL_REQUEST and aerosol_by_request(aer_props, optical_props, OpticalProps2str)
               and all((int(lo) - 1) % 2 == 0 for lo in k_dist.band_lims_gpt[:, 0])
               and not clrsky_fluxes.are_desired_gpt() and clrsky_fluxes.are_desired()
               and not (isinstance(clrsky_fluxes, FluxesByBand) and clrsky_fluxes.are_desired_byband()))
    if aer_props is not None and not aer_req:
        e = aer_props.increment(optical_props)
        if e:
            return e
    if aer_req:
        # the clear solve: the fused solve with the aerosol as its band increment; the gas g (0) is never read
        up, dn, dr = f(clrsky_fluxes.flux_up), f(clrsky_fluxes.flux_dn), f(clrsky_fluxes.flux_dn_dir)
        check(_lib.lib().rrtmgpnn_sw_solver_2stream_inc(
            ctx.h, ngpt, nlay, ncol, int(top_at_1), _p(toa_flux), None, _p(optical_props.tau), _p(optical_props.ssa),
            None, nband, lims, _p(aer_props.tau), _p(aer_props.ssa), _p(aer_props.g), _p(mu0), _p(albs[0]),
            _p(albs[1]), _p(up), _p(dn), _p(dr)), "sw_solver_2stream_inc")
        if clrsky_fluxes.flux_net is not None:
            torch.sub(dn, up, out=clrsky_fluxes.flux_net)
    else:
        e = api.rte_sw(optical_props, top_at_1, mu0, toa_flux, albs[0], albs[1], clrsky_fluxes)
        if e:
            return e
    if masked:
        if fused:
            up, dn, dr = f(allsky_fluxes.flux_up), f(allsky_fluxes.flux_dn), f(allsky_fluxes.flux_dn_dir)
            if aer_req:
                cloud_sampling.arm_aerosol(ctx, aer_props)
            cloud_sampling.arm_cloud_mask(ctx, ngpt, mask_bits)
            check(_lib.lib().rrtmgpnn_sw_solver_2stream_inc(
                ctx.h, ngpt, nlay, ncol, int(top_at_1), _p(toa_flux), None, _p(optical_props.tau),
                _p(optical_props.ssa), None if aer_req else _p(optical_props.g), nband, lims,
                _p(cloud_props.tau), _p(cloud_props.ssa), _p(cloud_props.g), _p(mu0), _p(albs[0]), _p(albs[1]),
                _p(up), _p(dn), _p(dr)), "sw_solver_2stream_inc")
            if allsky_fluxes.flux_net is not None:
                torch.sub(dn, up, out=allsky_fluxes.flux_net)
            return ""
        cloud_props, e = _sampled("rte_sw", cloud_mask, cloud_props, optical_props, k_dist)
        if e:
            return e
    e = cloud_props.increment(optical_props)
    if e:
        return e
    return api.rte_sw(optical_props, top_at_1, mu0, toa_flux, albs[0], albs[1], allsky_fluxes)
