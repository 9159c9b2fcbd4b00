"""mo_cloud_sampling (extensions/cloud_optics/mo_cloud_sampling.F90): McICA sampling of band-resolved cloud optical
properties, on the optical-props classes of api.py.

  sampled_mask_max_ran   :125-192   maximum-random overlap
  sampled_mask_exp_ran   :200-285   exponential-random overlap
  draw_samples           :36-120    the mask applied to the band properties (apply_cloud_mask, :291-307)

Functions RETURN the reference's error message ('' on success).  The extension predates this fork's layout: here,
as torch tensors in C order, randoms and cloud_mask are (ncol, nlay, ngpt), cloud_frac (ncol, nlay) and overlap_param
(ncol, nlay-1).  cloud_mask is a uint8 (or bool) tensor of 0 / 1; mask_bits, an int32 tensor (ncol, nlay,
ceil(ngpt / 32)), is the packed form the solvers take (rrtmgpnn_solver_request_cloud_mask): bit g % 32 of word g / 32.
Random numbers are the caller's, as in the reference; the *_seeded functions and mcica_randoms (no reference
counterpart) draw them on the device from (seed, stream, col0) with Philox4x32-10 (include/rrtmgpnn.h has the counter
layout): a column's numbers depend on the seed, the stream, its global index col0 + icol, the layer and the g-point
alone.  The value checks (cloud_frac in [0, 1], overlap_param in
[-1, 1]) follow api.check_values (rte_config_checks), as the other value checks of this layer do; extents are always
checked.  Quirk: a clear layer between cloudy ones is false in both masks; the reference's exp_ran
leaves it unassigned.
"""
from . import _lib, api
from ._lib import check, int_array
from .api import OpticalProps1scl, OpticalProps2str, _p, context


def _mask_args(who, randoms, cloud_frac, cloud_mask, mask_bits):
    """The extents checks both mask functions share, with the reference's messages (exp_ran's carry max_ran's prefix:
    the reference copied them, :221-238)."""
    if randoms.dim() != 3 or cloud_frac.dim() != 2:
        return "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and cloud_frac(ncol,nlay) are inconsistent"
    ncol, nlay, ngpt = randoms.shape
    if tuple(cloud_frac.shape) != (ncol, nlay):
        return "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and cloud_frac(ncol,nlay) are inconsistent"
    if cloud_mask is None and mask_bits is None:
        return "%s: neither cloud_mask nor mask_bits given" % who
    if cloud_mask is not None and (tuple(cloud_mask.shape) != (ncol, nlay, ngpt) or cloud_mask.element_size() != 1):
        return "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and cloud_mask(ncol,nlay,ngpt) are inconsistent"
    if mask_bits is not None and (tuple(mask_bits.shape) != (ncol, nlay, (ngpt + 31) // 32)
                                  or mask_bits.element_size() != 4):
        return "%s: mask_bits is not (ncol, nlay, ceil(ngpt/32)) 32-bit words" % who
    return ""


def _frac_check(cloud_frac):
    if api.check_values and (bool((cloud_frac > 1).any()) or bool((cloud_frac < 0).any())):
        return "sampled_mask_max_ran: cloud fraction values out of range [0,1]"
    return ""


def _contig(*ts):
    return all(t is None or t.is_contiguous() for t in ts)


def sampled_mask_max_ran(randoms, cloud_frac, cloud_mask=None, mask_bits=None):
    """sampled_mask_max_ran(randoms, cloud_frac, cloud_mask) (:125-192); mask_bits: also / instead the packed mask."""
    e = _mask_args("sampled_mask_max_ran", randoms, cloud_frac, cloud_mask, mask_bits) or _frac_check(cloud_frac)
    if e:
        return e
    if not _contig(randoms, cloud_frac, cloud_mask, mask_bits):
        return "sampled_mask_max_ran: arrays must be contiguous"
    ncol, nlay, ngpt = randoms.shape
    ctx = context(randoms.device.index)
    check(_lib.lib().rrtmgpnn_sampled_mask_max_ran(ctx.h, ngpt, nlay, ncol, _p(randoms), _p(cloud_frac),
                                                   _p(cloud_mask), _p(mask_bits)), "sampled_mask_max_ran")
    return ""


def sampled_mask_exp_ran(randoms, cloud_frac, overlap_param, cloud_mask=None, mask_bits=None):
    """sampled_mask_exp_ran(randoms, cloud_frac, overlap_param, cloud_mask) (:200-285)."""
    e = _mask_args("sampled_mask_exp_ran", randoms, cloud_frac, cloud_mask, mask_bits)
    if e and "cloud_frac(ncol,nlay)" in e:
        return e
    ncol, nlay, ngpt = randoms.shape
    if overlap_param.dim() != 2 or tuple(overlap_param.shape) != (ncol, nlay - 1):
        return "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and overlap_param(ncol,nlay-1) are inconsistent"
    e = e or _frac_check(cloud_frac)
    if e:
        return e
    if api.check_values and (bool((overlap_param > 1).any()) or bool((overlap_param < -1).any())):
        return "sampled_mask_max_ran: overlap_param values out of range [-1,1]"
    if not _contig(randoms, cloud_frac, overlap_param, cloud_mask, mask_bits):
        return "sampled_mask_exp_ran: arrays must be contiguous"
    ctx = context(randoms.device.index)
    check(_lib.lib().rrtmgpnn_sampled_mask_exp_ran(ctx.h, ngpt, nlay, ncol, _p(randoms), _p(cloud_frac),
                                                   _p(overlap_param) if nlay > 1 else None, _p(cloud_mask),
                                                   _p(mask_bits)), "sampled_mask_exp_ran")
    return ""


def _rng(ctx, seed, stream, col0):
    """The context's 4-word device buffer {seed low, seed high, stream, col0}, refilled (rrtmgpnn_mcica_rng_set: on the
    context's stream, after the work already issued there, and complete on return)."""
    import torch
    buf = getattr(ctx, "_mcica_rng", None)
    if buf is None:
        buf = ctx._mcica_rng = torch.zeros(4, dtype=torch.int32, device=torch.device("cuda", ctx.device))
    check(_lib.lib().rrtmgpnn_mcica_rng_set(ctx.h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF,
                                            int(col0) & 0xFFFFFFFF, _p(buf)), "mcica_rng_set")
    return buf


def mcica_randoms(seed, stream, col0, randoms):
    """Fill randoms (ncol, nlay, ngpt) float32 with the numbers the *_seeded mask functions draw for the columns
    col0 .. col0 + ncol - 1 (modulo 2^32)."""
    if randoms.dim() != 3 or randoms.element_size() != 4 or not randoms.is_floating_point():
        return "mcica_randoms: randoms is not a float32 (ncol, nlay, ngpt) array"
    if not randoms.is_contiguous():
        return "mcica_randoms: arrays must be contiguous"
    ncol, nlay, ngpt = randoms.shape
    ctx = context(randoms.device.index)
    check(_lib.lib().rrtmgpnn_mcica_randoms(ctx.h, ngpt, nlay, ncol, _p(_rng(ctx, seed, stream, col0)), _p(randoms)),
          "mcica_randoms")
    return ""


def _seeded_extents(who, cloud_frac, cloud_mask, mask_bits, ngpt):
    """_mask_args without randoms, with the reference's messages: (message, (ncol, nlay, ngpt)).  ngpt is cloud_mask's
    last extent; with mask_bits alone it must be given (the words round it up)."""
    pre = "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and "
    if cloud_mask is None and mask_bits is None:
        return "%s: neither cloud_mask nor mask_bits given" % who, None
    if cloud_frac.dim() != 2:
        return pre + "cloud_frac(ncol,nlay) are inconsistent", None
    ncol, nlay = cloud_frac.shape
    if cloud_mask is not None:
        if cloud_mask.dim() != 3 or tuple(cloud_mask.shape[:2]) != (ncol, nlay) or cloud_mask.element_size() != 1 \
                or (ngpt is not None and int(ngpt) != cloud_mask.shape[2]):
            return pre + "cloud_mask(ncol,nlay,ngpt) are inconsistent", None
        ngpt = cloud_mask.shape[2]
    elif ngpt is None:
        return "%s: ngpt is needed with mask_bits alone" % who, None
    ngpt = int(ngpt)
    if mask_bits is not None and (tuple(mask_bits.shape) != (ncol, nlay, (ngpt + 31) // 32)
                                  or mask_bits.element_size() != 4):
        return "%s: mask_bits is not (ncol, nlay, ceil(ngpt/32)) 32-bit words" % who, None
    return "", (ncol, nlay, ngpt)


def _seeded(who, exp_ran, seed, stream, col0, cloud_frac, overlap_param, cloud_mask, mask_bits, ngpt):
    e, ext = _seeded_extents(who, cloud_frac, cloud_mask, mask_bits, ngpt)
    if e:
        return e
    ncol, nlay, ngpt = ext
    if exp_ran and (overlap_param.dim() != 2 or tuple(overlap_param.shape) != (ncol, nlay - 1)):
        return "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and overlap_param(ncol,nlay-1) are inconsistent"
    e = _frac_check(cloud_frac)
    if e:
        return e
    if exp_ran and api.check_values and (bool((overlap_param > 1).any()) or bool((overlap_param < -1).any())):
        return "sampled_mask_max_ran: overlap_param values out of range [-1,1]"
    if not _contig(cloud_frac, overlap_param, cloud_mask, mask_bits):
        return "%s: arrays must be contiguous" % who
    ctx = context(cloud_frac.device.index)
    rng = _rng(ctx, seed, stream, col0)
    L = _lib.lib()
    if exp_ran:
        check(L.rrtmgpnn_sampled_mask_exp_ran_seeded(ctx.h, ngpt, nlay, ncol, _p(rng), _p(cloud_frac),
                                                     _p(overlap_param) if nlay > 1 else None, _p(cloud_mask),
                                                     _p(mask_bits)), who)
    else:
        check(L.rrtmgpnn_sampled_mask_max_ran_seeded(ctx.h, ngpt, nlay, ncol, _p(rng), _p(cloud_frac), _p(cloud_mask),
                                                     _p(mask_bits)), who)
    return ""


def sampled_mask_max_ran_seeded(seed, stream, col0, cloud_frac, cloud_mask=None, mask_bits=None, ngpt=None):
    """sampled_mask_max_ran with the random numbers drawn in the kernel from (seed, stream, col0); ngpt: the g-point
    count when only mask_bits is given."""
    return _seeded("sampled_mask_max_ran_seeded", False, seed, stream, col0, cloud_frac, None, cloud_mask, mask_bits,
                   ngpt)


def sampled_mask_exp_ran_seeded(seed, stream, col0, cloud_frac, overlap_param, cloud_mask=None, mask_bits=None,
                                ngpt=None):
    """sampled_mask_exp_ran with the random numbers drawn in the kernel from (seed, stream, col0)."""
    return _seeded("sampled_mask_exp_ran_seeded", True, seed, stream, col0, cloud_frac, overlap_param, cloud_mask,
                   mask_bits, ngpt)


def draw_samples(cloud_mask, clouds, clouds_sampled):
    """draw_samples(cloud_mask, clouds, clouds_sampled) (:36-120): clouds defined by band, clouds_sampled by g-point."""
    if not clouds.is_initialized():
        return "draw_samples: cloud optical properties are not initialized"
    if not clouds_sampled.is_initialized():
        return "draw_samples: sampled cloud optical properties are not initialized"
    in1, in2 = isinstance(clouds, OpticalProps1scl), isinstance(clouds, OpticalProps2str)
    out1, out2 = isinstance(clouds_sampled, OpticalProps1scl), isinstance(clouds_sampled, OpticalProps2str)
    if in1 and not out1:
        return "draw_samples: by-band and sampled cloud properties need to be the same variable type"
    if not in1 and not in2:
        return "draw_samples: sampling isn't implemented yet for ty_optical_props_nstr"
    if not clouds.bands_are_equal(clouds_sampled):
        return "draw_samples: by-band and sampled cloud properties spectral structure is different"
    ncol, nlay, nbnd = clouds.get_ncol(), clouds.get_nlay(), clouds.get_nband()
    ngpt = clouds_sampled.get_ngpt()
    if tuple(cloud_mask.shape) != (ncol, nlay, ngpt) or cloud_mask.element_size() != 1:
        return "draw_samples: cloud mask and cloud optical properties have different ncol and/or nlay"
    if (clouds_sampled.get_ncol(), clouds_sampled.get_nlay()) != (ncol, nlay):
        return "draw_samples: sampled/unsampled cloud optical properties have different ncol and/or nlay"
    if in2 and not out2:  # "2str is checked at assignment" (:60-62, :116-117)
        return "draw_samples: by-band and sampled cloud properties need to be the same variable type"
    if clouds.tau.shape[-1] != nbnd:
        return "draw_samples: cloud optical properties are not defined by band"
    two = in2
    ctx = context(clouds.tau.device.index)
    check(_lib.lib().rrtmgpnn_draw_samples(
        ctx.h, ngpt, nlay, ncol, nbnd, int_array(clouds_sampled.band_lims_gpt.ravel()), _p(cloud_mask),
        _p(clouds.tau), _p(clouds.ssa) if two else None, _p(clouds.g) if two else None, _p(clouds_sampled.tau),
        _p(clouds_sampled.ssa) if two else None, _p(clouds_sampled.g) if two else None), "draw_samples")
    return ""


def arm_cloud_mask(ctx, ngpt, mask_bits):
    """Arm the packed mask mask_bits (ncol, nlay, ceil(ngpt / 32)) for the next solver call on ctx
    (rrtmgpnn_solver_request_cloud_mask); that call clears it.  mask_bits None disarms."""
    if mask_bits is None:
        check(_lib.lib().rrtmgpnn_solver_request_cloud_mask(ctx.h, 0, 0, 0, None), "solver_request_cloud_mask")
        return
    ncol, nlay, _ = mask_bits.shape
    check(_lib.lib().rrtmgpnn_solver_request_cloud_mask(ctx.h, int(ngpt), nlay, ncol, _p(mask_bits)),
          "solver_request_cloud_mask")


def arm_aerosol(ctx, aer_props):
    """Arm aer_props (by band: tau (ncol, nlay, nbnd), with ssa and g when 2str) as the aerosol increment of the next
    solver call on ctx (rrtmgpnn_solver_request_aerosol), which applies it in front of its own band increment and
    clears it.  aer_props None disarms."""
    if aer_props is None:
        check(_lib.lib().rrtmgpnn_solver_request_aerosol(ctx.h, 0, 0, 0, None, None, None), "solver_request_aerosol")
        return
    ncol, nlay, nbnd = aer_props.tau.shape
    check(_lib.lib().rrtmgpnn_solver_request_aerosol(
        ctx.h, nbnd, nlay, ncol, _p(aer_props.tau), _p(getattr(aer_props, "ssa", None)),
        _p(getattr(aer_props, "g", None))), "solver_request_aerosol")


def arm_sfc_byband(ctx, band_lims_gpt, sfc_up, sfc_dn, sfc_dir=None):
    """Arm the by-band fluxes at the surface, outputs (ncol, nband) over band_lims_gpt (nband, 2; 1-based, inclusive: the
    call's own increment bands), for the next solver call on ctx (rrtmgpnn_solver_request_sfc_byband); that call clears
    it.  Taken by the fused shortwave call (api.rte_sw with band_inc=) beside arm_cloud_mask, arm_aerosol or both, also
    with active=; the values are the surface level of the by-band fluxes of the same problem.  An output that is None
    is not written; all three None disarm."""
    outs = [o for o in (sfc_up, sfc_dn, sfc_dir) if o is not None]
    if not outs:
        check(_lib.lib().rrtmgpnn_solver_request_sfc_byband(ctx.h, 0, None, 0, None, None, None), "solver_request_sfc_byband")
        return
    lims = [int(v) for pair in band_lims_gpt for v in pair]
    ncol, nbnd = outs[0].shape
    if nbnd != len(lims) // 2 or any(tuple(o.shape) != (ncol, nbnd) for o in outs):
        raise ValueError("arm_sfc_byband: the outputs are (ncol, nband) on the bands of band_lims_gpt")
    check(_lib.lib().rrtmgpnn_solver_request_sfc_byband(
        ctx.h, nbnd, int_array(lims), ncol, _p(sfc_up), _p(sfc_dn), _p(sfc_dir)), "solver_request_sfc_byband")


def arm_cloud_mask_byband(ctx, ngpt, mask_bits, band_lims_gpt, bnd_up, bnd_dn, bnd_dir=None):
    """Arm the packed mask mask_bits (ncol, nlay, ceil(ngpt / 32)) together with by-band outputs (ncol, nlay + 1, nbnd)
    over band_lims_gpt (nbnd, 2; 1-based, inclusive) for the next solver call on ctx
    (rrtmgpnn_solver_request_byband_mcica); that call clears the pair.  An output that is None is not written; bnd_dir
    is a shortwave output."""
    lims = [int(v) for pair in band_lims_gpt for v in pair]
    ncol, nlay, _ = mask_bits.shape
    check(_lib.lib().rrtmgpnn_solver_request_byband_mcica(
        ctx.h, len(lims) // 2, int_array(lims), _p(bnd_up), _p(bnd_dn), _p(bnd_dir), int(ngpt), nlay, ncol,
        _p(mask_bits)), "solver_request_byband_mcica")
