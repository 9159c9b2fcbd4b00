"""mo_compute_bc's compute_bc (extensions/mo_compute_bc.F90:43-210) on torch device tensors, over
rrtmgpnn_compute_bc_lw / _sw.

The upper boundary condition from one thin isothermal layer between the gas optics' minimum pressure and the model's
top: flux_bc (ncol, ngpt) -- the reference's (ngpt, ncol) bytes, as every tensor of the class layer -- is the spectrally
resolved downward flux at that layer's bottom, to be passed as inc_flux.  Error strings and the order of the checks are
the reference's; like the other class-level functions it RETURNS the message ('' on success).

Units (include/rrtmgpnn.h): the reference's LW flux_bc is a radiance, because its rte_lw call uses one angle; that is the
default here.  as_flux=True multiplies by the solver's 2 pi w, which is what rte_lw's inc_flux means.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, float_array, int_array, ptr_array
from .api import GAUSS_DS, GAUSS_WTS, _p, context
from .data import spacing


def pressure_check(plev_top, press_min):
    """The reference's test (:110-114) on the host values plev(:, top_lay): '' or its error string."""
    pmin = np.float32(press_min)
    if np.any(np.asarray(plev_top, np.float32) <= pmin + np.float32(2.0) * spacing(pmin)):
        return "compute_bc: pressures are too close to (or less than) min in gas optics "
    return ""


def gas_arguments(net, gas_concs):
    """(gas_conc, gas_ndims, '') of the C entries for a network's inputs, or (None, None, message)."""
    ptrs, nds = [], []
    for k, name in enumerate(net.input_names):
        if k < 2 or name not in gas_concs.concs:
            ptrs.append(None)
            nds.append(2)
            continue
        ptrs.append(gas_concs.concs[name].data_ptr())
        nds.append(gas_concs.ndims(name))
    if net.input_names[2] not in gas_concs.concs or net.input_names[3] not in gas_concs.concs:
        return None, None, "compute_nn_inputs: gas " + net.input_names[2] + "/" + net.input_names[3] + " not found"
    if "h2o" not in gas_concs.concs:
        return None, None, "gas_optics(): h2o concentration is required"
    return ptrs, nds, ""


def compute_bc(k_dist, play, plev, tlay, gas_concs, flux_bc, mu0=None, as_flux=False, neural_nets=None):
    """compute_bc(k_dist, play, plev, tlay, gas_concs, flux_bc, mu0): LW or SW by k_dist.source_is_internal(), one Gauss
    angle as the reference's rte_lw call.  neural_nets: the gas-optics networks ([abs, pfrac] or [both]; [abs, ray]),
    as GasOpticsRRTMGP.gas_optics takes them."""
    ncol, nlay = play.shape
    ngpt = k_dist.get_ngpt()
    if tuple(plev.shape) != (ncol, nlay + 1):
        return "compute_bc: array plev has wrong dimensions"
    if tuple(tlay.shape) != (ncol, nlay):
        return "compute_bc: array tlay has wrong dimensions"
    if mu0 is not None and mu0.numel() != ncol:
        return "compute bc: array mu0 has wrong dimensions"
    top_at_1 = bool(float(play[0, 0]) < float(play[0, nlay - 1]))
    top = 0 if top_at_1 else nlay - 1  # top_lay - 1
    e = pressure_check(plev[:, top].cpu().numpy(), k_dist.get_press_min())
    if e:
        return e
    if not k_dist.source_is_internal() and mu0 is None:
        return "compute_bc: have to supply mu0 for solar calculations"
    if neural_nets is None:
        return "gas_optics(): the lookup-table branch is not available (k-distribution files missing); pass neural_nets"
    if tuple(flux_bc.shape) != (ncol, ngpt):
        return "compute_bc: array flux_bc has wrong dimensions"
    net = neural_nets[0]
    ptrs, nds, e = gas_arguments(net, gas_concs)
    if e:
        return e
    ctx = context(play.device.index)
    L = _lib.lib()
    nets = ptr_array([n.h.value for n in neural_nets])
    head = (ctx.h, ncol, nlay, ngpt, net.dims[0], int(top_at_1), float(k_dist.get_press_min()), _p(play), _p(plev),
            _p(tlay), _p(gas_concs.concs["h2o"]), ptr_array(ptrs), int_array(nds), nets)
    if k_dist.source_is_internal():
        check(L.rrtmgpnn_compute_bc_lw(
            *head, len(neural_nets), k_dist.get_nband(), k_dist.get_nPlanckTemp(),
            int_array(k_dist.band_lims_gpt.ravel()), k_dist.temp_ref_min, k_dist.totplnk_delta, _p(k_dist.totplnk),
            1, float_array(GAUSS_DS[1]), float_array(GAUSS_WTS[1]), int(bool(as_flux)), _p(flux_bc)), "compute_bc_lw")
        return ""
    src = torch.as_tensor(np.ascontiguousarray(k_dist.solar_source, np.float32), device=play.device)
    check(L.rrtmgpnn_compute_bc_sw(*head, _p(src), _p(mu0), _p(flux_bc)), "compute_bc_sw")
    return ""
