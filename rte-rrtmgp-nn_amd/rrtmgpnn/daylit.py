"""Daylit columns: device-side column compaction for the shortwave chain.

The RFMIP driver marks the columns where the sun is up (usecol, examples/rfmip-clear-sky/rrtmgp_rfmip_sw.F90:285-287),
solves the others with mu0 = 1 (:433) and zeroes their fluxes afterwards (:456-463).  A host model compacts its block to
the daylit columns instead:

    pl = daylit.plan(sza, daylit.KIND_LT, daylit.SZA_BOUND)     # idx, slot, nday: device tensors
    daylit.gather(pl, [(play, d_play), (tlay, d_tlay), ...])     # row idx[j] of src -> row j of dst, j < nday
    ... rrtmgpnn_gas_optics_sw_nn_active(..., pl.nday) on the dense arrays ...
    api.rte_sw(dense_atmos, ..., dense_fluxes, active=pl)        # or daylit.arm_active_columns(ctx, pl) + a C entry
    daylit.scatter(pl, [(d_flux_up, flux_up), ...])              # zeros at night

With McICA-sampled clouds the packed mask is sampled for the compacted columns directly, from the full-extent cloud
fraction, overlap parameter and random numbers (nothing is gathered for it), and armed beside the count:

    daylit.sampled_mask_active(pl, randoms, cloud_frac, mask_bits, overlap_param)    # or sampled_mask_seeded_active
    cloud_sampling.arm_cloud_mask(ctx, ngpt, mask_bits)                               # and arm_aerosol(ctx, dense_aer)
    api.rte_sw(dense_atmos, ..., dense_fluxes, active=pl, band_inc=dense_clouds_by_band)

nday never leaves the device: the network and solver kernels read it, so the sequence can be captured in a hipGraph
once and replayed for any day / night pattern.  pipeline.ClearSkyStep(daylit=True) is this sequence as a step, and
ClearSkyStep(clouds=, mcica={..., "daylit": True}) the one with sampled clouds (and aerosols).
plan_host is the numpy restatement the tests compare with."""
import numpy as np

from . import _lib
from ._lib import check, int_array, ptr_array

KIND_LT, KIND_GT = 0, 1  # daylit iff v < bound (the driver's form on sza) / v > bound (callers that hold mu0)
# usecol = sza < 90 - 2 spacing(90) (rrtmgp_rfmip_sw.F90:285-287), spacing(90.) = 2^-17 in working precision
SZA_BOUND = float(np.float32(90.0) - np.float32(2.0) * np.spacing(np.float32(90.0)))
MAX_GATHER, MAX_SCATTER = 16, 6


def plan_host(values, kind, bound):
    """(idx, slot, nday) of rrtmgpnn_daylit_plan in numpy: the daylit columns in increasing order, then the night columns
    in increasing order; the dense position of each daylit column, -1 at night; the count.  A NaN is night."""
    if kind not in (KIND_LT, KIND_GT):
        raise ValueError("plan_host: kind must be 0 (v < bound) or 1 (v > bound)")
    v = np.asarray(values, np.float32).ravel()
    b = np.float32(bound)
    with np.errstate(invalid="ignore"):
        day = (v < b) if kind == KIND_LT else (v > b)
    d, n = np.flatnonzero(day), np.flatnonzero(~day)
    idx = np.concatenate([d, n]).astype(np.int32)
    slot = np.full(v.size, -1, np.int32)
    slot[d] = np.arange(d.size, dtype=np.int32)
    return idx, slot, int(d.size)


class Plan:
    """idx (ncol), slot (ncol) and nday (1): int32 device tensors (rrtmgpnn_daylit_plan)."""

    def __init__(self, idx, slot, nday):
        self.idx, self.slot, self.nday = idx, slot, nday
        self.ncol = int(idx.numel())


def _ctx(device):
    from .api import context
    return context(device.index)


def plan(values, kind=KIND_LT, bound=SZA_BOUND, out=None):
    """The daylit columns of `values` (a float32 device tensor of ncol elements) as a Plan; out: a Plan to refill."""
    import torch
    if values.dtype != torch.float32 or not values.is_contiguous():
        raise ValueError("daylit.plan: values must be a contiguous float32 device tensor")
    n, dev = int(values.numel()), values.device
    pl = out or Plan(*(torch.zeros(k, dtype=torch.int32, device=dev) for k in (n, n, 1)))
    if pl.ncol != n:
        raise ValueError("daylit.plan: the plan to refill holds %d columns, values %d" % (pl.ncol, n))
    check(_lib.lib().rrtmgpnn_daylit_plan(_ctx(dev).h, n, values.data_ptr(), int(kind), float(bound), pl.idx.data_ptr(),
                                          pl.slot.data_ptr(), pl.nday.data_ptr()), "daylit_plan")
    return pl


def _table(pl, pairs, who, limit):
    import torch
    pairs = list(pairs)
    if not 1 <= len(pairs) <= limit:
        raise ValueError("daylit.%s: 1..%d (source, destination) pairs" % (who, limit))
    rows = []
    for a, b in pairs:
        if a.dtype != torch.float32 or b.dtype != torch.float32 or not a.is_contiguous() or not b.is_contiguous():
            raise ValueError("daylit.%s: contiguous float32 device tensors" % who)
        if a.shape != b.shape or a.shape[0] != pl.ncol:
            raise ValueError("daylit.%s: each pair has one shape, (ncol, ...)" % who)
        rows.append(int(a.numel() // max(pl.ncol, 1)))
    return (ptr_array([a.data_ptr() for a, _ in pairs]), ptr_array([b.data_ptr() for _, b in pairs]), int_array(rows),
            len(pairs), pairs[0][0].device)


def gather(pl, pairs):
    """For each (src, dst) pair of (ncol, ...) tensors: row idx[j] of src to row j of dst for j < nday, one launch."""
    src, dst, rows, n, dev = _table(pl, pairs, "gather", MAX_GATHER)
    check(_lib.lib().rrtmgpnn_gather_columns(_ctx(dev).h, pl.ncol, n, src, dst, rows, pl.idx.data_ptr(),
                                             pl.nday.data_ptr()), "gather_columns")


def scatter(pl, pairs):
    """For each (dense, out) pair of (ncol, ...) tensors: column i of out from row slot[i] of dense, zeros at night."""
    src, dst, rows, n, dev = _table(pl, pairs, "scatter", MAX_SCATTER)
    check(_lib.lib().rrtmgpnn_scatter_columns(_ctx(dev).h, pl.ncol, n, src, dst, rows, pl.slot.data_ptr()),
          "scatter_columns")


def _compact_mask(who, pl, src, cloud_frac, overlap_param, mask_bits, ngpt, ctx):
    import torch
    exp_ran = overlap_param is not None
    if cloud_frac.dim() != 2 or cloud_frac.shape[0] != pl.ncol or cloud_frac.dtype != torch.float32:
        raise ValueError("daylit.%s: cloud_frac is a float32 (ncol, nlay) tensor of the plan's ncol" % who)
    ncol, nlay = cloud_frac.shape
    if exp_ran and tuple(overlap_param.shape) != (ncol, nlay - 1):
        raise ValueError("daylit.%s: overlap_param is (ncol, nlay - 1)" % who)
    if tuple(mask_bits.shape) != (ncol, nlay, (int(ngpt) + 31) // 32) or mask_bits.element_size() != 4:
        raise ValueError("daylit.%s: mask_bits is not (ncol, nlay, ceil(ngpt/32)) 32-bit words" % who)
    if not all(t is None or t.is_contiguous() for t in (src, cloud_frac, overlap_param, mask_bits)):
        raise ValueError("daylit.%s: arrays must be contiguous" % who)
    ctx = ctx or _ctx(cloud_frac.device)
    head = (ctx.h, int(ngpt), nlay, ncol, src.data_ptr(), cloud_frac.data_ptr())
    tail = (pl.idx.data_ptr(), pl.nday.data_ptr(), mask_bits.data_ptr())
    if exp_ran:
        head += (overlap_param.data_ptr() if nlay > 1 else None,)
    check(getattr(_lib.lib(), "rrtmgpnn_" + who)(*head, *tail), who)


def sampled_mask_active(pl, randoms, cloud_frac, mask_bits, overlap_param=None, ctx=None):
    """The packed McICA mask of the plan's daylit columns from the caller's randoms (ncol, nlay, ngpt): row j < nday of
    the dense mask_bits (ncol, nlay, ceil(ngpt / 32)) is column idx[j]'s mask, sampled from that column's randoms,
    cloud_frac (ncol, nlay) and overlap_param (ncol, nlay - 1) in place; rows at or past nday are left as they were.
    overlap_param None: maximum-random overlap, else exponential-random.  ctx: the api.Context to launch on."""
    import torch
    if randoms.dim() != 3 or tuple(randoms.shape[:2]) != tuple(cloud_frac.shape) or randoms.dtype != torch.float32:
        raise ValueError("daylit.sampled_mask_active: randoms is a float32 (ncol, nlay, ngpt) tensor")
    who = "sampled_mask_exp_ran_active" if overlap_param is not None else "sampled_mask_max_ran_active"
    _compact_mask(who, pl, randoms, cloud_frac, overlap_param, mask_bits, randoms.shape[2], ctx)


def sampled_mask_seeded_active(pl, rng, cloud_frac, mask_bits, ngpt, overlap_param=None, ctx=None):
    """As sampled_mask_active with the random numbers drawn in the kernel: rng is the 4-word device buffer of
    rrtmgpnn_mcica_rng_set {seed low, seed high, stream, col0}, and dense column j draws with the counter word
    col0 + idx[j] -- the clouds column idx[j] has in a block that is not compacted."""
    if rng.numel() != 4 or rng.element_size() != 4:
        raise ValueError("daylit.sampled_mask_seeded_active: rng is the 4-word buffer of rrtmgpnn_mcica_rng_set")
    who = "sampled_mask_exp_ran_seeded_active" if overlap_param is not None else "sampled_mask_max_ran_seeded_active"
    _compact_mask(who, pl, rng, cloud_frac, overlap_param, mask_bits, ngpt, ctx)


def arm_active_columns(ctx, pl):
    """Arm rrtmgpnn_solver_request_active_columns on `ctx` (an api.Context) for its next solver call: the first nday of
    the call's ncol columns."""
    check(_lib.lib().rrtmgpnn_solver_request_active_columns(ctx.h, pl.ncol, pl.nday.data_ptr()),
          "solver_request_active_columns")
