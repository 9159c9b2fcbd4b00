#!/usr/bin/env python3
"""Generate tests/golden/mcica_masks.npz from the REFERENCE's own extensions/cloud_optics/mo_cloud_sampling.F90.

Run in the build container, after `make -f oracle/Makefile.ref` (the module is compiled where it lies, with that
makefile's compiler and flags, against the reference modules under oracle/_ref/mod; nothing of it is copied):

    python tests/golden/make_mcica_golden.py

The fixture is DATA: the inputs tests/mcica_ref.py builds for FIXTURE_SHAPE / FIXTURE_SEED (randoms, cloud_frac,
overlap_param, in this project's layout) and the two logical masks sampled_mask_max_ran and sampled_mask_exp_ran
return on them.  The masks are pre-filled with .false. before each call: the reference's exp_ran leaves the mask of a
clear layer between cloudy ones unassigned.  The small driver below is this repository's own; the
work directory (driver, objects, module file, binary) is temporary.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mcica_ref as M  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
REF_FC = os.environ.get("REF_FC", "/opt/rocm/lib/llvm/bin/flang")
FFLAGS = os.environ.get("FFLAGS", "-O3 -cpp -fPIC -fopenmp").split()  # oracle/Makefile.ref
REFMOD = os.path.join(ROOT, "oracle", "_ref", "mod")
REFOBJ = os.path.join(ROOT, "oracle", "_ref", "obj")

DRIVER = """
program mcica_golden
  use mo_rte_kind, only: wp
  use mo_cloud_sampling, only: sampled_mask_max_ran, sampled_mask_exp_ran
  implicit none
  integer :: ngpt, nlay, ncol, u
  real(wp), allocatable :: randoms(:,:,:), cloud_frac(:,:), overlap_param(:,:)
  logical, allocatable :: mask(:,:,:)
  integer(1), allocatable :: bytes(:,:,:)
  character(len=128) :: msg
  open(newunit=u, file="in.bin", access="stream", form="unformatted", status="old")
  read(u) ngpt, nlay, ncol
  allocate(randoms(ngpt,nlay,ncol), cloud_frac(ncol,nlay), overlap_param(ncol,nlay-1))
  allocate(mask(ncol,nlay,ngpt), bytes(ncol,nlay,ngpt))
  read(u) randoms, cloud_frac, overlap_param
  close(u)
  open(newunit=u, file="out.bin", access="stream", form="unformatted", status="replace")
  mask = .false.
  msg = sampled_mask_max_ran(randoms, cloud_frac, mask)
  if (len_trim(msg) > 0) error stop "max_ran failed"
  bytes = merge(1_1, 0_1, mask)
  write(u) bytes
  mask = .false.
  msg = sampled_mask_exp_ran(randoms, cloud_frac, overlap_param, mask)
  if (len_trim(msg) > 0) error stop "exp_ran failed"
  bytes = merge(1_1, 0_1, mask)
  write(u) bytes
  close(u)
end program
"""


def main():
    ngpt, nlay, ncol = M.FIXTURE_SHAPE
    r, cf, ov = M.build(ngpt, nlay, ncol, M.FIXTURE_SEED)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "driver.F90"), "w") as f:
            f.write(DRIVER)
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            np.array([ngpt, nlay, ncol], np.int32).tofile(f)
            r.tofile(f)                                  # C (ncol, nlay, ngpt) = Fortran (ngpt, nlay, ncol)
            np.ascontiguousarray(cf.T).tofile(f)         # Fortran (ncol, nlay)
            np.ascontiguousarray(ov.T).tofile(f)         # Fortran (ncol, nlay-1)
        run = lambda *a: subprocess.run(list(a), cwd=tmp, check=True)
        run(REF_FC, *FFLAGS, "-J" + tmp, "-I" + REFMOD, "-c",
            os.path.join(REF, "extensions", "cloud_optics", "mo_cloud_sampling.F90"), "-o", "mo_cloud_sampling.o")
        objs = [os.path.join(REFOBJ, n + ".o") for n in ("mo_rte_kind", "mo_rte_rrtmgp_config", "mo_rte_util_array",
                                                        "mo_optical_props_kernels", "mo_optical_props")]
        run(REF_FC, *FFLAGS, "-I" + tmp, "-I" + REFMOD, "driver.F90", "mo_cloud_sampling.o", *objs, "-o", "driver")
        run(os.path.join(tmp, "driver"))
        out = np.fromfile(os.path.join(tmp, "out.bin"), np.int8)
    n = ncol * nlay * ngpt
    assert out.size == 2 * n
    # Fortran (ncol, nlay, ngpt) = C (ngpt, nlay, ncol) -> this project's (ncol, nlay, ngpt)
    to_ours = lambda a: np.ascontiguousarray(a.reshape(ngpt, nlay, ncol).transpose(2, 1, 0)).astype(np.uint8)
    dst = os.path.join(HERE, "mcica_masks.npz")
    np.savez_compressed(dst, randoms=r, cloud_frac=cf, overlap_param=ov, mask_max_ran=to_ours(out[:n]),
                        mask_exp_ran=to_ours(out[n:]))
    print("wrote %s (%d bytes)" % (dst, os.path.getsize(dst)))


if __name__ == "__main__":
    main()
