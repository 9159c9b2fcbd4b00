! mcica_seeded.F90 -- mo_cloud_sampling's seeded functions through the Fortran drop-in (tests/test_fortran_mcica_seeded.py).
! usage: mcica_seeded <input.rbin> <output.rbin> <ngpt> <seed> <stream> <col0>
!   input.rbin: cloud_frac (nlay, ncol), overlap_param (nlay-1, ncol)
!   output.rbin: randoms (ngpt, nlay, ncol) from mcica_randoms; mask_max_ran and mask_exp_ran (ngpt, nlay, ncol) as
!   0 / 1 reals from sampled_mask_max_ran_seeded / sampled_mask_exp_ran_seeded.
!   A cloud_mask of the wrong extents is refused with the reference's message (exit status 6).
program mcica_seeded
  use, intrinsic :: iso_fortran_env, only: int64
  use mo_rte_kind,       only: wp, wl
  use mo_cloud_sampling, only: mcica_randoms, sampled_mask_max_ran_seeded, sampled_mask_exp_ran_seeded, &
                               cloud_mask_update_host, cloud_mask_delete
  use mo_rrtmgpnn_rbin
  implicit none
  character(len=512) :: ifile, ofile, arg
  real(wp), allocatable :: cloud_frac(:,:), overlap_param(:,:), randoms(:,:,:), out(:,:,:)
  logical(wl), allocatable :: mask(:,:,:), bad(:,:,:)
  integer(int64) :: seed, stream, col0
  integer :: ngpt, nlay, ncol, u
  character(len=128) :: e

  call get_command_argument(1, ifile)
  call get_command_argument(2, ofile)
  call get_command_argument(3, arg); read(arg, *) ngpt
  call get_command_argument(4, arg); read(arg, *) seed
  call get_command_argument(5, arg); read(arg, *) stream
  call get_command_argument(6, arg); read(arg, *) col0
  call rbin_real2(ifile, "cloud_frac", cloud_frac, e); call chk(e)
  call rbin_real2(ifile, "overlap_param", overlap_param, e); call chk(e)
  nlay = size(cloud_frac, 1)
  ncol = size(cloud_frac, 2)
  allocate(randoms(ngpt, nlay, ncol), mask(ngpt, nlay, ncol), out(ngpt, nlay, ncol), bad(ngpt, nlay + 1, ncol))
  u = rbin_write_begin(ofile, 3)
  randoms = -1._wp
  call chk(mcica_randoms(seed, stream, col0, randoms))
  call rbin_write_real(u, "randoms", randoms, shape(randoms))
  call chk(sampled_mask_max_ran_seeded(seed, stream, col0, cloud_frac, mask))
  call cloud_mask_update_host(mask)
  out = merge(1._wp, 0._wp, mask)
  call rbin_write_real(u, "mask_max_ran", out, shape(out))
  call chk(sampled_mask_exp_ran_seeded(seed, stream, col0, cloud_frac, overlap_param, mask))
  call cloud_mask_update_host(mask)
  out = merge(1._wp, 0._wp, mask)
  call rbin_write_real(u, "mask_exp_ran", out, shape(out))
  call rbin_write_end(u)
  call cloud_mask_delete(mask)
  e = sampled_mask_max_ran_seeded(seed, stream, col0, cloud_frac, bad)
  if (e /= "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and cloud_mask(ncol,nlay,ngpt) are inconsistent") then
    write(*, '(a)') "a cloud_mask with one layer too many returned: '" // trim(e) // "'"
    error stop 6
  end if
contains
  subroutine chk(msg)
    character(len=*), intent(in) :: msg
    if (len_trim(msg) > 0) then
      write(*, '(a)') trim(msg)
      error stop 1
    end if
  end subroutine chk
end program mcica_seeded
