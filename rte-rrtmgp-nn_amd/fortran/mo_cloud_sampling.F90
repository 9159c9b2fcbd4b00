! mo_cloud_sampling -- McICA sampling of band-resolved cloud optical properties
! (extensions/cloud_optics/mo_cloud_sampling.F90) on the GPU: the reference's three public names.
!
!   sampled_mask_max_ran(randoms, cloud_frac, cloud_mask)                  :125-192
!   sampled_mask_exp_ran(randoms, cloud_frac, overlap_param, cloud_mask)   :200-285
!   draw_samples(cloud_mask, clouds, clouds_sampled)                       :36-120
!
! The extension predates this fork's layout (as mo_heating_rates does).  Here randoms and cloud_mask are
! (ngpt, nlay, ncol), cloud_frac (nlay, ncol) and overlap_param (nlay-1, ncol).  cloud_mask is logical(wl)
! (one byte); like the optical properties it stays on the device: the mask functions leave its device copy newer,
! draw_samples reads that copy, and a host program that wants the values calls cloud_mask_update_host first.
! randoms, cloud_frac and overlap_param are copied to the device by every call (a host program refills them).
! The value checks follow check_values (rte_config_checks) as the other value checks of this layer do, with the
! reference's messages -- exp_ran's carry max_ran's prefix there too.
! No reference counterpart: mcica_randoms, sampled_mask_max_ran_seeded and sampled_mask_exp_ran_seeded take
! (seed, stream, col0) in place of randoms and draw the numbers on the device (Philox4x32-10; include/rrtmgpnn.h has the
! counter layout): a column's numbers depend on the seed, the stream, its global index col0 + icol (0-based, modulo
! 2**32), the layer and the g-point alone.  seed is integer(int64) (its bit pattern is the 64-bit seed); stream and col0
! are integer(int64) holding 32-bit words (taken modulo 2**32).
! Quirk (SURVEY.md App. B, B-13): the reference's exp_ran never assigns the mask of a clear layer lying between cloudy
! ones; here those elements are .false., the evident meaning and what max_ran does.
module mo_cloud_sampling
  use, intrinsic :: iso_c_binding
  use, intrinsic :: iso_fortran_env, only: int64
  use mo_rte_kind,          only: wp, wl
  use mo_rte_rrtmgp_config, only: check_values
  use mo_optical_props,     only: ty_optical_props_arry, ty_optical_props_1scl, ty_optical_props_2str
  use mo_rrtmgpnn_c
  implicit none
  private
  public :: draw_samples, sampled_mask_max_ran, sampled_mask_exp_ran, cloud_mask_update_host, cloud_mask_delete
  public :: mcica_randoms, sampled_mask_max_ran_seeded, sampled_mask_exp_ran_seeded
contains
  ! the device copy of a logical(wl) mask of n elements (one byte each) in the context's data environment
  function mask_present(m, n, mode) result(d)
    logical(wl), dimension(*), intent(in), target :: m
    integer(c_long_long), intent(in) :: n
    integer(c_int), intent(in) :: mode
    type(c_ptr) :: d
    d = c_null_ptr
    if (c_rrtmgpnn_present(rrtmgpnn_ctx(), c_loc(m), n, mode, d) /= 0) then
      write(*, '(a)') "rrtmgpnn: present (cloud mask): " // trim(rrtmgpnn_error_message())
      error stop 1
    end if
  end function mask_present

  ! `!$acc update host` of a mask the mask functions produced
  subroutine cloud_mask_update_host(cloud_mask)
    logical(wl), dimension(*), intent(inout), target :: cloud_mask
    if (.not. rrtmgpnn_has_context()) return
    if (c_rrtmgpnn_present_update_host(rrtmgpnn_ctx(), c_loc(cloud_mask)) /= 0) then
      write(*, '(a)') "rrtmgpnn: update host (cloud mask): " // trim(rrtmgpnn_error_message())
      error stop 1
    end if
  end subroutine cloud_mask_update_host

  ! `!$acc exit data delete` of a mask's device copy (before the host array is deallocated)
  subroutine cloud_mask_delete(cloud_mask)
    logical(wl), dimension(*), intent(in), target :: cloud_mask
    if (.not. rrtmgpnn_has_context()) return
    if (c_rrtmgpnn_present_delete(rrtmgpnn_ctx(), c_loc(cloud_mask)) /= 0) then
      write(*, '(a)') "rrtmgpnn: delete (cloud mask): " // trim(rrtmgpnn_error_message())
      error stop 1
    end if
  end subroutine cloud_mask_delete

  function sampled_mask_max_ran(randoms, cloud_frac, cloud_mask) result(error_msg)
    real(wp),    dimension(:,:,:), intent(in ) :: randoms    ! ngpt, nlay, ncol
    real(wp),    dimension(:,:),   intent(in ) :: cloud_frac ! nlay, ncol
    logical(wl), dimension(:,:,:), intent(out) :: cloud_mask ! ngpt, nlay, ncol
    character(len=128) :: error_msg
    integer :: ncol, nlay, ngpt
    integer(c_long_long) :: n
    type(c_ptr) :: d_r, d_cf, d_m

    error_msg = ""
    ngpt = size(randoms, 1); nlay = size(randoms, 2); ncol = size(randoms, 3)
    if (any([nlay, ncol] /= [size(cloud_frac, 1), size(cloud_frac, 2)])) then
      error_msg = "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and cloud_frac(ncol,nlay) are inconsistent"
      return
    end if
    if (any([ngpt, nlay, ncol] /= [size(cloud_mask, 1), size(cloud_mask, 2), size(cloud_mask, 3)])) then
      error_msg = "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and cloud_mask(ncol,nlay,ngpt) are inconsistent"
      return
    end if
    if (check_values) then
      if (any(cloud_frac > 1._wp) .or. any(cloud_frac < 0._wp)) then
        error_msg = "sampled_mask_max_ran: cloud fraction values out of range [0,1]"
        return
      end if
    end if
    n = int(ngpt, c_long_long) * nlay * ncol
    d_r  = dev_stage(randoms, n)
    d_cf = dev_stage(cloud_frac, int(nlay, c_long_long) * ncol)
    d_m  = mask_present(cloud_mask, n, PRESENT_WRITE)
    error_msg = rrtmgpnn_check(c_rrtmgpnn_sampled_mask_max_ran(rrtmgpnn_ctx(), ngpt, nlay, ncol, d_r, d_cf, d_m, &
                               c_null_ptr), "sampled_mask_max_ran")
    call dev_release(d_r); call dev_release(d_cf)
  end function sampled_mask_max_ran

  function sampled_mask_exp_ran(randoms, cloud_frac, overlap_param, cloud_mask) result(error_msg)
    real(wp),    dimension(:,:,:), intent(in ) :: randoms       ! ngpt, nlay, ncol
    real(wp),    dimension(:,:),   intent(in ) :: cloud_frac    ! nlay, ncol
    real(wp),    dimension(:,:),   intent(in ) :: overlap_param ! nlay-1, ncol
    logical(wl), dimension(:,:,:), intent(out) :: cloud_mask    ! ngpt, nlay, ncol
    character(len=128) :: error_msg
    integer :: ncol, nlay, ngpt
    integer(c_long_long) :: n
    type(c_ptr) :: d_r, d_cf, d_ov, d_m

    error_msg = ""
    ngpt = size(randoms, 1); nlay = size(randoms, 2); ncol = size(randoms, 3)
    if (any([nlay, ncol] /= [size(cloud_frac, 1), size(cloud_frac, 2)])) then
      error_msg = "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and cloud_frac(ncol,nlay) are inconsistent"
      return
    end if
    if (any([nlay - 1, ncol] /= [size(overlap_param, 1), size(overlap_param, 2)])) then
      error_msg = "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and overlap_param(ncol,nlay-1) are inconsistent"
      return
    end if
    if (any([ngpt, nlay, ncol] /= [size(cloud_mask, 1), size(cloud_mask, 2), size(cloud_mask, 3)])) then
      error_msg = "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and cloud_mask(ncol,nlay,ngpt) are inconsistent"
      return
    end if
    if (check_values) then
      if (any(cloud_frac > 1._wp) .or. any(cloud_frac < 0._wp)) then
        error_msg = "sampled_mask_max_ran: cloud fraction values out of range [0,1]"
        return
      end if
      if (any(overlap_param > 1._wp) .or. any(overlap_param < -1._wp)) then
        error_msg = "sampled_mask_max_ran: overlap_param values out of range [-1,1]"
        return
      end if
    end if
    n = int(ngpt, c_long_long) * nlay * ncol
    d_r  = dev_stage(randoms, n)
    d_cf = dev_stage(cloud_frac, int(nlay, c_long_long) * ncol)
    d_ov = c_null_ptr
    if (nlay > 1) d_ov = dev_stage(overlap_param, int(nlay - 1, c_long_long) * ncol)
    d_m  = mask_present(cloud_mask, n, PRESENT_WRITE)
    error_msg = rrtmgpnn_check(c_rrtmgpnn_sampled_mask_exp_ran(rrtmgpnn_ctx(), ngpt, nlay, ncol, d_r, d_cf, d_ov, d_m, &
                               c_null_ptr), "sampled_mask_exp_ran")
    call dev_release(d_r); call dev_release(d_cf); call dev_release(d_ov)
  end function sampled_mask_exp_ran

  ! the low 32 bits of v as a C unsigned int's bit pattern
  pure function u32(v) result(w)
    integer(int64), intent(in) :: v
    integer(c_int) :: w
    integer(int64) :: m
    m = iand(v, 4294967295_int64)
    if (m >= 2147483648_int64) m = m - 4294967296_int64
    w = int(m, c_int)
  end function u32

  ! a pool buffer holding the four rng words {seed low, seed high, stream, col0}
  function rng_stage(seed, stream, col0, error_msg) result(d)
    integer(int64), intent(in) :: seed, stream, col0
    character(len=128), intent(out) :: error_msg
    type(c_ptr) :: d
    d = dev_scratch(4_c_long_long)
    error_msg = rrtmgpnn_check(c_rrtmgpnn_mcica_rng_set(rrtmgpnn_ctx(), int(seed, c_long_long), u32(stream), u32(col0), &
                               d), "mcica_rng_set")
  end function rng_stage

  function mcica_randoms(seed, stream, col0, randoms) result(error_msg)
    integer(int64),                intent(in ) :: seed, stream, col0
    real(wp), dimension(:,:,:),    intent(out) :: randoms ! ngpt, nlay, ncol
    character(len=128) :: error_msg
    integer :: ncol, nlay, ngpt
    integer(c_long_long) :: n
    type(c_ptr) :: d_rng, d_r

    error_msg = ""
    ngpt = size(randoms, 1); nlay = size(randoms, 2); ncol = size(randoms, 3)
    n = int(ngpt, c_long_long) * nlay * ncol
    if (n == 0) return
    d_rng = rng_stage(seed, stream, col0, error_msg)
    if (error_msg == "") then
      d_r = dev_scratch(n)
      error_msg = rrtmgpnn_check(c_rrtmgpnn_mcica_randoms(rrtmgpnn_ctx(), ngpt, nlay, ncol, d_rng, d_r), "mcica_randoms")
      if (error_msg == "") call dev_copy_out(randoms, d_r, n)
      call rrtmgpnn_sync(error_msg, "mcica_randoms")
      call dev_release(d_r)
    end if
    call dev_release(d_rng)
  end function mcica_randoms

  function sampled_mask_max_ran_seeded(seed, stream, col0, cloud_frac, cloud_mask) result(error_msg)
    integer(int64),                intent(in ) :: seed, stream, col0
    real(wp),    dimension(:,:),   intent(in ) :: cloud_frac ! nlay, ncol
    logical(wl), dimension(:,:,:), intent(out) :: cloud_mask ! ngpt, nlay, ncol
    character(len=128) :: error_msg
    integer :: ncol, nlay, ngpt
    integer(c_long_long) :: n
    type(c_ptr) :: d_rng, d_cf, d_m

    error_msg = ""
    ngpt = size(cloud_mask, 1); nlay = size(cloud_frac, 1); ncol = size(cloud_frac, 2)
    if (any([nlay, ncol] /= [size(cloud_mask, 2), size(cloud_mask, 3)])) then
      error_msg = "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and cloud_mask(ncol,nlay,ngpt) are inconsistent"
      return
    end if
    if (check_values) then
      if (any(cloud_frac > 1._wp) .or. any(cloud_frac < 0._wp)) then
        error_msg = "sampled_mask_max_ran: cloud fraction values out of range [0,1]"
        return
      end if
    end if
    n = int(ngpt, c_long_long) * nlay * ncol
    d_rng = rng_stage(seed, stream, col0, error_msg)
    if (error_msg == "") then
      d_cf = dev_stage(cloud_frac, int(nlay, c_long_long) * ncol)
      d_m  = mask_present(cloud_mask, n, PRESENT_WRITE)
      error_msg = rrtmgpnn_check(c_rrtmgpnn_sampled_mask_max_ran_seeded(rrtmgpnn_ctx(), ngpt, nlay, ncol, d_rng, d_cf, &
                                 d_m, c_null_ptr), "sampled_mask_max_ran_seeded")
      call dev_release(d_cf)
    end if
    call dev_release(d_rng)
  end function sampled_mask_max_ran_seeded

  function sampled_mask_exp_ran_seeded(seed, stream, col0, cloud_frac, overlap_param, cloud_mask) result(error_msg)
    integer(int64),                intent(in ) :: seed, stream, col0
    real(wp),    dimension(:,:),   intent(in ) :: cloud_frac    ! nlay, ncol
    real(wp),    dimension(:,:),   intent(in ) :: overlap_param ! nlay-1, ncol
    logical(wl), dimension(:,:,:), intent(out) :: cloud_mask    ! ngpt, nlay, ncol
    character(len=128) :: error_msg
    integer :: ncol, nlay, ngpt
    integer(c_long_long) :: n
    type(c_ptr) :: d_rng, d_cf, d_ov, d_m

    error_msg = ""
    ngpt = size(cloud_mask, 1); nlay = size(cloud_frac, 1); ncol = size(cloud_frac, 2)
    if (any([nlay - 1, ncol] /= [size(overlap_param, 1), size(overlap_param, 2)])) then
      error_msg = "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and overlap_param(ncol,nlay-1) are inconsistent"
      return
    end if
    if (any([nlay, ncol] /= [size(cloud_mask, 2), size(cloud_mask, 3)])) then
      error_msg = "sampled_mask_max_ran: sizes of randoms(ngpt,nlay,ncol) and cloud_mask(ncol,nlay,ngpt) are inconsistent"
      return
    end if
    if (check_values) then
      if (any(cloud_frac > 1._wp) .or. any(cloud_frac < 0._wp)) then
        error_msg = "sampled_mask_max_ran: cloud fraction values out of range [0,1]"
        return
      end if
      if (any(overlap_param > 1._wp) .or. any(overlap_param < -1._wp)) then
        error_msg = "sampled_mask_max_ran: overlap_param values out of range [-1,1]"
        return
      end if
    end if
    n = int(ngpt, c_long_long) * nlay * ncol
    d_rng = rng_stage(seed, stream, col0, error_msg)
    if (error_msg == "") then
      d_cf = dev_stage(cloud_frac, int(nlay, c_long_long) * ncol)
      d_ov = c_null_ptr
      if (nlay > 1) d_ov = dev_stage(overlap_param, int(nlay - 1, c_long_long) * ncol)
      d_m  = mask_present(cloud_mask, n, PRESENT_WRITE)
      error_msg = rrtmgpnn_check(c_rrtmgpnn_sampled_mask_exp_ran_seeded(rrtmgpnn_ctx(), ngpt, nlay, ncol, d_rng, d_cf, &
                                 d_ov, d_m, c_null_ptr), "sampled_mask_exp_ran_seeded")
      call dev_release(d_cf); call dev_release(d_ov)
    end if
    call dev_release(d_rng)
  end function sampled_mask_exp_ran_seeded

  function draw_samples(cloud_mask, clouds, clouds_sampled) result(error_msg)
    logical(wl), dimension(:,:,:), intent(in   ) :: cloud_mask     ! ngpt, nlay, ncol
    class(ty_optical_props_arry),  intent(in   ) :: clouds         ! defined by band
    class(ty_optical_props_arry),  intent(inout) :: clouds_sampled ! defined by g-point
    character(len=128) :: error_msg
    integer :: ncol, nlay, nbnd, ngpt
    integer(c_long_long) :: nb, ng
    type(c_ptr) :: d_m, tb, sb, gb, t, s, g

    error_msg = ""
    if (.not. clouds%is_initialized()) then
      error_msg = "draw_samples: cloud optical properties are not initialized"
      return
    end if
    if (.not. clouds_sampled%is_initialized()) then
      error_msg = "draw_samples: sampled cloud optical properties are not initialized"
      return
    end if
    ! clouds and clouds_sampled have to be of the same type (:59-76); nstr is not part of this layer
    select type (clouds)
    type is (ty_optical_props_1scl)
      select type (clouds_sampled)
      type is (ty_optical_props_2str)
        error_msg = "draw_samples: by-band and sampled cloud properties need to be the same variable type"
        return
      end select
    end select
    if (.not. clouds%bands_are_equal(clouds_sampled)) then
      error_msg = "draw_samples: by-band and sampled cloud properties spectral structure is different"
      return
    end if
    ncol = clouds%get_ncol()
    nlay = clouds%get_nlay()
    nbnd = clouds%get_nband()
    ngpt = clouds_sampled%get_ngpt()
    if (any([size(cloud_mask, 1), size(cloud_mask, 2), size(cloud_mask, 3)] /= [ngpt, nlay, ncol])) then
      error_msg = "draw_samples: cloud mask and cloud optical properties have different ncol and/or nlay"
      return
    end if
    if (any([clouds_sampled%get_ncol(), clouds_sampled%get_nlay()] /= [ncol, nlay])) then
      error_msg = "draw_samples: sampled/unsampled cloud optical properties have different ncol and/or nlay"
      return
    end if
    nb = int(nbnd, c_long_long) * nlay * ncol
    ng = int(ngpt, c_long_long) * nlay * ncol
    d_m = mask_present(cloud_mask, ng, PRESENT_READ)
    tb = dev_present(clouds%tau, nb, PRESENT_READ)
    t  = dev_present(clouds_sampled%tau, ng, PRESENT_WRITE)
    sb = c_null_ptr; gb = c_null_ptr; s = c_null_ptr; g = c_null_ptr
    select type (clouds)
    type is (ty_optical_props_2str)
      select type (clouds_sampled)
      type is (ty_optical_props_2str)
        if (clouds%g_zero) then
          error_msg = "draw_samples: by-band cloud properties have no asymmetry parameter"
          return
        end if
        sb = dev_present(clouds%ssa, nb, PRESENT_READ)
        gb = dev_present(clouds%g, nb, PRESENT_READ)
        s  = dev_present(clouds_sampled%ssa, ng, PRESENT_WRITE)
        g  = dev_present(clouds_sampled%g, ng, PRESENT_WRITE)
        clouds_sampled%g_zero = .false.
      class default
        error_msg = "draw_samples: by-band and sampled cloud properties need to be the same variable type"
        return
      end select
    end select
    error_msg = rrtmgpnn_check(c_rrtmgpnn_draw_samples(rrtmgpnn_ctx(), ngpt, nlay, ncol, nbnd, clouds_sampled%band2gpt, &
                               d_m, tb, sb, gb, t, s, g), "draw_samples")
  end function draw_samples
end module mo_cloud_sampling
