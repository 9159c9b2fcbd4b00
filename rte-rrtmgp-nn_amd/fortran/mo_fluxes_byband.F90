! mo_fluxes_byband -- drop-in for extensions/mo_fluxes_byband.F90 (ty_fluxes_byband, :31-131): the broadband and
! g-point outputs of ty_fluxes_flexible plus by-band fluxes, pointers into caller memory.  It extends
! ty_fluxes_flexible, so it passes through the class(ty_fluxes_flexible) dummies of rte_lw / rte_sw, which detect it
! with select type and have the solvers form the band sums (rrtmgpnn_solver_request_byband): each value is the
! reference's sum_byband (extensions/mo_fluxes_byband_kernels.F90:31-50) of the g-point fluxes.
! Layout: (nbnd, nlay+1, ncol), band fastest -- this project's spectral-dimension-first layout; the reference's arrays
! are (ncol, nlev, nband).  bnd_flux_net = bnd_flux_dn - bnd_flux_up (net_byband_precalc) needs both of those
! associated; the reference's net_byband_full order is not reproduced.
module mo_fluxes_byband
  use mo_rte_kind, only: wp
  use mo_fluxes,   only: ty_fluxes_flexible
  implicit none
  private

  type, extends(ty_fluxes_flexible), public :: ty_fluxes_byband
    real(wp), dimension(:,:,:), contiguous, pointer :: bnd_flux_up => NULL(), bnd_flux_dn => NULL()
    real(wp), dimension(:,:,:), contiguous, pointer :: bnd_flux_net => NULL(), bnd_flux_dn_dir => NULL()
  contains
    procedure, public :: are_desired => are_desired_byband
    procedure, public :: are_desired_bnd
    procedure, public :: check_extents_bnd
  end type ty_fluxes_byband

contains

  ! are_desired_byband (extensions/mo_fluxes_byband.F90:136-145): any by-band array, or any broadband one
  logical function are_desired_byband(this)
    class(ty_fluxes_byband), intent(in) :: this
    are_desired_byband = this%are_desired_bnd() .or. this%ty_fluxes_flexible%are_desired()
  end function are_desired_byband

  logical function are_desired_bnd(this)
    class(ty_fluxes_byband), intent(in) :: this
    are_desired_bnd = any([associated(this%bnd_flux_up), associated(this%bnd_flux_dn), &
                           associated(this%bnd_flux_dn_dir), associated(this%bnd_flux_net)])
  end function are_desired_bnd

  ! reduce_byband's checks (:72-97): every associated by-band array must be (nbnd, nlev, ncol), the last failing
  ! array's message is returned; then the direct beam must be supplied when bnd_flux_dn_dir is asked for.  Last, this
  ! layer's own condition on bnd_flux_net.
  function check_extents_bnd(this, nbnd, nlev, ncol, have_beam) result(error_msg)
    class(ty_fluxes_byband), intent(in) :: this
    integer,                 intent(in) :: nbnd, nlev, ncol
    logical,                 intent(in) :: have_beam
    character(len=128) :: error_msg
    error_msg = ""
    if (associated(this%bnd_flux_up)) then
      if (any(shape(this%bnd_flux_up) /= [nbnd, nlev, ncol])) &
        error_msg = "reduce: bnd_flux_up array incorrectly sized (can't compute net flux either)"
    end if
    if (associated(this%bnd_flux_dn)) then
      if (any(shape(this%bnd_flux_dn) /= [nbnd, nlev, ncol])) &
        error_msg = "reduce: bnd_flux_dn array incorrectly sized (can't compute net flux either)"
    end if
    if (associated(this%bnd_flux_dn_dir)) then
      if (any(shape(this%bnd_flux_dn_dir) /= [nbnd, nlev, ncol])) &
        error_msg = "reduce: bnd_flux_dn_dir array incorrectly sized"
    end if
    if (associated(this%bnd_flux_net)) then
      if (any(shape(this%bnd_flux_net) /= [nbnd, nlev, ncol])) &
        error_msg = "reduce: bnd_flux_net array incorrectly sized (can't compute net flux either)"
    end if
    if (error_msg /= "") return
    if (associated(this%bnd_flux_dn_dir) .and. .not. have_beam) then
      error_msg = "reduce: requesting bnd_flux_dn_dir but direct flux hasn't been supplied"
      return
    end if
    if (associated(this%bnd_flux_net) .and. .not. (associated(this%bnd_flux_up) .and. associated(this%bnd_flux_dn))) &
      error_msg = "reduce: bnd_flux_net needs bnd_flux_up and bnd_flux_dn (net_byband_full is not provided)"
  end function check_extents_bnd
end module mo_fluxes_byband
