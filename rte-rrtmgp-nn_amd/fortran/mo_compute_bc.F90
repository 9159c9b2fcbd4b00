! mo_compute_bc -- drop-in for extensions/mo_compute_bc.F90: the upper boundary condition from one thin isothermal
! layer between the gas optics' minimum pressure and the model's top.  compute_bc keeps the reference's arguments,
! checks and error strings (:43-210) in this library's layout -- play, tlay (nlay, ncol), plev (nlay+1, ncol), flux_bc
! (ngpt, ncol), the inc_flux of rte_lw / rte_sw -- and takes the gas-optics networks as gas_optics does.  The
! one-layer problem, its gas optics and its solve run on the device in at most three launches
! (rrtmgpnn_compute_bc_lw / _sw); flux_bc is valid on the host on return.
! Units: the reference's longwave flux_bc is a radiance (its rte_lw call uses one angle, and rte_lw's one-angle
! g-point output is the radiance); that is the default.  as_flux = .true. multiplies by the solver's 2 pi w, which
! is what rte_lw's inc_flux means.
module mo_compute_bc
  use, intrinsic :: iso_c_binding
  use mo_rte_kind,           only: wp
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_gas_optics_rrtmgp,  only: ty_gas_optics_rrtmgp, gas_inputs, MAX_INPUTS
  use mod_network_rrtmgp,    only: rrtmgp_network_type
  use mo_rrtmgpnn_c
  implicit none
  private
  public :: compute_bc

contains

  function compute_bc(k_dist, play, plev, tlay, gas_concs, flux_bc, mu0, neural_nets, as_flux) result(error_msg)
    class(ty_gas_optics_rrtmgp), intent(in) :: k_dist
    real(wp), dimension(:,:), intent(in) :: play, plev, tlay   ! (nlay, ncol), (nlay+1, ncol), (nlay, ncol)
    type(ty_gas_concs),       intent(in) :: gas_concs
    real(wp), dimension(:,:), contiguous, target, intent(out) :: flux_bc   ! (ngpt, ncol)
    real(wp), dimension(:),   intent(in), optional :: mu0
    type(rrtmgp_network_type), dimension(:), intent(in), optional :: neural_nets
    logical,                  intent(in), optional :: as_flux
    character(len=128) :: error_msg
    logical :: top_at_1
    integer :: ncol, nlay, ngpt, top_lay, ninputs, n
    integer(c_int) :: flux_units
    integer(c_int), allocatable :: lims(:,:)
    integer(c_long_long) :: nl, nv, ng
    type(c_ptr) :: d_play, d_plev, d_tlay, d_h2o, d_out, d_mu0, d_src, d_tot
    type(c_ptr) :: nets(2), gas_ptr(MAX_INPUTS)
    integer(c_int) :: gas_nd(MAX_INPUTS)
    logical :: h2o_tmp
    real(wp), parameter :: gauss_D(1) = [1.66_wp], gauss_w(1) = [0.5_wp]  ! rte_lw's one-angle quadrature

    error_msg = ''
    ncol = size(play, dim=2)
    nlay = size(play, dim=1)
    ngpt = k_dist%get_ngpt()
    if (any(shape(plev) /= [nlay + 1, ncol])) error_msg = "compute_bc: array plev has wrong dimensions"
    if (any(shape(tlay) /= [nlay, ncol]))     error_msg = "compute_bc: array tlay has wrong dimensions"
    if (present(mu0)) then
      if (size(mu0) /= ncol) error_msg = "compute bc: array mu0 has wrong dimensions"
    end if
    if (error_msg /= '') return
    top_at_1 = play(1, 1) < play(nlay, 1)
    top_lay = merge(1, nlay, top_at_1)
    if (any(plev(top_lay, :) <= k_dist%get_press_min() + 2._wp * spacing(k_dist%get_press_min()))) then
      error_msg = "compute_bc: pressures are too close to (or less than) min in gas optics "
      return
    end if
    if (.not. k_dist%source_is_internal() .and. .not. present(mu0)) then
      error_msg = "compute_bc: have to supply mu0 for solar calculations"
      return
    end if
    if (.not. present(neural_nets)) then
      error_msg = "gas_optics(): the lookup-table branch is not available (k-distribution files missing); " // &
                  "pass neural_nets"
      return
    end if
    if (any(shape(flux_bc) /= [ngpt, ncol])) then
      error_msg = "compute_bc: array flux_bc has wrong dimensions"
      return
    end if
    n = size(neural_nets)
    if (n < 1 .or. n > 2 .or. (n /= 2 .and. .not. k_dist%source_is_internal())) then
      error_msg = "compute_bc: neural_nets must hold the stream's gas-optics models"
      return
    end if
    ninputs = size(neural_nets(1)%layers(1)%w_transposed, 2)
    error_msg = gas_inputs(nlay, ncol, gas_concs, neural_nets(1), gas_ptr, gas_nd, d_h2o, h2o_tmp)
    if (error_msg /= '') return
    flux_units = 0_c_int
    if (present(as_flux)) flux_units = merge(1_c_int, 0_c_int, as_flux)
    nl = int(nlay, c_long_long) * ncol
    nv = int(nlay + 1, c_long_long) * ncol
    ng = int(ngpt, c_long_long) * ncol
    d_play = dev_stage(play, nl)
    d_plev = dev_stage(plev, nv)
    d_tlay = dev_stage(tlay, nl)
    d_out = dev_present(flux_bc, ng, PRESENT_WRITE)
    nets = c_null_ptr
    nets(1) = neural_nets(1)%handle
    if (n == 2) nets(2) = neural_nets(2)%handle
    if (k_dist%source_is_internal()) then
      lims = k_dist%get_band_lims_gpoint()
      d_tot = dev_present(k_dist%totplnk, size(k_dist%totplnk, kind=c_long_long), PRESENT_READ)
      error_msg = rrtmgpnn_check(c_rrtmgpnn_compute_bc_lw(rrtmgpnn_ctx(), ncol, nlay, ngpt, ninputs, &
                      merge(1_c_int, 0_c_int, top_at_1), k_dist%get_press_min(), d_play, d_plev, d_tlay, d_h2o, gas_ptr, &
                      gas_nd, nets, n, k_dist%get_nband(), k_dist%get_nPlanckTemp(), lims, k_dist%temp_ref_min, &
                      k_dist%totplnk_delta, d_tot, 1_c_int, gauss_D, gauss_w, flux_units, d_out), "compute_bc_lw")
    else
      d_mu0 = dev_stage(mu0, int(ncol, c_long_long))
      d_src = dev_stage(k_dist%solar_source, int(ngpt, c_long_long))
      error_msg = rrtmgpnn_check(c_rrtmgpnn_compute_bc_sw(rrtmgpnn_ctx(), ncol, nlay, ngpt, ninputs, &
                      merge(1_c_int, 0_c_int, top_at_1), k_dist%get_press_min(), d_play, d_plev, d_tlay, d_h2o, gas_ptr, &
                      gas_nd, nets, d_src, d_mu0, d_out), "compute_bc_sw")
      call dev_release(d_mu0)
      call dev_release(d_src)
    end if
    call dev_release(d_play)
    call dev_release(d_plev)
    call dev_release(d_tlay)
    if (h2o_tmp) call dev_release(d_h2o)
    ! flux_bc is an output of this call: bring it to the host (waits for the kernels) and leave no device copy behind
    if (error_msg == '') call dev_update_host(flux_bc)
    call dev_delete(flux_bc)
  end function compute_bc
end module mo_compute_bc
