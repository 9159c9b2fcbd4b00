! lw_scat_dual -- test host program: mo_rrtmgp_clr_all_sky's rte_lw with by-band two-stream (scattering) clouds and
! by-band 1scl aerosols (tests/test_fortran_lw_scat_dual.py).  The band properties are synthetic and formed from the indices alone, so that
! the Python class layer forms the same float32 values (1-based indices):
!   cloud tau(ibnd, ilay, icol) = 0.05 * (1 + mod(3 ibnd + 5 ilay + 7 icol, 13))
!   cloud ssa(ibnd, ilay, icol) = 0.2 + 0.05 * mod(ibnd + 2 ilay + 3 icol, 14)
!   cloud g(ibnd, ilay, icol)   = 0.5 + 0.03 * mod(2 ibnd + ilay + 5 icol, 15)
!   aerosol tau(ibnd, ilay, icol) = 0.01 * (1 + mod(ibnd + 3 ilay + 11 icol, 17))
! Two calls: (bnd) with the aerosols -- rrtmgpnn_solver_request_aerosol, then rrtmgpnn_lw_solver_1rescl_planck_clr_all,
! the clear sky gases + aerosols --, (none) without them.
!
! usage: lw_scat_dual <problem.rbin> <output.rbin> <data_dir>
program lw_scat_dual
  use mo_rte_kind,           only: wp
  use mo_optical_props,      only: ty_optical_props_1scl, ty_optical_props_2str
  use mo_fluxes,             only: ty_fluxes_flexible
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_gas_optics_rrtmgp,  only: ty_gas_optics_rrtmgp
  use mod_network_rrtmgp,    only: rrtmgp_network_type
  use mo_rrtmgp_clr_all_sky, only: rte_lw
  use mo_rrtmgpnn_rbin
  implicit none

  character(len=512) :: problem_file, output_file, data_dir
  real(wp), allocatable :: play(:,:), plev(:,:), tlay(:,:), tlev(:,:), tsfc(:), sfc_emis(:), vmr(:,:), emis(:,:)
  character(len=32), allocatable :: gas_names(:)
  real(wp), allocatable, target :: up(:,:,:), dn(:,:,:), upc(:,:,:), dnc(:,:,:)
  integer, allocatable :: lims(:,:)
  type(ty_gas_concs) :: gas_concs
  type(ty_gas_optics_rrtmgp) :: kdist
  type(rrtmgp_network_type), dimension(2) :: nets
  type(ty_optical_props_2str) :: clouds
  type(ty_optical_props_1scl) :: aer
  type(ty_fluxes_flexible) :: fluxes, fluxes_clr
  character(len=128) :: e
  integer :: ncol, nlay, nbnd, ig, ib, il, ic, k, u

  if (command_argument_count() < 3) stop 2
  call get_command_argument(1, problem_file)
  call get_command_argument(2, output_file)
  call get_command_argument(3, data_dir)
  call rbin_real2(problem_file, "play", play, e); call stop_on_err(e)
  call rbin_real2(problem_file, "plev", plev, e); call stop_on_err(e)
  call rbin_real2(problem_file, "tlay", tlay, e); call stop_on_err(e)
  call rbin_real2(problem_file, "tlev", tlev, e); call stop_on_err(e)
  call rbin_real1(problem_file, "tsfc", tsfc, e); call stop_on_err(e)
  call rbin_real1(problem_file, "sfc_emis", sfc_emis, e); call stop_on_err(e)
  call rbin_strings(problem_file, "gas_names", gas_names, e); call stop_on_err(e)
  nlay = size(play, 1)
  ncol = size(play, 2)
  call nets(1)%load_netcdf(trim(data_dir) // "/nn_lw_g256_abs.rbin")
  call nets(2)%load_netcdf(trim(data_dir) // "/nn_lw_g256_pfrac.rbin")
  call stop_on_err(kdist%load_rbin(trim(data_dir) // "/kdist_lw_g256.rbin", gas_names))
  call stop_on_err(gas_concs%init(gas_names))
  do ig = 1, size(gas_names)
    call rbin_real2(problem_file, "vmr_" // trim(gas_names(ig)), vmr, e); call stop_on_err(e)
    call stop_on_err(gas_concs%set_vmr(gas_names(ig), vmr))
  end do
  nbnd = kdist%get_nband()
  lims = kdist%get_band_lims_gpoint()

  call stop_on_err(clouds%alloc_2str(ncol, nlay, kdist%get_band_lims_wavenumber()))
  do ic = 1, ncol
    do il = 1, nlay
      do ib = 1, nbnd
        clouds%tau(ib, il, ic) = 0.05_wp * real(1 + mod(3 * ib + 5 * il + 7 * ic, 13), wp)
        clouds%ssa(ib, il, ic) = 0.2_wp + 0.05_wp * real(mod(ib + 2 * il + 3 * ic, 14), wp)
        clouds%g(ib, il, ic) = 0.5_wp + 0.03_wp * real(mod(2 * ib + il + 5 * ic, 15), wp)
      end do
    end do
  end do
  call stop_on_err(aer%alloc_1scl(ncol, nlay, kdist%get_band_lims_wavenumber()))
  do ic = 1, ncol
    do il = 1, nlay
      do ib = 1, nbnd
        aer%tau(ib, il, ic) = 0.01_wp * real(1 + mod(ib + 3 * il + 11 * ic, 17), wp)
      end do
    end do
  end do
  allocate(emis(nbnd, ncol))
  do ic = 1, ncol
    emis(:, ic) = sfc_emis(ic)
  end do
  allocate(up(nlay + 1, ncol, 2), dn(nlay + 1, ncol, 2), upc(nlay + 1, ncol, 2), dnc(nlay + 1, ncol, 2))
  do k = 1, 2
    fluxes%flux_up => up(:, :, k)
    fluxes%flux_dn => dn(:, :, k)
    fluxes_clr%flux_up => upc(:, :, k)
    fluxes_clr%flux_dn => dnc(:, :, k)
    if (k == 1) then
      call stop_on_err(rte_lw(kdist, gas_concs, play, tlay, plev, tsfc, emis, clouds, fluxes, fluxes_clr, &
                              aer_props=aer, t_lev=tlev, neural_nets=nets))
    else
      call stop_on_err(rte_lw(kdist, gas_concs, play, tlay, plev, tsfc, emis, clouds, fluxes, fluxes_clr, &
                              t_lev=tlev, neural_nets=nets))
    end if
  end do

  u = rbin_write_begin(output_file, 8)
  call put("bnd", 1)
  call put("none", 2)
  call rbin_write_end(u)

contains
  subroutine put(tag, k)
    character(len=*), intent(in) :: tag
    integer, intent(in) :: k
    call rbin_write_real(u, "up_" // tag, up(:, :, k), shape(up(:, :, k)))
    call rbin_write_real(u, "dn_" // tag, dn(:, :, k), shape(dn(:, :, k)))
    call rbin_write_real(u, "up_clr_" // tag, upc(:, :, k), shape(upc(:, :, k)))
    call rbin_write_real(u, "dn_clr_" // tag, dnc(:, :, k), shape(dnc(:, :, k)))
  end subroutine put

  subroutine stop_on_err(msg)
    character(len=*), intent(in) :: msg
    if (len_trim(msg) > 0) then
      write(*, '(a)') trim(msg)
      error stop 1
    end if
  end subroutine stop_on_err
end program lw_scat_dual
