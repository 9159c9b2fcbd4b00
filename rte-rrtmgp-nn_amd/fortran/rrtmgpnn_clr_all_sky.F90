! rrtmgpnn_clr_all_sky -- example host program: rrtmgpnn_allsky's problem, command line and cloud recipe
! (examples/all-sky/rrtmgp_allsky.F90:329-350) through mo_rrtmgp_clr_all_sky, which returns the clear-sky fluxes of
! the same columns beside the all-sky ones: per block one rte_lw call (cloud optics 1scl by band, LUT, ice roughness
! 2) and one rte_sw call (2str, delta-scaled), each doing gas optics once and solving twice -- the LW pair in one
! kernel.  The SW incident flux is the k-distribution's solar source renormalised to each column's TSI, as the RFMIP
! driver forms it (rrtmgp_rfmip_sw.F90:403-434), handed in as inc_flux.
!
! usage: rrtmgpnn_clr_all_sky <problem.rbin> <output.rbin> <data_dir> [block_size] [nc]
!   problem.rbin as for rrtmgpnn_rfmip_clear_sky; output.rbin holds lw_flux_up/dn, sw_flux_up/dn/dir (all sky) and the
!   same names with a _clr suffix (clear sky).  With "nc" the NN models and the cloud-optics
!   coefficients are the reference's own netCDF files, by their reference names, in data_dir (read by the
!   library's native readers: load_netcdf, load_cld_lutcoeff); otherwise their RBIN conversions.
program rrtmgpnn_clr_all_sky
  use mo_rte_kind,           only: wp
  use mo_optical_props,      only: ty_optical_props_1scl, ty_optical_props_2str
  use mo_fluxes,             only: ty_fluxes_flexible
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_gas_optics_rrtmgp,  only: ty_gas_optics_rrtmgp
  use mod_network_rrtmgp,    only: rrtmgp_network_type
  use mo_cloud_optics,       only: ty_cloud_optics
  use mo_load_cloud_coefficients, only: load_cld_lutcoeff
  use mo_rrtmgp_clr_all_sky, only: rte_lw, rte_sw
  use mo_rrtmgpnn_rbin
  implicit none

  character(len=512) :: problem_file, output_file, data_dir, arg
  real(wp), allocatable :: play(:,:), plev(:,:), tlay(:,:), tlev(:,:), tsfc(:), sfc_emis(:), sfc_alb(:)
  real(wp), allocatable :: mu0(:), tsi(:), usecol(:), scal(:), vmr(:,:)
  real(wp), allocatable :: lwp(:,:), iwp(:,:), rel(:,:), rei(:,:)
  character(len=32), allocatable :: gas_names(:)
  real(wp), allocatable, target :: lw_up(:,:), lw_dn(:,:), sw_up(:,:), sw_dn(:,:), sw_dir(:,:)
  real(wp), allocatable, target :: lw_up_clr(:,:), lw_dn_clr(:,:), sw_up_clr(:,:), sw_dn_clr(:,:), sw_dir_clr(:,:)
  real(wp), allocatable :: sfc_emis_spec(:,:), toa_flux(:,:), sfc_alb_spec(:,:), def_tsi(:)
  type(ty_gas_concs) :: gas_concs
  type(ty_gas_optics_rrtmgp) :: kdist_lw, kdist_sw
  type(rrtmgp_network_type), dimension(2) :: nets_lw, nets_sw
  type(ty_cloud_optics) :: cloud_optics_lw, cloud_optics_sw
  type(ty_optical_props_1scl) :: clouds_lw
  type(ty_optical_props_2str) :: clouds_sw
  type(ty_fluxes_flexible) :: fluxes, fluxes_clr
  character(len=128) :: e
  logical :: top_at_1, cloudy, nc
  real(wp) :: rel_val, rei_val
  integer :: ncol, nlay, ngas, nmus, block_size, b0, b1, nb, icol, ilay, igpt, ig, u

  if (command_argument_count() < 3) then
    write(*, '(a)') "usage: rrtmgpnn_clr_all_sky <problem.rbin> <output.rbin> <data_dir> [block_size] [nc]"
    stop 2
  end if
  call get_command_argument(1, problem_file)
  call get_command_argument(2, output_file)
  call get_command_argument(3, data_dir)
  block_size = 0
  if (command_argument_count() >= 4) then
    call get_command_argument(4, arg)
    read(arg, *) block_size
  end if
  nc = .false.
  if (command_argument_count() >= 5) then
    call get_command_argument(5, arg)
    nc = trim(arg) == "nc"
  end if

  call rbin_real2(problem_file, "play", play, e); call stop_on_err(e)
  call rbin_real2(problem_file, "plev", plev, e); call stop_on_err(e)
  call rbin_real2(problem_file, "tlay", tlay, e); call stop_on_err(e)
  call rbin_real2(problem_file, "tlev", tlev, e); call stop_on_err(e)
  call rbin_real1(problem_file, "tsfc", tsfc, e); call stop_on_err(e)
  call rbin_real1(problem_file, "sfc_emis", sfc_emis, e); call stop_on_err(e)
  call rbin_real1(problem_file, "sfc_alb", sfc_alb, e); call stop_on_err(e)
  call rbin_real1(problem_file, "mu0", mu0, e); call stop_on_err(e)
  call rbin_real1(problem_file, "tsi", tsi, e); call stop_on_err(e)
  call rbin_real1(problem_file, "usecol", usecol, e); call stop_on_err(e)
  call rbin_real1(problem_file, "top_at_1", scal, e); call stop_on_err(e)
  top_at_1 = scal(1) /= 0._wp
  call rbin_real1(problem_file, "n_gauss_angles", scal, e); call stop_on_err(e)
  nmus = nint(scal(1))
  call rbin_strings(problem_file, "gas_names", gas_names, e); call stop_on_err(e)
  nlay = size(play, 1)
  ncol = size(play, 2)
  ngas = size(gas_names)
  if (block_size <= 0) block_size = ncol

  if (nc) then  ! neural/data/ file names of the reference
    call nets_lw(1)%load_netcdf(trim(data_dir) // "/lw-g256-2018-12-04_absorption_58_58.nc")
    call nets_lw(2)%load_netcdf(trim(data_dir) // "/lw-g256-2018-12-04_planck_frac_16_16.nc")
    call nets_sw(1)%load_netcdf(trim(data_dir) // "/sw-g224-2018-12-04-absorption_16_16.nc")
    call nets_sw(2)%load_netcdf(trim(data_dir) // "/sw-g224-2018-12-04-rayleigh_16_16.nc")
  else
    call nets_lw(1)%load_netcdf(trim(data_dir) // "/nn_lw_g256_abs.rbin")
    call nets_lw(2)%load_netcdf(trim(data_dir) // "/nn_lw_g256_pfrac.rbin")
    call nets_sw(1)%load_netcdf(trim(data_dir) // "/nn_sw_g224_abs.rbin")
    call nets_sw(2)%load_netcdf(trim(data_dir) // "/nn_sw_g224_ray.rbin")
  end if
  call stop_on_err(kdist_lw%load_rbin(trim(data_dir) // "/kdist_lw_g256.rbin", gas_names))
  call stop_on_err(kdist_sw%load_rbin(trim(data_dir) // "/kdist_sw_g224.rbin", gas_names))
  call stop_on_err(kdist_sw%set_tsi(1361.0_wp))                  ! rrtmgp_rfmip_sw.F90:317
  if (nc) then  ! rrtmgp_allsky.F90:213-217
    call load_cld_lutcoeff(cloud_optics_lw, trim(data_dir) // "/rrtmgp-cloud-optics-coeffs-lw.nc")
    call load_cld_lutcoeff(cloud_optics_sw, trim(data_dir) // "/rrtmgp-cloud-optics-coeffs-sw.nc")
  else
    call stop_on_err(cloud_optics_lw%load_rbin(trim(data_dir) // "/cloud_optics_lw.rbin", .true.))
    call stop_on_err(cloud_optics_sw%load_rbin(trim(data_dir) // "/cloud_optics_sw.rbin", .true.))
  end if
  call stop_on_err(cloud_optics_lw%set_ice_roughness(2))         ! rrtmgp_allsky.F90:219
  call stop_on_err(cloud_optics_sw%set_ice_roughness(2))

  ! Clouds (rrtmgp_allsky.F90:329-350): between 100 and 900 hPa, in 2/3 of the columns
  allocate(lwp(nlay, ncol), iwp(nlay, ncol), rel(nlay, ncol), rei(nlay, ncol))
  rel_val = 0.5 * (cloud_optics_lw%get_min_radius_liq() + cloud_optics_lw%get_max_radius_liq())
  rei_val = 0.5 * (cloud_optics_lw%get_min_radius_ice() + cloud_optics_lw%get_max_radius_ice())
  do icol = 1, ncol
    do ilay = 1, nlay
      cloudy = play(ilay, icol) > 100._wp * 100._wp .and. play(ilay, icol) < 900._wp * 100._wp .and. &
               mod(icol, 3) /= 0
      lwp(ilay, icol) = merge(10._wp, 0._wp, cloudy .and. tlay(ilay, icol) > 263._wp)
      iwp(ilay, icol) = merge(10._wp, 0._wp, cloudy .and. tlay(ilay, icol) < 273._wp)
      rel(ilay, icol) = merge(rel_val, 0._wp, lwp(ilay, icol) > 0._wp)
      rei(ilay, icol) = merge(rei_val, 0._wp, iwp(ilay, icol) > 0._wp)
    end do
  end do

  allocate(lw_up(nlay + 1, ncol), lw_dn(nlay + 1, ncol), sw_up(nlay + 1, ncol), sw_dn(nlay + 1, ncol), &
           sw_dir(nlay + 1, ncol))
  allocate(lw_up_clr(nlay + 1, ncol), lw_dn_clr(nlay + 1, ncol), sw_up_clr(nlay + 1, ncol), &
           sw_dn_clr(nlay + 1, ncol), sw_dir_clr(nlay + 1, ncol))

  do b0 = 1, ncol, block_size
    b1 = min(ncol, b0 + block_size - 1)
    nb = b1 - b0 + 1
    call stop_on_err(gas_concs%init(gas_names))
    do ig = 1, ngas
      call rbin_real2(problem_file, "vmr_" // trim(gas_names(ig)), vmr, e); call stop_on_err(e)
      call stop_on_err(gas_concs%set_vmr(gas_names(ig), vmr(:, b0:b1)))
    end do

    ! ---- longwave: cloud optics, then gas optics + clear solve + increment + all-sky solve in rte_lw ----
    call stop_on_err(clouds_lw%alloc_1scl(nb, nlay, cloud_optics_lw))
    call stop_on_err(cloud_optics_lw%cloud_optics(lwp(:, b0:b1), iwp(:, b0:b1), rel(:, b0:b1), rei(:, b0:b1), &
                                                  clouds_lw))
    allocate(sfc_emis_spec(kdist_lw%get_nband(), nb))
    do icol = 1, nb
      sfc_emis_spec(:, icol) = sfc_emis(b0 + icol - 1)
    end do
    fluxes%flux_up => lw_up(:, b0:b1)
    fluxes%flux_dn => lw_dn(:, b0:b1)
    fluxes%flux_dn_dir => NULL()
    fluxes_clr%flux_up => lw_up_clr(:, b0:b1)
    fluxes_clr%flux_dn => lw_dn_clr(:, b0:b1)
    fluxes_clr%flux_dn_dir => NULL()
    call stop_on_err(rte_lw(kdist_lw, gas_concs, play(:, b0:b1), tlay(:, b0:b1), plev(:, b0:b1), tsfc(b0:b1), &
                            sfc_emis_spec, clouds_lw, fluxes, fluxes_clr, t_lev=tlev(:, b0:b1), n_gauss_angles=nmus, &
                            neural_nets=nets_lw))
    deallocate(sfc_emis_spec)

    ! ---- shortwave: cloud optics and delta scaling, then rte_sw with the TSI-normalised incident flux ----
    call stop_on_err(clouds_sw%alloc_2str(nb, nlay, cloud_optics_sw))
    call stop_on_err(cloud_optics_sw%cloud_optics(lwp(:, b0:b1), iwp(:, b0:b1), rel(:, b0:b1), rei(:, b0:b1), &
                                                  clouds_sw))
    allocate(toa_flux(kdist_sw%get_ngpt(), nb), sfc_alb_spec(kdist_sw%get_ngpt(), nb), def_tsi(nb))
    call stop_on_err(clouds_sw%delta_scale())
    do icol = 1, nb
      toa_flux(:, icol) = kdist_sw%solar_source(:)   ! gas_optics' toa_src (:594-599)
      def_tsi(icol) = 0._wp
      do igpt = 1, kdist_sw%get_ngpt()
        def_tsi(icol) = def_tsi(icol) + toa_flux(igpt, icol)
      end do
      do igpt = 1, kdist_sw%get_ngpt()
        toa_flux(igpt, icol) = toa_flux(igpt, icol) * tsi(b0 + icol - 1) / def_tsi(icol)
      end do
      sfc_alb_spec(:, icol) = sfc_alb(b0 + icol - 1)
    end do
    fluxes%flux_up => sw_up(:, b0:b1)
    fluxes%flux_dn => sw_dn(:, b0:b1)
    fluxes%flux_dn_dir => sw_dir(:, b0:b1)
    fluxes_clr%flux_up => sw_up_clr(:, b0:b1)
    fluxes_clr%flux_dn => sw_dn_clr(:, b0:b1)
    fluxes_clr%flux_dn_dir => sw_dir_clr(:, b0:b1)
    call stop_on_err(rte_sw(kdist_sw, gas_concs, play(:, b0:b1), tlay(:, b0:b1), plev(:, b0:b1), mu0(b0:b1), &
                            sfc_alb_spec, sfc_alb_spec, clouds_sw, fluxes, fluxes_clr, inc_flux=toa_flux, &
                            neural_nets=nets_sw))
    do icol = 1, nb
      if (usecol(b0 + icol - 1) == 0._wp) then
        sw_up(:, b0 + icol - 1) = 0._wp
        sw_dn(:, b0 + icol - 1) = 0._wp
        sw_up_clr(:, b0 + icol - 1) = 0._wp
        sw_dn_clr(:, b0 + icol - 1) = 0._wp
      end if
    end do
    deallocate(toa_flux, sfc_alb_spec, def_tsi)
  end do

  u = rbin_write_begin(output_file, 10)
  call rbin_write_real(u, "lw_flux_up", lw_up, shape(lw_up))
  call rbin_write_real(u, "lw_flux_dn", lw_dn, shape(lw_dn))
  call rbin_write_real(u, "sw_flux_up", sw_up, shape(sw_up))
  call rbin_write_real(u, "sw_flux_dn", sw_dn, shape(sw_dn))
  call rbin_write_real(u, "sw_flux_dir", sw_dir, shape(sw_dir))
  call rbin_write_real(u, "lw_flux_up_clr", lw_up_clr, shape(lw_up_clr))
  call rbin_write_real(u, "lw_flux_dn_clr", lw_dn_clr, shape(lw_dn_clr))
  call rbin_write_real(u, "sw_flux_up_clr", sw_up_clr, shape(sw_up_clr))
  call rbin_write_real(u, "sw_flux_dn_clr", sw_dn_clr, shape(sw_dn_clr))
  call rbin_write_real(u, "sw_flux_dir_clr", sw_dir_clr, shape(sw_dir_clr))
  call rbin_write_end(u)
  write(*, '(a,i0,a,i0,a)') "rrtmgpnn_clr_all_sky: ", ncol, " columns x ", nlay, " layers done"

contains
  subroutine stop_on_err(msg)
    character(len=*), intent(in) :: msg
    if (len_trim(msg) > 0) then
      write(*, '(a)') trim(msg)
      error stop 1
    end if
  end subroutine stop_on_err
end program rrtmgpnn_clr_all_sky
