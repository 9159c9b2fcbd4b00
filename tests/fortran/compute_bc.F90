! compute_bc.F90 -- mo_compute_bc's compute_bc through the Fortran drop-in (tests/test_fortran_compute_bc.py).
! usage: compute_bc <problem.rbin> <output.rbin> <data_dir>
!   (a) the longwave problem, the reference's behaviour (one angle: flux_bc is a radiance);
!   (b) the same with as_flux = .true. (the solver's 2 pi w applied: rte_lw's inc_flux);
!   (c) the shortwave problem with mu0;
!   (d) refusals, by the reference's strings: no mu0 for the solar problem (exit status 6 otherwise); the top level at the
!       gas optics' minimum pressure (7), flux_bc untouched; plev with one level too many (8).
program compute_bc_test
  use mo_rte_kind,           only: wp
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_gas_optics_rrtmgp,  only: ty_gas_optics_rrtmgp
  use mod_network_rrtmgp,    only: rrtmgp_network_type
  use mo_compute_bc,         only: compute_bc
  use mo_rrtmgpnn_rbin
  implicit none
  character(len=512) :: pfile, ofile, ddir
  real(wp), allocatable :: play(:,:), plev(:,:), tlay(:,:), mu0(:), vmr(:,:), pbad(:,:), plong(:,:)
  real(wp), allocatable :: bc_lw(:,:), bc_lw_flux(:,:), bc_sw(:,:), bad(:,:)
  character(len=32), allocatable :: gas_names(:)
  type(ty_gas_concs) :: gas_concs
  type(ty_gas_optics_rrtmgp) :: kd_lw, kd_sw
  type(rrtmgp_network_type), dimension(2) :: nets_lw, nets_sw
  character(len=128) :: e
  integer :: ncol, nlay, ig, u, top_lev
  real(wp), parameter :: mark = -7.5_wp

  call get_command_argument(1, pfile)
  call get_command_argument(2, ofile)
  call get_command_argument(3, ddir)
  call rbin_real2(pfile, "play", play, e); call chk(e)
  call rbin_real2(pfile, "plev", plev, e); call chk(e)
  call rbin_real2(pfile, "tlay", tlay, e); call chk(e)
  call rbin_real1(pfile, "mu0", mu0, e); call chk(e)
  call rbin_strings(pfile, "gas_names", gas_names, e); call chk(e)
  nlay = size(play, 1)
  ncol = size(play, 2)
  call chk(gas_concs%init(gas_names))
  do ig = 1, size(gas_names)
    call rbin_real2(pfile, "vmr_" // trim(gas_names(ig)), vmr, e); call chk(e)
    call chk(gas_concs%set_vmr(gas_names(ig), vmr))
  end do
  call nets_lw(1)%load_netcdf(trim(ddir) // "/nn_lw_g256_abs.rbin")
  call nets_lw(2)%load_netcdf(trim(ddir) // "/nn_lw_g256_pfrac.rbin")
  call nets_sw(1)%load_netcdf(trim(ddir) // "/nn_sw_g224_abs.rbin")
  call nets_sw(2)%load_netcdf(trim(ddir) // "/nn_sw_g224_ray.rbin")
  call chk(kd_lw%load_rbin(trim(ddir) // "/kdist_lw_g256.rbin", gas_names))
  call chk(kd_sw%load_rbin(trim(ddir) // "/kdist_sw_g224.rbin", gas_names))
  allocate(bc_lw(kd_lw%get_ngpt(), ncol), bc_lw_flux(kd_lw%get_ngpt(), ncol), bc_sw(kd_sw%get_ngpt(), ncol))
  ! (a), (b), (c)
  call chk(compute_bc(kd_lw, play, plev, tlay, gas_concs, bc_lw, neural_nets=nets_lw))
  call chk(compute_bc(kd_lw, play, plev, tlay, gas_concs, bc_lw_flux, neural_nets=nets_lw, as_flux=.true.))
  call chk(compute_bc(kd_sw, play, plev, tlay, gas_concs, bc_sw, mu0=mu0, neural_nets=nets_sw))
  ! (d)
  allocate(bad(kd_sw%get_ngpt(), ncol))
  bad = mark
  e = compute_bc(kd_sw, play, plev, tlay, gas_concs, bad, neural_nets=nets_sw)
  if (e /= "compute_bc: have to supply mu0 for solar calculations" .or. any(bad /= mark)) then
    write(*, '(a)') "compute_bc without mu0 returned: '" // trim(e) // "'"
    error stop 6
  end if
  top_lev = merge(1, nlay, play(1, 1) < play(nlay, 1))  ! the level the reference's check reads
  pbad = plev
  pbad(top_lev, :) = kd_sw%get_press_min() + 2._wp * spacing(kd_sw%get_press_min())
  e = compute_bc(kd_sw, play, pbad, tlay, gas_concs, bad, mu0=mu0, neural_nets=nets_sw)
  if (e /= "compute_bc: pressures are too close to (or less than) min in gas optics " .or. any(bad /= mark)) then
    write(*, '(a)') "compute_bc at the minimum pressure returned: '" // trim(e) // "'"
    error stop 7
  end if
  allocate(plong(nlay + 2, ncol))
  plong = 1000._wp
  e = compute_bc(kd_sw, play, plong, tlay, gas_concs, bad, mu0=mu0, neural_nets=nets_sw)
  if (e /= "compute_bc: array plev has wrong dimensions" .or. any(bad /= mark)) then
    write(*, '(a)') "compute_bc with a (nlay+2, ncol) plev returned: '" // trim(e) // "'"
    error stop 8
  end if
  u = rbin_write_begin(ofile, 3)
  call rbin_write_real(u, "bc_lw", bc_lw, shape(bc_lw))
  call rbin_write_real(u, "bc_lw_flux", bc_lw_flux, shape(bc_lw_flux))
  call rbin_write_real(u, "bc_sw", bc_sw, shape(bc_sw))
  call rbin_write_end(u)
contains
  subroutine chk(msg)
    character(len=*), intent(in) :: msg
    if (len_trim(msg) > 0) then
      write(*, '(a)') trim(msg)
      error stop 1
    end if
  end subroutine chk
end program compute_bc_test
