! lw_jacobian.F90 -- flux_up_Jac through the Fortran drop-in's rte_lw (tests/test_fortran_lw_jacobian.py).
! usage: lw_jacobian <problem.rbin> <output.rbin> <data_dir>
!   (off) compute_Jac off (the default): flux_up_Jac and flux_dn_Jac are accepted and left untouched (exit status 5
!         otherwise);
!   rte_rrtmgp_config_jacobian(.true.), then
!   (a) rte_lw, one angle, on the gas-optics output (Planck sources deferred: the fused-Planck solver forms
!       sfc_source_Jac in-kernel): flux_up/dn, flux_up_Jac;
!   (b) the same with three angles;
!   (c) rte_lw on two-stream properties tau = tau_a, ssa = 0.5, g = 0.3 (the rescaled solution, sources formed from the
!       deferred Planck sources): flux_up/dn, flux_up_Jac;
!   (d) the sources on the host (update_host / update_device: no longer deferred), one angle: sfc_source_Jac is read;
!   (e) no flux_up_Jac: "rte_lw: compute_Jac=true but Jacobian arrays not provided" (exit status 6 otherwise); one level
!       too many: "rte_lw: flux Jacobian inconsistently sized" (7), the array untouched; flux_dn_Jac stays untouched in
!       (a) (8).
program lw_jacobian
  use mo_rte_kind,           only: wp, wl
  use mo_optical_props,      only: ty_optical_props_1scl, ty_optical_props_2str
  use mo_source_functions,   only: ty_source_func_lw
  use mo_fluxes,             only: ty_fluxes_flexible
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_gas_optics_rrtmgp,  only: ty_gas_optics_rrtmgp
  use mod_network_rrtmgp,    only: rrtmgp_network_type
  use mo_rte_rrtmgp_config,  only: rte_rrtmgp_config_jacobian, compute_Jac
  use mo_rte_lw,             only: rte_lw
  use mo_rrtmgpnn_rbin
  implicit none
  character(len=512) :: pfile, ofile, ddir
  real(wp), allocatable :: play(:,:), plev(:,:), tlay(:,:), tlev(:,:), tsfc(:), sfc_emis(:), scal(:), vmr(:,:)
  real(wp), allocatable :: emis(:,:), tau0(:,:,:)
  real(wp), allocatable, target :: up(:,:), dn(:,:), up_a(:,:), dn_a(:,:), up_b(:,:), dn_b(:,:), up_c(:,:), dn_c(:,:)
  real(wp), allocatable, target :: up_d(:,:), dn_d(:,:)
  real(wp), allocatable :: jac_off(:,:), jdn(:,:), jac_a(:,:), jac_b(:,:), jac_c(:,:), jac_d(:,:), bad(:,:)
  character(len=32), allocatable :: gas_names(:)
  type(ty_gas_concs) :: gas_concs
  type(ty_gas_optics_rrtmgp) :: kdist
  type(rrtmgp_network_type), dimension(2) :: nets
  type(ty_optical_props_1scl) :: op
  type(ty_optical_props_2str) :: op2
  type(ty_source_func_lw) :: src
  type(ty_fluxes_flexible) :: f0, fa, fb, fc, fd
  character(len=128) :: e
  integer :: ncol, nlay, nlev, nbnd, ig, icol, u
  logical :: top_at_1
  real(wp), parameter :: mark = -7.5_wp

  call get_command_argument(1, pfile)
  call get_command_argument(2, ofile)
  call get_command_argument(3, ddir)
  call rbin_real2(pfile, "play", play, e); call chk(e)
  call rbin_real2(pfile, "plev", plev, e); call chk(e)
  call rbin_real2(pfile, "tlay", tlay, e); call chk(e)
  call rbin_real2(pfile, "tlev", tlev, e); call chk(e)
  call rbin_real1(pfile, "tsfc", tsfc, e); call chk(e)
  call rbin_real1(pfile, "sfc_emis", sfc_emis, e); call chk(e)
  call rbin_real1(pfile, "top_at_1", scal, e); call chk(e)
  top_at_1 = scal(1) /= 0._wp
  call rbin_strings(pfile, "gas_names", gas_names, e); call chk(e)
  nlay = size(play, 1)
  nlev = nlay + 1
  ncol = size(play, 2)
  call chk(gas_concs%init(gas_names))
  do ig = 1, size(gas_names)
    call rbin_real2(pfile, "vmr_" // trim(gas_names(ig)), vmr, e); call chk(e)
    call chk(gas_concs%set_vmr(gas_names(ig), vmr))
  end do
  call nets(1)%load_netcdf(trim(ddir) // "/nn_lw_g256_abs.rbin")
  call nets(2)%load_netcdf(trim(ddir) // "/nn_lw_g256_pfrac.rbin")
  call chk(kdist%load_rbin(trim(ddir) // "/kdist_lw_g256.rbin", gas_names))
  call chk(op%alloc_1scl(ncol, nlay, kdist))
  call chk(src%alloc(ncol, nlay, kdist))
  nbnd = kdist%get_nband()
  allocate(emis(nbnd, ncol))
  do icol = 1, ncol
    emis(:, icol) = sfc_emis(icol)
  end do
  call chk(kdist%gas_optics(play, plev, tlay, tsfc, gas_concs, op, src, tlev=tlev, neural_nets=nets))
  ! (off)
  if (compute_Jac) error stop 5
  allocate(up(nlev, ncol), dn(nlev, ncol), jac_off(nlev, ncol), jdn(nlev, ncol))
  jac_off = mark
  jdn = mark
  f0%flux_up => up
  f0%flux_dn => dn
  call chk(rte_lw(op, top_at_1, src, emis, f0, flux_up_Jac=jac_off, flux_dn_Jac=jdn))
  if (any(jac_off /= mark) .or. any(jdn /= mark)) error stop 5
  call rte_rrtmgp_config_jacobian(.true._wl)
  ! (a)
  allocate(up_a(nlev, ncol), dn_a(nlev, ncol), jac_a(nlev, ncol))
  fa%flux_up => up_a
  fa%flux_dn => dn_a
  call chk(rte_lw(op, top_at_1, src, emis, fa, flux_up_Jac=jac_a, flux_dn_Jac=jdn))
  if (any(jdn /= mark)) error stop 8
  ! (b)
  allocate(up_b(nlev, ncol), dn_b(nlev, ncol), jac_b(nlev, ncol))
  fb%flux_up => up_b
  fb%flux_dn => dn_b
  call chk(rte_lw(op, top_at_1, src, emis, fb, n_gauss_angles=3, flux_up_Jac=jac_b))
  ! (c)
  call op%update_host()
  tau0 = op%tau
  call chk(op2%alloc_2str(ncol, nlay, kdist))
  op2%tau = tau0
  op2%ssa = 0.5_wp
  op2%g = 0.3_wp
  allocate(up_c(nlev, ncol), dn_c(nlev, ncol), jac_c(nlev, ncol))
  fc%flux_up => up_c
  fc%flux_dn => dn_c
  call chk(rte_lw(op2, top_at_1, src, emis, fc, flux_up_Jac=jac_c))
  ! (e)
  e = rte_lw(op, top_at_1, src, emis, f0)
  if (e /= "rte_lw: compute_Jac=true but Jacobian arrays not provided") then
    write(*, '(a)') "rte_lw without flux_up_Jac returned: '" // trim(e) // "'"
    error stop 6
  end if
  allocate(bad(nlev + 1, ncol))
  bad = mark
  e = rte_lw(op, top_at_1, src, emis, f0, flux_up_Jac=bad)
  if (e /= "rte_lw: flux Jacobian inconsistently sized" .or. any(bad /= mark)) then
    write(*, '(a)') "rte_lw with a (nlev+1, ncol) flux_up_Jac returned: '" // trim(e) // "'"
    error stop 7
  end if
  ! (d)
  call src%update_host()
  call src%update_device()
  allocate(up_d(nlev, ncol), dn_d(nlev, ncol), jac_d(nlev, ncol))
  fd%flux_up => up_d
  fd%flux_dn => dn_d
  call chk(rte_lw(op, top_at_1, src, emis, fd, flux_up_Jac=jac_d))
  call rte_rrtmgp_config_jacobian(.false._wl)
  u = rbin_write_begin(ofile, 15)
  call rbin_write_real(u, "flux_up_off", up, shape(up))
  call rbin_write_real(u, "flux_dn_off", dn, shape(dn))
  call rbin_write_real(u, "flux_up_a", up_a, shape(up_a))
  call rbin_write_real(u, "flux_dn_a", dn_a, shape(dn_a))
  call rbin_write_real(u, "jac_a", jac_a, shape(jac_a))
  call rbin_write_real(u, "flux_up_b", up_b, shape(up_b))
  call rbin_write_real(u, "flux_dn_b", dn_b, shape(dn_b))
  call rbin_write_real(u, "jac_b", jac_b, shape(jac_b))
  call rbin_write_real(u, "flux_up_c", up_c, shape(up_c))
  call rbin_write_real(u, "flux_dn_c", dn_c, shape(dn_c))
  call rbin_write_real(u, "jac_c", jac_c, shape(jac_c))
  call rbin_write_real(u, "flux_up_d", up_d, shape(up_d))
  call rbin_write_real(u, "flux_dn_d", dn_d, shape(dn_d))
  call rbin_write_real(u, "jac_d", jac_d, shape(jac_d))
  call rbin_write_real(u, "tau", tau0, shape(tau0))
  call rbin_write_end(u)
contains
  subroutine chk(msg)
    character(len=*), intent(in) :: msg
    if (len_trim(msg) > 0) then
      write(*, '(a)') trim(msg)
      error stop 1
    end if
  end subroutine chk
end program lw_jacobian
