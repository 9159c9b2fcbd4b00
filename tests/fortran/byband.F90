! byband.F90 -- ty_fluxes_byband through the Fortran drop-in's rte_lw / rte_sw (tests/test_fortran_byband.py).
! usage: byband <problem.rbin> <output.rbin> <data_dir>
!   (a) rte_lw, one angle, on the gas-optics output (Planck sources deferred: the fused-Planck solver forms the band
!       sums itself): flux_up/dn, bnd_flux_up/dn/net;
!   (b) rte_lw, three angles, with g-point fluxes too (the g-point arrays are reduced with rrtmgpnn_sum_byband);
!   (c) rte_lw, one angle, with g-point fluxes too (radiances: the solver runs again with the by-band request);
!   (d) rte_sw on two-stream properties tau = 0.1 tau_a, ssa = 0.5, g = 0.3 (mu0 = 0.6, inc_flux = 1, albedos 0.2):
!       flux_up/dn/dn_dir, bnd_flux_up/dn/dn_dir/net;
!   (e) a bnd_flux_up with one band too many is refused with reduce_byband's message (exit status 6), a bnd_flux_dn_dir
!       handed to rte_lw likewise (7), a bnd_flux_net without bnd_flux_dn (8); the caller's array untouched.
program byband
  use mo_rte_kind,           only: wp
  use mo_optical_props,      only: ty_optical_props_1scl, ty_optical_props_2str
  use mo_source_functions,   only: ty_source_func_lw
  use mo_fluxes_byband,      only: ty_fluxes_byband
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_gas_optics_rrtmgp,  only: ty_gas_optics_rrtmgp
  use mod_network_rrtmgp,    only: rrtmgp_network_type
  use mo_rte_lw,             only: rte_lw
  use mo_rte_sw,             only: rte_sw
  use mo_rrtmgpnn_rbin
  implicit none
  character(len=512) :: pfile, ofile, ddir
  real(wp), allocatable :: play(:,:), plev(:,:), tlay(:,:), tlev(:,:), tsfc(:), sfc_emis(:), scal(:), vmr(:,:)
  real(wp), allocatable :: emis(:,:), tau0(:,:,:), inc(:,:), alb(:,:), mu0(:)
  real(wp), allocatable, target :: up_a(:,:), dn_a(:,:), bup_a(:,:,:), bdn_a(:,:,:), bnet_a(:,:,:)
  real(wp), allocatable, target :: up_b(:,:), dn_b(:,:), bup_b(:,:,:), bdn_b(:,:,:), gup_b(:,:,:), gdn_b(:,:,:)
  real(wp), allocatable, target :: up_c(:,:), dn_c(:,:), bup_c(:,:,:), bdn_c(:,:,:), gup_c(:,:,:), gdn_c(:,:,:)
  real(wp), allocatable, target :: up_d(:,:), dn_d(:,:), dir_d(:,:)
  real(wp), allocatable, target :: bup_d(:,:,:), bdn_d(:,:,:), bdir_d(:,:,:), bnet_d(:,:,:), bad(:,:,:)
  character(len=32), allocatable :: gas_names(:)
  type(ty_gas_concs) :: gas_concs
  type(ty_gas_optics_rrtmgp) :: kdist
  type(rrtmgp_network_type), dimension(2) :: nets
  type(ty_optical_props_1scl) :: op
  type(ty_optical_props_2str) :: op2
  type(ty_source_func_lw) :: src
  type(ty_fluxes_byband) :: fa, fb, fc, fd, fe
  character(len=128) :: e
  integer :: ncol, nlay, nlev, ngpt, nbnd, ig, icol, u
  logical :: top_at_1

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
  ngpt = kdist%get_ngpt()
  nbnd = kdist%get_nband()
  allocate(emis(nbnd, ncol))
  do icol = 1, ncol
    emis(:, icol) = sfc_emis(icol)
  end do
  call chk(kdist%gas_optics(play, plev, tlay, tsfc, gas_concs, op, src, tlev=tlev, neural_nets=nets))
  ! (a)
  allocate(up_a(nlev, ncol), dn_a(nlev, ncol), bup_a(nbnd, nlev, ncol), bdn_a(nbnd, nlev, ncol), bnet_a(nbnd, nlev, ncol))
  fa%flux_up => up_a
  fa%flux_dn => dn_a
  fa%bnd_flux_up => bup_a
  fa%bnd_flux_dn => bdn_a
  fa%bnd_flux_net => bnet_a
  call chk(rte_lw(op, top_at_1, src, emis, fa))
  ! (b)
  allocate(up_b(nlev, ncol), dn_b(nlev, ncol), bup_b(nbnd, nlev, ncol), bdn_b(nbnd, nlev, ncol))
  allocate(gup_b(ngpt, nlev, ncol), gdn_b(ngpt, nlev, ncol))
  fb%flux_up => up_b
  fb%flux_dn => dn_b
  fb%bnd_flux_up => bup_b
  fb%bnd_flux_dn => bdn_b
  fb%gpt_flux_up => gup_b
  fb%gpt_flux_dn => gdn_b
  call chk(rte_lw(op, top_at_1, src, emis, fb, n_gauss_angles=3))
  ! (c)
  allocate(up_c(nlev, ncol), dn_c(nlev, ncol), bup_c(nbnd, nlev, ncol), bdn_c(nbnd, nlev, ncol))
  allocate(gup_c(ngpt, nlev, ncol), gdn_c(ngpt, nlev, ncol))
  fc%flux_up => up_c
  fc%flux_dn => dn_c
  fc%bnd_flux_up => bup_c
  fc%bnd_flux_dn => bdn_c
  fc%gpt_flux_up => gup_c
  fc%gpt_flux_dn => gdn_c
  call chk(rte_lw(op, top_at_1, src, emis, fc))
  ! (d)
  call op%update_host()
  tau0 = op%tau
  call chk(op2%alloc_2str(ncol, nlay, kdist))
  op2%tau = 0.1_wp * tau0
  op2%ssa = 0.5_wp
  op2%g = 0.3_wp
  allocate(inc(ngpt, ncol), alb(ngpt, ncol), mu0(ncol))
  inc = 1._wp
  alb = 0.2_wp
  mu0 = 0.6_wp
  allocate(up_d(nlev, ncol), dn_d(nlev, ncol), dir_d(nlev, ncol))
  allocate(bup_d(nbnd, nlev, ncol), bdn_d(nbnd, nlev, ncol), bdir_d(nbnd, nlev, ncol), bnet_d(nbnd, nlev, ncol))
  fd%flux_up => up_d
  fd%flux_dn => dn_d
  fd%flux_dn_dir => dir_d
  fd%bnd_flux_up => bup_d
  fd%bnd_flux_dn => bdn_d
  fd%bnd_flux_dn_dir => bdir_d
  fd%bnd_flux_net => bnet_d
  call chk(rte_sw(op2, top_at_1, mu0, inc, alb, alb, fd))
  ! (e)
  allocate(bad(nbnd + 1, nlev, ncol))
  bad = -3._wp
  fe%flux_up => up_a
  fe%bnd_flux_up => bad
  e = rte_lw(op, top_at_1, src, emis, fe)
  if (e /= "reduce: bnd_flux_up array incorrectly sized (can't compute net flux either)" .or. any(bad /= -3._wp)) then
    write(*, '(a)') "rte_lw with a (nbnd+1, nlev, ncol) bnd_flux_up returned: '" // trim(e) // "'"
    error stop 6
  end if
  fe%bnd_flux_up => bup_a
  fe%bnd_flux_dn_dir => bdir_d
  e = rte_lw(op, top_at_1, src, emis, fe)
  if (e /= "reduce: requesting bnd_flux_dn_dir but direct flux hasn't been supplied") then
    write(*, '(a)') "rte_lw with bnd_flux_dn_dir returned: '" // trim(e) // "'"
    error stop 7
  end if
  fe%bnd_flux_dn_dir => NULL()
  fe%bnd_flux_net => bnet_a
  e = rte_lw(op, top_at_1, src, emis, fe)
  if (e /= "reduce: bnd_flux_net needs bnd_flux_up and bnd_flux_dn (net_byband_full is not provided)") then
    write(*, '(a)') "rte_lw with bnd_flux_net but no bnd_flux_dn returned: '" // trim(e) // "'"
    error stop 8
  end if
  u = rbin_write_begin(ofile, 25)
  call rbin_write_real(u, "flux_up_a", up_a, shape(up_a))
  call rbin_write_real(u, "flux_dn_a", dn_a, shape(dn_a))
  call rbin_write_real(u, "bnd_up_a", bup_a, shape(bup_a))
  call rbin_write_real(u, "bnd_dn_a", bdn_a, shape(bdn_a))
  call rbin_write_real(u, "bnd_net_a", bnet_a, shape(bnet_a))
  call rbin_write_real(u, "flux_up_b", up_b, shape(up_b))
  call rbin_write_real(u, "flux_dn_b", dn_b, shape(dn_b))
  call rbin_write_real(u, "bnd_up_b", bup_b, shape(bup_b))
  call rbin_write_real(u, "bnd_dn_b", bdn_b, shape(bdn_b))
  call rbin_write_real(u, "gpt_up_b", gup_b, shape(gup_b))
  call rbin_write_real(u, "gpt_dn_b", gdn_b, shape(gdn_b))
  call rbin_write_real(u, "flux_up_c", up_c, shape(up_c))
  call rbin_write_real(u, "flux_dn_c", dn_c, shape(dn_c))
  call rbin_write_real(u, "bnd_up_c", bup_c, shape(bup_c))
  call rbin_write_real(u, "bnd_dn_c", bdn_c, shape(bdn_c))
  call rbin_write_real(u, "gpt_up_c", gup_c, shape(gup_c))
  call rbin_write_real(u, "gpt_dn_c", gdn_c, shape(gdn_c))
  call rbin_write_real(u, "flux_up_d", up_d, shape(up_d))
  call rbin_write_real(u, "flux_dn_d", dn_d, shape(dn_d))
  call rbin_write_real(u, "flux_dir_d", dir_d, shape(dir_d))
  call rbin_write_real(u, "bnd_up_d", bup_d, shape(bup_d))
  call rbin_write_real(u, "bnd_dn_d", bdn_d, shape(bdn_d))
  call rbin_write_real(u, "bnd_dir_d", bdir_d, shape(bdir_d))
  call rbin_write_real(u, "bnd_net_d", bnet_d, shape(bnet_d))
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
end program byband
