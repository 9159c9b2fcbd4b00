! mo_rrtmgp_clr_all_sky -- drop-in for extensions/mo_rrtmgp_clr_all_sky.F90: rte_lw and rte_sw that start from
! pressures, temperatures and gas amounts and return clear-sky (gases + optional aerosols) and all-sky fluxes.
! Both follow the reference's sequence (:146-172 LW, :274-308 SW): gas optics once, aer_props%increment(optical_props),
! the clear solve into clrsky_fluxes, cloud_props%increment(optical_props), the all-sky solve into allsky_fluxes.
! Argument lists and error strings are the reference's (typos included), in this layer's array layout ((nlay, ncol),
! (ngpt, ncol), ...); ty_gas_optics_rrtmgp stands where the reference has the abstract ty_gas_optics, the flux objects
! are this layer's ty_fluxes_flexible (or an extension), the SW albedos are per g-point as this layer's rte_sw takes
! them, and the networks go in as the trailing neural_nets, as gas_optics takes them.
!
! rte_lw takes the library's dual entry (rrtmgpnn_lw_solver_noscat_planck_clr_all: tau, the Planck fraction and the
! band cloud optical depth read once, both flux sets from one kernel with one angle) when the cloud properties are
! 1scl and defined by band on the k-distribution's bands, gas optics left the Planck sources unformed
! (ty_source_func_lw%planck_deferred), and both flux objects want broadband up / down fluxes only.  With 2str clouds
! (LW scattering: the rescaled solver) in the same situation, without aerosols or with aerosols of the fused kind, it
! takes the fused scattering route: gas optics into a 1scl object (no ssa / g arrays), the clear solve
! rrtmgpnn_lw_solver_noscat_planck (the rescaled solver with ssa = g = 0 is the no-scattering one, bit for bit) and the
! all-sky solve rrtmgpnn_lw_solver_1rescl_planck_inc, which increments tau by the two-stream band cloud as it reads it;
! with the aerosols one call of rrtmgpnn_lw_solver_1rescl_planck_clr_all under the aerosol request gives both sets, the
! clear sky gases + aerosols.  Every other case -- 2str
! clouds with other aerosols, clouds on g-points, g-point, by-band or net outputs -- runs the two solves with
! mo_rte_lw's rte_lw.  rte_sw always runs the two solves.
!
! aer_props: where rte_lw takes the dual entry and the aerosols are of the fused kind (1scl, defined by band on the
! k-distribution's bands, the same ncol and nlay), they are not added to the g-point array by aer_props%increment but
! armed as the solver's aerosol request (rrtmgpnn_solver_request_aerosol), and the kernel adds them, then the clouds,
! as it reads tau: the clear-sky fluxes are those of tau + tau_aer(band), the all-sky ones those of that + the cloud's,
! bit for bit the reference's sequence.  Every other case (2str or g-point aerosols, no dual entry) keeps
! aer_props%increment; so does rte_sw, which calls no fused increment entry.
module mo_rrtmgp_clr_all_sky
  use, intrinsic :: iso_c_binding
  use mo_rte_kind,           only: wp
  use mo_gas_optics_rrtmgp,  only: ty_gas_optics_rrtmgp
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_optical_props,      only: ty_optical_props_arry, ty_optical_props_1scl, ty_optical_props_2str
  use mo_source_functions,   only: ty_source_func_lw
  use mo_fluxes,             only: ty_fluxes_flexible
  use mo_fluxes_byband,      only: ty_fluxes_byband
  use mod_network_rrtmgp,    only: rrtmgp_network_type
  use mo_rte_lw,             only: base_rte_lw => rte_lw
  use mo_rte_sw,             only: base_rte_sw => rte_sw
  use mo_rrtmgpnn_c
  implicit none
  private
  public :: rte_lw, rte_sw

  ! Diffusivity angle and Gauss-Jacobi-5 quadrature, as mo_rte_lw holds them (rte/mo_rte_lw.F90:113-125)
  real(c_float), parameter, dimension(4, 4) :: &
    gauss_Ds  = reshape([1.66_wp,         0._wp,           0._wp,           0._wp, &
                         1.18350343_wp,   2.81649655_wp,   0._wp,           0._wp, &
                         1.09719858_wp,   1.69338507_wp,   4.70941630_wp,   0._wp, &
                         1.06056257_wp,   1.38282560_wp,   2.40148179_wp,   7.15513024_wp], [4, 4]), &
    gauss_wts = reshape([0.5_wp,          0._wp,           0._wp,           0._wp, &
                         0.3180413817_wp, 0.1819586183_wp, 0._wp,           0._wp, &
                         0.2009319137_wp, 0.2292411064_wp, 0.0698269799_wp, 0._wp, &
                         0.1355069134_wp, 0.2034645680_wp, 0.1298475476_wp, 0.0311809710_wp], [4, 4])

contains

  function rte_lw(k_dist, gas_concs, p_lay, t_lay, p_lev, t_sfc, sfc_emis, cloud_props, allsky_fluxes, clrsky_fluxes, &
                  aer_props, col_dry, t_lev, inc_flux, n_gauss_angles, neural_nets) result(error_msg)
    class(ty_gas_optics_rrtmgp),  intent(in) :: k_dist
    type(ty_gas_concs),           intent(in) :: gas_concs
    real(wp), dimension(:,:),     intent(in) :: p_lay, t_lay   ! (nlay, ncol)
    real(wp), dimension(:,:),     intent(in) :: p_lev          ! (nlay+1, ncol)
    real(wp), dimension(:),       intent(in) :: t_sfc          ! (ncol)
    real(wp), dimension(:,:),     intent(in) :: sfc_emis       ! (nband, ncol)
    class(ty_optical_props_arry), intent(in) :: cloud_props
    class(ty_fluxes_flexible), intent(inout) :: allsky_fluxes, clrsky_fluxes
    class(ty_optical_props_arry), optional, intent(in) :: aer_props
    real(wp), dimension(:,:), optional, intent(in) :: col_dry  ! (nlay, ncol)
    real(wp), dimension(:,:), optional, intent(in) :: t_lev    ! (nlay+1, ncol)
    real(wp), dimension(:,:), contiguous, target, optional, intent(in) :: inc_flux   ! (ngpt, ncol)
    integer,  optional, intent(in) :: n_gauss_angles
    type(rrtmgp_network_type), dimension(:), optional, intent(in) :: neural_nets
    character(len=128) :: error_msg
    class(ty_optical_props_arry), allocatable :: optical_props
    type(ty_source_func_lw) :: sources
    integer :: ncol, nlay, ngpt, nband, nmus
    logical :: top_at_1, dual, aer_req, scat, aer_scat

    error_msg = ""
    ncol  = size(p_lay, 2)
    nlay  = size(p_lay, 1)
    ngpt  = k_dist%get_ngpt()
    nband = k_dist%get_nband()
    top_at_1 = p_lay(1, 1) < p_lay(nlay, 1)

    if (present(aer_props)) error_msg = aer_check(aer_props, "rrtmpg_lw: aerosol properties inconsistently sized")
    if (present(t_lev)) then
      if (any(shape(t_lev) /= [nlay + 1, ncol])) error_msg = "rrtmpg_lw: t_lev inconsistently sized"
    end if
    if (present(inc_flux)) then
      if (any(shape(inc_flux) /= [ngpt, ncol])) error_msg = "rrtmpg_lw: incident flux inconsistently sized"
    end if
    if (len_trim(error_msg) > 0) return

    ! optical properties of the clouds' class on the k-distribution's spectral grid (:117-137)
    select type (cloud_props)
    class is (ty_optical_props_1scl)
      allocate(ty_optical_props_1scl :: optical_props)
    class is (ty_optical_props_2str)
      allocate(ty_optical_props_2str :: optical_props)
    class default
      error_msg = "lw_solver(...ty_optical_props_nstr...) not yet implemented"; return
    end select
    error_msg = optical_props%init(k_dist)
    if (len_trim(error_msg) > 0) return
    nmus = 1
    if (present(n_gauss_angles)) nmus = n_gauss_angles
    ! scattering clouds by band, broadband fluxes, no aerosols or aerosols of the fused kind (1scl, by band on the
    ! k-distribution's bands, the call's extents: they go to the solver as its aerosol request): the gas atmosphere stays
    ! 1scl (its ssa and g are the solver's literal zeros, never arrays)
    scat = .false.
    aer_scat = .false.
    if (present(aer_props)) then
      select type (aer_props)
      class is (ty_optical_props_1scl)
        aer_scat = aer_props%bands_are_equal(optical_props) .and. .not. aer_props%gpoints_are_equal(optical_props) .and. &
                   aer_props%get_ngpt() == nband .and. aer_props%get_ncol() == ncol .and. aer_props%get_nlay() == nlay
      end select
    end if
    select type (cloud_props)
    class is (ty_optical_props_2str)
      scat = (.not. present(aer_props) .or. aer_scat) .and. cloud_props%bands_are_equal(optical_props) .and. &
             .not. cloud_props%gpoints_are_equal(optical_props) .and. cloud_props%get_ngpt() == nband .and. &
             cloud_props%get_ncol() == ncol .and. cloud_props%get_nlay() == nlay .and. &
             broadband_only(allsky_fluxes) .and. broadband_only(clrsky_fluxes) .and. nmus >= 1 .and. nmus <= 4 .and. &
             all(shape(sfc_emis) == [nband, ncol])
    end select
    if (scat) then
      deallocate(optical_props)
      allocate(ty_optical_props_1scl :: optical_props)
      error_msg = optical_props%init(k_dist)
      if (len_trim(error_msg) > 0) return
    end if
    select type (optical_props)
    class is (ty_optical_props_1scl)
      error_msg = optical_props%alloc_1scl(ncol, nlay)
    class is (ty_optical_props_2str)
      error_msg = optical_props%alloc_2str(ncol, nlay)
    end select
    if (error_msg /= '') return
    error_msg = sources%alloc(ncol, nlay, k_dist)
    if (error_msg /= '') return

    ! gas optics once (:150-153)
    error_msg = k_dist%gas_optics(p_lay, p_lev, t_lay, t_sfc, gas_concs, optical_props, sources, col_dry, t_lev, &
                                  neural_nets)
    if (error_msg /= '') return

    if (scat .and. .not. sources%planck_deferred) then
      error_msg = "rte_lw: gas optics left the Planck sources formed; the fused scattering solve forms them itself"
      return
    end if
    dual = .false.
    select type (cloud_props)
    class is (ty_optical_props_1scl)
      dual = sources%planck_deferred .and. cloud_props%bands_are_equal(optical_props) .and. &
             .not. cloud_props%gpoints_are_equal(optical_props) .and. cloud_props%get_ngpt() == nband .and. &
             cloud_props%get_ncol() == ncol .and. cloud_props%get_nlay() == nlay .and. &
             broadband_only(allsky_fluxes) .and. broadband_only(clrsky_fluxes) .and. nmus >= 1 .and. nmus <= 4 .and. &
             all(shape(sfc_emis) == [nband, ncol])
    end select
    ! the aerosols (:157).  In the dual case, aerosols of the fused kind -- 1scl, by band on the k-distribution's bands,
    ! the same extents -- go to the solver as its aerosol request (rrtmgpnn_solver_request_aerosol: tau + tau_aer(band),
    ! then + the cloud's, as tau is read; the same two increments in the same order, the same bits); every other case
    ! adds them to the g-point array here
    aer_req = .false.
    if (present(aer_props) .and. dual) then
      select type (aer_props)
      class is (ty_optical_props_1scl)
        aer_req = aer_props%bands_are_equal(optical_props) .and. .not. aer_props%gpoints_are_equal(optical_props) .and. &
                  aer_props%get_ngpt() == nband .and. aer_props%get_ncol() == ncol .and. aer_props%get_nlay() == nlay
      end select
    end if
    if (present(aer_props) .and. .not. aer_req .and. .not. (scat .and. aer_scat)) &
      error_msg = aer_props%increment(optical_props)
    if (error_msg /= '') return
    if (dual) then
      error_msg = allsky_fluxes%check_extents(nlay + 1, ncol)
      if (error_msg == '') error_msg = clrsky_fluxes%check_extents(nlay + 1, ncol)
      if (error_msg /= '') return
      call solve_dual()
    else if (scat) then
      error_msg = allsky_fluxes%check_extents(nlay + 1, ncol)
      if (error_msg == '') error_msg = clrsky_fluxes%check_extents(nlay + 1, ncol)
      if (error_msg /= '') return
      call solve_scat()
    else
      ! the clear solve, clouds%increment, the all-sky solve (:160-172)
      error_msg = base_rte_lw(optical_props, top_at_1, sources, sfc_emis, clrsky_fluxes, inc_flux, n_gauss_angles)
      if (error_msg /= '') return
      error_msg = cloud_props%increment(optical_props)
      if (error_msg /= '') return
      error_msg = base_rte_lw(optical_props, top_at_1, sources, sfc_emis, allsky_fluxes, inc_flux, n_gauss_angles)
    end if
    call sources%finalize()

  contains

    function aer_check(aer, msg) result(e)
      class(ty_optical_props_arry), intent(in) :: aer
      character(len=*), intent(in) :: msg
      character(len=128) :: e
      e = ""
      if (any([aer%get_ncol(), aer%get_nlay()] /= [ncol, nlay])) e = msg
      if (.not. any(aer%get_ngpt() /= [ngpt, nband])) e = msg   ! as written in the reference (:97-98)
    end function aer_check

    ! both flux sets from one call: the clear solve of tau and the all-sky solve of tau + cloud tau(band), sources
    ! formed in the solver from the Planck fraction gas optics left in lay_source
    subroutine solve_dual()
      integer(c_long_long) :: ng, nv
      integer(c_int), allocatable :: lims(:,:)
      type(c_ptr) :: d_emis, d_inc, d_up, d_dn, d_upc, d_dnc
      lims = optical_props%get_band_lims_gpoint()
      ng = int(ngpt, c_long_long) * nlay * ncol
      nv = int(nlay + 1, c_long_long) * ncol
      d_emis = dev_stage(sfc_emis, int(nband, c_long_long) * ncol)
      d_inc = c_null_ptr
      if (present(inc_flux)) d_inc = dev_stage(inc_flux, int(ngpt, c_long_long) * ncol)
      d_up = dev_scratch(nv); d_dn = dev_scratch(nv); d_upc = dev_scratch(nv); d_dnc = dev_scratch(nv)
      ! armed for the solver call below, which clears it whatever it returns
      if (aer_req) error_msg = rrtmgpnn_check(c_rrtmgpnn_solver_request_aerosol(rrtmgpnn_ctx(), nband, nlay, ncol, &
                    dev_present(aer_props%tau, size(aer_props%tau, kind=c_long_long), PRESENT_READ), c_null_ptr, &
                    c_null_ptr), "rte_lw: solver_request_aerosol")
      if (error_msg == '') &
      error_msg = rrtmgpnn_check(c_rrtmgpnn_lw_solver_noscat_planck_clr_all(rrtmgpnn_ctx(), ngpt, nlay, ncol, &
                    merge(1_c_int, 0_c_int, top_at_1), nmus, gauss_Ds(1:nmus, nmus), gauss_wts(1:nmus, nmus), d_inc, &
                    dev_present(optical_props%tau, ng, PRESENT_READ), &
                    dev_present(cloud_props%tau, size(cloud_props%tau, kind=c_long_long), PRESENT_READ), &
                    dev_present(sources%lay_source, ng, PRESENT_READ), nband, sources%pk_ntemp, &
                    dev_present(sources%pk_tlay, size(sources%pk_tlay, kind=c_long_long), PRESENT_READ), &
                    dev_present(sources%pk_tlev, size(sources%pk_tlev, kind=c_long_long), PRESENT_READ), &
                    dev_present(sources%pk_tsfc, size(sources%pk_tsfc, kind=c_long_long), PRESENT_READ), &
                    sources%pk_sfc_lay, lims, sources%pk_tmin, sources%pk_tdelta, sources%pk_totplnk, 1_c_int, d_emis, &
                    d_up, d_dn, d_upc, d_dnc), "rte_lw: lw_solver_noscat (clear + all sky)")
      if (error_msg == '') then
        call dev_copy_out(allsky_fluxes%flux_up, d_up, nv)
        call dev_copy_out(allsky_fluxes%flux_dn, d_dn, nv)
        call dev_copy_out(clrsky_fluxes%flux_up, d_upc, nv)
        call dev_copy_out(clrsky_fluxes%flux_dn, d_dnc, nv)
      end if
      call rrtmgpnn_sync(error_msg, "rte_lw")
      call dev_release(d_emis); call dev_release(d_inc)
      call dev_release(d_up); call dev_release(d_dn); call dev_release(d_upc); call dev_release(d_dnc)
    end subroutine solve_dual

    ! scattering clouds: the clear solve of tau without scattering and the all-sky solve by the rescaled solver, which
    ! increments (tau, 0, 0) by the cloud's (tau, ssa, g)(band) as it reads tau; with aerosols of the fused kind both
    ! from rrtmgpnn_lw_solver_1rescl_planck_clr_all under the aerosol request, tau + tau_aer(band) in both sets
    subroutine solve_scat()
      integer(c_long_long) :: ng, nv, nc
      integer(c_int), allocatable :: lims(:,:)
      type(c_ptr) :: d_emis, d_inc, d_up, d_dn, d_upc, d_dnc, d_tau, d_pf, d_tlay, d_tlev, d_tsfc
      lims = optical_props%get_band_lims_gpoint()
      ng = int(ngpt, c_long_long) * nlay * ncol
      nv = int(nlay + 1, c_long_long) * ncol
      nc = int(nband, c_long_long) * nlay * ncol
      d_emis = dev_stage(sfc_emis, int(nband, c_long_long) * ncol)
      d_inc = c_null_ptr
      if (present(inc_flux)) d_inc = dev_stage(inc_flux, int(ngpt, c_long_long) * ncol)
      d_up = dev_scratch(nv); d_dn = dev_scratch(nv); d_upc = dev_scratch(nv); d_dnc = dev_scratch(nv)
      d_tau = dev_present(optical_props%tau, ng, PRESENT_READ)
      d_pf = dev_present(sources%lay_source, ng, PRESENT_READ)
      d_tlay = dev_present(sources%pk_tlay, size(sources%pk_tlay, kind=c_long_long), PRESENT_READ)
      d_tlev = dev_present(sources%pk_tlev, size(sources%pk_tlev, kind=c_long_long), PRESENT_READ)
      d_tsfc = dev_present(sources%pk_tsfc, size(sources%pk_tsfc, kind=c_long_long), PRESENT_READ)
      if (aer_scat) then
        ! aerosols: armed for the solver call below, which clears it whatever it returns; both flux sets from the one
        ! entry, the clear sky gases + aerosols
        select type (aer_props)
        class is (ty_optical_props_1scl)
          error_msg = rrtmgpnn_check(c_rrtmgpnn_solver_request_aerosol(rrtmgpnn_ctx(), nband, nlay, ncol, &
                        dev_present(aer_props%tau, nc, PRESENT_READ), c_null_ptr, c_null_ptr), &
                        "rte_lw: solver_request_aerosol")
        end select
        select type (cloud_props)
        class is (ty_optical_props_2str)
          if (error_msg == '') &
          error_msg = rrtmgpnn_check(c_rrtmgpnn_lw_solver_1rescl_planck_clr_all(rrtmgpnn_ctx(), ngpt, nlay, ncol, &
                        merge(1_c_int, 0_c_int, top_at_1), nmus, gauss_Ds(1:nmus, nmus), gauss_wts(1:nmus, nmus), d_inc, &
                        d_tau, dev_present(cloud_props%tau, nc, PRESENT_READ), &
                        dev_present(cloud_props%ssa, nc, PRESENT_READ), dev_present(cloud_props%g, nc, PRESENT_READ), &
                        d_pf, nband, sources%pk_ntemp, d_tlay, d_tlev, d_tsfc, sources%pk_sfc_lay, lims, &
                        sources%pk_tmin, sources%pk_tdelta, sources%pk_totplnk, 1_c_int, d_emis, d_up, d_dn, d_upc, &
                        d_dnc), "rte_lw: lw_solver_1rescl (clear + all sky, scattering clouds, aerosols)")
        end select
      else
        ! no aerosols: the clear solve by the no-scattering fused-Planck entry, then the all-sky solve by the rescaled
        ! one (the same bits as the one entry gives)
        error_msg = rrtmgpnn_check(c_rrtmgpnn_lw_solver_noscat_planck(rrtmgpnn_ctx(), ngpt, nlay, ncol, &
                      merge(1_c_int, 0_c_int, top_at_1), nmus, gauss_Ds(1:nmus, nmus), gauss_wts(1:nmus, nmus), d_inc, &
                      d_tau, d_pf, nband, sources%pk_ntemp, d_tlay, d_tlev, d_tsfc, sources%pk_sfc_lay, lims, &
                      sources%pk_tmin, sources%pk_tdelta, sources%pk_totplnk, 1_c_int, d_emis, d_upc, d_dnc), &
                      "rte_lw: lw_solver_noscat (clear sky)")
        select type (cloud_props)
        class is (ty_optical_props_2str)
          if (error_msg == '') &
          error_msg = rrtmgpnn_check(c_rrtmgpnn_lw_solver_1rescl_planck_inc(rrtmgpnn_ctx(), ngpt, nlay, ncol, &
                        merge(1_c_int, 0_c_int, top_at_1), nmus, gauss_Ds(1:nmus, nmus), gauss_wts(1:nmus, nmus), d_inc, &
                        d_tau, dev_present(cloud_props%tau, nc, PRESENT_READ), &
                        dev_present(cloud_props%ssa, nc, PRESENT_READ), dev_present(cloud_props%g, nc, PRESENT_READ), &
                        d_pf, nband, sources%pk_ntemp, d_tlay, d_tlev, d_tsfc, sources%pk_sfc_lay, lims, &
                        sources%pk_tmin, sources%pk_tdelta, sources%pk_totplnk, 1_c_int, d_emis, d_up, d_dn), &
                        "rte_lw: lw_solver_1rescl (all sky, scattering clouds)")
        end select
      end if
      if (error_msg == '') then
        call dev_copy_out(allsky_fluxes%flux_up, d_up, nv)
        call dev_copy_out(allsky_fluxes%flux_dn, d_dn, nv)
        call dev_copy_out(clrsky_fluxes%flux_up, d_upc, nv)
        call dev_copy_out(clrsky_fluxes%flux_dn, d_dnc, nv)
      end if
      call rrtmgpnn_sync(error_msg, "rte_lw")
      call dev_release(d_emis); call dev_release(d_inc)
      call dev_release(d_up); call dev_release(d_dn); call dev_release(d_upc); call dev_release(d_dnc)
    end subroutine solve_scat
  end function rte_lw

  ! does this flux object want exactly the broadband up and down fluxes (what the dual entry writes)?
  logical function broadband_only(fluxes)
    class(ty_fluxes_flexible), intent(in) :: fluxes
    broadband_only = associated(fluxes%flux_up) .and. associated(fluxes%flux_dn) .and. &
                     .not. associated(fluxes%flux_net) .and. .not. fluxes%are_desired_gpt()
    select type (fluxes)
    class is (ty_fluxes_byband)
      if (fluxes%are_desired_bnd()) broadband_only = .false.
    end select
  end function broadband_only

  function rte_sw(k_dist, gas_concs, p_lay, t_lay, p_lev, mu0, sfc_alb_dir, sfc_alb_dif, cloud_props, allsky_fluxes, &
                  clrsky_fluxes, aer_props, col_dry, inc_flux, tsi_scaling, neural_nets) result(error_msg)
    class(ty_gas_optics_rrtmgp),  intent(in) :: k_dist
    type(ty_gas_concs),           intent(in) :: gas_concs
    real(wp), dimension(:,:),     intent(in) :: p_lay, t_lay   ! (nlay, ncol)
    real(wp), dimension(:,:),     intent(in) :: p_lev          ! (nlay+1, ncol)
    real(wp), dimension(:),       intent(in) :: mu0            ! (ncol)
    real(wp), dimension(:,:),     intent(in) :: sfc_alb_dir, sfc_alb_dif   ! (ngpt, ncol), as this layer's rte_sw
    class(ty_optical_props_arry), intent(in) :: cloud_props
    class(ty_fluxes_flexible), intent(inout) :: allsky_fluxes, clrsky_fluxes
    class(ty_optical_props_arry), optional, intent(in) :: aer_props
    real(wp), dimension(:,:), optional, intent(in) :: col_dry, &   ! (nlay, ncol)
                                                      inc_flux     ! (ngpt, ncol)
    real(wp), optional, intent(in) :: tsi_scaling
    type(rrtmgp_network_type), dimension(2), optional, intent(in) :: neural_nets
    character(len=128) :: error_msg
    class(ty_optical_props_arry), allocatable :: optical_props
    real(wp), dimension(:,:), allocatable :: toa_flux
    integer :: ncol, nlay, ngpt, nband
    logical :: top_at_1

    error_msg = ""
    ncol  = size(p_lay, 2)
    nlay  = size(p_lay, 1)
    ngpt  = k_dist%get_ngpt()
    nband = k_dist%get_nband()
    top_at_1 = p_lay(1, 1) < p_lay(nlay, 1)

    if (present(inc_flux) .and. present(tsi_scaling)) &
      error_msg = "rrtmpg_sw: only one of inc_flux, tsi_scaling may be supplied."
    if (present(aer_props)) then
      if (any([aer_props%get_ncol(), aer_props%get_nlay()] /= [ncol, nlay])) &
        error_msg = "rrtmpg_sw: aerosol properties inconsistently sized"
      if (.not. any(aer_props%get_ngpt() /= [ngpt, nband])) &   ! as written in the reference (:229-230)
        error_msg = "rrtmpg_sw: aerosol properties inconsistently sized"
    end if
    if (present(tsi_scaling)) then
      if (tsi_scaling <= 0._wp) error_msg = "rrtmpg_sw: tsi_scaling is < 0"
    end if
    if (present(inc_flux)) then
      if (any(shape(inc_flux) /= [ngpt, ncol])) error_msg = "rrtmpg_sw: incident flux inconsistently sized"
    end if
    if (len_trim(error_msg) > 0) return

    select type (cloud_props)
    class is (ty_optical_props_1scl)
      allocate(ty_optical_props_1scl :: optical_props)
    class is (ty_optical_props_2str)
      allocate(ty_optical_props_2str :: optical_props)
    class default
      error_msg = "sw_solver(...ty_optical_props_nstr...) not yet implemented"; return
    end select
    error_msg = optical_props%init(k_dist%get_band_lims_wavenumber(), k_dist%get_band_lims_gpoint())
    if (len_trim(error_msg) > 0) return
    select type (optical_props)
    class is (ty_optical_props_1scl)
      error_msg = optical_props%alloc_1scl(ncol, nlay)
    class is (ty_optical_props_2str)
      error_msg = optical_props%alloc_2str(ncol, nlay)
    end select
    if (error_msg /= '') return
    allocate(toa_flux(ngpt, ncol))

    ! gas optics once (:278-281); a supplied incident flux replaces its source, tsi_scaling scales it (:285-286)
    error_msg = k_dist%gas_optics(p_lay, p_lev, t_lay, gas_concs, optical_props, toa_flux, col_dry, neural_nets)
    if (error_msg /= '') return
    if (present(inc_flux))    toa_flux(:,:) = inc_flux(:,:)
    if (present(tsi_scaling)) toa_flux(:,:) = toa_flux(:,:) * tsi_scaling
    if (present(aer_props)) error_msg = aer_props%increment(optical_props)
    if (error_msg /= '') return

    ! the clear solve, clouds%increment, the all-sky solve (:293-308)
    error_msg = base_rte_sw(optical_props, top_at_1, mu0, toa_flux, sfc_alb_dir, sfc_alb_dif, clrsky_fluxes)
    if (error_msg /= '') return
    error_msg = cloud_props%increment(optical_props)
    if (error_msg /= '') return
    error_msg = base_rte_sw(optical_props, top_at_1, mu0, toa_flux, sfc_alb_dir, sfc_alb_dif, allsky_fluxes)
  end function rte_sw
end module mo_rrtmgp_clr_all_sky
