/*
 * rrtmgpnn.h -- C ABI of the MI355X-native RTE+RRTMGP-NN hot path.
 *
 * Plain pointers and sizes only (no torch / HIP types in the signatures): this is the
 * boundary the reference's Fortran class layer binds through ISO_C_BINDING
 * (see rte-rrtmgp-nn_amd/fortran/ and INTEGRATION.md).  All arrays use the reference's
 * Fortran column-major layout, g-point fastest:
 *     tau/lay_source/ssa/g      (ngpt, nlay,   ncol)
 *     lev_source                (ngpt, nlay+1, ncol)
 *     sfc_source/sfc_emis_gpt   (ngpt, ncol)
 *     play/tlay/col_dry/gases   (nlay, ncol)        plev/tlev (nlay+1, ncol)
 *     fluxes                    (nlay+1, ncol)
 * Array arguments are DEVICE pointers (hipMalloc'd or torch tensors) unless the comment
 * says "host".  Every call is asynchronous on the context's stream and reentrant across
 * contexts (one context per host thread / OpenMP block, as the reference drivers'
 * `!$OMP PARALLEL firstprivate(...)` loops require, rrtmgp_rfmip_lw.F90:364-367).
 *
 * Return value: RRTMGPNN_OK (0) or an error code; the message of the last failing call on
 * this host thread is rrtmgpnn_last_error().  The reference class layer returns
 * character(len=128) error_msg (empty on success); the Fortran glue maps one to the other.
 */
#ifndef RRTMGPNN_H
#define RRTMGPNN_H

#ifdef __cplusplus
extern "C" {
#endif

#define RRTMGPNN_OK               0
#define RRTMGPNN_ERR_ARGUMENT     1
#define RRTMGPNN_ERR_DEVICE       2
#define RRTMGPNN_ERR_IO           3
#define RRTMGPNN_ERR_UNSUPPORTED  4

#define RRTMGPNN_ACT_LINEAR       0
#define RRTMGPNN_ACT_SOFTSIGN     1
#define RRTMGPNN_ACT_RELU         2
#define RRTMGPNN_ACT_SIGMOID      3
#define RRTMGPNN_ACT_HARD_SIGMOID 4
#define RRTMGPNN_ACT_TANH         5
#define RRTMGPNN_ACT_GAUSSIAN     6

typedef struct rrtmgpnn_context rrtmgpnn_context;
typedef struct rrtmgpnn_network rrtmgpnn_network;
typedef struct rrtmgpnn_cloud_optics rrtmgpnn_cloud_optics;
typedef struct rrtmgpnn_file rrtmgpnn_file;

/* ---- runtime ------------------------------------------------------------------------------ */
int         rrtmgpnn_version(void);
const char *rrtmgpnn_last_error(void);
/* Creates a context on `device` that enqueues on `hip_stream` (a hipStream_t; NULL = the legacy default
 * stream, ordered with every other default-stream operation). */
int rrtmgpnn_context_create(int device, void *hip_stream, rrtmgpnn_context **ctx);
int rrtmgpnn_context_destroy(rrtmgpnn_context *ctx);
int rrtmgpnn_context_set_stream(rrtmgpnn_context *ctx, void *hip_stream);
/* MI355X tuning, no reference counterpart: which SW two-stream kernel rrtmgpnn_sw_solver_2stream* launch.
 * 0 (default): mode 3 when ngpt is even, one g-point per lane otherwise.  1: one g-point per lane.  2: two g-points
 * per lane (packed fp32, two columns per block) with per-level workspace planes.  3: two g-points per lane with
 * checkpointed passes (beam / adding state stored every 3 levels instead of per level).  2 and 3 need even ngpt.
 * All kernels give bit-identical fluxes.  ctx == NULL sets the default of every context not set itself. */
int rrtmgpnn_context_set_sw_kernel(rrtmgpnn_context *ctx, int mode);
/* MI355X tuning, no reference counterpart: how rrtmgpnn_lw_solver_noscat_planck_clr_all produces its two flux sets.
 * 0 (default): mode 1, measured 21 % faster than mode 2 at 10 000 x 60 columns.  1: the dual kernel, one launch that reads tau,
 * pfrac and tau_bnd once and carries a clear and an all-sky radiance per lane (one angle; several angles take mode 2).
 * 2: rrtmgpnn_lw_solver_noscat_planck followed by rrtmgpnn_lw_solver_noscat_planck_inc.
 * Bit-identical fluxes either way.  rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica follows the same setting with its
 * masked twins: 0 is mode 1 there too, measured 21 % faster than mode 2 at 10 000 x 60 columns.
 * ctx == NULL sets the default of every context not set itself. */
int rrtmgpnn_context_set_lw_clr_all(rrtmgpnn_context *ctx, int mode);
/* MI355X tuning, no reference counterpart: how rrtmgpnn_lw_solver_1rescl_planck_clr_all produces its two flux sets.
 * 1: the dual kernel, one launch of the fused rescaled solver in which a lane also carries the clear radiance (down in
 * the first pass, up in the second), reading tau, pfrac, the band rows and the mask word and building the Planck table
 * once (one angle; several angles take mode 2).  2: rrtmgpnn_lw_solver_noscat_planck[_inc] for the clear set, then the
 * single rescaled instance for the all-sky set.  0 (default): mode 1 -- at 10 000 x 60 columns, 256 g-points, under a
 * sampled mask it took 1.829 ms against mode 2's 1.976 ms (7.5 %; sample spreads 0.047 and 0.030 ms) and with the
 * aerosol 1.835 against 2.064 ms (11.1 %; spreads 0.024 and 0.025 ms); at 1800 x 60 3.8 % and 9.8 % (DESIGN.md
 * section 3, profiles/lw_scat_dual_ab.txt).  Where the dual kernel's LDS would not fit, mode 1 takes the two launches.
 * Bit-identical fluxes either way.  Any other value is RRTMGPNN_ERR_ARGUMENT.  ctx == NULL sets the default of every
 * context not set itself. */
int rrtmgpnn_context_set_lw_scat_clr_all(rrtmgpnn_context *ctx, int mode);
/* MI355X tuning, no reference counterpart: how rrtmgpnn_sw_solver_2stream_clr_all and
 * rrtmgpnn_sw_solver_2stream_rfmip_clr_all produce their two flux sets.
 * 0 (default): mode 2 -- at 10 000 x 60 columns the dual kernel's gain over the two launches (1.3-1.8 % in four runs)
 * did not exceed their sample spread in the run that decided it; mode 1 is 12 % faster there with a mask and aerosols
 * armed and 6.5 % faster at 1800 x 60.
 * 1: the dual kernel, one launch of the checkpointed solver in which a lane owns one g-point and carries
 * its all-sky and its clear-sky solve side by side (tau, ssa, g, the band rows and the mask word read once for both).
 * 2: two launches of the single-sky instances inside the entry, the
 * all-sky one with the armed requests, the clear one on the gases alone or with the requested aerosol as its band
 * increment; also what runs when the checkpointed kernel is not the context's SW kernel (rrtmgpnn_context_set_sw_kernel
 * mode 1 or 2).  Bit-identical fluxes wherever both modes take the call.  The two launches accept less: with an
 * aerosol request they need every band to start at an odd 1-based g-point (the single-sky aerosol instances' band-pair
 * layout; RRTMGPNN_ERR_UNSUPPORTED otherwise, where the dual kernel has no such restriction), and under SW kernel mode
 * 1 or 2 a cloud-mask or aerosol request is refused as rrtmgpnn_sw_solver_2stream_inc refuses it.  ctx == NULL sets the
 * default of every context not set itself. */
int rrtmgpnn_context_set_sw_clr_all(rrtmgpnn_context *ctx, int mode);
/* MI355X tuning, no reference counterpart: the MFMA tiling of the gas-optics networks (rrtmgpnn_predict_nn_lw/_sw,
 * rrtmgpnn_gas_optics_lw_nn/_sw_nn).  0 (default): v_mfma_f32_32x32x2_f32 tiles where an instance exists for the
 * networks, 16x16x4 otherwise.  1: 16x16x4 tiles.  The 32x32x2 instances, each for its own ngpt, with
 * softsign/softsign/linear and 16-byte aligned outputs, with and without the inputs formed in-kernel (the fused
 * entries): the LW g256 pair 18-58-58-256 + 18-16-16-256, the SW g224 pair 7-16-16-224 twice, the LW g128 single model
 * 18-64-64-256, and the reduced-resolution 2021 set, the LW g128 pair 18-72-72-128 + 18-24-24-128 and the SW g112 pair
 * 7-32-32-112 twice (its last tile of 32 g-points holds 16).  Without an in-kernel-input instance (every 16x16x4 route
 * of these three reduced-resolution sets) the fused entries run compute_nn_inputs, get_col_dry and the network kernel
 * on context workspace.
 * Bit-identical outputs either way.  ctx == NULL sets the default of every context not set itself.
 * The 16x16x4 kernel is compiled for 3-layer networks [nx, h1, h2, ny] of these shapes, written (K1S, H1T, H2T) =
 * (ceil(nx/4), ceil(h1/16), ceil(h2/16)): (2,1,1), (2,2,2), (5,1,1), (5,2,2), (5,3,3), (5,4,4), (5,5,5), (5,8,8) --
 * nx in 5..8 or 17..20, equal hidden tile counts -- each for any activations (softsign/softsign/linear inlined, any
 * other set by runtime code) and any ny, as long as the packed weights fit 160 KiB of LDS.  A single model
 * (rrtmgpnn_network_forward, rrtmgpnn_predict_nn_lw with nnets == 1, rrtmgpnn_predict_nn_sw with ssa == NULL) may
 * have any of them; the pairs compiled are LW (5,4,4)+(5,1,1), (5,5,5)+(5,2,2), (5,4,4)+(5,2,2) and SW (2,1,1)+(2,1,1),
 * (2,2,2)+(2,1,1), (2,2,2)+(2,2,2).  rrtmgpnn_predict_nn_lw/_sw return RRTMGPNN_ERR_UNSUPPORTED for anything else;
 * rrtmgpnn_network_forward runs anything else on the generic kernel. */
int rrtmgpnn_context_set_mlp_kernel(rrtmgpnn_context *ctx, int mode);
/* Which kernel served this context's last network launch (rrtmgpnn_network_forward, rrtmgpnn_predict_nn_lw/_sw,
 * rrtmgpnn_gas_optics_lw_nn/_sw_nn), for tests of the dispatch: path[0] one of RRTMGPNN_MLP_PATH_* (NONE before the
 * first launch); for MFMA16 path[1..3] = the first network's (K1S, H1T, H2T), path[4..6] the second's (0 without one);
 * path[7] flag bits: 1 softsign/softsign/linear inlined, 2 output tile count compiled in, 4 inputs formed in-kernel,
 * 8 16-byte output stores, 16 the active-column count read from a device word (rrtmgpnn_gas_optics_sw_nn_active). */
#define RRTMGPNN_MLP_PATH_NONE    0
#define RRTMGPNN_MLP_PATH_GENERIC 1
#define RRTMGPNN_MLP_PATH_MFMA32  2
#define RRTMGPNN_MLP_PATH_MFMA16  3
int rrtmgpnn_context_get_mlp_path(rrtmgpnn_context *ctx, int path[8]);
/* Which solver kernel instance served this context's last solver launch (the rrtmgpnn_lw_solver_* and
 * rrtmgpnn_sw_solver_* entries and the steps built on them), for tests of the dispatch.  path[0]: the kernel family, 0
 * before the first launch, 1 lw_noscat_kernel, 2 sw_2stream_ck_kernel, 3 lw_rescl_planck_inc_kernel, 4 lw_rescl_kernel,
 * 5 sw_2stream_kernel, 6 sw_2stream_x2_kernel (lw_2stream_kernel and sw_noscat_kernel, one flag each, record nothing).
 * path[1]: the instance's compile-time options, an OR of the family's bits:
 *   1 lw_noscat_kernel: 1 fused Planck sources, 2 band increment, 4 several angles or g-point outputs, 8 by-band
 *     outputs, 16 clear beside all sky (dual), 32 cloud mask, 64 the mask as the wave's scalar pair, 128 Jacobian,
 *     256 aerosol;
 *   2 sw_2stream_ck_kernel: 1 gas g, 2 band increment, 4 g-point outputs, 8 transmittance plane, 16 exp(-k tau) plane,
 *     32 band-pair increment, 64 by-band outputs, 128 cloud mask, 256 aerosol, 512 clear beside all sky (dual),
 *     1024 the small-grid instance;
 *   3 lw_rescl_planck_inc_kernel: 1 cloud mask, 2 aerosol, 4 clear beside all sky (dual);
 *   4 lw_rescl_kernel: 1 by-band outputs, 2 Jacobian;
 *   5 sw_2stream_kernel, 6 sw_2stream_x2_kernel: 1 gas g, 2 band increment, 4 g-point outputs, 8 by-band outputs;
 *   7 sw_2stream_ck_kernel with the active-column count read from a device word
 *     (rrtmgpnn_solver_request_active_columns): family 2's bits, and 2048 in every instance;
 *   8 sw_2stream_ck_kernel with that count beside a cloud mask and / or an aerosol (the requests armed together):
 *     family 2's bits, 2048 and 2 in every instance, with 128, 256 or both -- the masked cloud with and without the
 *     band-pair layout, the aerosol (band pair only) in front of the masked or the unmasked cloud, each with the
 *     transmittance plane and without;
 *   9 sw_2stream_ck_kernel with the by-band sums of the surface level (rrtmgpnn_solver_request_sfc_byband): the
 *     instance the same call runs without the request (family 2, or 8 beside an active-column count) and 4096 --
 *     2 and 32 in every instance, 128, 256 or both, with 2048 and without, with the transmittance plane and without.
 * path[2]: the launches the call made in these families, 2 where a clear + all-sky entry ran its two launches (path[0]
 * and path[1] are then the second's).  path[3]: the number of instances the family is compiled for; an options value
 * outside that list is refused with RRTMGPNN_ERR_UNSUPPORTED.  A call that launches nothing leaves the path as it was. */
int rrtmgpnn_context_get_solver_path(rrtmgpnn_context *ctx, int path[4]);
/* MI355X tuning, no reference counterpart: the gas-optics networks launched on this context use at most `cus` CUs'
 * worth of resident blocks (0, the default: every CU).  For a host that runs the LW and SW chains side by side on two
 * streams: an LW network confined to part of the chip leaves the other CUs to the SW solver from its start (each LW
 * network block holds a whole CU's LDS).  Bit-identical outputs. */
int rrtmgpnn_context_set_mlp_max_cus(rrtmgpnn_context *ctx, int cus);
/* The cap rrtmgpnn_context_set_mlp_max_cus left in force on this context (0: every CU). */
int rrtmgpnn_context_get_mlp_max_cus(rrtmgpnn_context *ctx, int *cus);
void *rrtmgpnn_context_stream(rrtmgpnn_context *ctx);
int rrtmgpnn_context_synchronize(rrtmgpnn_context *ctx);
/* The context's device workspace grows on demand.  A call issued while the context's stream is captured into a
 * hipGraph pins it (the graph holds its address): later calls that would need more fail with RRTMGPNN_ERR_ARGUMENT
 * instead of freeing memory the graph writes.  Unpin after destroying the graph (no reference counterpart). */
int rrtmgpnn_context_unpin_workspace(rrtmgpnn_context *ctx);
/* Device memory helpers for hosts without their own allocator (Fortran glue). */
int rrtmgpnn_malloc(rrtmgpnn_context *ctx, long long bytes, void **dptr);
int rrtmgpnn_free(rrtmgpnn_context *ctx, void *dptr);
int rrtmgpnn_memcpy_h2d(rrtmgpnn_context *ctx, void *dst, const void *src, long long bytes);
int rrtmgpnn_memcpy_d2h(rrtmgpnn_context *ctx, void *dst, const void *src, long long bytes);
/* A context whose work runs on a stream it creates and owns (non-blocking), so host threads with a context each
 * (OpenMP over blocks, rrtmgp_rfmip_lw.F90:364-367) run concurrently on the device.  No reference counterpart. */
int rrtmgpnn_context_create_owned(int device, rrtmgpnn_context **ctx);

/* ---- Device data environment of a context: the OpenACC data regions of the reference's GPU build ----
 * The reference keeps optical properties, sources and gas concentrations on the device between calls with
 * `!$acc enter data create/copyin` (ty_gas_concs%set_vmr, rrtmgp/mo_gas_concentrations.F90:166; the optical-property
 * and source constructors, examples/rfmip-clear-sky/rrtmgp_rfmip_lw.F90:325-327; gas_optics,
 * rrtmgp/mo_gas_optics_rrtmgp.F90:281-426) and `!$acc update host` / `exit data delete`.  Here a context maps a
 * host array (its address and size) to a device copy from the context's pool, with a state: host newer, both
 * current, device newer.  All transfers are ordered on the context's stream; a context serves one host thread.
 * rrtmgpnn_present: the device copy of host[0, bytes); mode RRTMGPNN_PRESENT_READ uploads it first when the host
 *   copy is newer (created on first use, `copyin`); RRTMGPNN_PRESENT_WRITE marks the device copy newer (the caller's
 *   kernel writes it; `create`); both bits: upload if needed, then device newer.  A different size for the same
 *   address replaces the entry (host newer).
 * rrtmgpnn_present_update_host: copy a device-newer array back (`!$acc update host`) and wait for it.
 * rrtmgpnn_present_update_device: the host copy changed: it is uploaded at its next READ (`!$acc update device`),
 *   in every context of the process (the reference's OpenACC data environment is process-wide).
 * rrtmgpnn_present_delete: drop the entry (its buffer returns to the pool; `!$acc exit data delete`); no-op if absent.
 *   Every other context's copy of that host array is stale from then on and is uploaded again at its next READ.
 * Cross-thread contract of update_device / delete: the host copy wins in every context.  A copy another context holds
 *   as device newer (a kernel result not yet copied back with update_host) is discarded too; a thread that still needs
 *   such a result must update_host it before any thread updates or deletes the same host array.  The process-wide
 *   generation table behind this keeps one 16-byte entry per host address ever updated or deleted (bounded by the
 *   distinct addresses the host program's allocator hands out).
 * rrtmgpnn_stage_h2d / rrtmgpnn_scratch / rrtmgpnn_release: stream-ordered per-call buffers from the same pool
 *   (a call's inputs copied in, its intermediates); released buffers are reused by later work on the stream.
 * rrtmgpnn_copy_d2h / rrtmgpnn_copy_h2d / rrtmgpnn_copy_d2d: enqueue a copy on the context's stream (the device side complete after
 *   rrtmgpnn_context_synchronize; the host buffer of an H2D copy may be reused on return).
 * rrtmgpnn_memset_async: bytes of a device buffer set to `value`, on the context's stream. */
#define RRTMGPNN_PRESENT_READ  1
#define RRTMGPNN_PRESENT_WRITE 2
int rrtmgpnn_present(rrtmgpnn_context *ctx, const void *host, long long bytes, int mode, void **dptr);
int rrtmgpnn_present_update_host(rrtmgpnn_context *ctx, void *host);
int rrtmgpnn_present_update_device(rrtmgpnn_context *ctx, const void *host);
int rrtmgpnn_present_delete(rrtmgpnn_context *ctx, const void *host);
int rrtmgpnn_stage_h2d(rrtmgpnn_context *ctx, const void *host, long long bytes, void **dptr);
int rrtmgpnn_scratch(rrtmgpnn_context *ctx, long long bytes, void **dptr);
int rrtmgpnn_release(rrtmgpnn_context *ctx, void *dptr);
int rrtmgpnn_copy_d2h(rrtmgpnn_context *ctx, void *host, const void *dptr, long long bytes);
int rrtmgpnn_copy_h2d(rrtmgpnn_context *ctx, void *dptr, const void *host, long long bytes);
int rrtmgpnn_copy_d2d(rrtmgpnn_context *ctx, void *dst, const void *src, long long bytes);
int rrtmgpnn_memset_async(rrtmgpnn_context *ctx, void *dptr, int value, long long bytes);

/* ---- neural networks: replaces rrtmgp_network_type (neural/mod_network_rrtmgp.F90:34-122) ---- */
/* Load an RBIN model file (converted from the reference's netCDF model files). */
int rrtmgpnn_network_load(rrtmgpnn_context *ctx, const char *path, rrtmgpnn_network **net);
/* Build from host arrays.  weights[n] is layer n's kernel, (dims[n], dims[n+1]) C-order
 * (= the netCDF variable nn_weights_<n+1> = the reference's w_transposed memory).
 * output_mean/std may be NULL (Planck-fraction models). */
int rrtmgpnn_network_create(rrtmgpnn_context *ctx, int nlayers, const int *dims, const int *activations,
                            const float *const *weights, const float *const *biases,
                            const float *input_min, const float *input_max,
                            const float *output_mean, const float *output_std,
                            const char *input_names /* nx*32 chars, space padded, may be NULL */,
                            rrtmgpnn_network **net);
int rrtmgpnn_network_destroy(rrtmgpnn_network *net);
/* host outputs */
int rrtmgpnn_network_get_dims(const rrtmgpnn_network *net, int *nlayers, int dims[8]);
int rrtmgpnn_network_get_input_name(const rrtmgpnn_network *net, int i, char *buf, int buflen);
int rrtmgpnn_network_get_input_scaling(const rrtmgpnn_network *net, float *input_min, float *input_max);

/* ---- gas-optics kernels --------------------------------------------------------------------- */
/* compute_nn_inputs (rrtmgp/mo_gas_optics_rrtmgp.F90:618-798).  gas_conc[k] (k>=2) is a device
 * pointer to the concentration of input k with gas_ndims[k] in {0:(1), 1:(nlay), 2:(nlay,ncol)},
 * or NULL when the gas is absent (reference uses ref_vmr = 0, :757-758).  Entries 0,1 ignored.
 * gas_conc/gas_ndims are HOST arrays of length ninputs (<= 32).  nn_inputs (ninputs,nlay,ncol). */
int rrtmgpnn_compute_nn_inputs(rrtmgpnn_context *ctx, int ncol, int nlay, int ninputs,
                               const float *play, const float *tlay,
                               const float *const *gas_conc, const int *gas_ndims,
                               const rrtmgpnn_network *net, float *nn_inputs);
/* get_col_dry (rrtmgp/mo_gas_optics_rrtmgp.F90:1662-1707), g0 = grav. */
int rrtmgpnn_get_col_dry(rrtmgpnn_context *ctx, int ncol, int nlay, const float *vmr_h2o, const float *plev,
                         float *col_dry);
/* Level temperatures from layers (rrtmgp/mo_gas_optics_rrtmgp.F90:317-337). */
int rrtmgpnn_interpolate_tlev(rrtmgpnn_context *ctx, int ncol, int nlay, const float *play, const float *plev,
                              const float *tlay, float *tlev);
/* predict_nn_lw_blas (rrtmgp/kernels/mo_gas_optics_kernels.F90:690-774).  nnets == 2: nets[0] =
 * absorption (tau = (std*y+mean)^8 * col_dry), nets[1] = Planck fraction (pfrac = y^2);
 * nnets == 1: single "both" model with 2*ngpt outputs (:744-772).
 * The networks' last layer is taken as linear, whatever its activation code (output_sgemm_tau / _lw add the bias and
 * scale: "linear layer, no activation"); the same holds for rrtmgpnn_predict_nn_sw and the fused entries.  Compiled
 * shapes and pairs: rrtmgpnn_context_set_mlp_kernel (RRTMGPNN_ERR_UNSUPPORTED otherwise); operand domain of softsign:
 * rrtmgpnn_network_forward. */
int rrtmgpnn_predict_nn_lw(rrtmgpnn_context *ctx, int ncol, int nlay, int ngpt, int ninputs,
                           const float *nn_inputs, const float *col_dry,
                           const rrtmgpnn_network *const *nets, int nnets, float *tau, float *pfrac);
/* predict_nn_sw_blas (:869-953) with INLINE_COMBINE: nets[0] absorption, nets[1] Rayleigh.
 * ssa == NULL -> tau = tau_abs only (1scl).  Otherwise tau = tau_abs + tau_ray, ssa = tau_ray/tau.
 * g != NULL -> zero-filled as gas_optics_ext does (mo_gas_optics_rrtmgp.F90:560-567). */
int rrtmgpnn_predict_nn_sw(rrtmgpnn_context *ctx, int ncol, int nlay, int ngpt, int ninputs,
                           const float *nn_inputs, const float *col_dry,
                           const rrtmgpnn_network *const *nets, float *tau, float *ssa, float *g);
/* Fused gas optics, NN path (MI355X): compute_nn_inputs + get_col_dry + predict_nn_lw in one kernel.  The network
 * inputs and the dry-air column amounts are formed per sample inside the MLP kernel with the expressions of
 * rrtmgpnn_compute_nn_inputs and rrtmgpnn_get_col_dry, so nn_inputs and col_dry never touch HBM; tau and pfrac are
 * bit-identical to the three separate calls (gas_optics_int's NN branch, rrtmgp/mo_gas_optics_rrtmgp.F90:342-391).
 * Arguments as those calls' (gas_conc / gas_ndims HOST arrays; vmr_h2o the h2o vmr get_col_dry reads).  Networks
 * without an in-kernel instance run the three kernels (nn_inputs and col_dry in the context workspace). */
int rrtmgpnn_gas_optics_lw_nn(rrtmgpnn_context *ctx, int ncol, int nlay, int ngpt, int ninputs, const float *play,
                              const float *tlay, const float *plev, const float *vmr_h2o,
                              const float *const *gas_conc, const int *gas_ndims,
                              const rrtmgpnn_network *const *nets, int nnets, float *tau, float *pfrac);
/* The same for the shortwave: compute_nn_inputs + get_col_dry + predict_nn_sw (gas_optics_ext's NN branch,
 * mo_gas_optics_rrtmgp.F90:433-602); ssa / g as rrtmgpnn_predict_nn_sw. */
int rrtmgpnn_gas_optics_sw_nn(rrtmgpnn_context *ctx, int ncol, int nlay, int ngpt, int ninputs, const float *play,
                              const float *tlay, const float *plev, const float *vmr_h2o,
                              const float *const *gas_conc, const int *gas_ndims,
                              const rrtmgpnn_network *const *nets, float *tau, float *ssa, float *g);
/* compute_bc (extensions/mo_compute_bc.F90): the upper boundary condition from one thin isothermal layer between the gas
 * optics' minimum pressure press_min and the model's top.  flux_bc (ngpt, ncol) DEVICE is the spectrally resolved
 * downward flux at that layer's bottom: the inc_flux of the solver entries.  At most three launches: the one-layer
 * problem gathered as :108-140 build it (top_lay = top_at_1 ? 1 : nlay; tlay1 = tlev1(1:2) = tsfc1 = tlay(top_lay);
 * plev1 = (press_min, plev(top_lay + 1)) -- literally, so with top_at_1 the layer overlaps the model's top layer,
 * SURVEY.md quirk B-15; play1 = 0.5f * (plev1(1) + plev1(2)); each gas at top_lay), the in-kernel-input gas optics of
 * rrtmgpnn_gas_optics_lw_nn / _sw_nn at nlay = 1, and the layer's solve at its bottom level.  The one-layer arrays, tau
 * and pfrac / ssa live in the context workspace; no source array and no (ngpt, 2, ncol) flux array exists.  Networks
 * without an in-kernel instance take the gas-optics entries' three-kernel fallback.
 * Arguments as rrtmgpnn_gas_optics_*_nn (gas_conc / gas_ndims HOST arrays, the rest DEVICE; play is not read: the
 * orientation is top_at_1) and rrtmgpnn_lw_solver_noscat_planck (band_lims_gpt, Ds, weights HOST; totplnk DEVICE).
 * nlay >= 1, nmus 1..4, SW ngpt even; RRTMGPNN_ERR_ARGUMENT with a message otherwise; ncol == 0 is OK.  Requests armed
 * on the context (rrtmgpnn_solver_request_*) are left for the next solver call.
 * PRESSURES are device arrays, so the reference's check "pressures are too close to (or less than) min in gas optics"
 * (plev(:, top_lay) <= press_min + 2 spacing(press_min), :110-114) is the class layers' part (rrtmgpnn/compute_bc.py,
 * fortran/mo_compute_bc.F90, ClearSkyStep), not this entry's.
 * LW: Planck sources as rrtmgpnn_compute_planck_source_nn's at nlay = 1 with tlev = tsfc = tlay; per angle
 * lw_source_noscat's source_dn and the transport from a zero incident radiance.  UNITS: with nmus == 1 and
 * as_flux == 0 flux_bc is the reference's own array, a RADIANCE (rte_lw's one-angle g-point output, quirk B-5; the
 * reference always calls rte_lw with one angle); as_flux != 0 multiplies by the solver's 2.0f * pi * weights[0], which
 * is what inc_flux means.  With nmus > 1 flux_bc is the angle-summed flux either way.  tau * D <= 2^126 as for every
 * rrtmgpnn_lw_solver_noscat* entry.
 * SW: tau = tau_abs + tau_ray as rrtmgpnn_predict_nn_sw forms it; flux_bc is sw_solver_2stream's direct beam at the
 * layer's bottom, (solar_source(g) * mu0) * exp(-tau / mu0) with that kernel's operations; solar_source (ngpt) and
 * mu0 (ncol) DEVICE. */
int rrtmgpnn_compute_bc_lw(rrtmgpnn_context *ctx, int ncol, int nlay, int ngpt, int ninputs, int top_at_1,
                           float press_min, const float *play, const float *plev, const float *tlay,
                           const float *vmr_h2o, const float *const *gas_conc, const int *gas_ndims,
                           const rrtmgpnn_network *const *nets, int nnets, int nbnd, int nPlanckTemp,
                           const int *band_lims_gpt, float temp_ref_min, float totplnk_delta, const float *totplnk,
                           int nmus, const float *Ds, const float *weights, int as_flux, float *flux_bc);
int rrtmgpnn_compute_bc_sw(rrtmgpnn_context *ctx, int ncol, int nlay, int ngpt, int ninputs, int top_at_1,
                           float press_min, const float *play, const float *plev, const float *tlay,
                           const float *vmr_h2o, const float *const *gas_conc, const int *gas_ndims,
                           const rrtmgpnn_network *const *nets, const float *solar_source, const float *mu0,
                           float *flux_bc);
/* Generic MLP forward (network_type%output_sgemm_flat, neural/mod_network.F90:273-354):
 * out(ny, nbatch) = net(x(nx, nbatch)), last-layer activation applied, no post-processing.  Any network
 * rrtmgpnn_network_create accepts with hidden widths <= 256 (RRTMGPNN_ERR_UNSUPPORTED beyond): the 16x16x4 MFMA
 * kernel where an instance is compiled for its shape (rrtmgpnn_context_set_mlp_kernel lists them), the one-thread-
 * per-sample generic kernel otherwise; the same bits either way (every dot product an fmaf chain in ascending k).
 * OPERAND DOMAIN of softsign in the MFMA kernels (this entry, rrtmgpnn_predict_nn_lw/_sw, rrtmgpnn_gas_optics_*_nn):
 * in a softsign, softsign, linear network (the inlined activation set) a hidden pre-activation must not exceed 2^126
 * (8.5e37) in magnitude: libm_ref.hpp div_softsign takes the hardware reciprocal of |x| + 1, which is 0 beyond, so the
 * unit gives +-0 where x / (|x| + 1) is +-1.  Up to 2^126, subnormals and +-0 included, and for +-inf and nan (nan
 * either way) the outputs are the reference's bit for bit (tests/test_gpu_mlp_shapes.py::test_mlp_operand_edges).
 * Networks with any other activation set divide plainly and have no such bound.  The reference's networks see inputs
 * scaled to about [0, 1] and pre-activations of order 1 to 10. */
int rrtmgpnn_network_forward(rrtmgpnn_context *ctx, const rrtmgpnn_network *net, long long nbatch,
                             const float *x, float *out);
/* compute_Planck_source_nn (rrtmgp/kernels/mo_gas_optics_kernels.F90:615-683).  sfc_lay 1-based.
 * band_lims_gpt: HOST (2,nbnd) 1-based.  totplnk: DEVICE (nPlanckTemp, nbnd).
 * pfrac is overwritten with lay_source.
 * BAND LIMITS must give every g-point exactly one band: limits that overlap or leave a g-point out are
 * RRTMGPNN_ERR_ARGUMENT, here and in every fused-Planck solver entry (rrtmgpnn_lw_solver_noscat_planck[_gpt / _inc /
 * _clr_all / _clr_all_mcica], rrtmgpnn_lw_solver_1rescl_planck_*) and in rrtmgpnn_compute_bc_lw, whether or not the
 * call has a band increment or a by-band emissivity: the reference leaves lev_source undefined and pfrac untouched at
 * a g-point outside every band and multiplies pfrac once per band at one in several, where the kernels' band lookup
 * would give band 0 and the first band (as rrtmgpnn_increment_bybnd states for the increments).
 * TEMPERATURES outside the table follow interpolate1D (:1024-1043) literally, bit for bit (tests/planck_edges.py):
 * with val0 = (T - temp_ref_min) / totplnk_delta the index is clamped to the table but the fraction is val0 - int(val0)
 * with int() truncating toward zero, so T = temp_ref_max returns the LAST BUT ONE table value, T above it extrapolates
 * the last interval by the fractional part alone, T <= temp_ref_min - totplnk_delta on a knot returns the first value
 * and between knots extrapolates the first interval with a negative fraction, and sfc_source_Jac is 0 wherever tsfc
 * and tsfc + 1 share an index and a fraction (tsfc = temp_ref_max - 1 with totplnk_delta 1). */
int rrtmgpnn_compute_planck_source_nn(rrtmgpnn_context *ctx, int ncol, int nlay, int nbnd, int ngpt,
                                      int nPlanckTemp, const float *tlay, const float *tlev, const float *tsfc,
                                      int sfc_lay, const int *band_lims_gpt, float temp_ref_min,
                                      float totplnk_delta, const float *totplnk, float *sfc_source,
                                      float *sfc_source_Jac, float *pfrac, float *lev_source);

/* ---- RTE solvers ---------------------------------------------------------------------------- */
/* lw_solver_noscat_GaussQuad (rte/kernels/mo_rte_solver_kernels.F90:332-415) without rescaling or
 * Jacobians.  Ds, weights: HOST arrays of nmus (<= 4) entries.  inc_flux may be NULL (zero). */
/* OPERAND BOUND of every rrtmgpnn_lw_solver_noscat* entry (plain, _planck, _planck_inc, _planck_clr_all,
 * _planck_clr_all_mcica, _gpt, _planck_gpt): the fluxes
 * are the reference's bit for bit for tau * D <= 2^126 (8.5e37) in every layer, g-point and secant D (Gauss or lw_Ds;
 * with _planck_inc and _planck_clr_all, tau is the incremented optical depth).  Beyond it the layer source's (1 - T) / (tau * D) is
 * taken as 0 where the reference has ~3e-39, and a tau * D that overflows to inf makes the column's fluxes nan where
 * the reference's are finite.  The shortened division that causes this saves 1.2 - 2.3 % of the solver's time
 * (DESIGN.md section 3); tests/test_gpu_solver_edges.py holds both sides of the bound for each of these entries (the
 * fused ones with the band increment, both modes of rrtmgpnn_context_set_lw_clr_all, the McICA mask and lw_Ds), and for
 * the clear-sky set of rrtmgpnn_lw_solver_1rescl_planck_clr_all, which carries the same bound.  Where the Planck level
 * sources beside the layer are not zero (every fused-Planck entry) a finite tau * D beyond 2^126 was still bitwise: the
 * flushed quotient is absorbed; a product that overflows to inf is nan there too.  The SW solvers have no such
 * bound: tau, ssa, g and mu0 over their whole float range (tau up to 2e38, ssa down to 1e-45, mu0 down to FLT_MIN) were
 * bitwise. */
int rrtmgpnn_lw_solver_noscat(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1, int nmus,
                              const float *Ds, const float *weights, const float *inc_flux,
                              const float *tau, const float *lay_source, const float *lev_source,
                              const float *sfc_emis_gpt, const float *sfc_source,
                              float *flux_up, float *flux_dn);
/* Fused clear-sky LW entry: compute_Planck_source_nn (rrtmgp/kernels/mo_gas_optics_kernels.F90:615-683)
 * + lw_solver_noscat_GaussQuad in one kernel.  Takes the Planck fraction (what predict_nn_lw writes into
 * lay_source) instead of lay/lev/sfc sources, forms every source in-kernel with the same products as
 * rrtmgpnn_compute_planck_source_nn, and never stores them: fluxes are bit-identical to
 * compute_planck_source_nn followed by lw_solver_noscat.  band_lims_gpt HOST (2,nbnd), every g-point in exactly one
 * band (rrtmgpnn_compute_planck_source_nn's rule); totplnk DEVICE.
 * emis_by_band == 0: sfc_emis is (ngpt, ncol) per g-point; 1: (nbnd, ncol) by band, as rte_lw takes it, expanded
 * in-kernel (expand, rte/mo_rte_lw.F90:429-447: the same values, no band-to-g-point array in HBM). */
int rrtmgpnn_lw_solver_noscat_planck(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1, int nmus,
                                     const float *Ds, const float *weights, const float *inc_flux, const float *tau,
                                     const float *pfrac, int nbnd, int nPlanckTemp, const float *tlay,
                                     const float *tlev, const float *tsfc, int sfc_lay, const int *band_lims_gpt,
                                     float temp_ref_min, float totplnk_delta, const float *totplnk,
                                     int emis_by_band, const float *sfc_emis, float *flux_up, float *flux_dn);
/* rrtmgpnn_lw_solver_noscat_planck with the atmosphere incremented by a band-resolved absorption optical depth
 * tau_bnd (nbnd, nlay, ncol), e.g. cloud optics: the same fluxes as rrtmgpnn_increment_bybnd (1scl by 1scl)
 * followed by rrtmgpnn_lw_solver_noscat_planck, but the g-point tau array is only read (it is left as it was). */
int rrtmgpnn_lw_solver_noscat_planck_inc(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                         int nmus, const float *Ds, const float *weights, const float *inc_flux,
                                         const float *tau, const float *tau_bnd, const float *pfrac, int nbnd,
                                         int nPlanckTemp, const float *tlay, const float *tlev, const float *tsfc,
                                         int sfc_lay, const int *band_lims_gpt, float temp_ref_min,
                                         float totplnk_delta, const float *totplnk, int emis_by_band,
                                         const float *sfc_emis, float *flux_up, float *flux_dn);
/* rte_lw of extensions/mo_rrtmgp_clr_all_sky.F90:146-172 on the fused-Planck path: the clear-sky fluxes of tau into
 * flux_up_clr / flux_dn_clr and the all-sky fluxes of tau + tau_bnd(band) into flux_up / flux_dn ((nlay+1, ncol) each),
 * i.e. what rrtmgpnn_lw_solver_noscat_planck and rrtmgpnn_lw_solver_noscat_planck_inc give on the same arguments, bit
 * for bit; tau and pfrac are only read.  With one angle (nmus == 1) a dual kernel reads the inputs once and solves
 * both in one launch; nmus 2..4 issue the two existing kernels back to back on the context's stream
 * (rrtmgpnn_context_set_lw_clr_all selects).  A by-band request armed on the context
 * (rrtmgpnn_solver_request_byband) is refused with RRTMGPNN_ERR_ARGUMENT, and cleared as every solver entry clears it. */
int rrtmgpnn_lw_solver_noscat_planck_clr_all(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                             int nmus, const float *Ds, const float *weights, const float *inc_flux,
                                             const float *tau, const float *tau_bnd, const float *pfrac, int nbnd,
                                             int nPlanckTemp, const float *tlay, const float *tlev,
                                             const float *tsfc, int sfc_lay, const int *band_lims_gpt,
                                             float temp_ref_min, float totplnk_delta, const float *totplnk,
                                             int emis_by_band, const float *sfc_emis, float *flux_up, float *flux_dn,
                                             float *flux_up_clr, float *flux_dn_clr);
/* rrtmgpnn_lw_solver_noscat_planck_clr_all with the all-sky increment switched per g-point by a McICA mask: mask_bits
 * (ceil(ngpt/32), nlay, ncol) DEVICE, bit g % 32 of word g / 32, the layout the mask kernels write
 * (rrtmgpnn_sampled_mask_*).  flux_up_clr / flux_dn_clr are what rrtmgpnn_lw_solver_noscat_planck gives on the same
 * arguments and flux_up / flux_dn what rrtmgpnn_lw_solver_noscat_planck_inc gives with that mask armed
 * (rrtmgpnn_solver_request_cloud_mask), bit for bit.  nmus == 1: one launch of the masked dual kernel, which reads tau,
 * pfrac, tau_bnd and the mask once (ngpt % 64 == 0 and mask_bits 8-byte aligned: each wave's two mask words from one
 * scalar load per layer; otherwise one word per lane).  nmus 2..4, or mode 2 of rrtmgpnn_context_set_lw_clr_all: those
 * two launches back to back on the context's stream, the mask armed internally.  Mode 0 is mode 1 for this entry:
 * at 10 000 x 60 columns the masked dual kernel measured 0.204 ms (21 %) below the two launches, four times their sample
 * spread.  The mask is an argument, not a request: mask_bits == NULL,
 * a cloud-mask request armed on the context and an armed by-band request are each refused with RRTMGPNN_ERR_ARGUMENT
 * (the requests are cleared, as every solver entry clears them).  The pointer is a kernel argument and nothing is
 * allocated with one angle, so the call can be captured in a hipGraph.  No reference counterpart. */
int rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                                   int nmus, const float *Ds, const float *weights,
                                                   const float *inc_flux, const float *tau, const float *tau_bnd,
                                                   const float *pfrac, int nbnd, int nPlanckTemp, const float *tlay,
                                                   const float *tlev, const float *tsfc, int sfc_lay,
                                                   const int *band_lims_gpt, float temp_ref_min, float totplnk_delta,
                                                   const float *totplnk, int emis_by_band, const float *sfc_emis,
                                                   float *flux_up, float *flux_dn, float *flux_up_clr,
                                                   float *flux_dn_clr, const unsigned int *mask_bits);
/* rte_lw on two-stream optical properties, default branch (rte/mo_rte_lw.F90:372-387): lw_solver_noscat_GaussQuad
 * with do_rescaling -- tau scaled by (1 - ssa + ssa(1-g)/2), a no-scattering pass down, then
 * lw_transport_1rescl up and down again with the adjustment terms (rte/kernels/mo_rte_solver_kernels.F90:209-233,
 * 1729-1795).  Arguments as rrtmgpnn_lw_solver_noscat plus ssa, g (ngpt, nlay, ncol).
 * OPERAND DOMAIN: ssa (1 + g) / 2 < 1 (the scaling 1 - ssa + ssa (1 - g) / 2 must not vanish, as in the reference); no
 * bound on tau: the rescaled layer divides plainly, and tau up to 3e38 (tau * D * scaling overflowing to inf included),
 * ssa from 1e-45 to 1 and g from -0.4 to 1 were the reference's bit for bit, as were rrtmgpnn_lw_solver_1rescl_gpt, the
 * flux Jacobian, rrtmgpnn_lw_solver_1rescl_planck_inc and rrtmgpnn_lw_solver_2stream[_gpt] on the same operands
 * (tests/test_gpu_solver_edges.py). */
int rrtmgpnn_lw_solver_1rescl(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1, int nmus,
                              const float *Ds, const float *weights, const float *inc_flux, const float *tau,
                              const float *ssa, const float *g, const float *lay_source, const float *lev_source,
                              const float *sfc_emis_gpt, const float *sfc_source, float *flux_up, float *flux_dn);
/* rrtmgpnn_lw_solver_1rescl on the fused-Planck path with the atmosphere incremented by band-resolved two-stream
 * properties (tau_bnd, ssa_bnd, g_bnd; (nbnd, nlay, ncol) DEVICE, all three required: NULL is RRTMGPNN_ERR_ARGUMENT),
 * e.g. LW cloud optics with scattering: the arguments of rrtmgpnn_lw_solver_noscat_planck_inc with ssa_bnd and g_bnd
 * after tau_bnd.  Per column, layer and g-point of band b, in float32: the optical properties are
 * inc_2stream_by_2stream_bybnd (rte/kernels/mo_optical_props_kernels.F90:430-463) of (tau, 0, 0) by
 * (tau_bnd(b), ssa_bnd(b), g_bnd(b)) -- the gas atmosphere is 1scl, its ssa and g the literal zeros a 2str copy of it
 * would hold, so no such arrays exist; the sources are formed in-kernel from pfrac as in rrtmgpnn_lw_solver_noscat_planck;
 * the transport is rrtmgpnn_lw_solver_1rescl's.  The fluxes are bit for bit those of rrtmgpnn_compute_planck_source_nn,
 * zero-filled ssa / g, rrtmgpnn_increment_bybnd and rrtmgpnn_lw_solver_1rescl on the same inputs; tau and pfrac are only
 * read.  Under rrtmgpnn_solver_request_cloud_mask the three band operands are 0 where the g-point's bit is clear: bit
 * for bit rrtmgpnn_draw_samples (2str) + rrtmgpnn_increment + rrtmgpnn_lw_solver_1rescl (an all-zero mask therefore
 * gives rrtmgpnn_lw_solver_noscat_planck's fluxes: the rescaled solver with ssa = 0 is the no-scattering one).
 * nmus 1..4, both orientations, ngpt <= 256, emis_by_band 0 or 1, inc_flux may be NULL.  Broadband fluxes only: an armed
 * by-band request (separate or paired with a mask), a flux-Jacobian request and an aerosol request are each refused
 * with RRTMGPNN_ERR_ARGUMENT and a message naming this entry, and cleared as every solver entry clears them.  The
 * workspace is one (ngpt, nlay+1, ncol) plane (three with several angles): half of rrtmgpnn_lw_solver_1rescl's, since
 * the first-pass radiance at a level is read for the last time just before the upward radiance of that level is
 * stored.  Nothing is allocated beyond the context workspace, so a warmed-up call can be captured in a hipGraph.
 * OPERAND BOUND: ssa_bnd * (1 + g_bnd) / 2 < 1, so that the scaling 1 - ssa + ssa (1 - g) / 2 does not vanish (as in the
 * reference).  No reference counterpart as one call. */
int rrtmgpnn_lw_solver_1rescl_planck_inc(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                         int nmus, const float *Ds, const float *weights, const float *inc_flux,
                                         const float *tau, const float *tau_bnd, const float *ssa_bnd,
                                         const float *g_bnd, const float *pfrac, int nbnd, int nPlanckTemp,
                                         const float *tlay, const float *tlev, const float *tsfc, int sfc_lay,
                                         const int *band_lims_gpt, float temp_ref_min, float totplnk_delta,
                                         const float *totplnk, int emis_by_band, const float *sfc_emis,
                                         float *flux_up, float *flux_dn);
/* Clear-sky beside all-sky LW fluxes for scattering clouds, with aerosols: rte_lw of
 * extensions/mo_rrtmgp_clr_all_sky.F90:146-172 (clear sky = gases + aerosols, all sky = that + clouds) where the clouds
 * are two-stream and rte_lw therefore takes the rescaled solver (rte/mo_rte_lw.F90:372-387).  The arguments of
 * rrtmgpnn_lw_solver_1rescl_planck_inc in its order, then flux_up_clr, flux_dn_clr ((nlay+1, ncol) DEVICE, required).
 * Requests it honours: rrtmgpnn_solver_request_cloud_mask, which switches the cloud in the all-sky set only, and a 1scl
 * rrtmgpnn_solver_request_aerosol (ssa_aer and g_aer NULL) on the call's bands and extents, which goes into both sets:
 * inc_2stream_by_1scalar_bybnd (rte/kernels/mo_optical_props_kernels.F90:426-484 holds it and the two-stream increment
 * that follows), i.e. tau + tau_aer(b) with ssa = g = +0, before the cloud: (tau + tau_aer) + tau_bnd, two separately
 * rounded adds.
 * flux_up_clr / flux_dn_clr: bit for bit rrtmgpnn_lw_solver_noscat_planck on the same arguments, with an aerosol
 * rrtmgpnn_lw_solver_noscat_planck_inc with tau_aer as its band increment (the rescaled solve of a 1scl atmosphere is the
 * no-scattering one).  flux_up / flux_dn: bit for bit rrtmgpnn_lw_solver_1rescl_planck_inc under the same mask request,
 * with an aerosol rrtmgpnn_increment_bybnd twice (aerosol, then cloud) and rrtmgpnn_lw_solver_1rescl.
 * Refused with RRTMGPNN_ERR_ARGUMENT and a message naming this entry, every request cleared: a by-band request
 * (separate or paired), a flux-Jacobian request, a 2str aerosol, mask or aerosol extents that are not the call's, NULL
 * band or clear-sky arrays; ngpt > 256 is RRTMGPNN_ERR_UNSUPPORTED.  ncol == 0 is OK.  How the two sets are produced:
 * rrtmgpnn_context_set_lw_scat_clr_all.  Operand bounds and workspace as rrtmgpnn_lw_solver_1rescl_planck_inc (the two
 * launches of mode 2 share the context workspace in stream order).  OPERAND BOUND of the clear-sky set, in either mode:
 * that of the rrtmgpnn_lw_solver_noscat* entries, (tau [+ tau_aer]) * D <= 2^126 -- the clear radiance is the
 * no-scattering step with its shortened division, so a product that overflows to inf gives nan in flux_up_clr /
 * flux_dn_clr where the reference is finite, while the all-sky set of the same call, which divides plainly, stays the
 * reference's (tests/test_gpu_solver_edges.py holds both).  No reference counterpart as one call. */
int rrtmgpnn_lw_solver_1rescl_planck_clr_all(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                             int nmus, const float *Ds, const float *weights, const float *inc_flux,
                                             const float *tau, const float *tau_bnd, const float *ssa_bnd,
                                             const float *g_bnd, const float *pfrac, int nbnd, int nPlanckTemp,
                                             const float *tlay, const float *tlev, const float *tsfc, int sfc_lay,
                                             const int *band_lims_gpt, float temp_ref_min, float totplnk_delta,
                                             const float *totplnk, int emis_by_band, const float *sfc_emis,
                                             float *flux_up, float *flux_dn, float *flux_up_clr, float *flux_dn_clr);
/* rte_lw(..., use_2stream=.true.): lw_solver_2stream (rte/kernels/mo_rte_solver_kernels.F90:426-486) with
 * lw_two_stream (:1018-1069), lw_source_2str (:1112-1162) and adding (:1526-1637).  inc_flux (ngpt, ncol) is a flux
 * (NULL: zero); the layer sources are not used (as in the reference).  Broadband sums are sequential over g
 * (sum_broadband_nocol). */
int rrtmgpnn_lw_solver_2stream(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                               const float *inc_flux, const float *tau, const float *ssa, const float *g,
                               const float *lev_source, const float *sfc_emis_gpt, const float *sfc_source,
                               float *flux_up, float *flux_dn);
/* sw_solver_2stream (:541-692).  inc_flux_dif may be NULL (zero, rte/mo_rte_sw.F90:197-210).
 * g may be NULL: asymmetry parameter identically zero, as gas_optics_ext's NN branch produces
 * (mo_gas_optics_rrtmgp.F90:560-567) -- same fluxes as passing a zero-filled array. */
int rrtmgpnn_sw_solver_2stream(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                               const float *inc_flux, const float *inc_flux_dif,
                               const float *tau, const float *ssa, const float *g, const float *mu0,
                               const float *sfc_alb_dir_gpt, const float *sfc_alb_dif_gpt,
                               float *flux_up, float *flux_dn, float *flux_dir);
/* The solvers above with the outputs of ty_fluxes_flexible (rte/mo_fluxes.F90:57-67) and rte_lw's lw_Ds
 * (rte/mo_rte_lw.F90:80-81, 239-246, 329-341).  gpt_flux_* (ngpt, nlay+1, ncol) device arrays, NULL for none.
 * LW: both or neither of gpt_flux_up/dn; with one angle they receive the g-point RADIANCES and the broadband fluxes
 * are reduced from them as lw_solver_noscat does (quirk B-5), with several angles the angle-summed fluxes.  lw_Ds
 * (NULL: the Gauss angles): ngpt*ncol column-dependent secants read as D(igpt, icol) -- the kernel's layout; the
 * reference's rte_lw checks the extents as (ncol, ngpt) but passes the array unchanged (quirk B-12) -- with one angle
 * (nmus must be 1) of weight weights[0].  SW: all three of up, down (TOTAL: diffuse + direct, as the reference
 * stores it) and direct, and the broadband down flux summed from the total (the reference's save_gpt_flux order,
 * :660-684); even ngpt.  Bit-identical to the reference (tests/test_oracle.py, tests/test_gpu_gpt.py). */
int rrtmgpnn_lw_solver_noscat_gpt(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1, int nmus,
                                  const float *Ds, const float *weights, const float *lw_Ds, const float *inc_flux,
                                  const float *tau, const float *lay_source, const float *lev_source,
                                  const float *sfc_emis_gpt, const float *sfc_source, float *flux_up, float *flux_dn,
                                  float *gpt_flux_up, float *gpt_flux_dn);
int rrtmgpnn_lw_solver_noscat_planck_gpt(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1, int nmus,
                                         const float *Ds, const float *weights, const float *lw_Ds,
                                         const float *inc_flux, const float *tau, const float *pfrac, int nbnd,
                                         int nPlanckTemp, const float *tlay, const float *tlev, const float *tsfc,
                                         int sfc_lay, const int *band_lims_gpt, float temp_ref_min,
                                         float totplnk_delta, const float *totplnk, int emis_by_band,
                                         const float *sfc_emis, float *flux_up, float *flux_dn, float *gpt_flux_up,
                                         float *gpt_flux_dn);
int rrtmgpnn_sw_solver_2stream_gpt(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                   const float *inc_flux, const float *inc_flux_dif, const float *tau,
                                   const float *ssa, const float *g, const float *mu0, const float *sfc_alb_dir_gpt,
                                   const float *sfc_alb_dif_gpt, float *flux_up, float *flux_dn, float *flux_dir,
                                   float *gpt_flux_up, float *gpt_flux_dn, float *gpt_flux_dir);
/* rte_sw on absorption-only (1scl) properties (rte/mo_rte_sw.F90:213-222): apply_BC_factor (top level =
 * inc_flux * mu0, rte/kernels/mo_rte_solver_kernels.F90:1685-1704) and sw_solver_noscat (:496-532), broadband direct
 * flux (nlay+1, ncol) = sum over g of each column's direct beam (sum_broadband_nocol, sequential).  The reference's
 * rte_sw swaps the spectral and broadband arguments of sw_solver_noscat (quirk B-10) and the kernel sums column 1 for
 * every column (B-11): this entry follows the kernels' evident meaning; the spectral beam is the reference's bit for
 * bit (tests/test_oracle.py).  inc_flux (ngpt, ncol), tau (ngpt, nlay, ncol), mu0 (ncol). */
int rrtmgpnn_sw_solver_noscat(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1, const float *inc_flux,
                              const float *tau, const float *mu0, float *flux_dir);
/* The scattering LW solvers and the SW direct beam with ty_fluxes_flexible's g-point outputs (ngpt, nlay+1, ncol),
 * both or neither of gpt_flux_up/dn for LW.
 * 1rescl: what lw_solver_noscat_GaussQuad leaves in flux_up_gpt/flux_dn_gpt with do_rescaling (rte/mo_rte_lw.F90:
 *   377-387; kernels :179-281, 383-411): with one angle the radiances of the final up and down passes (quirk B-5),
 *   with several the angle-summed fluxes.
 * 2stream: the adding fluxes lw_solver_2stream forms per g-point (:454-485).
 * noscat (SW, 1scl): the spectral direct beam, top level = inc_flux * mu0 (apply_BC_factor + sw_solver_noscat; the
 *   reference's rte_sw passes a local array to apply_BC_factor when g-point fluxes are desired, :155-163, 218: this
 *   entry applies the boundary condition to the caller's array, the evident meaning, as for B-10/B-11).
 * Broadband outputs as the entries above, bit for bit (tests/test_gpu_gpt.py). */
int rrtmgpnn_lw_solver_1rescl_gpt(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1, int nmus,
                                  const float *Ds, const float *weights, const float *inc_flux, const float *tau,
                                  const float *ssa, const float *g, const float *lay_source, const float *lev_source,
                                  const float *sfc_emis_gpt, const float *sfc_source, float *flux_up, float *flux_dn,
                                  float *gpt_flux_up, float *gpt_flux_dn);
int rrtmgpnn_lw_solver_2stream_gpt(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                   const float *inc_flux, const float *tau, const float *ssa, const float *g,
                                   const float *lev_source, const float *sfc_emis_gpt, const float *sfc_source,
                                   float *flux_up, float *flux_dn, float *gpt_flux_up, float *gpt_flux_dn);
int rrtmgpnn_sw_solver_noscat_gpt(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                  const float *inc_flux, const float *tau, const float *mu0, float *flux_dir,
                                  float *gpt_flux_dir);
/* rrtmgpnn_sw_solver_2stream of the atmosphere incremented by band-resolved two-stream properties
 * (tau, ssa, g)_bnd (nbnd, nlay, ncol) -- clouds%increment(atmos) (inc_2stream_by_2stream_bybnd,
 * rte/kernels/mo_optical_props_kernels.F90:430-463) fused into the solver: same fluxes, bit for bit, as
 * rrtmgpnn_increment_bybnd then rrtmgpnn_sw_solver_2stream; the inputs are left unchanged.  g may be NULL
 * (zero).  band_lims_gpt HOST (2, nbnd) and must put every g-point in a band. */
int rrtmgpnn_sw_solver_2stream_inc(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                   const float *inc_flux, const float *inc_flux_dif, const float *tau,
                                   const float *ssa, const float *g, int nbnd, const int *band_lims_gpt,
                                   const float *tau_bnd, const float *ssa_bnd, const float *g_bnd, const float *mu0,
                                   const float *sfc_alb_dir_gpt, const float *sfc_alb_dif_gpt, float *flux_up,
                                   float *flux_dn, float *flux_dir);
/* Clear-sky beside all-sky SW fluxes of the same columns: rte_sw on the gases (and aerosols), then on the atmosphere
 * incremented by the clouds, as rte_sw of extensions/mo_rrtmgp_clr_all_sky.F90:283-304 calls it twice.  The arguments
 * of rrtmgpnn_sw_solver_2stream_inc in its order, then the clear-sky outputs flux_*_clr (nlay+1, ncol).  flux_up / dn /
 * dir: bit for bit rrtmgpnn_sw_solver_2stream_inc's with the same requests; flux_*_clr: bit for bit
 * rrtmgpnn_sw_solver_2stream's on (tau, ssa, g).  Requests (below): a cloud mask (rrtmgpnn_solver_request_cloud_mask)
 * switches the cloud in the all-sky set only; a 2str aerosol (rrtmgpnn_solver_request_aerosol) goes into both sets,
 * the reference's clear sky being gases plus aerosols (:288-299) -- flux_*_clr are then rrtmgpnn_sw_solver_2stream_inc's
 * with the aerosol as its increment.  Refused: a by-band or Jacobian request, a 1scl aerosol, nbnd == 0, ngpt odd or
 * over 256.  rrtmgpnn_context_set_sw_clr_all selects one launch or two. */
int rrtmgpnn_sw_solver_2stream_clr_all(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                       const float *inc_flux, const float *inc_flux_dif, const float *tau,
                                       const float *ssa, const float *g, int nbnd, const int *band_lims_gpt,
                                       const float *tau_bnd, const float *ssa_bnd, const float *g_bnd, const float *mu0,
                                       const float *sfc_alb_dir_gpt, const float *sfc_alb_dif_gpt, float *flux_up,
                                       float *flux_dn, float *flux_dir, float *flux_up_clr, float *flux_dn_clr,
                                       float *flux_dir_clr);
/* ---- by-band fluxes: ty_fluxes_byband (extensions/mo_fluxes_byband.F90:31-131) ------------------
 * rrtmgpnn_solver_request_byband arms by-band outputs for the NEXT solver call on this context (any of the
 * rrtmgpnn_lw_solver_* / rrtmgpnn_sw_solver_* entries); that call clears the request whether it succeeds or fails.
 * bnd_flux_* are device arrays (nbnd, nlay+1, ncol), band fastest, NULL for "not wanted"; band_lims_gpt HOST
 * (2, nbnd), 1-based, copied by this call: any widths >= 1, any start parity, and the bands need not cover every
 * g-point.  Each value is the reference's sum_byband (extensions/mo_fluxes_byband_kernels.F90:31-50, called at
 * mo_fluxes_byband.F90:103-115) -- start from the band's first g-point, add the others one by one in increasing g -- of
 *   SW two-stream (also _inc and _rfmip): the g-point fluxes rte_sw saves: up, TOTAL down (diffuse + direct, rounded
 *     once per g-point, then added) and direct;
 *   SW no-scattering: the spectral direct beam (bnd_flux_dir only; up / dn are RRTMGPNN_ERR_ARGUMENT);
 *   LW two-stream, and LW no-scattering / rescaled with several angles: the g-point fluxes, as the _gpt entries
 *     return them;
 *   LW no-scattering / rescaled with one angle (also with lw_Ds): the float32 terms the broadband sum adds,
 *     fac * radiance with fac = 2 pi weight -- NOT sum_byband of the _gpt entries' output, which holds bare radiances
 *     there (quirk B-5).  When ngpt % 4 != 0 the reference's broadband sum itself adds bare radiances (fac = 1,
 *     rte/kernels/mo_rte_solver_kernels.F90:287-320), and the by-band values follow it.
 * The sums are formed inside the solver from the LDS rows its ordered broadband sum walks; the call's broadband
 * outputs are bit-identical to the same call without the request.  bnd_flux_dir on an LW entry is
 * RRTMGPNN_ERR_ARGUMENT; a by-band request together with g-point outputs (the _gpt entries) is
 * RRTMGPNN_ERR_UNSUPPORTED (reduce the g-point arrays with rrtmgpnn_sum_byband instead).  Nothing is allocated and
 * the pointers are kernel arguments, so an armed call can be captured in a hipGraph.  bnd_flux_net
 * (net_byband_precalc, mo_fluxes_byband_kernels.F90:54-70) = bnd_flux_dn - bnd_flux_up is left to the caller. */
int rrtmgpnn_solver_request_byband(rrtmgpnn_context *ctx, int nbnd, const int *band_lims_gpt, float *bnd_flux_up,
                                   float *bnd_flux_dn, float *bnd_flux_dir);
/* sum_byband (extensions/mo_fluxes_byband_kernels.F90:31-50) of an existing g-point flux array: gpt_flux
 * (ngpt, nlev, ncol) -> bnd_flux (nbnd, nlev, ncol), device arrays; band_lims_gpt HOST (2, nbnd) as above. */
int rrtmgpnn_sum_byband(rrtmgpnn_context *ctx, int ngpt, int nlev, int ncol, int nbnd, const int *band_lims_gpt,
                        const float *gpt_flux, float *bnd_flux);
/* expand (rte/mo_rte_lw.F90:429-447): (nband,ncol) -> (ngpt,ncol).  band_lims_gpt HOST (2,nband). */
int rrtmgpnn_expand_band_to_gpt(rrtmgpnn_context *ctx, int nband, int ngpt, int ncol, const int *band_lims_gpt,
                                const float *arr_in, float *arr_out);

/* ---- all-sky: cloud optics, increment, delta scaling ------------------ */
/* ty_cloud_optics%load, LUT form (extensions/cloud_optics/mo_cloud_optics.F90:load_lut).  HOST arrays in the
 * coefficient file's Fortran layout: liquid (nsize_liq, nband), ice (nsize_ice, nband, nrghice).
 * band_lims_wvn (2, nband) may be NULL.  Ice roughness starts at 1 (set_ice_roughness). */
int rrtmgpnn_cloud_optics_create_lut(rrtmgpnn_context *ctx, int nband, const float *band_lims_wvn, int nsize_liq,
                                     int nsize_ice, int nrghice, float radliq_lwr, float radliq_upr,
                                     float radice_lwr, float radice_upr, const float *lut_extliq,
                                     const float *lut_ssaliq, const float *lut_asyliq, const float *lut_extice,
                                     const float *lut_ssaice, const float *lut_asyice, rrtmgpnn_cloud_optics **co);
/* Pade form (load_pade): coefficients (nband, nsizereg, ncoef[, nrghice]) with ncoef_ext = 6 ([2/3]
 * approximants) and ncoef_ssa = 5 ([2/2]); size-regime bounds (nsizereg + 1) each; nsizereg must be 3. */
int rrtmgpnn_cloud_optics_create_pade(rrtmgpnn_context *ctx, int nband, const float *band_lims_wvn, int nsizereg,
                                      int ncoef_ext, int ncoef_ssa, int nrghice, const float *pade_extliq,
                                      const float *pade_ssaliq, const float *pade_asyliq, const float *pade_extice,
                                      const float *pade_ssaice, const float *pade_asyice,
                                      const float *sizreg_extliq, const float *sizreg_ssaliq,
                                      const float *sizreg_asyliq, const float *sizreg_extice,
                                      const float *sizreg_ssaice, const float *sizreg_asyice,
                                      rrtmgpnn_cloud_optics **co);
/* Load the RBIN conversion of rrtmgp-cloud-optics-coeffs-{lw,sw}.nc; use_lut selects the method. */
int rrtmgpnn_cloud_optics_load(rrtmgpnn_context *ctx, const char *path, int use_lut, rrtmgpnn_cloud_optics **co);
int rrtmgpnn_cloud_optics_set_ice_roughness(rrtmgpnn_cloud_optics *co, int icergh);
/* host outputs: nband, nrghice, radii = {liq min, liq max, ice min, ice max} (get_min/max_radius_*) */
int rrtmgpnn_cloud_optics_get(const rrtmgpnn_cloud_optics *co, int *nband, int *nrghice, float radii[4]);
int rrtmgpnn_cloud_optics_destroy(rrtmgpnn_cloud_optics *co);
/* cloud_optics (:354-535): clwp, ciwp, reliq, reice (nlay, ncol) -> by band (nband, nlay, ncol).
 * ssa == NULL: 1scl, tau = absorption optical depth; otherwise 2str (tau, ssa, g; g required). */
int rrtmgpnn_cloud_optics_compute(rrtmgpnn_context *ctx, const rrtmgpnn_cloud_optics *co, int ncol, int nlay,
                                  const float *clwp, const float *ciwp, const float *reliq, const float *reice,
                                  float *tau, float *ssa, float *g);
/* ty_optical_props_arry%increment of g-point properties (ngpt, nlay, ncol) by band-resolved ones
 * (nband, nlay, ncol) (rte/mo_optical_props.F90:882-1023, inc_*_bybnd).  ssa_io == NULL: 1scl target;
 * ssa_in == NULL: 1scl increment.  band_lims_gpt HOST (2, nband).  A g-point in no band is left untouched; limits
 * that overlap are RRTMGPNN_ERR_ARGUMENT (the reference would increment such a g-point once per band; the kernel
 * gives a g-point one band), here and in every fused entry that takes a band increment. */
int rrtmgpnn_increment_bybnd(rrtmgpnn_context *ctx, int ncol, int nlay, int ngpt, int nband, const int *band_lims_gpt,
                             float *tau_io, float *ssa_io, float *g_io, const float *tau_in, const float *ssa_in,
                             const float *g_in);
/* Same-resolution increment (increment_*_by_*, rte/kernels/mo_optical_props_kernels.F90:109-219):
 * both sets (ngpt, nlay, ncol); NULL ssa as above. */
int rrtmgpnn_increment(rrtmgpnn_context *ctx, int ncol, int nlay, int ngpt, float *tau_io, float *ssa_io, float *g_io,
                       const float *tau_in, const float *ssa_in, const float *g_in);
/* Heating rate [K/s] per layer, compute_heating_rate (extensions/mo_heating_rates.F90:26-53): grav = 9.80665,
 * cp_dry = 1004.64 (rrtmgp/mo_rrtmgp_constants.F90:50,53).  The extension predates this fork's layout; here fluxes and
 * plev are the fork's (nlay+1, ncol), level fastest, and heating_rate is (nlay, ncol). */
int rrtmgpnn_compute_heating_rate(rrtmgpnn_context *ctx, int ncol, int nlay, const float *flux_up, const float *flux_dn,
                                  const float *plev, float *heating_rate);
/* Heating rate [K/day] as the NN evaluation programs report it, calc_heating_rate
 * (examples/rrtmgp-nn-training/rrtmgp_lw_eval_nn_rfmip.F90:624-653): cp = 1004, -(86400 g / cp) d(F_dn - F_up) / dp.
 * Same layouts as rrtmgpnn_compute_heating_rate. */
int rrtmgpnn_calc_heating_rate_k_day(rrtmgpnn_context *ctx, int ncol, int nlay, const float *flux_up,
                                     const float *flux_dn, const float *plev, float *hr_k_day);
/* The RFMIP SW driver's per-block boundary conditions (examples/rfmip-clear-sky/rrtmgp_rfmip_sw.F90:403-434), with
 * gas_optics_ext's toa_src(igpt, icol) = solar_source(igpt) (rrtmgp/mo_gas_optics_rrtmgp.F90:594-599): per column
 * def_tsi = sum over g of toa_src in g order, toa_flux = toa_src * tsi / def_tsi, sfc_alb_gpt(g, icol) = sfc_alb(icol),
 * mu0 = merge(cos(sza * deg_to_rad), 1, usecol), usecol = sza < 90 - 2 spacing(90) (:236-238), cos with glibc's cosf
 * algorithm (the reference built here links it).  solar_source DEVICE (ngpt) after set_tsi; tsi, sfc_alb, sza DEVICE
 * (ncol); outputs DEVICE toa_flux and sfc_alb_gpt (ngpt, ncol), mu0 (ncol). */
int rrtmgpnn_sw_boundary_rfmip(rrtmgpnn_context *ctx, int ngpt, int ncol, const float *solar_source, const float *tsi,
                               const float *sfc_alb, const float *sza, float *toa_flux, float *sfc_alb_gpt, float *mu0);
/* rrtmgpnn_sw_boundary_rfmip followed by rrtmgpnn_sw_solver_2stream (nbnd == 0) or rrtmgpnn_sw_solver_2stream_inc
 * (nbnd > 0; band_lims_gpt, tau_bnd, ssa_bnd, g_bnd as there), with no diffuse incident flux and the albedo given for
 * both the direct and the diffuse beam, as the RFMIP and all-sky drivers call rte_sw (rrtmgp_rfmip_sw.F90:403-441):
 * the same fluxes, bit for bit.  The checkpointed solver forms the boundary conditions in its prologue (no separate
 * launch); the other solver kernels read them from toa_flux, sfc_alb_gpt and mu0 (DEVICE scratch, (ngpt, ncol),
 * (ngpt, ncol), (ncol); contents unspecified after the call). */
int rrtmgpnn_sw_solver_2stream_rfmip(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                     const float *solar_source, const float *tsi, const float *sfc_alb, const float *sza,
                                     const float *tau, const float *ssa, const float *g, int nbnd,
                                     const int *band_lims_gpt, const float *tau_bnd, const float *ssa_bnd,
                                     const float *g_bnd, float *toa_flux, float *sfc_alb_gpt, float *mu0,
                                     float *flux_up, float *flux_dn, float *flux_dir);
/* rrtmgpnn_sw_solver_2stream_rfmip's arguments (nbnd > 0 required), then the clear-sky outputs: the driver's boundary
 * conditions (rrtmgp_rfmip_sw.F90:403-441) formed once, in the dual kernel's prologue, for both skies of
 * rrtmgpnn_sw_solver_2stream_clr_all (extensions/mo_rrtmgp_clr_all_sky.F90:283-304).  Same requests, refusals and bits
 * as there: rrtmgpnn_sw_boundary_rfmip followed by rrtmgpnn_sw_solver_2stream_clr_all. */
int rrtmgpnn_sw_solver_2stream_rfmip_clr_all(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int top_at_1,
                                             const float *solar_source, const float *tsi, const float *sfc_alb,
                                             const float *sza, const float *tau, const float *ssa, const float *g,
                                             int nbnd, const int *band_lims_gpt, const float *tau_bnd,
                                             const float *ssa_bnd, const float *g_bnd, float *toa_flux,
                                             float *sfc_alb_gpt, float *mu0, float *flux_up, float *flux_dn,
                                             float *flux_dir, float *flux_up_clr, float *flux_dn_clr,
                                             float *flux_dir_clr);
/* ---- McICA cloud sampling: extensions/cloud_optics/mo_cloud_sampling.F90 ---------------------------
 * The extension predates this fork's layout (as mo_heating_rates does).  Here, first index fastest, DEVICE arrays:
 *   randoms (ngpt, nlay, ncol), read only where cloud_frac > 0, as in the reference (:17-18);
 *   cloud_frac (nlay, ncol); overlap_param (nlay-1, ncol), alpha(i) between layers i and i+1 (may be NULL for nlay 1);
 *   cloud_mask (ngpt, nlay, ncol) bytes, 0 / 1: the logical mask of the class layer (draw_samples);
 *   mask_bits  (nw, nlay, ncol) 32-bit words, nw = ceil(ngpt / 32): bit g % 32 of word g / 32 is the mask of
 *     0-based g-point g, unused high bits zero: the form the solvers take (rrtmgpnn_solver_request_cloud_mask).
 * Either output may be NULL, not both.  Random numbers are the caller's in these two entries, as in the reference; the
 * _seeded entries further down draw them inside the kernel from a seed (Philox4x32-10) and read no randoms array.
 * rrtmgpnn_sampled_mask_max_ran (sampled_mask_max_ran, :125-192), maximum-random overlap: a cloudy layer
 *   (cloud_frac > 0) under a cloudy one reuses its random deviates, one under a clear layer takes new ones; the mask is
 *   the strict float32 comparison local_rand > (1 - cloud_frac); clear layers, and so every layer outside the first ..
 *   last cloudy ones, are false.
 * rrtmgpnn_sampled_mask_exp_ran (sampled_mask_exp_ran, :200-285), exponential-random overlap: under a cloudy layer
 *   the deviates are rho * (local - 0.5) + sqrt(1 - rho * rho) * (rand - 0.5) + 0.5 with rho = overlap_param of the
 *   layer pair, evaluated left to right in float32 without fused multiply-adds, the root correctly rounded.
 *   QUIRK: the reference never assigns the mask of a clear layer lying between cloudy ones (its
 *   `if(cloud_mask_layer(ilay))` has no else, :261-279; the mask is intent(out)); here those elements are false, the
 *   evident meaning and what max_ran does.
 * Neither checks values: cloud_frac in [0, 1] and overlap_param in [-1, 1] are the class layer's checks (:151, :233-240),
 * made there with the reference's messages.  Bit-identical masks (tests/test_gpu_mcica.py, tests/golden/mcica_masks.npz). */
int rrtmgpnn_sampled_mask_max_ran(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const float *randoms,
                                  const float *cloud_frac, unsigned char *cloud_mask, unsigned int *mask_bits);
int rrtmgpnn_sampled_mask_exp_ran(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const float *randoms,
                                  const float *cloud_frac, const float *overlap_param, unsigned char *cloud_mask,
                                  unsigned int *mask_bits);
/* ---- McICA with in-kernel random numbers (counter-based, seeded).  No reference counterpart: the reference leaves
 * random numbers to the caller.
 * Generator: Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9,
 * 0xBB67AE85, 10 rounds).  One call gives the four 32-bit words of 4 consecutive layers of one g-point of one column:
 *   counter (g, l >> 2, (col0 + icol) mod 2^32, stream), key (seed & 0xffffffff, seed >> 32),
 *   g the 0-based g-point, l the 0-based layer in array order, icol the 0-based column of the call; the random number
 *   of layer l is word l & 3 as (float)(w >> 8) * 2^-24: exact in float32, in [0, 1 - 2^-24].
 * So a column's numbers depend on (seed, stream, global column col0 + icol, layer, g-point) and on nothing else: the
 * same clouds however the columns are split over ranks, chunks or blocks.  stream is a free word (LW / SW, time
 * steps).  col0 + icol wraps modulo 2^32.
 * rng: a caller-owned DEVICE array of 4 unsigned int, {seed low, seed high, stream, col0}.  The kernels read it on the
 *   device, so a captured hipGraph replays with whatever the words hold at replay time.
 * rrtmgpnn_mcica_rng_set fills rng on the context's stream and is complete on return.  It is a copy from the host:
 *   do not capture it (rewrite the words between replays instead). */
int rrtmgpnn_mcica_rng_set(rrtmgpnn_context *ctx, unsigned long long seed, unsigned int stream, unsigned int col0,
                           unsigned int *rng);
/* The generator's numbers as an array, randoms (ngpt, nlay, ncol) DEVICE: counter (g, l >> 2, (col0 + icol) mod 2^32,
 * stream) as above, col0 + icol wrapping modulo 2^32; what the _seeded mask entries draw, for hosts that want the numbers
 * themselves (rrtmgpnn_sampled_mask_* on this array give the _seeded entries' masks, bit for bit).  No reference
 * counterpart.  ncol == 0 is OK. */
int rrtmgpnn_mcica_randoms(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const unsigned int *rng, float *randoms);
/* rrtmgpnn_sampled_mask_max_ran / _exp_ran with the random numbers drawn in the kernel: counter (g, l >> 2,
 * (col0 + icol) mod 2^32, stream), key (seed low, seed high), word l & 3 (layout above); col0 + icol wraps modulo 2^32.
 * No randoms array is read or allocated; only cloud_frac and overlap_param are streamed, and a group of 4 layers
 * without a cloudy one draws nothing.  Everything after the deviate is the array entries' arithmetic, and their output
 * rules hold: either output may be NULL, not both; overlap_param may be NULL for nlay 1.  No reference counterpart. */
int rrtmgpnn_sampled_mask_max_ran_seeded(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const unsigned int *rng,
                                         const float *cloud_frac, unsigned char *cloud_mask, unsigned int *mask_bits);
/* As above with exponential-random overlap: counter (g, l >> 2, (col0 + icol) mod 2^32, stream), col0 + icol wrapping
 * modulo 2^32.  No reference counterpart. */
int rrtmgpnn_sampled_mask_exp_ran_seeded(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const unsigned int *rng,
                                         const float *cloud_frac, const float *overlap_param,
                                         unsigned char *cloud_mask, unsigned int *mask_bits);
/* The four packed masks above for a block compacted to its daylit columns (rrtmgp_rfmip_sw.F90:285-287, 433, 456-463):
 * idx (ncol) and nact (one DEVICE int) are rrtmgpnn_daylit_plan's idx and nday.  Dense column j < min(max(*nact, 0), ncol)
 * is source column i = idx[j]: its cloud_frac, overlap_param and, on the array route, randoms are read at column i in
 * place (nothing is gathered: all three keep their full extents), and the seeded route's counter word is col0 + i, so a
 * column has the same clouds whether the block is compacted or not.  The words go to row j of a dense mask_bits
 * (nw, nlay, ncol), what rrtmgpnn_solver_request_cloud_mask takes beside rrtmgpnn_solver_request_active_columns; rows at
 * or past the count are not written.  Packed words only.  The argument checks and messages of the full-extent twins;
 * idx, nact or mask_bits NULL is RRTMGPNN_ERR_ARGUMENT; ncol == 0 is OK.  The grid is ncol: the host never reads the
 * count, and nothing is allocated, so the calls capture into a hipGraph.  No reference counterpart. */
int rrtmgpnn_sampled_mask_max_ran_active(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const float *randoms,
                                         const float *cloud_frac, const int *idx, const int *nact,
                                         unsigned int *mask_bits);
/* As above with exponential-random overlap (rrtmgp_rfmip_sw.F90:285-287, 433, 456-463). */
int rrtmgpnn_sampled_mask_exp_ran_active(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const float *randoms,
                                         const float *cloud_frac, const float *overlap_param, const int *idx,
                                         const int *nact, unsigned int *mask_bits);
/* As above with the random numbers drawn in the kernel, counter word (col0 + idx[j]) mod 2^32 (rrtmgp_rfmip_sw.F90:285-287,
 * 433, 456-463). */
int rrtmgpnn_sampled_mask_max_ran_seeded_active(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol,
                                                const unsigned int *rng, const float *cloud_frac, const int *idx,
                                                const int *nact, unsigned int *mask_bits);
/* As above with exponential-random overlap (rrtmgp_rfmip_sw.F90:285-287, 433, 456-463). */
int rrtmgpnn_sampled_mask_exp_ran_seeded_active(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol,
                                                const unsigned int *rng, const float *cloud_frac,
                                                const float *overlap_param, const int *idx, const int *nact,
                                                unsigned int *mask_bits);
/* draw_samples / apply_cloud_mask (:36-120, :291-307): per g-point the band value (nbnd, nlay, ncol) where cloud_mask is
 * set, else 0, into (ngpt, nlay, ncol).  tau always; ssa and g when all of ssa_bnd, g_bnd, ssa, g are given (2str),
 * none of them for 1scl.  band_lims_gpt HOST (2, nbnd), every g-point in a band. */
int rrtmgpnn_draw_samples(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, int nbnd, const int *band_lims_gpt,
                          const unsigned char *cloud_mask, const float *tau_bnd, const float *ssa_bnd,
                          const float *g_bnd, float *tau, float *ssa, float *g);
/* Arms the packed cloud mask mask_bits (layout above) for the NEXT solver call on this context; that call clears the
 * request whether it succeeds or fails (mask_bits == NULL: nothing armed).  The fused increments then switch the band
 * value on or off per g-point: where a bit is clear the band operands are 0 (tau_bnd; and ssa_bnd, g_bnd in the SW), and
 * everything downstream is the _inc arithmetic, so the fluxes are bit for bit those of rrtmgpnn_draw_samples +
 * rrtmgpnn_increment (same resolution; inc_2stream_by_2stream with a zero increment still rounds
 * tau * ssa / max(eps, tau), and so does this) + the solver, without the g-point cloud arrays.  Honoured by
 * rrtmgpnn_lw_solver_noscat_planck_inc and rrtmgpnn_lw_solver_1rescl_planck_inc (every nmus; the latter switches
 * tau_bnd, ssa_bnd and g_bnd), rrtmgpnn_sw_solver_2stream_inc,
 * rrtmgpnn_sw_solver_2stream_rfmip with nbnd > 0 and rrtmgpnn_sw_solver_2stream_clr_all / _rfmip_clr_all (the all-sky
 * set only), the SW ones on the checkpointed kernel (the default of
 * rrtmgpnn_context_set_sw_kernel: even ngpt; other modes, and odd ngpt, RRTMGPNN_ERR_UNSUPPORTED).  Extents other than
 * the call's: RRTMGPNN_ERR_ARGUMENT; every other solver entry (the plain ones, _clr_all, _clr_all_mcica, which takes
 * its mask as an argument, the _gpt entries, the other scattering LW entries, _rfmip with nbnd == 0): RRTMGPNN_ERR_ARGUMENT;
 * together with a separate by-band request: RRTMGPNN_ERR_UNSUPPORTED (rrtmgpnn_solver_request_byband_mcica below
 * requests the pair).  The pointer becomes a kernel argument and nothing is allocated, so an armed call can be captured
 * in a hipGraph.  No reference counterpart (the reference samples into g-point arrays, draw_samples). */
int rrtmgpnn_solver_request_cloud_mask(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol,
                                       const unsigned int *mask_bits);
/* By-band fluxes under a McICA-sampled cloud: arms the by-band outputs of rrtmgpnn_solver_request_byband (the same
 * arrays, band limits and rules: any widths, any start parity, not necessarily every g-point; independent of the cloud
 * bands of the increment) and the packed mask of rrtmgpnn_solver_request_cloud_mask TOGETHER, as a pair, for the NEXT
 * solver call on this context; that call clears both whether it succeeds or fails.  The two separate requests beside
 * each other stay refused (RRTMGPNN_ERR_UNSUPPORTED: a by-band request left from an earlier call beside a fresh mask
 * is a mistake); this entry states the pair.  A later separate rrtmgpnn_solver_request_byband or
 * rrtmgpnn_solver_request_cloud_mask replaces its half and drops the pairing.
 * RRTMGPNN_ERR_ARGUMENT, with nothing armed and whatever was armed cleared: mask_bits NULL, all three outputs NULL,
 * ngpt < 1, nlay < 1, ncol < 0, nbnd outside 1..64, band limits outside [1, ngpt] or first > last.
 * Honoured by rrtmgpnn_lw_solver_noscat_planck_inc (every nmus; bnd_flux_dir must be NULL: RRTMGPNN_ERR_ARGUMENT),
 * rrtmgpnn_sw_solver_2stream_inc and rrtmgpnn_sw_solver_2stream_rfmip with nbnd > 0, the SW ones on the checkpointed
 * kernel (other modes of rrtmgpnn_context_set_sw_kernel, odd ngpt: RRTMGPNN_ERR_UNSUPPORTED).  Mask extents other than
 * the call's: RRTMGPNN_ERR_ARGUMENT.  Every entry that refuses a cloud mask refuses the pair and clears it.
 * The by-band values are those of the _inc entries with a by-band request (one angle: the float32 terms the broadband
 * sum adds; SW: up, total down, direct), on the sampled optical properties: bit for bit rrtmgpnn_draw_samples +
 * rrtmgpnn_increment + the plain solver with rrtmgpnn_solver_request_byband.  The call's broadband fluxes are bit for
 * bit those of the same masked call without by-band outputs.  Nothing is allocated and the pointers become kernel
 * arguments, so an armed call can be captured in a hipGraph.  No reference counterpart. */
int rrtmgpnn_solver_request_byband_mcica(rrtmgpnn_context *ctx, int nbnd, const int *band_lims_gpt, float *bnd_flux_up,
                                         float *bnd_flux_dn, float *bnd_flux_dir, int ngpt, int nlay, int ncol,
                                         const unsigned int *mask_bits);
/* rte_lw's flux_up_Jac: the Jacobian of the upward LW flux with respect to the surface temperature, at every level,
 * carried through the NEXT solver call on this context beside its upward radiance; that call clears the request whether
 * it succeeds or fails (flux_up_Jac == NULL: nothing armed).  flux_up_Jac DEVICE (nlay+1, ncol); sfc_source_Jac DEVICE
 * (ngpt, ncol), what rrtmgpnn_compute_planck_source_nn writes.  The reference's path
 * (rte/kernels/mo_rte_solver_kernels.F90:270, 290, 319, 390-411, 967, 975, 1761, 1782) is compiled out by compute_Jac =
 * .false. (rte/mo_rte_rrtmgp_config.F90:28); per column and g-point, in float32:
 *   J = sfc_emis * sfc_source_Jac at the surface, J = T * J through each layer going up, T the transmittance that
 *   multiplies the upward radiance there (of the incremented or masked tau; the rescaled one in lw_solver_1rescl),
 * and flux_up_Jac sums J over g-points exactly as the call sums flux_up (one angle: fac * J in four partial sums, the
 * bare J sequentially when ngpt % 4 != 0; several angles: fac * J accumulated per g-point in angle order, then summed
 * sequentially).  So flux_up_Jac is bit for bit the flux_up the same entry returns on the same optical properties with
 * zero layer and level sources, no incident flux and sfc_source_Jac as the surface source.  There is no downward
 * Jacobian.  The call's flux_up and flux_dn are bit for bit those of the call without the request.
 * Honoured by rrtmgpnn_lw_solver_noscat, rrtmgpnn_lw_solver_noscat_gpt without g-point outputs (lw_Ds is honoured) and
 * rrtmgpnn_lw_solver_1rescl, which need sfc_source_Jac, and by rrtmgpnn_lw_solver_noscat_planck and
 * rrtmgpnn_lw_solver_noscat_planck_inc (also beside a cloud-mask request), which form it in-kernel as
 * pfrac(g, sfc_lay) * (B_b(tsfc + 1) - B_b(tsfc)) and for which sfc_source_Jac must be NULL.  RRTMGPNN_ERR_ARGUMENT or
 * RRTMGPNN_ERR_UNSUPPORTED, with a message naming the entry: the NULL / non-NULL rule broken, extents other than the
 * call's, any by-band request beside it, g-point outputs, the _clr_all entries, every SW entry, and
 * rrtmgpnn_lw_solver_2stream ("rte_lw: can't provide Jacobian of fluxes w.r.t surface temperature with 2-stream").
 * Nothing is allocated beyond the context workspace and the pointers become kernel arguments. */
int rrtmgpnn_solver_request_jacobian(rrtmgpnn_context *ctx, int ngpt, int nlay, int ncol, const float *sfc_source_Jac,
                                     float *flux_up_Jac);
/* Aerosols (aer_props of extensions/mo_rrtmgp_clr_all_sky.F90:155-157, 288-290): a second band increment applied by the
 * NEXT solver call on this context in front of its fused band increment; that call clears the request whether it succeeds
 * or fails (all three arrays NULL: nothing armed).  tau_aer DEVICE (nbnd, nlay, ncol) on the call's own bands; ssa_aer and
 * g_aer both NULL for a 1scl (LW) aerosol, both set for a 2str (SW) one.  Per g-point, in float32, two separately
 * rounded adds in the reference's order, aerosols then clouds:
 *   ta = tau + tau_aer(band);  t = ta + tau_bnd(band), or ta + (bit ? tau_bnd(band) : 0) under a cloud mask,
 * bit for bit rrtmgpnn_increment_bybnd by the aerosol, then the entry's own increment, then the plain solver.  The sum of
 * the two increments or the other order gives other float32 values, so the two cannot be added on the host; a mask
 * switches the cloud and never the aerosol.
 * In the SW the properties are inc_2stream_by_2stream_bybnd (rte/kernels/mo_optical_props_kernels.F90:430-463) by the
 * aerosol, then by the (mask-selected) cloud; the gas g may be NULL as in the entry without the request (the literal 0
 * then goes into the first increment, so gas optics writes no g array).  A zero aerosol is still an increment (it
 * rounds tau * ssa / max(eps, tau)), not the call without the request.
 * Honoured, for a 1scl aerosol, by rrtmgpnn_lw_solver_noscat_planck_inc (nmus 1..4, also beside a cloud-mask request)
 * and by rrtmgpnn_lw_solver_noscat_planck_clr_all and _clr_all_mcica, whose clear-sky outputs are then the fluxes of
 * tau + tau_aer(band) (gases plus aerosols, as the reference defines clear sky) and whose all-sky outputs those of
 * (tau + tau_aer(band)) + [bit ?] tau_bnd(band); with two launches (mode 2, or nmus > 1) the clear launch is the _planck_inc
 * instance with the aerosol as its increment.  Honoured, for a 2str aerosol, by rrtmgpnn_sw_solver_2stream_inc,
 * rrtmgpnn_sw_solver_2stream_rfmip with nbnd > 0 and rrtmgpnn_sw_solver_2stream_clr_all / _rfmip_clr_all (both flux
 * sets; the dual kernel, mode 1 of rrtmgpnn_context_set_sw_clr_all, takes any band layout), on the checkpointed kernel (even ngpt, rrtmgpnn_context_set_sw_kernel
 * mode 0 or 3) with every band starting at an odd 1-based g-point, with or without a cloud-mask request; the
 * transmittance plane of the all-sky instances is used when its workspace fits, the same bits without it.
 * Clear sky with aerosols and no clouds needs no request and no kernel of its own: it is the existing
 * rrtmgpnn_lw_solver_noscat_planck_inc, rrtmgpnn_sw_solver_2stream_inc or rrtmgpnn_sw_solver_2stream_rfmip (nbnd > 0)
 * call with the aerosol arrays as its band increment.
 * RRTMGPNN_ERR_ARGUMENT: nbnd, nlay or ncol other than the call's; a 2str aerosol for an LW entry or a 1scl one for an SW
 * entry; every other solver entry, with a message naming the entries that take it.  RRTMGPNN_ERR_UNSUPPORTED: any by-band
 * request or a flux-Jacobian request beside it; in the SW also the other kernel modes, odd ngpt and a band starting at
 * an even 1-based g-point.
 * Nothing is allocated and the pointers become kernel arguments, so an armed call can be captured in a hipGraph. */
int rrtmgpnn_solver_request_aerosol(rrtmgpnn_context *ctx, int nbnd, int nlay, int ncol, const float *tau_aer,
                                    const float *ssa_aer, const float *g_aer);
/* ---- daylit columns: device-side column compaction for the shortwave chain ----------------------------
 * The RFMIP driver marks the columns where the sun is up (usecol, examples/rfmip-clear-sky/rrtmgp_rfmip_sw.F90:285-287),
 * solves the others with mu0 = 1 (:433) and zeroes their fluxes afterwards (:456-463).  These entries compact a block
 * to its daylit columns instead: plan, gather the inputs into dense arrays, run rrtmgpnn_gas_optics_sw_nn_active and an
 * SW solver armed with rrtmgpnn_solver_request_active_columns on them, scatter the fluxes back with zeros at night.
 * The number of daylit columns is one int (32 bits) in DEVICE memory that the kernels read: the host never sees it, so
 * a hipGraph captured once serves any day / night pattern.  Every array argument is a DEVICE pointer; src[], dst[],
 * dense[], out[] and row_floats[] themselves are HOST arrays.
 *
 * rrtmgpnn_daylit_plan (rrtmgp_rfmip_sw.F90:285-287, 433, 456-463): v (ncol); kind 0: column i is daylit iff
 * v[i] < bound (the driver's form on the zenith angle, bound = 90 - 2 spacing(90)), kind 1: iff v[i] > bound (callers
 * that hold mu0); a NaN is night under both.  idx (ncol): the daylit columns in increasing order, then the night columns
 * in increasing order (a permutation of 0..ncol-1); slot (ncol): the dense position of a daylit column, -1 for a night
 * column; nday: their count.  The order is stable: dense column j is the j-th daylit column.  In all five
 * entries ncol == 0 launches nothing (nday is then left as it was). */
int rrtmgpnn_daylit_plan(rrtmgpnn_context *ctx, int ncol, const float *v, int kind, float bound, int *idx, int *slot,
                         int *nday);
/* rrtmgpnn_gather_columns (rrtmgp_rfmip_sw.F90:285-287, 433, 456-463): one launch; for each of the narrays (1..16)
 * arrays of row_floats[a] floats per column, row idx[j] of src[a] goes to row j of dst[a] for j < *nday.  Rows of dst at
 * or past *nday are left as they were.  Rows need no alignment beyond a float's.  A table whose rows are all at least
 * 256 floats (an aerosol's band arrays) runs a kernel with one block per column and array; put such arrays in a call
 * of their own. */
int rrtmgpnn_gather_columns(rrtmgpnn_context *ctx, int ncol, int narrays, const float *const *src, float *const *dst,
                            const int *row_floats, const int *idx, const int *nday);
/* rrtmgpnn_scatter_columns (rrtmgp_rfmip_sw.F90:285-287, 433, 456-463): one launch; for each of the narrays (1..6)
 * arrays, column i of out[a] (row_floats[a], ncol) is row slot[i] of dense[a] where slot[i] >= 0 and zeros otherwise:
 * the driver's zeroing of the unused columns.  It applies to flux_dir as well, which the driver leaves at its mu0 = 1
 * value: here a night column's direct flux is 0. */
int rrtmgpnn_scatter_columns(rrtmgpnn_context *ctx, int ncol, int narrays, const float *const *dense, float *const *out,
                             const int *row_floats, const int *slot);
/* rrtmgpnn_gas_optics_sw_nn on the first *nact columns of dense arrays (rrtmgp_rfmip_sw.F90:285-287, 433, 456-463):
 * the same arguments, ncol the allocated extent of every array, nact one DEVICE int with 0 <= *nact <= ncol.  Samples
 * at or past nlay * (*nact) are neither read nor written.  Served by the in-kernel-input SW pairs of the 32x32x2 kernel
 * (the g224 and g112 models) only: RRTMGPNN_ERR_UNSUPPORTED for any other networks, for ssa == NULL and under
 * rrtmgpnn_context_set_mlp_kernel mode 1.  rrtmgpnn_context_get_mlp_path then reports flag bit 16. */
int rrtmgpnn_gas_optics_sw_nn_active(rrtmgpnn_context *ctx, int ncol, int nlay, int ngpt, int ninputs,
                                     const float *play, const float *tlay, const float *plev, const float *vmr_h2o,
                                     const float *const *gas_conc, const int *gas_ndims,
                                     const rrtmgpnn_network *const *nets, float *tau, float *ssa, float *g,
                                     const int *nact);
/* Ask this context's next solver call to solve the first *nact of its ncol columns only (rrtmgp_rfmip_sw.F90:285-287,
 * 433, 456-463): nact one DEVICE int, 0 <= *nact <= ncol, read by the kernel.  Flux rows at or past *nact are not
 * written.  Armed for one call, cleared by it whatever it returns; nact == NULL disarms.
 * Honoured by rrtmgpnn_sw_solver_2stream, rrtmgpnn_sw_solver_2stream_inc and rrtmgpnn_sw_solver_2stream_rfmip on the
 * checkpointed kernel (even ngpt, rrtmgpnn_context_set_sw_kernel mode 0 or 3), kernel family 7 of
 * rrtmgpnn_context_get_solver_path: the instances of family 2 with option bit 2048, for g == NULL and without or with
 * the band increment.  The instance and its workspace are chosen from ncol, as without the request.
 * On rrtmgpnn_sw_solver_2stream_inc and on rrtmgpnn_sw_solver_2stream_rfmip with nbnd > 0 it is also honoured together
 * with rrtmgpnn_solver_request_cloud_mask, rrtmgpnn_solver_request_aerosol (2str) or both (kernel family 8: a McICA
 * step on daylit columns): the mask's and the aerosol's extents are the call's ncol, their rows those of the dense
 * columns (rrtmgpnn_sampled_mask_*_active writes such a mask).
 * RRTMGPNN_ERR_ARGUMENT: every other solver entry, with a message naming the three; ncol other than the call's; a mask
 * or an aerosol of other extents than the call's.
 * Refused: RRTMGPNN_ERR_UNSUPPORTED, every armed request cleared, nothing written -- a by-band request beside it, alone
 * or paired with the mask (rrtmgpnn_solver_request_byband_mcica); a Jacobian request; a cloud-mask or aerosol request
 * ahead of rrtmgpnn_sw_solver_2stream; g-point outputs; a gas g array; an aerosol on bands outside the band-pair
 * layout; the other SW kernel modes; odd ngpt.  The clear + all-sky (_clr_all) entries take no count
 * (RRTMGPNN_ERR_ARGUMENT). */
int rrtmgpnn_solver_request_active_columns(rrtmgpnn_context *ctx, int ncol, const int *nact);
/* Ask this context's next solver call for the shortwave fluxes at the surface by band (ty_fluxes_byband,
 * extensions/mo_fluxes_byband.F90, at the surface level alone): what a host hands to its land, ocean and sea-ice models.
 * band_lims_gpt: HOST (2, nbnd), 1-based, copied by the call under the rules of rrtmgpnn_solver_request_byband.
 * sfc_bnd_up / sfc_bnd_dn / sfc_bnd_dir: DEVICE (nbnd, ncol), band fastest; a NULL pointer is not wanted, all three NULL
 * disarm.  Armed for one call, cleared by it whatever it returns.
 * The values are, bit for bit, what rrtmgpnn_solver_request_byband puts at the surface level (array index nlay when
 * top_at_1, else 0): sum_byband -- the band's first g-point, then the others one by one in increasing g -- of the
 * g-point up flux, the total down flux (diffuse + direct, rounded once per g-point) and the direct flux.  The call's
 * broadband outputs are those of the same call without the request.  Nothing is allocated and the pointers are kernel
 * arguments, so an armed call can be captured in a hipGraph.
 * Honoured by rrtmgpnn_sw_solver_2stream_inc and by rrtmgpnn_sw_solver_2stream_rfmip with nbnd > 0 on the checkpointed
 * kernel (even ngpt, rrtmgpnn_context_set_sw_kernel mode 0 or 3) for g == NULL, bands in the band-pair layout and a
 * cloud-mask request, a 2str aerosol request or both taken by the same call, with an active-column request beside them
 * or without (rows at or past *nact are not written): kernel family 9 of rrtmgpnn_context_get_solver_path.
 * RRTMGPNN_ERR_ARGUMENT: every other solver entry, with a message naming the two; ncol other than the call's; nbnd or
 * limits other than the call's increment bands.
 * Refused: RRTMGPNN_ERR_UNSUPPORTED, every armed request cleared, nothing written -- neither a mask nor an aerosol
 * beside it (rrtmgpnn_solver_request_byband has the surface level in its outputs); a by-band request beside it, alone or
 * as the _byband_mcica pair; a gas g array; bands outside the band-pair layout; the other SW kernel modes; odd ngpt.  A
 * Jacobian request beside it is refused as the two entries refuse it alone (RRTMGPNN_ERR_ARGUMENT; beside an
 * active-column request, that request's RRTMGPNN_ERR_UNSUPPORTED): an earlier request's refusal stands. */
int rrtmgpnn_solver_request_sfc_byband(rrtmgpnn_context *ctx, int nbnd, const int *band_lims_gpt, int ncol,
                                       float *sfc_bnd_up, float *sfc_bnd_dn, float *sfc_bnd_dir);
/* ty_optical_props_2str%delta_scale([for]) (rte/mo_optical_props.F90:576-604; kernels
 * rte/kernels/mo_optical_props_kernels.F90:41-92) on n values in place.  fwd == NULL: f = g**2. */
int rrtmgpnn_delta_scale_2str(rrtmgpnn_context *ctx, long long n, float *tau, float *ssa, float *g, const float *fwd);

/* ---- data files ---------------------------------------------------------
 * Native readers for the files the path consumes, replacing the netCDF-Fortran calls of
 * neural/mod_network_rrtmgp.F90:58-122 (load_netcdf), examples/all-sky/mo_load_cloud_coefficients.F90 and
 * examples/rfmip-clear-sky/mo_rfmip_io.F90: classic netCDF (CDF-1/2/5, parsed natively), netCDF-4 (HDF5,
 * through libhdf5 bound at run time: RRTMGPNN_HDF5_LIB or the loader path) and this repository's RBIN.
 * rrtmgpnn_network_load and rrtmgpnn_cloud_optics_load accept all three.  A file is read whole on open;
 * dims are in file (C) order; dtype 0 float32 (floating-point variables, doubles rounded), 1 int32,
 * 2 char.  Variable-length strings and netCDF-4 dimension-only scales are not exposed.  Host memory only. */
int rrtmgpnn_file_open(const char *path, rrtmgpnn_file **f);
int rrtmgpnn_file_close(rrtmgpnn_file *f);
int rrtmgpnn_file_nvars(const rrtmgpnn_file *f, int *nvars);
int rrtmgpnn_file_var_name(const rrtmgpnn_file *f, int i, char *name, int len);
/* dims: room for 8 entries */
int rrtmgpnn_file_var(const rrtmgpnn_file *f, const char *name, int *dtype, int *ndim, long long *dims);
/* count = number of elements; numeric variables convert to the requested dtype (0 or 1) */
int rrtmgpnn_file_read(const rrtmgpnn_file *f, const char *name, int dtype, void *out, long long count);
/* text attribute `att` of variable `var` (NULL or "": global) */
int rrtmgpnn_file_att(const rrtmgpnn_file *f, const char *var, const char *att, char *text, int len);

#ifdef __cplusplus
}
#endif
#endif /* RRTMGPNN_H */
