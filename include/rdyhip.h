/*
 * rdyhip.h -- C ABI of the MI355X-native shallow-water RHS operator.
 *
 * This library replaces ONE path of RDycore: the operator that PETSc's
 * explicit TS calls for every right-hand-side evaluation (first-order Roe
 * fluxes over edges + bed-slope / Manning friction / external sources over
 * cells).  Every entry point below names the RDycore interface it stands in
 * for (file:line relative to the RDycore source tree); INTEGRATION.md shows
 * the adapter a maintainer would add on the RDycore side.
 *
 * Conventions
 *  - plain C, no PETSc / torch types: pointers, sizes, an opaque handle;
 *  - every function returns 0 on success (PETSC_SUCCESS) or one of the
 *    RDYHIP_ERR_* codes, whose values are PETSc's (petscerror.h) so an adapter
 *    can pass them straight to PetscCall(); rdyhip_last_error() gives the text;
 *  - "device" pointers are HIP device memory on the device that was current at
 *    rdyhip_create(); "host" pointers are ordinary memory;
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *    the apply calls enqueue work and return without synchronising;
 *  - indices are 32-bit (a PetscInt=int32 build; a 64-bit-PetscInt adapter
 *    narrows local indices, which always fit), global ids are 64-bit;
 *  - one operator per rank, one rank per GPU, no threads (as in the reference).
 */
#ifndef RDYHIP_H
#define RDYHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDYHIP_VERSION 110

/* error codes = PETSc's values */
#define RDYHIP_SUCCESS 0
#define RDYHIP_ERR_MEM 55      /* PETSC_ERR_MEM */
#define RDYHIP_ERR_ARG_SIZ 60  /* PETSC_ERR_ARG_SIZ */
#define RDYHIP_ERR_ARG_OUTOFRANGE 63
#define RDYHIP_ERR_LIB 76      /* PETSC_ERR_LIB: a HIP runtime call failed */
#define RDYHIP_ERR_USER 83     /* PETSC_ERR_USER */

/* RDyConditionType (include/rdycore.h:133-139) */
#define RDYHIP_CONDITION_DIRICHLET 0
#define RDYHIP_CONDITION_REFLECTING 2
#define RDYHIP_CONDITION_CRITICAL_OUTFLOW 3

/* RDyFlowSourceMethod (include/private/rdyconfigimpl.h:52-56) */
#define RDYHIP_SOURCE_SEMI_IMPLICIT 0
#define RDYHIP_SOURCE_IMPLICIT_XQ2018 1

/* RDyWellBalanceMethod (include/private/rdyconfigimpl.h:58-62).  BS2002 exists only in
 * the reference's CEED backend (src/operator.c:388) and is rejected here too. */
#define RDYHIP_WELL_BALANCING_NONE 0
#define RDYHIP_WELL_BALANCING_HR 2

/* RDyLimiterType (include/private/rdyconfigimpl.h:64-71): slope limiter of the second-order reconstruction */
#define RDYHIP_LIMITER_MINMOD 0
#define RDYHIP_LIMITER_NONE 1
#define RDYHIP_LIMITER_VANLEER 2

/* RDyNumericsRiemann (include/private/rdyconfigimpl.h:118-122); only Roe exists
 * in the reference (src/swe/swe_petsc.c:264-270) */
#define RDYHIP_RIEMANN_ROE 0

/* The scalars of RDyConfig that reach the kernels
 * (config.physics.flow.{tiny_h,h_anuga_regular,source.method,source.xq2018_threshold,well_balancing},
 *  config.numerics.riemann; include/private/rdyconfigimpl.h:73-85,125-132). */
typedef struct {
  double  tiny_h;
  double  h_anuga_regular;
  double  xq2018_threshold;
  int32_t source_method; /* RDYHIP_SOURCE_* */
  int32_t riemann;       /* RDYHIP_RIEMANN_ROE */
  int32_t well_balancing; /* RDYHIP_WELL_BALANCING_*: HR = ApplyInteriorFluxHR + bed-slope-free source
                             (src/swe/swe_petsc.c:1000-1263); the mesh must then carry cell_zc and, as the
                             reference does (RDyMeshOverride2DProjection, src/rdymesh.c:1478-1509), x-y
                             projected edge lengths and cell areas */
  int32_t second_order;  /* config.numerics.second_order (rdyconfigimpl.h:129): MUSCL reconstruction of the interior
                            face states, ApplyInteriorFlux2R (src/swe/swe_petsc.c:98-213); the mesh must then carry
                            cell_centroids, edge_vertex_ids and vertex_points; not combinable with HR (src/operator.c:388-389) */
  int32_t limiter;       /* RDYHIP_LIMITER_* (config.numerics.limiter after the -no_limiter / -van_leer overrides,
                            src/swe/swe_petsc.c:357-367); read only if second_order */
  int32_t flags;         /* RDYHIP_CONFIG_* bits; 0 = defaults */
} RDyHipConfig;

/* RDyHipConfig.flags.
 * CACHED_F_STORES: the tiled kernels store F with the default cache policy instead of the non-temporal hint.  For a host that
 *   reads F straight back in a separate kernel -- PETSc's TSEULER: VecAXPY(U, dt, F) after every RHS (TSStep_Euler) -- the
 *   hint costs ~6 % of the RHS + axpy pair, because F has then left the Infinity Cache (DESIGN.md section 7 note 6); a host
 *   that takes the step through rdyhip_euler_step (F never stored) or lets F sit (RK stages summed later) leaves it clear.
 *   Honoured by the first-order and HR tiled kernels; the second-order kernels keep the hint. */
#define RDYHIP_CONFIG_CACHED_F_STORES 1
/* STREAMED_NORMALS: keeps the normal table off (see rdyhip_normal_table_info): every first-order / HR launch streams one
 *   double per edge record and rebuilds the normal from it, whatever the mesh.  The results are the same to the last bit
 *   either way; the bit is there for tests and for A/B timings of the two kernel families. */
#define RDYHIP_CONFIG_STREAMED_NORMALS 2

/* The RDyMesh arrays the SWE operators read (include/private/rdymeshimpl.h:26-202).
 * All host pointers, borrowed for the duration of rdyhip_create() only. */
typedef struct {
  int32_t num_cells;          /* mesh->num_cells (owned + ghost) */
  int32_t num_owned_cells;    /* mesh->num_owned_cells */
  int32_t num_edges;          /* mesh->num_edges */
  int32_t num_internal_edges; /* mesh->num_internal_edges */
  const int32_t *cell_is_owned;       /* cells.is_owned       [num_cells] */
  const int32_t *cell_local_to_owned; /* cells.local_to_owned [num_cells] */
  const int64_t *cell_global_ids;     /* cells.global_ids     [num_cells] */
  const double  *cell_areas;          /* cells.areas          [num_cells] */
  const double  *cell_dz_dx;          /* cells.dz_dx          [num_cells] */
  const double  *cell_dz_dy;          /* cells.dz_dy          [num_cells] */
  const int32_t *edge_cell_ids;       /* edges.cell_ids       [2*num_edges], right = -1 on the boundary */
  const int32_t *edge_internal_ids;   /* edges.internal_edge_ids [num_internal_edges] */
  const int64_t *edge_global_ids;     /* edges.global_ids     [num_edges] */
  const double  *edge_lengths;        /* edges.lengths        [num_edges] */
  const double  *edge_cn;             /* edges.cn             [num_edges] */
  const double  *edge_sn;             /* edges.sn             [num_edges] */
  const double  *cell_zc;             /* vertex-averaged bed elevation per cell [num_cells] (InteriorFluxHROperator.zc,
                                         src/swe/swe_petsc.c:1209-1224); may be NULL unless well_balancing == HR */
  /* second_order only (may be NULL / 0 otherwise): what PrecomputeLSGradCoeffs and ReconstructFaceValues read
   * (src/operator_fluxes_ceed.c:884-980, 1155-1206) */
  int32_t        num_vertices;        /* mesh->num_vertices */
  const double  *cell_centroids;      /* cells.centroids      [num_cells][3]    (RDyPoint.X) */
  const int32_t *edge_vertex_ids;     /* edges.vertex_ids     [2*num_edges] */
  const double  *vertex_points;       /* vertices.points      [num_vertices][3] (RDyPoint.X) */
  const int32_t *edge_is_owned;       /* edges.is_owned       [num_edges] (PetscBool; src/rdymesh.c:571-599).  Read by second_order
                                         only: ApplyInteriorFlux2R evaluates the Courant number of an edge on the rank that owns
                                         it (src/swe/swe_petsc.c:172-190); NULL: every edge of an owned cell counts (one rank) */
} RDyHipMesh;

/* RDyBoundary (include/private/rdyboundaryimpl.h:7-14) + the flow condition
 * type of the RDyCondition attached to it (include/private/rdyconditionimpl.h:12-24). */
typedef struct {
  int32_t        num_edges;
  const int32_t *edge_ids; /* local edge ids, host, borrowed during create */
  int32_t        condition_type; /* RDYHIP_CONDITION_* */
} RDyHipBoundary;

/* CourantNumberDiagnostics (include/private/rdyoperatorimpl.h:21-25) */
typedef struct {
  double  max_courant_num;
  int64_t global_edge_id;
  int64_t global_cell_id;
} RDyHipCourant;

/* opaque Operator (include/private/rdyoperatorimpl.h:103-201) */
typedef struct RDyHipOperator_s *RDyHipOperator;

/* device-resident operator fields that may be read (or, for inputs, written)
 * in place; see rdyhip_field_ptr() */
typedef enum {
  RDYHIP_FIELD_PRIMITIVE_VARIABLES = 0, /* Operator.primitive_variables [owned][3] (h,u,v); out.  Stored by the evaluations from the
                                           first rdyhip_field_ptr / _const for it until rdyhip_field_release (see there) */
  RDYHIP_FIELD_EXTERNAL_SOURCES    = 1, /* Operator.petsc.external_sources [owned][3]; in; also src_inst.  Read-only users
                                           take it through rdyhip_field_ptr_const (see "the water-source plane" below) */
  RDYHIP_FIELD_MANNINGS            = 2, /* Operator.petsc.material_properties [owned][1]; in */
  RDYHIP_FIELD_FLUX_DIVERGENCE     = 3, /* Operator.flux_divergence [owned][3]; out, only if enabled */
  RDYHIP_FIELD_GRADIENTS           = 4, /* second order: InteriorFluxOperator.grad_h/grad_hu/grad_hv interleaved,
                                           [num_cells][6] = (dh/dx, dh/dy, dhu/dx, dhu/dy, dhv/dx, dhv/dy), LOCAL cell index:
                                           owned rows are written by rdyhip_compute_gradients, ghost rows by the caller's
                                           halo exchange (CommunicateCellGradients, src/operator_fluxes_ceed.c:1058-1107) */
} RDyHipField;

/* which cells a partial apply covers (multi-GPU overlap, see rdyhip_apply_phase) */
#define RDYHIP_PHASE_ALL 0
#define RDYHIP_PHASE_INTERIOR 1 /* owned cells with no ghost neighbour */
#define RDYHIP_PHASE_HALO 2     /* owned cells with at least one ghost neighbour */

const char *rdyhip_last_error(void);
int32_t     rdyhip_version(void);

/* ---- lifecycle -------------------------------------------------------------
 * CreateOperator(RDyConfig*, DM, RDyMesh*, num_comp, num_regions, RDyRegion*,
 *                num_boundaries, RDyBoundary*, RDyCondition*, Operator**)
 *   include/private/rdyoperatorimpl.h:208, src/operator.c:348-417;
 * together with CreatePetscSWEInteriorFluxOperator / ...BoundaryFluxOperator /
 * ...SourceOperator (include/private/rdysweimpl.h:37-42, src/swe/swe_petsc.c:341,653,948).
 * num_comp is fixed at 3 (SWE); regions only matter to the setters below.
 * Repacks the mesh into the device layout and allocates the operator-owned
 * vectors (boundary values/fluxes/accum, external sources, Manning n,
 * primitive variables), all zero-initialised as in src/operator.c:91-129. */
int rdyhip_create(const RDyHipConfig *config, const RDyHipMesh *mesh, int32_t num_boundaries, const RDyHipBoundary *boundaries,
                  RDyHipOperator *op);

/* DestroyOperator(Operator**)  include/private/rdyoperatorimpl.h:210, src/operator.c:421-493 */
int rdyhip_destroy(RDyHipOperator *op);

/* ---- the hot path -----------------------------------------------------------
 * ApplyOperator(Operator*, PetscReal dt, Vec u_local, Vec f_global)
 *   include/private/rdyoperatorimpl.h:213, src/operator.c:680-690 (-> ApplyPetscOperator 656-672).
 * u_local: device, [num_cells][3] (h,hu,hv), ghosts filled by the caller.
 * f_global: device, [num_owned_cells][3]; the operator ADDS into it exactly as
 * the reference does, and the friction term sees the incoming content through
 * the flux-divergence sum (src/operator.c:663). */
int rdyhip_apply(RDyHipOperator op, double dt, const double *u_local, double *f_global, void *stream);

/* OperatorRHSFunction's "VecZeroEntries(F); ResetOperatorDiagnostics; ApplyOperator"
 *   src/rdysetup.c:1130,1136,1139 -- fused: f_global is overwritten (never read),
 * diagnostics are reset on the stream first.  The halo update of u_local
 * (rdysetup.c:1133-1134) stays with the caller. */
int rdyhip_rhs_function(RDyHipOperator op, double dt, const double *u_local, double *f_global, void *stream);

/* The same as rdyhip_rhs_function restricted to a subset of the owned cells, so
 * that a caller can overlap the halo exchange with the interior cells:
 *   apply_phase(INTERIOR, RDYHIP_PHASE_OVERWRITE | RDYHIP_PHASE_RESET_DIAGNOSTICS) || exchange;
 *   apply_phase(HALO, RDYHIP_PHASE_OVERWRITE).
 * `flags`: RDYHIP_PHASE_OVERWRITE gives rdyhip_rhs_function semantics (f = F(u)),
 * without it rdyhip_apply's (f += F(u)); RDYHIP_PHASE_RESET_DIAGNOSTICS resets the
 * Courant diagnostic first (no extra launch). */
#define RDYHIP_PHASE_OVERWRITE 1
#define RDYHIP_PHASE_RESET_DIAGNOSTICS 2
#define RDYHIP_PHASE_GRADIENTS_READY 4 /* second order: use the gradient field as it is (the caller has run
                                          rdyhip_compute_gradients and filled the ghost rows) */
int rdyhip_apply_phase(RDyHipOperator op, int32_t phase, int32_t flags, double dt, const double *u_local, double *f_global,
                       void *stream);

/* ---- second order (config.second_order) -------------------------------------
 * rdyhip_apply / rdyhip_rhs_function then run ApplyInteriorFlux2R (src/swe/swe_petsc.c:98-213):
 * least-squares gradients of the owned cells, limited reconstruction of both face states of every
 * interior edge, Roe flux on the reconstructed states; boundary edges and sources are unchanged.
 * On one rank nothing else is needed.  With ghost cells the gradients of the ghosts must come from
 * their owners (CommunicateCellGradients) before the fluxes are taken:
 *   [halo update of u_local]
 *   rdyhip_compute_gradients(op, RDYHIP_PHASE_ALL, u_local, stream)     ComputeLeastSquaresGradients, owned cells
 *   [halo update of the RDYHIP_FIELD_GRADIENTS rows, 6 values per cell: rdyhip_pack_rows / rdyhip_unpack_rows]
 *   rdyhip_apply_phase(op, RDYHIP_PHASE_ALL, flags | RDYHIP_PHASE_GRADIENTS_READY, ...)
 * Every rank then evaluates all edges of its owned cells itself (a cut edge on both ranks, from
 * identical operands), so the reference's reverse DMLocalToGlobal(ADD_VALUES) has no counterpart.
 * PHASE_INTERIOR / PHASE_HALO select owned cells without / with a ghost neighbour, for overlap.  With the default
 * fused kernel (RDyHipLayoutInfo.second_order_fused) the gradients of interior cells never leave the chip: only
 * rdyhip_compute_gradients(RDYHIP_PHASE_HALO) is needed to feed the exchange, and the INTERIOR tiles of
 * rdyhip_apply_phase need no data from other ranks at all. */
int rdyhip_compute_gradients(RDyHipOperator op, int32_t phase, const double *u_local, void *stream);

/* ---- operator data (host-side setters, as in the reference) -----------------
 * SetOperatorBoundaryValues(Operator*, RDyBoundary, comp_offset, num_comp, num_edges, values[num_comp*e+c])
 *   include/private/rdyoperatorimpl.h:254, src/operator.c:1045-1061.  `values` is a host pointer. */
int rdyhip_set_boundary_values(RDyHipOperator op, int32_t boundary, int32_t comp_offset, int32_t num_comp, int32_t num_edges,
                               const double *values);

/* ExtractOperatorBoundaryFluxes (include/private/rdyoperatorimpl.h:256): copies
 * boundary_fluxes[b] or boundary_fluxes_accum[b] ([num_edges][3], src/operator.c:124-129) to the host. */
int rdyhip_get_boundary_fluxes(RDyHipOperator op, int32_t boundary, int32_t accumulated, int32_t num_edges, double *fluxes);
int rdyhip_reset_boundary_fluxes_accum(RDyHipOperator op);

/* Get/RestoreOperator{Regional,Domain}ExternalSource (include/private/rdyoperatorimpl.h:258-261,
 *   src/operator.c:1203-1241,1394-1429) as used by RDySet{Regional,Domain}{Water,XMomentum,YMomentum}Source
 *   (src/rdydata.c:225-366): sets component `comp` of the external source of
 *   `n` owned cells; owned_cell_ids == NULL means owned cells 0..n-1 (domain). Host pointers.
 *
 * The water-source plane.  The momentum sources (components 1 and 2) are zero-initialised at create (src/operator.c:91-129)
 * and most runs never set them.  While that is known to hold, the first-order and hydrostatic-reconstruction kernels read the
 * water source from a dense [owned] mirror of component 0 that the library keeps beside the canonical [owned][3] array: 8 B
 * of memory traffic per cell instead of 24.  "Known" means: every write of the source so far went through a call that lets
 * the host see it.
 *   - comp 0, any setter below (this one, _on, rdyhip_forcing_fill_source / _gather_source): written to both arrays.
 *   - comp 1 / 2 with host values (this one, _on) or a host scalar (fill_source): the values are scanned; anything whose
 *     bit pattern is not that of +0.0 (-0.0 and NaN included) ends the mode.  gather_source on comp 1 / 2 ends it unseen.
 *   - rdyhip_refresh_field from a HOST array: momentum entries all +0.0 -> the plane is rewritten and the mode (re)starts;
 *     this is the only way back into it.  Otherwise it ends.  From a DEVICE array: the mode ends (the call must not block,
 *     so the host cannot look).
 *   - rdyhip_field_ptr(RDYHIP_FIELD_EXTERNAL_SOURCES): the caller may write the array in place, so the mode ends for the
 *     life of the operator.  rdyhip_field_ptr_const hands out the same pointer for reading and changes nothing.
 * Outside the mode the kernels read the [owned][3] array as before; the results are the same bits either way, and the
 * [owned][3] array is current at all times.  The mode is read when a launch is enqueued: launches and setters on one stream
 * stay consistent, across streams the caller orders them as for the data.  rdyhip_source_is_water_only reports it.
 *
 * Uniform fields.  A run without rain has a water source of +0.0 in every cell, a storm over a small domain one rate in every
 * cell; Manning's n is one number in most decks; a benchmark bed is often flat.  While every owned element of such a field is
 * known to hold the SAME 64-bit pattern (-0.0 is not +0.0; NaNs are equal if their payloads are), the first-order and
 * hydrostatic-reconstruction kernels read element 0 of it in every lane instead of streaming the plane: 8 B per cell and field
 * less memory traffic (16 B for the two bed slopes).  Element 0 of the array on the device, written on the stream by the same
 * setters as ever, is the value -- no copy of it travels with the launch, nothing can go stale -- and every array stays
 * allocated and current: entering or leaving a mode moves no data, the results are the same bits either way, and every other
 * kernel (second order, cell-centric, ensembles, tracers, output means, read-out) reads the arrays as before.  Per field the
 * host keeps a flag, the pattern and whether the array has escaped:
 *   - At create the source and Manning's n are uniform +0.0 (the arrays are zeroed); the bed is flat if every dz/dx and dz/dy
 *     of the mesh is +0.0, and being static it stays what it is.
 *   - A mode STARTS, or restarts with a new value, on a host write of all owned cells with equal values: this setter or _on
 *     (comp 0 for the source) or rdyhip_set_mannings[_on] with owned_cell_ids == NULL and n = the number of owned cells,
 *     rdyhip_refresh_field from a host array, rdyhip_forcing_fill_source on comp 0 with d_owned_cell_ids == NULL and n = owned
 *     cells.  The scan stops at the first element that differs; an array that is uniform is not uploaded at all but filled on
 *     the device from its one value.
 *   - It is KEPT by a write of some cells (an id list, fewer values) or a fill with a host scalar whose values all equal the
 *     stored pattern.
 *   - It ENDS with any other write of some cells, with a write of unequal values, and with a write whose values the host
 *     cannot see (rdyhip_forcing_gather_source, rdyhip_refresh_field from a device array).
 *   - rdyhip_field_ptr on the external source or on Manning's n ends the field's mode for the life of the operator;
 *     rdyhip_field_ptr_const changes nothing.
 *   - The source's mode is honoured only inside the water-only mode above (element 0 of the plane stands for all cells).
 * The modes are read when a launch is enqueued, like the water-only mode.  rdyhip_uniform_fields reports them;
 * RDYHIP_UNIFORM_FIELDS=0 in the environment of rdyhip_create keeps all of them off (an A/B and test knob). */
int rdyhip_set_external_source(RDyHipOperator op, int32_t comp, int32_t n, const int32_t *owned_cell_ids, const double *values);

/* Get/RestoreOperator{Regional,Domain}MaterialProperties (rdyoperatorimpl.h:263-266)
 *   as used by RDySet{Regional,Domain}ManningsN (src/rdydata.c:506-539). */
int rdyhip_set_mannings(RDyHipOperator op, int32_t n, const int32_t *owned_cell_ids, const double *values);

/* The same three setters ordered on a stream instead of synchronising the device: launches enqueued on `stream` before the
 * call see the old values, launches enqueued on it afterwards the new ones (applies running on OTHER streams are the
 * caller's to order).  `values` / `owned_cell_ids` are host arrays and may be reused as soon as the call returns: they are
 * copied into pinned staging memory of the operator, travel to the device on the operator's own copy stream beside whatever
 * `stream` is executing, and only the last step -- a scatter launch or a device-to-device copy -- is ordered on `stream`.
 * Arrays above 8 MB go in 8-MB chunks, the upload of a chunk beside the host copies of the chunks behind it: with an adaptive
 * time step the caller has just read the Courant struct back, the device is idle and waits for exactly this.
 * Nothing blocks and nothing drains the device: with a fixed time step RDyAdvance needs no synchronisation at all
 * (src/rdyadvance.c:303-305), and a drained device runs its next ~40 launches 20-30 % slow (profiles/r02_launch_series.json).
 * rdyhip_refresh_field replaces a whole input field (RDYHIP_FIELD_EXTERNAL_SOURCES [owned][3], RDYHIP_FIELD_MANNINGS [owned])
 * from a host or a device array -- what an adapter does when a PETSc Vec of the Operator changed (src/operator.c:91-96). */
int rdyhip_set_boundary_values_on(RDyHipOperator op, int32_t boundary, int32_t comp_offset, int32_t num_comp, int32_t num_edges,
                                  const double *values, void *stream);
int rdyhip_set_external_source_on(RDyHipOperator op, int32_t comp, int32_t n, const int32_t *owned_cell_ids, const double *values, void *stream);
int rdyhip_set_mannings_on(RDyHipOperator op, int32_t n, const int32_t *owned_cell_ids, const double *values, void *stream);

/* ---- forcing ingestion on the device -----------------------------------------
 * The per-step fill loops of RDyApplyForcing (src/forcing/rdyforcing.c:688-770)
 * with the dataset, the data->mesh map and the region's cell list resident in
 * HBM: nothing crosses PCIe between RHS evaluations.  All pointers are DEVICE
 * pointers; the calls are enqueued on `stream` and do not synchronise.
 * `d_owned_cell_ids` (the region's owned-cell indices, RDyRegion.owned_cell_ids;
 * NULL = owned cells 0..n-1) must hold valid indices: they cannot be range-checked
 * on the host.  The scalar time lookup (RDyForcingGetCurrentData,
 * src/forcing/rdyforcing_dataset.c:32-67) stays on the host (rdycore_amd/forcing.py).
 *
 * fill_source:     RDyForcingSetConstantRainfall / RDyForcingSetHomogeneousData (rdyforcing_dataset.c:282-288,
 *                  320-344) + RDySetRegionalWaterSource / RDySetHomogeneousRegionalWaterSource (src/rdydata.c:253-309):
 *                  ext[id[i]][comp] = value
 * gather_source:   RDyForcingSetRasterData (rdyforcing_dataset.c:295-314: stride 1, offset = header_offset,
 *                  scale = 1/(1000*3600)) and RDyForcingSetUnstructuredData (350-373: offset 2, scale 1):
 *                  ext[id[i]][comp] = data[data2mesh_idx[i]*stride + offset] * scale
 * fill_boundary:   RDyForcingSetHomogeneousBoundary (380-406) + RDySetFlowDirichletBoundaryValues: bvalues[e] = [h,0,0]
 * gather_boundary: RDyForcingSetUnstructuredData on a boundary dataset (stride 3):
 *                  bvalues[e][c] = data[data2mesh_idx[e]*stride + c + offset]
 * nearest_map:     RDyForcingCreateRasterDatasetMapping (src/forcing/rdyforcing_map.c:111-141; min_dist0 =
 *                  (max(ncols,nrows)+1)*cellsize, entries with no point nearer than that are left untouched) and
 *                  RDyForcingCreateUnstructuredDatasetMap (77-104; pass min_dist0 < 0): brute-force nearest
 *                  data point, first index wins ties. */
int rdyhip_forcing_fill_source(RDyHipOperator op, int32_t comp, int32_t n, const int32_t *d_owned_cell_ids, double value, void *stream);
int rdyhip_forcing_gather_source(RDyHipOperator op, int32_t comp, int32_t n, const int32_t *d_owned_cell_ids, const double *d_data,
                                 const int32_t *d_data2mesh_idx, int64_t stride, int64_t offset, double scale, void *stream);
int rdyhip_forcing_fill_boundary(RDyHipOperator op, int32_t boundary, int32_t num_edges, double h, void *stream);
int rdyhip_forcing_gather_boundary(RDyHipOperator op, int32_t boundary, int32_t num_edges, const double *d_data,
                                   const int32_t *d_data2mesh_idx, int64_t stride, int64_t offset, void *stream);
int rdyhip_forcing_nearest_map(int32_t n, const double *d_xc, const double *d_yc, int32_t ndata, const double *d_data_xc,
                               const double *d_data_yc, double min_dist0, int32_t *d_map, void *stream);

/* In-place access to the device-resident fields (no copy): e.g. a forcing
 * kernel can write the external source on the GPU, an output routine can read
 * primitive_variables (read by src/rdyadvance.c's averaging monitors). */
int rdyhip_field_ptr(RDyHipOperator op, RDyHipField field, double **device_ptr, int64_t *num_values);
/* Primitive variables on demand.  (h, u, v) of a cell are a function of its own state alone, and in the reference only the
 * output monitors read them, when primitive-variable output is configured (src/rdysetup.c:1535).  So the evaluations
 * (rdyhip_apply / _rhs_function / _apply_phase / _euler_step and the _overlapped forms) store them only once somebody can look:
 *   - A pointer obtained through rdyhip_field_ptr or rdyhip_field_ptr_const(RDYHIP_FIELD_PRIMITIVE_VARIABLES) is written by every
 *     evaluation from then on, until rdyhip_field_release: what every evaluation did before this became optional.  A host that
 *     asks once at setup sees no difference.
 *   - A host that never asks pays nothing: 24 B per cell of stores less in every launch.
 *   - The first request after evaluations that did not store fills ALL owned rows from the u_local array of the most recent of
 *     them (for rdyhip_euler_step: its INPUT state), with the arithmetic of the kernels (the same bits a storing launch writes),
 *     enqueued on the stream that evaluation was given.  That array must still exist and still hold that state when the request
 *     is made: in RDycore it does (u_local is rewritten only by the next RHS's DMGlobalToLocal).  The library checks that the
 *     pointer is still device memory of the operator's device and otherwise returns RDYHIP_ERR_USER without launching anything
 *     (storing is on from then on, the next evaluation writes the array); an array that was overwritten, or freed and
 *     allocated again, since cannot be told -- the values are then those of whatever it holds.
 *   - Before any evaluation the array holds the zeros of rdyhip_create.
 * Whether a launch stores is decided when it is enqueued, like the water-only mode of the source.
 *
 * rdyhip_field_release(RDYHIP_FIELD_PRIMITIVE_VARIABLES): the caller will not read through pointers obtained earlier until it
 * asks again; evaluations stop storing and the next request fills.  For a host whose output monitor fires every N steps: ask
 * per output, read, release.  Every other field: RDYHIP_ERR_USER.
 * rdyhip_primitive_variables_stored: *out = 1 while evaluations store them, else 0. */
int rdyhip_field_release(RDyHipOperator op, RDyHipField field);
int rdyhip_primitive_variables_stored(RDyHipOperator op, int32_t *out);
/* The same pointer for readers (output monitors of primitive_variables or the source): nothing is assumed to be written.
 * rdyhip_field_ptr(RDYHIP_FIELD_EXTERNAL_SOURCES) on the other hand hands out a pointer that MAY be written in place, which ends
 * the water-only mode of the source for good (see rdyhip_set_external_source). */
int rdyhip_field_ptr_const(RDyHipOperator op, RDyHipField field, const double **device_ptr, int64_t *num_values);
/* *out = 1 while the kernels read the water source from its own plane (see rdyhip_set_external_source), else 0 */
int rdyhip_source_is_water_only(RDyHipOperator op, int32_t *out);
/* *mask = the RDYHIP_UNIFORM_* bits of the fields whose element 0 the next first-order / HR launch would read for all cells
 * (see "Uniform fields" at rdyhip_set_external_source; the source bit only while the source is water only) */
#define RDYHIP_UNIFORM_SOURCE 1
#define RDYHIP_UNIFORM_MANNINGS 2
#define RDYHIP_UNIFORM_FLAT_BED 4
int rdyhip_uniform_fields(RDyHipOperator op, int32_t *mask);
/* The normal table.  The unit normals of a mesh cut from a raster take a handful of values (axis-parallel sides and the
 * diagonals, in both orientations: six or eight), and the mesh is static for the life of an operator.  rdyhip_create counts
 * the distinct normals of the tile edge records -- bit patterns, -0.0 is not +0.0 -- and, where there are at most 64, keeps
 * them in a table of the operator: the first-order / HR tiled kernels then take each edge's normal from on-chip memory
 * (kernel family swe_rhs_ntab_kernel) instead of streaming 8 B per record (swe_rhs_tiled_kernel).  Same results, bit for bit.
 *   *entries = the size of the table, *active = 1 if the operator's launches use it; (0, 0) for a mesh with more normals
 * or without edge records, under RDYHIP_CONFIG_STREAMED_NORMALS, for second_order and under RDYHIP_KERNEL=cell.  Either
 * pointer may be NULL.  Uses no device memory: rdyhip_device_bytes is what it was. */
int rdyhip_normal_table_info(RDyHipOperator op, int32_t *entries, int32_t *active);
/* A device array of external sources ends the water-only mode of the source: this call does not block, so the host cannot
 * look at the momentum entries (keeping the plane on this path is a follow-up).  A host array keeps or restarts it. */
int rdyhip_refresh_field(RDyHipOperator op, RDyHipField field, const double *values, int64_t num_values, int32_t values_on_device, void *stream);
/* keep Operator.flux_divergence (one extra [owned][3] store per apply); off by default */
int rdyhip_enable_flux_divergence(RDyHipOperator op, int32_t enable);

/* ---- diagnostics ------------------------------------------------------------
 * ResetOperatorDiagnostics / UpdateOperatorDiagnostics / GetOperatorDiagnostics
 *   include/private/rdyoperatorimpl.h:269-271, src/operator.c:772-784,867-893.
 * reset is enqueued on `stream`; update synchronises `stream`, copies the
 * 16-byte result to the host and resolves the edge/cell ids.  The cross-rank
 * MPI_Allreduce of src/operator.c:879 stays with the caller (one struct). */
int rdyhip_reset_diagnostics(RDyHipOperator op, void *stream);
int rdyhip_update_diagnostics(RDyHipOperator op, void *stream);
int rdyhip_get_diagnostics(RDyHipOperator op, RDyHipCourant *courant);

/* ---- diagnostics, non-blocking ----------------------------------------------
 * The read-back of the Courant record(s) in two halves, so that a host with an adaptive time step can prepare the next
 * coupling interval (RDyApplyForcing takes the time only, src/rdyadvance.c:351) beside the device and collect the 16 bytes
 * where it needs dt.  `scope` names whose record is read: RDYHIP_DIAGNOSTICS_OPERATOR is what rdyhip_update_diagnostics
 * reports (the most recent SWE or tracer evaluations), RDYHIP_DIAGNOSTICS_ENSEMBLE what rdyhip_ensemble_update_diagnostics
 * reports (B structs).  The two scopes are independent.
 * rdyhip_diagnostics_begin: enqueues on `stream` the merge launch of the blocking call, a copy of the record(s) into pinned
 *   memory the operator owns, and an event; returns without waiting for anything.  The pinned memory and the event are
 *   allocated by the first begin of a scope: only that call may synchronise.
 * rdyhip_diagnostics_wait: blocks on that event only, resolves the edge and cell ids as the blocking call does and stores the
 *   result where rdyhip_get_diagnostics / rdyhip_ensemble_get_diagnostics read it.
 * rdyhip_diagnostics_ready: *ready = 1 once the copy has landed (an event query; also after the wait), else 0.  It never
 *   stands in for the wait: only the wait delivers the result.
 * Place in the stream: the result is that of begin's place in `stream`.  Evaluations enqueued afterwards, their diagnostics
 *   reset and rdyhip_reset_diagnostics do not change what the wait delivers, and what resolving the ids needs (whether the
 *   numbers are a tracer evaluation's, which a later SWE evaluation would change) is remembered as of begin.  An evaluation
 *   or reset called after the wait resets what the getters return, as always.
 * One read per scope: a begin while an earlier one of the same scope has not been waited for replaces it -- not an error.  The
 *   new launch is first ordered behind the earlier copy (hipStreamWaitEvent), also when the two are on different streams: the
 *   device record is never rewritten under a running copy.
 * Nothing to wait for: a wait with no read in flight -- no begin yet, or a read that was already waited for or discarded -- is
 *   RDYHIP_ERR_USER; so is ready before any begin or after a discard.  Neither call touches an event that was not recorded.
 * The blocking calls keep their behaviour bit for bit.  A read of their scope that is in flight is discarded by them: a later
 *   wait is RDYHIP_ERR_USER, and the blocking call's result stands.
 * rdyhip_destroy waits for a copy still in flight before it frees the pinned memory.
 * A null operator, an unknown scope, or the ensemble scope before rdyhip_ensemble_enable is RDYHIP_ERR_USER before any device
 *   call.  A rank that owns nothing behaves as the blocking calls do there: (0, -1, -1). */
#define RDYHIP_DIAGNOSTICS_OPERATOR 0   /* what rdyhip_update_diagnostics reports: SWE or tracer evaluations */
#define RDYHIP_DIAGNOSTICS_ENSEMBLE 1   /* what rdyhip_ensemble_update_diagnostics reports: B structs */
int rdyhip_diagnostics_begin(RDyHipOperator op, int32_t scope, void *stream);
int rdyhip_diagnostics_ready(RDyHipOperator op, int32_t scope, int32_t *ready);
int rdyhip_diagnostics_wait(RDyHipOperator op, int32_t scope);

/* ---- halo helpers (DMGlobalToLocalBegin/End, src/rdysetup.c:1133-1134) -------
 * pack:   buf[i][0..2] = u_local[cell_ids[i]][0..2]   (cells a neighbour rank needs)
 * unpack: u_local[cell_ids[i]][0..2] = buf[i][0..2]   (this rank's ghost cells)
 * all device pointers; the transport between ranks (RCCL) is the caller's. */
int rdyhip_pack_cells(const double *u_local, const int32_t *cell_ids, int32_t n, double *buf, void *stream);
int rdyhip_unpack_cells(double *u_local, const int32_t *cell_ids, int32_t n, const double *buf, void *stream);
/* the same for rows of `ncomp` values (the [num_cells][6] gradient field): buf[i][:] = src[ids[i]][:] and back */
int rdyhip_pack_rows(const double *src, int32_t ncomp, const int32_t *row_ids, int32_t n, double *buf, void *stream);
int rdyhip_unpack_rows(double *dst, int32_t ncomp, const int32_t *row_ids, int32_t n, const double *buf, void *stream);

/* ---- the ghost update and its overlap with the interior cells, behind the ABI ----
 * OperatorRHSFunction's DMGlobalToLocalBegin/End (src/rdysetup.c:1133-1134) for a C host: the operator packs the owned
 * cells its neighbours need, exchanges them and unpacks into its ghost cells on an internal stream, while
 * the cells without ghost neighbours are evaluated on the caller's stream; the ghost-adjacent cells follow.
 *
 *   rdyhip_halo_create   the exchange pattern of this rank: for each of `npeers` neighbour ranks, the LOCAL ids of the
 *                        owned cells it needs from this rank (send lists) and of this rank's ghost cells it owns (receive
 *                        lists), in an order both sides agree on (e.g. ascending global id), concatenated in peer order.
 *                        `nccl_comm`: an RCCL communicator (ncclComm_t passed as void*) spanning the operator's ranks, or
 *                        NULL if the bytes travel through rdyhip_halo_set_transport.  With RCCL one exchange is
 *                        ncclGroupStart(); ncclSend / ncclRecv per peer; ncclGroupEnd() over xGMI -- point-to-point, no collective.
 *   rdyhip_halo_set_transport  replaces RCCL by the caller's transport (GPU-aware MPI_Isend/Irecv in an MPI code, a
 *                        host-staged exchange in the single-GPU tests): called once per exchange, after the send buffer has
 *                        been packed on `stream`, it must deliver d_send's per-peer slices into the peers' d_recv slices
 *                        ([cells][ncomp] doubles, peer order as at create) so that work enqueued on `stream` afterwards sees
 *                        d_recv filled; it may block the host (the interior launch is already enqueued by then).
 *   rdyhip_halo_exchange the plain ghost update of a [num_cells][ncomp] array (ncomp = 3: the solution; 6: the
 *                        second-order gradients, CommunicateCellGradients), all on `stream`
 *   rdyhip_rhs_overlapped        = halo update of u_local + rdyhip_rhs_function, overlapped (the whole OperatorRHSFunction)
 *   rdyhip_euler_step_overlapped = halo update of u_local + rdyhip_euler_step(PHASE_ALL), overlapped
 * The tiles that need ghost data follow the unpack on the library's stream, beside the tail of the other tiles.
 * Second order: the state exchange hides behind the tiles that need no ghost data, then the ghost-adjacent gradients are
 * computed, exchanged (6 values per cell) and the remaining tiles follow.  The exchanges are ordered after everything
 * already enqueued on `stream`; when the call returns all work is enqueued and later work on `stream` is ordered after it.
 * The form of a step -- everything in order on `stream`: exchange, (gradients, their exchange,) ONE launch over all tiles; or
 * on two streams as described above -- is chosen per halo and per kind of step by a TRIAL on the communicator the halo really
 * has: the first 16 calls alternate between the forms, each timed on the device, and the faster one stays (both forms post
 * the same send / receive group, so every rank chooses for itself).  A small part wants the first form (its interior tiles
 * run for less time than the exchange chain, and the two cross-stream dependencies cost more than they hide), a large one
 * behind a slow link the second.  rdyhip_halo_form_info() reports the choice and the two timings, rdyhip_halo_set_form()
 * forces a form or restarts the trial; RDYHIP_OVERLAP=0 / 1 and RDYHIP_OVERLAP_MIN_ROUNDS=n (the size rule of earlier
 * versions), read once at rdyhip_halo_create, force as well.  rdyhip_halo_overlaps() = the RHS step currently runs on two streams.
 *
 * Two ways to shorten the exchange chain of a small part (a 0.36 M-cell rank's kernel runs 17 us; a pack and an unpack launch
 * cost 3.5 us each):
 *   direct receive   when the ghost cells this rank receives are one run of consecutive local rows in arrival order -- peer
 *                    by peer, a peer's cells in the agreed order, which is how rdyhip_local_cell_order numbers them -- the
 *                    transfer lands in the caller's array itself (ncclRecv into u_local's ghost rows): no receive buffer, no
 *                    unpack launch.  Detected at rdyhip_halo_create; rdyhip_halo_direct_receive() says whether it applies.
 *   fused pack       rdyhip_halo_fuse_pack(halo, 1): the Euler-step kernels (first order, HR and fused second order) also store the new state of
 *                    the cells other ranks need into the send buffer as they store u_local_out, so that the NEXT
 *                    rdyhip_euler_step_overlapped, called with that array as its u_local, starts with the transfer: no pack
 *                    launch.  The promise the caller makes: between two such steps it does not write the owned rows of that
 *                    array itself -- or calls rdyhip_halo_invalidate() if it did (a host that sets the state, a restart).  A
 *                    step whose u_local is any other array packs as before.  One halo per operator can hold the fused pack.
 *                    Second order (fused form): the gradient launch over the ghost-adjacent cells then also stores each gradient
 *                    into the send rows it travels in, so the gradient exchange of rdyhip_rhs_overlapped /
 *                    rdyhip_euler_step_overlapped needs no pack launch either (RDYHIP_GRAD_PACK_FUSED=0: measurement knob).
 * With both, a step of rdyhip_euler_step_overlapped is the transfer and ONE kernel launch.
 * (A fused pack whose send lists hold a cell in a tile no ghost touches -- possible when the DM's overlap is vertex-adjacent,
 * src/rdydm.c:150 -- is only safe when nothing runs beside the transfer: such a halo keeps its Euler steps in order,
 * rdyhip_halo_form_info says RDYHIP_HALO_FORM_LOCKED_IN_ORDER.) */
typedef struct RDyHipHalo_s *RDyHipHalo;
typedef int (*RDyHipTransportFn)(void *ctx, const double *d_send, double *d_recv, int32_t ncomp, void *stream);
int rdyhip_halo_create(RDyHipOperator op, void *nccl_comm, int32_t npeers, const int32_t *peers, const int32_t *send_counts,
                       const int32_t *send_cell_ids, const int32_t *recv_counts, const int32_t *recv_cell_ids, RDyHipHalo *halo);
int rdyhip_halo_destroy(RDyHipHalo *halo);
int32_t rdyhip_halo_overlaps(RDyHipHalo halo);
int32_t rdyhip_halo_direct_receive(RDyHipHalo halo);
int rdyhip_halo_fuse_pack(RDyHipHalo halo, int32_t enable);
int32_t rdyhip_halo_pack_fused(RDyHipHalo halo);
/* which form the steps of a halo take and why (see above); kind: RDYHIP_HALO_STEP_RHS = rdyhip_rhs_overlapped,
 * RDYHIP_HALO_STEP_EULER = rdyhip_euler_step_overlapped, RDYHIP_HALO_STEP_TRACERS_RHS = rdyhip_halo_tracers_rhs,
 * RDYHIP_HALO_STEP_TRACERS_EULER = rdyhip_halo_tracers_euler_step (each kind has a trial and a choice of its own).  The two
 * tracer kinds stay in order -- rdyhip_halo_set_form leaves them at form 0, rdyhip_halo_form_info says
 * RDYHIP_HALO_FORM_LOCKED_IN_ORDER -- on a halo whose pattern receives into owned rows and on a halo without peers. */
#define RDYHIP_HALO_STEP_RHS 0
#define RDYHIP_HALO_STEP_EULER 1
#define RDYHIP_HALO_STEP_TRACERS_RHS 2
#define RDYHIP_HALO_STEP_TRACERS_EULER 3
#define RDYHIP_HALO_FORM_TRIAL_RUNNING 0   /* the first calls still alternate */
#define RDYHIP_HALO_FORM_MEASURED 1        /* the faster form of the trial */
#define RDYHIP_HALO_FORM_FORCED 2          /* environment or rdyhip_halo_set_form */
#define RDYHIP_HALO_FORM_DEFAULT 3         /* nothing to choose (no peers) or no timing available: in order */
#define RDYHIP_HALO_FORM_LOCKED_IN_ORDER 4 /* fused pack with a send cell outside the ghost-adjacent tiles; tracer kinds: see above */
typedef struct {
  int32_t form;           /* 0: in order on the caller's stream, 1: two streams */
  int32_t source;         /* RDYHIP_HALO_FORM_* */
  int32_t trial_steps;    /* calls the trial has used so far (16 when done) */
  double  in_order_ms;    /* mean device time per step of each form in the trial (0 until it is over) */
  double  two_stream_ms;
} RDyHipHaloFormInfo;
int rdyhip_halo_form_info(RDyHipHalo halo, int32_t kind, RDyHipHaloFormInfo *info);
int rdyhip_halo_set_form(RDyHipHalo halo, int32_t kind, int32_t form /* 0, 1, or < 0: run the trial again */);
int rdyhip_halo_invalidate(RDyHipHalo halo);
int rdyhip_halo_set_transport(RDyHipHalo halo, RDyHipTransportFn fn, void *ctx);
int rdyhip_halo_exchange(RDyHipHalo halo, double *rows, int32_t ncomp, void *stream);
int rdyhip_rhs_overlapped(RDyHipOperator op, RDyHipHalo halo, double dt, double *u_local, double *f_global, void *stream);
int rdyhip_euler_step_overlapped(RDyHipOperator op, RDyHipHalo halo, double dt, double *u_local, double *u_local_out, double *f_global,
                                 void *stream);
/* RCCL communicator helpers, so that a host needs no RCCL binding of its own: rank 0 calls rdyhip_comm_unique_id and
 * broadcasts the 128 bytes (MPI_Bcast in RDycore), then every rank calls rdyhip_comm_init_rank (ncclCommInitRank on the
 * current device; collective over the ranks). */
#define RDYHIP_COMM_ID_BYTES 128
int rdyhip_comm_unique_id(char id[RDYHIP_COMM_ID_BYTES]);
int rdyhip_comm_init_rank(int32_t nranks, int32_t rank, const char id[RDYHIP_COMM_ID_BYTES], void **nccl_comm);
int rdyhip_comm_destroy(void *nccl_comm);
int rdyhip_comm_count(void *nccl_comm, int32_t *nranks);   /* ncclCommCount: how many ranks the communicator really spans */
int32_t rdyhip_rccl_version(void);

/* ---- planning the exchange and the local numbering (host only: no device is touched, testable without a GPU) ----
 * What the DM's point SF knows (PetscSFGetGraph on DMGetPointSF(dm): for every ghost cell its owner rank and the owner's
 * index for it; the 1-cell overlap of src/rdydm.c:145-157) turned into rdyhip_halo_create's arguments.  The send side is the
 * transpose of the receive side, which needs ONE all-to-all; the library leaves that to the caller's own communicator:
 *
 *   rdyhip_halo_plan_create(world, rank, num_ghosts, ghost_cell_ids, ghost_owner_ranks, ghost_keys, &plan)
 *        ghost_cell_ids[i]    local id of my i-th ghost cell
 *        ghost_owner_ranks[i] the rank that owns it (iremote[i].rank)
 *        ghost_keys[i]        the OWNER's name for it: its local cell id there (iremote[i].index - cStart), or a global
 *                             cell id -- whichever rdyhip_halo_plan_finish is told the owner's cells are keyed by
 *   rdyhip_halo_plan_requests(plan, &counts, &keys)
 *        counts[r] = number of cells I need from rank r; keys = their keys grouped by r, ascending inside a group (the
 *        order both sides use).  Caller: MPI_Alltoall(counts -> incoming_counts), MPI_Alltoallv(keys -> incoming_keys).
 *   rdyhip_halo_plan_finish(plan, incoming_counts, incoming_keys, num_cells, cell_is_owned, cell_keys)
 *        resolves what the others ask of me to my local cells: cell_keys == NULL: a key IS my local cell id; else
 *        cell_keys[c] is the key of local cell c (e.g. cells.global_ids).  Every request must name a cell I own.
 *   rdyhip_halo_plan_get(plan, &npeers, &peers, &send_counts, &send_cell_ids, &recv_counts, &recv_cell_ids)
 *        exactly the arguments of rdyhip_halo_create (pointers valid until rdyhip_halo_plan_destroy).
 *
 *   rdyhip_hilbert_cell_order(num_cells, xy, stride, cell_is_owned, perm): perm[new] = old local cell id, owned cells first
 *        (so that they are a prefix: the owned rows of a local Vec are then one block), each group along a Hilbert curve
 *        through the centroids xy[c*stride + 0..1].  The tiles of the operator are runs of 256 consecutive owned cells, so
 *        this is the numbering a host should give its local cells before it builds RDyMesh (DMPlexPermute; DESIGN.md
 *        section 7 note 7 has the measurements: row-major -18 %, random order 3x slower than a curve order).
 *   rdyhip_local_cell_order(..., cell_owner_rank, cell_keys, perm): the same for the owned cells; the GHOST cells are grouped by
 *        owner rank (cell_owner_rank[c], read for ghosts only) and sorted by cell_keys[c] inside a group -- the key the plan is
 *        given for them (a global cell id; or the owner's local id, which is known once the owners have renumbered: a second
 *        pass over the ghosts only).  rdyhip_halo_plan_* then lists every peer's ghosts as consecutive rows in arrival order,
 *        and rdyhip_halo_create receives in place (direct receive, above).
 *   rdyhip_copy_owned_rows(op, u_global, u_local, stream): u_local[owned cell o] = u_global[o] -- the local half of
 *        DMGlobalToLocal (device pointers; one contiguous copy when the owned cells are numbered first) */
typedef struct RDyHipHaloPlan_s *RDyHipHaloPlan;
int rdyhip_halo_plan_create(int32_t world, int32_t rank, int32_t num_ghosts, const int32_t *ghost_cell_ids, const int32_t *ghost_owner_ranks,
                            const int64_t *ghost_keys, RDyHipHaloPlan *plan);
int rdyhip_halo_plan_requests(RDyHipHaloPlan plan, const int32_t **request_counts, const int64_t **request_keys);
int rdyhip_halo_plan_finish(RDyHipHaloPlan plan, const int32_t *incoming_counts, const int64_t *incoming_keys, int32_t num_cells,
                            const int32_t *cell_is_owned, const int64_t *cell_keys);
int rdyhip_halo_plan_get(RDyHipHaloPlan plan, int32_t *npeers, const int32_t **peers, const int32_t **send_counts, const int32_t **send_cell_ids,
                         const int32_t **recv_counts, const int32_t **recv_cell_ids);
int rdyhip_halo_plan_destroy(RDyHipHaloPlan *plan);
int rdyhip_hilbert_cell_order(int32_t num_cells, const double *xy, int32_t stride, const int32_t *cell_is_owned, int32_t *perm);
int rdyhip_local_cell_order(int32_t num_cells, const double *xy, int32_t stride, const int32_t *cell_is_owned, const int32_t *cell_owner_rank,
                            const int64_t *cell_keys, int32_t *perm);
int rdyhip_copy_owned_rows(RDyHipOperator op, const double *u_global, double *u_local, void *stream);

/* ---- explicit update kept on the device (what TSEULER does between RHS calls)
 * u_local[owned cell o] += dt * f_global[o]   (PETSc TSStep_Euler VecAXPY; the
 * scatter from the global to the local vector is folded in). */
int rdyhip_axpy_owned(RDyHipOperator op, double dt, const double *f_global, double *u_local, void *stream);

/* The whole forward-Euler step in one pass (TSStep_Euler: F = RHS(U); U += dt F, with OperatorRHSFunction's zeroing
 * of F, src/rdysetup.c:1120-1172): u_local_out[owned cell] = u_local[owned cell] + dt * F, where F is what
 * rdyhip_rhs_function would produce.  Not in place: the caller ping-pongs two local state arrays (the ghost rows of
 * u_local_out are left for the next halo update).  f_global may be NULL -- the first-order and HR tiled kernels then
 * never write F (one 24 B/cell stream less and no separate axpy pass); primitive_variables, boundary fluxes and the
 * Courant diagnostic are produced as by any RHS evaluation.  `phase` / `flags` as in rdyhip_apply_phase
 * (RDYHIP_PHASE_OVERWRITE is implied). */
int rdyhip_euler_step(RDyHipOperator op, int32_t phase, int32_t flags, double dt, const double *u_local, double *u_local_out, double *f_global,
                      void *stream);

/* One classical Runge-Kutta step behind one call: TSStep_RK with the TSRK4 tableau (the reference's `numerics.temporal:
 * rk4`, src/rdysetup.c:1187-1189; A = [[0], [1/2], [0, 1/2], [0, 0, 1]], b = [1/6, 1/3, 1/3, 1/6]).  u_local[owned cell]
 * advances by dt; the four stage vectors and the stage state stay on the device, in a workspace the operator owns.
 *   - Four stage evaluations, each what rdyhip_rhs_function does (halo NULL, or a halo without peers) or, with a halo,
 *     what rdyhip_rhs_overlapped does: its ghost update, the form the halo has chosen for RHS-kind steps (a stage counts as
 *     one such step in the halo's trial), the diagnostics reset.  Stage 1 runs on u_local itself (its ghost rows are
 *     updated as by any rdyhip_rhs_overlapped); every stage gets the FULL step's dt in the friction term (TSGetTimeStep,
 *     src/rdysetup.c:1129).  What is left behind -- Courant struct, boundary fluxes, primitive variables -- is stage 4's.
 *   - Between them one launch per stage state (y = u + c k on the owned rows: c = dt/2, dt/2, dt) and one at the end
 *     (u += dt/6 k1 + dt/3 k2 + dt/3 k3 + dt/6 k4, as a chain of fused multiply-adds in that order): the bits of
 *     rdyhip_axpy_owned applied stage by stage, in 8 launches and 360 B per cell instead of 14 and 648.
 *   - Ghost rows of the stage state that no exchange writes (halo NULL, or receive lists that leave some out) hold
 *     u_local's values.
 *   - Workspace: [num_cells][3] + 4 x [num_owned_cells][3] doubles, allocated by the FIRST call -- that one call may
 *     synchronise the device; no later one does -- counted in RDyHipLayoutInfo.device_bytes from then on and freed by
 *     rdyhip_destroy.
 *   - The owned rows of u_local are rewritten: a fused pack (rdyhip_halo_fuse_pack) of `halo`, or of whichever halo of this
 *     operator holds it, is invalidated as by rdyhip_halo_invalidate, so a later rdyhip_euler_step_overlapped on the same
 *     array packs again.
 *   - "The u_local of the most recent evaluation" (rdyhip_field_ptr, primitive variables on demand) is the operator's own
 *     stage state after this call: it outlives the call, a first request is filled from stage 4's state.
 * RDYHIP_ERR_USER before any device call: null op, null u_local on a rank with cells (owned or ghost), a halo of another operator.  A rank that
 * owns nothing still takes part in the four exchanges. */
int rdyhip_rk4_step(RDyHipOperator op, RDyHipHalo halo /* may be NULL */, double dt, double *u_local, void *stream);

/* ---- time-averaged output fields -----------------------------------------------
 * WriteXDMFOutput's three OutputVars (src/xdmf_output.c:436-504) -- the solution, the primitive variables
 * (op->primitive_variables, src/rdysetup.c:1535-1542) and the sources (op->src_inst, the copy of the external sources that
 * ApplyPetscOperator takes, src/operator.c:668-669) -- accumulated on the device:
 *   rdyhip_output_mean_accumulate  AccumulateOutputVar (196-206): accumulated_time += dt; VecAXPY(accum, dt, inst), once per step
 *   rdyhip_output_mean_get         ComputeMean (211-230): mean = accum * (1 / accumulated_time), at an output
 *   rdyhip_output_mean_reset       ResetOutputVar (233-241): accum = 0, accumulated_time = 0
 * `vars` is a mask of RDYHIP_OUTPUT_*; every variable has its own [num_owned_cells][3] accumulator and its own time.
 *   - _enable allocates a zeroed accumulator for each named variable that has none yet (an existing one keeps its content);
 *     the bytes are counted in RDyHipLayoutInfo.device_bytes and freed by rdyhip_destroy.  The only call of the five that
 *     may synchronise the device.
 *   - _accumulate enqueues ONE launch on `stream` for all of `vars` and adds dt to the host-side time of each:
 *       solution             u_local, device, [num_cells][3]: the state to average; needed only with RDYHIP_OUTPUT_SOLUTION.
 *       primitive variables  those of "the u_local of the most recent evaluation" as defined for rdyhip_field_ptr (for
 *                            rdyhip_euler_step its INPUT state, after rdyhip_rk4_step the operator's stage state; before any
 *                            evaluation the zeros of rdyhip_create).  While the evaluations do not store them they are formed
 *                            in the launch from that array, with the arithmetic of the kernels (the same bits a storing launch
 *                            writes), so the array must still hold that state and work that wrote it must be ordered before
 *                            `stream`'s; a pointer the runtime no longer knows as memory of the operator's device gives
 *                            RDYHIP_ERR_USER, nothing is launched and no time is added.  While they are stored (a pointer is
 *                            out) the stored rows are read -- whatever they hold: after a rdyhip_field_ptr that itself failed
 *                            with "the state array of the last evaluation is gone", they are those of the last storing
 *                            evaluation until the next evaluation writes them, and this call sums them without complaint.  Either way the call leaves the storing as it is: a host that
 *                            never takes the pointer keeps its evaluations free of the 24 B/cell store.
 *       sources              the operator's own [owned][3] array, read at the call's place in `stream` -- NOT at the
 *                            evaluation, where the reference takes its snapshot.  A host that changes the forcing between the
 *                            evaluation and the accumulate orders the two itself.  The water-only mode of the source
 *                            (rdyhip_set_external_source) is neither needed nor ended.
 *     A variable that is not enabled: RDYHIP_ERR_USER, no time changes.  A rank that owns nothing: the times advance, nothing
 *     is launched.  The sums are fused multiply-adds, the bits of rdyhip_axpy_owned(dt, inst, accum).
 *   - _get writes the mean of exactly one variable into d_mean (device, [num_owned_cells][3]) on `stream` and reports the
 *     accumulated time through `accumulated_time` if that is not NULL; it resets nothing.  No accumulated time:
 *     RDYHIP_ERR_USER, as the PetscCheck of ComputeMean (213).
 *   - _reset zeroes the named accumulators on `stream` and their times; _time reports the time of one variable.
 * Every argument error (null operator, unknown bits, a null array where one is needed) is reported before any device call. */
#define RDYHIP_OUTPUT_SOLUTION 1
#define RDYHIP_OUTPUT_PRIMITIVE_VARIABLES 2
#define RDYHIP_OUTPUT_SOURCES 4
int rdyhip_output_mean_enable(RDyHipOperator op, int32_t vars);
int rdyhip_output_mean_accumulate(RDyHipOperator op, int32_t vars, double dt, const double *u_local, void *stream);
int rdyhip_output_mean_get(RDyHipOperator op, int32_t var, double *d_mean, double *accumulated_time, void *stream);
int rdyhip_output_mean_reset(RDyHipOperator op, int32_t vars, void *stream);
int rdyhip_output_mean_time(RDyHipOperator op, int32_t var, double *accumulated_time);

/* ---- time series on the device --------------------------------------------------
 * WriteTimeSeries, the TS monitor of src/time_series.c:530-564, as launches on the caller's stream that append to a log in
 * device memory; the host reads the log when it writes its file (once per coupling interval, or at the end), so keeping a
 * series costs the step loop no synchronisation.  Two series, named by `kind` (exactly one per call):
 *   RDYHIP_SERIES_BOUNDARY_FLUXES  RecordBoundaryFluxes (270-296) + WriteBoundaryFluxes (298-335) +
 *                                  ResetAccumulatedBoundaryFluxes (508-527).  A record holds one row per boundary edge of the
 *                                  listed boundaries whose left cell is owned -- boundaries in ascending index, a boundary's
 *                                  edges in edge_ids order, as the reference's loops -- with (edge length * accumulated
 *                                  flux) / accumulated time for the 3 components: a product, then a division, the
 *                                  reference's two roundings (287-289, 325-327).  An accumulated time of exactly 0 divides by
 *                                  1 (311-313).  A NaN accumulator (an edge dry on both sides) is a NaN in the record.  The
 *                                  same launch stores +0.0 into the accumulators of EVERY boundary edge, the unlisted
 *                                  boundaries and the edges behind ghost cells included (520-523).
 *   RDYHIP_SERIES_OBSERVATIONS     InitObservations (165-250) + WriteObservations (395-448) with the VecCopy at 541: a record
 *                                  holds the 3 components of the state in every site's cell.
 *   - rdyhip_series_observations_enable / rdyhip_series_boundary_fluxes_enable (InitTimeSeries, 253-266) allocate the log --
 *     `capacity` records of entries x 3 doubles, entries = the number of sites S or of recorded edges E -- and upload the
 *     site / row / edge-length tables; the bytes are counted in RDyHipLayoutInfo.device_bytes and freed by rdyhip_destroy.
 *     Apart from rdyhip_series_read the only calls here that may synchronise.  A second enable of the same kind:
 *     RDYHIP_ERR_USER.  Sites are owned-cell indices (each range-checked on the host, mapped to the local cell where the owned
 *     cells are not numbered first); a site may repeat.  `boundaries`: the indices of the listed boundaries (what the reference
 *     calls not auto-generated), NULL: every boundary; a boundary named twice counts once.  num_sites == 0, or E == 0 (a rank
 *     without an owned boundary edge, an empty list), is valid: records then hold nothing and nothing is launched -- so with
 *     E == 0 the accumulators, which no record of this rank reads, stay as they are -- but the times and counts advance.
 *   - rdyhip_series_boundary_edges: the recorded edges in record order, their local edge ids and their boundaries (pointers valid
 *     until rdyhip_destroy): what a host needs for the metadata columns of its file, edge centroid, normal and condition type
 *     (InitBoundaryFluxes).  rdyhip_series_plan_boundary_edges: the same plan from the mesh arrays alone -- no device, no
 *     operator; the two output arrays need room for the edges of the listed boundaries and may be NULL (only the count).
 *   - rdyhip_series_boundary_fluxes_add_time: AccumulateBoundaryFluxes (464-468), accumulated_time += dt.  Host-side only.  The
 *     accumulation of dt x flux itself happens in the evaluations (the step's own dt), as in the reference's PETSc path (500).
 *   - rdyhip_series_record enqueues ONE launch on `stream` and appends `time` to a host-side list.  u_local (device,
 *     [num_cells][3]) is needed only for observations.  For boundary fluxes the call also sets the accumulated time back to 0,
 *     and it must be ordered after the evaluations whose fluxes it records: launching on their stream does that.  A full log:
 *     RDYHIP_ERR_USER, nothing is launched and neither the accumulators nor the accumulated time change.  A series that is not
 *     enabled: RDYHIP_ERR_USER.
 *   - rdyhip_series_info: rows of a record, records in the log, capacity, and the accumulated time (boundary fluxes; 0 for
 *     observations); any output may be NULL.
 *   - rdyhip_series_read copies records [first, first + count) ([count][entries][3]) and their times to the host and synchronises
 *     `stream` for that: the only blocking call.  rdyhip_series_device_log hands out the device pointer of the whole log
 *     ([capacity][entries][3]) for a view without a copy; reads of it are the caller's to order.
 *   - rdyhip_series_clear sets the number of records to 0; the accumulated time of the boundary series is untouched.
 * Runge-Kutta: every stage evaluation of rdyhip_rk4_step adds its dt x flux to the accumulators, as every RHS evaluation of the
 * reference's PETSc path does (TSRK calls OperatorRHSFunction four times); a record reports what is there.
 * Every argument error (null operator, unknown kind, a null array where one is needed, a negative count or capacity, a boundary
 * index or a site out of range) is RDYHIP_ERR_USER and is reported before any device call. */
#define RDYHIP_SERIES_OBSERVATIONS 1
#define RDYHIP_SERIES_BOUNDARY_FLUXES 2
int rdyhip_series_observations_enable(RDyHipOperator op, int32_t num_sites, const int32_t *owned_cell_ids /* host */, int32_t capacity);
int rdyhip_series_boundary_fluxes_enable(RDyHipOperator op, int32_t num_listed, const int32_t *boundaries /* host; NULL: all */, int32_t capacity);
int rdyhip_series_boundary_edges(RDyHipOperator op, int32_t *num_edges, const int32_t **local_edge_ids, const int32_t **boundary_of_edge);
int rdyhip_series_plan_boundary_edges(const RDyHipMesh *mesh, int32_t num_boundaries, const RDyHipBoundary *boundaries, int32_t num_listed,
                                      const int32_t *listed, int32_t *num_edges, int32_t *local_edge_ids, int32_t *boundary_of_edge);
int rdyhip_series_boundary_fluxes_add_time(RDyHipOperator op, double dt);
int rdyhip_series_record(RDyHipOperator op, int32_t kind, double time, const double *u_local, void *stream);
int rdyhip_series_info(RDyHipOperator op, int32_t kind, int32_t *entries, int32_t *count, int32_t *capacity, double *accumulated_time);
int rdyhip_series_read(RDyHipOperator op, int32_t kind, int32_t first, int32_t count, double *times, double *values /* host */, void *stream);
int rdyhip_series_device_log(RDyHipOperator op, int32_t kind, const double **d_log);
int rdyhip_series_clear(RDyHipOperator op, int32_t kind);

/* ---- state read-out: owned-cell getters and error sums -----------------------------
 * RDyGetOwnedCellHeights / XMomenta / YMomenta (src/rdydata.c:171-205) and the rank-local loops of RDyMMSComputeErrorNorms
 * (src/rdymms.c:869-880) without the blocking copy of the whole [num_cells][3] state that VecGetArrayRead makes of a Vec placed
 * on a device array: a de-interleave launch picks the wanted components on the device, 8 bytes per cell and component cross to
 * the host on the operator's copy stream, and only the call that hands the values over waits -- for that copy alone, not for
 * the device.  `comps` is a mask of RDYHIP_COMPONENT_*; `comp` is exactly one of them.
 *   - rdyhip_state_planes, the device form: ONE launch on `stream`, nothing else.
 *       d_planes[k][o] = u_local[loc(o)][c_k]      k over the set bits c_k of `comps`, ascending; o over the owned cells
 *     d_planes is device memory, [popcount(comps)][num_owned_cells]; u_local is [num_cells][3]; loc(o) is the local cell of owned
 *     cell o (o itself where the owned cells are numbered first).  Values are copied, never computed: every bit pattern
 *     survives (-0.0, NaN payloads, denormals).
 *   - rdyhip_state_read_begin, the host form: the same launch on `stream` into planes the operator owns, an event, a
 *     device-to-host copy into pinned memory the operator owns on the operator's copy stream behind that event (the stream of
 *     the rdyhip_set_*_on setters), and a second event.  It returns without blocking; nothing waits on the host and `stream`
 *     does not wait for the copy.  u_local is read at the call's place in `stream`: work enqueued later on that stream may
 *     overwrite it, rdyhip_rk4_step (which rewrites it in place) included.  The buffers are allocated by the first call that
 *     needs them and grow only (a wider mask later grows them); that one call may synchronise.  The device planes are counted
 *     in RDyHipLayoutInfo.device_bytes; rdyhip_destroy frees everything after waiting for a copy still in flight.
 *     A begin while an earlier read has not landed (not waited for): the new launch is ordered behind the earlier copy, so the
 *     device planes are never overwritten under a running copy, and the earlier result is discarded.  This is not an error.
 *   - rdyhip_state_read_ready: *ready = 1 once the copy has finished (an event query; it does not stand in for _wait).
 *   - rdyhip_state_read_wait blocks until the copy of the last begin has finished -- on its event only.  The only blocking call.
 *   - rdyhip_state_read_get copies one plane from pinned memory to `values` (host, [size]).  size != num_owned_cells:
 *     RDYHIP_ERR_ARG_SIZ (CheckNumOwnedCells, src/rdydata.c:54-58).  A component the last begin did not ask for, no begin at all,
 *     or a read that has not been waited for: RDYHIP_ERR_USER.  It never blocks.
 *   - rdyhip_state_read_ptr hands out the pinned plane itself (NULL on a rank that owns nothing), valid until the next begin.
 *   A rank that owns nothing: nothing is launched or copied; _wait and _get (size == 0) succeed.
 *
 * rdyhip_error_sums: for e = u_local[loc(o)][c] - d_exact[o][c] (one subtraction, as the VecAYPX at src/rdymms.c:857; d_exact is
 * device memory, [num_owned_cells][3], NULL = zeros) over the owned cells o of THIS rank,
 *     l1[c] += |e| * area(o)     l2_squared[c] += e * e * area(o)     linf[c] = max(|e|, linf[c])     area += area(o)
 * The MPI_Allreduce over the ranks and the square root of the L2 sums (src/rdymms.c:885-891) stay with the caller.  With
 * d_exact == NULL and h >= 0, l1[0] is the water volume of the rank.  Two launches on `stream` -- RDYHIP_ERROR_SUMS_BLOCK lanes
 * per workgroup, min(ceil(num_owned_cells / RDYHIP_ERROR_SUMS_BLOCK), RDYHIP_ERROR_SUMS_MAX_WORKGROUPS) workgroups that each
 * write one partial record of 10 doubles, then one workgroup that sums the records in a fixed order -- and an 80-byte copy into
 * pinned memory behind an event; the call does not block.  No floating-point atomics: the result is the same bits from run to
 * run and from stream to stream.  The sums are fused multiply-adds (|e| * area and (e * e) * area enter unrounded).  A NaN in e
 * makes l1 and l2_squared of its component NaN; linf with a NaN input is unspecified (the reference's PetscMax is
 * order-dependent there).  The cell areas [num_owned_cells] and the records [workgroups + 1][10] (the last one is the result) go
 * to the device at the first call, which may synchronise, and are counted in RDyHipLayoutInfo.device_bytes.  A call while an
 * earlier one is still running is ordered behind it and replaces its result.  A rank that owns nothing: all zeros, nothing
 * is launched.
 *   - rdyhip_error_sums_get waits for the result of the last call (its event only) and copies it out: the only blocking call.
 *     No call before it: RDYHIP_ERR_USER.
 * Every argument error (a null operator, a null array where one is needed, `comps` outside 1..7, a `comp` that is not one bit)
 * is RDYHIP_ERR_USER and is reported before any device call. */
#define RDYHIP_COMPONENT_H 1
#define RDYHIP_COMPONENT_HU 2
#define RDYHIP_COMPONENT_HV 4
#define RDYHIP_ERROR_SUMS_BLOCK 256
#define RDYHIP_ERROR_SUMS_MAX_WORKGROUPS 1024
typedef struct {
  double l1[3], l2_squared[3], linf[3], area;
} RDyHipErrorSums;
int rdyhip_state_planes(RDyHipOperator op, int32_t comps, const double *u_local, double *d_planes, void *stream);
int rdyhip_state_read_begin(RDyHipOperator op, int32_t comps, const double *u_local, void *stream);
int rdyhip_state_read_ready(RDyHipOperator op, int32_t *ready);
int rdyhip_state_read_wait(RDyHipOperator op);
int rdyhip_state_read_get(RDyHipOperator op, int32_t comp, int32_t size, double *values /* host */);
int rdyhip_state_read_ptr(RDyHipOperator op, int32_t comp, const double **pinned_values);
int rdyhip_error_sums(RDyHipOperator op, const double *u_local, const double *d_exact, void *stream);
int rdyhip_error_sums_get(RDyHipOperator op, RDyHipErrorSums *out);

/* ---- shallow water with advected tracers ------------------------------------------
 * The reference's PETSc tracer path -- physics.sediment (up to five size classes), salinity, temperature: shallow water with NT
 * advected tracers, first order, semi-implicit source -- beside the SWE operator, in a kernel of its own
 * (csrc/tracer_kernels.h).  The state is the reference's one Vec with block size n_dof = 3 + NT:
 *     u_local  device, [num_cells][3 + NT] = (h, hu, hv, h c_0 ...), ghosts filled by the caller
 *     f_global device, [num_owned_cells][3 + NT]
 *   rdyhip_tracers_enable              CreatePetscTracerInteriorFluxOperator / ...BoundaryFluxOperator / ...SourceOperator
 *                                      (src/tracer/tracer_petsc.c:295-332, 554-592, 756-785) and the n_dof-wide boundary and
 *                                      source Vecs of CreateOperator (src/operator.c:91-129)
 *   rdyhip_tracers_set_boundary_values SetOperatorBoundaryValues with all n_dof components, as RDySetFlowDirichletBoundaryValues
 *                                      + RDySetSedimentDirichletBoundaryValues leave them (src/rdymms.c:745-760)
 *   rdyhip_tracers_set_source          RDySetRegionalSedimentSource / RDySetDomain... (src/rdymms.c:630): source of tracer
 *                                      `tracer` in `n` owned cells
 *   rdyhip_tracers_rhs_function        OperatorRHSFunction (src/rdysetup.c:1130-1139) with ApplyTracerInteriorFlux,
 *                                      ApplyTracerBoundaryFlux and ApplyTracerSourceSemiImplicit (tracer_petsc.c:152, 405, 617)
 *   rdyhip_tracers_euler_step          TSStep_Euler on top of it
 *   rdyhip_tracers_primitive_variables Operator.primitive_variables as the tracer source operator writes it (715-724)
 *   rdyhip_tracers_get_boundary_fluxes ExtractOperatorBoundaryFluxes for the [num_edges][n_dof] flux Vec
 *
 * _enable allocates what the tracer path needs beyond the operator's own arrays -- boundary values [K][3 + NT], boundary fluxes
 * [K][3 + NT], tracer sources [owned][NT], all zero-initialised -- counted in RDyHipLayoutInfo.device_bytes and freed by
 * rdyhip_destroy; like rdyhip_output_mean_enable it may synchronise the device (as may the first
 * rdyhip_tracers_primitive_variables, which allocates, and the host-array setters / getter, which copy).  The two evaluations
 * enqueue one launch and never synchronise.  A second enable: RDYHIP_ERR_USER.  Refused with RDYHIP_ERR_USER before any device
 * call: num_tracers outside 1..RDYHIP_MAX_TRACERS; an unknown `riemann`; an operator created with second_order, with
 * well_balancing != NONE or with source_method != SEMI_IMPLICIT (the reference's PETSc tracer path has the semi-implicit source
 * only); any boundary of type critical outflow ("CONDITION_CRITICAL_OUTFLOW not supported for tracers", tracer_petsc.c:472-474).
 *
 * The flow part reuses what the operator already owns: Manning's n (rdyhip_set_mannings), the [owned][3] external source
 * (rdyhip_set_external_source: the flow components' source), the mesh tables and the Courant buckets --
 * rdyhip_update_diagnostics / rdyhip_get_diagnostics report the most recent evaluation, of either kind.  The SWE entry points of
 * an operator with tracers enabled behave exactly as before; their boundary values, fluxes and primitive variables are separate
 * arrays which the tracer calls neither read nor write.
 *
 * rdyhip_tracers_rhs_function: F is overwritten and never read, the diagnostics start anew (one launch).  There is no accumulate
 *   form; the phased forms are rdyhip_tracer_phase_* below.
 * rdyhip_tracers_euler_step: u_local_out[owned rows] = fma(dt, F, u_local) for all 3 + NT components, not in place; the ghost
 *   rows of u_local_out are left alone; with f_global == NULL F is never stored.
 * rdyhip_tracers_primitive_variables: the [owned][3 + NT] array (h, u, v, c_0 ...): velocities in the ANUGA form
 *   hu h / (h^2 + h_anuga^2), c_i = h c_i / h, all zero below tiny_h.  The first call allocates it and switches the storing on for
 *   every later evaluation; until one runs it holds zeros.
 * Arithmetic: Riemann states by ComputeRiemannVelocitiesAndConcentration (u = hu / h, c_i = h c_i / h, zero below tiny_h; no ANUGA
 *   regularisation there); flux by ComputeTracerRoeFlux (RDYHIP_TRACER_RIEMANN_ROE) or ComputeUpwindTracerRoeFlux
 *   (RDYHIP_TRACER_RIEMANN_UPWIND_ROE), src/tracer/tracer_roe_flux_petsc.h; Dirichlet and reflecting boundaries; erosion and
 *   deposition with the reference's constants.  Manning's n is indexed by owned cell, as everywhere in this library (the reference
 *   indexes by local cell there: the same on one rank).
 * Stated differences: the flux of a boundary edge is stored for edges whose left cell is owned; rows of edges behind ghost cells
 *   are left as they are.  There is no accumulated-flux array (the reference's tracer boundary operator keeps none).  On a rank
 *   with ghost cells the Courant diagnostic covers the edges of the owned cells with len / area_self only: edges between two
 *   ghosts, and the len / area of a ghost that is the smaller cell of a cut edge, do not enter; the cell reported for a cut edge
 *   is the owned one.  The maximum over the ranks is still the whole mesh's: the smaller cell of every cut edge is owned by someone.
 * Ghost rows of 3 + NT values travel through the halo object (rdyhip_halo_tracers_* below, rdyhip_halo_exchange with
 * ncomp = 3 + NT) or through rdyhip_pack_rows / rdyhip_unpack_rows; rdyhip_output_mean_*, rdyhip_series_* and rdyhip_state_* cover
 * the three flow components of the SWE state only: the 3 + NT-wide forms are "tracer output" below.
 *
 * On several ranks (a partitioned mesh; DMGlobalToLocalBegin/End of OperatorRHSFunction, src/rdysetup.c:1133-1134, ahead of
 * the tracer operators of src/tracer/tracer_petsc.c):
 *   rdyhip_tracer_phase_rhs / rdyhip_tracer_phase_euler_step   rdyhip_tracers_rhs_function / _euler_step restricted to
 *       RDYHIP_PHASE_INTERIOR (owned cells without a ghost neighbour) or RDYHIP_PHASE_HALO (with one); RDYHIP_PHASE_ALL with
 *       RDYHIP_PHASE_RESET_DIAGNOSTICS is exactly the unphased call.  `flags`: RDYHIP_PHASE_RESET_DIAGNOSTICS starts the Courant
 *       diagnostic anew, without it the launch merges into it (larger value, then the earlier edge of the reference's loop), so
 *       INTERIOR with the flag followed by HALO without it reports what one call over all cells reports;
 *       RDYHIP_PHASE_OVERWRITE is implied and accepted, any other bit is refused.  Rows of cells of the other phase -- F, the
 *       primitive variables, u_local_out, boundary fluxes -- are not touched.  A HALO call on a rank without ghost-adjacent cells
 *       launches nothing; with the reset flag it still restarts the diagnostic.
 *   rdyhip_halo_tracers_rhs / rdyhip_halo_tracers_euler_step   the ghost update of the [num_cells][3 + NT] state and the
 *       evaluation in one call, as rdyhip_rhs_overlapped / rdyhip_euler_step_overlapped are for the SWE state.  In order: pack,
 *       transfer, unpack of 3 + NT values per cell on `stream`, then ONE launch.  Two streams: the exchange on the halo's
 *       stream, the INTERIOR launch on `stream` meanwhile (enqueued before a transport callback is called, behind an RCCL
 *       group), the join, the HALO launch on `stream`.  The form is chosen per kind by the halo's trial
 *       (RDYHIP_HALO_STEP_TRACERS_RHS / _EULER).  Direct receive applies as it is.  The fused pack does not extend to tracer
 *       rows: a tracer step always packs, and the next rdyhip_euler_step_overlapped packs again.  A halo created after
 *       rdyhip_tracers_enable has buffers of max(3 or 6, 3 + NT) values per cell; on one created before, the first tracer step
 *       grows them -- it waits for what the halo's stream and `stream` still run, the only call of the tracer path that may
 *       synchronise -- and rdyhip_halo_exchange(halo, rows, 3 + NT, ...) works from then on.  A rank that owns nothing
 *       launches nothing but takes part in the exchange.
 *   Refused with RDYHIP_ERR_USER before any device call: a null operator or halo, tracers not enabled, a halo of another
 *   operator, a null u_local on a rank with cells, u_local_out == u_local (or null), an unknown phase, unknown flag bits.
 * Every argument error (a null operator, tracers not enabled, a null array where one is needed, a tracer or boundary index out of
 * range, num_edges not the boundary's) is RDYHIP_ERR_USER and is reported before any device call.  A rank that owns nothing
 * launches nothing and succeeds.
 *
 * Under hydrostatic reconstruction (ApplyTracerInteriorFluxHR, ApplyTracerSourceHRSemiImplicit, tracer_petsc.c:807-986,
 * 1067-1154; wired by CreatePetscFluxHROperator / CreatePetscSourceHROperator, src/operator_fluxes_petsc.c:59-95,
 * src/operator_sources_petsc.c:30-45):
 *   rdyhip_tracer_hr_enable   rdyhip_tracers_enable for an operator created with RDYHIP_WELL_BALANCING_HR: the same allocations,
 *       the same bytes in device_bytes, the same range checks.  After it every call of this section and of "tracer output" works
 *       unchanged and evaluates the HR form (tracer_hr_kernel, csrc/tracer_kernels.h); rdyhip_tracers_info keeps its two outputs.
 *       rdyhip_tracers_enable itself keeps refusing such an operator (its message names this call).  Refused with
 *       RDYHIP_ERR_USER before any device call, in this order: a null operator ("null operator"); tracers already enabled, by
 *       either call; num_tracers outside 1..RDYHIP_MAX_TRACERS; an unknown `riemann`; second_order; an operator without HR (the
 *       message points to rdyhip_tracers_enable); a source method other than semi-implicit ("Only semi_implicit is supported for
 *       tracer HR", tracer_petsc.c:1191); a critical-outflow boundary.
 *   rdyhip_tracer_hr_info     RDYHIP_WELL_BALANCING_HR after rdyhip_tracer_hr_enable, RDYHIP_WELL_BALANCING_NONE after
 *       rdyhip_tracers_enable and while tracers are off.
 * Arithmetic of an interior edge (boundary edges are those of the plain path: HR is a no-op there, operator_fluxes_petsc.c:79-93):
 *   velocities of both cells in the ANUGA form hu h / (h^2 + h_anuga^2) under the HR operator's wet test h > tiny_h (869-875),
 *   c_j = (h > tiny_h) ? h c_j / h : 0 (889-890); both depths reconstructed against max(zc_L, zc_R), h_rec = max(0, h + zc - z_max)
 *   (863-867), velocities and concentrations unchanged, so the tracer flux sees h_rec c (892-893).  The edge contributes unless both
 *   ORIGINAL depths are below tiny_h (922); inside that guard the 3 + NT flux components and the Courant candidate enter only where
 *   hL_rec > tiny_h or hR_rec > tiny_h (939) -- with both at 0 the Roe solver's 0 / 0 is discarded by a branch, never multiplied
 *   by zero --, and each side's pressure correction 0.5 g (h^2 - h_rec^2) (cn, sn) enters the two momentum components whenever the
 *   outer guard holds (964-977), after the edge's flux.  The source has no bed slope; friction, erosion, deposition and the
 *   primitive variables are those of the plain path.
 * Two wet rules: interior edges use "h > tiny_h" with the regularised velocity; boundary edges, the source and the primitive
 *   variables keep the plain path's "h < tiny_h => 0" (no regularisation on boundary edges and in the source).  They differ at
 *   h == tiny_h exactly and where h_anuga != 0.  The stated differences above (owned-side Courant rule, boundary fluxes stored where
 *   the left cell is owned) hold as they are. */
#define RDYHIP_MAX_TRACERS 7                 /* MAX_NUM_TRACERS: 5 sediment classes + salinity + temperature (CMakeLists.txt:12-22) */
#define RDYHIP_TRACER_RIEMANN_ROE 0          /* ComputeTracerRoeFlux */
#define RDYHIP_TRACER_RIEMANN_UPWIND_ROE 1   /* ComputeUpwindTracerRoeFlux (RIEMANN_UPWIND_ROE) */
int rdyhip_tracers_enable(RDyHipOperator op, int32_t num_tracers, int32_t riemann);
int rdyhip_tracers_info(RDyHipOperator op, int32_t *num_tracers, int32_t *riemann);            /* 0 tracers: not enabled */
int rdyhip_tracers_set_boundary_values(RDyHipOperator op, int32_t boundary, int32_t num_edges, const double *values /* host [num_edges][3+NT] */);
int rdyhip_tracers_set_source(RDyHipOperator op, int32_t tracer, int32_t n, const int32_t *owned_cell_ids /* NULL: 0..n-1 */, const double *values /* host */);
int rdyhip_tracers_rhs_function(RDyHipOperator op, double dt, const double *u_local, double *f_global, void *stream);
int rdyhip_tracers_euler_step(RDyHipOperator op, double dt, const double *u_local, double *u_local_out, double *f_global /* may be NULL */, void *stream);
int rdyhip_tracers_primitive_variables(RDyHipOperator op, const double **device_ptr, int64_t *num_values);
int rdyhip_tracers_get_boundary_fluxes(RDyHipOperator op, int32_t boundary, int32_t num_edges, double *fluxes /* host [num_edges][3+NT] */);
/* rdyhip_tracers_rhs_function / _euler_step restricted to a phase; flags: RDYHIP_PHASE_RESET_DIAGNOSTICS only
 * (RDYHIP_PHASE_OVERWRITE is implied and accepted; there is still no accumulate form) */
int rdyhip_tracer_phase_rhs(RDyHipOperator op, int32_t phase, int32_t flags, double dt, const double *u_local, double *f_global, void *stream);
int rdyhip_tracer_phase_euler_step(RDyHipOperator op, int32_t phase, int32_t flags, double dt, const double *u_local, double *u_local_out,
                                   double *f_global /* may be NULL */, void *stream);
/* ghost update of the [num_cells][3 + NT] state + the evaluation, as rdyhip_rhs_overlapped / rdyhip_euler_step_overlapped */
int rdyhip_halo_tracers_rhs(RDyHipOperator op, RDyHipHalo halo, double dt, double *u_local, double *f_global, void *stream);
int rdyhip_halo_tracers_euler_step(RDyHipOperator op, RDyHipHalo halo, double dt, double *u_local, double *u_local_out, double *f_global, void *stream);
/* tracers under hydrostatic reconstruction: the enable for an operator created with RDYHIP_WELL_BALANCING_HR, and which form runs */
int rdyhip_tracer_hr_enable(RDyHipOperator op, int32_t num_tracers, int32_t riemann);
int rdyhip_tracer_hr_info(RDyHipOperator op, int32_t *well_balancing);   /* RDYHIP_WELL_BALANCING_NONE or _HR; NONE also when tracers are off */

/* ---- tracer output: read-out, error sums, output means and observation series of the [num_cells][3 + NT] state ----------------
 * What the three sections "time-averaged output fields", "time series on the device" and "state read-out" above do for rows of
 * three doubles, for the tracer state's rows of N = 3 + NT (csrc/tracer_output_kernels.h), so that a sediment run needs no copy of
 * the whole state to the host for a concentration field, an MMS norm, an averaged output or a gauge record.  The reference treats
 * none of these as flow-only:
 *   rdyhip_tracer_state_planes / _read_*   RDyGetOwnedCell* of src/rdydata.c:171-205 for any component of the n_dof-wide Vec, and
 *                                          the XDMF output variables, Vecs of block size n_dof (src/xdmf_output.c:196-241)
 *   rdyhip_tracer_error_sums / _get        the rank-local loops of RDyMMSComputeErrorNorms over ndof (src/rdymms.c:859-880)
 *   rdyhip_tracer_output_mean_*            AccumulateOutputVar / ComputeMean / ResetOutputVar (src/xdmf_output.c:196-241, 436-504)
 *   rdyhip_tracer_series_*                 WriteObservations with num_comp columns per site (src/time_series.c:419-440)
 * The entry points carry the prefix rdyhip_tracer_ (as rdyhip_tracer_phase_*), not rdyhip_tracers_: that prefix names the eight
 * calls of the evaluation itself.  Every call reports a null operator first, "tracers are not enabled" next, and every other
 * argument error before any device call, all as RDYHIP_ERR_USER; on a rank that owns nothing it launches nothing while times
 * and record counts still advance; owned cells that are not the first rows of the local vector are found through the operator's
 * own table.  All device memory is counted in RDyHipLayoutInfo.device_bytes and freed by rdyhip_destroy, after a copy in flight.
 *
 * `comps` is a mask: bit i stands for component i of the row, 0 <= i < N (bits 0..2 are RDYHIP_COMPONENT_H / _HU / _HV, bit 3 + j
 * is tracer j).  An empty mask or a bit at N or above: RDYHIP_ERR_USER.  `comp` is exactly one bit.  `form`:
 *   RDYHIP_TRACER_FORM_CONSERVED  (h, hu, hv, h c_0 ...): the row as it is.  Nothing is computed, values move as 64-bit patterns:
 *                                 -0.0, NaN payloads and denormals survive.
 *   RDYHIP_TRACER_FORM_PRIMITIVE  (h, u, v, c_0 ...): what a tracer evaluation stores as primitive variables
 *                                 (rdyhip_tracers_primitive_variables), with that store's own arithmetic -- the same bits.
 *   - rdyhip_tracer_state_planes, the device form: ONE launch on `stream`.  d_planes[k][o] = row(loc(o))[c_k], k over the set bits
 *     c_k of `comps` ascending, o over the owned cells; d_planes is device memory [popcount(comps)][num_owned_cells].
 *   - rdyhip_tracer_state_read_begin / _ready / _wait / _get / _ptr: the state machine of rdyhip_state_read_* word for word --
 *     the launch on `stream`, an event, the copy into pinned memory on the operator's copy stream, a second event; only _wait
 *     blocks; a begin over a read in flight is ordered behind the earlier copy and replaces it; size != num_owned_cells is
 *     RDYHIP_ERR_ARG_SIZ -- with planes, pinned memory and events of its own: a flow read and a tracer read may be in flight at
 *     once and neither disturbs the other.
 *   - rdyhip_tracer_error_sums / _get: rdyhip_error_sums for N components; d_exact is device memory [num_owned_cells][N] or NULL.
 *     The same two launches without atomics, the same block size, workgroup count, lane-to-cell assignment and order of every
 *     addition, with records of 3 N + 1 doubles: components 0..2 are the SAME BITS rdyhip_error_sums gives for the [cell][3] slice
 *     of the same state, and a tracer column equal to the h column gives the h column's bits.  Entries at N and above are 0.  The
 *     area table is shared with rdyhip_error_sums; records and the pinned result are this feature's.  _get is the only blocking
 *     call.  The MPI_Allreduce and the square root stay with the caller.
 *   - rdyhip_tracer_output_mean_*: three accumulators [num_owned_cells][N] (`vars`: RDYHIP_OUTPUT_* bits), each with its own time.
 *     _accumulate is one launch for any subset: the solution fma(dt, u_solution[loc(o)], acc); the primitive variables formed in
 *     the launch from u_primitive[loc(o)] with the FORM_PRIMITIVE arithmetic -- there is no hidden "state of the last
 *     evaluation": the caller passes the array the reference's source operator saw, the input of a fused Euler step or the
 *     argument of a plain evaluation; where the two pointers are equal the row is read once; either may be NULL when its variable
 *     is not in `vars` --; the sources, row = the operator's [owned][3] external source followed by the [owned][NT] tracer source,
 *     read at the call's place in `stream` exactly as rdyhip_output_mean_accumulate documents (the water-only plane and the
 *     uniform-source mode of the SWE kernels change nothing: the canonical arrays are always current).  _get scales by 1 / time
 *     formed on the host into d_mean (device, [num_owned_cells][N]); no accumulated time: RDYHIP_ERR_USER.  A second _enable
 *     keeps an accumulator's content.
 *   - rdyhip_tracer_series_*: the semantics of RDYHIP_SERIES_OBSERVATIONS with N values per site -- sites are owned-cell ids,
 *     range-checked on the host; repeats are allowed; num_sites == 0 is valid; a full log is RDYHIP_ERR_USER with nothing
 *     launched; a second enable is RDYHIP_ERR_USER; _read (host arrays, values [count][num_sites][N]) is the only blocking call.
 *     There is no boundary-flux series for tracers: the reference refuses it (src/time_series.c:76-78, ndof == 3 only). */
#define RDYHIP_TRACER_FORM_CONSERVED 0
#define RDYHIP_TRACER_FORM_PRIMITIVE 1
typedef struct {
  double l1[10], l2_squared[10], linf[10], area;   /* entries >= 3 + NT are 0 */
} RDyHipTracerErrorSums;
int rdyhip_tracer_state_planes(RDyHipOperator op, int32_t comps, int32_t form, const double *u_local, double *d_planes, void *stream);
int rdyhip_tracer_state_read_begin(RDyHipOperator op, int32_t comps, int32_t form, const double *u_local, void *stream);
int rdyhip_tracer_state_read_ready(RDyHipOperator op, int32_t *ready);
int rdyhip_tracer_state_read_wait(RDyHipOperator op);
int rdyhip_tracer_state_read_get(RDyHipOperator op, int32_t comp, int32_t size, double *values /* host */);
int rdyhip_tracer_state_read_ptr(RDyHipOperator op, int32_t comp, const double **pinned_values);
int rdyhip_tracer_error_sums(RDyHipOperator op, const double *u_local, const double *d_exact /* [owned][N] or NULL */, void *stream);
int rdyhip_tracer_error_sums_get(RDyHipOperator op, RDyHipTracerErrorSums *out);
int rdyhip_tracer_output_mean_enable(RDyHipOperator op, int32_t vars);
int rdyhip_tracer_output_mean_accumulate(RDyHipOperator op, int32_t vars, double dt, const double *u_solution, const double *u_primitive, void *stream);
int rdyhip_tracer_output_mean_get(RDyHipOperator op, int32_t var, double *d_mean /* [owned][N] */, double *accumulated_time, void *stream);
int rdyhip_tracer_output_mean_reset(RDyHipOperator op, int32_t vars, void *stream);
int rdyhip_tracer_output_mean_time(RDyHipOperator op, int32_t var, double *accumulated_time);
int rdyhip_tracer_series_enable(RDyHipOperator op, int32_t num_sites, const int32_t *owned_cell_ids /* host */, int32_t capacity);
int rdyhip_tracer_series_record(RDyHipOperator op, double time, const double *u_local, void *stream);
int rdyhip_tracer_series_info(RDyHipOperator op, int32_t *entries, int32_t *count, int32_t *capacity);
int rdyhip_tracer_series_read(RDyHipOperator op, int32_t first, int32_t count, double *times, double *values /* host [count][S][N] */, void *stream);
int rdyhip_tracer_series_clear(RDyHipOperator op);

/* ---- ensembles: several simulations on one mesh, one launch per evaluation --------------------------------------------------------
 * The reference's `ensemble:` section (docs/common/input.md:158-225, docs/developer/organization.md:373-395; the test deck
 * driver/tests/swe_roe/ex2b-ensemble.yaml: two members, Manning 0.015 and 0.030): ConfigureEnsembleMember (src/ensemble.c:5-84)
 * splits the communicator, and every member gets ranks, a mesh copy, an operator and a TS of its own.  Here ONE operator holds
 * B members side by side and evaluates all of them in one launch (csrc/ensemble_kernels.h): a thread loads its cell's geometry once
 * and walks the members with it.  Results are per member, exactly as if each member ran alone.
 *
 * State: u_local is device memory [B][num_cells][3], f_global [B][num_owned_cells][3], member-major on purpose: member m's slice
 *   u_local + 3 m num_cells is an ordinary SWE state, and every existing call works on it unchanged -- rdyhip_halo_exchange,
 *   rdyhip_pack_cells, rdyhip_state_planes / rdyhip_state_read_*, rdyhip_error_sums, the output means.
 * rdyhip_ensemble_enable: allocates per member Manning's n [B][owned], the external source [B][owned][3], boundary values and
 *   boundary fluxes [B][K][3] each, the Courant buckets [B][W] (W = 4 x the workgroups of the cell-centric launch: 12 bytes each)
 *   and the B 16-byte diagnostics -- B (32 owned + 48 K + 12 W + 16) bytes, counted in RDyHipLayoutInfo.device_bytes and freed by
 *   rdyhip_destroy -- and fills every member's Manning's n, source and boundary values with the operator's current arrays by
 *   device copies: a member then overrides only what differs (the rule of ConfigureEnsembleMember).  Boundary fluxes start at
 *   zero.  It may synchronise.  rdyhip_ensemble_info: the number of members, 0: not enabled.
 * rdyhip_ensemble_set_mannings / _set_external_source / _set_boundary_values: member `member`'s values, with the arguments of
 *   rdyhip_set_mannings, rdyhip_set_external_source and rdyhip_set_boundary_values (all three components).  They synchronise.
 * dts: one dt per member (each member has its own TS); dt enters the friction term and the Courant number.  The host array [B] is
 *   read at the call and travels by value in the kernel arguments; neither evaluation call synchronises or copies.
 * rdyhip_ensemble_rhs_function: for each member F is overwritten and never read, its boundary fluxes are stored and its diagnostic
 *   starts anew; one launch serves all members.  RDYHIP_PHASE_ALL only, no accumulate form.
 * rdyhip_ensemble_euler_step: u_local_out[m][owned rows] = fma(dts[m], F, u_local), not in place (u_local_out == u_local is
 *   RDYHIP_ERR_USER); the ghost rows of u_local_out are left alone; with f_global == NULL F is never stored.
 * rdyhip_ensemble_update_diagnostics: one merge launch for all members, one copy of B x 16 bytes, one stream synchronise;
 *   rdyhip_ensemble_get_diagnostics then returns each member's value and ids, translated as rdyhip_update_diagnostics does.  Of
 *   edges that tie, the first in the reference's loop order wins.
 * Supported: first order, well_balancing NONE (HR: rdyhip_ens_hr_enable, below), both source methods, all three boundary types, triangles, quads and mixed meshes,
 *   ranks with ghost cells.
 * Stated differences: there is no accumulated boundary-flux array.  Primitive variables and the flux divergence are not stored.
 *   The flux of a boundary edge is stored where its left cell is owned; rows of edges behind ghost cells are left as they are.  On
 *   a rank with ghost cells the Courant diagnostic covers the edges of the owned cells with len / area_self only, and the cell
 *   reported for a cut edge is the owned one.  The SWE entry
 *   points of an operator with the ensemble enabled behave exactly as before and share no array with it.
 * Every argument error -- a null operator, num_members outside 1..RDYHIP_MAX_ENSEMBLE_MEMBERS, an operator created with
 *   second_order or hydrostatic reconstruction, a second enable, any other call before enable, a member, boundary or component
 *   index out of range, num_edges not the boundary's, a null array where one is needed -- is RDYHIP_ERR_USER and is reported
 *   before any device call.  A rank that owns nothing launches nothing and succeeds.
 *
 * Ensembles under hydrostatic reconstruction (members over real beds with wet / dry fronts):
 *   rdyhip_ens_hr_enable   rdyhip_ensemble_enable for an operator created with RDYHIP_WELL_BALANCING_HR: the same allocations, the
 *                          same copies of the operator's inputs into the members, the same member groups and checks; every
 *                          rdyhip_ensemble_* call above then works unchanged -- and rdyhip_diagnostics_begin / _wait in the ensemble
 *                          scope -- and evaluates ApplyInteriorFluxHR and the HR source (src/swe/swe_petsc.c:1000-1161, 1229-1263)
 *                          of every member in one launch of ensemble_hr_kernel: interior edges reconstruct both depths against
 *                          max(zc_L, zc_R) with the HR operator's wet test h > tiny_h and add each side's pressure correction,
 *                          boundary edges are the plain path's (HR is a no-op there), the source has no bed slope.  Both source
 *                          methods.  The bed elevations are the operator's own (shared by the members, like the mesh).
 *                          Refused with RDYHIP_ERR_USER before any device call: an operator created without
 *                          RDYHIP_WELL_BALANCING_HR, one created with second_order, a second enable (of either kind),
 *                          num_members outside 1..RDYHIP_MAX_ENSEMBLE_MEMBERS.  rdyhip_ensemble_enable keeps refusing an HR
 *                          operator.  The stated differences are those above.
 *   rdyhip_ens_hr_info     RDYHIP_WELL_BALANCING_HR after rdyhip_ens_hr_enable, RDYHIP_WELL_BALANCING_NONE after
 *                          rdyhip_ensemble_enable or before either. */
#define RDYHIP_MAX_ENSEMBLE_MEMBERS 64
int rdyhip_ens_hr_enable(RDyHipOperator op, int32_t num_members);
int rdyhip_ens_hr_info(RDyHipOperator op, int32_t *well_balancing);   /* RDYHIP_WELL_BALANCING_NONE or _HR; NONE also when the ensemble is off */
int rdyhip_ensemble_enable(RDyHipOperator op, int32_t num_members);
int rdyhip_ensemble_info(RDyHipOperator op, int32_t *num_members);                 /* 0: not enabled */
int rdyhip_ensemble_set_mannings(RDyHipOperator op, int32_t member, int32_t n, const int32_t *owned_cell_ids /* NULL: 0..n-1 */, const double *values /* host */);
int rdyhip_ensemble_set_external_source(RDyHipOperator op, int32_t member, int32_t comp, int32_t n, const int32_t *owned_cell_ids, const double *values);
int rdyhip_ensemble_set_boundary_values(RDyHipOperator op, int32_t member, int32_t boundary, int32_t num_edges, const double *values /* host [num_edges][3] */);
int rdyhip_ensemble_rhs_function(RDyHipOperator op, const double *dts /* host [B] */, const double *u_local, double *f_global, void *stream);
int rdyhip_ensemble_euler_step(RDyHipOperator op, const double *dts, const double *u_local, double *u_local_out, double *f_global /* may be NULL */, void *stream);
int rdyhip_ensemble_get_boundary_fluxes(RDyHipOperator op, int32_t member, int32_t boundary, int32_t num_edges, double *fluxes /* host [num_edges][3] */);
int rdyhip_ensemble_update_diagnostics(RDyHipOperator op, void *stream);
int rdyhip_ensemble_get_diagnostics(RDyHipOperator op, RDyHipCourant *courant /* [B] */);

/* ---- ensemble output: read-out, error sums, output means, observation series and statistics of the [B][num_cells][3] state --------
 * What the sections "state read-out", "time-averaged output fields" and "time series on the device" above do for one [cell][3]
 * state, for all B members of an ensemble in ONE launch per call (csrc/ens_output_kernels.h) instead of B launches and B blocking
 * round trips on the members' slices, and the per-cell statistics over the members, which the per-member calls cannot form without
 * copying B states to the host.  The reference runs every member as a simulation of its own (src/ensemble.c:5-84), so each member's
 * output is the reference's own:
 *   rdyhip_ens_state_planes / _read_*   RDyGetOwnedCell{Heights,XMomenta,YMomenta} (src/rdydata.c:171-205) of every member
 *   rdyhip_ens_error_sums / _get        the rank-local loops of RDyMMSComputeErrorNorms (src/rdymms.c:869-880) of every member
 *   rdyhip_ens_output_mean_*            AccumulateOutputVar / ComputeMean / ResetOutputVar (src/xdmf_output.c:196-241, 436-504)
 *   rdyhip_ens_series_*                 WriteObservations (src/time_series.c:399-402, 530-564) of every member
 *   rdyhip_ens_stats                    no counterpart: mean, minimum and maximum over the members (the inundation envelope)
 * Every call needs an enabled ensemble of either family (rdyhip_ensemble_enable or rdyhip_ens_hr_enable; after the enable the
 * family makes no difference): a null operator is reported first, "the ensemble is not enabled" next, every other argument error
 * before any device call, all as RDYHIP_ERR_USER.  u_local is device memory [B][num_cells][3], member-major, as
 * rdyhip_ensemble_rhs_function takes it; loc(o) is the local cell of owned cell o (the operator's own table where the owned cells
 * are not the first rows).  A rank that owns nothing launches nothing and succeeds, while times and record counts still advance.
 * Device memory, counted in RDyHipLayoutInfo.device_bytes as soon as it is allocated and freed by rdyhip_destroy, which waits for a
 * copy that is still in flight (B members, o = num_owned_cells, S sites, G = min(ceil(o / RDYHIP_ERROR_SUMS_BLOCK),
 * RDYHIP_ERROR_SUMS_MAX_WORKGROUPS)):
 *   the read-out     8 B k o bytes for the widest mask (k bits) begun so far; rdyhip_ens_state_planes writes the caller's memory
 *   the error sums   80 B (G + 1) bytes at the first call, and the area table 8 o + the 80 (G + 1) bytes of rdyhip_error_sums if
 *                    that has not been called yet (they are shared with it and counted once)
 *   the means        24 B o bytes per enabled variable
 *   the series       24 B S capacity + 4 S bytes
 *   the statistics   none
 *
 * `comps` is a mask of RDYHIP_COMPONENT_* (1..7), `comp` exactly one of them, `member` in [0, B).
 *   - rdyhip_ens_state_planes, the device form: ONE launch on `stream`.  d_planes[m][k][o] = u_local[m][loc(o)][c_k], k over the set
 *     bits c_k of `comps` ascending; d_planes is device memory [B][popcount(comps)][num_owned_cells].  Values move as 64-bit
 *     patterns: -0.0, NaN payloads and denormals survive.  Member m's planes are rdyhip_state_planes of member m's slice.
 *   - rdyhip_ens_state_read_begin / _ready / _wait / _get / _ptr: the state machine of rdyhip_state_read_* rule for rule -- the
 *     same launch into planes the operator owns, an event, ONE device-to-host copy of all B k planes on the operator's copy stream,
 *     a second event; only _wait blocks; buffers grow only; a begin over a read that has not landed is ordered behind the earlier
 *     copy and replaces it; _get / _ptr before _wait, or for a component the last begin did not ask for: RDYHIP_ERR_USER;
 *     size != num_owned_cells: RDYHIP_ERR_ARG_SIZ -- with planes, pinned memory and events of its own: the SWE read-out of the same
 *     operator may be in flight at the same time and is never disturbed.
 *   - rdyhip_ens_error_sums / _get: rdyhip_error_sums for all members in two launches; d_exact is device memory
 *     [B][num_owned_cells][3] or NULL; `out` of _get is [B].  The partial kernel runs on a (G, B) grid, the finalize kernel with
 *     workgroup m for member m, then B x 80 bytes go into pinned memory behind an event; _get is the only blocking call.  The
 *     lane-to-cell assignment, the order of every fold and the three operations per component are those of rdyhip_error_sums:
 *     member m's record is the SAME BITS rdyhip_error_sums gives for member m's slice (and its exact slice).  The result of
 *     rdyhip_error_sums on the same operator is left as it was.  NaN: as rdyhip_error_sums.
 *   - rdyhip_ens_output_mean_*: per enabled variable (`vars`: RDYHIP_OUTPUT_* bits) one accumulator [B][num_owned_cells][3] and one
 *     accumulated time per member, kept on the host.  _accumulate: `dts` is a host array [B], read at the call; ONE launch for all
 *     members and all of `vars`.  Per member m: the solution, acc = fma(dts[m], u_solution[m][loc(o)][c], acc); the primitive
 *     variables (h, u, v) formed in the launch from u_primitive[m][loc(o)] by the arithmetic with which the SWE kernels store them
 *     and rdyhip_output_mean_accumulate derives them -- the same bits; there is no hidden "state of the last evaluation": the
 *     caller passes the array the evaluation saw, after a fused Euler step its input; the sources, member m's own external source
 *     [num_owned_cells][3] (rdyhip_ensemble_set_external_source), read at the call's place in `stream`.  Where u_solution ==
 *     u_primitive the row is read once; either may be NULL when its variable is not in `vars`.  Each member's time advances by
 *     its own dts[m].  _get: d_mean (device, [B][num_owned_cells][3]) = accumulator x (1 / accumulated time of member m), the
 *     reciprocal formed on the host as rdyhip_output_mean_get forms it; accumulated_times is a host array [B] or NULL; a member
 *     with no accumulated time: RDYHIP_ERR_USER, nothing is launched and nothing written.  _reset: accumulators and all B times of
 *     `vars` back to zero.  _time: accumulated_times is a host array [B].  A variable that is not enabled, unknown bits, more or
 *     less than one bit where one variable is asked for, a null array where one is needed: RDYHIP_ERR_USER.  A second _enable
 *     keeps an accumulator's content.
 *   - rdyhip_ens_series_*: the semantics of RDYHIP_SERIES_OBSERVATIONS for all members at once -- sites are owned-cell ids, shared
 *     by the members and range-checked on the host; repeats are allowed; num_sites == 0 is valid; _record (`times`: host array [B],
 *     one time per member, read at the call) is ONE launch that appends a record [B][S][3] to the log [capacity][B][S][3]; a full
 *     log is RDYHIP_ERR_USER with nothing launched; a second enable is RDYHIP_ERR_USER; _read (host arrays, times [count][B],
 *     values [count][B][S][3]) is the only blocking call; _clear empties the log.
 *     There is no boundary-flux series for ensembles: the ensemble keeps no accumulated boundary-flux array (a stated difference
 *     above), so there is nothing to record; a member's instantaneous fluxes are rdyhip_ensemble_get_boundary_fluxes.
 *   - rdyhip_ens_stats: ONE launch, one lane per owned cell, which finds loc(o) once and walks the members.  d_stats is device
 *     memory [popcount(comps)][3][num_owned_cells]; for the k-th component c_k and x_m = u_local[m][loc(o)][c_k] the three planes are
 *       mean  s = x_0; s = s + x_m for m = 1 .. B-1 in that order; then s * (1.0 / B), the reciprocal formed on the host
 *       min   r = x_0; r = (x_m < r) ? x_m : r in member order
 *       max   r = x_0; r = (x_m > r) ? x_m : r in member order
 *     Comparisons, not fmin / fmax: of values that compare equal (a tie; +0.0 and -0.0) the EARLIER member's bits are kept; a NaN
 *     in a later member never replaces the running value; a NaN in member 0 stays to the end.  A NaN in any member makes the mean
 *     NaN.  The result is the same bits on every run. */
int rdyhip_ens_state_planes(RDyHipOperator op, int32_t comps, const double *u_local, double *d_planes /* [B][k][owned] */, void *stream);
int rdyhip_ens_state_read_begin(RDyHipOperator op, int32_t comps, const double *u_local, void *stream);
int rdyhip_ens_state_read_ready(RDyHipOperator op, int32_t *ready);
int rdyhip_ens_state_read_wait(RDyHipOperator op);
int rdyhip_ens_state_read_get(RDyHipOperator op, int32_t member, int32_t comp, int32_t size, double *values /* host */);
int rdyhip_ens_state_read_ptr(RDyHipOperator op, int32_t member, int32_t comp, const double **pinned_values);
int rdyhip_ens_error_sums(RDyHipOperator op, const double *u_local, const double *d_exact /* [B][owned][3] or NULL */, void *stream);
int rdyhip_ens_error_sums_get(RDyHipOperator op, RDyHipErrorSums *out /* [B] */);
int rdyhip_ens_output_mean_enable(RDyHipOperator op, int32_t vars);
int rdyhip_ens_output_mean_accumulate(RDyHipOperator op, int32_t vars, const double *dts /* host [B] */, const double *u_solution, const double *u_primitive, void *stream);
int rdyhip_ens_output_mean_get(RDyHipOperator op, int32_t var, double *d_mean /* [B][owned][3] */, double *accumulated_times /* host [B] or NULL */, void *stream);
int rdyhip_ens_output_mean_reset(RDyHipOperator op, int32_t vars, void *stream);
int rdyhip_ens_output_mean_time(RDyHipOperator op, int32_t var, double *accumulated_times /* host [B] */);
int rdyhip_ens_series_enable(RDyHipOperator op, int32_t num_sites, const int32_t *owned_cell_ids /* host */, int32_t capacity);
int rdyhip_ens_series_record(RDyHipOperator op, const double *times /* host [B] */, const double *u_local, void *stream);
int rdyhip_ens_series_info(RDyHipOperator op, int32_t *entries, int32_t *count, int32_t *capacity);
int rdyhip_ens_series_read(RDyHipOperator op, int32_t first, int32_t count, double *times /* host [count][B] */, double *values /* host [count][B][S][3] */, void *stream);
int rdyhip_ens_series_clear(RDyHipOperator op);
int rdyhip_ens_stats(RDyHipOperator op, int32_t comps, const double *u_local, double *d_stats /* [k][3][owned] */, void *stream);

/* ---- introspection ----------------------------------------------------------
 * numbers describing the device layout, for DESIGN.md / bench.py */
typedef struct {
  int32_t num_owned_cells, num_cells, slots_per_cell, num_boundary_edges;
  int32_t num_halo_cells;     /* owned cells with a ghost neighbour */
  int32_t tiled_kernel;       /* 1: tiled LDS kernel (default), 0: cell-centric kernel (RDYHIP_KERNEL=cell) */
  int32_t num_tiles;          /* tiles of 256 owned cells */
  int32_t num_halo_tiles;     /* tiles with a ghost-adjacent cell (second order: or a ghost-adjacent first-ring cell) */
  int32_t max_tile_edges;     /* largest edge list of a tile */
  int32_t max_tile_halo_cells; /* largest number of out-of-tile neighbour cells of a tile */
  int64_t num_halo_entries;   /* sum of the tiles' halo-cell lists */
  int64_t num_edge_records;   /* sum of the tiles' edge lists (cut edges appear in two tiles) */
  int32_t owned_is_prefix;    /* 1 if owned cell o is local cell o */
  int64_t device_bytes;       /* bytes of device memory held by the operator */
  int64_t bytes_per_apply;    /* bytes one full apply must move (layout-exact, not the 176 B/cell model); a create-time figure and
                                 an upper bound: it counts 24 B per cell for the external source, of which the first-order / HR
                                 kernels read 8 B while the source is water only (rdyhip_source_is_water_only) */
  int32_t second_order_fused; /* 1 for a second-order operator: the gradients are formed in LDS by the flux kernel, only
                                 rdyhip_compute_gradients(RDYHIP_PHASE_HALO) is needed before the gradient exchange (the
                                 two-launch form of rounds 1-4 is gone); 0: first order */
  int32_t max_tile_ring2_cells; /* second order: largest first + second ring of a tile */
  int32_t persistent_grid;    /* workgroups of a full apply of the tiled kernel (resident workgroups per CU x CUs) */
  int32_t lds_bytes;          /* dynamic LDS per workgroup of that kernel */
  int32_t lds_fixed_layout;   /* 1 for the tiled kernels: every tile is cut to their fixed capacities at create, the LDS planes have
                                 compile-time lengths (plane offsets are instruction immediates); 0: the cell-centric kernel */
} RDyHipLayoutInfo;
int rdyhip_layout_info(RDyHipOperator op, RDyHipLayoutInfo *info);
/* the same numbers from the host-side layout pass alone (validation of the mesh, slot tables, tiles): no device is
 * touched, so a mesh and its numbering can be checked -- and every rdyhip_create argument error reproduced -- on a
 * machine without a GPU; device_bytes and persistent_grid are 0 */
int rdyhip_probe_layout(const RDyHipConfig *config, const RDyHipMesh *mesh, int32_t num_boundaries, const RDyHipBoundary *boundaries,
                        RDyHipLayoutInfo *info);
/* resident workgroups per CU the first-order / HR tiled kernels of one family were built for (3 or 4; 0 for arguments that name
 * no family): slots_per_cell 3 | 4, source_method RDYHIP_SOURCE_*, hydrostatic_reconstruction 0 | 1.  A compile-time property
 * of the library, no device needed; persistent_grid of rdyhip_layout_info is this times the CU count unless a knob overrides it */
int32_t rdyhip_tiled_workgroups_per_cu(int32_t slots_per_cell, int32_t source_method, int32_t hydrostatic_reconstruction);

#ifdef __cplusplus
}
#endif
#endif /* RDYHIP_H */
