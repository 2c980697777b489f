/*
 * polystokes.h — C ABI of the MI355X-native PolyStokes hot path.
 *
 * Drop-in boundary for the reference's per-step reduced-viscosity Stokes solve
 * (panuelosj/polystokes).  Every entry point names the reference interface it
 * replaces (paths relative to the reference tree, file:line).
 *
 * The boundary is plain C: POD structs, raw pointers and sizes.  Host buffers
 * are owned by the caller (Houdini owns its SIM fields, exec/HDK_PolyStokes.C:235-246);
 * device memory is owned by the opaque ps_context and reused across steps.
 *
 * Array layout (all dense, x-fastest, i + dim0*(j + dim1*k)):
 *   cell   fields : nx   * ny   * nz
 *   faceX  fields : (nx+1)* ny   * nz        faceY: nx*(ny+1)*nz     faceZ: nx*ny*(nz+1)
 *   edgeXY fields : (nx+1)*(ny+1)* nz        edgeXZ: (nx+1)*ny*(nz+1) edgeYZ: nx*(ny+1)*(nz+1)
 * (exec/HDK_PolyStokesSolver.h:294-314 are the matching out-of-bounds predicates.)
 */
#ifndef POLYSTOKES_H
#define POLYSTOKES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Reduced model per tile: a compile-time choice, as in the reference (lib/include/units.h:9-18).  Default QUADRATIC_REGIONS,
 * 26 divergence-free quadratic DOFs; -DPS_AFFINE_REGIONS builds the AFFINE_REGIONS variant, 11 DOFs
 * (exec/HDK_PolyStokesSolver.cpp:2153-2184) -> libpolystokes_hip_affine.so, same ABI, ps_reduced_dof() tells which. */
#ifdef PS_AFFINE_REGIONS
#define PS_REDUCED_DOF 11
#else
#define PS_REDUCED_DOF 26
#endif

/* exec/HDK_PolyStokesSolver.h:61-70  enum class SolverResult */
enum ps_result {
    PS_UNSUPPORTED_SOLVER = -4,
    PS_INCOMPLETE = -3,
    PS_INVALID = -2,
    PS_FAILED = -1,
    PS_NOCONVERGE = 0,
    PS_SUCCESS = 1,
    PS_NOCHANGE = 2
};

/* exec/HDK_PolyStokesSolver.h:71-82  enum MaterialLabels */
enum ps_label {
    PS_UNASSIGNED = -1,
    PS_UNSOLVED = -2,
    PS_GENERICFLUID = -3,
    PS_ACTIVEFLUID = -4,
    PS_SOLID = -5,
    PS_REDUCED = -6,
    PS_UNVISITED = -7,
    PS_VISITED = -8,
    PS_BOUNDARY = -9
};

/* lib/include/units.h:76-94 */
enum ps_matrix_scheme { PS_PRESSURE_STRESS = 0 };
enum ps_solver_type { PS_PCG_MATRIX_VECTOR_PRODUCTS = 0, PS_EIGEN = 1 };
/* lib/include/units.h:47-53; DIAGONAL is the empty stub at
 * exec/HDK_PolyStokesSolver_Preconditioners.cpp:37-41 that BASELINE.json asks for (Jacobi-PCG). */
/* PS_PRE_CHEBYSHEV (extension): z = q(D^-1 A) D^-1 r with q the degree-(k-1) Chebyshev polynomial
 * of the interval [lmax/PS_CHEB_INTERVAL_RATIO, lmax], D = diag(A), k = ps_params.preconditionerDegree (default 4): k-1 operator applies per
 * CG iteration, the same smoother-as-preconditioner idea as the reference's abandoned GS designs
 * (lib/src/Preconditioner.cpp:30-158) on the live pressure-stress operator.  lmax = max(8.4, 1.25 x the estimate of 10 power iterations at setup).
 * PS_PRE_CHEBYSHEV_F32 (r06): the same polynomial with its INNER vectors — the iterates z_j and the face-row vector of the k-1 inner operator
 * applies — stored in single precision (half the bytes of those applies; every product, sum and recurrence, the residual r, the outer PCG
 * and its stop rule stay fp64).  The preconditioner only approximates an inverse, so its storage rounding (6e-8 relative per stored value)
 * perturbs the iteration count (<= +5 % accepted; equal on the scenes measured), not the solution: x converges to the same tolerance.  It runs
 * where the row-per-lane two-unit kernels run (coded stencil values, a value-set coded McInv, single domain, >= 8 chunks); elsewhere — fallback
 * formats, decompositions — the fp64 form above runs (array "chebInner32" says which). */
enum ps_preconditioner { PS_PRE_IDENTITY = 1, PS_PRE_DIAGONAL = 5, PS_PRE_CHEBYSHEV = 6, PS_PRE_CHEBYSHEV_F32 = 7 };
#define PS_CHEB_INTERVAL_RATIO 250.0   /* lmax / lmin of the Chebyshev interval: flat optimum 120..1000 on the 256^3 scenes (30: 5 % slower) */
/* order in which serialAssignFieldIndices walks a field (Classifier.cpp:1738-1770):
 * 0 = UT_VoxelArray order (16^3 voxel tiles, tile-linear, x-fastest inside), 1 = plain x-fastest. */
enum ps_index_order { PS_ORDER_VOXEL_TILES = 0, PS_ORDER_LINEAR = 1 };

/*
 * Node parameters: one member per entry of the reference's PRM template
 * (exec/HDK_PolyStokes.C:88-208, accessors exec/HDK_PolyStokes.h:23-43), same names.
 * Field-name string parms stay in the Houdini shim; they have no meaning below it.
 */
typedef struct ps_params {
    double mindensity;                  /* 1      clamp of a density field's face samples (ps_upload_density_field); the scalar density is not clamped */
    double maxdensity;                  /* 100000 */
    int32_t matrixSetup;                /* ps_matrix_scheme, 0 */
    int32_t solverType;                 /* ps_solver_type,   0 */
    int32_t doSolve;                    /* 1 */
    int32_t keepNonConvergedResults;    /* 1 */
    int32_t exportMatrices;             /* 0 */
    int32_t exportComponentMatrices;    /* 0 */
    int32_t exportStats;                /* 0 */
    int32_t useWarmStart;               /* 1 (built, then discarded: Solver.cpp:768) */
    double tolerance;                   /* 1e-3 */
    int32_t maxSolverIterations;        /* 5000 */
    int32_t useInputSurfaceWeights;     /* 1 (read, ignored by buildIntegrationWeightsAlt) */
    int32_t useInputCollisionWeights;   /* 1 (idem) */
    int32_t activeLiquidBoundaryLayerSize; /* 2 */
    int32_t activeSolidBoundaryLayerSize;  /* 2 */
    int32_t doReducedRegions;           /* 1 */
    int32_t doTile;                     /* 1 */
    int32_t tileSize;                   /* 16 */
    int32_t tilePadding;                /* 2 */
    /* --- extensions (not in the reference's template) --- */
    int32_t preconditioner;             /* ps_preconditioner, default PS_PRE_IDENTITY */
    int32_t indexOrder;                 /* ps_index_order, default PS_ORDER_VOXEL_TILES */
    int32_t negateCollision;            /* 1: `collision` is Houdini-convention (negative inside the
                                           solid) and is negated before the reference's
                                           computeSDFWeightsSampled(invert=false) call is applied
                                           (Solver.cpp:308-326); 0: use as given. default 1 */
    int32_t preconditionerDegree;       /* PS_PRE_CHEBYSHEV: terms k of the polynomial (k-1 applies); 0 = default 4 */
    const char* exportDataPrefix;       /* may be NULL */
} ps_params;

/* Inputs of solveGasSubclass (exec/HDK_PolyStokes.C:235-246, :319-320; Solver.cpp:39-44). */
typedef struct ps_fields_in {
    int32_t nx, ny, nz;
    double dx;                          /* max voxel size, HDK_PolyStokes.C:320 */
    double dt;                          /* timestep,       HDK_PolyStokes.C:319 */
    double orig[3];                     /* grid origin (debug output only, Solver.cpp:1134) */
    float density;                      /* constant liquid density, HDK_PolyStokes.C:298-304 (a field: ps_upload_density_field) */
    int32_t reserved;
    const float* vel[3];                /* face sampled velocity (in) */
    const float* surface;               /* cell, liquid SDF (<0 inside liquid) */
    const float* collision;             /* cell, solid SDF */
    const float* viscosity;             /* cell */
    const float* collisionvel[3];       /* face sampled */
    /* optional precomputed volume fractions, order:
     * 0 centerLiquid 1 faceXLiquid 2 faceYLiquid 3 faceZLiquid 4 edgeYZLiquid 5 edgeXZLiquid 6 edgeXYLiquid
     * 7..13 the same for Fluid.  All NULL -> the library samples the SDFs itself (Solver.cpp:238-326). */
    const float* weights[14];
} ps_fields_in;

/* Outputs (Solver.cpp:937-1028 velocity, Classifier.cpp:4-54 valid). */
typedef struct ps_fields_out {
    float* vel[3];                      /* may alias ps_fields_in.vel */
    float* valid[3];
} ps_fields_out;

/* exportStats(): dimData (27) + solveData (6), Solver.cpp:574-606, same order. */
typedef struct ps_stats {
    double dimData[27];
    double solveData[6];                /* error, iterations, solve CPU ms, solve wall ms, setup CPU ms, setup wall ms
                                         * (a mixed-precision solve, ps_set_solve_precision: the true error, the sum over its passes) */
    int32_t result;                     /* ps_result */
    int32_t usedBiCGStab;               /* CG hit maxit and the fallback ran (Solver.cpp:784-799) */
    double stage_ms[16];                /* device time per stage, see PS_STAGE_* */
} ps_stats;

enum ps_stage {
    PS_STAGE_WEIGHTS = 0, PS_STAGE_CLASSIFY = 1, PS_STAGE_REGIONS = 2, PS_STAGE_INDICES = 3,
    PS_STAGE_TILE_MATRICES = 4, PS_STAGE_BLOCKS = 5, PS_STAGE_ASSEMBLE = 6, PS_STAGE_PRECOND = 7,
    PS_STAGE_SOLVE = 8, PS_STAGE_RECOVER = 9, PS_STAGE_WRITEBACK = 10, PS_STAGE_COUNT = 11
};

typedef struct ps_context ps_context;

/* Library/ABI version and a loud availability check (0 devices -> error string). */
int32_t ps_abi_version(void);
int32_t ps_reduced_dof(void);                     /* REDUCED_DOF of this build: 26 (quadratic) or 11 (affine) */

/* Context = what `Solver mySolver(...)` owns for one call (HDK_PolyStokes.C:333-343), kept alive
 * across steps so device buffers are reused.  One context per GPU. */
ps_context* ps_context_create(int32_t device);
void ps_context_destroy(ps_context* ctx);
const char* ps_last_error(const ps_context* ctx); /* replaces addError strings, HDK_PolyStokes.C:251-314 */

void ps_params_default(ps_params* p);             /* defaults of HDK_PolyStokes.C:88-208 */

/* Host -> device copy of the SIM fields (no reference equivalent: Houdini fields are host memory). */
int32_t ps_upload_fields(ps_context* ctx, const ps_params* p, const ps_fields_in* in);

/* Variable density (extension; the reference's getLocalDensity hook, HDK_PolyStokesSolver.cpp:1915, HDK_PolyStokes.C:298-304).
 * density: cell field, nx*ny*nz, x-fastest, the grid of the last ps_upload_fields.  NULL drops it.
 * Call it after ps_upload_fields and before ps_setup_device / ps_step_device (on a slab / brick rank: after that rank's ps_upload_fields).
 * Every ps_upload_fields drops the field, so each step starts from the scalar ps_fields_in.density unless the field is passed again; a call
 * before any ps_upload_fields returns PS_INVALID.
 * The density of a face is the field sampled at the face centre with the viscosity's sampler (trilinear, clamped to the grid: an interior
 * x-face (i,j,k) gets rho[i-1,j,k] + (rho[i,j,k] - rho[i-1,j,k]) * 0.5f in fp32, a face on the grid boundary its one cell), then clamped to
 * [mindensity, maxdensity] of the ps_params of that upload (the scalar density is never clamped).  It replaces the scalar face by face in
 * McInv = 1 / (volume rho_f), the rhs u volume rho_f and Mc, and in each tile's Mr = sum_f rho_f C_f^T C_f (hence rhs_r = Mr c_fit); the fit,
 * K, uInv, recovery and export follow from these.  A field whose values all equal v runs the scalar path with density clamp(v), bit for bit.
 * Values <= 0 are legal (FLIP density is 0 in air; the clamp lifts them to mindensity): a caller who wants the liquid's densities at the free
 * surface extrapolates the field into the air first.  PS_INVALID (reason in ps_last_error): a NaN or infinite value, mindensity <= 0,
 * maxdensity < mindensity, or either non-finite; the field is then dropped.  Array "densityField" (int32): 1 if the last setup sampled a
 * non-constant field. */
int32_t ps_upload_density_field(ps_context* ctx, const float* density);

/* The whole hot path on device-resident inputs: buildIntegrationWeightsAlt ... solve ...
 * recoverVelocityFromPressureStress, applySolutionToVelocity (HDK_PolyStokes.C:344-583).
 * Returns ps_result. */
int32_t ps_step_device(ps_context* ctx, ps_stats* stats);

/* Setup only (everything before solve(), HDK_PolyStokes.C:344-476); used by tests and exports. */
int32_t ps_setup_device(ps_context* ctx, ps_stats* stats);
/* solve() + recover + write-back on an already set-up context (HDK_PolyStokes.C:518-583). */
int32_t ps_solve_device(ps_context* ctx, ps_stats* stats);

/* UT_Interrupt equivalent (the reference polls boss->opInterrupt() in its sweeps, e.g. Classifier.cpp:73,386): the
 * callback is polled between batches of CG iterations; a non-zero return stops the solve, which then reports
 * PS_INCOMPLETE and leaves the velocity untouched.  Pass NULL to clear. */
typedef int32_t (*ps_interrupt_fn)(void* user);
int32_t ps_set_interrupt(ps_context* ctx, ps_interrupt_fn cb, void* user);

/* Device -> host copy of vel / valid. */
int32_t ps_download_fields(ps_context* ctx, ps_fields_out* out);

/* Warm start (extension; the reference builds a guess under useWarmStart and then solves from zero, HDK_PolyStokesSolver.cpp:768).
 * PS_WARM_PREVIOUS_STEP: a single-domain PCG step whose velocity is written back (doSolve, not interrupted, SUCCESS or NOCONVERGE with
 * keepNonConvergedResults) keeps its [p; tau] on the device as fp32 grids, and the next PCG solve on the same (nx, ny, nz, dx) starts from
 * them (r0 = b - A x0, pcg.h:284): a DOF without a value in the previous step starts at 0.  The BiCGStab fallback still restarts from zero,
 * the EIGEN path keeps its guessVector, decompositions start cold.  Every call drops the carried solution; a mode other than these two
 * returns PS_INVALID.  Arrays "warmStartUsed" (int32) and "warmStartVector" (fp64, reference numbering: the x0 of the last PCG solve). */
enum ps_warm_start { PS_WARM_NONE = 0, PS_WARM_PREVIOUS_STEP = 1 };
int32_t ps_set_warm_start(ps_context* ctx, int32_t mode);

/* The last solve's [p; tau] as dense x-fastest grids: pressure and the stress diagonal txx / tyy / tzz on the cell grid, the off-diagonal
 * stresses tyz / txz / txy on the edgeYZ / edgeXZ / edgeXY grids (the layouts at the top of this file).  Each value is the solution vector's
 * entry rounded to fp32; a sample without that DOF reads 0.  Any pointer may be NULL.  Single domain only; an error before the first solve
 * after a setup.  (The reference fetches its `pressure` field, exec/HDK_PolyStokes.C:238, but never writes it.) */
typedef struct ps_solution_out {
    float* pressure;
    float* tauDiag[3];                  /* txx, tyy, tzz */
    float* tauEdge[3];                  /* tyz, txz, txy */
} ps_solution_out;
int32_t ps_download_solution_fields(ps_context* ctx, const ps_solution_out* out);

/* Surface tension (extension; neither the reference node nor its solver has one).  A context setting like ps_set_warm_start: it persists
 * across ps_upload_fields and applies to every later setup, so a polystokes_step caller sets it once.  sigma = 0 (the default) is off and
 * launches exactly the kernels of a context that never made the call.  sigma > 0 gives the non-liquid part of every cell next to a face
 * of the system the pressure sigma * kappa_c instead of 0 (a ghost-fluid pressure jump): with the stencil coefficient
 * gradSign * wF_f * liquidW_c / dx of face f and cell c, the ghost coefficient g(f,c) is gradSign * wF_f * (1 - liquidW_c) / dx for a cell with
 * a pressure DOF or inside a reduced tile, gradSign * wF_f / dx for any other cell of the grid, and the step adds the impulse
 * -dt * sum_c g(f,c) sigma kappa_c to the active rhs of f ("activeRHSVector"), or C_f^T times it to its tile's rhs ("reducedRHSVector").
 * b, the recovered velocity, the exports, the EIGEN path and ps_solve_exported_system follow from these two vectors.
 * kappa = div(grad phi / |grad phi|) of the uploaded `surface` SDF in fp64 (central differences, the mixed terms on the 4-point diagonal
 * stencil, indices clamped at the grid border; 0 where |grad phi| < 1e-6 / dx), stored in fp32 and sampled trilinearly (clamped to the grid)
 * at the closest interface point x_c - phi_c grad phi_c / |grad phi_c|^2, the step capped at 4 cells (a solid cell deep under the liquid
 * reads the level set 4 cells toward the surface), then clamped to [-1/dx, 1/dx]: that is kappa_c.  Every read lies within 7 cells of a face.
 * Orthogonal to the density field, warm start, the Chebyshev preconditioners and the BiCGStab fallback; slab and brick ranks compute it on
 * their own grid (the halo blocks cover the stencil).  PS_INVALID (reason in ps_last_error, the previous setting kept): sigma negative or
 * not finite.  Arrays: "surfaceTension" (fp64, 1: the sigma of the last setup), "surfaceCurvature" (fp32 cell grid: the kappa_c the last
 * setup used; only with sigma > 0), "surfaceTensionReducedFaces" (int32: reduced faces that received an impulse; only with sigma > 0). */
int32_t ps_set_surface_tension(ps_context* ctx, double sigma);

/* Free-surface fields (extension): the ghost pressure on the non-liquid side of the free surface as a per-cell quantity
 *   q_c = sigma_c * kappa_c + P_c
 * instead of the one sigma of ps_set_surface_tension and an ambient pressure of 0.
 * sigma: cell field of surface-tension coefficients, nx*ny*nz, x-fastest; NULL: the scalar of ps_set_surface_tension everywhere.
 * pressure: cell field of the ambient (air-side) pressure, same grid; NULL: 0.
 * The lifetime is the density field's: the fields belong to the grid of the last ps_upload_fields / ps_upload_fields_device; call after that
 * upload and before ps_setup_device / ps_step_device (on a slab / brick rank: after that rank's own upload, with the rank's local grid);
 * a call before any upload returns PS_INVALID; every field upload drops both fields.  A call replaces both members: a NULL member means
 * "not present", not "keep"; f == NULL or both members NULL drops them.  polystokes_step and ps_step_device_fields carry no such fields
 * (a caller uses upload + this call + ps_step_device + download); the Picard passes of ps_set_rheology re-run the setup without an upload
 * in between, so the fields stay for every pass.
 * Arithmetic (fp64 from the fp32 inputs): s_c = (double)sigma[c], or the scalar setting without a sigma field; kappa_c = the fp32 value of
 * "surfaceCurvature" (ps_set_surface_tension), computed when the sigma field is present or the scalar is > 0 and absent from q otherwise;
 * P_c = (double)pressure[c] or 0.  For a face f with wF != 0 the sum t starts at 0 and visits the lower cell (sign -1), then the upper
 * (sign +1), cells inside the grid only: ghost = 1 - liquidW_c for a cell with an active label or PS_REDUCED, else 1; a cell with ghost == 0
 * is skipped; t += sign * wF * ghost * invDx * q_c, left to right.  With t != 0 an active face gets rhsA[row] -= dt * t and a reduced face
 * C_f^T (-dt * t) into its tile's rhs; b, the recovery, the exports, the EIGEN path and ps_solve_exported_system follow from those two
 * vectors.  With no field present the setup runs exactly the kernels and arguments of ps_set_surface_tension alone.
 * sigma is sampled at the cell, not at the closest interface point; a varying sigma adds no Marangoni (tangential) stress; contact angles
 * are ps_set_contact_angle's (below); P is the caller's (no bubble model derives it from pocket volumes).
 * PS_INVALID (reason in ps_last_error, both fields dropped): "sigma: non-finite or negative value at cell N" (checked first; -0 is not
 * negative), "pressure: non-finite value at cell N", N the smallest such index in x-fastest numbering.  While present the fields cost two fp32 cell grids and,
 * from the next setup on, one fp64 cell grid; a drop releases them.
 * Arrays: "surfaceFields" (int32, 1: bit 0 / 1 = the last setup used the sigma / pressure field), "surfaceGhostPressure" (fp64 cell grid:
 * q_c; only when "surfaceFields" != 0), "surfaceCurvature" (also when only the sigma field asked for the curvature),
 * "surfaceTensionReducedFaces" (also when "surfaceFields" != 0), "surfaceTension" (the scalar setting, as before). */
typedef struct ps_surface_fields {
    const float* sigma;      /* cell field nx*ny*nz, x-fastest; NULL: the scalar of ps_set_surface_tension */
    const float* pressure;   /* cell field nx*ny*nz, x-fastest; NULL: 0 */
} ps_surface_fields;
int32_t ps_upload_surface_fields(ps_context* ctx, const ps_surface_fields* f);

/* Contact angles (extension): before the curvature of ps_set_surface_tension is taken, the liquid SDF inside the solid is rewritten so
 * that its slope along the wall normal is cos(theta); at the wall the level set then meets the solid at theta, and where the liquid's
 * current angle differs the curvature at the contact line changes and drives the line towards equilibrium.  Only the curvature reads the
 * rewritten field phi' ("surfaceWetted"): the stencil of kappa and the closest-point gradient of kappa_c read phi' wherever they read
 * `surface` otherwise; weights, classification, numbering, the operator and every other output are untouched.
 * ps_set_contact_angle is a context setting like ps_set_surface_tension: it persists across uploads and is read by every later setup.
 * degrees < 0 (the default: -1) is off; 0..180 is theta, measured inside the liquid.  The cosine is computed once on the host as
 * cos(degrees * (pi / 180)), and is exactly 0 for degrees == 90 (array "contactCosine").  PS_INVALID for a NaN, an infinity or a value
 * above 180 (reason "contact angle outside 0..180", the previous setting kept).
 * ps_upload_contact_cosine_field: one fp32 value per cell, nx*ny*nz, x-fastest: the cos(theta) of the solid that cell belongs to (painted
 * into the solid cells, like collider ids).  The lifetime and call order are the density field's: after an upload and before the setup,
 * dropped by every field upload, kept across the Picard passes, PS_INVALID before any upload; NULL drops it.  PS_INVALID with the field
 * dropped: "contact cosine: value outside [-1, 1] at cell N" (a NaN counts), N the smallest such index in x-fastest numbering whatever
 * the layout.  While present the field overrides the scalar cell by cell and turns the rule on when the scalar is off.  polystokes_step
 * and ps_step_device_fields carry no such field: the scalar setting applies to them.
 * The rule runs in a setup only when that setup computes the curvature (sigma > 0 or a sigma field) and the angle or the cosine field is
 * set; otherwise nothing is launched and nothing is allocated, and a context that never made these calls launches what it always did.
 * All arithmetic is fp64 from the fp32 inputs, unfused, in the order written:
 *   D_c = -collision[c] with negateCollision = 1, +collision[c] with 0 (the solid depth, positive inside the solid); phi^0 = `surface`;
 *   cos_c = (double)field[c], or the scalar's cosine without a field.
 *   U = { c : D_c > 0 and (double)D_c <= 6.0 * dx };  G_a(c) = (D[c + e_a] - D[c - e_a]) * 0.5, indices clamped to the grid;
 *   g(c) = sqrt(G_x*G_x + G_y*G_y + G_z*G_z), summed left to right.
 *   Sweep m = 1 .. PS_CONTACT_ANGLE_SWEEPS (Jacobi: it reads only phi^(m-1)).  c outside U: phi^m_c = phi^(m-1)_c.  c in U: from N = 0,
 *   W = 0 visit the axes x, y, z: the upwind cell is c - e_a for G_a > 0 and c + e_a for G_a < 0; an axis with G_a == 0, or whose upwind
 *   cell lies outside the grid, contributes nothing; otherwise N += |G_a| * (double)phi^(m-1)[up], W += |G_a|.  W == 0: the cell keeps
 *   its value; otherwise phi^m_c = (float)((N - (dx * cos_c) * g) / W).
 *   phi' = phi^PS_CONTACT_ANGLE_SWEEPS.
 * Slab and brick ranks run the rule on their own grid: a value that reaches an owned face depends on cells at most 7 + 6 + 1 layers
 * away, inside the 16-layer halo block.  No hysteresis or dynamic angle; the weights near walls do not change.
 * Memory: from the first setup that runs the rule the context holds two fp32 cell grids (phi' and the other Jacobi iterate), one flag byte
 * per 16x4x4 block of cells and a counter, plus one fp32 cell grid for the cosine field while present.  A setup that does not run the rule
 * drops them, and so does ps_set_contact_angle(ctx, -1) with no field present, which releases them at once; ps_memory_stats entry 2 is 0
 * after each of the three calls.
 * Arrays: "contactAngle" (fp64, 1: the degrees the last setup used; -1 when it used none or only the field) and, only when the last
 * setup ran the rule, "contactCosine" (fp64, 1: the scalar's cosine; 0 with the scalar off), "contactField" (int32, 1: 1 if the field
 * was used), "contactCells" (int32, 1: |U|), "surfaceWetted" (fp32 cell grid: phi'). */
#define PS_CONTACT_ANGLE_SWEEPS 6
int32_t ps_set_contact_angle(ps_context* ctx, double degrees);              /* < 0: off (default); 0..180 */
int32_t ps_upload_contact_cosine_field(ps_context* ctx, const float* cosTheta);   /* cell field nx*ny*nz, x-fastest; NULL drops it */

/* Solid boundary condition (extension; the reference node's colliders are all no-slip).  A context setting like ps_set_surface_tension: it
 * persists across ps_upload_fields and is read by every later setup.  PS_SOLID_NO_SLIP (the default) launches exactly the kernels of a
 * context that never made the call.  PS_SOLID_FREE_SLIP zeroes the shear stress tau_e of every active edge whose fluid weight is below 1
 * (an edge cut by a solid): its entries in S and St (face rows, skin rows included) hold the value 0, its rhs is 0 and its uInv is kept,
 * so the system row of tau_e reads uInv tau_e = 0.  The zeros keep no-slip's sparsity pattern (exports list them as explicit zeros).
 * Pressure and centre-stress columns, their collisionvel rhs terms (the wall's normal constraint), labels, numbering and dimData are
 * those of no-slip.  On axis-aligned walls that is free slip; on slanted walls the centre stresses still carry some tangential traction
 * (the usual MAC approximation).  Slab and brick ranks apply the rule on their own grid.  PS_INVALID (reason in ps_last_error, the previous setting kept): another mode.
 * Arrays: "solidBoundary" (int32, 1: the mode of the last setup), "solidSlipEdges" (int32, 1: the edges whose coupling the last setup
 * dropped; only in free-slip mode). */
enum ps_solid_boundary { PS_SOLID_NO_SLIP = 0, PS_SOLID_FREE_SLIP = 1 };
int32_t ps_set_solid_boundary(ps_context* ctx, int32_t mode);

/* Non-Newtonian viscosity (extension; the reference node takes the viscosity field as a fixed input).  A context setting like
 * ps_set_solid_boundary: it persists across ps_upload_fields and is read by every later setup.  PS_RHEOLOGY_NEWTONIAN (the default; the
 * other members are then ignored) launches exactly the kernels of a context that never made the call.  PS_RHEOLOGY_HERSCHEL_BULKLEY makes
 * the uploaded `viscosity` field the consistency K of the law (a scalar viscosity is a constant field) and replaces it, for the setup, by
 * mu_c computed on the device after the final labels exist.  A face sample is used iff its label is neither UNSOLVED nor UNASSIGNED (the
 * `valid` output of ps_download_fields).  For cell c and axes a != b, in fp64 from the fp32 inputs:
 *   D_aa(c) = (u_a[c+e_a] - u_a[c]) / dx if both a-faces of c are used, else 0;
 *   G_ab(c) = du_a/dx_b = the mean, over those of the two a-faces f in {c, c+e_a} for which it exists, of (u_a[f+e_b] - u_a[f-e_b]) / (2 dx);
 *             it exists when both samples lie inside the a-face grid and are used; G_ab(c) = 0 when it exists for neither face;
 *   D_ab = (G_ab + G_ba) / 2,  gammaDot_c = sqrt(2 sum_a D_aa^2 + 4 sum_{a<b} D_ab^2);
 *   s = max(gammaDot_c, minShearRate),  mu_c = min(max(K_c s^(n-1) + yieldStress / s, minViscosity), maxViscosity)  (n = flowIndex; with
 *   n == 1 the power is skipped, so K_c * 1 is exact), stored as fp32.  The uploaded field is kept (the passes need K).
 * The setup samples mu like an uploaded field (trilinear, no constant-field shortcut); the value and diagonal formats follow from it.
 * The velocity read is the uploaded `vel` for the first solve of a step.  With passes = k > 0, ps_step_device and polystokes_step repeat
 * k times on a single domain: a full setup that reads the last pass's output velocity, a solve started from the last pass's [p; tau]
 * (through the warm-start grids; the first solve honours ps_set_warm_start, PS_WARM_PREVIOUS_STEP carries the last pass's solution),
 * recovery and write-back.  The rhs always comes from the uploaded `vel`.  Stats hold the last pass's result, error and iterations; the
 * time entries and stage_ms are summed over the passes.  A pass whose result is neither SUCCESS nor a kept NOCONVERGE ends the step with
 * that result (an interrupt: PS_INCOMPLETE, the output velocity equal to the input).  ps_setup_device / ps_solve_device are single-shot
 * (passes ignored).  Slab and brick ranks compute mu on their own grid (every read lies within 3 cells of an owned face, inside the halo
 * block); passes > 0 on a decomposition makes the step fail on every rank (PS_FAILED, "rheology passes need a single domain").
 * Orthogonal to surface tension, free-slip solids, the density field and warm start.  PS_INVALID (reason in ps_last_error, the previous
 * setting kept): r null, an unknown model, passes outside 0..8, flowIndex outside (0, 4], yieldStress negative, minShearRate not positive,
 * not 0 < minViscosity <= maxViscosity, or a value not finite.
 * Arrays: "rheologyModel" (int32, 1: the model of the last setup), "rheologyStrainRate" (fp32 cell grid: gammaDot_c of the last setup),
 * "rheologyViscosity" (fp32 cell grid: the mu_c the last setup used), "rheologyIterations" (int32, one per solve of the last step: the
 * PCG iterations of each pass); the last three only with the model on. */
enum ps_rheology_model { PS_RHEOLOGY_NEWTONIAN = 0, PS_RHEOLOGY_HERSCHEL_BULKLEY = 1 };
typedef struct ps_rheology {
    int32_t model;          /* ps_rheology_model */
    int32_t passes;         /* extra Picard passes of ps_step_device / polystokes_step, 0..8 */
    double flowIndex;       /* n, 0 < n <= 4 */
    double yieldStress;     /* tau_y >= 0 */
    double minShearRate;    /* regularisation floor of the shear rate, > 0 */
    double minViscosity;    /* clamp, 0 < minViscosity <= maxViscosity, both finite */
    double maxViscosity;
} ps_rheology;
int32_t ps_set_rheology(ps_context* ctx, const ps_rheology* r);

/* Mixed-precision PCG (extension; the reference solves in fp64 throughout).  A context setting like ps_set_solid_boundary: it persists across
 * ps_upload_fields and is read by every later PCG solve.  PS_PRECISION_FP64 (the default) launches exactly the kernels of a context that never
 * made the call.  PS_PRECISION_MIXED keeps the solution x in fp64 and runs the PCG in passes on fp32 vectors: a pass solves A d = r with
 * r = b - A x formed in fp64 by the fp64 operator, and stores the correction d, the direction p, the residual r, A p and the face-row
 * vector t of the operator as fp32; every product, every partial sum and every scalar of the recurrence stays fp64, and r.r, r.z, d.d are
 * formed from the values as stored.  A pass ends when its recurrence meets the stop rule min(r.r, r.r / x.x) < tolerance^2 (pcg.h:319-325) or
 * when r.r has fallen to (1e-4)^2 of the true r.r it started from (fp32 carries 2^-24: about three digits are left for drift); then
 * x += d in fp64, r = b - A x is formed again, and the rule is evaluated on these true fp64 values: that evaluation alone decides SUCCESS.
 * x.x in a pass: the first pass of a cold solve has x = d and uses d.d as the fp64 solve does; any other pass uses x.x of the x it started
 * from (the evaluation at its end corrects it).  maxSolverIterations is one budget over all passes; when it runs out the fp64 BiCGStab
 * fallback runs from zero as in the fp64 solve.  At most 8 passes; a pass whose true ||r|| is not below half of the one it started from has
 * reached the floor of fp32, and the solve continues as the fp64 PCG from the current x.  Interrupts are polled between batches as in the
 * fp64 solve (PS_INCOMPLETE, velocity untouched).  A carried x0 (ps_set_warm_start, a Picard pass of ps_set_rheology) is a first pass with
 * x != 0.  ps_stats.solveData[0] is the true value of the last evaluation, solveData[1] the sum of the passes' iterations, each pass
 * counted by the iterations it ran (the fp64 solve reports the index of the iteration that met the rule, one less).
 * It runs in a single domain, with PS_PCG_MATRIX_VECTOR_PRODUCTS, preconditioner identity or Jacobi, on systems whose products run the
 * two-units-per-wave row-per-lane kernels (coded stencil values, 16-bit columns, at least 8 workgroups; the stress diagonal and the face mass
 * either value-set coded or fp64 fields), in both step forms.  Everywhere else — the Chebyshev preconditioners, solverType EIGEN, the other
 * stream formats, slab and brick ranks, in-process groups, ps_solve_exported_system — the setting is ignored and the solve is the fp64 one,
 * launch for launch.  The fp32 vectors (3 or 4 x 4 B per DOF, 4 B per face row) are allocated by the first mixed solve and released by
 * ps_set_solve_precision(ctx, PS_PRECISION_FP64).  PS_INVALID (reason in ps_last_error, the previous setting kept): another mode.
 * Arrays: "solvePrecisionUsed" (int32, 1: 0 = the last PCG solve ran in fp64, 1 = mixed throughout, 2 = started mixed and finished in
 * fp64), "solvePassIterations" (int32, one per fp32 pass; only when used != 0), "solveTrueResidual" (fp64, 1: sqrt(min(r.r, r.r / x.x)) of
 * r = b - A x in fp64 at the end of the last pass; only when used != 0). */
enum ps_solve_precision { PS_PRECISION_FP64 = 0, PS_PRECISION_MIXED = 1 };
int32_t ps_set_solve_precision(ps_context* ctx, int32_t mode);

/* Velocity extrapolation (extension; in Houdini the DOP network extrapolates after the node, a device-resident caller has nothing that does).
 * A context setting like ps_set_solid_boundary: it persists across ps_upload_fields and is read by every later step.  layers = 0 (the default)
 * is off and launches exactly the kernels of a context that never made the call.  layers = n > 0 carries the written velocity n faces deep
 * into the faces `valid` marks 0, on the device, right after the write-back.  Per axis a, on the face grid of that axis (the extents at the top
 * of this file), independently of the other two:
 *   L[f] = 0 where valid[f] == 1 (SOLID faces included: they hold the collision velocity and are sources like any valid face), -1 elsewhere;
 *   for k = 1 .. n: every face with L == -1 of whose six grid neighbours (-x, +x, -y, +y, -z, +z, inside the same face grid) at least one has
 *   0 <= L < k takes the fp32 rounding of sum / count — sum the fp64 sum of those neighbours' fp32 values in that order, starting from 0,
 *   count their number as a double — and L = k.  Neighbours assigned in the same sweep do not count (a Jacobi sweep: the result does not depend
 *   on the traversal order).
 * Faces no sweep reaches keep the input velocity, as without the setting; `valid` is not changed.
 * It runs after the write-back of every step whose velocity is written — SUCCESS, NOCONVERGE with keepNonConvergedResults, a doSolve = 0
 * step — in ps_step_device, ps_solve_device, polystokes_step and ps_step_device_fields, and every download returns the extrapolated
 * velocity.  A step that leaves the velocity alone (interrupted, failed, an unsupported solver, NOCONVERGE without keepNonConvergedResults) runs
 * none of it: the output is the input, bit for bit.  With the Picard passes of ps_set_rheology it runs after every pass's write-back; the next
 * pass reads used faces only, which no sweep changes, so the result is the extrapolation of the last pass's output.
 * Single domain only: slab and brick ranks, in-process groups and TCP / RCCL ranks ignore the setting (a rank's halo faces are not solved
 * values; the sweeps would need an exchange of their own).  The time is part of stage_ms[PS_STAGE_WRITEBACK].
 * Memory: one byte per face for L, (nx+1) ny nz + nx (ny+1) nz + nx ny (nz+1) bytes, plus PS_EXTRAPOLATION_MAX_LAYERS int32 counters (256 bytes):
 * allocated by the first step that runs a layer, released by ps_set_velocity_extrapolation(ctx, 0) (the layer and count arrays go with them).
 * PS_INVALID (reason "layers outside 0..64" in ps_last_error, the previous setting kept): layers < 0 or > PS_EXTRAPOLATION_MAX_LAYERS.
 * Arrays: "velocityExtrapolation" (int32, 1: the layers the last step ran; 0 when off, ignored, or the velocity was not written),
 * "extrapolationLayerX" / "extrapolationLayerY" / "extrapolationLayerZ" (int8, one per face: L) and "extrapolationCounts" (int32, one per
 * sweep: the faces it assigned, the three axes together); the last four only when the last step ran at least one layer. */
#define PS_EXTRAPOLATION_MAX_LAYERS 64
int32_t ps_set_velocity_extrapolation(ps_context* ctx, int32_t layers);   /* 0 = off (default) ... PS_EXTRAPOLATION_MAX_LAYERS */

/* Collider loads (extension; the reference returns the liquid's velocity and nothing of what the liquid does to the solids): the force and
 * the torque of the liquid on each collider, integrated on the device from the solve's own [p; tau] right after the write-back.
 * A context setting like ps_set_velocity_extrapolation: it persists across ps_upload_fields and is read by every later step.  count = 0 (the
 * default) is off and launches exactly the kernels of a context that never made the call.  count = n in 1..PS_COLLIDER_MAX computes the
 * loads of colliders 0..n-1; pivots: 3 * count doubles (x y z per collider) copied by the call, the points the torques are taken about;
 * NULL: ps_fields_in.orig of the step's upload for every collider.
 * Definition.  P, Txx, Tyy, Tzz (cell grid) and Tyz, Txz, Txy (the YZ, XZ, XY edge grids) are the grids of ps_download_solution_fields: the
 * solution entry rounded to fp32 and widened to double, 0 where the sample has no DOF — a caller can reproduce the loads from public
 * outputs.  wF_a = the array "faceXFluidWeights" / Y / Z of axis a, wL = the "...LiquidWeights" array of the sample's own grid (fp32, widened).
 * All arithmetic is fp64, unfused, in the order written; dx2 = dx * dx; e_a = one step along axis a.  Force on the solids along axis a:
 *   cell c, pressure:        d = wF_a[c + e_a] - wF_a[c];  f = ((-dx2 * wL[c]) * P[c]) * d
 *   cell c, normal stress:   same d;                       f = (( dx2 * wL[c]) * T_aa[c]) * d
 *     both at the cell centre r = orig + (i + 0.5, j + 0.5, k + 0.5) * dx  (each coordinate orig_m + ((double)index + 0.5) * dx);
 *   edge e of the ab edge grid (a != b), shear on axis a:  d = wF_a[e] - wF_a[e - e_b];  f = ((dx2 * wL[e]) * T_ab[e]) * d
 *     at the edge's position: the coordinates of a and b on grid lines (orig_m + (double)index * dx), the third at index + 0.5; the term
 *     is skipped when either face lies outside the a-face grid.  An edge gives up to two terms, one on axis a and one on axis b.
 * A term whose solution value is 0 or whose d is 0 is no term (not counted).  This is sigma_ab d_b(chi_fluid) summed over the grid; with the
 * wL factor it is the adjoint of the stencil coefficient wF * wL / dx of the system's blocks: the impulse the recovery u = u* - dt McInv C x
 * takes from the liquid, -dt dx^3 C x, arrives at the solids.  A grid border that liquid reaches without a solid counts as whatever wF says
 * there (wF differences across the outermost cells are terms like any other).
 * Torque of a term about the pivot o: with arm = r - o, a1 = (a + 1) % 3, a2 = (a + 2) % 3:  T[a1] += arm[a2] * f,  T[a2] += -(arm[a1] * f).
 * Attribution.  Without an id field every term belongs to collider 0.  With one (ps_upload_collider_ids: int32 per cell) a cell term takes
 * id[c]; an edge term takes the id of that cell, among the up to four cells around the edge that lie inside the grid, whose
 * "centerFluidWeights" is smallest, ties to the lowest x-fastest cell index.  An id < 0 or >= count drops the term; dropped terms are counted.
 * Per collider k the step leaves F_k, T_k, the number of its terms, and the scales A_k[a] = the sum of |f| over its terms of axis a and
 * B_k[m] = the sum of the absolute values of the addends of T_k[m] (|arm| |f|, component by component): any order of summation keeps
 * |F - F_exact| <= (terms_k + 8) 2^-53 A_k and the same with B_k for the torque.  The sums are formed in a fixed order (no floating-point
 * atomics): the result of a step is bitwise reproducible run to run and context to context.
 * It runs after the write-back, before the extrapolation of ps_set_velocity_extrapolation (which touches nothing the loads read), of every
 * step that solved and whose velocity is written — SUCCESS, NOCONVERGE with keepNonConvergedResults, after the BiCGStab fallback too — in
 * ps_step_device, ps_solve_device, polystokes_step and ps_step_device_fields, with both solverTypes and mixed precision; with the Picard
 * passes of ps_set_rheology after every pass (the last pass's values stand).  A step that leaves the velocity alone and a doSolve = 0 step
 * compute nothing.  Single domain only: slab and brick ranks, in-process groups and TCP / RCCL ranks ignore the setting ("colliderLoads" = 0;
 * loads there need a reduction over ranks and a rule for the halo blocks).  The loads read only: velocity, valid, stats and iterations of a
 * step are those of a step without the setting.  The time is part of stage_ms[PS_STAGE_WRITEBACK].
 * Memory: with W = 4 * min(1024, ceil(m / 256)) workgroups, m the samples of the largest of the four grids, W * (100 * count + 12) bytes
 * of partial sums plus 172 * count + 4 bytes of results and pivots: allocated by the first step that computes loads, released by
 * ps_set_collider_loads with count = 0 (the four result arrays go with them).  The id field costs one int32 cell grid while present.
 * ps_set_collider_loads: PS_INVALID (reason in ps_last_error, the previous setting kept) for loads == NULL, "count outside 0..64", or a pivot
 * that is not finite.  A successful call discards the loads of earlier steps (the getters then fail until the next step computes them).
 * ps_upload_collider_ids: a cell field with the lifetime and call order of the density field: it belongs to the grid of the last
 * ps_upload_fields / ps_upload_fields_device, follows that upload, and is dropped by every field upload; NULL drops it; a call before any
 * upload returns PS_INVALID.  The Picard passes keep it.  ps_upload_collider_ids_device takes it from device memory in either layout and
 * obeys the pointer refusals of the other ps_*_device calls (below); it returns with the input consumed.
 * ps_get_collider_loads writes Fx Fy Fz Tx Ty Tz per collider into out (host memory, out_len doubles); PS_FAILED (reason in ps_last_error)
 * when the last step computed no loads (none since the context was created, the setting was changed or fields were uploaded; a step that
 * was interrupted, dropped its result or ran on a decomposition) and when out_len < 6 * count.  ps_get_collider_loads_device writes the
 * same values into device memory of the context's device (8-byte aligned, len doubles), ordered against `stream` like a download, without
 * synchronising the host; PS_INVALID for the pointer refusals, PS_FAILED as above.
 * Arrays: "colliderLoads" (int32, 1: the count of the last step; 0 when off, ignored, or the step computed none), "colliderForce" and
 * "colliderTorque" (fp64, 3 * count), "colliderLoadTerms" (int32, count + 1: terms per collider, then the dropped terms) and
 * "colliderLoadScale" (fp64, 6 * count: A_k then B_k per collider); the last four only when the last step computed loads. */
#define PS_COLLIDER_MAX 64
typedef struct ps_collider_loads {
    int32_t count;          /* 0: off (the default); 1..PS_COLLIDER_MAX colliders */
    const double* pivots;   /* 3 * count doubles, copied by the call; NULL: ps_fields_in.orig for every collider */
} ps_collider_loads;
int32_t ps_set_collider_loads(ps_context* ctx, const ps_collider_loads* loads);
int32_t ps_upload_collider_ids(ps_context* ctx, const int32_t* ids);      /* cell field nx*ny*nz, x-fastest; NULL drops it */
int32_t ps_get_collider_loads(ps_context* ctx, double* out, int64_t out_len);

/* Collider motions (extension; the input half of rigid-collider coupling, the loads above being the output half): the rigid-body velocity
 * v + w x (r - o) of the collider a face belongs to, painted on the device into the context's collisionvel grids, from the collision SDF and
 * the id field the context already holds.  The integration of the bodies stays with the caller: loads out, its few lines of body dynamics,
 * motions in, with no host synchronisation in the device forms.
 * Call order and lifetime.  The call follows ps_upload_fields / ps_upload_fields_device, and ps_upload_collider_ids if there is one; it
 * precedes the setup.  It writes into the context's own collisionvel buffers at once, on the context's stream: what it wrote lives exactly as
 * long as that upload's collisionvel.  Every field upload replaces it; a setup, solve or step and the Picard passes of ps_set_rheology keep
 * it.  A second call paints over what is there, and faces it leaves alone keep what they hold.  Ids uploaded after a call do not repaint.
 * polystokes_step and ps_step_device_fields upload and therefore never see it: a caller uses upload + ids + ps_paint_collider_velocities +
 * ps_step_device + download.  It is not a context setting and has no "off".  A context that never makes the call launches exactly the
 * kernels it launched without it.
 * The rule.  All arithmetic is fp64 from the fp32 / fp64 inputs, unfused, in the order written.  For the face of axis a at indices
 * (i0, i1, i2) of the a-face grid, n_a the cells along a:
 *   adjacent cells:  the lower cell L has index i_a - 1 along a and exists iff i_a >= 1; the upper cell U has index i_a and exists iff
 *                    i_a <= n_a - 1; the other two indices are the face's;
 *   solid depth:     D_c = -collision[c] with negateCollision = 1, +collision[c] with negateCollision = 0 (the ps_params of that upload;
 *                    the D of the contact angles);
 *   chosen cell:     the only existing one; with both existing, U if D_U > D_L, else L — the more solid cell, ties and NaN to the lower;
 *   id:              k = ids[chosen cell], or 0 without an id field, as the loads do;
 *   left alone:      k < 0 or k >= count: the face keeps its value and is counted in slot count; the nine values of collider k not all
 *                    finite (the device form only; the host form refuses such a table): it keeps its value and is counted in slot count + 1;
 *   painted value:   r_m = orig_m + (double)i_m * dx for m == a and orig_m + ((double)i_m + 0.5) * dx for the other two (the positions the
 *                    loads use), arm_m = r_m - o_m, a1 = (a + 1) % 3, a2 = (a + 2) % 3:
 *                    collisionvel[a][face] = (float)( v[a] + (w[a1] * arm[a2] - w[a2] * arm[a1]) );  the face is counted in slot k.
 *                    (arm[a] does not occur: a rigid motion's component a is constant along a, so one collider's paint is divergence-free.)
 * The more solid cell decides because a face between a solid cell and a liquid cell is the solid's face: the write-back gives SOLID faces the
 * collision velocity, and the solid-boundary terms of the right-hand side read it at faces a solid cuts.  The counts are integers: the
 * result is bitwise reproducible and independent of the traversal (a collider's count wraps beyond 2^31 - 1 faces).
 * ps_paint_collider_velocities copies the table before it returns.  ps_paint_collider_velocities_device reads 9 * count doubles of device
 * memory of the context's device (8-byte aligned) behind what `stream` holds, makes `stream` wait until it has read them, and does not
 * synchronise the host — except a call whose count differs from the previous call's since the same upload, which releases the previous
 * table and counters first.
 * Refusals (PS_INVALID, reason in ps_last_error, nothing written): a call before any upload; motions == NULL or motion == NULL;
 * "count outside 1..64"; host form: "motion of collider N is not finite", N the smallest such collider; device form: the pointer refusals of the other
 * ps_*_device calls (below) — a pointer that is not 8-byte aligned, memory that is not device memory of the context's device, an allocation
 * that ends before 9 * count doubles.
 * Decompositions.  The call is local to a context: a slab or brick rank paints its own grid, from its own upload's orig and local indices;
 * the caller gives every rank the orig of its block: orig_m + origin_m * dx, origin the global index of the rank's local cell 0 (the
 * partition helper does).  A rank's result is the rule on its own grid.  It equals the result on the whole grid at every face, given equal
 * positions (exact where dx and orig are dyadic), with one exception the rule itself makes: a face of axis a on the outermost plane of a
 * halo side (local i_a = 0 on a side with a lower neighbour, local i_a = n_a on a side with an upper one, where that plane lies inside the
 * whole grid) has one cell on the rank and two in the whole grid, and may take the other collider's value.  That plane is the far edge
 * of the halo block and the solve does not read it: a step after the ranks' own paint equals, byte for byte, a step of ranks that were
 * uploaded the whole grid's paint (tested on slabs and bricks).
 * Memory: the table and the counters take 72 * count + 4 * (count + 2) bytes from the call to the next upload; nothing else is held, and
 * ps_memory_stats entry 2 is 0 after the call.
 * Arrays, registered by a successful call and erased by every upload: "colliderMotions" (int32, 1: the count), "colliderMotionTable" (fp64,
 * 9 * count: the table the kernel read), "colliderMotionFaces" (int32, count + 2: painted faces per collider over the three axes together,
 * then the two left-alone counts) and "collisionVelocityX" / Y / Z (fp32 face grids: the buffers the next setup will read). */
typedef struct ps_collider_motions {
    int32_t count;          /* 1..PS_COLLIDER_MAX */
    const double* motion;   /* 9 * count doubles per collider k: v[3] (linear velocity), w[3] (angular velocity, rad per time unit), o[3] (the point v is given at) */
} ps_collider_motions;
int32_t ps_paint_collider_velocities(ps_context* ctx, const ps_collider_motions* m);
int32_t ps_paint_collider_velocities_device(ps_context* ctx, const double* motion, int32_t count, void* stream);

/* Collider shapes (extension; the piece between "loads out" and "motions in" for colliders that move): each collider's shape is stored
 * once, as a small SDF volume in the body's own frame; per step a table of rigid poses places all of them into the context's collision
 * buffer and id field, on the device.  Without it both calls above read the geometry of the last upload, which is stale once a body has
 * moved, and the caller rasterises every collider into a new collision grid and id grid itself.
 * ps_set_collider_shapes is a context setting, like the pivots of the loads: it copies every volume to the device before it returns,
 * persists across uploads, may be called before any upload and touches no field.  count = 0, s == NULL or shape == NULL with count 0 drops
 * the shapes and releases their memory.  Refusals (PS_INVALID, reason in ps_last_error, the previous shapes kept): "count outside 0..64";
 * "shape N: extent outside 2..1022"; "shape N: spacing not positive and finite"; "shape N: origin not finite"; "shape N: no samples"
 * (sdf == NULL); "shape N: non-finite value at sample M" — N the smallest such shape, M its smallest such x-fastest index; shape == NULL with
 * a count above 0.
 * ps_place_colliders / _device is a call like the paint, not a setting.  Call order and lifetime: it follows ps_upload_fields /
 * ps_upload_fields_device, and ps_upload_collider_ids if there is one; it precedes ps_paint_collider_velocities, ps_label_air_pockets and
 * the setup.  It rewrites the context's own collision buffer and id field at once, on the context's stream: what it wrote lives exactly as
 * long as that upload's collision.  Every field upload replaces it; a setup, solve or step and the Picard passes of ps_set_rheology keep
 * it.  A second call unions on top of the first, and the same poses leave the same values.  ps_upload_collider_ids after a call replaces
 * the whole id field and does not re-place.  A successful placement drops the air-pocket labels, which described the old solids.
 * polystokes_step and ps_step_device_fields upload and therefore never see a placement: a caller uses upload + ps_place_colliders +
 * ps_paint_collider_velocities + ps_step_device + download.  With uploaded weights[14] the weights stay the caller's; the placement still
 * changes what the motions, the loads' attribution and the contact angles read.  A context that never makes the calls launches exactly the
 * kernels it launched without them.
 * The pose table holds 12 doubles per collider: R[9], row-major, maps body to world; t[3] is the translation: world = R body + t.  R is
 * taken as orthonormal and is not checked beyond finiteness (poses are rigid: no scale).
 * The rule.  All arithmetic is fp64 from the fp32 / fp64 inputs, unfused, in the order written.  For cell c = (i0, i1, i2):
 *   r_m = orig_m + ((double)i_m + 0.5) * dx;
 *   D_best = negate ? -(double)collision[c] : (double)collision[c], negate the negateCollision of that upload's ps_params;  k_best = -1.
 * For k = 0 .. count-1 in order, skipping a collider whose 12 pose values are not all finite (the device form only; each such collider is
 * counted once in slot count + 1):
 *   1. d_m = r_m - t_m;  q_a = (R[0][a]*d_0 + R[1][a]*d_1) + R[2][a]*d_2   (R^T d);
 *   2. s_a = (q_a - o_a) / h - 0.5;  E = (PS_COLLIDER_SHAPE_REACH * dx) / h;  the collider takes part at c iff s_a >= -E and
 *      s_a <= (double)(n_a - 1) + E for all three a;
 *   3. c_a = min(max(s_a, 0.0), (double)(n_a - 1));  i_a = min((int)floor(c_a), n_a - 2);  f_a = c_a - (double)i_a;
 *   4. val = the trilinear value of the eight samples widened to double, interpolated along x, then y, then z, each step lo + (hi - lo) * f;
 *   5. out_a = (s_a - c_a) * h;  dist = sqrt((out_0*out_0 + out_1*out_1) + out_2*out_2);
 *   6. D_k = (negate ? -val : val) - dist   (beyond its box a volume continues as its border value minus the distance to the box);
 *   7. if D_k > D_best then D_best = D_k and k_best = k   (strict: ties go to what the cell holds, then to the lower collider).
 * With k_best >= 0: collision[c] = (float)(negate ? -D_best : D_best), ids[c] = k_best, and the cell is counted in slot k_best.  Otherwise
 * the cell keeps both values and is counted in slot count.  If the context holds no id field, the call first creates one filled with -1,
 * with the lifetime of an uploaded id field, so the loads and the paint see it.  The counters are integers: the result is bitwise
 * reproducible and independent of the traversal.
 * ps_place_colliders copies the table before it returns and ends with the stream idle.  ps_place_colliders_device reads 12 * count doubles
 * of device memory of the context's device (8-byte aligned) behind what `stream` holds, makes `stream` wait until it has read them, and
 * does not synchronise the host — except a call that has something to release first: a table of another size, or air-pocket labels.
 * Refusals (PS_INVALID, reason in ps_last_error, nothing written, the context stays usable): a call before any upload; no shapes set;
 * p == NULL or pose == NULL; "count differs from the shapes' count"; host form: "pose of collider N is not finite", N the smallest such
 * collider; device form: the pointer refusals of the other ps_*_device calls (below) — a pointer that is not 8-byte aligned, memory that is
 * not device memory of the context's device, an allocation that ends before 12 * count doubles.
 * Memory: the shapes cost 4 bytes per sample plus a descriptor table (56 bytes per collider); a placement costs 96 * count + 4 * (count + 2)
 * bytes until the next upload; a created id field costs one int32 cell grid; ps_memory_stats entry 2 is 0 after each call.
 * Arrays: "colliderShapes" (int32, 1: the count) stays registered while shapes are set.  A successful placement registers, and every upload
 * erases: "colliderPlacement" (int32, 1: the count), "colliderPoseTable" (fp64, 12 * count: the table the kernel read),
 * "colliderPlacedCells" (int32, count + 2: cells per collider, cells left alone, colliders skipped), "collisionField" (fp32 cell grid: the
 * buffer the next setup reads) and "colliderCellIds" (int32 cell grid).
 * Out of scope: a device form of ps_set_collider_shapes; scaling or deforming poses; swept volumes for fast bodies; a per-shape contact
 * cosine; repainting after later id uploads.  Decompositions: a slab or brick rank places on its own grid from its own upload's orig, as
 * the paint does.  A rank's result is the rule on its own grid, halo blocks included (a collider that reaches only a halo block is placed
 * there), and its counters are those of its own grid.  A cell reads and writes only itself, so given equal positions the result equals
 * the whole grid's at every cell, and the two ranks that share a cut hold the same values on both sides of it (tested on slabs and
 * bricks, with the placement before and after ps_set_slab / ps_set_brick). */
#define PS_COLLIDER_SHAPE_REACH 4.0   /* world cells beyond a volume's box that a placement still writes */

typedef struct ps_collider_shape {
    int32_t n[3];        /* samples along the body's x, y, z; each 2..1022 */
    int32_t reserved;    /* 0 */
    double h;            /* sample spacing, > 0; the same length unit as the grid's dx (poses are rigid: no scale) */
    double orig[3];      /* body-frame low corner of the volume; sample (i,j,k) sits at orig + (i+0.5, j+0.5, k+0.5) * h */
    const float* sdf;    /* n0*n1*n2 floats, x fastest, host memory; sign convention of the `collision` it is placed into */
} ps_collider_shape;
typedef struct ps_collider_shapes { int32_t count; const ps_collider_shape* shape; } ps_collider_shapes;
int32_t ps_set_collider_shapes(ps_context* ctx, const ps_collider_shapes* s);

typedef struct ps_collider_poses { int32_t count; const double* pose; } ps_collider_poses;
int32_t ps_place_colliders(ps_context* ctx, const ps_collider_poses* p);
int32_t ps_place_colliders_device(ps_context* ctx, const double* pose, int32_t count, void* stream);

/* Air pockets (extension; the free-surface fields above take the air-side pressure P_c from the caller, and a device-resident caller has
 * nothing that finds trapped air): the connected air regions of the uploaded grid, their volumes and whether they reach the grid's border,
 * and a pressure per pocket painted into the pressure member of the free-surface fields.  The gas law and the tracking of a pocket from
 * step to step stay with the caller (isothermal or adiabatic, what happens on a merge): with the ids, volumes and open flags of this step
 * and the id grid of the last one they are a few lines of the caller's own code.
 * Call order and lifetime.  ps_label_air_pockets follows ps_upload_fields / ps_upload_fields_device of a single domain; the result belongs to
 * that upload's grid, like the density field and the collider ids: every field upload drops it, ps_set_slab / ps_set_brick drop it too, a
 * setup, solve or step (the Picard passes of ps_set_rheology included) keeps it.  Before any upload the call returns PS_INVALID; on a context
 * that has a slab or brick or belongs to a ps_group it returns PS_FAILED, "air pockets need a single domain".  The three getters and the
 * pressure call return PS_FAILED with a reason when there are no labels.  polystokes_step and ps_step_device_fields upload and therefore
 * never see pockets: a caller uses upload + ps_label_air_pockets + ps_set_air_pocket_pressures + ps_step_device + download.
 * Inputs.  The weights the next setup will use: lw = "centerLiquidWeights", fw = "centerFluidWeights", fwF_a = "faceX/Y/ZFluidWeights" —
 * sampled from the uploaded SDFs exactly as the setup samples them, or the uploaded weights[14] where the caller passed them.  The call runs
 * that stage itself; a setup after the call produces what it produces without the call, bit for bit.
 * Definition.  Cells in x-fastest numbering; directions in the order -x, +x, -y, +y, -z, +z.
 *   core cell:  fw_c > 0 and lw_c <= 0.5;
 *   link:       two core cells that are face neighbours inside the grid and whose common face has fwF > 0;
 *   pocket:     a connected component of core cells under these links; pockets are numbered 0 .. K-1 by their smallest x-fastest cell
 *               index, whatever indexOrder is;
 *   skin cell:  a cell that is not core, has fw_c > 0 and lw_c < 1, and has at least one core face neighbour across a face with fwF > 0;
 *               it takes the pocket of the neighbour with the smallest lw, ties to the first in direction order;
 *   every other cell has id -1;
 *   air content of a cell with an id:  u_c = llrint((double)fw_c * (1.0 - (double)lw_c) * 1048576.0);
 *   per pocket k:  units_k = the sum of u_c over its core and skin cells (64-bit integer), cells_k = the number of its core cells,
 *               open_k = 1 if a core cell of it lies in the outermost cell layer of the grid on any side, else 0,
 *               volume_k = ((double)units_k * (1.0 / 1048576.0)) * (dx * dx * dx).
 * The sums are integers: every output is independent of the order of summation and bitwise reproducible; with the library's own 2x2x2
 * sampler every u_c is exact.  K = 0 is legal (no air); the K-sized arrays then have zero elements.
 * ps_label_air_pockets writes K to *count (count may be NULL).  ps_get_air_pockets writes volume_k and open_k (host memory, either pointer
 * may be NULL) and needs len >= K, PS_FAILED otherwise.  ps_download_air_pocket_ids writes the id of every cell (host memory, nx*ny*nz,
 * x-fastest); ps_download_air_pocket_ids_device writes them into device memory of the context's device in either layout, ordered against
 * `stream` like a download, without synchronising the host, and obeys the pointer refusals of the other ps_*_device calls (PS_INVALID).
 * ps_set_air_pocket_pressures: len must equal K and every value must be finite as the fp32 the field stores, else PS_INVALID — "pressure of pocket N is not finite" for
 * the smallest such N — and nothing changes.  On the device it writes the cell field (float)pressure[id_c] for id_c >= 0 and 0.f elsewhere
 * and installs it as the `pressure` member of the free-surface fields, as ps_upload_surface_fields_device would install the same array,
 * except that a sigma field that is present stays; a later ps_upload_surface_fields / _device replaces both members as before;
 * pressure == NULL drops the pressure member alone.  From there the existing path runs unchanged: q_c = sigma_c kappa_c + P_c, the arrays
 * "surfaceFields" and "surfaceGhostPressure", the Picard passes keeping the field.
 * Memory: while labels exist one int32 cell grid (4 * nx*ny*nz bytes) plus 24 * K bytes of results; the labels and link bytes of the
 * propagation live in the cell scratch the setup uses anyway, and the pressure call's table (8 * K bytes) is released before it returns:
 * ps_memory_stats entry 2 is 0 after each of these calls.  A drop releases the grid and the results.
 * Arrays: "airPockets" (int32, 1: K of the current labels; absent without labels), "airPocketIds" (int32 cell grid), "airPocketUnits"
 * (int64, K), "airPocketCells" (int32, K), "airPocketOpen" (int32, K), "airPocketVolume" (fp64, K), "airPocketPasses" (int32, 1: the
 * grid-wide propagation passes the call ran, one host round trip each; above 1 when a pocket winds through several 16^3 boxes). */
int32_t ps_label_air_pockets(ps_context* ctx, int32_t* count);
int32_t ps_get_air_pockets(ps_context* ctx, double* volume, int32_t* open, int64_t len);
int32_t ps_download_air_pocket_ids(ps_context* ctx, int32_t* ids);
int32_t ps_download_air_pocket_ids_device(ps_context* ctx, int32_t* ids, int32_t layout, void* stream);
int32_t ps_set_air_pocket_pressures(ps_context* ctx, const double* pressure, int64_t len);

/* solveGasSubclass equivalent on host buffers: upload + step + download (HDK_PolyStokes.C:222-609). */
int32_t polystokes_step(ps_context* ctx, const ps_params* p, const ps_fields_in* in,
                        ps_fields_out* out, ps_stats* stats);

/* Device-resident callers (extension): the five calls above that move SIM fields, on arrays that already live on the context's GPU.
 * The structs are the ones of the host calls; every non-null field pointer in them is device memory of the context's device, while the
 * scalars, nx / ny / nz and orig are read on the host as before.  The host entry points are unchanged.
 *
 * layout says how EVERY field of the call is stored.  For a field whose sample grid has the extents (d0, d1, d2) along x, y, z (the table at
 * the top of this file), sample (i, j, k) is the float at
 *   PS_LAYOUT_X_FASTEST (0):  i + d0*(j + d1*k)    the rule of the host calls
 *   PS_LAYOUT_Z_FASTEST (1):  k + d2*(j + d1*i)    a C-contiguous array indexed [i][j][k] (a torch or numpy tensor of shape (d0, d1, d2))
 * Both are dense; general strides, other element types and streams under graph capture are not supported.
 *
 * stream is the caller's hipStream_t (NULL: the default stream).  The library never runs its own work on it; it orders its own stream
 * against it with events.  An upload makes the context's stream wait for everything queued on `stream` before the call, so inputs written
 * by kernels or copies queued there are seen; it returns with the inputs consumed (the caller may overwrite them) and, like the host upload,
 * with the host synchronised.  A download first waits likewise for what `stream` holds, runs on the context's stream, makes `stream` wait
 * for it and returns WITHOUT synchronising the host: work queued on `stream` after the call sees the outputs, and a host reader synchronises
 * `stream` first.  out->vel[a] may alias in->vel[a].  Pointers need 4-byte alignment only (a tensor view with a storage offset is fine).
 *
 * ps_upload_fields_device leaves the context in the state ps_upload_fields leaves it in for the same values (same buffers byte for byte, same
 * uniform-viscosity shortcut, density field dropped, decomposition dropped) and reports the same errors for the host-side checks;
 * slab / brick ranks and ps_group_rank contexts take it like the host upload, ps_set_slab / ps_set_brick follow it.
 * ps_upload_density_field_device follows ps_upload_density_field: a non-finite value is PS_INVALID with "non-finite value at cell N", N the
 * smallest such index in x-fastest numbering whatever the layout; a constant field runs the scalar path at its clamped value; the same clamp
 * errors; NULL drops the field.  ps_upload_surface_fields_device follows ps_upload_surface_fields the same way (both fields of a call in
 * `layout`, N in x-fastest numbering whatever the layout).  ps_step_device_fields is polystokes_step: upload, the step (with the Picard
 * passes of ps_set_rheology), download, the three export flags.  ps_download_solution_fields_device writes the grids of ps_download_solution_fields.
 *
 * Refusals: PS_INVALID with the reason in ps_last_error, nothing read through any pointer, the context unchanged and usable (one exception:
 * a refused ps_upload_surface_fields_device drops both free-surface fields, as every refusal of that call does):
 *   - a layout other than 0 or 1;
 *   - a required field that is null (the messages of ps_upload_fields: "Surface field is missing." ...);
 *   - a pointer that is not 4-byte aligned;
 *   - a pointer that hipPointerGetAttributes does not report as device memory of the context's device: host, pinned host, managed and
 *     other-device memory are all refused;
 *   - an allocation that ends before the field does (hipMemGetAddressRange). */
enum ps_field_layout { PS_LAYOUT_X_FASTEST = 0, PS_LAYOUT_Z_FASTEST = 1 };
int32_t ps_upload_fields_device(ps_context* ctx, const ps_params* p, const ps_fields_in* in, int32_t layout, void* stream);
int32_t ps_upload_density_field_device(ps_context* ctx, const float* density, int32_t layout, void* stream);
int32_t ps_upload_surface_fields_device(ps_context* ctx, const ps_surface_fields* f, int32_t layout, void* stream);
int32_t ps_upload_collider_ids_device(ps_context* ctx, const int32_t* ids, int32_t layout, void* stream);   /* ps_upload_collider_ids */
int32_t ps_upload_contact_cosine_field_device(ps_context* ctx, const float* cosTheta, int32_t layout, void* stream);   /* ps_upload_contact_cosine_field; a refused pointer or layout leaves the context unchanged */
int32_t ps_get_collider_loads_device(ps_context* ctx, double* dev, int64_t len, void* stream);              /* ps_get_collider_loads */
int32_t ps_download_fields_device(ps_context* ctx, const ps_fields_out* out, int32_t layout, void* stream);
int32_t ps_download_solution_fields_device(ps_context* ctx, const ps_solution_out* out, int32_t layout, void* stream);
int32_t ps_step_device_fields(ps_context* ctx, const ps_params* p, const ps_fields_in* in, const ps_fields_out* out,
                              ps_stats* stats, int32_t layout, void* stream);

/* Advection (extension; the one grid-sized pass of a time step that a device-resident caller still had to write itself): up to
 * PS_ADVECT_MAX_CELL_FIELDS cell fields — the liquid SDF, the viscosity, the density, a surfactant field — and the MAC velocity itself,
 * moved semi-Lagrangian by a face velocity, the carrier: the context's written velocity or the caller's own three face grids.  The call
 * reads the context and writes only the caller's arrays.
 * Call order and lifetime.  It follows ps_upload_fields / ps_upload_fields_device of a single domain; nx, ny, nz and dx are that upload's.
 * It is not a setting: it changes nothing a setup, solve, step, download or any other call reads, and a context that never makes the call
 * launches exactly what it launched without it.  With carrier all NULL it needs a step or solve since that upload and since any later setup; the carrier is then the
 * velocity ps_download_fields would return, as it stands: after the write-back and, where set, ps_set_velocity_extrapolation.  With the
 * caller's carrier no step is needed.
 * ps_advect_fields_device follows ps_download_fields_device: it waits for what `stream` holds, runs on the context's stream, makes `stream`
 * wait for the result and does not synchronise the host; layout applies to every array of the call; the pointer refusals of the other
 * ps_*_device calls (above) apply.  ps_advect_fields takes host arrays, x fastest, and stages them through device temporaries that it
 * releases before it returns: ps_memory_stats entry 2 is 0 afterwards and the stream is idle.
 * The rule.  All arithmetic is fp64 from the fp32 inputs, unfused, in the order written.
 *   Index space.  Grid kind g (0 cell, 1 faceX, 2 faceY, 3 faceZ) has the extents d_m of the table at the top of this file and the offsets
 *   o_m = 0.5, except o_a = 0 on face grid a.  Sample (i_0, i_1, i_2) sits at p0_m = (double)i_m + o_m.
 *   Sampler Smp(F, g, p) for a finite p.  Per axis m: s_m = p_m - o_m;  c_m = min(max(s_m, 0.0), (double)(d_m - 1));  l_m = (int)floor(c_m);
 *   h_m = min(l_m + 1, d_m - 1);  f_m = c_m - (double)l_m.  The eight samples F[l or h], widened to double, are interpolated along x, then
 *   y, then z, each step lo + (hi - lo) * f.  (h is clamped, not l: the last layer has f = 0, so dt = 0 returns every finite field bit for
 *   bit — but for a -0, which returns as +0.)
 *   Carrier velocity.  U(p) = (Smp(C_0, 1, p), Smp(C_1, 2, p), Smp(C_2, 3, p)).
 *   Step factor.  r = dt / dx, one division on the host (array "advectionStep").
 *   Departure point.  order 1: p1_m = p0_m - r * U_m(p0).  order 2: pm_m = p0_m - (0.5 * r) * U_m(p0), then p1_m = p0_m - r * U_m(pm).
 *   Left alone.  If any pm_m (order 2) or any p1_m is not finite, nothing further is sampled: the sample takes the bits of its own source
 *   sample (cellIn[q] at the cell, C_a at the face) and is counted in slot 4.
 *   Value.  A cell output gets (float)Smp(cellIn[q], 0, p1), a velocity output on face grid a gets (float)Smp(C_a, 1 + a, p1); a value that
 *   is a NaN is stored as the quiet NaN 0x7fc00000 (the bits of a NaN that arithmetic produced are not the same on every processor).  The
 *   sample is counted in slot g when, for the sampled grid, some s_m < 0 or s_m > d_m - 1: the departure point left the grid and was
 *   clamped.  A cell's departure point is computed once and serves every cell field; a sample is counted once, whatever the number of
 *   fields.  The counts are int32 and wrap; they are integers: the result is bitwise reproducible and independent of the traversal.
 * Refusals (PS_INVALID, reason in ps_last_error, nothing written, the context stays usable): a call before any upload; a == NULL; "order
 * outside 1..2"; "cellFields outside 0..8"; "dt not finite"; "cellIn[N] is null" / "cellOut[N] is null" among the first cellFields;
 * "carrier partly null"; "velOut partly null"; "nothing to do" (cellFields == 0 and no velOut); the device form's layout and pointer
 * refusals; "output N overlaps input M" / "output N overlaps output M" for any output range that overlaps an input or another output — the
 * gather reads neighbours, so no array may be advected in place.  Outputs are numbered cellOut[q] = q, velOut[a] = 8 + a; inputs
 * carrier[a] = a, cellIn[q] = 3 + q.  PS_FAILED: "advection needs a single domain" on a slab or brick rank or a context of a ps_group;
 * "no written velocity since the upload" when the carrier is NULL and nothing has stepped.
 * Memory: a call holds 20 bytes of counters from the first call to the next upload and nothing else; ps_memory_stats entry 2 is 0 after
 * each call.
 * Arrays, registered by a successful call and erased by every upload: "advection" (int32, 1: the order), "advectionStep" (fp64, 1: r),
 * "advectionCounts" (int32, 5: clamped samples of the cell grid and of the faceX / faceY / faceZ grids, samples left alone).
 * Out of scope: BFECC correction and higher-order interpolation (the MacCormack correction is ps_advect_fields_scheme, below); redistancing of the SDF; body forces; CFL sub-stepping (the
 * caller chooses dt); advection across the cuts of a decomposition; in-place operation. */
#define PS_ADVECT_MAX_CELL_FIELDS 8
typedef struct ps_advection {
    double dt;                 /* finite, any sign (negative traces forward); 0 copies */
    int32_t order;             /* 1: Euler back-trace, 2: midpoint back-trace */
    int32_t cellFields;        /* 0..PS_ADVECT_MAX_CELL_FIELDS */
    const float* carrier[3];   /* faceX / faceY / faceZ grids.  All NULL: the velocity ps_download_fields would return.
                                  All non-NULL: the caller's own arrays.  A mix of NULL and non-NULL is refused. */
    const float* cellIn[PS_ADVECT_MAX_CELL_FIELDS];    /* cell grids nx*ny*nz */
    float* cellOut[PS_ADVECT_MAX_CELL_FIELDS];
    float* velOut[3];          /* all NULL: the velocity is not advected.  All non-NULL: the carrier advected by itself.
                                  A mix of NULL and non-NULL is refused. */
} ps_advection;
int32_t ps_advect_fields(ps_context* ctx, const ps_advection* a);                                        /* host arrays, x fastest */
int32_t ps_advect_fields_device(ps_context* ctx, const ps_advection* a, int32_t layout, void* stream);   /* device arrays */

/* Advection schemes (extension): ps_advect_fields / _device with a scheme — the semi-Lagrangian gather above, or the modified MacCormack
 * scheme of Selle et al. (a forward pass, a reverse pass, half the difference added back) with a limiter.  The limiter needs the eight
 * samples the forward sampler read at the departure point, which only the kernel knows; a caller composing two ps_advect_fields_device
 * calls cannot apply it, and writes the intermediate grid twice.
 * Everything ps_advect_fields / _device say about call order, the carrier, the layouts, stream ordering, the single-domain rule and every
 * refusal and its text holds for these calls.  Added refusals (PS_INVALID, nothing written, nothing launched), checked after "a is null":
 * "s is null"; "scheme outside 0..1"; "limiter outside 0..2".  With scheme == PS_ADVECT_SEMI_LAGRANGIAN the limiter is still validated and
 * otherwise the call IS ps_advect_fields / _device: the same bytes, the same single launch, the same three arrays, 20 bytes held, no new
 * array registered.
 * The rule for scheme == PS_ADVECT_MACCORMACK.  All arithmetic is fp64, unfused, in the order written.  For the sample x at p0 of grid g with
 * the source F (cellIn[q] on the cell grid, C_a on face grid a; the carrier is C throughout and is never replaced):
 *   Forward pass.  The rule of ps_advect_fields unchanged: it gives p1, whether the sample is left alone, whether the sampler clamped, and
 *   hat[x], the fp32 value ps_advect_fields would store (the quiet-NaN rule included).  hat is an fp32 grid of its own.
 *   Reverse trace.  The departure rule with -r in place of r (negation is exact: this equals dt -> -dt), started at p0, not at p1.
 *   order 1: q1_m = p0_m - (-r) * U_m(p0).  order 2: qm_m = p0_m - (0.5 * (-r)) * U_m(p0), then q1_m = p0_m - (-r) * U_m(qm).
 *   bar = Smp(hat, g, q1), kept in fp64.
 *   Corrected value.  v = (double)hat[x] + 0.5 * ((double)F[x] - bar).
 *   Limits.  The eight samples F[l or h] of the forward sampler at p1, widened to double, in the order x fastest, then y, then z:
 *   lo = hi = the first; for each t of the next seven: if (t < lo) lo = t; if (t > hi) hi = t (a NaN sample fails both comparisons).
 *   outside = v < lo || v > hi.  PS_ADVECT_LIMIT_CLAMP: v = v < lo ? lo : (v > hi ? hi : v).  PS_ADVECT_LIMIT_REVERT: v = outside ?
 *   (double)hat[x] : v.  PS_ADVECT_LIMIT_NONE: v is unchanged and nothing is counted.  With a limiter, the value is counted as changed
 *   when outside holds.
 *   Fallback.  The sample takes the bits of hat[x], and the limiter is neither applied nor counted, if the forward pass left the sample
 *   alone; or the forward sampler clamped (the departure point left the grid); or any qm_m or q1_m is not finite; or the reverse sampler of
 *   hat clamped.
 *   Store.  Otherwise (float)v, a NaN as 0x7fc00000.  A cell's two traces are computed once for all its fields.
 * Arrays.  "advection", "advectionStep" and "advectionCounts" are as after the forward pass.  A successful scheme 1 call registers, and
 * every upload erases with the others: "advectionScheme" (int32, 2: the scheme and the limiter) and "advectionCorrection" (int32, 8: slots
 * 0..3 the values the limiter changed on the cell, faceX, faceY, faceZ grids — a cell counts once per field changed; slots 4..7 the
 * fallback samples of those grids — a cell counts once).  They describe the last scheme 1 call since the upload; a later scheme 0 call
 * leaves them.  The counts are int32 and wrap; they are integers: bitwise reproducible and independent of the traversal.
 * Memory.  A scheme 1 device call holds, from that call until the next upload, 32 more bytes of counters and an fp32 scratch for hat of
 * 4 * (cellFields * nx*ny*nz + (velOut ? the three face grids : 0)) bytes, sized to the largest such call since the upload; a call that
 * needs no more than what is held allocates nothing, and ps_memory_stats entry 2 is 0 after it (a call that has to grow the scratch leaves
 * the smaller one there until the context next synchronises).  The host form puts hat into its staging temporary and releases it before it
 * returns: only the 32 + 20 bytes of counters stay.  The overlap refusals are unchanged: the scratch is the library's own and overlaps
 * nothing.
 * Out of scope: BFECC; cubic interpolation; redistancing; CFL sub-stepping; advection across the cuts of a decomposition; in-place
 * operation; a caller-supplied scratch. */
#define PS_ADVECT_SEMI_LAGRANGIAN 0
#define PS_ADVECT_MACCORMACK      1
#define PS_ADVECT_LIMIT_NONE   0
#define PS_ADVECT_LIMIT_CLAMP  1
#define PS_ADVECT_LIMIT_REVERT 2
typedef struct ps_advection_scheme { int32_t scheme; int32_t limiter; } ps_advection_scheme;
int32_t ps_advect_fields_scheme(ps_context* ctx, const ps_advection* a, const ps_advection_scheme* s);
int32_t ps_advect_fields_scheme_device(ps_context* ctx, const ps_advection* a, const ps_advection_scheme* s, int32_t layout, void* stream);

/* y = A x for host vectors of length nPressures+nStresses:
 * ApplyPressureStressMatrix::apply (lib/include/ApplyPressureStressMatrix.h:102-184). */
int32_t ps_apply_operator(ps_context* ctx, const double* x, double* y);

/* z = M^-1 r with the preconditioner of the set-up context (identity, Jacobi, Chebyshev), host vectors in reference numbering:
 * the parity hook for the preconditioner (tests compare it with the oracle's). */
int32_t ps_apply_preconditioner(ps_context* ctx, const double* r, double* z);

/* Inspection of solver state by name — the data behind printAllData()'s 43 point clouds
 * (Solver.cpp:1030-1074) and exportComponentMatrices() (Solver.cpp:543-566).
 * ps_query_array returns the element count (or <0 if unknown) and the element size in bytes;
 * ps_read_array copies it to host.
 * Beside the reference's arrays there are a few int32 diagnostics of the device path: "valuesCoded" (1: stencil values are
 * int8 codes), "columns16" (bit 0 / 1: S / St have the compressed 16-bit-column stream), "diagonalsCoded" (bit 0 / 1: uInv /
 * McInv are 1-byte value-set codes), "fusedStep" (1: the last PCG solve ran the four-kernel step), "streamRuns" (4 values:
 * entries of the distinct runs / all entries of the compressed stream of S, then of St), "launchWalk" (5 records of 8 values for the
 * S product, then the St products of modes 0..3, of the last single-domain PCG solve: launched, kernel, chunks, workgroups, walk
 * parameter, 1 for the pair walk of the two-unit kernels, least and most steps with a chunk taken by one workgroup; zeros where that
 * product did not run). */
int64_t ps_query_array(ps_context* ctx, const char* name, int32_t* elem_bytes);
int32_t ps_read_array(ps_context* ctx, const char* name, void* dst, int64_t dst_bytes);

/* MatrixMarket export with the reference's file names and text format
 * (Solver.cpp:533-606; extern/eigen/unsupported/Eigen/src/SparseExtra/MarketIO.h:310-380). */
int32_t ps_export_component_matrices(ps_context* ctx, const char* prefix);
/* exportMatrices + exportMatricesPostSolve (Solver.cpp:533-572): <prefix>Mat_A.mtx (n x n, empty: the live factored path
 * never assembles A), Vec_b.mtx, Vec_guess.mtx (zero) and, after a solve, solutionVector.mtx. */
int32_t ps_export_matrices(ps_context* ctx, const char* prefix);
int32_t ps_export_stats(ps_context* ctx, const ps_stats* stats, const char* prefix);

/* Solve a component set exported by exportComponentMatrices() (Solver.cpp:543-566: <prefix>Mat_G.mtx, Mat_Dt, Mat_JG,
 * Mat_JDt, Mat_McInv, Mat_uInv, Mat_Inv_Mr_plus_2JDtuDJ, Vec_b) with the same PCG (params: tolerance,
 * maxSolverIterations, preconditioner); the operator is applied literally as in ApplyPressureStressMatrix.h:102-179.
 * x_out receives [p; tau] (length nPressures + nStresses, reference numbering).  `dt` is dimData entry 27. */
int32_t ps_solve_exported_system(ps_context* ctx, const char* prefix, const ps_params* params, double dt, double* x_out,
                                 int64_t x_len, ps_stats* stats);

/* Micro-benchmark hooks used by bench.py for the roofline object: run `iters` launches of the
 * dominant kernel(s) on the solver stream bracketed by HIP events, return avg ms per launch. */
int32_t ps_bench_kernel(ps_context* ctx, const char* kernel, int32_t iters, double* avg_ms,
                        double* algorithmic_bytes);

/* Device memory held through this library, for a host application's bookkeeping and for the tests that check a context does not grow
 * across steps: out4 = { bytes allocated by all contexts of this process (buffers waiting for release included), their peak,
 * bytes of buffers THIS context dropped that still wait for release (0 after every successful or failed setup / solve / step: they are
 * released where the context's stream has just been synchronised), live contexts }.  ctx may be null (entry 2 is then 0).
 * Replaces nothing in the reference (its Solver owns host temporaries for the duration of the call, exec/HDK_PolyStokesSolver.h:272-375). */
int32_t ps_memory_stats(const ps_context* ctx, int64_t* out4);

/* ---- Multi-GPU (not in the reference, which is single-process) -------------------------
 * Slab decomposition along z, cut at multiples of lcm(16, tileSize).  Each rank is given (as an ordinary
 * ps_fields_in) its slab plus one halo tile per interior side, and is told which local cell layers it owns.
 * Per operator apply the ranks exchange the one-cell layer of x their rows touch across each cut and the y
 * contributions their rows make to the neighbour's layer; CG scalars are all-reduced. */
typedef struct ps_slab {
    int32_t rank, world;
    int32_t zLoOwned, zHiOwned;     /* owned cell layers [zLo, zHi) in LOCAL grid coordinates (multiples of 16) */
    int32_t hasLower, hasUpper;     /* a neighbouring rank exists below / above */
    int32_t zGlobalOwned;           /* GLOBAL index of the cell layer zLoOwned: tile offsets are formed with global z, so a tile's
                                     * matrices and fit do not depend on the decomposition */
} ps_slab;
int32_t ps_set_slab(ps_context* ctx, const ps_slab* slab);            /* after ps_upload_fields, before setup */
/* The same along all three axes (bricks whose faces lie on tile-size multiples; 8 GPUs as 2 x 2 x 2): the rank's local
 * grid is its owned box plus one 16-cell halo block on every side that has a neighbour.  rank = c0 + dims[0] * (c1 + dims[1] * c2)
 * for the brick at (c0, c1, c2); the neighbour below / above along axis a is rank -+ the stride of a.  A plane on a cut belongs to the
 * rank above it (faces and edges with offset 0 along that axis).  Every rank exchanges with its <= 6 face neighbours only: the
 * DOFs a row touches across two cuts at once belong to rows of another rank.  ps_set_slab is ps_set_brick with dims = {1, 1, world}. */
typedef struct ps_brick {
    int32_t rank, world;
    int32_t dims[3];                /* ranks per axis */
    int32_t lo[3], hi[3];           /* owned cells [lo, hi) per axis in LOCAL grid coordinates (multiples of 16 and of the tile size) */
    int32_t hasLower[3], hasUpper[3];
    int32_t globalLo[3];            /* GLOBAL index of the cell lo: tile offsets are formed with global indices */
} ps_brick;
int32_t ps_set_brick(ps_context* ctx, const ps_brick* brick);         /* after ps_upload_fields, before setup */

/* One process per GPU: RCCL communicator on the solver stream.  Rank 0 calls ps_comm_unique_id and hands the
 * 128 bytes to the other ranks (bench.py broadcasts them over gloo); every rank then calls ps_comm_init_rccl.
 * ps_step_device then runs the distributed step; ps_setup_device / ps_solve_device / polystokes_step refuse a
 * context with a slab (a rank's local system is only a fragment).  The communicator is destroyed with the context.
 * An interrupt callback (ps_set_interrupt) on ANY rank stops all ranks at the same CG batch (PS_INCOMPLETE); a rank
 * whose setup fails makes every rank return PS_FAILED instead of leaving its neighbours waiting. */
int32_t ps_comm_unique_id(void* id128);
int32_t ps_comm_init_rccl(ps_context* ctx, const void* id128, int32_t rank, int32_t world);
int32_t ps_comm_selftest(ps_context* ctx);   /* collective: all-reduce, grouped send/recv to self, and (slab set, world > 1) one ring
                                              * step with the real neighbours and a check of the all-reduced sums */
/* What the last distributed solve of this rank did (no reference counterpart: the reference is single-process, its only parallelism
 * is lib/include/ApplyPressureStressMatrix.h:122-164): out8 = { bytes sent per CG iteration over the rank's cuts, owned DOFs,
 * 1 if the halo exchanges overlapped with the interior rows, sum [ms] and count of sampled x-exchange transports, sum [ms] and
 * count of sampled scalar all-reduces (incl. synchronisation), cells of the rank's halo blocks whose label was replaced by the
 * owner's during setup (the classification reaches beyond a halo block: boundary layers, fixReducedRegionBoundaries) }. */
int32_t ps_dist_stats(ps_context* ctx, double* out8);
/* Host-staged transport instead of RCCL (pack -> D2H -> TCP -> H2D -> unpack; scalar all-reduce through rank 0):
 * one process per rank, several ranks may share one GPU (RCCL refuses duplicate devices) — the route by which the
 * real multi-process path runs on a single-GPU box, and the fallback where librccl is missing.  Rank r listens on
 * base_port + r of `host` (dotted IPv4).  Collective over the `world` ranks. */
int32_t ps_comm_init_tcp(ps_context* ctx, int32_t rank, int32_t world, const char* host, int32_t base_port);

/* Several ranks inside ONE process on one GPU (device-to-device copies instead of RCCL): used to test the
 * distributed algorithm on a single-GPU box.  Same kernels, same exchange lists, same reduction order. */
typedef struct ps_group ps_group;
ps_group* ps_group_create(int32_t device, int32_t world);
void ps_group_destroy(ps_group* g);
ps_context* ps_group_rank(ps_group* g, int32_t rank);                 /* upload fields / set slab per rank */
int32_t ps_group_step(ps_group* g, ps_stats* stats);                  /* setup on every rank + distributed solve */

#ifdef __cplusplus
}
#endif
#endif /* POLYSTOKES_H */
