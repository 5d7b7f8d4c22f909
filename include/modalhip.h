/* modalhip -- C ABI of the MI355X-native modal-audio hot path (libmodalhip.so).
 *
 * The reference (khiner/MeshEditor) has no FFI layer for this path: it is reached through C++ free functions and
 * plain structs (src/audio/mesh2modes.h:77-88, src/audio/ModalAudio.h:294-315).  This header is the thin C ABI the
 * C++ mirror of those functions (mesheditor_amd/cpp/) and the Python binding (mesheditor_amd/api.py) sit on: opaque
 * handles, plain pointers and sizes, int status codes, no exceptions and no torch types across the boundary.
 * Every entry point names the reference interface it replaces.  All functions return MH_OK (0) or an MH_E* code;
 * mh_last_error() gives the message of the calling context's last failure.
 *
 * Threading: a context owns one HIP stream, its library handles and its device memory pool.  Calls on different
 * contexts may run concurrently from different host threads (the reference solves several entities concurrently,
 * src/audio/AudioSystem.cpp:812,865); calls on one context must be serialised by the caller.
 */
#ifndef MODALHIP_H
#define MODALHIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    MH_OK = 0,
    MH_EINVAL = 1, /* bad argument */
    MH_EHIP = 2, /* HIP / rocBLAS / rocSOLVER failure (no GPU, out of memory, ...) */
    MH_ECANCELLED = 3, /* JobMonitor::Cancelled() was observed (src/Job.h:13-19) -> empty result */
    MH_ENOTCONVERGED = 4, /* eigensolver hit its iteration limit -> empty result (mesh2modes.cpp:490) */
    MH_EFACTOR = 5, /* shifted operator not positive definite -> std::runtime_error (CholeskyShiftInvert.cpp:44) */
    MH_EEMPTY = 6 /* no tets left / no modes in band */
};

typedef struct mh_context mh_context;
typedef struct mh_mesh mh_mesh;
typedef struct mh_system mh_system;
typedef struct mh_bank mh_bank;

/* AcousticMaterialProperties, src/audio/AcousticMaterialProperties.h:6-16 */
typedef struct {
    double density, young_modulus, poisson_ratio, alpha, beta;
} mh_material;

/* modal::SolverConfig, src/audio/mesh2modes.h:17-26 */
typedef struct {
    float min_mode_freq, max_mode_freq;
    uint32_t num_modes, num_fem_modes;
    double tolerance, warm_tolerance;
    uint32_t max_restarts;
    int32_t has_fundamental;
    float fundamental_freq;
} mh_solver_config;

/* modal::SolveProfile, src/audio/mesh2modes.h:29-34.  Seconds per stage (HIP-event timed on the context's stream).
 * factorize = preconditioner set-up (the reference's Cholesky factorisation slot); op_solve = preconditioner
 * applications (the reference's triangular solves); op_applications = preconditioned block columns;
 * restarts = LOBPCG iterations. */
typedef struct {
    double mass_props, quad_mesh, assemble, sample_excite, factorize, iterate, op_solve, extract;
    uint32_t dofs, stiffness_nonzeros, op_applications, restarts;
    /* health of the device solve (no reference counterpart; zero / rounding level on a healthy run): Rayleigh-Ritz steps that were redone by a
     * fall-back because the multi-workgroup tridiagonalisation timed out, and the worst sampled residual of the steps' self-check against the
     * saved Rayleigh-Ritz matrix, max_i |A z - theta z|_i over max_i (sum_c |a_ic z_c| + |theta z_i|) -- 1e-13 ... 3e-12 measured; a solve
     * whose check exceeds 1e-6 fails with MH_EHIP */
    uint32_t sytrd_redos;
    /* wanted pairs that the LAST RESORT handed on with a residual still above the tolerance (below ten times it, unchanged for thirty iterations: the
     * rounding floor of a mesh at the edge of double precision -- raw Delaunay fills with cells at 1e-8); 0 on every solve that converged */
    uint32_t pairs_at_floor;
    double rr_selfcheck;
} mh_profile;

/* MassProperties, src/audio/ContactModel.h:16-23 (quaternion as w, x, y, z) */
typedef struct {
    double mass;
    float center_of_mass[3], inertia_diagonal[3], inertia_orientation_wxyz[4];
} mh_mass_props;

/* sizeof(mh_profile), sizeof(mh_solver_config), sizeof(mh_material), sizeof(mh_mass_props) as this library was built: a binding checks its own
 * struct images against them (needs no GPU) */
void mh_abi_struct_sizes(uint32_t out[4]);
int mh_context_create(int device, mh_context **out);
void mh_context_destroy(mh_context *);
const char *mh_last_error(const mh_context *);
/* Blocks until everything queued on the context's stream has finished. */
int mh_context_synchronize(mh_context *);
/* The context's hipStream_t, for callers that time with HIP events. */
void *mh_context_stream(mh_context *);
void mh_default_config(mh_solver_config *);
/* Kernel timing of the path itself (no reference counterpart; the one instrumentation hook that has to live in the product,
 * because it brackets the product's own launches in place -- bench.py's roofline objects read it; timing loops and experiments
 * are in libmodalhip_lab.so): when enabled, every launch of the path's named kernels is bracketed by
 * HIP events on the context's stream.  Kernel classes and their algorithmic work unit:
 *   MH_KERNEL_SPMM     the operator products y = (K - sigma M) x over n x w panels (both levels, all precisions);
 *                      bytes: (9 values + 1 index) per node block + 4 B per row pointer + every panel pass
 *   MH_KERNEL_ASSEMBLY the K/M assembly kernel of the quadratic level; bytes: per tet 16 B corners + 96 B coordinates
 *                      + 40 B node ids read, 80 B per node block written
 *   MH_KERNEL_BANK     the resonator kernel (RenderObjectFast); flops: 11 per rendered mode-sample
 *   MH_KERNEL_COMBINE  the basis updates out = [X | W | P] C of the eigensolver (k_combine, fp64 MFMA; the vendor dgemm for blocks of
 *                      >= 400 basis columns); flops: 2 n (basis columns) (output columns) per launch.  MH_KERNEL_COMBINE_BYTES carries
 *                      the same launches' algorithmic bytes (8 n (basis + output columns)) as its work, no time of its own.
 *                      MH_KERNEL_COMBINE_FULL: the subset of those launches with >= 200 basis and >= 128 output columns (an iteration's
 *                      full-size update of X and P together: 240 -> 160 columns on the 65-pair solve), same work unit.
 *   MH_KERNEL_JUNCTION the coupled resonator kernel of a block with contact junctions (k_bank_modes_coupled); work: frames x junctions,
 *                      the number of per-frame contact solves (its time is a serial chain per frame, not arithmetic)
 * Stats are the totals since the last enable: launches, summed device milliseconds, summed work. */
enum { MH_KERNEL_SPMM = 0, MH_KERNEL_ASSEMBLY = 1, MH_KERNEL_BANK = 2, MH_KERNEL_COMBINE = 3, MH_KERNEL_COMBINE_BYTES = 4, MH_KERNEL_COMBINE_FULL = 5, MH_KERNEL_JUNCTION = 6, MH_KERNEL_CLASSES = 7 };
int mh_context_time_kernels(mh_context *, int enable);
int mh_context_kernel_stats(mh_context *, uint64_t *launches, double *total_ms, double *total_bytes); /* MH_KERNEL_SPMM */
int mh_context_kernel_class_stats(mh_context *, int kernel_class, uint64_t *launches, double *total_ms, double *total_work);

/* ---- analysis half: modal::mesh2modes (src/audio/mesh2modes.cpp:605-658), stage by stage ---- */

/* TetMesh (src/mesh/TetMesh.h:10-13) -> HBM.  points: n_points x 3 doubles (AoS dvec3); tets: n_tets x 4 uint32. */
int mh_mesh_create(mh_context *, uint32_t n_points, const double *points_xyz, uint32_t n_tets, const uint32_t *tets, mh_mesh **out);
void mh_mesh_destroy(mh_mesh *);

/* FilterDegenerate + BuildQuadMesh + ComputeElementBases + AssembleQuadratic (mesh2modes.cpp:42-60,137-165,246-264,
 * 273-327) on the device: K as 3x3 node blocks (BSR), M as one scalar per node block (M = M_node (x) I3). */
int mh_assemble(mh_context *, const mh_mesh *, const mh_material *, mh_system **out);
/* What mh_assemble derives from the points and tets alone (numbering, interpolation lists, element bases, block patterns, aggregates,
 * components) is built on the first assembly with the mesh's own context and kept with the mesh; later assemblies on it only form K and M.
 * builds: how many times that structure has been built for this mesh (0 before the first assembly and after a failed one);
 * bytes: device memory the kept structure holds (0 while there is none).  Either pointer may be null. */
int mh_mesh_structure_stats(const mh_mesh *, uint64_t *builds, uint64_t *bytes);
void mh_system_destroy(mh_system *);
int mh_system_dims(const mh_system *, uint32_t *dofs, uint32_t *node_count, uint32_t *kept_tets, uint64_t *node_blocks);
/* QuadMesh::ElementNodes in the reference's numbering (corners, then midside ids in first-encounter order). */
int mh_system_element_nodes(const mh_system *, uint32_t *out_kept_tets_x10);
/* Every stored node block as (row node, col node, 9 row-major K entries, M scalar), reference numbering, full
 * (both triangles).  Arrays sized by mh_system_dims' node_blocks. */
int mh_system_export_blocks(const mh_system *, uint32_t *row_node, uint32_t *col_node, double *k_blocks, double *m_blocks);
/* y = K x (which = 0), M x (which = 1) or (K - sigma M) x at the reference's shift (which = 2) for `width` vectors, x and y column-major n x width in the reference's
 * DOF order (3*node + component).  The SpMM kernel of the eigensolver, exposed for parity and roofline measurement.
 * which = 3 / 4: the same shifted product as the preconditioner's smoothers form it -- single-precision values and panel
 * (3), double-precision values over a single-precision panel (4, width % 4 == 0) -- so those kernels can be checked too. */
int mh_system_matvec(mh_system *, int which, const double *x, double *y, uint32_t width);
/* The reference's shift-invert operator as an OPERATION (src/audio/CholeskyShiftInvert.h:11-30: set_shift + perform_op / solve_panel):
 * x = (K - sigma M)^-1 b for `width` right-hand sides, b and x column-major n x width in the reference's DOF order.  There is no
 * factorisation here: the panel is solved by preconditioned conjugate gradients (the eigensolver's three-level cycle as the
 * preconditioner) to a relative residual `rel_tol` per column (0 = 1e-11), at most `max_iters` steps (0 = 200).  sigma must be negative
 * (MH_EFACTOR otherwise: the reference's "Modal shift-invert factorization failed.", CholeskyShiftInvert.cpp:44).  *iterations and
 * *worst_relative_residual (nullable) report the solve.  The hierarchy of the shift is built on first use and kept with the system, as
 * set_shift keeps its factor.  mh_eigs is the fast path to the eigenpairs; this exists for callers that drive their own Lanczos. */
int mh_system_shift_invert(mh_system *, double sigma, const double *b, double *x, uint32_t width, double rel_tol, uint32_t max_iters, uint32_t *iterations,
                           double *worst_relative_residual);

/* The nearest tet point to each excitation position, first minimum wins (mesh2modes.cpp:626-636). */
int mh_nearest_points(mh_context *, const mh_mesh *, uint32_t n, const float *positions_xyz, uint32_t *nearest);

/* ComputeModes' eigensolve (mesh2modes.cpp:441-497): the `nev` lowest eigenpairs of K x = lambda M x, ascending,
 * M-orthonormal.  Replaces Spectra SymGEigsShiftSolver + CholeskyShiftInvert (cold) and SubspaceIterate (warm, when
 * seed_basis has n rows and >= nev columns; column-major float as ModalResult::Basis) with a block LOBPCG on the
 * shifted pencil (K - sigma M, M) preconditioned by a three-level cycle.  residual_tol is the relative residual
 * ||K x - lambda M x|| / (|lambda - sigma| ||M x||) every returned pair meets.  cancel (nullable; one byte, the storage of JobMonitor's
 * std::atomic<bool>) is polled between iterations; progress (nullable) receives 0.3 + 0.65 * converged / nev as the reference's warm path does. */
int mh_eigs(mh_system *, uint32_t nev, double sigma, double residual_tol, uint32_t max_iters,
            const float *seed_basis, uint32_t seed_rows, uint32_t seed_cols,
            const volatile unsigned char *cancel, volatile float *progress, double *eigenvalues, mh_profile *profile);
/* shapes[node][column][xyz] = eigenvector rows 3*node + {0,1,2} (mesh2modes.cpp:498-504), as float. */
int mh_system_gather_shapes(const mh_system *, uint32_t n_nodes, const uint32_t *nodes, uint32_t n_cols, float *shapes);
/* ModalResult::Basis: n x n_cols column-major float, rows in the reference's DOF order (mesh2modes.cpp:509). */
int mh_system_basis(const mh_system *, uint32_t n_cols, float *basis);
/* The same in double, for parity tests. */
int mh_system_eigenvectors(const mh_system *, uint32_t n_cols, double *vectors);
/* What `residual_tol` of mh_eigs meant in the last solve (no reference counterpart: Spectra's tolerance is on Ritz values).
 * On a mesh WITHOUT near-degenerate elements a pair is accepted at ||K x - lambda M x||_2 < residual_tol |lambda - sigma| ||M x||_2.
 * On a mesh WITH them (elements of shape measure < 0.02: the sliver patches of the preconditioner exist) the same test is made
 * in the Jacobi-scaled norm ||.||_{D^-1}, D = diag(K - sigma M): the rounding noise eps ||A|| |x| of the slivers' rows alone
 * exceeds the tolerance in the 2-norm, while in the scaled norm those rows count as little as their noise means (identical on
 * a uniform mesh).  *worst_plain_residual then holds the worst 2-norm relative residual among the returned elastic pairs,
 * measured once after convergence (-1 when the 2-norm was the criterion); eigenvalue accuracy is checked against the oracle
 * on every committed scan fixture (2e-11 ... 3e-9).  dropped_patches[2]: sliver patches of the P2 / P1 level whose block was
 * not safely positive definite and contribute nothing to the smoother. */
int mh_system_residual_report(const mh_system *, double *worst_plain_residual, uint32_t dropped_patches[2]);

/* Host-side scalar stages of the path (the reference runs them on the calling thread as well). */
/* ComputeMassProperties (mesh2modes.cpp:73-126) */
int mh_compute_mass_properties(uint32_t n_points, const double *points_xyz, uint32_t n_tets, const uint32_t *tets, double density,
                       const float baked_scale[3], double length_to_si, mh_mass_props *out);
/* modal::PostprocessModes (mesh2modes.cpp:515-588).  shapes: [position][eigenpair][xyz].  Returns the mode count in
 * *n_modes (0 = the reference's empty result); outputs hold at most n_eigs modes. */
int mh_postprocess_modes(uint32_t n_eigs, const double *eigenvalues, uint32_t n_pos, const float *shapes, float shape_scale,
                         const mh_material *, const mh_solver_config *, uint32_t *n_modes, float *freqs, float *t60s,
                         float *shapes_out, float *original_fundamental);
/* modal::RescaleModes (mesh2modes.cpp:590-603).  *scalable = 0 when the Poisson ratio differs (std::nullopt). */
int mh_rescale_modes(uint32_t n_eigs, const double *eigenvalues, uint32_t n_pos, const float *summary_shapes,
                     const mh_material *solved, const mh_material *edited, const mh_solver_config *, int *scalable,
                     uint32_t *n_modes, float *freqs, float *t60s, float *shapes_out, float *original_fundamental);

/* ---- synthesis half: the resonator bank (src/audio/ModalAudio.{h,cpp}) ---- */

/* ModalBank::ActiveImpact, src/audio/ModalAudio.h:150-162.  The host mirror owns the event queue, the impact list
 * and the object deal (ModalAudio.cpp:28-82,430-461); the device renders a block from them. */
typedef struct {
    uint32_t object, ex_pos, samples_left, reserved;
    /* Real-valued fields travel as double so that the fp64 bank keeps its recurrences exact between blocks; the fp32
     * bank's values are floats and round-trip through double unchanged. */
    double jx, jy, jz;
    double phase_re, phase_im, rot_re, rot_im;
    double gamma, accel_amp;
    double click_b0, click_a1, click_a2, click_z1, click_z2;
} mh_impact;

/* Device mirror of a published ModalBank (InstallModalBank, ModalAudio.cpp:277-289).  Per-mode columns are n_modes
 * long, shape columns n_shapes long, per-object columns n_objects long; layouts as ModalAudio.h:103-166.
 * use_double selects the fp64 bank (same layout, double state and arithmetic). */
int mh_bank_create(mh_context *, int use_double, uint32_t n_objects, uint32_t n_modes, uint32_t n_shapes,
                   const uint32_t *mode_offset, const uint32_t *mode_count, const uint32_t *shape_offset,
                   const float *shape_x, const float *shape_y, const float *shape_z, mh_bank **out);
void mh_bank_destroy(mh_bank *);
/* TuneModalObject's device effect (ModalAudio.cpp:340-393): overwrite coefficient columns [first, first+count). */
/* Column arrays are float for an fp32 bank and double for an fp64 bank. */
int mh_bank_set_coefficients(mh_bank *, uint32_t first, uint32_t count, const void *coeff_re, const void *coeff_im,
                             const void *radiation_gain, const void *out_phase_im, const void *out_phase_re);
/* SetModalObjectShapes (ModalAudio.cpp:395-410) */
int mh_bank_set_shapes(mh_bank *, uint32_t first, uint32_t count, const float *x, const float *y, const float *z);
/* SilenceObject's state clear (ModalAudio.cpp:53-56) */
int mh_bank_zero_state(mh_bank *, uint32_t first_mode, uint32_t count);
/* One block of RenderModal (ModalAudio.cpp:486-555): force curves + click per impact (:504-538), RenderObjectFast per
 * dealt object (:86-147), mix in renderer order (:553-555).  `out` (frames samples, float or double per the bank) is
 * ADDED to, as the reference does.  The deal arrives flattened: renderer r renders objects
 * deal_objects[deal_offset[r] .. deal_offset[r+1]) in that order, each with mode count render_count[i] (Tuned when the
 * object has impacts, Live otherwise).  impacts is updated in place (phase, samples_left, click state).
 * Per dealt object the device returns its post-block energy, its audible prefix (chunk-granular `live`) and whether
 * it fell silent (no impacts and gain-weighted energy below 1e-12: its state was zeroed, ModalAudio.cpp:141-144), plus
 * its share of the modal-energy diagnostic over its tuned_count modes (ModalAudio.cpp:564-577; nullable). */
int mh_bank_render(mh_bank *, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts,
                   uint32_t n_renderers, const uint32_t *deal_offset, const uint32_t *deal_objects, const uint32_t *render_count,
                   const uint32_t *tuned_count, const float *out_gain, const float *listener_gain, void *out, double *object_energy,
                   uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy);
/* A sustained force drive (no reference counterpart in ModalAudio; the bank-side primitive under the drive rows of the reference's
 * surface renderer, src/audio/surface/): a caller-supplied force signal applied to `object` at excitation position `ex_pos` along
 * (jx, jy, jz), for the block it is passed with.  Stateless between blocks, no force curve, no click filter.  Fields are float, as
 * ModalEvent's are (ModalAudio.h:28-37). */
typedef struct {
    uint32_t object, ex_pos;
    float jx, jy, jz;
} mh_drive;
/* sizeof(mh_drive) as this library was built (extends mh_abi_struct_sizes, whose four entries stay as they are) */
uint32_t mh_drive_struct_size(void);
/* mh_bank_render (one block of RenderModal, ModalAudio.cpp:486-555) with drives: signals is [n_drives][frames] float.  Per mode k of
 * its object a drive has the impact's gain, expression for expression (ImpactGainRow, ModalAudio.h:182-188):
 * rad_gain[k] * (shape_x[p,k]*jx + shape_y[p,k]*jy + shape_z[p,k]*jz); per sample the mode's excitation is the running sum of
 * f_row[t] * gain_row[k] from +0 over the object's impacts in impact order (:104-113), then over its drives in the order given here.
 * A sample that is not finite is rendered as 0.  A dealt object with a drive counts as excited like one with an impact: it is not
 * silenced, and the caller passes its tuned mode count as render_count.  A drive is left out when it names no object of the bank, an
 * object that is not dealt or has no modes, or an ex_pos beyond the object's shape columns.  With n_drives = 0 this is mh_bank_render. */
int mh_bank_render_driven(mh_bank *, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts,
                          uint32_t n_renderers, const uint32_t *deal_offset, const uint32_t *deal_objects, const uint32_t *render_count,
                          const uint32_t *tuned_count, const float *out_gain, const float *listener_gain, void *out, double *object_energy,
                          uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                          const mh_drive *drives, const float *signals);
/* TuneModalObject's DeflectionGain column (ModalAudio.cpp:380), [first, first+count): float for an fp32 bank, double for an fp64 bank.
 * Only pickups read it; a bank that never received it holds zeros there. */
int mh_bank_set_deflection_gain(mh_bank *, uint32_t first, uint32_t count, const void *deflection_gain);
/* A deflection pickup (no reference counterpart in ModalAudio; the bank-side primitive under the feedback reads of the reference's surface
 * renderer: ReadDeflection / ReadRow with ModeReadGains, src/audio/surface/): a read-only probe of `object`.  Per frame it returns the
 * object's modal displacement along (nx, ny, nz) at the blend weights[0..2] of the excitation positions points[0..2]
 * ({1,0,0} = points[0] alone), from the resonator state AFTER that frame's step.  Per mode k, in the bank's precision:
 *   shape = weights[0]*shape[points[0],k] + weights[1]*shape[points[1],k] + weights[2]*shape[points[2],k]   (x, y, z each)
 *   read  = scale * (shape_x*nx + shape_y*ny + shape_z*nz) * DeflectionGain[k]
 *   advance 0: g_im = read,                        g_re = 0
 *   advance 1: g_im = read * c_re,                 g_re = read * c_im
 *   advance 2: g_im = read * (c_re^2 - c_im^2),    g_re = read * (2 c_re c_im)
 * and frame s is the sum over the object's rendered modes of g_im[k]*Im z[k] + g_re[k]*Re z[k].  scale: the caller's coupling already
 * multiplied by the object's DeflectionScale. */
typedef struct {
    uint32_t object;
    uint32_t points[3];
    float weights[3];
    float nx, ny, nz;
    float scale;
    uint32_t advance;
} mh_pickup;
/* the most pickups one object can carry in a call; further ones (in the caller's order) are left out */
#define MH_PICKUPS_PER_OBJECT 8
/* sizeof(mh_pickup) as this library was built */
uint32_t mh_pickup_struct_size(void);
/* mh_bank_render_driven with pickups.  pickup_out is [n_pickups][frames] in the bank's precision, WRITTEN (not added to); pickup_read[q]
 * is 1 when pickup q was read, 0 when it was left out (its row is zeros then): an object the bank does not have or without modes, a
 * point beyond the object's shape columns, a weight, direction component or scale that is not finite, advance > 2, or more than
 * MH_PICKUPS_PER_OBJECT pickups on the object before it.  A pickup on an object that is not dealt (at rest) reads zeros and counts as
 * read.  Pickups observe: `out`, the state, the per-object results and the impacts are bit for bit those of the call without them.
 * A pickup's row depends on its object's state and its own record only (summation order: DESIGN.md section 3b).  With n_pickups = 0
 * this is mh_bank_render_driven. */
int mh_bank_render_read(mh_bank *, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts,
                        uint32_t n_renderers, const uint32_t *deal_offset, const uint32_t *deal_objects, const uint32_t *render_count,
                        const uint32_t *tuned_count, const float *out_gain, const float *listener_gain, void *out, double *object_energy,
                        uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                        const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out,
                        uint8_t *pickup_read);
/* A contact junction (no reference counterpart in ModalAudio; the bank-side primitive under the per-sample contact solve of the reference's
 * surface renderer, SolveChannelStep in src/audio/surface/, with a linear law): a unilateral -- or, MH_JUNCTION_BILATERAL, bilateral --
 * linear spring of stiffness K between a contact point on one bank object (side a) and either a second bank object (side b) or an
 * exciter the caller moves (b.object = MH_NO_OBJECT), solved implicitly once per frame inside the render call.  Passed with the block it
 * acts in; no state between blocks (but a damped junction's carry: "Contact damping" below).
 * A side is a pickup's contact point and a drive's direction in one record; (nx, ny, nz) is the direction in which the junction pushes
 * that side.  Per mode k of the side's object, in the bank's precision, with `shape` the pickup's blend (above):
 *   a[k]    = RadiationGain[k] * (shape_x*nx + shape_y*ny + shape_z*nz)            the drive gain (weights {1,0,0}: a drive's gain, bit for bit)
 *   read[k] = scale * (shape_x*nx + shape_y*ny + shape_z*nz) * DeflectionGain[k]   the pickup's `read`
 *   g_im[k] = read[k] * c_re[k],   g_re[k] = read[k] * c_im[k]                     the pickup's advance-1 row
 * With the junctions comes one approach signal u per junction, [n_junctions][frames] float: the rigid indentation the caller's physics
 * imposes (converted to the bank's precision like a drive's signal; a sample that is not finite counts as 0).
 * Per frame s, over the modes the block advances for each side's object (render_count: the caller passes the tuned count, an object on a
 * junction's side is excited for the block exactly as one with a drive is):
 *   1. the free step, as without the junction: z~ = z*c + e[s], e[s] the running sum over the object's impacts and drives;
 *   2. the free prediction of the next frame's deflection: d = sum_sides sum_k g_im[k]*Im z~[k] + g_re[k]*Re z~[k];
 *   3. the compliance, constant over the block: C = sum_sides sum_k g_re[k]*a[k]  (a force f at frame s enters Re z[s] and reaches
 *      Im z[s+1] through c_im: it moves the prediction by C f);
 *   4. x = u[s] - d;  f[s] = (K * max(x, 0)) / (1 + K*C);  bilateral: f[s] = (K * x) / (1 + K*C);
 *   5. Re z[k] = Re z~[k] + a[k]*f[s] on every side; the frame's output term is formed from that state.
 * So the force of frame s meets the spring law at the displacement of frame s + 1: f[s] = K*max(u[s] - sum read[k]*Im z[s+1][k], 0).
 * The sums of d and C have a fixed order that depends on the sides' mode counts only.
 * Returned per junction: the force row (force_out, [n_junctions][frames] in the bank's precision, WRITTEN, not added to), C as a double
 * (compliance_out) and a status byte (status_out): MH_JUNCTION_LEFT_OUT, MH_JUNCTION_SOLVED, or MH_JUNCTION_REFUSED -- 1 + K*C is not a
 * finite number above 0: f = 0 for the block and the objects render as with K = 0.
 * Left out (status 0, a zero row, C = 0; it excites nothing, like a dropped drive): a side naming no object of the bank, an object that is
 * not dealt, has no modes or renders none, a point beyond the object's shape columns, a weight, direction component, scale or K that is
 * not finite, K < 0, both sides the same object, an object already on a side of an earlier junction of the call that was not left out
 * (one junction per object, unless both junctions carry MH_JUNCTION_SHARED: "Groups" below), and a junction whose sides together take more than MH_JUNCTION_MODES / 128 waves of 128
 * rendered modes (each side's count rounded up to whole waves).  MH_JUNCTION_MODES = 1024 is what one workgroup holds: eight waves' output
 * tiles (16 640 B each) fill the 160 KiB of LDS; the registers (78 / 103 VGPRs in fp32 / fp64, nothing spilled, of the 256 a wave of an
 * eight-wave workgroup may take) would allow more.
 * In this version a pickup on an object that is on a junction's side is left out (pickup_read = 0, a zero row); mh_bank_render_observed
 * reads it ("Pickups on junction objects" below).
 *
 * The Hertzian law, flags & MH_JUNCTION_HERTZ: `stiffness` is K in N/m^1.5 and the junction obeys f = K * delta^(3/2), the law of
 * ContactModel (modal/contact.hpp).  Steps 1, 2, 3 and 5 are the ones above, bit for bit -- the free step, d, C, Re z = Re z~ + a*f[s], the
 * output term, the summation orders, the force row written in the bank's precision.  Step 4 becomes the implicit solve of the law:
 *   4h. x = u[s] - d.  If x > 0 fails (a NaN included): f[s] = 0.  Otherwise, with c = K*C formed once per block in the bank's precision,
 *       y is the root of  y + c*y*sqrt(y) = x  -- the compression of frame s + 1, since y = x - C*f -- and f[s] = (K*y)*sqrt(y).
 * So, as with the linear law, f[s] = K*max(u[s] - sum read[k]*Im z[s+1][k], 0)^(3/2) holds as an identity; the solve is what keeps a stiff
 * contact from overshooting.  The root is found by one fixed expression tree (the bits depend on it), every operation rounded to the bank's
 * precision, nothing contracted, no trip count that depends on data:
 *   y = x;
 *   if (c > 0) { g = cbrt(x / c); g = g*g; if (g < x) y = g; }       x and (x/c)^(2/3) both bound the root from above, and the smaller is
 *                                                                    within a factor 2 of it
 *   four times:  r = sqrt(y);  y = y - ((y + (c*y)*r) - x) / (1 + (1.5*c)*r);
 *   f = (K*y)*sqrt(y);
 * (Newton's steps on a convex increasing function from above: four of them leave f within 2.6 eps of the exact root's in float and in
 * double over c*sqrt(x) = 1e-8 ... 1e8; three are enough in float only.  A start value off by 1e-3 changes nothing, so cbrt need not be
 * correctly rounded.  x = 0, c = 0 (then y = x) and c = 1e30 give finite results.)  x is taken to be finite: u is (a sample that is not
 * is 0), and d is while the state is; where u[s] - d overflows the bank's precision, f[s] is not finite -- as the linear law's is not.
 * Status of a Hertz junction: MH_JUNCTION_REFUSED when C < 0, or C or K*C is not finite (1 + K*C plays no part); C = 0 is solved, f = K*x^1.5.
 * A refused junction gives a zero row and its objects render as with K = 0, as above.
 * MH_JUNCTION_HERTZ | MH_JUNCTION_BILATERAL is left out (status 0, a zero row, C = 0): the law has no tension branch.  Every other
 * left-out kind is as above.  Not in this version: a hysteretic law, roughness, other exponents (friction: "Friction" below; the damped -- Hunt-Crossley --
 * law and its state between blocks: "Contact damping" below).
 *
 * Groups, flags & MH_JUNCTION_SHARED: several junctions on one object (a bowl on three points, a table under several objects, a bar on two
 * supports under a mallet).  A junction with the flag may name an object that is already on a side of an earlier kept junction, provided
 * that junction carries the flag too.  A junction without it is treated as above: it is left out when it names an object of a kept
 * junction, and a later flagged junction on one of its objects is left out.  The kept flagged junctions of a call fall into connected
 * components over the objects they name (two junctions are connected when they share an object; an exciter side connects nothing).
 * A component of one junction is an ordinary junction -- the five steps above, linear or Hertz, bit for bit: the flag on a lone junction
 * changes nothing.  A component of 2 ... MH_JUNCTION_GROUP junctions is a GROUP of n members i = 0 ... n-1 in call order, solved together:
 *   1, 2. as above per member: d_i sums over member i's own sides, side a's modes, then side b's (DESIGN.md section 3c's order).
 *   3.  a matrix, constant over the block:  C_ij = sum over the objects o on a side of both i and j -- side a of i, then side b of i --
 *       of sum_k g_re_{i,o}[k] * a_{j,o}[k]  (a force f_j at frame s moves member i's prediction by C_ij f_j).  C_ii is the C of step 3
 *       above and what compliance_out[i] returns.
 *   4.  x_i = u_i[s] - d_i.  f is the solution of:  y = x - C f;  f_i = K_i max(y_i, 0)  (bilateral: f_i = K_i y_i)  for every member at
 *       once, so that every member's force meets its law at the displacement of frame s + 1.  With f = K y this is (I + C diag(K)) y = x
 *       on the members in contact.  TuneModalObject makes C a positive diagonal times a Gram matrix, so I + C diag(K) is a P-matrix (its
 *       principal minors are those of I + diag(K) C, all above 0) and the problem has exactly one solution.  It is found by enumerating
 *       the active sets, with no trip count that depends on data:
 *       Per block, for each subset A of the members that contains every bilateral one (bit i of the mask = member i; at most 16):
 *         M_A = (I + C_AA diag(K_A))^-1 in the bank's precision by the elimination of [B | I] over the members of A without pivoting, in
 *         ascending order:  B_ij = C_ij*K_j, plus 1 on the diagonal (1 + C_ii*K_i);  for p in A ascending: r = 1 / B_pp; row p of both
 *         halves times r;  for every i != p in A: t = B_ip; row i = row i - t * row p.  Nothing contracted.
 *       Per frame, for each such A:  y_i = sum_{j in A} M_ij*x_j (ascending j, from +0) and f_i = K_i*y_i on A, f_i = +0 off it.  A is
 *         CONSISTENT when y_j > 0 for every unilateral j in A and  x_j - sum_{i in A} C_ji*f_i > 0  (ascending i, from +0) fails for
 *         every j outside A.  Taken: the consistent subset of lowest mask.  The empty set is consistent exactly when no x_j > 0: a group
 *         out of contact gives exact zeros.
 *       If rounding leaves no subset consistent (x within a rounding of a boundary between two active sets, where both neighbours fail by
 *         that rounding): the subset that fails by least is taken -- the largest over its members of -y_j (unilateral j in A) and of the
 *         residual above (j outside A), above 0; lowest mask among equals -- with f_j = K_j*max(y_j, 0) on its unilateral members.  (The
 *         full set's clamped candidate, the obvious last resort, jumps there: tests/test_bank_groups_cpu.py.)
 *   5.  On each object  Re z[k] = (...((Re z~[k] + a_{j1}[k]*f_{j1}) + a_{j2}[k]*f_{j2})...)  over the members with a side on it, in
 *       ascending call order; the frame's output term is formed from that state.
 * M_{i} of a single member is formed by the same elimination, 1 / (1 + C_ii*K_i) times x and then times K_i: not the bits of step 4's
 * (K*x) / (1 + K*C).  A lone junction never takes this path, and a group compared with itself (other members dead) does on both sides.
 * Status: every member of a group gets MH_JUNCTION_REFUSED when a C_ij or C_ij*K_j is not finite or a pivot of an M_A is not a finite
 * number above 0 -- zero rows, the objects render as with K = 0 -- and MH_JUNCTION_SOLVED otherwise; compliance_out[i] = C_ii either way.
 * Left out (status 0, a zero row, C = 0, excites nothing), decided in call order: a flagged junction that would make a component larger
 * than MH_JUNCTION_GROUP; one with which the component's distinct objects would take more than MH_JUNCTION_MODES / 128 waves of 128
 * rendered modes (each object counted once, however many sides name it); one with MH_JUNCTION_HERTZ that would join a component of more
 * than one junction, and one that would join a component that holds a Hertz junction (the Hertz solve in more than one dimension is not in
 * this version); a flagged junction on an object of a kept unflagged one.  Two junctions between the same pair of objects, at different
 * points, are a legal group.  Pickups on a junction's object stay left out (mh_bank_render_observed reads them).  MH_JUNCTION_GROUP = 4 is what a wave's registers hold: one
 * gain triple per member per lane, 195 VGPRs in fp64 (118 in fp32), nothing in scratch.  (Hertz in groups: mh_bank_render_mixed; damping in groups:
 * mh_bank_render_damped_groups.)  Not in this version, as above: friction inside groups, roughness.
 *
 * Contact damping, flags & MH_JUNCTION_DAMPED (mh_bank_render_damped only: mh_bank_render_coupled ignores the bit): the Hunt-Crossley
 * term of the reference's surface renderer (DampingFactor = 1.5 (1 - e) ContactDamping, src/audio/surface/).  The junction obeys
 *     f = K * phi(y) * max(1 + l*(y - y_p), 0),    phi(y) = max(y, 0), or max(y, 0)^1.5 with MH_JUNCTION_HERTZ,
 * where y = x - C*f is the compression of frame s + 1 (the quantity step 4 is implicit in), y_p the compression the previous frame's
 * solve left (signed: a negative value is a gap) and l >= 0 the damping in 1/m per frame (damping[j]; a caller with D in s/m passes
 * l = D * sample rate).  The max(..., 0) is the non-adhesion clamp: a contact that opens faster than 1/l per frame gives no force.
 * Steps 1, 2, 3 and 5 stay bit for bit; step 4 becomes the implicit solve of this law, so that f[s] = K phi(y[s]) max(1 + l (y[s] -
 * y[s-1]), 0) holds as an identity.  One fixed expression tree per law, every operation rounded to the bank's precision, nothing
 * contracted, no trip count that depends on data; c = K*C and cl = c*l are formed once per block; min(a, b) is b < a ? b : a; on a frame
 * without history (below) l = 0, cl = 0 and y_p = 0 in every expression:
 *   4d. x = u[s] - d.  If x > 0 fails (a NaN included): f = +0, y = x.  Otherwise m_x = 1 + l*(x - y_p); if m_x > 0 fails: f = +0, y = x
 *       (exact, not a heuristic: g(y) = y + c phi(y) max(1 + l (y - y_p), 0) - x is convex and increasing, and its root lies above the
 *       kink y_p - 1/l exactly when m_x > 0).  Otherwise, with m0 = 1 - l*y_p:
 *       linear:  B = 1 + c*m0;  r = sqrt(B*B + (4*cl)*x);  y = min(x, B >= 0 ? (2*x)/(B + r) : (r - B)/(2*cl));
 *                (B < 0 implies cl > 0; x bounds the root from above.  Where B*B overflows -- |c*(1 - l*y_p)| above 1.8e19 in float, 1.3e154
 *                in double, far outside any physical damping -- the min keeps y and f finite and f >= 0, NOT accurate: r is infinite there,
 *                so y = 0 and f = 0 for B >= 0, and y = x for B < 0.  The quadratic is not rescaled: its bits in the range that occurs
 *                are what the tree above gives.)
 *                m = 1 + l*(y - y_p);  if (!(m > 0)) m = 0;  f = (K*y)*m;
 *       Hertz:   big = the largest finite number;  p5 = cl > 0 ? exp2(0.4*log2(x/cl)) : big;
 *                if (m0 >= 0) { cm = c*m0;  t = cbrt(x/cm);  g = cm > 0 ? t*t : big;  y = min(min(x, g), p5); }
 *                else         { ylo = -m0/l;  lin = x/((cl*ylo)*sqrt(ylo));  y = min(x, ylo + min(lin, p5)); }
 *                six times:   r = sqrt(y);  m = 1 + l*(y - y_p);  q = (c*y)*r;
 *                             y = y - ((y + q*m) - x) / ((1 + ((1.5*c)*r)*m) + q*l);
 *                m = 1 + l*(y - y_p);  if (!(m > 0)) m = 0;  f = ((K*y)*sqrt(y))*m;
 *       Every candidate start bounds the root from above (x; the roots of the equation with one of its terms alone), so Newton's steps
 *       descend on a convex increasing function.  Measured in float and in double over c (Hertz: c sqrt(x)) = 1e-8 ... 1e8, x = 1e-12 ... 1,
 *       l*x = 0 and 1e-6 ... 1e6, y_p/x in [-3, 3], against bisection in long double, as |f - f*| over K phi(y*) (1 + l (|y*| + |y_p|))
 *       (the plain relative error of f means nothing where 1 + l (y - y_p) cancels): tests/test_bank_damped_cpu.py holds the figures.  exp2,
 *       log2 and cbrt need not be correctly rounded (a start off by 1e-3 changes nothing).  The final clamp on m is needed: rounding can
 *       leave m one rounding below 0.
 * State: one value per junction, `carry` ([n_junctions], the bank's precision, in and out).  On entry a value that is not finite means
 * "no history": frame 0 is solved with l = 0 and y_p = 0 and its y starts the history.  On return: the last frame's y -- the root
 * itself, never x - C*f, which loses every digit on a stiff contact -- for a damped junction that was solved; a quiet NaN for every other
 * junction (undamped, left out, refused).  With frames = 0 the carry comes back unchanged.
 * With the bit set and l = 0 the junction takes the damped tree and returns a carry; its bits need not be those of the undamped law.
 * Status: MH_JUNCTION_REFUSED (a zero row, the objects render as with K = 0, carry NaN) for a damped junction, linear or Hertz, when
 * C < 0, or C, K*C or K*C*l is not finite (1 + K*C plays no part).  Left out (status 0, a zero row, C = 0, carry NaN, the bits of the call
 * without the junction): a damped junction whose l is not finite or below 0; MH_JUNCTION_DAMPED | MH_JUNCTION_BILATERAL (the clamp has no
 * tension branch); a damped junction that would join a component of more than one junction, and a junction that would join a component
 * that holds a damped one (decided with the groups, modalhip_groups.hpp).  A lone damped junction with MH_JUNCTION_SHARED is an ordinary
 * damped junction.  Every junction without the bit keeps its bits beside a damped one, and a call in which no kept junction has the bit
 * launches what mh_bank_render_coupled launches.
 * Not in this version: a bilateral damped law (damping in groups: mh_bank_render_damped_groups, below), hysteretic laws, friction on a damped junction, roughness, pickups on junction objects
 * (in this entry: mh_bank_render_observed reads them, "Pickups on junction objects" below).
 *
 * Pickups on junction objects, mh_bank_render_observed: mh_bank_render_damped -- its parameters in its order, nothing more -- except that a
 * pickup whose object is on a side of a KEPT junction (status solved or refused; a lone linear, Hertz or damped junction, or a member of a
 * group) is read.  Every other pickup, and every left-out kind of mh_bank_render_read -- an unknown object or one without modes, a point
 * beyond the shapes, a value that is not finite, advance > 2, more than MH_PICKUPS_PER_OBJECT on the object before it -- is as it is
 * there; an object on a LEFT-OUT junction is rendered by the main launch and read there, as today.
 * A row: frame s is the sum over the object's rendered modes of  g_im[k]*Im z[s][k] + g_re[k]*Re z[s][k],  with the pickup's gains of
 * mh_bank_render_read (`read`, advance 0, 1 or 2) and z[s] the state AFTER step 5 of frame s:  Re z = Re z~ + sum_j a_j*f_j[s],  the state
 * the frame's output term is formed from.  The advance is free: no contact force acts in the look-ahead.
 * Consequence: with advance-1 pickups at a junction's own sides (same points, weights, direction and scale),
 *     sum_sides read1[s] = d + C*f[s]      (step 2's prediction moved by the frame's force),
 * so  u[s] - sum_sides read1[s]  is the compression y of frame s + 1, the quantity every law above is implicit in:
 * f[s] = K*phi(u[s] - sum read1[s]) (times the damping factor for a damped junction) can be checked where it is solved, in either
 * precision, whatever else excites the objects.  For a damped junction the last frame's value is the returned carry, up to rounding.
 * Summation order: mh_bank_render_read's, unchanged.  Per (wave of 128 modes from the object's mode 0, half of 64
 * modes): acc = fma(g_im[k], Im z[k], acc), then acc = fma(g_re[k], Re z[k], acc), even modes into one accumulator and odd modes into a
 * second, k ascending from +0, the value even + odd; the partial rows are added in ascending (wave, half) order from +0.  The junction
 * kernels cut each object into waves at the same modes 0, 128, ..., so the partition is the same and a row depends on its object's state
 * trajectory and its own record only -- not on the deal, the renderer count, which kernel rendered the object, a tile length or anything
 * else in the call.  This is part of the contract: a row is bit for bit the row mh_bank_render_read gives for the same trajectory.
 * Pickups only observe: with the pickups on junction objects removed from the call, `out`, every state, the per-object results, the
 * force rows, compliances, statuses and carries are the same bits.  A refused junction's objects render as with K = 0 and are read.
 * With frames = 0 nothing is read and the carry comes back unchanged.  A call without a pickup on a kept junction's object launches
 * exactly what mh_bank_render_damped launches.  mh_bank_render_coupled and mh_bank_render_damped keep leaving such pickups out.
 * Not in this version: a bilateral damped law (Hertz inside groups: mh_bank_render_mixed, damping inside groups:
 * mh_bank_render_damped_groups, below; friction: mh_bank_render_friction, "Friction" below),
 * roughness, contact forces acting inside a pickup's look-ahead.
 *
 * Hertz junctions in groups, mh_bank_render_mixed: mh_bank_render_observed -- its parameters in its order -- followed by one output,
 * unconverged_out [n_junctions].  One difference: a kept junction with MH_JUNCTION_SHARED | MH_JUNCTION_HERTZ may be a member of a group,
 * beside linear unilateral, bilateral and other Hertz members (the group decision of modalhip_groups.hpp with hertz_in_groups = true).
 * Still left out, in call order, with the bits of the call without them: Hertz with bilateral, a damped junction in a group, a fifth
 * member, a ninth wave, a flagged junction on an unflagged junction's object.  A group without a Hertz member runs the enumeration of
 * MH_JUNCTION_SHARED, bit for bit, and a call without a Hertz junction in a group launches what mh_bank_render_observed launches.
 * A group with a Hertz member takes the steps of MH_JUNCTION_SHARED: steps 1, 2, 3 and 5 bit for bit (the free step, d_i, C_ij and their
 * summation orders, Re z = (...(Re z~ + a_j1 f_j1) + ...), the rows in the bank's precision).  Step 4 becomes
 *   4m. find y with y = x - C f(y): f_j = K_j max(y_j, 0) (linear), K_j y_j (bilateral), K_j max(y_j, 0)^1.5 (Hertz).  As with every law
 *       the force of frame s meets the law at the displacement of frame s + 1.  C = D G, a positive diagonal times a Gram matrix, so the
 *       problem is D^-1 x in G f + D^-1 phi^-1(f), a monotone operator plus a strictly monotone diagonal one: exactly one solution when
 *       every K_j > 0; a member with K_j = 0 has f_j = 0 and drops out.
 *       One fixed expression tree, every operation rounded to the bank's precision, nothing contracted (the one fused multiply-add below
 *       is written as such), no trip count that depends on data, no state between frames (a warm start would make the bits depend on
 *       the block length).  With ck_jj = C_jj K_j (once per block), phi_j(y) = p sqrt(p) with p = max(y, 0) (Hertz), y (bilateral),
 *       max(y, 0) (linear), phi'_j = 1.5 sqrt(p), 1, [y > 0], and f_j = K_j phi_j(y_j), kd_j = K_j phi'_j(y_j) formed after every change of y_j:
 *         alone_j(x): Hertz: x for x <= 0, else step 4h's tree up to y (the smaller of x and cbrt(x / ck_jj)^2, taken when ck_jj > 0;
 *                     four steps y -= ((y + (ck_jj y) sqrt(y)) - x) / (1 + (1.5 ck_jj) sqrt(y))); linear: x / (1 + ck_jj) for x > 0
 *                     or a bilateral member, else x.
 *         start:      y_j = alone_j(x_j), j ascending.
 *         1 sweep:    j ascending: y_j = alone_j(x_j - s), s = sum over i != j, ascending from +0, of C_ji f_i  (Gauss-Seidel).
 *         residual:   plain: F_i = (y_i + sum_j C_ij f_j, ascending from +0) - x_i.  In twice the precision: s = y_i, c = +0; j ascending:
 *                     p = C_ij f_j, e = fma(C_ij, f_j, -p), (s, r) = two_sum(s, p), c = c + (r + e); then (s, r) = two_sum(s, -x_i),
 *                     c = c + r; F_i = s + c.  two_sum(a, b): s = a + b, bb = s - a, r = (a - (s - bb)) + (b - bb).
 *         10 steps:   J_ij = C_ij kd_j, J_ii = 1 + C_ii kd_i; J d = F by elimination without pivoting in ascending order (inv = 1 / J_pp;
 *                     row p's later entries and r_p times inv; every later row i: t = J_ip, J_ij -= t J_pj, r_i -= t r_p), back
 *                     substitution in descending order (d_p = (...(r_p - J_p,p+1 d_p+1) - ...)); y_j = y_j - d_j; the residual of the
 *                     new y.  The residuals after steps 9 and 10 are the ones in twice the precision, the others plain: the last
 *                     step is one of iterative refinement, and the residual test sees the residual itself, not its rounding.
 *         The forces are the f_j of the last y.
 *       The residual is written in the forces the solve returns, f_j rounded, not in C_ij K_j: the y found satisfies y = x - C f for
 *       those very numbers, and the roundings of K phi(y) perturb the law by 1.5 u instead of being amplified by the elimination.
 *       The group is padded to MH_JUNCTION_GROUP members with K = 0, C = 0, x = 0, which changes no bit.
 *       The residual test of a frame: with F of the final y, some |F_i| > 16 u (|y_i| + sum_j |C_ij| |f_j| + |x_i|), u the unit roundoff.
 *       F_i has 6 terms; the last place of y_i (1 rounding) and of each f_j (3: the root, the product, K) moves F_i by up to 2 u of
 *       the magnitudes summed, which is how close to 0 the last step can bring it; the multiple is 8 times that.
 *       unconverged_out[j]: for a member of a group with a Hertz member, the number of
 *       frames of the block that failed the test; 0 for every other junction.  A correct solve on valid input returns 0 everywhere; a
 *       count above 0 says that the block's forces are not at the law.
 *       Accuracy (tests/test_bank_mixed_cpu.py, 36 sets of 1 000 cases): |f - f*| / max |f*| is 1.4 - 2.3 eps in every set, float32 and
 *       float64; against the error of step 4's linear solve on the linearisation at the solution that is 0.00 - 1.19 x (4 x allowed,
 *       2.4 x asserted).  (Sweeps, steps) = (1, 10) is a smallest pair: with 9 steps, or without the sweep, sets miss by factors of
 *       thousands; 0, 2 and 3 sweeps need 13, 12 and 12 steps.  The tests' numpy restatement forms the product's error e by Veltkamp's
 *       splitting where the device uses the fused multiply-add: the two are the same bits while neither the split (|C_ij|, |f_j| below
 *       the largest number / 2^27 in fp64, / 2^12 in fp32) nor e (|C_ij f_j| above the smallest normal number times 2^53, 2^24) leaves
 *       the format's range; outside it only the last step's correction differs, by less than the residual test resolves.
 * Status: refused (every member, zero rows, the objects render as with K = 0) when a C_ij or C_ij K_j is not finite, a |C_ij K_j| is
 * above the square root of the largest finite number (the elimination multiplies two entries of J), C_ii or C_ii K_i is below 0 on a Hertz
 * member, or 1 + C_ii K_i is not a finite number above 0 on a linear one; solved otherwise.  compliance_out[i] = C_ii in both cases.
 * k_bank_modes_grouped<Real, OBSERVE, true>: the same solve in every lane of every wave; 230 / 246 VGPRs (fp32 / fp64), nothing in scratch;
 * 512-frame blocks on an MI355X, n = 2 ... 4: fp32 20 600 - 27 100 cycles per frame, 4.6 - 6.1 ms; fp64 24 600 - 31 200 cycles, 5.4 - 6.9 ms.
 * Not in this version: a bilateral Hertz or damped law, more than four members, friction inside groups, roughness (damping inside groups:
 * mh_bank_render_damped_groups, next).
 *
 * Damped junctions in groups, mh_bank_render_damped_groups: mh_bank_render_mixed -- its parameters in its order and nothing more.  One
 * difference: a kept junction with MH_JUNCTION_SHARED | MH_JUNCTION_DAMPED, linear or Hertz, may be a member of a group, beside linear
 * unilateral, bilateral, Hertz and other damped members (the group decision of modalhip_groups.hpp with damped_in_groups = true).
 * Still left out, in call order, with the bits of the call without them: damped with bilateral, an l (damping[j]) that is not finite or
 * below 0, Hertz with bilateral, a fifth member, a ninth wave, a flagged junction on an unflagged junction's object.  A group with a
 * Hertz member and no damped one runs step 4m's kernel bit for bit, a linear group the enumeration of MH_JUNCTION_SHARED, a lone damped
 * junction k_bank_modes_coupled_damped: a call without a damped junction in a group launches exactly what mh_bank_render_mixed launches.
 * A group with a damped member takes steps 1, 2, 3 and 5 of MH_JUNCTION_SHARED bit for bit.  Step 4 becomes
 *   4g. find y with y = x - C f(y): f_j = K_j phi_j(y_j) max(1 + l_j (y_j - y_p,j), 0) on a damped member, phi_j = max(y, 0) or
 *       max(y, 0)^1.5 (MH_JUNCTION_HERTZ); step 4m's law on every other member.  y_p,j is the compression that member's solve left in the
 *       previous frame.  For l >= 0 each f_j is continuous and nondecreasing in y_j (on y >= 0 a product of two factors that are not below
 *       0 and do not decrease; 0 elsewhere), so with C = D G two solutions y, y' give sum_j df_j dy_j / D_j + df' G df = 0 with both terms
 *       >= 0: G df = 0, then dy = -C df = 0 -- exactly one solution, as in step 4m.
 *       The carry: one value of state per damped member, through `carry` in and out, with step 4d's meaning.  Not finite on entry: no
 *       history for this member -- frame 0 is solved with l_j = 0, y_p,j = 0 and its y_j starts the history.  On return: the last frame's
 *       y_j of the final iterate (never x - C f), for a damped member of a solved group; a quiet NaN for every other junction; frames = 0
 *       leaves it alone.  The solve keeps no other state between frames: one block of N frames and two of N / 2 with the carry passed
 *       on are the same bits.
 *       One fixed expression tree as in step 4m: every operation rounded to the bank's precision, nothing contracted, no trip count
 *       that depends on data.  With ck_jj = C_jj K_j, c15_jj = 1.5 ck_jj (once per block), l_j and y_p,j as this frame takes them (0
 *       without history), (phi_j, phi'_j) of step 4m, kp = K_j phi_j(y_j), kq = K_j phi'_j(y_j), formed after every change of y_j:
 *         law_j:      not damped: f_j = kp, kd_j = kq.  Damped: m = 1 + l_j (y_j - y_p,j); for m > 0 f_j = kp m, kd_j = kq m + kp l_j;
 *                     otherwise f_j = +0, kd_j = 0.
 *         alone_j(x): damped: step 4d's tree up to y, with c = ck_jj, c15 = c15_jj, cl = ck_jj l_j (x for x <= 0 or 1 + l_j (x - y_p,j)
 *                     <= 0; linear: the closed form; Hertz: the smallest of the upper bounds, six Newton steps); else step 4m's alone_j.
 *         start:      y_j = alone_j(x_j), j ascending.
 *         1 sweep:    j ascending: y_j = alone_j(x_j - s), s = sum over i != j, ascending from +0, of C_ji f_i.
 *         residual:   step 4m's, plain and in twice the precision, in the f_j above.
 *         8 steps:    J_ij = C_ij kd_j, J_ii = 1 + C_ii kd_i; J d = F by step 4m's elimination; t_j = y_j - d_j.  In steps 1 - 6 a
 *                     member that is not bilateral with kd_j = 0 or t_j > 2 y_j takes y_j = alone_j(t_j + C_jj (f_j + kd_j (t_j - y_j)))
 *                     -- its own tree at its row's linearised right-hand side, x_j - sum_{i != j} C_ji (f_i + kd_i dy_i): from below the
 *                     root Newton's iteration on a convex law lands far above it and creeps back by 0.6 per step, and an open or clamped
 *                     member (kd = 0) comes back at x_j - s --; every other member, and every member in steps 7 and 8, y_j = t_j.
 *                     Then law_j and the residual of the new y: plain after steps 1 - 5, in twice the precision after steps 6, 7
 *                     and 8 -- the last two steps are iterative refinement.
 *         The forces are the f_j of the last y; the carries its y_j.
 *       The final clamp on m is step 4d's: m <= 0 gives f_j = +0.  The group is padded to MH_JUNCTION_GROUP members with K = 0, C = 0,
 *       x = 0, which changes no bit.
 *       The residual test of a frame: some |F_i| > 32 u (|y_i| + sum_j |C_ij| s_j + |x_i|), with s_j = kp (1 + l_j (|y_j| + |y_p,j|)) on
 *       a damped member and |f_j| on every other.  A damped f_j has 7 roundings where step 4m's has 3: the root, the product and K
 *       (kp), then y - y_p, times l, plus 1 -- each within u of l (|y| + |y_p|) or of 1 + l (|y| + |y_p|), whatever m cancels to -- and
 *       the product kp m; the last place of y_j moves m by another u l |y_j|.  That is 8 u s_j per member against step 4m's 4 u |f_j|:
 *       the sum the last step can reach is 4 u of the magnitudes, and the multiple is 8 times that as in step 4m.  (With |f_j| in the
 *       place of s_j a stiff member whose m has cancelled to 1e-4 settles at 1e3 u and fails a test it has met.)
 *       unconverged_out[j]: for a member of a group with a Hertz or a damped member, the frames of the block that failed its test.
 *       Accuracy (tests/test_bank_damped_groups_cpu.py, section 3h's 36 sets of 1 000 cases with about half the unilateral members
 *       damped, l |x| = 0 and 1e-3 ... 1e3, y_p / x in [-3, 3]): |f - f*| / max_j s_j(y*) against the error of step 4's linear solve on
 *       the linearisation at the solution is at most 1.31 x (4 x allowed, 2.62 x asserted); the largest final |F_i| is 3.5 u of the
 *       magnitudes summed.  (Sweeps, steps, refined) = (1, 8, 2) is a smallest triple: with 7 steps 6 cases of 36 000 fail the residual
 *       test, without the sweep 12 (and a set misses the margin by 3.7e5), with one refined step 3.  Without the step through alone_j
 *       19 steps are needed.
 * Status: step 4m's conditions with a damped member counted as a Hertz one (C_ii and C_ii K_i not below 0), plus, on a damped member,
 * C_ii K_i l_i a finite number not below 0 and every |C_ij K_j l_j| within the square root of the largest finite number (kd_j holds
 * K_j phi l_j, and the elimination multiplies two entries of J; what kd_j becomes beyond that depends on y and cannot be decided per
 * block).  A refused group: every member status 2, zero rows, NaN carries, the objects render as with K = 0.
 * k_bank_modes_grouped<Real, OBSERVE, true, true>: C, K, ck, c15, l and the iterate in scalar registers, y_p per member in registers from frame to
 * frame, no barrier, LDS slot or global access per frame beyond step 4m's; the carries are written once after the loop.  Resources:
 * profiles/bank_damped_groups_resources.txt.  512-frame blocks on an MI355X, n = 2 ... 4: fp32 35 500 - 45 200 cycles per frame, 7.8 - 10.0 ms;
 * fp64 47 600 - 58 900 cycles, 10.4 - 12.8 ms: beyond the 10.67 ms of real time for n = 3 and 4.
 * Not in this version: a bilateral damped or Hertz law, more than four members, friction inside groups, roughness, hysteretic laws, a warm start of the
 * Newton iteration from the previous frame (the bits would depend on the block length).
 *
 * Friction, flags & MH_JUNCTION_FRICTION (mh_bank_render_friction only: every older entry ignores the bit): Coulomb friction with stiction
 * on a lone junction -- the tangential channel of the reference's surface contact (SolveVoiceFriction, src/audio/surface/).  Beside its
 * normal law (linear or Hertz, unilateral) the junction carries one slider behind one stick spring.  friction[j] (mh_friction) holds a
 * tangent per side (ta, tb: a positive f_t pushes side a's modes along ta and side b's along tb, exactly as f does along n; a two-sided
 * caller passes tb = -ta, as it passes opposite normals), the Coulomb coefficient mu and the stick spring's stiffness kt in N/m.  Per mode of
 * a side, in the bank's precision, with the side's blended shape:  a_t = RadiationGain*(shape . t),  read_t = scale*(shape . t)*
 * DeflectionGain,  gt_im = read_t*c_re,  gt_re = read_t*c_im  -- the gains of the normal channel with t in the place of n.
 * A second signal per junction comes beside `approach`: `travel`, [n_junctions][frames] float, w: the rigid tangential offset of the two
 * surfaces -- a position, as u is; a sample that is not finite counts as 0.  State: one value per junction, `anchor` ([n_junctions], the
 * bank's precision, in and out), q: where the slider stands.  A value that is not finite means "no history": the frame takes q = x_t (on
 * entry: frame 0).  On return: q after the last frame for a frictional junction that was solved, a quiet NaN for every other junction;
 * frames = 0 leaves it alone.  The solve keeps no other state: one block of N frames and two of N / 2 with the anchor passed on are the
 * same bits.
 * The law: f_t = kt*(e - q) while |f_t| <= mu*f_n (stick: q stays); otherwise |f_t| = mu*f_n and the slider moves in the direction of the
 * force, to q = e - f_t/kt (slip).  An open contact carries no shear and the slider follows it (q = x_t).  e is the tangential relative
 * displacement of the contact points in frame s + 1 and y the compression of frame s + 1: as with every law here, the forces of frame s
 * meet the law at the displacements of frame s + 1.
 *   1, 2. as in mh_bank_render_coupled, bit for bit, for d_n; a second sum d_t = sum_sides sum_k gt_im[k]*Im z~[k] + gt_re[k]*Re z~[k] with the
 *       same lane part, the same tree and the same order.
 *   3.  four compliances, constant over the block, each with step 3's summation order:  C_nn = sum g_re*a (the bits of step 3's C, and
 *       what compliance_out returns),  C_nt = sum g_re*a_t,  C_tn = sum gt_re*a,  C_tt = sum gt_re*a_t.  C_nt and C_tn are equal in exact
 *       arithmetic; each is used where it arises, C_nt in the normal row and C_tn in the tangential one.  Also once per block, nothing
 *       contracted:  den = 1 + kt*C_tt;  beta = (kt*C_tn)/den;  C_S = C_nn - C_nt*beta;  C_P = C_nn + mu*C_nt;  C_M = C_nn - mu*C_nt;  and for
 *       each C_b of the three:  K*C_b,  1.5*(K*C_b),  1 + K*C_b.
 *   4t. x_n = u[s] - d_n,  x_t = w[s] - d_t.  If q is not finite: q = x_t.  N(x, C_b) is the scalar solve of the junction's normal law:
 *       linear (K*max(x, 0)) / (1 + K*C_b), step 4's expression; Hertz step 4h's tree with c = K*C_b.
 *       If x_n > 0 fails (a NaN included): f_n = f_t = +0, q = x_t (branch O).  Otherwise r = x_t - q, alpha = (kt*r)/den, and three
 *       candidates:
 *         S (stick):   x_S = x_n - C_nt*alpha;  f_n = N(x_S, C_S);  f_t = alpha - beta*f_n;  q' = q;
 *                      consistent when |f_t| <= mu*f_n;  miss |f_t| - mu*f_n.
 *         P (slip +):  f_n = N(x_n, C_P);  f_t = mu*f_n;  e = (x_t - C_tn*f_n) - C_tt*f_t;  q' = e - f_t/kt;
 *                      consistent when q' >= q;  miss kt*(q - q').
 *         M (slip -):  f_n = N(x_n, C_M);  f_t = -(mu*f_n);  e and q' as in P;  consistent when q' <= q;  miss kt*(q' - q).
 *       Taken: the first consistent candidate in the order S, P, M; where rounding on a boundary leaves none, the one with the least miss,
 *       the earlier one on a tie (the rule of "Groups").  q becomes the taken candidate's q'.
 *       The stick candidate's elimination is exact: f_t*(1 + kt*C_tt) = kt*(x_t - q - C_tn*f_n) put into y = x_n - C_nn*f_n - C_nt*f_t leaves
 *       the normal law alone on (x_S, C_S); C_S is a Schur complement of a Gram matrix, so it is not below 0.  Nothing is iterated that
 *       the bank does not already iterate, no trip count depends on data, and there is no state but q.
 *   5.  Re z[k] = Re z~[k] + (a[k]*f_n + a_t[k]*f_t) on every side, the inner sum formed first -- the association in which two drives with
 *       the signals f_n and f_t excite the object --; the frame's output term is formed from that state.
 * Returned besides force_out (f_n), compliance_out (C_nn) and status_out: tangent_out, [n_junctions][frames] in the bank's precision, the f_t
 * rows, WRITTEN; the new anchor; friction_counts_out, [n_junctions][3]: the frames taken on S, the frames taken on P or M, and the frames
 * on which no candidate was consistent (they are counted under the candidate taken as well).  Zeros for every junction that is not a
 * solved frictional one.  On valid input the third count is small: a diagnostic in the sense of unconverged_out, not an error.
 * Status: MH_JUNCTION_REFUSED (zero rows, a NaN anchor, the objects render as with K = 0) on the normal law's own conditions, and when
 * C_tt, C_nt or C_tn is not finite, C_tt < 0, den is not a finite number above 0, C_P or C_M is not a finite number from 0 up -- that is
 * mu*|C_nt| <= C_nn, the condition under which exactly one candidate is consistent (tests/test_bank_friction_cpu.py counts them) --, or a
 * K*C_b is not finite.
 * Left out (status 0, zero rows, C = 0, a NaN anchor, the bits of the call without the junction): the flag together with
 * MH_JUNCTION_BILATERAL, MH_JUNCTION_DAMPED or MH_JUNCTION_SHARED; a tangent component, mu or kt that is not finite; mu < 0 or kt < 0; every
 * left-out kind of mh_bank_render_coupled.
 * Dead: kt = 0, mu = 0, or zero tangents leave f_n, `out` and every state equal to those of the same junction without the flag: C_S, C_P
 * and C_M are then the bits of C_nn, and N keeps step 4's and step 4h's trees.  (f_t is 0 for kt = 0 and for mu = 0; with zero tangents it
 * is the rigid slider's force under w, and it moves nothing.)
 * Every junction without the bit keeps its bits beside a frictional one, and a call without a kept frictional junction launches exactly
 * what mh_bank_render_damped_groups launches.  Pickups on a frictional junction's objects are read as in mh_bank_render_observed.
 * k_bank_modes_coupled_friction<Real>: the three candidates one per lane, a ballot and a lane read; resources:
 * profiles/bank_friction_resources.txt.  512-frame blocks on an MI355X, J = 1 ... 64: fp32 1 750 - 2 340 cycles per frame (linear - Hertz), 0.56 - 0.75 ms;
 * fp64 2 220 - 2 750 cycles, 0.69 - 0.80 ms (profiles/bank_friction.json).
 * Not in this version: friction inside groups, with damping or on a bilateral junction, a transverse second axis, Dahl micro-slip,
 * roughness. */
typedef struct {
    uint32_t object;
    uint32_t points[3];
    float weights[3];
    float nx, ny, nz;
    float scale; /* the caller's coupling already multiplied by the object's DeflectionScale */
} mh_junction_side;
typedef struct {
    mh_junction_side a, b;
    float stiffness; /* K: N/m for the linear law, N/m^1.5 with MH_JUNCTION_HERTZ */
    uint32_t flags;
} mh_junction;
#define MH_NO_OBJECT 0xffffffffu
#define MH_JUNCTION_BILATERAL 1u
#define MH_JUNCTION_HERTZ 2u
#define MH_JUNCTION_SHARED 4u
#define MH_JUNCTION_DAMPED 8u
#define MH_JUNCTION_FRICTION 16u
#define MH_JUNCTION_MODES 1024
#define MH_JUNCTION_GROUP 4 /* the most junctions one group may hold */
enum { MH_JUNCTION_LEFT_OUT = 0, MH_JUNCTION_SOLVED = 1, MH_JUNCTION_REFUSED = 2 };
/* sizeof(mh_junction) as this library was built */
uint32_t mh_junction_struct_size(void);
/* What a junction with MH_JUNCTION_FRICTION carries beside its record ("Friction" above), by the junction's index in the call. */
typedef struct {
    float ta[3], tb[3]; /* the tangent of side a and of side b */
    float mu; /* the Coulomb coefficient */
    float stiffness; /* kt: the stick spring of the contact patch, N/m */
} mh_friction;
/* sizeof(mh_friction) as this library was built */
uint32_t mh_friction_struct_size(void);
/* mh_bank_render_read with junctions.  Every object that is not on a solved or refused junction's side goes through the kernels it would
 * have gone through without junctions; `out`, the per-object results and the impacts come back as from mh_bank_render_read.  With
 * n_junctions = 0 this is mh_bank_render_read. */
int mh_bank_render_coupled(mh_bank *, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts,
                           uint32_t n_renderers, const uint32_t *deal_offset, const uint32_t *deal_objects, const uint32_t *render_count,
                           const uint32_t *tuned_count, const float *out_gain, const float *listener_gain, void *out, double *object_energy,
                           uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                           const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out,
                           uint8_t *pickup_read, uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out,
                           double *compliance_out, uint8_t *status_out);
/* mh_bank_render_coupled with contact damping: `damping` ([n_junctions] float, l in 1/m per frame, read only for junctions with
 * MH_JUNCTION_DAMPED) and `carry` ([n_junctions] in the bank's precision, in and out) as described under "Contact damping".  With no
 * flagged junction this is mh_bank_render_coupled, plus NaN carries. */
int mh_bank_render_damped(mh_bank *, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts,
                          uint32_t n_renderers, const uint32_t *deal_offset, const uint32_t *deal_objects, const uint32_t *render_count,
                          const uint32_t *tuned_count, const float *out_gain, const float *listener_gain, void *out, double *object_energy,
                          uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                          const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out,
                          uint8_t *pickup_read, uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out,
                          double *compliance_out, uint8_t *status_out, const float *damping, void *carry);
/* mh_bank_render_damped that also reads the pickups on objects of kept junctions: "Pickups on junction objects" above. */
int mh_bank_render_observed(mh_bank *, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts,
                            uint32_t n_renderers, const uint32_t *deal_offset, const uint32_t *deal_objects, const uint32_t *render_count,
                            const uint32_t *tuned_count, const float *out_gain, const float *listener_gain, void *out, double *object_energy,
                            uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                            const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out,
                            uint8_t *pickup_read, uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out,
                            double *compliance_out, uint8_t *status_out, const float *damping, void *carry);
/* mh_bank_render_observed in which a Hertz junction may join a group: "Hertz junctions in groups" above.  unconverged_out: [n_junctions]. */
int mh_bank_render_mixed(mh_bank *, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts,
                         uint32_t n_renderers, const uint32_t *deal_offset, const uint32_t *deal_objects, const uint32_t *render_count,
                         const uint32_t *tuned_count, const float *out_gain, const float *listener_gain, void *out, double *object_energy,
                         uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                         const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out,
                         uint8_t *pickup_read, uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out,
                         double *compliance_out, uint8_t *status_out, const float *damping, void *carry, uint32_t *unconverged_out);
/* mh_bank_render_mixed in which a damped junction may join a group as well: "Damped junctions in groups" above. */
int mh_bank_render_damped_groups(mh_bank *, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts,
                                 uint32_t n_renderers, const uint32_t *deal_offset, const uint32_t *deal_objects, const uint32_t *render_count,
                                 const uint32_t *tuned_count, const float *out_gain, const float *listener_gain, void *out, double *object_energy,
                                 uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                                 const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out,
                                 uint8_t *pickup_read, uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out,
                                 double *compliance_out, uint8_t *status_out, const float *damping, void *carry, uint32_t *unconverged_out);
/* mh_bank_render_damped_groups with Coulomb friction on lone junctions: "Friction" above.  friction: [n_junctions] records and travel:
 * [n_junctions][frames], both read for flagged junctions only; tangent_out: [n_junctions][frames] and anchor: [n_junctions], in the bank's
 * precision; friction_counts_out: [n_junctions][3].  With no flagged junction this is mh_bank_render_damped_groups, launch for launch. */
int mh_bank_render_friction(mh_bank *, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts,
                            uint32_t n_renderers, const uint32_t *deal_offset, const uint32_t *deal_objects, const uint32_t *render_count,
                            const uint32_t *tuned_count, const float *out_gain, const float *listener_gain, void *out, double *object_energy,
                            uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                            const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out,
                            uint8_t *pickup_read, uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out,
                            double *compliance_out, uint8_t *status_out, const float *damping, void *carry, uint32_t *unconverged_out,
                            const mh_friction *friction, const float *travel, void *tangent_out, void *anchor, uint32_t *friction_counts_out);
/* Read back state columns (for parity tests and the modal-energy diagnostic, ModalAudio.cpp:564-577). */
int mh_bank_read_state(const mh_bank *, uint32_t first, uint32_t count, double *state_re, double *state_im);

#ifdef __cplusplus
}
#endif
#endif
