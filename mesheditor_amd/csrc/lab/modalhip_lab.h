/* Lab bench of libmodalhip: measurement and experiment entry points OUTSIDE the path's ABI (libmodalhip_lab.so).
 * Nothing here replaces a reference interface; include/modalhip.h is the drop-in boundary. */
#pragma once
#include "../../../include/modalhip.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Average device time of `reps` back-to-back K x products over a resident n x width panel, and the algorithmic bytes of one
 * launch (76 B per node block + 4 B per row pointer + 16 B per panel entry). */
int mhl_system_bench_spmm(mh_system *, uint32_t width, uint32_t reps, double *avg_ms, double *algorithmic_bytes);
/* The matrix-free element-by-element operator: one product in the reference's DOF order, and its timing loop. */
int mhl_system_elementwise_matvec(mh_system *, const double *x, double *y, uint32_t width);
int mhl_system_bench_elementwise(mh_system *, uint32_t width, uint32_t reps, double *avg_ms);
/* The fp32 smoother's fused product-and-Chebyshev step on level 2 / 1 over an n x width panel cut into `slabs` contiguous panels. */
int mhl_system_bench_cheb_step(mh_system *, int level, uint32_t width, uint32_t slabs, uint32_t reps, double *avg_ms);
/* kind 0 = Gram G = X^T Y (X n x wa, Y n x wb), kind 1 = basis update Z = [X | W] C: average device time of `reps` launches;
 * kinds 2, 3 = a check, not a timing: the eigensolver's column-mapped basis update [X[:, map] | W | P] C (wa active columns of X through the
 * identity map / a map with gaps, W and P n x wb) in its one-destination and two-destination forms on the same inputs; *avg_ms
 * receives the number of entries that are not what the one-destination form's compact panel, scattered on the host, requires (0 = all equal). */
int mhl_context_bench_dense(mh_context *, int kind, uint64_t n, uint32_t wa, uint32_t wb, uint32_t reps, double *avg_ms);
/* The Rayleigh-Ritz step's Householder tridiagonalisation called directly: a (m x m, symmetric, both triangles, m <= 256) ->
 * d[m], e[m - 1]; variant 0 = one workgroup, 1 = several workgroups exchanging tagged values. */
int mhl_context_tridiagonalize(mh_context *, int variant, uint32_t m, const double *a, double *d, double *e, uint32_t reps, double *avg_ms);
/* the same with the reflectors (m x m, LAPACK's lower storage) and tau returned; variant 2 = the wide kernel, orders up to 768 */
int mhl_context_tridiagonalize_full(mh_context *, int variant, uint32_t m, const double *a, double *d, double *e, double *reflectors, double *tau, uint32_t reps, double *avg_ms);
/* The k lowest eigenpairs of a symmetric tridiagonal matrix (d[m], e[m - 1]) by the Rayleigh-Ritz step's partial-spectrum kernels (m <= 256:
 * one workgroup; 257 .. 768: the wide form): w[k], z (m x k, column-major), the kernels' own quality (NaN: a factorisation failed), taken = 0
 * when the call declined. */
int mhl_context_tridiag_lowest(mh_context *, uint32_t m, uint32_t k, const double *d, const double *e, double *w, double *z, double *quality, int *taken);
/* One Rayleigh-Ritz step (the solver's rr_solve) on host matrices, lower triangles, column-major: evals[ncols], vectors (m x ncols),
 * host_evals (nwant), trace[6] = reduction, defect, standard solver, partial quality, self-check word, host eigenvalue count */
int mhl_context_rr_solve(mh_context *, uint32_t m, const double *a, const double *mmat, uint32_t nwant, int gm_is_identity, double *evals, double *vectors, uint32_t *ncols,
                         double *host_evals, double *trace);
/* C (M x N, ldc) = alpha op(A) op(B) + beta C through the Rayleigh-Ritz step's small-product kernel; column-major host arrays, c in and out */
int mhl_context_potrf_inverse(mh_context *, uint32_t w, const double *a, const double *dscale, double *l, double *linv, int *info2);
int mhl_context_spd_inverse(mh_context *, uint32_t w, const double *a, double *out, uint32_t reps, double *avg_ms);
int mhl_context_small_gemm(mh_context *, int ta, int tb, uint32_t M, uint32_t N, uint32_t K, double alpha, const double *a, uint32_t lda, const double *b, uint32_t ldb, double beta, double *c,
                           uint32_t ldc, uint32_t reps, double *avg_ms);
/* G (wa x wb, column-major) = X^T Y for row-major host panels (n x wa), (n x wb): the solver's Gram kernel */
int mhl_context_gram(mh_context *, uint64_t n, const double *x, uint32_t wa, const double *y, uint32_t wb, double *g);
/* One form of the BSR 3x3 product (mh_spmm.hip) on the caller's own matrix, through the product's dispatchers: no node permutation, the
 * launch selection is the solver's.  Panels are row-major, 3 n_nodes rows of pitch w.  Every output is a host array of
 * MHL_SPMM_GUARD + entries + MHL_SPMM_GUARD values: the device buffer is pre-filled with the sentinel (a quiet NaN with a payload) and
 * copied back whole, so entries that were never written and entries that should not have been touched both show.  A form the
 * dispatcher refuses on the host (MH_EINVAL) leaves the outputs as the caller passed them. */
enum {
    MHL_SPMM_F64_A = 0,      /* y = A x                                  vals9, x double */
    MHL_SPMM_F64_M = 1,      /* y2 = M x                                 mscal, x double */
    MHL_SPMM_F64_AM = 2,     /* y = A x, y2 = M x in one launch */
    MHL_SPMM_F32_A = 3,      /* y = A x                                  vals9, x, y float */
    MHL_SPMM_MIXED = 4,      /* y (double) = A x                         vals9 double, x float */
    MHL_SPMM_MAPPED = 5,     /* columns omap[c], c < wreal, of y, y2 (3 n_nodes x ldy) */
    MHL_SPMM_MAPPED_RES = 6, /* the same with the residual epilogue: r_out (3 n_nodes x w), partial (n_nodes x 2 x w) */
    MHL_SPMM_F32_CHEB = 7    /* the fused Chebyshev step: x is d (float); cheb_r, cheb_x start as r, xs; cheb_d_in is d after the launch */
};
/* the guard and sentinel conventions of every "form" entry of this header (the sparse product's below, the dense products' further down) */
#define MHL_GUARD 64u
#define MHL_SENTINEL64 0x7ff8a5a5a5a5a5a5ull
#define MHL_SENTINEL32 0x7fd5a5a5u
#define MHL_SPMM_GUARD MHL_GUARD
#define MHL_SPMM_SENTINEL64 MHL_SENTINEL64
#define MHL_SPMM_SENTINEL32 MHL_SENTINEL32
typedef struct mhl_spmm_request {
    int32_t form;
    uint32_t misalign; /* plain fp64 forms: the x panel starts 8 bytes into its allocation (no 16-byte loads: k_spmm serves even widths too) */
    uint32_t n_nodes, w;
    uint32_t ldy, wreal; /* mapped forms */
    float c1, c2;        /* Chebyshev step */
    const uint32_t *row_ptr, *col, *omap;
    const void *vals9;   /* 9 per node block, row-major: double, or float for MHL_SPMM_F32_A and MHL_SPMM_F32_CHEB */
    const double *mscal; /* 1 per node block */
    const void *x;
    const double *theta, *dinv;   /* residual epilogue: w values; 3 n_nodes weights or null */
    const float *dinv32, *r, *xs; /* Chebyshev step: 3 n_nodes; panels */
    void *y, *y2;
    double *r_out, *partial;
    float *cheb_r, *cheb_d_out, *cheb_x, *cheb_d_in;
    int32_t taken; /* out: 0 when mh_spmm_f32_cheb_step declined the panel */
} mhl_spmm_request;
int mhl_context_spmm_form(mh_context *, mhl_spmm_request *);
/* One form of the dense tall products (mh_dense.hip) on the caller's arrays, through the solver's own dispatchers: mh_combine, mh_short_product,
 * mh_gram, and the two coefficient packers.  Panels are row-major.  Every output, and X (an output when the call runs in place, bit-unchanged
 * otherwise), is a host array of MHL_GUARD + entries + MHL_GUARD values: the device buffer is pre-filled with the sentinel -- its body with the
 * caller's values where the form reads them: X always, out1 / out2 under `accumulate` -- and copied back whole.  A request this entry itself
 * rejects leaves `dispatched` 0; one the dispatcher refuses on the host (MH_EINVAL) leaves it 1, and the host arrays as the caller passed them. */
enum {
    MHL_DENSE_COMBINE = 0,       /* mh_combine with exactly the request's arguments */
    MHL_DENSE_SHORT_PRODUCT = 1, /* mh_short_product: out1 (n x nc) = x (n x wx) ct, in `slices` K slices through `partial` (slices x n x nc) */
    MHL_DENSE_GRAM = 2,          /* mh_gram: the wx x ww block at (g_row0, g_col0) of g (ld x g_cols, column-major) = x^T y, y = w (n x ldy, columns through ymap) */
    MHL_DENSE_PACK = 3           /* the packer of `coeff_layout` alone: ct_out */
};
enum {
    MHL_COEFF_KMAJOR = 0,   /* ct: (wx + ww + wp) x nc, row-major, as the kernel reads it */
    MHL_COEFF_BLOCKS = 1,   /* mh_pack_coefficients: c1 (m x pack_a), c2 (m x pack_b), column-major at pack_ld, side by side; m = wx + ww + wp, nc = pack_a + pack_b */
    MHL_COEFF_STACKED = 2   /* mh_pack_stacked: c1 (pack_a x nc), c2 (pack_b x nc), column-major, one above the other, times pack_scale; pack_a + pack_b = wx + ww + wp */
};
typedef struct mhl_dense_request {
    int32_t form;
    int32_t in_place; /* 0: separate outputs; 1: out1 is the device copy of X (the Cholesky-QR call); 2: out1_also is the device copy of X (the basis update's call) */
    int32_t accumulate, coeff_layout;
    uint64_t n;
    uint32_t wx, ldx, ww, wp; /* ldx 0: wx */
    uint32_t nc, n1, ld1, ld1_also;
    uint32_t col_begin, col_count, slices;
    uint32_t pack_a, pack_b, pack_ld;
    uint32_t ldy, ld, g_cols, g_row0, g_col0; /* Gram; ldy 0: ww */
    uint32_t pad_;
    double pack_scale;
    const uint32_t *xmap, *omap, *omap_also, *ymap;
    const double *x, *w, *p; /* host panels: n x (ldx or wx), n x ww (Gram: n x ldy), n x wp; a null panel goes to the dispatcher as null */
    const double *ct, *c1, *c2;
    double *x_out;                    /* guarded n x (ldx or wx) */
    double *out1, *out2, *out1_also;  /* guarded n x (ld1 or n1), n x (nc - n1), n x ld1_also; out1 null with in_place 1, out1_also null with in_place 2 */
    double *partial, *ct_out, *g;     /* guarded slices x n x nc (slices > 1), m x nc (packed layouts), ld x g_cols */
    int32_t cu_count;                 /* out: the context's compute units (k_combine's grid is capped at 8 workgroups each) */
    int32_t dispatched;               /* out */
} mhl_dense_request;
int mhl_context_dense_form(mh_context *, mhl_dense_request *);
/* measured HBM ceilings of the device: a streaming copy (read + written bytes per second) and a streaming read, in GB/s */
int mhl_context_bench_stream(mh_context *, uint64_t bytes, uint32_t reps, double *copy_gbs, double *read_gbs);
/* the context's device pool: bytes held from the device, bytes of them idle in the cache, the cap on the idle part */
int mhl_context_pool_stats(mh_context *, uint64_t *reserved, uint64_t *idle, uint64_t *cap);
/* y = B x, the eigensolver's preconditioner cycle at the shift sigma, single- (precision 0) or double-precision (1) smoothers; x, y column-major
 * n x width (width <= 1 024), the reference's DOF order */
int mhl_system_precondition(mh_system *, double sigma, int precision, const double *x, double *y, uint32_t width);
/* The preconditioner's hierarchy: built at sigma (anew when rebuild != 0) with its sizes[20]; then the standing hierarchy's coarse level, P1
 * operator and cycle shape, and each smoothed level's sliver patches and clusters, in the reference's numbering (lab/mh_lab.hip lists the fields) */
int mhl_system_hierarchy_sizes(mh_system *, double sigma, int rebuild, uint64_t *sizes);
int mhl_system_hierarchy_export(mh_system *, uint32_t width, double *scalars, uint32_t *agg_of, double *agg_t, uint32_t *l1_row, uint32_t *l1_col, double *l1_val, double *a0);
int mhl_system_patch_export(mh_system *, int level, uint32_t *nodes, double *weight, double *inv64, uint32_t *cluster_row, uint32_t *cluster_ptr, double *cinv64);
/* The rigid-body level's graph aggregation (host code): CSR node graph in (diagonal entries included), aggregate per node out. */
uint32_t mhl_graph_aggregates(const uint32_t *row_ptr, const uint32_t *col, uint32_t n, uint32_t target, uint32_t max_order, uint32_t *agg_of);
/* Soak of the multi-workgroup tridiagonalisation's tagged exchange with its transport as a parameter (lab/mh_soak.hip): `launches` runs of
 * one fixed matrix, every collected value compared with a recorded undisturbed run; out receives the deviation records. */
int mhl_sytrd_soak(mh_context *, uint32_t transport, uint32_t m, uint32_t launches, volatile int *recorded, volatile int *go, void *out, uint64_t out_bytes);
uint64_t mhl_sytrd_soak_bytes(void);
/* one kind of a wide solve's work, alone, over and over on the context's stream until *stop (lab/mh_soak.hip lists the kinds) */
int mhl_soak_aggressor(mh_context *, int kind, volatile int *stop, uint64_t *count);
#ifdef __cplusplus
}
#endif
