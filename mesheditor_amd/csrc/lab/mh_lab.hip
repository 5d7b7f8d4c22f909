// libmodalhip_lab.so: measurement and experiment entry points that are NOT part of the path's ABI (include/modalhip.h has
// none of them): timing loops around the product's own kernels, the tridiagonalisation variants called directly, and the
// matrix-free element-by-element operator (lab/mh_elem.hip: built, measured 2.1-2.6x slower than the BSR product, kept here for
// the record).  Links libmodalhip.so and reaches its internals through mh_common.h; tests, tools/ and bench.py's secondary
// figures load it explicitly (tools/lab.py), the product never does.
#include "../mh_common.h"
#include "modalhip_lab.h"

#include <algorithm>
#include <optional>

void mh_elementwise_apply(mh_context *ctx, const mh_system *sys, double sigma, const double *x, double *y, uint32_t w); // lab/mh_elem.hip

namespace {
constexpr int TB = 256;
// reference DOF order (column-major n x width) <-> internal row-major panel
__global__ void k_lab_ref_to_panel(const double *__restrict__ x, const uint32_t *__restrict__ perm, uint32_t nnodes, uint32_t width, double *__restrict__ panel) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= size_t(nnodes) * 3 * width) return;
    const uint32_t c = uint32_t(i % width), comp = uint32_t((i / width) % 3), node = uint32_t(i / (size_t(3) * width));
    panel[i] = x[size_t(c) * (size_t(3) * nnodes) + size_t(3) * perm[node] + comp];
}
__global__ void k_lab_panel_to_ref(const double *__restrict__ panel, const uint32_t *__restrict__ perm, uint32_t nnodes, uint32_t width, double *__restrict__ y) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= size_t(nnodes) * 3 * width) return;
    const uint32_t c = uint32_t(i % width), comp = uint32_t((i / width) % 3), node = uint32_t(i / (size_t(3) * width));
    y[size_t(c) * (size_t(3) * nnodes) + size_t(3) * perm[node] + comp] = panel[i];
}
} // namespace

namespace {
typedef float f4_stream __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) k_stream_copy(const f4_stream *__restrict__ src, f4_stream *__restrict__ dst, size_t count) {
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < count; i += size_t(gridDim.x) * 256) dst[i] = src[i];
}
// U independent 16-byte loads in flight per lane before the first store (the one-load-per-iteration form above leaves the memory
// system with too few bytes in flight: 4.5 TB/s against the 6.3 the device reaches); NT: non-temporal loads and stores
template<int U, bool NT, int T = 256, bool NTL = NT> __global__ void __launch_bounds__(T) k_stream_copy_u(const f4_stream *__restrict__ src, f4_stream *__restrict__ dst, size_t count) {
    const size_t stride = size_t(gridDim.x) * T;
    for (size_t base = size_t(blockIdx.x) * T + threadIdx.x; base < count; base += stride * U) {
        f4_stream v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = base + size_t(u) * stride;
            if (i < count) v[u] = NTL ? __builtin_nontemporal_load(src + i) : src[i];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = base + size_t(u) * stride;
            if (i < count) {
                if (NT) __builtin_nontemporal_store(v[u], dst + i);
                else dst[i] = v[u];
            }
        }
    }
}
template<int U, bool NT> __global__ void __launch_bounds__(256) k_stream_read_u(const f4_stream *__restrict__ src, size_t count, float *__restrict__ out) {
    const size_t stride = size_t(gridDim.x) * 256;
    f4_stream acc = {0, 0, 0, 0};
    for (size_t base = size_t(blockIdx.x) * 256 + threadIdx.x; base < count; base += stride * U) {
        f4_stream v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = base + size_t(u) * stride;
            v[u] = i < count ? (NT ? __builtin_nontemporal_load(src + i) : src[i]) : f4_stream{0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc += v[u];
    }
    float s = acc[0] + acc[1] + acc[2] + acc[3];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out + blockIdx.x, s);
}
__global__ void __launch_bounds__(256) k_stream_read(const f4_stream *__restrict__ src, size_t count, float *__restrict__ out) {
    f4_stream acc = {0, 0, 0, 0};
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < count; i += size_t(gridDim.x) * 256) acc += src[i];
    float s = acc[0] + acc[1] + acc[2] + acc[3];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out + blockIdx.x, s); // (a workgroup's four waves: the value is never read)
}
} // namespace

namespace {
// reference node id of every P1 (internal) point: perm[p1_corner[p]], checked to be a permutation of the mesh points
std::vector<uint32_t> lab_point_ref(const mh_system *s) {
    const std::vector<uint32_t> perm = s->perm.to_host(), corner = s->p1_corner.to_host();
    std::vector<uint32_t> ref(s->n_points);
    std::vector<uint8_t> seen(s->n_points, 0);
    for (uint32_t p = 0; p < s->n_points; ++p) {
        ref[p] = perm[corner[p]];
        if (ref[p] >= s->n_points || seen[ref[p]]) mh_throw(MH_EINVAL, "hierarchy export: P1 point %u has reference id %u", p, ref[p]);
        seen[ref[p]] = 1;
    }
    return ref;
}
const PatchSet &lab_patches(const mh_system *s, int level) { return level == 2 ? s->patches2 : s->patches1; }
} // namespace

extern "C" {
// The rigid-body level's graph aggregation (host code, no device): CSR graph of a level's node blocks in, aggregate of every node
// out; returns the aggregate count.
uint32_t mhl_graph_aggregates(const uint32_t *row_ptr, const uint32_t *col, uint32_t n, uint32_t target, uint32_t max_order, uint32_t *agg_of) {
    std::vector<uint32_t> rp(row_ptr, row_ptr + n + 1), cl(col, col + row_ptr[n]), out;
    const uint32_t na = mh_graph_aggregates(rp, cl, n, target, max_order, out);
    std::copy(out.begin(), out.end(), agg_of);
    return na;
}

// y = (K - sigma M) x at the reference's shift, element by element without the assembled matrix (atomic scatter: equal to
// mh_system_matvec(which = 2) up to rounding, not bit-reproducible).  x, y: column-major n x width, the reference's DOF order.
int mhl_system_elementwise_matvec(mh_system *s, const double *x, double *y, uint32_t width) {
    if (!s || !x || !y || width == 0) return MH_EINVAL;
    mh_context *ctx = s->ctx;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t n = size_t(3) * s->n_nodes;
        DevArray<double> xr(ctx, n * width), xp(ctx, n * width), yp(ctx, n * width);
        xr.upload(x, n * width);
        k_lab_ref_to_panel<<<div_up(n * width, TB), TB, 0, ctx->stream>>>(xr, s->perm, s->n_nodes, width, xp);
        KERNEL_CHECK();
        mh_elementwise_apply(ctx, s, -15791.367041742974, xp, yp, width);
        k_lab_panel_to_ref<<<div_up(n * width, TB), TB, 0, ctx->stream>>>(yp, s->perm, s->n_nodes, width, xr.get());
        KERNEL_CHECK();
        xr.download(y, n * width);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

int mhl_system_bench_spmm(mh_system *s, uint32_t width, uint32_t reps, double *avg_ms, double *algorithmic_bytes) {
    if (!s || width == 0 || reps == 0 || !avg_ms) return MH_EINVAL;
    mh_context *ctx = s->ctx;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t n = size_t(3) * s->n_nodes;
        DevArray<double> x(ctx, n * width), y(ctx, n * width);
        std::vector<double> hx(n * width);
        for (size_t i = 0; i < hx.size(); ++i) hx[i] = double((i * 2654435761u) % 1000) * 1e-3 - 0.5;
        x.upload(hx.data(), hx.size());
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (int warm = 0; warm < 2; ++warm) mh_spmm(ctx, s->L2, s->L2.kval, x, y, nullptr, nullptr, width);
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipEventRecord(e0, ctx->stream));
        for (uint32_t r = 0; r < reps; ++r) mh_spmm(ctx, s->L2, s->L2.kval, x, y, nullptr, nullptr, width);
        HIP_CHECK(hipEventRecord(e1, ctx->stream));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        *avg_ms = ms / reps;
        if (algorithmic_bytes) *algorithmic_bytes = 76.0 * double(s->L2.n_blocks) + 4.0 * (double(s->n_nodes) + 1) + 16.0 * double(n) * width;
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

// The single-precision smoother's fused product-and-Chebyshev step (mh_spmm_f32_cheb_step) on level 2 (P2) or 1 (P1) over an n x width
// panel, `slabs` launches of width / slabs columns each on separate contiguous panels: does a wide block cost more per column than
// narrow ones?  (Needs mh_build_hierarchy: the fp32 copies of the operators; a solve of the system leaves them behind.)
int mhl_system_bench_cheb_step(mh_system *s, int level, uint32_t width, uint32_t slabs, uint32_t reps, double *avg_ms) {
    if (!s || !avg_ms || width == 0 || slabs == 0 || width % (4 * slabs) || reps == 0 || (level != 1 && level != 2)) return MH_EINVAL;
    mh_context *ctx = s->ctx;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        const BsrLevel &lvl = level == 2 ? s->L2 : s->L1;
        if (!lvl.aval32.get() || !lvl.dinv32.get()) mh_throw(MH_EINVAL, "bench_cheb_step: no single-precision operator (solve the system once first)");
        const size_t n = size_t(3) * lvl.n_nodes;
        const uint32_t wc = width / slabs;
        std::vector<DevArray<float>> d(slabs), d2(slabs), r(slabs), x(slabs);
        std::vector<float> h(n * wc);
        for (size_t i = 0; i < h.size(); ++i) h[i] = float((i * 2654435761u) % 1000) * 1e-3f - 0.5f;
        for (uint32_t q = 0; q < slabs; ++q) {
            for (auto *a : {&d[q], &d2[q], &r[q], &x[q]}) {
                a->reset(ctx, n * wc);
                a->upload(h.data(), h.size());
            }
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        auto run = [&] {
            for (uint32_t q = 0; q < slabs; ++q)
                if (!mh_spmm_f32_cheb_step(ctx, lvl, d[q], d2[q], r[q], x[q], lvl.dinv32, 0.3f, 0.1f, wc)) mh_throw(MH_EINVAL, "bench_cheb_step: width %u not served by the wide kernel", wc);
        };
        run();
        run();
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipEventRecord(e0, ctx->stream));
        for (uint32_t rep = 0; rep < reps; ++rep) run();
        HIP_CHECK(hipEventRecord(e1, ctx->stream));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        *avg_ms = ms / reps;
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

int mhl_system_bench_elementwise(mh_system *s, uint32_t width, uint32_t reps, double *avg_ms) {
    if (!s || width == 0 || reps == 0 || !avg_ms) return MH_EINVAL;
    mh_context *ctx = s->ctx;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t n = size_t(3) * s->n_nodes;
        DevArray<double> x(ctx, n * width), y(ctx, n * width);
        std::vector<double> hx(n * width);
        for (size_t i = 0; i < hx.size(); ++i) hx[i] = double((i * 2654435761u) % 1000) * 1e-3 - 0.5;
        x.upload(hx.data(), hx.size());
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (int warm = 0; warm < 2; ++warm) mh_elementwise_apply(ctx, s, -15791.367041742974, x, y, width);
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipEventRecord(e0, ctx->stream));
        for (uint32_t r = 0; r < reps; ++r) mh_elementwise_apply(ctx, s, -15791.367041742974, x, y, width);
        HIP_CHECK(hipEventRecord(e1, ctx->stream));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        *avg_ms = ms / reps;
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

} // extern "C"

namespace {
// Kinds 2 and 3 of mhl_context_bench_dense: the eigensolver's basis update with column maps, as update_basis calls it, in its two
// forms on the same inputs -- [X[:, map] | W | P] Ct with X n x b, wa active columns (map[k] = k, or k + k / 2: gaps), W and P n x wb,
// wa + wb output columns of which the first wa are the new Ritz vectors.  Form 0 stores them to the compact panel alone (pitch = wa
// rounded up to even), form 1 to the compact panel and to the mapped columns of X.  Returns the number of entries in which a result is
// not what form 0's compact panel, scattered here on the host, says it must be: X after form 1 (columns outside the map unchanged),
// the compact panel of form 1, its other wb output columns, X after form 0 (only read) -- and in which form 0 itself misses the
// product formed on the host by more than the rounding of a sum of m products.  With more rows than 64 x the workgroups the device
// holds, workgroups take several row tiles each: the persistent loop the in-place argument of k_combine is about.
double lab_mapped_update_mismatches(mh_context *ctx, bool gaps, size_t n, uint32_t wa, uint32_t wb) {
    const uint32_t b = (wa + wa / 2 + 3u) & ~1u, pitch = (wa + 1u) & ~1u, m = wa + 2 * wb, nc = wa + wb;
    std::vector<uint32_t> map(wa);
    for (uint32_t k = 0; k < wa; ++k) map[k] = gaps ? k + k / 2 : k;
    auto fill = [](std::vector<double> &v, size_t salt) {
        for (size_t i = 0; i < v.size(); ++i) v[i] = double(((i + salt) * 2654435761u) % 1000) * 1e-3 - 0.5;
    };
    std::vector<double> hx(n * b), hw(n * wb), hp(n * wb), hc(size_t(m) * nc);
    fill(hx, 0), fill(hw, 7919), fill(hp, 104729), fill(hc, 1299709);
    struct Out { std::vector<double> xn, x, p; };
    auto run = [&](int form) {
        DevArray<double> dx(ctx, n * b), dw(ctx, n * wb), dp(ctx, n * wb), dc(ctx, size_t(m) * nc), dxn(ctx, n * pitch), dpo(ctx, n * wb);
        DevArray<uint32_t> dmap(ctx, wa);
        dx.upload(hx.data(), hx.size());
        dw.upload(hw.data(), hw.size());
        dp.upload(hp.data(), hp.size());
        dc.upload(hc.data(), hc.size());
        dmap.upload(map.data(), wa);
        dxn.zero();
        MhCombine update{.x = dx, .wx = wa, .ldx = b, .xmap = dmap, .w = dw, .ww = wb, .p = dp, .wp = wb, .ct = dc, .nc = nc, .out1 = dxn, .n1 = wa, .ld1 = pitch, .out2 = dpo};
        if (form == 1) update.out1_also = dx, update.ld1_also = b, update.omap_also = dmap;
        mh_combine(ctx, n, update);
        Out o{std::vector<double>(n * pitch), std::vector<double>(n * b), std::vector<double>(n * wb)};
        dxn.download(o.xn.data(), o.xn.size());
        dx.download(o.x.data(), o.x.size());
        dpo.download(o.p.data(), o.p.size());
        return o;
    };
    const Out one = run(0), two = run(1);
    auto differing = [](const std::vector<double> &a, const std::vector<double> &c) {
        size_t d = 0;
        for (size_t i = 0; i < a.size(); ++i) d += !(a[i] == c[i]);
        return d;
    };
    size_t bad = differing(one.x, hx);
    for (size_t r = 0; r < n; ++r) // form 0 against the product on the host
        for (uint32_t c = 0; c < nc; ++c) {
            double ref = 0, mag = 0;
            for (uint32_t k = 0; k < m; ++k) {
                const double s = k < wa ? hx[r * b + map[k]] : k < wa + wb ? hw[r * wb + (k - wa)] : hp[r * wb + (k - wa - wb)];
                ref += s * hc[size_t(k) * nc + c];
                mag += std::abs(s * hc[size_t(k) * nc + c]);
            }
            const double got = c < wa ? one.xn[r * pitch + c] : one.p[r * wb + (c - wa)];
            bad += !(std::abs(got - ref) <= 2.0 * m * 2.3e-16 * mag);
        }
    std::vector<double> want = hx; // form 0's compact panel scattered on the host
    size_t written = 0;
    for (size_t r = 0; r < n; ++r)
        for (uint32_t k = 0; k < wa; ++k) {
            want[r * b + map[k]] = one.xn[r * pitch + k];
            written += want[r * b + map[k]] != hx[r * b + map[k]];
        }
    if (written < n * wa / 2) mh_throw(MH_EHIP, "mapped update check: the update left %zu of %zu entries as they were", n * wa - written, n * size_t(wa));
    bad += differing(two.xn, one.xn) + differing(two.x, want) + differing(two.p, one.p);
    return double(bad);
}
} // namespace

extern "C" {
int mhl_context_bench_dense(mh_context *ctx, int kind, uint64_t n, uint32_t wa, uint32_t wb, uint32_t reps, double *avg_ms) {
    if (!ctx || !avg_ms || n == 0 || wa == 0 || wb == 0 || reps == 0 || kind < 0 || kind > 3) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        std::lock_guard<std::mutex> lock(mh_solve_mutex());
        if (kind >= 2) { // (a check, not a timing: the count of wrong entries leaves in *avg_ms)
            *avg_ms = lab_mapped_update_mismatches(ctx, kind == 3, n, wa, wb);
            return MH_OK;
        }
        DevArray<double> x(ctx, n * wa), y(ctx, n * wb), g(ctx, size_t(wa + wb) * (wa + wb)), z(ctx, n * wa);
        std::vector<double> h(n * std::max(wa, wb));
        for (size_t i = 0; i < h.size(); ++i) h[i] = double((i * 2654435761u) % 1000) * 1e-3 - 0.5;
        x.upload(h.data(), n * wa);
        y.upload(h.data(), n * wb);
        g.upload(h.data(), g.count);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        auto run = [&]() {
            if (kind == 0) mh_gram(ctx, n, x, wa, y, wb, g, wa);
            else mh_combine(ctx, n, {.x = x, .wx = wa, .w = y, .ww = wb, .ct = g, .nc = wa, .out1 = z, .n1 = wa});
        };
        run();
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipEventRecord(e0, ctx->stream));
        for (uint32_t r = 0; r < reps; ++r) run();
        HIP_CHECK(hipEventRecord(e1, ctx->stream));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        *avg_ms = ms / reps;
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

int mhl_context_tridiagonalize_full(mh_context *ctx, int variant, uint32_t m, const double *a, double *d, double *e, double *reflectors, double *tau, uint32_t reps, double *avg_ms);
int mhl_context_tridiagonalize(mh_context *ctx, int variant, uint32_t m, const double *a, double *d, double *e, uint32_t reps, double *avg_ms) {
    return mhl_context_tridiagonalize_full(ctx, variant, m, a, d, e, nullptr, nullptr, reps, avg_ms);
}

// variant 2: the wide kernel (orders up to 768).  reflectors (m x m, LAPACK's lower storage) and tau (m) are returned when asked for.
int mhl_context_tridiagonalize_full(mh_context *ctx, int variant, uint32_t m, const double *a, double *d, double *e, double *reflectors, double *tau, uint32_t reps, double *avg_ms) {
    if (!ctx || !a || !d || !e || m < 2 || variant < 0 || variant > 3 || m > (variant == 2 ? 768u : 256u)) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        MhSharedPhase not_during_a_factorisation(ctx->device); // (no process-wide lock: calls on different contexts are meant to overlap)
        DevArray<double> da(ctx, size_t(m) * m), work(ctx, size_t(m) * m), dd(ctx, m), de(ctx, m), dtau(ctx, m);
        da.upload(a, size_t(m) * m);
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        float total = 0;
        for (uint32_t r = 0; r < std::max(1u, reps); ++r) {
            HIP_CHECK(hipMemcpyAsync(work, da, size_t(m) * m * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
            HIP_CHECK(hipEventRecord(e0, ctx->stream));
            if (variant == 2) mh_sytrd_wide(ctx, work, m, dd, de, dtau);
            else mh_sytrd_small(ctx, work, m, dd, de, dtau, variant);
            HIP_CHECK(hipEventRecord(e1, ctx->stream));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            total += ms;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        dd.download(d, m);
        de.download(e, m - 1);
        if (reflectors) work.download(reflectors, size_t(m) * m);
        if (tau) dtau.download(tau, m);
        if (mh_sytrd_gave_up(ctx)) mh_throw(MH_EHIP, "tridiagonalisation: a workgroup timed out waiting for the others' values");
        if (avg_ms) *avg_ms = total / std::max(1u, reps);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

// The k lowest eigenpairs of the symmetric tridiagonal (d[m], e[m - 1]) by the Rayleigh-Ritz step's partial-spectrum kernels:
// mh_tridiag_lowest for m <= 256, mh_tridiag_lowest_wide for 257 .. 768.  w[k], z (m x k, column-major), *quality the kernels' own
// residual measure (NaN when a factorisation failed); *taken = 0 when the call declined the problem (w, z, quality then untouched).
int mhl_context_tridiag_lowest(mh_context *ctx, uint32_t m, uint32_t k, const double *d, const double *e, double *w, double *z, double *quality, int *taken) {
    if (!ctx || !d || !e || !w || !z || !quality || !taken || m < 2 || m > 768 || k < 1) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        MhSharedPhase not_during_a_factorisation(ctx->device);
        DevArray<double> dd(ctx, m), de(ctx, m), dw(ctx, k), dz(ctx, size_t(m) * k);
        dd.upload(d, m);
        de.zero();
        de.upload(e, m - 1);
        bool ok;
        double q = std::numeric_limits<double>::quiet_NaN();
        if (m <= 256) {
            DevArray<double> ufac(ctx, size_t(3) * m * k), qv(ctx, 8), lam(ctx, k);
            ok = mh_tridiag_lowest(ctx, dd, de, m, k, dw, dz, m, ufac, qv, lam);
            if (ok) qv.download(&q, 1);
        } else {
            DevArray<double> work(ctx, size_t(5) * k * m + size_t(2) * k * k + 8);
            DevArray<int> info(ctx, 2);
            ok = mh_tridiag_lowest_wide(ctx, dd, de, m, k, dw, dz, m, work, info, &q);
        }
        *taken = ok ? 1 : 0;
        if (ok) {
            dw.download(w, k);
            dz.download(z, size_t(m) * k);
            *quality = q;
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return MH_OK;
    } catch (const std::exception &ex) { return mh_guard(ctx, ex); }
}

// One Rayleigh-Ritz step, mh_rr_solve itself, on host matrices (order m, column-major, lower triangles used; mmat may be null when
// gm_is_identity).  evals receives the *ncols eigenvalues, vectors (m x *ncols, column-major) the gM-orthonormal eigenvectors: nwant
// columns when a partial path delivered them, m otherwise.  host_evals (nwant) receives the eigenvalues the partial path read back
// itself.  trace[6]: reduction, measured defect (-1: none), standard solver (MhRrTrace's codes), partial quality (NaN: none ran),
// the self-check word (zeroed before the step, read after it), the count of host eigenvalues.  MH_EFACTOR when the step failed.
int mhl_context_rr_solve(mh_context *ctx, uint32_t m, const double *a, const double *mmat, uint32_t nwant, int gm_is_identity, double *evals, double *vectors, uint32_t *ncols,
                         double *host_evals, double *trace) {
    if (!ctx || !a || (!mmat && !gm_is_identity) || !evals || !vectors || !ncols || !trace || m < 1 || m > 1024 || nwant > m) return MH_EINVAL;
    struct TraceOn {
        mh_context *ctx;
        ~TraceOn() { ctx->rr_trace = nullptr; }
    };
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        MhSharedPhase not_during_a_factorisation(ctx->device);
        const size_t mm = size_t(m) * m;
        DevArray<double> gA(ctx, mm), gM(ctx, mm), ev(ctx, m), ework(ctx, m);
        DevArray<int> info(ctx, 2);
        info.zero();
        gA.upload(a, mm);
        if (mmat) gM.upload(mmat, mm);
        else gM.zero();
        if (ctx->rr_check) HIP_CHECK(hipMemsetAsync(ctx->rr_check, 0, sizeof(unsigned long long), ctx->stream));
        MhRrTrace tr;
        std::vector<double> hv;
        int hinfo;
        {
            ctx->rr_trace = &tr;
            TraceOn off{ctx};
            hinfo = mh_rr_solve(ctx, gA, gM, m, ev, ework, info, nwant, gm_is_identity != 0, host_evals ? &hv : nullptr);
        }
        unsigned long long check = 0;
        if (ctx->rr_check) HIP_CHECK(hipMemcpyAsync(&check, ctx->rr_check, sizeof(check), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        double checkd;
        memcpy(&checkd, &check, sizeof(checkd));
        const bool partial = tr.solver == MhRrTrace::SMALL_PARTIAL || tr.solver == MhRrTrace::WIDE_PARTIAL;
        *ncols = hinfo ? 0 : (partial ? nwant : m);
        trace[0] = tr.reduction, trace[1] = tr.defect, trace[2] = tr.solver, trace[3] = tr.quality, trace[4] = checkd, trace[5] = double(hv.size());
        if (hinfo) return MH_EFACTOR;
        ev.download(evals, *ncols);
        gA.download(vectors, size_t(m) * *ncols);
        if (host_evals && !hv.empty()) std::copy(hv.begin(), hv.end(), host_evals);
        return MH_OK;
    } catch (const std::exception &ex) { return mh_guard(ctx, ex); }
}

// y = B x: the eigensolver's preconditioner cycle at the shift sigma with single- (precision 0) or double-precision (1) smoothers, through
// mh_precondition_panel (the eigensolver's own slab loop above 256 columns).  x, y: column-major n x width (width <= 1 024), the reference's DOF order.
int mhl_system_precondition(mh_system *s, double sigma, int precision, const double *x, double *y, uint32_t width) {
    if (!s || !x || !y || width == 0 || width > 1024 || (precision != 0 && precision != 1)) return MH_EINVAL;
    mh_context *ctx = s->ctx;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t n = size_t(3) * s->n_nodes;
        DevArray<double> xr(ctx, n * width), xp(ctx, n * width), yp(ctx, n * width);
        xr.upload(x, n * width);
        k_lab_ref_to_panel<<<div_up(n * width, TB), TB, 0, ctx->stream>>>(xr, s->perm, s->n_nodes, width, xp);
        KERNEL_CHECK();
        mh_precondition_panel(s, sigma, precision, xp, yp, width);
        k_lab_panel_to_ref<<<div_up(n * width, TB), TB, 0, ctx->stream>>>(yp, s->perm, s->n_nodes, width, xr.get());
        KERNEL_CHECK();
        xr.download(y, n * width);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

// The preconditioner's hierarchy built at sigma (rebuild != 0: built anew even when one at sigma stands) and finished, and its sizes:
// sizes[0..3] = n_points, n_agg, n0 = 6 n_agg, node blocks of the P1 operator; then per level (P2 at 4, P1 at 12): patches, nodes per
// patch, clusters, cluster rows, cluster inverse values, bad elements, nodes of the largest cluster, patches and clusters dropped.
int mhl_system_hierarchy_sizes(mh_system *s, double sigma, int rebuild, uint64_t *sizes) {
    if (!s || !sizes) return MH_EINVAL;
    mh_context *ctx = s->ctx;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        std::lock_guard<std::mutex> lock(mh_solve_mutex());
        if (rebuild) s->hierarchy_ready = false;
        mh_build_hierarchy(s, sigma);
        sizes[0] = s->n_points, sizes[1] = s->n_agg, sizes[2] = uint64_t(6) * s->n_agg, sizes[3] = s->L1.n_blocks;
        for (int level : {2, 1}) {
            const PatchSet &ps = lab_patches(s, level);
            uint64_t *o = sizes + (level == 2 ? 4 : 12);
            o[0] = ps.n_patches, o[1] = ps.npe, o[2] = ps.n_clusters, o[3] = ps.cluster_rows, o[4] = ps.cinv64.count, o[5] = ps.n_bad_elements,
            o[6] = ps.largest_cluster, o[7] = s->dropped_patches[level == 2 ? 0 : 1];
        }
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

// The standing hierarchy (mhl_system_hierarchy_sizes first).  scalars[10] = lmax of L2 and of L1, the coarse diagonal lift applied, the cycle
// shape for `width` columns (deg2, ratio, deg1, gamma, ratio1), the shift, the worst element shape.  Per mesh point in the reference numbering:
// agg_of (its aggregate), agg_t (its 3 x 6 block, row-major).  The P1 operator's node blocks: l1_row, l1_col (reference point ids), l1_val (3 x 3
// row-major).  a0: the coarse operator's explicit inverse (n0 x n0, column-major).  Any output may be null.
int mhl_system_hierarchy_export(mh_system *s, uint32_t width, double *scalars, uint32_t *agg_of, double *agg_t, uint32_t *l1_row, uint32_t *l1_col, double *l1_val,
                                double *a0) {
    if (!s || !scalars || width == 0) return MH_EINVAL;
    mh_context *ctx = s->ctx;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        std::lock_guard<std::mutex> lock(mh_solve_mutex());
        if (!s->hierarchy_ready) mh_throw(MH_EINVAL, "hierarchy export: no hierarchy built");
        MhCycleShape sh;
        mh_cycle_shape(s, width, &sh);
        const double sc[10] = {s->L2.lmax, s->L1.lmax, mh_coarse_lift(s), double(sh.deg2), sh.ratio, double(sh.deg1), double(sh.gamma), sh.ratio1, s->sigma_built,
                               double(s->worst_quality)};
        std::copy(sc, sc + 10, scalars);
        const std::vector<uint32_t> ref = lab_point_ref(s);
        if (agg_of) {
            const std::vector<uint32_t> h = s->agg_of.to_host();
            for (uint32_t p = 0; p < s->n_points; ++p) agg_of[ref[p]] = h[p];
        }
        if (agg_t) {
            const std::vector<double> h = s->agg_t.to_host();
            for (uint32_t p = 0; p < s->n_points; ++p) std::copy(h.begin() + 18 * size_t(p), h.begin() + 18 * size_t(p + 1), agg_t + 18 * size_t(ref[p]));
        }
        if (l1_row || l1_col) {
            const std::vector<uint32_t> rp = s->L1.row_ptr.to_host(), cl = s->L1.col.to_host();
            for (uint32_t r = 0; r < s->L1.n_nodes; ++r)
                for (uint32_t b = rp[r]; b < rp[r + 1]; ++b) {
                    if (l1_row) l1_row[b] = ref[r];
                    if (l1_col) l1_col[b] = ref[cl[b]];
                }
        }
        if (l1_val) s->L1.aval.download(l1_val, s->L1.n_blocks * 9);
        if (a0) s->a0.download(a0, s->a0.count);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

// The sliver patches of level 2 (P2) or 1 (P1) of the standing hierarchy: nodes (patches x nodes per patch, the reference's node ids of that level:
// P2 nodes, or mesh points), weight, inv64 (per patch its weighted inverse, row-major); per cluster: cluster_row (its DOF rows, 3 node + k in the
// reference numbering), cluster_ptr (clusters + 1 row offsets), cinv64 (its inverse, order^2 values each, row-major).  Any output may be null.
int mhl_system_patch_export(mh_system *s, int level, uint32_t *nodes, double *weight, double *inv64, uint32_t *cluster_row, uint32_t *cluster_ptr, double *cinv64) {
    if (!s || (level != 1 && level != 2)) return MH_EINVAL;
    mh_context *ctx = s->ctx;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        std::lock_guard<std::mutex> lock(mh_solve_mutex());
        if (!s->hierarchy_ready) mh_throw(MH_EINVAL, "patch export: no hierarchy built");
        const PatchSet &ps = lab_patches(s, level);
        std::vector<uint32_t> node_ref;
        if (level == 2) node_ref = s->perm.to_host();
        else node_ref = lab_point_ref(s);
        if (nodes && ps.n_patches) {
            const std::vector<uint32_t> h = ps.nodes.to_host();
            for (size_t i = 0; i < h.size(); ++i) nodes[i] = node_ref[h[i]];
        }
        if (weight && ps.n_patches) ps.weight.download(weight, ps.n_patches);
        if (inv64 && ps.n_patches) ps.inv64.download(inv64, ps.inv64.count);
        if (cluster_row && ps.n_clusters) {
            const std::vector<uint32_t> h = ps.cluster_row.to_host();
            for (size_t i = 0; i < h.size(); ++i) cluster_row[i] = 3 * node_ref[h[i] / 3] + h[i] % 3;
        }
        if (cluster_ptr && ps.n_clusters) std::copy(ps.h_cluster_ptr.begin(), ps.h_cluster_ptr.end(), cluster_ptr);
        if (cinv64 && ps.n_clusters) ps.cinv64.download(cinv64, ps.cinv64.count);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

// The Cholesky-QR step's one-launch kernel: l <- diag(1 / dscale) chol(a) (lower, zeros above), linv <- l^-1; info[0] = 0 or the failing column,
// info[1] = the diagonal spread report.  Column-major host arrays of order w <= 128.
int mhl_context_potrf_inverse(mh_context *ctx, uint32_t w, const double *a, const double *dscale, double *l, double *linv, int *info2) {
    if (!ctx || !a || !dscale || !l || !linv || !info2 || w < 1 || w > 128) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        MhSharedPhase not_during_a_factorisation(ctx->device);
        DevArray<double> da(ctx, size_t(w) * w), dd(ctx, w), dl(ctx, size_t(w) * w);
        DevArray<int> info(ctx, 2);
        da.upload(a, size_t(w) * w);
        dd.upload(dscale, w);
        mh_potrf_small_inverse(ctx, da, w, info, dd, dl);
        da.download(l, size_t(w) * w);
        dl.download(linv, size_t(w) * w);
        info.download(info2, 2);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

// out = a^-1 for a symmetric positive definite a of order w <= 128 (column-major host arrays) through the coarse set-up's one-workgroup
// Gauss-Jordan kernel; the average of `reps` launches, HIP events around each.
int mhl_context_spd_inverse(mh_context *ctx, uint32_t w, const double *a, double *out, uint32_t reps, double *avg_ms) {
    if (!ctx || !a || !out || w < 1 || w > 128) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        MhSharedPhase not_during_a_factorisation(ctx->device);
        DevArray<double> da(ctx, size_t(w) * w), dout(ctx, size_t(w) * w);
        DevArray<int> info(ctx, 1);
        info.zero();
        da.upload(a, size_t(w) * w);
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        float total = 0;
        for (uint32_t r = 0; r < std::max(1u, reps); ++r) {
            HIP_CHECK(hipEventRecord(e0, ctx->stream));
            mh_spd_inverse_small(ctx, da, w, w, dout, w, info);
            HIP_CHECK(hipEventRecord(e1, ctx->stream));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            total += ms;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        dout.download(out, size_t(w) * w);
        int hinfo = 0;
        info.download(&hinfo, 1);
        if (avg_ms) *avg_ms = total / std::max(1u, reps);
        return hinfo ? MH_EFACTOR : MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

// C = alpha op(A) op(B) + beta C with the Rayleigh-Ritz step's small-product kernel (column-major host arrays; c in and out).
int mhl_context_small_gemm(mh_context *ctx, int ta, int tb, uint32_t M, uint32_t N, uint32_t K, double alpha, const double *a, uint32_t lda, const double *b, uint32_t ldb, double beta,
                           double *c, uint32_t ldc, uint32_t reps, double *avg_ms) {
    if (!ctx || !a || !b || !c || !M || !N || !K || lda < (ta ? K : M) || ldb < (tb ? N : K) || ldc < M) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        MhSharedPhase not_during_a_factorisation(ctx->device);
        const size_t na = size_t(lda) * (ta ? M : K), nb = size_t(ldb) * (tb ? K : N), nc = size_t(ldc) * N;
        DevArray<double> da(ctx, na), db(ctx, nb), dc(ctx, nc), work(ctx, nc);
        da.upload(a, na);
        db.upload(b, nb);
        dc.upload(c, nc);
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        float total = 0;
        for (uint32_t r = 0; r < std::max(1u, reps); ++r) {
            HIP_CHECK(hipMemcpyAsync(work, dc, nc * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
            HIP_CHECK(hipEventRecord(e0, ctx->stream));
            mh_small_gemm(ctx, ta != 0, tb != 0, M, N, K, alpha, da, lda, db, ldb, beta, work, ldc);
            HIP_CHECK(hipEventRecord(e1, ctx->stream));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            total += ms;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        work.download(c, nc);
        if (avg_ms) *avg_ms = total / std::max(1u, reps);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

// The context's device pool: bytes held from the device, bytes of them idle in the cache, and the cap on the idle part.
int mhl_context_pool_stats(mh_context *ctx, uint64_t *reserved, uint64_t *idle, uint64_t *cap) {
    if (!ctx || !reserved || !idle || !cap) return MH_EINVAL;
    *reserved = ctx->pool.bytes_reserved;
    *idle = ctx->pool.bytes_idle;
    *cap = ctx->pool.cap;
    return MH_OK;
}

// G (wa x wb, column-major) = X^T Y for row-major host panels X (n x wa), Y (n x wb): the solver's Gram kernel, for parity tests.
int mhl_context_gram(mh_context *ctx, uint64_t n, const double *x, uint32_t wa, const double *y, uint32_t wb, double *g) {
    if (!ctx || !x || !y || !g || !n || !wa || !wb) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        MhSharedPhase not_during_a_factorisation(ctx->device);
        DevArray<double> dx(ctx, n * wa), dy(ctx, n * wb), dg(ctx, size_t(wa) * wb);
        dx.upload(x, n * wa);
        dy.upload(y, n * wb);
        mh_gram(ctx, n, dx, wa, dy, wb, dg, wa);
        dg.download(g, size_t(wa) * wb);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

// Measured HBM ceilings of this device (SURVEY 8d asks for a measured copy-kernel ceiling beside the nominal 8 TB/s): a streaming copy
// (bytes read + bytes written per second) and a streaming read (a sum stored once per workgroup); 16-byte accesses, grid-stride, 16
// workgroups per CU.
int mhl_context_bench_stream(mh_context *ctx, uint64_t bytes, uint32_t reps, double *copy_gbs, double *read_gbs) {
    if (!ctx || !copy_gbs || !read_gbs || bytes < 4096 || !reps) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        MhSharedPhase not_during_a_factorisation(ctx->device);
        const size_t count = bytes / 16;
        const unsigned grid = unsigned(ctx->cu_count) * 32;
        DevArray<float> a(ctx, count * 4), b(ctx, count * 4), out(ctx, grid);
        a.zero();
        out.zero();
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        auto timed = [&](auto &&launch) {
            launch();
            HIP_CHECK(hipEventRecord(e0, ctx->stream));
            for (uint32_t r = 0; r < reps; ++r) launch();
            HIP_CHECK(hipEventRecord(e1, ctx->stream));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            return double(ms) * 1e-3 / reps;
        };
        // the best of a few forms of each (bytes in flight per lane, temporal or not, workgroups per CU): a ceiling, not a kernel of the path
        double t_copy = 1e30, t_read = 1e30;
        const f4_stream *src = reinterpret_cast<const f4_stream *>(a.get());
        f4_stream *dst = reinterpret_cast<f4_stream *>(b.get());
        for (unsigned per_cu : {4u, 8u, 16u, 32u}) {
            const unsigned g = std::min(grid, unsigned(ctx->cu_count) * per_cu);
            t_copy = std::min(t_copy, timed([&] { k_stream_copy<<<g, 256, 0, ctx->stream>>>(src, dst, count); }));
            t_copy = std::min(t_copy, timed([&] { k_stream_copy_u<4, false><<<g, 256, 0, ctx->stream>>>(src, dst, count); }));
            t_copy = std::min(t_copy, timed([&] { k_stream_copy_u<8, false><<<g, 256, 0, ctx->stream>>>(src, dst, count); }));
            t_copy = std::min(t_copy, timed([&] { k_stream_copy_u<4, true><<<g, 256, 0, ctx->stream>>>(src, dst, count); }));
            t_copy = std::min(t_copy, timed([&] { k_stream_copy_u<8, true><<<g, 256, 0, ctx->stream>>>(src, dst, count); }));
            t_copy = std::min(t_copy, timed([&] { k_stream_copy_u<16, false><<<g, 256, 0, ctx->stream>>>(src, dst, count); }));
            t_copy = std::min(t_copy, timed([&] { k_stream_copy_u<16, true><<<g, 256, 0, ctx->stream>>>(src, dst, count); }));
            t_copy = std::min(t_copy, timed([&] { k_stream_copy_u<8, true, 256, false><<<g, 256, 0, ctx->stream>>>(src, dst, count); })); // non-temporal stores only
            t_copy = std::min(t_copy, timed([&] { k_stream_copy_u<8, false, 1024><<<g / 4 + 1, 1024, 0, ctx->stream>>>(src, dst, count); }));
            t_copy = std::min(t_copy, timed([&] { k_stream_copy_u<4, true, 1024><<<g / 4 + 1, 1024, 0, ctx->stream>>>(src, dst, count); }));
            t_copy = std::min(t_copy, timed([&] { (void)hipMemcpyAsync(dst, src, count * 16, hipMemcpyDeviceToDevice, ctx->stream); })); // the runtime's own copy
            t_read = std::min(t_read, timed([&] { k_stream_read<<<g, 256, 0, ctx->stream>>>(src, count, out.get()); }));
            t_read = std::min(t_read, timed([&] { k_stream_read_u<4, false><<<g, 256, 0, ctx->stream>>>(src, count, out.get()); }));
            t_read = std::min(t_read, timed([&] { k_stream_read_u<8, false><<<g, 256, 0, ctx->stream>>>(src, count, out.get()); }));
            t_read = std::min(t_read, timed([&] { k_stream_read_u<8, true><<<g, 256, 0, ctx->stream>>>(src, count, out.get()); }));
        }
        KERNEL_CHECK();
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        *copy_gbs = 2.0 * double(count) * 16 / t_copy / 1e9;
        *read_gbs = double(count) * 16 / t_read / 1e9;
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}

}

// ---- the sparse block product's forms on a caller's matrix (tests/test_spmm_forms_gpu.py), and the helpers it shares with the dense
// products' forms at the end of this file ------------------------------------------------------------------------------------------
namespace {
// quiet NaNs with a payload: arithmetic on finite inputs produces the canonical NaN at most, never these
template<typename T> T lab_sentinel();
template<> double lab_sentinel<double>() {
    const uint64_t bits = MHL_SENTINEL64;
    double v;
    memcpy(&v, &bits, sizeof v);
    return v;
}
template<> float lab_sentinel<float>() {
    const uint32_t bits = MHL_SENTINEL32;
    float v;
    memcpy(&v, &bits, sizeof v);
    return v;
}

// A device buffer of n entries between two guards of MHL_GUARD entries, everything pre-filled with the sentinel (the body with
// `init` when given); fetch() copies guards and body back (nowhere when the caller has no array for it).  The guard is a multiple of
// 16 bytes: the body keeps the pool's alignment.
template<typename T> struct LabGuarded {
    DevArray<T> dev;
    size_t n;
    LabGuarded(mh_context *ctx, size_t n_, const T *init = nullptr) : n(n_) {
        std::vector<T> h(n + 2 * MHL_GUARD, lab_sentinel<T>());
        if (init) std::copy(init, init + n, h.begin() + MHL_GUARD);
        dev.reset(ctx, h.size());
        dev.upload(h.data(), h.size());
        HIP_CHECK(hipStreamSynchronize(ctx->stream)); // h goes out of scope
    }
    T *body() const { return dev.get() + MHL_GUARD; }
    void fetch(void *host) const {
        if (host) dev.download(static_cast<T *>(host), n + 2 * MHL_GUARD);
    }
};

template<typename T> void lab_upload(mh_context *ctx, DevArray<T> &d, const void *src, size_t n, size_t lead = 0) {
    d.reset(ctx, n + lead + 2); // (two spare entries: a pointer moved by `lead` stays inside, and no array is empty)
    if (n) HIP_CHECK(hipMemcpyAsync(d.get() + lead, src, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
}
} // namespace

extern "C" {
// One form of the BSR 3x3 product (modalhip_lab.h: MHL_SPMM_*) on the caller's matrix and panels, through the product's own dispatchers
// (mh_spmm, mh_spmm_f32, mh_spmm_mixed, mh_spmm_mapped, mh_spmm_f32_cheb_step): no node permutation, no kernel chosen here.  Every
// output comes back whole, guards included.  The arguments are checked on the host so that no launch reads or writes outside its arrays.
int mhl_context_spmm_form(mh_context *ctx, mhl_spmm_request *q) {
    if (!ctx || !q || !q->row_ptr || !q->col || !q->x || q->n_nodes == 0 || q->w == 0 || q->w > 4096) return MH_EINVAL;
    const int form = q->form;
    if (form < MHL_SPMM_F64_A || form > MHL_SPMM_F32_CHEB) return MH_EINVAL;
    const bool f64_plain = form <= MHL_SPMM_F64_AM, mapped = form == MHL_SPMM_MAPPED || form == MHL_SPMM_MAPPED_RES, cheb = form == MHL_SPMM_F32_CHEB;
    const bool with_a = form != MHL_SPMM_F64_M, with_m = form == MHL_SPMM_F64_M || form == MHL_SPMM_F64_AM || mapped;
    const bool vals_f32 = form == MHL_SPMM_F32_A || cheb, x_f32 = vals_f32 || form == MHL_SPMM_MIXED;
    if ((with_a && (!q->vals9 || (!q->y && !cheb))) || (with_m && (!q->mscal || !q->y2)) || (q->misalign && !f64_plain)) return MH_EINVAL;
    const uint32_t nn = q->n_nodes, w = q->w;
    if (q->row_ptr[0] != 0) return MH_EINVAL;
    for (uint32_t i = 0; i < nn; ++i)
        if (q->row_ptr[i + 1] < q->row_ptr[i]) return MH_EINVAL;
    const uint32_t nblocks = q->row_ptr[nn];
    for (uint32_t p = 0; p < nblocks; ++p)
        if (q->col[p] >= nn) return MH_EINVAL;
    if (mapped) {
        if (!q->omap || q->ldy == 0 || q->wreal == 0 || q->wreal > w) return MH_EINVAL;
        for (uint32_t c = 0; c < q->wreal; ++c)
            if (q->omap[c] >= q->ldy) return MH_EINVAL;
        if (form == MHL_SPMM_MAPPED_RES && (!q->theta || !q->r_out || !q->partial)) return MH_EINVAL;
    }
    if (cheb && (!q->dinv32 || !q->r || !q->xs || !q->cheb_r || !q->cheb_d_out || !q->cheb_x || !q->cheb_d_in)) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        MhSharedPhase not_during_a_factorisation(ctx->device);
        const size_t rows = size_t(3) * nn, panel = rows * w;
        BsrLevel lvl;
        lvl.n_nodes = nn;
        lvl.n_blocks = nblocks;
        lab_upload(ctx, lvl.row_ptr, q->row_ptr, size_t(nn) + 1);
        lab_upload(ctx, lvl.col, q->col, nblocks);
        if (with_a && vals_f32) lab_upload(ctx, lvl.aval32, q->vals9, size_t(9) * nblocks);
        else if (with_a) lab_upload(ctx, lvl.aval, q->vals9, size_t(9) * nblocks);
        if (with_m) lab_upload(ctx, lvl.mval, q->mscal, nblocks);
        q->taken = 1;
        if (cheb) {
            DevArray<float> dinv;
            lab_upload(ctx, dinv, q->dinv32, rows);
            LabGuarded<float> d_in(ctx, panel, static_cast<const float *>(q->x)), d_out(ctx, panel), r(ctx, panel, q->r), xs(ctx, panel, q->xs);
            q->taken = mh_spmm_f32_cheb_step(ctx, lvl, d_in.body(), d_out.body(), r.body(), xs.body(), dinv, q->c1, q->c2, w) ? 1 : 0;
            d_in.fetch(q->cheb_d_in);
            d_out.fetch(q->cheb_d_out);
            r.fetch(q->cheb_r);
            xs.fetch(q->cheb_x);
            return MH_OK;
        }
        const size_t lead = q->misalign ? 1 : 0; // 8 bytes into a larger allocation: launch_spmm_wide's aligned16 test fails
        DevArray<double> x64;
        DevArray<float> x32;
        if (x_f32) lab_upload(ctx, x32, q->x, panel);
        else lab_upload(ctx, x64, q->x, panel, lead);
        if (mapped) {
            const size_t out = rows * q->ldy;
            LabGuarded<double> y(ctx, out), y2(ctx, out);
            if (form == MHL_SPMM_MAPPED_RES) {
                DevArray<uint32_t> omap;
                DevArray<double> theta, dinv;
                lab_upload(ctx, omap, q->omap, q->wreal);
                lab_upload(ctx, theta, q->theta, w);
                if (q->dinv) lab_upload(ctx, dinv, q->dinv, rows);
                LabGuarded<double> r_out(ctx, panel), partial(ctx, size_t(2) * nn * w);
                mh_spmm_mapped(ctx, lvl, lvl.aval, x64, y.body(), lvl.mval, y2.body(), w, q->ldy, q->wreal, omap, theta, r_out.body(), partial.body(), q->dinv ? dinv.get() : nullptr);
                r_out.fetch(q->r_out);
                partial.fetch(q->partial);
            } else {
                DevArray<uint32_t> omap;
                lab_upload(ctx, omap, q->omap, q->wreal);
                mh_spmm_mapped(ctx, lvl, lvl.aval, x64, y.body(), lvl.mval, y2.body(), w, q->ldy, q->wreal, omap);
                HIP_CHECK(hipStreamSynchronize(ctx->stream)); // omap goes out of scope
            }
            y.fetch(q->y);
            y2.fetch(q->y2);
            return MH_OK;
        }
        if (form == MHL_SPMM_F32_A) {
            LabGuarded<float> y(ctx, panel);
            mh_spmm_f32(ctx, lvl, x32, y.body(), w);
            y.fetch(q->y);
            return MH_OK;
        }
        if (form == MHL_SPMM_MIXED) {
            LabGuarded<double> y(ctx, panel);
            mh_spmm_mixed(ctx, lvl, x32, y.body(), w);
            y.fetch(q->y);
            return MH_OK;
        }
        LabGuarded<double> y(ctx, with_a ? panel : 0), y2(ctx, with_m ? panel : 0);
        mh_spmm(ctx, lvl, with_a ? lvl.aval.get() : nullptr, x64.get() + lead, with_a ? y.body() : nullptr, with_m ? lvl.mval.get() : nullptr, with_m ? y2.body() : nullptr, w);
        if (with_a) y.fetch(q->y);
        if (with_m) y2.fetch(q->y2);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}
}

// ---- the dense tall products' forms on a caller's arrays (tests/test_combine_forms_gpu.py) -----------------------------------------
namespace {
bool lab_map_inside(const uint32_t *map, uint32_t count, uint32_t limit) {
    for (uint32_t c = 0; c < count; ++c)
        if (map[c] >= limit) return false;
    return true;
}
// The request's coefficient matrix on the device, k-major m x nc: uploaded as it is, or packed there by the solver's packer into a
// guarded buffer that returns to the caller as ct_out.
struct LabCoefficients {
    DevArray<double> plain, c1, c2;
    std::optional<LabGuarded<double>> packed;
    const double *ct{nullptr};
    static bool valid(const mhl_dense_request *q, uint32_t m, uint32_t nc) {
        if (q->coeff_layout == MHL_COEFF_KMAJOR) return q->ct != nullptr;
        if ((q->pack_a && !q->c1) || (q->pack_b && !q->c2)) return false;
        if (q->coeff_layout == MHL_COEFF_BLOCKS) return q->pack_a + q->pack_b == nc && q->pack_ld >= m;
        return q->coeff_layout == MHL_COEFF_STACKED && q->pack_a + q->pack_b == m;
    }
    LabCoefficients(mh_context *ctx, const mhl_dense_request *q, uint32_t m, uint32_t nc) {
        if (q->coeff_layout == MHL_COEFF_KMAJOR) {
            lab_upload(ctx, plain, q->ct, size_t(m) * nc);
            ct = plain.get();
            return;
        }
        packed.emplace(ctx, size_t(m) * nc);
        const bool blocks = q->coeff_layout == MHL_COEFF_BLOCKS;
        lab_upload(ctx, c1, q->c1, blocks ? size_t(q->pack_ld) * q->pack_a : size_t(q->pack_a) * nc);
        lab_upload(ctx, c2, q->c2, blocks ? size_t(q->pack_ld) * q->pack_b : size_t(q->pack_b) * nc);
        if (blocks) mh_pack_coefficients(ctx, c1, q->pack_a, c2, q->pack_b, m, q->pack_ld, packed->body());
        else mh_pack_stacked(ctx, c1, q->pack_a, c2, q->pack_b, nc, q->pack_scale, packed->body());
        ct = packed->body();
    }
    void fetch(double *host) const {
        if (packed) packed->fetch(host);
    }
};
} // namespace

extern "C" {
// One form of the dense tall products (modalhip_lab.h: MHL_DENSE_*) through the solver's own dispatchers: no kernel and no launch shape is
// chosen here.  The request is checked on the host for what the dispatchers take on trust -- pointers, maps and pitches that stay inside
// the arrays -- and for nothing that they check themselves (column ranges, the combinations a second destination allows, the width limits).
int mhl_context_dense_form(mh_context *ctx, mhl_dense_request *q) {
    if (!ctx || !q) return MH_EINVAL;
    q->dispatched = 0;
    q->cu_count = ctx->cu_count;
    const int form = q->form;
    if (form < MHL_DENSE_COMBINE || form > MHL_DENSE_PACK) return MH_EINVAL;
    const size_t n = q->n;
    const uint32_t wx = q->wx, ww = q->ww, wp = q->wp, nc = q->nc, n1 = q->n1, ldx = q->ldx ? q->ldx : wx;
    const uint32_t m = form == MHL_DENSE_GRAM ? 0 : wx + ww + wp;
    if (form != MHL_DENSE_GRAM && (!m || !nc || nc > 4096 || m > 4096 || !LabCoefficients::valid(q, m, nc))) return MH_EINVAL;
    if (form != MHL_DENSE_PACK && (!n || (wx && !q->x) || (ww && !q->w) || (wp && !q->p))) return MH_EINVAL;
    if (q->xmap ? !lab_map_inside(q->xmap, wx, ldx) : ldx < wx) return MH_EINVAL;
    const uint32_t ld1 = q->ld1 ? q->ld1 : n1, ldy = q->ldy ? q->ldy : ww;
    if (form == MHL_DENSE_COMBINE) {
        if (n1 > nc || (nc > n1 && !q->out2) || q->in_place < 0 || q->in_place > 2 || (q->in_place && !q->x)) return MH_EINVAL;
        if (q->in_place == 1 ? (q->out1 || ld1 != ldx) : !q->out1) return MH_EINVAL;
        if (q->omap ? !lab_map_inside(q->omap, n1, ld1) : ld1 < n1) return MH_EINVAL;
        if (q->in_place == 2 ? (q->out1_also || (q->ld1_also && q->ld1_also != ldx)) : (q->out1_also && !q->ld1_also)) return MH_EINVAL;
        if (q->omap_also && !lab_map_inside(q->omap_also, n1, q->in_place == 2 ? ldx : q->ld1_also)) return MH_EINVAL;
    } else if (form == MHL_DENSE_SHORT_PRODUCT) {
        if (ww || wp || ldx != wx || q->xmap || !q->out1 || !q->slices || q->slices > 64 || (q->slices > 1 && !q->partial)) return MH_EINVAL;
    } else if (form == MHL_DENSE_GRAM) {
        if (!wx || !ww || ldx != wx || q->xmap || !q->g || q->ld < q->g_row0 + wx || q->g_cols < q->g_col0 + ww) return MH_EINVAL;
        if (q->ymap ? !lab_map_inside(q->ymap, ww, ldy) : ldy < ww) return MH_EINVAL;
    }
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        MhSharedPhase not_during_a_factorisation(ctx->device);
        if (form == MHL_DENSE_PACK) {
            q->dispatched = 1;
            const LabCoefficients coeff(ctx, q, m, nc);
            coeff.fetch(q->ct_out);
            return MH_OK;
        }
        LabGuarded<double> x(ctx, n * ldx, q->x);
        DevArray<double> w, p;
        if (q->w) lab_upload(ctx, w, q->w, n * (form == MHL_DENSE_GRAM ? ldy : ww));
        if (q->p) lab_upload(ctx, p, q->p, n * wp);
        if (form == MHL_DENSE_GRAM) {
            DevArray<uint32_t> ymap;
            if (q->ymap) lab_upload(ctx, ymap, q->ymap, ww);
            LabGuarded<double> g(ctx, size_t(q->ld) * q->g_cols);
            q->dispatched = 1;
            mh_gram(ctx, n, x.body(), wx, w, ww, g.body() + size_t(q->g_col0) * q->ld + q->g_row0, q->ld, q->ldy, q->ymap ? ymap.get() : nullptr);
            g.fetch(q->g);
            x.fetch(q->x_out);
            return MH_OK;
        }
        const LabCoefficients coeff(ctx, q, m, nc);
        const double *xd = q->x ? x.body() : nullptr;
        if (form == MHL_DENSE_SHORT_PRODUCT) {
            LabGuarded<double> out(ctx, n * nc), partial(ctx, q->slices > 1 ? size_t(q->slices) * n * nc : 0);
            q->dispatched = 1;
            mh_short_product(ctx, n, xd, wx, coeff.ct, nc, out.body(), q->slices > 1 ? partial.body() : nullptr, q->slices);
            out.fetch(q->out1);
            if (q->slices > 1) partial.fetch(q->partial);
            x.fetch(q->x_out);
            coeff.fetch(q->ct_out);
            return MH_OK;
        }
        DevArray<uint32_t> xmap, omap, omap_also;
        if (q->xmap) lab_upload(ctx, xmap, q->xmap, wx);
        if (q->omap) lab_upload(ctx, omap, q->omap, n1);
        if (q->omap_also) lab_upload(ctx, omap_also, q->omap_also, n1);
        const bool old = q->accumulate != 0; // out += : the outputs start as the caller's values
        LabGuarded<double> out1(ctx, q->in_place == 1 ? 0 : n * ld1, old && q->out1 ? q->out1 + MHL_GUARD : nullptr);
        LabGuarded<double> out2(ctx, q->out2 ? n * (nc - n1) : 0, old && q->out2 ? q->out2 + MHL_GUARD : nullptr);
        LabGuarded<double> also(ctx, q->out1_also ? n * q->ld1_also : 0);
        double *d1 = q->in_place == 1 ? x.body() : out1.body(), *d2 = q->out2 ? out2.body() : nullptr;
        double *d_also = q->in_place == 2 ? x.body() : q->out1_also ? also.body() : nullptr;
        q->dispatched = 1;
        // (the request's layout is the lab's own: translated field by field; an absent host array is a null pointer here as it is there)
        mh_combine(ctx, n, {.x = xd, .wx = wx, .ldx = q->ldx, .xmap = q->xmap ? xmap.get() : nullptr, .w = q->w ? w.get() : nullptr, .ww = ww, .p = q->p ? p.get() : nullptr, .wp = wp,
                            .ct = coeff.ct, .nc = nc, .out1 = d1, .n1 = n1, .ld1 = q->ld1, .omap = q->omap ? omap.get() : nullptr, .out2 = d2, .accumulate = old,
                            .col_begin = q->col_begin, .col_count = q->col_count, .out1_also = d_also, .ld1_also = q->ld1_also, .omap_also = q->omap_also ? omap_also.get() : nullptr});
        HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (before anything is fetched: a launch error surfaces here, with the host arrays as passed)
        out1.fetch(q->out1);
        out2.fetch(q->out2);
        also.fetch(q->out1_also);
        x.fetch(q->x_out);
        coeff.fetch(q->ct_out);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}
}
