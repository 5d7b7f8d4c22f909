// Resonator bank on the device (gfx950): one thread per mode, coupled-form complex one-pole
//     z <- z*c + excitation,   out += p_im*Im z + p_re*Re z
// restating RenderModal / RenderObjectFast of the reference (src/audio/ModalAudio.cpp:86-147, 486-555).
//
// Bit-exactness contract: this file is compiled with -ffp-contract=off and follows the reference's expression trees
// and summation order exactly -- 8-mode chunks summed lane 0..7, chunks accumulated in ascending order into the
// renderer's buffer, objects in the renderer's deal order, renderers mixed in renderer order, click filters first --
// so the signal equals the CPU restatement's sample for sample, for fp32 (the reference's bank) and fp64 alike.
// The sequential part (ordered accumulation) is a separate pass over per-chunk partial signals staged in HBM.
#include "mh_common.h"
#include "../../include/modalhip_groups.hpp"

#include <algorithm>
#include <limits>
#include <memory>

namespace {
constexpr int LANES = 8; // ModalAudio.h:169
constexpr int WAVE = 64;

template<typename Real> struct ImpactDev {
    uint32_t object, ex_pos, samples_left, pad;
    Real jx, jy, jz, phase_re, phase_im, rot_re, rot_im, gamma, accel_amp, b0, a1, a2, z1, z2;
};

template<typename Real> struct ImpactBack { // an impact's state after the block, as the host reads it back
    uint32_t samples_left;
    Real phase_re, phase_im, z1, z2;
};

struct WaveDesc {
    uint32_t dealt; // index into the flattened deal
    uint32_t first_mode; // first mode of this wave inside the object (multiple of MODES_PER_WAVE)
};

// Force curve + click filter per impact (ModalAudio.cpp:504-538).  force/click: [impact][frames].
template<typename Real>
__global__ void k_bank_forces(ImpactDev<Real> *__restrict__ impacts, uint32_t n_impacts, const Real *__restrict__ listener_gain, Real click_gain,
                              uint32_t frames, Real *__restrict__ force, Real *__restrict__ click, ImpactBack<Real> *__restrict__ back) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_impacts) return;
    ImpactDev<Real> im = impacts[i];
    Real phase_re = im.phase_re, phase_im = im.phase_im;
    const Real rot_re = im.rot_re, rot_im = im.rot_im, gamma = im.gamma, amp = im.accel_amp, b0 = im.b0, a1 = im.a1, a2 = im.a2;
    const Real impact_click_gain = click_gain * listener_gain[im.object];
    Real z1 = im.z1, z2 = im.z2;
    uint32_t left = im.samples_left;
    Real *f = force + size_t(i) * frames, *ck = click + size_t(i) * frames;
    auto sample = [&](Real &force_out, Real &click_out) {
        Real cur = 0;
        if (left > 0) {
            const Real re = phase_re * rot_re - phase_im * rot_im;
            phase_im = phase_re * rot_im + phase_im * rot_re;
            phase_re = re;
            cur = gamma * Real(0.5) * (Real(1) - phase_re);
            --left;
        }
        force_out = cur;
        const Real u = amp * cur;
        const Real y = b0 * u + z1;
        z1 = -a1 * y + z2;
        z2 = -b0 * u - a2 * y;
        click_out = y * impact_click_gain;
    };
    // every thread writes its own two rows: four samples per store (a wave's store touches 64 rows either way, and the loop was
    // bound by issuing those stores, not by its recurrences)
    typedef Real Quad __attribute__((ext_vector_type(4)));
    uint32_t s = 0;
    if ((frames & 3u) == 0) {
        for (; s < frames; s += 4) {
            Real fv[4], cv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) sample(fv[u], cv[u]);
            *reinterpret_cast<Quad *>(f + s) = Quad{fv[0], fv[1], fv[2], fv[3]};
            *reinterpret_cast<Quad *>(ck + s) = Quad{cv[0], cv[1], cv[2], cv[3]};
        }
    }
    for (; s < frames; ++s) sample(f[s], ck[s]);
    im.phase_re = phase_re;
    im.phase_im = phase_im;
    im.samples_left = left;
    im.z1 = z1;
    im.z2 = z2;
    impacts[i] = im;
    back[i] = {left, phase_re, phase_im, z1, z2}; // what the host takes back, written where it reads it (pinned memory)
}

// A float sample as the bank takes it from a caller: one that is not finite is 0.
template<typename Real> __device__ __forceinline__ Real finite_or_zero(float v) {
    return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u ? Real(v) : Real(0); // exponent all ones: Inf or NaN
}

// Force rows of the caller's drives (mh_bank_render_driven): the float signals become `Real` rows that follow the impacts' rows in
// `force`, so the resonator kernel addresses both kinds alike.  A sample that is not finite is rendered as 0 -- one NaN would ring in
// the state for ever.  No curve, no click filter, no state: a drive lasts for the block it was passed with.
template<typename Real>
__global__ void __launch_bounds__(256) k_bank_drive_rows(const float *__restrict__ signals, size_t n, Real *__restrict__ rows) {
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    rows[i] = finite_or_zero<Real>(signals[i]);
}

template<typename Real> struct BankCols {
    Real *coeff_re, *coeff_im, *state_re, *state_im, *rad_gain, *phase_im, *phase_re, *shape_x, *shape_y, *shape_z;
    const uint32_t *mode_offset, *mode_count, *shape_offset;
};

// Cross-lane moves that stay on the VALU (no LDS crossbar): lane i reads lane i+N of its 16-lane row, and a
// wave-uniform lane broadcast.
template<int N> __device__ __forceinline__ float row_shl(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + N, 0xf, 0xf, true));
}
template<int N> __device__ __forceinline__ double row_shl(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, int(b), 0x100 + N, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, int(b >> 32), 0x100 + N, 0xf, 0xf, true);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ float lane_bcast(float v, uint32_t l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), int(l))); }
__device__ __forceinline__ double lane_bcast(double v, uint32_t l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane(int(b), int(l)), hi = __builtin_amdgcn_readlane(int(b >> 32), int(l));
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// One wave = 128 consecutive modes of one dealt object = 16 chunks, two adjacent modes per lane: the resonator arithmetic is
// issue bound (every operation its own instruction -- no contraction, the reference's expression tree), and on a pair of fp32
// values one packed instruction does the work of two (the fp64 bank runs the same code unpacked).  partial: [global chunk][frames].
// Samples run in tiles of TS: during a tile every lane advances its two resonators sample by sample and drops their output terms
// into an LDS tile [sample][mode]; after the tile the wave turns around -- lane = (chunk group, sample) -- and adds each chunk's 8
// terms in mode order 0..7, which is the reference's summation order at two LDS reads per mode-sample instead of a cross-lane
// chain per sample, and makes the partial-signal stores contiguous in the sample.
//
// Force rows.  An object's rows are its impacts in impact-list order, then its drives in the caller's order (imp_idx lists both: a drive
// is an ImpactDev entry behind the impacts, with a force row at the same index).  Per sample the excitation is the running sum over
// them, from +0.  Up to IMP_REG rows: gain and force tile in registers (run).  IMP_REG < rows <= ROWS_MAX, in a launch that carries
// drives (MANY): run_rows -- the force tiles of all rows go to LDS once per 32-sample tile, [sample][row], so that a sample's forces
// arrive with one or two wave-uniform LDS reads instead of a lane broadcast per row; the gains of the first ROWS_REG rows stay in
// registers, those of the rows behind them in LDS.  More rows than that (or a drive-free launch): the scratch-row path (EXTRA).
//
// Pickups (READ, mh_bank_render_read).  A wave of an object that carries pickups also keeps the tile's states -- Im z and Re z after each
// sample's step, [sample][mode] like the output terms -- and at the turn-around every lane (half, sample) adds, per pickup, the 64 modes of
// its half: acc = fma(g_im[k], Im z[k], acc), then acc = fma(g_re[k], Re z[k], acc), even modes into one accumulator and odd modes into a
// second one (a packed pair), k ascending, from +0; the lane's value is even + odd.  The gains of the object's pickups are staged once per
// block in LDS, [pickup][im | re][mode], and read wave-uniformly per half.  Each (wave, half) writes its own partial row; k_bank_read_rows
// adds an object's rows in ascending (wave, half) order, so a pickup's row does not depend on the deal or on anything else in the call.
// Waves of objects without a pickup take no part in any of it.
constexpr int MODES_PER_WAVE = 2 * WAVE;
constexpr uint32_t IMP_REG = 2, ROWS_REG = 8, ROWS_MAX = 12;
constexpr uint32_t PITCH = MODES_PER_WAVE + 2, CHUNKS = MODES_PER_WAVE / LANES; // a turn-around tile's row; chunks of a wave
constexpr uint32_t waves_of(uint32_t count) { return (count + MODES_PER_WAVE - 1) / MODES_PER_WAVE; }
template<typename Real> using PairOf = Real __attribute__((ext_vector_type(2)));

// A lane's share of a wave: two adjacent modes of one dealt object -- state, coefficients and output phases, zero where the object
// renders no such mode -- and where the wave's chunks go.  `count` is what the wave renders of the object: 0 for a wave that holds
// nothing (nothing is loaded or stored for it).
template<typename Real> struct WaveLane {
    uint32_t k0, stride, shape0, k; // the object's first mode, its mode count, its first shape entry; this lane's modes: k, k + 1
    bool live[2];
    uint32_t chunk0, chunks_here; // global index of this wave's first chunk; how many of its chunks hold a rendered mode
    PairOf<Real> z_re, z_im, c_re, c_im, p_re, p_im;
    Real mix_gain;
};
template<typename Real>
__device__ __forceinline__ WaveLane<Real> load_wave(const BankCols<Real> &b, const uint32_t *deal_objects, const uint32_t *chunk_base, const Real *out_gain,
                                                    const Real *listener_gain, uint32_t dealt, uint32_t first_mode, uint32_t count, uint32_t lane) {
    const uint32_t o = deal_objects[dealt];
    WaveLane<Real> w{};
    w.k0 = b.mode_offset[o], w.stride = b.mode_count[o], w.shape0 = b.shape_offset[o];
    w.k = first_mode + 2 * lane;
    w.live[0] = w.k < count, w.live[1] = w.k + 1 < count;
    w.chunk0 = chunk_base[dealt] + first_mode / LANES;
    w.chunks_here = min(CHUNKS, (count - first_mode + LANES - 1) / LANES);
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (w.live[h]) {
            w.z_re[h] = b.state_re[w.k0 + w.k + h]; w.z_im[h] = b.state_im[w.k0 + w.k + h];
            w.c_re[h] = b.coeff_re[w.k0 + w.k + h]; w.c_im[h] = b.coeff_im[w.k0 + w.k + h];
            w.p_im[h] = b.phase_im[w.k0 + w.k + h]; w.p_re[h] = b.phase_re[w.k0 + w.k + h];
        }
    w.mix_gain = out_gain[o] * listener_gain[o];
    return w;
}
// Gain pair of a force row -- an impact or a drive -- on this lane's modes (ImpactGainRow, ModalAudio.h:182-188); zero on padded modes.
template<typename Real> __device__ __forceinline__ Real row_gain_of(const BankCols<Real> &b, const WaveLane<Real> &w, const ImpactDev<Real> &im, int h) { // w.live[h] only
    const uint32_t base = w.shape0 + im.ex_pos * w.stride + w.k + h;
    return b.rad_gain[w.k0 + w.k + h] * (b.shape_x[base] * im.jx + b.shape_y[base] * im.jy + b.shape_z[base] * im.jz);
}
template<typename Real> __device__ __forceinline__ PairOf<Real> row_gain(const BankCols<Real> &b, const WaveLane<Real> &w, const ImpactDev<Real> &im) {
    return {w.live[0] ? row_gain_of(b, w, im, 0) : Real(0), w.live[1] ? row_gain_of(b, w, im, 1) : Real(0)};
}
// Three shape points blended along a direction: where a pickup reads and where a junction's side touches.  Per mode
// along = (w0 s[p0] + w1 s[p1] + w2 s[p2]) . n and read = scale * along * DeflectionGain; a read that looks `advance` free steps ahead
// (0, 1 or 2) has the gains of that row of ModeReadGains::Fill: read, 0; read c_re, read c_im; read (c_re^2 - c_im^2), read (2 c_re c_im).
template<typename Real> struct BlendDev {
    uint32_t p0, p1, p2;
    Real w0, w1, w2, nx, ny, nz, scale;
};
template<typename Real> struct BlendRead {
    Real along, read;
};
template<typename Real>
__device__ __forceinline__ BlendRead<Real> blend_read(const BankCols<Real> &b, const WaveLane<Real> &w, const BlendDev<Real> &p, const Real *defl_gain, int h) { // w.live[h] only
    const uint32_t i0 = w.shape0 + p.p0 * w.stride + w.k + h, i1 = w.shape0 + p.p1 * w.stride + w.k + h, i2 = w.shape0 + p.p2 * w.stride + w.k + h;
    const Real sx = p.w0 * b.shape_x[i0] + p.w1 * b.shape_x[i1] + p.w2 * b.shape_x[i2];
    const Real sy = p.w0 * b.shape_y[i0] + p.w1 * b.shape_y[i1] + p.w2 * b.shape_y[i2];
    const Real sz = p.w0 * b.shape_z[i0] + p.w1 * b.shape_z[i1] + p.w2 * b.shape_z[i2];
    const Real along = sx * p.nx + sy * p.ny + sz * p.nz;
    return {along, p.scale * along * defl_gain[w.k0 + w.k + h]};
}
template<typename Real> struct ReadGains {
    Real im, re; // on Im z and on Re z
};
template<typename Real> __device__ __forceinline__ ReadGains<Real> read_gains(Real read, Real cr, Real ci, uint32_t advance) {
    return {advance == 0 ? read : advance == 1 ? read * cr : read * (cr * cr - ci * ci), advance == 0 ? Real(0) : advance == 1 ? read * ci : read * (Real(2) * cr * ci)};
}
// The turn-around's sums, after a tile's samples and the caller's barrier: lane = (chunk group, sample) -- sample lane % TS of the
// WAVE / TS groups' chunks -- adds each of its chunks' 8 terms in mode order 0..7 from the tile [sample][mode] and stores the partial signal.
// (The loops sit in a lambda called on the spot: hipcc unrolls a lambda's loops before it inlines it and a named function's after, and in
// the second form every mode kernel takes two more vector registers -- profiles/bank_refactor_resources.txt.)
template<uint32_t TS, typename Real>
__device__ __forceinline__ void chunk_sums(const Real *tile, const WaveLane<Real> &w, uint32_t lane, uint32_t s0, uint32_t sn, Real *partial, uint32_t frames) {
    constexpr uint32_t PER_GROUP = CHUNKS / (WAVE / TS);
    const uint32_t group = lane / TS, ts = lane % TS;
    if (ts >= sn) return;
    [&] {
        const Real *row = tile + ts * PITCH + group * (PER_GROUP * LANES);
#pragma unroll
        for (uint32_t c = 0; c < PER_GROUP; ++c) {
            Real acc = 0;
#pragma unroll
            for (uint32_t l = 0; l < LANES; l += 2) {
                const PairOf<Real> v = *reinterpret_cast<const PairOf<Real> *>(row + c * LANES + l);
                acc += v.x;
                acc += v.y;
            }
            const uint32_t chunk = PER_GROUP * group + c;
            if (chunk < w.chunks_here) partial[size_t(w.chunk0 + chunk) * frames + s0 + ts] = acc * w.mix_gain;
        }
    }();
}
// A wave's epilogue: the states go back, and every chunk's energy is written.
template<typename Real> __device__ __forceinline__ void store_wave(const BankCols<Real> &b, const WaveLane<Real> &w, uint32_t lane, Real *chunk_energy) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (w.live[h]) {
            b.state_re[w.k0 + w.k + h] = w.z_re[h];
            b.state_im[w.k0 + w.k + h] = w.z_im[h];
        }
    // chunk energy: sum over the chunk's valid modes in order (padded modes hold zero state); a chunk is four lanes' pairs
    const PairOf<Real> e = w.z_re * w.z_re + w.z_im * w.z_im;
    const Real e0 = w.live[0] ? e.x : Real(0), e1 = w.live[1] ? e.y : Real(0);
    Real chunk = Real(0) + e0;
    chunk += e1;
    chunk += row_shl<1>(e0);
    chunk += row_shl<1>(e1);
    chunk += row_shl<2>(e0);
    chunk += row_shl<2>(e1);
    chunk += row_shl<3>(e0);
    chunk += row_shl<3>(e1);
    if ((lane & (LANES / 2 - 1)) == 0 && lane / (LANES / 2) < w.chunks_here) chunk_energy[w.chunk0 + lane / (LANES / 2)] = chunk;
}

template<typename Real> struct PickupDev { // a pickup the block reads: its record, and where its partial rows begin
    BlendDev<Real> at;
    uint32_t advance, first_row;
};
template<typename Real> struct ReadArgs {
    const Real *defl_gain; // DeflectionGain column
    const uint32_t *pick_ptr; // [dealt + 1] into pickups
    const PickupDev<Real> *pickups; // grouped by dealt object, the caller's order within one
    Real *rows; // [partial row][frames]
    uint32_t rows_loop; // what selects k_bank_modes_rows over k_bank_modes in a call without pickups
};
// The gains of an object's pickups on this lane's modes, staged for the block: [pickup][im | re][mode], zero on padded modes.
template<typename Real>
__device__ __forceinline__ void stage_pickup_gains(const BankCols<Real> &b, const WaveLane<Real> &w, const ReadArgs<Real> &rd, uint32_t pk0, uint32_t n_pick, uint32_t lane, Real *s_pick) {
    typedef PairOf<Real> Pair;
    for (uint32_t q = 0; q < n_pick; ++q) {
        const PickupDev<Real> pk = rd.pickups[pk0 + q];
        Pair g_im = {0, 0}, g_re = {0, 0};
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (w.live[h]) {
                const ReadGains<Real> g = read_gains(blend_read(b, w, pk.at, rd.defl_gain, h).read, w.c_re[h], w.c_im[h], pk.advance);
                g_im[h] = g.im;
                g_re[h] = g.re;
            }
        *reinterpret_cast<Pair *>(s_pick + (2 * q) * MODES_PER_WAVE + 2 * lane) = g_im;
        *reinterpret_cast<Pair *>(s_pick + (2 * q + 1) * MODES_PER_WAVE + 2 * lane) = g_re;
    }
}
// The per-half sum of G pickups from q0 on, after a tile's samples and the caller's barrier: lane = (half, sample ts) adds the 64 modes of
// its half from the state tiles [sample][mode] and the staged gains, and stores one value per pickup into the (wave, half)'s partial row.
// (The loop sits in a lambda called on the spot, as in chunk_sums.)
template<uint32_t G, typename Real>
__device__ __forceinline__ void read_group(const Real *s_zim, const Real *s_zre, const Real *s_pick, const ReadArgs<Real> &rd, uint32_t pk0, uint32_t q0, uint32_t first_mode,
                                           uint32_t half, uint32_t ts, uint32_t s0, uint32_t frames) {
    typedef PairOf<Real> Pair;
    [&] {
        Pair acc[G] = {};
        const Real *zi = s_zim + ts * PITCH + half * WAVE, *zr = s_zre + ts * PITCH + half * WAVE;
        const Real *g = s_pick + size_t(q0) * 2 * MODES_PER_WAVE + half * WAVE;
#pragma unroll 4
        for (uint32_t m = 0; m < WAVE; m += 2) {
            const Pair vi = *reinterpret_cast<const Pair *>(zi + m), vr = *reinterpret_cast<const Pair *>(zr + m);
#pragma unroll
            for (uint32_t j = 0; j < G; ++j) {
                acc[j] = __builtin_elementwise_fma(*reinterpret_cast<const Pair *>(g + (2 * j) * MODES_PER_WAVE + m), vi, acc[j]);
                acc[j] = __builtin_elementwise_fma(*reinterpret_cast<const Pair *>(g + (2 * j + 1) * MODES_PER_WAVE + m), vr, acc[j]);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < G; ++j)
            rd.rows[(size_t(rd.pickups[pk0 + q0 + j].first_row) + 2 * (first_mode / MODES_PER_WAVE) + half) * frames + s0 + ts] = acc[j].x + acc[j].y;
    }();
}
// All of an object's pickups, four at a time.
template<typename Real>
__device__ __forceinline__ void read_pickups(const Real *s_zim, const Real *s_zre, const Real *s_pick, const ReadArgs<Real> &rd, uint32_t pk0, uint32_t n_pick, uint32_t first_mode,
                                             uint32_t half, uint32_t ts, uint32_t s0, uint32_t frames) {
    uint32_t q = 0;
    for (; q + 4 <= n_pick; q += 4) read_group<4>(s_zim, s_zre, s_pick, rd, pk0, q, first_mode, half, ts, s0, frames);
    if (n_pick - q == 3) read_group<3>(s_zim, s_zre, s_pick, rd, pk0, q, first_mode, half, ts, s0, frames);
    else if (n_pick - q == 2) read_group<2>(s_zim, s_zre, s_pick, rd, pk0, q, first_mode, half, ts, s0, frames);
    else if (n_pick - q == 1) read_group<1>(s_zim, s_zre, s_pick, rd, pk0, q, first_mode, half, ts, s0, frames);
}
template<typename Real, bool MANY, bool READ = false>
__device__ __forceinline__ void bank_modes(const BankCols<Real> &b, const WaveDesc *__restrict__ waves, const uint32_t *__restrict__ deal_objects,
                                           const uint32_t *__restrict__ render_count, const uint32_t *__restrict__ chunk_base,
                                           const uint32_t *__restrict__ imp_ptr, const uint32_t *__restrict__ imp_idx,
                                           const ImpactDev<Real> *__restrict__ impacts, const Real *__restrict__ force,
                                           const Real *__restrict__ out_gain, const Real *__restrict__ listener_gain, uint32_t frames,
                                           Real *__restrict__ partial, Real *__restrict__ chunk_energy, Real *__restrict__ gain_scratch, uint32_t max_imp,
                                           const ReadArgs<Real> &rd = {}) {
    typedef PairOf<Real> Pair;
    constexpr uint32_t TS = 32;
    __shared__ __attribute__((aligned(16))) Real s_term[TS * PITCH];
    const WaveDesc wd = waves[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    WaveLane<Real> w = load_wave(b, deal_objects, chunk_base, out_gain, listener_gain, wd.dealt, wd.first_mode, render_count[wd.dealt], lane);
    const uint32_t i0 = imp_ptr[wd.dealt], n_imp = imp_ptr[wd.dealt + 1] - i0;
    // Hoisted impact gains (row_gain).  The first IMP_REG impacts of the object live in registers, further ones (rare) in a scratch row.
    Pair g_reg[IMP_REG] = {};
    uint32_t f_row[IMP_REG] = {};
    Real *g_mem = gain_scratch + size_t(blockIdx.x) * max_imp * MODES_PER_WAVE;
    const bool many_rows = MANY && (!READ || rd.rows_loop) && n_imp > IMP_REG && n_imp <= ROWS_MAX; // run_rows computes its own gains
    auto gain_of = [&](uint32_t t) { return row_gain(b, w, impacts[imp_idx[i0 + t]]); };
    for (uint32_t t = 0; t < (many_rows ? 0u : n_imp); ++t) {
        const Pair g = gain_of(t);
        if (t < IMP_REG) { g_reg[t] = g; f_row[t] = imp_idx[i0 + t]; }
        else *reinterpret_cast<Pair *>(g_mem + size_t(t) * MODES_PER_WAVE + 2 * lane) = g;
    }
    const uint32_t half = lane / TS, ts = lane % TS; // turn-around mapping: chunks 8*half .. 8*half+7 of sample ts
    // pickups of this wave's object: the state tiles and the staged gains (see above); none of it exists in the other entries
    __shared__ __attribute__((aligned(16))) Real s_zim[READ ? TS * PITCH : 1], s_zre[READ ? TS * PITCH : 1];
    __shared__ __attribute__((aligned(16))) Real s_pick[READ ? MH_PICKUPS_PER_OBJECT * 2 * MODES_PER_WAVE : 1]; // [pickup][im | re][mode]
    uint32_t pk0 = 0, n_pick = 0;
    if constexpr (READ) {
        pk0 = rd.pick_ptr[wd.dealt];
        n_pick = min(rd.pick_ptr[wd.dealt + 1] - pk0, uint32_t(MH_PICKUPS_PER_OBJECT));
        stage_pickup_gains(b, w, rd, pk0, n_pick, lane, s_pick);
    }
    // one sample of this lane's two resonators; their output terms go to the turn-around tile
    auto step = [&](const Pair &excite, uint32_t ds) {
        const Pair re = w.z_re * w.c_re - w.z_im * w.c_im + excite;
        w.z_im = w.z_re * w.c_im + w.z_im * w.c_re;
        w.z_re = re;
        *reinterpret_cast<Pair *>(s_term + ds * PITCH + 2 * lane) = w.p_im * w.z_im + w.p_re * re;
        if constexpr (READ)
            if (n_pick) {
                *reinterpret_cast<Pair *>(s_zim + ds * PITCH + 2 * lane) = w.z_im;
                *reinterpret_cast<Pair *>(s_zre + ds * PITCH + 2 * lane) = re;
            }
    };
    // after a tile's samples: every chunk's 8 terms added in mode order, sample ts of chunks 8*half .. 8*half+7 per lane
    auto turn_around = [&](uint32_t s0, uint32_t sn) {
        __syncthreads();
        chunk_sums<TS>(s_term, w, lane, s0, sn, partial, frames);
        if constexpr (READ) {
            if (ts < sn) read_pickups(s_zim, s_zre, s_pick, rd, pk0, n_pick, wd.first_mode, half, ts, s0, frames);
        }
        __syncthreads();
    };
    // NR = impacts held in registers (0, 1 or 2); EXTRA = the object has more than IMP_REG impacts.
    auto run = [&](auto nr_tag, auto extra_tag) {
        constexpr uint32_t NR = decltype(nr_tag)::value;
        constexpr bool EXTRA = decltype(extra_tag)::value;
        for (uint32_t s0 = 0; s0 < frames; s0 += TS) {
            const uint32_t sn = min(TS, frames - s0);
            Real f_tile[NR > 0 ? NR : 1] = {};
#pragma unroll
            for (uint32_t t = 0; t < NR; ++t)
                if (lane < sn) f_tile[t] = force[size_t(f_row[t]) * frames + s0 + lane];
            auto sample = [&](uint32_t ds) {
                Pair excite = {0, 0};
#pragma unroll
                for (uint32_t t = 0; t < NR; ++t) {
                    // a zero force sample is skipped by the reference; adding its product instead is the same bits: the product is a
                    // zero of either sign (the gains are finite), and excite -- never a negative zero, it starts at +0 -- is unchanged
                    // by one (a select here was two more vector instructions per impact and sample in an issue-bound loop)
                    const Real f = lane_bcast(f_tile[t], ds);
                    excite += f * g_reg[t];
                }
                if (EXTRA) {
                    for (uint32_t t = IMP_REG; t < n_imp; ++t) {
                        const Real f = force[size_t(imp_idx[i0 + t]) * frames + s0 + ds];
                        if (f == Real(0)) continue;
                        excite += f * *reinterpret_cast<const Pair *>(g_mem + size_t(t) * MODES_PER_WAVE + 2 * lane);
                    }
                }
                step(excite, ds);
            };
            if (sn == TS && !EXTRA) {
#pragma unroll
                for (uint32_t ds = 0; ds < TS; ++ds) sample(ds);
            } else {
                for (uint32_t ds = 0; ds < sn; ++ds) sample(ds);
            }
            turn_around(s0, sn);
        }
    };
    using T0 = std::integral_constant<uint32_t, 0>;
    using T1 = std::integral_constant<uint32_t, 1>;
    using T2 = std::integral_constant<uint32_t, 2>;
    if constexpr (MANY) {
        // R = rows whose gains are in registers (3 .. ROWS_REG); MORE = rows R .. n_imp-1 follow, their gains in LDS.
        __shared__ __attribute__((aligned(16))) Real s_force[TS * ROWS_MAX]; // [sample][row]: this tile's forces of every row
        __shared__ __attribute__((aligned(16))) Real s_gain[(ROWS_MAX - ROWS_REG) * MODES_PER_WAVE]; // [row - ROWS_REG][mode]
        auto run_rows = [&](auto r_tag, auto more_tag) {
            constexpr uint32_t R = decltype(r_tag)::value;
            constexpr bool MORE = decltype(more_tag)::value;
            Pair g[R];
#pragma unroll
            for (uint32_t t = 0; t < R; ++t) g[t] = gain_of(t);
            if (MORE) // a lane reads back only what it wrote itself: no barrier between these stores and the sample loop's reads
                for (uint32_t t = R; t < n_imp; ++t) *reinterpret_cast<Pair *>(s_gain + (t - R) * MODES_PER_WAVE + 2 * lane) = gain_of(t);
            // staging: lane = (row parity, sample); rows half, half + 2, ... of the object
            const Real *mine[ROWS_MAX / 2] = {};
#pragma unroll
            for (uint32_t j = 0; j < ROWS_MAX / 2; ++j)
                if (half + 2 * j < n_imp) mine[j] = force + size_t(imp_idx[i0 + half + 2 * j]) * frames + ts;
            for (uint32_t s0 = 0; s0 < frames; s0 += TS) {
                const uint32_t sn = min(TS, frames - s0);
#pragma unroll
                for (uint32_t j = 0; j < ROWS_MAX / 2; ++j)
                    if (half + 2 * j < n_imp) s_force[ts * ROWS_MAX + half + 2 * j] = ts < sn ? mine[j][s0] : Real(0);
                __syncthreads();
                auto sample = [&](uint32_t ds) {
                    const Real *f = s_force + ds * ROWS_MAX;
                    Pair excite = {0, 0};
                    // (zero samples are added, not skipped: the same bits, see run)
#pragma unroll
                    for (uint32_t t = 0; t < R; ++t) excite += f[t] * g[t];
                    if (MORE)
                        for (uint32_t t = R; t < n_imp; ++t) excite += f[t] * *reinterpret_cast<const Pair *>(s_gain + (t - R) * MODES_PER_WAVE + 2 * lane);
                    step(excite, ds);
                };
                if (sn == TS) {
#pragma unroll
                    for (uint32_t ds = 0; ds < TS; ++ds) sample(ds);
                } else {
                    for (uint32_t ds = 0; ds < sn; ++ds) sample(ds);
                }
                turn_around(s0, sn); // its last barrier also separates this tile's force reads from the next tile's staging
            }
        };
        if (many_rows) {
            switch (n_imp) {
            case 3: run_rows(std::integral_constant<uint32_t, 3>{}, std::false_type{}); break;
            case 4: run_rows(std::integral_constant<uint32_t, 4>{}, std::false_type{}); break;
            case 5: run_rows(std::integral_constant<uint32_t, 5>{}, std::false_type{}); break;
            case 6: run_rows(std::integral_constant<uint32_t, 6>{}, std::false_type{}); break;
            case 7: run_rows(std::integral_constant<uint32_t, 7>{}, std::false_type{}); break;
            case 8: run_rows(std::integral_constant<uint32_t, ROWS_REG>{}, std::false_type{}); break;
            default: run_rows(std::integral_constant<uint32_t, ROWS_REG>{}, std::true_type{}); break;
            }
        }
    }
    if (!many_rows) {
        if (n_imp == 0) run(T0{}, std::false_type{});
        else if (n_imp == 1) run(T1{}, std::false_type{});
        else if (n_imp == 2) run(T2{}, std::false_type{});
        else run(T2{}, std::true_type{});
    }
    store_wave(b, w, lane, chunk_energy);
}
// What every mode kernel takes, the coupled one below included (render_impl: launch_modes).  Separate parameters, not a struct: only a
// kernel's own parameter can be __restrict__, and without it the coupled kernel loses a wave of occupancy in fp32 and spills scalar
// registers in fp64 (its wave-uniform loads are no longer known to be unclobbered).
#define BANK_MODES_PARAMS                                                                                                                                  \
    BankCols<Real> b, const WaveDesc *__restrict__ waves, const uint32_t *__restrict__ deal_objects, const uint32_t *__restrict__ render_count,          \
        const uint32_t *__restrict__ chunk_base, const uint32_t *__restrict__ imp_ptr, const uint32_t *__restrict__ imp_idx,                             \
        const ImpactDev<Real> *__restrict__ impacts, const Real *__restrict__ force, const Real *__restrict__ out_gain,                                   \
        const Real *__restrict__ listener_gain, uint32_t frames, Real *__restrict__ partial, Real *__restrict__ chunk_energy,                             \
        Real *__restrict__ gain_scratch, uint32_t max_imp
#define BANK_MODES_ARGS b, waves, deal_objects, render_count, chunk_base, imp_ptr, imp_idx, impacts, force, out_gain, listener_gain, frames, partial, chunk_energy, gain_scratch, max_imp
// The launch of a block without drives, or whose objects have at most IMP_REG rows each: the turn-around tile is all its LDS.
template<typename Real> __global__ void __launch_bounds__(WAVE) k_bank_modes(BANK_MODES_PARAMS) { bank_modes<Real, false>(BANK_MODES_ARGS); }
// The launch of a block with drives in which some object has more than IMP_REG rows: the same code plus run_rows and its LDS.
template<typename Real> __global__ void __launch_bounds__(WAVE) k_bank_modes_rows(BANK_MODES_PARAMS) { bank_modes<Real, true>(BANK_MODES_ARGS); }
// The launch of a block with pickups: the same code again (both row loops) plus the state tiles, the staged pickup gains and the reads.
template<typename Real> __global__ void __launch_bounds__(WAVE) k_bank_modes_read(BANK_MODES_PARAMS, ReadArgs<Real> rd) {
    bank_modes<Real, true, true>(BANK_MODES_ARGS, rd);
}
// A pickup's row: its object's partial rows added in ascending (wave, half) order from +0, written (not added) where the host reads it.
// A pickup without rows (left out, or its object at rest) gets zeros.
struct PickupRows {
    uint32_t first_row, n_rows;
};
template<typename Real>
__global__ void __launch_bounds__(256) k_bank_read_rows(const Real *__restrict__ rows, const PickupRows *__restrict__ desc, uint32_t frames, Real *__restrict__ out_host) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= frames) return;
    const PickupRows d = desc[blockIdx.y];
    Real acc = 0;
    for (uint32_t r = 0; r < d.n_rows; ++r) acc += rows[size_t(d.first_row + r) * frames + s];
    out_host[size_t(blockIdx.y) * frames + s] = acc;
}

// Contact junctions (mh_bank_render_coupled; contract in modalhip.h).  ONE WORKGROUP PER JUNCTION, one wave per 128
// modes of each side (side a's waves first, then side b's), modes in registers two per lane as in bank_modes; the waves of a junction's
// objects are taken out of the main launch's wave list and write the same partial chunk rows and chunk energies here.  The workgroup has
// as many waves as the largest junction of the call; a wave beyond a junction's own holds no modes (zero gains, zero state), stores
// nothing to global memory and takes part in every barrier.
// Per frame: the free step -> the lane's part of d (four multiply-adds from +0: g_im*Im z~, g_re*Re z~ of its even mode, then of its odd
// mode) -> mh_wave_sum (DPP moves, never the LDS crossbar) -> one LDS slot per wave -> barrier -> every wave adds the junction's slots
// from +0 in ascending wave order and computes the same f -> Re z += a*f -> output term into the wave's turn-around tile.  C is one such
// reduction ahead of the loop.  The slots are double-buffered by frame parity (C uses the odd buffer, frame 0 the even one): a wave
// overwrites a buffer only after the barrier of the frame in between, which every wave reaches after it has read that buffer.
// Barriers: 1 + frames + 2 per tile, executed by every wave of the workgroup whatever it holds -- a function of `frames` alone.
// Force rows: the tile's excitation sums (the running sum over the object's rows from +0, uncontracted, as in bank_modes) are formed
// ahead of the tile's serial loop and parked in the turn-around tile, where each lane's output term replaces them frame by frame: the
// loads of forces and gains stay off the serial chain.
constexpr uint32_t JUNCTION_WAVES = MH_JUNCTION_MODES / MODES_PER_WAVE;
template<typename Real> struct JunctionSideDev {
    uint32_t dealt, waves;
    BlendDev<Real> at;
};
template<typename Real> struct JunctionDev {
    JunctionSideDev<Real> side[2]; // side[1].waves = 0: one-sided
    Real k;
    uint32_t flags, row, first_wave; // row: the caller's index (approach, force, compliance, status); first_wave: into the gain scratch
};
template<typename Real> struct CoupledArgs {
    const Real *defl_gain;
    const JunctionDev<Real> *junctions;
    const float *approach; // [caller's junction][frames]
    Real *force_out; // [caller's junction][frames], where the host reads it
    double *compliance_out;
    uint32_t *status_out;
};
template<typename Real> constexpr uint32_t coupled_tile() { return sizeof(Real) == 4 ? 32 : 16; } // samples per turn-around tile: 16 640 B per wave either way
template<typename Real> constexpr size_t coupled_lds(uint32_t waves) {
    return 2 * JUNCTION_WAVES * sizeof(Real) + size_t(waves) * coupled_tile<Real>() * (MODES_PER_WAVE + 2) * sizeof(Real);
}
__device__ __forceinline__ float fma_real(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_real(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float sqrt_real(float v) { return __builtin_sqrtf(v); }
__device__ __forceinline__ double sqrt_real(double v) { return __builtin_sqrt(v); }
__device__ __forceinline__ float cbrt_real(float v) { return cbrtf(v); }
__device__ __forceinline__ double cbrt_real(double v) { return cbrt(v); }
// Step 4 of a Hertz junction (modalhip.h, MH_JUNCTION_HERTZ): the root y of y + c y sqrt(y) = x by the header's expression tree -- the
// smaller of the two upper bounds x and (x / c)^(2/3), then four Newton steps, nothing contracted, no trip count that depends on data --
// and f = (K y) sqrt(y).  c = K C and c15 = 1.5 c are formed once per block.  Wave-uniform: every lane has the same x, c, K.
template<typename Real> __device__ __forceinline__ Real hertz_force(Real x, Real c, Real c15, Real k) {
    if (!(x > Real(0))) return Real(0); // open, or a NaN
    Real y = x;
    if (c > Real(0)) {
        Real g = cbrt_real(x / c);
        g = g * g;
        if (g < x) y = g;
    }
#pragma unroll
    for (int step = 0; step < 4; ++step) {
        const Real r = sqrt_real(y);
        y = y - ((y + (c * y) * r) - x) / (Real(1) + c15 * r);
    }
    return (k * y) * sqrt_real(y);
}
__device__ __forceinline__ float exp2_real(float v) { return exp2f(v); }
__device__ __forceinline__ double exp2_real(double v) { return exp2(v); }
__device__ __forceinline__ float log2_real(float v) { return log2f(v); }
__device__ __forceinline__ double log2_real(double v) { return log2(v); }
template<typename Real> __device__ __forceinline__ Real min_real(Real a, Real b) { return b < a ? b : a; }
// Step 4 of a damped junction (modalhip.h, MH_JUNCTION_DAMPED, 4d): the root y of y + c phi(y) max(1 + l (y - y_p), 0) = x by the header's
// expression trees -- the linear law's closed form; Hertz: the smallest of the upper bounds, then six Newton steps -- nothing contracted, no
// trip count that depends on data, and f = K phi(y) max(1 + l (y - y_p), 0).  c = K C, c15 = 1.5 c and cl = c l are formed once per block; on a
// frame without history the caller passes l = 0, cl = 0, yp = 0.  Wave-uniform: every lane has the same arguments.
template<typename Real> struct DampedStep {
    Real f, y; // the force, and the compression the solve left: the next frame's y_p
};
template<typename Real> __device__ __forceinline__ DampedStep<Real> damped_force(Real x, Real c, Real c15, Real cl, Real l, Real yp, Real k, bool hertz) {
    if (!(x > Real(0))) return {Real(0), x}; // open, or a NaN
    if (!(Real(1) + l * (x - yp) > Real(0))) return {Real(0), x}; // it opens faster than 1 / l per frame: the root is below the clamp's kink
    const Real m0 = Real(1) - l * yp;
    Real y;
    if (!hertz) {
        const Real b = Real(1) + c * m0;
        const Real r = sqrt_real(b * b + (Real(4) * cl) * x);
        y = min_real(x, b >= Real(0) ? (Real(2) * x) / (b + r) : (r - b) / (Real(2) * cl));
        Real m = Real(1) + l * (y - yp);
        if (!(m > Real(0))) m = Real(0);
        return {(k * y) * m, y};
    }
    const Real big = std::numeric_limits<Real>::max();
    const Real p5 = cl > Real(0) ? exp2_real(Real(0.4) * log2_real(x / cl)) : big;
    if (m0 >= Real(0)) {
        const Real cm = c * m0, t = cbrt_real(x / cm);
        const Real g = cm > Real(0) ? t * t : big;
        y = min_real(min_real(x, g), p5);
    } else {
        const Real ylo = -m0 / l;
        const Real lin = x / ((cl * ylo) * sqrt_real(ylo));
        y = min_real(x, ylo + min_real(lin, p5));
    }
#pragma unroll
    for (int step = 0; step < 6; ++step) {
        const Real r = sqrt_real(y), m = Real(1) + l * (y - yp), q = (c * y) * r;
        y = y - ((y + q * m) - x) / ((Real(1) + (c15 * r) * m) + q * l);
    }
    Real m = Real(1) + l * (y - yp);
    if (!(m > Real(0))) m = Real(0);
    return {((k * y) * sqrt_real(y)) * m, y};
}
// What the damped entry takes beyond CoupledArgs, by the caller's junction index: l in the bank's precision, the carry that came in and where
// the one that goes out is written (where the host reads it).
template<typename Real> struct DampedArgs : CoupledArgs<Real> {
    const Real *damping, *carry_in;
    Real *carry_out;
};
// Pickups on junction objects (mh_bank_render_observed; contract in modalhip.h).  A wave of a junction launch whose
// object carries a pickup is TAPPED: it streams Im z and Re z of every frame -- the state after step 5, the one the output term is formed
// from -- with two plain vector stores into `states`, [tapped wave][frame][Im z | Re z][128], zeros on padded modes.  Nothing waits for
// the stores: they are off the per-frame chain.  k_bank_observe_rows then forms the (wave, half) partial rows from them in the order
// k_bank_modes_read does.  tap: by the wave's index among the junction launches' waves (first_wave + wave); NO_TAP: not tapped.
constexpr uint32_t NO_TAP = 0xffffffffu;
constexpr uint32_t TAP_FRAME = 2 * MODES_PER_WAVE; // values a tapped wave stores per frame
template<typename Real, typename Base> struct ObservedArgs : Base {
    const uint32_t *tap;
    Real *states;
};
template<typename Real, typename Base, bool OBSERVE> using JunctionArgs = std::conditional_t<OBSERVE, ObservedArgs<Real, Base>, Base>;
// Where a tapped wave's lane stores frame 0 (its two modes of Im z; Re z is MODES_PER_WAVE further); null for a wave that is not tapped.
template<typename Real, typename Args> __device__ __forceinline__ Real *tap_of(const Args &args, bool active, uint32_t wave_index, uint32_t frames, uint32_t lane) {
    const uint32_t tap = active ? args.tap[wave_index] : NO_TAP;
    return tap != NO_TAP ? args.states + size_t(tap) * frames * TAP_FRAME + 2 * lane : nullptr;
}
template<typename Real> __device__ __forceinline__ void tap_store(Real *tap_row, uint32_t frame, const PairOf<Real> &z_im, const PairOf<Real> &z_re) {
    Real *at = tap_row + size_t(frame) * TAP_FRAME;
    *reinterpret_cast<PairOf<Real> *>(at) = z_im;
    *reinterpret_cast<PairOf<Real> *>(at + MODES_PER_WAVE) = z_re;
}
// Number checks on what a junction's block keeps; a NaN fails each of them.  (Where a kernel still spells one out, the named form changed the
// instructions of an entry that has none of the group solves in it: profiles/bank_junction_steps.txt.)
template<typename Real> __device__ __forceinline__ bool within_bound(Real v, Real bound) { return v >= -bound && v <= bound; }
template<typename Real> __device__ __forceinline__ bool is_finite(Real v) { return within_bound(v, std::numeric_limits<Real>::max()); }
template<typename Real> __device__ __forceinline__ bool finite_from_zero(Real v) { return v >= Real(0) && v <= std::numeric_limits<Real>::max(); } // finite and not below 0
template<typename Real> __device__ __forceinline__ bool finite_above_zero(Real v) { return v > Real(0) && v <= std::numeric_limits<Real>::max(); }
// The turn-around of bank_modes at the end of a junction kernel's tile: every chunk's 8 terms added in mode order.  Two barriers, taken by
// every wave of the workgroup.
template<uint32_t TS, typename Real>
__device__ __forceinline__ void junction_turn_around(const Real *s_term, const WaveLane<Real> &w, uint32_t lane, uint32_t s0, uint32_t sn, Real *partial, uint32_t frames) {
    mh_lds_writes_landed();
    __syncthreads();
    chunk_sums<TS>(s_term, w, lane, s0, sn, partial, frames);
    __syncthreads();
}
// HERTZ = false (k_bank_modes_coupled<Real>): every junction is a linear spring -- the entry of a call without a Hertz junction, instruction
// for instruction what it was before the parameter.  HERTZ = true: a junction with MH_JUNCTION_HERTZ takes hertz_force, a linear one the
// same expression as in the other entry through one workgroup-uniform branch.  DAMPED = true (with HERTZ: k_bank_modes_coupled_damped<Real>):
// a junction with MH_JUNCTION_DAMPED takes damped_force and keeps y_p in a register from frame to frame; every other junction the branch it
// takes in the Hertz entry.  The parameter type depends on DAMPED, so the other two entries are what they were.  OBSERVE = true: the entries
// of mh_bank_render_observed -- tapped waves also store their states (above); the parameter type grows by the tap list and the states' base.
template<typename Real, bool HERTZ = false, bool DAMPED = false, bool OBSERVE = false> __global__ void __launch_bounds__(JUNCTION_WAVES *WAVE) k_bank_modes_coupled(BANK_MODES_PARAMS, JunctionArgs<Real, std::conditional_t<DAMPED, DampedArgs<Real>, CoupledArgs<Real>>, OBSERVE> ca) { // (`waves`: the main launch's, not read here)
    static_assert(!DAMPED || HERTZ, "the damped entry is the Hertz entry plus the damped solve: K C and 1.5 K C are formed under HERTZ");
    typedef PairOf<Real> Pair;
    constexpr uint32_t TS = coupled_tile<Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char coupled_mem[];
    Real *s_slot = reinterpret_cast<Real *>(coupled_mem); // [2][JUNCTION_WAVES]
    const uint32_t wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    Real *s_term = s_slot + 2 * JUNCTION_WAVES + size_t(wave) * TS * PITCH; // this wave's tile, [sample][mode]
    const JunctionDev<Real> J = ca.junctions[blockIdx.x];
    const uint32_t waves_a = J.side[0].waves, n_w = waves_a + J.side[1].waves;
    const bool active = wave < n_w;
    const JunctionSideDev<Real> S = J.side[active && wave >= waves_a ? 1 : 0];
    const uint32_t first_mode = active ? (wave - (wave >= waves_a ? waves_a : 0u)) * MODES_PER_WAVE : 0u;
    // an idle wave has no live mode: nothing below loads or stores for it
    WaveLane<Real> w = load_wave(b, deal_objects, chunk_base, out_gain, listener_gain, S.dealt, first_mode, active ? render_count[S.dealt] : 0u, lane);
    Pair a = {0, 0}, g_im = {0, 0}, g_re = {0, 0}; // the junction's drive gain and its advance-1 read row
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (w.live[h]) {
            const BlendRead<Real> point = blend_read(b, w, S.at, ca.defl_gain, h);
            a[h] = b.rad_gain[w.k0 + w.k + h] * point.along;
            const ReadGains<Real> g = read_gains(point.read, w.c_re[h], w.c_im[h], 1u);
            g_im[h] = g.im;
            g_re[h] = g.re;
        }
    // the object's force rows: gains of the first IMP_REG in registers, of further ones in this wave's scratch rows (a lane reads back
    // what it wrote)
    const uint32_t i0 = imp_ptr[S.dealt], n_imp = active ? imp_ptr[S.dealt + 1] - i0 : 0u;
    Pair g_reg[IMP_REG] = {};
    Real *g_mem = gain_scratch + size_t(J.first_wave + wave) * max_imp * MODES_PER_WAVE;
    for (uint32_t t = 0; t < n_imp; ++t) {
        const Pair g = row_gain(b, w, impacts[imp_idx[i0 + t]]);
        if (t < IMP_REG) g_reg[t] = g;
        else *reinterpret_cast<Pair *>(g_mem + size_t(t) * MODES_PER_WAVE + 2 * lane) = g;
    }
    // a sum over the junction's modes: the lane's part -> the wave (DPP tree) -> the waves in ascending order from +0; the same bits in
    // every lane of every wave.  One barrier.
    auto junction_sum = [&](Real mine, uint32_t buffer) {
        const Real w = mh_wave_sum(mine);
        if (lane == 0) s_slot[buffer * JUNCTION_WAVES + wave] = w;
        mh_lds_writes_landed();
        __syncthreads();
        Real v[JUNCTION_WAVES];
#pragma unroll
        for (uint32_t i = 0; i < JUNCTION_WAVES; ++i) v[i] = s_slot[buffer * JUNCTION_WAVES + i];
        Real acc = 0;
#pragma unroll
        for (uint32_t i = 0; i < JUNCTION_WAVES; ++i) acc = i < n_w ? acc + v[i] : acc; // a slot beyond the junction's waves is not added
        return acc;
    };
    const Real zero = 0;
    const Real compliance = junction_sum(fma_real(g_re.y, a.y, fma_real(g_re.x, a.x, zero)), 1);
    const Real denom_k = Real(1) + J.k * compliance;
    bool solved = finite_above_zero(denom_k);
    bool hertz = false; // workgroup-uniform
    Real kc = 0, kc15 = 0; // Hertz: c = K C and 1.5 c, once per block
    if constexpr (HERTZ) {
        hertz = (J.flags & MH_JUNCTION_HERTZ) != 0;
        kc = J.k * compliance;
        kc15 = Real(1.5) * kc;
        const Real most = std::numeric_limits<Real>::max();
        if (hertz) solved = compliance >= Real(0) && compliance <= most && kc >= Real(0) && kc <= most; // C and K C finite and not below 0
    }
    bool damped = false; // workgroup-uniform
    Real lam = 0, kcl = 0, y_prev = 0, l_now = 0, cl_now = 0; // damped: l and c l; y_p; what this frame's solve takes of l and c l (0 without history)
    if constexpr (DAMPED) {
        damped = (J.flags & MH_JUNCTION_DAMPED) != 0;
        if (damped) {
            const Real most = std::numeric_limits<Real>::max();
            lam = ca.damping[J.row];
            kcl = kc * lam;
            solved = compliance >= Real(0) && compliance <= most && kc >= Real(0) && kc <= most && kcl >= Real(0) && kcl <= most; // C, K C and K C l finite and not below 0
            const Real came = ca.carry_in[J.row];
            if (came >= -most && came <= most) y_prev = came, l_now = lam, cl_now = kcl; // a finite carry: there is a history
        }
    }
    const Real stiffness = solved ? J.k : Real(0), denom = solved ? denom_k : Real(1);
    const bool bilateral = (J.flags & MH_JUNCTION_BILATERAL) != 0;
    if (threadIdx.x == 0) {
        ca.compliance_out[J.row] = double(compliance);
        ca.status_out[J.row] = solved ? MH_JUNCTION_SOLVED : MH_JUNCTION_REFUSED;
    }
    const float *u_row = ca.approach + size_t(J.row) * frames;
    Real *f_row = ca.force_out + size_t(J.row) * frames;
    Real *tap_row = nullptr;
    if constexpr (OBSERVE) tap_row = tap_of<Real>(ca, active, J.first_wave + wave, frames, lane);
    for (uint32_t s0 = 0; s0 < frames; s0 += TS) {
        const uint32_t sn = min(TS, frames - s0);
        // this tile's approach samples, lane = sample (not finite: 0, as a drive's)
        Real u_tile = 0;
        if (lane < sn) u_tile = finite_or_zero<Real>(u_row[s0 + lane]);
        // the tile's excitation, parked where the output terms will go
        for (uint32_t ds = 0; ds < sn; ++ds) {
            Pair excite = {0, 0};
            for (uint32_t t = 0; t < n_imp; ++t) {
                const Real f = force[size_t(imp_idx[i0 + t]) * frames + s0 + ds];
                excite += f * (t < IMP_REG ? g_reg[t] : *reinterpret_cast<const Pair *>(g_mem + size_t(t) * MODES_PER_WAVE + 2 * lane));
            }
            *reinterpret_cast<Pair *>(s_term + ds * PITCH + 2 * lane) = excite;
        }
        Real f_tile = 0;
        for (uint32_t ds = 0; ds < sn; ++ds) {
            const Pair excite = *reinterpret_cast<const Pair *>(s_term + ds * PITCH + 2 * lane); // what this lane parked
            const Pair re = w.z_re * w.c_re - w.z_im * w.c_im + excite;
            w.z_im = w.z_re * w.c_im + w.z_im * w.c_re;
            const Real mine = fma_real(g_re.y, re.y, fma_real(g_im.y, w.z_im.y, fma_real(g_re.x, re.x, fma_real(g_im.x, w.z_im.x, zero))));
            const Real d = junction_sum(mine, (s0 + ds) & 1u);
            const Real x = lane_bcast(u_tile, ds) - d;
            const Real reach = bilateral ? x : (x > Real(0) ? x : Real(0));
            Real f = solved ? (stiffness * reach) / denom : Real(0);
            if constexpr (HERTZ)
                if (hertz && !(DAMPED && damped)) f = solved ? hertz_force(x, kc, kc15, J.k) : Real(0);
            if constexpr (DAMPED)
                if (damped) {
                    const DampedStep<Real> step = damped_force(x, kc, kc15, cl_now, l_now, y_prev, J.k, hertz);
                    f = solved ? step.f : Real(0);
                    y_prev = step.y, l_now = lam, cl_now = kcl;
                }
            w.z_re = re + a * f;
            *reinterpret_cast<Pair *>(s_term + ds * PITCH + 2 * lane) = w.p_im * w.z_im + w.p_re * w.z_re;
            if constexpr (OBSERVE)
                if (tap_row) tap_store(tap_row, s0 + ds, w.z_im, w.z_re);
            if (lane == ds) f_tile = f;
        }
        if (wave == 0 && lane < sn) f_row[s0 + lane] = f_tile;
        junction_turn_around<TS>(s_term, w, lane, s0, sn, partial, frames);
    }
    if constexpr (DAMPED)
        if (damped && threadIdx.x == 0) ca.carry_out[J.row] = y_prev; // (the host hands it on only for a solved junction)
    store_wave(b, w, lane, chunk_energy);
}
// The launch of a call with a kept Hertz junction: the same kernel with the solve compiled in.  (An instantiation, not a wrapper around a
// shared body: with the body in a function of its own the linear entry keeps its resource report but not its register assignment.)
template<typename Real> constexpr auto k_bank_modes_coupled_hertz = &k_bank_modes_coupled<Real, true>;
// The launch of a call with a kept damped junction (MH_JUNCTION_DAMPED): the same kernel again, with both solves compiled in.
template<typename Real> constexpr auto k_bank_modes_coupled_damped = &k_bank_modes_coupled<Real, true, true>;
// The launches of mh_bank_render_observed when a kept junction's object carries a pickup: the three entries again, with the taps.
template<typename Real> constexpr auto k_bank_modes_coupled_observed = &k_bank_modes_coupled<Real, false, false, true>;
template<typename Real> constexpr auto k_bank_modes_coupled_hertz_observed = &k_bank_modes_coupled<Real, true, false, true>;
template<typename Real> constexpr auto k_bank_modes_coupled_damped_observed = &k_bank_modes_coupled<Real, true, true, true>;

// Friction (mh_bank_render_friction; contract in modalhip.h, step 4t).  A lone junction with MH_JUNCTION_FRICTION:
// the coupled kernel's workgroup -- one wave per 128 modes of each side, the same barriers -- with a second gain triple per lane
// (a_t, gt_im, gt_re: the side's blend along its tangent), a second sum d_t beside d_n (a second slot per wave, the same barrier), and
// step 4t in the place of step 4: the candidates S, P, M one per lane (lane & 3; the fourth repeats M and is not asked), each one scalar
// solve the bank already has, then a ballot over lanes 0 .. 2, its lowest set bit and a lane read per value.  The four compliances take
// two reductions ahead of the loop (C_nn and C_nt, then C_tn and C_tt).  Slots: [parity][n | t][wave]; the two rounds use the even and
// the odd buffer, frame 0 the even one again, as in the coupled kernel.  Barriers: 2 + frames + 2 per tile -- a function of `frames` alone.
// The anchor q sits in a register from frame to frame and is written once after the loop, with the counts, by wave 0.
// A kernel of its own from the leaf functions the coupled kernel is made of: that one's instantiations keep their resource reports
// (profiles/bank_friction_resources.txt).
template<typename Real> struct FrictionJunctionDev {
    JunctionDev<Real> j; // the normal channel, as the coupled kernel takes it
    Real t[2][3]; // the sides' tangents
    Real mu, kt;
};
template<typename Real> struct FrictionArgs {
    const Real *defl_gain;
    const FrictionJunctionDev<Real> *junctions;
    const float *approach, *travel; // [caller's junction][frames]
    Real *force_out, *tangent_out; // [caller's junction][frames], where the host reads them
    double *compliance_out;
    uint32_t *status_out;
    const Real *anchor_in; // by the caller's junction index
    Real *anchor_out;
    uint32_t *counts_out; // [caller's junction][3]: frames on S, on P or M, without a consistent candidate
};
template<typename Real> constexpr size_t friction_lds(uint32_t waves) {
    return 4 * JUNCTION_WAVES * sizeof(Real) + size_t(waves) * coupled_tile<Real>() * (MODES_PER_WAVE + 2) * sizeof(Real);
}
template<typename Real> struct FrictionSums {
    Real n, t;
};
template<typename Real, bool OBSERVE = false> __global__ void __launch_bounds__(JUNCTION_WAVES *WAVE) k_bank_modes_coupled_friction(BANK_MODES_PARAMS, JunctionArgs<Real, FrictionArgs<Real>, OBSERVE> fa) { // (`waves`: the main launch's, not read here)
    typedef PairOf<Real> Pair;
    constexpr uint32_t TS = coupled_tile<Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char friction_mem[];
    Real *s_slot = reinterpret_cast<Real *>(friction_mem); // [2][2][JUNCTION_WAVES]
    const uint32_t wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    Real *s_term = s_slot + 4 * JUNCTION_WAVES + size_t(wave) * TS * PITCH; // this wave's tile, [sample][mode]
    const FrictionJunctionDev<Real> *__restrict__ F = fa.junctions + blockIdx.x;
    const JunctionDev<Real> J = F->j;
    const uint32_t waves_a = J.side[0].waves, n_w = waves_a + J.side[1].waves;
    const bool active = wave < n_w;
    const uint32_t sd = active && wave >= waves_a ? 1 : 0;
    const JunctionSideDev<Real> S = J.side[sd];
    const uint32_t first_mode = active ? (wave - (wave >= waves_a ? waves_a : 0u)) * MODES_PER_WAVE : 0u;
    // an idle wave has no live mode: nothing below loads or stores for it
    WaveLane<Real> w = load_wave(b, deal_objects, chunk_base, out_gain, listener_gain, S.dealt, first_mode, active ? render_count[S.dealt] : 0u, lane);
    BlendDev<Real> along_t = S.at; // the side's blend with t in the place of n
    along_t.nx = F->t[sd][0], along_t.ny = F->t[sd][1], along_t.nz = F->t[sd][2];
    Pair a = {0, 0}, g_im = {0, 0}, g_re = {0, 0}, a_t = {0, 0}, gt_im = {0, 0}, gt_re = {0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (w.live[h]) {
            const BlendRead<Real> point = blend_read(b, w, S.at, fa.defl_gain, h), slide = blend_read(b, w, along_t, fa.defl_gain, h);
            a[h] = b.rad_gain[w.k0 + w.k + h] * point.along;
            a_t[h] = b.rad_gain[w.k0 + w.k + h] * slide.along;
            const ReadGains<Real> g = read_gains(point.read, w.c_re[h], w.c_im[h], 1u), gt = read_gains(slide.read, w.c_re[h], w.c_im[h], 1u);
            g_im[h] = g.im, g_re[h] = g.re;
            gt_im[h] = gt.im, gt_re[h] = gt.re;
        }
    // the object's force rows, as in the coupled kernel
    const uint32_t i0 = imp_ptr[S.dealt], n_imp = active ? imp_ptr[S.dealt + 1] - i0 : 0u;
    Pair g_reg[IMP_REG] = {};
    Real *g_mem = gain_scratch + size_t(J.first_wave + wave) * max_imp * MODES_PER_WAVE;
    for (uint32_t t = 0; t < n_imp; ++t) {
        const Pair g = row_gain(b, w, impacts[imp_idx[i0 + t]]);
        if (t < IMP_REG) g_reg[t] = g;
        else *reinterpret_cast<Pair *>(g_mem + size_t(t) * MODES_PER_WAVE + 2 * lane) = g;
    }
    // two sums over the junction's modes in one barrier, each as the coupled kernel's one: the lane's part -> the wave (DPP tree) -> the
    // waves in ascending order from +0; the same bits in every lane of every wave
    auto junction_sums = [&](Real mine_n, Real mine_t, uint32_t buffer) {
        const Real wn = mh_wave_sum(mine_n), wt = mh_wave_sum(mine_t);
        Real *slot = s_slot + buffer * 2 * JUNCTION_WAVES;
        if (lane == 0) slot[wave] = wn, slot[JUNCTION_WAVES + wave] = wt;
        mh_lds_writes_landed();
        __syncthreads();
        Real vn[JUNCTION_WAVES], vt[JUNCTION_WAVES];
#pragma unroll
        for (uint32_t i = 0; i < JUNCTION_WAVES; ++i) vn[i] = slot[i], vt[i] = slot[JUNCTION_WAVES + i];
        FrictionSums<Real> acc = {0, 0};
#pragma unroll
        for (uint32_t i = 0; i < JUNCTION_WAVES; ++i) { // a slot beyond the junction's waves is not added
            acc.n = i < n_w ? acc.n + vn[i] : acc.n;
            acc.t = i < n_w ? acc.t + vt[i] : acc.t;
        }
        return acc;
    };
    const Real zero = 0;
    // step 3: C_nn (the bits of the coupled kernel's C) and C_nt, then C_tn and C_tt
    const FrictionSums<Real> from_n = junction_sums(fma_real(g_re.y, a.y, fma_real(g_re.x, a.x, zero)), fma_real(g_re.y, a_t.y, fma_real(g_re.x, a_t.x, zero)), 0);
    const FrictionSums<Real> from_t = junction_sums(fma_real(gt_re.y, a.y, fma_real(gt_re.x, a.x, zero)), fma_real(gt_re.y, a_t.y, fma_real(gt_re.x, a_t.x, zero)), 1);
    const Real c_nn = from_n.n, c_nt = from_n.t, c_tn = from_t.n, c_tt = from_t.t;
    const Real mu = F->mu, kt = F->kt;
    const bool hertz = (J.flags & MH_JUNCTION_HERTZ) != 0; // workgroup-uniform
    // once per block: the stick elimination's den and beta, and the compliance each candidate's scalar solve sees
    const Real den = Real(1) + kt * c_tt, beta = (kt * c_tn) / den;
    const Real c_stick = c_nn - c_nt * beta, c_plus = c_nn + mu * c_nt, c_minus = c_nn - mu * c_nt;
    const Real kc_nn = J.k * c_nn, kc_stick = J.k * c_stick, kc_plus = J.k * c_plus, kc_minus = J.k * c_minus;
    bool solved = hertz ? finite_from_zero(c_nn) && finite_from_zero(kc_nn) : finite_above_zero(Real(1) + kc_nn); // the normal law's own conditions
    solved = solved && is_finite(c_tt) && is_finite(c_nt) && is_finite(c_tn) && c_tt >= Real(0) && finite_above_zero(den) && finite_from_zero(c_plus) && finite_from_zero(c_minus) &&
             is_finite(kc_stick) && is_finite(kc_plus) && is_finite(kc_minus);
    // this lane's candidate: 0 = S, 1 = P, 2 = M (lane 3 of a quad repeats M)
    const uint32_t cand = min(lane & 3u, 2u);
    const Real kc = cand == 0 ? kc_stick : cand == 1 ? kc_plus : kc_minus, kc15 = Real(1.5) * kc, denom = Real(1) + kc;
    if (threadIdx.x == 0) {
        fa.compliance_out[J.row] = double(c_nn);
        fa.status_out[J.row] = solved ? MH_JUNCTION_SOLVED : MH_JUNCTION_REFUSED;
    }
    Real q = fa.anchor_in[J.row]; // not finite: no history
    uint32_t n_stick = 0, n_slip = 0, n_none = 0;
    const float *u_row = fa.approach + size_t(J.row) * frames, *w_row = fa.travel + size_t(J.row) * frames;
    Real *f_row = fa.force_out + size_t(J.row) * frames, *ft_row = fa.tangent_out + size_t(J.row) * frames;
    Real *tap_row = nullptr;
    if constexpr (OBSERVE) tap_row = tap_of<Real>(fa, active, J.first_wave + wave, frames, lane);
    for (uint32_t s0 = 0; s0 < frames; s0 += TS) {
        const uint32_t sn = min(TS, frames - s0);
        // this tile's approach and travel samples, lane = sample (not finite: 0, as a drive's)
        Real u_tile = 0, w_tile = 0;
        if (lane < sn) u_tile = finite_or_zero<Real>(u_row[s0 + lane]), w_tile = finite_or_zero<Real>(w_row[s0 + lane]);
        // the tile's excitation, parked where the output terms will go
        for (uint32_t ds = 0; ds < sn; ++ds) {
            Pair excite = {0, 0};
            for (uint32_t t = 0; t < n_imp; ++t) {
                const Real f = force[size_t(imp_idx[i0 + t]) * frames + s0 + ds];
                excite += f * (t < IMP_REG ? g_reg[t] : *reinterpret_cast<const Pair *>(g_mem + size_t(t) * MODES_PER_WAVE + 2 * lane));
            }
            *reinterpret_cast<Pair *>(s_term + ds * PITCH + 2 * lane) = excite;
        }
        Real f_tile = 0, ft_tile = 0;
        for (uint32_t ds = 0; ds < sn; ++ds) {
            const Pair excite = *reinterpret_cast<const Pair *>(s_term + ds * PITCH + 2 * lane); // what this lane parked
            const Pair re = w.z_re * w.c_re - w.z_im * w.c_im + excite;
            w.z_im = w.z_re * w.c_im + w.z_im * w.c_re;
            const Real mine_n = fma_real(g_re.y, re.y, fma_real(g_im.y, w.z_im.y, fma_real(g_re.x, re.x, fma_real(g_im.x, w.z_im.x, zero))));
            const Real mine_t = fma_real(gt_re.y, re.y, fma_real(gt_im.y, w.z_im.y, fma_real(gt_re.x, re.x, fma_real(gt_im.x, w.z_im.x, zero))));
            const FrictionSums<Real> d = junction_sums(mine_n, mine_t, (s0 + ds) & 1u);
            const Real x_n = lane_bcast(u_tile, ds) - d.n, x_t = lane_bcast(w_tile, ds) - d.t;
            if (!is_finite(q)) q = x_t; // no history: the slider stands where the contact is
            Real f_n = 0, f_t = 0;
            if (!(x_n > Real(0))) { // branch O: open, or a NaN -- no shear, and the slider follows
                q = x_t;
            } else {
                // step 4t: this lane's candidate
                const Real alpha = (kt * (x_t - q)) / den;
                const Real x_c = cand == 0 ? x_n - c_nt * alpha : x_n;
                Real fn_c;
                if (hertz) fn_c = hertz_force(x_c, kc, kc15, J.k);
                else fn_c = (J.k * (x_c > Real(0) ? x_c : Real(0))) / denom;
                const Real cone = mu * fn_c;
                const Real ft_c = cand == 0 ? alpha - beta * fn_c : cand == 1 ? cone : -cone;
                const Real e = (x_t - c_tn * fn_c) - c_tt * ft_c;
                const Real q_c = cand == 0 ? q : e - ft_c / kt;
                const bool consistent = cand == 0 ? __builtin_fabs(ft_c) <= cone : cand == 1 ? q_c >= q : q_c <= q;
                const Real miss = cand == 0 ? __builtin_fabs(ft_c) - cone : cand == 1 ? kt * (q - q_c) : kt * (q_c - q);
                const uint32_t found = uint32_t(__builtin_amdgcn_ballot_w64(consistent)) & 7u; // lanes 0 .. 2
                uint32_t taken;
                if (found) {
                    taken = uint32_t(__builtin_ctz(found));
                } else { // rounding on a boundary left none: the one that misses by least, the earlier one on a tie
                    const Real m0 = lane_bcast(miss, 0u), m1 = lane_bcast(miss, 1u), m2 = lane_bcast(miss, 2u);
                    taken = m1 < m0 ? 1u : 0u;
                    if (m2 < (taken ? m1 : m0)) taken = 2u;
                    ++n_none;
                }
                taken = __builtin_amdgcn_readfirstlane(taken);
                if (taken == 0) ++n_stick;
                else ++n_slip;
                f_n = solved ? lane_bcast(fn_c, taken) : zero;
                f_t = solved ? lane_bcast(ft_c, taken) : zero;
                q = lane_bcast(q_c, taken);
            }
            w.z_re = re + (a * f_n + a_t * f_t);
            *reinterpret_cast<Pair *>(s_term + ds * PITCH + 2 * lane) = w.p_im * w.z_im + w.p_re * w.z_re;
            if constexpr (OBSERVE)
                if (tap_row) tap_store(tap_row, s0 + ds, w.z_im, w.z_re);
            if (lane == ds) f_tile = f_n, ft_tile = f_t;
        }
        if (wave == 0 && lane < sn) f_row[s0 + lane] = f_tile, ft_row[s0 + lane] = ft_tile;
        junction_turn_around<TS>(s_term, w, lane, s0, sn, partial, frames);
    }
    if (threadIdx.x == 0) { // (the host hands the anchor and the counts on only for a solved junction)
        fa.anchor_out[J.row] = q;
        fa.counts_out[3 * J.row] = n_stick, fa.counts_out[3 * J.row + 1] = n_slip, fa.counts_out[3 * J.row + 2] = n_none;
    }
    store_wave(b, w, lane, chunk_energy);
}
template<typename Real> constexpr auto k_bank_modes_coupled_friction_observed = &k_bank_modes_coupled_friction<Real, true>;

// Groups of junctions that share objects (MH_JUNCTION_SHARED; contract in modalhip.h).  ONE WORKGROUP PER GROUP, one
// wave per 128 modes of each DISTINCT object of the group (the objects in the order the members name them, side a before side b), modes
// in registers two per lane; a wave holds one gain triple (a, g_im, g_re) per member that has a side on its object -- up to
// MH_JUNCTION_GROUP -- and zeros for the others.  The launch has as many waves as the largest group of the call; a wave beyond a group's
// own holds no modes and takes part in every barrier.
// Per frame: the free step -> per member on the wave's object the lane's part of d_i (the four multiply-adds of the coupled kernel) ->
// mh_wave_sum -> one LDS slot per (member, place of the wave in that member's order: side a's waves, then side b's) -> barrier -> every
// wave adds each member's slots from +0 in that order, forms x and runs the group's solve: lane m (and every lane with m = lane % 16)
// holds the inverse M_A of the subset A with bit mask m, formed once per block, and computes A's candidate and whether it is consistent;
// a ballot over lanes 0 .. 15, its lowest set bit and one lane read per member give every lane of every wave the same f.  Then
// Re z += a_i f_i for the members on the wave's object in ascending order, and the output term goes to the wave's turn-around tile.
// The matrix C takes MH_JUNCTION_GROUP such reductions ahead of the loop (column j in round j).  The slots are double-buffered by parity
// (round j: buffer j % 2; frame s: buffer s % 2 -- the last round uses the odd buffer, frame 0 the even one) as in the coupled kernel.
// Barriers: 1 + MH_JUNCTION_GROUP + frames + 2 per tile, executed by every wave whatever it holds -- a function of `frames` alone.
constexpr uint32_t GROUP = MH_JUNCTION_GROUP, GROUP_SETS = 1u << GROUP, NO_SLOT = 0xffffffffu;
template<typename Real> struct GroupMemberDev {
    BlendDev<Real> at[2];
    Real k;
    uint32_t flags, row, slot[2]; // row: the caller's index; slot: the side's object among the group's, NO_SLOT for an exciter
};
template<typename Real> struct GroupDev {
    GroupMemberDev<Real> member[GROUP]; // in call order
    uint32_t n, n_objects, first_wave, n_waves; // first_wave: into the gain scratch
    uint32_t dealt[JUNCTION_WAVES], wave0[JUNCTION_WAVES], waves[JUNCTION_WAVES]; // per distinct object: the dealt object, its first wave in the workgroup, its waves
};
template<typename Real> struct GroupedArgs {
    const Real *defl_gain;
    const GroupDev<Real> *groups;
    const float *approach; // [caller's junction][frames]
    Real *force_out; // [caller's junction][frames], where the host reads it
    double *compliance_out;
    uint32_t *status_out;
};
template<typename Real> constexpr size_t grouped_lds(uint32_t waves) {
    return 2 * GROUP * JUNCTION_WAVES * sizeof(Real) + size_t(waves) * coupled_tile<Real>() * (MODES_PER_WAVE + 2) * sizeof(Real);
}
// A group with a Hertz member (mh_bank_render_mixed; contract in modalhip.h, step 4m).  What its entries take beyond
// GroupedArgs: where a member's count of frames that failed the residual test goes (where the host reads it), by the caller's index.
template<typename Real> struct MixedArgs : GroupedArgs<Real> {
    uint32_t *unconverged_out;
};
constexpr int MIXED_SWEEPS = 1, MIXED_STEPS = 10, MIXED_REFINED = 1; // step 4m's Gauss-Seidel sweeps, its Newton steps, and those of them that start from a residual in twice the precision
// A group with a damped member (mh_bank_render_damped_groups; contract in modalhip.h, step 4g).  What its entries take
// beyond MixedArgs, by the caller's junction index: l in the bank's precision, the carry that came in and where the one that goes out is
// written (where the host reads it).
template<typename Real> struct DampedGroupArgs : MixedArgs<Real> {
    const Real *damping, *carry_in;
    Real *carry_out;
};
constexpr int DAMPED_SWEEPS = 1, DAMPED_STEPS = 8, DAMPED_REFINED = 2; // step 4g's counts, as step 4m's
// a + b and a b as the rounded result and its rounding error, both exact (Knuth's six operations; one fused multiply-add).
template<typename Real> __device__ __forceinline__ Real two_sum(Real a, Real b, Real &err) {
    const Real s = a + b, bb = s - a;
    err = (a - (s - bb)) + (b - bb);
    return s;
}
template<typename Real> __device__ __forceinline__ Real two_product(Real a, Real b, Real &err) {
    const Real p = a * b;
    err = fma_real(a, b, -p);
    return p;
}
// Step 4m, a member alone: the root y of y + c phi(y) = x.  Hertz: step 4h's tree (hertz_force's) up to y; linear: x / (1 + c), for x > 0
// only unless bilateral; an open member keeps y = x.  c15 = 1.5 c.
template<typename Real> __device__ __forceinline__ Real mixed_alone(Real x, Real c, Real c15, bool hertz, bool bilateral) {
    if (hertz) {
        if (!(x > Real(0))) return x;
        Real y = x;
        if (c > Real(0)) {
            Real g = cbrt_real(x / c);
            g = g * g;
            if (g < x) y = g;
        }
#pragma unroll
        for (int step = 0; step < 4; ++step) {
            const Real r = sqrt_real(y);
            y = y - ((y + (c * y) * r) - x) / (Real(1) + c15 * r);
        }
        return y;
    }
    return bilateral || x > Real(0) ? x / (Real(1) + c) : x;
}
// Step 4g, a damped member alone: the root y of y + c phi(y) max(1 + l (y - y_p), 0) = x by step 4d's trees -- damped_force's up to y, the
// force left to the caller, so that nothing of it lives across the group's Newton loop.  cl = c l.
template<typename Real> __device__ __forceinline__ Real damped_root(Real x, Real c, Real c15, Real cl, Real l, Real yp, bool hertz) {
    if (!(x > Real(0))) return x; // open, or a NaN
    if (!(Real(1) + l * (x - yp) > Real(0))) return x; // below the clamp's kink
    const Real m0 = Real(1) - l * yp;
    if (!hertz) {
        const Real b = Real(1) + c * m0;
        const Real r = sqrt_real(b * b + (Real(4) * cl) * x);
        return min_real(x, b >= Real(0) ? (Real(2) * x) / (b + r) : (r - b) / (Real(2) * cl));
    }
    const Real big = std::numeric_limits<Real>::max();
    const Real p5 = cl > Real(0) ? exp2_real(Real(0.4) * log2_real(x / cl)) : big;
    Real y;
    if (m0 >= Real(0)) {
        const Real cm = c * m0, t = cbrt_real(x / cm);
        const Real g = cm > Real(0) ? t * t : big;
        y = min_real(min_real(x, g), p5);
    } else {
        const Real ylo = -m0 / l;
        const Real lin = x / ((cl * ylo) * sqrt_real(ylo));
        y = min_real(x, ylo + min_real(lin, p5));
    }
#pragma unroll
    for (int step = 0; step < 6; ++step) {
        const Real r = sqrt_real(y), m = Real(1) + l * (y - yp), q = (c * y) * r;
        y = y - ((y + q * m) - x) / ((Real(1) + (c15 * r) * m) + q * l);
    }
    return y;
}
// Step 4m, the laws: phi(y) and phi'(y) of a member.
template<typename Real> __device__ __forceinline__ void mixed_law(Real y, bool hertz, bool bilateral, Real &phi, Real &dphi) {
    const Real pos = y > Real(0) ? y : Real(0);
    if (hertz) {
        const Real r = sqrt_real(pos);
        phi = pos * r;
        dphi = Real(1.5) * r;
    } else {
        phi = bilateral ? y : pos;
        dphi = bilateral || y > Real(0) ? Real(1) : Real(0);
    }
}
// A value that is the same bits in every lane, handed to the compiler as such (it then lives in scalar registers): what a group's block
// keeps for step 4g -- C, K, C_jj K_j, l -- is wave-uniform, and so are x and y_p of every frame.
__device__ __forceinline__ float wave_uniform(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ double wave_uniform(double v) {
    const uint64_t bits = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(bits)), hi = __builtin_amdgcn_readfirstlane(uint32_t(bits >> 32));
    return __builtin_bit_cast(double, uint64_t(hi) << 32 | lo);
}
// What steps 4m and 4g share of a group's Newton iteration, one definition each.  c: the matrix C; y, f, kd: the iterate, its forces and
// df / dy; x: the frame's reaches.
// F_i = (y_i + sum_j C_ij f_j) - x_i; twice: the sum carried in twice the working precision.  UNIFORM: step 4g's placement -- F goes through
// wave_uniform (the iterate lives in scalar registers between the steps); step 4m leaves it where the compiler puts it.
template<bool UNIFORM, typename Real>
__device__ __forceinline__ void group_residual(const Real (&c)[GROUP][GROUP], const Real (&y)[GROUP], const Real (&f)[GROUP], const Real (&x)[GROUP], bool twice, Real (&F)[GROUP]) {
#pragma unroll
    for (uint32_t i = 0; i < GROUP; ++i) {
        Real Fi;
        if (!twice) {
            Real acc = 0;
#pragma unroll
            for (uint32_t j = 0; j < GROUP; ++j) acc = acc + c[i][j] * f[j];
            Fi = (y[i] + acc) - x[i];
        } else {
            Real sum = y[i], low = 0, r, e;
#pragma unroll
            for (uint32_t j = 0; j < GROUP; ++j) {
                const Real p = two_product(c[i][j], f[j], e);
                sum = two_sum(sum, p, r);
                low = low + (r + e);
            }
            sum = two_sum(sum, -x[i], r);
            low = low + r;
            Fi = sum + low;
        }
        if constexpr (UNIFORM) F[i] = wave_uniform(Fi);
        else F[i] = Fi;
    }
}
// The Newton direction d of J d = F, J = I + C diag(kd): J eliminated without pivoting in ascending order, back substitution in descending order.
template<typename Real> __device__ __forceinline__ void newton_direction(const Real (&c)[GROUP][GROUP], const Real (&kd)[GROUP], const Real (&F)[GROUP], Real (&d)[GROUP]) {
    Real Jm[GROUP][GROUP], r[GROUP];
#pragma unroll
    for (uint32_t i = 0; i < GROUP; ++i) {
#pragma unroll
        for (uint32_t j = 0; j < GROUP; ++j) Jm[i][j] = i == j ? Real(1) + c[i][j] * kd[j] : c[i][j] * kd[j];
        r[i] = F[i];
    }
#pragma unroll
    for (uint32_t p = 0; p < GROUP; ++p) {
        const Real inv = Real(1) / Jm[p][p];
#pragma unroll
        for (uint32_t j = p + 1; j < GROUP; ++j) Jm[p][j] = Jm[p][j] * inv;
        r[p] = r[p] * inv;
#pragma unroll
        for (uint32_t i = p + 1; i < GROUP; ++i) {
            const Real t = Jm[i][p];
#pragma unroll
            for (uint32_t j = p + 1; j < GROUP; ++j) Jm[i][j] = Jm[i][j] - t * Jm[p][j];
            r[i] = r[i] - t * r[p];
        }
    }
#pragma unroll
    for (int p = int(GROUP) - 1; p >= 0; --p) {
        Real acc = r[p];
#pragma unroll
        for (int j = p + 1; j < int(GROUP); ++j) acc = acc - Jm[p][j] * d[j];
        d[p] = acc;
    }
}
// The residual test: |F_i| against `units` u (|y_i| + sum_j |C_ij| size_j + |x_i|), size_j the magnitude member j's force is formed from.
template<typename Real>
__device__ __forceinline__ bool residual_met(const Real (&c)[GROUP][GROUP], const Real (&y)[GROUP], const Real (&size)[GROUP], const Real (&x)[GROUP], const Real (&F)[GROUP], Real units) {
    bool met = true;
#pragma unroll
    for (uint32_t i = 0; i < GROUP; ++i) {
        Real acc = 0;
#pragma unroll
        for (uint32_t j = 0; j < GROUP; ++j) acc = acc + __builtin_fabs(c[i][j]) * size[j];
        const Real mag = (__builtin_fabs(y[i]) + acc) + __builtin_fabs(x[i]);
        met = met && __builtin_fabs(F[i]) <= (units * (std::numeric_limits<Real>::epsilon() * Real(0.5))) * mag;
    }
    return met;
}
// Step 4g (modalhip.h, mh_bank_render_damped_groups): what a group with a damped member keeps for the block, all of it wave-uniform.
template<typename Real> struct DampedGroup {
    Real c[GROUP][GROUP], k[GROUP], ck[GROUP], ck15[GROUP], lam[GROUP]; // C, K, ck_jj = C_jj K_j, 1.5 ck_jj, l (0 on a member that is not damped)
    uint32_t hertz, bilateral, damped; // bit masks over the members
};
// Step 4g of one frame: step 4m's tree -- each member alone, DAMPED_SWEEPS Gauss-Seidel sweeps, DAMPED_STEPS Newton steps, the last
// DAMPED_REFINED from a residual in twice the precision, the residual test -- with the damped law on the damped members.  known: the
// damped members with a history (the others take l = 0, y_p = 0); y_prev: y_p in, the compression this frame's solve left out.  Returns
// whether the residual test is met; f: the forces of the last y.  The same bits in every lane.
template<typename Real> __device__ __forceinline__ bool damped_group_solve(const DampedGroup<Real> &g, const Real (&x)[GROUP], uint32_t known, Real (&y_prev)[GROUP], Real (&f)[GROUP]) {
    const Real zero = 0;
    Real y[GROUP], kd[GROUP], F[GROUP], l_now[GROUP]; // kd: df / dy; l_now: what this frame's solve takes of l
#pragma unroll
    for (uint32_t j = 0; j < GROUP; ++j) l_now[j] = (known >> j & 1u) ? g.lam[j] : zero;
    auto law = [&](uint32_t j) {
        Real phi, dphi;
        mixed_law(y[j], g.hertz >> j & 1u, g.bilateral >> j & 1u, phi, dphi);
        f[j] = g.k[j] * phi;
        kd[j] = g.k[j] * dphi;
        if (g.damped >> j & 1u) { // f = (K phi) m, f' = (K phi') m + (K phi) l for m = 1 + l (y - y_p) > 0; else +0 and 0
            const Real m = Real(1) + l_now[j] * (y[j] - y_prev[j]), kp = f[j];
            const bool closed = m > Real(0);
            kd[j] = closed ? kd[j] * m + kp * l_now[j] : zero;
            f[j] = closed ? kp * m : zero;
        }
        f[j] = wave_uniform(f[j]), kd[j] = wave_uniform(kd[j]); // (the iterate lives in scalar registers between the steps: the wave's gains keep their vector registers)
    };
    auto alone = [&](uint32_t j, Real xs) {
        if (g.damped >> j & 1u) return damped_root(xs, g.ck[j], g.ck15[j], g.ck[j] * l_now[j], l_now[j], y_prev[j], (g.hertz >> j & 1u) != 0);
        return mixed_alone(xs, g.ck[j], g.ck15[j], g.hertz >> j & 1u, g.bilateral >> j & 1u);
    };
#pragma unroll
    for (uint32_t j = 0; j < GROUP; ++j) y[j] = zero, f[j] = zero, kd[j] = zero;
    // pass -1 is the start, each member alone at x_j; the sweeps follow in the same loop, so that the members' trees are compiled once
#pragma unroll 1
    for (int sweep = -1; sweep < DAMPED_SWEEPS; ++sweep) {
#pragma unroll
        for (uint32_t j = 0; j < GROUP; ++j) {
            Real acc = 0;
#pragma unroll
            for (uint32_t i = 0; i < GROUP; ++i)
                if (i != j) acc = acc + g.c[j][i] * f[i];
            y[j] = wave_uniform(alone(j, wave_uniform(sweep < 0 ? x[j] : x[j] - acc)));
            law(j);
            __builtin_amdgcn_sched_barrier(0); // one member's tree at a time: their temporaries are not to be live side by side
        }
    }
    group_residual<true>(g.c, y, f, x, DAMPED_STEPS <= DAMPED_REFINED, F);
#pragma unroll 1
    for (int step = 0; step < DAMPED_STEPS; ++step) {
        Real d[GROUP];
        newton_direction(g.c, kd, F, d);
        // a unilateral member that was open or clamped (kd = 0), or whose step more than doubles y, takes its own tree at its row's
        // linearised right-hand side instead: from below the root Newton's iteration on a convex law lands far above it and creeps
        // back.  Not in the refined steps.
#pragma unroll
        for (uint32_t j = 0; j < GROUP; ++j) {
            Real moved = y[j] - d[j];
            if (step < DAMPED_STEPS - DAMPED_REFINED && !(g.bilateral >> j & 1u) && (kd[j] == zero || moved > Real(2) * y[j]))
                moved = alone(j, wave_uniform(moved + g.c[j][j] * (f[j] + kd[j] * (moved - y[j]))));
            y[j] = wave_uniform(moved);
            law(j);
            __builtin_amdgcn_sched_barrier(0);
        }
        group_residual<true>(g.c, y, f, x, step + 1 >= DAMPED_STEPS - DAMPED_REFINED, F);
    }
    // the residual test: |F_i| against 32 u (|y_i| + sum_j |C_ij| s_j + |x_i|), s_j = K phi(y) (1 + l (|y| + |y_p|)) on a damped member, |f_j| on every other
    Real size[GROUP];
#pragma unroll
    for (uint32_t j = 0; j < GROUP; ++j) {
        size[j] = __builtin_fabs(f[j]);
        if (g.damped >> j & 1u) {
            Real phi, dphi;
            mixed_law(y[j], g.hertz >> j & 1u, false, phi, dphi);
            size[j] = (g.k[j] * phi) * (Real(1) + l_now[j] * (__builtin_fabs(y[j]) + __builtin_fabs(y_prev[j])));
        }
    }
    const bool met = residual_met(g.c, y, size, x, F, Real(32));
#pragma unroll
    for (uint32_t j = 0; j < GROUP; ++j)
        if (g.damped >> j & 1u) y_prev[j] = wave_uniform(y[j]);
    return met;
}
// OBSERVE = true (k_bank_modes_grouped_observed<Real>): the entry of mh_bank_render_observed, with the taps of the coupled kernel's.
// MIXED = true (k_bank_modes_grouped_mixed<Real>, ..._mixed_observed<Real>): the entries of mh_bank_render_mixed for the groups with a Hertz
// member -- step 4 is step 4m, the same solve in every lane of every wave (its inputs are the same bits everywhere), no subset per lane,
// no ballot; what the block keeps is C in registers, J is rebuilt from it every Newton step.  The parameter type depends on
// MIXED, and the enumeration's matrix W is not formed: the other entries are what they were.
// DAMPED = true, with MIXED (k_bank_modes_grouped_damped<Real>, ..._damped_observed<Real>): the entries of mh_bank_render_damped_groups for
// the groups with a damped member -- step 4 is step 4g: step 4m's tree with the damped law on the damped members, y_p per member in
// registers from frame to frame, the carries written once after the loop.  No barrier, LDS slot or global access per frame beyond step 4m's.
template<typename Real, bool OBSERVE = false, bool MIXED = false, bool DAMPED = false> __global__ void __launch_bounds__(JUNCTION_WAVES *WAVE) k_bank_modes_grouped(BANK_MODES_PARAMS, JunctionArgs<Real, std::conditional_t<DAMPED, DampedGroupArgs<Real>, std::conditional_t<MIXED, MixedArgs<Real>, GroupedArgs<Real>>>, OBSERVE> ga) { // (`waves`: the main launch's, not read here)
    static_assert(!DAMPED || MIXED, "the damped entry is the mixed entry plus the damped law");
    typedef PairOf<Real> Pair;
    constexpr uint32_t TS = coupled_tile<Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char grouped_mem[];
    Real *s_slot = reinterpret_cast<Real *>(grouped_mem); // [2][GROUP][JUNCTION_WAVES]
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x % WAVE, block_waves = blockDim.x / WAVE;
    Real *s_term = s_slot + 2 * GROUP * JUNCTION_WAVES + size_t(wave) * TS * PITCH; // this wave's tile, [sample][mode]
    const GroupDev<Real> *__restrict__ G = ga.groups + blockIdx.x;
    const uint32_t n = G->n;
    // this wave's object among the group's; an idle wave has no live mode: nothing below loads or stores for it
    const bool active = wave < G->n_waves;
    uint32_t slot = 0;
    for (uint32_t o = 1; o < G->n_objects; ++o)
        if (active && wave >= G->wave0[o]) slot = o; // (wave0 ascends with the object)
    const uint32_t wave_in_object = active ? wave - G->wave0[slot] : 0u, dealt = G->dealt[slot];
    WaveLane<Real> w = load_wave(b, deal_objects, chunk_base, out_gain, listener_gain, dealt, wave_in_object * MODES_PER_WAVE, active ? render_count[dealt] : 0u, lane);
    // per member: is a side of it on this wave's object, the wave's place in the member's summation order, its gains here
    uint32_t on = 0, place[GROUP] = {}, bilateral = 0, hertz = 0;
    Pair a[GROUP] = {}, g_im[GROUP] = {}, g_re[GROUP] = {};
    Real k[GROUP] = {};
    uint32_t damped = 0, known = 0; // step 4g: the damped members, and those of them with a history
    Real lam[GROUP] = {}, y_prev[GROUP] = {}; // their l and y_p (0 without history)
#pragma unroll
    for (uint32_t i = 0; i < GROUP; ++i) {
        if (i >= n) continue;
        const GroupMemberDev<Real> *M = G->member + i;
        const uint32_t sa = M->slot[0], sb = M->slot[1], waves_a = G->waves[sa];
        k[i] = M->k;
        if constexpr (DAMPED) k[i] = wave_uniform(k[i]);
        if (M->flags & MH_JUNCTION_BILATERAL) bilateral |= 1u << i;
        if constexpr (MIXED)
            if (M->flags & MH_JUNCTION_HERTZ) hertz |= 1u << i;
        if constexpr (DAMPED)
            if (M->flags & MH_JUNCTION_DAMPED) {
                damped |= 1u << i;
                lam[i] = wave_uniform(ga.damping[M->row]);
                const Real came = wave_uniform(ga.carry_in[M->row]);
                if (is_finite(came)) y_prev[i] = came, known |= 1u << i; // a finite carry: there is a history
            }
        if (!active || (sa != slot && sb != slot)) continue;
        const uint32_t sd = sa == slot ? 0u : 1u;
        on |= 1u << i;
        place[i] = (sd ? waves_a : 0u) + wave_in_object;
        const BlendDev<Real> at = M->at[sd];
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (w.live[h]) {
                const BlendRead<Real> point = blend_read(b, w, at, ga.defl_gain, h);
                a[i][h] = b.rad_gain[w.k0 + w.k + h] * point.along;
                const ReadGains<Real> g = read_gains(point.read, w.c_re[h], w.c_im[h], 1u);
                g_im[i][h] = g.im;
                g_re[i][h] = g.re;
            }
    }
    on = __builtin_amdgcn_readfirstlane(on);
    // the object's force rows, as in the coupled kernel
    const uint32_t i0 = imp_ptr[dealt], n_imp = active ? imp_ptr[dealt + 1] - i0 : 0u;
    constexpr uint32_t REG_ROWS = DAMPED ? 0u : IMP_REG; // (step 4g's entries keep every row's gains in the scratch rows: the registers go to the members' gains)
    Pair g_reg[IMP_REG] = {};
    Real *g_mem = gain_scratch + size_t(G->first_wave + wave) * max_imp * MODES_PER_WAVE;
    for (uint32_t t = 0; t < n_imp; ++t) {
        const Pair g = row_gain(b, w, impacts[imp_idx[i0 + t]]);
        if (t < REG_ROWS) g_reg[t] = g;
        else *reinterpret_cast<Pair *>(g_mem + size_t(t) * MODES_PER_WAVE + 2 * lane) = g;
    }
    // one sum per member over that member's modes: the lane's part -> the wave (DPP tree) -> the member's waves in its order from +0; the
    // same bits in every lane of every wave.  One barrier.
    auto member_sums = [&](const Real (&mine)[GROUP], uint32_t buffer, Real (&sum)[GROUP]) {
#pragma unroll
        for (uint32_t i = 0; i < GROUP; ++i)
            if (on >> i & 1u) {
                const Real ws = mh_wave_sum(mine[i]);
                if (lane == 0) s_slot[(buffer * GROUP + i) * JUNCTION_WAVES + place[i]] = ws;
            }
        mh_lds_writes_landed();
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < GROUP; ++i) {
            Real v[JUNCTION_WAVES];
#pragma unroll
            for (uint32_t p = 0; p < JUNCTION_WAVES; ++p) v[p] = s_slot[(buffer * GROUP + i) * JUNCTION_WAVES + p];
            Real acc = 0;
#pragma unroll
            for (uint32_t p = 0; p < JUNCTION_WAVES; ++p) acc = acc + v[p]; // a slot beyond the member's waves holds the +0 it was given: the same bits as not adding it
            sum[i] = acc;
        }
    };
    const Real zero = 0, most = std::numeric_limits<Real>::max();
    // every slot starts as +0; the ones beyond a member's waves stay that way (acc, begun at +0, is never -0: acc + (+0) is acc)
    if (threadIdx.x < 2 * GROUP * JUNCTION_WAVES) s_slot[threadIdx.x] = zero;
    mh_lds_writes_landed();
    __syncthreads();
    // step 3: C[i][j], column j in round j; an object that is not on a side of both contributes +0.
    // Step 4, per block: lane m holds the subset A with mask m = lane % 16.  What it keeps for the block is one matrix W: row i of
    // M_A = (I + C_AA diag(K_A))^-1 (its columns in A) for a member of A, row i of C for one outside it -- built column by column as C
    // arrives, then eliminated in place over the rows and columns of A, without pivoting, in ascending order: column p, once eliminated,
    // receives column p of the inverse, which is the unit column until then, so the operations and their operands are those of the
    // elimination of [B | I].
    const uint32_t mask = lane % GROUP_SETS, full = (1u << n) - 1u;
    const bool admissible = lane < GROUP_SETS && mask <= full && (mask & bilateral) == bilateral;
    bool numbers_ok = true; // workgroup-uniform: every C_ij and C_ij K_j of the group is finite
    Real W[GROUP][GROUP], c_own[GROUP];
#pragma unroll
    for (uint32_t j = 0; j < GROUP; ++j) {
        Real mine[GROUP], col[GROUP];
#pragma unroll
        for (uint32_t i = 0; i < GROUP; ++i) mine[i] = (on >> j & 1u) ? fma_real(g_re[i].y, a[j].y, fma_real(g_re[i].x, a[j].x, zero)) : zero;
        member_sums(mine, j & 1u, col);
#pragma unroll
        for (uint32_t i = 0; i < GROUP; ++i) {
            const Real kc = col[i] * k[j];
            if (i < n && j < n) numbers_ok = numbers_ok && col[i] >= -most && col[i] <= most && kc >= -most && kc <= most;
            if constexpr (MIXED) {
                W[i][j] = col[i]; // step 4m keeps C alone
                if constexpr (DAMPED) W[i][j] = wave_uniform(col[i]); // (step 4g keeps it in scalar registers from here on)
                const Real range = sqrt_real(most); // and J multiplies two entries: |C_ij K_j| within the square root of the largest number
                if (i < n && j < n) numbers_ok = numbers_ok && within_bound(kc, range);
                if constexpr (DAMPED) { // and kd_j = K_j (phi' m + phi l_j): |C_ij K_j l_j| within it as well
                    const Real kcl = kc * lam[j];
                    if (i < n && j < n && (damped >> j & 1u)) numbers_ok = numbers_ok && within_bound(kcl, range);
                }
            }
            if constexpr (!MIXED) W[i][j] = (mask >> i & 1u) ? ((mask >> j & 1u) ? (i == j ? Real(1) + kc : kc) : zero) : col[i];
            if (i == j) c_own[i] = col[i];
        }
    }
    bool pivots_ok = true;
    Real ckd[GROUP] = {}, ck15[GROUP] = {}; // step 4m: ck_jj = C_jj K_j and 1.5 ck_jj, once per block
    if constexpr (MIXED) {
        // a Hertz member: C_ii and C_ii K_i not below 0, as in step 4h; a linear one: 1 + C_ii K_i a finite number above 0, as in step 4
#pragma unroll
        for (uint32_t i = 0; i < GROUP; ++i) {
            ckd[i] = W[i][i] * k[i];
            ck15[i] = Real(1.5) * ckd[i];
            if constexpr (DAMPED) ckd[i] = wave_uniform(ckd[i]), ck15[i] = wave_uniform(ck15[i]);
            const Real denom = Real(1) + ckd[i];
            if (i < n) pivots_ok = pivots_ok && ((hertz >> i & 1u) ? (W[i][i] >= Real(0) && ckd[i] >= Real(0)) : finite_above_zero(denom));
            if constexpr (DAMPED) { // a damped member: C_ii, C_ii K_i and C_ii K_i l_i not below 0, as in step 4d
                const Real cl = ckd[i] * lam[i];
                if (i < n && (damped >> i & 1u)) pivots_ok = pivots_ok && W[i][i] >= Real(0) && ckd[i] >= Real(0) && finite_from_zero(cl);
            }
        }
    }
#pragma unroll
    for (uint32_t p = 0; p < GROUP && !MIXED; ++p) {
        const bool in_p = mask >> p & 1u;
        const Real pivot = W[p][p];
        pivots_ok = pivots_ok && (!in_p || (pivot > Real(0) && pivot <= most)); // a finite number above 0 (a NaN fails both)
        const Real r = Real(1) / pivot;
        W[p][p] = in_p ? Real(1) : W[p][p];
#pragma unroll
        for (uint32_t j = 0; j < GROUP; ++j) W[p][j] = in_p ? W[p][j] * r : W[p][j];
#pragma unroll
        for (uint32_t i = 0; i < GROUP; ++i) {
            if (i == p) continue;
            const bool both = in_p && (mask >> i & 1u);
            const Real t = W[i][p];
            W[i][p] = both ? Real(0) : W[i][p];
#pragma unroll
            for (uint32_t j = 0; j < GROUP; ++j) W[i][j] = both ? W[i][j] - t * W[p][j] : W[i][j];
        }
    }
    const bool solved = numbers_ok && (MIXED ? pivots_ok : __builtin_amdgcn_ballot_w64(admissible && !pivots_ok) == 0);
    uint32_t unconverged = 0; // step 4m: frames of the block that failed the residual test
    DampedGroup<Real> dg; // step 4g: the block's constants as wave-uniform values
    if constexpr (DAMPED) {
#pragma unroll
        for (uint32_t i = 0; i < GROUP; ++i) {
#pragma unroll
            for (uint32_t j = 0; j < GROUP; ++j) dg.c[i][j] = wave_uniform(W[i][j]);
            dg.k[i] = wave_uniform(k[i]), dg.ck[i] = wave_uniform(ckd[i]), dg.ck15[i] = wave_uniform(ck15[i]), dg.lam[i] = wave_uniform(lam[i]);
            y_prev[i] = wave_uniform(y_prev[i]);
        }
        dg.hertz = __builtin_amdgcn_readfirstlane(hertz), dg.bilateral = __builtin_amdgcn_readfirstlane(bilateral), dg.damped = __builtin_amdgcn_readfirstlane(damped);
        known = __builtin_amdgcn_readfirstlane(known);
    }
    if (threadIdx.x == 0)
        for (uint32_t i = 0; i < n; ++i) {
            ga.compliance_out[G->member[i].row] = double(c_own[i]);
            ga.status_out[G->member[i].row] = solved ? MH_JUNCTION_SOLVED : MH_JUNCTION_REFUSED;
        }
    Real *tap_row = nullptr;
    if constexpr (OBSERVE) tap_row = tap_of<Real>(ga, active, G->first_wave + wave, frames, lane);
    for (uint32_t s0 = 0; s0 < frames; s0 += TS) {
        const uint32_t sn = min(TS, frames - s0);
        // this tile's approach samples, lane = sample (not finite: 0, as a drive's)
        using Approach = std::conditional_t<DAMPED, float, Real>; // (step 4g's entries keep the approach as the float it came as: the same bits once widened, half the registers in fp64)
        Approach u_tile[GROUP] = {};
#pragma unroll
        for (uint32_t i = 0; i < GROUP; ++i)
            if (i < n && lane < sn) u_tile[i] = finite_or_zero<Approach>(ga.approach[size_t(G->member[i].row) * frames + s0 + lane]);
        // the tile's excitation, parked where the output terms will go
        for (uint32_t ds = 0; ds < sn; ++ds) {
            Pair excite = {0, 0};
            for (uint32_t t = 0; t < n_imp; ++t) {
                const Real f = force[size_t(imp_idx[i0 + t]) * frames + s0 + ds];
                excite += f * (t < REG_ROWS ? g_reg[t] : *reinterpret_cast<const Pair *>(g_mem + size_t(t) * MODES_PER_WAVE + 2 * lane));
            }
            *reinterpret_cast<Pair *>(s_term + ds * PITCH + 2 * lane) = excite;
        }
        Real f_tile[GROUP] = {};
        for (uint32_t ds = 0; ds < sn; ++ds) {
            const Pair excite = *reinterpret_cast<const Pair *>(s_term + ds * PITCH + 2 * lane); // what this lane parked
            const Pair re = w.z_re * w.c_re - w.z_im * w.c_im + excite;
            w.z_im = w.z_re * w.c_im + w.z_im * w.c_re;
            Real mine[GROUP], d[GROUP], x[GROUP];
#pragma unroll
            for (uint32_t i = 0; i < GROUP; ++i)
                mine[i] = fma_real(g_re[i].y, re.y, fma_real(g_im[i].y, w.z_im.y, fma_real(g_re[i].x, re.x, fma_real(g_im[i].x, w.z_im.x, zero))));
            member_sums(mine, (s0 + ds) & 1u, d);
#pragma unroll
            for (uint32_t i = 0; i < GROUP; ++i) x[i] = Real(lane_bcast(u_tile[i], ds)) - d[i];
            Real f_now[GROUP];
            if constexpr (DAMPED) {
                // step 4g (modalhip.h): damped_group_solve; y_p and the history mask go from frame to frame in registers
                Real xs[GROUP], f[GROUP];
#pragma unroll
                for (uint32_t i = 0; i < GROUP; ++i) xs[i] = wave_uniform(x[i]);
                const bool met = damped_group_solve(dg, xs, known, y_prev, f);
                known = dg.damped;
                if (solved && !met) ++unconverged;
#pragma unroll
                for (uint32_t i = 0; i < GROUP; ++i) f_now[i] = solved ? f[i] : zero;
            } else if constexpr (MIXED) {
                // step 4m (modalhip.h): each member alone, MIXED_SWEEPS Gauss-Seidel sweeps, MIXED_STEPS Newton steps, the residual test
                Real y[GROUP], f[GROUP], kd[GROUP], F[GROUP]; // kd: K phi'
                auto law = [&](uint32_t j) {
                    Real phi, dphi;
                    mixed_law(y[j], hertz >> j & 1u, bilateral >> j & 1u, phi, dphi);
                    f[j] = k[j] * phi;
                    kd[j] = k[j] * dphi;
                };
#pragma unroll
                for (uint32_t j = 0; j < GROUP; ++j) {
                    y[j] = mixed_alone(x[j], ckd[j], ck15[j], hertz >> j & 1u, bilateral >> j & 1u);
                    law(j);
                }
#pragma unroll 1
                for (int sweep = 0; sweep < MIXED_SWEEPS; ++sweep) {
#pragma unroll
                    for (uint32_t j = 0; j < GROUP; ++j) {
                        Real acc = 0;
#pragma unroll
                        for (uint32_t i = 0; i < GROUP; ++i)
                            if (i != j) acc = acc + W[j][i] * f[i];
                        y[j] = mixed_alone(x[j] - acc, ckd[j], ck15[j], hertz >> j & 1u, bilateral >> j & 1u);
                        law(j);
                    }
                }
                group_residual<false>(W, y, f, x, MIXED_STEPS <= MIXED_REFINED, F);
#pragma unroll 1
                for (int step = 0; step < MIXED_STEPS; ++step) {
                    Real d[GROUP];
                    newton_direction(W, kd, F, d);
#pragma unroll
                    for (uint32_t j = 0; j < GROUP; ++j) {
                        y[j] = y[j] - d[j];
                        law(j);
                    }
                    group_residual<false>(W, y, f, x, step + 1 >= MIXED_STEPS - MIXED_REFINED, F);
                }
                // the residual test: |F_i| against 16 u (|y_i| + sum_j |C_ij f_j| + |x_i|)
                Real size[GROUP];
#pragma unroll
                for (uint32_t j = 0; j < GROUP; ++j) size[j] = __builtin_fabs(f[j]);
                const bool met = residual_met(W, y, size, x, F, Real(16));
                if (solved && !met) ++unconverged;
#pragma unroll
                for (uint32_t i = 0; i < GROUP; ++i) f_now[i] = solved ? f[i] : zero;
            } else {
            // this lane's subset: its candidate, and whether it is consistent
            Real y[GROUP], f[GROUP];
            bool consistent = admissible;
            Real miss = 0; // by how much the subset fails: the largest -y_j of a unilateral member, or residual of a member outside it, above 0
#pragma unroll
            for (uint32_t i = 0; i < GROUP; ++i) {
                Real acc = 0;
#pragma unroll
                for (uint32_t j = 0; j < GROUP; ++j) acc = (mask >> j & 1u) ? acc + W[i][j] * x[j] : acc;
                y[i] = acc;
                f[i] = (mask >> i & 1u) ? k[i] * acc : zero;
            }
#pragma unroll
            for (uint32_t j = 0; j < GROUP; ++j) {
                Real push = 0;
#pragma unroll
                for (uint32_t i = 0; i < GROUP; ++i) push = (mask >> i & 1u) ? push + W[j][i] * f[i] : push;
                const bool inside = mask >> j & 1u;
                const Real over = inside ? ((bilateral >> j & 1u) ? zero : zero - y[j]) : x[j] - push;
                const bool fits = inside ? ((bilateral >> j & 1u) || y[j] > Real(0)) : !(over > Real(0));
                consistent = consistent && fits;
                miss = over > miss ? over : miss;
            }
            uint64_t found = __builtin_amdgcn_ballot_w64(consistent);
            const bool clamp = found == 0; // no subset consistent (rounding, on a boundary between two of them): the one that fails by least, clamped
            if (clamp) {
                Real least = admissible ? miss : most; // over lanes 0 .. 15: one row of the DPP tree
                Real other = mh_dpp_move<MH_DPP_QUAD_XOR1>(least);
                least = other < least ? other : least;
                other = mh_dpp_move<MH_DPP_QUAD_XOR2>(least);
                least = other < least ? other : least;
                other = mh_dpp_move<MH_DPP_ROW_HALF_MIRROR>(least);
                least = other < least ? other : least;
                other = mh_dpp_move<MH_DPP_ROW_MIRROR>(least);
                least = other < least ? other : least;
                found = __builtin_amdgcn_ballot_w64(admissible && miss == least);
            }
            const uint32_t taken = found ? uint32_t(__builtin_ctzll(found)) : full; // (found = 0: a NaN; the full set stands in)
#pragma unroll
            for (uint32_t i = 0; i < GROUP; ++i) {
                // (off the lane's subset y[i] is a product with a row of C, not a displacement: the force there is +0, clamped or not)
                const Real clamped = (mask >> i & 1u) ? ((bilateral >> i & 1u) ? f[i] : k[i] * (y[i] > Real(0) ? y[i] : zero)) : zero;
                f_now[i] = solved ? lane_bcast(clamp ? clamped : f[i], taken) : zero;
            }
            }
            // step 5: the members on this wave's object, in ascending order
            Pair z = re;
#pragma unroll
            for (uint32_t i = 0; i < GROUP; ++i)
                if (on >> i & 1u) z = z + a[i] * f_now[i];
            w.z_re = z;
            *reinterpret_cast<Pair *>(s_term + ds * PITCH + 2 * lane) = w.p_im * w.z_im + w.p_re * w.z_re;
            if constexpr (OBSERVE)
                if (tap_row) tap_store(tap_row, s0 + ds, w.z_im, w.z_re);
#pragma unroll
            for (uint32_t i = 0; i < GROUP; ++i)
                if (lane == ds) f_tile[i] = f_now[i];
        }
        // member i's row: one store per tile, by wave i of the launch (or the wave that stands for it in a smaller one)
#pragma unroll
        for (uint32_t i = 0; i < GROUP; ++i)
            if (i < n && wave == i % block_waves && lane < sn) ga.force_out[size_t(G->member[i].row) * frames + s0 + lane] = f_tile[i];
        junction_turn_around<TS>(s_term, w, lane, s0, sn, partial, frames);
    }
    if constexpr (MIXED)
        if (threadIdx.x == 0)
            for (uint32_t i = 0; i < n; ++i) ga.unconverged_out[G->member[i].row] = unconverged;
    if constexpr (DAMPED)
        if (threadIdx.x == 0)
            for (uint32_t i = 0; i < n; ++i)
                if (damped >> i & 1u) ga.carry_out[G->member[i].row] = y_prev[i]; // (the host hands it on only for a solved group)
    store_wave(b, w, lane, chunk_energy);
}
template<typename Real> constexpr auto k_bank_modes_grouped_observed = &k_bank_modes_grouped<Real, true>;
template<typename Real> constexpr auto k_bank_modes_grouped_mixed = &k_bank_modes_grouped<Real, false, true>;
template<typename Real> constexpr auto k_bank_modes_grouped_mixed_observed = &k_bank_modes_grouped<Real, true, true>;
template<typename Real> constexpr auto k_bank_modes_grouped_damped = &k_bank_modes_grouped<Real, false, true, true>;
template<typename Real> constexpr auto k_bank_modes_grouped_damped_observed = &k_bank_modes_grouped<Real, true, true, true>;
#undef BANK_MODES_PARAMS
#undef BANK_MODES_ARGS
// The partial rows of the pickups on junction objects (mh_bank_render_observed), from the states the tapped waves stored: one wave per
// (tapped wave, tile of 32 frames) stages the object's pickup gains and the tile's states as k_bank_modes_read holds them -- [pickup][im | re]
// [mode], and Im z, Re z as [sample][mode] -- and runs the same per-half sums (read_pickups), so a row is the bits k_bank_modes_read would
// give for the same state trajectory.  taps: the tapped waves as (dealt object, first mode); grid: (tapped waves, tiles).
template<typename Real> constexpr size_t observe_rows_lds() { return (2 * 32 * PITCH + MH_PICKUPS_PER_OBJECT * 2 * MODES_PER_WAVE) * sizeof(Real); }
static_assert(observe_rows_lds<double>() <= 160 * 1024, "k_bank_observe_rows: two state tiles and the staged gains within the 160 KiB of LDS");
template<typename Real>
__global__ void __launch_bounds__(WAVE) k_bank_observe_rows(BankCols<Real> b, const WaveDesc *__restrict__ taps, const uint32_t *__restrict__ deal_objects, const uint32_t *__restrict__ render_count,
                                                            const uint32_t *__restrict__ chunk_base, const Real *__restrict__ out_gain, const Real *__restrict__ listener_gain, uint32_t frames,
                                                            const Real *__restrict__ states, ReadArgs<Real> rd) {
    typedef PairOf<Real> Pair;
    constexpr uint32_t TS = 32;
    __shared__ __attribute__((aligned(16))) Real s_zim[TS * PITCH], s_zre[TS * PITCH];
    __shared__ __attribute__((aligned(16))) Real s_pick[MH_PICKUPS_PER_OBJECT * 2 * MODES_PER_WAVE]; // [pickup][im | re][mode]
    const WaveDesc wd = taps[blockIdx.x];
    const uint32_t lane = threadIdx.x, half = lane / TS, ts = lane % TS, s0 = blockIdx.y * TS;
    if (s0 >= frames) return; // (wave-uniform; the grid has no such tile)
    const uint32_t sn = min(TS, frames - s0);
    const WaveLane<Real> w = load_wave(b, deal_objects, chunk_base, out_gain, listener_gain, wd.dealt, wd.first_mode, render_count[wd.dealt], lane);
    const uint32_t pk0 = rd.pick_ptr[wd.dealt], n_pick = min(rd.pick_ptr[wd.dealt + 1] - pk0, uint32_t(MH_PICKUPS_PER_OBJECT));
    stage_pickup_gains(b, w, rd, pk0, n_pick, lane, s_pick);
    const Real *tile = states + (size_t(blockIdx.x) * frames + s0) * TAP_FRAME + 2 * lane;
    for (uint32_t ds = 0; ds < sn; ++ds) {
        *reinterpret_cast<Pair *>(s_zim + ds * PITCH + 2 * lane) = *reinterpret_cast<const Pair *>(tile + size_t(ds) * TAP_FRAME);
        *reinterpret_cast<Pair *>(s_zre + ds * PITCH + 2 * lane) = *reinterpret_cast<const Pair *>(tile + size_t(ds) * TAP_FRAME + MODES_PER_WAVE);
    }
    mh_lds_writes_landed();
    __syncthreads();
    if (ts < sn) read_pickups(s_zim, s_zre, s_pick, rd, pk0, n_pick, wd.first_mode, half, ts, s0, frames);
}

// Per dealt object (one wave each): energy, audible prefix, whole-object silence (ModalAudio.cpp:132-146).  Loads are
// lane-parallel; every sum runs in the reference's order through wave-uniform lane broadcasts.
template<typename Real> struct ObjectPassArgs {
    BankCols<Real> b;
    const uint32_t *deal_objects, *render_count, *chunk_base, *imp_ptr;
    const Real *out_gain, *chunk_energy;
    uint32_t n_dealt;
    double *energy_out;
    uint32_t *live_out;
    uint8_t *silenced;
    const uint32_t *tuned_count;
    double *modal_energy;
};
template<typename Real> __device__ void bank_object_pass(const ObjectPassArgs<Real> &a, uint32_t d, uint32_t lane) {
    const BankCols<Real> &b = a.b;
    const uint32_t *deal_objects = a.deal_objects, *render_count = a.render_count, *chunk_base = a.chunk_base, *imp_ptr = a.imp_ptr, *tuned_count = a.tuned_count;
    const Real *out_gain = a.out_gain, *chunk_energy = a.chunk_energy;
    double *energy_out = a.energy_out, *modal_energy = a.modal_energy;
    uint32_t *live_out = a.live_out;
    uint8_t *silenced = a.silenced;
    if (d >= a.n_dealt) return;
    const uint32_t o = deal_objects[d], count = render_count[d];
    const Real og = out_gain[o];
    Real energy = 0;
    uint32_t live = 0;
    const uint32_t nchunks = (count + LANES - 1) / LANES, cb = chunk_base[d];
    for (uint32_t c0 = 0; c0 < nchunks; c0 += WAVE) {
        const uint32_t m = min(uint32_t(WAVE), nchunks - c0);
        const Real mine = lane < m ? chunk_energy[cb + c0 + lane] : Real(0);
        for (uint32_t l = 0; l < m; ++l) {
            const Real chunk = lane_bcast(mine, l);
            energy += chunk;
            if (chunk * og * og >= Real(1e-12f)) live = min(count, (c0 + l + 1) * LANES);
        }
    }
    const bool no_impacts = imp_ptr[d + 1] == imp_ptr[d];
    const bool silent = no_impacts && energy * og * og < Real(1e-12f);
    const uint32_t k0 = b.mode_offset[o];
    if (silent) {
        const uint32_t n = b.mode_count[o];
        for (uint32_t k = lane; k < n; k += WAVE) {
            b.state_re[k0 + k] = 0;
            b.state_im[k0 + k] = 0;
        }
    }
    // Mechanical energy behind the pressure-unit states (the diagnostic of ModalAudio.cpp:564-577), in double.
    double me = 0;
    if (!silent) {
        const uint32_t n = tuned_count[d];
        for (uint32_t q0 = 0; q0 < n; q0 += WAVE) {
            const uint32_t m = min(uint32_t(WAVE), n - q0);
            double term = 0;
            if (lane < m) {
                const double g = double(b.rad_gain[k0 + q0 + lane]);
                if (g > 0) {
                    const double re = double(b.state_re[k0 + q0 + lane]), im = double(b.state_im[k0 + q0 + lane]);
                    term = 0.5 * (re * re + im * im) / (g * g);
                }
            }
            for (uint32_t l = 0; l < m; ++l) me += lane_bcast(term, l);
        }
    }
    if (lane == 0) {
        energy_out[d] = double(energy);
        live_out[d] = live;
        silenced[d] = silent ? 1 : 0;
        modal_energy[d] = me;
    }
}

// Renderer r's private buffer: its chunks' partial signals added in chunk order (ModalAudio.cpp:130).  The chain of
// adds per sample is sequential by contract, so the work is a latency problem: one 1024-thread workgroup per
// (SW-sample strip, renderer) streams tiles of RPT*1024/SW chunk rows through LDS with all 16 waves loading (next tile
// in registers while the current one is consumed) and its first wave runs the ordered chain out of LDS.
// The passes after the resonators depend on them (or on the forces) but not on one another, and each is a latency chain that
// fills a few CUs: ONE launch runs them side by side, told apart by blockIdx.y --
//   y < n_renderers                 renderer y's ordered chunk sum
//   y == n_renderers (click_rows)   the impacts' click rows added, in impact order, to what the caller left in the block
//                                   (click_inout: a workgroup reads its own strip's start values before it writes them)
//   above                           the per-object pass, one wave per dealt object
template<typename Real, int SW>
__global__ void __launch_bounds__(1024) k_bank_post(const Real *__restrict__ partial, const uint32_t *__restrict__ renderer_chunk_ptr, uint32_t n_renderers, uint32_t frames,
                                                   Real *__restrict__ rout, const Real *__restrict__ click, uint32_t click_rows, Real *__restrict__ click_inout,
                                                   ObjectPassArgs<Real> objects) {
    // An ordered sum: the adds of one sample are a dependent chain (8 192 rows per renderer with every mode live), run by wave 0
    // out of LDS; the block's 16 waves stream tiles of rows in, transposed, so that a chain lane reads four consecutive rows with
    // one 16-byte LDS read.  Two tile buffers, one barrier per tile: the next tile lands while this one is added.
    constexpr int RPT = 32 / sizeof(Real), ROUND = 1024 / SW, TILE = RPT * ROUND, PITCH = TILE + 16 / sizeof(Real);
    extern __shared__ __attribute__((aligned(16))) unsigned char post_lds[];
    Real *xs = reinterpret_cast<Real *>(post_lds); // [2][SW][PITCH]
    const uint32_t tid = threadIdx.x, col = tid % SW, rr = tid / SW;
    const uint32_t sum_slices = n_renderers + (click_rows ? 1u : 0u);
    if (blockIdx.y >= sum_slices) {
        bank_object_pass<Real>(objects, ((blockIdx.y - sum_slices) * gridDim.x + blockIdx.x) * (1024 / WAVE) + tid / WAVE, tid % WAVE);
        return;
    }
    const uint32_t r = blockIdx.y;
    const bool clicks = r >= n_renderers;
    if (clicks) partial = click;
    const Real *start = clicks ? click_inout : nullptr;
    const uint32_t c_begin = clicks ? 0u : renderer_chunk_ptr[r], c_end = clicks ? click_rows : renderer_chunk_ptr[r + 1];
    const uint32_t s = blockIdx.x * SW + col;
    const bool in_range = s < frames;
    const uint32_t sc = in_range ? s : frames - 1; // loads of a strip's missing samples read the last one (never stored)
    // wave 0 runs the chain, a pure latency problem; the others (and whatever else shares the CU in this launch) only feed it: it
    // goes first whenever it can issue
    if (tid < WAVE) __builtin_amdgcn_s_setprio(3);
    Real pre[RPT];
    // rows past the end read the last row: the chain stops at the row count, nothing is zero-filled
    auto fetch = [&](uint32_t base) {
        if (base + TILE <= c_end) {
            const Real *p = partial + size_t(base + rr) * frames + sc;
#pragma unroll
            for (int j = 0; j < RPT; ++j) pre[j] = p[size_t(j) * ROUND * frames];
        } else {
#pragma unroll
            for (int j = 0; j < RPT; ++j) pre[j] = partial[size_t(min(base + j * ROUND + rr, c_end - 1)) * frames + sc];
        }
    };
    auto commit = [&](int buf) {
        Real *dst = xs + (size_t(buf) * SW + col) * PITCH + rr;
#pragma unroll
        for (int j = 0; j < RPT; ++j) dst[j * ROUND] = pre[j];
    };
    Real acc = (start && tid < SW && in_range) ? start[s] : Real(0);
    // (this load must have landed on every path into the tile loop: left pending on one of them, the compiler guards the chain's
    // first add with a wait for ALL outstanding loads -- which inside the loop are the next tile's, so the chain would start only
    // after its own prefetch had returned)
    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0)
    if (c_begin < c_end) {
        fetch(c_begin);
        commit(0);
    }
    __syncthreads();
    typedef Real Quad __attribute__((ext_vector_type(4)));
    int buf = 0;
    for (uint32_t base = c_begin; base < c_end; base += TILE, buf ^= 1) {
        const bool more = base + TILE < c_end;
        if (more) fetch(base + TILE);
        if (tid < SW) {
            const uint32_t cnt = min(uint32_t(TILE), c_end - base);
            const Real *row = xs + (size_t(buf) * SW + col) * PITCH;
            // the adds are one dependent chain; the LDS reads are not: the next sixteen rows are on their way while these sixteen are
            // added (a read's latency is about sixteen dependent adds)
            uint32_t q = 0;
            auto quad = [&](uint32_t at) { return *reinterpret_cast<const Quad *>(row + at); };
            auto add4 = [&](const Quad &v) { acc += v.x, acc += v.y, acc += v.z, acc += v.w; };
            if (cnt >= 16) {
                Quad a0 = quad(0), a1 = quad(4), a2 = quad(8), a3 = quad(12), b0, b1, b2, b3;
                for (; q + 48 <= cnt; q += 32) {
                    b0 = quad(q + 16), b1 = quad(q + 20), b2 = quad(q + 24), b3 = quad(q + 28);
                    add4(a0), add4(a1), add4(a2), add4(a3);
                    a0 = quad(q + 32), a1 = quad(q + 36), a2 = quad(q + 40), a3 = quad(q + 44);
                    add4(b0), add4(b1), add4(b2), add4(b3);
                }
                add4(a0), add4(a1), add4(a2), add4(a3);
                q += 16;
            }
            for (; q < cnt; ++q) acc += row[q];
        }
        if (more) commit(buf ^ 1); // the other buffer: its chain ended before the last barrier
        __syncthreads();
    }
    if (tid < SW && in_range) (clicks ? click_inout[s] : rout[size_t(r) * frames + s]) = acc;
}
template<typename Real, int SW> size_t bank_post_lds() { return size_t(2) * SW * ((32 / sizeof(Real)) * (1024 / SW) + 16 / sizeof(Real)) * sizeof(Real); }
// Host-pinned staging buffer mirrored by a device buffer: every small per-block array travels to the device in ONE copy.  Nothing
// is copied back: the kernels that produce what the host reads (impact states, per-object energies, the block's samples) write it
// into the pinned arena themselves, and the block's last kernel then raises a sequence number the host spins on -- a blit +
// hipStreamSynchronize cost the copy engine's completion signal and a thread wake-up (~40 us of a 0.34 ms block), a copy kernel for
// the ~120 KB region 15 us at the end of the chain; the spin sees the results ~2 us after the last kernel.
// That last kernel is the mix: out[s] += clicks in impact order (when they did not go through the streaming sum), then the
// renderers' buffers in renderer order (ModalAudio.cpp:531,553-555).
template<typename Real>
__global__ void __launch_bounds__(256) k_bank_mix(const Real *__restrict__ click, uint32_t n_impacts, const Real *__restrict__ rout, uint32_t n_renderers, uint32_t frames,
                                                  const Real *__restrict__ out_dev, Real *__restrict__ out_host, volatile uint32_t *flag_host, uint32_t seq) {
    for (uint32_t s = threadIdx.x; s < frames; s += 256) {
        Real acc = out_dev[s];
        for (uint32_t i = 0; i < n_impacts; ++i) acc += click[size_t(i) * frames + s];
        for (uint32_t r = 0; r < n_renderers; ++r) acc += rout[size_t(r) * frames + s];
        out_host[s] = acc;
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        *flag_host = seq;
        __threadfence_system();
    }
}

struct Arena {
    char *host{nullptr}, *dev{nullptr}, *host_seen_by_device{nullptr};
    uint32_t *flag{nullptr}, *flag_seen_by_device{nullptr}; // pinned word the download kernel raises
    uint32_t seq{0};
    size_t cap{0}, used{0};
    void reserve(size_t n) {
        if (n <= cap) return;
        release();
        cap = n + n / 2 + 4096;
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&host), cap, hipHostMallocMapped));
        HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void **>(&host_seen_by_device), host, 0));
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&flag), 64, hipHostMallocMapped));
        HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void **>(&flag_seen_by_device), flag, 0));
        *flag = 0;
        seq = 0;
        HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&dev), cap));
    }
    void release() {
        if (host) (void)hipHostFree(host);
        if (flag) (void)hipHostFree(flag);
        if (dev) (void)hipFree(dev);
        host = dev = host_seen_by_device = nullptr;
        flag = flag_seen_by_device = nullptr;
        cap = 0;
    }
    // the block's mix into the pinned arena, then wait for it: spin on the flag, with the stream's own synchronisation as the way
    // out of a stall (and the place where an asynchronous error would surface)
    template<typename Real>
    void mix_and_wait(hipStream_t st, const Real *click, uint32_t n_impacts, const Real *rout, uint32_t n_renderers, uint32_t frames, size_t out_off) {
        ++seq;
        k_bank_mix<Real><<<1, 256, 0, st>>>(click, n_impacts, rout, n_renderers, frames, d<Real>(out_off), hd<Real>(out_off), flag_seen_by_device, seq);
        HIP_CHECK(hipGetLastError());
        const volatile uint32_t *f = flag;
        for (uint64_t spin = 0; *f != seq; ++spin) {
            __builtin_ia32_pause();
            if (spin > (1ull << 22)) { // ~10 ms: not a normal block any more
                HIP_CHECK(hipStreamSynchronize(st));
                break;
            }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
    }
    size_t take(size_t bytes) {
        const size_t o = used;
        used += (bytes + 63) & ~size_t(63);
        return o;
    }
    template<typename T> T *h(size_t off) const { return reinterpret_cast<T *>(host + off); }
    template<typename T> T *d(size_t off) const { return reinterpret_cast<T *>(dev + off); }
    template<typename T> T *hd(size_t off) const { return reinterpret_cast<T *>(host_seen_by_device + off); } // the pinned arena as kernels address it
    ~Arena() { release(); }
};

// The junction groups of a call by what step 4 solves: linear members only (k_bank_modes_grouped), a Hertz member (mh_bank_render_mixed,
// step 4m), a damped member (mh_bank_render_damped_groups, step 4g).  Each class has a launch of its own, and the device's list holds the
// classes in this order.
enum { LINEAR_GROUPS, HERTZ_GROUPS, DAMPED_GROUPS, GROUP_CLASSES };
template<typename Real> struct GroupClass {
    std::vector<GroupDev<Real>> groups; // in call order, until they take their place in the device's list
    uint32_t widest{0}, members{0}; // the waves of the widest group; the junctions of all of them
    uint32_t count() const { return uint32_t(groups.size()); }
};

// The render entries are a ladder: each admits what the one before it admits, plus one thing.  mh_bank_render, _driven and _read are the
// coupled entry without junctions (and without pickups, without drives).
enum class Entry {
    Coupled, // junctions; MH_JUNCTION_DAMPED is ignored
    Damped, // + damping and the carry
    Observed, // + a pickup on a kept junction's object is read
    Mixed, // + a Hertz junction may join a group (step 4m), unconverged_out
    DampedGroups, // + a damped junction may join a group as well (step 4g)
    Friction, // + MH_JUNCTION_FRICTION on a lone junction (step 4t): the tangential channel, the anchor, the counts
};
// What the widest entry takes, in the order the entries name it; an entry leaves what it does not take at zero.
struct RenderRequest {
    Entry entry;
    uint32_t frames;
    float click_gain;
    uint32_t n_impacts;
    mh_impact *impacts;
    uint32_t n_renderers;
    const uint32_t *deal_offset, *deal_objects, *render_count, *tuned_count;
    const float *out_gain, *listener_gain;
    void *out;
    double *object_energy;
    uint32_t *object_live;
    uint8_t *object_silenced;
    double *object_modal_energy;
    uint32_t n_drives{0}; const mh_drive *drives{nullptr}; const float *signals{nullptr};
    uint32_t n_pickups{0}; const mh_pickup *pickups{nullptr}; void *pickup_out{nullptr}; uint8_t *pickup_read{nullptr};
    uint32_t n_junctions{0}; const mh_junction *junctions{nullptr}; const float *approach{nullptr}; void *force_out{nullptr}; double *compliance_out{nullptr}; uint8_t *status_out{nullptr};
    const float *damping{nullptr}; void *carry{nullptr};
    uint32_t *unconverged_out{nullptr};
    const mh_friction *friction{nullptr}; const float *travel{nullptr}; void *tangent_out{nullptr}; void *anchor{nullptr}; uint32_t *friction_counts_out{nullptr};
};

template<typename Real> struct BankImpl {
    using Scalar = Real;
    mh_context *ctx;
    uint32_t n_objects, n_modes, n_shapes;
    DevArray<Real> coeff_re, coeff_im, state_re, state_im, rad_gain, phase_im, phase_re, shape_x, shape_y, shape_z;
    DevArray<Real> defl_gain, read_rows; // the column only pickups read; their partial rows
    DevArray<uint32_t> mode_offset, mode_count, shape_offset;
    std::vector<uint32_t> h_mode_count, picks_on, pick_fill;
    std::vector<int32_t> pick_dealt;
    DevArray<Real> junction_gain; // the coupled kernel's scratch gain rows
    DevArray<Real> tap_states; // mh_bank_render_observed: what the tapped waves store, [tapped wave][frame][Im z | Re z][128]
    std::vector<uint8_t> on_junction; // per object: on a side of a junction of this call that was not left out
    std::vector<uint32_t> kept_rows; // the caller's indices of those junctions
    std::vector<uint32_t> mixed_rows; // mh_bank_render_mixed: those of them that are members of a group with a Hertz or a damped member
    std::vector<uint32_t> friction_rows; // mh_bank_render_friction: those of them with MH_JUNCTION_FRICTION
    GroupClass<Real> group_class[GROUP_CLASSES]; // the call's groups by class
    // per-block scratch
    Arena arena;
    DevArray<Real> force, click, partial, chunk_energy, gain_scratch, rout;
    std::vector<int32_t> dealt_of_object, drive_dealt;
    std::vector<uint32_t> imp_fill, h_shape_offset;
    BankCols<Real> cols() {
        return {coeff_re, coeff_im, state_re, state_im, rad_gain, phase_im, phase_re, shape_x, shape_y, shape_z, mode_offset, mode_count, shape_offset};
    }
    // The shape entries object o holds (positions x modes): an index a kernel follows into its shape columns must stay below this
    // (the read would leave the shape buffer).
    uint64_t shapes_held(uint32_t o) const { return uint64_t(o + 1 < n_objects ? h_shape_offset[o + 1] : n_shapes) - h_shape_offset[o]; }
    // A blend (a pickup's, a junction side's) the kernels may follow on its object, which the bank has: three points inside the object's
    // shape columns; finite weights, direction and scale.
    template<typename Record> bool blend_ok(const Record &m) const {
        bool ok = std::isfinite(m.nx) && std::isfinite(m.ny) && std::isfinite(m.nz) && std::isfinite(m.scale);
        for (int c = 0; c < 3; ++c) ok = ok && std::isfinite(m.weights[c]) && (uint64_t(m.points[c]) + 1) * h_mode_count[m.object] <= shapes_held(m.object);
        return ok;
    }
};
template<typename Real, typename Record> BlendDev<Real> blend_dev(const Record &m) {
    return {m.points[0], m.points[1], m.points[2], Real(m.weights[0]), Real(m.weights[1]), Real(m.weights[2]), Real(m.nx), Real(m.ny), Real(m.nz), Real(m.scale)};
}

template<typename T> void ensure(mh_context *ctx, DevArray<T> &a, size_t n) {
    if (a.count < n) a.reset(ctx, n + n / 4 + 16);
}

// A kernel's limit of dynamic LDS raised to the 160 KiB, once per (kernel, device): function attributes are per device, and the first
// blocks of two banks may race.  (A table, not a PerDeviceOnce per call site: which kernel a junction launch takes is decided at run time.)
void raise_lds_limit(int device, const void *kernel) {
    constexpr int MaxKernels = 32; // the junction kernels: 14 per precision
    static std::mutex guard;
    static const void *raised[PerDeviceOnce::MaxDevices][MaxKernels];
    const std::lock_guard<std::mutex> lock(guard);
    const void **row = raised[device >= 0 && device < PerDeviceOnce::MaxDevices ? device : 0];
    int n = 0;
    while (n < MaxKernels && row[n] && row[n] != kernel) ++n;
    if (n < MaxKernels && row[n] == kernel) return;
    HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (n < MaxKernels) row[n] = kernel; // (a full table would only set the attribute again)
}

template<typename Real, typename Src>
void upload_converted(mh_context *ctx, DevArray<Real> &dst, size_t offset, const Src *src, size_t n) {
    if (!n) return;
    std::vector<Real> tmp(src, src + n);
    HIP_CHECK(hipMemcpyAsync(dst.get() + offset, tmp.data(), n * sizeof(Real), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

template<typename Real>
void render_impl(BankImpl<Real> &B, const RenderRequest &r) {
    const auto admits = [&](Entry e) { return r.entry >= e; }; // what the call's entry takes beyond the coupled one's (Entry)
    const uint32_t frames = r.frames, n_impacts = r.n_impacts, n_renderers = r.n_renderers, n_drives = r.n_drives, n_pickups = r.n_pickups, n_junctions = r.n_junctions;
    mh_context *ctx = B.ctx;
    hipStream_t st = ctx->stream;
    Real *out = static_cast<Real *>(r.out);
    const uint32_t n_dealt = n_renderers ? r.deal_offset[n_renderers] : 0;
    uint32_t n_waves = 0;
    for (uint32_t d = 0; d < n_dealt; ++d) n_waves += waves_of(r.render_count[d]);
    // ---- arena layout: [upload only | both ways | download only] ----
    Arena &A = B.arena;
    A.used = 0;
    const size_t o_out_gain = A.take(B.n_objects * sizeof(Real)), o_listener = A.take(B.n_objects * sizeof(Real));
    const size_t o_waves = A.take((n_waves + 1) * sizeof(WaveDesc)), o_deal = A.take((n_dealt + 1) * 4), o_count = A.take((n_dealt + 1) * 4);
    const size_t o_tuned = A.take((n_dealt + 1) * 4), o_chunk_base = A.take((n_dealt + 1) * 4), o_imp_ptr = A.take((n_dealt + 1) * 4);
    // (a drive is a row like an impact's: entry n_impacts + j of the impact array and of the index list, force row n_impacts + j)
    const uint32_t n_rows = n_impacts + n_drives;
    const size_t o_imp_idx = A.take((n_rows + 1) * 4), o_rcp = A.take((n_renderers + 1) * 4);
    const size_t o_out = A.take(frames * sizeof(Real)), o_impacts = A.take((n_rows + 1) * sizeof(ImpactDev<Real>));
    const size_t o_signals = A.take(size_t(n_drives) * frames * sizeof(float));
    const size_t o_pick_ptr = A.take((n_dealt + 2) * 4), o_pick_dev = A.take((n_pickups + 1) * sizeof(PickupDev<Real>)), o_pick_rows = A.take((n_pickups + 1) * sizeof(PickupRows));
    const size_t o_excited = A.take((n_dealt + 1) * 4), o_junctions = A.take((n_junctions + 1) * sizeof(JunctionDev<Real>)), o_approach = A.take(size_t(n_junctions) * frames * sizeof(float));
    const size_t o_groups = A.take((n_junctions / 2 + 1) * sizeof(GroupDev<Real>));
    const size_t o_damping = A.take(admits(Entry::Damped) ? (n_junctions + 1) * sizeof(Real) : 0), o_carry_in = A.take(admits(Entry::Damped) ? (n_junctions + 1) * sizeof(Real) : 0);
    const size_t o_taps = A.take(admits(Entry::Observed) ? (n_waves + 1) * sizeof(WaveDesc) : 0), o_tap_of = A.take(admits(Entry::Observed) ? (n_waves + JUNCTION_WAVES + 1) * 4 : 0);
    const bool with_friction = admits(Entry::Friction) && n_junctions;
    const size_t o_friction = A.take(with_friction ? (n_junctions + 1) * sizeof(FrictionJunctionDev<Real>) : 0), o_travel = A.take(with_friction ? size_t(n_junctions) * frames * sizeof(float) : 0);
    const size_t o_anchor_in = A.take(with_friction ? (n_junctions + 1) * sizeof(Real) : 0);
    const size_t both_end = A.used;
    // (written by the kernels straight into the pinned arena -- no copy back: the host sees them once the block's last kernel has
    // raised the sequence number)
    const size_t o_energy = A.take((n_dealt + 1) * 8), o_modal = A.take((n_dealt + 1) * 8), o_live = A.take((n_dealt + 1) * 4), o_silenced = A.take(n_dealt + 1);
    const size_t o_back = A.take((n_impacts + 1) * sizeof(ImpactBack<Real>));
    const size_t o_pick_out = A.take(size_t(n_pickups) * frames * sizeof(Real));
    const size_t o_junction_force = A.take(size_t(n_junctions) * frames * sizeof(Real)), o_compliance = A.take((n_junctions + 1) * 8), o_status = A.take((n_junctions + 1) * 4);
    const size_t o_carry_out = A.take(admits(Entry::Damped) ? (n_junctions + 1) * sizeof(Real) : 0);
    const size_t o_unconverged = A.take(admits(Entry::Mixed) ? (n_junctions + 1) * 4 : 0);
    const size_t o_tangent = A.take(with_friction ? size_t(n_junctions) * frames * sizeof(Real) : 0), o_anchor_out = A.take(with_friction ? (n_junctions + 1) * sizeof(Real) : 0);
    const size_t o_friction_counts = A.take(with_friction ? (size_t(n_junctions) + 1) * 3 * 4 : 0);
    const size_t total = A.used;
    if (total > A.cap) {
        HIP_CHECK(hipStreamSynchronize(st));
        A.reserve(total);
    }
    // ---- host-side descriptors: waves, chunk bases, per-object impact lists (impact order kept) ----
    WaveDesc *waves = A.h<WaveDesc>(o_waves);
    uint32_t *chunk_base = A.h<uint32_t>(o_chunk_base), *imp_ptr = A.h<uint32_t>(o_imp_ptr), *imp_idx = A.h<uint32_t>(o_imp_idx), *rcp = A.h<uint32_t>(o_rcp);
    B.dealt_of_object.assign(B.n_objects, -1);
    for (uint32_t d = 0; d < n_dealt; ++d)
        if (r.deal_objects[d] < B.n_objects) B.dealt_of_object[r.deal_objects[d]] = int32_t(d);
    // ---- junctions: the ones the coupled kernel may follow, one workgroup each; everything else is left out with a zero row ----
    uint32_t n_coupled = 0, coupled_waves = 0, widest_junction = 0;
    uint32_t n_grouped = 0; // components of two or more junctions: k_bank_modes_grouped, one workgroup each, by class (GroupClass)
    uint32_t n_friction = 0, widest_friction = 0; // lone junctions with MH_JUNCTION_FRICTION: k_bank_modes_coupled_friction, a launch of their own
    B.friction_rows.clear();
    B.mixed_rows.clear();
    for (auto &c : B.group_class) c.groups.clear(), c.widest = c.members = 0;
    bool any_hertz = false; // a kept junction with MH_JUNCTION_HERTZ: the call takes the entry that has the solve
    bool any_damped = false; // a kept junction with MH_JUNCTION_DAMPED: the entry that has both solves and the carry
    const uint32_t flag_mask = (admits(Entry::Damped) ? ~0u : ~uint32_t(MH_JUNCTION_DAMPED)) & (admits(Entry::Friction) ? ~0u : ~uint32_t(MH_JUNCTION_FRICTION));
    B.kept_rows.clear();
    if (n_junctions) {
        JunctionDev<Real> *jd = A.h<JunctionDev<Real>>(o_junctions);
        GroupDev<Real> *gd = A.h<GroupDev<Real>>(o_groups);
        B.on_junction.assign(B.n_objects, 0);
        auto side_ok = [&](const mh_junction_side &sd) {
            if (sd.object >= B.n_objects || B.h_mode_count[sd.object] == 0 || B.dealt_of_object[sd.object] < 0 || r.render_count[B.dealt_of_object[sd.object]] == 0) return false;
            return B.blend_ok(sd);
        };
        auto side_waves = [&](const mh_junction_side &sd) { return waves_of(r.render_count[B.dealt_of_object[sd.object]]); };
        auto side_dev = [&](const mh_junction_side &sd) {
            const uint32_t d = uint32_t(B.dealt_of_object[sd.object]);
            return JunctionSideDev<Real>{d, waves_of(r.render_count[d]), blend_dev<Real>(sd)};
        };
        // which junctions are kept, and which share objects (modalhip_groups.hpp: one junction per object unless both carry MH_JUNCTION_SHARED)
        MhJunctionGroups grouping(B.n_objects);
        for (uint32_t j = 0; j < n_junctions; ++j) {
            const mh_junction &m = r.junctions[j];
            r.status_out[j] = MH_JUNCTION_LEFT_OUT;
            r.compliance_out[j] = 0;
            const bool two_sided = m.b.object != MH_NO_OBJECT;
            if (!std::isfinite(m.stiffness) || m.stiffness < 0 || !side_ok(m.a) || (two_sided && (m.a.object == m.b.object || !side_ok(m.b)))) continue;
            if ((m.flags & MH_JUNCTION_HERTZ) && (m.flags & MH_JUNCTION_BILATERAL)) continue; // the Hertz law is unilateral
            if (m.flags & flag_mask & MH_JUNCTION_DAMPED) { // the damped law is unilateral too, and its l a finite number from 0 up
                if ((m.flags & MH_JUNCTION_BILATERAL) || !std::isfinite(r.damping[j]) || r.damping[j] < 0) continue;
            }
            if (m.flags & flag_mask & MH_JUNCTION_FRICTION) { // friction goes with a lone unilateral undamped junction, and its numbers are finite and not below 0
                if (m.flags & (MH_JUNCTION_BILATERAL | MH_JUNCTION_DAMPED | MH_JUNCTION_SHARED)) continue;
                const mh_friction &t = r.friction[j];
                bool ok = std::isfinite(t.mu) && std::isfinite(t.stiffness) && t.mu >= 0 && t.stiffness >= 0;
                for (int c = 0; c < 3; ++c) ok = ok && std::isfinite(t.ta[c]) && std::isfinite(t.tb[c]);
                if (!ok) continue;
            }
            if (grouping.add(j, m.flags & flag_mask, m.a.object, side_waves(m.a), m.b.object, two_sided ? side_waves(m.b) : 0u, admits(Entry::Mixed), admits(Entry::DampedGroups)) < 0) continue;
            B.on_junction[m.a.object] = 1;
            if (two_sided) B.on_junction[m.b.object] = 1;
            B.kept_rows.push_back(j);
        }
        // a component of one junction is an ordinary junction: the coupled kernel, one workgroup each, in call order
        for (const uint32_t j : B.kept_rows) {
            const mh_junction &m = r.junctions[j];
            if (grouping.components[grouping.of_object[m.a.object]].members.size() != 1) continue;
            const bool two_sided = m.b.object != MH_NO_OBJECT;
            JunctionDev<Real> dev{{side_dev(m.a), two_sided ? side_dev(m.b) : JunctionSideDev<Real>{}}, Real(m.stiffness), m.flags & flag_mask, j, coupled_waves};
            const uint32_t w = dev.side[0].waves + dev.side[1].waves;
            if (dev.flags & MH_JUNCTION_FRICTION) { // a class of its own
                const mh_friction &t = r.friction[j];
                A.h<FrictionJunctionDev<Real>>(o_friction)[n_friction++] = {dev, {{Real(t.ta[0]), Real(t.ta[1]), Real(t.ta[2])}, {Real(t.tb[0]), Real(t.tb[1]), Real(t.tb[2])}}, Real(t.mu), Real(t.stiffness)};
                B.friction_rows.push_back(j);
                coupled_waves += w;
                widest_friction = std::max(widest_friction, w);
                continue;
            }
            jd[n_coupled++] = dev;
            any_hertz = any_hertz || (m.flags & MH_JUNCTION_HERTZ) != 0;
            any_damped = any_damped || (dev.flags & MH_JUNCTION_DAMPED) != 0;
            coupled_waves += w;
            widest_junction = std::max(widest_junction, w);
        }
        // a larger one is a group: its distinct objects in the order its members name them, a wave per 128 rendered modes of each
        for (const auto &comp : grouping.components) {
            if (comp.members.size() < 2) continue;
            GroupDev<Real> g{};
            g.n = uint32_t(comp.members.size());
            g.first_wave = coupled_waves;
            uint32_t object_of_slot[JUNCTION_WAVES];
            auto slot_of = [&](const mh_junction_side &sd) {
                for (uint32_t s = 0; s < g.n_objects; ++s)
                    if (object_of_slot[s] == sd.object) return s;
                if (g.n_objects == JUNCTION_WAVES) mh_throw(MH_EINVAL, "a junction group of more than %u objects", JUNCTION_WAVES); // (the grouping admits none)
                const uint32_t s = g.n_objects++, d = uint32_t(B.dealt_of_object[sd.object]);
                object_of_slot[s] = sd.object;
                g.dealt[s] = d, g.wave0[s] = g.n_waves, g.waves[s] = waves_of(r.render_count[d]);
                g.n_waves += g.waves[s];
                return s;
            };
            for (uint32_t i = 0; i < g.n; ++i) {
                const mh_junction &m = r.junctions[comp.members[i]];
                const bool two_sided = m.b.object != MH_NO_OBJECT;
                GroupMemberDev<Real> &dev = g.member[i];
                dev.k = Real(m.stiffness), dev.flags = m.flags, dev.row = comp.members[i];
                dev.slot[0] = slot_of(m.a), dev.at[0] = blend_dev<Real>(m.a);
                dev.slot[1] = two_sided ? slot_of(m.b) : NO_SLOT;
                if (two_sided) dev.at[1] = blend_dev<Real>(m.b);
            }
            if (g.n_waves > JUNCTION_WAVES) mh_throw(MH_EINVAL, "a junction group of %u waves", g.n_waves); // (the grouping admits none)
            coupled_waves += g.n_waves;
            // (a group has a Hertz member through mh_bank_render_mixed and later only, a damped one through mh_bank_render_damped_groups only)
            const int cls = comp.damped ? DAMPED_GROUPS : comp.hertz ? HERTZ_GROUPS : LINEAR_GROUPS;
            GroupClass<Real> &c = B.group_class[cls];
            c.groups.push_back(g);
            c.members += g.n;
            c.widest = std::max(c.widest, g.n_waves);
            if (cls != LINEAR_GROUPS) B.mixed_rows.insert(B.mixed_rows.end(), comp.members.begin(), comp.members.end());
        }
        for (const auto &c : B.group_class) { // the device's list: class after class
            std::copy(c.groups.begin(), c.groups.end(), gd + n_grouped);
            n_grouped += c.count();
        }
    }
    const bool any_junction = n_coupled || n_grouped || n_friction;
    chunk_base[0] = 0;
    uint32_t main_waves = 0; // the main launch's waves: every dealt object that is not on a junction's side
    for (uint32_t d = 0; d < n_dealt; ++d) {
        const uint32_t count = r.render_count[d];
        chunk_base[d + 1] = chunk_base[d] + (count + LANES - 1) / LANES;
        if (!(any_junction && r.deal_objects[d] < B.n_objects && B.on_junction[r.deal_objects[d]]))
            for (uint32_t k = 0; k < count; k += MODES_PER_WAVE) waves[main_waves++] = {d, k};
        imp_ptr[d + 1] = 0;
    }
    imp_ptr[0] = 0;
    uint32_t max_imp = 1, driven_rows = 0;
    if (n_dealt) {
        for (uint32_t i = 0; i < n_impacts; ++i) {
            const int32_t d = r.impacts[i].object < B.n_objects ? B.dealt_of_object[r.impacts[i].object] : -1;
            if (d >= 0) ++imp_ptr[d + 1];
        }
        // a drive the kernel must not follow is left out here: no such object, an object that was not dealt or has no modes, or an
        // excitation position beyond the object's shape columns (the read would leave the shape buffer)
        B.drive_dealt.assign(n_drives, -1);
        for (uint32_t j = 0; j < n_drives; ++j) {
            const uint32_t o = r.drives[j].object;
            if (o >= B.n_objects || B.dealt_of_object[o] < 0 || B.h_mode_count[o] == 0) continue;
            if ((uint64_t(r.drives[j].ex_pos) + 1) * B.h_mode_count[o] > B.shapes_held(o)) continue;
            B.drive_dealt[j] = B.dealt_of_object[o];
            ++imp_ptr[B.drive_dealt[j] + 1];
            ++driven_rows;
        }
        for (uint32_t d = 0; d < n_dealt; ++d) {
            max_imp = std::max(max_imp, imp_ptr[d + 1]);
            imp_ptr[d + 1] += imp_ptr[d];
        }
        B.imp_fill.assign(imp_ptr, imp_ptr + n_dealt);
        for (uint32_t i = 0; i < n_impacts; ++i) {
            const int32_t d = r.impacts[i].object < B.n_objects ? B.dealt_of_object[r.impacts[i].object] : -1;
            if (d >= 0) imp_idx[B.imp_fill[d]++] = i;
        }
        for (uint32_t j = 0; j < n_drives; ++j) // behind the object's impacts, in the caller's order
            if (B.drive_dealt[j] >= 0) imp_idx[B.imp_fill[B.drive_dealt[j]]++] = n_impacts + j;
    }
    // an object on a junction's side is excited for the block as one with a drive is: where the per-object pass asks "has it rows", it
    // sees one more for such an object (a list of its own: the kernels' row lists stay what they are)
    if (any_junction) {
        uint32_t *excited = A.h<uint32_t>(o_excited);
        excited[0] = 0;
        for (uint32_t d = 0; d < n_dealt; ++d)
            excited[d + 1] = excited[d] + (imp_ptr[d + 1] - imp_ptr[d]) + (r.deal_objects[d] < B.n_objects && B.on_junction[r.deal_objects[d]] ? 1u : 0u);
    }
    // ---- pickups: the ones the kernel may follow, grouped by dealt object in the caller's order; everything else gets a zero row ----
    uint32_t read_row_count = 0, picks_dealt = 0, picks_main = 0; // pickups with rows; those of them whose object the main launch renders
    uint32_t n_taps = 0; // waves of the junction launches whose object carries a pickup (mh_bank_render_observed)
    uint64_t picked_modes = 0; // a pickup adds two multiply-adds per mode-sample of its object
    if (n_pickups) {
        uint32_t *pick_ptr = A.h<uint32_t>(o_pick_ptr);
        PickupDev<Real> *pick_dev = A.h<PickupDev<Real>>(o_pick_dev);
        PickupRows *pick_rows = A.h<PickupRows>(o_pick_rows);
        std::fill(pick_ptr, pick_ptr + n_dealt + 2, 0u);
        B.picks_on.assign(B.n_objects, 0);
        B.pick_dealt.assign(n_pickups, -1);
        for (uint32_t q = 0; q < n_pickups; ++q) {
            const mh_pickup &m = r.pickups[q];
            r.pickup_read[q] = 0;
            pick_rows[q] = {0, 0};
            if (m.object >= B.n_objects || B.h_mode_count[m.object] == 0 || m.advance > 2) continue;
            const bool junction_object = any_junction && B.on_junction[m.object];
            if (junction_object && !admits(Entry::Observed)) continue; // its waves are the coupled kernel's, which reads for no pickup except in mh_bank_render_observed
            if (!B.blend_ok(m) || B.picks_on[m.object] >= MH_PICKUPS_PER_OBJECT) continue;
            ++B.picks_on[m.object];
            r.pickup_read[q] = 1;
            const int32_t d = B.dealt_of_object[m.object];
            if (d < 0 || r.render_count[d] == 0) continue; // at rest: read, and all zeros
            B.pick_dealt[q] = d;
            ++pick_ptr[d + 1];
            ++picks_dealt;
            if (!junction_object) ++picks_main;
        }
        for (uint32_t d = 0; d < n_dealt; ++d) pick_ptr[d + 1] += pick_ptr[d];
        B.pick_fill.assign(pick_ptr, pick_ptr + n_dealt + 1);
        for (uint32_t q = 0; q < n_pickups; ++q) {
            const int32_t d = B.pick_dealt[q];
            if (d < 0) continue;
            const mh_pickup &m = r.pickups[q];
            pick_rows[q] = {read_row_count, 2 * waves_of(r.render_count[d])}; // a row per (wave, half) of the object
            pick_dev[B.pick_fill[d]++] = {blend_dev<Real>(m), m.advance, read_row_count};
            read_row_count += pick_rows[q].n_rows;
            picked_modes += r.render_count[d];
        }
        // the waves of the junction launches that store their states: every wave of a junction object that carries a pickup, by its index
        // among those launches' waves
        if (admits(Entry::Observed) && picks_dealt > picks_main) {
            WaveDesc *taps = A.h<WaveDesc>(o_taps);
            uint32_t *tap_of = A.h<uint32_t>(o_tap_of);
            std::fill(tap_of, tap_of + n_waves + JUNCTION_WAVES + 1, NO_TAP);
            auto tap_object = [&](uint32_t d, uint32_t first_wave, uint32_t object_waves) {
                if (pick_ptr[d + 1] == pick_ptr[d]) return;
                for (uint32_t i = 0; i < object_waves; ++i) {
                    tap_of[first_wave + i] = n_taps;
                    taps[n_taps++] = {d, i * uint32_t(MODES_PER_WAVE)};
                }
            };
            const JunctionDev<Real> *jd = A.h<JunctionDev<Real>>(o_junctions);
            auto tap_junction = [&](const JunctionDev<Real> &j) {
                tap_object(j.side[0].dealt, j.first_wave, j.side[0].waves);
                if (j.side[1].waves) tap_object(j.side[1].dealt, j.first_wave + j.side[0].waves, j.side[1].waves);
            };
            for (uint32_t j = 0; j < n_coupled; ++j) tap_junction(jd[j]);
            for (uint32_t j = 0; j < n_friction; ++j) tap_junction(A.h<FrictionJunctionDev<Real>>(o_friction)[j].j);
            const GroupDev<Real> *gd = A.h<GroupDev<Real>>(o_groups);
            for (uint32_t g = 0; g < n_grouped; ++g)
                for (uint32_t o = 0; o < gd[g].n_objects; ++o) tap_object(gd[g].dealt[o], gd[g].first_wave + gd[g].wave0[o], gd[g].waves[o]);
        }
    }
    for (uint32_t q = 0; q <= n_renderers; ++q) {
        const uint32_t d0 = q < n_renderers ? r.deal_offset[q] : n_dealt;
        rcp[q] = chunk_base[std::min(d0, n_dealt)];
    }
    const uint32_t n_chunks = chunk_base[n_dealt];
    std::copy(r.out_gain, r.out_gain + B.n_objects, A.h<Real>(o_out_gain));
    std::copy(r.listener_gain, r.listener_gain + B.n_objects, A.h<Real>(o_listener));
    std::copy(r.deal_objects, r.deal_objects + n_dealt, A.h<uint32_t>(o_deal));
    std::copy(r.render_count, r.render_count + n_dealt, A.h<uint32_t>(o_count));
    std::copy(r.tuned_count, r.tuned_count + n_dealt, A.h<uint32_t>(o_tuned));
    std::copy(out, out + frames, A.h<Real>(o_out));
    ImpactDev<Real> *himp = A.h<ImpactDev<Real>>(o_impacts);
    for (uint32_t i = 0; i < n_impacts; ++i) {
        const mh_impact &m = r.impacts[i];
        himp[i] = {m.object, m.ex_pos, m.samples_left, 0, Real(m.jx), Real(m.jy), Real(m.jz), Real(m.phase_re), Real(m.phase_im), Real(m.rot_re), Real(m.rot_im),
                   Real(m.gamma), Real(m.accel_amp), Real(m.click_b0), Real(m.click_a1), Real(m.click_a2), Real(m.click_z1), Real(m.click_z2)};
    }
    for (uint32_t j = 0; j < n_drives; ++j) { // only object, ex_pos and the direction are read of a drive's entry
        const mh_drive &m = r.drives[j];
        himp[n_impacts + j] = {m.object, m.ex_pos, 0, 0, Real(m.jx), Real(m.jy), Real(m.jz), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    }
    if (n_drives) std::copy(r.signals, r.signals + size_t(n_drives) * frames, A.h<float>(o_signals));
    if (any_junction) std::copy(r.approach, r.approach + size_t(n_junctions) * frames, A.h<float>(o_approach));
    if (any_damped || B.group_class[DAMPED_GROUPS].count()) {
        std::copy(r.damping, r.damping + n_junctions, A.h<Real>(o_damping));
        std::copy(static_cast<const Real *>(r.carry), static_cast<const Real *>(r.carry) + n_junctions, A.h<Real>(o_carry_in));
    }
    for (const uint32_t j : B.friction_rows) { // travel and anchor are read for flagged junctions only
        std::copy(r.travel + size_t(j) * frames, r.travel + size_t(j + 1) * frames, A.h<float>(o_travel) + size_t(j) * frames);
        A.h<Real>(o_anchor_in)[j] = static_cast<const Real *>(r.anchor)[j];
    }
    HIP_CHECK(hipMemcpyAsync(A.dev, A.host, both_end, hipMemcpyHostToDevice, st));
    // ---- device passes ----
    Real *d_out_gain = A.d<Real>(o_out_gain), *d_listener = A.d<Real>(o_listener), *d_out = A.d<Real>(o_out);
    ImpactDev<Real> *d_impacts = A.d<ImpactDev<Real>>(o_impacts);
    ensure(ctx, B.force, size_t(std::max<uint32_t>(n_rows, 1)) * frames);
    ensure(ctx, B.click, size_t(std::max<uint32_t>(n_impacts, 1)) * frames);
    if (n_impacts) {
        k_bank_forces<Real><<<div_up(n_impacts, 64), 64, 0, st>>>(d_impacts, n_impacts, d_listener, Real(r.click_gain), frames, B.force, B.click, A.hd<ImpactBack<Real>>(o_back));
        KERNEL_CHECK();
    }
    if (n_drives) {
        const size_t n = size_t(n_drives) * frames;
        k_bank_drive_rows<Real><<<uint32_t(div_up(n, size_t(256))), 256, 0, st>>>(A.d<float>(o_signals), n, B.force.get() + size_t(n_impacts) * frames);
        KERNEL_CHECK();
    }
    ensure(ctx, B.rout, size_t(std::max<uint32_t>(n_renderers, 1)) * frames);
    if (n_dealt) {
        ensure(ctx, B.partial, size_t(n_chunks + 1) * frames);
        ensure(ctx, B.chunk_energy, n_chunks + 1);
        ensure(ctx, B.gain_scratch, size_t(n_waves + 1) * max_imp * MODES_PER_WAVE);
        // a mode kernel's launch: the common arguments (BANK_MODES_PARAMS), the launch's own scratch gain rows, then what only that kernel takes
        auto launch_modes = [&](auto *kernel, uint32_t grid, uint32_t block, size_t lds, Real *scratch, auto... more) {
            kernel<<<grid, block, lds, st>>>(B.cols(), A.d<WaveDesc>(o_waves), A.d<uint32_t>(o_deal), A.d<uint32_t>(o_count), A.d<uint32_t>(o_chunk_base), A.d<uint32_t>(o_imp_ptr),
                                             A.d<uint32_t>(o_imp_idx), d_impacts, B.force, d_out_gain, d_listener, frames, B.partial, B.chunk_energy, scratch, max_imp, more...);
            KERNEL_CHECK();
        };
        // A launch of junction objects, one workgroup per junction or per group: the scratch gain rows, the kernel's LDS limit, the bound on
        // the widest workgroup, and the kernel -- when some junction object carries a pickup, the one that also stores the tapped waves' states.
        // solved: the junctions the launch solves per frame (MH_KERNEL_JUNCTION's work).
        static_assert(coupled_lds<Real>(JUNCTION_WAVES) <= 160 * 1024 && grouped_lds<Real>(JUNCTION_WAVES) <= 160 * 1024 && friction_lds<Real>(JUNCTION_WAVES) <= 160 * 1024, "the junction kernels' LDS within the 160 KiB");
        auto launch_junctions = [&](auto *plain, auto *observed, const auto &args, uint32_t workgroups, uint32_t widest, size_t lds, uint32_t solved) {
            if (!workgroups) return;
            if (lds > 160 * 1024) mh_throw(MH_EINVAL, "a junction workgroup of %u waves", widest); // (none is kept)
            ensure(ctx, B.junction_gain, size_t(coupled_waves + JUNCTION_WAVES) * max_imp * MODES_PER_WAVE);
            if (n_taps) ensure(ctx, B.tap_states, size_t(n_taps) * frames * TAP_FRAME);
            raise_lds_limit(ctx->device, n_taps ? reinterpret_cast<const void *>(observed) : reinterpret_cast<const void *>(plain));
            TimedLaunch timed(ctx, MH_KERNEL_JUNCTION, double(solved) * double(frames));
            if (n_taps) launch_modes(observed, workgroups, widest * WAVE, lds, B.junction_gain, ObservedArgs<Real, std::decay_t<decltype(args)>>{args, A.d<uint32_t>(o_tap_of), B.tap_states});
            else launch_modes(plain, workgroups, widest * WAVE, lds, B.junction_gain, args);
        };
        Real *d_damping = A.d<Real>(o_damping), *d_carry_in = A.d<Real>(o_carry_in), *carry_out = A.hd<Real>(o_carry_out);
        // lone junctions: the kernel with the laws the kept ones need
        const CoupledArgs<Real> ca{B.defl_gain, A.d<JunctionDev<Real>>(o_junctions), A.d<float>(o_approach), A.hd<Real>(o_junction_force), A.hd<double>(o_compliance), A.hd<uint32_t>(o_status)};
        if (any_damped)
            launch_junctions(k_bank_modes_coupled_damped<Real>, k_bank_modes_coupled_damped_observed<Real>, DampedArgs<Real>{ca, d_damping, d_carry_in, carry_out}, n_coupled, widest_junction,
                             coupled_lds<Real>(widest_junction), n_coupled);
        else
            launch_junctions(any_hertz ? k_bank_modes_coupled_hertz<Real> : &k_bank_modes_coupled<Real>, any_hertz ? k_bank_modes_coupled_hertz_observed<Real> : k_bank_modes_coupled_observed<Real>, ca,
                             n_coupled, widest_junction, coupled_lds<Real>(widest_junction), n_coupled);
        // lone junctions with friction: the kernel with the tangential channel (step 4t)
        if (n_friction)
            launch_junctions(&k_bank_modes_coupled_friction<Real>, k_bank_modes_coupled_friction_observed<Real>,
                             FrictionArgs<Real>{B.defl_gain, A.d<FrictionJunctionDev<Real>>(o_friction), A.d<float>(o_approach), A.d<float>(o_travel), A.hd<Real>(o_junction_force), A.hd<Real>(o_tangent),
                                                A.hd<double>(o_compliance), A.hd<uint32_t>(o_status), A.d<Real>(o_anchor_in), A.hd<Real>(o_anchor_out), A.hd<uint32_t>(o_friction_counts)},
                             n_friction, widest_friction, friction_lds<Real>(widest_friction), n_friction);
        // groups, class after class: each class's entries of the device's list follow those of the class before
        const GroupClass<Real> &linear = B.group_class[LINEAR_GROUPS], &hertz = B.group_class[HERTZ_GROUPS], &damped = B.group_class[DAMPED_GROUPS];
        auto groups_from = [&](uint32_t first) {
            return GroupedArgs<Real>{B.defl_gain, A.d<GroupDev<Real>>(o_groups) + first, A.d<float>(o_approach), A.hd<Real>(o_junction_force), A.hd<double>(o_compliance), A.hd<uint32_t>(o_status)};
        };
        launch_junctions(&k_bank_modes_grouped<Real>, k_bank_modes_grouped_observed<Real>, groups_from(0), linear.count(), linear.widest, grouped_lds<Real>(linear.widest), linear.members);
        launch_junctions(k_bank_modes_grouped_mixed<Real>, k_bank_modes_grouped_mixed_observed<Real>, MixedArgs<Real>{groups_from(linear.count()), A.hd<uint32_t>(o_unconverged)}, hertz.count(), hertz.widest,
                         grouped_lds<Real>(hertz.widest), hertz.members);
        launch_junctions(k_bank_modes_grouped_damped<Real>, k_bank_modes_grouped_damped_observed<Real>,
                         DampedGroupArgs<Real>{{groups_from(linear.count() + hertz.count()), A.hd<uint32_t>(o_unconverged)}, d_damping, d_carry_in, carry_out}, damped.count(), damped.widest,
                         grouped_lds<Real>(damped.widest), damped.members);
        if (n_taps) { // the tapped waves' partial rows, in k_bank_modes_read's order; they join read_rows ahead of k_bank_read_rows
            ensure(ctx, B.read_rows, size_t(read_row_count + 1) * frames);
            const ReadArgs<Real> rd{B.defl_gain, A.d<uint32_t>(o_pick_ptr), A.d<PickupDev<Real>>(o_pick_dev), B.read_rows, 0u};
            TimedLaunch timed(ctx, MH_KERNEL_JUNCTION, 0.0);
            k_bank_observe_rows<Real><<<dim3(n_taps, div_up(frames, 32u)), WAVE, 0, st>>>(B.cols(), A.d<WaveDesc>(o_taps), A.d<uint32_t>(o_deal), A.d<uint32_t>(o_count), A.d<uint32_t>(o_chunk_base), d_out_gain,
                                                                                        d_listener, frames, B.tap_states, rd);
            KERNEL_CHECK();
        }
        if (main_waves) {
            uint64_t rendered_modes = 0;
            for (uint32_t d = 0; d < n_dealt; ++d) rendered_modes += r.render_count[d];
            uint64_t driven_modes = 0; // a drive row adds a multiply and an add per mode-sample of its object
            for (uint32_t j = 0; j < n_drives; ++j)
                if (B.drive_dealt[j] >= 0) driven_modes += r.render_count[B.drive_dealt[j]];
            TimedLaunch timed(ctx, MH_KERNEL_BANK, (11.0 * double(rendered_modes) + 2.0 * double(driven_modes) + 4.0 * double(picked_modes)) * double(frames)); // ~11 flop per mode-sample
            // a block without drives launches what it always did; one with drives takes the launch with the many-row loop (and its
            // LDS) only when some object has more rows than the register path holds
            const bool rows_loop = driven_rows && max_imp > IMP_REG;
            if (picks_main) { // a block with pickups some dealt object of the main launch carries: the entry that also reads
                ensure(ctx, B.read_rows, size_t(read_row_count + 1) * frames);
                const ReadArgs<Real> rd{B.defl_gain, A.d<uint32_t>(o_pick_ptr), A.d<PickupDev<Real>>(o_pick_dev), B.read_rows, rows_loop ? 1u : 0u};
                launch_modes(&k_bank_modes_read<Real>, main_waves, WAVE, 0, B.gain_scratch, rd);
            } else {
                launch_modes(rows_loop ? &k_bank_modes_rows<Real> : &k_bank_modes<Real>, main_waves, WAVE, 0, B.gain_scratch);
            }
        }
    } else if (n_renderers) {
        HIP_CHECK(hipMemsetAsync(B.rout.get(), 0, size_t(n_renderers) * frames * sizeof(Real), st));
    }
    if (picks_dealt) { // the pickups' rows, written straight into the pinned arena like everything else the host reads
        k_bank_read_rows<Real><<<dim3(div_up(frames, 256u), n_pickups), 256, 0, st>>>(B.read_rows, A.d<PickupRows>(o_pick_rows), frames, A.hd<Real>(o_pick_out));
        KERNEL_CHECK();
    }
    // out[s] += clicks in impact order, then the renderers in order.  With many impacts in flight the click chain is the
    // same latency problem as a renderer's chunks (1 024 impacts: 100 us as a per-sample loop): it goes through the streaming
    // sum, continuing from what the caller left in the block, and the mix then starts from its result.  That sum, the renderers'
    // sums and the per-object pass are one launch (k_bank_post).
    const uint32_t streamed_clicks = n_impacts > 64 ? n_impacts : 0;
    if (n_dealt || streamed_clicks) {
        constexpr int SW = 16;
        const uint32_t strips = div_up(frames, SW), sum_slices = (n_dealt ? n_renderers : 0) + (streamed_clicks ? 1 : 0);
        const uint32_t object_slices = n_dealt ? div_up(n_dealt, strips * (1024 / WAVE)) : 0;
        ObjectPassArgs<Real> objects{B.cols(), A.d<uint32_t>(o_deal), A.d<uint32_t>(o_count), A.d<uint32_t>(o_chunk_base), A.d<uint32_t>(any_junction ? o_excited : o_imp_ptr), d_out_gain, B.chunk_energy, n_dealt,
                                     A.hd<double>(o_energy), A.hd<uint32_t>(o_live), A.hd<uint8_t>(o_silenced), A.d<uint32_t>(o_tuned), A.hd<double>(o_modal)};
        static PerDeviceOnce attr;
        attr.run(ctx->device, [] { HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bank_post<Real, SW>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); });
        k_bank_post<Real, SW><<<dim3(strips, sum_slices + object_slices), 1024, bank_post_lds<Real, SW>(), st>>>(B.partial, A.d<uint32_t>(o_rcp), n_dealt ? n_renderers : 0, frames, B.rout, B.click, streamed_clicks,
                                                                                        d_out, objects);
        KERNEL_CHECK();
    }
    const uint32_t clicks_in_mix = streamed_clicks ? 0 : n_impacts;
    // ---- the mix, written to the host with the sequence number the host waits for ----
    A.template mix_and_wait<Real>(st, B.click, clicks_in_mix, B.rout, n_renderers, frames, o_out);
    std::copy(A.h<Real>(o_out), A.h<Real>(o_out) + frames, out);
    if (n_dealt) {
        std::copy(A.h<double>(o_energy), A.h<double>(o_energy) + n_dealt, r.object_energy);
        std::copy(A.h<uint32_t>(o_live), A.h<uint32_t>(o_live) + n_dealt, r.object_live);
        std::copy(A.h<uint8_t>(o_silenced), A.h<uint8_t>(o_silenced) + n_dealt, r.object_silenced);
        if (r.object_modal_energy) std::copy(A.h<double>(o_modal), A.h<double>(o_modal) + n_dealt, r.object_modal_energy);
    }
    if (n_pickups) {
        Real *pickup_out = static_cast<Real *>(r.pickup_out);
        if (picks_dealt) std::copy(A.h<Real>(o_pick_out), A.h<Real>(o_pick_out) + size_t(n_pickups) * frames, pickup_out);
        else std::fill(pickup_out, pickup_out + size_t(n_pickups) * frames, Real(0));
    }
    if (n_junctions) { // rows, compliances and statuses of the solved ones; a junction that was left out keeps its zero row
        Real *force_out = static_cast<Real *>(r.force_out);
        std::fill(force_out, force_out + size_t(n_junctions) * frames, Real(0));
        for (const uint32_t j : B.kept_rows) {
            std::copy(A.h<Real>(o_junction_force) + size_t(j) * frames, A.h<Real>(o_junction_force) + size_t(j + 1) * frames, force_out + size_t(j) * frames);
            r.compliance_out[j] = A.h<double>(o_compliance)[j];
            r.status_out[j] = uint8_t(A.h<uint32_t>(o_status)[j]);
        }
        if (admits(Entry::Mixed)) { // a member of a group with a Hertz or a damped member: its frames that failed the residual test; 0 for every other junction
            std::fill(r.unconverged_out, r.unconverged_out + n_junctions, 0u);
            for (const uint32_t j : B.mixed_rows) r.unconverged_out[j] = A.h<uint32_t>(o_unconverged)[j];
        }
        if (admits(Entry::Damped)) { // the carry of a damped junction that was solved; a quiet NaN for every other junction
            Real *carry = static_cast<Real *>(r.carry);
            std::fill(carry, carry + n_junctions, std::numeric_limits<Real>::quiet_NaN());
            for (const uint32_t j : B.kept_rows)
                if ((r.junctions[j].flags & MH_JUNCTION_DAMPED) && r.status_out[j] == MH_JUNCTION_SOLVED) carry[j] = A.h<Real>(o_carry_out)[j];
        }
        if (admits(Entry::Friction)) { // a solved frictional junction: its f_t row, its anchor and its counts; zeros, a quiet NaN and zeros for every other junction
            Real *tangent = static_cast<Real *>(r.tangent_out), *anchor = static_cast<Real *>(r.anchor);
            std::fill(tangent, tangent + size_t(n_junctions) * frames, Real(0));
            std::fill(anchor, anchor + n_junctions, std::numeric_limits<Real>::quiet_NaN());
            std::fill(r.friction_counts_out, r.friction_counts_out + size_t(n_junctions) * 3, 0u);
            for (const uint32_t j : B.friction_rows) {
                if (r.status_out[j] != MH_JUNCTION_SOLVED) continue;
                std::copy(A.h<Real>(o_tangent) + size_t(j) * frames, A.h<Real>(o_tangent) + size_t(j + 1) * frames, tangent + size_t(j) * frames);
                anchor[j] = A.h<Real>(o_anchor_out)[j];
                std::copy(A.h<uint32_t>(o_friction_counts) + 3 * size_t(j), A.h<uint32_t>(o_friction_counts) + 3 * size_t(j + 1), r.friction_counts_out + 3 * size_t(j));
            }
        }
    }
    const ImpactBack<Real> *back = A.h<ImpactBack<Real>>(o_back);
    for (uint32_t i = 0; i < n_impacts; ++i) {
        mh_impact &m = r.impacts[i];
        m.samples_left = back[i].samples_left;
        m.phase_re = double(back[i].phase_re);
        m.phase_im = double(back[i].phase_im);
        m.click_z1 = double(back[i].z1);
        m.click_z2 = double(back[i].z2);
    }
}
} // namespace

struct mh_bank {
    mh_context *ctx;
    bool dbl;
    std::unique_ptr<BankImpl<float>> f;
    std::unique_ptr<BankImpl<double>> d;
};
// f(the bank's implementation), in the bank's precision
template<typename Bank, typename F> static void in_precision(Bank *bank, F &&f) {
    if (bank->dbl) f(*bank->d);
    else f(*bank->f);
}

template<typename Real>
static std::unique_ptr<BankImpl<Real>> make_bank(mh_context *ctx, uint32_t n_objects, uint32_t n_modes, uint32_t n_shapes, const uint32_t *mode_offset,
                                                 const uint32_t *mode_count, const uint32_t *shape_offset, const float *sx, const float *sy, const float *sz) {
    auto B = std::make_unique<BankImpl<Real>>();
    B->ctx = ctx;
    B->n_objects = n_objects;
    B->n_modes = n_modes;
    B->n_shapes = n_shapes;
    for (auto *col : {&B->coeff_re, &B->coeff_im, &B->state_re, &B->state_im, &B->rad_gain, &B->phase_im, &B->phase_re, &B->defl_gain}) {
        col->reset(ctx, std::max<uint32_t>(n_modes, 1));
        col->zero();
    }
    B->shape_x.reset(ctx, std::max<uint32_t>(n_shapes, 1));
    B->shape_y.reset(ctx, std::max<uint32_t>(n_shapes, 1));
    B->shape_z.reset(ctx, std::max<uint32_t>(n_shapes, 1));
    upload_converted(ctx, B->shape_x, 0, sx, n_shapes);
    upload_converted(ctx, B->shape_y, 0, sy, n_shapes);
    upload_converted(ctx, B->shape_z, 0, sz, n_shapes);
    B->mode_offset.reset(ctx, std::max<uint32_t>(n_objects, 1));
    B->mode_count.reset(ctx, std::max<uint32_t>(n_objects, 1));
    B->shape_offset.reset(ctx, std::max<uint32_t>(n_objects, 1));
    if (n_objects) {
        B->mode_offset.upload(mode_offset, n_objects);
        B->mode_count.upload(mode_count, n_objects);
        B->shape_offset.upload(shape_offset, n_objects);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    B->h_mode_count.assign(mode_count, mode_count + n_objects);
    B->h_shape_offset.assign(shape_offset, shape_offset + n_objects);
    return B;
}

extern "C" {
int mh_bank_create(mh_context *ctx, int use_double, uint32_t n_objects, uint32_t n_modes, uint32_t n_shapes, const uint32_t *mode_offset,
                   const uint32_t *mode_count, const uint32_t *shape_offset, const float *shape_x, const float *shape_y, const float *shape_z, mh_bank **out) {
    if (!ctx || !out) return MH_EINVAL;
    *out = nullptr;
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        auto bank = std::make_unique<mh_bank>();
        bank->ctx = ctx;
        bank->dbl = use_double != 0;
        if (bank->dbl) bank->d = make_bank<double>(ctx, n_objects, n_modes, n_shapes, mode_offset, mode_count, shape_offset, shape_x, shape_y, shape_z);
        else bank->f = make_bank<float>(ctx, n_objects, n_modes, n_shapes, mode_offset, mode_count, shape_offset, shape_x, shape_y, shape_z);
        *out = bank.release();
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(ctx, e); }
}
void mh_bank_destroy(mh_bank *b) { delete b; }

int mh_bank_set_coefficients(mh_bank *bank, uint32_t first, uint32_t count, const void *coeff_re, const void *coeff_im, const void *radiation_gain,
                             const void *out_phase_im, const void *out_phase_re) {
    if (!bank || (count && (!coeff_re || !coeff_im || !radiation_gain || !out_phase_im || !out_phase_re))) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(bank->ctx->device));
        auto go = [&](auto &B) {
            using Real = typename std::decay_t<decltype(B)>::Scalar;
            if (size_t(first) + count > B.n_modes) mh_throw(MH_EINVAL, "mode range [%u, %u) outside the bank's %u modes", first, first + count, B.n_modes);
            upload_converted(bank->ctx, B.coeff_re, first, static_cast<const Real *>(coeff_re), count);
            upload_converted(bank->ctx, B.coeff_im, first, static_cast<const Real *>(coeff_im), count);
            upload_converted(bank->ctx, B.rad_gain, first, static_cast<const Real *>(radiation_gain), count);
            upload_converted(bank->ctx, B.phase_im, first, static_cast<const Real *>(out_phase_im), count);
            upload_converted(bank->ctx, B.phase_re, first, static_cast<const Real *>(out_phase_re), count);
        };
        in_precision(bank, go);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(bank->ctx, e); }
}
int mh_bank_set_shapes(mh_bank *bank, uint32_t first, uint32_t count, const float *x, const float *y, const float *z) {
    if (!bank || (count && (!x || !y || !z))) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(bank->ctx->device));
        auto go = [&](auto &B) {
            if (size_t(first) + count > B.n_shapes) mh_throw(MH_EINVAL, "shape range outside the bank");
            upload_converted(bank->ctx, B.shape_x, first, x, count);
            upload_converted(bank->ctx, B.shape_y, first, y, count);
            upload_converted(bank->ctx, B.shape_z, first, z, count);
        };
        in_precision(bank, go);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(bank->ctx, e); }
}
int mh_bank_zero_state(mh_bank *bank, uint32_t first, uint32_t count) {
    if (!bank) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(bank->ctx->device));
        auto go = [&](auto &B) {
            using Real = typename std::decay_t<decltype(B)>::Scalar;
            if (size_t(first) + count > B.n_modes) mh_throw(MH_EINVAL, "mode range outside the bank");
            if (!count) return;
            HIP_CHECK(hipMemsetAsync(B.state_re.get() + first, 0, count * sizeof(Real), bank->ctx->stream));
            HIP_CHECK(hipMemsetAsync(B.state_im.get() + first, 0, count * sizeof(Real), bank->ctx->stream));
            HIP_CHECK(hipStreamSynchronize(bank->ctx->stream));
        };
        in_precision(bank, go);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(bank->ctx, e); }
}
int mh_bank_set_deflection_gain(mh_bank *bank, uint32_t first, uint32_t count, const void *deflection_gain) {
    if (!bank || (count && !deflection_gain)) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(bank->ctx->device));
        auto go = [&](auto &B) {
            using Real = typename std::decay_t<decltype(B)>::Scalar;
            if (size_t(first) + count > B.n_modes) mh_throw(MH_EINVAL, "mode range [%u, %u) outside the bank's %u modes", first, first + count, B.n_modes);
            upload_converted(bank->ctx, B.defl_gain, first, static_cast<const Real *>(deflection_gain), count);
        };
        in_precision(bank, go);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(bank->ctx, e); }
}
// The render entries fill the request; the checks -- of what an entry's level takes first, then of what all share -- and the call are here.
static int render(mh_bank *bank, const RenderRequest &r) {
    if (r.entry >= Entry::Damped && r.n_junctions && (!r.damping || !r.carry)) return MH_EINVAL;
    if (r.entry >= Entry::Mixed && r.n_junctions && !r.unconverged_out) return MH_EINVAL;
    if (r.unconverged_out) std::fill(r.unconverged_out, r.unconverged_out + r.n_junctions, 0u); // (0 whatever becomes of the call)
    if (r.entry >= Entry::Friction && r.n_junctions) {
        if (!r.junctions || !r.tangent_out || !r.anchor || !r.friction_counts_out) return MH_EINVAL;
        for (uint32_t j = 0; j < r.n_junctions; ++j) // friction[j] and travel row j are read for flagged junctions only
            if ((r.junctions[j].flags & MH_JUNCTION_FRICTION) && (!r.friction || !r.travel)) return MH_EINVAL;
        std::fill(r.friction_counts_out, r.friction_counts_out + size_t(r.n_junctions) * 3, 0u);
    }
    if (!bank || !r.out || (r.n_impacts && !r.impacts) || (r.n_renderers && !r.deal_offset) || !r.out_gain || !r.listener_gain || (r.n_drives && (!r.drives || !r.signals))) return MH_EINVAL;
    if (r.n_pickups && (!r.pickups || !r.pickup_out || !r.pickup_read)) return MH_EINVAL;
    if (r.n_junctions && (!r.junctions || !r.approach || !r.force_out || !r.compliance_out || !r.status_out)) return MH_EINVAL;
    if (r.n_renderers && r.deal_offset[r.n_renderers] && (!r.deal_objects || !r.render_count || !r.tuned_count || !r.object_energy || !r.object_live || !r.object_silenced)) return MH_EINVAL;
    if (r.frames == 0) return MH_OK;
    try {
        MhSharedPhase not_during_a_factorisation(bank->ctx->device); // a solve's dense coarse factorisation runs alone on the device (mh_eigs.hip)
        HIP_CHECK(hipSetDevice(bank->ctx->device));
        in_precision(bank, [&](auto &B) { render_impl(B, r); });
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(bank->ctx, e); }
}
int mh_bank_render(mh_bank *bank, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts, uint32_t n_renderers, const uint32_t *deal_offset,
                   const uint32_t *deal_objects, const uint32_t *render_count, const uint32_t *tuned_count, const float *out_gain, const float *listener_gain,
                   void *out, double *object_energy, uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy) {
    return render(bank, {Entry::Coupled, frames, click_gain, n_impacts, impacts, n_renderers, deal_offset, deal_objects, render_count, tuned_count, out_gain, listener_gain, out, object_energy,
                         object_live, object_silenced, object_modal_energy});
}
int mh_bank_render_driven(mh_bank *bank, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts, uint32_t n_renderers, const uint32_t *deal_offset,
                          const uint32_t *deal_objects, const uint32_t *render_count, const uint32_t *tuned_count, const float *out_gain, const float *listener_gain,
                          void *out, double *object_energy, uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                          const mh_drive *drives, const float *signals) {
    return render(bank, {Entry::Coupled, frames, click_gain, n_impacts, impacts, n_renderers, deal_offset, deal_objects, render_count, tuned_count, out_gain, listener_gain, out, object_energy,
                         object_live, object_silenced, object_modal_energy, n_drives, drives, signals});
}
int mh_bank_render_read(mh_bank *bank, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts, uint32_t n_renderers, const uint32_t *deal_offset,
                        const uint32_t *deal_objects, const uint32_t *render_count, const uint32_t *tuned_count, const float *out_gain, const float *listener_gain,
                        void *out, double *object_energy, uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                        const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out, uint8_t *pickup_read) {
    return render(bank, {Entry::Coupled, frames, click_gain, n_impacts, impacts, n_renderers, deal_offset, deal_objects, render_count, tuned_count, out_gain, listener_gain, out, object_energy,
                         object_live, object_silenced, object_modal_energy, n_drives, drives, signals, n_pickups, pickups, pickup_out, pickup_read});
}
int mh_bank_render_coupled(mh_bank *bank, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts, uint32_t n_renderers, const uint32_t *deal_offset,
                           const uint32_t *deal_objects, const uint32_t *render_count, const uint32_t *tuned_count, const float *out_gain, const float *listener_gain,
                           void *out, double *object_energy, uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                           const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out, uint8_t *pickup_read,
                           uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out, double *compliance_out, uint8_t *status_out) {
    return render(bank, {Entry::Coupled, frames, click_gain, n_impacts, impacts, n_renderers, deal_offset, deal_objects, render_count, tuned_count, out_gain, listener_gain, out, object_energy,
                         object_live, object_silenced, object_modal_energy, n_drives, drives, signals, n_pickups, pickups, pickup_out, pickup_read, n_junctions, junctions, approach, force_out,
                         compliance_out, status_out});
}
int mh_bank_render_damped(mh_bank *bank, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts, uint32_t n_renderers, const uint32_t *deal_offset,
                          const uint32_t *deal_objects, const uint32_t *render_count, const uint32_t *tuned_count, const float *out_gain, const float *listener_gain,
                          void *out, double *object_energy, uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                          const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out, uint8_t *pickup_read,
                          uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out, double *compliance_out, uint8_t *status_out,
                          const float *damping, void *carry) {
    return render(bank, {Entry::Damped, frames, click_gain, n_impacts, impacts, n_renderers, deal_offset, deal_objects, render_count, tuned_count, out_gain, listener_gain, out, object_energy,
                         object_live, object_silenced, object_modal_energy, n_drives, drives, signals, n_pickups, pickups, pickup_out, pickup_read, n_junctions, junctions, approach, force_out,
                         compliance_out, status_out, damping, carry});
}
int mh_bank_render_observed(mh_bank *bank, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts, uint32_t n_renderers, const uint32_t *deal_offset,
                            const uint32_t *deal_objects, const uint32_t *render_count, const uint32_t *tuned_count, const float *out_gain, const float *listener_gain,
                            void *out, double *object_energy, uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                            const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out, uint8_t *pickup_read,
                            uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out, double *compliance_out, uint8_t *status_out,
                            const float *damping, void *carry) {
    return render(bank, {Entry::Observed, frames, click_gain, n_impacts, impacts, n_renderers, deal_offset, deal_objects, render_count, tuned_count, out_gain, listener_gain, out, object_energy,
                         object_live, object_silenced, object_modal_energy, n_drives, drives, signals, n_pickups, pickups, pickup_out, pickup_read, n_junctions, junctions, approach, force_out,
                         compliance_out, status_out, damping, carry});
}
int mh_bank_render_mixed(mh_bank *bank, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts, uint32_t n_renderers, const uint32_t *deal_offset,
                         const uint32_t *deal_objects, const uint32_t *render_count, const uint32_t *tuned_count, const float *out_gain, const float *listener_gain,
                         void *out, double *object_energy, uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                         const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out, uint8_t *pickup_read,
                         uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out, double *compliance_out, uint8_t *status_out,
                         const float *damping, void *carry, uint32_t *unconverged_out) {
    return render(bank, {Entry::Mixed, frames, click_gain, n_impacts, impacts, n_renderers, deal_offset, deal_objects, render_count, tuned_count, out_gain, listener_gain, out, object_energy,
                         object_live, object_silenced, object_modal_energy, n_drives, drives, signals, n_pickups, pickups, pickup_out, pickup_read, n_junctions, junctions, approach, force_out,
                         compliance_out, status_out, damping, carry, unconverged_out});
}
int mh_bank_render_damped_groups(mh_bank *bank, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts, uint32_t n_renderers, const uint32_t *deal_offset,
                                 const uint32_t *deal_objects, const uint32_t *render_count, const uint32_t *tuned_count, const float *out_gain, const float *listener_gain,
                                 void *out, double *object_energy, uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                                 const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out, uint8_t *pickup_read,
                                 uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out, double *compliance_out, uint8_t *status_out,
                                 const float *damping, void *carry, uint32_t *unconverged_out) {
    return render(bank, {Entry::DampedGroups, frames, click_gain, n_impacts, impacts, n_renderers, deal_offset, deal_objects, render_count, tuned_count, out_gain, listener_gain, out, object_energy,
                         object_live, object_silenced, object_modal_energy, n_drives, drives, signals, n_pickups, pickups, pickup_out, pickup_read, n_junctions, junctions, approach, force_out,
                         compliance_out, status_out, damping, carry, unconverged_out});
}
int mh_bank_render_friction(mh_bank *bank, uint32_t frames, float click_gain, uint32_t n_impacts, mh_impact *impacts, uint32_t n_renderers, const uint32_t *deal_offset,
                            const uint32_t *deal_objects, const uint32_t *render_count, const uint32_t *tuned_count, const float *out_gain, const float *listener_gain,
                            void *out, double *object_energy, uint32_t *object_live, uint8_t *object_silenced, double *object_modal_energy, uint32_t n_drives,
                            const mh_drive *drives, const float *signals, uint32_t n_pickups, const mh_pickup *pickups, void *pickup_out, uint8_t *pickup_read,
                            uint32_t n_junctions, const mh_junction *junctions, const float *approach, void *force_out, double *compliance_out, uint8_t *status_out,
                            const float *damping, void *carry, uint32_t *unconverged_out, const mh_friction *friction, const float *travel, void *tangent_out, void *anchor,
                            uint32_t *friction_counts_out) {
    return render(bank, {Entry::Friction, frames, click_gain, n_impacts, impacts, n_renderers, deal_offset, deal_objects, render_count, tuned_count, out_gain, listener_gain, out, object_energy,
                         object_live, object_silenced, object_modal_energy, n_drives, drives, signals, n_pickups, pickups, pickup_out, pickup_read, n_junctions, junctions, approach, force_out,
                         compliance_out, status_out, damping, carry, unconverged_out, friction, travel, tangent_out, anchor, friction_counts_out});
}
uint32_t mh_friction_struct_size(void) { return uint32_t(sizeof(mh_friction)); }
uint32_t mh_drive_struct_size(void) { return uint32_t(sizeof(mh_drive)); }
uint32_t mh_pickup_struct_size(void) { return uint32_t(sizeof(mh_pickup)); }
uint32_t mh_junction_struct_size(void) { return uint32_t(sizeof(mh_junction)); }
int mh_bank_read_state(const mh_bank *bank, uint32_t first, uint32_t count, double *state_re, double *state_im) {
    if (!bank || (count && (!state_re || !state_im))) return MH_EINVAL;
    try {
        HIP_CHECK(hipSetDevice(bank->ctx->device));
        auto go = [&](auto &B) {
            using Real = typename std::decay_t<decltype(B)>::Scalar;
            if (size_t(first) + count > B.n_modes) mh_throw(MH_EINVAL, "mode range outside the bank");
            std::vector<Real> re(count), im(count);
            if (!count) return;
            HIP_CHECK(hipMemcpyAsync(re.data(), B.state_re.get() + first, count * sizeof(Real), hipMemcpyDeviceToHost, bank->ctx->stream));
            HIP_CHECK(hipMemcpyAsync(im.data(), B.state_im.get() + first, count * sizeof(Real), hipMemcpyDeviceToHost, bank->ctx->stream));
            HIP_CHECK(hipStreamSynchronize(bank->ctx->stream));
            for (uint32_t i = 0; i < count; ++i) { state_re[i] = double(re[i]); state_im[i] = double(im[i]); }
        };
        in_precision(bank, go);
        return MH_OK;
    } catch (const std::exception &e) { return mh_guard(bank->ctx, e); }
}
}
