// Deflection pickups through the mirrored API (ModalPickup / RenderModalRead, modal/bank.hpp), included the way a caller of the
// reference includes the bank (<audio/ModalAudio.h>): a pickup observes (the block with pickups is, bit for bit, the block without
// them), a blend of three points reads the weighted sum of the three points' rows, and what cannot be read is left out with a row of
// zeros.  Compiles and links without a GPU; runs on one.
#include "harness.hpp"

#include <audio/ModalAudio.h>

#include <algorithm>
#include <cmath>
#include <span>

namespace {
constexpr float kRate = 48'000.f;
constexpr uint32_t kBlock = 512, kPoints = 4;

// The synthetic body of the render tests: 40 Hz x 1.031 x ordinal, decay times slowest / ordinal, trigonometric shapes
// of amplitude 0.01 on a zig-zag strip of four sample points.
ModalModes LadderModes(uint32_t n_modes, float slowest) {
    ModalModes body;
    body.Freqs.resize(n_modes);
    body.T60s.resize(n_modes);
    for (uint32_t k = 0; k < n_modes; ++k) {
        body.Freqs[k] = 40.f * float(k + 1) * 1.031f;
        body.T60s[k] = slowest / float(k + 1);
    }
    for (uint32_t p = 0; p < kPoints; ++p) {
        body.Positions.push_back({float(p) * 0.01f, 0.f, (p & 1u) ? 0.02f : 0.f});
        if (p >= 2) body.Indices.insert(body.Indices.end(), {p - 2, p - 1, p});
        auto &row = body.Shapes.emplace_back(n_modes);
        for (uint32_t k = 0; k < n_modes; ++k) {
            const float phase = float(k + 1) * 0.37f + float(p);
            row[k] = vec3{std::sin(phase), std::cos(phase * 1.7f), std::sin(phase * 2.3f)} * 0.01f;
        }
    }
    return body;
}

// A deterministic force signal: two tones and noise.
std::vector<float> Scrape(uint32_t voice, uint32_t blocks) {
    std::vector<float> f(size_t(blocks) * kBlock);
    uint32_t lcg = 4321u + 977u * voice;
    for (size_t s = 0; s < f.size(); ++s) {
        lcg = lcg * 1664525u + 1013904223u;
        f[s] = 0.6f * std::sin(float(s) * (0.013f + 0.004f * float(voice))) + 0.4f * (float(lcg >> 8) / float(1u << 24) - 0.5f);
    }
    return f;
}

template<typename Audio, typename Bank, typename Sample> struct RigT {
    Audio Engine;
    RigT(uint32_t bodies, uint32_t n_modes, uint32_t renderers) {
        const ModalModes body = LadderModes(n_modes, 0.3f);
        Engine.RenderPool.SetSize(renderers);
        Bank building;
        building.SampleRate = kRate;
        for (uint32_t i = 0; i < bodies; ++i) {
            const uint32_t slot = AddModalObject(building, entt::entity{i}, body);
            TuneModalObject(building, slot, body.Freqs, body.T60s);
            building.OutGain[slot] = 1;
        }
        InstallModalBank(Engine, building);
    }
    // `blocks` blocks: body 0 struck in the first and driven in every one, body 1 struck only.  Returns the signal; `reads` receives
    // every block's pickup rows, block after block, `flags` the last block's.
    std::vector<Sample> Run(uint32_t blocks, std::span<const ModalPickup> pickups, std::vector<Sample> *reads, std::vector<uint8_t> *flags, bool through_read) {
        for (uint32_t o = 0; o < 2; ++o) {
            ModalEvent e;
            e.Object = o, e.ExPos = o, e.Jx = 1.f, e.Jy = 0.5f, e.PulseStep = 1.f / 300.f, e.PulseGamma = 20.f;
            EnqueueModalEvent(Engine, e);
        }
        const std::vector<ModalDrive> drives{{0, 2, 0.5f, -0.25f, 1.f}};
        const std::vector<float> force = Scrape(0, blocks);
        std::vector<Sample> signal(size_t(blocks) * kBlock, Sample(0)), rows(pickups.size() * kBlock);
        std::vector<uint8_t> read(pickups.size());
        for (uint32_t i = 0; i < blocks; ++i) {
            Sample *out = signal.data() + size_t(i) * kBlock;
            if (through_read) RenderModalRead(Engine, drives, force.data() + size_t(i) * kBlock, pickups, rows.data(), out, kBlock, read.data());
            else RenderModalDriven(Engine, drives, force.data() + size_t(i) * kBlock, out, kBlock);
            if (reads) reads->insert(reads->end(), rows.begin(), rows.end());
        }
        if (flags) *flags = read;
        return signal;
    }
};
using Rig = RigT<ModalAudio, ModalBank, float>;
using Rig64 = RigT<ModalAudio64, ModalBank64, double>;

ModalPickup At(uint32_t object, uint32_t point, uint32_t advance = 0) {
    ModalPickup p;
    p.Object = object, p.Points[0] = p.Points[1] = p.Points[2] = point, p.Nx = 0.25f, p.Ny = -1.f, p.Nz = 0.5f, p.Coupling = 2.f, p.Advance = advance;
    return p;
}

template<typename R, typename Sample> void PickupsObserve() {
    std::vector<ModalPickup> probes;
    for (uint32_t o = 0; o < 2; ++o)
        for (uint32_t i = 0; i < 10; ++i) probes.push_back(At(o, i % kPoints, i % 3)); // ten per object: beyond the per-object cap
    R plain{2, 130, 1}, watched{2, 130, 1};
    std::vector<Sample> rows;
    const auto a = plain.Run(6, {}, nullptr, nullptr, false), b = watched.Run(6, probes, &rows, nullptr, true);
    EXPECT(*std::max_element(a.begin(), a.end()) > 0);
    EXPECT(a == b);
    SyncModalState(plain.Engine);
    SyncModalState(watched.Engine);
    EXPECT(LiveBank(plain.Engine).StateRe == LiveBank(watched.Engine).StateRe && LiveBank(plain.Engine).StateIm == LiveBank(watched.Engine).StateIm);
    EXPECT(LiveBank(plain.Engine).LiveModeCount == LiveBank(watched.Engine).LiveModeCount);
    EXPECT(std::any_of(rows.begin(), rows.end(), [](Sample v) { return v != 0; }));
}
} // namespace

CASE(pickups_change_nothing_they_observe) { PickupsObserve<Rig, float>(); }
CASE(pickups_change_nothing_they_observe_in_double) { PickupsObserve<Rig64, double>(); }

CASE(a_blend_reads_the_weighted_sum_of_its_points) {
    ModalPickup blend = At(0, 3, 1);
    blend.Points[1] = 0, blend.Points[2] = 1;
    blend.Weights[0] = 0.5f, blend.Weights[1] = 0.25f, blend.Weights[2] = 0.25f;
    const std::vector<ModalPickup> probes{blend, At(0, 3, 1), At(0, 0, 1), At(0, 1, 1)};
    Rig rig{2, 130, 1};
    std::vector<float> rows;
    std::vector<uint8_t> flags;
    rig.Run(4, probes, &rows, &flags, true);
    EXPECT(flags == std::vector<uint8_t>(4, 1));
    double peak = 0, gap = 0;
    for (uint32_t i = 0; i < 4; ++i)
        for (uint32_t s = 0; s < kBlock; ++s) {
            const float *r = rows.data() + size_t(i) * 4 * kBlock + s;
            peak = std::max(peak, std::abs(double(r[0])));
            gap = std::max(gap, std::abs(double(r[0]) - (0.5 * r[kBlock] + 0.25 * r[2 * kBlock] + 0.25 * r[3 * kBlock])));
        }
    EXPECT(peak > 0);
    EXPECT_NOTE(gap <= 1e-5 * peak, std::to_string(gap / peak));
}

CASE(what_cannot_be_read_is_left_out_with_a_row_of_zeros) {
    ModalPickup no_object = At(7, 0), no_point = At(0, kPoints), late = At(0, 0, 3), not_finite = At(0, 0);
    not_finite.Ny = std::nanf("");
    const std::vector<ModalPickup> probes{no_object, At(0, 1), no_point, late, not_finite};
    Rig rig{2, 64, 1};
    std::vector<float> rows;
    std::vector<uint8_t> flags;
    rig.Run(2, probes, &rows, &flags, true);
    EXPECT(flags == (std::vector<uint8_t>{0, 1, 0, 0, 0}));
    for (uint32_t i = 0; i < 2; ++i)
        for (uint32_t q = 0; q < 5; ++q) {
            const float *r = rows.data() + (size_t(i) * 5 + q) * kBlock;
            const bool silent = std::all_of(r, r + kBlock, [](float v) { return v == 0; });
            EXPECT(silent == (q != 1));
        }
}

int main() { return check::run_all(); }
