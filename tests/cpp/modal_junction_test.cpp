// Contact junctions through the mirrored API (ModalJunction / RenderModalCoupled, modal/bank.hpp), included the way a caller of the
// reference includes the bank (<audio/ModalAudio.h>): without junctions the call is RenderModalRead bit for bit, a junction of stiffness 0
// observes (no force, and the block is the one with a silent drive in its place), a closed contact pushes back and never pulls, and what
// cannot be solved is left out with a row of zeros.  Compiles and links without a GPU; runs on one.
#include "harness.hpp"

#include <audio/ModalAudio.h>

#include <algorithm>
#include <cmath>
#include <span>

namespace {
constexpr float kRate = 48'000.f;
constexpr uint32_t kBlock = 512, kPoints = 4;

// The synthetic body of the render tests (tests/cpp/modal_pickup_test.cpp).
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

std::vector<float> Scrape(uint32_t blocks) {
    std::vector<float> f(size_t(blocks) * kBlock);
    uint32_t lcg = 4321u;
    for (size_t s = 0; s < f.size(); ++s) {
        lcg = lcg * 1664525u + 1013904223u;
        f[s] = 0.6f * std::sin(float(s) * 0.013f) + 0.4f * (float(lcg >> 8) / float(1u << 24) - 0.5f);
    }
    return f;
}

template<typename Audio, typename Bank, typename Sample> struct RigT {
    Audio Engine;
    RigT(uint32_t bodies, uint32_t n_modes) {
        const ModalModes body = LadderModes(n_modes, 0.3f);
        Bank building;
        building.SampleRate = kRate;
        for (uint32_t i = 0; i < bodies; ++i) {
            const uint32_t slot = AddModalObject(building, entt::entity{i}, body);
            TuneModalObject(building, slot, body.Freqs, body.T60s);
            building.OutGain[slot] = 1;
        }
        InstallModalBank(Engine, building);
    }
    struct Result {
        std::vector<Sample> Signal, Forces;
        std::vector<double> Compliances;
        std::vector<uint8_t> Statuses;
    };
    // `blocks` blocks: body 0 driven in every one (plus `extra` drives), the junctions passed with an approach that rises and falls.
    // which: 0 = RenderModalRead, 1 = RenderModalCoupled.
    Result Run(uint32_t blocks, std::span<const ModalJunction> junctions, int which, std::vector<ModalDrive> extra = {}) {
        std::vector<ModalDrive> drives{{0, 2, 0.5f, -0.25f, 1.f}};
        drives.insert(drives.end(), extra.begin(), extra.end());
        const std::vector<float> force = Scrape(blocks);
        Result r;
        r.Signal.assign(size_t(blocks) * kBlock, Sample(0));
        r.Compliances.assign(junctions.size(), 0.0);
        r.Statuses.assign(junctions.size(), 0);
        std::vector<Sample> rows(junctions.size() * kBlock);
        std::vector<float> signals(drives.size() * kBlock, 0.f), approach(junctions.size() * kBlock);
        for (uint32_t i = 0; i < blocks; ++i) {
            std::copy(force.begin() + size_t(i) * kBlock, force.begin() + size_t(i + 1) * kBlock, signals.begin()); // the extra drives stay silent
            for (size_t j = 0; j < junctions.size(); ++j)
                for (uint32_t s = 0; s < kBlock; ++s) approach[j * kBlock + s] = 1e-4f * std::sin(float(i * kBlock + s) * 0.004f);
            Sample *out = r.Signal.data() + size_t(i) * kBlock;
            if (which == 0) RenderModalRead(Engine, drives, signals.data(), {}, static_cast<Sample *>(nullptr), out, kBlock);
            else RenderModalCoupled(Engine, drives, signals.data(), {}, static_cast<Sample *>(nullptr), junctions, approach.data(), rows.data(), out, kBlock, nullptr,
                                    r.Compliances.data(), r.Statuses.data());
            r.Forces.insert(r.Forces.end(), rows.begin(), rows.end());
        }
        return r;
    }
};
using Rig = RigT<ModalAudio, ModalBank, float>;
using Rig64 = RigT<ModalAudio64, ModalBank64, double>;

ModalJunctionSide At(uint32_t object, uint32_t point, float sign = 1.f) {
    ModalJunctionSide s;
    s.Object = object, s.Points[0] = s.Points[1] = s.Points[2] = point, s.Nx = 0.25f * sign, s.Ny = -1.f * sign, s.Nz = 0.5f * sign, s.Coupling = 2.f;
    return s;
}
ModalJunction Between(ModalJunctionSide a, ModalJunctionSide b, float stiffness, uint32_t flags = 0) {
    ModalJunction j;
    j.A = a, j.B = b, j.Stiffness = stiffness, j.Flags = flags;
    return j;
}
template<typename Audio> bool SameBank(Audio &a, Audio &b) {
    SyncModalState(a);
    SyncModalState(b);
    return LiveBank(a).StateRe == LiveBank(b).StateRe && LiveBank(a).StateIm == LiveBank(b).StateIm && LiveBank(a).LiveModeCount == LiveBank(b).LiveModeCount &&
           LiveBank(a).Ringing == LiveBank(b).Ringing;
}

template<typename R> void NoJunctionNoChange() {
    R plain{2, 130}, coupled{2, 130};
    const auto a = plain.Run(6, {}, 0), b = coupled.Run(6, {}, 1);
    EXPECT(*std::max_element(a.Signal.begin(), a.Signal.end()) > 0);
    EXPECT(a.Signal == b.Signal);
    EXPECT(SameBank(plain.Engine, coupled.Engine));
}

template<typename R> void ADeadJunctionObserves() {
    // stiffness 0 between bodies 0 and 1, against silent drives at the two contact points in its place
    const std::vector<ModalJunction> contact{Between(At(0, 1), At(1, 3, -1.f), 0.f)};
    R silent{3, 130}, coupled{3, 130};
    const auto a = silent.Run(6, {}, 0, {{0, 1, 0.25f, -1.f, 0.5f}, {1, 3, -0.25f, 1.f, -0.5f}}), b = coupled.Run(6, contact, 1);
    EXPECT(b.Statuses == std::vector<uint8_t>{1});
    EXPECT(std::all_of(b.Forces.begin(), b.Forces.end(), [](auto v) { return v == 0; }));
    EXPECT(a.Signal == b.Signal);
    EXPECT(SameBank(silent.Engine, coupled.Engine));
}
} // namespace

CASE(without_junctions_the_coupled_render_is_the_read_render) { NoJunctionNoChange<Rig>(); }
CASE(without_junctions_the_coupled_render_is_the_read_render_in_double) { NoJunctionNoChange<Rig64>(); }
CASE(a_junction_of_stiffness_zero_observes) { ADeadJunctionObserves<Rig>(); }
CASE(a_junction_of_stiffness_zero_observes_in_double) { ADeadJunctionObserves<Rig64>(); }

CASE(a_closed_contact_pushes_back_and_never_pulls) {
    Rig rig{2, 130};
    const std::vector<ModalJunction> probe{Between(At(0, 1), ModalJunctionSide{}, 0.f)};
    const double c = rig.Run(1, probe, 1).Compliances[0];
    EXPECT(c > 0);
    Rig free{2, 130}, held{2, 130};
    const std::vector<ModalJunction> contact{Between(At(0, 1), ModalJunctionSide{}, float(10.0 / c))}; // K C = 10
    const auto a = free.Run(4, probe, 1), b = held.Run(4, contact, 1);
    EXPECT(b.Statuses == std::vector<uint8_t>{1});
    EXPECT(std::all_of(b.Forces.begin(), b.Forces.end(), [](float v) { return v >= 0 && std::isfinite(v); }));
    const size_t pressed = size_t(std::count_if(b.Forces.begin(), b.Forces.end(), [](float v) { return v > 0; }));
    EXPECT_NOTE(pressed > b.Forces.size() / 10 && pressed < b.Forces.size() * 9 / 10, std::to_string(pressed));
    EXPECT(a.Signal != b.Signal);
}

CASE(what_cannot_be_solved_is_left_out_with_a_row_of_zeros) {
    ModalJunctionSide not_finite = At(1, 0);
    not_finite.Ny = std::nanf("");
    const std::vector<ModalJunction> contacts{Between(At(7, 0), ModalJunctionSide{}, 1.f), Between(At(0, 1), ModalJunctionSide{}, 1e3f), Between(At(1, kPoints), ModalJunctionSide{}, 1.f),
                                              Between(not_finite, ModalJunctionSide{}, 1.f), Between(At(1, 0), At(1, 2), 1.f), Between(At(1, 0), ModalJunctionSide{}, -1.f),
                                              Between(At(0, 2), At(1, 2), 1.f)}; // (the last: body 0 is already on the second junction)
    Rig rig{2, 64};
    const auto r = rig.Run(2, contacts, 1);
    EXPECT(r.Statuses == (std::vector<uint8_t>{0, 1, 0, 0, 0, 0, 0}));
    for (uint32_t i = 0; i < 2; ++i)
        for (uint32_t q = 0; q < contacts.size(); ++q) {
            const float *row = r.Forces.data() + (size_t(i) * contacts.size() + q) * kBlock;
            const bool silent = std::all_of(row, row + kBlock, [](float v) { return v == 0; });
            EXPECT(silent == (q != 1));
        }
}

int main() { return check::run_all(); }
