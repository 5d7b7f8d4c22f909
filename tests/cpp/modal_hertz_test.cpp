// Hertz junctions through the mirrored API (ModalJunctionHertz / RenderModalCoupled, modal/bank.hpp), included the way a caller of the
// reference includes the bank (<audio/ModalAudio.h>): the force row of a Hertz junction never pulls and obeys f = K max(u - read1, 0)^1.5
// against advance-1 pickups on a twin bank the row is replayed into as a drive, and Hertz together with bilateral is left out.  Compiles and
// links without a GPU; runs on one.
#include "harness.hpp"

#include <audio/ModalAudio.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <span>

static_assert(ModalJunctionHertz == 2u && ModalJunctionBilateral == 1u, "the flag bits of modalhip.h (MH_JUNCTION_HERTZ, MH_JUNCTION_BILATERAL)");

namespace {
constexpr float kRate = 48'000.f;
constexpr uint32_t kBlock = 512, kPoints = 4, kModes = 130, kRingUp = 3, kCoupled = 4;

// The synthetic body of the render tests (tests/cpp/modal_junction_test.cpp).
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

constexpr uint32_t kPoint = 1;
constexpr float kNormal[3] = {0.25f, -1.f, 0.5f}, kCoupling = 2.f;

// Two bodies; body 0 is rung up by a drive for kRingUp blocks and then left to itself: in the coupled blocks it carries no other row, so
// the force row replayed as a drive at the junction's point along its direction gives the coupled run's state bit for bit (a junction
// side with weights {1, 0, 0} has a drive's gain).
struct Rig {
    ModalAudio Engine;
    Rig() {
        const ModalModes body = LadderModes(kModes, 0.3f);
        ModalBank building;
        building.SampleRate = kRate;
        for (uint32_t i = 0; i < 2; ++i) {
            const uint32_t slot = AddModalObject(building, entt::entity{i}, body);
            TuneModalObject(building, slot, body.Freqs, body.T60s);
            building.OutGain[slot] = 1;
        }
        InstallModalBank(Engine, building);
        const std::vector<ModalDrive> drives{{0, 2, 0.5f, -0.25f, 1.f}};
        const std::vector<float> force = Scrape(kRingUp);
        std::vector<float> out(kBlock);
        for (uint32_t i = 0; i < kRingUp; ++i) RenderModalRead(Engine, drives, force.data() + size_t(i) * kBlock, {}, static_cast<float *>(nullptr), out.data(), kBlock);
    }
    static ModalPickup Probe() {
        ModalPickup p;
        p.Object = 0, p.Points[0] = p.Points[1] = p.Points[2] = kPoint, p.Nx = kNormal[0], p.Ny = kNormal[1], p.Nz = kNormal[2], p.Coupling = kCoupling, p.Advance = 1;
        return p;
    }
    // One block with `force` (nullable) as a drive at the junction's point along its direction; returns the advance-1 pickup's row.
    std::vector<float> Replay(const float *force, std::vector<float> &out) {
        const std::vector<ModalDrive> drives{{0, kPoint, kNormal[0], kNormal[1], kNormal[2]}};
        const std::vector<float> silent(kBlock, 0.f);
        const std::vector<ModalPickup> pickups{Probe()};
        std::vector<float> reads(kBlock);
        uint8_t flag = 0;
        out.assign(kBlock, 0.f);
        RenderModalRead(Engine, drives, force ? force : silent.data(), pickups, reads.data(), out.data(), kBlock, &flag);
        EXPECT(flag == 1);
        return reads;
    }
};

ModalJunction Contact(float stiffness, uint32_t flags) {
    ModalJunction j;
    j.A.Object = 0, j.A.Points[0] = j.A.Points[1] = j.A.Points[2] = kPoint, j.A.Nx = kNormal[0], j.A.Ny = kNormal[1], j.A.Nz = kNormal[2], j.A.Coupling = kCoupling;
    j.Stiffness = stiffness, j.Flags = flags;
    return j;
}

struct Coupled {
    std::vector<float> Forces, Out;
    double Compliance{0};
    uint8_t Status{0};
};
Coupled RunCoupled(Rig &rig, const ModalJunction &junction, const float *approach) {
    Coupled r;
    r.Forces.assign(kBlock, 0.f);
    r.Out.assign(kBlock, 0.f);
    RenderModalCoupled(rig.Engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), std::span<const ModalJunction>(&junction, 1), approach, r.Forces.data(),
                       r.Out.data(), kBlock, nullptr, &r.Compliance, &r.Status);
    return r;
}
bool SameBank(ModalAudio &a, ModalAudio &b) {
    SyncModalState(a);
    SyncModalState(b);
    return LiveBank(a).StateRe == LiveBank(b).StateRe && LiveBank(a).StateIm == LiveBank(b).StateIm;
}
} // namespace

CASE(a_hertz_contact_never_pulls_and_meets_its_law_in_a_replay) {
    // the size of the free deflection at the contact point, and C, from a scout
    Rig scout;
    std::vector<float> out;
    const std::vector<float> free_read = scout.Replay(nullptr, out);
    float x0 = 0;
    for (float v : free_read) x0 = std::max(x0, std::fabs(v));
    EXPECT(x0 > 0);
    const std::vector<float> still(kBlock, 0.f);
    const Coupled probe = RunCoupled(scout, Contact(0.f, ModalJunctionHertz), still.data());
    EXPECT(probe.Status == 1 && probe.Compliance > 0);
    const float stiffness = float(3.0 / (probe.Compliance * std::sqrt(double(x0)))); // K C sqrt(x0) = 3
    const ModalJunction hertz = Contact(stiffness, ModalJunctionHertz), linear = Contact(stiffness, 0);

    Rig a, b, c;
    EXPECT(SameBank(a.Engine, b.Engine));
    size_t pressed = 0, differing = 0;
    double worst = 0, peak = 0;
    std::vector<float> approach(kBlock);
    std::vector<double> law;
    std::vector<float> all_forces;
    for (uint32_t i = 0; i < kCoupled; ++i) {
        for (uint32_t s = 0; s < kBlock; ++s) approach[s] = x0 * (std::sin(float(i * kBlock + s) * 0.016f) + 0.1f);
        const Coupled got = RunCoupled(a, hertz, approach.data()), other = RunCoupled(c, linear, approach.data());
        EXPECT(got.Status == 1 && other.Status == 1);
        const std::vector<float> read1 = b.Replay(got.Forces.data(), out);
        EXPECT(out == got.Out);
        EXPECT(SameBank(a.Engine, b.Engine));
        for (uint32_t s = 0; s < kBlock; ++s) {
            const double f = got.Forces[s], y = std::max(double(approach[s]) - double(read1[s]), 0.0);
            EXPECT(f >= 0 && std::isfinite(f));
            pressed += f > 0;
            differing += got.Forces[s] != other.Forces[s];
            law.push_back(double(stiffness) * y * std::sqrt(y));
            all_forces.push_back(got.Forces[s]);
            peak = std::max(peak, f);
        }
    }
    for (size_t s = 0; s < law.size(); ++s) worst = std::max(worst, std::fabs(double(all_forces[s]) - law[s]));
    const size_t frames = size_t(kCoupled) * kBlock;
    EXPECT_NOTE(pressed > frames / 20 && pressed < frames * 19 / 20, std::to_string(pressed));
    EXPECT_NOTE(differing > frames / 20, std::to_string(differing)); // the flag selects another law
    // f = K y^1.5 with y = u - read1: a rounding dy of the pickup's 130-term float sum (at most 130 eps of |u| + |d| <= 4 y_max here: the
    // contact gives way by the factor 1 + K C sqrt(y) <= 4) moves the law by 1.5 K sqrt(y) dy, that is by 1.5 * 4 * 130 eps of its peak.
    const double bound = 1.5 * 4 * kModes * double(std::numeric_limits<float>::epsilon());
    EXPECT_NOTE(peak > 0 && worst <= bound * peak, std::to_string(worst / peak) + " of the peak, bound " + std::to_string(bound));
}

CASE(hertz_with_bilateral_is_left_out) {
    Rig with, without;
    std::vector<float> approach(kBlock, 1e-3f), out;
    const Coupled got = RunCoupled(with, Contact(1e6f, ModalJunctionHertz | ModalJunctionBilateral), approach.data());
    EXPECT(got.Status == 0 && got.Compliance == 0);
    EXPECT(std::all_of(got.Forces.begin(), got.Forces.end(), [](float v) { return v == 0; }));
    std::vector<float> plain(kBlock, 0.f);
    RenderModalRead(without.Engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), plain.data(), kBlock);
    EXPECT(plain == got.Out);
    EXPECT(SameBank(with.Engine, without.Engine));
}

int main() { return check::run_all(); }
