// Contact damping through the mirrored API (ModalJunctionDamped / RenderModalDamped, modal/bank.hpp; ContactDamping, modal/contact.hpp),
// included the way a caller of the reference includes the bank (<audio/ModalAudio.h>): the force row of a damped junction never pulls and
// obeys f = K max(y, 0) max(1 + l (y - y_p), 0) against advance-1 pickups on a twin bank the row is replayed into as a drive, with the
// carry handed from block to block; damped together with bilateral is left out; the carry of everything that is not a solved damped
// junction is a NaN, and a call without frames leaves it alone.  The cases whose names begin with host_ need no GPU (`--host` runs them
// alone): the grouping decision of modalhip_groups.hpp, and the damping helper.  Compiles and links without a GPU.
#include "harness.hpp"

#include <audio/ContactModel.h>
#include <audio/ModalAudio.h>
#include <modalhip_groups.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <span>

static_assert(ModalJunctionDamped == 8u && MH_JUNCTION_DAMPED == 8u, "the flag bit of modalhip.h (MH_JUNCTION_DAMPED)");

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

// tests/cpp/modal_hertz_test.cpp's rig: two bodies, body 0 rung up by a drive for kRingUp blocks and then left to itself.
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
    // One block with `force` (nullable) as a drive at the junction's point along its direction; returns the advance-1 pickup's row.
    std::vector<float> Replay(const float *force, std::vector<float> &out) {
        const std::vector<ModalDrive> drives{{0, kPoint, kNormal[0], kNormal[1], kNormal[2]}};
        const std::vector<float> silent(kBlock, 0.f);
        ModalPickup p;
        p.Object = 0, p.Points[0] = p.Points[1] = p.Points[2] = kPoint, p.Nx = kNormal[0], p.Ny = kNormal[1], p.Nz = kNormal[2], p.Coupling = kCoupling, p.Advance = 1;
        const std::vector<ModalPickup> pickups{p};
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

struct Damped {
    std::vector<float> Forces, Out;
    double Compliance{0};
    uint8_t Status{0};
};
Damped RunDamped(Rig &rig, const ModalJunction &junction, const float *approach, float damping, float &carry, uint32_t frames = kBlock) {
    Damped r;
    r.Forces.assign(kBlock, 0.f);
    r.Out.assign(kBlock, 0.f);
    RenderModalDamped(rig.Engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), std::span<const ModalJunction>(&junction, 1), approach,
                      std::span<const float>(&damping, 1), std::span<float>(&carry, 1), r.Forces.data(), r.Out.data(), frames, nullptr, &r.Compliance, &r.Status);
    return r;
}
bool SameBank(ModalAudio &a, ModalAudio &b) {
    SyncModalState(a);
    SyncModalState(b);
    return LiveBank(a).StateRe == LiveBank(b).StateRe && LiveBank(a).StateIm == LiveBank(b).StateIm;
}
constexpr float kNoHistory = std::numeric_limits<float>::quiet_NaN();
} // namespace

CASE(host_the_grouping_keeps_a_damped_junction_alone) {
    const uint32_t shared = MH_JUNCTION_SHARED, damped = MH_JUNCTION_SHARED | MH_JUNCTION_DAMPED;
    { // a damped junction that would join a component is left out; the component stays what it was
        MhJunctionGroups g(4);
        EXPECT(g.add(0, shared, 0, 1, 1, 1) == 0);
        EXPECT(g.add(1, damped, 1, 1, 2, 1) < 0);
        EXPECT(g.add(2, shared, 1, 1, 2, 1) == 0); // (an undamped one joins it still)
        EXPECT(g.components[0].members.size() == 2 && !g.components[0].damped && g.of_object[2] == 0);
    }
    { // a junction that would join a damped junction's component is left out, shared or not, damped or not
        MhJunctionGroups g(4);
        EXPECT(g.add(0, damped, 0, 1, 1, 1) == 0 && g.components[0].damped);
        EXPECT(g.add(1, shared, 1, 1, 2, 1) < 0);
        EXPECT(g.add(2, damped, 2, 1, 0, 1) < 0);
        EXPECT(g.add(3, 0u, 1, 1, MH_NO_OBJECT, 0) < 0);
        EXPECT(g.components[0].members.size() == 1 && g.of_object[2] < 0);
        EXPECT(g.add(4, damped, 2, 1, 3, 1) == 1); // (on other objects a second damped junction is a component of its own)
    }
    { // without the shared flag a damped junction is an ordinary junction: one per object
        MhJunctionGroups g(3);
        EXPECT(g.add(0, MH_JUNCTION_DAMPED, 0, 1, MH_NO_OBJECT, 0) == 0 && g.components[0].damped);
        EXPECT(g.add(1, MH_JUNCTION_DAMPED | MH_JUNCTION_HERTZ, 1, 1, 2, 1) == 1 && g.components[1].damped && g.components[1].hertz);
        EXPECT(g.add(2, MH_JUNCTION_DAMPED, 0, 1, MH_NO_OBJECT, 0) < 0);
    }
}

CASE(host_the_damping_helper_is_hunt_and_crossleys_relation) {
    EXPECT(ContactDamping(0.5, 2.0) == 1.5 * 0.5 / 2.0);
    EXPECT(ContactDamping(1.0, 2.0) == 0.0 && ContactDamping(1.25, 2.0) == 0.0); // a restitution of 1 or more: no damping
    EXPECT(ContactDamping(0.0, 0.25) == 6.0);
}

CASE(a_damped_contact_never_pulls_and_meets_its_law_in_a_replay) {
    Rig scout;
    std::vector<float> out;
    const std::vector<float> free_read = scout.Replay(nullptr, out);
    float x0 = 0;
    for (float v : free_read) x0 = std::max(x0, std::fabs(v));
    EXPECT(x0 > 0);
    const std::vector<float> still(kBlock, 0.f);
    float none = kNoHistory;
    const Damped probe = RunDamped(scout, Contact(0.f, ModalJunctionDamped), still.data(), 0.f, none);
    EXPECT(probe.Status == 1 && probe.Compliance > 0 && std::isfinite(none));
    const float stiffness = float(3.0 / probe.Compliance); // K C = 3
    const float damping = float(ContactDamping(0.5, 0.75 * double(x0) * double(kRate) / 4.0)); // l x0 = 4: D = 4 / (x0 rate), as restitution 0.5 at that speed
    const float per_frame = damping * kRate; // what RenderModalDamped forms: float(D) * float(rate), rounded once
    EXPECT(check::near(double(per_frame) * x0, 4.0, 1e-5));
    const ModalJunction junction = Contact(stiffness, ModalJunctionDamped), elastic = Contact(stiffness, 0);

    Rig a, b, c;
    EXPECT(SameBank(a.Engine, b.Engine));
    size_t pressed = 0, differing = 0;
    std::vector<float> approach(kBlock);
    std::vector<double> y, forces;
    float carry = kNoHistory, unused = kNoHistory;
    for (uint32_t i = 0; i < kCoupled; ++i) {
        for (uint32_t s = 0; s < kBlock; ++s) approach[s] = x0 * (std::sin(float(i * kBlock + s) * 0.016f) + 0.1f);
        const Damped got = RunDamped(a, junction, approach.data(), damping, carry), other = RunDamped(c, elastic, approach.data(), damping, unused);
        EXPECT(got.Status == 1 && other.Status == 1 && std::isfinite(carry) && std::isnan(unused)); // an undamped junction has no carry
        const std::vector<float> read1 = b.Replay(got.Forces.data(), out);
        EXPECT(out == got.Out);
        EXPECT(SameBank(a.Engine, b.Engine));
        for (uint32_t s = 0; s < kBlock; ++s) {
            EXPECT(got.Forces[s] >= 0 && std::isfinite(got.Forces[s]));
            pressed += got.Forces[s] > 0;
            differing += got.Forces[s] != other.Forces[s];
            y.push_back(double(approach[s]) - double(read1[s]));
            forces.push_back(got.Forces[s]);
        }
    }
    double worst = 0, peak = 0;
    for (size_t s = 0; s < y.size(); ++s) {
        const double l = s ? double(per_frame) : 0.0, before = s ? y[s - 1] : 0.0; // the run's first frame has no history
        const double law = double(stiffness) * std::max(y[s], 0.0) * std::max(1.0 + l * (y[s] - before), 0.0);
        worst = std::max(worst, std::fabs(forces[s] - law));
        peak = std::max(peak, forces[s]);
    }
    const size_t frames = size_t(kCoupled) * kBlock;
    EXPECT_NOTE(pressed > frames / 20 && pressed < frames * 19 / 20, std::to_string(pressed));
    EXPECT_NOTE(differing > frames / 20, std::to_string(differing)); // the flag selects another law
    // f = K y m with y = u - read1 and m = 1 + l (y - y_p): a rounding dy of the pickup's 130-term float sum (at most 130 eps of |u| + |d| <=
    // 4 y_max here) moves the law by K (m + 2 l y) dy <= K (m + 2 l x0) dy, m <= 1 + l x0 / 4 per frame of this slow approach: (2 + 10) * 4 * 130 eps
    // of K y_max, and the peak is at least K y_max.
    const double bound = 12.0 * 4 * kModes * double(std::numeric_limits<float>::epsilon());
    EXPECT_NOTE(peak > 0 && worst <= bound * peak, std::to_string(worst / peak) + " of the peak, bound " + std::to_string(bound));
}

CASE(damped_with_bilateral_is_left_out_and_no_frames_leave_the_carry) {
    Rig with, without;
    std::vector<float> approach(kBlock, 1e-3f), out;
    float carry = 0.125f;
    const Damped none = RunDamped(with, Contact(1e6f, ModalJunctionDamped), approach.data(), 1e-3f, carry, 0);
    EXPECT(carry == 0.125f && none.Status == 0); // no frames: nothing is touched
    const Damped got = RunDamped(with, Contact(1e6f, ModalJunctionDamped | ModalJunctionBilateral), approach.data(), 1e-3f, carry);
    EXPECT(got.Status == 0 && got.Compliance == 0 && std::isnan(carry));
    EXPECT(std::all_of(got.Forces.begin(), got.Forces.end(), [](float v) { return v == 0; }));
    std::vector<float> plain(kBlock, 0.f);
    RenderModalRead(without.Engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), plain.data(), kBlock);
    EXPECT(plain == got.Out);
    EXPECT(SameBank(with.Engine, without.Engine));
    for (const float bad : {-1e-3f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()}) { // a damping that is no finite number from 0 up
        carry = 0.125f;
        const Damped out_of_range = RunDamped(with, Contact(1e6f, ModalJunctionDamped), approach.data(), bad, carry);
        plain.assign(kBlock, 0.f); // (a render adds to what the block holds)
        RenderModalRead(without.Engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), plain.data(), kBlock);
        EXPECT_NOTE(out_of_range.Status == 0 && std::isnan(carry), std::to_string(out_of_range.Status) + " " + std::to_string(carry));
        EXPECT(plain == out_of_range.Out);
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--host") == 0) std::erase_if(check::cases(), [](const check::Case &c) { return c.name.rfind("host_", 0) != 0; });
    return check::run_all();
}
