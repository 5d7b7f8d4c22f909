// Junction groups through the mirrored API (ModalJunctionShared / RenderModalCoupled, modal/bank.hpp), included the way a caller of the
// reference includes the bank (<audio/ModalAudio.h>): a star of three junctions on one hub -- to a second body, to a third, to an exciter
// -- is solved as one group; no row pulls, and each obeys f_i = K_i max(u_i - sum_sides read1, 0) against advance-1 pickups on a twin
// bank the rows are replayed into as drives.  Without the flag the second and third junction are left out.  Compiles and links without a
// GPU; runs on one.
#include "harness.hpp"

#include <audio/ModalAudio.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <span>

static_assert(ModalJunctionShared == 4u, "the flag bit of modalhip.h (MH_JUNCTION_SHARED)");

namespace {
constexpr float kRate = 48'000.f;
constexpr uint32_t kBlock = 512, kPoints = 4, kModes = 130, kRingUp = 3, kCoupled = 3, kMembers = 3;

// The synthetic body of the render tests (tests/cpp/modal_junction_test.cpp).
ModalModes LadderModes(uint32_t n_modes, float slowest, float pitch) {
    ModalModes body;
    body.Freqs.resize(n_modes);
    body.T60s.resize(n_modes);
    for (uint32_t k = 0; k < n_modes; ++k) {
        body.Freqs[k] = 40.f * float(k + 1) * pitch;
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

std::vector<float> Scrape(uint32_t blocks, uint32_t seed) {
    std::vector<float> f(size_t(blocks) * kBlock);
    uint32_t lcg = seed;
    for (size_t s = 0; s < f.size(); ++s) {
        lcg = lcg * 1664525u + 1013904223u;
        f[s] = 0.6f * std::sin(float(s) * 0.013f) + 0.4f * (float(lcg >> 8) / float(1u << 24) - 0.5f);
    }
    return f;
}

struct Side {
    uint32_t Object, Point;
    float N[3], Coupling;
};
// member i: side a on the hub (body 0), side b on body i + 1 pushed the opposite way; the third member's other side is an exciter
constexpr Side kSides[kMembers][2] = {{{0, 1, {0.25f, -1.f, 0.5f}, 2.f}, {1, 2, {-0.25f, 1.f, -0.5f}, 2.f}},
                                      {{0, 2, {1.f, 0.5f, -0.25f}, 1.5f}, {2, 3, {-1.f, -0.5f, 0.25f}, 1.5f}},
                                      {{0, 3, {0.5f, 0.5f, -1.f}, 1.f}, {NoModalObject, 0, {0.f, 0.f, 0.f}, 1.f}}};

ModalJunctionSide SideRecord(const Side &s) {
    ModalJunctionSide r;
    r.Object = s.Object, r.Points[0] = r.Points[1] = r.Points[2] = s.Point, r.Nx = s.N[0], r.Ny = s.N[1], r.Nz = s.N[2], r.Coupling = s.Coupling;
    return r;
}
std::vector<ModalJunction> Star(const double *stiffness, uint32_t flags) {
    std::vector<ModalJunction> star(kMembers);
    for (uint32_t i = 0; i < kMembers; ++i) {
        star[i].A = SideRecord(kSides[i][0]);
        if (kSides[i][1].Object != NoModalObject) star[i].B = SideRecord(kSides[i][1]);
        star[i].Stiffness = float(stiffness[i]), star[i].Flags = flags;
    }
    return star;
}

// Three bodies, rung up by drives for kRingUp blocks and then left to themselves.
struct Rig {
    ModalAudio Engine;
    Rig() {
        ModalBank building;
        building.SampleRate = kRate;
        for (uint32_t i = 0; i < 3; ++i) {
            const ModalModes body = LadderModes(kModes, 0.3f, 1.031f + 0.017f * float(i));
            const uint32_t slot = AddModalObject(building, entt::entity{i}, body);
            TuneModalObject(building, slot, body.Freqs, body.T60s);
            building.OutGain[slot] = 1;
        }
        InstallModalBank(Engine, building);
        const std::vector<ModalDrive> drives{{0, 2, 0.5f, -0.25f, 1.f}, {1, 1, 1.f, 0.25f, 0.f}, {2, 0, 0.f, 1.f, 0.5f}};
        std::vector<float> force;
        for (uint32_t d = 0; d < 3; ++d) {
            const std::vector<float> f = Scrape(kRingUp, 4321u + d);
            force.insert(force.end(), f.begin(), f.end());
        }
        std::vector<float> out(kBlock), rows(3 * kBlock);
        for (uint32_t i = 0; i < kRingUp; ++i) {
            for (uint32_t d = 0; d < 3; ++d) std::copy_n(force.begin() + size_t(d) * kRingUp * kBlock + size_t(i) * kBlock, kBlock, rows.begin() + size_t(d) * kBlock);
            RenderModalRead(Engine, drives, rows.data(), {}, static_cast<float *>(nullptr), out.data(), kBlock);
        }
    }
    // One block with the members' rows (nullable: silence) as drives at every side; returns the advance-1 pickups' rows, side by side.
    std::vector<float> Replay(const float *forces) {
        std::vector<ModalDrive> drives;
        std::vector<ModalPickup> pickups;
        std::vector<float> signals;
        for (uint32_t i = 0; i < kMembers; ++i)
            for (const Side &s : kSides[i]) {
                if (s.Object == NoModalObject) continue;
                drives.push_back({s.Object, s.Point, s.N[0], s.N[1], s.N[2]});
                ModalPickup p;
                p.Object = s.Object, p.Points[0] = p.Points[1] = p.Points[2] = s.Point, p.Nx = s.N[0], p.Ny = s.N[1], p.Nz = s.N[2], p.Coupling = s.Coupling, p.Advance = 1;
                pickups.push_back(p);
                if (forces) signals.insert(signals.end(), forces + size_t(i) * kBlock, forces + size_t(i + 1) * kBlock);
                else signals.insert(signals.end(), kBlock, 0.f);
            }
        std::vector<float> reads(pickups.size() * kBlock), out(kBlock);
        std::vector<uint8_t> flags(pickups.size());
        RenderModalRead(Engine, drives, signals.data(), pickups, reads.data(), out.data(), kBlock, flags.data());
        EXPECT(std::all_of(flags.begin(), flags.end(), [](uint8_t f) { return f == 1; }));
        // per member: the sum over its sides
        std::vector<float> per_member(size_t(kMembers) * kBlock, 0.f);
        size_t at = 0;
        for (uint32_t i = 0; i < kMembers; ++i)
            for (const Side &s : kSides[i]) {
                if (s.Object == NoModalObject) continue;
                for (uint32_t t = 0; t < kBlock; ++t) per_member[size_t(i) * kBlock + t] += reads[at * kBlock + t];
                ++at;
            }
        return per_member;
    }
};

struct Coupled {
    std::vector<float> Forces;
    std::vector<double> Compliance;
    std::vector<uint8_t> Status;
};
Coupled RunCoupled(Rig &rig, const std::vector<ModalJunction> &junctions, const float *approach) {
    Coupled r;
    r.Forces.assign(junctions.size() * kBlock, 0.f);
    r.Compliance.assign(junctions.size(), 0.0);
    r.Status.assign(junctions.size(), 0);
    std::vector<float> out(kBlock);
    RenderModalCoupled(rig.Engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), junctions, approach, r.Forces.data(), out.data(), kBlock, nullptr,
                       r.Compliance.data(), r.Status.data());
    return r;
}
} // namespace

CASE(a_star_of_three_never_pulls_and_meets_its_laws_in_a_replay) {
    // the size of the free deflection at each member's sides, and C_ii, from a scout
    Rig scout;
    const std::vector<float> free_read = scout.Replay(nullptr);
    double x0[kMembers] = {};
    for (uint32_t i = 0; i < kMembers; ++i)
        for (uint32_t t = 0; t < kBlock; ++t) x0[i] = std::max(x0[i], std::fabs(double(free_read[size_t(i) * kBlock + t])));
    const double none[kMembers] = {0, 0, 0};
    const std::vector<float> still(size_t(kMembers) * kBlock, 0.f);
    const Coupled probe = RunCoupled(scout, Star(none, ModalJunctionShared), still.data());
    double stiffness[kMembers];
    for (uint32_t i = 0; i < kMembers; ++i) {
        EXPECT(probe.Status[i] == 1 && probe.Compliance[i] > 0 && x0[i] > 0);
        stiffness[i] = 3.0 / probe.Compliance[i]; // K C = 3
    }
    // without the flag the hub carries one junction
    Rig plain;
    const Coupled unshared = RunCoupled(plain, Star(stiffness, 0), still.data());
    EXPECT(unshared.Status[0] == 1 && unshared.Status[1] == 0 && unshared.Status[2] == 0);

    Rig a, b;
    const std::vector<ModalJunction> star = Star(stiffness, ModalJunctionShared);
    std::vector<float> approach(size_t(kMembers) * kBlock);
    size_t pressed[kMembers] = {};
    double worst = 0, peak = 0;
    for (uint32_t blk = 0; blk < kCoupled; ++blk) {
        for (uint32_t i = 0; i < kMembers; ++i)
            for (uint32_t s = 0; s < kBlock; ++s) approach[size_t(i) * kBlock + s] = float(x0[i]) * (std::sin(float(blk * kBlock + s) * 0.016f - 0.5f * float(i)) + 0.1f);
        const Coupled got = RunCoupled(a, star, approach.data());
        const std::vector<float> read1 = b.Replay(got.Forces.data());
        for (uint32_t i = 0; i < kMembers; ++i) {
            EXPECT(got.Status[i] == 1);
            for (uint32_t s = 0; s < kBlock; ++s) {
                const double f = got.Forces[size_t(i) * kBlock + s];
                const double law = double(float(stiffness[i])) * std::max(double(approach[size_t(i) * kBlock + s]) - double(read1[size_t(i) * kBlock + s]), 0.0);
                EXPECT(f >= 0 && std::isfinite(f));
                pressed[i] += f > 0;
                peak = std::max(peak, f);
                worst = std::max(worst, std::fabs(f - law) / (double(float(stiffness[i])) * x0[i]));
            }
        }
    }
    const size_t frames = size_t(kCoupled) * kBlock;
    for (uint32_t i = 0; i < kMembers; ++i) EXPECT_NOTE(pressed[i] > frames / 20 && pressed[i] < frames * 19 / 20, std::to_string(pressed[i]));
    // f_i = K_i (u_i - read1_i): a rounding of the pickups' float sums over a member's sides (2 x 130 terms, at most 260 eps of |u| + |d|
    // <= 4 x0) moves the law by K_i times that; the hub's state on the twin, which adds the three drives' products in another order than
    // the group adds a_i f_i, differs by roundings of the same size.  In units of K_i x0: 2 * 4 * 260 eps.
    const double bound = 2 * 4 * 2 * kModes * double(std::numeric_limits<float>::epsilon());
    EXPECT_NOTE(peak > 0 && worst <= bound, std::to_string(worst) + " of K x0, bound " + std::to_string(bound));
}

int main() { return check::run_all(); }
