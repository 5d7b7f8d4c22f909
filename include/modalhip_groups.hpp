// Which junctions of a render call are kept, and which of them form a group (modalhip.h, MH_JUNCTION_SHARED): the one definition of the
// decision that RenderBlock (modal/bank.hpp) takes when it packs the caller's junctions and that mh_bank_render_coupled takes again
// before a kernel follows any index.  Host code, header only.
//
// Junctions are offered in call order, after the checks that concern one junction alone (objects, points, numbers, Hertz or damped with
// bilateral, a damping that is not a finite number from 0 up).
// A junction without MH_JUNCTION_SHARED is kept when none of its objects is on a kept junction, and its sides take no more than
// MH_JUNCTION_MODES / 128 waves.  One with the flag may join the kept flagged junctions its objects are on: they and it become one
// component, unless that component would hold more than MH_JUNCTION_GROUP junctions, its distinct objects would take more waves than a
// workgroup holds (each object counted once), or it would hold a Hertz junction or a damped one (MH_JUNCTION_DAMPED) beside another
// junction.  mh_bank_render_mixed alone offers its junctions with hertz_in_groups = true: a Hertz junction then joins a group as a linear one
// does (Component::hertz: the group has a Hertz member and takes step 4m); a damped one still stays alone.  mh_bank_render_damped_groups
// alone offers them with damped_in_groups = true as well: a damped junction then joins too (Component::damped: the group has a damped
// member and takes step 4g).
#ifndef MODALHIP_GROUPS_HPP
#define MODALHIP_GROUPS_HPP
#include "modalhip.h"

#include <algorithm>
#include <cstdint>
#include <vector>

struct MhJunctionGroups {
    struct Component {
        std::vector<uint32_t> members; // the caller's ids of its junctions, ascending; empty: merged into another component
        std::vector<uint32_t> objects; // its distinct objects
        uint32_t waves{0}; // what those objects take, each counted once
        bool shared{false}, hertz{false}, damped{false};
    };
    std::vector<int32_t> of_object; // the component an object is on, -1: none
    std::vector<Component> components;

    explicit MhJunctionGroups(uint32_t n_objects) : of_object(n_objects, -1) {}

    // Offers junction `id` (ids ascend with the call order).  object_b = MH_NO_OBJECT: one-sided.  Returns the component it was kept in, or
    // -1: left out.  hertz_in_groups: mh_bank_render_mixed's decision; damped_in_groups: mh_bank_render_damped_groups's; false: every other
    // entry's.
    int32_t add(uint32_t id, uint32_t flags, uint32_t object_a, uint32_t waves_a, uint32_t object_b, uint32_t waves_b, bool hertz_in_groups = false,
                bool damped_in_groups = false) {
        constexpr uint32_t MOST_WAVES = MH_JUNCTION_MODES / 128;
        const bool two_sided = object_b != MH_NO_OBJECT, shared = (flags & MH_JUNCTION_SHARED) != 0, hertz = (flags & MH_JUNCTION_HERTZ) != 0,
                   damped = (flags & MH_JUNCTION_DAMPED) != 0;
        const int32_t ca = of_object[object_a], cb = two_sided ? of_object[object_b] : -1;
        if (!two_sided) waves_b = 0;
        if (!shared && (ca >= 0 || cb >= 0)) return -1; // one junction per object
        for (const int32_t c : {ca, cb})
            if (c >= 0 && !components[c].shared) return -1; // an object of an unflagged junction is shared with nobody
        const bool both = ca >= 0 && cb >= 0 && ca != cb;
        // the distinct components it would join, each once: ca, then cb where that is another one
        size_t members = 1;
        uint32_t waves = 0;
        bool hertz_inside = false, damped_inside = false;
        for (const int32_t c : {ca, cb == ca ? -1 : cb})
            if (c >= 0) {
                members += components[c].members.size(), waves += components[c].waves;
                hertz_inside = hertz_inside || components[c].hertz, damped_inside = damped_inside || components[c].damped;
            }
        if (ca < 0) waves += waves_a; // an object that is on no component yet brings its own waves
        if (two_sided && cb < 0) waves += waves_b;
        if (members > MH_JUNCTION_GROUP || waves > MOST_WAVES) return -1;
        if (members > 1 && (hertz || hertz_inside) && !hertz_in_groups) return -1; // a Hertz junction in a group: mh_bank_render_mixed only
        if (members > 1 && (damped || damped_inside) && !damped_in_groups) return -1; // a damped one in a group: mh_bank_render_damped_groups only
        int32_t into = ca >= 0 ? ca : cb;
        if (into < 0) {
            into = int32_t(components.size());
            components.emplace_back();
        }
        if (both) { // cb's junctions and objects move over
            Component &from = components[cb];
            for (const uint32_t o : from.objects) of_object[o] = into;
            components[into].members.insert(components[into].members.end(), from.members.begin(), from.members.end());
            components[into].objects.insert(components[into].objects.end(), from.objects.begin(), from.objects.end());
            from = Component{};
        }
        Component &c = components[into];
        for (const uint32_t o : {object_a, object_b})
            if (o != MH_NO_OBJECT && of_object[o] < 0) {
                of_object[o] = into;
                c.objects.push_back(o);
            }
        c.members.push_back(id);
        std::sort(c.members.begin(), c.members.end());
        c.waves = waves;
        c.shared = shared; // (every member of a component has the flag, or it is one unflagged junction)
        c.hertz = hertz || hertz_inside; // (without hertz_in_groups a Hertz junction is only ever a component of its own: the check above)
        c.damped = damped || damped_inside; // (and so is a damped one without damped_in_groups)
        return into;
    }
};
#endif
