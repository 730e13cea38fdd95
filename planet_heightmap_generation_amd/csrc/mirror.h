// The patch-major mirror of a planet's mesh (mirror.hip): the scope a pass enters to run on it.
#pragma once
#include "device.h"

namespace wo {

struct MirrorScope {
    wo_planet* p; bool on = false; float *cur = nullptr, *cur2 = nullptr;
    explicit MirrorScope(wo_planet* pl) : p(pl) {}
    MirrorScope(const MirrorScope&) = delete;
    void point_at_mirror(float* e, float* e2) {
        auto& M = p->mirror;
        p->d_off = M.off; p->d_adj = M.adj; p->d_dist = M.dist; p->d_xyz = M.xyz; p->d_e = e; p->d_e2 = e2; p->d_ocean = M.ocean; p->d_coast = M.coast;
    }
    void point_at_planet() {
        auto& M = p->mirror;
        p->d_off = M.o_off; p->d_adj = M.o_adj; p->d_dist = M.o_dist; p->d_xyz = M.o_xyz; p->d_e = M.o_e; p->d_e2 = M.o_e2; p->d_ocean = M.o_ocean; p->d_coast = M.o_coast;
    }
    // field and ocean mask into the mirror, the planet's pointers onto it
    void enter(const uint8_t* mask = nullptr);
    // the current field back in the planet's own buffer and order, the planet's pointers on its own buffers (flood stage)
    WO_LOCAL void suspend();
    WO_LOCAL void resume();
    void finish() {
        if (!on) return;
        suspend();
        p->mirror.active = on = false;
    }
    ~MirrorScope() { if (on) { point_at_planet(); p->mirror.active = false; } }      // error path: pointers only, the planet's field is what it was at the last suspend
};

// dst[i] = src[cell of mirror id i], all N cells: a per-cell field of the planet into the mirror's order
WO_LOCAL void mirror_gather_f32(wo_planet* p, const float* src, float* dst);
// out[i] = the mirror id of cell in[i]
WO_LOCAL void mirror_map_i32(wo_planet* p, const int32_t* in, int32_t* out, int32_t n);

}  // namespace wo
