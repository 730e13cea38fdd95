// The rivers block of a planet: the five results of wo_compute_rivers (rivers.hip), 24 bytes per cell.  wo_river_lines and
// wo_map_color_rivers read it; a second compute call replaces its contents; wo_planet_destroy drops it (rivers_free).
#pragma once
#include <cstdint>

#include "../../include/worogen.h"
#include "device.h"
#include "rivers_ops.h"
#include "stage_block.h"

struct wo_rivers_block : wo::StageBlock {                     // have: bit f is field f (rivers_ops.h: FIELD_*)
    int32_t* receiver = nullptr;                              // r_river_receiver: the final receiver, -1 at roots and off land
    int32_t* basin = nullptr;                                 // r_river_basin: the pit's cell id, -1 drained, -2 not land
    float* lake = nullptr;                                    // r_lake_level
    unsigned long long* discharge = nullptr;                  // r_river_discharge
    float* flow = nullptr;                                    // r_river_flow
    unsigned long long* ctl = nullptr;                        // the call's counters (rivers.hip: CTL_*)
    unsigned long long* h_ctl = nullptr;                      // pinned
    wo_rivers_info info{};
};

namespace wo {
const BlockDesc& rivers_desc();                               // rivers.hip: the block's descriptor
void rivers_free(wo_planet* p);
// rivers.hip: for wo_map_color_rivers, between the region colours and the pixels of map.hip's paint: regionRgba[r] := the river
// tint for every region that is a river cell under minQ or has a lake level; e: the elevation the colours were made of
WO_LOCAL void rivers_tint_regions(wo_planet* p, const float* e, uint64_t minQ, uint32_t* regionRgba);
}  // namespace wo
