// The flood stage of erodeComposite (flood.hip): priorityFloodCarve on the planet's resident field.
#pragma once
#include "device.h"

namespace wo {

// what the flood calls of one erodeComposite did (wo_last_erode_stats)
struct FloodRun { double deviceMs = 0; int64_t rounds = 0, epochs = 0, evals = 0, ties = 0; bool usedDevice = false, fellBack = false; FloodHostStats host; };

// the flood's tables for the planet's current mask
WO_LOCAL void ensure_flood_static(wo_planet* p);
// a share's part in a flood exchange (landmass decomposition); throws when the host's exchange function fails
WO_LOCAL void flood_exchange(wo_planet* p, double carveStrength, FloodHostStats* stats);
// the stage on the whole field in the planet's own order, and on the land heights alone inside the land-first mirror (allowed when
// flood_land_is_mirror_prefix says so)
WO_LOCAL void flood_stage(wo_planet* p, double carveStrength, FloodRun& R);
WO_LOCAL bool flood_land_is_mirror_prefix(wo_planet* p);
WO_LOCAL void flood_stage_land(wo_planet* p, double carveStrength, FloodRun& R);

}  // namespace wo
