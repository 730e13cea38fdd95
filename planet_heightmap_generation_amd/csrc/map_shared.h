// What globe.hip takes from map.hip: the topology check of a mesh's sides, the place of a named layer's values, and the two
// launches whose kernels both exports run (the range of a layer's values, the raw biome colours).  Host code only.
#pragma once
#include <cstdint>
#include <string>

#include "stage_block.h"

namespace wo {

// numSides % 3 == 0 was checked; every corner a region of the planet, every half-edge a side of the mesh
WO_LOCAL bool map_topology_ok(int32_t N, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, std::string& err);

// where a named layer's values live: the block, and the reference's result key of the field (two for the ocean-current layers)
struct LayerSource { const BlockDesc* block; const char *a, *b; const char* hint; };
WO_LOCAL LayerSource layer_source(int32_t layer);

// k_map_range over v into range[0], range[1] (cleared by the caller); k_map_biome_raw; both on the planet's stream under family fam
WO_LOCAL void map_launch_range(wo_planet* p, int fam, const float* v, int32_t N, uint32_t* range);
WO_LOCAL void map_launch_biome_raw(wo_planet* p, int fam, const float* e, const uint8_t* koppen, float* raw, int32_t N);

}  // namespace wo
