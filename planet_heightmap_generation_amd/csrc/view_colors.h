// The view-colour stage that the map export (map.hip) and the globe mesh (globe.hip) share: the checks of a view request, the place
// of a named layer's values, and the launches that give every region its colour, as an f32 triple or packed through the gamma
// table.  The kernels are in view_colors.hip.  Host code only.
#pragma once
#include <cstdint>
#include <functional>

#include "stage_block.h"

namespace wo {

// what a view colours its regions by; the first two are WO_GLOBE_SOURCE_* of worogen.h
enum : int32_t { VIEW_TYPE = 0, VIEW_LAYER = 1, VIEW_PLATES = 2 };

struct ViewRequest {
    int32_t source = VIEW_TYPE;
    int32_t id = 0;                                           // the map type or the map layer
    bool colors = true;                                       // false: the caller builds no colours, and only the id is checked
    const float* values = nullptr;                            // a layer's values from the caller, or nullptr: the resident field(s)
    const float* r_elevation = nullptr;
    const int32_t* r_plate = nullptr;                         // the plate view's arguments
    int32_t numPlates = 0;
    const int32_t* plateSeeds = nullptr;
    const float* plateColors = nullptr;
};

// a checked request and what it resolved to
struct ViewPlan {
    ViewRequest request;
    const uint8_t* koppen = nullptr;                          // the Koppen classes, for the types that read them
    const BlockDesc* block = nullptr;                         // a layer's resident field(s): the block and its slots
    int fa = -1, fb = -1;
};

// Every check of a request, with fn as the prefix of the message: the id's range and the plate view's table first, then `geometry`
// (the caller's checks of its own arguments, which stand between the two in every entry point), then what the colours need on the
// planet: the Koppen result, the values' rules, the resident fields.  Allocates nothing.
WO_LOCAL bool view_resolve(const char* fn, wo_planet* p, const ViewRequest& request, ViewPlan& plan, const std::function<bool()>& geometry);

// where the colours go: rgb (3 N floats), or rgba (N words) through the gamma table lut; all on the device
struct ViewSink { float* rgb; uint32_t* rgba; const uint8_t* lut; };
// the profiling families of the colour launches and of the range launch
struct ViewFamilies { int colors, range; };

// One colour per region for a resolved request, tinted by the highlight state if one is set: the range launch where the layer is
// coloured over its range, then the colour launch or launches, on the planet's stream.  e: the elevation on the device (read by the
// types and the ocean-current layers).  The temporaries go into T.
WO_LOCAL void view_region_colors(wo_planet* p, DeviceArena& T, const ViewPlan& plan, const float* e, const ViewSink& sink, ViewFamilies families);

// the sides of a mesh as every view takes them: no null pointer, numSides a multiple of 3 in range, every corner a region of the
// planet, every half-edge a side of the mesh
WO_LOCAL bool sides_ok(const char* fn, wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges);

}  // namespace wo
