// What the result blocks of the climate stages share (wind_block.h, ocean_block.h, precip_block.h, temp.hip): the header with the
// block's memory and its field bits, a descriptor per block, and the one path by which a field is downloaded, uploaded and asked
// for by a later stage.  Host code only.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "device.h"

namespace wo {

struct StageBlock {
    DeviceArena mem;                                          // owns every device and pinned buffer of the block
    uint32_t have = 0;                                        // bit f: field f was set, by the stage's compute call (all of them) or by an upload
};

constexpr uint32_t bit(int f) { return 1u << f; }

// where a field lives and how large it is
struct Slot { void* ptr; size_t bytes; bool host; };

struct BlockDesc {
    const char *noun, *compute;                               // as the messages name the block and its stage: "ocean", "wo_compute_ocean_currents"
    const char* const* keys; int count;                       // the reference's result keys, in field order
    StageBlock* (*get)(const wo_planet*);                     // the planet's block, or nullptr
    void (*alloc)(wo_planet*);                                // builds the block if the planet has none
    Slot (*slot)(StageBlock*, int f, size_t N);
    uint32_t all() const { return (1u << count) - 1u; }
    int index(const char* key) const {
        for (int i = 0; i < count; ++i) if (std::strcmp(key, keys[i]) == 0) return i;
        return -1;
    }
};
// the slot of a block whose fields are out[f], N floats each
template <class Block> Slot out_slot(StageBlock* b, int f, size_t N) { return Slot{static_cast<Block*>(b)->out[f], N * 4, false}; }

// The readiness test of a stage (or of a download, hint == nullptr: any field will do): the planet has the block and every field
// of `needed`.  Sets the error otherwise; `hint` names the uploads that would do instead of the compute call.
inline bool block_require(const wo_planet* p, const char* fn, const BlockDesc& D, uint32_t needed, const char* hint) {
    const StageBlock* B = D.get(p);
    if (B && (hint ? (B->have & needed) == needed : B->have != 0)) return true;
    set_error(std::string(fn) + ": no " + D.noun + " result on this planet (call " + D.compute + " first" + (hint ? std::string(", or ") + hint : std::string()) + ")");
    return false;
}

inline int block_download(wo_planet* p, const char* fn, const BlockDesc& D, const char* field, void* out, int64_t outBytes) {
    if (!check_planet(p, fn)) return 1;
    const std::string F = std::string(fn) + ": ";
    if (!field || !out) { set_error(F + "null pointer"); return 1; }
    if (!block_require(p, fn, D, 0, nullptr)) return 1;
    const int f = D.index(field);
    if (f < 0) { set_error(F + "unknown field '" + field + "'"); return 1; }
    StageBlock* B = D.get(p);
    if (!(B->have & bit(f))) { set_error(F + "no " + D.noun + " result on this planet: " + field + " was never set (call " + D.compute + " first)"); return 1; }
    WO_TRY
        const Slot s = D.slot(B, f, (size_t)p->N);
        if (outBytes < (int64_t)s.bytes) { set_error(F + field + " needs " + std::to_string(s.bytes) + " bytes, out has " + std::to_string(outBytes)); return 1; }
        if (s.host) { std::memcpy(out, s.ptr, s.bytes); return 0; }
        WO_HIP(hipMemcpyAsync(out, s.ptr, s.bytes, hipMemcpyDeviceToHost, p->ctx->stream));
        WO_HIP(hipStreamSynchronize(p->ctx->stream));
        return 0;
    WO_CATCH(fn)
}

// the field is looked up, the block built if absent, then the byte count compared: a refused size leaves an empty block, which
// the planet owns
inline int block_upload(wo_planet* p, const char* fn, const BlockDesc& D, const char* field, const void* data, int64_t bytes) {
    if (!check_planet(p, fn)) return 1;
    const std::string F = std::string(fn) + ": ";
    if (!field || !data) { set_error(F + "null pointer"); return 1; }
    const int f = D.index(field);
    if (f < 0) { set_error(F + "unknown field '" + field + "'"); return 1; }
    WO_TRY
        D.alloc(p);
        StageBlock* B = D.get(p);
        const Slot s = D.slot(B, f, (size_t)p->N);
        if (bytes != (int64_t)s.bytes) { set_error(F + field + " takes " + std::to_string(s.bytes) + " bytes, data has " + std::to_string(bytes)); return 1; }
        if (s.host) std::memcpy(s.ptr, data, s.bytes);
        else {
            WO_HIP(hipMemcpyAsync(s.ptr, data, s.bytes, hipMemcpyHostToDevice, p->ctx->stream));
            WO_HIP(hipStreamSynchronize(p->ctx->stream));     // `data` is the caller's, and pageable
        }
        B->have |= bit(f);
        return 0;
    WO_CATCH(fn)
}

// temp.hip: the temperature block's descriptor (those of the other three are declared beside their blocks)
const BlockDesc& temp_desc();
// wind.hip: the wind block's itczLatsSummer and itczLatsWinter, which lie one after the other, into `dst` (2 x ITCZ_SAMPLES floats
// on the device); the wind block outlives the copy
void stage_itcz(wo_planet* p, float* dst);
// the elevation a stage reads: the caller's, uploaded into the call's arena, or the resident field
inline const float* stage_elevation(wo_planet* p, DeviceArena& T, const float* r_elevation) {
    return r_elevation ? up(T, r_elevation, (size_t)p->N, p->ctx->stream) : p->d_e;
}

}  // namespace wo
