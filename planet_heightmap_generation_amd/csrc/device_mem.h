// Ownership of device and pinned host memory.  A DeviceArena is the owner: it allocates, remembers what it allocated and frees all
// of it when it goes away.  Everything else keeps plain T* views (struct members, Fields, kernel arguments), which may be swapped,
// aliased and redirected freely; none of them frees anything.  One arena per planet, one per lazily built block (dropping the block
// drops its memory), one on the stack for the temporaries of a call.  This is the only file that calls the HIP allocator.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace wo {

struct HipError { std::string msg; };

#define WO_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            throw ::wo::HipError{std::string(#call) + " -> " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + \
                                 std::to_string(__LINE__) + ")"};                                      \
    } while (0)

// process-wide: bytes the arenas hold now, allocations they have made so far (wo_memory_in_use)
struct MemoryInUse { std::atomic<int64_t> deviceBytes{0}, pinnedBytes{0}, allocCalls{0}; };
inline MemoryInUse& memory_in_use() { static MemoryInUse m; return m; }

class DeviceArena {
public:
    DeviceArena() = default;
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(const DeviceArena&) = delete;
    DeviceArena(DeviceArena&& o) noexcept { adopt(o); }
    DeviceArena& operator=(DeviceArena&& o) noexcept { if (this != &o) { clear(); adopt(o); } return *this; }
    ~DeviceArena() { clear(); }

    // n elements (at least one) of device / pinned host memory; HipError when there is none
    template <class T> T* dev(size_t n) { return (T*)get(false, bytes_of<T>(n), 0, true); }
    template <class T> T* pinned(size_t n, unsigned flags = 0) { return (T*)get(true, bytes_of<T>(n), flags, true); }
    // the same for the callers that have a fallback: nullptr when there is none
    template <class T> T* try_dev(size_t n) { return (T*)get(false, bytes_of<T>(n), 0, false); }
    template <class T> T* try_pinned(size_t n, unsigned flags = 0) { return (T*)get(true, bytes_of<T>(n), flags, false); }

    // frees one buffer of this arena now and nulls the view (a buffer about to be regrown); nothing to do for nullptr
    template <class T> void release(T*& q) {
        if (!q) return;
        if (!drop(dev_, (void*)q, false) && !drop(pinned_, (void*)q, true)) throw HipError{"DeviceArena::release: not a buffer of this arena"};
        q = nullptr;
    }
    // takes over everything o owns (a group of buffers built in an arena of its own, handed over once it is complete)
    void adopt(DeviceArena& o) {
        dev_.insert(dev_.end(), o.dev_.begin(), o.dev_.end()); o.dev_.clear();
        pinned_.insert(pinned_.end(), o.pinned_.begin(), o.pinned_.end()); o.pinned_.clear();
    }
    void clear() {
        for (auto& b : dev_) { (void)hipFree(b.first); memory_in_use().deviceBytes -= (int64_t)b.second; }
        for (auto& b : pinned_) { (void)hipHostFree(b.first); memory_in_use().pinnedBytes -= (int64_t)b.second; }
        dev_.clear(); pinned_.clear();
    }

private:
    using Block = std::pair<void*, size_t>;               // address, bytes
    std::vector<Block> dev_, pinned_;

    template <class T> static size_t bytes_of(size_t n) { return std::max<size_t>(n, 1) * sizeof(T); }
    void* get(bool pin, size_t bytes, unsigned flags, bool must) {
        void* q = nullptr;
        const hipError_t e = pin ? hipHostMalloc(&q, bytes, flags) : hipMalloc(&q, bytes);
        if (e != hipSuccess) {
            if (must) throw HipError{std::string(pin ? "hipHostMalloc" : "hipMalloc") + " of " + std::to_string(bytes) + " bytes -> " + hipGetErrorString(e)};
            return nullptr;
        }
        (pin ? pinned_ : dev_).push_back({q, bytes});
        (pin ? memory_in_use().pinnedBytes : memory_in_use().deviceBytes) += (int64_t)bytes;
        ++memory_in_use().allocCalls;
        return q;
    }
    static bool drop(std::vector<Block>& v, void* q, bool pin) {
        for (auto it = v.begin(); it != v.end(); ++it) {
            if (it->first != q) continue;
            if (pin) { (void)hipHostFree(q); memory_in_use().pinnedBytes -= (int64_t)it->second; }
            else { (void)hipFree(q); memory_in_use().deviceBytes -= (int64_t)it->second; }
            v.erase(it);
            return true;
        }
        return false;
    }
};

// a host array on the device: allocated in `a`, copied on stream s (nullptr stays nullptr)
template <class T> inline T* up(DeviceArena& a, const T* host, size_t n, hipStream_t s) {
    if (!host) return nullptr;
    T* d = a.dev<T>(n);
    WO_HIP(hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, s));
    return d;
}

}  // namespace wo
