/* query_call.h -- the seam the query entry points share (context_rays.cpp, context_nearest.cpp, context_winding.cpp,
 * context_radiance.cpp, context_bake.cpp, context_probes.cpp): a caller's arrays as the kernel sees them -- device pointers checked, host arrays staged
 * for the length of the call -- the launch between two events, and the refusals every entry point words alike.  What an entry point keeps to itself:
 * its pure refusal, what it asks of the scene, the order of both, and its launch. */
#pragma once
#include "context_internal.h"

namespace tbctx {

/* why a device pointer the caller gave is refused: `bytes` from it must lie inside one allocation of the context's device; null: they do */
inline const char* devicePointerRefusal(const tb_context* c, const void* p, size_t bytes)
{
    hipPointerAttribute_t a; hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipPointerGetAttributes(&a, p) != hipSuccess || hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError(); /* the refusal is ours: the runtime's error does not stay behind */
        return "not a device pointer";
    }
    if (a.type != hipMemoryTypeDevice) return "not device memory";
    if (a.device != c->device) return "memory of another device than the context's";
    if ((size_t)((const uint8_t*)p - (const uint8_t*)base) + bytes > size) return "the array runs past its allocation";
    return nullptr;
}

/* that refusal as every entry point words it, thrown: guarded() answers it with TB_E_INVALID */
inline void checkDevicePointer(const tb_context* c, const char* who, const char* name, const void* p, size_t bytes)
{
    if (const char* why = devicePointerRefusal(c, p, bytes)) throw Refusal{TB_E_INVALID, std::string(who) + ": " + name + ": " + why};
}

/* The arrays of one call.  On the device path (`device`) in() and out() check the caller's pointer and hand it back: nothing is allocated.  On the host
 * path in() hands back a copy on the device and out() a buffer to write into -- `seeded`: a copy of what the caller's array holds, for a kernel that
 * adds to it -- and finish(), after the call's synchronise, copies every out() back.  The buffers go with the object, inside guarded()'s DeviceScope.
 * Arrays are checked and staged in the order of the calls: that order is the entry point's. */
class QueryIo {
public:
    QueryIo(const tb_context* c, const char* who, bool device) : c(c), who(who), device(device) {}
    template <class T> const T* in(const char* name, const T* p, size_t bytes)
    {
        if (device) { checkDevicePointer(c, who, name, p, bytes); return p; }
        return (const T*)(bufs[taken(nullptr)] = staged(p, bytes)).p;
    }
    template <class T> T* out(const char* name, T* p, size_t bytes, bool seeded = false)
    {
        if (device) { checkDevicePointer(c, who, name, p, bytes); return p; }
        return (T*)(bufs[taken(p)] = seeded ? staged(p, bytes) : scratch(bytes)).p;
    }
    void finish() { for (int i = 0; i < used; i++) if (back[i]) copyBack(back[i], bufs[i]); }
private:
    int taken(void* host) { if (used == kMost) throw std::logic_error("QueryIo: more arrays than it holds"); back[used] = host; return used++; }
    static constexpr int kMost = 4; /* tb_sample_probes: three in, one out */
    const tb_context* c; const char* who; bool device;
    DevBuf bufs[kMost]; void* back[kMost] = {}; int used = 0; /* back: where finish() copies to; null for an in() */
};

/* the milliseconds between two recorded events once the stream has been waited for; 0 where the runtime cannot say */
inline float elapsed(hipEvent_t a, hipEvent_t b) { float ms = 0.0f; return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f; }

/* launch() -- it enqueues on `stream` and answers a hipError_t -- between ev[0] and ev[1], waited for, its time in ms.  orZero: a time the runtime
 * cannot give is 0 (the radiance query's way); else it is an error like any other */
template <class Launch> void timed(hipStream_t stream, DevEvent (&ev)[2], float& ms, Launch launch, bool orZero = false)
{
    HIP_TRY(hipEventRecord(ev[0].create(), stream));
    HIP_TRY(launch());
    HIP_TRY(hipEventRecord(ev[1].create(), stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (orZero) ms = elapsed(ev[0], ev[1]);
    else HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
}

/* a query is answered on one device: TB_OK, or the refusal of a group's context with the entry point's own reason behind it.  Where it stands among
 * an entry point's refusals is the entry point's */
inline int refuseGroup(tb_context* c, const char* who, const char* tail)
{
    if (!c || c->group.peers.empty()) return TB_OK;
    return fail(c, TB_E_UNSUPPORTED, std::string(who) + ": not supported for a multi-device group: " + tail);
}

inline tb_output_settings settingsOrDefault(const tb_output_settings* settings)
{
    tb_output_settings s; if (settings) s = *settings; else DefaultOutputSettings(s);
    return s;
}

} // namespace tbctx
