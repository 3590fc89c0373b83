/* context_group.cpp -- multi-device groups (include/tracerboy_hip.h tb_create_multi) and the tile assignment they are made of:
 * which tiles a context owns, the pack of its owned tiles and the un-permute of gathered ones as device entry points. */
#include "context_internal.h"

using namespace tbhost;
using namespace tbctx;

static uint32_t ownedTiles(uint32_t W, uint32_t H, const TbTileMap& t)
{
    uint32_t total = ((W + t.tileW - 1) / t.tileW) * ((H + t.tileH - 1) / t.tileH);
    return total > t.rank ? (total - t.rank + t.world - 1) / t.world : 0;
}

/* multi-device group: hand the owner's built scene to every peer (host arrays copied once per peer, then only the upload runs) */
int tbctx::shareSceneWithPeers(tb_context* c)
{
    for (tb_context* p : c->group.peers) {
        const int rc = guarded(p, [&]() { p->hasScene = false; p->options = c->options; p->scene = c->scene; finalizeScene(p, false); return TB_OK; });
        if (rc != TB_OK) return fail(c, rc, "peer device " + std::to_string(p->device) + ": " + p->err);
    }
    return TB_OK;
}

/* A render of a multi-device group: every device renders the tiles it owns (tile t -> device t % world, 64x64 tiles), then the peers'
 * packed tiles travel to the owner (hipMemcpyPeerAsync on the peer's stream, the owner's stream waits on the peer's event) and one
 * un-permute per surface writes the whole frame into the owner's accumulation surfaces.  Enqueues only; the caller syncs. */
int tbctx::renderGroup(tb_context* c, uint32_t W, uint32_t H, uint32_t n, const tb_output_settings* s, float t)
{
    const uint32_t world = 1u + (uint32_t)c->group.peers.size();
    if (opt<OPT_aov>(c)) return fail(c, TB_E_UNSUPPORTED, "tb_render: AOV targets are not gathered across the devices of a group");
    const std::vector<tb_context*> all = members(c);
    for (uint32_t i = 0; i < world; i++) if (all[i]->tiles.world != world || all[i]->tiles.rank != i) { all[i]->tiles = TbTileMap{i, world, 64, 64};
        resetHistory(all[i]); }
    for (uint32_t i = world; i-- > 0;) { /* the peers first: their launches are in flight while the owner's are enqueued */
        tb_context* x = all[i];
        const int rc = guarded(x, [&]() { x->options = c->options; x->selX = c->selX; x->selY = c->selY; x->rt.lastRender = false; touchAccumulation(x); return renderImpl(x, W,
            H, n, s, t, false); });
        if (rc != TB_OK) return x == c ? rc : fail(c, rc, "peer device " + std::to_string(x->device) + ": " + x->err);
    }
    if (n == 0) return TB_OK;
    /* pixels per device, padded to the largest owner */
    const uint64_t tilesTotal = (uint64_t)((W + 63) / 64) * ((H + 63) / 64), capacity = ((tilesTotal + world - 1) / world) * 64 * 64;
    const size_t bytes = (size_t)capacity * sizeof(TbFloat4);
    return guarded(c, [&]() {
        for (int k = 0; k < 2; k++) ensure(c->group.gathered[k], bytes * world);
        for (uint32_t i = 1; i < world; i++) {
            tb_context* p = all[i];
            HIP_TRY(hipSetDevice(p->device));
            /* the owner's un-permute of the call BEFORE this one reads `gathered`: the copies below must not overtake it (back-to-back
             * tb_render_async calls; a wait on an event never recorded is a no-op) */
            if (c->group.evDone) HIP_TRY(hipStreamWaitEvent(p->stream, c->group.evDone, 0));
            for (int k = 0; k < 2; k++) {
                ensure(p->group.packed[k], bytes);
                const TbFloat4* surface = (const TbFloat4*)(k ? p->jittered.p : p->output.p);
                HIP_TRY(pt_launch_pack_owned(p->stream, surface, (TbFloat4*)p->group.packed[k].p, W, H, &p->tiles, ownedTiles(W, H, p->tiles)));
                HIP_TRY(hipMemcpyPeerAsync((uint8_t*)c->group.gathered[k].p + bytes * i, c->device, p->group.packed[k].p, p->device, bytes, p->stream));
            }
            HIP_TRY(hipEventRecord(p->group.evSent.create(hipEventDisableTiming), p->stream));
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipStreamWaitEvent(c->stream, p->group.evSent, 0));
        }
        HIP_TRY(hipSetDevice(c->device));
        for (int k = 0; k < 2; k++) {
            TbFloat4* surface = (TbFloat4*)(k ? c->jittered.p : c->output.p);
            HIP_TRY(pt_launch_pack_owned(c->stream, surface, (TbFloat4*)c->group.gathered[k].p, W, H, &c->tiles, ownedTiles(W, H, c->tiles)));
            HIP_TRY(pt_launch_unpack_gathered(c->stream, (const TbFloat4*)c->group.gathered[k].p, (size_t)capacity, surface, W, H, world, 64, 64));
        }
        HIP_TRY(hipEventRecord(c->ev1, c->stream)); /* tb_last_render_ms of a group: render + gather + un-permute on the owner's stream */
        HIP_TRY(hipEventRecord(c->group.evDone.create(hipEventDisableTiming), c->stream));
        return TB_OK;
    });
}

extern "C" {

int tb_create_multi(tb_context** out, const int* device_ids, int n_devices)
{
    if (!out) return TB_E_INVALID;
    *out = nullptr;
    if (!device_ids || n_devices < 1) return fail(nullptr, TB_E_INVALID, "tb_create_multi: need at least one device id");
    tb_context* owner = nullptr;
    int rc = tb_create(&owner, device_ids[0]);
    if (rc != TB_OK) return rc;
    for (int i = 1; i < n_devices; i++) {
        tb_context* p = nullptr;
        rc = tb_create(&p, device_ids[i]);
        if (rc != TB_OK) { if (p) tb_destroy(p); tb_destroy(owner); return rc; }
        p->group.owner = owner; owner->group.peers.push_back(p);
        if (device_ids[i] != device_ids[0]) { /* direct peer copies over xGMI where the devices allow it; the copy works (staged) without */
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, device_ids[0], device_ids[i]) == hipSuccess && can) { (void)hipSetDevice(device_ids[0]);
                (void)hipDeviceEnablePeerAccess(device_ids[i], 0); (void)hipGetLastError(); }
            if (hipDeviceCanAccessPeer(&can, device_ids[i], device_ids[0]) == hipSuccess && can) { (void)hipSetDevice(device_ids[i]);
                (void)hipDeviceEnablePeerAccess(device_ids[0], 0); (void)hipGetLastError(); }
        }
    }
    (void)hipSetDevice(device_ids[0]);
    *out = owner;
    return TB_OK;
}

int tb_group_size(tb_context* c) { return c ? 1 + (int)c->group.peers.size() : 0; }

int tb_set_tile_assignment(tb_context* c, uint32_t rank, uint32_t world, uint32_t tw, uint32_t th)
{
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_INVALID, "tb_set_tile_assignment: a multi-device group deals its tiles itself");
    if (!c || world == 0 || rank >= world || tw == 0 || th == 0) return c ? fail(c, TB_E_INVALID, "tb_set_tile_assignment: bad arguments") : TB_E_INVALID;
    if (world > 1 && (tw % 16 || th % 16)) return fail(c, TB_E_INVALID,
        "tb_set_tile_assignment: tile width and height must be multiples of 16 (a workgroup renders 16x16 pixels)");
    c->tiles = TbTileMap{rank, world, tw, th}; resetHistory(c);
    return TB_OK;
}

uint64_t tb_owned_pixels(tb_context* c, uint32_t W, uint32_t H) { return c ? (uint64_t)ownedTiles(W, H, c->tiles) * c->tiles.tileW * c->tiles.tileH : 0; }

static int packOwned(tb_context* c, void* dst, const char* who, bool sync)
{
    return guarded(c, [&]() {
        if (!dst || !c->output.p) return fail(c, TB_E_INVALID, std::string(who) + ": nothing rendered / null destination");
        HIP_TRY(pt_launch_pack_owned(c->stream, (const TbFloat4*)c->output.p, (TbFloat4*)dst, c->width, c->height, &c->tiles, ownedTiles(c->width, c->height,
            c->tiles)));
        if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
        return TB_OK;
    });
}
int tb_pack_owned_device_async(tb_context* c, void* dst) { return packOwned(c, dst, "tb_pack_owned_device_async", false); }
int tb_pack_owned_device(tb_context* c, void* dst) { return packOwned(c, dst, "tb_pack_owned_device", true); } /* ... and the wait */

int tb_unpack_gathered_device(tb_context* c, void* stream, const void* gathered, uint64_t capacityPixels, uint32_t W, uint32_t H, uint32_t world, uint32_t tw,
    uint32_t th, void* full)
{
    return guarded(c, [&]() {
        if (!gathered || !full || world == 0 || tw == 0 || th == 0 || W == 0 || H == 0) return fail(c, TB_E_INVALID, "tb_unpack_gathered_device: bad argument");
        const uint64_t tilesTotal = (uint64_t)((W + tw - 1) / tw) * ((H + th - 1) / th);
        if (((tilesTotal + world - 1) / world) * tw * th > capacityPixels) return fail(c, TB_E_INVALID,
            "tb_unpack_gathered_device: per-rank capacity smaller than rank 0's tiles");
        HIP_TRY(pt_launch_unpack_gathered(stream ? (hipStream_t)stream : c->stream, (const TbFloat4*)gathered, (size_t)capacityPixels, (TbFloat4*)full, W, H,
            world, tw, th));
        return TB_OK;
    });
}

} // extern "C"
